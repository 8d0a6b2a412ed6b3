"""Flat, versioned key-blob format for evaluation keys.

The reference never serialises keys (every run regenerates them: test/KMS.jl:5-12).  A blob carries ONE
party's evaluation key (or the common reference string) in the integer layouts of include/mktfhe.h, so that
a client -- this package's seeded keygen, or the Julia reference through a 30-line writer -- can hand keys
to an evaluator process.  Secret keys are never written.

  offset  size  field
  0       8     magic  b"MKTKEY\\0\\1"  (last byte = format version: 1, 2 for a party in the seeded key form, 3 for a packing key)
  8       60    mkt_params: 15 little-endian int32 (scheme, n, N, k, W, l_gsw, logB_gsw, l_lev, logB_lev,
                l_uni, logB_uni, f, logD, blk_len, blk_d)
  68      4     party index (int32, -1 for a CRS blob)
  72      4     number of sections S (int32)
  76      S*32  section table: name[16] (ASCII, NUL padded), dtype code int32 (4 = uint32, 8 = uint64),
                reserved int32, byte length int64
  ...           section payloads, each 16-byte aligned, in table order; sections: "crs" | "brk", "ksk",
                "rlk_d", "rlk_f", "pubkey" (those that exist for the scheme)
  end     32    SHA-256 of everything before it

Format version 2 (include/mktfhe.h "seeded evaluation keys") replaces "brk" and "ksk" by "mask_seed" (8 x uint32: the PUBLIC 32-byte mask
seed as little-endian words), "brk_seeded" and "ksk_seeded" (the bodies, compact layouts of the header); the evaluator regenerates the masks
on its GPU.  Everything else is as in version 1, and version-1 blobs are written and read exactly as before.

Format version 3 (include/mktfhe_pack.h) is a PACKING-KEY blob: the same header and section table, and one party's packing key.  Sections:
"pk_gadget" (uint32[2] = l_pk, logB_pk: the gadget is not a field of mkt_params), then either "pk" (the full key, [n][l_pk][1 + kr][N] ring
words) or "pk_mask_seed" (8 x uint32, the PUBLIC mask seed as little-endian words) and "pk_seeded" (the bodies, [n][l_pk][N] ring words).  It
holds no other section.  Versions 1 and 2 are untouched, bytes and behaviour.
"""
import hashlib
import struct

import numpy as np

from .params import Params

MAGIC = b"MKTKEY\x00\x01"
MAGIC2 = b"MKTKEY\x00\x02"       # format version 2: the seeded key form
MAGIC3 = b"MKTKEY\x00\x03"       # format version 3: one party's packing key, full or seeded
_PFIELDS = ("scheme", "n", "N", "k", "W", "l_gsw", "logB_gsw", "l_lev", "logB_lev", "l_uni", "logB_uni", "f", "logD", "blk_len", "blk_d")


def _pack(params: Params, party, sections, magic=MAGIC):
    head = bytearray(magic)
    head += struct.pack("<15i", *[getattr(params, f) for f in _PFIELDS])
    head += struct.pack("<ii", party, len(sections))
    table, payload = bytearray(), bytearray()
    for name, arr in sections:
        a = np.ascontiguousarray(arr)
        assert a.dtype in (np.uint32, np.uint64)
        table += struct.pack("<16siiq", name.encode(), a.dtype.itemsize, 0, a.nbytes)
    base = len(head) + len(table)
    for name, arr in sections:
        pad = (-(base + len(payload))) % 16
        payload += b"\0" * pad + np.ascontiguousarray(arr).tobytes()
    body = bytes(head + table + payload)
    return body + hashlib.sha256(body).digest()


def dump_party(keys) -> bytes:
    """serialise a PartyKeys' EVALUATION key (never the secret key)"""
    p = keys.params
    seeded = getattr(keys, "seeded", False)
    if seeded:
        secs = [("mask_seed", np.frombuffer(keys.mask_seed, dtype="<u4").astype(np.uint32)), ("brk_seeded", keys.brk_seeded), ("ksk_seeded", keys.ksk_seeded)]
    else:
        secs = [("brk", keys.brk), ("ksk", keys.ksk)]
    for name in ("rlk_d", "rlk_f", "pubkey"):
        v = getattr(keys, name)
        if v is not None:
            secs.append((name, v))
    return _pack(p, keys.party, secs, MAGIC2 if seeded else MAGIC)


def dump_seeded_arrays(params: Params, party, mask_seed, brk_seeded, ksk_seeded, rlk_d=None, rlk_f=None, pubkey=None) -> bytes:
    """serialise a seeded party's evaluation key from its arrays (format version 2)"""
    secs = [("mask_seed", np.frombuffer(bytes(mask_seed), dtype="<u4").astype(np.uint32)),
            ("brk_seeded", np.ascontiguousarray(brk_seeded, dtype=params.ring_dtype).reshape(-1)), ("ksk_seeded", np.ascontiguousarray(ksk_seeded, dtype=np.uint32).reshape(-1))]
    for name, v in (("rlk_d", rlk_d), ("rlk_f", rlk_f), ("pubkey", pubkey)):
        if v is not None:
            secs.append((name, np.ascontiguousarray(v, dtype=params.ring_dtype).reshape(-1)))
    return _pack(params, party, secs, MAGIC2)


def dump_arrays(params: Params, party, brk, ksk, rlk_d=None, rlk_f=None, pubkey=None) -> bytes:
    """serialise evaluation-key arrays (e.g. the export of Scheme.keygen_device on the party's own GPU)"""
    secs = [("brk", np.ascontiguousarray(brk, dtype=params.ring_dtype).reshape(-1)), ("ksk", np.ascontiguousarray(ksk, dtype=np.uint32).reshape(-1))]
    for name, v in (("rlk_d", rlk_d), ("rlk_f", rlk_f), ("pubkey", pubkey)):
        if v is not None:
            secs.append((name, np.ascontiguousarray(v, dtype=params.ring_dtype).reshape(-1)))
    return _pack(params, party, secs)


def dump_crs(params: Params, crs) -> bytes:
    return _pack(params, -1, [("crs", np.ascontiguousarray(crs, dtype=params.ring_dtype).reshape(-1))])


def _gadget_section(l, logB):
    l, logB = int(l), int(logB)
    if not (1 <= logB <= 16 and l >= 1 and l * logB <= 32):
        raise ValueError(f"packing gadget (l = {l}, logB = {logB}): 1 <= logB <= 16, 1 <= l, l * logB <= 32")
    return ("pk_gadget", np.array([l, logB], dtype=np.uint32))


def dump_packing_key(params: Params, party, l, logB, pk) -> bytes:
    """serialise one party's packing key (format version 3, the full key)"""
    return _pack(params, party, [_gadget_section(l, logB), ("pk", np.ascontiguousarray(pk, dtype=params.ring_dtype).reshape(-1))], MAGIC3)


def dump_packing_key_seeded(params: Params, party, l, logB, mask_seed, pk_seeded) -> bytes:
    """serialise one party's packing key in the seeded form (format version 3): the public mask seed and the bodies"""
    secs = [_gadget_section(l, logB), ("pk_mask_seed", np.frombuffer(bytes(mask_seed), dtype="<u4").astype(np.uint32)),
            ("pk_seeded", np.ascontiguousarray(pk_seeded, dtype=params.ring_dtype).reshape(-1))]
    return _pack(params, party, secs, MAGIC3)


def load(blob: bytes):
    """-> (params dict, party, {section: ndarray}); raises ValueError on a corrupt or foreign blob"""
    if len(blob) < 76 + 32 or blob[:8] not in (MAGIC, MAGIC2, MAGIC3):
        raise ValueError("not a version-1, version-2 or version-3 MKTKEY blob")
    if hashlib.sha256(blob[:-32]).digest() != blob[-32:]:
        raise ValueError("key blob checksum mismatch")
    pv = struct.unpack_from("<15i", blob, 8)
    party, nsec = struct.unpack_from("<ii", blob, 68)
    off = 76 + 32 * nsec
    out = {}
    for s in range(nsec):
        name, isz, _, nbytes = struct.unpack_from("<16siiq", blob, 76 + 32 * s)
        off += (-off) % 16
        dt = {4: np.uint32, 8: np.uint64}[isz]
        out[name.rstrip(b"\0").decode()] = np.frombuffer(blob, dtype=dt, count=nbytes // isz, offset=off)
        off += nbytes
    pd = dict(zip(_PFIELDS, pv))
    if blob[:8] == MAGIC2:
        _check_seeded(pd, out)
    if blob[:8] == MAGIC3:
        _check_packing(pd, party, out)
    return pd, party, out


def _check_packing(pd, party, secs):
    """a version-3 blob holds pk_gadget and one of the two key shapes, at exactly the lengths its parameters and gadget give, and nothing else"""
    p = Params("blob", alpha=0.0, beta=0.0, **pd)
    if not 0 <= party < p.nparty:
        raise ValueError(f"a version-3 key blob belongs to a party: index {party}")
    g = secs.get("pk_gadget")
    if g is None or g.dtype != np.uint32 or g.size != 2:
        raise ValueError("a version-3 key blob needs the section pk_gadget: uint32[2]")
    l, logB = int(g[0]), int(g[1])
    _gadget_section(l, logB)
    kr = 1 if p.multikey else p.k
    full, seeded = {"pk_gadget", "pk"}, {"pk_gadget", "pk_mask_seed", "pk_seeded"}
    if set(secs) not in (full, seeded):
        raise ValueError(f"a version-3 key blob holds {sorted(full)} or {sorted(seeded)}, not {sorted(secs)}")
    want = (("pk", p.ring_dtype, p.n * l * (1 + kr) * p.N),) if "pk" in secs else (("pk_mask_seed", np.uint32, 8), ("pk_seeded", p.ring_dtype, p.n * l * p.N))
    for name, dt, n in want:
        if secs[name].dtype != dt or secs[name].size != n:
            raise ValueError(f"key blob section {name}: {secs[name].size} words of {secs[name].dtype}, its parameters and gadget need {n} of {np.dtype(dt)}")


def _check_seeded(pd, secs):
    """a version-2 blob holds the three seeded sections at exactly the lengths its parameters give"""
    if {"brk", "ksk"} & set(secs):
        raise ValueError("a version-2 key blob holds the seeded sections, not brk / ksk")
    p = Params("blob", alpha=0.0, beta=0.0, **pd)
    for name, dt, want in (("mask_seed", np.uint32, 8), ("brk_seeded", p.ring_dtype, p.brk_seeded_words), ("ksk_seeded", np.uint32, p.ksk_rows)):
        if name not in secs:
            raise ValueError(f"a version-2 key blob needs the section {name}")
        if secs[name].dtype != dt or secs[name].size != want:
            raise ValueError(f"key blob section {name}: {secs[name].size} words of {secs[name].dtype}, its parameters need {want} of {np.dtype(dt)}")


def load_into(scheme, blob: bytes):
    """upload a blob's keys into a Scheme (params must match the context)"""
    pd, party, secs = load(blob)
    mine = {f: getattr(scheme.params, f) for f in _PFIELDS}
    if pd != mine:
        raise ValueError("key blob was generated for different parameters")
    if blob[:8] == MAGIC3:         # format version 3 (sections and lengths checked by load): one party's packing key
        from .pack import load_packing_key, load_packing_key_seeded      # (the package's own `pack` is the function)
        l, logB = int(secs["pk_gadget"][0]), int(secs["pk_gadget"][1])
        if "pk" in secs:
            load_packing_key(scheme, party, secs["pk"], l, logB)
        else:
            load_packing_key_seeded(scheme, party, secs["pk_mask_seed"].astype("<u4").tobytes(), secs["pk_seeded"], l, logB)
    elif party < 0:
        scheme.load_crs(secs["crs"])
    elif "mask_seed" in secs:      # format version 2 (lengths checked by load): the masks are regenerated on the scheme's GPU
        scheme.load_party(party, mask_seed=secs["mask_seed"].astype("<u4").tobytes(), brk_seeded=secs["brk_seeded"], ksk_seeded=secs["ksk_seeded"],
                          rlk_d=secs.get("rlk_d"), rlk_f=secs.get("rlk_f"), pubkey=secs.get("pubkey"))
    else:
        scheme.load_party(party, brk=secs.get("brk"), ksk=secs.get("ksk"), rlk_d=secs.get("rlk_d"), rlk_f=secs.get("rlk_f"), pubkey=secs.get("pubkey"))
    return party
