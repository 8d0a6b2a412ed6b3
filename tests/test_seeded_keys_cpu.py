"""Seeded evaluation keys on the host (include/mktfhe.h "seeded evaluation keys"; mktfhe_amd/csrc/client.cpp): every mask word is the keystream
word the header names (tests/ref_seeded_keys.py, an independent numpy restatement), the expanded keys are ordinary keys that open under the
party's secrets within the laws and thresholds tests/test_keys_cpu.py holds the unseeded generator to, the small keys are those of
mkt_client_party_keygen, and the version-2 key blob carries the compact sections.  No GPU."""
import ctypes as C
import hashlib
import os
import re
import struct

import numpy as np
import pytest

import ref_keys as R
import ref_seeded_keys as RS
import test_keys_cpu as TK
from helpers import ROOT, mk
from mktfhe_amd import _lib

MS = bytes(range(100, 132))                    # a public mask seed
MS2 = bytes(range(7, 39))

# reduced shapes: all five schemes; n in {1, 15, 16, 17, 33} (partial and exact last keystream blocks) and 3 (n + 1 = the padded pitch of the
# resident table); both ring widths; RLWE lengths 1, 2, 3; N in {32, 64, 256}; a block shape with n > N.  (name, parameters, party)
SHAPES = [
    ("cggi-n1", mk.CGGIparam.scaled(n=1, N=32), 0),
    ("cggi-n3", mk.CGGIparam.scaled(n=3, N=256), 0),
    ("cggi-n15-k2", mk.CGGIparam.scaled(n=15, N=64, k=2), 0),
    ("cggi-n33-k3", mk.CGGIparam.scaled(n=33, N=32, k=3), 0),
    ("lmss-n150-k3", mk.Blockparam.scaled(n=150, N=64, k=3, blk_d=50), 0),
    ("lmss-n18", mk.Blockparam.scaled(n=18, N=64, blk_d=6), 0),
    ("ccs-n16", mk.CCS2party.scaled(n=16, N=64), 1),
    ("ccs4-n17", mk.CCS4party.scaled(n=17, N=32), 3),
    ("kms-n17", mk.KMS2party.scaled(n=17, N=32), 1),
    ("kms4-n16", mk.KMS4party.scaled(n=16, N=64), 2),
    ("kmsblock-n18", mk.KMS2partyblock.scaled(n=18, N=64, blk_d=6), 1),
]
# the 64-bit ring under RLWE length 2 (host calls only: no gate path serves it)
HOST_SHAPES = SHAPES + [("cggi-w64-k2", mk.CGGIparam.scaled(n=16, N=32, k=2, W=64, l_gsw=3, logB_gsw=9), 0)]
# the shipped gadgets and noise at reduced n: enough residuals for every statistic of ref_keys (as tests/test_keys_cpu.py SETS)
LAW_SETS = [("CGGI", mk.CGGIparam.scaled(n=16), 0), ("LMSS", mk.Blockparam.scaled(n=18, blk_d=6), 0), ("CCS", mk.CCS2party.scaled(n=20), 1),
            ("KMS", mk.KMS2party.scaled(n=16), 1), ("KMS_block", mk.KMS2partyblock.scaled(n=18, blk_d=6), 0)]
ids = lambda v: v[0]      # noqa: E731


def check(ps, what):
    """the threshold of tests/test_keys_cpu.py (ref_keys.ALPHA), without touching that module's count of its own checks"""
    for name, pv in ps.items():
        assert pv >= R.ALPHA, (what, name, "p = %.3g < %.3g" % (pv, R.ALPHA))


_cache = {}


def seeded_party(p, party, seed=77, mask_seed=MS):
    """(crs, seeded PartyKeys, host-expanded brk, ksk), generated once per shape"""
    key = (p, party, seed, mask_seed)
    if key not in _cache:
        crs = mk.CRS(p, seed) if p.multikey else None
        k = mk.party_keygen_seeded(crs, p, party=party, mask_seed=mask_seed, deterministic_seed=seed)
        brk, ksk = mk.seeded_keys_expand(p, party, k.mask_seed, k.brk_seeded, k.ksk_seeded)
        _cache[key] = (crs, k, brk, ksk)
    return _cache[key]


def open_expanded(p, crs, k, brk, ksk):
    s, z = np.array(k.lwekey), TK._ring_keys(p, k)
    o = {"brk": R.open_ccs_brk(p, brk, crs, s, z[0]) if p.scheme == mk.CCS else R.open_rgsw(p, brk, s, z)}
    o["ksk"] = R.open_ksk(p, ksk, s, z)           # asserts that absent block rows are all zero and live rows are not
    return o


@pytest.mark.parametrize("case", HOST_SHAPES, ids=ids)
def test_every_mask_word_is_the_keystream_word_the_header_names(case):
    """every a polynomial of the bootstrapping key and every mask word of the key-switching key equals the numpy restatement; in
    particular coefficient 0 of every a of the rows c >= 1 IS the public mask word (no secret bit sits in a seeded polynomial); the
    compact sections have the sizes of the formulas and the whole expansion is the restatement's; absent block rows are all zero"""
    _, p, party = case
    crs, k, brk, ksk = seeded_party(p, party)
    assert k.seeded and k.mask_seed == MS and k.brk is None and k.ksk is None
    wb, wk = RS.section_words(p)
    assert k.brk_seeded.size == wb and k.brk_seeded.dtype == p.ring_dtype and k.ksk_seeded.size == wk and k.ksk_seeded.dtype == np.uint32
    assert (wb, wk) == mk.seeded_section_words(p)
    nparty, kr, kk, dr = RS.shape(p)
    want_a = RS.brk_masks(p, MS, party)
    if p.scheme == mk.CCS:
        got = brk.reshape(p.n, 3 * p.l_uni, p.N)
        assert np.array_equal(got[:, p.l_uni + 1::2], want_a)
        assert np.array_equal(got[:, :p.l_uni], k.brk_seeded.reshape(p.n, 2 * p.l_uni, p.N)[:, :p.l_uni])      # the d rows ship whole
    else:
        got = brk.reshape(p.n, kr + 1, p.l_gsw, kr + 1, p.N)
        assert np.array_equal(got[..., 1:, :].reshape(want_a.shape), want_a)
        for c in range(1, kr + 1):
            assert np.array_equal(got[:, c, :, c, 0], want_a.reshape(p.n, kr + 1, p.l_gsw, kr, p.N)[:, c, :, c - 1, 0]), "coefficient 0 of a_{c-1} is not the public mask word"
    K = ksk.reshape(kk, p.N, dr, p.f, p.n + 1)
    live = RS.ksk_live(p)
    assert np.array_equal(K[live][..., :p.n], RS.ksk_masks(p, MS, party)[live])
    assert not K[~live].any() and not k.ksk_seeded.reshape(kk, p.N, dr, p.f)[~live].any()
    rb, rk = RS.expand(p, MS, party, k.brk_seeded, k.ksk_seeded)
    assert np.array_equal(brk, rb) and np.array_equal(ksk, rk)
    # either pair alone gives the same words
    assert np.array_equal(mk.seeded_keys_expand(p, party, MS, brk_seeded=k.brk_seeded)[0], brk)
    assert np.array_equal(mk.seeded_keys_expand(p, party, MS, ksk_seeded=k.ksk_seeded)[1], ksk)


def _shipped_sets():
    return [v for v in vars(mk.params).values() if isinstance(v, mk.Params)]


# every shipped parameter set as it ships, and the scaled shapes of the GPU route test (tests/test_gpu_seeded_keys.py ROUTE_SETS)
SIZE_SETS = _shipped_sets() + [mk.CGGIparam.scaled(n=16), mk.Blockparam.scaled(n=18, blk_d=6), mk.CCS2party.scaled(n=20), mk.KMS2party.scaled(n=16)]


@pytest.mark.parametrize("p", SIZE_SETS, ids=lambda p: f"{p.name}-n{p.n}")
def test_the_stated_sizes_are_those_of_the_host_keys(p):
    """Params.brk_words / ksk_rows / brk_seeded_words -- the one Python statement of a party's key sizes, which Scheme.brk_words,
    Scheme.get_ksk_shape, seeded_section_words, seeded_keys.full_key_words and the key blob read -- against the arrays the host keygen
    returns for the last party: brk, ksk, brk_seeded, ksk_seeded.  The arrays are the reference, not a formula"""
    party = p.nparty - 1
    crs = mk.CRS(p, 3) if p.multikey else None
    full = mk.party_keygen(crs, p, party=party, deterministic_seed=3)
    seeded = mk.party_keygen_seeded(crs, p, party=party, mask_seed=MS, deterministic_seed=3)
    assert (p.brk_words, p.ksk_rows * (p.n + 1)) == (full.brk.size, full.ksk.size)
    assert (p.brk_seeded_words, p.ksk_rows) == (seeded.brk_seeded.size, seeded.ksk_seeded.size)
    assert mk.seeded_section_words(p) == (seeded.brk_seeded.size, seeded.ksk_seeded.size)
    assert mk.seeded_keys.full_key_words(p) == (full.brk.size, (full.ksk.size // (p.n + 1), p.n + 1))
    s = object.__new__(mk.Scheme)               # no context behind it: the two size methods read the parameters only
    s.params, s.h = p, None
    assert s.brk_words() == full.brk.size and int(np.prod(s.get_ksk_shape())) == full.ksk.size and s.get_ksk_shape()[1] == p.n + 1


@pytest.mark.parametrize("case", HOST_SHAPES, ids=ids)
def test_expanded_keys_open_under_the_secrets(case):
    """ref_keys.open_rgsw / open_ccs_brk / open_ksk open the expanded keys unchanged: the phase of a seeded row is the reference's"""
    _, p, party = case
    crs, k, brk, ksk = seeded_party(p, party)
    o = open_expanded(p, crs, k, brk, ksk)
    for c, e in ([("brk d", o["brk"]["e_d"]), ("brk f", o["brk"]["e_f"])] if p.scheme == mk.CCS else [("brk", o["brk"]["e"])]):
        TK.bounded(e, p.beta, (case[0], c))
    TK.bounded(o["ksk"]["e"][o["ksk"]["live"]], p.alpha, (case[0], "ksk"))


@pytest.mark.parametrize("case", LAW_SETS, ids=ids)
def test_expanded_keys_follow_the_laws_of_the_unseeded_generator(case):
    """the residuals of the expanded keys pass every statistic tests/test_keys_cpu.py applies to the unseeded generator, at its thresholds:
    noise per component (pooled and per key-switching level), uniform masks, no mask or noise vector twice, no two noise vectors
    correlated, one uniform ternary r per key bit; and a second mask seed under the same secret seed gives other masks, the same law"""
    name, p, party = case
    crs, k, brk, ksk = seeded_party(p, party, seed=4300)
    o = open_expanded(p, crs, k, brk, ksk)
    comp = {"brk d": o["brk"]["e_d"], "brk f": o["brk"]["e_f"]} if p.scheme == mk.CCS else {"brk": o["brk"]["e"]}
    for c, e in comp.items():
        TK.bounded(e, p.beta, (name, c))
        check(R.noise_stats(e, p.beta), (name, c))
        assert e.size >= TK.POOL
    ksk_e = o["ksk"]["e"][o["ksk"]["live"]]
    TK.bounded(ksk_e, p.alpha, (name, "ksk"))
    check(R.noise_stats(ksk_e.reshape(-1, p.f), p.alpha), (name, "ksk"))
    for t in range(p.f):
        st = R.noise_stats(ksk_e[..., t].ravel(), p.alpha)
        check({q: st[q] for q in ("mean", "variance")}, (name, "ksk level %d" % t))
    masks = o["brk"]["masks"].reshape(-1, p.N)
    check(R.uniform_stats(masks, p.W), (name, "ring masks"))
    lwe_rows = o["ksk"]["masks"][o["ksk"]["live"]].reshape(-1, p.n)
    check(R.uniform_stats(lwe_rows, 32), (name, "LWE masks"))
    assert R.count_equal_rows(masks) == 0 and R.count_equal_rows(lwe_rows) == 0
    noise_rows = np.concatenate(list(comp.values()))
    assert R.count_equal_rows(noise_rows) == 0
    check({"noise rows": R.cross_correlation(noise_rows)}, (name, "cross-correlation"))
    levels = np.moveaxis(ksk_e, -1, 0).reshape(p.f, -1)
    assert R.count_equal_rows(levels) == 0
    check({"ksk levels": R.cross_correlation(levels)}, (name, "cross-correlation"))
    if p.scheme == mk.CCS:
        assert R.count_equal_rows(o["brk"]["r"]) == 0
        check({"ternary r": R.ternary_uniform(o["brk"]["r"])}, (name, "r"))
    # another mask seed, the same secret seed: other masks, residuals under the same law
    _, k2, brk2, ksk2 = seeded_party(p, party, seed=4300, mask_seed=MS2)
    o2 = open_expanded(p, crs, k2, brk2, ksk2)
    both = np.concatenate([masks, o2["brk"]["masks"].reshape(-1, p.N)])
    assert R.count_equal_rows(both) == 0 and (p.W == 32 or R.count_equal_words([masks, o2["brk"]["masks"].reshape(-1, p.N)]) == 0)
    assert R.count_equal_rows(np.concatenate([lwe_rows, o2["ksk"]["masks"][o2["ksk"]["live"]].reshape(-1, p.n)])) == 0
    for c, e in ({"brk d": o2["brk"]["e_d"], "brk f": o2["brk"]["e_f"]} if p.scheme == mk.CCS else {"brk": o2["brk"]["e"]}).items():
        TK.bounded(e, p.beta, (name, c, "second mask seed"))
        check(R.noise_stats(e, p.beta), (name, c, "second mask seed"))
    e2 = o2["ksk"]["e"][o2["ksk"]["live"]]
    TK.bounded(e2, p.alpha, (name, "ksk", "second mask seed"))
    check(R.noise_stats(e2.reshape(-1, p.f), p.alpha), (name, "ksk", "second mask seed"))


@pytest.mark.parametrize("case", SHAPES, ids=ids)
def test_secrets_and_small_keys_are_those_of_the_unseeded_keygen(case):
    """streams 1, 3, 4 are unchanged: secrets, public key and relinearisation key equal mkt_client_party_keygen's with the same seed; the
    noise of the large keys is NOT that of the unseeded form (streams 2 and 5 are not read)"""
    _, p, party = case
    crs, k, brk, ksk = seeded_party(p, party)
    ref = mk.party_keygen(crs, p, party=party, deterministic_seed=77)
    assert np.array_equal(k.lwekey, ref.lwekey)
    for a, b in zip(TK._ring_keys(p, k), TK._ring_keys(p, ref)):
        assert np.array_equal(a, b)
    for name in ("pubkey", "rlk_d", "rlk_f"):
        a, b = getattr(k, name), getattr(ref, name)
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), name
    s, z = np.array(k.lwekey), TK._ring_keys(p, k)
    e_seeded, e_ref = R.open_ksk(p, ksk, s, z), R.open_ksk(p, ref.ksk, s, z)
    live = e_ref["live"]
    if p.n >= 15:
        assert not np.array_equal(e_seeded["e"][live], e_ref["e"][live]), "the two key forms share their key-switching noise"


def test_refusals():
    """MKT_ERR_ARG: a NULL mask seed; a mask seed bytewise equal to the secret seed; a party out of range; a section without its output"""
    p = mk.CGGIparam.scaled(n=4, N=32)
    L, h = _lib.lib(), C.c_void_p()
    seed = (C.c_uint8 * 32)(*MS)
    assert L.mkt_client_party_keygen_seeded(C.byref(p.c()), None, None, 0, None, p.alpha, p.beta, C.byref(h)) == -1
    assert L.mkt_client_party_keygen_seeded(C.byref(p.c()), seed, seed, 0, None, p.alpha, p.beta, C.byref(h)) == -1
    assert L.mkt_client_party_keygen_seeded(C.byref(p.c()), None, seed, 1, None, p.alpha, p.beta, C.byref(h)) == -1 and not h.value
    with pytest.raises(mk.MktError):
        mk.party_keygen_seeded(None, p, mask_seed=MS, deterministic_seed=MS)
    with pytest.raises(ValueError):
        mk.party_keygen_seeded(None, p, mask_seed=b"short")
    k = mk.party_keygen_seeded(None, p, deterministic_seed=5)                        # a fresh mask seed per call
    assert len(k.mask_seed) == 32 and k.mask_seed != mk.party_keygen_seeded(None, p, deterministic_seed=5).mask_seed
    b = np.ascontiguousarray(k.brk_seeded)
    assert L.mkt_client_seeded_keys_expand(C.byref(p.c()), 0, None, b.ctypes.data_as(C.c_void_p), None, b.ctypes.data_as(C.c_void_p), None) == -1
    assert L.mkt_client_seeded_keys_expand(C.byref(p.c()), 0, seed, b.ctypes.data_as(C.c_void_p), None, None, None) == -1
    assert L.mkt_client_seeded_keys_expand(C.byref(p.c()), 1, seed, None, None, None, None) == -1
    with pytest.raises(ValueError):
        mk.seeded_keys_expand(p, 0, MS, brk_seeded=k.brk_seeded[:-1])
    plain = mk.party_keygen(None, p, deterministic_seed=5)
    assert not plain.seeded and plain.mask_seed is None and plain.brk_seeded is None and plain.ksk_seeded is None


def _pack_v1(p, party, sections):
    """format version 1 restated from the module docstring of mktfhe_amd/keyblob.py"""
    head = b"MKTKEY\x00\x01" + struct.pack("<15i", *[getattr(p, f) for f in mk.keyblob._PFIELDS]) + struct.pack("<ii", party, len(sections))
    table = b"".join(struct.pack("<16siiq", n.encode(), a.dtype.itemsize, 0, a.nbytes) for n, a in sections)
    body = head + table
    for _, a in sections:
        body += b"\0" * ((-len(body)) % 16) + a.tobytes()
    return body + hashlib.sha256(body).digest()


def test_key_blob_version_2():
    """a seeded party's blob: format version 2 with mask_seed, brk_seeded, ksk_seeded and the small keys, of exactly the computed length,
    round trip word for word; a version-1 blob is the bytes it always was; truncated blobs and wrong-length sections are refused"""
    p, party = mk.KMS2party.scaled(n=8, N=64), 1
    crs, k, brk, ksk = seeded_party(p, party)
    blob = mk.keyblob.dump_party(k)
    assert blob[:8] == b"MKTKEY\x00\x02"
    wb, wk = RS.section_words(p)
    payload = [32, wb * 8, wk * 4, k.rlk_d.nbytes, k.rlk_f.nbytes, k.pubkey.nbytes]
    size = 76 + 32 * len(payload)
    for nb in payload:
        size += (-size) % 16 + nb
    assert len(blob) == size + 32
    pd, pty, secs = mk.keyblob.load(blob)
    assert pty == party and pd == {f: getattr(p, f) for f in mk.keyblob._PFIELDS} and list(secs) == ["mask_seed", "brk_seeded", "ksk_seeded", "rlk_d", "rlk_f", "pubkey"]
    assert secs["mask_seed"].astype("<u4").tobytes() == MS
    for name in ("brk_seeded", "ksk_seeded", "rlk_d", "rlk_f", "pubkey"):
        assert np.array_equal(secs[name], getattr(k, name)), name
    assert mk.keyblob.dump_seeded_arrays(p, party, MS, k.brk_seeded, k.ksk_seeded, rlk_d=k.rlk_d, rlk_f=k.rlk_f, pubkey=k.pubkey) == blob
    # about a quarter of the full key's blob at this shape
    full = mk.party_keygen(crs, p, party=party, deterministic_seed=77)
    v1 = mk.keyblob.dump_party(full)
    assert v1 == _pack_v1(p, party, [(n, np.ascontiguousarray(getattr(full, n))) for n in ("brk", "ksk", "rlk_d", "rlk_f", "pubkey")])
    assert list(mk.keyblob.load(v1)[2]) == ["brk", "ksk", "rlk_d", "rlk_f", "pubkey"] and len(blob) < 0.6 * len(v1)
    for bad in (blob[:-1], blob[:200] + blob[232:], blob[:-33] + bytes([blob[-33] ^ 1]) + blob[-32:]):
        with pytest.raises(ValueError):
            mk.keyblob.load(bad)
    seed_words = np.frombuffer(MS, dtype="<u4").astype(np.uint32)
    for secs_bad in ([("mask_seed", seed_words[:7]), ("brk_seeded", k.brk_seeded), ("ksk_seeded", k.ksk_seeded)],
                     [("mask_seed", seed_words), ("brk_seeded", k.brk_seeded[:-p.N]), ("ksk_seeded", k.ksk_seeded)],
                     [("mask_seed", seed_words), ("brk_seeded", k.brk_seeded), ("ksk_seeded", np.concatenate([k.ksk_seeded, k.ksk_seeded[:1]]))],
                     [("mask_seed", seed_words), ("brk_seeded", k.brk_seeded.astype(np.uint32)), ("ksk_seeded", k.ksk_seeded)],
                     [("mask_seed", seed_words), ("brk_seeded", k.brk_seeded)],
                     [("mask_seed", seed_words), ("brk_seeded", k.brk_seeded), ("ksk_seeded", k.ksk_seeded), ("ksk", full.ksk)]):
        with pytest.raises(ValueError):
            mk.keyblob.load(mk.keyblob._pack(p, party, secs_bad, mk.keyblob.MAGIC2))


class _Refuses:
    """a scheme whose every upload is an error: load_into must raise before it is reached"""
    def __init__(self, p):
        self.params = p

    def __getattr__(self, name):
        raise AssertionError("upload attempted: " + name)


def test_load_into_refuses_before_any_upload():
    p = mk.KMS2party.scaled(n=8, N=64)
    crs, k, brk, ksk = seeded_party(p, 1)
    bad = mk.keyblob._pack(p, 1, [("mask_seed", np.frombuffer(MS, dtype="<u4").astype(np.uint32)), ("brk_seeded", k.brk_seeded[:-1]), ("ksk_seeded", k.ksk_seeded)], mk.keyblob.MAGIC2)
    with pytest.raises(ValueError):
        mk.keyblob.load_into(_Refuses(p), bad)
    with pytest.raises(ValueError):
        mk.keyblob.load_into(_Refuses(p.scaled(n=9)), mk.keyblob.dump_party(k))


NEW_SYMBOLS = ["mkt_client_party_keygen_seeded", "mkt_client_seeded_keys_expand", "mkt_seeded_keys_expand", "mkt_load_seeded_keys", "mkt_multi_load_seeded_keys"]
NEW_ACCESSORS = ["mkt_client_brk_seeded", "mkt_client_ksk_seeded", "mkt_client_mask_seed"]


def test_header_ctypes_and_package_hold_the_new_names():
    """the header declares the new symbols under "seeded evaluation keys" with the reuse rule in capitals, _lib binds each with the
    header's argument count, the library exports them, the package exports the Python names, and the C example uses only declared symbols"""
    hdr = open(os.path.join(ROOT, "include", "mktfhe.h")).read()
    assert "seeded evaluation keys" in hdr and "A (MASK SEED, PARTY) PAIR SERVES ONE KEY GENERATION" in hdr
    for name in NEW_SYMBOLS + NEW_ACCESSORS:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/mktfhe.h"
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == len(m.group(1).split(",")), name
        assert hasattr(_lib.lib(), name), f"{name} is not exported by the library"
    for name in ("party_keygen_seeded", "seeded_keys_expand", "load_seeded", "seeded_section_words"):
        assert getattr(mk, name) is getattr(mk.seeded_keys, name)
    rng = open(os.path.join(ROOT, "mktfhe_amd", "csrc", "rng_chacha.h")).read()
    for sid, cname in ((12, "STREAM_KSK_MASK"), (13, "STREAM_BRK_MASK"), (14, "STREAM_BRK_NOISE"), (15, "STREAM_KSK_NOISE"), (16, "STREAM_UNI_NOISE")):
        assert re.search(r"constexpr uint32_t %s = %d;" % (cname, sid), rng)
    used = set(re.findall(r"\b(mkt_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "examples", "seeded_keys.c")).read()))
    assert {"mkt_client_party_keygen_seeded", "mkt_load_seeded_keys"} <= used <= set(_lib.SYMBOLS), used - set(_lib.SYMBOLS)
