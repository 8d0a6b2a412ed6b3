"""The seeded packing key on the host (include/mktfhe_pack.h "SEEDED"; mktfhe_amd/csrc/client.cpp): the generator and the expansion against
the numpy restatement of tests/ref_pack_seeded.py, word for word (tolerance 0: both sides run one ChaCha20 block function and wrapping
integer arithmetic; the one Float64 step is the Gaussian deviate, restated in tests/ref_pack.py); the expanded key against the laws of
tests/ref_keys.py and as the key of a pack; the domain separation of the mask stream; the version-3 key blob; the refusals; the symbol table.
No GPU."""
import ctypes as C
import hashlib
import importlib
import os
import re

import numpy as np
import pytest

import ref_keys as RK
import ref_pack as RP
import ref_pack_seeded as RS
from helpers import ROOT, mk, secret_keys
from test_pack_cpu import GADGETS, SETS, fresh_rows, header_symbols, seed_bytes, zs_of

from mktfhe_amd import _lib

PK = importlib.import_module("mktfhe_amd.pack")      # (mk.pack is the function)

MS = bytes(range(40, 72))                      # a public mask seed
MS2 = bytes(range(3, 35))
NEW_SYMBOLS = ["mkt_client_packing_keygen_seeded", "mkt_client_packing_key_expand", "mkt_packing_key_expand", "mkt_load_packing_key_seeded",
               "mkt_packing_keygen_device"]
ARG = -1


@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("sigma", [None, 2.0 ** 55])
def test_keygen_and_expansion_equal_the_restatement_word_for_word(name, sigma):
    """every word of mkt_client_packing_keygen_seeded, noise included, for every party and every gadget; at sigma = 2^55 every noise word
    carries the deviate's whole mantissa.  Then mkt_client_packing_key_expand: bodies copied, every mask word the keystream word of stream 19"""
    p = SETS[name] if sigma is None else SETS[name].scaled(beta=sigma)
    keys = secret_keys(p, seed=31)
    kr = RP.shape(p)[1]
    for party in range(p.nparty):
        for l, logB in GADGETS:
            seed = seed_bytes(900 + party)
            ms, got = mk.packing_keygen_seeded(keys[party], p, l, logB, mask_seed=MS, deterministic_seed=seed)
            assert ms == MS and got.shape == (p.n, l, p.N) and got.dtype == p.ring_dtype
            want = RS.bodies(p, keys[party].lwekey, zs_of(p, keys[party]), party, l, logB, seed, MS, p.beta)
            assert np.array_equal(got.astype(np.uint64), want), f"{name} party {party} gadget {(l, logB)}"
            full = mk.packing_key_expand(p, party, l, logB, MS, got)
            assert full.shape == (p.n, l, 1 + kr, p.N) and full.dtype == p.ring_dtype
            assert np.array_equal(full[:, :, 1:].astype(np.uint64), RS.masks(p, MS, party, l, logB)), f"{name} party {party} gadget {(l, logB)}: masks"
            assert np.array_equal(full.astype(np.uint64), RS.expand(p, MS, party, l, logB, got))


def test_noise_is_not_that_of_the_unseeded_form_and_fresh_by_default():
    """stream 17 is not read: under one seed the two forms share no noise; a NULL seed draws fresh entropy, a None mask seed a fresh mask seed"""
    p = SETS["kms"]
    key = secret_keys(p, seed=47)[1]
    l, logB = 4, 4
    sd = seed_bytes(5)
    _, b = mk.packing_keygen_seeded(key, p, l, logB, mask_seed=MS, deterministic_seed=sd)
    e_seeded = RP.open_key(p, mk.packing_key_expand(p, 1, l, logB, MS, b), key.lwekey, zs_of(p, key), l, logB)[0]
    e_plain = RP.open_key(p, mk.packing_keygen(key, p, l, logB, deterministic_seed=sd), key.lwekey, zs_of(p, key), l, logB)[0]
    assert RK.count_equal_rows(np.concatenate([e_seeded, e_plain])) == 0
    a, b2 = (mk.packing_keygen_seeded(key, p, 1, 16, mask_seed=MS) for _ in range(2))
    assert not np.array_equal(a[1], b2[1]), "a NULL seed must draw fresh noise per call"
    m1, m2 = (mk.packing_keygen_seeded(key, p, 1, 16)[0] for _ in range(2))
    assert len(m1) == 32 and m1 != m2, "a None mask seed must draw a fresh public seed per call"


@pytest.mark.parametrize("name,sigma", [("cggi", None), ("kms", None), ("cggi_k2", None), ("kms", 2.0 ** 55)])
def test_expanded_key_rows_open_to_the_law(name, sigma):
    """the expanded key is an ordinary packing key: every row opens to s[q] g_t + e under the ring secrets; e, the masks and their independence
    held to the laws of tests/ref_keys.py at n = 64, N = 256, as tests/test_pack_cpu.py holds the unseeded generator"""
    p = SETS[name].scaled(n=64, N=256)
    if sigma is not None:
        p = p.scaled(beta=sigma)
    l, logB = 4, 4
    party = p.nparty - 1
    key = secret_keys(p, seed=47)[party]
    _, body = mk.packing_keygen_seeded(key, p, l, logB, mask_seed=MS, deterministic_seed=seed_bytes(5))
    pk = mk.packing_key_expand(p, party, l, logB, MS, body)
    e, masks = RP.open_key(p, pk, key.lwekey, zs_of(p, key), l, logB)
    assert e.size >= RK.MIN_SHAPE
    assert np.abs(e).max() <= 6 * p.beta + 1
    for stat, pv in RK.noise_stats(e, p.beta).items():
        assert pv >= RK.ALPHA, f"noise {stat}: p = {pv:.3g}"
    for stat, pv in RK.uniform_stats(masks, p.W).items():
        assert pv >= RK.ALPHA, f"masks {stat}: p = {pv:.3g}"
    assert RK.count_equal_rows(masks.reshape(-1, p.N)) == 0
    assert RK.cross_correlation(e[:64]) >= RK.ALPHA
    # another mask seed, the same generation seed: other masks, and the same noise words (stream 20 does not depend on the mask seed)
    _, body2 = mk.packing_keygen_seeded(key, p, l, logB, mask_seed=MS2, deterministic_seed=seed_bytes(5))
    e2, masks2 = RP.open_key(p, mk.packing_key_expand(p, party, l, logB, MS2, body2), key.lwekey, zs_of(p, key), l, logB)
    assert RK.count_equal_rows(np.concatenate([masks.reshape(-1, p.N), masks2.reshape(-1, p.N)])) == 0
    assert np.array_equal(e, e2)


@pytest.mark.parametrize("name", ["cggi", "cggi_k2", "lmss", "ccs", "kms", "kms3", "kms_block"])
@pytest.mark.parametrize("exact", [False, True])
def test_pack_with_expanded_keys_opens_every_bit(name, exact):
    """the inputs and the zero-failure condition of test_pack_cpu.test_definition_opens_every_bit, the keys being expansions of seeded ones.  The
    noise law of a seeded row is the same sigma_ring, so the margin of more than 2000 deviations of the pack error stated at the top of
    tests/test_pack_cpu.py holds unchanged"""
    p = SETS[name]
    keys = secret_keys(p, seed=53)
    l, logB = 4, 4
    pks = []
    for i in range(p.nparty):
        _, body = mk.packing_keygen_seeded(keys[i], p, l, logB, mask_seed=MS, deterministic_seed=seed_bytes(70 + i))
        pks.append(mk.packing_key_expand(p, i, l, logB, MS, body))
    rng = np.random.default_rng(3)
    B = p.N + 5
    bits = rng.integers(0, 2, B).astype(bool)
    rows = fresh_rows(p, keys, bits, 4000)
    ct = RP.pack(p, rows, pks, l, logB, exact=exact)
    zs = RP.ring_keys(p, keys)
    ph = np.concatenate([RP.phase(p, ct[g], zs) for g in range(2)])
    assert np.array_equal(RP.bit_of_phase(p, ph[:B]), bits)
    err = RK.centered((ph[:B] - RP.lwe_phase(p, rows, [k.lwekey for k in keys])).astype(np.uint32), 32)
    key_var, _ = RP.predicted(p, l, logB, p.N, p.beta)
    assert np.abs(err).max() <= 8.6 * np.sqrt(key_var) + p.nparty * p.n * 2.0 ** (32 - l * logB - 1) + 2, "pack error beyond the Gaussian's reach plus the worst rounding"
    assert np.abs(RK.centered(ph[B:], 32)).max() <= 8.6 * np.sqrt(key_var) + 2, "the coefficients of absent rows carry key noise only"


@pytest.mark.parametrize("name", ["kms3", "cggi_k2", "ccs"])
def test_domain_separation_of_the_mask_stream(name):
    """under ONE mask seed the expanded masks of two different gadgets share no polynomial -- also where the two gadgets have rows (q, t) and
    polynomial numbers P in common, as (4, 4) and (4, 5), (8, 4), (3, 5) do -- and neither do those of two parties; with the same seed, party
    and gadget the masks are equal, whatever the bodies"""
    p = SETS[name]
    body = lambda l: np.zeros((p.n, l, p.N), dtype=p.ring_dtype)      # noqa: E731
    m = lambda party, l, logB, seed=MS: mk.packing_key_expand(p, party, l, logB, seed, body(l))[:, :, 1:].reshape(-1, p.N)      # noqa: E731
    base = m(0, 4, 4)
    for l, logB in [(4, 5), (8, 4), (3, 5), (1, 16), (4, 3), (2, 4)]:
        assert RK.count_equal_rows(np.concatenate([base, m(0, l, logB)])) == 0, (l, logB)
    for party in range(1, p.nparty):
        assert RK.count_equal_rows(np.concatenate([base, m(party, 4, 4)])) == 0, party
    assert RK.count_equal_rows(np.concatenate([base, m(0, 4, 4, MS2)])) == 0
    assert np.array_equal(base, m(0, 4, 4))
    ones = np.full((p.n, 4, p.N), 1, dtype=p.ring_dtype)
    assert np.array_equal(base, mk.packing_key_expand(p, 0, 4, 4, MS, ones)[:, :, 1:].reshape(-1, p.N))
    # and none of them is a mask polynomial of the party's seeded bootstrapping key under the same seed (stream 13)
    import ref_seeded_keys as RSK
    brk = RSK.brk_mask_polys(p, MS, 0, np.arange(base.shape[0])).astype(p.ring_dtype)
    assert RK.count_equal_rows(np.concatenate([base, brk])) == 0


# SHA-256 of keyblob.dump_party for the two parties below, computed on the parent commit of the change that added format version 3
PARENT_V1_SHA256 = "3db2c712b742cf6be3cad15eba7a8753f556e39867215080f952944584826a8a"
PARENT_V2_SHA256 = "12a26ee52efa896642110b1f77ad68dece37adb8668b51f24fa216f3a8c225ba"


def test_blobs_of_versions_1_and_2_are_the_bytes_they_were():
    p, party = mk.KMS2party.scaled(n=8, N=64), 1
    crs = mk.CRS(p, 77)
    full = mk.party_keygen(crs, p, party=party, deterministic_seed=77)
    seeded = mk.party_keygen_seeded(crs, p, party=party, mask_seed=bytes(range(100, 132)), deterministic_seed=77)
    v1, v2 = mk.keyblob.dump_party(full), mk.keyblob.dump_party(seeded)
    assert v1[:8] == b"MKTKEY\x00\x01" and hashlib.sha256(v1).hexdigest() == PARENT_V1_SHA256
    assert v2[:8] == b"MKTKEY\x00\x02" and hashlib.sha256(v2).hexdigest() == PARENT_V2_SHA256
    assert list(mk.keyblob.load(v1)[2]) == ["brk", "ksk", "rlk_d", "rlk_f", "pubkey"]
    assert list(mk.keyblob.load(v2)[2]) == ["mask_seed", "brk_seeded", "ksk_seeded", "rlk_d", "rlk_f", "pubkey"]


class _Records:
    """a scheme that records what load_into hands to the library's loaders"""
    def __init__(self, p):
        self.params, self.h, self.calls = p, None, []

    def _ck(self, code):
        return code


@pytest.mark.parametrize("name", ["kms", "cggi_k2"])
def test_key_blob_version_3(name, monkeypatch):
    """both shapes of a packing-key blob round trip word for word at exactly the computed length; a flipped byte fails the checksum; wrong
    section lengths, dtypes, gadgets and a version-3 blob that holds brk are refused; load_into routes each shape to its loader"""
    p = SETS[name]
    party = p.nparty - 1
    key = secret_keys(p, seed=59)[party]
    l, logB = 3, 5
    kr = RP.shape(p)[1]
    _, body = mk.packing_keygen_seeded(key, p, l, logB, mask_seed=MS, deterministic_seed=seed_bytes(1))
    pk = mk.packing_key_expand(p, party, l, logB, MS, body)
    wb = p.W // 8
    for blob, payload, names in ((mk.keyblob.dump_packing_key(p, party, l, logB, pk), [8, pk.size * wb], ["pk_gadget", "pk"]),
                                 (mk.keyblob.dump_packing_key_seeded(p, party, l, logB, MS, body), [8, 32, body.size * wb], ["pk_gadget", "pk_mask_seed", "pk_seeded"])):
        assert blob[:8] == mk.keyblob.MAGIC3 == b"MKTKEY\x00\x03"
        size = 76 + 32 * len(payload)
        for nb in payload:
            size += (-size) % 16 + nb
        assert len(blob) == size + 32
        pd, pty, secs = mk.keyblob.load(blob)
        assert pty == party and pd == {f: getattr(p, f) for f in mk.keyblob._PFIELDS} and list(secs) == names
        assert secs["pk_gadget"].tolist() == [l, logB]
        if "pk" in secs:
            assert np.array_equal(secs["pk"], pk.reshape(-1)) and secs["pk"].dtype == p.ring_dtype
        else:
            assert secs["pk_mask_seed"].astype("<u4").tobytes() == MS and np.array_equal(secs["pk_seeded"], body.reshape(-1))
        for at in (9, 80, len(blob) // 2, len(blob) - 40, len(blob) - 1):
            with pytest.raises(ValueError, match="checksum"):
                mk.keyblob.load(blob[:at] + bytes([blob[at] ^ 1]) + blob[at + 1:])
        with pytest.raises(ValueError):
            mk.keyblob.load(blob[:-1])
    assert body.size * (1 + kr) == pk.size
    g = np.array([l, logB], dtype=np.uint32)
    seed_words = np.frombuffer(MS, dtype="<u4").astype(np.uint32)
    flat, bflat = pk.reshape(-1), body.reshape(-1)
    other = np.uint32 if p.W == 64 else np.uint64
    for bad in ([("pk_gadget", g), ("pk", flat[:-1])],
                [("pk_gadget", g), ("pk", flat.astype(other))],
                [("pk_gadget", g), ("pk", bflat)],
                [("pk_gadget", g[:1]), ("pk", flat)],
                [("pk_gadget", np.array([9, 4], dtype=np.uint32)), ("pk", flat)],
                [("pk", flat)],
                [("pk_gadget", g)],
                [("pk_gadget", g), ("pk_mask_seed", seed_words), ("pk_seeded", bflat[:-p.N])],
                [("pk_gadget", g), ("pk_mask_seed", seed_words[:7]), ("pk_seeded", bflat)],
                [("pk_gadget", g), ("pk_mask_seed", seed_words), ("pk_seeded", flat)],
                [("pk_gadget", g), ("pk_seeded", bflat)],
                [("pk_gadget", g), ("pk_mask_seed", seed_words)],
                [("pk_gadget", g), ("pk", flat), ("pk_mask_seed", seed_words), ("pk_seeded", bflat)],
                [("pk_gadget", g), ("pk", flat), ("brk", flat)],
                [("pk_gadget", g), ("pk_mask_seed", seed_words), ("pk_seeded", bflat), ("ksk", seed_words)]):
        with pytest.raises(ValueError):
            mk.keyblob.load(mk.keyblob._pack(p, party, bad, mk.keyblob.MAGIC3))
    for bad_party in (-1, p.nparty):
        with pytest.raises(ValueError):
            mk.keyblob.load(mk.keyblob._pack(p, bad_party, [("pk_gadget", g), ("pk", flat)], mk.keyblob.MAGIC3))
    with pytest.raises(ValueError):
        mk.keyblob.dump_packing_key(p, party, 9, 4, pk)
    # load_into: each shape reaches its own loader with the blob's words; foreign parameters are refused before any upload
    calls = []
    monkeypatch.setattr(PK, "load_packing_key", lambda s, i, k, ll, lb: calls.append(("full", i, np.array(k), ll, lb)))
    monkeypatch.setattr(PK, "load_packing_key_seeded", lambda s, i, m, k, ll, lb: calls.append(("seeded", i, m, np.array(k), ll, lb)))
    s = _Records(p)
    assert mk.keyblob.load_into(s, mk.keyblob.dump_packing_key(p, party, l, logB, pk)) == party
    assert mk.keyblob.load_into(s, mk.keyblob.dump_packing_key_seeded(p, party, l, logB, MS, body)) == party
    assert [c[0] for c in calls] == ["full", "seeded"]
    assert calls[0][1] == party and np.array_equal(calls[0][2], flat) and calls[0][3:] == (l, logB)
    assert calls[1][1] == party and calls[1][2] == MS and np.array_equal(calls[1][3], bflat) and calls[1][4:] == (l, logB)
    with pytest.raises(ValueError):
        mk.keyblob.load_into(_Records(p.scaled(n=p.n + 1)), mk.keyblob.dump_packing_key(p, party, l, logB, pk))
    assert len(calls) == 2


def test_refusals_of_the_host_calls():
    """every refusal is MKT_ERR_ARG and writes nothing: the output is pre-filled and compared after"""
    L = _lib.lib()
    p, q = SETS["kms"], SETS["ccs"]
    keys, foreign = secret_keys(p, seed=61), secret_keys(q, seed=61)
    pc = C.byref(p.c())
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    u8 = lambda b: (C.c_uint8 * 32)(*b)      # noqa: E731
    ms, sd = u8(MS), u8(seed_bytes(8))
    out = np.full((p.n, 8, p.N), 0xA5A5A5A5, dtype=p.ring_dtype)
    gen = L.mkt_client_packing_keygen_seeded
    for l, logB in [(0, 4), (1, 0), (1, 17), (9, 4), (3, 16), (3, 11), (-1, 4)]:
        assert gen(pc, keys[0].h, 0, l, logB, sd, ms, ptr(out)) == ARG, (l, logB)
        with pytest.raises(ValueError):
            mk.packing_keygen_seeded(keys[0], p, l, logB, mask_seed=MS)
    assert gen(pc, keys[0].h, 0, 4, 4, sd, None, ptr(out)) == ARG, "mask_seed NULL"
    assert gen(pc, keys[0].h, 0, 4, 4, ms, ms, ptr(out)) == ARG, "seed bytewise equal to mask_seed"
    assert gen(pc, keys[0].h, 0, 4, 4, u8(MS), ms, ptr(out)) == ARG, "seed bytewise equal to mask_seed (another buffer)"
    assert gen(None, keys[0].h, 0, 4, 4, sd, ms, ptr(out)) == ARG
    assert gen(pc, None, 0, 4, 4, sd, ms, ptr(out)) == ARG
    assert gen(pc, keys[0].h, 0, 4, 4, sd, ms, None) == ARG
    assert gen(pc, keys[0].h, 1, 4, 4, sd, ms, ptr(out)) == ARG, "wrong-party keys"
    assert gen(pc, keys[0].h, 2, 4, 4, sd, ms, ptr(out)) == ARG, "party out of range"
    assert gen(pc, keys[0].h, -1, 4, 4, sd, ms, ptr(out)) == ARG, "party out of range"
    assert gen(pc, foreign[0].h, 0, 4, 4, sd, ms, ptr(out)) == ARG, "foreign keys"
    assert (out == 0xA5A5A5A5).all(), "a refused call writes nothing"
    with pytest.raises(mk.MktError):
        mk.packing_keygen_seeded(keys[0], p, 4, 4, mask_seed=MS, deterministic_seed=MS)
    with pytest.raises(ValueError):
        mk.packing_keygen_seeded(keys[0], p, 4, 4, mask_seed=b"short")
    assert gen(pc, keys[0].h, 0, 8, 4, sd, ms, ptr(out)) == 0 and not (out == 0xA5A5A5A5).all()
    assert gen(pc, keys[0].h, 0, 8, 4, None, ms, ptr(out)) == 0, "seed NULL draws fresh entropy"
    body = np.ascontiguousarray(out[:, :4])
    full = np.full((p.n, 4, 2, p.N), 0x5A5A5A5A, dtype=p.ring_dtype)
    exp = L.mkt_client_packing_key_expand
    for l, logB in [(0, 4), (1, 0), (1, 17), (9, 4), (3, 11)]:
        assert exp(pc, 0, l, logB, ms, ptr(body), ptr(full)) == ARG, (l, logB)
    assert exp(pc, 0, 4, 4, None, ptr(body), ptr(full)) == ARG, "mask_seed NULL"
    assert exp(None, 0, 4, 4, ms, ptr(body), ptr(full)) == ARG
    assert exp(pc, 0, 4, 4, ms, None, ptr(full)) == ARG
    assert exp(pc, 0, 4, 4, ms, ptr(body), None) == ARG
    assert exp(pc, 2, 4, 4, ms, ptr(body), ptr(full)) == ARG and exp(pc, -1, 4, 4, ms, ptr(body), ptr(full)) == ARG, "party out of range"
    assert (full == 0x5A5A5A5A).all(), "a refused call writes nothing"
    assert exp(pc, 1, 4, 4, ms, ptr(body), ptr(full)) == 0, "expansion needs no key: any party index of the scheme"
    with pytest.raises(ValueError):
        mk.packing_key_expand(p, 0, 4, 4, MS, body.reshape(-1)[:-1])
    with pytest.raises(ValueError):
        mk.packing_key_expand(p, 0, 4, 4, b"short", body)


def test_header_symbol_table_and_package_hold_the_new_names():
    """every new name is declared in mktfhe_pack.h with the argument count _lib binds, is in PACK_SYMBOLS and exported; the header states the
    two streams, the reuse rule in capitals and the trust paragraph; NOT HERE no longer lists what now exists; the ABI version is 3"""
    hdr = open(os.path.join(ROOT, "include", "mktfhe_pack.h")).read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/mktfhe_pack.h"
        assert name in _lib.PACK_SYMBOLS and len(_lib.PACK_SYMBOLS[name][1]) == len(m.group(1).split(",")), name
        assert hasattr(_lib.lib(), name), f"{name} is not exported by the library"
    assert header_symbols("mktfhe_pack.h") == set(_lib.PACK_SYMBOLS)
    assert _lib.lib().mkt_abi_version() == 3
    assert "A (MASK SEED, PARTY) PAIR SERVES ONE PACKING-KEY GENERATION PER GADGET" in hdr
    assert "STREAM_PACK_MASK" in hdr and "STREAM_PACK_NOISE" in hdr and "mkt_keygen_device_seeded" in hdr
    not_here = hdr[hdr.index("NOT HERE"):hdr.index("*/", hdr.index("NOT HERE"))]
    assert "mkt_multi_" in not_here and "seeded" not in not_here and "blob" not in not_here and "party's GPU" not in not_here
    rng = open(os.path.join(ROOT, "mktfhe_amd", "csrc", "rng_chacha.h")).read()
    for sid, cname in ((17, "STREAM_PACK_KEY"), (18, "STREAM_PACK_SMUDGE"), (19, "STREAM_PACK_MASK"), (20, "STREAM_PACK_NOISE")):
        assert re.search(r"constexpr uint32_t %s = %d;" % (cname, sid), rng)
    for name in ("packing_keygen_seeded", "packing_key_expand", "load_packing_key_seeded", "packing_keygen_device"):
        assert getattr(mk, name) is getattr(PK, name)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "examples", "seeded_packing_key.c")).read(), flags=re.S)
    called = set(re.findall(r"\b(mkt_\w+)\s*\(", src))
    assert called <= header_symbols("mktfhe.h") | header_symbols("mktfhe_pack.h")
    assert {"mkt_packing_keygen_device", "mkt_load_packing_key_seeded", "mkt_pack_batch", "mkt_client_rlwe_partial_decrypt", "mkt_client_rlwe_merge_decrypt"} <= called
