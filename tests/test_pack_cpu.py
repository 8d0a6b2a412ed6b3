"""Packed outputs on the host (include/mktfhe_pack.h): the packing key against its restatement and against the laws of tests/ref_keys.py,
the definition of the pack on the reference side, the ring shares and their merge, the refusals, and the symbol table.

ZERO-FAILURE CONDITION the GPU test relies on (tests/test_gpu_pack.py, gate outputs packed and opened by shares): a bit sits at +-2^29 and is
decided at a distance of 2^29.  At the shapes packed there (n <= 64, nparty <= 3, gadget (4, 4), N <= 512 rows per pack) ref_pack.predicted
gives a pack error of deviation <= sqrt(96 * 2^32 / 12) = 2^17.5 from rounding and sqrt(20 * 4 * 256 * 2^8 / 12 * 2^14) = 2^16.4 from the key
(CGGI n = 20, 32-bit ring, sigma_ring = 2^7; 2^-14 on the 64-bit ring), on top of a gate output's own noise, which these sets decrypt
through in every other GPU test: the margin is > 2000 deviations of the pack error.
test_definition_opens_every_bit shows the restatement meets it on fresh encryptions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ref_keys as RK
import ref_pack as RP
from helpers import ROOT, mk, secret_keys

from mktfhe_amd import _lib

SETS = {
    "cggi": mk.CGGIparam.scaled(n=5, N=64),
    "cggi_k2": mk.CGGIparam.scaled(n=3, N=64, k=2),
    "lmss": mk.Blockparam.scaled(n=6, N=64, blk_len=3, blk_d=2),
    "ccs": mk.CCS2party.scaled(n=4, N=64),
    "kms": mk.KMS2party.scaled(n=4, N=64),
    "kms3": mk.KMS2party.scaled(n=3, N=64, k=3),
    "kms_block": mk.KMS2partyblock.scaled(n=6, N=64, blk_len=3, blk_d=2),
}
GADGETS = [(1, 16), (4, 4), (8, 4), (3, 5)]


def seed_bytes(n):
    buf = (C.c_uint8 * 32)()
    assert _lib.lib().mkt_client_test_seed(n, buf) == 0
    return bytes(buf)


def zs_of(p, key):
    return [np.asarray(key.ringkey(i), dtype=np.int64) for i in range({mk.CGGI: p.k, mk.LMSS: p.k, mk.CCS: 1}.get(p.scheme, 2))]


def header_symbols(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(mkt_\w+)\s*\(", text))


def test_header_equals_symbol_table_and_all_are_exported():
    assert header_symbols("mktfhe_pack.h") == set(_lib.PACK_SYMBOLS)
    assert not set(_lib.PACK_SYMBOLS) & set(_lib.SYMBOLS)
    for name in _lib.PACK_SYMBOLS:
        assert getattr(_lib.lib(), name) is not None
    assert _lib.lib().mkt_abi_version() == 3


def test_example_calls_only_declared_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "examples", "packed_outputs.c")).read(), flags=re.S)
    called = set(re.findall(r"\b(mkt_\w+)\s*\(", src))
    assert called and called <= header_symbols("mktfhe.h") | header_symbols("mktfhe_pack.h")
    assert {"mkt_load_packing_key", "mkt_pack_batch", "mkt_client_rlwe_partial_decrypt", "mkt_client_rlwe_merge_decrypt"} <= called


@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("sigma", [None, 2.0 ** 55])
def test_keygen_equals_restatement_word_for_word(name, sigma):
    """every word of the host generator, noise included; at sigma = 2^55 every noise word carries the deviate's whole mantissa"""
    p = SETS[name] if sigma is None else SETS[name].scaled(beta=sigma)
    keys = secret_keys(p, seed=31)
    for party in range(p.nparty):
        l, logB = GADGETS[(party + len(name)) % len(GADGETS)]
        got = mk.packing_keygen(keys[party], p, l, logB, deterministic_seed=seed_bytes(900 + party))
        want = RP.packing_key(p, keys[party].lwekey, zs_of(p, keys[party]), party, l, logB, seed_bytes(900 + party), p.beta)
        assert got.shape == want.shape == (p.n, l, 1 + RP.shape(p)[1], p.N)
        assert np.array_equal(got.astype(np.uint64), want), f"{name} party {party} gadget {(l, logB)}"


@pytest.mark.parametrize("name,sigma", [("cggi", None), ("kms", None), ("cggi_k2", None), ("kms", 2.0 ** 55)])
def test_key_rows_open_to_the_law(name, sigma):
    """every row opens to s[q] g_t + e under the ring secrets; e, the masks and their independence held to the laws of tests/ref_keys.py"""
    p = SETS[name].scaled(n=64, N=256)
    if sigma is not None:
        p = p.scaled(beta=sigma)
    l, logB = 4, 4
    key = secret_keys(p, seed=47)[p.nparty - 1]
    pk = mk.packing_keygen(key, p, l, logB, deterministic_seed=seed_bytes(5))
    e, masks = RP.open_key(p, pk, key.lwekey, zs_of(p, key), l, logB)
    assert e.size >= RK.MIN_SHAPE
    assert np.abs(e).max() <= 6 * p.beta + 1
    for stat, pv in RK.noise_stats(e, p.beta).items():
        assert pv >= RK.ALPHA, f"noise {stat}: p = {pv:.3g}"
    for stat, pv in RK.uniform_stats(masks, p.W).items():
        assert pv >= RK.ALPHA, f"masks {stat}: p = {pv:.3g}"
    assert RK.count_equal_rows(masks.reshape(-1, p.N)) == 0
    assert RK.cross_correlation(e[:64]) >= RK.ALPHA
    other = mk.packing_keygen(key, p, l, logB, deterministic_seed=seed_bytes(6))
    assert RK.count_equal_rows(np.concatenate([masks.reshape(-1, p.N), RP.open_key(p, other, key.lwekey, zs_of(p, key), l, logB)[1].reshape(-1, p.N)])) == 0
    fresh = [mk.packing_keygen(key, p, 1, 16) for _ in range(2)]
    assert not np.array_equal(fresh[0], fresh[1]), "a NULL seed must draw fresh entropy per call"


def fresh_rows(p, keys, bits, seed):
    return np.stack([mk.lwe_ith_encrypt(int(b), j % p.nparty, keys[j % p.nparty], p, deterministic_seed=seed + j) for j, b in enumerate(bits)])


@pytest.mark.parametrize("name", ["cggi", "cggi_k2", "lmss", "ccs", "kms", "kms3", "kms_block"])
@pytest.mark.parametrize("exact", [False, True])
def test_definition_opens_every_bit(name, exact):
    """fresh encryptions packed by the restatement open to their bits, coefficient by coefficient; the pack error stays inside the prediction"""
    p = SETS[name]
    keys = secret_keys(p, seed=53)
    l, logB = 4, 4
    pks = [mk.packing_keygen(keys[i], p, l, logB, deterministic_seed=seed_bytes(70 + i)) for i in range(p.nparty)]
    rng = np.random.default_rng(3)
    B = p.N + 5
    bits = rng.integers(0, 2, B).astype(bool)
    rows = fresh_rows(p, keys, bits, 4000)
    ct = RP.pack(p, rows, pks, l, logB, exact=exact)
    assert ct.shape == (2, p.k + 1, p.N)
    zs = RP.ring_keys(p, keys)
    ph = np.concatenate([RP.phase(p, ct[g], zs) for g in range(2)])
    assert np.array_equal(RP.bit_of_phase(p, ph[:B]), bits)
    err = RK.centered((ph[:B] - RP.lwe_phase(p, rows, [k.lwekey for k in keys])).astype(np.uint32), 32)
    key_var, rnd_var = RP.predicted(p, l, logB, p.N, p.beta)
    assert np.abs(err).max() <= 8.6 * np.sqrt(key_var) + p.nparty * p.n * 2.0 ** (32 - l * logB - 1) + 2, "pack error beyond the Gaussian's reach plus the worst rounding"
    assert np.abs(RK.centered(ph[B:], 32)).max() <= 8.6 * np.sqrt(key_var) + 2, "the coefficients of absent rows carry key noise only"
    assert rnd_var > 0
    # the library's harness and shares agree with the restatement, word for word
    for g in range(2):
        assert np.array_equal(mk.rlwe_phase(ct[g].astype(p.ring_dtype), keys, p), RP.phase(p, ct[g], zs))


@pytest.mark.parametrize("name", ["cggi_k2", "ccs", "kms3"])
def test_shares_and_merge(name):
    p = SETS[name]
    keys = secret_keys(p, seed=59)
    rng = np.random.default_rng(9)
    ct = rng.integers(0, 1 << 63, (3, p.k + 1, p.N), dtype=np.uint64) * 2 + rng.integers(0, 2, (3, p.k + 1, p.N), dtype=np.uint64)
    ct = (ct & np.uint64((1 << p.W) - 1)).astype(p.ring_dtype)
    zs = RP.ring_keys(p, keys)
    # sigma_smudge = 0: shares are the plain ring products, the merged phase is rlwe_phase word for word
    sh0 = [mk.rlwe_partial_decrypt(ct, keys[i], p, i, 0.0) for i in range(p.nparty)]
    for i in range(p.nparty):
        for g in range(3):
            assert np.array_equal(sh0[i][g].astype(np.uint64), RP.share(p, ct[g], zs[i], i))
    for g in range(3):
        want = mk.rlwe_phase(ct[g], keys, p)
        assert np.array_equal(want, RP.phase(p, ct[g], zs))
        assert np.array_equal(mk.rlwe_merge_phase(ct[g], [s[g] for s in sh0], p), want)
        assert np.array_equal(mk.rlwe_merge_phase(ct[g], [s[g] for s in sh0], p, count=7), want[:7])
        assert np.array_equal(mk.rlwe_merge_decrypt(ct[g], [s[g] for s in sh0], p), RP.bit_of_phase(p, want))
    # smudged: stream 18, one stream per pack index row0 + g, N words each, lifted to the ring's width
    sd = seed_bytes(77)
    for sigma in (3.0, 2.0 ** 31):
        got = mk.rlwe_partial_decrypt(ct, keys[1 % p.nparty], p, 1 % p.nparty, sigma, deterministic_seed=sd, row0=(1 << 32) - 1)
        for g in range(3):
            want = (RP.share(p, ct[g], zs[1 % p.nparty], 1 % p.nparty) + RP.smudge(p, sd, 1 % p.nparty, (1 << 32) - 1 + g, sigma)) & np.uint64((1 << p.W) - 1)
            assert np.array_equal(got[g].astype(np.uint64), want), f"sigma {sigma} pack {g}"
    a, b = (mk.rlwe_partial_decrypt(ct, keys[0], p, 0, 5.0) for _ in range(2))
    assert not np.array_equal(a, b), "a NULL seed must draw fresh smudging noise per call"


def test_refusals():
    L = _lib.lib()
    p, q = SETS["kms"], SETS["ccs"]
    keys, foreign = secret_keys(p, seed=61), secret_keys(q, seed=61)
    pc = C.byref(p.c())
    out = np.zeros((p.n, 4, 2, p.N), dtype=p.ring_dtype)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    ARG = -1
    for l, logB in [(0, 4), (1, 0), (1, 17), (9, 4), (3, 16), (3, 11), (-1, 4)]:
        assert L.mkt_client_packing_keygen(pc, keys[0].h, 0, l, logB, None, ptr(out)) == ARG, (l, logB)
        with pytest.raises(ValueError):
            mk.packing_keygen(keys[0], p, l, logB)
    assert not out.any(), "a refused call writes nothing"
    assert L.mkt_client_packing_keygen(pc, keys[0].h, 0, 2, 16, None, ptr(out)) == 0
    assert L.mkt_client_packing_keygen(None, keys[0].h, 0, 4, 4, None, ptr(out)) == ARG
    assert L.mkt_client_packing_keygen(pc, None, 0, 4, 4, None, ptr(out)) == ARG
    assert L.mkt_client_packing_keygen(pc, keys[0].h, 0, 4, 4, None, None) == ARG
    assert L.mkt_client_packing_keygen(pc, keys[0].h, 1, 4, 4, None, ptr(out)) == ARG, "wrong-party keys"
    assert L.mkt_client_packing_keygen(pc, keys[0].h, 2, 4, 4, None, ptr(out)) == ARG, "party out of range"
    assert L.mkt_client_packing_keygen(pc, foreign[0].h, 0, 4, 4, None, ptr(out)) == ARG, "foreign keys"
    ct = np.zeros((p.k + 1, p.N), dtype=p.ring_dtype)
    sh = np.full((p.k, p.N), 7, dtype=p.ring_dtype)
    ph = np.full(p.N, 9, dtype=np.uint32)
    bits = np.full(p.N + 1, 9, dtype=np.uint8)
    kp = (C.c_void_p * 2)(keys[0].h, keys[1].h)
    assert L.mkt_client_rlwe_phase(pc, kp, 1, ptr(ct), ptr(ph)) == ARG
    assert L.mkt_client_rlwe_phase(pc, (C.c_void_p * 2)(keys[1].h, keys[0].h), 2, ptr(ct), ptr(ph)) == ARG, "keys out of party order"
    assert L.mkt_client_rlwe_phase(pc, (C.c_void_p * 2)(keys[0].h, foreign[1].h), 2, ptr(ct), ptr(ph)) == ARG
    assert L.mkt_client_rlwe_phase(pc, kp, 2, None, ptr(ph)) == ARG and L.mkt_client_rlwe_phase(pc, kp, 2, ptr(ct), None) == ARG
    for sigma in (-1.0, 2.0 ** 31 + 1, float("nan"), float("inf")):
        assert L.mkt_client_rlwe_partial_decrypt(pc, keys[0].h, 0, ptr(ct), sigma, None, 0, ptr(sh), 1) == ARG
    assert L.mkt_client_rlwe_partial_decrypt(pc, keys[0].h, 1, ptr(ct), 0.0, None, 0, ptr(sh), 1) == ARG
    assert L.mkt_client_rlwe_partial_decrypt(pc, foreign[0].h, 0, ptr(ct), 0.0, None, 0, ptr(sh), 1) == ARG
    assert L.mkt_client_rlwe_partial_decrypt(pc, keys[0].h, 0, None, 0.0, None, 0, ptr(sh), 1) == ARG
    assert L.mkt_client_rlwe_partial_decrypt(pc, keys[0].h, 0, ptr(ct), 0.0, None, 0, None, 1) == ARG
    assert L.mkt_client_rlwe_partial_decrypt(pc, keys[0].h, 0, None, 0.0, None, 0, None, 0) == 0, "G == 0 succeeds"
    assert (sh == 7).all()
    assert L.mkt_client_rlwe_merge_phase(pc, ptr(ct), ptr(sh), 1, p.N, ptr(ph)) == ARG, "share count is the party count"
    assert L.mkt_client_rlwe_merge_phase(pc, ptr(ct), ptr(sh), 2, p.N + 1, ptr(ph)) == ARG, "count > N"
    assert L.mkt_client_rlwe_merge_decrypt(pc, ptr(ct), ptr(sh), 2, p.N + 1, ptr(bits)) == ARG, "count > N"
    assert L.mkt_client_rlwe_merge_phase(pc, None, ptr(sh), 2, 1, ptr(ph)) == ARG and L.mkt_client_rlwe_merge_phase(pc, ptr(ct), None, 2, 1, ptr(ph)) == ARG
    assert L.mkt_client_rlwe_merge_decrypt(pc, ptr(ct), ptr(sh), 2, 1, None) == ARG
    assert (ph == 9).all() and (bits == 9).all()
    assert L.mkt_client_rlwe_merge_phase(pc, ptr(ct), ptr(sh), 2, 0, ptr(ph)) == 0 and (ph == 9).all()
