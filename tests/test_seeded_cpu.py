"""Seeded ciphertexts on the host (include/mktfhe.h "seeded ciphertexts"; mktfhe_amd/seeded.py): mkt_client_seeded_expand and
mkt_client_seeded_encrypt, which are the definition the device kernels are held to (tests/test_gpu_seeded.py), against the numpy
restatement tests/ref_seeded.py -- itself pinned to RFC 8439's test vector first."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ref_seeded as RS
from helpers import ROOT, mk, party_set as _set, secret_keys as secrets
from mktfhe_amd import _lib, scheme as S

MASK_SEED = bytes(range(100, 132))
ROW0S = (0, 2**32 - 3)          # the second: the row index carries into the high nonce word inside a batch of 4 or more rows


def centered(w):
    return w.astype(np.int64) - ((w.astype(np.int64) >> 31) << 32)


def test_the_restatement_is_rfc8439():
    """RFC 8439 2.3.2: key 00 .. 1f, block counter 1, nonce 00 00 00 09 00 00 00 4a 00 00 00 00"""
    key = RS.seed_key(bytes(range(32)))
    nonce = [int(w) for w in np.frombuffer(bytes.fromhex("000000090000004a00000000"), dtype="<u4")]
    want = [0xe4e7f110, 0x15593bd1, 0x1fdd0f50, 0xc47120a3, 0xc7f4d1c7, 0x0368c033, 0x9aaa2204, 0x4e6cd4c3,
            0x466482d2, 0x09aa9f07, 0x05d7c214, 0xa2028bd9, 0xd19c12b5, 0xb94e16de, 0xe883d0cb, 0x4e3c50a2]
    assert RS.chacha20_block(key, 1, nonce)[0].tolist() == want
    assert RS.chacha20_block(key, [0, 1, 2], nonce)[1].tolist() == want


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_host_expand_is_the_restatement(n):
    """n below, at and past one keystream block, and three blocks; nparty 1 .. 3, the first and the last party; both row0; every word
    outside block i and the body is zero (the restatement's rows are built on zeros, and that is asserted on the library's rows too)"""
    rng = np.random.default_rng(n)
    for nparty in (1, 2, 3):
        p = _set(n, nparty)
        for party in sorted({0, nparty - 1}):
            for row0 in ROW0S:
                body = rng.integers(0, 2**32, 7, dtype=np.uint64).astype(np.uint32)
                got = mk.seeded_expand(mk.SeededBatch(party, MASK_SEED, row0, body), p)
                assert got.shape == (7, p.lwe_len) and got.dtype == np.uint32
                assert np.array_equal(got, RS.expand(MASK_SEED, party, row0, body, n, nparty)), (nparty, party, row0)
                rest = np.delete(got, np.r_[party * n:(party + 1) * n, p.lwe_len - 1], axis=1)
                assert not rest.any() and np.array_equal(got[:, -1], body)
                assert len({tuple(r) for r in got[:, party * n:(party + 1) * n]}) == 7 or n == 1, "rows share a mask"


def test_the_body_is_the_formula():
    """sigma = 0: body == mu - <a, s> with the restatement's mask; same seeds and two message vectors: the bodies differ by exactly
    mu1 - mu2, noise included"""
    p = mk.KMS2party.scaled(n=33, N=256)
    keys = secrets(p)
    rng = np.random.default_rng(1)
    mu1, mu2 = (rng.integers(0, 2**32, 9, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    for party in (0, 1):
        for row0 in ROW0S:
            b0 = mk.seeded_encrypt(mu1, keys[party], p.scaled(alpha=0.0), party, words=True, mask_seed=MASK_SEED, row0=row0)
            assert (b0.party, b0.mask_seed, b0.row0) == (party, MASK_SEED, row0)
            want = [RS.body_word(RS.mask_row(MASK_SEED, party, row0 + j, p.n), keys[party].lwekey, mu1[j]) for j in range(9)]
            assert b0.body.tolist() == want, (party, row0)
            a, b = (mk.seeded_encrypt(m, keys[party], p, party, words=True, mask_seed=MASK_SEED, deterministic_seed=5, row0=row0).body for m in (mu1, mu2))
            assert np.array_equal(a - b, mu1 - mu2) and not np.array_equal(a, b0.body)


@pytest.mark.parametrize("p", [_set(20, 1), _set(16, 2), _set(5, 3)], ids=lambda p: f"{p.name}-n{p.n}-k{p.k}")
def test_phase_of_the_expansion_is_the_message_at_sigma_zero(p):
    keys = secrets(p)
    mu = np.random.default_rng(2).integers(0, 2**32, 64, dtype=np.uint64).astype(np.uint32)
    for party in range(p.nparty):
        batch = mk.seeded_encrypt(mu, keys[party], p.scaled(alpha=0.0), party, words=True, mask_seed=MASK_SEED, row0=2**32 - 3)
        assert np.array_equal(mk.lwe_phase(mk.seeded_expand(batch, p), keys if p.multikey else keys[0], p), mu), party


def test_the_noise_has_the_deviation_asked_for():
    """sigma = params.alpha over B = 4096 rows: phase - mu (signed) is not all zero and its sample standard deviation is within 5.5 % of
    sigma: five standard errors of a deviation estimated from 4096 draws, 5 / sqrt(2 * 4095) = 5.53 %, rounded down"""
    p = mk.KMS2party.scaled(n=16, N=256)
    keys = secrets(p)
    B = 4096
    mu = np.random.default_rng(3).integers(0, 2**32, B, dtype=np.uint64).astype(np.uint32)
    batch = mk.seeded_encrypt(mu, keys[1], p, 1, words=True, deterministic_seed=8)
    e = centered(mk.lwe_phase(mk.seeded_expand(batch, p), keys, p) - mu)
    assert e.any()
    assert abs(e.std(ddof=1) / p.alpha - 1) < 0.055, e.std(ddof=1) / p.alpha


def test_a_batch_in_pieces_is_the_batch():
    """10 rows at row0 = 0 == 4 rows at row0 = 0 then 6 rows at row0 = 4, bodies and expanded rows"""
    p = mk.KMS2party.scaled(n=17, N=256)
    keys = secrets(p)
    mu = np.random.default_rng(4).integers(0, 2**32, 10, dtype=np.uint64).astype(np.uint32)
    kw = dict(words=True, mask_seed=MASK_SEED, deterministic_seed=6)
    whole = mk.seeded_encrypt(mu, keys[0], p, 0, **kw)
    head, tail = mk.seeded_encrypt(mu[:4], keys[0], p, 0, **kw), mk.seeded_encrypt(mu[4:], keys[0], p, 0, row0=4, **kw)
    assert np.array_equal(np.concatenate([head.body, tail.body]), whole.body)
    assert np.array_equal(np.concatenate([mk.seeded_expand(head, p), mk.seeded_expand(tail, p)]), mk.seeded_expand(whole, p))


@pytest.mark.parametrize("p", [mk.CGGIparam.scaled(n=16, N=256), mk.KMS2party.scaled(n=16, N=256)], ids=lambda p: p.name)
def test_bits_decrypt(p):
    """bits as +-2^29 under the set's own noise, a fresh mask seed and fresh noise per call; a batch of higher rank keeps its shape"""
    keys = secrets(p)
    bits = np.random.default_rng(5).integers(0, 2, (4, 32)).astype(bool)
    seeds = set()
    for party in range(p.nparty):
        batch = mk.seeded_encrypt(bits, keys[party], p, party)
        assert batch.body.shape == bits.shape and len(batch.mask_seed) == 32
        seeds.add(batch.mask_seed)
        rows = mk.seeded_expand(batch, p)
        assert rows.shape == bits.shape + (p.lwe_len,)
        assert np.array_equal(mk.lwe_decrypt(rows, keys if p.multikey else keys[0], p), bits), party
    assert len(seeds) == p.nparty, "two calls drew one mask seed"


def _raw(p):
    return C.byref(p.c())


def test_refusals_leave_the_output_untouched():
    """every refusal of the header's list is MKT_ERR_ARG = -1 with the 0xA5-filled outputs as they were; B == 0 succeeds and writes nothing"""
    p = mk.KMS2party.scaled(n=16, N=256)
    other = mk.KMS2party.scaled(n=17, N=256)
    keys, okeys = secrets(p), secrets(other)
    L = _lib.lib()
    mu = np.zeros(5, dtype=np.uint32)
    body = np.full(5, 0xA5A5A5A5, dtype=np.uint32)
    rows = np.full((5, p.lwe_len), 0xA5A5A5A5, dtype=np.uint32)
    ms = (C.c_uint8 * 32)(*MASK_SEED)
    same = (C.c_uint8 * 32)(*MASK_SEED)
    ns = (C.c_uint8 * 32)(*range(32))

    def enc(party=1, key=keys[1], sigma=p.alpha, mseed=ms, nseed=ns, B=5):
        return L.mkt_client_seeded_encrypt(_raw(p), key.h, party, S._np_ptr(mu), sigma, mseed, nseed, 0, S._np_ptr(body), B)

    def exp(party=1, mseed=ms, B=5):
        return L.mkt_client_seeded_expand(_raw(p), party, mseed, 0, S._np_ptr(mu), S._np_ptr(rows), B)

    for kw in (dict(mseed=None), dict(nseed=same), dict(party=-1), dict(party=2), dict(party=0), dict(key=okeys[1]), dict(sigma=-1.0),
               dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma=float(np.nextafter(2.0**31, np.inf)))):
        assert enc(**kw) == -1 and (body == 0xA5A5A5A5).all(), kw
    for kw in (dict(mseed=None), dict(party=-1), dict(party=2)):
        assert exp(**kw) == -1 and (rows == 0xA5A5A5A5).all(), kw
    assert enc(B=0) == 0 and exp(B=0) == 0 and (body == 0xA5A5A5A5).all() and (rows == 0xA5A5A5A5).all()
    assert enc(sigma=2.0**31) == 0 and enc(sigma=0.0) == 0 and exp() == 0 and not (rows == 0xA5A5A5A5).all()


def test_two_calls_without_a_noise_seed_differ():
    p = mk.KMS2party.scaled(n=16, N=256)
    keys = secrets(p)
    mu = np.zeros(64, dtype=np.uint32)
    a, b = (mk.seeded_encrypt(mu, keys[0], p, 0, words=True, mask_seed=MASK_SEED).body for _ in range(2))
    assert (a != b).mean() > 0.9, "two NULL-seed calls drew the same noise"
    pinned = [mk.seeded_encrypt(mu, keys[0], p, 0, words=True, mask_seed=MASK_SEED, deterministic_seed=1).body for _ in range(2)]
    assert np.array_equal(*pinned)


def test_the_new_streams_are_their_own():
    """under ONE key, the mask of stream 10 is not the mask stream 7 gives mkt_client_lwe_encrypt, and a row of stream 7 is reproducible
    as before: factoring row_noise_word out of smudge_word and adding ids 10 and 11 moved no existing word (the word-for-word pins of
    streams 7 and 9 are tests/test_keys_cpu.py's and tests/test_partial_decrypt_cpu.py's)"""
    p = mk.KMS2party.scaled(n=4, N=256)
    keys = secrets(p)
    seed = (C.c_uint8 * 32)()
    assert _lib.lib().mkt_client_test_seed(3, seed) == 0
    row = mk.lwe_ith_encrypt(1, 1, keys[1], p, deterministic_seed=bytes(seed))
    assert not row[:4].any() and np.array_equal(row, mk.lwe_ith_encrypt(1, 1, keys[1], p, deterministic_seed=3))
    batch = mk.seeded_encrypt([1], keys[1], p, 1, mask_seed=bytes(seed), deterministic_seed=4)
    assert not np.array_equal(mk.seeded_expand(batch, p)[0, 4:8], row[4:8])


def test_header_ctypes_and_package_hold_the_new_names():
    hdr = open(os.path.join(ROOT, "include", "mktfhe.h")).read()
    for name in ("mkt_client_seeded_encrypt", "mkt_client_seeded_expand", "mkt_seeded_expand_batch", "mkt_seeded_encrypt_batch"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/mktfhe.h"
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == len(m.group(1).split(",")), name
        assert hasattr(_lib.lib(), name)
    assert "seeded ciphertexts" in hdr
    for name in ("SeededBatch", "seeded_encrypt", "seeded_expand"):
        assert hasattr(mk, name)
    src = open(os.path.join(ROOT, "mktfhe_amd", "csrc", "rng_chacha.h")).read()
    assert "STREAM_ENC_MASK = 10" in src and "STREAM_ENC_NOISE = 11" in src
