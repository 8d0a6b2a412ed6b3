"""Distributed decryption on the host (include/mktfhe.h "distributed decryption"; mktfhe_amd/decrypt.py): a share per party from its own
block of the mask, smudged, merged by anyone.  What is held here: the merge identity against mkt_client_lwe_phase / _decrypt at
sigma_smudge = 0, that a share reads its own block only, that the smudging noise is the specified stream and follows its law (thresholds:
ref_keys.ALPHA, derived there from a 1e-6 false-failure budget), end-to-end bits, the refusals and the surface."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ref_keys as R
from helpers import ROOT, mk, secret_keys as secrets
from mktfhe_amd import _lib, decrypt as D, scheme as S

# one reduced set per scheme, plus KMS8party and CCS16party: the sizes of tests/test_gpu_parity.py SMALL
SETS = [
    mk.CGGIparam.scaled(n=20, N=256), mk.Blockparam.scaled(n=30, N=256, blk_d=10), mk.CCS2party.scaled(n=12, N=256),
    mk.KMS2party.scaled(n=16, N=256), mk.KMS2partyblock.scaled(n=24, N=256, blk_d=8), mk.KMS8party.scaled(n=4, N=256),
    mk.CCS16party.scaled(n=2, N=256),
]
IDS = lambda p: f"{p.name}-n{p.n}"      # noqa: E731
SIGMA = 2.0 ** 20


def shares_of(p, keys, ct, sigma, seed=5, row0=0):
    return [mk.partial_decrypt(ct, keys[i], p, i, sigma, deterministic_seed=seed, row0=row0) for i in range(p.nparty)]


def mask_sum(p, keys, ct):
    """sum_i <a_i, s_i> mod 2^32, in numpy"""
    s = np.concatenate([np.array(k.lwekey) for k in keys]).astype(np.uint32)
    return (ct[:, :-1] * s).sum(-1, dtype=np.uint32)


@pytest.mark.parametrize("p", SETS, ids=IDS)
def test_merge_identity_at_sigma_zero(p):
    """sigma_smudge = 0: merge_phase == mkt_client_lwe_phase word for word and merge_decrypt == mkt_client_lwe_decrypt bit for bit, on 257
    uniform rows, rows built to land the phase on 0, 2^31 - 1, 2^31, 2^32 - 1 (both sides of each decision border of either rule, and of the
    single-key rule's own borders 2^28 and 3 2^28), and a row of all-ones words"""
    rng = np.random.default_rng(1)
    keys = secrets(p)
    targets = [0, 2**31 - 1, 2**31, 2**32 - 1, 2**28 - 1, 2**28, 3 * 2**28 - 1, 3 * 2**28]
    ct = rng.integers(0, 2**32, (257 + len(targets) + 1, p.lwe_len), dtype=np.uint64).astype(np.uint32)
    edge = ct[257:257 + len(targets)]
    edge[:, -1] = (np.array(targets, dtype=np.uint64) - mask_sum(p, keys, edge)).astype(np.uint32)
    ct[-1] = 0xFFFFFFFF
    sh = shares_of(p, keys, ct, 0.0)
    assert all(s.shape == (ct.shape[0],) and s.dtype == np.uint32 for s in sh)
    want = mk.lwe_phase(ct, keys if p.multikey else keys[0], p)
    assert np.array_equal(want[257:257 + len(targets)], np.array(targets, dtype=np.uint32)), "the built rows miss their phases"
    assert np.array_equal(mk.merge_phase(ct, sh, p), want)
    bits = mk.merge_decrypt(ct, sh, p)
    assert bits.dtype == bool and np.array_equal(bits, mk.lwe_decrypt(ct, keys if p.multikey else keys[0], p))
    assert 0 < bits.sum() < bits.size
    # one row, and a batch of higher rank, keep their shapes
    assert mk.partial_decrypt(ct[3], keys[0], p, 0, 0.0).shape == (1,)
    cube = ct[:256].reshape(4, 64, p.lwe_len)
    assert np.array_equal(mk.merge_phase(cube, [s[:256].reshape(4, 64) for s in sh], p), want[:256].reshape(4, 64))


def test_a_share_reads_its_own_block_only():
    """rewriting every other party's block and b leaves share_i unchanged, word for word; changing one word of block i that meets a
    non-zero key word changes it"""
    p = mk.KMS4party.scaled(n=10, N=256)
    rng = np.random.default_rng(2)
    keys = secrets(p)
    ct = rng.integers(0, 2**32, (65, p.lwe_len), dtype=np.uint64).astype(np.uint32)
    for i in range(p.nparty):
        mine = mk.partial_decrypt(ct, keys[i], p, i, SIGMA, deterministic_seed=9)
        other = rng.integers(0, 2**32, ct.shape, dtype=np.uint64).astype(np.uint32)
        other[:, i * p.n:(i + 1) * p.n] = ct[:, i * p.n:(i + 1) * p.n]
        assert np.array_equal(mk.partial_decrypt(other, keys[i], p, i, SIGMA, deterministic_seed=9), mine), i
        q = int(np.flatnonzero(np.array(keys[i].lwekey))[0])
        touched = ct.copy()
        touched[7, i * p.n + q] += np.uint32(1)
        got = mk.partial_decrypt(touched, keys[i], p, i, SIGMA, deterministic_seed=9)
        assert got[7] != mine[7] and np.array_equal(np.delete(got, 7), np.delete(mine, 7)), i


NOISE_P = mk.KMS2party.scaled(n=4, N=256)
NOISE_B = 65_536


@pytest.fixture(scope="module")
def noise_case():
    keys = secrets(NOISE_P)
    return keys, np.zeros((NOISE_B, NOISE_P.lwe_len), dtype=np.uint32)      # block i zeroed: the shares ARE the noise words


@pytest.mark.parametrize("sigma", [3.0, SIGMA], ids=["sigma3", "sigma2^20"])
def test_the_noise_follows_its_law(noise_case, sigma):
    """65 536 noise words per sigma against round(sigma N(0, 1)), by the helpers and the threshold tests/test_keys_cpu.py applies to a
    fresh encryption's noise (ref_keys.noise_stats, p >= ref_keys.ALPHA = 2.5e-10 per check; this module makes some twenty such checks, far
    inside the 4000 the threshold was derived for): mean, variance, lag-1 correlation along rows of 256, and -- as noise_stats splits
    them -- the exact histogram at sigma = 3 (where a kurtosis estimate is biased by the rounding), kurtosis and the share beyond
    3 sigma at sigma = 2^20; max|e| <= 6 sigma + 1; no row of 256 words drawn twice.  Both parties' words are judged"""
    keys, ct = noise_case
    for i in range(2):
        e = R.centered(mk.partial_decrypt(ct, keys[i], NOISE_P, i, sigma, deterministic_seed=21), 32)
        assert int(np.abs(e).max()) <= 6 * sigma + 1
        stats = R.noise_stats(e.reshape(-1, 256), sigma)
        assert {"mean", "variance", "lag1"} <= set(stats) and ({"kurtosis", "beyond 3 sigma"} <= set(stats) if sigma > 128 else "histogram" in stats)
        for name, pv in stats.items():
            assert pv >= R.ALPHA, (i, sigma, name, "p = %.3g" % pv)
        assert R.count_equal_rows(e.reshape(-1, 256)) == 0


def test_the_noise_is_the_specified_stream(noise_case):
    """row j of a call with row0 = r is row r + j of a call with row0 = 0, also where the row index carries into the high word; two parties
    under one seed differ; two seeds differ; two NULL-seed calls differ; sigma scales one underlying draw"""
    keys, ct = noise_case
    p, c = NOISE_P, ct[:4096]
    base = mk.partial_decrypt(c, keys[0], p, 0, SIGMA, deterministic_seed=21)
    for r in (1, 1000, 4095):
        assert np.array_equal(mk.partial_decrypt(c[:4096 - r], keys[0], p, 0, SIGMA, deterministic_seed=21, row0=r), base[r:]), r
    hi = mk.partial_decrypt(c[:8], keys[0], p, 0, SIGMA, deterministic_seed=21, row0=2**32 - 3)
    assert np.array_equal(hi[3:], mk.partial_decrypt(c[:5], keys[0], p, 0, SIGMA, deterministic_seed=21, row0=2**32))
    assert np.array_equal(hi[:3], mk.partial_decrypt(c[:3], keys[0], p, 0, SIGMA, deterministic_seed=21, row0=2**32 - 3))
    assert not np.array_equal(hi[3:], base[:5]), "the high word of the row index does not reach the stream"
    top = mk.partial_decrypt(c[:2], keys[0], p, 0, SIGMA, deterministic_seed=21, row0=2**64 - 2)
    assert np.array_equal(top[:1], mk.partial_decrypt(c[:1], keys[0], p, 0, SIGMA, deterministic_seed=21, row0=2**64 - 2))
    other = mk.partial_decrypt(c, keys[1], p, 1, SIGMA, deterministic_seed=21)
    assert (other != base).mean() > 0.99, "two parties under one seed share noise"
    assert (mk.partial_decrypt(c, keys[0], p, 0, SIGMA, deterministic_seed=22) != base).mean() > 0.99
    a, b = (mk.partial_decrypt(c, keys[0], p, 0, SIGMA) for _ in range(2))
    assert (a != b).mean() > 0.99 and (a != base).mean() > 0.99, "two NULL-seed calls drew the same noise"
    # the same Gaussian draw under another sigma: e(2 sigma) = 2 e(sigma) up to the rounding
    twice = R.centered(mk.partial_decrypt(c, keys[0], p, 0, 2 * SIGMA, deterministic_seed=21), 32)
    assert np.abs(twice - 2 * R.centered(base, 32)).max() <= 1
    assert not mk.partial_decrypt(c, keys[0], p, 0, 0.0, deterministic_seed=21).any()


@pytest.mark.parametrize("p", [mk.KMS2party.scaled(n=16, N=256), mk.CCS4party.scaled(n=6, N=256)], ids=IDS)
def test_end_to_end_bits(p):
    """Known bits, each encrypted by one party (lwe_ith_encrypt: message +-2^29, noise alpha = 2^17 in that party's block) and summed with
    a fresh encryption of the torus word 0 under every other party, so that every block of every row is populated as in the tests' mixed
    inputs; every party smudges with sigma_smudge = 2^20 and merge_decrypt returns the bits.
    MARGIN.  The merged phase is +-2^29 + k encryption noises + k smudging noises: deviation sqrt(k (2^34 + 2^40)) = 2^20 sqrt(k) 1.008.
    The bit flips only beyond the margin 2^29, i.e. 2^9 / (1.008 sqrt k) deviations: 359 sigma at k = 2, 254 sigma at k = 4 -- more than
    100 sigma, so a wrong bit here is a bug, not noise"""
    k = p.nparty
    assert 2.0**29 / math.sqrt(k * (p.alpha**2 + SIGMA**2)) > 100
    rng = np.random.default_rng(4)
    keys = secrets(p)
    B = 96
    bits = rng.integers(0, 2, B).astype(bool)
    ct = np.zeros((B, p.lwe_len), dtype=np.uint32)
    for j in range(B):
        for i in range(k):
            ct[j] += mk.lwe_ith_encrypt(bits[j], i, keys[i], p) if i == j % k else mk.lwe_encrypt_word(0, i, keys[i], p)
    assert (ct[:, :-1].reshape(B, k, p.n) != 0).any(axis=2).all(), "every party block populated"
    sh = [mk.partial_decrypt(ct, keys[i], p, i, SIGMA) for i in range(k)]       # fresh entropy per party, as deployed
    assert np.array_equal(mk.merge_decrypt(ct, sh, p), bits)
    err = R.centered(mk.merge_phase(ct, sh, p) - np.where(bits, 2**29, 2**32 - 2**29).astype(np.uint32), 32)
    assert np.abs(err).max() < 2**29 // 32 and np.abs(err).max() > SIGMA / 4, "the merged phase is message + noise of the smudging size"
    # without the smudging the same rows carry the encryption noise only: the shares did add noise
    quiet = R.centered(mk.lwe_phase(ct, keys, p) - np.where(bits, 2**29, 2**32 - 2**29).astype(np.uint32), 32)
    assert np.abs(quiet).max() < 8 * math.sqrt(k) * p.alpha


# ---- refusals: MKT_ERR_ARG and no word written ----
SENT = 0xA5A5A5A5


def _raw(p):
    keys = secrets(p)
    ct = np.random.default_rng(6).integers(0, 2**32, (5, p.lwe_len), dtype=np.uint64).astype(np.uint32)
    return keys, ct, np.full(5, SENT, dtype=np.uint32)


def test_partial_decrypt_refusals():
    p = mk.KMS2party.scaled(n=16, N=256)
    L, pc = _lib.lib(), C.byref(p.c())
    keys, ct, out = _raw(p)
    ptr = S._np_ptr
    call = lambda party=0, key=keys[0].h, lwe=ptr(ct), sigma=SIGMA, o=ptr(out), B=5, par=pc: L.mkt_client_partial_decrypt(par, key, party, lwe, sigma, None, 0, o, B)   # noqa: E731
    bad = [dict(party=-1), dict(party=2), dict(party=1), dict(key=None), dict(lwe=None), dict(par=None), dict(sigma=-1.0), dict(sigma=-1e-300),
           dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma=float(np.nextafter(2.0**31, np.inf))), dict(sigma=2.0**32)]
    for kw in bad:       # (party = 1 with party 0's keys: keys made for another party index)
        assert call(**kw) == -1, kw
        assert (out == SENT).all(), kw
    assert call(o=None) == -1
    assert call(B=0) == 0 and (out == SENT).all(), "B = 0 succeeds and writes nothing"
    for ok in (0.0, 2.0**31):
        assert call(sigma=ok) == 0 and not (out == SENT).all()
        out[:] = SENT
    # keys made for other parameters
    q = mk.KMS2party.scaled(n=12, N=256)
    assert L.mkt_client_partial_decrypt(C.byref(q.c()), keys[0].h, 0, ptr(ct), SIGMA, None, 0, ptr(out), 1) == -1 and (out == SENT).all()
    # the Python layer raises MktError(-1) for the same arguments, ValueError for a batch that is not rows of lwe_len words
    for kw in (dict(party=2), dict(sigma_smudge=-1.0), dict(sigma_smudge=float("nan")), dict(sigma_smudge=2.0**31 + 1)):
        args = dict(party=0, sigma_smudge=SIGMA)
        args.update(kw)
        with pytest.raises(mk.MktError) as ei:
            mk.partial_decrypt(ct, keys[0], p, **args)
        assert ei.value.code == -1
    with pytest.raises(ValueError):
        mk.partial_decrypt(ct[:, :-1], keys[0], p, 0, SIGMA)
    with pytest.raises(ValueError):
        mk.partial_decrypt(ct, keys[0], p, 0, SIGMA, row0=2**64)


def test_lwe_decrypt_is_the_bit_rule_on_lwe_phase():
    """mkt_client_lwe_decrypt decides on mkt_client_lwe_phase's word -- for a multi-key set the bit is phase < 2^31 -- on 64 uniform rows;
    through the raw ABI a NULL entry in `keys` is MKT_ERR_ARG from either call, as a NULL `keys` is"""
    p = mk.KMS2party.scaled(n=16, N=256)
    keys = secrets(p)
    ct = np.random.default_rng(9).integers(0, 2**32, (64, p.lwe_len), dtype=np.uint64).astype(np.uint32)
    phase = mk.lwe_phase(ct, keys, p)
    bits = mk.lwe_decrypt(ct, keys, p)
    assert bits.dtype == bool and np.array_equal(bits, phase < 2**31) and 0 < bits.sum() < 64
    L, pc, word = _lib.lib(), C.byref(p.c()), C.c_uint32(SENT)
    for arr in ((C.c_void_p * 2)(keys[0].h, None), (C.c_void_p * 2)(None, keys[1].h), None):
        assert L.mkt_client_lwe_decrypt(pc, arr, 2, S._np_ptr(ct[0])) == -1
        assert L.mkt_client_lwe_phase(pc, arr, 2, S._np_ptr(ct[0]), C.byref(word)) == -1 and word.value == SENT
    both = (C.c_void_p * 2)(keys[0].h, keys[1].h)
    assert L.mkt_client_lwe_decrypt(pc, both, 2, S._np_ptr(ct[0])) == int(bits[0])
    assert L.mkt_client_lwe_decrypt(pc, both, 1, S._np_ptr(ct[0])) == -1       # a party count that is not the set's


@pytest.mark.parametrize("fn,dt", [("mkt_client_merge_phase", np.uint32), ("mkt_client_merge_decrypt", np.uint8)])
def test_merge_refusals(fn, dt):
    p = mk.KMS2party.scaled(n=16, N=256)
    L, pc, ptr = _lib.lib(), C.byref(p.c()), S._np_ptr
    keys, ct, _ = _raw(p)
    sh = np.zeros((3, 5), dtype=np.uint32)
    out = np.full(5, SENT & 0xFF, dtype=dt)
    f = getattr(L, fn)
    for nparties in (0, 1, 3, -2):
        assert f(pc, ptr(ct), ptr(sh), nparties, ptr(out), 5) == -1 and (out == (SENT & 0xFF)).all(), nparties
    for args in ((None, ptr(ct), ptr(sh), 2, ptr(out), 5), (pc, None, ptr(sh), 2, ptr(out), 5), (pc, ptr(ct), None, 2, ptr(out), 5), (pc, ptr(ct), ptr(sh), 2, None, 5)):
        assert f(*args) == -1 and (out == (SENT & 0xFF)).all()
    assert f(pc, ptr(ct), ptr(sh), 2, ptr(out), 0) == 0 and (out == (SENT & 0xFF)).all(), "B = 0 succeeds and writes nothing"
    assert f(pc, ptr(ct), ptr(sh), 2, ptr(out), 5) == 0
    py = mk.merge_phase if dt is np.uint32 else mk.merge_decrypt
    with pytest.raises(mk.MktError) as ei:
        py(ct, list(sh), p)                       # three shares for two parties
    assert ei.value.code == -1
    with pytest.raises(ValueError):
        py(ct, [sh[0], sh[1][:4]], p)             # a share that is not one word per ciphertext
    # a single-key scheme has ONE party whatever its RLWE length
    q = mk.CGGIparam.scaled(n=16, N=256, k=2)
    kq = secrets(q)
    cq = np.zeros((2, q.lwe_len), dtype=np.uint32)
    assert cq.shape[1] == q.n + 1 and py(cq, [mk.partial_decrypt(cq, kq[0], q, 0, 0.0)], q).shape == (2,)
    with pytest.raises(mk.MktError):
        py(cq, [np.zeros(2, np.uint32)] * 2, q)


# ---- the surface ----
NEW_SYMBOLS = ["mkt_client_partial_decrypt", "mkt_client_merge_phase", "mkt_client_merge_decrypt", "mkt_partial_decrypt_batch"]
NEW_NAMES = ["partial_decrypt", "merge_phase", "merge_decrypt"]


def test_header_ctypes_and_package_hold_the_new_names():
    """the header declares the four symbols under "distributed decryption", _lib binds each with the header's argument count, the library
    exports them, the package re-exports the module-level Python names, and neither Scheme nor MultiScheme gained a public method.
    MKT_ABI_VERSION stays 3: new symbols only"""
    hdr = open(os.path.join(ROOT, "include", "mktfhe.h")).read()
    assert "distributed decryption" in hdr
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/mktfhe.h"
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == len(m.group(1).split(",")), name
        assert hasattr(_lib.lib(), name), f"{name} is not exported by the library"
    assert re.search(r"#define\s+MKT_ABI_VERSION\s+3\b", hdr) and _lib.lib().mkt_abi_version() == 3
    for name in NEW_NAMES:
        assert getattr(mk, name) is getattr(D, name)
    for cls in (S.Scheme, S.MultiScheme):
        assert not [n for n in dir(cls) if "decrypt" in n or "merge" in n or "share" in n], cls.__name__
    used = set(re.findall(r"\b(mkt_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "examples", "distributed_decrypt.c")).read()))
    assert set(NEW_SYMBOLS[:1] + NEW_SYMBOLS[2:]) <= used <= set(_lib.SYMBOLS), used - set(_lib.SYMBOLS)


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("mkt_"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


def test_the_device_path_goes_through_the_checked_call(monkeypatch):
    """partial_decrypt(scheme=...) reaches mkt_partial_decrypt_batch through Scheme._call with the header's argument count, B rows and the
    memory kind of the arrays; a batch that is not B rows of lwe_len words never reaches the library (the library is a recording stub)"""
    p = mk.KMS2party.scaled(n=16, N=256)
    keys = secrets(p)
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    sch = object.__new__(S.Scheme)
    sch.params, sch.device, sch.h, sch._user_stream, sch._owned = p, 0, C.c_void_p(1), True, False
    ct = np.zeros((3, 7, p.lwe_len), dtype=np.uint32)
    out = mk.partial_decrypt(ct, keys[1], p, 1, 3.0, scheme=sch, deterministic_seed=4, row0=2**40)
    (name, args), = [c for c in rec.calls if c[0] == "mkt_partial_decrypt_batch"]
    assert out.shape == (3, 7) and out.dtype == np.uint32
    assert len(args) == len(_lib.SYMBOLS[name][1]) and args[1] == 1 and args[4] == 3.0 and args[6] == 2**40 and args[-2:] == (21, S.MEM_HOST)
    n = len(rec.calls)
    with pytest.raises(ValueError):
        mk.partial_decrypt(ct[..., :-1], keys[1], p, 1, 3.0, scheme=sch)
    assert len(rec.calls) == n


def test_smudged_failure_prediction():
    """tools/noise_theory.smudged_failure: erfc of the margin 1/8 over the deviation sqrt(sigma_b^2 + nparty sigma_smudge^2)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("noise_theory", os.path.join(ROOT, "tools", "noise_theory.py"))
    nt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(nt)
    p = mk.CCS4party
    assert nt.smudged_failure(p, 0.0, sigma_b=0.0) == 0.0
    assert nt.smudged_failure(p, 0.0, sigma_b=0.125) == pytest.approx(math.erfc(1 / math.sqrt(2)))            # one sigma
    assert nt.smudged_failure(p, 2.0**28, sigma_b=0.0) == pytest.approx(math.erfc(0.125 / (2 * 2.0**-4) / math.sqrt(2)))   # sqrt(4) 2^-4 = 1/8: one sigma
    assert nt.smudged_failure(mk.CGGIparam, 2.0**28, sigma_b=0.0) == pytest.approx(math.erfc(2 / math.sqrt(2)))   # one party
    f = [nt.smudged_failure(p, s, sigma_b=0.01) for s in (0.0, 2.0**20, 2.0**24, 2.0**26, 2.0**28)]
    assert f == sorted(f) and f[0] < 1e-30 and f[-1] > 0.1
