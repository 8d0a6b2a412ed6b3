"""Key switch at a coefficient / bootstrap at a coefficient list (include/mktfhe.h "key switch at a coefficient"), on the CPU:
the law that makes it useful -- coefficient v of X^phi * T is the single-table read of T at phi - v -- exhaustively at N = 64, the
thermometer law of the sign table, the whole construction on the CPU checker chain (oracle rotation, numpy extraction E_v, oracle key
switch) at CGGIparam, and the surface: header, ctypes table, Python names and their argument checks (recording stub, as
tests/test_batch_args_cpu.py)."""
import functools
import os
import re

import numpy as np
import pytest

import ref_lut as R
import ref_lut_many as RM
from helpers import ROOT, keygen, mk, oracle_scheme
from mktfhe_amd import _lib
from mktfhe_amd import scheme as S

NEW_SYMBOLS = ["mkt_keyswitch_at_batch", "mkt_lut_bootstrap_at_batch", "mkt_lut_batch_gather_at", "mkt_multi_lut_bootstrap_at_batch"]
NEW_NAMES = ["keyswitch_at", "lut_bootstrap_at", "lut_gather_at", "lut_threshold_coefs"]


# ---- the law ----
@pytest.mark.parametrize("W", [32, 64])
def test_coefficient_v_of_the_rotated_table_is_the_read_at_phi_minus_v(W):
    """EVERY v < N and every mod-switched phase phi < 2N: (X^phi T)[v] == what lut_bootstrap(T) extracts at (phi - v) mod 2N"""
    N = 64
    rng = np.random.default_rng(W)
    T = (rng.integers(0, 1 << 63, N, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, N, dtype=np.uint64)) & np.uint64((1 << W) - 1)
    T[:3] = [0, 1, 1 << (W - 1)]
    for phi in range(2 * N):
        rot = R.rotate(T, phi, W)
        for v in range(N):
            assert int(rot[v]) == R.extracted(T, (phi - v) % (2 * N), W), (phi, v)
            assert int(RM.extract(rot, v, W)[0]) == int(rot[v])          # E_v moves that coefficient to 0, where keyswitch! reads the body


def thermometer_coefs(P, N):
    assert N % P == 0
    return [w * (N // P) for w in range(P)]


@pytest.mark.parametrize("P", [2, 4, 8])
@pytest.mark.parametrize("W", [32, 64])
def test_thermometer_law_of_the_sign_table(W, P):
    """sign table, coef[w] = w N / P: for an input whose mod-switched phase lies inside window m of P (every such phase, the centre
    (2m + 1) N / 2P among them), output w reads +2^(W-3) iff m >= w"""
    N = 64
    p = mk.CGGIparam.scaled(n=8, N=N, W=W)
    T = mk.sign_lut(p)
    coefs = mk.lut_threshold_coefs(P, p)
    assert list(coefs) == thermometer_coefs(P, N) and coefs.dtype == np.uint32
    plus, minus = 1 << (W - 3), (1 << W) - (1 << (W - 3))
    for m in range(P):
        for phi in range(m * N // P + 1, (m + 1) * N // P):
            rot = R.rotate(T, phi, W)
            for w in range(P):
                assert int(rot[coefs[w]]) == (plus if m >= w else minus), (m, w, phi)
    with pytest.raises(ValueError):
        mk.lut_threshold_coefs(3, p)
    with pytest.raises(ValueError):
        mk.lut_threshold_coefs(0, p)


# ---- the whole construction on the CPU checker ----
def checker_at(so, T, lwe, coefs, W, nout=1):
    """the bootstrap at a coefficient list of ONE ciphertext on the CPU checker: sw_nu (nout = 2^nu; 1 = the fine switch), the table step,
    so.blindrotate, then for every coefficient the numpy extraction E_v and so.keyswitch -> (ncoef, lwe_len) uint32"""
    at, bt = RM.sw_row(lwe, len(T), nout)
    acc = so.blindrotate(at, R.testvector(T, bt, W, so.kacc))
    return np.stack([so.keyswitch(RM.extract(acc, int(v), W)) for v in coefs])


@functools.lru_cache(maxsize=None)
def thermometer_case(name, P=8, seed=81):
    """pinned keys, fresh inputs m = 0 .. P-1 at phase m / 2P + 1 / 4P, and the checker chain's words (P, P, lwe_len): computed once, shared
    with tests/test_gpu_keyswitch_at.py -> (p, crs, keys, c, words)"""
    p = getattr(mk, name)
    crs, keys = keygen(p, seed)
    step = (1 << 32) // (2 * P)
    c = np.stack([mk.lwe_encrypt_word(m * step + step // 2, m % p.nparty, keys[m % p.nparty], p, deterministic_seed=8100 + m) for m in range(P)])
    so = oracle_scheme(p, crs, keys)
    coefs = thermometer_coefs(P, p.N)
    words = np.stack([checker_at(so, mk.sign_lut(p), c[m], coefs, p.W) for m in range(P)])
    words.setflags(write=False); c.setflags(write=False)
    return p, crs, keys, c, words


def thermometer_bits(P=8):
    return np.array([[m >= w for w in range(P)] for m in range(P)])


def test_thermometer_decrypts_on_the_checker_chain():
    """CGGIparam, P = 8, fresh inputs: all 64 (m, w) outputs decrypt to [m >= w].  By DESIGN.md 1b's table the margin 1/32 is more than
    12 sigma of a fresh input's mod-switched phase, so a wrong bit is a bug"""
    p, crs, keys, c, words = thermometer_case("CGGIparam")
    assert words.shape == (8, 8, p.lwe_len)
    assert np.array_equal(mk.lwe_decrypt(words, keys[0], p), thermometer_bits())


# ---- the surface ----
def test_header_ctypes_and_package_hold_the_new_names():
    """fails without the feature: the header declares the four symbols, _lib binds each with the header's argument count, the library
    exports them, and the package exports the Python names.  MKT_ABI_VERSION stays 3: new symbols only"""
    hdr = open(os.path.join(ROOT, "include", "mktfhe.h")).read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/mktfhe.h"
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == len(m.group(1).split(",")), name
        assert hasattr(_lib.lib(), name), f"{name} is not exported by the library"
    assert re.search(r"#define\s+MKT_ABI_VERSION\s+3\b", hdr) and _lib.lib().mkt_abi_version() == 3
    from mktfhe_amd import lut as L
    for name in NEW_NAMES:
        assert getattr(mk, name) is getattr(L, name)
        assert not hasattr(S.Scheme, name) and not hasattr(S.MultiScheme, name)      # module-level, as the rest of the table-lookup surface
    jl = open(os.path.join(ROOT, "integration", "MKTFHEHip.jl")).read()
    assert all(":" + name in jl for name in NEW_SYMBOLS[:3])


# ---- argument checks of the Python layer (the library is a recording stub) ----
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("mkt_"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


@pytest.fixture
def lib(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    return rec


def _make(cls, p):
    s = object.__new__(cls)
    s.params, s.h, s.arith = p, None, S.ARITH_F64REF
    if cls is S.Scheme:
        s.device, s._user_stream = 0, False
    return s


PARAMS = [mk.CGGIparam.scaled(n=10, N=256), mk.KMS2party.scaled(n=8, N=256)]
B, NC = 3, 5


@pytest.mark.parametrize("p", PARAMS, ids=lambda p: p.name)
@pytest.mark.parametrize("cls", [S.Scheme, S.MultiScheme], ids=lambda c: c.__name__)
def test_bootstrap_at_reaches_its_symbol_and_refuses_wrong_sizes(lib, cls, p):
    s = _make(cls, p)
    x, T, coef = np.zeros((B, p.lwe_len), np.uint32), mk.sign_lut(p), np.arange(NC, dtype=np.uint32)
    out = mk.lut_bootstrap_at(s, T, x, coef, nu=1)
    name = ("mkt_multi_" if cls is S.MultiScheme else "mkt_") + "lut_bootstrap_at_batch"
    assert [c[0] for c in lib.calls] == [name] and out.shape == (B, NC, p.lwe_len)
    args = lib.calls[0][1]
    assert len(args) == len(_lib.SYMBOLS[name][1]) and args[-2:] == (B, S.MEM_HOST) and args[2] == 1 and args[3] is None and args[5] == 1 and args[7] == NC
    lib.calls.clear()
    for bad in (dict(coef=coef[:0]), dict(coef=np.arange(p.N + 1)), dict(coef=[0, p.N]), dict(coef=[-1]), dict(coef=np.zeros((2, 2), np.uint32)), dict(coef=[0.5]),
                dict(nu=4), dict(nu=-1), dict(out=np.zeros((B, NC - 1, p.lwe_len), np.uint32)), dict(sel=np.zeros(B + 1, np.uint32)),
                dict(luts=np.zeros(p.N - 1, p.ring_dtype))):
        kw = dict(luts=T, ctxt=x, coef=coef)
        kw.update(bad)
        with pytest.raises(ValueError):
            mk.lut_bootstrap_at(s, **kw)
        assert lib.calls == [], bad


@pytest.mark.parametrize("p", PARAMS, ids=lambda p: p.name)
def test_gather_at_and_keyswitch_at_reach_their_symbols_and_refuse_wrong_sizes(lib, p):
    s = _make(S.Scheme, p)
    P = 4
    pool, idx, wt, cst = np.zeros((P, p.lwe_len), np.uint32), np.zeros((B, 4), np.uint32), np.zeros((B, 4), np.int8), np.zeros(B, np.uint32)
    out, coef = np.zeros((B * NC, p.lwe_len), np.uint32), np.arange(NC, dtype=np.uint32)
    assert mk.lut_gather_at(s, mk.sign_lut(p), None, pool, idx, wt, cst, coef, out) is out
    name, args = lib.calls.pop()
    assert name == "mkt_lut_batch_gather_at" and len(args) == len(_lib.SYMBOLS[name][1]) and args[-2:] == (B, S.MEM_HOST) and args[5] == P and args[9] == 0 and args[11] == NC
    for bad in (dict(out=out[:-1]), dict(idx=idx[:-1]), dict(coef=[p.N]), dict(nu=9)):
        kw = dict(luts=mk.sign_lut(p), sel=None, pool=pool, idx=idx, wt=wt, cst=cst, coef=coef, out=out)
        kw.update(bad)
        with pytest.raises(ValueError):
            mk.lut_gather_at(s, **kw)
        assert lib.calls == [], bad
    nacc = 2
    acc = np.zeros((nacc, p.k + 1, p.N), p.ring_dtype)
    src, cf = np.zeros(B, np.uint32), np.zeros(B, np.uint32)
    assert mk.keyswitch_at(s, acc, src, cf).shape == (B, p.lwe_len)
    name, args = lib.calls.pop()
    assert name == "mkt_keyswitch_at_batch" and len(args) == len(_lib.SYMBOLS[name][1]) and args[2] == nacc and args[-2:] == (B, S.MEM_HOST)
    assert mk.keyswitch_at(s, acc).shape == (nacc, p.lwe_len)
    name, args = lib.calls.pop()
    assert args[3] is None and args[4] is None and args[2] == nacc and args[-2] == nacc
    assert mk.keyswitch_at(s, acc, coef=np.zeros(nacc, np.uint32)).shape == (nacc, p.lwe_len) and lib.calls.pop()[1][3] is None
    for bad in (dict(acc=acc.reshape(nacc, -1)), dict(src=src, coef=cf[:-1]), dict(acc=acc[..., :-1])):
        kw = dict(acc=acc, src=src, coef=cf)
        kw.update(bad)
        with pytest.raises(ValueError):
            mk.keyswitch_at(s, **kw)
        assert lib.calls == [], bad
