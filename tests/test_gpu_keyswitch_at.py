"""Key switch at a coefficient and the bootstrap at a coefficient list on the GPU (mktfhe.h "key switch at a coefficient", mktfhe_amd/lut.py,
DESIGN.md 1d), word for word (tolerance 0: every comparison is integer arithmetic).  The reference of the unit call is the numpy extraction
E_v (tests/ref_lut_many.py) followed by the CPU checker's keyswitch!; the bootstrap is held to the unit calls composed, to the three
identities of the header, and -- at the full CGGIparam and KMS2party sets -- to the checker chain's words and the thermometer's bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ref_lut as R
import ref_lut_many as RM
import edge_cases as EC
from helpers import ROOT, edge_words, gpu_scheme, keygen, ks_at_edge_check, ks_expected, ks_ran, mk, oracle_scheme
from test_gpu_lut import _dk, _exact_scheme, _gpu, _host, _inputs, _keys, _sid, _tables
from test_gpu_parity import SMALL
from test_keyswitch_at_cpu import checker_at, thermometer_bits, thermometer_case, thermometer_coefs

pytestmark = pytest.mark.gpu

NACC = 5


# ---- 1: the unit call against numpy extraction + the checker's key switch ----
def _acc(p, rng, nacc=NACC):
    """random words with the edge words at both ends and in the middle of every polynomial (helpers.edge_words): (nacc, 1 + k, N) uint64"""
    return np.stack([np.stack([edge_words(p.W, p.N, rng) for _ in range(p.k + 1)]) for _ in range(nacc)])


def _coefs(p):
    """the sign boundary j = v at both ends, the first and last word, the block schemes' copy / switch border n, the middle"""
    return sorted({v for v in (0, 1, p.n - 1, p.n, p.n + 1, p.N // 2, p.N - 1) if 0 <= v < p.N})


def _rows(p, B, rng, nacc=NACC):
    """-> (src, coef) of B output rows: src unsorted with repeats, row 0 and the last row among them; coef cycling through _coefs"""
    src = rng.integers(0, nacc, B).astype(np.uint32)
    if B >= 3:
        src[:3] = [nacc - 1, 0, nacc - 1]
    cs = _coefs(p)
    coef = np.array([cs[(g + 1) % len(cs)] for g in range(B)], dtype=np.uint32)
    return src, coef


def _unit_want(so, p, acc, src, coef):
    return np.stack([so.keyswitch(RM.extract(acc[int(src[g])], int(coef[g]), p.W)) for g in range(len(src))])


def _unit_check(p, so, sg, rng, batches=(1, 33), device=True, after=None):
    """after(B): called behind each key switch at a coefficient of the batch loop (the route children read which kernel it ran)"""
    acc = _acc(p, rng)
    a = acc.astype(p.ring_dtype)
    checks = 0
    for B in batches:
        src, coef = _rows(p, B, rng)
        want = _unit_want(so, p, acc, src, coef)
        assert np.array_equal(mk.keyswitch_at(sg, a, src, coef), want), ("host memory", _sid(p), B)
        if after:
            after(B)
        if device:
            assert np.array_equal(_host(mk.keyswitch_at(sg, _gpu(a), _gpu(src), _gpu(coef)), np.uint32), want), ("device memory", _sid(p), B)
        checks += B
    # the NULL forms: both = keyswitch!, src alone = keyswitch! of the named rows, coef alone = row g at coef[g]
    plain = sg.keyswitch(a)
    assert np.array_equal(mk.keyswitch_at(sg, a), plain), ("src = coef = NULL", _sid(p))
    src, coef = _rows(p, 7, rng)
    assert np.array_equal(mk.keyswitch_at(sg, a, src), plain[src]), ("coef = NULL", _sid(p))
    assert np.array_equal(mk.keyswitch_at(sg, a, coef=coef[:NACC]), _unit_want(so, p, acc, np.arange(NACC), coef[:NACC])), ("src = NULL", _sid(p))
    return checks + 2 * NACC + 7


@pytest.mark.parametrize("p", SMALL, ids=_sid)
def test_unit_call_equals_extraction_then_the_checkers_keyswitch(require_gpu, p):
    """every set of SMALL: all five schemes, both flavours of the block copy rule, LMSS with n > N, and -- the sets with f = 5 / f = 4,
    logD = 3 -- the per-digit kernel in process (the digit-pair route takes logD = 2 with an even f only)"""
    crs, keys = _keys(p)
    _unit_check(p, oracle_scheme(p, crs, keys), gpu_scheme(p, crs, keys), np.random.default_rng(p.N + p.n))


def test_small_sets_reach_both_routes_and_both_copy_rules():
    per_digit = [p for p in SMALL if p.logD != 2 or p.f % 2]
    assert per_digit and any(p.scheme == mk.LMSS for p in per_digit) and any(p.scheme == mk.CGGI for p in per_digit)
    assert any(p.scheme == mk.LMSS and p.n > p.N for p in SMALL) and any(p.scheme == mk.KMS_BLOCK for p in SMALL)
    assert {p.scheme for p in SMALL} == {mk.CGGI, mk.LMSS, mk.CCS, mk.KMS, mk.KMS_BLOCK}


# ---- 2: every key-switch route: the launcher switches are read once per process, so one child process per setting, one at a time ----
# (the older kernels run where the matrix cores do not: their settings name MKT_KS_MFMA = 0; the last child forces the matrix cores.  Each child
# reports which kernel its key switches ran and the parent holds the report to helpers.ks_expected)
KS_SETTINGS = [{**e, "MKT_KS_MFMA": "0"} for e in ({"MKT_KS_PAIR": "0"}, {"MKT_KS_G": "8"}, {"MKT_KS_G": "16"}, {"MKT_KS_WAVES": "1"})] + [{"MKT_KS_MFMA": "1"}]
CHILD_BATCHES = (1, 33, 70)
CHILD_SETS = [mk.CGGIparam.scaled(n=20, N=256), mk.Blockparam.scaled(n=30, N=256, blk_d=10)]
CHILD_TIMEOUT = 120
_child_fault = []          # a child that died by a signal / abort / segfault / time limit: no further child is started


@pytest.mark.parametrize("setting", KS_SETTINGS, ids=lambda v: "-".join(f"{k[4:]}{x}" for k, x in v.items()))
def test_key_switch_route_in_a_child_process(require_gpu, setting):
    assert not _child_fault, f"an earlier child process faulted: {_child_fault}"
    env = {k: v for k, v in os.environ.items() if not k.startswith("MKT_") or k == "MKT_LIB_PATH"}
    env.update(setting)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _child_fault.append((setting, "time limit"))
        raise
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137):
        _child_fault.append((setting, r.returncode))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, f"child {setting}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    j = json.loads(lines[-1])
    assert j["ok"] and j["checks"] > 0 and j["env"] == setting, j
    assert sorted(j["ran"]) == sorted(f"{i}:{B}" for i in range(len(CHILD_SETS)) for B in CHILD_BATCHES + ("edges",)), sorted(j["ran"])
    for key, seen in j["ran"].items():
        want = ks_expected(CHILD_SETS[int(key.split(":")[0])], setting)
        assert tuple(seen) == want, (setting, key, "ran (kernel, G, waves)", seen, "implied", want)


def _child():
    """-> (checks, {"<position in CHILD_SETS>:<batch, or edges>": the (kernel, G, waves) that key switch ran})"""
    rng = np.random.default_rng(97)
    checks, ran = 0, {}
    for i, p in enumerate(CHILD_SETS):
        crs, keys = keygen(p, 92)
        sg = gpu_scheme(p, crs, keys)
        so = oracle_scheme(p, crs, keys)
        checks += _unit_check(p, so, sg, rng, batches=CHILD_BATCHES, after=lambda B: ran.__setitem__(f"{i}:{B}", ks_ran(sg)))
        # the accumulators of tests/test_gpu_edges.py on the key-switch digits' boundaries, rotated by X^v and read back at v
        assert p in EC.KS_CHILD_SETS                                           # (tests/test_edges_cpu.py proves their classes for these sets)
        checks += ks_at_edge_check(p, so, sg, rng, EC.KS_BATCHES, EC.KS_AT_COEFS(p))
        ran[f"{i}:edges"] = ks_ran(sg)
        sg.close()
    return checks, ran


# ---- 3: the bootstrap against the unit calls composed, and the three identities ----
def _composed(sx, luts, c, coef, nu, sel):
    at, acc = mk.lut_many_testvector(sx, luts, c, 1 << nu, sel)
    acc = sx.blindrotate_(at, acc)
    B, nc = len(c), len(coef)
    src = (np.arange(B * nc) // nc).astype(np.uint32)
    return mk.keyswitch_at(sx, acc, src, np.tile(np.asarray(coef, dtype=np.uint32), B)).reshape(B, nc, -1)


def _eleven(p, rng):
    """11 coefficients: no power of two, beyond 8, unsorted, one repeated"""
    cf = rng.permutation(p.N)[:10].astype(np.uint32)
    cf[3] = p.N - 1
    return np.concatenate([cf, cf[:1]])


def _bootstrap_check(sx, p, c, luts, sel, rng, o, what):
    nu = RM.nu_of(o)
    packed = np.stack([mk.lut_pack(_tables(p, o, rng), p) for _ in range(len(luts))])
    got = mk.lut_bootstrap_at(sx, packed, c, np.arange(o, dtype=np.uint32), nu=nu, sel=sel)
    assert got.shape == (len(c), o, p.lwe_len)
    assert np.array_equal(got, mk.lut_many_bootstrap(sx, packed, c, o, sel)), (what, "coef = range(o) is the many-table bootstrap", o, _sid(p))
    assert np.array_equal(got, _composed(sx, packed, c, range(o), nu, sel)), (what, "composed", o, _sid(p))
    assert np.array_equal(mk.lut_bootstrap_at(sx, luts, c, [0], sel=sel)[:, 0], mk.lut_bootstrap(sx, luts, c, sel)), (what, "nu = 0, coef = [0] is lut_bootstrap", _sid(p))
    cf = _eleven(p, rng)
    for nu11 in (0, 1):
        got = mk.lut_bootstrap_at(sx, luts, c, cf, nu=nu11, sel=sel)
        assert np.array_equal(got, _composed(sx, luts, c, cf, nu11, sel)), (what, "eleven coefficients", nu11, _sid(p))
    assert np.array_equal(_host(mk.lut_bootstrap_at(sx, _gpu(luts), _gpu(c), _gpu(cf), nu=1, sel=_gpu(sel)), np.uint32), got), (what, "device memory", _sid(p))
    return got


@pytest.mark.parametrize("p", SMALL, ids=_sid)
def test_bootstrap_at_equals_the_composed_calls_and_its_identities(require_gpu, p):
    crs, keys = _keys(p)
    rng = np.random.default_rng(17)
    B, nluts = 3, 2
    c = _inputs(p, keys, B, rng)
    luts = _tables(p, nluts, rng)
    sel = np.array([1, 0, 1], dtype=np.uint32)
    o = (2, 8)[SMALL.index(p) % 2]
    sg = gpu_scheme(p, crs, keys)
    _bootstrap_check(sg, p, c, luts, sel, np.random.default_rng(18), o, "F64REF")
    sg.close()
    sx = _exact_scheme(p, crs, keys)
    if sx is not None:
        words = []
        for impl in (0, 1):
            sx.set_option("exact_impl", impl)
            words.append(_bootstrap_check(sx, p, c, luts, sel, np.random.default_rng(18), o, f"EXACT impl {impl}"))
        assert np.array_equal(words[0], words[1]), "EXACT: both implementations give the same words"
        sx.close()


# ---- 4: the chunk edge ----
def test_one_input_past_a_chunk_equals_two_calls(require_gpu):
    """a call is cut into chunks of 8192 // ncoef inputs: 8192 // 3 + 1 inputs in one call and as 2730 + 1"""
    p, nc = mk.CGGIparam.scaled(n=8, N=64), 3
    crs, keys = _keys(p)
    rng = np.random.default_rng(62)
    B = 8192 // nc + 1
    sg = gpu_scheme(p, crs, keys)
    luts, cf = _gpu(_tables(p, 3, rng)), _gpu(np.array([5, 63, 0], dtype=np.uint32))
    c = _gpu(rng.integers(0, 1 << 32, (B, p.lwe_len), dtype=np.uint64).astype(np.uint32))       # any words are an input
    sel = _gpu(rng.integers(0, 3, B).astype(np.uint32))
    whole = _host(mk.lut_bootstrap_at(sg, luts, c, cf, sel=sel), np.uint32)
    a = _host(mk.lut_bootstrap_at(sg, luts, c[:B - 1], cf, sel=sel[:B - 1]), np.uint32)
    b = _host(mk.lut_bootstrap_at(sg, luts, c[B - 1:], cf, sel=sel[B - 1:]), np.uint32)
    assert whole.shape == (B, nc, p.lwe_len) and np.array_equal(whole[:B - 1], a) and np.array_equal(whole[B - 1:], b)
    sg.close()


# ---- 5: the gather front end ----
@pytest.mark.parametrize("p", [mk.CGGIparam.scaled(n=20, N=256), mk.KMS2party.scaled(n=16, N=256), mk.CCS2party.scaled(n=12, N=256)], ids=_sid)
def test_gather_is_the_linear_combination_then_the_bootstrap(require_gpu, p):
    crs, keys = _keys(p)
    rng = np.random.default_rng(33)
    P, B, nluts = 6, 7, 3
    cf = np.array([7, 0, p.N - 1, 7, p.N // 2], dtype=np.uint32)
    nc = len(cf)
    sg = gpu_scheme(p, crs, keys)
    pool = _inputs(p, keys, P, rng)
    luts = _tables(p, nluts, rng)
    sel = rng.integers(0, nluts, B).astype(np.uint32)
    idx = rng.integers(0, P, (B, 4)).astype(np.uint32)
    wt = rng.integers(-4, 5, (B, 4)).astype(np.int8)
    wt[0] = [1, 2, 4, 0]; wt[1] = [0, 0, 0, 0]; wt[2] = [-128, 127, -1, 1]
    cst = rng.integers(0, 1 << 32, B, dtype=np.uint64).astype(np.uint32)
    for nu in (0, 2):
        want = mk.lut_bootstrap_at(sg, luts, R.linear(pool, idx, wt, cst), cf, nu=nu, sel=sel)
        out = np.full((B, nc, p.lwe_len), 0xA5A5A5A5, dtype=np.uint32)
        assert mk.lut_gather_at(sg, luts, sel, pool, idx, wt, cst, cf, out, nu=nu) is out and np.array_equal(out, want), ("host memory", nu)
    import torch
    big = torch.cat([_gpu(pool), torch.zeros((B * nc, p.lwe_len), dtype=torch.int32, device="cuda")])
    mk.lut_gather_at(sg, _gpu(luts), _gpu(sel), big[:P], _gpu(idx), _gpu(wt), _gpu(cst), _gpu(cf), big[P:], nu=2)
    assert np.array_equal(_host(big[P:], np.uint32).reshape(want.shape), want), "device memory, out a later region of the pool"
    assert np.array_equal(_host(big[:P], np.uint32), pool), "the pool rows are untouched"
    sentinel = np.full((B, nc, p.lwe_len), 0x5A5A5A5A, dtype=np.uint32)
    bad_sel = sel.copy(); bad_sel[0] = nluts
    bad_idx = idx.copy(); bad_idx[3, 1] = P
    for args in ((luts, bad_sel, pool, idx, wt, cst), (luts, sel, pool, bad_idx, wt, cst), (luts[:0], None, pool, idx, wt, cst), (luts, sel, pool[:0], idx, wt, cst)):
        out = sentinel.copy()
        with pytest.raises(mk.MktError) as e:
            mk.lut_gather_at(sg, *args, cf, out)
        assert e.value.code == -1 and np.array_equal(out, sentinel)
    sg.close()


# ---- 6: sharded ----
@pytest.mark.parametrize("flags", [{}, {"private_keys": True}, {"stage_always": True}], ids=lambda f: "-".join(f) or "plain")
@pytest.mark.parametrize("p", [mk.CGGIparam.scaled(n=20, N=256), mk.KMS2party.scaled(n=16, N=256)], ids=_sid)
def test_two_logical_shards_give_the_single_context_words(require_gpu, p, flags):
    crs, keys = _keys(p)
    rng = np.random.default_rng(43)
    sg = gpu_scheme(p, crs, keys)
    multi = mk.setup_multi(p, [0, 0], keys=keys if p.multikey else keys[0], a=crs, **flags)
    B = 5                                                                      # ragged: 3 + 2 inputs, 15 + 10 output rows
    cf = np.array([9, 0, 200, 9, 255], dtype=np.uint32)
    luts = _tables(p, 3, rng)
    c = _inputs(p, keys, B, rng, seed=900)
    sel = rng.integers(0, 3, B).astype(np.uint32)
    want = mk.lut_bootstrap_at(sg, luts, c, cf, nu=1, sel=sel)
    assert np.array_equal(mk.lut_bootstrap_at(multi, luts, c, cf, nu=1, sel=sel), want), "host memory"
    assert np.array_equal(_host(mk.lut_bootstrap_at(multi, _gpu(luts), _gpu(c), _gpu(cf), nu=1, sel=_gpu(sel)), np.uint32), want), "device memory"
    assert np.array_equal(mk.lut_bootstrap_at(multi, luts[1], c[:1], cf[:2]), mk.lut_bootstrap_at(sg, luts[1], c[:1], cf[:2])), "fewer inputs than shards"
    sentinel = np.full((B, len(cf), p.lwe_len), 0x5A5A5A5A, dtype=np.uint32)
    out = sentinel.copy()
    with pytest.raises(mk.MktError) as e:
        mk.lut_bootstrap_at(multi, luts, c, cf, sel=np.full(B, 3, np.uint32), out=out)
    assert e.value.code == -1 and np.array_equal(out, sentinel)
    multi.close(); sg.close()


# ---- 7: the thermometer at the full sets ----
@pytest.mark.parametrize("name", R.CHAIN_SETS)
def test_thermometer_bits_in_one_rotation(require_gpu, name):
    """P = 8, fresh inputs m = 0 .. 7 at phase m/16 + 1/32: the 64 outputs are the checker chain's words and decrypt to [m >= w].  The margin
    1/32 is more than 12 sigma of a fresh input's mod-switched phase, so a wrong bit is a bug, not noise"""
    p, crs, keys, c, words = thermometer_case(name)
    sg = gpu_scheme(p, crs, keys)
    cf = mk.lut_threshold_coefs(8, p)
    assert list(cf) == thermometer_coefs(8, p.N)
    out = mk.lut_bootstrap_at(sg, mk.sign_lut(p), np.array(c), cf)
    assert np.array_equal(out, words), "the checker chain's words"
    assert np.array_equal(mk.lwe_decrypt(out, _dk(p, keys), p), thermometer_bits()), "all 64 thermometer bits"
    sg.close()


# ---- 8: arguments ----
def _raw(sg, name, *args):
    """the C entry point itself: the Python layer refuses most of these calls before the library sees them"""
    from mktfhe_amd import _lib
    return getattr(_lib.lib(), name)(sg.h, *args)


def test_a_context_whose_first_table_call_is_bootstrap_at(require_gpu):
    p = mk.CGGIparam.scaled(n=20, N=256)
    crs, keys = keygen(p, 7)
    so, sg = oracle_scheme(p, crs, keys), gpu_scheme(p, crs, keys)
    rng = np.random.default_rng(8)
    c = _inputs(p, keys, 2, rng)
    T = _tables(p, 1, rng)[0]
    cf = [3, 250]
    got = mk.lut_bootstrap_at(sg, T, c, cf)
    assert np.array_equal(got, np.stack([checker_at(so, T, c[j], cf, p.W) for j in range(2)]))
    sg.close()


def test_refusals_clamps_empty_batches_overlap_and_forks(require_gpu):
    import ctypes as C
    import threading
    import torch
    from mktfhe_amd import _lib
    from mktfhe_amd.scheme import MEM_DEVICE, MEM_HOST, _np_ptr
    p = mk.KMS2party.scaled(n=16, N=256)
    crs, keys = _keys(p)
    rng = np.random.default_rng(53)
    so, sg = oracle_scheme(p, crs, keys), gpu_scheme(p, crs, keys)
    B, N = 6, p.N
    acc = _acc(p, rng)
    a = acc.astype(p.ring_dtype)
    src, coef = _rows(p, B, rng)
    want = _unit_want(so, p, acc, src, coef)
    canary = np.full((B, p.lwe_len), 0x5A5A5A5A, dtype=np.uint32)
    err = lambda: _lib.lib().mkt_last_error(sg.h)                       # noqa: E731

    def ks_at(accp, nacc, s, cf, out, rows, mem=MEM_HOST):
        return _raw(sg, "mkt_keyswitch_at_batch", accp, nacc, s, cf, out, rows, mem)

    # host memory: an index out of range, no accumulator, src NULL with nacc != B -- MKT_ERR_ARG, out untouched
    bad_src = src.copy(); bad_src[2] = NACC
    bad_coef = coef.copy(); bad_coef[4] = N
    for s, cf, nacc, rows in ((bad_src, coef, NACC, B), (src, bad_coef, NACC, B), (src, coef, 0, B), (None, coef, NACC, B), (None, None, NACC, B)):
        out = canary.copy()
        rc = ks_at(_np_ptr(a), nacc, None if s is None else _np_ptr(s), None if cf is None else _np_ptr(cf), _np_ptr(out), rows)
        assert rc == -1 and err() and np.array_equal(out, canary), (nacc, rows)
    assert ks_at(_np_ptr(a), 0, None, None, _np_ptr(canary.copy()), 0) == 0 and ks_at(_np_ptr(a), NACC, _np_ptr(src), None, _np_ptr(canary.copy()), 0) == 0, "B = 0 succeeds"
    assert mk.keyswitch_at(sg, a, src[:0], coef[:0]).shape == (0, p.lwe_len)
    # device memory: the same refusals that do not need the values; src clamped to the last row, coef read mod N
    da, dsrc, dcoef = _gpu(a), _gpu(bad_src), _gpu((coef + np.uint32(N) * np.arange(B, dtype=np.uint32)).astype(np.uint32))
    dout = _gpu(canary)
    vp = lambda t: C.c_void_p(t.data_ptr())                             # noqa: E731
    assert ks_at(vp(da), 0, vp(dsrc), vp(dcoef), vp(dout), B, MEM_DEVICE) == -1 and ks_at(vp(da), NACC, None, vp(dcoef), vp(dout), B, MEM_DEVICE) == -1
    torch.cuda.synchronize()
    assert np.array_equal(_host(dout, np.uint32), canary)
    clamped = bad_src.copy(); clamped[2] = NACC - 1
    assert np.array_equal(_host(mk.keyswitch_at(sg, da, dsrc, dcoef), np.uint32), _unit_want(so, p, acc, clamped, coef)), "device clamps"

    # the bootstrap: refusals in host memory leave out untouched
    c = _inputs(p, keys, 4, rng)
    luts = _tables(p, 2, rng)
    sel = np.array([1, 0, 1, 0], dtype=np.uint32)
    cf = np.array([1, 255, 17], dtype=np.uint32)
    want_b = mk.lut_bootstrap_at(sg, luts, c, cf, nu=1, sel=sel)
    can_b = np.full((4, 3, p.lwe_len), 0x5A5A5A5A, dtype=np.uint32)

    def bs_at(nu, cfa, ncoef, sela=sel, nluts=2, rows=4):
        out = can_b.copy()
        rc = _raw(sg, "mkt_lut_bootstrap_at_batch", _np_ptr(luts), nluts, _np_ptr(sela), _np_ptr(c), nu, _np_ptr(cfa), ncoef, _np_ptr(out), rows, MEM_HOST)
        return rc, out

    for args in ((4, cf, 3), (-1, cf, 3), (0, cf, 0), (0, np.zeros(N + 1, np.uint32), N + 1), (0, np.array([1, N, 17], np.uint32), 3),
                 (0, cf, 3, np.array([1, 0, 2, 0], np.uint32)), (0, cf, 3, sel, 0)):
        rc, out = bs_at(*args)
        assert rc == -1 and err() and np.array_equal(out, can_b), args[:1] + args[2:3]
    assert bs_at(0, cf, 3, rows=0)[0] == 0 and mk.lut_bootstrap_at(sg, luts, c[:0], cf).shape == (0, 3, p.lwe_len)
    # device memory: sel clamped, coef mod N; out overlapping lwe refused when ncoef > 1, served when ncoef == 1 (in place)
    got = mk.lut_bootstrap_at(sg, _gpu(luts), _gpu(c), _gpu(cf + np.uint32(3 * N)), nu=1, sel=_gpu(sel + np.uint32(2) * sel))
    assert np.array_equal(_host(got, np.uint32), want_b), "device clamps"
    buf = torch.zeros((16, p.lwe_len), dtype=torch.int32, device="cuda")
    buf[:4] = _gpu(c)
    dl, dsel, dcf = _gpu(luts), _gpu(sel), _gpu(cf)
    for out in (buf[:12], buf[3:15]):
        rc = _raw(sg, "mkt_lut_bootstrap_at_batch", vp(dl), 2, vp(dsel), vp(buf), 1, vp(dcf), 3, vp(out), 4, MEM_DEVICE)
        assert rc == -1 and b"overlap" in err()
    torch.cuda.synchronize()
    assert np.array_equal(_host(buf[:4], np.uint32), c) and not _host(buf[4:], np.uint32).any()
    mk.lut_bootstrap_at(sg, dl, buf[:4], dcf, nu=1, sel=dsel, out=buf[4:])     # adjacent, not overlapping: served
    assert np.array_equal(_host(buf[4:], np.uint32).reshape(want_b.shape), want_b)
    inplace = _gpu(c)
    mk.lut_bootstrap_at(sg, dl, inplace, dcf[1:2], nu=1, sel=dsel, out=inplace)
    assert np.array_equal(_host(inplace, np.uint32), want_b[:, 1]), "ncoef = 1 may run in place"

    # a fork gives the parent's words, also while the parent runs: each holds its own workspace and row table
    f = sg.fork()
    got = {}

    def run(name, s):
        got[name] = [mk.lut_bootstrap_at(s, luts, c, cf, nu=1, sel=sel) for _ in range(3)] + [mk.keyswitch_at(s, a, src, coef)]

    threads = [threading.Thread(target=run, args=("parent", sg)), threading.Thread(target=run, args=("fork", f))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert len(got) == 2 and all(np.array_equal(w, want_b) for name in got for w in got[name][:3]) and all(np.array_equal(got[name][3], want) for name in got)
    f.close(); sg.close()


if __name__ == "__main__":
    assert sys.argv[1:] == ["child"]
    n, ran = _child()
    print(json.dumps({"ok": True, "checks": n, "ran": ran, "env": {k: v for k, v in os.environ.items() if k.startswith("MKT_") and k != "MKT_LIB_PATH"}}))
