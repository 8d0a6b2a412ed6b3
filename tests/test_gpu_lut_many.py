"""Many-table bootstrap on the GPU (mktfhe.h "many-table bootstrap", mktfhe_amd/lut.py), word for word (tolerance 0) unless a
test says otherwise: the coarse switch and table step and the extraction against their numpy restatements (tests/ref_lut_many.py), the
whole call against the unit calls composed and against the CPU checker's chain, every scheme and both arithmetic modes, forced kernels,
the chunk boundary, the gather front end, logical shards, recipe (a), the argument edges, and the context's (row, coefficient) table across
calls and forks.  The bootstrap makes no copies E_v(acc): the composition of the unit calls (lut_many_testvector, blindrotate_, lut_extract,
the plain keyswitch) is its independent check -- test_small_sets_equal_the_composed_calls_and_the_checker reaches o = 2, 4, 8 on the 32-bit
ring (SMALL[0], [1], [2]) and on the 64-bit ring (SMALL[3], [4], [5]), where E_v negates the wrapped words before the truncation."""
import threading

import numpy as np
import pytest

import ref_lut as R
import ref_lut_many as RM
from helpers import gpu_scheme, mk, oracle_scheme
from test_gpu_lut import SWITCH_CASES, _dk, _exact_scheme, _gpu, _host, _inputs, _keys, _sid, _tables
from test_gpu_parity import FULL, SMALL
from test_lut_many_cpu import adder_case

pytestmark = pytest.mark.gpu

UNIT_SHAPES = [mk.CGGIparam.scaled(n=8, N=64), mk.CGGIparam.scaled(n=8, N=256, W=64), mk.CGGIparam.scaled(n=6, N=1024, k=2)]


def _odd(t):
    """the same device words one word past a 16-byte boundary: the word-by-word kernels"""
    import torch
    o = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")[1:].view(t.shape)
    o.copy_(t)
    assert o.data_ptr() % 16
    return o


def _packed(p, nluts, o, rng):
    """-> (tables (nluts, o, N), their packed forms (nluts, N))"""
    tabs = np.stack([_tables(p, o, rng) for _ in range(nluts)])
    return tabs, np.stack([mk.lut_pack(t, p) for t in tabs])


# ---- 1: the coarse switch and the table step ----
@pytest.mark.parametrize("nluts", [1, 5])
@pytest.mark.parametrize("o", [2, 8])
@pytest.mark.parametrize("p", UNIT_SHAPES, ids=_sid)
def test_testvector_and_coarse_switch_equal_numpy(require_gpu, p, o, nluts):
    rng = np.random.default_rng(p.N + 10 * o + nluts)
    sg = mk.Scheme(p)                                        # no keys: neither step needs one
    words = RM.sw_edge_words(p.N, o) + [int(w) for w in rng.integers(0, 1 << 32, 5)]
    B = len(words)
    lwe = np.array([[words[(j + 3 * c) % B] for c in range(p.lwe_len - 1)] + [words[j]] for j in range(B)], dtype=np.uint64).astype(np.uint32)
    assert {0, o, p.N, 2 * p.N - o, 2 * p.N} <= {RM.sw(w, p.N, o) for w in words}
    luts = _tables(p, nluts, rng)
    sel = rng.integers(0, nluts, B).astype(np.uint32)
    sel[0], sel[1] = 0, nluts - 1
    rows = [RM.sw_row(lwe[j], p.N, o) for j in range(B)]
    want_at = np.stack([r[0] for r in rows])
    want = np.stack([R.testvector(luts[sel[j]], rows[j][1], p.W, p.k) for j in range(B)])

    def check(got, what):
        at, acc = got
        at, acc = (at, acc) if isinstance(at, np.ndarray) else (_host(at, np.uint32), _host(acc, p.ring_dtype))
        assert np.array_equal(at, want_at), (what, "atilde")
        assert np.array_equal(acc.astype(np.uint64), want), (what, "acc")

    check(mk.lut_many_testvector(sg, luts, lwe, o, sel), "host memory")
    check(mk.lut_many_testvector(sg, _gpu(luts), _gpu(lwe), o, _gpu(sel)), "device memory")
    check(mk.lut_many_testvector(sg, _odd(_gpu(luts)), _gpu(lwe), o, _gpu(sel)), "unaligned tables")
    at0, acc0 = mk.lut_many_testvector(sg, luts[0], lwe, o)                     # no selector, a single (N,) table
    assert np.array_equal(at0, want_at) and np.array_equal(acc0.astype(np.uint64), np.stack([R.testvector(luts[0], rows[j][1], p.W, p.k) for j in range(B)]))
    # nout = 1 is the plain table step and mkt_modswitch_batch
    at1, acc1 = mk.lut_many_testvector(sg, luts, lwe, 1, sel)
    assert np.array_equal(acc1, mk.lut_testvector(sg, luts, lwe, sel)) and np.array_equal(at1, sg.modswitch(lwe)[0])
    sg.close()


# ---- 2: the extraction ----
def _acc_words(p, B, rng):
    """random words in all 1 + k polynomials, with 0, 1 and 2^(W-1) at both ends of each (where the sign flips)"""
    a = _tables(p, B * (p.k + 1), rng).reshape(B, p.k + 1, p.N)
    edge = np.array([0, 1, 1 << (p.W - 1)], dtype=np.uint64).astype(p.ring_dtype)
    a[..., :3], a[..., -3:] = edge, edge[::-1]
    return a


@pytest.mark.parametrize("o", RM.NOUT)
@pytest.mark.parametrize("p", UNIT_SHAPES + [mk.KMS2party.scaled(n=4, N=128)], ids=_sid)
def test_extract_equals_numpy(require_gpu, p, o):
    assert UNIT_SHAPES[2].k == 2 and (p.name != "KMS2party" or (p.k == 2 and p.W == 64))
    rng = np.random.default_rng(p.N + o)
    sg = mk.Scheme(p)
    for B in (1, 5):
        acc = _acc_words(p, B, rng)
        want = RM.extract_all(acc, o, p.W)
        got = mk.lut_extract(sg, acc, o)
        assert got.shape == (B, o, p.k + 1, p.N) and np.array_equal(got.astype(np.uint64), want), ("host memory", B)
        assert np.array_equal(_host(mk.lut_extract(sg, _gpu(acc), o), p.ring_dtype).astype(np.uint64), want), ("device memory", B)
        assert np.array_equal(_host(mk.lut_extract(sg, _odd(_gpu(acc)), o), p.ring_dtype).astype(np.uint64), want), ("unaligned accumulators", B)
    sg.close()


def test_extract_beyond_one_grid_of_workgroups(require_gpu):
    """one workgroup per ciphertext up to 65536, the rest by grid stride"""
    p, o, B = UNIT_SHAPES[0], 2, 65536 + 3
    rng = np.random.default_rng(3)
    sg = mk.Scheme(p)
    acc = rng.integers(0, 1 << 32, (B, p.k + 1, p.N), dtype=np.uint64).astype(np.uint32)
    got = _host(mk.lut_extract(sg, _gpu(acc), o), np.uint32)
    assert np.array_equal(got, RM.extract_all(acc, o, p.W).astype(np.uint32))
    sg.close()


# ---- 3 and 4: the whole call against the unit calls composed and against the checker's chain ----
def _composed(sx, U, c, o, sel):
    at, acc = mk.lut_many_testvector(sx, U, c, o, sel)
    accs = mk.lut_extract(sx, sx.blindrotate_(at, acc), o)
    return sx.keyswitch(accs)


def _sign_tables(p, o, rng):
    """o tables whose every entry is +-2^(W-3): whatever the phase, an output is a gate bit"""
    e = 1 << (p.W - 3)
    return np.where(rng.integers(0, 2, (o, p.N)).astype(bool), e, (1 << p.W) - e).astype(p.ring_dtype)


def _pre_rounded(c, p, o):
    """every word on the coarse grid, back at 32 bits: sw_nu(w) 2^(32 - logN - 1) (2N wraps to 0: both are the identity)"""
    bit0 = 32 - (p.N.bit_length() - 1) - 1
    return np.array([[(RM.sw(w, p.N, o) << bit0) & 0xFFFFFFFF for w in row] for row in c], dtype=np.uint32)


def _many_check(p, B, seed, o, oracle=True):
    crs, keys = _keys(p)
    rng = np.random.default_rng(seed)
    c = _inputs(p, keys, B, rng)
    nluts = 2
    tabs, U = _packed(p, nluts, o, rng)
    sel = (np.arange(B) % nluts).astype(np.uint32)[::-1].copy()
    sg = gpu_scheme(p, crs, keys)
    ref = _composed(sg, U, c, o, sel)
    assert ref.shape == (B, o, p.lwe_len)
    if oracle:
        so = oracle_scheme(p, crs, keys)
        assert np.array_equal(ref, np.stack([RM.checker_many(so, U[sel[j]], c[j], o, p.W) for j in range(B)])), ("the checker's chain", _sid(p))
    assert np.array_equal(mk.lut_many_bootstrap(sg, U, c, o, sel), ref), ("host memory", _sid(p))
    assert np.array_equal(_host(mk.lut_many_bootstrap(sg, _gpu(U), _gpu(c), o, _gpu(sel)), np.uint32), ref), ("device memory", _sid(p))
    assert np.array_equal(mk.lut_many_bootstrap(sg, U, c, 1, sel)[:, 0], mk.lut_bootstrap(sg, U, c, sel)), "nout = 1 is lut_bootstrap"
    if oracle:
        # the packed form against the single-table one.  The two rotate DIFFERENT polynomials (U, T_v), so their noise differs and the words
        # cannot agree; what is exact is the mod-switched phase -- integer arithmetic on the same rounded words -- hence the table entry both
        # read.  With entries +-2^(W-3) each output is a gate bit, 1/8 from the decision boundary like every gate of this suite: the bits agree
        signs = _sign_tables(p, o, rng)
        got = mk.lut_many_bootstrap(sg, mk.lut_pack(signs, p), c, o)
        cr = _pre_rounded(c, p, o)
        for v in range(o):
            one = mk.lut_bootstrap(sg, signs[v], cr)
            assert np.array_equal(mk.lwe_decrypt(got[:, v], _dk(p, keys), p), mk.lwe_decrypt(one, _dk(p, keys), p)), ("single table on pre-rounded words", v, _sid(p))
    sg.close()
    sx = _exact_scheme(p, crs, keys)
    if sx is not None:
        words = []
        for impl in (0, 1):
            sx.set_option("exact_impl", impl)
            got = mk.lut_many_bootstrap(sx, U, c, o, sel)
            assert np.array_equal(got, _composed(sx, U, c, o, sel)), ("EXACT", impl, _sid(p))
            assert np.array_equal(mk.lut_many_bootstrap(sx, U, c, 1, sel)[:, 0], mk.lut_bootstrap(sx, U, c, sel)), ("EXACT, nout = 1", impl)
            words.append(got)
        assert np.array_equal(words[0], words[1]), "EXACT: both implementations give the same words"
        sx.close()


@pytest.mark.parametrize("p", SMALL, ids=_sid)
def test_small_sets_equal_the_composed_calls_and_the_checker(require_gpu, p):
    _many_check(p, B=3, seed=13, o=(2, 4, 8)[SMALL.index(p) % 3])


@pytest.mark.parametrize("p", FULL, ids=lambda p: p.name)
def test_full_sets_equal_the_composed_calls(require_gpu, p):
    _many_check(p, B=2, seed=14, o=2, oracle=False)


# ---- 5: forced kernels ----
@pytest.mark.parametrize("p, opt, values", SWITCH_CASES, ids=lambda v: _sid(v) if isinstance(v, mk.Params) else str(v))
def test_forced_kernels_give_identical_words(require_gpu, p, opt, values):
    crs, keys = _keys(p)
    rng = np.random.default_rng(22)
    B, o = 3, 4
    c = _inputs(p, keys, B, rng)
    _, U = _packed(p, 2, o, rng)
    sel = (np.arange(B) % 2).astype(np.uint32)
    so = oracle_scheme(p, crs, keys)
    ref = np.stack([RM.checker_many(so, U[sel[j]], c[j], o, p.W) for j in range(B)])
    sg = gpu_scheme(p, crs, keys)
    names = set()
    for v in values:
        sg.set_option(opt, v)
        assert np.array_equal(mk.lut_many_bootstrap(sg, U, c, o, sel), ref), (opt, v)
        names.add(sg.last_kernel_name())
    assert names and "" not in names
    sg.close()


# ---- 6: the chunk boundary ----
def test_one_input_past_a_chunk_equals_two_calls(require_gpu):
    """a call is cut into chunks of 8192 / nout inputs: 8192 / 8 + 1 inputs in one call and as 1024 + 1"""
    p, o = mk.CGGIparam.scaled(n=8, N=64), 8
    crs, keys = _keys(p)
    rng = np.random.default_rng(61)
    B = 8192 // o + 1
    sg = gpu_scheme(p, crs, keys)
    _, U = _packed(p, 3, o, rng)
    c = _gpu(rng.integers(0, 1 << 32, (B, p.lwe_len), dtype=np.uint64).astype(np.uint32))       # any words are an input
    sel = _gpu(rng.integers(0, 3, B).astype(np.uint32))
    whole = _host(mk.lut_many_bootstrap(sg, _gpu(U), c, o, sel), np.uint32)
    a = _host(mk.lut_many_bootstrap(sg, _gpu(U), c[:B - 1], o, sel[:B - 1]), np.uint32)
    b = _host(mk.lut_many_bootstrap(sg, _gpu(U), c[B - 1:], o, sel[B - 1:]), np.uint32)
    assert whole.shape == (B, o, p.lwe_len) and np.array_equal(whole[:B - 1], a) and np.array_equal(whole[B - 1:], b)
    sg.close()


# ---- 7: the gather front end ----
@pytest.mark.parametrize("p", [mk.CGGIparam.scaled(n=20, N=256), mk.KMS2party.scaled(n=16, N=256), mk.CCS2party.scaled(n=12, N=256)], ids=_sid)
def test_gather_is_the_linear_combination_then_the_bootstrap(require_gpu, p):
    crs, keys = _keys(p)
    rng = np.random.default_rng(32)
    P, B, nluts, o = 6, 7, 3, 4
    sg = gpu_scheme(p, crs, keys)
    pool = _inputs(p, keys, P, rng)
    _, U = _packed(p, nluts, o, rng)
    sel = rng.integers(0, nluts, B).astype(np.uint32)
    idx = rng.integers(0, P, (B, 4)).astype(np.uint32)
    wt = rng.integers(-4, 5, (B, 4)).astype(np.int8)
    wt[0] = [1, 2, 4, 0]; wt[1] = [0, 0, 0, 0]; wt[2] = [-128, 127, -1, 1]
    cst = rng.integers(0, 1 << 32, B, dtype=np.uint64).astype(np.uint32)
    want = mk.lut_many_bootstrap(sg, U, R.linear(pool, idx, wt, cst), o, sel)
    out = np.full((B, o, p.lwe_len), 0xA5A5A5A5, dtype=np.uint32)
    assert mk.lut_many_gather(sg, U, sel, pool, idx, wt, cst, o, out) is out and np.array_equal(out, want), "host memory"
    import torch
    big = torch.cat([_gpu(pool), torch.zeros((B * o, p.lwe_len), dtype=torch.int32, device="cuda")])
    mk.lut_many_gather(sg, _gpu(U), _gpu(sel), big[:P], _gpu(idx), _gpu(wt), _gpu(cst), o, big[P:])
    assert np.array_equal(_host(big[P:], np.uint32).reshape(want.shape), want), "device memory, out a later region of the pool"
    assert np.array_equal(_host(big[:P], np.uint32), pool), "the pool rows are untouched"
    sentinel = np.full((B, o, p.lwe_len), 0x5A5A5A5A, dtype=np.uint32)
    bad_sel = sel.copy(); bad_sel[0] = nluts
    bad_idx = idx.copy(); bad_idx[3, 1] = P
    for args in ((U, bad_sel, pool, idx, wt, cst), (U, sel, pool, bad_idx, wt, cst), (U[:0], None, pool, idx, wt, cst), (U, sel, pool[:0], idx, wt, cst)):
        out = sentinel.copy()
        with pytest.raises(mk.MktError) as e:
            mk.lut_many_gather(sg, *args, o, out)
        assert e.value.code == -1 and np.array_equal(out, sentinel)
    sg.close()


# ---- 8: sharded ----
@pytest.mark.parametrize("flags", [{}, {"private_keys": True}, {"stage_always": True}], ids=lambda f: "-".join(f) or "plain")
@pytest.mark.parametrize("p", [mk.CGGIparam.scaled(n=20, N=256), mk.KMS2party.scaled(n=16, N=256)], ids=_sid)
def test_two_logical_shards_give_the_single_context_words(require_gpu, p, flags):
    crs, keys = _keys(p)
    rng = np.random.default_rng(42)
    sg = gpu_scheme(p, crs, keys)
    multi = mk.setup_multi(p, [0, 0], keys=keys if p.multikey else keys[0], a=crs, **flags)
    o, B = 4, 5                                                                # ragged: 3 + 2 inputs, 12 + 8 output rows
    _, U = _packed(p, 3, o, rng)
    c = _inputs(p, keys, B, rng, seed=900)
    sel = rng.integers(0, 3, B).astype(np.uint32)
    want = mk.lut_many_bootstrap(sg, U, c, o, sel)
    assert np.array_equal(mk.lut_many_bootstrap(multi, U, c, o, sel), want), "host memory"
    assert np.array_equal(_host(mk.lut_many_bootstrap(multi, _gpu(U), _gpu(c), o, _gpu(sel)), np.uint32), want), "device memory"
    assert np.array_equal(mk.lut_many_bootstrap(multi, U[1], c[:1], 2), mk.lut_many_bootstrap(sg, U[1], c[:1], 2)), "fewer inputs than shards"
    sentinel = np.full((B, o, p.lwe_len), 0x5A5A5A5A, dtype=np.uint32)
    for bad in (dict(sel=np.full(B, 3, np.uint32)),):
        out = sentinel.copy()
        with pytest.raises(mk.MktError) as e:
            mk.lut_many_bootstrap(multi, U, c, o, out=out, **bad)
        assert e.value.code == -1 and np.array_equal(out, sentinel)
    multi.close(); sg.close()


# ---- 9: recipe (a) ----
@pytest.mark.parametrize("name", R.CHAIN_SETS)
def test_full_adder_in_one_rotation(require_gpu, name):
    p = getattr(mk, name)
    crs, keys, lin, U = adder_case(p)
    so, sg = oracle_scheme(p, crs, keys), gpu_scheme(p, crs, keys)
    out = mk.lut_many_bootstrap(sg, U, lin, 2)
    assert np.array_equal(out, np.stack([RM.checker_many(so, U, lin[v], 2, p.W) for v in range(8)]))
    s = np.array([bin(v).count("1") for v in range(8)])
    assert np.array_equal(mk.lwe_decrypt(out[:, 0], _dk(p, keys), p), (s & 1).astype(bool)), "sum"
    assert np.array_equal(mk.lwe_decrypt(out[:, 1], _dk(p, keys), p), (s >> 1).astype(bool)), "carry"
    sg.close()


# ---- 10: argument edges and forks ----
def _raw(sg, name, *args):
    """the C entry point itself: the Python layer refuses these calls before the library sees them"""
    from mktfhe_amd import _lib
    return getattr(_lib.lib(), name)(sg.h, *args)


def test_empty_invalid_count_overlap_and_forks(require_gpu):
    from mktfhe_amd import _lib
    from mktfhe_amd.scheme import MEM_DEVICE, MEM_HOST, _np_ptr
    import ctypes as C
    p = mk.KMS2party.scaled(n=16, N=256)
    crs, keys = _keys(p)
    rng = np.random.default_rng(52)
    sg = gpu_scheme(p, crs, keys)
    o, B = 2, 4
    _, U = _packed(p, 2, o, rng)
    c = _inputs(p, keys, B, rng)
    sel = np.array([1, 0, 1, 0], dtype=np.uint32)
    want = mk.lut_many_bootstrap(sg, U, c, o, sel)
    assert mk.lut_many_bootstrap(sg, U, c[:0], o, sel[:0]).shape == (0, o, p.lwe_len)
    at, acc = mk.lut_many_testvector(sg, U, c[:0], o)
    assert at.shape == (0, p.lwe_len - 1) and mk.lut_extract(sg, acc, o).shape == (0, o, p.k + 1, p.N)
    assert np.array_equal(mk.lut_many_bootstrap(sg, U, c[0], o, sel[:1]), want[0]), "a 1-D ciphertext is a batch of one"
    # a table count the library does not take: MKT_ERR_ARG with a message, nothing written
    sentinel = np.full((B, 8, p.lwe_len), 0x5A5A5A5A, dtype=np.uint32)
    for bad in (0, 3, 16, -1):
        out = sentinel.copy()
        rc = _raw(sg, "mkt_lut_many_bootstrap_batch", _np_ptr(U), 2, _np_ptr(sel), _np_ptr(c), bad, _np_ptr(out), B, MEM_HOST)
        assert rc == -1 and b"nout" in _lib.lib().mkt_last_error(sg.h) and np.array_equal(out, sentinel), bad
        accs = np.zeros((B, 8, p.k + 1, p.N), p.ring_dtype)
        assert _raw(sg, "mkt_lut_extract_batch", _np_ptr(np.ones((B, p.k + 1, p.N), p.ring_dtype)), bad, _np_ptr(accs), B, MEM_HOST) == -1 and not accs.any()
    # device memory: out inside lwe's range at nout = 2 is refused, the input is left as it was
    import torch
    buf = torch.zeros((3 * B, p.lwe_len), dtype=torch.int32, device="cuda")
    buf[:B] = _gpu(c)
    dU, dsel = _gpu(U), _gpu(sel)
    for out in (buf[:2 * B], buf[B - 1:3 * B - 1]):
        rc = _raw(sg, "mkt_lut_many_bootstrap_batch", C.c_void_p(dU.data_ptr()), 2, C.c_void_p(dsel.data_ptr()), C.c_void_p(buf.data_ptr()), o, C.c_void_p(out.data_ptr()), B, MEM_DEVICE)
        assert rc == -1 and b"overlap" in _lib.lib().mkt_last_error(sg.h)
    torch.cuda.synchronize()
    assert np.array_equal(_host(buf[:B], np.uint32), c) and not _host(buf[B:], np.uint32).any()
    mk.lut_many_bootstrap(sg, dU, buf[:B], o, dsel, out=buf[B:])               # adjacent, not overlapping: served
    assert np.array_equal(_host(buf[B:], np.uint32).reshape(want.shape), want)
    # a fork runs the call while its parent does: each holds its own workspace
    f = sg.fork()
    got = {}

    def run(name, s):
        got[name] = [mk.lut_many_bootstrap(s, U, c, o, sel) for _ in range(3)]

    threads = [threading.Thread(target=run, args=("parent", sg)), threading.Thread(target=run, args=("fork", f))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(np.array_equal(w, want) for name in ("parent", "fork") for w in got[name]) and len(got) == 2
    f.close(); sg.close()


# ---- 11: one (row, coefficient) table per context, shared with the bootstrap at a coefficient list ----
TABLE_SETS = [mk.CGGIparam.scaled(n=8, N=64), mk.KMS2party.scaled(n=16, N=256)]


def _table_case(p):
    """-> (crs, keys, the named calls of one context in the order the tests make them); B = 3 host inputs"""
    crs, keys = _keys(p)
    rng = np.random.default_rng(71)
    c = _inputs(p, keys, 3, rng)
    T = _tables(p, 2, rng)
    U = {o: _packed(p, 2, o, rng)[1] for o in (2, 4, 8)}
    sel = np.array([1, 0, 1], dtype=np.uint32)
    coef11 = np.array([p.N - 1, 0, 17, 5, 40, 1, p.N - 2, 33, 8, 21, 2], dtype=np.uint32)       # unsorted, both ends of the polynomial
    coef3 = np.array([9, p.N - 1, 4], dtype=np.uint32)
    calls = {"at, 11 coefficients": lambda s: mk.lut_bootstrap_at(s, T, c, coef11, 0, sel),
             "many, o = 2": lambda s: mk.lut_many_bootstrap(s, U[2], c, 2, sel),
             "at, 3 coefficients": lambda s: mk.lut_bootstrap_at(s, T, c, coef3, 2, sel),
             "many, o = 8": lambda s: mk.lut_many_bootstrap(s, U[8], c, 8, sel),
             "one table": lambda s: mk.lut_bootstrap(s, T, c, sel),
             "many, o = 1": lambda s: mk.lut_many_bootstrap(s, T, c, 1, sel),
             "many, o = 4": lambda s: mk.lut_many_bootstrap(s, U[4], c, 4, sel)}
    return crs, keys, calls


def _fresh(p, crs, keys, call):
    """the call on a context that has made no other"""
    s = gpu_scheme(p, crs, keys)
    out = call(s)
    s.close()
    return out


@pytest.mark.parametrize("p", TABLE_SETS, ids=_sid)
def test_shared_table_holds_no_stale_rows(require_gpu, p):
    """the many-table bootstrap and the bootstrap at a coefficient list write the same table of the context: one left from a longer list, or
    laid out for another count per input, must not reach the next call.  Every call equals itself on a freshly created context"""
    crs, keys, calls = _table_case(p)
    sg = gpu_scheme(p, crs, keys)
    for name in ("at, 11 coefficients", "many, o = 2", "at, 3 coefficients", "many, o = 8", "one table"):
        got = calls[name](sg)
        assert np.array_equal(got, _fresh(p, crs, keys, calls[name])), (name, _sid(p))
    sg.close()


@pytest.mark.parametrize("p", TABLE_SETS, ids=_sid)
def test_one_table_takes_no_table_and_leaves_the_context_usable(require_gpu, p):
    """nout = 1 is the plain key switch (no coefficient table) beside nout > 1 (through the table), in either order on one context"""
    crs, keys, calls = _table_case(p)
    sg = gpu_scheme(p, crs, keys)
    one, four = calls["one table"](sg), _fresh(p, crs, keys, calls["many, o = 4"])
    for name, want in (("many, o = 1", one[:, None]), ("many, o = 4", four), ("many, o = 1", one[:, None])):
        assert np.array_equal(calls[name](sg), want), (name, _sid(p))
    sg.close()


@pytest.mark.parametrize("p", TABLE_SETS, ids=_sid)
def test_forks_hold_their_own_table(require_gpu, p):
    """two forks run o = 2 and o = 8 at once, each on its own stream: the parent's words"""
    crs, keys, calls = _table_case(p)
    sg = gpu_scheme(p, crs, keys)
    want = {name: calls[name](sg) for name in ("many, o = 2", "many, o = 8")}
    forks = {name: sg.fork() for name in want}
    got = {}

    def run(name):
        got[name] = [calls[name](forks[name]) for _ in range(3)]

    threads = [threading.Thread(target=run, args=(name,)) for name in want]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert len(got) == 2 and all(np.array_equal(w, want[name]) for name in want for w in got[name])
    for f in forks.values():
        f.close()
    sg.close()
