"""Programmable bootstrap on the GPU (mktfhe.h "programmable bootstrap", mktfhe_amd/lut.py), word for word (tolerance 0 everywhere): the table
step against its numpy restatement, the sign table against mkt_bootstrap_batch, random tables against the CPU checker's chain
(MKT_ARITH_EXACT: against the existing entry points composed), the gather front end, the sharded call, the three-input truth tables of
test_lut_cpu.py, and the edges (B = 0 / 1, out aliasing the input, a forked context)."""
import numpy as np
import pytest

import ref_lut as R
from helpers import btilde_words, gpu_scheme, keygen, mk, oracle_scheme
from test_gpu_parity import FULL, SMALL

pytestmark = pytest.mark.gpu

_KEYS = {}


def _keys(p, seed=5):
    k = (repr(p), seed)
    if k not in _KEYS:
        _KEYS[k] = keygen(p, seed)
    return _KEYS[k]


def _sid(p):
    return f"{p.name}-n{p.n}-N{p.N}-k{p.k}-b{p.blk_len}"


def _dk(p, keys):
    return keys if p.multikey else keys[0]


def _tables(p, nluts, rng):
    """random tables with the edge words 0, all ones and the most negative word in every row (the first row: only those)"""
    W = p.W
    edge = np.array([0, (1 << W) - 1, 1 << (W - 1)], dtype=np.uint64)
    t = (rng.integers(0, 1 << 63, (nluts, p.N), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (nluts, p.N), dtype=np.uint64)) & np.uint64((1 << W) - 1)
    t[:, :3] = edge
    t[:, -3:] = edge[::-1]
    t[0] = edge[np.arange(p.N) % 3]
    return t.astype(p.ring_dtype)


def _gpu(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.int8): np.int8, np.dtype(np.uint8): np.uint8}[a.dtype]
    return torch.from_numpy(a.view(signed)).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _inputs(p, keys, B, rng, seed=700):
    """fresh encryptions of ANY torus message under rotating parties"""
    return np.stack([mk.lwe_encrypt_word(int(rng.integers(0, 1 << 32)), j % p.nparty, keys[j % p.nparty], p, deterministic_seed=seed + j) for j in range(B)])


# ---- 1: the table step ----
@pytest.mark.parametrize("nluts", [1, 5])
@pytest.mark.parametrize("p", [mk.CGGIparam.scaled(n=8, N=64), mk.CGGIparam.scaled(n=8, N=256, W=64), mk.CGGIparam.scaled(n=6, N=1024, k=2),
                               mk.KMS2party.scaled(n=4, N=2048), mk.CGGIparam.scaled(n=4, N=4096, W=64), mk.KMS4party.scaled(n=3, N=128)], ids=_sid)
def test_testvector_equals_the_numpy_rotation(require_gpu, p, nluts):
    rng = np.random.default_rng(p.N + nluts)
    sg = mk.Scheme(p)                                        # no keys: the table step needs none
    bodies = [w for pair in btilde_words(p.N).values() for w in pair] + [int(w) for w in rng.integers(0, 1 << 32, 5)]
    B = len(bodies)
    lwe = rng.integers(0, 1 << 32, (B, p.lwe_len), dtype=np.uint64).astype(np.uint32)
    lwe[:, -1] = np.array(bodies, dtype=np.uint64).astype(np.uint32)
    bts = [R.btilde(w, p.N) for w in bodies]
    assert {0, 1, p.N - 1, p.N, p.N + 1, 2 * p.N - 1, 2 * p.N} <= set(bts)
    luts = _tables(p, nluts, rng)
    sel = rng.integers(0, nluts, B).astype(np.uint32)
    sel[0], sel[1], sel[2], sel[3] = 0, nluts - 1, nluts - 1, 0
    want = np.stack([R.testvector(luts[sel[j]], bts[j], p.W, p.k) for j in range(B)])
    assert np.array_equal(mk.lut_testvector(sg, luts, lwe, sel).astype(np.uint64), want), "host memory"
    acc = mk.lut_testvector(sg, _gpu(luts), _gpu(lwe), _gpu(sel))
    assert np.array_equal(_host(acc, p.ring_dtype).astype(np.uint64), want), "device memory"
    # no selector: row 0 for the whole batch; a single (N,) table
    want0 = np.stack([R.testvector(luts[0], bts[j], p.W, p.k) for j in range(B)])
    assert np.array_equal(mk.lut_testvector(sg, luts, lwe).astype(np.uint64), want0)
    assert np.array_equal(_host(mk.lut_testvector(sg, _gpu(luts[0]), _gpu(lwe)), p.ring_dtype).astype(np.uint64), want0)
    # device tables that are not 16-byte aligned take the word-by-word kernel: the same words
    import torch
    odd = torch.empty(nluts * p.N + 1, dtype=_gpu(luts).dtype, device="cuda")[1:].view(nluts, p.N)
    odd.copy_(_gpu(luts))
    assert np.array_equal(_host(mk.lut_testvector(sg, odd, _gpu(lwe), _gpu(sel)), p.ring_dtype).astype(np.uint64), want), "unaligned tables"
    # a selector beyond the tables: clamped to the last row in device memory, refused in host memory
    bad = sel.copy(); bad[B // 2] = nluts + 7
    wantc = want.copy(); wantc[B // 2] = R.testvector(luts[nluts - 1], bts[B // 2], p.W, p.k)
    assert np.array_equal(_host(mk.lut_testvector(sg, _gpu(luts), _gpu(lwe), _gpu(bad)), p.ring_dtype).astype(np.uint64), wantc)
    with pytest.raises(mk.MktError) as e:
        mk.lut_testvector(sg, luts, lwe, bad)
    assert e.value.code == -1
    sg.close()


# ---- 2 and 3: the sign table is bootstrapping!; random tables equal the checker's chain ----
def _exact_scheme(p, crs, keys):
    """an MKT_ARITH_EXACT context with keys, or None where the gate path is not offered for the set (MKT_ERR_UNSUPPORTED)"""
    try:
        return gpu_scheme(p, crs, keys, arith=mk.ARITH_EXACT)
    except mk.MktError as e:
        assert e.code == -2, e
        return None


def _sign_check(sg, p, c):
    want = sg.bootstrapping_(c.copy())
    got = mk.lut_bootstrap(sg, mk.sign_lut(p), c)
    assert np.array_equal(got, want), ("sign table", _sid(p))
    return want


def _composed(sx, luts, c, sel):
    """the programmable bootstrap through the existing entry points: table step, modswitch, blindrotate!, keyswitch!"""
    acc = mk.lut_testvector(sx, luts, c, sel)
    at, _ = sx.modswitch(c)
    return sx.keyswitch(sx.blindrotate_(at, acc))


def _lut_check(p, B, seed):
    crs, keys = _keys(p)
    rng = np.random.default_rng(seed)
    c = _inputs(p, keys, B, rng)
    nluts = 3
    luts = _tables(p, nluts, rng)
    sel = rng.integers(0, nluts, B).astype(np.uint32)
    sel[0], sel[-1] = nluts - 1, 0
    so = oracle_scheme(p, crs, keys)
    ref = np.stack([R.checker_bootstrap(so, luts[sel[j]], c[j], p.W) for j in range(B)])
    sg = gpu_scheme(p, crs, keys)
    _sign_check(sg, p, c)
    assert np.array_equal(mk.lut_bootstrap(sg, luts, c, sel), ref), ("random tables, host memory", _sid(p))
    assert np.array_equal(_host(mk.lut_bootstrap(sg, _gpu(luts), _gpu(c), _gpu(sel)), np.uint32), ref), ("random tables, device memory", _sid(p))
    assert np.array_equal(_composed(sg, luts, c, sel), ref), "the composed entry points"
    sg.close()
    sx = _exact_scheme(p, crs, keys)
    if sx is not None:
        words = []
        for impl in (0, 1):
            sx.set_option("exact_impl", impl)
            _sign_check(sx, p, c)
            got = mk.lut_bootstrap(sx, luts, c, sel)
            assert np.array_equal(got, _composed(sx, luts, c, sel)), ("EXACT, random tables", impl, _sid(p))
            words.append(got)
        assert np.array_equal(words[0], words[1]), "EXACT: both implementations give the same words"
        sx.close()


@pytest.mark.parametrize("p", SMALL, ids=_sid)
def test_small_sets_sign_table_and_random_tables(require_gpu, p):
    _lut_check(p, B=5, seed=11)


@pytest.mark.parametrize("p", FULL, ids=lambda p: p.name)
def test_full_sets_sign_table_and_random_tables(require_gpu, p):
    _lut_check(p, B=2, seed=12)


SWITCH_CASES = [(mk.Blockparam.scaled(n=30, N=256, blk_d=10), "rot_blkg", (1, 2, 4)), (mk.KMS2partyblock.scaled(n=24, N=256, blk_d=8), "rot_blkg", (1, 2, 4)),
                (mk.Blockparam_k2.scaled(n=12, N=1024, blk_d=4), "rot_blkg", (1, 4)),
                (mk.CCS2party.scaled(n=12, N=256), "ccs_pipe", (0, 1)), (mk.CCS4party.scaled(n=6, N=512), "ccs_pipe", (0, 1)),
                (mk.CGGIparam.scaled(n=20, N=256), "rot_wide", (1, 2)), (mk.KMS2party_N1024_l2.scaled(n=8), "rot_wide", (1, 2)),
                (mk.CGGIparam.scaled(n=12, N=1024, l_gsw=2, logB_gsw=10), "rot_wide", (1, 2))]


@pytest.mark.parametrize("p, opt, values", SWITCH_CASES, ids=lambda v: _sid(v) if isinstance(v, mk.Params) else str(v))
def test_forced_kernels_give_identical_words(require_gpu, p, opt, values):
    """the kernel switches the existing tests force: every forced rotation kernel returns the checker's words for random tables"""
    crs, keys = _keys(p)
    rng = np.random.default_rng(21)
    B = 5
    c = _inputs(p, keys, B, rng)
    luts = _tables(p, 2, rng)
    sel = (np.arange(B) % 2).astype(np.uint32)
    so = oracle_scheme(p, crs, keys)
    ref = np.stack([R.checker_bootstrap(so, luts[sel[j]], c[j], p.W) for j in range(B)])
    sg = gpu_scheme(p, crs, keys)
    names = set()
    for v in values:
        sg.set_option(opt, v)
        assert np.array_equal(mk.lut_bootstrap(sg, luts, c, sel), ref), (opt, v)
        names.add(sg.last_kernel_name())
    assert names and "" not in names
    sg.close()


# ---- 4: the gather front end ----
@pytest.mark.parametrize("p", [mk.CGGIparam.scaled(n=20, N=256), mk.KMS2party.scaled(n=16, N=256), mk.CCS2party.scaled(n=12, N=256)], ids=_sid)
def test_gather_is_the_linear_combination_then_the_bootstrap(require_gpu, p):
    crs, keys = _keys(p)
    rng = np.random.default_rng(31)
    P, B, nluts = 6, 7, 3
    sg = gpu_scheme(p, crs, keys)
    pool = _inputs(p, keys, P, rng)
    luts = _tables(p, nluts, rng)
    sel = rng.integers(0, nluts, B).astype(np.uint32)
    idx = rng.integers(0, P, (B, 4)).astype(np.uint32)
    wt = rng.integers(-4, 5, (B, 4)).astype(np.int8)
    wt[0] = [1, 2, 4, 0]; wt[1] = [0, 0, 0, 0]; wt[2] = [-128, 127, -1, 1]
    cst = rng.integers(0, 1 << 32, B, dtype=np.uint64).astype(np.uint32)
    lin = R.linear(pool, idx, wt, cst)
    assert not lin[1, :-1].any() and lin[1, -1] == cst[1]                     # all weights 0: the constant alone
    want = mk.lut_bootstrap(sg, luts, lin, sel)
    out = np.full((B, p.lwe_len), 0xA5A5A5A5, dtype=np.uint32)
    assert mk.lut_gather(sg, luts, sel, pool, idx, wt, cst, out) is out and np.array_equal(out, want), "host memory"
    # device memory, out a later region of the pool; indices beyond the pool are clamped to its last row
    import torch
    big = torch.cat([_gpu(pool), torch.zeros((B, p.lwe_len), dtype=torch.int32, device="cuda")])
    idx_bad = idx.copy(); idx_bad[3, 1] = P + 100; idx_bad[4, 0] = 0xFFFFFFFF
    wt2 = wt.copy(); wt2[3, 1] = 3; wt2[4, 0] = -2
    want_c = mk.lut_bootstrap(sg, luts, R.linear(pool, idx_bad, wt2, cst), sel)
    mk.lut_gather(sg, _gpu(luts), _gpu(sel), big[:P], _gpu(idx_bad), _gpu(wt2), _gpu(cst), big[P:])
    assert np.array_equal(_host(big[P:], np.uint32), want_c), "device memory, clamped rows, out inside the pool's allocation"
    assert np.array_equal(_host(big[:P], np.uint32), pool), "the pool rows are untouched"
    # host memory: a bad selector, a bad index, no table, an empty pool -> MKT_ERR_ARG, nothing written
    sentinel = np.full((B, p.lwe_len), 0x5A5A5A5A, dtype=np.uint32)
    bad_sel = sel.copy(); bad_sel[0] = nluts
    for args in ((luts, bad_sel, pool, idx, wt, cst), (luts, sel, pool, idx_bad, wt, cst), (luts[:0], None, pool, idx, wt, cst),
                 (luts, sel, pool[:0], idx, wt, cst)):
        out = sentinel.copy()
        with pytest.raises(mk.MktError) as e:
            mk.lut_gather(sg, *args, out)
        assert e.value.code == -1 and np.array_equal(out, sentinel)
    out = sentinel.copy()
    with pytest.raises(mk.MktError) as e:
        mk.lut_bootstrap(sg, luts, pool, bad_sel[:P], out=out[:P])
    assert e.value.code == -1 and np.array_equal(out, sentinel)
    sg.close()


# ---- 5: sharded ----
@pytest.mark.parametrize("flags", [{}, {"private_keys": True}, {"stage_always": True}], ids=lambda f: "-".join(f) or "plain")
@pytest.mark.parametrize("p", [mk.CGGIparam.scaled(n=20, N=256), mk.KMS2party.scaled(n=16, N=256)], ids=_sid)
def test_two_logical_shards_give_the_single_context_words(require_gpu, p, flags):
    crs, keys = _keys(p)
    rng = np.random.default_rng(41)
    sg = gpu_scheme(p, crs, keys)
    multi = mk.setup_multi(p, [0, 0], keys=keys if p.multikey else keys[0], a=crs, **flags)
    luts = _tables(p, 4, rng)
    for B in (5, 4, 1):                                                       # ragged, even, fewer ciphertexts than shards
        c = _inputs(p, keys, B, rng, seed=800 + B)
        sel = rng.integers(0, 4, B).astype(np.uint32)
        want = mk.lut_bootstrap(sg, luts, c, sel)
        assert np.array_equal(mk.lut_bootstrap(multi, luts, c, sel), want), ("host memory", B)
        assert np.array_equal(_host(mk.lut_bootstrap(multi, _gpu(luts), _gpu(c), _gpu(sel)), np.uint32), want), ("device memory", B)
        assert np.array_equal(mk.lut_bootstrap(multi, luts[1], c), mk.lut_bootstrap(sg, luts[1], c)), ("one table, no selector", B)
    with pytest.raises(mk.MktError) as e:
        mk.lut_bootstrap(multi, luts, c, np.full(B, 4, np.uint32))
    assert e.value.code == -1
    multi.close(); sg.close()


# ---- 6: the three-input truth tables and the re-encoding of test_lut_cpu.py ----
@pytest.mark.parametrize("name", R.CHAIN_SETS)
def test_truth_tables_have_the_checkers_words_and_decrypt(require_gpu, name):
    p = getattr(mk, name)
    crs, keys, x, y, z = R.chain_case(p)
    so, sg = oracle_scheme(p, crs, keys), gpu_scheme(p, crs, keys)
    lin = R.truth_linear(x, y, z)
    tables = list(R.TRUTH_TABLES.values())
    luts = np.stack([mk.lut_poly(R.truth_values(t, p.W), p) for t in tables])
    sel = np.repeat(np.arange(4, dtype=np.uint32), 8)
    out = mk.lut_bootstrap(sg, luts, np.concatenate([lin] * 4), sel)
    ref = np.stack([R.checker_bootstrap(so, luts[t], lin[v], p.W) for t in range(4) for v in range(8)])
    assert np.array_equal(out, ref)
    assert np.array_equal(mk.lwe_decrypt(out, _dk(p, keys), p), np.array(tables, dtype=bool).ravel())
    # the same level through the gather form: weights 1, 2, 4 and the centre 1/32
    pool = np.concatenate([x, y, z])
    v = np.tile(np.arange(8, dtype=np.uint32), 4)
    idx = np.stack([v, 8 + v, 16 + v, np.zeros_like(v)], axis=1)
    wt = np.tile(np.array([1, 2, 4, 0], dtype=np.int8), (32, 1))
    got = mk.lut_gather(sg, luts, sel, pool, idx, wt, np.full(32, R.CENTRE, np.uint32), np.empty_like(out))
    assert np.array_equal(got, ref)
    sg.close()


# ---- 7: edges ----
def test_empty_single_aliased_and_forked(require_gpu):
    p = mk.KMS2party.scaled(n=16, N=256)
    crs, keys = _keys(p)
    rng = np.random.default_rng(51)
    sg = gpu_scheme(p, crs, keys)
    luts = _tables(p, 2, rng)
    c = _inputs(p, keys, 4, rng)
    sel = np.array([1, 0, 1, 0], dtype=np.uint32)
    want = mk.lut_bootstrap(sg, luts, c, sel)
    assert mk.lut_bootstrap(sg, luts, c[:0], sel[:0]).shape == (0, p.lwe_len)
    assert mk.lut_testvector(sg, luts, c[:0]).shape == (0, p.k + 1, p.N)
    assert np.array_equal(mk.lut_bootstrap(sg, luts, c[:1], sel[:1]), want[:1])
    assert np.array_equal(mk.lut_bootstrap(sg, luts, c[0], sel[:1]), want[0])          # a 1-D ciphertext is a batch of one
    a = c.copy()
    assert mk.lut_bootstrap(sg, luts, a, sel, out=a) is a and np.array_equal(a, want), "out aliasing the input, host memory"
    t = _gpu(c)
    mk.lut_bootstrap(sg, _gpu(luts), t, _gpu(sel), out=t)
    assert np.array_equal(_host(t, np.uint32), want), "out aliasing the input, device memory"
    f = sg.fork()
    assert np.array_equal(mk.lut_bootstrap(f, luts, c, sel), want), "a forked context"
    f.synchronize()
    assert np.array_equal(_host(mk.lut_bootstrap(f, _gpu(luts), _gpu(c), _gpu(sel)), np.uint32), want)
    f.close(); sg.close()
