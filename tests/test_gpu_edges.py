"""The rounding steps that every rotation and key-switch kernel carries as its OWN fused copy, at their boundaries.

The standalone kernels (mkt_transform_*_batch, mkt_decompose_batch) see boundary words in tests/test_gpu_parity.py; the gate path
calls neither.  Fresh encryptions, the test-vector accumulator (b = +-2^(W-3), every a polynomial zero) and uniformly random key-switch
accumulators do not reach the boundaries below by construction, so these tests start the kernels from crafted valid inputs
(helpers.lwe_edge_rows, acc_edge, ks_edge_acc, ks_edge_acc_at, lut_edge_tables; tests/test_edges_cpu.py proves every class is in them for
every set used here) and
compare EVERY ciphertext with the oracle / tests/ref_exact.py.  Every rotation case asserts the kernel it reached.

| step | fused copies (not the standalone kernel) | boundary classes |
|---|---|---|
| mod switch divbits(w, 32-logN-1) | `pre_switched ? v : divbits(...)` in kernels.hip, rot_block.hip, ccs_pipe.hip, fx_exact.hip, ntt_exact.hip (some feeding an all-skipped shortcut `any |= ... != 0`) | words that round to 0 (raw word not 0), to 1 on a tie, to N-1 / N / N+1, to 2N-1, to 2N (full turn); masks all zero, all skipped, whole blocks / one party skipped |
| test vector from btilde | launch_testvector, inline in kms_phase2_kernel / exact_kms_phase2_kernel (`if (a.lin) { ... if (tb > N) ... }`) | btilde in {0, 1, N-1, N, N+1, 2N-1, 2N}, each through the smallest and the largest word that rounds to it |
| gadget digits Gadget::prep / digit_points | every rotation kernel, KMS phase 2 (LEV and UniEnc gadgets), CCS | ties of divbits(x, W - l logB), one below / above; the rounding carry out of the top digit; the carry of the prepared value (all digits -B/2); all digits B/2-1; 2^(W-1); W = 64: the same high parts over a low half of all ones / the top bit alone; index i and i + M, indices 0, M-1, M, N-1; non-zero acc.a on entry (KMS overwrites it, bootstrapping.jl:553-556) |
| key-switch digits | keyswitch_mg_kernel (`divbits(w, 32-f logD)` / gb.prep), ks_digits_kernel + keyswitch_pair_kernel, extract_word, ks_init_kernel | the carry that leaves the f logD-bit field, ties, all digits D-1 / -D/2 / D/2-1, zero, 0x80000000 at a negated position, j = 0 / 1 / N-1, both sides of the copied / switched border (n < N, n > N), W = 64: the low half cut off, ragged groups of 32 |
| key-switch digits at a coefficient | the `AT = true` instantiations of keyswitch_mg_kernel, ks_digits_kernel (+ keyswitch_pair_kernel), ks_init_kernel / ks_reduce_kernel; extract_word_at; ks_at_table_kernel (the coefficient list, NULL = 0 .. o-1) | the classes of the line above in X^v times the same accumulators, v in {0, 1, n-1, n, n+1, N/2, N-1}, rows and coefficients mixed in one call; W = 64, the borrow: a word wrapped by X^v was negated at 64 bits and is truncated and negated again at 32, so the extracted word is trunc(a) + (low half != 0) -- low halves 0 and 1, and a tie / carry (and the word one below) over a non-zero low half on both sides of j = v |
| lookup-table route (context.cpp lut_chunk) | lut_testvector_kernel: `divbits(w, 32-logN-1+nu) << nu` on b and (nu > 0) on the mask words, which the rotation reads pre-switched; the caller's table rotated into acc.b | the mod-switch classes of the first line on the plain (nu = 0) and the coarse grid (targets 0, nout, N-nout, N, N+nout, 2N-nout, 2N); tables whose words sit on the first CMux's gadget boundaries (and their negatives: the table step negates) at 0, M-1, M, N-1 and pairs (i, i + M) |

A kernel that gets its own copy of one of these steps gets a line in tests/edge_cases.py, and an instantiation that gets its own
compile-time gadget gets a line: every rotation case also asserts the (gadget length, base) that the instantiation it reached holds as
template constants (mkt_get_metric "rot_static_l" / "rot_static_logB"), and tests/test_edges_cpu.py reads the launchers' source so that
a specialisation without a line fails without a GPU.

`tb >= N` in place of `tb > N` is not a bug these tests could see: at tb == N both forms write +1/8 to all N coefficients
(tests/test_edges_cpu.py asserts it); the test-vector cases separate `i <= tb`, a sign not flipped, and a half turn taken one early / late.
"""
import numpy as np
import pytest

import edge_cases as EC
import ref_lut as R
import ref_lut_many as RM
from helpers import (O, gate_input, gpu_scheme, keygen, ks_at_edge_check, ks_edge_check, lut_edge_tables, lwe_edge_rows, mk, oracle_scheme)
from helpers import rot_inputs as _rot_inputs
from ref_gate3 import linear3
from test_keyswitch_at_cpu import checker_at

pytestmark = pytest.mark.gpu


def _cid(v):
    if isinstance(v, mk.Params):
        return EC.sid(v)
    if isinstance(v, dict):
        return "-".join(f"{k}{x}" for k, x in v.items()) or "default"
    return str(v)


def _engines(p, seed, opts, exact=False):
    crs, keys = keygen(p, seed)
    so = oracle_scheme(p, crs, keys)
    sg = gpu_scheme(p, crs, keys, arith=mk.ARITH_EXACT if exact else mk.ARITH_F64REF)
    for k, v in opts.items():
        sg.set_option(k, v)
    return crs, keys, so, sg


# ---------------------------------------------------------------- 1. blind rotation from arbitrary accumulators
def _static_gadget(s):
    """the compile-time (gadget length, log2 base) of the instantiation that the last rotation launched, 0 = a run-time value"""
    return int(s.get_metric("rot_static_l")), int(s.get_metric("rot_static_logB"))


@pytest.mark.parametrize("p,opts,kernel,B,static", EC.ROT_CASES, ids=["-".join(_cid(v) for v in c[:4]) for c in EC.ROT_CASES])
def test_blindrotate_from_edge_accumulators(require_gpu, p, opts, kernel, B, static):
    crs, keys, so, sg = _engines(p, 21, opts)
    for at, acc in _rot_inputs(p, B, 22):
        got = sg.blindrotate_(at, acc.astype(p.ring_dtype).copy()).astype(np.uint64).reshape(acc.shape)
        assert sg.last_kernel_name() == kernel, sg.last_kernel_name()
        assert _static_gadget(sg) == static, _static_gadget(sg)
        for j in range(len(at)):
            assert np.array_equal(got[j], so.blindrotate(at[j], acc[j])), (j, at[j].nonzero()[0], at[j][at[j] != 0][:1])
    sg.close()


def _ref_rotate(p, keys, crs, at, acc):
    import ref_exact as RX
    if p.scheme in (mk.KMS, mk.KMS_BLOCK):
        return RX.kms_blindrotate(p, keys, crs, at, acc)
    if p.scheme == mk.CCS:
        return RX.ccs_blindrotate(p, keys, crs, at, acc)
    return (RX.blindrotate_lmss if p.blk_len > 1 else RX.blindrotate)(p, keys[0].brk, at, acc)


@pytest.mark.parametrize("p,opts,kernel,B", EC.EXACT_CASES, ids=_cid)
def test_exact_blindrotate_from_edge_accumulators(require_gpu, p, opts, kernel, B):
    """MKT_ARITH_EXACT: the integer-NTT kernels and the Float64 pipe against the big-integer restatement, every ciphertext"""
    crs, keys, so, sx = _engines(p, 23, opts, exact=True)
    for at, acc in _rot_inputs(p, B, 24):
        got = sx.blindrotate_(at, acc.astype(p.ring_dtype).copy()).astype(np.uint64).reshape(len(at), -1)
        assert sx.last_kernel_name() == kernel, sx.last_kernel_name()
        for j in range(len(at)):
            assert np.array_equal(got[j], np.asarray(_ref_rotate(p, keys, crs, at[j], acc[j])).reshape(-1)), (j, at[j].nonzero()[0])
    sx.close()


@pytest.mark.parametrize("p", EC.EXACT_PAIR_SETS, ids=_cid)
def test_exact_implementations_agree_on_edge_accumulators(require_gpu, p):
    """integer NTT (exact_impl 0) against the Float64 pipe (1) word for word, up to N = 4096; where the pipe's proven bound does not certify
    the shape the engine serves the call with the integer kernels: the kernel name says which, and must agree with fx_available"""
    crs, keys, so, sx = _engines(p, 25, {}, exact=True)
    for at, acc in _rot_inputs(p, 5, 26):
        res = {}
        for impl in (0, 1):
            sx.set_option("exact_impl", impl)
            res[impl] = sx.blindrotate_(at, acc.astype(p.ring_dtype).copy())
            name = sx.last_kernel_name()
            assert ("fx_" in name) == (impl == 1 and sx.get_metric("fx_available") == 1.0), (impl, name)
            print(f"{EC.sid(p)} exact_impl={impl}: {name}")
        assert np.array_equal(res[0], res[1])
    sx.close()


# ---------------------------------------------------------------- 2. key switch, every ciphertext
@pytest.mark.parametrize("p", EC.KS_SETS, ids=_cid)
def test_keyswitch_at_digit_boundaries(require_gpu, p):
    crs, keys, so, sg = _engines(p, 27, {})
    assert ks_edge_check(p, so, sg, np.random.default_rng(28), EC.KS_BATCHES) == sum(EC.KS_BATCHES)
    # ... and at a coefficient: X^v times the same accumulators, read back at v (and, rows mixed, at every other coefficient of the list)
    assert p in EC.KS_AT_SETS
    full = p in EC.KS_AT_FULL
    batches, coefs = (EC.KS_AT_FULL_BATCHES, EC.KS_AT_FULL_COEFS(p)) if full else (EC.KS_BATCHES, EC.KS_AT_COEFS(p))
    n = ks_at_edge_check(p, so, sg, np.random.default_rng(35), batches, coefs)
    assert n == 2 * len(coefs) * sum(batches)
    print(f"{EC.sid(p)}: {sum(EC.KS_BATCHES)} + {n} ciphertexts compared (the latter in host and in device memory)")
    sg.close()


# ---------------------------------------------------------------- 3. fused mod switch and test vector: whole bootstraps on crafted rows
def _three_routes(p, so, sg, rows, kernel):
    """bootstrapping_(rows) -- the fused mod switch -- and keyswitch(blindrotate_(modswitch(rows), test vector)) -- the pre_switched branch"""
    out = sg.bootstrapping_(rows.copy())
    assert sg.last_kernel_name() == kernel, sg.last_kernel_name()
    at, bt = sg.modswitch(rows)
    for j in range(len(rows)):
        at_o, bt_o = so.modswitch(rows[j])
        assert np.array_equal(at[j], at_o) and bt[j] == bt_o, j
    acc0 = np.stack([so.testvector(int(b)) for b in bt]).astype(p.ring_dtype)
    staged = sg.keyswitch(sg.blindrotate_(at, acc0.copy()).reshape(acc0.shape))
    assert sg.last_kernel_name() == kernel, sg.last_kernel_name()
    assert np.array_equal(out, staged), np.nonzero((out != staged).any(axis=1))[0]
    return out, at, acc0


@pytest.mark.parametrize("p,opts,kernel", EC.BOOT_CASES, ids=_cid)
def test_bootstrap_on_edge_rows(require_gpu, p, opts, kernel):
    crs, keys, so, sg = _engines(p, 29, opts)
    rows, kinds = lwe_edge_rows(p, np.random.default_rng(30))
    out, _, _ = _three_routes(p, so, sg, rows, kernel)
    for j in range(len(rows)):
        assert np.array_equal(out[j], so.bootstrap(rows[j])), (j, kinds[j])
    sg.close()


@pytest.mark.parametrize("p,opts,kernel", EC.EXACT_BOOT_CASES, ids=_cid)
def test_exact_bootstrap_on_edge_rows(require_gpu, p, opts, kernel):
    """EXACT contexts: the fused route against the staged route on the same context and against ref_exact (the all-skipped rows meet the
    `any` shortcuts of ntt_exact.hip)"""
    crs, keys, so, sx = _engines(p, 31, opts, exact=True)
    rows, kinds = lwe_edge_rows(p, np.random.default_rng(32))
    out, at, acc0 = _three_routes(p, so, sx, rows, kernel)
    for j in range(len(rows)):
        want = so.keyswitch(np.asarray(_ref_rotate(p, keys, crs, at[j], acc0[j].astype(np.uint64))).reshape(1 + p.k, p.N))
        assert np.array_equal(out[j], want), (j, kinds[j])
    sx.close()


def _oracle_mux(p, so, sel, a, b):
    """two blindrotate! of the AND-linear parts of (sel, a) and (NOT sel, b), the accumulators added, + 1/8 at X^0 of b, one keyswitch!"""
    m = np.uint64((1 << p.W) - 1)
    accs = []
    for x, y in ((sel, a), ((0 - sel.astype(np.int64)).astype(np.uint32), b)):
        at, bt = so.modswitch(O.gate_linear(1, x, y))
        accs.append(so.blindrotate(at, so.testvector(bt)).astype(np.uint64))
    acc = ((accs[0] + accs[1]) & m).reshape(-1, p.N)
    acc[0, 0] = (int(acc[0, 0]) + (1 << (p.W - 3))) & int(m)
    return so.keyswitch(acc)


@pytest.mark.parametrize("p,opts,kernel", EC.GATE_CASES, ids=_cid)
def test_gate_entry_points_on_edge_rows(require_gpu, p, opts, kernel):
    """x chosen so that the gate's linear part IS the crafted row (the other operands zero rows; XOR, XNOR and the doubling three-input
    codes reach even words only): the six gates, gate_ops with NOT flags, every linear shape of gate3, MUX (two rotations per gate), on
    the kernel families of the bootstrap cases; each entry point asserts the kernel it reached"""
    crs, keys, so, sg = _engines(p, 33, opts)
    rng = np.random.default_rng(34)
    rows = {ev: lwe_edge_rows(p, rng, even=ev)[0] for ev in (False, True)}
    want = {ev: np.stack([so.bootstrap(r) for r in rows[ev]]) for ev in (False, True)}
    B = len(rows[False])
    zero = np.zeros_like(rows[False])
    neg = lambda v: (0 - v.astype(np.int64)).astype(np.uint32)      # noqa: E731

    def reached(out):
        assert sg.last_kernel_name() == kernel, sg.last_kernel_name()
        return out

    for op in range(6):
        ev = op in (3, 4)
        x = gate_input(op, rows[ev])
        assert all(np.array_equal(O.gate_linear(op, x[j], zero[j]), rows[ev][j]) for j in range(B))
        assert np.array_equal(reached(sg.gate(op, x, zero)), want[ev]), op
        ops = np.full(B, op | mk.OP_NOT_X, dtype=np.uint8)
        ops[1::2] = op | mk.OP_NOT_X | mk.OP_NOT_Y
        assert np.array_equal(reached(sg.gate_ops(ops, neg(x), zero)), want[ev]), (op, "NOT flags")
        assert np.array_equal(sg.gate_ops(np.full(B, op | mk.OP_NOT_Y, dtype=np.uint8), zero, neg(x)), want[ev]), (op, "NOT_Y")     # (every gate is symmetric in x, y)
    b30 = np.zeros_like(rows[False]).astype(np.int64)
    b30[:, -1] = 1 << 30
    for code in range(6):
        ev = code in (2, 3)
        r = rows[ev].astype(np.int64)
        x = {0: r, 1: -r, 2: -r // 2, 3: r // 2, 4: r - b30, 5: 3 * b30 - r}[code]
        x = (x & 0xFFFFFFFF).astype(np.uint32)
        for flags, xx in ((0, x), (mk.OP_NOT_X | mk.OP_NOT_Z, neg(x))):
            assert np.array_equal(linear3(code | flags, xx, zero, zero), rows[ev]), code
            assert np.array_equal(reached(sg.gate3(code | flags, xx, zero, zero)), want[ev]), (code, flags)
    # MUX(0-row, a, b): the two AND-linear parts are the crafted row j and row B-1-j
    a = gate_input(1, rows[False])
    b = a[::-1].copy()
    assert all(np.array_equal(O.gate_linear(1, zero[j], a[j]), rows[False][j]) for j in range(B))
    got = reached(sg.mux(zero, a, b))
    for j in range(B):
        assert np.array_equal(got[j], _oracle_mux(p, so, zero[j], a[j], b[j])), ("mux", j)
    sg.close()


# ---------------------------------------------------------------- 4. the lookup-table route: crafted rows through crafted tables
def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


def _lut_inputs(p, rng, nout):
    """lwe_edge_rows on the grid of nout and one or two random rows (an odd batch), a table row per input"""
    rows, kinds = lwe_edge_rows(p, rng, nout=nout)
    more = 1 + len(rows) % 2
    rows = np.concatenate([rows, rng.integers(0, 1 << 32, (more, p.lwe_len), dtype=np.uint64).astype(np.uint32)])
    assert len(rows) % 2 == 1
    sel = (np.arange(len(rows)) % 2).astype(np.uint32)[::-1].copy()
    return rows, kinds + ["random"] * more, sel


def _lut_calls(p):
    """(name, nout of the input grid, table count packed into a row, call, checker of one ciphertext)"""
    N = p.N
    at0, at1 = np.array([N - 1, 0, 1], dtype=np.uint32), np.array([0, 1], dtype=np.uint32)
    return [
        ("lut_bootstrap", 1, 1, lambda s, T, c, sel: mk.lut_bootstrap(s, T, c, sel)[:, None], None),
        ("lut_many_bootstrap o=2", 2, 2, lambda s, T, c, sel: mk.lut_many_bootstrap(s, T, c, 2, sel), None),
        ("lut_many_bootstrap o=8", 8, 8, lambda s, T, c, sel: mk.lut_many_bootstrap(s, T, c, 8, sel), None),
        ("lut_bootstrap_at nu=0", 1, 1, lambda s, T, c, sel: mk.lut_bootstrap_at(s, T, c, _like(c, at0), nu=0, sel=sel), at0),
        ("lut_bootstrap_at nu=1", 2, 2, lambda s, T, c, sel: mk.lut_bootstrap_at(s, T, c, _like(c, at1), nu=1, sel=sel), at1),
    ]


def _like(c, a):
    return a if isinstance(c, np.ndarray) else _t(a)


def _lut_reference(p, so, name, nout, T, row, coef):
    if name == "lut_bootstrap":
        return R.checker_bootstrap(so, T, row, p.W)[None]
    if coef is None:
        return RM.checker_many(so, T, row, nout, p.W)
    return checker_at(so, T, row, coef, p.W, nout)


def _lut_composed(sx, p, name, nout, luts, c, sel, coef):
    """MKT_ARITH_EXACT: the unit calls composed, none of them a key switch at a coefficient -- the table step on the grid of nout, the rotation,
    the extraction (mkt_lut_extract_batch for the many-table form, numpy for a coefficient list), the plain key switch"""
    at, acc = mk.lut_many_testvector(sx, luts, c, nout, sel)
    acc = sx.blindrotate_(at, acc)
    if name == "lut_bootstrap":
        return sx.keyswitch(acc)[:, None]
    if coef is None:
        return sx.keyswitch(mk.lut_extract(sx, acc, nout))
    accs = np.stack([RM.extract(acc, int(v), p.W) for v in coef], axis=1).astype(p.ring_dtype)
    return sx.keyswitch(accs)


@pytest.mark.parametrize("p,opts,kernel,exact", EC.LUT_BOOT_CASES, ids=_cid)
def test_table_bootstraps_on_edge_rows(require_gpu, p, opts, kernel, exact):
    """every lookup-table bootstrap (one route: table step, rotation, key switch -- at a coefficient for more than one output) on rows on the
    mod-switch boundaries of its grid through tables on the first CMux's digit boundaries, every ciphertext, host and device memory.
    Float64 mode: against the CPU checker's chains; EXACT: against the unit calls composed, both implementations where the other is offered"""
    crs, keys, so, sg = _engines(p, 37, opts, exact=exact)
    rng = np.random.default_rng(38)
    checks = 0
    for name, nout, o, call, coef in _lut_calls(p):
        rows, kinds, sel = _lut_inputs(p, rng, nout)
        luts = lut_edge_tables(p, o)
        got = call(sg, luts, rows, sel)
        assert sg.last_kernel_name() == kernel, (name, sg.last_kernel_name())
        if exact:
            want = _lut_composed(sg, p, name, nout, luts, rows, sel, coef)
            assert sg.last_kernel_name() == kernel, (name, sg.last_kernel_name())
        else:
            want = np.stack([_lut_reference(p, so, name, nout, luts[sel[j]], rows[j], coef) for j in range(len(rows))])
        assert got.shape == want.shape
        for j in range(len(rows)):
            assert np.array_equal(got[j], want[j]), (name, "host memory", j, kinds[j])
        dev = call(sg, _t(luts), _t(rows), _t(sel)).cpu().numpy().view(np.uint32).reshape(want.shape)
        for j in range(len(rows)):
            assert np.array_equal(dev[j], want[j]), (name, "device memory", j, kinds[j])
        if exact and "exact_impl" in opts:
            sg.set_option("exact_impl", 1 - opts["exact_impl"])
            other = call(sg, luts, rows, sel)
            fx = opts["exact_impl"] == 0 and sg.get_metric("fx_available") == 1.0 and not opts.get("exact_kany")      # (exact_kany forces the integer kernel)
            assert ("fx_" in sg.last_kernel_name()) == fx, sg.last_kernel_name()
            assert np.array_equal(other, want), (name, "the other exact_impl", sg.last_kernel_name())
            sg.set_option("exact_impl", opts["exact_impl"])
        checks += want.shape[0] * want.shape[1]
    print(f"{EC.sid(p)} {kernel}: {checks} ciphertexts compared (each in host and in device memory)")
    sg.close()
