"""tests/decode_cases.py on the reference side (no GPU): the harness is tested here, and every law tests/test_gpu_decode.py holds the
engine to is first shown to hold for the reference's restatement on a slice of each set's rows.

  * the ladder and its (set, mode) pairs: each pair is run or listed as refused; the GPU file runs exactly the lists of decode_cases.py;
  * the row builder reaches every switched phase on every grid, and the key-edge exponents occur (on a noiseless stand-in, every row);
  * the laws accept that stand-in with error 0 and reject two mutants: a table read at phi~ + 1, and a sign flipped at psi = N;
  * the oracle's chain (test_noise_live_cpu.OracleChain, extended with gate_ops, gate3_ops and mux over the oracle) keeps every law on the CPU
    slice -- all edge and key rows plus every eighth exhaustive row -- of every set, shipped noise and noise-free; the noise-free maxima are the
    figures decode_cases.REF_MAX_E stores for the GPU test's 4x condition;
  * MKT_ARITH_EXACT: tests/ref_exact.py's rotations with the oracle's key switch, lut_random, on a slice trimmed by the cost of the schoolbook products."""
import numpy as np
import pytest

import decode_cases as D
import noise_cases as NC
import ref_exact as RX
import ref_gate3 as G3
import ref_lut as R
from helpers import O, mk, oracle_scheme
from test_noise_live_cpu import OracleChain, ReferenceSwitch

BASES = [e for e in D.QUIET_LADDER if e.noise == D.SHIPPED]
_made = {}


def made(entry):
    """-> (crs, keys, rows) of an entry, made once"""
    if entry.id not in _made:
        crs, keys = D.keys_of(entry)
        _made[entry.id] = (crs, keys, D.build_rows(entry.p, keys, NC.set_seed(entry.base, 7)))
    return _made[entry.id]


# ---- the lists -------------------------------------------------------------------------------------------------------------------------
def test_ladder_holds_every_set_twice():
    assert len(D.QUIET_LADDER) == 36 and len(D.BY_ID) == 36
    for e in D.QUIET_LADDER:
        assert e.reason and (e.p.alpha, e.p.beta) == ((0.0, 0.0) if e.noise == D.QUIET else (2.0 ** 17, e.p.beta)) and (e.noise == D.QUIET or e.p.beta > 0)
    assert {e.p.scheme for e in D.QUIET_LADDER} == {mk.CGGI, mk.LMSS, mk.CCS, mk.KMS, mk.KMS_BLOCK}
    assert {e.p.N for e in D.QUIET_LADDER} == {128, 256, 1024, 4096} and {e.p.nparty for e in D.QUIET_LADDER} == {1, 2, 4, 8, 16}


def test_every_pair_is_run_or_listed_as_refused():
    pairs = D.all_pairs()
    assert len(set(pairs)) == len(pairs)
    for e in D.QUIET_LADDER:
        modes = [(m, i) for (s, m, i) in pairs if s == e.id]
        assert modes == [(NC.F64, None), (NC.EXACT, "ntt")] + ([(NC.EXACT, "fx")] if D.fx_shape(e.p) else []), e.id
    assert set(D.RUN_PAIRS) | set(D.REFUSED) == set(pairs) and not set(D.RUN_PAIRS) & set(D.REFUSED)
    assert all(code in (-1, -2) for code in D.REFUSED.values())          # MKT_ERR_ARG, MKT_ERR_UNSUPPORTED
    assert sorted(D.REFUSED) == [(f"CGGIparam-n20-N256-k1-W64-{noise}", NC.EXACT, impl) for noise in (D.QUIET, D.SHIPPED) for impl in ("fx", "ntt")]
    assert sorted({D.BY_ID[s].base for s, m, i in pairs if i == "fx"}) == sorted(D.set_id(p) for p in (
        mk.CGGIparam.scaled(n=20, N=256), mk.CGGI_N1024_l2.scaled(n=10), mk.CGGIparam.scaled(n=6, N=4096), mk.CGGIparam.scaled(n=20, N=256, W=64), mk.KMS2party.scaled(n=16, N=256),
        mk.KMS2party_N1024_l2.scaled(n=12)))


def test_every_pair_is_run_on_the_gpu():
    """each list of decode_cases.py is, whole and in order, the parameter list of a test of tests/test_gpu_decode.py, all of it marked gpu"""
    import test_gpu_decode as G
    assert G.pytestmark.name == "gpu"
    lists = []
    for name in dir(G):
        fn = getattr(G, name)
        if name.startswith("test_") and callable(fn):
            lists += [list(mark.args[1]) for mark in getattr(fn, "pytestmark", []) if mark.name == "parametrize"]
    assert lists.count(D.RUN_PAIRS) == 2 and len(lists) == 3, "switch + tables and gates + mux run RUN_PAIRS; one more list: the twiddle sets"
    assert G.TWIDDLE_SETS in lists and {D.BY_ID[s].p.scheme for s in G.TWIDDLE_SETS} == {mk.CGGI, mk.LMSS, mk.CCS, mk.KMS, mk.KMS_BLOCK}


# ---- a noiseless stand-in --------------------------------------------------------------------------------------------------------------
class Ideal(ReferenceSwitch):
    """decode_cases.Engine with no noise at all: the switch of the reference side, and for every output the trivial ciphertext (zero mask) of the
    word the law expects.  shift: the table is read at phi~ + shift; flip_at_N: the output is negated where it reads psi = N"""

    def __init__(self, p, keys, shift=0, flip_at_N=False):
        super().__init__(p)
        self.keys, self.shift, self.flip = keys, shift, flip_at_N

    def _out(self, T, phi, coef):
        p = self.p
        phi = (np.asarray(phi) + self.shift) % (2 * p.N)
        v = NC.table_values(T, phi, coef, p.W)
        if self.flip:
            v = np.where((phi - coef) % (2 * p.N) == p.N, -v, v)
        out = np.zeros(v.shape + (p.lwe_len,), dtype=np.uint32)
        out[..., -1] = NC.value_words(v, p.W)
        return out

    def lut(self, T, ct):
        return self._out(T, D.reference_phase(self.p, self.keys, ct), 0)

    def lut_many(self, U, ct, nout):
        return self._out(U, D.reference_phase(self.p, self.keys, ct, nout)[:, None], np.arange(nout)[None, :])

    def lut_at(self, T, ct, coef, nu):
        return self._out(T, D.reference_phase(self.p, self.keys, ct, 1 << nu)[:, None], np.asarray(coef).astype(np.int64)[None, :])

    def _lin(self, lin):
        return self.lut(mk.sign_lut(self.p), lin)

    def gate_ops(self, ops, x, y, mem=None):
        return self._lin(np.stack([O.gate_linear(int(o) & 7, D._flag(x[j:j + 1], ops[j:j + 1], mk.OP_NOT_X)[0], D._flag(y[j:j + 1], ops[j:j + 1], mk.OP_NOT_Y)[0])
                                   for j, o in enumerate(ops)]))

    def gate3_ops(self, ops, x, y, z, mem=None):
        return self._lin(G3.linear3_rows(ops, x, y, z))

    def mux(self, s, a, b, mem=None):
        o1 = self._lin(np.stack([O.gate_linear(1, s[j], a[j]) for j in range(len(s))]))
        o2 = self._lin(np.stack([O.gate_linear(1, D.neg(s[j]), b[j]) for j in range(len(s))]))
        out = o1 + o2
        out[:, -1] += np.uint32(1 << 29)
        return out


def gate_laws(eng, p, keys, targets, seed, dense):
    return D.gate_laws(eng, p, keys, D.gate_inputs(p, keys, targets, seed, dense))


@pytest.mark.parametrize("entry", BASES, ids=lambda e: e.base)
def test_row_builder_reaches_every_phase_and_the_laws_accept_a_noiseless_engine(entry):
    p = entry.p
    _, keys, rows = made(entry)
    assert np.array_equal(NC.key_ones(p, keys), NC.key_ones(p, D.keys_of(D.BY_ID[entry.base + "-" + D.QUIET])[1])), "the noise-free set has the same secrets"
    n = {k: int((rows.kind == k).sum()) for k in np.unique(rows.kind)}
    if p.N == 4096:
        assert n["x1"] == 8192 and set(n) == {"x1", "edge", "key"}
    else:
        assert [n[f"x{o}"] for o in D.GRIDS] == [2 * p.N // o for o in D.GRIDS] and n["uniform"] == D.UNIFORM_ROWS
    if p.N == 256:
        assert 1150 <= len(rows.ct) <= 1250, len(rows.ct)
    eng = Ideal(p, keys)
    phis = D.switch_law(eng, p, keys, rows)                  # every multiple of o met on every grid built; key-edge exponents occur
    assert sorted(phis) == [1, 2, 4, 8]
    for call in NC.DECODE_CALLS:
        wrong, bits, emax, phi = D.table_law(eng, p, keys, rows, call, 5)
        assert (wrong, emax) == (0, 0.0) and bits >= len(rows.for_grid(D.grid_of(call), p.N)), call
        if p.N < 4096 or D.grid_of(call) == 1:
            assert D.reaches_every_phase(p, phi, D.grid_of(call)) and NC.reads_the_corners(p, phi)
    targets = D.gate_rows(rows, p.N)
    assert len(targets) >= 2 * p.N + 28
    for what, (wrong, outs, emax) in gate_laws(eng, p, keys, targets, 6, D.dense_codes(p)).items():
        assert (wrong, emax) == (0, 0.0) and outs >= len(targets), what


@pytest.mark.parametrize("mutant", ["table read at phi~ + 1", "sign flipped at psi = N"])
def test_the_laws_reject_mutants(mutant):
    entry = BASES[0]
    p = entry.p
    _, keys, rows = made(entry)
    eng = Ideal(p, keys, shift=1) if "+ 1" in mutant else Ideal(p, keys, flip_at_N=True)
    got = {call: D.table_law(eng, p, keys, rows, call, 5)[0] for call in NC.DECODE_CALLS}
    gates = gate_laws(eng, p, keys, D.gate_rows(rows, p.N), 6, True)
    print(mutant, got, gates)
    assert all(w > 0 for w in got.values()), got
    assert all(w > 0 for w, _, _ in gates.values()), gates
    if "psi = N" in mutant:                                 # one phase in 2N: caught only because the rows reach it
        assert got["lut_sign"] == int((D.reference_phase(p, keys, rows.ct) == p.N).sum()) >= 1


# ---- the oracle's chain ----------------------------------------------------------------------------------------------------------------
class Chain(OracleChain):
    """OracleChain plus the gate calls over the oracle: NOT! on the flagged inputs and gate (gate.jl), bootstrapping! of the three-input linear
    part (ref_gate3.oracle_gate3), and the native MUX as tests/test_gpu_multi.py oracle_mux restates it"""

    def gate_ops(self, ops, x, y, mem=None):
        return np.stack([self.so.gate(int(o) & 7, D._flag(x[j:j + 1], ops[j:j + 1], mk.OP_NOT_X)[0], D._flag(y[j:j + 1], ops[j:j + 1], mk.OP_NOT_Y)[0])
                         for j, o in enumerate(ops)])

    def gate3_ops(self, ops, x, y, z, mem=None):
        return G3.oracle_gate3(self.so, ops, x, y, z)

    def mux(self, s, a, b, mem=None):
        from test_gpu_multi import oracle_mux
        return np.stack([oracle_mux(self.so, self.p, s[j], a[j], b[j]) for j in range(len(s))])


# rows of the slice where the oracle is slow (eight and sixteen parties; M = 2048 transforms; three accumulator polynomials at N = 1024, whose
# slice would hold 540 rows): each case stays under about 10 s
SLICE_CAP = {"CCS16party-n2-N256-k16": 64, "KMS8party-n4-N256-k8": 110, "CGGIparam-n6-N4096-k1": 96, "CCS2party-n4-N4096-k2": 80, "KMS2party_N1024_l2-n12-N1024-k2": 180,
             "Blockparam_k2-n24-N1024-k2": 230}


def chain_figures(entry):
    p = entry.p
    crs, keys, rows = made(entry)
    eng = Chain(p, oracle_scheme(p, crs, keys))
    idx = D.cpu_slice(rows, SLICE_CAP.get(entry.base))
    fig = {}
    for call in NC.DECODE_CALLS:
        wrong, bits, emax, _ = D.table_law(eng, p, keys, rows, call, 11, idx)
        fig[call] = (wrong, bits, emax)
    targets = rows.ct[np.intersect1d(idx, rows.of_kind("x1", "edge", "key"))]
    fig.update(gate_laws(eng, p, keys, targets, 12, False))
    return fig, len(idx)


@pytest.mark.parametrize("entry", D.QUIET_LADDER, ids=lambda e: e.id)
def test_the_oracle_chain_keeps_every_law_on_the_cpu_slice(entry):
    fig, rows = chain_figures(entry)
    tables = max(v[2] for k, v in fig.items() if k in NC.DECODE_CALLS)
    gates = max(v[2] for k, v in fig.items() if k not in NC.DECODE_CALLS)
    print("REF", entry.id, "rows", rows, "tables", tables, "gates", gates, fig)
    assert rows >= 64
    for what, (wrong, bits, emax) in fig.items():
        assert wrong == 0 and emax < D.MARGIN and bits >= 64, (entry.id, what, wrong, bits, emax)
    if entry.noise == D.QUIET:
        stored = D.REF_MAX_E[entry.base]
        assert stored["tables"] >= tables > 0.98 * stored["tables"] and stored["gates"] >= gates > 0.98 * stored["gates"], (entry.id, tables, gates, stored)


# ---- MKT_ARITH_EXACT on the reference side -----------------------------------------------------------------------------------------------
class ExactChain(OracleChain):
    """lut on exact arithmetic: the oracle's modswitch and key switch around tests/ref_exact.py's rotation (every transform-domain product
    replaced by the schoolbook product mod 2^W) of ref_lut's table step"""

    def __init__(self, p, so, crs, keys):
        super().__init__(p, so)
        self.crs, self.keys = crs, keys

    def lut(self, T, ct):
        p, out = self.p, []
        for c in ct:
            at, bt = self.so.modswitch(c)
            acc = R.testvector(T, bt, p.W, self.so.kacc)
            if p.scheme == mk.CCS:
                acc = RX.ccs_blindrotate(p, self.keys, self.crs, at, acc)
            elif p.scheme in (mk.KMS, mk.KMS_BLOCK):
                acc = RX.kms_blindrotate(p, self.keys, self.crs, at, acc)
            else:
                acc = (RX.blindrotate_lmss if p.blk_len > 1 else RX.blindrotate)(p, self.keys[0].brk, at, acc)
            out.append(self.so.keyswitch(np.ascontiguousarray(acc, dtype=np.uint64)))
        return np.stack(out)


# rows of the EXACT slice: 64 where the schoolbook products allow it, fewer where one row costs 0.1 s and more (measured: 0.1 s at N = 1024,
# 0.4 s at n = 300, 1 s at N = 4096 and at sixteen parties, 3 s for CCS at N = 4096), so that a case takes about 5 s -- spread evenly over the
# CPU slice, so that exhaustive, edge and key rows all occur
EXACT_ROWS = {"CGGI_N1024_l2-n10-N1024-k1": 46, "CGGIparam-n10-N256-k4": 60, "CGGIparam-n6-N4096-k1": 5, "Blockparam-n300-N128-k3": 12,
              "Blockparam_k2-n24-N1024-k2": 8, "KMS2party_N1024_l2-n12-N1024-k2": 15, "KMS4party-n10-N256-k4": 34, "KMS8party-n4-N256-k8": 28,
              "KMS2partyblock-n24-N256-k2": 46, "CCS2party-n12-N256-k2": 57, "CCS4party-n6-N256-k4": 31, "CCS16party-n2-N256-k16": 5,
              "CCS2party-n4-N4096-k2": 3}
assert set(EXACT_ROWS) <= {e.base for e in BASES}


@pytest.mark.parametrize("entry", D.QUIET_LADDER, ids=lambda e: e.id)
def test_exact_rotations_keep_the_table_law_on_the_cpu_slice(entry):
    p = entry.p
    crs, keys, rows = made(entry)
    idx = D.cpu_slice(rows)
    idx = idx[np.linspace(0, len(idx) - 1, EXACT_ROWS.get(entry.base, 64)).astype(int)]
    eng = ExactChain(p, oracle_scheme(p, crs, keys), crs, keys)
    wrong, bits, emax, _ = D.table_law(eng, p, keys, rows, "lut_random", 11, idx)
    print("REF exact", entry.id, "rows", bits, "wrong", wrong, "max |e|", emax)
    assert bits == len(idx) and wrong == 0 and emax < D.MARGIN, (entry.id, wrong, emax)
