"""Three-input gates in one bootstrap (mktfhe.h MKT_MAJ3 .. MKT_AE3) on the CPU: the linear parts on noiseless phases, the circuit
scheduler's three-input node kind (codes, indices, NOTs folded into the codes, one call per level and node kind), the full-adder
ripple adder, and a small circuit evaluated word for word through an oracle-backed pool evaluator."""
import itertools

import numpy as np
import pytest

from helpers import keygen, mk, oracle_scheme
from ref_gate3 import TRUTH, linear3, oracle_gate3, plain3
from mktfhe_amd import circuit as CI


def test_codes_and_flags_match_the_header():
    assert (mk.MAJ3_OP, mk.MIN3_OP, mk.XOR3_OP, mk.XNOR3_OP, mk.NAE3_OP, mk.AE3_OP) == tuple(range(6))
    assert (mk.OP_NOT_X, mk.OP_NOT_Y, mk.OP_NOT_Z) == (8, 16, 32)
    import os
    from helpers import ROOT
    hdr = open(os.path.join(ROOT, "include", "mktfhe.h")).read()
    assert "MKT_MAJ3 = 0, MKT_MIN3 = 1, MKT_XOR3 = 2, MKT_XNOR3 = 3, MKT_NAE3 = 4, MKT_AE3 = 5" in hdr
    assert "MKT_OP_NOT_Z = 32" in hdr


def _sign_bit(phase):
    """what a noiseless sign bootstrap decides: true iff the phase lies in (0, 1/2) of the torus"""
    p = int(phase) & 0xFFFFFFFF
    assert p not in (0, 1 << 31), "phase on a decision boundary"
    return p < (1 << 31)


@pytest.mark.parametrize("code", range(6))
def test_linear_parts_on_noiseless_phases_give_the_truth_tables(code):
    """x, y, z = +-2^29 trivial ciphertexts (mask 0, b word only): every code with every NOT flag combination gives the issue's truth
    table after the sign decision, and the plaintext evaluator of the circuit module agrees"""
    enc = lambda bit: np.array([0, 0, (1 << 29) if bit else (0 - (1 << 29)) & 0xFFFFFFFF], dtype=np.uint32)   # noqa: E731
    for flags in range(8):
        op = code | (flags << 3)
        for a, b, c in itertools.product((0, 1), repeat=3):
            lin = linear3(op, enc(a), enc(b), enc(c))
            assert not lin[:2].any()                         # the mask words stay zero
            a2, b2, c2 = a ^ (flags & 1), b ^ ((flags >> 1) & 1), c ^ ((flags >> 2) & 1)
            want = bool(TRUTH[code][a2 + b2 + c2])
            assert _sign_bit(lin[-1]) == want, (code, flags, a, b, c)
            assert plain3(np.array([op]), [a], [b], [c])[0] == want
            # circuit.plain of one node with the NOTs as explicit nodes
            circ = CI.Circuit(); u, v, w = circ.input(), circ.input(), circ.input()
            nu = circ.NOT(u) if flags & 1 else u
            nv = circ.NOT(v) if flags & 2 else v
            nw = circ.NOT(w) if flags & 4 else w
            circ.output(circ.gate3(code, nu, nv, nw))
            assert bool(circ.plain(np.array([[a], [b], [c]], dtype=bool))[0][0]) == want
    # the margins: 1/8 for the majority family, 1/4 for the parity family
    margins = set()
    for a, b, c in itertools.product((0, 1), repeat=3):
        ph = int(linear3(code, enc(a), enc(b), enc(c))[-1])
        ph = ph - (1 << 32) if ph >= (1 << 31) else ph
        margins.add(min(abs(ph), (1 << 31) - abs(ph)))
    assert margins == ({1 << 30} if code in (2, 3) else {1 << 29})           # distance to the nearer decision boundary, 0 or 1/2


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_full_adder_ripple_adder_adds(n):
    """Circuit.plain of ripple_adder_fa(n) == integer addition on EVERY input, and equals ripple_adder(n) output by output"""
    c, ref = CI.ripple_adder_fa(n), CI.ripple_adder(n)
    assert c.n_inputs == ref.n_inputs == 2 * n and len(c.outputs) == len(ref.outputs) == n + 1
    vals = np.arange(1 << (2 * n))
    bits = np.array([(vals >> i) & 1 for i in range(2 * n)], dtype=bool)
    outs = c.plain(bits)
    got = sum(o.astype(np.int64) << i for i, o in enumerate(outs))
    assert np.array_equal(got, (vals & ((1 << n) - 1)) + (vals >> n))
    for o, r in zip(outs, ref.plain(bits)):
        assert np.array_equal(o, r)


def _ncalls(plan):
    return sum((1 if l[1] else 0) + (1 if m else 0) + (1 if t else 0) for l, m, t in zip(plan.levels, plan.mux_levels, plan.gate3_levels))


def test_plan_of_the_full_adder_ripple_adder():
    """8 levels, 16 B gates, one engine call per level; level 1 the half adder (XOR, AND), levels 2..8 one XOR3 and one MAJ3 each, as one
    contiguous pool region read by row index (slot * B + instance)"""
    B = 3
    circ = CI.ripple_adder_fa(8)
    plan = CI.Plan(circ, B)
    depth, sched = circ.levels()
    assert len(plan.levels) == max(depth) == 8 and plan.gates == 16 * B
    assert _ncalls(plan) == 8
    inst = np.arange(B, dtype=np.uint32)
    a_slot, b_slot = list(range(8)), list(range(8, 16))
    slot0, n2, ops, ix, iy = plan.levels[0]
    assert (slot0, n2) == (16, 2) and plan.gate3_levels[0] is None and plan.mux_levels[0] is None
    assert np.array_equal(ops, np.repeat([mk.XOR_OP, mk.AND_OP], B).astype(np.uint8))
    assert np.array_equal(ix, np.concatenate([a_slot[0] * B + inst] * 2)) and np.array_equal(iy, np.concatenate([b_slot[0] * B + inst] * 2))
    carry = 17                                       # slot of the half adder's AND
    for lvl in range(1, 8):
        assert plan.levels[lvl][1] == 0 and plan.mux_levels[lvl] is None
        t0, nt, o3, jx, jy, jz = plan.gate3_levels[lvl]
        assert (t0, nt) == (16 + 2 * lvl, 2)
        assert np.array_equal(o3, np.repeat([mk.XOR3_OP, mk.MAJ3_OP], B).astype(np.uint8))
        assert np.array_equal(jx, np.concatenate([a_slot[lvl] * B + inst] * 2))
        assert np.array_equal(jy, np.concatenate([b_slot[lvl] * B + inst] * 2))
        assert np.array_equal(jz, np.concatenate([carry * B + inst] * 2))
        carry = t0 + 1
    assert plan.rows == (16 + 16) * B
    assert plan.outputs == [(16, False)] + [(16 + 2 * l, False) for l in range(1, 8)] + [(31, False)]


def test_plan_folds_nots_into_three_input_codes():
    """NOTs (and chains of them) on any input of a three-input node become its MKT_OP_NOT_X / _Y / _Z bits; a level mixing two-input
    gates, three-input gates and native MUX nodes puts each kind in its own contiguous region and costs one call per kind"""
    B = 2
    c = CI.Circuit(); a, b, d = c.input(), c.input(), c.input()
    borrow = c.MAJ3(c.NOT(a), b, d)                              # a subtractor's borrow
    t = c.AE3(c.NOT(c.NOT(a)), c.NOT(b), c.NOT(d))
    x = c.XOR(a, b)
    m = c.MUXN(a, b, d)
    c.output(borrow); c.output(t); c.output(x); c.output(m); c.output(c.NAE3(borrow, c.NOT(t), x))
    plan = CI.Plan(c, B)
    assert len(plan.levels) == 2 and _ncalls(plan) == 4 and plan.gates == 5 * B
    slot0, n2, ops, _, _ = plan.levels[0]
    assert (slot0, n2) == (3, 1)                                  # XOR first ...
    t0, nt, o3, jx, jy, jz = plan.gate3_levels[0]
    assert (t0, nt) == (4, 2)                                     # ... then the three-input gates ...
    assert plan.mux_levels[0][0] == 6                             # ... then the native MUX
    assert np.array_equal(o3, np.repeat([mk.MAJ3_OP | mk.OP_NOT_X, mk.AE3_OP | mk.OP_NOT_Y | mk.OP_NOT_Z], B).astype(np.uint8))
    t0, nt, o3, jx, jy, jz = plan.gate3_levels[1]
    assert (t0, nt) == (7, 1) and np.array_equal(o3, np.full(B, mk.NAE3_OP | mk.OP_NOT_Y, np.uint8))
    inst = np.arange(B, dtype=np.uint32)
    assert np.array_equal(jx, 4 * B + inst) and np.array_equal(jy, 5 * B + inst) and np.array_equal(jz, 3 * B + inst)
    with pytest.raises(AssertionError):
        c.gate3(6, a, b, d)                                       # AND3 / OR3 are not one-bootstrap gates


def test_two_input_circuits_plan_as_before():
    """guard: the adder of two-input gates keeps its schedule (37 gates over 15 levels) and has no three-input level"""
    for B in (1, 4):
        plan = CI.Plan(CI.ripple_adder(8), B)
        assert len(plan.levels) == 15 and plan.gates == 37 * B
        assert all(n > 0 for _, n, _, _, _ in plan.levels) and all(m is None for m in plan.mux_levels)      # one two-input call per level
        depth, _ = CI.ripple_adder(8).levels()
        assert max(depth) == 15


def test_full_adder_circuit_through_an_oracle_pool_evaluator():
    """evaluate_on with an oracle-backed stand-in for the engine (gate_gather / gate3_gather over the pool, NOT flags in the codes) gives the
    same words as evaluate with explicit NOT copies and gate3_fn = the oracle's restatement; it decrypts to a + b; a circuit with
    negated three-input operands too"""
    p = mk.CGGIparam.scaled(n=16, N=128)
    crs, keys = keygen(p, 81)
    so = oracle_scheme(p, crs, keys)
    neg = lambda v: (0 - v.astype(np.int64)).astype(np.uint32)   # noqa: E731

    class OracleAsScheme:
        calls = []

        def gate_gather(self, ops, pool, ix, iy, out):
            self.calls.append(("g2", len(ops)))
            for j in range(len(ops)):
                a = neg(pool[ix[j]]) if ops[j] & 8 else pool[ix[j]]
                b = neg(pool[iy[j]]) if ops[j] & 16 else pool[iy[j]]
                out[j] = so.gate(int(ops[j] & 7), a, b)
            return out

        def gate3_gather(self, ops, pool, ix, iy, iz, out):
            self.calls.append(("g3", len(ops)))
            out[:] = oracle_gate3(so, ops, pool[ix], pool[iy], pool[iz])
            return out

        def not_(self, x):
            x[...] = neg(x)
            return x

    B = 3
    rng = np.random.default_rng(82)
    c2 = CI.Circuit(); u, v, w = c2.input(), c2.input(), c2.input()
    c2.output(c2.MAJ3(c2.NOT(u), v, w)); c2.output(c2.NOT(c2.XNOR3(u, c2.NOT(v), c2.NOT(c2.NOT(w)))))
    for circ in (CI.ripple_adder_fa(3), c2):
        bits = rng.integers(0, 2, (circ.n_inputs, B)).astype(bool)
        inputs = [np.stack([mk.lwe_encrypt(int(bits[i, j]), keys[0], p, deterministic_seed=8200 + 10 * i + j) for j in range(B)]) for i in range(circ.n_inputs)]
        fake = OracleAsScheme(); fake.calls = []
        plan = CI.Plan(circ, B)
        outs = CI.evaluate_on(circ, inputs, fake, plan)
        depth, _ = circ.levels()
        assert len(fake.calls) == max(depth) and sum(n for _, n in fake.calls) == plan.gates
        ref = CI.evaluate(circ, inputs, lambda op, x, y: so.gate_batch(op, x, y), neg, gate3_fn=lambda ops, x, y, z: oracle_gate3(so, ops, x, y, z))
        for o, r, want in zip(outs, ref, circ.plain(bits)):
            assert np.array_equal(o, r)
            assert np.array_equal(mk.lwe_decrypt(o, keys[0], p), want)
