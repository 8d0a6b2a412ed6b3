"""Levelised gate-circuit evaluation on top of the batched gate primitive.

The reference's tests fold gates one at a time, a random gate per step (test/KMS.jl:29-34).  Here a circuit is a DAG of
two-input bootstrapped gates (gate.jl:1-53) and free NOTs (gate.jl:55-58); ALL gates of equal depth -- whatever their
type -- are evaluated in ONE engine call over all `B` independent input sets at once (mkt_gate_batch_gather: a per-gate op
code, operands picked by row index from a ciphertext pool that stays in HBM, NOTs folded into the gate's linear part), so a
level costs one round of launches however many gate kinds it mixes.

Three-input nodes (Circuit.MAJ3 / XOR3 / ...: one bootstrap each, mktfhe.h MKT_MAJ3 .. MKT_AE3) are a node kind of their own: the
three-input gates of a level are one contiguous pool region and one mkt_gate3_batch_gather call, so a level costs at most one
call per node kind.  ripple_adder_fa builds the adder from them: 2 bootstraps per bit instead of 5, one level per bit instead of 2.
"""
from collections import defaultdict

import numpy as np

from .params import NAND_OP, AND_OP, OR_OP, XOR_OP, XNOR_OP, NOR_OP, MAJ3_OP, MIN3_OP, XOR3_OP, XNOR3_OP, NAE3_OP, AE3_OP

_NOT = -1
_MUX = 6        # native three-input node (mkt_mux_batch_gather): nodes entry (_MUX, s, (a, b))
_G3 = 7         # three-input gate in one bootstrap (mkt_gate3_batch_gather): nodes entry (_G3, x, (y, z, code)), code MAJ3_OP .. AE3_OP
_KIND = {_MUX: 2, _G3: 1}      # pool order of the node kinds inside a level: two-input gates, three-input gates, native MUX nodes

# plaintext truth of the three-input codes, by number of true inputs (mktfhe.h)
_G3_TRUTH = {MAJ3_OP: (0, 0, 1, 1), MIN3_OP: (1, 1, 0, 0), XOR3_OP: (0, 1, 0, 1), XNOR3_OP: (1, 0, 1, 0), NAE3_OP: (0, 1, 1, 0), AE3_OP: (1, 0, 0, 1)}


class Circuit:
    def __init__(self):
        self.nodes = []      # (op, a, b) ; inputs: ("in", index, None)
        self.n_inputs = 0
        self.outputs = []

    def input(self):
        self.nodes.append(("in", self.n_inputs, None))
        self.n_inputs += 1
        return len(self.nodes) - 1

    def gate(self, op, a, b):
        assert 0 <= op <= 5 and 0 <= a < len(self.nodes) and 0 <= b < len(self.nodes)
        self.nodes.append((op, a, b))
        return len(self.nodes) - 1

    def NAND(self, a, b): return self.gate(NAND_OP, a, b)
    def AND(self, a, b): return self.gate(AND_OP, a, b)
    def OR(self, a, b): return self.gate(OR_OP, a, b)
    def XOR(self, a, b): return self.gate(XOR_OP, a, b)
    def XNOR(self, a, b): return self.gate(XNOR_OP, a, b)
    def NOR(self, a, b): return self.gate(NOR_OP, a, b)

    def NOT(self, a):
        self.nodes.append((_NOT, a, None))
        return len(self.nodes) - 1

    def MUX(self, s, a, b):
        """s ? a : b.  The reference has no MUX gate (gate.jl exports NAND..NOR, NOT!); this is the composite
        OR(AND(s, a), AND(NOT s, b)) of its gates: two levels, three bootstraps, the two ANDs in one batch."""
        return self.OR(self.AND(s, a), self.AND(self.NOT(s), b))

    def MUXN(self, s, a, b):
        """s ? a : b as ONE node: the engine's native MUX (two blind rotations + one key switch; mkt_mux_batch) instead of the three
        bootstraps of the composite.  One level deep."""
        assert all(0 <= v < len(self.nodes) for v in (s, a, b))
        self.nodes.append((_MUX, s, (a, b)))
        return len(self.nodes) - 1

    def gate3(self, op, a, b, c):
        """a three-input gate in ONE bootstrap (op = MAJ3_OP .. AE3_OP); NOTs on its inputs are folded into its code by Plan"""
        assert 0 <= op <= 5 and all(0 <= v < len(self.nodes) for v in (a, b, c))
        self.nodes.append((_G3, a, (b, c, op)))
        return len(self.nodes) - 1

    def MAJ3(self, a, b, c): return self.gate3(MAJ3_OP, a, b, c)
    def MIN3(self, a, b, c): return self.gate3(MIN3_OP, a, b, c)
    def XOR3(self, a, b, c): return self.gate3(XOR3_OP, a, b, c)
    def XNOR3(self, a, b, c): return self.gate3(XNOR3_OP, a, b, c)
    def NAE3(self, a, b, c): return self.gate3(NAE3_OP, a, b, c)
    def AE3(self, a, b, c): return self.gate3(AE3_OP, a, b, c)

    def output(self, w):
        self.outputs.append(w)
        return w

    def levels(self):
        """-> (depth per node, {level: {op: [node ids]}}) ; NOT and inputs cost no level; every three-input gate of a level is under
        the one key _G3 whatever its code"""
        depth = []
        for op, a, b in self.nodes:
            if op == "in":
                depth.append(0)
            elif op == _NOT:
                depth.append(depth[a])
            elif op in (_MUX, _G3):
                depth.append(1 + max(depth[a], depth[b[0]], depth[b[1]]))
            else:
                depth.append(1 + max(depth[a], depth[b]))
        sched = defaultdict(lambda: defaultdict(list))
        for i, (op, a, b) in enumerate(self.nodes):
            if op not in ("in", _NOT):
                sched[depth[i]][op].append(i)
        return depth, sched

    def plain(self, bits):
        """reference evaluation on plaintext bits: bits (n_inputs, ...) bool"""
        f = {0: lambda x, y: ~(x & y), 1: lambda x, y: x & y, 2: lambda x, y: x | y, 3: lambda x, y: x ^ y,
             4: lambda x, y: ~(x ^ y), 5: lambda x, y: ~(x | y)}
        v = []
        for op, a, b in self.nodes:
            if op == _MUX:
                v.append(np.where(v[a], v[b[0]], v[b[1]]))
            elif op == _G3:
                cnt = np.asarray(v[a], dtype=np.int8) + np.asarray(v[b[0]], dtype=np.int8) + np.asarray(v[b[1]], dtype=np.int8)
                v.append(np.array(_G3_TRUTH[b[2]], dtype=bool)[cnt])
            else:
                v.append(bits[a] if op == "in" else (~v[a] if op == _NOT else f[op](v[a], v[b])))
        return [v[w] for w in self.outputs]


def _cat(xs):
    if type(xs[0]).__module__.startswith("torch"):
        import torch
        return torch.cat(xs, 0)
    return np.concatenate(xs, 0)


def evaluate(circ: Circuit, inputs, gate_fn, not_fn, mux_fn=None, gate3_fn=None):
    """inputs: list of n_inputs arrays [B, lwe_len] (numpy or GPU tensors).  gate_fn(op, x, y) -> out is the
    batched gate (Scheme.gate), not_fn(x) -> negated COPY, mux_fn(s, a, b) -> out the native MUX (needed only for MUXN nodes),
    gate3_fn(ops, x, y, z) -> out the three-input gates with one uint8 code per row (Scheme.gate3_ops; needed only for three-input
    nodes: the codes carry no NOT flags, negated operands come from not_fn).
    Returns the output ciphertext arrays [B, lwe_len].
    Number of gate_fn calls = number of distinct (level, op) pairs, independent of the circuit width; one gate3_fn call per level
    that holds three-input gates."""
    assert len(inputs) == circ.n_inputs
    depth, sched = circ.levels()
    val = [None] * len(circ.nodes)

    def resolve(i):
        if val[i] is None:
            op, a, _ = circ.nodes[i]
            val[i] = inputs[a] if op == "in" else not_fn(resolve(a))
        return val[i]

    B = inputs[0].shape[0] if circ.n_inputs else 0
    for lvl in sorted(sched):
        for op, ids in sched[lvl].items():
            x = _cat([resolve(circ.nodes[i][1]) for i in ids])
            if op == _MUX:
                out = mux_fn(x, _cat([resolve(circ.nodes[i][2][0]) for i in ids]), _cat([resolve(circ.nodes[i][2][1]) for i in ids]))
            elif op == _G3:
                ops = np.repeat(np.array([circ.nodes[i][2][2] for i in ids], dtype=np.uint8), B)
                if type(x).__module__.startswith("torch"):
                    import torch
                    ops = torch.from_numpy(ops).to(x.device)
                out = gate3_fn(ops, x, _cat([resolve(circ.nodes[i][2][0]) for i in ids]), _cat([resolve(circ.nodes[i][2][1]) for i in ids]))
            else:
                y = _cat([resolve(circ.nodes[i][2]) for i in ids])
                out = gate_fn(op, x, y)
            for j, i in enumerate(ids):
                val[i] = out[j * B:(j + 1) * B]
    return [resolve(w) for w in circ.outputs]


class Plan:
    """The launch schedule of a circuit over B instances: one mkt_gate_batch_gather per level (plus one mkt_gate3_batch_gather /
    mkt_mux_batch_gather for a level that holds three-input gates / native MUX nodes).  Pool rows: node slot s,
    instance b -> row s * B + b; slots 0 .. n_inputs-1 are the inputs, then the gates level by level (so a level's outputs
    are one contiguous region of the pool, each node kind a contiguous part of it); NOT nodes own no slot -- they resolve to
    (slot of their source, negated), folded into the reading gate's code."""

    def __init__(self, circ: Circuit, B):
        depth, sched = circ.levels()
        self.B, self.n_inputs = B, circ.n_inputs
        slot, neg = [None] * len(circ.nodes), [False] * len(circ.nodes)
        for i, (op, a, _) in enumerate(circ.nodes):
            if op == "in":
                slot[i] = a
        nslots = circ.n_inputs
        order = []
        for lvl in sorted(sched):
            ids = sorted((i for lst in sched[lvl].values() for i in lst), key=lambda i: (_KIND.get(circ.nodes[i][0], 0), i))   # two-input gates, three-input gates, native MUX nodes: each kind one contiguous region of the pool
            for i in ids:
                slot[i] = nslots
                nslots += 1
            order.append(ids)

        def src(i):                      # -> (slot, negated) through chains of NOTs
            n = False
            while circ.nodes[i][0] == _NOT:
                n = not n
                i = circ.nodes[i][1]
            return slot[i], n

        inst = np.arange(B, dtype=np.uint32)
        self.levels = []        # two-input gates of a level: (first slot, count, ops, ix, iy)
        self.mux_levels = []    # its native MUX nodes, if any: (first slot, count, is, ia, ib, not_ab) or None
        self.gate3_levels = []  # its three-input gates, if any: (first slot, count, ops, ix, iy, iz) or None
        for ids in order:
            g2 = [i for i in ids if circ.nodes[i][0] not in (_MUX, _G3)]
            g3 = [i for i in ids if circ.nodes[i][0] == _MUX]
            t3 = [i for i in ids if circ.nodes[i][0] == _G3]
            ops = np.empty((len(g2), B), dtype=np.uint8)
            ix = np.empty((len(g2), B), dtype=np.uint32)
            iy = np.empty((len(g2), B), dtype=np.uint32)
            for j, i in enumerate(g2):
                op, a, b = circ.nodes[i]
                (sa, na), (sb, nb) = src(a), src(b)
                ops[j] = op | (8 if na else 0) | (16 if nb else 0)
                ix[j] = sa * B + inst
                iy[j] = sb * B + inst
            self.levels.append((slot[g2[0]] if g2 else 0, len(g2), ops.ravel(), ix.ravel(), iy.ravel()))
            if t3:
                o3 = np.empty((len(t3), B), dtype=np.uint8)
                jx, jy, jz = (np.empty((len(t3), B), dtype=np.uint32) for _ in range(3))
                for j, i in enumerate(t3):
                    _, a, (b, c, code) = circ.nodes[i]
                    (sa, na), (sb, nb), (sc, nc) = src(a), src(b), src(c)
                    o3[j] = code | (8 if na else 0) | (16 if nb else 0) | (32 if nc else 0)
                    jx[j], jy[j], jz[j] = sa * B + inst, sb * B + inst, sc * B + inst
                self.gate3_levels.append((slot[t3[0]], len(t3), o3.ravel(), jx.ravel(), jy.ravel(), jz.ravel()))
            else:
                self.gate3_levels.append(None)
            if g3:
                js, ja, jb = (np.empty((len(g3), B), dtype=np.uint32) for _ in range(3))
                fl = np.empty((len(g3), B), dtype=np.uint8)
                for j, i in enumerate(g3):
                    _, s_, (a, b) = circ.nodes[i]
                    (ss, ns), (sa, na), (sb, nb) = src(s_), src(a), src(b)
                    if ns:                                   # MUX(NOT s, a, b) = MUX(s, b, a)
                        (sa, na), (sb, nb) = (sb, nb), (sa, na)
                    js[j], ja[j], jb[j] = ss * B + inst, sa * B + inst, sb * B + inst
                    fl[j] = (1 if na else 0) | (2 if nb else 0)
                self.mux_levels.append((slot[g3[0]], len(g3), js.ravel(), ja.ravel(), jb.ravel(), fl.ravel()))
            else:
                self.mux_levels.append(None)
        self.rows = nslots * B
        self.gates = (sum(n for _, n, _, _, _ in self.levels) + sum(m[1] for m in self.mux_levels if m) + sum(t[1] for t in self.gate3_levels if t)) * B
        self.outputs = [src(w) for w in circ.outputs]


def evaluate_on(circ: Circuit, inputs, scheme, plan: Plan = None):
    """evaluate with an engine Scheme (GPU tensors or numpy arrays): one engine call per LEVEL and node kind (all two-input gate
    kinds merged; all three-input codes merged)."""
    B = inputs[0].shape[0]
    plan = plan or Plan(circ, B)
    assert plan.B == B and len(inputs) == plan.n_inputs
    lwe_len = inputs[0].shape[1]
    on_gpu = type(inputs[0]).__module__.startswith("torch")
    if on_gpu:
        import torch
        dev = inputs[0].device
        pool = torch.empty((plan.rows, lwe_len), dtype=inputs[0].dtype, device=dev)
        up = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)   # noqa: E731
    else:
        pool = np.empty((plan.rows, lwe_len), dtype=np.uint32)
        up = lambda a: a                                                                              # noqa: E731
    for s, x in enumerate(inputs):
        pool[s * B:(s + 1) * B] = x
    for (slot0, ngates, ops, ix, iy), mx, t3 in zip(plan.levels, plan.mux_levels, plan.gate3_levels):
        if ngates:
            scheme.gate_gather(up(ops), pool, up(ix), up(iy), pool[slot0 * B:(slot0 + ngates) * B])
        if t3:
            t0, nt, o3, jx, jy, jz = t3
            scheme.gate3_gather(up(o3), pool, up(jx), up(jy), up(jz), pool[t0 * B:(t0 + nt) * B])
        if mx:
            m0, nm, js, ja, jb, fl = mx
            scheme.mux_gather(pool, up(js), up(ja), up(jb), pool[m0 * B:(m0 + nm) * B], not_ab=up(fl))
    res = []
    for sl, negated in plan.outputs:
        o = pool[sl * B:(sl + 1) * B]
        o = o.clone() if on_gpu else o.copy()
        if negated:
            scheme.not_(o)
        res.append(o)
    return res


def evaluate_sharded(circ: Circuit, inputs, multi):
    """The B instances of a circuit sharded over the shards of a MultiScheme (one process, all GPUs): gates of different instances
    never meet, so every shard evaluates the WHOLE circuit on its contiguous slice of the instances (mkt_multi_shard_range), one host
    thread per shard, ciphertexts of a slice staying on that shard's device between levels; no exchange between shards.  inputs:
    host arrays, or GPU tensors (then all shards must sit on the tensors' device: logical shards)."""
    import threading
    B, n = inputs[0].shape[0], multi.nshards
    parts, errs = [None] * n, []

    def work(i):
        try:
            lo, hi = multi.shard_range(B, i)
            if lo < hi:
                sh = multi.shard(i)
                own = sh.get_stream()              # the shard's own stream: put back afterwards
                sh._user_stream = False            # GPU tensors: the shard enqueues on torch's current stream of its device, like Scheme
                try:
                    parts[i] = evaluate_on(circ, [x[lo:hi] for x in inputs], sh)
                    sh.synchronize()
                finally:
                    sh.set_stream(own or None)
        except Exception as e:      # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(1, n)]
    for t in th:
        t.start()
    work(0)
    for t in th:
        t.join()
    if errs:
        raise errs[0]
    done = [p for p in parts if p is not None]
    return [_cat([p[w] for p in done]) for w in range(len(circ.outputs))]


def ripple_adder(nbits):
    """nbits-bit adder: inputs a0..a{n-1}, b0..b{n-1} (LSB first), outputs s0..s{n-1}, carry"""
    c = Circuit()
    a = [c.input() for _ in range(nbits)]
    b = [c.input() for _ in range(nbits)]
    carry = None
    for i in range(nbits):
        p = c.XOR(a[i], b[i])
        g = c.AND(a[i], b[i])
        if carry is None:
            c.output(p); carry = g
        else:
            c.output(c.XOR(p, carry))
            carry = c.OR(g, c.AND(p, carry))
    c.output(carry)
    return c


def ripple_adder_fa(nbits):
    """the same adder as ripple_adder (same inputs and outputs) from full adders of three-input gates: a half adder (XOR, AND) at
    bit 0, then sum = XOR3(a, b, carry) and carry = MAJ3(a, b, carry), one bootstrap each: 2 nbits bootstraps over nbits levels"""
    c = Circuit()
    a = [c.input() for _ in range(nbits)]
    b = [c.input() for _ in range(nbits)]
    carry = None
    for i in range(nbits):
        if carry is None:
            c.output(c.XOR(a[i], b[i])); carry = c.AND(a[i], b[i])
        else:
            c.output(c.XOR3(a[i], b[i], carry)); carry = c.MAJ3(a[i], b[i], carry)
    c.output(carry)
    return c
