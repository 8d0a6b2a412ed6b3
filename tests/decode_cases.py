"""Law C of tests/noise_cases.py -- every output bit is the sign of the table read at the exactly computed switched phase -- taken from the
three shipped full-size sets to every scheme, arithmetic mode and kernel family, on ROWS OF PLAIN 32-BIT WORDS instead of encryptions.

phi~ is a function of a row and the keys, so the law needs no encryption and no margin argument: at the small sets below the output error of
a bootstrap stays far under the decision margin 1/8 (measured on the reference side: REF_MAX_E), and rows can be built so that EVERY switched
phase t in [0, 2N) is met, with the rounding edges of the switch at key positions that hold a one.  Nothing of oracle/ decides an expected
bit: the oracle supplies only the LINEAR PART of a gate (gate_linear, linear3_rows), which is a sum of words.

The harness is shared by tests/test_decode_cpu.py (the reference side, a slice of each set's rows, and the harness's own tests) and
tests/test_gpu_decode.py (the engine, every row).  Keys, phases, tables and errors are those of tests/noise_cases.py; nothing is restated."""
from typing import NamedTuple

import numpy as np

import helpers as H
import noise_cases as NC
import ref_gate3 as G3
from helpers import O
from noise_cases import EXACT, F64, mk

MARGIN = 1.0 / 16                   # half the decision margin 1/8: the stated bound on |e| of every output
DEVICE_OVER_REFERENCE = 4.0         # noise-free sets: the device's max |e| against the reference's on the CPU slice.  4: the GPU sample is about
                                    # ten times the slice, so its maximum lies higher, and a lost gadget digit costs a factor of at least 2^logB
SHIPPED, QUIET = "shipped", "quiet"
GRIDS = (1, 2, 4, 8)
UNIFORM_ROWS = 200


class Entry(NamedTuple):
    p: object               # the parameter set as the tests run it (noise included)
    base: str               # id of the set, without the noise
    noise: str              # SHIPPED or QUIET (alpha = beta = 0: what is left is rounding)
    reason: str

    @property
    def id(self):
        return f"{self.base}-{self.noise}"


def set_id(p):
    return f"{p.name}-n{p.n}-N{p.N}-k{p.k}" + ("" if p.W == getattr(mk, p.name).W else f"-W{p.W}")


# the sets of the issue, named as tests/test_gpu_parity.py's SMALL names them, each with what it is there for
_BASE = [
    (mk.CGGIparam.scaled(n=20, N=256), "CGGI, one mask polynomial: blindrotate_k1_kernel, fx_blindrotate_kernel, exact_blindrotate_kernel"),
    (mk.CGGI_N1024_l2.scaled(n=10), "CGGI at the headline shape N = 1024, l = 2: the specialised rotation instantiation"),
    (mk.CGGIparam.scaled(n=16, N=256, k=2), "RLWE length 2: blindrotate_kr_kernel / the grouped kernel, exact_blindrotate_kr_kernel"),
    (mk.CGGIparam.scaled(n=10, N=256, k=4), "RLWE length 4: blindrotate_kany_kernel, exact_blindrotate_kany_kernel"),
    (mk.CGGIparam.scaled(n=6, N=4096), "the largest ring: M = 2048 transforms"),
    (mk.CGGIparam.scaled(n=20, N=256, W=64), "CGGI on the 64-bit ring (Float64 only: MKT_ARITH_EXACT serves CGGI on the 32-bit ring)"),
    (mk.Blockparam.scaled(n=30, N=256, blk_d=10), "LMSS, block length 3: the block rotation"),
    (mk.Blockparam.scaled(n=300, N=128, blk_d=100, k=3), "LMSS with n > N: the key switch copies whole components"),
    (mk.Blockparam_k2.scaled(n=24, blk_d=8), "LMSS at RLWE length 2, N = 1024: the grouped block kernel"),
    (mk.KMS2party.scaled(n=16, N=256), "KMS on the 64-bit ring, Float64: blindrotate_k1_kernel phase 1 + kms_phase2_kernel; EXACT on both implementations"),
    (mk.KMS2party_N1024_l2.scaled(n=12), "KMS at the benchmark's shape N = 1024, l = 2"),
    (mk.KMS4party.scaled(n=10, N=256), "four parties, gadget lengths 5 / 2 / 7"),
    (mk.KMS8party.scaled(n=4, N=256), "eight parties"),
    (mk.KMS2partyblock.scaled(n=24, N=256, blk_d=8), "KMS_block: block-binary phase 1"),
    (mk.CCS2party.scaled(n=12, N=256), "CCS: UniEnc hybrid product, ccs_blindrotate_kernel / ccs_pipe_kernel, exact_ccs_kernel"),
    (mk.CCS4party.scaled(n=6, N=256), "CCS, four parties: a gadget that drops no bit (W = l logB)"),
    (mk.CCS16party.scaled(n=2, N=256), "CCS, sixteen parties, l = 12: the noisiest set of the ladder"),
    (mk.CCS2party.scaled(n=4, N=4096), "CCS at the largest ring"),
]
QUIET_LADDER = [Entry(p if noise == SHIPPED else p.scaled(alpha=0.0, beta=0.0), set_id(p), noise, why) for p, why in _BASE for noise in (SHIPPED, QUIET)]
BY_ID = {e.id: e for e in QUIET_LADDER}


def fx_shape(p):
    """the shapes whose EXACT rotation the Float64 pipe can serve (context.cpp fx_shape, rot_plan.h fx_supported), restated: CGGI at RLWE length 1
    and KMS, gadget length 2 or 3, M = 64 .. 2048.  Whether it DOES serve depends on the loaded keys (the proven bound, metric fx_available):
    the GPU test asserts that it certifies every key set of this ladder"""
    return ((p.scheme == mk.CGGI and p.k == 1) or p.scheme == mk.KMS) and p.l_gsw in (2, 3) and 64 <= p.N // 2 <= 2048


# every (set, arithmetic mode, EXACT implementation) is in exactly one of the two: run, or refused by the library with the code stated here
# (mktfhe.h MKT_ERR_*), which the GPU test asserts -- no pair is skipped.  MKT_ARITH_EXACT evaluates CGGI on the 32-bit ring only (context.cpp
# exact_gate_ok): MKT_ERR_UNSUPPORTED for the 64-bit set, on either implementation; every other set is served in both modes
UNSUPPORTED = -2
REFUSED = {(e.id, EXACT, impl): UNSUPPORTED for e in QUIET_LADDER if e.p.scheme == mk.CGGI and e.p.W == 64 for impl in ("ntt", "fx")}      # (entry id, mode, impl) -> code


def all_pairs():
    return [(e.id, mode, impl) for e in QUIET_LADDER for mode, impl in
            [(F64, None), (EXACT, "ntt")] + ([(EXACT, "fx")] if fx_shape(e.p) else [])]


RUN_PAIRS = [c for c in all_pairs() if c not in REFUSED]
GATE_PAIRS = RUN_PAIRS              # laws 3 and 4 run wherever law 2 runs

# the reference's max |e| on the CPU slice of each noise-free set (tests/test_decode_cpu.py recomputes and holds them): over every call of
# NC.DECODE_CALLS ("tables") and over gate_ops, gate3_ops and mux ("gates"); the figure stored is the measured one, rounded up in the third digit
REF_MAX_E = {
    "CGGIparam-n20-N256-k1": {"tables": 0.000208, "gates": 0.000148},                   # measured 0.000207874, 0.000147531
    "CGGI_N1024_l2-n10-N1024-k1": {"tables": 0.00123, "gates": 0.00105},              # measured 0.00122036, 0.00104466
    "CGGIparam-n16-N256-k2": {"tables": 0.000297, "gates": 0.000224},                   # measured 0.000296565, 0.000223584
    "CGGIparam-n10-N256-k4": {"tables": 0.000455, "gates": 0.00034},                   # measured 0.000454438, 0.000339825
    "CGGIparam-n6-N4096-k1": {"tables": 0.00069, "gates": 0.000638},                   # measured 0.000689988, 0.000637393
    "CGGIparam-n20-N256-k1-W64": {"tables": 0.000193, "gates": 0.000158},               # measured 0.000192415, 0.000157338
    "Blockparam-n30-N256-k1": {"tables": 0.000177, "gates": 0.000129},                  # measured 0.000176628, 0.000128536
    "Blockparam-n300-N128-k3": {"tables": 0.000105, "gates": 7.14e-05},                 # measured 0.000104733, 7.13791e-05
    "Blockparam_k2-n24-N1024-k2": {"tables": 0.000598, "gates": 0.00035},              # measured 0.00059799, 0.000349568
    "KMS2party-n16-N256-k2": {"tables": 0.000848, "gates": 0.000683},                   # measured 0.000847581, 0.000682527
    "KMS2party_N1024_l2-n12-N1024-k2": {"tables": 0.0164, "gates": 0.0121},         # measured 0.0163716, 0.012084
    "KMS4party-n10-N256-k4": {"tables": 0.000615, "gates": 0.000479},                   # measured 0.000614578, 0.000478811
    "KMS8party-n4-N256-k8": {"tables": 0.00179, "gates": 0.000477},                    # measured 0.00178909, 0.000476445
    "KMS2partyblock-n24-N256-k2": {"tables": 0.000855, "gates": 0.000651},              # measured 0.000854625, 0.000650188
    "CCS2party-n12-N256-k2": {"tables": 0.000313, "gates": 0.000273},                   # measured 0.000312262, 0.000272863
    "CCS4party-n6-N256-k4": {"tables": 0.000394, "gates": 0.000293},                    # measured 0.000393052, 0.000292674
    "CCS16party-n2-N256-k16": {"tables": 0.000688, "gates": 0.000432},                  # measured 0.000687363, 0.000431632
    "CCS2party-n4-N4096-k2": {"tables": 0.00102, "gates": 0.000708},                   # measured 0.00101508, 0.000707707
}


def pair_id(c):
    return NC.case_id(c)


def keys_of(entry):
    """-> (crs or None, [PartyKeys] with every evaluation key, made on the CPU): the same words for the oracle and for the engine"""
    return H.keygen(entry.p, NC.set_seed(entry.base) % (1 << 31))


# ---- rows ------------------------------------------------------------------------------------------------------------------------------
def shift_of(N):
    """the bits the mod switch drops: 32 - (log2 N + 1)"""
    return 32 - (N.bit_length() - 1) - 1


class Rows(NamedTuple):
    ct: np.ndarray          # (R, lwe_len) uint32: plain words, not encryptions
    kind: np.ndarray        # per row: "x1", "x2", "x4", "x8" (exhaustive on that grid), "edge" (helpers.lwe_edge_rows), "key" (key_edge_rows), "uniform"
    target: np.ndarray      # exhaustive rows: the switched phase the row was built for on its own grid; -1 elsewhere
    expect: list            # (row, mask position, switched exponent) the engine's switched row must show (key_edge_rows)

    def of_kind(self, *kinds):
        return np.flatnonzero(np.isin(self.kind, kinds))

    def for_grid(self, o, N):
        """the rows a call on grid o runs.  Every row -- except that at N = 4096, where the ladder builds exhaustive rows for o = 1 only, a
        call on a coarse grid (whose accumulators are read back: 100 MB per thousand rows) takes the edge rows and every eighth exhaustive one"""
        if o == 1 or N < 4096:
            return np.arange(len(self.ct))
        x = self.of_kind("x1")
        return np.sort(np.concatenate([x[::8], np.flatnonzero(self.kind != "x1")]))


def exhaustive_rows(p, ones, o, rng):
    """one row for every multiple t of o in [0, 2N) whose switched phase on grid o is exactly t: uniform mask words, then the body word ON the
    switch grid that puts phi~ = b~ + sum a~_i s_i at t -> (rows, t)"""
    N, nu = p.N, o.bit_length() - 1
    t = np.arange(0, 2 * N, o)
    rows = rng.integers(0, 1 << 32, (len(t), p.lwe_len), dtype=np.uint64).astype(np.uint32)
    s = NC.coarse_word(rows[:, :-1][:, ones], N, nu).sum(axis=1)
    rows[:, -1] = (((t - s) % (2 * N)) << shift_of(N)).astype(np.uint32)
    return rows, t


def key_edge_words(N):
    """name -> (mask word, the exponent the mod switch gives it): a~ = 0, N, 2N and the rounding ties one step either side of 0 / 2N"""
    h = 1 << (shift_of(N) - 1)
    return {"0": (0, 0), "N": (1 << 31, N), "ones->2N": (2**32 - 1, 2 * N), "tie->1": (h, 1), "below tie->0": (h - 1, 0),
            "tie->2N": (2**32 - h, 2 * N), "below tie->2N-1": (2**32 - h - 1, 2 * N - 1)}


def key_edge_rows(p, ones, rng):
    """uniform rows with one word of key_edge_words at a mask position whose key bit is one -- the first, a middle and the last such position --
    and one row per word with it at EVERY such position -> (rows, [(row, position, exponent)])"""
    rows, expect = [], []
    pos = sorted({int(ones[0]), int(ones[len(ones) // 2]), int(ones[-1])})
    for w, a in key_edge_words(p.N).values():
        for where in [[q] for q in pos] + [list(map(int, ones))]:
            row = rng.integers(0, 1 << 32, p.lwe_len, dtype=np.uint64).astype(np.uint32)
            row[where] = w
            expect += [(len(rows), q, a) for q in where]
            rows.append(row)
    return np.stack(rows), expect


def build_rows(p, keys, seed):
    """the rows of one set (module docstring; the issue's "Rows"): exhaustive on every grid (N = 4096: o = 1 only), helpers.lwe_edge_rows,
    key_edge_rows, and UNIFORM_ROWS uniform rows (not at N = 4096)"""
    rng = np.random.default_rng([seed, p.N, p.lwe_len])
    ones = NC.key_ones(p, keys)
    assert len(ones), "a key without a one: no rounding edge can sit at a key position"
    ct, kind, target = [], [], []
    for o in GRIDS if p.N < 4096 else (1,):
        r, t = exhaustive_rows(p, ones, o, rng)
        ct.append(r); kind += [f"x{o}"] * len(r); target.append(t)
    base = sum(len(c) for c in ct)
    edge, _ = H.lwe_edge_rows(p, rng)
    krows, expect = key_edge_rows(p, ones, rng)
    expect = [(base + len(edge) + r, q, a) for r, q, a in expect]
    ct += [edge, krows]; kind += ["edge"] * len(edge) + ["key"] * len(krows)
    if p.N < 4096:
        ct.append(rng.integers(0, 1 << 32, (UNIFORM_ROWS, p.lwe_len), dtype=np.uint64).astype(np.uint32)); kind += ["uniform"] * UNIFORM_ROWS
    ct = np.concatenate(ct)
    target = np.concatenate(target + [np.full(len(ct) - base, -1)])
    return Rows(ct, np.array(kind), target, expect)


def cpu_slice(rows, cap=None):
    """the rows the reference side runs: all edge and key rows plus every eighth exhaustive row of every grid (at least 64 rows); cap trims the
    exhaustive part (evenly) where the reference is slow"""
    x = np.flatnonzero(np.char.startswith(rows.kind, "x"))[::8]
    rest = rows.of_kind("edge", "key")
    if cap is not None and len(x) + len(rest) > cap:
        x = x[np.linspace(0, len(x) - 1, max(cap - len(rest), 8)).astype(int)]
    idx = np.sort(np.concatenate([x, rest]))
    assert len(idx) >= 64
    return idx


def reference_phase(p, keys, ct, o=1):
    """phi~ of rows on grid o by DESIGN.md 1c restated (NC.coarse_word) -- what law 1 requires the engine's switched row to be"""
    nu = o.bit_length() - 1
    c = np.asarray(ct)
    return NC.modswitched_phase(p, keys, NC.coarse_word(c[..., :-1], p.N, nu), NC.coarse_word(c[..., -1], p.N, nu), o)


def reaches_every_phase(p, phi, o):
    """is every multiple of o in [0, 2N) among phi?"""
    seen = np.zeros(2 * p.N, dtype=bool)
    seen[np.asarray(phi).astype(np.int64)] = True
    return bool(seen[::o].all())


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
class Engine(NC.Engine):
    """NC.Engine plus the gate calls, each in host or in device memory (helpers.to_mem) -> host words"""

    def gate_ops(self, ops, x, y, mem=mk.MEM_HOST):
        return H.host_words(self.s.gate_ops(*[H.to_mem(a, mem) for a in (ops, x, y)]))

    def gate3_ops(self, ops, x, y, z, mem=mk.MEM_HOST):
        return H.host_words(self.s.gate3_ops(*[H.to_mem(a, mem) for a in (ops, x, y, z)]))

    def mux(self, s, a, b, mem=mk.MEM_HOST):
        return H.host_words(self.s.mux(*[H.to_mem(v, mem) for v in (s, a, b)]))


# ---- law 1: the switch -----------------------------------------------------------------------------------------------------------------
def switch_law(eng, p, keys, rows):
    """the engine's modswitch row is coarse_word of every input word, on every row; the table step of lut_many_testvector returns coarse_word on
    its grid and rotates by the b~ DESIGN.md 1c defines (NC.switched_phase's assertion); the key-edge exponents occur -> {o: phi~}"""
    ct, N = rows.ct, p.N
    at, bt = eng.modswitch(ct)
    assert np.array_equal(np.asarray(at).astype(np.int64), NC.coarse_word(ct[:, :-1], N, 0)), "modswitch: a mask word is not coarse_word of its input"
    assert np.array_equal(np.asarray(bt).astype(np.int64).ravel(), NC.coarse_word(ct[:, -1], N, 0)), "modswitch: a body word is not coarse_word of its input"
    at = np.asarray(at)
    missing = [(r, q, a) for r, q, a in rows.expect if int(at[r, q]) != a]
    assert rows.expect and not missing, ("a key-edge exponent does not occur in the engine's switched row", missing[:4])
    assert {a for _, _, a in rows.expect} == {0, 1, N, 2 * N - 1, 2 * N}
    phis = {1: NC.modswitched_phase(p, keys, at, bt, 1)}
    for o in GRIDS[1:]:
        idx = rows.for_grid(o, N)
        at_o, _ = eng.many_testvector(NC.index_table(p), ct[idx], o)
        assert np.array_equal(np.asarray(at_o).astype(np.int64), NC.coarse_word(ct[idx, :-1], N, o.bit_length() - 1)), ("table step: a~ is not coarse_word on grid", o)
        phis[o] = NC.switched_phase(eng, p, keys, ct[idx], o)
    for o, phi in phis.items():
        assert np.array_equal(phi, reference_phase(p, keys, ct[rows.for_grid(o, N)], o))
        if N < 4096 or o == 1:
            x = rows.of_kind(f"x{o}")
            assert np.array_equal(phi[np.searchsorted(rows.for_grid(o, N), x)], rows.target[x]), ("an exhaustive row misses the phase it was built for", o)
            assert reaches_every_phase(p, phi, o), o
    return phis


# ---- law 2: tables ---------------------------------------------------------------------------------------------------------------------
def grid_of(call):
    return int(call[4:]) if call.startswith("many") else 1 << int(call[-1]) if call.startswith("at_") else 1


def table_law(eng, p, keys, rows, call, seed, idx=None):
    """NC.decode_call on the rows of the call's grid (idx: a slice of them) -> (wrong bits, bits, max |e|, phi~)"""
    own = rows.for_grid(grid_of(call), p.N)
    idx = own if idx is None else np.intersect1d(own, idx)
    wrong, bits, e, phi = NC.decode_call(eng, p, keys, rows.ct[idx], call, np.random.default_rng(seed))
    return wrong, bits, float(np.abs(e).max()), phi


# ---- laws 3 and 4: gates ---------------------------------------------------------------------------------------------------------------
GATE_CODES = np.array([op | fx | fy for op in range(6) for fx in (0, mk.OP_NOT_X) for fy in (0, mk.OP_NOT_Y)], dtype=np.uint8)
GATE3_CODES = np.array([op | fx | fy | fz for op in range(6) for fx in (0, mk.OP_NOT_X) for fy in (0, mk.OP_NOT_Y) for fz in (0, mk.OP_NOT_Z)], dtype=np.uint8)
assert len(GATE_CODES) == 24 and len(GATE3_CODES) == 48


def neg(c):
    return ((0 - np.asarray(c).astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32)


def _flag(c, ops, flag):
    return np.where((np.asarray(ops) & flag)[:, None] != 0, neg(c), c)


def _wrap(v):
    return (v & 0xFFFFFFFF).astype(np.uint32)


def gate_rows(rows, N):
    """the rows a gate's linear part is put on: exhaustive on the fine grid, edge and key rows"""
    return rows.ct[rows.of_kind("x1", "edge", "key")]


def dense_codes(p):
    """where every gate code meets every target row: the N <= 256 sets of one or two parties (a rotation of many parties, or of a large ring,
    costs ten times as much; there the codes cycle over the rows)"""
    return p.N <= 256 and p.nparty <= 2


def gate_cases(codes, targets, dense):
    """-> (ops, target rows): every code on every target row (dense), or the codes cycling over the rows with a stride coprime to their
    count, so that each code meets every part of the phase range"""
    if not dense:
        return codes[(np.arange(len(targets)) * 5) % len(codes)], targets
    return np.repeat(codes, len(targets)), np.tile(targets, (len(codes), 1))


def even(ops, targets, doubling):
    """bit 0 of every word cleared where the code's linear part is twice a sum (gate.jl:28-44; XOR3 / XNOR3): the only words it can take.  The mod
    switch never sees bit 0, so the row's switched phase stays what it was built for"""
    return np.where(np.isin(np.asarray(ops) & 7, doubling)[:, None], targets & np.uint32(0xFFFFFFFE), targets)


def gate_operands(ops, targets, rng):
    """-> (x, y, lin): operands of gate_ops whose linear part (oracle.gate_linear after NOT! on the flagged inputs) is the target row: y
    uniform, x solved from helpers.gate_input; lin is taken from the oracle and required to be the target"""
    targets = even(ops, targets, (3, 4))
    y = rng.integers(0, 1 << 32, targets.shape, dtype=np.uint64).astype(np.uint32)
    yf = _flag(y, ops, mk.OP_NOT_Y)
    x0 = np.empty_like(targets)
    for op in range(6):
        m = (ops & 7) == op
        x0[m] = H.gate_input(op, targets[m])
    xf = _wrap(x0.astype(np.int64) - yf.astype(np.int64))
    x = _flag(xf, ops, mk.OP_NOT_X)
    lin = np.stack([O.gate_linear(int(ops[j]) & 7, xf[j], yf[j]) for j in range(len(ops))])
    assert np.array_equal(lin, targets), "gate_operands: the oracle's linear part is not the target row"
    return x, y, lin


def gate3_operands(ops, targets, rng):
    """the same for gate3_ops, the linear part from ref_gate3.linear3_rows"""
    targets = even(ops, targets, (2, 3))
    y, z = (rng.integers(0, 1 << 32, targets.shape, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    yf, zf = _flag(y, ops, mk.OP_NOT_Y).astype(np.int64), _flag(z, ops, mk.OP_NOT_Z).astype(np.int64)
    r, g = targets.astype(np.int64), (ops & 7)[:, None]
    b = np.zeros_like(r)
    b[:, -1] = np.where(g[:, 0] == 4, 1 << 30, np.where(g[:, 0] == 5, 3 << 30, 0))
    s = np.select([g == 0, g == 1, g == 2, g == 3, g == 4, g == 5], [r, -r, -(r // 2), r // 2, r - b, b - r])
    x = _flag(_wrap(s - yf - zf), ops, mk.OP_NOT_X)
    lin = G3.linear3_rows(ops, x, y, z)
    assert np.array_equal(lin, targets), "gate3_operands: the restated linear part is not the target row"
    return x, y, z, lin


def sign_words(p, keys, lin):
    """-> (the 32-bit word sign_lut holds at the switched phase of each linear part: +-1/8, phi~)"""
    phi = reference_phase(p, keys, lin)
    want = NC.table_values(mk.sign_lut(p), phi, 0, p.W)
    assert (np.abs(want) == 1 << (p.W - 3)).all()
    return NC.value_words(want, p.W), phi


def held(p, keys, out, want_words):
    """-> (outputs off their expected word by 1/16 or more -- a +-1/8 word: a wrong bit --, outputs, max |e|)"""
    e = np.abs(NC.phase_error(p, keys, out, want_words))
    return int((e >= MARGIN).sum()), int(e.size), float(e.max())


def mux_operands(t1, t2, rng):
    """-> (s, a, b, lin1, lin2): operands of mux whose two AND-linear parts (tests/test_gpu_multi.py oracle_mux: (s, a) and (NOT s, b)) are the
    target rows t1, t2"""
    s = rng.integers(0, 1 << 32, t1.shape, dtype=np.uint64).astype(np.uint32)
    a = _wrap(H.gate_input(1, t1).astype(np.int64) - s.astype(np.int64))
    b = _wrap(H.gate_input(1, t2).astype(np.int64) + s.astype(np.int64))
    lin1 = np.stack([O.gate_linear(1, s[j], a[j]) for j in range(len(s))])
    lin2 = np.stack([O.gate_linear(1, neg(s[j]), b[j]) for j in range(len(s))])
    assert np.array_equal(lin1, t1) and np.array_equal(lin2, t2), "mux_operands: an AND-linear part is not its target row"
    return s, a, b, lin1, lin2


def mux_words(p, keys, lin1, lin2):
    """S(phi~1) + S(phi~2) + 1/8 as 32-bit words"""
    w1, _ = sign_words(p, keys, lin1)
    w2, _ = sign_words(p, keys, lin2)
    return _wrap(w1.astype(np.int64) + w2.astype(np.int64) + (1 << 29))


def gate_inputs(p, keys, targets, seed, dense):
    """the operands and expected words of laws 3 and 4 on target rows -> {call: (operands, expected 32-bit words)}; they depend on the set's rows
    and secrets alone, so one set of them serves every arithmetic mode"""
    rng = np.random.default_rng(seed)
    g = {}
    ops, t = gate_cases(GATE_CODES, targets, dense)
    x, y, lin = gate_operands(ops, t, rng)
    g["gate_ops"] = ((ops, x, y), sign_words(p, keys, lin)[0])
    ops, t = gate_cases(GATE3_CODES, targets, dense)
    x, y, z, lin = gate3_operands(ops, t, rng)
    g["gate3_ops"] = ((ops, x, y, z), sign_words(p, keys, lin)[0])
    s, a, b, l1, l2 = mux_operands(targets, np.roll(targets, 37, axis=0), rng)
    g["mux"] = ((s, a, b), mux_words(p, keys, l1, l2))
    return g


def gate_laws(eng, p, keys, g, mem=mk.MEM_HOST):
    """laws 3 and 4 -> {call: (wrong, outputs, max |e|)}"""
    return {call: held(p, keys, getattr(eng, call)(*args, mem=mem), want) for call, (args, want) in g.items()}
