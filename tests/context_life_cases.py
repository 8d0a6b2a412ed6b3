"""The case lists of tests/test_gpu_context_life.py: the parameter sets, one STEP per batch entry point of include/mktfhe.h, and the option
walks.  tests/test_context_life_cpu.py imports the same lists and holds them to the header and to context.cpp's switch table, so that a new
entry point or a new workspace-resetting option cannot join the library without joining the sequence.

A step is a function (scheme, inputs, B, mem) that makes ONE call of its entry point on B rows in memory kind `mem` (mk.MEM_HOST: numpy
arrays, mk.MEM_DEVICE: GPU tensors) and returns what the call wrote.  The inputs of a set are made once, from fixed seeds (make_inputs), and
never written: every step hands the library its own copy."""
import types
from collections import namedtuple

import numpy as np

from helpers import O, encrypt_bits, gpu_scheme, keygen, mk, ora_params, rot_gadgets, to_mem
from mktfhe_amd.scheme import _Buf

# name -> (parameter set, arithmetic): the smallest shapes at which each route of context.cpp's rot_route still has its own workspace needs
SETS = {
    "cggi": (mk.CGGIparam.scaled(n=12, N=256), mk.ARITH_F64REF),                 # register route, no scratch; carries the chunk-crossing steps
    "kany": (mk.CGGIparam.scaled(n=8, N=256, k=4), mk.ARITH_F64REF),             # F64_KANY: scratch in memory
    "lmss": (mk.Blockparam.scaled(n=30, N=256, blk_d=10), mk.ARITH_F64REF),      # balanced key-switch digits: never the matrix cores
    "kms": (mk.KMS2party.scaled(n=8, N=256), mk.ARITH_F64REF),                   # ws_lev + ws_scratch; 64-bit ring; key switch on the matrix cores (the digit-pair kernel under MKT_KS_MFMA = 0)
    "ccs": (mk.CCS2party.scaled(n=8, N=256), mk.ARITH_F64REF),                   # vscratch in ws_lev; ccs_pipe either way
    "x-kr": (mk.CGGIparam.scaled(n=8, N=256, k=2), mk.ARITH_EXACT),              # EXACT_KR <-> EXACT_KANY under exact_kany
    "x-kms": (mk.KMS2party_N1024_l2.scaled(n=6, N=256), mk.ARITH_EXACT),         # Float64 pipe <-> integer NTT under exact_impl, exact_wide, ws_fxacc
    "x-ccs": (mk.CCS2party.scaled(n=4, N=256), mk.ARITH_EXACT),                  # integer-only route
}
# a set of the option walks only: at N = 256 the latency variant of the rotation does not exist (wide_supported: N >= 512)
EXTRA_SETS = {"cggi-N512": (mk.CGGIparam.scaled(n=12, N=512), mk.ARITH_F64REF)}

B_CYCLE = (5, 1, 70, 33, 0, 5)          # the workspace grows, is reused at a smaller size, and meets an empty call
BMAX = max(B_CYCLE)
POOL = 18                               # rows of the gather steps' pool
NLUTS = 3
CHUNK = 8192                            # context.cpp CHUNK_GATES


def set_of(name):
    return (SETS.get(name) or EXTRA_SETS[name])


_KEYS = {}


def keys_of(name, seed=1):
    """-> (crs or None, [PartyKeys]) of the set from key seed `seed`, generated once"""
    if (name, seed) not in _KEYS:
        _KEYS[name, seed] = keygen(set_of(name)[0], seed)
    return _KEYS[name, seed]


def new_scheme(name, seed=1):
    """a context of the set, created and keyed from key seed `seed` the plain way (load_crs, load_party)"""
    p, arith = set_of(name)
    return gpu_scheme(p, *keys_of(name, seed), arith=arith)


def ring_words(p, rng, shape):
    m = np.uint64((1 << p.W) - 1)
    return ((rng.integers(0, 1 << 63, shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, shape, dtype=np.uint64)) & m).astype(p.ring_dtype)


def lwe_words(p, rng, B):
    """B rows of any 32-bit words: every word is an input of every entry point"""
    return rng.integers(0, 1 << 32, (B, p.lwe_len), dtype=np.uint64).astype(np.uint32)


def make_inputs(name, nrows=BMAX):
    """the inputs of every step for set `name` (needs the GPU: masks and transforms come from a context that is closed again).  Gate operands
    from encrypt_bits; accumulators and masks from a fresh context's modswitch and the oracle's testvector; tables from lut_poly"""
    p, arith = set_of(name)
    crs, keys = keys_of(name)
    rng = np.random.default_rng([77, sorted(list(SETS) + list(EXTRA_SETS)).index(name)])
    n = nrows
    i = types.SimpleNamespace(name=name, p=p, keys=keys, n=n)
    i.op = sorted(list(SETS) + list(EXTRA_SETS)).index(name) % 6                # the gate of the `gate` step: one per set, all six over the sets
    c = encrypt_bits(p, keys, rng.integers(0, 2, 3 * n).astype(bool), seed=9000)
    i.x, i.y, i.z = c[:n], c[n:2 * n], c[2 * n:]
    i.ops = (rng.integers(0, 6, n) | rng.choice([0, mk.OP_NOT_X, mk.OP_NOT_Y, mk.OP_NOT_X | mk.OP_NOT_Y], n)).astype(np.uint8)
    i.ops3 = (rng.integers(0, 6, n) | rng.choice([0, mk.OP_NOT_X, mk.OP_NOT_Y, mk.OP_NOT_Z, mk.OP_NOT_X | mk.OP_NOT_Y | mk.OP_NOT_Z], n)).astype(np.uint8)
    i.pool = np.concatenate([i.x[:POOL // 3], i.y[:POOL // 3], i.z[:POOL // 3]])
    i.ix, i.iy, i.iz = (rng.integers(0, POOL, n).astype(np.uint32) for _ in range(3))
    i.not_ab = rng.integers(0, 4, n).astype(np.uint8)
    # lookup tables: lut_poly over 8 windows of random torus words (in the top 32 bits of a 64-bit ring word); packed for 2 and 4 tables
    table = lambda: mk.lut_poly([int(v) << (p.W - 32) for v in rng.integers(0, 1 << 32, 8)], p)      # noqa: E731
    i.T = np.stack([table() for _ in range(NLUTS)])
    i.U = {o: np.stack([mk.lut_pack(np.stack([table() for _ in range(o)]), p) for _ in range(NLUTS)]) for o in (2, 4, 8)}
    i.sel = rng.integers(0, NLUTS, n).astype(np.uint32)
    i.idx = rng.integers(0, POOL, (n, 4)).astype(np.uint32)
    i.wt = rng.integers(-4, 5, (n, 4)).astype(np.int8)
    i.cst = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    i.coef = np.array([9, p.N - 1, 4], dtype=np.uint32)
    i.src = rng.integers(0, 1 << 30, n).astype(np.uint32)                       # read modulo the accumulator count of the call
    i.kcoef = rng.integers(0, p.N, n).astype(np.uint32)
    # stages: the masks a fresh context's modswitch gives for the NAND linear parts, the oracle's test vector for their bodies
    s = new_scheme(name)
    try:
        i.at, i.bt = s.modswitch(np.stack([O.gate_linear(0, i.x[j], i.y[j]) for j in range(n)]))
        i.polys = ring_words(p, rng, (n, p.N))
        i.tr = s.transform_fwd(i.polys)                                         # valid transforms (EXACT: residue pairs) for transform_inv
    finally:
        s.close()
    so = O.Scheme(ora_params(p))                                                # the test vector needs no key
    i.acc0 = np.stack([so.testvector(int(b)) for b in i.bt]).astype(p.ring_dtype)
    i.accr = ring_words(p, rng, (n, p.k + 1, p.N))                              # any ring words are an input of the key switch
    # exact product: digit polynomials well inside N max|a| <= 2^28 - 2^15, as W-bit two's complement
    digits = rng.integers(-(1 << 18), 1 << 18, (n, p.N))
    i.pa = digits.astype(np.int64).view(np.uint64) if p.W == 64 else digits.astype(np.int32).view(np.uint32)
    i.pb = ring_words(p, rng, (n, p.N))
    # party-local calls: the last party; public mask seeds, pinned secret seeds (tests only)
    i.party = p.nparty - 1
    i.mask_seed, i.key_mask_seed = bytes(range(32)), bytes(range(1, 33))
    i.body = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    i.mu = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    sk = mk.party_keygen_seeded(crs, p, party=0, mask_seed=i.key_mask_seed, deterministic_seed=21)
    i.brk_seeded, i.ksk_seeded = np.array(sk.brk_seeded), np.array(sk.ksk_seeded)
    return i


PER_ROW = ("x", "y", "z", "ops", "ops3", "ix", "iy", "iz", "not_ab", "sel", "idx", "wt", "cst", "src", "kcoef", "at", "bt", "acc0", "accr", "polys", "tr",
           "pa", "pb", "body", "mu")


def window(i, lo, hi):
    """the inputs whose row j is row lo + j of i, for lo <= lo + j < hi: one piece of a call made in pieces"""
    w = types.SimpleNamespace(**vars(i))
    for k in PER_ROW:
        setattr(w, k, getattr(i, k)[lo:hi])
    w.n = hi - lo
    return w


def _new(shape, dtype, mem):
    """an output buffer in `mem`, every byte 0xA5"""
    a = np.empty(shape, dtype=dtype)
    a.reshape(-1).view(np.uint8)[...] = 0xA5
    return to_mem(a, mem)


def _acc_words(p):
    return (p.k + 1) * p.N


# ---- gates ----
def _gate(s, i, B, mem):
    return s.gate(i.op, to_mem(i.x[:B], mem), to_mem(i.y[:B], mem))


def _gate_ops(s, i, B, mem):
    return s.gate_ops(to_mem(i.ops[:B], mem), to_mem(i.x[:B], mem), to_mem(i.y[:B], mem))


def _gate_gather(s, i, B, mem):
    return s.gate_gather(to_mem(i.ops[:B], mem), to_mem(i.pool, mem), to_mem(i.ix[:B], mem), to_mem(i.iy[:B], mem), _new((B, i.p.lwe_len), np.uint32, mem))


def _gate3_ops(s, i, B, mem):
    return s.gate3_ops(to_mem(i.ops3[:B], mem), to_mem(i.x[:B], mem), to_mem(i.y[:B], mem), to_mem(i.z[:B], mem))


def _gate3_gather(s, i, B, mem):
    return s.gate3_gather(to_mem(i.ops3[:B], mem), to_mem(i.pool, mem), to_mem(i.ix[:B], mem), to_mem(i.iy[:B], mem), to_mem(i.iz[:B], mem),
                          _new((B, i.p.lwe_len), np.uint32, mem))


def _mux(s, i, B, mem):
    return s.mux(to_mem(i.x[:B], mem), to_mem(i.y[:B], mem), to_mem(i.z[:B], mem))


def _mux_gather(s, i, B, mem):
    return s.mux_gather(to_mem(i.pool, mem), to_mem(i.ix[:B], mem), to_mem(i.iy[:B], mem), to_mem(i.iz[:B], mem), _new((B, i.p.lwe_len), np.uint32, mem),
                        to_mem(i.not_ab[:B], mem))


def _not(s, i, B, mem):
    return s.not_(to_mem(i.z[:B], mem))


def _bootstrap(s, i, B, mem):
    return s.bootstrapping_(to_mem(i.x[:B], mem))


# ---- stages (Scheme.modswitch / keyswitch / kms_phase1 / decompose allocate host outputs: the checked call path directly) ----
def _modswitch(s, i, B, mem):
    m = i.p.lwe_len - 1
    at, bt = _new((B, m), np.uint32, mem), _new((B,), np.uint32, mem)
    s._call("modswitch_batch", B, s._ct(to_mem(i.y[:B], mem), B), _Buf(at, np.uint32, B, m, out=True), _Buf(bt, np.uint32, B, out=True))
    return at, bt


def _blindrotate(s, i, B, mem):
    return s.blindrotate_(to_mem(i.at[:B], mem), to_mem(i.acc0[:B], mem))


def keyswitch_call(s, acc, mem):
    """mkt_keyswitch_batch on accumulators already in `mem` -> rows in `mem`"""
    p = s.params
    B = int(np.prod(tuple(acc.shape)[:-2]))
    out = _new((B, p.lwe_len), np.uint32, mem)
    return s._call("keyswitch_batch", B, _Buf(acc, p.ring_dtype, B * _acc_words(p)), s._ct(out, B, out=True))[1]


def _keyswitch(s, i, B, mem):
    return keyswitch_call(s, to_mem(i.accr[:B], mem), mem)


def kms_phase1_call(s, at, mem):
    """mkt_kms_phase1_batch on masks already in `mem` -> the rows in `mem`: [B][Rtot][2][M] complex (Float64), split residue tables
    [B][Rtot][2][2][N] uint64 (EXACT)"""
    p = s.params
    B, rtot = int(at.shape[0]), 1 + (p.k - 1) * p.l_lev
    row, dt = ((rtot, 2, 2, p.N), np.uint64) if s.arith == mk.ARITH_EXACT else ((rtot, 2, p.N // 2), np.complex128)
    out = _new((B,) + row, dt, mem)
    return s._call("kms_phase1_batch", B, _Buf(at, np.uint32, B, p.lwe_len - 1), _Buf(out, dt, B * int(np.prod(row)), out=True))[1]


def _kms_phase1(s, i, B, mem):
    return kms_phase1_call(s, to_mem(i.at[:B], mem), mem)


# ---- lookup tables ----
def _lut_testvector(s, i, B, mem):
    return mk.lut_testvector(s, to_mem(i.T, mem), to_mem(i.x[:B], mem), to_mem(i.sel[:B], mem))


def _lut_bootstrap(s, i, B, mem):
    return mk.lut_bootstrap(s, to_mem(i.T, mem), to_mem(i.x[:B], mem), to_mem(i.sel[:B], mem))


def _gather_args(i, B, mem):
    return to_mem(i.pool, mem), to_mem(i.idx[:B], mem), to_mem(i.wt[:B], mem), to_mem(i.cst[:B], mem)


def _lut_gather(s, i, B, mem):
    return mk.lut_gather(s, to_mem(i.T, mem), to_mem(i.sel[:B], mem), *_gather_args(i, B, mem), _new((B, i.p.lwe_len), np.uint32, mem))


def _lut_many_testvector(s, i, B, mem):
    return mk.lut_many_testvector(s, to_mem(i.U[4], mem), to_mem(i.y[:B], mem), 4, to_mem(i.sel[:B], mem))


def _lut_extract(s, i, B, mem):
    return mk.lut_extract(s, to_mem(i.accr[:B], mem), 4)


def _lut_many_bootstrap(s, i, B, mem, o=4):
    return mk.lut_many_bootstrap(s, to_mem(i.U[o], mem), to_mem(i.y[:B], mem), o, to_mem(i.sel[:B], mem))


def _lut_many_gather(s, i, B, mem):
    return mk.lut_many_gather(s, to_mem(i.U[2], mem), to_mem(i.sel[:B], mem), *_gather_args(i, B, mem), 2, _new((B, 2, i.p.lwe_len), np.uint32, mem))


def _keyswitch_at(s, i, B, mem):
    nacc = max(B, 1)
    return mk.keyswitch_at(s, to_mem(i.accr[:nacc], mem), to_mem(i.src[:B] % nacc, mem), to_mem(i.kcoef[:B], mem))


def _lut_bootstrap_at(s, i, B, mem, nu=2):
    return mk.lut_bootstrap_at(s, to_mem(i.T, mem), to_mem(i.z[:B], mem), to_mem(i.coef, mem), nu, to_mem(i.sel[:B], mem))


def _lut_gather_at(s, i, B, mem):
    return mk.lut_gather_at(s, to_mem(i.T, mem), to_mem(i.sel[:B], mem), *_gather_args(i, B, mem), to_mem(i.coef, mem), _new((B, 3, i.p.lwe_len), np.uint32, mem))


# ---- units ----
def _transform_fwd(s, i, B, mem):
    return s.transform_fwd(to_mem(i.polys[:B], mem))


def _transform_inv(s, i, B, mem):
    return s.transform_inv(to_mem(i.tr[:B], mem))


def _decompose(s, i, B, mem):
    p = i.p
    l, logB = rot_gadgets(p)[0]
    out = _new((B, l, p.N), p.ring_dtype, mem)
    return s._call("decompose_batch", B, _Buf(to_mem(i.polys[:B], mem), p.ring_dtype, B, p.N), _Buf(out, p.ring_dtype, B * l, p.N, out=True), l, logB)[1]


def _exact_polymul(s, i, B, mem):
    return s.exact_polymul(to_mem(i.pa[:B], mem), to_mem(i.pb[:B], mem))


# ---- party-local calls ----
def _partial_decrypt(s, i, B, mem):
    return mk.partial_decrypt(to_mem(i.x[:B], mem), i.keys[i.party], i.p, i.party, 2.0 ** 12, scheme=s, deterministic_seed=31, row0=3)


def _seeded_expand(s, i, B, mem):
    return mk.seeded_expand(mk.SeededBatch(i.party, i.mask_seed, 1 << 33, to_mem(i.body[:B], mem)), i.p, scheme=s)


def _seeded_encrypt(s, i, B, mem):
    return mk.seeded_encrypt(to_mem(i.mu[:B], mem), i.keys[i.party], i.p, i.party, words=True, scheme=s, mask_seed=i.mask_seed, deterministic_seed=32, row0=5).body


def _seeded_keys_expand(s, i, B, mem):
    """no batch count: one party's two keys, whatever B"""
    return mk.seeded_keys_expand(i.p, 0, i.key_mask_seed, to_mem(i.brk_seeded, mem), to_mem(i.ksk_seeded, mem), scheme=s)


def _every(p, arith):
    return True


def _kms_only(p, arith):
    return p.scheme in (mk.KMS, mk.KMS_BLOCK)


def _exact_only(p, arith):
    return arith == mk.ARITH_EXACT


# name, the entry point of include/mktfhe.h, the call, the sets it applies to -- in the order of the first round of the sequence test
Step = namedtuple("Step", "name entry fn applies")
STEPS = [
    Step("gate", "mkt_gate_batch", _gate, _every),
    Step("gate_ops", "mkt_gate_batch_ops", _gate_ops, _every),
    Step("gate_gather", "mkt_gate_batch_gather", _gate_gather, _every),
    Step("gate3_ops", "mkt_gate3_batch_ops", _gate3_ops, _every),
    Step("gate3_gather", "mkt_gate3_batch_gather", _gate3_gather, _every),
    Step("mux", "mkt_mux_batch", _mux, _every),
    Step("mux_gather", "mkt_mux_batch_gather", _mux_gather, _every),
    Step("not", "mkt_not_batch", _not, _every),
    Step("bootstrap", "mkt_bootstrap_batch", _bootstrap, _every),
    Step("modswitch", "mkt_modswitch_batch", _modswitch, _every),
    Step("blindrotate", "mkt_blindrotate_batch", _blindrotate, _every),
    Step("keyswitch", "mkt_keyswitch_batch", _keyswitch, _every),
    Step("kms_phase1", "mkt_kms_phase1_batch", _kms_phase1, _kms_only),
    Step("lut_testvector", "mkt_lut_testvector_batch", _lut_testvector, _every),
    Step("lut_bootstrap", "mkt_lut_bootstrap_batch", _lut_bootstrap, _every),
    Step("lut_gather", "mkt_lut_batch_gather", _lut_gather, _every),
    Step("lut_many_testvector", "mkt_lut_many_testvector_batch", _lut_many_testvector, _every),
    Step("lut_extract", "mkt_lut_extract_batch", _lut_extract, _every),
    Step("lut_many_bootstrap", "mkt_lut_many_bootstrap_batch", _lut_many_bootstrap, _every),
    Step("lut_many_gather", "mkt_lut_many_batch_gather", _lut_many_gather, _every),
    Step("keyswitch_at", "mkt_keyswitch_at_batch", _keyswitch_at, _every),
    Step("lut_bootstrap_at", "mkt_lut_bootstrap_at_batch", _lut_bootstrap_at, _every),
    Step("lut_gather_at", "mkt_lut_batch_gather_at", _lut_gather_at, _every),
    Step("transform_fwd", "mkt_transform_fwd_batch", _transform_fwd, _every),
    Step("transform_inv", "mkt_transform_inv_batch", _transform_inv, _every),
    Step("decompose", "mkt_decompose_batch", _decompose, _every),
    Step("exact_polymul", "mkt_exact_polymul_batch", _exact_polymul, _exact_only),
    Step("partial_decrypt", "mkt_partial_decrypt_batch", _partial_decrypt, _every),
    Step("seeded_expand", "mkt_seeded_expand_batch", _seeded_expand, _every),
    Step("seeded_encrypt", "mkt_seeded_encrypt_batch", _seeded_encrypt, _every),
    Step("seeded_keys_expand", "mkt_seeded_keys_expand", _seeded_keys_expand, _every),
]
STEP = {st.name: st for st in STEPS}
ORACLE_STEPS = ("gate", "gate_ops", "bootstrap", "mux")      # also held to the CPU oracle (EXACT sets: to tests/ref_exact.py)


def steps_of(name):
    p, arith = set_of(name)
    return [st for st in STEPS if st.applies(p, arith)]


def sequence(name):
    """the steps of the sequence test for a set, in order: the table's order, then np.random.default_rng(s).permutation for s = 1, 2 ->
    [(step, B, mem)], B cycling through B_CYCLE and mem alternating host arrays and GPU tensors (so the empty call is a host call: an empty
    tensor has no address to hand over)"""
    steps = steps_of(name)
    order = list(steps)
    for seed in (1, 2):
        order += [steps[j] for j in np.random.default_rng(seed).permutation(len(steps))]
    return [(st, B_CYCLE[j % len(B_CYCLE)], (mk.MEM_HOST, mk.MEM_DEVICE)[j % 2]) for j, st in enumerate(order)]


# ---- options changed under a live workspace: (set, options set before the first call, the option walked, its values, the kernel
#      mkt_last_kernel_name must name after a gate under each value).  The kernels are what do_blindrotate (context.cpp) and the launchers
#      decide at B = 5, 33, 70 for these shapes: N = 256 has no latency variant (wide_supported) and no grouped automatic choice (rot_blkg 0:
#      one rotation per workgroup below 1024 rotations); ccs_pipe -1 takes the two-group kernel below one chip-fill (2 B <= 1024) ----
Walk = namedtuple("Walk", "set before option values kernels")
OPTION_WALKS = [
    Walk("x-kr", {"exact_impl": 0}, "exact_kany", (0, 1, 0), ("exact_blindrotate_kr_kernel", "exact_blindrotate_kany_kernel", "exact_blindrotate_kr_kernel")),
    Walk("x-kms", {}, "exact_impl", (-1, 0, 1), ("fx_blindrotate_kernel", "exact_kms_phase1_p2pf_kernel", "fx_blindrotate_kernel")),
    Walk("x-kms", {"exact_impl": 0}, "exact_wide", (1, 0, 1), ("exact_kms_phase1_p2pf_kernel", "exact_kms_phase1_kernel", "exact_kms_phase1_p2pf_kernel")),
    Walk("ccs", {}, "ccs_pipe", (-1, 0, 1, -1), ("ccs_pipe_kernel", "ccs_blindrotate_kernel", "ccs_pipe_kernel", "ccs_pipe_kernel")),
    Walk("cggi", {}, "rot_wide", (0, 1, 2, 0), ("blindrotate_k1_kernel",) * 4),
    Walk("cggi-N512", {}, "rot_wide", (0, 1, 2, 0), ("blindrotate_wide_kernel", "blindrotate_k1_kernel", "blindrotate_wide_kernel", "blindrotate_wide_kernel")),
    Walk("lmss", {}, "rot_blkg", (0, 1, 4, 0), ("blindrotate_k1_kernel", "blindrotate_k1_kernel", "blindrotate_blk_kernel", "blindrotate_k1_kernel")),
]


def walk_id(w):
    return f"{w.set}-{w.option}"


# ---- key-set readiness: check_ready (context.cpp) restated.  loaded: the pieces present, ("brk" | "ksk" | "rlk" | "pubkey", party) and "crs" ----
PIECES = ("ksk", "crs", "pubkey", "rlk", "brk")             # the order the life-cycle test loads them in, the last party first


def pieces_of(p):
    return [k for k in PIECES if k in ("ksk", "brk") or (p.multikey and k in ("crs", "pubkey")) or (k == "rlk" and p.scheme in (mk.KMS, mk.KMS_BLOCK))]


def expected_refusal(p, loaded, need_brk, need_ksk):
    """-> the message mkt_last_error must hold when a call with these needs meets these pieces, None if the call must be served"""
    kms = p.scheme in (mk.KMS, mk.KMS_BLOCK)
    for i in range(p.nparty):
        if need_brk and ("brk", i) not in loaded:
            return "bootstrapping key not loaded"
        if need_ksk and ("ksk", i) not in loaded:
            return "key-switching key not loaded"
        if need_brk and p.scheme == mk.CCS and ("pubkey", i) not in loaded:
            return "public key not loaded"
        if need_brk and kms and (("rlk", i) not in loaded or ("pubkey", i) not in loaded):
            return "rlk / public key not loaded"
    if need_brk and p.multikey and "crs" not in loaded:
        return "crs not loaded"
    return None


PROBES = (("gate", True, True), ("blindrotate", True, False), ("keyswitch", False, True))      # step, needs the bootstrapping side, needs the key-switching key


# ---- tables T': the engine's own (mkt_make_twiddles) with every entry of Psi from index 4 on moved by one ulp, in both parts, in a seeded
#      direction, and Psiinv its conjugate: what mkt_set_twiddles admits (it checks conjugacy and the first three entries) ----
def make_twiddles(N):
    import ctypes as C
    from mktfhe_amd import _lib
    tabs = [np.empty(N // 2, dtype=np.complex128) for _ in range(4)]
    for which, t in enumerate(tabs):
        _lib.check(_lib.lib().mkt_make_twiddles(N, which, t.ctypes.data_as(C.c_void_p)))
    return tabs


def tprime(N, seed=5):
    psi, psiinv, roots, rootsinv = make_twiddles(N)
    way = np.random.default_rng(seed).choice([-np.inf, np.inf], (N // 2 - 4, 2))
    psi, psiinv = psi.copy(), psiinv.copy()
    psi.real[4:] = np.nextafter(psi.real[4:], way[:, 0])
    psi.imag[4:] = np.nextafter(psi.imag[4:], way[:, 1])
    psiinv[4:] = np.conj(psi[4:])
    return [psi, psiinv, roots, rootsinv]


def set_twiddles(s, tabs):
    """mkt_set_twiddles on a Scheme -> its return code"""
    import ctypes as C
    from mktfhe_amd import _lib
    keep = [np.ascontiguousarray(t, dtype=np.complex128) for t in tabs]
    return _lib.lib().mkt_set_twiddles(s.h, *[t.ctypes.data_as(C.c_void_p) for t in keep])
