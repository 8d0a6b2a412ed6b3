"""Every scheme's bootstraps against the exactly computed switched phase (tests/decode_cases.py): nothing of oracle/ decides an expected bit
here, so a sign convention, a window border or a rotation direction that kernel and oracle get wrong together does not pass.

For every (set, arithmetic mode, EXACT implementation) of decode_cases.RUN_PAIRS -- all five schemes, 1 to 16 parties, RLWE length 1 to 4,
N = 128 .. 4096, each set with its shipped noise and noise-free -- on rows of plain 32-bit words that meet EVERY switched phase on every grid:

  1  the engine's switched row is DESIGN.md 1c's rounding of every input word, and the table step rotates by the b~ it defines;
  2  every output of every call of NC.DECODE_CALLS is the table's word at phi~: no wrong bit, |e| < 1/16;
  3  gate_ops (24 codes) and gate3_ops (48 codes), host and device memory and one gather form each: sign_lut at the phi~ of the linear part;
  4  mux and mux_gather with its not_ab flags: S(phi~1) + S(phi~2) + 1/8 within 1/16.

Stated, not measured: no wrong output, |e| < 1/16 (half the decision margin), no row left out.  On the noise-free sets the device's max |e| is
also held to 4 x the reference's on the CPU slice (decode_cases.REF_MAX_E, recomputed by tests/test_decode_cpu.py).  Each test prints its
figures before it asserts.  A last test closes a gap docs/history.md logged: the twiddle tables are refused after ANY transformed key piece."""
import numpy as np
import pytest

import context_life_cases as K
import decode_cases as D
import helpers as H
import noise_cases as NC
from noise_cases import mk

pytestmark = pytest.mark.gpu
HOST, DEV = mk.MEM_HOST, mk.MEM_DEVICE
ERR_STATE = -5


class Bench:
    """the keys, rows, gate operands and contexts of ONE entry at a time (the pairs run entry by entry): made when first asked for, the
    contexts closed when the next entry comes"""

    def __init__(self):
        self.entry, self.ctx, self.rows = None, {}, {}

    def close(self):
        for s in self.ctx.values():
            s.close()
        self.ctx.clear()

    def get(self, case):
        name, mode, impl = case
        e = D.BY_ID[name]
        if self.entry is not e:
            self.close()
            self.entry, (self.crs, self.keys) = e, D.keys_of(e)
        if e.base not in self.rows:                             # rows and operands depend on the secrets alone: shipped and noise-free share them
            rows = D.build_rows(e.p, self.keys, NC.set_seed(e.base, 7))
            self.rows = {e.base: (rows, D.gate_inputs(e.p, self.keys, D.gate_rows(rows, e.p.N), 12, D.dense_codes(e.p)))}
        if mode not in self.ctx:
            self.ctx[mode] = H.gpu_scheme(e.p, self.crs, self.keys, arith=NC.ARITH[mode])
        s = self.ctx[mode]
        if impl is not None:
            s.set_option("exact_impl", 1 if impl == "fx" else 0)
            if impl == "fx":
                assert s.get_metric("fx_available") == 1.0, (name, "the Float64 pipe does not certify these keys", s.get_metric("fx_bound"))
        return D.Engine(s), e, self.keys, *self.rows[e.base]

    def served_by(self, case):
        """the rotation kernel of the last call is the implementation the case names (NC.Bench.served_by)"""
        name, mode, impl = case
        if impl is not None:
            kern = self.ctx[mode].last_kernel_name()
            assert ("fx_" in kern) == (impl == "fx"), (case, kern)


@pytest.fixture(scope="module")
def bench(require_gpu):
    b = Bench()
    yield b
    b.close()


def _against_reference(e, what, emax):
    if e.noise == D.QUIET:
        ref = D.REF_MAX_E[e.base][what]
        print("   noise-free: device max |e|", emax, "reference", ref, "ratio", emax / ref)
        assert emax <= D.DEVICE_OVER_REFERENCE * ref, (e.id, what, emax, ref)


# ---- laws 1 and 2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.RUN_PAIRS, ids=D.pair_id)
def test_switched_row_and_every_table_output(bench, case):
    eng, e, keys, rows, _ = bench.get(case)
    p = e.p
    D.switch_law(eng, p, keys, rows)
    worst = 0.0
    for call in NC.DECODE_CALLS:
        wrong, bits, emax, phi = D.table_law(eng, p, keys, rows, call, 109)
        bench.served_by(case)
        o = D.grid_of(call)
        print("C", D.pair_id(case), call, "rows", len(phi), "bits", bits, "wrong", wrong, "max |e|", emax)
        assert len(phi) == len(rows.for_grid(o, p.N)) and bits >= len(phi), "no row is left out"
        if p.N < 4096 or o == 1:
            assert D.reaches_every_phase(p, phi, o) and NC.reads_the_corners(p, phi), (call, "a switched phase is not met")
        assert wrong == 0, (case, call, wrong, bits)
        assert emax < D.MARGIN, (case, call, emax)
        worst = max(worst, emax)
    _against_reference(e, "tables", worst)


# ---- laws 3 and 4 ----------------------------------------------------------------------------------------------------------------------
def _gather(s, call, ops, operands, rng, flags=None, limit=512):
    """one gather form over a pool in device memory that holds every operand (operand t of every gate in block nin - 1 - t), `limit` of the
    gates in a random order -> (host words, the gates picked)"""
    B, nin = len(operands[0]), len(operands)
    pick = rng.permutation(B)[:limit]
    pool = np.concatenate(operands[::-1])
    dev = lambda a: H.to_mem(a, DEV)      # noqa: E731
    idx = [dev(((nin - 1 - t) * B + pick).astype(np.uint32)) for t in range(nin)]
    out = dev(np.zeros((len(pick), pool.shape[1]), dtype=np.uint32))
    if call == "mux_gather":
        got = s.mux_gather(dev(pool), *idx, out, not_ab=dev(flags[pick]))
    else:
        got = getattr(s, call)(dev(ops[pick]), dev(pool), *idx, out)
    return H.host_words(got), pick


@pytest.mark.parametrize("case", D.RUN_PAIRS, ids=D.pair_id)
def test_every_gate_output_is_the_sign_at_the_switched_phase(bench, case):
    eng, e, keys, rows, g = bench.get(case)
    p, s = e.p, eng.s
    rng = np.random.default_rng(113)
    worst = 0.0
    for mem in (HOST, DEV):
        for call, (wrong, outs, emax) in D.gate_laws(eng, p, keys, g, mem).items():
            bench.served_by(case)
            print("G", D.pair_id(case), call, "host" if mem == HOST else "device", "outputs", outs, "wrong", wrong, "max |e|", emax)
            assert outs == len(g[call][1]) >= len(D.gate_rows(rows, p.N)), "no row is left out"
            assert wrong == 0 and emax < D.MARGIN, (case, call, mem, wrong, emax)
            worst = max(worst, emax)
    # the gather forms, from a pool in device memory
    for call, src in (("gate_gather", "gate_ops"), ("gate3_gather", "gate3_ops")):
        args, want = g[src]
        got, pick = _gather(s, call, args[0], args[1:], rng)
        wrong, outs, emax = D.held(p, keys, got, want[pick])
        print("G", D.pair_id(case), call, "outputs", outs, "wrong", wrong, "max |e|", emax)
        assert wrong == 0 and emax < D.MARGIN, (case, call, wrong, emax)
        worst = max(worst, emax)
    (sel, a, b), want = g["mux"]
    flags = rng.integers(0, 4, len(sel)).astype(np.uint8)
    got, pick = _gather(s, "mux_gather", None, (sel, D._flag(a, flags, 1), D._flag(b, flags, 2)), rng, flags)
    assert {0, 1, 2, 3} <= set(flags[pick].tolist())
    wrong, outs, emax = D.held(p, keys, got, want[pick])
    print("G", D.pair_id(case), "mux_gather", "outputs", outs, "wrong", wrong, "max |e|", emax)
    assert wrong == 0 and emax < D.MARGIN, (case, "mux_gather", wrong, emax)
    _against_reference(e, "gates", max(worst, emax))


def test_refused_pairs_are_refused_with_their_code(require_gpu):
    """every pair decode_cases.REFUSED lists: the library refuses it -- at context creation, key load or the first bootstrap -- with the listed code"""
    for (name, mode, impl), code in D.REFUSED.items():
        e = D.BY_ID[name]
        crs, keys = D.keys_of(e)
        with pytest.raises(mk.MktError) as err:
            s = H.gpu_scheme(e.p, crs, keys, arith=NC.ARITH[mode])
            try:
                s.set_option("exact_impl", 1 if impl == "fx" else 0)
                mk.lut_bootstrap(s, mk.sign_lut(e.p), np.zeros((1, e.p.lwe_len), dtype=np.uint32))
            finally:
                s.close()
        assert err.value.code == code, (name, mode, impl, err.value.code, str(err.value))


# ---- the twiddle tables and every transformed key piece ----------------------------------------------------------------------------------
TWIDDLE_SETS = ["CGGIparam-n20-N256-k1-shipped", "Blockparam-n30-N256-k1-shipped", "KMS2party-n16-N256-k2-shipped", "KMS2partyblock-n24-N256-k2-shipped",
                "CCS2party-n12-N256-k2-shipped"]


@pytest.mark.parametrize("name", TWIDDLE_SETS)
def test_tables_are_refused_after_any_transformed_key_piece(require_gpu, name):
    """docs/history.md logged a mutant no test caught: any_transformed() without the public-key bit.  On a fresh Float64 context, each of the
    bootstrapping key, the relinearisation key, the public key (per party) and the CRS loaded ALONE makes mkt_set_twiddles return MKT_ERR_STATE and
    leaves mkt_get_twiddles as it was; the key-switching key alone -- integer data -- does not stand in the way"""
    from mktfhe_amd import _lib
    e = D.BY_ID[name]
    p = e.p
    crs, keys = D.keys_of(e)
    tabs, own = K.tprime(p.N), K.make_twiddles(p.N)
    kms = p.scheme in (mk.KMS, mk.KMS_BLOCK)
    loads = []
    for i, kk in enumerate(keys):
        loads.append((f"brk {i}", lambda s, i=i, kk=kk: s.load_party(i, brk=kk.brk)))
        if kms:
            loads.append((f"rlk {i}", lambda s, i=i, kk=kk: s.load_party(i, rlk_d=kk.rlk_d, rlk_f=kk.rlk_f)))
        if p.multikey:
            loads.append((f"pubkey {i}", lambda s, i=i, kk=kk: s.load_party(i, pubkey=kk.pubkey)))
    if p.multikey:
        loads.append(("crs", lambda s: s.load_crs(crs)))
    assert len(loads) == p.nparty * (1 + kms + p.multikey) + p.multikey
    for what, load in loads:
        s = mk.Scheme(p)
        load(s)
        rc = K.set_twiddles(s, tabs)
        msg = _lib.lib().mkt_last_error(s.h)
        after = [s.twiddles(w) for w in range(4)]
        s.close()
        assert rc == ERR_STATE and b"install the tables before the keys" in msg, (name, what, rc, msg)
        assert all(np.array_equal(a, t) for a, t in zip(after, own)), (name, what, "a refused call changed the tables")
    for i, kk in enumerate(keys):
        s = mk.Scheme(p)
        s.load_party(i, ksk=kk.ksk)
        rc = K.set_twiddles(s, tabs)
        after = [s.twiddles(w) for w in range(4)]
        s.close()
        assert rc == 0 and all(np.array_equal(a, t) for a, t in zip(after, tabs)), (name, "ksk alone", i, rc)
