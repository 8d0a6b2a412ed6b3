"""The transform-domain sums of a CMux start with their first product instead of adding it to a zero (fft_device.h, at cadd): the only
thing that can differ is the sign of a zero in an intermediate, and no output word may.  The inputs here make those zeros: accumulators
whose digits are all zero, so that every product of a sum is +0 or -0 and the sign of the sum depends on whether it started from +0 --
the phase-1 start (g X^0, 0), the all-zero accumulator, words that decompose into zero digits -- and helpers.acc_edge words; masks with
zeros in the leading positions, so that the first executed step (and, in a block, the first contributing key bit) varies.  Blind rotation
and KMS phase 1 (its rows are raw transform bits) against the oracle, tolerance 0, under every kernel the engine can be forced onto."""
import numpy as np
import pytest

from helpers import acc_edge, bits_equal, gpu_scheme, keygen, mk, oracle_scheme, rot_gadgets

pytestmark = pytest.mark.gpu

B = 3
_K = mk.KMS2party_N1024_l2.scaled(n=8)
# (parameter set, [(options, kernel the options select)]).  Blockparam keeps its block length 3 (the shipped instantiation), so n = 9
CASES = [
    (_K, [({"rot_wide": 1}, "blindrotate_k1_kernel"), ({"rot_wide": 2}, "blindrotate_wide_kernel")]),               # the l- and base-specialised headline instantiation
    (_K.scaled(N=128), [({"rot_wide": 1}, "blindrotate_k1_kernel")]),                                                # the generic one (no latency variant below N = 512)
    (mk.CGGIparam.scaled(n=8, N=1024), [({"rot_wide": 1}, "blindrotate_k1_kernel"), ({"rot_wide": 2}, "blindrotate_wide_kernel")]),
    (mk.Blockparam.scaled(n=9, N=1024, blk_d=3), [({"rot_blkg": 1}, "blindrotate_k1_kernel"), ({"rot_blkg": 2}, "blindrotate_blk_kernel"),
                                                  ({"rot_blkg": 4}, "blindrotate_blk_kernel")]),
    (mk.CCS2party.scaled(n=8, N=64), [({"ccs_pipe": 0}, "ccs_blindrotate_kernel"), ({"ccs_pipe": 1}, "ccs_pipe_kernel")]),
]


def _masks(p, rng):
    """B rows of switched exponents: leading zeros of a different length in every row (inside the first block and across it), a full
    turn and a half turn as the first executed step"""
    nm, N = p.lwe_len - 1, p.N
    at = rng.integers(1, 2 * N, (B, nm)).astype(np.uint32)
    at[0, :1] = 0; at[0, 1] = 2 * N
    at[1, :2] = 0; at[1, 2] = N
    at[2, :4] = 0; at[2, 5] = 0
    if p.nparty > 1:
        at[1, p.n:p.n + 3] = 0                                        # the second party's first steps too
    return at


def _gadget(p):
    """the gadget that decomposes the caller's accumulator first: GSW (CGGI, LMSS), UniEnc (CCS), LEV (KMS: phase 2; phase 1 starts from
    its own (g X^0, 0) rows)"""
    return rot_gadgets(p)[1 if p.scheme in (mk.KMS, mk.KMS_BLOCK) else 0]


def _zero_digit_words(p):
    """words whose digits are all zero under that gadget (gsw.jl:42-52): below half a unit of the last digit, and the smallest word
    that rounds up and carries out of the top digit"""
    l, logB = _gadget(p)
    bit = p.W - l * logB
    w = [0, (1 << p.W) - (1 << (bit - 1))]
    if bit >= 2:
        w += [1, (1 << (bit - 1)) - 1]
    return np.array(w, dtype=np.uint64)


def _accumulators(p, rng):
    N, k = p.N, p.k
    l, logB = _gadget(p)
    start = np.zeros((B, 1 + k, N), dtype=np.uint64)
    start[:, 0, 0] = [1 << (p.W - (1 + r % l) * logB) for r in range(B)]                                        # (g_r X^0, 0): all a digits zero
    zero = np.zeros((B, 1 + k, N), dtype=np.uint64)
    zw = _zero_digit_words(p)
    zdig = zw[rng.integers(0, len(zw), (B, 1 + k, N))]
    zdig[0, 0] = zw[1]; zdig[1, 1] = zw[-1]
    return {"start": start, "zero": zero, "zero-digits": zdig, "edge": acc_edge(p, rot_gadgets(p), rng, B)}


@pytest.mark.parametrize("p,forced", CASES, ids=lambda v: f"{v.name}-n{v.n}-N{v.N}" if isinstance(v, mk.Params) else "")
def test_rotation_outputs_do_not_see_the_sign_of_zero(require_gpu, p, forced):
    crs, keys = keygen(p, 41)
    so, sg = oracle_scheme(p, crs, keys), gpu_scheme(p, crs, keys)
    rng = np.random.default_rng(42)
    at = _masks(p, rng)
    accs = _accumulators(p, rng)
    ref = {name: np.stack([so.blindrotate(at[j], acc[j]) for j in range(B)]) for name, acc in accs.items()}
    lev_o = None
    if p.scheme in (mk.KMS, mk.KMS_BLOCK):
        lev_o = [np.concatenate([so.kms_phase1(party, at[j, party * p.n:(party + 1) * p.n]) for party in range(p.k)]) for j in range(B)]
    for opts, kernel in forced:
        for name, v in opts.items():
            sg.set_option(name, v)
        for name, acc in accs.items():
            got = sg.blindrotate_(at, acc.astype(p.ring_dtype).copy()).astype(np.uint64).reshape(acc.shape)
            assert sg.last_kernel_name() == kernel, (opts, sg.last_kernel_name())
            assert np.array_equal(got, ref[name]), (opts, name, np.argwhere(got != ref[name])[:3])
        if lev_o is not None:
            lev_g = sg.kms_phase1(at)
            for j in range(B):
                assert bits_equal(lev_g[j], lev_o[j]), (opts, "phase 1", j)
    sg.close()
