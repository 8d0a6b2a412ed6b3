"""The case lists of tests/test_gpu_size_ladder.py: every rotation kernel at every ring size the library admits, and the corners of
validate_params.  tests/test_size_ladder_cpu.py holds the same lists against the launchers without a GPU (tests/csrc/launch_log.cpp,
modes `kernels` and `reach`): every entry reaches the instantiation it names, and no rotation instantiation compiled into the library is
without an entry here, a case of tests/edge_cases.py, or an exclusion below.

Every rotation kernel is a template over the transform size LOGM (MKT_DISPATCH_LOGM: 4 .. 11, N = 32 .. 4096) and each size is separately
compiled code with its own exchange schedule (fft_device.h Plan<>), thread count, LDS layout and table strides.  A ladder row is
(parameter set, [(options, kernel it must reach), ...]): ONE context per parameter set, the option settings walked on it with set_option.

Shapes: n = 3 key bits (3 * blk_len for the block schemes: the next-block prefetch takes both branches), two parties for KMS and CCS,
B = 5 ciphertexts (one past a grouping of 4, ragged for 2)."""
from helpers import mk

SIZES = (32, 64, 128, 256, 512, 1024, 2048, 4096)
B = 5
# the switches a walk touches, at their defaults (context.cpp SWITCHES): every step starts from these
DEFAULTS = {"rot_variant": 0, "rot_wide": 0, "rot_blkg": 0, "ccs_pipe": -1, "exact_impl": -1, "exact_wide": 1, "exact_kany": 0}


def logM(N):
    return N.bit_length() - 2


# ---- which kernels exist for a shape: restated from rot_plan.h / rot_block.hip / ccs_pipe.hip (a wrong restatement names a kernel the
# launcher does not reach, and tests/test_size_ladder_cpu.py fails)
def wide_supported(lm, l, blk_len=1):
    return blk_len == 1 and 8 <= lm <= 10 and 2 <= l <= 4


def fx_supported(lm, W, l):
    return 6 <= lm <= 11 and W in (32, 64) and l in (2, 3)


def blockg_supported(lm, G):
    M = 1 << lm
    return 4 <= lm <= 11 and G in (2, 4) and G * M // 4 <= 1024 and (2 + 4 * G) * M * 16 <= 160 * 1024


def blockg_np_covers(W, kr, blk_len):
    return W == 32 and ((kr == 2 and blk_len in (1, 3)) or (kr == 3 and blk_len == 1))


def sid(p):
    return f"{p.name}-n{p.n}-N{p.N}-k{p.k}-W{p.W}-b{p.blk_len}-l{p.l_uni if p.scheme == mk.CCS else p.l_gsw}x{p.logB_uni if p.scheme == mk.CCS else p.logB_gsw}"


def words_only(p):
    """KMS on the 32-bit ring: a shape no shipped parameter set resembles, whose gate outputs decrypt wrongly now and then under the ORACLE
    (checked on the CPU at every size): the oracle's words are the criterion there, decryption is not asserted"""
    return p.scheme in (mk.KMS, mk.KMS_BLOCK) and p.W == 32


_K1, _WIDE, _BLK, _KR, _KANY, _CCS, _PIPE = ("blindrotate_k1_kernel", "blindrotate_wide_kernel", "blindrotate_blk_kernel", "blindrotate_kr_kernel",
                                            "blindrotate_kany_kernel", "ccs_blindrotate_kernel", "ccs_pipe_kernel")
_V21, _V22 = {"rot_wide": 1, "rot_variant": 21}, {"rot_wide": 1, "rot_variant": 22}


# ---- the parameter sets of the ladder, by family
def cggi(N, **kw):
    return mk.CGGIparam.scaled(n=3, N=N, **kw)


def kms(N, **kw):
    return mk.KMS2party.scaled(n=3, N=N, **kw)


def kms32(N, **kw):
    """KMS on the 32-bit ring (validate_params admits it): kms_phase2_kernel<.., uint32_t>; gadgets that fit 32 bits"""
    kw = {**dict(l_gsw=3, logB_gsw=9, l_lev=2, logB_lev=7, l_uni=3, logB_uni=10), **kw}
    return mk.KMS2party.scaled(name="KMS2party_w32", n=3, N=N, W=32, **kw)


def lmss(N, L, **kw):
    return mk.Blockparam.scaled(n=3 * L, N=N, blk_d=3, blk_len=L, **kw)


def kmsb(N, L, **kw):
    return mk.KMS2partyblock.scaled(n=3 * L, N=N, blk_d=3, blk_len=L, **kw)


def ccs(N, **kw):
    return mk.CCS2party.scaled(n=3, N=N, **kw)


def _k1_walk(p):
    """both rot_variants of blindrotate_k1_kernel (rot_wide 1: never the latency kernel), then the latency kernel where it exists"""
    walk = [(_V21, _K1), (_V22, _K1)]
    if p.blk_len <= 1 and wide_supported(logM(p.N), p.l_gsw):
        walk.append(({"rot_wide": 2}, _WIDE))
    return walk


def _blk_walk(p):
    """one rotation per workgroup (both rot_variants), then two and four where the grouped kernel exists at this size"""
    walk = [({"rot_blkg": 1, "rot_variant": 21}, _K1), ({"rot_blkg": 1, "rot_variant": 22}, _K1)]
    walk += [({"rot_blkg": G}, _BLK) for G in (2, 4) if blockg_supported(logM(p.N), G)]
    return walk


def _kr_walk(p):
    L = p.blk_len if p.scheme == mk.LMSS else 1
    walk = [({"rot_blkg": 1}, _KR)]
    if blockg_np_covers(p.W, p.k, L) and blockg_supported(logM(p.N), 4):
        walk.append(({"rot_blkg": 4}, _BLK))
    return walk


_CCS_WALK = [({"ccs_pipe": 0}, _CCS), ({"ccs_pipe": 1}, _PIPE)]          # ccs_pipe_supported: every size (asserted through `reach`)


def _ladder_at(N):
    rows = []
    # k1, block length 1: 32-bit CGGI, 64-bit KMS (and kms_phase2_kernel), KMS on the 32-bit ring
    rows += [(cggi(N), _k1_walk(cggi(N))), (kms(N), _k1_walk(kms(N))), (kms32(N), [(_V22, _K1)])]
    # the latency kernel's other two gadget lengths, both widths
    if wide_supported(logM(N), 2):
        rows += [(p, [({"rot_wide": 2}, _WIDE)]) for p in (cggi(N, l_gsw=2, logB_gsw=10), cggi(N, l_gsw=4, logB_gsw=7),
                                                        kms(N, l_gsw=2, logB_gsw=16), kms(N, l_gsw=4, logB_gsw=9))]
    # k1 at block length 2, 3, 4 and the grouped kernel: 32-bit LMSS, 64-bit KMS_block
    for L in (2, 3, 4):
        rows += [(lmss(N, L), _blk_walk(lmss(N, L))), (kmsb(N, L), _blk_walk(kmsb(N, L)))]
    # kr at RLWE length 2, 3, plain and block, both widths; the three- and four-polynomial forms of the grouped kernel (32-bit ring)
    for W in (32, 64):
        for p in (cggi(N, k=2, W=W), cggi(N, k=3, W=W), lmss(N, 2, k=2, W=W), lmss(N, 2, k=3, W=W)):
            rows.append((p, _kr_walk(p)))
    bk2 = mk.Blockparam_k2.scaled(n=9, N=N, blk_d=3)
    rows.append((bk2, _kr_walk(bk2)))
    # kany at RLWE length 4, both widths
    rows += [(cggi(N, k=4, W=W), [({}, _KANY)]) for W in (32, 64)]
    # CCS on one and on two thread groups, both widths
    rows += [(ccs(N), _CCS_WALK), (ccs(N, W=64), _CCS_WALK)]
    return rows


# The instantiations with a compile-time gadget exist at M = 512 and M = 1024 only, for the shipped gadgets: there the rows above reach those, and
# the run-time-gadget instantiation of the same size needs a gadget of its own.  tests/edge_cases.py covers the compile-time gadgets under the
# default rot_variant; here also the other one.  (Found by the guard: each line is an instantiation it reported orphaned.)
def _gadget_rows():
    rows = []
    # M = 512: (3, 9) on the 32-bit ring at block length 1 and 3; l = 2 with a run-time base on both rings; (2, 16) on the 64-bit ring; the run-time gadget
    rows += [(cggi(1024, l_gsw=4, logB_gsw=7), [(_V21, _K1), (_V22, _K1)]),
             (cggi(1024, l_gsw=2, logB_gsw=10), [(_V21, _K1), (_V22, _K1)]),
             (kms(1024, l_gsw=2, logB_gsw=15), [(_V21, _K1), (_V22, _K1)]),
             (kms(1024, l_gsw=2, logB_gsw=16), [(_V21, _K1), (_V22, _K1)]),
             (lmss(1024, 3, l_gsw=4, logB_gsw=7), _blk_walk(lmss(1024, 3))),
             (ccs(1024, l_uni=2, logB_uni=10), _CCS_WALK), (ccs(2048, l_uni=2, logB_uni=10), _CCS_WALK)]
    rows += [(ccs(N, l_uni=l, logB_uni=b), _CCS_WALK) for N in (1024, 2048) for (l, b) in ((4, 8), (5, 6))]
    # M = 1024, 64-bit ring: the four KMS gadgets at block length 1 and 3, both rot_variants; the run-time gadget
    for (l, b) in ((5, 8), (4, 9), (6, 7)):
        rows += [(kms(2048, l_gsw=l, logB_gsw=b), [(_V21, _K1), (_V22, _K1)]),
                 (kmsb(2048, 3, l_gsw=l, logB_gsw=b), [({"rot_blkg": 1, "rot_variant": 21}, _K1), ({"rot_blkg": 1, "rot_variant": 22}, _K1)])]
    rows += [(kms(2048, l_gsw=2, logB_gsw=16), [(_V21, _K1), (_V22, _K1)]),
             (kmsb(2048, 3, l_gsw=2, logB_gsw=16), _blk_walk(kmsb(2048, 3)))]
    # Blockparam_k2's own gadget (3, 7) on four rotations per workgroup: the ladder's row at N = 1024 reaches it, this one the run-time gadget
    bk2 = mk.Blockparam_k2.scaled(n=9, N=1024, blk_d=3, logB_gsw=6)
    rows.append((bk2, _kr_walk(bk2)))
    return rows


LADDER = [row for N in SIZES for row in _ladder_at(N)] + _gadget_rows()


# ---- the same ladder on MKT_ARITH_EXACT contexts.  (parameter set, [(options, kernel), ...] or a refusal: the words its message must hold)
_X0 = {"exact_impl": 0}


def _exact_at(N):
    lm = logM(N)
    rows = []
    # CGGI, RLWE length 1: the integer kernel, the run-time-RLWE-length kernel, and the Float64 pipe from N = 128 at gadget length 3 and 2
    walk = [(_X0, "exact_blindrotate_kernel"), ({"exact_impl": 0, "exact_kany": 1}, "exact_blindrotate_kany_kernel")]
    if fx_supported(lm, 32, 3):
        walk.append(({"exact_impl": 1}, "fx_blindrotate_kernel"))
    rows.append((cggi(N), walk))
    if fx_supported(lm, 32, 2):
        rows.append((cggi(N, l_gsw=2, logB_gsw=10), [({"exact_impl": 1}, "fx_blindrotate_kernel")]))
    # LMSS: block length 3 on exact_blindrotate_kernel<.., 3>, any other on the general kernel; RLWE length 2, 3
    rows.append((lmss(N, 3), [(_X0, "exact_blindrotate_kernel")]))
    rows.append((lmss(N, 2), [(_X0, "exact_blindrotate_kr_kernel")]))
    rows += [(cggi(N, k=k), [(_X0, "exact_blindrotate_kr_kernel")]) for k in (2, 3)]
    # KMS: phase 1 one transform at a time and on the Float64 pipe; gadget length 2: also the paired-transform kernel; always exact_kms_phase2_kernel
    walk = [(_X0, "exact_kms_phase1_kernel")] + ([({"exact_impl": 1}, "fx_blindrotate_kernel")] if fx_supported(lm, 64, 3) else [])
    rows.append((kms(N), walk))
    walk = [({"exact_impl": 0, "exact_wide": 0}, "exact_kms_phase1_kernel"), ({"exact_impl": 0, "exact_wide": 1}, "exact_kms_phase1_p2pf_kernel")]
    walk += [({"exact_impl": 1}, "fx_blindrotate_kernel")] if fx_supported(lm, 64, 2) else []
    rows.append((kms(N, l_gsw=2, logB_gsw=14, l_lev=2, logB_lev=6, l_uni=3, logB_uni=10), walk))          # KMS2party_N1024_l2's gadgets, the base within the two-prime modulus up to N = 4096
    # KMS_block: per-block digit transforms, and per key bit
    # (at N = 4096 a block of three key bits with Blockparam's base 2^12 is beyond the two-prime modulus: EXACT_REFUSED; base 2^11 there)
    rows.append((kmsb(N, 3, logB_gsw=11 if N == 4096 else 12), [({"exact_impl": 0, "exact_wide": 1}, "exact_kms_block_phase1_kernel"), ({"exact_impl": 0, "exact_wide": 0}, "exact_kms_phase1_kernel")]))
    rows.append((ccs(N), [(_X0, "exact_ccs_kernel")]))
    return rows


EXACT_LADDER = [row for N in SIZES for row in _exact_at(N)]
# a gadget beyond the two-prime modulus is a refusal, not a skipped case: KMS with (2, 16) keeps phase 1 below P / 2 up to N = 1024 only
# (context.cpp exact_gate_ok: 2 l 2^(logB - 1) N 2^31 < 2^58.99), KMS_block with (3, 12) and block length 3 up to N = 2048 (2 blk_len times that)
EXACT_REFUSED = [(kms(N, l_gsw=2, logB_gsw=16), "two-prime modulus") for N in (2048, 4096)] + [(kmsb(4096, 3), "two-prime modulus")]


# ---- instantiations that NO parameter set validate_params admits can reach under any documented option value.  (pattern of the
# instantiation, predicate over its template arguments that states why, reason).  tests/test_size_ladder_cpu.py evaluates the predicate for
# every instantiation the pattern takes, and sweeps the admitted shapes and switch values through `reach`: a reachable one may not be here
def _targs(name):
    return [a.strip() for a in name[name.index("<") + 1:-1].split(",")]


EXCLUSIONS = [
    # launch_rot_one takes the (2, 16) gadget as constants on the 64-bit ring alone: the dropped part is exactly the low half of a 64-bit word
    (r"blindrotate_k1_kernel<9, unsigned int, 1, 2, [12], 2, 16>", lambda t: t[1] == "unsigned int" and (t[5], t[6]) == ("2", "16"),
     "the (2, 16) constants are taken where sizeof(WORD) == 8"),
    # launch_kr_word takes the block-length-3 constant on the 32-bit ring alone
    (r"blindrotate_kr_kernel<\d+, unsigned long, 2, true, 3>", lambda t: t[1] == "unsigned long" and t[4] == "3",
     "the block length is a constant where sizeof(WORD) == 4"),
]


# ---- the admitted envelope: corners of validate_params (block length >= 1, gadget lengths 1 .. 32, logB up to 31, key-switch gadgets with
# f logD <= 32 and logD <= 5), each at N = 256 and N = 32 in both arithmetic modes.  (parameter set, EXACT, name of the corner).  The engine
# serves a corner word for word or refuses it with a message that holds one of LIMIT_WORDS
def _corners(N):
    c = []
    for L in (1, 5):
        c += [(lmss(N, L), f"lmss-k1-blk{L}"), (lmss(N, L, k=2), f"lmss-k2-blk{L}"), (kmsb(N, L), f"kmsblock-blk{L}")]
    c += [(cggi(N, l_gsw=l, logB_gsw=b), f"gsw-{l}x{b}") for (l, b) in ((1, 16), (8, 4), (32, 1))]
    c += [(kms(N, l_gsw=l, logB_gsw=b), f"kms-gsw-{l}x{b}") for (l, b) in ((1, 31), (16, 4))]
    c += [(ccs(N, l_uni=1, logB_uni=16), "ccs-uni-1x16"), (ccs(N, l_uni=8, logB_uni=4), "ccs-uni-8x4")]
    c += [(kms(N, l_uni=1, logB_uni=31), "kms-uni-1x31"), (kms(N, l_uni=8, logB_uni=4), "kms-uni-8x4"),
          (kms(N, l_lev=1, logB_lev=14), "kms-lev-1x14"), (kms(N, l_lev=8, logB_lev=4), "kms-lev-8x4")]
    c += [(cggi(N, f=f, logD=d), f"ks-{f}x{d}") for (f, d) in ((16, 2), (32, 1), (8, 4), (1, 5))]
    return c


ENVELOPE = [(p, exact, what) for N in (256, 32) for (p, what) in _corners(N) for exact in (False, True)]
LIMIT_WORDS = ("block length", "two-prime modulus", "gadget")
# corners where words are the criterion and decryption is not asserted: the key-switch gadget (1, 5) keeps 5 bits of every word, and with the
# one-digit gadgets (1, 31) of KMS and (1, 16) of CCS the oracle itself decrypts wrongly at N = 256 (a single digit drops the low half of
# every word); every other corner decrypts under the oracle and must decrypt here
ENVELOPE_WORDS_ONLY = ("ks-1x5", "kms-gsw-1x31", "ccs-uni-1x16")
