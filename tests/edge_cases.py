"""The case lists of tests/test_gpu_edges.py.  tests/test_edges_cpu.py imports the same lists and asserts that the builders of
helpers.py put every boundary class into the inputs of every set named here, so the GPU cases cannot drift into testing nothing."""
from helpers import mk

_CG = mk.CGGIparam.scaled(n=20, N=256)
_BL2 = mk.Blockparam.scaled(n=24, N=256, blk_d=12, blk_len=2)
_BL3 = mk.Blockparam.scaled(n=30, N=256, blk_d=10)
_BL4 = mk.Blockparam.scaled(n=24, N=512, blk_d=6, blk_len=4)
_K2 = mk.KMS2party.scaled(n=8, N=256)
_KB = mk.KMS2partyblock.scaled(n=12, N=256, blk_d=4)
_CC2 = mk.CCS2party.scaled(n=8, N=256)
_KX2 = mk.KMS2party_N1024_l2.scaled(n=6, N=256)
_KXB = mk.KMS2partyblock.scaled(n=6, N=256, blk_d=2)


def sid(p):
    """a set of KS_SETS that differs from an earlier one in the key-switch gadget alone names its gadget too"""
    return f"{p.name}-n{p.n}-N{p.N}-k{p.k}-b{p.blk_len}" + (f"-f{p.f}x{p.logD}" if p in _KS_GADGET_TWINS else "")


# (parameter set, options, kernel the case means to reach, batch size, the (gadget length, log2 base) that the instantiation it means to
# reach holds as compile-time constants -- mkt_get_metric "rot_static_l" / "rot_static_logB", 0 = a run-time value): blind rotation,
# Float64 mode.  B = 5 is ragged for every grouping; 9 is one past a grouping of 8 (rot_map), 3 / 5 one past 2 / 4 rotations per
# workgroup (rot_block.hip)
ROT_CASES = [
    (_CG, {"rot_wide": 1, "rot_variant": 21}, "blindrotate_k1_kernel", 5, (0, 0)),
    (_CG, {"rot_wide": 1, "rot_variant": 22}, "blindrotate_k1_kernel", 9, (0, 0)),
    (_CG, {"rot_wide": 1, "rot_map": 0}, "blindrotate_k1_kernel", 9, (0, 0)),
    (_CG, {"rot_wide": 1, "rot_map": 1, "rot_stagger": 64}, "blindrotate_k1_kernel", 5, (0, 0)),
    (mk.CGGIparam.scaled(n=12, N=512), {"rot_wide": 2}, "blindrotate_wide_kernel", 5, (3, 0)),
    (mk.CGGI_N1024_l2.scaled(n=8), {"rot_wide": 1, "rot_variant": 22}, "blindrotate_k1_kernel", 3, (2, 0)),
    (mk.CGGIparam.scaled(n=4, N=4096), {"rot_wide": 1}, "blindrotate_k1_kernel", 3, (0, 0)),
    (mk.CGGIparam.scaled(n=8, N=64), {"rot_wide": 1}, "blindrotate_k1_kernel", 5, (0, 0)),
    (mk.CGGIparam.scaled(n=12, N=256, k=2), {"rot_blkg": 1}, "blindrotate_kr_kernel", 5, (0, 0)),
    (mk.CGGIparam.scaled(n=12, N=256, k=2), {"rot_blkg": 4}, "blindrotate_blk_kernel", 5, (0, 0)),
    (mk.CGGIparam.scaled(n=8, N=512, k=3, l_gsw=2, logB_gsw=10), {"rot_blkg": 1}, "blindrotate_kr_kernel", 5, (0, 0)),
    (mk.CGGIparam.scaled(n=8, N=256, k=4), {}, "blindrotate_kany_kernel", 5, (0, 0)),
    (mk.CGGIparam.scaled(n=6, N=128, k=6, l_gsw=2, logB_gsw=10), {}, "blindrotate_kany_kernel", 5, (0, 0)),
    (_BL2, {"rot_blkg": 1}, "blindrotate_k1_kernel", 5, (0, 0)), (_BL2, {"rot_blkg": 2}, "blindrotate_blk_kernel", 3, (0, 0)), (_BL2, {"rot_blkg": 4}, "blindrotate_blk_kernel", 5, (0, 0)),
    (_BL3, {"rot_blkg": 1}, "blindrotate_k1_kernel", 5, (0, 0)), (_BL3, {"rot_blkg": 2}, "blindrotate_blk_kernel", 5, (0, 0)), (_BL3, {"rot_blkg": 4}, "blindrotate_blk_kernel", 9, (0, 0)),
    (_BL4, {"rot_blkg": 1}, "blindrotate_k1_kernel", 5, (0, 0)), (_BL4, {"rot_blkg": 2}, "blindrotate_blk_kernel", 5, (0, 0)), (_BL4, {"rot_blkg": 4}, "blindrotate_blk_kernel", 5, (0, 0)),
    (mk.Blockparam_k2.scaled(n=12, N=256, blk_d=4), {"rot_blkg": 4}, "blindrotate_blk_kernel", 5, (0, 0)),
    (mk.Blockparam_k2.scaled(n=12, N=256, blk_d=4), {"rot_blkg": 1}, "blindrotate_kr_kernel", 5, (0, 0)),
    (_CC2, {"ccs_pipe": 0}, "ccs_blindrotate_kernel", 5, (0, 0)), (_CC2, {"ccs_pipe": 1}, "ccs_pipe_kernel", 5, (0, 0)),
    (mk.CCS8party.scaled(n=2, N=512, k=3), {"ccs_pipe": 0}, "ccs_blindrotate_kernel", 5, (0, 0)), (mk.CCS8party.scaled(n=2, N=512, k=3), {"ccs_pipe": 1}, "ccs_pipe_kernel", 5, (0, 0)),
    (mk.CCS16party.scaled(n=2, N=128, k=5), {"ccs_pipe": 0}, "ccs_blindrotate_kernel", 5, (0, 0)), (mk.CCS16party.scaled(n=2, N=128, k=5), {"ccs_pipe": 1}, "ccs_pipe_kernel", 5, (0, 0)),
    (mk.CCS2party.scaled(n=2, N=4096), {"ccs_pipe": 0}, "ccs_blindrotate_kernel", 3, (0, 0)),
    (_K2, {"rot_wide": 1, "rot_variant": 21}, "blindrotate_k1_kernel", 5, (0, 0)),
    (mk.KMS2party_N1024_l2.scaled(n=6), {"rot_wide": 2}, "blindrotate_wide_kernel", 5, (2, 0)),
    (mk.KMS4party.scaled(n=6, N=256), {"rot_wide": 1, "rot_map": 1}, "blindrotate_k1_kernel", 5, (0, 0)),
    (mk.KMS2party.scaled(n=2, N=4096), {"rot_wide": 1}, "blindrotate_k1_kernel", 3, (0, 0)),
    (_KB, {"rot_blkg": 1}, "blindrotate_k1_kernel", 5, (0, 0)), (_KB, {"rot_blkg": 2}, "blindrotate_blk_kernel", 5, (0, 0)),
]

# The instantiations that the shipped sets and the benchmark run: gadget length and base are template constants, picked by the launchers
# (launch_rot_one, launch_blk_g / launch_blk_np, launch_ccs_blindrotate / launch_ccs_pipe, launch_wide_lm) at the shipped N, word, block
# length and gadget only.  Each set keeps those of its shipped set and reduces n, blk_d and the party count, which the dispatch does not
# read; one line per instantiation, and the pair it must reach.  With batches this small the default route at M <= 512 is the latency
# kernel: rot_wide 1 where blindrotate_k1_kernel is meant.  tests/test_edges_cpu.py holds this list against the launchers' source
_X2 = mk.KMS2party_N1024_l2.scaled(n=6)
_X2B15 = mk.KMS2party_N1024_l2.scaled(name="KMS2party_N1024_l2_logB15", n=6, logB_gsw=15)
_CG1 = mk.CGGIparam.scaled(n=8)
_BL1 = mk.Blockparam.scaled(n=12, blk_d=4)
_BLK2 = mk.Blockparam_k2.scaled(n=12, blk_d=4)
_KMS = [mk.KMS2party.scaled(n=6), mk.KMS4party.scaled(n=4, k=2), mk.KMS8party.scaled(n=4, k=2), mk.KMS32party.scaled(n=4, k=2)]
_KMSB = [q.scaled(n=6, blk_d=2, k=2) for q in (mk.KMS2partyblock, mk.KMS4partyblock, mk.KMS8partyblock, mk.KMS32partyblock)]
_CCS1 = [mk.CCS2party.scaled(n=4), mk.CCS4party.scaled(n=2, k=2), mk.CCS8party.scaled(n=2, k=2)]
_CCS2 = [mk.CCS2party.scaled(n=4, N=2048), mk.CCS4party.scaled(n=2, k=2, N=2048), mk.CCS8party_N2048.scaled(n=2, k=2)]
_K1, _BLK, _CCS, _PIPE, _WIDE = "blindrotate_k1_kernel", "blindrotate_blk_kernel", "ccs_blindrotate_kernel", "ccs_pipe_kernel", "blindrotate_wide_kernel"
ROT_CASES += [
    # blindrotate_k1_kernel, M = 512: the 64-bit ring's (2, 16) -- the dropped part is exactly the low half -- and l = 2 with a run-time base
    (_X2, {"rot_wide": 1}, _K1, 5, (2, 16)), (_X2, {"rot_wide": 1, "rot_variant": 21}, _K1, 3, (2, 16)),
    (_X2B15, {"rot_wide": 1}, _K1, 5, (2, 0)),
    # ... the 32-bit ring's (3, 9), block length 1 and 3
    (_CG1, {"rot_wide": 1}, _K1, 5, (3, 9)), (_CG1, {"rot_wide": 1, "rot_variant": 21}, _K1, 3, (3, 9)),
    (_BL1, {"rot_blkg": 1}, _K1, 5, (3, 9)),
    # ... M = 1024, 64-bit ring: the four KMS gadgets, block length 1 and 3
    (_KMS[0], {"rot_wide": 1}, _K1, 5, (3, 12)), (_KMS[0], {"rot_wide": 1, "rot_variant": 21}, _K1, 3, (3, 12)),
    (_KMS[1], {"rot_wide": 1}, _K1, 5, (5, 8)), (_KMS[2], {"rot_wide": 1}, _K1, 5, (4, 9)), (_KMS[3], {"rot_wide": 1}, _K1, 5, (6, 7)),
    (_KMSB[0], {"rot_blkg": 1}, _K1, 5, (3, 12)), (_KMSB[1], {"rot_blkg": 1}, _K1, 5, (5, 8)), (_KMSB[2], {"rot_blkg": 1}, _K1, 5, (4, 9)),
    (_KMSB[3], {"rot_blkg": 1}, _K1, 5, (6, 7)),
    # blindrotate_blk_kernel: two and four rotations per workgroup (one past each), and the three-polynomial form of Blockparam_k2
    (_BL1, {"rot_blkg": 2}, _BLK, 3, (3, 9)), (_BL1, {"rot_blkg": 4}, _BLK, 5, (3, 9)),
    (_KMSB[0], {"rot_blkg": 2}, _BLK, 3, (3, 12)),
    (_BLK2, {"rot_blkg": 4}, _BLK, 5, (3, 7)),
    # the CCS kernels, one and two thread groups per ciphertext, M = 512 and 1024
    (_CCS1[0], {"ccs_pipe": 0}, _CCS, 5, (3, 8)), (_CCS1[0], {"ccs_pipe": 1}, _PIPE, 5, (3, 8)),
    (_CCS1[1], {"ccs_pipe": 0}, _CCS, 5, (4, 8)), (_CCS1[1], {"ccs_pipe": 1}, _PIPE, 5, (4, 8)),
    (_CCS1[2], {"ccs_pipe": 0}, _CCS, 5, (5, 6)), (_CCS1[2], {"ccs_pipe": 1}, _PIPE, 5, (5, 6)),
    (_CCS2[0], {"ccs_pipe": 0}, _CCS, 3, (3, 8)), (_CCS2[0], {"ccs_pipe": 1}, _PIPE, 3, (3, 8)),
    (_CCS2[1], {"ccs_pipe": 0}, _CCS, 3, (4, 8)), (_CCS2[1], {"ccs_pipe": 1}, _PIPE, 3, (4, 8)),
    (_CCS2[2], {"ccs_pipe": 0}, _CCS, 3, (5, 6)), (_CCS2[2], {"ccs_pipe": 1}, _PIPE, 3, (5, 6)),
    # blindrotate_wide_kernel at M = 1024: eight points per thread, l = 3 and 4, both rings (its gadget length is always a constant)
    (_KMS[0], {"rot_wide": 2}, _WIDE, 5, (3, 0)), (_KMS[2], {"rot_wide": 2}, _WIDE, 5, (4, 0)),
    (mk.CGGIparam.scaled(n=6, N=2048), {"rot_wide": 2}, _WIDE, 5, (3, 0)),
]

# EXACT mode (N <= 256: compared with tests/ref_exact.py; above: the two implementations with each other).  exact_impl 1 with a
# kernel name of the integer NTT: a shape the Float64 pipe does not serve
EXACT_CASES = [
    (mk.CGGIparam.scaled(n=10, N=256), {"exact_impl": 0}, "exact_blindrotate_kernel", 5),
    (mk.CGGIparam.scaled(n=10, N=256), {"exact_impl": 1}, "fx_blindrotate_kernel", 5),
    (mk.CGGIparam.scaled(n=8, N=256), {"exact_impl": 0, "exact_kany": 1}, "exact_blindrotate_kany_kernel", 5),
    (mk.CGGIparam.scaled(n=8, N=128, k=2), {"exact_impl": 0}, "exact_blindrotate_kr_kernel", 5),
    (mk.Blockparam.scaled(n=12, N=256, blk_d=6, blk_len=2), {"exact_impl": 0}, "exact_blindrotate_kr_kernel", 5),
    (mk.Blockparam.scaled(n=12, N=256, blk_d=4), {"exact_impl": 0}, "exact_blindrotate_kernel", 5),
    (mk.Blockparam.scaled(n=12, N=256, blk_d=3, blk_len=4), {"exact_impl": 0}, "exact_blindrotate_kr_kernel", 5),
    # KMS phase 1 on the integer NTT: at l_gsw = 2 exact_wide picks the one-at-a-time (0) or the paired-transform kernel (1, the default);
    # at any other gadget length there is one kernel; KMS_block: per-block digit transforms (1, the default) or per key bit (0)
    (_KX2, {"exact_impl": 0, "exact_wide": 0}, "exact_kms_phase1_kernel", 3),
    (_KX2, {"exact_impl": 0, "exact_wide": 1}, "exact_kms_phase1_p2pf_kernel", 3),
    (mk.KMS2party.scaled(n=6, N=256), {"exact_impl": 0}, "exact_kms_phase1_kernel", 3),
    (mk.KMS2party.scaled(n=6, N=256), {"exact_impl": 1}, "fx_blindrotate_kernel", 3),
    (_KX2, {"exact_impl": 1}, "fx_blindrotate_kernel", 3),
    (_KXB, {"exact_impl": 0, "exact_wide": 1}, "exact_kms_block_phase1_kernel", 3),
    (_KXB, {"exact_impl": 0, "exact_wide": 0}, "exact_kms_phase1_kernel", 3),
    (mk.CCS2party.scaled(n=4, N=256), {"exact_impl": 0}, "exact_ccs_kernel", 3),
]
EXACT_PAIR_SETS = [mk.CGGIparam.scaled(n=6, N=1024), mk.CGGIparam.scaled(n=4, N=4096), mk.KMS2party_N1024_l2.scaled(n=4), mk.KMS2party.scaled(n=2, N=4096)]

# key switch: the four full-length sets (D = 4, f even: the matrix-core kernel for the unbalanced digits of CGGIparam and CCS2party, the
# digit-pair kernel for the balanced ones of Blockparam_k2 and KMS2partyblock -- and for all four under MKT_KS_MFMA = 0, as the switch
# children of tests/test_gpu_switches.py run them), other gadgets (per-digit kernel; f = 5: stage-buffer
# parity), LMSS with n > N (whole components copied), and the LMSS copy rule's remaining branches: a component wholly beyond n (every
# coefficient switched) on the per-digit and on the digit-pair kernel, components wholly copied (and one cut at 44) on the per-digit kernel
KS_SETS = [
    mk.CGGIparam, mk.Blockparam_k2, mk.KMS2partyblock, mk.CCS2party,
    mk.CGGIparam.scaled(n=20, N=256, f=5, logD=3), mk.Blockparam.scaled(n=30, N=256, blk_d=10, f=4, logD=3),
    mk.KMS2party.scaled(n=12, N=256, f=5, logD=3), mk.KMS2partyblock.scaled(n=24, N=256, blk_d=8, f=4, logD=3),
    mk.Blockparam.scaled(n=300, N=128, blk_d=100, k=3), mk.Blockparam.scaled(n=150, N=128, blk_d=50, k=2, blk_len=3),
    mk.Blockparam.scaled(n=96, N=128, blk_d=32, k=2, f=4, logD=3), mk.Blockparam.scaled(n=300, N=128, blk_d=100, k=3, f=4, logD=3),
    mk.Blockparam.scaled(n=96, N=128, blk_d=32, k=2),
]
_KS_GADGET_TWINS = [p for i, p in enumerate(KS_SETS) if any(q != p and q.scaled(f=p.f, logD=p.logD) == p for q in KS_SETS[:i])]
KS_BATCHES = (1, 33, 70)
# the sets of the launcher-switch child (tests/test_gpu_switches.py _child_ks), reduced n
KS_CHILD_FULL = (mk.CGGIparam, (33,))          # and the full key length (the child's own first context), one ragged batch
KS_CHILD_SETS = [mk.CGGIparam.scaled(n=20, N=256), mk.KMS2party.scaled(n=12, N=256), mk.CCS2party.scaled(n=12, N=256),
                 mk.Blockparam.scaled(n=30, N=256, blk_d=10), mk.KMS2partyblock.scaled(n=24, N=256, blk_d=8),
                 mk.CGGIparam.scaled(n=20, N=256, f=5, logD=3)]

# key switch at a coefficient (keyswitch_pair_kernel, ks_digits_kernel, keyswitch_mg_kernel, ks_init_kernel / ks_reduce_kernel with AT = true,
# extract_word_at; tests/test_gpu_keyswitch_at.py runs the launcher switches in child processes): the same sets, the accumulators rotated
# by X^v so that the extraction at v meets the same words.  The four full-length sets: one batch of 33 over v in {0, 1, N - 1}
KS_AT_SETS = KS_SETS
KS_AT_FULL = KS_SETS[:4]
KS_AT_FULL_BATCHES = (33,)


def KS_AT_COEFS(p):
    """the sign boundary j = v at both ends, the first and last word, the block schemes' copy / switch border n, the middle"""
    return sorted({v for v in (0, 1, p.n - 1, p.n, p.n + 1, p.N // 2, p.N - 1) if 0 <= v < p.N})


def KS_AT_FULL_COEFS(p):
    return [0, 1, p.N - 1]


# whole bootstraps on crafted rows: one representative set per kernel (the fused mod switch / test vector is per kernel)
BOOT_CASES = [
    (_CG, {"rot_wide": 1}, "blindrotate_k1_kernel"),
    (mk.CGGIparam.scaled(n=12, N=512), {"rot_wide": 2}, "blindrotate_wide_kernel"),
    (mk.CGGIparam.scaled(n=12, N=256, k=2), {"rot_blkg": 1}, "blindrotate_kr_kernel"),
    (mk.CGGIparam.scaled(n=12, N=256, k=2), {"rot_blkg": 4}, "blindrotate_blk_kernel"),
    (mk.CGGIparam.scaled(n=8, N=256, k=4), {}, "blindrotate_kany_kernel"),
    (_BL3, {"rot_blkg": 1}, "blindrotate_k1_kernel"), (_BL3, {"rot_blkg": 4}, "blindrotate_blk_kernel"), (_BL2, {"rot_blkg": 2}, "blindrotate_blk_kernel"),
    (_CC2, {"ccs_pipe": 0}, "ccs_blindrotate_kernel"), (_CC2, {"ccs_pipe": 1}, "ccs_pipe_kernel"),
    (_K2, {"rot_wide": 1}, "blindrotate_k1_kernel"), (mk.KMS2party_N1024_l2.scaled(n=6), {"rot_wide": 2}, "blindrotate_wide_kernel"),
    (_KB, {"rot_blkg": 1}, "blindrotate_k1_kernel"), (_KB, {"rot_blkg": 2}, "blindrotate_blk_kernel"),
    # (appended: LUT_BOOT_CASES below indexes this list by position) three of the compile-time-gadget instantiations of ROT_CASES:
    # the (2, 16) one-rotation kernel, Blockparam's four rotations per workgroup, CCS2party on two thread groups
    (_X2, {"rot_wide": 1}, _K1), (_BL1, {"rot_blkg": 4}, _BLK), (_CCS1[0], {"ccs_pipe": 1}, _PIPE),
]
# the gate entry points (six gates, gate_ops, gate3, MUX) on crafted rows: the same kernels
GATE_CASES = BOOT_CASES
GATE_SETS = [_CG, _BL3, _CC2, _K2, _KB]          # one per scheme: the oracle-only identities of tests/test_edges_cpu.py
EXACT_BOOT_CASES = [c[:3] for c in EXACT_CASES]

# the one lookup-table route (context.cpp lut_chunk: lut_testvector_kernel with its own mod switch -- nu = 0 the plain one, nu > 0 the coarse
# switch whose words the rotation reads pre-switched from ws_lin --, the rotation, ks_at_table_kernel and the key switch at a coefficient)
# on crafted rows and tables: one line per rotation kernel (and the 64-bit ring's two), then MKT_ARITH_EXACT, one line per kernel.
# (parameter set, options, kernel, EXACT context)
LUT_BOOT_CASES = [c + (False,) for c in (BOOT_CASES[0], BOOT_CASES[1], BOOT_CASES[2], BOOT_CASES[3], BOOT_CASES[4], BOOT_CASES[6], BOOT_CASES[8], BOOT_CASES[9],
                                          BOOT_CASES[10], BOOT_CASES[13])] + \
                 [EXACT_CASES[i][:3] + (True,) for i in (0, 1, 2, 3, 5, 7, 8, 12, 14)]
LUT_NOUTS = (2, 4, 8)


def all_rotation_sets():
    seen, out = set(), []
    for p in [c[0] for c in ROT_CASES + EXACT_CASES + BOOT_CASES + GATE_CASES + LUT_BOOT_CASES] + EXACT_PAIR_SETS + GATE_SETS + KS_AT_SETS:
        key = p.scaled(f=8, logD=2)          # (the key-switch gadget plays no part in a rotation: such twins would only repeat a case)
        if key not in seen:
            seen.add(key)
            out.append(p)
    return out
