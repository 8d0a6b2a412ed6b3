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


# (parameter set, options, kernel the case means to reach, batch size): blind rotation, Float64 mode.  B = 5 is ragged for every
# grouping; 9 is one past a grouping of 8 (rot_map), 3 / 5 one past 2 / 4 rotations per workgroup (rot_block.hip)
ROT_CASES = [
    (_CG, {"rot_wide": 1, "rot_variant": 21}, "blindrotate_k1_kernel", 5),
    (_CG, {"rot_wide": 1, "rot_variant": 22}, "blindrotate_k1_kernel", 9),
    (_CG, {"rot_wide": 1, "rot_map": 0}, "blindrotate_k1_kernel", 9),
    (_CG, {"rot_wide": 1, "rot_map": 1, "rot_stagger": 64}, "blindrotate_k1_kernel", 5),
    (mk.CGGIparam.scaled(n=12, N=512), {"rot_wide": 2}, "blindrotate_wide_kernel", 5),
    (mk.CGGI_N1024_l2.scaled(n=8), {"rot_wide": 1, "rot_variant": 22}, "blindrotate_k1_kernel", 3),
    (mk.CGGIparam.scaled(n=4, N=4096), {"rot_wide": 1}, "blindrotate_k1_kernel", 3),
    (mk.CGGIparam.scaled(n=8, N=64), {"rot_wide": 1}, "blindrotate_k1_kernel", 5),
    (mk.CGGIparam.scaled(n=12, N=256, k=2), {"rot_blkg": 1}, "blindrotate_kr_kernel", 5),
    (mk.CGGIparam.scaled(n=12, N=256, k=2), {"rot_blkg": 4}, "blindrotate_blk_kernel", 5),
    (mk.CGGIparam.scaled(n=8, N=512, k=3, l_gsw=2, logB_gsw=10), {"rot_blkg": 1}, "blindrotate_kr_kernel", 5),
    (mk.CGGIparam.scaled(n=8, N=256, k=4), {}, "blindrotate_kany_kernel", 5),
    (mk.CGGIparam.scaled(n=6, N=128, k=6, l_gsw=2, logB_gsw=10), {}, "blindrotate_kany_kernel", 5),
    (_BL2, {"rot_blkg": 1}, "blindrotate_k1_kernel", 5), (_BL2, {"rot_blkg": 2}, "blindrotate_blk_kernel", 3), (_BL2, {"rot_blkg": 4}, "blindrotate_blk_kernel", 5),
    (_BL3, {"rot_blkg": 1}, "blindrotate_k1_kernel", 5), (_BL3, {"rot_blkg": 2}, "blindrotate_blk_kernel", 5), (_BL3, {"rot_blkg": 4}, "blindrotate_blk_kernel", 9),
    (_BL4, {"rot_blkg": 1}, "blindrotate_k1_kernel", 5), (_BL4, {"rot_blkg": 2}, "blindrotate_blk_kernel", 5), (_BL4, {"rot_blkg": 4}, "blindrotate_blk_kernel", 5),
    (mk.Blockparam_k2.scaled(n=12, N=256, blk_d=4), {"rot_blkg": 4}, "blindrotate_blk_kernel", 5),
    (mk.Blockparam_k2.scaled(n=12, N=256, blk_d=4), {"rot_blkg": 1}, "blindrotate_kr_kernel", 5),
    (_CC2, {"ccs_pipe": 0}, "ccs_blindrotate_kernel", 5), (_CC2, {"ccs_pipe": 1}, "ccs_pipe_kernel", 5),
    (mk.CCS8party.scaled(n=2, N=512, k=3), {"ccs_pipe": 0}, "ccs_blindrotate_kernel", 5), (mk.CCS8party.scaled(n=2, N=512, k=3), {"ccs_pipe": 1}, "ccs_pipe_kernel", 5),
    (mk.CCS16party.scaled(n=2, N=128, k=5), {"ccs_pipe": 0}, "ccs_blindrotate_kernel", 5), (mk.CCS16party.scaled(n=2, N=128, k=5), {"ccs_pipe": 1}, "ccs_pipe_kernel", 5),
    (mk.CCS2party.scaled(n=2, N=4096), {"ccs_pipe": 0}, "ccs_blindrotate_kernel", 3),
    (_K2, {"rot_wide": 1, "rot_variant": 21}, "blindrotate_k1_kernel", 5),
    (mk.KMS2party_N1024_l2.scaled(n=6), {"rot_wide": 2}, "blindrotate_wide_kernel", 5),
    (mk.KMS4party.scaled(n=6, N=256), {"rot_wide": 1, "rot_map": 1}, "blindrotate_k1_kernel", 5),
    (mk.KMS2party.scaled(n=2, N=4096), {"rot_wide": 1}, "blindrotate_k1_kernel", 3),
    (_KB, {"rot_blkg": 1}, "blindrotate_k1_kernel", 5), (_KB, {"rot_blkg": 2}, "blindrotate_blk_kernel", 5),
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

# key switch: the four full-length sets (digit-pair kernel: D = 4, f even), other gadgets (per-digit kernel; f = 5: stage-buffer
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
