// The launch rules of the blind rotation, pure: what a rotation call is (RotCall), and for each kernel family one function that answers it
// with a plan (RotPlan) -- which kernel a batch gets, how many rotations a workgroup takes, where the batch is cut into launches.  run_rot_plan
// is the one loop that launches a plan.  Host-only and free of HIP (as device_mem.h): tests/csrc/rot_plan_check.cpp walks the rules on a CPU.
// A plan never names a kernel that refuses the shape: which kernels exist for a shape comes in as the can_* flags, from the constexpr
// predicates below or from the *_supported function exported beside a kernel whose limits are Plan<> constants (blockg_supported,
// ccs_pipe_supported).  A leaf launcher handed a shape it does not cover returns hipErrorInvalidValue, and that is an error.
#pragma once
#include <stddef.h>

namespace mktd {

enum class RotKernel {
    PLAIN,             // blindrotate_k1_kernel, block length 1: one rotation per workgroup
    BLOCK,             // blindrotate_k1_kernel<LB > 1>: the block schemes, one rotation per workgroup
    WIDE,              // blindrotate_wide_kernel: the latency variant, one rotation on 2l thread groups
    GROUPED,           // blindrotate_blk_kernel (rot_block.hip): `group` rotations of one slot per workgroup
    KR,                // blindrotate_kr_kernel: RLWE length 2, 3
    FX,                // fx_blindrotate_kernel: exact products on the Float64 pipe
    CCS,               // ccs_blindrotate_kernel: one thread group per ciphertext
    CCS_PIPE,          // ccs_pipe_kernel: two thread groups per ciphertext
    XKMS_BLOCK_WIDE,   // exact_kms_block_phase1_kernel
    XKMS_BLOCK,        // exact_kms_phase1_kernel<true>: per key bit
    XKMS_P2PF,         // exact_kms_phase1_p2pf_kernel: paired transforms, gadget length 2
    XKMS,              // exact_kms_phase1_kernel<false>: one transform at a time
};

// A rotation call.  split: -1 = one launch, 0 = the family's rule, n > 0 = n rotations per launch.  The other switches as device_api.h
// (RotArgs, FxRotArgs, ExactKmsArgs) and the SWITCHES table of context.cpp state them.
struct RotCall {
    int logM, W;                     // log2 of the transform size, ring width in bits
    int l, blk_len, kr;              // gadget length, block length (1: none), RLWE length
    size_t rows, ncts, nrot;         // rotations per ciphertext, ciphertexts, rotations of the call (rows * ncts from every caller)
    int wide, split, blk_group, variant, ccs_pipe, exact_wide;
    unsigned block0;                 // the caller's first rotation: every launch of the plan starts at block0 + its offset
    bool can_wide, can_g2, can_g4, can_fx, can_ccs_pipe;   // the kernels that exist for this shape
};

// rotations `first` .. `first + count - 1` of the call on one kernel, `per_launch` to a launch (the last launch takes what is left)
struct RotSeg {
    RotKernel kind;
    int group;                       // rotations per workgroup (1; 2 or 4: GROUPED)
    int variant;                     // PLAIN, BLOCK: 10 * LOGR + transforms per thread group, resolved (rot_variant); 0 elsewhere
    size_t first, count, per_launch;
    size_t launches() const { return (count + per_launch - 1) / per_launch; }
};
struct RotPlan {
    int nseg;
    RotSeg seg[3];
    void add(RotKernel kind, int group, int variant, size_t count, size_t per_launch) {   // behind what is planned; nothing for no rotation
        if (!count) return;
        const size_t first = nseg ? seg[nseg - 1].first + seg[nseg - 1].count : 0;
        seg[nseg++] = RotSeg{kind, group, variant, first, count, per_launch < count ? per_launch : count};
    }
};

// ---- which kernels exist for a shape
constexpr bool wide_supported(int logM, int l, int blk_len) { return blk_len == 1 && logM >= 8 && logM <= 10 && l >= 2 && l <= 4; }
constexpr bool fx_supported(int logM, int W, int l) { return logM >= 6 && logM <= 11 && (W == 32 || W == 64) && (l == 2 || l == 3); }
// the grouped kernel at three and four accumulator polynomials (RLWE length 2, 3; rot_block.hip launch_blk_np): the 32-bit ring, four rotations
// per workgroup, block length 3 at RLWE length 2 and the plain CMux at both
constexpr bool blockg_np_covers(int W, int kr, int blk_len) { return W == 32 && ((kr == 2 && (blk_len == 3 || blk_len == 1)) || (kr == 3 && blk_len == 1)); }

// variant = 10*LR + NB for the plain schemes (tuning knob).  Only LR == LOGR variants are built: the device
// point order of the key tables is tied to the points-per-thread of the schedule.
constexpr int rot_variant(int variant, int LM, int l, int blk_len) {
    if (variant == 0) variant = (LM <= 10 || blk_len > 1) ? 22 : 21;   // pairs of transforms up to M = 1024 (re-measured with the specialised kernels: +4 % at M = 1024) and for the block schemes; single transforms above (LDS)
    if ((2 * l) % (variant % 10) != 0) variant = (variant / 10) * 10 + 1;
    return variant;
}

// rotations per launch under the split switch where the family has no rule of its own
constexpr size_t split_launch(int split, size_t nrot) { return split > 0 && (size_t)split < nrot ? (size_t)split : nrot; }

// ---- k1: the Float64 single-polynomial family (CGGI / LMSS with RLWE length 1, and every row of KMS / KMS_block phase 1)
inline RotPlan plan_k1(const RotCall &c) {
    RotPlan p{};
    const size_t nrot = c.nrot;
    const int logM = c.logM, W = c.W;
    const int variant = rot_variant(c.variant, logM, c.l, c.blk_len);
    // few rotations in flight (a single gate, small batches): the latency variant spreads one rotation over 2l thread
    // groups of one CU; a.wide: 0 = automatic (at most one rotation per CU, M <= 512: measured 3-16 % less latency there,
    // 2x MORE at M = 1024 where the groups need 8 points per thread), 1 = never, 2 = always where supported
    if (c.wide != 1 && c.can_wide && (c.wide == 2 || (nrot <= 256 && logM <= 9))) {
        p.add(RotKernel::WIDE, 1, 0, nrot, nrot);
        return p;
    }
    // A batch is run in rounds of one chip-fill (256 CUs x 4 two-wave workgroups at M = 512), and a round costs one
    // rotation's serial latency however few workgroups it holds.  A last round of at most one rotation per CU goes to the
    // latency variant instead (3.2 instead of 5.9 ms at KMS k = 2, N = 1024); same (ciphertext, slot) numbering via block0.
    constexpr size_t FILL = 1024;
    if (c.wide == 0 && c.blk_len == 1 && logM == 9 && c.split == 0 && nrot > FILL && nrot % FILL != 0 && nrot % FILL <= 256 && c.can_wide) {
        const size_t rem = nrot % FILL, head = nrot - rem;
        p.add(RotKernel::PLAIN, 1, variant, head, head);
        p.add(RotKernel::WIDE, 1, 0, rem, rem);
        return p;
    }
    // ONE chip-fill and a remainder of 288..512 rotations run as two EQUAL launches (three workgroups per CU each) instead of four
    // per CU and then two: a round costs 3.4 / 5.0 / 5.35 / 6.3 ms at 1 / 2 / 3 / 4 workgroups per CU (KMS k = 2, N = 1024: two
    // workgroups of a CU land on the same SIMD pair), so 2 x 5.35 beats 6.3 + 5.0 -- measured 512 KMS gates 11.2 -> 10.1 ms, 470:
    // 11.1 -> 10.1, 448: equal, 427 (remainder 257): 9.6 -> 10.0, hence the lower bound; CGGIparam 1300 / 1536 gates 15.6 / 16.3 ->
    // 14.5 / 14.7 ms.  Behind two or more fills the single launch drains better (853 gates: 15.6 vs 16.0 ms) and keeps the batch.
    // Same (ciphertext, slot) numbering via block0; gates/s no longer dips below the 256-gate rate at 512 gates.
    if (c.blk_len == 1 && logM == 9 && c.split == 0 && nrot > FILL && nrot <= 2 * FILL && nrot % FILL >= 288 && nrot % FILL <= 512) {
        const size_t tail = FILL + nrot % FILL, head = nrot - tail, half = (tail + 1) / 2;
        p.add(RotKernel::PLAIN, 1, variant, head, head);
        p.add(RotKernel::PLAIN, 1, variant, half, half);
        p.add(RotKernel::PLAIN, 1, variant, tail - half, tail - half);
        return p;
    }
    if (c.blk_len > 1) {
        // block schemes: G rotations of one slot per workgroup (rot_block.hip) once the batch fills the chip that way
        // automatic: four rotations per workgroup where that workgroup exists (M <= 512) and the batch still fills the
        // chip with one workgroup per compute unit (measured: Blockparam 5.54 -> 5.39 ms per 1024 gates; one rotation per
        // workgroup below that, and at M = 1024 where only two rotations fit and run 15 % slower)
        int G = c.blk_group;
        if (G == 0) G = (c.can_g4 && logM == 9 && nrot >= 1024) ? ((W == 32 && nrot >= 4096) ? 2 : 4) : 1;   // from 4096 rotations two rotations per workgroup, two workgroups per CU: 204 k against 196 k gates/s (Blockparam, 8192 and 16 384 gates)
        // 257..512 rotations: one 4-wave workgroup of two rotations per CU instead of two 2-wave workgroups, which share a SIMD pair
        // (tools/simd_place.hip): Blockparam 384 / 512 gates 4.51 -> 3.90 ms; up to 256 and from 513 to 1023 one rotation per workgroup is ahead
        if (c.blk_group == 0 && W == 32 && logM == 9 && nrot > 256 && nrot <= 512 && c.can_g2) G = 2;
        // 64-bit ring at M = 1024 (KMS_block, params.jl:87-125): two rotations per workgroup halve the key elements a thread holds, which
        // leaves room to re-request each for the next digit right after its last use (rot_block.hip); ahead up to about one KMS2partyblock
        // batch of 1024 gates (512 / 1024 gates: 16.6 / 32.3 ms against 17.2 / 33.3), behind from 2048 (63.4 against 62.5 ms)
        if (c.blk_group == 0 && W == 64 && logM == 10 && nrot >= 1536 && nrot <= 4096 && c.can_g2) G = 2;
        // the grouped kernel takes whole slots: every rotation of the call in one launch (a shape it does not cover, by LDS budget: one rotation per workgroup below)
        if (((G == 2 && c.can_g2) || (G == 4 && c.can_g4)) && c.blk_len >= 2 && c.blk_len <= 4 && nrot == c.rows * c.ncts) {
            p.add(RotKernel::GROUPED, G, 0, nrot, nrot);
            return p;
        }
        p.add(RotKernel::BLOCK, 1, variant, nrot, split_launch(c.split, nrot));
        return p;
    }
    p.add(RotKernel::PLAIN, 1, variant, nrot, split_launch(c.split, nrot));
    return p;
}

// ---- kr: the Float64 family at RLWE length 2, 3
#ifndef MKT_KR_BLKG_MIN
#define MKT_KR_BLKG_MIN 1     // rotations from which the grouped kernel is the default: ahead at every batch size (128 gates: 9.1 vs 13.9 ms, tools/blkg_ab.sh)
#endif
inline RotPlan plan_kr(const RotCall &c) {
    RotPlan p{};
    const size_t nrot = c.nrot;
    // 32-bit ring, LMSS with RLWE length 2 and block length 3, CGGI with RLWE length 2 or 3: four rotations per workgroup share every
    // key element (rot_block.hip); blk_group (MKT_ROT_BLKG): 0 = by batch size, 1 = never, 4 = always
    if (c.ncts == nrot && blockg_np_covers(c.W, c.kr, c.blk_len)) {
        int G = c.blk_group;
        // by default where it measured ahead (tools/blkg_ab.sh, tools/kr_time.py): block length 3 at RLWE length 2 (14.1 -> 10.0 ms per 1024
        // gates) and the plain CMux at RLWE length 3 (38.8 -> 24.3 ms); the plain CMux at RLWE length 2 stays on the one-rotation kernel
        // (17.0 vs 17.9 ms at 1024 gates, 13.0 vs 17.8 at 256)
        if (G == 0) G = (c.can_g4 && nrot >= MKT_KR_BLKG_MIN && !(c.kr == 2 && c.blk_len == 1)) ? 4 : 1;
        if (G == 4 && c.can_g4) {
            p.add(RotKernel::GROUPED, 4, 0, nrot, nrot);
            return p;
        }
    }
    p.add(RotKernel::KR, 1, 0, nrot, nrot);
    return p;
}

// ---- the Float64-pipe exact kernel (fx_exact.hip); nothing where the kernel does not exist for the shape
inline RotPlan plan_fx(const RotCall &c) {
    RotPlan p{};
    if (!c.can_fx) return p;
    // One launch per chip-fill on the 64-bit ring up to N = 1024.  Every rotation of a party walks the same key rows, step by step, and the workgroups of ONE fill run in
    // lock-step, so a fill reads each row from the fabric once per L2 and then hits; in a single launch of several fills the later workgroups start whenever a slot frees,
    // the resident ones spread over all key bits and the 4 x larger key of this arithmetic no longer fits the L2s (headline: hit rate 0.66 -> 0.96, 34.3 -> 31.6 ms).  At
    // N = 2048 (512 workgroups per fill, hit rate 0.98 either way) the six launch tails cost more than the locality gives (KMS2party 105.2 vs 101.7 ms in one launch), on the
    // 32-bit ring it makes no difference (profiles/r06_experiments.txt).  a.split: 0 = this rule, -1 = one launch, > 0 = that many workgroups per launch.
    size_t chunk = c.nrot;
    if (c.split == 0 && c.W == 64 && c.logM <= 9) chunk = (size_t)256 * 4;
    else if (c.split > 0) chunk = (size_t)c.split;
    p.add(RotKernel::FX, 1, 0, c.nrot, chunk);
    return p;
}

// ---- CCS: one thread group per ciphertext, or two
inline RotPlan plan_ccs(const RotCall &c) {
    RotPlan p{};
    const size_t B = c.nrot;
    // batches that leave compute units idle run each ciphertext on two thread groups (ccs_pipe.hip); option ccs_pipe: 0 never,
    // 1 always, -1: below one chip-fill of one-group workgroups (4 per CU at M = 512, 2 at M = 1024)
    const int pipe = c.ccs_pipe;
    const size_t fill = (size_t)256 * (c.logM <= 9 ? 4 : 2);
    const bool use_pipe = pipe == 1 || (pipe < 0 && B * 2 <= fill);
    p.add(use_pipe && c.can_ccs_pipe ? RotKernel::CCS_PIPE : RotKernel::CCS, 1, 0, B, B);
    return p;
}

// ---- EXACT KMS phase 1 (ntt_exact.hip): which of the four kernels
inline RotPlan plan_exact_kms_phase1(const RotCall &c) {
    RotPlan p{};
    RotKernel kind = RotKernel::XKMS;
    if (c.blk_len > 1 && c.exact_wide != 0) kind = RotKernel::XKMS_BLOCK_WIDE;   // exact_wide = 0: the per-key-bit kernel below (tests force both)
    else if (c.blk_len > 1) kind = RotKernel::XKMS_BLOCK;
    else if (c.exact_wide != 0 && c.l == 2) kind = RotKernel::XKMS_P2PF;         // the paired-transform kernel (default); exact_wide = 0: the one-at-a-time kernel below (tests force both)
    p.add(kind, 1, 0, c.nrot, c.nrot);
    return p;
}

// ---- the one loop that launches a plan: leaf(segment, args of the launch, rotations of the launch) launches one kernel, one grid, and returns
// the runtime's error code (0: success), which ends the loop.  `a` is the argument struct of the family where it carries block0
template <typename Args, typename Leaf>
auto run_rot_plan(const RotPlan &p, const Args &a, Leaf leaf) -> decltype(leaf(p.seg[0], a, (size_t)0)) {
    Args b = a;
    for (int i = 0; i < p.nseg; i++) {
        const RotSeg &g = p.seg[i];
        for (size_t off = 0; off < g.count; off += g.per_launch) {
            b.block0 = a.block0 + (unsigned)(g.first + off);
            const auto e = leaf(g, b, g.count - off < g.per_launch ? g.count - off : g.per_launch);
            if (e != decltype(e){}) return e;
        }
    }
    return {};
}

}  // namespace mktd
