// The launch rules of the blind rotation (mktfhe_amd/csrc/rot_plan.h) on a CPU: every family's plan over a grid of shapes, switch values,
// capability flags (both ways: the plan takes them as inputs) and counts.  For every plan: the segments cover [0, count) in order without gap
// or overlap, every launch has at least one rotation, no kernel is planned whose capability is off or that belongs to another family, a grouped
// segment is a whole number of slots.  Then the fixed points of the k1 rule at M = 512, and run_rot_plan's block0 of every launch.
// Built by tests/test_rot_plan_cpu.py with AddressSanitizer and UBSan; includes the header alone.
#include "rot_plan.h"

#include <stdio.h>

#include <atomic>
#include <initializer_list>
#include <thread>
#include <vector>

using namespace mktd;

static std::atomic<long> g_failed{0}, g_plans{0};
static thread_local long t_plans = 0;   // a walker adds its count to g_plans when it ends
#define CHECK(cond, ...) do { if (!(cond)) { if (g_failed++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static const int SPLITS[] = {-1, 0, 1, 3, 7, 100, 1000, 5000}, WIDES[] = {0, 1, 2}, GROUPS[] = {0, 1, 2, 4};

static std::vector<size_t> counts() {
    std::vector<size_t> v;
    for (size_t n = 1; n <= 4200; n++) v.push_back(n);
    for (size_t n : {8191, 8192, 8193}) v.push_back(n);
    return v;
}
static const std::vector<size_t> COUNTS = counts();

static bool allowed(const RotCall &c, const RotSeg &g, std::initializer_list<RotKernel> family) {
    bool in = false;
    for (RotKernel k : family) in |= k == g.kind;
    if (!in) return false;
    switch (g.kind) {
    case RotKernel::WIDE:     return c.can_wide;
    case RotKernel::GROUPED:  return g.group == 2 ? c.can_g2 : g.group == 4 && c.can_g4;
    case RotKernel::FX:       return c.can_fx;
    case RotKernel::CCS_PIPE: return c.can_ccs_pipe;
    default:                  return true;
    }
}
// what every plan of every family keeps
static void check_plan(const char *family, const RotCall &c, const RotPlan &p, std::initializer_list<RotKernel> kinds) {
    size_t next = 0;
    bool ok = p.nseg >= 0 && p.nseg <= 3;
    for (int i = 0; ok && i < p.nseg; i++) {
        const RotSeg &g = p.seg[i];
        ok = g.first == next && g.count >= 1 && g.per_launch >= 1 && g.per_launch <= g.count && g.group >= 1 && allowed(c, g, kinds);
        if (g.kind == RotKernel::GROUPED) ok = ok && c.ncts && g.count % c.ncts == 0 && g.per_launch == g.count && (g.group == 2 || g.group == 4);
        else ok = ok && g.group == 1;
        if (g.kind == RotKernel::PLAIN || g.kind == RotKernel::BLOCK) ok = ok && g.variant == rot_variant(c.variant, c.logM, c.l, c.blk_len);
        next += g.count;
    }
    t_plans++;
    CHECK(ok && next == c.nrot, "%s logM %d W %d l %d blk %d kr %d rows %zu ncts %zu nrot %zu wide %d split %d blkg %d variant %d pipe %d xwide %d caps %d%d%d%d%d: %d segments, covered %zu",
          family, c.logM, c.W, c.l, c.blk_len, c.kr, c.rows, c.ncts, c.nrot, c.wide, c.split, c.blk_group, c.variant, c.ccs_pipe, c.exact_wide,
          c.can_wide, c.can_g2, c.can_g4, c.can_fx, c.can_ccs_pipe, p.nseg, next);
}

static void walk_k1(int logM, int W) {
    for (int l = 2; l <= 6; l++) for (int blk = 1; blk <= 4; blk++) for (int wide : WIDES) for (int G : GROUPS) for (int split : SPLITS) for (int caps = 0; caps < 8; caps++)
        for (int rows : {1, 4}) {
            if (rows == 4 && (blk == 1 || caps < 2 || split != 0)) continue;   // rotations per ciphertext matter to the grouped kernel alone, which no split cuts
            RotCall c{};
            c.logM = logM; c.W = W; c.l = l; c.blk_len = blk; c.kr = 1; c.wide = wide; c.blk_group = G; c.split = split;
            c.variant = (l + blk + caps) % 3 == 0 ? 0 : (l + blk + caps) % 3 == 1 ? 21 : 22;
            c.can_wide = caps & 1; c.can_g2 = caps & 2; c.can_g4 = caps & 4;
            for (size_t n : COUNTS) {
                c.nrot = n; c.rows = (size_t)rows; c.ncts = n / (size_t)rows;   // rows 4 at a count that is no multiple: no whole slots, nothing grouped
                check_plan("k1", c, plan_k1(c), {RotKernel::PLAIN, RotKernel::BLOCK, RotKernel::WIDE, RotKernel::GROUPED});
            }
        }
    g_plans += t_plans;
}
static void walk_rest() {
    for (int logM = 4; logM <= 11; logM++) for (int W : {32, 64}) for (int kr = 2; kr <= 3; kr++) for (int blk = 1; blk <= 4; blk++) for (int G : GROUPS) for (int split : SPLITS)
        for (int caps = 0; caps < 2; caps++) for (int rows : {1, 2}) {
            if (rows == 2 && split != 0) continue;
            RotCall c{};
            c.logM = logM; c.W = W; c.l = 3; c.blk_len = blk; c.kr = kr; c.blk_group = G; c.split = split; c.can_g2 = true; c.can_g4 = caps;
            for (size_t n : COUNTS) {
                c.nrot = n; c.rows = (size_t)rows; c.ncts = n / (size_t)rows;
                check_plan("kr", c, plan_kr(c), {RotKernel::KR, RotKernel::GROUPED});
            }
        }
    for (int logM = 6; logM <= 11; logM++) for (int W : {32, 64}) for (int l = 2; l <= 6; l++) for (int split : SPLITS) for (int can = 0; can < 2; can++) {
        RotCall c{};
        c.logM = logM; c.W = W; c.l = l; c.blk_len = 1; c.kr = 1; c.split = split; c.can_fx = can; c.rows = 1;
        for (size_t n : COUNTS) {
            c.nrot = c.ncts = n;
            const RotPlan p = plan_fx(c);
            if (!can) { t_plans++; CHECK(p.nseg == 0, "fx planned without the kernel"); continue; }
            check_plan("fx", c, p, {RotKernel::FX});
            if (split == 0 && W == 64 && logM <= 9) CHECK(p.seg[0].per_launch == (n < 1024 ? n : 1024), "fx chip-fill rule at %zu: %zu", n, p.seg[0].per_launch);
        }
    }
    for (int logM = 8; logM <= 11; logM++) for (int W : {32, 64}) for (int pipe : {-1, 0, 1}) for (int can = 0; can < 2; can++) {
        RotCall c{};
        c.logM = logM; c.W = W; c.l = 3; c.blk_len = 1; c.kr = 2; c.ccs_pipe = pipe; c.can_ccs_pipe = can; c.rows = 1;
        for (size_t n : COUNTS) {
            c.nrot = c.ncts = n;
            const RotPlan p = plan_ccs(c);
            check_plan("ccs", c, p, {RotKernel::CCS, RotKernel::CCS_PIPE});
            const bool want = can && (pipe == 1 || (pipe < 0 && 2 * n <= (size_t)(logM <= 9 ? 1024 : 512)));
            CHECK(p.nseg == 1 && (p.seg[0].kind == RotKernel::CCS_PIPE) == want, "ccs logM %d pipe %d can %d n %zu", logM, pipe, can, n);
        }
    }
    for (int l = 2; l <= 6; l++) for (int blk = 1; blk <= 4; blk++) for (int xw : {0, 1}) {
        RotCall c{};
        c.logM = 10; c.W = 64; c.l = l; c.blk_len = blk; c.kr = 1; c.exact_wide = xw; c.rows = 4;
        for (size_t n : COUNTS) {
            c.ncts = n; c.nrot = 4 * n;
            const RotPlan p = plan_exact_kms_phase1(c);
            check_plan("exact_kms", c, p, {RotKernel::XKMS, RotKernel::XKMS_P2PF, RotKernel::XKMS_BLOCK, RotKernel::XKMS_BLOCK_WIDE});
            const RotKernel want = blk > 1 ? (xw ? RotKernel::XKMS_BLOCK_WIDE : RotKernel::XKMS_BLOCK) : (xw && l == 2 ? RotKernel::XKMS_P2PF : RotKernel::XKMS);
            CHECK(p.nseg == 1 && p.seg[0].kind == want && p.seg[0].launches() == 1, "exact_kms l %d blk %d wide %d", l, blk, xw);
        }
    }
    g_plans += t_plans;
}

// ---- the launches of a plan as run_rot_plan issues them
struct Args { unsigned block0; };
struct Launch { RotKernel kind; size_t n; unsigned block0; };
static std::vector<Launch> launches(const RotCall &c, const RotPlan &p) {
    std::vector<Launch> v;
    const int e = run_rot_plan(p, Args{c.block0}, [&](const RotSeg &g, const Args &b, size_t n) { v.push_back(Launch{g.kind, n, b.block0}); return 0; });
    CHECK(e == 0, "run_rot_plan returned %d", e);
    return v;
}
static RotCall headline(size_t n) {   // M = 512, 32-bit ring, l = 3, every switch 0
    RotCall c{};
    c.logM = 9; c.W = 32; c.l = 3; c.blk_len = 1; c.kr = 1; c.rows = 1; c.ncts = c.nrot = n;
    c.can_wide = wide_supported(9, 3, 1); c.can_g2 = c.can_g4 = true;
    return c;
}
static void expect(size_t n, std::initializer_list<Launch> want) {
    const RotCall c = headline(n);
    const std::vector<Launch> got = launches(c, plan_k1(c));
    bool ok = got.size() == want.size();
    size_t i = 0;
    for (const Launch &w : want) { ok = ok && got[i].kind == w.kind && got[i].n == w.n && got[i].block0 == w.block0; i++; }
    CHECK(ok, "fixed point at %zu rotations: %zu launches", n, got.size());
}
static void fixed_points() {
    const RotKernel P = RotKernel::PLAIN, L = RotKernel::WIDE;
    expect(1, {{L, 1, 0}});            expect(256, {{L, 256, 0}});
    expect(257, {{P, 257, 0}});        expect(1024, {{P, 1024, 0}});
    expect(1124, {{P, 1024, 0}, {L, 100, 1024}});
    expect(1280, {{P, 1024, 0}, {L, 256, 1024}});
    expect(1281, {{P, 1281, 0}});      expect(1311, {{P, 1311, 0}});
    expect(1312, {{P, 656, 0}, {P, 656, 656}});
    expect(1424, {{P, 712, 0}, {P, 712, 712}});
    expect(1536, {{P, 768, 0}, {P, 768, 768}});
    expect(1537, {{P, 1537, 0}});      expect(2048, {{P, 2048, 0}});      expect(2348, {{P, 2348, 0}});
    // the loop: every launch starts where the one before ended, from the caller's block0; an error ends it
    for (int split : SPLITS) for (size_t n : {1, 99, 100, 101, 1124, 1312, 4200, 8193}) for (unsigned b0 : {0u, 5u}) {
        RotCall c = headline(n);
        c.split = split; c.block0 = b0; c.wide = split == 7 ? 1 : 0;
        const RotPlan p = plan_k1(c);
        size_t next = b0, total = 0;
        for (const Launch &x : launches(c, p)) { CHECK(x.block0 == next && x.n >= 1, "launch at %u, expected %zu", x.block0, next); next += x.n; total++; }
        size_t planned = 0;
        for (int i = 0; i < p.nseg; i++) planned += p.seg[i].launches();
        CHECK(next == b0 + n && total == planned, "split %d n %zu: %zu launches, %zu planned", split, n, total, planned);
        if (split > 0 && c.wide == 1) CHECK(total == (n + (size_t)split - 1) / (size_t)split, "split %d over %zu: %zu launches", split, n, total);
    }
    int calls = 0;
    const RotCall c = headline(1312);
    const int e = run_rot_plan(plan_k1(c), Args{0}, [&](const RotSeg &, const Args &, size_t) { calls++; return 7; });
    CHECK(e == 7 && calls == 1, "an error ends the loop: %d after %d calls", e, calls);
}

int main() {
    std::vector<std::thread> pool;
    for (int logM = 8; logM <= 11; logM++) for (int W : {32, 64}) pool.emplace_back(walk_k1, logM, W);
    pool.emplace_back(walk_rest);
    fixed_points();
    for (std::thread &t : pool) t.join();
    g_plans += t_plans;
    printf("%ld plans, %ld failed checks\n", g_plans.load(), g_failed.load());
    return g_failed ? 1 : 0;
}
