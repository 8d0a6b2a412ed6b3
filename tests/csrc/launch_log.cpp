// What the rotation launchers launch, launch for launch, without a GPU.  The library's units that hold rotation launchers are compiled
// host-only and linked with this file, which stands in for the HIP runtime: registration hands over each kernel's device name, and
// hipLaunchKernel logs the name (demangled: the instantiation shows transform size, word type, variant and static gadget), grid.x, block.x,
// the dynamic LDS bytes and, for the kernels whose first argument carries one, block0.  main drives the public launchers (device_api.h) over
// the shipped shapes, one shape per transform size, the batch sizes around every cutting rule and the switch values of
// tests/test_gpu_switches.py, and ends with the line count and an FNV-1a digest of the log.  `log` as first argument prints the log itself.
// `kernels` prints every instantiation the units registered, launched or not; `reach` answers, for the shapes and option settings on its
// standard input, which of them a call launches (tests/test_size_ladder_cpu.py: no instantiation without a case).
//
// One source for two trees: tests/test_rot_plan_cpu.py pins the digest of this program built against the commit before rot_plan.h.  That
// commit has no launch_ccs: its rule (one thread group per ciphertext or two) stood in context.cpp's do_blindrotate, and a build against it
// (-DLAUNCH_LOG_CCS_RULE_OF_DO_BLINDROTATE) carries those lines verbatim behind the new launcher's name, below.
#include <cxxabi.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>

#include "device_api.h"

namespace mktd {
thread_local const char *last_rot_kernel = "";
thread_local int last_rot_static_l = 0, last_rot_static_logB = 0;
const LaunchTuning &launch_tuning() { static const LaunchTuning t{}; return t; }
#ifdef LAUNCH_LOG_CCS_RULE_OF_DO_BLINDROTATE
hipError_t launch_ccs(int logM, int W, const CcsArgs &q, int pipe, size_t B, hipStream_t stream) {
    const size_t fill = (size_t)256 * (logM <= 9 ? 4 : 2);
    const bool use_pipe = pipe == 1 || (pipe < 0 && B * 2 <= fill);
    if (use_pipe) {
        const hipError_t e = mktd::launch_ccs_pipe(logM, W, q, B, stream);
        if (e == hipSuccess) return hipSuccess;
        if (e != hipErrorInvalidValue) return e;
    }
    return mktd::launch_ccs_blindrotate(logM, W, q, B, stream);
}
#endif
}  // namespace mktd

namespace {

bool g_print = false;
bool g_reach = false;            // `reach`: hipLaunchKernel notes the instantiation and logs nothing
std::string g_reached;
uint64_t g_hash = 0xcbf29ce484222325ull;
size_t g_lines = 0;
void emit(const std::string &line) {
    for (const char ch : line + "\n") { g_hash ^= (unsigned char)ch; g_hash *= 0x100000001b3ull; }
    g_lines++;
    if (g_print) puts(line.c_str());
}
// registration runs during static initialisation: the table is a function-local static
std::map<const void *, std::string> &names() { static std::map<const void *, std::string> m; return m; }

struct { dim3 grid, block; size_t lds; hipStream_t stream; } g_cfg;

}  // namespace

extern "C" {
void **__hipRegisterFatBinary(const void *) { static void *module; return &module; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host_fn, char *, const char *device_name, unsigned, void *, void *, void *, void *, int *) {
    int status = 1;
    char *d = abi::__cxa_demangle(device_name, nullptr, nullptr, &status);
    std::string n = status == 0 && d ? d : device_name;
    free(d);
    const size_t anon = n.find("(anonymous namespace)::");             // "void mktd::[(anonymous namespace)::]kernel<...>(args)" -> "kernel<...>"
    if (anon != std::string::npos) n.erase(anon, 23);
    const size_t paren = n.find('(');
    if (paren != std::string::npos) n.resize(paren);
    const size_t ns = n.find("mktd::");
    if (ns != std::string::npos) n = n.substr(ns + 6);
    names()[host_fn] = n;
}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) { g_cfg = {grid, block, lds, stream}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *lds, hipStream_t *stream) {
    *grid = g_cfg.grid; *block = g_cfg.block; *lds = g_cfg.lds; *stream = g_cfg.stream;
    return hipSuccess;
}
}
hipError_t hipLaunchKernel(const void *fn, dim3 grid, dim3 block, void **args, size_t lds, hipStream_t) {
    const auto it = names().find(fn);
    const std::string n = it == names().end() ? "?" : it->second;
    if (g_reach) { g_reached += (g_reached.empty() ? "" : " | ") + n; return hipSuccess; }
    char tail[96];
    long block0 = -1;                                                  // the kernels whose first argument is a RotArgs / an FxRotArgs
    if (n.rfind("blindrotate_k1_kernel", 0) == 0 || n.rfind("blindrotate_wide_kernel", 0) == 0 || n.rfind("blindrotate_kr_kernel", 0) == 0 ||
        n.rfind("blindrotate_kany_kernel", 0) == 0 || n.rfind("blindrotate_blk_kernel", 0) == 0)
        block0 = (long)static_cast<const mktd::RotArgs *>(args[0])->block0;
    else if (n.rfind("fx_blindrotate_kernel", 0) == 0) block0 = (long)static_cast<const mktd::FxRotArgs *>(args[0])->block0;
    snprintf(tail, sizeof tail, " grid %u block %u lds %zu block0 %ld", grid.x, block.x, lds, block0);
    emit("  " + n + tail);
    return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }

namespace {
using namespace mktd;

enum Scheme { CGGI, LMSS, CCS, KMS, KMS_BLOCK };
struct Shape { const char *name; Scheme scheme; int N, k, W, l, logB, blk_len, rows; };   // l, logB: the gadget of the rotation's digit loop; rows: rotations per ciphertext
// the shipped sets (mktfhe_amd/params.py; KMS rows = k * l_lev), then RLWE length 2, 3 and one shape per transform size from 16 to 2048 points
const Shape SHAPES[] = {
    {"CGGIparam", CGGI, 1024, 1, 32, 3, 9, 1, 1},          {"Blockparam", LMSS, 1024, 1, 32, 3, 9, 3, 1},
    {"KMS2party", KMS, 2048, 2, 64, 3, 12, 1, 4},          {"KMS2party_N1024_l2", KMS, 1024, 2, 64, 2, 16, 1, 4},
    {"KMS2partyblock", KMS_BLOCK, 2048, 2, 64, 3, 12, 3, 4}, {"KMS4party", KMS, 2048, 4, 64, 5, 8, 1, 8},
    {"KMS8party", KMS, 2048, 8, 64, 4, 9, 1, 24},          {"KMS32party", KMS, 2048, 32, 64, 6, 7, 1, 96},
    {"CCS2party", CCS, 1024, 2, 32, 3, 8, 1, 1},           {"CCS4party", CCS, 1024, 4, 32, 4, 8, 1, 1},
    {"CCS8party", CCS, 1024, 8, 32, 5, 6, 1, 1},           {"CCS8party_N2048", CCS, 2048, 8, 32, 5, 6, 1, 1},
    {"CCS8party_N4096", CCS, 4096, 8, 32, 5, 6, 1, 1},     {"CCS2party_w64", CCS, 1024, 2, 64, 3, 8, 1, 1},
    {"CGGI_k2", CGGI, 1024, 2, 32, 3, 9, 1, 1},            {"CGGI_k3", CGGI, 1024, 3, 32, 3, 9, 1, 1},
    {"CGGI_k2_w64", CGGI, 1024, 2, 64, 3, 9, 1, 1},        {"Blockparam_k2", LMSS, 1024, 2, 32, 3, 7, 3, 1},
    {"LMSS_k2_b2", LMSS, 1024, 2, 32, 3, 7, 2, 1},         {"CGGI_N1024_l2", CGGI, 1024, 1, 32, 2, 8, 1, 1},
    {"CGGI_N32", CGGI, 32, 1, 32, 3, 9, 1, 1},             {"Block_N64", LMSS, 64, 1, 32, 3, 9, 3, 1},
    {"KMS_N128", KMS, 128, 2, 64, 3, 12, 1, 4},            {"Block_N256_b2", LMSS, 256, 1, 64, 2, 9, 2, 1},
    {"CGGI_N512", CGGI, 512, 1, 32, 4, 7, 1, 1},           {"Block_N512_b4", LMSS, 512, 1, 32, 3, 9, 4, 1},
    {"KMSblock_N1024", KMS_BLOCK, 1024, 2, 64, 3, 12, 3, 4}, {"Block_N2048", LMSS, 2048, 1, 32, 3, 9, 3, 1},
    {"Block_N4096", LMSS, 4096, 1, 32, 3, 9, 3, 1},        {"CGGI_N4096", CGGI, 4096, 1, 32, 3, 9, 1, 1},
    {"CGGI_N4096_l5", CGGI, 4096, 1, 64, 5, 8, 1, 1},
    {"CGGI_k3_N32", CGGI, 32, 3, 32, 3, 9, 1, 1},          {"Block_k2_N64", LMSS, 64, 2, 32, 3, 7, 3, 1},
    {"CGGI_k3_N128", CGGI, 128, 3, 32, 3, 9, 1, 1},        {"Block_k2_N256", LMSS, 256, 2, 32, 3, 7, 3, 1},
    {"CGGI_k3_N512", CGGI, 512, 3, 32, 3, 9, 1, 1},        {"Block_k2_N2048", LMSS, 2048, 2, 32, 3, 7, 3, 1},
    {"CGGI_k3_N4096", CGGI, 4096, 3, 32, 3, 9, 1, 1},      {"CGGI_k5", CGGI, 1024, 5, 32, 3, 9, 1, 1},
};
const size_t COUNTS[] = {1, 13, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1280, 1281, 1311, 1312, 1535, 1536, 1537,
                         2047, 2048, 2049, 2304, 2305, 4095, 4096, 4097, 8192};
struct Opts { int variant, wide, blkg, split; };

int logm(const Shape &sh) { int lg = 0; while ((2 << lg) < sh.N) lg++; return lg; }

// count rotations as whole ciphertexts where the rows divide them (the shape every caller hands over), else one row per ciphertext
void gates_of(const Shape &sh, size_t count, int &rows, size_t &ngates) {
    if (count % (size_t)sh.rows == 0) { rows = sh.rows; ngates = count / (size_t)sh.rows; } else { rows = 1; ngates = count; }
}
RotArgs rot_args(const Shape &sh, size_t count, const Opts &o) {
    RotArgs a{};
    a.l = sh.l; a.logB = sh.logB; a.blk_len = sh.blk_len; a.blk_accum = sh.blk_len > 1;
    gates_of(sh, count, a.rows_per_gate, a.ngates);
    a.variant = o.variant; a.wide = o.wide; a.blk_group = o.blkg; a.split = (unsigned)o.split; a.map_mode = 1;
    return a;
}
void head(const char *family, const Shape &sh, size_t count, const char *opts) {
    char line[200];
    snprintf(line, sizeof line, "%s %s n %zu %s", family, sh.name, count, opts);
    emit(line);
}
void done(hipError_t e) { emit(std::string("  -> ") + (e == hipSuccess ? "ok" : e == hipErrorInvalidValue ? "invalid value" : "error")); }

void f64_calls(const Shape &sh, size_t count, const Opts &o) {
    char opts[96];
    snprintf(opts, sizeof opts, "variant %d wide %d blkg %d split %d", o.variant, o.wide, o.blkg, o.split);
    const RotArgs a = rot_args(sh, count, o);
    const int kr = sh.scheme == KMS || sh.scheme == KMS_BLOCK ? 1 : sh.k;
    if (kr == 1) { head("k1", sh, count, opts); done(launch_blindrotate_k1(logm(sh), sh.W, a, count, nullptr)); }
    else if (kr <= 3) { head("kr", sh, count, opts); done(launch_blindrotate_kr(logm(sh), sh.W, kr, a, count, nullptr)); }
    else { head("kany", sh, count, opts); done(launch_blindrotate_kany(logm(sh), sh.W, kr, a, reinterpret_cast<cplx *>(16), count, nullptr)); }
}
void fx_calls(const Shape &sh, size_t count, int split) {
    char opts[48];
    snprintf(opts, sizeof opts, "split %d", split);
    FxRotArgs f{};
    f.l = sh.l; f.logB = sh.logB; f.split = split; f.map_mode = 1;
    gates_of(sh, count, f.rows_per_gate, f.ngates);
    head("fx", sh, count, opts);
    done(launch_fx_blindrotate(logm(sh), sh.W, f, count, nullptr));
}
void exact_kms_calls(const Shape &sh, size_t B, int wide, int phase2_only) {
    char opts[64];
    snprintf(opts, sizeof opts, "exact_wide %d phase2_only %d", wide, phase2_only);
    ExactKmsArgs q{};
    q.k = sh.k; q.l_gsw = sh.l; q.logB_gsw = sh.logB; q.rtot = sh.rows; q.blk_len = sh.blk_len; q.wide = wide; q.phase2_only = phase2_only;
    head("exact_kms", sh, B, opts);
    done(launch_exact_kms(logm(sh) + 1, nullptr, q, B, nullptr));
}
void ccs_calls(const Shape &sh, size_t B, int pipe) {
    char opts[32];
    snprintf(opts, sizeof opts, "ccs_pipe %d", pipe);
    CcsArgs q{};
    q.k = sh.k; q.l = sh.l; q.logB = sh.logB;
    head("ccs", sh, B, opts);
    done(launch_ccs(logm(sh), sh.W, q, pipe, B, nullptr));
}

// ---- `kernels`: every instantiation the units registered, launched or not, one per line
int print_kernels() {
    std::map<std::string, int> sorted;
    for (const auto &kv : names()) sorted[kv.second]++;
    for (const auto &kv : sorted) puts(kv.first.c_str());
    return 0;
}

// ---- `reach`: one shape and one option setting per line of standard input, as key=value words (the members of Reach; scheme by name); the
// route is that of context.cpp (rot_route / do_blindrotate) over the same public launchers, and the answer is one line: the tag, then every
// instantiation launched, in order, " | " between them, or the launcher's refusal.  fx stands for fx_usable of a certified key: the
// Float64 pipe wherever exact_impl admits it and the kernel exists for the shape
struct Reach {
    char tag[64] = "-", scheme[16] = "CGGI";
    int N = 256, k = 1, W = 32, l = 3, logB = 9, blk_len = 1, rows = 1, count = 5;
    int variant = 0, wide = 0, blkg = 0, split = 0, ccs_pipe = -1, exact = 0, exact_wide = 1, exact_kany = 0, exact_impl = -1;
};
bool reach_parse(char *line, Reach &q) {
    const struct { const char *key; int Reach::*m; } ints[] = {
        {"N", &Reach::N}, {"k", &Reach::k}, {"W", &Reach::W}, {"l", &Reach::l}, {"logB", &Reach::logB}, {"blk_len", &Reach::blk_len}, {"rows", &Reach::rows},
        {"count", &Reach::count}, {"variant", &Reach::variant}, {"wide", &Reach::wide}, {"blkg", &Reach::blkg}, {"split", &Reach::split}, {"ccs_pipe", &Reach::ccs_pipe},
        {"exact", &Reach::exact}, {"exact_wide", &Reach::exact_wide}, {"exact_kany", &Reach::exact_kany}, {"exact_impl", &Reach::exact_impl}};
    for (char *tok = strtok(line, " \t\n"); tok; tok = strtok(nullptr, " \t\n")) {
        char *eq = strchr(tok, '=');
        if (!eq) return false;
        *eq = 0;
        bool known = false;
        if (!strcmp(tok, "tag")) { snprintf(q.tag, sizeof q.tag, "%s", eq + 1); known = true; }
        if (!strcmp(tok, "scheme")) { snprintf(q.scheme, sizeof q.scheme, "%s", eq + 1); known = true; }
        for (const auto &f : ints) if (!strcmp(tok, f.key)) { q.*f.m = atoi(eq + 1); known = true; }
        if (!known) return false;
    }
    return true;
}
hipError_t reach_one(const Reach &q) {
    const char *const schemes[] = {"CGGI", "LMSS", "CCS", "KMS", "KMS_BLOCK"};
    int sc = -1;
    for (int i = 0; i < 5; i++) if (!strcmp(q.scheme, schemes[i])) sc = i;
    if (sc < 0 || q.N < 32 || q.N > 4096 || (q.N & (q.N - 1)) || q.count < 1 || q.rows < 1) return hipErrorInvalidValue;
    const bool kms = sc == KMS || sc == KMS_BLOCK, block = sc == LMSS || sc == KMS_BLOCK;
    const Shape sh{q.tag, (Scheme)sc, q.N, q.k, q.W, q.l, q.logB, block ? q.blk_len : 1, kms ? q.rows : 1};
    const int lm = logm(sh), logN = lm + 1;
    const size_t B = (size_t)q.count, nrot = B * (size_t)sh.rows;
    cplx *const scratch = reinterpret_cast<cplx *>(16);
    uint64_t *const xscratch = reinterpret_cast<uint64_t *>(16);
    if (!q.exact) {
        if (sc == CCS) { CcsArgs c{}; c.k = sh.k; c.l = sh.l; c.logB = sh.logB; return launch_ccs(lm, sh.W, c, q.ccs_pipe, B, nullptr); }
        RotArgs a = rot_args(sh, nrot, Opts{q.variant, q.wide, q.blkg, q.split});
        a.blk_accum = block;
        if (kms) {
            const hipError_t e = launch_blindrotate_k1(lm, sh.W, a, nrot, nullptr);
            if (e != hipSuccess) return e;
            Phase2Args p2{};
            return launch_kms_phase2(lm, sh.W, p2, B, nullptr);
        }
        if (sh.k > 3) return launch_blindrotate_kany(lm, sh.W, sh.k, a, scratch, nrot, nullptr);
        if (sh.k > 1) return launch_blindrotate_kr(lm, sh.W, sh.k, a, nrot, nullptr);
        return launch_blindrotate_k1(lm, sh.W, a, nrot, nullptr);
    }
    const bool fx = q.exact_impl != 0 && fx_supported(lm, sh.W, sh.l);
    if (sc == CCS) { ExactCcsHostArgs c{}; c.k = sh.k; c.l = sh.l; c.logB = sh.logB; return launch_exact_ccs(logN, nullptr, c, B, nullptr); }
    if (kms) {
        ExactKmsArgs x{};
        x.k = sh.k; x.l_gsw = sh.l; x.logB_gsw = sh.logB; x.rtot = sh.rows; x.blk_len = sh.blk_len; x.wide = q.exact_wide;
        if (sc == KMS && fx) {
            FxRotArgs f{};
            f.l = sh.l; f.logB = sh.logB; f.split = q.split; f.map_mode = 1; f.rows_per_gate = sh.rows; f.ngates = B; f.init_mode = 1;
            const hipError_t e = launch_fx_blindrotate(lm, sh.W, f, nrot, nullptr);
            if (e != hipSuccess) return e;
            x.phase2_only = 1;
        }
        return launch_exact_kms(logN, nullptr, x, B, nullptr);
    }
    if (sh.k > 3 || q.exact_kany == 1) return launch_exact_blindrotate_kany(logN, nullptr, nullptr, nullptr, nullptr, 0, 1, sh.blk_len * 3, sh.k, sh.l, sh.logB, sh.blk_len, nullptr, xscratch, B, nullptr);
    if (sh.k > 1 || (block && sh.blk_len != 3)) return launch_exact_blindrotate_kr(logN, nullptr, nullptr, nullptr, nullptr, 0, 1, sh.blk_len * 3, sh.k, sh.l, sh.logB, sh.blk_len, nullptr, B, nullptr);
    if (sc == CGGI && fx) {
        FxRotArgs f{};
        f.l = sh.l; f.logB = sh.logB; f.split = q.split; f.map_mode = 1; f.rows_per_gate = 1; f.ngates = B;
        return launch_fx_blindrotate(lm, sh.W, f, B, nullptr);
    }
    return launch_exact_blindrotate(logN, nullptr, nullptr, nullptr, nullptr, 0, 1, sh.blk_len * 3, sh.l, sh.logB, sh.blk_len, nullptr, B, nullptr);
}
int reach_all() {
    g_reach = true;
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        Reach q;
        if (line[0] == '\n' || line[0] == '#') continue;
        if (!reach_parse(line, q)) { fprintf(stderr, "reach: a word that is no known key=value\n"); return 2; }
        g_reached.clear();
        const hipError_t e = reach_one(q);
        if (e != hipSuccess) g_reached += std::string(g_reached.empty() ? "" : " | ") + (e == hipErrorInvalidValue ? "-> invalid value" : "-> error");
        printf("%s: %s\n", q.tag, g_reached.c_str());
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "kernels")) return print_kernels();
    if (argc > 1 && !strcmp(argv[1], "reach")) return reach_all();
    g_print = argc > 1 && !strcmp(argv[1], "log");
    for (const Shape &sh : SHAPES) {
        for (const size_t count : COUNTS) {
            if (sh.scheme == CCS) {
                for (const int pipe : {-1, 0, 1}) ccs_calls(sh, count, pipe);
                continue;
            }
            // every value of a switch with the others at 0, and the companions test_gpu_switches.py gives it
            for (const int variant : {0, 21, 22}) for (const int wide : {0, 1, 2}) for (const int blkg : {0, 1, 2, 4}) f64_calls(sh, count, Opts{variant, wide, blkg, 0});
            for (const int split : {-1, 1, 3, 7, 100}) {
                if (split > 0 && split < 100 && count > 1025) continue;                       // (a log of reasonable length)
                for (const int wide : {0, 1, 2}) for (const int blkg : {0, 1}) f64_calls(sh, count, Opts{0, wide, blkg, split});
            }
            // both exact implementations: the Float64 pipe (CGGI at RLWE length 1, phase 1 of KMS) and the integer transforms (KMS, KMS_block)
            if ((sh.scheme == CGGI && sh.k == 1) || sh.scheme == KMS)
                for (const int split : {0, -1, 1, 3, 7, 100}) if (!(split > 0 && split < 100 && count > 1025)) fx_calls(sh, count, split);
            if ((sh.scheme == KMS || sh.scheme == KMS_BLOCK) && count % (size_t)sh.rows == 0) {
                for (const int wide : {0, 1}) exact_kms_calls(sh, count / (size_t)sh.rows, wide, 0);
                exact_kms_calls(sh, count / (size_t)sh.rows, 1, 1);
            }
        }
    }
    printf("%zu lines, digest %016llx\n", g_lines, (unsigned long long)g_hash);
    return 0;
}
