// C ABI of the engine (include/mktfhe.h): per-device context, key upload + on-device pre-transform,
// batched hot-path entry points.  Host code; kernels live in kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string.h>   // explicit_bzero
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "device_api.h"
#include "ks_mfma.h"
#include "device_mem.h"
#include "fft_device.h"
#include "host_internal.h"
#include "rng_chacha.h"
#include "../../include/mktfhe_ring_share.h"

using mktd::cplx;
using mkt::DevBuf;

namespace {
thread_local std::string g_create_error;

struct TimedSpan { int cls; hipEvent_t a, b; };

int env_int(const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; }

// Kernel-selection switches of one context (A/B runs and the parity tests that force every kernel variant).  The
// environment seeds them ONCE, at mkt_ctx_create; afterwards only mkt_set_option changes them -- the call path never
// reads the environment.
struct Tune {
    int rot_variant, rot_stagger, rot_split, rot_wide, rot_blkg, ccs_stagger, ccs_pipe, rot_map, exact_wide, exact_kany, fx_polymul_force, exact_impl;
};
// One row per switch: mkt_set_option name, the environment variable that seeds it (nullptr: none), the member, its default, the values it
// admits (none listed: any), and whether a change drops the workspace.
struct Switch { const char *name, *env; int Tune::*member; int dflt; std::vector<int> allowed; bool resets_workspace; };
const Switch SWITCHES[] = {
    {"rot_variant", "MKT_ROT_VARIANT", &Tune::rot_variant, 0, {0, 21, 22}, false},   // a selector with a fixed set of values refuses the others (a call would otherwise fail late, inside a gate, or run nothing)
    {"rot_stagger", "MKT_ROT_STAGGER", &Tune::rot_stagger, 16, {}, false},   // tools/stagger.sh: 16.99 -> 15.63 ms at KMS k=2 N=1024 on one device, neutral elsewhere
    {"rot_split", "MKT_ROT_SPLIT", &Tune::rot_split, 0, {}, false},
    {"rot_wide", "MKT_ROT_WIDE", &Tune::rot_wide, 0, {}, false},       // latency variant: 0 automatic, 1 never, 2 always where supported
    {"rot_blkg", "MKT_ROT_BLKG", &Tune::rot_blkg, 0, {}, false},       // block schemes: rotations per workgroup, 0 automatic
    {"ccs_stagger", "MKT_CCS_STAGGER", &Tune::ccs_stagger, 0, {}, false},
    {"ccs_pipe", "MKT_CCS_PIPE", &Tune::ccs_pipe, -1, {}, false},      // two-group CCS kernel: -1 automatic (below one chip-fill), 0 never, 1 always
    // workgroup id -> (ciphertext, slot) mapping of the k = 1 rotation kernels (kernel_common.h rot_decode): 1 = the RLEV rows of one
    // (ciphertext, party) on one XCD at one time -- 25 % less fabric traffic at KMS k = 2 (FETCH_SIZE 15.3 -> 11.4 GB per launch,
    // L2 misses -27 %), time -0.3 ... -2.5 % (profiles/r04j_bench_kms2_n1024_map{0,1}_pmc.txt)
    {"rot_map", "MKT_ROT_MAP", &Tune::rot_map, 1, {0, 1}, false},
    {"exact_wide", "MKT_EXACT_WIDE", &Tune::exact_wide, 1, {}, false},   // EXACT (integer NTT) KMS phase 1 at l_gsw = 2 and KMS_block phase 1: 1 = the paired-transform kernel / one set of digit transforms per block (default), 0 = the one-at-a-time kernel (reference loop order; tests force both)
    {"exact_kany", "MKT_EXACT_KANY", &Tune::exact_kany, 0, {}, true},    // EXACT CGGI / LMSS: 1 = the run-time-RLWE-length kernel (sums in memory) also where the register kernels serve (k <= 3); tests.  The workspace gains / loses the kernel's scratch at the next call
    {"fx_polymul_force", nullptr, &Tune::fx_polymul_force, 0, {}, false},   // diagnostic: 1 = mkt_exact_polymul_batch under exact_impl = 1 runs the Float64 kernel even where fx_polymul_bound does not certify the operands
    // EXACT blind rotation of CGGI (RLWE length 1) and KMS phase 1: 0 = integer NTT over two 30-bit primes (ntt_exact.hip), 1 / -1 = the Float64 pipe (ahead at every measured shape: profiles/r06_fx_shapes.txt)
    // (fx_exact.hip: FMA transforms over 16-bit key limbs) wherever its error bound certifies the loaded keys (fx_usable), the integer NTT elsewhere
    {"exact_impl", "MKT_EXACT_IMPL", &Tune::exact_impl, -1, {}, false},
};
struct DevGuard {   // make the context's device current for the duration of a call
    int prev = -1; bool ok = true;
    explicit DevGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) ok = hipSetDevice(dev) == hipSuccess; }
    ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
Tune tune_from_env() { Tune t; for (const Switch &w : SWITCHES) t.*w.member = w.env ? env_int(w.env, w.dflt) : w.dflt; return t; }
}  // namespace

thread_local const char *mktd::last_rot_kernel = "";
thread_local int mktd::last_rot_static_l = 0, mktd::last_rot_static_logB = 0;

// launcher-level switches (grid shapes of the transform and key-switch kernels): process-wide, read from the environment
// on first use only (device_api.h)
const mktd::LaunchTuning &mktd::launch_tuning() {
    static const LaunchTuning t = [] {
        LaunchTuning q{};
        q.fft_grid = env_int("MKT_FFT_GRID", 0); q.fft_nb = env_int("MKT_FFT_NB", 1); q.fft_igrid = env_int("MKT_FFT_IGRID", 0);
        q.ks_g = env_int("MKT_KS_G", 32); q.ks_blocks = env_int("MKT_KS_BLOCKS", 0); q.ks_waves = env_int("MKT_KS_WAVES", 0); q.ks_pair = env_int("MKT_KS_PAIR", -1); q.ks_mfma = env_int("MKT_KS_MFMA", -1); q.ntt_grid = env_int("MKT_NTT_GRID", 0);
        return q;
    }();
    return t;
}

// The resident tables of a key set, in the order they are allocated and replicated.  describe_key_set states each one ONCE;
// allocation, replication, release and the per-party base pointers all read that description.
enum KeyTable { T_TW, T_MONOMIAL, T_BRK, T_KSK, T_PUB, T_CRS, T_RLK_D, T_RLK_F, T_SLOT_PARTY, T_SLOT_ROW, T_FX_TAB, T_FX_BRK, T_FX_STAT, T_NTT, T_KSK_PLANES, T_COUNT };
struct ResidentTable {
    void **slot = nullptr; size_t elems = 0, esize = 0;   // the KeySet member that holds the device pointer; elements per party (or in the whole table): the party stride; bytes per element
    bool per_party = false, present = false, cloned = false;   // [nparty][elems], else one per key set; this scheme, arithmetic and shape have the table; mkt_internal_clone_keys copies it (false: every context builds its own at mkt_ctx_create)
    size_t bytes(int nparty) const { return (per_party ? (size_t)nparty : 1) * elems * esize; }
};
// The evaluation keys and tables of one scheme on one device: immutable once a second context shares them
// (mkt_ctx_fork), freed when the last context that holds them is destroyed.  This is the reference's scheme object
// proper -- read-only during evaluation, shared by concurrent callers (bootstrapping.jl:38-45 allocates all scratch per
// call) -- while mkt_ctx adds what a caller must not share: stream, workspace, timing spans, error string.
struct KeySet {
    int device = 0;
    mkt::Twiddles tw;
    cplx *d_tw = nullptr;        // psi | psiinv | roots | rootsinv, M each
    cplx *d_monomial = nullptr;  // [2N][M]
    cplx *d_brk = nullptr;
    uint32_t *d_ksk = nullptr; mkt::KskLayout ksk;   // host_internal.h: rows, the callers' pitch, the resident pitch
    int8_t *d_ksk_planes = nullptr;   // the same key as signed byte planes for the matrix-core key switch (ks_mfma.h), where the shape has the kernel and the memory was there; else null
    cplx *d_rlk_d = nullptr, *d_rlk_f = nullptr, *d_pub = nullptr, *d_crs = nullptr;
    mkt::LoadedKeys loaded;      // which pieces of which party are resident (host_internal.h)
    // rotation slots (KMS phase 1: party-major rows)
    int rtot = 1;
    int *d_slot_party = nullptr, *d_slot_row = nullptr;
    uint64_t *d_ntt = nullptr;   // MKT_ARITH_EXACT: psi_rev (negated) | N^-1, N^-1 w | N^-1 2^32, N^-1 2^32 w, with Shoup companions
    // MKT_ARITH_EXACT on the Float64 pipe (fx_exact.hip), where the shape has the kernel: the engine's own tables and the bootstrapping key as limb transforms
    cplx *d_fx_tab = nullptr;    // fx_om | fx_tw | fx_nat, M each
    cplx *d_fx_brk = nullptr;    // [party][n][2l][2][W/16][M], scaled by 1 / M
    unsigned long long *d_fx_stat = nullptr;   // largest |key transform value|^2 over the loaded keys (bit pattern)
    double fx_kmax = 0.0;        // sqrt of [0], read back after every key load
    // packed outputs (mktfhe_pack.h): every party's packing key, outside the table description below (no multi-device replica).  F64REF:
    // [party][n][l][1 + kr][M] transforms in the slot-major point order; EXACT: [party][1 + kr][n l][N] ring words, polynomial-major -- the
    // rows one exact-product launch reads in a run.  The first load fixes the gadget
    DevBuf d_pack; int pack_l = 0, pack_logB = 0; size_t pack_party_bytes = 0;
    std::vector<uint8_t> pack_loaded;   // [party]
    ResidentTable tab[T_COUNT];  // describe_key_set
    DevBuf own[T_COUNT];         // the owner of each table's memory (device_mem.h: guarded in guard mode like every other buffer); *tab[t].slot is own[t].p under the table's type
    size_t stride(KeyTable t) const { return tab[t].elems; }   // elements from one party's rows to the next
    template <class T> T *party(KeyTable t, int party) const { return static_cast<T *>(*tab[t].slot) + (size_t)party * tab[t].elems; }   // base of one party's rows
};
// a key set lets go of its tables and owners under its own device, whoever drops the last reference
static std::shared_ptr<KeySet> new_key_set() { return std::shared_ptr<KeySet>(new KeySet, [](KeySet *k) { DevGuard g(k->device); delete k; }); }

// The device memory a context keeps between calls, every buffer with its owner (device_mem.h), grouped as it grows.  mkt_ctx_destroy drops it whole
struct MKT_HIDDEN Workspace {
    // the rotation group, for `gates` gates, sized per gate by the route (ensure_workspace): the linear combinations, the accumulators, what the route's kernels are handed
    size_t gates = 0;
    DevBuf lin, acc, lev, scratch;
    DevBuf fxacc;                // fx_exact.hip, KMS: the phase-1 rows as ring words [gates][rtot][2][N] before they become split residue tables
    DevBuf ksd;                  // key switch: prepared digit words + partial sums per slab (grows with the largest batch seen)
    // lookup-table bootstrap with more than one output per input: (src | coef) rows of a chunk's key switch, 8 bytes per output row (first such call): the src half, then the coef half
    DevBuf at;
    uint32_t *at_src() const { return at.as<uint32_t>(); }
    uint32_t *at_coef() const { return at.as<uint32_t>() + at.cap / 8; }   // at the row count the table was allocated for
    // mkt_pack_batch: its own group for `packs` packs at a time -- the lifted columns; F64REF the product kernel's slabs; EXACT the digits and products of one chunk of columns
    size_t packs = 0;
    DevBuf pack_cols, pack_slabs, pack_dig, pack_prod;
    // mkt_exact_polymul_batch: [0] max|a_i| over the batch, [1] largest |limb transform of b|^2, [2] largest |q - round(q)| of the Float64 kernel (bit patterns)
    DevBuf pm_stat;
    unsigned long long *pm() const { return pm_stat.as<unsigned long long>(); }
};

struct mkt_ctx {
    mkt_params p;
    mkt::Shape sh;
    int device = 0;
    int logM = 0, logN = 0, M = 0;
    int dev_order = MKT_DEVORDER;   // device point order of this context's resident tables (fft_device.h dev_pos)
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;   // a fork's own non-blocking stream (destroyed with the context); `stream` may be re-pointed by mkt_set_stream
    hipEvent_t moved = nullptr;         // mkt_set_stream: recorded on the stream the context leaves, waited for by the one it moves to (no timing; destroyed with the context)
    std::string err;
    std::shared_ptr<KeySet> ks;  // shared with the contexts forked from this one
    bool exact = false;          // MKT_ARITH_EXACT (integer NTT, two 30-bit primes)
    int split = 1;               // EXACT on the 64-bit ring: every resident 64-bit table is kept as (low, high) residue polynomials -> 2 per logical polynomial
    Workspace ws;
    // timing
    bool timing = false;
    std::vector<TimedSpan> spans;
    Tune tune{};
    const char *last_rot_kernel = "";   // name of the blind-rotation kernel the last call launched (mkt_last_kernel_name)
    int ks_mfma_last = 0;               // 1 if the last key switch ran the matrix-core kernel (mkt_get_metric "ks_mfma_last")
    mktd::KsReport ks_last{};           // the plan of the last key switch (mkt_get_metric "ks_last_kernel" / "_g" / "_waves" / "_slabs"; kernel 0: none yet)
    int rot_static_l = 0, rot_static_logB = 0;   // ... and its compile-time gadget, 0 = taken at run time (mkt_get_metric "rot_static_l" / "rot_static_logB")
    // mkt_exact_polymul_batch: per-call scratch and what the last call measured (per context: forks run the product concurrently)
    double pm_amax = 0.0;               // max|a_i| of the last call
    double pm_bound = -1.0;             // fx_polymul_bound of the last call (-1: not evaluated -- exact_impl != 1 or no Float64 tables)
    double fx_last_resid = 0.0;         // largest |q - round(q)| of the last call that ran the Float64 kernel (diagnostic, not a certificate)

    const cplx *fx_om() const { return ks->d_fx_tab; }
    const cplx *fx_tw() const { return ks->d_fx_tab + M; }
    const cplx *fx_nat() const { return ks->d_fx_tab + 2 * (size_t)M; }
    mktd::TwPtrs twp() const { return mktd::TwPtrs{ks->d_tw, ks->d_tw + M, ks->d_tw + 2 * (size_t)M, ks->d_tw + 3 * (size_t)M}; }
    bool keys_shared() const { return ks.use_count() > 1; }
};

namespace {

int fail(mkt_ctx *c, int code, const std::string &msg) { if (c) c->err = msg; else g_create_error = msg; return code; }
int hipfail(mkt_ctx *c, hipError_t e, const char *what) {
    return fail(c, MKT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIPCHK(c, call) do { hipError_t _e = (call); if (_e != hipSuccess) return hipfail((c), _e, #call); } while (0)

int keys_writable(mkt_ctx *c) { return c->keys_shared() ? fail(c, MKT_ERR_STATE, "the key set is shared with forked contexts and immutable") : MKT_OK; }

struct Timer {
    mkt_ctx *c; int cls; hipEvent_t a = nullptr, b = nullptr;
    Timer(mkt_ctx *c_, int cls_) : c(c_), cls(cls_) {
        if (c->timing && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) (void)hipEventRecord(a, c->stream);
        else a = b = nullptr;
    }
    ~Timer() {
        if (cls == 1) { c->last_rot_kernel = mktd::last_rot_kernel; c->rot_static_l = mktd::last_rot_static_l; c->rot_static_logB = mktd::last_rot_static_logB; }   // the blind-rotation launcher noted which kernel it picked
        if (a && b) { (void)hipEventRecord(b, c->stream); c->spans.push_back(TimedSpan{cls, a, b}); }
    }
};

void clear_spans(mkt_ctx *c) {
    for (auto &s : c->spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
    c->spans.clear();
}

size_t poly_bytes(const mkt_ctx *c) { return (size_t)c->p.N * c->sh.word; }

hipError_t fx_after_key_load(mkt_ctx *c);
hipError_t install_brk(mkt_ctx *c, int party, const void *src);
bool fx_usable(const mkt_ctx *c);
mktd::FxRotArgs fx_rot_args(mkt_ctx *c, const uint32_t *lwe, int stride, int pre);
// `npolys` coefficient-form polynomials on the device (src) into the resident form of this context's tables at dst.  small: coefficients far below 2^32 in magnitude
// (monomials): never split; fx_dst: also as limb transforms (fx_exact.hip), their largest magnitude gathered in d_fx_stat (fx_after_key_load reads it once the stream is drained)
hipError_t to_resident(mkt_ctx *c, const void *src, size_t npolys, cplx *dst, bool small, cplx *fx_dst) {
    hipError_t e = !c->exact ? mktd::launch_transform_fwd(c->logM, c->p.W, c->twp(), src, dst, npolys, c->dev_order, c->stream)
                   : (c->split == 2 && !small) ? mktd::launch_ntt_fwd_split(c->logN, c->ks->d_ntt, src, reinterpret_cast<uint64_t *>(dst), npolys, c->stream)   // 2 residue polynomials per input
                   : mktd::launch_ntt_fwd(c->logN, c->p.W, c->ks->d_ntt, src, reinterpret_cast<uint64_t *>(dst), npolys, 1, c->stream);   // N residues = the bytes of M complex
    if (e == hipSuccess && fx_dst) e = mktd::launch_fx_key_fwd(c->logM, c->p.W, c->fx_om(), c->fx_tw(), src, fx_dst, npolys, c->ks->d_fx_stat, c->stream);
    return e;
}
// transform `npolys` coefficient-form polynomials (host) into TransPolys at `dst` (device); returns with the stream drained.  brk_party >= 0: they
// are that party's bootstrapping key, which in coefficient form goes through install_brk
int upload_polys(mkt_ctx *c, const void *host, size_t npolys, cplx *dst, int fmt, bool small = false, int brk_party = -1) {
    if (c->exact && fmt != MKT_FMT_INT_COEFF) return fail(c, MKT_ERR_UNSUPPORTED, "an MKT_ARITH_EXACT context takes keys in integer form (MKT_FMT_INT_COEFF)");
    if (fmt != MKT_FMT_F64_FFT && fmt != MKT_FMT_INT_COEFF) return fail(c, MKT_ERR_ARG, "unknown key format");
    const bool fft = fmt == MKT_FMT_F64_FFT;   // the reference's Trans* values: copy, then natural -> device point order
    const size_t nb = npolys * (fft ? (size_t)c->M * sizeof(cplx) : poly_bytes(c));
    DevBuf tmp;
    HIPCHK(c, tmp.alloc(nb));
    hipError_t e = hipMemcpyAsync(tmp.p, host, nb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = fft ? mktd::launch_reorder(c->logM, static_cast<cplx *>(tmp.p), dst, npolys, 1, c->dev_order, c->stream)
                                 : brk_party >= 0 ? install_brk(c, brk_party, tmp.p) : to_resident(c, tmp.p, npolys, dst, small, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hipfail(c, e, fft ? "key upload" : "key pre-transform");
    return MKT_OK;
}

int build_monomial(mkt_ctx *c) {   // scheme.jl:121-146
    const int N = c->p.N;
    const size_t wb = c->sh.word;
    std::vector<unsigned char> host((size_t)2 * N * N * wb, 0);
    auto set = [&](int e, int i, uint64_t v) {
        unsigned char *p = host.data() + ((size_t)(e - 1) * N + i) * wb;
        if (wb == 8) std::memcpy(p, &v, 8); else { uint32_t w = (uint32_t)v; std::memcpy(p, &w, 4); }
    };
    const uint64_t m1 = ~0ull;
    for (int e = 1; e < N; e++) { set(e, 0, m1); set(e, e, 1); }            // -1 + X^e
    set(N, 0, m1 - 1);                                                       // -2
    for (int e = N + 1; e < 2 * N; e++) { set(e, 0, m1); set(e, e - N, m1); } // -1 - X^(e-N)
    int r = upload_polys(c, host.data(), (size_t)2 * N, c->ks->d_monomial, MKT_FMT_INT_COEFF, true);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(c->ks->d_monomial + (size_t)(2 * N - 1) * c->M, 0, (size_t)c->M * sizeof(cplx), c->stream));  // entry 2N = 0
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MKT_OK;
}

// fft_device.h (MKT_FFT_SPECIAL): the butterflies of the first two forward / last two inverse stages are written for
// Psi[1] = (eps, -1), Psi[2] = (c, -c), Psi[3] = (-c, -c) -- the shape of the reference's tables (fft.jl:31-37 at any size)
static bool twiddle_shape_ok(const std::vector<double> &psi, int M) {
    if (M < 4) return false;
    return psi[3] == -1.0 && psi[5] == -psi[4] && psi[4] > 0.0 && psi[7] == psi[6] && psi[6] == -psi[4];
}
int upload_twiddles(mkt_ctx *c) {
    if (!twiddle_shape_ok(c->ks->tw.psi, c->M)) return fail(c, MKT_ERR_ARG, "twiddle table Psi does not have the reference's shape (Psi[1] = (eps,-1), Psi[2] = (c,-c), Psi[3] = (-c,-c))");
    const size_t tb = (size_t)c->M * sizeof(cplx);
    HIPCHK(c, hipMemcpy(c->ks->d_tw, c->ks->tw.psi.data(), tb, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->ks->d_tw + c->M, c->ks->tw.psiinv.data(), tb, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->ks->d_tw + 2 * (size_t)c->M, c->ks->tw.roots.data(), tb, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->ks->d_tw + 3 * (size_t)c->M, c->ks->tw.rootsinv.data(), tb, hipMemcpyHostToDevice));
    return MKT_OK;
}

// Which blind-rotation kernel family serves the context now: do_blindrotate launches by it, ensure_workspace sizes the scratch it hands over by it.
enum class Route { F64_K1, F64_KR, F64_KANY, F64_KMS, F64_CCS, EXACT_CCS, EXACT_KMS, EXACT_KANY, EXACT_KR, EXACT_FX, EXACT_K1 };   // what each is: do_blindrotate
Route rot_route(const mkt_ctx *c) {
    const mkt_params &p = c->p;
    if (p.scheme == MKT_CCS) return c->exact ? Route::EXACT_CCS : Route::F64_CCS;
    if (c->exact) {
        if (mkt::is_kms(p.scheme)) return Route::EXACT_KMS;
        if (p.k > 3 || c->tune.exact_kany == 1) return Route::EXACT_KANY;
        if (p.k > 1 || (mkt::is_block(p.scheme) && p.blk_len != 3)) return Route::EXACT_KR;
        return p.scheme == MKT_CGGI && fx_usable(c) ? Route::EXACT_FX : Route::EXACT_K1;
    }
    if (mkt::is_kms(p.scheme)) return Route::F64_KMS;
    return p.k > 3 ? Route::F64_KANY : p.k > 1 ? Route::F64_KR : Route::F64_K1;
}

int ensure_workspace(mkt_ctx *c, size_t gates) {
    Workspace &w = c->ws;
    if (gates <= w.gates) return MKT_OK;   // (reserve_group asks the same: the route is not looked up for a call that fits)
    const size_t tpoly = (size_t)c->M * sizeof(cplx);   // one transformed polynomial
    size_t lev = 0, scratch = 0, fxacc = 0;              // bytes per gate of what the route's kernels are handed
    switch (rot_route(c)) {
    case Route::F64_KMS: case Route::EXACT_KMS:
        lev = (size_t)c->ks->rtot * 2 * tpoly * c->split;
        scratch = (size_t)2 * (c->p.k + 1) * tpoly * c->split;
        if (c->ks->d_fx_brk) fxacc = (size_t)c->ks->rtot * 2 * poly_bytes(c);   // whenever the key set holds limb transforms: fx_phase1 is a per-call choice
        break;
    case Route::F64_CCS: case Route::EXACT_CCS:
        lev = 3 * poly_bytes(c);    // v scratch (ring words): parked v + two hand-off slots
        scratch = (size_t)(c->p.k + 1) * tpoly;
        break;
    case Route::F64_KANY: case Route::EXACT_KANY:   // CGGI / LMSS beyond RLWE length 3: tacc and tacc2 of blindrotate_kany_kernel / exact_blindrotate_kany_kernel (same byte count)
        scratch = (size_t)2 * (c->p.k + 1) * tpoly;
        break;
    default: break;                                 // the register kernels keep their sums to themselves
    }
    DevBuf *const group[] = {&w.lin, &w.acc, &w.lev, &w.scratch, &w.fxacc};
    const size_t need[] = {gates * c->sh.lwe_len * 4, gates * (1 + c->sh.kacc) * poly_bytes(c), gates * lev, gates * scratch, gates * fxacc};
    HIPCHK(c, mkt::reserve_group(w.gates, gates, group, need));
    return MKT_OK;
}

constexpr size_t CHUNK_GATES = 8192;   // bounds the workspace (KMS N=2048, k=2: ~1.9 GiB)

int check_ready(mkt_ctx *c, bool need_brk, bool need_ksk) {
    using L = mkt::LoadedKeys;
    const int s = c->p.scheme;
    // what every party must have resident, in the order it is refused: the side of the call that asks, the schemes it holds for, the pieces
    const struct { bool asked, applies; unsigned pieces; int code; const char *msg; } per_party[] = {
        {need_brk, true,           L::bit(mkt::K_BRK),                      MKT_ERR_STATE, "bootstrapping key not loaded"},
        {need_ksk, true,           L::bit(mkt::K_KSK),                      MKT_ERR_STATE, "key-switching key not loaded"},
        {need_brk, s == MKT_CCS,   L::bit(mkt::K_PUB),                      MKT_ERR_STATE, "public key not loaded"},
        {need_brk, mkt::is_kms(s), L::bit(mkt::K_RLK) | L::bit(mkt::K_PUB), MKT_ERR_STATE, "rlk / public key not loaded"}};
    for (int i = 0; i < c->sh.nparty; i++) for (const auto &r : per_party) if (r.asked && r.applies && !c->ks->loaded.has_all(r.pieces, i)) return fail(c, r.code, r.msg);
    if (need_brk && mkt::is_mk(s) && !c->ks->loaded.has(mkt::K_CRS, -1)) return fail(c, MKT_ERR_STATE, "crs not loaded");
    return MKT_OK;
}

mktd::RotArgs rot_args(mkt_ctx *c, const uint32_t *lwe, int stride, int pre) {
    const mkt_params &p = c->p;
    mktd::RotArgs a{};
    a.tw = c->twp(); a.brk = c->ks->d_brk; a.brk_party_stride = c->ks->stride(T_BRK); a.monomial = c->ks->d_monomial;
    a.lwe = lwe; a.lwe_stride = stride; a.pre_switched = pre; a.n = p.n; a.logN = c->logN;
    a.l = p.l_gsw; a.logB = p.logB_gsw;
    a.blk_len = mkt::is_block(p.scheme) ? p.blk_len : 1;
    a.blk_accum = mkt::is_block(p.scheme) ? 1 : 0;
    a.rows_per_gate = c->ks->rtot; a.slot_party = c->ks->d_slot_party; a.slot_row = c->ks->d_slot_row;
    a.logB_lev = p.logB_lev; a.dev_order = c->dev_order;
    a.variant = c->tune.rot_variant; a.stagger = c->tune.rot_stagger; a.split = (unsigned)c->tune.rot_split;
    a.wide = c->tune.rot_wide; a.blk_group = c->tune.rot_blkg; a.map_mode = c->tune.rot_map;
    return a;
}

// EXACT KMS (64-bit ring, split tables; ntt_exact.hip): everything the context and its key set fix; the caller adds levkey, the phase flags and, for phase 2, lin_for_tv / acc / scratch
mktd::ExactKmsArgs exact_kms_args(mkt_ctx *c, const uint32_t *lwe, int stride, int pre) {
    const mkt_params &p = c->p;
    mktd::ExactKmsArgs q{};
    q.brk = reinterpret_cast<const uint64_t *>(c->ks->d_brk); q.brk_party_stride = c->ks->stride(T_BRK) * 2 /* in 8-byte residue pairs */; q.mono = reinterpret_cast<const uint64_t *>(c->ks->d_monomial);
    q.lwe = lwe; q.lwe_stride = stride; q.pre_switched = pre; q.n = p.n; q.k = p.k; q.l_gsw = p.l_gsw; q.logB_gsw = p.logB_gsw;
    q.l_lev = p.l_lev; q.logB_lev = p.logB_lev; q.l_uni = p.l_uni; q.logB_uni = p.logB_uni; q.rtot = c->ks->rtot; q.lwe_len = c->sh.lwe_len; q.blk_len = p.scheme == MKT_KMS_BLOCK ? p.blk_len : 1;
    q.slot_party = c->ks->d_slot_party; q.slot_row = c->ks->d_slot_row;
    q.rlk_d = reinterpret_cast<const uint64_t *>(c->ks->d_rlk_d); q.rlk_f = reinterpret_cast<const uint64_t *>(c->ks->d_rlk_f);
    q.pub_b = reinterpret_cast<const uint64_t *>(c->ks->d_pub); q.crs = reinterpret_cast<const uint64_t *>(c->ks->d_crs);
    q.wide = c->tune.exact_wide;
    return q;
}
// EXACT KMS phase 1 of `gates` gates on the Float64 pipe (a per-call choice: fx_usable; ensure_workspace holds ws.fxacc whenever the key set has the limb transforms): rows as ring words in ws.fxacc, then as split residue tables at levkey for the integer phase 2
int fx_phase1(mkt_ctx *c, const uint32_t *lwe, int stride, int pre, size_t gates, uint64_t *levkey) {
    mktd::FxRotArgs f = fx_rot_args(c, lwe, stride, pre);
    f.init_mode = 1; f.acc_io = c->ws.fxacc.p; f.ngates = gates;
    const size_t nrot = gates * (size_t)c->ks->rtot;
    HIPCHK(c, mktd::launch_fx_blindrotate(c->logM, c->p.W, f, nrot, c->stream));
    HIPCHK(c, mktd::launch_ntt_fwd_split(c->logN, c->ks->d_ntt, c->ws.fxacc.p, levkey, nrot * 2, c->stream));
    return MKT_OK;
}

// blind rotation of `B` accumulators resident at `acc` ([B][1+k][N]); atilde source described by (lwe, stride, pre); the route's kernels are handed ws.lev and ws.scratch
int do_blindrotate(mkt_ctx *c, const uint32_t *lwe, int stride, int pre, const uint32_t *lin_for_tv, void *acc, size_t B) {
    const mkt_params &p = c->p;
    cplx *const lev = c->ws.lev.as<cplx>(), *const scratch = c->ws.scratch.as<cplx>();
    const Route route = rot_route(c);
    if (route == Route::F64_KMS) {   // phase 1 (the rows of every party, as transforms), then phase 2
        {
            mktd::RotArgs a = rot_args(c, lwe, stride, pre);
            a.init_mode = 1; a.out_mode = 1; a.tout = lev; a.tout_natural = 0; a.ngates = B;
            Timer tm(c, 1);
            HIPCHK(c, mktd::launch_blindrotate_k1(c->logM, p.W, a, B * (size_t)c->ks->rtot, c->stream));
        }
        mktd::Phase2Args q{};
        q.tw = c->twp(); q.lin = lin_for_tv; q.lwe_stride = c->sh.lwe_len; q.logN = c->logN;
        q.k = p.k; q.l_lev = p.l_lev; q.logB_lev = p.logB_lev; q.l_uni = p.l_uni; q.logB_uni = p.logB_uni;
        q.levkey = lev; q.rtot = c->ks->rtot; q.rlk_d = c->ks->d_rlk_d; q.rlk_f = c->ks->d_rlk_f; q.pub_b = c->ks->d_pub; q.crs = c->ks->d_crs;
        q.acc = acc; q.scratch = scratch; q.dev_order = c->dev_order;
        Timer tm(c, 4);
        HIPCHK(c, mktd::launch_kms_phase2(c->logM, p.W, q, B, c->stream));
        return MKT_OK;
    }
    const uint64_t *xbrk = reinterpret_cast<const uint64_t *>(c->ks->d_brk), *xmono = reinterpret_cast<const uint64_t *>(c->ks->d_monomial);   // the tables as the integer kernels read them
    const int blk_len = mkt::is_block(p.scheme) ? p.blk_len : 1;
    Timer tm(c, 1);   // every other route is one span of class 1 around its launches
    switch (route) {
    case Route::EXACT_CCS: {   // hybrid products over Z_P (ntt_exact.hip)
        mktd::ExactCcsHostArgs q{};
        q.lwe = lwe; q.lwe_stride = stride; q.pre_switched = pre; q.n = p.n; q.k = p.k; q.l = p.l_uni; q.logB = p.logB_uni;
        q.brk = xbrk; q.brk_party_stride = c->ks->stride(T_BRK) * 2;
        q.pub_b = reinterpret_cast<const uint64_t *>(c->ks->d_pub); q.crs = reinterpret_cast<const uint64_t *>(c->ks->d_crs);
        q.mono = xmono; q.acc = (uint32_t *)acc; q.scratch = reinterpret_cast<uint64_t *>(scratch);
        HIPCHK(c, mktd::launch_exact_ccs(c->logN, c->ks->d_ntt, q, B, c->stream));
        return MKT_OK;
    }
    case Route::F64_CCS: {
        mktd::CcsArgs q{};
        q.tw = c->twp(); q.lwe = lwe; q.lwe_stride = stride; q.pre_switched = pre; q.n = p.n; q.logN = c->logN; q.k = p.k;
        q.l = p.l_uni; q.logB = p.logB_uni; q.brk = c->ks->d_brk; q.brk_party_stride = c->ks->stride(T_BRK); q.pub_b = c->ks->d_pub; q.crs = c->ks->d_crs;
        q.monomial = c->ks->d_monomial; q.acc = acc; q.scratch = scratch; q.vscratch = lev;
        q.stagger = c->tune.ccs_stagger; q.dev_order = c->dev_order;
        HIPCHK(c, mktd::launch_ccs(c->logM, p.W, q, c->tune.ccs_pipe, B, c->stream));   // one thread group per ciphertext or two: rot_plan.h plan_ccs
        return MKT_OK;
    }
    case Route::EXACT_KMS: {   // 64-bit ring, split tables: phase 1 and phase 2 with exact products (ntt_exact.hip)
        mktd::ExactKmsArgs q = exact_kms_args(c, lwe, stride, pre);
        q.levkey = reinterpret_cast<uint64_t *>(lev); q.lin_for_tv = lin_for_tv; q.acc = reinterpret_cast<uint64_t *>(acc); q.scratch = reinterpret_cast<uint64_t *>(scratch);
        if (p.scheme == MKT_KMS && fx_usable(c)) {
            if (int r = fx_phase1(c, lwe, stride, pre, B, q.levkey)) return r;
            q.phase2_only = 1;
        }
        const int fx_l = mktd::last_rot_static_l;   // (phase 1 ran on the Float64 pipe: the call is named after it, with its gadget)
        HIPCHK(c, mktd::launch_exact_kms(c->logN, c->ks->d_ntt, q, B, c->stream));
        if (q.phase2_only) mktd::note_rot_kernel("fx_blindrotate_kernel", fx_l, 0);
        return MKT_OK;
    }
    case Route::EXACT_KANY:   // CGGI / LMSS, any RLWE length: sums in memory
        HIPCHK(c, mktd::launch_exact_blindrotate_kany(c->logN, c->ks->d_ntt, xbrk, xmono, lwe, stride, pre, p.n, p.k, p.l_gsw, p.logB_gsw, blk_len, (uint32_t *)acc,
                                                      reinterpret_cast<uint64_t *>(scratch), B, c->stream));
        return MKT_OK;
    case Route::EXACT_KR:     // CGGI / LMSS with RLWE length 2, 3 or another block length: the general kernel
        HIPCHK(c, mktd::launch_exact_blindrotate_kr(c->logN, c->ks->d_ntt, xbrk, xmono, lwe, stride, pre, p.n, p.k, p.l_gsw, p.logB_gsw, blk_len, (uint32_t *)acc, B, c->stream));
        return MKT_OK;
    case Route::EXACT_K1:     // CGGI / LMSS, RLWE length 1, 32-bit ring (exact_gate_ok): every product exact mod 2^32
        HIPCHK(c, mktd::launch_exact_blindrotate(c->logN, c->ks->d_ntt, xbrk, xmono, lwe, stride, pre, p.n, p.l_gsw, p.logB_gsw, blk_len, (uint32_t *)acc, B, c->stream));
        return MKT_OK;
    case Route::EXACT_FX: {   // CGGI on the Float64 pipe (fx_exact.hip)
        mktd::FxRotArgs f = fx_rot_args(c, lwe, stride, pre);
        f.init_mode = 0; f.acc_io = acc; f.ngates = B;
        HIPCHK(c, mktd::launch_fx_blindrotate(c->logM, p.W, f, B, c->stream));
        return MKT_OK;
    }
    default: break;           // F64_K1, F64_KR, F64_KANY
    }
    mktd::RotArgs a = rot_args(c, lwe, stride, pre);
    a.init_mode = 0; a.out_mode = 0; a.acc_io = acc; a.ngates = B;
    if (route == Route::F64_KANY) HIPCHK(c, mktd::launch_blindrotate_kany(c->logM, p.W, p.k, a, scratch, B, c->stream));   // any RLWE length: accumulators in memory (blindrotate_kany_kernel)
    else if (route == Route::F64_KR) HIPCHK(c, mktd::launch_blindrotate_kr(c->logM, p.W, p.k, a, B, c->stream));         // RLWE length 2, 3 (CGGI, LMSS): accumulators in registers
    else HIPCHK(c, mktd::launch_blindrotate_k1(c->logM, p.W, a, B, c->stream));
    return MKT_OK;
}

// src / coef (device, [B]) / nacc: the key switch at a coefficient, out[g] = keyswitch!(E_coef[g](acc[src[g]])) (device_api.h KsArgs); both null = keyswitch!
int do_keyswitch(mkt_ctx *c, const void *acc, uint32_t *out, size_t B, const uint32_t *src = nullptr, const uint32_t *coef = nullptr, size_t nacc = 0) {
    const mkt_params &p = c->p;
    mktd::KsArgs a{};
    a.src = src; a.coef = coef; a.nacc = nacc;
    a.acc = acc; a.out = out; a.ksk = c->ks->d_ksk; a.ksk_party_stride = c->ks->stride(T_KSK); a.n1p = c->ks->ksk.n1p;
    a.N = p.N; a.n = p.n; a.f = p.f; a.logD = p.logD; a.drows = c->sh.ksk_drows; a.kacc = c->sh.kacc;
    a.mk = mkt::is_mk(p.scheme) ? 1 : 0; a.balanced = mkt::is_block(p.scheme) ? 1 : 0; a.lmss = p.scheme == MKT_LMSS ? 1 : 0;
    a.planes = c->ks->d_ksk_planes; a.sum_mfma = mktd::launch_ks_mfma; a.planes_block_stride = mktd::ksm_block_bytes(p.N, p.f, a.n1p);   // (a party's key of a multi-key scheme is one block: describe_key_set)
    const mktd::KsReport plan = mktd::ks_report(mktd::ks_shape(a, true), B, mktd::launch_tuning());   // scratch present: it is sized from this plan, below
    if (B) c->ks_last = plan;
    c->ks_mfma_last = B && plan.kernel == 3;
    const size_t dw = plan.digit_words, pw = plan.partial_words;
    HIPCHK(c, c->ws.ksd.reserve((dw + pw) * 4));
    if (dw) { a.digits = c->ws.ksd.as<uint32_t>(); a.partial = a.digits + dw; }
    Timer tm(c, 2);
    HIPCHK(c, mktd::launch_keyswitch(p.W, a, B, c->stream));
    return MKT_OK;
}

// bootstrapping.jl:8-24 (mod-switch, test vector, blindrotate!) for a device-resident chunk of linear combinations: ws.acc <- accumulators
int rotate_chunk(mkt_ctx *c, const uint32_t *lin, size_t B) {
    const mkt_params &p = c->p;
    if (!mkt::is_kms(p.scheme)) {
        HIPCHK(c, mktd::launch_testvector(p.W, lin, c->sh.lwe_len, c->logN, c->sh.kacc, c->ws.acc.p, B, c->stream));
        return do_blindrotate(c, lin, c->sh.lwe_len, 0, nullptr, c->ws.acc.p, B);
    }
    return do_blindrotate(c, lin, c->sh.lwe_len, 0, lin, c->ws.acc.p, B);
}

// bootstrapping!(lin) -> out for a device-resident chunk
int bootstrap_chunk(mkt_ctx *c, const uint32_t *lin, uint32_t *out, size_t B) {
    int r;
    if ((r = rotate_chunk(c, lin, B))) return r;
    return do_keyswitch(c, c->ws.acc.p, out, B);
}

// A caller's lookup tables on the device: luts [nluts][N] ring words, sel [B] rows or nullptr (row 0)
struct LutArgs { const void *luts; size_t nluts; const uint32_t *sel; };

// ---- lookup-table bootstrap (mktfhe.h "programmable bootstrap", "many-table bootstrap", "key switch at a coefficient") ----
// One chunk of any of them: the tables, the mod-switch exponent nu (0: the caller's words as they are; 1 .. 3: the grid 2^nu times coarser),
// `per` outputs per input, and where the key switch reads.  at: output row j * per + i is accumulator j at coef[i] (coef [per] on the device;
// nullptr = the list 0 .. per - 1, the many-table form), through the context's (row, coefficient) table ws.at.  Not at (per == 1): the plain
// key switch, coefficient 0 of every accumulator
struct LutChunk { LutArgs t; int nu; size_t per; bool at; const uint32_t *coef; };

// ws.at <- where every output row of a chunk's key switch reads.  Written once per call, for its largest chunk (a shorter last chunk reads
// a prefix), 8 bytes per output row
int at_table(mkt_ctx *c, const LutChunk &k, size_t rows) {
    HIPCHK(c, c->ws.at.reserve(rows * 8));
    HIPCHK(c, mktd::launch_ks_at_table(k.coef, k.per, c->ws.at_src(), c->ws.at_coef(), rows, c->stream));
    return MKT_OK;
}

// a device-resident chunk of B inputs: lin [B][len] -> out [B * per][len] (out may be lin when per == 1: the masks and b are read before the
// key switch writes).  ws.acc <- (X^btilde T, 0 ...) for the caller's table, then blindrotate! with the accumulator it is handed (the multi-key
// phase 2 with lin_for_tv == nullptr, as mkt_blindrotate_batch runs it): on the caller's masks for nu = 0, else on the coarse-switched mask
// words, which go to ws.lin (rows of lwe_len words; lin may BE ws.lin, the gather form).  The key switch reads the B rotated accumulators
// where they lie in ws.acc
int lut_chunk(mkt_ctx *c, const LutChunk &k, const uint32_t *lin, uint32_t *out, size_t B) {
    const int len = c->sh.lwe_len;
    uint32_t *const ws_lin = c->ws.lin.as<uint32_t>();
    void *const acc = c->ws.acc.p;
    int r;
    if (!k.nu) HIPCHK(c, mktd::launch_lut_testvector(c->p.W, k.t.luts, k.t.nluts, k.t.sel, lin, len, c->logN, c->sh.kacc, acc, B, c->stream));
    else HIPCHK(c, mktd::launch_lut_many_testvector(c->p.W, k.t.luts, k.t.nluts, k.t.sel, lin, len, c->logN, c->sh.kacc, k.nu, ws_lin, len, acc, B, c->stream));
    if ((r = do_blindrotate(c, k.nu ? ws_lin : lin, len, k.nu ? 1 : 0, nullptr, acc, B))) return r;
    if (!k.at) return do_keyswitch(c, acc, out, B);
    return do_keyswitch(c, acc, out, B * k.per, c->ws.at_src(), c->ws.at_coef(), B);
}

// staging helper for MKT_MEM_HOST callers
struct Staged {
    mkt_ctx *c; void *dev = nullptr; size_t bytes = 0; DevBuf own;   // dev: the caller's device array, or own.p -- a host array's copy for this call
    template <class T> T *as() const { return static_cast<T *>(dev); }
    // align: what the kernels that are handed `dev` need beyond the alignment of the element type (mktfhe.h "ALIGNMENT"); a staged copy has hipMalloc's
    int in(const void *ptr, size_t nbytes, int mem, bool copy_in, size_t align = 1) {
        bytes = nbytes;
        if (mem == MKT_MEM_DEVICE) {
            if (reinterpret_cast<uintptr_t>(ptr) % align) return fail(c, MKT_ERR_ARG, "a device buffer of this call must be aligned to " + std::to_string(align) + " bytes");
            dev = const_cast<void *>(ptr); return MKT_OK;
        }
        hipError_t e = own.alloc(nbytes);
        if (e != hipSuccess) return hipfail(c, e, "hipMalloc(staging)");
        dev = own.p;
        if (copy_in && nbytes) { e = hipMemcpyAsync(dev, ptr, nbytes, hipMemcpyHostToDevice, c->stream); if (e != hipSuccess) return hipfail(c, e, "H2D"); }
        return MKT_OK;
    }
    int out(void *ptr) {
        if (!own.p || !bytes) return MKT_OK;
        hipError_t e = hipMemcpyAsync(ptr, dev, bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return hipfail(c, e, "D2H");
        return MKT_OK;
    }
    ~Staged() { if (own.p) (void)hipStreamSynchronize(c->stream); }   // drained, then `own` frees
};

// A secret on the device for the length of one scope (the TRUST note in mktfhe.h): uploaded on the context's stream; zeroed on that stream and
// the stream drained before the buffer is freed, by whatever path the scope is left.  Declared AFTER a call's Staged objects: its wipe is drained before they free
struct RingKeys { int first = 0, count = 0; };   // a party's ring-key polynomials [first, first + count)
struct DeviceSecret {
    mkt_ctx *c; DevBuf buf; size_t bytes = 0;
    template <class T> T *as() const { return buf.as<T>(); }
    hipError_t alloc(size_t nbytes) { bytes = nbytes; return buf.alloc(nbytes); }
    hipError_t in(const void *host, size_t nbytes) { const hipError_t e = alloc(nbytes); return e != hipSuccess ? e : hipMemcpyAsync(buf.p, host, nbytes, hipMemcpyHostToDevice, c->stream); }
    // ring-key polynomials rk of K, end to end (the host keeps them one vector each)
    hipError_t ring_keys(const mkt_client_party *K, RingKeys rk) {
        const size_t N = (size_t)c->p.N;
        hipError_t e = alloc((size_t)rk.count * N);
        for (int q = 0; q < rk.count && e == hipSuccess; q++) e = hipMemcpyAsync(as<int8_t>() + q * N, K->zring[(size_t)rk.first + q].data(), N, hipMemcpyHostToDevice, c->stream);
        return e;
    }
    hipError_t wipe_now() {   // behind everything enqueued so far; the result of draining the stream
        if (!buf.p) return hipSuccess;
        (void)hipMemsetAsync(buf.p, 0, bytes, c->stream);
        const hipError_t e = hipStreamSynchronize(c->stream);
        buf.release();
        return e;
    }
    ~DeviceSecret() { (void)wipe_now(); }
};
// the end of a party-local call: the secret wiped, and the host copy of the stream key in the argument struct (the kernel-argument copy: TRUST note in mktfhe.h)
template <class Args> hipError_t wipe_secrets(hipError_t e, DeviceSecret &secret, Args &a) {
    const hipError_t es = secret.wipe_now();
    explicit_bzero(&a, sizeof a);
    return e != hipSuccess ? e : es;   // the call's status so far, else that of the drain
}
// The start of both device keygens (keygen.hip, keygen_seeded.hip), on the context's stream: the party's LWE key and ring keys uploaded as secrets, the call's
// output buffers allocated (outs: owner, bytes), the integer CRS uploaded for CCS; and the fields KeygenArgs and KeygenSeededArgs share
struct KeygenOut { DevBuf *buf; size_t bytes; };
template <class Args> hipError_t keygen_setup(mkt_ctx *c, const mkt_client_party *K, const void *crs, DeviceSecret &lwe, DeviceSecret &z, std::initializer_list<KeygenOut> outs, DevBuf &crs_int, Args &a) {
    const mkt_params &p = c->p;
    const bool unienc = p.scheme == MKT_CCS;
    const int N = p.N;
    const size_t crs_bytes = (size_t)p.l_uni * poly_bytes(c);
    hipError_t e = lwe.in(K->lwekey.data(), (size_t)p.n * 4);
    if (e == hipSuccess) e = z.ring_keys(K, {0, (int)K->zring.size()});
    for (const KeygenOut &o : outs) if (e == hipSuccess) e = o.buf->alloc(o.bytes);
    if (e == hipSuccess && unienc) e = crs_int.alloc(crs_bytes);
    if (e == hipSuccess && unienc) e = hipMemcpyAsync(crs_int.p, crs, crs_bytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return e;   // (the stream key is copied only into a struct that the call goes on to wipe: wipe_secrets)
    std::memcpy(a.key, K->key, sizeof a.key); a.party = K->party; a.N = N; a.n = p.n; a.W = p.W; a.f = p.f; a.logD = p.logD;
    a.sigma_ring = K->sigma_ring; a.sigma_lwe = K->sigma_lwe;
    a.lwekey = lwe.as<const uint32_t>(); a.zring = z.as<const int8_t>(); a.crs = crs_int.p;
    if (unienc) { a.kr = 1; a.l = p.l_uni; a.logB = p.logB_uni; }
    else { a.kr = c->sh.kr; a.l = p.l_gsw; a.logB = p.logB_gsw; }
    return e;
}
// every ring key the keygen kernels index is there: kr of them from 0 for the bootstrapping key (one under CCS), ksk_kr of them from the key switch's
// first (the uni key of the KMS schemes: 1) -- the same in keygen.hip and keygen_seeded.hip
bool ring_keys_cover(const mkt_ctx *c, const mkt_client_party *K) {
    const int nz = (int)K->zring.size();
    return nz >= (c->p.scheme == MKT_CCS ? 1 : c->sh.kr) && nz >= (mkt::is_kms(c->p.scheme) ? 1 : 0) + c->sh.ksk_kr;
}
bool mem_ok(int mem) { return mem == MKT_MEM_DEVICE || mem == MKT_MEM_HOST; }
// the ring keys packed ciphertexts are under: the ones the key-switching key switches from (the uni key of the KMS schemes: 1)
RingKeys pack_ring_keys(const mkt_ctx *c) { return c ? RingKeys{mkt::is_kms(c->p.scheme) ? 1 : 0, c->sh.ksk_kr} : RingKeys{}; }
// The refusals a party-local call `who` opens with: a null context or key, a bad argument of its own (args_ok) or a party out of range; keys made
// for other parameters or another party; and, where the call reads ring keys itself, keys without the polynomials rk
int party_call_guard(mkt_ctx *c, const char *who, bool args_ok, int party, const mkt_client_party *K, RingKeys rk = {}) {
    if (!c || !K || !args_ok || party < 0 || party >= c->sh.nparty) return fail(c, MKT_ERR_ARG, "bad argument");
    if (!mkt::party_keys_match(K, c->p, party)) return fail(c, MKT_ERR_ARG, std::string(who) + ": the party's keys were made for other parameters / another party index");
    if ((int)K->zring.size() < rk.first + rk.count) return fail(c, MKT_ERR_ARG, std::string(who) + ": the party's keys lack a ring key");
    return MKT_OK;
}

// ---- MKT_ARITH_EXACT: tables of the two-prime negacyclic NTT (ntt_exact.hip), computed on the host, uploaded once ----
constexpr uint32_t NTT_P[2] = {1073668097u, 1073692673u};        // 131063 * 2^13 + 1, 131066 * 2^13 + 1: the two largest NTT primes below 2^30 (ntt_exact.hip)
uint32_t ntt_mulmod(uint32_t a, uint32_t b, uint32_t p) { return (uint32_t)((uint64_t)a * b % p); }
uint32_t ntt_powmod(uint32_t a, uint64_t e, uint32_t p) { uint32_t r = 1; while (e) { if (e & 1) r = ntt_mulmod(r, a, p); a = ntt_mulmod(a, a, p); e >>= 1; } return r; }
uint32_t ntt_shoup(uint32_t w, uint32_t p) { return (uint32_t)(((uint64_t)w << 32) / p); }

// per point (w mod p1, companion, w mod p2, companion; the table holds 2^32 - w): psi_rev[N] | N^-1, N^-1 w | N^-1 2^32, N^-1 2^32 w, for the transform of
// size N (no inverse table: psiinv_rev[m + i] = -psi_rev[2m - 1 - i], which the inverse butterflies read off the forward table, ntt_exact.hip bfly_inv); psi = g^((p - 1) / 2N) with g the smallest quadratic non-residue of p (so psi^N = -1: a primitive 2N-th root of unity)
int upload_ntt_tables(mkt_ctx *c) {
    const int N = c->p.N, logN = c->logN;
    std::vector<uint32_t> tab((size_t)(N + 4) * 4);
    for (int k = 0; k < 2; k++) {
        const uint32_t p = NTT_P[k];
        uint32_t g = 2;
        while (ntt_powmod(g, (p - 1) / 2, p) != p - 1) g++;
        const uint32_t psi = ntt_powmod(g, (p - 1) / (2 * (uint64_t)N), p), psiinv = ntt_powmod(psi, p - 2, p);
        if (ntt_powmod(psi, (uint64_t)N, p) != p - 1) return fail(c, MKT_ERR_UNSUPPORTED, "no primitive 2N-th root of unity for this ring dimension");
        for (int i = 0; i < N; i++) {
            int r = 0;
            for (int b = 0; b < logN; b++) r |= ((i >> b) & 1) << (logN - 1 - b);
            const uint32_t w = ntt_powmod(psi, (uint64_t)r, p);
            tab[(size_t)i * 4 + 2 * k] = 0u - w; tab[(size_t)i * 4 + 2 * k + 1] = ntt_shoup(w, p);   // the NEGATED twiddle (ntt_exact.hip bfly_fwd, bfly_inv)
        }
        // N^-1 and N^-1 2^32, each followed by its product with the one twiddle of the inverse's last stage (psiinv_rev[1])
        const uint32_t ninv = ntt_powmod((uint32_t)N, p - 2, p), ninv_r = (uint32_t)(((uint64_t)ninv << 32) % p);
        const uint32_t wlast = ntt_powmod(psiinv, (uint64_t)N / 2, p);                    // bitrev(1) = N / 2
        const uint32_t cs[4] = {ninv, ntt_mulmod(ninv, wlast, p), ninv_r, ntt_mulmod(ninv_r, wlast, p)};
        for (int q = 0; q < 4; q++) { tab[(size_t)(N + q) * 4 + 2 * k] = cs[q]; tab[(size_t)(N + q) * 4 + 2 * k + 1] = ntt_shoup(cs[q], p); }
    }
    HIPCHK(c, hipMemcpy(c->ks->d_ntt, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    return MKT_OK;
}
// (every true product coefficient below P / 2 = 2^58.9998: 2l polynomials of N digits of magnitude <= 2^(logB-1) against 32-bit words)
bool exact_gate_ok(const mkt_ctx *c) {
    const double half_P = 0.5 * (double)NTT_P[0] * (double)NTT_P[1];
    const mkt_params &p = c->p;
    // ring words and their 32-bit pieces enter as centered integers (magnitude <= 2^31: ntt_exact.hip res_word / piece_of)
    const double n31 = (double)p.N * 2147483648.0;
    if (mkt::is_kms(p.scheme) && p.W == 64) {
        // 64-bit ring: tables split into 32-bit halves, every accumulated product sum of one half must stay below P / 2:
        // phase 1 (KMS: the sum of the 2l products, the monomial X^a - 1 is applied after the lift; KMS_block: a block sums
        // its key bits' products times their monomials before the inverse), the LEV multiplication + relinearisation sums,
        // the v sum over the parties
        const double ph1 = (p.scheme == MKT_KMS_BLOCK ? 2.0 * p.blk_len : 1.0) * 2.0 * p.l_gsw * std::ldexp(1.0, p.logB_gsw - 1) * n31;
        const double acc = (p.l_lev * std::ldexp(1.0, p.logB_lev - 1) + 2.0 * p.l_uni * std::ldexp(1.0, p.logB_uni - 1)) * n31;
        const double tv = (double)p.k * p.l_uni * std::ldexp(1.0, p.logB_uni - 1) * n31;
        return ph1 < half_P && acc < half_P && tv < half_P;
    }
    if (p.scheme == MKT_CCS && p.W == 32)    // tacc.b gathers u_0 and the w of all np + 1 polynomials, then the monomial doubles it
        return 2.0 * (p.k + 2.0) * p.l_uni * std::ldexp(1.0, p.logB_uni - 1) * n31 < half_P;
    const bool lmss = p.scheme == MKT_LMSS;
    if (!((p.scheme == MKT_CGGI || lmss) && p.k >= 1 && p.W == 32)) return false;     // any RLWE length (exact_blindrotate_kr_kernel beyond the k = 1, block-length-3 shapes; exact_blindrotate_kany_kernel beyond k = 3)
    // the kernels multiply the product sum by the monomial X^a - 1 in the transform domain BEFORE the one lift (ntt_exact.hip
    // exact_blindrotate_kernel: s2 = tacc * mono), so the lifted integer is up to twice the sum -- for CGGI as for a block;
    // (k + 1) l digit polynomials per key bit
    const double bound = 2.0 * (lmss ? p.blk_len : 1.0) * (p.k + 1.0) * p.l_gsw * std::ldexp(1.0, p.logB_gsw - 1) * n31;
    return bound < half_P;
}
#define MKT_EXACT_GATE(c) do { if ((c) && (c)->exact && !exact_gate_ok(c)) return fail((c), MKT_ERR_UNSUPPORTED, "MKT_ARITH_EXACT evaluates gates for CGGI and LMSS (32-bit ring), for CCS (32-bit ring) and for KMS / KMS_block (64-bit ring, tables split in 32-bit halves), gadgets within the two-prime modulus; other schemes offer the transform-level entry points (mkt_transform_*_batch, mkt_exact_polymul_batch)"); } while (0)
#define MKT_F64_OR_EXACT_KMS(c) do { if ((c) && (c)->exact && !mkt::is_mk((c)->p.scheme)) return fail((c), MKT_ERR_UNSUPPORTED, "on an MKT_ARITH_EXACT context this entry point serves the multi-key gate paths only"); MKT_EXACT_GATE(c); } while (0)   // (a multi-key set beyond the modulus: the refusal that names it)
#define MKT_F64_ONLY(c) do { if ((c) && (c)->exact) return fail((c), MKT_ERR_UNSUPPORTED, "this entry point is the Float64-reference gate path; not offered by an MKT_ARITH_EXACT context"); } while (0)

// ---- MKT_ARITH_EXACT on the Float64 pipe (fx_exact.hip) ----
// Which shapes keep a second copy of the bootstrapping key as limb transforms: CGGI with RLWE length 1 and KMS (phase 1), gadget lengths the kernel holds in registers.
bool fx_shape(const mkt_ctx *c) {
    const mkt_params &p = c->p;
    return c->exact && ((p.scheme == MKT_CGGI && p.k == 1) || p.scheme == MKT_KMS) && mktd::fx_supported(c->logM, p.W, p.l_gsw);
}
// Proven bound on |computed coefficient - exact integer| of one rounded sum  sum_g d_g (*) limb_g  (DESIGN.md section 2), u = 2^-53:
//   transform-domain errors reach a coefficient through the 1-norm:  (gamma_f + gamma_k + gamma_m) sum_g |d_g|_2 |limb_g|_2
//   the inverse's own roundings are relative to the 2-norm of what it transforms:  gamma_i sum_g |d_g|_2 max_r |K_g[r]|
// with |d_g|_2 <= sqrt(N) 2^(logB-1), |limb_g|_2 <= sqrt(N) 2^15, max_r |K[r]| MEASURED over the loaded key (kmax; a random key sits near
// 4 sqrt(N) 2^15 / sqrt(3), an adversarial one at N 2^15 fails the bound and the integer NTT serves), per-stage constants 5.5 u (6-operation
// butterfly incl. the rounded twiddle), 1.5 u (product-free stages), 3 u (twist / untwist), (2 + 6 l) u for the multiply-add chain.
double fx_bound(const mkt_ctx *c, double kmax) {
    const mkt_params &p = c->p;
    const double u = std::ldexp(1.0, -53), g2 = 2.0 * p.l_gsw;
    const double gt = (3.0 + 5.5 * (c->logM - 2) + 1.5 * 2) * u, gm = (2.0 + 3.0 * g2) * u;     // (chain of 2 g2 fused operations per component, sqrt(2) for the complex value: 2.83 g2 u)
    const double dn = std::sqrt((double)p.N) * std::ldexp(1.0, p.logB_gsw - 1), kn = std::sqrt((double)p.N) * 32768.0;
    return (gt + (gt + u) + gm) * g2 * dn * kn + gt * g2 * dn * kmax * (1.0 + 1e-6);
}
bool fx_usable(const mkt_ctx *c) {
    if (!c->ks->d_fx_brk || c->tune.exact_impl == 0 || c->ks->fx_kmax <= 0.0) return false;
    const mkt_params &p = c->p;
    if (2.0 * p.l_gsw * p.N * std::ldexp(1.0, p.logB_gsw - 1) * 32768.0 >= std::ldexp(1.0, 50)) return false;   // the rounding trick holds integers below 2^51
    return fx_bound(c, c->ks->fx_kmax) < 0.45;
}
// The same bound for ONE product a (*) limb of mkt_exact_polymul_batch (one term instead of 2l): |a|_2 <= sqrt(N) amax, |limb|_2 <= sqrt(N) 2^15,
// kmax = the largest |transform value| of b's limbs, measured on the device before the product runs (fx_key_fwd_kernel without output);
// the multiply chain is one complex product (gamma_m = 5 u).  At the contract edge (N amax = 2^28 - 2^15) with a worst-case b (kmax = N 2^15)
// it is 0.37 at N = 128 and above 1/2 from N = 256 on -- such calls are served by the integer NTT.
double fx_polymul_bound(const mkt_ctx *c, double amax, double kmax) {
    const double u = std::ldexp(1.0, -53), N = (double)c->p.N;
    const double gt = (3.0 + 5.5 * (c->logM - 2) + 1.5 * 2) * u, gm = 5.0 * u;
    return (gt + (gt + u) + gm) * N * amax * 32768.0 + gt * std::sqrt(N) * amax * kmax * (1.0 + 1e-6);
}
hipError_t fx_after_key_load(mkt_ctx *c) {   // the key's largest transform magnitude, for fx_bound
    unsigned long long bits = 0;
    const hipError_t e = hipMemcpy(&bits, c->ks->d_fx_stat, 8, hipMemcpyDeviceToHost);
    double v; std::memcpy(&v, &bits, 8);
    if (e == hipSuccess) c->ks->fx_kmax = std::sqrt(v);
    return e;
}
mktd::FxRotArgs fx_rot_args(mkt_ctx *c, const uint32_t *lwe, int stride, int pre) {
    const mkt_params &p = c->p;
    mktd::FxRotArgs q{};
    q.om = c->fx_om(); q.twist = c->fx_tw(); q.nat = c->fx_nat(); q.brk = c->ks->d_fx_brk; q.brk_party_stride = c->ks->stride(T_FX_BRK);
    q.lwe = lwe; q.lwe_stride = stride; q.pre_switched = pre; q.n = p.n; q.logN = c->logN; q.l = p.l_gsw; q.logB = p.logB_gsw;
    q.rows_per_gate = c->ks->rtot; q.slot_party = c->ks->d_slot_party; q.slot_row = c->ks->d_slot_row; q.logB_lev = p.logB_lev;
    q.stagger = c->tune.rot_stagger; q.map_mode = c->tune.rot_map; q.split = c->tune.rot_split;
    return q;
}

// The one description of the resident key set of `c` (KeySet::tab, ksk); c->ks->rtot and the switches are set before.
void describe_key_set(mkt_ctx *c) {
    KeySet &ks = *c->ks;
    const mkt_params &p = c->p;
    const size_t M = (size_t)c->M, N = (size_t)p.N;
    const size_t tp = M * c->split;   // complex values of one resident key polynomial (EXACT on the 64-bit ring: two residue polynomials per logical one)
    const bool mk = mkt::is_mk(p.scheme), kms = mkt::is_kms(p.scheme);
    ks.ksk = mkt::ksk_layout(p, c->sh);
    // second copy of the bootstrapping key as limb transforms + the engine's own tables, where a party's copy fits one buffer descriptor (2 GiB)
    const size_t fx_per = (size_t)p.n * 2 * p.l_gsw * 2 * (p.W / 16) * M;
    const bool fx = fx_shape(c) && c->tune.exact_impl != 0 && fx_per * sizeof(cplx) <= 0x7fffffffull;
    auto row = [&](KeyTable t, auto &member, size_t elems, bool per_party, bool present, bool cloned) { ks.tab[t] = ResidentTable{(void **)&member, elems, sizeof(*member), per_party, present, cloned}; };
    //  table         pointer          elements                                                       per party  present  cloned
    row(T_TW,         ks.d_tw,         4 * M,                                                         false,     true,    true);    // a caller may have replaced them on the source (mkt_set_twiddles)
    row(T_MONOMIAL,   ks.d_monomial,   2 * N * M,                                                     false,     true,    true);    // depends on the twiddles; small coefficients, never split
    row(T_BRK,        ks.d_brk,        (size_t)p.n * c->sh.brk_polys * tp,                            true,      true,    true);
    row(T_KSK,        ks.d_ksk,        ks.ksk.resident_words(),                                        true,      true,    true);
    row(T_PUB,        ks.d_pub,        (size_t)p.l_uni * tp,                                          true,      mk,      true);
    row(T_CRS,        ks.d_crs,        (size_t)p.l_uni * tp,                                          false,     mk,      true);
    row(T_RLK_D,      ks.d_rlk_d,      (size_t)p.l_uni * tp,                                          true,      kms,     true);
    row(T_RLK_F,      ks.d_rlk_f,      (size_t)p.l_uni * 2 * tp,                                      true,      kms,     true);
    row(T_SLOT_PARTY, ks.d_slot_party, (size_t)ks.rtot,                                               false,     true,    false);
    row(T_SLOT_ROW,   ks.d_slot_row,   (size_t)ks.rtot,                                               false,     true,    false);
    row(T_FX_TAB,     ks.d_fx_tab,     3 * M,                                                         false,     fx,      false);
    row(T_FX_BRK,     ks.d_fx_brk,     fx_per,                                                        true,      fx,      true);
    row(T_FX_STAT,    ks.d_fx_stat,    1,                                                             false,     fx,      true);
    row(T_NTT,        ks.d_ntt,        (N + 4) * 2,                                                   false,     c->exact, false);   // (N + 4) points of 4 words (upload_ntt_tables)
    // second form of the key-switching key (ks_mfma.h): one block of planes per component of a party's key, 4/3 of its rows' bytes.  Unbalanced
    // digits with D = 4 (three rows per digit), no 32-bit sum able to overflow (ks_mfma_fits), MKT_KS_MFMA not 0.  OPTIONAL: mkt_ctx_create
    // goes on without it where the allocation fails, and every key switch then runs the kernels it ran before
    const bool planes = mktd::launch_tuning().ks_mfma != 0 && p.logD == 2 && !mkt::is_block(p.scheme) && c->sh.ksk_drows == 3 && (!mk || c->sh.ksk_kr == 1) &&
                        mkt::ks_mfma_fits(p.N, mk ? 1 : c->sh.kacc, p.f);
    row(T_KSK_PLANES, ks.d_ksk_planes, (size_t)c->sh.ksk_kr * mktd::ksm_block_bytes(p.N, p.f, ks.ksk.n1p),   true,      planes,   true);
}

// ---- the one install path of a party's keys ----  The start of every call that writes keys: the argument check (ptrs_ok: the call's own pointers; party NO_PARTY: the CRS, or a party
// checked further on; scheme_ok: the schemes that have the piece), the arithmetic gate, the key set still this context's alone
constexpr int NO_PARTY = -1; enum class Gate { EXACT, F64_OR_EXACT_KMS };   // MKT_EXACT_GATE, MKT_F64_OR_EXACT_KMS
int key_write_guard(mkt_ctx *c, bool ptrs_ok, int party, Gate gate, bool (*scheme_ok)(int) = nullptr) {
    if (!c || !ptrs_ok || (party != NO_PARTY && (party < 0 || party >= c->sh.nparty)) || (scheme_ok && !scheme_ok(c->p.scheme))) return fail(c, MKT_ERR_ARG, "bad argument");
    if (gate == Gate::EXACT) MKT_EXACT_GATE(c); else MKT_F64_OR_EXACT_KMS(c);
    return keys_writable(c);
}
// A party's bootstrapping key, in coefficient form on the device at `src`, into the resident tables: the transforms (and the limb
// transforms where the key set keeps them), the stream drained, the limb maximum read back; marked only once all of it has succeeded
hipError_t install_brk(mkt_ctx *c, int party, const void *src) {
    KeySet &ks = *c->ks;
    hipError_t e = to_resident(c, src, mkt::brk_polys_total(c->p, c->sh), ks.party<cplx>(T_BRK, party), false, ks.d_fx_brk ? ks.party<cplx>(T_FX_BRK, party) : nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && ks.d_fx_brk) e = fx_after_key_load(c);
    if (e == hipSuccess) ks.loaded.mark(mkt::K_BRK, party);
    return e;
}
// The key-switching key between its two layouts (mkt::KskLayout), on the context's stream: a party's table zeroed (the padding and the rows a
// generator leaves absent), rows at the callers' pitch into it, and rows at the resident pitch (`padded`) out to a caller
hipError_t ksk_zero(mkt_ctx *c, int party) { return hipMemsetAsync(c->ks->party<uint32_t>(T_KSK, party), 0, c->ks->stride(T_KSK) * sizeof(uint32_t), c->stream); }
hipError_t ksk_repitch(mkt_ctx *c, uint32_t *dst, int dpitch, const uint32_t *src, int spitch, hipMemcpyKind kind) { return hipMemcpy2DAsync(dst, (size_t)dpitch * 4, src, (size_t)spitch * 4, (size_t)c->ks->ksk.n1 * 4, c->ks->ksk.rows, kind, c->stream); }
hipError_t ksk_to_resident(mkt_ctx *c, int party, const uint32_t *rows, hipMemcpyKind kind) { return ksk_repitch(c, c->ks->party<uint32_t>(T_KSK, party), c->ks->ksk.n1p, rows, c->ks->ksk.n1, kind); }
hipError_t ksk_to_rows(mkt_ctx *c, const uint32_t *padded, uint32_t *rows, hipMemcpyKind kind) { return ksk_repitch(c, rows, c->ks->ksk.n1, padded, c->ks->ksk.n1p, kind); }
// ... and, once a party's rows stand in the resident table (every install ends here), their byte planes where the key set keeps them
hipError_t ksk_to_planes(mkt_ctx *c, int party) {
    KeySet &ks = *c->ks;
    if (!ks.d_ksk_planes) return hipSuccess;
    const size_t comp_words = (size_t)c->p.N * c->sh.ksk_drows * c->p.f * ks.ksk.n1p, block = mktd::ksm_block_bytes(c->p.N, c->p.f, ks.ksk.n1p);
    for (int comp = 0; comp < c->sh.ksk_kr; comp++)
        if (hipError_t e = mktd::launch_ks_mfma_pack(ks.party<uint32_t>(T_KSK, party) + comp * comp_words, ks.party<int8_t>(T_KSK_PLANES, party) + comp * block,
                                                     c->p.N, c->p.f, c->sh.ksk_drows, ks.ksk.n1p, c->stream); e != hipSuccess) return e;
    return hipSuccess;
}

}  // namespace

extern "C" {

int mkt_abi_version(void) { return MKT_ABI_VERSION; }

const char *mkt_last_error(const mkt_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int mkt_ctx_create(const mkt_params *params, int arith_mode, int device, mkt_ctx **out) {
    if (!params || !out) return fail(nullptr, MKT_ERR_ARG, "null argument");
    *out = nullptr;
    std::string why;
    if (mkt::validate_params(*params, why)) return fail(nullptr, MKT_ERR_ARG, why);
    if (arith_mode != MKT_ARITH_F64REF && arith_mode != MKT_ARITH_EXACT) return fail(nullptr, MKT_ERR_ARG, "unknown arithmetic mode");
    const int logN = __builtin_ctz((unsigned)params->N);
    if (!mktd::transform_supported(logN - 1)) return fail(nullptr, MKT_ERR_UNSUPPORTED, "ring dimension not instantiated (N must be 32..4096)");
    // the Float64 rotation of a block scheme with one mask polynomial (LMSS at RLWE length 1, KMS_block) holds the block length as a template
    // constant, 1 .. 4 (kernels.hip launch_rot_blk, rot_block.hip launch_blk_lb); refused here, not by the first rotation's launcher
    if (arith_mode == MKT_ARITH_F64REF && (params->scheme == MKT_KMS_BLOCK || (params->scheme == MKT_LMSS && params->k == 1)) && params->blk_len > 4)
        return fail(nullptr, MKT_ERR_UNSUPPORTED, "block length beyond 4 is not instantiated for MKT_ARITH_F64REF at RLWE length 1 (LMSS with k = 1, KMS_block): block length 1 .. 4 there, any with k >= 2 or under MKT_ARITH_EXACT");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(nullptr, MKT_ERR_NO_DEVICE, "no HIP device available: the engine has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(nullptr, MKT_ERR_ARG, "device index out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, MKT_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(nullptr, MKT_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", the engine is built for gfx950 only");

    // MKT_MEM_GUARD (KiB; device_mem.h), read where the switches are seeded: the guard length of every buffer the process allocates from here on, 0 or unset = none
    // (mkt_multi_create comes through here for every root shard)
    const int guard_kib = env_int("MKT_MEM_GUARD", 0);
    if (guard_kib < 0 || guard_kib > (1 << 20) || !mkt::memguard::set_guard_length((size_t)guard_kib * 1024)) return fail(nullptr, MKT_ERR_ARG, "MKT_MEM_GUARD: a guard length in KiB, 0 .. 2^20");

    auto *c = new mkt_ctx();
    c->ks = new_key_set();
    c->ks->device = device;
    c->p = *params; c->sh = mkt::shape_of(*params); c->device = device;
    c->logN = logN; c->logM = logN - 1; c->M = params->N / 2;
    c->exact = arith_mode == MKT_ARITH_EXACT;
    c->split = (c->exact && params->W == 64) ? 2 : 1;
    // the RLWE-length-k kernels of the plain schemes want the slot-pair order, everything else the slot-major one (fft_device.h)
    c->dev_order = ((params->scheme == MKT_CGGI || params->scheme == MKT_LMSS) && params->k > 1) ? MKT_DEVORDER_KR : MKT_DEVORDER;
    c->tune = tune_from_env();   // the one place the MKT_ROT_* / MKT_CCS_* environment is read; mkt_set_option afterwards
    DevGuard dg(device);
    auto bail = [&](int code) { std::string m = c->err; mkt_ctx_destroy(c); g_create_error = m; return code; };
    if (!dg.ok) { c->err = "hipSetDevice failed"; return bail(MKT_ERR_HIP); }
    const mkt_params &p = c->p;
    const int np = c->sh.nparty, M = c->M;
    c->ks->loaded.reset(np);
    mkt::make_twiddles(p.N, c->ks->tw);
    // rotation slots: KMS phase 1 runs 1 row for party 0 and l_lev rows for the others (bootstrapping.jl:400)
    std::vector<int> sp, sr;
    if (mkt::is_kms(p.scheme)) {
        for (int i = 0; i < p.k; i++) { int rows = i == 0 ? 1 : p.l_lev; for (int r = 0; r < rows; r++) { sp.push_back(i); sr.push_back(r); } }
    } else { sp.push_back(0); sr.push_back(0); }
    c->ks->rtot = (int)sp.size();
    describe_key_set(c);
    // the rotation kernels read a party's key rows through one buffer descriptor (kernel_common.h table_rsrc: 31-bit record
    // count, 32-bit row offsets); a larger key would read zeros silently, so it is refused here (largest shipped set: 0.25 GB)
    if (c->ks->stride(T_BRK) * sizeof(cplx) > 0x7fffffffull) { c->err = "per-party bootstrapping key exceeds the 2 GiB window of the rotation kernels' buffer descriptors"; return bail(MKT_ERR_UNSUPPORTED); }
#define CK(call) do { hipError_t _e = (call); if (_e != hipSuccess) { c->err = std::string(#call) + ": " + hipGetErrorString(_e); return bail(_e == hipErrorOutOfMemory ? MKT_ERR_NOMEM : MKT_ERR_HIP); } } while (0)
    for (int t = 0; t < T_COUNT; t++) if (c->ks->tab[t].present) {
        if (t == T_KSK_PLANES && c->ks->own[t].alloc(c->ks->tab[t].bytes(np)) != hipSuccess) { (void)hipGetLastError(); c->ks->tab[t].present = false; continue; }   // optional (describe_key_set)
        if (t != T_KSK_PLANES) CK(c->ks->own[t].alloc(c->ks->tab[t].bytes(np)));
        *c->ks->tab[t].slot = c->ks->own[t].p;
    }
    CK(hipMemcpy(c->ks->d_slot_party, sp.data(), sp.size() * sizeof(int), hipMemcpyHostToDevice));
    CK(hipMemcpy(c->ks->d_slot_row, sr.data(), sr.size() * sizeof(int), hipMemcpyHostToDevice));
    if (c->ks->d_fx_tab) {
        CK(hipMemset(c->ks->d_fx_stat, 0, 8));
        const size_t tb = (size_t)M * sizeof(cplx);
        CK(hipMemcpy(c->ks->d_fx_tab, c->ks->tw.fx_om.data(), tb, hipMemcpyHostToDevice));
        CK(hipMemcpy(c->ks->d_fx_tab + M, c->ks->tw.fx_tw.data(), tb, hipMemcpyHostToDevice));
        CK(hipMemcpy(c->ks->d_fx_tab + 2 * (size_t)M, c->ks->tw.fx_nat.data(), tb, hipMemcpyHostToDevice));
    }
#undef CK
    int r = upload_twiddles(c);
    if (!r && c->exact) r = upload_ntt_tables(c);
    if (!r) r = build_monomial(c);
    if (r) return bail(r);
    *out = c;
    return MKT_OK;
}

int mkt_ctx_destroy(mkt_ctx *c) {
    if (!c) return MKT_OK;
    DevGuard dg(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->own_stream && c->own_stream != c->stream) (void)hipStreamSynchronize(c->own_stream);   // before the workspace goes: work queued on the fork's own stream may still use it
    clear_spans(c);
    c->ws = Workspace();           // every owner lets go here: before the fork's stream and the key set
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->moved) (void)hipEventDestroy(c->moved);
    delete c;                      // drops this context's reference to the key set; the last one frees it
    return MKT_OK;
}

// A second context over the SAME resident keys and tables (no copy): own stream, own workspace, own timing -- one per
// concurrent caller / host thread / stream, as the reference's read-only scheme object is shared by concurrent
// bootstrapping! calls.  From the first fork on the key set is immutable (mkt_load_*, mkt_set_twiddles,
// mkt_keygen_device return MKT_ERR_STATE on every context that shares it).
int mkt_ctx_fork(mkt_ctx *c, mkt_ctx **out) {
    if (!c || !out) return fail(c, MKT_ERR_ARG, "null argument");
    auto *f = new mkt_ctx();
    f->p = c->p; f->sh = c->sh; f->device = c->device; f->logM = c->logM; f->logN = c->logN; f->M = c->M; f->dev_order = c->dev_order;
    f->ks = c->ks; f->exact = c->exact; f->split = c->split; f->tune = c->tune;
    // the fork's own stream: non-blocking, so forks driven from several host threads neither serialise on the NULL stream
    // nor against each other; mkt_set_stream may re-point the context at a caller's stream later
    {
        DevGuard dg(c->device);
        hipError_t e = hipStreamCreateWithFlags(&f->own_stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete f; return hipfail(c, e, "hipStreamCreateWithFlags(fork)"); }
        f->stream = f->own_stream;
    }
    *out = f;
    return MKT_OK;
}

// ---- internal (multi.cpp) ----
// The one device-to-device copy (the clone below, ShardArg::across in multi.cpp): hipMemcpyPeer (xGMI when the devices are linked; the runtime stages through the host otherwise); if the
// peer copy is refused or switched off, an explicit host bounce.  Returns a hipError_t value.  It does not synchronise: a peer copy may return before the data has landed, each caller drains what it has to.
int mkt_internal_copy_across(void *dst, int ddev, const void *src, int sdev, size_t bytes, int no_peer) {
    if (!bytes) return hipSuccess;
    if (!no_peer) {
        if (hipMemcpyPeer(dst, ddev, src, sdev, bytes) == hipSuccess) return hipSuccess;
        (void)hipGetLastError();
    }
    std::vector<unsigned char> bounce(bytes);
    hipError_t e;
    { DevGuard g(sdev); e = hipMemcpy(bounce.data(), src, bytes, hipMemcpyDeviceToHost); }
    if (e == hipSuccess) { DevGuard g(ddev); e = hipMemcpy(dst, bounce.data(), bytes, hipMemcpyHostToDevice); }
    return e;
}
// Replicate the resident, pre-transformed key set of `src` onto `dst`'s device.  dst is a fresh context of the same parameters and
// arithmetic on another device.  The key upload and its transforms run ONCE, on src's device ("optional one-time
// device-to-device key copy").
int mkt_internal_clone_keys(mkt_ctx *src, mkt_ctx *dst, int no_peer) {
    if (!src || !dst) return MKT_ERR_ARG;
    if (std::memcmp(&src->p, &dst->p, sizeof(mkt_params)) != 0 || src->exact != dst->exact) return fail(dst, MKT_ERR_ARG, "key replication between contexts of different parameters");
    if (int w = keys_writable(dst)) return w;
    { DevGuard g(src->device); HIPCHK(dst, hipStreamSynchronize(src->stream)); }
    const int sd = src->device, dd = dst->device;
    KeySet &a = *src->ks, &b = *dst->ks;
    b.tw = a.tw;   // tables a caller may have replaced on src (mkt_set_twiddles)
    // every table the two key sets both hold (the Float64-pipe copy of the key only where both contexts were created with it)
    for (int t = 0; t < T_COUNT; t++)
        if (a.tab[t].cloned && a.tab[t].present && b.tab[t].present)
            HIPCHK(dst, (hipError_t)mkt_internal_copy_across(*b.tab[t].slot, dd, *a.tab[t].slot, sd, a.tab[t].bytes(src->sh.nparty), no_peer));
    if (a.d_fx_brk && b.d_fx_brk) b.fx_kmax = a.fx_kmax;
    b.loaded = a.loaded;
    dst->tune = src->tune;
    // hipMemcpyPeer may return before the copy has landed, and the shards evaluate on non-blocking streams that the NULL stream does
    // not order: both devices are drained before the replica may be used (one-time cost, off the evaluation path)
    { DevGuard g(sd); HIPCHK(dst, hipDeviceSynchronize()); }
    { DevGuard g(dd); HIPCHK(dst, hipDeviceSynchronize()); }
    if (b.d_ksk_planes && !a.d_ksk_planes) {   // the optional planes: the source went without, the replica builds its own from the rows that have landed
        DevGuard g(dd);
        for (int party = 0; party < dst->sh.nparty; party++) if (b.loaded.has(mkt::K_KSK, party)) HIPCHK(dst, ksk_to_planes(dst, party));
        HIPCHK(dst, hipStreamSynchronize(dst->stream));
    }
    return MKT_OK;
}
// The host side of the matrix-core key switch, for the tests that need no device: the planes of one block from rows at the resident pitch
// (the function the device packer runs per byte), their size, the admission bound and MKT_KS_MFMA as the launcher reads it
size_t mkt_internal_ks_mfma_block_bytes(int N, int f, int n1p) { return mktd::ksm_block_bytes(N, f, n1p); }
void mkt_internal_ks_mfma_pack_host(const uint32_t *rows, int N, int f, int drows, int n1p, int8_t *planes) {
    const size_t bytes = mktd::ksm_block_bytes(N, f, n1p);
    for (size_t off = 0; off < bytes; off++) planes[off] = mktd::ksm_plane_byte(rows, N, f, drows, n1p, off);
}
int mkt_internal_ks_mfma_fits(long long N, long long kr, long long f) { return mkt::ks_mfma_fits(N, kr, f) ? 1 : 0; }
int mkt_internal_ks_mfma_env(void) { return env_int("MKT_KS_MFMA", -1); }   // what launch_tuning() reads, read again
// The launch rule of the key switch (kernels.hip ks_plan) for a set, a batch and the five switch values, no context and no device.
// set [10]: N, f, logD, drows, n1p, kacc, mk, balanced, planes present, scratch present; sw [5]: MKT_KS_G, _WAVES, _BLOCKS, _PAIR, _MFMA as read;
// out [9]: kernel (1 per-digit, 2 digit-pair, 3 matrix cores), G, waves, ngroups, parties, gblocks, slabs, digit words, partial words
void mkt_internal_ks_plan(const int *set, unsigned long long B, const int *sw, unsigned long long *out) {
    const mktd::KsShape a{set[0], set[1], set[2], set[3], set[4], set[5], set[6], set[7], set[8], set[9]};
    mktd::LaunchTuning lt{};
    lt.ks_g = sw[0]; lt.ks_waves = sw[1]; lt.ks_blocks = sw[2]; lt.ks_pair = sw[3]; lt.ks_mfma = sw[4];
    const mktd::KsReport r = mktd::ks_report(a, (size_t)B, lt);
    const unsigned long long v[9] = {(unsigned long long)r.kernel, (unsigned long long)r.G, (unsigned long long)r.waves, (unsigned long long)r.ngroups, (unsigned long long)r.parties,
                                     (unsigned long long)r.gblocks, (unsigned long long)r.slabs, r.digit_words, r.partial_words};
    for (int i = 0; i < 9; i++) out[i] = v[i];
}
#ifndef MKT_BUILD_ID
#define MKT_BUILD_ID "unknown"
#endif
const char *mkt_build_id(void) { return MKT_BUILD_ID; }
int mkt_internal_device_of(const mkt_ctx *c) { return c ? c->device : -1; }
size_t mkt_internal_lwe_len(const mkt_ctx *c) { return c ? (size_t)c->sh.lwe_len : 0; }
size_t mkt_internal_acc_bytes(const mkt_ctx *c) { return c ? (size_t)(1 + c->sh.kacc) * poly_bytes(c) : 0; }

// Calls on one context run in the order they were made, whatever stream each was enqueued on: the workspace is the context's, so the stream it moves to
// waits for everything enqueued on the stream it leaves (one event, recorded there).  Naming the stream it is on already costs nothing
int mkt_set_stream(mkt_ctx *c, void *hip_stream) {
    if (!c) return MKT_ERR_ARG;
    const hipStream_t next = (hipStream_t)hip_stream;
    if (next == c->stream) return MKT_OK;
    DevGuard dg(c->device);
    if (!c->moved) HIPCHK(c, hipEventCreateWithFlags(&c->moved, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->moved, c->stream));
    HIPCHK(c, hipStreamWaitEvent(next, c->moved, 0));
    c->stream = next;
    return MKT_OK;
}

int mkt_get_stream(mkt_ctx *c, void **hip_stream) { if (!c || !hip_stream) return MKT_ERR_ARG; *hip_stream = (void *)c->stream; return MKT_OK; }

// kernel-selection switches (parity tests force every kernel variant through this; A/B tools may seed them from the
// MKT_ROT_* / MKT_CCS_* environment, which is read once at mkt_ctx_create)
int mkt_set_option(mkt_ctx *c, const char *name, int value) {
    if (!c || !name) return fail(c, MKT_ERR_ARG, "null argument");
    const std::string k(name);
    for (const Switch &w : SWITCHES) {
        if (k != w.name) continue;
        if (!w.allowed.empty() && std::find(w.allowed.begin(), w.allowed.end(), value) == w.allowed.end()) {
            std::string list;
            for (int v : w.allowed) list += (list.empty() ? "" : ", ") + std::to_string(v);
            return fail(c, MKT_ERR_ARG, "mkt_set_option: " + k + " = " + std::to_string(value) + " is not one of " + list);
        }
        if (w.resets_workspace && c->tune.*w.member != value) c->ws.gates = 0;   // the next call allocates the rotation group anew (mkt::reserve_group), for the new route alone
        c->tune.*w.member = value;
        return MKT_OK;
    }
    return fail(c, MKT_ERR_ARG, "mkt_set_option: unknown option '" + k + "'");
}

const char *mkt_last_kernel_name(const mkt_ctx *c) { return c ? c->last_rot_kernel : ""; }

// diagnostics of the Float64-pipe EXACT implementation (fx_exact.hip): "fx_available" (1 if the loaded keys are certified and exact_impl admits it),
// "fx_bound" (proven bound on |computed - exact| of a rounded sum for the loaded keys), "fx_kmax" (largest |key transform value|); of the last
// mkt_exact_polymul_batch on this context: "fx_last_resid" (diagnostic), "polymul_amax" (max|a_i|), "fx_polymul_bound" (fx_polymul_bound, -1 if not evaluated);
// of the rotation launch that mkt_last_kernel_name names: "rot_static_l", "rot_static_logB" (its compile-time gadget, 0 = taken at run time);
// of the guard mode of device_mem.h (MKT_MEM_GUARD): "mem_guard_check" drains this context's device, compares the guards of every live guarded buffer of that
// device and gives the findings since the process started (the latest one's text: mkt_last_error), "mem_guard_buffers" the buffers that sweep looked at,
// "mem_guard_released" the guarded buffers compared at their release so far
int mkt_get_metric(mkt_ctx *c, const char *name, double *out) {
    if (!c || !name || !out) return fail(c, MKT_ERR_ARG, "null argument");
    const std::string k(name);
    if (k == "fx_available") *out = fx_usable(c) ? 1.0 : 0.0;
    else if (k == "ks_mfma") *out = mktd::launch_tuning().ks_mfma;          // MKT_KS_MFMA as read: negative automatic, 0 never, positive always where served
    else if (k == "ks_mfma_planes") *out = c->ks->d_ksk_planes ? 1.0 : 0.0; // the key set keeps the byte planes
    else if (k == "ks_mfma_last") *out = c->ks_mfma_last;                   // the last key switch on this context ran the matrix-core kernel
    else if (k == "ks_last_kernel") *out = c->ks_last.kernel;               // ... and its plan: 0 no key switch yet, 1 per-digit (keyswitch_mg_kernel), 2 digit-pair, 3 matrix cores
    else if (k == "ks_last_g") *out = c->ks_last.G;
    else if (k == "ks_last_waves") *out = c->ks_last.waves;
    else if (k == "ks_last_slabs") *out = c->ks_last.slabs;
    else if (k == "fx_bound") *out = c->ks->d_fx_brk ? fx_bound(c, c->ks->fx_kmax) : -1.0;
    else if (k == "fx_kmax") *out = c->ks->fx_kmax;
    else if (k == "fx_last_resid") *out = c->fx_last_resid;
    else if (k == "polymul_amax") *out = c->pm_amax;
    else if (k == "fx_polymul_bound") *out = c->pm_bound;
    else if (k == "rot_static_l") *out = c->rot_static_l;
    else if (k == "rot_static_logB") *out = c->rot_static_logB;
    else if (k == "mem_guard_check") {
        DevGuard dg(c->device);
        *out = (double)mkt::memguard::sweep(c->device);
        mkt::memguard::Finding f;
        if (mkt::memguard::last_finding(f)) c->err = mkt::memguard::text(f);
    }
    else if (k == "mem_guard_buffers") *out = (double)mkt::memguard::swept();
    else if (k == "mem_guard_released") *out = (double)mkt::memguard::released();
    else return fail(c, MKT_ERR_ARG, "mkt_get_metric: unknown metric '" + k + "'");
    return MKT_OK;
}

int mkt_synchronize(mkt_ctx *c) {
    if (!c) return MKT_ERR_ARG;
    DevGuard dg(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MKT_OK;
}

int mkt_get_twiddles(mkt_ctx *c, int which, double *out_host) {
    if (!c || !out_host || which < 0 || which > 3) return fail(c, MKT_ERR_ARG, "bad argument");
    MKT_F64_ONLY(c);
    DevGuard dg(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out_host, c->ks->d_tw + (size_t)which * c->M, (size_t)c->M * sizeof(cplx), hipMemcpyDeviceToHost));
    return MKT_OK;
}

int mkt_set_twiddles(mkt_ctx *c, const double *psi, const double *psiinv, const double *roots, const double *rootsinv) {
    if (!c || !psi || !psiinv || !roots || !rootsinv) return fail(c, MKT_ERR_ARG, "null table");
    MKT_F64_ONLY(c);
    if (int w = keys_writable(c)) return w;
    // tables first, then keys: a loaded bootstrapping key, relinearisation key, public key or CRS is resident as its transform under the tables
    // it met (or as the caller's Trans* values), and its integer form is not kept -- new tables would leave keys and transforms disagreeing
    if (c->ks->loaded.any_transformed() || c->ks->d_pack.p) return fail(c, MKT_ERR_STATE, "mkt_set_twiddles: install the tables before the keys (the loaded keys stay as they were transformed under the tables in place)");
    DevGuard dg(c->device);
    const size_t nd = (size_t)2 * c->M;
    // the kernels derive the inverse twiddles from the forward table: Psiinv must be conj(Psi) entry for entry,
    // which holds for the reference's tables (fft.jl:33-34: exp(-i*theta) and exp(+i*theta) of the same theta)
    for (int i = 1; i < c->M; i++)
        if (std::memcmp(&psi[2 * i], &psiinv[2 * i], 8) != 0 || psiinv[2 * i + 1] != -psi[2 * i + 1])
            return fail(c, MKT_ERR_ARG, "mkt_set_twiddles: Psiinv is not the conjugate of Psi");
    if (!twiddle_shape_ok(std::vector<double>(psi, psi + nd), c->M))   // checked BEFORE the host tables are replaced: a refused call leaves the context as it was
        return fail(c, MKT_ERR_ARG, "twiddle table Psi does not have the reference's shape (Psi[1] = (eps,-1), Psi[2] = (c,-c), Psi[3] = (-c,-c))");
    c->ks->tw.psi.assign(psi, psi + nd); c->ks->tw.psiinv.assign(psiinv, psiinv + nd);
    c->ks->tw.roots.assign(roots, roots + nd); c->ks->tw.rootsinv.assign(rootsinv, rootsinv + nd);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int r = upload_twiddles(c);
    if (r) return r;
    return build_monomial(c);   // the monomial table depends on the tables (scheme.jl:121-146)
}

int mkt_get_monomial(mkt_ctx *c, int e, double *out_host) {
    if (!c || !out_host || e < 1 || e > 2 * c->p.N) return fail(c, MKT_ERR_ARG, "bad argument");
    MKT_F64_ONLY(c);
    DevGuard dg(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<cplx> dev((size_t)c->M);
    HIPCHK(c, hipMemcpy(dev.data(), c->ks->d_monomial + (size_t)(e - 1) * c->M, (size_t)c->M * sizeof(cplx), hipMemcpyDeviceToHost));
    const int NT = c->M >> MKT_LOGR;              // device order -> the reference's order
    cplx *o = reinterpret_cast<cplx *>(out_host);
    for (int x = 0; x < c->M; x++) o[x] = dev[(size_t)mktd::dev_pos(c->dev_order, x, NT)];
    return MKT_OK;
}

int mkt_load_brk(mkt_ctx *c, int party, const void *data, int fmt) {
    if (int r = key_write_guard(c, data != nullptr, party, Gate::EXACT)) return r;
    DevGuard dg(c->device);
    int r = upload_polys(c, data, mkt::brk_polys_total(c->p, c->sh), c->ks->party<cplx>(T_BRK, party), fmt, false, party);
    if (!r && fmt != MKT_FMT_INT_COEFF) c->ks->loaded.mark(mkt::K_BRK, party);   // the caller's transforms, reordered only; install_brk marks a key it installed
    return r;
}

// on the context's stream like every other key load (mktfhe.h), and drained before the call returns: `data` is the caller's
int mkt_load_ksk(mkt_ctx *c, int party, const uint32_t *data) {
    if (int r = key_write_guard(c, data != nullptr, party, Gate::EXACT)) return r;
    DevGuard dg(c->device);
    HIPCHK(c, ksk_zero(c, party));
    HIPCHK(c, ksk_to_resident(c, party, data, hipMemcpyHostToDevice));
    HIPCHK(c, ksk_to_planes(c, party));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ks->loaded.mark(mkt::K_KSK, party);
    return MKT_OK;
}

int mkt_load_rlk(mkt_ctx *c, int party, const void *d, const void *f, int fmt) {
    if (int r = key_write_guard(c, d && f, party, Gate::F64_OR_EXACT_KMS, mkt::is_kms)) return r;
    DevGuard dg(c->device);
    const size_t l = (size_t)c->p.l_uni;
    int r = upload_polys(c, d, l, c->ks->party<cplx>(T_RLK_D, party), fmt);
    if (!r) r = upload_polys(c, f, 2 * l, c->ks->party<cplx>(T_RLK_F, party), fmt);
    if (!r) c->ks->loaded.mark(mkt::K_RLK, party);
    return r;
}

int mkt_load_pubkey(mkt_ctx *c, int party, const void *b, int fmt) {
    if (int r = key_write_guard(c, b != nullptr, party, Gate::F64_OR_EXACT_KMS, mkt::is_mk)) return r;
    DevGuard dg(c->device);
    int r = upload_polys(c, b, (size_t)c->p.l_uni, c->ks->party<cplx>(T_PUB, party), fmt);
    if (!r) c->ks->loaded.mark(mkt::K_PUB, party);
    return r;
}

int mkt_load_crs(mkt_ctx *c, const void *a, int fmt) {
    if (int r = key_write_guard(c, a != nullptr, NO_PARTY, Gate::F64_OR_EXACT_KMS, mkt::is_mk)) return r;
    DevGuard dg(c->device);
    int r = upload_polys(c, a, (size_t)c->p.l_uni, c->ks->d_crs, fmt);
    if (!r) c->ks->loaded.mark(mkt::K_CRS, NO_PARTY);
    return r;
}

// Bootstrapping key and key-switching key of party `party` generated on the device from the party's secrets
// (keygen.hip: the seeded streams of mkt_client_party_keygen, identical words), pre-transformed in place of an upload.
static int keygen_device_impl(mkt_ctx *c, int party, const mkt_client_party *K, const void *crs, void *brk_out, uint32_t *ksk_out) {
    if (int r = key_write_guard(c, K != nullptr, party, Gate::EXACT)) return r;
    if (int r = party_call_guard(c, "mkt_keygen_device", true, party, K)) return r;
    const mkt_params &p = c->p;
    const bool unienc = p.scheme == MKT_CCS;
    if (unienc && !crs) return fail(c, MKT_ERR_ARG, "mkt_keygen_device: CCS needs the integer CRS");
    DevGuard dg(c->device);
    const size_t brk_bytes = mkt::brk_polys_total(p, c->sh) * poly_bytes(c);
    DevBuf out, crs_int;                      // freed behind the secrets' drain of the stream
    DeviceSecret lwe{c}, z{c};
    mktd::KeygenArgs a{};
    hipError_t e = keygen_setup(c, K, crs, lwe, z, {{&out, brk_bytes}}, crs_int, a);
    if (e != hipSuccess) return hipfail(c, e, "device keygen setup");
    a.out = out.p; a.zoff = 0;
    if (!ring_keys_cover(c, K)) e = hipErrorInvalidValue;
    if (e == hipSuccess) e = mktd::launch_keygen_brk(a, unienc ? 1 : 0, c->stream);
    if (e == hipSuccess && brk_out) e = hipMemcpyAsync(brk_out, out.p, brk_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = install_brk(c, party, out.p);
    if (e == hipSuccess) e = ksk_zero(c, party);
    a.zoff = mkt::is_kms(p.scheme) ? 1 : 0;      // the key switch targets the uni key of the KMS schemes
    if (e == hipSuccess) e = mktd::launch_keygen_ksk(a, c->ks->party<uint32_t>(T_KSK, party), c->ks->ksk.n1p, c->sh.ksk_kr, c->sh.ksk_drows, mkt::is_block(p.scheme) ? 1 : 0, c->stream);
    if (e == hipSuccess) e = ksk_to_planes(c, party);
    e = wipe_secrets(wipe_secrets(e, z, a), lwe, a);
    if (e != hipSuccess) return hipfail(c, e, "device keygen");
    c->ks->loaded.mark(mkt::K_KSK, party);
    if (ksk_out) return mkt_get_ksk(c, party, ksk_out);
    return MKT_OK;
}

int mkt_keygen_device(mkt_ctx *c, int party, const mkt_client_party *K, const void *crs) {
    return keygen_device_impl(c, party, K, crs, nullptr, nullptr);
}

// the same, and the generated keys are also copied out in the host layouts of mkt_load_brk (MKT_FMT_INT_COEFF) /
// mkt_load_ksk: a party generates its evaluation keys on its OWN GPU and ships them (key blob) to the evaluator,
// which never sees a secret
int mkt_keygen_device_export(mkt_ctx *c, int party, const mkt_client_party *K, const void *crs, void *brk_out, uint32_t *ksk_out) {
    if (!brk_out || !ksk_out) return fail(c, MKT_ERR_ARG, "null output");
    return keygen_device_impl(c, party, K, crs, brk_out, ksk_out);
}

// Distributed decryption (mktfhe.h): party `party`'s shares of B rows on this context's device -- a party-local call like
// mkt_keygen_device, on a context that needs no evaluation key.  The n key words are uploaded for the call and wiped before they are freed.
int mkt_partial_decrypt_batch(mkt_ctx *c, int party, const mkt_client_party *K, const uint32_t *lwe, double sigma_smudge, const uint8_t *seed,
                              uint64_t row0, uint32_t *share_out, size_t B, int mem) {
    if (int r = party_call_guard(c, "mkt_partial_decrypt_batch", lwe && share_out && mem_ok(mem), party, K)) return r;
    if (!mkt::smudge_sigma_ok(sigma_smudge)) return fail(c, MKT_ERR_ARG, "mkt_partial_decrypt_batch: sigma_smudge must be finite, 0 <= sigma_smudge <= 2^31");
    const mkt_params &p = c->p;
    if (!B) return MKT_OK;
    DevGuard dg(c->device);
    Timer whole(c, 0);
    Staged sx{c}, so{c};
    DeviceSecret key{c};
    int r;
    if ((r = sx.in(lwe, B * (size_t)c->sh.lwe_len * 4, mem, true)) || (r = so.in(share_out, B * 4, mem, false))) return r;
    mktd::PartialDecryptArgs a{};
    if (mkt::seed_to_key(seed, a.key)) return fail(c, MKT_ERR_STATE, "mkt_partial_decrypt_batch: no entropy from the OS");
    hipError_t e = key.in(K->lwekey.data(), (size_t)p.n * 4);
    a.party = party; a.n = p.n; a.lwe_stride = c->sh.lwe_len; a.sigma = sigma_smudge; a.row0 = row0;
    a.lwe = sx.as<const uint32_t>(); a.lwekey = key.as<const uint32_t>(); a.out = so.as<uint32_t>(); a.B = B;
    if (e == hipSuccess) e = mktd::launch_partial_decrypt(a, c->stream);
    e = wipe_secrets(e, key, a);
    if (e != hipSuccess) return hipfail(c, e, "device partial decryption");
    return so.out(share_out);
}

// Seeded ciphertexts (mktfhe.h): the evaluator's call -- a public seed and B body words in, B ordinary rows out.  No key of any kind.
int mkt_seeded_expand_batch(mkt_ctx *c, int party, const uint8_t *mask_seed, uint64_t row0, const uint32_t *body, uint32_t *out, size_t B, int mem) {
    if (!c || !mask_seed || !mem_ok(mem) || party < 0 || party >= c->sh.nparty) return fail(c, MKT_ERR_ARG, "bad argument");
    if (!B) return MKT_OK;
    if (!body || !out) return fail(c, MKT_ERR_ARG, "bad argument");
    DevGuard dg(c->device);
    Timer whole(c, 0);
    Staged sb{c}, so{c};
    int r;
    if ((r = sb.in(body, B * 4, mem, true)) || (r = so.in(out, B * (size_t)c->sh.lwe_len * 4, mem, false))) return r;
    mktd::SeededArgs a{};
    mkt::seed_to_key(mask_seed, a.mkey);
    a.party = party; a.n = c->p.n; a.lwe_len = c->sh.lwe_len; a.row0 = row0;
    a.in = sb.as<const uint32_t>(); a.out = so.as<uint32_t>(); a.B = B;
    HIPCHK(c, mktd::launch_seeded_expand(a, c->stream));
    return so.out(out);
}

// the party's call, party-local like mkt_partial_decrypt_batch: the n key words are uploaded for the call and wiped before they are freed
int mkt_seeded_encrypt_batch(mkt_ctx *c, int party, const mkt_client_party *K, const uint32_t *mu, double sigma_lwe, const uint8_t *mask_seed,
                             const uint8_t *noise_seed, uint64_t row0, uint32_t *body_out, size_t B, int mem) {
    if (int r = party_call_guard(c, "mkt_seeded_encrypt_batch", mask_seed && mem_ok(mem), party, K)) return r;
    if (!mkt::smudge_sigma_ok(sigma_lwe)) return fail(c, MKT_ERR_ARG, "mkt_seeded_encrypt_batch: sigma_lwe must be finite, 0 <= sigma_lwe <= 2^31");
    if (noise_seed && std::memcmp(noise_seed, mask_seed, 32) == 0) return fail(c, MKT_ERR_ARG, "mkt_seeded_encrypt_batch: the noise seed is the public mask seed");
    const mkt_params &p = c->p;
    if (!B) return MKT_OK;
    if (!mu || !body_out) return fail(c, MKT_ERR_ARG, "bad argument");
    DevGuard dg(c->device);
    Timer whole(c, 0);
    Staged sx{c}, so{c};
    DeviceSecret key{c};
    int r;
    if ((r = sx.in(mu, B * 4, mem, true)) || (r = so.in(body_out, B * 4, mem, false))) return r;
    mktd::SeededArgs a{};
    mkt::seed_to_key(mask_seed, a.mkey);
    if (mkt::seed_to_key(noise_seed, a.nkey)) return fail(c, MKT_ERR_STATE, "mkt_seeded_encrypt_batch: no entropy from the OS");
    hipError_t e = key.in(K->lwekey.data(), (size_t)p.n * 4);
    a.party = party; a.n = p.n; a.lwe_len = c->sh.lwe_len; a.sigma = sigma_lwe; a.row0 = row0;
    a.in = sx.as<const uint32_t>(); a.lwekey = key.as<const uint32_t>(); a.out = so.as<uint32_t>(); a.B = B;
    if (e == hipSuccess) e = mktd::launch_seeded_encrypt(a, c->stream);
    e = wipe_secrets(e, key, a);
    if (e != hipSuccess) return hipfail(c, e, "device seeded encryption");
    return so.out(body_out);
}

// Seeded evaluation keys (mktfhe.h): party `party`'s two large keys regenerated on this context's device from the public mask seed and the
// compact sections (seeded_keys.hip), the words of mkt_client_seeded_keys_expand.  load: into the resident tables -- the bootstrapping key
// expanded into a coefficient-form buffer and installed like every other (install_brk), the key-switching key straight into its
// table at the padded pitch; else into the caller's brk_out / ksk_out (`mem`), the compact sections living there too.  Nothing is secret.
// `mem` says where the compact sections live in either case: MKT_MEM_DEVICE sections are read where they are, not staged -- the bodies
// mkt_keygen_device_seeded has just generated on this device are installed from there.
static int seeded_keys_impl(mkt_ctx *c, int party, const uint8_t *mask_seed, const void *brk_seeded, const uint32_t *ksk_seeded, bool load,
                            void *brk_out, uint32_t *ksk_out, int mem) {
    if (!c || !mask_seed || !mem_ok(mem) || party < 0 || party >= c->sh.nparty) return fail(c, MKT_ERR_ARG, "bad argument");
    if (!load && (!brk_seeded != !brk_out || !ksk_seeded != !ksk_out)) return fail(c, MKT_ERR_ARG, "mkt_seeded_keys_expand: a compact section and its output come together");
    const mkt_params &p = c->p;
    DevGuard dg(c->device);
    const size_t body_polys = mkt::brk_seeded_polys(p, c->sh), brk_polys_total = mkt::brk_polys_total(p, c->sh), rows = c->ks->ksk.rows;
    Staged sb{c}, sk{c}, so{c};
    DevBuf full, padded;                    // load: the expanded bootstrapping key in coefficient form; expand: the key-switching key at the padded pitch
    int r;
    hipError_t e = hipSuccess;
    if (brk_seeded) {
        // seeded_brk_expand_kernel copies bodies and writes polynomials 16 bytes at a time, from the base pointers on: both refused here, before any launch, unless so aligned
        if ((r = sb.in(brk_seeded, body_polys * poly_bytes(c), mem, true, 16))) return r;
        void *dst;
        if (load) { HIPCHK(c, full.alloc(brk_polys_total * poly_bytes(c))); dst = full.p; }
        else { if ((r = so.in(brk_out, brk_polys_total * poly_bytes(c), mem, false, 16))) return r; dst = so.dev; }
        mktd::SeededBrkArgs a{};
        mkt::seed_to_key(mask_seed, a.mkey);
        a.stream = mktrng::STREAM_BRK_MASK; a.party = party; a.unienc = p.scheme == MKT_CCS; a.kr = c->sh.kr; a.l = a.unienc ? p.l_uni : p.l_gsw;
        a.log_units = c->logN + (p.W == 64 ? 1 : 0) - 4; a.body = sb.dev; a.out = dst; a.npolys = brk_polys_total;
        e = mktd::launch_seeded_brk_expand(a, c->stream);
        if (e == hipSuccess && load) e = install_brk(c, party, dst);
        if (e != hipSuccess) return hipfail(c, e, "seeded bootstrapping key expansion");
    }
    if (ksk_seeded) {
        if ((r = sk.in(ksk_seeded, rows * 4, mem, true))) return r;
        uint32_t *dst = c->ks->party<uint32_t>(T_KSK, party);
        if (!load) { HIPCHK(c, padded.alloc(c->ks->ksk.resident_words() * 4)); dst = padded.as<uint32_t>(); }
        mktd::SeededKskArgs a{};
        mkt::seed_to_key(mask_seed, a.mkey);
        a.party = party; a.n = p.n; a.n1p = c->ks->ksk.n1p; a.rows_per_cj = (uint32_t)(c->sh.ksk_drows * p.f);
        a.absent_below = mkt::is_block(p.scheme) ? p.n : 0; a.body = sk.as<const uint32_t>(); a.out = dst; a.rows = rows;
        e = mktd::launch_seeded_ksk_expand(a, c->stream);
        if (e == hipSuccess && !load) e = ksk_to_rows(c, dst, ksk_out, mem == MKT_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
        if (e == hipSuccess && load) e = ksk_to_planes(c, party);
        if (e != hipSuccess) return hipfail(c, e, "seeded key-switching key expansion");
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!load) return brk_out ? so.out(brk_out) : MKT_OK;
    if (ksk_seeded) c->ks->loaded.mark(mkt::K_KSK, party);
    return MKT_OK;
}

int mkt_seeded_keys_expand(mkt_ctx *c, int party, const uint8_t *mask_seed, const void *brk_seeded, const uint32_t *ksk_seeded, void *brk_out, uint32_t *ksk_out, int mem) {
    return seeded_keys_impl(c, party, mask_seed, brk_seeded, ksk_seeded, false, brk_out, ksk_out, mem);
}

int mkt_load_seeded_keys(mkt_ctx *c, int party, const uint8_t *mask_seed, const void *brk_seeded, const uint32_t *ksk_seeded) {
    if (int r = key_write_guard(c, brk_seeded || ksk_seeded, NO_PARTY, Gate::EXACT)) return r;   // (the party and the seed: seeded_keys_impl)
    return seeded_keys_impl(c, party, mask_seed, brk_seeded, ksk_seeded, true, nullptr, nullptr, MKT_MEM_HOST);
}

// The seeded key form generated on the party's own GPU (keygen_seeded.hip): the compact sections of mkt_client_party_keygen_seeded for the seed
// `K` was made from, word for word, the large keys never expanded.  install: the sections, still on the device, also go through the
// expansion and install of mkt_load_seeded_keys.  Party-local like mkt_keygen_device: the secrets are wiped before they are freed.
int mkt_keygen_device_seeded(mkt_ctx *c, int party, const mkt_client_party *K, const void *crs, const uint8_t *mask_seed, void *brk_seeded_out,
                             uint32_t *ksk_seeded_out, int install) {
    if (int r = party_call_guard(c, "mkt_keygen_device_seeded", mask_seed != nullptr, party, K)) return r;
    if (!brk_seeded_out != !ksk_seeded_out) return fail(c, MKT_ERR_ARG, "mkt_keygen_device_seeded: the two compact outputs come together");
    if (!brk_seeded_out && !install) return fail(c, MKT_ERR_ARG, "mkt_keygen_device_seeded: neither an output nor an install was asked for");
    const mkt_params &p = c->p;
    const bool unienc = p.scheme == MKT_CCS;
    if (unienc && !crs) return fail(c, MKT_ERR_ARG, "mkt_keygen_device_seeded: CCS needs the integer CRS");
    // (the stream key is the seed's 32 bytes as eight little-endian words, seed_to_key: compared where it lies, no copy of it made)
    if (std::memcmp(mask_seed, K->key, sizeof K->key) == 0) return fail(c, MKT_ERR_ARG, "mkt_keygen_device_seeded: the mask seed is the party's secret seed (it is published: the secrets would be too)");
    if (install) if (int r = key_write_guard(c, true, party, Gate::EXACT)) return r;
    DevGuard dg(c->device);
    const size_t brk_bytes = mkt::brk_seeded_polys(p, c->sh) * poly_bytes(c), rows = c->ks->ksk.rows;
    DevBuf bodies, words, crs_int;            // freed behind the secrets' drain of the stream
    DeviceSecret lwe{c}, z{c};
    mktd::KeygenSeededArgs a{};
    hipError_t e = keygen_setup(c, K, crs, lwe, z, {{&bodies, brk_bytes}, {&words, rows * 4}}, crs_int, a);
    if (e != hipSuccess) return hipfail(c, e, "device seeded keygen setup");
    mkt::seed_to_key(mask_seed, a.mkey);
    a.brk_body = bodies.p; a.ksk_body = words.as<uint32_t>(); a.ksk_rows = rows;
    a.drows = c->sh.ksk_drows; a.absent_below = mkt::is_block(p.scheme) ? p.n : 0;
    a.zoff = mkt::is_kms(p.scheme) ? 1 : 0;      // the key switch targets the uni key of the KMS schemes
    if (!ring_keys_cover(c, K)) e = hipErrorInvalidValue;
    if (e == hipSuccess) e = mktd::launch_keygen_seeded_brk(a, unienc ? 1 : 0, c->stream);
    if (e == hipSuccess) e = mktd::launch_keygen_seeded_ksk(a, c->stream);
    if (e == hipSuccess && brk_seeded_out) e = hipMemcpyAsync(brk_seeded_out, bodies.p, brk_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && ksk_seeded_out) e = hipMemcpyAsync(ksk_seeded_out, words.p, rows * 4, hipMemcpyDeviceToHost, c->stream);
    e = wipe_secrets(wipe_secrets(e, z, a), lwe, a);       // (drains the stream: the outputs have landed)
    if (e != hipSuccess) return hipfail(c, e, "device seeded keygen");
    if (!install) return MKT_OK;
    return seeded_keys_impl(c, party, mask_seed, bodies.p, words.as<const uint32_t>(), true, nullptr, nullptr, MKT_MEM_DEVICE);
}

// debug / test read-back of a party's key-switching key in the host layout of mkt_load_ksk
int mkt_get_ksk(mkt_ctx *c, int party, uint32_t *out_host) {
    if (!c || !out_host || party < 0 || party >= c->sh.nparty) return fail(c, MKT_ERR_ARG, "bad argument");
    MKT_EXACT_GATE(c);
    DevGuard dg(c->device);
    HIPCHK(c, ksk_to_rows(c, c->ks->party<uint32_t>(T_KSK, party), out_host, hipMemcpyDeviceToHost));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MKT_OK;
}

// ---- batched hot path ----

// the gate entry points share one body: `op` for the whole batch or per-gate `ops`; `arity` (2 or 3) operands in batch order (v[i]:
// [B][len]) or picked by row index iv[i] from a pool (v[0] = pool, [rows][len]); arity 3 = the three-input linear part in one bootstrap
static int gate_impl(mkt_ctx *c, int arity, int op, const uint8_t *ops, const uint32_t *const *v, size_t rows, const uint32_t *const *iv,
                     uint32_t *out, size_t B, int mem) {
    MKT_EXACT_GATE(c);
    int r;
    if ((r = check_ready(c, true, true))) return r;
    DevGuard dg(c->device);
    Timer whole(c, 0);
    const size_t len = (size_t)c->sh.lwe_len;
    const bool pool = iv != nullptr;
    Staged sv[3]{{c}, {c}, {c}}, so{c}, sops{c}, si[3]{{c}, {c}, {c}};
    for (int i = 0; i < (pool ? 1 : arity); i++) if ((r = sv[i].in(v[i], rows * len * 4, mem, true))) return r;
    if ((r = so.in(out, B * len * 4, mem, false))) return r;
    if (ops && (r = sops.in(ops, B, mem, true))) return r;
    for (int i = 0; pool && i < arity; i++) if ((r = si[i].in(iv[i], B * 4, mem, true))) return r;
    for (size_t off = 0; off < B; off += CHUNK_GATES) {
        const size_t nb = std::min(CHUNK_GATES, B - off);
        if ((r = ensure_workspace(c, nb))) return r;
        uint32_t *const ws_lin = c->ws.lin.as<uint32_t>();
        const uint8_t *o = ops ? sops.as<const uint8_t>() + off : nullptr;
        const uint32_t *d[3] = {}, *di[3] = {};
        for (int i = 0; i < arity; i++) {
            d[i] = pool ? sv[0].as<const uint32_t>() : sv[i].as<const uint32_t>() + off * len;
            di[i] = pool ? si[i].as<const uint32_t>() + off : nullptr;
        }
        const size_t prows = pool ? rows : 0;
        HIPCHK(c, arity == 2 ? mktd::launch_gate_linear(op, o, d[0], d[1], di[0], di[1], prows, ws_lin, (int)len, nb, c->stream)
                             : mktd::launch_gate3_linear(o, d[0], d[1], d[2], di[0], di[1], di[2], prows, ws_lin, (int)len, nb, c->stream));
        if ((r = bootstrap_chunk(c, ws_lin, so.as<uint32_t>() + off * len, nb))) return r;
    }
    return so.out(out);
}

// host arrays only (a device array is not read back): every code's gate (bits 0-2) at most `max_code`, no bit outside `flags` above them
static bool codes_valid_host(const uint8_t *ops, size_t B, unsigned max_code, unsigned flags) {
    for (size_t j = 0; j < B; j++) if ((ops[j] & 7u) > max_code || (ops[j] & ~(7u | flags))) return false;
    return true;
}

// host arrays only: every entry of the n index arrays idx[i][0 .. B) names a row of the pool
static bool in_pool_host(const uint32_t *const *idx, int n, size_t B, size_t pool_rows) {
    for (int i = 0; i < n; i++) for (size_t j = 0; j < B; j++) if (idx[i][j] >= pool_rows) return false;
    return true;
}

int mkt_gate_batch(mkt_ctx *c, int op, const uint32_t *x, const uint32_t *y, uint32_t *out, size_t B, int mem) {
    if (!c || !x || !y || !out || !mem_ok(mem) || op < MKT_NAND || op > MKT_NOR) return fail(c, MKT_ERR_ARG, "bad argument");
    const uint32_t *v[] = {x, y};
    return gate_impl(c, 2, op, nullptr, v, B, nullptr, out, B, mem);
}

// a different gate per ciphertext pair -- the shape of the reference's own tests (test/KMS.jl:29-34 draws a random gate per step;
// gate.jl:1-53) -- in ONE launch sequence: ops[j] = MKT_NAND .. MKT_NOR, optionally | MKT_OP_NOT_X / MKT_OP_NOT_Y
int mkt_gate_batch_ops(mkt_ctx *c, const uint8_t *ops, const uint32_t *x, const uint32_t *y, uint32_t *out, size_t B, int mem) {
    if (!c || !ops || !x || !y || !out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    if (mem == MKT_MEM_HOST && !codes_valid_host(ops, B, MKT_NOR, MKT_OP_NOT_X | MKT_OP_NOT_Y)) return fail(c, MKT_ERR_ARG, "mkt_gate_batch_ops: unknown gate code");
    const uint32_t *v[] = {x, y};
    return gate_impl(c, 2, 0, ops, v, B, nullptr, out, B, mem);
}

// one circuit level: gate j reads pool[ix[j]] and pool[iy[j]] (rows of [pool_rows][k*n+1]) and writes out[j]; `out` may be a
// later region of the same pool as long as no gate of THIS call reads a row this call writes
int mkt_gate_batch_gather(mkt_ctx *c, const uint8_t *ops, const uint32_t *pool, size_t pool_rows, const uint32_t *ix, const uint32_t *iy,
                          uint32_t *out, size_t B, int mem) {
    if (!c || !ops || !pool || !ix || !iy || !out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    if (B && !pool_rows) return fail(c, MKT_ERR_ARG, "mkt_gate_batch_gather: gates over an empty pool");     // (the kernel clamps indices into [0, pool_rows): there must be a row to clamp to, in either memory kind)
    const uint32_t *v[] = {pool}, *iv[] = {ix, iy};
    if (mem == MKT_MEM_HOST) {
        if (!codes_valid_host(ops, B, MKT_NOR, MKT_OP_NOT_X | MKT_OP_NOT_Y)) return fail(c, MKT_ERR_ARG, "mkt_gate_batch_gather: unknown gate code");
        if (!in_pool_host(iv, 2, B, pool_rows)) return fail(c, MKT_ERR_ARG, "mkt_gate_batch_gather: operand index outside the pool");
    }
    return gate_impl(c, 2, 0, ops, v, pool_rows, iv, out, B, mem);
}

// three-input gates in one bootstrap (every scheme, both arithmetic modes): operands in batch order (x, y, z: [B][len]) or picked by
// row index from a pool
int mkt_gate3_batch_ops(mkt_ctx *c, const uint8_t *ops, const uint32_t *x, const uint32_t *y, const uint32_t *z, uint32_t *out, size_t B, int mem) {
    if (!c || !ops || !x || !y || !z || !out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    if (mem == MKT_MEM_HOST && !codes_valid_host(ops, B, MKT_AE3, MKT_OP_NOT_X | MKT_OP_NOT_Y | MKT_OP_NOT_Z)) return fail(c, MKT_ERR_ARG, "mkt_gate3_batch_ops: unknown gate code");
    const uint32_t *v[] = {x, y, z};
    return gate_impl(c, 3, 0, ops, v, B, nullptr, out, B, mem);
}

int mkt_gate3_batch_gather(mkt_ctx *c, const uint8_t *ops, const uint32_t *pool, size_t pool_rows, const uint32_t *ix, const uint32_t *iy, const uint32_t *iz,
                           uint32_t *out, size_t B, int mem) {
    if (!c || !ops || !pool || !ix || !iy || !iz || !out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    if (B && !pool_rows) return fail(c, MKT_ERR_ARG, "mkt_gate3_batch_gather: gates over an empty pool");
    const uint32_t *v[] = {pool}, *iv[] = {ix, iy, iz};
    if (mem == MKT_MEM_HOST) {
        if (!codes_valid_host(ops, B, MKT_AE3, MKT_OP_NOT_X | MKT_OP_NOT_Y | MKT_OP_NOT_Z)) return fail(c, MKT_ERR_ARG, "mkt_gate3_batch_gather: unknown gate code");
        if (!in_pool_host(iv, 3, B, pool_rows)) return fail(c, MKT_ERR_ARG, "mkt_gate3_batch_gather: operand index outside the pool");
    }
    return gate_impl(c, 3, 0, ops, v, pool_rows, iv, out, B, mem);
}

// MUX(s, a, b) = s ? a : b with TWO blind rotations and ONE key switch (the reference has no MUX gate, gate.jl:1-57; this is the
// CGGI16 construction written with the reference's own operators):
//   acc = blindrotate!(AND-linear(s, a)) + blindrotate!(AND-linear(NOT! s, b)), + 1/8 at X^0 of acc.b;  out = keyswitch!(acc)
// Each rotation leaves +-1/8 and at most one of the two ANDs holds, so the sum + 1/8 is +-1/8 again.  A composite of the
// reference's gates, OR(AND(s, a), AND(NOT s, b)), costs three full bootstraps.
// Both entry points share one body: operands v = (s, a, b) in batch order ([B][len]), or picked by row index iv[i] from a pool
// (v[0] = pool, [rows][len]) with the optional per-gate negations not_ab
static int mux_impl(mkt_ctx *c, const uint32_t *const *v, size_t rows, const uint32_t *const *iv, const uint8_t *not_ab, uint32_t *out, size_t B, int mem) {
    MKT_EXACT_GATE(c);
    int r;
    if ((r = check_ready(c, true, true))) return r;
    DevGuard dg(c->device);
    Timer whole(c, 0);
    const size_t len = (size_t)c->sh.lwe_len, words = (size_t)(1 + c->sh.kacc) * c->p.N;
    const bool pool = iv != nullptr;
    Staged sv[3]{{c}, {c}, {c}}, si[3]{{c}, {c}, {c}}, so{c}, sf{c};
    for (int i = 0; i < (pool ? 1 : 3); i++) if ((r = sv[i].in(v[i], rows * len * 4, mem, true))) return r;
    for (int i = 0; pool && i < 3; i++) if ((r = si[i].in(iv[i], B * 4, mem, true))) return r;
    if ((r = so.in(out, B * len * 4, mem, false))) return r;
    if (not_ab && (r = sf.in(not_ab, B, mem, true))) return r;
    constexpr size_t HALF = CHUNK_GATES / 2;                  // two rotations per gate share the workspace chunk
    for (size_t off = 0; off < B; off += HALF) {
        const size_t nb = std::min(HALF, B - off);
        if ((r = ensure_workspace(c, 2 * nb))) return r;
        uint32_t *const ws_lin = c->ws.lin.as<uint32_t>();
        if (pool) {
            HIPCHK(c, mktd::launch_mux_linear(sv[0].as<const uint32_t>(), rows, si[0].as<const uint32_t>() + off, si[1].as<const uint32_t>() + off, si[2].as<const uint32_t>() + off,
                                              not_ab ? sf.as<const uint8_t>() + off : nullptr, ws_lin, (int)len, nb, c->stream));
        } else {
            const uint32_t *ps = sv[0].as<const uint32_t>() + off * len;
            HIPCHK(c, mktd::launch_gate_linear(MKT_AND, nullptr, ps, sv[1].as<const uint32_t>() + off * len, nullptr, nullptr, 0, ws_lin, (int)len, nb, c->stream));
            HIPCHK(c, mktd::launch_gate_linear(MKT_AND | MKT_OP_NOT_X, nullptr, ps, sv[2].as<const uint32_t>() + off * len, nullptr, nullptr, 0, ws_lin + nb * len, (int)len, nb, c->stream));
        }
        if ((r = rotate_chunk(c, ws_lin, 2 * nb))) return r;
        HIPCHK(c, mktd::launch_mux_combine(c->p.W, c->ws.acc.p, nb, words, c->stream));
        if ((r = do_keyswitch(c, c->ws.acc.p, so.as<uint32_t>() + off * len, nb))) return r;
    }
    return so.out(out);
}

int mkt_mux_batch(mkt_ctx *c, const uint32_t *sel, const uint32_t *a, const uint32_t *b, uint32_t *out, size_t B, int mem) {
    if (!c || !sel || !a || !b || !out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    const uint32_t *v[] = {sel, a, b};
    return mux_impl(c, v, B, nullptr, nullptr, out, B, mem);
}

// the same MUX with its operands picked by row index from a ciphertext pool (a circuit level of MUX gates): gate j = MUX(pool[is[j]],
// pool[ia[j]], pool[ib[j]]) -> out[j]; out may be a later region of the pool that no gate of this call reads
// not_ab (optional, lives where the indices live): bit 0 / bit 1 of not_ab[j] = the a / b operand of gate j is negated first (a circuit's
// free NOTs; a negated SELECTOR is the caller swapping a and b)
int mkt_mux_batch_gather(mkt_ctx *c, const uint32_t *pool, size_t pool_rows, const uint32_t *is, const uint32_t *ia, const uint32_t *ib, const uint8_t *not_ab,
                         uint32_t *out, size_t B, int mem) {
    if (!c || !pool || !is || !ia || !ib || !out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    if (B && !pool_rows) return fail(c, MKT_ERR_ARG, "mkt_mux_batch_gather: gates over an empty pool");
    const uint32_t *v[] = {pool}, *iv[] = {is, ia, ib};
    if (mem == MKT_MEM_HOST && (!in_pool_host(iv, 3, B, pool_rows) || (not_ab && !codes_valid_host(not_ab, B, 3, 0))))   // not_ab[j] in 0 .. 3
        return fail(c, MKT_ERR_ARG, "mkt_mux_batch_gather: operand index outside the pool, or unknown flag");
    return mux_impl(c, v, pool_rows, iv, not_ab, out, B, mem);
}

int mkt_not_batch(mkt_ctx *c, uint32_t *x, size_t B, int mem) {
    if (!c || !x || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    DevGuard dg(c->device);
    Staged sx{c};
    int r;
    const size_t words = B * (size_t)c->sh.lwe_len;
    if ((r = sx.in(x, words * 4, mem, true))) return r;
    HIPCHK(c, mktd::launch_negate(sx.as<uint32_t>(), words, c->stream));
    return sx.out(x);
}

int mkt_bootstrap_batch(mkt_ctx *c, uint32_t *lwe, size_t B, int mem) {
    if (!c || !lwe || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    MKT_EXACT_GATE(c);
    int r;
    if ((r = check_ready(c, true, true))) return r;
    DevGuard dg(c->device);
    Timer whole(c, 0);
    const size_t len = (size_t)c->sh.lwe_len;
    Staged sx{c};
    if ((r = sx.in(lwe, B * len * 4, mem, true))) return r;
    for (size_t off = 0; off < B; off += CHUNK_GATES) {
        const size_t nb = std::min(CHUNK_GATES, B - off);
        if ((r = ensure_workspace(c, nb))) return r;
        uint32_t *chunk = sx.as<uint32_t>() + off * len;
        // the rotation reads the masks, phase 2 / the test vector read b, all before key switching overwrites them
        if ((r = bootstrap_chunk(c, chunk, chunk, nb))) return r;
    }
    return sx.out(lwe);
}

// ---- programmable bootstrap (mktfhe.h): a caller's lookup tables in place of the constant test vector ----
// the tables and row selectors of one call on the device; with MKT_MEM_HOST a selector beyond the table is refused here (a device array is
// clamped by the kernel: no out-of-bounds read)
struct StagedLuts {
    Staged luts, sel;
    explicit StagedLuts(mkt_ctx *c) : luts{c}, sel{c} {}
    int in(mkt_ctx *c, const char *who, const void *l, size_t nluts, const uint32_t *s, size_t B, int mem) {
        if (!nluts) return fail(c, MKT_ERR_ARG, std::string(who) + ": no lookup table");
        if (s && mem == MKT_MEM_HOST && !mkt::host_below(s, B, nluts)) return fail(c, MKT_ERR_ARG, std::string(who) + ": table selector outside the tables");
        int r;
        if ((r = luts.in(l, nluts * poly_bytes(c), mem, true))) return r;
        return s ? sel.in(s, B * 4, mem, true) : MKT_OK;
    }
    LutArgs chunk(size_t nluts, size_t off) const { return LutArgs{luts.dev, nluts, sel.dev ? sel.as<const uint32_t>() + off : nullptr}; }
};

// unit level: acc[j] = (X^btilde(lwe[j]) * luts[sel[j]], 0 ...), what the programmable bootstrap hands to blindrotate!; no keys needed
int mkt_lut_testvector_batch(mkt_ctx *c, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lwe, void *acc, size_t B, int mem) {
    if (!c || !luts || !lwe || !acc || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    DevGuard dg(c->device);
    const size_t len = (size_t)c->sh.lwe_len, accb = (size_t)(1 + c->sh.kacc) * poly_bytes(c);
    StagedLuts t(c);
    Staged sx{c}, sc{c};
    int r;
    if ((r = t.in(c, "mkt_lut_testvector_batch", luts, nluts, sel, B, mem)) || (r = sx.in(lwe, B * len * 4, mem, true)) || (r = sc.in(acc, B * accb, mem, false))) return r;
    const LutArgs a = t.chunk(nluts, 0);
    HIPCHK(c, mktd::launch_lut_testvector(c->p.W, a.luts, a.nluts, a.sel, sx.as<const uint32_t>(), (int)len, c->logN, c->sh.kacc, sc.dev, B, c->stream));
    return sc.out(acc);
}

// the gather front end of a circuit level: gate j's input is cst[j] e_b + sum_t wt[j][t] pool[idx[j][t]] (lut_linear_kernel); idx [B][4], wt [B][4], cst [B]
struct LutGather {
    const uint32_t *pool; size_t rows; const uint32_t *idx; const int8_t *wt; const uint32_t *cst;
    bool null() const { return !pool || !idx || !wt || !cst; }
};
// what every gather entry point refuses before anything is staged or written; validation as mkt_gate_batch_gather
static int gather_ok(mkt_ctx *c, const std::string &who, const LutGather &g, size_t B, int mem) {
    if (B && !g.rows) return fail(c, MKT_ERR_ARG, who + ": gates over an empty pool");
    if (mem == MKT_MEM_HOST && !mkt::host_below(g.idx, 4 * B, g.rows)) return fail(c, MKT_ERR_ARG, who + ": operand index outside the pool");
    return MKT_OK;
}

// all lookup-table bootstraps share one body.  k describes the call in the caller's memory (tables, selectors and coef are staged here); the
// inputs are lwe [B][len] in batch order, or built per gate from g's pool.  out [B][k.per][len], in chunks of max(1, CHUNK_GATES / k.per)
// inputs so that a key switch sees at most CHUNK_GATES rows (k.per rows where one input has more)
static int lut_impl(mkt_ctx *c, const char *who, LutChunk k, const uint32_t *lwe, const LutGather *g, uint32_t *out, size_t B, int mem) {
    const size_t step = std::max<size_t>(1, CHUNK_GATES / k.per), nluts = k.t.nluts;
    MKT_EXACT_GATE(c);
    int r;
    if ((r = check_ready(c, true, true))) return r;
    DevGuard dg(c->device);
    Timer whole(c, 0);
    const size_t len = (size_t)c->sh.lwe_len, rows = g ? g->rows : B;
    StagedLuts t(c);
    Staged sv{c}, so{c}, si{c}, sw{c}, sk{c}, sf{c};
    if (k.coef && !B) return MKT_OK;
    if (k.coef && (r = sf.in(k.coef, k.per * 4, mem, true))) return r;
    k.coef = sf.as<const uint32_t>();
    if (k.at && (r = at_table(c, k, std::min(step, B) * k.per))) return r;
    if ((r = t.in(c, who, k.t.luts, nluts, k.t.sel, B, mem)) || (r = sv.in(g ? g->pool : lwe, rows * len * 4, mem, true)) || (r = so.in(out, B * k.per * len * 4, mem, false))) return r;
    if (g && ((r = si.in(g->idx, B * 16, mem, true)) || (r = sw.in(g->wt, B * 4, mem, true)) || (r = sk.in(g->cst, B * 4, mem, true)))) return r;
    for (size_t off = 0; off < B; off += step) {
        const size_t nb = std::min(step, B - off);
        if ((r = ensure_workspace(c, nb))) return r;
        const uint32_t *lin = sv.as<const uint32_t>() + off * len;
        if (g) {
            HIPCHK(c, mktd::launch_lut_linear(sv.as<const uint32_t>(), rows, si.as<const uint32_t>() + off * 4, sw.as<const int8_t>() + off * 4, sk.as<const uint32_t>() + off,
                                              c->ws.lin.as<uint32_t>(), (int)len, nb, c->stream));
            lin = c->ws.lin.as<uint32_t>();
        }
        k.t = t.chunk(nluts, off);
        if ((r = lut_chunk(c, k, lin, so.as<uint32_t>() + off * k.per * len, nb))) return r;
    }
    return so.out(out);
}

// out[j] = keyswitch!(blindrotate!((X^btilde(lwe[j]) * luts[sel[j]], 0 ...))): bootstrapping! with a caller's table; out may be lwe
int mkt_lut_bootstrap_batch(mkt_ctx *c, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lwe, uint32_t *out, size_t B, int mem) {
    if (!c || !luts || !lwe || !out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    return lut_impl(c, "mkt_lut_bootstrap_batch", LutChunk{{luts, nluts, sel}, 0, 1, false, nullptr}, lwe, nullptr, out, B, mem);
}

// one circuit level of table lookups: gate j bootstraps cst[j] e_b + sum_t wt[j][t] pool[idx[j][t]] through luts[sel[j]]; out may be a later
// region of the pool that no gate of this call reads
int mkt_lut_batch_gather(mkt_ctx *c, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *pool, size_t pool_rows, const uint32_t *idx,
                         const int8_t *wt, const uint32_t *cst, uint32_t *out, size_t B, int mem) {
    const LutGather g{pool, pool_rows, idx, wt, cst};
    if (!c || !luts || g.null() || !out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    if (int r = gather_ok(c, "mkt_lut_batch_gather", g, B, mem)) return r;
    return lut_impl(c, "mkt_lut_batch_gather", LutChunk{{luts, nluts, sel}, 0, 1, false, nullptr}, nullptr, &g, out, B, mem);
}

// ---- many-table bootstrap (mktfhe.h): nout tables per blind rotation ----
// nu = log2(nout) for a table count the library takes, else -1
static int many_nu(const mkt_ctx *c, int nout) { return mkt::lut_nout_ok(nout, c->p.N) ? __builtin_ctz((unsigned)nout) : -1; }
static int bad_nout(mkt_ctx *c, const char *who, int nout) {
    return fail(c, MKT_ERR_ARG, std::string(who) + ": nout = " + std::to_string(nout) + ", expected 1, 2, 4 or 8 and at most N = " + std::to_string(c->p.N));
}
using mkt::ranges_overlap;

// unit level: the coarse-switched mask words atilde [B][k*n] and acc[j] = (X^btilde * luts[sel[j]], 0 ...) from the coarse btilde; no keys needed
int mkt_lut_many_testvector_batch(mkt_ctx *c, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lwe, int nout, uint32_t *atilde, void *acc, size_t B, int mem) {
    if (!c || !luts || !lwe || !atilde || !acc || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    const int nu = many_nu(c, nout);
    if (nu < 0) return bad_nout(c, "mkt_lut_many_testvector_batch", nout);
    DevGuard dg(c->device);
    const size_t len = (size_t)c->sh.lwe_len, accb = (size_t)(1 + c->sh.kacc) * poly_bytes(c);
    StagedLuts t(c);
    Staged sx{c}, sa{c}, sc{c};
    int r;
    if ((r = t.in(c, "mkt_lut_many_testvector_batch", luts, nluts, sel, B, mem)) || (r = sx.in(lwe, B * len * 4, mem, true)) || (r = sa.in(atilde, B * (len - 1) * 4, mem, false)) ||
        (r = sc.in(acc, B * accb, mem, false))) return r;
    const LutArgs a = t.chunk(nluts, 0);
    HIPCHK(c, mktd::launch_lut_many_testvector(c->p.W, a.luts, a.nluts, a.sel, sx.as<const uint32_t>(), (int)len, c->logN, c->sh.kacc, nu, sa.as<uint32_t>(), (int)len - 1, sc.dev, B, c->stream));
    if ((r = sa.out(atilde))) return r;
    return sc.out(acc);
}

// unit level: accs[j][v] = X^-v * acc[j], v < nout; acc [B][1+k][N] -> accs [B][nout][1+k][N]
int mkt_lut_extract_batch(mkt_ctx *c, const void *acc, int nout, void *accs, size_t B, int mem) {
    if (!c || !acc || !accs || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    if (many_nu(c, nout) < 0) return bad_nout(c, "mkt_lut_extract_batch", nout);
    const size_t accb = (size_t)(1 + c->sh.kacc) * poly_bytes(c);
    if (ranges_overlap(acc, B * accb, accs, B * nout * accb)) return fail(c, MKT_ERR_ARG, "mkt_lut_extract_batch: accs overlaps acc");
    DevGuard dg(c->device);
    Staged sc{c}, so{c};
    int r;
    if ((r = sc.in(acc, B * accb, mem, true)) || (r = so.in(accs, B * nout * accb, mem, false))) return r;
    HIPCHK(c, mktd::launch_lut_extract(c->p.W, sc.dev, nout, c->logN, c->sh.kacc, so.dev, B, c->stream));
    return so.out(accs);
}

// out[j][v] = keyswitch!(E_v(blindrotate!(coarse atilde(lwe[j]), (X^btilde * luts[sel[j]], 0 ...)))): nout tables in one rotation, the key switch
// at the coefficient list 0 .. nout - 1 (nout = 1: the plain key switch)
static LutChunk many_chunk(const void *luts, size_t nluts, const uint32_t *sel, int nu) { return LutChunk{{luts, nluts, sel}, nu, (size_t)1 << nu, nu > 0, nullptr}; }

int mkt_lut_many_bootstrap_batch(mkt_ctx *c, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lwe, int nout, uint32_t *out, size_t B, int mem) {
    if (!c || !luts || !lwe || !out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    const int nu = many_nu(c, nout);
    if (nu < 0) return bad_nout(c, "mkt_lut_many_bootstrap_batch", nout);
    const size_t rb = (size_t)c->sh.lwe_len * 4;
    if (nout > 1 && ranges_overlap(lwe, B * rb, out, B * (size_t)nout * rb)) return fail(c, MKT_ERR_ARG, "mkt_lut_many_bootstrap_batch: out overlaps lwe (nout > 1)");
    return lut_impl(c, "mkt_lut_many_bootstrap_batch", many_chunk(luts, nluts, sel, nu), lwe, nullptr, out, B, mem);
}

// the linear front end of mkt_lut_batch_gather, then the many-table bootstrap; out [B][nout][len] may be a later region of the pool
int mkt_lut_many_batch_gather(mkt_ctx *c, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *pool, size_t pool_rows, const uint32_t *idx,
                              const int8_t *wt, const uint32_t *cst, int nout, uint32_t *out, size_t B, int mem) {
    const LutGather g{pool, pool_rows, idx, wt, cst};
    if (!c || !luts || g.null() || !out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    const int nu = many_nu(c, nout);
    if (nu < 0) return bad_nout(c, "mkt_lut_many_batch_gather", nout);
    if (int r = gather_ok(c, "mkt_lut_many_batch_gather", g, B, mem)) return r;
    return lut_impl(c, "mkt_lut_many_batch_gather", many_chunk(luts, nluts, sel, nu), nullptr, &g, out, B, mem);
}

// ---- key switch at a coefficient (mktfhe.h): the bootstrap at a coefficient list ----
// what every such entry point refuses before anything is staged or written; coef on the host is checked against N here
static int at_args_ok(mkt_ctx *c, const std::string &who, int nu, const uint32_t *coef, size_t ncoef, int mem) {
    const int N = c->p.N;
    if (!mkt::lut_nu_ok(nu, N)) return fail(c, MKT_ERR_ARG, who + ": nu = " + std::to_string(nu) + ", expected 0 .. 3 with 2^nu at most N = " + std::to_string(N));
    if (!mkt::lut_ncoef_ok(ncoef, N)) return fail(c, MKT_ERR_ARG, who + ": " + std::to_string(ncoef) + " coefficients, expected 1 .. N = " + std::to_string(N));
    if (mem == MKT_MEM_HOST && !mkt::host_below(coef, ncoef, (size_t)N)) return fail(c, MKT_ERR_ARG, who + ": a coefficient is not below N");
    return MKT_OK;
}

// out[j][i] = keyswitch!(E_coef[i](blindrotate!(sw_nu(a_j), (X^sw_nu(b_j) * luts[sel[j]], 0 ...)))): ncoef outputs of one rotation
int mkt_lut_bootstrap_at_batch(mkt_ctx *c, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lwe, int nu, const uint32_t *coef, size_t ncoef, uint32_t *out, size_t B, int mem) {
    if (!c || !luts || !lwe || !coef || !out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    if (int r = at_args_ok(c, "mkt_lut_bootstrap_at_batch", nu, coef, ncoef, mem)) return r;
    const size_t rb = (size_t)c->sh.lwe_len * 4;
    if (ncoef > 1 && ranges_overlap(lwe, B * rb, out, B * ncoef * rb)) return fail(c, MKT_ERR_ARG, "mkt_lut_bootstrap_at_batch: out overlaps lwe (ncoef > 1)");
    return lut_impl(c, "mkt_lut_bootstrap_at_batch", LutChunk{{luts, nluts, sel}, nu, ncoef, true, coef}, lwe, nullptr, out, B, mem);
}

// the linear front end of mkt_lut_batch_gather, then the above; out [B][ncoef][len] may be a later region of the pool
int mkt_lut_batch_gather_at(mkt_ctx *c, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *pool, size_t pool_rows, const uint32_t *idx,
                            const int8_t *wt, const uint32_t *cst, int nu, const uint32_t *coef, size_t ncoef, uint32_t *out, size_t B, int mem) {
    const LutGather g{pool, pool_rows, idx, wt, cst};
    if (!c || !luts || g.null() || !coef || !out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    int r;
    if ((r = at_args_ok(c, "mkt_lut_batch_gather_at", nu, coef, ncoef, mem)) || (r = gather_ok(c, "mkt_lut_batch_gather_at", g, B, mem))) return r;
    return lut_impl(c, "mkt_lut_batch_gather_at", LutChunk{{luts, nluts, sel}, nu, ncoef, true, coef}, nullptr, &g, out, B, mem);
}

int mkt_modswitch_batch(mkt_ctx *c, const uint32_t *lwe, uint32_t *atilde, uint32_t *btilde, size_t B, int mem) {
    if (!c || !lwe || !atilde || !btilde || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    DevGuard dg(c->device);
    const size_t len = (size_t)c->sh.lwe_len;
    Staged sl{c}, sa{c}, sb{c};
    int r;
    if ((r = sl.in(lwe, B * len * 4, mem, true)) || (r = sa.in(atilde, B * (len - 1) * 4, mem, false)) || (r = sb.in(btilde, B * 4, mem, false))) return r;
    HIPCHK(c, mktd::launch_modswitch(sl.as<const uint32_t>(), sa.as<uint32_t>(), sb.as<uint32_t>(), (int)len, c->logN, B, c->stream));
    if ((r = sa.out(atilde))) return r;
    return sb.out(btilde);
}

int mkt_blindrotate_batch(mkt_ctx *c, const uint32_t *atilde, void *acc, size_t B, int mem) {
    if (!c || !atilde || !acc || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    MKT_EXACT_GATE(c);
    int r;
    if ((r = check_ready(c, true, false))) return r;
    DevGuard dg(c->device);
    Timer whole(c, 0);
    const size_t alen = (size_t)c->sh.lwe_len - 1, accb = (size_t)(1 + c->sh.kacc) * poly_bytes(c);
    Staged sa{c}, sc{c};
    if ((r = sa.in(atilde, B * alen * 4, mem, true)) || (r = sc.in(acc, B * accb, mem, true))) return r;
    for (size_t off = 0; off < B; off += CHUNK_GATES) {
        const size_t nb = std::min(CHUNK_GATES, B - off);
        if ((r = ensure_workspace(c, nb))) return r;
        if ((r = do_blindrotate(c, sa.as<const uint32_t>() + off * alen, (int)alen, 1, nullptr, sc.as<char>() + off * accb, nb))) return r;
    }
    return sc.out(acc);
}

int mkt_kms_phase1_batch(mkt_ctx *c, const uint32_t *atilde, double *levkey, size_t B, int mem) {
    if (!c || !atilde || !levkey || !mem_ok(mem) || !mkt::is_kms(c->p.scheme)) return fail(c, MKT_ERR_ARG, "bad argument");
    MKT_F64_OR_EXACT_KMS(c);
    int r;
    if ((r = check_ready(c, true, false))) return r;
    DevGuard dg(c->device);
    const size_t alen = (size_t)c->sh.lwe_len - 1, lb = (size_t)c->ks->rtot * 2 * c->M * sizeof(cplx) * c->split;
    Staged sa{c}, sl{c};
    if ((r = sa.in(atilde, B * alen * 4, mem, true)) || (r = sl.in(levkey, B * lb, mem, false))) return r;
    if (c->exact) {   // the rows as split residue tables [B][rows][2 polys][2 halves][N] (uint64 residue pairs, Montgomery form)
        if (c->p.scheme == MKT_KMS && fx_usable(c)) {
            if ((r = ensure_workspace(c, B < CHUNK_GATES ? B : CHUNK_GATES))) return r;
            for (size_t off = 0; off < B; off += CHUNK_GATES) {
                const size_t nb = B - off < CHUNK_GATES ? B - off : CHUNK_GATES;
                Timer tm(c, 1);
                if ((r = fx_phase1(c, sa.as<const uint32_t>() + off * alen, (int)alen, 1, nb, sl.as<uint64_t>() + off * (lb / 8)))) return r;
            }
        } else {
            mktd::ExactKmsArgs q = exact_kms_args(c, sa.as<const uint32_t>(), (int)alen, 1);
            q.levkey = sl.as<uint64_t>(); q.phase1_only = 1;
            Timer tm(c, 1);
            HIPCHK(c, mktd::launch_exact_kms(c->logN, c->ks->d_ntt, q, B, c->stream));
        }
        return sl.out(levkey);
    }
    mktd::RotArgs a = rot_args(c, sa.as<const uint32_t>(), (int)alen, 1);
    a.init_mode = 1; a.out_mode = 1; a.tout = sl.as<cplx>(); a.tout_natural = 1; a.ngates = B;
    { Timer tm(c, 1); HIPCHK(c, mktd::launch_blindrotate_k1(c->logM, c->p.W, a, B * (size_t)c->ks->rtot, c->stream)); }
    return sl.out(levkey);
}

int mkt_keyswitch_batch(mkt_ctx *c, const void *acc, uint32_t *out, size_t B, int mem) {
    if (!c || !acc || !out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    MKT_EXACT_GATE(c);
    int r;
    if ((r = check_ready(c, false, true))) return r;
    DevGuard dg(c->device);
    const size_t accb = (size_t)(1 + c->sh.kacc) * poly_bytes(c), len = (size_t)c->sh.lwe_len;
    Staged sc{c}, so{c};
    if ((r = sc.in(acc, B * accb, mem, true)) || (r = so.in(out, B * len * 4, mem, false))) return r;
    if ((r = do_keyswitch(c, sc.dev, so.as<uint32_t>(), B))) return r;
    return so.out(out);
}

// out[g] = keyswitch!(E_coef[g](acc[src[g]])); rows in chunks of CHUNK_GATES, each reading the whole of acc (src NULL: its own rows of it)
int mkt_keyswitch_at_batch(mkt_ctx *c, const void *acc, size_t nacc, const uint32_t *src, const uint32_t *coef, uint32_t *out, size_t B, int mem) {
    if (!c || !acc || !out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    if (B && !nacc) return fail(c, MKT_ERR_ARG, "mkt_keyswitch_at_batch: output rows over no accumulator");
    if (!src && nacc != B) return fail(c, MKT_ERR_ARG, "mkt_keyswitch_at_batch: src NULL names accumulator g for row g: nacc must equal B");
    if (mem == MKT_MEM_HOST) {
        const uint32_t *is[] = {src}, *ic[] = {coef};
        if (src && !in_pool_host(is, 1, B, nacc)) return fail(c, MKT_ERR_ARG, "mkt_keyswitch_at_batch: src names a row outside acc");
        if (coef && !in_pool_host(ic, 1, B, (size_t)c->p.N)) return fail(c, MKT_ERR_ARG, "mkt_keyswitch_at_batch: a coefficient is not below N");
    }
    MKT_EXACT_GATE(c);
    int r;
    if ((r = check_ready(c, false, true))) return r;
    if (!B) return MKT_OK;
    DevGuard dg(c->device);
    const size_t accb = (size_t)(1 + c->sh.kacc) * poly_bytes(c), len = (size_t)c->sh.lwe_len;
    Staged sc{c}, so{c}, ss{c}, sf{c};
    if ((r = sc.in(acc, nacc * accb, mem, true)) || (r = so.in(out, B * len * 4, mem, false))) return r;
    if (src && (r = ss.in(src, B * 4, mem, true))) return r;
    if (coef && (r = sf.in(coef, B * 4, mem, true))) return r;
    for (size_t off = 0; off < B; off += CHUNK_GATES) {
        const size_t nb = std::min(CHUNK_GATES, B - off);
        const void *a0 = src ? sc.dev : sc.as<const char>() + off * accb;
        if ((r = do_keyswitch(c, a0, so.as<uint32_t>() + off * len, nb, src ? ss.as<const uint32_t>() + off : nullptr, coef ? sf.as<const uint32_t>() + off : nullptr, src ? nacc : nb))) return r;
    }
    return so.out(out);
}

int mkt_transform_fwd_batch(mkt_ctx *c, const void *p, double *t, size_t B, int mem) {
    if (!c || !p || !t || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    DevGuard dg(c->device);
    Staged sp{c}, st{c};
    int r;
    if ((r = sp.in(p, B * poly_bytes(c), mem, true)) || (r = st.in(t, B * (size_t)c->M * sizeof(cplx), mem, false))) return r;
    if (c->exact) { Timer tm(c, 3); HIPCHK(c, mktd::launch_ntt_fwd(c->logN, c->p.W, c->ks->d_ntt, sp.dev, st.as<uint64_t>(), B, 0, c->stream)); }
    else { Timer tm(c, 3); HIPCHK(c, mktd::launch_transform_fwd(c->logM, c->p.W, c->twp(), sp.dev, st.as<cplx>(), B, 0, c->stream)); }
    return st.out(t);
}

int mkt_transform_inv_batch(mkt_ctx *c, const double *t, void *p, size_t B, int mem) {
    if (!c || !p || !t || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    DevGuard dg(c->device);
    Staged st{c}, sp{c};
    int r;
    if ((r = st.in(t, B * (size_t)c->M * sizeof(cplx), mem, true)) || (r = sp.in(p, B * poly_bytes(c), mem, false))) return r;
    if (c->exact) { Timer tm(c, 3); HIPCHK(c, mktd::launch_ntt_inv(c->logN, c->p.W, c->ks->d_ntt, st.as<const uint64_t>(), sp.dev, B, c->stream)); }
    else { Timer tm(c, 3); HIPCHK(c, mktd::launch_transform_inv(c->logM, c->p.W, c->twp(), st.as<const cplx>(), sp.dev, B, c->stream)); }
    return sp.out(p);
}

int mkt_decompose_batch(mkt_ctx *c, const void *p, void *digits, int l, int logB, size_t B, int mem) {
    if (!c || !p || !digits || !mem_ok(mem) || l < 1 || logB < 1 || l * logB > c->p.W) return fail(c, MKT_ERR_ARG, "bad argument");
    DevGuard dg(c->device);
    Staged sp{c}, sd{c};
    int r;
    if ((r = sp.in(p, B * poly_bytes(c), mem, true)) || (r = sd.in(digits, B * (size_t)l * poly_bytes(c), mem, false))) return r;
    HIPCHK(c, mktd::launch_decompose(c->p.W, sp.dev, sd.dev, c->p.N, l, logB, B, c->stream));
    return sd.out(digits);
}

// MKT_ARITH_EXACT: out = a (*) b in Z_{2^W}[X]/(X^N + 1), exact, for a signed polynomial a with N * max|a_i| <= 2^28 - 2^15 and any b.
// Contract: a true coefficient of a times a centered 32-bit piece of b is at most N max|a| 2^31 <= (2^28 - 2^15) 2^31 < P / 2 = 2^59 - 6.6e13, so
// the integer NTT's centred lift returns it (it would wrap from N max|a| = 268 404 738 on, 30 718 below 2^28); the Float64 pipe's limb sums stay
// below N max|a| 2^15 <= 2^43, inside its rounding trick.  max|a_i| is measured on the device over the whole batch; a call outside the contract is
// refused (MKT_ERR_ARG), no words written.  Under exact_impl = 1 the Float64 kernel runs only where fx_polymul_bound certifies the operands
// (< 0.45, a priori, from max|a_i| and the measured transform maximum of b's limbs); the integer NTT serves the other calls, with the same words.
// mkt_last_kernel_name names the kernel that served the call.
constexpr uint64_t POLYMUL_NA_MAX = (1ull << 28) - (1ull << 15);
int mkt_exact_polymul_batch(mkt_ctx *c, const void *a, const void *b, void *out, size_t B, int mem) {
    if (!c || !a || !b || !out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    if (!c->exact) return fail(c, MKT_ERR_UNSUPPORTED, "mkt_exact_polymul_batch needs an MKT_ARITH_EXACT context");
    DevGuard dg(c->device);
    c->last_rot_kernel = ""; c->rot_static_l = c->rot_static_logB = 0; c->pm_amax = 0.0; c->pm_bound = -1.0; c->fx_last_resid = 0.0;
    Staged sa{c}, sb{c}, so{c};
    int r;
    if ((r = sa.in(a, B * poly_bytes(c), mem, true)) || (r = sb.in(b, B * poly_bytes(c), mem, true)) || (r = so.in(out, B * poly_bytes(c), mem, false))) return r;
    HIPCHK(c, c->ws.pm_stat.reserve(3 * sizeof(unsigned long long)));   // at the first call
    const bool fx = c->ks->d_fx_tab && c->tune.exact_impl == 1;
    unsigned long long st[2] = {0, 0};
    HIPCHK(c, hipMemsetAsync(c->ws.pm(), 0, 3 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, mktd::launch_exact_amax(c->p.W, sa.dev, B * (size_t)c->p.N, c->ws.pm(), c->stream));
    if (fx) HIPCHK(c, mktd::launch_fx_key_fwd(c->logM, c->p.W, c->fx_om(), c->fx_tw(), sb.dev, nullptr, B, c->ws.pm() + 1, c->stream));
    HIPCHK(c, hipMemcpyAsync(st, c->ws.pm(), sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pm_amax = (double)st[0];
    if (st[0] > POLYMUL_NA_MAX / (uint64_t)c->p.N)
        return fail(c, MKT_ERR_ARG, "mkt_exact_polymul_batch: max|a_i| = " + std::to_string(st[0]) + " at N = " + std::to_string(c->p.N) +
                                    " is outside the contract N * max|a_i| <= 2^28 - 2^15 (max|a_i| <= " + std::to_string(POLYMUL_NA_MAX / (uint64_t)c->p.N) + ")");
    if (fx) {
        double k2; std::memcpy(&k2, &st[1], 8);
        c->pm_bound = fx_polymul_bound(c, (double)st[0], std::sqrt(k2));
        if (c->pm_bound < 0.45 || c->tune.fx_polymul_force) {   // the Float64-pipe product (fx_exact.hip)
            { Timer tm(c, 3); HIPCHK(c, mktd::launch_fx_polymul(c->logM, c->p.W, c->fx_om(), c->fx_tw(), c->fx_nat(), sa.dev, sb.dev, so.dev, B, c->ws.pm() + 2, c->stream)); }
            unsigned long long bits = 0;
            HIPCHK(c, hipMemcpyAsync(&bits, c->ws.pm() + 2, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            std::memcpy(&c->fx_last_resid, &bits, 8);
            c->last_rot_kernel = "fx_polymul_kernel";
            return so.out(out);
        }
    }
    { Timer tm(c, 3); HIPCHK(c, mktd::launch_exact_polymul(c->logN, c->p.W, c->ks->d_ntt, sa.dev, sb.dev, so.dev, B, c->stream)); }
    c->last_rot_kernel = "exact_polymul_kernel";
    return so.out(out);
}

// ---- packed outputs (mktfhe_pack.h): N LWE rows into one RLWE ciphertext by the packing key switch (pack.hip) ----
constexpr size_t PACK_CHUNK = 16;      // packs per launch sequence: bounds the workspace (KMS2party: 16 packs = 0.3 GiB of columns, 0.15 GiB of slabs)
constexpr int PACK_EXACT_COLS = 64;    // MKT_ARITH_EXACT: columns per decompose / exact-product launch

// what every load of a packing key checks before it touches anything (`who`: the entry point, for the message); then the party's slot of the
// resident table, allocated by the first load, which fixes the context's gadget
static int pack_load_guard(mkt_ctx *c, const std::string &who, int l_pk, int logB_pk) {
    if (!mkt::pack_gadget_ok(l_pk, logB_pk)) return fail(c, MKT_ERR_ARG, who + ": the packing gadget needs 1 <= logB_pk <= 16, 1 <= l_pk, l_pk * logB_pk <= 32");
    const mkt_params &p = c->p;
    if (!mktd::pack_supported(c->sh.ksk_kr + 1)) return fail(c, MKT_ERR_UNSUPPORTED, who + ": RLWE lengths beyond 3 are not served");
    // EXACT: every product of a digit polynomial (N digits of magnitude <= 2^(logB_pk - 1)) with a centered 32-bit piece of a key polynomial must stay below P / 2
    if (c->exact && (double)p.N * std::ldexp(1.0, logB_pk - 1) * 2147483648.0 >= 0.5 * (double)NTT_P[0] * (double)NTT_P[1])
        return fail(c, MKT_ERR_UNSUPPORTED, who + ": the rows of this gadget could reach P / 2 of the two-prime modulus");
    if (int w = keys_writable(c)) return w;
    const KeySet &ks = *c->ks;
    if (ks.d_pack.p && (ks.pack_l != l_pk || ks.pack_logB != logB_pk)) return fail(c, MKT_ERR_ARG, who + ": all parties of a context use one packing gadget");
    return MKT_OK;
}
static int pack_party_slot(mkt_ctx *c, int party, int l_pk, int logB_pk, char **dst) {
    KeySet &ks = *c->ks;
    const size_t polys = mkt::pack_key_polys(c->p, c->sh, l_pk);
    const size_t per = polys * (c->exact ? poly_bytes(c) : (size_t)c->M * sizeof(cplx));
    if (!ks.d_pack.p) {
        HIPCHK(c, ks.d_pack.alloc(per * c->sh.nparty));
        ks.pack_l = l_pk; ks.pack_logB = logB_pk; ks.pack_party_bytes = per; ks.pack_loaded.assign((size_t)c->sh.nparty, 0);
    }
    *dst = ks.d_pack.as<char>() + (size_t)party * per;
    return MKT_OK;
}

int mkt_load_packing_key(mkt_ctx *c, int party, const void *pk, int l_pk, int logB_pk) {
    if (!c || !pk || party < 0 || party >= c->sh.nparty) return fail(c, MKT_ERR_ARG, "bad argument");
    if (int r = pack_load_guard(c, "mkt_load_packing_key", l_pk, logB_pk)) return r;
    const mkt_params &p = c->p;
    const int np = c->sh.ksk_kr + 1;
    KeySet &ks = *c->ks;
    DevGuard dg(c->device);
    const size_t rows = (size_t)p.n * l_pk, polys = rows * np, pb = poly_bytes(c);
    char *dst;
    if (int r = pack_party_slot(c, party, l_pk, logB_pk, &dst)) return r;
    if (!c->exact) {          // pre-transformed like the bootstrapping key, in the slot-major point order whatever the context's own
        DevBuf tmp;
        HIPCHK(c, tmp.alloc(polys * pb));
        HIPCHK(c, hipMemcpyAsync(tmp.p, pk, polys * pb, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, mktd::launch_transform_fwd(c->logM, p.W, c->twp(), tmp.p, reinterpret_cast<cplx *>(dst), polys, 1, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {                  // coefficient form, [row][polynomial] -> [polynomial][row]
        std::vector<unsigned char> host(polys * pb);
        for (size_t r = 0; r < rows; r++) for (int q = 0; q < np; q++)
            std::memcpy(host.data() + ((size_t)q * rows + r) * pb, static_cast<const unsigned char *>(pk) + (r * np + q) * pb, pb);
        HIPCHK(c, hipMemcpyAsync(dst, host.data(), polys * pb, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    ks.pack_loaded[(size_t)party] = 1;
    return MKT_OK;
}

// The seeded packing key (mktfhe_pack.h "SEEDED"; pack_keys.hip): party `party`'s key regenerated on this context's device from the public mask
// seed and the bodies [n][l_pk][N], the words of mkt_client_packing_key_expand.  load: into the resident table -- F64REF through a coefficient
// staging buffer and the forward transform, as mkt_load_packing_key after its upload; EXACT straight into [polynomial][row] from the kernel --
// else into the caller's pk_out (`mem`).  `mem` says where pk_seeded lives in either case: the bodies mkt_packing_keygen_device has just made
// on this device are installed from there.  Nothing is secret.  The caller has checked the arguments (load: pack_load_guard)
static int pack_key_seeded_impl(mkt_ctx *c, int party, int l_pk, int logB_pk, const uint8_t *mask_seed, const void *pk_seeded, bool load, void *pk_out, int mem) {
    const mkt_params &p = c->p;
    DevGuard dg(c->device);
    const size_t rows = (size_t)p.n * l_pk, polys = mkt::pack_key_polys(p, c->sh, l_pk), pb = poly_bytes(c);
    Staged sb{c}, so{c};
    DevBuf full;              // F64REF load: the expanded key in coefficient form
    int r;
    // the expansion kernel copies bodies and writes polynomials 16 bytes at a time, from the base pointers on: refused before any launch unless so aligned
    if ((r = sb.in(pk_seeded, rows * pb, mem, true, 16))) return r;
    char *slot = nullptr;
    void *dst;
    if (!load) { if ((r = so.in(pk_out, polys * pb, mem, false, 16))) return r; dst = so.dev; }
    else {
        if ((r = pack_party_slot(c, party, l_pk, logB_pk, &slot))) return r;
        if (c->exact) dst = slot; else { HIPCHK(c, full.alloc(polys * pb)); dst = full.p; }
    }
    mktd::PackKeyExpandArgs a{};
    mkt::seed_to_key(mask_seed, a.mkey);
    a.party = party; a.kr = c->sh.ksk_kr; a.l = l_pk; a.logB = logB_pk; a.log_units = c->logN + (p.W == 64 ? 1 : 0) - 4;
    a.transposed = load && c->exact ? 1 : 0; a.body = sb.dev; a.out = dst; a.rows = rows;
    hipError_t e = mktd::launch_pack_key_expand(a, c->stream);
    if (e == hipSuccess && load && !c->exact) e = mktd::launch_transform_fwd(c->logM, p.W, c->twp(), dst, reinterpret_cast<cplx *>(slot), polys, 1, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hipfail(c, e, "seeded packing key expansion");
    if (!load) return so.out(pk_out);
    c->ks->pack_loaded[(size_t)party] = 1;
    return MKT_OK;
}

int mkt_packing_key_expand(mkt_ctx *c, int party, int l_pk, int logB_pk, const uint8_t *mask_seed, const void *pk_seeded, void *pk_out, int mem) {
    if (!c || !mask_seed || !pk_seeded || !pk_out || !mem_ok(mem) || party < 0 || party >= c->sh.nparty) return fail(c, MKT_ERR_ARG, "bad argument");
    if (!mkt::pack_gadget_ok(l_pk, logB_pk)) return fail(c, MKT_ERR_ARG, "mkt_packing_key_expand: the packing gadget needs 1 <= logB_pk <= 16, 1 <= l_pk, l_pk * logB_pk <= 32");
    return pack_key_seeded_impl(c, party, l_pk, logB_pk, mask_seed, pk_seeded, false, pk_out, mem);
}

int mkt_load_packing_key_seeded(mkt_ctx *c, int party, const uint8_t *mask_seed, const void *pk_seeded, int l_pk, int logB_pk) {
    if (!c || !mask_seed || !pk_seeded || party < 0 || party >= c->sh.nparty) return fail(c, MKT_ERR_ARG, "bad argument");
    if (int r = pack_load_guard(c, "mkt_load_packing_key_seeded", l_pk, logB_pk)) return r;
    return pack_key_seeded_impl(c, party, l_pk, logB_pk, mask_seed, pk_seeded, true, nullptr, MKT_MEM_HOST);
}

// The bodies generated on the party's own GPU (pack_keys.hip): the words of mkt_client_packing_keygen_seeded for the same `seed`, word for word.
// Party-local like mkt_keygen_device_seeded, and the stream key reaches the device as it does there: in the kernel-argument struct, whose host
// copy is zeroed with the device secrets (wipe_secrets) -- NULL `seed` draws fresh entropy on the host, only the derived ChaCha key travels.
// install: the bodies, still on the device, also go through the expansion and install of mkt_load_packing_key_seeded
int mkt_packing_keygen_device(mkt_ctx *c, int party, const mkt_client_party *K, int l_pk, int logB_pk, const uint8_t *seed, const uint8_t *mask_seed,
                              void *pk_seeded_out, int install) {
    const RingKeys rk = pack_ring_keys(c);
    if (int r = party_call_guard(c, "mkt_packing_keygen_device", mask_seed != nullptr, party, K, rk)) return r;
    if (!pk_seeded_out && !install) return fail(c, MKT_ERR_ARG, "mkt_packing_keygen_device: neither an output nor an install was asked for");
    if (!mkt::pack_gadget_ok(l_pk, logB_pk)) return fail(c, MKT_ERR_ARG, "mkt_packing_keygen_device: the packing gadget needs 1 <= logB_pk <= 16, 1 <= l_pk, l_pk * logB_pk <= 32");
    const mkt_params &p = c->p;
    const int N = p.N;
    if ((seed && std::memcmp(seed, mask_seed, 32) == 0) || std::memcmp(mask_seed, K->key, sizeof K->key) == 0)
        return fail(c, MKT_ERR_ARG, "mkt_packing_keygen_device: the mask seed is a secret seed of the call (it is published: the secrets would be too)");
    if (install) if (int r = pack_load_guard(c, "mkt_packing_keygen_device", l_pk, logB_pk)) return r;
    DevGuard dg(c->device);
    const size_t body_bytes = (size_t)p.n * l_pk * poly_bytes(c);
    DevBuf bodies;                            // freed behind the secrets' drain of the stream
    DeviceSecret lwe{c}, z{c};
    mktd::PackKeygenArgs a{};
    hipError_t e = lwe.in(K->lwekey.data(), (size_t)p.n * 4);
    if (e == hipSuccess) e = z.ring_keys(K, rk);
    if (e == hipSuccess) e = bodies.alloc(body_bytes);
    if (e != hipSuccess) return hipfail(c, e, "device packing keygen setup");
    if (mkt::seed_to_key(seed, a.key)) { explicit_bzero(&a, sizeof a); return fail(c, MKT_ERR_STATE, "mkt_packing_keygen_device: no entropy"); }
    mkt::seed_to_key(mask_seed, a.mkey);
    a.party = party; a.N = N; a.n = p.n; a.W = p.W; a.kr = rk.count; a.l = l_pk; a.logB = logB_pk; a.sigma_ring = K->sigma_ring;
    a.lwekey = lwe.as<const uint32_t>(); a.zring = z.as<const int8_t>(); a.body = bodies.p;
    e = mktd::launch_pack_keygen(a, c->stream);
    if (e == hipSuccess && pk_seeded_out) e = hipMemcpyAsync(pk_seeded_out, bodies.p, body_bytes, hipMemcpyDeviceToHost, c->stream);
    e = wipe_secrets(wipe_secrets(e, z, a), lwe, a);       // (drains the stream: the output has landed)
    if (e != hipSuccess) return hipfail(c, e, "device packing keygen");
    if (!install) return MKT_OK;
    return pack_key_seeded_impl(c, party, l_pk, logB_pk, mask_seed, bodies.p, true, nullptr, MKT_MEM_DEVICE);
}

// the readiness check of a pack: every party's packing key, and nothing else
static int pack_ready(mkt_ctx *c) {
    const KeySet &ks = *c->ks;
    for (int i = 0; i < c->sh.nparty; i++)
        if (!ks.d_pack.p || !ks.pack_loaded[(size_t)i]) return fail(c, MKT_ERR_STATE, "packing key not loaded");
    return MKT_OK;
}

static int ensure_pack_workspace(mkt_ctx *c, size_t packs, int nchunk) {
    Workspace &w = c->ws;
    const size_t pb = poly_bytes(c), np = (size_t)c->sh.ksk_kr + 1;
    const size_t slabs = c->exact ? 0 : packs * (size_t)c->sh.nparty * nchunk * np * pb, chunk = c->exact ? (size_t)PACK_EXACT_COLS * c->ks->pack_l * pb : 0;
    DevBuf *const group[] = {&w.pack_cols, &w.pack_slabs, &w.pack_dig, &w.pack_prod};
    const size_t need[] = {packs * (size_t)c->sh.lwe_len * pb, slabs, chunk, chunk};
    HIPCHK(c, mkt::reserve_group(w.packs, packs, group, need));
    return MKT_OK;
}

int mkt_pack_batch(mkt_ctx *c, const uint32_t *pool, size_t pool_rows, const uint32_t *idx, size_t B, void *rlwe_out, int mem) {
    if (!c || !pool || !rlwe_out || !mem_ok(mem)) return fail(c, MKT_ERR_ARG, "bad argument");
    if (B && !pool_rows) return fail(c, MKT_ERR_ARG, "mkt_pack_batch: rows of an empty pool");
    if (!idx && B > pool_rows) return fail(c, MKT_ERR_ARG, "mkt_pack_batch: idx NULL names rows 0 .. B-1: B must not exceed pool_rows");
    if (mem == MKT_MEM_HOST && idx) {
        const uint32_t *iv[] = {idx};
        if (!in_pool_host(iv, 1, B, pool_rows)) return fail(c, MKT_ERR_ARG, "mkt_pack_batch: row index outside the pool");
    }
    const mkt_params &p = c->p;
    const size_t N = (size_t)p.N, len = (size_t)c->sh.lwe_len, pb = poly_bytes(c), ctb = (size_t)(1 + c->sh.kacc) * pb;
    const size_t npacks = (B + N - 1) / N;
    if (mkt::ranges_overlap(pool, pool_rows * len * 4, rlwe_out, npacks * ctb)) return fail(c, MKT_ERR_ARG, "mkt_pack_batch: rlwe_out overlaps the pool");
    int r;
    if ((r = pack_ready(c))) return r;
    if (!B) return MKT_OK;
    DevGuard dg(c->device);
    const KeySet &ks = *c->ks;
    Staged sp{c}, si{c}, so{c};
    if ((r = sp.in(pool, pool_rows * len * 4, mem, true)) || (r = so.in(rlwe_out, npacks * ctb, mem, false))) return r;
    if (idx && (r = si.in(idx, B * 4, mem, true))) return r;
    mktd::PackArgs a{};
    a.tw = c->twp(); a.pool = sp.as<const uint32_t>(); a.pool_rows = pool_rows; a.idx = idx ? si.as<const uint32_t>() : nullptr; a.B = B;
    a.logN = c->logN; a.n = p.n; a.nparty = c->sh.nparty; a.lwe_len = (int)len; a.kacc = c->sh.kacc; a.mk = mkt::is_mk(p.scheme) ? 1 : 0;
    a.np = c->sh.ksk_kr + 1; a.l = ks.pack_l; a.logB = ks.pack_logB; a.nchunk = (p.n + mktd::PACK_QCHUNK - 1) / mktd::PACK_QCHUNK;
    a.key = ks.d_pack.as<const cplx>(); a.key_party_stride = ks.pack_party_bytes / sizeof(cplx);
    for (size_t g0 = 0; g0 < npacks; g0 += PACK_CHUNK) {
        const size_t nb = std::min(PACK_CHUNK, npacks - g0);
        if ((r = ensure_pack_workspace(c, nb, a.nchunk))) return r;
        a.pack0 = g0; a.cols = c->ws.pack_cols.p; a.slabs = c->ws.pack_slabs.p; a.out = so.as<char>() + g0 * ctb;
        HIPCHK(c, mktd::launch_pack_columns(p.W, a, nb, c->stream));
        if (!c->exact) {
            HIPCHK(c, mktd::launch_pack_product(c->logM, p.W, a, nb, c->stream));
            HIPCHK(c, mktd::launch_pack_reduce(p.W, a, nb, c->stream));
            continue;
        }
        // EXACT: per pack, the body column and zeros, then per party and chunk of columns the digits, the exact products with each key polynomial, their integer sum
        const size_t rows_all = (size_t)p.n * a.l;
        for (size_t g = 0; g < nb; g++) {
            char *o = static_cast<char *>(a.out) + g * ctb;
            const char *cols = static_cast<const char *>(a.cols) + g * len * pb;
            HIPCHK(c, hipMemcpyAsync(o, cols + (len - 1) * pb, pb, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemsetAsync(o + pb, 0, ctb - pb, c->stream));
            for (int i = 0; i < a.nparty; i++) for (int q0 = 0; q0 < p.n; q0 += PACK_EXACT_COLS) {
                const size_t cnt = (size_t)std::min(PACK_EXACT_COLS, p.n - q0), prods = cnt * a.l;
                HIPCHK(c, mktd::launch_decompose(p.W, cols + ((size_t)i * p.n + q0) * pb, c->ws.pack_dig.p, p.N, a.l, a.logB, cnt, c->stream));
                for (int q = 0; q < a.np; q++) {
                    const char *key = ks.d_pack.as<const char>() + (size_t)i * ks.pack_party_bytes + ((size_t)q * rows_all + (size_t)q0 * a.l) * pb;
                    HIPCHK(c, mktd::launch_exact_polymul(c->logN, p.W, ks.d_ntt, c->ws.pack_dig.p, key, c->ws.pack_prod.p, prods, c->stream));
                    const int slot = q == 0 ? 0 : (a.mk ? 1 + i : q);
                    HIPCHK(c, mktd::launch_pack_accumulate(p.W, o + (size_t)slot * pb, c->ws.pack_prod.p, prods, p.N, c->stream));
                }
            }
        }
    }
    return so.out(rlwe_out);
}

// Ring shares of packed results (mktfhe_ring_share.h; ring_share.hip): party `party`'s shares of G packs on this context's device, the words of
// mkt_client_rlwe_partial_decrypt -- a party-local call like mkt_partial_decrypt_batch, on a context that needs no key of any kind.  The kr ring
// key polynomials the packs are under are uploaded for the call and wiped before they are freed
int mkt_rlwe_partial_decrypt_batch(mkt_ctx *c, int party, const mkt_client_party *K, const void *rlwe, double sigma_smudge, const uint8_t *seed,
                                   uint64_t row0, void *share_out, size_t G, int mem) {
    const RingKeys rk = pack_ring_keys(c);
    if (int r = party_call_guard(c, "mkt_rlwe_partial_decrypt_batch", mem_ok(mem), party, K, rk)) return r;
    if (!mkt::smudge_sigma_ok(sigma_smudge)) return fail(c, MKT_ERR_ARG, "mkt_rlwe_partial_decrypt_batch: sigma_smudge must be finite, 0 <= sigma_smudge <= 2^31");
    const mkt_params &p = c->p;
    const int N = p.N;
    if (!G) return MKT_OK;
    if (!rlwe || !share_out) return fail(c, MKT_ERR_ARG, "bad argument");
    DevGuard dg(c->device);
    Timer whole(c, 0);
    const size_t pb = poly_bytes(c);
    Staged sx{c}, so{c};
    DeviceSecret z{c};
    int r;
    if ((r = sx.in(rlwe, G * (size_t)(1 + c->sh.kacc) * pb, mem, true)) || (r = so.in(share_out, G * pb, mem, false))) return r;
    mktd::RingShareArgs a{};
    if (mkt::seed_to_key(seed, a.key)) { explicit_bzero(&a, sizeof a); return fail(c, MKT_ERR_STATE, "mkt_rlwe_partial_decrypt_batch: no entropy from the OS"); }
    hipError_t e = z.ring_keys(K, rk);
    a.party = party; a.N = N; a.W = p.W; a.kr = rk.count; a.npoly = 1 + c->sh.kacc; a.sigma = sigma_smudge; a.row0 = row0;
    a.poly0 = mkt::is_mk(p.scheme) ? 1 + party : 1; a.poly_step = mkt::is_mk(p.scheme) ? 0 : 1;
    a.rlwe = sx.dev; a.zring = z.as<const int8_t>(); a.out = so.dev; a.G = G;
    if (e == hipSuccess) e = mktd::launch_ring_share(a, c->stream);
    e = wipe_secrets(e, z, a);
    if (e != hipSuccess) return hipfail(c, e, "device ring share");
    return so.out(share_out);
}

int mkt_enable_timing(mkt_ctx *c, int on) {
    if (!c) return MKT_ERR_ARG;
    DevGuard dg(c->device);
    (void)hipStreamSynchronize(c->stream);
    clear_spans(c);
    c->timing = on != 0;
    return MKT_OK;
}

// sum of the recorded spans of class `which` since timing was enabled (ms); *ms / count = average launch
int mkt_last_kernel_ms(mkt_ctx *c, int which, double *ms) {
    if (!c || !ms) return MKT_ERR_ARG;
    if (!c->timing) return fail(c, MKT_ERR_STATE, "timing not enabled");
    DevGuard dg(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double tot = 0.0; int cnt = 0;
    for (auto &s : c->spans) if (s.cls == which) { float f = 0; if (hipEventElapsedTime(&f, s.a, s.b) == hipSuccess) { tot += f; cnt++; } }
    *ms = tot;
    return cnt;
}

}  // extern "C"
