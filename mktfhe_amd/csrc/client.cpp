// Client side of the boundary (host only, no GPU): key generation, encryption, decryption.
// Counterpart of the reference's setup / party_keygen / lwe_encrypt / lwe_ith_encrypt / lwe_decrypt /
// CRS (src/tfhe/scheme.jl:151-410, src/tfhe/keygen.jl, src/ciphertext/{lwe,lev,gsw,unienc,key}.jl).
// Randomness: ChaCha20 streams keyed by a 256-bit seed (rng_chacha.h); a NULL seed draws fresh entropy from
// the OS for that call, as the reference does per call (ChaCha20Stream, sampler.jl:1-34) -- pinned seeds are
// for tests and benchmarks only.  Difference by design: the RLWE products are exact integer arithmetic
// mod 2^W (the reference approximates them with a Float64x2 FFT, params.jl:1).  Keys leave in integer (coefficient)
// form; the device pre-transforms them (mkt_load_* with MKT_FMT_INT_COEFF).
#include <cmath>
#include <cstring>
#include <string.h>   // explicit_bzero
#include <functional>
#include <thread>

#include <sys/random.h>

#include "host_internal.h"
#include "rng_chacha.h"

namespace mkt {

int validate_params(const mkt_params &p, std::string &why) {
    auto bad = [&](const char *m) { why = m; return (int)MKT_ERR_ARG; };
    if (p.scheme < MKT_CGGI || p.scheme > MKT_KMS_BLOCK) return bad("unknown scheme");
    if (p.N < 16 || p.N > 4096 || (p.N & (p.N - 1))) return bad("N must be a power of two in [16, 4096]");
    if (p.W != 32 && p.W != 64) return bad("W must be 32 or 64");
    if (p.k < 1 || p.k > 64) return bad("k out of range");
    if (p.n < 1) return bad("n must be positive");
    if (p.f < 1 || p.logD < 1 || p.f * p.logD > 32 || p.logD > 5) return bad("bad key-switch gadget (f*logD <= 32, logD <= 5)");
    if (p.n + 1 > 16384) return bad("n too large");
    auto gadget = [&](int l, int logB) { return l >= 1 && logB >= 1 && logB <= 31 && l * logB <= p.W && l <= 32; };
    if (p.scheme == MKT_CCS) { if (!gadget(p.l_uni, p.logB_uni)) return bad("bad uni gadget"); }
    else if (!gadget(p.l_gsw, p.logB_gsw)) return bad("bad gsw gadget");
    if (is_kms(p.scheme) && (!gadget(p.l_lev, p.logB_lev) || !gadget(p.l_uni, p.logB_uni))) return bad("bad lev/uni gadget");
    if (is_block(p.scheme)) {
        if (p.blk_len < 1 || p.blk_d < 1 || p.blk_len * p.blk_d != p.n) return bad("block schemes need n == blk_len*blk_d");
    }
    if (p.scheme == MKT_KMS_BLOCK && p.n > p.N) return bad("KMS_block needs n <= N");
    return MKT_OK;
}

// 256-bit seed -> key words; NULL = fresh OS entropy (getrandom), never a fixed default
int seed_to_key(const uint8_t *seed, uint32_t key[8]) {
    uint8_t tmp[32];
    if (!seed) {
        size_t got = 0;
        while (got < sizeof tmp) {
            ssize_t r = getrandom(tmp + got, sizeof tmp - got, 0);
            if (r <= 0) return MKT_ERR_STATE;
            got += (size_t)r;
        }
        seed = tmp;
    }
    std::memcpy(key, seed, 32);
    explicit_bzero(tmp, sizeof tmp);
    return MKT_OK;
}

namespace {

using mktrng::Rng;

inline uint64_t wmask(int W) { return W == 64 ? ~0ull : ((1ull << W) - 1); }

// out (+)= a * s in Z[X]/(X^N+1), s with entries in {-1,0,1}
void mul_small_acc(const uint64_t *a, const int8_t *s, uint64_t *out, int N, bool negate) {
    for (int i = 0; i < N; i++) {
        if (!s[i]) continue;
        bool neg = (s[i] < 0) != negate;
        if (!neg) {
            for (int j = 0; j < N - i; j++) out[i + j] += a[j];
            for (int j = N - i; j < N; j++) out[i + j - N] -= a[j];
        } else {
            for (int j = 0; j < N - i; j++) out[i + j] -= a[j];
            for (int j = N - i; j < N; j++) out[i + j - N] += a[j];
        }
    }
}

struct RingKey { std::vector<std::vector<int8_t>> z; };  // k polynomials, binary

}  // namespace
}  // namespace mkt

using namespace mkt;

namespace {

// polynomial poly_index of an array of native-width polynomials <- v
void store_poly(void *dst, size_t poly_index, const uint64_t *v, int N, int W) {
    if (W == 64) std::memcpy((uint8_t *)dst + poly_index * N * 8, v, (size_t)N * 8);
    else { uint32_t *d = (uint32_t *)dst + poly_index * N; for (int i = 0; i < N; i++) d[i] = (uint32_t)v[i]; }
}
void load_poly(const void *src, size_t poly_index, uint64_t *v, int N, int W) {
    if (W == 64) std::memcpy(v, (const uint8_t *)src + poly_index * N * 8, (size_t)N * 8);
    else { const uint32_t *s = (const uint32_t *)src + poly_index * N; for (int i = 0; i < N; i++) v[i] = s[i]; }
}

// The one step under every generator: body = -sum_c a_c (*) z_c + e + message.  Its two halves:
// b = -sum_{c < kz} a_c (*) z[zoff + c]; mask(c) supplies the N ring words of a_c when it is their turn (a stream is drawn there, in order)
template <typename MASK>
void rlwe_body_acc(uint64_t *b, const std::vector<std::vector<int8_t>> &z, int zoff, int kz, int N, MASK mask) {
    std::fill(b, b + N, 0);
    for (int c = 0; c < kz; c++) mul_small_acc(mask(c), z[(size_t)zoff + c].data(), b, N, true);
}
// b[q] = (b[q] + e_q + msg(q)) mod 2^W, e_q the next N deviates of rng in coefficient order.  The sums are wrapping integers, so the order of
// the terms is free; the number and the order of the draws is not
template <typename MSG>
void add_noise(uint64_t *b, int N, int W, Rng &rng, double sigma, MSG msg) {
    const uint64_t m = wmask(W);
    for (int q = 0; q < N; q++) b[q] = (b[q] + rng.noise(sigma) + msg(q)) & m;
}
inline uint64_t no_message(int) { return 0; }

// RLWEsample (lwe.jl:78-93): a_c uniform, b = -sum a_c z_c + e + msg; polys laid out (b, a_0..a_{kz-1}) in out.  Draw order: mask c, then
// its product, for each c; then the N noise draws
template <typename MSG>
void rlwe_sample(Rng &rng, const std::vector<std::vector<int8_t>> &z, int zoff, int kz, double sigma, int N, int W, uint64_t *out, MSG msg) {
    const uint64_t m = wmask(W);
    rlwe_body_acc(out, z, zoff, kz, N, [&](int c) {
        uint64_t *a = out + (size_t)(1 + c) * N;
        for (int i = 0; i < N; i++) a[i] = rng.next() & m;
        return a;
    });
    add_noise(out, N, W, rng, sigma, msg);
}

// the ternary r of UniEnc (unienc.jl:36-55): the next N draws of rng, (draw mod 3) - 1
std::vector<int8_t> draw_ternary(Rng &rng, int N) {
    std::vector<int8_t> rt(N);
    for (int q = 0; q < N; q++) rt[q] = (int8_t)((int)(rng.next() % 3) - 1);
    return rt;
}
// the UniEnc row d = crs_j r + msg + e (unienc.jl:36-55), e the next N deviates of rng; a is scratch
template <typename MSG>
void unienc_d_row(const void *crs, int j, const int8_t *rt, Rng &rng, double sigma, int N, int W, uint64_t *a, uint64_t *d, MSG msg) {
    load_poly(crs, j, a, N, W);
    std::fill(d, d + N, 0);
    mul_small_acc(a, rt, d, N, false);                 // crs[j]*r
    add_noise(d, N, W, rng, sigma, msg);
}

// key-switching row (d, t) of the extracted coefficient z = z_c[j] carries ((d + 1) z) << (32 - (t + 1) logD)  (lev.jl:31-37)
inline uint32_t ksk_row_msg(int8_t z, int d, int t, int logD) { return (uint32_t)((uint32_t)z * (uint32_t)(d + 1)) << (32 - (t + 1) * logD); }
// the rows (c, j), cj = c N + j, a block scheme leaves out: inside the embedded LWE key (keygen.jl:46,:147)
inline bool ksk_row_absent(const mkt_params &p, long cj) { return is_block(p.scheme) && cj < p.n; }

// the checked opening of an entry point: valid parameters and one of their parties -> the shape; MKT_ERR_ARG otherwise.  Calls that take
// every party at once open with party 0
int open_party(const mkt_params *params, int party, Shape &sh) {
    std::string why;
    if (!params || validate_params(*params, why)) return MKT_ERR_ARG;
    sh = shape_of(*params);
    return party < 0 || party >= sh.nparty ? (int)MKT_ERR_ARG : (int)MKT_OK;
}

void parallel_for(int n, const std::function<void(int)> &fn) {
    unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)(hw ? hw : 4); if (nt > 16) nt = 16; if (nt > n) nt = n; if (nt < 1) nt = 1;
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back([=, &fn] { for (int i = t; i < n; i += nt) fn(i); });
    for (auto &x : th) x.join();
}
}  // namespace

extern "C" {

int mkt_make_twiddles(int N, int which, double *out_host) {
    if (!out_host || which < 0 || which > 3 || N < 4 || N > 8192 || (N & (N - 1))) return MKT_ERR_ARG;
    Twiddles tw;
    make_twiddles(N, tw);
    const std::vector<double> &v = which == 0 ? tw.psi : which == 1 ? tw.psiinv : which == 2 ? tw.roots : tw.rootsinv;
    std::memcpy(out_host, v.data(), v.size() * sizeof(double));
    return MKT_OK;
}

// a fresh 256-bit seed from the OS (what a NULL seed argument uses internally)
int mkt_client_random_seed(uint8_t out[32]) {
    if (!out) return MKT_ERR_ARG;
    uint32_t key[8];
    if (seed_to_key(nullptr, key)) return MKT_ERR_STATE;
    std::memcpy(out, key, 32);
    explicit_bzero(key, sizeof key);
    return MKT_OK;
}

// TESTS AND BENCHMARKS ONLY: expands a small integer into a 256-bit seed so that keys and ciphertexts are
// reproducible.  Anything encrypted under such a seed is public.
int mkt_client_test_seed(uint64_t n, uint8_t out[32]) {
    if (!out) return MKT_ERR_ARG;
    uint64_t x = n ^ 0x6D6B746668655F74ull;
    for (int i = 0; i < 4; i++) {   // splitmix64
        uint64_t z = (x += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        std::memcpy(out + 8 * i, &z, 8);
    }
    return MKT_OK;
}

int mkt_client_crs(const mkt_params *params, const uint8_t *seed, void *crs_out) {
    Shape sh;
    if (!crs_out || open_party(params, 0, sh)) return MKT_ERR_ARG;
    const mkt_params &p = *params;
    if (!is_mk(p.scheme)) return MKT_ERR_ARG;
    uint32_t key[8];
    if (seed_to_key(seed, key)) return MKT_ERR_STATE;
    Rng rng(key, 0, 0xC125);
    uint64_t m = wmask(p.W);
    for (size_t i = 0; i < (size_t)p.l_uni * p.N; i++) {   // scheme.jl:409-410
        uint64_t v = rng.next() & m;
        if (p.W == 64) ((uint64_t *)crs_out)[i] = v; else ((uint32_t *)crs_out)[i] = (uint32_t)v;
    }
    explicit_bzero(key, sizeof key);
    return MKT_OK;
}

}  // extern "C"

// heavy = false: secrets and the small keys only (public key, relinearisation key); the bootstrapping and
// key-switching keys are then generated on the device (mkt_keygen_device) from the same seeded streams
static int party_keygen_impl(const mkt_params *params, const uint8_t *seed, int party, const void *crs,
                             double sigma_lwe, double sigma_ring, bool heavy, mkt_client_party **out) {
    Shape sh;
    if (!out || open_party(params, party, sh)) return MKT_ERR_ARG;
    const mkt_params &p = *params;
    if (is_mk(p.scheme) && !crs) return MKT_ERR_ARG;
    const int N = p.N, n = p.n, W = p.W;
    auto *K = new mkt_client_party();
    K->p = p; K->sh = sh; K->party = party;
    if (seed_to_key(seed, K->key)) { delete K; return MKT_ERR_STATE; }
    const uint32_t *ps = K->key; const uint32_t pa = (uint32_t)party;   // stream key, party index (in the nonce)
    K->sigma_lwe = sigma_lwe; K->sigma_ring = sigma_ring; K->heavy = heavy;

    // ---- secret keys: key.jl:12-19 (binary), sampler.jl:7-21 (block binary), key.jl:52-87 (partial ring key)
    {
        Rng r(ps, pa, 1);
        K->lwekey.assign(n, 0);
        if (is_block(p.scheme)) {
            for (int i = 0; i < p.blk_d; i++) {
                int idx = (int)(r.next() % (uint64_t)(p.blk_len + 1));   // rand(0:l)
                if (idx) K->lwekey[(size_t)i * p.blk_len + idx - 1] = 1;
            }
        } else for (int i = 0; i < n; i++) K->lwekey[i] = (uint32_t)(r.next() >> 63);
        auto binary_poly = [&](std::vector<int8_t> &z) { z.assign(N, 0); for (int i = 0; i < N; i++) z[i] = (int8_t)(r.next() >> 63); };
        auto partial = [&](std::vector<std::vector<int8_t>> &zs, int kz) {   // ring key embeds the LWE key (key.jl:52-69)
            zs.resize(kz);
            for (int c = 0; c < kz; c++) { binary_poly(zs[c]); for (int i = 0; i < N; i++) { long g = (long)c * N + i; if (g < n) zs[c][i] = (int8_t)K->lwekey[g]; } }
        };
        if (p.scheme == MKT_CGGI) { K->zring.resize(p.k); for (auto &z : K->zring) binary_poly(z); }
        else if (p.scheme == MKT_LMSS) partial(K->zring, p.k);
        else if (p.scheme == MKT_CCS) { K->zring.resize(1); binary_poly(K->zring[0]); }
        else if (p.scheme == MKT_KMS) { K->zring.resize(2); binary_poly(K->zring[0]); binary_poly(K->zring[1]); }
        else { K->zring.resize(2); binary_poly(K->zring[0]); std::vector<std::vector<int8_t>> u; partial(u, 1); K->zring[1] = u[0]; }
    }

    // ---- bootstrapping key
    if (!heavy) {
    } else if (p.scheme != MKT_CCS) {
        // brk[i] = RGSW_z(s_i): keygen.jl:13-15,:39-41,:106-108,:143-145; gsw.jl:174-178; lev.jl:88-102
        const int kr = sh.kr, l = p.l_gsw, rows = (kr + 1) * l, polys = kr + 1;
        K->brk.assign((size_t)n * rows * polys * N * sh.word, 0);
        parallel_for(n, [&](int i) {
            std::vector<uint64_t> buf((size_t)polys * N);
            for (int c = 0; c <= kr; c++) for (int j = 0; j < l; j++) {
                Rng r(ps, pa, 2, (uint32_t)i, (uint32_t)(c * l + j));
                rlwe_sample(r, K->zring, 0, kr, sigma_ring, N, W, buf.data(), no_message);
                uint64_t g = 1ull << (W - (j + 1) * p.logB_gsw);
                buf[(size_t)c * N] = (buf[(size_t)c * N] + (uint64_t)K->lwekey[i] * g) & wmask(W);  // c = 0: b[0]; c >= 1: a_{c-1}[0]
                for (int q = 0; q < polys; q++)
                    store_poly(K->brk.data(), ((size_t)i * rows + (size_t)c * l + j) * polys + q, buf.data() + (size_t)q * N, N, W);
            }
        });
    } else {
        // brk[i] = UniEnc_z(s_i): keygen.jl:71-73; unienc.jl:36-55
        const int l = p.l_uni;
        K->brk.assign((size_t)n * 3 * l * N * sh.word, 0);
        parallel_for(n, [&](int i) {
            Rng r(ps, pa, 2, (uint32_t)i);
            const std::vector<int8_t> rt = draw_ternary(r, N);
            std::vector<uint64_t> a(N), d(N), rl((size_t)2 * N);
            for (int j = 0; j < l; j++) {
                uint64_t g = 1ull << (W - (j + 1) * p.logB_uni);
                unienc_d_row(crs, j, rt.data(), r, sigma_ring, N, W, a.data(), d.data(), [&](int q) { return q ? 0 : (uint64_t)K->lwekey[i] * g; });
                store_poly(K->brk.data(), (size_t)i * 3 * l + j, d.data(), N, W);
                rlwe_sample(r, K->zring, 0, 1, sigma_ring, N, W, rl.data(), [&](int q) { return g * (uint64_t)(int64_t)rt[q]; });   // f.stack[j] = RLWE_z(g_j * r)
                store_poly(K->brk.data(), (size_t)i * 3 * l + l + 2 * j, rl.data(), N, W);
                store_poly(K->brk.data(), (size_t)i * 3 * l + l + 2 * j + 1, rl.data() + N, N, W);
            }
        });
    }

    // ---- CCS/KMS: public key b (unienc.jl:77-90) and KMS relinearisation key (keygen.jl:103)
    if (is_mk(p.scheme)) {
        const int l = p.l_uni;
        const int zi = is_kms(p.scheme) ? 1 : 0;   // uni key
        K->pub.assign((size_t)l * N * sh.word, 0);
        std::vector<uint64_t> a(N), b(N);
        Rng r(ps, pa, 3);
        for (int j = 0; j < l; j++) {
            rlwe_body_acc(b.data(), K->zring, zi, 1, N, [&](int) { load_poly(crs, j, a.data(), N, W); return a.data(); });   // -z*crs[j]
            add_noise(b.data(), N, W, r, sigma_ring, no_message);
            store_poly(K->pub.data(), j, b.data(), N, W);
        }
        if (is_kms(p.scheme)) {
            K->rlk_d.assign((size_t)l * N * sh.word, 0);
            K->rlk_f.assign((size_t)l * 2 * N * sh.word, 0);
            Rng r2(ps, pa, 4);
            const std::vector<int8_t> rt = draw_ternary(r2, N);
            std::vector<uint64_t> d(N), rl((size_t)2 * N);
            for (int j = 0; j < l; j++) {
                uint64_t g = 1ull << (W - (j + 1) * p.logB_uni);
                unienc_d_row(crs, j, rt.data(), r2, sigma_ring, N, W, a.data(), d.data(), [&](int q) { return g * (uint64_t)K->zring[0][q]; });  // + g_j * z'
                store_poly(K->rlk_d.data(), j, d.data(), N, W);
                rlwe_sample(r2, K->zring, 1, 1, sigma_ring, N, W, rl.data(), [&](int q) { return g * (uint64_t)(int64_t)rt[q]; });
                store_poly(K->rlk_f.data(), 2 * j, rl.data(), N, W);
                store_poly(K->rlk_f.data(), 2 * j + 1, rl.data() + N, N, W);
            }
        }
    }

    // ---- key-switching key: keygen.jl:17-23,:43-51,:75-79,:110-114,:147-151; lev.jl:31-37; lwe.jl:11-22
    if (heavy) {
        const int f = p.f, logD = p.logD, dr = sh.ksk_drows, kk = sh.ksk_kr;
        const int zoff = is_kms(p.scheme) ? 1 : 0;
        const size_t n1 = (size_t)n + 1;
        K->ksk.assign((size_t)kk * N * dr * f * n1, 0);
        parallel_for(kk * N, [&](int cj) {
            int c = cj / N, j = cj % N;
            if (ksk_row_absent(p, cj)) return;
            Rng r(ps, pa, 5, (uint32_t)cj);
            for (int d = 0; d < dr; d++) for (int t = 0; t < f; t++) {
                uint32_t *row = K->ksk.data() + ((((size_t)c * N + j) * dr + d) * f + t) * n1;
                uint32_t msg = ksk_row_msg(K->zring[zoff + c][j], d, t, logD);
                uint32_t dot = 0;
                for (int q = 0; q < n; q++) { row[q] = (uint32_t)r.next(); dot += row[q] * K->lwekey[q]; }
                row[n] = (uint32_t)r.noise(sigma_lwe) - dot + msg;
            }
        });
    }
    *out = K;
    return MKT_OK;
}

extern "C" {

int mkt_client_party_keygen(const mkt_params *params, const uint8_t *seed, int party, const void *crs,
                            double sigma_lwe, double sigma_ring, mkt_client_party **out) {
    return party_keygen_impl(params, seed, party, crs, sigma_lwe, sigma_ring, true, out);
}

int mkt_client_party_secrets(const mkt_params *params, const uint8_t *seed, int party, const void *crs,
                             double sigma_lwe, double sigma_ring, mkt_client_party **out) {
    return party_keygen_impl(params, seed, party, crs, sigma_lwe, sigma_ring, false, out);
}

int mkt_client_party_destroy(mkt_client_party *p) {
    if (!p) return MKT_OK;
    // wipe the secrets before the memory goes back to the allocator
    explicit_bzero(p->key, sizeof p->key);
    if (!p->lwekey.empty()) explicit_bzero(p->lwekey.data(), p->lwekey.size() * sizeof(uint32_t));
    for (auto &z : p->zring) if (!z.empty()) explicit_bzero(z.data(), z.size());
    delete p;
    return MKT_OK;
}
const uint32_t *mkt_client_lwekey(const mkt_client_party *p) { return p ? p->lwekey.data() : nullptr; }
// ring secret key polynomial idx (SK schemes: idx < k; CCS: 0; KMS: 0 = gsw key z', 1 = uni key z), N entries 0/1
const int8_t *mkt_client_ringkey(const mkt_client_party *p, int idx, size_t *bytes) {
    if (!p || idx < 0 || idx >= (int)p->zring.size()) { if (bytes) *bytes = 0; return nullptr; }
    if (bytes) *bytes = p->zring[idx].size();
    return p->zring[idx].data();
}
const void *mkt_client_brk(const mkt_client_party *p, size_t *bytes) { if (bytes) *bytes = p->brk.size(); return p->brk.data(); }
const uint32_t *mkt_client_ksk(const mkt_client_party *p, size_t *bytes) { if (bytes) *bytes = p->ksk.size() * 4; return p->ksk.data(); }
const void *mkt_client_rlk_d(const mkt_client_party *p, size_t *bytes) { if (bytes) *bytes = p->rlk_d.size(); return p->rlk_d.data(); }
const void *mkt_client_rlk_f(const mkt_client_party *p, size_t *bytes) { if (bytes) *bytes = p->rlk_f.size(); return p->rlk_f.data(); }
const void *mkt_client_pubkey(const mkt_client_party *p, size_t *bytes) { if (bytes) *bytes = p->pub.size(); return p->pub.data(); }

// scheme.jl:352-386 lwe_encrypt / lwe_ith_encrypt with ANY torus message: b = e - <a,s> + mu, mask in the party's block
int mkt_client_lwe_encrypt_word(const mkt_params *params, const mkt_client_party *K, int party, uint32_t mu,
                                double sigma_lwe, const uint8_t *seed, uint32_t *out) {
    if (!params || !K || !out) return MKT_ERR_ARG;
    const mkt_params &p = *params;
    Shape sh = shape_of(p);
    if (party < 0 || party >= sh.nparty) return MKT_ERR_ARG;
    std::memset(out, 0, sizeof(uint32_t) * (size_t)sh.lwe_len);
    uint32_t key[8];
    if (seed_to_key(seed, key)) return MKT_ERR_STATE;
    Rng r(key, (uint32_t)party, 7);
    uint32_t *a = out + (size_t)party * p.n;
    uint32_t dot = 0;
    uint32_t e = (uint32_t)r.noise(sigma_lwe);
    for (int i = 0; i < p.n; i++) { a[i] = (uint32_t)r.next(); dot += a[i] * K->lwekey[i]; }
    out[sh.lwe_len - 1] = e + (0u - dot + mu);
    explicit_bzero(key, sizeof key);
    return MKT_OK;
}

// the reference's bit encryption: the message (2m - 1) 2^29
int mkt_client_lwe_encrypt(const mkt_params *params, const mkt_client_party *K, int party, int bit,
                           double sigma_lwe, const uint8_t *seed, uint32_t *out) {
    return mkt_client_lwe_encrypt_word(params, K, party, (uint32_t)(2 * (bit ? 1 : 0) - 1) << 29, sigma_lwe, seed, out);
}

// the phase lwe_decrypt decides on (scheme.jl:388-407 before its rounding): b + sum_i <a_i, s_i>, message + noise on the 32-bit torus
int mkt_client_lwe_phase(const mkt_params *params, const mkt_client_party *const *keys, int nparties, const uint32_t *lwe, uint32_t *phase) {
    if (!params || !keys || !lwe || !phase) return MKT_ERR_ARG;
    const mkt_params &p = *params;
    Shape sh = shape_of(p);
    if (nparties != sh.nparty) return MKT_ERR_ARG;
    uint32_t b = lwe[sh.lwe_len - 1];
    for (int i = 0; i < nparties; i++) {
        if (!keys[i]) return MKT_ERR_ARG;
        for (int q = 0; q < p.n; q++) b += keys[i]->lwekey[q] * lwe[(size_t)i * p.n + q];
    }
    *phase = b;
    return MKT_OK;
}

// the bit a phase decides (scheme.jl:388-407 after the sum): shared by mkt_client_lwe_decrypt and mkt_client_merge_decrypt
static int bit_of_phase(const mkt_params &p, uint32_t b) {
    if (!is_mk(p.scheme)) {                       // divbits(phase, 29) == 1
        uint32_t carry = (b << 3) >> 31;
        return ((b >> 29) + carry) == 1 ? 1 : 0;
    }
    return b < (1u << 31) ? 1 : 0;
}

// b + the k shares of row j; shares [nparty][B]
static uint32_t merged_phase(const Shape &sh, const uint32_t *lwe, const uint32_t *shares, size_t B, size_t j) {
    uint32_t b = lwe[j * (size_t)sh.lwe_len + sh.lwe_len - 1];
    for (int i = 0; i < sh.nparty; i++) b += shares[(size_t)i * B + j];
    return b;
}

// scheme.jl:388-407
int mkt_client_lwe_decrypt(const mkt_params *params, const mkt_client_party *const *keys, int nparties, const uint32_t *lwe) {
    uint32_t b;
    if (int r = mkt_client_lwe_phase(params, keys, nparties, lwe, &b)) return r;
    return bit_of_phase(*params, b);
}

// ---- distributed decryption (mktfhe.h): a share per party from its own mask block, merged by anyone ----

// share_i[j] = <a_i, s_i> + e_i[j], e_i[j] the smudging noise of row row0 + j (rng_chacha.h smudge_word)
int mkt_client_partial_decrypt(const mkt_params *params, const mkt_client_party *K, int party, const uint32_t *lwe, double sigma_smudge,
                               const uint8_t *seed, uint64_t row0, uint32_t *share_out, size_t B) {
    if (!params || !K || !lwe || !share_out || !smudge_sigma_ok(sigma_smudge)) return MKT_ERR_ARG;
    const mkt_params &p = *params;
    Shape sh = shape_of(p);
    if (party < 0 || party >= sh.nparty) return MKT_ERR_ARG;
    if (!party_keys_match(K, p, party)) return MKT_ERR_ARG;   // (as mkt_keygen_device)
    uint32_t key[8];
    if (seed_to_key(seed, key)) return MKT_ERR_STATE;
    for (size_t j = 0; j < B; j++) {
        const uint32_t *a = lwe + j * (size_t)sh.lwe_len + (size_t)party * p.n;
        uint32_t dot = 0;
        for (int q = 0; q < p.n; q++) dot += a[q] * K->lwekey[q];
        share_out[j] = dot + mktrng::smudge_word(key, (uint32_t)party, row0 + j, sigma_smudge);
    }
    explicit_bzero(key, sizeof key);
    return MKT_OK;
}

// phase[j] = b[j] + sum_i share_i[j]; shares [nparty][B]
int mkt_client_merge_phase(const mkt_params *params, const uint32_t *lwe, const uint32_t *shares, int nparties, uint32_t *phase_out, size_t B) {
    if (!params || !lwe || !shares || !phase_out) return MKT_ERR_ARG;
    Shape sh = shape_of(*params);
    if (nparties != sh.nparty) return MKT_ERR_ARG;
    for (size_t j = 0; j < B; j++) phase_out[j] = merged_phase(sh, lwe, shares, B, j);
    return MKT_OK;
}

// the bit mkt_client_lwe_decrypt decides from that phase
int mkt_client_merge_decrypt(const mkt_params *params, const uint32_t *lwe, const uint32_t *shares, int nparties, uint8_t *bits_out, size_t B) {
    if (!params || !lwe || !shares || !bits_out) return MKT_ERR_ARG;
    Shape sh = shape_of(*params);
    if (nparties != sh.nparty) return MKT_ERR_ARG;
    for (size_t j = 0; j < B; j++) bits_out[j] = (uint8_t)bit_of_phase(*params, merged_phase(sh, lwe, shares, B, j));
    return MKT_OK;
}

// ---- seeded ciphertexts (mktfhe.h): a public mask seed and one body word per row; these two functions are the definition ----

// body[j] = e[j] - <a[j], s> + mu[j], a[j] the n mask words of row row0 + j (rng_chacha.h mask_block), e[j] its noise word on stream 11
int mkt_client_seeded_encrypt(const mkt_params *params, const mkt_client_party *K, int party, const uint32_t *mu, double sigma_lwe,
                              const uint8_t *mask_seed, const uint8_t *noise_seed, uint64_t row0, uint32_t *body_out, size_t B) {
    if (!params || !K || !mask_seed || !smudge_sigma_ok(sigma_lwe)) return MKT_ERR_ARG;
    if (noise_seed && std::memcmp(noise_seed, mask_seed, 32) == 0) return MKT_ERR_ARG;    // the mask seed is published: the noise would be too
    const mkt_params &p = *params;
    Shape sh = shape_of(p);
    if (party < 0 || party >= sh.nparty) return MKT_ERR_ARG;
    if (!party_keys_match(K, p, party)) return MKT_ERR_ARG;
    if (!B) return MKT_OK;
    if (!mu || !body_out) return MKT_ERR_ARG;
    uint32_t mkey[8], nkey[8];
    seed_to_key(mask_seed, mkey);
    if (seed_to_key(noise_seed, nkey)) return MKT_ERR_STATE;
    for (size_t j = 0; j < B; j++) {
        uint32_t dot = 0, a[16];
        for (int q0 = 0; q0 < p.n; q0 += 16) {
            mktrng::mask_block(mkey, (uint32_t)party, row0 + j, (uint32_t)(q0 >> 4), a);
            for (int i = 0; i < 16 && q0 + i < p.n; i++) dot += a[i] * K->lwekey[q0 + i];
        }
        body_out[j] = mktrng::row_noise_word(nkey, (uint32_t)party, mktrng::STREAM_ENC_NOISE, row0 + j, sigma_lwe) + (0u - dot + mu[j]);
    }
    explicit_bzero(nkey, sizeof nkey);
    return MKT_OK;
}

// row j = zeros, the mask of row row0 + j in block `party`, body[j] last: an ordinary ciphertext; needs no key
int mkt_client_seeded_expand(const mkt_params *params, int party, const uint8_t *mask_seed, uint64_t row0, const uint32_t *body, uint32_t *out, size_t B) {
    if (!params || !mask_seed) return MKT_ERR_ARG;
    const mkt_params &p = *params;
    Shape sh = shape_of(p);
    if (p.n < 1 || party < 0 || party >= sh.nparty) return MKT_ERR_ARG;
    if (!B) return MKT_OK;
    if (!body || !out) return MKT_ERR_ARG;
    uint32_t mkey[8];
    seed_to_key(mask_seed, mkey);
    for (size_t j = 0; j < B; j++) {
        uint32_t *row = out + j * (size_t)sh.lwe_len, a[16];
        std::memset(row, 0, sizeof(uint32_t) * (size_t)sh.lwe_len);
        for (int q0 = 0; q0 < p.n; q0 += 16) {
            mktrng::mask_block(mkey, (uint32_t)party, row0 + j, (uint32_t)(q0 >> 4), a);
            for (int i = 0; i < 16 && q0 + i < p.n; i++) row[(size_t)party * p.n + q0 + i] = a[i];
        }
        row[sh.lwe_len - 1] = body[j];
    }
    return MKT_OK;
}

}  // extern "C"

// ---- seeded evaluation keys (mktfhe.h): a public mask seed and the bodies of the two large keys; these functions are the definition ----

namespace {

// the mask polynomial at index `idx` of a public stream as ring words: every keystream word used, 16 coefficients of a block on the 32-bit
// ring, 8 on the 64-bit one (low word first)
void mask_poly(const uint32_t mkey[8], uint32_t stream, uint32_t party, uint64_t idx, int N, int W, uint64_t *a) {
    uint32_t w[16];
    if (W == 32) for (int q0 = 0; q0 < N; q0 += 16) {
        mktrng::stream_block(mkey, stream, party, idx, (uint32_t)(q0 >> 4), w);
        for (int i = 0; i < 16; i++) a[q0 + i] = w[i];
    } else for (int q0 = 0; q0 < N; q0 += 8) {
        mktrng::stream_block(mkey, stream, party, idx, (uint32_t)(q0 >> 3), w);
        for (int i = 0; i < 8; i++) a[q0 + i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
    }
}
// mask polynomial P of the bootstrapping key (stream 13) as ring words
void brk_mask_poly(const uint32_t mkey[8], uint32_t party, uint64_t P, int N, int W, uint64_t *a) {
    mask_poly(mkey, mktrng::STREAM_BRK_MASK, party, P, N, W, a);
}
// the n mask words of key-switching-key row R (stream 12)
void ksk_mask_row(const uint32_t mkey[8], uint32_t party, uint64_t R, int n, uint32_t *row) {
    uint32_t w[16];
    for (int q0 = 0; q0 < n; q0 += 16) {
        mktrng::stream_block(mkey, mktrng::STREAM_KSK_MASK, party, R, (uint32_t)(q0 >> 4), w);
        for (int i = 0; i < 16 && q0 + i < n; i++) row[q0 + i] = w[i];
    }
}
// sample S of an expanded key (b, a_0 .. a_{kz-1}): the body as it was shipped, the kz masks mask(c) regenerated behind it
template <typename MASK>
void expand_sample(void *out, size_t S, const void *bodies, int kz, int N, int W, MASK mask) {
    const size_t pb = (size_t)N * (W / 8);
    std::memcpy((uint8_t *)out + S * (kz + 1) * pb, (const uint8_t *)bodies + S * pb, pb);
    for (int c = 0; c < kz; c++) store_poly(out, S * (kz + 1) + 1 + c, mask(c), N, W);
}

}  // namespace

extern "C" {

int mkt_client_party_keygen_seeded(const mkt_params *params, const uint8_t *seed, const uint8_t *mask_seed, int party, const void *crs,
                                   double sigma_lwe, double sigma_ring, mkt_client_party **out) {
    if (!mask_seed) return MKT_ERR_ARG;
    if (seed && std::memcmp(seed, mask_seed, 32) == 0) return MKT_ERR_ARG;      // the mask seed is published: the secrets would be too
    mkt_client_party *K = nullptr;
    if (int r = party_keygen_impl(params, seed, party, crs, sigma_lwe, sigma_ring, false, &K)) return r;
    const mkt_params &p = K->p;
    const Shape &sh = K->sh;
    const int N = p.N, n = p.n, W = p.W;
    const uint32_t *ps = K->key; const uint32_t pa = (uint32_t)party;
    uint32_t mkey[8];
    seed_to_key(mask_seed, mkey);
    K->seeded = true;
    std::memcpy(K->mask_seed, mask_seed, 32);
    K->brk_seeded.assign(brk_seeded_polys(p, sh) * N * sh.word, 0);
    if (p.scheme != MKT_CCS) {
        // RGSW_z(s_i) with the message in the body: row (c, j) is (b, a_0 ..) with the a_cc the public masks as they are and
        // b = -sum a_cc z_cc + e + s_i g_j m_c, m_0 = 1, m_c = z_{c-1}: the phase of gsw.jl:174-178, which adds s_i g_j to a_{c-1}[0]
        const int kr = sh.kr, l = p.l_gsw, rows = (kr + 1) * l;
        parallel_for(n, [&](int i) {
            std::vector<uint64_t> a(N), b(N);
            for (int c = 0; c <= kr; c++) for (int j = 0; j < l; j++) {
                const uint64_t S = (uint64_t)i * rows + (uint64_t)c * l + j;
                rlwe_body_acc(b.data(), K->zring, 0, kr, N, [&](int cc) { brk_mask_poly(mkey, pa, S * kr + cc, N, W, a.data()); return a.data(); });
                Rng r(ps, pa, mktrng::STREAM_BRK_NOISE, (uint32_t)S, (uint32_t)(S >> 32));
                const uint64_t g = (uint64_t)K->lwekey[i] << (W - (j + 1) * p.logB_gsw);
                add_noise(b.data(), N, W, r, sigma_ring, [&](int q) { return g * (c == 0 ? (q == 0 ? 1u : 0u) : (uint64_t)K->zring[c - 1][q]); });
                store_poly(K->brk_seeded.data(), S, b.data(), N, W);
            }
        });
    } else {
        // UniEnc_z(s_i): d_j = crs_j r + s_i g_j + e ships whole (its "mask" is the common CRS); f_j = RLWE_z(g_j r) ships its body
        const int l = p.l_uni;
        parallel_for(n, [&](int i) {
            Rng r(ps, pa, mktrng::STREAM_UNI_NOISE, (uint32_t)i);
            const std::vector<int8_t> rt = draw_ternary(r, N);
            std::vector<uint64_t> a(N), d(N);
            for (int j = 0; j < l; j++) {
                const uint64_t g = 1ull << (W - (j + 1) * p.logB_uni);
                unienc_d_row(crs, j, rt.data(), r, sigma_ring, N, W, a.data(), d.data(), [&](int q) { return q ? 0 : (uint64_t)K->lwekey[i] * g; });
                store_poly(K->brk_seeded.data(), (size_t)i * 2 * l + j, d.data(), N, W);
                rlwe_body_acc(d.data(), K->zring, 0, 1, N, [&](int) { brk_mask_poly(mkey, pa, (uint64_t)i * l + j, N, W, a.data()); return a.data(); });
                add_noise(d.data(), N, W, r, sigma_ring, [&](int q) { return g * (uint64_t)(int64_t)rt[q]; });
                store_poly(K->brk_seeded.data(), (size_t)i * 2 * l + l + j, d.data(), N, W);
            }
        });
    }
    {
        const int f = p.f, logD = p.logD, dr = sh.ksk_drows, kk = sh.ksk_kr;
        const int zoff = is_kms(p.scheme) ? 1 : 0;
        K->ksk_seeded.assign(ksk_rows(p, sh), 0);
        parallel_for(kk * N, [&](int cj) {
            if (ksk_row_absent(p, cj)) return;
            const int c = cj / N, j = cj % N;
            std::vector<uint32_t> row(n);
            for (int d = 0; d < dr; d++) for (int t = 0; t < f; t++) {
                const uint64_t R = ((uint64_t)cj * dr + d) * f + t;
                const uint32_t msg = ksk_row_msg(K->zring[zoff + c][j], d, t, logD);
                ksk_mask_row(mkey, pa, R, n, row.data());
                uint32_t dot = 0;
                for (int q = 0; q < n; q++) dot += row[q] * K->lwekey[q];
                K->ksk_seeded[R] = mktrng::row_noise_word(ps, pa, mktrng::STREAM_KSK_NOISE, R, sigma_lwe) - dot + msg;
            }
        });
    }
    *out = K;
    return MKT_OK;
}

const void *mkt_client_brk_seeded(const mkt_client_party *p, size_t *bytes) { if (bytes) *bytes = p ? p->brk_seeded.size() : 0; return p ? p->brk_seeded.data() : nullptr; }
const uint32_t *mkt_client_ksk_seeded(const mkt_client_party *p, size_t *bytes) { if (bytes) *bytes = p ? p->ksk_seeded.size() * 4 : 0; return p ? p->ksk_seeded.data() : nullptr; }
const uint8_t *mkt_client_mask_seed(const mkt_client_party *p) { return p && p->seeded ? p->mask_seed : nullptr; }

// the ordinary keys of a seeded party: the layouts of mkt_load_brk (MKT_FMT_INT_COEFF) and mkt_load_ksk; needs no key
int mkt_client_seeded_keys_expand(const mkt_params *params, int party, const uint8_t *mask_seed, const void *brk_seeded, const uint32_t *ksk_seeded,
                                  void *brk_out, uint32_t *ksk_out) {
    Shape sh;
    if (!mask_seed || open_party(params, party, sh)) return MKT_ERR_ARG;
    const mkt_params &p = *params;
    if (!brk_seeded != !brk_out || !ksk_seeded != !ksk_out) return MKT_ERR_ARG;
    const int N = p.N, n = p.n, W = p.W;
    const uint32_t pa = (uint32_t)party;
    uint32_t mkey[8];
    seed_to_key(mask_seed, mkey);
    const size_t pb = (size_t)N * sh.word;
    if (brk_out && p.scheme != MKT_CCS) {
        const int kr = sh.kr;
        const size_t samples = (size_t)n * (kr + 1) * p.l_gsw;
        parallel_for((int)samples, [&](int S) {
            std::vector<uint64_t> a(N);
            expand_sample(brk_out, (size_t)S, brk_seeded, kr, N, W, [&](int cc) { brk_mask_poly(mkey, pa, (uint64_t)S * kr + cc, N, W, a.data()); return a.data(); });
        });
    } else if (brk_out) {
        const int l = p.l_uni;
        parallel_for(n, [&](int i) {
            std::vector<uint64_t> a(N);
            const uint8_t *src = (const uint8_t *)brk_seeded + (size_t)i * 2 * l * pb;
            uint8_t *o = (uint8_t *)brk_out + (size_t)i * 3 * l * pb;
            std::memcpy(o, src, (size_t)l * pb);                       // the d_j as they are; behind them the f_j are l samples of one mask each
            for (int j = 0; j < l; j++)
                expand_sample(o + (size_t)l * pb, (size_t)j, src + (size_t)l * pb, 1, N, W, [&](int) { brk_mask_poly(mkey, pa, (uint64_t)i * l + j, N, W, a.data()); return a.data(); });
        });
    }
    if (ksk_out) {
        const size_t per = (size_t)sh.ksk_drows * p.f, n1 = (size_t)n + 1;
        parallel_for(sh.ksk_kr * N, [&](int cj) {
            for (size_t u = 0; u < per; u++) {
                const uint64_t R = (uint64_t)cj * per + u;
                uint32_t *row = ksk_out + R * n1;
                if (ksk_row_absent(p, cj)) { std::memset(row, 0, n1 * 4); continue; }
                ksk_mask_row(mkey, pa, R, n, row);
                row[n] = ksk_seeded[R];
            }
        });
    }
    return MKT_OK;
}

}  // extern "C"

// ---- packed outputs (mktfhe_pack.h): the packing key, and the ring forms of the phase, the decryption share and the merge ----

namespace {

// the ring keys a packed ciphertext is under (the ones the key-switching key switches from): first ring-key polynomial of a party, how many
inline int pack_zoff(const mkt_params &p) { return is_kms(p.scheme) ? 1 : 0; }
// mask polynomial P of a party's packing key (stream 19, the gadget in the high index word) as ring words, into a
const uint64_t *pack_mask_poly(const uint32_t mkey[8], int party, uint32_t P, int l_pk, int logB_pk, int N, int W, uint64_t *a) {
    mask_poly(mkey, mktrng::STREAM_PACK_MASK, (uint32_t)party, mktrng::pack_mask_index(P, l_pk, logB_pk), N, W, a);
    return a;
}
// acc += sum_c a_{slot(party, c)} (*) z_{party, c} for one party's components of one packed ciphertext [1 + k][N]
void ring_share_acc(const mkt_params &p, const Shape &sh, const mkt_client_party *K, int party, const void *rlwe, uint64_t *acc, uint64_t *a) {
    for (int c = 0; c < sh.ksk_kr; c++) {
        load_poly(rlwe, (size_t)1 + (is_mk(p.scheme) ? party : c), a, p.N, p.W);
        mul_small_acc(a, K->zring[(size_t)pack_zoff(p) + c].data(), acc, p.N, false);
    }
}

}  // namespace

extern "C" {

// row (q, t) = RLWE_z(s[q] g_t): rlev_encrypt (lev.jl:88-94) of the constant s[q]; one stream per row
int mkt_client_packing_keygen(const mkt_params *params, const mkt_client_party *K, int party, int l_pk, int logB_pk, const uint8_t *seed, void *pk_out) {
    Shape sh;
    if (!K || !pk_out || !pack_gadget_ok(l_pk, logB_pk) || open_party(params, party, sh)) return MKT_ERR_ARG;
    const mkt_params &p = *params;
    if (!party_keys_match(K, p, party)) return MKT_ERR_ARG;
    const int N = p.N, W = p.W, kr = sh.ksk_kr, polys = kr + 1;
    uint32_t key[8];
    if (seed_to_key(seed, key)) return MKT_ERR_STATE;
    parallel_for(p.n, [&](int q) {
        std::vector<uint64_t> buf((size_t)polys * N);
        for (int t = 0; t < l_pk; t++) {
            Rng r(key, (uint32_t)party, mktrng::STREAM_PACK_KEY, (uint32_t)q, (uint32_t)t);
            const uint64_t g = (uint64_t)K->lwekey[q] << (W - (t + 1) * logB_pk);
            rlwe_sample(r, K->zring, pack_zoff(p), kr, K->sigma_ring, N, W, buf.data(), [&](int j) { return j ? 0 : g; });
            for (int c = 0; c < polys; c++) store_poly(pk_out, ((size_t)q * l_pk + t) * polys + c, buf.data() + (size_t)c * N, N, W);
        }
    });
    explicit_bzero(key, sizeof key);
    return MKT_OK;
}

// the seeded form (mktfhe_pack.h "SEEDED"): the bodies of the rows, masks from the public stream 19, noise from the secret stream 20
int mkt_client_packing_keygen_seeded(const mkt_params *params, const mkt_client_party *K, int party, int l_pk, int logB_pk, const uint8_t *seed,
                                     const uint8_t *mask_seed, void *pk_seeded_out) {
    Shape sh;
    if (!K || !pk_seeded_out || !mask_seed || !pack_gadget_ok(l_pk, logB_pk) || open_party(params, party, sh)) return MKT_ERR_ARG;
    if (seed && std::memcmp(seed, mask_seed, 32) == 0) return MKT_ERR_ARG;      // the mask seed is published: the noise would be too
    const mkt_params &p = *params;
    if (!party_keys_match(K, p, party)) return MKT_ERR_ARG;
    if (std::memcmp(mask_seed, K->key, sizeof K->key) == 0) return MKT_ERR_ARG;  // nor may it be the seed of the party's secrets
    const int N = p.N, W = p.W, kr = sh.ksk_kr;
    uint32_t key[8], mkey[8];
    if (seed_to_key(seed, key)) return MKT_ERR_STATE;
    seed_to_key(mask_seed, mkey);
    parallel_for(p.n, [&](int q) {
        std::vector<uint64_t> a(N), b(N);
        const auto pack_mask = [&](uint32_t S, int c) { return pack_mask_poly(mkey, party, S * (uint32_t)kr + (uint32_t)c, l_pk, logB_pk, N, W, a.data()); };
        for (int t = 0; t < l_pk; t++) {
            const uint32_t S = (uint32_t)q * (uint32_t)l_pk + (uint32_t)t;
            rlwe_body_acc(b.data(), K->zring, pack_zoff(p), kr, N, [&](int c) { return pack_mask(S, c); });
            Rng r(key, (uint32_t)party, mktrng::STREAM_PACK_NOISE, (uint32_t)q, (uint32_t)t);
            const uint64_t g = (uint64_t)K->lwekey[q] << (W - (t + 1) * logB_pk);
            add_noise(b.data(), N, W, r, K->sigma_ring, [&](int j) { return j ? 0 : g; });
            store_poly(pk_seeded_out, S, b.data(), N, W);
        }
    });
    explicit_bzero(key, sizeof key);
    return MKT_OK;
}

// the definition of expansion: bodies copied, masks regenerated; needs no key
int mkt_client_packing_key_expand(const mkt_params *params, int party, int l_pk, int logB_pk, const uint8_t *mask_seed, const void *pk_seeded, void *pk_out) {
    Shape sh;
    if (!mask_seed || !pk_seeded || !pk_out || !pack_gadget_ok(l_pk, logB_pk) || open_party(params, party, sh)) return MKT_ERR_ARG;
    const mkt_params &p = *params;
    const int N = p.N, W = p.W, kr = sh.ksk_kr;
    uint32_t mkey[8];
    seed_to_key(mask_seed, mkey);
    parallel_for(p.n, [&](int q) {
        std::vector<uint64_t> a(N);
        for (int t = 0; t < l_pk; t++) {
            const uint32_t S = (uint32_t)q * (uint32_t)l_pk + (uint32_t)t;
            expand_sample(pk_out, S, pk_seeded, kr, N, W, [&](int c) { return pack_mask_poly(mkey, party, S * (uint32_t)kr + (uint32_t)c, l_pk, logB_pk, N, W, a.data()); });
        }
    });
    return MKT_OK;
}

// TEST HARNESS: the top 32 bits of b + sum a z, every product exact
int mkt_client_rlwe_phase(const mkt_params *params, const mkt_client_party *const *keys, int nparties, const void *rlwe, uint32_t *phase_out) {
    Shape sh;
    if (!keys || !rlwe || !phase_out || open_party(params, 0, sh)) return MKT_ERR_ARG;
    const mkt_params &p = *params;
    if (nparties != sh.nparty) return MKT_ERR_ARG;
    for (int i = 0; i < nparties; i++) if (!keys[i] || !party_keys_match(keys[i], p, i)) return MKT_ERR_ARG;
    std::vector<uint64_t> acc(p.N), a(p.N);
    load_poly(rlwe, 0, acc.data(), p.N, p.W);
    for (int i = 0; i < nparties; i++) ring_share_acc(p, sh, keys[i], i, rlwe, acc.data(), a.data());
    for (int j = 0; j < p.N; j++) phase_out[j] = (uint32_t)((acc[j] & wmask(p.W)) >> (p.W - 32));
    return MKT_OK;
}

// share[g] = sum_c a_{slot(party,c)}[g] (*) z_c + e[g], e[g] the N smudging words of pack row0 + g (stream 18), lifted to the ring's width
int mkt_client_rlwe_partial_decrypt(const mkt_params *params, const mkt_client_party *K, int party, const void *rlwe, double sigma_smudge,
                                    const uint8_t *seed, uint64_t row0, void *share_out, size_t G) {
    Shape sh;
    if (!K || !smudge_sigma_ok(sigma_smudge) || open_party(params, party, sh)) return MKT_ERR_ARG;
    const mkt_params &p = *params;
    if (!party_keys_match(K, p, party)) return MKT_ERR_ARG;
    if (!G) return MKT_OK;
    if (!rlwe || !share_out) return MKT_ERR_ARG;
    uint32_t key[8];
    if (seed_to_key(seed, key)) return MKT_ERR_STATE;
    const size_t ctb = (size_t)(1 + sh.kacc) * p.N * sh.word;
    std::vector<uint64_t> acc(p.N), a(p.N);
    for (size_t g = 0; g < G; g++) {
        std::fill(acc.begin(), acc.end(), 0);
        ring_share_acc(p, sh, K, party, (const uint8_t *)rlwe + g * ctb, acc.data(), a.data());
        Rng r(key, (uint32_t)party, mktrng::STREAM_PACK_SMUDGE, (uint32_t)(row0 + g), (uint32_t)((row0 + g) >> 32));
        for (int j = 0; j < p.N; j++) acc[j] = (acc[j] + (r.noise(sigma_smudge) << (p.W - 32))) & wmask(p.W);
        store_poly(share_out, g, acc.data(), p.N, p.W);
    }
    explicit_bzero(key, sizeof key);
    return MKT_OK;
}

// top 32 bits of b[j] + sum_i share_i[j], j < count; shares [nparty][N]
static int rlwe_merge(const mkt_params *params, const void *rlwe, const void *shares, int nparties, size_t count, uint32_t *phase_out, uint8_t *bits_out) {
    Shape sh;
    if (!rlwe || !shares || (!phase_out && !bits_out) || open_party(params, 0, sh)) return MKT_ERR_ARG;
    const mkt_params &p = *params;
    if (nparties != sh.nparty || count > (size_t)p.N) return MKT_ERR_ARG;
    std::vector<uint64_t> acc(p.N), s(p.N);
    load_poly(rlwe, 0, acc.data(), p.N, p.W);
    for (int i = 0; i < nparties; i++) { load_poly(shares, (size_t)i, s.data(), p.N, p.W); for (int j = 0; j < p.N; j++) acc[j] += s[j]; }
    for (size_t j = 0; j < count; j++) {
        const uint32_t ph = (uint32_t)((acc[j] & wmask(p.W)) >> (p.W - 32));
        if (phase_out) phase_out[j] = ph;
        if (bits_out) bits_out[j] = (uint8_t)bit_of_phase(p, ph);
    }
    return MKT_OK;
}
int mkt_client_rlwe_merge_phase(const mkt_params *params, const void *rlwe, const void *shares, int nparties, size_t count, uint32_t *phase_out) {
    return phase_out ? rlwe_merge(params, rlwe, shares, nparties, count, phase_out, nullptr) : (int)MKT_ERR_ARG;
}
int mkt_client_rlwe_merge_decrypt(const mkt_params *params, const void *rlwe, const void *shares, int nparties, size_t count, uint8_t *bits_out) {
    return bits_out ? rlwe_merge(params, rlwe, shares, nparties, count, nullptr, bits_out) : (int)MKT_ERR_ARG;
}

}  // extern "C"
