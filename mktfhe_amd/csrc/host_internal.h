// Internal host-side declarations shared by the C-ABI translation units.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mktfhe.h"
#include "../../include/mktfhe_pack.h"

namespace mkt {

struct Twiddles {  // fft.jl:18-45, M interleaved complex each
    std::vector<double> psi, psiinv, roots, rootsinv;
    // tables of the engine's OWN transform for MKT_ARITH_EXACT on the Float64 pipe (fx_exact.hip; not the reference's network), M complex each,
    // every entry a correctly rounded double of the 576-bit value:
    //   fx_om[m + i]  = exp(-i pi rev_s(i) / m), m = 2^s, i < m   cyclic Cooley-Tukey twiddles by block, bit-reversed inside a stage ([0] unused)
    //   fx_tw[j]      = exp(-i pi j / N)                          the twist rho^j, rho^M = -i (the inverse multiplies by its conjugate)
    //   fx_nat[h + j] = exp(+i pi j / h), h = 2^b, j < h          decimation-in-time inverse twiddles by position ([0] unused)
    std::vector<double> fx_om, fx_tw, fx_nat;
};
void make_twiddles(int N, Twiddles &tw);

inline bool is_mk(int s) { return s == MKT_CCS || s == MKT_KMS || s == MKT_KMS_BLOCK; }
inline bool is_kms(int s) { return s == MKT_KMS || s == MKT_KMS_BLOCK; }
inline bool is_block(int s) { return s == MKT_LMSS || s == MKT_KMS_BLOCK; }

// derived shape facts used on both sides of the ABI
struct Shape {
    int nparty;     // 1 (SK) or k (MK)
    int kr;         // RLWE length of the RGSW rotation: k (SK), 1 (KMS)
    int kacc;       // mask polys of the accumulator
    int brk_polys;  // polynomials per BRK entry
    int ksk_drows;  // D-1 or D/2
    int ksk_kr;     // ring components covered by one party's KSK
    int lwe_len;    // k*n+1 (MK) or n+1
    size_t word;    // ring word bytes
};
inline Shape shape_of(const mkt_params &p) {
    Shape s;
    s.nparty = is_mk(p.scheme) ? p.k : 1;
    s.kr = is_kms(p.scheme) ? 1 : p.k;
    s.kacc = p.k;
    s.brk_polys = p.scheme == MKT_CCS ? 3 * p.l_uni : (s.kr + 1) * p.l_gsw * (s.kr + 1);
    int D = 1 << p.logD;
    s.ksk_drows = is_block(p.scheme) ? D / 2 : D - 1;
    s.ksk_kr = is_mk(p.scheme) ? 1 : p.k;
    s.lwe_len = s.nparty * p.n + 1;
    s.word = p.W == 64 ? 8 : 4;
    return s;
}
int validate_params(const mkt_params &p, std::string &why);
// 256-bit seed -> key words; NULL = fresh OS entropy (getrandom), never a fixed default (client.cpp)
int seed_to_key(const uint8_t *seed, uint32_t key[8]);
// the smudging deviation a decryption share admits (mktfhe.h "distributed decryption"): finite, 0 <= sigma <= 2^31 (NaN fails both comparisons)
inline bool smudge_sigma_ok(double sigma) { return sigma >= 0.0 && sigma <= 2147483648.0; }

// what a lookup-table bootstrap admits (mktfhe.h "many-table bootstrap", "key switch at a coefficient"), asked by a context before it stages
// anything and by the multi-device evaluator before any shard starts
inline bool lut_nout_ok(int nout, int N) { return (nout == 1 || nout == 2 || nout == 4 || nout == 8) && nout <= N; }   // tables per rotation
inline bool lut_nu_ok(int nu, int N) { return nu >= 0 && nu <= 3 && (1 << nu) <= N; }                                   // mod-switch exponent
inline bool lut_ncoef_ok(size_t ncoef, int N) { return ncoef >= 1 && ncoef <= (size_t)N; }                             // coefficients per rotation
// host arrays only: every word below `bound` -- a coefficient list against N, table selectors against the table count
inline bool host_below(const uint32_t *v, size_t n, size_t bound) {
    for (size_t j = 0; j < n; j++) if (v[j] >= bound) return false;
    return true;
}
// seeded evaluation keys (mktfhe.h): polynomials of one party's compact bootstrapping-key section, rows (= body words) of its key-switching key
inline size_t brk_seeded_polys(const mkt_params &p, const Shape &s) { return (size_t)p.n * (p.scheme == MKT_CCS ? 2 * (size_t)p.l_uni : (size_t)(s.kr + 1) * p.l_gsw); }
inline size_t ksk_rows(const mkt_params &p, const Shape &s) { return (size_t)s.ksk_kr * p.N * s.ksk_drows * p.f; }
// a party's bootstrapping key: polynomials in coefficient form (mkt_load_brk, MKT_FMT_INT_COEFF)
inline size_t brk_polys_total(const mkt_params &p, const Shape &s) { return (size_t)p.n * s.brk_polys; }
// The key-switching key of one party in its two layouts: ksk_rows rows of n1 = n + 1 words as a caller holds them (mkt_load_ksk, mkt_get_ksk),
// the same rows at the pitch n1p -- padded to 16 bytes, the padding zero -- in the resident table
struct KskLayout {
    size_t rows = 0; int n1 = 0, n1p = 0;
    size_t resident_words() const { return rows * (size_t)n1p; }
};
inline KskLayout ksk_layout(const mkt_params &p, const Shape &s) { return KskLayout{ksk_rows(p, s), p.n + 1, (p.n + 1 + 3) / 4 * 4}; }
// The second resident form of the same key (ks_mfma.h: signed byte planes for the int8 matrix cores) is admitted where no 32-bit accumulator
// can overflow: one product of at most 255 in magnitude per (component summed into the output word, coefficient, digit)
inline bool ks_mfma_fits(long long N, long long kr, long long f) { return N > 0 && kr > 0 && f > 0 && N * kr * f * 255 < (1ll << 31); }

// Which key pieces of which party are resident (KeySet::loaded): the one record that key loads write and check_ready, mkt_set_twiddles and
// the key replication read.  The CRS belongs to no party (party < 0): it is marked for all of them.
enum KeyPiece { K_BRK, K_KSK, K_RLK, K_PUB, K_CRS };
struct LoadedKeys {
    std::vector<uint8_t> of;   // [party]: bit k = piece k of the party is resident
    static constexpr unsigned bit(KeyPiece k) { return 1u << k; }
    void reset(int nparty) { of.assign((size_t)nparty, 0); }
    void mark(KeyPiece k, int party) { for (size_t i = 0; i < of.size(); i++) if (party < 0 || (size_t)party == i) of[i] |= (uint8_t)bit(k); }
    bool has_all(unsigned pieces, int party) const { return (of[(size_t)party] & pieces) == pieces; }
    bool has(KeyPiece k, int party) const { return has_all(bit(k), party < 0 ? 0 : party); }
    // pieces that are resident as transforms under the tables they met (the key-switching key is integer data): mkt_set_twiddles
    bool any_transformed() const {
        for (uint8_t m : of) if (m & (bit(K_BRK) | bit(K_RLK) | bit(K_PUB) | bit(K_CRS))) return true;
        return false;
    }
};
// packed outputs (mktfhe_pack.h): the gadget a packing key admits; the polynomials of one party's key [n][l_pk][1 + kr][N], kr = ksk_kr
inline bool pack_gadget_ok(int l, int logB) { return logB >= 1 && logB <= 16 && l >= 1 && l * logB <= 32; }
inline size_t pack_key_polys(const mkt_params &p, const Shape &s, int l) { return (size_t)p.n * l * (s.ksk_kr + 1); }
inline bool ranges_overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return abytes && bbytes && a0 < b0 + bbytes && b0 < a0 + abytes;
}

}  // namespace mkt

// context.cpp internals used by multi.cpp (the multi-device evaluator)
#define MKT_HIDDEN __attribute__((visibility("hidden")))
extern "C" {
MKT_HIDDEN int mkt_internal_clone_keys(mkt_ctx *src, mkt_ctx *dst, int no_peer);   // replicate src's resident key set onto dst's device (peer copy; no_peer: through a host buffer, as when the peer copy is refused)
MKT_HIDDEN int mkt_internal_copy_across(void *dst, int ddev, const void *src, int sdev, size_t bytes, int no_peer);   // device -> device, peer copy or host bounce; a hipError_t value; does not synchronise
MKT_HIDDEN int mkt_internal_device_of(const mkt_ctx *c);
MKT_HIDDEN size_t mkt_internal_lwe_len(const mkt_ctx *c);
MKT_HIDDEN size_t mkt_internal_acc_bytes(const mkt_ctx *c);            // bytes of one RLWE accumulator [1 + k][N]
}

// one party's keys as generated by client.cpp (opaque to callers of the ABI)
struct mkt_client_party {
    mkt_params p;
    mkt::Shape sh;
    int party;
    uint32_t key[8];                        // 256-bit ChaCha20 key of this party's streams (rng_chacha.h)
    double sigma_lwe, sigma_ring;
    bool heavy;                             // false: brk / ksk left empty (generated on the device)
    std::vector<uint32_t> lwekey;           // [n]
    std::vector<std::vector<int8_t>> zring; // SK: k polys; CCS: 1; KMS: [0] = gsw key z', [1] = uni key z
    std::vector<uint8_t> brk, rlk_d, rlk_f, pub;  // ring words at native width
    std::vector<uint32_t> ksk;
    // the seeded key form (mkt_client_party_keygen_seeded): the public mask seed and the bodies; brk / ksk above stay empty
    bool seeded = false;
    uint8_t mask_seed[32] = {};
    std::vector<uint8_t> brk_seeded;        // ring words at native width
    std::vector<uint32_t> ksk_seeded;
};

namespace mkt {
// these keys were made for these parameters and this party index: asked by every call that takes a party's keys beside a parameter set
inline bool party_keys_match(const mkt_client_party *K, const mkt_params &p, int party) {
    return std::memcmp(&K->p, &p, sizeof(mkt_params)) == 0 && K->party == party;
}
}  // namespace mkt
