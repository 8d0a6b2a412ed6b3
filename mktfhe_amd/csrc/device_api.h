// Host-callable launchers of the HIP kernels (kernels.hip).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rot_plan.h"

namespace mktd {

struct cplx;

struct TwPtrs { const cplx *psi, *psiinv, *roots, *rootsinv; };

// Launcher-level A/B switches (grid shapes of the transform and key-switch kernels): process-wide, read from the
// environment on FIRST USE only -- the call path never calls getenv (context.cpp).  0 = the built-in default.
struct LaunchTuning { int fft_grid, fft_nb, fft_igrid, ks_g, ks_blocks, ks_waves, ks_pair, ntt_grid, ks_mfma; };
const LaunchTuning &launch_tuning();
// base name of the blind-rotation kernel the calling thread launched last (set by every rotation launcher; read by
// mkt_last_kernel_name so that bench.py's roofline names the kernel that actually ran)
extern thread_local const char *last_rot_kernel;
// the compile-time gadget of that launch, (length, log2 of the base): 0 where the instantiation takes the value at run time
// (mkt_get_metric "rot_static_l" / "rot_static_logB": which specialisation a test reached; no result depends on them)
extern thread_local int last_rot_static_l, last_rot_static_logB;
// the one way a launcher notes its kernel: a launcher that names no compile-time gadget clears the pair of the launch before
inline void note_rot_kernel(const char *name, int static_l = 0, int static_logB = 0) {
    last_rot_kernel = name; last_rot_static_l = static_l; last_rot_static_logB = static_logB;
}

// Blind rotation with an RLWE accumulator of length 1 (b, a): CGGI/LMSS with k = 1 and every row of
// KMS / KMS_block phase 1.  One workgroup per rotation.
struct RotArgs {
    TwPtrs tw;
    const cplx *brk;          // party 0 base; [n][2l rows][2 polys][M], DEVICE point order
    size_t brk_party_stride;  // in cplx
    const cplx *monomial;     // [2N][M], entry e-1
    const uint32_t *lwe;      // [B][lwe_stride]: LWE words (mod-switched on the fly) or atilde
    int lwe_stride;
    int pre_switched;         // 1: `lwe` already holds atilde values
    int n, logN;
    int l, logB;              // RGSW gadget
    int blk_len;              // 1, or the block length of LMSS / KMS_block
    int blk_accum;            // block schemes: tacc2 += monomial*tacc form (bootstrapping.jl:157,:648)
    int rows_per_gate;        // rotations per ciphertext
    size_t ngates;            // ciphertexts in this launch (grid = ngates * rows_per_gate)
    const int *slot_party;    // [rows_per_gate]
    const int *slot_row;      // [rows_per_gate]
    int init_mode;            // 0: load acc from acc_io; 1: trivial RLEV row b = 2^(W-(row+1)*logB_lev)
    int logB_lev;
    int out_mode;             // 0: write acc to acc_io; 1: write fft(acc) to tout
    void *acc_io;             // [rot][2][N] ring words
    cplx *tout;               // [rot][2][M]
    int tout_natural;         // 1: reference point order (API output); 0: device order (feeds phase 2)
    int variant;              // tuning: 10*LOGR + transforms per group (0 = default)
    int stagger;              // start-up delay of alternate workgroup groups, in units of 512 cycles (0 = off)
    int wide;                 // latency variant: 0 automatic, 1 never, 2 always where supported (MKT_ROT_WIDE)
    unsigned block0;          // first rotation of this launch: the kernels add it to their workgroup index; the caller's value (0) is RotCall::block0, run_rot_plan sets it for every launch
    unsigned split;           // rotations per launch (MKT_ROT_SPLIT): 0 = the family's rule, (unsigned)-1 = one launch; read by rot_call for plan_k1 as an int, by no launcher and no kernel
    int dev_order;            // device point order of the resident tables (fft_device.h dev_pos)
    int map_mode;             // workgroup id -> (ciphertext, slot): 0 slot-major, 1 rows of one (ciphertext, party) eight ids apart (kernel_common.h rot_decode)
    int blk_group;            // rotations per workgroup (MKT_ROT_BLKG) -- 0 automatic, 1 one (blindrotate_k1_kernel<LB>, blindrotate_kr_kernel), 2 / 4 (rot_block.hip); read by rot_call for plan_k1 / plan_kr alone
};

// KMS phase 2 (bootstrapping.jl:448-558), one workgroup per ciphertext.
struct Phase2Args {
    TwPtrs tw;
    const uint32_t *lin;      // [B][lwe_stride] linear-combined LWE (b last) for the test vector, or NULL
    int lwe_stride;
    int logN;
    int k, l_lev, logB_lev, l_uni, logB_uni;
    const cplx *levkey;       // [B][Rtot][2][M]
    int rtot;
    const cplx *rlk_d;        // [k][l_uni][M]
    const cplx *rlk_f;        // [k][l_uni][2][M]
    const cplx *pub_b;        // [k][l_uni][M]
    const cplx *crs;          // [l_uni][M]
    void *acc;                // [B][1+k][N] ring words (in: test vector unless lin != NULL; out: result)
    cplx *scratch;            // [B][2*(k+1)][M]
    int dev_order;            // device point order of the resident tables
};

// CCS blind rotation (bootstrapping.jl:234-328), one workgroup per ciphertext.
struct CcsArgs {
    TwPtrs tw;
    const uint32_t *lwe;      // [B][lwe_stride] LWE words or atilde
    int lwe_stride, pre_switched;
    int n, logN, k, l, logB;
    const cplx *brk;          // [party][n][3l][M]: d[l], then (f[j].b, f[j].a) j-major; device point order
    size_t brk_party_stride;
    const cplx *pub_b;        // [party][l][M]
    const cplx *crs;          // [l][M]
    const cplx *monomial;
    void *acc;                // [B][1+k][N] ring words, in place
    cplx *scratch;            // [B][k+1][M]
    void *vscratch;           // [B][3][N] ring words (the two-group kernel uses all three, the one-group kernel the first)
    int stagger;              // start-up delay between the workgroups that share a compute unit, in units of 64 cycles (0 = off)
    int dev_order;            // device point order of the resident tables
};

struct KsmArgs;
struct KsArgs {
    const void *acc;          // [B][1+kacc][N] ring words
    uint32_t *out;            // [B][lwe_len]
    const uint32_t *ksk;      // party 0 base; [kr][N][drows][f][n1p] rows padded to n1p = 4*ceil((n+1)/4) words
    size_t ksk_party_stride;  // words
    int n1p;
    int N, n, f, logD, drows;
    int kacc;                 // ring components
    int mk;                   // 1: component i -> party i's KSK and mask block i; 0: single block, ksk comp i
    int balanced;             // block schemes: copy the first words, balanced digits
    int lmss;                 // LMSS flavour of the copy rule (global coefficient index across components)
    uint32_t *digits;         // scratch of the digit-pair kernel (both or neither; sizes: ks_report): prepared digit words
    uint32_t *partial;        //   and the partial sums of every slab; null: the per-digit kernel with atomics
    // key switch at a coefficient (mktfhe.h): out[g] = keyswitch!(E_coef[g](acc[src[g]])).  Both null = the plain key switch, which runs
    // kernels of its own; else acc holds nacc rows, src [B] rows of acc (null: g; clamped to nacc - 1), coef [B] (null: 0; read mod N)
    const uint32_t *src;
    const uint32_t *coef;
    size_t nacc;
    // the key as signed byte planes (ks_mfma.h), one block per party or per component, or null: the matrix-core kernel in place of the
    // digit-pair kernel where the launch-shape rule picks it (unbalanced digits, D = 4; the AT rows come through the same digit words)
    const int8_t *planes;
    size_t planes_block_stride;   // bytes
    // ... and the launcher of that kernel (launch_ks_mfma): handed in by the caller that owns the planes, so that this unit names nothing of ks_mfma.hip
    hipError_t (*sum_mfma)(const struct KsmArgs &, hipStream_t);
};
// What the launch rule of the key switch reads of a call, as plain values (planes: the byte planes and their launcher are there; scratch: digits
// and partial are), and what it decides.  kernel: 1 per-digit (keyswitch_mg_kernel), 2 digit-pair, 3 matrix cores; digit_words / partial_words:
// the words of KsArgs::digits / KsArgs::partial for the batch, computed with scratch taken as present (the caller sizes its buffer from them before there is
// one; 0, 0: this shape runs on the per-digit kernel).  No device, no context: mkt_internal_ks_plan hands the rule to tests/test_ks_plan_cpu.py
struct KsShape { int N, f, logD, drows, n1p, kacc, mk, balanced, planes, scratch; };
struct KsReport { int kernel, G, waves, ngroups, parties, gblocks, slabs; size_t digit_words, partial_words; };
inline KsShape ks_shape(const KsArgs &a, bool scratch) {
    return KsShape{a.N, a.f, a.logD, a.drows, a.n1p, a.kacc, a.mk, a.balanced, a.planes && a.sum_mfma ? 1 : 0, scratch ? 1 : 0};
}
KsReport ks_report(const KsShape &a, size_t B, const LaunchTuning &lt);
// ks_mfma.hip: the byte planes of one block from its resident rows [N][drows][f][n1p]; digit words x planes -> partial sums per slab
struct KsmArgs;
hipError_t launch_ks_mfma_pack(const uint32_t *rows, int8_t *planes, int N, int f, int drows, int n1p, hipStream_t s);
hipError_t launch_ks_mfma(const KsmArgs &a, hipStream_t s);

// Evaluation-key generation on the device (keygen.hip): one party's secrets and the stream key of client.cpp
struct KeygenArgs {
    uint32_t key[8];             // the party's 256-bit ChaCha20 stream key (rng_chacha.h)
    int party;                   // party index (carried in the stream nonce)
    int N, n, W;
    int kr, l, logB;             // RGSW: RLWE length, gadget ; UniEnc: l_uni, logB_uni
    int zoff;                    // first ring-key polynomial used
    int f, logD;                 // key-switching gadget
    double sigma_ring, sigma_lwe;
    const uint32_t *lwekey;      // [n]
    const int8_t *zring;         // [nz][N], entries 0/1
    const void *crs;             // [l][N] ring words (UniEnc only)
    void *out;                   // bootstrapping key, coefficient form, native word width
};
hipError_t launch_keygen_brk(const KeygenArgs &a, int unienc, hipStream_t s);
hipError_t launch_keygen_ksk(const KeygenArgs &a, uint32_t *ksk, int n1p, int kk, int dr, int is_block, hipStream_t s);

// The seeded key form generated on the device (keygen_seeded.hip; mktfhe.h "seeded evaluation keys"): the BODIES of one party's two large
// keys, the words of mkt_client_party_keygen_seeded.  Masks come from the public streams 12 and 13 and are never stored
struct KeygenSeededArgs {
    uint32_t key[8];             // the party's 256-bit ChaCha20 stream key: the secret streams 14, 15, 16
    uint32_t mkey[8];            // key of the mask streams 12, 13: the PUBLIC mask seed
    int party;
    int N, n, W;
    int kr, l, logB;             // RGSW: RLWE length, gadget ; UniEnc: l_uni, logB_uni
    int zoff;                    // ring-key polynomial the key switch starts from (the uni key of the KMS schemes: 1)
    int f, logD, drows;          // key-switching gadget
    int absent_below;            // key-switching rows (c, j) with c N + j below it are absent (block schemes: n, else 0)
    int width;                   // key-switching kernel: lanes that share a row's keystream blocks (set by the launcher, as SeededArgs::width)
    double sigma_ring, sigma_lwe;
    const uint32_t *lwekey;      // [n]
    const int8_t *zring;         // [nz][N]
    const void *crs;             // [l][N] ring words (UniEnc only)
    void *brk_body;              // compact bootstrapping-key section, native word width
    uint32_t *ksk_body;          // [ksk_rows]
    uint64_t ksk_rows;
};
hipError_t launch_keygen_seeded_brk(const KeygenSeededArgs &a, int unienc, hipStream_t s);
hipError_t launch_keygen_seeded_ksk(KeygenSeededArgs a, hipStream_t s);

// A party's decryption shares on the device (partial_decrypt.hip; mktfhe.h "distributed decryption"):
// out[j] = <lwe[j] block `party`, lwekey> + smudge_word(key, party, row0 + j, sigma), j < B
struct PartialDecryptArgs {
    uint32_t key[8];             // 256-bit ChaCha20 key of the call's noise streams (rng_chacha.h)
    int party, n, lwe_stride;    // party block, words per block, words per row
    double sigma;
    uint64_t row0;
    const uint32_t *lwe;         // [B][lwe_stride]
    const uint32_t *lwekey;      // [n]
    uint32_t *out;               // [B]
    size_t B;
};
hipError_t launch_partial_decrypt(const PartialDecryptArgs &a, hipStream_t s);

// Seeded ciphertexts on the device (seeded.hip; mktfhe.h "seeded ciphertexts"), the words of mkt_client_seeded_expand / _encrypt:
// expand:  out[j] = zeros, mask_block words of row row0 + j in block `party`, in[j] last     (in = body [B], out [B][lwe_len], dense)
// encrypt: out[j] = row_noise_word(nkey, party, 11, row0 + j, sigma) - <mask of row row0 + j, lwekey> + in[j]     (in = mu [B], out = body [B])
struct SeededArgs {
    uint32_t mkey[8];            // ChaCha20 key of the mask streams: the PUBLIC mask seed
    uint32_t nkey[8];            // encrypt: key of the noise streams (secret)
    int party, n, lwe_len;
    int tile_words;              // expand: words of the output span per tile (set by the launcher)
    int width;                   // encrypt: lanes that share a row's keystream blocks, a power of two in 4 .. 64 (set by the launcher)
    double sigma;                // encrypt
    uint64_t row0;
    const uint32_t *lwekey;      // encrypt: [n]
    const uint32_t *in;          // [B]
    uint32_t *out;
    size_t B;
};
hipError_t launch_seeded_expand(SeededArgs a, hipStream_t s);
hipError_t launch_seeded_encrypt(SeededArgs a, hipStream_t s);
// the words per tile the expand launcher picks for a shape (what the tests size their grid-stride case by; the workgroup cap of a launch
// and the encrypt kernel's rows per tile: party_rows.h)
int seeded_expand_tile_words(int n, int lwe_len);

// Seeded evaluation keys on the device (seeded_keys.hip; mktfhe.h "seeded evaluation keys"), the words of mkt_client_seeded_keys_expand.
// Key-switching key: out = [rows][n1p] words, the RESIDENT pitch (n1p = 4 ceil((n + 1) / 4), out 16-byte aligned): row R = the n mask words of
// stream 12 at index R, body[R], zeros; all zeros where R / rows_per_cj < absent_below (block schemes: absent_below = n, else 0)
struct SeededKskArgs {
    uint32_t mkey[8];            // ChaCha20 key of the mask streams: the PUBLIC mask seed
    int party, n, n1p;
    uint32_t rows_per_cj;        // Drows * f
    int absent_below;
    const uint32_t *body;        // [rows]
    uint32_t *out;
    uint64_t rows;
};
// Bootstrapping key: out = npolys polynomials in the coefficient layout of mkt_load_brk, each 1 << log_units units of 64 bytes (N W / 512);
// bodies copied from `body` (the compact section), masks from stream 13.  unienc 0: groups of kr + 1 (b, a_0 ..); 1: groups of 3 l (CCS)
// stream / idx_hi: the mask stream (13; 19 for a packing key, pack_keys.hip) and the high word of its stream index (0; the packing gadget).
// t_rows != 0 (unienc 0 only): out is [kr + 1][t_rows] polynomials, polynomial q of group r at q t_rows + r, t_rows = npolys / (kr + 1)
struct SeededBrkArgs {
    uint32_t mkey[8];
    uint32_t stream, idx_hi;
    uint64_t t_rows;
    int party, unienc, kr, l, log_units;
    const void *body;            // 16-byte aligned
    void *out;                   // 16-byte aligned
    uint64_t npolys;
};
hipError_t launch_seeded_ksk_expand(const SeededKskArgs &a, hipStream_t s);
hipError_t launch_seeded_brk_expand(const SeededBrkArgs &a, hipStream_t s);

// The seeded packing key (pack_keys.hip; mktfhe_pack.h "SEEDED").  Expansion: the words of mkt_client_packing_key_expand through the tile frame of
// seeded_brk_expand_kernel -- body [rows][N] -> out [rows][1 + kr][N], or [1 + kr][rows][N] with `transposed` (the EXACT resident layout), rows = n l_pk
struct PackKeyExpandArgs {
    uint32_t mkey[8];            // the PUBLIC mask seed
    int party, kr, l, logB, log_units, transposed;
    const void *body;            // 16-byte aligned
    void *out;                   // 16-byte aligned
    uint64_t rows;
};
hipError_t launch_pack_key_expand(const PackKeyExpandArgs &a, hipStream_t s);
// Generation: the words of mkt_client_packing_keygen_seeded, one workgroup per row (q, t); only the bodies are stored
struct PackKeygenArgs {
    uint32_t key[8];             // ChaCha20 key of the SECRET noise stream 20 (the generation seed)
    uint32_t mkey[8];            // key of the mask stream 19: the PUBLIC mask seed
    int party, N, n, W, kr, l, logB;
    double sigma_ring;
    const uint32_t *lwekey;      // [n]
    const int8_t *zring;         // [kr][N]: the ring keys the key-switching key switches from
    void *body;                  // [n][l][N] ring words
};
hipError_t launch_pack_keygen(const PackKeygenArgs &a, hipStream_t s);

// A party's ring shares of packed ciphertexts on the device (ring_share.hip; mktfhe_ring_share.h), the words of mkt_client_rlwe_partial_decrypt:
// out[g] = sum_{c < kr} rlwe[g][poly0 + c * poly_step] (*) zring[c] + (draw j of stream 18 at pack row0 + g, lifted by W - 32 bits)_j, g < G
struct RingShareArgs {
    uint32_t key[8];             // 256-bit ChaCha20 key of the call's noise streams (rng_chacha.h)
    int party, N, W, kr;
    int npoly;                   // polynomials of one ciphertext, 1 + k
    int poly0, poly_step;        // ciphertext polynomial of component c: the multi-key schemes (1 + party, 0), else (1, 1)
    int slices;                  // workgroups that share one pack (set by the launcher: ring_share_slices)
    double sigma;
    uint64_t row0;
    const void *rlwe;            // [G][npoly][N] ring words
    const int8_t *zring;         // [kr][N]: the ring keys the packed ciphertext is under
    void *out;                   // [G][N] ring words
    size_t G;
};
int ring_share_slices(int N, size_t G);   // a power of two in N / 256 (one below N = 256) .. N / 16: more of them the fewer packs there are
hipError_t launch_ring_share(RingShareArgs a, hipStream_t s);

// Packed outputs (pack.hip; mktfhe_pack.h): one launch sequence packs `npacks` ciphertexts, pack0 .. pack0 + npacks - 1 of the call
constexpr int PACK_QCHUNK = 4;   // mask words per workgroup of the product kernel: k n / 4 workgroups per pack (280 at the headline shape)
struct PackArgs {
    TwPtrs tw;
    const uint32_t *pool;     // [pool_rows][lwe_len]
    size_t pool_rows;
    const uint32_t *idx;      // [B] rows of the pool (clamped), or null: row r of the call = row r of the pool
    size_t B, pack0;          // picked rows of the whole call; first pack of this launch sequence
    int logN, n, nparty, lwe_len, kacc;
    int mk;                   // 1: party i's polynomial 1 -> slot i; 0: party 0's polynomial 1 + c -> slot c
    int np;                   // polynomials of a key row, 1 + kr
    int l, logB;              // packing gadget
    int nchunk;               // ceil(n / PACK_QCHUNK)
    const cplx *key;          // party 0 base; [n][l][np][M], slot-major point order (dev_pos order 1)
    size_t key_party_stride;  // in cplx
    void *cols;               // [npacks][lwe_len][N] ring words: the lifted columns
    void *slabs;              // [npacks][nparty][nchunk][np][N] ring words
    void *out;                // [npacks][1 + kacc][N] ring words
};
bool pack_supported(int np);
hipError_t launch_pack_columns(int W, const PackArgs &a, size_t npacks, hipStream_t s);
hipError_t launch_pack_product(int logM, int W, const PackArgs &a, size_t npacks, hipStream_t s);
hipError_t launch_pack_reduce(int W, const PackArgs &a, size_t npacks, hipStream_t s);
hipError_t launch_pack_accumulate(int W, void *dst, const void *prod, size_t rows, int N, hipStream_t s);

hipError_t launch_transform_fwd(int logM, int W, TwPtrs tw, const void *p, cplx *t, size_t B, int dev_order, hipStream_t s);
hipError_t launch_reorder(int logM, const cplx *in, cplx *out, size_t npolys, int to_device, int order, hipStream_t s);
hipError_t launch_transform_inv(int logM, int W, TwPtrs tw, const cplx *t, void *p, size_t B, hipStream_t s);
hipError_t launch_decompose(int W, const void *p, void *digits, int N, int l, int logB, size_t B, hipStream_t s);
// ops / ix / iy may be NULL: one op for the batch / operands in batch order (kernels.hip gate_linear_kernel)
hipError_t launch_gate_linear(int op, const uint8_t *ops, const uint32_t *x, const uint32_t *y, const uint32_t *ix, const uint32_t *iy, size_t pool_rows, uint32_t *out, int len, size_t B, hipStream_t s);   // pool_rows > 0: ix / iy are clamped into the pool (no out-of-bounds read whatever a device-side index array holds)
// the three-input linear part (mktfhe.h MKT_MAJ3 .. MKT_AE3, flags MKT_OP_NOT_X / _Y / _Z): ops [B] per gate; ix / iy / iz NULL = operands in
// batch order, else rows of a pool clamped into [0, pool_rows) as launch_gate_linear does; out [B][len]
hipError_t launch_gate3_linear(const uint8_t *ops, const uint32_t *x, const uint32_t *y, const uint32_t *z, const uint32_t *ix, const uint32_t *iy, const uint32_t *iz,
                               size_t pool_rows, uint32_t *out, int len, size_t B, hipStream_t s);
hipError_t launch_negate(uint32_t *x, size_t words, hipStream_t s);
hipError_t launch_mux_linear(const uint32_t *pool, size_t pool_rows, const uint32_t *is, const uint32_t *ia, const uint32_t *ib, const uint8_t *not_ab, uint32_t *out, int len, size_t B, hipStream_t s);   // [2B][len]: AND(s, a'), then AND(NOT s, b')
hipError_t launch_mux_combine(int W, void *acc, size_t B, size_t words, hipStream_t s);   // acc[j] += acc[B + j], + 2^(W-3) at X^0 of b: [2B][words] -> [B][words]
hipError_t launch_modswitch(const uint32_t *lwe, uint32_t *atilde, uint32_t *btilde, int len, int logN, size_t B, hipStream_t s);
hipError_t launch_testvector(int W, const uint32_t *lin, int lwe_stride, int logN, int kacc, void *acc, size_t B, hipStream_t s);
// programmable bootstrap (lut.hip; mktfhe.h "programmable bootstrap"): acc[g] = (X^btilde(lin[g]) * luts[sel[g]], 0 ...), luts [nluts][N] ring
// words, sel [B] or NULL (row 0), rows clamped to nluts - 1; acc [B][1+kacc][N]
hipError_t launch_lut_testvector(int W, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lin, int lwe_stride, int logN, int kacc, void *acc, size_t B, hipStream_t s);
// the many-table form (mktfhe.h "many-table bootstrap"), nu = log2(nout) in 0 .. 3: body and mask words go onto the grid 2^nu times coarser,
// sw(w) = divbits(w, 32 - logN - 1 + nu) << nu.  acc as above from the coarse btilde; atilde (NULL: not wanted) receives the lwe_stride - 1
// switched mask words of each ciphertext, rows of at_stride words -- it may be lin itself (every word is read and written by the same lane,
// the b word is left alone).  nu = 0 with atilde NULL is launch_lut_testvector
hipError_t launch_lut_many_testvector(int W, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lin, int lwe_stride, int logN, int kacc, int nu,
                                      uint32_t *atilde, int at_stride, void *acc, size_t B, hipStream_t s);
// accs[g][v] = X^-v * acc[g] for v < nout (1, 2, 4, 8; nout <= N): acc [B][1+kacc][N] -> accs [B][nout][1+kacc][N]; the two must not overlap
hipError_t launch_lut_extract(int W, const void *acc, int nout, int logN, int kacc, void *accs, size_t B, hipStream_t s);
// the (src, coef) rows of a bootstrap with ncoef outputs per input (KsArgs): src[g] = g / ncoef, coef_rows[g] = coef[g % ncoef] (coef NULL: g % ncoef) for g < rows
hipError_t launch_ks_at_table(const uint32_t *coef, size_t ncoef, uint32_t *src, uint32_t *coef_rows, size_t rows, hipStream_t s);
// its gather front end: out[g] = cst[g] e_b + sum_{t<4} wt[g][t] pool[idx[g][t]] (int8 weights, 0 skips the term; rows clamped into the pool); out [B][len]
hipError_t launch_lut_linear(const uint32_t *pool, size_t pool_rows, const uint32_t *idx, const int8_t *wt, const uint32_t *cst, uint32_t *out, int len, size_t B, hipStream_t s);
bool blockg_supported(int logM, int G);
bool ccs_pipe_supported(int logM);   // the two-group CCS kernel at this size (workgroup of 2 * M / 16 threads, LDS budget; ccs_pipe.hip)
// the rotation call of a RotArgs launch (rot_plan.h): the switches travel in the argument struct, the kernels that exist come from their predicates
inline RotCall rot_call(int logM, int W, int kr, const RotArgs &a, size_t nrot) {
    RotCall c{};
    c.logM = logM; c.W = W; c.l = a.l; c.blk_len = a.blk_len; c.kr = kr;
    c.rows = (size_t)a.rows_per_gate; c.ncts = a.ngates; c.nrot = nrot;
    c.wide = a.wide; c.split = (int)a.split; c.blk_group = a.blk_group; c.variant = a.variant; c.block0 = a.block0;
    c.can_wide = wide_supported(logM, a.l, a.blk_len); c.can_g2 = blockg_supported(logM, 2); c.can_g4 = blockg_supported(logM, 4);
    return c;
}
hipError_t launch_blindrotate_k1(int logM, int W, const RotArgs &a, size_t nrot, hipStream_t s);
hipError_t launch_rot_blockg_u32(int logM, int G, int npolys, const RotArgs &a, size_t nslots, hipStream_t s);   // npolys = RLWE length + 1 (2; 3 at block length 1 or 3 and 4 at block length 1, 32-bit ring, G = 4)
hipError_t launch_rot_blockg_u64(int logM, int G, int npolys, const RotArgs &a, size_t nslots, hipStream_t s);
hipError_t launch_blindrotate_kr(int logM, int W, int kr, const RotArgs &a, size_t nrot, hipStream_t s);
// any RLWE length (run-time k; accumulators in memory): scratch = 2 * (kr + 1) * M points per rotation
hipError_t launch_blindrotate_kany(int logM, int W, int kr, const RotArgs &a, cplx *scratch, size_t nrot, hipStream_t s);
hipError_t launch_kms_phase2(int logM, int W, const Phase2Args &a, size_t B, hipStream_t s);
hipError_t launch_ccs_blindrotate(int logM, int W, const CcsArgs &a, size_t B, hipStream_t s);
hipError_t launch_ccs_pipe(int logM, int W, const CcsArgs &a, size_t B, hipStream_t s);   // one ciphertext on two thread groups (ccs_pipe.hip); vscratch [B][3][N]
hipError_t launch_ccs(int logM, int W, const CcsArgs &a, int pipe, size_t B, hipStream_t s);   // one of the two by plan_ccs; pipe: the option ccs_pipe
hipError_t launch_keyswitch(int W, const KsArgs &a, size_t B, hipStream_t s);
bool transform_supported(int logM);

// MKT_ARITH_EXACT (ntt_exact.hip): tab = psi_rev[N] | psiinv_rev[N] | N^-1 | N^-1 2^32, each entry (w mod p1, companion, w mod p2, companion)
hipError_t launch_ntt_fwd(int logN, int W, const uint64_t *tab, const void *p, uint64_t *t, size_t B, int montgomery, hipStream_t s);   // montgomery: output for a resident table (keys, monomials)
hipError_t launch_ntt_inv(int logN, int W, const uint64_t *tab, const uint64_t *t, void *p, size_t B, hipStream_t s);
// CGGI blind rotation (RLWE length 1, 32-bit ring) with exact products; brk [n][2l][2][N], mono [2N][N] residues, natural order
hipError_t launch_exact_blindrotate(int logN, const uint64_t *tab, const uint64_t *brk, const uint64_t *mono, const uint32_t *lwe, int lwe_stride,
                                    int pre_switched, int n, int l, int logB, int blk_len, uint32_t *acc, size_t B, hipStream_t s);
// the same for any RLWE length kr = 1 .. 3 and any block length (digit transforms recomputed per key bit of a block); brk [n][(kr+1) l][kr+1][N]
hipError_t launch_exact_blindrotate_kr(int logN, const uint64_t *tab, const uint64_t *brk, const uint64_t *mono, const uint32_t *lwe, int lwe_stride,
                                       int pre_switched, int n, int kr, int l, int logB, int blk_len, uint32_t *acc, size_t B, hipStream_t s);
// any RLWE length (run-time kr): the transform-domain sums in scratch [B][2][kr+1][N] packed residue pairs
hipError_t launch_exact_blindrotate_kany(int logN, const uint64_t *tab, const uint64_t *brk, const uint64_t *mono, const uint32_t *lwe, int lwe_stride,
                                         int pre_switched, int n, int kr, int l, int logB, int blk_len, uint32_t *acc, uint64_t *scratch, size_t B, hipStream_t s);
// the 64-bit ring with exact products (KMS): resident 64-bit tables as (low, high) residue polynomials per logical polynomial
hipError_t launch_ntt_fwd_split(int logN, const uint64_t *tab, const void *p, uint64_t *out, size_t B, hipStream_t s);
struct ExactKmsArgs {
    const uint64_t *brk; size_t brk_party_stride;   // split tables, u64 units; [n][2l][2 polys][2 halves][N] per party
    const uint64_t *mono;                           // [2N][N] (not split)
    const uint32_t *lwe; int lwe_stride, pre_switched;
    int n, k, l_gsw, logB_gsw, l_lev, logB_lev, l_uni, logB_uni, rtot, lwe_len;
    int blk_len;                                    // KMS_block: key bits per block (1 for KMS)
    const int *slot_party, *slot_row;
    uint64_t *levkey;                               // [B][rtot][2][2][N]
    const uint64_t *rlk_d, *rlk_f, *pub_b, *crs;    // split tables
    const uint32_t *lin_for_tv;                     // bootstrapping.jl:11-23 from the linear combination, or NULL (acc holds the test vector)
    uint64_t *acc, *scratch;                        // [B][1+k][N] ; [B][4(k+1)][N]
    int phase1_only;
    int phase2_only;                                // phase 1 was run elsewhere (fx_exact.hip) and levkey is filled
    int wide;                                       // phase 1, l_gsw = 2: the digit products of an accumulator gathered in 64 bits, one reduction (speed only)
};
hipError_t launch_exact_kms(int logN, const uint64_t *tab, const ExactKmsArgs &a, size_t B, hipStream_t s);
// CCS blind rotation with exact products (32-bit ring); tables as residue pairs, natural order, Montgomery form
struct ExactCcsHostArgs {
    const uint32_t *lwe; int lwe_stride, pre_switched;
    int n, k, l, logB;
    const uint64_t *brk; size_t brk_party_stride;   // 8-byte residue pairs
    const uint64_t *pub_b, *crs, *mono;
    uint32_t *acc; uint64_t *scratch;
};
hipError_t launch_exact_ccs(int logN, const uint64_t *tab, const ExactCcsHostArgs &a, size_t B, hipStream_t s);
hipError_t launch_exact_polymul(int logN, int W, const uint64_t *tab, const void *a, const void *b, void *out, size_t B, hipStream_t s);
// largest |a_i| over n signed W-bit ring words (atomicMax into *amax, which the caller zeroes): the operand measure of mkt_exact_polymul_batch
hipError_t launch_exact_amax(int W, const void *a, size_t n, unsigned long long *amax, hipStream_t s);

// MKT_ARITH_EXACT on the Float64 pipe (fx_exact.hip): exact products from FMA complex transforms over 16-bit key limbs.
// Tables (host_internal.h Twiddles::fx_*): om = cyclic forward twiddles by block, twist = rho^j, nat = inverse twiddles by position.
struct FxRotArgs {
    const cplx *om, *twist, *nat;
    const cplx *brk;          // party 0 base; [n][2l][2 polys][W/16 limbs][M], device point order, scaled by 1 / M
    size_t brk_party_stride;  // in cplx
    const uint32_t *lwe; int lwe_stride, pre_switched;
    int n, logN, l, logB;
    int rows_per_gate; size_t ngates;
    const int *slot_party, *slot_row;
    int init_mode;            // 0: load acc from acc_io; 1: trivial RLEV row (bootstrapping.jl:403-406)
    int logB_lev;
    void *acc_io;             // [rot][2][N] ring words, in place
    int stagger; unsigned block0; int map_mode;
    int split;                // rotations per launch: 0 = the family's rule, -1 = everything in one launch; read by launch_fx_blindrotate for plan_fx alone (block0: as RotArgs)
};
hipError_t launch_fx_key_fwd(int logM, int W, const cplx *om, const cplx *twist, const void *p, cplx *out, size_t npolys, unsigned long long *kmax, hipStream_t s);   // out [npolys][W/16][M] or NULL (measure only); kmax: largest |transform value|^2 (bit pattern, atomicMax) or NULL
hipError_t launch_fx_polymul(int logM, int W, const cplx *om, const cplx *twist, const cplx *nat, const void *a, const void *b, void *out, size_t B, unsigned long long *resid, hipStream_t s);
hipError_t launch_fx_blindrotate(int logM, int W, const FxRotArgs &a, size_t nrot, hipStream_t s);

}  // namespace mktd
