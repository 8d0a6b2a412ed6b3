/*
 * mktfhe.h -- C ABI of the MI355X-native multi-key TFHE gate-bootstrapping engine.
 *
 * Drop-in boundary for the hot path of SNUCP/MKTFHE (reference: Julia, /root/reference/src).
 * The reference has no FFI; its boundary is the Julia dispatch surface
 *     bootstrapping!(ctxt::LWE, scheme)          src/tfhe/bootstrapping.jl:4
 *     NAND/AND/OR/XOR/XNOR/NOR(c1, c2, scheme)   src/tfhe/gate.jl:1-53,  NOT!(c) gate.jl:55
 *     blindrotate!(atilde, acc, scheme)          bootstrapping.jl:32,:114,:234,:369
 *     keyswitch!(res, acc, scheme)               bootstrapping.jl:81,:170,:333,:564,:664
 * A Julia `ccall` shim flattens its pointer-graph objects into the flat
 * layouts documented here and calls these entry points.  Plain pointers and sizes only.
 *
 * Every function returns MKT_OK (0) or a negative mkt_status; none throws.
 * The engine REQUIRES a gfx950 GPU: there is no CPU fallback on any compute entry point.
 *
 * Layouts (0-based, row-major, innermost last)
 *   LWE ciphertext      : uint32 [k*n + 1] = [a_0 .. a_{k*n-1}, b]   (lwe.jl:1-9; MK mask is the
 *                         concatenation of k per-party blocks of n words, scheme.jl:379-386)
 *   ring polynomial     : N ring words; ring word = uint32 if W == 32, uint64 if W == 64
 *   RLWE accumulator    : [1 + kacc][N] ring words = (b, a_0 .. a_{kacc-1})   (lwe.jl:61-76)
 *   TransPoly           : M = N/2 complex doubles (re, im interleaved) in the order the reference's
 *                         transform leaves them (bit-reversed; fft.jl:105-155)
 *   BRK, RGSW schemes   : per party [n][(kr+1)*l_gsw rows][kr+1 polys] polynomials; rows ordered
 *                         basketb.stack[0..l), basketa[0].stack[0..l), ...  (gsw.jl:219-227);
 *                         polys ordered (b, a_0 ..) (lwe.jl:165-179); kr = k (SK) or 1 (KMS)
 *   BRK, CCS            : per party [n][3*l_uni]: d[0..l), then (f.stack[j].b, f.stack[j].a) j-major
 *                         (unienc.jl:92-99)
 *   KSK                 : per party [kr][N][Drows][f][n+1] uint32 LWE rows ([a.., b]); entry d
 *                         encrypts (d+1)*z_j*2^(32-(t+1)logD); Drows = D-1, or D/2 for the block
 *                         schemes (keygen.jl:17-23,:37,:141)
 */
#ifndef MKTFHE_H
#define MKTFHE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MKT_ABI_VERSION 3

typedef enum {
    MKT_OK = 0,
    MKT_ERR_ARG = -1,          /* bad argument / size mismatch (reference: @assert, polynomial.jl:10,19-20) */
    MKT_ERR_UNSUPPORTED = -2,  /* parameter combination not implemented */
    MKT_ERR_NO_DEVICE = -3,    /* no gfx950 device / HIP runtime failure at context creation */
    MKT_ERR_HIP = -4,          /* HIP runtime error, see mkt_last_error */
    MKT_ERR_STATE = -5,        /* keys not loaded */
    MKT_ERR_NOMEM = -6
} mkt_status;

/* scheme kinds: scheme.jl:107 (CGGI), :168 (LMSS), :209 (CCS), :256 (KMS), :301 (KMS_block) */
enum { MKT_CGGI = 0, MKT_LMSS = 1, MKT_CCS = 2, MKT_KMS = 3, MKT_KMS_BLOCK = 4 };
/* gates: gate.jl:1-53 */
enum { MKT_NAND = 0, MKT_AND = 1, MKT_OR = 2, MKT_XOR = 3, MKT_XNOR = 4, MKT_NOR = 5 };
/* per-gate codes of mkt_gate_batch_ops / _gather: a gate of the enum above, optionally with one or both inputs negated first
 * (NOT!, gate.jl:55-58, folded into the gate's linear part: the same words as NOT! followed by the gate) */
enum { MKT_OP_NOT_X = 8, MKT_OP_NOT_Y = 16, MKT_OP_NOT_Z = 32 };
/* three-input gates in ONE bootstrap (mkt_gate3_batch_*): codes 0-5 in bits 0-2, MKT_OP_NOT_X / _Y / _Z in bits 3-5, bits 6-7 clear.
 * Built as gate.jl builds a gate -- a linear part, then bootstrapping! (bootstrapping.jl:4-27) as a sign function -- with a third
 * operand: with a bit at +-2^29 (+-1/8) and x, y, z the operands after their flagged NOTs (NOT!, gate.jl:55-58), the linear part on
 * the 32-bit torus (constant added to the b word) and the truth for 0 / 1 / 2 / 3 true inputs are
 *   MKT_MAJ3  x + y + z                F F T T        MKT_MIN3   -(x + y + z)             T T F F
 *   MKT_XOR3  -2(x + y + z)            F T F T        MKT_XNOR3  2(x + y + z)             T F T F
 *   MKT_NAE3  x + y + z + 2^30         F T T F        MKT_AE3    3 2^30 - (x + y + z)     T F F T
 * (NAE3 = not all equal, AE3 = all equal).  The test vector is antiperiodic, f(phase + 1/2) = -f(phase), so these six are exactly the
 * symmetric three-input functions one bootstrap of the unweighted sum computes: AND3 and OR3 take two.  A full adder is
 * sum = XOR3, carry = MAJ3; per-input NOTs give the asymmetric variants (a subtractor's borrow is MAJ3(NOT a, b, c)).
 * NOISE: MAJ3 / MIN3 / NAE3 / AE3 put 3 sigma^2 on a margin of 1/8, XOR3 / XNOR3 12 sigma^2 on a margin of 1/4: in both cases
 * margin / sigma is sqrt(2/3) of a two-input gate's, so the per-gate failure rate of a set is much higher than for its two-input
 * gates (Gaussian predictions per shipped set, and measured rates). */
enum { MKT_MAJ3 = 0, MKT_MIN3 = 1, MKT_XOR3 = 2, MKT_XNOR3 = 3, MKT_NAE3 = 4, MKT_AE3 = 5 };
/* arithmetic modes of the negacyclic transform */
enum {
    MKT_ARITH_F64REF = 0, /* the reference's Float64 twisted FFT, operation for operation (fft.jl) */
    MKT_ARITH_EXACT = 1   /* EXACT products (what the reference's transform approximates, polynomial.jl:99-113; its MultiFloat option, README.md:9), two
                             implementations with the same words (option "exact_impl"): Float64 FMA transforms over centered 16-bit key limbs whose rounding
                             is proven exact for the loaded keys (fx_exact.hip: CGGI with RLWE length 1, KMS phase 1; mkt_get_metric "fx_bound"), and
                             exact integer arithmetic: the negacyclic NTT over Z_P[X]/(X^N+1) in residue form, P = p1 p2 =
                             (131063 * 2^13 + 1)(131066 * 2^13 + 1) = 2^59.9998, the two largest NTT primes below 2^30
                             (4 p < 2^32: lazy butterflies).
                             Transform-level entry points (mkt_transform_*_batch, mkt_exact_polymul_batch,
                             mkt_decompose_batch, mkt_modswitch_batch, mkt_not_batch) for every scheme; the gate path
                             (mkt_load_*, mkt_keygen_device, mkt_gate, mkt_bootstrap, mkt_blindrotate, mkt_keyswitch) for
                             MKT_CGGI / MKT_LMSS (any RLWE length and block length, 32-bit ring), MKT_CCS (32-bit ring) and MKT_KMS /
                             MKT_KMS_BLOCK (64-bit ring: every 64-bit table kept as the transforms of its two centered
                             32-bit pieces), provided the context's gadgets keep every product sum below P / 2 (checked at the
                             first key upload: MKT_ERR_UNSUPPORTED otherwise).  The ciphertexts are valid -- on the
                             64-bit ring 3-4x LESS noisy than the Float64 path, whose transform error dominates there --
                             but NOT the reference's words (no Float64 rounding); keys in MKT_FMT_INT_COEFF only.
                             On such a KMS context mkt_kms_phase1_batch returns the rows as split residue tables
                             [B][rows][2 polynomials][low, high half][N] uint64 (Montgomery form)   */
};
/* where batch pointers live.  ALIGNMENT: a buffer, in either memory, needs the alignment of its element type and no more -- 1 byte for gate codes,
 * 4 for 32-bit words, 8 for 64-bit words, 16 for the complex Float64 values of a transform -- whatever its row length: the kernels that move 16
 * bytes at a time find the 16-byte boundaries of a row themselves.  The one exception is stated at mkt_seeded_keys_expand, which refuses
 * (MKT_ERR_ARG) what it cannot take.  tests/test_gpu_footprint.py runs every batch call on buffers so aligned and no better. */
enum { MKT_MEM_DEVICE = 0, MKT_MEM_HOST = 1 };
/* key data formats */
enum {
    MKT_FMT_INT_COEFF = 0, /* coefficient-form ring words; the engine transforms on device
                              (replaces keygen.jl:14,:67,:99-108 `fft(..., ffter)`) */
    MKT_FMT_F64_FFT = 1    /* the reference's Trans* values (TransPoly layout above) */
};

/* parameter block: scheme.jl:6-101 / params.jl.  LWE word is 32 bit in every shipped set. */
typedef struct {
    int32_t scheme;          /* MKT_CGGI .. MKT_KMS_BLOCK */
    int32_t n;               /* LWE dimension per party (block schemes: blk_d * blk_len) */
    int32_t N;               /* ring dimension (power of two, 32..4096) */
    int32_t k;               /* SK: RLWE length (any; beyond 3 on a run-time-k kernel, F64REF only); MK: number of parties */
    int32_t W;               /* ring word bits: 32 or 64 */
    int32_t l_gsw, logB_gsw; /* RGSW gadget (CGGI/LMSS/KMS) */
    int32_t l_lev, logB_lev; /* LEV gadget (KMS) */
    int32_t l_uni, logB_uni; /* UniEnc gadget (CCS/KMS) */
    int32_t f, logD;         /* key-switch gadget */
    int32_t blk_len, blk_d;  /* block length and count (LMSS/KMS_block).  Any block length >= 1 is a valid parameter; an MKT_ARITH_F64REF context serves
                                block length 1 .. 4 at RLWE length 1 (LMSS with k = 1, KMS_block) and mkt_ctx_create refuses a longer one there with
                                MKT_ERR_UNSUPPORTED.  LMSS with k >= 2 and MKT_ARITH_EXACT contexts serve any block length */
} mkt_params;

typedef struct mkt_ctx mkt_ctx;
typedef struct mkt_client_party mkt_client_party;   /* one party's keys (client section below) */

/* ---- context: replaces the scheme object (scheme.jl:107-116 ...), FFTransformer (fft.jl:18-45)
 *      and getmonomial (scheme.jl:121-146), all built on device `device`. ---- */
int mkt_abi_version(void);
/* which source tree this library was built from: 16 hex digits of the SHA-256 over the engine's sources and build flags (csrc/Makefile).
 * Measurement bookkeeping only: profiles record it, bench.py quotes profile-derived numbers only for the library that produced them */
const char *mkt_build_id(void);
int mkt_ctx_create(const mkt_params *params, int arith_mode, int device, mkt_ctx **out);
int mkt_ctx_destroy(mkt_ctx *ctx);
/* a second context over the SAME resident keys and tables (no copy; freed with the last context that holds them; both
 * arithmetic modes): own stream, workspace and timing -- one per concurrent caller, matching the reference's contract of one read-only scheme
 * shared by concurrent bootstrapping! calls (bootstrapping.jl:38-45: all scratch is per call).  Once forked, the key set
 * is immutable: mkt_load_*, mkt_set_twiddles and mkt_keygen_device return MKT_ERR_STATE on every sharer. */
int mkt_ctx_fork(mkt_ctx *ctx, mkt_ctx **out);
const char *mkt_last_error(const mkt_ctx *ctx); /* ctx may be NULL: last creation error */
/* HIP stream (hipStream_t) all subsequent batch calls are enqueued on; NULL = default stream.  The per-batch workspace
 * belongs to the context, so CALLS ON ONE CONTEXT RUN IN THE ORDER THEY WERE MADE, WHATEVER STREAM EACH WAS ENQUEUED ON: when
 * mkt_set_stream moves the context to another stream, that stream first waits (one event, no host synchronisation) for everything
 * the context enqueued on the stream it leaves.  The stream it leaves must therefore still exist at that moment.  Naming the stream
 * the context is on already does nothing.  Only the context's own calls are ordered this way: one context still serves one host
 * thread at a time (a context per concurrent caller: mkt_ctx_fork).
 * STREAM ORDER.  A context made by mkt_ctx_create starts on the NULL stream.  A context made by mkt_ctx_fork starts on its
 * OWN stream, created hipStreamNonBlocking: its calls are NOT ordered against work on the NULL stream or on any other
 * stream.  A caller that hands MKT_MEM_DEVICE buffers to a fork must order producer and consumer itself: point the fork at
 * the producing stream (mkt_set_stream), or wait on the fork's stream (mkt_get_stream + events, or mkt_synchronize). */
int mkt_set_stream(mkt_ctx *ctx, void *hip_stream);
int mkt_get_stream(mkt_ctx *ctx, void **hip_stream);   /* the stream the context enqueues on right now */
int mkt_synchronize(mkt_ctx *ctx);
/* kernel-selection switches (where a step has more than one kernel, parity tests force each; A/B tools): name one of
 * "rot_variant", "rot_stagger", "rot_split", "rot_wide" (latency variant: 0 auto, 1 never, 2 always), "rot_blkg" (block
 * schemes, rotations per workgroup: 0 auto, 1, 2, 4), "rot_map" (workgroup -> (ciphertext, slot) dealing: 0 plain, 1 XCD-aware),
 * "ccs_stagger", "ccs_pipe" (-1 auto, 0 never, 1 always), "exact_wide" (MKT_ARITH_EXACT on the integer NTT, KMS phase 1 at l_gsw = 2 / KMS_block: 1 the default kernel, 0 the one-at-a-time form),
 * "exact_kany" (MKT_ARITH_EXACT CGGI / LMSS: 1 = the run-time-RLWE-length kernel also at k <= 3),
 * "exact_impl" (MKT_ARITH_EXACT blind rotation of CGGI with RLWE length 1 and of KMS phase 1, and mkt_exact_polymul_batch:
 * 0 = the integer NTT over two 30-bit primes, 1 = Float64 FMA transforms over 16-bit key limbs wherever the proven rounding bound
 * certifies the loaded keys (for mkt_exact_polymul_batch: the call's operands), -1 (default) = 1 for the gate paths, 0 for
 * mkt_exact_polymul_batch; both give the same words), "fx_polymul_force" (DIAGNOSTIC: 1 = mkt_exact_polymul_batch under exact_impl = 1
 * runs the Float64 kernel even where its bound does not certify the operands -- the words are then unproven; tests measure the kernel
 * at adversarial operands with it).  Results never depend on them, "fx_polymul_force" excepted.  The environment (MKT_ROT_*, MKT_CCS_*) seeds them once, at mkt_ctx_create; no batch call reads it. */
int mkt_set_option(mkt_ctx *ctx, const char *name, int value);
/* base name of the blind-rotation kernel the last batch call of this context launched ("" before the first); after
 * mkt_exact_polymul_batch the product kernel that served it: "fx_polymul_kernel" (Float64 pipe) or "exact_polymul_kernel" (integer NTT) */
const char *mkt_last_kernel_name(const mkt_ctx *ctx);
/* diagnostics of the Float64-pipe implementation of MKT_ARITH_EXACT: "fx_available" (1: the loaded keys are certified and exact_impl
 * admits it), "fx_bound" (proven bound on |computed - exact| of a rounded product sum for the loaded keys; must stay below 1/2),
 * "fx_kmax" (largest transform-domain magnitude of the loaded key limbs); of the last mkt_exact_polymul_batch of this context:
 * "polymul_amax" (max|a_i| over its batch), "fx_polymul_bound" (the proven bound of its Float64 product, evaluated under exact_impl = 1
 * before the kernel runs: below 0.45 the Float64 pipe served it; -1 = not evaluated), "fx_last_resid" (largest distance |q - round(q)|
 * met by the Float64 kernel: a DIAGNOSTIC beside the proven bound, not a certificate; 0 when the integer NTT served).
 * Of the blind-rotation launch that mkt_last_kernel_name names: "rot_static_l", "rot_static_logB" -- the gadget length and the log2 of the
 * gadget base that the instantiation which ran holds as COMPILE-TIME constants, each 0 where it takes the value at run time (and after
 * mkt_exact_polymul_batch).  They say which specialisation of a kernel name a call reached (the tests assert it); no result depends on them.
 * Of the context's last key switch (plain, at a coefficient, or inside a gate or bootstrap): "ks_last_kernel" -- 0 none yet, 1 the per-digit
 * kernel, 2 the digit-pair kernel, 3 the matrix cores --, "ks_last_g" (ciphertexts per wave tile), "ks_last_waves" (waves per workgroup),
 * "ks_last_slabs"; "ks_mfma_last" = 1 iff "ks_last_kernel" = 3.  What the MKT_KS_* variables chose; no result depends on them.
 * MEMORY GUARDS (diagnostic): with MKT_MEM_GUARD=<KiB> in the environment at mkt_ctx_create / mkt_multi_create (0 or unset: off; no batch call reads
 * it), every device buffer the library allocates from then on -- key tables, workspace, staged copies -- lies between two filled guards of that length.
 * "mem_guard_check" drains the context's device, compares the guards of every live buffer of that device and gives the number of guards found written
 * since the process started (buffers are also compared when they are freed; mkt_last_error then describes the latest finding: which guard, the
 * buffer's size, the first changed byte); "mem_guard_buffers" is how many buffers that sweep looked at, "mem_guard_released" how many were compared
 * at their release so far.  It sees stores only, and only those that leave a buffer by less than a guard */
int mkt_get_metric(mkt_ctx *ctx, const char *name, double *out);

/* twiddle tables (fft.jl:31-41): which = 0 Psi, 1 Psiinv, 2 roots, 3 rootsinv; M complex each.
 * mkt_set_twiddles lets a caller install the reference's own ffter tables verbatim.
 * ORDER: tables first, then keys.  Loaded keys are resident as their transforms under the tables in place when they arrived (or as the
 * caller's own Trans* values) and their integer form is not kept, so once a bootstrapping key, relinearisation key, public key or the CRS
 * is loaded (mkt_load_*, mkt_keygen_device, mkt_load_seeded_keys; either format) mkt_set_twiddles returns MKT_ERR_STATE and changes nothing. */
int mkt_get_twiddles(mkt_ctx *ctx, int which, double *out_host);
int mkt_set_twiddles(mkt_ctx *ctx, const double *psi, const double *psiinv,
                     const double *roots, const double *rootsinv);

/* host-only (no GPU needed): the engine's table generator for ring dimension N, same `which` */
int mkt_make_twiddles(int N, int which, double *out_host);

/* ---- evaluation keys (host pointers, copied; keygen.jl:3-155).  Every load works on the context's stream (mkt_set_stream) and returns with
 *      that stream drained, the host buffer free to reuse.  mkt_load_ksk too: it once wrote the table through the NULL stream, which a
 *      context pinned to a non-blocking stream does not wait for; now a batch still in flight on that stream reads the old key to its end,
 *      and every call after the load the new one ---- */
int mkt_load_brk(mkt_ctx *ctx, int party, const void *data, int fmt);
int mkt_load_ksk(mkt_ctx *ctx, int party, const uint32_t *data);
int mkt_load_rlk(mkt_ctx *ctx, int party, const void *d, const void *f, int fmt); /* KMS: keygen.jl:103 */
int mkt_load_pubkey(mkt_ctx *ctx, int party, const void *b, int fmt);             /* CCS/KMS: keygen.jl:67,:100 */
int mkt_load_crs(mkt_ctx *ctx, const void *a, int fmt);

/* ---- key generation on the device: replaces keygen.jl:13-23, :39-51, :71-79, :106-114,
 *      :143-151 (RGSW / UniEnc bootstrapping key, LEV key-switching key) for party `party`.  Exact integer arithmetic;
 *      `keys` holds the party's secrets (mkt_client_party_secrets or _keygen); `crs` = the integer CRS
 *      (mkt_client_crs) for CCS, NULL otherwise.  Equivalent to mkt_load_brk + mkt_load_ksk of the host-generated
 *      keys of the same seed, word for word.
 *      TRUST: this call hands party `party`'s SECRET keys to the GPU of this context.  It is a party-local operation:
 *      a party runs it on its own machine / GPU and ships the resulting evaluation keys (key blob) to the evaluator.
 *      An evaluator context that runs it for every party holds all k secrets -- acceptable only in tests and
 *      benchmarks.  The secret buffers are zeroed on the device before they are freed and the host-side copies of the
 *      party's stream key are wiped; the copy of that key carried in the kernel-argument segment of the keygen launches
 *      lives in runtime-owned memory the library cannot erase (it is overwritten by later launches). ---- */
int mkt_keygen_device(mkt_ctx *ctx, int party, const mkt_client_party *keys, const void *crs);
/* the same, and the keys are also copied to the host: brk_out in the MKT_FMT_INT_COEFF layout of mkt_load_brk, ksk_out
 * in the layout of mkt_load_ksk -- what a party ships to the evaluator after generating its keys on its own GPU */
int mkt_keygen_device_export(mkt_ctx *ctx, int party, const mkt_client_party *keys, const void *crs,
                             void *brk_out, uint32_t *ksk_out);
/* read a party's key-switching key back in the host layout of mkt_load_ksk (tests) */
int mkt_get_ksk(mkt_ctx *ctx, int party, uint32_t *out_host);                           /* scheme.jl:409-410 */

/* ---- hot path, batched: B independent ciphertexts per call (the reference does one per call) ---- */
/* gate.jl:1-53: out = bootstrapping!(linear(op, x, y)); x, y, out: [B][k*n+1] */
int mkt_gate_batch(mkt_ctx *ctx, int op, const uint32_t *x, const uint32_t *y, uint32_t *out, size_t B, int mem);
/* a different gate per ciphertext pair, one launch sequence for the batch -- the shape of the reference's tests, which draw a
 * random gate per step (test/KMS.jl:29-34): ops[j] = MKT_NAND .. MKT_NOR, optionally | MKT_OP_NOT_X / MKT_OP_NOT_Y; ops
 * lives where x, y, out live (`mem`) */
int mkt_gate_batch_ops(mkt_ctx *ctx, const uint8_t *ops, const uint32_t *x, const uint32_t *y, uint32_t *out, size_t B, int mem);
/* one level of a gate circuit: gate j reads rows ix[j] and iy[j] of pool [pool_rows][k*n+1] and writes out[j]; out may be a
 * later region of the same pool provided no gate of this call reads a row this call writes.
 * Validation: with MKT_MEM_HOST every index and gate code is checked (MKT_ERR_ARG).  With MKT_MEM_DEVICE the arrays cannot be read by
 * the host without a synchronising copy, so valid indices (< pool_rows) and codes (bits 0-2 <= MKT_NOR, bits 5-7 clear) are the CALLER's
 * precondition (mktfhe_amd/circuit.py builds them from a validated plan); what the engine guarantees regardless is memory safety -- an
 * index beyond the pool is clamped to its last row, a code is read modulo its defined bits -- never an out-of-bounds access.  The same
 * holds for mkt_gate_batch_ops and mkt_mux_batch_gather. */
int mkt_gate_batch_gather(mkt_ctx *ctx, const uint8_t *ops, const uint32_t *pool, size_t pool_rows, const uint32_t *ix,
                          const uint32_t *iy, uint32_t *out, size_t B, int mem);
/* three-input gates, one bootstrap each (codes above): out[j] = bootstrapping!(linear3(ops[j], x[j], y[j], z[j])); x, y, z, out: [B][k*n+1];
 * ops lives where x, y, z, out live (`mem`).  With MKT_MEM_HOST a bad code is MKT_ERR_ARG. */
int mkt_gate3_batch_ops(mkt_ctx *ctx, const uint8_t *ops, const uint32_t *x, const uint32_t *y, const uint32_t *z, uint32_t *out, size_t B, int mem);
/* one circuit level of three-input gates: gate j reads rows ix[j], iy[j], iz[j] of pool [pool_rows][k*n+1] and writes out[j]; out may
 * be a later region of the pool that no gate of this call reads.  Validation as mkt_gate_batch_gather: with MKT_MEM_HOST a bad code or
 * index is MKT_ERR_ARG; with MKT_MEM_DEVICE an index beyond the pool is clamped to its last row and a code is read modulo its defined
 * bits (gate values 6 and 7 act as MKT_AE3).  An empty pool is refused. */
int mkt_gate3_batch_gather(mkt_ctx *ctx, const uint8_t *ops, const uint32_t *pool, size_t pool_rows, const uint32_t *ix, const uint32_t *iy,
                           const uint32_t *iz, uint32_t *out, size_t B, int mem);
/* MUX(s, a, b) = s ? a : b -- named by the north star; the reference has no MUX gate (gate.jl:1-57).  Two blind rotations and one
 * key switch, built from the reference's own operators as CGGI16 builds it:
 *   acc = blindrotate!(AND-linear(s, a)) + blindrotate!(AND-linear(NOT! s, b)), + 1/8 at X^0 of acc.b;  out = keyswitch!(acc)
 * (a composite OR(AND(s, a), AND(NOT s, b)) of the reference's gates takes three full bootstraps).  s, a, b, out: [B][k*n+1] */
int mkt_mux_batch(mkt_ctx *ctx, const uint32_t *s, const uint32_t *a, const uint32_t *b, uint32_t *out, size_t B, int mem);
/* a circuit level of MUX gates: gate j = MUX(pool[is[j]], a', b') -> out[j], a' = pool[ia[j]] or its negation (NOT!) if bit 0 of
 * not_ab[j] is set, b' likewise with bit 1; not_ab may be NULL (rows of pool [pool_rows][k*n+1]; a negated selector = a and b swapped) */
int mkt_mux_batch_gather(mkt_ctx *ctx, const uint32_t *pool, size_t pool_rows, const uint32_t *is, const uint32_t *ia, const uint32_t *ib,
                         const uint8_t *not_ab, uint32_t *out, size_t B, int mem);
/* gate.jl:55-58 NOT!: in-place negation, no bootstrap */
int mkt_not_batch(mkt_ctx *ctx, uint32_t *x, size_t B, int mem);
/* bootstrapping.jl:4-27 bootstrapping!: in place on [B][k*n+1] */
int mkt_bootstrap_batch(mkt_ctx *ctx, uint32_t *lwe, size_t B, int mem);
/* bootstrapping.jl:8-9: atilde [B][k*n], btilde [B] */
int mkt_modswitch_batch(mkt_ctx *ctx, const uint32_t *lwe, uint32_t *atilde, uint32_t *btilde, size_t B, int mem);
/* blindrotate!(atilde, acc, scheme): acc [B][1+k][N] ring words, updated in place */
int mkt_blindrotate_batch(mkt_ctx *ctx, const uint32_t *atilde, void *acc, size_t B, int mem);
/* keyswitch!(res, acc, scheme): acc [B][1+k][N] -> out [B][k*n+1] */
int mkt_keyswitch_batch(mkt_ctx *ctx, const void *acc, uint32_t *out, size_t B, int mem);
/* KMS phase_1 (bootstrapping.jl:389-443 / :599-659) of every party: atilde [B][k*n] ->
 * levkey [B][Rtot][2][M] complex, Rtot = 1 + (k-1)*l_lev, party-major rows */
int mkt_kms_phase1_batch(mkt_ctx *ctx, const uint32_t *atilde, double *levkey, size_t B, int mem);

/* ---- programmable bootstrap: bootstrapping! (bootstrapping.jl:4-27) with a caller-supplied lookup table in place of its constant test
 *      vector.  A lookup table (LUT) is a test-vector polynomial T: N ring words.  For a ciphertext whose body word mod-switches to
 *      btilde in [0, 2N] (bootstrapping.jl:8-9, divbits), the accumulator handed to blindrotate! is acc = (X^btilde * T, 0, ..., 0) in
 *      Z[X]/(X^N + 1): with r = btilde mod N and s = -1 for N <= btilde < 2N, else +1 (btilde = 2N is the identity),
 *          acc.b[i] = s T[i - r] for i >= r,        acc.b[i] = -s T[N + i - r] for i < r.
 *      blindrotate! and keyswitch! follow unchanged.  With T = (-2^(W-3), ..., -2^(W-3)) this is bootstrapping.jl:11-23 word for word, and
 *      mkt_lut_bootstrap_batch returns the words of mkt_bootstrap_batch.
 *      LAYING OUT A TABLE.  The bootstrap rotates T by the mod-switched phase phi in [0, 2N) of the input and extracts coefficient 0:
 *          T[0] for phi = 0,        -T[N - phi] for 1 <= phi <= N,        T[2N - phi] for N < phi < 2N
 *      (times the ring word's scale; the key switch keeps the top 32 bits).  The function computed is negacyclic by construction,
 *      f(phi + 1/2) = -f(phi): a table is free on one half of the torus only (layout, recipes, noise).  Every ring word is
 *      a valid table entry; tables are not validated.
 *      luts: [nluts][N] ring words; sel: [B] rows of luts, or NULL = row 0 for the whole batch; both live where the ciphertexts live
 *      (`mem`).  Validation as mkt_gate_batch_gather: with MKT_MEM_HOST a sel[j] >= nluts or an operand index >= pool_rows is MKT_ERR_ARG
 *      and nothing is written; with MKT_MEM_DEVICE they are clamped to the last row -- never an out-of-bounds access.  nluts == 0 and
 *      gates over an empty pool are refused in either memory kind.  Both arithmetic modes, every scheme the gate path serves. ---- */
/* unit level: acc[j] = (X^btilde(lwe[j]) * luts[sel[j]], 0 ...); lwe [B][k*n+1], acc [B][1+k][N] ring words.  Needs no keys */
int mkt_lut_testvector_batch(mkt_ctx *ctx, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lwe, void *acc, size_t B, int mem);
/* out[j] = keyswitch!(blindrotate!(acc[j] as above)); lwe, out: [B][k*n+1]; out may alias lwe */
int mkt_lut_bootstrap_batch(mkt_ctx *ctx, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lwe, uint32_t *out, size_t B, int mem);
/* one circuit level of table lookups: gate j bootstraps  cst[j] e_b + sum_{t<4} wt[j][t] pool[idx[j][t]]  through luts[sel[j]] -> out[j]
 * (pool [pool_rows][k*n+1]; idx [B][4] rows; wt [B][4] int8 weights, 0 = no term; cst [B] added to the b word); out may be a later region of
 * the pool that no gate of this call reads */
int mkt_lut_batch_gather(mkt_ctx *ctx, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *pool, size_t pool_rows,
                         const uint32_t *idx, const int8_t *wt, const uint32_t *cst, uint32_t *out, size_t B, int mem);

/* ---- many-table bootstrap (Chillotti et al., "PBSmanyLUT"): nout = 2^nu functions of ONE encrypted input for one blind rotation and
 *      nout key switches.  nout is 1, 2, 4 or 8 and at most N; any other count is MKT_ERR_ARG and nothing is written.
 *      COARSE MOD-SWITCH.  Every 32-bit LWE word w, mask words and b alike, goes onto a grid nout times coarser:
 *          sw(w) = divbits32(w, 32 - (log2 N + 1) + nu) << nu,
 *      a multiple of nout in [0, 2N] (2N is the identity, as above); nu = 0 is mkt_modswitch_batch word for word.  The rotated phase is
 *      then a multiple of nout too.
 *      PACKED TABLE.  From tables T_0 .. T_{nout-1} laid out as above, U[nout i + v] = T_v[nout i] for 0 <= i < N / nout: only every
 *      nout-th entry of a table is ever read.  For every phase phi in {0, nout, ..., 2N - nout}, coefficient v of X^phi * U is what a
 *      single-table bootstrap of T_v extracts at phi.  `luts` holds PACKED tables here: [nluts][N] ring words, `sel` as above.
 *      EXTRACTION AT COEFFICIENT v.  E_v(acc) = X^-v * acc on every one of the 1 + k polynomials: E_v(acc)[c][i] = acc[c][i + v] for
 *      i + v < N, -acc[c][i + v - N] otherwise.  Output v of input j is keyswitch!(E_v(blindrotate!(sw(a), (X^sw(b) * U, 0, ...)))).
 *      nout = 1 returns the words of mkt_lut_bootstrap_batch.  The output noise is that of any bootstrap; the INPUT's mod-switch error
 *      grows nout-fold.  No copy E_v(acc) is made: the key switch reads coefficient v of the rotated accumulator where it
 *      lies, as the bootstrap at the coefficient list 0 .. nout - 1 does (next block); mkt_lut_extract_batch is the definition as a unit call.
 *      Validation of luts, sel, pool indices: as in the programmable-bootstrap block.  Both arithmetic modes, every scheme. ---- */
/* out [B][nout][k*n+1]: output v of input j at row j * nout + v.  out must not overlap lwe when nout > 1 (MKT_ERR_ARG) */
int mkt_lut_many_bootstrap_batch(mkt_ctx *ctx, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lwe, int nout, uint32_t *out, size_t B,
                                 int mem);
/* the linear front end of mkt_lut_batch_gather, then the above; out [B][nout][k*n+1] may be a later region of the pool that no gate of
 * this call reads */
int mkt_lut_many_batch_gather(mkt_ctx *ctx, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *pool, size_t pool_rows,
                              const uint32_t *idx, const int8_t *wt, const uint32_t *cst, int nout, uint32_t *out, size_t B, int mem);
/* unit level: atilde [B][k*n] = sw of the mask words, acc[j] = (X^sw(b) * luts[sel[j]], 0 ...) [B][1+k][N].  Needs no keys */
int mkt_lut_many_testvector_batch(mkt_ctx *ctx, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lwe, int nout, uint32_t *atilde,
                                  void *acc, size_t B, int mem);
/* unit level: accs[j][v] = E_v(acc[j]); acc [B][1+k][N] -> accs [B][nout][1+k][N], which must not overlap acc.  Needs no keys */
int mkt_lut_extract_batch(mkt_ctx *ctx, const void *acc, int nout, void *accs, size_t B, int mem);

/* ---- key switch at a coefficient; the bootstrap at a coefficient list: ncoef outputs of ONE blind rotation with no copy of the accumulator.
 *      keyswitch! sample-extracts coefficient 0.  With E_v(acc) = X^-v * acc as defined above, keyswitch!(E_v(acc)) reads acc itself at
 *      other places: the body word is acc.b[v] >> (W - 32), and word j of a mask component a is  a[v] >> (W - 32)  for j = 0,
 *      -((-a[v - j]) >> (W - 32))  for 0 < j <= v (the inner negation at the ring's width, as E_v writes it: on the 32-bit ring this is
 *      a[v - j]),  -(a[N + v - j] >> (W - 32))  for j > v.  Every output row g names its accumulator src[g] and its coefficient coef[g].
 *      WHAT IT COMPUTES.  Coefficient v of X^phi * T is what a single-table bootstrap of T reads at phase phi - v: one rotation returns
 *      f(m - w) for every shift w asked for, at the fine mod-switch (nu = 0).  E_v is a signed permutation, so the output noise is that of
 *      one bootstrap and the input margin that of one lookup.  THERMOMETER.  With the sign table and coef[w] = w N / P,
 *      output w of an input on window m of P (phase m / 2P + 1 / 4P) decrypts to [m >= w], for all w < P at once.
 *      nu in 0 .. 3 with 2^nu <= N is the coarse mod-switch sw of the many-table block (nu = 0: mkt_modswitch_batch); 1 <= ncoef <= N and
 *      coef[i] < N.  Word for word:  mkt_keyswitch_at_batch(src = coef = NULL) = mkt_keyswitch_batch;  mkt_lut_bootstrap_at_batch(nu = 0,
 *      coef = {0}) = mkt_lut_bootstrap_batch;  (nu = log2 o, coef = {0 .. o-1}) on a packed table = mkt_lut_many_bootstrap_batch(nout = o).
 *      src, coef and sel live where the ciphertexts live (`mem`).  Validation as mkt_gate_batch_gather: with MKT_MEM_HOST a src[g] >= nacc,
 *      a coef >= N or a sel >= nluts is MKT_ERR_ARG and nothing is written; with MKT_MEM_DEVICE src is clamped to the last row and coef
 *      read mod N -- never an out-of-bounds access.  nacc == 0 with B > 0, ncoef == 0 or > N, a bad nu, and src == NULL with nacc != B are
 *      refused in either memory kind; B == 0 succeeds and writes nothing.  A call runs in chunks of max(1, 8192 / ncoef) inputs (8192 rows
 *      for mkt_keyswitch_at_batch).  No buffer of extracted accumulators exists: the key switch reads the rotated accumulators
 *      in the workspace through a (row, coefficient) table of 8 bytes per output row.  Both arithmetic modes, every scheme; forks hold
 *      their own workspace. ---- */
/* out[g] = keyswitch!(E_{coef[g]}(acc[src[g]])); acc [nacc][1+k][N] ring words, out [B][k*n+1]; src [B] or NULL (= g; then nacc must
 * equal B), coef [B] or NULL (= 0) */
int mkt_keyswitch_at_batch(mkt_ctx *ctx, const void *acc, size_t nacc, const uint32_t *src, const uint32_t *coef, uint32_t *out, size_t B, int mem);
/* one rotation per input, ncoef outputs: out[j][i] = keyswitch!(E_{coef[i]}(blindrotate!(sw_nu(a_j), (X^sw_nu(b_j) * luts[sel[j]], 0, ...))));
 * coef [ncoef], shared by the batch; out [B][ncoef][k*n+1] must not overlap lwe when ncoef > 1 (MKT_ERR_ARG) */
int mkt_lut_bootstrap_at_batch(mkt_ctx *ctx, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lwe, int nu, const uint32_t *coef,
                               size_t ncoef, uint32_t *out, size_t B, int mem);
/* the linear front end of mkt_lut_batch_gather, then the above; out [B][ncoef][k*n+1] may be a later region of the pool that no gate of
 * this call reads */
int mkt_lut_batch_gather_at(mkt_ctx *ctx, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *pool, size_t pool_rows,
                            const uint32_t *idx, const int8_t *wt, const uint32_t *cst, int nu, const uint32_t *coef, size_t ncoef, uint32_t *out,
                            size_t B, int mem);

/* ---- unit-level entry points (parity tests, transform roofline) ----
 * On an MKT_ARITH_EXACT context a TransPoly is N residue pairs (x mod p1) | (x mod p2) << 32 (uint64, the same 8 N bytes as
 * M complex doubles), in the bit-reversed order the Cooley-Tukey network with psi_rev[m + i] leaves them; forward reads
 * ring words as SIGNED integers, inverse returns the integer of least magnitude mod P (the identity for |x| < P / 2),
 * reduced mod 2^W. */
/* fft.jl:57-63 fftto!: p [B][N] ring words -> t [B][M] complex */
int mkt_transform_fwd_batch(mkt_ctx *ctx, const void *p, double *t, size_t B, int mem);
/* fft.jl:74-81 ifftto!: t [B][M] complex -> p [B][N] ring words (t is left unmodified) */
int mkt_transform_inv_batch(mkt_ctx *ctx, const double *t, void *p, size_t B, int mem);
/* gsw.jl:86-96 decompto!: p [B][N] -> digits [B][l][N] ring words (wrapped signed digits) */
int mkt_decompose_batch(mkt_ctx *ctx, const void *p, void *digits, int l, int logB, size_t B, int mem);
/* MKT_ARITH_EXACT only: out = a (*) b in Z_{2^W}[X]/(X^N+1), EXACTLY, for a gadget-digit polynomial a (signed W-bit words,
 * N * max|a_i| <= 2^28 - 2^15 over the whole batch) and any ring polynomial b -- the product the reference's Float64 transform approximates
 * (polynomial.jl:99-113); a, b, out: [B][N] ring words.  The bound keeps every true coefficient of a times a centered 32-bit piece of b,
 * at most N max|a| 2^31, below P / 2 = 2^59 - 6.6e13 (the integer NTT's lift; it would wrap from N max|a| = 268 404 738 on).  max|a_i| is
 * measured on the device; a batch outside the bound is refused with MKT_ERR_ARG and no words are written.  Under exact_impl = 1 the
 * Float64 pipe serves the call where its proven error bound for these operands (from max|a_i| and the measured transform maximum of
 * b's 16-bit limbs) is below 0.45, the integer NTT otherwise -- the same words (mkt_last_kernel_name says which served). */
int mkt_exact_polymul_batch(mkt_ctx *ctx, const void *a, const void *b, void *out, size_t B, int mem);
/* scheme.jl:121-146: copy monomial table entry e (1..2N) to host, M complex */
int mkt_get_monomial(mkt_ctx *ctx, int e, double *out_host);

/* ---- one evaluator over several GPUs, one caller process (the reference's caller is ONE process whose threads
 *      share one read-only scheme: README.md:38-44, bootstrapping.jl:38-45).  Shard i runs on HIP device devices[i]; naming a
 *      device more than once makes logical shards that share that device's ONE key set (forked contexts).  Keys are loaded /
 *      generated once, on devices[0]; mkt_multi_replicate copies the resident pre-transformed tables to the other devices
 *      (hipMemcpyPeer over xGMI; host bounce if refused) and seals them.  A batch call cuts [0, B) into contiguous balanced
 *      slices (the first B mod nshards slices hold one more: mkt_multi_shard_range), one host thread per shard, every shard
 *      writing its slice of the caller's ONE output array; no collective.  MKT_MEM_DEVICE arrays may live on any of the
 *      devices (slices are peer-copied to and from the shards on other devices).  Calls return when all shards are done; one call
 *      at a time per handle (the shards' workspaces and staging buffers belong to it) -- concurrent callers take one handle each, or
 *      fork the shard contexts (mkt_multi_ctx + mkt_ctx_fork). ---- */
typedef struct mkt_multi mkt_multi;
/* flags: MKT_MULTI_PRIVATE_KEYS = shards that share a device do NOT share its key set: each gets its own replicated copy, as
 * shards on distinct devices do (exercises the device-to-device replication on a one-GPU box; costs one key copy per shard) */
/* MKT_MULTI_STAGE_ALWAYS = device-resident arguments always travel through the shards' staging buffers (peer copies), as they do
 * for a shard on another device than the array's (that path on a one-GPU box) */
/* MKT_MULTI_NO_PEER = every device-to-device copy (key replication, staged arguments) goes through a host buffer instead of
 * hipMemcpyPeer: the path the engine falls back to by itself where a peer copy is refused, selectable so that it can be tested */
enum { MKT_MULTI_PRIVATE_KEYS = 1, MKT_MULTI_STAGE_ALWAYS = 2, MKT_MULTI_NO_PEER = 4 };
int mkt_multi_create(const mkt_params *params, int arith_mode, const int *devices, int nshards, int flags, mkt_multi **out);
int mkt_multi_destroy(mkt_multi *m);
const char *mkt_multi_last_error(const mkt_multi *m);  /* m may be NULL: last creation error */
int mkt_multi_nshards(const mkt_multi *m);
int mkt_multi_device(const mkt_multi *m, int shard);
mkt_ctx *mkt_multi_ctx(mkt_multi *m, int shard);        /* borrowed: timing (mkt_enable_timing), kernel names; NULL for a logical shard before mkt_multi_replicate */
int mkt_multi_shard_range(const mkt_multi *m, size_t B, int shard, size_t *lo, size_t *hi);
int mkt_multi_load_brk(mkt_multi *m, int party, const void *data, int fmt);
int mkt_multi_load_ksk(mkt_multi *m, int party, const uint32_t *data);
int mkt_multi_load_rlk(mkt_multi *m, int party, const void *d, const void *f, int fmt);
int mkt_multi_load_pubkey(mkt_multi *m, int party, const void *b, int fmt);
int mkt_multi_load_crs(mkt_multi *m, const void *a, int fmt);
int mkt_multi_keygen_device(mkt_multi *m, int party, const mkt_client_party *keys, const void *crs);
int mkt_multi_replicate(mkt_multi *m);
int mkt_multi_set_option(mkt_multi *m, const char *name, int value);
int mkt_multi_gate_batch(mkt_multi *m, int op, const uint32_t *x, const uint32_t *y, uint32_t *out, size_t B, int mem);
int mkt_multi_gate_batch_ops(mkt_multi *m, const uint8_t *ops, const uint32_t *x, const uint32_t *y, uint32_t *out, size_t B, int mem);
int mkt_multi_gate3_batch_ops(mkt_multi *m, const uint8_t *ops, const uint32_t *x, const uint32_t *y, const uint32_t *z, uint32_t *out, size_t B, int mem);
int mkt_multi_mux_batch(mkt_multi *m, const uint32_t *s, const uint32_t *a, const uint32_t *b, uint32_t *out, size_t B, int mem);
int mkt_multi_bootstrap_batch(mkt_multi *m, uint32_t *lwe, size_t B, int mem);
/* mkt_lut_bootstrap_batch, sharded: lwe, out and sel are cut with the batch; every shard reads all of luts (in place, or staged per shard) */
int mkt_multi_lut_bootstrap_batch(mkt_multi *m, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lwe, uint32_t *out, size_t B, int mem);
/* sharded as mkt_multi_lut_bootstrap_batch; out [B][nout][k*n+1] is cut at nout rows per input */
int mkt_multi_lut_many_bootstrap_batch(mkt_multi *m, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lwe, int nout, uint32_t *out,
                                       size_t B, int mem);
/* mkt_lut_bootstrap_at_batch, sharded by input as the call above: out is cut at ncoef rows per input; coef reaches every shard as luts does */
int mkt_multi_lut_bootstrap_at_batch(mkt_multi *m, const void *luts, size_t nluts, const uint32_t *sel, const uint32_t *lwe, int nu,
                                     const uint32_t *coef, size_t ncoef, uint32_t *out, size_t B, int mem);
int mkt_multi_not_batch(mkt_multi *m, uint32_t *x, size_t B, int mem);
int mkt_multi_blindrotate_batch(mkt_multi *m, const uint32_t *atilde, void *acc, size_t B, int mem);
int mkt_multi_keyswitch_batch(mkt_multi *m, const void *acc, uint32_t *out, size_t B, int mem);

/* Device-time accounting with hipEvents recorded on the context's stream around each kernel class:
 * mkt_enable_timing(ctx, 1) clears and starts recording, mkt_last_kernel_ms stores the TOTAL ms of
 * class `which` (0 = whole call, 1 = blind rotation, 2 = key switch, 3 = transform, 4 = KMS phase 2)
 * since then and returns the number of recorded launches (average = total / count); <0 on error. */
int mkt_enable_timing(mkt_ctx *ctx, int on);
int mkt_last_kernel_ms(mkt_ctx *ctx, int which, double *ms);

/* ---- client side (host only, no GPU): counterparts of the reference's key generation and encryption,
 *      exact integer arithmetic.  setup/party_keygen scheme.jl:151,:190,:227,:273,:324; keygen.jl;
 *      lwe_encrypt scheme.jl:352-386; lwe_decrypt scheme.jl:388-407; CRS scheme.jl:409
 *
 *      RANDOMNESS.  Every `seed` below is a 256-bit value (32 bytes) keying ChaCha20 streams, or NULL.
 *      NULL -- what a caller should pass -- draws a fresh seed from the OS (getrandom) for that call, as the
 *      reference draws fresh ChaCha20 entropy per call (sampler.jl:1-34).  A pinned seed makes keys and
 *      ciphertexts reproducible and therefore PUBLIC: pinned seeds (mkt_client_test_seed) are for tests and
 *      benchmarks only. ---- */
int mkt_client_random_seed(uint8_t out[32]);            /* 32 bytes of OS entropy */
int mkt_client_test_seed(uint64_t n, uint8_t out[32]);  /* TESTS / BENCHMARKS ONLY: deterministic expansion of n */
/* crs: [l_uni][N] ring words (MK schemes) */
int mkt_client_crs(const mkt_params *params, const uint8_t *seed, void *crs_out);
/* one party's secret + evaluation keys; crs may be NULL for SK schemes; sigma_lwe/sigma_ring are the
 * absolute noise standard deviations alpha/beta of params.jl */
int mkt_client_party_keygen(const mkt_params *params, const uint8_t *seed, int party, const void *crs,
                            double sigma_lwe, double sigma_ring, mkt_client_party **out);
/* the same party WITHOUT the two large keys (bootstrapping key, key-switching key: mkt_client_brk / _ksk are empty):
 * secrets, public key and relinearisation key only -- for mkt_keygen_device, which generates the large keys on the
 * GPU from the same streams (identical words to mkt_client_party_keygen with the same seed) */
int mkt_client_party_secrets(const mkt_params *params, const uint8_t *seed, int party, const void *crs,
                             double sigma_lwe, double sigma_ring, mkt_client_party **out);
int mkt_client_party_destroy(mkt_client_party *p);   /* wipes the secrets */
/* sizes in bytes / pointers to the flat key material (layouts above), valid until destroy */
const uint32_t *mkt_client_lwekey(const mkt_client_party *p);             /* [n] 0/1 */
/* ring secret polynomial idx, N entries 0/1 (SK schemes: idx < k; CCS: 0; KMS: 0 = gsw key, 1 = uni key); key.jl */
const int8_t *mkt_client_ringkey(const mkt_client_party *p, int idx, size_t *bytes);
const void *mkt_client_brk(const mkt_client_party *p, size_t *bytes);     /* INT_COEFF */
const uint32_t *mkt_client_ksk(const mkt_client_party *p, size_t *bytes);
const void *mkt_client_rlk_d(const mkt_client_party *p, size_t *bytes);
const void *mkt_client_rlk_f(const mkt_client_party *p, size_t *bytes);
const void *mkt_client_pubkey(const mkt_client_party *p, size_t *bytes);
/* lwe_encrypt (SK: party = 0) / lwe_ith_encrypt (MK): out [k*n+1] */
int mkt_client_lwe_encrypt(const mkt_params *params, const mkt_client_party *p, int party, int bit,
                           double sigma_lwe, const uint8_t *seed, uint32_t *out);
/* the same encryption of ANY message mu on the 32-bit torus (mkt_client_lwe_encrypt is mu = +-2^29): multi-valued inputs of a programmable
 * bootstrap.  Same streams: with the same seed and mu = +-2^29 the words of mkt_client_lwe_encrypt */
int mkt_client_lwe_encrypt_word(const mkt_params *params, const mkt_client_party *p, int party, uint32_t mu,
                                double sigma_lwe, const uint8_t *seed, uint32_t *out);
/* lwe_decrypt: keys = nparties pointers; returns 0/1, <0 on error */
int mkt_client_lwe_decrypt(const mkt_params *params, const mkt_client_party *const *keys, int nparties,
                           const uint32_t *lwe);
/* the phase lwe_decrypt rounds: message + noise on the 32-bit torus.  In this library's sign convention (the mask is stored with the sign
 * that makes decryption a sum) that is b + sum_i <a_i, s_i> */
int mkt_client_lwe_phase(const mkt_params *params, const mkt_client_party *const *keys, int nparties, const uint32_t *lwe, uint32_t *phase);

/* ---- distributed decryption: every party opens its OWN block of the mask; nobody holds two secrets.  mkt_client_lwe_decrypt / _phase take
 *      all k secret keys in one process (the reference's lwe_decrypt, scheme.jl:388-407, a test harness); the multi-key protocols
 *      behind the CCS and KMS schemes (Chen, Chillotti, Song 2019; Kwak, Min, Song 2022) end instead with one share per party, blurred by
 *      fresh noise, that anyone may add up.
 *      LAYOUT.  Unchanged: a row is [a_0 (n words) .. a_{nparty-1} (n words), b], 32-bit words; nparty = k for the multi-key schemes and 1
 *      for MKT_CGGI / MKT_LMSS whatever their RLWE length.
 *      SHARE.  Party i's share of row j of a batch is  share_i[j] = sum_q a_i[q] * s_i[q] + e_i[j]  (mod 2^32): wrapping uint32_t arithmetic,
 *      the key word multiplied (not assumed binary), as mkt_client_lwe_phase does.  Only block i of the row is read.
 *      SMUDGING NOISE.  e_i[j] = (uint32_t) Rng(key, i, 9, lo32(row0 + j), hi32(row0 + j)).noise(sigma_smudge): the ChaCha20 streams of
 *      every client call (256-bit `seed` as in the RANDOMNESS note above, NULL = fresh OS entropy per call), stream id 9, one stream per
 *      row, its first Gaussian draw rounded.  sigma_smudge is a standard deviation in words of the 32-bit torus (the unit of sigma_lwe); it
 *      must be finite with 0 <= sigma_smudge <= 2^31, anything else is MKT_ERR_ARG and no word is written.  row0 is the index of the
 *      call's first row in a larger logical batch: a caller streams one batch in pieces under one seed without drawing a noise word twice.
 *      A SEED MUST NEVER SERVE TWO DIFFERENT CIPHERTEXTS AT ONE ROW INDEX: the difference of the two shares is then noise-free.
 *      MERGE.  phase[j] = b[j] + sum_i share_i[j]; the bit is what mkt_client_lwe_decrypt decides from that phase for the scheme.  With
 *      sigma_smudge = 0 the merged phase is mkt_client_lwe_phase word for word.  Merging needs no key.
 *      WHAT IS NOT CLAIMED.  No sigma_smudge is certified as simulation-secure: on a 32-bit torus with a decision margin of 1/8 the
 *      flooding noise a statistical argument asks for does not fit.  The value is the deployment's choice (failure
 *      predictions per shipped set). ---- */
/* lwe [B][lwe_len] -> share_out [B]; keys = party `party`'s keys, made for these parameters and that party index.  B == 0 succeeds */
int mkt_client_partial_decrypt(const mkt_params *params, const mkt_client_party *keys, int party, const uint32_t *lwe, double sigma_smudge,
                               const uint8_t *seed, uint64_t row0, uint32_t *share_out, size_t B);
/* shares [nparties][B] (party-major) -> phase_out [B] / bits_out [B] (0 / 1); nparties must be the scheme's party count (MKT_ERR_ARG) */
int mkt_client_merge_phase(const mkt_params *params, const uint32_t *lwe, const uint32_t *shares, int nparties, uint32_t *phase_out, size_t B);
int mkt_client_merge_decrypt(const mkt_params *params, const uint32_t *lwe, const uint32_t *shares, int nparties, uint8_t *bits_out, size_t B);
/* the share on the GPU of `ctx`, for a party that opens many rows: the same words as mkt_client_partial_decrypt for the same seed and
 * row0.  lwe and share_out live in `mem` (MKT_MEM_DEVICE / MKT_MEM_HOST); the call runs on the context's stream and needs NO evaluation
 * key loaded (a context made by mkt_ctx_create alone serves).  It returns once the share is written and the key copy is wiped.
 * TRUST: this call hands party `party`'s SECRET LWE key to the GPU of this context.  It is a party-local operation: a party runs it on
 * its own machine / GPU and ships the shares to whoever merges.  An evaluator context that runs it for every party holds all k secrets
 * -- acceptable only in tests and benchmarks.  The n key words are uploaded per call and zeroed on the device before they are freed, and
 * the host-side copy of the stream key is wiped; the copy of that key carried in the kernel-argument segment of the launch lives in
 * runtime-owned memory the library cannot erase (it is overwritten by later launches). */
int mkt_partial_decrypt_batch(mkt_ctx *ctx, int party, const mkt_client_party *keys, const uint32_t *lwe, double sigma_smudge, const uint8_t *seed,
                              uint64_t row0, uint32_t *share_out, size_t B, int mem);

/* ---- seeded ciphertexts: a fresh ciphertext of party i is (k-1) n zero words, n uniform mask words that say nothing about the message, and
 *      one body word.  A party therefore sends a PUBLIC 256-bit mask seed and one body word per ciphertext, and whoever holds the seed
 *      regenerates the rows -- on the evaluator's GPU, where they are needed.  A SEEDED BATCH of party i is (mask_seed[32], row0, i,
 *      body[B]); row0 is the index of its first row in a larger logical batch, as for a decryption share above.
 *      LAYOUT.  Unchanged: an expanded row is an ordinary ciphertext [a_0 .. a_{nparty-1}, b] that every call of this header accepts.
 *      MASK.  Word q < n of row j is 32-bit word (q & 15) of chacha20_block(key(mask_seed), q >> 4, nonce), nonce the one of
 *      Rng(key, i, 10, lo32(row0 + j), hi32(row0 + j)): stream id 10, one stream per row, RFC 8439 block function with the block counter
 *      starting at 0.  Every keystream word is used (the 64-bit draws of the other streams keep one word in two); the surplus words of a
 *      row's last block are dropped.  key(seed) = the 32 bytes as eight little-endian words, as for every seed of this header.
 *      NOISE.  e[j] = (uint32_t) Rng(key(noise_seed), i, 11, lo32(row0 + j), hi32(row0 + j)).noise(sigma_lwe): stream id 11, the first
 *      Gaussian draw of the row's stream, rounded.  noise_seed is SECRET; NULL -- what a caller should pass -- is fresh OS entropy per call.
 *      BODY.  body[j] = e[j] - sum_q a[j][q] * s_i[q] + mu[j]  (mod 2^32): wrapping uint32_t arithmetic, the key word multiplied (not
 *      assumed binary), as mkt_client_lwe_encrypt_word does.  mu is any word of the 32-bit torus; a bit is mu = +-2^29.
 *      EXPANSION.  Row j is all zeros except block i, which holds the mask, and the last word, which holds body[j]; so
 *      mkt_client_lwe_phase(expand(...)) == mu + e word for word.  Expansion needs no key.
 *      REFUSALS (MKT_ERR_ARG, no word written): mask_seed NULL; noise_seed given and bytewise equal to mask_seed (publishing the one would
 *      publish the noise); party out of range; keys made for other parameters or another party index; sigma_lwe not finite, negative or
 *      above 2^31; an unknown `mem`.  B == 0 succeeds and writes nothing.
 *      A (mask_seed, party, row index) MUST NEVER SERVE TWO ENCRYPTIONS: the two rows then share their mask, and the difference of the two
 *      bodies is the difference of the messages plus two noise words.  Draw a fresh mask seed (mkt_client_random_seed) per batch, or
 *      continue one batch under its seed with row0.
 *      mkt_client_lwe_encrypt(_word) and its stream 7 are unchanged; their rows cannot be compressed this way. ---- */
/* mu [B] -> body_out [B]; keys = party `party`'s keys, made for these parameters and that party index */
int mkt_client_seeded_encrypt(const mkt_params *params, const mkt_client_party *keys, int party, const uint32_t *mu, double sigma_lwe,
                              const uint8_t *mask_seed, const uint8_t *noise_seed, uint64_t row0, uint32_t *body_out, size_t B);
/* body [B] -> out [B][k*n+1] */
int mkt_client_seeded_expand(const mkt_params *params, int party, const uint8_t *mask_seed, uint64_t row0, const uint32_t *body, uint32_t *out,
                             size_t B);
/* the evaluator's call: the rows of mkt_client_seeded_expand written on the GPU of `ctx`, word for word.  body and out live in `mem`
 * (MKT_MEM_DEVICE / MKT_MEM_HOST); the call runs on the context's stream and needs NO evaluation key loaded (a context made by
 * mkt_ctx_create alone serves).  It reads B words and writes B * (k*n+1); nothing it touches is secret. */
int mkt_seeded_expand_batch(mkt_ctx *ctx, int party, const uint8_t *mask_seed, uint64_t row0, const uint32_t *body, uint32_t *out, size_t B, int mem);
/* the party's call on its OWN GPU: the words of mkt_client_seeded_encrypt for the same seeds and row0.  mu and body_out live in `mem`; the
 * call runs on the context's stream, needs no evaluation key and returns once the bodies are written and the key copy is wiped.  The mask
 * words are never written to device memory.
 * TRUST: as mkt_partial_decrypt_batch, this call hands party `party`'s SECRET LWE key and the noise seed to the GPU of this context.  It is
 * a party-local operation; an evaluator context that runs it for every party holds all k secrets -- acceptable only in tests and
 * benchmarks.  The n key words are uploaded per call and zeroed on the device before they are freed, and the host-side copy of the noise
 * stream key is wiped; the copy of that key carried in the kernel-argument segment of the launch lives in runtime-owned memory the
 * library cannot erase (it is overwritten by later launches). */
int mkt_seeded_encrypt_batch(mkt_ctx *ctx, int party, const mkt_client_party *keys, const uint32_t *mu, double sigma_lwe, const uint8_t *mask_seed,
                             const uint8_t *noise_seed, uint64_t row0, uint32_t *body_out, size_t B, int mem);

/* ---- seeded evaluation keys: almost all of a party's two large keys is public randomness -- every key-switching-key row is n uniform words
 *      and one body word, every RLWE sample of the bootstrapping key kr uniform polynomials and one body polynomial.  A party therefore ships a
 *      PUBLIC 256-bit mask seed and the bodies (the COMPACT sections below), and the evaluator regenerates the masks on its GPU, where the
 *      resident tables live.  This is a key form of its own beside mkt_client_party_keygen, whose calls, streams and words are unchanged; the
 *      expanded keys are ordinary keys in the layouts at the top of this header.  New symbols only: MKT_ABI_VERSION is unchanged.
 *      STREAMS.  Keyed by the PUBLIC mask seed, read as 32-bit words with every keystream word used (as stream 10 of the seeded ciphertexts):
 *      12, key-switching-key mask; 13, bootstrapping-key mask.  Keyed by the party's SECRET seed (the `seed` of the keygen call), 64-bit draws
 *      as every other secret stream: 14 noise of the RGSW bootstrapping key, 15 noise of the key-switching key, 16 UniEnc (CCS).  Streams 1, 3, 4
 *      are those of mkt_client_party_keygen: with the same seed the secrets, the public key and the relinearisation key are the same, word for
 *      word.  Streams 2 and 5 are not read: a party that publishes both key forms from one seed shares no noise between them.
 *      KEY-SWITCHING KEY.  Row index R = ((c N + j) Drows + d) f + t.  Mask word q < n of row R is 32-bit word (q & 15) of
 *      chacha20_block(key(mask_seed), q >> 4, {12 | party << 16, lo32(R), hi32(R)}); the surplus of a row's last block is dropped.
 *      e_R = (uint32_t) Rng(key(seed), party, 15, lo32(R), hi32(R)).noise(sigma_lwe), the first draw of the row's stream.
 *      body[R] = e_R - sum_q a_R[q] * s[q] + msg(c, j, d, t),  msg = ((d + 1) z_c[j]) << (32 - (t + 1) logD)  (mod 2^32, wrapping uint32_t
 *      arithmetic, the key word multiplied; z = the uni key for the KMS schemes).  For the block schemes (MKT_LMSS, MKT_KMS_BLOCK) the rows
 *      with c N + j < n are absent (keygen.jl:46,:147): their body is 0, and expansion leaves the whole row zero without generating a mask.
 *      BOOTSTRAPPING KEY, RGSW (all schemes but MKT_CCS).  Sample index S = i rows + c l_gsw + j (key bit i, rows = (kr + 1) l_gsw, row
 *      (c, j) as in the BRK layout above); mask polynomial index P = S kr + cc.  Coefficient q of mask polynomial P comes from
 *      chacha20_block(key(mask_seed), blk, {13 | party << 16, lo32(P), hi32(P)}): on the 32-bit ring word (q & 15) of block q >> 4, on the
 *      64-bit ring  w[2 (q & 7)] | w[2 (q & 7) + 1] << 32  of block q >> 3.  Noise: Rng(key(seed), party, 14, lo32(S), hi32(S)), N draws
 *      noise(sigma_ring) in coefficient order.  THE MESSAGE IS IN THE BODY: for every row a_cc is the public mask unmodified, and
 *          b = -sum_cc a_cc z_cc + e + s_i g_j m_c,    g_j = 2^(W - (j + 1) logB_gsw),  m_0 = 1 (coefficient 0 only),  m_c = z_{c-1} for c >= 1.
 *      The reference adds s_i g_j to coefficient 0 of the MASK a_{c-1} (gsw.jl:174-178); under a public mask that word would reveal s_i.
 *      a -> a + s_i g_j X^0 is a bijection on uniform masks, so the distribution is the reference's, the phase b + sum a z =
 *      e + s_i g_j z_{c-1} is the same, and the expanded key is an ordinary key.
 *      BOOTSTRAPPING KEY, UniEnc (MKT_CCS).  d_j = crs_j r + s_i g_j + e depends on the common CRS, not on a fresh mask: the d rows ship in
 *      full.  f_j = (b, a): a = mask polynomial P = i l_uni + j of stream 13 as above, b = -a z + e + g_j r.  ONE secret stream per key bit,
 *      Rng(key(seed), party, 16, i), read in this order: N draws next() % 3 - 1 (the ternary r); then for j = 0 .. l_uni - 1: N draws
 *      noise(sigma_ring) for d_j, N draws noise(sigma_ring) for f_j.b, each in coefficient order.
 *      COMPACT LAYOUTS.  ksk_seeded: uint32 [kr][N][Drows][f], bodies only (index R).  brk_seeded, RGSW: [n][(kr + 1) l_gsw][N] ring words,
 *      the b polynomials (index S).  brk_seeded, CCS: [n][2 l_uni][N]: d_0 .. d_{l-1}, then f_0.b .. f_{l-1}.b.  Expansion yields exactly the
 *      MKT_FMT_INT_COEFF layout of mkt_load_brk and the layout of mkt_load_ksk.
 *      TRUST.  The mask seed is NOT a secret: it travels with the bodies, and anyone may expand.  The secret seed is, as ever.
 *      A (MASK SEED, PARTY) PAIR SERVES ONE KEY GENERATION.  TWO GENERATIONS UNDER IT SHARE THEIR MASKS, AND THEIR BODIES DIFFER BY NOISE
 *      ALONE (under one secret) OR BY <a, s - s'> (under two).  Draw a fresh mask seed (mkt_client_random_seed) per generation.
 *      REFUSALS (MKT_ERR_ARG): mask_seed NULL; seed given and bytewise equal to mask_seed (publishing the one would publish the secrets);
 *      party out of range; a compact section without its output or the reverse (expansion).
 *      NOT SEEDED: the small keys (public key, relinearisation key: O(l) polynomials), which ship as before. ---- */
/* one party's secrets, small keys and the compact sections; mkt_client_brk / _ksk are empty on it, as after mkt_client_party_secrets */
int mkt_client_party_keygen_seeded(const mkt_params *params, const uint8_t *seed, const uint8_t *mask_seed, int party, const void *crs,
                                   double sigma_lwe, double sigma_ring, mkt_client_party **out);
const void *mkt_client_brk_seeded(const mkt_client_party *p, size_t *bytes);      /* compact layout above; valid until destroy */
const uint32_t *mkt_client_ksk_seeded(const mkt_client_party *p, size_t *bytes);
const uint8_t *mkt_client_mask_seed(const mkt_client_party *p);                   /* 32 bytes; NULL unless the party is a seeded one */
/* the definition of expansion, host only, needs no key: brk_out in the MKT_FMT_INT_COEFF layout of mkt_load_brk, ksk_out in the layout of
 * mkt_load_ksk.  Either pair (brk_seeded, brk_out) / (ksk_seeded, ksk_out) may be NULL */
int mkt_client_seeded_keys_expand(const mkt_params *params, int party, const uint8_t *mask_seed, const void *brk_seeded, const uint32_t *ksk_seeded,
                                  void *brk_out, uint32_t *ksk_out);
/* the same words written by the GPU of `ctx` into caller memory; the four arrays live in `mem`.  With MKT_MEM_DEVICE, brk_seeded and brk_out must
 * be 16-byte aligned (the kernel moves them 16 bytes at a time): another pointer is MKT_ERR_ARG, before anything is launched or written.  Needs no
 * key loaded and changes no resident table */
int mkt_seeded_keys_expand(mkt_ctx *ctx, int party, const uint8_t *mask_seed, const void *brk_seeded, const uint32_t *ksk_seeded, void *brk_out,
                           uint32_t *ksk_out, int mem);
/* the evaluator's call (host pointers in; either section may be NULL): the resident state of mkt_load_brk + mkt_load_ksk fed with the host
 * expansion, including the Float64-pipe limbs and "fx_bound" of an MKT_ARITH_EXACT context.  The expanded key never travels to the host: the
 * key-switching key is generated into its resident table, the bootstrapping key into the coefficient-form staging buffer mkt_keygen_device
 * uses and pre-transformed from there; peak extra device memory = that buffer plus the compact sections.  MKT_ERR_STATE once the key set is
 * shared (mkt_ctx_fork); MKT_ERR_UNSUPPORTED where mkt_load_brk is */
int mkt_load_seeded_keys(mkt_ctx *ctx, int party, const uint8_t *mask_seed, const void *brk_seeded, const uint32_t *ksk_seeded);
int mkt_multi_load_seeded_keys(mkt_multi *m, int party, const uint8_t *mask_seed, const void *brk_seeded, const uint32_t *ksk_seeded);
/* the compact sections GENERATED ON THE PARTY'S OWN GPU: brk_seeded_out / ksk_seeded_out (HOST pointers, the compact layouts above; both given or
 * both NULL) receive the sections mkt_client_party_keygen_seeded(params, seed, mask_seed, party, crs, sigmas of `keys`) writes for the seed `keys`
 * was made from, word for word: noise from the secret streams 14, 15, 16, masks from the public streams 12, 13 keyed by `mask_seed`.  The
 * large keys are never expanded, on the host or on the device.  `keys` is any party object of these parameters and this party index
 * (mkt_client_party_keygen, _secrets or _keygen_seeded): only its secrets, its stream key and its sigmas are read.  `crs` = the integer CRS
 * for MKT_CCS, NULL otherwise.
 * install = 0: changes no resident table, needs no key loaded, runs on the context's stream; a context from mkt_ctx_create alone serves it.
 * install = 1: the sections, still on the device, are also expanded and installed: the resident state of mkt_load_seeded_keys fed with them,
 * including the Float64-pipe limbs and "fx_bound" of an MKT_ARITH_EXACT context; refused as mkt_keygen_device is (MKT_ERR_STATE once the key
 * set is shared, MKT_ERR_UNSUPPORTED where mkt_load_brk is).
 * REFUSALS (MKT_ERR_ARG, no output word written, no resident table touched): mask_seed NULL; mask_seed, read as eight little-endian words,
 * equal to the party's stream key (publishing it would publish the secrets); party out of range; `keys` made for other parameters or another
 * party; MKT_CCS without crs; exactly one output NULL; both outputs NULL with install = 0.
 * TRUST: this call hands party `party`'s SECRET keys to the GPU of this context.  It is a party-local operation: a party runs it on its own
 * machine / GPU and ships the compact sections with the mask seed (key blob, format version 2) to the evaluator.  An evaluator context that
 * runs it for every party holds all k secrets -- acceptable only in tests and benchmarks.  The secret buffers (LWE key, ring keys) are zeroed
 * on the device before they are freed and the host-side copies of the party's stream key are wiped; the copy of that key carried in the
 * kernel-argument segment of the launches lives in runtime-owned memory the library cannot erase (it is overwritten by later launches).  The
 * compact sections and the mask seed are public.  A (mask seed, party) pair serves one key generation, as above */
int mkt_keygen_device_seeded(mkt_ctx *ctx, int party, const mkt_client_party *keys, const void *crs, const uint8_t *mask_seed, void *brk_seeded_out,
                             uint32_t *ksk_seeded_out, int install);

#ifdef __cplusplus
}
#endif
#endif
