/*
 * mktfhe_pack.h -- packed outputs: N result ciphertexts folded into ONE RLWE ciphertext on the GPU (packing key switch, LWE -> RLWE).
 *
 * An extension of mktfhe.h (new symbols only: MKT_ABI_VERSION is unchanged).  Results leave the evaluator of mktfhe.h as LWE rows of
 * k*n + 1 words; N of them fit one RLWE ciphertext [1 + k][N] whose coefficient j carries the phase of row j -- (k*n + 1) * 4 * N bytes
 * against (1 + k) * N * W / 8.  The reference has no packing key switch; it is built here from the reference's own operators, cited by line.
 *
 * NOTATION.  kr = 1 for the multi-key schemes (MKT_CCS, MKT_KMS, MKT_KMS_BLOCK), kr = k for MKT_CGGI / MKT_LMSS (the ring components one
 * party's key-switching key covers).  nparty = k for the multi-key schemes, 1 otherwise.  An LWE row is [a_0 (n words) .. a_{nparty-1}, b].
 * Every polynomial lives in Z_{2^W}[X]/(X^N + 1); the sign convention is the library's: phase = b + sum_c a_c z_c.
 *
 * GADGET.  (l_pk, logB_pk), chosen by the caller at key generation and at load -- not a field of mkt_params, which is ABI.
 *     1 <= logB_pk <= 16,   1 <= l_pk,   l_pk * logB_pk <= 32            (anything else: MKT_ERR_ARG)
 * g_t = 2^(W - (t + 1) logB_pk), t < l_pk.  All parties of a context use one gadget.  On an MKT_ARITH_EXACT context a gadget whose product
 * rows could reach P / 2 (N 2^(logB_pk - 1) 2^31 >= P / 2, P the two-prime modulus of mktfhe.h) is refused at load with MKT_ERR_UNSUPPORTED.
 *
 * RING KEY.  The ring key(s) the key-switching key switches FROM: the uni key (mkt_client_ringkey index 1) for MKT_KMS / MKT_KMS_BLOCK, key 0
 * for MKT_CCS, keys 0 .. k-1 for MKT_CGGI / MKT_LMSS.  A packed ciphertext is therefore an ordinary accumulator of mkt_keyswitch_at_batch,
 * which reads an LWE row back out of any of its coefficients.  Slot of component c of party i in the ciphertext: slot(i, c) = i for the
 * multi-key schemes (c = 0), c otherwise (i = 0); polynomial 1 + slot of [1 + k][N].
 *
 * PACKING KEY of party i: [n][l_pk][1 + kr][N] ring words, polynomials ordered (b, a_0 ..).  Row (q, t) is an RLWE sample (lwe.jl:78-93)
 * under z_{i,0 .. kr-1} of  s_i[q] * g_t  at coefficient 0 -- rlev_encrypt (lev.jl:88-94) of the constant s_i[q]: a_c uniform,
 * b = -sum_c a_c z_c + e + s_i[q] g_t X^0, e of deviation sigma_ring (the party's, in ring words).  It encrypts bits of s_i under z_i as the
 * bootstrapping key does: no new assumption.
 * STREAMS (rng_chacha.h; ids 1-16 are taken): 17, the packing key -- keyed by the `seed` of mkt_client_packing_keygen, one stream
 * Rng(key(seed), i, 17, q, t) per row, read as rlwe_sample reads it: for c < kr the N mask words of a_c (64-bit draws masked to W bits), then
 * N draws noise(sigma_ring) in coefficient order.  18, the smudging noise of a ring share -- keyed by the `seed` of
 * mkt_client_rlwe_partial_decrypt, one stream Rng(key(seed), i, 18, lo32(row0 + g), hi32(row0 + g)) per PACK, N draws noise(sigma_smudge) in
 * coefficient order.  Both are SECRET streams; NULL seed = fresh OS entropy per call.
 *
 * PACK.  Rows x_0 .. x_{B-1} of a pool [pool_rows][k*n + 1], picked by idx[B] (NULL: rows 0 .. B-1).  Pack g takes rows g N ..
 * min(B, (g + 1) N) - 1 at coefficients 0 ..; absent rows are zero.  Output [ceil(B / N)][1 + k][N] ring words.  For each pack:
 *     P_{i,q}(X) = sum_j (x_j.a_i[q] << (W - 32)) X^j
 *     D_{i,q,t}  = decompto! (gsw.jl:86-96, mkt_decompose_batch) of P_{i,q} with the packing gadget, t = 0 most significant
 *     G_{i,q}    = one gadget product formed exactly as bootstrapping.jl:62-72 forms one: fftto! of every digit polynomial, initialise!,
 *                  muladdto! over t ascending for each of the 1 + kr key polynomials of row (q, t), one ifftto! each back to ring words
 *     out.b             = sum_j (x_j.b << (W - 32)) X^j + sum_{i,q} G_{i,q}.b
 *     out.a_{slot(i,c)} = sum_q G_{i,q}.a_c
 * all sums wrapping integer sums mod 2^W.  The Float64 operation order is fixed INSIDE a gadget product; the sums ACROSS (i, q) are integer
 * and order-free.  Phase: coefficient j of out.b + sum a z is  phase(x_j) << (W - 32)  plus the key-switch error
 *     sum_{i,q,t} D_{i,q,t} e_{i,q,t}  +  sum_{i,q} s_i[q] (recomposed - lifted a_i[q])        (predicted deviation).
 * ARITHMETIC.  MKT_ARITH_F64REF: the gadget product is the Float64 one above, bit for bit.  MKT_ARITH_EXACT: every product D (*) key polynomial
 * is exact (the product kernel behind mkt_exact_polymul_batch), the key stays resident in coefficient form.
 *
 * TRUST.  The packing key is an evaluation key: public, shipped to the evaluator with the others.  mkt_client_rlwe_phase is a test harness
 * that takes all secrets; the protocol's end is one ring share per party (mkt_client_rlwe_partial_decrypt), merged by anyone.
 *
 * SEEDED (DESIGN.md 1h "Seeded, in a blob, made on the party's GPU").  kr of the 1 + kr polynomials of every row are uniform randomness, so a
 * party ships a PUBLIC 256-bit mask seed and the b polynomials, and the evaluator regenerates the masks -- the seeded form of mktfhe.h "seeded
 * evaluation keys", for the third large key.  The message s_i[q] g_t already sits in the body, so nothing else changes.
 * STREAMS 19 and 20 (rng_chacha.h; ids 1-18 are taken).
 *   19, STREAM_PACK_MASK: keyed by the PUBLIC mask seed and read through stream_block exactly as stream 13 is.  Mask polynomial
 *     P = (q l_pk + t) kr + c.  32-bit ring: coefficient j = word j & 15 of block j >> 4; 64-bit ring: words 2 (j & 7), 2 (j & 7) + 1 of block
 *     j >> 3, low word first.  The stream index is  P | (uint64)(l_pk | logB_pk << 8) << 32:  P always fits 32 bits, the gadget rides in the high
 *     word.  This domain separation is required, not decoration: under one mask seed two generations with DIFFERENT gadgets would otherwise
 *     share the mask of row (q, t), their bodies would differ by s_i[q] (g_t - g'_t) plus noise, and that opens the LWE key bit to anyone.
 *   20, STREAM_PACK_NOISE: keyed by the party's SECRET seed, Rng(key(seed), i, 20, q, t): N draws noise(sigma_ring) in coefficient order, from
 *     the first draw; no mask is drawn from it.  Stream 17 is not read: a party that publishes both forms from one seed shares no noise
 *     between them.
 * ROW (q, t): a_c = mask polynomial P, unmodified;  b = -sum_c a_c (*) z_c + e + s_i[q] 2^(W - (t + 1) logB_pk) X^0;  z as above (RING KEY).
 * COMPACT LAYOUT pk_seeded: [n][l_pk][N] ring words, the b polynomials.  Expansion yields exactly the layout of mkt_load_packing_key,
 * [n][l_pk][1 + kr][N] ordered (b, a_0 ..): the expanded key is an ordinary packing key.  Sizes at the gadget (4, 4): KMS2party 73.4 MB ->
 * 36.7 MB per party, CGGIparam 20.6 MB -> 10.3 MB.
 * A (MASK SEED, PARTY) PAIR SERVES ONE PACKING-KEY GENERATION PER GADGET: two generations under it with one gadget share their masks, and the
 * difference of their bodies is noise alone.  The same public mask seed may serve the party's seeded evaluation keys too (mktfhe.h): the
 * stream ids differ.  The mask seed is published; it must not be the generation seed nor the seed of the party's secrets (MKT_ERR_ARG).
 * TRUST of mkt_packing_keygen_device: the trust paragraph of mkt_keygen_device_seeded (mktfhe.h) applies verbatim -- a PARTY-LOCAL call that
 * hands the party's secret keys and the stream key of its noise to this context's GPU, the party's own; on a shared evaluator it would hand the
 * secrets to the evaluator.  The secrets are uploaded for the length of the call, zeroed on the device before they are freed, and the host
 * copy of the stream key in the kernel-argument struct is zeroed with them.
 *
 * NOT HERE: mkt_multi_* variants, the ring share on the GPU, mod-switching the packed ciphertext, rotating it as a table.
 */
#ifndef MKTFHE_PACK_H
#define MKTFHE_PACK_H

#include "mktfhe.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- host (no GPU) ---- */
/* party `party`'s packing key in the layout above -> pk_out, [n][l_pk][1 + kr][N] ring words.  keys = that party's keys, made for these
 * parameters and that party index (its LWE key, ring keys and sigma_ring are read).  seed: 256 bits keying stream 17, NULL = fresh.
 * MKT_ERR_ARG: NULL pointers, a bad gadget, party out of range, foreign or wrong-party keys */
int mkt_client_packing_keygen(const mkt_params *params, const mkt_client_party *keys, int party, int l_pk, int logB_pk, const uint8_t *seed,
                              void *pk_out);
/* the same key in the SEEDED form above -> pk_seeded_out, [n][l_pk][N] ring words (the bodies).  seed: 256 bits keying the SECRET stream 20,
 * NULL = fresh; mask_seed: the PUBLIC 256 bits keying stream 19, which the party ships with the bodies.  MKT_ERR_ARG, nothing written: what
 * mkt_client_packing_keygen refuses, mask_seed NULL, seed given and bytewise equal to mask_seed, mask_seed equal to the seed of the party's secrets */
int mkt_client_packing_keygen_seeded(const mkt_params *params, const mkt_client_party *keys, int party, int l_pk, int logB_pk, const uint8_t *seed,
                                     const uint8_t *mask_seed, void *pk_seeded_out);
/* the definition of expansion: pk_seeded [n][l_pk][N] -> pk_out [n][l_pk][1 + kr][N], bodies copied, masks from stream 19.  Needs no key.
 * MKT_ERR_ARG, nothing written: NULL pointers, a bad gadget, party out of range */
int mkt_client_packing_key_expand(const mkt_params *params, int party, int l_pk, int logB_pk, const uint8_t *mask_seed, const void *pk_seeded,
                                  void *pk_out);
/* TEST HARNESS (needs all keys): phase_out[j] = the top 32 bits of coefficient j of  b + sum_slot a_slot z_slot,  computed exactly;
 * rlwe [1 + k][N] ring words, keys = nparties pointers in party order */
int mkt_client_rlwe_phase(const mkt_params *params, const mkt_client_party *const *keys, int nparties, const void *rlwe, uint32_t *phase_out);
/* the ring form of mkt_client_partial_decrypt: rlwe [G][1 + k][N] -> share_out [G][N] RING words,
 *     share_i[g] = sum_c a_{slot(i,c)}[g] (*) z_{i,c} + e[g]   (mod 2^W),
 * e[g] = N words of stream 18 at pack index row0 + g, deviation sigma_smudge IN 32-BIT-TORUS WORDS (the unit of mkt_client_partial_decrypt;
 * on the 64-bit ring the draw is lifted by 32 bits), finite with 0 <= sigma_smudge <= 2^31 (MKT_ERR_ARG otherwise, nothing written).
 * A SEED MUST NEVER SERVE TWO DIFFERENT CIPHERTEXTS AT ONE PACK INDEX: the difference of the two shares is then noise-free.  No
 * sigma_smudge is certified as simulation-secure (mktfhe.h "distributed decryption").  G == 0 succeeds */
int mkt_client_rlwe_partial_decrypt(const mkt_params *params, const mkt_client_party *keys, int party, const void *rlwe, double sigma_smudge,
                                    const uint8_t *seed, uint64_t row0, void *share_out, size_t G);
/* ONE packed ciphertext rlwe [1 + k][N] and its shares [nparties][N] ring words (party-major) -> the first `count` <= N coefficients:
 * phase_out[j] = top 32 bits of  b[j] + sum_i share_i[j];  bits_out[j] = what mkt_client_lwe_decrypt decides from that phase.  With
 * sigma_smudge = 0 the merged phase is mkt_client_rlwe_phase word for word.  Needs no key; nparties must be the scheme's party count */
int mkt_client_rlwe_merge_phase(const mkt_params *params, const void *rlwe, const void *shares, int nparties, size_t count, uint32_t *phase_out);
int mkt_client_rlwe_merge_decrypt(const mkt_params *params, const void *rlwe, const void *shares, int nparties, size_t count, uint8_t *bits_out);

/* ---- device ---- */
/* party `party`'s packing key (HOST pointer, coefficient form, the layout above) becomes resident on the context's device: pre-transformed
 * on an MKT_ARITH_F64REF context as the bootstrapping key is, in coefficient form on an MKT_ARITH_EXACT one.  Same write guard as every key
 * load: MKT_ERR_STATE once the key set is shared (mkt_ctx_fork); forks share the resident key.  The first load fixes the context's gadget; a
 * later load with another gadget is MKT_ERR_ARG.  RLWE lengths kr > 3 are MKT_ERR_UNSUPPORTED.  Like every key that is resident as a
 * transform, a loaded packing key makes mkt_set_twiddles return MKT_ERR_STATE */
int mkt_load_packing_key(mkt_ctx *ctx, int party, const void *pk, int l_pk, int logB_pk);
/* the words of mkt_client_packing_key_expand, written on the context's device and stream into caller memory: pk_seeded and pk_out both live in
 * `mem`.  Needs no key loaded and changes no resident table.  With MKT_MEM_DEVICE both pointers must be 16-byte aligned (the kernel moves 16
 * bytes at a time): MKT_ERR_ARG otherwise, before anything is launched -- the rule of mkt_seeded_keys_expand.  Returns once the words are written */
int mkt_packing_key_expand(mkt_ctx *ctx, int party, int l_pk, int logB_pk, const uint8_t *mask_seed, const void *pk_seeded, void *pk_out, int mem);
/* mkt_load_packing_key of the expansion of (mask_seed, pk_seeded), HOST pointers: exactly the same resident state, the masks regenerated on the
 * device (MKT_ARITH_F64REF: expanded into a staging buffer, then pre-transformed slot-major; MKT_ARITH_EXACT: written in coefficient form,
 * [polynomial][row], by the expansion kernel itself).  The expanded key never travels to the host.  Refusals as mkt_load_packing_key, plus
 * mask_seed NULL.  One party may load seeded and another unseeded in one context */
int mkt_load_packing_key_seeded(mkt_ctx *ctx, int party, const uint8_t *mask_seed, const void *pk_seeded, int l_pk, int logB_pk);
/* PARTY-LOCAL (TRUST above): the words of mkt_client_packing_keygen_seeded for the same `seed`, word for word, made on this context's device
 * -> pk_seeded_out (HOST, may be NULL with install).  seed: the generation seed as in the host call; NULL draws fresh entropy ON THE HOST and
 * only the derived ChaCha20 key goes to the device -- in the kernel-argument struct, the way the party's stream key reaches the device in
 * mkt_keygen_device_seeded.  install = 1: the bodies, still on the device, are also expanded and installed as mkt_load_packing_key_seeded
 * would (its refusals apply, checked before anything runs).  install = 0 needs no key loaded and changes no resident table; with a NULL
 * output it is MKT_ERR_ARG.  MKT_ERR_ARG, nothing written and no table touched: mask_seed NULL, seed given and equal to mask_seed, mask_seed
 * equal to the seed of the party's secrets, a bad gadget, party out of range, foreign or wrong-party keys */
int mkt_packing_keygen_device(mkt_ctx *ctx, int party, const mkt_client_party *keys, int l_pk, int logB_pk, const uint8_t *seed,
                              const uint8_t *mask_seed, void *pk_seeded_out, int install);
/* the pack defined above: pool [pool_rows][k*n + 1], idx [B] or NULL, rlwe_out [ceil(B / N)][1 + k][N] ring words, all living in `mem`.
 * Validation as mkt_gate_batch_gather: with MKT_MEM_HOST an idx[j] >= pool_rows is MKT_ERR_ARG and nothing is written; with MKT_MEM_DEVICE
 * indices are clamped to the last row.  idx NULL needs B <= pool_rows.  B == 0 succeeds and writes nothing; an empty pool with B > 0 and an
 * rlwe_out that overlaps the pool are MKT_ERR_ARG.  MKT_ERR_STATE until every party's packing key is loaded; no other key is needed.
 * The call keeps a workspace of its own and leaves the gate workspace, the options and mkt_last_kernel_name as it found them */
int mkt_pack_batch(mkt_ctx *ctx, const uint32_t *pool, size_t pool_rows, const uint32_t *idx, size_t B, void *rlwe_out, int mem);

#ifdef __cplusplus
}
#endif
#endif
