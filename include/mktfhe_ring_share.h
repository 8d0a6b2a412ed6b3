/*
 * mktfhe_ring_share.h -- ring shares of packed results on the party's own GPU.
 *
 * An extension of mktfhe_pack.h, as that header extends mktfhe.h (new symbols only: MKT_ABI_VERSION is unchanged).  mktfhe_pack.h lists "the
 * ring share on the GPU" under NOT HERE: this header supplies that item.  Every other party-side step of the protocol already has a device
 * form -- seeded inputs (mkt_seeded_encrypt_batch), keys (mkt_keygen_device_seeded, mkt_packing_keygen_device), LWE decryption shares
 * (mkt_partial_decrypt_batch) --; the ring share with which a party opens a PACKED result existed on the host alone, as a sequential loop
 * over packs (mkt_client_rlwe_partial_decrypt).
 *
 * DEFINITION.  That of mkt_client_rlwe_partial_decrypt (mktfhe_pack.h), unchanged: for pack g of rlwe [G][1 + k][N]
 *     share_i[g] = sum_c a_{slot(i,c)}[g] (*) z_{i,c} + e[g]   (mod 2^W),
 * z_{i,c} the ring key(s) of mktfhe_pack.h "RING KEY" (the uni key for MKT_KMS / MKT_KMS_BLOCK, key 0 for MKT_CCS, keys 0 .. k-1 for MKT_CGGI /
 * MKT_LMSS), the ciphertext polynomial 1 + i for the multi-key schemes and 1 + c otherwise, the product negacyclic and wrapping mod 2^W;
 * coefficient j of e[g] is draw j of Rng(key(seed), i, 18, lo32(row0 + g), hi32(row0 + g)).noise(sigma_smudge), shifted left by W - 32 bits and
 * added mod 2^W.  The device call returns the words of the host call for the same (params, keys, party, rlwe, sigma_smudge, seed, row0, G),
 * word for word: both sides run wrapping integer arithmetic, one ChaCha20 block function and one Box-Muller with contraction off.  No stream
 * id is added; stream 18 is the one of mktfhe_pack.h.
 *
 * SEED.  seed: 256 bits keying stream 18, NULL = fresh OS entropy per call, drawn on the host; only the derived ChaCha20 key travels.  row0 is
 * the index of the call's first PACK in a larger logical batch opened in pieces under one seed.
 * A SEED MUST NEVER SERVE TWO DIFFERENT CIPHERTEXTS AT ONE PACK INDEX: the difference of the two shares is then noise-free.  No sigma_smudge is
 * certified as simulation-secure (mktfhe.h "distributed decryption").
 *
 * TRUST: as mkt_partial_decrypt_batch (mktfhe.h), for the ring keys: this call hands party `party`'s SECRET ring key(s) to the GPU of this
 * context.  It is a party-local operation: a party runs it on its own machine / GPU and ships the shares to whoever merges.  An evaluator
 * context that runs it for every party holds all k secrets -- acceptable only in tests and benchmarks.  The key polynomials are uploaded per
 * call and zeroed on the device before they are freed, and the host-side copy of the stream key is wiped; the copy of that key carried in the
 * kernel-argument segment of the launch lives in runtime-owned memory the library cannot erase (it is overwritten by later launches).
 *
 * NOT HERE: mkt_multi_* variants of the pack and of the share, mod-switching a packed ciphertext or its shares to 32-bit words,
 * a device merge (k + 1 additions per coefficient: mkt_client_rlwe_merge_decrypt serves), rotating a packed ciphertext as a table.
 */
#ifndef MKTFHE_RING_SHARE_H
#define MKTFHE_RING_SHARE_H

#include "mktfhe_pack.h"

#ifdef __cplusplus
extern "C" {
#endif

/* PARTY-LOCAL (TRUST above).  rlwe [G][1 + k][N] ring words -> share_out [G][N] ring words, both living in `mem` (MKT_MEM_DEVICE /
 * MKT_MEM_HOST).  ALIGNMENT as in mktfhe.h: a buffer needs the alignment of its element type (4 bytes on the 32-bit ring, 8 on the 64-bit
 * one) and no more.  keys = party `party`'s keys, made for these parameters and that party index.  The call runs on the context's stream and
 * needs NO evaluation key and NO packing key loaded: a context made by mkt_ctx_create alone serves, and so does a fork.  It gives the same
 * words on an MKT_ARITH_F64REF and an MKT_ARITH_EXACT context, leaves the gate workspace, the options and mkt_last_kernel_name as it found
 * them, and returns once the shares are written and the secret copies are wiped.
 * MKT_ERR_ARG, no word written and nothing launched: what mkt_client_rlwe_partial_decrypt refuses (keys NULL, sigma_smudge not finite or
 * outside 0 .. 2^31, party out of range, foreign or wrong-party keys, rlwe or share_out NULL with G > 0) and an unknown `mem`.  G == 0 succeeds */
int mkt_rlwe_partial_decrypt_batch(mkt_ctx *ctx, int party, const mkt_client_party *keys, const void *rlwe, double sigma_smudge,
                                   const uint8_t *seed, uint64_t row0, void *share_out, size_t G, int mem);

#ifdef __cplusplus
}
#endif
#endif
