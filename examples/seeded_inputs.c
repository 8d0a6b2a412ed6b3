/* Seeded ciphertexts through the C ABI (include/mktfhe.h "seeded ciphertexts"): two-party KMS, NAND of bits that the two parties send as
 * a public mask seed and one body word per bit instead of full rows:
 *   party 0     seeded-encrypts its bits on the host                                  (mkt_client_seeded_encrypt)
 *   party 1     seeded-encrypts its bits on a GPU context of its own, no evaluation key loaded   (mkt_seeded_encrypt_batch)
 *   evaluator   evaluation keys only; regenerates both parties' rows on its GPU from (seed, bodies) and computes z = NAND(x, y)
 *               (mkt_seeded_expand_batch, mkt_gate_batch)
 * Per bit a party ships 4 bytes (and 32 bytes of seed per batch) where a full row has 4 (2 n + 1).  The result is opened with all keys
 * (mkt_client_lwe_decrypt) to check it; examples/distributed_decrypt.c shows the opening in which nobody holds two keys.
 * (One process plays all roles here; what each role is handed is what its function call takes.)  Build (from the repo root):
 *   gcc -O2 -Iinclude examples/seeded_inputs.c -o examples/seeded_inputs -Lmktfhe_amd/lib -lmktfhe_hip -Wl,-rpath,$PWD/mktfhe_amd/lib
 */
#include <stdio.h>
#include <stdlib.h>

#include "mktfhe.h"

#define CK(call) do { int _r = (call); if (_r < 0) { fprintf(stderr, "%s failed: %d (%s)\n", #call, _r, mkt_last_error(ctx)); return 1; } } while (0)

int main(int argc, char **argv) {
    /* KMS2party (src/tfhe/params.jl:47-53), optionally with a reduced n / N for a quick run */
    mkt_params p = { MKT_KMS, 560, 2048, 2, 64, 3, 12, 2, 7, 3, 10, 8, 2, 0, 0 };
    if (argc > 2) { p.n = atoi(argv[1]); p.N = atoi(argv[2]); }
    const double alpha = 131072.0, beta = 85.4084;
    enum { B = 8 };
    const int len = p.k * p.n + 1;
    mkt_ctx *ctx = NULL, *own = NULL;

    uint64_t *crs = malloc(sizeof(uint64_t) * (size_t)p.l_uni * p.N);
    /* pinned seeds so the keys are reproducible -- a real client passes NULL (fresh OS entropy per call), as the encryptions below do */
    uint8_t seed[32];
    CK(mkt_client_test_seed(1, seed));
    CK(mkt_client_crs(&p, seed, crs));
    mkt_client_party *party[2];
    for (int i = 0; i < 2; i++) CK(mkt_client_party_keygen(&p, seed, i, crs, alpha, beta, &party[i]));

    /* the parties: a fresh PUBLIC mask seed per batch, fresh secret noise (NULL), one body word per bit */
    uint32_t mu[2][B], body[2][B];
    uint8_t mask_seed[2][32];
    int bit[2][B], bad = 0;
    for (int j = 0; j < B; j++) {
        bit[0][j] = j & 1; bit[1][j] = (j >> 1) & 1;
        for (int i = 0; i < 2; i++) mu[i][j] = bit[i][j] ? 1u << 29 : 7u << 29;      /* +-2^29 */
    }
    for (int i = 0; i < 2; i++) CK(mkt_client_random_seed(mask_seed[i]));
    CK(mkt_client_seeded_encrypt(&p, party[0], 0, mu[0], alpha, mask_seed[0], NULL, 0, body[0], B));
    CK(mkt_ctx_create(&p, MKT_ARITH_F64REF, 0, &own));
    int r = mkt_seeded_encrypt_batch(own, 1, party[1], mu[1], alpha, mask_seed[1], NULL, 0, body[1], B, MKT_MEM_HOST);
    if (r < 0) { fprintf(stderr, "mkt_seeded_encrypt_batch failed: %d (%s)\n", r, mkt_last_error(own)); return 1; }
    mkt_ctx_destroy(own);

    /* the evaluator: evaluation keys only; it receives (mask_seed, body) of each party and regenerates the rows where they are used */
    CK(mkt_ctx_create(&p, MKT_ARITH_F64REF, 0, &ctx));
    CK(mkt_load_crs(ctx, crs, MKT_FMT_INT_COEFF));
    for (int i = 0; i < 2; i++) {
        size_t nb;
        CK(mkt_load_brk(ctx, i, mkt_client_brk(party[i], &nb), MKT_FMT_INT_COEFF));
        CK(mkt_load_ksk(ctx, i, mkt_client_ksk(party[i], &nb)));
        CK(mkt_load_rlk(ctx, i, mkt_client_rlk_d(party[i], &nb), mkt_client_rlk_f(party[i], &nb), MKT_FMT_INT_COEFF));
        CK(mkt_load_pubkey(ctx, i, mkt_client_pubkey(party[i], &nb), MKT_FMT_INT_COEFF));
    }
    uint32_t *x = malloc(sizeof(uint32_t) * (size_t)B * len), *y = malloc(sizeof(uint32_t) * (size_t)B * len), *z = malloc(sizeof(uint32_t) * (size_t)B * len);
    CK(mkt_seeded_expand_batch(ctx, 0, mask_seed[0], 0, body[0], x, B, MKT_MEM_HOST));
    CK(mkt_seeded_expand_batch(ctx, 1, mask_seed[1], 0, body[1], y, B, MKT_MEM_HOST));
    CK(mkt_gate_batch(ctx, MKT_NAND, x, y, z, B, MKT_MEM_HOST));

    const mkt_client_party *both[2] = { party[0], party[1] };
    for (int j = 0; j < B; j++) {
        int got = mkt_client_lwe_decrypt(&p, both, 2, z + (size_t)j * len);
        printf("NAND(%d, %d) = %d\n", bit[0][j], bit[1][j], got);
        bad += got != !(bit[0][j] && bit[1][j]);
    }
    mkt_ctx_destroy(ctx);
    for (int i = 0; i < 2; i++) mkt_client_party_destroy(party[i]);
    free(crs); free(x); free(y); free(z);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad != 0;
}
