/* Seeded evaluation keys generated on the party's own GPU, through the C ABI (include/mktfhe.h "seeded evaluation keys"): two-party KMS, NAND.
 *   each party   holds its secrets and small keys only (mkt_client_party_secrets), draws a fresh PUBLIC mask seed and has its OWN GPU -- a
 *                context of its own that never holds an evaluation key -- write the compact sections (mkt_keygen_device_seeded, install = 0):
 *                the words the host generator mkt_client_party_keygen_seeded makes, in a fraction of its time, the large keys never expanded
 *   evaluator    a second context: loads (mask seed, compact sections) and regenerates the masks on its GPU (mkt_load_seeded_keys); the small
 *                keys (relinearisation key, public key) are loaded as ever.  It never sees a secret.
 * (One process plays all roles here; what each role is handed is what its function call takes.)  Build (from the repo root):
 *   gcc -O2 -Iinclude examples/seeded_keygen_gpu.c -o examples/seeded_keygen_gpu -Lmktfhe_amd/lib -lmktfhe_hip -Wl,-rpath,$PWD/mktfhe_amd/lib
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mktfhe.h"

#define CK(call) do { int _r = (call); if (_r < 0) { fprintf(stderr, "%s failed: %d (%s)\n", #call, _r, mkt_last_error(ctx)); return 1; } } while (0)

int main(int argc, char **argv) {
    /* KMS2party (src/tfhe/params.jl:47-53), optionally with a reduced n / N for a quick run */
    mkt_params p = { MKT_KMS, 560, 2048, 2, 64, 3, 12, 2, 7, 3, 10, 8, 2, 0, 0 };
    if (argc > 2) { p.n = atoi(argv[1]); p.N = atoi(argv[2]); }
    const double alpha = 131072.0, beta = 85.4084;
    enum { B = 4 };
    const int len = p.k * p.n + 1;
    /* the compact layouts of the header: brk_seeded [n][2 l_gsw][N] 64-bit ring words, ksk_seeded [N][D - 1][f] words */
    const size_t nbrk = sizeof(uint64_t) * (size_t)p.n * 2 * p.l_gsw * p.N, nksk = sizeof(uint32_t) * (size_t)p.N * ((1u << p.logD) - 1) * p.f;
    mkt_ctx *ctx = NULL;

    uint64_t *crs = malloc(sizeof(uint64_t) * (size_t)p.l_uni * p.N);
    /* pinned secret seeds so the run is reproducible -- a real client passes NULL (fresh OS entropy per call) */
    uint8_t seed[32], mask_seed[2][32];
    CK(mkt_client_test_seed(1, seed));
    CK(mkt_client_crs(&p, seed, crs));

    /* the parties, each on its own GPU context: secrets in, (fresh public mask seed, compact sections) out; nothing is installed */
    mkt_client_party *party[2];
    void *brk[2];
    uint32_t *ksk[2];
    for (int i = 0; i < 2; i++) {
        CK(mkt_client_party_secrets(&p, seed, i, crs, alpha, beta, &party[i]));
        CK(mkt_client_random_seed(mask_seed[i]));
        brk[i] = malloc(nbrk); ksk[i] = malloc(nksk);
        CK(mkt_ctx_create(&p, MKT_ARITH_F64REF, 0, &ctx));
        CK(mkt_keygen_device_seeded(ctx, i, party[i], NULL, mask_seed[i], brk[i], ksk[i], 0));
        mkt_ctx_destroy(ctx); ctx = NULL;
        printf("party %d: %zu bytes of compact keys made on its GPU (full keys: %zu)\n", i, 32 + nbrk + nksk, 2 * nbrk + nksk * (size_t)(p.n + 1));
    }

    /* the evaluator: a second context; the masks are regenerated on its GPU */
    CK(mkt_ctx_create(&p, MKT_ARITH_F64REF, 0, &ctx));
    CK(mkt_load_crs(ctx, crs, MKT_FMT_INT_COEFF));
    for (int i = 0; i < 2; i++) {
        size_t nb;
        CK(mkt_load_seeded_keys(ctx, i, mask_seed[i], brk[i], ksk[i]));
        CK(mkt_load_rlk(ctx, i, mkt_client_rlk_d(party[i], &nb), mkt_client_rlk_f(party[i], &nb), MKT_FMT_INT_COEFF));
        CK(mkt_load_pubkey(ctx, i, mkt_client_pubkey(party[i], &nb), MKT_FMT_INT_COEFF));
    }

    uint32_t *x = malloc(sizeof(uint32_t) * (size_t)B * len), *y = malloc(sizeof(uint32_t) * (size_t)B * len), *z = malloc(sizeof(uint32_t) * (size_t)B * len);
    int bad = 0;
    for (int j = 0; j < B; j++) {
        CK(mkt_client_lwe_encrypt(&p, party[0], 0, j & 1, alpha, NULL, x + (size_t)j * len));
        CK(mkt_client_lwe_encrypt(&p, party[1], 1, (j >> 1) & 1, alpha, NULL, y + (size_t)j * len));
    }
    CK(mkt_gate_batch(ctx, MKT_NAND, x, y, z, B, MKT_MEM_HOST));
    const mkt_client_party *both[2] = { party[0], party[1] };
    for (int j = 0; j < B; j++) {
        int got = mkt_client_lwe_decrypt(&p, both, 2, z + (size_t)j * len);
        printf("NAND(%d, %d) = %d\n", j & 1, (j >> 1) & 1, got);
        bad += got != !((j & 1) && ((j >> 1) & 1));
    }
    mkt_ctx_destroy(ctx);
    for (int i = 0; i < 2; i++) { mkt_client_party_destroy(party[i]); free(brk[i]); free(ksk[i]); }
    free(crs); free(x); free(y); free(z);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad != 0;
}
