/* Ring shares on the party's own GPU through the C ABI (include/mktfhe_ring_share.h): two-party KMS, a batch of NANDs packed into one RLWE
 * ciphertext by the evaluator, opened by one ring share per party that the party makes on ITS OWN context:
 *   party i     generates its evaluation keys and its packing key                  (mkt_client_packing_keygen)
 *   evaluator   loads evaluation keys only, computes z = NAND(x, y), packs z       (mkt_load_packing_key, mkt_pack_batch)
 *   party i     a context of its own, no key loaded: its ring share on its GPU     (mkt_ctx_create, mkt_rlwe_partial_decrypt_batch)
 *   merger      holds the packed ciphertext and the shares, no key: reads the bits (mkt_client_rlwe_merge_decrypt)
 * (One process and one GPU play all roles here; what each role is handed is what its function call takes.)  Build (from the repo root):
 *   gcc -O2 -Iinclude examples/ring_share_gpu.c -o examples/ring_share_gpu -Lmktfhe_amd/lib -lmktfhe_hip -Wl,-rpath,$PWD/mktfhe_amd/lib
 */
#include <stdio.h>
#include <stdlib.h>

#include "mktfhe_ring_share.h"

#define CK(call) do { int _r = (call); if (_r < 0) { fprintf(stderr, "%s failed: %d (%s)\n", #call, _r, mkt_last_error(ctx)); return 1; } } while (0)

int main(int argc, char **argv) {
    /* KMS2party (src/tfhe/params.jl:47-53), optionally with a reduced n / N for a quick run */
    mkt_params p = { MKT_KMS, 560, 2048, 2, 64, 3, 12, 2, 7, 3, 10, 8, 2, 0, 0 };
    if (argc > 2) { p.n = atoi(argv[1]); p.N = atoi(argv[2]); }
    const double alpha = 131072.0, beta = 85.4084, sigma_smudge = 1048576.0;   /* smudging: the deployment's choice */
    const int l_pk = 4, logB_pk = 4;
    enum { B = 40 };
    const int len = p.k * p.n + 1;
    const size_t N = (size_t)p.N;
    mkt_ctx *ctx = NULL;

    uint64_t *crs = malloc(sizeof(uint64_t) * (size_t)p.l_uni * N);
    uint8_t seed[32];   /* pinned so the keys are reproducible -- a real client passes NULL (fresh OS entropy per call), as the calls below do */
    CK(mkt_client_test_seed(1, seed));
    CK(mkt_client_crs(&p, seed, crs));
    mkt_client_party *party[2];
    uint64_t *pk[2];
    for (int i = 0; i < 2; i++) {
        CK(mkt_client_party_keygen(&p, seed, i, crs, alpha, beta, &party[i]));
        pk[i] = malloc(sizeof(uint64_t) * (size_t)p.n * l_pk * 2 * N);        /* [n][l_pk][1 + kr][N], kr = 1 */
        CK(mkt_client_packing_keygen(&p, party[i], i, l_pk, logB_pk, NULL, pk[i]));
    }

    /* the evaluator: evaluation keys only, the packing keys among them */
    CK(mkt_ctx_create(&p, MKT_ARITH_F64REF, 0, &ctx));
    CK(mkt_load_crs(ctx, crs, MKT_FMT_INT_COEFF));
    for (int i = 0; i < 2; i++) {
        size_t nb;
        CK(mkt_load_brk(ctx, i, mkt_client_brk(party[i], &nb), MKT_FMT_INT_COEFF));
        CK(mkt_load_ksk(ctx, i, mkt_client_ksk(party[i], &nb)));
        CK(mkt_load_rlk(ctx, i, mkt_client_rlk_d(party[i], &nb), mkt_client_rlk_f(party[i], &nb), MKT_FMT_INT_COEFF));
        CK(mkt_load_pubkey(ctx, i, mkt_client_pubkey(party[i], &nb), MKT_FMT_INT_COEFF));
        CK(mkt_load_packing_key(ctx, i, pk[i], l_pk, logB_pk));
    }
    uint32_t *x = malloc(sizeof(uint32_t) * (size_t)B * len), *y = malloc(sizeof(uint32_t) * (size_t)B * len), *z = malloc(sizeof(uint32_t) * (size_t)B * len);
    int bx[B], by[B], bad = 0;
    for (int j = 0; j < B; j++) {
        bx[j] = j & 1; by[j] = (j >> 1) & 1;
        CK(mkt_client_lwe_encrypt(&p, party[0], 0, bx[j], alpha, NULL, x + (size_t)j * len));   /* party 0's bit */
        CK(mkt_client_lwe_encrypt(&p, party[1], 1, by[j], alpha, NULL, y + (size_t)j * len));   /* party 1's bit */
    }
    CK(mkt_gate_batch(ctx, MKT_NAND, x, y, z, B, MKT_MEM_HOST));
    uint64_t *packed = malloc(sizeof(uint64_t) * 3 * N);                      /* [1 + k][N]: what leaves the evaluator */
    CK(mkt_pack_batch(ctx, z, B, NULL, B, packed, MKT_MEM_HOST));
    mkt_ctx_destroy(ctx);
    ctx = NULL;

    /* every party, alone, on a context that holds no key: its ring share of the one packed ciphertext, blurred by fresh smudging noise */
    uint64_t *shares = malloc(sizeof(uint64_t) * 2 * N);
    for (int i = 0; i < 2; i++) {
        CK(mkt_ctx_create(&p, MKT_ARITH_F64REF, 0, &ctx));
        CK(mkt_rlwe_partial_decrypt_batch(ctx, i, party[i], packed, sigma_smudge, NULL, 0, shares + (size_t)i * N, 1, MKT_MEM_HOST));
        mkt_ctx_destroy(ctx);
        ctx = NULL;
    }

    /* the merger: the packed ciphertext and the shares, no key; coefficient j is result j */
    uint8_t bits[B];
    CK(mkt_client_rlwe_merge_decrypt(&p, packed, shares, 2, B, bits));
    for (int j = 0; j < B; j++) bad += bits[j] != !(bx[j] && by[j]);
    for (int j = 0; j < 4; j++) printf("NAND(%d, %d) = %d\n", bx[j], by[j], bits[j]);
    for (int i = 0; i < 2; i++) { mkt_client_party_destroy(party[i]); free(pk[i]); }
    free(crs); free(x); free(y); free(z); free(packed); free(shares);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad != 0;
}
