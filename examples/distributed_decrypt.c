/* Distributed decryption through the C ABI (include/mktfhe.h "distributed decryption"): two-party KMS, one NAND whose inputs were
 * encrypted by different parties, opened by the protocol's roles -- no role is handed more than one secret key:
 *   evaluator   a context loaded with EVALUATION keys only; computes z = NAND(x, y)
 *   party 0     makes its share of z on the host            (mkt_client_partial_decrypt)
 *   party 1     makes its share of z on a GPU context of its own, with no evaluation key loaded   (mkt_partial_decrypt_batch)
 *   merger      holds z and the two shares, no key: adds them up and reads the bit   (mkt_client_merge_decrypt)
 * (One process plays all four roles here; what each role is handed is what its function call takes.)  Build (from the repo root):
 *   gcc -O2 -Iinclude examples/distributed_decrypt.c -o examples/distributed_decrypt -Lmktfhe_amd/lib -lmktfhe_hip -Wl,-rpath,$PWD/mktfhe_amd/lib
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
    /* the smudging deviation is the deployment's choice; 2^20 leaves the margin 2^29 hundreds of deviations away */
    const double sigma_smudge = 1048576.0;
    enum { B = 8 };
    const int len = p.k * p.n + 1;
    mkt_ctx *ctx = NULL, *own = NULL;

    uint64_t *crs = malloc(sizeof(uint64_t) * (size_t)p.l_uni * p.N);
    /* pinned seeds so the keys are reproducible -- a real client passes NULL (fresh OS entropy per call), as the calls below do */
    uint8_t seed[32];
    CK(mkt_client_test_seed(1, seed));
    CK(mkt_client_crs(&p, seed, crs));
    mkt_client_party *party[2];
    for (int i = 0; i < 2; i++) CK(mkt_client_party_keygen(&p, seed, i, crs, alpha, beta, &party[i]));

    /* the evaluator: evaluation keys only */
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
    int bx[B], by[B], bad = 0;
    for (int j = 0; j < B; j++) {
        bx[j] = j & 1; by[j] = (j >> 1) & 1;
        CK(mkt_client_lwe_encrypt(&p, party[0], 0, bx[j], alpha, NULL, x + (size_t)j * len));   /* party 0's bit */
        CK(mkt_client_lwe_encrypt(&p, party[1], 1, by[j], alpha, NULL, y + (size_t)j * len));   /* party 1's bit */
    }
    CK(mkt_gate_batch(ctx, MKT_NAND, x, y, z, B, MKT_MEM_HOST));

    uint32_t shares[2][B];
    /* party 0, on the host: its key, the ciphertexts, fresh smudging noise */
    CK(mkt_client_partial_decrypt(&p, party[0], 0, z, sigma_smudge, NULL, 0, shares[0], B));
    /* party 1, on its own GPU context: no evaluation key is ever loaded into it */
    CK(mkt_ctx_create(&p, MKT_ARITH_F64REF, 0, &own));
    int r = mkt_partial_decrypt_batch(own, 1, party[1], z, sigma_smudge, NULL, 0, shares[1], B, MKT_MEM_HOST);
    if (r < 0) { fprintf(stderr, "mkt_partial_decrypt_batch failed: %d (%s)\n", r, mkt_last_error(own)); return 1; }

    /* the merger: ciphertexts and shares, no key */
    uint8_t bits[B];
    CK(mkt_client_merge_decrypt(&p, z, &shares[0][0], 2, bits, B));
    for (int j = 0; j < B; j++) {
        printf("NAND(%d, %d) = %d\n", bx[j], by[j], bits[j]);
        bad += bits[j] != !(bx[j] && by[j]);
    }
    mkt_ctx_destroy(own);
    mkt_ctx_destroy(ctx);
    for (int i = 0; i < 2; i++) mkt_client_party_destroy(party[i]);
    free(crs); free(x); free(y); free(z);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad != 0;
}
