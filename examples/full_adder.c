/* A multi-party full adder from plain C (include/mktfhe.h only): sum = XOR3(a, b, c) and carry = MAJ3(a, b, c), each ONE gate
 * bootstrap (mkt_gate3_batch_ops), for all eight input combinations in one call of 16 gates; a, b and c are encrypted under three
 * different parties and the results are decrypted with all parties' keys (mkt_client_*).  The composite of the two-input gates
 * (XOR, XOR, AND, AND, OR) takes five bootstraps per adder.
 *   gcc -O2 -Iinclude examples/full_adder.c -o examples/full_adder -Lmktfhe_amd/lib -lmktfhe_hip -Wl,-rpath,$PWD/mktfhe_amd/lib
 *   examples/full_adder [<n> <N>]      KMS4party (src/tfhe/params.jl:55-61), optionally with a reduced n and N
 */
#include <stdio.h>
#include <stdlib.h>

#include "mktfhe.h"

#define CK(call) do { int _r = (call); if (_r < 0) { fprintf(stderr, "%s failed: %d (%s)\n", #call, _r, mkt_last_error(ctx)); return 1; } } while (0)
#define K 4

int main(int argc, char **argv) {
    mkt_params p = { MKT_KMS, 560, 2048, K, 64, 5, 8, 2, 8, 7, 6, 8, 2, 0, 0 };        /* KMS4party */
    if (argc > 2) { p.n = atoi(argv[1]); p.N = atoi(argv[2]); }
    const double alpha = 131072.0, beta = 85.4084;
    const int B = 8, len = p.k * p.n + 1;                                              /* 8 adders: 8 sums, then 8 carries */
    mkt_ctx *ctx = NULL;

    uint8_t seed[32];
    uint64_t *crs = malloc(sizeof(uint64_t) * (size_t)p.l_uni * p.N);
    CK(mkt_client_test_seed(7, seed));                                                 /* pinned: reproducible example, NOT for real keys */
    CK(mkt_client_crs(&p, seed, crs));
    mkt_client_party *party[K];
    for (int i = 0; i < K; i++) CK(mkt_client_party_keygen(&p, seed, i, crs, alpha, beta, &party[i]));

    CK(mkt_ctx_create(&p, MKT_ARITH_F64REF, 0, &ctx));
    CK(mkt_load_crs(ctx, crs, MKT_FMT_INT_COEFF));
    for (int i = 0; i < K; i++) {
        size_t nb;
        CK(mkt_load_brk(ctx, i, mkt_client_brk(party[i], &nb), MKT_FMT_INT_COEFF));
        CK(mkt_load_ksk(ctx, i, mkt_client_ksk(party[i], &nb)));
        CK(mkt_load_rlk(ctx, i, mkt_client_rlk_d(party[i], &nb), mkt_client_rlk_f(party[i], &nb), MKT_FMT_INT_COEFF));
        CK(mkt_load_pubkey(ctx, i, mkt_client_pubkey(party[i], &nb), MKT_FMT_INT_COEFF));
    }

    /* rows 0..7 and 8..15 see the same operands: row j + 8 computes the carry of adder j */
    const size_t bytes = 4 * (size_t)2 * B * len;
    uint32_t *x = malloc(bytes), *y = malloc(bytes), *z = malloc(bytes), *out = malloc(bytes);
    uint8_t ops[2 * B];
    for (int j = 0; j < B; j++) {
        const int a = j & 1, b = (j >> 1) & 1, c = (j >> 2) & 1;
        CK(mkt_client_lwe_encrypt(&p, party[0], 0, a, alpha, NULL, x + (size_t)j * len));
        CK(mkt_client_lwe_encrypt(&p, party[1], 1, b, alpha, NULL, y + (size_t)j * len));
        CK(mkt_client_lwe_encrypt(&p, party[2], 2, c, alpha, NULL, z + (size_t)j * len));
        for (int w = 0; w < len; w++) {
            x[(size_t)(j + B) * len + w] = x[(size_t)j * len + w];
            y[(size_t)(j + B) * len + w] = y[(size_t)j * len + w];
            z[(size_t)(j + B) * len + w] = z[(size_t)j * len + w];
        }
        ops[j] = MKT_XOR3;
        ops[j + B] = MKT_MAJ3;
    }
    CK(mkt_gate3_batch_ops(ctx, ops, x, y, z, out, 2 * B, MKT_MEM_HOST));
    int bad = 0;
    for (int j = 0; j < B; j++) {
        const int a = j & 1, b = (j >> 1) & 1, c = (j >> 2) & 1;
        const int s = mkt_client_lwe_decrypt(&p, (const mkt_client_party *const *)party, K, out + (size_t)j * len);
        const int cy = mkt_client_lwe_decrypt(&p, (const mkt_client_party *const *)party, K, out + (size_t)(j + B) * len);
        bad += s != (a ^ b ^ c);
        bad += cy != (a + b + c >= 2);
        printf("%d + %d + %d = carry %d, sum %d\n", a, b, c, cy, s);
    }
    mkt_ctx_destroy(ctx);
    for (int i = 0; i < K; i++) mkt_client_party_destroy(party[i]);
    free(crs); free(x); free(y); free(z); free(out);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad != 0;
}
