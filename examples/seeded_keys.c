/* Seeded evaluation keys through the C ABI (include/mktfhe.h "seeded evaluation keys"): two-party KMS, NAND under keys that travel as a public
 * mask seed and their bodies instead of in full:
 *   each party   generates its keys in the seeded form with a fresh PUBLIC mask seed and writes the compact sections to a file
 *                (mkt_client_party_keygen_seeded, mkt_client_mask_seed, mkt_client_brk_seeded, mkt_client_ksk_seeded)
 *   evaluator    reads the files and loads them; its GPU regenerates the masks where the resident tables live -- the expanded keys never exist
 *                on a host (mkt_load_seeded_keys); the small keys (relinearisation key, public key) are loaded as ever
 * The files hold 32 + 8 n 2 l_gsw N + 4 N (D - 1) f bytes per party where the full keys hold 8 n 2 l_gsw 2 N + 4 N (D - 1) f (n + 1).
 * (One process plays all roles here; what each role is handed is what its function call takes.)  Build (from the repo root):
 *   gcc -O2 -Iinclude examples/seeded_keys.c -o examples/seeded_keys -Lmktfhe_amd/lib -lmktfhe_hip -Wl,-rpath,$PWD/mktfhe_amd/lib
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mktfhe.h"

#define CK(call) do { int _r = (call); if (_r < 0) { fprintf(stderr, "%s failed: %d (%s)\n", #call, _r, mkt_last_error(ctx)); return 1; } } while (0)

int main(int argc, char **argv) {
    /* KMS2party (src/tfhe/params.jl:47-53), optionally with a reduced n / N for a quick run; argv[3] = directory for the key files */
    mkt_params p = { MKT_KMS, 560, 2048, 2, 64, 3, 12, 2, 7, 3, 10, 8, 2, 0, 0 };
    if (argc > 2) { p.n = atoi(argv[1]); p.N = atoi(argv[2]); }
    const char *dir = argc > 3 ? argv[3] : ".";
    const double alpha = 131072.0, beta = 85.4084;
    enum { B = 4 };
    const int len = p.k * p.n + 1;
    mkt_ctx *ctx = NULL;

    uint64_t *crs = malloc(sizeof(uint64_t) * (size_t)p.l_uni * p.N);
    /* pinned secret seeds so the run is reproducible -- a real client passes NULL (fresh OS entropy per call) */
    uint8_t seed[32], mask_seed[32];
    CK(mkt_client_test_seed(1, seed));
    CK(mkt_client_crs(&p, seed, crs));

    /* the parties: a fresh PUBLIC mask seed per key generation; the compact sections go to a file */
    mkt_client_party *party[2];
    char path[2][512];
    size_t nbrk = 0, nksk = 0;
    for (int i = 0; i < 2; i++) {
        CK(mkt_client_random_seed(mask_seed));
        CK(mkt_client_party_keygen_seeded(&p, seed, mask_seed, i, crs, alpha, beta, &party[i]));
        const void *brk = mkt_client_brk_seeded(party[i], &nbrk);
        const uint32_t *ksk = mkt_client_ksk_seeded(party[i], &nksk);
        snprintf(path[i], sizeof path[i], "%s/party%d.seeded_keys", dir, i);
        FILE *f = fopen(path[i], "wb");
        if (!f || fwrite(mkt_client_mask_seed(party[i]), 1, 32, f) != 32 || fwrite(brk, 1, nbrk, f) != nbrk || fwrite(ksk, 1, nksk, f) != nksk || fclose(f)) {
            fprintf(stderr, "cannot write %s\n", path[i]);
            return 1;
        }
        printf("party %d: %zu bytes of compact keys (full keys: %zu)\n", i, 32 + nbrk + nksk, 2 * nbrk + nksk * (size_t)(p.n + 1));
    }

    /* the evaluator: reads (mask seed, bodies) and loads them; the masks are regenerated on its GPU */
    CK(mkt_ctx_create(&p, MKT_ARITH_F64REF, 0, &ctx));
    CK(mkt_load_crs(ctx, crs, MKT_FMT_INT_COEFF));
    unsigned char *buf = malloc(32 + nbrk + nksk);
    for (int i = 0; i < 2; i++) {
        size_t nb;
        FILE *f = fopen(path[i], "rb");
        if (!f || fread(buf, 1, 32 + nbrk + nksk, f) != 32 + nbrk + nksk) { fprintf(stderr, "cannot read %s\n", path[i]); return 1; }
        fclose(f);
        remove(path[i]);
        CK(mkt_load_seeded_keys(ctx, i, buf, buf + 32, (const uint32_t *)(buf + 32 + nbrk)));
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
    for (int i = 0; i < 2; i++) mkt_client_party_destroy(party[i]);
    free(crs); free(buf); free(x); free(y); free(z);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad != 0;
}
