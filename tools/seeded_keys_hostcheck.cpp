// Stand-alone host check of the seeded-key functions of mktfhe_amd/csrc/client.cpp (no GPU, no Python): generates a seeded party and expands
// it at two reduced shapes (RGSW on the 64-bit ring with two parties; UniEnc; a block scheme with absent rows), and compares the expansion's
// bodies with the compact sections.  Meant to be built with the host sanitizers, from the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Iinclude \
//       tools/seeded_keys_hostcheck.cpp mktfhe_amd/csrc/client.cpp mktfhe_amd/csrc/twiddle.cpp -lpthread -o seeded_keys_hostcheck && ./seeded_keys_hostcheck
#include <cstdio>
#include <cstring>
#include <vector>

#include "mktfhe.h"

static int run(mkt_params p, int party, double beta) {
    const int nparty = (p.scheme >= MKT_CCS) ? p.k : 1, kr = (p.scheme >= MKT_KMS) ? 1 : p.k, word = p.W / 8;
    const int D = 1 << p.logD, dr = (p.scheme == MKT_LMSS || p.scheme == MKT_KMS_BLOCK) ? D / 2 : D - 1, kk = nparty > 1 ? 1 : p.k;
    uint8_t seed[32], mseed[32];
    mkt_client_test_seed(3, seed);
    mkt_client_test_seed(4, mseed);
    std::vector<uint8_t> crs((size_t)(p.l_uni ? p.l_uni : 1) * p.N * word);
    if (nparty > 1 && mkt_client_crs(&p, seed, crs.data())) return 1;
    mkt_client_party *K = nullptr;
    if (mkt_client_party_keygen_seeded(&p, seed, mseed, party, nparty > 1 ? crs.data() : nullptr, 131072.0, beta, &K)) return 2;
    size_t nb = 0, nk = 0;
    const void *bs = mkt_client_brk_seeded(K, &nb);
    const uint32_t *ks = mkt_client_ksk_seeded(K, &nk);
    const size_t polys = p.scheme == MKT_CCS ? (size_t)3 * p.l_uni : (size_t)(kr + 1) * p.l_gsw * (kr + 1);
    const size_t rows = (size_t)kk * p.N * dr * p.f;
    if (nk != rows * 4 || std::memcmp(mkt_client_mask_seed(K), mseed, 32)) return 3;
    std::vector<uint8_t> brk((size_t)p.n * polys * p.N * word);
    std::vector<uint32_t> ksk(rows * (size_t)(p.n + 1));
    if (mkt_client_seeded_keys_expand(&p, party, mseed, bs, ks, brk.data(), ksk.data())) return 4;
    if (mkt_client_seeded_keys_expand(&p, party, mseed, nullptr, ks, nullptr, ksk.data())) return 5;
    if (mkt_client_seeded_keys_expand(&p, party, mseed, bs, nullptr, brk.data(), nullptr)) return 6;
    for (size_t R = 0; R < rows; R++) if (ksk[R * (p.n + 1) + p.n] != ks[R]) return 7;
    if (p.scheme != MKT_CCS && std::memcmp(brk.data(), bs, (size_t)p.N * word)) return 8;    // the first b polynomial
    mkt_client_party_destroy(K);
    std::printf("scheme %d n %d N %d W %d: %zu + %zu compact bytes -> %zu + %zu\n", p.scheme, p.n, p.N, p.W, nb, nk, brk.size(), ksk.size() * 4);
    return 0;
}

int main() {
    const mkt_params kms = { MKT_KMS, 17, 32, 2, 64, 3, 12, 2, 7, 3, 10, 8, 2, 0, 0 };
    const mkt_params ccs = { MKT_CCS, 16, 64, 2, 32, 0, 0, 0, 0, 3, 8, 8, 2, 0, 0 };
    const mkt_params lmss = { MKT_LMSS, 150, 64, 3, 32, 3, 9, 0, 0, 0, 0, 8, 2, 3, 50 };
    int r;
    if ((r = run(kms, 1, 85.4084)) || (r = run(ccs, 1, 16.0)) || (r = run(lmss, 0, 128.0))) { std::printf("FAILED at step %d\n", r); return 1; }
    std::printf("ok\n");
    return 0;
}
