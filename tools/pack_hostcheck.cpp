// Stand-alone host check of the packed-output functions of mktfhe_amd/csrc/client.cpp (no GPU, no Python): generates packing keys at reduced
// shapes (KMS on the 64-bit ring with two parties; CCS; CGGI with RLWE length 2), builds a packed ciphertext of known phase by hand from the
// key rows (coefficient 0 of row (q, t) carries s[q] g_t), opens it with the all-keys harness, by ring shares with and without smudging noise
// and by the merge, and runs the refusals.  Then the evaluation keys: one full and one seeded generation and the expansion of the seeded
// sections, so that every shared step of the generators runs under the sanitizers.  Meant to be built with them, from the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Iinclude \
//       tools/pack_hostcheck.cpp mktfhe_amd/csrc/client.cpp mktfhe_amd/csrc/twiddle.cpp -lpthread -o pack_hostcheck && ./pack_hostcheck
#include <cstdio>
#include <cstring>
#include <vector>

#include "mktfhe_pack.h"

static int run(mkt_params p, int l, int logB, double beta) {
    const int nparty = (p.scheme >= MKT_CCS) ? p.k : 1, kr = nparty > 1 ? 1 : p.k, word = p.W / 8, N = p.N;
    uint8_t seed[32];
    mkt_client_test_seed(3, seed);
    std::vector<uint8_t> crs((size_t)(p.l_uni ? p.l_uni : 1) * N * word);
    if (nparty > 1 && mkt_client_crs(&p, seed, crs.data())) return 1;
    std::vector<mkt_client_party *> K((size_t)nparty, nullptr);
    std::vector<std::vector<uint8_t>> pk((size_t)nparty);
    for (int i = 0; i < nparty; i++) {
        if (mkt_client_party_secrets(&p, seed, i, nparty > 1 ? crs.data() : nullptr, 131072.0, beta, &K[i])) return 2;
        pk[i].assign((size_t)p.n * l * (kr + 1) * N * word, 0);
        if (mkt_client_packing_keygen(&p, K[i], i, l, logB, i ? nullptr : seed, pk[i].data())) return 3;
        if (mkt_client_packing_keygen(&p, K[i], (i + 1) % (nparty > 1 ? nparty : 2), l, logB, seed, pk[i].data()) != MKT_ERR_ARG) return 4;
    }
    if (mkt_client_packing_keygen(&p, K[0], 0, 3, 11, seed, pk[0].data()) != MKT_ERR_ARG) return 5;
    // a ciphertext made of key row (q = 0, t = 0) of party 0: polynomial 0 = its b, the party's slot(s) = its a_c, every other slot zero
    std::vector<uint8_t> ct((size_t)(1 + p.k) * N * word, 0);
    std::memcpy(ct.data(), pk[0].data(), (size_t)N * word);
    for (int c = 0; c < kr; c++) std::memcpy(ct.data() + (size_t)(1 + c) * N * word, pk[0].data() + (size_t)(1 + c) * N * word, (size_t)N * word);
    std::vector<uint32_t> ph((size_t)N), merged((size_t)N);
    if (mkt_client_rlwe_phase(&p, K.data(), nparty, ct.data(), ph.data())) return 6;
    const uint32_t want0 = mkt_client_lwekey(K[0])[0] << (32 - logB);        // s[0] g_0 on the 32-bit torus, plus noise
    if ((uint32_t)(ph[0] - want0 + (1u << 20)) > (2u << 20)) return 7;
    for (int j = 1; j < N; j++) if ((uint32_t)(ph[(size_t)j] + (1u << 20)) > (2u << 20)) return 8;
    std::vector<uint8_t> shares((size_t)nparty * N * word), noisy((size_t)N * word);
    for (int i = 0; i < nparty; i++)
        if (mkt_client_rlwe_partial_decrypt(&p, K[i], i, ct.data(), 0.0, nullptr, 0, shares.data() + (size_t)i * N * word, 1)) return 9;
    if (mkt_client_rlwe_merge_phase(&p, ct.data(), shares.data(), nparty, (size_t)N, merged.data())) return 10;
    if (std::memcmp(merged.data(), ph.data(), (size_t)N * 4)) return 11;                           // sigma_smudge = 0: word for word
    if (mkt_client_rlwe_partial_decrypt(&p, K[0], 0, ct.data(), 2147483648.0, seed, ~0ull, noisy.data(), 1)) return 12;
    if (!std::memcmp(noisy.data(), shares.data(), (size_t)N * word)) return 13;
    std::vector<uint8_t> bits((size_t)N);
    if (mkt_client_rlwe_merge_decrypt(&p, ct.data(), shares.data(), nparty, (size_t)N, bits.data())) return 14;
    if (mkt_client_rlwe_merge_decrypt(&p, ct.data(), shares.data(), nparty, (size_t)N + 1, bits.data()) != MKT_ERR_ARG) return 15;
    if (mkt_client_rlwe_merge_phase(&p, ct.data(), shares.data(), nparty + 1, 1, merged.data()) != MKT_ERR_ARG) return 16;
    if (mkt_client_rlwe_partial_decrypt(&p, K[0], 0, ct.data(), -1.0, seed, 0, noisy.data(), 1) != MKT_ERR_ARG) return 17;
    if (mkt_client_rlwe_partial_decrypt(&p, K[0], 0, nullptr, 0.0, seed, 0, nullptr, 0)) return 18;
    // the seeded form (mktfhe_pack.h "SEEDED"): bodies, then the expansion; row (0, 0) of the expanded key opens like a row of the full one
    uint8_t mseed[32];
    mkt_client_test_seed(4, mseed);
    std::vector<uint8_t> body((size_t)p.n * l * N * word, 0xA5), full((size_t)p.n * l * (kr + 1) * N * word, 0x5A), was = body;
    if (mkt_client_packing_keygen_seeded(&p, K[0], 0, l, logB, seed, nullptr, body.data()) != MKT_ERR_ARG) return 19;
    if (mkt_client_packing_keygen_seeded(&p, K[0], 0, l, logB, mseed, mseed, body.data()) != MKT_ERR_ARG) return 20;
    if (mkt_client_packing_keygen_seeded(&p, K[0], nparty > 1 ? 1 : 2, l, logB, seed, mseed, body.data()) != MKT_ERR_ARG) return 21;
    if (mkt_client_packing_keygen_seeded(&p, K[0], 0, 3, 11, seed, mseed, body.data()) != MKT_ERR_ARG || body != was) return 22;
    if (mkt_client_packing_keygen_seeded(&p, K[0], 0, l, logB, nullptr, mseed, body.data())) return 23;
    if (mkt_client_packing_key_expand(&p, 0, l, logB, nullptr, body.data(), full.data()) != MKT_ERR_ARG) return 24;
    if (mkt_client_packing_key_expand(&p, nparty, l, logB, mseed, body.data(), full.data()) != MKT_ERR_ARG) return 25;
    if (mkt_client_packing_key_expand(&p, 0, l, logB, mseed, body.data(), full.data())) return 26;
    if (std::memcmp(full.data(), body.data(), (size_t)N * word)) return 27;                        // polynomial 0 of row (0, 0) is its body
    std::memcpy(ct.data(), full.data(), (size_t)(1 + kr) * N * word);
    if (nparty > 1) std::memset(ct.data() + (size_t)2 * N * word, 0, (size_t)(p.k - 1) * N * word);
    if (mkt_client_rlwe_phase(&p, K.data(), nparty, ct.data(), ph.data())) return 28;
    if ((uint32_t)(ph[0] - want0 + (1u << 20)) > (2u << 20)) return 29;
    for (int j = 1; j < N; j++) if ((uint32_t)(ph[(size_t)j] + (1u << 20)) > (2u << 20)) return 30;
    for (auto *k : K) mkt_client_party_destroy(k);
    std::printf("scheme %d n %d N %d W %d gadget (%d, %d): %zu key bytes per party\n", p.scheme, p.n, N, p.W, l, logB, pk[0].size());
    return 0;
}

// one party's evaluation keys in both forms, and the seeded sections expanded: the expansion carries the bodies where the layout puts them
static int keys(mkt_params p) {
    const int nparty = (p.scheme >= MKT_CCS) ? p.k : 1, word = p.W / 8, N = p.N;
    uint8_t seed[32], mseed[32];
    mkt_client_test_seed(5, seed);
    mkt_client_test_seed(6, mseed);
    std::vector<uint8_t> crs((size_t)(p.l_uni ? p.l_uni : 1) * N * word);
    if (nparty > 1 && mkt_client_crs(&p, seed, crs.data())) return 40;
    const void *a = nparty > 1 ? crs.data() : nullptr;
    mkt_client_party *F = nullptr, *S = nullptr;
    if (mkt_client_party_keygen(&p, seed, nparty - 1, a, 131072.0, 16.0, &F)) return 41;
    if (mkt_client_party_keygen_seeded(&p, seed, seed, nparty - 1, a, 131072.0, 16.0, &S) != MKT_ERR_ARG || S) return 42;
    if (mkt_client_party_keygen_seeded(&p, seed, mseed, nparty - 1, a, 131072.0, 16.0, &S)) return 43;
    size_t brk_bytes = 0, ksk_bytes = 0, sb = 0, sk = 0;
    mkt_client_brk(F, &brk_bytes);
    mkt_client_ksk(F, &ksk_bytes);
    const uint8_t *bodies = (const uint8_t *)mkt_client_brk_seeded(S, &sb);
    const uint32_t *words = mkt_client_ksk_seeded(S, &sk);
    if (!brk_bytes || !ksk_bytes || !sb || !sk || sb >= brk_bytes || sk >= ksk_bytes) return 44;
    std::vector<uint8_t> brk(brk_bytes, 0x5A);
    std::vector<uint32_t> ksk(ksk_bytes / 4, 0x5A5A5A5Au);
    if (mkt_client_seeded_keys_expand(&p, nparty, mseed, bodies, words, brk.data(), ksk.data()) != MKT_ERR_ARG) return 45;
    if (mkt_client_seeded_keys_expand(&p, nparty - 1, mseed, bodies, words, brk.data(), ksk.data())) return 46;
    if (std::memcmp(brk.data(), bodies, (size_t)N * word)) return 47;                              // polynomial 0 is the first body in both forms
    const size_t rows = sk / 4, n1 = (size_t)p.n + 1;
    if (rows * n1 * 4 != ksk_bytes) return 48;
    for (size_t R = 0; R < rows; R++) if (ksk[R * n1 + (size_t)p.n] != words[R]) return 49;         // the last word of a row is its body (0 where absent)
    mkt_client_party_destroy(F);
    mkt_client_party_destroy(S);
    std::printf("scheme %d n %d N %d W %d: %zu + %zu key bytes, %zu + %zu seeded\n", p.scheme, p.n, N, p.W, brk_bytes, ksk_bytes, sb, sk);
    return 0;
}

int main() {
    const mkt_params kms = { MKT_KMS, 5, 32, 2, 64, 3, 12, 2, 7, 3, 10, 8, 2, 0, 0 };
    const mkt_params ccs = { MKT_CCS, 4, 64, 3, 32, 0, 0, 0, 0, 3, 8, 8, 2, 0, 0 };
    const mkt_params cggi = { MKT_CGGI, 3, 32, 2, 32, 3, 9, 0, 0, 0, 0, 8, 2, 0, 0 };
    const mkt_params ccs32 = { MKT_CCS, 3, 32, 2, 32, 0, 0, 0, 0, 3, 8, 8, 2, 0, 0 };
    const mkt_params kmsblk = { MKT_KMS_BLOCK, 6, 32, 2, 64, 3, 12, 2, 7, 3, 10, 8, 2, 3, 2 };
    int r;
    if ((r = run(kms, 4, 4, 85.4084)) || (r = run(ccs, 3, 5, 16.0)) || (r = run(cggi, 8, 4, 128.0)) || (r = run(kms, 1, 16, 85.4084)) ||
        (r = run(ccs32, 4, 4, 16.0)) || (r = run(kmsblk, 3, 5, 85.4084)) || (r = keys(cggi)) || (r = keys(ccs32)) || (r = keys(kmsblk))) { std::printf("FAILED at step %d\n", r); return 1; }
    std::printf("ok\n");
    return 0;
}
