// The Gaussian deviate of rng_chacha.h laid bare for tests/test_rng_cpu.py: what box_muller returns, bit for bit, on inputs the caller
// names, and what a changed deviate does to the noise word at a given sigma.
//   gauss_check pairs           reads "r1 r2" (hex) lines from stdin; prints "r1 r2 bits(box_muller(r1, r2))" (hex) per line
//   gauss_check draws K         the same lines for K pairs drawn from one stream
//   gauss_check stream N sigma  binary to stdout: N x uint64 bits of Rng::gauss(), then N x uint64 Rng::noise(sigma) of the same draws
// sigma is read with strtod, so a hexadecimal float (0x1p55) names it exactly.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rng_chacha.h"

static void line(uint64_t r1, uint64_t r2) {
    printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", r1, r2, mktrng::double_to_bits(mktrng::box_muller(r1, r2)));
}

int main(int argc, char **argv) {
    uint32_t key[8];
    for (int i = 0; i < 8; i++) key[i] = 0x9E3779B9u * (uint32_t)(i + 1);
    if (argc == 2 && !strcmp(argv[1], "pairs")) {
        uint64_t r1, r2;
        while (scanf("%" SCNx64 " %" SCNx64, &r1, &r2) == 2) line(r1, r2);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "draws")) {
        mktrng::Rng r(key, 0, 3);
        for (long i = 0, K = atol(argv[2]); i < K; i++) { const uint64_t r1 = r.next(), r2 = r.next(); line(r1, r2); }
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "stream")) {
        const size_t N = (size_t)atol(argv[2]);
        const double sigma = strtod(argv[3], nullptr);
        std::vector<uint64_t> out(2 * N);
        mktrng::Rng g(key, 0, 4), w(key, 0, 4);                // two readers of one stream
        for (size_t i = 0; i < N; i++) { out[i] = mktrng::double_to_bits(g.gauss()); out[N + i] = w.noise(sigma); }
        return fwrite(out.data(), 8, 2 * N, stdout) == 2 * N ? 0 : 1;
    }
    fprintf(stderr, "usage: gauss_check pairs | draws K | stream N sigma\n");
    return 2;
}
