"""Client-side randomness (mktfhe_amd/csrc/rng_chacha.h, client.cpp): ChaCha20 against the RFC 8439 block-function
vector, the deterministic Box-Muller against libm, and the API contract -- fresh OS entropy by default on every key
generation and every encryption (reference: ChaCha20Stream per call, sampler.jl:1-34), reproducible only when a
deterministic_seed is passed explicitly.

The Gaussian deviate itself (tests/csrc/gauss_check.cpp): box_muller against sqrt(-2 ln u1) cos(2 pi u2) at 60 digits on a directed
list of its edges (u1 = 2^-53 and 1, powers of two, both sides of the mantissa switch, every quadrant boundary of u2) and on 30 000
draws; the same bits from both host compilers; and the sensitivity of the "device words == host words" tests: a build with
contraction on changes a fifth of the deviates, no noise word at the sigmas of the shipped sets, and nine in ten of the changed
deviates' words at sigma = 2^55 -- which is why tests/test_gpu_keygen.py compares keys made at that sigma.  Last, the compile lines of
every object that inlines box_muller carry -ffp-contract=off and nothing that overrides it."""
import os
import shlex
import subprocess

import numpy as np
import pytest

from helpers import ROOT, mk

RFC8439_BLOCK = ("e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 "
                 "466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2")


def test_chacha20_rfc8439_vector_and_gaussian(tmp_path):
    exe = str(tmp_path / "rng_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "mktfhe_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "rng_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0].strip() == RFC8439_BLOCK                      # RFC 8439 section 2.3.2 test vector
    stats = dict(zip(out[1].split()[0::2], out[1].split()[1::2]))
    assert abs(float(stats["mean"])) < 5e-3 and abs(float(stats["var"]) - 1) < 5e-3 and abs(float(stats["kurt"]) - 3) < 0.02
    assert float(stats["max"]) > 4.8                            # real Gaussian tails (4e6 draws reach ~5.2 sigma)
    assert float(out[2].split()[-1]) < 1e-12                    # agrees with libm's sqrt(-2 ln u1) cos(2 pi u2)


def test_default_randomness_is_fresh():
    p = mk.CGGIparam.scaled(n=16, N=64)
    k1, k2 = mk.PartyKeys(p), mk.PartyKeys(p)
    assert not np.array_equal(k1.brk, k2.brk) and not np.array_equal(k1.ksk, k2.ksk)
    keys = [mk.PartyKeys(p) for _ in range(6)]
    assert len({bytes(k.lwekey) for k in keys}) == 6            # 16-bit keys: a collision among 6 is < 0.03 %
    c0, c1, c0b = mk.lwe_encrypt(0, k1, p), mk.lwe_encrypt(1, k1, p), mk.lwe_encrypt(0, k1, p)
    assert not np.array_equal(c0[:-1], c1[:-1]) and not np.array_equal(c0, c0b)     # fresh mask and noise per call
    assert mk.lwe_decrypt(c0, k1, p) is False and mk.lwe_decrypt(c1, k1, p) is True
    q = mk.KMS2party.scaled(n=8, N=64)
    assert not np.array_equal(mk.CRS(q), mk.CRS(q))


def test_deterministic_seed_is_explicit_and_reproducible():
    p = mk.KMS2party.scaled(n=8, N=64)
    a = mk.CRS(p, deterministic_seed=3)
    assert np.array_equal(a, mk.CRS(p, deterministic_seed=3)) and not np.array_equal(a, mk.CRS(p, deterministic_seed=4))
    k0 = mk.party_keygen(a, p, party=0, deterministic_seed=3)
    k0b = mk.party_keygen(a, p, party=0, deterministic_seed=3)
    k1 = mk.party_keygen(a, p, party=1, deterministic_seed=3)
    assert np.array_equal(k0.brk, k0b.brk) and np.array_equal(k0.lwekey, k0b.lwekey)
    assert not np.array_equal(k0.lwekey, k1.lwekey)            # parties draw from different streams of one seed
    c = mk.lwe_ith_encrypt(1, 1, k1, p, deterministic_seed=9)
    assert np.array_equal(c, mk.lwe_ith_encrypt(1, 1, k1, p, deterministic_seed=9))
    raw = bytes(range(32))
    assert np.array_equal(mk.CRS(p, deterministic_seed=raw), mk.CRS(p, deterministic_seed=raw))


def test_native_conversion_without_compare_matches_the_reference_form(tmp_path):
    """fft_device.h native(): the select-free conversion (low dword of v + 2^52) equals arithmetic.jl:1-9's
    `x == 2^W ? 0 : trunc(x)` on every input class: both signs, every exponent from denormals to 2^119, exact multiples
    of 2^W minus tiny offsets (the rounded-up-to-2^W case), fractions"""
    exe = str(tmp_path / "native_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "csrc", "native_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith(" 0 mismatches"), out.stdout[-500:]


# ---- the deviate itself: tests/csrc/gauss_check.cpp ----
CSRC = os.path.join(ROOT, "mktfhe_amd", "csrc")
ROCM_CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")   # compiles the host half of every .hip file
BUILDS = {"g++": ["g++", "-O2", "-ffp-contract=off"],                       # as the Makefile builds client.cpp
          "clang++": [ROCM_CLANG, "-O3", "-ffp-contract=off"],
          "contracted": ["g++", "-O2", "-ffp-contract=fast", "-mfma"]}      # the mutant: what one lost flag on one translation unit gives
WIDE = 2.0 ** 55                                                            # the sigma of tests/test_gpu_keygen.py's wide-noise test
SUITE_SIGMAS = (85.4084, 2.0**4, 2.0**7, 2.0**17, 2.0**20, 2.0**31)         # every sigma the GPU suite compared words at before it
STREAM = 4_000_000
G_MAX_BITS = 0x402124B2800EDA48                                             # 8.5716743486529055 = box_muller(r1 < 2^11, r2 < 2^11): sqrt(-2 ln 2^-53)
# Worst |box_muller - reference| over the directed list and the 30 000 draws, measured with the reference at 60 digits: 2.249668e-15 at
# u1 = 2^-53 (r1 = 0), u2 one step under 1 (r2 = 0xffffffffffffffff) and, the mirror image, one step under 1/2 (r2 = 0x7ffffffffffff800):
# the sine polynomial returns 1 + 2^-52 there, so |g| is 8.571674348652907, one ulp (1.78e-15) above the r of 8.5716743486529055.  The
# 30 000 draws alone: 1.03e-15.  The bound is twice the measured worst.
ABS_ERR_BOUND = 2 * 2.249668e-15


@pytest.fixture(scope="module")
def gauss_exe(tmp_path_factory):
    d, made = tmp_path_factory.mktemp("gauss_check"), {}

    def get(name):
        if name not in made:
            made[name] = str(d / ("gauss_check_" + name.replace("+", "x")))
            subprocess.check_call(BUILDS[name] + ["-I" + CSRC, os.path.join(ROOT, "tests", "csrc", "gauss_check.cpp"), "-o", made[name]])
        return made[name]
    return get


def _need_rocm_clang():
    if not os.path.exists(ROCM_CLANG):
        pytest.skip(f"no ROCm host compiler at {ROCM_CLANG}")


def _need_fma():
    with open("/proc/cpuinfo") as f:
        if not any(line.startswith("flags") and "fma" in line.split() for line in f):
            pytest.skip("this CPU has no fma: the contracted build would not run")


def _u1_r1(k):
    """the smallest r1 with u1 = k 2^-53"""
    return (k - 1) << 11


def directed_pairs():
    """-> (r1 list, r2 list), to be crossed"""
    switch = int(0.70710678118654752 * 2**53)                   # the constant of the m < switch test, as a 53-bit u1
    assert float(switch) * 2.0**-53 == 0.70710678118654752
    r1 = [0, 1, 2**11 - 1, 2**11, 2**64 - 1, 2**64 - 2**11, 2**64 - 2**11 - 1, 2**63, 2**63 - 1, 2**63 - 2**11]
    r1 += [_u1_r1(2**(53 - j)) for j in (1, 2, 3, 10, 26, 27, 51, 52)]      # u1 = 2^-j: m = 1/2 exactly, doubled to 1, s = 0
    r1 += [_u1_r1(switch + d) for d in (-1, 0, 1)]                          # u1 one step under, at and one step over the switch
    r2 = [0, 2**11, 2**64 - 1] + [k * 2**62 + d for k in (1, 2, 3) for d in (-2**11, 0, 2**11)]
    return r1, r2


def _bits_of(exe, mode, stdin=None):
    out = subprocess.run([exe] + mode, input=stdin, capture_output=True, text=True, check=True).stdout
    return [tuple(int(x, 16) for x in ln.split()) for ln in out.splitlines()]


def _directed_lines():
    r1, r2 = directed_pairs()
    return "".join(f"{a:x} {b:x}\n" for a in r1 for b in r2)


def _as_double(bits):
    return float(np.array([bits], dtype=np.uint64).view(np.float64)[0])


def test_deviate_against_a_60_digit_reference_on_its_edges(gauss_exe):
    """box_muller(r1, r2) against sqrt(-2 ln u1) cos(2 pi u2) in mpmath at 60 digits (the cosine as cospi, so that a quarter turn is an
    exact zero), on directed_pairs() crossed and on 30 000 pairs of a stream.  u1 = 1 gives +-0 for every r2; u2 = 1/4 and 3/4 give +-0
    for every r1; u2 = 0 and 1/2 give +r and -r of one r; |g| <= 8.5717 everywhere with the maximum at u1 = 2^-53, where r is
    8.5716743486529055 bit for bit; and the absolute error stays under ABS_ERR_BOUND (twice the measured worst, see there)."""
    mpmath = pytest.importorskip("mpmath")
    exe = gauss_exe("g++")
    r1s, r2s = directed_pairs()
    rows = _bits_of(exe, ["pairs"], _directed_lines())
    assert [(a, b) for a, b, _ in rows] == [(a, b) for a in r1s for b in r2s]
    g = {(a, b): bits for a, b, bits in rows}
    sign = 1 << 63
    for b in r2s:
        for a in (2**64 - 1, 2**64 - 2**11):
            assert g[a, b] & ~sign == 0, ("u1 = 1 is not +-0", hex(a), hex(b))
    for a in r1s:
        assert g[a, 2**62] & ~sign == 0 and g[a, 3 * 2**62] & ~sign == 0, ("a quarter turn is not +-0", hex(a))
        assert g[a, 0] & sign == 0 and g[a, 2**63] == g[a, 0] ^ sign, ("u2 = 0 and 1/2 are not +r and -r", hex(a))
    for a in (0, 1, 2**11 - 1):
        assert g[a, 0] == G_MAX_BITS, hex(g[a, 0])
    assert _as_double(G_MAX_BITS) == 8.5716743486529055
    rows += _bits_of(exe, ["draws", "30000"])
    assert len(rows) == len(r1s) * len(r2s) + 30000
    worst, at, gmax, gat = 0.0, None, 0.0, None
    with mpmath.workdps(60):
        for a, b, bits in rows:
            got = _as_double(bits)
            u1, u2 = mpmath.mpf((a >> 11) + 1) / 2**53, mpmath.mpf(b >> 11) / 2**53
            ref = mpmath.sqrt(-2 * mpmath.log(u1)) * mpmath.cospi(2 * u2)
            err = float(abs(mpmath.mpf(got) - ref))
            if err > worst:
                worst, at = err, (hex(a), hex(b), got)
            if abs(got) > gmax:
                gmax, gat = abs(got), (hex(a), hex(b))
    print(f"box_muller: worst absolute error {worst:.6e} at (r1, r2, g) = {at}; largest |g| {gmax!r} at {gat}")
    assert gmax <= 8.5717 and int(gat[0], 16) < 2**11, (gmax, gat)
    assert worst <= ABS_ERR_BOUND, (worst, at)


def _stream(exe, sigma):
    """-> (bits of STREAM deviates, their noise words at sigma), uint64 each"""
    raw = subprocess.run([exe, "stream", str(STREAM), float(sigma).hex()], capture_output=True, check=True).stdout
    a = np.frombuffer(raw, dtype=np.uint64)
    assert a.size == 2 * STREAM
    return a[:STREAM], a[STREAM:]


def test_both_host_compilers_give_the_same_bits(gauss_exe):
    """g++ (client.cpp) and the ROCm clang++ (the host half of every .hip file), contraction off on both: the same deviate bits on the
    directed list, on 30 000 drawn pairs and on 4 000 000 deviates of a stream, and the same noise words at sigma = 2^55"""
    _need_rocm_clang()
    a, b = gauss_exe("g++"), gauss_exe("clang++")
    lines = _directed_lines()
    assert _bits_of(a, ["pairs"], lines) == _bits_of(b, ["pairs"], lines)
    assert _bits_of(a, ["draws", "30000"]) == _bits_of(b, ["draws", "30000"])
    (ga, wa), (gb, wb) = _stream(a, WIDE), _stream(b, WIDE)
    assert np.array_equal(ga, gb), ("deviates that differ between the compilers", int((ga != gb).sum()))
    assert np.array_equal(wa, wb)


def test_a_contracted_build_shows_at_wide_sigma_only(gauss_exe):
    """What the word-for-word tests can see.  The mutant is the header compiled with -ffp-contract=fast -mfma.  Over 4 000 000 deviates
    it changes deviate bits (about a fifth of them), and at sigma = 2^55 at least 90 % of the changed deviates give another 64-bit noise
    word and another low 32-bit half -- so keys made at that sigma expose it on either ring width.  At the sigmas the GPU suite otherwise
    compares words at the count of changed words is printed, not asserted: measured 0 at every one of them, which is the blindness the
    wide-noise test closes ("The shared Gaussian")."""
    _need_fma()
    ref, mut = gauss_exe("g++"), gauss_exe("contracted")
    (g0, w0), (g1, w1) = _stream(ref, WIDE), _stream(mut, WIDE)
    changed = g0 != g1
    nch = int(changed.sum())
    assert nch > 0, "contraction changes no deviate: the mutant is not a mutant"
    seen64 = int((changed & (w0 != w1)).sum())
    seen32 = int((changed & ((w0 ^ w1) & np.uint64(0xFFFFFFFF) != 0)).sum())
    print(f"contracted build: {nch} of {STREAM} deviates change ({nch / STREAM:.1%}); at sigma 2^55 {seen64} words change "
          f"({seen64 / nch:.1%}), {seen32} low halves ({seen32 / nch:.1%})")
    for sigma in SUITE_SIGMAS:
        (_, v0), (_, v1) = _stream(ref, sigma), _stream(mut, sigma)
        print(f"contracted build: sigma {sigma!r}: {int((v0 != v1).sum())} noise words change")
    assert seen64 >= 0.9 * nch, f"only {seen64 / nch:.1%} of the changed deviates change the 64-bit word at sigma 2^55"
    assert seen32 >= 0.9 * nch, f"only {seen32 / nch:.1%} of the changed deviates change the low 32 bits at sigma 2^55"


# ---- the compile lines of the objects that inline box_muller ----
NOISE_OBJECTS = {"keygen.o": "keygen.hip", "partial_decrypt.o": "partial_decrypt.hip", "seeded.o": "seeded.hip", "client.o": "client.cpp",
                 "context.o": "context.cpp"}
_FP_OVERRIDES = ("-ffp-contract", "-ffast-math", "-Ofast", "-ffp-model", "-funsafe-math-optimizations", "-menable-unsafe-fp-math")


def contraction_fault(argv):
    """None if the compile line has -ffp-contract=off and, after it, no option that sets the contraction mode again; else what is wrong"""
    if "-ffp-contract=off" not in argv:
        return "no -ffp-contract=off"
    last = len(argv) - 1 - argv[::-1].index("-ffp-contract=off")
    later = [a for a in argv[last + 1:] if a.startswith(_FP_OVERRIDES)]
    return f"{later} after -ffp-contract=off" if later else None


def test_objects_that_inline_box_muller_are_built_without_contraction():
    """make -n prints the command of each of the five objects (MKT_TUNE=0: as a clean checkout with an older compiler builds them): each
    has -ffp-contract=off with nothing after it that sets the mode again, and none of the three .hip units carries a per-unit -mllvm option"""
    cmd = ["make", "-n", "-B", "-C", CSRC, "MKT_TUNE=0", "SFX="] + ["build/" + o for o in NOISE_OBJECTS]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    lines = [shlex.split(ln) for ln in out.splitlines() if " -c " in ln and " -o " in ln]
    by_obj = {os.path.basename(a[a.index("-o") + 1]): a for a in lines}
    assert sorted(by_obj) == sorted(NOISE_OBJECTS), out
    for obj, src in NOISE_OBJECTS.items():
        argv = by_obj[obj]
        assert argv[argv.index("-c") + 1] == src, (obj, argv)
        assert contraction_fault(argv) is None, (obj, contraction_fault(argv), argv)
        if src.endswith(".hip"):
            assert "-mllvm" not in argv, (obj, argv)
    # the judge itself: the lines it must refuse
    good = by_obj["keygen.o"]
    assert contraction_fault([a for a in good if a != "-ffp-contract=off"]) == "no -ffp-contract=off"
    for extra in ("-ffp-contract=fast", "-ffp-contract=on", "-ffast-math", "-Ofast", "-ffp-model=fast"):
        assert contraction_fault(good + [extra]) is not None, extra
    assert contraction_fault(["hipcc", "-ffp-contract=fast", "-ffp-contract=off", "-c", "x.hip"]) is None
