"""Independent opener and statistics for generated keys and ciphertexts: what every key component must BE under the party's
secrets, in plain numpy / Python integers (oracle.negacyclic for the exact ring product; nothing of mktfhe_amd/csrc), and how far
its noise, masks and secrets may lie from the law the reference states.  Nothing here knows how the generator lays out its random
streams: independence is judged by distinctness and correlation of what was produced.

Laws (reference, restated):
  noise        round(sigma * N(0,1))                                  sampler.jl:24-28
  masks, CRS   uniform words mod 2^W                                   lwe.jl:11-22, :78-93; scheme.jl:409-410
  binary key   independent fair bits                                   key.jl:12-19
  ternary r    uniform on {-1, 0, 1}                                   sampler.jl:1-5, unienc.jl:36-55
  block key    per block one index uniform on 0..blk_len, 0 = no 1     sampler.jl:7-21

THRESHOLDS.  Every statistic returns a two-sided p-value against its law (a maximum over several positions or pairs is already
multiplied by their number).  A check passes when p >= ALPHA = BUDGET / CHECKS:
  BUDGET = 1e-6   false-failure probability allowed to one whole run of tests/test_keys_cpu.py on law-abiding keys
  CHECKS = 4000   upper bound on the p-value checks of one run (the module counts them and asserts the bound at its end:
                  ~20 parameter sets x <= 8 components x <= 12 statistics, plus masks, independence and secrets)
  ALPHA  = 2.5e-10, i.e. |z| <= 6.33 for a normal statistic.
At m = 10^5 residuals the variance statistic has a standard error of sqrt(2/m) = 0.45 %, so 6.33 of them is 2.8 % of sigma^2:
a 2 % error in sigma (4 % in the variance) fails.  Seeds are pinned, so a pass is reproducible; the budget matters for the
fresh-entropy case.  Normal approximations are used only where they hold at that depth: the variance goes through Wilson-Hilferty
(chi-square with m degrees of freedom, good from m ~ 30), counts through the exact binomial tail, chi-squares through the exact
survival function; kurtosis and the 3-sigma share are evaluated on pools of >= MIN_SHAPE residuals only (the kurtosis estimate is
still skewed below that).
The one bound that is not a p-value is the issue's max|e| <= 6 sigma + 1 (the bound tests/test_gpu_parity.py already applies to
the device keys): the generator's Gaussian reaches 8.5 sigma, so a law-abiding draw exceeds it with probability 2e-9; on pinned
seeds that is a fixed outcome, on the fresh-entropy case (2e4 residuals) a 4e-5 chance per run.
"""
import math

import numpy as np

from oracle import oracle as O

BUDGET, CHECKS = 1e-6, 4000
ALPHA = BUDGET / CHECKS                     # 2.5e-10 per check: two-sided z = 6.33
MIN_SHAPE = 50_000                          # residuals a shape statistic (kurtosis, 3-sigma share) needs
CGGI, LMSS, CCS, KMS, KMS_BLOCK = range(5)  # scheme codes of the parameter sets (mktfhe.h)


# ------------------------------------------------------------------------------------------------------------------
# exact arithmetic mod 2^W
# ------------------------------------------------------------------------------------------------------------------
def _mask(W):
    return np.uint64((1 << W) - 1)


def words(x, W):
    """any integer array -> uint64 holding the words mod 2^W"""
    x = np.asarray(x)
    if x.dtype.kind == "i":
        x = x.astype(np.int64).astype(np.uint64)
    return x.astype(np.uint64) & _mask(W)


def centered(x, W):
    """words mod 2^W -> int64 in [-2^(W-1), 2^(W-1))"""
    x = np.asarray(x, dtype=np.uint64) & _mask(W)
    if W == 64:
        return x.astype(np.int64)
    v = x.astype(np.int64)
    return np.where(v >= (1 << (W - 1)), v - (1 << W), v)


def ring_mul(a, s, W):
    """a * s in Z_{2^W}[X]/(X^N + 1), exactly; s small signed integers"""
    return O.negacyclic(words(a, W), words(np.asarray(s, dtype=np.int64), W), W) & _mask(W)


def _add(*xs):
    with np.errstate(over="ignore"):
        out = np.zeros_like(np.asarray(xs[0], dtype=np.uint64))
        for x in xs:
            out = out + np.asarray(x, dtype=np.uint64)
    return out


def _sub(a, b):
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.uint64) - np.asarray(b, dtype=np.uint64)


def _gadget(W, j, logB):
    return (1 << (W - (j + 1) * logB)) & ((1 << 64) - 1)


def shape_of(p):
    """(ring keys under the RGSW rows, key-switch ring keys, first key-switch ring key, key-switch digit rows)"""
    mkey = p.scheme in (CCS, KMS, KMS_BLOCK)
    D = 1 << p.logD
    return (1 if mkey else p.k), (1 if mkey else p.k), (1 if p.scheme in (KMS, KMS_BLOCK) else 0), (D // 2 if p.scheme in (LMSS, KMS_BLOCK) else D - 1)


# ------------------------------------------------------------------------------------------------------------------
# openers: component -> dict(masks=[...] ring polynomials or LWE rows, e=int64 residuals, r=recovered ternary or None)
# ------------------------------------------------------------------------------------------------------------------
def open_rgsw(p, brk, lwekey, z):
    """RGSW bootstrapping key [n][(kr+1) l][kr+1][N]: row (i, c, j) is an RLWE sample (b, a_0..a_{kr-1}) under z with s_i g_j added to
    coefficient 0 of polynomial c (gsw.jl:174-178, lev.jl:88-102, lwe.jl:78-93) -> masks [rows][kr][N], e [rows][N]"""
    N, W, n, l, logB = p.N, p.W, p.n, p.l_gsw, p.logB_gsw
    kr = shape_of(p)[0]
    rows = np.array(brk, dtype=np.uint64).reshape(n, kr + 1, l, kr + 1, N)
    for i in range(n):
        for c in range(kr + 1):
            for j in range(l):
                rows[i, c, j, c, 0] = (int(rows[i, c, j, c, 0]) - int(lwekey[i]) * _gadget(W, j, logB)) % (1 << W)
    rows = rows.reshape(-1, kr + 1, N)
    e = np.empty((rows.shape[0], N), dtype=np.int64)
    for r, row in enumerate(rows):
        e[r] = centered(_add(row[0], *[ring_mul(row[1 + q], z[q], W) for q in range(kr)]), W)
    return dict(masks=rows[:, 1:, :], e=e, r=None)


def open_unienc(p, d, f, crs, z, mu):
    """UniEnc of the polynomial mu under z (unienc.jl:36-55): d_j = crs_j r + mu g_j + e1_j, f_j = (b, a) = RLWE_z(g_j r), one ternary r;
    d [l][N], f [l][2][N].  r is read off the phase of f_0 (g_0 r + e), then everything is opened with it
    -> masks [l][N] (the a of f), e_d [l][N], e_f [l][N], r [N]"""
    N, W, l, logB = p.N, p.W, p.l_uni, p.logB_uni
    d = words(np.asarray(d).reshape(l, N), W)
    f = words(np.asarray(f).reshape(l, 2, N), W)
    crs = words(np.asarray(crs).reshape(l, N), W)
    ph = [_add(f[j, 0], ring_mul(f[j, 1], z, W)) for j in range(l)]
    g0 = _gadget(W, 0, logB)
    c0 = centered(ph[0], W)
    r = np.array([(int(v) + g0 // 2) // g0 for v in c0], dtype=np.int64)            # exact integer rounding
    assert set(np.unique(r).tolist()) <= {-1, 0, 1}, "UniEnc: f_0 does not open to a ternary r"
    e_d = np.empty((l, N), dtype=np.int64)
    e_f = np.empty((l, N), dtype=np.int64)
    mu = words(np.asarray(mu, dtype=np.int64), W)
    for j in range(l):
        g = np.uint64(_gadget(W, j, logB))
        with np.errstate(over="ignore"):
            e_f[j] = centered(_sub(ph[j], words(r, W) * g), W)
            e_d[j] = centered(_sub(_sub(d[j], ring_mul(crs[j], r, W)), mu * g), W)
    return dict(masks=f[:, 1, :], e_d=e_d, e_f=e_f, r=r)


def open_ccs_brk(p, brk, crs, lwekey, z):
    """CCS bootstrapping key [n][3 l][N] (d_0..d_{l-1}, then (b, a) of f_0..f_{l-1}): UniEnc_z(s_i), one r per key bit"""
    N, l = p.N, p.l_uni
    rows = np.asarray(brk).reshape(p.n, 3 * l, N)
    out = []
    for i in range(p.n):
        mu = np.zeros(N, dtype=np.int64)
        mu[0] = int(lwekey[i])
        out.append(open_unienc(p, rows[i, :l], rows[i, l:], crs, z, mu))
    return dict(masks=np.concatenate([o["masks"] for o in out]), e_d=np.concatenate([o["e_d"] for o in out]),
                e_f=np.concatenate([o["e_f"] for o in out]), r=np.stack([o["r"] for o in out]))


def open_pubkey(p, pub, crs, z):
    """b_j = -z crs_j + e (unienc.jl:77-90) -> e [l][N]"""
    N, W, l = p.N, p.W, p.l_uni
    pub, crs = words(np.asarray(pub).reshape(l, N), W), words(np.asarray(crs).reshape(l, N), W)
    return dict(masks=[], e=np.stack([centered(_add(pub[j], ring_mul(crs[j], z, W)), W) for j in range(l)]), r=None)


def open_ksk(p, ksk, lwekey, zs):
    """key-switching key [kk][N][dr][f][n+1]: row (c, j, d, t) is an LWE sample (a, b = e - <a, s> + msg) of
    msg = (d+1) z_c[j] 2^(32-(t+1) logD) (keygen.jl:17-23, lev.jl:31-37); block schemes: the rows of the coefficients below the
    embedded LWE key are absent, i.e. all zero (keygen.jl:43-51, :147-151) -> masks [kk][N][dr][f][n], e [kk][N][dr][f], live [kk][N]"""
    N, n = p.N, p.n
    _, kk, zoff, dr = shape_of(p)
    K = np.asarray(ksk, dtype=np.uint32).reshape(kk, N, dr, p.f, n + 1)
    s = np.asarray(lwekey, dtype=np.uint32)
    phase = (K[..., n] + (K[..., :n] * s).sum(-1, dtype=np.uint32)).astype(np.uint32)
    e = np.empty(phase.shape, dtype=np.int64)
    for c in range(kk):
        zc = np.asarray(zs[zoff + c], dtype=np.int64)
        for t in range(p.f):
            want = ((np.arange(1, dr + 1)[None, :] * zc[:, None]) << (32 - (t + 1) * p.logD)) & 0xFFFFFFFF
            e[c, :, :, t] = centered((phase[c, :, :, t].astype(np.int64) - want) & 0xFFFFFFFF, 32)
    live = np.ones((kk, N), dtype=bool)
    if p.scheme in (LMSS, KMS_BLOCK):
        live = (np.arange(kk)[:, None] * N + np.arange(N)[None, :]) >= n
    assert not K[~live].any(), "key-switching rows below the embedded LWE key must be absent (all zero)"
    assert K[live][..., :n].reshape(-1, n).any(axis=1).all(), "a key-switching row that must be present is empty"
    return dict(masks=K[..., :n], e=e, live=live, r=None)


def open_lwe(p, ct, party, lwekey, bit):
    """lwe_ith_encrypt (scheme.jl:352-386): mask in the party's block only, b = e - <a, s> + (2 bit - 1) 2^29 -> (mask [B][n], e [B]);
    asserts that every other party's block is zero, word for word"""
    n = p.n
    ct = np.asarray(ct, dtype=np.uint32).reshape(-1, p.lwe_len)
    blocks = ct[:, :-1].reshape(ct.shape[0], -1, n)
    other = np.delete(blocks, party, axis=1)
    assert not other.any(), "an encryption under party %d has words in another party's block" % party
    a = blocks[:, party, :]
    mu = np.where(np.asarray(bit, dtype=bool), 1 << 29, (1 << 32) - (1 << 29)).astype(np.uint32)
    e = (ct[:, -1] + (a * np.asarray(lwekey, dtype=np.uint32)).sum(-1, dtype=np.uint32) - mu).astype(np.uint32)
    return a, centered(e, 32)


# ------------------------------------------------------------------------------------------------------------------
# p-values
# ------------------------------------------------------------------------------------------------------------------
def p_of_z(z, tries=1):
    """two-sided normal p-value of the largest of `tries` z-scores (Bonferroni)"""
    return min(1.0, tries * math.erfc(abs(float(z)) / math.sqrt(2.0)))


def chi2_sf(x, df):
    """P(chi-square with df degrees of freedom >= x), exact: Q(df) = Q(df - 2) + (x/2)^(df/2 - 1) e^(-x/2) / Gamma(df/2)"""
    if x <= 0:
        return 1.0
    h = x / 2.0
    if df % 2:
        q, k = math.erfc(math.sqrt(h)), 0.5
    else:
        q, k = math.exp(-h), 1.0
    while k < df / 2.0 - 1e-9:
        q += math.exp(k * math.log(h) - h - math.lgamma(k + 1.0))
        k += 1.0
    return min(1.0, q)


def p_chi2(counts, probs):
    """chi-square of observed counts against cell probabilities (every expected count should be >= 5) -> upper-tail p"""
    counts, probs = np.asarray(counts, dtype=np.float64), np.asarray(probs, dtype=np.float64)
    ex = counts.sum() * probs / probs.sum()
    return chi2_sf(float(((counts - ex) ** 2 / ex).sum()), len(counts) - 1)


def p_binom(k, m, q):
    """exact two-sided binomial p-value: 2 min(P(X <= k), P(X >= k)), X ~ Bin(m, q)"""
    if q <= 0.0 or q >= 1.0:
        return 1.0 if k == (m if q >= 1.0 else 0) else 0.0
    lq, l1 = math.log(q), math.log1p(-q)
    pmf = lambda i: math.exp(math.lgamma(m + 1) - math.lgamma(i + 1) - math.lgamma(m - i + 1) + i * lq + (m - i) * l1)   # noqa: E731

    def tail(step):
        tot, i = 0.0, k
        while 0 <= i <= m:
            t = pmf(i)
            tot += t
            if t < 1e-18 * tot and ((i - m * q) * step > 0):
                break
            i += step
        return tot
    return min(1.0, 2.0 * min(tail(-1), tail(+1)))


def _phi(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def noise_pmf(v, sigma):
    """P(round(sigma N(0,1)) = v): Phi((v + 1/2) / sigma) - Phi((v - 1/2) / sigma), computed in the tail that keeps its digits"""
    v = abs(v)
    return 0.5 * (math.erfc((v - 0.5) / sigma / math.sqrt(2.0)) - math.erfc((v + 0.5) / sigma / math.sqrt(2.0)))


def noise_stats(e, sigma):
    """e: residuals [rows][N] (or flat) that should be round(sigma N(0,1)) -> {name: p}: mean (SE sqrt(var/m)), variance against
    sigma^2 + 1/12 (Wilson-Hilferty on sum e^2 / var ~ chi-square(m); SE var sqrt(2/m) for large m), lag-1 autocorrelation along
    each row (SE 1/sqrt(m)); for sigma <= 128 the chi-square of the histogram against the exact pmf (this is what tells rounding
    from truncation: at sigma = 1, P(0) = 0.383 against 0.683); on >= MIN_SHAPE residuals also the sample-normalised excess
    kurtosis (SE sqrt(24/m)) and the share beyond 3 sigma (exact binomial)"""
    e2 = np.atleast_2d(np.asarray(e, dtype=np.int64))
    x = e2.astype(np.float64).ravel()
    m = x.size
    var = sigma * sigma + 1.0 / 12.0
    out = {"mean": p_of_z(x.mean() / math.sqrt(var / m))}
    s = float((x * x).sum()) / var
    out["variance"] = p_of_z(((s / m) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * m))) / math.sqrt(2.0 / (9.0 * m)))
    if e2.shape[1] > 1:
        pairs = e2.shape[0] * (e2.shape[1] - 1)
        out["lag1"] = p_of_z(float((e2[:, 1:].astype(np.float64) * e2[:, :-1]).sum()) / (var * math.sqrt(pairs)))
    if sigma <= 128.0:
        K = max(1, int(2.5 * sigma))
        while K > 1 and m * noise_pmf(K, sigma) < 8.0:
            K -= 1
        xi = e2.ravel()
        inner = np.bincount(np.clip(xi, -K - 1, K + 1) + K + 1, minlength=2 * K + 3)
        probs = [noise_pmf(v, sigma) for v in range(-K, K + 1)]
        tailp = (1.0 - sum(probs)) / 2.0
        out["histogram"] = p_chi2(inner, [tailp] + probs + [tailp])
    if m >= MIN_SHAPE and sigma >= 4.0:
        c = x - x.mean()
        out["kurtosis"] = p_of_z(((c ** 4).mean() / (c * c).mean() ** 2 - 3.0) / math.sqrt(24.0 / m))
        cut = math.floor(3.0 * sigma)
        out["beyond 3 sigma"] = p_binom(int((np.abs(x) > cut).sum()), m, math.erfc((cut + 0.5) / sigma / math.sqrt(2.0)))
    return out


def uniform_stats(w, W):
    """w: words that should be uniform mod 2^W -> {name: p}: frequency of each of the W bit positions (largest |z| of W), chi-square
    over the top byte and over the low byte"""
    w = np.asarray(w, dtype=np.uint64).ravel()
    m = w.size
    ones = np.array([int(((w >> np.uint64(b)) & np.uint64(1)).sum()) for b in range(W)], dtype=np.float64)
    out = {"bit frequency": p_of_z(np.abs((ones - m / 2.0) / math.sqrt(m / 4.0)).max(), tries=W)}
    if m >= 256 * 8:
        out["top byte"] = p_chi2(np.bincount((w >> np.uint64(W - 8)).astype(np.int64), minlength=256), np.full(256, 1.0))
        out["low byte"] = p_chi2(np.bincount((w & np.uint64(255)).astype(np.int64), minlength=256), np.full(256, 1.0))
    return out


def count_equal_rows(rows):
    """number of rows of a 2-D array that repeat an earlier row"""
    rows = np.ascontiguousarray(rows)
    if rows.shape[0] < 2:
        return 0
    v = rows.view(np.dtype((np.void, rows.dtype.itemsize * rows.shape[1]))).ravel()
    return int(v.size - np.unique(v).size)


def count_equal_words(chunks):
    """number of words, over all the arrays in `chunks`, that repeat another word"""
    w = np.concatenate([np.asarray(c).ravel() for c in chunks])
    return int(w.size - np.unique(w).size)


def cross_correlation(vectors):
    """vectors [R][L] -> p of the largest normalised cross-correlation over all R (R-1) / 2 pairs: rho sqrt(L) is a unit normal for
    independent rows (its true tail is lighter, so the union bound over the pairs errs on the side of passing)"""
    v = np.asarray(vectors, dtype=np.float64)
    v = v - v.mean(axis=1, keepdims=True)
    nrm = np.sqrt((v * v).sum(axis=1, keepdims=True))
    assert (nrm > 0).all(), "a constant noise vector"
    c = (v / nrm) @ (v / nrm).T
    np.fill_diagonal(c, 0.0)
    R, L = v.shape
    return p_of_z(float(np.abs(c).max()) * math.sqrt(L), tries=R * (R - 1) // 2)


def binary_weight(bits):
    bits = np.asarray(bits).ravel()
    assert set(np.unique(bits).tolist()) <= {0, 1}
    return p_of_z((float(bits.sum()) - bits.size / 2.0) / math.sqrt(bits.size / 4.0))


def ternary_uniform(r):
    r = np.asarray(r).ravel()
    assert set(np.unique(r).tolist()) <= {-1, 0, 1}
    return p_chi2(np.bincount(r + 1, minlength=3), [1.0, 1.0, 1.0])


def block_indices(lwekeys, blk_len):
    """block-binary keys [keys][blk_d * blk_len] -> the drawn index of every block (0 = no 1); asserts at most one 1 per block"""
    b = np.asarray(lwekeys).reshape(-1, blk_len)
    assert set(np.unique(b).tolist()) <= {0, 1} and (b.sum(axis=1) <= 1).all(), "a block holds more than one 1"
    return np.where(b.any(axis=1), b.argmax(axis=1) + 1, 0)


def block_uniform(lwekeys, blk_len):
    return p_chi2(np.bincount(block_indices(lwekeys, blk_len), minlength=blk_len + 1), np.full(blk_len + 1, 1.0))
