"""Independent restatement of packed outputs (include/mktfhe_pack.h): packing-key generation from the ChaCha20 streams, the pack itself, the
ring phase and the ring shares.  Integer parts are numpy / Python integers; a gadget product takes its transforms from the checker's
primitives (oracle.Ffter.fwd / inv, oracle.decomp_poly) and its product step from tests/ref_numpy.py (explicit real operations); the exact
form takes the schoolbook product (oracle.negacyclic).  Nothing of mktfhe_amd/csrc is called.

NOISE PREDICTION (32-bit torus words, per coefficient of a pack holding c rows; nparty n mask words per row):
    key term       nparty n l_pk c E[d^2] sigma_ring^2 / 2^(2 (W - 32)),   E[d^2] = 2^(2 logB_pk) / 12
    rounding term  (nparty n / 2) 2^(2 (32 - l_pk logB_pk)) / 12           when l_pk logB_pk < 32, else 0
BAND of measured / predicted deviation over m samples, derived as law A of tests/noise_cases.py derives its own: 5 standard errors of a
sample deviation, sqrt((kappa - 1) / 4m), plus a stated model term.
    rounding case: the error is a sum of hw uniform terms (hw = ones of the LWE keys), kappa = 3 - 1.2 / hw; the prediction puts
        nparty n / 2 for hw, which is binomial: model term 5 standard deviations of sqrt(hw / (nparty n / 2)) = 2.5 / sqrt(nparty n).
        Against the keys' own hw the model term is 0.
    key case: kappa = 3 (a sum of nparty n l_pk c terms); model terms: the key noise is drawn once, so the variance given the key is
        sum d^2 e^2 over nparty n l_pk N noise words -- 5 sqrt(2 / (nparty n l_pk N)) / 2; integer digits on [-B/2, B/2) have
        E[d^2] = (B^2 + 2) / 12 and rounded noise sigma^2 + 1/12: (2 / B^2 + 1 / (12 sigma^2)) / 2; the rounding term is part of the prediction.
"""
import math

import numpy as np

from oracle import oracle as O
from ref_keys import centered, ring_mul, words
from ref_numpy import C
from ref_seeded import chacha20_block, seed_key

STREAM_PACK_KEY, STREAM_PACK_SMUDGE = 17, 18
CGGI, LMSS, CCS, KMS, KMS_BLOCK = range(5)
M64 = (1 << 64) - 1


def shape(p):
    """(nparty, kr: ring components per party, zoff: first ring key used, mk)"""
    mk = p.scheme in (CCS, KMS, KMS_BLOCK)
    return (p.k if mk else 1), (1 if mk else p.k), (1 if p.scheme in (KMS, KMS_BLOCK) else 0), mk


def slot(p, party, c):
    return party if shape(p)[3] else c


def gadget_ok(l, logB):
    return 1 <= logB <= 16 and l >= 1 and l * logB <= 32


# ---- the streams: 64-bit draws are word pairs of the keystream, low word first; the deviate of rng_chacha.h restated in Python floats ----
def draws(seed, party, stream, b, c, count):
    """the first `count` 64-bit draws of stream (stream, party, b, c) keyed by the 32 seed bytes -> uint64 [count]"""
    nblk = (count + 7) // 8
    w = chacha20_block(seed_key(seed), np.arange(nblk, dtype=np.uint32), [np.uint32((stream & 0xFFFF) | (party << 16)), np.uint32(b), np.uint32(c)]).reshape(-1).astype(np.uint64)
    return (w[0::2] | (w[1::2] << np.uint64(32)))[:count]


def _cos_sin(t2):
    c = 1.0 / 2432902008176640000.0
    for k in (-1.0 / 6402373705728000.0, 1.0 / 20922789888000.0, -1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0,
              1.0 / 24.0, -0.5, 1.0):
        c = c * t2 + k
    s = 1.0 / 51090942171709440000.0
    for k in (-1.0 / 121645100408832000.0, 1.0 / 355687428096000.0, -1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800.0, 1.0 / 362880.0,
              -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0, 1.0):
        s = s * t2 + k
    return c, s


def gauss(r1, r2):
    """unit normal deviate of two 64-bit draws: Box-Muller with ln, sqrt and cos written out in IEEE add, multiply, divide"""
    import struct
    u1 = float((r1 >> 11) + 1) * 2.0 ** -53
    u2 = float(r2 >> 11) * 2.0 ** -53
    b = struct.unpack("<Q", struct.pack("<d", u1))[0]
    e = ((b >> 52) & 0x7FF) - 1022
    m = struct.unpack("<d", struct.pack("<Q", (b & 0x000FFFFFFFFFFFFF) | 0x3FE0000000000000))[0]
    if m < 0.70710678118654752:
        m, e = m * 2.0, e - 1
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    pl = 1.0 / 21.0
    for k in (19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        pl = pl * s2 + 1.0 / k
    pl = pl * s2 + 1.0
    x = -2.0 * (float(e) * 0.6931471805599453 + 2.0 * s * pl)
    r = 0.0
    if x > 0.0:
        r = struct.unpack("<d", struct.pack("<Q", (struct.unpack("<Q", struct.pack("<d", x))[0] >> 1) + 0x1FF8000000000000))[0]
        for _ in range(6):
            r = 0.5 * (r + x / r)
    f4 = u2 * 4.0
    q = int(f4)
    th = (f4 - float(q)) * 1.5707963267948966
    c, sn = _cos_sin(th * th)
    sn = sn * th
    return r * (c, -sn, -c, sn)[q]


def noise_words(d, sigma):
    """draws [2 m] -> m noise words round(sigma g) as Python integers (round half to even, as rint)"""
    return [int(round(sigma * gauss(int(d[2 * i]), int(d[2 * i + 1])))) for i in range(len(d) // 2)]


# ---- the packing key ----
def packing_key(p, lwekey, zs, party, l, logB, seed, sigma_ring):
    """[n][l][1 + kr][N] uint64: row (q, t) = (b, a_0 ..), a_c the first kr N draws of stream (17, party, q, t) masked to W bits,
    b = -sum a_c z_c + e + s[q] 2^(W - (t+1) logB) X^0, e the next N noise draws.  zs: the party's ring keys as mkt_client_ringkey numbers them"""
    _, kr, zoff, _ = shape(p)
    N, W = p.N, p.W
    mask = (1 << W) - 1
    out = np.zeros((p.n, l, 1 + kr, N), dtype=np.uint64)
    for q in range(p.n):
        for t in range(l):
            d = draws(seed, party, STREAM_PACK_KEY, q, t, kr * N + 2 * N)
            b = np.zeros(N, dtype=np.uint64)
            for c in range(kr):
                a = d[c * N:(c + 1) * N] & np.uint64(mask)
                out[q, t, 1 + c] = a
                with np.errstate(over="ignore"):
                    b = b - ring_mul(a, zs[zoff + c], W)
            e = noise_words(d[kr * N:], sigma_ring)
            bb = [(int(b[j]) + e[j]) & mask for j in range(N)]
            bb[0] = (bb[0] + (int(lwekey[q]) << (W - (t + 1) * logB))) & mask
            out[q, t, 0] = np.array(bb, dtype=np.uint64)
    return out


def open_key(p, pk, lwekey, zs, l, logB):
    """every row under the ring secrets, minus s[q] g_t at coefficient 0 -> residuals e int64 [n l][N], masks [n l][kr][N]"""
    _, kr, zoff, _ = shape(p)
    N, W = p.N, p.W
    rows = words(np.asarray(pk).reshape(p.n, l, 1 + kr, N), W)
    e = np.empty((p.n * l, N), dtype=np.int64)
    for q in range(p.n):
        for t in range(l):
            ph = rows[q, t, 0].copy()
            with np.errstate(over="ignore"):
                for c in range(kr):
                    ph = ph + ring_mul(rows[q, t, 1 + c], zs[zoff + c], W)
            ph[0] = np.uint64((int(ph[0]) - (int(lwekey[q]) << (W - (t + 1) * logB))) & M64)
            e[q * l + t] = centered(ph, W)
    return e, rows[:, :, 1:, :].reshape(p.n * l, kr, N)


# ---- the pack ----
def columns(p, rows, g):
    """lifted columns of pack g of the picked rows [B][lwe_len] -> uint64 [lwe_len][N]; absent rows are zero"""
    N, W = p.N, p.W
    part = np.asarray(rows, dtype=np.uint32)[g * N:(g + 1) * N]
    col = np.zeros((part.shape[1] if part.ndim == 2 else 0, N), dtype=np.uint64)
    col[:, :part.shape[0]] = part.T.astype(np.uint64) << np.uint64(W - 32)
    return col


def digits(p, cols, l, logB):
    """decompto! of columns [c][N] with the packing gadget -> uint64 [c][l][N] (wrapped signed digits)"""
    c, N = cols.shape
    return O.decomp_poly(np.ascontiguousarray(cols).reshape(-1), l, logB, p.W).reshape(l, c, N).transpose(1, 0, 2)


def _cparts(t):
    return C(np.ascontiguousarray(t.real), np.ascontiguousarray(t.imag))


def pack(p, rows, pks, l, logB, exact=False, idx=None, pool=None):
    """rows [B][lwe_len] (or pool + idx) -> [ceil(B / N)][1 + k][N] uint64; pks[i]: party i's key [n][l][1 + kr][N]"""
    if pool is not None:
        rows = np.asarray(pool, dtype=np.uint32).reshape(-1, p.lwe_len)[np.asarray(idx, dtype=np.int64)]
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, p.lwe_len)
    nparty, kr, _, _ = shape(p)
    N, W, n = p.N, p.W, p.n
    mask = np.uint64((1 << W) - 1)
    f = O.Ffter(N, W)
    npacks = -(-rows.shape[0] // N)
    out = np.zeros((npacks, 1 + p.k, N), dtype=np.uint64)
    keys = [words(np.asarray(pk).reshape(n, l, 1 + kr, N), W) for pk in pks]
    fkeys = None if exact else [f.fwd(k) for k in keys]
    for g in range(npacks):
        col = columns(p, rows, g)
        with np.errstate(over="ignore"):
            out[g, 0] = col[-1]
            for i in range(nparty):
                D = digits(p, col[i * n:(i + 1) * n], l, logB)                    # [n][l][N]
                if exact:
                    for q in range(n):
                        for t in range(l):
                            for c in range(1 + kr):
                                dst = 0 if c == 0 else 1 + slot(p, i, c - 1)
                                out[g, dst] = out[g, dst] + O.negacyclic(D[q, t], keys[i][q, t, c], W)
                    continue
                fd = f.fwd(D)                                                      # fftto! of every digit polynomial
                for c in range(1 + kr):
                    acc = C(np.zeros((n, N // 2)), np.zeros((n, N // 2)))          # initialise!
                    for t in range(l):                                             # muladdto!, t ascending
                        acc = acc + _cparts(fd[:, t]) * _cparts(fkeys[i][:, t, c])
                    G = f.inv(acc.re + 1j * acc.im)                                # one ifftto! per key polynomial and (i, q)
                    dst = 0 if c == 0 else 1 + slot(p, i, c - 1)
                    out[g, dst] = out[g, dst] + G.sum(axis=0, dtype=np.uint64)
        out[g] &= mask
    return out


# ---- opening ----
def ring_keys(p, keys):
    """[party][c] -> the ring key polynomial a packed ciphertext's component c of that party is under; keys[i].ringkey(idx)"""
    nparty, kr, zoff, _ = shape(p)
    return [[np.asarray(keys[i].ringkey(zoff + c), dtype=np.int64) for c in range(kr)] for i in range(nparty)]


def share(p, ct, zs_party, party):
    """sum_c a_{slot(party, c)} (*) z_c of one packed ciphertext [1 + k][N] -> uint64 [N] (no smudging noise)"""
    ct = words(np.asarray(ct).reshape(1 + p.k, p.N), p.W)
    s = np.zeros(p.N, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for c, z in enumerate(zs_party):
            s = s + ring_mul(ct[1 + slot(p, party, c)], z, p.W)
    return s & np.uint64((1 << p.W) - 1)


def smudge(p, seed, party, pack_index, sigma):
    """the N smudging words of pack `pack_index` (stream 18), lifted to the ring's width -> uint64 [N]"""
    d = draws(seed, party, STREAM_PACK_SMUDGE, pack_index & 0xFFFFFFFF, pack_index >> 32, 2 * p.N)
    return np.array([(e << (p.W - 32)) & ((1 << p.W) - 1) for e in noise_words(d, sigma)], dtype=np.uint64)


def phase(p, ct, zs):
    """top 32 bits of b + sum a z per coefficient -> uint32 [N]; zs = ring_keys(p, keys)"""
    ct = words(np.asarray(ct).reshape(1 + p.k, p.N), p.W)
    with np.errstate(over="ignore"):
        ph = ct[0].copy()
        for i, zp in enumerate(zs):
            ph = ph + share(p, ct, zp, i)
    return ((ph & np.uint64((1 << p.W) - 1)) >> np.uint64(p.W - 32)).astype(np.uint32)


def lwe_phase(p, rows, lwekeys):
    """b + sum <a_i, s_i> of rows [B][lwe_len] -> uint32 [B]"""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, p.lwe_len)
    s = np.concatenate([np.asarray(k, dtype=np.uint32) for k in lwekeys])
    return (rows[:, -1] + (rows[:, :-1] * s).sum(-1, dtype=np.uint32)).astype(np.uint32)


def bit_of_phase(p, ph):
    ph = np.asarray(ph, dtype=np.uint32)
    if shape(p)[3]:
        return ph < (1 << 31)
    return ((ph >> 29) + ((ph >> 28) & 1)) == 1


def recomposed(p, a, l, logB):
    """32-bit mask words -> what the gadget keeps of them: sum_t digit_t 2^(32 - (t+1) logB) mod 2^32, uint32"""
    a = np.asarray(a, dtype=np.uint32)
    d = centered(O.decomp_poly(a.astype(np.uint64).reshape(-1), l, logB, 32), 32).reshape((l,) + a.shape)
    r = np.zeros(a.shape, dtype=np.int64)
    for t in range(l):
        r += d[t] << (32 - (t + 1) * logB)
    return (r & 0xFFFFFFFF).astype(np.uint32)


# ---- noise prediction ----
def predicted(p, l, logB, c, sigma_ring, hw=None):
    """-> (key-term variance, rounding-term variance) on the 32-bit torus; hw None: nparty n / 2"""
    nparty = shape(p)[0]
    key = nparty * p.n * l * c * (4.0 ** logB / 12.0) * sigma_ring ** 2 / 4.0 ** (p.W - 32)
    rnd = (nparty * p.n / 2.0 if hw is None else hw) * 4.0 ** (32 - l * logB) / 12.0 if l * logB < 32 else 0.0
    return key, rnd


def band_rounding(p, m, hw):
    """(band against the prediction at nparty n / 2, band against the keys' own hw)"""
    se = 5.0 * math.sqrt((3.0 - 1.2 / hw - 1.0) / (4.0 * m))
    return se + 2.5 / math.sqrt(shape(p)[0] * p.n), se


def band_key(p, l, logB, m, sigma_ring):
    terms = shape(p)[0] * p.n * l * p.N
    return 5.0 * math.sqrt(2.0 / (4.0 * m)) + 2.5 * math.sqrt(2.0 / terms) + 0.5 * (2.0 / 4.0 ** logB + 1.0 / (12.0 * sigma_ring ** 2))
