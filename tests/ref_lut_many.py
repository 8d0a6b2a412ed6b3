"""numpy restatement of the many-table bootstrap (include/mktfhe.h "many-table bootstrap"): the coarse mod-switch sw_nu, the
packed table, the extraction E_v at coefficient v, and the checker chain sw_nu -> table step -> blindrotate! -> E_v -> keyswitch!."""
import numpy as np

import ref_lut as R

NOUT = (1, 2, 4, 8)


def nu_of(nout):
    assert nout in NOUT
    return nout.bit_length() - 1


def sw(w, N, nout):
    """sw_nu(w) = divbits32(w, 32 - (logN + 1) + nu) << nu: a multiple of nout in [0, 2N]"""
    nu = nu_of(nout)
    return R.divbits32(w, 32 - (N.bit_length() - 1) - 1 + nu) << nu


def sw_row(lwe, N, nout):
    """every word of one ciphertext -> (atilde (k*n,) uint32, btilde)"""
    v = [sw(w, N, nout) for w in np.asarray(lwe).ravel()]
    return np.array(v[:-1], dtype=np.uint32), v[-1]


def sw_edge_words(N, nout):
    """the 32-bit words at the rounding edges of sw_nu: around every kind of half-way point (2m + 1) 2^(bit - 1) -- the first, one in the
    middle, the last, which rounds up to 2N -- and 0 and 0xFFFFFFFF"""
    bit = 32 - (N.bit_length() - 1) - 1 + nu_of(nout)
    half = 1 << (bit - 1)
    cells = (2 * N) // nout
    out = [0, 0xFFFFFFFF]
    for m in (0, 1, cells // 2 - 1, cells // 2, cells - 2, cells - 1):
        mid = (2 * m + 1) * half
        out += [mid - 1, mid, mid + 1]
    return [w & 0xFFFFFFFF for w in out]


def pack(tables):
    """U[o i + v] = T_v[o i]: (o, N) -> (N,)"""
    t = np.asarray(tables)
    o, N = t.shape
    assert o in NOUT and o <= N
    U = np.empty(N, dtype=t.dtype)
    for i in range(N // o):
        for v in range(o):
            U[o * i + v] = t[v][o * i]
    return U


def extract(acc, v, W):
    """E_v(acc) = X^-v acc on every polynomial: out[c][i] = acc[c][i + v] for i + v < N, else -acc[c][i + v - N] (mod 2^W).  acc (..., N) of
    W-bit words in any unsigned dtype -> uint64"""
    a = np.asarray(acc).astype(np.uint64)
    N = a.shape[-1]
    mask = np.uint64((1 << W) - 1)
    out = np.roll(a, -v, axis=-1)
    if v:
        out[..., N - v:] = (np.uint64(0) - out[..., N - v:]) & mask
    return out


def extract_all(acc, nout, W):
    """acc (B, 1 + k, N) -> (B, nout, 1 + k, N) uint64"""
    return np.stack([extract(acc, v, W) for v in range(nout)], axis=1)


def checker_many(so, U, lwe, nout, W):
    """the many-table bootstrap of ONE ciphertext on the CPU checker: so.modswitch replaced by sw_nu, then the table step, so.blindrotate,
    E_v and so.keyswitch -> (nout, lwe_len) uint32"""
    N = len(U)
    at, bt = sw_row(lwe, N, nout)
    acc = so.blindrotate(at, R.testvector(U, bt, W, so.kacc))
    return np.stack([so.keyswitch(extract(acc, v, W)) for v in range(nout)])     # (the checker holds W-bit words in uint64)


# ---- recipe (a) of DESIGN.md 1c: a full adder of three fresh inputs at scale 1/16 in one rotation ----
def adder_linear(x, y, z):
    """x + y + z + 1/32 on the b word: the sum s = 0 .. 3 in sixteenths sits in the middle of window s of P = 8"""
    lin = x.astype(np.int64) + y.astype(np.int64) + z.astype(np.int64)
    lin[:, -1] += R.CENTRE
    return (lin & 0xFFFFFFFF).astype(np.uint32)


def adder_values(W):
    """-> (sum, carry) window values for P = 8: window s -> +-2^(W-3) for s & 1 and s >> 1 (windows 4 .. 7 are never met: s <= 3)"""
    e = 1 << (W - 3)
    return [e if s & 1 else -e for s in range(8)], [e if (s >> 1) & 1 else -e for s in range(8)]
