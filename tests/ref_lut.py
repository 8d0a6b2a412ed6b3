"""numpy restatement of the programmable bootstrap's table step (include/mktfhe.h "programmable bootstrap"; the semantics are the
reference's own bootstrap, tfhe/bootstrapping.jl:4-27, with an arbitrary test vector): the rotated accumulator, the table layout of
lut_poly, the gather front end's linear combination, and the checker chain modswitch -> testvector -> blindrotate -> keyswitch."""
import numpy as np


def rotate(T, bt, W):
    """X^bt * T in Z_{2^W}[X]/(X^N + 1) for bt in [0, 2N] -> (N,) uint64 holding W-bit words.  With r = bt mod N and s = -1 for
    N <= bt < 2N, else +1:  out[i] = s T[i - r] for i >= r, -s T[N + i - r] for i < r; bt = 2N is the identity"""
    T = np.asarray(T).astype(np.uint64)
    N, mask = T.size, (1 << W) - 1
    bt = int(bt)
    assert 0 <= bt <= 2 * N
    r, s = bt % N, (-1 if N <= bt < 2 * N else 1)
    out = np.empty(N, dtype=np.uint64)
    for i in range(N):
        v = s * int(T[i - r]) if i >= r else -s * int(T[N + i - r])
        out[i] = v & mask
    return out


def testvector(T, bt, W, kacc):
    """(X^bt * T, 0, ..., 0): (1 + kacc, N) uint64"""
    acc = np.zeros((1 + kacc, np.asarray(T).size), dtype=np.uint64)
    acc[0] = rotate(T, bt, W)
    return acc


def lut_poly(values, N, W):
    """T[0] = values[0], T[j] = -values[floor((N - j) P / N)] for j >= 1"""
    P, mask = len(values), (1 << W) - 1
    assert N % P == 0
    return np.array([int(values[0]) & mask] + [(-int(values[(N - j) * P // N])) & mask for j in range(1, N)], dtype=np.uint64)


def extracted(T, phi, W):
    """coefficient 0 of X^phi * T as the header documents it, phi in [0, 2N)"""
    N, mask = len(T), (1 << W) - 1
    if phi == 0:
        return int(T[0])
    return (-int(T[N - phi])) & mask if phi <= N else int(T[2 * N - phi])


def divbits32(w, bit):
    """arithmetic.jl:23-27 on a 32-bit word"""
    w = int(w) & 0xFFFFFFFF
    return w if bit <= 0 else ((w >> bit) + ((w >> (bit - 1)) & 1)) & 0xFFFFFFFF


def btilde(body, N):
    return divbits32(body, 32 - (N.bit_length() - 1) - 1)


def linear(pool, idx, wt, cst):
    """lin[g] = cst[g] on the b word + sum_t wt[g][t] pool[idx[g][t]], mod 2^32 (weight 0: no term; rows clamped into the pool)"""
    pool = np.asarray(pool, dtype=np.uint32)
    out = np.zeros((len(cst), pool.shape[1]), dtype=np.int64)
    for g in range(len(cst)):
        for t in range(4):
            if int(wt[g][t]):
                out[g] += int(wt[g][t]) * pool[min(int(idx[g][t]), pool.shape[0] - 1)].astype(np.int64)
        out[g, -1] += int(cst[g])
    return (out & 0xFFFFFFFF).astype(np.uint32)


def checker_bootstrap(so, T, lwe, W):
    """the programmable bootstrap of ONE ciphertext on the CPU checker: its modswitch, the table step above, its blindrotate! and keyswitch!"""
    at, bt = so.modswitch(lwe)
    acc = so.blindrotate(at, testvector(T, bt, W, so.kacc))
    return so.keyswitch(acc)


# ---- recipes of DESIGN.md 1.2 ----
SCALE16 = 1 << 28          # 1/16 of the 32-bit torus: one input step of the three-input recipe
CENTRE = 1 << 27           # 1/32: puts the sum x + 2y + 4z (in sixteenths) in the middle of window v = x + 2y + 4z of P = 8


def truth_values(table, W):
    """table[v] for v = x + 2y + 4z -> the 8 window values +-2^(W-3): the output is an ordinary gate bit"""
    e = 1 << (W - 3)
    return [e if table[v] else -e for v in range(8)]


TRUTH_TABLES = {
    "AND3": [int(v == 7) for v in range(8)],
    "OR3": [int(v != 0) for v in range(8)],
    "x?y:z": [((v >> 1) & 1) if (v & 1) else ((v >> 2) & 1) for v in range(8)],
    "random": [int(b) for b in np.random.default_rng(20261017).integers(0, 2, 8)],
}


def truth_inputs(p, keys, mk, seed):
    """the 8 input combinations as fresh encryptions at scale 1/16 (bit b -> message b / 16), party j mod nparty -> (x, y, z): (8, lwe_len) each"""
    rows = [[], [], []]
    for v in range(8):
        for t in range(3):
            i = (v + t) % p.nparty
            rows[t].append(mk.lwe_encrypt_word(((v >> t) & 1) * SCALE16, i, keys[i], p, deterministic_seed=seed + 3 * v + t))
    return [np.stack(r) for r in rows]


def truth_linear(x, y, z):
    """x + 2y + 4z + 1/32 on the b word"""
    lin = (x.astype(np.int64) + 2 * y.astype(np.int64) + 4 * z.astype(np.int64))
    lin[:, -1] += CENTRE
    return (lin & 0xFFFFFFFF).astype(np.uint32)


# the sets of the whole-construction tests (CPU: on the checker alone; GPU: the same inputs, the same words): the shipped CGGI and
# two-party KMS sets, with their own noise
CHAIN_SETS = ("CGGIparam", "KMS2party")


def chain_case(p, seed=61):
    """-> (crs, keys, x, y, z): pinned keys and the 8 input combinations of the three-input recipe"""
    from helpers import keygen, mk
    crs, keys = keygen(p, seed)
    return (crs, keys) + tuple(truth_inputs(p, keys, mk, 6100))
