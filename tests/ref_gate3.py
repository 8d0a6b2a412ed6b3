"""numpy restatement of the three-input linear parts (include/mktfhe.h MKT_MAJ3 .. MKT_AE3, flags MKT_OP_NOT_X / _Y / _Z), 32-bit
wrap: what the engine feeds to bootstrapping! for a three-input gate.  Independent of the HIP kernel; shared by the CPU and GPU tests."""
import numpy as np

MASK = 0xFFFFFFFF
# truth by number of true inputs (0, 1, 2, 3), per code
TRUTH = {0: (0, 0, 1, 1), 1: (1, 1, 0, 0), 2: (0, 1, 0, 1), 3: (1, 0, 1, 0), 4: (0, 1, 1, 0), 5: (1, 0, 0, 1)}


def linear3(code, x, y, z):
    """x, y, z: uint32 arrays [..., len] (b word last) -> the linear part of gate `code` (uint32, same shape)"""
    v = [np.asarray(u, dtype=np.uint32).astype(np.int64) for u in (x, y, z)]
    for i, flag in enumerate((8, 16, 32)):
        if code & flag:
            v[i] = -v[i]
    s = v[0] + v[1] + v[2]
    b = np.zeros(s.shape, dtype=np.int64)
    g = code & 7
    if g == 0:
        r = s
    elif g == 1:
        r = -s
    elif g == 2:
        r = -2 * s
    elif g == 3:
        r = 2 * s
    elif g == 4:
        b[..., -1] = 1 << 30
        r = s + b
    else:
        b[..., -1] = 3 << 30
        r = b - s
    return (r & MASK).astype(np.uint32)


def linear3_rows(ops, x, y, z):
    """one code per row"""
    return np.stack([linear3(int(ops[j]), x[j], y[j], z[j]) for j in range(len(ops))])


def oracle_gate3(so, ops, x, y, z):
    """the expected words: the oracle's bootstrapping! (bootstrapping.jl:4-27) of the restated linear part, row by row"""
    lin = linear3_rows(ops, x, y, z)
    return np.stack([so.bootstrap(lin[j]) for j in range(len(ops))])


def plain3(ops, bx, by, bz):
    """plaintext truth of coded three-input gates (NOT flags applied to the inputs first)"""
    out = np.empty(len(ops), dtype=bool)
    for j, o in enumerate(ops):
        a = bool(bx[j]) ^ bool(o & 8)
        b = bool(by[j]) ^ bool(o & 16)
        c = bool(bz[j]) ^ bool(o & 32)
        out[j] = bool(TRUTH[int(o & 7)][a + b + c])
    return out
