"""numpy restatement of the seeded packing key (include/mktfhe_pack.h "SEEDED"): which keystream word every mask coefficient is (stream 19,
the gadget in the high word of the stream index), the bodies with their noise from stream 20, and the expansion into the ordinary layout.
Built on ref_seeded.chacha20_block (pinned to RFC 8439 by tests/test_seeded_cpu.py), ref_seeded_keys._blocks and the deviate of ref_pack; it
never calls the library."""
import numpy as np

import ref_pack as RP
from ref_keys import ring_mul
from ref_seeded_keys import _blocks

STREAM_PACK_MASK, STREAM_PACK_NOISE = 19, 20


def mask_index(P, l, logB):
    """stream index of mask polynomial P: P | (l | logB << 8) << 32"""
    return np.asarray(P, dtype=np.uint64) | np.uint64((l | (logB << 8)) << 32)


def masks(p, mask_seed, party, l, logB):
    """[n][l][kr][N] uint64: polynomial P = (q l + t) kr + c.  32-bit ring: coefficient j = word j & 15 of block j >> 4; 64-bit ring: coefficient
    j = w[2 (j & 7)] | w[2 (j & 7) + 1] << 32 of block j >> 3"""
    kr = RP.shape(p)[1]
    idx = mask_index(np.arange(p.n * l * kr), l, logB)
    if p.W == 32:
        a = _blocks(mask_seed, STREAM_PACK_MASK, party, idx, p.N // 16).astype(np.uint64)
    else:
        w = _blocks(mask_seed, STREAM_PACK_MASK, party, idx, p.N // 8).astype(np.uint64)
        a = w[:, 0::2] | (w[:, 1::2] << np.uint64(32))
    return a.reshape(p.n, l, kr, p.N)


def bodies(p, lwekey, zs, party, l, logB, seed, mask_seed, sigma_ring):
    """[n][l][N] uint64: b = -sum_c a_c (*) z_c + e + s[q] 2^(W - (t + 1) logB) X^0, e the first N noise draws of stream (20, party, q, t)
    keyed by `seed`.  zs: the party's ring keys as mkt_client_ringkey numbers them"""
    _, kr, zoff, _ = RP.shape(p)
    N, W = p.N, p.W
    mask = (1 << W) - 1
    a = masks(p, mask_seed, party, l, logB)
    out = np.zeros((p.n, l, N), dtype=np.uint64)
    for q in range(p.n):
        for t in range(l):
            b = np.zeros(N, dtype=np.uint64)
            with np.errstate(over="ignore"):
                for c in range(kr):
                    b = b - ring_mul(a[q, t, c], zs[zoff + c], W)
            e = RP.noise_words(RP.draws(seed, party, STREAM_PACK_NOISE, q, t, 2 * N), sigma_ring)
            bb = [(int(b[j]) + e[j]) & mask for j in range(N)]
            bb[0] = (bb[0] + (int(lwekey[q]) << (W - (t + 1) * logB))) & mask
            out[q, t] = np.array(bb, dtype=np.uint64)
    return out


def expand(p, mask_seed, party, l, logB, pk_seeded):
    """-> [n][l][1 + kr][N] uint64, the layout of mkt_load_packing_key: (b, a_0 ..)"""
    kr = RP.shape(p)[1]
    out = np.empty((p.n, l, 1 + kr, p.N), dtype=np.uint64)
    out[:, :, 0] = np.asarray(pk_seeded).astype(np.uint64).reshape(p.n, l, p.N)
    out[:, :, 1:] = masks(p, mask_seed, party, l, logB)
    return out
