"""numpy restatement of the mask rules and index formulas of the seeded evaluation keys (include/mktfhe.h "seeded evaluation keys"): which
keystream word every mask word of the key-switching key and every mask coefficient of the bootstrapping key is, the compact section sizes,
and the expansion into the ordinary layouts.  Built on ref_seeded.chacha20_block (pinned to RFC 8439 by tests/test_seeded_cpu.py); it never
calls the library."""
import numpy as np

from ref_seeded import chacha20_block, seed_key

STREAM_KSK_MASK, STREAM_BRK_MASK = 12, 13
CGGI, LMSS, CCS, KMS, KMS_BLOCK = range(5)


def shape(p):
    """(nparty, kr, key-switch ring components kk, key-switch digit rows Drows)"""
    mkey = p.scheme in (CCS, KMS, KMS_BLOCK)
    D = 1 << p.logD
    return (p.k if mkey else 1), (1 if p.scheme in (KMS, KMS_BLOCK) else p.k), (1 if mkey else p.k), (D // 2 if p.scheme in (LMSS, KMS_BLOCK) else D - 1)


def _blocks(mask_seed, stream, party, idx, nblk):
    """keystream blocks 0 .. nblk - 1 of the streams (stream, party, idx[...]) -> uint32 [len(idx)][nblk * 16]"""
    idx = np.asarray(idx, dtype=np.uint64).reshape(-1)
    lo = np.repeat((idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), nblk)
    hi = np.repeat((idx >> np.uint64(32)).astype(np.uint32), nblk)
    ctr = np.tile(np.arange(nblk, dtype=np.uint32), idx.size)
    return chacha20_block(seed_key(mask_seed), ctr, [np.uint32(stream | (party << 16)), lo, hi]).reshape(idx.size, nblk * 16)


def ksk_masks(p, mask_seed, party):
    """[kk][N][Drows][f][n] mask words: word q of row R = ((c N + j) Drows + d) f + t is word q & 15 of block q >> 4 of stream (12, party, R)"""
    _, _, kk, dr = shape(p)
    rows = kk * p.N * dr * p.f
    return _blocks(mask_seed, STREAM_KSK_MASK, party, np.arange(rows), (p.n + 15) // 16)[:, :p.n].reshape(kk, p.N, dr, p.f, p.n)


def ksk_live(p):
    """[kk][N]: False for the rows (c, j) a block scheme leaves out (c N + j < n)"""
    _, _, kk, _ = shape(p)
    cj = np.arange(kk)[:, None] * p.N + np.arange(p.N)[None, :]
    return cj >= p.n if p.scheme in (LMSS, KMS_BLOCK) else np.ones((kk, p.N), dtype=bool)


def brk_mask_polys(p, mask_seed, party, P):
    """mask polynomials P[...] of stream 13 -> ring words [len(P)][N]: 32-bit ring: coefficient q = word q & 15 of block q >> 4; 64-bit ring:
    coefficient q = w[2 (q & 7)] | w[2 (q & 7) + 1] << 32 of block q >> 3"""
    if p.W == 32:
        return _blocks(mask_seed, STREAM_BRK_MASK, party, P, p.N // 16)
    w = _blocks(mask_seed, STREAM_BRK_MASK, party, P, p.N // 8).astype(np.uint64)
    return w[:, 0::2] | (w[:, 1::2] << np.uint64(32))


def brk_masks(p, mask_seed, party):
    """RGSW: [n][(kr+1) l][kr][N], polynomial index P = (i rows + c l + j) kr + cc; CCS: [n][l][N], P = i l + j"""
    _, kr, _, _ = shape(p)
    if p.scheme == CCS:
        return brk_mask_polys(p, mask_seed, party, np.arange(p.n * p.l_uni)).reshape(p.n, p.l_uni, p.N)
    rows = (kr + 1) * p.l_gsw
    return brk_mask_polys(p, mask_seed, party, np.arange(p.n * rows * kr)).reshape(p.n, rows, kr, p.N)


def section_words(p):
    """(ring words of brk_seeded, words of ksk_seeded)"""
    _, kr, kk, dr = shape(p)
    brk = p.n * (2 * p.l_uni if p.scheme == CCS else (kr + 1) * p.l_gsw) * p.N
    return brk, kk * p.N * dr * p.f


def expand(p, mask_seed, party, brk_seeded, ksk_seeded):
    """-> (brk, ksk) in the layouts of mkt_load_brk (integer form) and mkt_load_ksk"""
    _, kr, kk, dr = shape(p)
    dt = np.uint64 if p.W == 64 else np.uint32
    a = brk_masks(p, mask_seed, party).astype(dt)
    if p.scheme == CCS:
        l = p.l_uni
        body = np.asarray(brk_seeded, dtype=dt).reshape(p.n, 2 * l, p.N)
        brk = np.empty((p.n, 3 * l, p.N), dtype=dt)
        brk[:, :l] = body[:, :l]
        brk[:, l::2] = body[:, l:]
        brk[:, l + 1::2] = a
    else:
        rows = (kr + 1) * p.l_gsw
        brk = np.empty((p.n, rows, kr + 1, p.N), dtype=dt)
        brk[:, :, 0] = np.asarray(brk_seeded, dtype=dt).reshape(p.n, rows, p.N)
        brk[:, :, 1:] = a
    ksk = np.zeros((kk, p.N, dr, p.f, p.n + 1), dtype=np.uint32)
    ksk[..., :p.n] = ksk_masks(p, mask_seed, party)
    ksk[..., p.n] = np.asarray(ksk_seeded, dtype=np.uint32).reshape(kk, p.N, dr, p.f)
    ksk[~ksk_live(p)] = 0
    return brk.reshape(-1), ksk.reshape(-1, p.n + 1)
