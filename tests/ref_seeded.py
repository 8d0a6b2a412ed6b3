"""numpy restatement of the seeded-ciphertext definition (include/mktfhe.h "seeded ciphertexts"): the ChaCha20 block function of RFC 8439,
the mask words of a row, the body word given the noise word, and the expansion.  It never calls the library; chacha20_block is pinned to
RFC 8439 2.3.2's test vector in tests/test_seeded_cpu.py before anything is compared with it."""
import numpy as np

STREAM_ENC_MASK, STREAM_ENC_NOISE = 10, 11
_M = np.uint32(0xFFFFFFFF)


def _rotl(v, c):
    return ((v << np.uint32(c)) | (v >> np.uint32(32 - c))) & _M


def _qr(x, a, b, c, d):
    x[a] = x[a] + x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = x[c] + x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = x[a] + x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = x[c] + x[d]; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_block(key, counter, nonce):
    """RFC 8439 2.3: key 8 words, nonce 3 words; counter a word or an array of words (one block each) -> uint32 (..., 16)"""
    counter = np.atleast_1d(np.asarray(counter, dtype=np.uint32))
    s = [np.full(counter.shape, v, dtype=np.uint32) for v in (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574, *key, 0, *nonce)]
    s[12] = counter.copy()
    x = [v.copy() for v in s]
    with np.errstate(over="ignore"):
        for _ in range(10):
            _qr(x, 0, 4, 8, 12); _qr(x, 1, 5, 9, 13); _qr(x, 2, 6, 10, 14); _qr(x, 3, 7, 11, 15)
            _qr(x, 0, 5, 10, 15); _qr(x, 1, 6, 11, 12); _qr(x, 2, 7, 8, 13); _qr(x, 3, 4, 9, 14)
        return np.stack([a + b for a, b in zip(x, s)], axis=-1)


def seed_key(seed):
    """the 32 seed bytes as eight little-endian words"""
    return [int(w) for w in np.frombuffer(bytes(seed), dtype="<u4")]


def mask_row(mask_seed, party, row, n):
    """the n mask words of logical row `row` of party `party`: word q = word q & 15 of block q >> 4 of the row's stream"""
    nonce = [(STREAM_ENC_MASK & 0xFFFF) | (party << 16), row & 0xFFFFFFFF, row >> 32]
    return chacha20_block(seed_key(mask_seed), np.arange((n + 15) // 16), nonce).reshape(-1)[:n]


def body_word(mask, lwekey, mu, e=0):
    """e - <a, s> + mu in wrapping 32-bit arithmetic"""
    dot = int((mask.astype(np.uint64) * np.asarray(lwekey, dtype=np.uint64)).sum() & np.uint64(0xFFFFFFFF))
    return (int(e) - dot + int(mu)) & 0xFFFFFFFF


def expand(mask_seed, party, row0, body, n, nparty):
    """rows [B][nparty n + 1]: zeros, the mask in block `party`, the body last"""
    out = np.zeros((len(body), nparty * n + 1), dtype=np.uint32)
    for j in range(len(body)):
        out[j, party * n:(party + 1) * n] = mask_row(mask_seed, party, (row0 + j) & (2**64 - 1), n)
        out[j, -1] = body[j]
    return out
