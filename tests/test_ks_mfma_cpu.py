"""The host side of the key switch on the matrix cores (mktfhe_amd/csrc/ks_mfma.h, host_internal.h), without a GPU: the packer of the signed
byte planes against numpy, the overflow bound at its edge, and how MKT_KS_MFMA is read."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mktfhe_amd import _lib  # noqa: E402


def L():
    lib = _lib.lib()
    lib.mkt_internal_ks_mfma_block_bytes.restype, lib.mkt_internal_ks_mfma_block_bytes.argtypes = C.c_size_t, [C.c_int] * 3
    lib.mkt_internal_ks_mfma_pack_host.restype, lib.mkt_internal_ks_mfma_pack_host.argtypes = None, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]
    lib.mkt_internal_ks_mfma_fits.restype, lib.mkt_internal_ks_mfma_fits.argtypes = C.c_int, [C.c_longlong] * 3
    lib.mkt_internal_ks_mfma_env.restype, lib.mkt_internal_ks_mfma_env.argtypes = C.c_int, []
    return lib


def signed_bytes(w):
    """w (uint32 array) -> (4, ...) int64 with w = sum_b s_b 256^b mod 2^32, every s_b in [-128, 127]"""
    w = w.astype(np.int64)
    out = []
    for _ in range(4):
        s = ((w & 0xFF) ^ 0x80) - 0x80
        out.append(s)
        w = ((w - s) & 0xFFFFFFFF) >> 8
    return np.stack(out)


def planes_numpy(rows, N, f, drows, n1p):
    """[step][tile of 32 words][plane][lane][16]: lane = 32 h + r holds, for word 32 tile + r, k = 16 h + e with k = 4 (digit in step) + d,
    digit s = 8 step + 4 h + e // 4 = j f + t, d = e % 4 the row (0: the all-zero row)"""
    steps, tiles = (N * f + 7) // 8, (n1p + 31) // 32
    key = rows.reshape(N, drows, f, n1p)
    sb = signed_bytes(key)                                        # [plane][j][d - 1][t][q]
    out = np.zeros((steps, tiles, 4, 64, 16), dtype=np.int8)
    for step in range(steps):
        for lane in range(64):
            r, h = lane & 31, lane >> 5
            for e in range(16):
                s, d = 8 * step + 4 * h + e // 4, e % 4
                if d == 0 or d > drows or s >= N * f:
                    continue
                j, t = divmod(s, f)
                for tile in range(tiles):
                    q = 32 * tile + r
                    if q < n1p:
                        out[step, tile, :, lane, e] = sb[:, j, d - 1, t, q]
    return out


@pytest.mark.parametrize("N,f,n1p", [(32, 2, 12), (32, 3, 12), (16, 8, 36), (16, 5, 32)])
def test_host_packer_against_numpy(N, f, n1p):
    rng = np.random.default_rng(N + f + n1p)
    rows = rng.integers(0, 2**32, (N * 3 * f, n1p), dtype=np.uint64).astype(np.uint32)
    rows[:8] = np.array([0, 0x80, 0x7F, 0xFF, 0x8000, 0x80808080, 0xFFFFFFFF, 0x7F7F7F7F], dtype=np.uint32)[:, None]     # carries through every plane
    lib = L()
    nbytes = lib.mkt_internal_ks_mfma_block_bytes(N, f, n1p)
    want = planes_numpy(rows, N, f, 3, n1p)
    assert nbytes == want.size
    got = np.empty(nbytes, dtype=np.int8)
    lib.mkt_internal_ks_mfma_pack_host(rows.ctypes.data, N, f, 3, n1p, got.ctypes.data)
    assert np.array_equal(got.reshape(want.shape), want)


def test_signed_bytes_rebuild_every_word():
    w = np.concatenate([np.arange(0, 2**32, 65537, dtype=np.uint64), [0x80, 0x8000, 0x800000, 0x80000000, 0xFFFFFFFF, 0x7FFFFFFF, 0x80808080]]).astype(np.uint32)
    s = signed_bytes(w)
    assert s.min() >= -128 and s.max() <= 127
    assert np.array_equal(sum(s[b] << (8 * b) for b in range(4)) & 0xFFFFFFFF, w.astype(np.int64))


def test_overflow_bound_at_its_edge():
    fits = L().mkt_internal_ks_mfma_fits
    edge = (2**31 - 1) // 255                                     # the largest N kr f with N kr f 255 < 2^31
    assert edge * 255 < 2**31 <= (edge + 1) * 255
    assert fits(edge, 1, 1) == 1 and fits(edge + 1, 1, 1) == 0
    assert fits(1, edge, 1) == 1 and fits(1, 1, edge + 1) == 0
    assert fits(4096, 64, 32) == 1 and fits(4096, 64, 33) == 0   # 4096 * 64 * 32 = 8 388 608 <= edge = 8 421 504 < 4096 * 64 * 33
    assert fits(1024, 1, 8) == 1 and fits(2048, 2, 8) == 1        # the headline, KMS2party
    assert fits(0, 1, 1) == 0 and fits(1, 0, 1) == 0 and fits(1, 1, -1) == 0


def test_switch_as_the_launcher_reads_it(monkeypatch):
    """MKT_KS_MFMA goes through the env_int every launcher switch goes through (mkt_internal_ks_mfma_env reads it again with the same call);
    the launch-shape rule asks only `!= 0` (planes kept, kernel admitted) and `> 0` (at every batch)"""
    env = L().mkt_internal_ks_mfma_env
    monkeypatch.delenv("MKT_KS_MFMA", raising=False)
    assert env() == -1                                            # unset: automatic
    for text, want in (("-1", -1), ("0", 0), ("1", 1), ("2", 2), ("-7", -7), (" 1", 1), ("", 0), ("off", 0)):      # atoi: no digits read as 0
        monkeypatch.setenv("MKT_KS_MFMA", text)
        assert env() == want, text
