"""mkt_pack_batch in the life of one context (tests/context_life_cases.py holds the calls of mktfhe.h; this is the call of mktfhe_pack.h): one
context runs a gate batch, a pack, a gate batch of another size, a pack from device memory, is forked, and the fork packs.  Every result
equals the same call on a fresh context; gates after a pack equal gates without one (the pack keeps its own workspace)."""
import ctypes as C

import numpy as np
import pytest

from helpers import encrypt_bits, gpu_scheme, keygen, mk
from helpers import to_device as _dev

from mktfhe_amd import _lib

pytestmark = pytest.mark.gpu
L_PK, LOGB_PK = 4, 4


def _seed(n):
    buf = (C.c_uint8 * 32)()
    assert _lib.lib().mkt_client_test_seed(n, buf) == 0
    return bytes(buf)


def _fresh(p, crs, keys, pks):
    s = gpu_scheme(p, crs, keys)
    for i, pk in enumerate(pks):
        mk.load_packing_key(s, i, pk, L_PK, LOGB_PK)
    return s


def _once(p, crs, keys, pks, call):
    """`call` on a context that has done nothing else"""
    s = _fresh(p, crs, keys, pks)
    try:
        r = call(s)
        return r.cpu().numpy() if hasattr(r, "is_cuda") else np.array(r, copy=True)
    finally:
        s.close()


@pytest.mark.parametrize("p", [mk.KMS2party.scaled(n=16, N=256), mk.CGGIparam.scaled(n=20, N=256)], ids=lambda p: p.name)
def test_one_context_equals_fresh_ones(require_gpu, p):
    crs, keys = keygen(p, 9)
    pks = [mk.packing_keygen(keys[i], p, L_PK, LOGB_PK, deterministic_seed=_seed(20 + i)) for i in range(p.nparty)]
    bits = np.random.default_rng(2).integers(0, 2, 2 * (p.N + 9)).astype(bool)
    c = encrypt_bits(p, keys, bits, seed=300)
    x, y = c[0::2], c[1::2]
    steps = [
        ("gate, 7 rows", lambda s: s.gate(0, x[:7], y[:7])),
        ("pack, N + 9 host rows", lambda s: mk.pack(s, x)),
        ("gate, 33 rows", lambda s: s.gate(3, x[:33], y[:33])),
        ("pack, device rows picked by index", lambda s: mk.pack(s, _dev(y), _dev(np.arange(p.N + 2, dtype=np.uint32)[::-1].copy()))),
        ("gate, 5 rows on the device", lambda s: s.gate(1, _dev(x[:5]), _dev(y[:5]))),
    ]
    want = [_once(p, crs, keys, pks, call) for _, call in steps]
    one = _fresh(p, crs, keys, pks)
    for (name, call), w in zip(steps, want):
        r = call(one)
        got = r.cpu().numpy() if hasattr(r, "is_cuda") else r
        assert np.array_equal(got, w), name
    fork = one.fork()
    for who, s in (("fork", fork), ("parent after the fork", one)):
        assert np.array_equal(mk.pack(s, x), want[1]), who
        assert np.array_equal(s.gate(0, x[:7], y[:7]), want[0]), who
    fork.close()
    one.close()
