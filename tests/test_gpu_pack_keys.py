"""The seeded packing key on the GPU (mktfhe_amd/csrc/pack_keys.hip; include/mktfhe_pack.h "SEEDED"): the device expansion is the host's
(mkt_client_packing_key_expand, held to the definition in tests/test_pack_keys_cpu.py) word for word; a seeded load leaves the resident
state of mkt_load_packing_key fed with the host expansion, on both arithmetic modes; the bodies generated on the device are those of
mkt_client_packing_keygen_seeded word for word; device keygen -> version-3 blob -> an evaluator that never sees a secret -> gates -> pack ->
ring shares -> merge gives the plaintext bits; the refusals; the C example.  Every comparison is exact: one ChaCha20 block function and
wrapping integer arithmetic on both sides, the Gaussian deviate the shared box_muller with contraction off.

The shapes are the points where the kernels' indexing changes, not workload sizes.  The P / 2 refusal of an MKT_ARITH_EXACT context is not
reachable: N 2^(logB_pk - 1) 2^31 >= P / 2 ~ 2^59 needs N >= 8192 at logB_pk = 16, and the library admits N <= 4096."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ref_pack as RP
from helpers import GATE_FUNCS, ROOT, encrypt_bits, keygen, mk, secret_keys
from test_gpu_pack import F64_SETS, GADGETS, crafted_pool, seed_bytes

from mktfhe_amd import _lib
from mktfhe_amd import scheme as S

pytestmark = pytest.mark.gpu
FILL = 0xA5A5A5A5
MS = bytes(range(40, 72))                      # a public mask seed
ARG, UNSUPPORTED, STATE = -1, -2, -5
TILE = 256                                     # units (keystream blocks of 64 bytes) per tile of the expansion kernel
MAX_GRID = 2048                                # workgroups of one launch; more tiles than that: grid-stride


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _kr(p):
    return RP.shape(p)[1]


def units(p, l):
    """(units per polynomial, units of the whole expanded key): a unit is one keystream block, 64 bytes of output"""
    per = p.N * p.W // 512
    return per, p.n * l * (1 + _kr(p)) * per


def _bodies(p, l, seed):
    """expansion needs no key: any words serve as bodies"""
    b = np.random.default_rng(seed).integers(0, 2**63, (p.n, l, p.N), dtype=np.uint64)
    return b if p.W == 64 else (b & 0xFFFFFFFF).astype(np.uint32)


def _check_expansion(p, party, sch, l, logB, body):
    """host arrays, device tensors, and the raw call into 0xA5-filled allocations with 8 guard words behind the output"""
    import torch
    want = mk.packing_key_expand(p, party, l, logB, MS, body)
    got = mk.packing_key_expand(p, party, l, logB, MS, body, scheme=sch)
    assert isinstance(got, np.ndarray) and got.dtype == p.ring_dtype and np.array_equal(got, want), "host arrays"
    d = mk.packing_key_expand(p, party, l, logB, MS, _dev(body), scheme=sch)
    assert d.is_cuda and tuple(d.shape) == want.shape and np.array_equal(_host(d, p.ring_dtype), want), "device tensors"
    g = torch.full((want.size * (2 if p.W == 64 else 1) + 8,), FILL - 2**32, dtype=torch.int32, device="cuda")
    tb = _dev(body)
    assert _lib.lib().mkt_packing_key_expand(sch.h, party, l, logB, (C.c_uint8 * 32)(*MS), C.c_void_p(tb.data_ptr()), C.c_void_p(g.data_ptr()), S.MEM_DEVICE) == 0
    h = _host(g, np.uint32)
    assert np.array_equal(h[:-8].view(p.ring_dtype), want.reshape(-1)), "raw call"
    assert (h[-8:] == FILL).all(), "a word behind the output was written"


# (name, parameters, party, gadget, the tiling fact the shape is there for).  A polynomial is N W / 512 units; a group (b, a_0 ..) 1 + kr of them
EXPAND_SHAPES = [
    ("N32-w32-kr2", mk.CGGIparam.scaled(n=50, N=32, k=2), 0, (3, 5), "2 units per polynomial, groups of 6: 42 groups and 4 units per tile -- tile boundaries inside a (b, a) group; short last tile"),
    ("N32-w32-kr1", mk.CCS2party.scaled(n=33, N=32), 1, (3, 5), "2 units per polynomial, 64 groups per tile; short last tile"),
    ("N64-w64", mk.KMS2party.scaled(n=33, N=64), 1, (3, 5), "8 units per polynomial on the 64-bit ring, 16 groups per tile; short last tile"),
    ("N64-w32-kr3", mk.CGGIparam.scaled(n=17, N=64, k=3), 0, (4, 4), "groups of 4 polynomials: the body stride at kr = 3"),
    ("N256-w32", mk.CGGIparam.scaled(n=17, N=256), 0, (1, 16), "a polynomial of 16 units"),
    ("N256-w64", mk.KMS2party.scaled(n=17, N=256, k=3), 2, (4, 4), "a polynomial of 32 units; the last party of three"),
    ("N256-w32-kr2", mk.CGGIparam.scaled(n=5, N=256, k=2), 0, (8, 4), "groups of 3 polynomials of 16 units: 5 1/3 groups per tile"),
    ("N2048-w32", mk.CGGIparam.scaled(n=3, N=2048), 0, (3, 5), "a polynomial of 128 units: half a tile"),
    ("N2048-w64", mk.KMS2party.scaled(n=3, N=2048), 1, (3, 5), "a polynomial equals one tile"),
    ("lmss-N64", mk.Blockparam.scaled(n=18, N=64, blk_d=6), 0, (3, 5), "a block scheme"),
]
# whole tiles only, and a short last tile: both occur (a context exists for N = 32 .. 4096 only: 2 units are the fewest a polynomial has)
assert {units(c[1], c[3][0])[1] % TILE == 0 for c in EXPAND_SHAPES} == {True, False}
assert {units(c[1], c[3][0])[0] for c in EXPAND_SHAPES} == {2, 4, 8, 16, 32, 128, 256}


@pytest.mark.parametrize("case", EXPAND_SHAPES, ids=lambda v: v[0])
def test_device_expansion_equals_host_expansion(require_gpu, case):
    """mkt_packing_key_expand = mkt_client_packing_key_expand word for word, on a context that never sees a key, and it changes no resident
    table: a pack afterwards still answers MKT_ERR_STATE"""
    name, p, party, (l, logB), _ = case
    per, total = units(p, l)
    if name == "N32-w32-kr2":
        assert per == 2 and total > TILE and total % TILE and TILE % ((1 + _kr(p)) * per) != 0
    if name == "N2048-w64":
        assert per == TILE
    assert party == p.nparty - 1
    sch = mk.Scheme(p)
    _check_expansion(p, party, sch, l, logB, _bodies(p, l, 11))
    with pytest.raises(mk.MktError) as ei:
        mk.pack(sch, np.zeros((1, p.lwe_len), dtype=np.uint32))
    assert ei.value.code == STATE
    sch.close()


def test_grid_stride(require_gpu):
    """more tiles than the 2048 workgroups of one launch: the 64-bit ring at N = 2048 (a polynomial = one tile), n = 130, l_pk = 8, kr = 1:
    2080 tiles, 34 MB; the first 32 workgroups take a second tile"""
    p, l, logB = mk.KMS2party.scaled(n=130, N=2048), 8, 4
    per, total = units(p, l)
    assert per == TILE and total // TILE == 2080 > MAX_GRID and total % TILE == 0
    sch = mk.Scheme(p)
    body = _bodies(p, l, 6)
    want = mk.packing_key_expand(p, 1, l, logB, MS, body)
    assert want.nbytes == 2080 * TILE * 64
    got = mk.packing_key_expand(p, 1, l, logB, MS, _dev(body), scheme=sch)
    assert np.array_equal(_host(got, np.uint64), want)
    sch.close()


def test_expansion_refusals_leave_the_output_untouched(require_gpu):
    """a device pointer that is not 16-byte aligned -- input or output -- is MKT_ERR_ARG before anything is launched; so are a NULL mask
    seed, NULL pointers, a bad gadget, a party out of range and an unknown memory kind"""
    import torch
    p, l, logB = mk.KMS2party.scaled(n=3, N=64), 3, 5
    sch = mk.Scheme(p)
    L, seed = _lib.lib(), (C.c_uint8 * 32)(*MS)
    body = _bodies(p, l, 3)
    words = body.size * 2 * 2                                  # 32-bit words of the expanded key: 1 + kr = 2 polynomials of 64-bit words
    tb = torch.zeros(body.size * 2 + 8, dtype=torch.int32, device="cuda")
    tb[4:4 + body.size * 2] = _dev(body).view(torch.int32).reshape(-1)
    out = torch.full((words + 16,), FILL - 2**32, dtype=torch.int32, device="cuda")
    assert tb.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0

    def ex(party=1, ll=l, lb=logB, mseed=seed, src=tb.data_ptr() + 16, dst=out.data_ptr(), mem=S.MEM_DEVICE):
        return L.mkt_packing_key_expand(sch.h, party, ll, lb, mseed, C.c_void_p(src) if src else None, C.c_void_p(dst) if dst else None, mem)

    for kw in (dict(dst=out.data_ptr() + 8), dict(dst=out.data_ptr() + 4), dict(src=tb.data_ptr() + 8), dict(src=tb.data_ptr() + 24), dict(mseed=None),
               dict(src=0), dict(dst=0), dict(party=2), dict(party=-1), dict(ll=0), dict(lb=17), dict(ll=9, lb=4), dict(mem=7)):
        assert ex(**kw) == ARG, kw
        assert (_host(out, np.uint32) == FILL).all(), kw
    assert ex() == 0
    h = _host(out, np.uint32)
    assert np.array_equal(h[:words].view(np.uint64), mk.packing_key_expand(p, 1, l, logB, MS, body).reshape(-1)) and (h[words:] == FILL).all()
    sch.close()


# ---- mkt_load_packing_key_seeded ----
def _seeded_keys(p, l, logB, seed=71):
    """-> (secrets, [(mask seed, bodies)] per party, [host expansion] per party); every party its own mask seed"""
    keys = secret_keys(p, seed=seed)
    seeded = [mk.packing_keygen_seeded(keys[i], p, l, logB, mask_seed=seed_bytes(300 + i), deterministic_seed=seed_bytes(seed + 1 + i)) for i in range(p.nparty)]
    return keys, seeded, [mk.packing_key_expand(p, i, l, logB, *seeded[i]) for i in range(p.nparty)]


def _pack_words(p, arith, load, pool):
    """the words of one pack on a fresh context keyed by load(scheme): host arrays and device tensors"""
    sch = mk.Scheme(p, arith=arith)
    load(sch)
    got = mk.pack(sch, pool)
    dev = _host(mk.pack(sch, _dev(pool)), p.ring_dtype)
    sch.close()
    assert np.array_equal(got, dev)
    return got


LOAD_CASES = [(name, mk.ARITH_F64REF, GADGETS[i % 4]) for i, name in enumerate(sorted(F64_SETS))] + \
             [(name, mk.ARITH_EXACT, g) for name in ("cggi-n17", "kms-k2-n64", "cggi-k2-n3", "ccs-k2-n64", "cggi-k3-n17-N512") for g in ((4, 4), (3, 5))]


@pytest.mark.parametrize("name, arith, gadget", LOAD_CASES, ids=lambda v: v if isinstance(v, str) else ("exact" if v == 1 else "f64") if isinstance(v, int) else f"l{v[0]}-logB{v[1]}")
def test_seeded_load_leaves_the_state_of_the_host_expansion(require_gpu, name, arith, gadget):
    """pack words after mkt_load_packing_key_seeded = pack words after mkt_load_packing_key(host expansion) on a fresh context; the pool holds
    crafted_pool's edge words and makes two packs, the second ragged"""
    p = F64_SETS[name]
    if arith == mk.ARITH_EXACT:
        p = p.scaled(n=min(p.n, 17))
    l, logB = gadget
    keys, seeded, full = _seeded_keys(p, l, logB)
    pool = crafted_pool(p, p.N + 3, l, logB, np.random.default_rng(len(name)))
    want = _pack_words(p, arith, lambda s: [mk.load_packing_key(s, i, full[i], l, logB) for i in range(p.nparty)], pool)
    got = _pack_words(p, arith, lambda s: [mk.load_packing_key_seeded(s, i, *seeded[i], l, logB) for i in range(p.nparty)], pool)
    assert got.shape == (2, p.k + 1, p.N) and np.array_equal(got, want)


@pytest.mark.parametrize("arith", [mk.ARITH_F64REF, mk.ARITH_EXACT], ids=["f64", "exact"])
def test_one_party_seeded_and_another_unseeded(require_gpu, arith):
    p, (l, logB) = (F64_SETS["kms-k2-n64"] if arith == mk.ARITH_F64REF else F64_SETS["ccs-k2-n64"]).scaled(n=17), (4, 4)
    keys, seeded, full = _seeded_keys(p, l, logB)
    pool = crafted_pool(p, p.N + 1, l, logB, np.random.default_rng(4))
    want = _pack_words(p, arith, lambda s: [mk.load_packing_key(s, i, full[i], l, logB) for i in range(2)], pool)
    got = _pack_words(p, arith, lambda s: (mk.load_packing_key(s, 0, full[0], l, logB), mk.load_packing_key_seeded(s, 1, *seeded[1], l, logB)), pool)
    assert np.array_equal(got, want)
    got = _pack_words(p, arith, lambda s: (mk.load_packing_key_seeded(s, 1, *seeded[1], l, logB), mk.load_packing_key(s, 0, full[0], l, logB)), pool)
    assert np.array_equal(got, want)


def test_seeded_load_refusals_leave_the_packs_unchanged(require_gpu):
    """a second gadget, NULL pointers, a party out of range, a bad gadget: MKT_ERR_ARG; after fork: MKT_ERR_STATE; RLWE length 4:
    MKT_ERR_UNSUPPORTED.  After each refusal the pack gives the words it gave before"""
    p, (l, logB) = F64_SETS["kms-k2-n64"].scaled(n=5), (4, 4)
    keys, seeded, full = _seeded_keys(p, l, logB)
    _, other, _ = _seeded_keys(p, 2, 4)
    L, ptr = _lib.lib(), S._np_ptr
    u8 = lambda b: (C.c_uint8 * 32)(*b)      # noqa: E731
    pool = crafted_pool(p, p.N, l, logB, np.random.default_rng(2))
    sch = mk.Scheme(p)
    body = [np.ascontiguousarray(s[1]) for s in seeded]
    raw = lambda party=1, ms=u8(seeded[1][0]), b=body[1], ll=l, lb=logB, s=sch: L.mkt_load_packing_key_seeded(s.h, party, ms, None if b is None else ptr(b), ll, lb)   # noqa: E731
    mk.load_packing_key_seeded(sch, 0, *seeded[0], l, logB)
    with pytest.raises(mk.MktError) as ei:
        mk.pack(sch, pool)
    assert ei.value.code == STATE, "MKT_ERR_STATE until every party has loaded"
    for kw in (dict(ll=2, lb=4, b=np.ascontiguousarray(other[1][1])), dict(ms=None), dict(b=None), dict(party=2), dict(party=-1), dict(ll=3, lb=11), dict(ll=0), dict(lb=17)):
        assert raw(**kw) == ARG, kw
    with pytest.raises(mk.MktError) as ei:
        mk.pack(sch, pool)
    assert ei.value.code == STATE, "a refused load marks nothing"
    assert raw() == 0
    want = mk.pack(sch, pool)
    assert np.array_equal(want, _pack_words(p, mk.ARITH_F64REF, lambda s: [mk.load_packing_key(s, i, full[i], l, logB) for i in range(2)], pool))
    for kw in (dict(ll=2, lb=4, b=np.ascontiguousarray(other[1][1])), dict(ms=None), dict(party=2)):
        assert raw(**kw) == ARG and np.array_equal(mk.pack(sch, pool), want), kw
    fork = sch.fork()
    junk = np.zeros_like(body[0])
    for s in (sch, fork):
        assert raw(party=0, ms=u8(MS), b=junk, s=s) == STATE, "the key set is immutable once shared"
        with pytest.raises(mk.MktError) as ei:
            mk.packing_keygen_device(s, 0, keys[0], l, logB, mask_seed=MS, install=True)
        assert ei.value.code == STATE
    assert np.array_equal(mk.pack(sch, pool), want) and np.array_equal(mk.pack(fork, pool), want)
    fork.close(); sch.close()
    q = mk.CGGIparam.scaled(n=3, N=64, k=4)                    # RLWE length 4: 5 polynomials per row
    sq = mk.Scheme(q)
    bq = _bodies(q, l, 1)
    assert L.mkt_load_packing_key_seeded(sq.h, 0, u8(MS), ptr(bq), l, logB) == UNSUPPORTED
    assert L.mkt_load_packing_key(sq.h, 0, ptr(np.zeros((q.n, l, 5, q.N), dtype=np.uint32)), l, logB) == UNSUPPORTED, "the refusal of the unseeded load"
    assert np.array_equal(mk.packing_key_expand(q, 0, l, logB, MS, bq, scheme=sq), mk.packing_key_expand(q, 0, l, logB, MS, bq)), "expansion serves any RLWE length"
    sq.close()


# ---- mkt_packing_keygen_device ----
BIG = 2.0 ** 55
# (name, parameters, party, gadget, sigma_ring or None for the set's own).  N = 256 = the workgroup; 1024: the last size with 4 accumulators
# per lane; 2048: 16.  KMS: the ring key is mkt_client_ringkey index 1; CCS: key 0; CGGI k = 2, 3: keys 0 .. k - 1
KEYGEN_SHAPES = [
    ("cggi-N64", mk.CGGIparam.scaled(n=5, N=64), 0, (3, 5), None),
    ("cggi-k2-N256", mk.CGGIparam.scaled(n=3, N=256, k=2), 0, (1, 16), BIG),
    ("cggi-k3-N512", mk.CGGIparam.scaled(n=3, N=512, k=3), 0, (3, 5), None),
    ("cggi-N1024", mk.CGGIparam.scaled(n=3, N=1024), 0, (3, 5), BIG),
    ("cggi-N2048", mk.CGGIparam.scaled(n=2, N=2048), 0, (1, 16), None),
    ("lmss-N256", mk.Blockparam.scaled(n=6, N=256, blk_len=3, blk_d=2), 0, (3, 5), None),
    ("kms-N64", mk.KMS2party.scaled(n=4, N=64), 1, (3, 5), None),
    ("kms3-N256", mk.KMS2party.scaled(n=3, N=256, k=3), 2, (1, 16), BIG),
    ("kms-N512", mk.KMS2party.scaled(n=3, N=512), 0, (3, 5), BIG),
    ("kms-N1024", mk.KMS2party.scaled(n=2, N=1024), 0, (3, 5), None),
    ("kms-N2048", mk.KMS2party.scaled(n=2, N=2048), 1, (3, 5), BIG),
    ("kmsblock-N256", mk.KMS2partyblock.scaled(n=6, N=256, blk_len=3, blk_d=2), 1, (1, 16), None),
    ("ccs-N512", mk.CCS2party.scaled(n=3, N=512), 1, (3, 5), None),
    ("ccs3-N64", mk.CCS2party.scaled(n=3, N=64, k=3), 2, (1, 16), BIG),
]


@pytest.mark.parametrize("case", KEYGEN_SHAPES, ids=lambda v: v[0])
def test_device_keygen_equals_host_keygen(require_gpu, case):
    """mkt_packing_keygen_device = mkt_client_packing_keygen_seeded for the same seed, word for word, noise included (at sigma = 2^55 every
    noise word carries the deviate's whole mantissa).  install = 0: a context that never saw a key serves the call and no resident table
    changes -- a pack afterwards still answers MKT_ERR_STATE"""
    name, p, party, (l, logB), sigma = case
    if sigma is not None:
        p = p.scaled(beta=sigma)
    key = secret_keys(p, seed=83)[party]
    sd = seed_bytes(500 + len(name))
    ms, want = mk.packing_keygen_seeded(key, p, l, logB, mask_seed=MS, deterministic_seed=sd)
    sch = mk.Scheme(p)
    ms2, got = mk.packing_keygen_device(sch, party, key, l, logB, mask_seed=MS, deterministic_seed=sd)
    assert ms2 == ms == MS and got.shape == want.shape == (p.n, l, p.N) and got.dtype == p.ring_dtype
    bad = np.nonzero((got != want).reshape(p.n * l, -1).any(axis=1))[0]
    assert not len(bad), (name, "rows (q l + t) that differ", bad[:8])
    with pytest.raises(mk.MktError) as ei:
        mk.pack(sch, np.zeros((1, p.lwe_len), dtype=np.uint32))
    assert ei.value.code == STATE
    a, b = (mk.packing_keygen_device(sch, party, key, 1, 16, mask_seed=MS)[1] for _ in range(2))
    assert not np.array_equal(a, b), "a NULL seed must draw fresh entropy per call"
    sch.close()


@pytest.mark.parametrize("name, arith", [("kms-k2-n64", mk.ARITH_F64REF), ("cggi-k2-n3", mk.ARITH_F64REF), ("cggi-k2-n3", mk.ARITH_EXACT), ("ccs-k2-n64", mk.ARITH_EXACT)],
                         ids=lambda v: v if isinstance(v, str) else ("exact" if v else "f64"))
def test_device_keygen_with_install_gives_the_packs_of_the_host_path(require_gpu, name, arith):
    """install = 1: the bodies are expanded and installed where they were made; the packs are those of a context fed the host generator's
    key through the host expansion and mkt_load_packing_key, and the returned bodies are the host's"""
    p, (l, logB) = F64_SETS[name].scaled(n=min(F64_SETS[name].n, 17)), (4, 4)
    keys = secret_keys(p, seed=71)
    sds = [seed_bytes(72 + i) for i in range(p.nparty)]
    host = [mk.packing_keygen_seeded(keys[i], p, l, logB, mask_seed=seed_bytes(300 + i), deterministic_seed=sds[i]) for i in range(p.nparty)]
    pool = crafted_pool(p, p.N + 3, l, logB, np.random.default_rng(9))
    want = _pack_words(p, arith, lambda s: [mk.load_packing_key(s, i, mk.packing_key_expand(p, i, l, logB, *host[i]), l, logB) for i in range(p.nparty)], pool)
    made = []
    got = _pack_words(p, arith, lambda s: made.extend(mk.packing_keygen_device(s, i, keys[i], l, logB, mask_seed=host[i][0], deterministic_seed=sds[i], install=True)
                                                      for i in range(p.nparty)), pool)
    assert np.array_equal(got, want)
    for i in range(p.nparty):
        assert made[i][0] == host[i][0] and np.array_equal(made[i][1], host[i][1]), i


def test_device_keygen_refusals_write_nothing_and_touch_no_table(require_gpu):
    """every refusal is MKT_ERR_ARG with the pre-filled output as it was, on a context whose packs keep their words"""
    p, q, (l, logB) = F64_SETS["kms-k2-n64"].scaled(n=5), mk.CCS2party.scaled(n=5, N=256), (4, 4)
    keys, foreign = secret_keys(p, seed=71), secret_keys(q, seed=71)
    L, ptr = _lib.lib(), S._np_ptr
    u8 = lambda b: (C.c_uint8 * 32)(*b)      # noqa: E731
    ms, sd = u8(MS), u8(seed_bytes(8))
    out = np.full((p.n, 8, p.N), FILL, dtype=p.ring_dtype)
    empty, loaded = mk.Scheme(p), mk.Scheme(p)
    _, seeded, full = _seeded_keys(p, l, logB)
    for i in range(2):
        mk.load_packing_key_seeded(loaded, i, *seeded[i], l, logB)
    pool = crafted_pool(p, 5, l, logB, np.random.default_rng(2))
    want = mk.pack(loaded, pool)
    for sch in (empty, loaded):
        gen = lambda party=0, k=keys[0], ll=l, lb=logB, seed=sd, mseed=ms, o=out, install=0: L.mkt_packing_keygen_device(   # noqa: E731
            sch.h, party, None if k is None else k.h, ll, lb, seed, mseed, None if o is None else ptr(o), install)
        for install in (0, 1):
            for kw in (dict(mseed=None), dict(seed=ms), dict(seed=u8(MS)), dict(ll=0), dict(lb=0), dict(lb=17), dict(ll=9, lb=4), dict(ll=3, lb=11), dict(ll=-1),
                       dict(party=2), dict(party=-1), dict(party=1), dict(k=keys[1]), dict(k=foreign[0]), dict(k=None)):
                assert gen(install=install, **kw) == ARG, (kw, install)
        assert gen(o=None, install=0) == ARG, "install = 0 with a NULL output"
        if sch is loaded:
            assert gen(ll=2, lb=4, install=1) == ARG, "a second gadget"
            assert np.array_equal(mk.pack(loaded, pool), want), "a refused call touches no table"
        else:
            with pytest.raises(mk.MktError) as ei:
                mk.pack(empty, pool)
            assert ei.value.code == STATE, "a refused call touches no table"
        assert (out == FILL).all(), "a refused call writes nothing"
    with pytest.raises(mk.MktError):
        mk.packing_keygen_device(empty, 0, keys[0], l, logB, mask_seed=MS, deterministic_seed=MS)
    with pytest.raises(ValueError):
        mk.packing_keygen_device(empty, 0, keys[0], 9, 4, mask_seed=MS)
    empty.close(); loaded.close()


# ---- end to end ----
@pytest.mark.parametrize("p", [mk.KMS2party.scaled(n=16, N=256), mk.CGGIparam.scaled(n=20, N=256)], ids=lambda p: p.name)
def test_device_keygen_to_blob_to_evaluator_to_merged_bits(require_gpu, p):
    """every party makes its packing key on its own context (which holds no key) and ships a version-3 blob; the evaluator is keyed from blobs
    alone -- it never sees a secret --, computes NANDs, packs them; one ring share per party, merged, equals the plaintext bits.  Zero wrong
    bits are required: the condition at the top of tests/test_pack_cpu.py (these two sets, gadget (4, 4), N = 256 rows per pack: a margin of
    more than 2000 deviations of the pack error) holds for a seeded key, whose noise law is the same sigma_ring"""
    N, l, logB = p.N, 4, 4
    crs, keys = keygen(p, 5)
    blobs = ([mk.keyblob.dump_crs(p, crs)] if p.multikey else []) + [mk.keyblob.dump_party(k) for k in keys]
    for i in range(p.nparty):
        own = mk.Scheme(p)
        ms, body = mk.packing_keygen_device(own, i, keys[i], l, logB)
        own.close()
        blobs.append(mk.keyblob.dump_packing_key_seeded(p, i, l, logB, ms, body))
        assert blobs[-1][:8] == mk.keyblob.MAGIC3 and len(blobs[-1]) < 0.51 * (p.n * l * (1 + RP.shape(p)[1]) * N * p.W // 8) + 512
    ev = mk.Scheme(p)
    for b in blobs:
        mk.keyblob.load_into(ev, b)
    B = N + 3
    bits = np.random.default_rng(8).integers(0, 2, 2 * B).astype(bool)
    c = encrypt_bits(p, keys, bits, seed=500)
    packed = mk.pack(ev, mk.NAND(_to_dev32(c[0::2]), _to_dev32(c[1::2]), ev))
    assert packed.is_cuda and tuple(packed.shape) == (2, p.k + 1, N)
    shares = [mk.rlwe_partial_decrypt(packed, keys[i], p, i, 2.0 ** 20, deterministic_seed=60 + i) for i in range(p.nparty)]
    got = np.concatenate([mk.rlwe_merge_decrypt(packed[g], [s[g] for s in shares], p) for g in range(2)])[:B]
    assert np.array_equal(got, GATE_FUNCS[0](bits[0::2], bits[1::2])), "wrong bits after device keygen, blob, pack, shares and merge"
    ev.close()


def _to_dev32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def test_c_example_through_the_abi(require_gpu, tmp_path):
    """examples/seeded_packing_key.c: device keygen on the parties' contexts, seeded load on the evaluator, gates, pack, shares and merge from
    plain C (gcc, no Python)"""
    exe = str(tmp_path / "seeded_packing_key")
    lib = os.path.join(ROOT, "mktfhe_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "seeded_packing_key.c"),
                           "-o", exe, "-L" + lib, "-lmktfhe_hip", "-Wl,-rpath," + lib])
    out = subprocess.run([exe, "24", "256"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith("OK"), out.stdout + out.stderr
