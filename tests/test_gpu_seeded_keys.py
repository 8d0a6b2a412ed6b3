"""Seeded evaluation keys on the GPU (mkt_seeded_keys_expand / mkt_load_seeded_keys, mktfhe_amd/csrc/seeded_keys.hip): the device words are
the host's (mkt_client_seeded_keys_expand, held to the definition in tests/test_seeded_keys_cpu.py) word for word -- one stream_block on both
sides, copies elsewhere, so equality is exact -- at the shapes where the kernels' indexing changes; a scheme loaded from seeded keys computes
the words of a scheme that received the host-expanded keys through load_party, on both arithmetic modes; a version-2 blob serves a shipped
set end to end; forks refuse the load; the multi-device evaluator and the C example run."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from helpers import GATE_FUNCS, ROOT, encrypt_bits, gpu_scheme, mk, oracle_scheme
from test_seeded_keys_cpu import MS, SHAPES, seeded_party

pytestmark = pytest.mark.gpu
FILL = 0xA5A5A5A5

# beside the host tests' shapes (n in {1, 3, 15, 16, 17, 33}: n + 1 equal to the padded pitch at n = 3 and 15, different elsewhere; N in
# {32, 64, 256}; both ring widths; RLWE lengths 1 .. 3; UniEnc; block shapes): N = 2048 on both ring widths
EXPAND_SHAPES = SHAPES + [("cggi-n17-N2048", mk.CGGIparam.scaled(n=17, N=2048), 0), ("kms-n3-N2048", mk.KMS2party.scaled(n=3, N=2048), 1),
                          ("ccs-n3-N2048", mk.CCS2party.scaled(n=3, N=2048), 0)]


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _random_sections(p, seed):
    """expansion needs no key: any words serve as bodies"""
    rng = np.random.default_rng(seed)
    wb, wk = mk.seeded_section_words(p)
    b = rng.integers(0, 2**63, wb, dtype=np.uint64)
    return (b if p.W == 64 else (b & 0xFFFFFFFF).astype(np.uint32)), rng.integers(0, 2**32, wk, dtype=np.uint64).astype(np.uint32)


def _check_expansion(p, party, sch, bs, ks):
    """host arrays, device tensors, and the raw call into 0xA5-filled allocations with guard words behind both outputs"""
    import torch
    from mktfhe_amd import _lib
    want_b, want_k = mk.seeded_keys_expand(p, party, MS, bs, ks)
    got_b, got_k = mk.seeded_keys_expand(p, party, MS, bs, ks, scheme=sch)
    assert isinstance(got_b, np.ndarray) and np.array_equal(got_b, want_b) and np.array_equal(got_k, want_k), "host arrays"
    db, dk = mk.seeded_keys_expand(p, party, MS, _dev(bs), _dev(ks), scheme=sch)
    assert db.is_cuda and dk.is_cuda and np.array_equal(_host(db, p.ring_dtype), want_b) and np.array_equal(_host(dk, np.uint32), want_k), "device tensors"
    only_k = mk.seeded_keys_expand(p, party, MS, ksk_seeded=_dev(ks), scheme=sch)
    assert only_k[0] is None and np.array_equal(_host(only_k[1], np.uint32), want_k)
    only_b = mk.seeded_keys_expand(p, party, MS, brk_seeded=bs, scheme=sch)
    assert only_b[1] is None and np.array_equal(only_b[0], want_b)
    gb = torch.full((want_b.size * (2 if p.W == 64 else 1) + 8,), FILL - 2**32, dtype=torch.int32, device="cuda")
    gk = torch.full((want_k.size + 8,), FILL - 2**32, dtype=torch.int32, device="cuda")
    tb, tk = _dev(bs), _dev(ks)
    seed = (C.c_uint8 * 32)(*MS)
    assert _lib.lib().mkt_seeded_keys_expand(sch.h, party, seed, C.c_void_p(tb.data_ptr()), C.c_void_p(tk.data_ptr()), C.c_void_p(gb.data_ptr()),
                                             C.c_void_p(gk.data_ptr()), 0) == 0
    hb, hk = _host(gb, np.uint32), _host(gk, np.uint32)
    assert np.array_equal(hb[:-8].view(p.ring_dtype), want_b) and np.array_equal(hk[:-8], want_k.ravel())
    assert (hb[-8:] == FILL).all() and (hk[-8:] == FILL).all(), "a word behind an output was written"


@pytest.mark.parametrize("case", EXPAND_SHAPES, ids=lambda v: v[0])
def test_device_expansion_equals_host_expansion(require_gpu, case):
    """mkt_seeded_keys_expand = mkt_client_seeded_keys_expand word for word, on a context that never sees a key"""
    _, p, party = case
    sch = mk.Scheme(p)
    _check_expansion(p, party, sch, *_random_sections(p, 11))
    sch.close()


def test_grid_stride(require_gpu):
    """a launch has at most 2048 workgroups of 256 units (one keystream block each).  Key-switching key: n = 3 (one unit per row),
    3 * 2048 * 31 * 6 = 1 142 784 rows > 2 * 2048 * 256: every workgroup takes a third tile.  Bootstrapping key: 64-bit ring, N = 2048 (256
    units per polynomial), n = 172: 172 * 12 * 256 = 528 384 units > 2048 * 256"""
    p = mk.CGGIparam.scaled(n=3, N=2048, k=3, f=6, logD=5)
    wb, wk = mk.seeded_section_words(p)
    assert wk > 2 * 2048 * 256
    sch = mk.Scheme(p)
    ks = np.random.default_rng(5).integers(0, 2**32, wk, dtype=np.uint64).astype(np.uint32)
    want = mk.seeded_keys_expand(p, 0, MS, ksk_seeded=ks)[1]
    assert np.array_equal(_host(mk.seeded_keys_expand(p, 0, MS, ksk_seeded=_dev(ks), scheme=sch)[1], np.uint32), want)
    sch.close()
    q = mk.KMS2party.scaled(n=172, N=2048)
    assert 172 * 12 * 256 > 2048 * 256
    sch = mk.Scheme(q)
    bs = np.random.default_rng(6).integers(0, 2**63, mk.seeded_section_words(q)[0], dtype=np.uint64)
    want = mk.seeded_keys_expand(q, 1, MS, brk_seeded=bs)[0]
    assert np.array_equal(_host(mk.seeded_keys_expand(q, 1, MS, brk_seeded=_dev(bs), scheme=sch)[0], np.uint64), want)
    sch.close()


def _seeded_set(p, seed=77):
    """(crs, [seeded PartyKeys], [(brk, ksk) host-expanded]) of every party"""
    out = [seeded_party(p, i, seed=seed) for i in range(p.nparty)]
    return out[0][0], [o[1] for o in out], [(o[2], o[3]) for o in out]


def _plain_scheme(p, crs, keys, expanded, arith=mk.ARITH_F64REF):
    """the host-expanded keys through the existing load_party"""
    sch = mk.Scheme(p, arith=arith)
    if p.multikey:
        sch.load_crs(crs)
    for i, (k, (brk, ksk)) in enumerate(zip(keys, expanded)):
        sch.load_party(i, brk=brk, ksk=ksk, rlk_d=k.rlk_d, rlk_f=k.rlk_f, pubkey=k.pubkey)
    return sch


GATE_SETS = [(mk.CGGIparam.scaled(n=16, N=256), mk.ARITH_F64REF), (mk.Blockparam.scaled(n=18, N=256, blk_d=6), mk.ARITH_F64REF),
             (mk.CCS2party.scaled(n=12, N=256), mk.ARITH_F64REF), (mk.KMS2party.scaled(n=17, N=256), mk.ARITH_F64REF),
             (mk.KMS2partyblock.scaled(n=12, N=256, blk_d=4), mk.ARITH_F64REF),
             (mk.CGGIparam.scaled(n=16, N=256), mk.ARITH_EXACT), (mk.KMS2party.scaled(n=16, N=256), mk.ARITH_EXACT)]


@pytest.mark.parametrize("p, arith", GATE_SETS, ids=lambda v: v.name if hasattr(v, "name") else ("exact" if v else "f64"))
def test_a_seeded_scheme_computes_the_words_of_the_expanded_keys(require_gpu, p, arith):
    """setup() with seeded PartyKeys (mkt_load_seeded_keys) against a Scheme fed the host-expanded keys through load_party: get_ksk is the
    host-expanded key, 8 NANDs and a table bootstrap are bit-identical (the resident tables are the same), "fx_available" agrees; the
    NANDs decrypt"""
    crs, keys, expanded = _seeded_set(p)
    want_s = _plain_scheme(p, crs, keys, expanded, arith)
    got_s = gpu_scheme(p, crs, keys, arith=arith)
    for i in range(p.nparty):
        assert np.array_equal(got_s.get_ksk(i), expanded[i][1]), i
    bits = np.random.default_rng(2).integers(0, 2, 16).astype(bool)
    c = encrypt_bits(p, keys, bits, seed=500)
    want, got = mk.NAND(c[:8], c[8:], want_s), mk.NAND(c[:8], c[8:], got_s)
    assert np.array_equal(got, want)
    assert np.array_equal(mk.lwe_decrypt(got, keys if p.multikey else keys[0], p), GATE_FUNCS[0](bits[:8], bits[8:]))
    lut = mk.sign_lut(p)
    assert np.array_equal(mk.lut_bootstrap(got_s, lut, c[:1]), mk.lut_bootstrap(want_s, lut, c[:1]))
    if arith == mk.ARITH_EXACT:
        assert got_s.get_metric("fx_available") == want_s.get_metric("fx_available")
        assert got_s.get_metric("fx_kmax") == want_s.get_metric("fx_kmax") > 0.0 and got_s.get_metric("fx_bound") == want_s.get_metric("fx_bound")
    # one section at a time gives the same tables
    one = mk.Scheme(p, arith=arith)
    mk.load_seeded(one, 0, mask_seed=MS, ksk_seeded=keys[0].ksk_seeded)
    assert np.array_equal(one.get_ksk(0), expanded[0][1])
    one.close(); want_s.close(); got_s.close()


class _Expanded:
    """a seeded party's secrets and small keys, with the two large keys as expanded on the host"""

    def __init__(self, party, brk, ksk):
        self._s, self.brk, self.ksk = party, brk, ksk

    def __getattr__(self, name):
        return getattr(self._s, name)


def _neg(c):
    return (0 - c.astype(np.int64)).astype(np.uint32)


def _reference_row(p, arith, crs, keys, op, x, y):
    """one gate_ops row under `keys`: the CPU oracle (Float64 reference) or its exact-arithmetic restatement (tests/ref_exact.py)"""
    import ref_exact as RX
    so = oracle_scheme(p, crs, keys)
    x, y = _neg(x) if op & mk.OP_NOT_X else x, _neg(y) if op & mk.OP_NOT_Y else y
    if arith == mk.ARITH_F64REF:
        return so.gate(op & 7, x, y)
    if p.scheme == mk.KMS:
        return RX.kms_gate(p, so, keys, crs, op & 7, x, y)
    return RX.gate(p, so, keys[0].brk, op & 7, x, y)


@functools.lru_cache(maxsize=None)
def _unseeded_set(p, seed):
    """([party_keygen's PartyKeys], [the same parties' secrets and small keys only]) of every party, under the CRS of _seeded_set"""
    crs = mk.CRS(p, seed) if p.multikey else None
    return [mk.party_keygen(crs, p, party=i, deterministic_seed=seed) for i in range(p.nparty)], \
        [mk.party_keygen(crs, p, party=i, secrets_only=True, deterministic_seed=seed) for i in range(p.nparty)]


# one party set per scheme family at the shapes tests/test_gpu_keygen.py judges exported keys at, in the Float64 reference; CGGI and KMS also
# in MKT_ARITH_EXACT, where the key set keeps the limb transforms of the bootstrapping key and (KMS, 64-bit ring) the split residue tables
ROUTE_SETS = [(mk.CGGIparam.scaled(n=16), mk.ARITH_F64REF), (mk.Blockparam.scaled(n=18, blk_d=6), mk.ARITH_F64REF), (mk.CCS2party.scaled(n=20), mk.ARITH_F64REF),
              (mk.KMS2party.scaled(n=16), mk.ARITH_F64REF), (mk.CGGIparam.scaled(n=16), mk.ARITH_EXACT), (mk.KMS2party.scaled(n=16), mk.ARITH_EXACT)]


@pytest.mark.parametrize("p, arith", ROUTE_SETS, ids=lambda v: v.name if hasattr(v, "name") else ("exact" if v else "f64"))
def test_three_routes_leave_one_resident_state(require_gpu, p, arith):
    """The three ways a party's large keys become resident -- host upload (load_party), device generation (keygen_device), seeded load
    (mkt_load_seeded_keys) -- end in one install path; contexts keyed by different routes with the same keys hold the same state: get_ksk of
    every party word for word, "fx_kmax" bit for bit (> 0 on the MKT_ARITH_EXACT sets, which keep the limb transforms), and the words of one
    gate_ops batch of 8 rows (row j under party j mod nparty, so the last party and, as every gate reads every polynomial of every party's
    key, the last polynomial of a party's stride are met).
    One key set cannot go through all three: the device generator makes the words of party_keygen, a seeded party's large keys come from
    other streams (test_secrets_and_small_keys_are_those_of_the_unseeded_keygen).  So, secrets and small keys from one seed throughout:
    device generation against an upload of party_keygen's keys, which are also the resident key-switching key (the rule of
    tests/test_gpu_keygen.py: the device's words are the host's); the seeded load against an upload of the host-expanded keys, and rows 0 and
    7 of that pair against the CPU oracle (the EXACT sets: row 7 against tests/ref_exact.py)"""
    seed = 77
    crs, seeded, expanded = _seeded_set(p, seed)
    host, secrets = _unseeded_set(p, seed)
    rng = np.random.default_rng(3)
    c = encrypt_bits(p, host, rng.integers(0, 2, 16).astype(bool), seed=900)
    ops = (rng.integers(0, 6, 8) | rng.choice([0, mk.OP_NOT_X, mk.OP_NOT_Y, mk.OP_NOT_X | mk.OP_NOT_Y], 8)).astype(np.uint8)

    def state(s):
        out = [s.get_ksk(i) for i in range(p.nparty)], s.get_metric("fx_kmax"), s.gate_ops(ops, c[:8], c[8:])
        s.close()
        return out

    def same(a, b, what):
        for i in range(p.nparty):
            assert np.array_equal(a[0][i], b[0][i]), (what, "key-switching key of party", i)
        assert a[1] == b[1] and (a[1] > 0.0) == (arith == mk.ARITH_EXACT), (what, "fx_kmax", a[1], b[1])
        assert np.array_equal(a[2], b[2]), (what, "gate_ops rows that differ", np.nonzero((a[2] != b[2]).any(axis=1))[0])

    uploaded = state(gpu_scheme(p, crs, host, arith=arith))
    same(state(gpu_scheme(p, crs, secrets, arith=arith)), uploaded, "device generation against upload")
    for i in range(p.nparty):
        assert np.array_equal(uploaded[0][i].ravel(), host[i].ksk), i
    uploaded = state(_plain_scheme(p, crs, seeded, expanded, arith))
    same(state(gpu_scheme(p, crs, seeded, arith=arith)), uploaded, "seeded load against upload")
    keys = [_Expanded(k, *e) for k, e in zip(seeded, expanded)]
    for i in range(p.nparty):
        assert np.array_equal(uploaded[0][i], expanded[i][1]), i
    for j in ((0, 7) if arith == mk.ARITH_F64REF else (7,)):
        assert np.array_equal(uploaded[2][j], _reference_row(p, arith, crs, keys, int(ops[j]), c[j], c[8 + j])), ("reference, row", j)


def test_a_shipped_set_from_a_version_2_blob(require_gpu):
    """CGGIparam end to end: the party dumps a version-2 blob, the evaluator loads it (keyblob.load_into -> mkt_load_seeded_keys), the four
    NAND inputs decrypt correctly"""
    p = mk.CGGIparam
    k = mk.party_keygen_seeded(None, p, deterministic_seed=9)
    blob = mk.keyblob.dump_party(k)
    wb, wk = mk.seeded_section_words(p)
    assert len(blob) < 32 + 4 * (wb + wk) + 1024 and 5 * len(blob) < 4 * (2 * wb + wk * (p.n + 1))      # a fifth of the full key
    sch = mk.Scheme(p)
    assert mk.keyblob.load_into(sch, blob) == 0
    x, y = np.array([0, 0, 1, 1], dtype=bool), np.array([0, 1, 0, 1], dtype=bool)
    c = encrypt_bits(p, [k], np.concatenate([x, y]), seed=40)
    assert np.array_equal(mk.lwe_decrypt(mk.NAND(c[:4], c[4:], sch), k, p), ~(x & y))
    sch.close()


def test_forks_refuse_and_bad_arguments(require_gpu):
    """after fork() the key set is immutable: load_seeded is MKT_ERR_STATE; through the raw ABI a NULL mask seed, a party out of range, a
    section without its output and an unknown memory kind are MKT_ERR_ARG and leave the outputs as they were; expansion needs no key on
    either arithmetic mode"""
    from mktfhe_amd import _lib, scheme as S
    p = mk.KMS2party.scaled(n=16, N=256)
    crs, keys, expanded = _seeded_set(p)
    sg = gpu_scheme(p, crs, keys)
    f = sg.fork()
    for s in (sg, f):
        with pytest.raises(mk.MktError) as ei:
            mk.load_seeded(s, 0, keys[0])
        assert ei.value.code == -5
    f.close(); sg.close()
    L, seed = _lib.lib(), (C.c_uint8 * 32)(*MS)
    bs, ks = np.ascontiguousarray(keys[1].brk_seeded), np.ascontiguousarray(keys[1].ksk_seeded)
    for arith in (mk.ARITH_F64REF, mk.ARITH_EXACT):
        sch = mk.Scheme(p, arith=arith)
        ob, ok = np.full(expanded[1][0].size, FILL, dtype=np.uint64), np.full(expanded[1][1].shape, FILL, dtype=np.uint32)

        def ex(party=1, mseed=seed, b=bs, k=ks, outb=ob, outk=ok, mem=S.MEM_HOST):
            ptr = lambda v: None if v is None else S._np_ptr(v)      # noqa: E731
            return L.mkt_seeded_keys_expand(sch.h, party, mseed, ptr(b), ptr(k), ptr(outb), ptr(outk), mem)

        for kw in (dict(mseed=None), dict(party=-1), dict(party=2), dict(outb=None), dict(k=None), dict(mem=7)):
            assert ex(**kw) == -1 and (ob == FILL).all() and (ok == FILL).all(), kw
        assert L.mkt_load_seeded_keys(sch.h, 1, None, S._np_ptr(bs), S._np_ptr(ks)) == -1 and L.mkt_load_seeded_keys(sch.h, 1, seed, None, None) == -1
        assert ex() == 0 and np.array_equal(ob, expanded[1][0]) and np.array_equal(ok, expanded[1][1])
        with pytest.raises(mk.MktError) as ei:
            sch.gate(0, np.zeros((1, p.lwe_len), np.uint32), np.zeros((1, p.lwe_len), np.uint32))
        assert ei.value.code == -5
        sch.close()


def test_multi_device_evaluator_takes_seeded_keys(require_gpu):
    """setup_multi(devices=[0, 0]) with seeded keys (mkt_multi_load_seeded_keys, then replication) gives the single-context words"""
    p = mk.KMS2party.scaled(n=16, N=256)
    crs, keys, expanded = _seeded_set(p)
    single = _plain_scheme(p, crs, keys, expanded)
    multi = mk.setup_multi(p, [0, 0], keys=keys, a=crs)
    c = encrypt_bits(p, keys, np.random.default_rng(4).integers(0, 2, 16).astype(bool), seed=700)
    assert np.array_equal(multi.gate(0, c[:8], c[8:]), single.gate(0, c[:8], c[8:]))
    multi.close(); single.close()


def test_c_example_through_the_abi(require_gpu, tmp_path):
    """examples/seeded_keys.c: parties write compact keys, the evaluator loads them and runs NAND, the result decrypts (gcc, no Python)"""
    exe = str(tmp_path / "seeded_keys")
    lib = os.path.join(ROOT, "mktfhe_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "seeded_keys.c"),
                           "-o", exe, "-L" + lib, "-lmktfhe_hip", "-Wl,-rpath," + lib])
    out = subprocess.run([exe, "24", "256", str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
