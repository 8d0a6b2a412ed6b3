"""The seeded key form generated on the party's own GPU (mkt_keygen_device_seeded, mktfhe_amd/csrc/keygen_seeded.hip) against the host
generator (mkt_client_party_keygen_seeded) word for word -- BOTH compact sections -- at every shape where the kernels' indexing changes:
N below one workgroup (idle lanes), both accumulator instantiations, both widths of the mask words, several ring keys, every UniEnc depth,
block schemes with absent rows and n > N, the edges of the key-switching mask's keystream blocks, every key-switch gadget, more rows than
one launch holds, two parties of one seed.  The same comparison at sigma = 2^55 sees every bit of the Gaussian deviate
(tests/test_gpu_keygen.py says why).  Then the device-made sections of one set per scheme, expanded on the host, go through the independent
opener and statistics of tests/ref_keys.py, so the judgement does not rest on client.cpp.  install=1 leaves the resident state of
load_seeded; install=0 and every refusal leave a loaded scheme alone; the C example runs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, encrypt_bits, mk

pytestmark = pytest.mark.gpu
FILL = 0xA5A5A5A5
MS = bytes(range(60, 92))                      # a public mask seed

_RING = {32: mk.CGGIparam, 64: mk.KMS2party}          # an RGSW scheme on each ring width
_GADGETS = ((8, 2), (5, 3), (4, 3), (6, 5))
SHAPES = (
    # N = 32 .. 4096 on both rings: N < 256 leaves lanes idle, N <= 1024 takes the 4-register accumulator, N > 1024 the 16-register one;
    # a mask polynomial is N / 16 keystream blocks on the 32-bit ring and N / 8 on the 64-bit one
    [_RING[W].scaled(n=3, N=N) for W in (32, 64) for N in (32, 64, 128, 256, 1024, 2048, 4096)] + [
        mk.CGGIparam.scaled(n=3, N=256, k=2), mk.CGGIparam.scaled(n=3, N=256, k=3), mk.CGGIparam.scaled(n=2, N=256, k=5),     # kr ring keys: m_c = z_{c-1}
        mk.CGGIparam.scaled(n=2, N=2048, k=3),
        mk.CCS2party.scaled(n=3, N=256), mk.CCS2party.scaled(n=3, N=2048), mk.CCS2party.scaled(n=3, N=32),                  # UniEnc depths
        mk.CCS8party.scaled(n=3, N=512), mk.CCS16party.scaled(n=3, N=128), mk.CCS16party.scaled(n=2, N=4096, k=2),
        mk.KMS32party.scaled(n=2, N=256), mk.KMS4party.scaled(n=3, N=512),                                                  # other gadget depths
        mk.Blockparam.scaled(n=150, N=64, k=3, blk_d=50), mk.Blockparam.scaled(n=12, N=256, blk_d=4),                        # absent rows, n > N
        mk.KMS2partyblock.scaled(n=12, N=256, blk_d=4), mk.KMS2partyblock.scaled(n=30, N=32, blk_d=10),
    ] + [mk.CGGIparam.scaled(n=n, N=64) for n in (1, 15, 16, 17, 33)]                                                        # key-switch mask block edges
    + [q.scaled(f=f, logD=logD) for (f, logD) in _GADGETS                                                                    # key-switch gadgets
       for q in (mk.CGGIparam.scaled(n=3, N=128), mk.Blockparam.scaled(n=6, N=128, blk_d=2), mk.KMS2party.scaled(n=3, N=64))]
    + [mk.CGGIparam.scaled(n=2, N=4096, k=2)])                                                                               # 196 608 rows > 2048 workgroups * 64


def _id(p):
    return f"{p.name}-n{p.n}-N{p.N}-k{p.k}-W{p.W}-f{p.f}x{p.logD}"


def _same_words(got, want, what, p, party):
    """got == want word for word, or: the set and the party, the section, the first differing word with both words in hex, and how many differ"""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.dtype == want.dtype and got.size == want.size, (what, _id(p), "party", party, got.dtype, got.size, want.dtype, want.size)
    bad = np.nonzero(got != want)[0]
    if len(bad):
        i = int(bad[0])
        pytest.fail(f"{what} of {_id(p)}, party {party}: {len(bad)} of {got.size} words differ, the first at word {i}: "
                    f"device {int(got[i]):#x}, host {int(want[i]):#x}")


def _device_equals_host(p, seed):
    crs = mk.CRS(p, seed) if p.multikey else None
    sd = mk.Scheme(p)                                                   # no key is ever loaded: install=False needs none
    made = []
    for i in range(min(p.nparty, 2)):                                   # two parties of one seed
        host = mk.party_keygen_seeded(crs, p, party=i, mask_seed=MS, deterministic_seed=seed)
        secr = mk.party_keygen(crs, p, party=i, secrets_only=True, deterministic_seed=seed)
        dev = mk.keygen_device_seeded(sd, i, secr, mask_seed=MS)
        assert dev.seeded and dev.mask_seed == MS and dev.brk is None and dev.ksk is None and dev.brk_seeded.dtype == p.ring_dtype
        _same_words(dev.brk_seeded, host.brk_seeded, "brk_seeded", p, i)
        _same_words(dev.ksk_seeded, host.ksk_seeded, "ksk_seeded", p, i)
        made.append((dev.brk_seeded.copy(), dev.ksk_seeded.copy()))
    if len(made) == 2:
        assert not np.array_equal(made[0][0], made[1][0]), "two parties of one seed were given one bootstrapping-key section"
        assert not np.array_equal(made[0][1], made[1][1]), "two parties of one seed were given one key-switching-key section"
    sd.close()


def test_the_grid_stride_shape_exceeds_one_launch():
    p = SHAPES[-1]
    assert p.ksk_rows == 196608 > 2048 * 64


@pytest.mark.parametrize("p", SHAPES, ids=_id)
def test_device_sections_are_the_host_sections_word_for_word(require_gpu, p):
    _device_equals_host(p, 6600 + SHAPES.index(p))


WIDE = 2.0 ** 55
WIDE_SHAPES = [p.scaled(alpha=WIDE, beta=WIDE) for p in (
    mk.CGGIparam.scaled(n=3, N=256), mk.CGGIparam.scaled(n=2, N=2048),          # RGSW kernel, W = 32: 4- and 16-register accumulator
    mk.KMS2party.scaled(n=3, N=256), mk.KMS2party.scaled(n=2, N=2048),          # RGSW kernel, W = 64
    mk.CCS2party.scaled(n=3, N=256), mk.CCS2party.scaled(n=2, N=2048),          # UniEnc kernel, both of its noise sites
    mk.KMS2partyblock.scaled(n=12, N=256, blk_d=4),                             # the key-switching noise word, absent rows beside it
    mk.CGGIparam.scaled(n=3, N=32), mk.KMS2party.scaled(n=3, N=32))]            # N = 32: idle lanes in fill_noise, on both ring widths


@pytest.mark.parametrize("p", WIDE_SHAPES, ids=_id)
def test_device_sections_are_the_host_sections_at_full_mantissa_noise(require_gpu, p):
    """the same comparison with alpha = beta = 2^55, where every noise word carries the deviate's mantissa (tests/test_gpu_keygen.py): it holds
    "box_muller gives the same bits on host and device" for the three noise sites of keygen_seeded.hip"""
    _device_equals_host(p, 7700 + WIDE_SHAPES.index(p))


class _DeviceKeys:
    """a party's secrets and small keys, with the two large keys expanded on the host from the sections the device made"""

    def __init__(self, secrets, brk, ksk):
        self._s, self.brk, self.ksk = secrets, brk, ksk

    def __getattr__(self, name):
        return getattr(self._s, name)


@pytest.mark.parametrize("p", [mk.CGGIparam.scaled(n=16), mk.Blockparam.scaled(n=18, blk_d=6), mk.CCS2party.scaled(n=20), mk.KMS2party.scaled(n=16),
                               mk.KMS2partyblock.scaled(n=18, blk_d=6)], ids=_id)
def test_device_made_sections_follow_their_laws(require_gpu, p):
    """the judgement of tests/test_keys_cpu.py (exact opening, max|e| <= 6 sigma + 1, noise / mask / independence statistics per
    component) on the host expansion of sections keygen_seeded.hip made, one set per scheme: independent of client.cpp's generator"""
    import test_keys_cpu as T
    seed = 8600 + p.scheme
    crs = mk.CRS(p, seed) if p.multikey else None
    sd = mk.Scheme(p)
    full = []
    for i in range(min(p.nparty, 2)):
        secr = mk.party_keygen(crs, p, party=i, secrets_only=True, deterministic_seed=seed)
        dev = mk.keygen_device_seeded(sd, i, secr, mask_seed=bytes([i + 1]) * 32)
        brk, ksk = mk.seeded_keys_expand(p, i, dev.mask_seed, dev.brk_seeded, dev.ksk_seeded)
        full.append(_DeviceKeys(secr, brk, ksk.ravel()))
    sd.close()
    T.judge_keys(p, crs, full, [], enc_seed=710_000, encryptions=2000)


def _gate_words(sch, c):
    return [mk.NAND(c[:8], c[8:16], sch), mk.XOR(c[:8], c[8:16], sch), mk.MUX(c[16:24], c[:8], c[8:16], sch)]


def _loaded(p, crs, host, arith=mk.ARITH_F64REF):
    """a scheme with the host-generated seeded parties loaded (load_seeded)"""
    sch = mk.Scheme(p, arith=arith)
    if p.multikey:
        sch.load_crs(crs)
    for i, k in enumerate(host):
        mk.load_seeded(sch, i, k)
    return sch


def _host_set(p, seed):
    crs = mk.CRS(p, seed) if p.multikey else None
    return crs, [mk.party_keygen_seeded(crs, p, party=i, mask_seed=MS, deterministic_seed=seed) for i in range(p.nparty)], \
        [mk.party_keygen(crs, p, party=i, secrets_only=True, deterministic_seed=seed) for i in range(p.nparty)]


INSTALL_SETS = [(mk.CGGIparam.scaled(n=16, N=256), mk.ARITH_F64REF), (mk.CCS2party.scaled(n=20), mk.ARITH_F64REF), (mk.KMS2party.scaled(n=16), mk.ARITH_EXACT)]


@pytest.mark.parametrize("p, arith", INSTALL_SETS, ids=lambda v: v.name if hasattr(v, "name") else ("exact" if v else "f64"))
def test_install_leaves_the_resident_state_of_load_seeded(require_gpu, p, arith):
    """scheme A: every party installed from the device (install=1); scheme B: load_seeded of the host-generated party of the same seeds.
    get_ksk is equal, NAND / XOR / MUX words of 8 rows are equal; on the MKT_ARITH_EXACT set "fx_bound" and "fx_kmax" too"""
    seed = 31
    crs, host, secr = _host_set(p, seed)
    A = mk.Scheme(p, arith=arith)
    if p.multikey:
        A.load_crs(crs)
    for i, s in enumerate(secr):
        dev = mk.keygen_device_seeded(A, i, s, mask_seed=MS, install=True)
        _same_words(dev.brk_seeded, host[i].brk_seeded, "brk_seeded", p, i)
        _same_words(dev.ksk_seeded, host[i].ksk_seeded, "ksk_seeded", p, i)
    B = _loaded(p, crs, host, arith)
    for i in range(p.nparty):
        _same_words(A.get_ksk(i), B.get_ksk(i), "resident key-switching key", p, i)
    c = encrypt_bits(p, host, np.random.default_rng(8).integers(0, 2, 24).astype(bool), seed=1200)
    for name, a, b in zip(("NAND", "XOR", "MUX"), _gate_words(A, c), _gate_words(B, c)):
        _same_words(a, b, name + " output", p, -1)
    if arith == mk.ARITH_EXACT:
        assert A.get_metric("fx_kmax") == B.get_metric("fx_kmax") > 0.0 and A.get_metric("fx_bound") == B.get_metric("fx_bound")
    A.close(); B.close()


def test_without_install_a_loaded_scheme_is_left_alone(require_gpu):
    p = mk.KMS2party.scaled(n=16, N=256)
    crs, host, secr = _host_set(p, 32)
    sch = _loaded(p, crs, host)
    c = encrypt_bits(p, host, np.random.default_rng(9).integers(0, 2, 24).astype(bool), seed=1300)
    before, ksk = _gate_words(sch, c), [sch.get_ksk(i) for i in range(p.nparty)]
    other = mk.party_keygen(crs, p, party=1, secrets_only=True, deterministic_seed=999)      # another secret: an install would change the tables
    dev = mk.keygen_device_seeded(sch, 1, other, mask_seed=bytes(range(32)))
    assert not np.array_equal(dev.ksk_seeded, host[1].ksk_seeded)
    for a, b in zip(before, _gate_words(sch, c)):
        assert np.array_equal(a, b)
    for i in range(p.nparty):
        assert np.array_equal(ksk[i], sch.get_ksk(i))
    sch.close()


def test_refusals_write_nothing_and_touch_nothing(require_gpu):
    """every MKT_ERR_ARG refusal of the header through the raw ABI: the 0xA5-filled outputs are untouched and a loaded scheme computes the
    words it computed before; install=1 on a forked context is MKT_ERR_STATE on both sharers"""
    from mktfhe_amd import _lib, scheme as S
    L = _lib.lib()
    p = mk.KMS2party.scaled(n=16, N=256)
    crs, host, secr = _host_set(p, 33)
    sch = _loaded(p, crs, host)
    c = encrypt_bits(p, host, np.random.default_rng(10).integers(0, 2, 24).astype(bool), seed=1400)
    before = _gate_words(sch, c)
    wb, wk = mk.seeded_section_words(p)
    ob, ok = np.full(wb, FILL, dtype=p.ring_dtype), np.full(wk, FILL, dtype=np.uint32)
    seed = (C.c_uint8 * 32)(*MS)
    own = (C.c_uint8 * 32)()
    assert L.mkt_client_test_seed(33, own) == 0                       # the seed secr[1] was made from: its stream key, byte for byte
    other_p = mk.KMS2party.scaled(n=17, N=256)
    foreign = mk.party_keygen(mk.CRS(other_p, 33), other_p, party=1, secrets_only=True, deterministic_seed=33)

    def gen(party=1, keys=secr[1], mseed=seed, outb=ob, outk=ok, install=0):
        ptr = lambda v: None if v is None else S._np_ptr(v)      # noqa: E731
        return L.mkt_keygen_device_seeded(sch.h, party, keys.h if keys is not None else None, None, mseed, ptr(outb), ptr(outk), install)

    refused = (dict(mseed=None), dict(mseed=own), dict(party=-1), dict(party=2), dict(keys=None), dict(keys=secr[0]), dict(keys=foreign),
               dict(outb=None), dict(outk=None), dict(outb=None, outk=None))
    for install in (0, 1):
        for kw in refused:
            if install and kw == dict(outb=None, outk=None):
                continue                                              # (with install=1 that is a call that asks for something)
            assert gen(install=install, **kw) == -1, (kw, install)
            assert (ob == np.asarray(FILL, dtype=ob.dtype)).all() and (ok == FILL).all(), ("an output word was written", kw, install)
    for a, b in zip(before, _gate_words(sch, c)):
        assert np.array_equal(a, b), "a refused call changed a resident table"
    # CCS without the CRS
    q = mk.CCS2party.scaled(n=3, N=256)
    sq, kq = mk.Scheme(q), mk.party_keygen(mk.CRS(q, 5), q, party=0, secrets_only=True, deterministic_seed=5)
    qb, qk = np.full(mk.seeded_section_words(q)[0], FILL, dtype=np.uint32), np.full(mk.seeded_section_words(q)[1], FILL, dtype=np.uint32)
    assert L.mkt_keygen_device_seeded(sq.h, 0, kq.h, None, seed, S._np_ptr(qb), S._np_ptr(qk), 0) == -1
    assert (qb == FILL).all() and (qk == FILL).all()
    sq.close()
    # a shared key set: install is MKT_ERR_STATE on both sharers, and generation without install still serves
    f = sch.fork()
    for s in (sch, f):
        with pytest.raises(mk.MktError) as ei:
            mk.keygen_device_seeded(s, 1, secr[1], mask_seed=MS, install=True)
        assert ei.value.code == -5
    _same_words(mk.keygen_device_seeded(f, 1, secr[1], mask_seed=MS).ksk_seeded, host[1].ksk_seeded, "ksk_seeded (fork)", p, 1)
    for a, b in zip(before, _gate_words(sch, c)):
        assert np.array_equal(a, b), "a refused install changed a resident table"
    f.close(); sch.close()


def test_c_example_through_the_abi(require_gpu, tmp_path):
    """examples/seeded_keygen_gpu.c: parties make their compact sections on the GPU from their secrets, a second context loads them and
    runs NAND, the result decrypts (gcc, no Python)"""
    exe = str(tmp_path / "seeded_keygen_gpu")
    lib = os.path.join(ROOT, "mktfhe_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "seeded_keygen_gpu.c"),
                           "-o", exe, "-L" + lib, "-lmktfhe_hip", "-Wl,-rpath," + lib])
    out = subprocess.run([exe, "24", "256"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
