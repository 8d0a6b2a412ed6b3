"""Seeded ciphertexts on the GPU (mkt_seeded_expand_batch / mkt_seeded_encrypt_batch, mktfhe_amd/csrc/seeded.hip): the device words are
the host's (mkt_client_seeded_expand / _encrypt, held to the definition in tests/test_seeded_cpu.py) word for word -- one mask_block and
one noise function on both sides, integer arithmetic elsewhere, so equality is exact -- at the shapes where the kernels' indexing changes;
expanded rows feed a gate; neither call needs an evaluation key; the C example runs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, gpu_scheme, keygen, mk
from helpers import device_words as _words, party_set as _set, secret_keys as _secrets, to_device as _dev

pytestmark = pytest.mark.gpu
MASK_SEED = bytes(range(100, 132))
SEED = 31
FILL = 0xA5A5A5A5


# n: below, at and past one keystream block (1, 3, 15, 16, 17) / four blocks less a word, exactly, plus a word (63, 64, 65) / a row longer
# than the 1024 words the workgroup stores per pass (257 x 3 is not; 1500 is) and than a tile of 4096 words (1500 x 3)
NS = [1, 3, 15, 16, 17, 63, 64, 65, 257, 1500]


@pytest.mark.parametrize("n", NS)
def test_device_expand_equals_host_expand(require_gpu, n):
    """nparty in {1, 2, 3} (rows of n + 1, 2 n + 1, 3 n + 1 words: every 16-byte phase of a block start occurs), the first and the last
    party, B in {1, 63, 64, 65}, row0 = 0 and 2^32 - 3 (the row index carries into the high nonce word inside the batch), host arrays and
    device tensors -- the output tensor a slice that starts one row into a 0xA5-filled allocation with one guard row behind it: the row
    before and the guard row stay as they were"""
    import torch
    rng = np.random.default_rng(n)
    for nparty in (1, 2, 3):
        p = _set(n, nparty)
        sch = mk.Scheme(p)                                   # no evaluation key is ever loaded
        body = rng.integers(0, 2**32, 65, dtype=np.uint64).astype(np.uint32)
        body_d = _dev(body)
        for party in sorted({0, nparty - 1}):
            for B in (1, 63, 64, 65):
                for row0 in (0, 2**32 - 3):
                    want = mk.seeded_expand(mk.SeededBatch(party, MASK_SEED, row0, body[:B]), p)
                    got = mk.seeded_expand(mk.SeededBatch(party, MASK_SEED, row0, body[:B]), p, scheme=sch)
                    assert isinstance(got, np.ndarray) and np.array_equal(got, want), (nparty, party, B, row0, "host arrays")
                    alloc = torch.full((B + 2, p.lwe_len), FILL - 2**32, dtype=torch.int32, device="cuda")
                    got_d = mk.seeded_expand(mk.SeededBatch(party, MASK_SEED, row0, body_d[:B]), p, scheme=sch, out=alloc[1:1 + B])
                    assert got_d.is_cuda and got_d.shape == (B, p.lwe_len)
                    a = _words(alloc)
                    assert np.array_equal(a[1:1 + B], want), (nparty, party, B, row0, "device tensors")
                    assert (a[0] == FILL).all() and (a[B + 1] == FILL).all(), (nparty, party, B, row0, "a word outside the rows was written")
        sch.close()


# the noise at the set's alpha (2^17) on every n; at n = 3, 64, 257 also at both ends of the admitted range 0 <= sigma <= 2^31, B the smallest
# and the largest of the grid
ENC_CASES = ([pytest.param(n, None, (1, 63, 64, 65), id=str(n)) for n in NS] +
             [pytest.param(n, s, (1, 65), id=f"{n}-sigma{name}") for n in (3, 64, 257) for s, name in ((0.0, "0"), (2.0**31, "2^31"))])


@pytest.mark.parametrize("n, sigma, batches", ENC_CASES)
def test_device_encrypt_equals_host_encrypt(require_gpu, n, sigma, batches):
    """the same grid of n, nparty, party, B and row0; mu a device tensor (and once per set a host array); noise at the set's alpha, and at
    n = 3, 64, 257 also at sigma = 0 and 2^31.  At sigma = 0 a batch encrypted on the device, expanded on the device and opened with
    mk.lwe_phase gives mu word for word: the definition, on the device.
    What the equality can and cannot see: the noise word is 32 bits of rint(sigma g) with sigma <= 2^31, and a one-ulp change of the
    deviate g never reaches it (0 of 4 000 000 words at any such sigma under a contracted build, tests/test_rng_cpu.py).  The cap is part
    of the contract, so for this translation unit the bit identity of the Gaussian rests on the shared header -- held at sigma = 2^55 by
    tests/test_gpu_keygen.py and on the host by tests/test_rng_cpu.py -- and on the shared compile flags, held by tests/test_rng_cpu.py."""
    rng = np.random.default_rng(100 + n)
    for nparty in (1, 2, 3):
        p = _set(n, nparty)
        if sigma is not None:
            p = p.scaled(alpha=sigma)                        # the deviation both calls are given
        keys = _secrets(p)
        sch = mk.Scheme(p)
        mu = rng.integers(0, 2**32, 65, dtype=np.uint64).astype(np.uint32)
        mu_d = _dev(mu)
        for party in sorted({0, nparty - 1}):
            for B in batches:
                for row0 in (0, 2**32 - 3):
                    kw = dict(words=True, mask_seed=MASK_SEED, deterministic_seed=SEED, row0=row0)
                    want = mk.seeded_encrypt(mu[:B], keys[party], p, party, **kw).body
                    got = mk.seeded_encrypt(mu_d[:B], keys[party], p, party, scheme=sch, **kw)
                    assert got.body.is_cuda and got.body.shape == (B,) and np.array_equal(_words(got.body), want), (nparty, party, B, row0)
                    if sigma == 0.0:
                        rows = mk.seeded_expand(got, p, scheme=sch)
                        assert rows.is_cuda and np.array_equal(mk.lwe_phase(_words(rows), keys if p.multikey else keys[0], p), mu[:B]), (nparty, party, B, row0)
            got = mk.seeded_encrypt(mu, keys[party], p, party, scheme=sch, words=True, mask_seed=MASK_SEED, deterministic_seed=SEED)
            assert isinstance(got.body, np.ndarray)
            assert np.array_equal(got.body, mk.seeded_encrypt(mu, keys[party], p, party, words=True, mask_seed=MASK_SEED, deterministic_seed=SEED).body)
        sch.close()


def test_grid_stride(require_gpu):
    """n = 4, nparty = 2 (rows of 9 words), row0 = 2^32 - 70 000.  A launch has at most 2048 workgroups.  The expand kernel's tile is 2288
    words here (the most for which at most 256 keystream blocks begin in tile + 15 words: 2303 // 9 + 1 = 256), so 2049 tiles and a
    ragged row need 2049 * 2288 // 9 + 2 rows; the encrypt kernel's tile is 64 rows, so 2048 * 64 + 65 rows do there"""
    p = _set(4, 2)
    keys = _secrets(p)
    sch = mk.Scheme(p)
    row0 = 2**32 - 70_000
    B = 2049 * 2288 // 9 + 2
    assert B * p.lwe_len > 2049 * 2288 and B > 2048 * 64 + 65
    rng = np.random.default_rng(3)
    mu = rng.integers(0, 2**32, B, dtype=np.uint64).astype(np.uint32)
    for party in (0, 1):
        want = mk.seeded_encrypt(mu, keys[party], p, party, words=True, mask_seed=MASK_SEED, deterministic_seed=SEED, row0=row0)
        got = mk.seeded_encrypt(_dev(mu), keys[party], p, party, scheme=sch, words=True, mask_seed=MASK_SEED, deterministic_seed=SEED, row0=row0)
        assert np.array_equal(_words(got.body), want.body), party
        rows = mk.seeded_expand(got, p, scheme=sch)
        assert np.array_equal(_words(rows), mk.seeded_expand(want, p)), party
    sch.close()


@pytest.mark.parametrize("p", [mk.KMS2party.scaled(n=16, N=256), mk.CCS2party.scaled(n=12, N=256)], ids=lambda p: p.name)
def test_seeded_inputs_feed_a_gate(require_gpu, p):
    """each party seeded-encrypts 64 bits on the device; the evaluator expands on the device, the rows equal the host expansion; NAND of
    the two runs and decrypts to NAND of the bits"""
    B = 64
    crs, keys = keygen(p, 7)
    sg = gpu_scheme(p, crs, keys)
    bits = np.random.default_rng(8).integers(0, 2, (2, B)).astype(bool)
    rows = []
    for i in range(2):
        own = mk.Scheme(p)                                   # the party's own context: no evaluation key
        mu = np.where(bits[i], np.uint32(1 << 29), np.uint32(7 << 29)).astype(np.uint32)
        batch = mk.seeded_encrypt(_dev(mu), keys[i], p, i, words=True, scheme=own)
        own.close()
        sent = mk.SeededBatch(batch.party, batch.mask_seed, batch.row0, _words(batch.body))        # what travels
        r = mk.seeded_expand(mk.SeededBatch(i, sent.mask_seed, sent.row0, _dev(sent.body)), p, scheme=sg)
        assert r.is_cuda and np.array_equal(_words(r), mk.seeded_expand(sent, p)), i
        assert np.array_equal(mk.lwe_decrypt(_words(r), keys, p), bits[i]), i
        rows.append(r)
    out = mk.NAND(rows[0], rows[1], sg)
    assert np.array_equal(mk.lwe_decrypt(_words(out), keys, p), ~(bits[0] & bits[1]))
    sg.close()


def test_no_evaluation_keys_and_refusals(require_gpu):
    """a context made by Scheme(p) alone -- no key loaded, where a gate raises MKT_ERR_STATE -- serves both calls, on both arithmetic
    modes; every refusal of the header's list is MKT_ERR_ARG through the raw ABI and leaves the output as it was"""
    from mktfhe_amd import _lib, scheme as S
    p = mk.KMS2party.scaled(n=16, N=256)
    keys, okeys = _secrets(p), _secrets(mk.KMS2party.scaled(n=17, N=256))
    mu = np.random.default_rng(5).integers(0, 2**32, 9, dtype=np.uint64).astype(np.uint32)
    want = mk.seeded_encrypt(mu, keys[1], p, 1, words=True, mask_seed=MASK_SEED, deterministic_seed=SEED)
    ms, same, ns = (C.c_uint8 * 32)(*MASK_SEED), (C.c_uint8 * 32)(*MASK_SEED), (C.c_uint8 * 32)(*range(32))
    L = _lib.lib()
    for arith in (mk.ARITH_F64REF, mk.ARITH_EXACT):
        sch = mk.Scheme(p, arith=arith)
        ct = np.zeros((9, p.lwe_len), dtype=np.uint32)
        with pytest.raises(mk.MktError) as ei:
            sch.gate(0, ct, ct)
        assert ei.value.code == -5
        got = mk.seeded_encrypt(mu, keys[1], p, 1, words=True, scheme=sch, mask_seed=MASK_SEED, deterministic_seed=SEED)
        assert np.array_equal(got.body, want.body)
        assert np.array_equal(mk.seeded_expand(got, p, scheme=sch), mk.seeded_expand(want, p))
        body = np.full(9, FILL, dtype=np.uint32)
        rows = np.full((9, p.lwe_len), FILL, dtype=np.uint32)

        def enc(party=1, key=keys[1], sigma=p.alpha, mseed=ms, nseed=ns, B=9, mem=S.MEM_HOST):
            return L.mkt_seeded_encrypt_batch(sch.h, party, key.h, S._np_ptr(mu), sigma, mseed, nseed, 0, S._np_ptr(body), B, mem)

        def exp(party=1, mseed=ms, B=9, mem=S.MEM_HOST):
            return L.mkt_seeded_expand_batch(sch.h, party, mseed, 0, S._np_ptr(mu), S._np_ptr(rows), B, mem)

        for kw in (dict(mseed=None), dict(nseed=same), dict(party=-1), dict(party=2), dict(party=0), dict(key=okeys[1]), dict(sigma=-1.0),
                   dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma=float(np.nextafter(2.0**31, np.inf))), dict(mem=7)):
            assert enc(**kw) == -1 and (body == FILL).all(), kw
        for kw in (dict(mseed=None), dict(party=-1), dict(party=2), dict(mem=7)):
            assert exp(**kw) == -1 and (rows == FILL).all(), kw
        assert enc(B=0) == 0 and exp(B=0) == 0 and (body == FILL).all() and (rows == FILL).all()
        # two calls without a noise seed draw different noise on the device
        a, b = (mk.seeded_encrypt(mu, keys[1], p, 1, words=True, scheme=sch, mask_seed=MASK_SEED).body for _ in range(2))
        assert (a != b).sum() >= 8
        sch.close()


def test_c_example_through_the_abi(require_gpu, tmp_path):
    """examples/seeded_inputs.c: parties, evaluator and decryption from plain C (gcc, no Python), built and run as
    tests/test_gpu_partial_decrypt.py runs distributed_decrypt.c"""
    exe = str(tmp_path / "seeded_inputs")
    lib = os.path.join(ROOT, "mktfhe_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "seeded_inputs.c"),
                           "-o", exe, "-L" + lib, "-lmktfhe_hip", "-Wl,-rpath," + lib])
    out = subprocess.run([exe, "24", "256"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
