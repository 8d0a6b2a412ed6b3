"""Distributed decryption on the GPU (mkt_partial_decrypt_batch, mktfhe_amd/csrc/partial_decrypt.hip): the device shares are the host's
(mkt_client_partial_decrypt, held to its definition in tests/test_partial_decrypt_cpu.py) word for word -- integer dot products and one
shared noise function, so equality is exact -- at the shapes where the kernel's indexing changes; on gate outputs the merged phase differs
from the all-keys phase by exactly the k noise words; the call needs no evaluation keys; the C example runs."""
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, encrypt_bits, gpu_scheme, keygen, mk
from helpers import device_words as _words, party_set as _set, secret_keys as _secrets, to_device as _dev

pytestmark = pytest.mark.gpu
SIGMA = 2.0 ** 20
SEED = 31


# n: below a wave, the 16-byte body absent (1, 3) / one lane short of, exactly and one past one 16-byte pass of 16 lanes (63, 64, 65) /
# one word past a full wave pass of 256 words (257) / several passes with a ragged end (1500).  Every n is admitted by validate_params.
# Both ends of the admitted range 0 <= sigma <= 2^31, one n of each class, the smallest and the largest B: at 0 the share is the dot product
# alone; at 2^31 the noise word is the low half of a product of up to 2^34.1, the widest cast the call can be asked for.
CASES = ([pytest.param(n, SIGMA, (1, 63, 64, 65), id=str(n)) for n in (1, 3, 63, 64, 65, 257, 1500)] +
         [pytest.param(n, s, (1, 65), id=f"{n}-sigma{name}") for n in (3, 64, 257) for s, name in ((0.0, "0"), (2.0**31, "2^31"))])


@pytest.mark.parametrize("n, sigma, batches", CASES)
def test_device_shares_equal_host_shares(require_gpu, n, sigma, batches):
    """nparty in {1, 2, 3} (rows of n + 1, 2 n + 1, 3 n + 1 words: every 16-byte phase of a block start occurs), the first and the last
    party, B in {1, 63, 64, 65} (one tile short, full, one row over), row0 = 0 and 2^32 - 3 (the row index carries into the high nonce
    word inside the batch), host arrays and device tensors -- the tensor a slice that starts one row into its allocation.  sigma = 2^20,
    and at n = 3, 64, 257 also 0 and 2^31, the ends of the admitted range.  At sigma = 0 the device shares of all parties merge to
    mk.lwe_phase word for word: the definition, on the device.
    What the equality can and cannot see: the noise word is 32 bits of rint(sigma g) with sigma <= 2^31, and a one-ulp change of the
    deviate g never reaches it (0 of 4 000 000 words at any such sigma under a contracted build, tests/test_rng_cpu.py).  The cap is part
    of the contract, so for this translation unit the bit identity of the Gaussian rests on the shared header -- held at sigma = 2^55 by
    tests/test_gpu_keygen.py and on the host by tests/test_rng_cpu.py -- and on the shared compile flags, held by tests/test_rng_cpu.py."""
    rng = np.random.default_rng(n)
    for nparty in (1, 2, 3):
        p = _set(n, nparty)
        keys = _secrets(p)
        sch = mk.Scheme(p)                                   # no evaluation key is ever loaded
        ct = rng.integers(0, 2**32, (66, p.lwe_len), dtype=np.uint64).astype(np.uint32)
        ct_d = _dev(ct)
        for party in sorted({0, nparty - 1}):
            for B in batches:
                for row0 in (0, 2**32 - 3):
                    want = mk.partial_decrypt(ct[1:1 + B], keys[party], p, party, sigma, deterministic_seed=SEED, row0=row0)
                    got = mk.partial_decrypt(ct[1:1 + B], keys[party], p, party, sigma, scheme=sch, deterministic_seed=SEED, row0=row0)
                    assert isinstance(got, np.ndarray) and np.array_equal(got, want), (nparty, party, B, row0, "host arrays")
                    got_d = mk.partial_decrypt(ct_d[1:1 + B], keys[party], p, party, sigma, scheme=sch, deterministic_seed=SEED, row0=row0)
                    assert got_d.is_cuda and got_d.shape == (B,) and np.array_equal(_words(got_d), want), (nparty, party, B, row0, "device tensors")
        if sigma == 0.0:
            shares = [mk.partial_decrypt(ct_d, keys[i], p, i, 0.0, scheme=sch, deterministic_seed=SEED + i) for i in range(nparty)]
            assert np.array_equal(mk.merge_phase(ct, shares, p), mk.lwe_phase(ct, keys if p.multikey else keys[0], p)), (nparty, "merge at sigma 0")
        sch.close()


def test_grid_stride_and_large_batch(require_gpu):
    """B = 131 137 at n = 4: 2050 tiles of 64 rows, more than the 2048 workgroups of a launch, so workgroups 0 and 1 take a second tile
    (the grid-stride path: the cap is on workgroups of 64 rows each, so it is met above 131 072 rows, not 65 535), the last tile ragged"""
    p = _set(4, 2)
    keys = _secrets(p)
    sch = mk.Scheme(p)
    B = 2048 * 64 + 65
    ct = np.random.default_rng(3).integers(0, 2**32, (B, p.lwe_len), dtype=np.uint64).astype(np.uint32)
    for party in (0, 1):
        want = mk.partial_decrypt(ct, keys[party], p, party, SIGMA, deterministic_seed=SEED, row0=2**32 - 70_000)
        got = mk.partial_decrypt(_dev(ct), keys[party], p, party, SIGMA, scheme=sch, deterministic_seed=SEED, row0=2**32 - 70_000)
        assert np.array_equal(_words(got), want), party
    sch.close()


@pytest.mark.parametrize("p", [mk.KMS2party.scaled(n=16, N=256), mk.CCS2party.scaled(n=12, N=256)], ids=lambda p: p.name)
def test_gate_outputs_open_to_phase_plus_noise(require_gpu, p):
    """64 NANDs on the GPU, input x of every gate encrypted by party 0 and y by party 1; every party makes its share of the outputs on the
    device, each under its own pinned seed.  merge_phase - lwe_phase == the sum of the k noise words, exactly, the noise words recomputed
    on the host from the same seeds (the host shares of all-zero rows); merge_decrypt == lwe_decrypt == NAND of the bits (sigma_smudge =
    2^20 against the margin 2^29)"""
    B = 64
    crs, keys = keygen(p, 7)
    sg = gpu_scheme(p, crs, keys)
    bits = np.random.default_rng(8).integers(0, 2, 2 * B).astype(bool)
    c = encrypt_bits(p, keys, bits, seed=500)                # row j under party j mod 2
    x, y = c[0::2], c[1::2]
    out = mk.NAND(_dev(x), _dev(y), sg)
    shares = [mk.partial_decrypt(out, keys[i], p, i, SIGMA, scheme=sg, deterministic_seed=40 + i) for i in range(2)]
    assert all(s.is_cuda for s in shares)
    z = _words(out)
    noise = [mk.partial_decrypt(np.zeros_like(z), keys[i], p, i, SIGMA, deterministic_seed=40 + i) for i in range(2)]
    assert all(w.any() for w in noise)
    assert np.array_equal(mk.merge_phase(z, shares, p) - mk.lwe_phase(z, keys, p), noise[0] + noise[1])
    got = mk.merge_decrypt(out, shares, p)
    assert np.array_equal(got, mk.lwe_decrypt(z, keys, p)) and np.array_equal(got, ~(bits[0::2] & bits[1::2]))
    sg.close()


def test_no_evaluation_keys_and_refusals(require_gpu):
    """a context made by Scheme(p) alone -- no key loaded, where a gate raises MKT_ERR_STATE -- serves the call, on both arithmetic modes;
    a bad party, sigma or key set is MKT_ERR_ARG and leaves the output as it was"""
    import ctypes as C
    from mktfhe_amd import _lib, scheme as S
    p = mk.KMS2party.scaled(n=16, N=256)
    keys = _secrets(p)
    ct = np.random.default_rng(5).integers(0, 2**32, (9, p.lwe_len), dtype=np.uint64).astype(np.uint32)
    want = mk.partial_decrypt(ct, keys[1], p, 1, SIGMA, deterministic_seed=SEED)
    for arith in (mk.ARITH_F64REF, mk.ARITH_EXACT):
        sch = mk.Scheme(p, arith=arith)
        with pytest.raises(mk.MktError) as ei:
            sch.gate(0, ct, ct)
        assert ei.value.code == -5
        assert np.array_equal(mk.partial_decrypt(ct, keys[1], p, 1, SIGMA, scheme=sch, deterministic_seed=SEED), want)
        out = np.full(9, 0xA5A5A5A5, dtype=np.uint32)
        call = lambda party, key, sigma, B=9: _lib.lib().mkt_partial_decrypt_batch(sch.h, party, key.h, S._np_ptr(ct), sigma, None, 0, S._np_ptr(out), B, S.MEM_HOST)   # noqa: E731
        for args in ((-1, keys[0], SIGMA), (2, keys[1], SIGMA), (0, keys[1], SIGMA), (1, keys[1], -1.0), (1, keys[1], float("nan")),
                     (1, keys[1], float(np.nextafter(2.0**31, np.inf)))):
            assert call(*args) == -1 and (out == 0xA5A5A5A5).all(), args
        assert call(1, keys[1], SIGMA, B=0) == 0 and (out == 0xA5A5A5A5).all()
        assert _lib.lib().mkt_partial_decrypt_batch(sch.h, 1, keys[1].h, S._np_ptr(ct), SIGMA, None, 0, S._np_ptr(out), 9, 7) == -1     # unknown memory kind
        # two NULL-seed calls on the device draw different noise
        a, b = (mk.partial_decrypt(ct, keys[1], p, 1, SIGMA, scheme=sch) for _ in range(2))
        assert (a != b).all() or (a != b).sum() >= 8
        sch.close()


def test_c_example_through_the_abi(require_gpu, tmp_path):
    """examples/distributed_decrypt.c: the four roles from plain C (gcc, no Python), built and run as tests/test_gpu_parity.py runs kms_nand.c"""
    exe = str(tmp_path / "distributed_decrypt")
    lib = os.path.join(ROOT, "mktfhe_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "distributed_decrypt.c"),
                           "-o", exe, "-L" + lib, "-lmktfhe_hip", "-Wl,-rpath," + lib])
    out = subprocess.run([exe, "24", "256"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
