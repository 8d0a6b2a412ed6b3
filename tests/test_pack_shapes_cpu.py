"""The shapes of tests/pack_cases.py on the host: what vouches for the restatement tests/ref_pack.py at the ring sizes, sequence counts, column
counts and tile edges at which tests/test_gpu_pack_shapes.py compares the device with it word for word.  At every set the restatement, alone,
packs fresh encryptions into ciphertexts that open to their bits under the secrets with an error inside the bound of
test_pack_cpu.test_definition_opens_every_bit, and the library's host harness mk.rlwe_phase reads the words RP.phase reads.  The last tests hold
the case lists themselves: every instantiation of the product kernel has a set, every gadget occurs at every multi-wave size.

THE GADGET.  Every set is opened with gadget (4, 4), the gadget of test_definition_opens_every_bit, whose bound is used as it stands there.  The
other gadgets of the GPU test cannot all be opened at these sizes: (1, 16) on the 32-bit ring with sigma_ring = 2^7 has a key term of
sqrt(n c 2^32 / 12) 2^7 = 2^25.8 at n = 5 and c = 128 rows, 8.6 times which is the distance 2^29 between a bit and its threshold, and on the
64-bit ring its 16-bit digits times 64-bit key words leave the Float64 transform a rounding error of a few units of the 32-bit torus, which the
bound (exact but for its "+ 2") does not model.  What these sets are about is the ring size, the row count and the column count, and those are
the same under any gadget; tests/test_pack_cpu.py holds the restatement to its definition gadget by gadget."""
import numpy as np
import pytest

import ref_keys as RK
import ref_pack as RP
from helpers import mk, secret_keys
from pack_cases import EXACT_COLUMN_SETS, EXACT_NOISE_FREE_SET, GADGETS, KERNEL_SETS, SEQUENCE_SETS, TILE_SETS, kernel_key, sid
from test_pack_cpu import fresh_rows, seed_bytes

OPEN_CASES = ([("kernel", p) for p, _ in KERNEL_SETS] + [("sequence", p) for p, _ in SEQUENCE_SETS] + [("exact-columns", p) for p in EXACT_COLUMN_SETS]
              + [("tile", p) for p, _ in TILE_SETS])
L_PK, LOGB_PK = 4, 4


def error_bound(p, l, logB):
    """the bound of test_definition_opens_every_bit on the error of a coefficient that holds a row: the Gaussian's reach over the key term plus
    the worst rounding"""
    key_var, _ = RP.predicted(p, l, logB, p.N, p.beta)
    return 8.6 * np.sqrt(key_var) + p.nparty * p.n * 2.0 ** (32 - l * logB - 1) + 2, 8.6 * np.sqrt(key_var) + 2


def open_check(p, exact):
    l, logB = L_PK, LOGB_PK
    keys = secret_keys(p, seed=53)
    pks = [mk.packing_keygen(keys[i], p, l, logB, deterministic_seed=seed_bytes(70 + i)) for i in range(p.nparty)]
    B = p.N + 1                                                     # a full pack and a pack of one row
    bits = np.random.default_rng(p.N + p.n).integers(0, 2, B).astype(bool)
    rows = fresh_rows(p, keys, bits, 4000)
    ct = RP.pack(p, rows, pks, l, logB, exact=exact)
    assert ct.shape == (2, p.k + 1, p.N)
    zs = RP.ring_keys(p, keys)
    ph = np.concatenate([RP.phase(p, ct[g], zs) for g in range(2)])
    bound, bound_absent = error_bound(p, l, logB)
    assert bound <= 2.0 ** 28, "half the distance between a bit and its threshold; the fresh encryption's own 8.6 alpha = 2^20.1 has the rest"
    err = RK.centered((ph[:B] - RP.lwe_phase(p, rows, [k.lwekey for k in keys])).astype(np.uint32), 32)
    assert np.abs(err).max() <= bound, "pack error beyond the Gaussian's reach plus the worst rounding"
    assert np.abs(RK.centered(ph[B:], 32)).max() <= bound_absent, "the coefficients of absent rows carry key noise only"
    assert np.array_equal(RP.bit_of_phase(p, ph[:B]), bits)
    for g in range(2):
        assert np.array_equal(mk.rlwe_phase(ct[g].astype(p.ring_dtype), keys, p), RP.phase(p, ct[g], zs))


@pytest.mark.parametrize("kind,p", OPEN_CASES, ids=[f"{k}-{sid(p)}" for k, p in OPEN_CASES])
def test_restatement_opens_at_every_shape(kind, p):
    open_check(p, exact=False)


EXACT_OPEN = [(k, p) for k, p in OPEN_CASES if p.N <= 128]


@pytest.mark.parametrize("kind,p", EXACT_OPEN, ids=[f"{k}-{sid(p)}" for k, p in EXACT_OPEN])
def test_schoolbook_form_opens_at_every_small_shape(kind, p):
    open_check(p, exact=True)


def test_noise_free_set_differs_in_the_noise_alone():
    assert EXACT_NOISE_FREE_SET.scaled(beta=EXACT_COLUMN_SETS[1].beta) == EXACT_COLUMN_SETS[1] and EXACT_NOISE_FREE_SET.beta == 0.0


def test_every_product_kernel_instantiation_has_a_set():
    """pack_product_kernel<LOGM, WORD, NP> is dispatched over LOGM = 4 .. 11, both ring words and NP = 2, 3, 4 (pack.hip: MKT_DISPATCH_LOGM,
    launch_product_np): KERNEL_SETS and the N = 256 / 512 sets of test_gpu_pack.F64_SETS run all 48, computed from the parameter sets"""
    from test_gpu_pack import F64_SETS
    assert all(p.N in (256, 512) for p in F64_SETS.values())
    have = {kernel_key(p) for p, _ in KERNEL_SETS} | {kernel_key(p) for p in F64_SETS.values()}
    want = {(logM, W, NP) for logM in range(4, 12) for W in (32, 64) for NP in (2, 3, 4)}
    assert want - have == set(), sorted(want - have)
    assert have <= want
    ids = [sid(p) for p, _ in KERNEL_SETS]
    assert len(set(ids)) == len(ids)


def test_every_gadget_occurs_at_every_multi_wave_size():
    assert all(g in GADGETS for _, g in KERNEL_SETS)
    for N in (1024, 2048, 4096):
        assert {g for p, g in KERNEL_SETS if p.N == N} == set(GADGETS), N
    for N in (32, 64, 128, 1024, 2048, 4096):
        assert {kernel_key(p) for p, _ in KERNEL_SETS if p.N == N} == {(N.bit_length() - 2, W, NP) for W in (32, 64) for NP in (2, 3, 4)}, N


def test_lists_name_the_edges_they_are_for():
    """the sequence, column-chunk and tile lists sit on the constants of context.cpp and pack.hip they are about"""
    PACK_QCHUNK, PACK_EXACT_COLS, PACK_TILE = 4, 64, 64
    assert all(p.n % PACK_QCHUNK and p.n > PACK_QCHUNK for p, _ in KERNEL_SETS), "a whole chunk of mask words and a ragged one"
    assert all(p.N == 32 for p, _ in SEQUENCE_SETS) and {p.W for p, _ in SEQUENCE_SETS} == {32, 64}
    assert sorted({p.n for p in EXACT_COLUMN_SETS}) == [PACK_EXACT_COLS, PACK_EXACT_COLS + 1, 2 * PACK_EXACT_COLS + 1]
    assert {(p.W, p.nparty, RP.shape(p)[1]) for p in EXACT_COLUMN_SETS} == {(32, 1, 1), (32, 1, 2), (64, 2, 1)}
    assert sorted((p.lwe_len, p.N, p.nparty) for p, _ in TILE_SETS) == [(PACK_TILE, 32, 1), (PACK_TILE, 64, 1), (PACK_TILE + 1, 64, 1), (PACK_TILE + 1, 64, 2)]
