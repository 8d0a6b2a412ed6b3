"""Packed outputs on the GPU (mkt_pack_batch, mktfhe_amd/csrc/pack.hip): the device words equal tests/ref_pack.py word for word -- Float64
mode on a scaled set of each scheme, both ring widths, 1 to 3 parties, RLWE length 2; EXACT mode against the schoolbook product --, the packed
ciphertext opens and key-switches back to its rows, gate outputs survive pack + ring shares + merge, the refusals, and the pack noise
against its prediction.

Shapes: N in {256, 512}; n in {3, 17, 64}: a single ragged q-chunk (3 < 4 words per workgroup), 17 = 4 chunks and one word, 64 = 16 whole
chunks.  B in {0, 1, N - 1, N, N + 1, 2N + 3}: no pack, one row, one short of / exactly / one past a pack, three packs with a ragged last.
The generators of tests/edge_cases.py are case lists of whole parameter sets; the crafted mask words here are this gadget's own boundaries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ref_keys as RK
import ref_pack as RP
from helpers import GATE_FUNCS, ROOT, encrypt_bits, gpu_scheme, keygen, mk, secret_keys
from helpers import to_device as _dev

from mktfhe_amd import _lib

pytestmark = pytest.mark.gpu
GADGETS = [(1, 16), (4, 4), (8, 4), (3, 5)]

# one scaled set per scheme (the five), both ring widths, k = 1, 2, 3 parties, CGGI with RLWE length 2 and 3
F64_SETS = {
    "cggi-n17": mk.CGGIparam.scaled(n=17, N=256),
    "cggi-k2-n3": mk.CGGIparam.scaled(n=3, N=256, k=2),
    "cggi-k3-n17-N512": mk.CGGIparam.scaled(n=17, N=512, k=3),
    "lmss-n18": mk.Blockparam.scaled(n=18, N=256, blk_d=6),
    "ccs-k2-n64": mk.CCS2party.scaled(n=64, N=256),
    "ccs-k3-n3-N512": mk.CCS2party.scaled(n=3, N=512, k=3),
    "kms-k1-n3": mk.KMS2party.scaled(n=3, N=256, k=1),
    "kms-k2-n64": mk.KMS2party.scaled(n=64, N=256),
    "kms-k3-n17-N512": mk.KMS2party.scaled(n=17, N=512, k=3),
    "kmsblock-k2-n18": mk.KMS2partyblock.scaled(n=18, N=256, blk_d=6),
}


def seed_bytes(n):
    buf = (C.c_uint8 * 32)()
    assert _lib.lib().mkt_client_test_seed(n, buf) == 0
    return bytes(buf)


def edge_words(l, logB):
    """32-bit mask words at the decomposition's carry and rounding boundaries: the ends and the middle of the torus, +-1 around the half-step
    of the gadget's last digit (where divbits rounds up), and every digit at and beside B/2, where the balanced digit turns negative and
    carries into the next"""
    T = l * logB
    w = [0, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 1, 0x80000001]
    if T < 32:
        h = 1 << (31 - T)
        w += [h - 1, h, h + 1, 0xFFFFFFFF - h, 0x100000000 - h, 0x100000000 - h - 1, 0x80000000 - h, 0x80000000 + h - 1]
    for t in range(l):
        g = 1 << (32 - (t + 1) * logB)
        half = (g << (logB - 1)) & 0xFFFFFFFF
        w += [half, (half - 1) & 0xFFFFFFFF, (half + 1) & 0xFFFFFFFF, (half - g) & 0xFFFFFFFF, (0x100000000 - g) & 0xFFFFFFFF]
    carry = sum((1 << (logB - 1)) << (32 - (t + 1) * logB) for t in range(l)) & 0xFFFFFFFF       # every digit at B/2: a carry chain end to end
    return np.array(w + [carry, (carry - 1) & 0xFFFFFFFF], dtype=np.uint32)


def crafted_pool(p, rows, l, logB, rng):
    """random rows with the boundary words planted in every party's block (first, last and an inner word), in the body, and as whole rows"""
    pool = rng.integers(0, 2**32, (rows, p.lwe_len), dtype=np.uint64).astype(np.uint32)
    e = edge_words(l, logB)
    for j in range(min(rows, 3 * len(e))):
        w = e[j % len(e)]
        if j < len(e):
            for i in range(p.nparty):
                pool[j, i * p.n] = w
                pool[j, (i + 1) * p.n - 1] = e[(j + i + 1) % len(e)]
        elif j < 2 * len(e):
            pool[j, :] = w
        else:
            pool[j, -1] = w
    return pool


def pack_setup(p, l, logB, arith=mk.ARITH_F64REF, seed=71):
    """-> (keys: secrets only, packing keys, a Scheme with the packing keys loaded and NO other key)"""
    keys = secret_keys(p, seed=seed)
    pks = [mk.packing_keygen(keys[i], p, l, logB, deterministic_seed=seed_bytes(seed + 1 + i)) for i in range(p.nparty)]
    sch = mk.Scheme(p, arith=arith)
    for i in range(p.nparty):
        mk.load_packing_key(sch, i, pks[i], l, logB)
    return keys, pks, sch


def run_batches(p, sch, pks, l, logB, exact, batches, rng):
    """every B with a way of picking rows and a memory kind, cycling so that each (idx kind, memory kind) pair occurs"""
    N = p.N
    pool = crafted_pool(p, 2 * N + 7, l, logB, rng)
    pool_d = _dev(pool)
    for case, B in enumerate(batches):
        kind = ("none", "perm", "repeat")[case % 3]
        idx = None if kind == "none" else rng.permutation(pool.shape[0])[:B].astype(np.uint32) if kind == "perm" else rng.integers(0, 5, B).astype(np.uint32)
        src = pool[:B] if idx is None else pool
        want = RP.pack(p, pool[:B] if idx is None else pool[idx], pks, l, logB, exact=exact).astype(p.ring_dtype) if B else np.zeros((0, p.k + 1, N), dtype=p.ring_dtype)
        for device in [case % 2 == 1] + ([case % 2 == 0] if B in (1, N + 1) else []):      # host arrays / device tensors in turn; both at B = 1 and N + 1
            if device:
                got = mk.pack(sch, pool_d[:B] if idx is None else pool_d, None if idx is None else _dev(idx))
                assert got.is_cuda and tuple(got.shape) == want.shape
                got = got.cpu().numpy().view(p.ring_dtype)
            else:
                got = mk.pack(sch, src, idx)
                assert isinstance(got, np.ndarray) and got.dtype == p.ring_dtype
            assert got.shape == want.shape and np.array_equal(got, want), (B, kind, "device" if device else "host")


@pytest.mark.parametrize("name", sorted(F64_SETS))
def test_f64_words_equal_the_restatement(require_gpu, name):
    p = F64_SETS[name]
    N = p.N
    rng = np.random.default_rng(len(name))
    order = sorted(F64_SETS).index(name)
    for gi in (order % 4, (order + 2) % 4) if N == 256 else (order % 4,):
        l, logB = GADGETS[gi]
        keys, pks, sch = pack_setup(p, l, logB)
        run_batches(p, sch, pks, l, logB, False, (0, 1, N - 1, N, N + 1, 2 * N + 3) if gi == order % 4 else (1, N + 1), rng)
        sch.close()


@pytest.mark.parametrize("name", ["cggi-n17", "kms-k2-n64"])
@pytest.mark.parametrize("gadget", GADGETS, ids=lambda g: f"l{g[0]}-logB{g[1]}")
def test_every_gadget_on_both_ring_widths(require_gpu, name, gadget):
    """the four gadgets -- one digit of 16 bits, 16 bits in four, all 32 bits (no rounding), 15 bits unaligned -- on the 32-bit and the 64-bit ring"""
    p = F64_SETS[name].scaled(n=17)
    keys, pks, sch = pack_setup(p, *gadget)
    run_batches(p, sch, pks, *gadget, False, (p.N + 1,), np.random.default_rng(sum(gadget)))
    sch.close()


@pytest.mark.parametrize("name", ["cggi-n17", "kms-k2-n64", "cggi-k2-n3", "ccs-k2-n64"])
def test_exact_words_equal_the_schoolbook(require_gpu, name):
    """MKT_ARITH_EXACT: every product exact (big-integer words), one set per ring width and the two slot rules; gadgets (4, 4) and (3, 5)"""
    p = F64_SETS[name].scaled(n=min(F64_SETS[name].n, 17))
    for l, logB in ((4, 4), (3, 5)):
        keys, pks, sch = pack_setup(p, l, logB, arith=mk.ARITH_EXACT)
        run_batches(p, sch, pks, l, logB, True, (1, p.N + 1), np.random.default_rng(l))
        sch.close()


@pytest.mark.parametrize("name", ["cggi-n17", "kms-k2-n64", "ccs-k3-n3-N512"])
def test_exact_noise_free_key_gives_the_recomposed_phase(require_gpu, name):
    """EXACT with sigma_ring = 0: phase(pack(x)) minus the LWE phase of row j equals sum_q s[q] (recomposed(a_q) - a_q), word for word, per coefficient"""
    p = F64_SETS[name].scaled(beta=0.0)
    for l, logB in ((4, 4), (3, 5), (8, 4)):
        keys, pks, sch = pack_setup(p, l, logB, arith=mk.ARITH_EXACT)
        rows = crafted_pool(p, p.N, l, logB, np.random.default_rng(5))
        ct = mk.pack(sch, rows)
        ph = mk.rlwe_phase(ct[0], keys, p)
        s = np.concatenate([np.asarray(k.lwekey, dtype=np.uint32) for k in keys])
        want = ((RP.recomposed(p, rows[:, :-1], l, logB) - rows[:, :-1]) * s).sum(-1, dtype=np.uint32)
        assert np.array_equal((ph - RP.lwe_phase(p, rows, [k.lwekey for k in keys])).astype(np.uint32), want), (l, logB)
        if l * logB == 32:
            assert not want.any()
        sch.close()


def test_keyswitch_at_reads_the_rows_back_and_shares_open_gate_outputs(require_gpu):
    """a packed ciphertext is an ordinary accumulator of keyswitch_at: coefficient j decrypts to bit j (j = 0, 1, N - 1); the outputs of a gate
    batch, packed and opened by ring shares plus merge, are the plain circuit with zero wrong bits (tests/test_pack_cpu.py: the margin)"""
    for p in (mk.KMS2party.scaled(n=16, N=256), mk.CGGIparam.scaled(n=20, N=256)):
        N, l, logB = p.N, 4, 4
        crs, keys = keygen(p, 5)
        sg = gpu_scheme(p, crs, keys)
        for i in range(p.nparty):
            mk.load_packing_key(sg, i, mk.packing_keygen(keys[i], p, l, logB, deterministic_seed=seed_bytes(40 + i)), l, logB)
        B = N + 3
        bits = np.random.default_rng(8).integers(0, 2, 2 * B).astype(bool)
        c = encrypt_bits(p, keys, bits, seed=500)
        x, y = c[0::2], c[1::2]
        # fresh encryptions, packed: the key switch at coefficient j returns row j
        ct = mk.pack(sg, x[:N])
        back = mk.keyswitch_at(sg, ct, src=np.zeros(3, dtype=np.uint32), coef=np.array([0, 1, N - 1], dtype=np.uint32))
        assert np.array_equal(mk.lwe_decrypt(back, keys if p.multikey else keys[0], p), bits[0::2][[0, 1, N - 1]])
        # gate outputs on the device, packed there, opened by shares
        name_before = sg.last_kernel_name()
        out = mk.NAND(_dev(x), _dev(y), sg)
        name_gate = sg.last_kernel_name()
        packed = mk.pack(sg, out)
        assert sg.last_kernel_name() == name_gate and name_before in ("", name_gate)
        assert packed.is_cuda and tuple(packed.shape) == (2, p.k + 1, N)
        shares = [mk.rlwe_partial_decrypt(packed, keys[i], p, i, 2.0 ** 20, deterministic_seed=60 + i) for i in range(p.nparty)]
        got = np.concatenate([mk.rlwe_merge_decrypt(packed[g], [s[g] for s in shares], p) for g in range(2)])[:B]
        assert np.array_equal(got, GATE_FUNCS[0](bits[0::2], bits[1::2])), "wrong bits after pack + shares + merge"
        hostct = packed.cpu().numpy().view(p.ring_dtype)
        assert np.array_equal(np.concatenate([RP.bit_of_phase(p, mk.rlwe_phase(hostct[g], keys, p)) for g in range(2)])[:B], got)
        sg.close()


def test_refusals_leave_the_output_untouched(require_gpu):
    from mktfhe_amd import scheme as S
    p = mk.KMS2party.scaled(n=3, N=256)
    keys = secret_keys(p, seed=3)
    pks = [mk.packing_keygen(keys[i], p, 4, 4, deterministic_seed=seed_bytes(i)) for i in range(2)]
    sch = mk.Scheme(p)
    pool = np.random.default_rng(1).integers(0, 2**32, (p.N + 2, p.lwe_len), dtype=np.uint64).astype(np.uint32)
    out = np.full((2, p.k + 1, p.N), 0xA5, dtype=p.ring_dtype)
    L, ptr = _lib.lib(), S._np_ptr
    call = lambda pool_, rows, idx, B, o=out, mem=S.MEM_HOST: L.mkt_pack_batch(sch.h, ptr(pool_), rows, None if idx is None else ptr(idx), B, ptr(o), mem)   # noqa: E731
    assert call(pool, 5, None, 5) == -5, "MKT_ERR_STATE before any packing key"
    mk.load_packing_key(sch, 0, pks[0], 4, 4)
    assert call(pool, 5, None, 5) == -5 and call(pool, 5, None, 0) == -5, "MKT_ERR_STATE until every party has loaded"
    with pytest.raises(mk.MktError) as ei:
        mk.load_packing_key(sch, 1, pks[1][:, :2], 2, 4)
    assert ei.value.code == -1, "one gadget per context"
    assert L.mkt_load_packing_key(sch.h, 2, ptr(pks[1]), 4, 4) == -1 and L.mkt_load_packing_key(sch.h, 1, None, 4, 4) == -1
    assert L.mkt_load_packing_key(sch.h, 1, ptr(pks[1]), 3, 11) == -1
    mk.load_packing_key(sch, 1, pks[1], 4, 4)
    bad = np.array([0, 1, 5, 2], dtype=np.uint32)
    assert call(pool, 5, bad, 4) == -1, "host index outside the pool"
    assert call(pool, 0, None, 1) == -1, "rows of an empty pool"
    assert call(pool, 3, None, 4) == -1, "idx NULL names rows 0 .. B-1"
    assert L.mkt_pack_batch(sch.h, None, 5, None, 5, ptr(out), 1) == -1 and L.mkt_pack_batch(sch.h, ptr(pool), 5, None, 5, None, 1) == -1
    assert call(pool, 5, None, 5, mem=7) == -1, "unknown memory kind"
    over = pool.reshape(-1).view(p.ring_dtype)
    assert L.mkt_pack_batch(sch.h, ptr(pool), p.N + 2, None, 5, ptr(over), 1) == -1, "rlwe_out overlaps the pool"
    assert (out == 0xA5).all()
    assert call(pool, 5, None, 0) == 0 and (out == 0xA5).all(), "B == 0 succeeds and writes nothing"
    # a device index beyond the pool is clamped to the last row: the words of the same call with the clamped index
    got = mk.pack(sch, _dev(pool[:5]), _dev(bad)).cpu().numpy().view(p.ring_dtype)
    assert np.array_equal(got, mk.pack(sch, pool[:5], np.array([0, 1, 4, 2], dtype=np.uint32)))
    # options and the kernel name are as the call found them; the key set closes with the first fork
    assert sch.last_kernel_name() == ""
    fork = sch.fork()
    assert L.mkt_load_packing_key(sch.h, 0, ptr(pks[0]), 4, 4) == -5 and L.mkt_load_packing_key(fork.h, 0, ptr(pks[0]), 4, 4) == -5
    assert np.array_equal(mk.pack(fork, pool[:5]), mk.pack(sch, pool[:5]))
    fork.close(); sch.close()


def pack_errors(p, l, logB, packs, arith, seed):
    """random rows packed on the GPU, opened under the secrets: per-coefficient error on the 32-bit torus, int64 [packs N]"""
    keys, pks, sch = pack_setup(p, l, logB, arith=arith, seed=seed)
    rows = np.random.default_rng(seed).integers(0, 2**32, (packs * p.N, p.lwe_len), dtype=np.uint64).astype(np.uint32)
    ct = mk.pack(sch, rows)
    sch.close()
    ph = np.concatenate([mk.rlwe_phase(ct[g], keys, p) for g in range(packs)])
    hw = int(sum(int(np.asarray(k.lwekey).sum()) for k in keys))
    return RK.centered((ph - RP.lwe_phase(p, rows, [k.lwekey for k in keys])).astype(np.uint32), 32), hw


NOISE_CASES = {
    # the rounding term alone: a noise-free key, 16 of 32 bits kept; key term dominant: all 32 bits kept (no rounding), sigma_ring = 2^10 on the 32-bit ring
    "rounding": (mk.KMS2party.scaled(n=64, N=256, beta=0.0), 4, 4, mk.ARITH_EXACT),
    "rounding-f64": (mk.KMS2party.scaled(n=64, N=256, beta=0.0), 4, 4, mk.ARITH_F64REF),
    "key": (mk.CGGIparam.scaled(n=64, N=256, beta=1024.0), 8, 4, mk.ARITH_F64REF),
}


def measure_noise(name, packs=4):
    """-> record of one noise case: measured and predicted deviation, their ratio, the derived band(s)"""
    p, l, logB, arith = NOISE_CASES[name]
    e, hw = pack_errors(p, l, logB, packs, arith, seed=90 + len(name))
    m, sigma = e.size, float(np.sqrt((e.astype(np.float64) ** 2).mean()))
    key, rnd = RP.predicted(p, l, logB, p.N, p.beta)
    rec = {"case": name, "set": p.name, "n": p.n, "N": p.N, "nparty": p.nparty, "W": p.W, "gadget": [l, logB], "sigma_ring": p.beta, "samples": m,
           "mean": float(e.mean()), "sigma": sigma, "sigma_pred": float(np.sqrt(key + rnd)), "ratio": sigma / float(np.sqrt(key + rnd))}
    if name.startswith("rounding"):
        rec["band"], rec["band_hw"] = RP.band_rounding(p, m, hw)
        rec["hw"], rec["ratio_hw"] = hw, sigma / float(np.sqrt(RP.predicted(p, l, logB, p.N, p.beta, hw=hw)[1]))
    else:
        rec["band"] = RP.band_key(p, l, logB, m, p.beta)
    return rec


@pytest.mark.parametrize("name", sorted(NOISE_CASES))
def test_pack_noise_meets_its_prediction(require_gpu, name):
    """measured / predicted deviation of the pack error, live under the secrets, inside the band tests/ref_pack.py derives (sample count plus
    the stated model term); the mean within 5 standard errors of zero"""
    r = measure_noise(name)
    print(r)
    assert abs(r["ratio"] - 1.0) <= r["band"], r
    assert abs(r["mean"]) <= 5.0 * r["sigma_pred"] / np.sqrt(r["samples"]), r
    if "ratio_hw" in r:
        assert abs(r["ratio_hw"] - 1.0) <= r["band_hw"], r


def test_c_example_through_the_abi(require_gpu, tmp_path):
    """examples/packed_outputs.c: keys, gates, pack, per-party ring shares and merge from plain C (gcc, no Python)"""
    exe = str(tmp_path / "packed_outputs")
    lib = os.path.join(ROOT, "mktfhe_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "packed_outputs.c"),
                           "-o", exe, "-L" + lib, "-lmktfhe_hip", "-Wl,-rpath," + lib])
    out = subprocess.run([exe, "24", "256"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
