"""GPU tests of the three-input gates in one bootstrap (mkt_gate3_batch_ops / _gather, mkt_multi_gate3_batch_ops, Scheme.gate3*,
full_adder, Circuit three-input nodes, ripple_adder_fa).  Expected words: the linear part restated in numpy with 32-bit wrap
(tests/ref_gate3.py), then the CPU oracle's bootstrapping! -- word for word."""
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, encrypt_bits, gpu_scheme, keygen, mk, oracle_scheme
from ref_gate3 import linear3_rows, oracle_gate3, plain3
from mktfhe_amd import circuit as CI

pytestmark = pytest.mark.gpu

SMALL = [
    mk.CGGIparam.scaled(n=20, N=256),
    mk.Blockparam.scaled(n=30, N=256, blk_d=10),
    mk.KMS2party.scaled(n=16, N=256),
    mk.KMS2partyblock.scaled(n=24, N=256, blk_d=8),
    mk.CCS2party.scaled(n=12, N=256),
    mk.KMS4party.scaled(n=8, N=256),
]


def td(a):
    import torch
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _keys(p, keys):
    return keys if p.multikey else keys[0]


def _triples(p, keys, B, seed):
    """B random bit triples, operand r of triple j encrypted under party (j + r) mod k"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (3, B)).astype(bool)
    k = p.nparty
    ct = [np.stack([mk.lwe_ith_encrypt(int(bits[r, j]), (j + r) % k, keys[(j + r) % k], p, deterministic_seed=seed * 100 + 10 * j + r)
                    for j in range(B)]) for r in range(3)]
    return bits, ct


def _random_ops(rng, B):
    ops = (rng.integers(0, 6, B) | (rng.integers(0, 8, B) << 3)).astype(np.uint8)
    m = min(6, B)
    ops[:m] = np.arange(m)                                                     # every code at least once (B >= 6), unflagged
    return ops


@pytest.mark.parametrize("p", SMALL, ids=lambda p: f"{p.name}-n{p.n}-N{p.N}")
def test_gate3_ops_matches_the_oracle(require_gpu, p):
    """random codes and NOT flags, operands of a gate under different parties: == the oracle's bootstrap of the restated linear part,
    host and device memory; it decrypts to the truth table; gate3 with one code == gate3_ops; bad codes refused"""
    import torch
    crs, keys = keygen(p, 31)
    so, sg = oracle_scheme(p, crs, keys), gpu_scheme(p, crs, keys)
    B = 14
    bits, (x, y, z) = _triples(p, keys, B, 32)
    ops = _random_ops(np.random.default_rng(33), B)
    want = oracle_gate3(so, ops, x, y, z)
    got = sg.gate3_ops(ops, x, y, z)
    assert np.array_equal(got, want)
    got_d = sg.gate3_ops(td(ops), td(x), td(y), td(z))
    torch.cuda.synchronize()
    assert np.array_equal(got_d.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(mk.lwe_decrypt(got, _keys(p, keys), p), plain3(ops, *bits))
    for op in (mk.MAJ3_OP, mk.XOR3_OP | mk.OP_NOT_Z):
        assert np.array_equal(sg.gate3(op, x, y, z), sg.gate3_ops(np.full(B, op, np.uint8), x, y, z))
    assert np.array_equal(mk.MAJ3(x, y, z, sg), sg.gate3(mk.MAJ3_OP, x, y, z))
    assert np.array_equal(mk.XOR3(td(x), td(y), td(z), sg).cpu().numpy().view(np.uint32), sg.gate3(mk.XOR3_OP, x, y, z))
    for bad in (6, 7, 64, 128):
        with pytest.raises(mk.MktError, match="unknown gate code"):
            sg.gate3_ops(np.full(B, bad, np.uint8), x, y, z)
    sg.close()


@pytest.mark.parametrize("p", [mk.CGGIparam.scaled(n=20, N=256), mk.KMS2party.scaled(n=16, N=256)], ids=lambda p: p.name)
def test_gate3_gather_into_the_same_pool(require_gpu, p):
    """mkt_gate3_batch_gather: operands by row index, output into a later region of the SAME pool (device) or a separate array (host);
    the operand rows stay untouched; with host arrays an index outside the pool or a bad code is refused; an empty pool is refused;
    device-side indices beyond the pool are clamped to its last row"""
    import torch
    crs, keys = keygen(p, 35)
    so, sg = oracle_scheme(p, crs, keys), gpu_scheme(p, crs, keys)
    rng = np.random.default_rng(36)
    P, B = 9, 11
    pool = encrypt_bits(p, keys, rng.integers(0, 2, P).astype(bool), seed=3600)
    ix, iy, iz = (rng.integers(0, P, B).astype(np.uint32) for _ in range(3))
    ops = _random_ops(rng, B)
    want = oracle_gate3(so, ops, pool[ix], pool[iy], pool[iz])
    out_h = np.empty((B, p.lwe_len), dtype=np.uint32)
    sg.gate3_gather(ops, pool, ix, iy, iz, out_h)
    assert np.array_equal(out_h, want)
    big = torch.zeros((P + B, p.lwe_len), dtype=torch.int32, device="cuda")
    big[:P] = td(pool)
    sg.gate3_gather(td(ops), big, td(ix), td(iy), td(iz), big[P:])
    torch.cuda.synchronize()
    assert np.array_equal(big[P:].cpu().numpy().view(np.uint32), want)
    assert np.array_equal(big[:P].cpu().numpy().view(np.uint32), pool)
    # device indices past the pool read its last row (memory safety, not an API): the same words as naming row P - 1
    far = iz.copy(); far[::2] = P + 1000
    clamped = iz.copy(); clamped[::2] = P - 1
    out_d = torch.zeros((B, p.lwe_len), dtype=torch.int32, device="cuda")
    sg.gate3_gather(td(ops), td(pool), td(ix), td(iy), td(far), out_d)
    torch.cuda.synchronize()
    assert np.array_equal(out_d.cpu().numpy().view(np.uint32), sg.gate3_gather(ops, pool, ix, iy, clamped, out_h.copy()))
    with pytest.raises(mk.MktError, match="outside the pool"):
        sg.gate3_gather(ops, pool, ix, iy, iz + P, out_h)
    with pytest.raises(mk.MktError, match="unknown gate code"):
        sg.gate3_gather(np.full(B, 6, np.uint8), pool, ix, iy, iz, out_h)
    with pytest.raises(mk.MktError, match="empty pool"):
        sg.gate3_gather(ops, pool[:0], ix, iy, iz, out_h)
    sg.close()


@pytest.mark.parametrize("p", [mk.CGGIparam.scaled(n=12, N=256), mk.KMS2party.scaled(n=8, N=256), mk.CCS2party.scaled(n=12, N=256)], ids=lambda p: p.name)
def test_gate3_exact_mode_is_bootstrap_of_the_linear_part(require_gpu, p):
    """MKT_ARITH_EXACT: gate3_ops == the same context's bootstrapping! applied to the restated linear part, and it decrypts"""
    crs, keys = keygen(p, 37)
    sx = gpu_scheme(p, crs, keys, arith=mk.ARITH_EXACT)
    B = 12
    bits, (x, y, z) = _triples(p, keys, B, 38)
    ops = _random_ops(np.random.default_rng(39), B)
    got = sx.gate3_ops(ops, x, y, z)
    assert np.array_equal(got, sx.bootstrapping_(linear3_rows(ops, x, y, z)))
    assert np.array_equal(mk.lwe_decrypt(got, _keys(p, keys), p), plain3(ops, *bits))
    sx.close()


def test_full_adder_ripple_adder_on_the_engine(require_gpu):
    """ripple_adder_fa(8) through evaluate_on: one engine call per level (8), the words of evaluate(..., gate3_fn=oracle), a + b after
    decryption; the same words through evaluate_sharded on two logical shards (host arrays and GPU tensors); MultiScheme.gate3_ops and
    full_adder on a single context and on the multi handle"""
    import torch
    p = mk.KMS2party.scaled(n=16, N=256)
    crs, keys = keygen(p, 41)
    so, sg = oracle_scheme(p, crs, keys), gpu_scheme(p, crs, keys)
    circ = CI.ripple_adder_fa(8)
    B = 5
    rng = np.random.default_rng(42)
    bits = rng.integers(0, 2, (16, B)).astype(bool)
    inputs = [np.stack([mk.lwe_ith_encrypt(int(bits[i, j]), (i + j) % 2, keys[(i + j) % 2], p, deterministic_seed=4200 + 10 * i + j) for j in range(B)]) for i in range(16)]
    calls = []
    o2, o3 = sg.gate_gather, sg.gate3_gather
    sg.gate_gather = lambda *a: (calls.append(("g2", len(a[0]))), o2(*a))[1]
    sg.gate3_gather = lambda *a: (calls.append(("g3", len(a[0]))), o3(*a))[1]
    outs = CI.evaluate_on(circ, inputs, sg)
    assert calls == [("g2", 2 * B)] + [("g3", 2 * B)] * 7
    neg = lambda v: (0 - v.astype(np.int64)).astype(np.uint32)      # noqa: E731
    ref = CI.evaluate(circ, inputs, lambda op, x, y: so.gate_batch(op, x, y, threads=8), neg, gate3_fn=lambda ops, x, y, z: oracle_gate3(so, ops, x, y, z))
    for o, r in zip(outs, ref):
        assert np.array_equal(o, r)
    a = sum(bits[i].astype(int) << i for i in range(8)); b = sum(bits[8 + i].astype(int) << i for i in range(8))
    assert np.array_equal(sum(mk.lwe_decrypt(o, keys, p).astype(int) << i for i, o in enumerate(outs)), a + b)
    del sg.gate_gather, sg.gate3_gather
    outs_d = CI.evaluate_on(circ, [td(v) for v in inputs], sg)
    torch.cuda.synchronize()
    assert all(np.array_equal(od.cpu().numpy().view(np.uint32), o) for od, o in zip(outs_d, outs))
    multi = mk.setup_multi(p, [0, 0], keys=keys, a=crs)
    sh = CI.evaluate_sharded(circ, inputs, multi)
    sh_d = CI.evaluate_sharded(circ, [td(v) for v in inputs], multi)
    torch.cuda.synchronize()
    for o, s_, sd in zip(outs, sh, sh_d):
        assert np.array_equal(s_, o) and np.array_equal(sd.cpu().numpy().view(np.uint32), o)
    x, y, z = inputs[0], inputs[8], inputs[1]
    ops = _random_ops(rng, B)
    assert np.array_equal(multi.gate3_ops(ops, x, y, z), sg.gate3_ops(ops, x, y, z))
    assert np.array_equal(multi.gate3_ops(td(ops), td(x), td(y), td(z)).cpu().numpy().view(np.uint32), sg.gate3_ops(ops, x, y, z))
    assert np.array_equal(multi.gate3(mk.MAJ3_OP, x, y, z), sg.gate3(mk.MAJ3_OP, x, y, z))
    s1, c1 = mk.full_adder(x, y, z, sg)
    s2, c2 = mk.full_adder(x, y, z, multi)
    assert np.array_equal(s1, sg.gate3(mk.XOR3_OP, x, y, z)) and np.array_equal(c1, sg.gate3(mk.MAJ3_OP, x, y, z))
    assert np.array_equal(s1, s2) and np.array_equal(c1, c2)
    st, ct = mk.full_adder(td(x), td(y), td(z), sg)
    assert np.array_equal(st.cpu().numpy().view(np.uint32), s1) and np.array_equal(ct.cpu().numpy().view(np.uint32), c1)
    cnt = bits[0].astype(int) + bits[8] + bits[1]
    assert np.array_equal(mk.lwe_decrypt(s1, keys, p), cnt % 2 == 1) and np.array_equal(mk.lwe_decrypt(c1, keys, p), cnt >= 2)
    multi.close(); sg.close()


@pytest.mark.parametrize("p,B", [(mk.CGGIparam, 4096), (mk.KMS4party, 2048)], ids=lambda v: getattr(v, "name", str(v)))
def test_gate3_full_size_decrypts(require_gpu, p, B):
    """full-size sets with a negligible predicted three-input failure rate (tools/noise_theory.predict: 7.5e-9 / 7.3e-11 per gate): a few
    thousand random three-input gates (codes, NOT flags) with ZERO decrypt errors; an oracle sample.  The operands are GATE OUTPUTS, as
    inside a circuit (it is the operands' noise that a three-input gate adds up, and a fresh encryption's is far below a bootstrap's):
    each its own ciphertext -- CGGI: a fresh encryption bootstrapped once; KMS: a NAND fold over one fresh encryption per party, so that
    every party's rotation runs (bench.py `mixed` inputs)"""
    crs, keys = keygen(p, 43)
    sg = gpu_scheme(p, crs, keys)
    rng = np.random.default_rng(44)
    k = p.nparty
    bits, opnd = [], []
    for r in range(3):
        fb = rng.integers(0, 2, (k, B)).astype(bool)
        fresh = [np.stack([mk.lwe_ith_encrypt(int(fb[i, j]), i, keys[i], p, deterministic_seed=4400000 + 100000 * r + k * j + i) for j in range(B)])
                 for i in range(k)]
        acc, ab = fresh[0], fb[0]
        if k == 1:
            sg.bootstrapping_(acc)
        for i in range(1, k):
            acc, ab = mk.NAND(acc, fresh[i], sg), ~(ab & fb[i])
        assert np.array_equal(mk.lwe_decrypt(acc, _keys(p, keys), p), ab)
        bits.append(ab); opnd.append(acc)
    x, y, z = opnd
    ops = _random_ops(np.random.default_rng(45), B)
    got = sg.gate3_ops(ops, x, y, z)
    assert int((mk.lwe_decrypt(got, _keys(p, keys), p) != plain3(ops, *bits)).sum()) == 0
    so = oracle_scheme(p, crs, keys)
    assert np.array_equal(got[:2], oracle_gate3(so, ops[:2], x[:2], y[:2], z[:2]))
    sg.close()


def test_gate3_batches_past_one_workspace_chunk(require_gpu):
    """more gates than one workspace chunk (context.cpp CHUNK_GATES = 8192): the second chunk's operand, code and index offsets, in batch
    order (gate3_ops) and by row index from a pool (gate3_gather), host and device memory; an oracle sample across the chunk boundary and
    at the end, word for word"""
    import torch
    p = mk.CGGIparam.scaled(n=20, N=256)
    crs, keys = keygen(p, 49)
    so, sg = oracle_scheme(p, crs, keys), gpu_scheme(p, crs, keys)
    rng = np.random.default_rng(50)
    P, B = 64, 8192 + 37
    pool = encrypt_bits(p, keys, rng.integers(0, 2, P).astype(bool), seed=5000)
    ix, iy, iz = (rng.integers(0, P, B).astype(np.uint32) for _ in range(3))
    ops = (rng.integers(0, 6, B) | (rng.integers(0, 8, B) << 3)).astype(np.uint8)
    x, y, z = pool[ix], pool[iy], pool[iz]
    got = sg.gate3_ops(ops, x, y, z)
    sample = np.r_[0:3, 8189:8195, B - 3:B]
    assert np.array_equal(got[sample], oracle_gate3(so, ops[sample], x[sample], y[sample], z[sample]))
    assert np.array_equal(sg.gate3_ops(td(ops), td(x), td(y), td(z)).cpu().numpy().view(np.uint32), got)
    out_h = np.empty((B, p.lwe_len), dtype=np.uint32)
    sg.gate3_gather(ops, pool, ix, iy, iz, out_h)
    assert np.array_equal(out_h, got)
    big = torch.zeros((P + B, p.lwe_len), dtype=torch.int32, device="cuda")
    big[:P] = td(pool)
    sg.gate3_gather(td(ops), big, td(ix), td(iy), td(iz), big[P:])
    torch.cuda.synchronize()
    assert np.array_equal(big[P:].cpu().numpy().view(np.uint32), got)
    sg.close()


def test_gate3_oracle_parity_at_the_headline_set(require_gpu):
    """KMS2party_N1024_l2 (the headline shape): word-for-word parity on a sample, every code once.  Decryption is NOT asserted: the
    predicted three-input failure rate there is ~1e-3 per gate"""
    p = mk.KMS2party_N1024_l2
    crs, keys = keygen(p, 47)
    so, sg = oracle_scheme(p, crs, keys), gpu_scheme(p, crs, keys)
    bits, (x, y, z) = _triples(p, keys, 6, 48)
    ops = (np.arange(6) | (np.arange(6) % 8) << 3).astype(np.uint8)
    assert np.array_equal(sg.gate3_ops(ops, x, y, z), oracle_gate3(so, ops, x, y, z))
    sg.close()


def test_full_adder_c_example(require_gpu, tmp_path):
    """examples/full_adder.c: a plain C caller of mkt_gate3_batch_ops (header only), decrypted through mkt_client_*"""
    exe = str(tmp_path / "full_adder")
    lib = os.path.join(ROOT, "mktfhe_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "full_adder.c"),
                           "-o", exe, "-L" + lib, "-lmktfhe_hip", "-Wl,-rpath," + lib])
    out = subprocess.run([exe, "8", "256"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    assert "1 + 1 + 1 = carry 1, sum 1" in out.stdout
