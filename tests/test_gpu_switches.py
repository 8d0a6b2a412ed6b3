"""Every kernel-selection switch (INTEGRATION.md "Runtime switches") against the oracle, word for word.

The switches choose kernels, grid shapes and workgroup -> work mappings; the results must not depend on them.  Per-context
switches are set in process through Scheme.set_option.  The launcher-level switches (MKT_KS_*, MKT_FFT_*, MKT_NTT_GRID) are
read once per process, so each setting runs in a fresh child process (this file run as a script) that makes its own checks
against the oracle / the exact restatements and prints one JSON line.

SWITCHES lists every switch; tests/test_switches_cpu.py checks that it covers INTEGRATION.md's table and mkt_set_option,
and that every entry appears in a parametrised case below.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import (GATE_FUNCS, O, ROOT, bits_equal, edge_words, encrypt_bits, gpu_scheme, keygen, ks_edge_check, ks_expected, ks_ran,
                     mixed_party_check, mk, oracle_scheme)

pytestmark = pytest.mark.gpu

# per-context options (mkt_set_option) and the environment variables that seed them / the launcher
SWITCHES = [
    "rot_variant", "rot_stagger", "rot_split", "rot_wide", "rot_blkg", "ccs_stagger", "ccs_pipe", "exact_wide", "exact_impl",
    "rot_map", "fx_polymul_force", "exact_kany",
    "MKT_ROT_WIDE", "MKT_ROT_BLKG", "MKT_ROT_VARIANT", "MKT_ROT_SPLIT", "MKT_ROT_STAGGER", "MKT_CCS_STAGGER", "MKT_CCS_PIPE",
    "MKT_EXACT_IMPL", "MKT_EXACT_WIDE", "MKT_EXACT_KANY", "MKT_ROT_MAP",
    "MKT_KS_G", "MKT_KS_WAVES", "MKT_KS_BLOCKS", "MKT_KS_PAIR", "MKT_KS_MFMA", "MKT_FFT_NB", "MKT_FFT_GRID", "MKT_FFT_IGRID", "MKT_NTT_GRID",
]


def _sample(B, rng, n=4):
    return sorted({0, B - 1, *rng.integers(0, B, n).tolist()})


def _ctx_check(p, opts, B=5, seed=1):
    """Options `opts` set on a fresh context: blindrotate_ on given accumulators (skipped and
    full-turn mask words included), KMS phase 1 (Float64 bits), all six gates, and for multi-key sets the dense all-party check."""
    crs, keys = keygen(p, seed)
    so = oracle_scheme(p, crs, keys)
    sg = gpu_scheme(p, crs, keys)
    for k, v in opts.items():
        sg.set_option(k, v)
    rng = np.random.default_rng(seed + 7)
    bits = rng.integers(0, 2, 2 * B).astype(bool)
    c = encrypt_bits(p, keys, bits, seed=500 + seed)
    x, y = c[:B], c[B:]
    lin = np.stack([O.gate_linear(0, x[j], y[j]) for j in range(B)])
    at, bt = sg.modswitch(lin)
    at[0, :3] = [0, 2 * p.N, p.N]
    acc0 = np.stack([so.testvector(bt[j]) for j in range(B)])
    acc_o = np.stack([so.blindrotate(at[j], acc0[j]) for j in range(B)])
    assert np.array_equal(sg.blindrotate_(at, acc0.astype(p.ring_dtype).copy()).astype(np.uint64), acc_o), ("blindrotate", opts)
    if p.scheme in (mk.KMS, mk.KMS_BLOCK):
        lev = sg.kms_phase1(at)
        for j in (0, B - 1):
            row = 0
            for party in range(p.k):
                lev_o = so.kms_phase1(party, at[j, party * p.n:(party + 1) * p.n])
                assert bits_equal(lev[j, row:row + lev_o.shape[0]], lev_o), ("phase1", j, party, opts)
                row += lev_o.shape[0]
    for op in range(6):
        out = sg.gate(op, x, y)
        assert np.array_equal(out, np.stack([so.gate(op, x[j], y[j]) for j in range(B)])), (f"gate {op}", opts)
        assert np.array_equal(mk.lwe_decrypt(out, keys if p.multikey else keys[0], p), GATE_FUNCS[op](bits[:B], bits[B:]))
    if p.multikey:
        mixed_party_check(p, keys, so, sg, rng)
    sg.close()


def _sid(p):
    return f"{p.name}-n{p.n}-N{p.N}-b{p.blk_len}"


# ---- rot_variant: single (21) / paired (22) digit transforms of the plain and block rotation kernels.  rot_wide = 1 keeps the
# latency kernel (which ignores the variant) out; rot_blkg = 1 keeps the block sets on blindrotate_k1_kernel<LB>.
VARIANT_SETS = [
    mk.CGGIparam.scaled(n=20, N=256), mk.KMS2party.scaled(n=12, N=256), mk.CGGI_N1024_l2.scaled(n=10), mk.KMS2party_N1024_l2.scaled(n=8),
    mk.CGGIparam.scaled(n=6, N=4096),
    mk.Blockparam.scaled(n=24, N=256, blk_d=12, blk_len=2), mk.Blockparam.scaled(n=30, N=256, blk_d=10),
    mk.Blockparam.scaled(n=24, N=512, blk_d=6, blk_len=4), mk.KMS2partyblock.scaled(n=12, N=2048, blk_d=4),
]
VARIANT_CASES = [{"rot_variant": v, "rot_wide": 1, "rot_blkg": 1} for v in (21, 22)]


@pytest.mark.parametrize("opts", VARIANT_CASES, ids=lambda o: f"v{o['rot_variant']}")
@pytest.mark.parametrize("p", VARIANT_SETS, ids=_sid)
def test_rot_variant(require_gpu, p, opts):
    if p.N // 2 < 2048:
        _ctx_check(p, opts)
        return
    # M = 2048: the paired form may not fit the LDS budget.  Either the oracle's words, or a refused call after which the same
    # context gives the oracle's words under the default.  Never other words.
    crs, keys = keygen(p, 1)
    so = oracle_scheme(p, crs, keys)
    sg = gpu_scheme(p, crs, keys)
    for k, v in opts.items():
        sg.set_option(k, v)
    c = encrypt_bits(p, keys, [1, 0, 1, 1, 0, 1], seed=41)
    want = np.stack([so.gate(0, c[j], c[3 + j]) for j in range(3)])
    try:
        out = sg.gate(0, c[:3], c[3:])
        refused = False
    except mk.MktError:
        refused = True
        sg.set_option("rot_variant", 0)
        out = sg.gate(0, c[:3], c[3:])
    assert np.array_equal(out, want)
    sg.close()
    print(f"rot_variant={opts['rot_variant']} at M = {p.N // 2}: {'refused' if refused else 'words'}")
    if not refused:
        _ctx_check(p, opts)


# ---- rot_map: slot-major (0) / rows of one (ciphertext, party) eight ids apart (1).  Batches not multiples of 8 (the g8 < 8 tail).
MAP_SETS = [
    (mk.CGGIparam.scaled(n=20, N=256), {"rot_wide": 1}),
    (mk.KMS4party.scaled(n=10, N=256), {"rot_wide": 1}),
    (mk.KMS2party_N1024_l2.scaled(n=8), {"rot_wide": 1}),
    (mk.Blockparam.scaled(n=30, N=256, blk_d=10), {"rot_wide": 1, "rot_blkg": 1}),
    (mk.CGGIparam.scaled(n=20, N=512), {"rot_wide": 2}),                     # the latency kernel forced
    (mk.KMS2party_N1024_l2.scaled(n=8), {"rot_wide": 2}),
]


@pytest.mark.parametrize("rot_map", [0, 1])
@pytest.mark.parametrize("p,extra", MAP_SETS, ids=lambda v: _sid(v) if isinstance(v, mk.Params) else "w" + str(v.get("rot_wide")))
def test_rot_map(require_gpu, p, extra, rot_map):
    _ctx_check(p, {**extra, "rot_map": rot_map}, B=13, seed=2)


def _planned(p, B, seed):
    crs, keys = keygen(p, seed)
    so = oracle_scheme(p, crs, keys)
    sg = gpu_scheme(p, crs, keys)
    rng = np.random.default_rng(seed + 1)
    bits = rng.integers(0, 2, 2 * B).astype(bool)
    uniq = encrypt_bits(p, keys, bits[:64], seed=100 * seed)
    idx = rng.integers(0, 64, 2 * B)
    c = uniq[idx]
    return so, sg, c[:B], c[B:], rng


@pytest.mark.parametrize("opt,values", [("rot_map", (0, 1)), ("rot_split", (1, 3, 7, 100))])
@pytest.mark.parametrize("B", [1024 + 100, 1024 + 400])
def test_planned_launches_meet_map_and_split(require_gpu, B, opt, values):
    """The planned launches of test_rotation_launch_plans_agree (block0 > 0: a latency launch after one fill, two equal launches)
    under every map / split: the whole batch equals the default's words, a sample the oracle's."""
    p = mk.CGGIparam.scaled(n=8)
    so, sg, x, y, rng = _planned(p, B, 71)
    ref = sg.gate(0, x, y)
    js = _sample(B, rng, 6)
    assert np.array_equal(ref[js], so.gate_batch(0, x[js], y[js], threads=8))
    for v in values:
        sg.set_option(opt, v)
        assert np.array_equal(sg.gate(0, x, y), ref), (opt, v)
    sg.close()


# ---- rot_split: rotations per launch (-1 / past the batch: one launch)
SPLIT_SETS = [(mk.CGGIparam.scaled(n=20, N=256), {"rot_wide": 1}), (mk.KMS2party_N1024_l2.scaled(n=8), {"rot_wide": 1}),
              (mk.Blockparam.scaled(n=30, N=256, blk_d=10), {"rot_wide": 1, "rot_blkg": 1}), (mk.CGGIparam.scaled(n=20, N=512), {"rot_wide": 2})]


@pytest.mark.parametrize("rot_split", [1, 3, 7, 100])
@pytest.mark.parametrize("p,extra", SPLIT_SETS, ids=lambda v: _sid(v) if isinstance(v, mk.Params) else "w" + str(v.get("rot_wide")))
def test_rot_split(require_gpu, p, extra, rot_split):
    _ctx_check(p, {**extra, "rot_split": rot_split}, B=13, seed=3)


# ---- EXACT on the Float64 pipe (exact_impl = 1): map and split reach fx_blindrotate_kernel through FxRotArgs
FX_SETS = [mk.CGGIparam.scaled(n=12, N=256), mk.KMS2party_N1024_l2.scaled(n=8), mk.KMS2party.scaled(n=8, N=256)]
FX_CASES = [{"exact_impl": 1, "rot_map": 0}, {"exact_impl": 1, "rot_map": 1}, {"exact_impl": 1, "rot_split": -1}, {"exact_impl": 1, "rot_split": 3},
            {"exact_impl": 1, "rot_split": 100}, {"exact_impl": 1, "rot_map": 0, "rot_split": 7}]


def _exact_scheme(p, crs, keys):
    sx = mk.Scheme(p, arith=mk.ARITH_EXACT)
    if p.multikey:
        sx.load_crs(crs)
    for i, kk in enumerate(keys):
        sx.load_party(i, kk)
    return sx


@pytest.mark.parametrize("opts", FX_CASES, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
@pytest.mark.parametrize("p", FX_SETS, ids=_sid)
def test_fx_pipe_map_and_split(require_gpu, p, opts):
    """Accumulators and gate outputs equal the big-integer restatement (tests/ref_exact.py), and the integer NTT's words over an odd batch."""
    import ref_exact as RX
    crs, keys = keygen(p, 51)
    so = oracle_scheme(p, crs, keys)
    sx = _exact_scheme(p, crs, keys)
    for k, v in opts.items():
        sx.set_option(k, v)
    assert sx.get_metric("fx_available") == 1.0
    B = 9 if p.multikey else 13
    rng = np.random.default_rng(52)
    bits = rng.integers(0, 2, 2 * B).astype(bool)
    c = encrypt_bits(p, keys, bits, seed=5200)
    x, y = c[:B], c[B:]
    lin = np.stack([O.gate_linear(0, x[j], y[j]) for j in range(B)])
    at, bt = sx.modswitch(lin)
    at[0, :2] = [0, 2 * p.N]
    acc0 = np.stack([so.testvector(bt[j]) for j in range(B)]).astype(p.ring_dtype)
    acc_x = sx.blindrotate_(at, acc0.copy())
    assert sx.last_kernel_name() == "fx_blindrotate_kernel"
    for j in (0, B - 1):
        want = RX.kms_blindrotate(p, keys, crs, at[j], acc0[j]) if p.multikey else RX.blindrotate(p, keys[0].brk, at[j], acc0[j])
        assert np.array_equal(acc_x[j].astype(np.uint64).reshape(want.shape), want), j
    out = sx.gate(0, x, y)
    js = (0, B - 1)
    want = [RX.kms_gate(p, so, keys, crs, 0, x[j], y[j]) if p.multikey else RX.gate(p, so, keys[0].brk, 0, x[j], y[j]) for j in js]
    assert np.array_equal(out[list(js)], np.stack(want))
    sx.set_option("exact_impl", 0)
    assert np.array_equal(sx.blindrotate_(at, acc0.copy()), acc_x) and np.array_equal(sx.gate(0, x, y), out)
    sx.close()


def test_fx_headline_shape_chunk_rule_against_splits(require_gpu):
    """EXACT KMS at W = 64, M = 512 with more than 1024 rotations: the default chunk rule (split 0: one launch per chip-fill) against
    one launch (-1) and other splits, whole batch; a sample against ref_exact."""
    import ref_exact as RX
    p = mk.KMS2party_N1024_l2.scaled(n=6)
    crs, keys = keygen(p, 53)
    so = oracle_scheme(p, crs, keys)
    sx = _exact_scheme(p, crs, keys)
    sx.set_option("exact_impl", 1)
    B = 520
    rng = np.random.default_rng(54)
    bits = rng.integers(0, 2, 2 * B).astype(bool)
    uniq = encrypt_bits(p, keys, bits[:32], seed=5400)
    c = uniq[rng.integers(0, 32, 2 * B)]
    x, y = c[:B], c[B:]
    lin = np.stack([O.gate_linear(0, x[j], y[j]) for j in range(B)])
    at, _ = sx.modswitch(lin)
    lev = sx.kms_phase1(at)
    assert lev.shape[0] * lev.shape[1] > 1024 and sx.last_kernel_name() == "fx_blindrotate_kernel"
    out = sx.gate(0, x, y)
    for v in (-1, 100, 1000):
        sx.set_option("rot_split", v)
        assert np.array_equal(sx.gate(0, x, y), out), v
        assert np.array_equal(sx.kms_phase1(at).view(np.uint64), lev.view(np.uint64)), v
    for j in (0, B - 1):
        assert np.array_equal(out[j], RX.kms_gate(p, so, keys, crs, 0, x[j], y[j])), j
    sx.close()


# ---- stagger: the sleep branches run from workgroup 256 on (CCS: (g >> 8) & 3 != 0), so every batch holds >= 512 workgroups.
# The whole batch against the default setting, a sample against the oracle.
STAGGER_CASES = [
    (mk.CGGIparam.scaled(n=8, N=256), 600, {"rot_wide": 1}, "rot_stagger", (0, 64)),
    (mk.KMS2party.scaled(n=6, N=256), 300, {"rot_wide": 1}, "rot_stagger", (0, 64)),
    (mk.Blockparam.scaled(n=12, N=256, blk_d=4), 600, {"rot_blkg": 1}, "rot_stagger", (0, 64)),
    (mk.Blockparam.scaled(n=12, N=256, blk_d=4), 2100, {"rot_blkg": 4}, "rot_stagger", (0, 64)),     # rot_block.hip: four rotations per workgroup
    (mk.CCS2party.scaled(n=6, N=256), 600, {"ccs_pipe": 0}, "ccs_stagger", (0, 3)),
    (mk.CCS2party.scaled(n=6, N=256), 600, {"ccs_pipe": 1}, "ccs_stagger", (0, 3)),
]


@pytest.mark.parametrize("p,B,extra,opt,values", STAGGER_CASES, ids=lambda v: _sid(v) if isinstance(v, mk.Params) else str(v))
def test_stagger(require_gpu, p, B, extra, opt, values):
    so, sg, x, y, rng = _planned(p, B, 61)
    ref = sg.gate(0, x, y)
    js = _sample(B, rng)
    assert np.array_equal(ref[js], so.gate_batch(0, x[js], y[js], threads=8))
    for k, v in extra.items():
        sg.set_option(k, v)
    for v in values:
        sg.set_option(opt, v)
        out = sg.gate(0, x, y)
        assert np.array_equal(out, ref), (opt, v, extra)
    sg.close()


@pytest.mark.parametrize("rot_stagger", [0, 64])
def test_stagger_fx_pipe(require_gpu, rot_stagger):
    """the sleep branch of fx_blindrotate_kernel (EXACT, Float64 pipe): 600 rotations against the default setting and ref_exact"""
    import ref_exact as RX
    p = mk.CGGIparam.scaled(n=8, N=256)
    crs, keys = keygen(p, 63)
    so = oracle_scheme(p, crs, keys)
    sx = _exact_scheme(p, crs, keys)
    sx.set_option("exact_impl", 1)
    B = 600
    rng = np.random.default_rng(64)
    c = encrypt_bits(p, keys, rng.integers(0, 2, 64).astype(bool), seed=6400)[rng.integers(0, 64, 2 * B)]
    x, y = c[:B], c[B:]
    ref = sx.gate(0, x, y)
    sx.set_option("rot_stagger", rot_stagger)
    out = sx.gate(0, x, y)
    assert sx.last_kernel_name() == "fx_blindrotate_kernel" and np.array_equal(out, ref)
    for j in (0, B - 1):
        assert np.array_equal(out[j], RX.gate(p, so, keys[0].brk, 0, x[j], y[j]))
    sx.close()


# ---- the other per-context switches, here so that every entry of SWITCHES has a case of its own (their kernels have dedicated
# parity tests too: tests/test_gpu_parity.py, tests/test_gpu_fx.py)
@pytest.mark.parametrize("opts", [{"rot_wide": 2}, {"rot_blkg": 2}, {"ccs_pipe": 1}], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_other_rotation_switches(require_gpu, opts):
    p = {"rot_wide": mk.KMS2party.scaled(n=10, N=512), "rot_blkg": mk.Blockparam.scaled(n=30, N=256, blk_d=10),
         "ccs_pipe": mk.CCS2party.scaled(n=8, N=256)}[next(iter(opts))]
    _ctx_check(p, opts, B=5, seed=4)


@pytest.mark.parametrize("opts", [{"exact_impl": 0, "exact_wide": 0}, {"exact_impl": 0, "exact_kany": 1}], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_exact_kernel_switches(require_gpu, opts):
    import ref_exact as RX
    p = mk.KMS2party_N1024_l2.scaled(n=6, N=256) if "exact_wide" in opts else mk.CGGIparam.scaled(n=8, N=256, k=2)
    crs, keys = keygen(p, 55)
    so = oracle_scheme(p, crs, keys)
    sx = _exact_scheme(p, crs, keys)
    for k, v in opts.items():
        sx.set_option(k, v)
    c = encrypt_bits(p, keys, [1, 0, 1, 1, 0, 1], seed=5500)
    out = sx.gate(0, c[:3], c[3:])
    want = [RX.kms_gate(p, so, keys, crs, 0, c[j], c[3 + j]) if p.multikey else RX.gate(p, so, keys[0].brk, 0, c[j], c[3 + j]) for j in range(3)]
    assert np.array_equal(out, np.stack(want))
    sx.close()


@pytest.mark.parametrize("opts", [{"fx_polymul_force": 0}, {"fx_polymul_force": 1}], ids=lambda o: f"force{o['fx_polymul_force']}")
def test_fx_polymul_force(require_gpu, opts):
    """fx_polymul_force on certified operands: the Float64 product kernel serves either way, the schoolbook product's words"""
    N, W = 256, 32
    p = mk.CGGIparam.scaled(n=8, N=N, W=W)
    ex = mk.Scheme(p, arith=mk.ARITH_EXACT)
    ex.set_option("exact_impl", 1)
    ex.set_option("fx_polymul_force", opts["fx_polymul_force"])
    rng = np.random.default_rng(56)
    a = (rng.integers(-256, 256, (5, N)).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    b = np.stack([edge_words(W, N, rng) for _ in range(5)]).astype(np.uint32)
    got = ex.exact_polymul(a, b)
    assert "fx" in ex.last_kernel_name()
    for j in range(5):
        assert np.array_equal(got[j].astype(np.uint64), O.negacyclic(a[j].astype(np.uint64), b[j].astype(np.uint64), W))
    ex.close()


def test_set_option_refuses_values_outside_the_documented_sets(require_gpu):
    """rot_variant outside {0, 21, 22} and rot_map outside {0, 1} are refused with MKT_ERR_ARG; the context keeps its previous value
    (rot_variant = 23 at l = 3 used to fail late, inside a gate call)"""
    p = mk.CGGIparam.scaled(n=12, N=256)
    crs, keys = keygen(p, 57)
    so = oracle_scheme(p, crs, keys)
    sg = gpu_scheme(p, crs, keys)
    sg.set_option("rot_wide", 1)
    sg.set_option("rot_variant", 21)
    sg.set_option("rot_map", 0)
    for name, bad in (("rot_variant", 23), ("rot_variant", 1), ("rot_variant", -1), ("rot_map", 2), ("rot_map", -1)):
        with pytest.raises(mk.MktError) as e:
            sg.set_option(name, bad)
        assert e.value.code == -1 or "not one of" in str(e.value)
    c = encrypt_bits(p, keys, [1, 0, 1, 1, 0, 1, 0, 0], seed=5700)
    assert np.array_equal(sg.gate(0, c[:4], c[4:]), np.stack([so.gate(0, c[j], c[4 + j]) for j in range(4)]))
    sg.close()


# ---- the per-context switches seeded from the environment at context creation (Tune::from_env), then never read again
ENV_SEED_CASES = [
    ({"MKT_ROT_VARIANT": "21", "MKT_ROT_WIDE": "1", "MKT_ROT_SPLIT": "3", "MKT_ROT_MAP": "0", "MKT_ROT_STAGGER": "0"}, mk.CGGIparam.scaled(n=20, N=256)),
    ({"MKT_ROT_WIDE": "2", "MKT_ROT_MAP": "0"}, mk.KMS2party.scaled(n=10, N=512)),
    ({"MKT_ROT_BLKG": "4"}, mk.Blockparam.scaled(n=30, N=256, blk_d=10)),
    ({"MKT_CCS_PIPE": "1", "MKT_CCS_STAGGER": "3"}, mk.CCS2party.scaled(n=8, N=256)),
    ({"MKT_EXACT_IMPL": "0", "MKT_EXACT_WIDE": "0"}, mk.KMS2party_N1024_l2.scaled(n=6, N=256)),
    ({"MKT_EXACT_IMPL": "0", "MKT_EXACT_KANY": "1"}, mk.CGGIparam.scaled(n=8, N=256, k=2)),
]


@pytest.mark.parametrize("env,p", ENV_SEED_CASES, ids=lambda v: _sid(v) if isinstance(v, mk.Params) else "-".join(f"{k[4:]}{x}" for k, x in v.items()))
def test_context_switches_seeded_from_the_environment(require_gpu, env, p, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if "MKT_EXACT_IMPL" not in env:
        _ctx_check(p, {}, B=5, seed=6)
        return
    import ref_exact as RX
    crs, keys = keygen(p, 58)
    so = oracle_scheme(p, crs, keys)
    sx = _exact_scheme(p, crs, keys)
    c = encrypt_bits(p, keys, [1, 0, 1, 1, 0, 1], seed=5800)
    out = sx.gate(0, c[:3], c[3:])
    name = sx.last_kernel_name()
    assert "fx_" not in name and ("kany" in name) == ("MKT_EXACT_KANY" in env), name
    want = [RX.kms_gate(p, so, keys, crs, 0, c[j], c[3 + j]) if p.multikey else RX.gate(p, so, keys[0].brk, 0, c[j], c[3 + j]) for j in range(3)]
    assert np.array_equal(out, np.stack(want))
    sx.close()


# ---- default grid-stride of the batched Float64 transforms (no switch): batches past twice the cap (two rows in flight per workgroup)
@pytest.mark.parametrize("N,W,B", [(2048, 64, 2 * 4096 + 37), (64, 32, 2 * 32768 + 5)])
def test_transform_default_grid_stride(require_gpu, N, W, B):
    rng = np.random.default_rng(N + B)
    p = mk.CGGIparam.scaled(n=8, N=N, W=W)
    s = mk.Scheme(p)
    f = O.Ffter(N, W)
    polys = rng.integers(0, 1 << 63, (B, N), dtype=np.uint64) & np.uint64((1 << W) - 1)
    polys[:8] = np.stack([edge_words(W, N, rng) for _ in range(8)])
    polys[-8:] = np.stack([edge_words(W, N, rng) for _ in range(8)])
    t_gpu = s.transform_fwd(polys.astype(p.ring_dtype))
    t_ref = f.fwd(polys)
    assert bits_equal(t_gpu, t_ref)
    assert np.array_equal(s.transform_inv(t_ref).astype(np.uint64), f.inv(t_ref))
    s.close()


# ---- process-wide launcher switches: one child process per setting, strictly one at a time
# The first eleven select among the older key-switch kernels, which run where the matrix cores do not: they name MKT_KS_MFMA = 0, or every
# unbalanced D = 4 set of the child would run ks_mfma_kernel whatever else the setting says (ks_plan asks the matrix cores first).  The last
# three: the matrix cores forced, forced with switches of the older kernels beside them (which then choose nothing), and automatic.
# Every child reports which kernel each of its key switches ran; the parent holds the report to helpers.ks_expected
KS_SETTINGS = [{**e, "MKT_KS_MFMA": "0"} for e in (
    {"MKT_KS_PAIR": "0"}, {"MKT_KS_G": "8"}, {"MKT_KS_G": "16"}, {"MKT_KS_WAVES": "1"}, {"MKT_KS_WAVES": "2"},
    {"MKT_KS_PAIR": "0", "MKT_KS_WAVES": "1"}, {"MKT_KS_PAIR": "0", "MKT_KS_WAVES": "2"}, {"MKT_KS_BLOCKS": "1"},
    {"MKT_KS_BLOCKS": "100000"}, {"MKT_KS_G": "12"}, {"MKT_KS_G": "64"})]
KS_SETTINGS += [{"MKT_KS_MFMA": "1"}, {"MKT_KS_MFMA": "1", "MKT_KS_G": "8", "MKT_KS_PAIR": "0"}, {"MKT_KS_MFMA": "-1"}]
# What each setting is WRITTEN to reach, (kernel, G, waves), on a set with unbalanced digits, D = 4 and an even digit count (the child's first,
# CGGIparam): helpers.ks_expected says what a setting implies, this says what it is for -- an entry that lost its "MKT_KS_MFMA": "0" would
# still run what it implies (the matrix cores) and no longer what it is for.  tests/test_ks_plan_cpu.py holds the list to the rule without a GPU
KS_MEANT = [(1, 32, 4), (1, 8, 1), (1, 16, 1), (2, 32, 1), (2, 32, 2), (1, 32, 1), (1, 32, 2), (2, 32, 4), (2, 32, 4), (2, 32, 4), (2, 32, 4),
            (3, 32, 4), (3, 32, 4), (3, 32, 4)]
FFT_SETTINGS = [{"MKT_FFT_NB": "2"}, {"MKT_FFT_GRID": "1", "MKT_FFT_IGRID": "3"}, {"MKT_FFT_GRID": "3", "MKT_FFT_IGRID": "1"},
                {"MKT_FFT_NB": "2", "MKT_FFT_GRID": "3"}]
NTT_SETTINGS = [{"MKT_NTT_GRID": "1"}, {"MKT_NTT_GRID": "3"}]
CHILD_CASES = [("ks", e) for e in KS_SETTINGS] + [("fft", e) for e in FFT_SETTINGS] + [("ntt", e) for e in NTT_SETTINGS]
CHILD_TIMEOUT = {"ks": 300, "fft": 180, "ntt": 240}
_child_fault = []          # a child that died by a signal / abort / segfault / time limit: no further child is started


def _run_child(kind, setting):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MKT_") or k == "MKT_LIB_PATH"}     # (MKT_LIB_PATH names the library, it is no switch)
    env.update(setting)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), kind], env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT[kind], cwd=ROOT)
    except subprocess.TimeoutExpired:
        _child_fault.append((kind, setting, "time limit"))
        raise
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137):
        _child_fault.append((kind, setting, r.returncode))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, f"child {kind} {setting}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return json.loads(lines[-1])


@pytest.mark.parametrize("kind,setting", CHILD_CASES, ids=lambda v: v if isinstance(v, str) else "-".join(f"{k[4:]}{x}" for k, x in v.items()))
def test_launcher_switch_in_a_child_process(require_gpu, kind, setting):
    assert not _child_fault, f"an earlier child process faulted: {_child_fault}"
    j = _run_child(kind, setting)
    assert j["ok"] and j["checks"] > 0 and j["env"] == setting, j
    if kind == "ks":
        assert_ks_ran(j["ran"], setting)


# the sets of the key-switch child: random accumulators at four batches and one NAND each, then (edge_cases.py) the gadget's own boundaries
KS_PLAIN_SETS = [(p, (1, 33, 257, 1000)) for p in (
    mk.CGGIparam, mk.CGGIparam.scaled(n=20, N=256), mk.KMS2party.scaled(n=12, N=256), mk.CCS2party.scaled(n=12, N=256),
    mk.Blockparam.scaled(n=30, N=256, blk_d=10), mk.KMS2partyblock.scaled(n=24, N=256, blk_d=8))]
KS_NAND_BATCH = 33


def ks_child_calls():
    """[(set, batch)] of every key switch the child reports, in its order; the report's keys are "<position of the set>:<batch>" """
    from edge_cases import KS_BATCHES, KS_CHILD_FULL, KS_CHILD_SETS
    calls = [(p, batches + (KS_NAND_BATCH,)) for p, batches in KS_PLAIN_SETS]
    return calls + [KS_CHILD_FULL] + [(q, KS_BATCHES) for q in KS_CHILD_SETS]


def assert_ks_ran(ran, setting):
    """every key switch of the child ran the kernel, tile width and wave count that its set and the setting imply"""
    calls = ks_child_calls()
    assert setting in KS_SETTINGS and calls[0][0] == mk.CGGIparam
    meant = KS_MEANT[KS_SETTINGS.index(setting)]
    assert all(tuple(ran[f"0:{B}"]) == meant for B in calls[0][1]), (setting, "is written to reach (kernel, G, waves)", meant, "and ran", [ran[f"0:{B}"] for B in calls[0][1]])
    assert sorted(ran) == sorted(f"{i}:{B}" for i, (_, batches) in enumerate(calls) for B in set(batches)), sorted(ran)
    for i, (p, batches) in enumerate(calls):
        for B in batches:
            assert tuple(ran[f"{i}:{B}"]) == ks_expected(p, setting), (setting, _sid(p), p.f, p.logD, B, "ran (kernel, G, waves)", ran[f"{i}:{B}"], "implied", ks_expected(p, setting))


# ---- child side
def _child_ks():
    """-> (checks, {"<position in ks_child_calls()>:<batch>": what that key switch ran})"""
    rng = np.random.default_rng(91)
    checks, ran = 0, {}
    for i, (p, batches) in enumerate(KS_PLAIN_SETS):
        crs, keys = keygen(p, 92)
        so = oracle_scheme(p, crs, keys)
        sg = gpu_scheme(p, crs, keys)
        assert ks_ran(sg)[0] == 0, "no key switch yet"
        for B in batches:
            acc = rng.integers(0, 2**p.W, (B, 1 + p.k, p.N), dtype=np.uint64)
            out = sg.keyswitch(acc.astype(p.ring_dtype))
            ran[f"{i}:{B}"] = ks_ran(sg)
            for j in _sample(B, rng):
                assert np.array_equal(out[j], so.keyswitch(acc[j])), (p.name, p.n, B, j)
                checks += 1
        B = KS_NAND_BATCH
        c = encrypt_bits(p, keys, rng.integers(0, 2, 2 * B).astype(bool), seed=9300)
        out = sg.gate(0, c[:B], c[B:])
        assert ran[f"{i}:{B}"] == ks_ran(sg), "the gate's key switch runs what the plain call of its batch ran"
        js = _sample(B, rng)
        assert np.array_equal(out[js], so.gate_batch(0, c[:B][js], c[B:][js], threads=8)), (p.name, "NAND")
        checks += len(js)
        sg.close()
    # the key-switch gadget's own boundaries (tests/test_gpu_edges.py), every ciphertext compared
    for i, (p, batches) in list(enumerate(ks_child_calls()))[len(KS_PLAIN_SETS):]:      # the full key length first: the launcher settings tile it
        crs, keys = keygen(p, 98)
        sg = gpu_scheme(p, crs, keys)
        checks += ks_edge_check(p, oracle_scheme(p, crs, keys), sg, rng, batches, after=lambda B: ran.__setitem__(f"{i}:{B}", ks_ran(sg)))
        sg.close()
    return checks, ran


def _child_fft():
    checks = 0
    rng = np.random.default_rng(94)
    for N in (256, 1024):
        for W in (32, 64):
            p = mk.CGGIparam.scaled(n=8, N=N, W=W)
            s = mk.Scheme(p)
            f = O.Ffter(N, W)
            polys = np.stack([edge_words(W, N, rng) for _ in range(37)])
            t = s.transform_fwd(polys.astype(p.ring_dtype))
            assert bits_equal(t, f.fwd(polys)), (N, W, "fwd")
            assert np.array_equal(s.transform_inv(t).astype(np.uint64), f.inv(t)), (N, W, "inv")
            checks += 2
            s.close()
    for p in (mk.CGGIparam.scaled(n=12, N=256), mk.KMS2party.scaled(n=8, N=256)):      # key upload through the capped grid
        crs, keys = keygen(p, 95)
        so = oracle_scheme(p, crs, keys)
        sg = gpu_scheme(p, crs, keys)
        c = encrypt_bits(p, keys, rng.integers(0, 2, 10).astype(bool), seed=9500)
        assert np.array_equal(sg.gate(0, c[:5], c[5:]), so.gate_batch(0, c[:5], c[5:], threads=5)), p.name
        checks += 1
        sg.close()
    return checks


def _child_ntt():
    import ref_exact as RX
    import ref_ntt as R
    checks = 0
    rng = np.random.default_rng(96)
    for N, W in ((256, 32), (1024, 64), (2048, 64)):
        p = mk.CGGIparam.scaled(n=8, N=N, W=W)
        ex = mk.Scheme(p, arith=mk.ARITH_EXACT)
        ex.set_option("exact_impl", 0)
        polys = np.stack([edge_words(W, N, rng) for _ in range(37)]).astype(p.ring_dtype)
        t = ex.transform_fwd(polys).view(np.uint64)
        for b in (0, 36):
            if N <= 1024:
                assert [int(v) for v in t[b]] == R.fwd(polys[b], W), (N, W, b)
                assert [int(v) for v in ex.transform_inv(t.view(np.complex128))[b]] == R.inv([int(v) for v in t[b]], W), (N, W, b)
                checks += 2
        a = rng.integers(-256, 256, (37, N)).astype(np.int64)
        aw = a.astype(np.uint64).astype(p.ring_dtype) if W == 64 else (a & 0xFFFFFFFF).astype(np.uint32)
        got = ex.exact_polymul(aw, polys)
        for b in (0, 17, 36):
            assert np.array_equal(got[b].astype(np.uint64), O.negacyclic(aw[b].astype(np.uint64) & np.uint64((1 << W) - 1), polys[b].astype(np.uint64), W)), (N, W, b)
            checks += 1
        ex.close()
    for p in (mk.KMS2party.scaled(n=6, N=256), mk.CGGIparam.scaled(n=10, N=256)):          # split / unsplit key tables uploaded through the capped grid
        crs, keys = keygen(p, 97)
        so = oracle_scheme(p, crs, keys)
        sx = _exact_scheme(p, crs, keys)
        sx.set_option("exact_impl", 0)
        c = encrypt_bits(p, keys, [1, 0, 1, 1], seed=9700)
        out = sx.gate(0, c[:2], c[2:])
        for j in range(2):
            want = RX.kms_gate(p, so, keys, crs, 0, c[j], c[2 + j]) if p.multikey else RX.gate(p, so, keys[0].brk, 0, c[j], c[2 + j])
            assert np.array_equal(out[j], want), (p.name, j)
            checks += 1
        sx.close()
    return checks


if __name__ == "__main__":
    kind = sys.argv[1]
    env = {k: v for k, v in os.environ.items() if k.startswith("MKT_") and k != "MKT_LIB_PATH"}
    try:
        n = {"ks": _child_ks, "fft": _child_fft, "ntt": _child_ntt}[kind]()
        n, ran = n if kind == "ks" else (n, None)
        print(json.dumps({"kind": kind, "env": env, "ok": True, "checks": n, **({"ran": ran} if kind == "ks" else {})}))
    except AssertionError as e:
        print(json.dumps({"kind": kind, "env": env, "ok": False, "checks": 0, "error": repr(e)[:2000]}))
        sys.exit(1)
