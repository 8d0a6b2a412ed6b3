"""The key switch on the matrix cores (mktfhe_amd/csrc/ks_mfma.hip): forced on (MKT_KS_MFMA=1) it gives the words of the digit-pair kernel
(MKT_KS_MFMA=0) and of the oracle's keyswitch!, word for word.  The switch is read once per process, so the cases run in two child processes,
one per setting, each started once for the whole module; the parent compares their outputs with each other and with the oracle.

Shapes: the smallest where the tiling can go wrong -- N = 32 with f = 2 (K = 4 * 64 = 8 steps of the 32-deep MFMA, more than one round of the
six-deep operand ring) and f = 3 (a ragged last step); n = 8 / 9 (one ragged tile of 32 key words) and n = 40 (two tiles, the second ragged);
batches 1, 15, 16, 17, 33 (ragged 32-gate tiles; 33 = two of them); one and two parties, both ring widths; keys of all-ones words under
all-ones digits, of the sign bit alone, of zeros, and random ones.  The key switch at a coefficient is served (same digit words): one case with
repeated and out-of-order rows.  Balanced digits are NOT served: the block set keeps its kernel under the forced switch and the test says so.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mktfhe_amd as mk  # noqa: E402
from helpers import ora_params  # noqa: E402

pytestmark = pytest.mark.gpu

BATCHES = (1, 15, 16, 17, 33)
BASE = {
    "k1_w32": mk.CGGIparam.scaled(n=8, N=32, f=2),
    "k1_w64": mk.CGGIparam.scaled(n=8, N=32, f=2, W=64),
    "k2_w32": mk.CCS2party.scaled(n=8, N=32, f=2),
    "k2_w64": mk.KMS2party.scaled(n=8, N=32, f=2),
}
# name -> (params, key kind, batches, at a coefficient, served by the matrix-core kernel)
CASES = {f"base_{t}": (p, "random", BATCHES, False, True) for t, p in BASE.items()}
CASES.update({
    "ragged_k_k1": (mk.CGGIparam.scaled(n=8, N=32, f=3), "random", (17,), False, True),
    "ragged_k_k2": (mk.KMS2party.scaled(n=8, N=32, f=3), "random", (17,), False, True),
    "ragged_tile_n9": (mk.KMS2party.scaled(n=9, N=32, f=2), "random", (17,), False, True),
    "two_tiles_n40": (mk.CGGIparam.scaled(n=40, N=32, f=2), "random", (33,), False, True),
    "f8_path": (mk.KMS2party.scaled(n=12, N=32), "random", (33,), False, True),
    "key_ones": (BASE["k2_w64"], "ones", (17,), False, True),
    "key_sign": (BASE["k2_w64"], "sign", (17,), False, True),
    "key_zero": (BASE["k2_w32"], "zero", (17,), False, True),
    "at_rows": (BASE["k2_w64"], "random", (33,), True, True),
    "balanced_kept": (mk.KMS2partyblock.scaled(n=9, N=32, f=2, blk_d=3), "random", (17,), False, False),
    "headline_b64": (mk.KMS2party_N1024_l2, "random", (64,), False, True),
})


def case_inputs(name):
    """-> (params, [ksk of every party], {B: (acc, src, coef)}); the same in the parent and in both children"""
    p, kind, batches, at, _ = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 700)
    shape = (p.ksk_rows, p.n + 1)
    nparty = p.k if p.multikey else 1
    fill = {"ones": 0xFFFFFFFF, "sign": 0x80000000, "zero": 0}
    ksk = [rng.integers(0, 2**32, shape, dtype=np.uint64).astype(np.uint32) if kind == "random" else np.full(shape, fill[kind], dtype=np.uint32)
           for _ in range(nparty)]
    ins = {}
    for B in batches:
        acc = rng.integers(0, 2**63, (B, 1 + p.k, p.N), dtype=np.uint64) * 2 + rng.integers(0, 2, (B, 1 + p.k, p.N), dtype=np.uint64)
        if kind == "ones":
            # every extracted word (a_0, -a_{N-1}, ..., -a_1, top 32 bits) has ones in its f digits and a zero below them: every digit D - 1
            w = ((1 << (2 * p.f)) - 1) << (32 - 2 * p.f)
            acc[:, 1:, 0] = w << (p.W - 32)
            acc[:, 1:, 1:] = ((1 << 32) - w) << (p.W - 32)
        acc &= np.uint64((1 << p.W) - 1)
        src = coef = None
        if at:
            src = rng.permutation(B).astype(np.uint32)
            src[-1] = src[0]; src[3] = src[0]                                   # repeated rows, out of order
            coef = rng.integers(0, p.N, B).astype(np.uint32)
            coef[:4] = (0, p.N - 1, 1, p.N - 1)
        ins[B] = (acc.astype(p.ring_dtype), src, coef)
    return p, ksk, ins


def _child(out_path):
    res, outs = {"env": os.environ.get("MKT_KS_MFMA"), "last": {}}, {}
    for name in sorted(CASES):
        p, ksk, ins = case_inputs(name)
        s = mk.Scheme(p)
        for i, kk in enumerate(ksk):
            s.load_party(i, ksk=kk)
        res["seed"], res.setdefault("planes", {})[name] = s.get_metric("ks_mfma"), s.get_metric("ks_mfma_planes")
        for B, (acc, src, coef) in ins.items():
            outs[f"{name}:{B}"] = s.keyswitch(acc) if src is None else mk.keyswitch_at(s, acc, src, coef)
            res["last"][f"{name}:{B}"] = s.get_metric("ks_mfma_last")
        s.close()
    np.savez(out_path, **outs)
    print(json.dumps(res))


_fault = []


@pytest.fixture(scope="module")
def children(require_gpu, tmp_path_factory):
    """{"0" / "1": (the child's report, its outputs)}: one child process per setting of MKT_KS_MFMA, one at a time"""
    got = {}
    for setting in ("0", "1"):
        assert not _fault, f"an earlier child process faulted: {_fault}"
        out = str(tmp_path_factory.mktemp("ksmfma") / f"out{setting}.npz")
        env = {k: v for k, v in os.environ.items() if not k.startswith("MKT_") or k == "MKT_LIB_PATH"}
        env["MKT_KS_MFMA"] = setting
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
        except subprocess.TimeoutExpired:
            _fault.append((setting, "time limit"))
            raise
        if r.returncode < 0 or r.returncode in (134, 139, 124, 137):
            _fault.append((setting, r.returncode))
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert r.returncode == 0 and lines, f"child MKT_KS_MFMA={setting}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
        got[setting] = (json.loads(lines[-1]), dict(np.load(out)))
    return got


def test_the_two_children_ran_the_two_kernels(children):
    off, on = children["0"][0], children["1"][0]
    assert off["seed"] == 0 and on["seed"] == 1
    assert not any(off["planes"].values()) and not any(off["last"].values())           # switched off: no second key form, the older kernels
    for name, (p, _, batches, _, served) in CASES.items():
        assert on["planes"][name] == (1.0 if served else 0.0), name
        for B in batches:
            assert on["last"][f"{name}:{B}"] == (1.0 if served else 0.0), (name, B)


@pytest.mark.parametrize("name", sorted(CASES))
def test_matrix_core_key_switch_equals_the_pair_kernel_and_the_oracle(children, name):
    import oracle.oracle as O
    import ref_lut_many as RM
    p, ksk, ins = case_inputs(name)
    so = O.Scheme(ora_params(p))
    for i, kk in enumerate(ksk):
        so.set_ksk(i, kk)
    rng = np.random.default_rng(3)
    for B, (acc, src, coef) in ins.items():
        a, b = children["0"][1][f"{name}:{B}"], children["1"][1][f"{name}:{B}"]
        assert a.shape == (B, p.lwe_len) and np.array_equal(a, b), (name, B, "matrix cores != digit-pair kernel")
        rows = range(B) if p.N <= 32 else rng.choice(B, 4, replace=False)       # the full-size set: four rows against the oracle
        for g in rows:
            x = acc[g if src is None else src[g]].astype(np.uint64)
            if coef is not None:
                x = RM.extract(x, int(coef[g]), p.W)                            # X^-v * acc: the extraction at coefficient v
            assert np.array_equal(b[g], so.keyswitch(x)), (name, B, int(g), "matrix cores != oracle")


if __name__ == "__main__":
    _child(sys.argv[1])
