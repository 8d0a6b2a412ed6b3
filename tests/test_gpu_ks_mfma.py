"""The key switch on the matrix cores (mktfhe_amd/csrc/ks_mfma.hip): forced on (MKT_KS_MFMA=1) it gives the words of the older kernels
(MKT_KS_MFMA=0: the digit-pair kernel, the per-digit kernel at an odd digit count) and of the oracle's keyswitch!, word for word.  The switch
is read once per process, so the cases run in two child processes, one per setting, each started once for the whole module; the parent
compares their outputs with each other and with the oracle, and holds what each child says it ran (mkt_get_metric "ks_last_kernel", "_g",
"_waves", "_slabs") to helpers.ks_expected.

Shapes: the smallest where the tiling can go wrong -- N = 32 with f = 2 (K = 4 * 64 = 8 steps of the 32-deep MFMA, more than one round of the
six-deep operand ring) and f = 3 (steps that straddle coefficients: 8 digits a step, 3 a coefficient; N f is a multiple of 8 for every
admitted N, so no step is ragged); n = 8 / 9 (one ragged tile of 32 key words) and n = 40 (two tiles, the second ragged); batches 1, 15,
16, 17, 33 (ragged 32-gate tiles; 33 = two of them); one and two parties, both ring widths; keys of all-ones words under all-ones digits,
of the sign bit alone, of zeros, and random ones.  The key switch at a coefficient is served (same digit words).  Balanced digits are NOT
served: the block set keeps its kernel under the forced switch and the test says so.

The launch shape (128 gates a wave, 4 waves a workgroup, gate tiles of 512 on blockIdx.x interleaved with slabs):
  waves_*       batches 127 .. 512: waves 1 - 3 of a workgroup, the exit of a wave past the batch, the clamp of its last 32-gate groups
  gate_tiles    513 and 1025 gates at two slabs: blockIdx.x -> (tile, slab), a last tile of one gate
  k2, k3, k2_*  single-key sets of RLWE length 2 and 3: the component loop, the planes' block stride, the digit words of each component
  full_tile_*   n + 1 = 32 and 64 (no lane past the row: every column tile exactly full), 33 -> a pitch of 36 (one word past a full tile)
  many_slabs    N = 128, f = 8: the largest slab count the rule gives (19 of 7 steps, the last of 2), equal to the CPU plan export's
  bytes_*       key words whose four signed byte planes are -128/-127/-127/-127, all +127, and -128 with a carry of +1 into the next plane,
                under all-ones digits (rows 0 .. 8) and random accumulators (the rest): every product at the planes' extremes
  at_*          the key switch at a coefficient on the 32-bit ring, on a single-key set, and over three waves -- row src[0] named again in
                every wave, coefficients 0, 1, N - 1 at the head of every wave that has three rows (the last wave of 257 has one: 0)
Every row of every case is compared with the oracle (the whole module's oracle time is a few seconds), and with the other child.

Key installs: every path that ends in the planes' packer -- an upload over an earlier key, a party loaded out of order and its neighbour
reloaded, device generation, a seeded load -- on a multi-key and a single-key set (INSTALLS), each followed by a key switch of 17
accumulators held to the oracle loaded with the rows get_ksk returns.
"""
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mktfhe_amd as mk  # noqa: E402
from helpers import KS_MFMA, ks_expected, ks_plan_of, ks_ran, ks_set_ints, ora_params  # noqa: E402

pytestmark = pytest.mark.gpu

# key: random / ones / sign / zero / min / max / carry; acc: random / ones / ones+random; at: at a coefficient; served: by the matrix-core kernel
Case = namedtuple("Case", "p key batches at served acc", defaults=("random",))
BATCHES = (1, 15, 16, 17, 33)
WAVE_BATCHES = (127, 128, 129, 257, 511, 512)
BASE = {
    "k1_w32": mk.CGGIparam.scaled(n=8, N=32, f=2),
    "k1_w64": mk.CGGIparam.scaled(n=8, N=32, f=2, W=64),
    "k2_w32": mk.CCS2party.scaled(n=8, N=32, f=2),
    "k2_w64": mk.KMS2party.scaled(n=8, N=32, f=2),
}
_K2 = mk.CGGIparam.scaled(n=8, N=32, f=2, k=2)
CASES = {f"base_{t}": Case(p, "random", BATCHES, False, True) for t, p in BASE.items()}
CASES.update({
    "ragged_k_k1": Case(mk.CGGIparam.scaled(n=8, N=32, f=3), "random", (17,), False, True),
    "ragged_k_k2": Case(mk.KMS2party.scaled(n=8, N=32, f=3), "random", (17,), False, True),
    "ragged_tile_n9": Case(mk.KMS2party.scaled(n=9, N=32, f=2), "random", (17,), False, True),
    "two_tiles_n40": Case(mk.CGGIparam.scaled(n=40, N=32, f=2), "random", (33,), False, True),
    "f8_path": Case(mk.KMS2party.scaled(n=12, N=32), "random", (33,), False, True),
    "key_ones": Case(BASE["k2_w64"], "ones", (17,), False, True, "ones"),
    "key_sign": Case(BASE["k2_w64"], "sign", (17,), False, True),
    "key_zero": Case(BASE["k2_w32"], "zero", (17,), False, True),
    "at_rows": Case(BASE["k2_w64"], "random", (33,), True, True),
    "balanced_kept": Case(mk.KMS2partyblock.scaled(n=9, N=32, f=2, blk_d=3), "random", (17,), False, False),
    "headline_b64": Case(mk.KMS2party_N1024_l2, "random", (64,), False, True),
    # ---- the launch shape
    "waves_k2_w64": Case(BASE["k2_w64"], "random", WAVE_BATCHES, False, True),
    "waves_k1_w32": Case(BASE["k1_w32"], "random", WAVE_BATCHES, False, True),
    "gate_tiles": Case(mk.KMS2party.scaled(n=8, N=32, f=3), "random", (513, 1025), False, True),
    "k2": Case(_K2, "random", (17, 129), False, True),
    "k3": Case(_K2.scaled(k=3), "random", (17, 129), False, True),
    "k2_w64": Case(_K2.scaled(W=64), "random", (17, 129), False, True),
    "k2_f8": Case(_K2.scaled(f=8), "random", (33,), False, True),
    "full_tile_n31": Case(mk.CGGIparam.scaled(n=31, N=32, f=2), "random", (33,), False, True),
    "full_tile_n32": Case(mk.CGGIparam.scaled(n=32, N=32, f=2), "random", (33,), False, True),
    "full_tile_n63": Case(mk.CGGIparam.scaled(n=63, N=32, f=2), "random", (33,), False, True),
    "full_tile_n31_k2": Case(mk.KMS2party.scaled(n=31, N=32, f=2), "random", (33,), False, True),
    "many_slabs": Case(mk.CGGIparam.scaled(n=8, N=128, f=8), "random", (1, 129), False, True),
    "bytes_min": Case(BASE["k2_w64"], "min", (17,), False, True, "ones+random"),
    "bytes_max": Case(BASE["k2_w64"], "max", (17,), False, True, "ones+random"),
    "bytes_carry": Case(BASE["k2_w64"], "carry", (17,), False, True, "ones+random"),
    "at_w32": Case(BASE["k2_w32"], "random", (33,), True, True),
    "at_k1": Case(_K2, "random", (33,), True, True),
    "at_waves": Case(BASE["k2_w64"], "random", (257,), True, True),
})
WAVE = 128                                      # gates per wave of the matrix-core kernel (ks_mfma.h KSM_WAVE_GATES)
FILL = {"ones": 0xFFFFFFFF, "sign": 0x80000000, "zero": 0, "min": 0x80808080, "max": 0x7F7F7F7F}


def key_words(p, kind, rng):
    """one party's key-switching key, (ksk_rows, n + 1): rows [component][coefficient][d - 1][digit position]"""
    shape = (p.ksk_rows, p.n + 1)
    if kind == "random":
        return rng.integers(0, 2**32, shape, dtype=np.uint64).astype(np.uint32)
    if kind == "carry":                         # row d of every digit: -128 in plane d - 1 and the carry +1 in plane d
        d = (np.arange(p.ksk_rows) // p.f) % 3
        return np.repeat(np.array([0x80, 0x8000, 0x800000], dtype=np.uint32)[d][:, None], p.n + 1, axis=1)
    return np.full(shape, FILL[kind], dtype=np.uint32)


def random_acc(p, rng, B):
    acc = rng.integers(0, 2**63, (B, 1 + p.k, p.N), dtype=np.uint64) * 2 + rng.integers(0, 2, (B, 1 + p.k, p.N), dtype=np.uint64)
    return acc & np.uint64((1 << p.W) - 1)


def case_inputs(name):
    """-> (params, [ksk of every party], {B: (acc, src, coef)}); the same in the parent and in both children"""
    c = CASES[name]
    p = c.p
    rng = np.random.default_rng(sorted(CASES).index(name) + 700)
    ksk = [key_words(p, c.key, rng) for _ in range(p.nparty)]
    ins = {}
    for B in c.batches:
        acc = random_acc(p, rng, B)
        if c.acc != "random":
            # every extracted word (a_0, -a_{N-1}, ..., -a_1, top 32 bits) has ones in its f digits and a zero below them: every digit D - 1
            rows = B if c.acc == "ones" else B // 2 + 1
            w = ((1 << (2 * p.f)) - 1) << (32 - 2 * p.f)
            acc[:rows, 1:, 0] = w << (p.W - 32)
            acc[:rows, 1:, 1:] = ((1 << 32) - w) << (p.W - 32)
        src = coef = None
        if c.at:
            src = rng.permutation(B).astype(np.uint32)
            src[-1] = src[0]; src[3] = src[0]                                   # repeated rows, out of order
            coef = rng.integers(0, p.N, B).astype(np.uint32)
            coef[:4] = (0, p.N - 1, 1, p.N - 1)
            for g0 in range(WAVE, B, WAVE):                                     # every further wave: the same row again, the edge coefficients
                edge = np.array([0, 1, p.N - 1], dtype=np.uint32)[:B - g0]
                coef[g0:g0 + len(edge)] = edge
                src[min(g0 + 3, B - 1)] = src[0]
        ins[B] = (acc.astype(p.ring_dtype), src, coef)
    return p, ksk, ins


# ---- key installs: name -> parameter set; the steps each set goes through are INSTALL_STEPS (the out-of-order load needs two parties)
INSTALLS = {"kms": mk.KMS2party.scaled(n=8, N=32, f=2), "cggi_k2": _K2}
INSTALL_STEPS = ("load_a", "load_b_over_a", "party1_first", "party0_reloaded", "keygen_device", "seeded")
INSTALL_B, INSTALL_SEED = 17, 77


def install_steps(name):
    return [s for s in INSTALL_STEPS if INSTALLS[name].multikey or s not in ("party1_first", "party0_reloaded")]


def install_inputs(name):
    """-> ({letter: [ksk of every party]} for the uploaded keys A .. D, the 17 accumulators every step key-switches)"""
    p = INSTALLS[name]
    rng = np.random.default_rng(sorted(INSTALLS).index(name) + 900)
    return {k: [key_words(p, "random", rng) for _ in range(p.nparty)] for k in "ABCD"}, random_acc(p, rng, INSTALL_B).astype(p.ring_dtype)


def _child_installs(res, outs):
    from helpers import gpu_scheme
    from test_seeded_keys_cpu import seeded_party
    for name, p in INSTALLS.items():
        up, acc = install_inputs(name)

        def note(step, s):
            outs[f"install:{name}:{step}"] = s.keyswitch(acc)
            res["ran"][f"install:{name}:{step}"] = ks_ran(s) + (int(s.get_metric("ks_last_slabs")),)
            for i in range(p.nparty):
                outs[f"install:{name}:{step}:ksk{i}"] = s.get_ksk(i)

        s = mk.Scheme(p)                                                         # an upload, then another over it on the same context
        for letter, step in (("A", "load_a"), ("B", "load_b_over_a")):
            for i in range(p.nparty):
                s.load_party(i, ksk=up[letter][i])
            note(step, s)
        s.close()
        if p.multikey:                                                           # party 1 before party 0, then party 0 again with another key
            s = mk.Scheme(p)
            s.load_party(1, ksk=up["C"][1])
            s.load_party(0, ksk=up["C"][0])
            note("party1_first", s)
            s.load_party(0, ksk=up["D"][0])
            note("party0_reloaded", s)
            s.close()
        crs = mk.CRS(p, INSTALL_SEED) if p.multikey else None
        secrets = [mk.party_keygen(crs, p, party=i, secrets_only=True, deterministic_seed=INSTALL_SEED) for i in range(p.nparty)]
        s = gpu_scheme(p, crs, secrets)                                          # Scheme.keygen_device
        note("keygen_device", s)
        s.close()
        s = gpu_scheme(p, crs, [seeded_party(p, i, seed=INSTALL_SEED)[1] for i in range(p.nparty)])      # mkt_load_seeded_keys, as tests/test_gpu_seeded_keys.py
        note("seeded", s)
        s.close()


def _child(out_path):
    res, outs = {"env": os.environ.get("MKT_KS_MFMA"), "ran": {}}, {}
    for name in sorted(CASES):
        p, ksk, ins = case_inputs(name)
        s = mk.Scheme(p)
        for i, kk in enumerate(ksk):
            s.load_party(i, ksk=kk)
        res["seed"], res.setdefault("planes", {})[name] = s.get_metric("ks_mfma"), s.get_metric("ks_mfma_planes")
        for B, (acc, src, coef) in ins.items():
            outs[f"{name}:{B}"] = s.keyswitch(acc) if src is None else mk.keyswitch_at(s, acc, src, coef)
            res["ran"][f"{name}:{B}"] = ks_ran(s) + (int(s.get_metric("ks_last_slabs")),)
            assert s.get_metric("ks_mfma_last") == (1.0 if ks_ran(s)[0] == KS_MFMA else 0.0)
        s.close()
    _child_installs(res, outs)
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
    assert not any(off["planes"].values())                                              # switched off: no second key form, the older kernels
    for name, c in CASES.items():
        assert on["planes"][name] == (1.0 if c.served else 0.0), name
        assert (ks_expected(c.p, {"MKT_KS_MFMA": "1"})[0] == KS_MFMA) == c.served, name
        for B in c.batches:
            for rep, setting in ((off, "0"), (on, "1")):
                assert tuple(rep["ran"][f"{name}:{B}"][:3]) == ks_expected(c.p, {"MKT_KS_MFMA": setting}), (name, B, setting, rep["ran"][f"{name}:{B}"])


def test_the_largest_slab_count_is_the_plan_exports(children):
    """N = 128, f = 8: 128 steps, the operand ring allows 21 slabs and 19 have steps (7 each, the last 2) -- what the CPU export says"""
    c = CASES["many_slabs"]
    for B in c.batches:
        slabs = children["1"][0]["ran"][f"many_slabs:{B}"][3]
        assert slabs > 6 and slabs == ks_plan_of(ks_set_ints(c.p, 1), B, (32, 0, 0, -1, 1))["slabs"] == 19, (B, slabs)
    for B in CASES["gate_tiles"].batches:
        assert children["1"][0]["ran"][f"gate_tiles:{B}"][3] == 2, B


@pytest.mark.parametrize("name", sorted(CASES))
def test_matrix_core_key_switch_equals_the_pair_kernel_and_the_oracle(children, name):
    import oracle.oracle as O
    import ref_lut_many as RM
    p, ksk, ins = case_inputs(name)
    so = O.Scheme(ora_params(p))
    for i, kk in enumerate(ksk):
        so.set_ksk(i, kk)
    for B, (acc, src, coef) in ins.items():
        a, b = children["0"][1][f"{name}:{B}"], children["1"][1][f"{name}:{B}"]
        assert a.shape == (B, p.lwe_len) and np.array_equal(a, b), (name, B, "matrix cores != the older kernel")
        for g in range(B):                                                      # every row against the oracle
            x = acc[g if src is None else src[g]].astype(np.uint64)
            if coef is not None:
                x = RM.extract(x, int(coef[g]), p.W)                            # X^-v * acc: the extraction at coefficient v
            assert np.array_equal(b[g], so.keyswitch(x)), (name, B, int(g), "matrix cores != oracle")


@pytest.mark.parametrize("name", sorted(INSTALLS))
def test_every_key_install_path_feeds_the_key_switch(children, name):
    import oracle.oracle as O
    p = INSTALLS[name]
    up, acc = install_inputs(name)
    uploaded = {"load_a": up["A"], "load_b_over_a": up["B"], "party1_first": up["C"], "party0_reloaded": [up["D"][0]] + up["C"][1:]}
    seen = []
    for step in install_steps(name):
        key = f"install:{name}:{step}"
        rows = [children["1"][1][f"{key}:ksk{i}"] for i in range(p.nparty)]
        for i in range(p.nparty):
            assert np.array_equal(rows[i], children["0"][1][f"{key}:ksk{i}"]), (key, "the two children hold different keys", i)
            if step in uploaded:
                assert np.array_equal(rows[i].ravel(), uploaded[step][i].ravel()), (key, "get_ksk is not the key uploaded last", i)
        assert rows[0].any() and not any(np.array_equal(rows[0], r) for r in seen), (key, "a key of its own")
        seen.append(rows[0])
        so = O.Scheme(ora_params(p))
        for i in range(p.nparty):
            so.set_ksk(i, rows[i].reshape(p.ksk_rows, p.n + 1))
        want = np.stack([so.keyswitch(acc[g].astype(np.uint64)) for g in range(INSTALL_B)])
        for setting in ("1", "0"):
            assert np.array_equal(children[setting][1][key], want), (key, "MKT_KS_MFMA", setting, "!= the oracle under the rows get_ksk returns")
            assert tuple(children[setting][0]["ran"][key][:3]) == ks_expected(p, {"MKT_KS_MFMA": setting}), (key, setting, children[setting][0]["ran"][key])
        assert children["1"][0]["ran"][key][0] == KS_MFMA, key


if __name__ == "__main__":
    _child(sys.argv[1])
