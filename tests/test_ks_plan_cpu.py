"""The launch rule of the key switch (mktfhe_amd/csrc/kernels.hip ks_plan) without a GPU, through mkt_internal_ks_plan: the set as ten plain
ints, the batch and the five switch values in, the plan out.

1. Which kernel: every set and setting the GPU switch children run (tests/test_gpu_switches.py, test_gpu_footprint.py,
   test_gpu_keyswitch_at.py, test_gpu_ks_mfma.py), with and without scratch and byte planes, against helpers.ks_kernel_rule -- the rule
   restated in Python, which the same children hold their `ks_last_kernel` reports to.
2. The slab rule of the matrix-core kernel over a grid of shapes: the kernel cuts per = ceil(steps / slabs) steps per slab, so a slab count
   that is not renormalised after `per` is known launches workgroups with nothing to sum (N = 128, f = 8, n1p = 12, one party, B = 1:
   128 steps, 21 slabs, per = 7, slabs 19 and 20 begin past the end).  No slab may be empty, none shorter than the operand ring.
3. The plans of the shipped sets, recorded from the rule before the renormalisation: the merged timings rest on them, they must not move.
"""
import itertools

import pytest

import edge_cases as EC
from helpers import KS_MFMA, KS_PAIR, KS_PER_DIGIT, KS_PLAN_FIELDS as FIELDS, ks_kernel_rule, ks_plan_of as plan, ks_set_ints, ks_switch_values, mk

KSM_RING, KSM_STEP_DIGITS, KSM_GATES = 6, 8, 512          # ks_mfma.h: operand ring, digits per step, gates per workgroup


# ---- 1 ----
def child_settings():
    import test_gpu_footprint as TF
    import test_gpu_keyswitch_at as TA
    import test_gpu_switches as TS
    seen = [{}]
    for e in TS.KS_SETTINGS + TF.KS_SETTINGS + TA.KS_SETTINGS + [{"MKT_KS_MFMA": "0"}, {"MKT_KS_MFMA": "1"}]:
        if e not in seen:
            seen.append(e)
    return seen


def child_sets():
    import context_life_cases as K
    import test_gpu_footprint as TF
    import test_gpu_keyswitch_at as TA
    import test_gpu_ks_mfma as TM
    import test_gpu_switches as TS
    sets = [EC.KS_CHILD_FULL[0]] + list(EC.KS_CHILD_SETS) + [p for p, _ in TS.KS_PLAIN_SETS] + [K.set_of(n)[0] for n in TF.KS_CHILD_SETS] + list(TA.CHILD_SETS)
    sets += [c[0] for c in TM.CASES.values()] + list(EC.KS_SETS)
    sets += [mk.CGGIparam.scaled(f=3), mk.CGGIparam.scaled(f=4, logD=3), mk.KMS2party, mk.KMS2party_N1024_l2, mk.CCS2party, mk.CCS8party_N2048]
    out = []
    for p in sets:
        if p not in out:
            out.append(p)
    return out


def test_the_sweep_holds_every_child_setting_and_set():
    import test_gpu_footprint as TF
    import test_gpu_keyswitch_at as TA
    import test_gpu_switches as TS
    settings, sets = child_settings(), child_sets()
    for lst in (TS.KS_SETTINGS, TF.KS_SETTINGS, TA.KS_SETTINGS):
        assert all(e in settings for e in lst) and all("MKT_KS_MFMA" in e for e in lst), "every child names the matrix-core switch"
    assert all(p in sets for p in EC.KS_CHILD_SETS)
    rule = {ks_kernel_rule(ks_set_ints(p, ks_switch_values(e)[4]), ks_switch_values(e)) for p in sets for e in settings}
    assert {k for k, _, _ in rule} == {KS_PER_DIGIT, KS_PAIR, KS_MFMA}
    assert {(k, g) for k, g, _ in rule} >= {(KS_PER_DIGIT, 8), (KS_PER_DIGIT, 16), (KS_PER_DIGIT, 32), (KS_PAIR, 32), (KS_MFMA, 32)}
    assert {(k, w) for k, _, w in rule} >= {(KS_PER_DIGIT, 1), (KS_PER_DIGIT, 2), (KS_PER_DIGIT, 4), (KS_PAIR, 1), (KS_PAIR, 2), (KS_PAIR, 4), (KS_MFMA, 4)}


def test_every_switch_child_setting_reaches_what_it_is_written_for():
    """an entry of KS_SETTINGS that names an older kernel's switch without MKT_KS_MFMA = 0 implies the matrix cores: it fails here, before any GPU run"""
    import context_life_cases as K
    import test_gpu_footprint as TF
    import test_gpu_switches as TS
    assert len(TS.KS_MEANT) == len(TS.KS_SETTINGS) and TF.KS_SETTINGS == TS.KS_SETTINGS
    for e, meant in zip(TS.KS_SETTINGS, TS.KS_MEANT):
        for p in (mk.CGGIparam, K.set_of("cggi")[0], K.set_of("kms")[0]):
            assert ks_kernel_rule(ks_set_ints(p, ks_switch_values(e)[4]), ks_switch_values(e)) == meant, (e, p.name, meant)
            assert tuple(plan(ks_set_ints(p, ks_switch_values(e)[4]), 33, ks_switch_values(e))[k] for k in ("kernel", "G", "waves")) == meant, (e, p.name, meant)
    assert {m[0] for m in TS.KS_MEANT[:11]} == {KS_PER_DIGIT, KS_PAIR} and {m[0] for m in TS.KS_MEANT[11:]} == {KS_MFMA}
    reverted = {k: v for k, v in TS.KS_SETTINGS[0].items() if k != "MKT_KS_MFMA"}
    assert ks_kernel_rule(ks_set_ints(mk.CGGIparam), ks_switch_values(reverted))[0] == KS_MFMA != TS.KS_MEANT[0][0]


def test_kernel_choice_follows_the_restated_rule():
    n = 0
    for p, e in itertools.product(child_sets(), child_settings()):
        sw = ks_switch_values(e)
        base = ks_set_ints(p, sw[4])
        for planes, scratch, B in itertools.product({base[8], 0}, (1, 0), (1, 33, 1000)):      # planes 0: the optional allocation failed
            ints = base[:8] + [planes, scratch]
            q = plan(ints, B, sw)
            assert (q["kernel"], q["G"], q["waves"]) == ks_kernel_rule(ints, sw), (p, e, planes, scratch, B, q)
            n += 1
    assert n > 1000


def test_the_rule_in_words():
    """the issue's three sentences on one set each, so that a helper that drifted with the library still fails here"""
    cggi, block = ks_set_ints(mk.CGGIparam), ks_set_ints(mk.Blockparam)
    assert cggi[:4] == [1024, 8, 2, 3] and cggi[6:] == [0, 0, 1, 1] and block[3] == 2 and block[7:9] == [1, 0]
    k = lambda ints, **s: plan(ints, 33, ks_switch_values({f"MKT_KS_{a}": str(v) for a, v in s.items()}))      # noqa: E731
    assert k(cggi)["kernel"] == 3 and k(cggi, MFMA=1)["kernel"] == 3 and k(cggi, MFMA=-1)["kernel"] == 3
    assert k(cggi, MFMA=1, G=8, PAIR=0) == k(cggi, MFMA=1), "the matrix cores are asked first"
    assert k(cggi, MFMA=0)["kernel"] == 2 and k(cggi[:8] + [0, 1])["kernel"] == 2 and k(cggi[:9] + [0])["kernel"] == 1
    assert k(cggi, MFMA=0, PAIR=0)["kernel"] == 1 and k(cggi, MFMA=0, G=16)["kernel"] == 1 and k(cggi, MFMA=0, G=16)["G"] == 16
    assert k(cggi, MFMA=0, G=12)["kernel"] == 2 and k(cggi, MFMA=0, G=12)["G"] == 32
    assert k(block, MFMA=1)["kernel"] == 2 and k(block, MFMA=1, PAIR=0)["waves"] == 1 and k(block, PAIR=0, WAVES=2)["waves"] == 2
    odd = ks_set_ints(mk.CGGIparam.scaled(f=3))
    assert k(odd)["kernel"] == 3 and k(odd, MFMA=0)["kernel"] == 1
    d8 = ks_set_ints(mk.CGGIparam.scaled(f=4, logD=3))
    assert d8[8] == 0 and k(d8, MFMA=1)["kernel"] == 1 and k(d8[:8] + [1, 1], MFMA=1)["kernel"] == 1


# ---- 2 ----
SLAB_GRID = list(itertools.product((32, 64, 128, 256, 512, 1024, 2048, 4096), (2, 3, 5, 8, 16), (12, 32, 36, 564, 632), (1, 2, 4, 8),
                                   (1, 128, 129, 512, 513, 1024, 4096, 65536)))


def test_matrix_core_slabs_are_never_empty():
    empty = []
    for N, f, n1p, parties, B in SLAB_GRID:
        for mkey, kacc in (((0, 1), (0, 2), (0, 3), (1, 1)) if parties == 1 else ((1, parties),)):      # a single-key set runs its components in one workgroup
            ints = [N, f, 2, 3, n1p, kacc, mkey, 0, 1, 1]
            q = plan(ints, B)
            what = (N, f, n1p, parties, mkey, kacc, B, q)
            steps = (N * f + KSM_STEP_DIGITS - 1) // KSM_STEP_DIGITS
            assert q["kernel"] == KS_MFMA and q["parties"] == parties and q["ngroups"] == (B + 31) // 32 and q["gblocks"] == (B + KSM_GATES - 1) // KSM_GATES, what
            assert 1 <= q["slabs"] <= max(1, steps // KSM_RING), what
            per = (steps + q["slabs"] - 1) // q["slabs"]
            if (q["slabs"] - 1) * per >= steps:
                empty.append(what)
            assert per >= KSM_RING or steps < KSM_RING, what
            assert q["partial_words"] == q["slabs"] * parties * B * n1p and q["digit_words"] == ints[5] * q["ngroups"] * N * 32, what
            # without scratch the call falls to the per-digit kernel, and the sizes asked for are still those of the plan with scratch
            bare = plan(ints[:9] + [0], B)
            assert bare["kernel"] == KS_PER_DIGIT and (bare["digit_words"], bare["partial_words"]) == (q["digit_words"], q["partial_words"]), what
    assert not empty, (len(empty), "plans with slabs that begin past the last step", empty[:5])


def test_the_named_example_of_empty_slabs():
    q = plan([128, 8, 2, 3, 12, 1, 0, 0, 1, 1], 1)
    assert q["slabs"] == 19, q                                                # 128 steps: 21 asked for, per = 7, ceil(128 / 7) = 19 have steps


# ---- 3 ----
# (kernel, G, waves, ngroups, parties, gblocks, slabs, digit words, partial words) under the defaults, recorded before the slab count was renormalised
SHIPPED = {
    ("CGGIparam", 1): (3, 32, 4, 1, 1, 1, 25, 32768, 15800),
    ("CGGIparam", 64): (3, 32, 4, 2, 1, 1, 25, 65536, 1011200),
    ("CGGIparam", 512): (3, 32, 4, 16, 1, 1, 25, 524288, 8089600),
    ("CGGIparam", 1024): (3, 32, 4, 32, 1, 2, 12, 1048576, 7766016),
    ("CGGIparam", 4096): (3, 32, 4, 128, 1, 8, 3, 4194304, 7766016),
    ("KMS2party", 1): (3, 32, 4, 1, 2, 1, 14, 131072, 15792),
    ("KMS2party", 64): (3, 32, 4, 2, 2, 1, 14, 262144, 1010688),
    ("KMS2party", 512): (3, 32, 4, 16, 2, 1, 14, 2097152, 8085504),
    ("KMS2party", 1024): (3, 32, 4, 32, 2, 2, 7, 4194304, 8085504),
    ("KMS2party", 4096): (3, 32, 4, 128, 2, 8, 4, 16777216, 18481152),
    ("KMS2party_N1024_l2", 1): (3, 32, 4, 1, 2, 1, 14, 65536, 15792),
    ("KMS2party_N1024_l2", 64): (3, 32, 4, 2, 2, 1, 14, 131072, 1010688),
    ("KMS2party_N1024_l2", 512): (3, 32, 4, 16, 2, 1, 14, 1048576, 8085504),
    ("KMS2party_N1024_l2", 1024): (3, 32, 4, 32, 2, 2, 7, 2097152, 8085504),
    ("KMS2party_N1024_l2", 4096): (3, 32, 4, 128, 2, 8, 4, 8388608, 18481152),
    ("CCS2party", 1): (3, 32, 4, 1, 2, 1, 14, 65536, 15792),
    ("CCS2party", 64): (3, 32, 4, 2, 2, 1, 14, 131072, 1010688),
    ("CCS2party", 512): (3, 32, 4, 16, 2, 1, 14, 1048576, 8085504),
    ("CCS2party", 1024): (3, 32, 4, 32, 2, 2, 7, 2097152, 8085504),
    ("CCS2party", 4096): (3, 32, 4, 128, 2, 8, 4, 8388608, 18481152),
    ("CCS8party_N2048", 1): (3, 32, 4, 1, 8, 1, 5, 524288, 22560),
    ("CCS8party_N2048", 64): (3, 32, 4, 2, 8, 1, 5, 1048576, 1443840),
    ("CCS8party_N2048", 512): (3, 32, 4, 16, 8, 1, 5, 8388608, 11550720),
    ("CCS8party_N2048", 1024): (3, 32, 4, 32, 8, 2, 4, 16777216, 18481152),
    ("CCS8party_N2048", 4096): (3, 32, 4, 128, 8, 8, 1, 67108864, 18481152),
}


@pytest.mark.parametrize("name", sorted({n for n, _ in SHIPPED}))
def test_shipped_plans_stay_put(name):
    for B in (1, 64, 512, 1024, 4096):
        q = plan(ks_set_ints(getattr(mk, name)), B)
        assert tuple(q[k] for k in FIELDS) == SHIPPED[name, B], (name, B, q)
