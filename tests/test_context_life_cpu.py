"""The case lists of tests/test_gpu_context_life.py stay complete (no GPU): every batch entry point of include/mktfhe.h is a step of the
sequence, every option that drops the workspace is walked under a live one, and the tables T' of the either-order test are what that test
says they are."""
import os
import re

import numpy as np

import context_life_cases as K
from helpers import ROOT, mk


def _batch_entry_points():
    """every function of mktfhe.h, mkt_multi_ and mkt_client_ apart, whose parameters include `mkt_ctx *` and `int mem`"""
    text = open(os.path.join(ROOT, "include", "mktfhe.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    found = set()
    for name, params in re.findall(r"\bint\s+(mkt_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        if name.startswith(("mkt_multi_", "mkt_client_")):
            continue
        params = " ".join(params.split())
        if re.search(r"\bmkt_ctx \*", params) and re.search(r"\bint mem\b", params):
            found.add(name)
    return found


def _workspace_resetting_options():
    """the options with resets_workspace true in context.cpp's SWITCHES table (the last field of a row), read from the source text"""
    text = open(os.path.join(ROOT, "mktfhe_amd", "csrc", "context.cpp")).read()
    assert re.search(r"struct Switch \{[^}]*bool resets_workspace; \};", text), "the row layout this parse relies on"
    body = text[text.index("const Switch SWITCHES[] = {"):]
    body = body[:body.index("\n};\n")]
    rows = re.findall(r'^\s*\{"([a-z0-9_]+)", (?:"MKT_[A-Z0-9_]+"|nullptr), &Tune::\1, -?\d+, \{[^}]*\}, (true|false)\},', body, re.M)
    return {n for n, _ in rows}, {n for n, r in rows if r == "true"}


def test_every_batch_entry_point_is_a_step():
    entries = _batch_entry_points()
    assert {"mkt_gate_batch", "mkt_keyswitch_at_batch", "mkt_lut_batch_gather_at", "mkt_seeded_keys_expand", "mkt_partial_decrypt_batch"} <= entries \
        and len(entries) >= 31, sorted(entries)
    named = [st.entry for st in K.STEPS]
    assert len(named) == len(set(named)) and len({st.name for st in K.STEPS}) == len(K.STEPS), "one step per entry point"
    assert entries == set(named), ("without a step:", sorted(entries - set(named)), "not in the header:", sorted(set(named) - entries))
    for st in K.STEPS:
        assert any(st.applies(*K.SETS[name]) for name in K.SETS), (st.name, "applies to no set")
    # the selective steps are selective in the way the header says
    assert [n for n in K.SETS if K.STEP["kms_phase1"].applies(*K.SETS[n])] == ["kms", "x-kms"]
    assert [n for n in K.SETS if K.STEP["exact_polymul"].applies(*K.SETS[n])] == ["x-kr", "x-kms", "x-ccs"]
    assert all(K.STEP[s].applies(*K.SETS[n]) for s in ("transform_fwd", "transform_inv", "decompose") for n in K.SETS)


def test_the_sequence_is_what_the_test_says():
    for name in K.SETS:
        seq, steps = K.sequence(name), K.steps_of(name)
        assert [st for st, _, _ in seq[:len(steps)]] == steps, "first round: the table's order"
        for r, seed in ((1, 1), (2, 2)):
            assert [st for st, _, _ in seq[r * len(steps):(r + 1) * len(steps)]] == [steps[j] for j in np.random.default_rng(seed).permutation(len(steps))]
        assert [B for _, B, _ in seq[:6]] == [5, 1, 70, 33, 0, 5] and {m for _, _, m in seq[0::2]} == {mk.MEM_HOST} and {m for _, _, m in seq[1::2]} == {mk.MEM_DEVICE}
        assert all(m == mk.MEM_HOST for _, B, m in seq if B == 0), "an empty tensor has no address: the empty call is a host call"


def test_every_workspace_resetting_option_is_walked():
    every, resetting = _workspace_resetting_options()
    assert "exact_kany" in resetting and {"rot_wide", "ccs_pipe", "exact_impl"} <= every - resetting, (sorted(every), sorted(resetting))
    walked = {w.option for w in K.OPTION_WALKS}
    assert resetting <= walked, f"options that drop the workspace without a walk under a live one: {sorted(resetting - walked)}"
    for w in K.OPTION_WALKS:
        assert w.option in every and all(k in every for k in w.before) and len(w.values) == len(w.kernels) >= 3 and w.values[0] != w.values[1]
        assert w.set in K.SETS or w.set in K.EXTRA_SETS


def test_tprime_is_admitted_and_differs_from_entry_4_on():
    """T' passes the two checks mkt_set_twiddles makes (context.cpp), restated: Psiinv[i] = conj(Psi[i]) for i >= 1 -- the real parts the same
    bits, the imaginary parts negated -- and Psi[1] = (eps, -1), Psi[2] = (c, -c), Psi[3] = (-c, -c) with c > 0; and it differs from
    mkt_make_twiddles in every entry of Psi and Psiinv from 4 on, in both parts, by one ulp, and nowhere else"""
    for name in ("kms", "cggi"):
        N = K.set_of(name)[0].N
        own, (psi, psiinv, roots, rootsinv) = K.make_twiddles(N), K.tprime(N)
        for t in (own[0], psi):
            assert np.array_equal(t.real[1:].view(np.uint64), (psiinv if t is psi else own[1]).real[1:].view(np.uint64))
            assert np.array_equal((psiinv if t is psi else own[1]).imag[1:], -t.imag[1:])
            c = t[2].real
            assert t[1].imag == -1.0 and t[2].imag == -c and c > 0.0 and t[3].real == t[3].imag == -c
        assert np.array_equal(psi[:4], own[0][:4]) and np.array_equal(psiinv[:4], own[1][:4]) and np.array_equal(roots, own[2]) and np.array_equal(rootsinv, own[3])
        for part in ("real", "imag"):
            a, b = getattr(psi, part)[4:], getattr(own[0], part)[4:]
            assert (a != b).all() and (np.isfinite(a)).all()
            assert ((np.nextafter(b, np.inf) == a) | (np.nextafter(b, -np.inf) == a)).all(), "one ulp"
            assert (getattr(psiinv, part)[4:] != getattr(own[1], part)[4:]).all()
        assert set(np.sign(psi.real[4:] - own[0].real[4:])) == {-1.0, 1.0}, "both directions"
        assert np.array_equal(K.tprime(N)[0], psi), "seeded"


def test_check_ready_restated_matches_the_source():
    """expected_refusal words its refusals as check_ready does, in check_ready's order"""
    text = open(os.path.join(ROOT, "mktfhe_amd", "csrc", "context.cpp")).read()
    body = text[text.index("int check_ready(mkt_ctx *c, bool need_brk, bool need_ksk) {"):]
    body = body[:body.index("\n}\n")]
    assert re.findall(r'MKT_ERR_STATE, "([^"]+)"', body) == ["bootstrapping key not loaded", "key-switching key not loaded", "public key not loaded",
                                                              "rlk / public key not loaded", "crs not loaded"]
    p = K.SETS["kms"][0]
    everything = {(k, i) for k in ("brk", "ksk", "rlk", "pubkey") for i in range(p.nparty)} | {"crs"}
    assert K.expected_refusal(p, everything, True, True) is None and K.expected_refusal(p, set(), False, False) is None
    assert K.expected_refusal(p, everything - {("rlk", 1)}, True, False) == "rlk / public key not loaded"
    assert K.expected_refusal(p, everything - {("rlk", 1)}, False, True) is None
    assert K.expected_refusal(p, everything - {"crs"}, True, True) == "crs not loaded"
    assert K.expected_refusal(K.SETS["ccs"][0], everything - {("pubkey", 0), ("rlk", 0), ("rlk", 1)}, True, True) == "public key not loaded"
    assert K.pieces_of(K.SETS["cggi"][0]) == ["ksk", "brk"] and K.pieces_of(K.SETS["ccs"][0]) == ["ksk", "crs", "pubkey", "brk"] and K.pieces_of(p) == list(K.PIECES)
