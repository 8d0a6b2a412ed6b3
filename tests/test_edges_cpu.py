"""The inputs of tests/test_gpu_edges.py, checked with the oracle alone (no GPU): every boundary class is present in what the
builders of helpers.py produce for every parameter set of tests/edge_cases.py (a count per class > 0: the condition that keeps
the GPU tests from silently testing nothing), the oracle's own composition identity holds on the crafted rows, and each class
separates the oracle from the plausible wrong variant written next to it."""
import os
import re

import numpy as np
import pytest

import edge_cases as EC
import ref_lut as R
import ref_lut_many as RM
from helpers import (BT_TARGETS, KS_LOW_HALVES, O, acc_edge, bt_values, btilde_words, extract_words, gadget_words, gate_input, keygen, ks_border,
                     ks_borrow_decides, ks_edge_acc, ks_edge_acc_at, ks_words, lut_edge_tables, lwe_edge_rows, mk, modswitch_words, oracle_scheme,
                     rot_gadgets)


def _switch(w, N):
    return O.divbits(int(w), 32 - (N.bit_length() - 1) - 1, 32)


def _sw_row(row, N, nout=1):
    return np.array([RM.sw(w, N, nout) for w in row], dtype=np.int64)


# ---------------------------------------------------------------- 1. class counts
@pytest.mark.parametrize("even", [False, True], ids=["any", "even"])
@pytest.mark.parametrize("p", EC.all_rotation_sets(), ids=EC.sid)
def test_lwe_edge_rows_hold_every_class(p, even):
    _rows_hold_every_class(p, even, 1)


@pytest.mark.parametrize("nout", EC.LUT_NOUTS)
@pytest.mark.parametrize("p", list(dict.fromkeys(c[0] for c in EC.LUT_BOOT_CASES)), ids=EC.sid)
def test_lwe_edge_rows_hold_every_class_on_the_coarse_grid(p, nout):
    """the rows of the many-table / coefficient-list bootstraps: every kind meets every target 0, nout, N - nout, N, N + nout, 2N - nout, 2N
    of sw_nu (tests/ref_lut_many.py), ties and words that round to 0 included"""
    assert RM.sw(1 << 31, p.N, nout) == p.N and {RM.sw(w, p.N, nout) for w in RM.sw_edge_words(p.N, nout)} >= {0, nout, p.N, 2 * p.N - nout, 2 * p.N}
    _rows_hold_every_class(p, False, nout)


def _rows_hold_every_class(p, even, nout):
    N, n, nm = p.N, p.n, p.lwe_len - 1
    rows, kinds = lwe_edge_rows(p, np.random.default_rng(1), even=even, nout=nout)
    if even:
        assert not (rows & 1).any()
    want = bt_values(N, nout)
    assert nout > 1 or want == {"0": 0, "1": 1, "N-1": N - 1, "N": N, "N+1": N + 1, "2N-1": 2 * N - 1, "2N": 2 * N}
    sw = np.stack([_sw_row(r, N, nout) for r in rows])
    if nout == 1:
        assert all(int(v) == _switch(w, N) for v, w in zip(sw[0], rows[0]))
    for kind in ("zero", "skip", "dense", "blocks") + (("party",) if p.multikey else ()):
        sel = [i for i, k in enumerate(kinds) if k == kind]
        assert {int(sw[i, nm]) for i in sel} >= set(want.values()), (kind, "btilde")                    # every btilde in every kind
        for i in sel:
            raw, s = rows[i, :nm], sw[i, :nm]
            if kind == "zero":
                assert not raw.any()
            if kind == "skip":
                assert raw.all() and not s.any()                                                       # raw words non-zero, every step skipped
            if kind == "dense":
                assert s[0] and s[nm - 1]
                for q in range(1, p.nparty):
                    assert s[q * n - 1] and s[q * n], "party border"
            if kind == "party":
                dead = [q for q in range(p.nparty) if not s[q * n:(q + 1) * n].any()]
                assert dead and all(rows[i, q * n:(q + 1) * n].all() for q in dead) and s.any()
        if kind == "blocks":
            L = p.blk_len if p.blk_len > 1 else 1
            hit = 0
            for i in sel:
                b = sw[i, :nm // L * L].reshape(-1, L)
                dead, full = ~b.any(axis=1), b.all(axis=1)
                assert (dead | full).all() and rows[i, :nm].all()
                hit += int((dead[:-1] & full[1:]).sum() + (full[:-1] & dead[1:]).sum())
            assert hit > 0, "a block that rounds to 0 next to a full block"
    mask_sw = sw[:, :nm]
    counts = {k: int((mask_sw == v).sum()) for k, v in want.items()}
    counts["raw != 0 -> 0"] = int(((mask_sw == 0) & (rows[:, :nm] != 0)).sum())
    h = (1 << (32 - (N.bit_length() - 1) - 2)) * nout
    counts["tie"] = int(((rows[:, :nm] & np.uint32(2 * h - 1)) == h).sum())
    assert all(c > 0 for c in counts.values()), counts


def _digit_classes(words, l, logB, W):
    """class -> boolean array over words, by the oracle's digits (O.decomp_poly) and the words' own low bits"""
    w = np.asarray(words, dtype=np.uint64).ravel()
    d = O.decomp_poly(w, l, logB, W).astype(np.int64) if W == 64 else O.decomp_poly(w, l, logB, W).astype(np.uint32).astype(np.int32).astype(np.int64)
    half, bit = 1 << (logB - 1), W - l * logB
    cls = {"all-min": (d == -half).all(axis=0), "all-max": (d == half - 1).all(axis=0), "top-min": w == np.uint64(1 << (W - 1))}
    if bit >= 1:
        hb = 1 << (bit - 1)
        low = w & np.uint64((1 << bit) - 1)
        cls["tie"] = low == np.uint64(hb)
        cls["tie-1"] = low == np.uint64(hb - 1)
        cls["round-carry"] = (w >= np.uint64((1 << W) - hb)) & (d == 0).all(axis=0)
        cls["tie->all-min"] = cls["tie"] & cls["all-min"]
        if bit >= 2:
            cls["tie+1"] = low == np.uint64(hb + 1)
    return cls


@pytest.mark.parametrize("p", EC.all_rotation_sets(), ids=EC.sid)
def test_acc_edge_holds_every_class_for_every_gadget(p):
    N, M, W = p.N, p.N // 2, p.W
    acc = acc_edge(p, rot_gadgets(p), np.random.default_rng(2), 3)
    assert acc.shape == (3, 1 + p.k, N) and (acc.reshape(-1, N) != 0).any(axis=1).all(), "every polynomial populated"
    for (l, logB) in rot_gadgets(p):
        cls = _digit_classes(acc, l, logB, W)
        counts = {k: int(v.sum()) for k, v in cls.items()}
        assert all(c > 0 for c in counts.values()), ((l, logB), counts)
        special = np.zeros(acc.size, dtype=bool)
        for v in cls.values():
            special |= v
        special = special.reshape(-1, N)
        assert all(special[:, i].any() for i in (0, M - 1, M, N - 1)), "a boundary word at each of 0, M - 1, M, N - 1"
        for k, v in cls.items():
            v = v.reshape(-1, N)
            assert v[:, :M].any() and v[:, M:].any(), (k, "both halves")
        if W == 64 and W - l * logB > 32:            # the gadget reads the high half only: the same digits over a low half of all ones / the top bit alone
            low = (acc & np.uint64(0xFFFFFFFF)).ravel()
            for k in ("all-min", "all-max"):
                assert (cls[k] & (low == 0xFFFFFFFF)).any() and (cls[k] & (low == 0x80000000)).any(), (k, "low half")
    if W == 64:
        low = acc & np.uint64(0xFFFFFFFF)
        assert (low == 0xFFFFFFFF).any() and (low == 0x80000000).any()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("p", EC.KS_SETS + EC.KS_CHILD_SETS, ids=EC.sid)
def test_ks_edge_acc_holds_every_class(p, B):
    _ks_acc_holds_every_class(p, ks_edge_acc(p, np.random.default_rng(3), B), B)


def _ks_acc_holds_every_class(p, acc, B):
    N, f, logD = p.N, p.f, p.logD
    Lb, bit, D = f * logD, 32 - f * logD, 1 << logD
    balanced = p.scheme in (mk.LMSS, mk.KMS_BLOCK)
    special_words = set(ks_words(f, logD).values())
    counts = {}
    for b in range(B):
        for c in range(p.k):
            w = extract_words(p, acc[b, 1 + c])
            j0 = ks_border(p, c)
            src = acc[b, 1 + c]
            for name, j in (("0", 0), ("1", 1), ("N-1", N - 1), ("border-1", j0 - 1), ("border", j0)):
                if name.startswith("border") and not 0 < j0 < N:
                    continue                                                  # this component has no copied / switched border
                here = int(w[j]) in special_words
                if p.W == 64:                                                 # ... over one of the crafted low halves (cut off, never rounded in)
                    here = here and int(src[0 if j == 0 else N - j]) & 0xFFFFFFFF in KS_LOW_HALVES
                counts["a boundary word at j = " + name] = counts.get("a boundary word at j = " + name, 0) + here
            sw = w[j0:]                                                       # the switched words
            if not len(sw):
                continue
            jj = np.arange(j0, N)
            add = lambda k, m: counts.__setitem__(k, counts.get(k, 0) + int(np.sum(m)))      # noqa: E731
            add("zero", sw == 0)
            add("0x80000000 at a negated position", (sw == 0x80000000) & (jj > 0))
            if balanced:
                for k, m in _digit_classes(sw, f, logD, 32).items():
                    add("b-" + k, m)
            else:
                dg = np.stack([O.unbalanced_decomp_word(int(x), f, logD, 32) for x in np.unique(sw)])
                rounded = np.array([O.divbits(int(x), bit, 32) for x in np.unique(sw)])
                add("carry leaves the field (digits 0, word not 0)", (rounded == 1 << Lb) & ~dg.any(axis=1))
                add("all digits D-1", (dg == D - 1).all(axis=1))
                if bit >= 1:
                    low = np.unique(sw) & np.uint32((1 << bit) - 1)
                    add("tie", low == 1 << (bit - 1))
                    add("tie-1", low == (1 << (bit - 1)) - 1)
    assert all(v > 0 for v in counts.values()), counts
    assert {"a boundary word at j = 0", "a boundary word at j = 1", "a boundary word at j = N-1"} <= set(counts)
    if any(0 < ks_border(p, c) < N for c in range(p.k)):
        assert {"a boundary word at j = border-1", "a boundary word at j = border"} <= set(counts)
    if balanced:
        assert any(ks_border(p, c) > 0 for c in range(p.k))
    if p.W == 64:
        low = acc[:, 1:] & np.uint64(0xFFFFFFFF)
        assert (low == 0xFFFFFFFF).any() and (low == 0x80000000).any()
        cut = N - np.arange(N - 1, 0, -1)[None, None, :] >= np.array([ks_border(p, c) for c in range(p.k)])[None, :, None]      # a[N - j], j switched
        for h in (0, 1):                                                      # a wrapped word with and without a borrow from the high half
            assert ((low[:, :, 1:] == h) & cut).any(), ("low half", h)


def _at_sets():
    return list(dict.fromkeys(EC.KS_AT_SETS + EC.KS_CHILD_SETS))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("p", _at_sets(), ids=EC.sid)
def test_ks_edge_acc_at_holds_every_class_at_every_coefficient(p, B):
    """X^v * ks_edge_acc: the extraction at v is an accumulator that the assertion above accepts -- every class at every position class --
    and, 64-bit ring, on each side of j = v that exists every ciphertext holds a word over a non-zero low half where moving the negation
    across the truncation changes an output word (ks_borrow_decides)"""
    N = p.N
    for v in EC.KS_AT_COEFS(p):
        acc = ks_edge_acc_at(p, np.random.default_rng(3), B, v)
        assert acc.dtype == np.uint64 and acc.shape == (B, 1 + p.k, N) and not (acc >> np.uint64(p.W - 1) >> np.uint64(1)).any()
        base = RM.extract(acc, v, p.W)
        for b in range(B):                                                    # the rotation itself, restated: out[i] = a[i - v], -a[N + i - v]
            for c in range(1 + p.k):
                assert np.array_equal(acc[b, c], R.rotate(base[b, c], v, p.W)), (v, b, c)
        _ks_acc_holds_every_class(p, base, B)
        if p.W == 64 and p.f * p.logD < 32:
            for b in range(B):
                for name, side in (("wrapped", range(1, v + 1)), ("not wrapped", range(v + 1, N))):
                    if len(side):
                        assert any(ks_borrow_decides(p, c, j, base[b, 1 + c, N - j]) for c in range(p.k) for j in side), (v, b, name)
    assert set(EC.KS_AT_FULL_COEFS(p)) <= set(EC.KS_AT_COEFS(p))


def _mutant_base(acc, v):
    """the v = 0 accumulators whose key switch is what a kernel gives that takes -trunc(x) for trunc(-x) at the wrapped positions
    1 <= j <= v of a 64-bit accumulator: its word there is trunc(acc[v - j]), without the + 1 of a non-zero low half"""
    N = acc.shape[-1]
    base = RM.extract(acc, v, 64)
    for j in range(1, v + 1):
        base[..., 1:, N - j] = ((np.uint64(0) - (acc[..., 1:, v - j] >> np.uint64(32))) & np.uint64(0xFFFFFFFF)) << np.uint64(32)
    return base


@pytest.mark.parametrize("p", [p for p in _at_sets() if p.W == 64], ids=EC.sid)
def test_the_borrow_class_separates_the_oracle_from_a_negation_moved_across_the_truncation(p):
    """the mutant changes an output word of the oracle's key switch for every v >= 1, in every ciphertext: the GPU comparison at these
    accumulators sees a kernel that drops the + 1"""
    crs, keys = keygen(p, 12)
    so = oracle_scheme(p, crs, keys)
    B = 2
    for v in (EC.KS_AT_FULL_COEFS(p) if p in EC.KS_AT_FULL else EC.KS_AT_COEFS(p)):
        acc = ks_edge_acc_at(p, np.random.default_rng(4), B, v)
        good, bad = RM.extract(acc, v, 64), _mutant_base(acc, v)
        if v == 0:
            assert np.array_equal(good, bad)
            continue
        for b in range(B):
            assert not np.array_equal(so.keyswitch(good[b]), so.keyswitch(bad[b])), (v, b)
    # and the restatement is the mutant: where the low half is 0 it is the right word
    x = np.zeros((1, 2, 8), dtype=np.uint64)
    x[0, 1, :3] = [5 << 32, (5 << 32) | 1, (1 << 64) - 1]
    g, m = RM.extract(x, 4, 64), _mutant_base(x, 4)
    assert np.array_equal((g[0, 1, 4:7] >> np.uint64(32)) == (m[0, 1, 4:7] >> np.uint64(32)), [True, False, False])


@pytest.mark.parametrize("o", [1, 2, 8])
@pytest.mark.parametrize("p", list(dict.fromkeys(c[0] for c in EC.LUT_BOOT_CASES)), ids=EC.sid)
def test_lut_edge_tables_hold_every_class_after_every_rotation(p, o):
    """whatever target btilde rotates the table, the polynomial that the first CMux decomposes holds a boundary word of every class of its
    gadget in both halves; a packed row is the packing of o tables"""
    N, M, W = p.N, p.N // 2, p.W
    l, logB = rot_gadgets(p)[0]
    luts = lut_edge_tables(p, o)
    assert luts.shape == (2, N) and luts.dtype == np.dtype(p.ring_dtype) and not np.array_equal(luts[0], luts[1])
    for T in luts:
        for bt in sorted(set(bt_values(N, o).values()) | set(bt_values(N, 1).values())):
            tv = R.testvector(T, bt, W, p.k)
            assert not tv[1:].any()
            for k, m in _digit_classes(tv[0], l, logB, W).items():
                assert m[:M].any() and m[M:].any(), (k, bt, "both halves")
            if W == 64 and W - l * logB > 32:
                low = tv[0] & np.uint64(0xFFFFFFFF)
                assert (low == 0xFFFFFFFF).any() and (low == 0x80000000).any()


# ---------------------------------------------------------------- 1b. the compile-time-gadget instantiations and their cases
_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mktfhe_amd", "csrc")
# launcher of a specialised instantiation -> (source file, kernel name of its cases, positions of LB, LT, BT, NP among its template arguments;
# None: the launcher has no such argument).  launch_rot_lt<LM, WORD, LB, LR, NB, LT, BT = 0>, launch_blk_lt<LM, WORD, LB, G, LT, BT, NP = 2>,
# launch_ccs_one / launch_ccs_pipe_one<LM, WORD, LT, BT>
_LAUNCHERS = {
    "launch_rot_lt": ("kernels.hip", "blindrotate_k1_kernel", 2, 5, 6, None),
    "launch_blk_lt": ("rot_block.hip", "blindrotate_blk_kernel", 2, 4, 5, 6),
    "launch_ccs_one": ("kernels.hip", "ccs_blindrotate_kernel", None, 2, 3, None),
    "launch_ccs_pipe_one": ("ccs_pipe.hip", "ccs_pipe_kernel", None, 2, 3, None),
}
_WORDS = {"uint32_t": 4, "uint64_t": 8}


def _conditions(lines, i, col):
    """the text of every `if` / `if constexpr` condition that the call at lines[i][:col] sits under: the headers of the braces open at
    that point, and what stands before the call on its own line.  The branch after `{ return hipErrorInvalidValue; } else {` holds the
    NEGATION of its header (a chain of ||): there each `x != v` reads `x == v`, and what is no equality is dropped"""
    stack = []
    for ln in lines[:i]:
        code = ln.split("//")[0]
        for m in re.finditer(r"[{}]", code):
            if m.group() == "}":
                if stack:
                    stack.pop()
                if re.match(r"\s*else\s*\{", code[m.end():]) and re.search(r"\{\s*return hipErrorInvalidValue;\s*$", code[:m.start()]):
                    head = code[:code.index("{")]
                    stack.append(" && ".join(a.replace("!=", "==") for a in head.split("||") if "!=" in a))
                    break
            else:
                stack.append(code[:m.start()] if re.search(r"\bif\b", code[:m.start()]) else "")
    return " && ".join(stack + [lines[i][:col]])


def _one_of(cond, pattern, every):
    """the values that `pattern == v` admits in a conjunction of conditions (a parenthesised `x == 1 || x == 3` admits both); none named: every"""
    found = [int(v) for v in re.findall(pattern + r" == (\d+)", cond)]
    return sorted(set(found)) if found else list(every)


def source_specialisations():
    """every (launcher, LM, word bytes, LB, NP, l, logB) whose gadget length is a non-zero literal in a launcher call of the sources (logB 0:
    the base stays a run-time value); a template argument or a condition that the call leaves open expands over every value the dispatch has"""
    out = []
    for name, (fname, _, i_lb, i_lt, i_bt, i_np) in _LAUNCHERS.items():
        lines = open(os.path.join(_CSRC, fname)).read().split("\n")
        for i, ln in enumerate(lines):
            for m in re.finditer(name + r"<([^<>()]*)>\(a, ", ln.split("//")[0]):
                args = [a.strip() for a in m.group(1).split(",")]
                lt, bt = args[i_lt], args[i_bt] if i_bt < len(args) else "0"
                if not (lt.isdigit() and int(lt) > 0):
                    continue
                assert bt.isdigit(), (fname, i + 1, "a literal gadget length with a base that is no literal")
                cond = _conditions(lines, i, m.start())
                assert re.search(r"a\.l == " + lt + r"\b", cond) and (bt == "0" or re.search(r"a\.logB == " + bt + r"\b", cond)), (fname, i + 1, cond)
                words = [_WORDS[args[1]]] if args[1] in _WORDS else _one_of(cond, r"sizeof\(WORD\)", (4, 8))
                lbs = [None] if i_lb is None else [int(args[i_lb])] if args[i_lb].isdigit() else _one_of(cond, "LB", (1, 2, 3, 4))
                np_ = None if i_np is None else int(args[i_np]) if i_np < len(args) else 2
                for lm in _one_of(cond, "LM", ()):
                    out += [(name, lm, w, lb, np_, int(lt), int(bt)) for w in words for lb in lbs]
                assert _one_of(cond, "LM", ()), (fname, i + 1, "a specialisation at every ring size: name the sizes here")
    return out


def _case_shape(p, kernel):
    """what the dispatch reads of a set: (log2 M, word bytes, block length as the rotation kernels see it, accumulator polynomials of a
    rotation, the gadget of the kernel's digit loop)"""
    block = p.scheme in (mk.LMSS, mk.KMS_BLOCK)
    gadget = (p.l_uni, p.logB_uni) if p.scheme == mk.CCS else (p.l_gsw, p.logB_gsw)
    kr = 1 if p.scheme in (mk.KMS, mk.KMS_BLOCK) else p.k
    return p.N.bit_length() - 2, p.W // 8, p.blk_len if block else 1, kr + 1, gadget


def test_every_specialisation_in_the_source_has_a_rotation_case():
    """a launcher call with a literal gadget is an instantiation of its own, which only its own shipped shape reaches: each has a line in
    ROT_CASES whose set has that ring size, word, block length and gadget and which expects that pair"""
    specs = source_specialisations()
    assert {s[0] for s in specs} == set(_LAUNCHERS), "the reader found no specialisation of a launcher: has the source changed its form?"
    assert len(set(specs)) == len(specs)
    missing = []
    for (name, lm, w, lb, np_, l, logB) in specs:
        kernel = _LAUNCHERS[name][1]
        hit = False
        for (p, opts, k, B, static) in EC.ROT_CASES:
            LM, word, LB, NP, gadget = _case_shape(p, k)
            hit |= (k == kernel and static == (l, logB) and LM == lm and word == w and lb in (None, LB) and np_ in (None, NP)
                    and gadget[0] == l and (logB == 0 or gadget[1] == logB))
        if not hit:
            missing.append((name, lm, w, lb, np_, l, logB))
    assert not missing, missing
    print(f"{len(specs)} specialisations, each with a case")


def _dispatch_static(p, opts, kernel):
    """the launchers' conditions restated (launch_rot_one, launch_blk_g / launch_blk_np, launch_ccs_blindrotate / launch_ccs_pipe,
    launch_wide_lm): the (gadget length, log2 base) that the instantiation serving this set holds as constants"""
    LM, word, LB, NP, (l, logB) = _case_shape(p, kernel)
    if kernel == "blindrotate_wide_kernel":
        return (l, 0)                                                          # the gadget length is always a template argument, the base never
    if kernel in ("ccs_blindrotate_kernel", "ccs_pipe_kernel"):
        return (l, logB) if word == 4 and LM in (9, 10) and (l, logB) in ((3, 8), (4, 8), (5, 6)) else (0, 0)
    if kernel == "blindrotate_k1_kernel":
        if LB == 1 and LM == 9 and l == 2:
            return (2, 16) if logB == 16 and word == 8 else (2, 0)
        if LB in (1, 3) and LM == 9 and word == 4 and (l, logB) == (3, 9):
            return (3, 9)
        if LB in (1, 3) and LM == 10 and word == 8 and (l, logB) in ((3, 12), (5, 8), (4, 9), (6, 7)):
            return (l, logB)
        return (0, 0)
    if kernel == "blindrotate_blk_kernel":
        if NP == 2:
            if LB == 3 and ((LM == 9 and word == 4 and (l, logB) == (3, 9)) or (LM == 10 and word == 8 and (l, logB) == (3, 12))):
                return (l, logB)
            return (0, 0)
        return (3, 7) if NP == 3 and LB == 3 and LM == 9 and word == 4 and (l, logB) == (3, 7) else (0, 0)
    assert kernel in ("blindrotate_kr_kernel", "blindrotate_kany_kernel"), kernel
    return (0, 0)


@pytest.mark.parametrize("i", range(len(EC.ROT_CASES)), ids=lambda i: "-".join([EC.sid(EC.ROT_CASES[i][0]), EC.ROT_CASES[i][2]]))
def test_every_rotation_case_expects_the_pair_of_its_instantiation(i):
    p, opts, kernel, B, static = EC.ROT_CASES[i]
    assert static == _dispatch_static(p, opts, kernel), (EC.sid(p), opts, kernel)


def test_the_specialised_sets_keep_their_shipped_shape():
    """each rotation set at a compile-time base keeps N (CCS: or 2048), W, block length and gadgets of the shipped set it reduces; the whole-bootstrap
    list ends with one such line per kernel family, behind every line that LUT_BOOT_CASES picks by position"""
    shipped = {q.name: q for q in vars(mk).values() if isinstance(q, mk.Params)}
    for (p, opts, kernel, B, static) in EC.ROT_CASES:
        if static[1] and p.name in shipped:
            q = shipped[p.name]
            assert (p.W, p.blk_len, p.l_gsw, p.logB_gsw, p.l_uni, p.logB_uni) == (q.W, q.blk_len, q.l_gsw, q.logB_gsw, q.l_uni, q.logB_uni), EC.sid(p)
            assert p.N == q.N or (p.scheme == mk.CCS and p.N == 2048), EC.sid(p)
    rot = {(EC.sid(p), tuple(sorted(o.items())), k): s for (p, o, k, B, s) in EC.ROT_CASES}
    tail = [rot[(EC.sid(p), tuple(sorted(o.items())), k)] for (p, o, k) in EC.BOOT_CASES[14:]]
    assert tail == [(2, 16), (3, 9), (3, 8)] and EC.GATE_CASES is EC.BOOT_CASES


# ---------------------------------------------------------------- 2. the oracle's composition identity on the crafted rows
@pytest.mark.parametrize("p", EC.GATE_SETS, ids=EC.sid)
def test_oracle_bootstrap_is_the_composition_of_its_stages_on_edge_rows(p):
    crs, keys = keygen(p, 11)
    so = oracle_scheme(p, crs, keys)
    rows, kinds = lwe_edge_rows(p, np.random.default_rng(4))
    for row, kind in zip(rows, kinds):
        at, bt = so.modswitch(row)
        assert np.array_equal(so.bootstrap(row), so.keyswitch(so.blindrotate(at, so.testvector(bt)))), kind
        if kind in ("zero", "skip"):                                          # nothing rotates: the key switch of the test vector itself
            assert np.array_equal(so.bootstrap(row), so.keyswitch(so.testvector(bt)))
    # an accumulator word of all ones key-switches like a zero word under the unbalanced gadget: the carry leaves the field
    if p.scheme not in (mk.LMSS, mk.KMS_BLOCK):
        a0 = np.zeros((1 + p.k, p.N), dtype=np.uint64)
        a1 = a0.copy()
        a1[1, 0] = (1 << p.W) - 1
        assert np.array_equal(so.keyswitch(a0), so.keyswitch(a1))


def test_gate_inputs_reproduce_the_crafted_rows():
    """x with gate_linear(op, x, 0) == row for the six gates (helpers.gate_input); XOR / XNOR reach even words only"""
    p = EC.GATE_SETS[0]
    for op in range(6):
        rows, _ = lwe_edge_rows(p, np.random.default_rng(5), even=op in (3, 4))
        x = gate_input(op, rows)
        for j in range(len(rows)):
            assert np.array_equal(O.gate_linear(op, x[j], np.zeros_like(x[j])), rows[j]), op


# ---------------------------------------------------------------- 3. each class separates the oracle from a plausible wrong variant
@pytest.mark.parametrize("N", [64, 256, 1024, 4096])
def test_modswitch_classes_discriminate(N):
    s = 32 - (N.bit_length() - 1) - 1
    h = 1 << (s - 1)
    mw = modswitch_words(N)
    ora = {k: _switch(w, N) for k, w in mw.items()}
    assert [ora[k] for k in ("zero", "max->0", "tie->1", "->N-1", "tie->N", "->N", "max->N", "tie->N+1", "->2N-1", "min->2N", "ones->2N")] == \
        [0, 0, 1, N - 1, N, N, N, N + 1, 2 * N - 1, 2 * N, 2 * N]
    for k in ("tie->1", "tie->N", "tie->N+1", "min->2N", "ones->2N"):
        assert mw[k] >> s != ora[k], ("a plain shift (truncation)", k)
    for k in ("tie->1", "tie->N", "tie->N+1", "min->2N"):
        assert (mw[k] + h - 1) >> s != ora[k], ("ties rounded down", k)
    assert ora["min->2N"] & (2 * N - 1) != ora["min->2N"], "the full turn reduced mod 2N (entry 2N of the monomial table is its own)"
    assert (mw["max->0"] != 0) != (ora["max->0"] != 0), "the skip decided on the raw word"
    for t, (lo, hi) in btilde_words(N).items():
        v = {"0": 0, "1": 1, "N-1": N - 1, "N": N, "N+1": N + 1, "2N-1": 2 * N - 1, "2N": 2 * N}[t]
        assert _switch(lo, N) == v == _switch(hi, N)
        assert lo == 0 or _switch(lo - 1, N) == v - 1
        assert hi == 2**32 - 1 or _switch(hi + 1, N) == v + 1


@pytest.mark.parametrize("W", [32, 64])
def test_testvector_classes_discriminate(W):
    N = 64
    so = O.Scheme(O.OraParams(O.CGGI, 4, N, 1, W, 2, 8, 0, 0, 0, 0, 8, 2, 0, 0))
    e, m = 1 << (W - 3), (1 << W) - 1
    i = np.arange(N)

    def tv(bt, above=lambda tb: tb > N, below=lambda i, tb: i < tb, flip=True):
        lo, hi = e, (-e) & m
        if above(bt):
            bt -= N
            if flip:
                lo, hi = hi, lo
        return np.where(below(i, bt), lo, hi).astype(np.uint64)

    vals = {"0": 0, "1": 1, "N-1": N - 1, "N": N, "N+1": N + 1, "2N-1": 2 * N - 1, "2N": 2 * N}
    for t in BT_TARGETS:
        bt = vals[t]
        want = so.testvector(bt)[0]
        assert np.array_equal(tv(bt), want), t
        # `tb >= N` in place of `tb > N` is the SAME function: at tb == N either branch writes +1/8 to all N coefficients
        assert np.array_equal(tv(bt, above=lambda tb: tb >= N), want), t
    differs = lambda **kw: {t for t in BT_TARGETS if not np.array_equal(tv(vals[t], **kw), so.testvector(vals[t])[0])}      # noqa: E731
    assert differs(below=lambda i, tb: i <= tb) >= {"0", "1", "N-1", "N+1", "2N-1"}, "i <= tb for i < tb"
    assert differs(flip=False) >= {"N+1", "2N-1", "2N"}, "the sign not flipped above N"
    assert differs(above=lambda tb: tb > N + 1) >= {"N+1"}, "the half turn taken one late"
    assert differs(above=lambda tb: tb >= N - 1) >= {"N-1"}, "the half turn taken one early"


def _digits_variant(x, l, logB, W, mode):
    """gsw.jl:42-52 in Python integers, in the kernels' form (digit j = field j of divbits(x, W - l logB) + sum_j B/2 B^j, minus B/2),
    with one step changed: "trunc" a plain shift for divbits; "tiedown"; "carry" the top field keeps what lies above its logB bits"""
    bit, B, m = W - l * logB, 1 << logB, (1 << W) - 1
    a = x >> bit if mode == "trunc" else (x + (1 << (bit - 1)) - (mode == "tiedown")) >> bit if bit else x
    tp = a + sum((B >> 1) << (logB * j) for j in range(l))
    return [(((tp >> (logB * (l - 1 - j))) & (B - 1 if (j or mode != "carry") else ~0)) - (B >> 1)) & m for j in range(l)]


@pytest.mark.parametrize("l,logB,W", sorted({(l, logB, p.W) for p in EC.all_rotation_sets() for (l, logB) in rot_gadgets(p)}
                                             | {(p.f, p.logD, 32) for p in EC.KS_SETS}))
def test_gadget_classes_discriminate(l, logB, W):
    gw = gadget_words(l, logB, W)
    ora = {k: [int(v) for v in O.decomp_word(x, l, logB, W)] for k, x in gw.items()}
    for k, x in gw.items():
        assert _digits_variant(x, l, logB, W, "ok") == ora[k], k                                       # the restatement is the oracle's function
    half, m = 1 << (logB - 1), (1 << W) - 1
    assert ora["all-min"] == [(-half) & m] * l and ora["all-max"] == [half - 1] * l and ora["top-min"][0] == (-half) & m
    assert _digits_variant(gw["all-min"], l, logB, W, "carry") != ora["all-min"], "the carry of the prepared value kept in the top digit"
    if W - l * logB >= 1:
        assert ora["round-carry"] == [0] * l and ora["tie->all-min"] == ora["all-min"]
        assert _digits_variant(gw["round-carry"], l, logB, W, "carry") != ora["round-carry"], "the rounding carry kept"
        for k in ("tie", "round-carry", "tie->all-min"):
            assert _digits_variant(gw[k], l, logB, W, "trunc") != ora[k], ("truncation", k)
            assert _digits_variant(gw[k], l, logB, W, "tiedown") != ora[k], ("tie down", k)
        assert _digits_variant(gw["tie-1"], l, logB, W, "trunc") == ora["tie-1"]                        # one below the tie: both agree, the tie alone tells


@pytest.mark.parametrize("f,logD", sorted({(p.f, p.logD) for p in EC.KS_SETS + EC.KS_CHILD_SETS}))
def test_keyswitch_classes_discriminate(f, logD):
    Lb, bit, D = f * logD, 32 - f * logD, 1 << logD
    kw = ks_words(f, logD)
    dig = lambda w: [int(v) for v in O.unbalanced_decomp_word(w, f, logD, 32)]      # noqa: E731
    assert dig(kw["all-D-1"]) == [D - 1] * f and dig(kw["zero"]) == [0] * f
    if bit >= 1:
        v = O.divbits(kw["u-carry"], bit, 32)
        assert v == 1 << Lb and dig(kw["u-carry"]) == [0] * f                       # like the zero word
        assert [(v >> (logD * (f - 1 - t))) & (D - 1 if t else ~0) for t in range(f)] != dig(kw["u-carry"]), "the carry kept in the top digit's index (no & Dm)"
        assert dig(kw["u-carry-1"]) == [D - 1] * f
        assert [(kw["u-tie"] >> bit >> (logD * (f - 1 - t))) & (D - 1) for t in range(f)] != dig(kw["u-tie"]), "truncation"
        assert [(kw["u-tie-1"] >> bit >> (logD * (f - 1 - t))) & (D - 1) for t in range(f)] == dig(kw["u-tie-1"])
    # 64-bit ring: the extracted word is the HIGH half, cut off (bootstrapping.jl:575): rounding the low half in gives another word
    p = mk.KMS2party.scaled(n=4, N=64)
    a = np.zeros(64, dtype=np.uint64)
    a[0], a[63] = (5 << 32) | 0xFFFFFFFF, (7 << 32) | 0x80000000
    w = extract_words(p, a)
    assert int(w[0]) == 5 and int(w[1]) == (-7) & 0xFFFFFFFF
    assert ((int(a[0]) + (1 << 31)) >> 32) != int(w[0]) and (-((int(a[63]) + (1 << 31)) >> 32)) & 0xFFFFFFFF != int(w[1])
    assert int(extract_words(p, np.full(64, 1 << 63, dtype=np.uint64))[1]) == 0x80000000                # -x wraps to itself
