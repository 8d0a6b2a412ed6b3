"""No rotation instantiation without a case, checked without a GPU.

tests/csrc/launch_log.cpp stands in for the HIP runtime over the library's rotation units: `kernels` prints every instantiation compiled into
them (registered, launched or not), `reach` answers which of them a shape under an option setting launches, through the same public launchers
and the route of context.cpp.  Held against tests/size_ladder.py and the rotation cases of tests/edge_cases.py:

(a) every entry reaches the kernel it names, at the transform size and word type of its parameter set;
(b) every registered instantiation of a rotation kernel is claimed by an entry, or excluded -- and an exclusion holds only where its predicate
    is true of the instantiation and a sweep of admitted shapes and switch values does not reach it;
(c) the control: with one ladder row removed, (b) names the instantiation that row alone reached."""
import itertools
import re
import subprocess

import pytest

import edge_cases as EC
import size_ladder as SL
from helpers import LAUNCH_LOG_CSRC, build_launch_log, mk

SCHEME = {mk.CGGI: "CGGI", mk.LMSS: "LMSS", mk.CCS: "CCS", mk.KMS: "KMS", mk.KMS_BLOCK: "KMS_BLOCK"}
ROTATION = re.compile(r"(blindrotate_(k1|wide|blk|kr|kany)_kernel|kms_phase2_kernel|ccs_blindrotate_kernel|ccs_pipe_kernel|fx_blindrotate_kernel|"
                      r"exact_(blindrotate|blindrotate_kr|blindrotate_kany|kms_phase1|kms_phase1_p2pf|kms_block_phase1|kms_phase2|ccs)_kernel)<")


def reach_line(tag, p, opts, exact, count):
    ccs, kms, block = p.scheme == mk.CCS, p.scheme in (mk.KMS, mk.KMS_BLOCK), p.scheme in (mk.LMSS, mk.KMS_BLOCK)
    f = dict(tag=tag, scheme=SCHEME[p.scheme], N=p.N, k=p.k, W=p.W, l=p.l_uni if ccs else p.l_gsw, logB=p.logB_uni if ccs else p.logB_gsw,
             blk_len=p.blk_len if block else 1, rows=1 + (p.k - 1) * p.l_lev if kms else 1, count=count,
             variant=opts.get("rot_variant", 0), wide=opts.get("rot_wide", 0), blkg=opts.get("rot_blkg", 0), split=opts.get("rot_split", 0),
             ccs_pipe=opts.get("ccs_pipe", -1), exact=int(exact), exact_wide=opts.get("exact_wide", 1), exact_kany=opts.get("exact_kany", 0),
             exact_impl=opts.get("exact_impl", -1))
    return " ".join(f"{k}={v}" for k, v in f.items())


def entries():
    """(source, row index, parameter set, options, kernel, EXACT, batch size) of every entry that may claim an instantiation"""
    out = []
    for i, (p, walk) in enumerate(SL.LADDER):
        out += [("ladder", i, p, o, k, False, SL.B) for o, k in walk]
    for i, (p, walk) in enumerate(SL.EXACT_LADDER):
        out += [("exact-ladder", i, p, o, k, True, SL.B) for o, k in walk]
    out += [("edge", i, c[0], c[1], c[2], False, c[3]) for i, c in enumerate(EC.ROT_CASES)]
    out += [("exact-edge", i, c[0], c[1], c[2], True, c[3]) for i, c in enumerate(EC.EXACT_CASES)]
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_launch_log(LAUNCH_LOG_CSRC, str(tmp_path_factory.mktemp("launch_log_reach")))


def run_reach(exe, lines):
    out = subprocess.run([exe, "reach"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [ln.split(": ", 1) for ln in out.stdout.splitlines()]
    assert len(got) == len(lines)
    return [r.split(" | ") if r else [] for _, r in got]


@pytest.fixture(scope="module")
def reached(exe):
    es = entries()
    return es, run_reach(exe, [reach_line(f"e{j}", e[2], e[3], e[5], e[6]) for j, e in enumerate(es)])


@pytest.fixture(scope="module")
def registered(exe):
    out = subprocess.run([exe, "kernels"], capture_output=True, text=True, check=True).stdout.split("\n")
    return sorted(n for n in out if ROTATION.match(n))


def test_every_entry_reaches_its_kernel(reached):
    es, got = reached
    for (src, i, p, opts, kernel, exact, _), names in zip(es, got):
        assert names and not any(n.startswith("->") for n in names), (src, i, SL.sid(p), opts, names)
        size = str(p.N.bit_length() - 1 if kernel.startswith("exact_") else SL.logM(p.N))     # the integer-NTT kernels are templates over log2 N
        word = {32: "unsigned int", 64: "unsigned long"}[p.W]
        hit = [n for n in names if n.startswith(kernel + "<") and SL._targs(n)[0] == size and (kernel.startswith("exact_") or SL._targs(n)[1] == word)]
        assert hit, (src, i, SL.sid(p), opts, kernel, names)


def sweep_lines():
    """admitted shapes and documented switch values around every dispatch condition of the launchers: both widths, every scheme and size, RLWE
    lengths 1 .. 4, block lengths 1 .. 5, the gadgets the launchers name and others, every value of the kernel-selection switches"""
    lines = []
    gadgets = [(2, 16), (2, 10), (3, 9), (3, 12), (3, 7), (3, 8), (4, 8), (4, 9), (5, 8), (5, 6), (6, 7), (4, 7)]
    for N, W in itertools.product(SL.SIZES, (32, 64)):
        for l, b in gadgets:
            if l * b > W:
                continue
            sets = [mk.CGGIparam.scaled(n=3, N=N, W=W, k=k, l_gsw=l, logB_gsw=b) for k in (1, 2, 3, 4)]
            sets += [mk.Blockparam.scaled(n=3 * L, N=N, W=W, k=k, blk_d=3, blk_len=L, l_gsw=l, logB_gsw=b) for L in (1, 2, 3, 4, 5) for k in (1, 2, 3)]
            sets += [mk.KMS2party.scaled(n=3, N=N, W=W, l_gsw=l, logB_gsw=b, l_lev=2, logB_lev=7)]
            sets += [mk.KMS2partyblock.scaled(n=3 * L, N=N, W=W, blk_d=3, blk_len=L, l_gsw=l, logB_gsw=b, l_lev=2, logB_lev=7) for L in (1, 2, 3, 4, 5)]
            sets += [mk.CCS2party.scaled(n=3, N=N, W=W, l_uni=l, logB_uni=b)]
            for p in sets:
                if p.scheme == mk.CCS:
                    walks = [{"ccs_pipe": v} for v in (-1, 0, 1)]
                else:
                    walks = [{"rot_variant": v, "rot_wide": w, "rot_blkg": g} for v in (0, 21, 22) for w in (0, 1, 2) for g in (0, 1, 2, 4)]
                lines += [reach_line("s", p, o, False, count) for o in walks for count in (5, 2048)]
                lines += [reach_line("s", p, {"exact_impl": i, "exact_wide": w, "exact_kany": a}, True, 5) for i in (-1, 0, 1) for w in (0, 1) for a in (0, 1)]
    return lines


def unclaimed(registered, es, got, without=None):
    """the registered rotation instantiations that no entry reaches and no exclusion takes -> (orphans, claimed, excluded)"""
    claimed = {n for e, names in zip(es, got) if (e[0], e[1]) != without for n in names}
    excluded = {n for n in registered if any(re.fullmatch(pat, n) for pat, _, _ in SL.EXCLUSIONS)}
    return sorted(set(registered) - claimed - excluded), claimed, excluded


def test_every_registered_instantiation_is_claimed(exe, registered, reached):
    es, got = reached
    assert len(registered) > 500, len(registered)
    orphans, claimed, excluded = unclaimed(registered, es, got)
    assert claimed <= set(registered) | {n for names in got for n in names if not ROTATION.match(n)}, sorted(claimed - set(registered))[:10]
    print(f"{len(registered)} rotation instantiations registered: {len(claimed & set(registered))} claimed by {len(es)} entries, {len(excluded)} excluded")
    assert not orphans, (len(orphans), orphans[:40])
    # an exclusion states its reason as a predicate, and holds for an instantiation no admitted shape reaches
    for pat, pred, why in SL.EXCLUSIONS:
        taken = [n for n in registered if re.fullmatch(pat, n)]
        assert taken, ("an exclusion that takes nothing", pat)
        assert all(pred(SL._targs(n)) for n in taken), (pat, why)
    assert not excluded & claimed, sorted(excluded & claimed)
    swept = {n for names in run_reach(exe, sweep_lines()) for n in names}
    assert not excluded & swept, ("a reachable instantiation may not be excluded", sorted(excluded & swept))
    assert len(swept & set(registered)) > 400, len(swept & set(registered))          # (the sweep is not a sweep of nothing)


def test_a_removed_row_orphans_its_instantiation(registered, reached):
    """the must-fail control of the guard: the ladder without its N = 32 row of blindrotate_kany_kernel on the 64-bit ring"""
    es, got = reached
    row = next(i for i, (p, walk) in enumerate(SL.LADDER) if p.N == 32 and p.k == 4 and p.W == 64 and walk[0][1] == "blindrotate_kany_kernel")
    orphans, _, _ = unclaimed(registered, es, got, without=("ladder", row))
    assert orphans == ["blindrotate_kany_kernel<4, unsigned long>"], orphans
