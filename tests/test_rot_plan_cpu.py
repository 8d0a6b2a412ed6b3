"""The launch rules of the blind rotation (mktfhe_amd/csrc/rot_plan.h) without a GPU, by two stand-alone programs.

tests/csrc/rot_plan_check.cpp includes the header alone (AddressSanitizer, UBSan) and walks every family's plan over transform sizes, ring
widths, gadget and block lengths, every switch value, every capability flag both ways and every count from 1 to 4200 (and 8191 .. 8193): the
segments cover [0, count) in order without gap or overlap, every launch has a rotation, no kernel is planned whose capability is off, a grouped
segment is a whole number of slots; and the fixed points of the k1 rule at M = 512.

tests/csrc/launch_log.cpp is the behaviour check: the library's units that hold rotation launchers, compiled host-only and linked against a
stand-in HIP runtime that logs every launch (kernel instantiation, grid, workgroup, LDS bytes, block0).  The same source was built against the
csrc of the commit before the header existed (PARENT; there the CCS rule of do_blindrotate stands in the program, see its head): PARENT_LINES
and PARENT_DIGEST are what that build printed, and this tree must print the same -- launch for launch what the parent launched."""
import os
import re
import subprocess

import pytest

from helpers import LAUNCH_LOG_CSRC as CSRC, ROOT, build_launch_log

PARENT = "2bc678c"
PARENT_LINES, PARENT_DIGEST = 1076909, "d962c193e7d1c656"


@pytest.fixture(scope="module")
def launch_log(tmp_path_factory):
    exe = build_launch_log(CSRC, str(tmp_path_factory.mktemp("launch_log")))
    out = subprocess.run([exe, "log"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def test_rot_plan_rules(tmp_path):
    exe = str(tmp_path / "rot_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + CSRC, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                           os.path.join(ROOT, "tests", "csrc", "rot_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith(" 0 failed checks"), (out.stdout[-2000:], out.stderr[-2000:])
    assert int(re.search(r"(\d+) plans", out.stdout).group(1)) > 10_000_000, out.stdout[-500:]


def test_launches_are_the_parents(launch_log):
    assert launch_log.endswith(f"{PARENT_LINES} lines, digest {PARENT_DIGEST}\n"), (f"the launches differ from those of {PARENT}", launch_log[-200:])


def _calls(log):
    """[(head line, [launch lines])]"""
    calls = []
    for ln in log.split("\n"):
        if ln.startswith("  -> ") or not ln or " lines, digest " in ln:
            continue
        if ln.startswith("  "):
            calls[-1][1].append(ln.strip())
        else:
            calls.append((ln, []))
    return calls


def test_the_log_is_not_empty_or_short(launch_log):
    """a log that misses a kernel kind, a specialised instantiation or the multi-launch cases cannot pass on its digest alone"""
    calls = _calls(launch_log)
    kernels = {ln.split(" grid ")[0] for _, ls in calls for ln in ls}
    # every kernel kind of the plan (RotKernel): PLAIN, BLOCK, WIDE, GROUPED, KR, FX, CCS, CCS_PIPE and the four of EXACT KMS phase 1
    kinds = {"PLAIN": r"blindrotate_k1_kernel<\d+, unsigned (int|long), 1,", "BLOCK": r"blindrotate_k1_kernel<\d+, unsigned (int|long), [234],",
             "WIDE": r"blindrotate_wide_kernel<", "GROUPED": r"blindrotate_blk_kernel<", "KR": r"blindrotate_kr_kernel<", "FX": r"fx_blindrotate_kernel<",
             "CCS": r"ccs_blindrotate_kernel<", "CCS_PIPE": r"ccs_pipe_kernel<", "XKMS_BLOCK_WIDE": r"exact_kms_block_phase1_kernel<",
             "XKMS_BLOCK": r"exact_kms_phase1_kernel<\d+, true>", "XKMS_P2PF": r"exact_kms_phase1_p2pf_kernel<", "XKMS": r"exact_kms_phase1_kernel<\d+, false>"}
    missing = [k for k, pat in kinds.items() if not any(re.match(pat, n) for n in kernels)]
    assert not missing, (missing, sorted(kernels)[:40])
    # every (rot_static_l, rot_static_logB) instantiation that tests/test_gpu_edges.py asserts for the shipped sets (edge_cases.ROT_CASES): the
    # pair closes the template arguments of its kernel
    import edge_cases as EC
    pairs = {(k, static) for (_, _, k, _, static) in EC.ROT_CASES if static[0] and k != "blindrotate_wide_kernel"}
    assert len(pairs) >= 10, pairs
    for k, (l, logB) in sorted(pairs):
        pat = {"blindrotate_blk_kernel": rf"{k}<.*, {l}, {logB}, \d>$"}.get(k, rf"{k}<.*, {l}, {logB}>$")
        assert any(re.match(pat, n) for n in kernels), (k, l, logB, sorted(n for n in kernels if n.startswith(k))[:20])
    wide = {static[0] for (_, _, k, _, static) in EC.ROT_CASES if k == "blindrotate_wide_kernel"}
    for l in wide:
        assert any(re.match(rf"blindrotate_wide_kernel<.*, {l}>$", n) for n in kernels), l
    # a multi-launch entry of each cutting rule of k1 (a last fill to the latency kernel; one fill and a remainder as two equal launches), of
    # the chip-fill rule of the Float64-pipe kernel, and of rot_split
    by_head = dict(calls)
    tail = by_head["k1 CGGIparam n 1280 variant 0 wide 0 blkg 0 split 0"]
    assert [(ln.split("<")[0], ln.split(" grid ")[1].split(" ")[0] + ln[ln.index(" block0"):]) for ln in tail] == [("blindrotate_k1_kernel", "1024 block0 0"), ("blindrotate_wide_kernel", "256 block0 1024")], tail
    halves = by_head["k1 CGGIparam n 1312 variant 0 wide 0 blkg 0 split 0"]
    assert [ln.split(" grid ")[1].split(" ")[0] + ln[ln.index(" block0"):] for ln in halves] == ["656 block0 0", "656 block0 656"], halves
    fills = by_head["fx KMS2party_N1024_l2 n 2304 split 0"]
    assert [ln.split(" grid ")[1].split(" ")[0] + ln[ln.index(" block0"):] for ln in fills] == ["1024 block0 0", "1024 block0 1024", "256 block0 2048"], fills
    split = by_head["k1 CGGIparam n 257 variant 0 wide 1 blkg 0 split 100"]
    assert [ln.split(" grid ")[1].split(" ")[0] + ln[ln.index(" block0"):] for ln in split] == ["100 block0 0", "100 block0 100", "57 block0 200"], split
    assert len(calls) > 50_000 and sum(len(ls) for _, ls in calls) > 2 * len(calls)
