"""The owner of host-side device memory (mktfhe_amd/csrc/device_mem.h) without a GPU: tests/csrc/device_mem_check.cpp includes the header over
stand-in hipMalloc / hipFree that log every call, and checks the grow rule (enough: no call; too small: free, then allocate, nothing live in
between; a failed allocation leaves the buffer empty), the zero-byte allocation, release / move / destructor, and the group helper (every
member released before the first allocation, the unit count recorded last, a failure part-way leaves it 0).  The program alone is built
with AddressSanitizer and UBSan; it links without the HIP runtime.

The guard mode (MKT_MEM_GUARD): with it off the program makes no runtime call but hipMalloc / hipFree, and the log of its first part is, call
for call, the one the header gave before it had the mode (OFF_CALLS, OFF_DIGEST: FNV-1a over kind, size and live allocations of every call,
taken from that header).  With it on: the sizes, the pointers, the same rules, and a byte stored into either guard found once by the sweep
and by release.  That the detector can fail is shown by the same program with its read-back stubbed to "clean": it must not pass."""
import os
import subprocess

import pytest

from helpers import ROOT

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
OFF_CALLS, OFF_DIGEST = 43, "56753cbc3f4e88fd"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("device_mem") / "device_mem_check")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                           "-I" + os.path.join(ROOT, "mktfhe_amd", "csrc"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "device_mem_check.cpp"), "-o", exe])
    return exe


def test_device_mem_owner_and_group_rules(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith(" 0 failed checks"), (out.stdout[-2000:], out.stderr[-2000:])
    assert f"mode off: {OFF_CALLS} runtime calls, digest {OFF_DIGEST}\n" in out.stdout, ("the call log with the guard mode off changed", out.stdout[-500:])


def test_guard_sweep_stubbed_clean_is_noticed(exe):
    """the stand-in read-back hands the sweep untouched guards: every check that a written guard is found must fail, and no other"""
    out = subprocess.run([exe, "stub-clean"], capture_output=True, text=True)
    assert out.returncode == 1 and not out.stdout.strip().endswith(" 0 failed checks"), (out.stdout[-2000:], out.stderr[-2000:])
    assert "G::sweep(0) == 1 && last_is(false, 64, GLEN - 1)" in out.stdout and "check_reserve" not in out.stdout
    assert f"mode off: {OFF_CALLS} runtime calls, digest {OFF_DIGEST}\n" in out.stdout
