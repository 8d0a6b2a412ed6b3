"""The owner of host-side device memory (mktfhe_amd/csrc/device_mem.h) without a GPU: tests/csrc/device_mem_check.cpp includes the header over
stand-in hipMalloc / hipFree that log every call, and checks the grow rule (enough: no call; too small: free, then allocate, nothing live in
between; a failed allocation leaves the buffer empty), the zero-byte allocation, release / move / destructor, and the group helper (every
member released before the first allocation, the unit count recorded last, a failure part-way leaves it 0).  The program alone is built
with AddressSanitizer and UBSan; it links without the HIP runtime."""
import os
import subprocess

from helpers import ROOT

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_device_mem_owner_and_group_rules(tmp_path):
    exe = str(tmp_path / "device_mem_check")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                           "-I" + os.path.join(ROOT, "mktfhe_amd", "csrc"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "device_mem_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith(" 0 failed checks"), (out.stdout[-2000:], out.stderr[-2000:])
