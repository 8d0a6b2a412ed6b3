"""fft_device.h native() / native_add() with the exact steps fused: tests/csrc/native_fused_check.cpp restates arithmetic.jl:1-9 literally
(multiply, floor, multiply, subtract, compare, convert) and the device bodies with std::fma and a truncate-and-saturate convert, and
compares them on the input classes of native_check.cpp: specials and their neighbours, every binade from 2^-60 to 2^120 with both
signs, values just below and just above multiples of 2^32 and 2^64."""
import os
import re
import subprocess

from helpers import ROOT


def test_fused_native_forms_match_the_reference_form(tmp_path):
    exe = str(tmp_path / "native_fused_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "csrc", "native_fused_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith(" 0 mismatches"), out.stdout[-500:]
    assert int(out.stdout.split()[0]) > 20_000_000


def test_device_bodies_are_the_ones_the_check_restates():
    """A tripwire, no proof: the three fused expressions stand in the header as the check restates them.  It trips on a harmless
    reformatting too, and it does not see the rest of native_halves (the convert of the low half, the 2^52 sum kept for the high
    half): those are what tests/test_gpu_native_fused.py compares on the device."""
    src = open(os.path.join(ROOT, "mktfhe_amd", "csrc", "fft_device.h")).read()
    chk = open(os.path.join(ROOT, "tests", "csrc", "native_fused_check.cpp")).read()
    flat = lambda s: re.sub(r"\s+", "", s)
    for dev, host in (("__builtin_fma(floor(x * 5.421010862427522e-20), -1.8446744073709552e19, x)", "std::fma(floor(x*5.421010862427522e-20),-1.8446744073709552e19,x)"),
                      ("__builtin_fma(hi, -4.294967296e9, x)", "std::fma(hi,-4.294967296e9,x)"),
                      ("__builtin_fma(floor(x * 2.3283064365386963e-10), -4.294967296e9, x)", "std::fma(floor(x*2.3283064365386963e-10),-4.294967296e9,x)")):
        assert flat(dev) in flat(src) and flat(host) in flat(chk), dev
    assert "#pragma clang fp contract(off)" in src
