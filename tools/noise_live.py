"""The record behind tests/test_gpu_noise.py: the same harness (tests/noise_cases.py) on the same cases, measured and printed instead of
asserted.  One JSON line per case -- set, mode, call, n, mean, sigma, excess kurtosis, largest error, predicted sigma
(tests/golden/noise_predicted.json), their ratio, the build id -- and:
  * the ratio to the sigma recorded in profiles/r03_noise_measured.jsonl (Float64) / profiles/r04_noise_measured_exact.jsonl (EXACT).  Not a
    check: those samples hold 256 gates on other keys and older kernels, and the KMS sets vary by +-25 % per key;
  * the native MUX also at the CCS and KMS sets, whose rotations carry coherent terms that do not add in quadrature (recorded, not asserted);
  * how many inputs of DESIGN.md 1c's P = 8 recipe leave their window under the coarse mod switch at o = 2 and o = 4, beside the prediction.
Run on the GPU box from the repository root:  python tools/noise_live.py [--out profiles/noise_live_<build id>.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import noise_cases as NC   # noqa: E402
from noise_cases import mk  # noqa: E402


def recorded():
    out = {NC.F64: {}, NC.EXACT: {}}
    for ln in open(os.path.join(ROOT, "profiles", "r03_noise_measured.jsonl")):
        d = json.loads(ln)
        if d["variant"] == "as shipped":
            out[NC.F64][d["set"]] = d["sigma_after_parties"][-1] if (d["fails"] > 0 and d["sigma_after_parties"]) else d["sigma"]
    for ln in open(os.path.join(ROOT, "profiles", "r04_noise_measured_exact.jsonl")):
        d = json.loads(ln)
        out[NC.EXACT][d["set"]] = d["sigma"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pred, old, bench, lines = NC.predicted(), recorded(), NC.Bench(), []
    build = mk.build_id()

    def emit(**r):
        r["build_id"] = build
        lines.append(r)
        print(json.dumps(r), flush=True)

    def noise_line(call, case, e, wrong, rotations=1, asserted=True):
        name, mode, impl = case[:3]
        sigma, band = NC.predicted_sigma(pred, name, mode, rotations)
        st = NC.stats(e)
        was = old[mode].get(name) if rotations == 1 else None
        emit(law="B", set=name, mode=mode, impl=impl, call=call, **st, wrong=wrong, sigma_pred=sigma, ratio=st["sigma"] / sigma, band=band,
             margin_sigmas=0.125 / sigma, asserted=asserted, sigma_recorded=was, ratio_to_recorded=st["sigma"] / was if was else None)

    try:
        for name, o in NC.SWITCH_CASES:
            eng, p, keys = bench.engine(name, NC.F64)
            r = NC.measure_switch(eng, p, keys, bench.uniform(name)[:NC.ROWS_A], o)
            emit(law="A", set=name, mode=NC.F64, call="modswitch" if o == 1 else "lut_many_testvector", **r)
        for case in NC.NAND_CASES:
            eng, p, keys = bench.engine(*case)
            ct, b = bench.bits(case[0])
            noise_line("NAND", case, *NC.measure_gate(eng, p, keys, "nand", ct[:2], b[:2]))
        for case, asserted in [(c, True) for c in NC.MUX_CASES] + [(c, False) for c in NC.MUX_RECORDED]:
            eng, p, keys = bench.engine(*case)
            ct, b = bench.bits(case[0])
            noise_line("MUX", case, *NC.measure_gate(eng, p, keys, "mux", ct, b), rotations=2, asserted=asserted)
        for case in NC.TABLE_CASES:
            eng, p, keys = bench.engine(*case)
            wrong, _, e, _ = NC.decode_call(eng, p, keys, bench.uniform(case[0])[-NC.ROWS_B:], "lut_random", np.random.default_rng(107))
            noise_line("lut_bootstrap", case, e, wrong)
        for case in NC.DECODE_CASES:
            eng, p, keys = bench.engine(*case[:3])
            wrong, bits, e, phi = NC.decode_call(eng, p, keys, bench.uniform(case[0]), case[3], np.random.default_rng(109))
            sigma, _ = NC.predicted_sigma(pred, case[0], case[1])
            st = NC.stats(e)
            emit(law="C", set=case[0], mode=case[1], impl=case[2], call=case[3], bits=bits, wrong=wrong, **st, sigma_pred=sigma, ratio=st["sigma"] / sigma,
                 reads_corners=NC.reads_the_corners(p, phi))
        for name in NC.SWITCH_SETS[:4]:
            eng, p, keys = bench.engine(name, NC.F64)
            for o in (2, 4):
                emit(law="1c window misses, P = 8", set=name, **NC.window_misses(eng, p, keys, o, NC.ROWS_A, NC.set_seed(name, 77_000)))
    finally:
        bench.close()
    if args.out:
        with open(args.out.replace("<build id>", build), "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
