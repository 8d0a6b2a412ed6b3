#!/usr/bin/env python3
"""Predicted output noise of a bootstrap per parameter set and arithmetic mode, as a fixture: (sigma of the blind rotation, sigma of
the key switch) in torus units from tools/noise_theory.py -- the schemes' variance formulas, nothing of the engine or the oracle.  The KMS
simulations take 6-27 s per set, which a GPU test cannot spend; tests/test_gpu_noise.py reads this file instead, and
tests/test_noise_live_cpu.py recomputes the closed forms and one simulated entry so that a change of the model cannot leave it stale.

Closed-form sets: noise_theory.predict (the same figures in both modes: the closed forms hold no Float64 term).  KMS sets: noise_theory.kms
with the trials and seeds of tests/test_noise_theory_cpu.py; "exact" sets the Float64 product error to zero, as that test does.
Regenerate from the repo root:  python tests/golden/gen_noise_predicted.py
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)
import noise_theory as T   # noqa: E402
import mktfhe_amd as mk    # noqa: E402

PATH = os.path.join(HERE, "noise_predicted.json")
CLOSED = ("CGGIparam", "Blockparam", "CCS2party")
# name -> mode -> (trials, seed): tests/test_noise_theory_cpu.py's (KMS2partyblock has no Float64 case there: the EXACT one's)
KMS = {"KMS2party_N1024_l2": {"f64": (40, 3), "exact": (40, 7)}, "KMS2partyblock": {"f64": (12, 7), "exact": (12, 7)}}


def closed(name):
    br, ks, _ = T.predict(getattr(mk, name))
    return {"sigma_br": br, "sigma_ks": ks, "kind": "closed"}


def simulated(name, mode):
    trials, seed = KMS[name][mode]
    keep = T.float64_product_error
    if mode == "exact":
        T.float64_product_error = lambda N, logB, W, ndig: 0.0
    try:
        br, ks = T.kms(getattr(mk, name), trials=trials, seed=seed, block=name.endswith("block"))
    finally:
        T.float64_product_error = keep
    return {"sigma_br": math.sqrt(br), "sigma_ks": math.sqrt(ks), "kind": "kms", "trials": trials, "seed": seed}


def make():
    out = {}
    for name in CLOSED:
        out[name] = {"f64": closed(name), "exact": closed(name)}
    for name in KMS:
        out[name] = {mode: simulated(name, mode) for mode in ("f64", "exact")}
    return out


def load():
    with open(PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    with open(PATH, "w") as f:
        json.dump(make(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(open(PATH).read())
