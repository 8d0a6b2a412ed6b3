#!/usr/bin/env python3
"""Time of generating a party's seeded key form on its own GPU against the two ways that existed before, on the GPU.

For each parameter set, for one party with a pinned seed, on one context with the device pinned, alternating, after one warm-up of each:
  host     party_keygen_seeded(...)                               mkt_client_party_keygen_seeded: the host loop, the compact sections
  full     Scheme.keygen_device(party, secrets, export=True)      mkt_keygen_device_export: the full keys made on the GPU and copied out
  seeded   keygen_device_seeded(scheme, party, secrets, mask)     mkt_keygen_device_seeded with outputs, install = 0: the compact sections
Every device call returns after a device synchronise (the outputs have landed on the host), so a host clock around it is the call's time.
The sections of `seeded` are checked against those of `host` word for word.  Prints one JSON line and writes it to --out with the library's
build id.  A measurement path: it fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mktfhe_amd as mk  # noqa: E402

MASK_SEED = bytes(range(32, 64))


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def measure(p, party, reps, device):
    crs = mk.CRS(p, 1) if p.multikey else None
    secrets = mk.party_keygen(crs, p, party=party, secrets_only=True, deterministic_seed=1)
    sch = mk.Scheme(p, device=device)
    last = {}

    def host():
        last["host"] = mk.party_keygen_seeded(crs, p, party=party, mask_seed=MASK_SEED, deterministic_seed=1)

    def full():
        last["full"] = sch.keygen_device(party, secrets, export=True)
        sch.synchronize()

    def seeded():
        last["seeded"] = mk.keygen_device_seeded(sch, party, secrets, mask_seed=MASK_SEED)
        sch.synchronize()

    calls = {"host": host, "full": full, "seeded": seeded}
    for fn in calls.values():
        fn()                                            # warm-up: code objects, first allocations
    ms = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():                  # alternating
            ms[name].append(timed(fn))
    h, d = last["host"], last["seeded"]
    assert np.array_equal(d.brk_seeded, h.brk_seeded) and np.array_equal(d.ksk_seeded, h.ksk_seeded), "the device sections are not the host's"
    brk, ksk = last["full"]
    sch.close()
    return {
        "set": p.name, "party": party, "reps": reps,
        "compact_bytes": int(32 + d.brk_seeded.nbytes + d.ksk_seeded.nbytes), "full_bytes": int(brk.nbytes + ksk.nbytes),
        "ms_median": {n: round(statistics.median(v), 3) for n, v in ms.items()}, "ms_min": {n: round(min(v), 3) for n, v in ms.items()},
        "ms_max": {n: round(max(v), 3) for n, v in ms.items()},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="CGGIparam:0,KMS2party:1", help="comma-separated set:party")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "a GPU is required: nothing here is measured on a CPU"
    res = {"tool": "seeded_keygen_time", "build_id": mk.build_id(), "device": torch.cuda.get_device_name(a.device), "results": []}
    for item in a.sets.split(","):
        name, _, party = item.partition(":")
        res["results"].append(measure(getattr(mk, name), int(party or 0), a.reps, a.device))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
