#!/usr/bin/env python3
"""Load time of seeded evaluation keys against the full upload, on the GPU.

For each parameter set one party's keys are generated on the host in the seeded form and expanded on the host (the full keys the existing
path uploads).  Then, on one context with the device pinned, alternating, after one warm-up of each:
  full     Scheme.load_party(party, brk=, ksk=)                 mkt_load_brk + mkt_load_ksk: the unchanged path
  seeded   load_seeded(scheme, party, mask_seed=, ...)          mkt_load_seeded_keys
  ksk      the same with the key-switching section alone        (196 KB of bodies up, the expansion kernel, a drain)
  brk      the same with the bootstrapping section alone
Every call returns after a device synchronise, so a host clock around it is the call's time.  The key-switching rate is the bytes of the
resident table (rows * n1p * 4) over the `ksk` call: a whole-call rate, a lower bound of the kernel's.  Prints one JSON line and writes it to
--out with the library's build id.  A measurement path: it fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mktfhe_amd as mk  # noqa: E402


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def measure(p, reps, device):
    party = p.nparty - 1
    crs = mk.CRS(p, 1) if p.multikey else None
    t0 = time.perf_counter()
    k = mk.party_keygen_seeded(crs, p, party=party, deterministic_seed=1)
    t_gen = time.perf_counter() - t0
    t0 = time.perf_counter()
    brk, ksk = mk.seeded_keys_expand(p, party, k.mask_seed, k.brk_seeded, k.ksk_seeded)
    t_exp = time.perf_counter() - t0
    sch = mk.Scheme(p, device=device)
    calls = {
        "full": lambda: sch.load_party(party, brk=brk, ksk=ksk),
        "seeded": lambda: mk.load_seeded(sch, party, mask_seed=k.mask_seed, brk_seeded=k.brk_seeded, ksk_seeded=k.ksk_seeded),
        "ksk": lambda: mk.load_seeded(sch, party, mask_seed=k.mask_seed, ksk_seeded=k.ksk_seeded),
        "brk": lambda: mk.load_seeded(sch, party, mask_seed=k.mask_seed, brk_seeded=k.brk_seeded),
        "full_ksk": lambda: sch.load_party(party, ksk=ksk),
        "full_brk": lambda: sch.load_party(party, brk=brk),
    }
    for fn in calls.values():
        fn()                                            # warm-up: code objects, first allocations
    ms = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():                  # alternating
            ms[name].append(timed(fn))
    assert np.array_equal(sch.get_ksk(party), ksk), "the seeded load does not leave the host-expanded key-switching key"
    sch.close()
    n1p = (p.n + 4) // 4 * 4
    table = ksk.shape[0] * n1p * 4
    med = {name: statistics.median(v) for name, v in ms.items()}
    return {
        "set": p.name, "party": party, "reps": reps,
        "compact_bytes": int(32 + k.brk_seeded.nbytes + k.ksk_seeded.nbytes), "full_bytes": int(brk.nbytes + ksk.nbytes),
        "host_keygen_seeded_s": round(t_gen, 3), "host_expand_s": round(t_exp, 3),
        "ms_median": {n: round(v, 3) for n, v in med.items()}, "ms_min": {n: round(min(v), 3) for n, v in ms.items()},
        "ms_max": {n: round(max(v), 3) for n, v in ms.items()},
        "ksk_table_bytes": int(table), "ksk_call_write_GBps": round(table / med["ksk"] / 1e6, 2),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="CGGIparam,KMS2party")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "a GPU is required: nothing here is measured on a CPU"
    res = {"tool": "seeded_keys_load", "build_id": mk.build_id(), "device": torch.cuda.get_device_name(a.device),
           "results": [measure(getattr(mk, s), a.reps, a.device) for s in a.sets.split(",")]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
