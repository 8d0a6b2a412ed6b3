"""What seeded inputs cost on the device, against the upload they replace (mkt_seeded_expand_batch / mkt_seeded_encrypt_batch).
GPU only, one process.

Workload: device tensors at KMS2party (n = 560, rows of 1121 words), party 1, B = 65 536 rows.  Procedure of DESIGN.md 1e: 30 launches after
30 untimed, bracketed by HIP events on the context's stream (torch's current stream, which the context follows for GPU tensors), the kinds
alternating twice.  Timed: seeded_expand into a preallocated tensor; seeded_encrypt on the device (a call is more than its kernel: it
allocates, uploads and wipes the party's n key words and synchronises before it returns); a device-to-device copy of the expanded
batch's bytes -- the write-stream yardstick; a host-to-device upload of the expanded rows from pinned memory -- what the feature replaces.
Reported: ms per call, bytes of expanded rows per second for each, and the two ratios expand / copy and expand / upload (rates; above 1 =
expansion is faster).  The batch partly sits in the Infinity Cache, so the ratios are the finding, not the absolute rates.  The kernels
alone: rocprofv3 --kernel-trace --stats -- python tools/seeded_rate.py.

  python tools/seeded_rate.py [--set KMS2party] [--batch 65536] [--launches 30] [--out FILE]  ->  one JSON line"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _event_ms(torch, call, launches):
    for _ in range(launches):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="KMS2party")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "tools/seeded_rate.py measures on the GPU"
    import mktfhe_amd as mk
    p = getattr(mk, a.set)
    B, party = a.batch, p.nparty - 1
    crs = mk.CRS(p, 5) if p.multikey else None
    key = mk.PartyKeys(p, party=party, crs=crs, secrets_only=True, deterministic_seed=5)
    sch = mk.Scheme(p)                                           # no evaluation key: neither call needs one
    seed = bytes(range(32))
    mu = torch.from_numpy(np.random.default_rng(3).integers(0, 2**32, B, dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
    batch = mk.seeded_encrypt(mu, key, p, party, words=True, scheme=sch, mask_seed=seed, deterministic_seed=9)
    rows = torch.empty((B, p.lwe_len), dtype=torch.int32, device="cuda")
    mk.seeded_expand(batch, p, scheme=sch, out=rows)
    # the device words are the host's (checked once on the first 1000 rows, before anything is timed)
    host = mk.seeded_encrypt(mu[:1000].cpu().numpy().view(np.uint32), key, p, party, words=True, mask_seed=seed, deterministic_seed=9)
    assert np.array_equal(batch.body[:1000].cpu().numpy().view(np.uint32), host.body)
    assert np.array_equal(rows[:1000].cpu().numpy().view(np.uint32), mk.seeded_expand(host, p))
    row_bytes = B * p.lwe_len * 4
    dst = torch.empty_like(rows)
    pinned = rows.cpu().pin_memory()
    kinds = {
        "expand": lambda: mk.seeded_expand(batch, p, scheme=sch, out=rows),
        "encrypt": lambda: mk.seeded_encrypt(mu, key, p, party, words=True, scheme=sch, mask_seed=seed, deterministic_seed=9),
        "copy": lambda: dst.copy_(rows),
        "upload": lambda: dst.copy_(pinned, non_blocking=True),
    }
    runs = {k: [] for k in kinds}
    for _ in range(2):                                           # the kinds alternate
        for k, call in kinds.items():
            runs[k].append(_event_ms(torch, call, a.launches))
    ms = {k: float(np.mean(v)) for k, v in runs.items()}
    r = {"tool": "seeded_rate", "build_id": mk.build_id(), "device": torch.cuda.get_device_name(0), "set": a.set, "batch": B, "n": p.n,
         "lwe_len": p.lwe_len, "party": party, "launches": a.launches, "row_bytes": row_bytes, "mask_bytes": B * p.n * 4,
         "ms": ms, "ms_runs": runs, "row_bytes_per_s": {k: row_bytes / (v * 1e-3) for k, v in ms.items()},
         "encrypt_rows_per_s": B / (ms["encrypt"] * 1e-3),
         "expand_over_copy_rate": ms["copy"] / ms["expand"], "expand_over_upload_rate": ms["upload"] / ms["expand"]}
    sch.close()
    line = json.dumps(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
