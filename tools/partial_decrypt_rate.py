"""What a party's decryption shares cost on the device (mkt_partial_decrypt_batch).  GPU only, one process.

Workload: device tensors at KMS2party (n = 560, rows of 1121 words), B = 65 536 rows, party 1's shares at sigma_smudge = 2^20.  Procedure
of DESIGN.md 1b: 30 launches after 30 untimed, bracketed by HIP events on the context's stream (torch's current stream, which the
context follows for GPU tensors).  A call is more than its kernel: it allocates, uploads and wipes the party's n key words and
synchronises before it returns, and the events see all of that.  Reported: ms per call; bytes of the party's blocks (B n 4) read per second
of a call; in the same run the rate of a device-to-device copy of the same number of bytes (read + written = twice that many bytes moved),
as the yardstick; their ratio.  The kernel alone: rocprofv3 --kernel-trace --stats -- python tools/partial_decrypt_rate.py.

  python tools/partial_decrypt_rate.py [--set KMS2party] [--batch 65536] [--launches 30] [--out FILE]  ->  one JSON line"""
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
    assert torch.cuda.is_available(), "tools/partial_decrypt_rate.py measures on the GPU"
    import mktfhe_amd as mk
    p = getattr(mk, a.set)
    B, party, sigma = a.batch, p.nparty - 1, 2.0 ** 20
    crs = mk.CRS(p, 5) if p.multikey else None
    key = mk.PartyKeys(p, party=party, crs=crs, secrets_only=True, deterministic_seed=5)
    sch = mk.Scheme(p)                                           # a party's own context: no evaluation key
    rng = np.random.default_rng(3)
    ct = torch.from_numpy(rng.integers(0, 2**32, (B, p.lwe_len), dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
    # the device words are the host's (checked once on the first 1000 rows, before anything is timed)
    want = mk.partial_decrypt(ct[:1000].cpu().numpy().view(np.uint32), key, p, party, sigma, deterministic_seed=9)
    got = mk.partial_decrypt(ct, key, p, party, sigma, scheme=sch, deterministic_seed=9)
    assert np.array_equal(got[:1000].cpu().numpy().view(np.uint32), want)
    block_bytes = B * p.n * 4
    src = torch.empty(block_bytes // 4, dtype=torch.int32, device="cuda").random_()
    dst = torch.empty_like(src)
    ms, copy_ms = [], []
    for _ in range(2):                                           # the two kinds alternate
        ms.append(_event_ms(torch, lambda: mk.partial_decrypt(ct, key, p, party, sigma, scheme=sch, deterministic_seed=9), a.launches))
        copy_ms.append(_event_ms(torch, lambda: dst.copy_(src), a.launches))
    call_ms, cp_ms = float(np.mean(ms)), float(np.mean(copy_ms))
    r = {"tool": "partial_decrypt_rate", "build_id": mk.build_id(), "device": torch.cuda.get_device_name(0), "set": a.set, "batch": B, "n": p.n,
         "lwe_len": p.lwe_len, "party": party, "sigma_smudge": sigma, "launches": a.launches, "ms_per_call": call_ms, "ms_per_call_runs": ms,
         "block_bytes": block_bytes, "block_bytes_per_s": block_bytes / (call_ms * 1e-3),
         "copy_ms": cp_ms, "copy_ms_runs": copy_ms, "copy_bytes_per_s": block_bytes / (cp_ms * 1e-3), "call_over_copy_rate": cp_ms / call_ms}
    sch.close()
    line = json.dumps(r)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
