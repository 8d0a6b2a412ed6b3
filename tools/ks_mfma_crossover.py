"""Whole key switch (ks_digits_kernel, the sum kernel, ks_reduce_kernel) per batch under the process's MKT_KS_MFMA, on device tensors with hip
events: the measurement behind the launch rule of the matrix-core key switch (kernels.hip ks_plan) and profiles/ks_mfma_crossover.txt.
The switch is read once per process, so one run per setting; each writes its outputs so that the two can be compared word for word:

    MKT_KS_MFMA=0 python tools/ks_mfma_crossover.py KMS2party_N1024_l2 off OUTDIR
    MKT_KS_MFMA=1 python tools/ks_mfma_crossover.py KMS2party_N1024_l2 on OUTDIR
    python tools/ks_mfma_crossover.py --compare KMS2party_N1024_l2 OUTDIR
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

BATCHES = (1, 2, 4, 8, 16, 32, 64, 128, 256, 384, 512, 768, 1024, 2048, 4096)
KEEP = 1024          # outputs kept for the comparison up to this batch


def compare(pname, outdir):
    a, b = (np.load(os.path.join(outdir, f"ks_cross_{pname}_{t}.npz")) for t in ("off", "on"))
    bad = 0
    for k in a.files:
        same = np.array_equal(a[k], b[k])
        bad += not same
        print(pname, k, "equal" if same else "DIFFERENT", a[k].shape)
    return 1 if bad else 0


def main():
    if sys.argv[1] == "--compare":
        return compare(sys.argv[2], sys.argv[3])
    import torch
    import mktfhe_amd as mk
    from mktfhe_amd.lut import keyswitch_at
    pname, tag, outdir = sys.argv[1], sys.argv[2], sys.argv[3]
    p = getattr(mk, pname)
    if p.multikey:
        crs = mk.CRS(p, 1)
        s = mk.setup(p, keys=[mk.party_keygen(crs, p, party=i, secrets_only=True, deterministic_seed=1) for i in range(p.k)], a=crs, device=0)
    else:
        s = mk.setup(p, keys=mk.PartyKeys(p, secrets_only=True, deterministic_seed=1), device=0)[1]
    rng = np.random.default_rng(5)
    res = {"params": pname, "MKT_KS_MFMA": os.environ.get("MKT_KS_MFMA"), "planes": s.get_metric("ks_mfma_planes"), "rows": []}
    outs = {}
    for B in BATCHES:
        acc = rng.integers(0, 2**63, (B, 1 + p.k, p.N), dtype=np.uint64).astype(p.ring_dtype)
        t = torch.from_numpy(acc.view(np.int64 if p.W == 64 else np.int32)).cuda()
        out = keyswitch_at(s, t)                                   # no rows, no coefficients: the plain key switch, tensors in and out
        torch.cuda.synchronize()
        used = s.get_metric("ks_mfma_last")
        for _ in range(3):
            keyswitch_at(s, t)
        torch.cuda.synchronize()
        ts = []
        for _ in range(15):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); keyswitch_at(s, t); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        res["rows"].append({"B": B, "mfma": used, "min_ms": round(ts[0], 4), "median_ms": round(ts[len(ts) // 2], 4)})
        if B <= KEEP:
            outs[str(B)] = out.cpu().numpy().view(np.uint32)
        print(res["rows"][-1], flush=True)
    os.makedirs(outdir, exist_ok=True)
    np.savez(os.path.join(outdir, f"ks_cross_{pname}_{tag}.npz"), **outs)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
