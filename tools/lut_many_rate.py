"""What nout functions of one input cost through the many-table bootstrap (lut_many_bootstrap) against nout single lookups
(lut_bootstrap), in the same process.  GPU only.

Procedure of DESIGN.md 1b: device tensors of B ciphertexts, per call kind 30 launches after 30 untimed, the kinds alternating twice;
times are the engine's own event spans (mkt_enable_timing: class 0 whole call, 1 blind rotation, 4 KMS phase 2, 2 key switch).  The
bootstrap is one rotation and one key switch over nout B rows that reads the B rotated accumulators in place, every row at its own
coefficient; the expectation for nout outputs is (t_rot + nout t_ks) / (t_rot + t_ks), t_rot and t_ks being THIS run's lut_bootstrap
spans.  No bootstrap runs the extraction kernel; it is a unit call (lut_extract), timed alone on device tensors with HIP events of the
same stream and reported as a separate figure (extract_alone_ms).  The library is the one MKT_LIB_PATH names: for a comparison with an
earlier commit run the tool once per library, one process at a time.

  python tools/lut_many_rate.py [--set KMS2party_N1024_l2] [--batch 1024] [--launches 30]  ->  one JSON line"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mktfhe_amd as mk  # noqa: E402
from adder_rate import setup  # noqa: E402


def timed(sch, call, launches):
    """-> ms per call of classes (whole, rotation incl. KMS phase 2, key switch): `launches` timed calls after as many untimed"""
    for _ in range(launches):
        call()
    sch.enable_timing(True)
    for _ in range(launches):
        call()
    ms = [sch.kernel_ms(c)[0] / launches for c in (0, 1, 4, 2)]
    sch.enable_timing(False)
    return np.array([ms[0], ms[1] + ms[2], ms[3]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="KMS2party_N1024_l2")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=30)
    a = ap.parse_args()
    import torch
    p = getattr(mk, a.set)
    keys, sch = setup(p, 5)
    B, rng = a.batch, np.random.default_rng(3)
    dev = lambda x: torch.from_numpy(x).cuda()                                  # noqa: E731
    signed = np.int64 if p.W == 64 else np.int32
    # any words are an input and any words a table: the kernels' work does not depend on them
    c = dev(rng.integers(0, 1 << 32, (B, p.lwe_len), dtype=np.uint64).astype(np.uint32).view(np.int32))
    U = dev(rng.integers(0, 1 << 63, (1, p.N), dtype=np.uint64).astype(p.ring_dtype).view(signed))
    outs = {o: torch.empty((B, o, p.lwe_len), dtype=torch.int32, device="cuda") for o in (1, 2, 4, 8)}
    kinds = {"lut_bootstrap": lambda: mk.lut_bootstrap(sch, U, c, out=outs[1][:, 0])}
    for o in (1, 2, 4, 8):
        kinds[f"many{o}"] = (lambda o: lambda: mk.lut_many_bootstrap(sch, U, c, o, out=outs[o]))(o)
    spans = {k: np.zeros(3) for k in kinds}
    for _ in range(2):
        for k, call in kinds.items():
            spans[k] += timed(sch, call, a.launches) / 2
    # the extraction alone (a unit call: no part of the bootstrap)
    acc = dev(rng.integers(0, 1 << 63, (B, p.k + 1, p.N), dtype=np.uint64).astype(p.ring_dtype).view(signed))
    extract = {}
    for o in (2, 4, 8):
        for _ in range(a.launches):
            mk.lut_extract(sch, acc, o)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            mk.lut_extract(sch, acc, o)
        e1.record()
        torch.cuda.synchronize()
        extract[o] = e0.elapsed_time(e1) / a.launches
    whole1, rot1, ks1 = spans["lut_bootstrap"]
    r = {"tool": "lut_many_rate", "set": p.name, "batch": B, "launches": a.launches, "build_id": mk.build_id(),
         "lut_bootstrap": {"ms_per_call": whole1, "rotation_ms": rot1, "keyswitch_ms": ks1}}
    for o in (1, 2, 4, 8):
        whole, rot, ks = spans[f"many{o}"]
        ex = extract.get(o, 0.0)
        r[f"nout{o}"] = {"ms_per_call": whole, "ms_per_output": whole / o, "rotation_ms": rot, "keyswitch_ms": ks, "extract_alone_ms": ex,
                         "ratio_to_one_lookup": whole / whole1, "expected_ratio": (rot1 + o * ks1) / (rot1 + ks1),
                         "ratio_to_nout_lookups": whole / (o * whole1)}
    sch.close()
    print(json.dumps(r))


if __name__ == "__main__":
    main()
