#!/usr/bin/env python3
"""Cost of packing results (mkt_pack_batch) beside the cost of producing them, on the GPU, and the live pack noise.

For each parameter set, on one context with evaluation keys generated on the device and host-generated packing keys (gadget --gadget):
B = N and 8 N rows; alternating, after a warm-up of each, `reps` times:
  gate   mkt_gate_batch NAND of B row pairs                      the bootstraps that produce B results
  pack   mkt_pack_batch of those B rows                          ceil(B / N) packed ciphertexts
every call on device tensors between two device events; the medians are reported.  Beside them the transform counts the two are made of:
a pack runs nparty n (l_pk + 1 + kr) transforms, a bootstrap nparty n (kr + 1) (l_gsw + 1) (the blind rotation's CMux count; the KMS
schemes' second phase and every key switch are left out, so the estimate flatters the pack).
--noise: the three cases of tests/test_gpu_pack.py (measured / predicted deviation, derived bands), written beside the timings.
--keys: instead of the above, the cost of the packing KEY of one party (the last), alternating after one warm-up of each, `reps` times:
  keygen_host     mkt_client_packing_keygen (the host generator, up to 16 threads)          wall clock: host work
  keygen_device   mkt_packing_keygen_device (pack_keys.hip; secrets up, bodies down)        device events on the context's stream, and wall clock
  load_full       mkt_load_packing_key from a host array [n][l][1 + kr][N]                  device events, and wall clock
  load_seeded     mkt_load_packing_key_seeded from a host array [n][l][N]                   device events, and wall clock
on a context that holds no other key; medians with the spread (min, max).  Writes pack_keys_<build id>.json.
--shares: instead of the above, the ring share of one party (the last) at G = 1, 8, 64 packs, alternating after one warm-up of each, `reps` times:
  host     mkt_client_rlwe_partial_decrypt on host arrays (one thread, a loop over packs)            wall clock: host work
  device   mkt_rlwe_partial_decrypt_batch on device tensors (ring_share.hip; ring keys up, wiped)     wall clock, and device events
a sample is as many back-to-back calls as fill 20 ms; per-call medians with the spread.  Writes ring_share_<build id>.json.
Writes pack_<build id>.json (and pack_noise_<build id>.json) into --out-dir.  A measurement path: it fails without a GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mktfhe_amd as mk  # noqa: E402


def setup(p, seed):
    """secrets on the CPU, evaluation keys generated on the device"""
    if p.multikey:
        crs = mk.CRS(p, seed)
        keys = [mk.party_keygen(crs, p, party=i, secrets_only=True, deterministic_seed=seed + i) for i in range(p.k)]
        return keys, mk.setup(p, keys=keys, a=crs)
    k, sch = mk.setup(p, keys=mk.PartyKeys(p, party=0, secrets_only=True, deterministic_seed=seed))
    return [k], sch


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(p, l, logB, reps, torch):
    keys, sch = setup(p, 11)
    for i in range(p.nparty):
        mk.load_packing_key(sch, i, mk.packing_keygen(keys[i], p, l, logB, deterministic_seed=70 + i), l, logB)
    kr = 1 if p.multikey else p.k
    rot_kr = 1 if p.scheme in (mk.KMS, mk.KMS_BLOCK) else p.k
    l_rot = p.l_uni if p.scheme == mk.CCS else p.l_gsw
    t_pack, t_boot = p.nparty * p.n * (l + 1 + kr), p.nparty * p.n * (rot_kr + 1) * (l_rot + 1)
    rng = np.random.default_rng(5)
    out = {"set": p.name, "n": p.n, "N": p.N, "nparty": p.nparty, "W": p.W, "gadget": [l, logB], "reps": reps,
           "transforms_per_pack": t_pack, "transforms_per_bootstrap": t_boot, "batches": []}
    for B in (p.N, 8 * p.N):
        x = torch.from_numpy(rng.integers(0, 2**32, (B, p.lwe_len), dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
        y = torch.from_numpy(rng.integers(0, 2**32, (B, p.lwe_len), dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
        res = torch.empty_like(x)
        packed = mk.pack(sch, x)
        calls = {"gate": lambda: sch.gate(0, x, y, out=res), "pack": lambda: mk.pack(sch, res, out=packed)}
        for fn in calls.values():
            fn()                                        # warm-up: code objects, workspaces
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(reps):
            for k, fn in calls.items():                 # alternating
                ms[k].append(event_ms(torch, fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        packs = -(-B // p.N)
        out["batches"].append({
            "B": B, "packs": packs, "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
            "ms_max": {k: round(max(v), 4) for k, v in ms.items()}, "pack_over_gate": round(med["pack"] / med["gate"], 5),
            "transform_estimate_pack_over_gate": round(packs * t_pack / (B * t_boot), 5),
            "lwe_bytes": B * p.lwe_len * 4, "packed_bytes": packs * (p.k + 1) * p.N * p.W // 8})
    sch.close()
    return out


def measure_keys(p, l, logB, reps, torch):
    import time
    party = p.nparty - 1
    crs = mk.CRS(p, 11) if p.multikey else None
    key = mk.PartyKeys(p, party=party, crs=crs, secrets_only=True, deterministic_seed=11 + party)
    sch = mk.Scheme(p)
    st = torch.cuda.Stream()
    sch.set_stream(st.cuda_stream)                      # the events below are recorded on the stream the context enqueues on
    ms_seed, body = mk.packing_keygen_seeded(key, p, l, logB, deterministic_seed=70)
    full = mk.packing_key_expand(p, party, l, logB, ms_seed, body)
    calls = {"keygen_host": lambda: mk.packing_keygen(key, p, l, logB, deterministic_seed=70),
             "keygen_device": lambda: mk.packing_keygen_device(sch, party, key, l, logB, mask_seed=ms_seed, deterministic_seed=70),
             "load_full": lambda: mk.load_packing_key(sch, party, full, l, logB),
             "load_seeded": lambda: mk.load_packing_key_seeded(sch, party, ms_seed, body, l, logB)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    for fn in calls.values():
        fn()                                            # warm-up: code objects, the resident table
    ev, wall = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():                     # alternating
            a, b = timed(fn)
            ev[k].append(a)
            wall[k].append(b)
    sch.close()
    stat = lambda v: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}      # noqa: E731
    kr = 1 if p.multikey else p.k
    return {"set": p.name, "n": p.n, "N": p.N, "W": p.W, "kr": kr, "gadget": [l, logB], "party": party, "reps": reps,
            "full_bytes": int(full.nbytes), "seeded_bytes": int(body.nbytes) + 32, "host_threads": min(16, os.cpu_count() or 4),
            "device_event_ms": {k: stat(v) for k, v in ev.items() if k != "keygen_host"}, "wall_ms": {k: stat(v) for k, v in wall.items()}}


SHARE_PACKS = (1, 8, 64)
SHARE_WINDOW_MS = 20.0      # a sample times as many back-to-back calls as fill this window: one call is a sub-millisecond window


def measure_shares(p, reps, torch):
    """the ring share of the last party, G = 1, 8, 64 packs of uniform ring words: host (mkt_client_rlwe_partial_decrypt, host arrays) against
    device (mkt_rlwe_partial_decrypt_batch, device tensors in and out, on a context that holds no key).  Both calls return with their words
    written -- the device call drains its stream when it wipes the secrets -- so both are timed by the host clock; the device call also
    between two events on its stream"""
    import time
    party = p.nparty - 1
    crs = mk.CRS(p, 11) if p.multikey else None
    key = mk.PartyKeys(p, party=party, crs=crs, secrets_only=True, deterministic_seed=11 + party)
    sch = mk.Scheme(p)
    st = torch.cuda.Stream()
    sch.set_stream(st.cuda_stream)
    rng = np.random.default_rng(5)
    sigma, seed = 2.0 ** 20, bytes(range(32))
    stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}      # noqa: E731
    rows = []
    for G in SHARE_PACKS:
        ct = rng.integers(0, 2**63, (G, p.k + 1, p.N), dtype=np.uint64).astype(p.ring_dtype)
        dct = torch.from_numpy(ct.view(np.int64 if p.W == 64 else np.int32)).cuda()
        calls = {"host": lambda: mk.rlwe_partial_decrypt(ct, key, p, party, sigma, deterministic_seed=seed),
                 "device": lambda: mk.rlwe_partial_decrypt(dct, key, p, party, sigma, deterministic_seed=seed, scheme=sch)}

        def timed(fn, inner):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(st)
            for _ in range(inner):
                fn()
            e1.record(st)
            e1.synchronize()
            return (time.perf_counter() - t0) * 1e3 / inner, e0.elapsed_time(e1) / inner

        same = np.array_equal(calls["host"](), calls["device"]().cpu().numpy().view(p.ring_dtype))      # warm-up of each, and the words agree
        inner = {k: max(1, min(500, int(np.ceil(SHARE_WINDOW_MS / max(timed(fn, 3)[0], 1e-3))))) for k, fn in calls.items()}
        wall, ev = {k: [] for k in calls}, []
        for _ in range(reps):
            for k, fn in calls.items():                 # alternating
                w, e = timed(fn, inner[k])
                wall[k].append(w)
                if k == "device":
                    ev.append(e)
        rows.append({"G": G, "same_words": bool(same), "calls_per_sample": inner, "wall_ms_per_call": {k: stat(v) for k, v in wall.items()},
                     "device_event_ms_per_call": stat(ev), "host_over_device": round(statistics.median(wall["host"]) / statistics.median(wall["device"]), 3)})
    sch.close()
    return {"set": p.name, "N": p.N, "W": p.W, "k": p.k, "kr": 1 if p.multikey else p.k, "party": party, "reps": reps, "sigma_smudge": sigma, "packs": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="KMS2party_N1024_l2,KMS2party")
    ap.add_argument("--gadget", default="4,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--noise", action="store_true")
    ap.add_argument("--keys", action="store_true")
    ap.add_argument("--shares", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "a GPU is required: nothing here is measured on a CPU"
    l, logB = (int(v) for v in a.gadget.split(","))
    head = {"build_id": mk.build_id(), "device": torch.cuda.get_device_name(0)}
    if a.keys or a.shares:
        if a.keys:
            name, rec = "pack_keys", dict(head, tool="pack_time --keys", results=[measure_keys(getattr(mk, s), l, logB, a.reps, torch) for s in a.sets.split(",")])
        else:
            name, rec = "ring_share", dict(head, tool="pack_time --shares", results=[measure_shares(getattr(mk, s), a.reps, torch) for s in a.sets.split(",")])
        os.makedirs(a.out_dir, exist_ok=True)
        line = json.dumps(rec)
        print(line)
        with open(os.path.join(a.out_dir, f"{name}_{mk.build_id()}.json"), "w") as f:
            f.write(line + "\n")
        return
    res = dict(head, tool="pack_time", results=[measure(getattr(mk, s), l, logB, a.reps, torch) for s in a.sets.split(",")])
    files = {f"pack_{mk.build_id()}.json": res}
    if a.noise:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import test_gpu_pack as T
        files[f"pack_noise_{mk.build_id()}.json"] = dict(head, tool="pack_time --noise", cases=[T.measure_noise(c) for c in sorted(T.NOISE_CASES)])
    os.makedirs(a.out_dir, exist_ok=True)
    for name, rec in files.items():
        line = json.dumps(rec)
        print(line)
        with open(os.path.join(a.out_dir, name), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
