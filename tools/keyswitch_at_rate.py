"""What the key switch at a coefficient (mkt_keyswitch_at_batch) costs.  GPU only.  Two questions:

 (a) does the plain key switch pay for the feature?  mkt_keyswitch_batch of THIS library against the same call of the parent commit's
     library (--parent-lib: that commit built beside this one, e.g. make -C mktfhe_amd/csrc SFX=_parent in its checkout), same session,
     same device, one process at a time, the two libraries alternating (parent, this, parent, this).  The yardstick is the spread between
     the parent's own two repeats.
 (b) the fused path against the existing one, o = 4: keyswitch_at over 4 B rows reading B accumulators in place, against
     lut_extract (B -> 4 B copies) + keyswitch over the same 4 B rows.

Procedure of DESIGN.md 1b: device tensors at the headline set, B = 1024, per kind 30 launches after 30 untimed, the kinds alternating twice,
mkt_enable_timing spans (class 2, key switch); (b) also brackets each kind's 30 launches with HIP events of the stream, since the extraction
has no class of its own.

  python tools/keyswitch_at_rate.py [--parent-lib PATH] [--set KMS2party_N1024_l2] [--batch 1024] [--launches 30] [--out FILE]  ->  one JSON line"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_TIMEOUT = 240


def _load(older_ok):
    """the package on the library MKT_LIB_PATH names; older_ok: a library of an earlier commit lacks the newest symbols -- they are dropped
    from the ctypes table of THIS process (which then calls none of them) instead of failing the load"""
    import torch  # noqa: F401  (first: mktfhe_amd/_lib.py explains the order)
    from mktfhe_amd import _lib
    if older_ok:
        L = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.SYMBOLS if not hasattr(L, n)]:
            del _lib.SYMBOLS[name]
    import mktfhe_amd as mk
    return mk


def _setup(mk, a):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from adder_rate import setup
    p = getattr(mk, a.set)
    keys, sch = setup(p, 5)
    rng = np.random.default_rng(3)
    signed = np.int64 if p.W == 64 else np.int32
    # any words are an accumulator: the kernels' work does not depend on them
    acc = torch.from_numpy(rng.integers(0, 1 << 63, (a.batch, p.k + 1, p.N), dtype=np.uint64).astype(p.ring_dtype).view(signed)).cuda()
    return p, sch, acc, torch


def _spans(sch, torch, call, launches):
    """-> (ms per call of the key-switch class, ms per call between HIP events around the timed launches)"""
    for _ in range(launches):
        call()
    sch.enable_timing(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        call()
    e1.record()
    torch.cuda.synchronize()
    ks = sch.kernel_ms(2)[0] / launches
    sch.enable_timing(False)
    return ks, e0.elapsed_time(e1) / launches


def child_plain(a):
    mk = _load(older_ok=True)
    from mktfhe_amd.scheme import _Buf
    p, sch, acc, torch = _setup(mk, a)
    B = a.batch
    out = torch.empty((B, p.lwe_len), dtype=torch.int32, device="cuda")
    call = lambda: sch._call("keyswitch_batch", B, _Buf(acc, p.ring_dtype, B * (p.k + 1) * p.N), sch._ct(out, B, out=True))    # noqa: E731
    reps = [_spans(sch, torch, call, a.launches)[0] for _ in range(2)]
    r = {"build_id": mk.build_id(), "device": torch.cuda.get_device_name(0), "keyswitch_ms": reps}
    sch.close()
    print(json.dumps(r))


def child_fused(a):
    mk = _load(older_ok=False)
    from mktfhe_amd.scheme import _Buf
    p, sch, acc, torch = _setup(mk, a)
    B, o = a.batch, 4
    rows = B * o
    g = torch.arange(rows, dtype=torch.int32, device="cuda")
    src, coef = (g // o).contiguous(), (g % o).contiguous()
    out = torch.empty((rows, p.lwe_len), dtype=torch.int32, device="cuda")

    def fused():
        mk.keyswitch_at(sch, acc, src, coef)

    def copied():
        accs = mk.lut_extract(sch, acc, o)
        sch._call("keyswitch_batch", rows, _Buf(accs, p.ring_dtype, rows * (p.k + 1) * p.N), sch._ct(out, rows, out=True))

    # the two kinds give the same words (checked once, before anything is timed)
    copied()
    assert torch.equal(mk.keyswitch_at(sch, acc, src, coef), out)
    kinds = {"keyswitch_at": fused, "extract_then_keyswitch": copied}
    tot = {k: np.zeros(2) for k in kinds}
    for _ in range(2):
        for k, call in kinds.items():
            tot[k] += np.array(_spans(sch, torch, call, a.launches)) / 2
    r = {"build_id": mk.build_id(), "device": torch.cuda.get_device_name(0), "o": o, "rows": rows}
    for k in kinds:
        r[k] = {"keyswitch_class_ms": tot[k][0], "event_ms": tot[k][1]}
    r["ratio_event_ms"] = tot["keyswitch_at"][1] / tot["extract_then_keyswitch"][1]
    r["ratio_keyswitch_class_ms"] = tot["keyswitch_at"][0] / tot["extract_then_keyswitch"][0]
    sch.close()
    print(json.dumps(r))


def _run(kind, a, lib):
    """one child process with the GPU open, under its own time limit; a child that does not end well ends the tool"""
    env = dict(os.environ)
    env.pop("MKT_LIB_PATH", None)
    if lib:
        env["MKT_LIB_PATH"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--set", a.set, "--batch", str(a.batch), "--launches", str(a.launches)],
                       env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        sys.exit(f"child {kind} ({lib or 'this library'}): rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="KMS2party_N1024_l2")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["plain", "fused"])
    a = ap.parse_args()
    if a.child:
        return {"plain": child_plain, "fused": child_fused}[a.child](a)
    r = {"tool": "keyswitch_at_rate", "set": a.set, "batch": a.batch, "launches": a.launches}
    if a.parent_lib:
        order = [("parent", os.path.abspath(a.parent_lib)), ("this", None)] * 2
        runs = {"parent": [], "this": []}
        for who, lib in order:
            runs[who].append(_run("plain", a, lib))
        pm = [ms for x in runs["parent"] for ms in x["keyswitch_ms"]]
        tm = [ms for x in runs["this"] for ms in x["keyswitch_ms"]]
        r["plain_keyswitch"] = {"parent_build_id": runs["parent"][0]["build_id"], "build_id": runs["this"][0]["build_id"], "device": runs["this"][0]["device"],
                                "parent_ms": pm, "this_ms": tm, "parent_mean_ms": float(np.mean(pm)), "this_mean_ms": float(np.mean(tm)),
                                "parent_spread": (max(pm) - min(pm)) / float(np.mean(pm)), "this_over_parent": float(np.mean(tm) / np.mean(pm)),
                                "within_parent_spread": bool(min(pm) <= np.mean(tm) <= max(pm) or abs(np.mean(tm) / np.mean(pm) - 1) <= (max(pm) - min(pm)) / np.mean(pm))}
    else:
        r["plain_keyswitch"] = "not measured: no --parent-lib"
    r["fused_o4"] = _run("fused", a, None)
    r["build_id"] = r["fused_o4"]["build_id"]
    line = json.dumps(r)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
