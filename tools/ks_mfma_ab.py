"""The step-level rule of docs/history.md (2026-10-18) as a program: a parent build of the library (MKT_LIB_PATH) and this tree's alternated
round by round on the plain `python bench.py [--workload W]` command, one process at a time, every run's result line kept.

    python tools/ks_mfma_ab.py PARENT_LIB WORKLOAD ROUNDS OUT.json [DUMPDIR] [DEADLINE_S]

DUMPDIR: one more round at the end with --dump-outputs DUMPDIR/<parent|new> (marked "dumped", not one of the ROUNDS); their .npy files are
compared word for word.  DEADLINE_S: no new ROUND is started once that many seconds have passed since the program began (the record says how many ran)."""
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    parent, workload, rounds, out_path = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    dump = sys.argv[5] if len(sys.argv) > 5 and sys.argv[5] != "-" else None
    deadline = time.time() + (float(sys.argv[6]) if len(sys.argv) > 6 else 1e9)
    out = {"workload": workload, "command": "python bench.py" + ("" if workload == "kms2_n1024" else f" --workload {workload}"), "rounds_asked": rounds,
           "runs": {"parent": [], "new": []}}
    for tag in ("parent", "new"):      # which builds these are (csrc/Makefile BUILD_ID)
        env = dict(os.environ)
        env.pop("MKT_LIB_PATH", None)
        if tag == "parent":
            env["MKT_LIB_PATH"] = os.path.abspath(parent)
        out[f"{tag}_build_id"] = subprocess.run([sys.executable, "-c", "from mktfhe_amd import _lib; print(_lib.build_id())"], cwd=ROOT, env=env,
                                                capture_output=True, text=True, timeout=120).stdout.strip().splitlines()[-1]
    plan = [False] * rounds + ([True] if dump else [])
    for r, dumped in enumerate(plan):
        if not dumped and time.time() > deadline:
            continue
        for tag in ("parent", "new"):
            env = dict(os.environ)
            env.pop("MKT_LIB_PATH", None)
            if tag == "parent":
                env["MKT_LIB_PATH"] = os.path.abspath(parent)
            cmd = [sys.executable, "bench.py"] + ([] if workload == "kms2_n1024" else ["--workload", workload])
            if dumped:
                cmd += ["--dump-outputs", os.path.join(dump, tag)]
            t0 = time.time()
            p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
            if p.returncode != 0:
                print(tag, r, "rc", p.returncode, p.stdout[-2000:], p.stderr[-2000:])
                return p.returncode if p.returncode > 0 else 1
            line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            rec = {"round": r, "ms_per_step": round(line["ms_per_step"], 4), "kernels_ms_per_step": line.get("kernels_ms_per_step"),
                   "decrypt_ok": line.get("decrypt_ok"), "dumped": dumped}
            out["runs"][tag].append(rec)
            print(workload, r, tag, rec["ms_per_step"], rec["kernels_ms_per_step"], f"{time.time() - t0:.0f}s", flush=True)
            json.dump(out, open(out_path, "w"), indent=1)
    counted = {t: [x["ms_per_step"] for x in out["runs"][t] if not x["dumped"]] for t in ("parent", "new")}
    if counted["parent"] and counted["new"]:
        out["rounds_run"] = len(counted["new"])
        out["every_new_below_every_parent"] = max(counted["new"]) < min(counted["parent"])
    if dump:
        a, b = (sorted(glob.glob(os.path.join(dump, t, "*.npy"))) for t in ("parent", "new"))
        import numpy as np
        out["outputs_equal"] = bool(a) and len(a) == len(b) and all(np.array_equal(np.load(x), np.load(y)) for x, y in zip(a, b))
    json.dump(out, open(out_path, "w"), indent=1)
    print(workload, "rounds", out.get("rounds_run"), "every new below every parent:", out.get("every_new_below_every_parent"), "outputs equal:", out.get("outputs_equal"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
