"""8-bit adders per second from two-input gates (circuit.ripple_adder: 37 bootstraps over 15 levels) and from three-input gates
(circuit.ripple_adder_fa: 16 bootstraps over 8 levels) through circuit.evaluate_on, in the same run; and the measured decrypt-failure
rates of random two-input and three-input gates (random codes and NOT flags, operands under different parties).  GPU only.

The operands of the rate measurement are GATE OUTPUTS, as a gate's operands are inside a circuit: the input noise a three-input gate
adds up (3 or 12 sigma^2) is the output noise of the gates before it, ~700x a fresh encryption's at the headline set.
Each operand is bench.py's `mixed` input: a NAND fold over k fresh encryptions, one per party (so every party's mask block is
populated and its rotation runs, as inside a multi-party circuit; a bootstrap of a one-party ciphertext skips the other parties'
rotations and carries less noise).  Every operand slot of every gate is its own ciphertext, so no two gates share a noise sample, and
a gate's expected bit is computed from its operands' DECRYPTED bits, so that a wrong operand fold is not counted against the gate.
The adders' inputs are fresh encryptions, one per (input, instance); their "output_bits_wrong" is a correctness count of the timed
evaluation, not a failure rate (the 16 gates of an adder are not independent samples).

  python tools/adder_rate.py [--set KMS2party_N1024_l2] [--instances 1024] [--gates 16384] [--steps 5] [--warmup 2]  ->  one JSON line"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mktfhe_amd as mk  # noqa: E402
from mktfhe_amd import circuit as CI  # noqa: E402


def setup(p, seed):
    """keys made on the CPU as secrets only; the evaluation keys are generated on the device"""
    if p.multikey:
        crs = mk.CRS(p, seed)
        keys = [mk.party_keygen(crs, p, party=i, secrets_only=True, deterministic_seed=seed + i) for i in range(p.k)]
        return keys, mk.setup(p, keys=keys, a=crs)
    k, sch = mk.setup(p, keys=mk.PartyKeys(p, party=0, secrets_only=True, deterministic_seed=seed))
    return [k], sch


def adder_rate(circ, p, keys, sch, inst, steps, warmup, torch):
    plan = CI.Plan(circ, inst)
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2, (circ.n_inputs, inst)).astype(bool)
    party = lambda i: (i // 8) % p.nparty                                     # noqa: E731  (inputs 0-7 = a, 8-15 = b)
    inputs = [torch.from_numpy(np.stack([mk.lwe_ith_encrypt(int(bits[i, j]), party(i), keys[party(i)], p, deterministic_seed=9000 + inst * i + j)
                                         for j in range(inst)]).view(np.int32)).cuda() for i in range(circ.n_inputs)]
    for _ in range(warmup):
        outs = CI.evaluate_on(circ, inputs, sch, plan)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        outs = CI.evaluate_on(circ, inputs, sch, plan)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    wrong = sum(int(np.count_nonzero(mk.lwe_decrypt(o.cpu().numpy().view(np.uint32), keys if p.multikey else keys[0], p) != w))
                for o, w in zip(outs, circ.plain(bits)))
    return {"adders_per_s": inst * steps / dt, "ms_per_evaluation": 1e3 * dt / steps, "bootstraps_per_adder": plan.gates // inst,
            "levels": len(plan.levels), "output_bits_wrong": wrong, "output_bits_checked": len(circ.outputs) * inst}


def operands(p, keys, sch, n, seed, torch):
    """n gate-output operands -> (their planned bits, device tensor [n][lwe_len]): for k parties a NAND fold over k fresh encryptions of
    random bits (party i for the i-th), for one party a fresh encryption bootstrapped once"""
    rng = np.random.default_rng(seed)
    k = p.nparty
    fb = rng.integers(0, 2, (k, n)).astype(bool)
    fresh = [torch.from_numpy(np.stack([mk.lwe_ith_encrypt(int(fb[i, j]), i, keys[i], p, deterministic_seed=seed + k * j + i) for j in range(n)]).view(np.int32)).cuda()
             for i in range(k)]
    if k == 1:
        sch.bootstrapping_(fresh[0])
        return fb[0], fresh[0]
    acc, ab = fresh[0], fb[0]
    for i in range(1, k):
        acc = mk.NAND(acc, fresh[i], sch)
        ab = ~(ab & fb[i])
    return ab, acc


def failure_rates(p, keys, sch, G, torch):
    """G random two-input and G random three-input gates (random codes and NOT flags); operand r of gate g is its own gate-output
    ciphertext (`operands`)"""
    rng = np.random.default_rng(11)
    kk = keys if p.multikey else keys[0]
    truth2 = np.array([[1, 1, 1, 0], [0, 0, 0, 1], [0, 1, 1, 1], [0, 1, 1, 0], [1, 0, 0, 1], [1, 0, 0, 0]], dtype=bool)   # NAND..NOR by 2x + y
    truth3 = np.array([[0, 0, 1, 1], [1, 1, 0, 0], [0, 1, 0, 1], [1, 0, 1, 0], [0, 1, 1, 0], [1, 0, 0, 1]], dtype=bool)   # MAJ3..AE3 by count
    dv = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()   # noqa: E731
    res = {}
    for arity in (2, 3):
        planned, pool = operands(p, keys, sch, arity * G, 1_000_000 * arity, torch)
        torch.cuda.synchronize()
        pbits = mk.lwe_decrypt(pool.cpu().numpy().view(np.uint32), kk, p).astype(bool)
        codes = rng.integers(0, 6, G) | (rng.integers(0, 1 << arity, G) << 3)
        ops = codes.astype(np.uint8)
        idx = [np.arange(r * G, (r + 1) * G, dtype=np.uint32) for r in range(arity)]
        v = [pbits[idx[r]] ^ ((codes & (8 << r)) > 0) for r in range(arity)]
        out = torch.empty((G, p.lwe_len), dtype=torch.int32, device="cuda")
        if arity == 2:
            sch.gate_gather(dv(ops), pool, dv(idx[0]), dv(idx[1]), out)
            want = truth2[codes & 7, 2 * v[0].astype(int) + v[1]]
        else:
            sch.gate3_gather(dv(ops), pool, dv(idx[0]), dv(idx[1]), dv(idx[2]), out)
            want = truth3[codes & 7, sum(x.astype(int) for x in v)]
        torch.cuda.synchronize()
        errs = int(np.count_nonzero(mk.lwe_decrypt(out.cpu().numpy().view(np.uint32), kk, p) != want))
        res[f"gate{arity}"] = {"gates": G, "operands": "gate outputs (NAND folds over one fresh encryption per party), one per operand slot",
                               "decrypt_errors": errs, "failure_rate": errs / G, "operand_gates_wrong": int(np.count_nonzero(pbits != planned))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="KMS2party_N1024_l2")
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--gates", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    p = getattr(mk, a.set)
    keys, sch = setup(p, 5)
    r = {"tool": "adder_rate", "set": p.name, "instances": a.instances, "build_id": mk.build_id(),
         "ripple_adder": adder_rate(CI.ripple_adder(8), p, keys, sch, a.instances, a.steps, a.warmup, torch),
         "ripple_adder_fa": adder_rate(CI.ripple_adder_fa(8), p, keys, sch, a.instances, a.steps, a.warmup, torch)}
    r["fa_speedup"] = r["ripple_adder_fa"]["adders_per_s"] / r["ripple_adder"]["adders_per_s"]
    r.update(failure_rates(p, keys, sch, a.gates, torch))
    sch.close()
    print(json.dumps(r))


if __name__ == "__main__":
    main()
