"""Shared test helpers: build the ORACLE scheme object from the product's client-side keys."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
import mktfhe_amd as mk  # noqa: E402


def ora_params(p: mk.Params):
    return O.OraParams(p.scheme, p.n, p.N, p.k, p.W, p.l_gsw, p.logB_gsw, p.l_lev, p.logB_lev,
                       p.l_uni, p.logB_uni, p.f, p.logD, p.blk_len, p.blk_d)


def keygen(p: mk.Params, seed=1):
    """-> (crs or None, [PartyKeys])"""
    if p.multikey:
        a = mk.CRS(p, seed)
        return a, [mk.party_keygen(a, p, deterministic_seed=seed, party=i) for i in range(p.k)]
    return None, [mk.PartyKeys(p, deterministic_seed=seed, party=0)]


def oracle_scheme(p: mk.Params, crs, keys):
    s = O.Scheme(ora_params(p))
    if crs is not None:
        s.set_crs(crs.astype(np.uint64))
    for i, k in enumerate(keys):
        s.set_brk(i, k.brk.astype(np.uint64))
        s.set_ksk(i, k.ksk)
        if p.multikey:
            s.set_pubkey(i, k.pubkey.astype(np.uint64))
        if p.scheme in (mk.KMS, mk.KMS_BLOCK):
            s.set_rlk(i, k.rlk_d.astype(np.uint64), k.rlk_f.astype(np.uint64))
    return s


def gpu_scheme(p: mk.Params, crs, keys, device=0, arith=0):
    if p.multikey:
        return mk.setup(p, keys=keys, a=crs, device=device, arith=arith)
    return mk.setup(p, keys=keys[0], device=device, arith=arith)[1]


def encrypt_bits(p: mk.Params, keys, bits, seed=100):
    """bit j is encrypted under party (j mod nparty) (lwe_ith_encrypt layout, scheme.jl:379-386)"""
    out = np.empty((len(bits), p.lwe_len), dtype=np.uint32)
    for j, b in enumerate(bits):
        i = j % p.nparty
        out[j] = mk.lwe_ith_encrypt(int(b), i, keys[i], p, deterministic_seed=seed + j)
    return out


GATE_FUNCS = {
    0: lambda x, y: ~(x & y), 1: lambda x, y: x & y, 2: lambda x, y: x | y,
    3: lambda x, y: x ^ y, 4: lambda x, y: ~(x ^ y), 5: lambda x, y: ~(x | y),
}


def bits_equal(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def edge_words(W, n, rng):
    m = (1 << W) - 1
    special = [0, 1, 2, m, m - 1, 1 << (W - 1), (1 << (W - 1)) - 1, (1 << (W - 1)) + 1, 1 << (W - 3), m - (1 << (W - 3)) + 1]
    v = rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + rng.integers(0, 2, n, dtype=np.uint64)
    v &= np.uint64(m)
    v[: len(special)] = np.array(special, dtype=np.uint64)
    # the same words in the UPPER half of the polynomial: coefficient i + M feeds the imaginary slot through
    # -signed(p[i + M]) (fft.jl:60), where typemin wraps to itself
    if n >= 4 * len(special):
        v[n // 2: n // 2 + len(special)] = np.array(special, dtype=np.uint64)
        v[n - len(special):] = np.array(special[::-1], dtype=np.uint64)
    return v


def mixed_party_check(p, keys, so, sg, rng, B=3):
    """Fresh encryptions populate one party's mask block and same-party gates keep it so (the other parties' rotations
    are all skips, bootstrapping.jl:413 / :261).  Here every ciphertext involves ALL k parties: NAND folds over one
    fresh encryption per party (as test/KMS.jl:29-34), then every stage and gate on those dense ciphertexts."""
    k = p.nparty
    bits = rng.integers(0, 2, 2 * B * k).astype(bool)
    c = encrypt_bits(p, keys, bits, seed=7700)                      # ciphertext j under party j mod k
    acc_g, acc_b = c[0::k].copy(), bits[0::k].copy()
    for i in range(1, k):
        nxt = c[i::k]
        ref = np.stack([so.gate(0, acc_g[j], nxt[j]) for j in range(2 * B)])
        acc_g = sg.gate(0, acc_g, nxt)
        assert np.array_equal(acc_g, ref), f"fold step {i}"
        acc_b = ~(acc_b & bits[i::k])
    assert (acc_g[:, :-1].reshape(2 * B, k, p.n) != 0).any(axis=2).all(), "every party block populated"
    x, y = acc_g[:B], acc_g[B:]
    lin = np.stack([O.gate_linear(0, x[j], y[j]) for j in range(B)])
    at_g, bt_g = sg.modswitch(lin)
    acc0 = np.stack([so.testvector(bt_g[j]) for j in range(B)])
    acc_o = np.stack([so.blindrotate(at_g[j], acc0[j]) for j in range(B)])
    assert np.array_equal(sg.blindrotate_(at_g, acc0.astype(p.ring_dtype).copy()).astype(np.uint64), acc_o), "blindrotate (mixed)"
    assert np.array_equal(sg.keyswitch(acc_o.astype(p.ring_dtype)), np.stack([so.keyswitch(acc_o[j]) for j in range(B)])), "keyswitch (mixed)"
    for op in range(6):
        out_g = sg.gate(op, x, y)
        assert np.array_equal(out_g, np.stack([so.gate(op, x[j], y[j]) for j in range(B)])), f"gate {op} (mixed)"
        if p.name not in NOISY:
            got = mk.lwe_decrypt(out_g, keys, p)
            assert np.array_equal(got, GATE_FUNCS[op](acc_b[:B], acc_b[B:])), f"decrypt {op} (mixed)"


# parameter sets whose own noise makes gates on many-party ciphertexts decrypt wrongly now and then (the oracle
# produces the identical words): bit parity is asserted for them, decryption is not
NOISY = {"CCS16party", "CCS8party", "CCS4party", "KMS8party"}


# ---- tests/golden/kat_tiny.npz (gen_kat.py): fixture with inputs AND expected outputs ----
def kat_cases():
    import types
    from golden.gen_kat import params_of
    g = np.load(os.path.join(ROOT, "tests", "golden", "kat_tiny.npz"))
    names = sorted({k.split("/")[0] for k in g.files})
    for name in names:
        d = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(name + "/")}
        p = params_of(d["params"], name="kat_" + name)
        keys = []
        for i in range(p.nparty):
            keys.append(types.SimpleNamespace(brk=d[f"brk{i}"], ksk=d[f"ksk{i}"], pubkey=d.get(f"pub{i}"),
                                              rlk_d=d.get(f"rlkd{i}"), rlk_f=d.get(f"rlkf{i}"), lwekey=d["lwekeys"][i]))
        yield name, p, d, keys


def kat_decrypt(p, d, ct):
    """scheme.jl:388-407 with the fixture's LWE secrets, in numpy"""
    ph = ct[..., -1].astype(np.uint64)
    for i in range(p.nparty):
        ph = ph + (ct[..., i * p.n:(i + 1) * p.n].astype(np.uint64) * d["lwekeys"][i].astype(np.uint64)).sum(-1)
    ph = ph & np.uint64(0xFFFFFFFF)
    if p.multikey:
        return ph < (1 << 31)
    return ((ph >> np.uint64(29)) + ((ph >> np.uint64(28)) & np.uint64(1))) == 1
