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


def party_set(n, nparty):
    """n words per party block, nparty blocks: CGGI for one block (a single-key scheme), KMS with k parties otherwise"""
    return mk.CGGIparam.scaled(n=n, N=256) if nparty == 1 else mk.KMS2party.scaled(n=n, N=256, k=nparty)


def secret_keys(p, seed=11):
    """-> [PartyKeys] holding the secrets only (no bootstrapping / key-switching key: for tests that evaluate nothing)"""
    crs = mk.CRS(p, seed) if p.multikey else None
    return [mk.PartyKeys(p, party=i, crs=crs, secrets_only=True, deterministic_seed=seed) for i in range(p.nparty)]


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def device_words(t):
    return t.cpu().numpy().view(np.uint32)


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


# ---- boundary inputs of the rotation / key-switch kernels' own rounding steps (tests/test_edges_cpu.py, tests/test_gpu_edges.py) ----
BT_TARGETS = ("0", "1", "N-1", "N", "N+1", "2N-1", "2N")


def _nu(nout):
    assert nout in (1, 2, 4, 8)
    return nout.bit_length() - 1


def modswitch_words(N, nout=1):
    """name -> 32-bit word at a boundary of divbits(w, 32 - logN - 1) (bootstrapping.jl:8-9, arithmetic.jl:23-27).  nout = 2^nu > 1: of the
    coarse switch sw_nu(w) = divbits(w, 32 - logN - 1 + nu) << nu (tests/ref_lut_many.py): read 1, N-1, N+1, 2N-1 in the names as nout,
    N - nout, N + nout, 2N - nout"""
    s = 32 - (N.bit_length() - 1) - 1 + _nu(nout)
    h = 1 << (s - 1)
    return {"zero": 0, "max->0": h - 1, "tie->1": h, "->N-1": 2**31 - h - 1, "tie->N": 2**31 - h, "->N": 2**31, "max->N": 2**31 + h - 1,
            "tie->N+1": 2**31 + h, "->2N-1": 2**32 - h - 1, "min->2N": 2**32 - h, "ones->2N": 2**32 - 1}


def bt_values(N, nout=1):
    """BT_TARGETS name -> the switched value: 0, nout, N - nout, N, N + nout, 2N - nout, 2N"""
    return {"0": 0, "1": nout, "N-1": N - nout, "N": N, "N+1": N + nout, "2N-1": 2 * N - nout, "2N": 2 * N}


def btilde_words(N, nout=1):
    """BT_TARGETS name -> (smallest, largest) 32-bit word that the mod switch (nout > 1: the coarse switch sw_nu) rounds to it"""
    s = 32 - (N.bit_length() - 1) - 1 + _nu(nout)
    T, h = 1 << s, 1 << (s - 1)
    return {k: (max(v // nout * T - h, 0), min(v // nout * T + h - 1, 2**32 - 1)) for k, v in bt_values(N, nout).items()}


def lwe_edge_rows(p, rng, even=False, nout=1):
    """LWE rows (not encryptions) on the boundaries of the mod switch -> (rows uint32 [R][lwe_len], kinds [R]).
    kinds: "zero" mask of zero words; "skip" every mask word non-zero but rounding to 0; "dense" random words with the boundary words
    at the first / last position and on both sides of every block and party border; "blocks" whole blocks (block length, or single
    words) of non-zero words that round to 0 next to blocks of boundary words that do not; "party" (multi-key) one party's block all
    rounding to 0, the others dense.  Every kind meets every btilde of BT_TARGETS, through the smallest or the largest word that
    rounds to it.  even: bit 0 of every word cleared -- the words a XOR / XNOR linear part 2 (x + y) can take (gate.jl:28-44).
    nout = 2, 4, 8: the same rows on the boundaries of the coarse switch sw_nu of the many-table bootstrap (tests/ref_lut_many.py), the
    btilde targets 0, nout, N - nout, N, N + nout, 2N - nout, 2N."""
    N, n, nm = p.N, p.n, p.lwe_len - 1
    s = 32 - (N.bit_length() - 1) - 1 + _nu(nout)
    h = 1 << (s - 1)
    mw = modswitch_words(N, nout)
    live = [v for k, v in mw.items() if k not in ("zero", "max->0")]           # boundary words that do not round to 0
    L = p.blk_len if p.blk_len > 1 else 1
    borders = {0, nm - 1} | {b for i in range(1, p.nparty) for b in (i * n - 1, i * n)}
    if L > 1:
        borders |= {b for i in range(1, nm // L) for b in (i * L - 1, i * L)}
    borders = sorted(borders)
    skipw = lambda m: rng.integers(2, h, m, dtype=np.uint64).astype(np.uint32)      # noqa: E731  (non-zero also after bit 0 is cleared)
    rows, kinds = [], []
    kindlist = ["zero", "skip", "dense", "blocks"] + (["party"] if p.multikey else [])
    r = 0
    for kind in kindlist:
        for ti, t in enumerate(BT_TARGETS):
            row = np.zeros(p.lwe_len, dtype=np.uint32)
            if kind == "skip":
                row[:nm] = skipw(nm)
                row[0], row[nm - 1] = mw["max->0"], 1 if not even else 2
            elif kind in ("dense", "party"):
                row[:nm] = rng.integers(0, 2**32, nm, dtype=np.uint64).astype(np.uint32)
                for i, b in enumerate(borders):
                    row[b] = live[(i + r) % len(live)]
                if kind == "party":
                    pi = ti % p.nparty
                    row[pi * n:(pi + 1) * n] = skipw(n)
            elif kind == "blocks":
                for b0 in range(0, nm, L):
                    blk = (b0 // L + ti) % 2
                    row[b0:b0 + L] = skipw(min(L, nm - b0)) if blk else [live[(b0 + j + r) % len(live)] for j in range(min(L, nm - b0))]
            lo, hi = btilde_words(N, nout)[t]
            row[nm] = hi if (ti + len(rows)) % 2 else lo
            rows.append(row)
            kinds.append(kind)
            r += 1
    rows = np.stack(rows)
    if even:
        rows &= np.uint32(0xFFFFFFFE)
    return rows, kinds


def gadget_words(l, logB, W):
    """name -> W-bit word on a boundary of the balanced decomposition with l digits of logB bits (gsw.jl:42-52): the digits are the
    logB-bit fields of divbits(x, W - l logB) + sum_j B/2 B^j, each minus B/2; the top field drops its carry"""
    Lb, bit, m = l * logB, W - l * logB, (1 << W) - 1
    off = sum((1 << (logB - 1)) << (logB * j) for j in range(l))
    out = {"all-min": ((1 << Lb) - off) << bit,                 # prepared value 2^Lb: the smallest that carries out of the field; all digits -B/2
           "all-max": ((1 << Lb) - 1 - off) << bit,             # prepared value 2^Lb - 1: all digits B/2 - 1
           "top-min": (1 << (Lb - 1)) << bit}                   # 2^(W-1): top digit -B/2 (the word that is its own negative)
    if bit >= 1:
        hb = 1 << (bit - 1)
        out.update({"tie": (0x5 << bit | hb) & m, "tie-1": (0x5 << bit | hb) - 1 & m,
                    "round-carry": (1 << W) - hb,               # the smallest word that rounds to 2^Lb: every digit 0
                    "round-carry-1": (1 << W) - hb - 1,         # one below: rounds to 2^Lb - 1, the lowest digit -1, the others 0
                    "tie->all-min": ((((1 << Lb) - off - 1) << bit) | hb) & m})    # a tie that rounds up INTO the carry of the prepared value
    if bit >= 2:
        out["tie+1"] = ((0x5 << bit | (1 << (bit - 1))) + 1) & m
    if W == 64:                                                 # the same high parts over a low half of all ones / only the top bit
        for k, v in list(out.items()):
            out[k + "|lowFF"] = (v & ~0xFFFFFFFF) | 0xFFFFFFFF
            out[k + "|low80"] = (v & ~0xFFFFFFFF) | 0x80000000
    return out


def rot_gadgets(p):
    """the (l, logB) gadgets a blind rotation applies to its accumulator: GSW (CGGI, LMSS, KMS phase 1), LEV and UniEnc (KMS phase 2),
    UniEnc (CCS)"""
    if p.scheme == mk.CCS:
        return [(p.l_uni, p.logB_uni)]
    if p.scheme in (mk.KMS, mk.KMS_BLOCK):
        return [(p.l_gsw, p.logB_gsw), (p.l_lev, p.logB_lev), (p.l_uni, p.logB_uni)]
    return [(p.l_gsw, p.logB_gsw)]


def edge_positions(N):
    """0, M - 1, M, N - 1 first (index i and i + M feed the real and imaginary slot of one transform point), then pairs (i, i + M)"""
    M = N // 2
    pos = [0, M - 1, M, N - 1]
    for i in range(1, M - 1):
        pos += [i, i + M]
    return pos


def acc_edge(p, gadgets, rng, B):
    """accumulators [B][1 + k][N] (uint64 holding W-bit words) with EVERY polynomial populated: edge_words, and on top the
    gadget_words of every gadget in `gadgets` at the first edge_positions, the list rotated from polynomial to polynomial (what that
    reaches -- every class in both halves, a boundary word at each of 0, M - 1, M, N - 1 -- is asserted in tests/test_edges_cpu.py).
    A lone gadget that drops no bit (W = l logB: CCS4party) has three words only, which the rotation below does not move: they are laid
    down four times over, so that each still meets both halves and the four corner positions hold one"""
    N, W = p.N, p.W
    S = [v for (l, logB) in gadgets for v in gadget_words(l, logB, W).values()]
    pos = edge_positions(N)
    m = min(len(S) * (4 if len(S) < 4 else 1), len(pos), N // 2)
    acc = np.empty((B, 1 + p.k, N), dtype=np.uint64)
    for b in range(B):
        for q in range(1 + p.k):
            acc[b, q] = edge_words(W, N, rng)
            rot = (b * (1 + p.k) + q) * 3
            for i in range(m):
                acc[b, q, pos[i]] = S[(i + rot) % len(S)]
    return acc


def single_exponent_rows(p):
    """rows of switched exponents with exactly ONE non-zero entry: at the first / last mask position and on both sides of the first block
    and party border, each with every value of {1, N-1, N, N+1, 2N-1, 2N} (one CMux: a mismatch points at a digit); one more row makes
    the batch odd"""
    N, nm = p.N, p.lwe_len - 1
    L = p.blk_len if p.blk_len > 1 else 1
    pos = sorted({0, nm - 1, L - 1, min(L, nm - 1)} | ({p.n - 1, p.n} if p.nparty > 1 else set()))
    vals = (1, N - 1, N, N + 1, 2 * N - 1, 2 * N)
    at = np.zeros((len(pos) * len(vals) + 1, nm), dtype=np.uint32)
    for i, q in enumerate(pos):
        for j, v in enumerate(vals):
            at[i * len(vals) + j, q] = v
    at[-1, nm // 2] = N + 1
    return at


def dense_exponents(p, rng, B):
    at = rng.integers(0, 2 * p.N + 1, (B, p.lwe_len - 1)).astype(np.uint32)
    at[0, :3] = [0, 2 * p.N, p.N]
    return at


def rot_inputs(p, B, seed):
    """the crafted inputs of a blind rotation: the single-exponent rows, then one dense batch of B, each with accumulators on the gadgets' digit
    boundaries and a non-zero acc.a on entry -> (atilde [R][lwe_len - 1], acc [R][1 + k][N] uint64) twice"""
    rng = np.random.default_rng(seed)
    for at in (single_exponent_rows(p), dense_exponents(p, rng, B)):
        acc = acc_edge(p, rot_gadgets(p), rng, len(at))
        assert (acc[:, 1:].reshape(len(at), -1) != 0).any(axis=1).all()                  # acc.a is not zero on entry
        yield at, acc


def ks_words(f, logD):
    """name -> 32-bit extracted word on a boundary of the key switch's digits (unbalanced: the fields of divbits(w, 32 - f logD),
    gsw.jl:34-40; balanced: gadget_words)"""
    Lb, bit = f * logD, 32 - f * logD
    out = {"zero": 0, "0x80000000": 1 << 31, "all-D-1": ((1 << Lb) - 1) << bit, "one": 1, "ones": 2**32 - 1}
    if bit >= 1:
        hb = 1 << (bit - 1)
        out.update({"u-carry": 2**32 - hb,                      # rounds to 2^Lb: the carry leaves the field, every digit 0, like the zero word
                    "u-carry-1": 2**32 - hb - 1,                # every digit D - 1
                    "u-tie": (0x9 << bit) | hb, "u-tie-1": ((0x9 << bit) | hb) - 1})
    out.update({"b-" + k: v for k, v in gadget_words(f, logD, 32).items()})
    return out


def ks_border(p, c):
    """first switched coefficient of component c: below it the block schemes copy the extracted word (bootstrapping.jl:179-204, :676-690)"""
    if p.scheme == mk.LMSS:
        cur = c * p.N
        return 0 if cur >= p.n else min(p.N, p.n - cur)
    return p.n if p.scheme == mk.KMS_BLOCK else 0


def ks_positions(p, c):
    js = border = ks_border(p, c)
    return sorted({j for j in (0, 1, p.N - 1, p.N // 2, border - 1, border, js + 1) if 0 <= j < p.N})


def extract_words(p, poly):
    """the N extracted LWE words of an accumulator mask polynomial: c_0 = a[0], c_j = -a[N - j], after the truncation of a 64-bit
    word to its high half (bootstrapping.jl:91, :99, :575, :583)"""
    a = (np.asarray(poly, dtype=np.uint64) >> np.uint64(p.W - 32)).astype(np.uint32)
    out = (0 - a[::-1]).astype(np.uint32)
    return np.concatenate([a[:1], out[:-1]])


KS_LOW_HALVES = (0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0, 1)          # of a crafted 64-bit accumulator word (ks_edge_acc)
KS_BORROW_WORDS = ("u-tie", "u-tie-1", "u-carry", "u-carry-1", "b-tie", "b-tie-1")


def ks_edge_acc(p, rng, B):
    """accumulators [B][1 + k][N] whose EXTRACTED words sit on the key-switch gadget's boundaries: in every ciphertext and component
    the ks_words at ks_positions (j = 0 is not negated, j = N - 1 reads a[1]; both sides of the copied / switched border), rotated
    from ciphertext to ciphertext, and the whole list from the first switched coefficient on.  64-bit ring: the low half of those
    words is all ones, the top bit alone or all ones below it -- it is cut off, never rounded into the word -- and, in the list, also 0 and 1:
    where X^v wraps such a word (ks_edge_acc_at) its 64-bit negation borrows from the high half, or does not"""
    N, W, sh = p.N, p.W, p.W - 32
    S = list(ks_words(p.f, p.logD).values())
    acc = rng.integers(0, 2**63, (B, 1 + p.k, N), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (B, 1 + p.k, N), dtype=np.uint64)
    acc &= np.uint64((1 << W) - 1)

    def put(b, c, j, w, t, lows=KS_LOW_HALVES[:3]):
        v = (w if j == 0 else (-w) & 0xFFFFFFFF) << sh
        if sh:
            v |= lows[t % len(lows)]
        acc[b, 1 + c, 0 if j == 0 else N - j] = v

    for b in range(B):
        acc[b, 0, 0] = (S[b % len(S)] << sh) | ((0xFFFFFFFF, 0x80000000)[b % 2] if sh else 0)
        for c in range(p.k):
            j0 = ks_border(p, c)
            if j0 < N:
                for i, w in enumerate(S):
                    j = j0 + 2 + i
                    if j < N - 1:
                        put(b, c, j, S[(i + b) % len(S)], i + b, KS_LOW_HALVES)
            for i, j in enumerate(ks_positions(p, c)):
                put(b, c, j, S[(i + b + c) % len(S)], i + b)
    return acc


def ks_borrow_decides(p, c, j, word64):
    """64-bit ring: does moving the negation of accumulator word a[N - j] (j >= 1) across the truncation change an output word?  The
    extracted word is w = -trunc(a); trunc(-a) is w - 1 where a's low half is not 0.  A copied word (j below the border) IS an output;
    a switched one changes the output where w and w - 1 differ in a digit (w a tie or a carry: w - 1 is the word one below)"""
    if not int(word64) & 0xFFFFFFFF:
        return False
    if j < ks_border(p, c):
        return True
    w = (-(int(word64) >> 32)) & 0xFFFFFFFF
    if p.scheme in (mk.LMSS, mk.KMS_BLOCK):
        return list(O.decomp_word(w, p.f, p.logD, 32)) != list(O.decomp_word((w - 1) & 0xFFFFFFFF, p.f, p.logD, 32))
    return list(O.unbalanced_decomp_word(w, p.f, p.logD, 32)) != list(O.unbalanced_decomp_word((w - 1) & 0xFFFFFFFF, p.f, p.logD, 32))


def ks_edge_acc_at(p, rng, B, v):
    """X^v * ks_edge_acc(p, rng, B) on W-bit words: out[i] = a[i - v] for i >= v, -a[N + i - v] mod 2^W otherwise, so that the extraction
    at coefficient v (ref_lut_many.extract(out, v, W)) is the v = 0 accumulator exactly and every class of ks_edge_acc carries over.
    64-bit ring: the wrapped words (extracted coefficients 1 <= j <= v) were negated at 64 bits, and the key switch truncates and negates
    them at 32 bits: its word is trunc(out[v - j]) + (low half != 0).  That + 1 decides a digit only where the truncated word sits one
    below a tie or a carry, so on each side of j = v (wrapped: 1 <= j <= v, not wrapped: j > v) every ciphertext gets the ks_words
    u-tie, u-carry, b-tie and the words one below them over a non-zero low half: the list words of those classes that lie there
    are given one, and the same words are placed at the free positions next to j = v (at position v or v + 1 itself where a side holds
    nothing else)"""
    N, W, sh = p.N, p.W, p.W - 32
    a = ks_edge_acc(p, rng, B)
    if sh and p.f * p.logD < 32:
        kw = ks_words(p.f, p.logD)
        D = [kw[k] for k in KS_BORROW_WORDS]
        lows = [h for h in KS_LOW_HALVES if h]
        for b in range(B):
            for c in range(p.k):
                j0 = ks_border(p, c)
                taken = set(ks_positions(p, c)) | set(range(j0 + 2, j0 + 2 + len(kw)))
                for side in (range(v, 0, -1), range(v + 1, N)):
                    if not len(side):
                        continue
                    for j in side:                                  # list words of these classes: a low half that borrows
                        x = int(a[b, 1 + c, N - j])
                        if (-(x >> 32)) & 0xFFFFFFFF in D and not x & 0xFFFFFFFF:
                            a[b, 1 + c, N - j] = x | lows[(j + b) % len(lows)]
                    free = [j for j in side if j not in taken and j >= j0][:len(D)] or [j for j in side if j not in taken][:len(D)] or [side[0]]
                    for i, j in enumerate(free):                    # (a single position: a tie or a carry itself, never the word one below)
                        w = D[(i + b) % len(D)] if len(free) > 1 else D[2 * (b % 3)]
                        a[b, 1 + c, N - j] = (((-w) & 0xFFFFFFFF) << 32) | lows[(i + b + c) % len(lows)]
    m = np.uint64((1 << W) - 1)
    out = np.roll(a, v, axis=-1)
    if v:
        out[..., :v] = (np.uint64(0) - out[..., :v]) & m
    return out


def lut_edge_tables(p, o, nluts=2, seed=0):
    """lookup tables (nluts, N) ring words on the digit boundaries of the gadget that decomposes them in the first CMux (rot_gadgets(p)[0];
    the constant test vector +-2^(W-3) reaches none): its gadget_words and their negatives (the table step negates the wrapped part and,
    above N, the rest) at edge_positions(N) -- the four corners 0, M - 1, M, N - 1, then the whole list twice at the pairs (i, i + M) --
    with helpers.edge_words elsewhere, the list rotated from row to row.  o > 1: each row is the PACKED table of o tables T_v (mk.lut_pack:
    U[o i + v] = T_v[o i]) chosen so that the packed row is the one described"""
    N, W = p.N, p.W
    l, logB = rot_gadgets(p)[0]
    rng = np.random.default_rng([seed, N, W, o, l, logB])
    S = list(gadget_words(l, logB, W).values())
    S += [(-w) & ((1 << W) - 1) for w in S]
    pos = edge_positions(N)
    assert 4 + 4 * len(S) <= len(pos), "the list fits twice"
    rows = []
    for r in range(nluts):
        U = edge_words(W, N, rng)
        for i in range(4 + 4 * len(S)):
            U[pos[i]] = S[(5 * r + (i if i < 4 else (i - 4) // 2)) % len(S)]
        if o > 1:
            T = np.stack([edge_words(W, N, rng) for _ in range(o)])
            for t in range(o):
                T[t, ::o] = U[t::o]
            packed = mk.lut_pack(T.astype(p.ring_dtype), p)
            assert np.array_equal(packed.astype(np.uint64), U)
            rows.append(packed)
        else:
            rows.append(U.astype(p.ring_dtype))
    return np.stack(rows)


_GATE_CONST = {0: 1 << 29, 1: 7 << 29, 2: 1 << 29, 3: 1 << 30, 4: 3 << 30, 5: 7 << 29}


def gate_input(op, rows):
    """x with gate_linear(op, x, 0-row) == rows[j] (gate.jl:1-53 solved for x); XOR / XNOR: rows of even words only (their linear part
    is 2 (x + y) plus a constant), the halved word"""
    r = rows.astype(np.int64)
    c = np.zeros_like(r)
    c[..., -1] = _GATE_CONST[op]
    x = {0: c - r, 1: r - c, 2: r - c, 3: (r - c) // 2, 4: (c - r) // 2, 5: c - r}[op]
    return (x & 0xFFFFFFFF).astype(np.uint32)


def ks_edge_check(p, so, sg, rng, batches, after=None):
    """sg.keyswitch(ks_edge_acc) == the oracle's keyswitch! for EVERY ciphertext of every batch size -> number of ciphertexts compared.
    after(B): called behind each key switch (the switch children read which kernel it ran)"""
    checks = 0
    for B in batches:
        acc = ks_edge_acc(p, rng, B)
        out = sg.keyswitch(acc.astype(p.ring_dtype))
        if after:
            after(B)
        for j in range(B):
            assert np.array_equal(out[j], so.keyswitch(acc[j])), ("keyswitch (edge words)", p.name, p.n, p.f, p.logD, B, j)
            checks += 1
    return checks


def ks_at_rows(p, rng, B, coefs):
    """-> (src, coef) of B output rows over B accumulators: src unsorted with one repeat, coef cycling through coefs"""
    src = rng.permutation(B).astype(np.uint32)
    if B >= 3:
        src[-1] = src[0]
    return src, np.array([coefs[(g + 1) % len(coefs)] for g in range(B)], dtype=np.uint32)


def ks_at_edge_check(p, so, sg, rng, batches, coefs, device=True):
    """mk.keyswitch_at(sg, ks_edge_acc_at(v), src, coef) == the oracle's keyswitch! of the numpy extraction (ref_lut_many.extract) for
    EVERY row, for every v of coefs and every batch size: coef cycling through coefs (one call mixes coefficients) and coef = v throughout
    (every row on the crafted boundaries), in host and in device memory -> number of ciphertexts compared (each in both memories)"""
    import ref_lut_many as RM
    checks = 0
    for v in coefs:
        for B in batches:
            acc = ks_edge_acc_at(p, rng, B, v)
            a = acc.astype(p.ring_dtype)
            src, cyc = ks_at_rows(p, rng, B, coefs)
            for coef in (cyc, np.full(B, v, dtype=np.uint32)):
                want = np.stack([so.keyswitch(RM.extract(acc[int(src[g])], int(coef[g]), p.W)) for g in range(B)])
                got = mk.keyswitch_at(sg, a, src, coef)
                bad = np.nonzero((got != want).any(axis=1))[0]
                assert not len(bad), ("keyswitch_at (edge words), host memory", p.name, p.n, p.f, p.logD, v, B, bad[:4], src[bad[:4]], coef[bad[:4]])
                if device:
                    import torch
                    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view({4: np.int32, 8: np.int64}[x.dtype.itemsize])).cuda()      # noqa: E731
                    got = mk.keyswitch_at(sg, t(a), t(src), t(coef)).cpu().numpy().view(np.uint32)
                    bad = np.nonzero((got != want).any(axis=1))[0]
                    assert not len(bad), ("keyswitch_at (edge words), device memory", p.name, p.n, p.f, p.logD, v, B, bad[:4])
                checks += B
    return checks


# ---- which key-switch kernel a set and a setting of the launcher switches imply: the rule of kernels.hip ks_plan RESTATED (never read from
# the library), for tests/test_ks_plan_cpu.py and for the switch children, which report what ran (mkt_get_metric "ks_last_kernel" ...)
KS_PER_DIGIT, KS_PAIR, KS_MFMA = 1, 2, 3
KS_SWITCH_DEFAULTS = {"MKT_KS_G": 32, "MKT_KS_WAVES": 0, "MKT_KS_BLOCKS": 0, "MKT_KS_PAIR": -1, "MKT_KS_MFMA": -1}      # an unset variable reads as


def ks_switch_values(setting):
    """{variable: text} -> (MKT_KS_G, MKT_KS_WAVES, MKT_KS_BLOCKS, MKT_KS_PAIR, MKT_KS_MFMA) as the launcher reads them"""
    assert set(setting) <= set(KS_SWITCH_DEFAULTS), setting
    return tuple(int(setting.get(k, d)) for k, d in KS_SWITCH_DEFAULTS.items())


def ks_set_ints(p, mfma=-1, scratch=1):
    """-> [N, f, logD, rows per digit, n1p, kacc, mk, balanced, planes present, scratch present] of a parameter set on a context created under
    MKT_KS_MFMA = mfma: the byte planes are kept where the matrix-core kernel can serve (unbalanced D = 4, no 32-bit sum able to overflow)"""
    block = p.scheme in (mk.LMSS, mk.KMS_BLOCK)
    D = 1 << p.logD
    planes = mfma != 0 and p.logD == 2 and not block and p.N * (1 if p.multikey else p.k) * p.f * 255 < 2**31
    return [p.N, p.f, p.logD, D // 2 if block else D - 1, 4 * ((p.n + 1 + 3) // 4), p.k, int(p.multikey), int(block), int(planes), scratch]


def ks_kernel_rule(ints, sw):
    """(the ten values of ks_set_ints, the five of ks_switch_values) -> (kernel, tile width G, waves per workgroup).  The matrix cores are
    asked first: where they serve, MKT_KS_G / _WAVES / _BLOCKS / _PAIR choose nothing"""
    N, f, logD, drows, n1p, kacc, mk_, balanced, planes, scratch = ints
    g, waves, blocks, pair, mfma = sw
    if mfma != 0 and planes and scratch and not balanced and logD == 2 and drows == 3:
        return KS_MFMA, 32, 4
    G = g if g in (8, 16) else 32
    is_pair = pair != 0 and logD == 2 and f % 2 == 0 and G == 32 and bool(scratch)
    w = waves if waves > 0 else 4
    if w not in (2, 4) or G != 32 or (balanced and waves <= 0 and not is_pair):
        w = 1
    return (KS_PAIR if is_pair else KS_PER_DIGIT), G, w


def ks_expected(p, setting):
    """the (kernel, G, waves) a key switch of set p runs in a process started under `setting`"""
    sw = ks_switch_values(setting)
    return ks_kernel_rule(ks_set_ints(p, sw[4]), sw)


def ks_ran(s):
    """what the last key switch on the context ran, as ks_expected states it"""
    return tuple(int(s.get_metric(m)) for m in ("ks_last_kernel", "ks_last_g", "ks_last_waves"))


KS_PLAN_FIELDS = ("kernel", "G", "waves", "ngroups", "parties", "gblocks", "slabs", "digit_words", "partial_words")


def ks_plan_of(ints, B, sw=tuple(KS_SWITCH_DEFAULTS.values())):
    """the library's own plan (mkt_internal_ks_plan: no context, no device) for the ten values of ks_set_ints, a batch and the five switch values"""
    import ctypes as C
    from mktfhe_amd import _lib
    f = _lib.lib().mkt_internal_ks_plan
    f.restype, f.argtypes = None, [C.POINTER(C.c_int), C.c_ulonglong, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]
    out = (C.c_ulonglong * len(KS_PLAN_FIELDS))()
    f((C.c_int * 10)(*ints), B, (C.c_int * 5)(*sw), out)
    return dict(zip(KS_PLAN_FIELDS, (int(v) for v in out)))


# ---- one call in host or in device memory, and the same call on a context that has made no other (tests/context_life_cases.py) ----
_SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def _signed(a):
    return a.view(_SIGNED.get(a.dtype, a.dtype))


def device_tensor(a):
    """the GPU tensor to_mem makes of a contiguous host array: copied on torch's current stream, the host waiting for it.  The one place
    it is made, so that the stream-order tests can put LateProducer.tensor here (pytest's monkeypatch) and leave every step function alone"""
    import torch
    return torch.from_numpy(_signed(a)).cuda()


def to_mem(a, mem):
    """a host array as the argument of a call in memory kind `mem`: its own contiguous copy (MEM_HOST) or a GPU tensor of the same words
    (MEM_DEVICE; torch has no unsigned 32- / 64-bit tensors: the signed type of the same size)"""
    a = np.array(a, order="C", copy=True)
    if mem == mk.MEM_HOST:
        return a
    return device_tensor(a)


def host_words(x):
    """what a call returned -- an array, a GPU tensor or a tuple of them -- as host arrays; integer words as unsigned"""
    if isinstance(x, (tuple, list)):
        return tuple(host_words(v) for v in x)
    if type(x).__module__.startswith("torch"):
        x = x.cpu().numpy()
    x = np.ascontiguousarray(x)
    return x.view({"i4": np.uint32, "i8": np.uint64}.get(x.dtype.str[1:], x.dtype))


def same_words(a, b):
    """exact equality of two results of host_words, bit for bit (transforms included: no floating-point comparison)"""
    if isinstance(a, tuple) or isinstance(b, tuple):
        return isinstance(a, tuple) and isinstance(b, tuple) and len(a) == len(b) and all(same_words(u, v) for u, v in zip(a, b))
    return a.dtype == b.dtype and bits_equal(a, b)


def fresh(make, call):
    """call(scheme) on a context that make() has just created and keyed, used for this one call and closed -> host_words of the result"""
    s = make()
    try:
        return host_words(call(s))
    finally:
        s.close()


# ---- a producer that is late on purpose (tests/test_gpu_stream_order.py; the case lists are tests/stream_cases.py) ----
def sleep_cycles_per_ms():
    """how many cycles of torch.cuda._sleep last one millisecond on this GPU: _sleep(10**7) between two timing events, after a short one
    that takes the first launch's set-up out of the measurement"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(10**5)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(10**7)
    b.record()
    b.synchronize()
    return 10**7 / a.elapsed_time(b)


class LateProducer:
    """Device tensors whose real words arrive late.  delay() enqueues a spin of `cycles` on `stream`; tensor(a) -- what device_tensor is
    replaced with -- returns a tensor that holds POISON (all-zero words: valid indices, selectors, gate codes and ciphertext words for
    every entry point, so a mis-ordered call computes wrong words and never faults), written and waited for on a side stream at once, and
    enqueues on `stream`, behind the delay, the asynchronous copy of the real words from pinned host memory.  A call that is ordered behind
    `stream` reads the real words; any step of it that is not reads zeros, every time.  The poison is written, not assumed: the caching
    allocator may hand out the block that held the real words a moment before.  Everything made here is kept until the caller has drained
    the device and drops the producer"""

    def __init__(self, stream, cycles, side=None):
        import torch
        self.stream, self.cycles, self.side, self.kept = stream, int(cycles), side or torch.cuda.Stream(), []

    def delay(self):
        import torch
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(self.cycles)

    def tensor(self, a):
        import torch
        assert a.size and a.view(np.uint8).any(), "the real words are the poison words: this tensor could not show a mis-ordered read"
        host = torch.from_numpy(_signed(a)).pin_memory()
        with torch.cuda.stream(self.side):
            t = torch.zeros(host.shape, dtype=host.dtype, device="cuda")
        self.side.synchronize()
        with torch.cuda.stream(self.stream):
            t.copy_(host, non_blocking=True)
        self.kept.append((host, t))
        return t


# ---- tests/csrc/launch_log.cpp, built over the library's rotation units (tests/test_rot_plan_cpu.py, tests/test_size_ladder_cpu.py) ----
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LAUNCH_LOG_CSRC = os.path.join(ROOT, "mktfhe_amd", "csrc")

# UNITS: (source, defines, object name): kernels.hip units 0-7, rot_block.hip at both widths, ccs_pipe.hip, fx_exact.hip, ntt_exact.hip units 1 (the
# CGGI / LMSS rotations), 2 (KMS phase 1) and 3 (launch_exact_kms, which calls it, and CCS)
LAUNCH_LOG_UNITS = ([("kernels.hip", [f"-DMKT_TU={t}"], f"kernels_tu{t}") for t in range(8)] + [("rot_block.hip", [f"-DMKT_BLK_WORD={w}"], f"rot_block_{w}") for w in (32, 64)]
         + [("ccs_pipe.hip", [], "ccs_pipe"), ("fx_exact.hip", [], "fx_exact")] + [("ntt_exact.hip", [f"-DMKT_NTT_TU={t}"], f"ntt_exact_{t}") for t in (1, 2, 3)])


def build_launch_log(csrc, out, defines=()):
    """the launch-log program over the units of `csrc`: host-only objects, a dummy for each unit's fat-binary symbol, no HIP runtime"""
    import re
    import subprocess
    from concurrent.futures import ThreadPoolExecutor
    hipcc = os.path.join(ROCM, "bin", "hipcc")
    flags = ["-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-cuda-compat", "-Wno-pass-failed", "-Wno-unused-function", "-Wno-unused-value"]

    def unit(u):
        src, defs, name = u
        obj = os.path.join(out, name + ".o")
        subprocess.run([hipcc, "--cuda-host-only", *flags, *defs, "-c", os.path.join(csrc, src), "-o", obj], check=True, capture_output=True, text=True)
        return obj

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        objs = list(pool.map(unit, LAUNCH_LOG_UNITS))
    syms = sorted(set(re.findall(r"\bU (__hip_fatbin_\w+)", subprocess.run(["nm", *objs], check=True, capture_output=True, text=True).stdout)))
    assert len(syms) == len(LAUNCH_LOG_UNITS), syms
    fat = os.path.join(out, "fatbins.cpp")
    with open(fat, "w") as f:
        f.write('extern "C" {\n' + "".join(f"unsigned long long {s}[4];\n" for s in syms) + "}\n")
    exe = os.path.join(out, "launch_log")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + csrc, *defines,
                    os.path.join(ROOT, "tests", "csrc", "launch_log.cpp"), fat, *objs, "-lpthread", "-o", exe], check=True, capture_output=True, text=True)
    return exe
