"""Oracle-independent checks of the engine's outputs under the secret keys: the case lists and the measuring functions that
tests/test_noise_live_cpu.py (on the reference side, no GPU), tests/test_gpu_noise.py (on the engine) and tools/noise_live.py (the record) share.

Everything here is plain numpy and Python integers on the 32-bit torus; nothing of oracle/ is called.  The engine is an argument: an object
with the methods of Engine below (the GPU tests wrap a keyed mk.Scheme in it, the CPU tests a stand-in made of the reference side).

Three laws, none of which is a comparison of words with another implementation:
  A  the mod switch rounds every word to the nearest point of the stated grid, so the switched phase misses the true one by a sum of 1 + hw
     independent uniform rounding errors (hw = the ones of the LWE keys): mean 0, variance o^2 (1 + hw) / 12 / (2N)^2, an Irwin-Hall shape;
  B  a bootstrap's output carries the noise tools/noise_theory.py predicts for the set (tests/golden/noise_predicted.json);
  C  every output bit of every table-lookup call is the sign of coefficient v of X^phi~ T, phi~ being computed exactly from the engine's own
     switched row and the keys -- at every phase, window borders included, with no case left out.
"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import mktfhe_amd as mk  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- case lists ------------------------------------------------------------------------------------------------------------------------
ROWS_A, ROWS_B, ROWS_C = 4096, 2048, 4096
SETS = {n: getattr(mk, n) for n in ("CGGIparam", "Blockparam", "CCS2party", "KMS2party_N1024_l2", "KMS2partyblock")}
SETS["CGGI_n20_N256"] = mk.CGGIparam.scaled(n=20, N=256)
F64, EXACT = "f64", "exact"
ARITH = {F64: mk.ARITH_F64REF, EXACT: mk.ARITH_EXACT}
KEY_SEED = 2026
PINNED = 64                                     # inputs of the uniform sample pinned to message 0, and as many to 1/2 (Bench.uniform)


def set_seed(name, base=KEY_SEED):
    """a seed of the set's own: two sets of one LWE shape (KMS2party_N1024_l2, CCS2party) get other keys and other inputs"""
    return base + 1000 * sum((i + 1) * ord(c) for i, c in enumerate(name))

# A: (set, o)
SWITCH_SETS = ("CGGIparam", "Blockparam", "KMS2party_N1024_l2", "CCS2party", "CGGI_n20_N256")
SWITCH_CASES = [(s, o) for s in SWITCH_SETS for o in (1, 2, 4, 8)]

# B: measured / predicted bands by (kind of prediction, mode): those of tests/test_noise_theory_cpu.py
BANDS = {("closed", F64): (0.85, 1.30), ("kms", F64): (0.8, 1.3), ("closed", EXACT): (0.9, 1.1), ("kms", EXACT): (0.8, 1.2)}
# (set, mode, EXACT implementation: "fx" the Float64 pipe, "ntt" the integer NTT, None in Float64 mode)
NAND_CASES = [("CGGIparam", F64, None), ("Blockparam", F64, None), ("CCS2party", F64, None), ("KMS2party_N1024_l2", F64, None),
              ("KMS2partyblock", F64, None),
              ("CGGIparam", EXACT, "fx"), ("KMS2party_N1024_l2", EXACT, "fx"), ("Blockparam", EXACT, "ntt"), ("CCS2party", EXACT, "ntt")]
MUX_CASES = [("CGGIparam", F64, None), ("Blockparam", F64, None)]                       # asserted
MUX_RECORDED = [("CCS2party", F64, None), ("KMS2party_N1024_l2", F64, None)]            # coherent terms do not add in quadrature: the record only
TABLE_CASES = [c for c in NAND_CASES if c[1] == F64]
MARGIN_SIGMAS = 8.0                                                                     # decryption of every output is required from here on

# C: (set, mode, EXACT implementation) x call
DECODE_SETS = [("CGGIparam", F64, None), ("Blockparam", F64, None), ("KMS2party_N1024_l2", EXACT, "fx")]
DECODE_CALLS = ("lut_random", "lut_sign", "many2", "many4", "many8", "at_threshold_nu0", "at_threshold_nu2", "at_random_nu0", "at_random_nu2")
DECODE_CASES = [(s, m, i, c) for (s, m, i) in DECODE_SETS for c in DECODE_CALLS]


def case_id(c):
    return "-".join(str(x) for x in c if x is not None)


def predicted():
    """tests/golden/noise_predicted.json: set -> mode -> {sigma_br, sigma_ks, kind}"""
    with open(os.path.join(GOLD, "noise_predicted.json")) as f:
        return json.load(f)


def predicted_sigma(pred, name, mode, rotations=1):
    """-> (sigma of an output after `rotations` blind rotations and one key switch, band)"""
    e = pred[name][mode]
    return math.sqrt(rotations * e["sigma_br"] ** 2 + e["sigma_ks"] ** 2), BANDS[(e["kind"], mode)]


def must_decrypt(pred, name, mode, rotations=1):
    return 0.125 / predicted_sigma(pred, name, mode, rotations)[0] >= MARGIN_SIGMAS


# ---- keys and inputs -------------------------------------------------------------------------------------------------------------------
def secret_keys(p, seed=KEY_SEED):
    """-> (crs or None, [PartyKeys] holding secrets only: a context generates the large keys on its device from them)"""
    crs = mk.CRS(p, seed) if p.multikey else None
    return crs, [mk.PartyKeys(p, party=i, crs=crs, secrets_only=True, deterministic_seed=seed) for i in range(p.nparty)]


def key_ones(p, keys):
    """positions of the ones in the concatenated LWE keys (binary or block-binary: words 0 / 1)"""
    s = np.concatenate([np.asarray(k.lwekey) for k in keys])
    assert s.size == p.nparty * p.n and np.isin(s, (0, 1)).all()
    return np.flatnonzero(s)


def hamming(keys):
    """the number of ones over all parties' LWE keys"""
    return int(sum(int(np.asarray(k.lwekey, dtype=np.int64).sum()) for k in keys))


def quiet_inputs(p, keys, messages, seed):
    """one ciphertext per message word of the 32-bit torus in which EVERY party is involved (so every party's rotation runs): party 0's
    lwe_encrypt_word(mu) plus an encryption of +1/8 and one of -1/8 from every other party.  Its noise is that of 2k - 1 fresh encryptions,
    far below a bootstrap's, and its mask words are uniform in every party's block -> (len(messages), lwe_len) uint32"""
    msgs = [int(m) & 0xFFFFFFFF for m in np.asarray(messages).ravel()]
    out = np.empty((len(msgs), p.lwe_len), dtype=np.uint32)
    per = 2 * p.nparty - 1
    for j, mu in enumerate(msgs):
        ct = mk.lwe_encrypt_word(mu, 0, keys[0], p, deterministic_seed=seed + per * j)
        for i in range(1, p.nparty):
            for t, w in enumerate((1 << 29, -(1 << 29))):
                ct = ct + mk.lwe_encrypt_word(w, i, keys[i], p, deterministic_seed=seed + per * j + 2 * i - 1 + t)
        out[j] = ct
    return out


def bit_words(bits):
    """bit -> +-1/8 as a torus word"""
    return np.where(np.asarray(bits, dtype=bool), 1 << 29, (1 << 32) - (1 << 29)).astype(np.uint32)


# ---- exact phases ----------------------------------------------------------------------------------------------------------------------
def phase_words(p, keys, ct):
    """b + <a, s> mod 2^32 for every row of ct (..., lwe_len), in integers: an int64 restatement of mk.lwe_phase"""
    c = np.asarray(ct, dtype=np.uint32).astype(np.uint64)
    ones = key_ones(p, keys)
    return (c[..., -1] + c[..., ones].sum(axis=-1, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)      # (sums of < 2^16 words: no 64-bit wrap)


def centred(words):
    """32-bit words -> signed int64 in [-2^31, 2^31)"""
    w = np.asarray(words).astype(np.int64) & 0xFFFFFFFF
    return np.where(w >= 1 << 31, w - (1 << 32), w)


def phase_error(p, keys, ct, expected_word):
    """the exact signed error of ct's phase against expected_word, in torus units (a multiple of 2^-32: exact in float64)"""
    return centred(phase_words(p, keys, ct).astype(np.int64) - (np.asarray(expected_word).astype(np.int64) & 0xFFFFFFFF)) / 2.0 ** 32


def modswitched_phase(p, keys, atilde, btilde, o=1):
    """the exact integer phi~ = b~ + <a~, s> mod 2N of switched rows under the real keys; every word must lie on the grid of multiples of o"""
    at = np.asarray(atilde).astype(np.int64)
    bt = np.asarray(btilde).astype(np.int64).reshape(at.shape[:-1])
    assert at.shape[-1] == p.nparty * p.n
    assert (at >= 0).all() and (at <= 2 * p.N).all() and (bt >= 0).all() and (bt <= 2 * p.N).all(), "switched words lie in [0, 2N]"
    assert not (at % o).any() and not (bt % o).any(), f"switched words are multiples of {o}"
    return (bt + at[..., key_ones(p, keys)].sum(axis=-1)) % (2 * p.N)


def switch_error(p, keys, ct, phi):
    """e = phi~ / 2N - phase(ct) mod 1, centred, in torus units"""
    shift = 32 - (p.N.bit_length() - 1) - 1
    return centred((np.asarray(phi).astype(np.int64) << shift) - phase_words(p, keys, ct).astype(np.int64)) / 2.0 ** 32


def coarse_word(w, N, nu):
    """DESIGN.md 1c restated on arrays: sw_nu(w) = divbits32(w, 32 - (log2 N + 1) + nu) << nu, with divbits32(w, bit) = (w >> bit) + bit
    (bit - 1) of w -- round to nearest, ties up -> a multiple of 2^nu in [0, 2N]"""
    w = np.asarray(w).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    bit = 32 - (N.bit_length() - 1) - 1 + nu
    return (((w >> np.uint64(bit)) + ((w >> np.uint64(bit - 1)) & np.uint64(1))) << np.uint64(nu)).astype(np.int64)


def index_table(p):
    """T[j] = j + 1: a table every rotation of which names its own b~ (btilde_of_acc)"""
    return np.arange(1, p.N + 1).astype(p.ring_dtype)


def btilde_of_acc(p, acc):
    """b~ mod 2N read back from acc = (X^b~ index_table, 0, ...) by DESIGN.md 1b's layout: with r = b~ mod N, acc.b[0] is s T[0] = s for
    r = 0 and -s T[N - r] = -s (N - r + 1) otherwise, s = -1 on N <= b~ < 2N; the mask polynomials must be zero"""
    a = np.asarray(acc).reshape(-1, p.k + 1, p.N)
    assert not a[:, 1:].any(), "mask polynomials of a test vector are zero"
    W = p.W
    v = a[:, 0, 0].astype(np.int64) if W == 64 else centred(a[:, 0, 0])
    out = np.empty(len(v), dtype=np.int64)
    for j, x in enumerate(v.tolist()):
        if abs(x) == 1:
            out[j] = 0 if x == 1 else p.N
        else:
            assert 2 <= abs(x) <= p.N, x
            r = p.N + 1 - abs(x)
            out[j] = r if x < 0 else p.N + r
    first = a[:, 0, :].astype(np.int64) if W == 64 else centred(a[:, 0, :])
    assert (np.sort(np.abs(first), axis=1) == np.arange(1, p.N + 1)).all(), "a signed permutation of the index table"
    return out


# ---- what a table bootstrap reads ------------------------------------------------------------------------------------------------------
def table_value(T, phi, coef, W):
    """coefficient `coef` of X^phi T in Z_{2^W}[X] / (X^N + 1) as DESIGN.md 1b and 1d define it -> a W-bit word (Python int).
    1d: coefficient v of X^phi T is what 1b's bootstrap reads at psi = phi - v mod 2N; 1b: T[0] for psi = 0, -T[N - psi] for 1 <= psi <= N,
    T[2N - psi] for N < psi < 2N"""
    N, mask = len(T), (1 << W) - 1
    psi = (int(phi) - int(coef)) % (2 * N)
    if psi == 0:
        return int(T[0]) & mask
    if psi <= N:
        return (-int(T[N - psi])) & mask
    return int(T[2 * N - psi]) & mask


def table_values(T, phi, coef, W):
    """table_value on arrays (phi and coef broadcast) -> signed int64: the W-bit word read as a two's complement number"""
    t = np.asarray(T).astype(np.uint64).astype(np.int64) if W == 64 else centred(T)
    N = len(t)
    psi = (np.asarray(phi).astype(np.int64) - np.asarray(coef).astype(np.int64)) % (2 * N)
    lo = -t[np.clip(N - psi, 0, N - 1)]                 # 1 <= psi <= N  (W = 64: -(-2^63) wraps to itself, as the ring does)
    hi = t[np.clip(2 * N - psi, 0, N - 1)]              # N < psi < 2N
    out = np.where(psi == 0, t[0], np.where(psi <= N, lo, hi))
    return out if W == 64 else centred(out)


def value_words(vals, W):
    """signed W-bit table words -> the 32-bit torus words the key switch keeps (the high half of a 64-bit word)"""
    return ((np.asarray(vals).astype(np.int64) >> (W - 32)) & 0xFFFFFFFF).astype(np.uint32)


def window_table(p, rng, P=8):
    """-> (values, T): a random table of P windows with the values +-1/8, laid out by mk.lut_poly"""
    e = 1 << (p.W - 3)
    values = [e if b else -e for b in rng.integers(0, 2, P)]
    return values, mk.lut_poly(values, p)


# ---- statistics ------------------------------------------------------------------------------------------------------------------------
def irwin_hall_kurtosis(m):
    """kurtosis (not excess) of a sum of m independent uniform terms of one width"""
    return 3.0 - 1.2 / m


def stats(e):
    """sample mean, standard deviation, excess kurtosis and largest magnitude"""
    e = np.asarray(e, dtype=np.float64).ravel()
    m, s = float(e.mean()), float(e.std())
    return {"n": int(e.size), "mean": m, "sigma": s, "kurtosis": float(((e - m) ** 4).mean() / s ** 4 - 3.0) if s > 0 else 0.0,
            "max": float(np.abs(e).max())}


def switch_law(p, keys, e, o):
    """law A on measured switch errors e -> stats plus the exact prediction and the two derived bands: the deviation of a sample of n
    is within 5 standard errors sqrt((kappa - 1) / 4n) of sigma (kappa = 3 - 1.2 / (1 + hw)), its mean within 5 sigma / sqrt n of zero"""
    hw, n = hamming(keys), int(np.size(e))
    sigma = o * math.sqrt((1 + hw) / 12.0) / (2 * p.N)
    kappa = irwin_hall_kurtosis(1 + hw)
    r = stats(e)
    r.update(hw=hw, o=o, sigma_pred=sigma, ratio=r["sigma"] / sigma, band_ratio=5.0 * math.sqrt((kappa - 1.0) / (4.0 * n)),
             band_mean=5.0 * sigma / math.sqrt(n), kurtosis_pred=kappa - 3.0)
    r["ok"] = abs(r["ratio"] - 1.0) <= r["band_ratio"] and abs(r["mean"]) <= r["band_mean"]
    return r


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
class Engine:
    """the calls the harness makes, on a keyed mk.Scheme (a stand-in offers the same methods)"""

    def __init__(self, scheme):
        self.s, self.p = scheme, scheme.params

    def modswitch(self, ct):
        return self.s.modswitch(ct)

    def many_testvector(self, T, ct, nout):
        return mk.lut_many_testvector(self.s, T, ct, nout)

    def lut(self, T, ct):
        return mk.lut_bootstrap(self.s, T, ct)

    def lut_many(self, U, ct, nout):
        return mk.lut_many_bootstrap(self.s, U, ct, nout)

    def lut_at(self, T, ct, coef, nu):
        return mk.lut_bootstrap_at(self.s, T, ct, coef, nu=nu)

    def gate(self, op, x, y):
        return self.s.gate(op, x, y)

    def mux(self, s, a, b):
        return mk.MUX(s, a, b, self.s)


class Bench:
    """what the GPU tests and tools/noise_live.py share: one set of secrets, one keyed context per (set, arithmetic mode) and one set of
    inputs per set, each made when first asked for; close() closes every context"""

    def __init__(self):
        self.keys, self.ctx, self.rows = {}, {}, {}

    def secrets(self, name):
        if name not in self.keys:
            self.keys[name] = (SETS[name],) + secret_keys(SETS[name], set_seed(name))
        return self.keys[name]

    def engine(self, name, mode, impl=None):
        p, crs, keys = self.secrets(name)
        if (name, mode) not in self.ctx:
            self.ctx[(name, mode)] = mk.setup(p, keys=keys, a=crs, arith=ARITH[mode]) if p.multikey else mk.setup(p, keys=keys[0], arith=ARITH[mode])[1]
        s = self.ctx[(name, mode)]
        if impl is not None:
            s.set_option("exact_impl", 1 if impl == "fx" else 0)
        return Engine(s), p, keys

    def served_by(self, name, mode, impl):
        """the rotation kernel of the last call is the implementation the case names"""
        if impl is not None:
            kern = self.ctx[(name, mode)].last_kernel_name()
            assert ("fx_" in kern) == (impl == "fx"), (name, mode, impl, kern)

    def uniform(self, name):
        return uniform_inputs(name, *self.secrets(name)[::2], self.rows)

    def bits(self, name):
        """three operands of ROWS_B quiet encryptions of random bits -> (ct [3][ROWS_B][lwe_len], bits [3][ROWS_B])"""
        if (name, "bits") not in self.rows:
            p, _, keys = self.secrets(name)
            b = np.random.default_rng(set_seed(name, 103)).integers(0, 2, (3, ROWS_B)).astype(bool)
            ct = quiet_inputs(p, keys, bit_words(b.ravel()), set_seed(name, 900_000)).reshape(3, ROWS_B, p.lwe_len)
            self.rows[(name, "bits")] = (ct, b)
        return self.rows[(name, "bits")]

    def close(self):
        for s in self.ctx.values():
            s.close()
        self.ctx.clear()


def uniform_inputs(name, p, keys, cache=None):
    """ROWS_C quiet inputs with messages uniform over the 32-bit torus, except that the first PINNED carry the message 0 and the next
    PINNED the message 1/2: the switch moves a phase by a few slots either way, so among that many the switched phases 0 and N occur
    (at every o: asserted where the sample is used, reads_the_corners), which 4096 uniform draws over 2N values miss one time in eight"""
    cache = {} if cache is None else cache
    if (name, "uniform") not in cache:
        msgs = np.random.default_rng(set_seed(name, 101)).integers(0, 1 << 32, ROWS_C, dtype=np.uint64)
        msgs[:PINNED], msgs[PINNED:2 * PINNED] = 0, 1 << 31
        msgs[2 * PINNED:2 * PINNED + 4] = [(1 << 32) - 1, 1 << 28, (1 << 31) - 1, 3 << 30]
        cache[(name, "uniform")] = quiet_inputs(p, keys, msgs, set_seed(name, 10_000))
    return cache[(name, "uniform")]


def switched_phase(eng, p, keys, ct, o):
    """phi~ of every row of ct from the ENGINE's switched row: o = 1 the mod-switch stage; o = 2, 4, 8 the many-table table step -- a~ as it
    returns it, b~ restated from DESIGN.md 1c (coarse_word) and required to be the rotation its accumulator shows (btilde_of_acc)"""
    if o == 1:
        at, bt = eng.modswitch(ct)
    else:
        at, acc = eng.many_testvector(index_table(p), ct, o)
        bt = coarse_word(np.asarray(ct)[..., -1], p.N, o.bit_length() - 1)
        shown = btilde_of_acc(p, acc)
        assert np.array_equal(shown, bt % (2 * p.N)), ("the accumulator is rotated by another b~ than 1c defines", o,
                                                        np.flatnonzero(shown != bt % (2 * p.N))[:4])
    return modswitched_phase(p, keys, at, bt, o)


def measure_switch(eng, p, keys, ct, o):
    """law A on the engine -> switch_law's record"""
    return switch_law(p, keys, switch_error(p, keys, ct, switched_phase(eng, p, keys, ct, o)), o)


def measure_gate(eng, p, keys, kind, ct, bits):
    """law B: kind "nand" (ct, bits: two operands) or "mux" (three: s, a, b) on quiet inputs -> (errors against +-1/8, wrong decryptions)"""
    if kind == "nand":
        out, want = eng.gate(mk.NAND_OP, ct[0], ct[1]), ~(bits[0] & bits[1])
    else:
        out, want = eng.mux(ct[0], ct[1], ct[2]), np.where(bits[0], bits[1], bits[2])
    want = np.asarray(want, dtype=bool)
    return phase_error(p, keys, out, bit_words(want)), int(((centred(phase_words(p, keys, out)) > 0) != want).sum())


def decode_call(eng, p, keys, ct, call, rng):
    """law C for one call of DECODE_CALLS on inputs ct -> (wrong bits, output bits, errors against the table's own words): every output
    bit against sign(table_value(T, phi~, v)), nothing left out"""
    W, N = p.W, p.N
    _, T = window_table(p, rng)
    if call in ("lut_random", "lut_sign"):
        T = T if call == "lut_random" else mk.sign_lut(p)
        phi = switched_phase(eng, p, keys, ct, 1)
        out, want = eng.lut(T, ct), table_values(T, phi, 0, W)
    elif call.startswith("many"):
        o = int(call[4:])
        tables = np.stack([window_table(p, rng)[1] for _ in range(o)])
        U = mk.lut_pack(tables, p)
        phi = switched_phase(eng, p, keys, ct, o)
        out = eng.lut_many(U, ct, o)
        want = table_values(U, phi[:, None], np.arange(o)[None, :], W)
        packed = np.stack([table_values(tables[v], phi, 0, W) for v in range(o)], axis=1)
        assert np.array_equal(want, packed), "packing law: coefficient v of X^phi~ U is what table v reads at phi~"
    else:
        nu = int(call[-1])
        if "threshold" in call:
            T, coef = mk.sign_lut(p), mk.lut_threshold_coefs(8, p)
        else:
            coef = np.concatenate([[0, 1, N - 1], rng.choice(np.arange(2, N - 1), 13, replace=False)]).astype(np.uint32)
            coef = coef[rng.permutation(16)]
        phi = switched_phase(eng, p, keys, ct, 1 << nu)
        out = eng.lut_at(T, ct, coef, nu)
        want = table_values(T, phi[:, None], coef.astype(np.int64)[None, :], W)
    out = np.asarray(out).reshape(want.shape + (p.lwe_len,))
    assert (want != 0).all()
    e = phase_error(p, keys, out, value_words(want, W))
    got = centred(phase_words(p, keys, out)) > 0
    return int((got != (want > 0)).sum()), int(want.size), e, phi


def reads_the_corners(p, phi, coef=(0,)):
    """does a sample of switched phases read the table at psi = phi~ - v = 0 (T[0], the one entry not negated) and at psi = N (-T[0])?"""
    psi = (np.asarray(phi).astype(np.int64)[:, None] - np.asarray(coef).astype(np.int64)[None, :]) % (2 * p.N)
    return bool((psi == 0).any() and (psi == p.N).any())


def window_misses(eng, p, keys, o, rows, seed):
    """DESIGN.md 1c's P = 8 recipe on quiet inputs at window centres m / 16 + 1 / 32: how many switched phases leave their window, beside the
    Gaussian prediction erfc(margin / (sigma sqrt 2)) for the exact mod-switch sigma of law A"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 8, rows)
    ct = quiet_inputs(p, keys, (m.astype(np.int64) << 28) + (1 << 27), seed)
    phi = switched_phase(eng, p, keys, ct, o)
    sigma = o * math.sqrt((1 + hamming(keys)) / 12.0) / (2 * p.N)
    return {"o": o, "rows": rows, "misses": int((phi * 8 // p.N != m).sum()), "sigma_switch": sigma,
            "predicted_rate": math.erfc((1 / 32.0) / (sigma * math.sqrt(2.0)))}
