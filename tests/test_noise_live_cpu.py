"""tests/noise_cases.py against the reference side alone (no GPU): the harness is itself tested here, and every law that
tests/test_gpu_noise.py holds the engine to is first shown to hold for the restatements of the reference -- the mod-switch law on
ref_numpy's divbits and ref_lut_many's coarse switch at the sets and sample sizes of the GPU test, table_value exhaustively against
ref_lut's rotated table, the exact-phase decode through the oracle's chain at a reduced set.  The predictions the GPU test reads
(tests/golden/noise_predicted.json) are recomputed so that the file cannot go stale, and every case the harness names is one the GPU file runs."""
import math

import numpy as np
import pytest

import noise_cases as NC
import ref_lut as R
import ref_lut_many as RM
import ref_numpy as RN
from golden import gen_noise_predicted as GEN
from helpers import keygen, mk, oracle_scheme


# ---- the predictions -------------------------------------------------------------------------------------------------------------------
def test_predicted_fixture_is_current():
    """every closed-form entry, and the simulated KMS2partyblock EXACT entry (6 s), recomputed from tools/noise_theory.py"""
    have = NC.predicted()
    assert set(have) == set(GEN.CLOSED) | set(GEN.KMS) and all(set(v) == {NC.F64, NC.EXACT} for v in have.values())
    for name in GEN.CLOSED:
        for mode in (NC.F64, NC.EXACT):
            assert have[name][mode] == GEN.closed(name), (name, mode)
    want = GEN.simulated("KMS2partyblock", NC.EXACT)
    got = have["KMS2partyblock"][NC.EXACT]
    assert (got["kind"], got["trials"], got["seed"]) == (want["kind"], want["trials"], want["seed"])
    assert got["sigma_br"] == pytest.approx(want["sigma_br"], rel=1e-9) and got["sigma_ks"] == pytest.approx(want["sigma_ks"], rel=1e-9)
    for name, modes in GEN.KMS.items():
        for mode, (trials, seed) in modes.items():
            assert (have[name][mode]["trials"], have[name][mode]["seed"], have[name][mode]["kind"]) == (trials, seed, "kms")


def test_every_asserted_case_has_a_prediction_and_a_band():
    pred = NC.predicted()
    for name, mode, _ in NC.NAND_CASES + NC.MUX_CASES + NC.MUX_RECORDED + NC.TABLE_CASES:
        sigma, (lo, hi) = NC.predicted_sigma(pred, name, mode)
        assert 0.003 < sigma < 0.04 and lo < 1.0 < hi
    # what has to decrypt follows from the prediction: 8 sigma of margin.  (CCS2party's closed form is one figure for both arithmetic
    # modes, 4.0 sigma: its EXACT case is measured, not required to decrypt)
    need = {(n, m) for n, m, _ in NC.NAND_CASES if NC.must_decrypt(pred, n, m)}
    assert need == {("CGGIparam", NC.F64), ("Blockparam", NC.F64), ("CGGIparam", NC.EXACT), ("Blockparam", NC.EXACT), ("KMS2party_N1024_l2", NC.EXACT)}
    assert all(NC.must_decrypt(pred, n, m) for n, m, _ in NC.DECODE_SETS), "law C runs where the outputs keep 8 sigma"


# ---- statistics and phases -------------------------------------------------------------------------------------------------------------
def test_statistics():
    rng = np.random.default_rng(1)
    for m in (1, 2, 11, 309):
        e = (rng.random((200000, m)) - 0.5).sum(axis=1)
        st = NC.stats(e)
        assert st["sigma"] == pytest.approx(math.sqrt(m / 12.0), rel=0.01) and abs(st["mean"]) < 5 * st["sigma"] / math.sqrt(e.size)
        assert st["kurtosis"] == pytest.approx(NC.irwin_hall_kurtosis(m) - 3.0, abs=0.03), m
    assert NC.irwin_hall_kurtosis(1) == pytest.approx(1.8) and NC.stats([1.0, -1.0, 3.0, -3.0])["max"] == 3.0


def test_phases_are_the_clients_own():
    """phase_words is mk.lwe_phase on every kind of key (binary, block-binary, two parties); quiet inputs involve every party and carry
    the noise of 2k - 1 fresh encryptions"""
    for name in ("CGGI_n20_N256", "Blockparam", "KMS2party_N1024_l2"):
        p = NC.SETS[name]
        _, keys = NC.secret_keys(p)
        msgs = np.random.default_rng(3).integers(0, 1 << 32, 400, dtype=np.uint64)
        ct = NC.quiet_inputs(p, keys, msgs, 50)
        assert np.array_equal(NC.phase_words(p, keys, ct), mk.lwe_phase(ct, keys, p))
        assert (ct[:, :-1].reshape(400, p.nparty, p.n) != 0).any(axis=2).all()
        e = NC.phase_error(p, keys, ct, msgs)
        sigma = math.sqrt(2 * p.nparty - 1) * p.alpha / 2.0 ** 32
        assert NC.stats(e)["sigma"] == pytest.approx(sigma, rel=5 * math.sqrt(1 / 800.0)) and np.abs(e).max() < 6 * sigma
        ones = p.nparty * (p.blk_d * p.blk_len / (p.blk_len + 1.0) if p.blk_len else p.n / 2.0)          # binary: n / 2; block-binary: L / (L + 1) per block
        assert NC.hamming(keys) == len(NC.key_ones(p, keys)) and abs(NC.hamming(keys) - ones) < 5 * math.sqrt(ones)


# ---- what a table bootstrap reads ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [32, 64])
def test_table_value_is_the_rotated_table(W):
    """exhaustively at N = 64: coefficient v of ref_lut.rotate(T, phi, W) for every phi < 2N and v < N, scalar and array form; phi = 2N
    reads as phi = 0"""
    N = 64
    rng = np.random.default_rng(W)
    T = (rng.integers(0, 1 << 63, N, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, N, dtype=np.uint64)) & np.uint64((1 << W) - 1)
    T[3], T[N - 1] = 1 << (W - 1), (1 << W) - 1
    T = T.astype(np.uint64 if W == 64 else np.uint32)
    vs = np.arange(N)
    for phi in range(2 * N + 1):
        rot = R.rotate(T, phi, W)
        assert [NC.table_value(T, phi, v, W) for v in range(N)] == [int(x) for x in rot], phi
        signed = rot.astype(np.int64) if W == 64 else NC.centred(rot)
        assert np.array_equal(NC.table_values(T, phi, vs, W), signed), phi
        assert NC.table_value(T, phi, 0, W) == R.extracted(T, phi % (2 * N), W)
    assert np.array_equal(NC.value_words(NC.table_values(T, 5, vs, W), W), (R.rotate(T, 5, W) >> np.uint64(W - 32)).astype(np.uint32))


def test_window_tables_read_their_windows():
    """mk.lut_poly against table_value: window v of the half torus reads values[v], half a turn further -values[v]"""
    p = mk.CGGIparam.scaled(n=20, N=256, W=64)
    values, T = NC.window_table(p, np.random.default_rng(5))
    assert sorted(set(abs(v) for v in values)) == [1 << 61]
    for phi in range(2 * p.N):
        want = values[(phi % p.N) * 8 // p.N] * (1 if phi < p.N else -1)
        if phi == 0:
            want = values[0]
        if phi == p.N:
            want = -values[0]
        assert NC.table_values(T, phi, 0, 64) == want, phi


def test_btilde_is_read_back_from_an_accumulator():
    p = mk.KMS2party.scaled(n=16, N=256)
    T = NC.index_table(p)
    bts = [0, 1, 2, p.N - 1, p.N, p.N + 1, 2 * p.N - 1, 2 * p.N, 77, 300]
    acc = np.stack([R.testvector(T, bt, p.W, p.k) for bt in bts])
    assert np.array_equal(NC.btilde_of_acc(p, acc.astype(p.ring_dtype)), np.array(bts) % (2 * p.N))
    acc[3, 0, 5] += np.uint64(1)
    with pytest.raises(AssertionError):
        NC.btilde_of_acc(p, acc.astype(p.ring_dtype))


# ---- law A on the reference side -------------------------------------------------------------------------------------------------------
def _rotated_rows(T, bt, W):
    """(X^bt[j] T, 0 ...) for every j at once, by ref_lut.rotate's rule (held to it row by row in test_reference_switch_stand_in)"""
    T = np.asarray(T).astype(np.uint64)
    N = T.size
    bt = np.asarray(bt).astype(np.int64)
    r, s = bt % N, np.where((bt >= N) & (bt < 2 * N), -1, 1)
    i = np.arange(N)[None, :]
    idx = (i - r[:, None]) % N
    neg = (np.where(i >= r[:, None], 1, -1) * s[:, None]) < 0
    rows = T[idx]
    return np.where(neg, np.uint64(0) - rows, rows) & np.uint64((1 << W) - 1)


class ReferenceSwitch:
    """the switch calls of noise_cases.Engine on the reference side: ref_numpy.divbits on every word (arithmetic.jl:23-27), and for the
    coarse grid ref_lut_many's sw_nu -- divbits by nu more bits, shifted back -- with the table step of ref_lut"""

    def __init__(self, p):
        self.p = p

    def _words(self, ct, nu):
        bit = 32 - (self.p.N.bit_length() - 1) - 1 + nu
        return RN.divbits(np.ascontiguousarray(ct, dtype=np.uint32), bit, 32) << np.uint32(nu)

    def modswitch(self, ct):
        w = self._words(ct, 0)
        return w[..., :-1], w[..., -1]

    def many_testvector(self, T, ct, nout):
        w = self._words(ct, RM.nu_of(nout))
        acc = np.zeros((len(w), self.p.k + 1, self.p.N), dtype=np.uint64)
        acc[:, 0] = _rotated_rows(T, w[:, -1], self.p.W)
        return w[:, :-1], acc.astype(self.p.ring_dtype)


def test_reference_switch_stand_in():
    """the stand-in's array forms are ref_lut_many.sw and ref_lut.rotate, word for word, at the rounding edges and on random words"""
    p = NC.SETS["CGGI_n20_N256"]
    rng = np.random.default_rng(9)
    sw = ReferenceSwitch(p)
    for nout in (1, 2, 4, 8):
        words = np.array(RM.sw_edge_words(p.N, nout) + [int(x) for x in rng.integers(0, 1 << 32, 200)], dtype=np.uint32)
        want = np.array([RM.sw(int(w), p.N, nout) for w in words])
        assert np.array_equal(sw._words(words, RM.nu_of(nout)), want) and np.array_equal(NC.coarse_word(words, p.N, RM.nu_of(nout)), want)
    for W in (32, 64):
        T = rng.integers(0, 1 << 32, p.N, dtype=np.uint64) << np.uint64(W - 32)
        bts = np.array([0, 1, p.N - 1, p.N, p.N + 1, 2 * p.N - 1, 2 * p.N, 100, 400])
        assert np.array_equal(_rotated_rows(T, bts, W), np.stack([R.rotate(T, b, W) for b in bts]))


_inputs = {}


def _switch_inputs(name):
    """the keys and the uniform sample of the GPU tests themselves (noise_cases.Bench)"""
    p = NC.SETS[name]
    if name not in _inputs:
        _inputs[name] = NC.secret_keys(p, NC.set_seed(name))[1]
    return p, _inputs[name], NC.uniform_inputs(name, p, _inputs[name], _inputs)[:NC.ROWS_A]


def test_sets_of_one_shape_are_separate_samples():
    (_, ka, ca), (_, kb, cb) = _switch_inputs("KMS2party_N1024_l2"), _switch_inputs("CCS2party")
    assert not np.array_equal(NC.key_ones(NC.SETS["CCS2party"], kb), NC.key_ones(NC.SETS["KMS2party_N1024_l2"], ka)) and not np.array_equal(ca[:, -1], cb[:, -1])


@pytest.mark.parametrize("name,mode,impl", NC.DECODE_SETS)
def test_uniform_sample_reads_the_table_corners(name, mode, impl):
    """phi~ = 0 and phi~ = N occur in the GPU tests' own sample at every grid, by the reference switch (the GPU test asserts it of the engine's)"""
    p, keys, _ = _switch_inputs(name)
    ct = NC.uniform_inputs(name, p, keys, _inputs)
    for o in (1, 2, 4, 8):
        phi = NC.switched_phase(ReferenceSwitch(p), p, keys, ct, o)
        assert NC.reads_the_corners(p, phi), (name, o)
        assert not NC.reads_the_corners(p, phi[(phi != 0)]) and not NC.reads_the_corners(p, phi[phi != p.N])


@pytest.mark.parametrize("case", NC.SWITCH_CASES, ids=NC.case_id)
def test_mod_switch_law_on_the_reference(case):
    name, o = case
    p, keys, ct = _switch_inputs(name)
    r = NC.measure_switch(ReferenceSwitch(p), p, keys, ct, o)
    print(name, o, r)
    assert r["n"] == NC.ROWS_A and r["band_ratio"] == pytest.approx(0.055, abs=0.002)
    assert abs(r["ratio"] - 1.0) <= r["band_ratio"] and abs(r["mean"]) <= r["band_mean"], r


@pytest.mark.parametrize("wrong", ["truncate", "finer grid", "half the key"])
def test_mod_switch_law_rejects_wrong_switches(wrong):
    """what the law is for: a truncating switch (mean off by (1 + hw) / 2 slots), a grid one step finer than nu says (sigma halves) and a
    parity that ignores a party's key (its rounding errors are missing) all leave the bands, or the grid"""
    name, o = "KMS2party_N1024_l2", 4
    p, keys, ct = _switch_inputs(name)
    sw = ReferenceSwitch(p)
    if wrong == "truncate":
        bit = 32 - (p.N.bit_length() - 1) - 1 + 2
        at = ((ct[:, :-1] >> np.uint32(bit)) << np.uint32(2)).astype(np.int64)
        bt = (ct[:, -1] >> np.uint32(bit)) << np.uint32(2)
        r = NC.switch_law(p, keys, NC.switch_error(p, keys, ct, NC.modswitched_phase(p, keys, at, bt, o)), o)
        assert not r["ok"] and abs(r["mean"]) > 100 * r["band_mean"]
    elif wrong == "finer grid":
        w = sw._words(ct, 1)
        with pytest.raises(AssertionError, match="multiples of 4"):
            NC.modswitched_phase(p, keys, w[:, :-1], w[:, -1], o)
        r = NC.switch_law(p, keys, NC.switch_error(p, keys, ct, NC.modswitched_phase(p, keys, w[:, :-1], w[:, -1], 2)), o)
        assert not r["ok"] and r["ratio"] == pytest.approx(0.5, abs=0.03)
    else:
        at, acc = sw.many_testvector(NC.index_table(p), ct, o)
        at = at.copy()
        at[:, p.n:] = 0
        phi = NC.modswitched_phase(p, keys, at, NC.coarse_word(ct[:, -1], p.N, 2), o)
        r = NC.switch_law(p, keys, NC.switch_error(p, keys, ct, phi), o)
        assert not r["ok"]


# ---- law C through the oracle's chain --------------------------------------------------------------------------------------------------
class OracleChain(ReferenceSwitch):
    """noise_cases.Engine on the CPU checker: its modswitch, ref_lut's table step, its blindrotate! and keyswitch! (ref_lut.checker_bootstrap,
    ref_lut_many.checker_many), and for a coefficient list the extraction E_v before the key switch"""

    def __init__(self, p, so):
        super().__init__(p)
        self.so = so

    def modswitch(self, ct):
        rows = [self.so.modswitch(c) for c in ct]
        return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows])

    def lut(self, T, ct):
        return np.stack([R.checker_bootstrap(self.so, T, c, self.p.W) for c in ct])

    def lut_many(self, U, ct, nout):
        return np.stack([RM.checker_many(self.so, U, c, nout, self.p.W) for c in ct])

    def lut_at(self, T, ct, coef, nu):
        out = []
        for c in ct:
            at, bt = RM.sw_row(c, self.p.N, 1 << nu)
            acc = self.so.blindrotate(at, R.testvector(T, bt, self.p.W, self.so.kacc))
            out.append(np.stack([self.so.keyswitch(RM.extract(acc, int(v), self.p.W)) for v in coef]))
        return np.stack(out)


# CGGIparam.scaled(n=20, N=256) is tests/test_gpu_parity.py's first SMALL set; noise_theory.predict gives it sigma = 0.0016: 78 sigma of
# output margin (asserted below), so the shape of the issue stands
CHAIN_SET = NC.SETS["CGGI_n20_N256"]
CHAIN_ROWS = 256


@pytest.fixture(scope="module")
def chain():
    import noise_theory as T
    p = CHAIN_SET
    assert 0.125 / T.predict(p)[2] >= NC.MARGIN_SIGMAS
    crs, keys = keygen(p, 41)
    msgs = np.random.default_rng(23).integers(0, 1 << 32, CHAIN_ROWS, dtype=np.uint64)
    msgs[:6] = [0, 1 << 31, (1 << 32) - 1, 1 << 28, (1 << 31) - 1, 3 << 30]              # the torus' own corners among the uniform ones
    return p, keys, OracleChain(p, oracle_scheme(p, crs, keys)), NC.quiet_inputs(p, keys, msgs, 3000), T.predict(p)[2]


@pytest.mark.parametrize("call", NC.DECODE_CALLS)
def test_exact_phase_decode_through_the_oracle_chain(chain, call):
    p, keys, eng, ct, sigma = chain
    wrong, bits, e, phi = NC.decode_call(eng, p, keys, ct, call, np.random.default_rng(31))
    st = NC.stats(e)
    print(call, bits, wrong, st, sigma)
    per_input = 1 if call.startswith("lut") else int(call[4:]) if call.startswith("many") else 8 if "threshold" in call else 16
    assert bits == CHAIN_ROWS * per_input
    assert wrong == 0
    assert 0.85 < st["sigma"] / sigma < 1.30 and st["max"] < 0.125


# ---- drift -----------------------------------------------------------------------------------------------------------------------------
def test_every_named_case_is_run_on_the_gpu():
    """each case list of noise_cases.py is, whole and in order, the parameter list of a test of tests/test_gpu_noise.py, all of it marked gpu"""
    import test_gpu_noise as G
    assert G.pytestmark.name == "gpu"
    lists = []
    for name in dir(G):
        fn = getattr(G, name)
        if name.startswith("test_") and callable(fn):
            lists += [list(mark.args[1]) for mark in getattr(fn, "pytestmark", []) if mark.name == "parametrize"]
    for which in ("SWITCH_CASES", "NAND_CASES", "MUX_CASES", "TABLE_CASES", "DECODE_CASES"):
        cases = getattr(NC, which)
        assert cases and any(ran is cases or ran == cases for ran in lists), which
    assert len(lists) == 5, "a parametrised GPU test whose cases noise_cases.py does not name"
