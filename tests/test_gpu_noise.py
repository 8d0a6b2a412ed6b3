"""The engine's outputs opened under the secret keys and held to laws that follow from the schemes' definitions -- nothing of oracle/ is
called here, so a sign convention, a window border, a rounding direction or a grid factor that kernel and oracle got wrong alike does not pass.

  A  the mod switch (the stage, and the many-table table step at o = 2, 4, 8) rounds to nearest on the stated grid: the switched phase under
     the real keys misses the true one by mean 0 and variance o^2 (1 + hw) / 12 / (2N)^2 exactly, hw the keys' Hamming weight.  4096 rows
     per case; |s / sigma - 1| <= 5 sqrt((kappa - 1) / 4n) ~ 0.055 with kappa = 3 - 1.2 / (1 + hw) (five standard errors of a sample
     deviation: derived, not measured) and |mean| <= 5 sigma / sqrt n.
  B  the output noise of a bootstrap, live: 2048 outputs per case on quiet all-party inputs against tests/golden/noise_predicted.json
     (tools/noise_theory.py), within the bands tests/test_noise_theory_cpu.py holds per kind; where the prediction leaves 8 sigma of margin
     every output decrypts.  NAND in both arithmetic modes, the native MUX, and a table bootstrap (the table changes the message, not the noise).
  C  every output bit of lut_bootstrap, lut_many_bootstrap and lut_bootstrap_at on 4096 inputs uniform over the whole torus (128 of
     them pinned to the messages 0 and 1/2, so that phi~ = 0 and phi~ = N are met: asserted) equals sign(table_value(T, phi~, v)), phi~
     computed exactly from the engine's own switched row and the secret keys: no case left out.

The harness is tests/noise_cases.py; tests/test_noise_live_cpu.py shows it against the reference side and keeps these case lists whole.
Each test prints its figures before it asserts."""
import numpy as np
import pytest

import noise_cases as NC
from noise_cases import mk

pytestmark = pytest.mark.gpu
PRED = NC.predicted()


@pytest.fixture(scope="module")
def bench(require_gpu):
    b = NC.Bench()
    yield b
    b.close()


# ---- A ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NC.SWITCH_CASES, ids=NC.case_id)
def test_mod_switch_rounds_to_nearest_on_the_stated_grid(bench, case):
    name, o = case
    eng, p, keys = bench.engine(name, NC.F64)
    ct = bench.uniform(name)[:NC.ROWS_A]
    r = NC.measure_switch(eng, p, keys, ct, o)
    print("A", name, o, r)
    assert r["n"] == NC.ROWS_A == 4096
    assert abs(r["ratio"] - 1.0) <= r["band_ratio"], r
    assert abs(r["mean"]) <= r["band_mean"], r


# ---- B ---------------------------------------------------------------------------------------------------------------------------------
def _held_to_prediction(tag, case, e, wrong, rotations=1):
    name, mode, _ = case
    sigma, (lo, hi) = NC.predicted_sigma(PRED, name, mode, rotations)
    st = NC.stats(e)
    need = NC.must_decrypt(PRED, name, mode, rotations)
    print(tag, NC.case_id(case), st, "predicted", sigma, "ratio", st["sigma"] / sigma, "band", (lo, hi), "wrong", wrong, "must decrypt", need)
    assert lo < st["sigma"] / sigma < hi, (tag, case, st, sigma)
    if need:
        assert wrong == 0, (tag, case, wrong)


@pytest.mark.parametrize("case", NC.NAND_CASES, ids=NC.case_id)
def test_nand_output_noise_is_the_predicted(bench, case):
    name, mode, impl = case
    eng, p, keys = bench.engine(name, mode, impl)
    ct, b = bench.bits(name)
    e, wrong = NC.measure_gate(eng, p, keys, "nand", ct[:2], b[:2])
    bench.served_by(name, mode, impl)
    assert e.size == NC.ROWS_B == 2048
    _held_to_prediction("B nand", case, e, wrong)


@pytest.mark.parametrize("case", NC.MUX_CASES, ids=NC.case_id)
def test_native_mux_output_noise_is_two_rotations_and_a_key_switch(bench, case):
    name, mode, impl = case
    eng, p, keys = bench.engine(name, mode, impl)
    ct, b = bench.bits(name)
    e, wrong = NC.measure_gate(eng, p, keys, "mux", ct, b)
    _held_to_prediction("B mux", case, e, wrong, rotations=2)


@pytest.mark.parametrize("case", NC.TABLE_CASES, ids=NC.case_id)
def test_table_bootstrap_noise_does_not_depend_on_the_table(bench, case):
    """an eight-window +-1/8 table on ROWS_B uniform inputs, its errors against the word the table holds at the switched phase"""
    name, mode, impl = case
    eng, p, keys = bench.engine(name, mode, impl)
    wrong, bits, e, _ = NC.decode_call(eng, p, keys, bench.uniform(name)[-NC.ROWS_B:], "lut_random", np.random.default_rng(107))
    assert bits == NC.ROWS_B
    _held_to_prediction("B table", case, e, wrong)


# ---- C ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NC.DECODE_CASES, ids=NC.case_id)
def test_every_output_bit_is_what_the_switched_phase_says(bench, case):
    name, mode, impl, call = case
    eng, p, keys = bench.engine(name, mode, impl)
    ct = bench.uniform(name)
    wrong, bits, e, phi = NC.decode_call(eng, p, keys, ct, call, np.random.default_rng(109))
    bench.served_by(name, mode, impl)
    sigma, _ = NC.predicted_sigma(PRED, name, mode)
    print("C", NC.case_id(case), "bits", bits, "wrong", wrong, NC.stats(e), "predicted", sigma)
    assert len(ct) == NC.ROWS_C == 4096 and bits >= NC.ROWS_C
    assert NC.reads_the_corners(p, phi), "the sample meets phi~ = 0 and phi~ = N (every coefficient list holds v = 0)"
    assert wrong == 0, (case, wrong, bits)
