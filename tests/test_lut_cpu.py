"""Programmable bootstrap on the CPU (mktfhe.h "programmable bootstrap", mktfhe_amd/lut.py): the table step against the checker's own test
vector, the documented table layout, the client calls that encrypt and read back any torus message, the whole construction on the CPU
checker (three-input truth tables, the re-encoding recipe: DESIGN.md 1.2), and the argument checks of every lut.py function."""

import numpy as np
import pytest

import ref_lut as R
from helpers import keygen, mk, oracle_scheme, ora_params
from mktfhe_amd import _lib
from mktfhe_amd import lut as L
from mktfhe_amd import scheme as S
from oracle import oracle as O


@pytest.mark.parametrize("W", [32, 64])
@pytest.mark.parametrize("N", [64, 256])
def test_sign_table_gives_the_checkers_test_vector(N, W):
    """T = (-2^(W-3), ...) is bootstrapping.jl:11-23 word for word, for every btilde in 0 .. 2N"""
    p = mk.CGGIparam.scaled(n=8, N=N, W=W)
    so = O.Scheme(ora_params(p))
    T = mk.sign_lut(p)
    assert T.dtype == p.ring_dtype and T.shape == (N,) and int(T[0]) == (1 << W) - (1 << (W - 3))
    for bt in range(2 * N + 1):
        assert np.array_equal(R.testvector(T, bt, W, so.kacc), so.testvector(bt)), bt


@pytest.mark.parametrize("W, N, P", [(32, 64, 8), (32, 256, 1), (64, 128, 4), (64, 64, 64), (32, 1024, 8)])
def test_lut_poly_puts_each_value_on_its_window(W, N, P):
    """for every mod-switched phase phi in 0 .. 2N - 1, coefficient 0 of X^phi * lut_poly(values) is values[window] on the first half of the
    torus and its negation on the second -- through the rotation AND through the header's extraction formula"""
    p = mk.CGGIparam.scaled(n=8, N=N, W=W)
    rng = np.random.default_rng(N + P)
    mask = (1 << W) - 1
    values = [int(v) for v in rng.integers(0, 1 << 63, P, dtype=np.uint64) * 2 + 1]
    values[0], values[-1] = (1 << (W - 1)), mask                       # the word that is its own negative; all ones
    values = [v & mask for v in values]
    T = mk.lut_poly(values, p)
    assert T.dtype == p.ring_dtype and np.array_equal(T.astype(np.uint64), R.lut_poly(values, N, W))
    for phi in range(2 * N):
        want = values[phi * P // N] if phi < N else (-values[(phi - N) * P // N]) & mask
        assert int(R.rotate(T, phi, W)[0]) == want == R.extracted(T.astype(np.uint64), phi, W), phi
    with pytest.raises(ValueError):
        mk.lut_poly([1, 2, 3], p)                                       # 3 does not divide N


@pytest.mark.parametrize("p", [mk.CGGIparam.scaled(n=20, N=256), mk.KMS2party.scaled(n=16, N=256)], ids=lambda p: p.name)
def test_client_calls_encrypt_and_read_back_any_message(p):
    crs, keys = keygen(p, 31)
    dk = keys if p.multikey else keys[0]
    for j, bit in enumerate((0, 1, 1, 0)):
        i = j % p.nparty
        mu = (1 << 29) if bit else (0 - (1 << 29)) & 0xFFFFFFFF
        c = mk.lwe_encrypt_word(mu, i, keys[i], p, deterministic_seed=4100 + j)
        assert np.array_equal(c, mk.lwe_ith_encrypt(bit, i, keys[i], p, deterministic_seed=4100 + j))
        ph = mk.lwe_phase(c, dk, p)
        err = ((ph - mu + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
        # fresh-noise law: a rounded Gaussian of standard deviation alpha (params.py, absolute on the 32-bit torus); 8 sigma + the rounding
        assert abs(err) <= 8 * p.alpha + 1, (err, p.alpha)
        assert bool(mk.lwe_decrypt(c, dk, p)) == (ph < (1 << 31)) == bool(bit)
    # any message: the phase returns it
    batch = np.stack([mk.lwe_encrypt_word(m, 0, keys[0], p, deterministic_seed=4200 + m) for m in (0, 1 << 28, 3 << 28, 0xF0000000)])
    ph = mk.lwe_phase(batch, dk, p)
    assert ph.shape == (4,) and ph.dtype == np.uint32
    for m, v in zip((0, 1 << 28, 3 << 28, 0xF0000000), ph):
        assert abs(((int(v) - m + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)) <= 8 * p.alpha + 1


# the whole construction on the CPU checker (ref_lut.CHAIN_SETS: the shipped CGGI and two-party KMS sets, their own noise, their own N)
CHAIN_SETS = [getattr(mk, name) for name in R.CHAIN_SETS]


@pytest.mark.parametrize("p", CHAIN_SETS, ids=lambda p: p.name)
def test_truth_tables_and_reencoding_decode_on_the_checker(p):
    """modswitch -> table step -> blindrotate! -> keyswitch! on the checker alone: all 8 input combinations of AND3, OR3, x ? y : z and a
    random table decrypt to the table's bit (inputs at scale 1/16 with weights 1, 2, 4, centre 1/32, P = 8, outputs +-1/8), and the
    re-encoding recipe turns a gate bit into a scale-1/16 input (a +-1/32 table, then + 1/32).  Pinned keys and inputs: the truth-table
    inputs are fresh encryptions (margin 1/32 against sigma 0.002); a re-encoding's margin of 1/32 is only 1.3 - 2.5 sigma of these sets'
    bootstrap output (DESIGN.md 1b gives the predicted miss rates), so that part shows the construction, not a reliability"""
    crs, keys, x, y, z = R.chain_case(p)
    so = oracle_scheme(p, crs, keys)
    dk = keys if p.multikey else keys[0]
    lin = R.truth_linear(x, y, z)
    ph = mk.lwe_phase(lin, dk, p)
    for v in range(8):                                   # the inputs sit inside their windows with at least half the margin to spare
        assert abs(int(ph[v]) - (v * R.SCALE16 + R.CENTRE)) < (1 << 26), v
    assert len(set(map(tuple, R.TRUTH_TABLES.values()))) == 4
    for name, table in R.TRUTH_TABLES.items():
        T = mk.lut_poly(R.truth_values(table, p.W), p)
        out = np.stack([R.checker_bootstrap(so, T, lin[v], p.W) for v in range(8)])
        assert np.array_equal(mk.lwe_decrypt(out, dk, p), np.array(table, dtype=bool)), name
    # re-encoding: gate bits +-1/8 -> {0, 1/16}
    T = mk.lut_poly([1 << (p.W - 5)], p)
    for bit in (0, 1):
        c = mk.lwe_ith_encrypt(bit, bit % p.nparty, keys[bit % p.nparty], p, deterministic_seed=6200 + bit)
        out = R.checker_bootstrap(so, T, c, p.W)
        out[-1] += np.uint32(1 << 27)
        ph = int(mk.lwe_phase(out, dk, p))
        assert ((ph + (1 << 27)) >> 28) & 15 == bit, (bit, ph)        # decodes: the nearest sixteenth of the torus is bit / 16


# ---- argument checks, with the recording-stub pattern of test_batch_args_cpu.py ----
PARAMS = [mk.CGGIparam.scaled(n=10, N=256), mk.KMS2party.scaled(n=8, N=256)]
B, P, NL = 3, 5, 2
ROWS, COUNT, POOL, SOLO, TABLE = "rows", "count", "pool", "solo", "table"


def _specs(p):
    Ln, N, rd = p.lwe_len, p.N, p.ring_dtype
    ct = lambda n=B: np.zeros((n, Ln), np.uint32)                       # noqa: E731
    luts = lambda: np.zeros((NL, N), rd)                                # noqa: E731
    sel = lambda: np.zeros(B, np.uint32)                                # noqa: E731
    return {
        "lut_testvector": ("lut_testvector_batch", [("luts", luts(), TABLE), ("ctxt", ct(), SOLO), ("sel", sel(), COUNT)], None),
        "lut_bootstrap": ("lut_bootstrap_batch", [("luts", luts(), TABLE), ("ctxt", ct(), ROWS), ("sel", sel(), COUNT), ("out", ct(), ROWS)], "out"),
        "lut_gather": ("lut_batch_gather", [("luts", luts(), TABLE), ("sel", sel(), COUNT), ("pool", ct(P), POOL), ("idx", np.zeros((B, 4), np.uint32), ROWS),
                                            ("wt", np.zeros((B, 4), np.int8), ROWS), ("cst", np.zeros(B, np.uint32), COUNT), ("out", ct(), ROWS)], "out"),
    }


def _wrong(a, how, p):
    out = []
    if how in (ROWS, COUNT):
        out += [("one row short", a[:-1].copy()), ("one row long", np.concatenate([a, a[:1]]))]
    if how in (ROWS, POOL, TABLE) or (how == SOLO and a.ndim > 1):
        out.append(("wrong row length", np.ascontiguousarray(a[..., :-1])))
    if how == TABLE:
        other = np.uint32 if p.W == 64 else np.uint64
        out += [("wrong word size", a.astype(other)), ("floating point", a.astype(np.float64))]
    return out


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("mkt_"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


@pytest.fixture
def lib(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    return rec


def _make(cls, p):
    s = object.__new__(cls)
    s.params, s.h, s.arith = p, None, S.ARITH_F64REF
    if cls is S.Scheme:
        s.device, s._user_stream = 0, False
    return s


CASES = [(S.Scheme, "lut_testvector"), (S.Scheme, "lut_bootstrap"), (S.Scheme, "lut_gather"), (S.MultiScheme, "lut_bootstrap")]
PREFIX = {S.Scheme: "mkt_", S.MultiScheme: "mkt_multi_"}


def _invoke(cls, p, method, named):
    return getattr(L, method)(_make(cls, p), **named)


@pytest.mark.parametrize("p", PARAMS, ids=lambda p: p.name)
@pytest.mark.parametrize("cls, method", CASES, ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_a_correct_call_reaches_one_symbol_with_its_batch(lib, cls, method, p):
    sym, args, ret = _specs(p)[method]
    named = {n: v for n, v, _ in args}
    got = _invoke(cls, p, method, named)
    name = PREFIX[cls] + sym
    assert [c[0] for c in lib.calls] == [name]
    cargs = lib.calls[0][1]
    assert len(cargs) == len(_lib.SYMBOLS[name][1]), "argument count of the ABI symbol"
    assert cargs[-2:] == (B, S.MEM_HOST) and cargs[2] == NL
    if "pool" in named:
        assert cargs[5] == P, "pool rows"
    if ret is not None:
        assert got is named[ret]
    else:
        assert got.shape == (B, p.k + 1, p.N) and got.dtype == p.ring_dtype


@pytest.mark.parametrize("p", PARAMS, ids=lambda p: p.name)
@pytest.mark.parametrize("cls, method", CASES, ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_a_wrongly_sized_buffer_is_refused_before_the_library(lib, cls, method, p):
    sym, args, _ = _specs(p)[method]
    tried = 0
    for i, (name, value, how) in enumerate(args):
        for label, bad in _wrong(value, how, p):
            named = {n: v for n, v, _ in args}
            named[name] = bad
            with pytest.raises(ValueError):
                _invoke(cls, p, method, named)
            assert lib.calls == [], (name, label)
            tried += 1
    assert tried >= 4


def test_defaults_one_table_no_selector(lib):
    """a single (N,) table is one row, sel None reaches the library as NULL, out None is a new array of the input's shape"""
    p = PARAMS[0]
    x = np.zeros((2, B, p.lwe_len), np.uint32)
    out = L.lut_bootstrap(_make(S.Scheme, p), mk.sign_lut(p), x)
    assert out.shape == x.shape and out is not x
    name, cargs = lib.calls[0]
    assert name == "mkt_lut_bootstrap_batch" and cargs[2] == 1 and cargs[3] is None and cargs[-2] == 2 * B
    acc = L.lut_testvector(_make(S.Scheme, p), mk.sign_lut(p), x)
    assert acc.shape == (2, B, p.k + 1, p.N)


def test_the_public_method_sets_are_untouched():
    """the LUT surface is module-level: no public method joined Scheme, MultiScheme or their shared base"""
    for name in ("lut_testvector", "lut_bootstrap", "lut_gather"):
        assert not hasattr(S.Scheme, name) and not hasattr(S.MultiScheme, name)
        assert getattr(mk, name) is getattr(L, name)
