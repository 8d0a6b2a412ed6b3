"""Many-table bootstrap on the CPU (mktfhe.h "many-table bootstrap", mktfhe_amd/lut.py): the packing law, the extraction
E_v, the coarse mod-switch at its rounding edges, recipe (a) -- a full adder of three fresh inputs in one rotation -- on the CPU checker,
and the argument checks of every new lut.py function against a recording stub."""
import os
import re

import numpy as np
import pytest

import ref_lut as R
import ref_lut_many as RM
from helpers import ROOT, mk, oracle_scheme
from mktfhe_amd import _lib
from mktfhe_amd import lut as L
from mktfhe_amd import scheme as S


def _random_tables(o, N, W, rng):
    t = (rng.integers(0, 1 << 63, (o, N), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (o, N), dtype=np.uint64)) & np.uint64((1 << W) - 1)
    t[:, 0], t[:, -1] = 1 << (W - 1), (1 << W) - 1                   # the word that is its own negative; all ones
    return t


# ---- the packing law ----
@pytest.mark.parametrize("o", RM.NOUT)
@pytest.mark.parametrize("W", [32, 64])
def test_packing_law_holds_for_every_grid_phase_and_output(W, o):
    """coefficient v of X^phi * U is what the single-table bootstrap of T_v extracts at phi, for EVERY phi on the coarse grid and every v"""
    N = 64
    p = mk.CGGIparam.scaled(n=8, N=N, W=W)
    tables = _random_tables(o, N, W, np.random.default_rng(100 * W + o)).astype(p.ring_dtype)
    U = mk.lut_pack(tables, p)
    assert U.dtype == p.ring_dtype and U.shape == (N,) and np.array_equal(U, RM.pack(tables))
    if o == 1:
        assert np.array_equal(U, tables[0])
    for phi in range(0, 2 * N, o):
        rot = R.rotate(U, phi, W)
        for v in range(o):
            assert int(rot[v]) == R.extracted(tables[v].astype(np.uint64), phi, W), (phi, v)


def test_packing_refuses_other_counts_and_foreign_words():
    p = mk.CGGIparam.scaled(n=8, N=64)
    t = np.zeros((3, 64), np.uint32)
    for bad in (t, t[:0], np.zeros((16, 64), np.uint32), np.zeros((2, 32), np.uint32), np.zeros((2, 64), np.uint64), np.zeros((2, 64), np.float64), np.zeros(64, np.uint32)):
        with pytest.raises(ValueError):
            mk.lut_pack(bad, p)
    with pytest.raises(ValueError):
        mk.lut_pack(np.zeros((8, 4), np.uint32), mk.CGGIparam.scaled(n=8, N=4))       # more tables than coefficients


# ---- the extraction ----
@pytest.mark.parametrize("W", [32, 64])
def test_extraction_moves_coefficient_v_to_zero_and_composes(W):
    N = 64
    rng = np.random.default_rng(W)
    acc = _random_tables(3, N, W, rng)
    acc[1, :3] = [0, 1, 1 << (W - 1)]
    mask = (1 << W) - 1
    for v in range(9):
        e = RM.extract(acc, v, W)
        assert np.array_equal(e[:, 0], acc[:, v]), v
        assert np.array_equal(e[:, N - v:], (np.uint64(0) - acc[:, :v]) & np.uint64(mask)), "exactly the last v words are negated"
        assert np.array_equal(e[:, :N - v], acc[:, v:])
    assert np.array_equal(RM.extract(acc, 0, W), acc)
    for u, v in ((1, 2), (3, 5), (7, 7), (N - 3, 7), (N - 1, 1)):          # the last two wrap past N: E_{u+v} = -E_{u+v-N}
        both = RM.extract(RM.extract(acc, u, W), v, W)
        want = RM.extract(acc, u + v, W) if u + v < N else (np.uint64(0) - RM.extract(acc, u + v - N, W)) & np.uint64(mask)
        assert np.array_equal(both, want), (u, v)
    assert RM.extract_all(acc[None], 4, W).shape == (1, 4, 3, N)


# ---- the coarse mod-switch ----
@pytest.mark.parametrize("N", [64, 1024])
@pytest.mark.parametrize("o", RM.NOUT)
def test_coarse_modswitch_at_its_rounding_edges(N, o):
    nu = RM.nu_of(o)
    bit = 32 - (N.bit_length() - 1) - 1 + nu
    words = RM.sw_edge_words(N, o)
    got = [RM.sw(w, N, o) for w in words]
    assert all(g % o == 0 and 0 <= g <= 2 * N for g in got)
    assert RM.sw(0, N, o) == 0 and RM.sw(0xFFFFFFFF, N, o) == 2 * N
    assert 2 * N in [RM.sw(w, N, o) for w in words[2:]], "a word that rounds up to 2N"
    for m in (0, 1, N // o, 2 * N // o - 1):                               # below the half-way point: down; at it and above: up
        mid = (2 * m + 1) << (bit - 1)
        assert (RM.sw(mid - 1, N, o), RM.sw(mid, N, o), RM.sw(mid + 1, N, o)) == (m * o, (m + 1) * o, (m + 1) * o), m
    if o == 1:                                                             # nu = 0 is the reference's mod-switch word for word
        assert got == [R.btilde(w, N) for w in words]
    # the nearest grid point, ties upwards: exact rational arithmetic on the 32-bit torus
    for w in words + [int(x) for x in np.random.default_rng(N + o).integers(0, 1 << 32, 50)]:
        assert RM.sw(w, N, o) == ((w + (1 << (bit - 1))) >> bit) * o, w


# ---- recipe (a) on the checker ----
def adder_case(p, seed=71):
    """-> (crs, keys, lin, U): pinned keys, the 8 input combinations of three fresh scale-1/16 bits summed with the centre 1/32, and the packed
    (sum, carry) table"""
    from helpers import keygen
    crs, keys = keygen(p, seed)
    x, y, z = R.truth_inputs(p, keys, mk, 7100)
    sv, cv = RM.adder_values(p.W)
    U = mk.lut_pack(np.stack([mk.lut_poly(sv, p), mk.lut_poly(cv, p)]), p)
    return crs, keys, RM.adder_linear(x, y, z), U


@pytest.mark.parametrize("p", [getattr(mk, name) for name in R.CHAIN_SETS], ids=lambda p: p.name)
def test_full_adder_in_one_rotation_decrypts_on_the_checker(p):
    """phase (x + y + z)/16 + 1/32, P = 8, nout = 2: sum = s & 1 and carry = s >> 1 of all 8 input combinations, outputs +-2^(W-3)"""
    crs, keys, lin, U = adder_case(p)
    so = oracle_scheme(p, crs, keys)
    dk = keys if p.multikey else keys[0]
    out = np.stack([RM.checker_many(so, U, lin[v], 2, p.W) for v in range(8)])
    assert out.shape == (8, 2, p.lwe_len)
    s = np.array([bin(v).count("1") for v in range(8)])
    assert np.array_equal(mk.lwe_decrypt(out[:, 0], dk, p), (s & 1).astype(bool)), "sum"
    assert np.array_equal(mk.lwe_decrypt(out[:, 1], dk, p), (s >> 1).astype(bool)), "carry"


# ---- argument checks, with the recording-stub pattern of test_batch_args_cpu.py ----
PARAMS = [mk.CGGIparam.scaled(n=10, N=256), mk.KMS2party.scaled(n=8, N=256)]
B, P, NL, NOUT = 3, 5, 2, 4
ROWS, COUNT, POOL, SOLO, TABLE = "rows", "count", "pool", "solo", "table"


def _specs(p, nout=NOUT):
    Ln, N, rd = p.lwe_len, p.N, p.ring_dtype
    ct = lambda n=B: np.zeros((n, Ln), np.uint32)                       # noqa: E731
    luts = lambda: np.zeros((NL, N), rd)                                # noqa: E731
    sel = lambda: np.zeros(B, np.uint32)                                # noqa: E731
    return {
        "lut_many_testvector": ("lut_many_testvector_batch", [("luts", luts(), TABLE), ("ctxt", ct(), SOLO), ("nout", nout, None), ("sel", sel(), COUNT)], None),
        "lut_extract": ("lut_extract_batch", [("acc", np.zeros((B, p.k + 1, N), rd), SOLO), ("nout", nout, None)], None),
        "lut_many_bootstrap": ("lut_many_bootstrap_batch", [("luts", luts(), TABLE), ("ctxt", ct(), ROWS), ("nout", nout, None), ("sel", sel(), COUNT),
                                                            ("out", ct(B * nout), ROWS)], "out"),
        "lut_many_gather": ("lut_many_batch_gather", [("luts", luts(), TABLE), ("sel", sel(), COUNT), ("pool", ct(P), POOL), ("idx", np.zeros((B, 4), np.uint32), ROWS),
                                                      ("wt", np.zeros((B, 4), np.int8), ROWS), ("cst", np.zeros(B, np.uint32), COUNT), ("nout", nout, None),
                                                      ("out", ct(B * nout), ROWS)], "out"),
    }


def _wrong(a, how, p):
    out = []
    if how in (ROWS, COUNT):
        out += [("one row short", a[:-1].copy()), ("one row long", np.concatenate([a, a[:1]]))]
    if how in (ROWS, POOL, TABLE, SOLO):
        out.append(("one word narrow", np.ascontiguousarray(a[..., :-1])))
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


CASES = [(S.Scheme, "lut_many_testvector"), (S.Scheme, "lut_extract"), (S.Scheme, "lut_many_bootstrap"), (S.Scheme, "lut_many_gather"),
         (S.MultiScheme, "lut_many_bootstrap")]
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
    assert cargs[-2:] == (B, S.MEM_HOST) and NOUT in cargs
    if "luts" in named:
        assert cargs[2] == NL
    if "pool" in named:
        assert cargs[5] == P, "pool rows"
    if ret is not None:
        assert got is named[ret]
    elif method == "lut_extract":
        assert got.shape == (B, NOUT, p.k + 1, p.N) and got.dtype == p.ring_dtype
    else:
        at, acc = got
        assert at.shape == (B, p.lwe_len - 1) and at.dtype == np.uint32 and acc.shape == (B, p.k + 1, p.N) and acc.dtype == p.ring_dtype


@pytest.mark.parametrize("p", PARAMS, ids=lambda p: p.name)
@pytest.mark.parametrize("cls, method", CASES, ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_a_wrongly_sized_buffer_is_refused_before_the_library(lib, cls, method, p):
    sym, args, _ = _specs(p)[method]
    tried = 0
    for name, value, how in args:
        for label, bad in _wrong(value, how, p) if how else []:
            named = {n: v for n, v, _ in args}
            named[name] = bad
            with pytest.raises(ValueError):
                _invoke(cls, p, method, named)
            assert lib.calls == [], (name, label)
            tried += 1
    assert tried


@pytest.mark.parametrize("p", PARAMS, ids=lambda p: p.name)
@pytest.mark.parametrize("cls, method", [c for c in CASES if c[1] in ("lut_many_bootstrap", "lut_many_gather")], ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_out_sized_for_one_output_fewer_is_refused(lib, cls, method, p):
    sym, args, _ = _specs(p)[method]
    named = {n: v for n, v, _ in args}
    named["out"] = np.zeros((B * (NOUT - 1), p.lwe_len), np.uint32)
    with pytest.raises(ValueError):
        _invoke(cls, p, method, named)
    named["out"] = np.zeros((B, NOUT - 1, p.lwe_len), np.uint32)
    with pytest.raises(ValueError):
        _invoke(cls, p, method, named)
    assert lib.calls == []
    named["out"] = np.zeros((B, NOUT, p.lwe_len), np.uint32)               # (inputs, outputs, words) is the same buffer
    assert _invoke(cls, p, method, named) is named["out"] and len(lib.calls) == 1


@pytest.mark.parametrize("nout", [0, 3, 16, -2, 2.0 + 0.5, None])
@pytest.mark.parametrize("cls, method", CASES, ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_a_table_count_that_is_no_power_of_two_up_to_eight_is_refused(lib, cls, method, nout):
    p = PARAMS[0]
    sym, args, _ = _specs(p, nout=2)[method]
    named = {n: v for n, v, _ in args}
    named["nout"] = nout
    with pytest.raises(ValueError):
        _invoke(cls, p, method, named)
    assert lib.calls == []


def test_more_tables_than_coefficients_are_refused(lib):
    p = mk.CGGIparam.scaled(n=4, N=4)
    with pytest.raises(ValueError):
        L.lut_many_bootstrap(_make(S.Scheme, p), np.zeros(4, np.uint32), np.zeros((B, p.lwe_len), np.uint32), 8)
    assert lib.calls == []


def test_defaults_one_table_no_selector(lib):
    """a single (N,) packed table is one row, sel None reaches the library as NULL, out None is a new (..., nout, lwe_len) array"""
    p = PARAMS[0]
    x = np.zeros((2, B, p.lwe_len), np.uint32)
    out = L.lut_many_bootstrap(_make(S.Scheme, p), mk.sign_lut(p), x, 8)
    assert out.shape == (2, B, 8, p.lwe_len) and out.dtype == np.uint32
    name, cargs = lib.calls[0]
    assert name == "mkt_lut_many_bootstrap_batch" and cargs[2] == 1 and cargs[3] is None and cargs[5] == 8 and cargs[-2] == 2 * B
    at, acc = L.lut_many_testvector(_make(S.Scheme, p), mk.sign_lut(p), x, 2)
    assert at.shape == (2, B, p.lwe_len - 1) and acc.shape == (2, B, p.k + 1, p.N)
    assert L.lut_extract(_make(S.Scheme, p), acc, 2).shape == (2, B, 2, p.k + 1, p.N)


def test_the_public_method_sets_are_untouched():
    """the surface is module-level: no public method joined Scheme, MultiScheme or their shared base"""
    for name in ("lut_pack", "lut_many_bootstrap", "lut_many_gather", "lut_many_testvector", "lut_extract"):
        assert not hasattr(S.Scheme, name) and not hasattr(S.MultiScheme, name)
        assert getattr(mk, name) is getattr(L, name)


def test_every_new_symbol_of_the_header_is_declared_to_ctypes_with_its_argument_count():
    hdr = open(os.path.join(ROOT, "include", "mktfhe.h")).read()
    new = ["mkt_lut_many_bootstrap_batch", "mkt_lut_many_batch_gather", "mkt_lut_many_testvector_batch", "mkt_lut_extract_batch", "mkt_multi_lut_many_bootstrap_batch"]
    for name in new:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/mktfhe.h"
        assert name in _lib.SYMBOLS, name
        assert len(_lib.SYMBOLS[name][1]) == m.group(1).count(",") + 1, name
