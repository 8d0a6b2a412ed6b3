"""Argument checks of every batch method of Scheme and MultiScheme, on the CPU.  The C ABI takes plain pointers and a batch count B,
so the Python layer is the only place where a buffer's size is compared with what the library reads or writes.  Here the library is a
recording stub: a correct call reaches exactly one symbol with the expected B, and a buffer one row short, one row long or with a
wrong row length is refused with ValueError before any library call."""
import numpy as np
import pytest

from helpers import mk
from mktfhe_amd import _lib
from mktfhe_amd import scheme as S

PARAMS = [mk.CGGIparam.scaled(n=10, N=256), mk.KMS2party.scaled(n=8, N=256)]     # a 32-bit ring, a KMS 64-bit ring
B, P = 3, 5                                                                      # gates, pool rows

# how a buffer can be wrong: ROWS = one row short, one row long or a wrong row length; COUNT = one element short or long (one per
# gate); POOL and SOLO (the only input: it sets B) = a wrong row length only
ROWS, COUNT, POOL, SOLO = "rows", "count", "pool", "solo"

SHARED = ["gate", "gate_ops", "gate3", "gate3_ops", "mux", "bootstrapping_", "not_", "blindrotate_", "keyswitch"]
SCHEME_ONLY = ["gate_gather", "gate3_gather", "mux_gather", "modswitch", "kms_phase1", "transform_fwd", "transform_inv", "exact_polymul",
               "decompose"]


def _specs(p):
    """method -> (symbol without its prefix, [(name, argument, how it can be wrong)] in call order, the name of the argument returned)"""
    L, N, rd = p.lwe_len, p.N, p.ring_dtype
    ct = lambda n=B: np.zeros((n, L), np.uint32)                        # noqa: E731
    each = lambda dt=np.uint32: np.zeros(B, dt)                         # noqa: E731
    poly = lambda: np.zeros((B, N), rd)                                 # noqa: E731
    trans = lambda: np.zeros((B, N // 2), np.complex128)                # noqa: E731
    atilde = lambda: np.zeros((B, L - 1), np.uint32)                    # noqa: E731
    acc = lambda: np.zeros((B, p.k + 1, N), rd)                         # noqa: E731
    return {
        "gate": ("gate_batch", [("op", 0, None), ("x", ct(), ROWS), ("y", ct(), ROWS), ("out", ct(), ROWS)], "out"),
        "gate_ops": ("gate_batch_ops", [("ops", each(np.uint8), COUNT), ("x", ct(), ROWS), ("y", ct(), ROWS), ("out", ct(), ROWS)], "out"),
        "gate3": ("gate3_batch_ops", [("op", 0, None), ("x", ct(), ROWS), ("y", ct(), ROWS), ("z", ct(), ROWS), ("out", ct(), ROWS)], "out"),
        "gate3_ops": ("gate3_batch_ops", [("ops", each(np.uint8), COUNT), ("x", ct(), ROWS), ("y", ct(), ROWS), ("z", ct(), ROWS),
                                          ("out", ct(), ROWS)], "out"),
        "mux": ("mux_batch", [("s", ct(), ROWS), ("a", ct(), ROWS), ("b", ct(), ROWS), ("out", ct(), ROWS)], "out"),
        "bootstrapping_": ("bootstrap_batch", [("ctxt", ct(), SOLO)], "ctxt"),
        "not_": ("not_batch", [("ctxt", ct(), SOLO)], "ctxt"),
        "blindrotate_": ("blindrotate_batch", [("atilde", atilde(), ROWS), ("acc", acc(), ROWS)], "acc"),
        "keyswitch": ("keyswitch_batch", [("acc", acc(), SOLO)], None),
        "gate_gather": ("gate_batch_gather", [("ops", each(np.uint8), COUNT), ("pool", ct(P), POOL), ("ix", each(), COUNT), ("iy", each(), COUNT),
                                              ("out", ct(), ROWS)], "out"),
        "gate3_gather": ("gate3_batch_gather", [("ops", each(np.uint8), COUNT), ("pool", ct(P), POOL), ("ix", each(), COUNT), ("iy", each(), COUNT),
                                                ("iz", each(), COUNT), ("out", ct(), ROWS)], "out"),
        "mux_gather": ("mux_batch_gather", [("pool", ct(P), POOL), ("i_s", each(), COUNT), ("i_a", each(), COUNT), ("i_b", each(), COUNT),
                                            ("out", ct(), ROWS), ("not_ab", each(np.uint8), COUNT)], "out"),
        "modswitch": ("modswitch_batch", [("ctxt", ct(), SOLO)], None),
        "kms_phase1": ("kms_phase1_batch", [("atilde", atilde(), SOLO)], None),
        "transform_fwd": ("transform_fwd_batch", [("p", poly(), ROWS), ("out", trans(), ROWS)], "out"),
        "transform_inv": ("transform_inv_batch", [("t", trans(), ROWS), ("out", poly(), ROWS)], "out"),
        "exact_polymul": ("exact_polymul_batch", [("a", poly(), ROWS), ("b", poly(), ROWS), ("out", poly(), ROWS)], "out"),
        "decompose": ("decompose_batch", [("p", poly(), SOLO), ("l", 2, None), ("logB", 4, None)], None),
    }


def _wrong(a, how):
    """(label, variant) pairs of a buffer that must be refused"""
    out = []
    if how in (ROWS, COUNT):
        out += [("one row short", a[:-1].copy()), ("one row long", np.concatenate([a, a[:1]]))]
    if how in (ROWS, POOL, SOLO):
        out.append(("wrong row length", np.ascontiguousarray(a[..., :-1])))
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
    """an evaluator with no context behind it (h None: closing it calls nothing), as MultiScheme.shard builds its views"""
    s = object.__new__(cls)
    s.params, s.h, s.arith = p, None, S.ARITH_F64REF
    if cls is S.Scheme:
        s.device, s._user_stream = 0, False
    return s


CASES = [(S.Scheme, m) for m in SHARED + SCHEME_ONLY] + [(S.MultiScheme, m) for m in SHARED]
PREFIX = {S.Scheme: "mkt_", S.MultiScheme: "mkt_multi_"}


def test_cases_cover_every_batch_method():
    """a new batch method of either class has to join this file; MultiScheme has no method the multi ABI lacks"""
    other = {"close", "fork", "load_party", "keygen_device", "brk_words", "get_ksk_shape", "get_ksk", "load_crs", "set_stream", "synchronize",
             "get_stream", "set_option", "get_metric", "last_kernel_name", "twiddles", "monomial", "enable_timing", "kernel_ms",
             "nshards", "shard_range", "shard", "replicate"}
    for cls in (S.Scheme, S.MultiScheme):
        public = {n for n in dir(cls) if not n.startswith("_")} - other
        assert public == {m for c, m in CASES if c is cls}, cls.__name__


@pytest.mark.parametrize("p", PARAMS, ids=lambda p: p.name)
@pytest.mark.parametrize("cls, method", CASES, ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_a_correct_call_reaches_one_symbol_with_its_batch(lib, cls, method, p):
    sym, args, ret = _specs(p)[method]
    named = {n: v for n, v, _ in args}
    got = getattr(_make(cls, p), method)(*named.values())
    name = PREFIX[cls] + sym
    assert [c[0] for c in lib.calls] == [name]
    cargs = lib.calls[0][1]
    assert len(cargs) == len(_lib.SYMBOLS[name][1]), "argument count of the ABI symbol"
    assert cargs[-2:] == (B, S.MEM_HOST)
    if "pool" in named:
        assert P in cargs, "pool rows"
    if ret is not None:
        assert got is named[ret]


@pytest.mark.parametrize("p", PARAMS, ids=lambda p: p.name)
@pytest.mark.parametrize("cls, method", CASES, ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_a_wrongly_sized_buffer_is_refused_before_the_library(lib, cls, method, p):
    sym, args, _ = _specs(p)[method]
    tried = 0
    for i, (name, value, how) in enumerate(args):
        for label, bad in _wrong(value, how) if how else []:
            call = [v for _, v, _ in args]
            call[i] = bad
            with pytest.raises(ValueError):
                getattr(_make(cls, p), method)(*call)
            assert lib.calls == [], (name, label)
            tried += 1
    assert tried


@pytest.mark.parametrize("p", PARAMS, ids=lambda p: p.name)
def test_default_outputs_take_the_shape_the_call_writes(lib, p):
    s = _make(S.Scheme, p)
    x = np.zeros((2, B, p.lwe_len), np.uint32)
    assert s.gate(0, x, x).shape == x.shape and s.gate3(0, x, x, x).shape == x.shape and s.mux(x, x, x).shape == x.shape
    assert s.gate_ops(np.zeros((2, B), np.uint8), x, x).shape == x.shape
    poly = np.zeros((B, p.N), p.ring_dtype)
    t = s.transform_fwd(poly)
    assert t.shape == (B, p.N // 2) and t.dtype == np.complex128
    assert s.transform_inv(t).shape == poly.shape and s.exact_polymul(poly, poly).shape == poly.shape
    assert [c[1][-2] for c in lib.calls] == [2 * B] * 4 + [B] * 3


@pytest.mark.parametrize("cls", [S.Scheme, S.MultiScheme], ids=lambda c: c.__name__)
def test_keyswitch_refuses_a_flat_accumulator(lib, cls):
    """a (B, (k+1) N) accumulator was once read as ONE ciphertext; blindrotate_ takes it (element count only), keyswitch does not"""
    p = PARAMS[1]
    flat = np.zeros((B, (p.k + 1) * p.N), p.ring_dtype)
    s = _make(cls, p)
    with pytest.raises(ValueError):
        s.keyswitch(flat)
    assert lib.calls == []
    s.blindrotate_(np.zeros((B, p.lwe_len - 1), np.uint32), flat)
    assert lib.calls[0][1][-2] == B


def test_mux_gather_without_flags_passes_null(lib):
    p = PARAMS[0]
    e = np.zeros(B, np.uint32)
    _make(S.Scheme, p).mux_gather(np.zeros((P, p.lwe_len), np.uint32), e, e, e, np.zeros((B, p.lwe_len), np.uint32))
    assert lib.calls[0][1][6] is None
