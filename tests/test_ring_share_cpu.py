"""The surface of the ring share on the GPU (include/mktfhe_ring_share.h), as far as it shows without one: the header, the ctypes table, the
library's export, the Python operator's two routes, the example, the build.  What the device call computes is tests/test_gpu_ring_share.py's."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

from helpers import ROOT, mk, secret_keys

from mktfhe_amd import _lib
from mktfhe_amd import scheme as S

PK = importlib.import_module("mktfhe_amd.pack")      # (mk.pack is the function)
NAME = "mkt_rlwe_partial_decrypt_batch"
HEADER = "mktfhe_ring_share.h"


def header_symbols(name):
    """tests/test_pack_cpu.py header_symbols restated: every mkt_ name a header declares, comments dropped"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(mkt_\w+)\s*\(", text))


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_table_and_export_hold_the_new_name():
    """declared in the NEW header with the argument count _lib binds, in RING_SHARE_SYMBOLS and in no other table, exported; the two older
    headers still equal their tables, so the new entry point is in neither; MKT_ABI_VERSION stays 3"""
    hdr = read("include", HEADER)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{NAME} is not declared in include/{HEADER}"
    assert set(_lib.RING_SHARE_SYMBOLS) == header_symbols(HEADER) == {NAME}
    res, args = _lib.RING_SHARE_SYMBOLS[NAME]
    assert res is C.c_int and len(args) == len(m.group(1).split(",")) == 10
    assert args == _lib.SYMBOLS["mkt_partial_decrypt_batch"][1], "the argument kinds of the LWE share's device call"
    fn = getattr(_lib.lib(), NAME)
    assert fn.argtypes == args and fn.restype is res
    assert header_symbols("mktfhe.h") == set(_lib.SYMBOLS) and header_symbols("mktfhe_pack.h") == set(_lib.PACK_SYMBOLS)
    assert not set(_lib.RING_SHARE_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.PACK_SYMBOLS))
    assert '#include "mktfhe_pack.h"' in hdr and "MKT_ABI_VERSION" in hdr and not re.search(r"#define\s+MKT_ABI_VERSION", hdr)
    assert _lib.lib().mkt_abi_version() == 3


def test_header_carries_the_trust_paragraph_and_the_seed_rule():
    hdr = " ".join(read("include", HEADER).replace("*", " ").split())
    assert "A SEED MUST NEVER SERVE TWO DIFFERENT CIPHERTEXTS AT ONE PACK INDEX" in hdr
    assert "TRUST: as mkt_partial_decrypt_batch" in hdr and "SECRET ring key(s)" in hdr and "party-local operation" in hdr
    assert "zeroed on the device before they are freed" in hdr and "kernel-argument segment" in hdr
    assert "NOT HERE" in hdr and "this header supplies that item" in hdr
    for word in ("MKT_ERR_ARG", "G == 0 succeeds", "no word written and nothing launched", "needs the alignment of its element type", "a fork"):
        assert word in hdr, word
    pack = read("include", "mktfhe_pack.h")
    assert "the ring share on the GPU" in pack[pack.index("NOT HERE"):], "mktfhe_pack.h stays as it is"


HOST_SETS = [mk.KMS2party.scaled(n=5, N=64, k=3), mk.CGGIparam.scaled(n=5, N=32, k=2, W=32), mk.CCS2party.scaled(n=5, N=64)]


@pytest.mark.parametrize("p", HOST_SETS, ids=lambda p: f"{p.name}-N{p.N}-k{p.k}-W{p.W}")
def test_scheme_none_returns_the_words_of_the_host_function(p):
    """mk.rlwe_partial_decrypt(..., scheme=None), and the call without the argument, against mkt_client_rlwe_partial_decrypt called directly"""
    keys = secret_keys(p, seed=23)
    rng = np.random.default_rng(p.N)
    ct = rng.integers(0, 2**63, (3, p.k + 1, p.N), dtype=np.uint64).astype(p.ring_dtype)
    seed = bytes(range(7, 39))
    for party in range(p.nparty):
        want = np.full((3, p.N), 0xA5, dtype=p.ring_dtype)
        r = _lib.lib().mkt_client_rlwe_partial_decrypt(C.byref(p.c()), keys[party].h, party, S._np_ptr(ct), 2.0 ** 20, (C.c_uint8 * 32)(*seed), 2**32 - 1,
                                                       S._np_ptr(want), 3)
        assert r == 0
        for kw in (dict(scheme=None), dict()):
            got = mk.rlwe_partial_decrypt(ct, keys[party], p, party, 2.0 ** 20, deterministic_seed=seed, row0=2**32 - 1, **kw)
            assert got.dtype == p.ring_dtype and got.shape == (3, p.N) and np.array_equal(got, want), (party, kw)
    one = mk.rlwe_partial_decrypt(ct[1], keys[0], p, 0, 0.0)
    assert one.shape == (p.N,) and np.array_equal(one, mk.rlwe_partial_decrypt(ct, keys[0], p, 0, 0.0)[1])
    sig = inspect.signature(mk.rlwe_partial_decrypt)
    assert sig.parameters["scheme"].default is None and mk.rlwe_partial_decrypt is PK.rlwe_partial_decrypt


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("mkt_"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


def test_the_device_route_goes_through_the_checked_call(monkeypatch):
    """scheme= reaches mkt_rlwe_partial_decrypt_batch through Scheme._call with the header's argument count, G packs and the memory kind of
    the arrays, and never the host function; input that is not (G, 1 + k, N) or (1 + k, N) never reaches the library (a recording stub)"""
    p = mk.KMS2party.scaled(n=5, N=64)
    keys = secret_keys(p, seed=23)
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    sch = object.__new__(S.Scheme)
    sch.params, sch.device, sch.h, sch._user_stream, sch._owned = p, 0, C.c_void_p(1), True, False
    ct = np.zeros((5, p.k + 1, p.N), dtype=p.ring_dtype)
    out = mk.rlwe_partial_decrypt(ct, keys[1], p, 1, 3.0, deterministic_seed=4, row0=2**40, scheme=sch)
    (name, args), = [c for c in rec.calls if "rlwe" in c[0]]
    assert name == NAME and out.shape == (5, p.N) and out.dtype == p.ring_dtype
    assert len(args) == len(_lib.RING_SHARE_SYMBOLS[NAME][1]) and args[1] == 1 and args[4] == 3.0 and args[6] == 2**40 and args[-2:] == (5, S.MEM_HOST)
    assert mk.rlwe_partial_decrypt(ct[0], keys[1], p, 1, 0.0, scheme=sch).shape == (p.N,) and rec.calls[-1][1][-2:] == (1, S.MEM_HOST)
    n = len(rec.calls)
    for bad in (ct[:, :2], ct[..., :-1], ct.reshape(1, 5, p.k + 1, p.N)):
        with pytest.raises(ValueError):
            mk.rlwe_partial_decrypt(bad, keys[1], p, 1, 3.0, scheme=sch)
    with pytest.raises(ValueError):
        mk.rlwe_partial_decrypt(ct, keys[1], p, 1, 3.0, row0=2**64, scheme=sch)
    assert len(rec.calls) == n


def test_example_calls_only_declared_symbols():
    src = re.sub(r"/\*.*?\*/", "", read("examples", "ring_share_gpu.c"), flags=re.S)
    called = set(re.findall(r"\b(mkt_\w+)\s*\(", src))
    assert called <= header_symbols("mktfhe.h") | header_symbols("mktfhe_pack.h") | header_symbols(HEADER)
    assert {"mkt_gate_batch", "mkt_pack_batch", NAME, "mkt_client_rlwe_merge_decrypt"} <= called and "mkt_client_rlwe_partial_decrypt" not in called
    assert '#include "mktfhe_ring_share.h"' in src


def test_build_covers_the_kernel_and_the_kernel_keeps_its_rules():
    """the Makefile links ring_share.o and hashes the new header into the build id; ring_share.hip holds no inline assembly and no atomic,
    reaches the noise through the shared generator, and its grid cap is a named constant (the GPU test reads it); the host definition and the
    stream ids are untouched"""
    mkf = read("mktfhe_amd", "csrc", "Makefile")
    assert "$(B)/ring_share.o" in mkf.split("\nOBJ =")[1].split("\n")[0] and "../../include/" + HEADER in mkf.split("SRCS_ALL =")[1].split("\n")[0]
    assert re.search(r"\$\(B\)/ring_share\.o:.*keygen_common\.h.*rng_chacha\.h", mkf) and "-ffp-contract=off" in mkf
    src = read("mktfhe_amd", "csrc", "ring_share.hip")
    code = re.sub(r"//[^\n]*", "", src)
    assert "asm" not in code and "atomic" not in code and "fill_noise(" in code and "STREAM_PACK_SMUDGE" in code
    assert re.search(r"constexpr unsigned RS_MAX_GRID = \d+;", src)
    api = read("mktfhe_amd", "csrc", "device_api.h")
    assert "struct RingShareArgs" in api and "launch_ring_share(" in api
    rng = read("mktfhe_amd", "csrc", "rng_chacha.h")
    assert max(int(v) for v in re.findall(r"constexpr uint32_t STREAM_\w+ = (\d+);", rng)) == 20, "no stream id was added"
    ctx = read("mktfhe_amd", "csrc", "context.cpp")
    body = ctx[ctx.index("int " + NAME):]
    body = body[:body.index("\n}\n")]
    for word in ("DevGuard", "Timer whole(c, 0)", "Staged", "DeviceSecret", "seed_to_key", "wipe_secrets", "hipfail", "mem_ok(mem)"):
        assert word in body, word
    assert "ws." not in body and "last_kernel" not in body, "the gate workspace and mkt_last_kernel_name are left alone"
