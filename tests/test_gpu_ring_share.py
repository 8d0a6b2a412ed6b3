"""Ring shares of packed results on the party's GPU (include/mktfhe_ring_share.h; mktfhe_amd/csrc/ring_share.hip): the device call gives the
words of mkt_client_rlwe_partial_decrypt for the same arguments, word for word -- wrapping integer arithmetic, one ChaCha20 block function
and the shared box_muller with contraction off on both sides, so every comparison is exact --; gates -> pack -> device shares -> merge opens
the plaintext bits, on a fork and on an MKT_ARITH_EXACT context too; the refusals write nothing; the call writes only share_out; it is
ordered on the context's stream; the C example.

The shapes are those at which the kernel's indexing changes, not workload sizes.  A pack is dealt over `slices` workgroups by slices of
L = N / slices output coefficients (ring_share_slices, restated below from the source's constants): G = 1 and 3 run L = 16 at every ring size,
G one over the grid cap at N = 32 runs L = 32 and the stride loop, and test_every_slice_width runs L = 32 .. 256."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import footprint as F
import helpers
import stream_cases as SC
from helpers import GATE_FUNCS, ROOT, encrypt_bits, gpu_scheme, host_words, keygen, mk, same_words, secret_keys, to_mem

from mktfhe_amd import _lib
from mktfhe_amd import scheme as S

pytestmark = pytest.mark.gpu

H, D = mk.MEM_HOST, mk.MEM_DEVICE
ARG = -1
FILL = 0xA5
SEED = bytes(range(90, 122))
ROW0S = (0, 2**32 - 1)                          # with G >= 2 the pack index crosses into the high nonce word
SIGMAS = (0.0, 2.0 ** 20, 2.0 ** 31)
_SRC = open(os.path.join(ROOT, "mktfhe_amd", "csrc", "ring_share.hip")).read()
_KG = open(os.path.join(ROOT, "mktfhe_amd", "csrc", "keygen_common.h")).read()


def _const(name, text=_SRC):
    return int(re.search(r"constexpr (?:unsigned|int) %s = (\d+);" % name, text).group(1))


MAX_GRID, RS_FILL, MIN_SLICE, THREADS = _const("RS_MAX_GRID"), _const("RS_FILL"), _const("RS_MIN_SLICE"), _const("KG_THREADS", _KG)


def slices(N, G):
    """ring_share.hip ring_share_slices restated"""
    s, hi = max(N // THREADS, 1), N // MIN_SLICE
    while s < hi and G * s < RS_FILL:
        s *= 2
    return s


def sid(p):
    return f"{p.name}-N{p.N}-k{p.k}-W{p.W}"


SETS = [mk.CGGIparam.scaled(n=5, N=N, k=kr, W=W) for N in (32, 256, 512, 4096) for W in (32, 64) for kr in (1, 3)] + [
    mk.KMS2party.scaled(n=5, N=1024, k=3),               # every party: the slot rule, the uni key
    mk.CCS2party.scaled(n=5, N=2048),                    # key 0
    mk.KMS2partyblock.scaled(n=6, N=4096, blk_d=2),
    mk.Blockparam.scaled(n=6, N=32, blk_d=2),
]
SMALLEST, LARGEST = SETS[0], SETS[15]
assert (SMALLEST.N, SMALLEST.W, SMALLEST.k) == (32, 32, 1) and (LARGEST.N, LARGEST.W, LARGEST.k) == (4096, 64, 3)


def u8(b):
    return (C.c_uint8 * 32)(*b)


def host_share(p, key, party, ct, sigma, row0, seed=SEED):
    """mkt_client_rlwe_partial_decrypt called directly: the definition"""
    ct = np.ascontiguousarray(ct, dtype=p.ring_dtype)
    out = np.empty((ct.shape[0], p.N), dtype=p.ring_dtype)
    assert _lib.lib().mkt_client_rlwe_partial_decrypt(C.byref(p.c()), key.h, party, S._np_ptr(ct), float(sigma), u8(seed), row0, S._np_ptr(out), ct.shape[0]) == 0
    return out


def input_batches(p, rng):
    """three batches of three packs: uniform ring words; every word 2^W - 1; the monomial ciphertexts -- one non-zero coefficient at 0, 1 and
    N - 1 of every mask polynomial, which place the negacyclic sign and the wrap"""
    shape = (3, p.k + 1, p.N)
    uni = (rng.integers(0, 2**63, shape, dtype=np.uint64) * 2 + rng.integers(0, 2, shape, dtype=np.uint64)).astype(p.ring_dtype)
    ones = np.full(shape, 2**p.W - 1, dtype=p.ring_dtype)
    mono = np.zeros(shape, dtype=p.ring_dtype)
    for g, at in enumerate((0, 1, p.N - 1)):
        mono[g, 1:, at] = uni[g, 1:, at] | 1
    return {"uniform": uni, "ones": ones, "monomials": mono}


def offset_tensor(a, fill=None):
    """-> (owner, view): a device tensor of a's words that starts ONE ELEMENT into its allocation (bare 4- or 8-byte alignment), FILL bytes
    round it (fill given: the view holds FILL bytes too -- an output); 8 elements behind the view belong to the owner"""
    import torch
    a = np.ascontiguousarray(a)
    whole = np.empty(a.size + 9, dtype=a.dtype)
    whole.view(np.uint8)[...] = FILL
    if fill is None:
        whole[1:1 + a.size] = a.reshape(-1)
    t = torch.from_numpy(helpers._signed(whole)).cuda()
    view = t[1:1 + a.size].view(a.shape)
    assert view.data_ptr() == t.data_ptr() + a.dtype.itemsize and view.data_ptr() % 16 != 0
    return t, view


def device_share(sch, p, key, party, ct, sigma, row0, seed=SEED):
    """the raw call on device tensors at bare element alignment -> host words; the elements round the output keep their fill"""
    tin, vin = offset_tensor(ct)
    out_shape = (ct.shape[0], p.N)
    tout, vout = offset_tensor(np.empty(out_shape, dtype=p.ring_dtype), fill=True)
    r = _lib.lib().mkt_rlwe_partial_decrypt_batch(sch.h, party, key.h, C.c_void_p(vin.data_ptr()), float(sigma), u8(seed), row0, C.c_void_p(vout.data_ptr()),
                                                  ct.shape[0], D)
    assert r == 0, (_lib.lib().mkt_last_error(sch.h) or b"").decode()
    whole = host_words(tout)
    n = ct.shape[0] * p.N
    assert (whole[:1].view(np.uint8) == FILL).all() and (whole[1 + n:].view(np.uint8) == FILL).all(), "an element beside share_out was written"
    assert same_words(host_words(tin)[1:1 + ct.size].reshape(ct.shape), ct), "the input was written"
    return whole[1:1 + n].reshape(out_shape)


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return None if not len(bad) else (tuple(bad[0]), hex(int(got[tuple(bad[0])])), hex(int(want[tuple(bad[0])])), len(bad))


# ---- 1: device equals host, word for word ----
@pytest.mark.parametrize("p", SETS, ids=sid)
def test_device_share_equals_host_share(require_gpu, p):
    """every party, every input batch, row0 in ROW0S, sigma in SIGMAS: the host function once at G = 3; the device call at G = 3 and at G = 1 on
    each of the three packs (pack j at row0 + j: the same noise stream), on host arrays through the operator and on device tensors one element
    into their allocation through the raw call.  The context holds no key"""
    keys = secret_keys(p, seed=29)
    sch = mk.Scheme(p)
    try:
        for party in range(p.nparty):
            for name, ct in input_batches(p, np.random.default_rng(p.N + p.W + party)).items():
                for row0 in ROW0S:
                    for sigma in SIGMAS:
                        want = host_share(p, keys[party], party, ct, sigma, row0)
                        what = (party, name, row0, sigma)
                        got = mk.rlwe_partial_decrypt(ct, keys[party], p, party, sigma, deterministic_seed=SEED, row0=row0, scheme=sch)
                        assert isinstance(got, np.ndarray) and got.dtype == p.ring_dtype and got.shape == (3, p.N)
                        assert first_difference(got, want) is None, (what, "host arrays, G = 3", first_difference(got, want))
                        got = device_share(sch, p, keys[party], party, ct, sigma, row0)
                        assert first_difference(got, want) is None, (what, "device tensors, G = 3", first_difference(got, want))
                        for j in range(3):
                            r = (row0 + j) % 2**64
                            got = mk.rlwe_partial_decrypt(ct[j], keys[party], p, party, sigma, deterministic_seed=SEED, row0=r, scheme=sch)
                            assert got.shape == (p.N,) and first_difference(got, want[j]) is None, (what, "host arrays, G = 1, pack", j)
                            got = device_share(sch, p, keys[party], party, ct[j:j + 1], sigma, r)
                            assert first_difference(got[0], want[j]) is None, (what, "device tensors, G = 1, pack", j)
        if p.multikey and p.nparty > 1:
            ct = input_batches(p, np.random.default_rng(1))["uniform"]
            a, b = (host_share(p, keys[i], i, ct, 0.0, 0) for i in (0, 1))
            assert (a != b).any(), "two parties' shares of one ciphertext differ: the slot rule and the keys are the parties' own"
    finally:
        sch.close()


@pytest.mark.parametrize("W", (32, 64))
def test_one_pack_more_than_the_grid_cap(require_gpu, W):
    """N = 32, G = RS_MAX_GRID + 1: one slice per pack, one (pack, slice) pair more than the launch has workgroups -- the stride loop runs"""
    p = mk.CGGIparam.scaled(n=5, N=32, k=3, W=W)
    G = MAX_GRID + 1
    assert slices(p.N, G) == 1 and G * slices(p.N, G) > MAX_GRID
    key = secret_keys(p, seed=29)[0]
    rng = np.random.default_rng(W)
    ct = (rng.integers(0, 2**63, (G, p.k + 1, p.N), dtype=np.uint64) * 2 + 1).astype(p.ring_dtype)
    sch = mk.Scheme(p)
    try:
        for row0 in ROW0S:
            want = host_share(p, key, 0, ct, 2.0 ** 20, row0)
            got = mk.rlwe_partial_decrypt(ct, key, p, 0, 2.0 ** 20, deterministic_seed=SEED, row0=row0, scheme=sch)
            assert first_difference(got, want) is None, ("host arrays", row0, first_difference(got, want))
            got = device_share(sch, p, key, 0, ct, 2.0 ** 20, row0)
            assert first_difference(got, want) is None, ("device tensors", row0, first_difference(got, want))
    finally:
        sch.close()


WIDTH_CASES = [(256, 32, 64), (256, 64, 128), (256, 32, 256), (256, 64, 512), (4096, 64, 64), (1024, 32, 32)]      # (N, W, G)


def test_every_slice_width(require_gpu):
    """the slice widths G = 1 and 3 do not reach: L = 32, 64, 128, 256 at N = 256 (16, 8, 4, 2, 1 parts of the key walk per coefficient), the
    widest slice at N = 4096 and an inner one at N = 1024"""
    widths = {N // slices(N, G) for N, _, G in WIDTH_CASES} | {N // slices(N, 1) for N in (32, 4096)}
    assert widths == {16, 32, 64, 128, 256}, widths
    for N, W, G in WIDTH_CASES:
        p = mk.CGGIparam.scaled(n=5, N=N, k=2, W=W)
        key = secret_keys(p, seed=31)[0]
        rng = np.random.default_rng(G)
        ct = (rng.integers(0, 2**63, (G, p.k + 1, p.N), dtype=np.uint64) * 2 + 1).astype(p.ring_dtype)
        sch = mk.Scheme(p)
        try:
            want = host_share(p, key, 0, ct, 2.0 ** 31, 2**32 - 2)
            got = device_share(sch, p, key, 0, ct, 2.0 ** 31, 2**32 - 2)
            assert first_difference(got, want) is None, (N, W, G, N // slices(N, G), first_difference(got, want))
        finally:
            sch.close()


# ---- 2: end to end ----
def _dev32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def test_gates_pack_device_shares_merge(require_gpu):
    """the smallest multi-key set: NANDs, packed; every party's shares made on a context of its own that holds no key.  sigma 0: the merged
    phase is mkt_client_rlwe_phase word for word; sigma 2^20: the merged bits are the plain gate outputs (the zero-failure condition at the top
    of tests/test_pack_cpu.py for this set and gadget); NULL seed: two calls differ at sigma > 0 and agree at sigma 0.  The same words come
    from a fork and from an MKT_ARITH_EXACT context"""
    p, (l, logB) = mk.KMS2party.scaled(n=16, N=256), (4, 4)
    N = p.N
    crs, keys = keygen(p, 5)
    ev = gpu_scheme(p, crs, keys)
    for i in range(p.nparty):
        mk.load_packing_key(ev, i, mk.packing_keygen(keys[i], p, l, logB, deterministic_seed=40 + i), l, logB)
    B = N + 3
    bits = np.random.default_rng(8).integers(0, 2, 2 * B).astype(bool)
    c = encrypt_bits(p, keys, bits, seed=500)
    packed = mk.pack(ev, mk.NAND(_dev32(c[0::2]), _dev32(c[1::2]), ev))
    assert packed.is_cuda and tuple(packed.shape) == (2, p.k + 1, N)
    ev.close()
    hp = host_words(packed)
    phase = mk.rlwe_phase(hp, keys, p)
    own = mk.Scheme(p)
    fork = own.fork()
    exact = mk.Scheme(p, arith=mk.ARITH_EXACT)
    try:
        for sch in (own, fork, exact):
            zero = [mk.rlwe_partial_decrypt(packed, keys[i], p, i, 0.0, scheme=sch) for i in range(p.nparty)]
            assert all(s.is_cuda and tuple(s.shape) == (2, N) for s in zero)
            for g in range(2):
                assert np.array_equal(mk.rlwe_merge_phase(hp[g], [host_words(s)[g] for s in zero], p), phase[g]), ("sigma 0: merged phase", g)
            noisy = [mk.rlwe_partial_decrypt(packed, keys[i], p, i, 2.0 ** 20, scheme=sch) for i in range(p.nparty)]
            got = np.concatenate([mk.rlwe_merge_decrypt(hp[g], [host_words(s)[g] for s in noisy], p) for g in range(2)])[:B]
            assert np.array_equal(got, GATE_FUNCS[0](bits[0::2], bits[1::2])), "wrong bits after gates, pack, device shares and merge"
            again = mk.rlwe_partial_decrypt(packed, keys[0], p, 0, 2.0 ** 20, scheme=sch)
            assert (host_words(again) != host_words(noisy[0])).mean() > 0.99, "a NULL seed must draw fresh entropy per call"
            assert same_words(host_words(mk.rlwe_partial_decrypt(packed, keys[0], p, 0, 0.0, scheme=sch)), host_words(zero[0]))
            for i in range(p.nparty):
                pinned = mk.rlwe_partial_decrypt(packed, keys[i], p, i, 2.0 ** 20, deterministic_seed=SEED, row0=2**32 - 1, scheme=sch)
                assert same_words(host_words(pinned), host_share(p, keys[i], i, hp, 2.0 ** 20, 2**32 - 1)), ("the host's words", i)
        with pytest.raises(mk.MktError) as ei:
            mk.pack(own, np.zeros((1, p.lwe_len), dtype=np.uint32))
        assert ei.value.code == -5, "the share contexts never held a key"
    finally:
        fork.close(); own.close(); exact.close()


# ---- 3: refusals ----
@pytest.mark.parametrize("mem", (H, D), ids=("host", "device"))
def test_refusals_write_nothing(require_gpu, mem):
    p, q = mk.KMS2party.scaled(n=5, N=64), mk.CCS2party.scaled(n=5, N=256)
    keys, foreign = secret_keys(p, seed=29), secret_keys(q, seed=29)
    L = _lib.lib()
    G = 2
    ct = input_batches(p, np.random.default_rng(3))["uniform"][:G]
    sch = mk.Scheme(p)
    if mem == D:
        tin, vin = offset_tensor(ct)
        tout, vout = offset_tensor(np.empty((G, p.N), dtype=p.ring_dtype), fill=True)
        src, dst = vin.data_ptr(), vout.data_ptr()
        untouched = lambda: (host_words(tout).view(np.uint8) == FILL).all()      # noqa: E731
    else:
        out = np.empty((G, p.N), dtype=p.ring_dtype)
        out.view(np.uint8)[...] = FILL
        src, dst = ct.ctypes.data, out.ctypes.data
        untouched = lambda: (out.view(np.uint8) == FILL).all()      # noqa: E731

    def call(party=0, k=keys[0], rlwe=src, sigma=2.0 ** 20, o=dst, g=G, m=mem):
        return L.mkt_rlwe_partial_decrypt_batch(sch.h, party, None if k is None else k.h, C.c_void_p(rlwe) if rlwe else None, sigma, u8(SEED), 0,
                                                C.c_void_p(o) if o else None, g, m)

    try:
        for kw in (dict(party=2), dict(party=-1), dict(party=1), dict(k=keys[1]), dict(k=foreign[0]), dict(k=None), dict(sigma=-1.0), dict(sigma=2.0 ** 31 + 1.0),
                   dict(sigma=float("nan")), dict(sigma=float("inf")), dict(rlwe=0), dict(o=0), dict(m=7)):
            assert call(**kw) == ARG, kw
            assert untouched(), kw
        assert call(g=0) == 0 and call(g=0, rlwe=0, o=0) == 0 and untouched(), "G == 0 succeeds and writes nothing"
        assert call(g=0, sigma=-1.0) == ARG and call(g=0, m=7) == ARG, "the refusals come before the count"
        assert call() == 0 and not untouched()
        got = host_words(tout)[1:1 + G * p.N].reshape(G, p.N) if mem == D else out
        assert same_words(got, host_share(p, keys[0], 0, ct, 2.0 ** 20, 0))
    finally:
        sch.close()


# ---- 4: footprint ----
@pytest.mark.parametrize("layout", F.LAYOUTS)
@pytest.mark.parametrize("p", (SMALLEST, LARGEST), ids=sid)
def test_the_call_writes_only_share_out(require_gpu, p, layout):
    """the call's device tensors carved from the arena of tests/footprint.py, at 256-byte and at bare element alignment: no guard byte and no
    byte of the packs changes"""
    import torch
    key = secret_keys(p, seed=29)[0]
    arena = F.Arena(4 << 20, layout)
    sch = mk.Scheme(p)
    try:
        for G in (1, 3):
            ct = input_batches(p, np.random.default_rng(G))["uniform"][:G]
            arena.reset()
            with F.tensors_in(arena):
                out = mk.rlwe_partial_decrypt(helpers.device_tensor(ct), key, p, 0, 2.0 ** 20, deterministic_seed=SEED, scheme=sch)
            torch.cuda.synchronize()
            assert len(arena.carvings) == 2 and (layout == "aligned" or any((arena.base + c.offset) % 16 for c in arena.carvings))
            assert arena.check(written=out) == [], (G, arena.check(written=out))
            assert same_words(host_words(out), host_share(p, key, 0, ct, 2.0 ** 20, 0))
    finally:
        sch.close()


def _guard_child():
    """under MKT_MEM_GUARD: every buffer of the engine -- the staged copies of host arrays and the staged secrets among them -- lies between
    guards that are compared when it is released"""
    assert os.environ.get("MKT_MEM_GUARD")
    calls = 0
    for p in (SMALLEST, LARGEST):
        key = secret_keys(p, seed=29)[0]
        sch = mk.Scheme(p)
        try:
            assert int(sch.get_metric("mem_guard_check")) == 0
            for G in (1, 3):
                ct = input_batches(p, np.random.default_rng(G))["uniform"][:G]
                want = host_share(p, key, 0, ct, 2.0 ** 20, 2**32 - 1)
                for mem in (H, D):
                    released = sch.get_metric("mem_guard_released")
                    got = mk.rlwe_partial_decrypt(to_mem(ct, mem), key, p, 0, 2.0 ** 20, deterministic_seed=SEED, row0=2**32 - 1, scheme=sch)
                    assert same_words(host_words(got), want), (sid(p), G, mem)
                    assert int(sch.get_metric("mem_guard_check")) == 0, (sid(p), G, mem, "a guard of the engine's own memory was written")
                    assert sch.get_metric("mem_guard_released") > released, (sid(p), G, mem, "no staged buffer was compared at its release")
                    calls += 1
        finally:
            sch.close()
    return calls


def test_engine_buffers_keep_their_guards(require_gpu):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MKT_") or k == "MKT_LIB_PATH"}
    env["MKT_MEM_GUARD"] = "64"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "guard"], env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, f"child: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert json.loads(lines[-1]) == {"ok": True, "calls": 8}


# ---- 5: stream order ----
def test_shares_behind_a_late_producer(require_gpu, monkeypatch):
    """the pattern of test_gpu_stream_order.test_packed_outputs_behind_a_late_producer: the packs are written late on the tested stream, behind
    a spin, and the call still gives the reference words -- pinned to the stream, and following torch's current one; the control, with the
    producer on another stream, does not"""
    import test_gpu_stream_order as SO
    p = mk.KMS2party.scaled(n=5, N=256)
    key = secret_keys(p, seed=29)[1]
    ct = input_batches(p, np.random.default_rng(12))["uniform"]
    s = mk.Scheme(p)
    try:
        share = lambda: mk.rlwe_partial_decrypt(to_mem(ct, D), key, p, 1, 2.0 ** 20, deterministic_seed=SEED, scheme=s)      # noqa: E731
        want = SO.reference(share)
        assert same_words(want, host_share(p, key, 1, ct, 2.0 ** 20, 0))
        got, ms = SO.late_call(monkeypatch, s, share, 0, SO.streams().a, SC.PINNED)
        assert same_words(got, want)
        delay = SC.delay_ms([ms])
        cycles = SC.delay_cycles(delay, SO.rate())
        print(f"[stream order] ring share: host enqueue {ms:.3f} ms, delay {delay:.1f} ms = {cycles} cycles")
        got, _ = SO.late_call(monkeypatch, s, share, cycles, SO.streams().b, SC.PINNED, producer=SO.streams().a)
        assert not same_words(got, want), ("ring share", "delay too short or producer not late", delay)
        for how in (SC.PINNED, SC.TORCH):
            got, _ = SO.late_call(monkeypatch, s, share, cycles, SO.streams().a, how)
            assert same_words(got, want), ("ring share behind a late producer", how)
    finally:
        s.close()


# ---- 6: the C example ----
def test_c_example_through_the_abi(require_gpu, tmp_path):
    """examples/ring_share_gpu.c: gates, pack, every party's share on a context of its own, merge, from plain C (gcc, no Python)"""
    exe = str(tmp_path / "ring_share_gpu")
    lib = os.path.join(ROOT, "mktfhe_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "ring_share_gpu.c"),
                           "-o", exe, "-L" + lib, "-lmktfhe_hip", "-Wl,-rpath," + lib])
    out = subprocess.run([exe, "24", "256"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


if __name__ == "__main__":
    assert sys.argv[1:] == ["guard"]
    print(json.dumps({"ok": True, "calls": _guard_child()}))
