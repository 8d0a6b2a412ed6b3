"""WHERE every batch call writes (tests/footprint.py holds the arena and the step list; tests/test_footprint_cpu.py tests both without a GPU).

Almost every other GPU test pins the words a call returns.  Here every device tensor of a call -- arguments made by helpers.device_tensor,
outputs the binding allocates through scheme._empty -- is carved from one arena of pseudo-random bytes with guards on every side, and the
context is created under MKT_MEM_GUARD=64: every buffer of the engine itself (key tables, workspace, the staged copies of host arrays, the
shards' staging buffers) lies between two 64 KiB guards (mktfhe_amd/csrc/device_mem.h).  After EACH call:

  1. the words are those of the same call on plain tensors on a context created with the mode off (computed once per step and B);
  2. the arena holds its fill outside the carvings and the source words in every carving the call did not return (device memory);
  3. "mem_guard_check" has not moved -- no guard of a live buffer, and none of a buffer freed since (a call's staged copies), was written --
     and "mem_guard_buffers" > 0: the sweep looked at something.  A host-memory call has no arena: the guards round its staged copies are the
     only witness of a store behind a staged output, and "mem_guard_released" must have moved, so that they were in fact compared.

B = 1, 5, 33, 64, 65 (footprint.BATCHES says which tile each straddles).  Both arena layouts: in the packed one a pointer has the alignment
of its element type and no more, which is what include/mktfhe.h promises to take; mkt_seeded_keys_expand states that it needs 16 bytes for
two of its arguments, and its refusal of the packed pointers -- arena untouched -- is asserted instead of the call."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import context_life_cases as K
import footprint as F
import stream_cases as S
from context_life_cases import CHUNK, STEP
from helpers import ROOT, host_words, ks_expected, ks_ran, mk, same_words

pytestmark = pytest.mark.gpu

H, D = mk.MEM_HOST, mk.MEM_DEVICE
ERR_ARG = -1
GUARD_KIB = "64"
ARENA_BYTES = 16 << 20
WHERES = ("aligned", "packed", "host")          # device tensors in either arena layout; host arrays
_ARENAS, _REF, _INPUTS = {}, {}, {}
_TOTAL = [0]                                    # findings the process has seen so far: every check compares with it


def arena_of(layout):
    if layout not in _ARENAS:
        _ARENAS[layout] = F.Arena(ARENA_BYTES, layout)
    return _ARENAS[layout]


def inputs(name):
    """context_life_cases.make_inputs, once per set (it opens and closes a context of its own: before the guard mode is switched on)"""
    if name not in _INPUTS:
        assert "MKT_MEM_GUARD" not in os.environ
        _INPUTS[name] = K.make_inputs(name)
    return _INPUTS[name]


def big_inputs(name, n, seed):
    """n rows of any words in place of the per-row arrays the chunk-crossing steps read (as tests/test_gpu_context_life.py makes them)"""
    i = inputs(name)
    p, rng = i.p, np.random.default_rng(seed)
    b = K.window(i, 0, 0)
    b.x, b.y, b.z = (K.lwe_words(p, rng, n) for _ in range(3))
    b.ops = rng.integers(0, 6, n).astype(np.uint8) | rng.choice(np.array([0, 8, 16, 24], dtype=np.uint8), n)
    b.sel = rng.integers(0, K.NLUTS, n).astype(np.uint32)
    b.n = n
    return b


def last_error(s):
    from mktfhe_amd import _lib
    return (_lib.lib().mkt_last_error(s.h) or b"").decode()


def swept(s):
    """-> (findings since the process started, buffers the sweep looked at) after draining the context's device"""
    return int(s.get_metric("mem_guard_check")), int(s.get_metric("mem_guard_buffers"))


def references(tag, make, i, steps, Bs, **kw):
    """the words of every (step, B) on plain tensors, on a context that make() creates with the guard mode off; once per (tag, step, B, kw)"""
    need = [(st, B) for st in steps for B in Bs if (tag, st.name, B, tuple(sorted(kw.items()))) not in _REF]
    if need:
        assert "MKT_MEM_GUARD" not in os.environ
        s = make()
        try:
            assert swept(s) == (_TOTAL[0], 0), "a context created without MKT_MEM_GUARD has guarded buffers"
            for st, B in need:
                _REF[tag, st.name, B, tuple(sorted(kw.items()))] = host_words(st.fn(s, i, B, D, **kw))
        finally:
            s.close()
    return lambda st, B: _REF[tag, st.name, B, tuple(sorted(kw.items()))]


def guarded(monkeypatch, make, sweep_on=None):
    """a context created and keyed by make() under MKT_MEM_GUARD: right after keying no guard has been written -- the key loads stayed inside
    the resident tables -- and the sweep saw those tables"""
    monkeypatch.setenv("MKT_MEM_GUARD", GUARD_KIB)
    s = make()
    for c in (sweep_on(s) if sweep_on else [s]):
        total, nbuf = swept(c)
        assert total == _TOTAL[0], ("a key load wrote a guard", last_error(c))
        assert nbuf > 0, "the sweep saw no guarded buffer: the mode is not on"
    return s


def one_call(s, step, i, B, where, want, sweep_on=None, **kw):
    """ONE call of the step at B in `where`, then the three assertions"""
    import torch
    ctxs = sweep_on(s) if sweep_on else [s]
    released = ctxs[0].get_metric("mem_guard_released")
    what = (step.name, B, where, kw)
    findings = []
    if where == "host":
        got = host_words(step.fn(s, i, B, H, **kw))
    else:
        arena = arena_of(where)
        arena.reset()
        with F.tensors_in(arena):
            if step.name == "seeded_keys_expand" and where == "packed":
                # brk_seeded, the first carving, lies 4 or 8 bytes off a 16-byte boundary: mkt_seeded_keys_expand refuses it before any launch
                with pytest.raises(mk.MktError) as ei:
                    step.fn(s, i, B, D, **kw)
                assert ei.value.code == ERR_ARG and "aligned to 16 bytes" in str(ei.value), (what, str(ei.value))
                assert (arena.base + arena.carvings[0].offset) % 16 != 0, "the pointer that was refused"
                r, got = [], None
            else:
                r = step.fn(s, i, B, D, **kw)
                got = host_words(r)
        torch.cuda.synchronize()
        findings = arena.check(written=r)
        assert arena.carvings, (what, "no tensor of the call was carved from the arena")
    for c in ctxs:
        total, nbuf = swept(c)
        assert total == _TOTAL[0], (what, "a guard of the engine's own memory was written", last_error(c))
        assert nbuf > 0, (what, "the sweep saw no guarded buffer")
    if where == "host":
        assert ctxs[0].get_metric("mem_guard_released") > released, (what, "no staged copy was compared at its release")
    assert not findings, (what, findings)
    if got is not None:
        assert same_words(got, want), (what, "the words differ from the plain call's with the guard mode off")


def call_loop(s, i, steps, Bs, ref, wheres=WHERES, sweep_on=None, after=None, **kw):
    """-> calls made.  A finding fails the test at once; the total the later tests compare with follows what the process has seen.
    after(step, B): called behind each call (the key-switch children read which kernel it ran)"""
    n = 0
    try:
        for step in steps:
            for B in Bs:
                for where in wheres:
                    one_call(s, step, i, B, where, ref(step, B), sweep_on, **kw)
                    if after:
                        after(step, B)
                    n += 1
    finally:
        _TOTAL[0] = swept((sweep_on(s) if sweep_on else [s])[0])[0]
    return n


# ---- every entry point, every set ----
@pytest.mark.parametrize("where", WHERES)
@pytest.mark.parametrize("name", list(K.SETS))
def test_every_call_writes_only_what_it_owns(require_gpu, monkeypatch, name, where):
    i, steps = inputs(name), K.steps_of(name)
    assert [st.name for st in steps] == [st.name for st in F.FOOTPRINT_STEPS if st.name != "pack" and st.applies(*K.set_of(name))]
    ref = references(name, lambda: K.new_scheme(name), i, steps, F.BATCHES)
    s = guarded(monkeypatch, lambda: K.new_scheme(name))
    try:
        assert call_loop(s, i, steps, F.BATCHES, ref, (where,)) == len(steps) * len(F.BATCHES)
    finally:
        s.close()


# ---- the arena on the device: the comparison that every test above relies on finds a byte stored by the GPU ----
def test_the_arena_finds_stores_made_on_the_device(require_gpu):
    import torch
    for layout in F.LAYOUTS:
        a = arena_of(layout)
        a.reset()
        x = a.carve(np.arange(5 * 13, dtype=np.uint32).reshape(5, 13))
        y = a.carve_empty((5, 13), np.int32)
        assert a.check() == [] and x.dtype == torch.int32 and tuple(y.shape) == (5, 13) and x.data_ptr() == a.base + a.carvings[0].offset
        assert (x.data_ptr() % 256 == 0) if layout == "aligned" else (x.data_ptr() % 16 == 4 and y.data_ptr() % 16 == 8)
        behind = a.carvings[0].offset + a.carvings[0].size
        a.buf[behind:behind + 52] = 0                                           # one row of zeros behind x, and a word of x itself
        x[2, 3] = -1
        y.fill_(7)
        got = a.check(written=[y])
        assert got[0][:2] == ("input written", 0) and got[0][2] == a.carvings[0].offset + (2 * 13 + 3) * 4 and got[0][3] == 4, got
        assert len(got) > 1 and all(g[0] == "guard written" and behind <= g[2] < behind + 52 for g in got[1:]) and 48 <= sum(g[3] for g in got[1:]) <= 52, got
        a.reset()
        assert a.check() == []


# ---- the tile of the seeded expansion that the five batch sizes do not reach ----
@pytest.mark.parametrize("name", ["cggi", "lmss", "kms"])
def test_seeded_expansion_round_its_output_tile(require_gpu, monkeypatch, name):
    p = K.set_of(name)[0]
    Bs = F.seeded_expand_batches(p)
    assert Bs[0] > max(F.BATCHES) and Bs[0] * p.lwe_len <= F.seeded_expand_tile_words(p.n, p.lwe_len) < Bs[1] * p.lwe_len
    i = K.window(inputs(name), 0, 0)
    i.body = np.random.default_rng(87).integers(0, 1 << 32, max(Bs), dtype=np.uint64).astype(np.uint32)
    ref = references(name + "-tile", lambda: K.new_scheme(name), i, [STEP["seeded_expand"]], Bs)
    s = guarded(monkeypatch, lambda: K.new_scheme(name))
    try:
        call_loop(s, i, [STEP["seeded_expand"]], Bs, ref)
    finally:
        s.close()


# ---- kernel variants: the option walked on the live context, so that the workspace it regrows is a guarded one ----
# (context_life_cases.OPTION_WALKS takes the block kernel to 4 rotations per workgroup; 2 is its other grouped form, and B = 5 and 33 are ragged under both)
WALKS = K.OPTION_WALKS + [K.Walk("lmss", {}, "rot_blkg", (2, 0), ("blindrotate_blk_kernel", "blindrotate_k1_kernel"))]


@pytest.mark.parametrize("w", WALKS, ids=lambda w: K.walk_id(w) + "".join(str(v) for v in w.values))
def test_kernel_variants_write_only_what_they_own(require_gpu, monkeypatch, w):
    i, steps, Bs = inputs(w.set), K.steps_of(w.set), (5, 33)
    ref = references(w.set, lambda: K.new_scheme(w.set), i, steps, Bs)          # options do not change words (mktfhe.h): the plain context's
    s = guarded(monkeypatch, lambda: K.new_scheme(w.set))
    try:
        for k, v in w.before.items():
            s.set_option(k, v)
        for value, kernel in zip(w.values, w.kernels):
            s.set_option(w.option, value)
            call_loop(s, i, [STEP["gate"]], (33,), ref, ("aligned",))
            assert s.last_kernel_name() == kernel, (K.walk_id(w), value, s.last_kernel_name(), "expected", kernel)
            call_loop(s, i, steps, Bs, ref)
    finally:
        s.close()


# ---- the shorter last chunk inside a workspace sized for a full one ----
@pytest.mark.parametrize("step,B,kw", [("gate_ops", CHUNK + 3, {}), ("lut_many_bootstrap", CHUNK + 3, {"o": 4}), ("mux", CHUNK // 2 + 3, {})], ids=lambda v: v if isinstance(v, str) else None)
def test_a_short_last_chunk_stays_inside_the_workspace(require_gpu, monkeypatch, step, B, kw):
    name = "cggi"
    big = big_inputs(name, CHUNK + 3, 83)
    ref = references(name + "-big", lambda: K.new_scheme(name), big, [STEP[step]], (B,), **kw)
    s = guarded(monkeypatch, lambda: K.new_scheme(name))
    try:
        call_loop(s, big, [STEP[step]], (B,), ref, **kw)
    finally:
        s.close()


# ---- packed outputs ----
@pytest.mark.parametrize("case", F.PACK_SETS, ids=lambda c: ("exact-" if c[1] == mk.ARITH_EXACT else "f64-") + F.PC.sid(c[0][0]))
def test_packed_outputs_write_only_what_they_own(require_gpu, monkeypatch, case):
    from test_gpu_pack import pack_setup
    (p, (l, logB)), arith = case
    counts = F.PACK_COUNTS(p.N)
    rng = np.random.default_rng(85)
    i = types.SimpleNamespace(p=p, x=K.lwe_words(p, rng, max(counts)), pack_idx=rng.permutation(max(counts)).astype(np.uint32))
    step = F.FOOTPRINT_STEPS[-1]

    def idx_within(B):
        w = types.SimpleNamespace(**vars(i))
        w.pack_idx = (i.pack_idx[:B] % B).astype(np.uint32)                       # indices into the B rows handed over (some rows picked twice)
        return w

    class Within:
        """the step on indices that stay inside the rows of the call"""
        name, entry = step.name, step.entry

        @staticmethod
        def fn(s, i_, B, mem, **kw):
            return step.fn(s, idx_within(B), B, mem, **kw)

    make = lambda: pack_setup(p, l, logB, arith=arith)[2]      # noqa: E731
    ref = references(("pack", F.PC.sid(p), arith), make, i, [Within], counts)
    s = guarded(monkeypatch, make)
    try:
        call_loop(s, i, [Within], counts, ref)
    finally:
        s.close()


# ---- shards: the replicated tables and the shards' staging buffers ----
def test_shards_write_only_what_they_own(require_gpu, monkeypatch):
    name = S.SHARD_SET
    p, arith = K.set_of(name)
    crs, keys = K.keys_of(name)
    i, steps, Bs = inputs(name), [STEP[n] for n in S.SHARD_STEPS], (7, 2)       # B = 2 leaves one of the three shards empty
    ref = references(name, lambda: K.new_scheme(name), i, steps, Bs)
    make = lambda: mk.setup_multi(p, S.SHARD_DEVICES, keys=keys, a=crs, arith=arith, private_keys=True, stage_always=True)      # noqa: E731
    every = lambda m: [m.shard(j) for j in range(m.nshards)]      # noqa: E731
    multi = guarded(monkeypatch, make, every)
    try:
        call_loop(multi, i, steps, Bs, ref, sweep_on=every)
    finally:
        multi.close()


# ---- the key-switch kernel choices: process-wide launcher switches, one child process per setting (as tests/test_gpu_switches.py forces them);
#      and the transforms at two per block (MKT_FFT_NB = 2: NBT), where B = 5 and 33 leave the last block half empty ----
#      Every setting of the older kernels names MKT_KS_MFMA = 0 (else the matrix cores serve "cggi" and "kms" whatever it says); the last three
#      are the matrix cores forced, forced beside switches that then choose nothing, and automatic.  Every key-switch child reports which
#      kernel each call ran and the parent holds the report to helpers.ks_expected
KS_SETTINGS = [{**e, "MKT_KS_MFMA": "0"} for e in (
    {"MKT_KS_PAIR": "0"}, {"MKT_KS_G": "8"}, {"MKT_KS_G": "16"}, {"MKT_KS_WAVES": "1"}, {"MKT_KS_WAVES": "2"},
    {"MKT_KS_PAIR": "0", "MKT_KS_WAVES": "1"}, {"MKT_KS_PAIR": "0", "MKT_KS_WAVES": "2"}, {"MKT_KS_BLOCKS": "1"},
    {"MKT_KS_BLOCKS": "100000"}, {"MKT_KS_G": "12"}, {"MKT_KS_G": "64"})]
KS_SETTINGS += [{"MKT_KS_MFMA": "1"}, {"MKT_KS_MFMA": "1", "MKT_KS_G": "8", "MKT_KS_PAIR": "0"}, {"MKT_KS_MFMA": "-1"}]
KS_CHILD_SETS = ("cggi", "lmss", "kms")          # unbalanced digits on one key and on one key per party (the matrix cores, or the older kernels under MKT_KS_MFMA = 0); balanced digits (never the matrix cores)
KS_CHILD_STEPS = ("gate_ops", "mux", "keyswitch", "keyswitch_at", "lut_many_bootstrap", "lut_bootstrap_at")
FFT_SETTING = {"MKT_FFT_NB": "2"}
FFT_CHILD_SETS = ("cggi", "kms", "ccs")
FFT_CHILD_STEPS = ("transform_fwd", "transform_inv", "gate_ops")
CHILD = {"ks": (KS_CHILD_SETS, KS_CHILD_STEPS), "fft": (FFT_CHILD_SETS, FFT_CHILD_STEPS)}
CHILD_TIMEOUT = 240
_child_fault = []          # a child that died by a signal / abort / segfault / time limit: no further child is started


def test_key_switch_settings_are_those_the_switch_test_forces():
    import test_gpu_switches
    assert KS_SETTINGS == test_gpu_switches.KS_SETTINGS and FFT_SETTING in test_gpu_switches.FFT_SETTINGS


@pytest.mark.parametrize("kind,setting", [("ks", e) for e in KS_SETTINGS] + [("fft", FFT_SETTING)], ids=lambda e: e if isinstance(e, str) else "-".join(f"{k[4:]}{x}" for k, x in e.items()))
def test_launcher_kernel_choices_write_only_what_they_own(require_gpu, kind, setting):
    assert not _child_fault, f"an earlier child process faulted: {_child_fault}"
    env = {k: v for k, v in os.environ.items() if not k.startswith("MKT_") or k == "MKT_LIB_PATH"}
    env.update(setting)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), kind], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _child_fault.append((setting, "time limit"))
        raise
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137):
        _child_fault.append((setting, r.returncode))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, f"child {setting}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    j = json.loads(lines[-1])
    assert j["ok"] and j["calls"] == len(CHILD[kind][0]) * len(CHILD[kind][1]) * 2 * len(WHERES) and j["env"] == setting, j
    if kind == "ks":             # every call of every step ran the kernel, tile width and wave count that its set and the setting imply
        assert sorted(j["ran"]) == sorted(f"{name}:{step}:{B}" for name in KS_CHILD_SETS for step in KS_CHILD_STEPS for B in (5, 33)), sorted(j["ran"])
        import test_gpu_switches
        for key, seen in j["ran"].items():
            want = ks_expected(K.set_of(key.split(":")[0])[0], setting)
            assert [tuple(r) for r in seen] == [want], (setting, key, "ran (kernel, G, waves)", seen, "implied", want)
            if not key.startswith("lmss:"):      # unbalanced digits, D = 4, f = 8: also what the setting is written to reach (test_gpu_switches.KS_MEANT)
                assert want == test_gpu_switches.KS_MEANT[KS_SETTINGS.index(setting)], (setting, key, want)


class _Env:
    """what the child needs of pytest's monkeypatch"""

    @staticmethod
    def setenv(k, v):
        os.environ[k] = v


def _child(kind):
    """-> (calls, {"<set>:<step>:<B>": the distinct (kernel, G, waves) that the key switches of those calls ran})"""
    calls, ran = 0, {}

    def note(name, s):
        def after(step, B):
            seen = ran.setdefault(f"{name}:{step.name}:{B}", [])
            if ks_ran(s) not in seen:
                seen.append(ks_ran(s))
        return after

    for name in CHILD[kind][0]:
        os.environ.pop("MKT_MEM_GUARD", None)
        i, steps, Bs = inputs(name), [STEP[n] for n in CHILD[kind][1]], (5, 33)
        ref = references(name, lambda: K.new_scheme(name), i, steps, Bs)
        s = guarded(_Env, lambda: K.new_scheme(name))
        try:
            calls += call_loop(s, i, steps, Bs, ref, after=note(name, s) if kind == "ks" else None)
        finally:
            s.close()
    return calls, ran


if __name__ == "__main__":
    assert len(sys.argv) == 2 and sys.argv[1] in CHILD
    env = {k: v for k, v in os.environ.items() if k.startswith("MKT_") and k not in ("MKT_LIB_PATH", "MKT_MEM_GUARD")}
    calls, ran = _child(sys.argv[1])
    print(json.dumps({"ok": True, "calls": calls, "env": env, "ran": ran}))
