"""WHEN the steps of a call run (tests/stream_cases.py holds the case lists, helpers.LateProducer the mechanism).

Every other GPU test synchronises the host around its calls, so a kernel, a memset or a staging copy enqueued on the wrong stream would
compute the right words all the same.  Here the inputs of a call are LATE: its device tensors hold zeros, and their real words arrive by
an asynchronous copy that waits behind a long spin on the stream the call is to be ordered with.  A step that runs anywhere else reads
zeros -- every time, not one run in a hundred -- and the words differ from the REFERENCE: the same call on the same context with everything
synchronous (default stream, inputs landed, the device drained), which the rest of the suite ties to the oracle and to fresh contexts.
Equality is bit for bit (helpers.same_words).

THE DELAY is not fixed in advance.  torch.cuda._sleep is calibrated once per module (helpers.sleep_cycles_per_ms); per set the spin lasts
stream_cases.delay_ms of the host wall times of its calls made through the same harness WITHOUT the spin.  Whether that is long enough is not
judged by its value: every test first runs THE CONTROL -- gate_ops and transform_fwd with the context on another stream than the one the
inputs arrive on -- which must NOT give the reference's words, else the test fails with "delay too short or producer not late".

THE STREAMS.  A HIP process drives a few hardware queues, and two streams that share one run in order whatever the library does; the
control would then fail and the order test (e) could not fail.  So the streams used here are picked once per module from torch's pool by a
probe: a kernel on one must finish while a spin on the other is still running.

e is what found the defect mkt_set_stream had: it only stored the pointer, so two calls on one Scheme under two torch streams shared a
workspace and were ordered by nothing (a call B made after a call A finished BEFORE it; e measured that as a negative time from the end
of A to the end of B, the whole delay long).  mkt_set_stream now makes the stream a context moves to wait for the one it leaves."""
import time
import types

import numpy as np
import pytest

import context_life_cases as K
import helpers
import pack_cases as PC
import stream_cases as S
import test_gpu_context_life as L
from context_life_cases import STEP
from helpers import LateProducer, encrypt_bits, gpu_scheme, host_words, keygen, mk, same_words, sleep_cycles_per_ms, to_mem

pytestmark = pytest.mark.gpu

H, D, B = mk.MEM_HOST, mk.MEM_DEVICE, S.B
_MODULE = {}


def _torch():
    import torch
    return torch


def rate():
    """cycles of torch.cuda._sleep per millisecond, measured once"""
    if "rate" not in _MODULE:
        _MODULE["rate"] = sleep_cycles_per_ms()
        print(f"\n[stream order] torch.cuda._sleep: {_MODULE['rate']:.0f} cycles per ms (10**7 cycles = {1e7 / _MODULE['rate']:.2f} ms)")
    return _MODULE["rate"]


def _independent(x, y):
    """does a kernel on stream y finish while a 20 ms spin on stream x is still running?  (Polled for 10 ms at the most)"""
    torch = _torch()
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    with torch.cuda.stream(x):
        torch.cuda._sleep(S.delay_cycles(20.0, rate()))
    with torch.cuda.stream(y):
        torch.zeros(64, device="cuda")
        done.record()
    t0 = time.perf_counter()
    while not done.query() and time.perf_counter() - t0 < 0.010:
        pass
    ok = done.query()
    torch.cuda.synchronize()
    return ok


def streams():
    """-> a, b, side: three non-blocking streams of torch's pool that do not hold each other up, a not held up by the NULL stream either"""
    if "streams" not in _MODULE:
        torch = _torch()
        torch.zeros(64, device="cuda")
        null, picked, tried = torch.cuda.default_stream(), [], 0
        while len(picked) < 3 and tried < 16:
            c, tried = torch.cuda.Stream(), tried + 1
            if all(_independent(o, c) and _independent(c, o) for o in picked) and (picked or (_independent(c, null) and _independent(null, c))):
                picked.append(c)
        assert len(picked) == 3, f"only {len(picked)} of {tried} streams run independently of each other: the late producer needs three"
        print(f"[stream order] three independent streams after {tried} tried")
        _MODULE["streams"] = types.SimpleNamespace(a=picked[0], b=picked[1], side=picked[2], null=null)
    return _MODULE["streams"]


def reference(call):
    """call() with everything synchronous -> host words"""
    torch = _torch()
    torch.cuda.synchronize()
    r = call()
    torch.cuda.synchronize()
    return host_words(r)


def late_call(mp, s, call, cycles, on, how, producer=None, before=None):
    """call() on context s behind a late producer -> (host words, host milliseconds from the spin to the return of the call).
    on: the stream the call is to run on -- how = PINNED: s.set_stream(on.cuda_stream), put back to None afterwards; TORCH: the call is made
    under torch.cuda.stream(on) and s is left to follow (or, a MultiScheme, to do what it does).  producer: the stream of the spin and of the
    copies of the real words (default: `on`; the control names another).  cycles = 0: no spin.  before(): enqueued first, after the device has
    been drained.  The result is read back on `on`; then the device is drained, and only then are the tensors let go"""
    torch = _torch()
    st = streams()
    lp = LateProducer(producer or on, cycles, st.side)
    torch.cuda.synchronize()
    if how == S.PINNED:
        s.set_stream(on.cuda_stream)
    try:
        if before:
            before()
        with mp.context() as m:
            m.setattr(helpers, "device_tensor", lp.tensor)
            t0 = time.perf_counter()
            if cycles:
                lp.delay()
            if how == S.TORCH:
                with torch.cuda.stream(on):
                    r = call()
            else:
                r = call()
            ms = (time.perf_counter() - t0) * 1e3
        with torch.cuda.stream(on):
            got = host_words(r)
        torch.cuda.synchronize()
    finally:
        if how == S.PINNED:
            s.set_stream(None)
    return got, ms


def prepared(mp, name):
    """the set's long-lived context, its inputs, the reference of every step in both memory kinds, the host time of every step made through
    the harness without the spin (pinned, device memory: also the warm-up, so that no workspace grows behind a spin) and the delay"""
    sets = _MODULE.setdefault("sets", {})
    if name not in sets:
        st = types.SimpleNamespace(name=name, s=K.new_scheme(name), i=L.inputs(name), ref={}, host_ms={})
        for step in K.steps_of(name):
            for mem in (D, H):
                st.ref[step.name, mem] = reference(lambda: step.fn(st.s, st.i, B, mem))
            for _ in range(2):      # the second time counts: the first also pays what is paid once (pinned buffers, the allocator's blocks on a new stream)
                got, st.host_ms[step.name] = late_call(mp, st.s, lambda: step.fn(st.s, st.i, B, D), 0, streams().a, S.PINNED)
                assert same_words(got, st.ref[step.name, D]), (name, step.name, "made through the harness without a spin")
        st.delay_ms = S.delay_ms(list(st.host_ms.values()))
        st.cycles = S.delay_cycles(st.delay_ms, rate())
        slow = max(st.host_ms, key=st.host_ms.get)
        print(f"[stream order] {name}: longest host enqueue {st.host_ms[slow]:.3f} ms ({slow}), delay {st.delay_ms:.1f} ms = {st.cycles} cycles")
        sets[name] = st
    return sets[name]


def control(mp, st):
    """the harness must be able to fail: with the context on stream b and the inputs arriving on stream a, the words must differ"""
    for name in S.CONTROL_STEPS:
        got, _ = late_call(mp, st.s, lambda: STEP[name].fn(st.s, st.i, B, D), st.cycles, streams().b, S.PINNED, producer=streams().a)
        assert not same_words(got, st.ref[name, D]), (st.name, name, "delay too short or producer not late", st.delay_ms)


@pytest.fixture(scope="module", autouse=True)
def _contexts_closed_at_the_end():
    yield
    for st in _MODULE.pop("sets", {}).values():
        st.s.close()


# ---- a: every entry point ----
@pytest.mark.parametrize("name", S.SETS)
def test_every_entry_point_is_ordered_behind_a_late_producer(require_gpu, monkeypatch, name):
    """every step of the set, device tensors and host arrays, the stream pinned with set_stream or followed from torch: behind the spin,
    with late inputs, the words are the reference's"""
    st = prepared(monkeypatch, name)
    control(monkeypatch, st)
    wrong = []
    for step, mem, how in S.cases(name):
        got, _ = late_call(monkeypatch, st.s, lambda: step.fn(st.s, st.i, B, mem), st.cycles, streams().a, how)
        if not same_words(got, st.ref[step.name, mem]):
            wrong.append((step.name, S.variant_id((mem, how))))
    assert not wrong, (name, "steps that did not wait for their inputs", wrong)


# ---- b: forks ----
@pytest.mark.parametrize("name", S.SETS)
def test_forks_are_ordered_on_their_own_and_on_torchs_stream(require_gpu, monkeypatch, name):
    """the parent pinned to stream b and busy behind its own spin (a device-memory gate): the fork makes a gate, a table bootstrap and a key
    switch on host arrays on its own stream, then the same three on late device tensors following torch's stream a"""
    torch = _torch()
    st = prepared(monkeypatch, name)
    control(monkeypatch, st)
    sa, sb = streams().a, streams().b
    parent = []

    def busy():
        with torch.cuda.stream(sb):
            torch.cuda._sleep(st.cycles)
        parent.append(STEP["gate"].fn(st.s, st.i, B, D))

    f = st.s.fork()
    st.s.set_stream(sb.cuda_stream)
    try:
        torch.cuda.synchronize()
        busy()
        for step in S.FORK_STEPS:
            got = host_words(STEP[step].fn(f, st.i, B, H))
            assert same_words(got, st.ref[step, H]), (name, step, "the fork on its own stream, host arrays")
        for step in S.FORK_STEPS:
            got, _ = late_call(monkeypatch, f, lambda: STEP[step].fn(f, st.i, B, D), st.cycles, sa, S.TORCH, before=busy)
            assert same_words(got, st.ref[step, D]), (name, step, "the fork following torch's stream, late device tensors")
        torch.cuda.synchronize()
        assert all(same_words(host_words(r), st.ref["gate", D]) for r in parent) and len(parent) == 1 + len(S.FORK_STEPS), (name, "the parent's gates")
    finally:
        st.s.set_stream(None)
        f.close()


# ---- c: packed outputs ----
def test_packed_outputs_behind_a_late_producer(require_gpu, monkeypatch):
    """mktfhe_pack.h on the smallest set of tests/pack_cases.py: on the tested stream a spin, load_packing_key (it drains the stream, spin
    included), a second spin, and pack of rows picked by index, rows and indices late.  Control: the same with the context on another stream"""
    p, (l, logB) = PC.KERNEL_SETS[0]
    assert (p.n, p.N, p.nparty) == (5, 32, 1)
    crs, keys = keygen(p, 9)
    pk = mk.packing_keygen(keys[0], p, l, logB, deterministic_seed=20)
    x = encrypt_bits(p, keys, np.random.default_rng(3).integers(0, 2, B).astype(bool), seed=400)
    idx = np.random.default_rng(4).permutation(B).astype(np.uint32)
    s = gpu_scheme(p, crs, keys)
    try:
        mk.load_packing_key(s, 0, pk, l, logB)
        pack = lambda: mk.pack(s, to_mem(x, D), to_mem(idx, D))      # noqa: E731
        want = reference(pack)
        assert want.shape == (2, p.k + 1, p.N) and want.any()
        got, ms = late_call(monkeypatch, s, pack, 0, streams().a, S.PINNED)
        assert same_words(got, want)
        delay = S.delay_ms([ms])
        cycles = S.delay_cycles(delay, rate())
        print(f"[stream order] pack: host enqueue {ms:.3f} ms, delay {delay:.1f} ms = {cycles} cycles")
        got, _ = late_call(monkeypatch, s, pack, cycles, streams().b, S.PINNED, producer=streams().a)
        assert not same_words(got, want), ("pack", "delay too short or producer not late", delay)
        for how in (S.PINNED, S.TORCH):
            def load_then_pack():
                mk.load_packing_key(s, 0, pk, l, logB)
                with _torch().cuda.stream(streams().a):
                    _torch().cuda._sleep(cycles)
                return pack()

            got, _ = late_call(monkeypatch, s, load_then_pack, cycles, streams().a, how)
            assert same_words(got, want), ("load_packing_key, then pack", how)
    finally:
        s.close()


# ---- d: key loads behind a batch, as a detector ----
def mixed_keys(name, piece):
    """keys of seed 1 loaded the plain way, then `piece` of every party (the CRS: the one there is) loaded again from the keys of seed 2"""
    def keyed(s):
        L.key_plain(name, S.KEY_SEEDS[0])(s)
        reload_piece(s, name, piece)
    return keyed


def reload_piece(s, name, piece):
    crs, keys = K.keys_of(name, S.KEY_SEEDS[1])
    for party in ([None] if piece == "crs" else range(len(keys))):
        L.load_piece(s, piece, party, crs, keys)


@pytest.mark.parametrize("name", S.KEY_SETS)
def test_key_loads_are_ordered_behind_a_batch(require_gpu, monkeypatch, name):
    """for every piece of the key set (context_life_cases.pieces_of): on a context pinned to a non-blocking stream, a spin, a device-memory
    gate_ops batch, that piece loaded again from another key seed with nothing in between, the batch again.  The first result is the words
    under the old keys: a load that did not wait for the stream would change the keys under a batch that has not started.  The second is the
    words of a fresh context keyed the same mixed way.  (test_gpu_context_life.ksk_reload_behind_a_batch loads the words the table already
    holds and passes either way.)  That the mixed keys give other words than the old ones is asserted for the two keys every gate reads"""
    torch = _torch()
    st = prepared(monkeypatch, name)
    control(monkeypatch, st)
    gate_ops, sa = STEP["gate_ops"], streams().a
    old = st.ref["gate_ops", D]
    for piece in K.pieces_of(K.set_of(name)[0]):
        want = L.fresh_step(name, gate_ops, B, D, S.KEY_SEEDS[1], L.made(name, mixed_keys(name, piece)), f"seed 1, {piece} of seed 2")
        if piece in ("brk", "ksk"):
            assert not same_words(want, old), (name, piece, "the mixed keys give the old keys' words")
        s = K.new_scheme(name)
        try:
            assert same_words(reference(lambda: gate_ops.fn(s, st.i, B, D)), old), (name, "a second context under the old keys")
            ops, x, y = (to_mem(v[:B], D) for v in (st.i.ops, st.i.x, st.i.y))
            torch.cuda.synchronize()
            s.set_stream(sa.cuda_stream)
            with torch.cuda.stream(sa):
                torch.cuda._sleep(st.cycles)
            first = s.gate_ops(ops, x, y)
            reload_piece(s, name, piece)
            second = s.gate_ops(ops, x, y)
            s.synchronize()
            torch.cuda.synchronize()
            assert same_words(host_words(first), old), (name, piece, "the batch enqueued before the load ran under the new keys")
            assert same_words(host_words(second), want), (name, piece, "the batch after the load")
        finally:
            s.close()


# ---- e: order across streams ----
@pytest.mark.parametrize("way", S.ORDER_WAYS)
def test_calls_on_one_context_run_in_the_order_they_were_made(require_gpu, monkeypatch, way):
    """set cggi, gate_ops, device tensors.  Call A on rows 0 .. 32 on stream a, behind the spin, its inputs late, then a timing event eA;
    call B on rows 33 .. 65 (landed) on another stream, then eB.  B was made after A, so it must end after A: eA.elapsed_time(eB) >= 0.
    Unordered, B runs to its end inside A's spin and the time is negative by about the whole delay; ordered, no host however slow can make
    it negative.  Both results are their references' either way (nothing overlaps in this schedule).  way: the context follows torch from
    stream a to stream b; is pinned with set_stream to a, then b; is pinned to a, then put back to the NULL stream; a fork follows torch"""
    torch = _torch()
    name = "cggi"
    st = prepared(monkeypatch, name)
    control(monkeypatch, st)
    go, sa, sb = STEP["gate_ops"], streams().a, streams().b
    rows_b = K.window(st.i, B, 2 * B)
    s = st.s.fork() if way == "fork" else st.s
    try:
        want_a = st.ref["gate_ops", D]
        want_b = reference(lambda: go.fn(s, rows_b, B, D))
        assert not same_words(want_a, want_b)
        ops, x, y = (to_mem(v, D) for v in (rows_b.ops, rows_b.x, rows_b.y))
        e_a, e_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        lp = LateProducer(sa, st.cycles, streams().side)
        torch.cuda.synchronize()
        with monkeypatch.context() as m:
            m.setattr(helpers, "device_tensor", lp.tensor)
            if way in ("torch", "fork"):
                with torch.cuda.stream(sa):
                    lp.delay()
                    r_a = go.fn(s, st.i, B, D)
                    e_a.record()
            else:
                s.set_stream(sa.cuda_stream)
                lp.delay()
                r_a = go.fn(s, st.i, B, D)
                e_a.record(sa)
        second = streams().null if way == "null" else sb
        if way == "set_stream":
            s.set_stream(sb.cuda_stream)
        elif way == "null":
            s.set_stream(None)
        with torch.cuda.stream(second):
            r_b = s.gate_ops(ops, x, y)
            e_b.record()
        torch.cuda.synchronize()
        ms = e_a.elapsed_time(e_b)
        print(f"[stream order] {way}: call B ended {ms:.3f} ms after call A (delay {st.delay_ms:.1f} ms)")
        assert same_words(host_words(r_a), want_a) and same_words(host_words(r_b), want_b), (way, "the words")
        assert ms >= 0, (way, "call B, made after call A on the same context, ended before it, by ms", -ms)
    finally:
        s.set_stream(None)
        if way == "fork":
            s.close()


# ---- f: sharded calls ----
def test_sharded_calls_wait_for_late_inputs(require_gpu, monkeypatch):
    """three logical shards over one device's key set: gate_ops and lut_bootstrap on late device tensors on a non-blocking stream give the
    single context's words (multi.cpp settle_inputs drains the device that owns an input before the shards read it)"""
    name = S.SHARD_SET
    st = prepared(monkeypatch, name)
    control(monkeypatch, st)
    p, arith = K.set_of(name)
    crs, keys = K.keys_of(name)
    multi = mk.setup_multi(p, S.SHARD_DEVICES, keys=keys, a=crs, arith=arith)
    try:
        for step in S.SHARD_STEPS:
            assert same_words(reference(lambda: STEP[step].fn(multi, st.i, B, D)), st.ref[step, D]), (step, "sharded, synchronous")
            got, _ = late_call(monkeypatch, multi, lambda: STEP[step].fn(multi, st.i, B, D), st.cycles, streams().a, S.TORCH)
            assert same_words(got, st.ref[step, D]), (step, "sharded, late inputs")
    finally:
        multi.close()
