"""One long-lived context against fresh ones, across call sequences (tests/context_life_cases.py holds the sets, steps and option walks).

Every other GPU test builds a context, makes one kind of call and closes it.  Here a context lives through every batch entry point, growing
and shrinking batches, both memory kinds, option changes, refused calls, key reloads and forks, and after each step its words are compared
with words it did not produce: the same step on a context created, keyed, used once and closed (`fresh_step`), and for gate, gate_ops,
bootstrap and mux also the CPU oracle (on the MKT_ARITH_EXACT sets its exact-arithmetic restatement, tests/ref_exact.py) on rows 0, B - 1
and both sides of every chunk boundary.  Equality is
exact throughout (bit for bit: helpers.same_words), so there is no tolerance to choose.  Fresh results are computed once per (set, step,
B, memory kind, key seed) and shared between the tests."""
import ctypes as C

import numpy as np
import pytest

import context_life_cases as K
from context_life_cases import CHUNK, NLUTS, OPTION_WALKS, POOL, SETS, STEP
from helpers import O, fresh, host_words, mk, oracle_scheme, same_words, to_mem
from mktfhe_amd import _lib

pytestmark = pytest.mark.gpu

H, D = mk.MEM_HOST, mk.MEM_DEVICE
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -2, -5
_INPUTS, _FRESH, _ORACLE, _ROWS = {}, {}, {}, {}


def inputs(name):
    if name not in _INPUTS:
        _INPUTS[name] = K.make_inputs(name)
    return _INPUTS[name]


def plain(name, seed=1):
    return lambda: K.new_scheme(name, seed)


def fresh_step(name, step, B, mem, seed=1, keyed=None, how=""):
    """the step on a context created, keyed (key seed `seed`, the plain way, or by `keyed`, named `how`), used for this one call and closed"""
    k = (name, step.name, B, mem, seed, how)
    if k not in _FRESH:
        _FRESH[k] = fresh(keyed or plain(name, seed), lambda s: step.fn(s, inputs(name), B, mem))
    return _FRESH[k]


def oracle(name):
    if name not in _ORACLE:
        _ORACLE[name] = oracle_scheme(K.set_of(name)[0], *K.keys_of(name))
    return _ORACLE[name]


def _neg(c):
    return (0 - c.astype(np.int64)).astype(np.uint32)


def rotated(name, lin):
    """blindrotate! of the linear part `lin` (bootstrapping.jl:8-24) -> accumulator [(b, a_0 ..)][N] as uint64: the CPU oracle on a
    Float64-reference set, the exact-arithmetic restatement (tests/ref_exact.py: the oracle's integer steps, exact schoolbook products) on
    an MKT_ARITH_EXACT one"""
    import ref_exact as RX
    p, arith = K.set_of(name)
    crs, keys = K.keys_of(name)
    so = oracle(name)
    at, bt = so.modswitch(lin)
    acc = so.testvector(bt)
    if arith == mk.ARITH_F64REF:
        out = so.blindrotate(at, acc)
    elif p.scheme in (mk.KMS, mk.KMS_BLOCK):
        out = RX.kms_blindrotate(p, keys, crs, at, acc)
    elif p.scheme == mk.CCS:
        out = RX.ccs_blindrotate(p, keys, crs, at, acc)
    else:
        out = (RX.blindrotate_lmss if p.blk_len > 1 else RX.blindrotate)(p, keys[0].brk, at, acc)
    return np.asarray(out).astype(np.uint64).reshape(-1, p.N)


def oracle_mux(name, s, a, b):
    """the native MUX on the oracle's operators: two blindrotate! of the AND-linear parts (gate.jl:10-17, NOT! :55-58), the accumulators
    added, + 1/8 at X^0 of b, one keyswitch!"""
    p = K.set_of(name)[0]
    mask = np.uint64((1 << p.W) - 1)
    acc = (rotated(name, O.gate_linear(1, s, a)) + rotated(name, O.gate_linear(1, _neg(s), b))) & mask
    acc[0, 0] = np.uint64((int(acc[0, 0]) + (1 << (p.W - 3))) & int(mask))
    return oracle(name).keyswitch(acc)


def oracle_row(name, step, i, j):
    """row j of gate, gate_ops, bootstrap or mux on inputs i by the CPU oracle (Float64-reference sets: its own gate and bootstrap entry
    points) or by the exact restatement (EXACT sets: keyswitch! of `rotated`)"""
    k = (name, step, i.n, j)                 # (computed once per row of a set's inputs: the sequence meets the same rows again)
    if k not in _ROWS:
        _ROWS[k] = _oracle_row(name, step, i, j)
    return _ROWS[k]


def _oracle_row(name, step, i, j):
    p, arith = K.set_of(name)
    so = oracle(name)
    if step == "mux":
        return oracle_mux(name, i.x[j], i.y[j], i.z[j])
    if step == "bootstrap":
        return so.bootstrap(i.x[j]) if arith == mk.ARITH_F64REF else so.keyswitch(rotated(name, i.x[j]))
    o = i.op if step == "gate" else int(i.ops[j])
    x, y = _neg(i.x[j]) if o & mk.OP_NOT_X else i.x[j], _neg(i.y[j]) if o & mk.OP_NOT_Y else i.y[j]
    return so.gate(o & 7, x, y) if arith == mk.ARITH_F64REF else so.keyswitch(rotated(name, O.gate_linear(o & 7, x, y)))


def edge_rows(B, chunk=CHUNK):
    """rows 0, B - 1 and both sides of every chunk boundary"""
    return sorted({0, B - 1} | {r for c in range(chunk, B, chunk) for r in (c - 1, c)}) if B else []


def oracle_check(name, step, i, B, got, chunk=CHUNK):
    """gate, gate_ops, bootstrap, mux: oracle_row's words on edge_rows"""
    if step.name not in K.ORACLE_STEPS:
        return
    for j in edge_rows(B, chunk):
        assert np.array_equal(got[j], oracle_row(name, step.name, i, j)), (name, step.name, B, "oracle, row", j)


def run(s, name, step, B, mem, label=""):
    """the step on the long-lived context s == the fresh context's words (and the oracle's where it is held to it) -> the words"""
    got = host_words(step.fn(s, inputs(name), B, mem))
    assert same_words(got, fresh_step(name, step, B, mem)), (name, step.name, B, "host" if mem == H else "device", label)
    oracle_check(name, step, inputs(name), B, got)
    return got


# ---- a: every call kind in sequence ----
@pytest.mark.parametrize("name", list(SETS))
def test_every_call_kind_in_sequence(require_gpu, name):
    """one context makes every applicable call once in the table's order and twice more in seeded permutations, B cycling through
    (5, 1, 70, 33, 0, 5), host arrays and GPU tensors alternating; every result is the fresh context's.  Then the context is forked and
    closed, and the fork makes the first five steps"""
    seq = K.sequence(name)
    assert {st.name for st, _, _ in seq} == {st.name for st in K.steps_of(name)} and len(seq) == 3 * len(K.steps_of(name))
    s = K.new_scheme(name)
    for j, (st, B, mem) in enumerate(seq):
        run(s, name, st, B, mem, f"step {j}")
    f = s.fork()
    s.close()
    for j, (st, B, mem) in enumerate(seq[:5]):
        run(f, name, st, B, mem, f"fork, step {j}")
    f.close()


# ---- b: workspace growth and chunk edges ----
def big_inputs(name, n, seed):
    """the set's inputs with n rows of any words in place of the per-row arrays the chunk-crossing steps read"""
    i = inputs(name)
    p = i.p
    rng = np.random.default_rng(seed)
    b = K.window(i, 0, 0)
    b.x, b.y, b.z = (K.lwe_words(p, rng, n) for _ in range(3))
    b.ops = rng.integers(0, 6, n).astype(np.uint8) | rng.choice(np.array([0, 8, 16, 24], dtype=np.uint8), n)
    b.ix, b.iy = (rng.integers(0, POOL, n).astype(np.uint32) for _ in range(2))
    b.sel = rng.integers(0, NLUTS, n).astype(np.uint32)
    b.accr = K.ring_words(p, rng, (n, p.k + 1, p.N))
    b.n = n
    return b


def test_workspace_growth_and_chunk_edges(require_gpu):
    """set cggi, GPU tensors: a small workspace, then calls past the chunk boundaries of mux (2 x 4096 rotations per chunk), the gates (8192),
    the many-table bootstrap (8192 / nout inputs) and the two unit key switches (mkt_keyswitch_batch launches over the whole batch), the
    (row, coefficient) table grown to 8192 rows and then used for fewer, and a small call in the grown workspace.  A call past a boundary
    equals the same call made in two pieces split there on a fresh context; the others equal the fresh context's.  Then the unchunked
    Float64 mkt_kms_phase1_batch at 8192 + 3 on set kms against two split calls, compared on the device"""
    import torch
    name = "cggi"
    big = big_inputs(name, CHUNK + 3, 81)
    s = K.new_scheme(name)

    def whole(step, B, **kw):
        return host_words(STEP[step].fn(s, big, B, D, **kw))

    def once(step, B, **kw):
        return fresh(plain(name), lambda f: STEP[step].fn(f, big, B, D, **kw))

    def pieces(step, B, cut, **kw):
        def two(f):
            a = host_words(STEP[step].fn(f, K.window(big, 0, cut), cut, D, **kw))
            return np.concatenate([a, host_words(STEP[step].fn(f, K.window(big, cut, B), B - cut, D, **kw))])
        return fresh(plain(name), two)

    def held(step, B, got, chunk):
        oracle_check(name, STEP[step], big, B, got, chunk)

    got = whole("gate", 5)
    assert same_words(got, once("gate", 5)), "gate, small workspace first"
    held("gate", 5, got, CHUNK)
    B = CHUNK // 2 + 1
    got = whole("mux", B)
    assert same_words(got, pieces("mux", B, CHUNK // 2)), "mux: 2 * nb gates of workspace, second chunk of one gate"
    held("mux", B, got, CHUNK // 2)
    B = CHUNK + 3
    assert same_words(whole("gate_gather", B), pieces("gate_gather", B, CHUNK)), "gate_gather: regrown to a full chunk"
    B = CHUNK // 8 + 1
    assert same_words(whole("lut_many_bootstrap", B, o=8), pieces("lut_many_bootstrap", B, CHUNK // 8, o=8)), "lut_many_bootstrap, 8 tables: the table sized for 8192 rows"
    assert same_words(whole("lut_bootstrap_at", 5), once("lut_bootstrap_at", 5)), "lut_bootstrap_at, 3 coefficients: a smaller table inside the larger capacity"
    assert same_words(whole("lut_many_bootstrap", 70, o=2), once("lut_many_bootstrap", 70, o=2)), "lut_many_bootstrap, 2 tables: the same, caller list absent"
    B = CHUNK + 3
    acc = to_mem(big.accr, D)
    want = pieces("keyswitch", B, CHUNK)
    assert same_words(host_words(K.keyswitch_call(s, acc, D)), want), "keyswitch: the unchunked unit call"
    assert same_words(host_words(mk.keyswitch_at(s, acc)), want), "keyswitch_at, src = coef = NULL: its chunked twin, the same words"
    got = whole("gate", 5)
    assert same_words(got, once("gate", 5)), "gate, small call in the grown workspace"
    s.close()

    # Float64 KMS phase 1 launches over the whole batch: 8192 + 3 against 8192 and 3 on a fresh context (about 100 MB of rows: on the device)
    name = "kms"
    pk = K.set_of(name)[0]
    s = K.new_scheme(name)
    run(s, name, STEP["gate"], 5, D, "kms, a gate first")
    at = to_mem(np.random.default_rng(82).integers(0, 2 * pk.N + 1, (B, pk.lwe_len - 1)).astype(np.uint32), D)      # mod-switched masks: 0 .. 2N
    bits = lambda t: torch.view_as_real(t).view(torch.int64)      # noqa: E731
    got = bits(K.kms_phase1_call(s, at, D))
    f = K.new_scheme(name)
    assert torch.equal(got[:CHUNK], bits(K.kms_phase1_call(f, at[:CHUNK], D))), "kms_phase1, rows below the boundary"
    assert torch.equal(got[CHUNK:], bits(K.kms_phase1_call(f, at[CHUNK:], D))), "kms_phase1, rows past the boundary"
    assert bool(got.any()), "the rows were written"
    f.close(); s.close()


# ---- c: options changed under a live workspace ----
@pytest.mark.parametrize("w", OPTION_WALKS, ids=K.walk_id)
def test_options_changed_under_a_live_workspace(require_gpu, w):
    """gate at B = 33 under the walk's first value; under each later value gate at B = 5 and B = 70; B = 33 again under the last.  Options
    do not change words (mktfhe.h): every result is the fresh context's with NO option set, and mkt_last_kernel_name names the kernel the
    value selects.  exact_kany is the one option with resets_workspace: set_option drops ws_gates to 0, so the next ensure_workspace
    reallocates for the new route -- with the run-time-k kernel's scratch, which a context that started on the register route never had"""
    gate = STEP["gate"]
    s = K.new_scheme(w.set)
    for k, v in w.before.items():
        s.set_option(k, v)

    def at(B, mem, value, kernel):
        got = host_words(gate.fn(s, inputs(w.set), B, mem))
        assert s.last_kernel_name() == kernel, (K.walk_id(w), value, B, s.last_kernel_name(), "expected", kernel)
        assert same_words(got, fresh_step(w.set, gate, B, mem)), (K.walk_id(w), value, B)

    s.set_option(w.option, w.values[0])
    at(33, D, w.values[0], w.kernels[0])
    for value, kernel in zip(w.values[1:], w.kernels[1:]):
        s.set_option(w.option, value)
        at(5, H, value, kernel)
        at(70, D, value, kernel)
    at(33, D, w.values[-1], w.kernels[-1])
    s.close()


# ---- d: refused calls ----
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def refusals(s, i):
    """-> [(what, call)]: call() makes one refused call in host memory -> (return code, output buffer or None, what it held before)"""
    p, L, B = i.p, _lib.lib(), 4
    x, y, ops, ix, iy, sel = (np.ascontiguousarray(v[:B]) for v in (i.x, i.y, i.ops, i.ix, i.iy, i.sel))
    T, U = np.ascontiguousarray(i.T), {o: np.ascontiguousarray(i.U[o]) for o in (2, 4)}
    pool = np.ascontiguousarray(i.pool)
    sent = lambda rows: np.full((rows, p.lwe_len), 0xA5A5A5A5, dtype=np.uint32)      # noqa: E731

    def bad_gate_code():
        out = sent(B)
        return L.mkt_gate_batch(s.h, 6, _ptr(x), _ptr(y), _ptr(out), B, H), out, sent(B)

    def index_outside_the_pool():
        out, bad = sent(B), ix.copy()
        bad[B - 1] = POOL
        return L.mkt_gate_batch_gather(s.h, _ptr(ops), _ptr(pool), POOL, _ptr(bad), _ptr(iy), _ptr(out), B, H), out, sent(B)

    def selector_beyond_the_tables():
        out, bad = sent(B), sel.copy()
        bad[0] = NLUTS
        return L.mkt_lut_bootstrap_batch(s.h, _ptr(T), NLUTS, _ptr(bad), _ptr(x), _ptr(out), B, H), out, sent(B)

    def nout_3():
        out = sent(3 * B)
        return L.mkt_lut_many_bootstrap_batch(s.h, _ptr(U[4]), NLUTS, _ptr(sel), _ptr(x), 3, _ptr(out), B, H), out, sent(3 * B)

    def coefficient_not_below_N():
        out, coef = sent(2 * B), np.array([0, p.N], dtype=np.uint32)
        return L.mkt_lut_bootstrap_at_batch(s.h, _ptr(T), NLUTS, _ptr(sel), _ptr(x), 0, _ptr(coef), 2, _ptr(out), B, H), out, sent(2 * B)

    def out_overlapping_lwe():
        buf = sent(2 * B)
        buf[:B] = x
        before = buf.copy()
        return L.mkt_lut_many_bootstrap_batch(s.h, _ptr(U[2]), NLUTS, _ptr(sel), _ptr(buf), 2, _ptr(buf), B, H), buf, before

    def unknown_mem():
        out = sent(B)
        return L.mkt_gate_batch(s.h, 0, _ptr(x), _ptr(y), _ptr(out), B, 2), out, sent(B)

    def rot_variant_23():
        return L.mkt_set_option(s.h, b"rot_variant", 23), None, None

    return [(f.__name__, f) for f in (bad_gate_code, index_outside_the_pool, selector_beyond_the_tables, nout_3, coefficient_not_below_N, out_overlapping_lwe,
                                      unknown_mem, rot_variant_23)]


@pytest.mark.parametrize("name", ["cggi", "kms", "x-kms"])
def test_refused_calls_leave_the_context_as_it_was(require_gpu, name):
    """between the first steps of the sequence: a bad gate code, an index outside the pool, a selector beyond the tables, nout = 3, a
    coefficient >= N, out overlapping lwe at nout = 2, an unknown mem, rot_variant = 23.  Each returns MKT_ERR_ARG, leaves an output filled
    with 0xA5A5A5A5 untouched, and the valid step after it gives the fresh context's words.  None of them reaches a kernel"""
    seq = K.sequence(name)
    s = K.new_scheme(name)
    st, B, mem = seq[0]
    run(s, name, st, B, mem, "before the first refusal")
    for j, (what, call) in enumerate(refusals(s, inputs(name))):
        rc, out, before = call()
        assert rc == ERR_ARG, (name, what, rc)
        assert _lib.lib().mkt_last_error(s.h), (name, what, "no message")
        assert out is None or np.array_equal(out, before), (name, what, "the output was written")
        st, B, mem = seq[j + 1]
        run(s, name, st, B, mem, f"after {what}")
    s.close()


# ---- e: the key set's life cycle ----
def load_piece(s, piece, party, crs, keys):
    k = keys[party] if party is not None else None
    if piece == "crs":
        s.load_crs(crs)
    elif piece == "rlk":
        s.load_party(party, rlk_d=k.rlk_d, rlk_f=k.rlk_f)
    else:
        s.load_party(party, **{piece: getattr(k, piece)})


def readiness(name, order, parties):
    """from an empty context, load the pieces of `order` one at a time for `parties`; before each load and after the last, every probe
    (gate, blindrotate_, keyswitch) is refused with MKT_ERR_STATE and check_ready's message for the first piece it misses, or -- once it
    misses none -- served with the fresh context's words -> the refusals met"""
    p, arith = K.set_of(name)
    crs, keys = K.keys_of(name)
    s = mk.Scheme(p, arith=arith)
    loaded, met = set(), set()

    def probe():
        for step, need_brk, need_ksk in K.PROBES:
            want = K.expected_refusal(p, loaded, need_brk, need_ksk)
            if want is None:
                run(s, name, STEP[step], 5, H, f"{step} with {sorted(map(str, loaded))}")
                continue
            with pytest.raises(mk.MktError) as e:
                STEP[step].fn(s, inputs(name), 5, H)
            assert e.value.code == ERR_STATE and want in str(e.value), (name, step, sorted(map(str, loaded)), str(e.value), "expected", want)
            met.add(want)

    for piece in order:
        for party in ([None] if piece == "crs" else parties):
            probe()
            load_piece(s, piece, party, crs, keys)
            loaded.add("crs" if piece == "crs" else (piece, party))
    probe()
    s.close()
    return met


def key_plain(name, seed):
    def keyed(s):
        crs, keys = K.keys_of(name, seed)
        if crs is not None:
            s.load_crs(crs)
        for i, kk in enumerate(keys):
            s.load_party(i, kk)
    return keyed


def secrets_of(name, seed):
    p = K.set_of(name)[0]
    crs = K.keys_of(name, seed)[0]
    return [mk.PartyKeys(p, party=i, crs=crs, secrets_only=True, deterministic_seed=seed) for i in range(p.nparty)]


def key_mixed(name, seed):
    """party 0 by load_party, the last party by keygen_device (the same party where there is one: generated over the loaded keys)"""
    def keyed(s):
        crs, keys = K.keys_of(name, seed)
        if crs is not None:
            s.load_crs(crs)
        last = len(keys) - 1
        for i, kk in enumerate(keys[:last] or keys):
            s.load_party(i, kk)
        s.keygen_device(last, secrets_of(name, seed)[last])
    return keyed


def key_seeded(name, seed):
    """every party by load_seeded: the public mask seed and the bodies, the masks regenerated on the GPU"""
    def keyed(s):
        p = K.set_of(name)[0]
        crs = K.keys_of(name, seed)[0]
        if crs is not None:
            s.load_crs(crs)
        for i in range(p.nparty):
            mk.load_seeded(s, i, mk.party_keygen_seeded(crs, p, party=i, mask_seed=bytes([seed + i] * 32), deterministic_seed=seed))
    return keyed


def made(name, keyed):
    """-> make(): an empty context of the set, keyed by `keyed` alone"""
    def make():
        p, arith = K.set_of(name)
        s = mk.Scheme(p, arith=arith)
        keyed(s)
        return s
    return make


def ksk_reload_behind_a_batch(s, name, want):
    """the context pinned to a fresh non-blocking stream: a device-memory gate_ops batch, the last party's key-switching key loaded again
    (load_party(ksk=...), the words it already holds) with no synchronisation in between, the batch again; both results are `want`, the
    fresh context's.  A GUARD, NOT A RACE DETECTOR: it passes whether or not the reload is ordered behind the first batch, as long as the
    copy happens to land outside the key switch.  That mkt_load_ksk IS ordered -- it zeroes and fills the table on the context's stream and
    drains it, where it once used the NULL stream, which a non-blocking stream does not wait for -- is an argument made by reading
    context.cpp.  The operands are held here until the stream is drained: the batch reads them after the calls have returned"""
    import torch
    i, B = inputs(name), 33
    party = i.p.nparty - 1
    ksk = s.get_ksk(party)
    ops, x, y = to_mem(i.ops[:B], D), to_mem(i.x[:B], D), to_mem(i.y[:B], D)
    stream = torch.cuda.Stream()                # torch creates its streams non-blocking
    torch.cuda.synchronize()                    # the operands are there before the pinned stream reads them
    s.set_stream(stream.cuda_stream)
    first = s.gate_ops(ops, x, y)
    s.load_party(party, ksk=ksk)
    second = s.gate_ops(ops, x, y)
    s.synchronize()
    s.set_stream(None)
    assert same_words(host_words(first), want), (name, "the batch before the key-switching key was loaded again")
    assert same_words(host_words(second), want), (name, "the batch after the key-switching key was loaded again")
    assert np.array_equal(s.get_ksk(party), ksk)


@pytest.mark.parametrize("name", ["cggi", "kms", "ccs", "x-kms"])
def test_key_set_life_cycle(require_gpu, name):
    """READINESS: the pieces one at a time in the order ksk, crs, pubkey, rlk, brk, the last party first -- and, so that every line of
    check_ready is the first to refuse at some point, also in the reverse order, the first party first: every refusal is MKT_ERR_STATE
    with check_ready's message, keyswitch is served as soon as every key-switching key is there, blindrotate_ as soon as everything but
    them is.  RELOAD: keys of another seed over the resident ones, party by party, then mixed loading routes (load_party, keygen_device,
    load_seeded): the words of a fresh context that only ever saw those keys.  Then a key-switching key loaded again between two batches on a
    pinned non-blocking stream (ksk_reload_behind_a_batch: a guard, not a race detector).  IMMUTABILITY: after fork() every loading call and
    mkt_set_twiddles return MKT_ERR_STATE on parent and fork, and both still serve gates"""
    p, arith = K.set_of(name)
    gate = STEP["gate"]
    parties = list(range(p.nparty))
    met = readiness(name, K.pieces_of(p), parties[::-1]) | readiness(name, K.pieces_of(p)[::-1], parties)
    lines = {"bootstrapping key not loaded", "key-switching key not loaded"} | ({"crs not loaded"} if p.multikey else set()) | \
        ({"public key not loaded"} if p.scheme == mk.CCS else set()) | ({"rlk / public key not loaded"} if p.scheme in (mk.KMS, mk.KMS_BLOCK) else set())
    assert met == lines, (name, "refusals of check_ready met", sorted(met))

    # reload: A, then B over it, then the mixed routes; the inputs stay those of seed 1 (any words are an input)
    s = K.new_scheme(name, 1)
    run(s, name, gate, 33, D, "keys A")
    rounds = [("B, party by party", 2, key_plain(name, 2)), ("C: load_party and keygen_device", 3, key_mixed(name, 3))]
    if name in ("cggi", "kms"):
        rounds.append(("D: load_seeded", 4, key_seeded(name, 4)))
    for how, seed, keyed in rounds:
        keyed(s)
        for B, mem in ((5, H), (33, D)):
            got = host_words(gate.fn(s, inputs(name), B, mem))
            assert same_words(got, fresh_step(name, gate, B, mem, seed, made(name, keyed), how)), (name, "reloaded with keys", how, B)
        assert not same_words(got, fresh_step(name, gate, 33, D)), (name, how, "the reloaded keys give the words of keys A")
        if name == "x-kms":       # the transform maximum is an atomic maximum over every upload of the context: never below a fresh context's
            f = made(name, keyed)()
            kmax = f.get_metric("fx_kmax")
            f.close()
            assert s.get_metric("fx_kmax") >= kmax > 0, (how, s.get_metric("fx_kmax"), kmax)
            assert s.last_kernel_name() in ("fx_blindrotate_kernel", "exact_kms_phase1_p2pf_kernel"), s.last_kernel_name()
    seed, keyed, how = rounds[-1][1], rounds[-1][2], rounds[-1][0]
    ksk_reload_behind_a_batch(s, name, fresh_step(name, STEP["gate_ops"], 33, D, seed, made(name, keyed), how))

    # immutability
    f = s.fork()
    crs, keys = K.keys_of(name, 1)
    tabs = K.make_twiddles(p.N)
    seeded0 = mk.party_keygen_seeded(crs, p, party=0, mask_seed=bytes([9] * 32), deterministic_seed=1)
    for who, c in (("parent", s), ("fork", f)):
        writes = [("load_party", lambda: c.load_party(0, keys[0])), ("keygen_device", lambda: c.keygen_device(0, secrets_of(name, 1)[0]))]
        if p.multikey:            # (a single-key context refuses a CRS as a bad argument, whoever shares its keys)
            writes.append(("load_crs", lambda: c.load_crs(crs)))
        if name in ("cggi", "kms"):
            writes.append(("load_seeded", lambda: mk.load_seeded(c, 0, seeded0)))
        for what, call in writes:
            with pytest.raises(mk.MktError) as e:
                call()
            assert e.value.code == ERR_STATE and "immutable" in str(e.value), (name, who, what, str(e.value))
        rc = K.set_twiddles(c, tabs)            # the Float64 tables: an EXACT context does not offer the call at all
        assert rc == (ERR_UNSUPPORTED if arith == mk.ARITH_EXACT else ERR_STATE), (name, who, "mkt_set_twiddles", rc)
        assert arith == mk.ARITH_EXACT or b"immutable" in _lib.lib().mkt_last_error(c.h)
        got = host_words(gate.fn(c, inputs(name), 5, H))
        assert same_words(got, fresh_step(name, gate, 5, H, seed, made(name, keyed), how)), (name, who, "a gate after the refused loads")
    f.close(); s.close()


# ---- f: tables and keys in either order ----
def test_tables_and_keys_in_either_order(require_gpu):
    """set kms (64-bit ring, Float64).  T' = the engine's tables with every entry of Psi from 4 on one ulp off (context_life_cases.tprime).
    Context P installs T', then the keys; context Q the keys, then T'.  Non-vacuity first: P's blindrotate_ words differ from a
    default-table context's (expected: on the 64-bit ring a Float64 product carries about eleven bits of rounding in every word).  THE LAW:
    Q gives P's words for blindrotate_ and gate, or the mkt_set_twiddles call on Q is refused with MKT_ERR_STATE.
    WHAT THIS FOUND: before the refusal was added Q did neither -- mkt_set_twiddles rebuilt the monomial table and left the bootstrapping key,
    public keys, rlk and CRS as transformed under the old tables (their integer form is not kept), and nothing refused.  mkt_set_twiddles
    now returns MKT_ERR_STATE ("install the tables before the keys") once any of them is loaded, and leaves the context as it was"""
    name = "kms"
    p, arith = K.set_of(name)
    crs, keys = K.keys_of(name)
    rot, gate = STEP["blindrotate"], STEP["gate"]
    tabs = K.tprime(p.N)

    def words(s):
        return host_words(rot.fn(s, inputs(name), 5, H)), host_words(gate.fn(s, inputs(name), 5, D))

    P = mk.Scheme(p, arith=arith)
    assert K.set_twiddles(P, tabs) == 0, _lib.lib().mkt_last_error(P.h)
    assert all(np.array_equal(P.twiddles(w), tabs[w]) for w in range(4)), "T' is installed"
    key_plain(name, 1)(P)
    p_rot, p_gate = words(P)
    P.close()
    d_rot, d_gate = fresh_step(name, rot, 5, H), fresh_step(name, gate, 5, D)
    assert not same_words(p_rot, d_rot), "T' gives the default tables' accumulators: the test would hold nothing"

    Q = made(name, key_plain(name, 1))()
    rc = K.set_twiddles(Q, tabs)
    q_rot, q_gate = words(Q)
    if rc == 0:
        assert same_words(q_rot, p_rot) and same_words(q_gate, p_gate), "tables after keys: neither P's words nor a refusal"
    else:
        assert rc == ERR_STATE and b"install the tables before the keys" in _lib.lib().mkt_last_error(Q.h), (rc, _lib.lib().mkt_last_error(Q.h))
        assert all(np.array_equal(Q.twiddles(w), t) for w, t in enumerate(K.make_twiddles(p.N))), "a refused call changed the tables"
        assert same_words(q_rot, d_rot) and same_words(q_gate, d_gate), "a refused call changed the context"
    # the key-switching key is integer data: it does not stand in the way of the tables
    R = mk.Scheme(p, arith=arith)
    for i, kk in enumerate(keys):
        R.load_party(i, ksk=kk.ksk)
    assert K.set_twiddles(R, tabs) == 0
    R.load_crs(crs)
    for i, kk in enumerate(keys):
        R.load_party(i, brk=kk.brk, rlk_d=kk.rlk_d, rlk_f=kk.rlk_f, pubkey=kk.pubkey)
    r_rot, r_gate = words(R)
    assert same_words(r_rot, p_rot) and same_words(r_gate, p_gate), "key-switching key, tables, then the other keys"
    Q.close(); R.close()


# ---- g: logical shards across calls ----
def test_logical_shards_across_calls(require_gpu):
    """three logical shards over one device's key set (setup_multi(p, [0, 0, 0])) on set kms make the evaluator's calls in sequence at
    B = 2 (one shard empty), 70, 1, 7, host arrays and GPU tensors alternating: each result is the single context's fresh words"""
    import torch
    name = "kms"
    p, arith = K.set_of(name)
    crs, keys = K.keys_of(name)
    multi = mk.setup_multi(p, [0, 0, 0], keys=keys, a=crs, arith=arith)
    j = 0
    for B in (2, 70, 1, 7):
        for step in ("gate", "gate_ops", "gate3_ops", "mux", "bootstrap", "not", "blindrotate", "keyswitch", "lut_bootstrap", "lut_many_bootstrap", "lut_bootstrap_at"):
            mem = (H, D)[j % 2]
            j += 1
            torch.cuda.synchronize()        # the shards run on their own streams: the tensors are there before they read
            got = host_words(STEP[step].fn(multi, inputs(name), B, mem))
            assert same_words(got, fresh_step(name, STEP[step], B, mem)), (step, B, "host" if mem == H else "device")
    multi.close()
