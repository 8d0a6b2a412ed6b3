"""The case lists of tests/test_gpu_stream_order.py stay complete and its control cannot pass vacuously (no GPU): every step of
context_life_cases.STEPS -- one per batch entry point of include/mktfhe.h, tests/test_context_life_cpu.py -- is made behind the late producer
for every set it applies to, in both memory kinds and both ways of choosing the stream; the poison differs from the real words of every
per-row input; and the rule that sizes the delay (20 times the longest host enqueue time, floor, cap) is a pure function, held here on made-up
timings."""
import numpy as np
import pytest

import context_life_cases as K
import stream_cases as S
from helpers import mk


def test_every_step_is_made_behind_the_late_producer():
    assert S.SETS == list(K.SETS) and S.B == 33
    assert sorted(S.VARIANTS) == sorted((m, h) for m in (mk.MEM_DEVICE, mk.MEM_HOST) for h in (S.PINNED, S.TORCH))
    for name in K.SETS:
        got = S.cases(name)
        assert len(got) == len(set((st.name, m, h) for st, m, h in got)) == 4 * len(K.steps_of(name))
        for st in K.STEPS:
            mine = [(m, h) for s2, m, h in got if s2 is st]
            assert sorted(mine) == (sorted(S.VARIANTS) if st.applies(*K.SETS[name]) else []), (name, st.name)
    for st in K.STEPS:
        assert any(s2 is st for name in K.SETS for s2, _, _ in S.cases(name)), (st.name, "is made on no set")
    assert set(S.CONTROL_STEPS) == {"gate_ops", "transform_fwd"} and all(K.STEP[s].applies(*K.SETS[n]) for s in S.CONTROL_STEPS for n in K.SETS)
    assert all(K.STEP[s].applies(*K.SETS[n]) for s in S.FORK_STEPS for n in K.SETS) and set(S.KEY_SETS) <= set(K.SETS)
    assert S.SHARD_SET in K.SETS and all(s in K.STEP for s in S.SHARD_STEPS)


@pytest.mark.parametrize("name", list(K.SETS))
def test_poison_differs_from_every_per_row_input(name):
    """all-zero words against the B rows every step hands over: a field whose real words were zero could not show a read that came too
    early.  The host-side fields are make_inputs' own; at, bt, acc0 and tr come from the CPU references (stream_cases.host_inputs).  On
    the GPU, LateProducer.tensor asserts the same of every tensor it is actually given"""
    i = S.host_inputs(name, 2 * S.B)
    for k in K.PER_ROW:
        real = np.ascontiguousarray(getattr(i, k)[:S.B])
        assert real.shape[0] == S.B, (name, k)
        assert not np.array_equal(real.view(np.uint8), S.poison(real).view(np.uint8)), (name, k, "the real words are all zero")
        assert not S.poison(real).view(np.uint8).any()
    # the inputs that are not per row: tables, the pool, coefficients, the seeded keys
    for k in ("T", "pool", "coef", "brk_seeded", "ksk_seeded"):
        assert np.ascontiguousarray(getattr(i, k)).view(np.uint8).any(), (name, k)
    assert all(u.view(np.uint8).any() for u in i.U.values())
    # rows 33 .. 66, call B of the order test, are other rows than call A's
    w = K.window(i, S.B, 2 * S.B)
    assert w.n == S.B and w.ops.shape == (S.B,) and not np.array_equal(w.x, i.x[:S.B]) and not np.array_equal(w.y, i.y[:S.B])


def test_the_delay_rule():
    """20 times the longest host enqueue time, floored at 20 ms, capped at 250 ms; cycles rounded up"""
    assert S.delay_ms([0.1, 0.4, 0.2]) == 20.0                  # 8 ms: the floor
    assert S.delay_ms([1.0]) == 20.0 and S.delay_ms([1.0 + 2 ** -20]) > 20.0
    assert S.delay_ms([0.5, 3.0, 2.9]) == 60.0                  # the longest decides
    assert S.delay_ms([12.5]) == 250.0 and S.delay_ms([12.4]) == pytest.approx(248.0)
    assert S.delay_ms([400.0, 1.0]) == 250.0                    # the cap
    assert S.delay_cycles(20.0, 100000.0) == 2000000 and S.delay_cycles(20.0, 100000.01) == 2000001
    with pytest.raises(ValueError):
        S.delay_ms([])
