"""The arena of tests/footprint.py on numpy memory, and its step list held to include/mktfhe.h (no GPU).

The arena must find what tests/test_gpu_footprint.py relies on it to find: one byte stored before, behind and between carvings; a store
into an input; a guard overwritten with a constant or with zeros -- and must not report a store into a declared output.  With its comparison
stubbed to "clean" the same stores go unseen, which test_a_stubbed_comparison_sees_nothing pins: the findings come from the comparison."""
import numpy as np
import pytest

import context_life_cases as K
import footprint as F
from footprint import Arena


def carved(layout):
    rng = np.random.default_rng(5)
    a = Arena(1 << 20, layout, device="numpy")
    src = [rng.integers(0, 256, 7, dtype=np.uint8),                                    # gate codes
           rng.integers(0, 1 << 32, (5, 13), dtype=np.uint64).astype(np.uint32),       # ciphertext rows
           rng.integers(0, 1 << 63, (3, 2, 256), dtype=np.uint64),                      # accumulators on the 64-bit ring
           (rng.standard_normal((2, 3000)) + 1j * rng.standard_normal((2, 3000))).astype(np.complex128),   # a row longer than 4 KiB
           rng.integers(0, 1 << 32, 9, dtype=np.uint64).astype(np.uint32)]
    return a, src, [a.carve(x) for x in src]


@pytest.mark.parametrize("layout", F.LAYOUTS)
def test_carvings_hold_their_words_between_guards(layout):
    a, src, views = carved(layout)
    assert a.check() == []
    end = 0
    for j, (c, x, v) in enumerate(zip(a.carvings, src, views)):
        assert v.dtype == x.dtype and v.shape == x.shape and np.array_equal(v, x) and np.array_equal(c.source, x)
        row = int(np.prod(x.shape[1:])) * x.dtype.itemsize
        assert c.guard >= max(4096, row) and c.size == x.nbytes
        gap = c.offset - end
        assert gap >= c.guard and (j == 0 or gap >= a.carvings[j - 1].guard), "a guard as long as either neighbour's largest row"
        assert np.array_equal(a.buf[end:c.offset], a.fill[end:c.offset])
        addr = a.base + c.offset
        assert addr % x.dtype.itemsize == 0
        if layout == "aligned":
            assert addr % 256 == 0
        end = c.offset + c.size
    assert a.nbytes - end >= a.carvings[-1].guard
    if layout == "packed":
        phase = [(a.base + c.offset) % 16 for c in a.carvings]
        assert phase[0] == 1 and phase[1] == 8 and phase[2] == 8 and phase[3] == 0 and phase[4] == 4, phase      # k * alignment mod 16, k = 1, 2, ...
        more = [a.carve(np.arange(3, dtype=np.uint32)) for _ in range(4)]
        assert {(a.base + c.offset) % 16 for c in a.carvings if c.source.dtype == np.uint32} == {0, 4, 8, 12}, "32-bit words meet all four phases"
        assert a.check() == [] and len(more) == 4
    assert len(np.unique(a.fill)) == 256, "the fill is no constant"


@pytest.mark.parametrize("layout", F.LAYOUTS)
def test_stray_stores_are_found_and_declared_outputs_are_not(layout):
    a, src, views = carved(layout)
    c = a.carvings
    spots = {"before the first": c[0].offset - 1, "behind the first": c[0].offset + c[0].size, "between": (c[1].offset + c[1].size + c[2].offset) // 2,
             "one row behind": c[3].offset + c[3].size + 3000 * 16 - 1, "one row before": c[3].offset - 3000 * 16,
             "behind the last": c[4].offset + c[4].size, "the arena's first byte": 0, "the arena's last byte": a.nbytes - 1}
    for what, off in spots.items():
        keep = a.buf[off]
        a.buf[off] ^= 0x40
        got = a.check(written=[views[1]])
        assert len(got) == 1 and got[0][0] == "guard written" and got[0][2] == off and got[0][3] == 1, (what, got)
        a.buf[off] = keep
        assert a.check() == []
    # a store into an input is found, with the carving; the same store into a declared output is not
    views[2][1, 1, 7] ^= np.uint64(1) << np.uint64(40)
    got = a.check(written=[views[1]])
    assert len(got) == 1 and got[0][:2] == ("input written", 2) and got[0][2] == c[2].offset + (3 * 256 + 7) * 8 + 5 and got[0][3] == 1, got
    assert a.check(written=[views[2]]) == [] and a.check(written=(views[0], [views[2], None])) == []
    views[1][...] = 0
    assert a.check(written=[views[1], views[2]]) == []
    assert [g[:2] for g in a.check(written=[views[2]])] == [("input written", 1)]
    # a guard filled with a constant, and with zeros: the fill is neither
    for const in (0xA5, 0):
        lo = c[1].offset + c[1].size
        keep = a.buf[lo:lo + 64].copy()
        a.buf[lo:lo + 64] = const
        got = a.check(written=[views[1], views[2]])
        # (one byte of the fill in 256 is the constant itself, and splits the run)
        assert got and all(g[0] == "guard written" and lo <= g[2] < lo + 64 for g in got) and 56 <= sum(g[3] for g in got) <= 64, (const, got)
        a.buf[lo:lo + 64] = keep
    with pytest.raises(AssertionError):
        a.check(written=[np.zeros(4, dtype=np.uint32)])       # what the call returned must be a carving
    a.reset()
    assert a.check() == [] and not a.carvings and np.array_equal(a.buf, a.fill)


def test_a_stubbed_comparison_sees_nothing(monkeypatch):
    """the detector is the comparison: stubbed to "clean", a stray store and a written input pass"""
    a, src, views = carved("packed")
    a.buf[a.carvings[0].offset - 1] ^= 1
    views[4][0] ^= 1
    assert len(a.check()) == 2
    monkeypatch.setattr(Arena, "_differs", lambda self: np.zeros(self.nbytes, dtype=bool))
    assert a.check() == []


def test_every_entry_point_of_the_header_has_a_footprint_step():
    """FOOTPRINT_STEPS is context_life_cases.STEPS -- which tests/test_context_life_cpu.py holds to the batch entry points of include/mktfhe.h --
    plus the pack call of include/mktfhe_pack.h: a new entry point cannot join the header without joining tests/test_gpu_footprint.py"""
    assert F.FOOTPRINT_STEPS[:len(K.STEPS)] == K.STEPS and [st.entry for st in F.FOOTPRINT_STEPS[len(K.STEPS):]] == ["mkt_pack_batch"]
    assert len({st.name for st in F.FOOTPRINT_STEPS}) == len(F.FOOTPRINT_STEPS)
    import re
    from helpers import ROOT
    import os
    pack_h = open(os.path.join(ROOT, "include", "mktfhe_pack.h")).read()
    batch = set(re.findall(r"\b(mkt_\w*batch\w*)\s*\(", pack_h))
    assert batch == {"mkt_pack_batch"}, batch
    for name in K.SETS:
        p, arith = K.set_of(name)
        assert [st.name for st in F.FOOTPRINT_STEPS if st.applies(p, arith)][:-1] == [st.name for st in K.steps_of(name)]
