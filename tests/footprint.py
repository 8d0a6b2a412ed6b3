"""WHERE a call writes (tests/test_gpu_footprint.py; the arena's own test is tests/test_footprint_cpu.py).

Every other GPU test pins the words a call returns.  A launcher whose last workgroup is ragged can store a row past the end of its buffer and
still return every expected word: with device arguments the store lands in the caller's neighbouring tensor, which torch's allocator carved
from the same block, and nothing faults.  An Arena puts every device tensor of a call into ONE flat byte buffer filled with seeded
pseudo-random bytes -- a stray store of a constant or of zeros cannot coincide with it -- each carving between guards at least as long as its
own largest row (and never under 4 KiB), so that a store one whole row off either end still lands in a guard.  After the call, check() compares
the whole buffer with what it must hold: the fill outside the carvings, the source words in every carving the call was not to write.

Two layouts.  "aligned": every carving starts at a multiple of 256 bytes, what torch's allocator gives.  "packed": every carving starts at
the alignment of its element type and no more (1 byte for uint8 codes, 4 / 8 for 32- / 64-bit words, 16 for complex Float64), successive
carvings walking through the 16-byte phases their element size allows, the first one off the 16-byte boundary wherever its type permits --
the contract include/mktfhe.h states under ALIGNMENT.

The buffer is a torch.uint8 CUDA tensor (the comparison then runs on the device: one expected image of the arena, one mask, no per-byte host
loop) or, for the CPU test, a numpy array handled by the same code."""
import contextlib

import numpy as np

import context_life_cases as K
import helpers
import pack_cases as PC
from helpers import mk

MIN_GUARD = 4096
LAYOUTS = ("aligned", "packed")
_SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def alignment_of(dtype):
    """what the packed layout gives a carving of this element type: the element size (complex Float64: 16)"""
    return np.dtype(dtype).itemsize


def guard_of(shape, dtype):
    """the guard on either side of a carving: its largest row -- the product of all but the first dimension times the element size -- and at least 4 KiB"""
    row = int(np.prod(shape[1:], dtype=np.int64)) * np.dtype(dtype).itemsize if len(shape) else np.dtype(dtype).itemsize
    return max(MIN_GUARD, row)


class Carving:
    def __init__(self, offset, size, guard, source, view):
        self.offset, self.size, self.guard, self.source, self.view = offset, size, guard, source, view

    def __repr__(self):
        return f"carving at {self.offset}, {self.size} bytes, {self.source.dtype}{list(self.source.shape)}"


def _addr(x):
    return int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x.__array_interface__["data"][0])


def flatten(result):
    """the tensors / arrays in what a step returned (one, or tuples and lists of them; None and plain numbers are skipped)"""
    if isinstance(result, (tuple, list)):
        return [t for r in result for t in flatten(r)]
    return [result] if hasattr(result, "data_ptr") or isinstance(result, np.ndarray) else []


class Arena:
    """nbytes of memory on `device` ("cuda": torch; "numpy": host), filled from `seed`; layout one of LAYOUTS"""

    def __init__(self, nbytes, layout, device="cuda", seed=2024):
        assert layout in LAYOUTS and nbytes % 256 == 0
        self.layout, self.nbytes, self.gpu = layout, nbytes, device != "numpy"
        fill = np.random.default_rng([seed, nbytes]).integers(0, 256, nbytes, dtype=np.uint8)
        if self.gpu:
            import torch
            self.torch = torch
            self.fill = torch.from_numpy(fill).to(device)
            self.buf, self.expect, self.own = self.fill.clone(), self.fill.clone(), torch.zeros(nbytes, dtype=torch.bool, device=device)
        else:
            self.fill = fill
            self.buf, self.expect, self.own = fill.copy(), fill.copy(), np.zeros(nbytes, dtype=bool)
        self.base = _addr(self.buf)
        self.reset(refill=False)

    def reset(self, refill=True):
        """forget every carving; the arena holds the fill again"""
        if refill:
            if self.gpu:
                self.buf.copy_(self.fill); self.expect.copy_(self.fill); self.own.zero_()
            else:
                self.buf[:] = self.fill; self.expect[:] = self.fill; self.own[:] = False
        self.carvings, self.cursor, self.last_guard, self.k = [], 0, 0, 0

    def _place(self, size, guard, align):
        lo = self.cursor + max(guard, self.last_guard)          # the first byte this carving may start at
        self.k += 1
        if self.layout == "aligned":
            phase, period = 0, 256
        else:
            phase, period = (self.k * align) % 16 if align < 16 else 0, max(16, align)
        start = lo + (phase - (self.base + lo)) % period
        assert (self.base + start) % align == 0
        assert start + size + guard <= self.nbytes, f"arena of {self.nbytes} bytes is too small for {len(self.carvings) + 1} carvings (needs {start + size + guard})"
        self.cursor, self.last_guard = start + size, guard
        return start

    def carve(self, a):
        """the host array's words copied into the arena -> a view of them with its dtype and shape (GPU: the signed torch type of the same size)"""
        a = np.ascontiguousarray(a)
        size = a.nbytes
        start = self._place(size, guard_of(a.shape, a.dtype), alignment_of(a.dtype))
        raw = a.reshape(-1).view(np.uint8)
        if self.gpu:
            signed = a.view(_SIGNED.get(a.dtype, a.dtype))
            view = self.buf[start:start + size].view(getattr(self.torch, str(signed.dtype))).view(tuple(a.shape))
            if size:
                view.copy_(self.torch.from_numpy(signed))
                self.expect[start:start + size].copy_(self.buf[start:start + size])
        else:
            self.buf[start:start + size] = raw
            self.expect[start:start + size] = raw
            view = self.buf[start:start + size].view(a.dtype).reshape(a.shape)
        self.own[start:start + size] = True
        self.carvings.append(Carving(start, size, guard_of(a.shape, a.dtype), a.copy(), view))
        return view

    def carve_empty(self, shape, dtype):
        """an output of a call: a carving whose source words are the bytes 0xA5"""
        a = np.empty(shape, dtype=dtype)
        a.reshape(-1).view(np.uint8)[...] = 0xA5
        return self.carve(a)

    def _differs(self):
        """the comparison itself: a mask over the arena, true where a byte is not what it must be"""
        return self.buf != self.expect

    def check(self, written=()):
        """-> findings, empty when all is well.  written: the tensors the call was to write (by address: each must be a carving).  A byte
        outside every carving that is not the fill, or a carving not in `written` that no longer holds its source words, is a finding:
        (kind, carving index or None, arena offset of the first such byte, how many bytes)"""
        starts = {self.base + c.offset: j for j, c in enumerate(self.carvings)}
        outs = set()
        for t in flatten(written):
            if t.size if isinstance(t, np.ndarray) else t.numel():
                assert _addr(t) in starts, ("a tensor the call returned does not start a carving of the arena", _addr(t) - self.base, self.carvings)
                outs.add(starts[_addr(t)])
        bad = self._differs()
        for j in outs:
            c = self.carvings[j]
            bad[c.offset:c.offset + c.size] = False
        if not bool(bad.any()):
            return []
        where = (bad.nonzero().reshape(-1).cpu().numpy() if self.gpu else np.nonzero(bad)[0]).astype(np.int64)
        findings = []
        for j, c in enumerate(self.carvings):
            hit = where[(where >= c.offset) & (where < c.offset + c.size)]
            if len(hit):
                findings.append(("input written", j, int(hit[0]), len(hit), repr(c)))
        own = (self.own.cpu().numpy() if self.gpu else self.own)
        out = where[~own[where]]
        if len(out):
            cuts = np.nonzero(np.diff(out) > 1)[0] + 1            # one finding per run of neighbouring bytes
            for run in np.split(out, cuts)[:16]:
                nearest = min(range(len(self.carvings)), key=lambda j: min(abs(int(run[0]) - self.carvings[j].offset), abs(int(run[0]) - self.carvings[j].offset - self.carvings[j].size)), default=None)
                c = self.carvings[nearest] if nearest is not None else None
                rel = "" if c is None else (f"{c.offset - int(run[0])} bytes before" if run[0] < c.offset else f"{int(run[0]) - c.offset - c.size} bytes behind") + f" {c!r}"
                findings.append(("guard written", None, int(run[0]), len(run), rel))
        return findings


# ---- a step's tensors in the arena ----
_EMPTY_USERS = ("scheme", "lut", "seeded", "seeded_keys", "decrypt", "pack")      # the modules that hold scheme._empty under their own name


@contextlib.contextmanager
def tensors_in(arena):
    """for the length of one call: helpers.device_tensor and mktfhe_amd.scheme._empty (wherever the binding's modules reach it: the one function
    through which it allocates an output "where x lives") carve from the arena"""
    import importlib
    import mktfhe_amd.scheme as S
    keep_dt, keep_empty = helpers.device_tensor, S._empty

    def empty(like, shape, dtype, tdtype=None):
        if not S._is_torch(like):
            return keep_empty(like, shape, dtype, tdtype)
        if tdtype is None:
            tdtype = str(like.dtype).split(".")[-1]
        return arena.carve_empty(tuple(int(v) for v in shape), np.dtype(tdtype))

    mods = [importlib.import_module("mktfhe_amd." + m) for m in _EMPTY_USERS]
    assert all(getattr(m, "_empty") is keep_empty for m in mods)
    helpers.device_tensor = arena.carve
    for m in mods:
        m._empty = empty
    try:
        yield arena
    finally:
        helpers.device_tensor = keep_dt
        for m in mods:
            m._empty = keep_empty


# ---- the steps: every batch entry point (context_life_cases.STEPS) and the pack call ----
BATCHES = (1, 5, 33, 64, 65)
# B = 5: a ragged workgroup under 2 and 4 rotations per workgroup; 33: one over the key switch's 32-group tile; 64 / 65: at and one over
# PR_TILE, PACK_TILE and the key switch's 64 lanes.  SE_SLOTS = 256 is a tile of 16-word mask blocks, not of rows (B rows have B ceil(n / 16)
# of them) inside tiles of up to 4096 output words, which no B here reaches: seeded_expand_batches adds the sizes round that tile.  The
# transforms run NBT = 1 per block unless MKT_FFT_NB says otherwise: tests/test_gpu_footprint.py runs them at NBT = 2 in a child process
def seeded_expand_tile_words(n, lwe_len):
    """seeded.hip seeded_expand_tile_words restated: the output words per tile of seeded_expand_kernel -- 4096, less where more than
    SE_SLOTS = 256 keystream blocks could begin in a window of that many words"""
    nb = (n + 15) // 16
    window = lambda L: (L // lwe_len) * nb + min((L % lwe_len) // 16 + 2, nb)      # noqa: E731
    tw = 4096
    while tw > 4 and window(tw + 15) > 256:
        tw -= 4
    return tw


def seeded_expand_batches(p):
    """the tile that BATCHES does not straddle: seeded_expand_kernel cuts its output into tiles of seeded_expand_tile_words words, over 120
    rows at every set here.  r = the rows that fit one tile: B = r (one tile, full or nearly), r + 1 (a second tile of one row or less:
    the ragged one), 2 r + 3 (a third)"""
    r = seeded_expand_tile_words(p.n, p.lwe_len) // p.lwe_len
    return (r, r + 1, 2 * r + 3)


PACK_COUNTS = lambda N: (1, 63, 64, 65, N + 1)      # noqa: E731


def _pack(s, i, B, mem):
    """mkt_pack_batch on the first B rows of the pool, picked by index"""
    return mk.pack(s, helpers.to_mem(i.x[:B], mem), helpers.to_mem(i.pack_idx[:B], mem))


FOOTPRINT_STEPS = list(K.STEPS) + [K.Step("pack", "mkt_pack_batch", _pack, lambda p, arith: True)]
PACK_SETS = [(PC.KERNEL_SETS[0], mk.ARITH_F64REF), ((PC.EXACT_COLUMN_SETS[0], PC.EXACT_GADGETS[0]), mk.ARITH_EXACT)]
