"""mkt_pack_batch at the shapes tests/test_gpu_pack.py does not run (tests/pack_cases.py; tests/test_pack_shapes_cpu.py vouches for the
restatement there): every instantiation of the product kernel -- workgroups of 4, 8, 16 threads and of 2, 4, 8 waves, the 64-bit ring with RLWE
length 2 and 3 --, more than one launch sequence of PACK_CHUNK = 16 packs, more than one chunk of PACK_EXACT_COLS = 64 columns in EXACT mode,
the edges of the PACK_TILE = 64 transpose, and the out= argument.  Every comparison is np.array_equal against tests/ref_pack.py.

The pools, the batches and the ways of picking rows are those of tests/test_gpu_pack.py (crafted_pool, run_batches), imported.  Where a test
needs boundary words in columns crafted_pool does not plant (the columns beside a chunk cut, the body), `planting` puts them into the pools
run_batches makes."""
import numpy as np
import pytest

import ref_pack as RP
import test_gpu_pack as TP
from helpers import mk
from helpers import to_device as _dev
from pack_cases import (EXACT_COLUMN_SETS, EXACT_GADGETS, EXACT_NOISE_FREE_SET, KERNEL_SETS, SEQUENCE_EXACT_GADGET, SEQUENCE_SETS, TILE_SETS, sid)
from test_gpu_pack import crafted_pool, edge_words, pack_setup, run_batches

pytestmark = pytest.mark.gpu
PACK_CHUNK = 16          # packs per launch sequence (context.cpp)


def planted(cols):
    """crafted_pool, and on top the boundary words of edge_words down the given columns: row j gets word j + c in the c-th column, for as
    many rows as there are words, from row 0 on (the rows every batch of run_batches without an index array reads)"""
    def make(p, rows, l, logB, rng):
        pool = crafted_pool(p, rows, l, logB, rng)
        e = edge_words(l, logB)
        for c, col in enumerate(cols):
            m = min(rows, len(e))
            pool[:m, col] = np.roll(e, -c)[:m]
        return pool
    return make


@pytest.fixture
def planting(monkeypatch):
    """planting(cols): run_batches builds its pool with planted(cols) for the rest of the test"""
    return lambda cols: monkeypatch.setattr(TP, "crafted_pool", planted(cols))


def words(p, x):
    return x.cpu().numpy().view(p.ring_dtype) if hasattr(x, "is_cuda") else x


@pytest.mark.parametrize("p,gadget", KERNEL_SETS, ids=[sid(p) for p, _ in KERNEL_SETS])
def test_every_product_kernel_equals_the_restatement(require_gpu, p, gadget):
    """one row, then a full pack followed by a pack of one row, at every (LOGM, WORD, NP).  From N = 1024 on the workgroup has more than one
    wave: the barriers between the l forward and NP inverse transforms of one mask word, and of the next, are what these sizes are for"""
    N, (l, logB) = p.N, gadget
    keys, pks, sch = pack_setup(p, l, logB)
    rng = np.random.default_rng([N, p.W, p.k, p.scheme])
    run_batches(p, sch, pks, l, logB, False, (1, N + 1), rng)
    if N >= 1024:
        # the comparison sees one mask word: the restatement of a pool that differs in bit 31 of one word (the top digit of every gadget) differs
        pool = crafted_pool(p, N + 1, l, logB, rng)
        got = mk.pack(sch, pool)
        want = RP.pack(p, pool, pks, l, logB).astype(p.ring_dtype)
        assert np.array_equal(got, want)
        other = pool[:N].copy()
        other[N // 2 + 3, p.lwe_len - 2] ^= 0x80000000
        assert not np.array_equal(got[0], RP.pack(p, other, pks, l, logB).astype(p.ring_dtype)[0])
    sch.close()


def sequence_calls(p, sch, pks, l, logB, exact, sizes):
    """the calls of test_launch_sequences, in the order of `sizes`, on one context.  One restatement serves them all: R, the rows picked, is
    the same for every way of picking -- R as its own pool without an index; a pool without the repeated rows and an index array that repeats
    five of them (seven in a call of three sequences); a shuffled pool and the permutation that undoes the shuffle -- and a shorter call is a
    prefix of it (its last, ragged pack restated alone)"""
    N = p.N
    Bmax = max(sizes)
    rng = np.random.default_rng([N, p.W, l, logB])
    # the repeats: five in the first 16 N + 1 rows -- in the first pack, across the first pack's end, on both sides of the first sequence's end --
    # and, in a longer call, one in the third sequence and the last row
    at = sorted({3, N - 1, N, PACK_CHUNK * N - 1, PACK_CHUNK * N} | ({2 * PACK_CHUNK * N + 5, Bmax - 1} if Bmax > PACK_CHUNK * N + 1 else set()))
    base = crafted_pool(p, Bmax - len(at), l, logB, rng)
    rep = np.arange(base.shape[0], dtype=np.uint32)
    for i, pos in enumerate(at):
        rep = np.insert(rep, pos, (7 * i + 11) % base.shape[0])
    assert rep.size == Bmax and np.unique(rep).size == base.shape[0] and sum(pos <= PACK_CHUNK * N for pos in at) == 5
    R = base[rep]
    sigma = rng.permutation(Bmax)
    shuffled, undo = R[sigma], np.argsort(sigma).astype(np.uint32)
    assert np.array_equal(shuffled[undo], R) and not np.array_equal(shuffled, R)
    full = RP.pack(p, R, pks, l, logB, exact=exact).astype(p.ring_dtype)

    def want(rows, B):
        g = B // N
        return full[:g] if B % N == 0 else np.concatenate([full[:g], RP.pack(p, rows[g * N:B], pks, l, logB, exact=exact).astype(p.ring_dtype)])

    device = False
    for B in sizes:
        w = want(R, B)
        ways = [("none", R[:B], None)]
        if B > PACK_CHUNK * N:
            ways += [("repeat", base, rep[:B]), ("perm", shuffled, undo[:B])]
        for kind, pool, idx in ways:
            device = not device                                              # host arrays and device tensors in turn
            got = mk.pack(sch, _dev(pool), None if idx is None else _dev(idx)) if device else mk.pack(sch, pool, idx)
            got = words(p, got)
            assert got.shape == w.shape and np.array_equal(got, w), (B, kind, "device" if device else "host")
        if B > PACK_CHUNK * N:
            # a device index beyond the pool, in the second sequence: the call with that entry clamped to the last row of the pool
            clamp_at = min(B - 1, PACK_CHUNK * N + 5)
            bad, clamped = undo[:B].copy(), undo[:B].copy()
            bad[clamp_at], clamped[clamp_at] = Bmax + 9, Bmax - 1
            got = words(p, mk.pack(sch, _dev(shuffled), _dev(bad)))
            assert np.array_equal(got, mk.pack(sch, shuffled, clamped)), (B, "clamped")
            rows = shuffled[clamped]
            g = clamp_at // N
            w2 = w.copy()
            w2[g] = RP.pack(p, rows[g * N:min((g + 1) * N, B)], pks, l, logB, exact=exact).astype(p.ring_dtype)[0]
            assert np.array_equal(got, w2) and not np.array_equal(got[g], w[g]), (B, "clamped, against the restatement")


@pytest.mark.parametrize("p,gadget", SEQUENCE_SETS, ids=[sid(p) for p, _ in SEQUENCE_SETS])
def test_launch_sequences(require_gpu, p, gadget):
    """B = 1, 16 N (exactly one sequence), 16 N + 1 (the second holds one row), 33 N + 1 (three sequences, the last of two packs, one ragged), 1
    again, on one context: the row arithmetic g = pack0 + blockIdx.z, the output offset g0 * ctb, the reuse of the column and slab workspace by
    the next sequence, its growth from 1 to 16 packs on a live context.  A second context makes 33 N + 1 its first call"""
    N, (l, logB) = p.N, gadget
    keys, pks, sch = pack_setup(p, l, logB)
    sizes = (1, PACK_CHUNK * N, PACK_CHUNK * N + 1, (2 * PACK_CHUNK + 1) * N + 1, 1)
    sequence_calls(p, sch, pks, l, logB, False, sizes)
    sch.close()
    fresh = pack_setup(p, l, logB)[2]
    sequence_calls(p, fresh, pks, l, logB, False, ((2 * PACK_CHUNK + 1) * N + 1,))
    fresh.close()


@pytest.mark.parametrize("p", [p for p, _ in SEQUENCE_SETS], ids=[sid(p) for p, _ in SEQUENCE_SETS])
def test_launch_sequences_exact(require_gpu, p):
    """MKT_ARITH_EXACT past one sequence: the per-pack loop over a.out + g * ctb and the columns of pack g of the second sequence"""
    N, (l, logB) = p.N, SEQUENCE_EXACT_GADGET
    keys, pks, sch = pack_setup(p, l, logB, arith=mk.ARITH_EXACT)
    sequence_calls(p, sch, pks, l, logB, True, (1, PACK_CHUNK * N + 1, 1))
    sch.close()


def chunk_cut_columns(p):
    """columns 63, 64 and n - 1 of every party's block: both sides of the cut after PACK_EXACT_COLS = 64 columns, and the last of a ragged chunk"""
    return sorted({i * p.n + q for i in range(p.nparty) for q in (63, 64, p.n - 1) if q < p.n})


@pytest.mark.parametrize("p", EXACT_COLUMN_SETS, ids=[sid(p) for p in EXACT_COLUMN_SETS])
def test_exact_column_chunks(require_gpu, planting, p):
    """EXACT mode decomposes and multiplies 64 columns per launch: the key offset of the second and third chunk and a ragged count, against the
    schoolbook product"""
    planting(chunk_cut_columns(p))
    for l, logB in EXACT_GADGETS:
        keys, pks, sch = pack_setup(p, l, logB, arith=mk.ARITH_EXACT)
        run_batches(p, sch, pks, l, logB, True, (1, p.N + 1), np.random.default_rng([p.n, p.k, l]))
        sch.close()


def test_exact_noise_free_key_past_one_column_chunk(require_gpu):
    """the identity of test_gpu_pack.test_exact_noise_free_key_gives_the_recomposed_phase at n = 65: with sigma_ring = 0, phase(pack(x)) minus the
    LWE phase of row j is sum_q s[q] (recomposed(a_q) - a_q) word for word.  Noise-free key rows of equal key bits open alike, so the identity
    tells a column multiplied with another column's key rows only where the two key bits differ: the key is chosen with s[0] != s[64], column
    64 under the key rows of column 0 being what the key offset without its q0 term gives"""
    p = EXACT_NOISE_FREE_SET
    for l, logB in ((4, 4), (3, 5), (8, 4)):
        keys, pks, sch = pack_setup(p, l, logB, arith=mk.ARITH_EXACT, seed=86)          # this key: s[0] = 0, s[63] = s[64] = 1
        rows = planted(chunk_cut_columns(p))(p, p.N, l, logB, np.random.default_rng(5))
        ct = mk.pack(sch, rows)
        ph = mk.rlwe_phase(ct[0], keys, p)
        s = np.concatenate([np.asarray(k.lwekey, dtype=np.uint32) for k in keys])
        assert s[63] == 1 and s[64] == 1 and s[0] == 0, "a key bit on either side of the chunk cut, none at column 0"
        want = ((RP.recomposed(p, rows[:, :-1], l, logB) - rows[:, :-1]) * s).sum(-1, dtype=np.uint32)
        assert np.array_equal((ph - RP.lwe_phase(p, rows, [k.lwekey for k in keys])).astype(np.uint32), want), (l, logB)
        if l * logB == 32:
            assert not want.any()
        sch.close()


@pytest.mark.parametrize("p,gadget", TILE_SETS, ids=[sid(p) for p, _ in TILE_SETS])
def test_column_tiles(require_gpu, planting, p, gadget):
    """the transpose at lwe_len = 64 and 65 and at N below the tile, one row short of a pack, a full pack, one row past it; boundary words in
    the first and the last mask word (crafted_pool) and in the body"""
    N, (l, logB) = p.N, gadget
    planting([0, p.lwe_len - 2, p.lwe_len - 1])
    keys, pks, sch = pack_setup(p, l, logB)
    run_batches(p, sch, pks, l, logB, False, (N - 1, N, N + 1), np.random.default_rng([N, p.lwe_len]))
    sch.close()


def test_out_argument(require_gpu):
    """mk.pack(..., out=buf) writes buf and returns it, on the host and on the device; a wrong shape raises before anything runs; a buf that
    overlaps the rows is refused by the library (MKT_ERR_ARG); a refused buf is as it was"""
    import torch
    p, (l, logB) = mk.KMS2party.scaled(n=5, N=64), (4, 4)
    keys, pks, sch = pack_setup(p, l, logB)
    B = p.N + 2                                                           # an even count of 32-bit words: the 64-bit views below stay aligned
    rows = crafted_pool(p, B, l, logB, np.random.default_rng(12))
    want = RP.pack(p, rows, pks, l, logB).astype(p.ring_dtype)
    assert np.array_equal(mk.pack(sch, rows), want)
    shape = (2, p.k + 1, p.N)
    # host
    buf = np.full(shape, 0xA5, dtype=p.ring_dtype)
    assert mk.pack(sch, rows, out=buf) is buf and np.array_equal(buf, want)
    idx = np.arange(B, dtype=np.uint32)[::-1].copy()
    assert mk.pack(sch, rows, idx, out=buf) is buf and np.array_equal(buf, RP.pack(p, rows[idx], pks, l, logB).astype(p.ring_dtype))
    # device
    rows_d = _dev(rows)
    buf_d = torch.full(shape, 0x5A, dtype=torch.int64, device="cuda")
    assert mk.pack(sch, rows_d, out=buf_d) is buf_d and np.array_equal(words(p, buf_d), want)
    # wrong shapes: one pack too few, one too many, a polynomial too few, flat
    for bad in ((1, p.k + 1, p.N), (3, p.k + 1, p.N), (2, p.k, p.N), (2 * (p.k + 1) * p.N,)):
        b = np.full(bad, 0xA5, dtype=p.ring_dtype)
        with pytest.raises(ValueError):
            mk.pack(sch, rows, out=b)
        assert (b == 0xA5).all()
        b_d = torch.full(bad, 0x5A, dtype=torch.int64, device="cuda")
        with pytest.raises(ValueError):
            mk.pack(sch, rows_d, out=b_d)
        assert (b_d == 0x5A).all()
    # out overlapping the rows: one allocation holds both, out begins inside the last row
    nout = int(np.prod(shape)) * 2                                        # 32-bit words of the output
    back = np.random.default_rng(13).integers(0, 2**32, rows.size + nout, dtype=np.uint64).astype(np.uint32)
    back[:rows.size] = rows.reshape(-1)
    off = rows.size - 2
    assert rows.size % 2 == 0
    for mem in ("host", "device"):
        store = back.copy() if mem == "host" else _dev(back)
        r = store[:rows.size].reshape(rows.shape)
        o = store[off:off + nout]
        o = o.view(p.ring_dtype).reshape(shape) if mem == "host" else o.view(torch.int64).reshape(shape)
        with pytest.raises(mk.MktError) as ei:
            mk.pack(sch, r, out=o)
        assert ei.value.code == -1, mem
        assert np.array_equal(store if mem == "host" else store.cpu().numpy().view(np.uint32), back), mem
        # the same allocation, out behind the rows: served
        o = store[rows.size:rows.size + nout]
        o = o.view(p.ring_dtype).reshape(shape) if mem == "host" else o.view(torch.int64).reshape(shape)
        assert np.array_equal(words(p, mk.pack(sch, r, out=o)), want), mem
    sch.close()
