"""The case lists of tests/test_gpu_pack_shapes.py: the shapes of mkt_pack_batch (mktfhe_amd/csrc/pack.hip, the pack section of context.cpp)
that tests/test_gpu_pack.py does not reach.  tests/test_pack_shapes_cpu.py imports the same lists, holds the restatement (tests/ref_pack.py) to
the definition at every set named here, and asserts that KERNEL_SETS leaves no instantiation of the product kernel out.

The product kernel is pack_product_kernel<LOGM, WORD, NP>: LOGM = log2(N / 2) (4 .. 11 for N = 32 .. 4096), WORD the ring word (32 or 64 bits),
NP = 1 + the ring components a party's key covers (2 for the multi-key schemes, 1 + RLWE length otherwise); its workgroup has N / 8 threads."""
from helpers import mk

GADGETS = [(1, 16), (4, 4), (8, 4), (3, 5)]          # those of tests/test_gpu_pack.py


def sid(p):
    return f"{p.name}-n{p.n}-N{p.N}-k{p.k}-W{p.W}" + (f"-b{p.blk_len}x{p.blk_d}" if p.blk_len else "")


def kernel_key(p):
    """the instantiation (LOGM, W, NP) of pack_product_kernel a parameter set runs"""
    return p.N.bit_length() - 2, p.W, 2 if p.multikey else 1 + p.k


# ---- one set per instantiation that tests/test_gpu_pack.py does not run ----
# n = 5: one whole chunk of PACK_QCHUNK = 4 mask words and a ragged one, so the slab reducer adds two slabs.  N = 32, 64, 128: workgroups of
# 4, 8, 16 threads; N = 1024, 2048, 4096: 2, 4, 8 waves, two staging buffers and the guard barriers of fft_device.h.  The six CGGI sets at
# N = 256 and 512 are the instantiations that F64_SETS of tests/test_gpu_pack.py leaves out at its own ring sizes (the 64-bit ring with RLWE
# length 2 and 3, the 32-bit ring with length 3 at 256 and length 2 at 512).  The five sets after them run the multi-key slot rule (a party's
# polynomial 1 goes to ciphertext polynomial 1 + party) and the block schemes at the multi-wave sizes and at N = 32.
_GRID = [mk.CGGIparam.scaled(n=5, N=N, k=kr, W=W) for N in (32, 64, 128, 1024, 2048, 4096) for W in (32, 64) for kr in (1, 2, 3)]
_REST = [mk.CGGIparam.scaled(n=5, N=N, k=kr, W=W) for N, W, kr in ((256, 32, 3), (256, 64, 2), (256, 64, 3), (512, 32, 2), (512, 64, 2), (512, 64, 3))]
_MULTIKEY = [
    mk.KMS2party.scaled(n=5, N=1024, k=3),
    mk.KMS2party_N1024_l2.scaled(n=5),
    mk.CCS2party.scaled(n=5, N=2048),
    mk.KMS2partyblock.scaled(n=6, N=4096, blk_d=2),
    mk.Blockparam.scaled(n=6, N=32, blk_d=2),
]
# (parameter set, gadget): the gadgets dealt round-robin over the list; tests/test_pack_shapes_cpu.py asserts that all four occur at every N >= 1024
KERNEL_SETS = [(p, GADGETS[i % len(GADGETS)]) for i, p in enumerate(_GRID + _REST + _MULTIKEY)]

# ---- more than one launch sequence (PACK_CHUNK = 16 packs): N = 32 keeps 34 packs at 1089 rows ----
SEQUENCE_SETS = [(mk.CGGIparam.scaled(n=5, N=32), (8, 4)), (mk.KMS2party.scaled(n=5, N=32), (3, 5))]
SEQUENCE_EXACT_GADGET = (4, 4)

# ---- MKT_ARITH_EXACT past one chunk of PACK_EXACT_COLS = 64 columns: n = 64 one whole chunk, 65 a chunk of one column after it, 129 two whole
# chunks and one column; three key polynomials; two parties on the 64-bit ring ----
EXACT_COLUMN_SETS = [
    mk.CGGIparam.scaled(n=64, N=64),
    mk.CGGIparam.scaled(n=65, N=64),
    mk.CGGIparam.scaled(n=129, N=64),
    mk.CGGIparam.scaled(n=65, N=64, k=2),
    mk.KMS2party.scaled(n=65, N=64),
]
EXACT_GADGETS = [(4, 4), (3, 5)]
EXACT_NOISE_FREE_SET = mk.CGGIparam.scaled(n=65, N=64, beta=0.0)

# ---- the PACK_TILE = 64 tiles of pack_columns_kernel: lwe_len = 64 (the body is the last column of the first tile), 65 (the body alone in a
# second tile; with two parties the second party's block runs into it), N below the tile ----
TILE_SETS = [
    (mk.CGGIparam.scaled(n=63, N=64), (4, 4)),
    (mk.CGGIparam.scaled(n=64, N=64), (3, 5)),
    (mk.KMS2party.scaled(n=32, N=64), (8, 4)),
    (mk.CGGIparam.scaled(n=63, N=32), (1, 16)),
]
