"""The device generator (mktfhe_amd/csrc/keygen.hip) against the host generator word for word -- BOTH keys, the exported
coefficient-form bootstrapping key and the key-switching key -- at every shape where its indexing changes: N below one workgroup
(idle lanes), both accumulator instantiations on both ring widths, several ring keys, every UniEnc depth, block schemes with the
LWE key spanning ring keys, n = 1, every key-switch gadget, a key-switch grid smaller than one block, two parties of one seed.
Then the exported keys of one set per scheme go through the independent opener and statistics of tests/ref_keys.py, so the
two-sided judgement of the device keys does not rest on client.cpp.

At the sets' own noise (sigma <= 2^17) the comparison cannot see the Gaussian deviate's last bits: rint(sigma g) absorbs them (a build
with contraction on changes a fifth of the deviates and not one of those words, tests/test_rng_cpu.py).  The wide-noise test makes the
same comparison at sigma = 2^55, where every noise word carries the deviate's mantissa: it is the test that holds "box_muller gives the
same bits on host and device" for keygen.hip's noise sites."""
import numpy as np
import pytest

from helpers import mk

pytestmark = pytest.mark.gpu

_RING = {32: mk.CGGIparam, 64: mk.KMS2party}          # an RGSW scheme on each ring width (l = 3)
SHAPES = (
    # N = 32 .. 4096 on both rings: N < 256 leaves lanes idle (one coefficient per lane at most), N <= 1024 takes the 4-register
    # accumulator, N > 1024 the 16-register one; at N = 32 the key-switching grid (32 lanes) is smaller than one block
    [_RING[W].scaled(n=3, N=N) for W in (32, 64) for N in (32, 64, 128, 256, 1024, 2048, 4096)] + [
        mk.CGGIparam.scaled(n=3, N=256, k=2), mk.CGGIparam.scaled(n=3, N=256, k=3), mk.CGGIparam.scaled(n=2, N=256, k=5),     # kr ring keys
        mk.CGGIparam.scaled(n=2, N=2048, k=3), mk.CGGIparam.scaled(n=2, N=32, k=2),
        mk.CCS2party.scaled(n=3, N=256), mk.CCS2party.scaled(n=3, N=2048), mk.CCS2party.scaled(n=3, N=32),                  # UniEnc l = 3, 5, 12
        mk.CCS8party.scaled(n=3, N=512), mk.CCS8party_N2048.scaled(n=2), mk.CCS16party.scaled(n=3, N=128), mk.CCS16party.scaled(n=2, N=4096, k=2),
        mk.KMS32party.scaled(n=2, N=256), mk.KMS4party.scaled(n=3, N=512),                                                  # l_gsw = 6, 5
        mk.Blockparam.scaled(n=150, N=64, k=3, blk_d=50), mk.Blockparam.scaled(n=150, N=128, k=2, blk_d=50),                  # n > N: the LWE key spans ring keys
        mk.Blockparam.scaled(n=12, N=256, blk_d=4), mk.Blockparam_k2.scaled(n=6, N=2048, blk_d=2),
        mk.KMS2partyblock.scaled(n=12, N=256, blk_d=4), mk.KMS2partyblock.scaled(n=6, N=4096, blk_d=2), mk.KMS2partyblock.scaled(n=30, N=32, blk_d=10),
        mk.CGGIparam.scaled(n=1, N=256), mk.KMS2party.scaled(n=1, N=2048), mk.CCS2party.scaled(n=1, N=128),                  # n = 1
    ] + [q.scaled(f=f, logD=logD) for (f, logD) in ((8, 2), (5, 3), (4, 3), (6, 5))                                           # key-switch gadgets
         for q in (mk.CGGIparam.scaled(n=3, N=128), mk.Blockparam.scaled(n=6, N=128, blk_d=2), mk.KMS2party.scaled(n=3, N=64))])


def _id(p):
    return f"{p.name}-n{p.n}-N{p.N}-k{p.k}-W{p.W}-f{p.f}x{p.logD}"


@pytest.mark.parametrize("p", SHAPES, ids=_id)
def test_device_keys_are_the_host_keys_word_for_word(require_gpu, p):
    seed = 8800 + SHAPES.index(p)
    crs = mk.CRS(p, seed) if p.multikey else None
    sd = mk.Scheme(p)
    if p.multikey:
        sd.load_crs(crs)
    made = []
    for i in range(min(p.nparty, 2)):                                   # two parties of one seed
        host = mk.party_keygen(crs, p, party=i, deterministic_seed=seed)
        secr = mk.party_keygen(crs, p, party=i, secrets_only=True, deterministic_seed=seed)
        brk, ksk = sd.keygen_device(i, secr, export=True)
        assert brk.dtype == p.ring_dtype and brk.size == host.brk.size and ksk.size == host.ksk.size
        assert np.array_equal(brk, host.brk), ("bootstrapping key", _id(p), "party", i, "first differing word", int(np.argmax(brk != host.brk)))
        assert np.array_equal(ksk, host.ksk), ("key-switching key", _id(p), "party", i, "first differing word", int(np.argmax(ksk != host.ksk)))
        assert np.array_equal(sd.get_ksk(i).ravel(), host.ksk), "the resident key-switching key is the exported one"
        made.append(brk.copy())
    if len(made) == 2:
        assert not np.array_equal(made[0], made[1]), "two parties of one seed were given one key"
    sd.close()


WIDE = 2.0 ** 55
WIDE_SHAPES = [p.scaled(alpha=WIDE, beta=WIDE) for p in (
    mk.CGGIparam.scaled(n=3, N=256), mk.CGGIparam.scaled(n=2, N=2048),          # RGSW kernel, W = 32: 4- and 16-register accumulator
    mk.KMS2party.scaled(n=3, N=256), mk.KMS2party.scaled(n=2, N=2048),          # RGSW kernel, W = 64
    mk.CCS2party.scaled(n=3, N=256), mk.CCS2party.scaled(n=2, N=2048),          # UniEnc kernel, both of its noise sites
    mk.KMS2partyblock.scaled(n=12, N=256, blk_d=4),                             # the block key-switch path
    mk.CGGIparam.scaled(n=3, N=32), mk.KMS2party.scaled(n=3, N=32))]            # N = 32: idle lanes in fill_noise, on both ring widths


def _same_words(got, want, what, p, party):
    """got == want word for word, or: the set and the party, the key, the first differing word with both words in hex, and how many differ
    (about a fifth of the noise-carrying words: contraction; a handful: an edge of the deviate or of the rounding)"""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.dtype == want.dtype and got.size == want.size, (what, _id(p), "party", party, got.dtype, got.size, want.dtype, want.size)
    bad = np.nonzero(got != want)[0]
    if len(bad):
        i = int(bad[0])
        pytest.fail(f"{what} of {_id(p)}, party {party}: {len(bad)} of {got.size} words differ, the first at word {i}: "
                    f"device {int(got[i]):#x}, host {int(want[i]):#x}")


@pytest.mark.parametrize("p", WIDE_SHAPES, ids=_id)
def test_device_keys_are_the_host_keys_at_full_mantissa_noise(require_gpu, p):
    """the comparison of test_device_keys_are_the_host_keys_word_for_word with alpha = beta = 2^55 (the generators take both deviations
    as free doubles; such keys are useless as keys and exact as a probe).  A deviate has 53 significant bits, so sigma g has its last
    bit at 2^3 or below and a one-ulp change of g changes the word -- the 64-bit one and its low 32 bits, which is all a 32-bit ring and
    the key-switching key keep.  The cast stays defined: 2^55 leaves a factor of 256 under 2^63 and the largest |g| the sampler returns is 8.5717
    (u1 = 2^-53), so (int64_t) rint(sigma g) is in range on both sides."""
    seed = 9900 + WIDE_SHAPES.index(p)
    crs = mk.CRS(p, seed) if p.multikey else None
    sd = mk.Scheme(p)
    if p.multikey:
        sd.load_crs(crs)
    made = []
    for i in range(min(p.nparty, 2)):                                   # two parties of one seed
        host = mk.party_keygen(crs, p, party=i, deterministic_seed=seed)
        secr = mk.party_keygen(crs, p, party=i, secrets_only=True, deterministic_seed=seed)
        brk, ksk = sd.keygen_device(i, secr, export=True)
        assert brk.dtype == p.ring_dtype
        _same_words(brk, host.brk, "bootstrapping key", p, i)
        _same_words(ksk, host.ksk, "key-switching key", p, i)
        _same_words(sd.get_ksk(i), host.ksk, "resident key-switching key", p, i)
        made.append(brk.copy())
    if len(made) == 2:
        assert not np.array_equal(made[0], made[1]), "two parties of one seed were given one key"
    sd.close()


@pytest.mark.parametrize("W", (32, 64))
def test_ring_dimension_16_is_refused_before_any_kernel_runs(require_gpu, W):
    """the host generator makes keys at N = 16 (tests/test_keys_cpu.py judges them); the engine instantiates N = 32 .. 4096 only, so a
    context -- and with it keygen.hip -- cannot exist at N = 16: creating one raises, nothing is launched"""
    with pytest.raises(mk.MktError) as ei:
        mk.Scheme(_RING[W].scaled(n=3, N=16))
    assert "N must be 32..4096" in str(ei.value)


class _DeviceKeys:
    """a party's secrets and small keys, with the two large keys as the device made them"""

    def __init__(self, secrets, brk, ksk):
        self._s, self.brk, self.ksk = secrets, brk, ksk

    def __getattr__(self, name):
        return getattr(self._s, name)


@pytest.mark.parametrize("p", [mk.CGGIparam.scaled(n=16), mk.Blockparam.scaled(n=18, blk_d=6), mk.CCS2party.scaled(n=20), mk.KMS2party.scaled(n=16),
                               mk.KMS2partyblock.scaled(n=18, blk_d=6)], ids=_id)
def test_exported_device_keys_follow_their_laws(require_gpu, p):
    """the judgement of tests/test_keys_cpu.py (exact opening, max|e| <= 6 sigma + 1, noise / mask / independence statistics per
    component) on keys keygen.hip made, one set per scheme"""
    import test_keys_cpu as T
    seed = 8700 + p.scheme
    crs = mk.CRS(p, seed) if p.multikey else None
    sd = mk.Scheme(p)
    if p.multikey:
        sd.load_crs(crs)
    full = []
    for i in range(min(p.nparty, 2)):
        secr = mk.party_keygen(crs, p, party=i, secrets_only=True, deterministic_seed=seed)
        brk, ksk = sd.keygen_device(i, secr, export=True)
        full.append(_DeviceKeys(secr, brk.copy(), ksk.copy()))
    sd.close()
    T.judge_keys(p, crs, full, [], enc_seed=700_000, encryptions=2000)
