"""The reference's shipped parameter sets, mirrored as data (src/tfhe/params.jl:1-125; field
meaning src/tfhe/scheme.jl:6-101).  alpha / beta are absolute noise standard deviations."""
from dataclasses import dataclass, replace

from ._lib import MktParams

CGGI, LMSS, CCS, KMS, KMS_BLOCK = range(5)
NAND_OP, AND_OP, OR_OP, XOR_OP, XNOR_OP, NOR_OP = range(6)
MAJ3_OP, MIN3_OP, XOR3_OP, XNOR3_OP, NAE3_OP, AE3_OP = range(6)     # three-input gates, one bootstrap each (mktfhe.h MKT_MAJ3 .. MKT_AE3)


@dataclass(frozen=True)
class Params:
    name: str
    scheme: int
    n: int
    N: int
    k: int
    W: int
    alpha: float
    beta: float
    l_gsw: int = 0
    logB_gsw: int = 0
    l_lev: int = 0
    logB_lev: int = 0
    l_uni: int = 0
    logB_uni: int = 0
    f: int = 8
    logD: int = 2
    blk_len: int = 0
    blk_d: int = 0

    @property
    def multikey(self):
        return self.scheme in (CCS, KMS, KMS_BLOCK)

    @property
    def nparty(self):
        return self.k if self.multikey else 1

    @property
    def lwe_len(self):
        return self.nparty * self.n + 1

    @property
    def ring_dtype(self):
        import numpy as np
        return np.uint64 if self.W == 64 else np.uint32

    # -- sizes of one party's two large keys (include/mktfhe.h layouts), stated here once: everything that allocates, checks or ships them reads these
    @property
    def _kr(self):
        """RLWE length of the RGSW rotation: 1 for the KMS schemes, else k"""
        return 1 if self.scheme in (KMS, KMS_BLOCK) else self.k

    @property
    def brk_words(self):
        """ring words of the bootstrapping key"""
        return self.n * (3 * self.l_uni if self.scheme == CCS else (self._kr + 1) * self.l_gsw * (self._kr + 1)) * self.N

    @property
    def brk_seeded_words(self):
        """ring words of the compact bootstrapping-key section (seeded key form): the bodies, and for CCS the d rows whole"""
        return self.n * (2 * self.l_uni if self.scheme == CCS else (self._kr + 1) * self.l_gsw) * self.N

    @property
    def ksk_rows(self):
        """rows of the key-switching key, n + 1 words each; the compact section holds one body word per row"""
        D = 1 << self.logD
        return (1 if self.multikey else self.k) * self.N * (D // 2 if self.scheme in (LMSS, KMS_BLOCK) else D - 1) * self.f

    def c(self):
        return MktParams(self.scheme, self.n, self.N, self.k, self.W, self.l_gsw, self.logB_gsw, self.l_lev,
                         self.logB_lev, self.l_uni, self.logB_uni, self.f, self.logD, self.blk_len, self.blk_d)

    def scaled(self, **kw):
        """a reduced copy for fast tests (e.g. n=16, N=256)"""
        return replace(self, **kw)


# params.jl:1-6, :8-13
CGGIparam = Params("CGGIparam", CGGI, 630, 1024, 1, 32, 2.0**17, 2.0**7, l_gsw=3, logB_gsw=9)
Blockparam = Params("Blockparam", LMSS, 229 * 3, 1024, 1, 32, 2.0**17, 2.0**7, l_gsw=3, logB_gsw=9, blk_len=3, blk_d=229)


def _ccs(k, l, logB):   # params.jl:15-45
    return Params(f"CCS{k}party", CCS, 560, 1024, k, 32, 2.0**17, 2.0**4, l_uni=l, logB_uni=logB)


CCS2party, CCS4party, CCS8party, CCS16party = _ccs(2, 3, 8), _ccs(4, 4, 8), _ccs(8, 5, 6), _ccs(16, 12, 2)


def _kms(k, g, lv, u, block=False):   # params.jl:47-125
    kw = dict(l_gsw=g[0], logB_gsw=g[1], l_lev=lv[0], logB_lev=lv[1], l_uni=u[0], logB_uni=u[1])
    if block:
        return Params(f"KMS{k}partyblock", KMS_BLOCK, 203 * 3, 2048, k, 64, 2.0**17, 85.4084, blk_len=3, blk_d=203, **kw)
    return Params(f"KMS{k}party", KMS, 560, 2048, k, 64, 2.0**17, 85.4084, **kw)


_KMS_G = {2: ((3, 12), (2, 7), (3, 10)), 4: ((5, 8), (2, 8), (7, 6)), 8: ((4, 9), (3, 6), (8, 4)),
          16: ((5, 8), (3, 6), (9, 4)), 32: ((6, 7), (3, 7), (16, 2))}
KMS2party, KMS4party, KMS8party, KMS16party, KMS32party = (_kms(k, *_KMS_G[k]) for k in (2, 4, 8, 16, 32))
KMS2partyblock, KMS4partyblock, KMS8partyblock, KMS16partyblock, KMS32partyblock = (
    _kms(k, *_KMS_G[k], block=True) for k in (2, 4, 8, 16, 32))

# BASELINE.json config 2: "KMS multi-key k=2, N=1024, l=2" -- NOT a shipped constant of the reference
# (SURVEY.md 0.5); a legal KMSparams value used as the synthetic performance shape.  Decryption
# correctness at this shape is not vouched for by the reference; the gadget bases are the ones with the
# smallest output noise on cross-party gates at l_gsw = 2, l_lev = 2 (tools/param_noise_sweep2.py: phase
# error std 0.025 against the 0.125 margin; the reference's own KMS2party has l_gsw = 3 and N = 2048).
KMS2party_N1024_l2 = Params("KMS2party_N1024_l2", KMS, 560, 1024, 2, 64, 2.0**17, 85.4084,
                            l_gsw=2, logB_gsw=16, l_lev=2, logB_lev=6, l_uni=3, logB_uni=10)

# BASELINE.json configs[0]: "CGGI single-key NAND bootstrap, N=1024, n=630, l=2" -- the reference's CGGIparam has l = 3
# (params.jl:1-6); this is the l = 2 gadget with the base of least output noise (tools/noise_probe.py on the GPU:
# phase error std 0.006 at logB = 8 against the 0.125 margin; 0.010 at 7 and 9, 0.020 at 10 -- CGGIparam itself: 0.012).
CGGI_N1024_l2 = Params("CGGI_N1024_l2", CGGI, 630, 1024, 1, 32, 2.0**17, 2.0**7, l_gsw=2, logB_gsw=8)
# BASELINE.json configs[3]: "CCS multi-key k=8, N=2048" -- the reference's CCS8party has N = 1024 (params.jl:31-37) and
# is noisy already (phase error std 0.040: 1-3 % wrong decryptions on 8-party gates); at N = 2048 the same beta = 2^4
# gives 0.075 (25 % wrong).  The doubled ring dimension carries its security with less noise: beta = 1 (std 0.011, no
# failures in 2048 gates, tools/noise_probe.py); gadget as CCS8party.
CCS8party_N2048 = Params("CCS8party_N2048", CCS, 560, 2048, 8, 32, 2.0**17, 1.0, l_uni=5, logB_uni=6)
# BASELINE.json configs[4]: "LMSS block-binary blind-rotation, N=1024, k=2": Blockparam (params.jl:8-13) with RLWE
# length 2 -- a legal TFHEparams_block value (scheme.jl:22-36), not a shipped constant; noise as Blockparam, gadget
# base 2^7 instead of 2^9 (twice the key dimension: phase error std 0.005 instead of 0.015, tools/noise_probe.py).
Blockparam_k2 = Params("Blockparam_k2", LMSS, 229 * 3, 1024, 2, 32, 2.0**17, 2.0**7, l_gsw=3, logB_gsw=7, blk_len=3, blk_d=229)
