"""mktfhe_amd -- MI355X-native batched multi-key TFHE gate-bootstrapping engine.

Keeps the operator surface of the Julia reference SNUCP/MKTFHE for the gate-bootstrapping hot
path (bootstrapping!, blindrotate!, keyswitch!, NAND/AND/OR/XOR/XNOR/NOR/NOT!, and three-input gates in one
bootstrap: MAJ3/XOR3/..., full_adder; programmable bootstrap with caller-supplied lookup tables: lut_bootstrap) behind a C ABI
(include/mktfhe.h) implemented with hand-written HIP kernels for gfx950.  No CPU fallback.
"""
from .params import *  # noqa: F401,F403
from .params import Params  # noqa: F401
from .scheme import (  # noqa: F401
    CRS, PartyKeys, Scheme, MultiScheme, party_keygen, setup, setup_multi, OP_NOT_X, OP_NOT_Y, OP_NOT_Z, lwe_encrypt, lwe_ith_encrypt, lwe_decrypt,
    bootstrapping_, blindrotate_, keyswitch, NAND, AND, OR, XOR, XNOR, NOR, NOT_, MUX, MUX_composite, MAJ3, XOR3, full_adder,
    MEM_DEVICE, MEM_HOST, FMT_INT_COEFF, FMT_F64_FFT, ARITH_F64REF, ARITH_EXACT,
)
from .lut import lut_poly, sign_lut, lut_testvector, lut_bootstrap, lut_gather, lwe_encrypt_word, lwe_phase  # noqa: F401
from .lut import keyswitch_at, lut_bootstrap_at, lut_gather_at, lut_threshold_coefs  # noqa: F401
from .lut import lut_pack, lut_many_bootstrap, lut_many_gather, lut_many_testvector, lut_extract  # noqa: F401
from .decrypt import partial_decrypt, merge_phase, merge_decrypt  # noqa: F401
from .seeded import SeededBatch, seeded_encrypt, seeded_expand  # noqa: F401
from .seeded_keys import party_keygen_seeded, seeded_keys_expand, load_seeded, seeded_section_words, keygen_device_seeded  # noqa: F401
from .pack import packing_keygen, load_packing_key, pack, rlwe_phase, rlwe_partial_decrypt, rlwe_merge_phase, rlwe_merge_decrypt  # noqa: F401
from .pack import packing_keygen_seeded, packing_key_expand, load_packing_key_seeded, packing_keygen_device  # noqa: F401
from ._lib import MktError, LIB_PATH, build_id  # noqa: F401
from . import keyblob  # noqa: F401,E402
from . import circuit  # noqa: F401,E402
