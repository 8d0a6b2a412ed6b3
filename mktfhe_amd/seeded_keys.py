"""Seeded evaluation keys (include/mktfhe.h "seeded evaluation keys"): almost all of a party's two large keys is public randomness, so a
party ships a PUBLIC mask seed and the bodies, and the evaluator's GPU regenerates the masks where the resident tables live:

    keys = party_keygen_seeded(crs, params, party=i)                party i, on the host: secrets, small keys, compact sections
    blob = keyblob.dump_party(keys)                                 format version 2: mask_seed, brk_seeded, ksk_seeded (+ small keys)
    load_seeded(evaluator, i, keys)  /  keyblob.load_into(...)      the evaluator: masks expanded on its GPU, never on a host
    brk, ksk = seeded_keys_expand(params, i, keys.mask_seed, keys.brk_seeded, keys.ksk_seeded)      anyone: the ordinary keys; needs no key
    keys = keygen_device_seeded(own_scheme, i, party_keygen(crs, params, party=i, secrets_only=True))      party i, the compact sections made on
                                                                                                            its OWN GPU: the same words

A (mask seed, party) pair serves ONE key generation: two generations under it share their masks.  party_keygen_seeded draws a fresh mask
seed unless one is given.  The mask seed is not a secret.  This module holds no arithmetic: all of it is the C ABI's.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .params import CCS, Params
from .scheme import MEM_DEVICE, PartyKeys, _arg, _Buf, _empty, _np_ptr, _seed32, _seeded_sections, seeded_section_words


def party_keygen_seeded(a, params: Params, party=0, mask_seed=None, deterministic_seed=None):
    """party_keygen in the seeded key form -> PartyKeys with mask_seed, brk_seeded, ksk_seeded (brk and ksk are None); secrets, public key
    and relinearisation key are those of party_keygen with the same deterministic_seed.  mask_seed None draws a fresh public seed"""
    return PartyKeys(params, party=party, crs=a, deterministic_seed=deterministic_seed, seeded=True, mask_seed=mask_seed)


def full_key_words(params: Params):
    """(ring words of the bootstrapping key, (rows, n + 1) of the key-switching key) of one party: the layouts of load_party"""
    return params.brk_words, (params.ksk_rows, params.n + 1)


def seeded_keys_expand(params: Params, party, mask_seed, brk_seeded=None, ksk_seeded=None, scheme=None):
    """-> (brk, ksk): the ordinary keys of a seeded party in the layouts of load_party (None for a section that was not given).  Needs no key.
    scheme None: on the host (mkt_client_seeded_keys_expand, the definition), numpy.  scheme = a Scheme: on its GPU (mkt_seeded_keys_expand;
    no evaluation keys needed, no resident table changed), the same words, living where the compact sections live (numpy arrays or GPU tensors)"""
    mp, _keep = _seed32(mask_seed)
    wb, (rows, n1) = full_key_words(params)
    if scheme is None:
        b, k = _seeded_sections(params, brk_seeded, ksk_seeded)
        brk = None if b is None else np.empty(wb, dtype=params.ring_dtype)
        ksk = None if k is None else np.empty((rows, n1), dtype=np.uint32)
        ptr = lambda v: None if v is None else _np_ptr(v)      # noqa: E731
        check(_lib.lib().mkt_client_seeded_keys_expand(C.byref(params.c()), int(party), mp, ptr(b), ptr(k), ptr(brk), ptr(ksk)))
        return brk, ksk
    sb, sk = seeded_section_words(params)
    like = brk_seeded if brk_seeded is not None else ksk_seeded
    if like is None:
        return None, None
    brk = None if brk_seeded is None else _empty(like, (wb,), params.ring_dtype, "int64" if params.W == 64 else "int32")
    ksk = None if ksk_seeded is None else _empty(like, (rows, n1), np.uint32, "int32")
    buf = lambda v, dt, n, out=False: None if v is None else _Buf(v, dt, n, out=out)      # noqa: E731
    # (_call appends a batch count, which this entry point does not take: the call goes to the library directly, sizes checked here)
    args = [buf(brk_seeded, params.ring_dtype, sb), buf(ksk_seeded, np.uint32, sk), buf(brk, params.ring_dtype, wb, True), buf(ksk, np.uint32, rows * n1, True)]
    return _expand_on(scheme, int(party), mp, args, brk, ksk)


def _expand_on(scheme, party, mp, args, brk, ksk):
    ptrs, mems, kept = [], set(), []
    for a in args:
        if a is None:
            ptrs.append(None)
            continue
        ptr, mem, k = _arg(a.x, a.dtype, writable=a.out)
        if int(np.prod(tuple(k.shape))) != a.n:
            raise ValueError(f"mkt_seeded_keys_expand: an argument of {int(np.prod(tuple(k.shape)))} words, expected {a.n}")
        ptrs.append(ptr)
        mems.add(mem)
        kept.append(k)
    if len(mems) > 1:
        raise ValueError("mkt_seeded_keys_expand: all arguments must be host arrays or all be GPU tensors")
    mem = mems.pop()
    if mem == MEM_DEVICE:
        scheme._follow_torch(kept)
    scheme._ck(_lib.lib().mkt_seeded_keys_expand(scheme.h, party, mp, *ptrs, mem))      # (returns once the words are written)
    return brk, ksk


def load_seeded(scheme, party, keys: PartyKeys = None, *, mask_seed=None, brk_seeded=None, ksk_seeded=None):
    """upload a seeded party into a Scheme or MultiScheme: the large keys through mkt_load_seeded_keys (masks regenerated on the GPU), the
    small keys of `keys` as load_party uploads them.  Same resident state as load_party of the expanded keys"""
    if keys is not None:
        if not getattr(keys, "seeded", False):
            raise ValueError("load_seeded takes a seeded party (party_keygen_seeded)")
        return scheme.load_party(party, keys)
    return scheme.load_party(party, mask_seed=mask_seed, brk_seeded=brk_seeded, ksk_seeded=ksk_seeded)


class SeededDeviceKeys:
    """a party in the seeded key form whose compact sections were generated on its own GPU (keygen_device_seeded): mask_seed, brk_seeded,
    ksk_seeded as party_keygen_seeded gives them, brk = ksk = None; params, party, the small keys and the secret accessors are those of the
    party object the sections were made from"""
    seeded, secrets_only, brk, ksk = True, False, None, None

    def __init__(self, keys, mask_seed, brk_seeded, ksk_seeded):
        self._keys, self.mask_seed, self.brk_seeded, self.ksk_seeded = keys, mask_seed, brk_seeded, ksk_seeded

    def __getattr__(self, name):        # params, party, rlk_d, rlk_f, pubkey, lwekey, ringkey, h, _crs
        return getattr(self._keys, name)


def keygen_device_seeded(scheme, party, keys: PartyKeys, mask_seed=None, install=False):
    """the seeded key form generated on the party's OWN GPU (mkt_keygen_device_seeded) -> a seeded party view (SeededDeviceKeys): the compact
    sections are those party_keygen_seeded makes on the host for the seed `keys` was made from, word for word, and the large keys are never
    expanded.  `keys`: any PartyKeys of these parameters and this party (secrets_only=True is enough).  mask_seed None draws a fresh public
    seed.  This hands the party's SECRETS to scheme's GPU: the party's own step.  install=True: the sections also become the resident keys of
    `party` on `scheme`, as load_seeded of the result would make them, and the small keys of `keys` are uploaded as Scheme.keygen_device does"""
    if mask_seed is None:
        buf = (C.c_uint8 * 32)()
        check(_lib.lib().mkt_client_random_seed(buf))
        mask_seed = bytes(buf)
    mp, _keep = _seed32(mask_seed)
    params = scheme.params
    sb, sk = seeded_section_words(params)
    brk = np.empty(sb, dtype=params.ring_dtype)
    ksk = np.empty(sk, dtype=np.uint32)
    crs_p = _np_ptr(keys._crs) if (params.scheme == CCS and keys._crs is not None) else None
    scheme._ck(_lib.lib().mkt_keygen_device_seeded(scheme.h, int(party), keys.h, crs_p, mp, _np_ptr(brk), _np_ptr(ksk), 1 if install else 0))
    if install:
        scheme.load_party(party, rlk_d=keys.rlk_d, rlk_f=keys.rlk_f, pubkey=keys.pubkey)
    return SeededDeviceKeys(keys, bytes(mask_seed), brk, ksk)
