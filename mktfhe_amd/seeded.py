"""Seeded ciphertexts (include/mktfhe.h "seeded ciphertexts"): a fresh ciphertext of party i is zeros, n uniform mask words and one body
word, so a party ships a PUBLIC mask seed and the bodies, and the evaluator regenerates the rows on its GPU:

    batch = seeded_encrypt(bits, key_i, params, i)                  party i, on the host (or scheme=: on its own GPU)
    rows  = seeded_expand(batch, params, scheme=evaluator)          anyone: needs no key; ordinary ciphertexts (B, k*n+1)

A (mask_seed, party, row index) must never serve two encryptions: the difference of the two bodies is then the difference of the
messages plus two noise words.  seeded_encrypt draws a fresh mask seed per call unless one is given; a caller that continues a batch
under one seed passes row0.  A MultiScheme caller expands per shard with row0 + the shard's offset.  This module holds no arithmetic:
all of it is the C ABI's.
"""
import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import check
from .params import Params
from .scheme import PartyKeys, _Buf, _empty, _is_torch, _np_ptr, _row0, _seed32, _seed_arg


class SeededBatch(NamedTuple):
    """what travels: the party index, the public 32-byte mask seed, the index of the first row, and one body word per ciphertext
    (uint32 numpy array or GPU tensor, any shape)"""
    party: int
    mask_seed: bytes
    row0: int
    body: object


def seeded_encrypt(msgs, key: PartyKeys, params: Params, party, *, words=False, scheme=None, mask_seed=None, deterministic_seed=None, row0=0):
    """party `party`'s seeded encryptions of msgs (any shape) -> SeededBatch with one body word per message.  words=False: msgs are bits,
    encoded as +-2^29 like lwe_ith_encrypt; words=True: msgs are words of the 32-bit torus, used as they are (a GPU tensor is taken as
    words only).  mask_seed None draws a fresh public seed (mkt_client_random_seed); the noise comes from fresh OS randomness per call,
    deterministic_seed (tests only) pins it.  scheme None: on the host (mkt_client_seeded_encrypt), numpy bodies.  scheme = a Scheme: on
    its GPU (mkt_seeded_encrypt_batch; no evaluation keys needed), the same words, the bodies living where msgs live.  That hands this
    party's secret key to that GPU: the party's own device, not the evaluator's."""
    if mask_seed is None:
        buf = (C.c_uint8 * 32)()
        check(_lib.lib().mkt_client_random_seed(buf))
        mask_seed = bytes(buf)
    mp, _mkeep = _seed32(mask_seed)
    sp, _keep = _seed_arg(deterministic_seed)
    row0 = _row0(row0)
    if _is_torch(msgs):
        if not words:
            raise ValueError("a GPU tensor of messages holds torus words: pass words=True")
        mu = msgs
    else:
        m = np.asarray(msgs)
        mu = np.ascontiguousarray(m, dtype=np.uint32) if words else np.where(m.astype(bool), np.uint32(1 << 29), np.uint32(7 << 29)).astype(np.uint32)
    shape = tuple(mu.shape)
    B = int(np.prod(shape))
    if scheme is not None:
        out = _empty(mu, shape, np.uint32)
        body = scheme._call("seeded_encrypt_batch", B, int(party), key.h, _Buf(mu, np.uint32, B), float(params.alpha), mp, sp, row0,
                            _Buf(out, np.uint32, B, out=True))[-1]
    else:
        body = np.empty(shape, dtype=np.uint32)
        check(_lib.lib().mkt_client_seeded_encrypt(C.byref(params.c()), key.h, int(party), _np_ptr(mu), float(params.alpha), mp, sp, row0, _np_ptr(body), B))
    return SeededBatch(int(party), bytes(mask_seed), row0, body)


def seeded_expand(batch: SeededBatch, params: Params, scheme=None, out=None):
    """the ciphertexts of a seeded batch, body shape (...) -> uint32 (..., k*n+1): zeros, the regenerated mask in the party's block, the
    body last.  Needs no key.  scheme None: on the host (mkt_client_seeded_expand), numpy.  scheme = a Scheme: on its GPU
    (mkt_seeded_expand_batch; no evaluation keys needed), the same words; the rows live where batch.body lives (out: write them there)."""
    mp, _mkeep = _seed32(batch.mask_seed)
    row0 = _row0(batch.row0)
    body = batch.body
    shape = tuple(body.shape)
    B = int(np.prod(shape))
    if scheme is not None:
        if out is None:
            out = _empty(body, shape + (params.lwe_len,), np.uint32)
        return scheme._call("seeded_expand_batch", B, int(batch.party), mp, row0, _Buf(body, np.uint32, B), scheme._ct(out, B, out=True))[-1]
    b = np.ascontiguousarray(body, dtype=np.uint32)
    if out is None:
        out = np.empty(shape + (params.lwe_len,), dtype=np.uint32)
    if not (isinstance(out, np.ndarray) and out.dtype == np.uint32 and out.flags.c_contiguous and out.size == B * params.lwe_len):
        raise ValueError(f"out must be a contiguous uint32 array of {B} rows of {params.lwe_len}")
    check(_lib.lib().mkt_client_seeded_expand(C.byref(params.c()), int(batch.party), mp, row0, _np_ptr(b), _np_ptr(out), B))
    return out
