"""Distributed decryption (include/mktfhe.h "distributed decryption"): every party opens its own block of the mask and nobody holds two
secret keys.  lwe_decrypt takes all k keys in one process, as the reference's test harness does (scheme.jl:388-407); here

    share_i = partial_decrypt(ctxt, key_i, params, i, sigma_smudge)        party i, alone, on its own machine (or its own GPU)
    bits    = merge_decrypt(ctxt, [share_0, ..., share_{k-1}], params)     anyone: needs the ciphertexts and the k shares, no key

share_i[j] = <a_i[j], s_i> + e_i[j] on the 32-bit torus, e_i[j] fresh Gaussian smudging noise of deviation sigma_smudge (in torus words,
the unit of params.alpha) so that the share does not give s_i away; merge adds the shares to b and decides the bit as lwe_decrypt does.
sigma_smudge is the deployment's choice: the library certifies no value as simulation-secure, and a pinned seed must never
be reused for different ciphertexts.  This module holds no arithmetic: all of it is the C ABI's.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .params import Params
from .scheme import PartyKeys, _Buf, _empty, _is_torch, _np_ptr, _row0, _rows, _seed_arg


def _batch_shape(shape, params):
    if not shape or shape[-1] != params.lwe_len:
        raise ValueError(f"ciphertexts of shape {shape}, expected (..., {params.lwe_len})")
    return shape[:-1] if len(shape) > 1 else (1,)


def _host_words(x):
    """-> contiguous numpy uint32 (a GPU tensor is copied to the host: merging is host work)"""
    if _is_torch(x):
        x = x.detach().cpu().numpy()
        if x.dtype.itemsize != 4:
            raise ValueError(f"tensor of dtype {x.dtype}, expected 32-bit words")
        return np.ascontiguousarray(x).view(np.uint32)
    return np.ascontiguousarray(x, dtype=np.uint32)


def partial_decrypt(ctxt, key: PartyKeys, params: Params, party, sigma_smudge, scheme=None, deterministic_seed=None, row0=0):
    """party `party`'s decryption shares of a batch (..., k*n+1) -> uint32 (...,): <a_party, s_party> + e per row, reading that party's
    block only.  sigma_smudge: deviation of the smudging noise e in torus words, 0 <= sigma_smudge <= 2^31 (MktError otherwise).
    scheme None: on the host (mkt_client_partial_decrypt), numpy in and out.  scheme = a Scheme: on its GPU (mkt_partial_decrypt_batch; it
    needs no evaluation keys loaded), the same words; ctxt a numpy array or a GPU tensor, the shares live where ctxt lives.  That hands this
    party's secret key to that GPU: the party's own device, not the evaluator's.
    The noise comes from fresh OS randomness per call; deterministic_seed (tests only) pins it, and row0 is then the index of this call's
    first row in a larger batch opened in pieces under that one seed (row j draws the noise of row row0 + j)."""
    sp, _keep = _seed_arg(deterministic_seed)
    row0 = _row0(row0)
    if scheme is not None:
        shape = _batch_shape(tuple(ctxt.shape) if _is_torch(ctxt) else np.shape(ctxt), params)
        B = int(np.prod(shape))
        out = _empty(ctxt, shape, np.uint32)
        return scheme._call("partial_decrypt_batch", B, int(party), key.h, scheme._ct(ctxt, B), float(sigma_smudge), sp, row0,
                            _Buf(out, np.uint32, B, out=True))[-1]
    c = np.ascontiguousarray(ctxt, dtype=np.uint32)
    shape = _batch_shape(c.shape, params)
    out = np.empty(shape, dtype=np.uint32)
    check(_lib.lib().mkt_client_partial_decrypt(C.byref(params.c()), key.h, int(party), _np_ptr(c), float(sigma_smudge), sp, row0, _np_ptr(out), out.size))
    return out


def _merge(fn, ctxt, shares, params, dtype):
    c = _host_words(ctxt)
    shape = _batch_shape(c.shape, params)
    B = int(np.prod(shape))
    s = np.ascontiguousarray(np.stack([_host_words(v).reshape(-1) for v in shares])) if len(shares) else np.empty((0, B), dtype=np.uint32)
    if s.shape[1:] != (B,):
        raise ValueError(f"shares of {s.shape[1:]} words each, expected {B}: one per ciphertext")
    out = np.empty(shape, dtype=dtype)
    check(fn(C.byref(params.c()), _np_ptr(c), _np_ptr(s), s.shape[0], _np_ptr(out), B))
    return out


def merge_phase(ctxt, shares, params: Params):
    """b + the sum of the k parties' shares (shares[i] = partial_decrypt of party i, in party order) -> uint32 phase per ciphertext:
    message + noise + smudging noise on the 32-bit torus; with sigma_smudge = 0 the words of lwe_phase.  Needs no key; a share count other
    than the scheme's party count raises MktError"""
    return _merge(_lib.lib().mkt_client_merge_phase, ctxt, shares, params, np.uint32)


def merge_decrypt(ctxt, shares, params: Params):
    """the bits lwe_decrypt decides from merge_phase -> bool per ciphertext"""
    return _merge(_lib.lib().mkt_client_merge_decrypt, ctxt, shares, params, np.uint8).astype(bool)
