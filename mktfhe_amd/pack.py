"""Packed outputs (include/mktfhe_pack.h): N result ciphertexts folded into one RLWE ciphertext on the GPU, opened by one ring share per party.

    pk_i   = packing_keygen(keys_i, params, l, logB)                  party i, once: an evaluation key, shipped with the others
    load_packing_key(scheme, i, pk_i, l, logB)                        evaluator, for every party
    rlwe   = pack(scheme, results)                                    evaluator: (ceil(B / N), k + 1, N) ring words for B rows of k*n+1
    sh_i   = rlwe_partial_decrypt(rlwe, keys_i, params, i, sigma)     party i, alone: (packs, N) ring words (scheme=: on the party's own GPU)
    bits   = rlwe_merge_decrypt(rlwe[g], [sh_0[g], ...], params)      anyone: coefficient j = result row g N + j

Coefficient j of a packed ciphertext carries the phase of row j, so it is also an ordinary accumulator of keyswitch_at, which reads row j
back out.  This module holds no arithmetic: all of it is the C ABI's.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .params import Params
from .scheme import MEM_DEVICE, PartyKeys, _arg, _Buf, _count, _empty, _is_torch, _np_ptr, _row0, _rows, _seed32, _seed_arg


def _kr(params):
    """ring components one party's packing key covers: 1 for the multi-key schemes, the RLWE length otherwise"""
    return 1 if params.multikey else params.k


def _gadget(l, logB):
    l, logB = int(l), int(logB)
    if not (1 <= logB <= 16 and l >= 1 and l * logB <= 32):
        raise ValueError(f"packing gadget (l = {l}, logB = {logB}): 1 <= logB <= 16, 1 <= l, l * logB <= 32")
    return l, logB


def _ring_words(x, params):
    """-> contiguous host array of ring words (a GPU tensor is copied to the host: opening is host work)"""
    if _is_torch(x):
        x = x.detach().cpu().numpy()
        if x.dtype.itemsize != params.W // 8:
            raise ValueError(f"tensor of dtype {x.dtype}, expected {params.W}-bit ring words")
        return np.ascontiguousarray(x).view(params.ring_dtype)
    return np.ascontiguousarray(x, dtype=params.ring_dtype)


def _cts(rlwe, params):
    """packed ciphertexts (..., k + 1, N) on the host -> (array, leading shape)"""
    c = _ring_words(rlwe, params)
    if c.shape[-2:] != (params.k + 1, params.N):
        raise ValueError(f"packed ciphertexts of shape {c.shape}, expected (..., {params.k + 1}, {params.N})")
    return c, c.shape[:-2]


def packing_keygen(keys: PartyKeys, params: Params, l=4, logB=4, deterministic_seed=None):
    """mkt_client_packing_keygen: the packing key of the party `keys` belongs to -> (n, l, 1 + kr, N) ring words; row (q, t) is an RLWE sample
    of s[q] 2^(W - (t + 1) logB) under the ring key(s) the key-switching key switches from.  Fresh OS randomness unless deterministic_seed
    (tests only) pins it"""
    l, logB = _gadget(l, logB)
    sp, _keep = _seed_arg(deterministic_seed)
    out = np.empty((params.n, l, 1 + _kr(params), params.N), dtype=params.ring_dtype)
    check(_lib.lib().mkt_client_packing_keygen(C.byref(params.c()), keys.h, int(keys.party), l, logB, sp, _np_ptr(out)))
    return out


def load_packing_key(scheme, party, pk, l, logB):
    """mkt_load_packing_key: party `party`'s packing key (host array, coefficient form) becomes resident on the scheme's GPU.  Every party
    loads with the same gadget; refused once the scheme has been forked, as every key load"""
    l, logB = _gadget(l, logB)
    p = scheme.params
    pk = np.ascontiguousarray(pk, dtype=p.ring_dtype)
    if pk.size != p.n * l * (1 + _kr(p)) * p.N:
        raise ValueError(f"packing key of {pk.size} ring words, expected {(p.n, l, 1 + _kr(p), p.N)}")
    scheme._ck(_lib.lib().mkt_load_packing_key(scheme.h, int(party), _np_ptr(pk), l, logB))


def _fresh_seed():
    buf = (C.c_uint8 * 32)()
    check(_lib.lib().mkt_client_random_seed(buf))
    return bytes(buf)


def _bodies(params, pk_seeded, l):
    """the compact section -> contiguous host array of n l N ring words"""
    b = np.ascontiguousarray(pk_seeded, dtype=params.ring_dtype)
    if b.size != params.n * l * params.N:
        raise ValueError(f"seeded packing key of {b.size} ring words, expected {(params.n, l, params.N)}")
    return b


def packing_keygen_seeded(keys: PartyKeys, params: Params, l=4, logB=4, mask_seed=None, deterministic_seed=None):
    """mkt_client_packing_keygen_seeded: the packing key of the party `keys` belongs to in the seeded form -> (mask_seed, pk_seeded): the
    PUBLIC 32-byte mask seed (None draws a fresh one) and the bodies (n, l, N) ring words; the party ships both, the evaluator regenerates
    the masks (load_packing_key_seeded).  A (mask seed, party) pair serves ONE generation per gadget.  Fresh noise unless deterministic_seed
    (tests only) pins it"""
    l, logB = _gadget(l, logB)
    mask_seed = _fresh_seed() if mask_seed is None else bytes(mask_seed)
    mp, _keepm = _seed32(mask_seed)
    sp, _keep = _seed_arg(deterministic_seed)
    out = np.empty((params.n, l, params.N), dtype=params.ring_dtype)
    check(_lib.lib().mkt_client_packing_keygen_seeded(C.byref(params.c()), keys.h, int(keys.party), l, logB, sp, mp, _np_ptr(out)))
    return mask_seed, out


def packing_key_expand(params: Params, party, l, logB, mask_seed, pk_seeded, scheme=None):
    """-> the ordinary packing key (n, l, 1 + kr, N) of a seeded one.  Needs no key.  scheme None: on the host (mkt_client_packing_key_expand,
    the definition), numpy.  scheme = a Scheme: on its GPU (mkt_packing_key_expand; no key needed, no resident table changed), the same words,
    living where pk_seeded lives (numpy array or GPU tensor)"""
    l, logB = _gadget(l, logB)
    mp, _keep = _seed32(mask_seed)
    shape = (params.n, l, 1 + _kr(params), params.N)
    if scheme is None:
        b = _bodies(params, pk_seeded, l)
        out = np.empty(shape, dtype=params.ring_dtype)
        check(_lib.lib().mkt_client_packing_key_expand(C.byref(params.c()), int(party), l, logB, mp, _np_ptr(b), _np_ptr(out)))
        return out
    if int(np.prod(tuple(np.shape(pk_seeded)))) != params.n * l * params.N:
        raise ValueError(f"seeded packing key of shape {tuple(np.shape(pk_seeded))}, expected {(params.n, l, params.N)}")
    out = _empty(pk_seeded, shape, params.ring_dtype, "int64" if params.W == 64 else "int32")
    src, dst = _arg(pk_seeded, params.ring_dtype), _arg(out, params.ring_dtype, writable=True)
    if src[1] == MEM_DEVICE:
        scheme._follow_torch([src[2], dst[2]])
    scheme._ck(_lib.lib().mkt_packing_key_expand(scheme.h, int(party), l, logB, mp, src[0], dst[0], src[1]))      # (returns once the words are written)
    return out


def load_packing_key_seeded(scheme, party, mask_seed, pk_seeded, l, logB):
    """mkt_load_packing_key_seeded: the resident state of load_packing_key(packing_key_expand(...)), the masks regenerated on the scheme's GPU;
    the expanded key never exists on the host"""
    l, logB = _gadget(l, logB)
    mp, _keep = _seed32(mask_seed)
    b = _bodies(scheme.params, pk_seeded, l)
    scheme._ck(_lib.lib().mkt_load_packing_key_seeded(scheme.h, int(party), mp, _np_ptr(b), l, logB))


def packing_keygen_device(scheme, party, keys: PartyKeys, l=4, logB=4, mask_seed=None, deterministic_seed=None, install=False):
    """mkt_packing_keygen_device: packing_keygen_seeded on the party's OWN GPU -> (mask_seed, pk_seeded), word for word what the host call
    makes for the same deterministic_seed.  This hands the party's SECRETS to scheme's GPU: the party's own step.  install=True: the key
    also becomes resident on `scheme`, as load_packing_key_seeded of the result would make it"""
    l, logB = _gadget(l, logB)
    mask_seed = _fresh_seed() if mask_seed is None else bytes(mask_seed)
    mp, _keepm = _seed32(mask_seed)
    sp, _keep = _seed_arg(deterministic_seed)
    p = scheme.params
    out = np.empty((p.n, l, p.N), dtype=p.ring_dtype)
    scheme._ck(_lib.lib().mkt_packing_keygen_device(scheme.h, int(party), keys.h, l, logB, sp, mp, _np_ptr(out), 1 if install else 0))
    return mask_seed, out


def pack(scheme, ct_or_pool, idx=None, out=None):
    """mkt_pack_batch: rows of ct_or_pool (..., k*n+1) -- all of them in order, or those named by idx (uint32 array / int32 tensor, repeats
    allowed) -- packed N at a time: row g N + j goes to coefficient j of ciphertext g, absent rows are zero.  numpy arrays or GPU tensors;
    -> (ceil(B / N), k + 1, N) ring words living where the rows live (out: such an array, not overlapping them)"""
    p = scheme.params
    shape = tuple(np.shape(ct_or_pool))
    if shape[-1:] != (p.lwe_len,):
        raise ValueError(f"ciphertexts of shape {shape}, expected (..., {p.lwe_len})")
    rows = _rows(shape)
    B = rows if idx is None else _count(idx)
    npacks = -(-B // p.N)
    if out is None:
        out = _empty(ct_or_pool, (npacks, p.k + 1, p.N), p.ring_dtype, "int64" if p.W == 64 else "int32")
    if tuple(np.shape(out)) != (npacks, p.k + 1, p.N):
        raise ValueError(f"out of shape {tuple(np.shape(out))}, expected {(npacks, p.k + 1, p.N)}")
    if B == 0:                  # nothing to pack: the library would write nothing
        return out
    if idx is not None and not _is_torch(idx):
        idx = np.ascontiguousarray(idx)
        if idx.dtype.kind not in "iu" or (idx.size and (idx.min() < 0 or idx.max() >= 2**32)):
            raise ValueError("idx: expected row indices")
        idx = idx.astype(np.uint32)
    args = [_arg(ct_or_pool, np.uint32), _arg(out, p.ring_dtype, writable=True)] + ([] if idx is None else [_arg(idx, np.uint32)])
    mems = {m for _, m, _ in args}
    if len(mems) > 1:
        raise ValueError("mkt_pack_batch: all arguments must be host arrays or all be GPU tensors")
    mem = mems.pop()
    if mem == MEM_DEVICE:
        scheme._follow_torch([k for _, _, k in args])
    scheme._ck(_lib.lib().mkt_pack_batch(scheme.h, args[0][0], rows, None if idx is None else args[2][0], B, args[1][0], mem))
    return args[1][2]


def rlwe_phase(rlwe, keys, params: Params):
    """TEST HARNESS (all keys in one process): the top 32 bits of b + sum a z of packed ciphertexts (..., k + 1, N) -> uint32 (..., N);
    keys: the parties' PartyKeys in party order, or one PartyKeys for CGGI / LMSS"""
    keys = [keys] if isinstance(keys, PartyKeys) else list(keys)
    c, lead = _cts(rlwe, params)
    c = c.reshape((-1,) + c.shape[-2:])
    out = np.empty((c.shape[0], params.N), dtype=np.uint32)
    kp = (C.c_void_p * len(keys))(*[k.h for k in keys])
    for g in range(c.shape[0]):
        check(_lib.lib().mkt_client_rlwe_phase(C.byref(params.c()), kp, len(keys), _np_ptr(c[g]), _np_ptr(out[g])))
    return out.reshape(lead + (params.N,))


def rlwe_partial_decrypt(rlwe, key: PartyKeys, params: Params, party, sigma_smudge, deterministic_seed=None, row0=0, scheme=None):
    """party `party`'s ring shares of packed ciphertexts (..., k + 1, N) -> ring words (..., N): sum_c a_c (*) z_c + e, reading that party's
    polynomial(s) only.  sigma_smudge: deviation of the smudging noise in words of the 32-bit torus, 0 <= sigma_smudge <= 2^31.  The noise is
    fresh per call; deterministic_seed (tests only) pins it, and row0 is then the index of this call's first PACK under that seed.
    scheme None: on the host (mkt_client_rlwe_partial_decrypt), numpy out.  scheme = a Scheme: on its GPU (mkt_rlwe_partial_decrypt_batch of
    include/mktfhe_ring_share.h; it needs no key loaded), the same words; rlwe a numpy array or a GPU tensor, (G, k + 1, N) or one pack
    (k + 1, N), the shares live where rlwe lives.  That hands this party's secret ring key(s) to that GPU: the party's own device, not the
    evaluator's"""
    sp, _keep = _seed_arg(deterministic_seed)
    if scheme is not None:
        shape = tuple(np.shape(rlwe))
        if shape[-2:] != (params.k + 1, params.N) or len(shape) > 3:
            raise ValueError(f"packed ciphertexts of shape {shape}, expected (G, {params.k + 1}, {params.N}) or ({params.k + 1}, {params.N})")
        G = int(np.prod(shape[:-2]))
        out = _empty(rlwe, shape[:-2] + (params.N,), params.ring_dtype, "int64" if params.W == 64 else "int32")
        return scheme._call("rlwe_partial_decrypt_batch", G, int(party), key.h, _Buf(rlwe, params.ring_dtype, G * (params.k + 1), params.N),
                            float(sigma_smudge), sp, _row0(row0), _Buf(out, params.ring_dtype, G, params.N, out=True))[-1]
    c, lead = _cts(rlwe, params)
    G = int(np.prod(lead))
    out = np.empty(lead + (params.N,), dtype=params.ring_dtype)
    check(_lib.lib().mkt_client_rlwe_partial_decrypt(C.byref(params.c()), key.h, int(party), _np_ptr(c), float(sigma_smudge), sp, _row0(row0), _np_ptr(out), G))
    return out


def _merge(fn, rlwe, shares, params, count, dtype):
    c, lead = _cts(rlwe, params)
    if lead not in ((), (1,)):
        raise ValueError("merge opens one packed ciphertext per call")
    s = np.ascontiguousarray(np.stack([_ring_words(v, params).reshape(-1) for v in shares])) if len(shares) else np.empty((0, params.N), dtype=params.ring_dtype)
    if s.shape[1:] != (params.N,):
        raise ValueError(f"shares of {s.shape[1:]} ring words each, expected {params.N}")
    count = params.N if count is None else int(count)
    out = np.empty(max(count, 0), dtype=dtype)
    check(fn(C.byref(params.c()), _np_ptr(c), _np_ptr(s), s.shape[0], count, _np_ptr(out)))
    return out


def rlwe_merge_phase(rlwe, shares, params: Params, count=None):
    """the top 32 bits of b + the k parties' ring shares (in party order) of ONE packed ciphertext -> uint32 (count,), count <= N (None: N);
    with sigma_smudge = 0 the words of rlwe_phase.  Needs no key"""
    return _merge(_lib.lib().mkt_client_rlwe_merge_phase, rlwe, shares, params, count, np.uint32)


def rlwe_merge_decrypt(rlwe, shares, params: Params, count=None):
    """the bits lwe_decrypt decides from rlwe_merge_phase -> bool (count,)"""
    return _merge(_lib.lib().mkt_client_rlwe_merge_decrypt, rlwe, shares, params, count, np.uint8).astype(bool)
