"""Programmable bootstrap (include/mktfhe.h "programmable bootstrap"): bootstrapping! (tfhe/bootstrapping.jl:4-27) with a caller-supplied
lookup table in place of its constant test vector -- any negacyclic function of the input's phase in one bootstrap.

A lookup table is a test-vector polynomial T of N ring words; lut_poly lays one out from the output word wanted on each of P equal windows of
the half torus (the other half is the negation: f(phi + 1/2) = -f(phi)), sign_lut is the reference's own table.  The functions take the
scheme as an argument -- a Scheme, or for lut_bootstrap also a MultiScheme -- and go through its checked call path: every buffer's size is
compared with what the library reads or writes before the library is called.  Arrays are numpy arrays (host) or GPU tensors, all of one kind
per call.  This module holds no arithmetic beyond laying out tables.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .params import Params
from .scheme import PartyKeys, _Buf, _count, _empty, _is_torch, _np_ptr, _rows, _seed_arg


def lut_poly(values, params: Params):
    """the table whose bootstrap returns values[v] for an input phase in window [v/(2P), (v+1)/(2P)) of the torus, P = len(values) a divisor
    of N, and -values[v] half a turn further: T[0] = values[0], T[j] = -values[floor((N - j) P / N)] for j >= 1 (mktfhe.h: the bootstrap
    extracts -T[N - phi] for a mod-switched phase 1 <= phi <= N).  values: ring words (any integers, taken mod 2^W) -> (N,) ring words"""
    N, W = params.N, params.W
    vals = [int(v) & ((1 << W) - 1) for v in np.asarray(values, dtype=object).ravel()]
    P = len(vals)
    if P < 1 or N % P:
        raise ValueError(f"{P} table values: the count must divide N = {N}")
    t = np.empty(N, dtype=object)
    t[0] = vals[0]
    for j in range(1, N):
        t[j] = (-vals[(N - j) * P // N]) & ((1 << W) - 1)
    return t.astype(params.ring_dtype)


def sign_lut(params: Params):
    """the reference's test vector (bootstrapping.jl:11-23): every coefficient -2^(W-3).  lut_bootstrap with it is bootstrapping!"""
    return np.full(params.N, (1 << params.W) - (1 << (params.W - 3)), dtype=params.ring_dtype)


def _tables(luts, params):
    """-> the _Buf of luts ((nluts, N) or (N,) ring words) and nluts.  Host tables must already hold ring words: integers of the ring's word
    size (another size would be converted silently, value by value, into something else than the caller laid out)"""
    rd = np.dtype(params.ring_dtype)
    if not _is_torch(luts):
        luts = np.asarray(luts)
        if luts.dtype.kind not in "iu" or luts.dtype.itemsize != rd.itemsize:
            raise ValueError(f"lookup tables of dtype {luts.dtype}, expected {rd} (ring words)")
        luts = np.ascontiguousarray(luts).view(rd)
    shape = tuple(luts.shape)
    if not shape or shape[-1] != params.N:
        raise ValueError(f"lookup tables of shape {shape}, expected (nluts, {params.N})")
    nluts = _rows(shape)
    return _Buf(luts, rd, nluts, params.N), nluts


def _sel(sel, B):
    return None if sel is None else _Buf(sel, np.uint32, B)


def lut_testvector(scheme, luts, ctxt, sel=None):
    """mkt_lut_testvector_batch: the accumulators (X^btilde(ctxt[j]) * luts[sel[j]], 0 ...) a programmable bootstrap hands to blindrotate!
    -> (..., k + 1, N) ring words living where ctxt lives.  sel: uint32 rows of luts (int32 tensor), None = row 0"""
    p = scheme.params
    shape = tuple(np.shape(ctxt))
    B = _rows(shape)
    tb, nluts = _tables(luts, p)
    acc = _empty(ctxt, shape[:-1] + (p.k + 1, p.N), p.ring_dtype, "int64" if p.W == 64 else "int32")
    return scheme._call("lut_testvector_batch", B, tb, nluts, _sel(sel, B), scheme._ct(ctxt, B), _Buf(acc, p.ring_dtype, B * (p.k + 1) * p.N, out=True))[-1]


def lut_bootstrap(scheme, luts, ctxt, sel=None, out=None):
    """mkt_lut_bootstrap_batch (a Scheme) / mkt_multi_lut_bootstrap_batch (a MultiScheme): out[j] = the bootstrap of ctxt[j] through table
    luts[sel[j]] (None: row 0).  out None = a new array where ctxt lives; out may be ctxt"""
    shape = tuple(np.shape(ctxt))
    B = _rows(shape)
    tb, nluts = _tables(luts, scheme.params)
    if out is None:
        out = _empty(ctxt, shape, np.uint32)
    return scheme._call("lut_bootstrap_batch", B, tb, nluts, _sel(sel, B), scheme._ct(ctxt, B), scheme._ct(out, B, out=True))[-1]


def lut_gather(scheme, luts, sel, pool, idx, wt, cst, out):
    """one circuit level of table lookups (mkt_lut_batch_gather): gate j bootstraps cst[j] on the b word + sum_t wt[j][t] * pool[idx[j][t]]
    through luts[sel[j]] -> out[j].  pool (rows, k*n+1); idx (B, 4) uint32 rows (int32 tensor), wt (B, 4) int8 weights (0: no term),
    cst (B,) uint32; sel (B,) or None; out may be a later region of the pool"""
    B, P = _count(cst), _rows(np.shape(pool))
    tb, nluts = _tables(luts, scheme.params)
    return scheme._call("lut_batch_gather", B, tb, nluts, _sel(sel, B), scheme._ct(pool, P), P, _Buf(idx, np.uint32, B, 4), _Buf(wt, np.int8, B, 4),
                        _Buf(cst, np.uint32, B), scheme._ct(out, B, out=True))[-1]


# ---- many-table bootstrap (include/mktfhe.h "many-table bootstrap"): nout functions of one input for one blind rotation ----
NOUT = (1, 2, 4, 8)


def _nout(nout, params):
    if nout not in NOUT or nout > params.N:
        raise ValueError(f"nout = {nout!r}: the table count must be 1, 2, 4 or 8 and at most N = {params.N}")
    return int(nout)


def lut_pack(tables, params: Params):
    """the packed table of nout = len(tables) tables laid out as lut_poly does: U[nout * i + v] = tables[v][nout * i].  tables (nout, N) ring
    words -> (N,) ring words; one table packs to itself"""
    rd = np.dtype(params.ring_dtype)
    t = np.asarray(tables)
    if t.dtype.kind not in "iu" or t.dtype.itemsize != rd.itemsize:
        raise ValueError(f"lookup tables of dtype {t.dtype}, expected {rd} (ring words)")
    if t.ndim != 2 or t.shape[1] != params.N:
        raise ValueError(f"tables of shape {t.shape}, expected (nout, {params.N})")
    o = _nout(t.shape[0], params)
    return np.ascontiguousarray(t.view(rd)[:, ::o].T).reshape(params.N)


def _out_many(scheme, ctxt, nout, out):
    """-> (B, out): out None = a new (..., nout, lwe_len) array where ctxt lives; a given out must hold exactly B * nout rows"""
    shape = tuple(np.shape(ctxt))
    B = _rows(shape)
    if out is None:
        out = _empty(ctxt, shape[:-1] + (nout, scheme.params.lwe_len), np.uint32)
    return B, out


def lut_many_testvector(scheme, luts, ctxt, nout, sel=None):
    """mkt_lut_many_testvector_batch: what the many-table bootstrap hands to blindrotate! -> (atilde (..., k*n) uint32 on the grid nout times
    coarser, acc (..., k + 1, N) ring words), living where ctxt lives.  luts: packed tables (lut_pack)"""
    p = scheme.params
    nout = _nout(nout, p)
    shape = tuple(np.shape(ctxt))
    B = _rows(shape)
    tb, nluts = _tables(luts, p)
    at = _empty(ctxt, shape[:-1] + (p.lwe_len - 1,), np.uint32)
    acc = _empty(ctxt, shape[:-1] + (p.k + 1, p.N), p.ring_dtype, "int64" if p.W == 64 else "int32")
    kept = scheme._call("lut_many_testvector_batch", B, tb, nluts, _sel(sel, B), scheme._ct(ctxt, B), nout, _Buf(at, np.uint32, B, p.lwe_len - 1, out=True),
                        _Buf(acc, p.ring_dtype, B * (p.k + 1) * p.N, out=True))
    return kept[-2], kept[-1]


def lut_extract(scheme, acc, nout):
    """mkt_lut_extract_batch: acc (..., k + 1, N) ring words -> (..., nout, k + 1, N), copy v = X^-v * acc (coefficient v moved to 0)"""
    p = scheme.params
    nout = _nout(nout, p)
    shape = tuple(np.shape(acc))
    if shape[-2:] != (p.k + 1, p.N):
        raise ValueError(f"accumulator of shape {shape}, expected (..., {p.k + 1}, {p.N})")
    B, words = int(np.prod(shape[:-2])), (p.k + 1) * p.N
    accs = _empty(acc, shape[:-2] + (nout,) + shape[-2:], p.ring_dtype)
    return scheme._call("lut_extract_batch", B, _Buf(acc, p.ring_dtype, B * words), nout, _Buf(accs, p.ring_dtype, B * nout * words, out=True))[-1]


def lut_many_bootstrap(scheme, luts, ctxt, nout, sel=None, out=None):
    """mkt_lut_many_bootstrap_batch (a Scheme) / mkt_multi_lut_many_bootstrap_batch (a MultiScheme): out[j][v] = the bootstrap of ctxt[j]
    through table v of the packed table luts[sel[j]] (None: row 0), nout tables for ONE blind rotation.  The input's words are rounded to a
    grid nout times coarser (noise).  out None = a new (..., nout, lwe_len) array where ctxt lives; out must not overlap ctxt
    when nout > 1"""
    nout = _nout(nout, scheme.params)
    B, out = _out_many(scheme, ctxt, nout, out)
    tb, nluts = _tables(luts, scheme.params)
    return scheme._call("lut_many_bootstrap_batch", B, tb, nluts, _sel(sel, B), scheme._ct(ctxt, B), nout, scheme._ct(out, B * nout, out=True))[-1]


def lut_many_gather(scheme, luts, sel, pool, idx, wt, cst, nout, out):
    """one circuit level of many-table lookups (mkt_lut_many_batch_gather): the linear front end of lut_gather, then lut_many_bootstrap.
    out: B * nout rows, output v of gate j at row j * nout + v; it may be a later region of the pool"""
    nout = _nout(nout, scheme.params)
    B, P = _count(cst), _rows(np.shape(pool))
    tb, nluts = _tables(luts, scheme.params)
    return scheme._call("lut_many_batch_gather", B, tb, nluts, _sel(sel, B), scheme._ct(pool, P), P, _Buf(idx, np.uint32, B, 4), _Buf(wt, np.int8, B, 4),
                        _Buf(cst, np.uint32, B), nout, scheme._ct(out, B * nout, out=True))[-1]


# ---- bootstrap at a coefficient list (include/mktfhe.h "key switch at a coefficient"): ncoef outputs of one blind rotation, no copy ----
def lut_threshold_coefs(P, params: Params):
    """the coefficients w * N / P, w < P: with sign_lut, output w of an input on window m of P (phase m / 2P + 1 / 4P) is + iff m >= w --
    the thermometer bits of a P-valued message from ONE rotation.  P divides N"""
    P = int(P)
    if P < 1 or params.N % P:
        raise ValueError(f"P = {P}: the window count must divide N = {params.N}")
    return np.array([w * (params.N // P) for w in range(P)], dtype=np.uint32)


def keyswitch_at(scheme, acc, src=None, coef=None):
    """mkt_keyswitch_at_batch (a Scheme): out[g] = keyswitch!(X^-coef[g] * acc[src[g]]) -- the key switch extracting at coefficient coef[g]
    of accumulator src[g], no rotated copy made.  acc: (..., k+1, N) ring words; src, coef: uint32 arrays (int32 tensors) of one shape living
    where acc lives; src None = row g of acc (as many rows as accumulators), coef None = 0.  Both None is scheme.keyswitch(acc), word for
    word.  -> (shape of src / coef / the accumulators, k*n+1) uint32 where acc lives"""
    p = scheme.params
    shape = tuple(np.shape(acc))
    if shape[-2:] != (p.k + 1, p.N):
        raise ValueError(f"accumulator of shape {shape}, expected (..., {p.k + 1}, {p.N})")
    nacc = int(np.prod(shape[:-2]))
    rows = shape[:-2] if src is None and coef is None else tuple(np.shape(coef if src is None else src))
    if src is not None and coef is not None and tuple(np.shape(coef)) != rows:
        raise ValueError(f"src of shape {rows} and coef of shape {tuple(np.shape(coef))}: one entry each per output row")
    B = int(np.prod(rows))
    out = _empty(acc, rows + (p.lwe_len,), np.uint32, "int32")
    return scheme._call("keyswitch_at_batch", B, _Buf(acc, p.ring_dtype, nacc * (p.k + 1) * p.N), nacc, None if src is None else _Buf(src, np.uint32, B),
                        None if coef is None else _Buf(coef, np.uint32, B), scheme._ct(out, B, out=True))[-1]


def _coef(coef, params):
    """-> the _Buf of a coefficient list and its length; a host list is checked here (1 .. N entries, each below N)"""
    if not _is_torch(coef):
        coef = np.ascontiguousarray(coef)
        if coef.dtype.kind not in "iu" or coef.ndim != 1 or not 1 <= coef.size <= params.N or coef.min() < 0 or coef.max() >= params.N:
            raise ValueError(f"coef: expected 1 .. {params.N} integers in [0, {params.N})")
        coef = coef.astype(np.uint32)
    n = _count(coef)
    return _Buf(coef, np.uint32, n), n


def _nu(nu, params):
    if nu not in (0, 1, 2, 3) or (1 << nu) > params.N:
        raise ValueError(f"nu = {nu!r}: the coarse mod-switch is 0 .. 3 with 2^nu at most N = {params.N}")
    return int(nu)


def lut_bootstrap_at(scheme, luts, ctxt, coef, nu=0, sel=None, out=None):
    """mkt_lut_bootstrap_at_batch (a Scheme) / mkt_multi_lut_bootstrap_at_batch (a MultiScheme): ONE blind rotation of ctxt[j] through table
    luts[sel[j]] (None: row 0), then out[j][i] = the key switch extracting at coefficient coef[i] -- what a bootstrap of the same table
    reads at phase phi - coef[i], for every i, at the noise of one bootstrap.  nu: the coarse mod-switch of the many-table
    form (0 = the fine one).  coef (ncoef,) lives where ctxt lives.  -> (..., ncoef, lwe_len); out must not overlap ctxt when ncoef > 1"""
    nu = _nu(nu, scheme.params)
    cb, ncoef = _coef(coef, scheme.params)
    B, out = _out_many(scheme, ctxt, ncoef, out)
    tb, nluts = _tables(luts, scheme.params)
    return scheme._call("lut_bootstrap_at_batch", B, tb, nluts, _sel(sel, B), scheme._ct(ctxt, B), nu, cb, ncoef, scheme._ct(out, B * ncoef, out=True))[-1]


def lut_gather_at(scheme, luts, sel, pool, idx, wt, cst, coef, out, nu=0):
    """one circuit level of lookups at a coefficient list (mkt_lut_batch_gather_at): the linear front end of lut_gather, then
    lut_bootstrap_at.  out: B * ncoef rows, output i of gate j at row j * ncoef + i; it may be a later region of the pool"""
    nu = _nu(nu, scheme.params)
    cb, ncoef = _coef(coef, scheme.params)
    B, P = _count(cst), _rows(np.shape(pool))
    tb, nluts = _tables(luts, scheme.params)
    return scheme._call("lut_batch_gather_at", B, tb, nluts, _sel(sel, B), scheme._ct(pool, P), P, _Buf(idx, np.uint32, B, 4), _Buf(wt, np.int8, B, 4),
                        _Buf(cst, np.uint32, B), nu, cb, ncoef, scheme._ct(out, B * ncoef, out=True))[-1]


def lwe_encrypt_word(mu, i, key: PartyKeys, params: Params, deterministic_seed=None):
    """lwe_ith_encrypt (scheme.jl:370-386) of ANY message mu on the 32-bit torus under party i (single-key schemes: 0): a multi-valued input
    of a programmable bootstrap.  mu = +-2^29 with the same pinned seed gives the words of lwe_ith_encrypt"""
    out = np.empty(params.lwe_len, dtype=np.uint32)
    sp, _keep = _seed_arg(deterministic_seed)
    check(_lib.lib().mkt_client_lwe_encrypt_word(C.byref(params.c()), key.h, i, int(mu) & 0xFFFFFFFF, params.alpha, sp, _np_ptr(out)))
    return out


def lwe_phase(ctxt, keys, params: Params):
    """the phase lwe_decrypt rounds (scheme.jl:388-407): message + noise as a uint32 torus word (an array of them for a batch)"""
    keys = [keys] if isinstance(keys, PartyKeys) else list(keys)
    arr = (C.c_void_p * len(keys))(*[k.h for k in keys])
    c = np.ascontiguousarray(ctxt, dtype=np.uint32)
    flat = c.reshape(-1, params.lwe_len)
    res = np.empty(flat.shape[0], dtype=np.uint32)
    ph = C.c_uint32(0)
    for j in range(flat.shape[0]):
        check(_lib.lib().mkt_client_lwe_phase(C.byref(params.c()), arr, len(keys), _np_ptr(flat[j]), C.byref(ph)))
        res[j] = ph.value
    return res.reshape(c.shape[:-1]) if c.ndim > 1 else int(res[0])
