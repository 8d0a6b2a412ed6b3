"""Host-side mirror of the reference's operator surface for the gate-bootstrapping path.

Reference (Julia, /root/reference/src): exports at MKTFHE.jl:21-35 --
    setup, party_keygen, CRS, lwe_encrypt, lwe_ith_encrypt, lwe_decrypt      tfhe/scheme.jl
    bootstrapping!                                                            tfhe/bootstrapping.jl:4
    NAND, AND, OR, XOR, XNOR, NOR, NOT!                                       tfhe/gate.jl
plus the internal blindrotate! / keyswitch! named by the north star.  Same names and argument
meaning (`!` dropped: in-place functions carry a trailing underscore); every ciphertext argument
is a BATCH: a numpy uint32 array (..., k*n+1) in host memory or a torch CUDA int32/uint32 tensor
(device memory, zero copy).  All compute goes through the C ABI (include/mktfhe.h); this module
holds no arithmetic of its own and raises if the HIP library or a gfx950 GPU is missing.
"""
import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import MktError, check
from .params import CCS, Params

MEM_DEVICE, MEM_HOST = 0, 1
FMT_INT_COEFF, FMT_F64_FFT = 0, 1
ARITH_F64REF, ARITH_EXACT = 0, 1


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _arg(x, dtype, writable=False):
    """-> (pointer, mem kind, keepalive)"""
    if _is_torch(x):
        if not x.is_cuda:
            raise ValueError("torch tensors must live on the GPU; pass numpy arrays for host memory")
        if not x.is_contiguous():
            raise ValueError("tensor must be contiguous")
        if x.element_size() != np.dtype(dtype).itemsize:
            raise ValueError(f"tensor element size {x.element_size()} does not match {np.dtype(dtype)}")
        return C.c_void_p(x.data_ptr()), MEM_DEVICE, x
    a = np.ascontiguousarray(x, dtype=dtype)
    if writable and a is not x:
        raise ValueError("output / in-place argument must be a contiguous numpy array of dtype %s" % np.dtype(dtype))
    return _np_ptr(a), MEM_HOST, a


def _rows(shape):
    """gates in an array of shape (..., row): a 1-D array is one"""
    return int(np.prod(shape[:-1])) if len(shape) > 1 else 1


def _count(x):
    return int(np.prod(np.shape(x)))


def _empty(like, shape, dtype, tdtype=None):
    """a new array of `shape` living where `like` lives: numpy `dtype` on the host; on the GPU a tensor of the torch type named
    `tdtype`, by default like's own"""
    if _is_torch(like):
        import torch
        return like.new_empty(shape, dtype=getattr(torch, tdtype) if tdtype else like.dtype)
    return np.empty(shape, dtype=dtype)


def _one_shape(x, *others, out, dtype=np.uint32):
    """-> (B, out) of a batch-ordered call: the other operands and out have x's shape; out None = a new array where x lives"""
    shape = tuple(np.shape(x))
    if out is None:
        out = _empty(x, shape, dtype)
    if any(tuple(np.shape(v)) != shape for v in (*others, out)):
        raise ValueError(f"operands and out must all have the shape {shape}")
    return _rows(shape), out


class _Buf(NamedTuple):
    """a buffer argument of a batch call: it must hold n rows of `row` elements (shape (..., row)), or, with row None, n elements in any
    shape -- exactly what the C function reads or writes through it.  out: the library writes it, so a host array must already be
    contiguous and of `dtype`"""
    x: object
    dtype: type
    n: int
    row: int = None
    out: bool = False


# ------------------------------------------------------------------------------------------------
# client side: CRS, party_keygen / setup keys, encrypt, decrypt  (CPU, exact integer arithmetic)
# ------------------------------------------------------------------------------------------------
def _seed_arg(deterministic_seed):
    """-> (pointer or None, keepalive).  None (the default everywhere) = the library draws a fresh 256-bit seed from the
    OS for this call, like the reference's per-call ChaCha20 entropy (sampler.jl:1-34).  An int (tests / benchmarks
    ONLY: the result is reproducible, hence public) is expanded by mkt_client_test_seed; 32 bytes are used as they are."""
    if deterministic_seed is None:
        return None, None
    buf = (C.c_uint8 * 32)()
    if isinstance(deterministic_seed, (bytes, bytearray)):
        if len(deterministic_seed) != 32:
            raise ValueError("a seed is 32 bytes")
        buf[:] = deterministic_seed
    else:
        check(_lib.lib().mkt_client_test_seed(int(deterministic_seed) & (2**64 - 1), buf))
    return C.cast(buf, C.c_void_p), buf


def _seed32(seed):
    """a public 32-byte seed -> (pointer, keepalive)"""
    if not isinstance(seed, (bytes, bytearray)) or len(seed) != 32:
        raise ValueError("a mask seed is 32 bytes")
    buf = (C.c_uint8 * 32)(*seed)
    return C.cast(buf, C.c_void_p), buf


def _row0(row0):
    """the index of a call's first row in a larger batch under one seed, as the library takes it: 64 bits"""
    row0 = int(row0)
    if not 0 <= row0 < 2**64:
        raise ValueError("row0 must fit 64 bits")
    return row0


def CRS(params: Params, deterministic_seed=None):
    """scheme.jl:409-410 CRS(params): l_uni uniform ring polynomials -> (l_uni, N) ring words.
    Fresh OS randomness unless `deterministic_seed` (tests / benchmarks only) pins it."""
    out = np.empty((params.l_uni, params.N), dtype=params.ring_dtype)
    sp, _keep = _seed_arg(deterministic_seed)
    check(_lib.lib().mkt_client_crs(C.byref(params.c()), sp, _np_ptr(out)))
    return out


class PartyKeys:
    """One party's secret and evaluation keys (party_keygen, scheme.jl:227,:273,:324; setup for the
    single-key schemes, scheme.jl:151,:190).  Evaluation keys are in integer (coefficient) form."""

    def __init__(self, params: Params, party=0, crs=None, secrets_only=False, deterministic_seed=None, seeded=False, mask_seed=None):
        """Keys are drawn from fresh OS randomness; `deterministic_seed` (an int, or 32 bytes) pins the streams for
        tests and benchmarks ONLY -- such keys are reproducible by anyone.
        secrets_only: leave out the two large keys (bootstrapping key, key-switching key); they are then generated
        on the GPU by Scheme.keygen_device from the same streams (identical words).  That hands this party's secrets
        to that GPU: a party-local step (own machine), not something an evaluator does for every party.
        seeded: the seeded key form (mktfhe.h "seeded evaluation keys"): the two large keys as a PUBLIC 32-byte mask seed
        (mask_seed; None draws a fresh one) and their bodies (brk_seeded, ksk_seeded); brk and ksk are None.  A (mask seed,
        party) pair serves one key generation."""
        self.params, self.party, self.secrets_only, self.seeded = params, party, secrets_only and not seeded, bool(seeded)
        h = C.c_void_p()
        self._crs = np.ascontiguousarray(crs, dtype=params.ring_dtype) if crs is not None else None
        crs_p = _np_ptr(self._crs) if crs is not None else None
        sp, _keep = _seed_arg(deterministic_seed)
        if seeded:
            if mask_seed is None:
                buf = (C.c_uint8 * 32)()
                check(_lib.lib().mkt_client_random_seed(buf))
                mask_seed = bytes(buf)
            mp, _mkeep = _seed32(mask_seed)
            check(_lib.lib().mkt_client_party_keygen_seeded(C.byref(params.c()), sp, mp, party, crs_p, params.alpha, params.beta, C.byref(h)))
        else:
            fn = _lib.lib().mkt_client_party_secrets if secrets_only else _lib.lib().mkt_client_party_keygen
            check(fn(C.byref(params.c()), sp, party, crs_p, params.alpha, params.beta, C.byref(h)))
        self.h = h

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            try:
                _lib.lib().mkt_client_party_destroy(self.h)
            except Exception:       # interpreter shutdown: the library may already be gone
                pass
            self.h = None

    def _view(self, addr, nbytes, dtype):
        """zero-copy numpy view of key material owned by the C object; the view keeps this PartyKeys (and with it the
        memory) alive"""
        raw = (C.c_uint8 * nbytes).from_address(addr)
        raw._owner = self
        return np.frombuffer(raw, dtype=dtype)

    def _buf(self, fn, dtype):
        n = C.c_size_t(0)
        p = fn(self.h, C.byref(n))
        if not n.value:
            return None
        return self._view(p, n.value, dtype)

    @property
    def lwekey(self):
        return self._view(_lib.lib().mkt_client_lwekey(self.h), 4 * self.params.n, np.uint32)

    def ringkey(self, idx=0):
        """ring secret polynomial idx as int8 [N] (SK schemes: idx < k; CCS: 0; KMS: 0 = gsw key, 1 = uni key)"""
        n = C.c_size_t(0)
        p = _lib.lib().mkt_client_ringkey(self.h, idx, C.byref(n))
        return self._view(p, n.value, np.int8) if n.value else None

    @property
    def brk(self):
        return self._buf(_lib.lib().mkt_client_brk, self.params.ring_dtype)

    @property
    def ksk(self):
        return self._buf(_lib.lib().mkt_client_ksk, np.uint32)

    @property
    def mask_seed(self):
        """the public 32-byte mask seed of a seeded party, else None"""
        p = _lib.lib().mkt_client_mask_seed(self.h)
        return bytes((C.c_uint8 * 32).from_address(p)) if p else None

    @property
    def brk_seeded(self):
        return self._buf(_lib.lib().mkt_client_brk_seeded, self.params.ring_dtype)

    @property
    def ksk_seeded(self):
        return self._buf(_lib.lib().mkt_client_ksk_seeded, np.uint32)

    @property
    def rlk_d(self):
        return self._buf(_lib.lib().mkt_client_rlk_d, self.params.ring_dtype)

    @property
    def rlk_f(self):
        return self._buf(_lib.lib().mkt_client_rlk_f, self.params.ring_dtype)

    @property
    def pubkey(self):
        return self._buf(_lib.lib().mkt_client_pubkey, self.params.ring_dtype)


def party_keygen(a, params: Params, party=0, secrets_only=False, deterministic_seed=None, seeded=False, mask_seed=None):
    """scheme.jl:227/:273/:324 party_keygen(a, params) -> PartyKeys (lwekey + bootstrapping key); fresh randomness
    per call unless `deterministic_seed` (tests / benchmarks only) is given.  seeded=True: the seeded key form (a public
    mask seed and the bodies of the two large keys; PartyKeys)"""
    return PartyKeys(params, party=party, crs=a, secrets_only=secrets_only, deterministic_seed=deterministic_seed, seeded=seeded, mask_seed=mask_seed)


def lwe_encrypt(m, key: PartyKeys, params: Params, deterministic_seed=None):
    """scheme.jl:352-368 lwe_encrypt(m, key, params) (single-key schemes); fresh mask and noise per call"""
    return lwe_ith_encrypt(m, 0, key, params, deterministic_seed)


def lwe_ith_encrypt(m, i, key: PartyKeys, params: Params, deterministic_seed=None):
    """scheme.jl:370-386 lwe_ith_encrypt(m, i, key, params); i is the 0-based party index.  Mask and noise come from
    fresh OS randomness on every call; `deterministic_seed` (tests / benchmarks only) pins them"""
    out = np.empty(params.lwe_len, dtype=np.uint32)
    sp, _keep = _seed_arg(deterministic_seed)
    check(_lib.lib().mkt_client_lwe_encrypt(C.byref(params.c()), key.h, i, int(bool(m)), params.alpha, sp, _np_ptr(out)))
    return out


def lwe_decrypt(ctxt, keys, params: Params):
    """scheme.jl:388-407 lwe_decrypt(lwe, key(s)[, params]) -> bool (or array of bool for a batch)"""
    keys = [keys] if isinstance(keys, PartyKeys) else list(keys)
    arr = (C.c_void_p * len(keys))(*[k.h for k in keys])
    c = np.ascontiguousarray(ctxt, dtype=np.uint32)
    flat = c.reshape(-1, params.lwe_len)
    res = np.empty(flat.shape[0], dtype=bool)
    for j in range(flat.shape[0]):
        res[j] = bool(check(_lib.lib().mkt_client_lwe_decrypt(C.byref(params.c()), arr, len(keys), _np_ptr(flat[j]))))
    return res.reshape(c.shape[:-1]) if c.ndim > 1 else bool(res[0])


# ------------------------------------------------------------------------------------------------
# evaluator: the scheme object lives on one MI355X
# ------------------------------------------------------------------------------------------------
class _Batched:
    """The batch methods Scheme and MultiScheme share, and the one checked path every batch call of either class takes.  The C ABI
    takes plain pointers and a batch count B, so _call is where each buffer's size is compared with what the library reads or writes."""
    _PREFIX = "mkt_"

    def _follow_torch(self, tensors):
        """hook run once per call with GPU tensor arguments, before the library call: MultiScheme takes tensors on any device, and its
        calls are synchronous"""

    def _ct(self, x, n, out=False):
        return _Buf(x, np.uint32, n, self.params.lwe_len, out)

    def _call(self, name, B, *args):
        """_PREFIX + name called as (handle, *args, B, mem), every _Buf in args passed as its pointer -> the _Bufs as _arg resolved
        them, in order.  Before any library call: ValueError unless all of them live in one memory kind and each holds exactly what
        the C function reads or writes for B gates"""
        fn, cargs, kept, mems = self._PREFIX + name, [], [], set()
        for a in args:
            if isinstance(a, _Buf):
                ptr, mem, k = _arg(a.x, a.dtype, writable=a.out)
                shape = tuple(k.shape)
                if a.row is None:
                    ok, want = int(np.prod(shape)) == a.n, f"{a.n} elements"
                else:
                    ok, want = shape[-1:] == (a.row,) and _rows(shape) == a.n, f"{a.n} rows of {a.row}"
                if not ok:
                    raise ValueError(f"{fn}: an argument of shape {shape}, expected {want}")
                a = ptr
                kept.append(k)
                mems.add(mem)
            cargs.append(a)
        if len(mems) > 1:
            raise ValueError(f"{fn}: all arguments must be host arrays or all be GPU tensors")
        mem = mems.pop()
        if mem == MEM_DEVICE:
            self._follow_torch(kept)
        self._ck(getattr(_lib.lib(), fn)(self.h, *cargs, B, mem))
        return kept

    # -- keys (MultiScheme: once, on the first device; replicate() copies them to the others)
    def load_party(self, party, keys: "PartyKeys" = None, *, brk=None, ksk=None, rlk_d=None, rlk_f=None, pubkey=None, fmt=FMT_INT_COEFF,
                   mask_seed=None, brk_seeded=None, ksk_seeded=None):
        """upload one party's evaluation keys.  A seeded party (PartyKeys(seeded=True)), or mask_seed with brk_seeded / ksk_seeded, goes
        through mkt_load_seeded_keys: the masks are regenerated on the GPU, the expanded keys never exist on the host"""
        fn = lambda name: getattr(_lib.lib(), self._PREFIX + name)      # noqa: E731
        if keys is not None:
            brk, ksk, rlk_d, rlk_f, pubkey = keys.brk, keys.ksk, keys.rlk_d, keys.rlk_f, keys.pubkey
            if getattr(keys, "seeded", False):
                mask_seed, brk_seeded, ksk_seeded = keys.mask_seed, keys.brk_seeded, keys.ksk_seeded
        if mask_seed is not None:
            _load_seeded(self, party, mask_seed, brk_seeded, ksk_seeded)
        kd = np.complex128 if fmt == FMT_F64_FFT else self.params.ring_dtype
        if brk is not None:
            self._ck(fn("load_brk")(self.h, party, _np_ptr(np.ascontiguousarray(brk, dtype=kd)), fmt))
        if ksk is not None:
            self._ck(fn("load_ksk")(self.h, party, _np_ptr(np.ascontiguousarray(ksk, dtype=np.uint32))))
        if rlk_d is not None:
            self._ck(fn("load_rlk")(self.h, party, _np_ptr(np.ascontiguousarray(rlk_d, dtype=kd)), _np_ptr(np.ascontiguousarray(rlk_f, dtype=kd)), fmt))
        if pubkey is not None:
            self._ck(fn("load_pubkey")(self.h, party, _np_ptr(np.ascontiguousarray(pubkey, dtype=kd)), fmt))

    def load_crs(self, a, fmt=FMT_INT_COEFF):
        kd = np.complex128 if fmt == FMT_F64_FFT else self.params.ring_dtype
        self._ck(getattr(_lib.lib(), self._PREFIX + "load_crs")(self.h, _np_ptr(np.ascontiguousarray(a, dtype=kd)), fmt))

    def gate(self, op, x, y, out=None):
        B, out = _one_shape(x, y, out=out)
        return self._call("gate_batch", B, op, self._ct(x, B), self._ct(y, B), self._ct(out, B, out=True))[-1]

    def gate_ops(self, ops, x, y, out=None):
        """a different gate per ciphertext pair (mkt_gate_batch_ops; the reference's tests draw a random gate per step,
        test/KMS.jl:29-34): ops[j] in 0..5 (NAND..NOR), optionally | OP_NOT_X / OP_NOT_Y (that input negated first, NOT!);
        a uint8 array living where x and y live"""
        B, out = _one_shape(x, y, out=out)
        return self._call("gate_batch_ops", B, _Buf(ops, np.uint8, B), self._ct(x, B), self._ct(y, B), self._ct(out, B, out=True))[-1]

    def gate3(self, op, x, y, z, out=None):
        """a three-input gate in ONE bootstrap for the whole batch (MAJ3_OP .. AE3_OP, optionally | OP_NOT_X / _Y / _Z): gate3_ops with
        one code"""
        return self.gate3_ops(_full_ops(op, x, _rows(np.shape(x))), x, y, z, out)

    def gate3_ops(self, ops, x, y, z, out=None):
        """a three-input gate per ciphertext triple, one bootstrap each (mkt_gate3_batch_ops): ops[j] in 0..5 (MAJ3..AE3), optionally
        | OP_NOT_X / OP_NOT_Y / OP_NOT_Z; a uint8 array living where x, y and z live"""
        B, out = _one_shape(x, y, z, out=out)
        return self._call("gate3_batch_ops", B, _Buf(ops, np.uint8, B), self._ct(x, B), self._ct(y, B), self._ct(z, B), self._ct(out, B, out=True))[-1]

    def mux(self, s, a, b, out=None):
        """MUX(s, a, b) = s ? a : b with two blind rotations and one key switch (mkt_mux_batch; the reference has no MUX gate)"""
        B, out = _one_shape(s, a, b, out=out)
        return self._call("mux_batch", B, self._ct(s, B), self._ct(a, B), self._ct(b, B), self._ct(out, B, out=True))[-1]

    def bootstrapping_(self, ctxt):
        B = _rows(np.shape(ctxt))
        return self._call("bootstrap_batch", B, self._ct(ctxt, B, out=True))[0]

    def not_(self, ctxt):
        B = _rows(np.shape(ctxt))
        return self._call("not_batch", B, self._ct(ctxt, B, out=True))[0]

    def blindrotate_(self, atilde, acc):
        """acc: (k+1) * N ring words per ciphertext of atilde, in any shape"""
        p = self.params
        B = _rows(np.shape(atilde))
        return self._call("blindrotate_batch", B, _Buf(atilde, np.uint32, B, p.lwe_len - 1), _Buf(acc, p.ring_dtype, B * (p.k + 1) * p.N, out=True))[1]

    def keyswitch(self, acc):
        """acc: (..., k+1, N) ring words"""
        p = self.params
        shape = tuple(np.shape(acc))
        if shape[-2:] != (p.k + 1, p.N):
            raise ValueError(f"accumulator of shape {shape}, expected (..., {p.k + 1}, {p.N})")
        B = int(np.prod(shape[:-2]))
        out = np.empty(shape[:-2] + (p.lwe_len,), dtype=np.uint32)
        return self._call("keyswitch_batch", B, _Buf(acc, p.ring_dtype, B * (p.k + 1) * p.N), self._ct(out, B, out=True))[1]


def seeded_section_words(params: Params):
    """(ring words of brk_seeded, words of ksk_seeded) of one party (include/mktfhe.h "seeded evaluation keys", compact layouts)"""
    return params.brk_seeded_words, params.ksk_rows


def _seeded_sections(params, brk_seeded, ksk_seeded):
    """the compact sections as contiguous arrays of exactly the lengths the library reads -> (brk or None, ksk or None)"""
    wb, wk = seeded_section_words(params)
    out = []
    for name, v, dt, want in (("brk_seeded", brk_seeded, params.ring_dtype, wb), ("ksk_seeded", ksk_seeded, np.uint32, wk)):
        if v is not None:
            v = np.ascontiguousarray(v, dtype=dt)
            if v.size != want:
                raise ValueError(f"{name} holds {v.size} words, these parameters need {want}")
        out.append(v)
    return out


def _load_seeded(sch, party, mask_seed, brk_seeded, ksk_seeded):
    """mkt_load_seeded_keys / mkt_multi_load_seeded_keys on a Scheme / MultiScheme: sizes checked before the library is called"""
    b, k = _seeded_sections(sch.params, brk_seeded, ksk_seeded)
    if b is None and k is None:
        raise ValueError("a mask seed without a compact section")
    mp, _keep = _seed32(mask_seed)
    fn = getattr(_lib.lib(), sch._PREFIX + "load_seeded_keys")
    sch._ck(fn(sch.h, int(party), mp, None if b is None else _np_ptr(b), None if k is None else _np_ptr(k)))


class Scheme(_Batched):
    """The reference's CGGI / LMSS / CCS / KMS / KMS_block scheme object (scheme.jl:107-116, :168-179,
    :209-219, :256-265, :301-312) as a per-device engine context: twiddle tables (fft.jl:18-45),
    monomial table (scheme.jl:121-146) and the pre-transformed evaluation keys, all resident in HBM."""

    def __init__(self, params: Params, device=0, arith=ARITH_F64REF):
        self.params = params
        self.device = device
        h = C.c_void_p()
        check(_lib.lib().mkt_ctx_create(C.byref(params.c()), arith, device, C.byref(h)))
        self.h = h
        self.arith = arith
        self._user_stream = False     # True once set_stream pinned a stream; else torch's current stream is followed

    def _follow_torch(self, tensors):
        """GPU tensors must live on this scheme's device; unless the caller pinned a stream with set_stream, the engine enqueues on
        torch's CURRENT stream of that device, so its kernels are ordered with the producer and the consumer of the tensors like any
        torch op.  Calls on one Scheme run in the order they were made, whatever stream each was enqueued on: when the current stream
        has changed since the last call, mkt_set_stream makes the new one wait for what this Scheme enqueued on the old one (the
        workspace is the Scheme's); while it stays the same the call below does nothing"""
        for t in tensors:
            if t.device.index != self.device:
                raise ValueError(f"tensor lives on cuda:{t.device.index}, this scheme on device {self.device}")
        if not self._user_stream:
            import torch
            self._ck(_lib.lib().mkt_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(tensors[0].device).cuda_stream)))

    def fork(self):
        """a second Scheme over the SAME resident keys (mkt_ctx_fork: no copy) with its own stream and workspace -- one
        per concurrent caller, as concurrent bootstrapping! calls share one read-only scheme object in the reference.
        From then on the keys are immutable on every sharer."""
        f = object.__new__(Scheme)
        f.params, f.device, f.arith, f._user_stream = self.params, self.device, self.arith, False
        h = C.c_void_p()
        self._ck(_lib.lib().mkt_ctx_fork(self.h, C.byref(h)))
        f.h = h
        return f

    def close(self):
        if getattr(self, "h", None):
            if getattr(self, "_owned", True):        # a borrowed view (MultiScheme.shard) never destroys the context
                try:
                    _lib.lib().mkt_ctx_destroy(self.h)
                except Exception:                    # interpreter shutdown: the module globals may already be gone
                    pass
            self.h = None

    __del__ = close

    def _ck(self, code):
        return check(code, self.h)

    # -- keys (load_party, load_crs: _Batched)
    def keygen_device(self, party, keys: PartyKeys, export=False):
        """keygen.jl:13-23 etc. on the GPU: bootstrapping + key-switching key of `party` from its secrets (the small
        keys -- public key, relinearisation key -- are uploaded from `keys`).  This hands the party's SECRETS to this
        context's GPU: it is the party's own step.  export=True also returns (brk, ksk) in the integer layouts of
        load_party, i.e. what the party ships to the evaluator (keyblob.dump_arrays)."""
        L = _lib.lib()
        crs_p = _np_ptr(keys._crs) if (self.params.scheme == CCS and keys._crs is not None) else None
        out = None
        if export:
            brk = np.empty(self.brk_words(), dtype=self.params.ring_dtype)
            ksk = np.empty(self.get_ksk_shape(), dtype=np.uint32)
            self._ck(L.mkt_keygen_device_export(self.h, party, keys.h, crs_p, _np_ptr(brk), _np_ptr(ksk)))
            out = (brk, ksk.ravel())
        else:
            self._ck(L.mkt_keygen_device(self.h, party, keys.h, crs_p))
        self.load_party(party, rlk_d=keys.rlk_d, rlk_f=keys.rlk_f, pubkey=keys.pubkey)
        return out

    def brk_words(self):
        """ring words of one party's bootstrapping key (include/mktfhe.h layouts)"""
        return self.params.brk_words

    def get_ksk_shape(self):
        return (self.params.ksk_rows, self.params.n + 1)

    def get_ksk(self, party):
        out = np.empty(self.get_ksk_shape(), dtype=np.uint32)
        self._ck(_lib.lib().mkt_get_ksk(self.h, party, _np_ptr(out)))
        return out

    def set_stream(self, stream_handle):
        """pin the HIP stream (hipStream_t handle) every later call is enqueued on; None = back to the default:
        follow torch's current stream for GPU tensors (the NULL stream for host arrays)"""
        self._user_stream = stream_handle is not None
        self._ck(_lib.lib().mkt_set_stream(self.h, C.c_void_p(stream_handle or 0)))

    def synchronize(self):
        self._ck(_lib.lib().mkt_synchronize(self.h))

    def get_stream(self):
        """the hipStream_t handle (int) this context enqueues on right now (a fork: its own non-blocking stream)"""
        st = C.c_void_p()
        self._ck(_lib.lib().mkt_get_stream(self.h, C.byref(st)))
        return st.value or 0

    def set_option(self, name, value):
        """kernel-selection switch (mkt_set_option; INTEGRATION.md "Runtime switches"): "rot_wide", "rot_blkg", "rot_variant",
        "rot_map", "rot_split", "rot_stagger", "ccs_stagger", "ccs_pipe", "exact_impl", "exact_wide", "exact_kany", "fx_polymul_force".
        Results never depend on them (tests/test_gpu_switches.py forces each one).  An unknown name, rot_variant
        outside {0, 21, 22} or rot_map outside {0, 1} raises MktError and leaves the context as it was.  The launcher-level
        MKT_KS_* / MKT_FFT_* / MKT_NTT_GRID switches are environment variables read once per process, not options."""
        self._ck(_lib.lib().mkt_set_option(self.h, name.encode(), int(value)))

    def get_metric(self, name):
        """diagnostics of the Float64-pipe EXACT implementation (mkt_get_metric): "fx_available", "fx_bound", "fx_kmax"; of the last exact_polymul:
        "polymul_amax", "fx_polymul_bound" (-1: not evaluated), "fx_last_resid" (a diagnostic, not a certificate); of the rotation launch that
        last_kernel_name() names: "rot_static_l", "rot_static_logB" (the instantiation's compile-time gadget, 0 = taken at run time); of the
        guard mode of the engine's device memory (MKT_MEM_GUARD in the environment when the context is created; mktfhe.h): "mem_guard_check"
        (drains the device, compares every guard, -> guards found written since the process started), "mem_guard_buffers" and "mem_guard_released";
        of the context's last key switch: "ks_last_kernel" (0 none yet, 1 per-digit, 2 digit-pair, 3 matrix cores), "ks_last_g", "ks_last_waves", "ks_last_slabs" """
        v = C.c_double(0.0)
        self._ck(_lib.lib().mkt_get_metric(self.h, name.encode(), C.byref(v)))
        return v.value

    def last_kernel_name(self):
        """base name of the blind-rotation kernel the last batch call launched (after exact_polymul: the product kernel that served it)"""
        return (_lib.lib().mkt_last_kernel_name(self.h) or b"").decode()

    # -- tables (tests)
    def twiddles(self, which):
        out = np.empty(self.params.N // 2, dtype=np.complex128)
        self._ck(_lib.lib().mkt_get_twiddles(self.h, which, _np_ptr(out)))
        return out

    def monomial(self, e):
        out = np.empty(self.params.N // 2, dtype=np.complex128)
        self._ck(_lib.lib().mkt_get_monomial(self.h, e, _np_ptr(out)))
        return out

    # -- timing
    def enable_timing(self, on=True):
        self._ck(_lib.lib().mkt_enable_timing(self.h, int(on)))

    def kernel_ms(self, which):
        """(total ms, launches) of kernel class `which` since enable_timing: 0 whole call, 1 blind
        rotation, 2 key switch, 3 transform, 4 KMS phase 2"""
        ms = C.c_double(0)
        n = self._ck(_lib.lib().mkt_last_kernel_ms(self.h, which, C.byref(ms)))
        return ms.value, n

    # -- hot path: the shared batch methods (_Batched) and these
    def gate_gather(self, ops, pool, ix, iy, out):
        """one circuit level (mkt_gate_batch_gather): gate j = ops[j](pool[ix[j]], pool[iy[j]]) -> out[j]; pool (rows, k*n+1),
        ix / iy uint32 (int32 tensors) row indices; out may be a later region of the pool"""
        B, P = _count(ops), _rows(np.shape(pool))
        return self._call("gate_batch_gather", B, _Buf(ops, np.uint8, B), self._ct(pool, P), P, _Buf(ix, np.uint32, B), _Buf(iy, np.uint32, B),
                          self._ct(out, B, out=True))[-1]

    def gate3_gather(self, ops, pool, ix, iy, iz, out):
        """one circuit level of three-input gates (mkt_gate3_batch_gather): gate j = ops[j](pool[ix[j]], pool[iy[j]], pool[iz[j]]) -> out[j];
        out may be a later region of the pool"""
        B, P = _count(ops), _rows(np.shape(pool))
        return self._call("gate3_batch_gather", B, _Buf(ops, np.uint8, B), self._ct(pool, P), P, _Buf(ix, np.uint32, B), _Buf(iy, np.uint32, B),
                          _Buf(iz, np.uint32, B), self._ct(out, B, out=True))[-1]

    def mux_gather(self, pool, i_s, i_a, i_b, out, not_ab=None):
        """a circuit level of native MUX gates (mkt_mux_batch_gather): out[j] = MUX(pool[i_s[j]], a', b'), a' = pool[i_a[j]] or its
        negation if bit 0 of not_ab[j] is set (b' likewise, bit 1)"""
        B, P = _count(i_s), _rows(np.shape(pool))
        return self._call("mux_batch_gather", B, self._ct(pool, P), P, _Buf(i_s, np.uint32, B), _Buf(i_a, np.uint32, B), _Buf(i_b, np.uint32, B),
                          None if not_ab is None else _Buf(not_ab, np.uint8, B), self._ct(out, B, out=True))[-1]

    def modswitch(self, ctxt):
        shape = tuple(np.shape(ctxt))
        B = _rows(shape)
        at = np.empty(shape[:-1] + (self.params.lwe_len - 1,), dtype=np.uint32)
        bt = np.empty(shape[:-1] if len(shape) > 1 else (1,), dtype=np.uint32)
        self._call("modswitch_batch", B, self._ct(ctxt, B), _Buf(at, np.uint32, B, self.params.lwe_len - 1, out=True), _Buf(bt, np.uint32, B, out=True))
        return at, bt

    def kms_phase1(self, atilde):
        p = self.params
        shape = tuple(np.shape(atilde))
        B = _rows(shape)
        rtot = 1 + (p.k - 1) * p.l_lev
        if self.arith == ARITH_EXACT:    # split residue tables: [rows][polynomial b / a][low / high 32-bit half][N] residue pairs, Montgomery form
            row, dt = (rtot, 2, 2, p.N), np.uint64
        else:
            row, dt = (rtot, 2, p.N // 2), np.complex128
        out = np.empty(shape[:-1] + row, dtype=dt)
        return self._call("kms_phase1_batch", B, _Buf(atilde, np.uint32, B, p.lwe_len - 1), _Buf(out, dt, B * int(np.prod(row)), out=True))[1]

    def transform_fwd(self, p, out=None):
        N, shape = self.params.N, tuple(np.shape(p))
        B = _rows(shape)
        if out is None:
            out = _empty(p, shape[:-1] + (N // 2,), np.complex128, "complex128")
        return self._call("transform_fwd_batch", B, _Buf(p, self.params.ring_dtype, B, N), _Buf(out, np.complex128, B, N // 2, out=True))[1]

    def transform_inv(self, t, out=None):
        N, shape = self.params.N, tuple(np.shape(t))
        B = _rows(shape)
        if out is None:
            out = _empty(t, shape[:-1] + (N,), self.params.ring_dtype, "int64" if self.params.W == 64 else "int32")
        return self._call("transform_inv_batch", B, _Buf(t, np.complex128, B, N // 2), _Buf(out, self.params.ring_dtype, B, N, out=True))[1]

    def exact_polymul(self, a, b, out=None):
        """MKT_ARITH_EXACT contexts: a (*) b mod (X^N + 1, 2^W), exactly, for digit polynomials a (signed W-bit words,
        N * max|a_i| <= 2^28 - 2^15 over the batch: outside it the call raises MktError and writes nothing) and ring polynomials b;
        (..., N) numpy arrays, or GPU tensors of the ring's word size.  Under exact_impl = 1 the Float64 pipe serves the call where its
        proven bound certifies the operands, the integer NTT otherwise (same words; last_kernel_name() says which)"""
        rd, N = self.params.ring_dtype, self.params.N
        B, out = _one_shape(a, b, out=out, dtype=rd)
        return self._call("exact_polymul_batch", B, _Buf(a, rd, B, N), _Buf(b, rd, B, N), _Buf(out, rd, B, N, out=True))[-1]

    def decompose(self, p, l, logB):
        rd, N, shape = self.params.ring_dtype, self.params.N, tuple(np.shape(p))
        B = _rows(shape)
        out = np.empty(shape[:-1] + (l, N), dtype=rd)
        return self._call("decompose_batch", B, _Buf(p, rd, B, N), _Buf(out, rd, B * l, N, out=True), l, logB)[1]


OP_NOT_X, OP_NOT_Y = 8, 16      # mktfhe.h MKT_OP_NOT_X / _Y: per-gate code bits of gate_ops / gate_gather
OP_NOT_Z = 32                   # mktfhe.h MKT_OP_NOT_Z: the third input of gate3_ops / gate3_gather


def _full_ops(op, like, B):
    """B copies of one gate code, living where `like` lives"""
    if _is_torch(like):
        import torch
        return torch.full((B,), int(op), dtype=torch.uint8, device=like.device)
    return np.full(B, op, dtype=np.uint8)


class MultiScheme(_Batched):
    """ONE scheme object over several MI355X (mkt_multi_*): the reference's caller is one process whose threads
    share one read-only scheme (README.md:38-44, bootstrapping.jl:38-45); here the batch is cut into contiguous shards, one per
    entry of `devices` (a device named twice = two logical shards over that device's one key set), keys uploaded once and
    replicated device-to-device, every shard writing its slice of the caller's one output array.  No collective.  Same batch
    methods as Scheme; arrays are host numpy arrays or GPU tensors on ANY of the devices."""
    _PREFIX = "mkt_multi_"

    def __init__(self, params: Params, devices, arith=ARITH_F64REF, private_keys=False, stage_always=False, no_peer=False):
        """private_keys: shards that share a device each get their own replicated key copy (MKT_MULTI_PRIVATE_KEYS: the
        device-to-device replication path, testable on one GPU) instead of sharing that device's one key set"""
        self.params, self.devices, self.arith = params, list(devices), arith
        h = C.c_void_p()
        arr = (C.c_int * len(self.devices))(*self.devices)
        code = _lib.lib().mkt_multi_create(C.byref(params.c()), arith, arr, len(self.devices), (1 if private_keys else 0) | (2 if stage_always else 0) | (4 if no_peer else 0), C.byref(h))
        if code < 0:
            raise MktError(code, (_lib.lib().mkt_multi_last_error(None) or b"").decode())
        self.h = h
        self._sealed = False

    def _ck(self, code):
        if code < 0:
            raise MktError(code, (_lib.lib().mkt_multi_last_error(self.h) or b"").decode())
        return code

    def close(self):
        if getattr(self, "h", None):
            try:
                _lib.lib().mkt_multi_destroy(self.h)
            except Exception:                        # interpreter shutdown
                pass
            self.h = None

    __del__ = close

    @property
    def nshards(self):
        return len(self.devices)

    def shard_range(self, B, shard):
        lo, hi = C.c_size_t(), C.c_size_t()
        self._ck(_lib.lib().mkt_multi_shard_range(self.h, B, shard, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def shard(self, i):
        """borrowed Scheme view of shard i's context (timing, kernel names); valid while this object lives"""
        s = object.__new__(Scheme)
        s.params, s.device, s.arith, s._user_stream = self.params, self.devices[i], self.arith, True
        s.h = C.c_void_p(_lib.lib().mkt_multi_ctx(self.h, i))
        s._owned = False
        return s

    # -- keys: once, on the first device; replicate() copies them to the others (load_party, load_crs: _Batched)
    def keygen_device(self, party, keys: "PartyKeys"):
        crs_p = _np_ptr(keys._crs) if (self.params.scheme == CCS and keys._crs is not None) else None
        self._ck(_lib.lib().mkt_multi_keygen_device(self.h, party, keys.h, crs_p))
        self.load_party(party, rlk_d=keys.rlk_d, rlk_f=keys.rlk_f, pubkey=keys.pubkey)

    def replicate(self):
        self._ck(_lib.lib().mkt_multi_replicate(self.h))
        self._sealed = True

    def set_option(self, name, value):
        self._ck(_lib.lib().mkt_multi_set_option(self.h, name.encode(), int(value)))


def _install(sch, party, keys):
    """one party's keys into a Scheme or MultiScheme; keys made with secrets_only=True get their large keys generated on the device"""
    (sch.keygen_device if keys.secrets_only else sch.load_party)(party, keys)


def setup_multi(params: Params, devices, keys=None, a=None, arith=ARITH_F64REF, private_keys=False, stage_always=False, no_peer=False):
    """setup (scheme.jl:151 / :190 / :244 / :292 / :343) for a MultiScheme: evaluation keys uploaded (or, for keys made with
    secrets_only=True, generated) once on devices[0], pre-transformed there and replicated to the other devices"""
    sch = MultiScheme(params, devices, arith=arith, private_keys=private_keys, stage_always=stage_always, no_peer=no_peer)
    if params.multikey:
        sch.load_crs(a)
        klist = list(keys)
    else:
        klist = [keys if isinstance(keys, PartyKeys) else keys[0]]
    for i, kk in enumerate(klist):
        _install(sch, i, kk)
    sch.replicate()
    return sch


def setup(params: Params, keys=None, a=None, device=0, deterministic_seed=None, arith=ARITH_F64REF):
    """scheme.jl:151 / :190 setup(params) -> (keys, scheme) for the single-key schemes, and
    scheme.jl:244 / :292 / :343 setup(a, btk, params) -> scheme for the multi-key ones
    (keys = list of PartyKeys, a = CRS).  The evaluation keys are uploaded and pre-transformed
    on `device`."""
    if not params.multikey:
        ks = keys if keys is not None else PartyKeys(params, party=0, deterministic_seed=deterministic_seed)
        sch = Scheme(params, device=device, arith=arith)
        _install(sch, 0, ks)
        return ks, sch
    sch = Scheme(params, device=device, arith=arith)
    sch.load_crs(a)
    for i, kk in enumerate(keys):
        _install(sch, i, kk)
    return sch


def bootstrapping_(ctxt, scheme: Scheme):
    """bootstrapping.jl:4 bootstrapping!(ctxt, scheme): in place on the batch"""
    return scheme.bootstrapping_(ctxt)


def blindrotate_(atilde, acc, scheme: Scheme):
    """bootstrapping.jl:32/:114/:234/:369 blindrotate!(atilde, acc, scheme)"""
    return scheme.blindrotate_(atilde, acc)


def keyswitch(acc, scheme: Scheme):
    """bootstrapping.jl:81/:170/:333/:564/:664 keyswitch!(res, acc, scheme) -> res"""
    return scheme.keyswitch(acc)


def NAND(c1, c2, scheme: Scheme, out=None):
    """gate.jl:1-8"""
    return scheme.gate(0, c1, c2, out)


def AND(c1, c2, scheme: Scheme, out=None):
    """gate.jl:10-17"""
    return scheme.gate(1, c1, c2, out)


def OR(c1, c2, scheme: Scheme, out=None):
    """gate.jl:19-26"""
    return scheme.gate(2, c1, c2, out)


def XOR(c1, c2, scheme: Scheme, out=None):
    """gate.jl:28-35"""
    return scheme.gate(3, c1, c2, out)


def XNOR(c1, c2, scheme: Scheme, out=None):
    """gate.jl:37-44"""
    return scheme.gate(4, c1, c2, out)


def MUX(s, c1, c2, scheme: Scheme, out=None):
    """s ? c1 : c2 -- not a reference operator (gate.jl has none; the north star names it): two blind rotations and one key
    switch, blindrotate!(AND-linear(s, c1)) + blindrotate!(AND-linear(NOT s, c2)) + 1/8, then keyswitch! (mkt_mux_batch)"""
    return scheme.mux(s, c1, c2, out)


def MUX_composite(s, c1, c2, scheme: Scheme):
    """the same function as the composite OR(AND(s, c1), AND(NOT s, c2)) of the reference's gates (three bootstraps), the two
    ANDs evaluated as one batch"""
    ns = s.clone() if hasattr(s, "clone") else np.array(s, copy=True)
    NOT_(ns, scheme)
    if hasattr(s, "clone"):
        import torch
        both = scheme.gate(1, torch.cat([s, ns]), torch.cat([c1, c2]))
    else:
        both = scheme.gate(1, np.concatenate([np.atleast_2d(s), np.atleast_2d(ns)]), np.concatenate([np.atleast_2d(c1), np.atleast_2d(c2)]))
    h = both.shape[0] // 2
    return scheme.gate(2, both[:h], both[h:])      # 1 = AND, 2 = OR (params.py)


def MAJ3(c1, c2, c3, scheme: Scheme, out=None):
    """majority of three in ONE bootstrap (linear part c1 + c2 + c3; not a reference operator: mktfhe.h MKT_MAJ3)"""
    return scheme.gate3(0, c1, c2, c3, out)


def XOR3(c1, c2, c3, scheme: Scheme, out=None):
    """c1 ^ c2 ^ c3 in ONE bootstrap (linear part -2(c1 + c2 + c3); mktfhe.h MKT_XOR3)"""
    return scheme.gate3(2, c1, c2, c3, out)


def full_adder(a, b, c, scheme: Scheme):
    """-> (sum, carry) = (XOR3(a, b, c), MAJ3(a, b, c)): ONE gate3_ops call over 2B gates, two bootstraps per adder (the composite of
    the reference's gates takes five: XOR, XOR, AND, AND, OR)"""
    on_gpu = _is_torch(a)
    if on_gpu:
        import torch
        cat = lambda u: torch.cat([u.reshape(-1, u.shape[-1])] * 2)      # noqa: E731
    else:
        cat = lambda u: np.concatenate([np.reshape(np.asarray(u, dtype=np.uint32), (-1, u.shape[-1]))] * 2)   # noqa: E731
    x, y, z = cat(a), cat(b), cat(c)
    B = x.shape[0] // 2
    ops = np.repeat(np.array([2, 0], dtype=np.uint8), B)                # XOR3_OP for the sums, MAJ3_OP for the carries
    out = scheme.gate3_ops(torch.from_numpy(ops).to(a.device) if on_gpu else ops, x, y, z)
    shape = tuple(a.shape)
    return out[:B].reshape(shape), out[B:].reshape(shape)


def NOR(c1, c2, scheme: Scheme, out=None):
    """gate.jl:46-53"""
    return scheme.gate(5, c1, c2, out)


def NOT_(ctxt, scheme: Scheme):
    """gate.jl:55-58 NOT!(ctxt): negation, no bootstrap"""
    return scheme.not_(ctxt)
