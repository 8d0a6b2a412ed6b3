"""Every rotation kernel at every ring size the library admits (tests/size_ladder.py), word for word against the oracle / tests/ref_exact.py.

One context per ladder row; its option settings are walked with set_option.  Under each setting: blindrotate_ from the crafted rows of
helpers.rot_inputs (the single-exponent rows 1, N - 1, N, N + 1, 2N - 1, 2N at the first and last mask position and at the block and party
borders, then one dense batch, accumulators on the gadgets' digit boundaries with a non-zero acc.a), EVERY ciphertext compared, the kernel
reached asserted; then one NAND batch against the reference's gate (mod switch, test vector, rotation, key switch, linear part at that ring
size), decryption asserted (but for size_ladder.words_only sets, which the oracle itself decrypts wrongly).  KMS / KMS_block: also the phase-1 rows, so that a mismatch points at phase 1 or phase 2.  Tolerance zero.

The references of a row are computed once and shared by its settings.  tests/test_size_ladder_cpu.py proves without a GPU that every entry
reaches the instantiation it names and that no rotation instantiation of the library is without an entry.

The last part is the admitted envelope (size_ladder.ENVELOPE): at each corner of validate_params the engine equals the reference on the same
checks, or refuses with MKT_ERR_UNSUPPORTED / MKT_ERR_ARG and a message that names the limit.  MKT_ERR_HIP is not a refusal."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ref_exact as RX
import size_ladder as SL
from helpers import GATE_FUNCS, bits_equal, encrypt_bits, gpu_scheme, keygen, mk, oracle_scheme, rot_inputs
from mktfhe_amd._lib import MktError

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED, ERR_HIP = -1, -2, -4          # include/mktfhe.h


def _ids(rows):
    return [SL.sid(r[0]) for r in rows]


def ref_rotate(p, keys, crs, at, acc):
    """tests/ref_exact.py: the rotation with every product exact mod 2^W"""
    if p.scheme in (mk.KMS, mk.KMS_BLOCK):
        return RX.kms_blindrotate(p, keys, crs, at, acc)
    if p.scheme == mk.CCS:
        return RX.ccs_blindrotate(p, keys, crs, at, acc)
    return (RX.blindrotate_lmss if p.scheme == mk.LMSS else RX.blindrotate)(p, keys[0].brk, at, acc)


class Reference:
    """keys, the crafted rotation inputs with the reference's answer to each, and one NAND batch with its answer, for one parameter set"""

    def __init__(self, p, seed, exact):
        self.p, self.exact = p, exact
        self.crs, self.keys = keygen(p, seed)
        self.so = so = oracle_scheme(p, self.crs, self.keys)
        # EXACT: the restatement's products are the oracle's C schoolbook, pure functions that release the interpreter: the rows of a batch on threads
        rot = (lambda a: np.asarray(ref_rotate(p, self.keys, self.crs, a[0], a[1])).reshape(-1)) if exact else (lambda a: so.blindrotate(a[0], a[1]).reshape(-1))
        self.bits = np.random.default_rng(seed + 2).integers(0, 2, 2 * SL.B).astype(bool)
        c = encrypt_bits(p, self.keys, self.bits, seed=900 + seed)
        self.x, self.y = c[:SL.B], c[SL.B:]
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1) if exact else 1) as pool:
            self.rot = [(at, acc, np.stack(list(pool.map(rot, zip(at, acc))))) for at, acc in rot_inputs(p, SL.B, seed + 1)]
            if exact:
                lin = [so.modswitch(gate_linear(0, self.x[j], self.y[j])) for j in range(SL.B)]
                accs = pool.map(rot, [(at, so.testvector(bt)) for at, bt in lin])
                self.gate = np.stack([so.keyswitch(acc.reshape(1 + p.k, p.N)) for acc in accs])
            else:
                self.gate = np.stack([so.gate(0, self.x[j], self.y[j]) for j in range(SL.B)])
        self.want = GATE_FUNCS[0](self.bits[:SL.B], self.bits[SL.B:])

    def decrypt(self, out):
        return mk.lwe_decrypt(out, self.keys if self.p.multikey else self.keys[0], self.p)

    def phase1(self, j, at):
        """the oracle's phase-1 rows of ciphertext j (Float64 mode): [rtot][2][M]"""
        p = self.p
        return np.concatenate([self.so.kms_phase1(i, at[j, i * p.n:(i + 1) * p.n]) for i in range(p.k)])


def gate_linear(op, x, y):
    from helpers import O
    return O.gate_linear(op, x, y)


def walk_checks(ref, sg, walk):
    """the rotation and gate checks under every option setting of `walk` -> (option setting, phase-1 rows or None) per setting.  A HIP runtime
    error ends the session: nothing more is started on a device that may have faulted"""
    try:
        return _walk_checks(ref, sg, walk)
    except MktError as e:
        if e.code == ERR_HIP:
            pytest.exit(f"HIP runtime error in {SL.sid(ref.p)}: {e}", returncode=3)
        raise


def _walk_checks(ref, sg, walk):
    p, seen = ref.p, []
    for opts, kernel in walk:
        for k, v in {**SL.DEFAULTS, **opts}.items():
            if ref.exact or not k.startswith("exact_"):
                sg.set_option(k, v)
        for at, acc, want in ref.rot:
            got = sg.blindrotate_(at, acc.astype(p.ring_dtype).copy()).astype(np.uint64).reshape(len(at), -1)
            assert sg.last_kernel_name() == kernel, (opts, sg.last_kernel_name())
            for j in range(len(at)):
                assert np.array_equal(got[j], want[j]), (opts, kernel, j, at[j].nonzero()[0], at[j][at[j] != 0][:1])
        lev = None
        if p.scheme in (mk.KMS, mk.KMS_BLOCK):
            at = ref.rot[-1][0]                                                   # the dense batch
            lev = sg.kms_phase1(at)
            if not ref.exact:
                for j in range(len(at)):
                    assert bits_equal(lev[j], ref.phase1(j, at)), (opts, "phase 1", j)
        seen.append((opts, lev))
        out = sg.gate(0, ref.x, ref.y)
        assert sg.last_kernel_name() == kernel, (opts, sg.last_kernel_name())
        assert np.array_equal(out, ref.gate), (opts, kernel, "NAND", np.nonzero((out != ref.gate).any(axis=1))[0])
        assert SL.words_only(p) or np.array_equal(ref.decrypt(out), ref.want), (opts, "decrypt")
    # EXACT KMS: the phase-1 rows are residue tables without a host reference -- the implementations agree with one another on them
    # wherever they write the same form (the integer kernels), and all of them with tests/ref_exact.py on the rotation above
    if ref.exact:
        tables = [lev for opts, lev in seen if lev is not None and opts.get("exact_impl") == 0]
        for lev in tables[1:]:
            assert bits_equal(lev, tables[0]), "EXACT phase 1: two integer kernels differ"
    return seen


@pytest.mark.parametrize("p,walk", SL.LADDER, ids=_ids(SL.LADDER))
def test_ladder(require_gpu, p, walk):
    ref = Reference(p, 41, exact=False)
    sg = gpu_scheme(p, ref.crs, ref.keys)
    walk_checks(ref, sg, walk)
    sg.close()


@pytest.mark.parametrize("p,walk", SL.EXACT_LADDER, ids=_ids(SL.EXACT_LADDER))
def test_exact_ladder(require_gpu, p, walk):
    ref = Reference(p, 43, exact=True)
    sx = gpu_scheme(p, ref.crs, ref.keys, arith=mk.ARITH_EXACT)
    walk_checks(ref, sx, walk)
    sx.close()


@pytest.mark.parametrize("p,words", SL.EXACT_REFUSED, ids=_ids(SL.EXACT_REFUSED))
def test_exact_ladder_refuses_a_gadget_beyond_the_modulus(require_gpu, p, words):
    crs, keys = keygen(p, 45)
    with pytest.raises(MktError) as e:
        gpu_scheme(p, crs, keys, arith=mk.ARITH_EXACT)
    assert e.value.code == ERR_UNSUPPORTED and words in str(e.value), str(e.value)


# ---------------------------------------------------------------- the admitted envelope: served word for word, or refused cleanly
def _refusal(e):
    assert e.code in (ERR_ARG, ERR_UNSUPPORTED), ("not a refusal", str(e))
    assert any(w in str(e) for w in SL.LIMIT_WORDS), ("the message does not name the limit", str(e))
    return f"refused ({e.code}, {str(e).split(': ', 1)[-1]!r})"


@pytest.mark.parametrize("p,exact,what", SL.ENVELOPE, ids=[f"{w}-N{p.N}-{'exact' if x else 'f64'}" for p, x, w in SL.ENVELOPE])
def test_envelope_corner_is_served_or_refused(require_gpu, p, exact, what):
    crs, keys = keygen(p, 47)
    try:
        sg = gpu_scheme(p, crs, keys, arith=mk.ARITH_EXACT if exact else mk.ARITH_F64REF)
    except MktError as e:
        print(f"ENVELOPE {what} N={p.N} {'EXACT' if exact else 'F64REF'}: {_refusal(e)} at mkt_ctx_create / the key load")
        return
    so = oracle_scheme(p, crs, keys)
    at, acc = list(rot_inputs(p, SL.B, 48))[-1]
    buf = acc.astype(p.ring_dtype)
    fill = buf.copy()                                                               # (the accumulators are rotated in place: input and output buffer)
    try:
        got = sg.blindrotate_(at, buf).astype(np.uint64).reshape(len(at), -1)
    except MktError as e:
        outcome = _refusal(e)
        assert np.array_equal(buf, fill), "a refused call wrote its output buffer"
        ok = sg.modswitch(np.zeros((1, p.lwe_len), dtype=np.uint32))                # the context still serves a supported call
        assert ok[0].shape == (1, p.lwe_len - 1)
        print(f"ENVELOPE {what} N={p.N} {'EXACT' if exact else 'F64REF'}: {outcome} at the call")
        sg.close()
        return
    for j in range(len(at)):
        want = np.asarray(ref_rotate(p, keys, crs, at[j], acc[j])).reshape(-1) if exact else so.blindrotate(at[j], acc[j]).reshape(-1)
        assert np.array_equal(got[j], want), (what, "rotation", j)
    bits = np.random.default_rng(49).integers(0, 2, 2 * SL.B).astype(bool)
    c = encrypt_bits(p, keys, bits, seed=950)
    x, y = c[:SL.B], c[SL.B:]
    out = sg.gate(0, x, y)
    for j in range(SL.B):
        if exact:
            a, b = so.modswitch(gate_linear(0, x[j], y[j]))
            want = so.keyswitch(np.asarray(ref_rotate(p, keys, crs, a, so.testvector(b))).reshape(1 + p.k, p.N))
        else:
            want = so.gate(0, x[j], y[j])
        assert np.array_equal(out[j], want), (what, "NAND", j)
    dec = np.array_equal(mk.lwe_decrypt(out, keys if p.multikey else keys[0], p), GATE_FUNCS[0](bits[:SL.B], bits[SL.B:]))
    assert dec or what in SL.ENVELOPE_WORDS_ONLY, (what, "decrypt")
    print(f"ENVELOPE {what} N={p.N} {'EXACT' if exact else 'F64REF'}: served ({sg.last_kernel_name()}; decrypts: {dec})")
    sg.close()
