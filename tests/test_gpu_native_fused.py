"""native() with its exact steps fused (fft_device.h: one FMA for the reduction, one for the low half, one truncating convert) on the
GPU: transform_inv at N = 64 on both rings, on transform-domain inputs crafted so that the values native() receives hit every class --
tiny negatives that round up to 2^W, exact multiples of 2^W, values >= 2^W, fractions below 2^52 -- against the numpy restatement of
ifftto! + native (tests/ref_numpy.py, arithmetic.jl:1-9 literally), tolerance 0.

A transform whose M points all equal (c, d) is the transform of c - d X^M up to the exact scaling by M: the inverse network adds equals
and multiplies zeros, so native() receives exactly c at coefficient 0, -d at coefficient M and a zero of either sign everywhere else.
The test does not rely on that: it records what the restatement hands to its native() and asserts the classes on those values."""
import numpy as np
import pytest

import ref_numpy as RN
from helpers import O, mk

pytestmark = pytest.mark.gpu

N = 64


def _fft(W):
    """ref_numpy.FFT at N = 64: the golden table file has no entry for this size, the oracle's generator (the one
    tests/test_oracle_cpu.py compares with that file at the other sizes) supplies the tables"""
    f = RN.FFT.__new__(RN.FFT)
    f.N, f.M, f.W = N, N // 2, W
    o = O.Ffter(N, W)
    tabs = [o.table(w) for w in range(4)]
    f.psi, f.psiinv, f.roots, f.rootsinv = (RN.C(t.real.copy(), t.imag.copy()) for t in tabs)
    f.udt, f.sdt = (np.uint64, np.int64) if W == 64 else (np.uint32, np.int32)
    return f


def _inputs(W):
    two = 2.0 ** W
    vals = []
    vals += [-1e-30, -2.0 ** -40, -2.0 ** -70, np.nextafter(0.0, -1.0) * 2.0 ** 60, -1e-5 * 2.0 ** -20]                  # tiny negatives: x + 2^W rounds to 2^W
    vals += [k * two for k in (0.0, 1.0, -1.0, 2.0, 3.0, -7.0, 1024.0, -1000.0, 2.0 ** 20)] + [-0.0]                      # exact multiples of 2^W
    vals += [two + 5.5, 3 * two + 0.75 * 2.0 ** (W - 40), 2.0 ** (W + 6) + 2.0 ** (W - 20), np.nextafter(two, np.inf),
             2.0 ** 100, 5 * two - 2.0 ** (W - 30), -(two + 1.0) * 3, 2.0 ** (W + 20) + 2.0 ** (W - 31)]                   # values >= 2^W (and below -2^W)
    vals += [12345.678, 0.999999, 2.0 ** 52 - 0.5, 2.0 ** 32 - 0.25, 2.0 ** 32 + 0.5, 2.0 ** 31 + 0.5, 4294967295.7,
             -0.3, -1023.9999, -4294967295.7, 2.0 ** 51 + 0.25, 1.5]                                                         # fractions below 2^52
    vals += [np.nextafter(two, 0.0), two / 2, np.nextafter(two / 2, 0.0), two - 2.0 ** (W - 52), 2.0 ** 32, 2.0 ** 32 - 1.0, 2.0 ** 33 - 1.0]
    vals = np.array(vals)
    M = N // 2
    rows = []
    for i, c in enumerate(vals):                                     # constant transforms: (c, d) with d the next value of the list
        rows.append(np.full(M, complex(c, vals[(i + 1) % len(vals)])))
    rng = np.random.default_rng(W)
    for e in (10, 30, W - 6, W + 4, W + 30):                          # dense transforms at growing magnitudes: every coefficient a fraction / >= 2^W
        rows.append((rng.standard_normal(M) + 1j * rng.standard_normal(M)) * 2.0 ** e)
    return np.stack(rows)


@pytest.mark.parametrize("W", [32, 64])
def test_transform_inv_native_classes(require_gpu, W):
    f = _fft(W)
    t = _inputs(W)
    seen = []
    native = f.native
    f.native = lambda x: (seen.append(x.copy()), native(x))[1]
    ref = np.stack([f.inv(RN.C(r.real.copy(), r.imag.copy())) for r in t]).astype(np.uint64)
    x = np.concatenate(seen)
    two = 2.0 ** W
    red = x - np.floor(x * 2.0 ** -W) * two
    classes = {"tiny negative rounding up to 2^W": (x < 0) & (red == two),
               "exact multiple of 2^W": (x != 0) & (np.abs(x) >= two) & (red == 0),
               "zero of either sign": (x == 0) & np.signbit(x), "+0": (x == 0) & ~np.signbit(x),
               "value >= 2^W": (x >= two) & (red != 0), "value <= -2^W": (x <= -two),
               "fraction below 2^52": (np.abs(x) < 2.0 ** 52) & (x != np.trunc(x)),
               "low half with a fraction": (red != np.trunc(red)) & (red > 2.0 ** 32) if W == 64 else (red != np.trunc(red))}
    for name, m in classes.items():
        assert m.any(), name
    s = mk.Scheme(mk.CGGIparam.scaled(n=8, N=N, W=W))
    got = s.transform_inv(t).astype(np.uint64)
    s.close()
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (len(bad), bad[:4], [(hex(int(got[tuple(b)])), hex(int(ref[tuple(b)]))) for b in bad[:4]])
