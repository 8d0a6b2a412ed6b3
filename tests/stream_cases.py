"""The case lists of tests/test_gpu_stream_order.py: which calls are made behind a late producer (helpers.LateProducer), in which memory kind,
on a stream chosen in which way, and the rule that sizes the delay.  tests/test_stream_order_cpu.py imports the same lists and holds them to
context_life_cases.STEPS -- which tests/test_context_life_cpu.py holds to include/mktfhe.h -- so that a new entry point cannot join the header
without joining the stream test.

Every other GPU test pins the WORDS of a call; these cases pin WHEN its steps run: each kernel, memset and staging copy of a call on the
stream the context is on, and calls on one context in the order they were made."""
import numpy as np

import context_life_cases as K
from helpers import O, mk, ora_params

B = 33                                          # rows of every call: more than one workgroup of the row kernels, no multiple of a tile
SETS = list(K.SETS)

# ---- a: every entry point.  (memory kind, how the stream is chosen): "pinned" = set_stream(S.cuda_stream), S a fresh non-blocking stream;
#      "torch" = no stream pinned, the call made under `with torch.cuda.stream(S)` ----
PINNED, TORCH = "pinned", "torch"
VARIANTS = [(mk.MEM_DEVICE, PINNED), (mk.MEM_DEVICE, TORCH), (mk.MEM_HOST, PINNED), (mk.MEM_HOST, TORCH)]


def variant_id(v):
    return ("device" if v[0] == mk.MEM_DEVICE else "host") + "-" + v[1]


def cases(name):
    """-> [(step, memory kind, how)] of set `name`: every step that applies to it, in every variant"""
    return [(st, mem, how) for st in K.steps_of(name) for mem, how in VARIANTS]


# the control, once per parametrised test: the context on another stream than the one the inputs arrive on must NOT give the reference's words
CONTROL_STEPS = ("gate_ops", "transform_fwd")

# ---- b: forks ----
FORK_STEPS = ("gate", "lut_bootstrap", "keyswitch")          # one gate, one table bootstrap, one key switch
# ---- d: key loads behind a batch ----
KEY_SETS = ("cggi", "kms", "ccs", "x-kms")
KEY_SEEDS = (1, 2)                                           # the resident keys, the keys one piece is loaded from again
# ---- e: order across streams: how the context gets from the stream of call A to that of call B ----
ORDER_WAYS = ("torch", "set_stream", "null", "fork")
# ---- f: sharded calls ----
SHARD_SET, SHARD_DEVICES, SHARD_STEPS = "cggi", [0, 0, 0], ("gate_ops", "lut_bootstrap")


# ---- the delay ----
DELAY_FACTOR, DELAY_FLOOR_MS, DELAY_CAP_MS = 20.0, 20.0, 250.0


def delay_ms(host_ms):
    """the delay behind which the inputs of a set arrive: 20 times the longest host wall time of one undelayed device-memory call of its
    steps (so the whole call is enqueued while the spin has run a twentieth), at least 20 ms, at most 250 ms.  Whether it is LONG ENOUGH
    is not judged by its value: the control of every test fails if it is not"""
    return min(DELAY_CAP_MS, max(DELAY_FLOOR_MS, DELAY_FACTOR * max(host_ms)))


def delay_cycles(ms, cycles_per_ms):
    return int(np.ceil(ms * cycles_per_ms))


# ---- poison ----
def poison(a):
    """the words a late tensor holds until its real words arrive: all zero"""
    return np.zeros_like(a)


class _HostScheme:
    """what make_inputs asks of a context, from the CPU references the suite holds the device to elsewhere: the mod switch of the oracle,
    the oracle's Float64 transform, the integer transform of tests/ref_ntt.py"""

    def __init__(self, name):
        self.p, self.arith = K.set_of(name)

    def modswitch(self, rows):
        so = O.Scheme(ora_params(self.p))
        got = [so.modswitch(r) for r in rows]
        return np.stack([a for a, _ in got]), np.array([b for _, b in got], dtype=np.uint32)

    def transform_fwd(self, polys):
        if self.arith == mk.ARITH_EXACT:
            import ref_ntt
            return np.stack([np.array(ref_ntt.fwd(r, self.p.W), dtype=np.uint64) for r in polys]).view(np.complex128)
        return O.Ffter(self.p.N, self.p.W).fwd(polys.astype(np.uint64))

    def close(self):
        pass


def host_inputs(name, nrows=B):
    """context_life_cases.make_inputs without a GPU: the same seeds and the same host-side words; the three fields a context computes
    there (at, bt, tr -- and acc0, made from bt) from _HostScheme"""
    keep = K.new_scheme
    K.new_scheme = lambda n, seed=1: _HostScheme(n)
    try:
        return K.make_inputs(name, nrows)
    finally:
        K.new_scheme = keep
