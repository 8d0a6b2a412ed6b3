"""mkt_keygen_device_seeded without a GPU: the header declares it and the library exports it; the Python wrapper checks its seed before the
library is called; the party view it returns serialises like a host-generated seeded party."""
import os
import re

import numpy as np
import pytest

from helpers import ROOT, mk
from mktfhe_amd import _lib


def test_header_ctypes_library_and_package_hold_the_new_name():
    hdr = open(os.path.join(ROOT, "include", "mktfhe.h")).read()
    name = "mkt_keygen_device_seeded"
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/mktfhe.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 8 and args[0].startswith("mkt_ctx *") and args[-1] == "int install" and not any(a == "int mem" for a in args)
    assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == len(args)
    assert hasattr(_lib.lib(), name), f"{name} is not exported by the library"
    assert _lib.lib().mkt_abi_version() == 3
    assert mk.keygen_device_seeded is mk.seeded_keys.keygen_device_seeded
    assert not hasattr(mk.Scheme, "keygen_device_seeded") and not hasattr(mk.MultiScheme, "keygen_device_seeded")
    used = set(re.findall(r"\b(mkt_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "examples", "seeded_keygen_gpu.c")).read()))
    assert {name, "mkt_client_party_secrets", "mkt_load_seeded_keys"} <= used <= set(_lib.SYMBOLS), used - set(_lib.SYMBOLS)


class _NoLibrary:
    """stands where a Scheme would: reaching for its context means the library was about to be called"""
    params = mk.CGGIparam.scaled(n=3, N=32)

    @property
    def h(self):
        raise AssertionError("the library was reached")


@pytest.mark.parametrize("bad", [bytes(31), bytes(33), "x" * 32, list(range(32))], ids=["31", "33", "str", "list"])
def test_a_mask_seed_that_is_not_32_bytes_is_a_value_error_before_the_library(bad):
    p = _NoLibrary.params
    keys = mk.party_keygen(None, p, secrets_only=True, deterministic_seed=1)
    with pytest.raises(ValueError):
        mk.keygen_device_seeded(_NoLibrary(), 0, keys, mask_seed=bad)


@pytest.mark.parametrize("p", [mk.CGGIparam.scaled(n=3, N=32), mk.KMS2party.scaled(n=3, N=32)], ids=lambda p: p.name)
def test_the_party_view_serialises_as_a_version_2_blob(p):
    """the view keygen_device_seeded returns, built by hand around a host-generated seeded party: dump_party writes a version-2 blob that
    load (and with it _check_seeded) accepts, with the sections of the host party; the view forwards what it does not hold"""
    ms = bytes(range(1, 33))
    crs = mk.CRS(p, 4) if p.multikey else None
    host = mk.party_keygen_seeded(crs, p, party=p.nparty - 1, mask_seed=ms, deterministic_seed=4)
    secr = mk.party_keygen(crs, p, party=p.nparty - 1, secrets_only=True, deterministic_seed=4)
    view = mk.seeded_keys.SeededDeviceKeys(secr, ms, np.array(host.brk_seeded), np.array(host.ksk_seeded))
    assert view.seeded is True and view.mask_seed == ms and view.brk is None and view.ksk is None and not view.secrets_only
    assert view.params is p and view.party == p.nparty - 1 and np.array_equal(view.lwekey, host.lwekey) and np.array_equal(view.ringkey(0), host.ringkey(0))
    for name in ("rlk_d", "rlk_f", "pubkey"):
        a, b = getattr(view, name), getattr(host, name)
        assert (a is None and b is None) or np.array_equal(a, b), name
    blob = mk.keyblob.dump_party(view)
    assert blob[:8] == mk.keyblob.MAGIC2 and blob == mk.keyblob.dump_party(host)
    pd, party, secs = mk.keyblob.load(blob)
    mk.keyblob._check_seeded(pd, secs)
    assert party == p.nparty - 1 and secs["mask_seed"].astype("<u4").tobytes() == ms
    assert np.array_equal(secs["brk_seeded"], host.brk_seeded) and np.array_equal(secs["ksk_seeded"], host.ksk_seeded)
