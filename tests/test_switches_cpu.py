"""The switch table stays tested: every switch that INTEGRATION.md documents and every option mkt_set_option accepts is in
tests/test_gpu_switches.py's SWITCHES, and every entry there is exercised by a parametrised case of that module."""
import os
import re

import test_gpu_switches as S
from helpers import ROOT


def _table_switches():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## Runtime switches"):]
    sec = sec[:sec.index("\n## ", 1)]
    names = set()
    for line in sec.splitlines():
        if line.startswith("| `MKT_"):
            names |= set(re.findall(r"`(MKT_[A-Z0-9_]+)`", line.split("|")[1]))
    return names


def _set_option_names():
    text = open(os.path.join(ROOT, "mktfhe_amd", "csrc", "context.cpp")).read()
    body = text[text.index("const Switch SWITCHES[] = {"):]      # the one table mkt_set_option and the environment seeding loop over
    body = body[:body.index("\n};\n")]
    return set(re.findall(r'^\s*\{"([a-z0-9_]+)", (?:"MKT_[A-Z0-9_]+"|nullptr), &Tune::\1,', body, re.M))


def _strings(v):
    if isinstance(v, str):
        yield v
    elif isinstance(v, dict):
        for k, x in v.items():
            yield from _strings(k)
            yield from _strings(x)
    elif isinstance(v, (list, tuple, set)):
        for x in v:
            yield from _strings(x)


def _parametrised_strings():
    found = set()
    for name in dir(S):
        fn = getattr(S, name)
        if not (name.startswith("test_") and callable(fn)):
            continue
        for mark in getattr(fn, "pytestmark", []):
            if mark.name == "parametrize":
                found |= set(_strings(list(mark.args[1:]) + list(mark.kwargs.values())))
    return found


def test_table_and_set_option_parse():
    table, opts = _table_switches(), _set_option_names()
    assert {"MKT_KS_G", "MKT_FFT_NB", "MKT_NTT_GRID", "MKT_ROT_VARIANT"} <= table and len(table) >= 15, table
    assert opts == set("rot_variant rot_stagger rot_split rot_wide rot_blkg ccs_stagger ccs_pipe exact_wide exact_impl rot_map fx_polymul_force "
                       "exact_kany".split()), opts


def test_every_documented_switch_is_listed():
    missing = (_table_switches() | _set_option_names()) - set(S.SWITCHES)
    assert not missing, f"switches without a test in tests/test_gpu_switches.py: {sorted(missing)}"


def test_every_listed_switch_has_a_parametrised_case():
    assert len(S.SWITCHES) == len(set(S.SWITCHES))
    unexercised = set(S.SWITCHES) - _parametrised_strings()
    assert not unexercised, f"SWITCHES entries no parametrised case sets: {sorted(unexercised)}"
