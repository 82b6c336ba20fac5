"""DESIGN.md §9b lists exactly the run-time switches the sources read.

A switch is an `MSFNO_*` name passed to one of the readers of csrc/switches.h (GETENV;
the header holds the only getenv() of csrc/) or read from os.environ in msfno_amd/.  Status codes
(`MSFNO_OK`, ...) and bench.py's `MSFNO_BENCH_*` names are not switches: neither is read from the environment by the library."""
import glob
import os
import re

from conftest import PKG_DIR, REPO

NAME = r"MSFNO_[A-Z0-9_]+"
# the readers of csrc/switches.h: each hands its first argument to the one getenv()
GETENV = ("sw_raw", "sw_set", "sw_char", "sw_on", "sw_is1", "sw_is1_or", "sw_eq", "sw_int")
SWITCHES_H = "switches.h"


def _read(path):
    with open(path, encoding="utf-8") as fh:
        return fh.read()


def _csrc_files():
    return [f for f in glob.glob(os.path.join(PKG_DIR, "csrc", "*"))
            if os.path.isfile(f) and f.endswith((".hip", ".cpp", ".h"))]


def source_switches():
    names = set()
    for f in _csrc_files():
        names |= set(re.findall(r'\b(?:%s)\(\s*"(%s)"' % ("|".join(GETENV), NAME), _read(f)))
    for f in glob.glob(os.path.join(PKG_DIR, "msfno_amd", "**", "*.py"), recursive=True):
        names |= set(re.findall(r'os\.environ(?:\.get\(|\[)\s*"(%s)"' % NAME, _read(f)))
    return {n for n in names if not n.startswith("MSFNO_BENCH_")}


def table_switches():
    text = _read(os.path.join(REPO, "DESIGN.md"))
    start = text.index("\n## 9b. ")
    sec = text[start:text.index("\n## ", start + 1)]
    names = set()
    for line in sec.splitlines():
        if line.startswith("| `MSFNO_"):
            names |= set(re.findall(NAME, line.split("|")[1]))
    return names


def test_only_the_switch_header_calls_getenv():
    assert "getenv(" in _read(os.path.join(PKG_DIR, "csrc", SWITCHES_H))
    others = [os.path.basename(f) for f in _csrc_files()
              if os.path.basename(f) != SWITCHES_H and "getenv(" in _read(f)]
    assert not others, f"getenv( outside csrc/{SWITCHES_H}: {others}"


def test_sources_read_switches_at_all():
    assert len(source_switches()) > 20  # the patterns above still match the code's idiom


def test_design_9b_table_equals_the_switches_the_sources_read():
    src, tab = source_switches(), table_switches()
    assert src == tab, (f"read by the sources but not in DESIGN §9b: {sorted(src - tab)}; "
                        f"in DESIGN §9b but read nowhere: {sorted(tab - src)}")
