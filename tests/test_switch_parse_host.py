"""csrc/switches.h on the host: each reader follows the rule its comment states.

A tiny main is compiled against the header alone with the system C++17 compiler (the
header includes no HIP) and run once per value of one variable: unset, then each of
VALUES.  The expected answers below are the header comment's rules written in Python,
not the program's output."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG_DIR

HEADER_DIR = os.path.join(PKG_DIR, "csrc")
VAR = "MSFNO_PARSE_PROBE"
VALUES = [None, "", "0", "1", "00", "10", "x6", "x6 ", "4x128", "-3"]

MAIN = r"""
#include <cstdio>
#include "switches.h"
using namespace msfno;
int main() {
  const char* n = "%s";
  const char* raw = sw_raw(n);
  std::printf("raw=%%s|set=%%d|char=%%d|on=%%d|is1=%%d|is1_or_t=%%d|is1_or_f=%%d|eq_x6=%%d|"
              "int7=%%d\n",
              raw ? raw : "(null)", (int)sw_set(n), (int)sw_char(n), (int)sw_on(n), (int)sw_is1(n),
              (int)sw_is1_or(n, true), (int)sw_is1_or(n, false), (int)sw_eq(n, "x6"),
              sw_int(n, 7));
  return 0;
}
""" % VAR


def _atoi(v):
    m = re.match(r"[ \t\n\v\f\r]*([+-]?\d+)", v)
    return int(m.group(1)) if m else 0


def expected(v):
    """The rules of the header comment for the variable unset (None) / set to v."""
    first = 0 if not v else ord(v[0])
    is1 = first == ord("1")
    return {
        "raw": "(null)" if v is None else v,
        "set": int(v is not None),
        "char": first,
        "on": int(first != ord("0")),
        "is1": int(is1),
        "is1_or_t": int(True if v is None else is1),
        "is1_or_f": int(False if v is None else is1),
        "eq_x6": int(v == "x6"),
        "int7": 7 if v is None else _atoi(v),
    }


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("switch_parse")
    src, exe = d / "main.cpp", d / "probe"
    src.write_text(MAIN)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", HEADER_DIR, str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr  # plain C++17, no HIP include
    return str(exe)


@pytest.mark.parametrize("value", VALUES, ids=lambda v: "unset" if v is None else repr(v))
def test_every_reader_follows_its_rule(probe, value):
    env = {k: v for k, v in os.environ.items() if k != VAR}
    if value is not None:
        env[VAR] = value
    out = subprocess.run([probe], env=env, capture_output=True, text=True, check=True).stdout
    got = dict(kv.split("=", 1) for kv in out.rstrip("\n").split("|"))
    want = expected(value)
    assert got == {k: str(x) for k, x in want.items()}
