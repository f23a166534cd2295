"""CPU: the RD trials' bit count (x264_vs2008_amd/csrc/cabac_price.h) replayed on real chains.  tests/cabac_price_devhost.cpp defines the
devhost_* entry points of oracle/devcheck.cpp, its whole-macroblock bit count running the mask-driven pricing; it is linked with the
CPU twin's own sources built with -DX264O_DEVCHECK (the sources and flags of oracle/Makefile's libdevcheck.so rule, into a temporary directory),
which replays EVERY call it makes while it encodes a chain and compares count, context states and record -- over the chains of
tests/test_devhost.py."""
import ctypes
import glob
import os
import re
import subprocess

import pytest

from paths import ROOT
from oracle import refslice as rs
from oracle.gen_golden_slice import CASES2, case_inputs

def makefile_rule():
    """What oracle/Makefile's libdevcheck.so rule compiles with, read from the Makefile so that it cannot drift: (OFLAGS, OSRC with its wildcard
    resolved, the g++ flags of the devcheck.cpp line)."""
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    oflags = re.search(r"^OFLAGS\s*=\s*(.+)$", text, re.M).group(1).split()
    osrc = re.search(r"^OSRC\s*=\s*(.+)$", text, re.M).group(1)
    osrc = re.sub(r"\$\(wildcard ([^)]+)\)", lambda m: " ".join(os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "oracle", m.group(1)))), osrc).split()
    rule = text[text.index("libdevcheck.so:"):]
    gxx = re.search(r"^\tg\+\+ (.+) -c devcheck\.cpp -o devcheck\.o$", rule, re.M).group(1).split()
    link = re.search(r"^\t\$\(CC\) \$\(OFLAGS\) (.+) -shared -o \$@ \$\(OSRC\) devcheck\.o (.+)$", rule, re.M)
    return oflags, osrc, gxx, link.group(1).split(), link.group(2).split()


@pytest.fixture(scope="module")
def price_devcheck_lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cabac_price_devhost")
    obj, so = str(tmp / "cabac_price_devhost.o"), str(tmp / "libdevcheck_price.so")
    oflags, osrc, gxx, defs, libs = makefile_rule()
    assert "-DX264O_DEVCHECK" in defs
    subprocess.run(["g++", *gxx, "-I", os.path.join(ROOT, "x264_vs2008_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-c", os.path.join(ROOT, "tests", "cabac_price_devhost.cpp"), "-o", obj], check=True)
    subprocess.run([os.environ.get("CC", "gcc"), *oflags, *defs, "-shared", "-o", so, *osrc, obj, *libs], cwd=os.path.join(ROOT, "oracle"), check=True)
    return ctypes.CDLL(so)


@pytest.mark.parametrize("name,size,frames,kind,kw,ekw", CASES2, ids=[c[0] for c in CASES2])
def test_trial_pricing_on_every_call_of_a_chain(price_devcheck_lib, name, size, frames, kind, kw, ekw):
    lib = price_devcheck_lib
    before_calls, before_bad = lib.x264o_devcheck_calls(), lib.x264o_devcheck_bad()
    p = rs.make_params(size[0], size[1], frames, **kw)
    y, u, v = case_inputs(size, frames, kind)
    rs.run2(lib, "x264o_encode_chain2", p, rs.make_ext(**ekw), y, u, v)
    assert lib.x264o_devcheck_calls() - before_calls > 100      # the replay really ran
    assert lib.x264o_devcheck_bad() == before_bad
