"""The argument parsers of the five terrain-index command-line tools (taudem_amd/csrc/tools/indices_args.hpp) in a stand-alone program
(tests/indices/args_main.cpp) built with -fsanitize=address,undefined and run as a process of its own, on good and on malformed argument lists: the
flag and simple-use forms, the -par and -id defaults of the reference's mains, and a usage answer - never a read past argv - for everything else.
No GPU is needed and no sanitizer comes near code loaded into Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("indices_args") / "args_main")
    subprocess.run(["c++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "taudem_amd", "csrc", "tools"), os.path.join(ROOT, "tests", "indices", "args_main.cpp"), "-o", out], check=True)
    return out


def _run(exe, *args):
    p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stderr == "", (args, p.returncode, p.stderr)   # a sanitizer report goes to stderr and ends the process with a code
    return p.stdout.strip()


def _bits(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", np.float32(v)))[0]


def test_flag_forms_in_any_order(exe):
    assert _run(exe, "twi", "-twi", "o.tif", "-sca", "a.tif", "-slp", "s.tif") == f"files [s.tif] [a.tif] [o.tif] par 0 0 {_bits(0)} {_bits(0)} id 1"
    assert _run(exe, "slopearearatio", "-slp", "s.tif", "-sca", "a.tif", "-sar", "o.tif").startswith("files [s.tif] [a.tif] [o.tif]")
    assert _run(exe, "slopearea", "-slp", "s", "-sca", "a", "-sa", "o") == f"files [s] [a] [o] par 2 1 {_bits(2)} {_bits(1)} id 1"
    assert _run(exe, "slopearea", "-par", "1.5", "-0.75", "-slp", "s", "-sca", "a", "-sa", "o") == f"files [s] [a] [o] par 1.5 -0.75 {_bits(1.5)} {_bits(-0.75)} id 1"
    assert _run(exe, "lengtharea", "-plen", "l", "-ad8", "a", "-ss", "o").endswith(f"{_bits(0.03)} {_bits(1.3)} id 1")   # the floats 0.03f and 1.3f
    assert _run(exe, "lengtharea", "-ss", "o", "-par", "0.5", "1", "-ad8", "a", "-plen", "l") == f"files [l] [a] [o] par 0.5 1 {_bits(0.5)} {_bits(1)} id 1"
    assert _run(exe, "setregion", "-p", "p", "-gw", "g", "-out", "o").endswith("id 1")
    assert _run(exe, "setregion", "-id", "-7", "-out", "o", "-gw", "g", "-p", "p") == f"files [p] [g] [o] par 0 0 {_bits(0)} {_bits(0)} id -7"
    assert _run(exe, "twi", "-slp", "s.tif", "-slp", "t.tif").startswith("files [t.tif] [] []")   # a file that is not named stays empty: the tool cannot open it


def test_simple_use_adds_the_suffixes(exe):
    assert _run(exe, "twi", "dir.v1/base.tif").startswith("files [dir.v1/baseslp.tif] [dir.v1/basesca.tif] [dir.v1/basetwi.tif]")
    assert _run(exe, "slopearea", "base").startswith("files [baseslp] [basesca] [basesa] par 2 1")
    assert _run(exe, "slopearearatio", "base.tif").startswith("files [baseslp.tif] [basesca.tif] [basesar.tif]")
    assert _run(exe, "lengtharea", "base.tif").startswith("files [baseplen.tif] [basead8.tif] [basess.tif] par 0.0299999993 1.29999995")
    assert _run(exe, "setregion", "base.tif") == "usage"   # SetRegion has no simple use
    assert _run(exe, "twi", "-slp").startswith("files [-slpslp] [-slpsca] [-slptwi]")   # one word is a base name whatever it looks like, as in the reference


@pytest.mark.parametrize("args", [("twi",), ("twi", "-slp", "s", "-sca"), ("twi", "-slp", "s", "-par", "1", "2"), ("twi", "-slp", "s", "extra"),
                                  ("slopearea", "-par", "1"), ("slopearea", "-slp", "s", "-par", "1"), ("slopearea", "-id", "3", "-slp", "s"),
                                  ("lengtharea", "-plen", "l", "-ad8"), ("lengtharea", "-ss", "o", "-par", "0.5"), ("setregion",), ("setregion", "-p"),
                                  ("setregion", "-p", "p", "-id"), ("setregion", "-p", "p", "-par", "1", "2"), ("slopearearatio", "", "")])
def test_malformed_lists_get_the_usage(exe, args):
    assert _run(exe, *args) == "usage"


def test_words_that_are_no_numbers_leave_the_defaults(exe):
    assert _run(exe, "slopearea", "-slp", "s", "-par", "x", "y").endswith(f"{_bits(2)} {_bits(1)} id 1")
    assert _run(exe, "setregion", "-p", "p", "-id", "seven").endswith("id 1")
    assert _run(exe, "lengtharea", "-par", "1e-3", "nan", "-plen", "l").startswith("files [l] [] [] par 0.00100000005 nan")
