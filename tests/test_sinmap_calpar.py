"""The -calpar reader of the library (tdx_sinmap_read_calpar through taudem_amd.read_calpar) against the Python model of tests/sinmap_model.py, on every
file variant of the goldens and a few more, the refused short line and the missing file.  No GPU is needed."""
import numpy as np
import pytest

import sinmap_model as M
import taudem_amd as T

HEAD = "id,tmin,tmax,cmin,cmax,phimin,phimax,rhos\n"
TEXTS = {
    "plain": M.CALPAR,
    "variant": M.CALPAR_VARIANT,                               # duplicate id, hexadecimal and octal ids, blanks after commas, a trailing blank line
    "no_final_newline": M.CALPAR.rstrip("\n"),
    "several_blank_lines": M.CALPAR + "\n   \n\n",
    "crlf": M.CALPAR.replace("\n", "\r\n"),
    "negative_and_large_ids": HEAD + "-3,1,2,0,0.25,30,45,2000\n70000,1,2,0,0.25,30,45,2000\n010,1.5,2.5,0.125,0.5,20,40,1500\n",
    "exponents": HEAD + "5,2e0,3.0E0,1e-1,2.5e-1,3e1,45,2e3\n",
    "header_only": HEAD,
}


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_reader_equals_the_model(tmp_path, name):
    path = tmp_path / "calpar.csv"
    path.write_bytes(TEXTS[name].encode())
    got, want = T.read_calpar(str(path)), M.parse_calpar(TEXTS[name].replace("\r", ""))
    assert list(got) == list(M.FIELDS)
    for k in M.FIELDS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, k, got[k], want[k])


@pytest.mark.parametrize("name, ids", [("variant", [1, 2, 1, 7, 300]), ("negative_and_large_ids", [-3, 70000, 8])])
def test_variant_file_ids(tmp_path, name, ids):
    """the ids as written here, from the library's reader and from the model (hexadecimal and leading-zero octal ids among them: 010 is 8)"""
    path = tmp_path / "calpar.csv"
    path.write_text(TEXTS[name])
    assert T.read_calpar(str(path))["id"].tolist() == ids and M.parse_calpar(TEXTS[name])["id"].tolist() == ids


@pytest.mark.parametrize("bad, line", [(HEAD + "1,2.0,3.0,0.0,0.25,30.0,45.0\n", 2), (M.CALPAR + "9,1.0\n", 6), (HEAD + "1,2,3,0,0.25,30,45,2000\nabc\n", 3)])
def test_short_line_is_refused_with_its_line_number(tmp_path, bad, line):
    path = tmp_path / "short.csv"
    path.write_text(bad)
    with pytest.raises(T.TdxError) as e:
        T.read_calpar(str(path))
    assert e.value.code == -1 and f"line {line} " in str(e.value)
    with pytest.raises(ValueError, match=f"line {line}"):
        M.parse_calpar(bad)


def test_stand_alone_program_on_the_library_source(tmp_path):
    """tests/sinmap/calpar_main.cpp with taudem_amd/csrc/sinmap_table.cpp, the file the library is built from: the table's bits, the derived constants
    (tan of the float-rounded angle and the float division, from the host libm) and the first-match lookup"""
    import math
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "taudem_amd", "csrc")
    exe = str(tmp_path / "calpar_main")
    subprocess.run(["c++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + csrc, os.path.join(root, "tests", "sinmap", "calpar_main.cpp"),
                    os.path.join(csrc, "sinmap_table.cpp"), "-o", exe], check=True)
    files = []
    for name in ("variant", "negative_and_large_ids"):
        f = tmp_path / (name + ".csv")
        f.write_text(TEXTS[name])
        files.append(str(f))
    long_line = tmp_path / "long.csv"
    long_line.write_text(HEAD + "1,2,3,0,0.25,30,45,2000" + " " * 6000 + "\n2,2,3,0,0.25,30,45,2000\n")   # a line longer than the 4096-byte buffer: its rest is a line without fields
    short = tmp_path / "short.csv"
    short.write_text(HEAD + "1,2\n")
    r = subprocess.run([exe, *files, str(long_line), str(short), str(tmp_path / "nope.csv")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    out = r.stdout.split("file ")[1:]
    assert out[0].startswith("1 rc 0 regions 5 err -") and out[1].startswith("2 rc 0 regions 3 err -")
    assert out[2].startswith("3 rc 0 regions 2 err -") and out[3].startswith("4 rc -1 regions 0") and "line 2 " in out[3] and out[4].startswith("5 rc 15 ")
    t = M.parse_calpar(M.CALPAR_VARIANT)
    lines = out[0].splitlines()
    for k in range(5):
        want = [str(int(t["id"][k]))] + [f"{int(np.float32(t[f][k]).view(np.uint32)):08x}" for f in M.FIELDS[1:]]
        assert lines[1 + k].split() == want, (k, lines[1 + k])
        ang = [float(np.float32(float(t[f][k]) * 3.14159265358979 / 180)) for f in ("phimin", "phimax")]
        r_ = np.float32(1000.0) / t["rhos"][k]
        want = [f"{np.float64(math.tan(a)).view(np.uint64):016x}" for a in ang] + [f"{np.float64(r_).view(np.uint64):016x}"]
        assert lines[6 + k].split()[2:] == want, (k, lines[6 + k])
    # id 1 is listed twice: the first entry (0) wins; 7 is entry 3, 300 entry 4; the nodata value, 0 and 99 match nothing
    assert lines[11].split() == ["lut", "-32768:-1", "-3:-1", "0:-1", "1:0", "2:1", "7:3", "8:-1", "99:-1", "300:4", "32767:-1"]
    assert out[1].splitlines()[-1].split() == ["lut", "-32768:-1", "-3:0", "0:-1", "1:-1", "2:-1", "7:-1", "8:2", "99:-1", "300:-1", "32767:-1"]   # 70000 is no int16


def test_missing_file_is_code_15(tmp_path):
    with pytest.raises(T.TdxError) as e:
        T.read_calpar(str(tmp_path / "nope.csv"))
    assert e.value.code == 15


def test_tool_function_returns_15_for_an_unreadable_calpar(tmp_path, capfd):
    from taudem_amd import tools

    rc = tools.sinmapsi(str(tmp_path / "slp.tif"), str(tmp_path / "sca.tif"), str(tmp_path / "cal.tif"), str(tmp_path / "nope.csv"), str(tmp_path / "si.tif"),
                        str(tmp_path / "sat.tif"), 0.0009, 0.00135)
    assert rc == 15 and "SinmapSI version" in capfd.readouterr().out
