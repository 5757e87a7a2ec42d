"""The host ring builder and the polygon layer writer in a stand-alone program (tests/polygonize/rings_main.cpp) built with
-fsanitize=address,undefined -fno-sanitize-recover=all and run as a process of its own: on the hand cases (one part, three parts, a part per edge
or so) its text equals the model's polygons and both layer formats are written; on malformed edge lists - shuffled, truncated, successors that point
nowhere, beyond the raster or at each other - it answers "refused" and never reads past an array.  No GPU is needed and no sanitizer comes near
code loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import polygon_parse as P
import polygonize_model as M
from test_polygonize_model import HAND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "taudem_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("polygonize_rings") / "rings_main")
    subprocess.run(["c++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "polygonize", "rings_main.cpp"), os.path.join(CSRC, "polygon_rings.cpp"), os.path.join(CSRC, "vector_layer.cpp"),
                    "-o", out], check=True)
    return out


def _run(exe, *args):
    p = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (args, p.returncode, p.stderr)   # a sanitizer report goes to stderr and ends the process with a code
    return p.stdout


def _edges_file(path, keys, nxt, ids):
    with open(path, "w") as f:
        for k, n, i in zip(keys.tolist(), nxt.tolist(), ids.tolist()):
            f.write(f"{k} {n} {i}\n")
    return path


def _text(m):
    out = []
    for a, cells, polys in M.features(m):
        out.append(f"feature {a} {cells}")
        for p in polys:
            out.append("polygon")
            out += ["ring " + " ".join(f"{c} {r}" for c, r in ring) for ring in p]
    return "".join(line + "\n" for line in out)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases_under_sanitizers(exe, name, tmp_path):
    w = HAND[name]
    ny, nx = w.shape
    m = M.polygonize(w)
    edges = _edges_file(tmp_path / "edges.txt", m.keys, m.next_keys, m.edge_ids)
    want = _text(m)
    for parts in (1, 3, max(1, len(m.keys))):
        assert _run(exe, edges, nx, ny, parts) == want
    for ext in (".shp", ".geojson"):
        assert _run(exe, edges, nx, ny, 2, tmp_path / ("layer" + ext)) == want
    shp_rings = [r for _, rr in P.shapefile_features(str(tmp_path / "layer.shp")) for r in rr]
    assert shp_rings == [[(float(c), -float(r)) for c, r in ring] for _, _, polys in M.features(m) for p in polys for ring in p]
    assert [len(polys) for _, polys in P.geojson(str(tmp_path / "layer.geojson"))[0]] == [len(polys) for _, _, polys in M.features(m)]


def test_malformed_edge_lists_are_refused(exe, tmp_path):
    w = HAND["cut"]
    ny, nx = w.shape
    m = M.polygonize(w)
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(m.keys))
    cases = {
        "shuffled": (m.keys[perm], m.next_keys[perm], m.edge_ids[perm]),
        "truncated": (m.keys[:-7], m.next_keys[:-7], m.edge_ids[:-7]),
        "middle_missing": (np.delete(m.keys, slice(20, 40)), np.delete(m.next_keys, slice(20, 40)), np.delete(m.edge_ids, slice(20, 40))),
        "successor_nowhere": (m.keys, np.where(np.arange(len(m.keys)) == 5, -1, m.next_keys), m.edge_ids),
        "successor_beyond": (m.keys, np.where(np.arange(len(m.keys)) == 5, 2 ** 62, m.next_keys), m.edge_ids),
        "successors_rotated": (m.keys, np.roll(m.next_keys, 1), m.edge_ids),
        "self_successors": (m.keys, m.keys, m.edge_ids),
        "keys_beyond": (m.keys + 4 * nx * ny, m.next_keys + 4 * nx * ny, m.edge_ids),
        "negative_keys": (m.keys - 4 * nx * ny, m.next_keys, m.edge_ids),
        "duplicate_keys": (np.repeat(m.keys, 2), np.repeat(m.next_keys, 2), np.repeat(m.edge_ids, 2)),
    }
    for name, (k, n, i) in cases.items():
        out = _run(exe, _edges_file(tmp_path / (name + ".txt"), np.asarray(k), np.asarray(n), np.asarray(i)), nx, ny, 2)
        assert out.startswith("refused: polygon rings: "), (name, out)
    # a raster narrower than the keys were made for: keys and successors land in other cells
    out = _run(exe, _edges_file(tmp_path / "narrow.txt", m.keys, m.next_keys, m.edge_ids), nx - 1, ny + 2, 1)
    assert out.startswith("refused: polygon rings: ")
    assert _run(exe, _edges_file(tmp_path / "none.txt", m.keys[:0], m.next_keys[:0], m.edge_ids[:0]), nx, ny, 1) == ""
