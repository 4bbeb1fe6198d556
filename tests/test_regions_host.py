"""Smooth regions (contract (J)), the parts that need no GPU: the companion header and the binding, the
argument checks of smooth_regions, and the reference tests/regions_ref.py held to things it shares no code with -- surfaces with
analytic normals whose regions are known, and the contract's details on hand-made clouds.  The cosines come from the library's
own argument check (features.regions_arguments), as smooth_regions forms them on the host."""
import ctypes as C
import inspect
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import plane_ref
import regions_ref

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "simpleicp_hip_regions.h"


def cos_min(max_angle, oriented=False):
    from simpleicp_amd import features
    c = features.regions_arguments(max_angle=max_angle, oriented=oriented)[1]
    assert c == math.cos(math.radians(max_angle))
    return c


# ---- header, exports, binding ----
def test_header_names_are_exported_and_bound():
    from simpleicp_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text))) == sorted(_lib.REGIONS_EXPORTS) == ["sicp_regions", "sicp_regions_version"]
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    assert set(_lib.REGIONS_EXPORTS) <= set(re.findall(r" T (sicp_\w+)", out))
    others = set(_lib.EXPORTS)
    for name, f in _lib.FEATURES.items():
        if name != "regions":
            others |= set(f.exports)
    assert not set(_lib.REGIONS_EXPORTS) & others
    f = _lib.FEATURES["regions"]
    assert f.exports == _lib.REGIONS_EXPORTS and f.header == HEADER.name and f.version == 1 and f.exports[0] == "sicp_regions_version"
    L = _lib.load()
    assert "#define SICP_REGIONS_VERSION 1" in HEADER.read_text()
    assert L.sicp_regions_version() == _lib.REGIONS_VERSION == 1 and _lib.regions_version() == 1
    assert C.sizeof(_lib.RegionsStats) == 72 and [n for n, _ in _lib.RegionsStats._fields_] == list(regions_ref.KEYS)
    assert "contract (J)" in HEADER.read_text() and "(nx_i * nx_j + ny_i * ny_j) + nz_i * nz_j" in HEADER.read_text()
    # the main header and its version are untouched
    assert L.sicp_abi_version() == _lib.ABI_VERSION == 7
    assert "regions" not in (ROOT / "include" / "simpleicp_hip.h").read_text()
    assert any(p.name == "sicp_regions.hip" for p in build.SOURCES) and any(p.name == HEADER.name for p in build.HEADERS)
    assert any(p.name == "sicp_union_dev.h" for p in build.HEADERS)
    assert list(inspect.signature(_lib.Context.regions).parameters)[1:9] == ["slot", "normals", "k", "cos_min", "radius", "oriented", "seeds",
                                                                             "min_size"]
    assert 'getenv("SICP_REGIONS_CHUNK")' in (ROOT / "simpleicp_amd" / "csrc" / "sicp_api.cpp").read_text()


def test_header_is_plain_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "probe.c"
    src.write_text('#include "simpleicp_hip_regions.h"\n'
                   "int probe(sicp_ctx *c, const float *nrm, const uint8_t *seeds, int32_t *labels)\n{\n"
                   "    sicp_regions_stats a;\n"
                   "    int rc = sicp_regions_version() + sicp_regions(c, SICP_FIX, nrm, 16, 0.5, 0.99, 0, seeds, 1, labels, &a);\n"
                   "    return rc + (int)(a.n_points + a.n_void + a.n_smooth + a.n_border + a.n_regions_all + a.n_regions + a.n_labelled\n"
                   "                      + a.largest_label + a.largest_size) + SICP_REGIONS_VERSION;\n}\n")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", "-c", str(src), "-o",
                        str(tmp_path / "probe.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_ctx_is_refused_not_dereferenced():
    from simpleicp_amd import _lib
    L = _lib.load()
    N, labels, st = np.zeros((8, 3), np.float32), np.full(8, 77, np.int32), _lib.RegionsStats()
    rc = L.sicp_regions(None, _lib.FIX, _lib._ptr(N), 4, math.inf, 0.5, 0, None, 1, _lib._ptr(labels), C.byref(st))
    assert rc == _lib.ERR_INVALID and b"null ctx" in L.sicp_last_error() and np.all(labels == 77)


def test_argument_errors_name_the_keyword_and_an_empty_input_touches_nothing(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import backend
    monkeypatch.setattr(backend, "get_context", lambda: pytest.fail("the library is not touched"))
    E = np.zeros((0, 3))
    labels, info = simpleicp_amd.smooth_regions(E, return_info=True)
    assert labels.shape == (0,) and labels.dtype == np.int32
    assert info == dict(dict.fromkeys(regions_ref.KEYS, 0), cos_min=math.cos(math.radians(5.0)))
    assert simpleicp_amd.smooth_regions(E, max_angle=180.0, oriented=True, return_info=True)[1]["cos_min"] == -1.0
    assert simpleicp_amd.smooth_regions(E, cos_min=0.25, return_info=True)[1]["cos_min"] == 0.25
    X, N = np.zeros((5, 3)), np.ones((5, 3))
    for word, kw in (("max_angle", dict(max_angle=0.0)), ("max_angle", dict(max_angle=90.5)), ("max_angle", dict(max_angle=181.0, oriented=True)),
                     ("max_angle", dict(max_angle=math.nan)), ("max_angle", dict(max_angle="5")), ("cos_min", dict(cos_min=1.5)),
                     ("cos_min", dict(cos_min=-0.1)), ("cos_min", dict(cos_min=-1.5, oriented=True)), ("cos_min", dict(cos_min=math.nan)),
                     ("max_angle", dict(cos_min=0.5, max_angle=10.0)), ("radius", dict(radius=0.0)), ("radius", dict(radius=math.nan)),
                     ("radius", dict(radius="1")), ("min_size", dict(min_size=0)), ("min_size", dict(min_size=1.5)),
                     ("neighbors", dict(neighbors=1)), ("neighbors", dict(neighbors=129)), ("neighbors", dict(neighbors=6)),
                     ("normal_neighbors", dict(normal_neighbors=1)), ("oriented", dict(oriented=1)), ("return_info", dict(return_info=1)),
                     ("min_planarity", dict(min_planarity="x")), ("min_planarity", dict(min_planarity=0.5, normals=N)),
                     ("min_planarity", dict(min_planarity=0.5, seeds=np.ones(5, bool))), ("seeds", dict(normals=N, seeds=np.ones(4, bool))),
                     ("normals", dict(normals=N[:4]))):
        with pytest.raises(ValueError, match=word):
            simpleicp_amd.smooth_regions(X, **kw)
    assert "smooth_regions" in simpleicp_amd.__all__


# ---- analytic normals, max_angle = 5 ----
def test_a_cubes_six_faces_are_six_regions():
    X, N, face = regions_ref.cube(1, m=12)
    ref = regions_ref.regions(X, N, 8, cos_min(5.0))
    assert ref["n_regions"] == ref["n_regions_all"] == 6 and ref["n_border"] == 0 and ref["n_labelled"] == len(X)
    for f in range(6):
        lab = np.unique(ref["labels"][face == f])
        assert len(lab) == 1 and (ref["labels"] == lab[0]).sum() == 144
    assert ref["labels"][0] == 0 and ref["largest_label"] == 0 and ref["largest_size"] == 144
    # the labels follow the lowest indices: shuffled, the partition is the same and the numbering follows the new first points
    p = np.random.default_rng(2).permutation(len(X))
    again = regions_ref.regions(X[p], N[p], 8, cos_min(5.0))
    first = [int(np.flatnonzero(again["labels"] == lab)[0]) for lab in range(6)]
    assert first == sorted(first) and all(len(np.unique(face[p][again["labels"] == lab])) == 1 for lab in range(6))


def test_two_half_planes_at_ten_degrees():
    X, N, side = regions_ref.hinge(3, 10.0)
    ref = regions_ref.regions(X, N, 8, cos_min(5.0))
    assert ref["n_regions"] == 2 and np.array_equal(ref["labels"], side)
    assert regions_ref.regions(X, N, 8, cos_min(15.0))["n_regions"] == 1


def test_a_cylinders_mantle_is_one_region_and_no_plane_covers_it():
    X, N = regions_ref.cylinder(2.0)
    ref = regions_ref.regions(X, N, 9, cos_min(5.0))
    assert ref["n_regions"] == 1 and ref["n_labelled"] == len(X) == ref["largest_size"]
    found = plane_ref.segment_plane(X, 0.01, hypotheses=256, seed=0)
    assert found is None or found[2] < len(X) // 4


# ---- contract details ----
def strip_scene():
    """One flat sheet, equal normals: columns x < 1 (plane A), 1 <= x < 1.3 (the rough strip: no seeds), x >= 1.3 (plane B)."""
    h = 0.05
    u, v = np.meshgrid(np.arange(0.0, 2.3, h) + 0.01, np.arange(0.0, 0.5, h), indexing="ij")
    X = np.column_stack([u.ravel(), v.ravel(), np.zeros(u.size)])
    X += np.random.default_rng(4).uniform(-0.01, 0.01, X.shape) * [1, 1, 0]
    N = np.tile([0.0, 0.0, 1.0], (len(X), 1))
    part = np.where(X[:, 0] < 1.0, 0, np.where(X[:, 0] < 1.3, 1, 2))
    return np.ascontiguousarray(X), N, part


def test_a_rough_strip_between_two_planes_bridges_nothing():
    X, N, part = strip_scene()
    assert regions_ref.regions(X, N, 8, cos_min(5.0))["n_regions"] == 1
    ref = regions_ref.regions(X, N, 8, cos_min(5.0), seeds=part != 1)
    lab = ref["labels"]
    assert ref["n_regions"] == 2 and set(lab[part == 0]) == {0} and set(lab[part == 2]) == {1}
    strip = part == 1
    assert ref["n_smooth"] == int((~strip).sum()) and 0 < ref["n_border"] < strip.sum()      # the strip's middle column sees no seed
    # a border point belongs to the lower root among the planes it touches: what touches A is A's, whatever else it touches
    idx = regions_ref.lists(X, 8)[0]
    sees_a = np.array([(part[idx[i]] == 0).any() or (part[(idx == i).any(axis=1)] == 0).any() for i in np.flatnonzero(strip)])
    assert sees_a.any() and (lab[strip][sees_a] == 0).all() and set(lab[strip][~sees_a]) <= {1, -1} and (lab[strip] == -1).any()


def test_min_size_drops_a_patch_renumbers_and_leaves_its_border_unlabelled():
    X, N, part = strip_scene()
    far = np.array([[10.0, 0, 0], [10.05, 0, 0], [10.1, 0, 0], [10.15, 0, 0]])              # a small patch: three seeds and a border
    X2 = np.ascontiguousarray(np.vstack([far, X]))
    N2 = np.vstack([np.tile([0.0, 0.0, 1.0], (4, 1)), N])
    seeds = np.concatenate([[True, True, True, False], part != 1])
    all_ = regions_ref.regions(X2, N2, 4, cos_min(5.0), seeds=seeds)
    assert all_["n_regions"] == 3 and all_["labels"][:4].tolist() == [0, 0, 0, 0] and all_["kind"][3] == 1
    kept = regions_ref.regions(X2, N2, 4, cos_min(5.0), seeds=seeds, min_size=5)
    assert kept["n_regions_all"] == 3 and kept["n_regions"] == 2 and kept["labels"][:4].tolist() == [-1, -1, -1, -1]
    assert kept["n_border"] == all_["n_border"] and kept["n_labelled"] == all_["n_labelled"] - 4
    assert np.array_equal(kept["labels"][4:], np.where(all_["labels"][4:] >= 0, all_["labels"][4:] - 1, -1))
    none = regions_ref.regions(X2, N2, 4, cos_min(5.0), seeds=seeds, min_size=len(X2) + 1)
    assert none["n_regions"] == 0 and (none["labels"] == -1).all() and (none["largest_label"], none["largest_size"]) == (-1, 0)


def test_oriented_separates_the_two_sides_of_a_thin_plate():
    xy = regions_ref.hinge(6, 0.0, m=15)[0][:225, :2]
    xy = np.vstack([xy, xy[:75] + [0.0, 1.0]])                                              # a jittered lattice of 300 points
    top = np.column_stack([xy, np.full(300, 0.001)])
    X = np.ascontiguousarray(np.vstack([top, top * [1, 1, -1]]))
    N = np.vstack([np.tile([0.0, 0.0, 1.0], (300, 1)), np.tile([0.0, 0.0, -1.0], (300, 1))])
    assert regions_ref.regions(X, N, 8, cos_min(5.0))["n_regions"] == 1
    ref = regions_ref.regions(X, N, 8, cos_min(5.0, oriented=True), oriented=True)
    assert ref["n_regions"] == 2 and np.array_equal(ref["labels"], np.repeat([0, 1], 300))


def test_void_normals_have_no_edges_and_no_label():
    X, N, _ = regions_ref.hinge(7, 0.0, m=10)
    N = N.astype(np.float32)
    N[0] = (np.nan, 0, 1)
    N[5] = (0, 0, 0)
    N[9] = (np.inf, 0, 1)
    N[11] = (-0.0, 0.0, -0.0)
    ref = regions_ref.regions(X, N, 6, cos_min(5.0))
    assert ref["n_void"] == 4 and (ref["labels"][[0, 5, 9, 11]] == -1).all() and ref["n_labelled"] == len(X) - 4
    assert ref["n_regions"] == 1 and ref["labels"][1] == 0 and ref["root"][1] == 1         # the lowest index that is not void


def test_a_border_edge_that_only_the_smooth_point_lists():
    X = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.5, 0, 0]])
    idx = regions_ref.lists(X, 2)[0]
    assert idx.tolist() == [[0, 1], [1, 2], [2, 1]]                                          # point 1 does not list point 0
    N = np.tile([0.0, 0.0, 1.0], (3, 1))
    ref = regions_ref.regions(X, N, 2, cos_min(5.0), seeds=[1, 0, 0])
    assert ref["labels"].tolist() == [0, 0, -1] and ref["n_border"] == 1 and ref["largest_size"] == 2
    assert regions_ref.record(ref) == dict(n_points=3, n_void=0, n_smooth=1, n_border=1, n_regions_all=1, n_regions=1, n_labelled=2,
                                           largest_label=0, largest_size=2)
