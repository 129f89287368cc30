"""The premises of the fixtures of tests/remesh_feature_oracle.py, on the CPU: that each is a valid input with the classes its
docstring names, that each collapse rule of the "Creases" section is the only thing between some candidate and its collapse,
that the hinge is an exact tie, and what the rules buy on the cube.  A failure of tests/test_gpu_remesh_features.py then means
the device."""
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest

import collapse_oracle as CO
import remesh_feature_oracle as FO
import remesh_oracle as RO


def classes(name, cos_t=FO.COS30):
    vs, faces = FO.FIXTURES[name]()
    return FO.features(vs, faces, cos_t)


@pytest.mark.parametrize("name", sorted(FO.FIXTURES))
def test_fixture_is_a_valid_input(name):
    vs, faces = FO.FIXTURES[name]()
    assert vs.dtype == np.float32 and faces.dtype == np.int64
    assert all(v == 0 for k, v in RO.check_input(vs, faces).items() if k.startswith("n_"))
    assert RO.directed_once(faces) and FO.TARGETS[name] > 0
    if name not in ("roof", "bent"):
        assert not RO.valences(faces)[1] and FO.volume(vs, faces) > 0          # closed, outward


def test_classes_of_the_fixtures():
    vclass, nbr, edges = classes("cube")
    assert vclass.tolist() == [FO.CORNER] * 8 and len(edges) == 12 and (nbr == -1).all()
    assert all(int((FO.cube()[0][a] != FO.cube()[0][b]).sum()) == 1 for a, b in edges)       # the cube's edges, not the diagonals

    vclass, nbr, edges = classes("roof")
    assert edges.tolist() == [[1, 4], [4, 7], [7, 10], [10, 13]]
    assert [v for v in range(15) if vclass[v] == FO.LINE] == [4, 7, 10] and nbr[4].tolist() == [1, 7] and nbr[10].tolist() == [7, 13]
    assert vclass[1] == vclass[13] == FO.BORDER and Counter(vclass.tolist()) == {FO.LINE: 3, FO.BORDER: 12}

    vclass, nbr, edges = classes("prism16")
    assert Counter(vclass.tolist()) == {FO.LINE: 32, FO.SMOOTH: 18} and len(edges) == 32
    assert (vclass[:16] == FO.LINE).all() and (vclass[16:32] == FO.SMOOTH).all() and (vclass[32:48] == FO.LINE).all()
    assert nbr[0].tolist() == [1, 15] and nbr[5].tolist() == [4, 6] and nbr[47].tolist() == [32, 46]

    vclass, _, edges = classes("l_prism")
    assert vclass.tolist() == [FO.CORNER] * 12 and len(edges) == 18
    nc = FO.crease_counts({tuple(e) for e in edges.tolist()})[0]
    assert set(nc.values()) == {3} and [3, 9] in edges.tolist()                # the reflex edge at (1, 1) is a crease too

    vclass, _, edges = classes("pyramid")
    nc = FO.crease_counts({tuple(e) for e in edges.tolist()})[0]
    assert vclass.tolist() == [FO.CORNER] * 5 and nc[4] == 4 and [nc[v] for v in range(4)] == [3] * 4
    vclass, nbr, edges = classes("pyramid", FO.feature_cos(120.0))              # cos_t < 0: only the base edges (135 degrees)
    assert vclass.tolist() == [FO.LINE] * 4 + [FO.SMOOTH] and edges.tolist() == [[0, 1], [0, 3], [1, 2], [2, 3]]
    assert nbr[:4].tolist() == [[1, 3], [0, 2], [1, 3], [0, 2]]

    vclass, nbr, edges = classes("bent")
    assert vclass.tolist() == [FO.LINE] + [FO.BORDER] * 10 and edges.tolist() == [[0, 1], [0, 2]] and nbr[0].tolist() == [1, 2]


def test_hinge_is_an_exact_tie():
    vs, faces = FO.hinge60()
    n1, n2 = RO._normal(vs, 0, 1, 2), RO._normal(vs, 1, 0, 3)
    assert n1 == (1.0, 1.0, 0.0) and n2 == (1.0, 0.0, 1.0)
    dd, q = RO._dot(n1, n2), RO._dot(n1, n1) * RO._dot(n2, n2)
    assert (dd, q) == (1.0, 4.0) and dd * dd == (0.5 * 0.5) * q                # the float64 products as the kernel forms them
    assert Fraction(dd) ** 2 == Fraction(1, 4) * Fraction(q)                   # and in exact arithmetic
    up = float(np.nextafter(0.5, 1.0))
    assert dd * dd < (up * up) * q
    assert not FO.is_crease(vs, 0, 1, 2, 3, 0.5) and FO.is_crease(vs, 0, 1, 2, 3, up)
    assert (0, 1) not in FO.crease_set(vs, faces, 0.5) and (0, 1) in FO.crease_set(vs, faces, up)
    # the lower half-edge names a, b, c: face 0 runs the edge from vertex 0 to vertex 1
    assert FO._quad(faces, RO.edge_table(faces)[0][(0, 1)]) == (0, 1, 2, 3)


def _guard_log(name):
    vs, faces = FO.FIXTURES[name]()
    log = []
    cands = FO.collapse_candidates(vs, faces, CO.collapse_threshold(FO.BENT_TARGET), RO.split_threshold(FO.BENT_TARGET), FO.COS30, log)
    plain = CO.collapse_candidates(vs, faces, CO.collapse_threshold(FO.BENT_TARGET), RO.split_threshold(FO.BENT_TARGET))
    return log, cands, plain


def test_each_collapse_rule_is_the_only_reason_for_some_refusal():
    """``log`` holds, per short edge, whether every condition of 2a. holds for the kept vertex and which crease rule refuses it;
    the three rules exclude one another, so (conditions hold, rule) names the rule as the only reason."""
    log, cands, plain = _guard_log("cube")
    only = [l for l in log if l[3] and l[4] == "corner"]
    assert len(only) == 12 and not cands and len(plain) == 12                   # every candidate of the plain rules removes a corner
    log, cands, plain = _guard_log("bent")
    by = {l[0]: l for l in log}
    assert by[(0, 1)][1:] == (1, 0, True, "bent") and by[(0, 2)][1:] == (2, 0, True, "bent")
    assert (0, 1) in plain and (0, 2) in plain and not cands
    assert FO.straight(*[FO.bent()[0]] + [1, 0, 2]) is False
    u = FO.bent()[0][0].astype(np.float64) - FO.bent()[0][1]
    v = FO.bent()[0][2].astype(np.float64) - FO.bent()[0][0]
    assert float(u @ v) == 0.0                                                # a turn of exactly 90 degrees: the strict > refuses it
    off = [l for l in log if l[3] and l[4] == "off-crease"]
    assert len(off) == 5 and all(l[2] == 0 and l[0] in plain for l in off)     # the hub would leave along a spoke of the cone
    log, cands, _ = _guard_log("roof")
    assert Counter(l[4] for l in log if l[3]) == {"off-crease": 6, None: 4}
    assert sorted(cands) == [(1, 4), (4, 7), (7, 10), (10, 13)]                # what is left runs along the ridge ...
    assert cands[(1, 4)][1:3] == (1, 4) and cands[(10, 13)][1:3] == (13, 10)   # ... and into the border end where there is one


def test_kept_vertex_precedence():
    border, nc = {7}, {1: 2, 2: 2, 3: 3, 4: 1}
    assert FO.kept_vertex(7, 3, border, nc) == 7 and FO.kept_vertex(3, 7, border, nc) == 7       # 1. the border end
    assert FO.kept_vertex(0, 1, border, nc) == 1 and FO.kept_vertex(2, 9, border, nc) == 2       # 2. the end with a crease
    assert FO.kept_vertex(1, 3, border, nc) == 3 and FO.kept_vertex(4, 2, border, nc) == 4       # 3. the corner end
    assert FO.kept_vertex(2, 1, border, nc) == 1 and FO.kept_vertex(3, 4, border, nc) == 3       # 4. min(a, b)
    assert FO.kept_vertex(9, 8, border, nc) == 8


def test_crease_step_is_the_border_rule_of_the_smoothing():
    """(R[v] + R[lo] + R[hi]) / 3: ``prepare_oracle.smooth_step`` on an open polyline strip moves a border vertex with two
    border edges the same way (there in float64)."""
    import prepare_oracle as PO
    vs, faces = RO.grid(3)
    vs = (vs + np.random.default_rng(3).normal(0, 0.1, vs.shape)).astype(np.float32)
    want = PO.smooth_step(vs, faces)
    nbr = np.full((16, 2), -1, np.int64)
    nbr[1], nbr[2], nbr[4], nbr[8] = (0, 2), (1, 3), (0, 8), (4, 12)            # border vertices between two border neighbours
    got = FO.crease_step(vs, nbr)
    moved = nbr[:, 0] >= 0
    assert got.dtype == np.float32 and np.array_equal(got[~moved], vs[~moved])
    assert np.abs(got[moved] - want[moved]).max() <= 2.0 ** -22 * np.abs(vs).max()
    assert got[1, 0] == np.float32(np.float32(np.float32(vs[1, 0] + vs[0, 0]) + vs[2, 0]) / np.float32(3.0))


@pytest.fixture(scope="module")
def cube_runs():
    vs, faces = FO.cube()
    return FO.refine_mesh(vs, faces, 0.25, FO.COS30, iterations=3), FO.refine_mesh(vs, faces, 0.25, None, iterations=3)


def test_cube_keeps_its_corners_edges_and_volume_under_the_oracle(cube_runs):
    (vs, faces, report), _ = cube_runs
    assert np.array_equal(vs[:8].view(np.uint32), FO.cube()[0].view(np.uint32))                  # all 8 corners, bit for bit
    vclass = FO.features(vs, faces, FO.COS30)[0]
    assert (vclass[:8] == FO.CORNER).all() and report["n_corners_end"] == 8 and report["n_crease_edges_start"] == 12
    line = vs[vclass == FO.LINE]
    assert len(line) > 12 and (np.isin(line, (0.0, 1.0)).sum(1) == 2).all()     # two coordinates in {0, 1}, exactly
    vol = FO.volume(vs, faces)
    print("cube with the angle: V", len(vs), "volume", vol)
    assert abs(vol - 1.0) <= 1e-5


def test_cube_without_the_angle_loses_its_corners(cube_runs):
    _, (vs, faces, _) = cube_runs
    vol = FO.volume(vs, faces)
    print("cube without the angle: V", len(vs), "volume", vol)
    assert vol < 0.95 and len(vs) == 194
    rows = {r.tobytes() for r in vs}
    assert not any(c.tobytes() in rows for c in FO.cube()[0])
    # cos_t None is today's oracle, call for call
    want = RO.refine_mesh(*FO.cube(), 0.25, iterations=3)
    assert np.array_equal(vs.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(faces, want[1])


def test_smooth_control_never_has_a_crease():
    vs, faces = FO.smooth_control()
    target = FO.SMOOTH_TARGET * RO.median_edge(vs, faces)
    FO.SEEN = seen = []
    try:
        _, _, report = FO.refine_mesh(vs, faces, target, FO.COS30, iterations=1, collapse=True)
    finally:
        FO.SEEN = None
    it = report["iterations"][0]
    print("smooth control: evaluations", len(seen), "splits", sum(it["split"]), "collapses", sum(it["collapse"]), "flips", sum(it["flip"]))
    assert len(seen) > 4 and max(seen) == 0 and sum(it["collapse"]) > 0 and sum(it["flip"]) > 0
