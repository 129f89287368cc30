"""Host side of the scoring step (semigcn_amd.evaluate, check/dist_check.py:13-67): the OBJ reader, the float64 oracle
on closed-form cases, and the absence of a CPU path."""
import numpy as np
import pytest
import torch

import mesh_distance_oracle as MO
from semigcn_amd import evaluate, synth
from semigcn_amd.capi import SemigcnLibraryError


def test_read_obj_round_trips_write_obj(tmp_path):
    m = synth.torus_mesh(12, 8, masks=False)
    p = tmp_path / "t.obj"
    synth.write_obj(str(p), m.vs, m.faces)
    vs, faces = evaluate.read_obj(str(p))
    assert vs.dtype == np.float32 and faces.dtype == np.int64
    assert vs.shape == m.vs.shape and np.array_equal(faces, m.faces)
    np.testing.assert_allclose(vs, m.vs, rtol=1e-6, atol=1e-6)


def test_read_obj_dialect(tmp_path):
    p = tmp_path / "d.obj"
    p.write_text("# comment\n"
                 "v 0 0 0 1 0 0\n"          # a coloured vertex (util/mesh.py:47-48)
                 "v 1 0 0\n"
                 "\n"
                 "vn 0 0 1\n"
                 "v 0 1 0 0.5 0.5 0.5\n"
                 "v 1 1 0\n"
                 "f 1/1/1 2/2/1 3/3/1\n"    # slash forms
                 "f 2//1 4//1 3//1\n"
                 "f -3 -1 -2\n")            # negative = relative to the vertices read so far
    vs, faces = evaluate.read_obj(str(p))
    assert vs.shape == (4, 3)
    np.testing.assert_array_equal(vs[3], [1, 1, 0])
    np.testing.assert_array_equal(faces, [[0, 1, 2], [1, 3, 2], [1, 3, 2]])
    q = tmp_path / "quad.obj"
    q.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3 4\n")
    with pytest.raises(ValueError, match="only triangles"):
        evaluate.read_obj(str(q))


def _one(p, a, b, c):
    d, cl, ins, side = MO.point_triangles(p, np.array([a], float), np.array([b], float), np.array([c], float))
    return d[0], cl[0], ins[0], side[0]


def test_oracle_closed_forms():
    a, b, c = [0, 0, 0], [2, 0, 0], [0, 2, 0]
    d, cl, ins, side = _one([0.5, 0.5, 3.0], a, b, c)            # above the interior
    assert d == pytest.approx(3.0) and ins and side > 0
    np.testing.assert_allclose(cl, [0.5, 0.5, 0.0])
    d, cl, ins, side = _one([0.5, 0.5, -2.0], a, b, c)           # below: the other side of the normal
    assert d == pytest.approx(2.0) and side < 0
    d, cl, ins, _ = _one([1.0, -3.0, 4.0], a, b, c)              # beyond edge a-b
    assert d == pytest.approx(5.0) and not ins
    np.testing.assert_allclose(cl, [1.0, 0.0, 0.0])
    d, cl, ins, _ = _one([2.0, 2.0, 0.0], a, b, c)               # beyond the hypotenuse, in plane
    assert d == pytest.approx(np.sqrt(2.0))
    np.testing.assert_allclose(cl, [1.0, 1.0, 0.0])
    d, cl, _, _ = _one([-3.0, -4.0, 0.0], a, b, c)               # beyond vertex a
    assert d == pytest.approx(5.0)
    np.testing.assert_allclose(cl, [0.0, 0.0, 0.0])
    d, cl, _, _ = _one([5.0, -4.0, 0.0], a, b, c)                # beyond vertex b
    assert d == pytest.approx(5.0)
    np.testing.assert_allclose(cl, b)


def test_oracle_degenerate_triangles():
    # collinear: the segment [0, 4] on x
    d, cl, ins, side = _one([1.0, 3.0, 4.0], [0, 0, 0], [4, 0, 0], [2, 0, 0])
    assert d == pytest.approx(5.0) and not ins and side == 0
    d, _, _, _ = _one([7.0, 4.0, 0.0], [0, 0, 0], [4, 0, 0], [2, 0, 0])
    assert d == pytest.approx(5.0)
    # repeated vertex: the segment [0, 2] on y
    d, cl, _, _ = _one([3.0, 1.0, 4.0], [0, 0, 0], [0, 2, 0], [0, 0, 0])
    assert d == pytest.approx(5.0)
    np.testing.assert_allclose(cl, [0, 1, 0])
    # all three the same point
    d, cl, _, _ = _one([3.0, 4.0, 12.0], [1, 1, 1], [1, 1, 1], [1, 1, 1])
    assert d == pytest.approx(np.linalg.norm([2, 3, 11]))
    np.testing.assert_allclose(cl, [1, 1, 1])


def test_oracle_surface_prunes_exactly():
    m = synth.octahedron_sphere(2)
    s = MO.SurfaceOracle(m.vs, m.faces)
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(40, 3)) * 3.0
    r = s.query(pts)
    for i in range(pts.shape[0]):       # against all faces, no pruning
        d = MO.point_triangles(pts[i], s.A, s.B, s.C)[0]
        assert r["dist"][i] == d.min() and r["face"][i] == int(np.argmin(d))


def test_evaluate_has_no_cpu_path():
    m = synth.torus_mesh(8, 6, masks=False)
    vs, faces = torch.from_numpy(m.vs.astype(np.float32)), torch.from_numpy(m.faces)
    with pytest.raises(SemigcnLibraryError, match="no CPU path"):
        evaluate.Surface(vs, faces)
    with pytest.raises(SemigcnLibraryError):
        evaluate.mesh_distance((vs, faces), (vs, faces), (vs, faces))
    with pytest.raises(SemigcnLibraryError):
        evaluate.simple_mesh_distance(vs, (vs, faces))
