"""The numpy restatement of the registration rule (tests/align_oracle.py) against itself and against the float64
closest-point oracle: the Cayley form, inverses, the normal equations against a dense J^T J, the whole loop on the fixtures."""
import math

import numpy as np
import pytest

import align_fixtures as AF
import align_oracle as AO
import mesh_distance_oracle as MO
from semigcn_amd import align


def test_cayley_is_a_rotation():
    rng = np.random.default_rng(5)
    omegas = [np.zeros(3), np.array([1.0, 0, 0]), np.array([0.6, -0.6, 0.52])] + [rng.uniform(-1, 1, 3) for _ in range(50)]
    for omega in omegas:
        omega = omega / max(1.0, np.linalg.norm(omega))               # |omega| up to 1
        for R in (AO.cayley(omega), align.cayley(omega)):
            assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1.0) <= 1e-14
        assert np.array_equal(AO.cayley(omega), align.cayley(omega))
    # first order: a rotation by |omega| about omega
    w = np.array([1e-4, -2e-4, 3e-4])
    x = np.array([0.3, 0.7, -0.2])
    assert np.abs(AO.cayley(w) @ x - (x + np.cross(w, x))).max() < 1e-7


def test_an_alignment_composed_with_its_inverse_is_the_identity():
    for seed in (None, 1, 2, 3):
        for ws in (True, False):
            S = AF.similarity(seed, ws)
            inv = align.inverse(S)
            assert np.abs(inv @ S - np.eye(4)).max() <= 1e-15 and np.abs(S @ inv - np.eye(4)).max() <= 1e-15
            assert np.array_equal(inv[3], [0, 0, 0, 1])
    assert np.array_equal(align.similarity(), np.eye(4))
    S = align.random_similarity(4, extent=8.0)
    assert np.array_equal(S, align.random_similarity(4, extent=8.0)) and abs(np.cbrt(np.linalg.det(S[:3, :3])) - 1) <= 0.08
    assert abs(np.linalg.det(align.random_similarity(4, False)[:3, :3]) - 1.0) <= 1e-14


@pytest.mark.parametrize("with_scale", [False, True])
def test_accumulate_equals_a_dense_product(with_scale):
    vs, faces = AF.lumpy_torus()
    so = MO.SurfaceOracle(vs, faces)
    rng = np.random.default_rng(11)
    pts = (vs[rng.integers(0, len(vs), 300)] + rng.normal(0, 0.2, (300, 3))).astype(np.float32)
    pts[7] = np.nan
    S = AF.similarity(2, with_scale)
    dist, face, closest = AO.oracle_query(so)(AO.transform(S, pts))
    face[9] = AO.NO_FACE
    md = float(np.median(dist[np.isfinite(dist)]))
    out, sabs = AO.accumulate(vs, faces, pts, S, closest, face, dist, md, with_scale, with_abs=True)
    q = AO.rows(vs, faces, pts, S, closest, face, dist, md, with_scale)
    assert (out[37], out[38], out[39]) == (q["used"].sum(), q["far"].sum(), 2) and out[37] + out[38] + out[39] == 300
    assert 100 < out[37] < 200 and q["skipped"][7] and q["skipped"][9]
    J, r, d = q["J"], q["r"], q["d"]
    A, g = J.T @ J, J.T @ r
    n = int(out[37])
    for k, (i, j) in enumerate(AO.TRIU):
        assert abs(out[k] - A[i, j]) <= (n + 16) * 2.0 ** -52 * sabs[k]
    for j in range(7):
        assert abs(out[28 + j] - g[j]) <= (n + 16) * 2.0 ** -52 * sabs[28 + j]
    assert abs(out[35] - r @ r) <= n * 2.0 ** -52 * sabs[35] and abs(out[36] - d @ d) <= n * 2.0 ** -52 * sabs[36]
    if not with_scale:
        assert not J[:, 6].any() and not out[[6, 12, 17, 21, 24, 26, 27, 34]].any()
    else:
        assert J[:, 6].any()
    # everything rejected: the sums are 0, the count is in out[38]
    out0 = AO.accumulate(vs, faces, pts, S, closest, face, dist, -1.0, with_scale)
    assert not out0[:38].any() and out0[38] == 298 and out0[39] == 2


@pytest.mark.parametrize("with_scale", [True, False])
def test_loop_recovers_the_similarity(with_scale):
    vs, faces = AF.lumpy_torus()
    assert vs.shape == (200, 3) and faces.shape == (400, 3)
    S = AF.similarity(None, with_scale)
    src = AF.moved(S, vs)
    r = AO.align_loop(src, vs, faces, AO.oracle_query(MO.SurfaceOracle(vs, faces)), with_scale=with_scale)
    err = float(np.linalg.norm(AO.transform(r["matrix"], src).astype(np.float64) - vs, axis=1).max())
    merr = float(np.abs(r["matrix"] @ S - np.eye(4)).max())
    print(f"with_scale={with_scale}: {r['iterations']} iterations, rms {[h['rms'] for h in r['history']]}, "
          f"point error E_o = {err:.3e}, matrix error {merr:.3e}")
    assert r["converged"] and r["reason"] == "converged" and r["iterations"] <= 6
    assert r["history"][-1]["step"] <= 1e-6 and r["history"][-1]["n_used"] == 200
    # E_O is this run's own figure where it was recorded; another LAPACK may round the 7 x 7 solve differently, which
    # moves single float32 roundings of the moved points: the bound here is the one the device gets
    assert err <= 4 * AF.E_O and merr <= 1e-6


def test_flat_grid_is_degenerate():
    vs, faces = AF.flat_grid()
    assert vs.shape == (36, 3)
    S = AF.similarity(None, False)
    r = AO.align_loop(AF.moved(S, vs), vs, faces, AO.oracle_query(MO.SurfaceOracle(vs, faces)))
    assert r["reason"] == "degenerate" and not r["converged"] and r["iterations"] == 1
    assert np.array_equal(r["matrix"], np.eye(4)) and math.isnan(r["history"][0]["step"])
    # too few rows is degenerate too, whatever they are
    tv, tf = AF.tetrahedron()
    r = AO.align_loop(tv[:3], tv, tf, AO.oracle_query(MO.SurfaceOracle(tv, tf)))
    assert r["reason"] == "degenerate" and np.array_equal(r["matrix"], np.eye(4))


def test_host_step_of_the_package_is_the_oracle_s():
    vs, faces = AF.lumpy_torus()
    S = AF.similarity(3, True)
    src = AF.moved(S, vs)
    dist, face, closest = AO.oracle_query(MO.SurfaceOracle(vs, faces))(src)
    for ws in (False, True):
        out = AO.accumulate(vs, faces, src, np.eye(4), closest, face, dist, math.inf, ws)
        a = AO.host_step(out, np.eye(3), np.zeros(3), ws, 7.5)
        b = align._host_step(out, np.eye(3), np.zeros(3), ws, 7.5)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert align._host_step(np.zeros(40), np.eye(3), np.zeros(3), False, 1.0) is None


def test_fixtures():
    vs, faces = AF.lumpy_torus()
    cut = AF.cut_faces(vs, faces)
    assert len(cut) == 280 and set(map(tuple, cut)) <= set(map(tuple, faces))
    # one patch: the removed faces are connected through shared edges
    gone = [f for f in faces.tolist() if tuple(f) not in set(map(tuple, cut))]
    seen, todo = {0}, [0]
    edges = [set(map(frozenset, ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])))) for f in gone]
    while todo:
        i = todo.pop()
        for j in range(len(gone)):
            if j not in seen and edges[i] & edges[j]:
                seen.add(j)
                todo.append(j)
    assert len(seen) == len(gone) == 120
    assert len(AF.without_ring(faces, 57)) == 394
    tv, tf = AF.tetrahedron()
    c = tv.mean(0)
    for f in tf:                                                    # outward
        assert np.dot(np.cross(tv[f[1]] - tv[f[0]], tv[f[2]] - tv[f[0]]), tv[f[0]] - c) > 0
