"""The device closest-point query and the scoring metric (semigcn_amd.evaluate, csrc/mesh_dist.hip) against the float64
oracle of tests/mesh_distance_oracle.py -- the reference's check/dist_check.py:13-67 with pymeshlab's
distance_from_reference_mesh replaced by an exact query (rules: INTEGRATION.md section 5)."""
import numpy as np
import pytest
import torch

import mesh_distance_oracle as MO
from semigcn_amd import evaluate, meshprep, synth, train
from semigcn_amd.capi import SemigcnLibraryError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device=DEV, dtype=dtype)


def _check_query(surf_vs, surf_faces, pts, ora=None, signed=True):
    """Device query of pts against the surface, checked against the oracle: distance within 1e-5 (d64 + L_max); the
    face wherever the runner-up is farther than that; the sign where the closest point is interior and |d64| > tol."""
    vs32 = np.asarray(surf_vs, np.float32)
    ora = ora or MO.SurfaceOracle(vs32, surf_faces)
    pts32 = np.asarray(pts, np.float32)
    s = evaluate.Surface(_t(vs32), _t(surf_faces, torch.int64))
    d, f, c = s.query(_t(pts32), signed=signed)
    d, f, c = d.cpu().numpy().astype(np.float64), f.cpu().numpy(), c.cpu().numpy().astype(np.float64)
    r = ora.query(pts32)
    tol = 1e-5 * (r["dist"] + ora.l_max)
    bad = np.abs(np.abs(d) - r["dist"]) > tol
    assert not bad.any(), (np.flatnonzero(bad)[:10], d[bad][:10], r["dist"][bad][:10])
    clear = r["second"] - r["dist"] > tol
    assert (f[clear] == r["face"][clear]).all(), np.flatnonzero(clear & (f != r["face"]))[:10]
    assert (np.abs(c - r["closest"]).max(1)[clear] <= 4 * tol[clear]).all()
    if signed:
        sgn = clear & r["inside"] & (r["dist"] > tol)
        assert (np.sign(d[sgn]) == np.sign(r["signed"][sgn])).all()
    else:
        assert (d >= 0).all()
    return d, f, c, r


def _probe_points(vs, faces, rng, n_near=1500):
    vs = np.asarray(vs, np.float64)
    diag = np.linalg.norm(vs.max(0) - vs.min(0))
    near = vs[rng.integers(0, len(vs), n_near)] + rng.normal(0, 0.3, (n_near, 3))
    on_v = vs[rng.integers(0, len(vs), 200)]
    fe = faces[rng.integers(0, len(faces), 200)]
    on_e = 0.5 * (vs[fe[:, 0]] + vs[fe[:, 1]])
    centre = vs.mean(0, keepdims=True)
    u = rng.normal(size=(50, 3))
    far = centre + 100 * diag * u / np.linalg.norm(u, axis=1, keepdims=True)
    return np.concatenate([near, on_v, on_e, centre, far])


def _holed(m):
    """m's surface with the faces of its v_mask holes removed (org, util/datamaker.py:156-159): open boundaries."""
    topo = meshprep.MeshTopology(m.faces, m.num_vertices, DEV, with_f2f=False)
    keep = meshprep.vmask_to_fmask(topo, torch.from_numpy(m.v_mask)).cpu().numpy()
    assert 0 < keep.sum() < len(keep)
    return m.faces[keep]


@pytest.mark.parametrize("kind", ["sphere", "torus", "open_torus"])
def test_query_matches_oracle(kind):
    rng = np.random.default_rng(11)
    m = synth.octahedron_sphere(4) if kind == "sphere" else synth.torus_mesh(100, 50)
    faces = _holed(m) if kind == "open_torus" else m.faces
    pts = _probe_points(m.vs, faces, rng)
    _check_query(m.vs, faces, pts, signed=True)
    _check_query(m.vs, faces, pts[:300], signed=False)


def test_degenerate_triangles_and_invalid_faces():
    vs = np.array([[0, 0, 0], [4, 0, 0], [2, 0, 0],          # collinear: the segment [0, 4] on x
                   [0, 50, 0], [0, 52, 0],                   # repeated vertex: a segment on y
                   [90, 90, 90],                             # one point three times
                   [200, 0, 0], [202, 0, 0], [200, 2, 0]], np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 3], [5, 5, 5], [6, 7, 8]], np.int64)
    pts = np.array([[1, 3, 4], [7, 4, 0], [3, 51, 4], [0, 55, 0], [90, 90, 95], [200.5, 0.5, -3], [202, -1, 0]],
                   np.float32)
    d, f, c, r = _check_query(vs, faces, pts)
    np.testing.assert_allclose(np.abs(d), [5, 5, 5, 3, 5, 3, 1], rtol=1e-6)
    assert list(f) == [0, 0, 1, 1, 2, 3, 3]
    assert (d[:5] >= 0).all()                                  # zero-area faces have no normal: the sign is +
    # an index of V: SG_ERR_INVALID, and the process stays healthy
    bad = faces.copy()
    bad[2, 1] = len(vs)
    with pytest.raises(SemigcnLibraryError, match="outside"):
        evaluate.Surface(_t(vs), _t(bad, torch.int64))
    with pytest.raises(SemigcnLibraryError, match="at least one face"):
        evaluate.Surface(_t(vs), torch.zeros((0, 3), dtype=torch.int64, device=DEV))
    d2 = evaluate.Surface(_t(vs), _t(faces, torch.int64)).query(_t(pts))[0]
    assert torch.equal(d2.cpu(), torch.from_numpy(d.astype(np.float32)))


def test_bit_identical_and_order_independent():
    m = synth.torus_mesh(100, 50)
    rng = np.random.default_rng(3)
    pts = _t(_probe_points(m.vs, m.faces, rng, 4000))
    s = evaluate.Surface(m)
    a = s.query(pts)
    b = s.query(pts)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    perm = torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(1)).to(DEV)
    p = s.query(pts[perm])
    inv = torch.argsort(perm)
    for x, y in zip(a, p):
        assert torch.equal(x, y[inv])


def _noisy_torus(nu, nv, sigma, seed):
    o = synth.torus_mesh(nu, nv, masks=False, seed=seed)
    return (o.vs + np.random.default_rng(seed).normal(0, sigma, o.vs.shape)).astype(np.float32), o.faces


def test_metric_against_float64_oracle():
    m = synth.torus_mesh(100, 50)
    gt_vs, gt_f = m.vs.astype(np.float32), m.faces
    org_f = _holed(m)
    out_vs, out_f = _noisy_torus(96, 50, 0.03, 21)     # same torus, another triangulation
    res = evaluate.mesh_distance((gt_vs, gt_f), (gt_vs, org_f), (out_vs, out_f))
    ref = MO.mesh_distance(gt_vs, gt_f, gt_vs, org_f, out_vs, out_f, eps=0.05)
    lmax = MO.SurfaceOracle(gt_vs, org_f).l_max
    tol = 1e-5 * (np.abs(ref["q_org"]) + lmax)
    sure = np.abs(ref["q_org"] - 0.05) > tol
    hole = res["hole"].cpu().numpy()
    assert hole.dtype == bool and (hole[sure] == ref["hole"][sure]).all() and 0 < res["n_hole"] < len(gt_vs)
    assert abs(res["hd_all"] - ref["hd_all"]) < 2e-6 and abs(res["hd_hole"] - ref["hd_hole"]) < 2e-6
    assert res["diag"] == pytest.approx(ref["diag"], rel=1e-12)
    assert res["q"].shape == (len(gt_vs),) and res["q_out"].shape == (len(out_vs),)
    # real=True: EPS = 1.0 (check/dist_check.py:37-38)
    res_r = evaluate.mesh_distance((gt_vs, gt_f), (gt_vs, org_f), (out_vs, out_f), real=True)
    sure_r = np.abs(ref["q_org"] - 1.0) > tol
    assert (res_r["hole"].cpu().numpy()[sure_r] == (ref["q_org"] > 1.0)[sure_r]).all()
    assert res_r["n_hole"] < res["n_hole"]
    # many results against one gt: the hole mask of a first call, org not needed
    res_b = evaluate.mesh_distance((gt_vs, gt_f), None, (out_vs, out_f), hole=res["hole"])
    assert res_b["hd_all"] == res["hd_all"] and res_b["hd_hole"] == res["hd_hole"]
    # no hole at all: hd_hole is nan, as the reference's 0 / 0
    res0 = evaluate.mesh_distance((gt_vs, gt_f), (gt_vs, gt_f), (out_vs, out_f))
    assert res0["n_hole"] == 0 and np.isnan(res0["hd_hole"]) and res0["hd_all"] == res["hd_all"]
    assert evaluate.simple_mesh_distance((gt_vs, gt_f), (out_vs, out_f)) == res["hd_all"]


def test_metric_translated_flat_patch():
    n, t = 40, 0.37
    u, v = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    vs = np.stack([u.ravel(), v.ravel(), np.zeros(n * n)], 1).astype(np.float32)
    a = (u[:-1, :-1] * n + v[:-1, :-1]).ravel()
    faces = np.concatenate([np.stack([a, a + n, a + n + 1], 1), np.stack([a, a + n + 1, a + 1], 1)]).astype(np.int64)
    moved = vs + np.float32(t) * np.array([0, 0, 1], np.float32)
    res = evaluate.mesh_distance((vs, faces), (vs, faces), (moved, faces), hole=np.zeros(n * n, bool))
    q = res["q"].cpu().numpy()
    interior = ((u > 0) & (u < n - 1) & (v > 0) & (v < n - 1)).ravel()
    np.testing.assert_allclose(np.abs(q[interior]), t, rtol=1e-6)
    diag = np.linalg.norm(vs.max(0) - vs.min(0))
    assert res["hd_all"] == pytest.approx(t / diag, rel=1e-6)


@pytest.mark.parametrize("nu,nv,nq", [(1000, 1000, 980), (2000, 2000, 1990)])
def test_scale(nu, nv, nq):
    """c4 (1 M vertices, 2 M triangles) and 4 M vertices / 8 M triangles: every vertex of a second, noisy torus of
    another resolution is queried; a seeded sample of 4096 is checked against the oracle."""
    m = synth.torus_mesh(nu, nv, masks=False)
    q_vs, _ = _noisy_torus(nq, nv, 0.05, 7)
    s = evaluate.Surface(m)
    d, f, c = s.query(_t(q_vs))
    idx = np.random.default_rng(4096).choice(len(q_vs), 4096, replace=False)
    ora = MO.SurfaceOracle(m.vs.astype(np.float32), m.faces)
    r = ora.query(q_vs[idx])
    dd, ff = d.cpu().numpy()[idx].astype(np.float64), f.cpu().numpy()[idx]
    tol = 1e-5 * (r["dist"] + ora.l_max)
    assert (np.abs(np.abs(dd) - r["dist"]) <= tol).all()
    clear = r["second"] - r["dist"] > tol
    assert (ff[clear] == r["face"][clear]).all()


def test_end_to_end_sgcn_output():
    """A few SGCNTrainer iterations on a holed 100 x 50 torus, the eval forward with dm = v_mask (sgcn.py:186-188),
    scored: the metric equals the float64 oracle's on the same positions."""
    from semigcn_amd.networks import SingleScaleGCN
    m = synth.torus_mesh(100, 50)
    V = m.num_vertices
    faces = torch.from_numpy(m.faces).to(DEV)
    target = torch.from_numpy(m.vs.astype(np.float32)).to(DEV)
    v_keep = torch.from_numpy(m.v_mask.astype(np.float32)).view(-1, 1).to(DEV)
    f_keep = v_keep[faces[:, 0]] * v_keep[faces[:, 1]] * v_keep[faces[:, 2]]
    dms = torch.from_numpy(synth.make_dummy_masks(m.edge_index, V, dm_size=4, k=3, p=0.014, seed=317)).to(DEV)

    class Data:
        z1 = torch.from_numpy(m.z1).to(DEV).requires_grad_(True)
        x_pos = torch.from_numpy(m.x_pos).to(DEV)
        edge_index = torch.from_numpy(m.edge_index).to(DEV)

    torch.manual_seed(0)
    net = SingleScaleGCN(DEV).to(DEV)
    tr = train.SGCNTrainer(net, train.MeshBatch(Data, faces, target, train.face_normals(target, faces), v_keep, f_keep, dms))
    for _ in range(5):
        tr.iteration_step()
    net.eval()
    with torch.no_grad():
        out_pos = net(Data, torch.from_numpy(m.v_mask).to(DEV).reshape(-1, 1).float()).float().contiguous()
    assert torch.isfinite(out_pos).all()
    gt_vs = m.vs.astype(np.float32)
    org_f = _holed(m)
    res = evaluate.mesh_distance((gt_vs, m.faces), (gt_vs, org_f), (out_pos, faces))
    ref = MO.mesh_distance(gt_vs, m.faces, gt_vs, org_f, out_pos.cpu().numpy(), m.faces, eps=0.05)
    assert res["n_hole"] > 0
    assert abs(res["hd_all"] - ref["hd_all"]) < 2e-6 and abs(res["hd_hole"] - ref["hd_hole"]) < 2e-6
