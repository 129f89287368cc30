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


def _check_query(surf_vs, surf_faces, pts, ora=None, signed=True, extra=0.0, min_clear=0.0, ref=None):
    """Device query of pts against the surface, checked against the oracle: distance within 1e-5 (d64 + L_max); the
    face wherever the runner-up is farther than that; the sign where the closest point is interior and |d64| > tol.
    ``extra``: a term added to the tolerance (the far-from-the-origin cases alone); ``min_clear``: the least share of
    the points whose face and closest point are checked; ``ora`` / ``ref``: an oracle (of the same triangles, possibly
    under other face indices) and its answer for pts, when the caller has them already."""
    vs32 = np.asarray(surf_vs, np.float32)
    ora = ora or MO.SurfaceOracle(vs32, surf_faces)
    pts32 = np.asarray(pts, np.float32)
    s = evaluate.Surface(_t(vs32), _t(surf_faces, torch.int64))
    d, f, c = s.query(_t(pts32), signed=signed)
    d, f, c = d.cpu().numpy().astype(np.float64), f.cpu().numpy(), c.cpu().numpy().astype(np.float64)
    r = ref or ora.query(pts32)
    assert len(r["dist"]) == len(pts32), (len(r["dist"]), len(pts32))   # a ref handed in belongs to these points
    tol = 1e-5 * (r["dist"] + ora.l_max) + extra
    clear = r["second"] - r["dist"] > tol
    err = np.abs(np.abs(d) - r["dist"])
    cerr = np.abs(c - r["closest"]).max(1)
    assert clear.mean() >= min_clear, clear.mean()
    bad = err > tol
    assert not bad.any(), (f"worst |d - d64| / tol = {(err / tol).max():.3g}, {int(bad.sum())} of {len(bad)} over",
                           np.flatnonzero(bad)[:10], d[bad][:10], r["dist"][bad][:10])
    assert (f[clear] == r["face"][clear]).all(), np.flatnonzero(clear & (f != r["face"]))[:10]
    assert (cerr[clear] <= 4 * tol[clear]).all(), f"worst closest-point error / 4 tol = {(cerr / (4 * tol))[clear].max():.3g}"
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


# ---- thin triangles, far coordinates, small and tied trees, the query's own edges --------------------------------------------
def _rotations(rng, n):
    """n uniformly random rotation matrices [n, 3, 3] (QR of a normal matrix, the determinant made +1)."""
    q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def _needles(rng, n, sin_a, centres, frames=None):
    """n needle triangles, one about each of ``centres`` [n, 3]: the angle at the apex has the sine ``sin_a``, the two
    long edges 0.8 to 1.2: equal in every other group of four (the short edge is then sin_a long and its angles are near
    90 degrees), and unequal in the rest (the three vertices are then nearly collinear, with a second thin angle and one
    near 180 degrees).  Half the faces start at the apex (their e1, e2 are then the nearly parallel pair), a quarter at
    either vertex of the third edge.  ``frames`` [n, 3, 3]: the columns are the needle's axis, its in-plane
    perpendicular and its normal (default: random rotations).  Returns (vs float32 [3 n, 3], faces int64 [n, 3], probes
    [15 n, 3]); the probes are laid out on the float32 triangles (storing a needle in float32 tilts its plane): per needle
    10 inside the prism at the heights 1e-3, 1e-2 and 1e-1 on either side, and 5 outside it, 1e-3 or 1e-2 beyond a
    long edge."""
    rot = _rotations(rng, n) if frames is None else frames
    l1, l2 = rng.uniform(0.8, 1.2, (2, n))
    l2 = np.where(np.arange(n) % 8 >= 4, l1, l2)
    tri = np.zeros((n, 3, 3))
    tri[:, 1, 0] = l1
    tri[:, 2, 0], tri[:, 2, 1] = l2 * np.sqrt(1 - sin_a ** 2), l2 * sin_a
    tri -= tri.mean(1, keepdims=True)
    vs = (np.einsum("nij,nkj->nki", rot, tri) + centres[:, None]).astype(np.float32)
    apex, e = vs[:, 0].astype(np.float64), (vs[:, 1:] - vs[:, :1]).astype(np.float64)
    normal = np.cross(e[:, 0], e[:, 1])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)

    def lifted(k):
        return (rng.choice([1e-3, 1e-2, 1e-1], (n, k, 1)) * rng.choice([-1.0, 1.0], (n, k, 1))) * normal[:, None]

    b = 1 - np.sqrt(rng.uniform(size=(n, 10, 1)))               # uniform over the triangle: most of them far from the apex
    c = (1 - b) * rng.uniform(size=(n, 10, 1))
    inside = apex[:, None] + b * e[:, None, 0] + c * e[:, None, 1] + lifted(10)
    which = rng.integers(0, 2, (n, 5))                          # beyond the edge apex -> vertex 1 or apex -> vertex 2
    edge = np.take_along_axis(e, which[..., None], 1)
    out = np.cross(edge, normal[:, None]) * np.where(which == 0, 1.0, -1.0)[..., None]
    out /= np.linalg.norm(out, axis=2, keepdims=True)
    outside = apex[:, None] + rng.uniform(0.05, 0.95, (n, 5, 1)) * edge + rng.choice([1e-3, 1e-2], (n, 5, 1)) * out + lifted(5)
    start = np.array([0, 0, 1, 2])[np.arange(n) % 4]            # the face's first vertex: the apex for every other needle
    faces = 3 * np.arange(n)[:, None] + (start[:, None] + np.arange(3)) % 3
    return vs.reshape(-1, 3), faces.astype(np.int64), np.concatenate([inside, outside], 1).reshape(-1, 3)


SLIVER_SINES = [1e-2, 1e-3, 1e-4, 3e-5, 2e-5, 5e-6]     # 2e-5: just above the kernel's zero-area threshold; 5e-6: below it


def _isolated_needles(sin_a, n=200):
    """Needles on a jittered grid, 5 lengths apart: every probe's runner-up face is lengths away."""
    rng = np.random.default_rng(int(round(1e7 * sin_a)))
    g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(216)[:n]]
    return _needles(rng, n, sin_a, 5.0 * (g - 2.5) + rng.uniform(-0.5, 0.5, (n, 3)))


def _needles_on_torus(sin_a, n=200):
    """torus_mesh(40, 20) plus needles as extra faces on extra vertices, lying 0.5 above the surface in its tangent
    plane: the Morton order puts them into leaves with ordinary faces.  Probes: the needles' and 401 around the torus."""
    rng = np.random.default_rng(int(round(1e7 * sin_a)) + 1)
    m = synth.torus_mesh(40, 20, masks=False)
    at = rng.permutation(m.num_vertices)[:n]
    th, ph = 2 * np.pi * (at // 20) / 40, 2 * np.pi * (at % 20) / 20
    normal = np.stack([np.cos(ph) * np.cos(th), np.cos(ph) * np.sin(th), np.sin(ph)], 1)
    t1 = np.stack([-np.sin(th), np.cos(th), np.zeros(n)], 1)
    spin = rng.uniform(0, 2 * np.pi, (n, 1))
    axis = np.cos(spin) * t1 + np.sin(spin) * np.cross(normal, t1)
    frames = np.stack([axis, np.cross(normal, axis), normal], 2)
    nvs, nfaces, probes = _needles(rng, n, sin_a, m.vs[at] + 0.5 * normal, frames)
    vs = np.concatenate([m.vs.astype(np.float32), nvs])
    faces = np.concatenate([m.faces, nfaces + m.num_vertices])
    around = _probe_points(m.vs, m.faces, rng, 300)            # 300 near, every 8th of those on vertices and edges, the far ones
    return vs, faces, np.concatenate([probes, around[:300], around[300:700:8], around[700:]])


@pytest.mark.parametrize("form", ["isolated", "on_torus"])
@pytest.mark.parametrize("sin_a", SLIVER_SINES)
def test_sliver_band(sin_a, form):
    """Needle triangles down to and below the zero-area threshold, at the tolerance of every other case.  Measured on an
    MI355X, worst |d - d64| / tol for the sines 1e-2, 1e-3, 1e-4, 3e-5, 2e-5, 5e-6: with the normal in float32 (before)
    0.17, 1.1, 11, 56, 71, 13 isolated and 0.066, 0.69, 8.3, 27, 36, 15 on the torus (and the closest point off by more
    than 4 tol from 1e-2 on); with the normal in float64 below 0.001 isolated and 0.012 on the torus at every sine."""
    vs, faces, probes = _isolated_needles(sin_a) if form == "isolated" else _needles_on_torus(sin_a)
    _check_query(vs, faces, probes, signed=True, min_clear=0.9)


@pytest.mark.parametrize("shift", [(1e3, -2e3, 5e2), (1e5, 1e5, 1e5)])
@pytest.mark.parametrize("kind", ["sphere", "torus"])
def test_query_far_from_the_origin(kind, shift):
    """The local-frame claim of csrc/mesh_dist.hip: the cases of test_query_matches_oracle, vertices and probes translated
    in float32, the oracle built from the translated float32 arrays.  One term is added to the tolerance, for the
    rounding of p - a and of the stored closest point: 8 * 2^-23 * max |coordinate| (the bound of test_gpu_remesh.py).
    At the first shift that term is 0.002 and at least half the probes keep their face, closest-point and sign checks; at
    (1e5, 1e5, 1e5) it is 0.095 on a surface of unit edges, 7 % of the probes stay clear, and the case checks little more
    than the distance."""
    rng = np.random.default_rng(11)
    m = synth.octahedron_sphere(4) if kind == "sphere" else synth.torus_mesh(100, 50)
    t = np.asarray(shift, np.float32)
    vs = m.vs.astype(np.float32) + t
    pts = _probe_points(m.vs, m.faces, rng).astype(np.float32) + t
    extra = 8 * 2.0 ** -23 * float(np.abs(vs).max())
    _check_query(vs, m.faces, pts, signed=True, extra=extra, min_clear=0.5 if shift[0] == 1e3 else 0.0)


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 7, 8, 9, 12, 13])
def test_small_trees(F):
    """One to four leaves of kLeaf = 4 faces, the last one partial or full; F <= 4 is the lone-leaf node with its empty
    second box, F = 5 ... 8 the smallest Karras tree."""
    m = synth.octahedron_sphere(1)
    faces = m.faces[:F]
    rng = np.random.default_rng(100 + F)
    pts = _probe_points(m.vs, faces, rng, 300)
    pts = pts[rng.permutation(len(pts))[:300]]
    ora = MO.SurfaceOracle(m.vs.astype(np.float32), faces)
    ref = ora.query(pts.astype(np.float32))
    _check_query(m.vs, faces, pts, ora=ora, ref=ref, signed=True)
    if F == 1:
        _check_query(m.vs, faces, pts, ora=ora, ref=ref, signed=False)
        tri = m.vs[faces[0]]
        u = rng.normal(size=(20, 3))
        far = tri.mean(0) + 100 * np.linalg.norm(tri.max(0) - tri.min(0)) * u / np.linalg.norm(u, axis=1, keepdims=True)
        d, f, _, r = _check_query(m.vs, faces, far, ora=ora, min_clear=1.0)
        assert (f == 0).all() and np.allclose(np.abs(d), r["dist"], rtol=1e-5, atol=0)


def _dyadic_triangles(rng, n, rotated):
    """n triangles [n, 3, 3] whose vertices sum to zero exactly, in float32 as well: coordinates are multiples of 1/64
    and c = -(a + b).  ``rotated``: copies of one triangle turned about its centroid (rounded to the grid); else random."""
    if rotated:
        ab = np.einsum("nij,kj->nki", _rotations(rng, n), np.array([[1.5, 0.25, 0.0], [-0.5, 1.25, 0.0]]))
    else:
        ab = rng.uniform(-2, 2, (n, 2, 3)) * rng.uniform(0.1, 1, (n, 1, 1))
    ab = np.round(ab * 64) / 64
    return np.concatenate([ab, -ab.sum(1, keepdims=True)], 1)


@pytest.mark.parametrize("case", ["fan64", "line", "same33"])
def test_constant_morton_codes(case):
    """Centroids that coincide exactly (the same float32 sum for every face) or lie on a line: the centroid box has
    three or two zero extents, the Morton part of the keys is constant in them and the tree rests on the face index."""
    rng = np.random.default_rng({"fan64": 64, "line": 2, "same33": 33}[case])
    if case == "fan64":
        tri = _dyadic_triangles(rng, 64, rotated=True)
    elif case == "same33":
        tri = _dyadic_triangles(rng, 33, rotated=False) + np.array([3.0, -2.0, 1.5])
    else:
        tri = _dyadic_triangles(rng, 41, rotated=False)
        tri[:, :, 0] += 0.5 * rng.permutation(41)[:, None]
    vs = tri.reshape(-1, 3)
    faces = np.arange(len(vs), dtype=np.int64).reshape(-1, 3)
    v32 = vs.astype(np.float32)
    assert (v32 == vs).all()
    cent = (v32[faces[:, 0]] + v32[faces[:, 1]] + v32[faces[:, 2]]) * np.float32(1 / 3)     # as face_keys sums them
    assert (np.ptp(cent, 0) == 0).sum() == (2 if case == "line" else 3)
    pts = _probe_points(vs, faces, rng, 600)
    _check_query(vs, faces, pts, signed=True)


def test_duplicate_faces_lowest_index():
    """Every triangle twice, at k and 2 F - 1 - k: the two distances are the same bits, and the face is the lower index,
    whether the pair shares a leaf or not.  The oracle is that of the single surface: its face is the lower index, and
    its runner-up is over the geometrically different faces."""
    m = synth.torus_mesh(30, 20, masks=False)
    F = len(m.faces)
    twice = np.concatenate([m.faces, m.faces[::-1]])
    pts = _probe_points(m.vs, m.faces, np.random.default_rng(6), 1500)
    ora = MO.SurfaceOracle(m.vs.astype(np.float32), m.faces)
    d, f, c, r = _check_query(m.vs, twice, pts, ora=ora, min_clear=0.5)
    clear = r["second"] - r["dist"] > 1e-5 * (r["dist"] + ora.l_max)
    assert (f[clear] < F).all() and (f[clear] == r["face"][clear]).all()
    assert (f < F).all()               # where the oracle cannot name the face: still the lower index of the pair that won


def test_query_sizes():
    m = synth.torus_mesh(40, 20, masks=False)
    pts = _t(_probe_points(m.vs, m.faces, np.random.default_rng(8), 3549))
    assert pts.shape[0] == 4000
    s = evaluate.Surface(m)
    whole = s.query(pts)
    for n in (1, 63, 64, 65, 129):
        for lo in (0, 1777):
            part = s.query(pts[lo:lo + n].clone())
            for x, y in zip(whole, part):
                assert torch.equal(x[lo:lo + n], y), (n, lo)
    d, f, c = s.query(pts[:0])
    assert (d.shape, f.shape, c.shape) == ((0,), (0,), (0, 3))
    assert (d.dtype, f.dtype, c.dtype) == (torch.float32, torch.int32, torch.float32)
    assert d.device == pts.device and f.device == pts.device and c.device == pts.device


def test_non_finite_probes():
    """A point with a NaN or an infinite coordinate has no distance: its row is (inf, 0x7fffffff, nan nan nan), signed or
    not, and the other rows are the bits they are without it.  The callers: scan_mask says False for it, the metric
    carries the inf into hd_all, and remesh refuses non-finite vertices before it queries (test_gpu_remesh.py)."""
    from semigcn_amd import prepare
    m = synth.torus_mesh(40, 20, masks=False)
    clean = _probe_points(m.vs, m.faces, np.random.default_rng(9), 49).astype(np.float32)
    assert len(clean) == 500
    dirty = clean.copy()
    dirty[3, 1] = np.nan
    dirty[77, 0] = np.inf
    rows = [3, 77]
    others = np.setdiff1d(np.arange(500), rows)
    s = evaluate.Surface(m)
    for signed in (True, False):
        a, b = s.query(_t(clean), signed=signed), s.query(_t(dirty), signed=signed)
        for x, y in zip(a, b):
            assert torch.equal(x[others], y[others])
        d, f, c = (x.cpu().numpy() for x in b)
        assert (d[rows] == np.inf).all() and (f[rows] == 0x7fffffff).all() and np.isnan(c[rows]).all()
        assert np.isfinite(d[others]).all() and (f[others] < len(m.faces)).all() and np.isfinite(c[others]).all()
    on_scan = prepare.scan_mask(_t(dirty), s, eps=1e30).cpu().numpy()
    assert not on_scan[rows].any() and on_scan[others].all()
    assert evaluate.simple_mesh_distance(_t(np.where(np.isnan(dirty), np.nan, clean)), s) == np.inf
