"""sg_surface_raycast on the device against the rule's numpy restatement (tests/ray_oracle.py): t, face and bary bit for bit,
on every size at which the walk takes another path, and on integer data against exact arithmetic."""
import numpy as np
import pytest
import torch

import ray_fixtures as RF
import ray_oracle as R
from semigcn_amd import synth
from semigcn_amd.capi import SemigcnLibraryError
from semigcn_amd.evaluate import Hits, Surface

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cast(vs, faces, o, d, t_min=0.0, t_max=np.inf, visits_are=None):
    """The device's rows as arrays, with the checks every call must pass: stats[0] == 0 (Surface.ray_cast raises
    otherwise) and a second run that gives identical bytes and leaf visits.  ``visits_are``: what the leaf visits must be."""
    with Surface(torch.from_numpy(vs).to(DEV), torch.from_numpy(faces).to(DEV)) as s:
        h, visits = s.ray_cast(torch.from_numpy(np.ascontiguousarray(o)).to(DEV),
                               torch.from_numpy(np.ascontiguousarray(d)).to(DEV), t_min, t_max, with_visits=True)
        h2 = s.ray_cast(o, d, t_min, t_max)                                       # arrays are taken as well
        assert isinstance(h, Hits) and isinstance(h2, Hits) and s.ray_cast(o, d, t_min, t_max, with_visits=True)[1] == visits
        assert h.t.dtype == torch.float32 and h.face.dtype == torch.int32 and h.bary.shape == (len(o), 2)
        got = tuple(x.cpu().numpy() for x in h)
        for a, b in zip(got, h2):
            assert np.array_equal(RF.bits(a), RF.bits(b.cpu().numpy()))
        assert 0 <= visits and (visits_are is None or visits == visits_are), (visits, visits_are)
    return got


def check(vs, faces, o, d, t_min=0.0, t_max=np.inf, what="", visits_are=None):
    want = R.ray_cast(vs, faces, o, d, t_min, t_max)
    got = cast(vs, faces, o, d, t_min, t_max, visits_are)
    RF.assert_rows_equal(got, want, what)
    return got


@pytest.mark.parametrize("F", [1, 4, 5, 7])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_tiny_trees_and_partial_wavefronts(F, N):
    """a lone leaf (its node holds an empty second child), a full leaf, two leaves, a ragged last leaf.  A lone leaf that
    was walked twice -- through the inverted infinite box of the empty child, which a slab test passes -- would give the same
    rows; the leaf visits tell: exactly one for every ray whose interval meets the leaf's box, none for the others."""
    rng = np.random.default_rng(100 * F + N)
    vs, faces = RF.mesh("sphere")
    faces = faces[:F]
    target = vs[faces].astype(np.float64).mean(1)[rng.integers(0, F, N)] + rng.normal(0, 0.3, (N, 3))
    o = (target * 2.5 + rng.normal(0, 0.2, (N, 3))).astype(np.float32)
    d = (target - o).astype(np.float32)
    o[::7], d[::7] = vs[faces[0, 0]] * 2, -vs[faces[0, 0]]                       # through a vertex
    bound = None
    if F <= 4:                                               # one leaf: the rays whose slab interval reaches its box
        p = vs[faces].reshape(-1, 3)
        ok, tn, tf = R.slab(p.min(0)[:, None], p.max(0)[:, None], o.astype(np.float64).T, d.astype(np.float64).T)
        bound = int((ok & (tn <= tf) & (tf >= 0.0)).sum())
        assert bound <= N
    t, face, _ = check(vs, faces, o, d, what=f"F={F} N={N}", visits_are=bound)
    assert (face != R.NO_FACE).sum() > 0 or N == 1


@pytest.mark.parametrize("inside", [True, False])
def test_sphere_rays_through_vertices_edges_and_centroids(inside):
    vs, faces = RF.mesh("sphere")
    o, d, _ = RF.feature_rays("sphere", inside)
    _, face, _ = check(vs, faces, o, d, what="features")
    assert (face == R.NO_FACE).sum() == 0


def test_torus_rays_through_vertices_edges_and_centroids():
    vs, faces = RF.mesh("torus")
    (v, m, c), _ = RF.feature_targets("torus")
    tg = np.concatenate([v, m, c])
    eye = np.array([3.0, -40.0, 25.0], np.float32)
    _, face, _ = check(vs, faces, np.broadcast_to(eye, tg.shape).copy(), (tg - eye).astype(np.float32), what="torus features")
    assert (face != R.NO_FACE).mean() > 0.9                   # a feature on the silhouette may be missed by its rounded ray
    check(vs, faces, tg, np.broadcast_to(np.array([0, 0, 1], np.float32), tg.shape).copy(), what="torus, origins on the surface")


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_random_rays_zero_components_and_origins_on_vertices(name):
    vs, faces = RF.mesh(name)
    o, d = RF.random_lines(name, 600, seed=1)                                  # 100 with one zero component, 50 with two
    check(vs, faces, o, d, what="random rays")
    check(vs, faces, o, d, -np.inf, np.inf, what="random lines")
    rng = np.random.default_rng(4)
    ov = vs[rng.integers(0, len(vs), 300)]
    dv = rng.normal(size=(300, 3)).astype(np.float32)
    dv[:60, rng.integers(0, 3)] = 0
    dv[60:120] = vs[rng.integers(0, len(vs), 60)] - ov[60:120]                   # from a vertex towards a vertex
    t, face, _ = check(vs, faces, ov, dv, what="origins on vertices")
    assert (t == 0).sum() > 0


def test_the_integer_box_against_exact_arithmetic():
    vs, faces, o, d, exact = RF.int_box()
    got = cast(vs, faces, o, d)
    RF.assert_rows_equal(got, exact, "integer box, exact", zero_sign=False)
    RF.assert_rows_equal(got, R.ray_cast(vs, faces, o, d), "integer box, numpy")


def test_closed_ends_of_the_range():
    vs, faces, o, d, exact = RF.int_box()
    at = np.flatnonzero(exact[0] == 1.5)
    assert len(at) >= 20
    o, d = o[at], d[at]
    for t_min, t_max in ((1.5, np.inf), (0.0, 1.5), (1.5, 1.5)):
        t, face, _ = check(vs, faces, o, d, t_min, t_max, what=f"[{t_min}, {t_max}]")
        assert (t == 1.5).all() and np.array_equal(face, exact[1][at])
    t, face, _ = check(vs, faces, o, d, 0.0, np.nextafter(1.5, 0), what="just short")
    assert (face == R.NO_FACE).all()
    t, face, _ = check(vs, faces, o, d, np.nextafter(1.5, 2), np.inf, what="just past: the far side")
    assert (t > 1.5).all()


@pytest.mark.parametrize("n", [37, 300])
def test_copies_of_one_face(n):
    """equal keys, a deep tree: the lowest id wins"""
    vs, faces = RF.one_face_copies(n)
    o = np.array([[0.5, 0.5, 3], [1, 1, 3], [0, 0, -2], [2, 0, 1], [0.5, 0.5, 0], [5, 5, 5]], np.float32)
    d = np.array([[0, 0, -1], [0, 0, -2], [0, 0, 1], [0, 0, -1], [0.25, 0.25, 0], [1, 0, 0]], np.float32)
    t, face, _ = check(vs, faces, o, d, what=f"{n} copies")
    assert list(face) == [0, 0, 0, 0, R.NO_FACE, R.NO_FACE] and list(t[:4]) == [3.0, 1.5, 2.0, 1.0]


def test_needles_far_from_the_origin():
    vs, faces, o, d = RF.needles()
    e = vs[faces].astype(np.float64)
    aspect = np.linalg.norm(e[:, 2] - e[:, 0], axis=1) / np.linalg.norm(e[:, 1] - e[:, 0], axis=1)
    assert aspect.min() > 5e4 and np.abs(vs).min() > 900
    t, face, _ = check(vs, faces, o, d, what="needles")
    assert (face != R.NO_FACE).sum() > 50


def test_rows_without_a_ray_do_not_disturb_their_neighbours():
    vs, faces = RF.mesh("torus")
    o, d = RF.random_lines("torus", 300, seed=8)
    clean = check(vs, faces, o, d, what="clean")
    bad = np.arange(3, 300, 11)
    o2, d2 = o.copy(), d.copy()
    o2[bad[0::4], 0], o2[bad[1::4], 2], d2[bad[2::4], 1], d2[bad[3::4]] = np.nan, np.inf, -np.inf, 0.0
    t, face, bary = check(vs, faces, o2, d2, what="mixed")
    assert np.isinf(t[bad]).all() and (face[bad] == R.NO_FACE).all() and np.isnan(bary[bad]).all()
    keep = np.setdiff1d(np.arange(300), bad)
    RF.assert_rows_equal((t[keep], face[keep], bary[keep]), tuple(x[keep] for x in clean), "neighbours")


def test_a_shuffled_ray_order_gives_the_same_rows():
    vs, faces = RF.mesh("torus")
    o, d = RF.random_lines("torus", 600, seed=1)
    perm = np.random.default_rng(9).permutation(600)
    a = cast(vs, faces, o, d)
    b = cast(vs, faces, o[perm], d[perm])
    RF.assert_rows_equal(b, tuple(x[perm] for x in a), "shuffled")


def test_a_large_torus_by_properties():
    """2^17 rays on a 200 x 100 torus, where brute force is too slow: the reported face passes the oracle's predicate at the
    reported t, and no face of a brute-forced subset of 2,000 rays beats it."""
    m = synth.torus_mesh(200, 100, masks=False)
    vs, faces = m.vs.astype(np.float32), m.faces
    rng = np.random.default_rng(12)
    N = 1 << 17
    c, r = vs.mean(0), np.abs(vs - vs.mean(0)).max()
    o = (c + rng.uniform(-1.2, 1.2, (N, 3)) * r).astype(np.float32)
    d = rng.normal(size=(N, 3)).astype(np.float32)
    d[:N // 8, rng.integers(0, 3)] = 0
    t, face, bary = cast(vs, faces, o, d)
    hit = np.flatnonzero(face != R.NO_FACE)
    assert 0.2 * N < len(hit) < N and face[hit].min() >= 0 and face[hit].max() < len(faces)
    h, tt, b1, b2 = (x[:, 0] for x in R.hits(vs, faces[face[hit]], o[hit], d[hit], pairwise=True))
    ok = (h & (tt.astype(np.float32) == t[hit]) & (b1.astype(np.float32) == bary[hit, 0])
          & (b2.astype(np.float32) == bary[hit, 1]))
    assert ok.all(), np.flatnonzero(~ok)[:5]
    sub = rng.choice(N, 2000, replace=False)
    RF.assert_rows_equal((t[sub], face[sub], bary[sub]), R.ray_cast_culled(vs, faces, o[sub], d[sub]), "subset")


def test_arguments_the_device_refuses():
    vs, faces = RF.mesh("sphere")
    with Surface(vs, faces) as s:
        o = torch.zeros(4, 3, device=DEV)
        with pytest.raises(ValueError, match="4 origins and 3 directions"):
            s.ray_cast(o, o[:3])
        with pytest.raises(SemigcnLibraryError, match="t_min"):
            s.ray_cast(o, o, 2.0, 1.0)
        with pytest.raises(SemigcnLibraryError, match="t_min"):
            s.ray_cast(o, o, float("nan"), 1.0)
        with pytest.raises(SemigcnLibraryError, match="the surface was built from"):
            s._h.ray_cast(s.vs, s.faces[:5].contiguous(), o, o)
        h = s.ray_cast(o[:0], o[:0])
        assert h.t.shape == (0,) and h.face.shape == (0,) and h.bary.shape == (0, 2)
