"""semigcn_amd.manifold on the device against the numpy restatement in tests/manifold_oracle.py.  Every comparison is exact:
ids, flags and counts equal, positions bit-identical; there is no tolerance anywhere.  The premises of the fixtures (what
each contains, and that the outward step decides away from zero) are pinned without a device in
tests/test_manifold_oracle.py; the one fixture that is built on the device (``holes.cut_torus``) asserts them here.

Shapes: the hand cases; F = 0, F = 1, degenerate faces only; a 24 x 16 torus as a permuted soup, also with -0.0; the same
torus half reversed, an inverted cube and an inverted open patch; a 1 x 20 000 strip with every second face reversed (a path
of 40 000 links in the double cover: hooks across many blocks, in three face orders); 5 000 interleaved octahedra (many
roots, the smallest-face rule); the Moebius strip; a 96 x 96 torus with 8 pinches beside a fan of 64 faces and two tori
that share a ring; and everything at once on a cut 48 x 32 torus, through repair and prepare."""
import functools

import numpy as np
import pytest
import torch

import holes_oracle as HO
import manifold_oracle as MO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ARRAYS = ("faces", "vertex_map", "vertex_ids", "face_ids", "flipped", "nonorientable")
FUNCTIONS = ("weld_vertices", "split_nonmanifold", "orient_faces", "make_manifold")


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)           # a copy: the shared fixtures are read-only


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(name, vs, faces, want=None, **kw):
    """``manifold.<name>`` on the device equals the oracle in every array and count; returns (device result, oracle's)."""
    from semigcn_amd import manifold
    want = getattr(MO, name)(vs, faces, **kw) if want is None else want
    got = getattr(manifold, name)((dev(vs), dev(np.asarray(faces, np.int64).reshape(-1, 3))), **kw)
    assert got.vs.dtype == torch.float32 and got.flipped.dtype == torch.bool and got.nonorientable.dtype == torch.bool
    assert tuple(got.vs.shape) == want.vs.shape and np.array_equal(bits(got.vs), bits(want.vs))
    for a in ARRAYS:
        g, w = getattr(got, a), getattr(want, a)
        assert (g.dtype == torch.bool) == (w.dtype == bool) and (g.dtype == torch.bool or g.dtype == torch.int64), a
        assert tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w), a
    assert got.counts() == {k: getattr(want, k) for k in MO.COUNTS}
    return got, want


@functools.lru_cache(maxsize=None)
def oracle_of(fixture, name="make_manifold", *args):
    mesh = getattr(MO, fixture)(*args)
    return mesh, getattr(MO, name)(*mesh)


# ---- sizes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["two_tetrahedra_sharing_a_vertex", "two_tetrahedra_sharing_an_edge", "octahedron_with_fin",
                                  "moebius", "moebius_and_cube"])
def test_hand_cases(mesh):
    vs, f = getattr(MO, mesh)()
    for name in FUNCTIONS:
        check(name, vs, f)
    check("make_manifold", vs, f, weld=False, outward=False)


def test_fans():
    for n in (3, 64):
        for name in FUNCTIONS:
            check(name, *MO.fan(n))


def test_small_sizes():
    vs = np.random.default_rng(0).standard_normal((5, 3)).astype(np.float32)
    for name in FUNCTIONS:
        got, _ = check(name, vs, np.zeros((0, 3), np.int64))                       # F = 0
        assert got.faces.shape == (0, 3) and got.vs.shape[0] == (5 if name == "orient_faces" else 0)
        check(name, vs, np.array([[4, 0, 2]]))                                      # F = 1
        check(name, vs, np.array([[1, 1, 0], [2, 0, 2], [3, 3, 3]]))                # degenerate faces only
        check(name, vs, np.array([[1, 1, 0], [0, 1, 2], [2, 1, 0], [4, 2, 1]]))     # degenerate, duplicate and plain
    check("make_manifold", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))


def test_duplicates_and_negative_zero():
    vs = np.array([[0.0, 1, 2], [-0.0, 1, 2], [3, -0.0, 0.0], [3, 0.0, -0.0], [1, 1, 1], [np.nan, 0, 0], [np.nan, 0, 0]], np.float32)
    f = np.array([[0, 2, 4], [1, 4, 3], [5, 0, 2], [6, 1, 3], [4, 3, 0]])
    got, want = check("weld_vertices", vs, f)
    assert want.vertex_map.tolist() == [0, 0, 2, 2, 4, 5, 5] and want.n_duplicate_faces == 3
    check("make_manifold", vs, f)
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    got, _ = check("make_manifold", tri, np.array([[1, 2, 0], [0, 1, 2], [2, 1, 0]]))
    assert got.faces.tolist() == [[1, 2, 0]] and got.n_duplicate_faces == 2


# ---- soup ------------------------------------------------------------------------------------------------------------------
def test_soup_welds_back():
    (vs, f), want = oracle_of("soup_torus")
    got, _ = check("make_manifold", vs, f, want)
    assert got.vs.shape[0] == 384 and got.n_welded == 3 * 768 - 384
    check("weld_vertices", vs, f)
    neg, _ = check("make_manifold", MO.negative_zeros(vs, 21), f)
    assert torch.equal(neg.faces, got.faces) and torch.equal(neg.vertex_ids, got.vertex_ids) and neg.counts() == got.counts()


# ---- orient ----------------------------------------------------------------------------------------------------------------
def test_half_reversed_torus():
    (vs, f), want = oracle_of("half_reversed_torus", "orient_faces")
    got, _ = check("orient_faces", vs, f, want)
    out = got.faces.cpu().numpy()
    assert HO.half_edge_stats(out) == (1, 0)
    assert MO.orient_faces(vs, out).vol6[0] > 0 and torch.equal(got.vs, dev(vs))
    check("orient_faces", vs, f, outward=False)
    check("make_manifold", vs, f)


def test_inverted_cube_and_patch():
    got, _ = check("orient_faces", *MO.cube(inverted=True))
    assert bool(got.flipped.all()) and np.array_equal(got.faces.cpu().numpy(), MO.cube()[1])
    got, _ = check("orient_faces", *MO.cube(inverted=True), outward=False)
    assert not bool(got.flipped.any())
    got, _ = check("orient_faces", *MO.patch(4, inverted=True))
    assert not bool(got.flipped.any())


@pytest.mark.parametrize("order", [0, 1, 2])
def test_zigzag_strip(order):
    (vs, f), want = oracle_of("zigzag_strip", "orient_faces", order)
    got, _ = check("orient_faces", vs, f, want)
    assert got.n_components == 1 and got.n_flipped == 20000 and not bool(got.flipped[0])


def test_interleaved_octahedra():
    (vs, f), want = oracle_of("reversed_octahedra", "orient_faces")
    got, _ = check("orient_faces", vs, f, want)
    assert (got.n_components, got.n_closed) == (5000, 5000)
    got, _ = check("orient_faces", vs, f, outward=False)
    assert not bool(got.flipped[:5000].any())                                       # every smallest face stays


# ---- cut -------------------------------------------------------------------------------------------------------------------
def test_cut_and_hand_over():
    from semigcn_amd import capi, holes
    (vs, f), want = oracle_of("cut_fixture")
    got, _ = check("make_manifold", vs, f, want)
    check("split_nonmanifold", vs, f)
    loops = holes.boundary_loops(got.faces, got.vs.shape[0])                        # does not raise
    assert len(loops) == len(HO.boundary_loops(want.faces))
    with capi.RemeshPlan(got.vs, got.faces) as plan:
        assert plan.n_nonmanifold == 0 and plan.n_misoriented == 0
    with capi.RemeshPlan(dev(vs), dev(f)) as plan:                                  # the input is what remesh refuses
        assert plan.n_nonmanifold > 0


# ---- whole -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def whole_fixture():
    """A cut 48 x 32 torus with 4 pinches and three octahedra beside it, a seeded third of the faces reversed, degenerate and
    duplicate faces appended, the first half of the faces written as a soup (the indexed half is still one piece, so that
    ``repair`` has a component to refuse), under one permutation."""
    from semigcn_amd import components, holes
    t_vs, t_f = holes.cut_torus(48, 32, 6)
    used_before = t_vs.shape[0]
    t_vs, t_f = components.with_fragments(t_vs, t_f, 3)
    vs, f = t_vs.cpu().numpy(), t_f.cpu().numpy()
    full = np.flatnonzero(np.bincount(f.reshape(-1), minlength=vs.shape[0])[:used_before] == 6)    # interior vertices
    pairs = [(int(full[(k * full.shape[0]) // 8]), int(full[(k * full.shape[0]) // 8 + full.shape[0] // 2])) for k in range(4)]
    f = MO.pinched(f, pairs)
    rng = np.random.default_rng(31)
    f = MO.reversed_faces(f, rng.random(f.shape[0]) < 1 / 3)
    f = np.concatenate([f, f[rng.permutation(f.shape[0])[:20]][:, [2, 0, 1]], f[:10, [1, 0, 2]],
                        np.stack([f[:15, 0], f[:15, 1], f[:15, 0]], 1)])
    return MO.permuted(*MO.partial_soup(vs, f, f.shape[0] // 2), seed=32)


def test_whole():
    from semigcn_amd import manifold
    vs, f = whole_fixture()
    want = MO.make_manifold(vs, f)
    assert want.n_split_vertices == 4 and want.n_duplicate_faces == 30 and want.n_degenerate == 15 and want.n_welded > 0
    assert (want.n_components, want.n_closed, want.n_nonorientable) == (4, 3, 0) and want.n_flipped > 100
    assert MO.volume_is_decided(want)
    got, _ = check("make_manifold", vs, f, want)
    again = manifold.make_manifold((dev(vs), dev(f)))
    for a in ("vs",) + ARRAYS:
        x, y = getattr(got, a), getattr(again, a)
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), a
    assert again.counts() == got.counts()
    check("make_manifold", vs, f, weld=False)                                       # the soup stays a soup


def test_whole_through_repair_and_prepare():
    from semigcn_amd import manifold, prepare, repair
    vs, f = whole_fixture()
    mesh = (dev(vs), dev(f))
    with pytest.raises(ValueError):
        repair.repair(mesh)
    out_vs, out_faces, report = repair.repair(mesh, make_manifold=True)
    assert report.remaining == 0 and HO.half_edge_stats(out_faces.cpu().numpy()) == (1, 0)
    ids = report.vertex_ids.cpu().numpy()
    old = ids >= 0
    assert old.sum() > 1000 and ids.max() < vs.shape[0]
    assert np.array_equal(bits(out_vs)[old], bits(vs)[ids[old]])
    assert MO.orient_faces(out_vs.cpu().numpy(), out_faces.cpu().numpy()).n_flipped == 0     # closed, and outward
    first = manifold.make_manifold(mesh)
    p = prepare.prepare_inputs(initial=(out_vs, out_faces), original=(first.vs, first.faces))
    assert p.topology.manifold and bool(torch.isfinite(p.x_pos).all())


# ---- identity and errors ---------------------------------------------------------------------------------------------------
def test_a_clean_mesh_comes_back_as_it_is():
    vs, f = MO.torus(24, 16)
    for name in FUNCTIONS:
        got, _ = check(name, vs, f)
        assert np.array_equal(bits(got.vs), bits(vs)) and np.array_equal(got.faces.cpu().numpy(), f)
        assert all(v == 0 for k, v in got.counts().items() if k not in ("n_components", "n_closed"))
        assert got.vertex_ids.tolist() == list(range(384)) and got.face_ids.tolist() == list(range(768))


def test_errors():
    from semigcn_amd import manifold
    from semigcn_amd.capi import SemigcnLibraryError
    vs, f = MO.cube()
    for name in FUNCTIONS:
        fn = getattr(manifold, name)
        with pytest.raises(SemigcnLibraryError):
            fn((torch.from_numpy(vs), torch.from_numpy(f)))
        for bad in (8, -1):
            g = f.copy()
            g[5, 1] = bad
            with pytest.raises(SemigcnLibraryError, match="outside"):
                fn((dev(vs), dev(g)))
    plan = manifold.ManifoldPlan(dev(vs), dev(f))
    plan.close()
    with pytest.raises(SemigcnLibraryError, match="closed"):
        plan.export(dev(vs))
    got = manifold.make_manifold((vs, f), timings=True)                             # numpy in, and the stage times
    assert set(got.stage_ms) == {"manifold_ms", "export_ms"} and got.n_closed == 1
