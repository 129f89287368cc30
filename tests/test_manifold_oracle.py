"""tests/manifold_oracle.py against answers computed by hand, the two invariants of the cut on seeded random soups, and the
premises of the fixtures tests/test_gpu_manifold.py compares the device against (what each of them is meant to contain, and
|vol6| > 1e-6 sum |term| wherever the outward step decides something).  No device."""
import numpy as np
import pytest

import holes_oracle as HO
import manifold_oracle as MO


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def counts(r):
    return {k: getattr(r, k) for k in MO.COUNTS}


def test_two_tetrahedra_sharing_a_vertex():
    vs, f = MO.two_tetrahedra_sharing_a_vertex()
    r = MO.make_manifold(vs, f)
    assert vs.shape[0] == 7 and r.vs.shape[0] == 8 and r.n_split_vertices == 1
    assert (r.n_components, r.n_closed, r.n_nonmanifold_edges, r.n_flipped) == (2, 2, 0, 0)
    assert r.vertex_ids.tolist() == [0, 1, 2, 3, 3, 4, 5, 6] and same_bits(r.vs, vs[r.vertex_ids])
    assert r.faces[:4].tolist() == MO.TET.tolist() and r.faces[4:].tolist() == (np.array([4, 5, 6, 7])[MO.TET]).tolist()
    assert MO.volume_is_decided(r) and all(v > 0 for v in r.vol6.values())


def test_two_tetrahedra_sharing_an_edge():
    vs, f = MO.two_tetrahedra_sharing_an_edge()
    r = MO.make_manifold(vs, f)
    assert vs.shape[0] == 6 and r.vs.shape[0] == 8 and r.n_split_vertices == 2 and r.n_nonmanifold_edges == 1
    assert (r.n_components, r.n_closed) == (2, 2) and r.vertex_ids.tolist() == [0, 0, 1, 1, 2, 3, 4, 5]
    assert MO.max_faces_per_edge(r.faces) == 2 and MO.volume_is_decided(r)


def test_three_faces_on_one_edge():
    vs, f = MO.fan(3)
    r = MO.make_manifold(vs, f)
    assert vs.shape[0] == 5 and r.vs.shape[0] == 9 and (r.n_components, r.n_closed, r.n_nonmanifold_edges) == (3, 0, 1)
    assert r.faces.tolist() == [[0, 3, 6], [4, 1, 7], [2, 5, 8]] and r.n_flipped == 0      # three faces, each its own smallest


def test_octahedron_with_a_fin():
    vs, f = MO.octahedron_with_fin()
    r = MO.make_manifold(vs, f)
    assert (r.n_components, r.n_closed, r.n_nonmanifold_edges, r.n_split_vertices) == (2, 1, 1, 2)
    assert set(r.faces[8].tolist()).isdisjoint(r.faces[:8].reshape(-1).tolist())           # the fin is alone
    assert HO.half_edge_stats(r.faces[:8]) == (1, 0)                                        # the octahedron is closed
    assert r.vs.shape[0] == 9 and MO.volume_is_decided(r) and r.n_flipped == 0


def test_one_face_three_times():
    vs = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    r = MO.make_manifold(vs, np.array([[1, 2, 0], [0, 1, 2], [2, 1, 0]]))
    assert r.faces.tolist() == [[1, 2, 0]] and r.face_ids.tolist() == [0] and r.n_duplicate_faces == 2
    r = MO.weld_vertices(vs, np.array([[1, 2, 0], [0, 2, 1], [1, 1, 2]]))
    assert r.faces.tolist() == [[1, 2, 0]] and (r.n_duplicate_faces, r.n_degenerate) == (1, 1)
    assert MO.split_nonmanifold(vs, np.array([[1, 2, 0], [0, 2, 1]])).faces.shape[0] == 2   # the cut alone keeps duplicates


def test_negative_zero_welds_with_zero():
    vs = np.array([[0.0, 1, 2], [-0.0, 1, 2], [3, -0.0, 0.0], [3, 0.0, -0.0], [1, 1, 1], [np.nan, 0, 0], [np.nan, 0, 0]], np.float32)
    assert MO.weld_map(vs).tolist() == [0, 0, 2, 2, 4, 5, 5]                               # bit-identical NaNs coincide
    r = MO.weld_vertices(vs, np.array([[0, 2, 4], [1, 4, 3]]))
    # welded, the second face is the first one reflected
    assert r.faces.tolist() == [[0, 1, 2]] and r.vertex_ids.tolist() == [0, 2, 4] and (r.n_welded, r.n_duplicate_faces) == (3, 1)
    assert r.vertex_map.tolist() == [0, 0, 2, 2, 4, 5, 5]


def test_moebius_strip():
    vs, f = MO.moebius(16)
    assert f.shape == (32, 3) and HO.half_edge_stats(f)[0] == 2                             # one seam runs the same way twice
    r = MO.make_manifold(vs, f)
    assert r.n_nonorientable == 1 and r.nonorientable.all() and np.array_equal(r.faces, f) and r.n_flipped == 0
    assert same_bits(r.vs, vs) and (r.n_components, r.n_closed) == (1, 0)
    vs, f = MO.moebius_and_cube()
    r = MO.make_manifold(vs, f)
    assert (r.n_components, r.n_nonorientable, r.n_closed) == (2, 1, 1) and r.nonorientable.tolist() == [True] * 32 + [False] * 12
    assert MO.volume_is_decided(r) and np.array_equal(r.faces, f)


def test_clean_meshes_come_back_as_they_are():
    for vs, f in (MO.torus(24, 16), MO.cube(), MO.patch(4)):
        for r in (MO.weld_vertices(vs, f), MO.split_nonmanifold(vs, f), MO.orient_faces(vs, f), MO.make_manifold(vs, f)):
            assert same_bits(r.vs, vs) and np.array_equal(r.faces, f) and MO.volume_is_decided(r)
            assert all(v == 0 for k, v in counts(r).items() if k not in ("n_components", "n_closed"))
    r = MO.make_manifold(*MO.torus(24, 16))
    assert (r.n_components, r.n_closed) == (1, 1) and r.vol6[0] > 0


def test_empty_and_degenerate_only():
    vs = np.zeros((3, 3), np.float32)
    r = MO.make_manifold(vs, np.zeros((0, 3), np.int64))
    assert r.vs.shape == (0, 3) and r.faces.shape == (0, 3) and r.vertex_map.tolist() == [0, 1, 2]
    assert MO.orient_faces(vs, np.zeros((0, 3), np.int64)).vs.shape == (3, 3)
    r = MO.make_manifold(np.arange(9, dtype=np.float32).reshape(3, 3), np.array([[0, 0, 1], [2, 1, 2]]))
    assert r.vs.shape == (0, 3) and r.faces.shape == (0, 3) and r.n_degenerate == 2 and r.n_components == 0
    r = MO.orient_faces(np.arange(9, dtype=np.float32).reshape(3, 3), np.array([[0, 0, 1], [0, 1, 2]]))
    assert r.faces.tolist() == [[0, 0, 1], [0, 1, 2]] and (r.n_degenerate, r.n_components) == (1, 1)
    with pytest.raises(ValueError):
        MO.make_manifold(vs, np.array([[0, 1, 3]]))


def test_the_cut_leaves_two_faces_per_edge_and_one_fan_per_vertex():
    rng = np.random.default_rng(2024)
    n_cut = 0
    for _ in range(3000):
        V, F = int(rng.integers(4, 9)), int(rng.integers(1, 14))
        vs, f = rng.standard_normal((V, 3)).astype(np.float32), rng.integers(0, V, (F, 3))
        r = MO.make_manifold(vs, f)
        assert MO.max_faces_per_edge(r.faces) <= 2 and MO.every_vertex_is_one_fan(r.faces)
        assert (np.diff(r.vertex_ids) >= 0).all() and (np.diff(r.face_ids) > 0).all()
        assert r.faces.shape[0] == F - r.n_degenerate - r.n_duplicate_faces                 # the cut deletes no face
        orientable = ~r.nonorientable
        if orientable.any():
            assert HO.half_edge_stats(r.faces[orientable])[0] == 1
        s = MO.split_nonmanifold(vs, f)
        assert MO.max_faces_per_edge(s.faces) <= 2 and MO.every_vertex_is_one_fan(s.faces)
        n_cut += r.n_nonmanifold_edges > 0
    assert n_cut > 300                                                                    # the soups do hold what is cut


# ---- the premises of the device fixtures ---------------------------------------------------------------------------------
def test_premises_soup():
    vs, f = MO.soup_torus()
    assert vs.shape == (3 * 768, 3) and np.unique(f).shape[0] == 3 * 768
    r = MO.make_manifold(vs, f)
    assert r.vs.shape[0] == 384 and r.n_welded == 3 * 768 - 384 and (r.n_components, r.n_closed) == (1, 1)
    assert MO.volume_is_decided(r) and HO.half_edge_stats(r.faces) == (1, 0)
    neg = MO.negative_zeros(vs, 21)
    changed = neg.view(np.uint32) != vs.view(np.uint32)
    assert changed.sum() >= 24 and np.array_equal(neg, vs)                                  # other bits, equal values
    assert len({tuple(row) for row in neg.view(np.uint32).tolist()}) > 384                  # copies of one vertex now differ
    n = MO.make_manifold(neg, f)
    assert np.array_equal(n.faces, r.faces) and np.array_equal(n.vertex_ids, r.vertex_ids) and counts(n) == counts(r)


def test_premises_orient():
    vs, f = MO.half_reversed_torus()
    assert HO.half_edge_stats(f)[0] == 2
    r = MO.orient_faces(vs, f)
    assert 300 < r.n_flipped < 468 and HO.half_edge_stats(r.faces) == (1, 0) and MO.volume_is_decided(r)
    assert MO.run(vs, r.faces, orient=True, outward=True).vol6[0] > 0
    r = MO.orient_faces(*MO.cube(inverted=True))
    assert r.flipped.all() and MO.volume_is_decided(r)
    r = MO.orient_faces(*MO.patch(4, inverted=True))
    assert not r.flipped.any() and r.n_closed == 0
    for order in range(3):
        vs, f = MO.zigzag_strip(order)
        r = MO.orient_faces(vs, f)
        assert f.shape[0] == 40000 and r.n_components == 1 and r.n_flipped == 20000 and not r.flipped[0]
        assert HO.half_edge_stats(r.faces)[0] == 1
    vs, f = MO.reversed_octahedra()
    r = MO.orient_faces(vs, f)
    assert (r.n_components, r.n_closed) == (5000, 5000) and MO.volume_is_decided(r) and 10000 < r.n_flipped < 14000
    assert HO.half_edge_stats(r.faces) == (1, 0)
    t = MO.orient_faces(vs, f, outward=False)                   # the topological rule alone: the smallest face stays
    assert not t.flipped[:5000].any() and t.n_flipped != r.n_flipped


def test_premises_cut():
    vs, f = MO.cut_fixture()
    r = MO.make_manifold(vs, f)
    assert r.n_nonmanifold_edges == 1 + 24 and r.n_nonorientable == 0 and r.n_degenerate == r.n_duplicate_faces == 0
    # 8 bow-ties, 63 more copies of each end of the fan's edge, three more of each of the ring's 24 vertices
    assert r.n_split_vertices == 8 + 2 * 63 + 3 * 24
    assert r.n_components == 1 + 64 + 2 and r.n_closed == 1 and MO.volume_is_decided(r)
    assert MO.max_faces_per_edge(r.faces) == 2 and MO.every_vertex_is_one_fan(r.faces) and HO.half_edge_stats(r.faces)[0] == 1
    HO.boundary_loops(r.faces)                                                             # orderable
