"""semigcn_amd.components on the device against the numpy restatement in tests/components_oracle.py.  Every comparison is
exact: labels, counts and ids equal, positions bit-identical; there is no tolerance anywhere.

Shapes: the hand cases; F = 0, F = 1, degenerate faces only; a 1 x 20 000 strip (one component whose face graph is a path of
40 000: hooks across many waves and blocks, in three face orders); 5 000 interleaved octahedra (many roots, the tie rule);
a cut 96 x 96 torus among fragments, degenerate faces and unreferenced vertices under one permutation; a fan of 64 faces on
one edge; two tori that share one vertex; and the hand-over to fill_holes and prepare_inputs."""
import functools
import json

import numpy as np
import pytest
import torch

import components_oracle as CO
import holes_oracle as HO
from semigcn_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOTH = ("edge", "vertex")


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x)).to(DEV)             # a copy: the shared fixtures are read-only
    return t if dtype is None else t.to(dtype)


def positions(V, seed=0):
    return np.random.default_rng(seed).standard_normal((V, 3)).astype(np.float32)


def check_components(faces, V, connectivity, want=None):
    """face_components on the device equals the oracle; returns the oracle's tuple."""
    from semigcn_amd import components
    want = CO.face_components(faces, V, connectivity) if want is None else want
    got = components.face_components(dev(np.asarray(faces, np.int64).reshape(-1, 3)), V, connectivity)
    assert got.labels.dtype == torch.int64 and got.face_count.dtype == torch.int64
    assert np.array_equal(got.labels.cpu().numpy(), want[0])
    assert np.array_equal(got.face_count.cpu().numpy(), want[1])
    assert (got.largest, got.n_degenerate, len(got)) == (want[2], want[3], want[1].shape[0])
    return want


def check_kept(vs, faces, want=None, **kw):
    """keep_components on the device equals the oracle's five arrays; returns the device result."""
    from semigcn_amd import components
    want = CO.keep_components(vs, faces, **kw) if want is None else want
    got = components.keep_components((dev(vs), dev(faces)), **kw)
    assert got.vs.dtype == torch.float32 and got.faces.dtype == torch.int64 and got.kept.dtype == torch.bool
    assert got.vertex_ids.dtype == torch.int64 and got.face_ids.dtype == torch.int64
    assert tuple(got.vs.shape) == want[0].shape and tuple(got.faces.shape) == want[1].shape
    assert np.array_equal(got.vs.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got.faces.cpu().numpy(), want[1])
    assert np.array_equal(got.vertex_ids.cpu().numpy(), want[2])
    assert np.array_equal(got.face_ids.cpu().numpy(), want[3])
    assert np.array_equal(got.kept.cpu().numpy(), want[4])
    return got


# ---- hand cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", BOTH)
def test_hand_cases(connectivity):
    V, faces = CO.two_tetrahedra_sharing_a_vertex()
    want = check_components(faces, V, connectivity)
    assert want[1].tolist() == ([4, 4] if connectivity == "edge" else [8])
    check_kept(positions(V), faces, connectivity=connectivity)

    V, faces = CO.fan(3)
    assert check_components(faces, V, connectivity)[1].tolist() == [3]

    faces = np.array([[0, 1, 2], [0, 1, 3]], np.int64)                    # the same directed half-edge twice
    assert check_components(faces, 4, connectivity)[1].tolist() == [2]

    faces = np.array([[0, 1, 2], [2, 2, 3], [3, 4, 5], [1, 2, 2]], np.int64)
    want = check_components(faces, 6, connectivity)
    assert want[0].tolist() == [0, -1, 1, -1] and want[3] == 2
    got = check_kept(positions(6), faces, keep="all", connectivity=connectivity)
    assert got.face_ids.cpu().tolist() == [0, 2]

    a, b, c = [[0, 1, 2], [2, 1, 3]], [[4, 5, 6], [6, 5, 7]], [[8, 9, 10], [10, 9, 11]]
    faces = np.array([b[0], c[0], a[0], c[1], a[1], b[1]], np.int64)      # equal sizes: the lower smallest face wins
    want = check_components(faces, 12, connectivity)
    assert want[0].tolist() == [0, 1, 2, 1, 2, 0] and want[2] == 0
    got = check_kept(positions(12), faces, connectivity=connectivity)
    assert got.face_ids.cpu().tolist() == [0, 5] and got.vertex_ids.cpu().tolist() == [4, 5, 6, 7]
    check_kept(positions(12), faces, keep=np.array([0, 1, 1], np.uint8), connectivity=connectivity)
    check_kept(positions(12), faces, keep=np.array([True, True, False]), min_faces=2, connectivity=connectivity)

    faces = np.array([[6, 5, 4], [5, 4, 2], [9, 8, 10]], np.int64)        # vertices 0, 1, 3, 7 are unreferenced
    got = check_kept(positions(11), faces, keep="all", connectivity=connectivity)
    assert got.vertex_ids.cpu().tolist() == [2, 4, 5, 6, 8, 9, 10]
    got = check_kept(positions(11), faces, connectivity=connectivity)
    assert got.vertex_ids.cpu().tolist() == [2, 4, 5, 6] and got.faces.cpu().tolist() == [[3, 2, 1], [2, 1, 0]]


@pytest.mark.parametrize("connectivity", BOTH)
def test_empty_single_and_degenerate_only(connectivity):
    from semigcn_amd import components
    empty = np.zeros((0, 3), np.int64)
    for V in (0, 5):
        want = check_components(empty, V, connectivity)
        assert want[1].shape == (0,) and want[2] == -1
        got = check_kept(positions(V), empty, connectivity=connectivity)
        assert got.vs.shape == (0, 3) and got.faces.shape == (0, 3) and got.kept.numel() == 0
        check_kept(positions(V), empty, keep="all", connectivity=connectivity)
    one = np.array([[4, 2, 3]], np.int64)
    want = check_components(one, 6, connectivity)
    assert want[0].tolist() == [0] and want[1].tolist() == [1] and want[2] == 0
    got = check_kept(positions(6), one, connectivity=connectivity)
    assert got.vertex_ids.cpu().tolist() == [2, 3, 4] and got.faces.cpu().tolist() == [[2, 0, 1]]
    only = np.array([[1, 1, 0], [2, 0, 2], [3, 3, 3]], np.int64)
    want = check_components(only, 4, connectivity)
    assert want[0].tolist() == [-1, -1, -1] and want[1].shape == (0,) and want[2] == -1 and want[3] == 3
    for keep in ("largest", "all"):
        got = check_kept(positions(4), only, keep=keep, connectivity=connectivity)
        assert got.vs.shape[0] == 0 and got.faces.shape[0] == 0
    with pytest.raises(components.SemigcnLibraryError, match="outside"):
        components.face_components(dev(np.array([[0, 1, 6]], np.int64)), 6, connectivity)
    with pytest.raises(ValueError, match="components"):
        components.keep_components((positions(6), one), keep=np.array([True, False]), connectivity=connectivity)


# ---- serpentine strip --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def strip_orders():
    V, faces = CO.strip(20000)
    assert faces.shape == (40000, 3)
    orders = {"natural": faces, "reversed": faces[::-1].copy(), "permuted": faces[np.random.default_rng(314).permutation(40000)]}
    for a in orders.values():
        a.setflags(write=False)
    return V, orders


@pytest.mark.parametrize("order", ["natural", "reversed", "permuted"])
@pytest.mark.parametrize("connectivity", BOTH)
def test_serpentine_strip(connectivity, order):
    """One component whose face graph is a path of 40 000: a union that hooks without finding the roots again splits it."""
    from semigcn_amd import components
    V, orders = strip_orders()
    faces = orders[order]
    got = components.face_components(dev(faces), V, connectivity)
    assert len(got) == 1 and got.largest == 0 and got.n_degenerate == 0
    assert got.face_count.cpu().tolist() == [40000]
    assert int(got.labels.min()) == 0 and int(got.labels.max()) == 0


# ---- many small --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", BOTH)
def test_many_small(connectivity):
    from semigcn_amd import components
    n = 5000
    vs, faces = CO.octahedra(n)
    got = components.face_components(dev(faces), vs.shape[0], connectivity)
    assert len(got) == n and got.largest == 0 and got.n_degenerate == 0
    assert bool((got.face_count == 8).all())
    assert np.array_equal(got.labels.cpu().numpy(), np.tile(np.arange(n), 8))          # canonical: face j n + i is of octahedron i
    none = components.keep_components((vs, faces), keep="all", min_faces=9, connectivity=connectivity)
    assert none.vs.shape == (0, 3) and none.faces.shape == (0, 3) and not bool(none.kept.any())
    first = components.keep_components((vs, faces), keep="largest", connectivity=connectivity)
    assert first.kept.cpu().numpy().nonzero()[0].tolist() == [0]
    assert first.face_ids.cpu().tolist() == [j * n for j in range(8)] and first.vertex_ids.cpu().tolist() == list(range(6))
    assert np.array_equal(first.faces.cpu().numpy(), CO.OCT) and np.array_equal(first.vs.cpu().numpy().view(np.uint32), vs[:6].view(np.uint32))
    every = components.keep_components((vs, faces), keep="all", min_faces=8, connectivity=connectivity)
    assert torch.equal(every.faces, dev(faces)) and torch.equal(every.vs.view(torch.int32), dev(vs).view(torch.int32))


# ---- one large among fragments -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fragments_case():
    """(vs, faces, torus vertices, torus faces, the oracle's keep="largest"): the cut torus of test_gpu_holes.one_large, 50
    octahedra, one floating triangle, three degenerate faces (two of them on torus vertices, one touching a fragment too:
    as links they would join components) and ten unreferenced vertices, under one permutation of faces and vertex ids."""
    import test_gpu_holes as TH
    t_vs, t_faces = TH.one_large()
    V0 = t_vs.shape[0]
    o_vs, o_faces = CO.octahedra(50, interleave=False)
    o_vs = o_vs + np.array([t_vs[:, 0].max() + 3.0, 0.0, 0.0], np.float32)
    tri_vs = np.array([[0, 0, 60], [1, 0, 60], [0, 1, 60]], np.float32)
    V1 = V0 + o_vs.shape[0]
    loose = positions(10, seed=5) + np.float32(100.0)
    vs = np.concatenate([t_vs, o_vs, tri_vs, loose]).astype(np.float32)
    degenerate = np.array([[0, 0, 1], [5, V0 + 2, 5], [V1, V1, V1 + 1]], np.int64)
    faces = np.concatenate([t_faces, V0 + o_faces, [[V1, V1 + 1, V1 + 2]], degenerate])
    rng = np.random.default_rng(2718)
    v_perm, f_perm = rng.permutation(vs.shape[0]), rng.permutation(faces.shape[0])        # old vertex v becomes v_perm[v]
    p_vs = np.empty_like(vs)
    p_vs[v_perm] = vs
    p_faces = np.ascontiguousarray(v_perm[faces][f_perm])
    want = CO.keep_components(p_vs, p_faces)
    for a in (p_vs, p_faces) + want:
        a.setflags(write=False)
    return p_vs, p_faces, V0, t_faces.shape[0], want


@pytest.mark.parametrize("connectivity", BOTH)
def test_one_large_among_fragments(connectivity):
    vs, faces, V0, F0, want = fragments_case()
    comps = check_components(faces, vs.shape[0], connectivity)
    assert comps[1].shape[0] == 52 and comps[3] == 3 and sorted(comps[1].tolist()) == [1] + [8] * 50 + [F0]
    got = check_kept(vs, faces, want=want if connectivity == "edge" else None, connectivity=connectivity)
    assert got.vs.shape[0] == V0 and got.faces.shape[0] == F0
    assert HO.euler_characteristic(got.faces.cpu().numpy()) == HO.euler_characteristic(faces[want[3]])
    every = check_kept(vs, faces, keep="all", connectivity=connectivity)
    assert every.faces.shape[0] == faces.shape[0] - 3 and every.vs.shape[0] == vs.shape[0] - 10
    bad = CO.degenerate(faces)
    assert np.array_equal(every.face_ids.cpu().numpy(), np.nonzero(~bad)[0])
    check_kept(vs, faces, keep="all", min_faces=8, connectivity=connectivity)


def test_determinism():
    from semigcn_amd import components
    vs, faces, _, _, _ = fragments_case()
    f = dev(faces)
    for connectivity in BOTH:
        first = components.face_components(f, vs.shape[0], connectivity)
        for _ in range(4):
            again = components.face_components(f, vs.shape[0], connectivity)
            assert torch.equal(again.labels, first.labels) and torch.equal(again.face_count, first.face_count)
            assert again.largest == first.largest


# ---- non-manifold ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", BOTH)
def test_non_manifold(connectivity):
    V, faces = CO.fan(64)                                   # a run of 64 equal keys in the sort
    want = check_components(faces, V, connectivity)
    assert want[1].tolist() == [64]
    check_kept(positions(V), faces[np.random.default_rng(1).permutation(64)], connectivity=connectivity)

    m = synth.torus_mesh(32, 32, masks=False)
    n = m.num_vertices
    second = m.faces + n
    second[second == n + 7] = 7                             # vertex 7 of the first torus is vertex 7 of the second too
    faces = np.concatenate([m.faces, second]).astype(np.int64)
    want = check_components(faces, 2 * n, connectivity)
    assert want[1].tolist() == ([m.faces.shape[0]] * 2 if connectivity == "edge" else [2 * m.faces.shape[0]])
    vs = np.concatenate([m.vs, m.vs + 100.0]).astype(np.float32)
    got = check_kept(vs, faces, connectivity=connectivity)
    assert got.vs.shape[0] == (n if connectivity == "edge" else 2 * n - 1)      # vertex n + 7 is referenced by no face


# ---- hand-over ---------------------------------------------------------------------------------------------------------
def test_hand_over_to_fill_holes():
    import test_gpu_holes as TH
    from semigcn_amd import components, holes
    vs, faces = TH.planar()
    V = vs.shape[0]
    inner = next(l for l in HO.boundary_loops(faces) if len(l) == 12)
    v = inner[3]
    flake_vs = np.concatenate([vs, vs[v] + np.array([[0.3, 0.1, 1.0], [0.1, 0.3, 1.0]], np.float32)]).astype(np.float32)
    flake = np.concatenate([faces, [[v, V, V + 1]]]).astype(np.int64)
    with pytest.raises(HO.Unorderable) as e:
        HO.boundary_loops(flake)
    assert (e.value.n_repeated, e.value.n_bowtie, e.value.vertex) == (0, 1, v)
    with pytest.raises(ValueError, match=f"vertex {v}$"):
        holes.fill_holes((flake_vs, flake))
    kept = components.keep_components((flake_vs, flake))
    assert len(kept.components) == 2 and kept.components.face_count.cpu().tolist() == [faces.shape[0], 1]
    assert np.array_equal(kept.faces.cpu().numpy(), faces) and np.array_equal(kept.vs.cpu().numpy().view(np.uint32), vs.view(np.uint32))
    assert sorted(len(l) for l in HO.boundary_loops(kept.faces.cpu().numpy())) == [12, 38]
    a = holes.fill_holes((kept.vs, kept.faces), max_hole_edges=12)
    b = holes.fill_holes((vs, faces), max_hole_edges=12)
    assert torch.equal(a.faces, b.faces) and torch.equal(a.vs.view(torch.int32), b.vs.view(torch.int32))
    assert a.filled.cpu().tolist() == b.filled.cpu().tolist() and sum(a.filled.cpu().tolist()) == 1


def test_chain_keep_fill_prepare():
    from semigcn_amd import components, holes, prepare
    vs, faces, V0, F0, _ = fragments_case()
    kept = components.keep_components((vs, faces))
    filled = holes.fill_holes((kept.vs, kept.faces))
    p = prepare.prepare_inputs(initial=(filled.vs, filled.faces), original=(kept.vs, kept.faces))
    g = p.faces.cpu().numpy()
    assert g.shape[0] > F0 and HO.half_edge_stats(g) == (1, 0) and HO.euler_characteristic(g) == 0
    assert p.topology.manifold and bool(torch.isfinite(p.x_pos).all())
    assert bool(p.v_mask[:V0].all())                                   # the kept vertices are the scan's


# ---- plan reuse --------------------------------------------------------------------------------------------------------
def test_plan_reuse():
    from semigcn_amd import components
    vs, faces = CO.octahedra(3)
    more = np.concatenate([faces, [[0, 2, 5]]])                          # one more face on octahedron 0: it is the largest
    first = components.PartsPlan(dev(more), vs.shape[0])
    with pytest.raises(components.SemigcnLibraryError, match="select"):
        first.emit(dev(vs))
    for keep in (np.array([True, False, True]), np.array([False, True, False]), np.array([False, False, False])):
        want = CO.keep_components(vs, more, keep)
        assert first.select(dev(keep)) == (want[0].shape[0], want[1].shape[0])
        got = first.emit(dev(vs))
        assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32))
        for g, w in zip(got[1:], want[1:4]):
            assert np.array_equal(g.cpu().numpy(), w)
    assert (first.num_components, first.largest, first.largest_faces, first.n_degenerate) == (3, 0, 9, 0)
    torch.cuda.synchronize()
    first.close()
    first.close()
    with pytest.raises(components.SemigcnLibraryError, match="closed"):
        first.labels()
    V, other = CO.two_tetrahedra_sharing_a_vertex()
    second = components.PartsPlan(dev(other), V, "vertex")
    labels, count = second.labels()
    assert labels.cpu().tolist() == [0] * 8 and count.cpu().tolist() == [8]
    torch.cuda.synchronize()
    second.close()


# ---- command lines -----------------------------------------------------------------------------------------------------
HOLES_KEYS = ["n_vertices", "n_faces", "n_loops", "n_filled", "n_inserted_vertices", "n_inserted_faces", "fair_steps", "loops_ms",
              "emit_ms", "fair_ms"]


def last_json(capsys):
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_command_lines(tmp_path, capsys):
    from semigcn_amd import components, holes, prepare
    from semigcn_amd.evaluate import read_obj
    t_vs, t_faces = holes.cut_torus(96, 96, 4)
    assert components.main(["--torus", "96", "96", "--cut", "4", "--fragments", "7"]) == 0
    rec = last_json(capsys)
    assert rec["n_components"] == 8 and rec["kept_faces"] == t_faces.shape[0] == rec["largest_faces"]
    assert rec["kept_vertices"] == t_vs.shape[0] and rec["n_degenerate"] == 0
    assert rec["n_vertices"] == t_vs.shape[0] + 42 and rec["n_faces"] == t_faces.shape[0] + 56
    assert all(rec[k] >= 0.0 for k in ("label_ms", "select_ms", "emit_ms"))

    assert holes.main(["--torus", "96", "96", "--cut", "4"]) == 0
    plain = last_json(capsys)
    assert list(plain) == HOLES_KEYS                                      # the keys, in the order the parent commit prints
    assert holes.main(["--torus", "96", "96", "--cut", "4", "--largest-component"]) == 0
    flagged = last_json(capsys)
    assert list(flagged) == HOLES_KEYS + ["n_components", "n_dropped_faces"]
    assert (flagged["n_components"], flagged["n_dropped_faces"]) == (1, 0)
    assert all(flagged[k] == plain[k] for k in HOLES_KEYS if not k.endswith("_ms"))

    vs, faces = CO.octahedra(2, interleave=False)
    faces = np.concatenate([faces, [[0, 2, 5]]])
    scan, dst = str(tmp_path / "a.obj"), str(tmp_path / "b.obj")
    prepare.write_obj(scan, vs, faces)
    assert components.main(["--scan", scan, "--out", dst]) == 0
    rec = last_json(capsys)
    assert (rec["n_components"], rec["largest_faces"], rec["kept_vertices"], rec["kept_faces"]) == (2, 9, 6, 9)
    k_vs, k_faces = read_obj(dst)
    assert np.array_equal(k_faces, faces[[0, 1, 2, 3, 4, 5, 6, 7, 16]]) and np.array_equal(k_vs.view(np.uint32), vs[:6].view(np.uint32))
    assert components.main(["--scan", scan, "--out", dst, "--keep", "all", "--min-faces", "9", "--connectivity", "vertex"]) == 0
    assert last_json(capsys)["kept_faces"] == 9
    with pytest.raises(SystemExit):
        components.main(["--out", dst])
