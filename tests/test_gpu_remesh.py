"""semigcn_amd.remesh on the device against the numpy restatement in tests/remesh_oracle.py.  Every comparison with the
oracle is exact: positions bit-identical, faces, parents and round counts equal.  The one bound is "on the surface":
``Surface.query`` distance <= 8 * 2^-23 * max |coordinate|, the float32 rounding of a midpoint and of the query.

Shapes: the hand cases (F = 1, 2, 4, 8); an open 8 x 8 grid of integer coordinates (ties in len2, border edges); the
level-3 octahedron sphere; the stretched 20 x 12 and 40 x 30 tori (the latter: 7 200 half-edges, 29 workgroups of 256, and
buffers that grow several times); 50 and 500 random flips on the regular 40 x 30 torus; the pipeline and the hand-over to
prepare_inputs and repair; a filled cut torus; and a stretched 200 x 200 torus for the invariants alone."""
import functools

import numpy as np
import pytest
import torch

import intersect_oracle as IO
import remesh_oracle as RO
from semigcn_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x)).to(DEV)             # a copy: the shared fixtures are read-only
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.cpu().numpy()


def surface_bound(vs):
    return 8 * 2.0 ** -23 * float(np.abs(np.asarray(vs)).max())


def len2_all(vs, faces):
    """len2 of every half-edge's edge as the module defines it: float32, one rounding per operation, left to right."""
    vs, faces = np.asarray(vs, np.float32), np.asarray(faces)
    a, b = faces.reshape(-1), faces[:, [1, 2, 0]].reshape(-1)
    d = vs[np.maximum(a, b)] - vs[np.minimum(a, b)]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def half_edge_counts(faces, V):
    """(every directed half-edge once, V - E + F over the used vertices, border-vertex flags) with numpy sorts."""
    f = np.asarray(faces, np.int64)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    directed = a * V + b
    und, cnt = np.unique(np.minimum(a, b) * V + np.maximum(a, b), return_counts=True)
    border = np.zeros(V, bool)
    border[und[cnt == 1] // V] = True
    border[und[cnt == 1] % V] = True
    return np.unique(directed).shape[0] == directed.shape[0] and cnt.max() <= 2, np.unique(f).shape[0] - und.shape[0] + f.shape[0], border


# ---- fixtures: (vs, faces, target), and the oracle's answer computed once --------------------------------------------------
def _with_median_target(vs, faces):
    return vs, faces, 0.6 * RO.median_edge(vs, faces)


SPLIT_CASES = {
    "one_triangle": lambda: RO.one_triangle() + (1.0,),
    "two_triangles": lambda: RO.two_triangles() + (3.0,),
    "grid8": lambda: RO.grid(8) + (0.6,),
    "sphere3": lambda: _with_median_target(synth.octahedron_sphere(3).vs.astype(np.float32), synth.octahedron_sphere(3).faces),
    "torus20x12": lambda: _with_median_target(*RO.stretched_torus(20, 12)),
    "torus40x30": lambda: _with_median_target(*RO.stretched_torus(40, 30)),
}


@functools.lru_cache(maxsize=None)
def split_case(name):
    vs, faces, target = SPLIT_CASES[name]()
    return vs, faces, target, RO.split_long_edges(vs, faces, target)


@functools.lru_cache(maxsize=None)
def regular_torus():
    m = synth.torus_mesh(40, 30, flip_frac=0.0, jitter=0.0, masks=False)
    return m.vs.astype(np.float32), m.faces.astype(np.int64)


@functools.lru_cache(maxsize=None)
def flipped_torus(n_flips):
    vs, faces = regular_torus()
    if n_flips:
        faces = synth.random_edge_flips(faces, vs.astype(np.float64), n_flips, np.random.default_rng(7 + n_flips))
    return vs, faces, RO.flip_edges(vs, faces)


def device_split(vs, faces, target, **kw):
    from semigcn_amd import remesh
    d_vs, d_faces = dev(vs, torch.float32), dev(faces)
    keep = (d_vs.clone(), d_faces.clone())
    got = remesh.split_long_edges(d_vs, d_faces, target, **kw)
    assert torch.equal(d_vs, keep[0]) and torch.equal(d_faces, keep[1])
    assert got.vs.dtype == torch.float32 and got.faces.dtype == torch.int64 and got.parents.dtype == torch.int64
    return got


def device_flip(vs, faces, **kw):
    from semigcn_amd import remesh
    d_vs, d_faces = dev(vs, torch.float32), dev(faces)
    keep = d_faces.clone()
    got = remesh.flip_edges(d_vs, d_faces, **kw)
    assert torch.equal(d_faces, keep) and got.faces.dtype == torch.int64 and tuple(got.faces.shape) == tuple(keep.shape)
    return got


# ---- split ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SPLIT_CASES))
def test_split_equals_the_oracle(name):
    vs, faces, target, (w_vs, w_faces, w_parents, w_counts, w_long) = split_case(name)
    got = device_split(vs, faces, target)
    print(name, "rounds", got.counts, "V", got.vs.shape[0], "F", got.faces.shape[0])
    assert got.counts == w_counts and got.n_long == w_long == 0
    assert tuple(got.vs.shape) == w_vs.shape and tuple(got.faces.shape) == w_faces.shape
    assert np.array_equal(host(got.vs).view(np.uint32), w_vs.view(np.uint32))
    assert np.array_equal(host(got.faces), w_faces)
    assert np.array_equal(host(got.parents), w_parents)
    if name == "torus40x30":
        assert 3 * faces.shape[0] == 7200 and len(w_counts) > 4


@pytest.mark.parametrize("name", sorted(SPLIT_CASES))
def test_split_invariants(name):
    from semigcn_amd import evaluate, remesh
    vs, faces, target, _ = split_case(name)
    got = device_split(vs, faces, target)
    V0, V1 = vs.shape[0], got.vs.shape[0]
    g_vs, g_faces = host(got.vs), host(got.faces)
    once0, euler0, border0 = half_edge_counts(faces, V0)
    once1, euler1, border1 = half_edge_counts(g_faces, V1)
    assert once0 and once1 and euler1 == euler0
    assert border1[:V0][border0].all() and border1[:V0].sum() == border0.sum()
    assert got.n_long == 0 and len2_all(g_vs, g_faces).max() <= np.float32(remesh.split_threshold(target))
    assert np.array_equal(g_vs[:V0].view(np.uint32), vs.view(np.uint32))
    surf = evaluate.Surface(dev(vs, torch.float32), dev(faces))
    dist = surf.query(got.vs[V0:], signed=False)[0]
    print(name, "inserted", V1 - V0, "max distance", float(dist.max()), "bound", surface_bound(vs))
    assert float(dist.max()) <= surface_bound(vs)
    surf.close()


def test_split_round_cap_is_reported_not_raised():
    vs, faces, target, (_, _, _, w_counts, _) = split_case("torus20x12")
    for cap in (0, 1, 3):
        want = RO.split_long_edges(vs, faces, target, max_rounds=cap)
        got = device_split(vs, faces, target, max_rounds=cap)
        assert got.counts == want[3] == w_counts[:cap] and got.n_long == want[4] > 0
        assert np.array_equal(host(got.faces), want[1]) and np.array_equal(host(got.vs).view(np.uint32), want[0].view(np.uint32))


# ---- flip -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_flips", [0, 50, 500])
def test_flip_equals_the_oracle_on_the_torus(n_flips):
    vs, faces, (w_faces, w_flips, w_before, w_after, trail) = flipped_torus(n_flips)
    got = device_flip(vs, faces)
    print(n_flips, "flips per round", got.flips, "deviation", got.deviation_before, "->", got.deviation_after)
    assert got.flips == w_flips and (got.deviation_before, got.deviation_after) == (w_before, w_after)
    assert np.array_equal(host(got.faces), w_faces)
    if n_flips == 0:
        assert got.flips == [] and got.deviation_before == 0 and np.array_equal(host(got.faces), faces)
    else:
        # 50 flips lie apart and are undone in one round; 500 interact and take several
        assert len(w_flips) >= (1 if n_flips == 50 else 2) and all(b < a for a, b in zip(trail, trail[1:]))
        # the deviation after every round, from the device: stop after k rounds and look
        for k in range(1, len(w_flips)):
            part = device_flip(vs, faces, max_rounds=k)
            assert part.flips == w_flips[:k] and part.deviation_after == trail[k] < trail[k - 1]
        assert half_edge_counts(host(got.faces), vs.shape[0])[:2] == (True, 0)


@pytest.mark.parametrize("name", ["fan8", "fan8_pulled", "tetrahedron"])
def test_flip_hand_cases(name):
    vs, faces = {"fan8": RO.fan8, "fan8_pulled": lambda: RO.fan8(pulled=True), "tetrahedron": RO.tetrahedron}[name]()
    w_faces, w_flips, w_before, w_after, _ = RO.flip_edges(vs, faces)
    got = device_flip(vs, faces)
    assert got.flips == w_flips and (got.deviation_before, got.deviation_after) == (w_before, w_after)
    assert np.array_equal(host(got.faces), w_faces)
    if name == "tetrahedron":
        assert got.flips == [] and np.array_equal(host(got.faces), faces)
    else:
        # the conflict: eight candidates of gain 2 share the hub; one flips in round 1, another is re-evaluated in round 2
        assert got.flips == [1, 1] and (w_before, w_after) == (10, 6)
        first = device_flip(vs, faces, max_rounds=1)
        assert first.flips == [1] and np.array_equal(host(first.faces), RO.flip_round(vs, faces)[0])
    if name == "fan8_pulled":                              # the guard: spoke {0, 1} is never the one that goes
        table = RO.edge_table(host(got.faces))[0]
        assert (0, 1) in table and (2, 8) not in table


# ---- rejections -------------------------------------------------------------------------------------------------------------
def _bad_inputs():
    vs, faces = RO.tetrahedron()
    more = np.concatenate([vs, [[1, 1, 1]]]).astype(np.float32)
    nan = vs.copy()
    nan[2, 1] = np.nan
    return {"three faces": (more, np.concatenate([faces, [[0, 1, 4]]]), r"1 edge\(s\) with three or more faces.*edge \(0, 1\)"),
            "misoriented": (vs, np.concatenate([faces[:3], faces[3:, ::-1]]), r"3 edge\(s\) whose two faces run"),
            "degenerate": (vs, np.concatenate([faces, [[2, 2, 3]]]), r"1 face\(s\) with a repeated vertex \(smallest 4\)"),
            "nan": (nan, faces, r"1 vertex/vertices with a non-finite coordinate \(smallest 2\)")}


@pytest.mark.parametrize("name", sorted(_bad_inputs()))
def test_invalid_input_raises_and_leaves_the_input_alone(name):
    from semigcn_amd import remesh
    vs, faces, pattern = _bad_inputs()[name]
    with pytest.raises(ValueError):
        RO.check_input(vs, faces)
    d_vs, d_faces = dev(vs, torch.float32), dev(faces)
    keep = (d_vs.clone(), d_faces.clone())
    for call in (lambda: remesh.split_long_edges(d_vs, d_faces, 0.5), lambda: remesh.flip_edges(d_vs, d_faces),
                 lambda: remesh.refine_mesh((d_vs, d_faces), target=0.5),
                 lambda: remesh.relax_project(d_vs, d_faces, (d_vs, d_faces))):
        with pytest.raises(ValueError, match=pattern):
            call()
    assert np.array_equal(host(d_vs).view(np.uint32), host(keep[0]).view(np.uint32)) and torch.equal(d_faces, keep[1])


# ---- refine_mesh ------------------------------------------------------------------------------------------------------------
def test_refine_mesh_repeats_bit_for_bit():
    from semigcn_amd import remesh
    vs, faces, target, _ = split_case("torus40x30")
    a = remesh.refine_mesh((dev(vs, torch.float32), dev(faces)), target=target)
    b = remesh.refine_mesh((dev(vs, torch.float32), dev(faces)), target=target)
    assert host(a.vs).tobytes() == host(b.vs).tobytes() and host(a.faces).tobytes() == host(b.faces).tobytes()
    assert host(a.parents).tobytes() == host(b.parents).tobytes() and a.report == b.report


def test_pipeline_on_the_stretched_torus():
    """The fixture whose oracle pipeline has no self-intersection (tests/test_remesh_capi.py checks that on the CPU)."""
    from semigcn_amd import evaluate, prepare, remesh, repair
    vs, faces, target, _ = split_case("torus20x12")
    scan = (dev(vs, torch.float32), dev(faces))
    out = remesh.refine_mesh(scan, target=target, iterations=3)
    rep = out.report
    print({k: v for k, v in rep.items() if k != "iterations"}, [(sum(i["split"]), sum(i["flip"])) for i in rep["iterations"]])
    V0, V1 = vs.shape[0], out.vs.shape[0]
    assert rep["n_long"] == 0 and all(i["n_long"] == 0 for i in rep["iterations"]) and len(rep["iterations"]) == 3
    assert len2_all(host(out.vs), host(out.faces)).max() <= np.float32(remesh.split_threshold(target))
    surf = evaluate.Surface(*scan)
    dist = surf.query(out.vs, signed=False)[0]
    surf.close()
    print("max distance to the input surface", float(dist.max()), "bound", surface_bound(vs))
    assert float(dist.max()) <= surface_bound(vs)
    assert rep["deviation_end"] <= rep["iterations"][0]["deviation_after_split"]
    assert rep["deviation_end"] == RO.deviation(host(out.faces)) and rep["deviation_start"] == RO.deviation(faces)
    assert half_edge_counts(host(out.faces), V1)[:2] == (True, 0)
    # parents lead every vertex back to the input's vertices
    par = host(out.parents)
    assert par.shape == (V1, 2) and (par[:V0] == np.arange(V0)[:, None]).all() and (par[V0:] < np.arange(V0, V1)[:, None]).all()
    assert (par[V0:, 0] < par[V0:, 1]).all()
    # the hand-over: prepare_inputs takes it as the initial mesh, repair sees what the intersection oracle sees
    prepared = prepare.prepare_inputs((out.vs, out.faces), scan)
    assert prepared.v_mask.shape[0] == V1 and bool(torch.isfinite(prepared.z1).all())
    want = IO.self_intersections(host(out.vs), host(out.faces))
    got = repair.self_intersections(out.vs, out.faces)
    assert np.array_equal(host(got.pairs), want.pairs) and len(want.pairs) == 0


def test_hole_patches_are_refined_to_the_border_edge_length():
    from semigcn_amd import holes, remesh
    cut = holes.cut_torus(48, 32, 3)
    filled = holes.fill_holes(cut, max_hole_edges=10 ** 6)
    assert len(filled.loops) == 3 and bool(filled.filled.all())
    ring = filled.loops.verts
    nxt = torch.cat([ring[1:], ring[:1]])
    ends = filled.loops.ptr[1:] - 1                        # the last vertex of a loop closes on its first
    nxt[ends] = ring[filled.loops.ptr[:-1]]
    target = float((filled.vs[ring] - filled.vs[nxt]).norm(dim=1).double().mean())
    out = remesh.refine_mesh((filled.vs, filled.faces), target=target)
    l2 = len2_all(host(out.vs), host(out.faces))
    thr2 = np.float32(remesh.split_threshold(target))
    print("target", target, "longest edge / target", float(np.sqrt(l2.max())) / target, "closing", out.report["closing"],
          "V", filled.vs.shape[0], "->", out.vs.shape[0])
    assert out.report["n_long"] == 0
    assert l2.max() <= thr2                                # longest edge <= 4/3 target, as the module forms it in float32
    assert half_edge_counts(host(out.faces), out.vs.shape[0])[:2] == (True, 0)


def test_mid_size_torus_keeps_the_invariants():
    """The stretched 200 x 200 torus, built like the smaller ones (``synth.torus_mesh`` with its default jitter, x scaled by 3,
    target 0.6 x the median edge); no oracle, the invariants alone."""
    from semigcn_amd import remesh
    vs, faces = RO.stretched_torus(200, 200)
    a, b = faces.reshape(-1), faces[:, [1, 2, 0]].reshape(-1)
    target = 0.6 * float(np.median(np.linalg.norm(vs[a] - vs[b], axis=1)))
    out = remesh.refine_mesh((dev(vs), dev(faces)), target=target, iterations=2)
    rep = out.report
    print({k: v for k, v in rep.items() if k != "iterations"},
          [(len(i["split"]), sum(i["split"]), len(i["flip"]), sum(i["flip"])) for i in rep["iterations"]])
    assert rep["n_long"] == 0 and all(i["n_long"] == 0 for i in rep["iterations"])
    assert 0 < len(rep["iterations"][0]["split"]) and 0 < len(rep["iterations"][0]["flip"])
    assert all(len(i["split"]) < 64 and len(i["flip"]) < 32 for i in rep["iterations"])          # below the caps
    assert len(rep["closing"]) < remesh.CLOSING_PASSES
    g_faces = host(out.faces)
    assert half_edge_counts(g_faces, out.vs.shape[0])[:2] == (True, 0)
    assert len2_all(host(out.vs), g_faces).max() <= np.float32(remesh.split_threshold(target))
    assert rep["deviation_end"] < rep["iterations"][0]["deviation_after_split"]
