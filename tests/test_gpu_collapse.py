"""Edge collapse of semigcn_amd.remesh on the device against the numpy restatement in tests/collapse_oracle.py.  Every
comparison with the oracle is exact: positions bit-identical, faces, vertex_ids, merged_into, round counts and n_short equal.

Shapes: the hand cases (fan, pulled fan, tetrahedron, 3 x 3 grid: one collapse per round or none); the open 8 x 8 grid at a
target where the length guard blocks everything and at one where it does not; the level-3 octahedron sphere (1536
half-edges: scans and compaction span 6 workgroups); the stretched 20 x 12 and 40 x 30 tori (the latter: 7200 half-edges,
56 rounds that each compact); split -> collapse -> flip on one plan; the pipeline with the hand-over to prepare_inputs and
repair; and a stretched 200 x 200 torus for the invariants alone."""
import functools
import threading
import time

import numpy as np
import pytest
import torch

import collapse_oracle as CO
import remesh_oracle as RO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x)).to(DEV)             # a copy: the shared fixtures are read-only
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.cpu().numpy()


def surface_bound(vs):
    return 8 * 2.0 ** -23 * float(np.abs(np.asarray(vs)).max())


def edges_len2(vs, faces):
    """(the unique undirected edges [E, 2] with lo < hi, their len2 as the module defines it: float32, left to right)"""
    vs, f = np.asarray(vs, np.float32), np.asarray(faces, np.int64)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    e = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], 1), axis=0)
    d = vs[e[:, 1]] - vs[e[:, 0]]
    return e, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def half_edge_counts(faces, V):
    """(every directed half-edge once and no edge with three faces, V - E + F over the used vertices, border-vertex flags)"""
    f = np.asarray(faces, np.int64)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    directed = a * V + b
    und, cnt = np.unique(np.minimum(a, b) * V + np.maximum(a, b), return_counts=True)
    border = np.zeros(V, bool)
    border[und[cnt == 1] // V] = True
    border[und[cnt == 1] % V] = True
    return np.unique(directed).shape[0] == directed.shape[0] and cnt.max() <= 2, np.unique(f).shape[0] - und.shape[0] + f.shape[0], border


# ---- fixtures: (vs, faces, target), and the oracle's answer computed once --------------------------------------------------
def _times_median(factor, vs, faces):
    return vs, faces, factor * RO.median_edge(vs, faces)


CASES = {
    "fan8": lambda: RO.fan8() + (10.0,),
    "fan8_pulled": lambda: RO.fan8(pulled=True) + (10.0,),
    "tetrahedron": lambda: RO.tetrahedron() + (10.0,),
    "grid3": lambda: RO.grid(3) + (10.0,),
    "grid8_blocked": lambda: RO.grid(8) + (1.3,),
    "grid8": lambda: RO.grid(8) + (2.0,),
    "sphere3": lambda: _times_median(2.0, *CO.octa_sphere(3)),
    "torus20x12": lambda: _times_median(1.8, *RO.stretched_torus(20, 12)),
    "torus40x30": lambda: _times_median(1.8, *RO.stretched_torus(40, 30)),
}
# (rounds, vertices before, vertices after) of the serial prototype
PROTOTYPE = {"fan8": (1, 9, 8), "fan8_pulled": (1, 9, 8), "tetrahedron": (0, 4, 4), "grid3": (4, 16, 12), "grid8_blocked": (0, 81, 81),
             "grid8": (14, 81, 48), "sphere3": (24, 258, 66), "torus20x12": (33, 240, 97), "torus40x30": (56, 1200, 509)}


@functools.lru_cache(maxsize=None)
def case(name):
    vs, faces, target = CASES[name]()
    return vs, faces, target, CO.collapse_short_edges(vs, faces, target)


def device_collapse(vs, faces, target, **kw):
    from semigcn_amd import remesh
    d_vs, d_faces = dev(vs, torch.float32), dev(faces)
    keep = (d_vs.clone(), d_faces.clone())
    got = remesh.collapse_short_edges(d_vs, d_faces, target, **kw)
    assert torch.equal(d_vs, keep[0]) and torch.equal(d_faces, keep[1])
    assert got.vs.dtype == torch.float32 and {got.faces.dtype, got.vertex_ids.dtype, got.merged_into.dtype} == {torch.int64}
    return got


def assert_equals(got, want):
    w_vs, w_faces, w_ids, w_merged, w_counts, w_short = want
    assert got.counts == w_counts and got.n_short == w_short
    assert tuple(got.vs.shape) == w_vs.shape and tuple(got.faces.shape) == w_faces.shape
    assert np.array_equal(host(got.vs).view(np.uint32), w_vs.view(np.uint32))
    assert np.array_equal(host(got.faces), w_faces)
    assert np.array_equal(host(got.vertex_ids), w_ids) and np.array_equal(host(got.merged_into), w_merged)


@pytest.mark.parametrize("name", sorted(CASES))
def test_collapse_equals_the_oracle(name):
    vs, faces, target, want = case(name)
    got = device_collapse(vs, faces, target)
    print(name, "rounds", len(got.counts), got.counts, "V", vs.shape[0], "->", got.vs.shape[0], "n_short", got.n_short)
    assert (len(want[4]), vs.shape[0], want[0].shape[0]) == PROTOTYPE[name]
    assert_equals(got, want)
    if name == "sphere3":
        assert 3 * faces.shape[0] == 1536
    if name == "torus40x30":
        assert 3 * faces.shape[0] == 7200


def test_round_cap_is_reported_not_raised():
    vs, faces, target, want = case("torus20x12")
    first = CO.collapse_short_edges(vs, faces, target, max_rounds=1)
    got = device_collapse(vs, faces, target, max_rounds=1)
    assert got.counts == want[4][:1] and got.n_short == first[5] > want[5]
    assert_equals(got, first)
    none = device_collapse(vs, faces, target, max_rounds=0)
    V = vs.shape[0]
    assert none.counts == [] and none.n_short == 517
    assert np.array_equal(host(none.vs).view(np.uint32), vs.view(np.uint32)) and np.array_equal(host(none.faces), faces)
    assert np.array_equal(host(none.vertex_ids), np.arange(V)) and np.array_equal(host(none.merged_into), np.arange(V))


@pytest.mark.parametrize("name", ["grid8", "sphere3", "torus40x30"])
def test_collapse_invariants(name):
    vs, faces, target, _ = case(name)
    a, b = device_collapse(vs, faces, target), device_collapse(vs, faces, target)
    for x, y in ((a.vs, b.vs), (a.faces, b.faces), (a.vertex_ids, b.vertex_ids), (a.merged_into, b.merged_into)):
        assert host(x).tobytes() == host(y).tobytes()
    assert (a.counts, a.n_short) == (b.counts, b.n_short)
    ids, merged = host(a.vertex_ids), host(a.merged_into)
    assert np.array_equal(host(a.vs).view(np.uint32), vs[ids].view(np.uint32))
    assert merged.shape == (vs.shape[0],) and np.array_equal(merged[ids], np.arange(ids.shape[0]))
    assert (np.diff(ids) > 0).all()                        # stable compaction
    once0, euler0, border0 = half_edge_counts(faces, vs.shape[0])
    once1, euler1, border1 = half_edge_counts(host(a.faces), ids.shape[0])
    assert once0 and once1 and euler1 == euler0 and np.array_equal(border1, border0[ids])


def test_border_flags_are_carried_over_on_the_open_grid():
    from semigcn_amd import remesh
    vs, faces, target, want = case("grid8")
    plan = remesh.RemeshPlan(dev(vs, torch.float32), dev(faces))
    try:
        assert plan.collapse(remesh.collapse_threshold(target), remesh.split_threshold(target)) == (want[4], want[5])
        g_vs, g_faces, g_par, g_border = plan.export()
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert np.array_equal(host(g_faces), want[1])
    numpy_border = half_edge_counts(want[1], want[0].shape[0])[2]
    assert np.array_equal(host(g_border), numpy_border) and numpy_border.sum() == 32      # the rim is untouched
    assert np.array_equal(host(g_par), np.repeat(np.arange(want[0].shape[0])[:, None], 2, 1))


def test_split_collapse_flip_on_one_plan():
    from semigcn_amd import remesh
    vs, faces = RO.stretched_torus(20, 12)
    target = 0.6 * RO.median_edge(vs, faces)
    s_vs, s_faces, s_par, s_counts, s_long = RO.split_long_edges(vs, faces, target)
    c_vs, c_faces, ids, merged, c_counts, c_short = CO.collapse_short_edges(s_vs, s_faces, target)
    w_faces, w_flips, w_before, w_after, _ = RO.flip_edges(c_vs, c_faces)
    assert c_counts and w_flips and c_vs.shape[0] < s_vs.shape[0]
    plan = remesh.RemeshPlan(dev(vs, torch.float32), dev(faces))
    try:
        assert plan.valid
        i0, m0 = plan.collapse_maps()                      # before any collapse: the identity
        assert np.array_equal(host(i0), np.arange(240)) and np.array_equal(host(m0), np.arange(240))
        assert plan.split(remesh.split_threshold(target)) == (s_counts, s_long)
        assert plan.collapse(remesh.collapse_threshold(target), remesh.split_threshold(target)) == (c_counts, c_short)
        assert (plan.num_vertices, plan.num_faces) == (c_vs.shape[0], c_faces.shape[0])
        assert plan.flip() == (w_flips, w_before, w_after)
        g_vs, g_faces, g_par, g_border = plan.export()
        g_ids, g_merged = plan.collapse_maps()
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert np.array_equal(host(g_vs).view(np.uint32), c_vs.view(np.uint32)) and np.array_equal(host(g_faces), w_faces)
    assert np.array_equal(host(g_ids), ids) and np.array_equal(host(g_merged), merged)
    assert np.array_equal(host(g_par), merged[s_par[ids]])  # renumbered; a removed end names the vertex it went into
    assert np.array_equal(host(g_border), half_edge_counts(w_faces, c_vs.shape[0])[2])
    assert host(g_border).dtype == bool and not host(g_border).any()


def test_pipeline_with_collapse_on_the_stretched_torus():
    import intersect_oracle as IO
    from semigcn_amd import evaluate, prepare, remesh, repair
    vs, faces = RO.stretched_torus(20, 12)
    target = 0.6 * RO.median_edge(vs, faces)
    scan = (dev(vs, torch.float32), dev(faces))
    plain = remesh.refine_mesh(scan, target=target, iterations=3)
    out = remesh.refine_mesh(scan, target=target, iterations=3, collapse=True, timings=True)
    rep = out.report
    print({k: v for k, v in rep.items() if k != "iterations"},
          [(sum(i["split"]), sum(i["collapse"]), len(i["collapse"]), sum(i["flip"])) for i in rep["iterations"]])
    print("n_short", plain.report["n_short"], "->", rep["n_short"], "V", plain.vs.shape[0], "->", out.vs.shape[0])
    assert out.parents is None and plain.parents is not None
    assert len(rep["iterations"]) == 3 and all(sum(i["collapse"]) > 0 and i["n_short_after_collapse"] >= 0 for i in rep["iterations"])
    assert "collapse_ms" in out.stage_ms and "collapse" not in plain.report["iterations"][0]
    V1 = out.vs.shape[0]
    check = remesh.RemeshPlan(out.vs, out.faces)           # a valid input
    try:
        assert check.valid and (check.num_vertices, check.num_faces) == (V1, out.faces.shape[0])
    finally:
        check.close()
    assert half_edge_counts(host(out.faces), V1)[:2] == (True, 0)
    assert rep["n_long"] == 0 and all(i["n_long"] == 0 for i in rep["iterations"])
    assert edges_len2(host(out.vs), host(out.faces))[1].max() <= np.float32(remesh.split_threshold(target))
    surf = evaluate.Surface(*scan)
    dist = surf.query(out.vs, signed=False)[0]
    surf.close()
    print("max distance to the input surface", float(dist.max()), "bound", surface_bound(vs))
    assert float(dist.max()) <= surface_bound(vs)
    want = IO.self_intersections(host(out.vs), host(out.faces))
    got = repair.self_intersections(out.vs, out.faces)
    assert np.array_equal(host(got.pairs), want.pairs) and len(want.pairs) == 0
    assert rep["n_short"] < 0.5 * plain.report["n_short"]  # the prototype: 357 / 2282 = 0.16
    prepared = prepare.prepare_inputs((out.vs, out.faces), scan)
    assert prepared.v_mask.shape[0] == V1 and bool(torch.isfinite(prepared.z1).all())


def test_refine_mesh_without_collapse_is_unchanged():
    from semigcn_amd import remesh
    vs, faces = RO.stretched_torus(20, 12)
    target = 0.6 * RO.median_edge(vs, faces)
    a = remesh.refine_mesh((dev(vs, torch.float32), dev(faces)), target=target, iterations=2, timings=True)
    b = remesh.refine_mesh((dev(vs, torch.float32), dev(faces)), target=target, iterations=2, timings=True, collapse=False)
    for x, y in ((a.vs, b.vs), (a.faces, b.faces), (a.parents, b.parents)):
        assert host(x).tobytes() == host(y).tobytes()
    assert a.report == b.report and sorted(a.stage_ms) == sorted(b.stage_ms) == ["flip_ms", "relax_ms", "report_ms", "split_ms", "surface_ms"]
    assert sorted(a.report["iterations"][0]) == ["deviation_after_flip", "deviation_after_split", "flip", "n_long", "split"]


def test_mid_size_torus_keeps_the_invariants():
    """The stretched 200 x 200 torus at 1.8 x the median edge; no oracle, the invariants alone.  The time limit: the 40 x 30
    case is timed first; this mesh has 40000 / 1200 times its elements and may take 128 rounds instead of that case's 56, and
    a round costs at most in proportion to the elements (the small case is bound by launches, not by elements), so the limit is
    that time x (40000 / 1200) x (128 / 56), and never below 5 s."""
    from semigcn_amd import remesh
    s_vs, s_faces, s_target, s_want = case("torus40x30")
    device_collapse(s_vs, s_faces, s_target)              # warm: buffers of the allocator, code objects
    t0 = time.perf_counter()
    small = device_collapse(s_vs, s_faces, s_target)
    torch.cuda.synchronize()
    t_small = time.perf_counter() - t0
    limit = max(5.0, t_small * (40000 / 1200) * (128 / len(small.counts)))
    vs, faces = RO.stretched_torus(200, 200)
    e0, l0 = edges_len2(vs, faces)
    target = 1.8 * float(np.median(np.sqrt(l0.astype(np.float64))))
    thr2 = np.float32(remesh.split_threshold(target))
    box = {}

    def run():
        try:
            box["out"] = remesh.collapse_short_edges(dev(vs), dev(faces), target)
            torch.cuda.synchronize()
        except BaseException as e:                         # noqa: BLE001 -- reported below, in the test's thread
            box["error"] = e

    t0 = time.perf_counter()
    th = threading.Thread(target=run, daemon=True)
    th.start()
    th.join(limit)
    took = time.perf_counter() - t0
    assert not th.is_alive(), f"no result within {limit:.1f} s (the 40 x 30 case took {t_small:.3f} s)"
    assert "error" not in box, box.get("error")
    out = box["out"]
    print("rounds", len(out.counts), "V", vs.shape[0], "->", out.vs.shape[0], "n_short", out.n_short, f"{took:.2f} s of {limit:.1f} s")
    assert out.counts and all(c > 0 for c in out.counts) and sum(out.counts) == vs.shape[0] - out.vs.shape[0]
    check = remesh.RemeshPlan(out.vs, out.faces)
    try:
        assert check.valid
    finally:
        check.close()
    g_vs, g_faces, ids = host(out.vs), host(out.faces), host(out.vertex_ids)
    assert half_edge_counts(g_faces, g_vs.shape[0])[:2] == (True, 0) == half_edge_counts(faces, vs.shape[0])[:2]
    assert np.array_equal(g_vs.view(np.uint32), vs[ids].view(np.uint32))
    e1, l1 = edges_len2(g_vs, g_faces)
    V = vs.shape[0]
    long_before = set((e0[l0 > thr2] @ np.array([V, 1])).tolist())
    long_after = (ids[e1[l1 > thr2]] @ np.array([V, 1])).tolist()      # stable compaction keeps lo < hi
    assert all(k in long_before for k in long_after)
