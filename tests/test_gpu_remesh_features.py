"""The crease rules of semigcn_amd.remesh on the device against tests/remesh_feature_oracle.py.  Every comparison with the
oracle is exact: classes, crease neighbours, crease edges, faces, maps, counts, and positions bit for bit.  For relax_project
and refine_mesh the oracle is given the device's ``laplacian_smooth`` and ``Surface.query`` as its primitives (pinned by
tests/test_gpu_prepare.py and tests/test_gpu_mesh_distance.py): what it restates -- the classes, who moves, the float32 crease
step, what is projected where, every topological decision taken on the projected positions -- then has to agree to the bit.

The bounds: the cube's volume within 1e-5 of 1 (positions lie within one float32 ulp of planes of total area 6), its crease
edges covering each cube edge to 1e-6, and the prism's crease-line vertices within 1e-6 of the input's rims (float64 on the
host).  Premises of the fixtures: tests/test_remesh_feature_fixtures.py, on the CPU."""
import functools

import numpy as np
import pytest
import torch

import remesh_feature_oracle as FO
import remesh_oracle as RO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = sorted(FO.FIXTURES)


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x)).to(DEV)             # a copy: the shared fixtures are read-only
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the device's smoothing and closest-point query as the oracle's primitives --------------------------------------------------
def _smooth(vs, faces, steps, movable):
    from semigcn_amd import prepare
    return host(prepare.laplacian_smooth(dev(vs, torch.float32), dev(faces), steps=steps, movable=dev(movable)))


def _closest(pts, svs, sfaces):
    from semigcn_amd.evaluate import Surface
    with Surface(dev(svs, torch.float32), dev(sfaces)) as s:
        return host(s.query(dev(pts, torch.float32), signed=False)[2])


def _closest_seg(pts, svs, edges):
    from semigcn_amd import remesh
    return _closest(pts, svs, host(remesh.segment_faces(dev(edges))))


PRIMS = dict(smooth=_smooth, closest=_closest, closest_seg=_closest_seg)


@functools.lru_cache(maxsize=None)
def case(name):
    """(vs, faces, target, the oracle's split of it, the oracle's crease edges of the input)"""
    vs, faces = FO.FIXTURES[name]()
    target = FO.TARGETS[name]
    split = RO.split_long_edges(vs, faces, target)
    edges = FO.features(vs, faces, FO.COS30)[2]
    for a in (vs, faces, split[0], split[1], edges):
        a.setflags(write=False)
    return vs, faces, target, split, edges


def device_features(vs, faces, cos_t):
    from semigcn_amd.capi import RemeshPlan
    with RemeshPlan(dev(vs, torch.float32), dev(faces)) as plan:
        assert plan.valid
        plan.set_feature(cos_t)
        vclass, nbr, edges = plan.features()
        assert vclass.dtype == torch.uint8 and nbr.dtype == torch.int64 and edges.dtype == torch.int64
        again = plan.features()                           # asking twice changes nothing
        assert all(torch.equal(a, b) for a, b in zip((vclass, nbr, edges), again))
        return host(vclass), host(nbr), host(edges)


def assert_features(vs, faces, cos_t):
    got, want = device_features(vs, faces, cos_t), FO.features(vs, faces, cos_t)
    for g, w, what in zip(got, want, ("vclass", "crease_nbr", "edges")):
        assert g.shape == w.shape and np.array_equal(g, w), what
    return want


# ---- 1. the predicate and the classes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_features_equal_the_oracle(name):
    vs, faces, _, split, _ = case(name)
    vclass, _, edges = assert_features(vs, faces, FO.COS30)
    print(name, "classes", np.bincount(vclass, minlength=4).tolist(), "C", len(edges))
    assert_features(split[0], split[1], FO.COS30)          # several hundred half-edges, inserted vertices on the creases
    off = device_features(vs, faces, None)
    assert off[2].shape == (0, 2) and set(off[0].tolist()) <= {0, 3} and (off[1] == -1).all()
    assert np.array_equal(off[0] == 3, RO.border_vertices(faces, vs.shape[0]))


def test_hinge_tie_is_not_a_crease_and_one_ulp_more_is():
    vs, faces = FO.hinge60()
    at_tie = assert_features(vs, faces, 0.5)[2].tolist()
    above = assert_features(vs, faces, float(np.nextafter(0.5, 1.0)))[2].tolist()
    assert [0, 1] not in at_tie and [0, 1] in above and len(above) == len(at_tie) + 1


def test_obtuse_feature_angle_on_the_pyramid():
    vs, faces = FO.pyramid()
    vclass, nbr, edges = assert_features(vs, faces, FO.feature_cos(120.0))
    assert vclass.tolist() == [1, 1, 1, 1, 0] and len(edges) == 4
    from semigcn_amd import remesh
    got = remesh.flip_edges(dev(vs), dev(faces), feature_angle=120.0)
    want = FO.flip_edges(vs, faces, FO.feature_cos(120.0))
    assert np.array_equal(host(got.faces), want[0]) and got.flips == want[1]


# ---- 2. flip and collapse ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_flip_equals_the_oracle(name):
    from semigcn_amd import remesh
    _, _, _, split, _ = case(name)
    got = remesh.flip_edges(dev(split[0]), dev(split[1]), feature_angle=30.0)
    w_faces, w_flips, w_before, w_after, _ = FO.flip_edges(split[0], split[1], FO.COS30)
    print(name, "flips", got.flips)
    assert got.flips == w_flips and (got.deviation_before, got.deviation_after) == (w_before, w_after)
    assert np.array_equal(host(got.faces), w_faces)


def assert_collapse(vs, faces, target):
    from semigcn_amd import remesh
    got = remesh.collapse_short_edges(dev(vs), dev(faces), target, feature_angle=30.0)
    w_vs, w_faces, w_ids, w_into, w_counts, w_short = FO.collapse_short_edges(vs, faces, target, FO.COS30)
    assert got.counts == w_counts and got.n_short == w_short
    assert same_bits(host(got.vs), w_vs) and np.array_equal(host(got.faces), w_faces)
    assert np.array_equal(host(got.vertex_ids), w_ids) and np.array_equal(host(got.merged_into), w_into)
    return got


@pytest.mark.parametrize("name", NAMES)
def test_collapse_equals_the_oracle(name):
    _, _, target, split, _ = case(name)
    got = assert_collapse(split[0], split[1], target)
    print(name, "collapses", got.counts)


@pytest.mark.parametrize("name", ["bent", "cube", "l_prism", "pyramid"])
def test_collapse_guards_on_the_unsplit_fixture(name):
    """Everything is short and no length guard holds: what stays is decided by the corner, off-crease and straightness rules."""
    vs, faces = FO.FIXTURES[name]()
    got = assert_collapse(vs, faces, FO.BENT_TARGET)
    if name == "bent":
        assert FO.BENT_HUB in host(got.vertex_ids).tolist()


# ---- 3. relax and project, the pipeline ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_relax_project_equals_the_oracle(name):
    from semigcn_amd import remesh
    vs, faces, _, split, edges = case(name)
    m_vs, m_faces = split[0], FO.flip_edges(split[0], split[1], FO.COS30)[0]
    want = FO.relax_project(m_vs, m_faces, vs, faces, edges, FO.COS30, steps=2, **PRIMS)
    got = host(remesh.relax_project(dev(m_vs), dev(m_faces), (dev(vs), dev(faces)), steps=2, feature_angle=30.0, creases=dev(edges)))
    vclass = FO.features(m_vs, m_faces, FO.COS30)[0]
    fixed = vclass >= FO.CORNER
    print(name, "moved", int((got != m_vs).any(1).sum()), "of", len(got), "max |device - float64 oracle|",
          float(np.abs(got - FO.relax_project(m_vs, m_faces, vs, faces, edges, FO.COS30, steps=2)).max()))
    assert same_bits(got, want)
    assert same_bits(got[fixed], m_vs[fixed])               # corners and border vertices: bit for bit where they were
    # without a segment surface the crease-line vertices stay
    bare = host(remesh.relax_project(dev(m_vs), dev(m_faces), (dev(vs), dev(faces)), steps=2, feature_angle=30.0))
    line = vclass == FO.LINE
    assert same_bits(bare[line], m_vs[line]) and same_bits(bare[~line], got[~line])


def assert_refine(name, collapse):
    from semigcn_amd import remesh
    vs, faces, target, _, _ = case(name)
    got = remesh.refine_mesh((dev(vs), dev(faces)), target=target, iterations=2, collapse=collapse, feature_angle=30.0)
    w_vs, w_faces, w = FO.refine_mesh(vs, faces, target, FO.COS30, iterations=2, collapse=collapse, **PRIMS)
    r = got.report
    print(name, "collapse" if collapse else "", "V", r["n_vertices"], "closing", r["closing"], "creases", r["n_crease_edges_start"],
          r["n_crease_edges_end"], "corners", r["n_corners_start"], r["n_corners_end"])
    for g, o in zip(r["iterations"], w["iterations"]):
        assert {k: g[k] for k in o} == o
    assert len(r["iterations"]) == len(w["iterations"]) and r["closing"] == w["closing"]
    for key in ("n_long", "n_short", "deviation_end", "n_crease_edges_start", "n_crease_edges_end", "n_corners_start", "n_corners_end"):
        assert r[key] == w[key], key
    assert r["feature_angle"] == 30.0
    assert same_bits(host(got.vs), w_vs) and np.array_equal(host(got.faces), w_faces)
    return got


@pytest.mark.parametrize("collapse", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_refine_mesh_equals_the_oracle(name, collapse):
    assert_refine(name, collapse)


# ---- the cube and the prism ---------------------------------------------------------------------------------------------------
def _cube_run(collapse):
    from semigcn_amd import remesh
    vs, faces = FO.cube()
    return remesh.refine_mesh((dev(vs), dev(faces)), target=0.25, iterations=3, collapse=collapse, feature_angle=30.0)


@pytest.mark.parametrize("collapse", [False, True])
def test_cube_keeps_corners_edges_and_volume(collapse):
    out = _cube_run(collapse)
    vs, faces = host(out.vs), host(out.faces)
    rows = {r.tobytes() for r in vs}
    assert all(c.tobytes() in rows for c in FO.cube()[0])                       # the 8 corners, bit for bit
    vol = FO.volume(vs, faces)
    print("cube", "collapse" if collapse else "", "V", len(vs), "volume", vol, "report", {k: v for k, v in out.report.items() if k.startswith("n_c")})
    assert abs(vol - 1.0) <= 1e-5
    assert out.report["n_corners_start"] == out.report["n_corners_end"] == 8 and out.report["n_crease_edges_start"] == 12
    vclass, _, edges = device_features(vs, faces, FO.COS30)
    line = vclass == FO.LINE
    assert (np.isin(vs[line], (0.0, 1.0)).sum(1) == 2).all()                   # crease-line vertices lie on the cube's edges, exactly
    cover = {}
    p = vs.astype(np.float64)
    for lo, hi in edges:
        on = np.isin(vs[lo], (0.0, 1.0)) & np.isin(vs[hi], (0.0, 1.0)) & (vs[lo] == vs[hi])
        assert on.sum() == 2, (lo, hi)                                         # along one cube edge
        key = (int(np.flatnonzero(~on)[0]),) + tuple(float(x) for x in vs[lo][on])
        cover[key] = cover.get(key, 0.0) + float(np.linalg.norm(p[hi] - p[lo]))
    assert len(cover) == 12 and all(abs(v - 1.0) <= 1e-6 for v in cover.values()), cover


def test_cube_repeats_bit_for_bit():
    a, b = _cube_run(True), _cube_run(True)
    assert host(a.vs).tobytes() == host(b.vs).tobytes() and host(a.faces).tobytes() == host(b.faces).tobytes()
    assert a.report == b.report


def test_prism_rims_stay_on_the_input_rims():
    vs, faces, _, _, edges = case("prism16")
    out = assert_refine("prism16", True)
    o_vs, o_faces = host(out.vs), host(out.faces)
    vclass = device_features(o_vs, o_faces, FO.COS30)[0]
    d = FO.distance_to_segments(o_vs[vclass == FO.LINE], vs, edges)
    print("prism16 crease-line vertices", len(d), "max distance to the input's rims", d.max())
    assert len(d) >= 32 and d.max() <= 1e-6


# ---- off means off; a mesh without creases is refined as before ----------------------------------------------------------------
def test_smooth_mesh_is_refined_as_without_the_angle():
    from semigcn_amd import remesh
    vs, faces = FO.smooth_control()
    target = FO.SMOOTH_TARGET * RO.median_edge(vs, faces)
    d_vs, d_faces = dev(vs), dev(faces)
    split = remesh.split_long_edges(d_vs, d_faces, target)
    for angle in (None, 30.0):
        f = remesh.flip_edges(split.vs, split.faces, **({} if angle is None else {"feature_angle": angle}))
        c = remesh.collapse_short_edges(split.vs, split.faces, target, **({} if angle is None else {"feature_angle": angle}))
        r = remesh.refine_mesh((d_vs, d_faces), target=target, iterations=1, collapse=True, feature_angle=angle)
        if angle is None:
            f0, c0, r0 = f, c, r
    assert sum(f.flips) > 0 and sum(c.counts) > 0
    assert torch.equal(f.faces, f0.faces) and f.flips == f0.flips
    assert torch.equal(c.vs, c0.vs) and torch.equal(c.faces, c0.faces) and c.counts == c0.counts and torch.equal(c.merged_into, c0.merged_into)
    assert host(r.vs).tobytes() == host(r0.vs).tobytes() and torch.equal(r.faces, r0.faces)
    assert r.report["n_crease_edges_start"] == r.report["n_crease_edges_end"] == r.report["n_corners_end"] == 0
    assert {k: v for k, v in r.report.items() if k in r0.report} == r0.report and "feature_angle" not in r0.report


def test_bad_feature_angle_raises_before_any_device_work():
    from semigcn_amd import remesh
    vs, faces = (dev(x) for x in FO.cube())
    for bad in (0, 180, float("nan")):
        for call in (lambda: remesh.flip_edges(vs, faces, feature_angle=bad),
                     lambda: remesh.collapse_short_edges(vs, faces, 0.25, feature_angle=bad),
                     lambda: remesh.relax_project(vs, faces, (vs, faces), feature_angle=bad),
                     lambda: remesh.refine_mesh((vs, faces), target=0.25, feature_angle=bad)):
            with pytest.raises(ValueError, match="feature_angle"):
                call()
