"""semigcn_amd.remesh below the C ABI (csrc/mesh_remesh.hip), without a device: the entry points exist in the header, the
ctypes table and the library; they reject bad arguments before touching a device; the Python functions have no CPU path and
raise their ValueErrors first; and the numpy oracle the GPU tests compare against (tests/remesh_oracle.py) gives the
hand-computed answers and keeps its own invariants."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import remesh_oracle as RO
from semigcn_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sg_remesh_create", "sg_remesh_destroy", "sg_remesh_query", "sg_remesh_split", "sg_remesh_flip", "sg_remesh_export")


def test_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "semigcn.h")).read()
    declared = re.findall(r"^SG_API\s+[\w\s\*]+?\b(sg_\w+)\s*\(", text, flags=re.M)
    lib = ctypes.CDLL(capi.library_path())
    for name in NEW:
        assert name in declared, name
        assert name in capi._SIGNATURES, name
        assert hasattr(lib, name), name
    assert "typedef struct sg_remesh sg_remesh;" in text
    assert capi.load().sg_abi_version() == 1
    assert callable(capi.RemeshPlan.close) and callable(capi.RemeshPlan.__del__)


def test_argument_validation_without_gpu():
    lib = capi.load()
    buf = (ctypes.c_int64 * 16)()          # host memory: every call below must return before it would be touched
    p = ctypes.c_void_p(ctypes.addressof(buf))
    plan = ctypes.c_void_p()
    n = ctypes.c_int64()

    create = lib.sg_remesh_create
    assert create(p, 4, p, 2, None, None) == -1 and b"null out" in lib.sg_last_error()
    assert create(p, -1, p, 2, None, ctypes.byref(plan)) == -1 and b"negative" in lib.sg_last_error() and not plan.value
    assert create(p, 4, p, -1, None, ctypes.byref(plan)) == -1 and b"negative" in lib.sg_last_error() and not plan.value
    assert create(None, 4, p, 2, None, ctypes.byref(plan)) == -1 and b"null pointer" in lib.sg_last_error() and not plan.value
    assert create(p, 4, None, 2, None, ctypes.byref(plan)) == -1 and b"null pointer" in lib.sg_last_error() and not plan.value
    # sizes the 32-bit sort and indices cannot hold
    assert create(p, 4, p, (1 << 31) // 3 + 1, None, ctypes.byref(plan)) == -1 and b"int32" in lib.sg_last_error() and not plan.value
    assert create(p, 1 << 31, p, 2, None, ctypes.byref(plan)) == -1 and b"int32" in lib.sg_last_error() and not plan.value
    # faces without vertices
    assert create(None, 0, p, 2, None, ctypes.byref(plan)) == -1 and b"outside" in lib.sg_last_error() and not plan.value

    assert lib.sg_remesh_query(None, buf) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_remesh_split(None, 1.0, 4, None, buf, ctypes.byref(n), ctypes.byref(n)) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_remesh_flip(None, 4, None, buf, ctypes.byref(n), buf) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_remesh_export(None, p, p, p, p, None) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_remesh_destroy(None) == 0


def test_empty_plan_without_gpu():
    """V = F = 0 needs no device: the checks that need a plan can be exercised on it."""
    lib = capi.load()
    plan = ctypes.c_void_p()
    n_rounds, n_long = ctypes.c_int64(7), ctypes.c_int64(7)
    counts = (ctypes.c_int64 * 4)()
    dev = (ctypes.c_int64 * 2)(5, 5)
    info = (ctypes.c_int64 * 16)()
    assert lib.sg_remesh_create(None, 0, None, 0, None, ctypes.byref(plan)) == 0 and plan.value
    try:
        assert lib.sg_remesh_query(plan, None) == -1 and b"null pointer" in lib.sg_last_error()
        assert lib.sg_remesh_query(plan, info) == 0
        assert list(info) == [0, 0, 0, 0, 0, 0, 0, 0, -1, -1, -1, -1, 0, 0, 1, 0]
        split, flip = lib.sg_remesh_split, lib.sg_remesh_flip
        assert split(plan, 1.0, -1, None, counts, ctypes.byref(n_rounds), ctypes.byref(n_long)) == -1 and b"max_rounds" in lib.sg_last_error()
        for bad in (0.0, -1.0, float("nan")):
            assert split(plan, bad, 4, None, counts, ctypes.byref(n_rounds), ctypes.byref(n_long)) == -1 and b"thr2" in lib.sg_last_error()
        assert split(plan, 1.0, 4, None, None, ctypes.byref(n_rounds), ctypes.byref(n_long)) == -1 and b"null pointer" in lib.sg_last_error()
        assert split(plan, 1.0, 4, None, counts, None, ctypes.byref(n_long)) == -1 and b"null pointer" in lib.sg_last_error()
        assert flip(plan, -1, None, counts, ctypes.byref(n_rounds), dev) == -1 and b"max_rounds" in lib.sg_last_error()
        assert flip(plan, 4, None, counts, ctypes.byref(n_rounds), None) == -1 and b"null pointer" in lib.sg_last_error()
        assert split(plan, 1.0, 4, None, counts, ctypes.byref(n_rounds), ctypes.byref(n_long)) == 0
        assert (n_rounds.value, n_long.value) == (0, 0)
        assert flip(plan, 4, None, counts, ctypes.byref(n_rounds), dev) == 0 and list(dev) == [0, 0] and n_rounds.value == 0
        assert lib.sg_remesh_export(plan, None, None, None, None, None) == 0
    finally:
        assert lib.sg_remesh_destroy(plan) == 0


def test_python_functions_have_no_cpu_path():
    from semigcn_amd import remesh
    vs, faces = (torch.from_numpy(x) for x in RO.tetrahedron())
    with pytest.raises(capi.SemigcnLibraryError):
        remesh.split_long_edges(vs, faces, 0.5)
    with pytest.raises(capi.SemigcnLibraryError):
        remesh.flip_edges(vs, faces)
    with pytest.raises(capi.SemigcnLibraryError):
        remesh.relax_project(vs, faces, (vs, faces))
    with pytest.raises(capi.SemigcnLibraryError):
        remesh.refine_mesh((vs, faces))
    with pytest.raises(capi.SemigcnLibraryError):
        remesh.RemeshPlan(vs, faces)
    # the ValueErrors come before the device check
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="target"):
            remesh.split_long_edges(vs, faces, bad)
        with pytest.raises(ValueError, match="target"):
            remesh.refine_mesh((vs, faces), target=bad)
        with pytest.raises(ValueError, match="target_percent"):
            remesh.refine_mesh((vs, faces), target_percent=bad)
    with pytest.raises(ValueError, match="max_rounds"):
        remesh.split_long_edges(vs, faces, 0.5, max_rounds=-1)
    with pytest.raises(ValueError, match="max_rounds"):
        remesh.flip_edges(vs, faces, max_rounds=-1)
    with pytest.raises(ValueError, match="steps"):
        remesh.relax_project(vs, faces, (vs, faces), steps=-1)
    with pytest.raises(ValueError, match="iterations"):
        remesh.refine_mesh((vs, faces), iterations=-1)
    for fn in (lambda v, f: remesh.split_long_edges(v, f, 0.5), remesh.flip_edges, lambda v, f: remesh.refine_mesh((v, f)),
               lambda v, f: remesh.relax_project(v, f, (vs, faces))):
        with pytest.raises(ValueError, match="vs must be"):
            fn(vs[:, :2], faces)
        with pytest.raises(ValueError, match="vs must hold floats"):
            fn(vs.long(), faces)
        with pytest.raises(ValueError, match="faces must be"):
            fn(vs, faces.reshape(-1))
        with pytest.raises(ValueError, match="faces must hold integers"):
            fn(vs, faces.float())
    assert remesh.split_threshold(0.75) == 1.0 and remesh.split_threshold(1.0) == float(np.float32(16.0 / 9.0))


# ---- the oracle's own pins ---------------------------------------------------------------------------------------------
def test_oracle_hash_is_the_stated_mixer():
    assert RO.hash32(0) == 0
    x = 1
    x ^= x >> 16
    x = (x * 0x7FEB352D) % 2 ** 32
    x ^= x >> 15
    x = (x * 0x846CA68B) % 2 ** 32
    x ^= x >> 16
    assert RO.hash32(1) == x
    assert len({RO.hash32(i) for i in range(4096)}) == 4096


def test_oracle_one_triangle_with_three_long_edges():
    """Edges of length 3, 4, 5, target 1: all long; a face has one selected edge, the longest ({1, 2}, from corner 1)."""
    vs, faces = RO.one_triangle()
    thr2 = RO.split_threshold(1.0)
    new_vs, new_faces, ends, n_long = RO.split_round(vs, faces, thr2)
    assert n_long == 3 and ends == [[1, 2]]
    assert new_vs.tolist() == [[0, 0, 0], [3, 0, 0], [0, 4, 0], [1.5, 2, 0]]
    assert new_faces.tolist() == [[1, 3, 0], [3, 2, 0]]
    # round 2: {0, 2} (len2 16) in face 1, {0, 1} (len2 9) in face 0 -- {0, 3} (len2 6.25) loses in both
    vs2, faces2, ends2, n_long2 = RO.split_round(new_vs, new_faces, thr2)
    assert n_long2 == 5 and ends2 == [[0, 1], [0, 2]]
    assert vs2[4:].tolist() == [[1.5, 0, 0], [0, 2, 0]]
    assert faces2.tolist() == [[0, 4, 3], [2, 5, 3], [4, 1, 3], [5, 0, 3]]
    out_vs, out_faces, parents, counts, left = RO.split_long_edges(vs, faces, 1.0)
    assert left == 0 and counts[:2] == [1, 2] and float(RO.max_len2(out_vs, out_faces)) <= float(thr2)
    assert parents[:5].tolist() == [[0, 0], [1, 1], [2, 2], [1, 2], [0, 1]]
    assert RO.euler(out_faces) == 1 and RO.directed_once(out_faces)
    # a cap is reported, not raised
    capped = RO.split_long_edges(vs, faces, 1.0, max_rounds=1)
    assert capped[3] == [1] and capped[4] == 5 and capped[1].tolist() == new_faces.tolist()
    assert RO.split_long_edges(vs, faces, 1.0, max_rounds=0)[3:] == ([], 3)


def test_oracle_two_triangles_share_the_new_vertex():
    """The diagonal {0, 2} (len2 32) is the only edge above thr2 = 16: one vertex, (2, 2, 0), serves both faces."""
    vs, faces = RO.two_triangles()
    assert float(RO.split_threshold(3.0)) == 16.0
    out_vs, out_faces, parents, counts, left = RO.split_long_edges(vs, faces, 3.0)
    assert counts == [1] and left == 0 and out_vs[4].tolist() == [2, 2, 0] and parents[4].tolist() == [0, 2]
    assert out_faces.tolist() == [[2, 4, 1], [0, 4, 3], [4, 0, 1], [4, 2, 3]]


def test_oracle_flip_hand_cases():
    # the tetrahedron: {c, d} always exists and no valence may fall below 3
    vs, faces = RO.tetrahedron()
    assert RO.flip_candidates(vs, faces) == {}
    out, flips, before, after, _ = RO.flip_edges(vs, faces)
    assert flips == [] and before == after == 12 and np.array_equal(out, faces)
    # the fan: hub valence 8 (target 6), rim valence 3 (border, target 4); every spoke gains 1 + (-1) + 1 + 1 = 2
    vs, faces = RO.fan8()
    cands = RO.flip_candidates(vs, faces)
    assert sorted(cands) == [(0, i) for i in range(1, 9)] and {c[0][0] for c in cands.values()} == {2}
    assert RO.deviation(faces) == 2 + 8
    # conflict: all eight share the hub, one wins per round; after two the hub is regular and nothing gains
    out, flips, before, after, trail = RO.flip_edges(vs, faces)
    assert flips == [1, 1] and trail == [10, 8, 6]
    first, sel = RO.flip_round(vs, faces)
    (e, (a, b, c, d)), = sel
    rim = e[1]                                             # the lower half-edge names a: the hub for spoke 1, the rim vertex otherwise
    assert e == max(cands, key=lambda k: cands[k][0]) and {a, b} == {0, rim} and {c, d} == {1 + (rim - 2) % 8, 1 + rim % 8}
    f0, f1 = cands[e][2]
    assert first[f0].tolist() == [a, d, c] and first[f1].tolist() == [d, b, c]
    # the guard: vertex 1 pulled inside the chord from 8 to 2 -- the same topology, the same gain, but spoke {0, 1} is refused
    vs_p, faces_p = RO.fan8(pulled=True)
    assert RO.guard(vs, 0, 1, 2, 8) and not RO.guard(vs_p, 0, 1, 2, 8)
    assert sorted(RO.flip_candidates(vs_p, faces_p)) == [(0, i) for i in range(2, 9)]


def test_oracle_rejections():
    vs, faces = RO.tetrahedron()
    assert RO.check_input(vs, faces)["n_nonmanifold"] == 0
    with pytest.raises(ValueError, match="'n_nonmanifold': 1.*'bad_edge': \\(0, 1\\)"):
        RO.check_input(np.concatenate([vs, [[1, 1, 1]]]).astype(np.float32), np.concatenate([faces, [[0, 1, 4]]]))
    with pytest.raises(ValueError, match="'n_misoriented': 3"):
        RO.check_input(vs, np.concatenate([faces[:3], faces[3:, ::-1]]))
    with pytest.raises(ValueError, match="'n_degenerate': 1.*'bad_face': 4"):
        RO.check_input(vs, np.concatenate([faces, [[2, 2, 3]]]))
    bad = vs.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="'n_nonfinite': 1.*'bad_vertex': 2"):
        RO.check_input(bad, faces)


def test_oracle_invariants_on_the_stretched_torus():
    """Never two selected edges in one face (split_round asserts it), flips vertex-disjoint, every round lowers the deviation;
    the figures of the prototype: 240 / 480 -> 1138 / 2276, no long edge left, Euler characteristic unchanged."""
    vs, faces = RO.stretched_torus(20, 12)
    target = 0.6 * RO.median_edge(vs, faces)
    thr2 = RO.split_threshold(target)
    selected, n_long, table = RO.select_split(vs, faces, thr2)
    per_face = {}
    for e in selected:
        for h in table[e]:
            per_face[h // 3] = per_face.get(h // 3, 0) + 1
    assert selected and n_long > len(selected) and set(per_face.values()) == {1}
    out_vs, out_faces, parents, counts, left = RO.split_long_edges(vs, faces, target)
    assert (out_vs.shape[0], out_faces.shape[0]) == (1138, 2276) and left == 0 and 8 <= len(counts) <= 16
    assert float(RO.max_len2(out_vs, out_faces)) <= float(thr2)
    assert RO.euler(out_faces) == RO.euler(faces) == 0 and RO.directed_once(out_faces)
    assert (parents[:240, 0] == np.arange(240)).all() and (parents[240:] < np.arange(240, 1138)[:, None]).all()
    cur = out_faces
    trail = [RO.deviation(cur)]
    for _ in range(3):
        cur, sel = RO.flip_round(out_vs, cur)
        used = [v for _, quad in sel for v in quad]
        assert sel and len(used) == len(set(used))
        trail.append(RO.deviation(cur))
        assert RO.directed_once(cur) and RO.euler(cur) == 0
    assert all(b < a for a, b in zip(trail, trail[1:]))


def test_oracle_pipeline_on_the_fixture_of_the_gpu_test_has_no_self_intersection():
    """tests/test_gpu_remesh.py compares repair.self_intersections on the device's refined torus with the intersection
    oracle; that says most when the expected answer is known: the oracle pipeline (float64 smoothing, brute-force closest
    point) gives zero pairs on the stretched 20 x 12 torus after 3 iterations."""
    import intersect_oracle as IO
    vs, faces = RO.stretched_torus(20, 12)
    out_vs, out_faces, parents = RO.refine_mesh(vs, faces, 0.6 * RO.median_edge(vs, faces), iterations=3)
    assert out_vs.shape[0] > 1138 and parents.shape == (out_vs.shape[0], 2)
    assert len(IO.self_intersections(out_vs, out_faces).pairs) == 0
    assert RO.closest_points(out_vs, vs, faces)[1].max() <= 8 * 2.0 ** -23 * np.abs(vs).max()
