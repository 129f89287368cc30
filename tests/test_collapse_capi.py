"""Edge collapse of semigcn_amd.remesh below the C ABI (csrc/mesh_remesh.hip), without a device: the two entry points exist in
the header, the ctypes table and the library; they reject bad arguments before touching a device; the Python functions have no
CPU path and raise their ValueErrors first; and the numpy oracle the GPU tests compare against (tests/collapse_oracle.py) gives
the hand-computed answers and keeps its own invariants."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import collapse_oracle as CO
import remesh_oracle as RO
from semigcn_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sg_remesh_collapse", "sg_remesh_collapse_maps")


def test_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "semigcn.h")).read()
    declared = re.findall(r"^SG_API\s+[\w\s\*]+?\b(sg_\w+)\s*\(", text, flags=re.M)
    lib = ctypes.CDLL(capi.library_path())
    for name in NEW:
        assert name in declared, name
        assert name in capi._SIGNATURES, name
        assert hasattr(lib, name), name
    assert capi.load().sg_abi_version() == 1
    assert callable(capi.RemeshPlan.collapse) and callable(capi.RemeshPlan.collapse_maps)
    assert "Edge collapse is not part of it" not in text


def test_argument_validation_without_gpu():
    lib = capi.load()
    buf = (ctypes.c_int64 * 16)()          # host memory: every call below must return before it would be touched
    p = ctypes.c_void_p(ctypes.addressof(buf))
    n = ctypes.c_int64()
    assert lib.sg_remesh_collapse(None, 1.0, 2.0, 4, None, buf, ctypes.byref(n), ctypes.byref(n)) == -1
    assert b"null plan" in lib.sg_last_error()
    assert lib.sg_remesh_collapse_maps(None, p, p, None) == -1 and b"null plan" in lib.sg_last_error()


def test_empty_plan_without_gpu():
    """V = F = 0 needs no device: the checks that need a plan can be exercised on it."""
    lib = capi.load()
    plan = ctypes.c_void_p()
    n_rounds, n_short = ctypes.c_int64(7), ctypes.c_int64(7)
    counts = (ctypes.c_int64 * 4)()
    info = (ctypes.c_int64 * 16)()
    nr, ns = ctypes.byref(n_rounds), ctypes.byref(n_short)
    assert lib.sg_remesh_create(None, 0, None, 0, None, ctypes.byref(plan)) == 0 and plan.value
    try:
        collapse = lib.sg_remesh_collapse
        assert collapse(plan, 1.0, 2.0, -1, None, counts, nr, ns) == -1 and b"max_rounds" in lib.sg_last_error()
        for bad in (0.0, -1.0, float("nan")):
            assert collapse(plan, bad, 2.0, 4, None, counts, nr, ns) == -1 and b"lo2" in lib.sg_last_error()
            assert collapse(plan, 1.0, bad, 4, None, counts, nr, ns) == -1 and b"thr2" in lib.sg_last_error()
        for lo2, thr2 in ((2.0, 2.0), (3.0, 2.0)):
            assert collapse(plan, lo2, thr2, 4, None, counts, nr, ns) == -1 and b"below thr2" in lib.sg_last_error()
        assert collapse(plan, 1.0, 2.0, 4, None, None, nr, ns) == -1 and b"null pointer" in lib.sg_last_error()
        assert collapse(plan, 1.0, 2.0, 4, None, counts, None, ns) == -1 and b"null pointer" in lib.sg_last_error()
        assert collapse(plan, 1.0, 2.0, 4, None, counts, nr, None) == -1 and b"null pointer" in lib.sg_last_error()
        assert (n_rounds.value, n_short.value) == (7, 7)                  # nothing was written by a refused call
        assert lib.sg_remesh_collapse_maps(plan, None, None, None) == 0   # the identity over no vertex
        assert collapse(plan, 1.0, 2.0, 4, None, counts, nr, ns) == 0
        assert (n_rounds.value, n_short.value) == (0, 0)
        assert collapse(plan, 1.0, 2.0, 0, None, None, nr, ns) == 0       # no round, no counts needed
        assert lib.sg_remesh_collapse_maps(plan, None, None, None) == 0
        assert lib.sg_remesh_query(plan, info) == 0
        assert list(info) == [0, 0, 0, 0, 0, 0, 0, 0, -1, -1, -1, -1, 0, 0, 1, 0]
    finally:
        assert lib.sg_remesh_destroy(plan) == 0


def test_python_functions_have_no_cpu_path():
    from semigcn_amd import remesh
    vs, faces = (torch.from_numpy(x) for x in RO.tetrahedron())
    with pytest.raises(capi.SemigcnLibraryError):
        remesh.collapse_short_edges(vs, faces, 0.5)
    with pytest.raises(capi.SemigcnLibraryError):
        remesh.refine_mesh((vs, faces), collapse=True)
    # the ValueErrors come before the device check
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="target"):
            remesh.collapse_short_edges(vs, faces, bad)
    with pytest.raises(ValueError, match="max_rounds"):
        remesh.collapse_short_edges(vs, faces, 0.5, max_rounds=-1)
    with pytest.raises(ValueError, match="collapse_rounds"):
        remesh.refine_mesh((vs, faces), collapse=True, collapse_rounds=-1)
    fn = lambda v, f: remesh.collapse_short_edges(v, f, 0.5)
    with pytest.raises(ValueError, match="vs must be"):
        fn(vs[:, :2], faces)
    with pytest.raises(ValueError, match="vs must hold floats"):
        fn(vs.long(), faces)
    with pytest.raises(ValueError, match="faces must be"):
        fn(vs, faces.reshape(-1))
    with pytest.raises(ValueError, match="faces must hold integers"):
        fn(vs, faces.float())
    assert remesh.collapse_threshold(1.25) == 1.0
    assert remesh.collapse_threshold(1.0) == float(np.float32(0.8 ** 2)) == float(CO.collapse_threshold(1.0))
    assert "Collapsed" in remesh.__all__ and "collapse_short_edges" in remesh.__all__
    assert "2a. collapse_short_edges" in remesh.__doc__


# ---- the oracle's own pins ---------------------------------------------------------------------------------------------
def _cands(vs, faces, target):
    return CO.collapse_candidates(vs, faces, CO.collapse_threshold(target), RO.split_threshold(target))


def test_oracle_fan():
    """Target 10: everything is short.  The rim is the border, so every spoke keeps its rim vertex and removes the hub; all
    footprints hold the hub and one spoke wins."""
    vs, faces = RO.fan8()
    cands = _cands(vs, faces, 10.0)
    assert sorted(cands) == [(0, i) for i in range(1, 9)]
    assert all((k, r) == (e[1], 0) and foot == frozenset(range(9)) for e, (_, k, r, foot) in cands.items())
    lo2, thr2 = CO.collapse_threshold(10.0), RO.split_threshold(10.0)
    (e, k, r, _), = CO.select_collapse(vs, faces, lo2, thr2)
    assert e == max(cands, key=lambda x: cands[x][0])
    out_vs, out_faces, ids, merged, counts, n_short = CO.collapse_short_edges(vs, faces, 10.0)
    assert counts == [1] and out_vs.shape[0] == 8 and out_faces.shape[0] == 6 and RO.euler(out_faces) == 1
    assert ids.tolist() == list(range(1, 9))                # every vertex index shifts down by one
    assert merged.tolist() == [k - 1] + list(range(8)) and np.array_equal(out_vs, vs[ids])
    assert RO.directed_once(out_faces) and (out_faces == k - 1).any(1).all()
    assert _cands(out_vs, out_faces, 10.0) == {}            # all border now: a second round finds nothing
    assert n_short == len(RO.edge_table(out_faces)[0]) == 13


def test_oracle_fold_over_guard():
    """Rim vertex 1 pulled inside the chord from 8 to 2: moving the hub to rim vertex 2, 7 or 8 would fold a face over."""
    vs, faces = RO.fan8(pulled=True)
    assert sorted(_cands(vs, faces, 10.0)) == [(0, i) for i in (1, 3, 4, 5, 6)]


def test_oracle_tetrahedron_has_no_candidate():
    vs, faces = RO.tetrahedron()
    assert _cands(vs, faces, 10.0) == {}
    out = CO.collapse_short_edges(vs, faces, 10.0)
    assert out[4] == [] and out[5] == 6 and np.array_equal(out[1], faces) and out[2].tolist() == out[3].tolist() == [0, 1, 2, 3]


def test_oracle_grids():
    vs, faces = RO.grid(3)
    out = CO.collapse_short_edges(vs, faces, 10.0)
    assert out[4] == [1, 1, 1, 1] and (out[0].shape[0], out[1].shape[0]) == (12, 10)
    # target 1.3: the 144 unit edges are short, and every collapse would create a knight's move, len2 = 5 > thr2 = 3.004
    vs, faces = RO.grid(8)
    lo2, thr2 = CO.collapse_threshold(1.3), RO.split_threshold(1.3)
    assert CO.n_short(vs, faces, lo2) == 144 and 3.0 < float(thr2) < 3.01
    out = CO.collapse_short_edges(vs, faces, 1.3)
    assert out[4] == [] and out[5] == 144 and np.array_equal(out[1], faces)
    out = CO.collapse_short_edges(vs, faces, 2.0)
    assert (sum(out[4]), len(out[4])) == (33, 14) and (out[0].shape[0], out[1].shape[0]) == (48, 62) and out[5] == 63
    assert float(RO.max_len2(out[0], out[1])) == 5.0 <= float(RO.split_threshold(2.0))
    assert RO.euler(out[1]) == 1 and RO.directed_once(out[1])


def test_oracle_invariants_on_the_stretched_torus():
    vs, faces = RO.stretched_torus(20, 12)
    target = 1.8 * RO.median_edge(vs, faces)
    lo2, thr2 = CO.collapse_threshold(target), RO.split_threshold(target)
    assert CO.n_short(vs, faces, lo2) == 517
    long_before = {tuple(vs[list(e)].ravel().tolist()) for e in RO.edge_table(faces)[0] if RO.len2(vs, *e) > thr2}
    cur_vs, cur_faces, rounds = vs, faces, 0
    while True:
        new_vs, new_faces, keep, old_to_new, selected = CO.collapse_round(cur_vs, cur_faces, lo2, thr2)
        if not selected:
            break
        used = [v for _, _, _, foot in selected for v in foot]
        assert len(used) == len(set(used))                  # footprints pairwise disjoint
        assert all(k in foot and r in foot for _, k, r, foot in selected)
        cur_vs, cur_faces, rounds = new_vs, new_faces, rounds + 1
        assert RO.directed_once(cur_faces) and RO.euler(cur_faces) == 0
    assert rounds == 33 and (cur_vs.shape[0], cur_faces.shape[0]) == (97, 194)
    out = CO.collapse_short_edges(vs, faces, target)
    assert np.array_equal(out[0], cur_vs) and np.array_equal(out[1], cur_faces) and len(out[4]) == 33 and out[5] == 94
    assert RO.check_input(out[0], out[1])["n_nonmanifold"] == 0
    for e in RO.edge_table(out[1])[0]:                      # no long edge that was not there before (ends never move)
        assert not RO.len2(out[0], *e) > thr2 or tuple(out[0][list(e)].ravel().tolist()) in long_before
    assert np.array_equal(out[0], vs[out[2]]) and np.array_equal(out[3][out[2]], np.arange(97))
