"""semigcn_amd.simplify below the C ABI (csrc/mesh_remesh.hip), without a device: the entry points exist in the header, the
ctypes table and the library; they reject bad arguments before touching a device and a refused call writes nothing; the
Python functions have no CPU path and raise their ValueErrors first."""
import ctypes
import os
import re

import pytest
import torch

import remesh_oracle as RO
from semigcn_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sg_remesh_simplify", "sg_remesh_quadrics")


def test_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "semigcn.h")).read()
    declared = re.findall(r"^SG_API\s+[\w\s\*]+?\b(sg_\w+)\s*\(", text, flags=re.M)
    lib = ctypes.CDLL(capi.library_path())
    for name in NEW:
        assert name in declared, name
        assert name in capi._SIGNATURES, name
        assert hasattr(lib, name), name
    assert "SG_QUADRICS_OWN = 0" in text and "SG_QUADRICS_SUM = 1" in text
    assert capi.RemeshPlan.QUADRICS == {"own": 0, "sum": 1} and callable(capi.RemeshPlan.simplify)
    assert "whichever ran last" in text                        # sg_remesh_collapse_maps serves both


def test_argument_validation_on_the_empty_plan_and_a_refused_call_writes_nothing():
    """V = F = 0 needs no device: every refusal is exercised on it, and counts / n_rounds / n_refused keep their bytes."""
    lib = capi.load()
    simplify = lib.sg_remesh_simplify
    counts = (ctypes.c_int64 * 12)(*([7] * 12))
    n_rounds, n_refused = ctypes.c_int64(7), ctypes.c_int64(7)
    r, f = ctypes.byref(n_rounds), ctypes.byref(n_refused)
    untouched = lambda: list(counts) == [7] * 12 and (n_rounds.value, n_refused.value) == (7, 7)
    assert simplify(None, 0, 0, 4, None, counts, r, f) == -1 and b"null plan" in lib.sg_last_error() and untouched()
    assert lib.sg_remesh_quadrics(None, None, None) == -1 and b"null plan" in lib.sg_last_error()
    plan = ctypes.c_void_p()
    assert lib.sg_remesh_create(None, 0, None, 0, None, ctypes.byref(plan)) == 0 and plan.value
    try:
        assert simplify(plan, -1, 0, 4, None, counts, r, f) == -1 and b"target_v" in lib.sg_last_error() and untouched()
        assert simplify(plan, 0, 0, -1, None, counts, r, f) == -1 and b"max_rounds" in lib.sg_last_error() and untouched()
        for mode in (-1, 2, 7):
            assert simplify(plan, 0, mode, 4, None, counts, r, f) == -1 and b"quadrics_mode" in lib.sg_last_error() and untouched()
        assert simplify(plan, 0, 0, 4, None, None, r, f) == -1 and b"null pointer" in lib.sg_last_error() and untouched()
        assert simplify(plan, 0, 0, 4, None, counts, None, f) == -1 and b"null pointer" in lib.sg_last_error() and untouched()
        assert simplify(plan, 0, 0, 4, None, counts, r, None) == -1 and b"null pointer" in lib.sg_last_error() and untouched()
        # the crease rules: crease-aware simplification is not part of the stage
        assert lib.sg_remesh_set_feature(plan, 1, 0.5) == 0
        assert simplify(plan, 0, 1, 4, None, counts, r, f) == -1 and b"crease" in lib.sg_last_error() and untouched()
        assert lib.sg_remesh_set_feature(plan, 0, 0.0) == 0
        # accepted: nothing to do, no device asked
        assert simplify(plan, 0, 1, 4, None, counts, r, f) == 0 and (n_rounds.value, n_refused.value) == (0, 0)
        assert simplify(plan, 5, 0, 0, None, None, r, f) == 0 and list(counts) == [7] * 12
        assert lib.sg_remesh_quadrics(plan, None, None) == 0
        assert lib.sg_remesh_collapse_maps(plan, None, None, None) == 0
    finally:
        assert lib.sg_remesh_destroy(plan) == 0


def test_simplify_mesh_has_no_cpu_path_and_raises_its_value_errors_first():
    from semigcn_amd import simplify
    vs, faces = (torch.from_numpy(x) for x in RO.tetrahedron())
    with pytest.raises(capi.SemigcnLibraryError):
        simplify.simplify_mesh(vs, faces, target_v=3)
    with pytest.raises(ValueError, match="exactly one"):
        simplify.simplify_mesh(vs, faces)
    with pytest.raises(ValueError, match="exactly one"):
        simplify.simplify_mesh(vs, faces, target_v=3, ratio=0.5)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ratio"):
            simplify.simplify_mesh(vs, faces, ratio=bad)
    for bad in (5, -1):
        with pytest.raises(ValueError, match="target_v"):
            simplify.simplify_mesh(vs, faces, target_v=bad)
    with pytest.raises(ValueError, match="quadrics"):
        simplify.simplify_mesh(vs, faces, target_v=3, quadrics="mean")
    with pytest.raises(ValueError, match="max_rounds"):
        simplify.simplify_mesh(vs, faces, target_v=3, max_rounds=-1)
    with pytest.raises(ValueError, match="vs must be"):
        simplify.simplify_mesh(vs[:, :2], faces, target_v=3)
    with pytest.raises(ValueError, match="faces must hold integers"):
        simplify.simplify_mesh(vs, faces.float(), target_v=3)
    assert simplify.resolve_target(258, ratio=0.6) == 154 and simplify.resolve_target(258, ratio=1.0) == 258
    assert simplify.resolve_target(258, target_v=0) == 0


def test_device_mesh_rejects_unknown_criteria_before_any_device():
    from semigcn_amd import meshprep
    vs, faces = RO.tetrahedron()
    with pytest.raises(ValueError, match="criterion"):
        meshprep.DeviceMesh(vs, faces, "cuda", criterion="quadric")
    assert meshprep.DeviceMesh.CRITERIA == ("qem", "length", "collapse")
