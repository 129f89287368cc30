"""The crease entry points of csrc/mesh_remesh.hip below the C ABI, without a device: they are declared in the header, bound in
the ctypes table and exported by the library; they reject bad arguments before touching a device; the empty plan reports no
crease; and the Python functions raise their ValueErrors for a bad ``feature_angle`` before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import remesh_oracle as RO
from semigcn_amd import capi, remesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sg_remesh_set_feature", "sg_remesh_features", "sg_remesh_crease_edges", "sg_crease_step")


def test_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "semigcn.h")).read()
    declared = re.findall(r"^SG_API\s+[\w\s\*]+?\b(sg_\w+)\s*\(", text, flags=re.M)
    lib = ctypes.CDLL(capi.library_path())
    for name in NEW:
        assert name in declared, name
        assert name in capi._SIGNATURES, name
        assert hasattr(lib, name), name
    assert callable(capi.RemeshPlan.set_feature) and callable(capi.RemeshPlan.features) and callable(capi.crease_step)


def test_null_plan_and_argument_errors_without_gpu():
    lib = capi.load()
    buf = (ctypes.c_int64 * 16)()          # host memory: every call below must return before it would be touched
    p = ctypes.c_void_p(ctypes.addressof(buf))
    n = ctypes.c_int64()
    assert lib.sg_remesh_set_feature(None, 1, 0.5) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_remesh_features(None, None, p, p, ctypes.byref(n)) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_remesh_crease_edges(None, p, None) == -1 and b"null plan" in lib.sg_last_error()
    step = lib.sg_crease_step
    assert step(p, p, p, -1, None) == -1 and b"negative" in lib.sg_last_error()
    assert step(None, p, p, 4, None) == -1 and b"null pointer" in lib.sg_last_error()
    assert step(p, None, p, 4, None) == -1 and b"null pointer" in lib.sg_last_error()
    assert step(p, ctypes.c_void_p(p.value + 64), None, 4, None) == -1 and b"null pointer" in lib.sg_last_error()
    assert step(p, p, p, 4, None) == -1 and b"in place" in lib.sg_last_error()
    assert step(None, None, None, 0, None) == 0


def test_empty_plan_reports_no_crease():
    """V = F = 0 needs no device: the setting, the query and the edge list can be exercised on it."""
    lib = capi.load()
    plan = ctypes.c_void_p()
    n = ctypes.c_int64(7)
    assert lib.sg_remesh_create(None, 0, None, 0, None, ctypes.byref(plan)) == 0 and plan.value
    try:
        assert lib.sg_remesh_crease_edges(plan, None, None) == -1 and b"sg_remesh_features first" in lib.sg_last_error()
        assert lib.sg_remesh_features(plan, None, None, None, None) == -1 and b"null pointer" in lib.sg_last_error()
        assert lib.sg_remesh_features(plan, None, None, None, ctypes.byref(n)) == 0 and n.value == 0
        assert lib.sg_remesh_crease_edges(plan, None, None) == 0
        for bad in (1.0, -1.0, 1.5, float("nan")):
            assert lib.sg_remesh_set_feature(plan, 1, bad) == -1 and b"cos_t" in lib.sg_last_error()
        assert lib.sg_remesh_set_feature(plan, 0, float("nan")) == 0          # off: the value is not looked at
        assert lib.sg_remesh_set_feature(plan, 1, 0.5) == 0
        assert lib.sg_remesh_crease_edges(plan, None, None) == -1            # the setting changed: ask again
        n.value = 7
        assert lib.sg_remesh_features(plan, None, None, None, ctypes.byref(n)) == 0 and n.value == 0
        assert lib.sg_remesh_set_feature(plan, 1, -0.5) == 0 and lib.sg_remesh_set_feature(plan, 0, 0.0) == 0
    finally:
        assert lib.sg_remesh_destroy(plan) == 0


def test_feature_cos():
    assert remesh.feature_cos(30) == float(np.cos(np.radians(np.float64(30.0))))
    assert remesh.feature_cos(90.0) == float(np.cos(np.radians(np.float64(90.0)))) and abs(remesh.feature_cos(90.0)) < 1e-16
    assert remesh.feature_cos(120) < 0 < remesh.feature_cos(60)
    for bad in (0, 180, -5.0, 200.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="feature_angle"):
            remesh.feature_cos(bad)


def test_bad_feature_angle_raises_before_the_device_check():
    """On this machine's CPU tensors every function would raise SemigcnLibraryError; the ValueError comes first."""
    vs, faces = (torch.from_numpy(x) for x in RO.tetrahedron())
    for bad in (0, 180, float("nan")):
        with pytest.raises(ValueError, match="feature_angle"):
            remesh.flip_edges(vs, faces, feature_angle=bad)
        with pytest.raises(ValueError, match="feature_angle"):
            remesh.collapse_short_edges(vs, faces, 0.5, feature_angle=bad)
        with pytest.raises(ValueError, match="feature_angle"):
            remesh.relax_project(vs, faces, (vs, faces), feature_angle=bad)
        with pytest.raises(ValueError, match="feature_angle"):
            remesh.refine_mesh((vs, faces), target=0.5, feature_angle=bad)
    with pytest.raises(ValueError, match="creases needs feature_angle"):
        remesh.relax_project(vs, faces, (vs, faces), creases=[[0, 1]])
    with pytest.raises(capi.SemigcnLibraryError):                      # a good angle: no CPU path
        remesh.refine_mesh((vs, faces), target=0.5, feature_angle=30)
    with pytest.raises(capi.SemigcnLibraryError):
        capi.crease_step(vs, torch.zeros((4, 2), dtype=torch.int64))


def test_box_mesh_is_a_closed_cube_with_shared_edges():
    from semigcn_amd import synth
    for n in (1, 2, 5):
        vs, faces = synth.box_mesh(n)
        assert vs.dtype == np.float32 and faces.dtype == np.int64
        assert vs.shape == (6 * n * n + 2, 3) and faces.shape == (12 * n * n, 3)
        RO.check_input(vs, faces)
        assert RO.euler(faces) == 2 and not RO.valences(faces)[1]
        p = vs.astype(np.float64)
        a, b, c = (p[faces[:, k]] for k in range(3))
        assert abs(float((a * np.cross(b, c)).sum() / 6.0) - 1.0) < 1e-12
    with pytest.raises(ValueError):
        synth.box_mesh(0)
