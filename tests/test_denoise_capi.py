"""The vertex update below and above the C ABI (csrc/mesh_denoise.hip), without a device: the entry points exist in the
header, the ctypes table and the library; they reject bad arguments before touching a device; the Python functions raise
their argument errors before any device is asked for and have no CPU path."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from semigcn_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sg_vupdate_create", "sg_vupdate_destroy", "sg_vupdate_query", "sg_vupdate_run")


def test_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "semigcn.h")).read()
    declared = re.findall(r"^SG_API\s+[\w\s\*]+?\b(sg_\w+)\s*\(", text, flags=re.M)
    lib = ctypes.CDLL(capi.library_path())
    for name in NEW:
        assert name in declared, name
        assert name in capi._SIGNATURES, name
        assert hasattr(lib, name), name
    assert capi.load().sg_abi_version() == 1


def test_argument_validation_without_gpu():
    lib = capi.load()
    buf = (ctypes.c_int64 * 32)()          # host memory: every call below must return before it would be touched
    p = ctypes.c_void_p(ctypes.addressof(buf))
    q = ctypes.c_void_p(ctypes.addressof(buf) + 128)
    plan = ctypes.c_void_p()

    create = lib.sg_vupdate_create
    assert create(p, 2, 4, None, None) == -1 and b"null out" in lib.sg_last_error()
    assert create(p, -1, 4, None, ctypes.byref(plan)) == -1 and b"negative" in lib.sg_last_error() and not plan.value
    assert create(p, 2, -1, None, ctypes.byref(plan)) == -1 and b"negative" in lib.sg_last_error() and not plan.value
    assert create(None, 2, 4, None, ctypes.byref(plan)) == -1 and b"null pointer" in lib.sg_last_error() and not plan.value
    assert create(p, 2, 0, None, ctypes.byref(plan)) == -1 and b"outside [0, 0)" in lib.sg_last_error() and not plan.value
    assert create(p, 1 << 30, 4, None, ctypes.byref(plan)) == -1 and b"int32" in lib.sg_last_error() and not plan.value

    assert lib.sg_vupdate_query(None, buf) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_vupdate_run(None, p, p, None, 1, q, None) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_vupdate_destroy(None) == 0

    # a mesh without faces makes a plan without touching a device; the argument checks of the calls on it come first
    info = (ctypes.c_int64 * 4)()
    for V in (0, 5):
        assert create(None, 0, V, None, ctypes.byref(plan)) == 0 and plan.value
        assert lib.sg_vupdate_query(plan, None) == -1 and b"null pointer" in lib.sg_last_error()
        assert lib.sg_vupdate_query(plan, info) == 0 and list(info) == [V, 0, 0, V]
        run = lib.sg_vupdate_run
        assert run(plan, p, p, None, -1, q, None) == -1 and b"negative steps" in lib.sg_last_error()
        assert run(plan, None, p, None, 1, q, None) == -1 and b"null pointer" in lib.sg_last_error()
        assert run(plan, p, None, None, 1, q, None) == -1 and b"null pointer" in lib.sg_last_error()
        assert run(plan, p, p, None, 1, None, None) == -1 and b"null pointer" in lib.sg_last_error()
        assert run(plan, p, q, None, 1, p, None) == -1 and b"out is pos" in lib.sg_last_error()
        if V:      # 15 floats from p reach into the 15 floats that start 8 floats later
            o = ctypes.c_void_p(ctypes.addressof(buf) + 32)
            assert run(plan, p, q, None, 1, o, None) == -1 and b"overlaps" in lib.sg_last_error()
        else:
            assert run(plan, p, p, None, 3, q, None) == 0       # V = 0: nothing to do
        assert lib.sg_vupdate_destroy(plan) == 0


def test_python_errors_come_before_any_device():
    from semigcn_amd import denoise
    vs = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    faces = torch.tensor([[0, 1, 3], [1, 2, 3], [2, 0, 3]])
    n = torch.zeros(3, 3)
    with pytest.raises(ValueError, match="steps must be >= 0"):
        denoise.update_vertices(vs, faces, n, -1)
    with pytest.raises(ValueError, match=r"normals must be \[F, 3\] = \[3, 3\], got \(4, 3\)"):
        denoise.update_vertices(vs, faces, torch.zeros(4, 3))
    with pytest.raises(ValueError, match=r"normals must be \[F, 3\]"):
        denoise.update_vertices(vs.numpy(), faces.numpy(), np.zeros(9, np.float32))
    with pytest.raises(ValueError, match=r"one entry per vertex \(4\), got 3"):
        denoise.update_vertices(vs, faces, n, movable=torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"vs must be \[V, 3\]"):
        denoise.update_vertices(vs[:, :2], faces, n)
    with pytest.raises(ValueError, match="faces must hold integers"):
        denoise.update_vertices(vs, faces.float(), n)
    for key in ("iterations", "normal_rounds", "vertex_steps"):
        with pytest.raises(ValueError, match=f"{key} must be >= 0"):
            denoise.denoise_mesh(vs, faces, **{key: -1})
    for bad in (0.0, -0.3, float("nan")):
        with pytest.raises(ValueError, match="sigma_s must be > 0"):
            denoise.denoise_mesh(vs, faces, sigma_s=bad)
    with pytest.raises(ValueError, match=r"one entry per vertex \(4\), got 5"):
        denoise.denoise_mesh(vs, faces, movable=np.zeros(5, bool))
    with pytest.raises(ValueError, match=r"f2f must be \[F, 3\]"):
        denoise.denoise_mesh(vs, faces, f2f=torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="no faces"):
        denoise.denoise_mesh(vs, faces[:0])
    with pytest.raises(ValueError, match="steps must be >= 0"):
        capi.VertexUpdatePlan.run(object.__new__(capi.VertexUpdatePlan), vs, n, None, -2)


def test_python_functions_have_no_cpu_path():
    from semigcn_amd import denoise
    vs = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    faces = torch.tensor([[0, 1, 3], [1, 2, 3], [2, 0, 3]])
    with pytest.raises(capi.SemigcnLibraryError):
        denoise.update_vertices(vs, faces, torch.zeros(3, 3))
    with pytest.raises(capi.SemigcnLibraryError):
        denoise.denoise_mesh(vs, faces)
    with pytest.raises(capi.SemigcnLibraryError):
        denoise.VertexUpdatePlan(faces, 4)
    assert "update_vertices" in denoise.__all__ and "denoise_mesh" in denoise.__all__ and "VertexUpdatePlan" in denoise.__all__
