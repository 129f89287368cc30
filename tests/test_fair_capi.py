"""The thin-plate fairing below and above the C ABI (csrc/mesh_fair.hip), without a device: the entry points exist in the
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
NEW = ("sg_fair_create", "sg_fair_destroy", "sg_fair_query", "sg_fair_diagonal", "sg_fair_apply", "sg_fair_solve")


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
    buf = (ctypes.c_int64 * 16)()          # host memory: every call below must return before it would be touched
    p = ctypes.c_void_p(ctypes.addressof(buf))
    q = ctypes.c_void_p(ctypes.addressof(buf) + 64)
    plan = ctypes.c_void_p()
    it, ok, res = ctypes.c_int64(), ctypes.c_int(), (ctypes.c_double * 3)()

    create = lib.sg_fair_create
    assert create(p, 2, 4, p, None, None) == -1 and b"null out" in lib.sg_last_error()
    assert create(p, -1, 4, p, None, ctypes.byref(plan)) == -1 and b"negative" in lib.sg_last_error() and not plan.value
    assert create(p, 2, -1, p, None, ctypes.byref(plan)) == -1 and b"negative" in lib.sg_last_error() and not plan.value
    assert create(None, 2, 4, p, None, ctypes.byref(plan)) == -1 and b"null pointer" in lib.sg_last_error() and not plan.value
    assert create(p, 2, 4, None, None, ctypes.byref(plan)) == -1 and b"null pointer" in lib.sg_last_error() and not plan.value

    assert lib.sg_fair_query(None, buf) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_fair_diagonal(None, p, None) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_fair_apply(None, p, q, None) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_fair_solve(None, p, p, 1e-10, 10, 32, None, ctypes.byref(it), res, ctypes.byref(ok)) == -1
    assert b"null plan" in lib.sg_last_error()
    assert lib.sg_fair_destroy(None) == 0

    # an empty mesh makes a plan without touching a device; the argument checks of the calls on it come first
    assert create(None, 0, 0, None, None, ctypes.byref(plan)) == 0 and plan.value
    info = (ctypes.c_int64 * 8)()
    assert lib.sg_fair_query(plan, info) == 0 and list(info)[:5] == [0, 0, 0, -1, 0] and info[6] <= 4
    assert lib.sg_fair_apply(plan, p, p, None) == -1 and b"q is p" in lib.sg_last_error()
    assert lib.sg_fair_apply(plan, None, q, None) == -1 and b"null pointer" in lib.sg_last_error()
    solve = lib.sg_fair_solve
    assert solve(plan, p, p, -1.0, 10, 32, None, ctypes.byref(it), res, ctypes.byref(ok)) == -1 and b"tol" in lib.sg_last_error()
    assert solve(plan, p, p, 1e-10, -1, 32, None, ctypes.byref(it), res, ctypes.byref(ok)) == -1 and b"max_iter" in lib.sg_last_error()
    assert solve(plan, p, p, 1e-10, 10, 0, None, ctypes.byref(it), res, ctypes.byref(ok)) == -1 and b"check_every" in lib.sg_last_error()
    assert solve(plan, None, p, 1e-10, 10, 32, None, ctypes.byref(it), res, ctypes.byref(ok)) == -1
    assert solve(plan, p, p, 1e-10, 10, 32, None, ctypes.byref(it), res, ctypes.byref(ok)) == 0       # V = 0: nothing to do
    assert (it.value, ok.value, list(res)) == (0, 1, [0.0, 0.0, 0.0])
    assert lib.sg_fair_destroy(plan) == 0


def test_python_errors_come_before_any_device():
    from semigcn_amd import holes, repair
    vs = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    faces = torch.tensor([[0, 1, 3], [1, 2, 3], [2, 0, 3]])
    free = torch.tensor([False, False, False, True])
    with pytest.raises(ValueError, match="fair must be one of"):
        holes.fill_holes((vs, faces), fair="membrane")
    with pytest.raises(ValueError, match="fair must be"):
        repair.repair((vs, faces), fair="membrane")
    with pytest.raises(ValueError, match="fair must be"):
        repair.remove_self_intersections((vs, faces), fair="membrane")
    with pytest.raises(ValueError, match="max_iter"):
        holes.fair_thin_plate(vs, faces, free, max_iter=-1)
    with pytest.raises(ValueError, match="max_iter"):
        holes.fill_holes((vs, faces), fair="thin_plate", fair_max_iter=-1)
    with pytest.raises(ValueError, match="tol"):
        holes.fair_thin_plate(vs, faces, free, tol=-1e-3)
    with pytest.raises(ValueError, match="tol"):
        holes.fill_holes((vs, faces), fair="thin_plate", fair_tol=float("nan"))
    with pytest.raises(ValueError, match="check_every"):
        holes.fair_thin_plate(vs, faces, free, check_every=0)
    with pytest.raises(ValueError, match=r"one entry per vertex \(4\), got 3"):
        holes.fair_thin_plate(vs, faces, free[:3])
    with pytest.raises(ValueError, match=r"one entry per vertex \(4\), got 5"):
        holes.fair_thin_plate(vs.numpy(), faces.numpy(), np.zeros(5, bool))
    with pytest.raises(ValueError, match=r"vs must be \[V, 3\]"):
        holes.fair_thin_plate(vs[:, :2], faces, free)
    with pytest.raises(ValueError, match="faces must hold integers"):
        holes.fair_thin_plate(vs, faces.float(), free)


def test_python_functions_have_no_cpu_path():
    from semigcn_amd import holes
    vs = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    faces = torch.tensor([[0, 1, 3], [1, 2, 3], [2, 0, 3]])
    free = torch.tensor([False, False, False, True])
    with pytest.raises(capi.SemigcnLibraryError):
        holes.fair_thin_plate(vs, faces, free)
    with pytest.raises(capi.SemigcnLibraryError):
        holes.fill_holes((vs, faces), fair="thin_plate")
    with pytest.raises(capi.SemigcnLibraryError):
        holes.FairPlan(faces, 4, free)
    assert "fair_thin_plate" in holes.__all__ and "FairPlan" in holes.__all__
