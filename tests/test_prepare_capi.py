"""semigcn_amd.prepare below the C ABI (csrc/mesh_smooth.hip), without a device: the entry points exist in the header, the
ctypes table and the library; they reject bad arguments before touching a device; the Python functions have no CPU path;
write_obj is the inverse of read_obj; and the float64 oracle the GPU tests compare against (tests/prepare_oracle.py)
gives the hand-computed answers on a single triangle and on a tetrahedron."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import prepare_oracle as PO
from semigcn_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sg_edge_length_blocks", "sg_mean_edge_length", "sg_smooth_create", "sg_smooth_run", "sg_smooth_destroy")


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
    buf = (ctypes.c_double * 16)()         # host memory: every call below must return before it would be touched
    p = ctypes.c_void_p(ctypes.addressof(buf))
    plan = ctypes.c_void_p()

    assert lib.sg_edge_length_blocks(-1) == -1
    assert lib.sg_edge_length_blocks(0) == 1 and lib.sg_edge_length_blocks(256) == 1 and lib.sg_edge_length_blocks(257) == 2
    assert lib.sg_edge_length_blocks(10 ** 9) == lib.sg_edge_length_blocks(10 ** 8)       # capped: a fixed reduction tree

    mel = lib.sg_mean_edge_length
    assert mel(p, -1, p, 1, p, p, None) == -1 and b"negative" in lib.sg_last_error()
    assert mel(p, 4, p, -1, p, p, None) == -1 and b"negative" in lib.sg_last_error()
    assert mel(p, 4, p, 1, None, p, None) == -1 and b"null pointer" in lib.sg_last_error()
    assert mel(p, 4, p, 1, p, None, None) == -1 and b"null pointer" in lib.sg_last_error()
    assert mel(None, 4, p, 1, p, p, None) == -1 and b"null pointer" in lib.sg_last_error()
    assert mel(p, 4, None, 1, p, p, None) == -1 and b"null pointer" in lib.sg_last_error()

    create = lib.sg_smooth_create
    assert create(p, 2, 4, None, None) == -1 and b"null out" in lib.sg_last_error()
    assert create(p, -1, 4, None, ctypes.byref(plan)) == -1 and b"negative" in lib.sg_last_error() and not plan.value
    assert create(p, 2, -1, None, ctypes.byref(plan)) == -1 and b"negative" in lib.sg_last_error() and not plan.value
    assert create(None, 2, 4, None, ctypes.byref(plan)) == -1 and b"null pointer" in lib.sg_last_error() and not plan.value

    run = lib.sg_smooth_run
    assert run(None, p, p, None, -1, None) == -1 and b"negative steps" in lib.sg_last_error()
    assert run(p, p, p, None, -3, None) == -1 and b"negative steps" in lib.sg_last_error()      # before the plan is looked at
    assert run(None, p, p, None, 1, None) == -1 and b"null plan" in lib.sg_last_error()
    assert run(None, p, p, None, 0, None) == -1 and b"null plan" in lib.sg_last_error()

    assert lib.sg_smooth_destroy(None) == 0


def test_python_functions_have_no_cpu_path():
    from semigcn_amd import prepare
    vs = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    faces = torch.tensor([[0, 1, 2]])
    edges = torch.tensor([[0, 1], [1, 2], [0, 2]])
    with pytest.raises(capi.SemigcnLibraryError):
        prepare.mean_edge_length(vs, edges)
    with pytest.raises(capi.SemigcnLibraryError):
        prepare.laplacian_smooth(vs, faces)
    with pytest.raises(capi.SemigcnLibraryError):
        prepare.SmoothPlan(faces, 3)
    with pytest.raises(capi.SemigcnLibraryError):
        prepare.scan_mask(vs, (vs, faces))
    with pytest.raises(capi.SemigcnLibraryError):
        prepare.prepare_inputs((vs, faces), (vs, faces))
    with pytest.raises(capi.SemigcnLibraryError):
        prepare.prepare_inputs((vs, faces), (vs, faces), gt=(vs, faces), rescale=False, device="cpu")
    # a negative step count is refused before anything else is looked at
    with pytest.raises(ValueError, match="steps"):
        prepare.laplacian_smooth(vs, faces, steps=-1)
    with pytest.raises(ValueError, match="steps"):
        prepare.prepare_inputs((vs, faces), (vs, faces), steps=-1)


def test_write_obj_read_obj_roundtrip(tmp_path):
    from semigcn_amd.evaluate import read_obj
    from semigcn_amd.prepare import write_obj
    rng = np.random.default_rng(5)
    vs = (rng.standard_normal((500, 3)) * np.exp(rng.uniform(-20, 20, (500, 1)))).astype(np.float32)
    vs[:4] = np.array([[0.0, -0.0, 1.0], [1e-38, 3.4e38, -1e-45], [1 / 3, 2 / 3, 0.1], [16777216.0, 16777217.0, -5e-7]], np.float32)
    faces = rng.integers(0, 500, (300, 3))
    path = str(tmp_path / "a.obj")
    write_obj(path, vs, faces)
    v2, f2 = read_obj(path)
    assert v2.dtype == np.float32 and np.array_equal(v2.view(np.uint32), vs.view(np.uint32))
    assert f2.dtype == np.int64 and np.array_equal(f2, faces)
    write_obj(path, torch.from_numpy(vs), torch.from_numpy(faces))          # tensors as well
    v3, f3 = read_obj(path)
    assert np.array_equal(v3.view(np.uint32), vs.view(np.uint32)) and np.array_equal(f3, faces)
    write_obj(path, vs[:7])                                                   # vertices only (<name>_inserted.obj)
    v4, f4 = read_obj(path)
    assert np.array_equal(v4.view(np.uint32), vs[:7].view(np.uint32)) and f4.shape == (0, 3)
    assert open(path).read().count("\n") == 7


def test_oracle_single_triangle():
    """Every edge is a border edge, every vertex a border vertex with weight 1 on both its edges: one step moves each
    vertex to the mean of all three."""
    p = np.array([[0.0, 0, 0], [3, 0, 0], [0, 6, 3]])
    faces = np.array([[0, 1, 2]])
    out = PO.smooth_step(p, faces)
    assert np.allclose(out, np.tile(p.mean(0), (3, 1)), rtol=0, atol=1e-15)
    assert np.array_equal(PO.smooth(p, faces, 0), p)
    d_max, C = PO.neighbour_lists(faces, 3)
    assert d_max == 2 and np.array_equal(C, [2.0, 2.0, 2.0])
    # a fixed vertex stays, the others still read it
    out = PO.smooth_step(p, faces, movable=[False, True, True])
    assert np.array_equal(out[0], p[0]) and np.allclose(out[1:], np.tile(p.mean(0), (2, 1)), rtol=0, atol=1e-15)


def test_oracle_tetrahedron():
    """Closed: every edge has two faces, every neighbour weighs 2 -- p' = (p + 2 sum of the other three) / 7."""
    p = np.array([[0.0, 0, 0], [1, 0, 0], [0, 2, 0], [0.5, 0.25, 4]])
    faces = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    out = PO.smooth_step(p, faces)
    total = p.sum(0)
    want = np.stack([(p[i] + 2.0 * (total - p[i])) / 7.0 for i in range(4)])
    assert np.allclose(out, want, rtol=0, atol=1e-15)
    d_max, C = PO.neighbour_lists(faces, 4)
    assert d_max == 3 and np.array_equal(C, [6.0] * 4)
    # the operator is symmetric on a closed mesh: sum_i (1 + sum_j w_ij) p_i is conserved
    assert np.allclose((7.0 * out).sum(0), (7.0 * p).sum(0), rtol=0, atol=1e-13)
    # an isolated fifth vertex keeps its position
    p5 = np.concatenate([p, [[9.0, 9, 9]]])
    assert np.array_equal(PO.smooth(p5, faces, 3)[4], p5[4])


def test_oracle_open_strip_border_rule():
    """Two triangles sharing the edge 1-2: all four vertices are border vertices; 1 and 2 ignore their shared interior
    edge (weight 0) and average over their two border edges only."""
    p = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 5]])
    faces = np.array([[0, 1, 2], [1, 3, 2]])
    out = PO.smooth_step(p, faces)
    assert np.allclose(out[1], (p[1] + p[0] + p[3]) / 3.0, rtol=0, atol=1e-15)
    assert np.allclose(out[2], (p[2] + p[0] + p[3]) / 3.0, rtol=0, atol=1e-15)
    assert np.allclose(out[0], (p[0] + p[1] + p[2]) / 3.0, rtol=0, atol=1e-15)


def test_oracle_mean_edge_length():
    p = np.array([[0.0, 0, 0], [3, 0, 0], [0, 4, 0]])
    e = PO.unique_edges(np.array([[0, 1, 2]]), 3)
    assert e.shape == (3, 2) and PO.mean_edge_length(p, e) == 4.0
    assert np.isnan(PO.mean_edge_length(p, np.zeros((0, 2), np.int64)))
