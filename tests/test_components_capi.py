"""semigcn_amd.components below the C ABI (csrc/mesh_parts.hip), without a device: the entry points exist in the header, the
ctypes table and the library; they reject bad arguments before touching a device; the Python functions have no CPU path and
raise their ValueErrors first; and the numpy oracle the GPU tests compare against (tests/components_oracle.py) gives the
hand-computed answers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import components_oracle as CO
from semigcn_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sg_parts_create", "sg_parts_destroy", "sg_parts_query", "sg_parts_labels", "sg_parts_select", "sg_parts_emit")


def test_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "semigcn.h")).read()
    declared = re.findall(r"^SG_API\s+[\w\s\*]+?\b(sg_\w+)\s*\(", text, flags=re.M)
    lib = ctypes.CDLL(capi.library_path())
    for name in NEW:
        assert name in declared, name
        assert name in capi._SIGNATURES, name
        assert hasattr(lib, name), name
    assert "typedef struct sg_parts sg_parts;" in text
    assert capi.load().sg_abi_version() == 1
    assert callable(capi.PartsPlan.close) and callable(capi.PartsPlan.__del__)


def test_argument_validation_without_gpu():
    lib = capi.load()
    buf = (ctypes.c_int64 * 16)()          # host memory: every call below must return before it would be touched
    p = ctypes.c_void_p(ctypes.addressof(buf))
    plan = ctypes.c_void_p()
    n = ctypes.c_int64()

    create = lib.sg_parts_create
    assert create(p, 2, 4, 0, None, None) == -1 and b"null out" in lib.sg_last_error()
    assert create(p, -1, 4, 0, None, ctypes.byref(plan)) == -1 and b"negative" in lib.sg_last_error() and not plan.value
    assert create(p, 2, -1, 0, None, ctypes.byref(plan)) == -1 and b"negative" in lib.sg_last_error() and not plan.value
    for bad in (-1, 2, 7):
        assert create(p, 2, 4, bad, None, ctypes.byref(plan)) == -1 and b"connectivity" in lib.sg_last_error() and not plan.value
    assert create(None, 2, 4, 0, None, ctypes.byref(plan)) == -1 and b"null pointer" in lib.sg_last_error() and not plan.value
    assert create(None, 2, 4, 1, None, ctypes.byref(plan)) == -1 and b"null pointer" in lib.sg_last_error() and not plan.value
    # sizes the 32-bit sort and parents cannot hold
    assert create(p, (1 << 31) // 3 + 1, 4, 0, None, ctypes.byref(plan)) == -1 and b"int32" in lib.sg_last_error() and not plan.value
    assert create(p, 2, 1 << 31, 1, None, ctypes.byref(plan)) == -1 and b"int32" in lib.sg_last_error() and not plan.value

    assert lib.sg_parts_query(None, buf) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_parts_labels(None, p, p, None) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_parts_select(None, p, None, ctypes.byref(n), ctypes.byref(n)) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_parts_emit(None, p, p, p, p, p, None) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_parts_destroy(None) == 0


def test_empty_plan_without_gpu():
    """F = 0 needs no device: K = 0, and the checks that need a plan can be exercised on it."""
    lib = capi.load()
    plan = ctypes.c_void_p()
    n_v, n_f = ctypes.c_int64(5), ctypes.c_int64(5)
    info = (ctypes.c_int64 * 8)()
    assert lib.sg_parts_create(None, 0, 0, 0, None, ctypes.byref(plan)) == 0 and plan.value
    try:
        assert lib.sg_parts_query(plan, None) == -1 and b"null pointer" in lib.sg_last_error()
        assert lib.sg_parts_query(plan, info) == 0
        assert list(info) == [0, 0, 0, 0, -1, 0, -1, -1]
        assert lib.sg_parts_select(plan, None, None, None, ctypes.byref(n_f)) == -1 and b"null pointer" in lib.sg_last_error()
        assert lib.sg_parts_emit(plan, None, None, None, None, None, None) == -1 and b"sg_parts_select first" in lib.sg_last_error()
    finally:
        assert lib.sg_parts_destroy(plan) == 0


def test_python_functions_have_no_cpu_path():
    from semigcn_amd import components
    vs = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    faces = torch.tensor([[0, 1, 3], [1, 2, 3], [2, 0, 3]])
    with pytest.raises(capi.SemigcnLibraryError):
        components.keep_components((vs, faces))
    with pytest.raises(capi.SemigcnLibraryError):
        components.face_components(faces, 4)
    with pytest.raises(capi.SemigcnLibraryError):
        components.PartsPlan(faces, 4)
    # the ValueErrors come before the device check
    with pytest.raises(ValueError, match="connectivity"):
        components.face_components(faces, 4, connectivity="corner")
    with pytest.raises(ValueError, match="connectivity"):
        components.keep_components((vs, faces), connectivity="corner")
    with pytest.raises(ValueError, match="connectivity"):
        components.PartsPlan(faces, 4, "corner")
    with pytest.raises(ValueError, match="keep"):
        components.keep_components((vs, faces), keep="biggest")
    with pytest.raises(ValueError, match="keep"):
        components.keep_components((vs, faces), keep=3)
    with pytest.raises(ValueError, match="keep"):
        components.keep_components((vs, faces), keep=torch.tensor([1.0]))
    with pytest.raises(ValueError, match="min_faces"):
        components.keep_components((vs, faces), min_faces=-1)


# ---- the oracle's own pins ---------------------------------------------------------------------------------------------
def test_oracle_two_tetrahedra_sharing_a_vertex():
    V, faces = CO.two_tetrahedra_sharing_a_vertex()
    labels, count, largest, n_deg = CO.face_components(faces, V, "edge")
    assert labels.tolist() == [0] * 4 + [1] * 4 and count.tolist() == [4, 4] and largest == 0 and n_deg == 0
    labels, count, largest, n_deg = CO.face_components(faces, V, "vertex")
    assert labels.tolist() == [0] * 8 and count.tolist() == [8] and largest == 0


def test_oracle_three_faces_on_one_edge():
    V, faces = CO.fan(3)
    for c in ("edge", "vertex"):
        labels, count, largest, _ = CO.face_components(faces, V, c)
        assert labels.tolist() == [0, 0, 0] and count.tolist() == [3]


def test_oracle_same_directed_half_edge():
    """(0, 1, 2) and (0, 1, 3) both hold the directed half-edge (0, 1): inconsistently oriented, still one component."""
    faces = np.array([[0, 1, 2], [0, 1, 3]])
    labels, count, _, _ = CO.face_components(faces, 4, "edge")
    assert labels.tolist() == [0, 0] and count.tolist() == [2]


def test_oracle_degenerate_face():
    """Face 1 repeats vertex 2; it would otherwise join faces 0 and 2 (it shares an edge with each)."""
    faces = np.array([[0, 1, 2], [2, 2, 3], [3, 4, 5], [1, 2, 2]])
    vs = np.arange(18, dtype=np.float32).reshape(6, 3)
    for c in ("edge", "vertex"):
        labels, count, largest, n_deg = CO.face_components(faces, 6, c)
        assert labels.tolist() == [0, -1, 1, -1] and count.tolist() == [1, 1] and largest == 0 and n_deg == 2
        _, new_faces, vertex_ids, face_ids, kept = CO.keep_components(vs, faces, "all", connectivity=c)
        assert face_ids.tolist() == [0, 2] and kept.tolist() == [True, True] and vertex_ids.tolist() == [0, 1, 2, 3, 4, 5]
        assert new_faces.tolist() == [[0, 1, 2], [3, 4, 5]]
    labels, count, largest, n_deg = CO.face_components(np.array([[1, 1, 0], [2, 0, 2]]), 3)
    assert labels.tolist() == [-1, -1] and count.shape == (0,) and largest == -1 and n_deg == 2


def test_oracle_equal_sizes_the_lower_smallest_face_wins():
    """Three components of two faces each, their faces interleaved: the one that holds face 0 is the largest."""
    a, b, c = [[0, 1, 2], [2, 1, 3]], [[4, 5, 6], [6, 5, 7]], [[8, 9, 10], [10, 9, 11]]
    faces = np.array([b[0], c[0], a[0], c[1], a[1], b[1]])
    labels, count, largest, _ = CO.face_components(faces, 12)
    assert labels.tolist() == [0, 1, 2, 1, 2, 0] and count.tolist() == [2, 2, 2] and largest == 0
    vs = np.arange(36, dtype=np.float32).reshape(12, 3)
    new_vs, new_faces, vertex_ids, face_ids, kept = CO.keep_components(vs, faces)
    assert kept.tolist() == [True, False, False] and face_ids.tolist() == [0, 5] and vertex_ids.tolist() == [4, 5, 6, 7]
    assert new_faces.tolist() == [[0, 1, 2], [2, 1, 3]] and np.array_equal(new_vs, vs[4:8])
    # one more face on the component numbered 1: now it is the largest
    more = np.concatenate([faces, [[11, 9, 8]]])
    assert CO.face_components(more, 12)[2] == 1
    # min_faces drops from what keep holds; a keep array is taken as it is
    assert CO.keep_components(vs, more, "all", min_faces=3)[4].tolist() == [False, True, False]
    assert CO.keep_components(vs, more, "largest", min_faces=4)[4].tolist() == [False, False, False]
    assert CO.keep_components(vs, more, np.array([0, 1, 1], np.uint8))[3].tolist() == [1, 2, 3, 4, 6]


def test_oracle_unreferenced_vertices_and_ascending_ids():
    """Vertices 0, 1, 3 and 7 belong to no face; ids are new to old, ascending, and the faces are renumbered through them."""
    faces = np.array([[6, 5, 4], [5, 4, 2], [9, 8, 10]])
    vs = np.random.default_rng(0).standard_normal((11, 3)).astype(np.float32)
    new_vs, new_faces, vertex_ids, face_ids, kept = CO.keep_components(vs, faces, "all")
    assert vertex_ids.tolist() == [2, 4, 5, 6, 8, 9, 10] and face_ids.tolist() == [0, 1, 2]
    assert np.array_equal(vertex_ids[new_faces], faces)
    assert np.array_equal(new_vs.view(np.uint32), vs[vertex_ids].view(np.uint32))
    new_vs, new_faces, vertex_ids, face_ids, kept = CO.keep_components(vs, faces)              # edge: {0, 1}, {2}
    assert kept.tolist() == [True, False] and vertex_ids.tolist() == [2, 4, 5, 6] and face_ids.tolist() == [0, 1]
    assert new_faces.tolist() == [[3, 2, 1], [2, 1, 0]]
    assert (np.diff(vertex_ids) > 0).all() and (np.diff(face_ids) > 0).all()


def test_oracle_shared_meshes():
    V, f = CO.strip(5)
    assert V == 12 and f.shape == (10, 3) and CO.face_components(f, V)[1].tolist() == [10]
    vs, f = CO.octahedra(3)
    labels, count, largest, _ = CO.face_components(f, vs.shape[0])
    assert labels.tolist() == [0, 1, 2] * 8 and count.tolist() == [8, 8, 8] and largest == 0
    V, f = CO.fan(64)
    assert CO.face_components(f, V)[1].tolist() == [64]
