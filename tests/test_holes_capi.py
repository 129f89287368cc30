"""semigcn_amd.holes below the C ABI (csrc/mesh_fill.hip), without a device: the entry points exist in the header, the
ctypes table and the library; they reject bad arguments before touching a device; the Python functions have no CPU path;
and the numpy oracle the GPU tests compare against (tests/holes_oracle.py) gives the hand-computed answers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import holes_oracle as HO
from semigcn_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sg_fill_create", "sg_fill_destroy", "sg_fill_query", "sg_fill_loops", "sg_fill_plan", "sg_fill_emit")


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
    plan = ctypes.c_void_p()
    n = ctypes.c_int64()

    create = lib.sg_fill_create
    assert create(p, 2, 4, None, None) == -1 and b"null out" in lib.sg_last_error()
    assert create(p, -1, 4, None, ctypes.byref(plan)) == -1 and b"negative" in lib.sg_last_error() and not plan.value
    assert create(p, 2, -1, None, ctypes.byref(plan)) == -1 and b"negative" in lib.sg_last_error() and not plan.value
    assert create(None, 2, 4, None, ctypes.byref(plan)) == -1 and b"null pointer" in lib.sg_last_error() and not plan.value

    assert lib.sg_fill_query(None, buf) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_fill_loops(None, p, p, None) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_fill_plan(None, -1, None, ctypes.byref(n), ctypes.byref(n)) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_fill_emit(None, p, p, p, p, None) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_fill_destroy(None) == 0


def test_python_functions_have_no_cpu_path():
    from semigcn_amd import holes
    vs = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    faces = torch.tensor([[0, 1, 3], [1, 2, 3], [2, 0, 3]])
    with pytest.raises(capi.SemigcnLibraryError):
        holes.fill_holes((vs, faces))
    with pytest.raises(capi.SemigcnLibraryError):
        holes.boundary_loops(faces, 4)
    with pytest.raises(capi.SemigcnLibraryError):
        holes.FillPlan(faces, 4)
    with pytest.raises(ValueError, match="fair_steps"):
        holes.fill_holes((vs, faces), fair_steps=-1)
    with pytest.raises(ValueError, match="max_hole_edges"):
        holes.fill_holes((vs, faces), max_hole_edges=-2)


# ---- the oracle's own pins ---------------------------------------------------------------------------------------------
TET_VS = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
TET = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])       # outward


def test_oracle_tetrahedron_minus_a_face():
    """Without (1, 2, 3) the half-edges (2, 1), (3, 2), (1, 3) lose their opposites; the loop runs against them from its
    smallest vertex: 1, 2, 3 -- exactly the missing face."""
    open_faces = TET[[0, 1, 3]]
    loops = HO.boundary_loops(open_faces)
    assert loops == [[1, 2, 3]]
    vs, faces, inserted, filled, _ = HO.fill_holes(TET_VS, open_faces)
    assert vs.shape == (4, 3) and not inserted.any() and filled.tolist() == [True]
    assert np.array_equal(faces[:3], open_faces) and faces[3].tolist() == [1, 2, 3]
    assert HO.half_edge_stats(faces) == (1, 0) and HO.euler_characteristic(faces) == 2
    assert HO.boundary_loops(TET) == []


def test_oracle_square_hole():
    """Octahedron minus the four faces at vertex 4 (the top): a loop of four, one centre vertex at their mean, four faces."""
    vs = np.array([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    faces = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    bottom = faces[4:]
    loops = HO.boundary_loops(bottom)
    assert loops == [[0, 2, 1, 3]]                   # the bottom has (2, 0): the loop lists 0 then 2
    new_vs, new_faces, inserted, filled, _ = HO.fill_holes(vs, bottom)
    assert new_vs.shape == (7, 3) and inserted.tolist() == [False] * 6 + [True]
    assert np.array_equal(new_vs[6], vs[[0, 2, 1, 3]].mean(0)) and np.array_equal(new_vs[6], [0.0, 0, 0])
    assert new_faces[4:].tolist() == [[0, 2, 6], [2, 1, 6], [1, 3, 6], [3, 0, 6]]
    assert HO.half_edge_stats(new_faces) == (1, 0) and HO.euler_characteristic(new_faces) == 2


def test_oracle_ring_count_table():
    """R(n) = max(1, (113 n + 355) // 710) = n / (2 pi) rounded, and the ring sizes, for n = 3 ... 12."""
    assert [HO.ring_count(n) for n in range(3, 13)] == [1, 1, 1, 1, 1, 1, 1, 2, 2, 2]
    assert [HO.ring_count(n) for n in range(3, 13)] == [max(1, int(np.floor(n / (2 * np.pi) + 0.5))) for n in range(3, 13)]
    assert HO.ring_sizes(4) == [4, 1] and HO.ring_sizes(9) == [9, 1]
    assert HO.ring_sizes(10) == [10, 5, 1] and HO.ring_sizes(11) == [11, 6, 1] and HO.ring_sizes(12) == [12, 6, 1]
    assert HO.ring_sizes(16) == [16, 11, 5, 1]       # R = 3: 16 * 2 / 3 = 10.67 -> 11, 16 / 3 = 5.33 -> 5
    assert HO.ring_sizes(13)[1:-1] == [7]
    assert min(min(HO.ring_sizes(n)[:-1]) for n in range(4, 400)) >= 3


def test_oracle_unorderable():
    fans = np.array([[0, 1, 2], [0, 3, 4]])           # two triangles that share only vertex 0
    with pytest.raises(HO.Unorderable) as e:
        HO.boundary_loops(fans)
    assert (e.value.n_repeated, e.value.n_bowtie, e.value.vertex) == (0, 1, 0)
    with pytest.raises(HO.Unorderable) as e:
        HO.boundary_loops(np.concatenate([TET, TET[2:3]]))
    assert (e.value.n_repeated, e.value.n_bowtie, e.value.vertex) == (3, 0, 1)


@pytest.mark.parametrize("n", [4, 7, 10, 16, 64, 100, 333])
def test_oracle_regular_polygon_patch(n):
    """The unfaired patch of a regular planar n-gon of edge length h: a closed disc whose boundary is the polygon, every
    directed half-edge once, no degenerate face, every edge in [0.5 h, 2.5 h] (measured for this construction:
    0.707 h ... 2.236 h), every face counter-clockwise like the polygon."""
    h = 0.37
    b = HO.regular_polygon(n, h)
    new, faces = HO.fill_loop(b)
    P = np.concatenate([b, new])
    assert len(new) == sum(HO.ring_sizes(n)[1:]) and faces.max() == len(P) - 1
    assert all(len(set(f)) == 3 for f in faces.tolist())
    count = __import__("collections").Counter(HO.half_edges(faces))
    assert max(count.values()) == 1
    border = sorted(e for e in count if (e[1], e[0]) not in count)
    assert border == sorted((i, (i + 1) % n) for i in range(n))
    assert HO.euler_characteristic(faces) == 1
    lengths = HO.edge_lengths(P, faces) / h
    print(f"n={n}: edges {lengths.min():.3f} h ... {lengths.max():.3f} h")
    assert lengths.min() >= 0.5 and lengths.max() <= 2.5
    nz = np.cross(P[faces[:, 1]] - P[faces[:, 0]], P[faces[:, 2]] - P[faces[:, 0]])[:, 2]
    assert (nz > 0).all()
