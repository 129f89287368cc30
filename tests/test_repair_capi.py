"""semigcn_amd.repair below the C ABI (csrc/mesh_isect.hip), without a device: the entry points exist in the header, the
ctypes table and the library; they reject bad arguments before touching a device; the Python functions have no CPU path and
raise their ValueErrors first; the numpy oracle the GPU tests compare against (tests/intersect_oracle.py) gives the
hand-computed answers, one per branch of the predicate; and the oracle's repair loop converges on the folded sphere of the
GPU test with the default grow = 1 (one round), so that the convergence asserted there is a property of the algorithm on
that input."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import holes_oracle as HO
import intersect_oracle as IO
from semigcn_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sg_surface_self_count", "sg_surface_self_pairs")


def test_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "semigcn.h")).read()
    declared = re.findall(r"^SG_API\s+[\w\s\*]+?\b(sg_\w+)\s*\(", text, flags=re.M)
    lib = ctypes.CDLL(capi.library_path())
    for name in NEW:
        assert name in declared, name
        assert name in capi._SIGNATURES, name
        assert hasattr(lib, name), name
    assert capi.load().sg_abi_version() == 1
    assert callable(capi.SurfaceHandle.self_count) and callable(capi.SurfaceHandle.self_pairs)


def test_argument_validation_without_gpu():
    lib = capi.load()
    buf = (ctypes.c_int64 * 16)()          # host memory: every call below must return before it would be touched
    p = ctypes.c_void_p(ctypes.addressof(buf))
    count, pairs = lib.sg_surface_self_count, lib.sg_surface_self_pairs

    assert count(None, p, p, 5, p, p, p, None) == -1 and b"null surface" in lib.sg_last_error()
    assert count(None, None, p, 5, p, p, p, None) == -1 and b"null pointer" in lib.sg_last_error()
    assert count(None, p, None, 5, p, p, p, None) == -1 and b"null pointer" in lib.sg_last_error()
    assert count(None, p, p, -1, p, p, p, None) == -1 and b"negative" in lib.sg_last_error()
    assert count(None, p, p, 1 << 31, p, p, p, None) == -1 and b"int32" in lib.sg_last_error()

    assert pairs(None, p, p, 5, p, 3, p, None) == -1 and b"null surface" in lib.sg_last_error()
    assert pairs(None, None, p, 5, p, 3, p, None) == -1 and b"null pointer" in lib.sg_last_error()
    assert pairs(None, p, p, 5, p, -1, p, None) == -1 and b"negative n_pairs" in lib.sg_last_error()
    assert pairs(None, p, p, 5, p, 1 << 31, p, None) == -1 and b"int32" in lib.sg_last_error()
    assert pairs(None, p, p, -1, p, 3, p, None) == -1 and b"negative" in lib.sg_last_error()
    assert pairs(None, p, p, 1 << 31, p, 3, p, None) == -1 and b"int32" in lib.sg_last_error()


def test_empty_face_list_needs_no_device():
    """F = 0 returns before any argument is looked at: there is no surface of no faces to pass."""
    lib = capi.load()
    assert lib.sg_surface_self_count(None, None, None, 0, None, None, None, None) == 0
    assert lib.sg_surface_self_pairs(None, None, None, 0, None, 0, None, None) == 0


def test_python_functions_have_no_cpu_path():
    from semigcn_amd import repair
    vs = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    faces = torch.tensor([[0, 1, 3], [1, 2, 3], [2, 0, 3]])
    for fn in (repair.self_intersections, repair.remove_self_intersections, repair.repair):
        with pytest.raises(capi.SemigcnLibraryError):
            fn((vs, faces))
        with pytest.raises(ValueError, match="faces"):       # the ValueErrors come before the device check
            fn((vs, faces.reshape(-1)))
        with pytest.raises(ValueError, match="faces"):
            fn((vs, torch.zeros((3, 4), dtype=torch.int64)))
    for fn in (repair.remove_self_intersections, repair.repair):
        with pytest.raises(ValueError, match="grow"):
            fn((vs, faces), grow=-1)
        with pytest.raises(ValueError, match="max_rounds"):
            fn((vs, faces), max_rounds=-1)


# ---- the oracle's own pins -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IO.hand_cases()))
def test_oracle_hand_cases(name):
    vs, faces, pairs, n_degenerate = IO.hand_cases()[name]
    for x in (vs, vs.astype(np.float32)):                    # exact integers, and float64 on the same values
        got = IO.self_intersections(x, faces)
        assert got.pairs.tolist() == pairs.tolist()
        assert got.n_degenerate == n_degenerate
        assert got.face_mask.tolist() == [bool((pairs == i).any()) for i in range(faces.shape[0])]
    assert len(IO.self_intersections(vs, faces).marginal) == 0


def test_oracle_hand_cases_cover_every_branch():
    assert set(IO.hand_cases()) == {
        "edge_pierces_interior", "endpoint_on_face_touches", "coplanar_one_inside", "coplanar_disjoint",
        "shared_vertex_clean", "shared_vertex_opposite_edge_pierces", "shared_edge_folded_flat", "shared_edge_fold_opened",
        "duplicate_faces", "degenerate_faces"}


def test_oracle_flat_grid_has_no_pair():
    vs, faces = IO.flat_grid(8)
    assert faces.shape == (128, 3)
    got = IO.self_intersections(vs, faces)
    assert len(got) == 0 and got.n_degenerate == 0 and not got.face_mask.any()


def test_oracle_shared_meshes():
    vs, faces = IO.two_boxes()
    F = faces.shape[0]
    assert F == 299 and F % 4 and F % 64 and F > 2 * 64 and np.abs(vs).max() <= 1 << 10
    assert len(IO.self_intersections(vs, faces)) == 66
    for big_first in (True, False):
        vs, faces = IO.crossed_grid(30, big_first)
        big = 0 if big_first else faces.shape[0] - 1
        got = IO.self_intersections(vs, faces)
        assert np.abs(vs).max() <= 1 << 10 and len(got) == 1200 and int((got.pairs == big).any(1).sum()) == 1200


def test_torus_pair_has_no_marginal_pair():
    """A condition on the input of the GPU float test (this seed): every sign the oracle takes there is safe."""
    vs, faces = IO.torus_pair(40, 38, seed=314)
    got = IO.self_intersections(vs, faces)
    assert vs.dtype == np.float32 and faces.shape[0] == 6080 and len(got) > 100 and len(got.marginal) == 0


def test_oracle_repair_converges_on_the_folded_sphere():
    vs, faces = IO.folded_sphere()
    first = IO.self_intersections(vs, faces)
    assert len(first) > 0 and len(first.marginal) == 0 and len(HO.boundary_loops(faces)) == 0
    out_vs, out_faces, rounds, removed, remaining, ids = IO.repair_oracle(vs, faces)      # the defaults: grow = 1
    assert remaining == 0 and 1 <= rounds <= 10 and len(removed) == rounds
    assert len(HO.boundary_loops(out_faces)) == 0
    kept = ids >= 0
    assert np.array_equal(out_vs[kept].view(np.uint32), vs[ids[kept]].view(np.uint32))
    assert IO.repair_oracle(vs, faces, max_rounds=0)[4] == len(first)
