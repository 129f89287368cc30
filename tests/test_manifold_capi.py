"""semigcn_amd.manifold below the C ABI (csrc/mesh_manifold.hip), without a device: the entry points exist in the header, the
ctypes table and the library; they reject bad arguments before touching a device; the empty plan works; and the Python
functions have no CPU path and raise their ValueErrors first."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from semigcn_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sg_manifold_create", "sg_manifold_destroy", "sg_manifold_query", "sg_manifold_export")
WELD, DEDUP, CUT, ORIENT, OUTWARD, DROP = 1, 2, 4, 8, 16, 32
ALL = WELD | DEDUP | CUT | ORIENT | OUTWARD | DROP


def test_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "semigcn.h")).read()
    declared = re.findall(r"^SG_API\s+[\w\s\*]+?\b(sg_\w+)\s*\(", text, flags=re.M)
    lib = ctypes.CDLL(capi.library_path())
    for name in NEW:
        assert name in declared, name
        assert name in capi._SIGNATURES, name
        assert hasattr(lib, name), name
    assert "typedef struct sg_manifold sg_manifold;" in text
    for name, bit in capi.ManifoldPlan.STEPS.items():
        assert re.search(rf"^#define SG_MANIFOLD_{name.upper()} {bit}$", text, flags=re.M), name
    assert capi.load().sg_abi_version() == 1
    assert callable(capi.ManifoldPlan.close) and callable(capi.ManifoldPlan.__del__)
    assert callable(capi.ManifoldPlan.__enter__) and callable(capi.ManifoldPlan.__exit__)


def test_the_union_find_lives_in_one_header():
    """mesh_parts.hip and mesh_manifold.hip include the one copy; the Makefile knows both depend on it."""
    csrc = os.path.join(ROOT, "semigcn_amd", "csrc")
    header = open(os.path.join(csrc, "mesh_union.h")).read()
    for name in ("load_parent", "find_root", "unite", "iota32", "flatten"):
        assert re.search(rf"\b{name}\(", header), name
        for source in ("mesh_parts.hip", "mesh_manifold.hip"):
            text = open(os.path.join(csrc, source)).read()
            assert '#include "mesh_union.h"' in text
            assert not re.search(rf"^__(?:device|global)__ [\w\s]*\b{name}\(", text, flags=re.M), (source, name)
    assert "Why the union terminates" in header and "__HIP_MEMORY_SCOPE_AGENT" in header
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"mesh_parts\.o \$\(BUILD\)/mesh_manifold\.o: mesh_union\.h", make)
    assert re.search(r"mesh_manifold\.o: CXXFLAGS \+= -ffp-contract=off", make)


def test_argument_validation_without_gpu():
    lib = capi.load()
    buf = (ctypes.c_int64 * 16)()          # host memory: every call below must return before it would be touched
    p = ctypes.c_void_p(ctypes.addressof(buf))
    plan = ctypes.c_void_p()
    create = lib.sg_manifold_create

    def fails(word, *args):
        return create(*args) == -1 and word in lib.sg_last_error() and not plan.value

    assert create(p, 4, p, 2, ALL, None, None) == -1 and b"null out" in lib.sg_last_error()
    assert fails(b"negative", p, 4, p, -1, ALL, None, ctypes.byref(plan))
    assert fails(b"negative", p, -1, p, 2, ALL, None, ctypes.byref(plan))
    for bad in (-1, 64, 1 << 20):
        assert fails(b"flags", p, 4, p, 2, bad, None, ctypes.byref(plan))
    for bad in (WELD, DEDUP, CUT, WELD | ORIENT):
        assert fails(b"SG_MANIFOLD_DROP", p, 4, p, 2, bad, None, ctypes.byref(plan))
    assert fails(b"SG_MANIFOLD_ORIENT", p, 4, p, 2, OUTWARD, None, ctypes.byref(plan))
    assert fails(b"null pointer", p, 4, None, 2, ALL, None, ctypes.byref(plan))
    assert fails(b"null pointer", None, 4, p, 2, ALL, None, ctypes.byref(plan))
    assert fails(b"null pointer", None, 4, p, 2, ORIENT | OUTWARD, None, ctypes.byref(plan))
    # sizes the 32-bit sorts and parents cannot hold
    assert fails(b"int32", p, 4, p, (1 << 31) // 3 + 1, ALL, None, ctypes.byref(plan))
    assert fails(b"int32", p, 4, p, (1 << 31) // 3 + 1, ORIENT, None, ctypes.byref(plan))
    assert fails(b"int32", p, 1 << 31, p, 2, ALL, None, ctypes.byref(plan))

    assert lib.sg_manifold_query(None, buf) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_manifold_export(None, p, p, p, p, p, p, p, p, None) == -1 and b"null plan" in lib.sg_last_error()
    assert lib.sg_manifold_destroy(None) == 0


@pytest.mark.parametrize("flags,v_out", [(ALL, 0), (CUT | DROP, 0), (ORIENT | OUTWARD, 5), (0, 5)])
def test_empty_plan_without_gpu(flags, v_out):
    """F = 0 needs no device: nothing comes out, and without SG_MANIFOLD_DROP the vertices stay."""
    lib = capi.load()
    plan = ctypes.c_void_p()
    info = (ctypes.c_int64 * 16)()
    assert lib.sg_manifold_create(None, 5, None, 0, flags, None, ctypes.byref(plan)) == 0 and plan.value
    try:
        assert lib.sg_manifold_query(plan, None) == -1 and b"null pointer" in lib.sg_last_error()
        assert lib.sg_manifold_query(plan, info) == 0
        assert list(info) == [5, 0, v_out, 0, flags] + [0] * 11
        assert lib.sg_manifold_export(plan, None, None, None, None, None, None, None, None, None) == 0
    finally:
        assert lib.sg_manifold_destroy(plan) == 0


def test_python_functions_have_no_cpu_path():
    from semigcn_amd import manifold, repair
    vs = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    faces = torch.tensor([[0, 1, 3], [1, 2, 3], [2, 0, 3]])
    calls = (manifold.weld_vertices, manifold.split_nonmanifold, manifold.orient_faces, manifold.make_manifold)
    for fn in calls:
        with pytest.raises(capi.SemigcnLibraryError):
            fn((vs, faces))
        with pytest.raises(capi.SemigcnLibraryError):
            fn((vs, faces[:0]))
    with pytest.raises(capi.SemigcnLibraryError):
        manifold.ManifoldPlan(vs, faces)
    with pytest.raises(capi.SemigcnLibraryError):
        repair.repair((vs, faces), make_manifold=True)
    # the ValueErrors come before the device check
    for fn in calls:
        with pytest.raises(ValueError, match=r"vs must be \[V, 3\]"):
            fn((vs[:, :2], faces))
        with pytest.raises(ValueError, match=r"faces must be \[F, 3\]"):
            fn((vs, faces.reshape(-1)))
        with pytest.raises(ValueError, match="faces must hold integers"):
            fn((vs, faces.float()))
        with pytest.raises(ValueError, match="vs must hold floats"):
            fn((np.zeros((4, 3), np.int32), faces))
    with pytest.raises(ValueError, match="steps"):
        manifold.ManifoldPlan(vs, faces, ("weld",))
    with pytest.raises(ValueError, match="steps"):
        manifold.ManifoldPlan(vs, faces, ("outward", "drop"))
    with pytest.raises(ValueError, match="steps"):
        manifold.ManifoldPlan(vs, faces, ("orient", "sew"))


def test_mangled_torus_is_deterministic_and_holds_what_it_names():
    """The synthetic input of the command line: sizes, the reversed share, the pinches (no device)."""
    import holes_oracle as HO
    import manifold_oracle as MO
    from semigcn_amd import manifold
    vs, f = manifold.mangled_torus(32, 16)
    assert vs.shape == (512, 3) and vs.dtype == np.float32 and f.shape == (1024, 3) and HO.half_edge_stats(f) == (1, 0)
    vs2, f2 = manifold.mangled_torus(32, 16, soup=True, flip_permille=500, pinch=4)
    again = manifold.mangled_torus(32, 16, soup=True, flip_permille=500, pinch=4)
    assert np.array_equal(vs2.view(np.uint32), again[0].view(np.uint32)) and np.array_equal(f2, again[1])
    assert vs2.shape == (3072, 3) and np.array_equal(f2, np.arange(3072).reshape(-1, 3))
    r = MO.make_manifold(vs2, f2)
    assert r.vs.shape[0] == 512 and r.n_split_vertices == 4 and 400 < r.n_flipped < 624 and (r.n_components, r.n_closed) == (1, 1)
    assert MO.volume_is_decided(r) and HO.half_edge_stats(r.faces) == (1, 0)
    with pytest.raises(ValueError, match="pinch"):
        manifold.mangled_torus(32, 16, pinch=5)
