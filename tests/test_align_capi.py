"""The registration below and above the C ABI (csrc/mesh_align.hip), without a device: the entry points exist in the header,
the ctypes table and the library; they reject bad arguments before touching a device; the Python functions raise their
argument errors before any device is asked for and have no CPU path."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from semigcn_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sg_align_transform", "sg_align_accumulate")


def test_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "semigcn.h")).read()
    declared = re.findall(r"^SG_API\s+[\w\s\*]+?\b(sg_\w+)\s*\(", text, flags=re.M)
    lib = ctypes.CDLL(capi.library_path())
    for name in NEW:
        assert name in declared, name
        assert name in capi._SIGNATURES, name
        assert hasattr(lib, name), name
    assert capi.load().sg_abi_version() == 1
    assert capi.ALIGN_SUMS == 40 and "#define SG_REDUCE_BLOCKS 1024" in text and capi.REDUCE_BLOCKS == 1024


def test_argument_validation_without_gpu():
    lib = capi.load()
    buf = (ctypes.c_int64 * 32)()          # host memory: every call below must return before it would be touched
    p = ctypes.c_void_p(ctypes.addressof(buf))
    pose = (ctypes.c_double * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    inf = float("inf")

    tr = lib.sg_align_transform
    assert tr(p, -1, pose, p, None) == -1 and b"[0, 2^31)" in lib.sg_last_error()
    assert tr(p, 1 << 31, pose, p, None) == -1 and b"[0, 2^31)" in lib.sg_last_error()
    assert tr(p, 4, None, p, None) == -1 and b"null pose" in lib.sg_last_error()
    assert tr(None, 4, pose, p, None) == -1 and b"null pointer" in lib.sg_last_error()
    assert tr(p, 4, pose, None, None) == -1 and b"null pointer" in lib.sg_last_error()
    assert tr(None, 0, pose, None, None) == 0                      # nothing to do, nothing launched

    acc = lib.sg_align_accumulate
    ok = [p, 4, p, 4, p, 2, pose, p, p, p, inf, 0, p, p, None]

    def call(**kw):
        names = ("vs", "V", "faces", "F", "pts", "N", "pose", "closest", "face", "dist", "max_dist", "with_scale", "partial",
                 "out", "stream")
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return acc(*a)

    assert call(N=-1) == -1 and b"[0, 2^31)" in lib.sg_last_error()
    assert call(N=1 << 31) == -1 and b"[0, 2^31)" in lib.sg_last_error()
    assert call(V=-1) == -1 and b"negative size" in lib.sg_last_error()
    assert call(F=-1) == -1 and b"negative size" in lib.sg_last_error()
    assert call(pose=None) == -1 and b"null pose" in lib.sg_last_error()
    assert call(max_dist=float("nan")) == -1 and b"NaN" in lib.sg_last_error()
    for name in ("vs", "faces", "pts", "closest", "face", "dist", "partial", "out"):
        assert call(**{name: None}) == -1 and b"null pointer" in lib.sg_last_error(), name
    assert call(N=0, vs=None, out=None) == 0                        # nothing to do, nothing launched or written


def test_python_errors_come_before_any_device():
    from semigcn_amd import align
    vs = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    faces = torch.tensor([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    m = (vs, faces)
    with pytest.raises(ValueError, match="points must be one of"):
        align.align(m, m, points="faces")
    for bad in (0, -5):
        with pytest.raises(ValueError, match="n must be > 0"):
            align.align(m, m, n=bad)
    with pytest.raises(ValueError, match="max_iter must be >= 0"):
        align.align(m, m, max_iter=-1)
    for bad in (0.0, -1e-6, float("nan")):
        with pytest.raises(ValueError, match="tol must be > 0"):
            align.align(m, m, tol=bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_dist must be >= 0"):
            align.align(m, m, max_dist=bad)
    with pytest.raises(ValueError, match=r"init must be a 4 x 4 matrix, got shape \(3, 3\)"):
        align.align(m, m, init=np.eye(3))
    with pytest.raises(ValueError, match=r"init must be a 4 x 4 matrix"):
        align.align(m, m, init=np.zeros(16))
    with pytest.raises(ValueError, match="init must be None, a 4 x 4 matrix or 'centroid'"):
        align.align(m, m, init="pca")
    with pytest.raises(ValueError, match=r"vs must be \[V, 3\]"):
        align.align((vs[:, :2], faces), m)
    with pytest.raises(ValueError, match="faces must hold integers"):
        align.align(m, (vs, faces.float()))
    with pytest.raises(ValueError, match=r"matrix must be a 4 x 4 matrix"):
        align.apply(np.eye(3), vs)
    with pytest.raises(ValueError, match=r"vs must be \[V, 3\], got \(4, 2\)"):
        align.apply(np.eye(4), vs[:, :2])
    with pytest.raises(ValueError, match=r"matrix must be a 4 x 4 matrix"):
        align.inverse(np.eye(3))
    with pytest.raises(ValueError, match="pose must be a 4 x 4 matrix or 12 values"):
        capi.align_transform(vs, np.eye(3))
    with pytest.raises(ValueError, match="max_dist is NaN"):
        capi.align_accumulate(vs, faces, vs, np.eye(4), vs, faces[:, 0].int(), vs[:, 0], max_dist=float("nan"))


def test_python_functions_have_no_cpu_path():
    from semigcn_amd import align
    vs = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    faces = torch.tensor([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    with pytest.raises(capi.SemigcnLibraryError):
        align.align((vs, faces), (vs, faces))
    with pytest.raises(capi.SemigcnLibraryError):
        align.align((vs, faces), (vs, faces), points="vertices", max_iter=0)
    with pytest.raises(capi.SemigcnLibraryError):
        align.apply(np.eye(4), vs)
    with pytest.raises(capi.SemigcnLibraryError):
        capi.align_transform(vs, np.eye(4))
    with pytest.raises(capi.SemigcnLibraryError):
        capi.align_accumulate(vs, faces, vs, np.eye(4), vs, faces[:, 0].int(), vs[:, 0])
    for name in ("align", "apply", "inverse", "Alignment"):
        assert name in align.__all__


def test_command_lines_know_their_options():
    from semigcn_amd import align, evaluate
    for argv in (["--torus", "8", "8", "--box", "2"], ["a.obj"], ["a.obj", "b.obj", "--perturb", "1"],
                 ["--torus", "8", "8", "--samples", "10", "--vertices"], ["a.obj", "b.obj", "--init", "pca"]):
        with pytest.raises(SystemExit):
            align.main(argv)
    with pytest.raises(SystemExit):
        evaluate.main(["--gt", "a.obj", "--out", "b.obj", "--align", "affine"])
