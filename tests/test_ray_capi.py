"""The ray query and the renderer below and above the C ABI (csrc/mesh_ray.hip), without a device: the entry points exist in
the header, the ctypes table and the library; they reject bad arguments before touching a device; the Python functions
raise their argument errors before any device is asked for and have no CPU path."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from semigcn_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sg_surface_raycast", "sg_surface_render", "sg_shade_hits")


def test_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "semigcn.h")).read()
    declared = re.findall(r"^SG_API\s+[\w\s\*]+?\b(sg_\w+)\s*\(", text, flags=re.M)
    lib = ctypes.CDLL(capi.library_path())
    for name in NEW:
        assert name in declared, name
        assert name in capi._SIGNATURES, name
        assert hasattr(lib, name), name
    assert capi.load().sg_abi_version() == 1
    for name, value in (("SG_SHADE_CONSTANT", 0), ("SG_SHADE_FACE", 1), ("SG_SHADE_SCALAR", 2)):
        assert re.search(rf"^#define {name} {value}$", text, flags=re.M), name
    assert capi.SHADE_MODES == {"constant": 0, "face": 1, "scalar": 2}


def test_argument_validation_without_gpu():
    lib = capi.load()
    buf = (ctypes.c_int64 * 32)()          # host memory: every call below must return before it would be touched
    p = ctypes.c_void_p(ctypes.addressof(buf))
    inf, nan = math.inf, math.nan
    err = lib.sg_last_error

    # the sizes and the range come first, as n_pairs does in sg_surface_self_pairs: no surface is needed to refuse them
    cast = lib.sg_surface_raycast
    assert cast(None, p, p, 4, p, p, -1, 0.0, inf, p, p, p, p, None) == -1 and b"negative N" in err()
    assert cast(None, p, p, 4, p, p, 1 << 31, 0.0, inf, p, p, p, p, None) == -1 and b"does not fit int32" in err()
    assert cast(None, p, p, -1, p, p, 1, 0.0, inf, p, p, p, p, None) == -1 and b"negative F" in err()
    assert cast(None, p, p, 4, p, p, 1, 2.0, 1.0, p, p, p, p, None) == -1 and b"t_min = 2 > t_max = 1" in err()
    assert cast(None, p, p, 4, p, p, 1, nan, 1.0, p, p, p, p, None) == -1 and b"t_min" in err()
    assert cast(None, p, p, 4, p, p, 1, 0.0, nan, p, p, p, p, None) == -1 and b"t_min" in err()
    assert cast(None, None, p, 4, p, p, 1, 0.0, inf, p, p, p, p, None) == -1 and b"null pointer" in err()
    assert cast(None, p, None, 4, p, p, 1, 0.0, inf, p, p, p, p, None) == -1 and b"null pointer" in err()
    assert cast(None, p, p, 4, p, p, 1, 0.0, inf, p, p, p, p, None) == -1 and b"null surface" in err()
    assert cast(None, p, p, 4, p, p, 1, 1.5, 1.5, p, p, p, p, None) == -1 and b"null surface" in err()   # t_min == t_max is a range
    assert cast(None, p, p, 4, p, p, 0, 0.0, inf, p, p, p, p, None) == -1 and b"null surface" in err()   # before N == 0

    render = lib.sg_surface_render
    cam = (ctypes.c_double * 14)(*range(14))
    assert render(None, p, p, 4, cam, 0, -1, 8, 0.0, inf, p, p, p, p, None) == -1 and b"negative width or height" in err()
    assert render(None, p, p, 4, cam, 0, 8, -1, 0.0, inf, p, p, p, p, None) == -1 and b"negative width or height" in err()
    assert render(None, p, p, 4, cam, 0, 1 << 24, 1, 0.0, inf, p, p, p, p, None) == -1 and b"do not fit int32" in err()
    assert render(None, p, p, 4, cam, 0, 1, 1 << 24, 0.0, inf, p, p, p, p, None) == -1 and b"do not fit int32" in err()
    assert render(None, p, p, 4, cam, 0, 1 << 16, 1 << 15, 0.0, inf, p, p, p, p, None) == -1 and b"do not fit int32" in err()
    assert render(None, p, p, -1, cam, 0, 8, 8, 0.0, inf, p, p, p, p, None) == -1 and b"negative F" in err()
    assert render(None, p, p, 4, cam, 0, 8, 8, 3.0, -3.0, p, p, p, p, None) == -1 and b"t_min = 3 > t_max = -3" in err()
    assert render(None, None, p, 4, cam, 0, 8, 8, 0.0, inf, p, p, p, p, None) == -1 and b"null pointer" in err()
    assert render(None, p, None, 4, cam, 0, 8, 8, 0.0, inf, p, p, p, p, None) == -1 and b"null pointer" in err()
    assert render(None, p, p, 4, cam, 0, 8, 8, 0.0, inf, p, p, p, p, None) == -1 and b"null surface" in err()
    assert render(None, p, p, 4, cam, 0, 0, 8, 0.0, inf, p, p, p, p, None) == -1 and b"null surface" in err()   # before zero pixels

    shade = lib.sg_shade_hits
    ok = dict(V=4, F=2, n=4, mode=0, ambient=0.25, dirs=p, cam=None, w=0, h=0, fc=None, sc=None, rgb=p, vs=p, face=p)

    def call(**kw):
        a = dict(ok, **kw)
        return shade(a["vs"], a["V"], p, a["F"], a["face"], p, a["dirs"], a["cam"], 0, a["w"], a["h"], a["n"], a["mode"],
                     0xFFA500, a["fc"], a["sc"], 0.0, 1.0, 0xFFFFFF, a["ambient"], a["rgb"], None)
    assert call(V=-1) == -1 and b"negative size" in err()
    assert call(F=-1) == -1 and b"negative size" in err()
    assert call(n=-1) == -1 and b"negative size" in err()
    assert call(n=1 << 31) == -1 and b"int32" in err()
    assert call(mode=3) == -1 and b"unknown mode 3" in err()
    assert call(ambient=1.5) == -1 and b"ambient" in err()
    assert call(ambient=math.nan) == -1 and b"ambient" in err()
    assert call(dirs=None) == -1 and b"neither directions nor a camera" in err()
    assert call(dirs=None, cam=cam, w=3, h=2) == -1 and b"3 x 2 pixels are not the 4 rows" in err()
    assert call(dirs=None, cam=cam, w=-2, h=-2) == -1 and b"pixels are not" in err()
    assert call(vs=None) == -1 and b"null pointer" in err()
    assert call(face=None) == -1 and b"null pointer" in err()
    assert call(rgb=None) == -1 and b"null pointer" in err()
    assert call(mode=1) == -1 and b"null face_colors" in err()
    assert call(mode=2) == -1 and b"null scalars" in err()
    assert call(n=0, vs=None, face=None, rgb=None) == 0                          # nothing to do: nothing is read
    assert call(n=0, dirs=None, cam=cam, w=0, h=5, rgb=None) == 0


MESH = (torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]), torch.tensor([[0, 1, 3], [1, 2, 3], [2, 0, 3]]))


def test_python_errors_come_before_any_device():
    from semigcn_amd import render as R
    vs, faces = MESH
    cam = R.look_at((2, 2, 2), (0, 0, 0))
    assert abs(np.dot(cam.right, cam.up)) < 1e-15 and abs(np.dot(cam.right, cam.forward)) < 1e-15
    assert np.allclose(np.cross(cam.right, cam.up), -np.asarray(cam.forward)) and len(cam.params(400, 300)) == 14
    assert cam.params(400, 300)[12] == cam.params(400, 300)[13] * (400 / 300) and not cam.ortho
    assert R.look_at((0, 0, 5), (0, 0, 0), ortho_height=3.0).params(10, 10)[12:] == [1.5, 1.5]
    for kw, msg in ((dict(eye=(1, 1, 1), target=(1, 1, 1)), "no view direction"),
                    (dict(eye=(0, 5, 0), target=(0, 0, 0)), "parallel"),
                    (dict(eye=(1, 0, 0), target=(0, 0, 0), fov_deg=180), "fov_deg"),
                    (dict(eye=(1, 0, 0), target=(0, 0, 0), ortho_height=0), "ortho_height")):
        with pytest.raises(ValueError, match=msg):
            R.look_at(**kw)
    for size in ((0, 8), (8, -1)):
        with pytest.raises(ValueError, match="at least 1 x 1"):
            R.render((vs, faces), cam, *size)
        with pytest.raises(ValueError, match="at least 1 x 1"):
            R.turntable((vs, faces), 4, size)
    with pytest.raises(TypeError, match="camera must be a Camera"):
        R.render((vs, faces), None, 8, 8)
    with pytest.raises(ValueError, match=r"vs must be \[V, 3\]"):
        R.render((vs[:, :2], faces), cam, 8, 8)
    with pytest.raises(ValueError, match="faces must hold integers"):
        R.render((vs, faces.float()), cam, 8, 8)
    with pytest.raises(ValueError, match="no faces"):
        R.render((vs, faces[:0]), cam, 8, 8)
    with pytest.raises(ValueError, match="no faces"):
        R.turntable((vs, faces[:0]))
    for bad in (0, 5, -1):
        with pytest.raises(ValueError, match="ssaa must be one of"):
            R.render((vs, faces), cam, 8, 8, ssaa=bad)
    with pytest.raises(ValueError, match=r"ambient must be in \[0, 1\]"):
        R.render((vs, faces), cam, 8, 8, ambient=1.2)
    with pytest.raises(ValueError, match=r"one value per vertex \(4\), got \(3,\)"):
        R.render((vs, faces), cam, 8, 8, scalars=torch.zeros(3))
    with pytest.raises(ValueError, match=r"face_colors must be \[F, 3\] = \[3, 3\], got \(4, 3\)"):
        R.render((vs, faces), cam, 8, 8, face_colors=torch.zeros(4, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="face_colors must be uint8"):
        R.render((vs, faces), cam, 8, 8, face_colors=np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="not both"):
        R.render((vs, faces), cam, 8, 8, scalars=torch.zeros(4), face_colors=torch.zeros(3, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="three levels"):
        R.render((vs, faces), cam, 8, 8, color=(256, 0, 0))
    with pytest.raises(ValueError, match="three levels"):
        R.turntable((vs, faces), 2, (8, 8), background=(0, 0))
    with pytest.raises(ValueError, match="frames must be >= 1"):
        R.turntable((vs, faces), 0)
    assert np.array_equal(R.mask_colors(np.array([1, 0, 1])), [[85, 169, 255], [255, 0, 255], [85, 169, 255]])
    assert R.mask_colors(torch.tensor([False, True])).tolist() == [[255, 0, 255], [85, 169, 255]]


@pytest.mark.parametrize("ortho", [False, True])
def test_camera_rays_are_the_rule_s(ortho):
    """render.camera_rays (the host's copy of what the render kernel generates) against the oracle's restatement, bit for bit"""
    import ray_oracle
    from semigcn_amd import render as R
    cam = R.look_at((1.7, -0.4, 2.9), (0.1, 0.2, -0.3), fov_deg=37.0, ortho_height=2.5 if ortho else None)
    for W, H in ((1, 1), (9, 7), (65, 33)):
        o, d = R.camera_rays(cam, W, H)
        wo, wd = ray_oracle.camera_rays(cam.params(W, H), ortho, W, H)
        assert o.dtype == d.dtype == np.float32 and o.shape == d.shape == (W * H, 3)
        assert np.array_equal(o.view(np.uint32), wo.view(np.uint32)) and np.array_equal(d.view(np.uint32), wd.view(np.uint32))
    with pytest.raises(ValueError, match="at least 1 x 1"):
        R.camera_rays(cam, 0, 4)


def test_python_functions_have_no_cpu_path():
    from semigcn_amd import evaluate, render as R
    vs, faces = MESH
    cam = R.look_at((2, 2, 2), (0, 0, 0))
    with pytest.raises(capi.SemigcnLibraryError):
        R.render((vs, faces), cam, 8, 8)
    with pytest.raises(capi.SemigcnLibraryError):
        R.render((vs, faces), cam, 8, 8, scalars=torch.zeros(4))
    with pytest.raises(capi.SemigcnLibraryError):
        R.turntable((vs, faces), 2, (8, 8))
    with pytest.raises(capi.SemigcnLibraryError):
        R.error_colors(vs, (vs, faces))
    with pytest.raises(capi.SemigcnLibraryError):
        evaluate.Surface(vs, faces)
    z = torch.zeros(2, 3)
    with pytest.raises(capi.SemigcnLibraryError, match="is on cpu"):
        capi.SurfaceHandle.ray_cast(object.__new__(capi.SurfaceHandle), vs, faces, z, z)
    with pytest.raises(capi.SemigcnLibraryError, match="is on cpu"):
        capi.SurfaceHandle.render(object.__new__(capi.SurfaceHandle), vs, faces, [0.0] * 14, False, 8, 8)
    with pytest.raises(capi.SemigcnLibraryError, match="is on cpu"):
        capi.shade_hits(vs, faces, torch.zeros(2, dtype=torch.int32), None, dirs=z)
    for name in ("Camera", "look_at", "camera_rays", "render", "turntable", "error_colors", "mask_colors", "write_png", "write_apng"):
        assert name in R.__all__ and hasattr(R, name)
    assert ("write_gif" in R.__all__) == hasattr(R, "write_gif")
    assert "ray_cast" in dir(evaluate.Surface) and evaluate.Hits._fields == ("t", "face", "bary")
