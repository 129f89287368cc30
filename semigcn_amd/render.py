"""Look at a mesh on the device: the first hit of a ray on a surface, and a small renderer on it.

The reference shows its results through ``util/render.py`` (a pyvista turntable GIF), a viser viewer and the coloured mask
mesh of ``util/datamaker.py:161-171``.  Here ``evaluate.Surface.ray_cast`` is the query underneath (visibility, projection
along a normal and rendering all rest on it), and ``render`` / ``turntable`` give flat-shaded, scalar-coloured (an error heat
map) or face-coloured (a mask) images with no dependency beyond the standard library.  The walk is ``csrc/mesh_ray.hip``;
``tests/ray_oracle.py`` restates the rule below in numpy, and the device equals it bit for bit.

The rule
========

**Inputs and conventions.**  Inputs are float32 and all arithmetic is float64 on the widened values: plain multiplies and adds
in the written order, no fused multiply-add.  ``det3(u,v,w) = u.x*(v.y*w.z - v.z*w.y) + u.y*(v.z*w.x - v.x*w.z) +
u.z*(v.x*w.y - v.y*w.x)`` (the order of operations of the self-intersection predicate's ``det3``).  A ray is an origin ``o``,
a direction ``d`` (any length) and a closed range ``[t_min, t_max]``, by default ``[0, +inf]``.  The predicate reads the
original ``vs`` / ``faces`` rows, never the surface's rounded copies.

**Face f = (A, B, C) is hit at t iff all of the following hold.**

1. The face is usable: its three ids are distinct, and ``n = e1 x e2`` is not exactly zero, where ``e1 = B - A``,
   ``e2 = C - A`` and ``n = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x)``.
2. With ``a = A - o``, ``b = B - o``, ``c = C - o``: ``U = det3(d,b,c)``, ``V = det3(d,c,a)``, ``W = det3(d,a,b)``,
   ``Sb = (U + V) + W``; ``Sb != 0``, and either ``U, V, W >= 0`` or ``U, V, W <= 0`` (closed: touching counts).
3. ``den = (d.x*n.x + d.y*n.y) + d.z*n.z != 0``; ``num = (a.x*n.x + a.y*n.y) + a.z*n.z``; ``t = num / den``, one IEEE float64
   division.
4. The own-box clause.  ``lo`` / ``hi`` are the exact min / max of the three float32 vertices.  For each axis ``k`` with
   ``d_k == 0``: require ``lo_k <= o_k <= hi_k``.  Otherwise ``inv = 1.0 / d_k``, ``t1 = (lo_k - o_k)*inv``,
   ``t2 = (hi_k - o_k)*inv``; ``tn = max_k min(t1, t2)`` starting from ``-inf``, ``tf = min_k max(t1, t2)`` starting from
   ``+inf``.  Then widen: ``tn *= (tn > 0 ? 1 - 2^-30 : 1 + 2^-30)`` and ``tf *= (tf > 0 ? 1 + 2^-30 : 1 - 2^-30)``.  Require
   ``tn <= t <= tf``.
5. ``t_min <= t <= t_max``.

**Result per ray.**  The hit with the smallest float64 ``t``, and the lowest face id on an exact tie.  The outputs are ``t``
rounded to float32, ``face`` as int32 and ``bary = (float32(V/Sb), float32(W/Sb))``: the weights of B and C.  A miss, a
non-finite ``o`` or ``d``, and ``d == 0`` give ``t = +inf``, ``face = 0x7fffffff`` and a NaN ``bary`` row -- the "no face"
convention of ``Surface.query``.

**Why clause 4 is there.**  It is what makes a tree walk equal brute force exactly.  Every step of the slab interval is a
monotone function of ``lo`` / ``hi`` under rounding, so the interval of a node's box contains the interval of every face box
inside it.  A walk may therefore drop a node iff ``tn > tf``, ``tf < t_min`` or ``tn > min(t_max, best t)`` (closed, so ties
survive) and needs no margin of its own; leaf and node boxes of the surface are exact min / max of the vertices, so the
premise holds.  With integer ``o``, ``d`` and vertices of magnitude <= 2^10 every determinant, ``num`` and ``den`` is exact
(below 2^37) and the only rounding is the division: a predicate in Python ``Fraction``s is then the truth, and the rule
equals it.

**Known and accepted.**  A face seen within about 2^-22 rad of edge-on can lose its hit to clause 4, because its ``t`` is
garbage (``num`` and ``den`` are both rounding noise); the neighbour across the edge still takes the ray.  There is no
watertightness guarantee at silhouettes beyond the rule.

Camera rays
===========

A ``Camera`` gives, for an image of ``W x H`` pixels, 14 float64 values built on the host: the eye ``e``, the orthonormal
``r`` (right), ``u`` (up), ``w`` (forward), and ``tx``, ``ty`` -- the tangents of the half view angles, or the half extents
of an orthographic view.  For pixel ``(x, y)``, ``y`` downwards: ``sx = ((2*(x + 0.5))/W - 1)*tx``,
``sy = (1 - (2*(y + 0.5))/H)*ty``; perspective: ``o = float32(e)``, ``d = float32((w + sx*r) + sy*u)``; orthographic:
``o = float32((e + sx*r) + sy*u)``, ``d = float32(w)``; per component, in the written order.  The predicate then runs on those
float32 values: the G-buffer (face, t, bary per pixel) equals ``Surface.ray_cast`` on the same rays bit for bit.

Shading
=======

A pixel without a face takes the background.  Otherwise, with the face normal ``n`` of clause 1 and the ray direction ``d``:
``intensity = ambient + ((1 - ambient)*|d.n|) / sqrt((d.d)*(n.n))`` in float64 with the dot products as in clause 3 --
two-sided, flat, a light at the eye.  The colour level ``c`` in ``[0, 255]`` per channel is a constant, the face's row of a
uint8 ``[F, 3]`` table, or a per-vertex float32 scalar ``s = (((1 - b1) - b2)*s_A + b1*s_B) + b2*s_C`` mapped as
``x = clamp((s - vmin)/(vmax - vmin), 0, 1)`` (``x = 0`` when ``vmax <= vmin`` and for a NaN) through the five-stop
piecewise-linear map

    ======  =====  =====  =====  ======  =====
    x       0      1/4    1/2    3/4     1
    colour  blue   cyan   green  yellow  red
    (r,g,b) 0,0,1  0,1,1  0,1,0  1,1,0   1,0,0
    ======  =====  =====  =====  ======  =====

as ``k = min(int(4x), 3)``, ``f = 4x - k``, ``c = 255*(stop_k + f*(stop_{k+1} - stop_k))``.  ``out = floor(c*intensity +
0.5)``.

The turntable reproduces ``util/render.py:19-45``: positions normalised to the box ``[-0.5, 0.5]^3``, the eye at ``(2, 2, 2)``,
the focus at the origin, ``frames`` frames ``360/frames`` degrees apart about +y.  The *camera* turns, not the mesh: the
images are the same and the tree is built once.  The up vector (+y) and the 30 degree view angle are this module's choice;
pixel parity with pyvista is not a goal.

Command line: ``python -m semigcn_amd.render --mesh out.obj [--gt gt.obj --error [--vmax X]] [--mask vmask.json]
[--turntable N] [--size W H] [--ssaa S] -o out.png`` (``--torus NU NV`` and ``--box N`` give synthetic inputs).
"""
from __future__ import annotations

import argparse
import contextlib
import json
import math
import struct
import sys
import zlib
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import capi
from .capi import SemigcnLibraryError
from .evaluate import Surface
from .mesh_common import Stages, check_mesh, device_tensor, points, read_obj, vs_faces

__all__ = ["Camera", "look_at", "camera_rays", "Image", "render", "turntable", "error_colors", "mask_colors", "write_png", "write_apng"]

#: util/datamaker.py:161-168: the colour of a kept face and of a masked one, as uint8 levels
MASK_KEPT, MASK_DROPPED = (85, 169, 255), (255, 0, 255)


@dataclass(frozen=True)
class Camera:
    """A pinhole (or, with ``ortho_height``, an orthographic) camera: the eye and an orthonormal basis in float64."""
    eye: tuple
    right: tuple
    up: tuple
    forward: tuple
    fov_deg: float = 30.0                      # the vertical view angle
    ortho_height: Optional[float] = None       # not None: orthographic, the view is this high

    @property
    def ortho(self) -> bool:
        return self.ortho_height is not None

    def params(self, width: int, height: int) -> list:
        """The 14 values eye, right, up, forward, tx, ty for an image of ``width x height`` pixels (square pixels)."""
        ty = 0.5 * float(self.ortho_height) if self.ortho else math.tan(math.radians(float(self.fov_deg)) / 2.0)
        tx = ty * (float(width) / float(height))
        return [*map(float, self.eye), *map(float, self.right), *map(float, self.up), *map(float, self.forward), tx, ty]


def look_at(eye, target, up=(0.0, 1.0, 0.0), fov_deg: float = 30.0, ortho_height: Optional[float] = None) -> Camera:
    """The camera at ``eye`` that looks at ``target``: forward = the unit vector eye -> target, right = forward x up, up =
    right x forward, in float64 on the host."""
    e, t, u = (np.asarray(x, np.float64).reshape(3) for x in (eye, target, up))
    w = t - e
    if not np.isfinite(w).all() or not np.linalg.norm(w) > 0:
        raise ValueError(f"look_at: eye {tuple(e)} and target {tuple(t)} give no view direction")
    w = w / np.linalg.norm(w)
    r = np.cross(w, u)
    if not np.linalg.norm(r) > 1e-12 * max(np.linalg.norm(u), 1e-300):
        raise ValueError(f"look_at: up {tuple(u)} is parallel to the view direction")
    r = r / np.linalg.norm(r)
    if not 0.0 < float(fov_deg) < 180.0:
        raise ValueError(f"fov_deg must be in (0, 180), got {fov_deg}")
    if ortho_height is not None and not float(ortho_height) > 0:
        raise ValueError(f"ortho_height must be > 0, got {ortho_height}")
    return Camera(tuple(e.tolist()), tuple(r.tolist()), tuple(np.cross(r, w).tolist()), tuple(w.tolist()), float(fov_deg),
                  None if ortho_height is None else float(ortho_height))


def camera_rays(camera: Camera, width: int, height: int):
    """``(origins, directions)`` float32 arrays [H * W, 3] of the primary rays of "Camera rays", pixel ``(x, y)`` at row
    ``y * width + x``, on the host: what ``render`` casts, for ``Surface.ray_cast`` or a caller's own use."""
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError(f"the image size must be at least 1 x 1, got {width} x {height}")
    p = np.asarray(camera.params(width, height), np.float64)
    e, r, u, w, tx, ty = p[0:3], p[3:6], p[6:9], p[9:12], p[12], p[13]
    y, x = (g.reshape(-1).astype(np.float64) for g in np.meshgrid(np.arange(height), np.arange(width), indexing="ij"))
    sx = ((2.0 * (x + 0.5)) / float(width) - 1.0) * tx
    sy = (1.0 - (2.0 * (y + 0.5)) / float(height)) * ty
    base = e if camera.ortho else w
    moving = np.stack([(base[k] + sx * r[k]) + sy * u[k] for k in range(3)], 1).astype(np.float32)
    fixed = np.ascontiguousarray(np.broadcast_to((w if camera.ortho else e).astype(np.float32), moving.shape))
    return (moving, fixed) if camera.ortho else (fixed, moving)


class Image(NamedTuple):
    """What ``render`` returns.  With ``ssaa = s > 1`` ``face`` and ``depth`` keep the ``s`` times larger sample grid."""
    rgb: torch.Tensor                  # uint8 [H, W, 3]
    face: torch.Tensor                 # int32 [s H, s W]: the face seen, 0x7fffffff where none
    depth: torch.Tensor                # float32 [s H, s W]: t of the hit along the pixel's ray, inf where none
    info: Optional[dict] = None        # rays, hit_fraction, leaf_visits_per_ray; with timings the stage times as well


def _size(width, height):
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError(f"the image size must be at least 1 x 1, got {width} x {height}")
    return width, height


def _check_colors(V: int, F: int, scalars, face_colors, ambient, ssaa):
    if int(ssaa) not in (1, 2, 3, 4):
        raise ValueError(f"ssaa must be one of 1, 2, 3, 4, got {ssaa}")
    if not 0.0 <= float(ambient) <= 1.0:
        raise ValueError(f"ambient must be in [0, 1], got {ambient}")
    if scalars is not None and face_colors is not None:
        raise ValueError("give scalars or face_colors, not both")
    if scalars is not None:
        shape = tuple(scalars.shape) if hasattr(scalars, "shape") else np.shape(scalars)
        if int(np.prod(shape)) != V or len(shape) > 2:
            raise ValueError(f"scalars must hold one value per vertex ({V}), got {shape}")
    if face_colors is not None:
        shape = tuple(face_colors.shape) if hasattr(face_colors, "shape") else np.shape(face_colors)
        if shape != (F, 3):
            raise ValueError(f"face_colors must be [F, 3] = [{F}, 3], got {shape}")
        dt = face_colors.dtype
        if dt not in (torch.uint8, np.dtype(np.uint8)):
            raise ValueError(f"face_colors must be uint8, got {dt}")


def _rgb(c, name: str):
    c = tuple(int(x) for x in c)
    if len(c) != 3 or min(c) < 0 or max(c) > 255:
        raise ValueError(f"{name} must be three levels in 0 .. 255, got {c}")
    return c


def _downsample(rgb: torch.Tensor, s: int) -> torch.Tensor:
    """uint8 [s H, s W, 3] -> uint8 [H, W, 3]: the integer average (sum + s*s // 2) // (s*s)."""
    if s == 1:
        return rgb
    H, W = rgb.shape[0] // s, rgb.shape[1] // s
    total = rgb.view(H, s, W, s, 3).to(torch.int32).sum(dim=(1, 3))
    return torch.div(total + (s * s) // 2, s * s, rounding_mode="floor").to(torch.uint8)


def _render(surf: Surface, camera: Camera, width: int, height: int, color, scalars, vmin, vmax, face_colors, background,
            ambient: float, ssaa: int, st: Stages) -> Image:
    cam = camera.params(width, height)
    W, H = width * ssaa, height * ssaa
    (depth, face, bary), visits, hit = surf.camera_cast(cam, camera.ortho, W, H)      # the frame's one synchronisation
    st.mark("render")                                                               # with the count of the pixels that hit
    scalars = None if scalars is None else scalars.to(surf.device)
    face_colors = None if face_colors is None else face_colors.to(surf.device)
    rgb = capi.shade_hits(surf.vs, surf.faces, face.view(-1), bary.view(-1, 2), cam=cam, ortho=camera.ortho, size=(W, H),
                          color=color, face_colors=face_colors, scalars=scalars, vmin=vmin, vmax=vmax, background=background,
                          ambient=ambient).view(H, W, 3)
    rgb = _downsample(rgb, ssaa)
    st.mark("shade")
    return Image(rgb, face, depth, {"rays": W * H, "hit_fraction": hit / (W * H), "leaf_visits_per_ray": visits / (W * H)})


def _prepare(mesh, scalars, vmin, vmax, face_colors, color, background, ambient, ssaa):
    """The argument errors that come before any device, then the device inputs: (context of a Surface, scalars, vmin, vmax,
    face_colors)."""
    if isinstance(mesh, Surface):
        V, F = mesh.vs.shape[0], mesh.faces.shape[0]
    else:
        vs, faces = check_mesh(mesh)
        V = int(vs.shape[0]) if hasattr(vs, "shape") else len(vs)
        F = int(faces.shape[0]) if hasattr(faces, "shape") else len(faces)
        if F == 0:
            raise ValueError("render: the mesh has no faces")
    _check_colors(V, F, scalars, face_colors, ambient, ssaa)
    color, background = _rgb(color, "color"), _rgb(background, "background")
    if scalars is not None:
        scalars = device_tensor(scalars, torch.float32, "scalars").reshape(-1)
        if vmin is None or vmax is None:                      # the range of the finite values: one synchronisation
            fin = scalars[torch.isfinite(scalars)]
            lo, hi = (float(fin.min()), float(fin.max())) if fin.numel() else (0.0, 0.0)
            vmin, vmax = (lo if vmin is None else vmin), (hi if vmax is None else vmax)
    if face_colors is not None:
        face_colors = device_tensor(face_colors, torch.uint8, "face_colors")
    surf = contextlib.nullcontext(mesh) if isinstance(mesh, Surface) else Surface(mesh)       # last: it lives in a with
    return surf, scalars, float(vmin or 0.0), float(vmax or 0.0), face_colors, color, background


def render(mesh, camera: Camera, width: int, height: int, *, color=(255, 165, 0), scalars=None, vmin=None, vmax=None,
           face_colors=None, background=(255, 255, 255), ambient: float = 0.25, ssaa: int = 1, timings: bool = False) -> Image:
    """One image of ``mesh`` -- a ``Surface``, a mesh object or a ``(vs, faces)`` pair -- by the rule of the module docstring.

    The base colour is ``color`` (the reference's orange), or per vertex ``scalars`` float [V] through the five-stop map
    over ``[vmin, vmax]`` (None: the range of the finite scalars), or ``face_colors`` uint8 [F, 3].  ``ssaa`` in 1..4 renders
    at ``ssaa`` times the size and averages in integers, ``(sum + s*s//2) // (s*s)``.  A ``Surface`` passed in is reused
    and left open; otherwise one is built here and closed.  One host synchronisation (the walk's own check; the counts of
    ``Image.info`` are read with it), and one more where the range of ``scalars`` has to be found."""
    width, height = _size(width, height)
    if not isinstance(camera, Camera):
        raise TypeError(f"camera must be a Camera (see look_at), got {type(camera).__name__}")
    ctx, scalars, vmin, vmax, face_colors, color, background = _prepare(mesh, scalars, vmin, vmax, face_colors, color,
                                                                        background, ambient, ssaa)
    with ctx as surf, capi._on_device(surf.device):
        st = Stages(surf.device, timings)
        img = _render(surf, camera, width, height, color, scalars, vmin, vmax, face_colors, background, float(ambient),
                      int(ssaa), st)
        if timings:
            img.info.update(st.result())
        return img


def normalize_to_box(vs: torch.Tensor) -> torch.Tensor:
    """util/render.py:19-25: every axis scaled to [-0.5, 0.5] on its own (float64, stored as float32); an axis without
    extent goes to -0.5."""
    v = vs.double()
    lo, hi = v.min(0).values, v.max(0).values
    ext = torch.where(hi > lo, hi - lo, torch.ones_like(lo))
    return ((v - lo) / ext - 0.5).float()


def turntable_camera(i: int, frames: int, fov_deg: float = 30.0) -> Camera:
    """The camera of frame ``i``: the mesh of util/render.py turns by ``360 i / frames`` degrees about +y under an eye at
    (2, 2, 2); here the eye turns the other way round."""
    a = -2.0 * math.pi * i / frames
    eye = (2.0 * math.cos(a) + 2.0 * math.sin(a), 2.0, -2.0 * math.sin(a) + 2.0 * math.cos(a))
    return look_at(eye, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), fov_deg)


def turntable(mesh, frames: int = 60, size=(400, 300), *, fov_deg: float = 30.0, color=(255, 165, 0), scalars=None, vmin=None,
              vmax=None, face_colors=None, background=(255, 255, 255), ambient: float = 0.25, ssaa: int = 1,
              timings: bool = False):
    """``Render(mesh, gif_name)`` of util/render.py:19-45 as uint8 [frames, H, W, 3] on the device (``size`` = (W, H)): the
    positions normalised to ``[-0.5, 0.5]^3``, the eye at (2, 2, 2), the focus at the origin, a frame every ``360/frames``
    degrees about +y.  One tree for all frames, one host synchronisation per frame.  With ``timings`` returns
    ``(images, info)``."""
    frames = int(frames)
    if frames < 1:
        raise ValueError(f"frames must be >= 1, got {frames}")
    width, height = _size(*size)
    if isinstance(mesh, Surface):
        mesh = (mesh.vs, mesh.faces)
    vs, faces = check_mesh(mesh)
    F = int(faces.shape[0]) if hasattr(faces, "shape") else len(faces)
    if F == 0:
        raise ValueError("turntable: the mesh has no faces")
    _check_colors(int(vs.shape[0]) if hasattr(vs, "shape") else len(vs), F, scalars, face_colors, ambient, ssaa)
    color, background = _rgb(color, "color"), _rgb(background, "background")
    p, f = vs_faces(vs, faces)
    with capi._on_device(p.device):
        st = Stages(p.device, timings)
        ctx, scalars, vmin, vmax, face_colors, color, background = _prepare((normalize_to_box(p), f), scalars, vmin, vmax,
                                                                            face_colors, color, background, ambient, ssaa)
        with ctx as surf:
            st.mark("build")
            out = torch.empty((frames, height, width, 3), dtype=torch.uint8, device=p.device)
            rays = hits = visits = 0.0
            for i in range(frames):
                img = _render(surf, turntable_camera(i, frames, fov_deg), width, height, color, scalars, vmin, vmax, face_colors,
                              background, float(ambient), int(ssaa), st)
                out[i] = img.rgb
                rays += img.info["rays"]
                hits += img.info["hit_fraction"] * img.info["rays"]
                visits += img.info["leaf_visits_per_ray"] * img.info["rays"]
        if not timings:
            return out
        info = {"frames": frames, "rays": int(rays), "hit_fraction": hits / rays, "leaf_visits_per_ray": visits / rays}
        info.update(st.result())
        return out, info


def error_colors(out, gt) -> torch.Tensor:
    """float32 [V_out]: the unsigned distance of every vertex of ``out`` to the surface ``gt`` (``Surface.query``), for use
    as ``scalars=`` of a render of ``out``."""
    pts = vs_faces(out)[0] if isinstance(out, (tuple, list)) else points(out)       # out's faces are not needed
    if isinstance(gt, Surface):
        return gt.query(pts, signed=False)[0]
    check_mesh(gt)
    with Surface(gt) as s:
        return s.query(pts, signed=False)[0]


def mask_colors(fmask):
    """uint8 [F, 3] for ``face_colors=``: the two colours of ``color_mask`` (util/datamaker.py:161-168), a kept face
    (``fmask != 0``) light blue, a masked one magenta.  A device tensor gives a device tensor, anything else an array."""
    if isinstance(fmask, torch.Tensor):
        keep = fmask.reshape(-1, 1) != 0
        return torch.where(keep, torch.tensor(MASK_KEPT, dtype=torch.uint8, device=fmask.device),
                           torch.tensor(MASK_DROPPED, dtype=torch.uint8, device=fmask.device))
    keep = np.asarray(fmask).reshape(-1, 1) != 0
    return np.where(keep, np.asarray(MASK_KEPT, np.uint8), np.asarray(MASK_DROPPED, np.uint8))


# ---- image files: zlib and struct only ----------------------------------------------------------------------------------

_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def _host_rgb(rgb, dims: int) -> np.ndarray:
    a = rgb.detach().cpu().numpy() if isinstance(rgb, torch.Tensor) else np.asarray(rgb)
    if a.dtype != np.uint8 or a.ndim != dims or a.shape[-1] != 3 or 0 in a.shape:
        raise ValueError(f"expected a non-empty uint8 array of {dims} dimensions with 3 channels, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def _scanlines(img: np.ndarray) -> bytes:
    """the zlib stream of an image: every row behind a filter byte 0"""
    H, W, _ = img.shape
    rows = np.zeros((H, 1 + 3 * W), np.uint8)
    rows[:, 1:] = img.reshape(H, 3 * W)
    return zlib.compress(rows.tobytes(), 6)


def _ihdr(W: int, H: int) -> bytes:
    return _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))      # 8 bits, truecolour


def write_png(path: str, rgb) -> None:
    """``rgb`` uint8 [H, W, 3] (a tensor or an array) as an 8-bit truecolour PNG."""
    img = _host_rgb(rgb, 3)
    with open(path, "wb") as f:
        f.write(_PNG_MAGIC + _ihdr(img.shape[1], img.shape[0]) + _chunk(b"IDAT", _scanlines(img)) + _chunk(b"IEND", b""))


def write_apng(path: str, frames, delay_ms: int = 50) -> None:
    """``frames`` uint8 [N, H, W, 3] as an animated PNG that loops for ever, ``delay_ms`` per frame; a viewer without APNG
    support shows frame 0."""
    a = _host_rgb(frames, 4)
    N, H, W, _ = a.shape
    delay_ms = int(delay_ms)
    if not 0 <= delay_ms <= 0xFFFF:
        raise ValueError(f"delay_ms must be in 0 .. 65535, got {delay_ms}")
    out = [_PNG_MAGIC, _ihdr(W, H), _chunk(b"acTL", struct.pack(">II", N, 0))]
    seq = 0
    for i in range(N):
        out.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, W, H, 0, 0, delay_ms, 1000, 0, 0)))
        seq += 1
        data = _scanlines(a[i])
        if i == 0:
            out.append(_chunk(b"IDAT", data))
        else:
            out.append(_chunk(b"fdAT", struct.pack(">I", seq) + data))
            seq += 1
    out.append(_chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(b"".join(out))


try:
    from PIL import Image as _PILImage
except ImportError:
    _PILImage = None

if _PILImage is not None:
    __all__.append("write_gif")

    def write_gif(path: str, frames, delay_ms: int = 50) -> None:
        """``frames`` uint8 [N, H, W, 3] as a looping GIF, as util/render.py:45 saves it (offered only where PIL imports)."""
        ims = [_PILImage.fromarray(x) for x in _host_rgb(frames, 4)]
        ims[0].save(path, save_all=True, append_images=ims[1:], optimize=True, duration=int(delay_ms), loop=0)


def main(argv=None) -> int:
    from . import synth
    ap = argparse.ArgumentParser(prog="python -m semigcn_amd.render",
                                 description="render a triangle mesh on the device: one image from (2, 2, 2) or the "
                                             "turntable of util/render.py, flat-shaded, as an error heat map or with its mask")
    ap.add_argument("--mesh", help="the mesh to look at (OBJ)")
    ap.add_argument("--torus", type=int, nargs=2, metavar=("NU", "NV"), help="a synthetic torus instead of an OBJ")
    ap.add_argument("--box", type=int, metavar="N", help="the unit box with an N x N grid per side instead of an OBJ")
    ap.add_argument("--gt", help="the ground truth (OBJ) of --error")
    ap.add_argument("--error", action="store_true", help="colour by the distance of the mesh's vertices to --gt")
    ap.add_argument("--vmax", type=float, help="the distance that maps to red (default: the largest)")
    ap.add_argument("--mask", help="a vertex mask (JSON list, 1 = kept): colour the faces as util/datamaker.py's color_mask")
    ap.add_argument("--turntable", type=int, metavar="N", help="N frames about +y, written as an animated PNG")
    ap.add_argument("--size", type=int, nargs=2, default=(400, 300), metavar=("W", "H"))
    ap.add_argument("--ssaa", type=int, default=1, choices=(1, 2, 3, 4), help="samples per pixel and axis")
    ap.add_argument("--repeat", type=int, default=1, help="run this many times and report the last")
    ap.add_argument("-o", "--output", help="where the image goes (PNG; APNG with --turntable)")
    args = ap.parse_args(argv)
    if (args.mesh is not None) + (args.torus is not None) + (args.box is not None) != 1:
        ap.error("give exactly one of --mesh IN.obj, --torus NU NV and --box N")
    if args.error != (args.gt is not None):
        ap.error("--error and --gt go together")
    if args.error and args.mask:
        ap.error("give --error or --mask, not both")
    if min(args.size) < 1 or args.repeat < 1 or (args.turntable is not None and args.turntable < 1):
        ap.error("--size, --repeat and --turntable must be >= 1")
    if args.mesh is not None:
        vs, faces = read_obj(args.mesh)
    elif args.box is not None:
        vs, faces = synth.box_mesh(args.box)
    else:
        m = synth.torus_mesh(args.torus[0], args.torus[1], jitter=0.0, masks=False)
        vs, faces = m.vs.astype(np.float32), m.faces
    p, f = vs_faces(vs, faces)
    kw = {"ssaa": args.ssaa}
    if args.error:
        kw.update(scalars=error_colors(p, read_obj(args.gt)), vmin=0.0, vmax=args.vmax)
    if args.mask:
        with open(args.mask) as fh:
            vmask = torch.as_tensor(np.asarray(json.load(fh)).reshape(-1) != 0).to(p.device)
        if vmask.numel() != p.shape[0]:
            ap.error(f"--mask holds {vmask.numel()} entries, the mesh has {p.shape[0]} vertices")
        kw.update(face_colors=mask_colors(vmask[f].all(1)))               # vmask_to_fmask: a face is kept with all its vertices
    for _ in range(args.repeat):
        if args.turntable is not None:
            images, info = turntable((p, f), args.turntable, tuple(args.size), timings=True, **kw)
        else:
            st = Stages(p.device, True)
            with Surface(normalize_to_box(p), f) as surf:            # turntable() normalises by itself
                st.mark("build")
                img = render(surf, turntable_camera(0, 1), args.size[0], args.size[1], timings=True, **kw)
            images, info = img.rgb, dict(img.info)
            info.update(st.result())
    rec = {"n_vertices": int(p.shape[0]), "n_faces": int(f.shape[0]), "size": list(args.size), "ssaa": args.ssaa}
    rec.update({k: (round(v, 4) if isinstance(v, float) else v) for k, v in info.items()})
    if rec.get("render_ms"):
        rec["mrays_per_s"] = round(rec["rays"] / rec["render_ms"] / 1e3, 2)
    if args.output:
        (write_apng if args.turntable is not None else write_png)(args.output, images)
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
