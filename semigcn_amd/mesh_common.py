"""What the mesh stages share in Python: the sibling of csrc/mesh_common.h.

``evaluate``, ``prepare``, ``holes``, ``manifold``, ``components``, ``repair``, ``remesh``, ``simplify``, ``denoise``, ``render`` and ``align`` take their inputs, read and write their OBJ
files and time their stages through this module, and through nothing of each other's that starts with an underscore.

The lifetime rule of the objects those stages build (``capi.SmoothPlan`` / ``FillPlan`` / ``FairPlan`` / ``PartsPlan`` / ``ManifoldPlan`` / ``RemeshPlan`` / ``SamplerPlan`` / ``VertexUpdatePlan``,
``evaluate.Surface``): one made inside a function lives in a ``with``.  Leaving the block waits for the device's current
stream and then closes the object, in that order, with or without an exception -- the object's buffers are freed with it,
and a kernel launched inside the block may still read them.
"""
from __future__ import annotations

import numpy as np
import torch

from .capi import SemigcnLibraryError

__all__ = ["device_tensor", "vs_faces", "points", "check_mesh", "read_obj", "write_obj", "Stages"]


def device_tensor(x, dtype: torch.dtype, name: str) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            raise SemigcnLibraryError(
                f"{name} is on {x.device}: semigcn_amd.evaluate runs on a HIP device only (there is no CPU path; "
                "pass a cuda tensor or a numpy array)")
        return x.detach().to(dtype).contiguous()
    if not torch.cuda.is_available():
        raise SemigcnLibraryError(f"{name}: no HIP device to copy the array to (semigcn_amd.evaluate has no CPU path)")
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x)), dtype=dtype).to(
        torch.device("cuda", torch.cuda.current_device())).contiguous()


def _pair(mesh, faces=None):
    """(vs, faces) as they were passed: from the two arguments, a (vs, faces) pair or an object with .vs / .faces."""
    if faces is not None:
        return mesh, faces
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        return tuple(mesh)
    if hasattr(mesh, "vs") and hasattr(mesh, "faces"):
        return mesh.vs, mesh.faces
    raise TypeError("expected a mesh with .vs / .faces or a (vs, faces) pair")


def vs_faces(mesh, faces=None):
    """(vs float32 [V, 3], faces int64 [F, 3]) on the device from a mesh object or a (vs, faces) pair."""
    mesh, faces = _pair(mesh, faces)
    vs = device_tensor(mesh, torch.float32, "vs")
    f = device_tensor(faces, torch.int64, "faces")
    if f.device != vs.device:
        f = f.to(vs.device)
    return vs.reshape(-1, 3), f.reshape(-1, 3)


def points(x) -> torch.Tensor:
    if hasattr(x, "vs"):
        x = x.vs
    return device_tensor(x, torch.float32, "points").reshape(-1, 3)


def check_mesh(mesh, faces=None, dtypes: bool = True):
    """The ``TypeError`` and ``ValueError``s of a tensor / array mesh that come before any device is asked for: ``vs`` must
    be [V, 3] and ``faces`` [F, 3]; with ``dtypes``, ``vs`` must hold floats and ``faces`` integers.  Returns the
    ``(vs, faces)`` pair as it was passed."""
    pair = _pair(mesh, faces)
    for x, name, kinds in zip(pair, ("vs", "faces"), ("f", "iu")):
        shape = tuple(x.shape) if hasattr(x, "shape") else np.shape(x)
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError(f"{name} must be [{name[0].upper()}, 3], got {shape}")
        if not dtypes:
            continue
        if isinstance(x, torch.Tensor):
            ok = x.dtype.is_floating_point if kinds == "f" else x.dtype in (torch.int64, torch.int32)
        else:
            ok = np.asarray(x).dtype.kind in kinds
        if not ok:
            raise ValueError(f"{name} must hold {'floats' if kinds == 'f' else 'integers'}, got {getattr(x, 'dtype', type(x))}")
    return pair


def read_obj(path: str):
    """(vs float32 [V, 3], faces int64 [F, 3]) in the dialect util/mesh.py:35-58 reads: ``v x y z`` with an optional
    colour, ``f a b c`` with ``a/b/c`` slash forms and negative (relative) indices; anything but a triangle is an
    error."""
    vs, faces = [], []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                vs.append([float(t) for t in tok[1:4]])
            elif tok[0] == "f":
                ids = [int(t.split("/")[0]) for t in tok[1:]]
                if len(ids) != 3:
                    raise ValueError(f"{path}:{ln}: face with {len(ids)} vertices (only triangles are read)")
                faces.append([i - 1 if i >= 0 else len(vs) + i for i in ids])
    v = np.asarray(vs, dtype=np.float32).reshape(-1, 3)
    fc = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if fc.size and (fc.min() < 0 or fc.max() >= v.shape[0]):
        raise ValueError(f"{path}: face index outside [0, {v.shape[0]})")
    return v, fc


def write_obj(path: str, vs, faces=None) -> None:
    """The inverse of ``read_obj``, from tensors or arrays: ``v x y z`` lines with ``%.9g`` (a float32 round-trips bit for
    bit) and 1-based ``f a b c`` lines; ``faces`` None or empty: vertices only."""
    v = (vs.detach().cpu().numpy() if isinstance(vs, torch.Tensor) else np.asarray(vs)).reshape(-1, 3)
    with open(path, "w") as f:
        f.write("".join("v %.9g %.9g %.9g\n" % (p[0], p[1], p[2]) for p in v.tolist()))
        if faces is not None:
            fc = (faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)).reshape(-1, 3)
            f.write("".join("f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1) for t in fc.tolist()))


class Stages:
    """Device time of named stages, from events on the current stream, summed by name.  With ``on=False`` every method
    returns at once and no CUDA call is made."""

    def __init__(self, device, on: bool):
        self.on, self.device, self.marks = on, device, []
        self.mark(None)

    def mark(self, name):
        """The time since the previous mark goes to ``name``; ``None`` restarts the clock and charges that time to nobody."""
        if self.on:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(self.device))
            self.marks.append((name, e))

    def result(self):
        """``{name + "_ms": milliseconds}`` in the order the names first came up (one synchronisation); None when off."""
        if not self.on:
            return None
        torch.cuda.synchronize(self.device)
        ms = {}
        for (_, start), (name, end) in zip(self.marks, self.marks[1:]):
            if name is not None:
                ms[name + "_ms"] = ms.get(name + "_ms", 0.0) + start.elapsed_time(end)
        return ms

    @staticmethod
    def record(stage_ms: dict) -> dict:
        """``stage_ms`` as the command lines print it."""
        return {k: round(v, 4) for k, v in stage_ms.items()}
