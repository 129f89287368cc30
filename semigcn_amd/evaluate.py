"""Scoring a completed mesh on the device: the reference's quality metric.

Replaces check/dist_check.py:13-67 (``simple_mesh_distance`` / ``mesh_distance``), which sgcn.py:183,193 and
mgcn.py:175,201,213 call after training and after refinement, and the loop of check/batch_dist_check.py.  The
reference gets its numbers from pymeshlab's ``distance_from_reference_mesh`` filter; here the closest-point query runs
on a bounding-volume hierarchy built on the device (csrc/mesh_dist.hip, ``sg_surface_*``).

Rules where MeshLab's behaviour cannot be reproduced:
  * the search is exact and has no bound (MeshLab's ``maxdist`` is not imitated);
  * the closest face is the one with the smallest float32 distance, the lowest face index on an exact tie;
  * a signed distance has the sign of ``dot((b - a) x (c - a), p - closest)`` for that face; a zero distance is +0.

Inputs: CUDA tensors, numpy arrays (copied to the current device), or objects with ``.vs`` / ``.faces`` (the
reference's ``Mesh``, ``meshprep.DeviceMesh``, ``synth.SynthMesh``).  There is no CPU path: a CPU tensor raises
``SemigcnLibraryError``.

Command line::

    python -m semigcn_amd.evaluate --gt gt.obj --org original.obj --out out.obj [--real]

prints one JSON line with ``hd_all``, ``hd_hole``, ``n_hole`` and ``diag``.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from typing import Optional

import torch

from . import capi, mesh_common
from .capi import SemigcnLibraryError
from .mesh_common import device_tensor, read_obj, vs_faces

#: check/dist_check.py:36-40: the hole threshold on the unsigned distance gt -> org (meshes scaled to unit mean edge)
EPS_SIMULATED, EPS_REAL = 0.05, 1.0


class Surface:
    """The triangles of one surface, with their hierarchy built once on the device; ``query`` then scores any number
    of point sets against it.  Open and non-manifold surfaces are fine (the reference loads org with manifold=False)."""

    def __init__(self, vs, faces=None):
        self.vs, self.faces = vs_faces(vs, faces)
        self._h = capi.SurfaceHandle(self.vs, self.faces)

    @property
    def device(self) -> torch.device:
        return self.vs.device

    def query(self, points, signed: bool = True):
        """(dist float32 [N], face int32 [N], closest float32 [N, 3]): the distance from every point to the surface
        (signed by the face normal when ``signed``), the face the closest point lies on, and that point.  A point with a
        NaN or an infinite coordinate gets ``dist = inf``, ``face = 0x7fffffff`` and a NaN ``closest`` row, and leaves
        the other rows alone: test ``torch.isinf(dist)`` before indexing with ``face``."""
        pts = mesh_common.points(points)
        if pts.device != self.device:
            pts = pts.to(self.device)
        return self._h.query(pts, signed=signed)

    def close(self):
        self._h.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._h.__exit__(*exc)


def _surface(x) -> Surface:
    return x if isinstance(x, Surface) else Surface(x)


def mesh_distance(gt, org, out, real: bool = False, eps: Optional[float] = None, hole=None) -> dict:
    """The reference's ``mesh_distance(gt_path, org_path, out_path, real)`` (check/dist_check.py:35-67).

    ``hd_all = mean(|q|) / diag`` and ``hd_hole = mean(|q[hole]|) / diag``, where ``q[i]`` is the signed distance
    from gt vertex i to the surface of ``out``, ``diag`` the diagonal of gt's vertex box, and ``hole = q_org > eps``
    with ``q_org[i]`` the unsigned distance from gt vertex i to the surface of ``org`` (eps = 0.05, or 1.0 when
    ``real``).  Despite the names the reference uses, these are mean one-sided distances, not Hausdorff distances.
    When no vertex is in the hole (``n_hole == 0``) ``hd_hole`` is nan, as the reference's 0 / 0 gives.

    To score many results against one gt (check/batch_dist_check.py), take ``hole`` from a first call and pass it
    in: ``org`` is then not used and may be None.

    Returns a dict: the scalars ``hd_all``, ``hd_hole``, ``n_hole``, ``diag``; per gt vertex ``q`` (signed, gt -> out)
    and ``hole`` (bool); per out vertex ``q_out`` (signed, out -> gt: the reference's second filter call, which only
    colours out's vertices).  ``gt`` needs faces (it is the surface of the q_out query).  The scalars cost one host
    synchronisation."""
    gt_s, out_s = _surface(gt), _surface(out)
    gt_vs = gt_s.vs
    if eps is None:
        eps = EPS_REAL if real else EPS_SIMULATED
    q_org = None
    if hole is None:
        if org is None:
            raise ValueError("mesh_distance: org is needed unless hole is given")
        q_org = _surface(org).query(gt_vs, signed=False)[0]
    else:
        hole = device_tensor(hole, torch.bool, "hole")
    q = out_s.query(gt_vs, signed=True)[0]
    q_out = gt_s.query(out_s.vs, signed=True)[0]
    sums, hole_mask = capi.mesh_distance_reduce(q, gt_vs, q_org=q_org, eps=float(eps), hole=hole)
    s_all, s_hole, n_hole, diag = sums.tolist()         # the one host synchronisation
    N = gt_vs.shape[0]
    hd_all = s_all / N / diag if N and diag else float("nan")
    hd_hole = s_hole / n_hole / diag if n_hole and diag else float("nan")
    return {"hd_all": hd_all, "hd_hole": hd_hole, "n_hole": int(n_hole), "diag": diag,
            "q": q, "hole": hole_mask, "q_out": q_out}


def simple_mesh_distance(gt, out) -> float:
    """``hd_all`` alone, without org (check/dist_check.py:13-33)."""
    gt_vs = vs_faces(gt)[0] if isinstance(gt, (tuple, list)) else mesh_common.points(gt)     # gt's faces are not needed
    q = _surface(out).query(gt_vs, signed=True)[0]
    sums, _ = capi.mesh_distance_reduce(q, gt_vs, hole=torch.zeros(gt_vs.shape[0], dtype=torch.bool, device=q.device))
    s_all, _, _, diag = sums.tolist()
    return s_all / gt_vs.shape[0] / diag if gt_vs.shape[0] and diag else float("nan")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m semigcn_amd.evaluate",
                                 description="mean point-to-surface distances of a completed mesh "
                                             "(check/dist_check.py::mesh_distance)")
    ap.add_argument("--gt", required=True, help="ground-truth mesh (OBJ)")
    ap.add_argument("--org", help="original scan with holes (OBJ); without it only hd_all is reported")
    ap.add_argument("--out", required=True, help="completed mesh to score (OBJ)")
    ap.add_argument("--real", action="store_true", help="hole threshold 1.0 instead of 0.05 (real scans)")
    args = ap.parse_args(argv)
    gt, out = read_obj(args.gt), read_obj(args.out)
    if args.org:
        r = mesh_distance(gt, read_obj(args.org), out, real=args.real)
        res = {k: r[k] for k in ("hd_all", "hd_hole", "n_hole", "diag")}
    else:
        res = {"hd_all": simple_mesh_distance(gt, out)}
    print(json.dumps({k: (None if isinstance(v, float) and math.isnan(v) else v) for k, v in res.items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
