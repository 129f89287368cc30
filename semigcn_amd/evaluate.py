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

prints one JSON line with ``hd_all``, ``hd_hole``, ``n_hole`` and ``diag``.  With ``--sampled N [--seed S] [--tau T]
[--order face|draw]`` the line also carries the two-sided sampled distance of ``surface_distance`` (``hausdorff``,
``chamfer``, their ``_rel``, ``max_ab`` .. ``rms_ba``, ``normal_consistency``) and the device time of its stages
(``sample_ms``, ``query_ms``, ``stats_ms``); ``--org`` is then optional.  With ``--align rigid|similarity`` ``out`` is first
moved onto ``gt`` by ``semigcn_amd.align.align`` (both complete meshes; samples of ``out`` with ``--seed``) and ``org`` by
the same matrix, and the line gains ``align_scale``, ``align_iterations`` and ``align_converged``.

Sampling rule
-------------
``mesh_distance`` is the reference's number: a mean over the *vertices of gt* of the distance to ``out``.  It never looks
from ``out`` to ``gt`` (a spike, a fold or a ballooned patch of ``out`` costs nothing) and it weights the surface by where
its vertices happen to be.  ``surface_distance`` measures both directions on area-weighted samples, as MeshLab's
``hausdorff_distance`` filter does.  The samples are DEFINED by the rule below, and every choice in it is integer
arithmetic: csrc/mesh_sample.hip and the numpy restatement tests/sample_oracle.py give identical bytes, and so do two runs.

**Weights.**  Per face, ``A, B, C`` are the float32 vertices widened to float64, ``e1 = B - A``, ``e2 = C - A``,
``n = e1 x e2`` written out (``nx = e1y*e2z - e1z*e2y``, ...), ``nn = (nx*nx + ny*ny) + nz*nz`` -- plain multiplies and
adds in that order, no fused multiply-add.  A vertex id outside ``[0, V)`` or a non-finite ``nn`` is a ``ValueError``
(checked on the device before anything is read through the id).  A face whose ``face_mask`` entry is 0 has ``nn = 0``.
With ``m = max nn`` (exact in any order): ``m == 0`` makes every weight 0; otherwise ``m = f * 2^e``, ``f`` in
``[0.5, 1)``, ``s = 62 - e``, ``q_f = floor(ldexp(nn_f, s))`` as a uint64 below 2^62 and ``w_f = isqrt(q_f)``, the exact
integer square root (a float64 ``sqrt`` estimate corrected by ``while r*r > q: r -= 1`` and ``while (r+1)*(r+1) <= q:
r += 1``, so it does not depend on how ``sqrt`` rounds).  ``w_f < 2^31`` is proportional to the face's area.  A face
below 2^-31 of the largest area gets weight 0 and is never drawn; ``n_zero_weight`` counts the faces of weight 0 (masked
ones included).  ``cdf`` uint64 ``[F + 1]`` is the exclusive prefix sum of ``w`` (integer, so order-free) and
``W = cdf[F]``.

**Draw k** (``k = offset + i``, a uint64).  ``x0..x3 = Philox4x32-10(counter = (k lo32, k hi32, 0, 0), key = (seed lo32,
seed hi32))``; ``r = x1 << 32 | x0``; ``t = mulhi64(r, W)``; the face is the ``f`` with ``cdf[f] <= t < cdf[f+1]`` (binary
search, upper bound minus one); ``a = x2 >> 8``, ``b = x3 >> 8``, and if ``a + b > 2^24`` then ``a = 2^24 - a``,
``b = 2^24 - b``; ``w0 = 2^24 - a - b`` (a reflection, no square root).  The point is ``((w0*A + a*B) + b*C) * 2^-24``
in float64 per coordinate, rounded to float32 once.  A draw depends on ``(seed, k)`` and the mesh only: chunks of one
stream (``offset``) concatenate.

**Order.**  ``order="face"`` (the default) emits the draws sorted by ``(face, k)`` -- one stable radix sort --, so that
neighbouring lanes of the closest-point walk start near each other; ``"draw"`` emits them by ``k``.

**Limits.**  ``F < 2^31`` and ``n < 2^31`` per call.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import math
import sys
from typing import NamedTuple, Optional

import torch

from . import capi, mesh_common
from .capi import SemigcnLibraryError
from .mesh_common import device_tensor, read_obj, vs_faces

#: check/dist_check.py:36-40: the hole threshold on the unsigned distance gt -> org (meshes scaled to unit mean edge)
EPS_SIMULATED, EPS_REAL = 0.05, 1.0


class Hits(NamedTuple):
    """What ``Surface.ray_cast`` returns, one row per ray; a ray that hits nothing has ``t = inf``, ``face = 0x7fffffff`` and
    a NaN ``bary`` row."""
    t: torch.Tensor           # float32 [N]: the hit is at origin + t * direction
    face: torch.Tensor        # int32 [N]: the face hit
    bary: torch.Tensor        # float32 [N, 2]: the weights of the face's second and third vertex at the hit


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

    def ray_cast(self, origins, directions, t_min: float = 0.0, t_max: float = math.inf, with_visits: bool = False):
        """The first hit of every ray ``origins[i] + t * directions[i]``, ``t`` in the closed range ``[t_min, t_max]``, by
        the rule of ``semigcn_amd.render`` ("The rule"): ``Hits`` with the smallest ``t``, the lowest face id on an exact tie;
        the directions need not be unit vectors (``t`` counts in their length).  A miss, a ray with a NaN or an infinite
        component and a zero direction get ``t = inf``, ``face = 0x7fffffff`` and a NaN ``bary`` row, and leave the other rows
        alone: test ``torch.isinf(t)`` before indexing with ``face``.  ``with_visits``: ``(Hits, leaves visited)``, the visits
        summed over the rays, for profiles.  One host synchronisation (the walk's own check that it dropped no subtree)."""
        o, d = mesh_common.points(origins).to(self.device), mesh_common.points(directions).to(self.device)
        if o.shape != d.shape:
            raise ValueError(f"{o.shape[0]} origins and {d.shape[0]} directions")
        t, face, bary, stats = self._h.ray_cast(self.vs, self.faces, o, d, t_min, t_max)
        visits = capi.check_walk_stats(stats, "Surface.ray_cast")
        return (Hits(t, face, bary), visits) if with_visits else Hits(t, face, bary)

    def camera_cast(self, cam, ortho: bool, width: int, height: int, t_min: float = 0.0, t_max: float = math.inf):
        """``ray_cast`` on the ``width x height`` primary rays of a camera, generated on the device (``semigcn_amd.render``,
        "Camera rays"; ``cam``: the 14 values of ``render.Camera.params``): ``(Hits`` with [H, W] rows, leaves visited,
        pixels that see a face``)``.  What ``render.render`` is built on.  The same check and the same one synchronisation
        as ``ray_cast``; the two counts are read with it."""
        face, t, bary, stats = self._h.render(self.vs, self.faces, cam, ortho, width, height, t_min, t_max)
        visits, seen = capi.check_walk_stats(stats, "Surface.camera_cast", (face != capi.NO_FACE).sum())
        return Hits(t, face, bary), visits, seen

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


class Samples(NamedTuple):
    """What ``sample_surface`` returns: ``points`` float32 [n, 3]; ``face`` int64 [n], the face each point lies on;
    ``bary`` int32 [n, 3] = (w0, a, b) out of 2^24, the weights of the face's three vertices; ``index`` int64 [n], the
    draw k of each row; ``total_weight`` = W and ``n_zero_weight``, the faces that are never drawn."""
    points: torch.Tensor
    face: torch.Tensor
    bary: torch.Tensor
    index: torch.Tensor
    total_weight: int
    n_zero_weight: int


def _face_mask(mask, device):
    return None if mask is None else device_tensor(mask, torch.bool, "face_mask").reshape(-1).to(device)


def sample_surface(mesh, n: int, seed: int = 0, offset: int = 0, face_mask=None, order: str = "face") -> Samples:
    """``n`` area-weighted points on the surface of ``mesh`` by the sampling rule of the module docstring: draws
    ``offset .. offset + n - 1`` of the stream ``seed``, sorted by (face, index) or, with ``order="draw"``, by index.
    ``face_mask`` [F] (0 = never draw from this face).  ``ValueError`` for a face index outside [0, V), a NaN or
    infinite vertex of a face, and for ``n > 0`` when every face has weight 0.  HIP device only."""
    vs, faces = vs_faces(*mesh_common.check_mesh(mesh))
    with capi.SamplerPlan(vs, faces, _face_mask(face_mask, vs.device)) as plan:
        points, face, bary, index = plan.draw(n, seed=seed, offset=offset, order=order)
        return Samples(points, face.to(torch.int64), bary, index, plan.total_weight, plan.n_zero_weight)


def _direction(src: Surface, src_mask, dst: Surface, n: int, seed: int, vertices: bool, tau, order: str, st, extra):
    """One direction of ``surface_distance``: the per-sample tensors, and the device scalars (5 of sg_distance_stats, 2 of
    sg_normal_agreement, then ``extra``) as one host list -- the direction's one synchronisation for scalars."""
    n = int(n)
    if n > 0:
        with capi.SamplerPlan(src.vs, src.faces, _face_mask(src_mask, src.device)) as plan:
            points, face = plan.draw(n, seed=seed, order=order)[:2]
    else:
        points = torch.empty((0, 3), dtype=torch.float32, device=src.device)
        face = torch.empty(0, dtype=torch.int32, device=src.device)
    face_from = face.to(torch.int64)
    if vertices:
        points = torch.cat([points, src.vs])
        face_from = torch.cat([face_from, torch.full((src.vs.shape[0],), -1, dtype=torch.int64, device=src.device)])
    st.mark("sample")
    dist, face_to, closest = dst.query(points, signed=False)
    st.mark("query")
    stats = capi.distance_stats(dist, tau)
    agree = capi.normal_agreement(src.vs, src.faces, face, dst.vs, dst.faces, face_to[:n])   # the vertices take no part
    st.mark("stats")
    mx, s1, s2, cnt, skipped, cos_sum, cos_n, *rest = torch.cat([stats, agree] + extra).tolist()
    nv = points.shape[0] - int(skipped)
    nan = float("nan")
    res = {"max": mx, "mean": s1 / nv if nv else nan, "rms": math.sqrt(s2 / nv) if nv else nan, "n": nv,
           "within": None if tau is None else (cnt / nv if nv else nan),
           "normal_consistency": cos_sum / cos_n if cos_n else nan,
           "points": points, "dist": dist, "face_from": face_from, "face_to": face_to, "closest": closest}
    return res, rest


def surface_distance(a, b, n: int = 100000, seed: int = 0, vertices: bool = True, tau: Optional[float] = None,
                     a_face_mask=None, b_face_mask=None, order: str = "face", stages=None) -> dict:
    """The two-sided sampled distance between the surfaces ``a`` and ``b`` (meshes, or ``Surface`` s already built).

    Direction ``ab``: ``n`` samples on ``a`` by the sampling rule of the module docstring (stream ``seed``; only faces
    with a non-zero ``a_face_mask`` entry when that is given), with ``vertices`` followed by all of ``a``'s vertices;
    the unsigned distance of each to the surface of ``b``.  Direction ``ba``: the same from ``b`` with ``b_face_mask``
    and the stream ``seed + 1``.  Each direction is a dict of ``max``, ``mean``, ``rms`` of the distances, their count
    ``n`` (a point without a closest point -- a NaN vertex -- is left out), ``within`` (the share with distance <=
    ``tau``; None without ``tau``), ``normal_consistency`` (the mean of ``|cos|`` between the normal of the face a sample
    was drawn from and that of the face its closest point lies on; appended vertices and zero-area faces take no part),
    and per point ``points``, ``dist``, ``face_from`` (-1 for an appended vertex), ``face_to``, ``closest``.

    On top: ``hausdorff = max(ab.max, ba.max)``, ``chamfer = ab.mean + ba.mean``, ``normal_consistency`` (the mean of the
    two directions'), ``diag`` (the diagonal of the box of ``a``'s vertices, as in ``mesh_distance``) and
    ``hausdorff_rel``, ``chamfer_rel``: the two divided by ``diag``.  To score a patch alone, mask ``a`` down to it:
    ``a_face_mask = meshprep.vmask_to_fmask(topology, ~prepared.v_mask)`` (the faces among the vertices that
    ``Prepared.inserted`` lists) and ``vertices=False``.

    Two calls give identical bytes in every tensor and scalar.  The scalars cost one host synchronisation per direction.
    ``stages``: a ``mesh_common.Stages`` that is charged ``sample``, ``query`` and ``stats``."""
    n = int(n)
    if n < 0:
        raise ValueError(f"surface_distance: n must be >= 0, got {n}")
    if tau is not None and not float(tau) >= 0.0:
        raise ValueError(f"surface_distance: tau must be >= 0 or None, got {tau}")
    for x in (a, b):
        if not isinstance(x, Surface):
            mesh_common.check_mesh(x)
    with contextlib.ExitStack() as stack:
        sa, sb = (x if isinstance(x, Surface) else stack.enter_context(Surface(x)) for x in (a, b))
        if sb.device != sa.device:
            raise SemigcnLibraryError(f"a on {sa.device}, b on {sb.device}")
        st = stages if stages is not None else mesh_common.Stages(sa.device, False)
        st.mark(None)
        box = sa.vs.to(torch.float64)
        ext = box.amax(0) - box.amin(0) if box.shape[0] else box.new_zeros(3)
        ab, (diag,) = _direction(sa, a_face_mask, sb, n, seed, vertices, tau, order, st, [(ext * ext).sum().sqrt().reshape(1)])
        ba, _ = _direction(sb, b_face_mask, sa, n, seed + 1, vertices, tau, order, st, [])
    hausdorff, chamfer = max(ab["max"], ba["max"]), ab["mean"] + ba["mean"]
    rel = (lambda v: v / diag) if diag else (lambda v: float("nan"))
    return {"ab": ab, "ba": ba, "hausdorff": hausdorff, "chamfer": chamfer, "diag": diag,
            "hausdorff_rel": rel(hausdorff), "chamfer_rel": rel(chamfer),
            "normal_consistency": 0.5 * (ab["normal_consistency"] + ba["normal_consistency"])}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m semigcn_amd.evaluate",
                                 description="mean point-to-surface distances of a completed mesh "
                                             "(check/dist_check.py::mesh_distance)")
    ap.add_argument("--gt", required=True, help="ground-truth mesh (OBJ)")
    ap.add_argument("--org", help="original scan with holes (OBJ); without it only hd_all is reported")
    ap.add_argument("--out", required=True, help="completed mesh to score (OBJ)")
    ap.add_argument("--real", action="store_true", help="hole threshold 1.0 instead of 0.05 (real scans)")
    ap.add_argument("--sampled", type=int, metavar="N", help="also the two-sided sampled distance (surface_distance) "
                                                             "on N area-weighted samples per direction")
    ap.add_argument("--seed", type=int, default=0, help="sample stream of --sampled (gt -> out; out -> gt takes seed + 1)")
    ap.add_argument("--tau", type=float, help="with --sampled: also the share of samples within this distance")
    ap.add_argument("--order", choices=tuple(capi.SAMPLE_ORDERS), default="face", help="row order of the samples")
    ap.add_argument("--align", choices=("rigid", "similarity"),
                    help="first move out onto gt by point-to-plane ICP (semigcn_amd.align; with 'similarity' also a uniform "
                         "scale) and org by the same matrix: for an out and org in another frame than gt")
    args = ap.parse_args(argv)
    gt, out = read_obj(args.gt), read_obj(args.out)
    org = read_obj(args.org) if args.org else None
    aligned = None
    if args.align:
        from . import align as _align             # imported here: that module imports this one
        aligned = _align.align(out, gt, with_scale=args.align == "similarity", seed=args.seed)
        out = (_align.apply(aligned.matrix, out[0]), out[1])
        if org is not None:
            org = (_align.apply(aligned.matrix, org[0]), org[1])
    if org is not None:
        r = mesh_distance(gt, org, out, real=args.real)
        res = {k: r[k] for k in ("hd_all", "hd_hole", "n_hole", "diag")}
    else:
        res = {"hd_all": simple_mesh_distance(gt, out)}
    if aligned is not None:
        res.update({"align_scale": aligned.scale, "align_iterations": aligned.iterations, "align_converged": aligned.converged})
    if args.sampled is not None:
        with Surface(gt) as gs, Surface(out) as os_:
            st = mesh_common.Stages(gs.device, True)
            r = surface_distance(gs, os_, n=args.sampled, seed=args.seed, tau=args.tau, order=args.order, stages=st)
            res.update({k: r[k] for k in ("hausdorff", "chamfer", "hausdorff_rel", "chamfer_rel")})
            for d in ("ab", "ba"):
                res.update({f"{k}_{d}": r[d][k] for k in ("max", "mean", "rms")})
                if args.tau is not None:
                    res[f"within_{d}"] = r[d]["within"]
            res["normal_consistency"] = r["normal_consistency"]
            res.update(mesh_common.Stages.record(st.result()))
    print(json.dumps({k: (None if isinstance(v, float) and math.isnan(v) else v) for k, v in res.items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
