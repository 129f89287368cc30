"""Align a mesh to another on the device: point-to-plane ICP, rigid or with a uniform scale.

Every scorer of the package (``evaluate.mesh_distance``, ``simple_mesh_distance``, ``surface_distance``,
``render.error_colors``) assumes that its meshes share one coordinate frame.  That holds when the ground truth went
through ``prepare.prepare_inputs`` together with the scan, and not when it is the CAD model of a scanned part, a ground
truth kept at its own scale and origin, or a result exported by another tool.  The reference leaves that step to MeshLab
by hand; ``align`` does it here: it finds the similarity that moves ``source`` onto ``target``, ``apply`` moves vertices by
it, ``inverse`` turns it round.

The rule
--------
The two kernels (csrc/mesh_align.hip) are DEFINED by this rule; tests/align_oracle.py restates it in numpy.  A pose is
``(M, t)``: ``M`` float64 [3, 3], ``t`` float64 [3]; the ``matrix`` is the 4 x 4 ``[[M, t], [0, 1]]``.  Everything below is
float64 with plain multiplies and adds in the written order (nothing is fused); square root and division are the correctly
rounded ones.

* **Transform.**  For a float32 point ``p``: ``x_r = ((M_r0 p_x + M_r1 p_y) + M_r2 p_z) + t_r``.  ``sg_align_transform``
  rounds ``x`` to float32 once; non-finite values propagate.
* **Correspondences.**  ``Surface.query`` of the target on the float32 ``x``: per point the closest point ``c``, the face
  it lies on and the unsigned distance ``d``, all float32 (the rules of ``semigcn_amd.evaluate``).
* **Row.**  From the unrounded ``x``: ``N = (B - A) x (C - A)`` of that face on the float32 vertices, each component
  ``u_y v_z - u_z v_y``; ``nn = (N_x^2 + N_y^2) + N_z^2``; ``n = N / sqrt(nn)``.  The row is *skipped* if there is no face
  (negative, or ``0x7fffffff``), ``x`` is not finite or ``nn == 0``; otherwise *rejected as far* if ``d > max_dist``;
  otherwise *used*: ``e = x - c``, ``r = (n_x e_x + n_y e_y) + n_z e_z`` and ``J = (x x n, n, n . x)``, seven entries, the
  last exactly 0 without ``with_scale``.  ``r + J . (omega, tau, sigma)`` is the residual after the small motion
  ``x -> (1 + sigma)(x + omega x x) + tau``, to first order.
* **Sums.**  Over the used rows: ``A_jk = sum J_j J_k`` (``j <= k``), ``g_j = sum J_j r``, ``sum r^2``, ``sum d^2``, and the
  three counts.  Block partials over fixed runs of consecutive rows, added in block order: no floating-point atomics, two
  runs give identical bytes.  The order is not that of ``math.fsum``: a sum is within ``(n_used + 16) 2^-52 sum |term|``
  of the exact one.
* **Step** (host, numpy float64).  With fewer used rows than unknowns (6, or 7 with scale), a non-finite sum, or an ``A``
  that ``numpy.linalg.cholesky`` refuses, the iteration stops with ``reason="degenerate"`` and the pose as it was.
  Otherwise ``A delta = -g``, ``delta = (omega, tau[, sigma])``; the rotation is the Cayley map of ``omega`` in closed form,
  ``k = omega / 2``, ``a = k . k``, ``R = ((1 - a) I + 2 k k^T + 2 [k]_x) / (1 + a)`` -- orthogonal for every ``omega``, no
  trigonometry --; ``s_d = 1 + sigma``; ``M <- s_d R M``, ``t <- s_d R t + tau``.
* **Stop.**  ``step = max(|omega|_inf, |sigma|, |tau|_inf / diag)`` with ``diag`` the diagonal of the target's vertex
  box; ``step <= tol`` ends the iteration with ``converged=True``.  ``max_iter`` iterations without that end it with
  ``converged=False`` and ``reason="max_iter"``: a report, not an error.  The query rounds the moved points to float32, so
  the step jitters around 1e-9 once the pose has settled: the default ``tol`` of 1e-6 is above that, a much smaller one
  is never met.

``init="centroid"`` starts from ``M = s I``, ``t = c_T - s c_S``: ``c`` the centroids and ``rho`` the RMS radii (float64)
of the source points and of the target's points of the same kind -- its samples with the same ``n`` and ``seed``, or its
vertices --, ``s = rho_T / rho_S`` with scale and 1 without.  That removes a shift and a scale of any size; a rotation
beyond the basin of the iteration (some tens of degrees) needs an ``init`` from elsewhere: there is no global search here.

The source should be the less complete of the two meshes (a scan onto its ground truth): a source point over a hole of
the target is pulled to the hole's rim.  ``max_dist`` leaves such points, and far clutter, out of the sums.

HIP device only, like the rest of the package: a CPU tensor raises ``SemigcnLibraryError``.  One small device-to-host copy
(40 doubles) per iteration; the device never waits on the host inside a kernel.

Command line::

    python -m semigcn_amd.align SRC.obj DST.obj [-o OUT.obj] [--scale] [--init centroid] [--max-dist D]
                                [--samples N | --vertices] [--seed K] [--max-iter N] [--tol T]
                                [--torus NU NV | --box N] [--perturb SEED]

prints one JSON line: ``matrix``, ``scale``, ``iterations``, ``converged``, ``reason``, ``rms`` and the stage times
(``sample_ms``, ``transform_ms``, ``query_ms``, ``accumulate_ms``); ``-o`` writes the moved source.  With ``--torus`` or
``--box`` the target is that mesh and the source the same mesh, with ``--perturb SEED`` under ``random_similarity(SEED)``;
the line then also holds ``matrix_error``, the largest entry of ``matrix @ perturbation - I``.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import math
import sys
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import capi, mesh_common
from .capi import SemigcnLibraryError
from .evaluate import Surface, sample_surface
from .mesh_common import Stages, check_mesh, read_obj, write_obj

__all__ = ["align", "apply", "inverse", "Alignment", "cayley", "similarity", "random_similarity"]

POINTS = ("samples", "vertices")


class Alignment(NamedTuple):
    """What ``align`` returns: ``matrix`` moves the source onto the target."""
    matrix: np.ndarray            # float64 [4, 4]
    scale: float                  # cbrt(det M)
    rotation: np.ndarray          # M / scale, float64 [3, 3]
    translation: np.ndarray       # float64 [3]
    iterations: int
    converged: bool
    reason: str                   # "converged", "max_iter" or "degenerate"
    rms: float                    # the last sqrt(sum d^2 / n_used); nan before the first iteration
    history: list                 # per iteration: rms, n_used, n_far, n_skipped, step (nan for a degenerate one)
    stage_ms: Optional[dict]      # with timings=True: device time per stage


def cayley(omega) -> np.ndarray:
    """The rotation ``((1 - a) I + 2 k k^T + 2 [k]_x) / (1 + a)``, ``k = omega / 2``, ``a = k . k`` (float64 [3, 3])."""
    k = np.asarray(omega, np.float64).reshape(3) / 2.0
    a = float(k @ k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return ((1.0 - a) * np.eye(3) + 2.0 * np.outer(k, k) + 2.0 * K) / (1.0 + a)


def similarity(omega=(0.0, 0.0, 0.0), scale: float = 1.0, translation=(0.0, 0.0, 0.0)) -> np.ndarray:
    """The 4 x 4 matrix of ``x -> scale * cayley(omega) x + translation``."""
    m = np.eye(4)
    m[:3, :3] = float(scale) * cayley(omega)
    m[:3, 3] = np.asarray(translation, np.float64).reshape(3)
    return m


def random_similarity(seed: int, with_scale: bool = True, extent: float = 1.0) -> np.ndarray:
    """A seeded perturbation inside the basin of the iteration: ``|omega_i| <= 0.1``, ``|scale - 1| <= 0.08`` (1 without
    ``with_scale``), ``|t_i| <= 0.05 extent`` (``extent``: the size of the mesh it is meant for)."""
    rng = np.random.default_rng(int(seed))
    omega, ds, t = rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.08, 0.08), rng.uniform(-0.05, 0.05, 3) * float(extent)
    return similarity(omega, 1.0 + ds if with_scale else 1.0, t)


def _matrix(matrix, name: str = "matrix") -> np.ndarray:
    m = np.array(matrix.detach().cpu().numpy() if isinstance(matrix, torch.Tensor) else matrix, dtype=np.float64)
    if m.shape != (4, 4):
        raise ValueError(f"{name} must be a 4 x 4 matrix, got shape {m.shape}")
    return m


def inverse(matrix) -> np.ndarray:
    """The 4 x 4 matrix that undoes ``matrix`` (host, float64)."""
    m = _matrix(matrix)
    Mi = np.linalg.inv(m[:3, :3])
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = Mi, -Mi @ m[:3, 3]
    return out


def apply(matrix, vs) -> torch.Tensor:
    """float32 [V, 3] on the device: the vertices ``vs`` (an array, a tensor or a mesh) under ``matrix``, by the transform of
    the rule (``sg_align_transform``)."""
    m = _matrix(matrix)
    x = getattr(vs, "vs", vs)
    shape = tuple(x.shape) if hasattr(x, "shape") else np.shape(x)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"vs must be [V, 3], got {shape}")
    return capi.align_transform(mesh_common.points(vs), m)


def _host_step(out, M, t, with_scale: bool, diag: float):
    """(M', t', step) from the 40 sums, or None: the step of the rule."""
    k = 7 if with_scale else 6
    if int(out[37]) < k or not np.isfinite(out[:35]).all():
        return None
    A = np.zeros((7, 7))
    A[np.triu_indices(7)] = out[:28]
    A = (A + np.triu(A, 1).T)[:k, :k]
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    delta = np.linalg.solve(L.T, np.linalg.solve(L, -out[28:28 + k]))
    if not np.isfinite(delta).all():
        return None
    omega, tau, sigma = delta[:3], delta[3:6], float(delta[6]) if with_scale else 0.0
    R, s_d = cayley(omega), 1.0 + sigma
    step = max(float(np.abs(omega).max()), abs(sigma), float(np.abs(tau).max()) / diag if diag else float(np.abs(tau).max()))
    return s_d * (R @ M), s_d * (R @ t) + tau, step


def _centroid_radius(p: torch.Tensor):
    p = p.to(torch.float64)
    c = p.mean(0)
    return c, ((p - c) ** 2).sum(1).mean().sqrt()


def _result(M, t, history, converged, reason, rms, stage_ms) -> Alignment:
    matrix = np.eye(4)
    matrix[:3, :3], matrix[:3, 3] = M, t
    scale = float(np.cbrt(np.linalg.det(M)))
    rotation = M / scale if scale else np.full((3, 3), np.nan)
    return Alignment(matrix, scale, rotation, np.array(t, np.float64), len(history), converged, reason, rms, history, stage_ms)


def align(source, target, *, points: str = "samples", n: int = 100000, seed: int = 0, with_scale: bool = False, init=None,
          max_dist: Optional[float] = None, max_iter: int = 50, tol: float = 1e-6, timings: bool = False) -> Alignment:
    """The similarity that moves ``source`` onto ``target`` by the rule of the module docstring.

    ``source``: a mesh; its points are ``sample_surface(source, n, seed)`` (``points="samples"``, drawn once) or its
    vertices (``"vertices"``).  ``target``: a ``Surface``, a mesh or a ``(vs, faces)`` pair.  ``with_scale``: also a uniform
    scale (7 unknowns instead of 6).  ``init``: None (the identity), a 4 x 4 matrix, or ``"centroid"``.  ``max_dist``: leave
    out the points farther than this from the target, counted in ``n_far``.  ``max_iter=0`` returns ``init``.  Two calls give
    identical bytes in ``matrix`` and ``history``."""
    if points not in POINTS:
        raise ValueError(f"points must be one of {POINTS}, got {points!r}")
    n, max_iter, tol = int(n), int(max_iter), float(tol)
    if n <= 0:
        raise ValueError(f"n must be > 0, got {n}")
    if max_iter < 0:
        raise ValueError(f"max_iter must be >= 0, got {max_iter}")
    if not tol > 0.0:
        raise ValueError(f"tol must be > 0, got {tol}")
    md = math.inf if max_dist is None else float(max_dist)
    if not md >= 0.0:
        raise ValueError(f"max_dist must be >= 0 or None, got {max_dist}")
    if isinstance(init, str):
        if init != "centroid":
            raise ValueError(f"init must be None, a 4 x 4 matrix or 'centroid', got {init!r}")
    elif init is not None:
        init = _matrix(init, "init")
    check_mesh(source)
    if not isinstance(target, Surface):
        check_mesh(target)

    with contextlib.ExitStack() as stack:
        ts = target if isinstance(target, Surface) else stack.enter_context(Surface(target))
        dev = ts.device
        st = Stages(dev, bool(timings))
        if points == "samples":
            pts = sample_surface(source, n, seed).points
        else:
            pts = mesh_common.points(source[0] if isinstance(source, (tuple, list)) else source)
        if pts.device != dev:
            raise SemigcnLibraryError(f"source on {pts.device}, target on {dev}")
        pts = pts.contiguous()
        box = ts.vs.to(torch.float64)
        ext = box.amax(0) - box.amin(0)
        scalars = [(ext * ext).sum().sqrt().reshape(1)]
        if isinstance(init, str):
            tp = sample_surface((ts.vs, ts.faces), n, seed).points if points == "samples" else ts.vs
            (cS, rS), (cT, rT) = _centroid_radius(pts), _centroid_radius(tp)
            scalars += [cS, cT, rS.reshape(1), rT.reshape(1)]
        st.mark("sample")
        host = torch.cat(scalars).tolist()                   # one synchronisation before the loop
        diag = host[0]
        M, t = np.eye(3), np.zeros(3)
        if isinstance(init, str):
            cS, cT, rS, rT = np.array(host[1:4]), np.array(host[4:7]), host[7], host[8]
            s = rT / rS if with_scale else 1.0
            M, t = s * np.eye(3), cT - s * cS
        elif init is not None:
            M, t = init[:3, :3].copy(), init[:3, 3].copy()

        moved = torch.empty_like(pts)
        scratch = torch.empty(capi.ALIGN_SUMS * capi.REDUCE_BLOCKS, dtype=torch.float64, device=dev)
        history, converged, reason, rms = [], False, "max_iter", float("nan")
        for _ in range(max_iter):
            pose = np.concatenate([M.reshape(-1), t])
            st.mark(None)
            capi.align_transform(pts, pose, out=moved)
            st.mark("transform")
            dist, face, closest = ts.query(moved, signed=False)
            st.mark("query")
            sums = capi.align_accumulate(ts.vs, ts.faces, pts, pose, closest, face, dist, md, with_scale, scratch)
            st.mark("accumulate")
            out = np.array(sums.tolist())                    # the iteration's one device-to-host copy
            n_used = int(out[37])
            rms = math.sqrt(out[36] / n_used) if n_used else float("nan")
            rec = {"rms": rms, "n_used": n_used, "n_far": int(out[38]), "n_skipped": int(out[39]), "step": float("nan")}
            history.append(rec)
            res = _host_step(out, M, t, with_scale, diag)
            if res is None:
                reason = "degenerate"
                break
            M, t, rec["step"] = res
            if rec["step"] <= tol:
                converged, reason = True, "converged"
                break
        return _result(M, t, history, converged, reason, rms, st.result())


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m semigcn_amd.align",
                                 description="move SRC onto DST by point-to-plane ICP, rigid or with a uniform scale")
    ap.add_argument("source", nargs="?", help="the mesh to move (OBJ): the less complete of the two")
    ap.add_argument("target", nargs="?", help="the mesh to move it onto (OBJ)")
    ap.add_argument("-o", "--output", help="where the moved source goes (OBJ)")
    ap.add_argument("--scale", action="store_true", help="also find a uniform scale")
    ap.add_argument("--init", choices=("centroid",), help="start from matched centroids (and RMS radii with --scale)")
    ap.add_argument("--max-dist", type=float, metavar="D", help="leave out source points farther than D from the target")
    ap.add_argument("--samples", type=int, metavar="N", help="N area-weighted samples of the source (default: 100000)")
    ap.add_argument("--vertices", action="store_true", help="the source's vertices instead of samples")
    ap.add_argument("--seed", type=int, default=0, help="sample stream")
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--torus", type=int, nargs=2, metavar=("NU", "NV"), help="a synthetic torus as source and target")
    ap.add_argument("--box", type=int, metavar="N", help="the unit box with an N x N grid per side as source and target")
    ap.add_argument("--perturb", type=int, metavar="SEED", help="with --torus / --box: move the source by random_similarity(SEED)")
    args = ap.parse_args(argv)
    synthetic = args.torus is not None or args.box is not None
    if args.torus is not None and args.box is not None:
        ap.error("give one of --torus NU NV and --box N")
    if synthetic == (args.source is not None) or (not synthetic and args.target is None):
        ap.error("give SRC.obj and DST.obj, or one of --torus NU NV and --box N")
    if args.samples is not None and args.vertices:
        ap.error("give one of --samples N and --vertices")
    if args.perturb is not None and not synthetic:
        ap.error("--perturb needs --torus or --box")
    truth = None
    if synthetic:
        from . import synth
        if args.box is not None:
            vs, faces = synth.box_mesh(args.box)
        else:
            m = synth.torus_mesh(args.torus[0], args.torus[1], masks=False)
            vs, faces = m.vs.astype(np.float32), m.faces
        dst = (vs, faces)
        src_vs = vs
        if args.perturb is not None:
            v64 = vs.astype(np.float64)
            truth = random_similarity(args.perturb, args.scale, float(np.linalg.norm(v64.max(0) - v64.min(0))))
            src_vs = (v64 @ truth[:3, :3].T + truth[:3, 3]).astype(np.float32)
        src = (src_vs, faces)
    else:
        src, dst = read_obj(args.source), read_obj(args.target)
    a = align(src, dst, points="vertices" if args.vertices else "samples", n=100000 if args.samples is None else args.samples,
              seed=args.seed, with_scale=args.scale, init=args.init, max_dist=args.max_dist, max_iter=args.max_iter,
              tol=args.tol, timings=True)
    res = {"matrix": a.matrix.tolist(), "scale": a.scale, "iterations": a.iterations, "converged": a.converged,
           "reason": a.reason, "rms": a.rms}
    if truth is not None:
        res["matrix_error"] = float(np.abs(a.matrix @ truth - np.eye(4)).max())
    res.update(Stages.record(a.stage_ms))
    if args.output:
        write_obj(args.output, apply(a.matrix, src[0]), src[1])
    print(json.dumps({k: (None if isinstance(v, float) and math.isnan(v) else v) for k, v in res.items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
