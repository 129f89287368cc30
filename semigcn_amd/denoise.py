"""Denoise a mesh on the device: bilateral filtering of the face normals, then vertex updating.

The classical two-stage denoiser.  Stage one filters the face normals so that they are smooth inside a flat or curved
region and stay apart across a crease: ``functional.bilateral_normal_filter`` (``Models.bnf``, util/models.py:209-237;
csrc/mesh_bnf.hip).  Stage two moves the vertices so that the faces meet those normals: ``update_vertices``
(``Models.vertex_updating``, util/models.py:239-252, there a Python loop over every vertex and every step;
csrc/mesh_denoise.hip).  ``denoise_mesh`` alternates the two.  Measurement noise is what it is for: uniform Laplacian
smoothing (``prepare.laplacian_smooth``) rounds creases and shrinks the body, this keeps both.

  ============================  ==========================================================
  here                          reference
  ============================  ==========================================================
  ``update_vertices``           ``Models.vertex_updating(pos, norm, mesh, loop)``   util/models.py:239-252
  ``denoise_mesh``              ``Models.bnf`` followed by ``Models.vertex_updating``, repeated
  ============================  ==========================================================

The rule
--------
The kernel is DEFINED by this rule.  Everything is float32, every operation is rounded on its own (nothing is fused), and
the divisions are the correctly rounded ones.  One step, for all vertices at once from the positions ``p`` of the step
before (Jacobi):

* ``c_f = ((p_a + p_b) + p_c) / 3.0f`` per component, with ``a, b, c = faces[f]``.
* Vertex ``i`` has the incident faces ``f_1 < ... < f_k``: ascending face index, ``k`` = the number of faces that name ``i``.
* Start ``s = 0``.  For each incident face in that order:

  - ``d = c_f - p_i``
  - ``t = (n_x d_x + n_y d_y) + n_z d_z``      with ``n = normals[f]``
  - ``s = s + t n``

* ``p_i' = p_i + s / float(k)``.
* If ``k = 0``, or ``movable[i] == 0``, then ``p_i'`` is ``p_i`` bit for bit.  Such vertices still feed the centroids.
* The normals are used as given.  They are not normalised, and non-finite values propagate, as in the reference.

``steps`` steps apply this ``steps`` times; ``steps == 0`` copies.  Every vertex sums its own face list in a fixed order
(no atomics), so the result is bit-reproducible, and ``a`` steps followed by ``b`` steps equal ``a + b`` steps bit for bit.
tests/denoise_oracle.py restates the rule in numpy; the device equals it bit for bit.  The reference's own loop stays
within 3e-8 of it, relative to the largest coordinate (tests/golden/g8_vertex_update.npz).

The algebraically cheaper form ``sum n (n . c) - (sum n n^T) p_i`` is not used: it subtracts two large numbers for a mesh
far from the origin, and it is not the reference's formula.

HIP device only, like the rest of the package: a CPU tensor raises ``SemigcnLibraryError``.  No autograd through any of it.

Command line::

    python -m semigcn_amd.denoise IN.obj [-o OUT.obj] [--iterations N] [--normal-rounds N] [--sigma-s S] [--vertex-steps N]
                                  [--torus NU NV | --box N] [--noise SIGMA --seed K] [--repeat R]

prints one JSON line: the report and the stage times (``topology_ms``, ``plan_ms``, ``filter_ms``, ``update_ms``) of the
last repeat.  ``--noise SIGMA`` adds Gaussian noise of ``SIGMA`` mean edge lengths to the input first; with a synthetic
input the line also holds the mean angle between the face normals and the clean mesh's, before and after.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import math
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import capi
from .capi import SemigcnLibraryError, VertexUpdatePlan
from .mesh_common import Stages, check_mesh, device_tensor, read_obj, vs_faces, write_obj

__all__ = ["update_vertices", "denoise_mesh", "Denoised", "VertexUpdatePlan"]


def _count(value, name: str) -> int:
    value = int(value)
    if value < 0:
        raise ValueError(f"{name} must be >= 0, got {value}")
    return value


def _sizes(vs, faces):
    return int(vs.shape[0]) if hasattr(vs, "shape") else len(vs), int(faces.shape[0]) if hasattr(faces, "shape") else len(faces)


def _check_movable(movable, V: int):
    if movable is not None:
        n = movable.numel() if isinstance(movable, torch.Tensor) else np.asarray(movable).size
        if n != V:
            raise ValueError(f"movable must hold one entry per vertex ({V}), got {n}")


def _plan_for(plan, faces: torch.Tensor, V: int):
    """A context that gives a VertexUpdatePlan: the caller's own, left open, or one made here and closed."""
    if plan is None:
        return VertexUpdatePlan(faces, V)
    if not isinstance(plan, VertexUpdatePlan):
        raise TypeError(f"plan must be a VertexUpdatePlan, got {type(plan).__name__}")
    if (plan.num_vertices, plan.num_faces) != (V, faces.shape[0]):
        raise SemigcnLibraryError(f"plan of {plan.num_vertices} vertices and {plan.num_faces} faces, mesh has {V} and "
                                  f"{faces.shape[0]}")
    return contextlib.nullcontext(plan)


def update_vertices(vs, faces, normals, steps: int = 10, *, movable=None, plan: Optional[VertexUpdatePlan] = None) -> torch.Tensor:
    """``Models.vertex_updating(pos, norm, mesh, loop)`` (util/models.py:239-252): ``steps`` steps that move the vertices
    ``vs`` [V, 3] of the triangle list ``faces`` [F, 3] towards the face normals ``normals`` [F, 3], by the rule of the
    module docstring; returns float32 [V, 3] on the device.  ``movable`` bool [V]: False = the vertex stays.  ``plan``: a
    ``VertexUpdatePlan`` of the same faces, reused as it is (None: one is made here and closed).  No autograd."""
    vs, faces = check_mesh((vs, faces))
    steps = _count(steps, "steps")
    V, F = _sizes(vs, faces)
    shape = tuple(normals.shape) if hasattr(normals, "shape") else np.shape(normals)
    if shape != (F, 3):
        raise ValueError(f"normals must be [F, 3] = [{F}, 3], got {shape}")
    _check_movable(movable, V)
    p, f = vs_faces(vs, faces)
    n = device_tensor(normals, torch.float32, "normals").to(p.device)
    if movable is not None:
        movable = device_tensor(movable, torch.bool, "movable").to(p.device)
    with _plan_for(plan, f, V) as pl:
        return pl.run(p, n, movable, steps)


@dataclass
class Denoised:
    """What ``denoise_mesh`` returns."""
    vs: torch.Tensor                    # float32 [V, 3]
    normals: Optional[torch.Tensor]     # float32 [F, 3]: the last filtered normals (None with iterations == 0)
    report: dict
    stage_ms: Optional[dict] = None


def denoise_mesh(vs, faces, *, iterations: int = 1, normal_rounds: int = 5, sigma_s: float = 0.3, vertex_steps: int = 10,
                 movable=None, f2f=None, plan: Optional[VertexUpdatePlan] = None, timings: bool = False) -> Denoised:
    """``iterations`` times: ``normal_rounds`` rounds of the bilateral face-normal filter (``sigma_s`` as in
    ``functional.bilateral_normal_filter``), then ``vertex_steps`` steps of ``update_vertices`` towards the filtered normals.
    Each iteration is exactly ``functional.bilateral_normal_filter(p, faces, f2f, loop=normal_rounds, sigma_s=sigma_s)``
    followed by ``update_vertices(p, faces, that, vertex_steps, movable=movable)``, bit for bit.

    ``f2f`` int64 [F, 3] is the face ring (``meshprep.MeshTopology.f2f``; None: computed once here), ``plan`` a
    ``VertexUpdatePlan`` of the same faces.  The report holds ``n_vertices``, ``n_faces``, ``n_unused`` (vertices without a
    face), ``max_valence`` and, per iteration, ``normal_residual = sum |n_filtered - fn|_1 / F`` with ``fn`` the face normals
    going into the filter; the residuals are read with one synchronisation at the end.  ``timings``: also measure the
    device time of the stages (``Denoised.stage_ms``; one more synchronisation)."""
    vs, faces = check_mesh((vs, faces))
    iterations, normal_rounds = _count(iterations, "iterations"), _count(normal_rounds, "normal_rounds")
    vertex_steps = _count(vertex_steps, "vertex_steps")
    sigma_s = float(sigma_s)
    if not sigma_s > 0:                                           # false for a NaN as well
        raise ValueError(f"sigma_s must be > 0, got {sigma_s}")
    V, F = _sizes(vs, faces)
    if F == 0 and iterations > 0:
        raise ValueError("denoise_mesh: the mesh has no faces")
    _check_movable(movable, V)
    if f2f is not None:
        shape = tuple(f2f.shape) if hasattr(f2f, "shape") else np.shape(f2f)
        if shape != (F, 3):
            raise ValueError(f"f2f must be [F, 3] = [{F}, 3], got {shape}")
    p, f = vs_faces(vs, faces)
    if movable is not None:
        movable = device_tensor(movable, torch.bool, "movable").to(p.device)
    with capi._on_device(p.device):
        st = Stages(p.device, timings)
        if f2f is None:
            f2f = capi.mesh_edges(f, V, with_f2f=True)[1]
        else:
            f2f = device_tensor(f2f, torch.int64, "f2f").to(p.device)
        st.mark("topology")
        with _plan_for(plan, f, V) as pl:
            st.mark("plan")
            scratch = capi.bnf_scratch(F, p.device) if iterations else None
            normals, partials = None, []
            if iterations == 0:
                p = p.clone()
            for _ in range(iterations):
                _, normals, part = capi.bnf_filter(p, f, f2f, normal_rounds, sigma_s, with_partials=True, scratch=scratch)
                partials.append(part)
                st.mark("filter")
                p = pl.run(p, normals, movable, vertex_steps)
                st.mark("update")
            report = {"n_vertices": V, "n_faces": F, "n_unused": pl.num_unused, "max_valence": pl.max_valence,
                      "iterations": iterations, "normal_rounds": normal_rounds, "sigma_s": sigma_s, "vertex_steps": vertex_steps}
        residual = torch.stack([t.double().sum() for t in partials]).div(F).tolist() if partials else []
        report["normal_residual"] = residual
        return Denoised(p, normals, report, st.result())


def _mean_normal_angle(vs: torch.Tensor, clean: torch.Tensor, faces: torch.Tensor) -> float:
    """Mean angle in degrees between the face normals of two vertex arrays over the same faces (float64)."""
    def unit(v):
        v = v.double()
        n = torch.linalg.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]], dim=1)
        return n / n.norm(dim=1, keepdim=True).clamp_min(1e-300)
    return float(torch.rad2deg(torch.acos((unit(vs) * unit(clean)).sum(1).clamp(-1.0, 1.0))).mean())


def main(argv=None) -> int:
    from . import synth
    ap = argparse.ArgumentParser(prog="python -m semigcn_amd.denoise",
                                 description="denoise a triangle mesh: bilateral filtering of the face normals, then vertex "
                                             "updating (Models.bnf and Models.vertex_updating, util/models.py:209-252)")
    ap.add_argument("input", nargs="?", help="the mesh to denoise (OBJ)")
    ap.add_argument("-o", "--output", help="where the result goes (OBJ)")
    ap.add_argument("--iterations", type=int, default=1, help="filter-then-update iterations")
    ap.add_argument("--normal-rounds", type=int, default=5, help="rounds of the normal filter per iteration")
    ap.add_argument("--sigma-s", type=float, default=0.3, help="width of the filter's normal-difference weight")
    ap.add_argument("--vertex-steps", type=int, default=10, help="vertex-update steps per iteration")
    ap.add_argument("--torus", type=int, nargs=2, metavar=("NU", "NV"), help="run on a synthetic torus instead of an OBJ")
    ap.add_argument("--box", type=int, metavar="N", help="run on the unit box with an N x N grid per side instead of an OBJ")
    ap.add_argument("--noise", type=float, default=0.0, metavar="SIGMA", help="add Gaussian noise of SIGMA mean edge lengths first")
    ap.add_argument("--seed", type=int, default=7, help="seed of the noise")
    ap.add_argument("--repeat", type=int, default=1, help="run this many times and report the last")
    args = ap.parse_args(argv)
    if (args.input is not None) + (args.torus is not None) + (args.box is not None) != 1:
        ap.error("give exactly one of IN.obj, --torus NU NV and --box N")
    if min(args.iterations, args.normal_rounds, args.vertex_steps) < 0 or args.repeat < 1:
        ap.error("--iterations, --normal-rounds and --vertex-steps must be >= 0, --repeat >= 1")
    if not args.sigma_s > 0 or not args.noise >= 0 or math.isinf(args.noise):
        ap.error("--sigma-s must be > 0 and --noise >= 0")
    if args.input is not None:
        vs, faces = read_obj(args.input)
    elif args.box is not None:
        vs, faces = synth.box_mesh(args.box)
    else:
        m = synth.torus_mesh(args.torus[0], args.torus[1], jitter=0.0, masks=False)
        vs, faces = m.vs.astype(np.float32), m.faces
    clean = vs
    if args.noise > 0:
        e = synth.edges_from_faces(faces, vs.shape[0])
        v64 = vs.astype(np.float64)
        scale = float(np.linalg.norm(v64[e[:, 0]] - v64[e[:, 1]], axis=1).mean()) if len(e) else 1.0
        vs = (v64 + np.random.default_rng(args.seed).normal(0.0, args.noise * scale, v64.shape)).astype(np.float32)
    p, f = vs_faces(vs, faces)
    for _ in range(args.repeat):
        out = denoise_mesh(p, f, iterations=args.iterations, normal_rounds=args.normal_rounds, sigma_s=args.sigma_s,
                           vertex_steps=args.vertex_steps, timings=True)
    rec = dict(out.report)
    rec.update(Stages.record(out.stage_ms))
    if args.noise > 0 and args.input is None:
        c = device_tensor(clean, torch.float32, "clean")
        rec.update({"noise": args.noise, "seed": args.seed, "normal_angle_before_deg": round(_mean_normal_angle(p, c, f), 4),
                    "normal_angle_after_deg": round(_mean_normal_angle(out.vs, c, f), 4)})
    if args.output:
        write_obj(args.output, out.vs, f)
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
