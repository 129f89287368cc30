"""Simplify a mesh to a vertex budget on the device: quadric edge collapse.

Replaces the pooling hierarchy's simplifier, ``Mesh.simplification`` of the reference (util/mesh.py:394-482, SURVEY.md section
8(f)-4): the quadric error of the edge midpoint under the sum of the two ends' quadrics, times the valence penalty.  The
reference collapses one heap-ordered edge at a time and tests only the link condition; here a round collapses every edge that
is the cheapest of its neighbourhood, under the guards of ``remesh.collapse_short_edges`` (remesh.py, 2a.) and a vertex budget.
The construction below is this module's own and is the specification the tests pin (tests/simplify_oracle.py restates it in
numpy with serial, dictionary-based code).  The kernels are in csrc/mesh_remesh.hip and run on a ``RemeshPlan``: the edge
table, ranks, ``val``, border flags, ``hash``, the float64 normals and products and the stable compaction are those of
remesh.py and are not repeated here.  No epsilon anywhere; every float operation is a fixed sequence of multiplies, adds and
divisions (the file is built with ``-ffp-contract=off``); there are no float atomics.

**Input.**  As ``remesh``: ``(vs float32 [V, 3], faces int64 [F, 3])``, every edge with one face or with two that run it in
opposite directions; otherwise ``ValueError`` with the counts, and nothing is done.

**Quadrics.**  Once per call, on the mesh the call starts with (util/mesh.py:397-406 computes ``Q_s`` once).  Per face
``(a, b, c)``, in float64 from the float32 corners: ``n = (b - a) x (c - a)`` (differences, cross and dot product as in the
flip guard, summed left to right), ``nn = n . n``, ``d = -(n_x a_x + n_y a_y + n_z a_z)``, ``p = (n_x, n_y, n_z, d)``.
``K = p p^T / nn``: the ten entries ``K_ij = (p_i * p_j) / nn`` for ``i <= j``, in the order ``(xx, xy, xz, xw, yy, yz, yw, zz,
zw, ww)`` -- ten products, ten float64 divisions, no square root: the plane quadric of the unit normal without the root.  A
face with ``nn == 0`` contributes nothing.  ``Q[v]`` starts at 0 and receives ``Q[v] = Q[v] + K(f)`` for the faces ``f`` at
``v`` in ascending face index.  80 bytes per vertex; it is compacted with the vertices.

**A round** works on the mesh it starts with: edge table, ranks, ``val``, border flags, positions and ``Q``.  ``ring(v)`` is
the set of vertices that share an edge with ``v``; ``need = V_now - target_v``.

* *Eligible* is an edge ``{a, b}`` with exactly two faces, not both of whose ends are border vertices.  The kept vertex ``k``
  is the border end when there is one, and keeps its position ``P = vs[k]``; otherwise ``k = min(a, b)`` and moves to the
  float32 midpoint ``P = (vs[lo] + vs[hi]) * 0.5f`` per component, as the split forms it.  The removed vertex ``r`` is the other end.
* An eligible edge is *refused* when any of the following holds; it is counted (``refused``) and takes no part in the round.
  With ``c`` the third vertex of the face of the lower half-edge and ``d`` that of the other face: ``c == d``.  The faces at
  ``r`` or the faces at ``k`` are not one fan (all faces at the vertex reachable from one another through edges at the
  vertex: a vertex at which two fans touch is neither removed nor merged into).  *Link:* the vertices ``w != k`` of
  ``ring(r)`` with ``{k, w}`` an edge of the round's mesh are not exactly two (util/mesh.py:459-462).  *Valence floors* of
  2a.: ``val[c] - 1``, ``val[d] - 1`` or ``val_new = val[k] + val[r] - 4`` falls below 3 (2 for a border vertex).  *Fold-over
  guard:* a face at ``r`` without ``k``, rotated to read ``(r, x, y)``, or -- when ``k`` moves -- a face at ``k`` without
  ``r``, rotated to ``(k, x, y)``, does not have ``n_old . n_new > 0`` strictly, where ``n_old = (x - v) x (y - v)`` with
  ``v`` the position of ``r`` (of ``k``) and ``n_new = (x - P) x (y - P)``, float64 on the float32 coordinates.  The cost is
  not finite.
* *Cost*, float64: ``q_i = Q[k]_i + Q[r]_i`` for the ten entries; with ``(x, y, z) = P``,
  ``s0 = q_xx x + q_xy y + q_xz z + q_xw``, ``s1 = q_xy x + q_yy y + q_yz z + q_yw``, ``s2 = q_xz x + q_yz y + q_zz z + q_zw``,
  ``s3 = q_xw x + q_yw y + q_zw z + q_ww``, ``err = x s0 + y s1 + z s2 + s3``, each sum left to right.  ``pen = |val_new - 6| + 1``
  and ``pen = pen * 100000`` when ``val_new == 3`` (util/mesh.py:10-11, 470-478); ``cost = err * pen``; not finite: refused;
  then ``cost = cost > 0 ? cost : 0``.
* *Priority* of a legal (eligible, not refused) edge: ``(0xFFFFFFFF - bits(c32)) << 32 | hash(rank)`` with ``c32 =
  float32(cost)`` (round to nearest even), the float32 maximum when ``cost`` is above it.  ``hash`` is a bijection: no two
  edges tie, and edges whose costs agree after rounding to float32 are ordered by the hash alone.
* *Budget:* of the ``C`` legal edges only the ``A = min(need, C)`` of highest priority are *admitted*.  At most ``need`` bid,
  so at most ``need`` win: the stage lands on ``target_v`` exactly, never below, and never collapses an edge that is not
  among the ``need`` cheapest legal edges of the current mesh.
* The *footprint* of an edge is ``{k, r} + ring(k) + ring(r)`` -- both rings, because ``k`` moves.  An admitted edge is
  *selected* when no admitted edge whose footprint meets its own has a higher priority.  A collapse reads and writes only
  inside its footprint ("Simplification"), so footprint-disjoint winners are independent.  The best admitted
  edge always wins: a round with a legal edge makes progress.
* *Apply,* as 2a.: the two faces of the edge are deleted, every other face at ``r`` gets ``k`` in ``r``'s slot, ``r`` is
  deleted, survivors keep their relative order; plus ``vs[k] = P``, and with ``quadrics="sum"`` ``Q[k] = Q[k] + Q[r]``
  entry by entry.  With ``quadrics="own"``, the default, ``k`` keeps its own quadric, as the reference does
  (util/mesh.py:564-571 never updates ``Q_s``).
* Rounds repeat while ``V_now > target_v``; the stage stops early when a round selects nothing or after ``max_rounds``
  rounds, which is reported (``reached=False``), not raised.  ``counts`` holds ``(C, A, winners)`` of every round that
  collapsed something.  One host synchronisation per round reads the three; the cut is found by one radix sort of the
  64-bit priorities and stays in device memory.

**Result.**  ``Simplified``: ``vs``, ``faces``; ``vertex_ids`` int64 [V'], the input id of every survivor, ascending;
``coarse_of`` int64 [V], where every input vertex ended up (``coarse_of[vertex_ids]`` is the identity); ``counts``;
``reached``; ``report`` with V and F before and after, the largest cluster, the refused edges of the last round analysed and
``cluster_quadric_error``: the sum over the result's vertices of ``err`` at the vertex's position under the sum of the INPUT
quadrics of its cluster (a float64 reduction in torch: a figure for the report, not part of the rule; ``error_report=False``
leaves it and the largest cluster out).  Border vertices
never move and a border vertex is never removed, so on an open mesh the border survives bit for bit.  On a closed mesh the
kept vertex of every collapse is the smaller id, so the survivor of a cluster is its smallest member.

HIP device only: a CPU tensor raises ``SemigcnLibraryError``; the ``ValueError``s come before any device is asked for.

Command line::

    python -m semigcn_amd.simplify in.obj out.obj (--target-v N | --ratio R) [--levels L] [--quadrics own|sum] [--json]
    python -m semigcn_amd.simplify --torus NU NV (--target-v N | --ratio R) [--levels L] [--quadrics own|sum] [--json]

simplifies ``L`` times in a row (``--ratio`` applies to each level's own vertex count; ``--target-v`` needs ``--levels 1``)
and writes the last level.  Prints one line per level; with ``--json`` one JSON line with the levels' reports, rounds and
the device time ``simplify_ms`` of each.
"""
from __future__ import annotations

import argparse
import json
import sys
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import capi
from .capi import RemeshPlan
from .mesh_common import Stages, check_mesh, read_obj, vs_faces, write_obj

__all__ = ["simplify_mesh", "Simplified", "resolve_target"]


@dataclass
class Simplified:
    """What ``simplify_mesh`` returns."""
    vs: torch.Tensor            # float32 [V', 3]
    faces: torch.Tensor         # int64 [F', 3]
    vertex_ids: torch.Tensor    # int64 [V']: the input index of every vertex of the result, ascending
    coarse_of: torch.Tensor     # int64 [V]: the index in the result of the vertex every input vertex ended up in
    counts: List[Tuple[int, int, int]]   # per round: legal candidates, admitted, winners
    reached: bool               # V' == target_v
    report: dict
    stage_ms: Optional[dict] = None


def resolve_target(V: int, target_v=None, ratio=None) -> int:
    """The vertex budget from exactly one of ``target_v`` (0 <= target_v <= V) and ``ratio`` (0 < ratio <= 1:
    ``int(V * ratio)``, as ``MGCN.__init__`` forms it)."""
    if (target_v is None) == (ratio is None):
        raise ValueError("give exactly one of target_v and ratio")
    if ratio is not None:
        ratio = float(ratio)
        if not 0.0 < ratio <= 1.0:                                 # false for a NaN as well
            raise ValueError(f"ratio must lie in (0, 1], got {ratio}")
        return int(V * ratio)
    target_v = int(target_v)
    if target_v < 0 or target_v > V:
        raise ValueError(f"target_v must lie in [0, V = {V}], got {target_v}")
    return target_v


def _quadric_form(Q: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    x, y, z = (pos[:, i].double() for i in range(3))
    s0 = Q[:, 0] * x + Q[:, 1] * y + Q[:, 2] * z + Q[:, 3]
    s1 = Q[:, 1] * x + Q[:, 4] * y + Q[:, 5] * z + Q[:, 6]
    s2 = Q[:, 2] * x + Q[:, 5] * y + Q[:, 7] * z + Q[:, 8]
    s3 = Q[:, 3] * x + Q[:, 6] * y + Q[:, 8] * z + Q[:, 9]
    return x * s0 + y * s1 + z * s2 + s3


def _plan(vs: torch.Tensor, faces: torch.Tensor) -> RemeshPlan:
    plan = RemeshPlan(vs, faces)
    if not plan.valid:
        msg = (f"the mesh cannot be simplified: {plan.n_nonmanifold} edge(s) with three or more faces, {plan.n_misoriented} "
               f"edge(s) whose two faces run them in the same direction (smallest offending edge {plan.bad_edge}), "
               f"{plan.n_degenerate} face(s) with a repeated vertex (smallest {plan.bad_face}), {plan.n_nonfinite} "
               f"vertex/vertices with a non-finite coordinate (smallest {plan.bad_vertex})")
        plan.close()
        raise ValueError(msg)
    return plan


def simplify_mesh(vs, faces, target_v: Optional[int] = None, ratio: Optional[float] = None, quadrics: str = "own",
                  max_rounds: int = 256, timings: bool = False, error_report: bool = True) -> Simplified:
    """Simplify ``(vs, faces)`` to ``target_v`` vertices (or ``int(V * ratio)``) by quadric edge collapse (module docstring).
    ``quadrics``: ``"own"`` -- a kept vertex keeps its quadric, as the reference -- or ``"sum"``.  ``timings``: also measure
    the device time (``Simplified.stage_ms``; one more synchronisation).  ``error_report=False`` leaves ``largest_cluster`` and
    ``cluster_quadric_error`` out of the report and with them a copy of the input's quadrics and two reductions (what
    ``meshprep.DeviceMesh`` asks for: it keeps the maps only).  With it, the quadrics the report reads are the ones the stage
    then works on: they are computed once."""
    vs, faces = check_mesh((vs, faces))
    if quadrics not in RemeshPlan.QUADRICS:
        raise ValueError(f"quadrics must be 'own' or 'sum', got {quadrics!r}")
    max_rounds = int(max_rounds)
    if max_rounds < 0:
        raise ValueError(f"max_rounds must be >= 0, got {max_rounds}")
    V0 = int(vs.shape[0]) if hasattr(vs, "shape") else len(vs)
    target = resolve_target(V0, target_v, ratio)
    vs, faces = vs_faces(vs, faces)
    with capi._on_device(vs.device):
        st = Stages(vs.device, timings)
        with _plan(vs, faces) as plan:
            Q0 = plan.quadrics() if error_report else None          # the plan keeps them: simplify does not form them again
            st.mark("quadrics")
            counts, refused = plan.simplify(target, quadrics, max_rounds)
            out_vs, out_faces, _, _ = plan.export()
            vertex_ids, coarse_of = plan.collapse_maps()
            st.mark("simplify")
        Vc = int(out_vs.shape[0])
        report = {"n_vertices_in": V0, "n_faces_in": int(faces.shape[0]), "n_vertices": Vc, "n_faces": int(out_faces.shape[0]),
                  "target_v": target, "rounds": len(counts), "n_refused": refused}
        if error_report:
            Qc = torch.zeros((Vc, 10), dtype=torch.float64, device=vs.device).index_add_(0, coarse_of, Q0)
            report.update({"largest_cluster": int(torch.bincount(coarse_of, minlength=Vc).max()) if Vc else 0,
                           "cluster_quadric_error": float(_quadric_form(Qc, out_vs).sum()) if Vc else 0.0})
        st.mark("report")
        return Simplified(out_vs, out_faces, vertex_ids, coarse_of, counts, Vc == target, report, st.result())


def main(argv=None) -> int:
    from . import synth
    ap = argparse.ArgumentParser(prog="python -m semigcn_amd.simplify",
                                 description="simplify a triangle mesh to a vertex budget by quadric edge collapse (the "
                                             "pooling hierarchy of util/mesh.py:394-482)")
    ap.add_argument("input", nargs="?", help="the mesh to simplify (OBJ)")
    ap.add_argument("output", nargs="?", help="where the last level goes (OBJ)")
    ap.add_argument("--target-v", type=int, default=None, help="vertices to keep")
    ap.add_argument("--ratio", type=float, default=None, help="fraction of the vertices to keep, per level")
    ap.add_argument("--levels", type=int, default=1, help="simplify this many times in a row")
    ap.add_argument("--quadrics", choices=sorted(RemeshPlan.QUADRICS), default="own")
    ap.add_argument("--torus", type=int, nargs=2, metavar=("NU", "NV"), help="run on a synthetic torus instead of an OBJ")
    ap.add_argument("--json", action="store_true", help="print one JSON line instead of one line per level")
    args = ap.parse_args(argv)
    if (args.input is not None) + (args.torus is not None) != 1:
        ap.error("give either in.obj out.obj or --torus NU NV")
    if args.input is not None and args.output is None:
        ap.error("in.obj needs out.obj")
    if (args.target_v is None) == (args.ratio is None):
        ap.error("give exactly one of --target-v and --ratio")
    if args.levels < 1 or (args.target_v is not None and args.levels != 1):
        ap.error("--levels must be >= 1, and 1 with --target-v")
    if args.input is not None:
        vs, faces = read_obj(args.input)
    else:
        m = synth.torus_mesh(args.torus[0], args.torus[1], masks=False)
        vs, faces = m.vs.astype(np.float32), m.faces
    levels = []
    for _ in range(args.levels):
        out = simplify_mesh(vs, faces, target_v=args.target_v, ratio=args.ratio, quadrics=args.quadrics, timings=True)
        vs, faces = out.vs, out.faces
        rec = dict(out.report)
        rec.update({"reached": out.reached, "winners": [c[2] for c in out.counts]})
        rec.update(Stages.record(out.stage_ms))
        levels.append(rec)
        if not args.json:
            print(f"{rec['n_vertices_in']} -> {rec['n_vertices']} vertices ({rec['n_faces_in']} -> {rec['n_faces']} faces) in "
                  f"{rec['rounds']} rounds, reached={out.reached}, largest cluster {rec['largest_cluster']}, quadric error "
                  f"{rec['cluster_quadric_error']:.6g}, {rec['simplify_ms']:.3f} ms")
    if args.output:
        write_obj(args.output, vs, faces)
    if args.json:
        print(json.dumps({"quadrics": args.quadrics, "levels": levels}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
