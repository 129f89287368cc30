"""Close the holes of a scan on the device: boundary loops, one ring patch per loop, fairing of the inserted vertices.

Replaces the hole-closing part of ``MeshFix.repair()`` in the reference's preprocess/prepare.py:28-33 -- the step that
creates the vertices the network exists to place.  Keeping the largest component, which MeshFix does first, is
``components.keep_components``; removing self-intersecting triangles, which it does last, is
``repair.remove_self_intersections``.  The isotropic remesh of the whole surface that follows
(preprocess/prepare.py:35-42) is ``remesh.refine_mesh`` (``collapse=True`` for its edge collapse, ``feature_angle=30`` for
MeshLab's crease angle: sharp edges and corners of a ``-CAD`` input are kept).  MeshFix is
not available to compare against; the construction below is this module's own and is the specification the tests pin
(tests/holes_oracle.py restates it in numpy / float64).  The kernels are csrc/mesh_fill.hip; the fairing is
``prepare.laplacian_smooth`` (csrc/mesh_smooth.hip) with only the inserted vertices movable, or with
``fair="thin_plate"`` the solve of "Thin-plate fairing" below (csrc/mesh_fair.hip).

**Boundary.**  A directed half-edge ``(a, b)`` of a face (``(f0, f1)``, ``(f1, f2)``, ``(f2, f0)``) whose opposite
``(b, a)`` belongs to no face is a boundary half-edge.  The boundary is *unorderable*, and ``ValueError`` is raised, when
a directed half-edge occurs more than once or a vertex has more than one outgoing boundary half-edge (a "bow-tie").

**Loops.**  Otherwise ``next[b] = a`` is a permutation of the boundary vertices; its cycles are the loops.  Canonical
form: loops are numbered by ascending smallest vertex, each starts at its smallest vertex, and each runs AGAINST the
mesh's boundary half-edges (the mesh has ``(a, b)``: the loop lists ``b`` then ``a``), so that a patch face
``(loop[i], loop[i + 1], x)`` is oriented like the mesh.  ``ptr`` int64 [L + 1] and ``verts`` int64 [sum n] hold them.

**Patch of a loop of n edges** -- topology in integer arithmetic only (``/`` below is floor division):

* ``n = 3``: the one face ``(loop[0], loop[1], loop[2])``, no new vertex.
* otherwise ``R = max(1, (113 n + 355) / 710)`` rings (``n / 2 pi`` rounded: the rings are about one border edge apart
  on a round hole).  Ring 0 is the loop; ring ``r``, ``0 < r < R``, has ``n_r = max(3, (2 n (R - r) + R) / (2 R))``
  vertices (``n (R - r) / R`` rounded); ring ``R`` is one vertex.
* Vertex ``j`` of ring ``r < R`` is ``B(s) + (r / R) (c - B(s))`` with ``s = j / n_r * perimeter``: ``B`` is the loop's
  closed polyline parameterised by arc length from ``loop[0]`` (float64 segment lengths and prefix sums in loop order,
  ``B(s)`` on the segment ``i`` with ``cum[i] <= s < cum[i + 1]``), ``c`` the mean of the loop's vertices.  Ring ``R`` is
  ``c``.  Computed in float64 from the float32 positions and rounded to float32 once.
* The strip between ring ``r`` (``m`` vertices ``o``) and ring ``r + 1`` (``k > 1`` vertices ``i``) has ``m + k``
  faces; with ``A = t m / (m + k)``, ``A' = (t + 1) m / (m + k)`` and ``B = t - A``, face ``t`` is
  ``(o[A % m], o[(A + 1) % m], i[B % k])`` when ``A' > A`` (the outer ring advances) and
  ``(o[A % m], i[(B + 1) % k], i[B % k])`` otherwise.  The last strip is the fan ``(o[t], o[(t + 1) % m], centre)``.
* New vertices and faces follow the originals in loop order, then ring order, then index order.

On a regular planar n-gon of edge length h (n = 4 ... 333) the unfaired patch is a closed disc with edges between
0.707 h and 2.236 h.  An irregular loop can give much longer edges (25 h at a 30 % radial wobble, n = 1000), which is why
the inserted vertices are faired by default.  The patch is the network's starting point, not a minimal surface: the
default fairing pulls it towards a membrane, flat across the hole and creased at the border; ``fair="thin_plate"`` makes it
leave the border along the scan's tangent instead (a cap cut from a sphere comes back round, not as a dent).

**Thin-plate fairing** (``fair_thin_plate``; tests/fair_oracle.py restates it in numpy / float64).  On a mesh
``(vs, faces)`` with a bool mask ``free`` [V]:

* Graph: the unique undirected edges of ``faces``; ``N(i)`` the distinct neighbours of ``i``, ``d_i = |N(i)|``;
  ``(Lx)_i = x_i - (1 / d_i) sum_{j in N(i)} x_j``.
* Rows ``S = free u N(free)``; energy ``E(x) = sum_{i in S} ||(Lx)_i||^2``; the unknowns are ``x_free``, every other
  vertex is fixed at its float32 input position.  Because a row reaches one ring past the patch into the scan, the
  minimiser continues the scan's tangent across the border.
* With ``M`` the rows ``S`` of ``L``: ``A x_free = b``, ``A = M_free^T M_free``, ``b = -M_free^T M_fixed x_fixed``; the
  three coordinates are three right-hand sides.  ``A`` is SPD exactly when every connected class of free vertices (under
  free-free edges) has an edge to a fixed vertex; this is checked on the device by union-find before any solve, and
  ``ValueError`` names the smallest vertex of an offending class.  A free vertex without edges is an error too.  The
  patches of ``fill_holes`` always satisfy the condition.
* Solver: conjugate gradients with the Jacobi preconditioner ``diag(A)_i = 1 + sum_{j in N(i)} 1 / d_j^2``, entirely in
  float64, from ``x0`` = the input positions (for ``fill_holes``: the raw construction).  ``||b||^2`` comes from
  ``M^T M`` applied to the positions with the free ones taken as 0, the first residual ``r0 = -M^T M x`` from all
  positions.  Each coordinate has its own ``alpha``, ``beta`` and stop test on the recursive residual,
  ``||r||^2 <= tol^2 ||b||^2``.  A coordinate with ``b.b = 0`` -- every fixed vertex its rows reach has that coordinate
  exactly 0 -- is measured against its first residual instead, ``||r||^2 <= tol^2 ||r0||^2``, and its
  ``relative_residual`` is ``||r|| / ||r0||``; with ``r0 = 0`` too it stops at once and reports 0.  A coordinate with
  ``b.b > 0`` is tested against ``tol^2 ||b||^2`` exactly.  A coordinate that has met its test is frozen -- its
  ``alpha`` and ``beta`` are 0 from then on -- so the result does not depend on how often the host looks.
  The solve ends when all three are frozen or after ``max_iter`` iterations: a cap that is reported
  (``converged = False``), not an error.  The result is rounded to float32 once; fixed vertices are copied bit for bit.
* Arithmetic: ``A p`` is two gathers, ``y_i = p_i - (1 / d_i) s_i`` over ``S`` with ``s_i`` the sum of the free ``p_j``,
  ``j in N(i)``, and ``q_i = y_i - sum_{j in N(i)} y_j (1 / d_j)`` over the free ``i``; ``1 / d`` is the rounded float64
  reciprocal, neighbour sums run in ascending neighbour order, every product and sum rounds on its own (no fused
  multiply-add).  Dot products are fixed-size block partials in index order, added up in a fixed order; no
  floating-point atomics: two runs give identical bytes.

Inputs are what ``evaluate`` accepts; HIP device only: a CPU tensor raises ``SemigcnLibraryError``.

Command line::

    python -m semigcn_amd.holes --scan A.obj --out A_filled.obj [--max-hole-edges N] [--fair-steps K] [--largest-component]
                                [--fair laplacian|thin-plate]
    python -m semigcn_amd.holes --torus NU NV --cut K [--out A_filled.obj] [--fair laplacian|thin-plate]

prints one JSON line with ``n_loops``, ``n_filled``, ``n_inserted_vertices``, ``n_inserted_faces`` and the device time of
each stage (``loops_ms``, ``emit_ms``, ``fair_ms``) and, when ``--fair`` is given, the fairing (``fair``) and the
``fair_iterations`` and ``fair_converged`` of the thin-plate solve (``null`` for the smoothing).  ``--torus NU NV --cut K`` runs on ``synth.torus_mesh(NU, NV)``
with K discs removed, sized as ``synth.make_v_mask`` sizes its holes (5 % of the vertices in all).
``--largest-component`` first runs ``components.keep_components(..., keep="largest")`` and adds ``n_components`` and
``n_dropped_faces`` to the line.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import capi, prepare
from .capi import FairPlan, FillPlan, SemigcnLibraryError
from .mesh_common import Stages, check_mesh, device_tensor, read_obj, vs_faces, write_obj

__all__ = ["boundary_loops", "fill_holes", "fair_thin_plate", "BoundaryLoops", "Filled", "FillPlan", "FairPlan"]

FAIR = ("laplacian", "thin_plate")


@dataclass
class BoundaryLoops:
    """The boundary loops of a mesh in canonical form (module docstring), on the device."""
    ptr: torch.Tensor          # int64 [L + 1]
    verts: torch.Tensor        # int64 [sum n]
    sizes: torch.Tensor        # int64 [L], edges (= vertices) per loop

    def __len__(self) -> int:
        return int(self.sizes.shape[0])


@dataclass
class Filled:
    """What ``fill_holes`` returns.  The original vertices and faces are the prefix of ``vs`` / ``faces``, bit-identical."""
    vs: torch.Tensor                  # float32 [V + Vn, 3]
    faces: torch.Tensor               # int64 [F + Fn, 3]
    num_original_vertices: int
    num_original_faces: int
    inserted: torch.Tensor            # bool [V + Vn], True = a vertex of a patch
    loops: BoundaryLoops
    filled: torch.Tensor              # bool [L], False = left open (more than max_hole_edges edges)
    stage_ms: Optional[dict] = None   # device time of the stages, when asked for
    fair_info: Optional[dict] = None  # fair="thin_plate": what fair_thin_plate reports about its solve


def _plan(faces: torch.Tensor, num_vertices: int) -> FillPlan:
    plan = FillPlan(faces, int(num_vertices))
    if not plan.orderable:
        msg = (f"the boundary cannot be ordered into loops: {plan.n_repeated} directed half-edge(s) occur more than once, "
               f"{plan.n_bowtie} vertex/vertices have more than one outgoing boundary half-edge; smallest offending "
               f"vertex {plan.bad_vertex}")
        plan.close()
        raise ValueError(msg)
    return plan


def _loops_of(plan: FillPlan) -> BoundaryLoops:
    ptr, verts = plan.loops()
    return BoundaryLoops(ptr, verts, ptr[1:] - ptr[:-1])


def boundary_loops(faces, num_vertices: int) -> BoundaryLoops:
    """The boundary loops of the triangle list ``faces`` [F, 3] over ``num_vertices`` vertices.  ``ValueError`` when the
    boundary is unorderable; the message names the number of repeated directed half-edges, the number of vertices with
    more than one outgoing boundary half-edge and the smallest offending vertex."""
    f = device_tensor(faces, torch.int64, "faces").reshape(-1, 3)
    with _plan(f, num_vertices) as plan:
        return _loops_of(plan)


def _solver_args(who: str, tol, max_iter, check_every=1):
    tol, max_iter, check_every = float(tol), int(max_iter), int(check_every)
    if not (tol >= 0.0 and math.isfinite(tol)):
        raise ValueError(f"{who}: tol must be finite and >= 0, got {tol}")
    if max_iter < 0:
        raise ValueError(f"{who}: max_iter must be >= 0, got {max_iter}")
    if check_every < 1:
        raise ValueError(f"{who}: check_every must be >= 1, got {check_every}")
    return tol, max_iter, check_every


def _solve_thin_plate(vs, faces, free, tol, max_iter, check_every):
    with FairPlan(faces, vs.shape[0], free) as plan:
        if plan.bad_kind == 1:
            raise ValueError(f"fair_thin_plate: free vertex {plan.bad_vertex} has no edges")
        if plan.bad_kind:
            raise ValueError("fair_thin_plate: the system is singular: a connected class of free vertices has no edge to a "
                             f"fixed vertex; its smallest vertex is {plan.bad_vertex}")
        return plan.solve(vs, tol, max_iter, check_every)


def fair_thin_plate(vs, faces, free, tol: float = 1e-10, max_iter: int = 10000, check_every: int = 32,
                    return_info: bool = False):
    """float32 [V, 3]: ``vs`` with the vertices ``free`` bool [V] at the minimiser of the thin-plate energy of the module
    docstring and every other vertex bit for bit; any mesh, any mask.  ``return_info``: also a dict with ``iterations``,
    the per-coordinate ``relative_residual`` (``||r|| / ||b||``; ``||r|| / ||r0||`` where ``b = 0``), ``converged`` and ``n_free``.  ``max_iter`` is a cap that
    is reported (``converged`` False), not an error; the host looks at the device's stop flag every ``check_every``
    iterations, which does not change the result.  An empty ``free`` returns a copy.  ``ValueError`` for a mask of the
    wrong length and for a singular system (it names the vertex)."""
    tol, max_iter, check_every = _solver_args("fair_thin_plate", tol, max_iter, check_every)
    vs, faces = check_mesh(vs, faces)
    n_free = int(free.numel()) if isinstance(free, torch.Tensor) else int(np.size(free))
    if n_free != int(vs.shape[0]):
        raise ValueError(f"fair_thin_plate: free must hold one entry per vertex ({int(vs.shape[0])}), got {n_free}")
    vs, faces = vs_faces(vs, faces)
    free = device_tensor(free, torch.bool, "free").reshape(-1).to(vs.device)
    with capi._on_device(vs.device):
        out, info = _solve_thin_plate(vs, faces, free, tol, max_iter, check_every)
    return (out, info) if return_info else out


def fill_holes(mesh, max_hole_edges: Optional[int] = None, fair_steps: int = prepare.SMOOTH_ITER,
               timings: bool = False, fair: str = "laplacian", fair_tol: float = 1e-10,
               fair_max_iter: int = 10000) -> Filled:
    """Close every boundary loop of ``mesh`` with at most ``max_hole_edges`` edges (``None``: every loop, as
    ``MeshFix.repair()`` does; a cap leaves e.g. the outer border of an open scan open) by the patch of the module
    docstring, then run ``fair_steps`` steps of ``prepare.laplacian_smooth`` with only the inserted vertices movable
    (``0``: the raw construction).  ``ValueError`` when the boundary is unorderable; nothing is partially filled.
    ``(Filled.vs, Filled.faces)`` is a valid ``initial`` for ``prepare.prepare_inputs``.  ``timings``: also measure the
    device time of the stages (``Filled.stage_ms``; one more synchronisation).  ``fair="thin_plate"``: fair by
    ``fair_thin_plate(..., tol=fair_tol, max_iter=fair_max_iter)`` instead; ``fair_steps`` is then ignored, except that 0
    still means the raw construction, and ``Filled.fair_info`` holds what the solve reports."""
    if fair not in FAIR:
        raise ValueError(f"fill_holes: fair must be one of {FAIR}, got {fair!r}")
    fair_tol, fair_max_iter, _ = _solver_args("fill_holes", fair_tol, fair_max_iter)
    fair_steps = int(fair_steps)
    if fair_steps < 0:
        raise ValueError(f"fill_holes: fair_steps must be >= 0, got {fair_steps}")
    if max_hole_edges is not None and int(max_hole_edges) < 0:
        raise ValueError(f"fill_holes: max_hole_edges must be >= 0 or None, got {max_hole_edges}")
    vs, faces = vs_faces(mesh)
    V, F = vs.shape[0], faces.shape[0]
    with capi._on_device(vs.device):
        st = Stages(vs.device, timings)
        with _plan(faces, V) as plan:
            loops = _loops_of(plan)
            st.mark("loops")
            Vn, Fn = plan.plan(max_hole_edges)
            out_vs = torch.empty((V + Vn, 3), dtype=torch.float32, device=vs.device)
            out_faces = torch.empty((F + Fn, 3), dtype=torch.int64, device=vs.device)
            out_vs[:V].copy_(vs)
            out_faces[:F].copy_(faces)
            filled = plan.emit(vs, out_vs[V:], out_faces[F:])
            st.mark("emit")
        inserted = torch.zeros(V + Vn, dtype=torch.bool, device=vs.device)
        inserted[V:] = True
        info = None
        if fair_steps > 0 and Vn > 0 and fair == "laplacian":
            out_vs = prepare.laplacian_smooth(out_vs, out_faces, steps=fair_steps, movable=inserted)
        elif fair_steps > 0 and fair == "thin_plate":
            out_vs, info = _solve_thin_plate(out_vs, out_faces, inserted, fair_tol, fair_max_iter, 32) if Vn > 0 else (
                out_vs, {"iterations": 0, "relative_residual": [0.0, 0.0, 0.0], "converged": True, "n_free": 0})
        st.mark("fair")
        return Filled(out_vs, out_faces, V, F, inserted, loops, filled, st.result(), info)


def cut_torus(nu: int, nv: int, n_discs: int, frac: float = 0.05, device=None):
    """``synth.torus_mesh(nu, nv)`` with ``n_discs`` graph-geodesic discs removed, as (vs float32, faces int64) device
    tensors without the removed vertices.  The discs have the ring count ``synth.make_v_mask`` gives ``n_discs`` holes that
    total ``frac`` of the vertices; their centres sit on a regular grid of the torus' parameter plane, far enough apart
    that no two discs touch."""
    from . import meshprep, synth
    m = synth.torus_mesh(nu, nv, masks=False)
    V = m.num_vertices
    target = frac * V / max(n_discs, 1)
    rings = max(1, int(round((math.sqrt(max(12 * target - 3, 0.0)) - 3) / 6)))      # synth.make_v_mask
    gu = max(1, int(math.ceil(math.sqrt(n_discs * nu / nv))))
    gv = max(1, int(math.ceil(n_discs / gu)))
    if n_discs > 0 and min(nu // gu, nv // gv) < 2 * rings + 3:
        raise ValueError(f"cut_torus: {n_discs} discs of {rings} rings do not fit a {nu} x {nv} torus without touching")
    cells = [(a, b) for a in range(gu) for b in range(gv)][:n_discs]
    seeds = np.array([((a * nu) // gu + nu // (2 * gu)) * nv + (b * nv) // gv + nv // (2 * gv) for a, b in cells], np.int64)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    faces = torch.from_numpy(m.faces).to(dev)
    vs = torch.from_numpy(m.vs.astype(np.float32)).to(dev)
    if n_discs == 0:
        return vs, faces
    topo = meshprep.MeshTopology(faces, V, dev, with_f2f=False)
    seed_mask = torch.zeros((V, 1), dtype=torch.bool, device=dev)
    seed_mask[torch.from_numpy(seeds).to(dev)] = True
    hole = meshprep.dilate(topo, seed_mask, rings)[:, 0]
    keep_f = ~hole[faces].any(1)
    faces = faces[keep_f]
    used = torch.zeros(V, dtype=torch.bool, device=dev)
    used[faces.reshape(-1)] = True
    new_id = torch.cumsum(used.to(torch.int64), 0) - 1
    return vs[used].contiguous(), new_id[faces].contiguous()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m semigcn_amd.holes",
                                 description="close the holes of a triangle mesh (the hole filling of MeshFix.repair())")
    ap.add_argument("--scan", help="the mesh with holes (OBJ)")
    ap.add_argument("--out", help="where the filled mesh goes (OBJ)")
    ap.add_argument("--max-hole-edges", type=int, default=None, help="leave loops with more edges open (default: fill all)")
    ap.add_argument("--fair-steps", type=int, default=prepare.SMOOTH_ITER, help="smoothing steps on the inserted vertices")
    ap.add_argument("--fair", choices=("laplacian", "thin-plate"), default=None,
                    help="how the inserted vertices are faired: smoothing steps (the default), or the thin-plate solve")
    ap.add_argument("--torus", type=int, nargs=2, metavar=("NU", "NV"), help="run on a synthetic torus instead of --scan")
    ap.add_argument("--cut", type=int, default=40, help="with --torus: the number of discs removed")
    ap.add_argument("--repeat", type=int, default=1, help="run this many times and report the last (the first ones warm up)")
    ap.add_argument("--largest-component", action="store_true",
                    help="keep only the largest connected component before filling (components.keep_components)")
    args = ap.parse_args(argv)
    if (args.scan is None) == (args.torus is None):
        ap.error("give exactly one of --scan and --torus")
    if args.scan is not None and args.out is None:
        ap.error("--scan needs --out")
    if args.fair_steps < 0 or args.repeat < 1 or args.cut < 0:
        ap.error("--fair-steps, --cut must be >= 0 and --repeat >= 1")
    if args.max_hole_edges is not None and args.max_hole_edges < 0:
        ap.error("--max-hole-edges must be >= 0")
    mesh = read_obj(args.scan) if args.scan is not None else cut_torus(args.torus[0], args.torus[1], args.cut)
    extra = {}
    if args.largest_component:
        from .components import keep_components
        kept = keep_components(mesh, keep="largest")
        extra = {"n_components": len(kept.components), "n_dropped_faces": int(mesh[1].shape[0] - kept.faces.shape[0])}
        mesh = (kept.vs, kept.faces)
    for _ in range(args.repeat):
        out = fill_holes(mesh, max_hole_edges=args.max_hole_edges, fair_steps=args.fair_steps, timings=True,
                         fair=(args.fair or "laplacian").replace("-", "_"))
    if args.out:
        write_obj(args.out, out.vs, out.faces)
    rec = {"n_vertices": out.num_original_vertices, "n_faces": out.num_original_faces, "n_loops": len(out.loops),
           "n_filled": int(out.filled.sum()), "n_inserted_vertices": int(out.vs.shape[0] - out.num_original_vertices),
           "n_inserted_faces": int(out.faces.shape[0] - out.num_original_faces), "fair_steps": args.fair_steps}
    if args.fair is not None:            # without the option the line is what it was
        rec.update({"fair": args.fair, "fair_iterations": out.fair_info["iterations"] if out.fair_info else None,
                    "fair_converged": out.fair_info["converged"] if out.fair_info else None})
    rec.update(Stages.record(out.stage_ms))
    rec.update(extra)
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
