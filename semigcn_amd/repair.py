"""Find the self-intersections of a scan on the device and remove them: the third part of ``MeshFix.repair()``.

``MeshFix.repair()`` in the reference's preprocess/prepare.py:28-33 keeps the main component
(``components.keep_components``), closes the holes (``holes.fill_holes``) and removes self-intersecting triangles until
none are left.  This module is that last part and the whole stage in one call (``repair``).  As MeshFix does, it removes
the crossing faces and patches the holes that leaves; it does not cut and re-triangulate along the intersection curves.
MeshFix is not available to compare against; the predicate below is this module's own and is the specification the tests
pin (tests/intersect_oracle.py restates it in numpy, exact integers on integer input).  The kernels are
csrc/mesh_isect.hip: a self-overlap walk of the hierarchy ``evaluate.Surface`` builds (csrc/mesh_dist.hip).

**The predicate.**  All determinants are evaluated in float64 on the float32 coordinates, with plain multiplies and adds
(no fused multiply-add), in the order written here.  ``det[u, v, w] = u.x (v.y w.z - v.z w.y) + u.y (v.z w.x - v.x w.z)
+ u.z (v.x w.y - v.y w.x)``; ``orient3d(a, b, c, d) = det[a - d, b - d, c - d]``.  ``orient2d(a, b, c) = (a.u - c.u)
(b.v - c.v) - (a.v - c.v) (b.u - c.u)`` is taken after dropping the coordinate axis in which the float64 normal ``(b - a)
x (c - a)`` of the triangle in question is largest in magnitude (ties: the lowest axis); ``u``, ``v`` are the two remaining
axes in ascending order.  Only the SIGN of a determinant is used and exactly zero is its own case: there is no epsilon.
For integer coordinates of magnitude at most 2^10 every determinant is exact, so the device agrees with an exact
evaluation pair for pair, coplanar and touching cases included.

*Faces that take part in no pair* (counted in ``n_degenerate``): a face with a repeated vertex id, and a face whose
float64 normal is exactly zero.

*Segment pq against the closed triangle abc.*  ``sp = orient3d(a, b, c, p)``, ``sq = orient3d(a, b, c, q)``.  If they are
not both zero the segment hits when ``sp sq <= 0`` and the signs of ``orient3d(p, q, a, b)``, ``orient3d(p, q, b, c)``,
``orient3d(p, q, c, a)`` are all ``>= 0`` or all ``<= 0``.  If both are zero the segment lies in the plane: in the
projection (abc's axis) it hits when ``p`` or ``q`` lies in the closed triangle (the three ``orient2d`` of the point
against ab, bc, ca all ``>= 0`` or all ``<= 0``) or when it meets one of the closed edges ab, bc, ca: the closed
segment-segment test with ``orient2d``, collinear overlap (all four signs zero and the coordinate intervals overlap)
included.

*A pair (i, j), i < j,* is tested with face i first.  The faces' vertices are compared by id:

* no shared vertex: a pair when one of the edges ``(f0, f1), (f1, f2), (f2, f0)`` of i hits j or one of j's hits i;
* exactly one shared vertex: only the edge opposite the shared vertex, of each face against the other one; meeting at the
  shared vertex alone is not an intersection;
* exactly two shared vertices: with ``a`` the apex of i, ``(u, v)`` the two vertices that follow it in i's cyclic order
  and ``b`` the apex of j, a pair only when ``orient3d(u, v, a, b) == 0`` and ``orient2d(u, v, a) orient2d(u, v, b) > 0``
  in the projection of i (a fold-over: coplanar, both apexes strictly on one side of the shared edge);
* the same three vertices: always a pair (a duplicate).

**The result** of ``self_intersections``: ``pairs`` int64 [P, 2] in canonical order (``i < j``, rows sorted
lexicographically), ``face_mask`` bool [F] (the faces that appear in a pair) and ``n_degenerate``.  Two calls return
identical bytes.

**The repair loop** (``remove_self_intersections``), per round: detect; stop when there is no pair; delete the flagged
faces together with ``grow`` rings of faces that share a vertex with them; ``components.keep_components(..., "largest")``
(which also drops the vertices the deletion left unreferenced and any piece it cut off); ``holes.fill_holes``.  Running
out of rounds returns with ``remaining > 0``; it does not raise.  ``holes.fill_holes`` raises ``ValueError`` when a
deletion leaves a boundary that cannot be ordered into loops.

Inputs are what ``evaluate`` accepts; HIP device only: a CPU tensor raises ``SemigcnLibraryError``.

Command line::

    python -m semigcn_amd.repair in.obj out.obj [--grow G] [--max-rounds N] [--max-hole-edges N] [--fair-steps K] [--manifold]
    python -m semigcn_amd.repair --torus NU NV --fold K [--repeat R] [--out B.obj]

prints one JSON line.  The file form runs ``repair`` and reports ``rounds``, ``removed_per_round``, ``remaining`` and the
sizes; ``--manifold`` is ``repair(..., make_manifold=True)``.  ``--torus NU NV --fold K`` runs on
``fold_torus(NU, NV, K)`` and reports the device time (events) of the stages of
one detection -- ``tree_ms`` (the hierarchy), ``count_ms``, ``scan_ms`` (offsets and the one host read of P),
``emit_sort_ms`` -- of the last of ``--repeat`` runs, then ``round_ms``: one full repair round (detect, delete, keep the
largest component, fill) with the detection that re-checks its result, and ``remaining_after_round``.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import sys
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from . import capi, prepare
from .capi import SemigcnLibraryError
from .evaluate import Surface
from .mesh_common import Stages, check_mesh, read_obj, vs_faces, write_obj

__all__ = ["self_intersections", "remove_self_intersections", "repair", "fold_torus", "Intersections", "Repaired"]


@dataclass
class Intersections:
    """The self-intersections of a face list (module docstring), on the device."""
    pairs: torch.Tensor         # int64 [P, 2], i < j, rows sorted lexicographically
    face_mask: torch.Tensor     # bool [F], True = the face appears in a pair
    n_degenerate: int           # faces with a repeated vertex id or a zero normal: they take part in no pair
    stage_ms: Optional[dict] = None

    def __len__(self) -> int:
        return int(self.pairs.shape[0])


@dataclass
class Repaired:
    """What ``remove_self_intersections`` returns and ``repair`` reports."""
    vs: torch.Tensor                  # float32 [V', 3]
    faces: torch.Tensor               # int64 [F', 3]
    rounds: int                       # rounds that deleted and patched
    removed_per_round: List[int] = field(default_factory=list)   # faces deleted in each round (flagged and grown)
    remaining: int = -1               # pairs of the returned mesh; -1: the last state was not re-checked
    vertex_ids: Optional[torch.Tensor] = None    # int64 [V'], new to original id, -1 for an inserted vertex


def self_intersections(vs, faces=None, surface: Optional[Surface] = None, timings: bool = False) -> Intersections:
    """The pairs of faces of ``(vs, faces)`` that cross (module docstring).  ``surface``: an ``evaluate.Surface`` already
    built from exactly these ``vs`` / ``faces`` -- the same device arrays, ``surface.vs`` and ``surface.faces``; anything
    else is a ``ValueError`` -- so that the hierarchy is not built twice; without it one is built and
    released.  One host synchronisation (the pair count).  ``timings``: also the device time of the stages."""
    vs, faces = vs_faces(*check_mesh(vs, faces, dtypes=False))
    V, F = vs.shape[0], faces.shape[0]
    dev = vs.device
    if surface is not None:
        if surface.device != dev or surface.faces.shape[0] != F or surface.vs.shape[0] != V:
            raise ValueError(f"self_intersections: the surface holds {surface.vs.shape[0]} vertices and "
                             f"{surface.faces.shape[0]} faces on {surface.device}, the mesh {V} and {F} on {dev}")
        if F and (surface.vs.data_ptr() != vs.data_ptr() or surface.faces.data_ptr() != faces.data_ptr()):
            raise ValueError("self_intersections: the surface was built from other arrays than vs / faces (pass "
                             "surface.vs and surface.faces, or no surface)")
    with capi._on_device(dev):
        if F == 0:
            return Intersections(torch.zeros((0, 2), dtype=torch.int64, device=dev),
                                 torch.zeros(0, dtype=torch.bool, device=dev), 0, {} if timings else None)
        st = Stages(dev, timings)
        with (Surface(vs, faces) if surface is None else contextlib.nullcontext(surface)) as s:
            st.mark("tree")
            n_any, n_upper, n_deg = s._h.self_count(vs, faces)
            st.mark("count")
            offsets = torch.zeros(F + 1, dtype=torch.int64, device=dev)
            torch.cumsum(n_upper, 0, dtype=torch.int64, out=offsets[1:])
            P, n_degenerate, dropped = torch.cat([offsets[F:], n_deg]).tolist()   # the one host synchronisation
            if dropped:
                raise SemigcnLibraryError(f"self_intersections: the walk's stack overflowed {dropped} time(s): the "
                                          "result would miss pairs (the hierarchy is deeper than its builder allows)")
            st.mark("scan")
            pairs = s._h.self_pairs(vs, faces, offsets, P)
            st.mark("emit_sort")
        return Intersections(pairs, n_any > 0, int(n_degenerate), st.result())


def _grown(faces: torch.Tensor, flagged: torch.Tensor, num_vertices: int, grow: int) -> torch.Tensor:
    """``flagged`` with ``grow`` rings of faces that share a vertex with it."""
    for _ in range(grow):
        touched = torch.zeros(num_vertices, dtype=torch.bool, device=faces.device)
        touched[faces[flagged].reshape(-1)] = True
        flagged = touched[faces].any(1)
    return flagged


def _loop(vs, faces, ids, grow, max_rounds, max_hole_edges, fair_steps, cut=False, fair="laplacian") -> Repaired:
    """``cut``: a deletion may leave two fans hanging on one vertex; cut them apart (``manifold.split_nonmanifold``) before
    the largest component is taken, so that the boundary can always be ordered into loops."""
    from . import components, holes, manifold
    rounds, removed = 0, []
    while True:
        hits = self_intersections(vs, faces)
        if len(hits) == 0 or rounds >= max_rounds:
            return Repaired(vs, faces, rounds, removed, len(hits), ids)
        drop = _grown(faces, hits.face_mask, vs.shape[0], grow)
        removed.append(int(drop.sum()))
        left = faces[~drop].contiguous()
        if cut:
            split = manifold.split_nonmanifold((vs, left))
            vs, left, ids = split.vs, split.faces, ids[split.vertex_ids]
        kept = components.keep_components((vs, left), keep="largest")
        ids = ids[kept.vertex_ids]
        if kept.faces.shape[0] == 0:
            vs, faces = kept.vs, kept.faces
        else:
            filled = holes.fill_holes((kept.vs, kept.faces), max_hole_edges=max_hole_edges, fair_steps=fair_steps, fair=fair)
            vs, faces = filled.vs, filled.faces
            ids = torch.cat([ids, ids.new_full((vs.shape[0] - ids.shape[0],), -1)])
        rounds += 1


def _check_loop_args(grow, max_rounds, max_hole_edges, fair_steps, fair="laplacian"):
    if fair not in ("laplacian", "thin_plate"):
        raise ValueError(f"remove_self_intersections: fair must be 'laplacian' or 'thin_plate', got {fair!r}")
    if int(grow) < 0:
        raise ValueError(f"remove_self_intersections: grow must be >= 0, got {grow}")
    if int(max_rounds) < 0:
        raise ValueError(f"remove_self_intersections: max_rounds must be >= 0, got {max_rounds}")
    if max_hole_edges is not None and int(max_hole_edges) < 0:
        raise ValueError(f"remove_self_intersections: max_hole_edges must be >= 0 or None, got {max_hole_edges}")
    if int(fair_steps) < 0:
        raise ValueError(f"remove_self_intersections: fair_steps must be >= 0, got {fair_steps}")
    return int(grow), int(max_rounds), max_hole_edges, int(fair_steps)


def remove_self_intersections(mesh, grow: int = 1, max_rounds: int = 10, max_hole_edges: Optional[int] = None,
                              fair_steps: int = prepare.SMOOTH_ITER, fair: str = "laplacian") -> Repaired:
    """The repair loop of the module docstring on ``mesh``.  A clean mesh comes back as it is (``rounds == 0``, the same
    ``vs`` and ``faces`` bytes); ``max_rounds = 0`` only detects (``remaining = P``).  ``max_hole_edges``,
    ``fair_steps`` and ``fair`` go to ``holes.fill_holes``."""
    args = _check_loop_args(grow, max_rounds, max_hole_edges, fair_steps, fair)
    vs, faces = vs_faces(*check_mesh(mesh, dtypes=False))
    with capi._on_device(vs.device):
        return _loop(vs, faces, torch.arange(vs.shape[0], dtype=torch.int64, device=vs.device), *args, fair=fair)


def repair(mesh, grow: int = 1, max_rounds: int = 10, max_hole_edges: Optional[int] = None,
           fair_steps: int = prepare.SMOOTH_ITER, make_manifold: bool = False, fair: str = "laplacian"):
    """The whole ``MeshFix.repair()`` stage: keep the largest component, close the holes, remove the self-intersections.
    Returns ``(vs, faces, report)``: ``(vs, faces)`` is a valid ``initial`` for ``prepare.prepare_inputs``; ``report`` is
    the ``Repaired`` of the last step, its ``vertex_ids`` referring to the vertices of ``mesh``.  ``make_manifold``: run
    ``manifold.make_manifold`` first -- a soup, bow-tie vertices, edges with three faces and disagreeing orientations are
    then taken instead of refused -- and ``manifold.orient_faces`` once more after the holes are closed, since only then
    can the kept component be turned outward, and the bow-ties a round's deletion leaves are cut
    (``manifold.split_nonmanifold``) instead of stopping ``fill_holes``; ``vertex_ids`` then name the weld
    representatives.  ``fair`` goes to every ``holes.fill_holes`` call."""
    from . import components, holes, manifold
    args = _check_loop_args(grow, max_rounds, max_hole_edges, fair_steps, fair)
    vs, faces = vs_faces(*check_mesh(mesh, dtypes=False))
    with capi._on_device(vs.device):
        first = manifold.make_manifold((vs, faces)) if make_manifold else None
        if first is not None:
            vs, faces = first.vs, first.faces
        kept = components.keep_components((vs, faces), keep="largest")
        ids = kept.vertex_ids if first is None else first.vertex_ids[kept.vertex_ids]
        vs, faces = kept.vs, kept.faces
        if faces.shape[0]:
            filled = holes.fill_holes((vs, faces), max_hole_edges=max_hole_edges, fair_steps=args[3], fair=fair)
            vs, faces = filled.vs, filled.faces
            ids = torch.cat([ids, ids.new_full((vs.shape[0] - ids.shape[0],), -1)])
            if first is not None:
                faces = manifold.orient_faces((vs, faces), outward=True).faces
        report = _loop(vs, faces, ids, *args, cut=first is not None, fair=fair)
        return report.vs, report.faces, report


def fold_torus(nu: int, nv: int, n_folds: int, device=None):
    """``synth.torus_mesh(nu, nv)`` with ``n_folds`` patches of vertices pushed through the opposite wall of the tube, as
    (vs float32, faces int64) device tensors.  Deterministic.  Patch k is centred on the outer equator (tube angle 0) at
    ring ``(k nu) // n_folds + nu // (2 n_folds)`` and spans ``w = max(2, nv // 8)`` vertices to each side in both
    parameter directions; the vertex at offset ``(du, dv)`` from the centre moves against the tube's outward normal by
    ``2.5 r cos^2(pi du / 2 (w + 1)) cos^2(pi dv / 2 (w + 1))`` with ``r = nv / 2 pi`` the tube radius, so that the
    centre ends half a tube radius beyond the opposite wall.  ``ValueError`` when the patches would touch."""
    from . import synth
    if n_folds < 0:
        raise ValueError(f"fold_torus: n_folds must be >= 0, got {n_folds}")
    m = synth.torus_mesh(nu, nv, masks=False)
    vs = np.array(m.vs, np.float64)
    w = max(2, nv // 8)
    if n_folds > 0 and nu // n_folds < 2 * w + 3:
        raise ValueError(f"fold_torus: {n_folds} patches of half-width {w} do not fit {nu} rings without touching")
    r = nv / (2 * np.pi)
    d = np.arange(-w, w + 1)
    bump = np.cos(np.pi * d / (2 * (w + 1))) ** 2
    for k in range(n_folds):
        u0 = (k * nu) // n_folds + nu // (2 * n_folds)
        uu, vv = (u0 + d) % nu, d % nv
        idx = (uu[:, None] * nv + vv[None, :]).reshape(-1)
        th, ph = 2 * np.pi * uu / nu, 2 * np.pi * vv / nv
        normal = np.stack([np.cos(ph)[None, :] * np.cos(th)[:, None], np.cos(ph)[None, :] * np.sin(th)[:, None],
                           np.broadcast_to(np.sin(ph)[None, :], (d.shape[0], d.shape[0]))], -1).reshape(-1, 3)
        vs[idx] -= (2.5 * r * (bump[:, None] * bump[None, :]).reshape(-1, 1)) * normal
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return torch.from_numpy(vs.astype(np.float32)).to(dev), torch.from_numpy(m.faces).to(dev)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m semigcn_amd.repair",
                                 description="remove the self-intersections of a triangle mesh (MeshFix.repair())")
    ap.add_argument("scan", nargs="?", help="the mesh to repair (OBJ)")
    ap.add_argument("out_path", nargs="?", metavar="out", help="where the repaired mesh goes (OBJ)")
    ap.add_argument("--out", help="with --torus: where the mesh after one round goes (OBJ)")
    ap.add_argument("--grow", type=int, default=1, help="rings of neighbouring faces deleted with the crossing ones")
    ap.add_argument("--max-rounds", type=int, default=10)
    ap.add_argument("--max-hole-edges", type=int, default=None, help="leave loops with more edges open (default: fill all)")
    ap.add_argument("--fair-steps", type=int, default=prepare.SMOOTH_ITER, help="smoothing steps on the inserted vertices")
    ap.add_argument("--manifold", action="store_true", help="weld, cut and orient the input first (semigcn_amd.manifold)")
    ap.add_argument("--torus", type=int, nargs=2, metavar=("NU", "NV"), help="time the stages on a synthetic torus")
    ap.add_argument("--fold", type=int, default=0, help="with --torus: the number of patches pushed through the tube")
    ap.add_argument("--repeat", type=int, default=1, help="run the detection this many times and report the last")
    args = ap.parse_args(argv)
    if (args.scan is None) == (args.torus is None):
        ap.error("give either in.obj out.obj or --torus NU NV")
    if args.scan is not None and args.out_path is None:
        ap.error("in.obj needs out.obj")
    if args.grow < 0 or args.max_rounds < 0 or args.fair_steps < 0 or args.fold < 0 or args.repeat < 1:
        ap.error("--grow, --max-rounds, --fair-steps, --fold must be >= 0 and --repeat >= 1")
    if args.max_hole_edges is not None and args.max_hole_edges < 0:
        ap.error("--max-hole-edges must be >= 0")
    kw = dict(grow=args.grow, max_hole_edges=args.max_hole_edges, fair_steps=args.fair_steps)
    if args.scan is not None:
        mesh = read_obj(args.scan)
        vs, faces, rep = repair(mesh, max_rounds=args.max_rounds, make_manifold=args.manifold, **kw)
        write_obj(args.out_path, vs, faces)
        print(json.dumps({"n_vertices": int(mesh[0].shape[0]), "n_faces": int(mesh[1].shape[0]),
                          "out_vertices": int(vs.shape[0]), "out_faces": int(faces.shape[0]), "rounds": rep.rounds,
                          "removed_per_round": rep.removed_per_round, "remaining": rep.remaining}))
        return 0
    vs, faces = fold_torus(args.torus[0], args.torus[1], args.fold)
    for _ in range(args.repeat):
        hits = self_intersections(vs, faces, timings=True)
    rec = {"n_vertices": int(vs.shape[0]), "n_faces": int(faces.shape[0]), "n_folds": args.fold, "n_pairs": len(hits),
           "n_flagged_faces": int(hits.face_mask.sum()), "n_degenerate": hits.n_degenerate}
    rec.update(Stages.record(hits.stage_ms))
    st = Stages(vs.device, True)
    one = remove_self_intersections((vs, faces), max_rounds=1, **kw)
    st.mark("round")
    rec.update(Stages.record(st.result()))
    rec.update({"removed": one.removed_per_round, "out_vertices": int(one.vs.shape[0]), "out_faces": int(one.faces.shape[0]),
                "remaining_after_round": one.remaining})
    if args.out:
        write_obj(args.out, one.vs, one.faces)
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
