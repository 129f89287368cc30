"""Refine a mesh to a target edge length on the device: split long edges, collapse short ones, flip towards regular
valence, relax and re-project.

Replaces the isotropic remesh the reference runs between MeshFix and the scaling (preprocess/prepare.py:35-42: MeshLab's
``remeshing_isotropic_explicit_remeshing`` at 0.6 % of the box diagonal).  What the networks need from that step is a
uniform edge length and valences near 6; ``holes.fill_holes`` patches at roughly the border's edge length, a ``-CAD``
input arrives with a few huge triangles, and ``meshprep.qem_contract`` only coarsens.  Edge collapse is its own operation
(2a.) and ``refine_mesh`` runs it only when asked (``collapse=True``); without it short edges stay and are only counted
(``n_short``).  MeshLab is not available to compare against; the construction below is this module's own and is the
specification the tests pin (tests/remesh_oracle.py and tests/collapse_oracle.py restate it in numpy with serial,
dictionary-based code).  The kernels are csrc/mesh_remesh.hip.

**Input.**  ``(vs float32 [V, 3], faces int64 [F, 3])``, as ``repair.repair`` returns it.  Every undirected edge must have
one face (a border edge) or two faces that run it in opposite directions.  ``ValueError`` is raised -- and nothing is done --
when an edge has three or more faces, when the two faces of an edge run it in the same direction, when a face repeats a
vertex or when a coordinate is not finite; the message gives the four counts and the smallest offending edge ``(lo, hi)``,
face and vertex.

**Edges.**  Half-edge ``h = 3 f + k`` of face ``f`` runs from ``faces[f, k]`` to ``faces[f, (k + 1) % 3]``.  The undirected
edges in ascending ``(lo, hi)`` order have the ranks ``r = 0, 1, ...``.  ``hash(r)`` is the 32-bit mixer ``x ^= x >> 16;
x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16`` (arithmetic modulo 2^32).  It is a bijection of the 32-bit
integers, so the hashes of two edges never tie; it breaks the long tie chains of regular grids.

**1. split_long_edges.**  A round works on the mesh it starts with.

* ``len2 = dx * dx + dy * dy + dz * dz`` in float32, summed left to right, with ``d = vs[hi] - vs[lo]``.  An edge is *long*
  when ``len2 > thr2``; ``thr2 = float32((4/3 target)^2)`` is formed once on the host in float64.
* The priority of a long edge is the tuple (``len2`` as its bit pattern, ``hash(r)``, lower ``r``); the third component
  never decides.  A long edge is *selected* when, in each of its faces, no other long edge has a higher priority.  A face
  therefore has at most one selected edge, and the longest edge of the mesh is always selected.
* Selected edges in ascending rank ``s = 0, 1, ...`` get vertex ``V + s`` at ``(vs[lo] + vs[hi]) * 0.5f`` per component,
  with ``parents[V + s] = (lo, hi)``.  A face ``f`` whose corner ``k`` starts the selected edge, ``a = v_k, b = v_{k+1},
  c = v_{k+2}``, becomes ``(a, m, c)`` in slot ``f`` and produces ``(m, b, c)`` in slot ``F + t``, ``t`` being its rank
  among the split faces in ascending ``f``.  Orientation is preserved; the topology is integers only.
* Rounds repeat until no edge is long or ``max_rounds`` rounds ran; running out of rounds is reported (``n_long > 0``),
  not raised.  A long edge waits for every longer long edge of its two faces, so where the edge length falls steadily
  along the surface (a regular grid under a smooth stretch, without noise) the rounds follow that slope one face at a time
  and their number grows with its length; scans and jittered meshes break such chains after a few faces.  ``parents`` is ``(i, i)`` for a vertex of the input; the ends of an inserted vertex may be inserted ones.

**2a. collapse_short_edges.**  A round works on the mesh it starts with: edge table, ranks, ``val``, border flags and
positions.  ``ring(v)`` is the set of vertices that share an edge with ``v``.

* ``lo2 = float32((4/5 target)^2)`` and ``thr2 = float32((4/3 target)^2)``, each formed once on the host in float64
  (``collapse_threshold``, ``split_threshold``).  An edge is *short* when ``len2 < lo2``, ``len2`` as in 1.
* A short edge ``{a, b}`` with two faces is a *candidate* when all of the following holds.  At most one end is a border
  vertex.  The kept vertex ``k`` is the border end when there is one, ``min(a, b)`` otherwise (vertices of the input
  outlive inserted ones); the removed vertex ``r`` is the other end, so ``r`` is interior and the faces at ``r`` form a
  fan; that fan must be one closed cycle (a vertex at which two fans touch is never removed).  With ``c`` the third vertex of
  the face of the lower half-edge and ``d`` that of the other face, ``c != d``.  *Link:* among ``ring(r) - {k}`` exactly
  two vertices ``w`` have ``{k, w}`` as an edge of the round's mesh (necessarily ``c`` and ``d``).  *Valence floors:*
  ``val[c] - 1``, ``val[d] - 1`` and ``val[k] + val[r] - 4`` each stay at or above 3 (2 for a border vertex), which refuses
  the tetrahedron.  *Length guard:* for every ``w`` in ``ring(r) - {k}``, not ``len2(k, w) > thr2``: a collapse never
  creates an edge that 1. would split, so the two stages cannot feed each other and ``n_long == 0`` keeps its exact
  meaning.  *Fold-over guard:* every face at ``r`` that does not contain ``k``, rotated to read ``(r, x, y)``, has
  ``n(r, x, y) . n(k, x, y) > 0`` strictly, with ``n``, the cross and the dot product of the flip guard (2.), in float64.
* The priority is (``0xFFFFFFFF - bits(len2)``, ``hash(rank)``, lower rank): the shortest edge comes first; packed as
  ``key << 32 | hash`` as in 2.  The hash is a bijection, so two candidates never tie.
* The *footprint* of a candidate is ``{r} + ring(r)``; it contains ``k``, ``c`` and ``d``.  A candidate is *selected* when no
  candidate whose footprint meets its own has a higher priority.  A collapse reads and writes only inside its own
  footprint: it rewrites the faces at ``r`` (all their vertices are in the footprint), creates the edges ``{k, w}`` for ``w``
  in ``ring(r)``, and changes the valences of ``k``, ``c`` and ``d``.  Footprint-disjoint winners are therefore independent,
  and the round's analysis stays valid for all of them.  The best candidate of the mesh always wins, so a round with a
  candidate makes progress.
* Apply: the two faces of the edge are deleted; every other face at ``r`` gets ``k`` in place of ``r`` in the same slot
  (orientation is preserved); vertex ``r`` is deleted; no position changes.  Surviving vertices and faces keep their relative
  order (stable compaction).  The border flags are carried over: a collapse here cannot change which vertices lie on a
  border.  ``parents`` entries are renumbered, and an entry that named a removed vertex names the vertex it went into.
* Rounds repeat until none is selected or ``max_rounds`` rounds ran (default 128); running out of rounds is reported, not
  raised.  ``counts`` holds the collapses per round, ``n_short`` the short edges of the result, whether or not a guard
  blocked them.  ``vertex_ids[i]`` is the input index of vertex ``i`` of the result (``vs == input[vertex_ids]``, bit for
  bit); ``merged_into[j]`` is the index in the result of the vertex that input vertex ``j`` ended up in.

**2. flip_edges.**  ``val[v]`` is the number of distinct edges at ``v``; the target valence is 6, or 4 for a vertex on a
border edge.  The *deviation* is the sum of ``|val - target|`` over the vertices that have an edge.

* A candidate is an interior edge ``{a, b}`` with the face ``(a, b, c)`` on one side and ``(b, a, d)`` on the other; of its
  two half-edges the one with the lower index ``h`` names ``a``, ``b`` and ``c``.  It needs ``c != d``; the edge ``{c, d}``
  must be absent from the round's mesh; ``val[a] - 1`` and ``val[b] - 1`` must not fall below 3 (2 for a border vertex);
  the *gain* -- the sum over ``a, b, c, d`` of ``|val - target|`` before, minus the same with ``a, b`` one lower and
  ``c, d`` one higher -- must be positive; and the *guard* must hold: with ``n(p, q, r) = (q - p) x (r - p)`` in float64 from
  the float32 coordinates, ``u x v = (u_y v_z - u_z v_y, u_z v_x - u_x v_z, u_x v_y - u_y v_x)`` and ``u . v = u_x v_x +
  u_y v_y + u_z v_z`` summed left to right, the normals ``n(a, d, c)`` and ``n(d, b, c)`` of the new triangles each have a
  strictly positive dot product with both ``n(a, b, c)`` and ``n(b, a, d)``.
* The priority is (gain, ``hash(r)``, lower ``r``).  A candidate is *selected* when no other candidate whose vertex set
  ``{a, b, c, d}`` meets its own has a higher priority.  Selected flips are vertex-disjoint.  ``(a, d, c)`` goes into the
  slot of ``(a, b, c)``, ``(d, b, c)`` into the slot of ``(b, a, d)``.
* Rounds repeat until none is selected or ``max_rounds`` rounds ran.  The deviation strictly falls every round.

**3. relax_project.**  ``prepare.laplacian_smooth(..., steps, movable=interior vertices)``, then
``evaluate.Surface.query`` on the moved vertices: the closest points become the positions.  Border vertices never move.

**4. refine_mesh.**  ``target`` defaults to ``target_percent`` % of the input's box diagonal (MeshLab's ``Percentage``).
The ``Surface`` is built once, from the input.  Each iteration is split (all rounds) -> flip -> relax_project, or with
``collapse=True`` split -> collapse -> flip -> relax_project on one plan: the splits that repair long edges leave slivers,
the collapse removes them before the flips see the valences.  A collapse renumbers the vertices, so ``Refined.parents`` is
``None`` then.  The closing passes are the same either way: a collapse creates no long edge, and they never collapse.  Since
relax_project moves vertices, it can push an edge back over 4/3 target; after the last iteration up to ``CLOSING_PASSES``
closing passes therefore split again (all rounds) and project only the vertices they insert (border ones stay), until a
pass finds no long edge: ``n_long == 0`` in the report then means that no edge of the RESULT has ``len2 > thr2``, exactly.
The result is a valid ``initial`` for ``prepare.prepare_inputs``.  The report holds, per iteration, the split and flip counts per round,
and for the result ``n_long`` (0 unless a cap ran out), ``n_short`` (the edges with ``len2 < lo2`` as 2a. defines it,
counted by the closing plan; they are treated only with ``collapse=True``), the min / mean / max edge length and the valence
deviation at the start (the input) and the end.

**Creases (``feature_angle``).**  Off by default: ``feature_angle=None`` is everything above, launch for launch.  With an
angle in degrees, ``0 < angle < 180``, the sharp edges of the input survive (MeshLab's ``featuredeg``, 30 there);
``cos_t = feature_cos(angle)`` is the float64 cosine of the float64 radians and goes to the plan (``RemeshPlan.set_feature``).
tests/remesh_feature_oracle.py restates this section.

* *The predicate.*  Every analysis -- each split, flip and collapse round, and ``RemeshPlan.features`` -- evaluates it for every
  edge with two faces, on the positions the round starts with.  With ``a, b, c, d`` named as in 2. (the lower half-edge names
  ``a, b, c``), ``n1 = n(a, b, c)``, ``n2 = n(b, a, d)`` with ``n``, the cross and the dot product of the flip guard (float64 on
  the float32 coordinates, summed left to right), ``dd = n1 . n2``, ``q = (n1 . n1) * (n2 . n2)`` and ``c2 = cos_t * cos_t``
  (float64 products as written), the edge is a *crease* when ``dd < 0 || dd * dd < c2 * q`` for ``cos_t >= 0``, and when
  ``dd < 0 && dd * dd > c2 * q`` for ``cos_t < 0``.  No square root, no epsilon, no normalisation: a tie is not a crease.  A face
  of zero area gives ``dd == 0 == q``: not a crease.  Border edges are never creases; they are features already.
* *Classes.*  ``nc[v]`` is the number of crease edges at ``v``.  A vertex is *border* as before; otherwise a *corner* when
  ``nc`` is neither 0 nor 2, *crease-line* when ``nc == 2`` -- its crease neighbours are ``lo(v) < hi(v)`` -- and *smooth* when
  ``nc == 0``.  ``RemeshPlan.features()`` returns ``vclass uint8 [V]`` (0 smooth, 1 crease-line, 2 corner, 3 border),
  ``crease_nbr int64 [V, 2]`` (``(lo, hi)`` for a crease-line vertex, ``(-1, -1)`` otherwise) and the crease edges
  ``int64 [C, 2]`` in ascending ``(lo, hi)``; with the setting off ``C = 0`` and the classes are 0 or 3.
* *Split* is unchanged: the midpoint of a crease edge lies on it.
* *Flip*: a crease edge is not a candidate.  Gain, targets, guard and priority are those of 2.
* *Collapse*: the conditions of 2a. with another choice of the kept vertex and two refusals.  ``k`` is, in this order, the
  border end if there is one; else the end with ``nc > 0`` if exactly one end has it; else the corner end if exactly one end is
  a corner; else ``min(a, b)``.  No candidate when the removed vertex ``r`` is a corner.  No candidate when ``r`` is crease-line
  and ``{a, b}`` is not a crease: a crease-line vertex leaves only along its crease.  *Straightness guard* for a crease-line
  ``r`` with ``w'`` its other crease neighbour: ``u = p_r - p_k``, ``v = p_w' - p_r`` (float64 differences of the float32
  coordinates) must have ``u . v > 0`` strictly, summed left to right.  Length guard, link, valence floors, fold-over guard,
  priority, footprint and apply are untouched; all flags come from the round's own analysis, so footprint-disjoint winners stay
  independent.
* *relax_project* takes ``feature_angle`` and ``creases``, a ``Surface`` of segments or an edge list ``[C, 2]`` into ``vs``; a
  segment ``{i, j}`` is the degenerate face ``(i, j, j)``, for which the closest-point query is specified (``segment_faces``).
  With ``P`` the positions: ``Q = laplacian_smooth(P, steps, movable = smooth class)``; ``R = P``, then ``steps`` Jacobi steps in
  which every crease-line vertex becomes ``(R[v] + R[lo] + R[hi]) / 3`` per component in float32, summed in that order and
  divided once (``sg_crease_step``: the arithmetic of the smoothing for a border vertex with two border edges; one launch per
  step, no atomics), corners and border vertices feeding in where they are.  A smooth vertex goes to the closest point of the
  triangle surface to ``Q[v]``, a crease-line vertex to the closest point of the segment surface to ``R[v]`` (it stays at
  ``P[v]`` when there is no segment surface), corners and border vertices keep ``P[v]`` bit for bit.
* *refine_mesh* sets the angle on every plan it makes and builds the segment ``Surface`` once, from the crease edges of the
  INPUT, beside the triangle ``Surface``; an input without a crease has none.  The closing passes project an inserted vertex
  by the same class rule, its class taken from ``features()`` after the split.  The report gains ``feature_angle``,
  ``n_crease_edges_start`` / ``n_crease_edges_end`` and ``n_corners_start`` / ``n_corners_end`` (the input and the result).
* *A limit.*  A crease-line vertex goes to the nearest segment of the input's creases however far that is.  The angle is for
  inputs whose creases are real (CAD meshes).  On a noisy scan, where a few scattered edges pass the predicate and the refined
  mesh grows crease-line vertices of its own, those vertices are dragged to the scattered segments, the edges between them are
  split again, and the mesh grows with every iteration until ``sg_remesh_split`` refuses the size ("With a feature
  angle").

Nothing here uses a float atomic; integer maxima and sums do not depend on order, so every output is bit-reproducible.
Inputs are what ``evaluate`` accepts; HIP device only: a CPU tensor raises ``SemigcnLibraryError``.

Command line::

    python -m semigcn_amd.remesh in.obj out.obj [--target X | --target-percent P] [--iterations N] [--collapse]
                                 [--feature-angle DEG]
    python -m semigcn_amd.remesh --torus NU NV --stretch S [--repeat R] [--target X | --target-percent P] [--iterations N]
                                 [--collapse] [--feature-angle DEG]
    python -m semigcn_amd.remesh --box N [--repeat R] ... (as --torus)

prints one JSON line with the sizes before and after, the rounds, the report and the device time of each stage
(``surface_ms``, ``split_ms``, ``flip_ms``, ``relax_ms`` and ``report_ms``, summed over the iterations).  ``--torus NU NV --stretch S`` runs on
``synth.torus_mesh(NU, NV)`` with x scaled by S.  ``--collapse`` runs the collapse stage in every iteration and adds
``n_collapsed``, ``collapse_rounds`` and ``collapse_ms``.  ``--box N`` runs on ``synth.box_mesh(N)``, the unit cube with an
N x N grid per face.  ``--feature-angle DEG`` keeps the creases and adds ``crease_ms``: the crease analysis of the input and
of every iteration, the segment ``Surface``, and the crease steps and their projection.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import math
import sys
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import capi, prepare
from .capi import RemeshPlan, SemigcnLibraryError
from .evaluate import Surface
from .mesh_common import Stages, check_mesh, read_obj, vs_faces, write_obj

__all__ = ["split_long_edges", "collapse_short_edges", "flip_edges", "relax_project", "refine_mesh", "Split", "Collapsed",
           "Flipped", "Refined", "RemeshPlan", "split_threshold", "collapse_threshold", "feature_cos", "segment_faces",
           "CLOSING_PASSES"]

#: refine_mesh: at most this many closing passes (split, project the inserted vertices) after the last iteration
CLOSING_PASSES = 4


@dataclass
class Split:
    """What ``split_long_edges`` returns.  The input's vertices are the prefix of ``vs``, bit-identical."""
    vs: torch.Tensor            # float32 [V', 3]
    faces: torch.Tensor         # int64 [F', 3]
    parents: torch.Tensor       # int64 [V', 2]
    counts: List[int]           # edges split per round
    n_long: int                 # long edges left: 0 unless max_rounds ran out


@dataclass
class Collapsed:
    """What ``collapse_short_edges`` returns.  ``vs == input[vertex_ids]``, bit for bit."""
    vs: torch.Tensor            # float32 [V', 3]
    faces: torch.Tensor         # int64 [F', 3]
    vertex_ids: torch.Tensor    # int64 [V']: the input index of every vertex of the result
    merged_into: torch.Tensor   # int64 [V]: the index in the result of the vertex every input vertex ended up in
    counts: List[int]           # collapses per round
    n_short: int                # short edges left, whether or not a guard blocked them


@dataclass
class Flipped:
    """What ``flip_edges`` returns; the positions are untouched."""
    faces: torch.Tensor         # int64 [F, 3]
    flips: List[int]            # flips per round
    deviation_before: int
    deviation_after: int


@dataclass
class Refined:
    """What ``refine_mesh`` returns."""
    vs: torch.Tensor            # float32 [V', 3]
    faces: torch.Tensor         # int64 [F', 3]
    parents: Optional[torch.Tensor]   # int64 [V', 2]: (i, i) for a vertex of the input, the ends of the split edge otherwise;
                                      # None with collapse=True: a collapse renumbers the vertices
    report: dict
    stage_ms: Optional[dict] = None


def split_threshold(target: float) -> float:
    """``thr2 = float32((4/3 target)^2)``, formed in float64."""
    return float(np.float32((4.0 / 3.0 * float(target)) ** 2))


def collapse_threshold(target: float) -> float:
    """``lo2 = float32((4/5 target)^2)``, formed in float64."""
    return float(np.float32((4.0 / 5.0 * float(target)) ** 2))


def _check_target(target, what="target"):
    t = float(target)
    if not (t > 0.0) or math.isinf(t):
        raise ValueError(f"{what} must be a positive finite number, got {target}")
    return t


def _check_rounds(n, what):
    n = int(n)
    if n < 0:
        raise ValueError(f"{what} must be >= 0, got {n}")
    return n


def feature_cos(angle_deg) -> float:
    """``cos_t`` of the crease predicate for a feature angle in degrees, ``0 < angle_deg < 180``: float64 ``cos`` of the
    float64 radians."""
    angle = float(angle_deg)
    if not 0.0 < angle < 180.0:                                # false for a NaN as well
        raise ValueError(f"feature_angle must lie strictly between 0 and 180 degrees, got {angle_deg}")
    return float(np.cos(np.radians(np.float64(angle))))


def _feature(feature_angle) -> Optional[float]:
    return None if feature_angle is None else feature_cos(feature_angle)


def _plan(vs: torch.Tensor, faces: torch.Tensor, cos_t: Optional[float] = None) -> RemeshPlan:
    plan = RemeshPlan(vs, faces)
    if cos_t is not None:
        plan.set_feature(cos_t)
    if not plan.valid:
        msg = (f"the mesh cannot be refined: {plan.n_nonmanifold} edge(s) with three or more faces, {plan.n_misoriented} "
               f"edge(s) whose two faces run them in the same direction (smallest offending edge {plan.bad_edge}), "
               f"{plan.n_degenerate} face(s) with a repeated vertex (smallest {plan.bad_face}), {plan.n_nonfinite} "
               f"vertex/vertices with a non-finite coordinate (smallest {plan.bad_vertex})")
        plan.close()
        raise ValueError(msg)
    return plan


def split_long_edges(vs, faces, target: float, max_rounds: int = 64) -> Split:
    """Split every edge longer than 4/3 ``target`` (module docstring, 1.)."""
    target, max_rounds = _check_target(target), _check_rounds(max_rounds, "max_rounds")
    vs, faces = vs_faces(*check_mesh((vs, faces)))
    with capi._on_device(vs.device):
        with _plan(vs, faces) as plan:
            counts, n_long = plan.split(split_threshold(target), max_rounds)
            out_vs, out_faces, parents, _ = plan.export()
    return Split(out_vs, out_faces, parents, counts, n_long)


def collapse_short_edges(vs, faces, target: float, max_rounds: int = 128, feature_angle: Optional[float] = None) -> Collapsed:
    """Collapse the interior edges shorter than 4/5 ``target`` that the guards allow (module docstring, 2a.; with
    ``feature_angle``, in degrees, also "Creases")."""
    target, max_rounds = _check_target(target), _check_rounds(max_rounds, "max_rounds")
    cos_t = _feature(feature_angle)
    vs, faces = vs_faces(*check_mesh((vs, faces)))
    with capi._on_device(vs.device):
        with _plan(vs, faces, cos_t) as plan:
            counts, n_short = plan.collapse(collapse_threshold(target), split_threshold(target), max_rounds)
            out_vs, out_faces, _, _ = plan.export()
            vertex_ids, merged_into = plan.collapse_maps()
    return Collapsed(out_vs, out_faces, vertex_ids, merged_into, counts, n_short)


def flip_edges(vs, faces, max_rounds: int = 32, feature_angle: Optional[float] = None) -> Flipped:
    """Flip edges towards valence 6 (4 on the border) (module docstring, 2.; with ``feature_angle``, in degrees, never a
    crease edge)."""
    max_rounds = _check_rounds(max_rounds, "max_rounds")
    cos_t = _feature(feature_angle)
    vs, faces = vs_faces(*check_mesh((vs, faces)))
    with capi._on_device(vs.device):
        with _plan(vs, faces, cos_t) as plan:
            flips, before, after = plan.flip(max_rounds)
            _, out_faces, _, _ = plan.export()
    return Flipped(out_faces, flips, before, after)


def _relax_project(vs, faces, border, surface: Surface, steps: int) -> torch.Tensor:
    interior = ~border
    moved = prepare.laplacian_smooth(vs, faces, steps=steps, movable=interior) if steps > 0 else vs
    closest = surface.query(moved, signed=False)[2]
    return torch.where(interior[:, None], closest, vs).contiguous()


def segment_faces(edges: torch.Tensor) -> torch.Tensor:
    """The segments ``{i, j}`` as the degenerate faces ``(i, j, j)`` that ``Surface`` takes: int64 [C, 3]."""
    edges = edges.reshape(-1, 2)
    return torch.stack([edges[:, 0], edges[:, 1], edges[:, 1]], 1).contiguous()


def _relax_smooth(vs, faces, vclass, surface: Surface, steps: int) -> torch.Tensor:
    """Creases, relax: the smooth class takes the umbrella steps and goes to the triangle surface; the rest stays."""
    smooth = vclass == 0
    moved = prepare.laplacian_smooth(vs, faces, steps=steps, movable=smooth) if steps > 0 else vs
    return torch.where(smooth[:, None], surface.query(moved, signed=False)[2], vs).contiguous()


def _relax_creases(out, vs, vclass, crease_nbr, segments: Optional[Surface], steps: int) -> torch.Tensor:
    """Creases, relax: the crease-line class takes ``steps`` steps along its polyline and goes to the closest segment; without
    a segment surface it stays where it is."""
    if segments is None:
        return out
    moved = vs
    for _ in range(steps):
        moved = capi.crease_step(moved, crease_nbr)
    return torch.where((vclass == 1)[:, None], segments.query(moved, signed=False)[2], out).contiguous()


def _as_surface(surface):
    return contextlib.nullcontext(surface) if isinstance(surface, Surface) else Surface(surface)


def _as_segments(creases, vs):
    """``creases`` of ``relax_project``: a ``Surface`` of segments, an edge list into ``vs`` (empty: none) or None."""
    if creases is None or isinstance(creases, Surface):
        return contextlib.nullcontext(creases)
    edges = creases if isinstance(creases, torch.Tensor) else torch.as_tensor(np.asarray(creases))
    if edges.numel() == 0:
        return contextlib.nullcontext(None)
    if edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError(f"creases must be a Surface or an edge list [C, 2], got {tuple(edges.shape)}")
    return Surface(vs, segment_faces(edges.to(device=vs.device, dtype=torch.int64)))


def relax_project(vs, faces, surface, steps: int = 1, feature_angle: Optional[float] = None, creases=None) -> torch.Tensor:
    """``steps`` Laplacian steps on the interior vertices, then their closest points on ``surface`` (a ``Surface``, a mesh
    object or a ``(vs, faces)`` pair) become the positions; border vertices never move (module docstring, 3.).  With
    ``feature_angle`` (degrees) the class rule of "Creases" holds: smooth vertices as before, crease-line vertices step along
    their crease and go to the closest point of ``creases`` (a ``Surface`` of segments, or an edge list ``[C, 2]`` into
    ``vs``; None or empty: they stay), corners and border vertices stay."""
    steps = _check_rounds(steps, "steps")
    cos_t = _feature(feature_angle)
    if cos_t is None and creases is not None:
        raise ValueError("creases needs feature_angle")
    vs, faces = vs_faces(*check_mesh((vs, faces)))
    with capi._on_device(vs.device):
        with _plan(vs, faces, cos_t) as plan:
            border = plan.export()[3]
            vclass, crease_nbr, _ = plan.features() if cos_t is not None else (None, None, None)
        with _as_surface(surface) as surf:
            if cos_t is None:
                return _relax_project(vs, faces, border, surf, steps)
            with _as_segments(creases, vs) as segs:
                out = _relax_smooth(vs, faces, vclass, surf, steps)
                return _relax_creases(out, vs, vclass, crease_nbr, segs, steps)


def _edge_report(vs, faces, n_short: int) -> dict:
    """Lengths of the unique edges (``meshprep.MeshTopology``): their number and min / mean / max.  ``n_short`` is handed in:
    it is ``len2 < lo2`` as 2a. defines it, and the closing plan counts it."""
    from .meshprep import MeshTopology
    edges = MeshTopology(faces, vs.shape[0], vs.device, with_f2f=False).edges
    if edges.shape[0] == 0:
        return {"n_edges": 0, "n_short": n_short, "edge_min": None, "edge_mean": None, "edge_max": None}
    length = (vs[edges[:, 0]] - vs[edges[:, 1]]).norm(dim=1)
    return {"n_edges": int(edges.shape[0]), "n_short": n_short, "edge_min": float(length.min()),
            "edge_mean": float(prepare.mean_edge_length(vs, edges)), "edge_max": float(length.max())}


def refine_mesh(mesh, target: Optional[float] = None, target_percent: float = 0.6, iterations: int = 5,
                split_rounds: int = 64, flip_rounds: int = 32, relax_steps: int = 1, timings: bool = False,
                collapse: bool = False, collapse_rounds: int = 128, feature_angle: Optional[float] = None) -> Refined:
    """Refine ``mesh`` to the edge length ``target`` (default: ``target_percent`` % of the box diagonal) by ``iterations``
    of split -> flip -> relax_project against the input's surface (module docstring, 4.).  ``timings``: also measure the
    device time of the stages (``Refined.stage_ms``; one more synchronisation).  ``collapse``: every iteration is
    split -> collapse -> flip -> relax_project (at most ``collapse_rounds`` rounds of 2a.); the vertices are renumbered, so
    ``Refined.parents`` is ``None``, and every iteration's report entry gains ``"collapse"`` and
    ``"n_short_after_collapse"``.  ``feature_angle`` (degrees): keep the creases of the input ("Creases"); it is set on every
    plan, the segment ``Surface`` is built from the input's crease edges, and the report gains the crease-edge and corner
    counts at the start and the end (with ``timings``, a ``crease`` stage)."""
    cos_t = _feature(feature_angle)
    iterations = _check_rounds(iterations, "iterations")
    split_rounds, flip_rounds = _check_rounds(split_rounds, "split_rounds"), _check_rounds(flip_rounds, "flip_rounds")
    collapse_rounds = _check_rounds(collapse_rounds, "collapse_rounds")
    relax_steps = _check_rounds(relax_steps, "relax_steps")
    if target is not None:
        target = _check_target(target)
    else:
        target_percent = _check_target(target_percent, "target_percent")
    vs, faces = vs_faces(*check_mesh(mesh))
    V0 = vs.shape[0]
    with capi._on_device(vs.device):
        if target is None:
            if V0 == 0:
                raise ValueError("refine_mesh: an empty mesh has no box diagonal; give target")
            diag = float((vs.max(0).values.double() - vs.min(0).values.double()).norm())
            target = _check_target(target_percent / 100.0 * diag, "target (target_percent of the box diagonal)")
        thr2, lo2 = split_threshold(target), collapse_threshold(target)
        _plan(vs, faces).close()                                  # refuse an invalid input before anything is built
        parents = torch.arange(V0, dtype=torch.int64, device=vs.device)[:, None].repeat(1, 2)
        rounds, dev_start = [], None
        st = Stages(vs.device, timings)
        with contextlib.ExitStack() as stack:
            surf = stack.enter_context(Surface(vs, faces))
            st.mark("surface")
            segs, feat_start, feat_end = None, None, None
            if cos_t is not None:                 # the creases of the INPUT: what crease-line vertices are projected to
                with _plan(vs, faces, cos_t) as plan:
                    vclass, _, crease_edges = plan.features()
                feat_start = (int(crease_edges.shape[0]), int((vclass == 2).sum()))
                if feat_start[0] > 0:
                    segs = stack.enter_context(Surface(vs, segment_faces(crease_edges)))
                st.mark("crease")
            st.result()               # with timings: wait for the device here and after every iteration, as the figures always did
            for _ in range(iterations):
                st.mark(None)
                with _plan(vs, faces, cos_t) as plan:
                    if dev_start is None:
                        dev_start = plan.flip(0)[1]
                        st.mark("report")
                    counts, n_long = plan.split(thr2, split_rounds)
                    st.mark("split")
                    if collapse:
                        collapsed, n_short = plan.collapse(lo2, thr2, collapse_rounds)
                        st.mark("collapse")
                    flips, before, after = plan.flip(flip_rounds)
                    vs, faces, par, border = plan.export()
                    st.mark("flip")
                    if cos_t is not None:
                        vclass, crease_nbr, _ = plan.features()
                        st.mark("crease")
                if not collapse:
                    parents = torch.cat([parents, par[parents.shape[0]:]])
                if cos_t is None:
                    vs = _relax_project(vs, faces, border, surf, relax_steps)
                    st.mark("relax")
                else:
                    moved = _relax_smooth(vs, faces, vclass, surf, relax_steps)
                    st.mark("relax")
                    vs = _relax_creases(moved, vs, vclass, crease_nbr, segs, relax_steps)
                    st.mark("crease")
                st.result()
                rounds.append({"split": counts, "flip": flips, "n_long": n_long, "deviation_after_split": before,
                               "deviation_after_flip": after})
                if collapse:
                    rounds[-1].update({"collapse": collapsed, "n_short_after_collapse": n_short})
            # closing: relax_project can push an edge back over the threshold.  Split again (all rounds), project only what
            # was inserted, and repeat until a pass finds nothing to split: then no position changed after the last analysis,
            # so n_long == 0 in the report means that no edge of the RESULT has len2 > thr2, exactly.
            st.mark(None)
            closing, n_long, dev_end, n_short = [], None, None, None
            for _ in range(CLOSING_PASSES + 1 if iterations > 0 else 1):
                with _plan(vs, faces, cos_t) as plan:
                    last = len(closing) == CLOSING_PASSES or iterations == 0
                    counts, n_long = plan.split(thr2, 0 if last else split_rounds)
                    if not counts:
                        dev_end = plan.flip(0)[1]
                        n_short = plan.collapse(lo2, thr2, 0)[1]          # no round: the count alone, len2 < lo2 as in 2a.
                        if cos_t is not None:
                            vclass, _, crease_edges = plan.features()
                            feat_end = (int(crease_edges.shape[0]), int((vclass == 2).sum()))
                        break
                    n_before = vs.shape[0]
                    vs, faces, par, border = plan.export()
                    if cos_t is not None:
                        vclass = plan.features()[0][n_before:]
                closing.append(sum(counts))
                if not collapse:
                    parents = torch.cat([parents, par[n_before:]])
                closest = surf.query(vs[n_before:], signed=False)[2]
                if cos_t is None:
                    vs[n_before:] = torch.where(border[n_before:, None], vs[n_before:], closest)
                else:                                     # the class rule of relax_project, without a step
                    new = torch.where((vclass == 0)[:, None], closest, vs[n_before:])
                    if segs is not None:
                        new = torch.where((vclass == 1)[:, None], segs.query(vs[n_before:], signed=False)[2], new)
                    vs[n_before:] = new
            st.mark("split")
            dev_start = dev_end if dev_start is None else dev_start
        report = {"target": target, "iterations": rounds, "closing": closing, "n_long": n_long, "deviation_start": dev_start, "deviation_end": dev_end,
                  "n_vertices": int(vs.shape[0]), "n_faces": int(faces.shape[0])}
        report.update(_edge_report(vs, faces, n_short))
        if cos_t is not None:
            report.update({"feature_angle": float(feature_angle), "n_crease_edges_start": feat_start[0],
                           "n_crease_edges_end": feat_end[0], "n_corners_start": feat_start[1], "n_corners_end": feat_end[1]})
        st.mark("report")
        return Refined(vs, faces, None if collapse else parents, report, st.result())


def main(argv=None) -> int:
    from . import synth
    ap = argparse.ArgumentParser(prog="python -m semigcn_amd.remesh",
                                 description="refine a triangle mesh to a target edge length: split, collapse (--collapse), flip, "
                                             "relax and project (the isotropic remesh of preprocess/prepare.py)")
    ap.add_argument("input", nargs="?", help="the mesh to refine (OBJ)")
    ap.add_argument("output", nargs="?", help="where the refined mesh goes (OBJ)")
    ap.add_argument("--target", type=float, default=None, help="target edge length")
    ap.add_argument("--target-percent", type=float, default=0.6, help="target as a percentage of the box diagonal")
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--torus", type=int, nargs=2, metavar=("NU", "NV"), help="run on a synthetic torus instead of an OBJ")
    ap.add_argument("--stretch", type=float, default=1.0, help="with --torus: scale x by this factor")
    ap.add_argument("--box", type=int, metavar="N", help="run on a synthetic unit cube with an N x N grid per face instead of an OBJ")
    ap.add_argument("--collapse", action="store_true", help="collapse short edges between the splits and the flips")
    ap.add_argument("--feature-angle", type=float, default=None, metavar="DEG",
                    help="keep the edges whose faces turn by more than DEG degrees (creases) and the corners where they meet")
    ap.add_argument("--repeat", type=int, default=1, help="run this many times and report the last (the first ones warm up)")
    args = ap.parse_args(argv)
    if (args.input is not None) + (args.torus is not None) + (args.box is not None) != 1:
        ap.error("give either in.obj out.obj or --torus NU NV" if args.box is None else "give one of in.obj out.obj, --torus NU NV and --box N")
    if args.input is not None and args.output is None:
        ap.error("in.obj needs out.obj")
    if args.iterations < 0 or args.repeat < 1 or not args.stretch > 0:
        ap.error("--iterations must be >= 0, --repeat >= 1 and --stretch > 0")
    if args.box is not None and args.box < 1:
        ap.error("--box must be >= 1")
    if args.input is not None:
        mesh = read_obj(args.input)
    elif args.box is not None:
        mesh = synth.box_mesh(args.box)
    else:
        m = synth.torus_mesh(args.torus[0], args.torus[1], masks=False)
        mesh = ((m.vs * np.array([args.stretch, 1.0, 1.0])).astype(np.float32), m.faces)
    for _ in range(args.repeat):
        out = refine_mesh(mesh, target=args.target, target_percent=args.target_percent, iterations=args.iterations, timings=True,
                          collapse=args.collapse, feature_angle=args.feature_angle)
    if args.output:
        write_obj(args.output, out.vs, out.faces)
    nv, nf = (int(x.shape[0]) for x in vs_faces(mesh))
    rep = dict(out.report)
    its = rep.pop("iterations")
    rep["n_closing"] = rep.pop("closing")
    rec = {"n_vertices_in": nv, "n_faces_in": nf, "split_rounds": [len(i["split"]) for i in its],
           "flip_rounds": [len(i["flip"]) for i in its], "n_split": [sum(i["split"]) for i in its],
           "n_flipped": [sum(i["flip"]) for i in its]}
    if args.collapse:
        rec.update({"n_collapsed": [sum(i["collapse"]) for i in its], "collapse_rounds": [len(i["collapse"]) for i in its]})
    rec.update(rep)
    rec.update(Stages.record(out.stage_ms))
    rec["total_ms"] = round(sum(out.stage_ms.values()), 4)
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
