"""Make a raw scan manifold on the device: weld coincident vertices, cut what is not manifold, orient the faces.

``MeshFix(v, f).repair()`` in the reference's preprocess/prepare.py:28-33 takes a triangle soup, bow-tie vertices, edges
with three faces and faces that disagree about their orientation: it joins, cuts and orients before it selects
(``components``), fills (``holes``) and repairs (``repair``).  Those stages refuse such input; this module is the part
in front of them.  MeshFix is not available to compare against; the rules below are the specification the tests pin
(tests/manifold_oracle.py restates them serially in numpy; the device equals it exactly: ids equal, positions
bit-identical).  The kernels are csrc/mesh_manifold.hip.  Two calls return identical bytes.

The steps run in this order; ``V``, ``F`` are the input's sizes.  A vertex index outside ``[0, V)`` is an error.

**1. Weld.**  Two vertices are *coincident* when their three float32 coordinates have equal bits after ``-0.0`` is replaced
by ``+0.0``.  Bit-identical NaNs therefore coincide (and NaNs with different payloads do not).  Every vertex is replaced
by the lowest index of its class: ``vertex_map`` int64 [V], old to representative.  There is no distance tolerance: a
soup written from one vertex array repeats positions exactly, and welding within a tolerance is a different,
non-transitive problem.

**2. Clean faces**, after the weld.  A face with a repeated vertex is *degenerate*: dropped and counted
(``n_degenerate``), as in ``components``.  Faces with the same vertex *set*, in any rotation or reflection, are
duplicates: the lowest face index stays, the others are dropped and counted (``n_duplicate_faces``).

**3. Cut: the corner union.**  The elements are the 3 F' corners ``3 f + k`` of the surviving faces.  An undirected edge
with exactly two faces ``f``, ``g`` is a *link*: it unites ``f``'s and ``g``'s corners at one of its ends, and their
corners at the other end.  An edge with one face, or with three or more (``n_nonmanifold_edges``), unites nothing.  Every
class of corners becomes one output vertex with the position of its input vertex; output vertices are numbered by ascending
(input vertex, smallest corner of the class), vertices no surviving face uses are dropped.  ``vertex_ids`` int64 [V'] maps
new to input (the weld representative) and is non-decreasing; ``n_split_vertices`` = V' - (distinct input vertices in
use).  No face is deleted: two tetrahedra that share a vertex get a copy of it each; two that share an edge stay two closed
tetrahedra with their own copies of its ends; a fin on an edge of a closed surface comes loose and the surface stays closed,
because its two faces on that edge are still joined round both ends.  Afterwards every edge has at most two faces and the
faces at every vertex form one fan: at one vertex a face on a cut edge has at most one link left, so it ends a path of
corners, and a path has two ends.

**4. Orient.**  The edges are taken again from the *cut* faces (two faces of a cut edge share the new edge again when their
copies agree at both ends).  Two faces on an edge are *consistent* when they run along it in opposite directions; only
edges with exactly two faces count.  The parities are solved on the double cover, nodes ``2 f + s``: a consistent pair
unites ``(f, 0) ~ (g, 0)`` and ``(f, 1) ~ (g, 1)``, an inconsistent one ``(f, 0) ~ (g, 1)`` and ``(f, 1) ~ (g, 0)``.  With
``r0``, ``r1`` the smallest nodes of the classes of ``2 f`` and ``2 f + 1``: ``r0 == r1`` puts the face in a
*non-orientable* component, which is left exactly as given (``nonorientable`` per face, ``n_nonorientable`` components);
otherwise the face is flipped -- its last two vertices swapped -- when ``r1 < r0``.  The smallest face of every component
keeps its orientation.  ``n_components`` counts the components of this step, ``n_closed`` those with exactly two faces on
every edge.

**5. Outward** (optional).  For every orientable closed component, ``vol6`` = the sum over its faces, as step 4 left
them, of ``det[a, b, c] = a.x (b.y c.z - b.z c.y) + a.y (b.z c.x - b.x c.z) + a.z (b.x c.y - b.y c.x)``, each term in
float64 on the float32 coordinates by plain multiplies and adds (no fused multiply-add).  ``vol6 < 0`` flips the whole
component.  The order of the sum is not specified: only its sign is defined, and only away from zero.  Open components
keep the rule of step 4.

**6. Export.**  ``vs`` are rows of the input bit for bit, ``face_ids`` (new to old) ascends: the compaction is stable.
``flipped`` is the net effect of steps 4 and 5.

``weld_vertices`` runs steps 1-2 (the vertices in use are compacted stably), ``split_nonmanifold`` step 3 on the mesh as
given (degenerate faces go, duplicates stay), ``orient_faces`` steps 4-5 on the mesh as given: nothing is dropped or
renumbered, a degenerate face links to nothing and is never flipped.  ``make_manifold`` runs everything with one plan and
one upload.  A clean mesh comes back from each with the same ``vs`` and ``faces`` bytes.  With ``F = 0`` no device work is
done and nothing is welded.

Inputs are what ``evaluate`` accepts; HIP device only: a CPU tensor raises ``SemigcnLibraryError``.

Command line::

    python -m semigcn_amd.manifold in.obj out.obj [--no-weld] [--no-outward]
    python -m semigcn_amd.manifold --torus NU NV [--soup] [--flip PERMILLE] [--pinch K] [--repeat R] [--out B.obj]

prints one JSON line: the sizes, the counts and the device time of the stages (``manifold_ms``: everything the plan does;
``export_ms``).  ``--torus`` runs on ``mangled_torus`` and reports the last of ``--repeat`` runs.
"""
from __future__ import annotations

import argparse
import json
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import capi
from .capi import ManifoldPlan, SemigcnLibraryError  # noqa: F401
from .mesh_common import Stages, check_mesh, read_obj, vs_faces, write_obj

__all__ = ["weld_vertices", "split_nonmanifold", "orient_faces", "make_manifold", "mangled_torus", "Manifold", "ManifoldPlan"]


@dataclass
class Manifold:
    """What the functions of this module return (module docstring), on the device."""
    vs: torch.Tensor                  # float32 [V', 3], rows of the input bit for bit
    faces: torch.Tensor               # int64 [F', 3]
    vertex_map: torch.Tensor          # int64 [V], input vertex to its weld representative
    vertex_ids: torch.Tensor          # int64 [V'], new to input vertex (the representative), non-decreasing
    face_ids: torch.Tensor            # int64 [F'], new to old, ascending
    flipped: torch.Tensor             # bool [F']
    nonorientable: torch.Tensor       # bool [F']
    n_welded: int = 0
    n_degenerate: int = 0
    n_duplicate_faces: int = 0
    n_nonmanifold_edges: int = 0
    n_split_vertices: int = 0
    n_flipped: int = 0
    n_nonorientable: int = 0
    n_components: int = 0             # of step 4; 0 when it did not run
    n_closed: int = 0
    stage_ms: Optional[dict] = None   # device time of the stages, when asked for

    def counts(self) -> dict:
        return {name: getattr(self, name) for name in ManifoldPlan.COUNTS}


def _run(mesh, steps, timings) -> Manifold:
    vs, faces = vs_faces(*check_mesh(mesh))
    with capi._on_device(vs.device):
        st = Stages(vs.device, timings)
        with ManifoldPlan(vs, faces, steps) as plan:
            st.mark("manifold")
            out = plan.export(vs)
            st.mark("export")
            return Manifold(*out, **plan.counts, stage_ms=st.result())


def weld_vertices(mesh, timings: bool = False) -> Manifold:
    """Steps 1-2: coincident vertices joined, degenerate and duplicate faces dropped, the vertices in use compacted."""
    return _run(mesh, ("weld", "dedup", "drop"), timings)


def split_nonmanifold(mesh, timings: bool = False) -> Manifold:
    """Step 3 on ``mesh`` as given: bow-tie vertices and edges with three or more faces are cut apart."""
    return _run(mesh, ("cut", "drop"), timings)


def orient_faces(mesh, outward: bool = True, timings: bool = False) -> Manifold:
    """Steps 4-5 on ``mesh`` as given; the sizes stay and ``vs`` is the input's."""
    return _run(mesh, ("orient", "outward") if outward else ("orient",), timings)


def make_manifold(mesh, weld: bool = True, outward: bool = True, timings: bool = False) -> Manifold:
    """Every step of the module docstring.  ``(Manifold.vs, Manifold.faces)`` has at most two faces on every edge, one fan
    at every vertex and consistently oriented orientable components: ``components``, ``holes`` and ``remesh`` take it."""
    steps = ("dedup", "cut", "orient", "drop") + (("weld",) if weld else ()) + (("outward",) if outward else ())
    return _run(mesh, steps, timings)


def mangled_torus(nu: int, nv: int, soup: bool = False, flip_permille: int = 0, pinch: int = 0):
    """``synth.torus_mesh(nu, nv)`` as a scanner might write it, as (vs float32, faces int64) numpy arrays.  Deterministic.
    ``pinch``: pair k of K gives vertex ``a = (k nu // 2 K) nv`` and the vertex half way round the torus,
    ``a + (nu // 2) nv``, one shared index (the second is left unused): K bow-ties, K <= nu // 8.  ``flip_permille``: face f is reversed when
    ``(f * 2654435761 mod 2^32) mod 1000 < flip_permille``.  ``soup``: every face gets three vertices of its own."""
    from . import synth
    if pinch < 0 or not 0 <= flip_permille <= 1000:
        raise ValueError(f"mangled_torus: pinch must be >= 0 and flip_permille in [0, 1000], got {pinch}, {flip_permille}")
    if pinch > max(nu // 8, 0):
        raise ValueError(f"mangled_torus: {pinch} pinches do not fit {nu} rings (at most {nu // 8})")
    m = synth.torus_mesh(nu, nv, masks=False)
    vs, faces = m.vs.astype(np.float32), np.array(m.faces, np.int64)
    for k in range(pinch):
        a = ((k * nu) // (2 * pinch)) * nv
        faces[faces == a + (nu // 2) * nv] = a
    f = np.arange(faces.shape[0], dtype=np.uint64)
    rev = ((f * np.uint64(2654435761)) % np.uint64(1 << 32)) % np.uint64(1000) < np.uint64(flip_permille)
    faces[rev] = faces[rev][:, [0, 2, 1]]
    if soup:
        vs, faces = vs[faces.reshape(-1)], np.arange(3 * faces.shape[0], dtype=np.int64).reshape(-1, 3)
    return np.ascontiguousarray(vs), np.ascontiguousarray(faces)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m semigcn_amd.manifold",
                                 description="weld, cut and orient a raw triangle mesh (what MeshFix.repair() does first)")
    ap.add_argument("scan", nargs="?", help="the raw mesh (OBJ)")
    ap.add_argument("out_path", nargs="?", metavar="out", help="where the manifold mesh goes (OBJ)")
    ap.add_argument("--out", help="with --torus: where the result goes (OBJ)")
    ap.add_argument("--no-weld", action="store_true", help="leave coincident vertices apart")
    ap.add_argument("--no-outward", action="store_true", help="do not turn closed components outward")
    ap.add_argument("--torus", type=int, nargs=2, metavar=("NU", "NV"), help="run on a synthetic torus instead")
    ap.add_argument("--soup", action="store_true", help="with --torus: three vertices of its own for every face")
    ap.add_argument("--flip", type=int, default=0, metavar="PERMILLE", help="with --torus: the share of reversed faces")
    ap.add_argument("--pinch", type=int, default=0, help="with --torus: the number of bow-tie vertices")
    ap.add_argument("--repeat", type=int, default=1, help="run this many times and report the last (the first ones warm up)")
    args = ap.parse_args(argv)
    if (args.scan is None) == (args.torus is None):
        ap.error("give either in.obj out.obj or --torus NU NV")
    if args.scan is not None and args.out_path is None:
        ap.error("in.obj needs out.obj")
    if args.repeat < 1 or args.pinch < 0 or not 0 <= args.flip <= 1000:
        ap.error("--repeat must be >= 1, --pinch >= 0 and --flip in [0, 1000]")
    if args.scan is not None:
        mesh = read_obj(args.scan)
    else:
        mesh = mangled_torus(args.torus[0], args.torus[1], args.soup, args.flip, args.pinch)
    n_v, n_f = int(mesh[0].shape[0]), int(mesh[1].shape[0])
    mesh = vs_faces(mesh)                          # one upload, whatever --repeat says
    for _ in range(args.repeat):
        out = make_manifold(mesh, weld=not args.no_weld, outward=not args.no_outward, timings=True)
    dest = args.out_path if args.scan is not None else args.out
    if dest:
        write_obj(dest, out.vs, out.faces)
    rec = {"n_vertices": n_v, "n_faces": n_f, "out_vertices": int(out.vs.shape[0]), "out_faces": int(out.faces.shape[0])}
    rec.update(out.counts())
    rec.update(Stages.record(out.stage_ms))
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
