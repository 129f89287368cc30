"""Keep the scan's main component on the device: connected components of the face list, selection, stable compaction.

Replaces the first step of ``MeshFix.repair()`` in the reference's preprocess/prepare.py:28-33, which removes everything
but the scan's main connected component before it closes holes (``holes.fill_holes`` is the hole closing).  Floating
specks, scanner-bed remnants and flakes hanging on one vertex go here, so that ``fill_holes`` and ``prepare.prepare_inputs``
take the result as it is.  MeshFix is not available to compare against; the definitions below are the specification the
tests pin (tests/components_oracle.py restates them in numpy, with a serial union-find).  The kernels are
csrc/mesh_parts.hip.

**Degenerate faces.**  A face with a repeated vertex is *degenerate*: its label is -1, it is connected to nothing, it is
never kept, and it is counted (``n_degenerate``).  A vertex index outside ``[0, V)`` is an error.

**Connectivity.**  ``"edge"`` (the default, MeshFix's notion): two non-degenerate faces are connected when they share an
undirected edge -- orientation does not matter, and neither does how many faces meet on that edge.  ``"vertex"``: two
non-degenerate faces are connected when they share a vertex.  A component is a class of the transitive closure.  Two
tetrahedra that touch in one vertex are two components under ``"edge"`` and one under ``"vertex"``.

**Numbering.**  Components are numbered ``0 .. K - 1`` by ascending smallest face index, under both connectivities.
``face_count[k]`` is the number of faces of component ``k``.  The *largest* component has the most faces; among equals
the lower id wins, that is the one whose smallest face comes first (``-1`` when there is no component).  Nothing depends
on the order in which the device happens to unite faces.

**Selection.**  A face is kept when its component is kept; a vertex is kept when a kept face uses it.  ``keep="largest"``
keeps the largest component, ``keep="all"`` every component (so only degenerate faces and unreferenced vertices go), a
bool / uint8 tensor or array of length K keeps where it is non-zero.  ``min_faces=N`` additionally drops kept components
with fewer than N faces.

**Compaction.**  Stable: kept vertices and kept faces keep their relative order.  ``vs`` are the kept rows bit for bit,
``faces`` the kept faces with the new vertex ids, ``vertex_ids`` / ``face_ids`` (both ascending) map new to old.

Inputs are what ``evaluate`` accepts; HIP device only: a CPU tensor raises ``SemigcnLibraryError``.

Command line::

    python -m semigcn_amd.components --scan A.obj --out B.obj [--keep largest|all] [--min-faces N] [--connectivity edge|vertex]
    python -m semigcn_amd.components --torus NU NV --cut K --fragments M [--repeat R] [--out B.obj]

prints one JSON line with ``n_vertices``, ``n_faces``, ``n_components``, ``n_degenerate``, ``largest_faces``,
``kept_vertices``, ``kept_faces`` and the device time of each stage (``label_ms``, ``select_ms``, ``emit_ms``).
``--torus NU NV --cut K --fragments M`` runs on ``holes.cut_torus(NU, NV, K)`` with M fragments appended: octahedra of
edge length 1 placed outside the torus' bounding box, their vertices and faces after the torus'.
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
from .capi import PartsPlan, SemigcnLibraryError
from .mesh_common import Stages, device_tensor, read_obj, vs_faces, write_obj

__all__ = ["face_components", "keep_components", "Components", "Kept", "PartsPlan"]

_CONNECTIVITIES = ("edge", "vertex")


@dataclass
class Components:
    """The connected components of a face list (module docstring), on the device."""
    labels: torch.Tensor        # int64 [F], -1 = degenerate face
    face_count: torch.Tensor    # int64 [K]
    largest: int                # id of the component with the most faces (ties: the lower id), -1 when K = 0
    n_degenerate: int

    def __len__(self) -> int:
        return int(self.face_count.shape[0])


@dataclass
class Kept:
    """What ``keep_components`` returns."""
    vs: torch.Tensor                  # float32 [V', 3], the kept rows bit for bit
    faces: torch.Tensor               # int64 [F', 3], renumbered
    vertex_ids: torch.Tensor          # int64 [V'], new to old, ascending
    face_ids: torch.Tensor            # int64 [F'], new to old, ascending
    components: Components            # of the input
    kept: torch.Tensor                # bool [K]
    stage_ms: Optional[dict] = None   # device time of the stages, when asked for


def _check_connectivity(connectivity):
    if connectivity not in _CONNECTIVITIES:
        raise ValueError(f"connectivity must be 'edge' or 'vertex', got {connectivity!r}")


def _components_of(plan: PartsPlan) -> Components:
    labels, count = plan.labels()
    return Components(labels, count, plan.largest, plan.n_degenerate)


def face_components(faces, num_vertices: int, connectivity: str = "edge") -> Components:
    """The connected components of the triangle list ``faces`` [F, 3] over ``num_vertices`` vertices."""
    _check_connectivity(connectivity)
    f = device_tensor(faces, torch.int64, "faces").reshape(-1, 3)
    with capi._on_device(f.device), PartsPlan(f, int(num_vertices), connectivity) as plan:
        return _components_of(plan)


def _keep_mask(keep, comps: Components, min_faces, device) -> torch.Tensor:
    K = len(comps)
    if isinstance(keep, str):
        mask = torch.zeros(K, dtype=torch.bool, device=device)
        if keep == "all":
            mask[:] = True
        elif comps.largest >= 0:
            mask[comps.largest] = True
    else:
        mask = torch.as_tensor(np.asarray(keep) if not isinstance(keep, torch.Tensor) else keep).to(device).reshape(-1) != 0
        if mask.numel() != K:
            raise ValueError(f"keep_components: keep holds {mask.numel()} entries, the mesh has {K} components")
    if min_faces is not None:
        mask = mask & (comps.face_count >= int(min_faces))
    return mask


def keep_components(mesh, keep="largest", min_faces: Optional[int] = None, connectivity: str = "edge",
                    timings: bool = False) -> Kept:
    """Keep some connected components of ``mesh`` and compact what is left (module docstring).  ``keep``: ``"largest"``,
    ``"all"`` or a bool / uint8 tensor or array with one entry per component; ``min_faces``: also drop kept components
    with fewer faces.  ``(Kept.vs, Kept.faces)`` is a valid input to ``holes.fill_holes`` and ``prepare.prepare_inputs``.
    ``timings``: also measure the device time of the stages (``Kept.stage_ms``; one more synchronisation)."""
    _check_connectivity(connectivity)
    if isinstance(keep, str):
        if keep not in ("largest", "all"):
            raise ValueError(f"keep_components: keep must be 'largest', 'all' or one flag per component, got {keep!r}")
    elif not isinstance(keep, (torch.Tensor, np.ndarray, list, tuple)):
        raise ValueError(f"keep_components: keep must be 'largest', 'all' or one flag per component, got {type(keep).__name__}")
    elif ((isinstance(keep, torch.Tensor) and keep.dtype not in (torch.bool, torch.uint8)) or
          (isinstance(keep, np.ndarray) and keep.dtype not in (np.dtype(bool), np.dtype(np.uint8)))):
        raise ValueError(f"keep_components: keep must be bool or uint8, got {keep.dtype}")
    if min_faces is not None and int(min_faces) < 0:
        raise ValueError(f"keep_components: min_faces must be >= 0 or None, got {min_faces}")
    vs, faces = vs_faces(mesh)
    with capi._on_device(vs.device):
        st = Stages(vs.device, timings)
        with PartsPlan(faces, vs.shape[0], connectivity) as plan:
            comps = _components_of(plan)
            st.mark("label")
            mask = _keep_mask(keep, comps, min_faces, vs.device)
            plan.select(mask)
            st.mark("select")
            new_vs, new_faces, vertex_ids, face_ids = plan.emit(vs)
            st.mark("emit")
        return Kept(new_vs, new_faces, vertex_ids, face_ids, comps, mask, st.result())


def with_fragments(vs: torch.Tensor, faces: torch.Tensor, n_fragments: int):
    """``(vs, faces)`` with ``n_fragments`` octahedra of edge length 1 appended, their vertices and faces after the
    mesh's: fragment i sits 2 (i + 1) beyond the bounding box along x, level with the box's centre."""
    if n_fragments <= 0:
        return vs, faces
    unit = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64) / np.sqrt(2.0)
    tri = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)
    lo, hi = vs.min(0).values.cpu().numpy().astype(np.float64), vs.max(0).values.cpu().numpy().astype(np.float64)
    centre = np.stack([hi[0] + 2.0 * (np.arange(n_fragments) + 1), np.full(n_fragments, 0.5 * (lo[1] + hi[1])),
                       np.full(n_fragments, 0.5 * (lo[2] + hi[2]))], 1)
    f_vs = (centre[:, None, :] + unit[None]).reshape(-1, 3).astype(np.float32)
    f_faces = (vs.shape[0] + 6 * np.arange(n_fragments)[:, None, None] + tri[None]).reshape(-1, 3)
    return (torch.cat([vs, torch.from_numpy(f_vs).to(vs.device)]).contiguous(),
            torch.cat([faces, torch.from_numpy(f_faces).to(faces.device)]).contiguous())


def main(argv=None) -> int:
    from . import holes
    ap = argparse.ArgumentParser(prog="python -m semigcn_amd.components",
                                 description="keep the main connected component of a triangle mesh (the component "
                                             "selection of MeshFix.repair())")
    ap.add_argument("--scan", help="the mesh with fragments (OBJ)")
    ap.add_argument("--out", help="where the kept mesh goes (OBJ)")
    ap.add_argument("--keep", choices=("largest", "all"), default="largest")
    ap.add_argument("--min-faces", type=int, default=None, help="also drop kept components with fewer faces")
    ap.add_argument("--connectivity", choices=_CONNECTIVITIES, default="edge")
    ap.add_argument("--torus", type=int, nargs=2, metavar=("NU", "NV"), help="run on a synthetic torus instead of --scan")
    ap.add_argument("--cut", type=int, default=40, help="with --torus: the number of discs removed")
    ap.add_argument("--fragments", type=int, default=0, help="with --torus: the number of octahedra appended")
    ap.add_argument("--repeat", type=int, default=1, help="run this many times and report the last (the first ones warm up)")
    args = ap.parse_args(argv)
    if (args.scan is None) == (args.torus is None):
        ap.error("give exactly one of --scan and --torus")
    if args.scan is not None and args.out is None:
        ap.error("--scan needs --out")
    if args.repeat < 1 or args.cut < 0 or args.fragments < 0:
        ap.error("--cut, --fragments must be >= 0 and --repeat >= 1")
    if args.min_faces is not None and args.min_faces < 0:
        ap.error("--min-faces must be >= 0")
    if args.scan is not None:
        mesh = read_obj(args.scan)
    else:
        mesh = with_fragments(*holes.cut_torus(args.torus[0], args.torus[1], args.cut), args.fragments)
    for _ in range(args.repeat):
        out = keep_components(mesh, keep=args.keep, min_faces=args.min_faces, connectivity=args.connectivity, timings=True)
    if args.out:
        write_obj(args.out, out.vs, out.faces)
    c = out.components
    rec = {"n_vertices": int(mesh[0].shape[0]), "n_faces": int(mesh[1].shape[0]), "n_components": len(c),
           "n_degenerate": c.n_degenerate, "largest_faces": int(c.face_count[c.largest]) if len(c) else 0,
           "kept_vertices": int(out.vs.shape[0]), "kept_faces": int(out.faces.shape[0])}
    rec.update(Stages.record(out.stage_ms))
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
