"""Network inputs from a hole-filled, remeshed mesh and the original scan, on the device.

Replaces the tail of the reference's preprocess/prepare.py -- everything after the remesh:

  ============================  ==========================================================
  here                          reference
  ============================  ==========================================================
  ``mean_edge_length``          ``edge_based_scaling``   preprocess/prepare.py:48-52
  ``scan_mask``                 ``write_mask``           preprocess/prepare.py:93-108
  ``laplacian_smooth``          ``smooth``               preprocess/prepare.py:110-114
  ``prepare_inputs``            ``normalize_scale`` -> ``write_mask`` -> ``smooth``  (:81-91, :135-137)
  ``Prepared.mesh_batch``       ``Datamaker.create_dataset``  util/datamaker.py:33-38,70-73
  ============================  ==========================================================

MeshFix's stage before them is ``semigcn_amd.components`` / ``holes`` / ``repair``; the isotropic remesh between the two is
``semigcn_amd.remesh`` (splits, collapses, flips, relaxation and re-projection).  The reference does the mask and the smoothing with pymeshlab filters and the scaling with numpy over a ``Mesh`` object; here the mask is the closest-point
query of ``evaluate.Surface`` (csrc/mesh_dist.hip) and the other two are csrc/mesh_smooth.hip.  HIP device only, like
the rest of the package: a CPU tensor raises ``SemigcnLibraryError``.

Inputs are what ``evaluate`` accepts: objects with ``.vs`` / ``.faces``, ``(vs, faces)`` pairs, cuda tensors or numpy
arrays (copied to the device).

Command line::

    python -m semigcn_amd.prepare --initial A_initial.obj --original A_original.obj [--gt A_gt.obj] [--out-dir D]
                                  [--no-rescale] [--eps 0.2] [--steps 30]

writes ``<name>_initial.obj``, ``<name>_original.obj``, ``<name>_gt.obj`` (rescaled), ``<name>_smooth.obj``,
``<name>_vmask.json`` and ``<name>_inserted.obj`` -- the names util/datamaker.py:33-38 reads -- and prints one JSON line
with ``scale``, ``n_vertices``, ``n_masked`` and ``steps``.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import capi, meshprep
from .capi import SemigcnLibraryError, SmoothPlan
from .evaluate import Surface
from .mesh_common import device_tensor, points, read_obj, vs_faces, write_obj
from .meshprep import MeshTopology

#: preprocess/prepare.py:12-14
SMOOTH_ITER, EPSILON = 30, 0.2

__all__ = ["mean_edge_length", "laplacian_smooth", "scan_mask", "prepare_inputs", "Prepared", "SmoothPlan", "write_obj",
           "SMOOTH_ITER", "EPSILON"]


def mean_edge_length(vs, edges) -> torch.Tensor:
    """``sum ||vs[a] - vs[b]|| / E`` over the UNIQUE edge list ``edges`` int64 [E, 2] (``MeshTopology.edges``) -- what
    ``edge_based_scaling`` divides by (preprocess/prepare.py:48-52) -- as a 0-dim float64 device tensor.  Float32 lengths,
    float64 sums in a fixed order (bit-reproducible); no host synchronisation.  ``E == 0`` gives NaN, the reference's 0 / 0."""
    return capi.mean_edge_length(points(vs), device_tensor(edges, torch.int64, "edges").reshape(-1, 2))


def _plan_for(topology_or_faces, num_vertices: int):
    """A context that gives a SmoothPlan for the argument: the caller's own, left open, or one made here and closed."""
    if isinstance(topology_or_faces, SmoothPlan):
        return contextlib.nullcontext(topology_or_faces)
    if isinstance(topology_or_faces, MeshTopology):
        faces = topology_or_faces.faces
        if topology_or_faces.num_vertices != num_vertices:
            raise SemigcnLibraryError(f"topology of {topology_or_faces.num_vertices} vertices, vs has {num_vertices}")
    else:
        faces = device_tensor(topology_or_faces, torch.int64, "faces").reshape(-1, 3)
    return SmoothPlan(faces, num_vertices)


def laplacian_smooth(vs, topology_or_faces, steps: int = SMOOTH_ITER, movable=None) -> torch.Tensor:
    """``steps`` steps of uniform-weight Laplacian smoothing with MeshLab's border rule (preprocess/prepare.py:110-114:
    ``laplacian_smooth`` with ``stepsmoothnum=30, cotangentweight=False``); returns float32 [V, 3].

    The rule:

    * ``k_ij`` is the number of faces that use the undirected edge ``{i, j}``.  An edge with ``k = 1`` is a border edge.
    * A vertex is a border vertex if any of its edges is a border edge.
    * Neighbour weights ``w_ij``: for an interior vertex ``w_ij = k_ij`` (on a closed manifold every neighbour therefore
      weighs 2); for a border vertex ``w_ij = 1`` on its border edges and ``w_ij = 0`` on all its other edges -- it slides
      along the border only.
    * One step is Jacobi -- every right-hand side reads the previous step's positions:
      ``p_i <- (p_i + sum_j w_ij p_j) / (1 + sum_j w_ij)``.
    * A vertex with no edges keeps its position, and so does a vertex with ``movable[i] == False``.
    * ``steps = 0`` returns a copy; ``steps < 0`` is an error raised before any device call.

    The rule restates vcglib's ``VertexCoordLaplacian`` from memory; the library is not available to compare against, so
    bit-parity with MeshLab is NOT claimed.  The rule above is the specification the tests pin.

    Every vertex sums its own neighbour list in ascending neighbour order (csrc/mesh_smooth.hip): no atomics, the result
    is bit-reproducible, and ``a`` steps followed by ``b`` steps equal ``a + b`` steps bit for bit.
    ``topology_or_faces``: a ``SmoothPlan`` (reused as it is), a ``MeshTopology`` or a face array [F, 3]."""
    steps = int(steps)
    if steps < 0:
        raise ValueError(f"laplacian_smooth: steps must be >= 0, got {steps}")
    p = points(vs)
    if movable is not None:
        movable = device_tensor(movable, torch.bool, "movable")
    with _plan_for(topology_or_faces, p.shape[0]) as plan:
        return plan.run(p, steps, movable)


def scan_mask(initial_vs, original, eps: float = EPSILON) -> torch.Tensor:
    """bool [V], True = the vertex lies on the scan: its unsigned distance to the surface ``original`` is below ``eps``
    (``write_mask``, preprocess/prepare.py:98-100; ``EPSILON = 0.2`` there, on meshes of unit mean edge length).
    ``original``: a ``Surface``, a mesh object or a ``(vs, faces)`` pair."""
    pts = points(initial_vs)
    surf = original if isinstance(original, Surface) else Surface(original)
    if pts.device != surf.device:
        pts = pts.to(surf.device)
    return surf._h.query(pts, signed=False, with_closest=False)[0] < float(eps)


@dataclass
class Prepared:
    """What ``prepare_inputs`` returns: everything the trainers read, resident on the device."""
    scale: torch.Tensor                  # 0-dim float64: mean edge length of ``initial`` before rescaling (1.0 when not rescaled)
    initial_vs: torch.Tensor             # [V, 3] float32, rescaled
    original_vs: torch.Tensor            # [Vo, 3] float32, rescaled
    original_faces: torch.Tensor         # [Fo, 3] int64
    gt_vs: Optional[torch.Tensor]        # [Vg, 3] float32, rescaled (None without gt)
    gt_faces: Optional[torch.Tensor]
    faces: torch.Tensor                  # [F, 3] int64, of ``initial``
    topology: MeshTopology               # edges, edge_index, f2f of ``initial``
    v_mask: torch.Tensor                 # [V] bool, True = on the scan
    f_mask: torch.Tensor                 # [F] bool, all three vertices on the scan
    x_pos: torch.Tensor                  # [V, 3] float32, the smoothed positions
    z1: torch.Tensor                     # [V, 3] float32, initial_vs - x_pos  (util/datamaker.py:70-73)
    steps: int = SMOOTH_ITER

    @property
    def inserted(self) -> torch.Tensor:
        """The vertices that fill the holes, ``initial_vs[~v_mask]`` (preprocess/prepare.py:105; one host synchronisation)."""
        return self.initial_vs[~self.v_mask]

    def mesh_batch(self, dm_size: int = 40, kn: Sequence[int] = (4,), rng=None):
        """The ``train.MeshBatch`` of this mesh, every field filled: ``SGCNTrainer`` / ``MGCNTrainer`` (``k2 > 0`` included)
        run on it as it is.  ``dm_size``, ``kn``, ``rng``: as ``meshprep.make_dummy_mask``."""
        from . import train
        z1, x_pos, ei = self.z1, self.x_pos, self.topology.edge_index

        class Data:
            pass
        data = Data()
        data.z1 = z1.clone().requires_grad_(True)         # util/datamaker.py:71
        data.x_pos = x_pos
        data.edge_index = ei
        dm = meshprep.make_dummy_mask(self.topology, dm_size=dm_size, kn=kn, rng=rng)[0]
        return train.MeshBatch(data, self.faces, self.initial_vs, train.face_normals(self.initial_vs, self.faces),
                               self.v_mask.float().view(-1, 1), self.f_mask.float().view(-1, 1), dm, f2f=self.topology.f2f)


def prepare_inputs(initial, original, gt=None, rescale: bool = True, eps: float = EPSILON, steps: int = SMOOTH_ITER,
                   device=None) -> Prepared:
    """``normalize_scale`` -> ``write_mask`` -> ``smooth`` of preprocess/prepare.py, from the hole-filled remeshed mesh
    ``initial`` and the scan ``original`` (``gt``: optional ground truth, only rescaled):

    1. divide ``initial``, ``original`` and ``gt`` by the mean edge length of ``initial`` (when ``rescale``);
    2. ``v_mask = scan_mask(initial, original, eps)``;
    3. ``x_pos = laplacian_smooth(initial, steps)``, ``z1 = initial - x_pos``.

    ``device``: the HIP device numpy inputs are copied to and the result lives on (default: the current one)."""
    if int(steps) < 0:
        raise ValueError(f"prepare_inputs: steps must be >= 0, got {steps}")
    ctx = torch.cuda.device(torch.device(device)) if device is not None and torch.cuda.is_available() else capi._NO_GUARD
    with ctx:
        vs, faces = vs_faces(initial)
        dev = vs.device if device is None else torch.device(device)
        if dev.type != "cuda":
            raise SemigcnLibraryError(f"prepare_inputs: device {dev} is not a HIP device (there is no CPU path)")
        o_vs, o_faces = vs_faces(original)
        g_vs, g_faces = vs_faces(gt) if gt is not None else (None, None)
        vs, faces, o_vs, o_faces = vs.to(dev), faces.to(dev), o_vs.to(dev), o_faces.to(dev)
        if g_vs is not None:
            g_vs, g_faces = g_vs.to(dev), g_faces.to(dev)
        topo = MeshTopology(faces, vs.shape[0], dev, with_f2f=True)
        if rescale:
            scale = capi.mean_edge_length(vs, topo.edges)
            # vs / scale with the quotient formed in float64 and rounded once (mesh.vs /= ave_len, preprocess/prepare.py:51,82,88)
            vs, o_vs = (vs.double() / scale).float(), (o_vs.double() / scale).float()
            if g_vs is not None:
                g_vs = (g_vs.double() / scale).float()
        else:
            scale = torch.ones((), dtype=torch.float64, device=dev)
        with Surface(o_vs, o_faces) as surf:
            v_mask = scan_mask(vs, surf, eps)
        x_pos = laplacian_smooth(vs, topo, steps)
        f_mask = meshprep.vmask_to_fmask(topo, v_mask)
        return Prepared(scale, vs, o_vs, o_faces, g_vs, g_faces, topo.faces, topo, v_mask, f_mask, x_pos, vs - x_pos, int(steps))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m semigcn_amd.prepare",
                                 description="scale, scan mask and smoothing of a remeshed mesh (the tail of "
                                             "preprocess/prepare.py)")
    ap.add_argument("--initial", required=True, help="hole-filled, remeshed mesh (OBJ)")
    ap.add_argument("--original", required=True, help="the scan with its holes (OBJ)")
    ap.add_argument("--gt", help="ground truth (OBJ); only rescaled")
    ap.add_argument("--out-dir", help="where the files go (default: a directory 'prepared' next to --initial)")
    ap.add_argument("--name", help="file name stem (default: that of --initial without '_initial')")
    ap.add_argument("--no-rescale", action="store_true", help="keep the scale (the meshes already have unit mean edge length)")
    ap.add_argument("--eps", type=float, default=EPSILON, help="mask threshold on the distance to the scan")
    ap.add_argument("--steps", type=int, default=SMOOTH_ITER, help="smoothing steps")
    args = ap.parse_args(argv)
    if args.steps < 0:
        ap.error("--steps must be >= 0")
    stem = os.path.splitext(os.path.basename(args.initial))[0]
    name = args.name or (stem[: -len("_initial")] if stem.endswith("_initial") and len(stem) > len("_initial") else stem)
    out_dir = args.out_dir or os.path.join(os.path.dirname(os.path.abspath(args.initial)), "prepared")
    os.makedirs(out_dir, exist_ok=True)
    p = prepare_inputs(read_obj(args.initial), read_obj(args.original), read_obj(args.gt) if args.gt else None,
                       rescale=not args.no_rescale, eps=args.eps, steps=args.steps)
    mask = p.v_mask.cpu().numpy()
    base = os.path.join(out_dir, name)
    write_obj(base + "_initial.obj", p.initial_vs, p.faces)
    write_obj(base + "_original.obj", p.original_vs, p.original_faces)
    if p.gt_vs is not None:
        write_obj(base + "_gt.obj", p.gt_vs, p.gt_faces)
    write_obj(base + "_smooth.obj", p.x_pos, p.faces)
    with open(base + "_vmask.json", "w") as f:
        json.dump(mask.tolist(), f)
    write_obj(base + "_inserted.obj", p.initial_vs.cpu().numpy()[~mask])
    print(json.dumps({"scale": float(p.scale), "n_vertices": int(mask.shape[0]), "n_masked": int(mask.sum()),
                      "steps": p.steps}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
