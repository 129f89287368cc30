"""What semigcn_amd.prepare costs on the benchmark mesh (synth.torus_mesh(1000, 1000): V = 1 M, F = 2 M).

Times, in ONE process, with device events around chunks of calls after a warm-up, the variants taking turns:

  (a) smooth_hip      30 smoothing steps through sg_smooth_run (csrc/mesh_smooth.hip), the plan built beforehand
  (b) smooth_torch    the same 30 steps composed from what the package offered before: torch.index_add_ over
                      topology.edge_index with the same weights (the torus is closed: every weight is 2)
  (c) mean_edge       prepare.mean_edge_length over the 3 M unique edges
  (d) scan_mask       prepare.scan_mask against a copy of the torus with a patch of faces removed (surface built beforehand)

and checks first that (a) and (b) agree to rounding.  The bar: (a) is not slower than (b) in the same run.

    python tools/prepare_bench.py --out profiles/prepare_1m.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semigcn_amd import prepare, synth  # noqa: E402
from semigcn_amd.evaluate import Surface  # noqa: E402
from semigcn_amd.meshprep import MeshTopology  # noqa: E402


def timed_chunks(variants, chunk, chunks, warmup):
    """{name: [ms per call of each chunk]}: the variants take turns, one chunk of ``chunk`` calls each per round."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(chunks):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(chunk):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) / chunk)
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "chunks": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="1000x1000")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--chunk", type=int, default=10)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prepare_bench.py needs a HIP device: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    nu, nv = map(int, args.mesh.split("x"))
    m = synth.torus_mesh(nu, nv, masks=False)
    V, F = m.num_vertices, int(m.faces.shape[0])
    vs = torch.from_numpy(m.vs.astype(np.float32)).to(dev)
    faces = torch.from_numpy(m.faces).to(dev)
    topo = MeshTopology(faces, V, dev, with_f2f=False)
    plan = prepare.SmoothPlan(faces, V)
    steps = args.steps

    # (b): p <- (p + 2 sum_j p_j) / (1 + 2 deg) with the sums scattered over the directed edge list
    src, dst = topo.edge_index[0], topo.edge_index[1]
    deg = torch.bincount(dst, minlength=V).to(torch.float32)
    den = (1.0 + 2.0 * deg).unsqueeze(1)

    def smooth_torch():
        p = vs
        for _ in range(steps):
            acc = p.clone()
            acc.index_add_(0, dst, p[src], alpha=2.0)
            p = acc / den
        return p

    def smooth_hip():
        return plan.run(vs, steps)

    a, b = smooth_hip(), smooth_torch()
    agree = float((a - b).abs().max())
    tol = 2.0 * steps * (int(deg.max()) + 3) * 2.0 ** -24 * float(vs.abs().max()) * 2      # both sides carry the rounding bound
    if not agree <= tol:
        raise SystemExit(f"smooth_hip and smooth_torch differ by {agree:.3e} (> {tol:.3e})")

    # (d): `original` = the torus without the faces inside a box around one vertex (a patch of a few thousand faces)
    centre = m.vs[(nu // 2) * nv]
    inside = (np.abs(m.vs - centre) < 30.0).all(1)
    org_faces = torch.from_numpy(m.faces[~inside[m.faces].any(1)]).to(dev)
    surf = Surface(vs, org_faces)
    n_masked = int(prepare.scan_mask(vs, surf).sum())

    variants = {"smooth_hip": smooth_hip, "smooth_torch": smooth_torch,
                "mean_edge": lambda: prepare.mean_edge_length(vs, topo.edges),
                "scan_mask": lambda: prepare.scan_mask(vs, surf)}
    t = {k: summary(v) for k, v in timed_chunks(variants, args.chunk, args.chunks, args.warmup).items()}
    d_mean = 2.0 * topo.edges.shape[0] / V
    res = {"mesh": args.mesh, "V": V, "F": F, "E": int(topo.edges.shape[0]), "steps": steps,
           "device": torch.cuda.get_device_name(0), "timed_calls_per_variant": args.chunk * args.chunks,
           "smooth_max_abs_difference_hip_vs_torch": agree, "scan_mask_faces_removed": F - int(org_faces.shape[0]),
           "scan_mask_vertices_on_scan": n_masked, "mean_edge_length": float(prepare.mean_edge_length(vs, topo.edges)),
           # bytes one step asks for per vertex (csrc/mesh_smooth.hip): 16 d gathers + 16 own + 16 store + 4 d ids + d weights + 8 row bounds
           "smooth_bytes_per_step": int(V * (21 * d_mean + 40)),
           "times": t,
           "smooth_hip_ms_per_step": t["smooth_hip"]["median_ms"] / steps,
           "smooth_torch_over_hip": t["smooth_torch"]["median_ms"] / t["smooth_hip"]["median_ms"]}
    print(json.dumps({k: (v if k != "times" else {n: round(s["median_ms"], 4) for n, s in v.items()}) for k, v in res.items()}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    if t["smooth_hip"]["median_ms"] > t["smooth_torch"]["median_ms"]:
        raise SystemExit("sg_smooth_run is slower than the torch composition: the kernel has no reason to exist")


if __name__ == "__main__":
    main()
