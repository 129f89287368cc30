"""Build and query time of the device point-to-surface query (csrc/mesh_dist.hip; semigcn_amd.evaluate.Surface).

Surfaces: the c4 torus (1000 x 1000: 1 M vertices, 2 M triangles) and a 2000 x 2000 torus (4 M vertices, 8 M
triangles).  Queries: every vertex of a second torus of another resolution (nu - 10 x nv) with Gaussian noise, so the
two triangulations do not match.  Device events around each step, after a warm-up of both; prints one JSON line.

    python tools/mesh_distance_bench.py [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semigcn_amd import capi, evaluate, synth  # noqa: E402


def _time(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,2000")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_distance_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0)}
    for n in (int(s) for s in args.sizes.split(",")):
        m = synth.torus_mesh(n, n, masks=False)
        q = synth.torus_mesh(n - 10, n, masks=False, seed=7)
        qv = q.vs + np.random.default_rng(7).normal(0, 0.05, q.vs.shape)
        vs = torch.from_numpy(m.vs.astype(np.float32)).to(dev)
        faces = torch.from_numpy(m.faces).to(dev)
        pts = torch.from_numpy(qv.astype(np.float32)).to(dev)
        surf = evaluate.Surface(vs, faces)               # warm-up: code objects, allocator pools
        surf.query(pts)
        torch.cuda.synchronize()
        holder = {}

        def build():
            holder["s"] = capi.SurfaceHandle(vs, faces)

        b_med, b_min = _time(build, args.reps)
        q_med, q_min = _time(lambda: surf._h.query(pts), args.reps)
        res[f"V{m.num_vertices}"] = {"F": int(m.faces.shape[0]), "N_query": int(pts.shape[0]),
                                     "build_ms": round(b_med, 3), "build_ms_min": round(b_min, 3),
                                     "query_ms": round(q_med, 3), "query_ms_min": round(q_min, 3),
                                     "query_mpts_per_s": round(pts.shape[0] / q_med / 1e3, 1)}
        del holder, surf
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
