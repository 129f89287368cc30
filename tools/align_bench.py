"""What semigcn_amd.align costs on the benchmark mesh (synth.torus_mesh(1000, 1000): V = 1 M, F = 2 M), in one process.

The target is the torus; the source is the same mesh under align.random_similarity(SEED, extent = the box diagonal), sampled
with n = 100000.  First ``align`` itself (device events per stage, summed over its iterations), rigid and with scale, twice
each (the first run warms up).  Then, at the pose it ended with, each of the three device steps of one iteration on its own:
20 timed repetitions after 3 warm-up ones, device events around each, and the bytes sg_align_accumulate has to move
(computed from the shapes) over its time.

    python tools/align_bench.py --out profiles/align_1m.json

profiles/align_1m.json is this file's output with one key, "reading", added by hand.
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
from semigcn_amd import align, capi, synth  # noqa: E402
from semigcn_amd.evaluate import Surface, sample_surface  # noqa: E402
from semigcn_amd.mesh_common import Stages, vs_faces  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--torus", type=int, nargs=2, default=(1000, 1000))
ap.add_argument("--samples", type=int, default=100000)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()
N = args.samples
out = {"command": "python tools/align_bench.py --out profiles/align_1m.json", "device": "MI355X",
       "mesh": f"{args.torus[0]}x{args.torus[1]}", "samples": N, "perturbation_seed": args.seed,
       "what": "align() of n samples of the perturbed torus onto the torus (stage times: device events, summed over the "
               "iterations; second of two runs), then 20 timed repetitions of each device step of one iteration at the final "
               "pose (device events around each; 3 warm-up repetitions)"}

m = synth.torus_mesh(args.torus[0], args.torus[1], masks=False)
vs, faces = m.vs.astype(np.float32), m.faces
v64 = vs.astype(np.float64)
diag = float(np.linalg.norm(v64.max(0) - v64.min(0)))
out["V"], out["F"], out["diag"] = int(vs.shape[0]), int(faces.shape[0]), diag
dvs, dfaces = vs_faces(vs, faces)
dev = dvs.device


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


with Surface(dvs, dfaces) as s:
    out["align"] = {}
    for with_scale in (False, True):
        truth = align.random_similarity(args.seed, with_scale, diag)
        src = ((v64 @ truth[:3, :3].T + truth[:3, 3]).astype(np.float32), faces)
        dsrc = vs_faces(*src)
        for _ in range(2):
            a = align.align(dsrc, s, n=N, with_scale=with_scale, timings=True)
        it = max(a.iterations, 1)
        rec = {"iterations": a.iterations, "converged": a.converged, "reason": a.reason, "rms": a.rms, "scale": a.scale,
               "matrix_error": float(np.abs(a.matrix @ truth - np.eye(4)).max()),
               "history": a.history, "stage_ms": Stages.record(a.stage_ms),
               "per_iteration_ms": {k: round(v / it, 4) for k, v in a.stage_ms.items() if k != "sample_ms"}}
        out["align"]["similarity" if with_scale else "rigid"] = rec
        print(json.dumps({k: rec[k] for k in rec if k != "history"}), flush=True)

    # one iteration's three steps at the final pose of the run with scale
    pts = sample_surface(dsrc, N, 0).points.contiguous()
    pose = np.concatenate([a.matrix[:3, :3].reshape(-1), a.matrix[:3, 3]])
    moved = torch.empty_like(pts)
    scratch = torch.empty(capi.ALIGN_SUMS * capi.REDUCE_BLOCKS, dtype=torch.float64, device=dev)
    times = {"transform": [], "query": [], "accumulate": []}
    for i in range(23):
        st = Stages(dev, True)
        capi.align_transform(pts, pose, out=moved)
        st.mark("transform")
        dist, face, closest = s.query(moved, signed=False)
        st.mark("query")
        capi.align_accumulate(dvs, dfaces, pts, pose, closest, face, dist, float("inf"), True, scratch)
        st.mark("accumulate")
        ms = st.result()
        if i >= 3:
            for k in times:
                times[k].append(ms[k + "_ms"])
    out["step_ms"] = {k: spread(v) for k, v in times.items()}
    nb = min((N + 255) // 256, capi.REDUCE_BLOCKS)
    # per row: pts 12 + closest 12 + face 4 + dist 4 + the face's three ids 24 + its nine coordinates 36; the block partials
    # are written once and read once; 40 doubles out
    moved_bytes = N * (12 + 12 + 4 + 4 + 24 + 36) + 2 * nb * 40 * 8 + 40 * 8
    t = out["step_ms"]["accumulate"]["median"]
    out["accumulate"] = {"rows": N, "blocks": nb, "bytes": moved_bytes, "ms_median": t, "gb_per_s": moved_bytes / t / 1e6,
                         "note": "two launches (block partials, then 40 lanes adding them in block order); the bytes are what "
                                 "the algorithm needs, gathers through face ids counted once per row"}
    out["transform"] = {"rows": N, "bytes": 24 * N, "ms_median": out["step_ms"]["transform"]["median"],
                        "gb_per_s": 24 * N / out["step_ms"]["transform"]["median"] / 1e6}
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
print(json.dumps({k: out[k] for k in ("step_ms", "accumulate", "transform")}, indent=1))
