"""What semigcn_amd.render costs on the benchmark mesh (synth.torus_mesh(1000, 1000): V = 1 M, F = 2 M), in one process.

First the command line itself, for 400 x 300 and 1600 x 1200 pixels, one frame and the 60-frame turntable:

    python -m semigcn_amd.render --torus 1000 1000 --size W H [--turntable 60] --repeat 3

(its JSON line is that of the last repeat).  Then, on one Surface of the box-normalised mesh: 7 timed single frames per size
after 2 warm-up frames (device events per stage), Surface.query on 2^20 vertices moved by N(0, 0.05 mean edge lengths) for context, and the
1600 x 1200 primary rays passed to Surface.ray_cast as an array (the sorted path).

    python tools/ray_bench.py --out profiles/ray_1m.json

profiles/ray_1m.json is this file's output with one key, "reading", added by hand.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semigcn_amd import render, synth  # noqa: E402
from semigcn_amd.evaluate import Surface  # noqa: E402
from semigcn_amd.mesh_common import Stages, vs_faces  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
out = {"command": "python tools/ray_bench.py --out profiles/ray_1m.json",
       "cli_command": "python -m semigcn_amd.render --torus 1000 1000 --size W H [--turntable 60] --repeat 3",
       "what": "one process: the command line's JSON line of its third repeat for each size, one frame and the 60-frame "
               "turntable (device events per stage); then 7 timed single frames per size, Surface.query on 2^20 vertices "
               "of the same surface moved by N(0, 0.05 mean edge lengths), and the 1600 x 1200 primary rays as an array "
               "through Surface.ray_cast, timed with device events",
       "device": "MI355X", "mesh": "1000x1000", "cli": {}}
for W, H in ((400, 300), (1600, 1200)):
    for extra, tag in (([], "frame"), (["--turntable", "60"], "turntable60")):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            render.main(["--torus", "1000", "1000", "--size", str(W), str(H), "--repeat", "3"] + extra)
        out["cli"][f"{W}x{H}_{tag}"] = json.loads(buf.getvalue().strip().splitlines()[-1])
        print(tag, W, H, buf.getvalue().strip(), flush=True)

m = synth.torus_mesh(1000, 1000, jitter=0.0, masks=False)
p, f = vs_faces(m.vs.astype(np.float32), m.faces)
p = render.normalize_to_box(p)
out["V"], out["F"] = int(p.shape[0]), int(f.shape[0])
dev = p.device
with Surface(p, f) as s:
    cam = render.turntable_camera(0, 1)
    out["times"] = {}
    for W, H in ((400, 300), (1600, 1200)):
        rs, ss = [], []
        for i in range(9):
            img = render.render(s, cam, W, H, timings=True)
            if i >= 2:
                rs.append(img.info["render_ms"]); ss.append(img.info["shade_ms"])
        out["times"][f"{W}x{H}"] = {"render_ms_median": statistics.median(rs), "render_ms_min": min(rs), "render_ms_max": max(rs),
                                    "shade_ms_median": statistics.median(ss), "rays": W * H,
                                    "mrays_per_s": W * H / statistics.median(rs) / 1e3,
                                    "hit_fraction": img.info["hit_fraction"], "leaf_visits_per_ray": img.info["leaf_visits_per_ray"]}
    g = torch.Generator(device="cpu").manual_seed(1)
    N = 1 << 20
    idx = torch.randint(0, p.shape[0], (N,), generator=g).to(dev)
    edge = float((p[f[:, 0]] - p[f[:, 1]]).norm(dim=1).mean())
    pts = (p[idx] + 0.05 * edge * torch.randn(N, 3, generator=g).to(dev)).contiguous()
    qs = []
    for i in range(9):
        st = Stages(dev, True)
        s.query(pts, signed=False)
        st.mark("query")
        if i >= 2:
            qs.append(st.result()["query_ms"])
    out["query"] = {"points": N, "jitter": 0.05 * edge, "query_ms_median": statistics.median(qs), "query_ms_min": min(qs), "query_ms_max": max(qs),
                    "mpoints_per_s": N / statistics.median(qs) / 1e3}
    # arbitrary rays through the sorted path: the same primary rays as an array
    o, d = render.camera_rays(cam, 1600, 1200)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    cs = []
    for i in range(7):
        st = Stages(dev, True)
        visits = s.ray_cast(o, d, with_visits=True)[1]
        st.mark("cast")
        if i >= 2:
            cs.append(st.result()["cast_ms"])
    out["ray_cast_1600x1200_rays_as_array"] = {"rays": 1600 * 1200, "cast_ms_median": statistics.median(cs),
                                               "mrays_per_s": 1600 * 1200 / statistics.median(cs) / 1e3,
                                               "leaf_visits_per_ray": visits / (1600 * 1200)}
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
print(json.dumps({k: out[k] for k in ("times", "query", "ray_cast_1600x1200_rays_as_array")}, indent=1))
