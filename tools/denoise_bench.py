"""What semigcn_amd.denoise costs on the benchmark mesh (synth.torus_mesh(1000, 1000): V = 1 M, F = 2 M).

First the command line itself, in this process:

    python -m semigcn_amd.denoise --torus 1000 1000 --noise 0.1 --iterations 3 --repeat 4

(its JSON line is that of the last repeat).  Then, in the same process and with the same device-event timing around chunks of
calls after a warm-up, the variants taking turns:

  (a) update_hip      10 vertex-update steps through sg_vupdate_run (csrc/mesh_denoise.hip), the plan built beforehand
  (b) smooth_hip      30 smoothing steps through sg_smooth_run (csrc/mesh_smooth.hip): the yardstick, a one-launch Jacobi
                      gather over the same mesh
  (c) update_torch    the same 10 update steps composed from torch ops: gathers over the 3 F corners and index_add_

and checks first that (a) and (c) agree to rounding.

    python tools/denoise_bench.py --out profiles/denoise_1m.json
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from prepare_bench import summary, timed_chunks  # noqa: E402
from semigcn_amd import denoise, prepare, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="1000x1000")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--smooth-steps", type=int, default=30)
    ap.add_argument("--chunk", type=int, default=10)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("denoise_bench.py needs a HIP device: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    nu, nv = map(int, args.mesh.split("x"))
    cli = ["--torus", str(nu), str(nv), "--noise", "0.1", "--iterations", "3", "--repeat", "4"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        denoise.main(cli)
    line = json.loads(buf.getvalue().strip().splitlines()[-1])

    m = synth.torus_mesh(nu, nv, jitter=0.0, masks=False)
    V, F = m.num_vertices, int(m.faces.shape[0])
    vs = torch.from_numpy((m.vs + np.random.default_rng(7).normal(0.0, 0.1, m.vs.shape)).astype(np.float32)).to(dev)
    faces = torch.from_numpy(m.faces).to(dev)
    n = torch.linalg.cross(vs[faces[:, 1]] - vs[faces[:, 0]], vs[faces[:, 2]] - vs[faces[:, 0]], dim=1)
    normals = (n / n.norm(dim=1, keepdim=True)).contiguous()
    steps = args.steps
    plan = denoise.VertexUpdatePlan(faces, V)
    smooth = prepare.SmoothPlan(faces, V)

    cv = faces.reshape(-1)                                              # corner -> vertex
    cf = torch.arange(F, device=dev).repeat_interleave(3)               # corner -> face
    k = torch.bincount(cv, minlength=V).to(torch.float32).unsqueeze(1)
    nc = normals[cf]

    def update_torch():
        p = vs
        for _ in range(steps):
            c = ((p[faces[:, 0]] + p[faces[:, 1]]) + p[faces[:, 2]]) / 3.0
            t = (nc * (c[cf] - p[cv])).sum(1, keepdim=True)
            p = p + torch.zeros_like(p).index_add_(0, cv, t * nc) / k
        return p

    def update_hip():
        return plan.run(vs, normals, None, steps)

    a, b = update_hip(), update_torch()
    agree = float((a - b).abs().max())
    tol = 2.0 * steps * (plan.max_valence + 6) * 2.0 ** -24 * float(vs.abs().max()) * 2
    if not agree <= tol:
        raise SystemExit(f"update_hip and update_torch differ by {agree:.3e} (> {tol:.3e})")

    variants = {"update_hip": update_hip, "smooth_hip": lambda: smooth.run(vs, args.smooth_steps), "update_torch": update_torch}
    t = {name: summary(v) for name, v in timed_chunks(variants, args.chunk, args.chunks, args.warmup).items()}
    d_mean = 3.0 * F / V
    upd, smo = t["update_hip"]["median_ms"] / steps, t["smooth_hip"]["median_ms"] / args.smooth_steps
    res = {"command": "python -m semigcn_amd.denoise " + " ".join(cli),
           "what": "one process: the command line's JSON line of its fourth repeat (device events per stage), then chunks of "
                   "calls timed with device events, the variants taking turns",
           "cli": line, "update_ms_per_step_in_cli": line["update_ms"] / (line["iterations"] * line["vertex_steps"]),
           "mesh": args.mesh, "V": V, "F": F, "max_valence": plan.max_valence, "device": torch.cuda.get_device_name(0),
           "steps": steps, "smooth_steps": args.smooth_steps, "timed_calls_per_variant": args.chunk * args.chunks,
           "update_max_abs_difference_hip_vs_torch": agree,
           # bytes one step asks for (csrc/mesh_denoise.hip): per vertex 36 d + 40, per face 12 + 48 + 16
           "update_bytes_per_step": int(V * (36 * d_mean + 40) + F * 76), "smooth_bytes_per_step": int(V * (21 * d_mean + 40)),
           "times": t, "update_ms_per_step": upd, "smooth_ms_per_step": smo, "update_over_smooth_per_step": upd / smo,
           "update_torch_over_hip": t["update_torch"]["median_ms"] / t["update_hip"]["median_ms"]}
    print(json.dumps({key: (v if key != "times" else {name: round(s["median_ms"], 4) for name, s in v.items()})
                      for key, v in res.items()}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
