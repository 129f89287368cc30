"""`DeviceMesh.simplification` with ``criterion="qem"`` against ``criterion="collapse"`` on one mesh: three levels at ratio
0.6, alternating in one process after a warm-up of each.  Per side and level: wall time ending in a synchronise, the rounds
(collapse only: the stage reports them) and the summed cluster quadric error of the level against the level it came from
(``meshprep._vertex_quadrics`` of the finer level, the quantity tests/test_gpu_parity.py::_cluster_quadric_error computes).

    python tools/simplify_bench.py --torus 1000 1000 [--repeat 3] [--out profiles/simplify_1m.json]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semigcn_amd import meshprep, simplify, synth  # noqa: E402


def quadric_error(fine, coarse):
    Q = meshprep._vertex_quadrics(fine.vs, fine.faces)
    co = torch.from_numpy(coarse.pool_hash[:, 1]).to(fine.vs.device)
    Qc = torch.zeros((coarse.vs.shape[0], 4, 4), dtype=torch.float64, device=fine.vs.device).index_add_(0, co, Q)
    p4 = torch.cat([coarse.vs.double(), torch.ones((coarse.vs.shape[0], 1), dtype=torch.float64, device=fine.vs.device)], 1)
    return float(torch.einsum("ci,cij,cj->c", p4, Qc, p4).sum())


def levels(mesh, criterion, ratio, n_levels):
    out, cur, V = [], mesh, mesh.vs.shape[0]
    for l in range(n_levels):
        target = int(V * ratio ** (l + 1))                 # util/meshnet.py:172
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nxt = cur.simplification(target, criterion=criterion)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        rec = {"level": l + 1, "target_v": target, "n_vertices": int(nxt.vs.shape[0]), "n_faces": int(nxt.faces.shape[0]),
               "wall_ms": round(ms, 3), "cluster_quadric_error": quadric_error(cur, nxt)}
        if criterion == "collapse":                        # the same call again, for the stage's own report (not timed)
            rep = simplify.simplify_mesh(cur.vs, cur.faces, target_v=target, quadrics="sum", timings=True)
            rec.update({"rounds": len(rep.counts), "simplify_ms": round(rep.stage_ms["simplify_ms"], 3),
                        "largest_cluster": rep.report["largest_cluster"], "n_refused": rep.report["n_refused"]})
        out.append(rec)
        cur = nxt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--torus", type=int, nargs=2, default=(1000, 1000))
    ap.add_argument("--ratio", type=float, default=0.6)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m = synth.torus_mesh(args.torus[0], args.torus[1], masks=False)
    mesh = meshprep.DeviceMesh(m.x_pos, m.faces, "cuda:0")
    for crit in ("qem", "collapse"):                       # warm-up of each
        levels(mesh, crit, args.ratio, args.levels)
    runs = [{crit: levels(mesh, crit, args.ratio, args.levels) for crit in ("qem", "collapse")} for _ in range(args.repeat)]
    rec = {"mesh": f"torus {args.torus[0]} x {args.torus[1]}", "n_vertices": int(mesh.vs.shape[0]), "ratio": args.ratio,
           "device": torch.cuda.get_device_name(0), "runs": runs}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
