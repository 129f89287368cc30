"""What the -CAD term (k2 * fn_bnf_detach_loss, sgcn.py:133-135) costs a training iteration.

On the benchmark mesh (synth.torus_mesh(1000, 1000): V = 1 M, F = 2 M) it times, in ONE process, alternating between
the variants chunk by chunk after a warm-up, with device events around every chunk:

  SGCNTrainer.iteration_step   k2 = 0 | k2 = 4 on the fused loss node (csrc/mesh_bnf.hip) | k2 = 4 on the torch composition
  the loss step alone          forward + backward from a fixed position tensor, the same three variants

for bf16 feature storage (bench.py's headline configuration) and fp32.  A tree without the fused path (no
train.FUSED_CAD_TERM: the commit before it) runs the torch composition only, so the same file times the parent commit.

    python tools/cad_loss_bench.py --out profiles/cad_loss_ab.json --tag this
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from semigcn_amd import meshprep, synth, train  # noqa: E402
from semigcn_amd.networks import SingleScaleGCN  # noqa: E402

HAS_FUSED = hasattr(train, "FUSED_CAD_TERM")


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
    ap.add_argument("--chunk", type=int, default=10)
    ap.add_argument("--chunks", type=int, default=6, help="chunks per variant: chunk * chunks >= 50 timed iterations")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--out", default=None, help="JSON file to merge the result into, under --tag")
    ap.add_argument("--tag", default="this")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    nu, nv = map(int, args.mesh.split("x"))
    m = synth.torus_mesh(nu, nv)
    batch = bench.build_mesh_batch(m, dev, n_masks=5)
    batch.f2f = meshprep.MeshTopology(m.faces, m.num_vertices, dev).f2f
    res = {"mesh": args.mesh, "V": m.num_vertices, "F": int(m.faces.shape[0]), "fused_path": HAS_FUSED,
           "timed_iterations_per_variant": args.chunk * args.chunks, "device": torch.cuda.get_device_name(0)}

    def set_route(fused):
        if HAS_FUSED:
            train.FUSED_CAD_TERM = fused

    for name in [d for d in args.dtypes.split(",") if d]:      # --dtypes "": the loss step alone (profiling runs)
        dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[name]

        def trainer(k2):
            torch.manual_seed(314)
            net = SingleScaleGCN(dev).to(dev)
            if dtype != torch.float32:
                net.set_feature_dtype(dtype)
            return train.SGCNTrainer(net, batch, k2=k2)
        t0, tf, tt = trainer(0.0), (trainer(4.0) if HAS_FUSED else None), trainer(4.0)

        def step(tr, fused):
            def run():
                set_route(fused)
                tr.iteration_step()
            return run
        variants = {"k2=0": step(t0, True), "k2=4 torch": step(tt, False)}
        if HAS_FUSED:
            variants["k2=4 fused"] = step(tf, True)
        it = timed_chunks(variants, args.chunk, args.chunks, args.warmup)
        res[f"iteration_{name}"] = {k: summary(v) for k, v in it.items()}
        del t0, tf, tt
        torch.cuda.empty_cache()

    # the loss step alone, from a fixed position tensor (fp32: the network's output dtype in every configuration)
    pos0 = batch.target_pos + 0.02 * torch.randn(batch.target_pos.shape, device=dev, generator=torch.Generator(dev).manual_seed(5))
    holder = train.SGCNTrainer.__new__(train.SGCNTrainer)
    holder.mesh, holder.k1 = batch, 4.0

    def loss_step(k2, fused):
        def run():
            set_route(fused)
            holder.k2 = k2
            pos = pos0.detach().requires_grad_(True)
            train.SGCNTrainer.loss(holder, pos).backward()
        return run
    variants = {"k2=0": loss_step(0.0, True), "k2=4 torch": loss_step(4.0, False)}
    if HAS_FUSED:
        variants["k2=4 fused"] = loss_step(4.0, True)
    res["loss_step"] = {k: summary(v) for k, v in timed_chunks(variants, args.chunk, args.chunks, args.warmup).items()}

    for key in [k for k in res if k.startswith(("iteration_", "loss_step"))]:
        base = res[key]["k2=0"]["median_ms"]
        res[key]["added_by_cad_ms"] = {k: v["median_ms"] - base for k, v in res[key].items()
                                       if isinstance(v, dict) and k != "k2=0" and "median_ms" in v}
    print(json.dumps({k: ({kk: (round(vv["median_ms"], 3) if isinstance(vv, dict) and "median_ms" in vv else vv)
                           for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in res.items()}))
    if args.out:
        allr = json.load(open(args.out)) if os.path.isfile(args.out) else {}
        allr[args.tag] = res
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(allr, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
