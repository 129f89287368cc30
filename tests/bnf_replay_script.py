"""Run by tests/test_gpu_bnf.py::test_cad_iteration_replays_from_a_hipgraph in a SUBPROCESS whose environment carries
DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 from the start: an SGCN trainer with the -CAD term (k2 = 4) on the fused loss node is
captured into a hipGraph, the replay must pass train.replay_matches_eager (loss and gradient increments of one replayed
iteration against an eager one) and then reproduce an eager trainer's losses bit for bit."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import golden_util as GU  # noqa: E402
from semigcn_amd import meshprep, synth, train  # noqa: E402
from semigcn_amd.networks import SingleScaleGCN  # noqa: E402

DEV = "cuda:0"
if not train.graphs_usable():
    print("GRAPHS_NOT_USABLE")
    sys.exit(0)
m = synth.torus_mesh(60, 40)
batch = bench.build_mesh_batch(m, torch.device(DEV), n_masks=3)
batch.f2f = meshprep.MeshTopology(m.faces, m.num_vertices, DEV).f2f


def build():
    net = SingleScaleGCN(DEV)
    GU.fill_state(net, seed=21)
    return net.to(DEV)


def run(capture):
    tr = train.SGCNTrainer(build(), batch, k2=4.0, capture=capture)
    losses = [float(tr.iteration_step()) for _ in range(8)]
    assert (tr._graphed is not None and tr._graphed.graph is not None) == capture
    return tr, losses


tr, lg = run(True)
assert train.replay_matches_eager(tr), "the replayed -CAD iteration differs from the eager one"
assert tr._graphed is not None
_, le = run(False)
assert lg == le, (lg, le)                      # no atomics anywhere: bit-identical
plain = train.SGCNTrainer(build(), batch)
assert le[0] > float(plain.iteration_step())   # the term is in the captured loss
print("CAD_REPLAY_OK", le[-1])
