"""N > 1 path on CPU: world_size 2 and 3 over gloo, HIP handles swapped for the oracle-backed
doubles (conftest.py).  Contract: N-rank result == 1-rank result (outputs, loss, parameter
gradients after the gradient all-reduce, BatchNorm running statistics)."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _install_doubles():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import conftest
    from semigcn_amd import capi
    capi.GraphHandle = conftest.OracleGraphDouble
    capi.PoolHandle = conftest.OraclePoolDouble
    capi.gather_rows = lambda rows, X, out=None: X.index_select(0, rows.long())


GENERAL_KS = (1, 2, 4)            # K = 3 takes the two-ring shortcut; every other K the loop with one exchange per aggregation


def _general_loop_layers(g, x_all, r_all):
    """ChebConv(12, 20, K) (aggregate first) and ChebConv(20, 12, K) (product first for K >= 2) on this rank's rows:
    outputs, input gradients, reduced parameter gradients and the number of halo exchanges they took."""
    import golden_util as GU
    from semigcn_amd import dist as sgdist, nn as sgnn
    out, before = {}, sgdist.collective_counts["all_to_all"]
    for K in GENERAL_KS:
        for xs, rs in ((x_all, r_all), (r_all, x_all)):
            conv = sgnn.ChebConv(xs.shape[1], rs.shape[1], K=K)
            GU.fill_state(conv, seed=10 * K + xs.shape[1])
            x = xs[g.start:g.end].clone().requires_grad_(True)
            y = conv(x, g)
            (y * rs[g.start:g.end]).sum().backward()
            sgdist.all_reduce_gradients(list(conv.parameters()))
            key = f"gen_K{K}_{xs.shape[1]}_{rs.shape[1]}"
            out[key + "_y"], out[key + "_dx"] = y.detach().clone(), x.grad.clone()
            out[key + "_dw"], out[key + "_db"] = conv.lins[K - 1].weight.grad.clone(), conv.bias.grad.clone()
    out["gen_all_to_all"] = sgdist.collective_counts["all_to_all"] - before
    return out


def _run_rank(rank, world, port, out_dir, skip):
    _install_doubles()
    torch.set_num_threads(1)
    if world > 1:
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    import golden_util as GU
    from semigcn_amd import dist as sgdist, synth
    from semigcn_amd.networks import SingleScaleGCN
    mesh = synth.torus_mesh(24, 16, permute=True)
    part = sgdist.partition_mesh(mesh, rank, world, torch.device("cpu"), n_masks=2)
    model = SingleScaleGCN("cpu", skip=skip)
    GU.fill_state(model, seed=77)
    # (0) the pieces that talk across ranks, without kinks: one ChebConv layer and one BatchNorm
    from semigcn_amd import nn as sgnn
    g = part.graph
    V = mesh.num_vertices
    order = sgdist._reorder.morton_order(torch.from_numpy(mesh.x_pos))[0]
    gen = torch.Generator().manual_seed(5)
    x_all = torch.randn(V, 12, generator=gen)[order]            # processing order
    r_all = torch.randn(V, 20, generator=gen)[order]
    conv = sgnn.ChebConv(12, 20, K=3)
    GU.fill_state(conv, seed=1)
    x = x_all[g.start:g.end].clone().requires_grad_(True)
    y = conv(x, g)
    (y * r_all[g.start:g.end]).sum().backward()
    sgdist.all_reduce_gradients(list(conv.parameters()))
    bn = sgdist.DistBatchNorm1d(20)
    GU.fill_state(bn, seed=2)
    bn.train()
    xb = r_all[g.start:g.end].clone().requires_grad_(True)
    yb = bn(xb)
    (yb * yb * x_all[g.start:g.end, :1]).sum().backward()
    sgdist.all_reduce_gradients(list(bn.parameters()))
    conv2 = sgnn.ChebConv(20, 12, K=3)                            # narrowing: GEMM first, Clenshaw aggregation after
    GU.fill_state(conv2, seed=3)
    x2 = r_all[g.start:g.end].clone().requires_grad_(True)
    y2 = conv2(x2, g)
    (y2 * x_all[g.start:g.end]).sum().backward()
    sgdist.all_reduce_gradients(list(conv2.parameters()))
    zz = part.z1.detach().clone().requires_grad_(True)             # bounding box: gradient reaches the arg-extreme's owner
    lo_mm, hi_mm = sgdist.dist_min_max(zz)
    ((2.0 * lo_mm.sum() + 3.0 * hi_mm.sum()) / world).backward()      # each rank holds 1/world of the replicated term
    # the same extreme value on EVERY rank: the bound's gradient must still reach exactly one vertex of the mesh
    zt = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [0.0, 0.5, -0.5]], requires_grad=True)
    lo_t, hi_t = sgdist.dist_min_max(zt)
    ((2.0 * lo_t.sum() + 3.0 * hi_t.sum()) / world).backward()
    lin = {"tie_dz": zt.grad.clone(), "mm_lo": lo_mm.detach().clone(), "mm_hi": hi_mm.detach().clone(), "mm_dz": zz.grad.clone(),
           "conv_y": y.detach().clone(), "conv_dx": x.grad.clone(), "conv_dw": conv.lins[2].weight.grad.clone(),
           "conv_db": conv.bias.grad.clone(), "conv2_y": y2.detach().clone(), "conv2_dx": x2.grad.clone(),
           "conv2_dw": conv2.lins[1].weight.grad.clone(), "conv2_db": conv2.bias.grad.clone(), "bn_y": yb.detach().clone(), "bn_dx": xb.grad.clone(),
           "bn_dw": bn.weight.grad.clone(), "bn_db": bn.bias.grad.clone(),
           "bn_rm": bn.running_mean.clone(), "bn_rv": bn.running_var.clone()}
    lin.update(_general_loop_layers(g, x_all, r_all))

    tr = sgdist.DistSGCNTrainer(model, part, accumulate=2)
    # (1) one forward/backward on the initial parameters, gradients reduced explicitly
    model.train()
    pos = model(part, part.v_keep * part.dummy_masks[:, :1])
    loss = tr.loss(pos)
    loss.backward()
    sgdist.all_reduce_gradients(tr.params)
    g = part.graph
    out = {"lin": lin, "dz1": part.z1.grad.clone(), "loss0": float(loss.detach()), "pos": pos.detach().clone(), "range": (g.start, g.end), "n_halo": g.n_halo,
           "grads": {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None},
           "bn": {k: v.clone() for k, v in model.state_dict().items() if "running" in k}}
    tr.opt.zero_grad(set_to_none=True)
    # (1b) the input gradient without activation kinks (slope 1: LeakyReLU is the identity), mask all ones, on a copy
    #      of the model: every cross-rank term of dz1 (halo exchanges, mesh-wide BatchNorm, bounding box, loss sums)
    #      must then agree closely with the single-rank run
    import copy
    smooth = copy.deepcopy(model)
    smooth.blocks[0].module_2.negative_slope = 1.0           # ONE shared instance (util/networks.py:17-18)
    part.z1.grad = None
    tr.loss(smooth(part, torch.ones_like(part.v_keep))).backward()
    out["dz1_smooth"] = part.z1.grad.clone()
    part.z1.grad = None
    # (2) the training loop proper: two accumulated iterations, then Adam on the reduced gradients
    c0 = dict(sgdist.collective_counts)
    out["losses"] = [float(tr.iteration_step().detach())]
    out["collectives_first_iteration"] = {k: v - c0[k] for k, v in sgdist.collective_counts.items()}
    out["losses"].append(float(tr.iteration_step().detach()))
    out["params"] = {n: p.detach().clone() for n, p in model.named_parameters()}
    torch.save(out, os.path.join(out_dir, f"w{world}_r{rank}.pt"))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _launch(world, out_dir, skip, port):
    if world == 1:
        _run_rank(0, 1, port, out_dir, skip)
    else:
        mp.spawn(_run_rank, args=(world, port, out_dir, skip), nprocs=world, join=True)
    return [torch.load(os.path.join(out_dir, f"w{world}_r{r}.pt")) for r in range(world)]


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


@pytest.mark.parametrize("world,skip", [(2, False), (3, True)])
def test_partitioned_training_matches_single_rank(world, skip):
    with tempfile.TemporaryDirectory() as d:
        ref = _launch(1, d, skip, 0)[0]
        parts = _launch(world, d, skip, 29600 + world)
    assert sum(p["range"][1] - p["range"][0] for p in parts) == 384
    assert all(p["n_halo"] > 0 for p in parts)
    tie = [p["lin"]["tie_dz"] for p in parts]
    assert torch.equal(tie[0], torch.tensor([[2.0] * 3, [3.0] * 3, [0.0] * 3])) and all(float(t.abs().max()) == 0.0 for t in tie[1:])
    assert torch.equal(ref["lin"]["tie_dz"], tie[0])
    # exact pieces: partitioned ChebConv and mesh-wide BatchNorm == their single-rank results
    for key in ("conv_y", "conv_dx", "conv2_y", "conv2_dx", "bn_y", "bn_dx"):
        assert rel_l2(torch.cat([p["lin"][key] for p in parts], dim=0), ref["lin"][key]) < 2e-6, key
    for key in ("conv_dw", "conv_db", "conv2_dw", "conv2_db", "bn_dw", "bn_db", "bn_rm", "bn_rv"):
        for p in parts:
            assert rel_l2(p["lin"][key], ref["lin"][key]) < 5e-6, key
    # the general loop of the two recurrences (K != 3), both evaluation orders: the same bounds, and exactly one halo
    # exchange per aggregation -- (K - 1) per layer and pass, two layers per K, forward and backward
    for key in (f"gen_K{K}_{io}" for K in GENERAL_KS for io in ("12_20", "20_12")):
        for t in ("_y", "_dx"):
            assert rel_l2(torch.cat([p["lin"][key + t] for p in parts], dim=0), ref["lin"][key + t]) < 2e-6, key + t
        for t in ("_dw", "_db"):
            for p in parts:
                assert rel_l2(p["lin"][key + t], ref["lin"][key + t]) < 5e-6, key + t
    assert ref["lin"]["gen_all_to_all"] == 0
    for p in parts:
        assert p["lin"]["gen_all_to_all"] == 2 * sum(K - 1 for K in GENERAL_KS) * 2 == 16
    for p in parts:
        assert torch.equal(p["lin"]["mm_lo"], ref["lin"]["mm_lo"]) and torch.equal(p["lin"]["mm_hi"], ref["lin"]["mm_hi"])
    mm_dz = torch.cat([p["lin"]["mm_dz"] for p in parts], dim=0)
    assert torch.equal(mm_dz, ref["lin"]["mm_dz"]) and int((mm_dz != 0).sum()) == 6      # one arg-min and one arg-max per axis
    pos = torch.cat([p["pos"] for p in parts], dim=0)        # blocks are contiguous in processing order
    assert rel_l2(pos, ref["pos"]) < 2e-5
    dz1 = torch.cat([p["dz1_smooth"] for p in parts], dim=0)  # input gradient incl. the bounding-box terms, no LeakyReLU kinks
    assert rel_l2(dz1, ref["dz1_smooth"]) < 1e-3
    assert float(ref["dz1_smooth"].abs().max()) > 0
    gmax = max(float(v.abs().max()) for v in ref["grads"].values())
    for p in parts:
        assert abs(p["loss0"] - ref["loss0"]) < 2e-5 * abs(ref["loss0"])
        assert np.allclose(p["losses"], ref["losses"], rtol=1e-4)     # 2nd/3rd forward: BN running stats moved
        for n, g in ref["grads"].items():     # kink-limited (L1 on unit normals, LeakyReLU sign flips): see (0) for exact
            scale = max(float(g.norm()), 1e-3 * gmax * g.numel() ** 0.5)
            assert float((p["grads"][n] - g).norm()) <= 3e-2 * scale, n
        for k, v in ref["bn"].items():
            assert rel_l2(p["bn"][k], v) < 1e-5, k
        # Adam moved every parameter by <= lr; where the gradient is not rounding noise the move agrees
        for n, v in ref["params"].items():
            assert float((p["params"][n] - v).abs().max()) <= 2.5e-2, n
    for n in parts[0]["grads"]:                                # every rank holds the same reduced gradient
        assert torch.equal(parts[0]["grads"][n], parts[1]["grads"][n]), n
    # collectives of one training iteration (no optimiser step): ONE halo exchange per ChebConv forward and one per
    # backward (two-ring halo), one all-gather / all-reduce per BatchNorm forward / backward, five for bounding box
    # and losses -- VERDICT r1 counted ~130 with two exchanges per aggregation pair
    for p in parts:
        c = p["collectives_first_iteration"]
        # (the CPU loss path reduces its two masked sums separately: 13 + 2 + 2 all-reduces; the fused device loss 13 + 2 + 1)
        assert c["all_to_all"] == 13 * 2 + 2 and c["all_gather"] == 13 and c["all_reduce"] == 13 + 4, c
        assert sum(c.values()) <= 60


def test_partition_plan_is_consistent():
    _install_doubles()
    from semigcn_amd import dist as sgdist, reorder, synth
    mesh = synth.torus_mesh(48, 32, permute=True)     # (rank 0 of 4 has a ring-1 row all of whose neighbours are owned)
    V = mesh.num_vertices
    order, rank_of = reorder.morton_order(torch.from_numpy(mesh.x_pos))
    ei = reorder.permute_edge_index(torch.from_numpy(mesh.edge_index), rank_of)
    world = 4
    gs = [sgdist.DistMeshGraph(ei, V, r, world) for r in range(world)]
    assert [g.start for g in gs] == [0, 384, 768, 1152]
    for r, g in enumerate(gs):
        for q, h in enumerate(gs):
            # what r sends to q is exactly what q expects from r, in the same order
            sent = g.send_rows[sum(g.send_splits[:q]):sum(g.send_splits[:q + 1])].long() + g.start
            want = h.halo_ids[sum(h.recv_splits[:r]):sum(h.recv_splits[:r + 1])]
            assert torch.equal(sent, want), (r, q)
        assert g.send_splits[r] == 0 and g.recv_splits[r] == 0
    # the partitioned operator reproduces the global one row for row
    x = torch.randn(V, 5)
    full = sgdist.DistMeshGraph(ei, V, 0, 1)
    y_full = full.handle.spmm(x, torch.empty(V, 5))
    for g in gs:
        x_ext = torch.cat([x[g.start:g.end], x[g.halo_ids]])
        y = g.handle.spmm(x_ext, torch.empty(g.n_own, 5))
        assert torch.allclose(y, y_full[g.start:g.end], atol=1e-6)
        # the wide operator (owned + ring-1 rows) and its interior / rest halves write the same rows with the same values
        ids_ext = torch.cat([torch.arange(g.start, g.end), g.halo_ids])
        yw = g.handle_wide.spmm(x_ext, torch.zeros(g.n_ext, 5))
        ys = torch.full((g.n_ext, 5), float("nan"))
        g._split[0].spmm(x_ext, ys)
        assert g.n_interior > 0 and int(torch.isfinite(ys[:, 0]).sum()) == g.n_interior      # interior rows only
        assert not bool(torch.isfinite(ys[g.n_own:]).any())                                     # ... all of them owned
        g._split[1].spmm(x_ext, ys)
        done = torch.isfinite(ys[:, 0])
        assert int(done.sum()) == g.n_own + g.n_halo1 and bool(done[:g.n_own].all())
        assert torch.allclose(ys[done], yw[done], atol=1e-6)
        assert torch.allclose(ys[done], y_full[ids_ext[done]], atol=1e-6)                     # ring-1 rows are complete rows
    with pytest.raises(ValueError, match="symmetric"):
        sgdist.DistMeshGraph(ei[:, :-1], V, 0, 2)


# --------------------------------------------------------------------------------------
# MGCN on a partition: N ranks == 1 rank == the unpartitioned model, on the REFERENCE's own
# hierarchy (golden g3: QEM clusters of 1..5 vertices, 258 -> 154 -> 92 -> 55)
# --------------------------------------------------------------------------------------
def _run_mgcn_rank(rank, world, port, out_dir, partitioned):
    _install_doubles()
    torch.set_num_threads(1)
    if world > 1:
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    import golden_util as GU
    from test_host_logic import _mgcn_from_golden
    from semigcn_amd import dist as sgdist, train
    g3 = GU.load("g3_mgcn.npz")
    g0 = GU.load("g0_mesh_layout.npz")
    net = _mgcn_from_golden("cpu", g3, skip=True)
    GU.fill_state(net, seed=2718)
    for mod in net.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0                                   # dropout masks are per-rank random streams
    faces = torch.from_numpy(g0["sphere/faces"]).long()
    V = g3["z1"].shape[0]
    v_keep = torch.from_numpy(g3["v_masks/0"]).float()
    target_pos = torch.from_numpy(g3["poss/0"])

    class D:
        z1 = torch.from_numpy(g3["z1"])
        x_pos = None
    batch = train.MeshBatch(D, faces, target_pos, train.face_normals(target_pos, faces), v_keep,
                            (v_keep[:, 0][faces] > 0).all(1).float().view(-1, 1), torch.ones(V, 2))
    out = {}
    if partitioned:
        part = sgdist.partition_mgcn(net, rank, world)
        tr = sgdist.DistMGCNTrainer(net, part, batch, accumulate=2)
        out["bounds"], out["n_halo"] = part.bounds, [g.n_halo for g in part.graphs]
        out["pool_halo"] = [(p.fine_plan.n_halo, p.coarse_plan.n_halo) for p in part.pools]
        # the pool / unpool pair on its own, no kinks: linear in x
        gen = torch.Generator().manual_seed(9)
        xf = torch.randn(V, 6, generator=gen)
        x_own = xf[part.own_ids[0]].clone().requires_grad_(True)
        pooled = part.pools[0].pool(x_own)
        back = part.pools[0].unpool(pooled)
        (back * xf[part.own_ids[0]]).sum().backward()
        out["pool"] = sgdist.gather_level(pooled, part, 1)
        out["unpool"] = sgdist.gather_level(back, part, 0)
        out["pool_dx"] = sgdist.gather_level(x_own.grad, part, 0)
    else:
        tr = train.MGCNTrainer(net, batch, accumulate=2)
        gen = torch.Generator().manual_seed(9)
        xf = torch.randn(V, 6, generator=gen).requires_grad_(True)
        pooled = net.encoder1.model1.module_4(xf)
        back = net.decoder1[0].model1.module_1(pooled)
        (back * xf.detach()).sum().backward()
        out["pool"], out["unpool"], out["pool_dx"] = pooled.detach(), back.detach(), xf.grad.clone()
    net.eval()
    with torch.no_grad():
        ev = net(D, None)
    net.train()
    poss = net(D, None)
    loss = tr.loss(poss) if partitioned else sum(
        w * train.masked_position_rmse(p, t, k, n) for w, p, t, k, n in zip(tr.weights, poss, net.poss_list, tr.keeps, tr.counts)
    ) + tr.k1 * train.masked_normal_l1(train.face_normals(poss[0], faces), batch.target_fn, batch.f_keep, batch.n_f_keep)
    loss.backward()
    if partitioned:
        sgdist.all_reduce_gradients(tr.params)
        out["eval"] = [sgdist.gather_level(p, part, l) for l, p in enumerate(ev)]
        out["train"] = [sgdist.gather_level(p, part, l) for l, p in enumerate(poss)]
    else:
        out["eval"], out["train"] = [p.clone() for p in ev], [p.detach().clone() for p in poss]
    out["loss"] = float(loss.detach())
    out["grads"] = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    out["bn"] = {k: v.clone() for k, v in net.state_dict().items() if "running" in k}
    tr.opt.zero_grad(set_to_none=True)
    out["losses"] = [float(tr.iteration_step().detach()) for _ in range(2)]
    torch.save(out, os.path.join(out_dir, f"m{int(partitioned)}_w{world}_r{rank}.pt"))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _launch_mgcn(world, out_dir, partitioned, port):
    if world == 1:
        _run_mgcn_rank(0, 1, port, out_dir, partitioned)
    else:
        mp.spawn(_run_mgcn_rank, args=(world, port, out_dir, partitioned), nprocs=world, join=True)
    return [torch.load(os.path.join(out_dir, f"m{int(partitioned)}_w{world}_r{r}.pt")) for r in range(world)]


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_mgcn_matches_unpartitioned(world):
    with tempfile.TemporaryDirectory() as d:
        ref = _launch_mgcn(1, d, False, 0)[0]
        one = _launch_mgcn(1, d, True, 0)[0]
        parts = _launch_mgcn(world, d, True, 29700 + world)
    assert [b[-1] for b in parts[0]["bounds"]] == [258, 154, 92, 55]
    assert all(sum(h) > 0 for p in parts for h in p["pool_halo"][:2])          # clusters do span the cut
    for p in [one] + parts:
        for key in ("pool", "unpool", "pool_dx"):
            assert rel_l2(p[key], ref[key]) < 2e-6, key
        for l in range(4):
            assert rel_l2(p["eval"][l], ref["eval"][l]) < 5e-5, l       # the MGCN bar (33 layers; tests/test_gpu_parity.py)
            assert rel_l2(p["train"][l], ref["train"][l]) < 5e-5, l
        assert abs(p["loss"] - ref["loss"]) < 2e-5 * abs(ref["loss"])
        assert np.allclose(p["losses"], ref["losses"], rtol=2e-4)
        gmax = max(float(v.abs().max()) for v in ref["grads"].values())
        for n, g in ref["grads"].items():          # kink-limited, as in the SGCN test above
            scale = max(float(g.norm()), 1e-3 * gmax * g.numel() ** 0.5)
            assert float((p["grads"][n] - g).norm()) <= 3e-2 * scale, n
        for k, v in ref["bn"].items():
            assert rel_l2(p["bn"][k], v) < 1e-5, k
    for n in parts[0]["grads"]:
        assert torch.equal(parts[0]["grads"][n], parts[1]["grads"][n]), n


# --------------------------------------------------------------------------------------
# the folded layout of the phase-by-phase block path (dist.FoldedLayout; sg_block_run needs a device, its exchange plan does not)
# --------------------------------------------------------------------------------------
def _folded_layouts(world, nu=48, nv=32):
    _install_doubles()
    from semigcn_amd import dist as sgdist, reorder, synth
    mesh = synth.torus_mesh(nu, nv, permute=True)
    V = mesh.num_vertices
    order, rank_of = reorder.morton_order(torch.from_numpy(mesh.x_pos))
    ei = reorder.permute_edge_index(torch.from_numpy(mesh.edge_index), rank_of)
    gs = [sgdist.DistMeshGraph(ei, V, r, world) for r in range(world)]
    return sgdist, ei, V, gs, [g.folded() for g in gs]


def test_folded_layout_plan_is_consistent():
    """[owned | per peer: its halo rows, PAD_ROWS pad rows]: what rank r packs for peer q (send_index) is, row for row, what q
    keeps in r's segment of its buffer; the pad rows sit where stats_rows says; the two operators on the folded numbering
    reproduce the global operator on the owned rows (one hop) and on the owned + ring-1 rows (the wide one)."""
    world = 4
    sgdist, ei, V, gs, lays = _folded_layouts(world)
    P = sgdist.PAD_ROWS
    for r, (g, lay) in enumerate(zip(gs, lays)):
        assert lay.n_own == g.n_own and lay.send_splits[r] == 0 and lay.recv_splits[r] == 0
        assert lay.n_ext == g.n_own + sum(lay.recv_splits) and lay.n_send == sum(lay.send_splits)
        assert torch.equal(lay.ext_src[:g.n_own], torch.arange(g.start, g.end))
        at_recv = g.n_own
        for q in range(world):
            if q == r:
                assert int(lay.stats_rows[q]) == -1
                continue
            n_rows = lay.recv_splits[q] - P
            seg = lay.ext_src[at_recv:at_recv + lay.recv_splits[q]]
            assert n_rows >= 0 and bool((seg[:n_rows] >= gs[q].start).all()) and bool((seg[:n_rows] < gs[q].end).all())
            assert (n_rows < 2 or bool((seg[1:n_rows] > seg[:n_rows - 1]).all())) and bool((seg[n_rows:] == -1).all())
            assert int(lay.stats_rows[q]) == at_recv + n_rows
            # what q sends to r
            lq = lays[q]
            at_send = sum(lq.send_splits[:r])
            sent = lq.send_index[at_send:at_send + lq.send_splits[r]].long()
            assert lq.send_splits[r] == lay.recv_splits[q]
            assert torch.equal(sent[:n_rows] + gs[q].start, seg[:n_rows]), (r, q)
            assert torch.equal(sent[n_rows:], -1 - torch.arange(P)), (r, q)
            at_recv += lay.recv_splits[q]
    # operators: one hop on the owned rows; the wide one on every row whose neighbours all lie in the buffer (owned + ring 1)
    x = torch.randn(V, 6)
    full = sgdist.DistMeshGraph(ei, V, 0, 1)
    y_full = full.handle.spmm(x, torch.empty(V, 6))
    for g, lay in zip(gs, lays):
        idx = lay.ext_src
        x_ext = x[idx.clamp(min=0)] * (idx >= 0).view(-1, 1)
        y = lay.handle.spmm(x_ext, torch.empty(lay.n_own, 6))
        assert torch.allclose(y, y_full[g.start:g.end], atol=1e-6)
        yw = lay.handle_wide.spmm(x_ext, torch.zeros(lay.n_ext, 6))
        assert torch.allclose(yw[:lay.n_own], y_full[g.start:g.end], atol=1e-6)
        ring1 = torch.unique(ei[1][(ei[0] >= g.start) & (ei[0] < g.end)])          # sources of the owned rows
        ring1 = ring1[(ring1 < g.start) | (ring1 >= g.end)]
        pos = {int(v): i for i, v in enumerate(idx.tolist()) if v >= 0}
        rows = torch.tensor([pos[int(v)] for v in ring1.tolist()])
        assert rows.numel() > 0 and torch.allclose(yw[rows], y_full[ring1], atol=1e-6)
        # two hops with ONE exchange: Tx2 = 2 L (L x) - x on the owned rows from the wide first hop
        t2 = 2.0 * lay.handle.spmm(yw, torch.empty(lay.n_own, 6)) - x[g.start:g.end]
        want = 2.0 * full.handle.spmm(y_full, torch.empty(V, 6)) - x
        assert torch.allclose(t2, want[g.start:g.end], atol=1e-5)


def _folded_exchange_rank(rank, world, port, out_dir):
    _install_doubles()
    torch.set_num_threads(1)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sgdist, ei, V, gs, lays = _folded_layouts(world, 24, 16)
    g, lay = gs[rank], lays[rank]
    C, P = 6, sgdist.PAD_ROWS
    x = torch.randn(V, C, generator=torch.Generator().manual_seed(9))
    blob = lambda q: torch.arange(2 * C + 1, dtype=torch.float32) + 100.0 * (q + 1)       # rank q's "statistics"
    buf = torch.full((lay.n_ext, C), float("nan"))
    buf[:lay.n_own] = x[g.start:g.end]
    # what SG_PHASE_CONV's pack kernel does (csrc/block.hip pack_rows): rows by send_index, the blob across the pad rows
    pad = torch.zeros(P * C)
    pad[:2 * C + 1] = blob(rank)
    idx = lay.send_index.long()
    send = torch.where((idx >= 0).view(-1, 1), buf[idx.clamp(min=0)], pad.view(P, C)[(-1 - idx).clamp(min=0)])
    lay.exchange(buf[lay.n_own:], send)
    src = lay.ext_src
    ok_rows = torch.equal(buf[src >= 0], x[src[src >= 0]])
    ok_stats = all(torch.equal(buf[int(lay.stats_rows[q]):int(lay.stats_rows[q]) + P].reshape(-1)[:2 * C + 1], blob(q))
                   for q in range(world) if q != rank)
    torch.save({"rows": ok_rows, "stats": ok_stats, "n_halo": lay.n_ext - lay.n_own - P * (world - 1)},
               os.path.join(out_dir, f"fold_r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_folded_exchange_lands_rows_and_statistics_in_place(world):
    """ONE all-to-all per block on the folded layout, over gloo: the receive buffer is rows [n_own:] of the feature buffer
    itself, every halo row arrives at its place and every peer's statistics blob in the pad rows of that peer's segment."""
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_folded_exchange_rank, args=(world, 29650 + world, d), nprocs=world, join=True)
        res = [torch.load(os.path.join(d, f"fold_r{r}.pt")) for r in range(world)]
    assert all(r["rows"] and r["stats"] and r["n_halo"] > 0 for r in res), res
