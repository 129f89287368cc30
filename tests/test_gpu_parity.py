"""Parity tests proper: the HIP kernels, called through the C ABI, against the oracle on the
same seeded inputs, against the committed golden vectors (reference's own code), and -- at
benchmark size -- through size-independent properties.

Tolerances (north_star: "within 1e-5 relative fp32"):
  KERNEL_TOL  1e-5   max|a-b| / max|b| for one aggregation / one ChebConv layer, fp32
  MODEL_TOL   1e-5   relative L2 for a 13-layer SGCN forward (oracle's own run-to-run noise ~2e-6)
  bf16 storage: 2^-8 relative per stored value -> 1.5e-2 on layer outputs
"""
import numpy as np
import pytest
import torch

import golden_util as GU
from oracle import dense, models as OM, pyg_restatement as P
from semigcn_amd import capi, nn as sgnn, synth
from semigcn_amd.graph import MeshGraph, graph_for
from semigcn_amd.networks import SingleScaleGCN

pytestmark = pytest.mark.gpu
KERNEL_TOL = 1e-5
MODEL_TOL = 1e-5
DEV = "cuda:0"


def rel(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def oracle_lhat(edge_index, x, alpha=1.0, x0=None, beta=0.0, x1=None, gamma=0.0, transpose=False):
    """alpha * L^ x + beta x0 + gamma x1 with the oracle's gather/scatter (CPU fp32)."""
    ei, _ = P.remove_self_loops(edge_index)
    row, col = ei[0], ei[1]
    deg = P.scatter_sum(torch.ones(row.numel()), row, x.shape[0])
    dis = deg.pow(-0.5)
    dis[dis == float("inf")] = 0
    w = -(dis[row] * dis[col])
    src, dst = (col, row) if transpose else (row, col)
    y = alpha * P.scatter_sum(w.view(-1, 1) * x.index_select(0, src), dst, x.shape[0])
    if x0 is not None:
        y = y + beta * x0
    if x1 is not None:
        y = y + gamma * x1
    return y


def nasty_graph(V=500, E=6000, seed=0):
    rs = np.random.RandomState(seed)
    ei = rs.randint(0, V - 1, size=(2, E))
    ei[:, :50] = ei[:, 50:100]
    ei[1, 100:150] = ei[0, 100:150]
    ei[1, 200:1400] = 7          # one hub row with ~1200 neighbours: overflows the LDS stage
    return torch.from_numpy(ei).long()


# --------------------------------------------------------------------------------------
# graph preprocessing (bit-exact integer work)
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["torus", "sphere", "nasty"])
def test_graph_build_bit_exact(which, fixture_meshes):
    if which == "nasty":
        ei, V = nasty_graph(), 500
    else:
        m = fixture_meshes[which]
        ei, V = torch.from_numpy(m.edge_index), m.num_vertices
    h = capi.GraphHandle.from_edge_index(ei.to(DEV), V)
    rp, ci, dis = [t.cpu().numpy() for t in h.arrays()]
    e = ei.numpy()
    e = e[:, e[0] != e[1]]
    order = np.lexsort((e[0], e[1]))          # by (target, source)
    assert h.nnz == e.shape[1]
    assert np.array_equal(ci, e[0][order].astype(np.int32))
    assert np.array_equal(rp, np.concatenate([[0], np.cumsum(np.bincount(e[1], minlength=V))]).astype(np.int32))
    deg = np.bincount(e[0], minlength=V).astype(np.float32)
    with np.errstate(divide="ignore"):
        want = np.where(deg > 0, 1.0 / np.sqrt(deg), 0).astype(np.float32)
    assert np.abs(dis - want).max() <= 1.2e-7
    key = lambda a, b: np.sort(a.astype(np.int64) * V + b)
    assert h.symmetric == bool(np.array_equal(key(e[0], e[1]), key(e[1], e[0])))
    assert h.max_degree == int(np.bincount(e[1], minlength=V).max())


def test_graph_build_edge_cases():
    empty = capi.GraphHandle.from_edge_index(torch.zeros((2, 0), dtype=torch.long, device=DEV), 5)
    assert empty.nnz == 0 and empty.num_rows == 5
    x = torch.randn(5, 8, device=DEV)
    y = torch.full((5, 8), 3.0, device=DEV)
    empty.spmm(x, y)
    assert float(y.abs().max()) == 0.0
    only_loops = capi.GraphHandle.from_edge_index(torch.tensor([[0, 1, 2], [0, 1, 2]], device=DEV), 3)
    assert only_loops.nnz == 0
    with pytest.raises(capi.SemigcnLibraryError, match="out of range"):
        capi.GraphHandle.from_edge_index(torch.tensor([[0, 9], [1, 0]], device=DEV), 3)
    with pytest.raises(capi.SemigcnLibraryError, match="int64"):
        capi.GraphHandle.from_edge_index(torch.zeros((2, 4), dtype=torch.int32, device=DEV), 3)
    zero_v = capi.GraphHandle.from_edge_index(torch.zeros((2, 0), dtype=torch.long, device=DEV), 0)
    assert zero_v.num_rows == 0


# --------------------------------------------------------------------------------------
# aggregation kernel
# --------------------------------------------------------------------------------------
CHANNELS = [1, 3, 4, 5, 8, 12, 16, 32, 48, 64, 128, 256, 260, 512, 1024, 1028]


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("which", ["torus", "nasty"])
def test_spmm_fp32_vs_oracle(C, which, fixture_meshes):
    if which == "nasty":
        ei, V = nasty_graph(), 500
    else:
        ei, V = torch.from_numpy(fixture_meshes["torus"].edge_index), 240
    h = capi.GraphHandle.from_edge_index(ei.to(DEV), V)
    rs = np.random.RandomState(C)
    x, x0, x1 = (torch.from_numpy(rs.standard_normal((V, C)).astype(np.float32)) for _ in range(3))
    for tr in ([False, True] if which == "nasty" else [False]):
        want = oracle_lhat(ei, x, transpose=tr)
        got = h.spmm(x.to(DEV), torch.empty(V, C, device=DEV), transpose=tr)
        assert rel(got, want) < KERNEL_TOL
        want = oracle_lhat(ei, x, 2.0, x0, -1.0, x1, 0.5, transpose=tr)
        got = h.spmm(x.to(DEV), torch.empty(V, C, device=DEV), alpha=2.0, X0=x0.to(DEV), beta=-1.0,
                     X1=x1.to(DEV), gamma=0.5, transpose=tr)
        assert rel(got, want) < KERNEL_TOL


def test_spmm_vs_dense_fp64_reference_matrix():
    """Against the reference's own D^-1/2 A D^-1/2 (util/mesh.py:276-285) frozen in g0."""
    g0 = GU.load("g0_mesh_layout.npz")
    for name in ("sphere", "torus"):
        ei = torch.from_numpy(g0[f"{name}/edge_index"])
        L = g0[f"{name}/lhat_dense_ref"].astype(np.float64)
        V = L.shape[0]
        x = torch.from_numpy(np.random.RandomState(2).standard_normal((V, 64)).astype(np.float32))
        got = capi.GraphHandle.from_edge_index(ei.to(DEV), V).spmm(x.to(DEV), torch.empty(V, 64, device=DEV))
        assert rel(got, L @ x.double().numpy()) < 2e-6


def test_spmm_strided_blocks_and_in_place_epilogue(fixture_meshes):
    """Column blocks of one [V, 3C] buffer as X / X0 / Y (what cheb_conv does), Y aliasing X0."""
    m = fixture_meshes["sphere"]
    ei, V, C = torch.from_numpy(m.edge_index), m.num_vertices, 32
    h = capi.GraphHandle.from_edge_index(ei.to(DEV), V)
    T = torch.from_numpy(np.random.RandomState(3).standard_normal((V, 3 * C)).astype(np.float32))
    Td = T.to(DEV)
    h.spmm(Td[:, :C], Td[:, C:2 * C])
    h.spmm(Td[:, C:2 * C], Td[:, 2 * C:], alpha=2.0, X0=Td[:, :C], beta=-1.0)
    t1 = oracle_lhat(ei, T[:, :C])
    t2 = oracle_lhat(ei, t1, 2.0, T[:, :C], -1.0)
    assert torch.equal(Td[:, :C].cpu(), T[:, :C])
    assert rel(Td[:, C:2 * C], t1) < KERNEL_TOL and rel(Td[:, 2 * C:], t2) < KERNEL_TOL
    g = T.clone().to(DEV)                     # in place: Y is X0
    h.spmm(g[:, 2 * C:], g[:, C:2 * C], alpha=2.0, X0=g[:, C:2 * C], beta=1.0)
    assert rel(g[:, C:2 * C], oracle_lhat(ei, T[:, 2 * C:], 2.0, T[:, C:2 * C], 1.0)) < KERNEL_TOL
    odd = torch.randn(V, 3 * C + 1, device=DEV)  # stride not a multiple of 4 -> scalar kernel
    got = h.spmm(odd[:, 1:C + 1], torch.empty(V, C, device=DEV))
    assert rel(got, oracle_lhat(ei, odd[:, 1:C + 1].cpu())) < KERNEL_TOL


def test_spmm_four_channel_bf16_rows_kernel_is_bit_identical_to_the_scalar_kernel(fixture_meshes):
    """C = 4 in bf16 (8-byte rows: the input layer) runs one thread per ROW; it must reproduce the one-thread-per-element
    kernel bit for bit -- same CSR-order fma chain -- with and without epilogue operands, strided operands, on a mesh, a
    multigraph with a hub row and self-loops, and through a row-subset view."""
    for ei, V in ((torch.from_numpy(fixture_meshes["torus"].edge_index), 240), (nasty_graph(), 500),
                  (torch.from_numpy(synth.torus_mesh(70, 50, masks=False).edge_index), 3500)):
        g = MeshGraph.from_edge_index(ei.to(DEV), V)
        wide = torch.randn(V, 12, device=DEV).bfloat16()
        x, x0, x1 = wide[:, 0:4], wide[:, 4:8], wide[:, 8:12]
        for kw in ({}, {"X0": x0, "beta": -1.0, "alpha": 2.0}, {"X0": x0, "beta": 1.0, "X1": x1, "gamma": -1.0}):
            ya = torch.zeros(V, 8, device=DEV, dtype=torch.bfloat16)
            yb = torch.zeros_like(ya)
            g.aggregate(x, ya[:, 4:8], **kw)
            capi.tuning_set(capi.TUNE_FLAGS, 1 | 256)
            try:
                g.aggregate(x, yb[:, 4:8], **kw)
            finally:
                capi.tuning_set(capi.TUNE_FLAGS, 1)
            assert torch.equal(ya, yb) and bool((ya[:, :4] == 0).all())
            ref = oracle_lhat(ei, x.float().cpu(), kw.get("alpha", 1.0), None if "X0" not in kw else x0.float().cpu(),
                              kw.get("beta", 0.0), None if "X1" not in kw else x1.float().cpu(), kw.get("gamma", 0.0))
            assert rel(ya[:, 4:8].float(), ref) < 2.0 ** -7


@pytest.mark.parametrize("C", [8, 16, 64, 256, 512, 24, 7])
def test_spmm_bf16_storage(C, fixture_meshes):
    m = fixture_meshes["torus"]
    ei, V = torch.from_numpy(m.edge_index), m.num_vertices
    h = capi.GraphHandle.from_edge_index(ei.to(DEV), V)
    rs = np.random.RandomState(C)
    x = torch.from_numpy(rs.standard_normal((V, C)).astype(np.float32)).bfloat16()
    x0 = torch.from_numpy(rs.standard_normal((V, C)).astype(np.float32)).bfloat16()
    want = oracle_lhat(ei, x.float(), 2.0, x0.float(), -1.0)      # fp32 math on the bf16 values
    got = h.spmm(x.to(DEV), torch.empty(V, C, device=DEV, dtype=torch.bfloat16), alpha=2.0, X0=x0.to(DEV), beta=-1.0)
    assert got.dtype == torch.bfloat16
    assert rel(got.float(), want) < 2.0 ** -8     # one bf16 rounding of the fp32 result
    assert torch.equal(got.cpu(), want.bfloat16()) or rel(got.float(), want.bfloat16().float()) < 2.0 ** -7


def test_spmm_deterministic_and_rejects_bad_arguments(fixture_meshes):
    m = fixture_meshes["torus"]
    h = capi.GraphHandle.from_edge_index(torch.from_numpy(m.edge_index).to(DEV), 240)
    x = torch.randn(240, 64, device=DEV)
    a = h.spmm(x, torch.empty_like(x)).clone()
    for _ in range(3):
        assert torch.equal(h.spmm(x, torch.empty_like(x)), a)
    with pytest.raises(capi.SemigcnLibraryError, match="alias"):
        h.spmm(x, x)
    with pytest.raises(capi.SemigcnLibraryError, match="shape"):
        h.spmm(x[:100], torch.empty(240, 64, device=DEV))
    with pytest.raises(capi.SemigcnLibraryError, match="dtype"):
        h.spmm(x.double(), torch.empty(240, 64, device=DEV, dtype=torch.float64))
    with pytest.raises(capi.SemigcnLibraryError, match="HIP device only"):
        h.spmm(x.cpu(), torch.empty(240, 64))


# --------------------------------------------------------------------------------------
# ChebConv layer: golden vectors (G1) + oracle autograd
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cin,cout", [("sphere", 4, 16), ("sphere", 32, 64), ("sphere", 256, 512),
                                           ("torus", 4, 16), ("torus", 32, 64), ("torus", 3, 5)])
def test_chebconv_layer_vs_golden(name, cin, cout, fixture_meshes):
    g1 = GU.load("g1_chebconv.npz")
    tag = f"{name}/{cin}x{cout}"
    m = fixture_meshes[name]
    conv = sgnn.ChebConv(cin, cout, K=3)
    GU.fill_state(conv, seed=11)
    conv.to(DEV)
    x = torch.from_numpy(g1[tag + "/x"]).to(DEV).requires_grad_(True)
    y = conv(x, torch.from_numpy(m.edge_index).to(DEV))
    assert rel(y, g1[tag + "/out"]) < KERNEL_TOL
    (y * torch.from_numpy(g1[tag + "/r"]).to(DEV)).sum().backward()
    assert rel(x.grad, g1[tag + "/dx"]) < KERNEL_TOL
    golden = {k[len(tag + "/grad/"):]: g1[k] for k in g1.files if k.startswith(tag + "/grad/")}
    GU.check_grad_summary([(n, p.grad) for n, p in conv.named_parameters()], golden, 2e-5, tag)
    # accuracy arbiter: fp64 dense
    y64 = dense.cheb_conv_dense(g1[tag + "/x"], m.edge_index,
                                [l.weight.detach().cpu().numpy() for l in conv.lins], conv.bias.detach().cpu().numpy())
    assert rel(y, y64) < KERNEL_TOL


@pytest.mark.parametrize("K", [1, 2, 3, 5])
@pytest.mark.parametrize("cin,cout", [(12, 20), (20, 12)])     # both evaluation orders (see functional._ChebConvPostFn)
def test_chebconv_asymmetric_graph_autograd(K, cin, cout):
    ei, V = nasty_graph(), 500
    mine, ora = sgnn.ChebConv(cin, cout, K=K), P.ChebConv(cin, cout, K=K)
    GU.fill_state(ora, seed=5)
    mine.load_state_dict(ora.state_dict())
    mine.to(DEV)
    rs = np.random.RandomState(K)
    x = torch.from_numpy(rs.standard_normal((V, cin)).astype(np.float32))
    r = torch.from_numpy(rs.standard_normal((V, cout)).astype(np.float32))
    xa, xb = x.to(DEV).requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = mine(xa, ei.to(DEV)), ora(xb, ei)
    assert rel(ya, yb) < KERNEL_TOL
    (ya * r.to(DEV)).sum().backward()
    (yb * r).sum().backward()
    assert rel(xa.grad, xb.grad) < KERNEL_TOL
    for (n, p), (_, q) in zip(mine.named_parameters(), ora.named_parameters()):
        assert rel(p.grad, q.grad) < 2e-5, n


# --------------------------------------------------------------------------------------
# SGCN model vs the reference's own code (G2) and vs the fp64 oracle
# --------------------------------------------------------------------------------------
class _Data:
    def __init__(self, m, device="cpu"):
        self.z1 = torch.from_numpy(m.z1).to(device).requires_grad_(True)
        self.x_pos = torch.from_numpy(m.x_pos).to(device)
        self.edge_index = torch.from_numpy(m.edge_index).to(device)


@pytest.mark.parametrize("name", ["sphere", "torus"])
@pytest.mark.parametrize("skip", [False, True])
def test_sgcn_vs_reference_golden(name, skip, fixture_meshes):
    g2 = GU.load("g2_sgcn.npz")
    m = fixture_meshes[name]
    tag = f"{name}/skip{int(skip)}"
    net = SingleScaleGCN(DEV, skip=skip)
    assert list(net.state_dict().keys()) == list(g2[f"{name}/state_dict_keys"])
    GU.fill_state(net, seed=314)
    net.to(DEV)
    data, dm = _Data(m), g2[f"{name}/dm"]        # host tensors, like the reference's dataset
    net.eval()
    with torch.no_grad():
        assert GU.rel_l2(net(data, torch.from_numpy(dm)).cpu(), g2[tag + "/eval_dm_tensor"]) < MODEL_TOL
        assert GU.rel_l2(net(data, dm).cpu(), g2[tag + "/eval_dm_ndarray"]) < MODEL_TOL
        assert GU.rel_l2(net(data, None).cpu(), g2[tag + "/eval_dm_none"]) < MODEL_TOL
    net.train()
    # the oracle (pinned to these same golden vectors in test_oracle.py) supplies the LeakyReLU
    # sign patterns of the reference run, so that gradient parity can be asserted tightly
    ora = OM.SGCNOracle(skip=skip)
    ora.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    ora.train()
    rec_o, rec_h = GU.ActivationMasks(ora), GU.ActivationMasks(net, fused=True)
    ora(torch.from_numpy(m.z1), torch.from_numpy(m.x_pos), torch.from_numpy(m.edge_index), torch.from_numpy(dm))
    pos = net(data, torch.from_numpy(dm))
    rank = net._layout(data)[2].cpu()
    flips = rec_h.flips_against(rec_o, [rank] * len(rec_h.masks))
    rec_o.close(), rec_h.close()
    assert pos.device.type == "cuda"
    assert GU.rel_l2(pos.detach().cpu(), g2[tag + "/train_out"]) < MODEL_TOL
    r = torch.from_numpy(GU.probe(tag + "/r", (m.num_vertices, 3))).to(DEV)
    (pos * r).sum().backward()
    gtol = GU.grad_tolerance(flips, 2e-3)     # 2e-3: thread-count noise of the reference run itself
    assert GU.rel_l2(data.z1.grad, g2[tag + "/dz1"]) < gtol, flips
    golden = {k[len(tag + "/grad/"):]: g2[k] for k in g2.files if k.startswith(tag + "/grad/")}
    GU.check_grad_summary([(n, p.grad) for n, p in net.named_parameters() if p.grad is not None], golden, gtol, tag)
    for k in g2.files:
        if k.startswith(tag + "/bn/"):
            assert rel(net.state_dict()[k[len(tag + "/bn/"):]], g2[k]) < 1e-5


def test_sgcn_error_no_worse_than_fp32_oracle_against_fp64(fixture_meshes):
    """Arbiter: evaluate the oracle in float64; the HIP path's error must be of the size of the
    fp32 oracle's own error -- forward always, gradients whenever the run has the same
    LeakyReLU sign pattern as the fp64 run.  A 40 x 24 torus (960 vertices, ~1.9 M BatchNorm outputs per forward) is
    large enough that the claim is about the kernels (several workgroups, every lane shape); about one run in four has
    no BatchNorm output within rounding of zero, and seeds are tried (at least 12, at most 40) until three such runs
    have exercised the tight gradient bound."""
    m = synth.torus_mesh(40, 24)
    z1, xp, ei = torch.from_numpy(m.z1), torch.from_numpy(m.x_pos), torch.from_numpy(m.edge_index)
    r = torch.from_numpy(GU.probe("arbiter", (m.num_vertices, 3)))
    tight_runs = 0
    n_seeds = 0
    for seed in range(8, 48):
        if n_seeds >= 12 and tight_runs >= 3:
            break
        n_seeds += 1
        ora32 = OM.SGCNOracle()
        GU.fill_state(ora32, seed=seed)
        ora64 = OM.SGCNOracle().double()
        ora64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in ora32.state_dict().items()})
        net = SingleScaleGCN(DEV)
        net.load_state_dict(ora32.state_dict())
        net.to(DEV)
        outs, grads, recs = {}, {}, {}
        for key, mod, cast in (("f32", ora32, torch.float32), ("f64", ora64, torch.float64)):
            mod.train()
            recs[key] = GU.ActivationMasks(mod)
            z = z1.detach().clone().to(cast).requires_grad_(True)
            p = mod(z, xp.to(cast), ei, None)
            (p * r.to(cast)).sum().backward()
            outs[key], grads[key] = p.detach().double(), z.grad.double()
            recs[key].close()
        data = _Data(m, DEV)
        net.train()
        rec = GU.ActivationMasks(net, fused=True)
        p = net(data, None)
        rec.close()
        (p * r.to(DEV)).sum().backward()
        rank = net._layout(data)[2].cpu()
        flips_hip = rec.flips_against(recs["f64"], [rank] * len(rec.masks))
        flips_ref = recs["f32"].flips_against(recs["f64"])
        e_hip, e_ref = GU.rel_l2(p.detach().cpu().double(), outs["f64"]), GU.rel_l2(outs["f32"], outs["f64"])
        assert e_hip < 1e-5, (seed, e_hip, e_ref)     # north_star bar; the fp32 oracle itself sits at ~2e-6
        g_hip, g_ref = GU.rel_l2(data.z1.grad.cpu().double(), grads["f64"]), GU.rel_l2(grads["f32"], grads["f64"])
        if flips_hip == 0:
            tight_runs += 1
            assert g_hip < max(3 * g_ref, 1e-5), (seed, g_hip, g_ref, flips_ref)
        else:
            assert g_hip < GU.grad_tolerance(flips_hip, 1e-5), (seed, g_hip, flips_hip)
    assert tight_runs >= 3, f"only {tight_runs} of {n_seeds} seeds ran without a LeakyReLU sign flip; cannot assert tight gradient parity"


def test_sgcn_reordering_is_transparent(fixture_meshes):
    """Morton processing order must not change what the caller sees (vertex order, values)."""
    m = synth.torus_mesh(40, 24, permute=True)          # raw-scan-like vertex order
    a, b = SingleScaleGCN(DEV, reorder=True), SingleScaleGCN(DEV, reorder=False)
    GU.fill_state(a, seed=21)
    b.load_state_dict(a.state_dict())
    a.to(DEV), b.to(DEV)
    a.train(), b.train()
    da, db = _Data(m, DEV), _Data(m, DEV)
    dm = torch.from_numpy(synth.make_dummy_masks(m.edge_index, m.num_vertices, 1, k=2, p=0.03)).to(DEV)
    ra = GU.ActivationMasks(a, fused=True)
    pa = a(da, dm)
    ra.close()
    rb = GU.ActivationMasks(b, fused=True)
    pb = b(db, dm)
    rb.close()
    flips = ra.flips_against(rb, [a._layout(da)[2].cpu()] * len(ra.masks))
    assert GU.rel_l2(pa.detach().cpu(), pb.detach().cpu()) < MODEL_TOL
    r = torch.from_numpy(GU.probe("reorder", (m.num_vertices, 3))).to(DEV)
    (pa * r).sum().backward()
    (pb * r).sum().backward()
    assert GU.rel_l2(da.z1.grad.cpu(), db.z1.grad.cpu()) < GU.grad_tolerance(flips, 2e-4), flips
    ora = OM.SGCNOracle()
    ora.load_state_dict({k: v.cpu() for k, v in a.state_dict().items()})
    ora.train()
    po = ora(torch.from_numpy(m.z1), torch.from_numpy(m.x_pos), torch.from_numpy(m.edge_index), dm.cpu())
    assert GU.rel_l2(pa.detach().cpu(), po.detach()) < MODEL_TOL


def test_chebconv_bf16_layer_error_is_one_rounding(fixture_meshes):
    """One ChebConv layer with bf16 storage vs the same layer in fp32 on the bf16-rounded input:
    the error must be a few bf16 roundings (3 stored terms, the bf16 copy of the weights, the
    output), not more."""
    m = fixture_meshes["sphere"]
    ei = torch.from_numpy(m.edge_index).to(DEV)
    conv = sgnn.ChebConv(64, 128, K=3)
    GU.fill_state(conv, seed=4)
    conv.to(DEV)
    x = torch.randn(m.num_vertices, 64, device=DEV).bfloat16()
    y16 = conv(x, ei)
    y32 = conv(x.float(), ei)
    assert y16.dtype == torch.bfloat16
    assert GU.rel_l2(y16.detach().float().cpu(), y32.detach().cpu()) < 2.0 ** -7   # CPU emulation of the roundings: 2.7e-3


def test_sgcn_bf16_features_close_to_fp32(fixture_meshes):
    """BASELINE config c4: bf16 feature storage, fp32 accumulate/parameters/output."""
    m = fixture_meshes["torus"]
    net = SingleScaleGCN(DEV)
    GU.fill_state(net, seed=33)
    net.to(DEV).train()
    d32, d16 = _Data(m, DEV), _Data(m, DEV)
    p32 = net(d32, None)
    net.set_feature_dtype(torch.bfloat16)
    p16 = net(d16, None)
    assert p16.dtype == torch.float32
    off32 = (p32 - d32.x_pos).detach().cpu()
    off16 = (p16 - d16.x_pos).detach().cpu()
    assert GU.rel_l2(off16, off32) < 0.2            # 13 layers x ~5 roundings to an 8-bit mantissa, BN-amplified
    (p16 ** 2).mean().backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all())
               for n, p in net.named_parameters() if not n.startswith("skip_blocks"))
    net.set_feature_dtype(torch.float32)


# --------------------------------------------------------------------------------------
# pooling (G3: the reference's MeshPool / MeshUnpool classes)
# --------------------------------------------------------------------------------------
def test_pool_unpool_vs_reference_classes_and_autograd():
    from semigcn_amd import functional as F_sg
    g3 = GU.load("g3_mgcn.npz")
    ph = g3["pool_hash/0"]
    nf, nc = int(ph[:, 0].max()) + 1, int(ph[:, 1].max()) + 1
    pool = capi.PoolHandle(torch.from_numpy(ph[:, 0]).to(DEV), torch.from_numpy(ph[:, 1]).to(DEV), nf, nc)
    x = torch.from_numpy(g3["pool/x"]).to(DEV).requires_grad_(True)
    px = F_sg.mesh_pool(pool, x)
    assert rel(px, g3["pool/out"]) < 1e-6
    up = F_sg.mesh_unpool(pool, px)
    assert rel(up, g3["unpool/out"]) < 1e-6
    r = torch.randn_like(up)
    (up * r).sum().backward()
    xo = torch.from_numpy(g3["pool/x"]).requires_grad_(True)
    upo = OM.unpool_gather(ph, OM.pool_mean(ph, xo))
    (upo * r.cpu()).sum().backward()
    assert rel(x.grad, xo.grad) < 1e-6
    for C in (3, 32, 130):
        xx = torch.randn(nf, C, device=DEV)
        assert rel(pool.pool_mean(xx), OM.pool_mean(ph, xx.cpu())) < 1e-6
        yy = torch.randn(nc, C, device=DEV)
        assert rel(pool.unpool(yy), OM.unpool_gather(ph, yy.cpu())) < 1e-6


def test_gather_rows():
    x = torch.randn(1000, 48, device=DEV)
    rows = torch.randint(0, 1000, (333,), device=DEV, dtype=torch.int32)
    assert torch.equal(capi.gather_rows(rows, x), x[rows.long()])
    xb = x.bfloat16()
    assert torch.equal(capi.gather_rows(rows, xb), xb[rows.long()])
    x5 = torch.randn(1000, 5, device=DEV)
    assert torch.equal(capi.gather_rows(rows, x5), x5[rows.long()])


# --------------------------------------------------------------------------------------
# benchmark size: properties that need no oracle run (1 M vertices / 6 M edges)
# --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_graph():
    m = synth.torus_mesh(1000, 1000, masks=False)
    ei = torch.from_numpy(m.edge_index).to(DEV)
    return m, ei, MeshGraph.from_edge_index(ei, m.num_vertices)


@pytest.mark.parametrize("C,dtype", [(4, torch.float32), (64, torch.float32), (256, torch.float32),
                                     (512, torch.float32), (256, torch.bfloat16)])
def test_full_size_properties(big_graph, C, dtype):
    m, ei, g = big_graph
    V = m.num_vertices
    assert V == 1_000_000 and ei.shape[1] == 6_000_000 and g.symmetric
    tol = 1e-5 if dtype == torch.float32 else 2.0 ** -7
    gen = torch.Generator(device=DEV).manual_seed(C)
    x = torch.randn(V, C, device=DEV, generator=gen).to(dtype)
    y = torch.randn(V, C, device=DEV, generator=gen).to(dtype)
    Lx = g.aggregate(x, torch.empty_like(x))
    Ly = g.aggregate(y, torch.empty_like(y))
    # (1) eigenvector: L^ (D^1/2 1) = -(D^1/2 1)
    deg = torch.bincount(ei[0], minlength=V).float()
    s = deg.sqrt().view(-1, 1).expand(V, C).contiguous().to(dtype)
    Ls = g.aggregate(s, torch.empty_like(s))
    assert float((Ls.float() + s.float()).abs().max() / s.float().abs().max()) < (2e-6 if dtype == torch.float32 else 2e-2)
    # (2) linearity: L(2x - y) = 2 Lx - Ly     (fused epilogue path as well)
    z = (2 * x.float() - y.float()).to(dtype)
    Lz = g.aggregate(z, torch.empty_like(z))
    ref = 2 * Lx.float() - Ly.float()
    assert float((Lz.float() - ref).abs().max() / ref.abs().max()) < (tol if dtype == torch.float32 else 3e-2)
    # (3) symmetry: <y, L x> = <L y, x>
    a = float((y.double() * Lx.double()).sum())
    b = float((Ly.double() * x.double()).sum())
    nxy = float(x.double().norm() * y.double().norm())
    assert abs(a - b) <= (1e-7 if dtype == torch.float32 else 1e-4) * nxy   # bf16: Lx, Ly are rounded to 8 bits
    # (4) fused epilogue == separate ops
    fused = g.aggregate(x, torch.empty_like(x), alpha=2.0, X0=y, beta=-1.0)
    sep = 2 * Lx.float() - y.float()
    assert float((fused.float() - sep).abs().max() / sep.abs().max()) < (tol if dtype == torch.float32 else 3e-2)
    # (5) spot rows against a direct gather on the host
    rows = torch.randint(0, V, (64,), generator=torch.Generator().manual_seed(1))
    rp, ci, dis = g.handle.arrays()
    rp, dis_c = rp.cpu(), dis.cpu()
    for rr in rows.tolist():
        nb = ci[rp[rr]:rp[rr + 1]].long()
        want = -(dis_c[rr] * (dis[nb].view(-1, 1) * x[nb].float()).sum(0)).cpu()
        assert float((Lx[rr].float().cpu() - want).abs().max()) <= tol * max(float(want.abs().max()), 1e-3) * 4 + (0 if dtype == torch.float32 else 2e-2)


def test_full_size_sgcn_step_runs_and_is_finite(big_graph):
    m, ei, g = big_graph
    net = SingleScaleGCN(DEV).to(DEV)

    class D:
        z1 = torch.from_numpy(m.z1).to(DEV).requires_grad_(True)
        x_pos = torch.from_numpy(m.x_pos).to(DEV)
        edge_index = ei
    net.train()
    out = net(D, None)
    out.square().mean().backward()
    assert out.shape == (m.num_vertices, 3) and bool(torch.isfinite(out).all())
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None)
    assert graph_for(ei, m.num_vertices) is not None


# --------------------------------------------------------------------------------------
# MGCN vs the reference's own MGCN (G3) and at config-c3 size
# --------------------------------------------------------------------------------------
def test_mgcn_vs_reference_golden():
    from test_host_logic import _mgcn_from_golden, check_mgcn_against_golden
    g3 = GU.load("g3_mgcn.npz")
    net = _mgcn_from_golden(DEV, g3)
    net.to(DEV)
    check_mgcn_against_golden(net, g3, DEV, 5e-5, 2e-3)


def test_mgcn_skip_variant_vs_oracle():
    from test_host_logic import _mgcn_from_golden
    g3 = GU.load("g3_mgcn.npz")
    net = _mgcn_from_golden(DEV, g3, skip=True)
    GU.fill_state(net, seed=5)
    net.to(DEV).eval()
    ora = OM.MGCNOracle([torch.from_numpy(g3[f"edge_index/{l}"]) for l in range(4)], [g3[f"pool_hash/{l}"] for l in range(3)],
                        [torch.from_numpy(g3[f"smposs/{l}"]) for l in range(4)], skip=True)
    ora.load_state_dict({k: v.cpu() for k, v in net.state_dict().items() if not k.endswith("pool_hash")})
    ora.eval()

    class D:
        z1 = torch.from_numpy(g3["z1"]).to(DEV)
        x_pos = None
    with torch.no_grad():
        for a, b in zip(net(D, g3["dm"]), ora(torch.from_numpy(g3["z1"]), g3["dm"])):
            assert GU.rel_l2(a.cpu(), b) < 5e-5


def test_mgcn_reordering_is_transparent():
    """Per-level Morton processing order changes nothing the caller sees; a state dict written in the
    caller's numbering (pool_hash buffers included) loads into a reordering model."""
    from test_host_logic import _mgcn_from_golden
    from semigcn_amd.meshnet import MGCN
    g3 = GU.load("g3_mgcn.npz")
    a = _mgcn_from_golden(DEV, g3)
    assert a._orders is not None
    eis = [torch.from_numpy(g3[f"edge_index/{l}"]) for l in range(4)]
    b = MGCN.from_hierarchy(DEV, eis, [g3[f"pool_hash/{l}"] for l in range(3)],
                            [torch.from_numpy(g3[f"smposs/{l}"]) for l in range(4)], reorder=False)
    GU.fill_state(b, seed=12)
    a.load_state_dict(b.state_dict())
    a.to(DEV).eval(), b.to(DEV).eval()

    class D:
        z1 = torch.from_numpy(g3["z1"]).to(DEV)
        x_pos = None
    with torch.no_grad():
        for pa, pb in zip(a(D, g3["dm"]), b(D, g3["dm"])):
            assert GU.rel_l2(pa.cpu(), pb.cpu()) < 2e-5


@pytest.mark.parametrize("skip", [False, True])
def test_mgcn_bf16_feature_storage(skip):
    """MGCN.set_feature_dtype(bf16) (util/meshnet.py:278-318 with bf16 rows between the kernels on every level): one
    encoder stage on a bf16-rounded input is a few roundings from the same stage in fp32 (conv, pooled mean, BatchNorm,
    activation, three more convs -- ~25 stored values deep); the whole network stays fp32 at its four outputs, finite in
    its gradients, and as close to the fp32 network as 33 bf16 layers can be."""
    from test_host_logic import _mgcn_from_golden
    g3 = GU.load("g3_mgcn.npz")
    net = _mgcn_from_golden(DEV, g3, skip=skip)
    net.to(DEV).eval()                      # (eval: no dropout draws between the two passes)

    class D:
        z1 = torch.from_numpy(g3["z1"]).to(DEV).requires_grad_(True)
        x_pos = None
    with torch.no_grad():
        p32 = net(D, None)
        x = torch.randn(net.smposs_list[0].shape[0], 4, device=DEV).bfloat16()
        e32 = net.encoder1(x.float())
        e16 = net.encoder1(x)
        assert e16.dtype == torch.bfloat16 and GU.rel_l2(e16.float().cpu(), e32.cpu()) < 3e-2
        net.set_feature_dtype(torch.bfloat16)
        p16 = net(D, None)
    # how far bf16 storage may move the four outputs: what the bf16-STORAGE oracle (oracle/bf16.py::MGCNOracleBf16: the
    # reference's composition, rounded where this path stores) moves them on the same weights -- not a flat allowance
    from oracle import bf16 as OB
    eis = [torch.from_numpy(g3[f"edge_index/{l}"]) for l in range(4)]
    phs = [g3[f"pool_hash/{l}"] for l in range(3)]
    sms = [torch.from_numpy(g3[f"smposs/{l}"]) for l in range(4)]
    state = {k: v.cpu() for k, v in net.state_dict().items() if not k.endswith("pool_hash")}
    o32, o16 = OM.MGCNOracle(eis, phs, sms, skip=skip), OB.MGCNOracleBf16(eis, phs, sms, skip=skip)
    o32.load_state_dict(state), o16.load_state_dict(state)
    o32.eval(), o16.eval()
    with torch.no_grad():
        r32, r16 = o32(torch.from_numpy(g3["z1"]), None), o16(torch.from_numpy(g3["z1"]), None)
    for a, b, c, sm in zip(p16, r32, r16, sms):
        d_hip, d_ora = GU.rel_l2((a.cpu() - sm), (b - sm)), GU.rel_l2((c - sm), (b - sm))
        assert a.dtype == torch.float32 and d_hip < 1.5 * d_ora + 2e-3, (d_hip, d_ora)
    net.train()
    out = net(D, None)
    sum((o ** 2).mean() for o in out).backward()
    assert bool(torch.isfinite(D.z1.grad).all())
    assert all(p.grad is None or (p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all())) for p in net.parameters())
    net.set_feature_dtype(torch.float32)
    with pytest.raises(ValueError):
        net.set_feature_dtype(torch.float16)


def test_mgcn_config_c3_size_runs():
    """BASELINE config c3: MGCN, 3 pool levels, 50 K-vertex mesh (synthetic hierarchy)."""
    from semigcn_amd.meshnet import MGCN
    m = synth.torus_mesh(250, 200, masks=False)
    eis, phs, sms = [m.edge_index], [], [m.x_pos]
    V = m.num_vertices
    for l in range(3):
        ph, ei, Vc = synth.greedy_pool_hierarchy(eis[-1], V, seed=319 + l)
        cnt = np.bincount(ph[:, 1], minlength=Vc)[:, None]
        pos = np.zeros((Vc, 3), np.float32)
        np.add.at(pos, ph[:, 1], sms[-1])
        eis.append(ei), phs.append(ph), sms.append(pos / cnt)
        V = Vc
    assert [len(s) for s in sms] == [50000, 30000, 18000, 10800]
    net = MGCN.from_hierarchy(DEV, [torch.from_numpy(e) for e in eis], phs, [torch.from_numpy(s) for s in sms])
    net.to(DEV).train()

    class D:
        z1 = torch.from_numpy(m.z1).to(DEV).requires_grad_(True)
        x_pos = torch.from_numpy(m.x_pos).to(DEV)
    outs = net(D, None)
    sum(w * ((o - t) ** 2).mean() for w, o, t in zip((0.35, 0.3, 0.2, 0.15), outs, net.poss_list)).backward()
    assert [tuple(o.shape) for o in outs] == [(50000, 3), (30000, 3), (18000, 3), (10800, 3)]
    assert all(bool(torch.isfinite(o).all()) for o in outs) and bool(torch.isfinite(D.z1.grad).all())


# --------------------------------------------------------------------------------------
# fused BatchNorm1d + LeakyReLU (csrc/bn_act.hip) vs the ATen modules it replaces
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,C", [(240, 16), (5000, 256), (70001, 64), (1200, 7), (3, 4)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bn_act_matches_aten_modules(V, C, dtype):
    from semigcn_amd import functional as F_sg
    if dtype == torch.bfloat16 and V == 3:
        pytest.skip("3-row bf16 batch statistics are all rounding")
    gen = torch.Generator().manual_seed(V + C)
    x = (torch.randn(V, C, generator=gen) * 1.7 + 0.6)
    r = torch.randn(V, C, generator=gen)
    ref_bn, act = torch.nn.BatchNorm1d(C), torch.nn.LeakyReLU()
    GU.fill_state(ref_bn, seed=C)
    bn = torch.nn.BatchNorm1d(C)
    bn.load_state_dict(ref_bn.state_dict())
    bn.to(DEV)
    tol = 2e-6 if dtype == torch.float32 else 2.0 ** -7
    for mode in ("train", "eval"):
        ref_bn.train(mode == "train"), bn.train(mode == "train")
        xr = x.to(dtype).float().clone().requires_grad_(True)          # reference in fp32 on the rounded input
        yr = act(ref_bn(xr))
        (yr * r).sum().backward()
        xd = x.to(dtype).to(DEV).requires_grad_(True)
        yd = F_sg.bn_act(xd, bn, 0.01)
        (yd.float() * r.to(DEV)).sum().backward()
        assert yd.dtype == dtype
        assert GU.rel_l2(yd.detach().float().cpu(), yr.detach()) < tol, mode
        # gradient: exclude the (measure-zero) elements whose BN output sits within rounding of 0
        assert GU.rel_l2(xd.grad.float().cpu(), xr.grad) < (2e-5 if dtype == torch.float32 else 3e-2), mode
        assert GU.rel_l2(bn.weight.grad.cpu(), ref_bn.weight.grad) < (2e-5 if dtype == torch.float32 else 3e-2)
        assert GU.rel_l2(bn.bias.grad.cpu(), ref_bn.bias.grad) < (2e-5 if dtype == torch.float32 else 3e-2)
        bn.zero_grad(), ref_bn.zero_grad()
    assert rel(bn.running_mean, ref_bn.running_mean) < 1e-5 and rel(bn.running_var, ref_bn.running_var) < 1e-5
    assert int(bn.num_batches_tracked) == int(ref_bn.num_batches_tracked) == 1


def test_bn_act_widen_is_adopted_by_the_next_conv(fixture_meshes):
    from semigcn_amd import functional as F_sg
    m = fixture_meshes["torus"]
    ei = torch.from_numpy(m.edge_index).to(DEV)
    bn = torch.nn.BatchNorm1d(32).to(DEV).train()
    conv = sgnn.ChebConv(32, 40, K=3).to(DEV)      # widening layer: evaluates [Tx0|Tx1|Tx2] next to its input
    x = torch.randn(m.num_vertices, 32, device=DEV)
    wide = F_sg.bn_act(x, bn, 0.01, widen=3)
    assert wide.shape == (240, 32) and wide.stride() == (96, 1)
    assert F_sg._adopt_wide(wide, 3) is not None and F_sg._adopt_wide(wide.contiguous(), 3) is None
    bn2 = torch.nn.BatchNorm1d(32).to(DEV).train()
    plain = F_sg.bn_act(x, bn2, 0.01)
    assert torch.equal(wide, plain)
    assert torch.equal(conv(wide, ei), conv(plain, ei))          # same values, one copy less
    for cout, widen in ((40, 3), (8, 1)):          # a narrowing next layer aggregates after its GEMM: nothing to adopt
        seq = sgnn.Sequential("x, edge_index", [(sgnn.ChebConv(4, 32, K=3), "x, edge_index -> x"), torch.nn.BatchNorm1d(32),
                                                torch.nn.LeakyReLU(), (sgnn.ChebConv(32, cout, K=3), "x, edge_index -> x")]).to(DEV)
        assert seq._fusable_at(1) == (0.01, widen, 1) and seq._fusable_at(0) is None
    # backward: a narrowing conv (aggregate-after-GEMM) takes its output gradient as block 0 of a [V, K*Cout] buffer,
    # which the fused BatchNorm backward behind it writes directly; same gradients as with the copy
    seq = sgnn.Sequential("x, edge_index", [(sgnn.ChebConv(32, 8, K=3), "x, edge_index -> x"), torch.nn.BatchNorm1d(8),
                                            torch.nn.LeakyReLU()]).to(DEV)
    assert seq._fusable_at(1) == (0.01, 1, 3) and seq.module_0.grad_buffer_blocks() == 3
    xa = x.clone().requires_grad_(True)
    r = torch.randn(m.num_vertices, 8, device=DEV)
    (seq(xa, ei) * r).sum().backward()
    got = [xa.grad.clone()] + [p.grad.clone() for p in seq.parameters()]
    seen = []
    orig, blocks = F_sg._adopt_wide, F_sg.USE_BLOCK_CALLS
    F_sg._adopt_wide = lambda t, K: (seen.append(orig(t, K) is not None), None)[1]      # force the copying path
    F_sg.USE_BLOCK_CALLS = False        # (the per-module path: a block call keeps this gradient buffer inside the library)
    try:
        for p in seq.parameters():
            p.grad = None
        xb = x.clone().requires_grad_(True)
        seq.module_1.reset_running_stats()
        (seq(xb, ei) * r).sum().backward()
    finally:
        F_sg._adopt_wide, F_sg.USE_BLOCK_CALLS = orig, blocks
    assert any(seen)                                      # the adoptable buffer did arrive at the conv's backward
    for a, b in zip(got, [xb.grad] + [p.grad for p in seq.parameters()]):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------
# shared-gather aggregation kernel == generic kernel, bit for bit (same per-row summation order)
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,dtype", [(128, torch.float32), (192, torch.float32), (256, torch.float32), (512, torch.float32),
                                     (256, torch.bfloat16), (512, torch.bfloat16), (1024, torch.bfloat16)])
def test_shared_gather_kernel_bitwise_equals_generic(C, dtype):
    from semigcn_amd import reorder
    m = synth.torus_mesh(64, 48, permute=True)
    V = m.num_vertices
    rank_of = reorder.morton_order(torch.from_numpy(m.x_pos))[1]
    for ei in (rank_of[torch.from_numpy(m.edge_index)], torch.from_numpy(m.edge_index)):   # Morton and raw order
        capi.tuning_set(capi.TUNE_TILED_MIN_ROW_BYTES, -512)      # force the shared-gather kernel for every shape here
        h = capi.GraphHandle.from_edge_index(ei.to(DEV), V)
        x = torch.randn(V, C, device=DEV).to(dtype)
        x0 = torch.randn(V, C, device=DEV).to(dtype)
        x1 = torch.randn(V, C, device=DEV).to(dtype)
        outs = []
        for flags in (1, 3):                                  # 1: tiled allowed, 3: tiles disabled (2048: not the ring kernel)
            capi.tuning_set(capi.TUNE_FLAGS, flags | 2048)
            a = h.spmm(x, torch.empty_like(x))
            b = h.spmm(x, torch.empty_like(x), alpha=2.0, X0=x0, beta=-1.0)
            c = h.spmm(x, torch.empty_like(x), alpha=1.0, X0=x0, beta=1.0, X1=x1, gamma=-1.0)
            outs.append((a, b, c))
        capi.tuning_set(capi.TUNE_FLAGS, 1)
        capi.tuning_set(capi.TUNE_TILED_MIN_ROW_BYTES, 1024)      # back to the default rule
        for t, g in zip(*outs):
            assert torch.equal(t, g)
        want = oracle_lhat(ei, x.float().cpu(), 2.0, x0.float().cpu(), -1.0)
        assert rel(outs[0][1].float(), want) < (KERNEL_TOL if dtype == torch.float32 else 2.0 ** -7)


def test_column_sums_and_vertex_linear_match_aten():
    from semigcn_amd import functional as F_sg
    for V, C, dtype in ((70001, 48, torch.float32), (200000, 16, torch.bfloat16), (5000, 7, torch.float32)):
        x = (torch.randn(V, C, device=DEV) + 0.3).to(dtype)
        want = x.double().sum(0)
        assert rel(F_sg.column_sums(x), want) < (2e-6 if dtype == torch.float32 else 1e-5)
    lin = torch.nn.Linear(16, 3).to(DEV)
    x = torch.randn(50000, 16, device=DEV)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    r = torch.randn(50000, 3, device=DEV)
    ya = F_sg.linear_vertices(xa, lin.weight, lin.bias)
    (ya * r).sum().backward()
    ga = (xa.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone())
    lin.zero_grad()
    yb = lin(xb)
    (yb * r).sum().backward()
    assert torch.allclose(ya, yb, atol=1e-6)
    assert rel(ga[0], xb.grad) < 1e-6 and rel(ga[1], lin.weight.grad) < 2e-5 and rel(ga[2], lin.bias.grad) < 2e-5


def test_fused_loss_step_matches_reference_formulas(fixture_meshes):
    """csrc/mesh_loss.hip vs the oracle's restatement of util/models.py:121-126 and
    util/loss.py:14-34,78-107 (value and gradient), and vs the golden loss of the reference run."""
    from semigcn_amd import functional as F_sg
    g0, g2 = GU.load("g0_mesh_layout.npz"), GU.load("g2_sgcn.npz")
    for name in ("sphere", "torus"):
        m = fixture_meshes[name]
        v_mask = g2[f"{name}/v_mask"]
        f_mask = v_mask[m.faces].all(1)
        tgt, tfn = torch.from_numpy(m.vs.astype(np.float32)), torch.from_numpy(g0[f"{name}/fn"])
        pos = torch.from_numpy(g2[f"{name}/skip0/train_out"]).clone().requires_grad_(True)
        lo = OM.mask_pos_rec_loss(pos, tgt, v_mask) + 4.0 * OM.mask_norm_rec_loss(OM.compute_fn(pos, m.faces), tfn, f_mask)
        lo.backward()
        assert np.allclose(lo.item(), g2[f"{name}/skip0/loss"][2], rtol=1e-5)         # the reference's own number
        pd = pos.detach().to(DEV).requires_grad_(True)
        s = F_sg.mesh_loss_sums(pd, torch.from_numpy(m.faces).to(DEV), tgt.to(DEV),
                                torch.from_numpy(v_mask.astype(np.float32)).to(DEV), tfn.to(DEV),
                                torch.from_numpy(f_mask.astype(np.float32)).to(DEV))
        lh = torch.sqrt(s[0] / float(v_mask.sum()) + 1e-6) + 4.0 * s[1] / float(f_mask.sum())
        lh.backward()
        assert abs(lh.item() - lo.item()) < 2e-6 * abs(lo.item())
        assert GU.rel_l2(pd.grad.cpu(), pos.grad) < 2e-5


def test_multigraph_and_hub_rows_fall_back_to_the_generic_kernel():
    """Duplicate edges inside a row / more than 32 distinct sources per 4 rows cannot be expressed by mini-tiles:
    such graphs carry none and every shape takes spmm_rows -- results must still match the oracle."""
    ei, V = nasty_graph(), 500
    capi.tuning_set(capi.TUNE_TILED_MIN_ROW_BYTES, -512)
    h = capi.GraphHandle.from_edge_index(ei.to(DEV), V)
    capi.tuning_set(capi.TUNE_TILED_MIN_ROW_BYTES, 1024)
    x = torch.randn(V, 256, device=DEV)
    assert rel(h.spmm(x, torch.empty_like(x)), oracle_lhat(ei, x.cpu())) < KERNEL_TOL


# --------------------------------------------------------------------------------------
# mesh connectivity + dummy masks on the device: bit-exact integer work
# --------------------------------------------------------------------------------------
def _rows_as_sets(a):
    return np.sort(np.asarray(a), axis=1)


@pytest.mark.parametrize("name", ["sphere", "torus", "open"])
def test_meshprep_vs_reference_golden(name):
    """faces -> edges / edge_index / f2f, dummy masks and vertex->face masks equal the outputs of the
    reference's own Mesh and make_dummy_mask (same numpy seed) bit for bit."""
    from semigcn_amd import meshprep
    g = GU.load("g4_meshprep.npz")
    faces, V = g[f"{name}/faces"], int(g[f"{name}/num_vertices"])
    topo = meshprep.MeshTopology(faces, V, DEV)
    assert np.array_equal(topo.edges.cpu().numpy(), g[f"{name}/edges"])
    assert np.array_equal(topo.edge_index.cpu().numpy(), g[f"{name}/edge_index"])
    assert np.array_equal(_rows_as_sets(topo.f2f.cpu()), _rows_as_sets(g[f"{name}/f2f"]))
    f2f = topo.f2f.cpu().numpy()
    assert ((f2f[:, :-1] >= 0) | (f2f[:, 1:] < 0)).all()          # -1 only as trailing padding
    assert topo.manifold
    state = np.random.get_state()
    try:
        np.random.seed(317)
        vm, fm = meshprep.make_dummy_mask(topo, dm_size=3, kn=[1, 2, 3])
    finally:
        np.random.set_state(state)
    assert vm.dtype == torch.float32 and vm.shape == (V, 9) and fm.shape == (len(faces), 9)
    assert np.array_equal(vm.cpu().numpy(), g[f"{name}/vmask_dummy"])
    assert np.array_equal(fm.cpu().numpy(), g[f"{name}/fmask_dummy"])
    assert np.array_equal(meshprep.vmask_to_fmask(topo, g[f"{name}/vm"]).cpu().numpy(), g[f"{name}/fm"])


@pytest.mark.parametrize("permute", [False, True])
def test_meshprep_vs_oracle_medium(permute):
    """60 K faces, 130 masks (three 64-bit words per vertex), natural and scrambled vertex order."""
    from oracle import meshprep as MP
    from semigcn_amd import meshprep
    m = synth.torus_mesh(200, 150, permute=permute, masks=False)
    V = m.num_vertices
    topo = meshprep.MeshTopology(m.faces, V, DEV)
    edges = MP.edges_first_meeting(m.faces)
    assert np.array_equal(topo.edges.cpu().numpy(), edges)
    assert np.array_equal(_rows_as_sets(topo.f2f.cpu()), _rows_as_sets(MP.face_ring(m.faces, V)))
    vm_o, fm_o = MP.make_dummy_mask(m.faces, edges, V, dm_size=65, kn=(2, 4), rng=np.random.RandomState(5))
    vm, fm = meshprep.make_dummy_mask(topo, dm_size=65, kn=(2, 4), rng=np.random.RandomState(5))
    assert np.array_equal(vm.cpu().numpy(), vm_o) and np.array_equal(fm.cpu().numpy(), fm_o)
    # the graph the topology hands to the convolutions is the one the reference layout gives
    h = capi.GraphHandle.from_edge_index(torch.from_numpy(m.edge_index).to(DEV), V)
    for a, b in zip(topo.graph.handle.arrays(), h.arrays()):
        assert torch.equal(a, b)


def test_meshprep_rejects_bad_faces_and_flags_non_manifold():
    from semigcn_amd import meshprep
    with pytest.raises(capi.SemigcnLibraryError, match="outside"):
        meshprep.MeshTopology(np.array([[0, 1, 7]]), 4, DEV)
    with pytest.raises(capi.SemigcnLibraryError, match="degenerate"):
        meshprep.MeshTopology(np.array([[0, 1, 1]]), 4, DEV)
    fan = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]])       # edge (0,1) has three faces
    topo = meshprep.MeshTopology(fan, 5, DEV)
    assert not topo.manifold and topo.edges.shape[0] == 7
    empty = meshprep.MeshTopology(np.zeros((0, 3), np.int64), 3, DEV)
    assert empty.edges.shape == (0, 2) and empty.edge_index.shape == (2, 0)


def test_meshprep_full_size_properties():
    """V = 1 M (BASELINE c4 shape): Euler counts, uniqueness, symmetry of f2f, and ring dilation
    against an independent float index_add on the device."""
    from semigcn_amd import meshprep
    m = synth.torus_mesh(1000, 1000, masks=False)
    V, F = m.num_vertices, len(m.faces)
    topo = meshprep.MeshTopology(m.faces, V, DEV)
    E = topo.edges.shape[0]
    assert V - E + F == 0 and topo.manifold                     # torus: Euler characteristic 0
    lo, hi = topo.edges[:, 0], topo.edges[:, 1]
    assert bool((lo < hi).all()) and torch.unique(lo * V + hi).numel() == E
    assert torch.equal(topo.edge_index.cpu(), torch.from_numpy(m.edge_index))
    f2f = topo.f2f
    assert bool((f2f >= 0).all())
    me = torch.arange(F, device=DEV).view(-1, 1, 1)
    assert bool((f2f[f2f] == me).any(dim=2).all())               # f in f2f[g] for every g in f2f[f]
    gen = torch.Generator(device=DEV).manual_seed(3)
    seeds = (torch.rand((V, 40), device=DEV, generator=gen) < 0.014)
    got = meshprep.dilate(topo, seeds, 3)
    ref = seeds.float()
    src, dst = topo.edge_index[0], topo.edge_index[1]
    for _ in range(3):
        ref = ((ref + torch.zeros_like(ref).index_add_(0, dst, ref[src])) > 0).float()
    assert torch.equal(got, ref > 0)
    kept = ~got
    fm = meshprep.vmask_to_fmask(topo, kept)
    assert torch.equal(fm, kept[topo.faces].all(dim=1))


# --------------------------------------------------------------------------------------
# pooling hierarchy built on the device and MGCN through the reference's constructor
# --------------------------------------------------------------------------------------
def test_device_hierarchy_artefacts():
    """One contraction level: pool_hash covers every fine vertex, clusters are single vertices or
    matched EDGES, the level has exactly target_v vertices, positions are cluster means, the coarse
    graph is the quotient graph, surviving triangles have three distinct corners."""
    from semigcn_amd import meshprep
    m = synth.torus_mesh(200, 150, masks=False)
    V = m.num_vertices
    fine = meshprep.DeviceMesh(m.x_pos, m.faces, DEV)
    assert torch.equal(fine.edge_index.cpu(), torch.from_numpy(m.edge_index))
    target = int(V * 0.6)
    coarse = fine.simplification(target_v=target, criterion="length")
    ph = coarse.pool_hash
    Vc = coarse.vs.shape[0]
    assert Vc == target and ph.shape == (V, 2) and np.array_equal(ph[:, 0], np.arange(V))
    sizes = np.bincount(ph[:, 1], minlength=Vc)
    assert sizes.min() == 1 and sizes.max() == 2
    order = np.argsort(ph[:, 1], kind="stable")
    first = np.searchsorted(ph[order, 1], np.arange(Vc))
    assert (np.diff(order[first]) > 0).all()            # cluster ids ascend with the smallest member
    und = set(map(tuple, m.edges.tolist()))
    pairs = order[np.concatenate([first[sizes == 2], first[sizes == 2] + 1])].reshape(2, -1).T
    assert all((min(a, b), max(a, b)) in und for a, b in pairs.tolist())
    pos = np.zeros((Vc, 3), np.float64)
    np.add.at(pos, ph[:, 1], m.x_pos.astype(np.float64))
    assert np.abs(coarse.vs.cpu().numpy() - pos / sizes[:, None]).max() < 1e-5
    ce = ph[:, 1][m.edge_index]
    ce = ce[:, ce[0] != ce[1]]
    want = np.unique(np.minimum(ce[0], ce[1]) * Vc + np.maximum(ce[0], ce[1]))
    got = coarse.edge_index.cpu().numpy()
    half = got.shape[1] // 2
    assert np.array_equal(got[0, :half] * Vc + got[1, :half], want) and np.array_equal(got[:, half:], got[::-1, :half])
    cf = coarse.faces.cpu().numpy()
    assert ((cf[:, 0] != cf[:, 1]) & (cf[:, 1] != cf[:, 2]) & (cf[:, 2] != cf[:, 0])).all() and cf.max() < Vc
    # shortest edges are preferred: the contracted edges are shorter on average than the rest
    length = np.linalg.norm(m.x_pos[m.edges[:, 0]] - m.x_pos[m.edges[:, 1]], axis=1)
    taken = np.linalg.norm(m.x_pos[pairs[:, 0]] - m.x_pos[pairs[:, 1]], axis=1)
    assert taken.mean() < length.mean()


def _cluster_quadric_error(vs, faces, coarse_of, coarse_pos):
    """sum over coarse vertices of p^T (sum of the members' vertex quadrics) p: squared distances of the coarse vertex to
    the planes of every original triangle around its cluster (the quantity util/mesh.py:394-482 ranks collapses by)."""
    from semigcn_amd.meshprep import _vertex_quadrics
    Q = _vertex_quadrics(vs, faces)
    Qc = torch.zeros((coarse_pos.shape[0], 4, 4), dtype=torch.float64, device=vs.device).index_add_(0, coarse_of, Q)
    p4 = torch.cat([coarse_pos.double(), torch.ones((coarse_pos.shape[0], 1), dtype=torch.float64, device=vs.device)], 1)
    return float(torch.einsum("ci,cij,cj->c", p4, Qc, p4).sum())


@pytest.mark.parametrize("which", ["torus", "sphere"])
def test_device_hierarchy_by_quadric_error(which):
    """The default criterion: the reference's quadric error with its valence penalty (util/mesh.py:394-482), collapsed in
    rounds of a parallel matching.  Artefact contract as above; clusters of 1 .. 5 (the reference's range); the coarse
    mesh stays a closed manifold of the same genus; and it is a BETTER approximation of the fine surface than the
    shortest-edge matching of rounds 1-2 (lower summed quadric error)."""
    from semigcn_amd import meshprep
    m = synth.torus_mesh(200, 150, masks=False) if which == "torus" else synth.octahedron_sphere(5)
    V = m.num_vertices
    fine = meshprep.DeviceMesh(m.x_pos, m.faces, DEV)
    target = int(V * 0.6)
    coarse = fine.simplification(target_v=target)
    ph = coarse.pool_hash
    Vc = coarse.vs.shape[0]
    assert Vc == target and ph.shape == (V, 2) and np.array_equal(ph[:, 0], np.arange(V))
    sizes = np.bincount(ph[:, 1], minlength=Vc)
    assert sizes.min() == 1 and 3 <= sizes.max() <= 5
    order = np.argsort(ph[:, 1], kind="stable")
    first = np.searchsorted(ph[order, 1], np.arange(Vc))
    assert (np.diff(order[first]) > 0).all()            # cluster ids ascend with the smallest member
    ce = ph[:, 1][m.edge_index]
    ce = ce[:, ce[0] != ce[1]]
    want = np.unique(np.minimum(ce[0], ce[1]) * Vc + np.maximum(ce[0], ce[1]))
    got = coarse.edge_index.cpu().numpy()
    half = got.shape[1] // 2
    assert np.array_equal(got[0, :half] * Vc + got[1, :half], want) and np.array_equal(got[:, half:], got[::-1, :half])
    cf = coarse.faces.cpu().numpy()
    assert ((cf[:, 0] != cf[:, 1]) & (cf[:, 1] != cf[:, 2]) & (cf[:, 2] != cf[:, 0])).all() and cf.max() < Vc
    e = np.sort(np.concatenate([cf[:, [0, 1]], cf[:, [1, 2]], cf[:, [2, 0]]]), 1)
    key, cnt = np.unique(e[:, 0] * Vc + e[:, 1], return_counts=True)
    assert (cnt == 2).all()                              # closed manifold: every edge in two triangles
    assert Vc - key.shape[0] + cf.shape[0] == (0 if which == "torus" else 2)      # Euler characteristic kept
    assert np.array_equal(key, want)                     # the quotient graph IS the edge set of the surviving triangles
    by_len = fine.simplification(target_v=target, criterion="length")
    co_q, co_l = torch.from_numpy(ph[:, 1]).to(DEV), torch.from_numpy(by_len.pool_hash[:, 1]).to(DEV)
    e_q = _cluster_quadric_error(fine.vs, fine.faces, co_q, coarse.vs)
    e_l = _cluster_quadric_error(fine.vs, fine.faces, co_l, by_len.vs)
    print(which, "summed quadric error: qem matching", e_q, "shortest-edge matching", e_l)
    assert e_q < 0.8 * e_l
    # a second and third level from the first (what MGCN.__init__ does)
    c2 = coarse.simplification(target_v=int(V * 0.36))
    c3 = c2.simplification(target_v=int(V * 0.216))
    assert c2.vs.shape[0] == int(V * 0.36) and c3.vs.shape[0] == int(V * 0.216)


def test_mgcn_trains_on_the_device_hierarchy_as_on_the_references_own():
    """is a hierarchy built on the device as good FOR THE NETWORK as the one the reference's QEM simplifier
    builds?  Golden g3 holds the reference's own three-level hierarchy of the 258-vertex sphere (its Mesh.simplification
    run through oracle/ref_shim.py).  The same MGCN (same seed, same data, 60 training iterations, Adam every 5th) is
    trained on it and on the hierarchy DeviceMesh.simplification builds from the same faces; compared: the geometric
    error of the three coarse levels and the training loss reached (measured: quadric error per level 7.6 / 25 / 85 on the
    device-built hierarchy against 15.5 / 57 / 179 on the reference's; loss 3.71 -> 0.73 against 3.83 -> 0.78)."""
    from test_host_logic import _mgcn_from_golden
    from semigcn_amd import meshprep, train
    from semigcn_amd.meshnet import MGCN
    g3 = GU.load("g3_mgcn.npz")
    m = synth.octahedron_sphere(3)
    assert np.array_equal(m.edge_index, g3["edge_index/0"])          # the fixture mesh
    V = m.num_vertices
    smo = meshprep.DeviceMesh(g3["smposs/0"], m.faces, DEV)
    ini = meshprep.DeviceMesh(g3["poss/0"], m.faces, DEV)
    v_mask = torch.from_numpy(g3["v_masks/0"][:, 0] > 0)
    faces = torch.from_numpy(m.faces).to(DEV)
    target = torch.from_numpy(g3["poss/0"]).to(DEV)
    v_keep = v_mask.float().view(-1, 1).to(DEV)
    f_keep = v_keep[faces[:, 0]] * v_keep[faces[:, 1]] * v_keep[faces[:, 2]]
    dms = torch.from_numpy(synth.make_dummy_masks(m.edge_index, V, dm_size=10, k=1, p=0.05)).to(DEV)

    def run(build):
        torch.manual_seed(7)
        net = build().to(DEV)

        class D:
            z1 = torch.from_numpy(g3["z1"]).to(DEV).requires_grad_(True)
            x_pos = None
        batch = train.MeshBatch(D, faces, target, train.face_normals(target, faces), v_keep, f_keep, dms)
        tr = train.MGCNTrainer(net, batch, lr=0.01)
        losses = [float(tr.iteration_step()) for _ in range(60)]
        return net, float(np.mean(losses[:5])), float(np.mean(losses[-5:])), float(np.min(losses))
    net_r, first_r, last_r, best_r = run(lambda: _mgcn_from_golden(DEV, g3))
    net_d, first_d, last_d, best_d = run(lambda: MGCN(DEV, smo, ini, v_mask))
    assert [p.shape[0] for p in net_d.smposs_list] == [p.shape[0] for p in net_r.smposs_list] == [258, 154, 92, 55]
    # geometry: summed quadric error of each coarse level against the FINE surface, device-built vs reference-built
    fine_vs, fine_faces = smo.vs, smo.faces
    for name, net in (("reference", net_r), ("device", net_d)):
        comp = torch.arange(V, device=DEV)
        errs = []
        for l in range(3):
            ph = torch.from_numpy(np.asarray(net._pool_pairs[l])).to(DEV)
            comp = ph[:, 1][comp]                      # fine vertex -> its cluster on level l + 1
            errs.append(_cluster_quadric_error(fine_vs, fine_faces, comp, net.smposs_list[l + 1]))
        print(name, "hierarchy: quadric error per level", [f"{e:.3e}" for e in errs])
        if name == "reference":
            ref_errs = errs
        else:
            assert all(e < 2.0 * r + 1e-9 for e, r in zip(errs, ref_errs)), (errs, ref_errs)
    print(f"training: reference hierarchy loss {first_r:.4f} -> {last_r:.4f} (best {best_r:.4f}); "
          f"device hierarchy loss {first_d:.4f} -> {last_d:.4f} (best {best_d:.4f})")
    assert last_r < 0.8 * first_r and last_d < 0.8 * first_d                 # both train
    assert last_d < 1.25 * last_r and best_d < 1.25 * best_r                  # and to the same place


def test_mgcn_reference_constructor_with_device_meshes_vs_oracle():
    """``MGCN(device, smo_mesh, ini_mesh, v_mask)`` -- the reference's constructor signature -- fed
    with meshprep.DeviceMesh objects; the forward equals the oracle's MGCN on the same hierarchy."""
    from semigcn_amd import meshprep
    from semigcn_amd.meshnet import MGCN
    m = synth.torus_mesh(40, 30)
    smo = meshprep.DeviceMesh(m.x_pos, m.faces, DEV)
    ini = meshprep.DeviceMesh(m.vs.astype(np.float32), m.faces, DEV)
    net = MGCN(DEV, smo, ini, torch.from_numpy(m.v_mask))
    sizes = [p.shape[0] for p in net.smposs_list]
    assert sizes == [1200, 720, 432, 259] and sizes[1:] == net.nvs
    GU.fill_state(net, seed=77)
    net.to(DEV).eval()
    ora = OM.MGCNOracle([e.cpu() for e in net.edge_inds], [np.asarray(mm.pool_hash) for mm in net.meshes[1:]],
                        [s.cpu() for s in net.smposs_list])
    ora.load_state_dict({k: v.cpu() for k, v in net.state_dict().items() if not k.endswith("pool_hash")})
    ora.eval()

    class D:
        z1 = torch.from_numpy(m.z1).to(DEV)
        x_pos = None
    with torch.no_grad():
        for a, b in zip(net(D, None), ora(torch.from_numpy(m.z1), None)):
            assert GU.rel_l2(a.cpu(), b) < 5e-5
    assert len(net.f_masks_list) == 4 and all(fm is not None for fm in net.f_masks_list)


def test_mgcn_one_million_vertices_end_to_end_from_faces():
    """Faces -> hierarchy -> MGCN training iteration at V = 1 M without any host-side mesh code."""
    from semigcn_amd import meshprep
    from semigcn_amd.meshnet import MGCN
    m = synth.torus_mesh(1000, 1000, masks=False)
    smo = meshprep.DeviceMesh(m.x_pos, m.faces, DEV)
    net = MGCN(DEV, smo, smo, torch.ones(m.num_vertices, dtype=torch.bool))
    assert [p.shape[0] for p in net.smposs_list] == [1000000] + net.nvs     # int(V * 0.6**i), util/meshnet.py:172
    assert net.nvs[:2] == [600000, 360000]
    net.to(DEV).train()

    class D:
        z1 = torch.from_numpy(m.z1).to(DEV)
        x_pos = None
    outs = net(D, None)
    sum(w * ((o - t) ** 2).mean() for w, o, t in zip((0.35, 0.3, 0.2, 0.15), outs, net.poss_list)).backward()
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None)


# --------------------------------------------------------------------------------------
# refinement solve (Mesh.mesh_merge, util/mesh.py:678-698) by CG on the aggregation kernel
# --------------------------------------------------------------------------------------
REFINE_TOL = 2e-5     # max|x - ref| / max|ref|: the reference solves densely in fp32 (own error ~4e-6 vs fp64)


class _OrgMesh:
    def __init__(self, vs, edge_index=None):
        self.vs = vs
        if edge_index is not None:
            self.edge_index = edge_index


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_mesh_merge_vs_reference_golden(name):
    from semigcn_amd import refine
    g = GU.load("g5_refine.npz")
    ei = torch.from_numpy(g[f"{name}/edge_index"])
    V = g[f"{name}/org_pos"].shape[0]
    # the reference hands over its sparse Lap = I - D^-1 A (util/mesh.py:262-274); only the pattern is read
    deg = torch.bincount(ei[0], minlength=V).float()
    lap = torch.sparse_coo_tensor(torch.cat([ei, torch.arange(V).repeat(2, 1)], 1),
                                  torch.cat([-1.0 / deg[ei[0]], torch.ones(V)]), (V, V))
    for tag in ("w1", "w03", "wb"):
        w, wb = g[f"{name}/{tag}/w"]
        ref = g[f"{name}/{tag}/ref_pos"]
        for lap_arg, mesh in ((lap, _OrgMesh(g[f"{name}/org_pos"])), (None, _OrgMesh(g[f"{name}/org_pos"], ei))):
            x, info = refine.mesh_merge(lap_arg, mesh, torch.from_numpy(g[f"{name}/new_pos"]),
                                        torch.from_numpy(g[f"{name}/preserve"]), w=w, w_b=wb, device=DEV,
                                        return_info=True)
            assert x.dtype == torch.float32 and x.shape == (V, 3) and info["relative_residual"] < 1e-6
            assert rel(x, ref) < REFINE_TOL, (tag, rel(x, ref), info)


def test_mesh_merge_vs_oracle_medium_and_full_size_optimality():
    from oracle import refine as R
    from semigcn_amd import refine, meshprep
    m = synth.torus_mesh(100, 50, permute=True)
    rs = np.random.RandomState(2)
    new = (m.x_pos + 0.05 * rs.standard_normal(m.x_pos.shape)).astype(np.float32)
    want = R.mesh_merge(m.edge_index, m.vs.astype(np.float32), new, m.v_mask, 1.0, 0.0)
    got = refine.mesh_merge(None, _OrgMesh(m.vs.astype(np.float32), torch.from_numpy(m.edge_index)), new, m.v_mask,
                            device=DEV)
    assert rel(got, want) < REFINE_TOL
    # V = 1 M: the normal equations hold, evaluated with an independent index_add Laplacian in float64
    m = synth.torus_mesh(1000, 1000)
    V = m.num_vertices
    topo = meshprep.MeshTopology(m.faces, V, DEV)
    org = torch.from_numpy(m.vs.astype(np.float32)).to(DEV)
    new = torch.from_numpy(m.x_pos).to(DEV) + 0.05 * torch.randn(V, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    keep = torch.from_numpy(m.v_mask).to(DEV)

    class M:
        vs, topology = org, topo
    x, info = refine.mesh_merge(None, M, new, keep, w=1.0, return_info=True)
    assert info["relative_residual"] < 1e-6 and info["iterations"] < 2000
    src, dst = topo.edge_index[0], topo.edge_index[1]
    deg = torch.bincount(dst, minlength=V).double().view(-1, 1)

    def L(v):
        return v - torch.zeros_like(v).index_add_(0, dst, v[src]) / deg

    def Lt(v):
        return v - torch.zeros_like(v).index_add_(0, dst, (v / deg)[src])
    holes = (~keep).double().view(-1, 1)
    inner = (holes + torch.zeros_like(holes).index_add_(0, dst, holes[src])) == 0
    xd, od, nd = x.double(), org.double(), new.double()
    b_mix = torch.where(inner, L(od), L(nd))
    grad = Lt(L(xd) - b_mix) + inner.double() * (xd - od)
    rhs = Lt(b_mix) + inner.double() * od
    assert float(grad.norm() / rhs.norm()) < 1e-5
    assert float((xd - od)[inner.view(-1)].abs().max()) < 0.2 and float((xd - nd).abs().max()) > 1e-3


@pytest.mark.parametrize("name", ["sphere", "open"])
def test_bilateral_normal_loss_with_device_f2f(name):
    """The -CAD term on the device with the face ring from sg_mesh_edges (row order differs from the reference's
    Python-set order; the filter sums over the ring, so only rounding changes)."""
    from semigcn_amd import meshprep, train
    g = GU.load("g6_bnf.npz")
    topo = meshprep.MeshTopology(g[f"{name}/faces"], g[f"{name}/pos"].shape[0], DEV)
    pos = torch.from_numpy(g[f"{name}/pos"]).to(DEV).requires_grad_(True)
    loss, new_fn = train.bilateral_normal_loss(pos, train.face_normals(pos, topo.faces), topo.faces, topo.f2f)
    loss.backward()
    assert abs(float(loss.detach()) - float(g[f"{name}/loss"])) < 2e-6 * float(g[f"{name}/loss"])
    assert rel(new_fn, g[f"{name}/new_fn"]) < 2e-6 and rel(pos.grad, g[f"{name}/dpos"]) < 2e-5


def test_trainer_with_cad_term_runs():
    import bench
    from semigcn_amd import meshprep, train
    m = synth.torus_mesh(40, 30)
    batch = bench.build_mesh_batch(m, torch.device(DEV), n_masks=2)
    with pytest.raises(ValueError, match="f2f"):
        train.SGCNTrainer(SingleScaleGCN(DEV).to(DEV), batch, k2=4.0)
    batch.f2f = meshprep.MeshTopology(m.faces, m.num_vertices, DEV).f2f
    plain = train.SGCNTrainer(SingleScaleGCN(DEV).to(DEV), batch)
    cad = train.SGCNTrainer(SingleScaleGCN(DEV).to(DEV), batch, k2=4.0)
    cad.model.load_state_dict(plain.model.state_dict())
    l0, l1 = float(plain.iteration_step(0).detach()), float(cad.iteration_step(0).detach())
    pos = cad.model(batch.data, batch.v_keep * batch.dummy_masks[:, :1])
    extra = float(train.bilateral_normal_loss(pos, train.face_normals(pos, batch.faces), batch.faces, batch.f2f)[0])
    assert l1 > l0 and abs((l1 - l0) - 4.0 * extra) < 0.05 * (l1 - l0)     # BN statistics moved by one step in between


# --------------------------------------------------------------------------------------
# every code path of the aggregation kernels gives the same bits: the A/B switches of SG_TUNE_FLAGS select the
# 64-bit addressing fallback, fixed-size batches, workgroup barriers, the unpacked neighbour lists
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,dtype", [(4, torch.float32), (24, torch.float32), (64, torch.float32), (256, torch.float32),
                                     (512, torch.float32), (64, torch.bfloat16), (256, torch.bfloat16), (512, torch.bfloat16)])
def test_aggregation_code_paths_are_bit_identical(C, dtype):
    graphs = [(nasty_graph(), 500)]                      # hubs, duplicates, self loops, isolated vertices
    m = synth.torus_mesh(48, 40, permute=True)
    graphs.append((torch.from_numpy(m.edge_index), m.num_vertices))
    try:
        for ei, V in graphs:
            h = capi.GraphHandle.from_edge_index(ei.to(DEV), V)
            x = torch.randn(V, C, device=DEV).to(dtype)
            x0 = torch.randn(V, C, device=DEV).to(dtype)
            ref = None
            for flags in (1, 1 | 16, 1 | 32, 1 | 8, 1 | 4, 1 | 2, 0):
                capi.tuning_set(capi.TUNE_FLAGS, flags | 2048)      # 2048: spmm_rows / spmm_shared, not the ring kernel
                y = h.spmm(x, torch.empty_like(x), alpha=2.0, X0=x0, beta=-1.0)
                z = h.spmm(x, torch.empty_like(x))
                if ref is None:
                    ref = (y.clone(), z.clone())
                    want = oracle_lhat(ei, x.float().cpu(), 2.0, x0.float().cpu(), -1.0)
                    tol = KERNEL_TOL if dtype == torch.float32 else 2.0 ** -6
                    assert rel(y.float(), want) < tol
                else:
                    assert torch.equal(y, ref[0]) and torch.equal(z, ref[1]), flags
    finally:
        capi.tuning_set(capi.TUNE_FLAGS, 1)


def test_loss_backward_without_atomics_is_reproducible_and_matches_atomic_kernel():
    """functional.DETERMINISTIC_LOSS_BACKWARD: per-corner gradients + fixed-order CSR sum == the atomic kernel up to
    fp32 summation order, and identical bits from run to run (with halo rows: V_ext > V).  The normal term is an L1
    norm: a face with a component of n - n_t within rounding of zero may take either sign in either kernel (they are
    compiled separately; with unseeded inputs that happened in ~30 % of the runs of the round-1 version of this test),
    so the vertices of such faces are compared against neither."""
    from semigcn_amd import functional as F_sg, train
    m = synth.torus_mesh(120, 90)
    V = m.num_vertices
    faces = torch.from_numpy(m.faces).to(DEV)
    n_own = V - 700                                            # pretend the last 700 rows are halo rows
    own_faces = faces[(faces[:, 0] < n_own)]
    gen = torch.Generator(device=DEV).manual_seed(1234)
    vs = torch.from_numpy(m.vs.astype(np.float32)).to(DEV)
    pos = vs + 0.01 * torch.randn(V, 3, device=DEV, generator=gen)
    tpos = vs[:n_own]
    tfn = train.face_normals(vs, own_faces)
    vk = (torch.rand(n_own, device=DEV, generator=gen) > 0.1).float()
    fk = (torch.rand(own_faces.shape[0], device=DEV, generator=gen) > 0.1).float()
    at_kink = ((train.face_normals(pos, own_faces) - tfn).abs() < 1e-5).any(1)
    safe = torch.ones(V, dtype=torch.bool, device=DEV)
    safe[own_faces[at_kink].reshape(-1)] = False
    assert int(safe.sum()) > V - 1000                     # ~80 of 21 K faces sit within 1e-5 of a kink

    def grad(det):
        F_sg.DETERMINISTIC_LOSS_BACKWARD = det
        p = pos.clone().requires_grad_(True)
        s = F_sg.mesh_loss_sums(p, own_faces, tpos, vk, tfn, fk)
        (0.7 * torch.sqrt(s[0] / 1000.0 + 1e-6) + 4.0 * s[1] / 2000.0).backward()
        return p.grad.clone()
    try:
        a, b, c = grad(True), grad(True), grad(False)
    finally:
        F_sg.DETERMINISTIC_LOSS_BACKWARD = True
    assert torch.equal(a, b)
    assert rel(a[safe], c[safe]) < 2e-6 and bool((a[n_own:] != 0).any())      # halo rows receive face contributions only
    # both against autograd in float64 through the plain formulas
    p64 = pos.double().requires_grad_(True)
    d = (tpos.double() - p64[:n_own]) * vk.double().view(-1, 1)
    s1 = ((train.face_normals(p64, own_faces) - tfn.double()).abs() * fk.double().view(-1, 1)).sum()
    (0.7 * torch.sqrt((d * d).sum() / 1000.0 + 1e-6) + 4.0 * s1 / 2000.0).backward()
    assert rel(a[safe], p64.grad[safe]) < 2e-6 and rel(c[safe], p64.grad[safe]) < 2e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_training_is_bit_reproducible(dtype):
    """No atomics anywhere on the iteration path (CSR-owned aggregation rows, fixed-order reductions, the loss backward
    through the corner incidence): two runs from the same state give identical bits after an optimiser step."""
    import bench
    from semigcn_amd import train
    m = synth.torus_mesh(200, 150)
    batch = bench.build_mesh_batch(m, torch.device(DEV), n_masks=3)

    def run():
        net = SingleScaleGCN(DEV)
        GU.fill_state(net, seed=9)
        net.to(DEV).set_feature_dtype(dtype)
        tr = train.SGCNTrainer(net, batch)
        losses = [tr.iteration_step().detach().clone() for _ in range(6)]
        return torch.stack(losses), {k: v.clone() for k, v in net.state_dict().items()}
    la, sa = run()
    lb, sb = run()
    assert torch.equal(la, lb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


# --------------------------------------------------------------------------------------
# hipGraph replay of the training iteration (opt-in; needs a runtime flag from process start)
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sgcn", "mgcn"])
def test_graphed_training_matches_eager(kind):
    import os
    import subprocess
    import sys
    from semigcn_amd import train
    env = dict(os.environ)
    env[train.GRAPH_ENV[0]] = train.GRAPH_ENV[1]
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "graph_replay_script.py")
    out = subprocess.run([sys.executable, script, kind], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "GRAPH_REPLAY_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_graph_capture_refuses_without_the_runtime_flag(monkeypatch):
    import bench
    from semigcn_amd import train
    monkeypatch.delenv(train.GRAPH_ENV[0], raising=False)
    m = synth.torus_mesh(20, 12)
    batch = bench.build_mesh_batch(m, torch.device(DEV), n_masks=2)
    with pytest.raises(RuntimeError, match="DEBUG_CLR_GRAPH_PACKET_CAPTURE"):
        train.SGCNTrainer(SingleScaleGCN(DEV).to(DEV), batch, capture=True)


# --------------------------------------------------------------------------------------
# locality view: a graph whose numbering has no locality gets its rows processed in a graph-derived order
# --------------------------------------------------------------------------------------
def test_graph_locality_view_is_transparent_and_bit_identical():
    """Operator tier on a raw-scan numbering (no positions to sort by): sg_graph_create orders the ROWS by two levels
    of multi-source-BFS cells.  Nothing the caller sees may change: same CSR export, same rows of Y, bit-identical
    values (a row's neighbours are still summed in ascending id order) -- against the same graph built with the view
    switched off, for every kernel family, and against the oracle."""
    m = synth.torus_mesh(300, 250, permute=True, masks=False)          # 75 000 vertices in random order
    V = m.num_vertices
    ei = torch.from_numpy(m.edge_index).to(DEV)
    g_auto = capi.GraphHandle.from_edge_index(ei, V)
    capi.tuning_set(capi.TUNE_GRAPH_REORDER, 1)
    try:
        g_plain = capi.GraphHandle.from_edge_index(ei, V)
    finally:
        capi.tuning_set(capi.TUNE_GRAPH_REORDER, 0)
    assert g_auto.reordered and not g_plain.reordered
    for a, b in zip(g_auto.arrays(), g_plain.arrays()):
        assert torch.equal(a, b)
    gen = torch.Generator(device=DEV).manual_seed(5)
    for C, dtype in ((4, torch.float32), (24, torch.float32), (64, torch.float32), (256, torch.float32), (512, torch.float32),
                     (7, torch.float32), (16, torch.bfloat16), (128, torch.bfloat16), (256, torch.bfloat16)):
        x = torch.randn(V, C, device=DEV, generator=gen).to(dtype)
        x0 = torch.randn(V, C, device=DEV, generator=gen).to(dtype)
        x1 = torch.randn(V, C, device=DEV, generator=gen).to(dtype)
        ring = dtype == torch.bfloat16 and C in (128, 256)               # served by spmm_ring (tile records of each graph)
        for kw in ({}, {"alpha": 2.0, "X0": x0, "beta": -1.0}, {"alpha": 1.0, "X0": x0, "beta": 1.0, "X1": x1, "gamma": -1.0},
                   {"transpose": True}):
            ya = g_auto.spmm(x, torch.empty_like(x), **kw)
            yb = g_plain.spmm(x, torch.empty_like(x), **kw)
            if ring:      # the ring kernel's tiles follow the processing order: the matrix cores' accumulation order differs
                d = (ya.float() - yb.float()).abs()
                assert bool((d <= 2.0 ** -7 * yb.float().abs() + 1e-5).all()), (C, list(kw), float(d.max()))
                capi.tuning_set(capi.TUNE_FLAGS, 1 | 2048)           # and spmm_rows under it stays bit-identical
                try:
                    ya = g_auto.spmm(x, torch.empty_like(x), **kw)
                    yb = g_plain.spmm(x, torch.empty_like(x), **kw)
                finally:
                    capi.tuning_set(capi.TUNE_FLAGS, 1)
            assert torch.equal(ya, yb), (C, dtype, list(kw))
        # strided operands: column blocks of a wider buffer, output in place of the epilogue operand
        wide_a = torch.randn(V, 3 * C, device=DEV, generator=gen).to(dtype)
        wide_b = wide_a.clone()
        g_auto.spmm(wide_a[:, :C], wide_a[:, C:2 * C], alpha=2.0, X0=wide_a[:, C:2 * C], beta=1.0)
        g_plain.spmm(wide_b[:, :C], wide_b[:, C:2 * C], alpha=2.0, X0=wide_b[:, C:2 * C], beta=1.0)
        if ring:
            d = (wide_a.float() - wide_b.float()).abs()
            assert bool((d <= 2.0 ** -7 * wide_b.float().abs() + 1e-5).all()), (C, float(d.max()))
        else:
            assert torch.equal(wide_a, wide_b)
    x = torch.randn(V, 12, device=DEV, generator=gen)
    assert rel(g_auto.spmm(x, torch.empty_like(x)), oracle_lhat(torch.from_numpy(m.edge_index), x.cpu())) < 1e-5
    bits = torch.randint(0, 2 ** 62, (V, 1), device=DEV, generator=gen)
    assert torch.equal(g_auto.dilate_bits(bits), g_plain.dilate_bits(bits))
    # numberings WITH locality keep the plain path: grid order, and the Morton order the model tier produces
    grid = synth.torus_mesh(300, 250, masks=False)
    assert not capi.GraphHandle.from_edge_index(torch.from_numpy(grid.edge_index).to(DEV), V).reordered
    from semigcn_amd import reorder
    _, rank = reorder.morton_order(torch.from_numpy(m.x_pos).to(DEV))
    assert not capi.GraphHandle.from_edge_index(reorder.permute_edge_index(ei, rank), V).reordered


def test_graph_locality_view_forced_on_small_and_degenerate_graphs(fixture_meshes):
    """SG_TUNE_GRAPH_REORDER = 2 forces the view: tiny meshes, isolated vertices and vertices in components without a
    seed must come out exactly as without it; an asymmetric graph never gets one."""
    capi.tuning_set(capi.TUNE_GRAPH_REORDER, 2)
    try:
        for name in ("sphere", "torus"):
            m = fixture_meshes[name]
            V = m.num_vertices + 5                                         # five isolated vertices at the end
            ei = torch.from_numpy(m.edge_index).to(DEV)
            g = capi.GraphHandle.from_edge_index(ei, V)
            assert g.reordered
            x = torch.randn(V, 20, device=DEV)
            y = g.spmm(x, torch.empty_like(x), alpha=2.0, X0=x, beta=-1.0)
            want = oracle_lhat(torch.from_numpy(m.edge_index), x.cpu(), alpha=2.0, x0=x.cpu(), beta=-1.0)
            capi.tuning_set(capi.TUNE_GRAPH_REORDER, 1)
            g0 = capi.GraphHandle.from_edge_index(ei, V)
            capi.tuning_set(capi.TUNE_GRAPH_REORDER, 2)
            assert torch.equal(y, g0.spmm(x, torch.empty_like(x), alpha=2.0, X0=x, beta=-1.0))
            assert torch.equal(y[-5:], -x[-5:])                            # isolated rows: only the epilogue term
            assert rel(y, want) < 1e-5
        h = capi.GraphHandle.from_edge_index(nasty_graph().to(DEV), 500)
        assert not h.symmetric and not h.reordered
    finally:
        capi.tuning_set(capi.TUNE_GRAPH_REORDER, 0)


def test_partition_operators_wide_and_row_subsets_agree():
    """One rank's operators of a 4-way partition, real kernels, no process group needed: the wide operator (owned +
    ring-1 rows, sg_graph_create_rect) == its interior / rest halves (sg_graph_create_rows: row subsets that write
    only their own rows) == the owned-rows operator, bit for bit, and == the global operator's rows to rounding."""
    from semigcn_amd import dist as sgdist, reorder
    m = synth.torus_mesh(96, 64, permute=True, masks=False)
    V = m.num_vertices
    _, rank_of = reorder.morton_order(torch.from_numpy(m.x_pos).to(DEV))
    ei = reorder.permute_edge_index(torch.from_numpy(m.edge_index).to(DEV), rank_of)
    full = capi.GraphHandle.from_edge_index(ei, V)
    def same(a, b, ring):
        if not ring:
            return torch.equal(a, b)
        d = (a.float() - b.float()).abs()      # spmm_ring: the tiles of the two operators differ, and with them the accumulation order
        return bool((d <= 2.0 ** -7 * b.float().abs() + 1e-5).all())

    for C, dtype, flags in ((16, torch.float32, 1), (64, torch.bfloat16, 1), (256, torch.float32, 1), (256, torch.bfloat16, 1),
                            (128, torch.bfloat16, 1), (256, torch.bfloat16, 1 | 2048)):
        ring = dtype == torch.bfloat16 and C in (128, 256) and not flags & 2048
        capi.tuning_set(capi.TUNE_FLAGS, flags)
        try:
            x = torch.randn(V, C, device=DEV).to(dtype)
            x0 = torch.randn(V, C, device=DEV).to(dtype)
            y_full = full.spmm(x, torch.empty_like(x), alpha=2.0, X0=x0, beta=-1.0)
            for r in (0, 3):
                g = sgdist.DistMeshGraph(ei, V, r, 4)
                ids = torch.cat([torch.arange(g.start, g.end, device=DEV), g.halo_ids])
                x_ext, x0_ext = x[ids].contiguous(), x0[ids].contiguous()
                yw = g.handle_wide.spmm(x_ext, torch.zeros_like(x_ext), alpha=2.0, X0=x0_ext, beta=-1.0)
                ys = torch.full_like(x_ext, float("nan"))
                g._split[0].spmm(x_ext, ys, alpha=2.0, X0=x0_ext, beta=-1.0)
                done = torch.isfinite(ys.float()[:, 0])
                assert int(done.sum()) == g.n_interior > 0 and not bool(done[g.n_own:].any())
                g._split[1].spmm(x_ext, ys, alpha=2.0, X0=x0_ext, beta=-1.0)
                done = torch.isfinite(ys.float()[:, 0])
                assert int(done.sum()) == g.n_own + g.n_halo1 and bool(done[:g.n_own].all())
                assert same(ys[done], yw[done], ring)
                # against the global operator: same rows, neighbours summed in a different order ([owned | halo] ids)
                tol = 1e-5 if dtype == torch.float32 else 2.0 ** -7
                assert rel(ys[done].float(), y_full[ids[done]].float()) < tol
                yo = g.handle.spmm(x_ext, torch.empty((g.n_own, C), dtype=dtype, device=DEV), alpha=2.0, X0=x0_ext[:g.n_own], beta=-1.0)
                assert same(yo, ys[:g.n_own], ring)
        finally:
            capi.tuning_set(capi.TUNE_FLAGS, 1)


@pytest.mark.parametrize("V,C,dtype", [(5000, 256, torch.float32), (70001, 64, torch.bfloat16), (1200, 8, torch.float32),
                                       (300000, 16, torch.bfloat16), (999, 512, torch.bfloat16)])
def test_bn_backward_apply_with_fused_column_sums(V, C, dtype):
    """sg_bn_act_bwd_apply_colsum == sg_bn_act_bwd_apply bit for bit, and its column sums == the sums of the dH it
    stored (the bias gradient of the ChebConv in front of the BatchNorm)."""
    g = torch.Generator(device=DEV).manual_seed(V + C)
    dA = torch.randn(V, C, device=DEV, generator=g).to(dtype)
    H = torch.randn(V, C, device=DEV, generator=g).to(dtype)
    vec = lambda: torch.randn(C, device=DEV, generator=g)
    scale, shift, mean, k, c1, c2 = vec(), vec(), vec(), vec(), vec() * 0.01, vec() * 0.01
    invstd = torch.rand(C, device=DEV, generator=g) + 0.5
    ref = capi.bn_act_bwd_apply(dA, H, scale, shift, mean, invstd, k, c1, c2, 0.01)
    wide = torch.zeros(V, 3 * C, device=DEV, dtype=dtype)
    got, sums = capi.bn_act_bwd_apply_colsum(dA, H, scale, shift, mean, invstd, k, c1, c2, 0.01, out=wide[:, :C])
    assert sums is not None and torch.equal(got, ref) and bool((wide[:, C:] == 0).all())
    want = ref.double().sum(0)
    assert float((sums.double() - want).abs().max()) <= 1e-5 * float(ref.double().abs().sum(0).max())
    _, sums2 = capi.bn_act_bwd_apply_colsum(dA, H, scale, shift, mean, invstd, k, c1, c2, 0.01)
    assert torch.equal(sums, sums2)                                    # deterministic
    # a shape the row-owning kernel does not serve falls back (no sums)
    odd = capi.bn_act_bwd_apply_colsum(dA[:, :7].contiguous(), H[:, :7].contiguous(), scale[:7].contiguous(), shift[:7].contiguous(),
                                       mean[:7].contiguous(), invstd[:7].contiguous(), k[:7].contiguous(), c1[:7].contiguous(),
                                       c2[:7].contiguous(), 0.01)
    assert odd[1] is None and odd[0].shape == (V, 7)


NO_RING = 2048         # SG_TUNE_FLAGS bit 11: bf16 rows of 128 / 256 channels stay on spmm_rows (graph creation: no tile records)


def _ring_graph(ei, V):
    return capi.GraphHandle.from_edge_index(ei, V)


def _ring_and_rows(g, calls, ring_flags=1):
    out = {}
    for flags in (1 | NO_RING, ring_flags):
        capi.tuning_set(capi.TUNE_FLAGS, flags)
        try:
            out[flags] = [f() for f in calls]
        finally:
            capi.tuning_set(capi.TUNE_FLAGS, 1)
    return out[1 | NO_RING], out[ring_flags]


@pytest.mark.parametrize("ring_flags", [1, 1 | 4096])   # how the tile leaves: full rows through LDS (default where LDS lasts) / direct
@pytest.mark.parametrize("C", [128, 256])
def test_ring_kernel_matches_the_rows_kernel_and_the_float64_oracle(C, ring_flags):
    """spmm_ring (the default for bf16 rows of 128 / 256 channels; SG_TUNE_FLAGS bit 11 switches it off): a persistent workgroup pipelines LDS-DMA of each tile's distinct source rows under
    the reduction of the tile before, and reduces on the matrix cores (the tile's fp32 weights as three bf16 pieces:
    exact products, the MFMA's own accumulation order).  Against spmm_rows (sequential fma chain) the bf16 outputs may
    differ by the rounding of the last accumulated bit: every element within one bf16 ulp (2^-7 relative; plus the fp32
    rounding noise of a cancelling sum), almost all identical; against the float64 oracle it is as close as spmm_rows.
    On a Morton-ordered mesh and through the locality view of a randomly numbered one, every epilogue arity, strided
    column blocks, and deterministic run to run."""
    from semigcn_amd import reorder
    dtype = torch.bfloat16
    for permute in (False, True):
        m = synth.torus_mesh(320, 250, permute=permute, masks=False)
        V = m.num_vertices
        ei = torch.from_numpy(m.edge_index).to(DEV)
        if not permute:
            ei = reorder.permute_edge_index(ei, reorder.morton_order(torch.from_numpy(m.x_pos).to(DEV))[1])
        g = _ring_graph(ei, V)
        assert g.reordered == permute
        gen = torch.Generator(device=DEV).manual_seed(C)
        wide = torch.randn(V, 3 * C, device=DEV, generator=gen).to(dtype)
        x, x0, x1 = wide[:, :C], wide[:, C:2 * C], wide[:, 2 * C:]
        calls = [lambda: g.spmm(x, torch.empty((V, C), dtype=dtype, device=DEV)),
                 lambda: g.spmm(x, torch.empty((V, C), dtype=dtype, device=DEV), alpha=2.0, X0=x0, beta=-1.0),
                 lambda: g.spmm(x, torch.empty((V, C), dtype=dtype, device=DEV), alpha=1.0, X0=x0, beta=1.0, X1=x1, gamma=-1.0)]
        rows, ring = _ring_and_rows(g, calls, ring_flags)
        _, ring2 = _ring_and_rows(g, calls, ring_flags)
        for a, b, b2 in zip(rows, ring, ring2):
            assert torch.equal(b, b2)                                       # deterministic
            d = (a.float() - b.float()).abs()
            assert bool((d <= 2.0 ** -7 * a.float().abs() + 1e-5).all()), float(d.max())
            assert float((d > 0).float().mean()) < 0.02                     # a different last bit is the exception
        exact = oracle_lhat(ei.cpu(), x.float().cpu())
        e_rows, e_ring = rel(rows[0].float(), exact), rel(ring[0].float(), exact)
        assert e_ring < 1.02 * e_rows + 1e-6, (e_ring, e_rows)


@pytest.mark.parametrize("C", [128, 256])
def test_ring_kernel_on_a_graph_with_hubs_repeats_isolated_vertices_and_no_symmetry(C):
    """The ring kernel on the graph the other kernels are tortured with: a hub row with ~1200 neighbours, repeated edges,
    self loops, isolated vertices, NOT symmetric (so the transposed operator has a CSR and tile records of its own), a
    vertex count that is no multiple of 16, sparse random rows whose tiles mix records that fit with records that do not.
    Both directions, every epilogue arity, against spmm_rows to one bf16 ulp and against the oracle."""
    ei, V = nasty_graph(), 500
    g = capi.GraphHandle.from_edge_index(ei.to(DEV), V)
    gen = torch.Generator(device=DEV).manual_seed(11 + C)
    x = torch.randn(V, C, device=DEV, generator=gen).bfloat16()
    x0 = torch.randn(V, C, device=DEV, generator=gen).bfloat16()
    x1 = torch.randn(V, C, device=DEV, generator=gen).bfloat16()
    new = lambda: torch.empty((V, C), dtype=torch.bfloat16, device=DEV)
    calls = [lambda: g.spmm(x, new()), lambda: g.spmm(x, new(), transpose=True),
             lambda: g.spmm(x, new(), alpha=2.0, X0=x0, beta=-1.0), lambda: g.spmm(x, new(), alpha=2.0, X0=x0, beta=-1.0, transpose=True),
             lambda: g.spmm(x, new(), alpha=1.0, X0=x0, beta=1.0, X1=x1, gamma=-1.0)]
    for ring_flags in (1, 1 | 4096):
        rows, ring = _ring_and_rows(g, calls, ring_flags)
        for a, b in zip(rows, ring):
            d = (a.float() - b.float()).abs()
            assert bool((d <= 2.0 ** -7 * a.float().abs() + 1e-4).all()), float(d.max())
    assert rel(ring[0].float(), oracle_lhat(ei, x.float().cpu())) < 2.0 ** -7


def test_ring_kernel_on_tiny_and_random_graphs():
    """Sizes around the tile and workgroup boundaries (1 .. 4099 vertices: fewer tiles than workgroups, a last tile of one
    row), random asymmetric graphs from half an edge to eight edges per vertex (records that fit, records that do not,
    empty rows), both directions, every epilogue arity, both store modes: finite, and within one bf16 ulp of spmm_rows."""
    rs = np.random.RandomState(0)
    checked = 0
    try:
        for V in (1, 2, 5, 15, 16, 17, 31, 32, 33, 47, 100, 257, 1000, 4099):
            for density in (0.5, 3, 8):
                ei = torch.from_numpy(rs.randint(0, V, size=(2, max(1, int(V * density))))).long().to(DEV)
                g = capi.GraphHandle.from_edge_index(ei, V)
                for C in (128, 256):
                    x, x0, x1 = (torch.randn(V, C, device=DEV).bfloat16() for _ in range(3))
                    for kw in ({}, {"alpha": 2.0, "X0": x0, "beta": -1.0}, {"alpha": 1.0, "X0": x0, "beta": 1.0, "X1": x1, "gamma": -1.0},
                               {"transpose": True}):
                        outs = []
                        for flags in (1 | NO_RING, 1, 1 | 4096):
                            capi.tuning_set(capi.TUNE_FLAGS, flags)
                            outs.append(g.spmm(x, torch.full((V, C), 7.0, device=DEV, dtype=torch.bfloat16), **kw))
                        for o in outs[1:]:
                            d = (o.float() - outs[0].float()).abs()
                            assert bool(torch.isfinite(o.float()).all()) and bool((d <= 2.0 ** -7 * outs[0].float().abs() + 1e-4).all()), \
                                (V, density, C, list(kw), float(d.max()))
                            checked += 1
    finally:
        capi.tuning_set(capi.TUNE_FLAGS, 1)
    assert checked == 672


def test_ring_kernel_tiles_that_do_not_fit_gather_from_global_memory():
    """A graph without locality (random sources, ~20 per row, repeated edges): no 16-row or 8-row tile fits the LDS budget
    of spmm_ring (48 distinct sources, 16 neighbours per row, no repeats), every record says so and the kernel's in-loop
    fallback sums the rows from global memory with the sequential fma chain of spmm_rows: identical bits."""
    V, C = 5000, 256
    gen = torch.Generator().manual_seed(7)
    a = torch.randint(0, V, (50000,), generator=gen)
    b = torch.randint(0, V, (50000,), generator=gen)
    keep = a != b
    a, b = a[keep], b[keep]
    ei = torch.stack([torch.cat([a, b]), torch.cat([b, a])]).to(DEV)
    capi.tuning_set(capi.TUNE_GRAPH_REORDER, 1)
    try:
        g = _ring_graph(ei, V)
    finally:
        capi.tuning_set(capi.TUNE_GRAPH_REORDER, 0)
    x = torch.randn(V, C, device=DEV).bfloat16()
    x0 = torch.randn(V, C, device=DEV).bfloat16()
    calls = [lambda: g.spmm(x, torch.empty((V, C), dtype=torch.bfloat16, device=DEV)),
             lambda: g.spmm(x, torch.empty((V, C), dtype=torch.bfloat16, device=DEV), alpha=2.0, X0=x0, beta=-1.0)]
    rows, ring = _ring_and_rows(g, calls)
    for r, q in zip(rows, ring):
        assert torch.equal(r, q)


NO_RING_F32 = 8192     # SG_TUNE_FLAGS bit 13: float32 rows stay on spmm_rows


def _f32_ring_and_rows(calls):
    out = {}
    for flags in (1 | NO_RING_F32, 1):
        capi.tuning_set(capi.TUNE_FLAGS, flags)
        try:
            out[flags] = [f() for f in calls]
        finally:
            capi.tuning_set(capi.TUNE_FLAGS, 1)
    return out[1 | NO_RING_F32], out[1]


@pytest.mark.parametrize("C", [128, 256])
def test_f32_ring_kernel_equals_the_rows_kernel_bit_for_bit(C):
    """spmm_ring_f32 (float32 rows of 128 channels, rows of 256 as their two halves -- the reference's own precision;
    SG_TUNE_FLAGS bit 13 switches it off): the tile pipeline of spmm_ring with float32 operands on v_mfma_f32_16x16x4_f32.
    The matrix core adds the products of a step in slot order into its float32 accumulator, the slots of a tile are its
    sources in ascending order and an unused slot contributes weight 0: the sum of every row is spmm_rows' fma chain over
    the neighbours in ascending id -- the SAME BITS (and so the same distance from the float64 oracle).  Morton-ordered mesh
    and the locality view of a randomly numbered one, every epilogue arity, column blocks of a wider buffer.  (That the tiled
    kernel is what runs: tools/ring_f32_probe.py times the two, profiles/r05_ring_f32_probe.txt.)"""
    from semigcn_amd import reorder
    for permute in (False, True):
        m = synth.torus_mesh(320, 250, permute=permute, masks=False)
        V = m.num_vertices
        ei = torch.from_numpy(m.edge_index).to(DEV)
        if not permute:
            ei = reorder.permute_edge_index(ei, reorder.morton_order(torch.from_numpy(m.x_pos).to(DEV))[1])
        g = _ring_graph(ei, V)
        gen = torch.Generator(device=DEV).manual_seed(C)
        wide = torch.randn(V, 3 * C, device=DEV, generator=gen)
        x, x0, x1 = wide[:, :C], wide[:, C:2 * C], wide[:, 2 * C:]
        outw = torch.zeros((V, C + 8), device=DEV)
        calls = [lambda: g.spmm(x, torch.empty((V, C), device=DEV)),
                 lambda: g.spmm(x, torch.empty((V, C), device=DEV), alpha=2.0, X0=x0, beta=-1.0),
                 lambda: g.spmm(x, torch.empty((V, C), device=DEV), alpha=1.0, X0=x0, beta=1.0, X1=x1, gamma=-1.0),
                 lambda: g.spmm(x, outw[:, 4:4 + C], alpha=2.0, X0=x0, beta=-1.0).clone()]
        rows, ring = _f32_ring_and_rows(calls)
        assert torch.all(outw[:, :4] == 0) and torch.all(outw[:, 4 + C:] == 0)
        for a, b in zip(rows, ring):
            assert torch.equal(a, b)
        assert rel(ring[0], oracle_lhat(ei.cpu(), x.cpu())) < 1e-6


@pytest.mark.parametrize("C", [128, 256])
def test_f32_ring_kernel_on_nasty_tiny_and_random_graphs(C):
    """The float32 tile kernel where the bf16 one is tortured: a hub row, repeated edges, self loops, isolated vertices, no
    symmetry (both directions); vertex counts around the tile and workgroup boundaries, random graphs from half an edge to
    eight per vertex (records that fit and records that do not), every epilogue arity: the bits of spmm_rows."""
    rs = np.random.RandomState(1)
    graphs = [(nasty_graph().to(DEV), 500)]
    for V in (1, 2, 15, 16, 17, 33, 100, 257, 1000, 4099):
        for density in (0.5, 3, 8):
            graphs.append((torch.from_numpy(rs.randint(0, V, size=(2, max(1, int(V * density))))).long().to(DEV), V))
    checked = 0
    try:
        for ei, V in graphs:
            g = capi.GraphHandle.from_edge_index(ei, V)
            x, x0, x1 = (torch.randn(V, C, device=DEV) for _ in range(3))
            for kw in ({}, {"alpha": 2.0, "X0": x0, "beta": -1.0}, {"alpha": 1.0, "X0": x0, "beta": 1.0, "X1": x1, "gamma": -1.0},
                       {"transpose": True}, {"transpose": True, "alpha": 2.0, "X0": x0, "beta": -1.0}):
                outs = []
                for flags in (1 | NO_RING_F32, 1):
                    capi.tuning_set(capi.TUNE_FLAGS, flags)
                    outs.append(g.spmm(x, torch.full((V, C), 7.0, device=DEV), **kw))
                assert torch.equal(outs[1], outs[0]), (V, C, list(kw), float((outs[1] - outs[0]).abs().max()))
                checked += 1
    finally:
        capi.tuning_set(capi.TUNE_FLAGS, 1)
    assert checked == 155


def test_f32_ring_kernel_tiles_that_do_not_fit_gather_from_global_memory():
    """No tile of a graph without locality fits: every record says so and the in-loop fallback of spmm_ring_f32 sums the rows
    from global memory with the sequential fma chain of spmm_rows: identical bits."""
    V, C = 5000, 256
    gen = torch.Generator().manual_seed(7)
    a = torch.randint(0, V, (50000,), generator=gen)
    b = torch.randint(0, V, (50000,), generator=gen)
    keep = a != b
    a, b = a[keep], b[keep]
    ei = torch.stack([torch.cat([a, b]), torch.cat([b, a])]).to(DEV)
    capi.tuning_set(capi.TUNE_GRAPH_REORDER, 1)
    try:
        g = _ring_graph(ei, V)
    finally:
        capi.tuning_set(capi.TUNE_GRAPH_REORDER, 0)
    x, x0 = torch.randn(V, C, device=DEV), torch.randn(V, C, device=DEV)
    calls = [lambda: g.spmm(x, torch.empty((V, C), device=DEV)),
             lambda: g.spmm(x, torch.empty((V, C), device=DEV), alpha=2.0, X0=x0, beta=-1.0)]
    rows, ring = _f32_ring_and_rows(calls)
    for r, q in zip(rows, ring):
        assert torch.equal(r, q)


# --------------------------------------------------------------------------------------
# documented deviations from the reference's arithmetic (include/semigcn.h), one test each
# --------------------------------------------------------------------------------------
def test_non_finite_input_rows_stay_local_to_a_bounded_set_of_output_rows(fixture_meshes):
    """semigcn.h, sg_spmm: "an Inf/NaN in X can turn into NaN in a few output rows that are not its neighbours" (the
    switched-off slots of a gather batch carry weight ZERO on a row that is read anyway).  What that means in numbers: with
    ONE non-finite input row every neighbour's output is non-finite (as with the reference's scatter_add), every output
    row that is finite equals the oracle's, and the non-finite rows that are NOT neighbours are few and share a wavefront
    chunk with a neighbour (within 32 rows of one)."""
    m = synth.torus_mesh(60, 40, masks=False)
    V = m.num_vertices
    ei = torch.from_numpy(m.edge_index)
    g = MeshGraph.from_edge_index(ei.to(DEV), V)
    for C, dtype in ((64, torch.float32), (256, torch.bfloat16), (4, torch.bfloat16)):
        x = torch.randn(V, C).to(dtype)
        bad = 1234
        x[bad, ::2] = float("inf")
        x[bad, 1::2] = float("nan")
        y = torch.empty(V, C, device=DEV, dtype=dtype)
        g.aggregate(x.to(DEV), y)
        ref = oracle_lhat(ei, x.float())
        nonfinite = ~torch.isfinite(y.float().cpu()).all(1)
        nbrs = torch.zeros(V, dtype=torch.bool)
        nbrs[ei[1][ei[0] == bad]] = True
        assert bool(nonfinite[nbrs].all())                                   # the neighbours, as in the reference
        assert torch.equal(~torch.isfinite(ref).all(1), nbrs)                # (the oracle: exactly the neighbours)
        fin = ~nonfinite
        tol = KERNEL_TOL if dtype == torch.float32 else 2.0 ** -7
        assert rel(y.float().cpu()[fin], ref[fin]) < tol                     # finite rows are the CSR sums
        extra = torch.nonzero(nonfinite & ~nbrs).reshape(-1)
        assert extra.numel() <= 64
        nb_ids = torch.nonzero(nbrs).reshape(-1)
        if extra.numel():
            assert int((extra.view(-1, 1) - nb_ids.view(1, -1)).abs().min(1)[0].max()) <= 32


def test_empty_coarse_cluster_yields_zero_where_the_reference_yields_nan():
    """semigcn.h, sg_pool_mean: "a coarse row with no member yields 0 (the reference yields 0/0 = NaN there)":
    util/meshnet.py:14-17 divides the summed rows by the row sums of the dense pool matrix."""
    fine = torch.tensor([0, 1, 2, 3, 4], device=DEV)
    coarse = torch.tensor([0, 0, 2, 2, 2], device=DEV)          # coarse vertex 1 has no member
    pool = capi.PoolHandle(fine, coarse, 5, 3)
    x = torch.arange(10, dtype=torch.float32, device=DEV).view(5, 2)
    out = pool.pool_mean(x)
    assert torch.equal(out.cpu(), torch.tensor([[1.0, 2.0], [0.0, 0.0], [6.0, 7.0]]))
    dense = torch.zeros(3, 5)
    dense[coarse.cpu(), fine.cpu()] = 1.0
    ref = (dense @ x.cpu()) / dense.sum(1, keepdim=True)        # the reference's formula
    assert bool(torch.isnan(ref[1]).all()) and torch.equal(ref[[0, 2]], out.cpu()[[0, 2]])
    # and the gradient of the empty row goes nowhere
    assert torch.equal(pool.pool_mean_bwd(torch.ones(3, 2, device=DEV)).cpu(),
                       torch.tensor([[0.5] * 2] * 2 + [[1.0 / 3] * 2] * 3))


@pytest.mark.parametrize("dtype,C", [(torch.float32, 256), (torch.float32, 512), (torch.bfloat16, 512), (torch.bfloat16, 256), (torch.float32, 64)])
def test_batchnorm_apply_passes_do_not_depend_on_which_rows_a_workgroup_takes(dtype, C):
    """SG_TUNE_BN_ROWS (round 5): the apply passes of BatchNorm + LeakyReLU give every workgroup one contiguous range of rows
    where the rows are wide, row groups strided over the grid elsewhere.  The value of every element is a function of its own
    row alone: the two assignments write the same bits (forward and backward, column blocks of wider buffers, a row count that
    is no multiple of anything); the column sums taken on the way (the bias gradient) add the same values in another order."""
    V = 100003
    g = torch.Generator(device=DEV).manual_seed(C)
    wide = torch.randn((V, 3 * C), device=DEV, generator=g).to(dtype)
    x, da = wide[:, C:2 * C], wide[:, 2 * C:]
    vec = [torch.rand(C, device=DEV, generator=g) + 0.5 for _ in range(7)]
    res = {}
    try:
        for rows in (1, 2):
            capi.tuning_set(capi.TUNE_BN_ROWS, rows)
            outw = torch.zeros((V, 2 * C), device=DEV, dtype=dtype)
            y = capi.scale_shift_act(x, vec[0], vec[1], 0.01, out=outw[:, C:])
            dh, sums = capi.bn_act_bwd_apply_colsum(da, x, *vec, 0.01)
            assert bool((outw[:, :C] == 0).all())
            res[rows] = (y.clone(), dh, sums)
    finally:
        capi.tuning_set(capi.TUNE_BN_ROWS, 0)
    assert torch.equal(res[1][0], res[2][0]) and torch.equal(res[1][1], res[2][1])
    if res[1][2] is not None:
        ref = res[1][1].double().sum(0)
        for rows in (1, 2):
            assert float((res[rows][2].double() - ref).abs().max()) <= 2e-5 * float(res[1][1].double().abs().sum(0).max())


def test_graph_prepare_builds_the_tile_records_ahead_of_the_first_aggregation():
    """sg_graph_prepare: the tile records that the first 128- / 256-channel aggregation would build -- an allocation and
    two stream synchronisations inside sg_spmm -- built ahead of time; idempotent, a no-op for widths that use no records, and the
    aggregation that follows gives the bits of one on a graph that built them lazily."""
    m = synth.torus_mesh(96, 64)
    V = m.num_vertices
    ei = torch.from_numpy(m.edge_index).to(DEV)
    lazy, ahead = _ring_graph(ei, V), _ring_graph(ei, V)
    gen = torch.Generator(device=DEV).manual_seed(3)
    for dtype in (torch.bfloat16, torch.float32):
        x = torch.randn(V, 256, device=DEV, generator=gen).to(dtype)
        ahead.prepare(64, dtype)              # no records for this width: nothing happens
        ahead.prepare(256, dtype)
        ahead.prepare(256, dtype)             # idempotent
        a = ahead.spmm(x, torch.empty_like(x))
        b = lazy.spmm(x, torch.empty_like(x))
        assert torch.equal(a, b)
        assert rel(a.float(), oracle_lhat(ei.cpu(), x.float().cpu())) < (1e-6 if dtype == torch.float32 else 1e-2)
