"""``-m gpu``: every tensor one block call returns -- y, dx, the K weight gradients, the conv-bias gradient, d gamma, d beta,
the BatchNorm buffers -- against a float64 reference of the block (tests/block_reference.py), on EVERY weight-gradient
engine behind ``dense_tn`` (csrc/dense.hip) and under every switch that changes which kernel writes which gradient.

Why this file exists.  ``sg_block_backward`` hands the weight gradient to one of seven engines, and since the conv-bias sums
"ride" in the reduce kernel of that engine (GradSink::cs_*), WHICH engine ran decides who writes the bias gradient.  The other
block tests are A/B against the per-module path (same kernels, and the same blind spot for a bias gradient that is zero in
exact arithmetic behind a training-mode BatchNorm).  Here the reference is independent, the conv-bias gradient is measured
on a cancellation-aware scale, and each case ASSERTS the engine the launch trace names, so a change of the dispatch rule
cannot silently move a case off the engine it is there for.

Engines (``ENGINE`` below; trace name in brackets) and the shapes that reach them, from reading dense_tn:
  thin [thin]        N x pitch(Kp) <= 256: 4 -> 16
  mid [thin]         fp32, N, Kp <= 48 and multiples of 4: 16 -> 32 (order 0), 32 -> 16 (order 1); 6 -> 32 at K = 2 (Cin % 4 != 0)
  split [split]      fp32, >= 4096 rows, N, Kp >= 64: 64 -> 128, 256 -> 128 (order 1); 34 -> 64 at K = 2 (Cin % 4 != 0)
  mfma128 [mfma]     bf16, N, Kp multiples of 8: 64 -> 128 (order 0, T kept as planes: sg_block_planar); 32 -> 16 and 64 -> 16
                     (order 1; the library keeps G as planes for 64 -> 16 -- its own choice, not visible to the caller;
                     test_planes_of_a_single_narrow_block_against_column_blocks holds planes against column blocks)
  mfma256 [mfma]     bf16, capi.gemm_tn_takes_big_tile: 256 -> 256 at 20 480 rows
  blas1 [blas]       one hipBLASLt product (fewer than 8192 rows): 32 -> 32 fp32, 4 -> 32 bf16 at 5000 rows
  blas_slabs [blas]  hipBLASLt cut into S = rows / 4096 row slabs + slab_sum: 32 -> 32 fp32 at 20 480 (S = 5, no tail) and
                     50 000 rows (S = 12 slabs of 4166 rows + a tail slab of 8), 4 -> 32 bf16, 6 -> 32 fp32 (Cin % 4 != 0),
                     64 -> 128 fp32 with SG_TUNE_F32_ENGINE = 1 and = 8 (the split engine switched off)
The ``can == false`` branch (Cin % 4 != 0: the engine's reduce does not accumulate, sg_multi_add does) exists for mid and split
and is hit by the two K = 2 cases; the thin engine has no such branch, and no block shape reaches it on the MFMA engines:
they need Kp % 8 == 0 with Kp = K * Cin (order 0, K <= 3) or Kp = Cin (order 1), which forces Cin % 4 == 0.
Crossed with BatchNorm training / eval and four accumulator modes (``MODES``): every case runs all of them; plus, on the
32 -> 32 fp32 slab shape, a pool and an unpool between conv and BatchNorm and K = 2 (K = 1 at 64 -> 32: 32 -> 32 with one
term is a 32 x 32 product, which the mid engine takes); plus the asymmetric graph with isolated vertices.  The partition
phase path (sg_block_run, block.hip) REFUSES eval mode ("the backward phases of a partition block are for training mode")
and its accumulators are driven only through dist.py's process groups, so it has no
eval-mode case here; its conv-bias launch is gated by the same ``sunk`` answer of dense_tn that these cases pin.

What is compared (block_reference.errors): relative L2 against the float64 block evaluated with the HIP forward's activation
pattern; the TRAINING-mode conv-bias gradient (zero in exact arithmetic) as |db - db_ref| / sum |dH| per column, worst
column -- a value that was never written is O(1) or NaN there.  Bound per tensor kind = max(FLOOR, 2 x yardstick), the
yardstick being the same block in float32 on the CPU (fp32 cases) or the bf16-storage oracle block (bf16 cases: inputs and dY
bf16-representable on both sides), both at a fixed thread count; the factor 2 is _assert_fp32_parity's.  A bound is never
derived from the HIP path's own error.  The pattern may differ from the float64 block's own sign on at most 2e-5 of the
elements, each with |z| <= 1e-3 rms(z) (_assert_pattern_only_overridden_at_kinks' numbers; bf16 storage: PATTERN_CAP).  Gradients accumulated over two
passes into zero-filled accumulators are held against 2 x the reference under the same bound and are bit-equal to twice the
gradient of the run without accumulators (0 + g + g == 2 g exactly; every engine here reduces in a fixed order).

bf16 cases, d bias / d gamma / d beta: fp32 sums over rows on both sides, but NOT over the same rows -- the path's stored dH
and H differ from the storage oracle's wherever an fp32 sum lands on the other side of a bf16 rounding boundary (a few per
cent of the elements, one bf16 ulp each), and the block call does not return its dH.  They are therefore bounded like every
other bf16 tensor, by the storage oracle's own distance from the float64 block.

Measured on an MI355X (this change on top of a036c9f; worst case over the engine's cases, both BatchNorm modes and all four
accumulator modes).  Error against the float64 block: yardstick / HIP path.  db0: training-mode conv-bias gradient on its
cancellation scale; db: eval mode; dbn: d gamma, d beta; bn: running statistics (training mode; untouched in eval mode: 0).

  engine      dtype   y                dx               dW               db               db0              dbn              bn
  thin        fp32    1.2e-7 / 1.2e-7  1.4e-7 / 1.3e-7  3.1e-6 / 3.6e-7  2.1e-7 / 2.7e-7  2.7e-8 / 3.9e-8  6.1e-7 / 1.8e-7  6.7e-8 / 6.7e-8
  mid         fp32    1.5e-7 / 1.5e-7  1.6e-7 / 1.6e-7  2.9e-6 / 4.2e-7  1.7e-7 / 1.3e-7  3.5e-8 / 2.5e-8  8.0e-7 / 2.2e-7  7.5e-8 / 8.0e-8
  split       fp32    2.3e-7 / 2.4e-7  2.3e-7 / 3.8e-7  7.9e-7 / 3.0e-7  1.6e-7 / 1.0e-7  4.1e-8 / 2.8e-8  9.4e-7 / 3.0e-7  1.1e-7 / 1.0e-7
  blas1       fp32    1.3e-7 / 2.0e-7  1.4e-7 / 1.3e-7  3.0e-7 / 1.3e-6  1.2e-7 / 1.6e-7  2.8e-8 / 2.2e-8  4.1e-7 / 2.4e-7  7.6e-8 / 7.6e-8
  blas_slabs  fp32    1.8e-7 / 2.7e-7  2.3e-7 / 2.2e-7  2.7e-6 / 1.2e-6  2.1e-7 / 2.0e-7  4.4e-8 / 2.8e-8  1.6e-6 / 3.1e-7  9.3e-8 / 9.7e-8
  thin        bf16    3.1e-3 / 3.1e-3  3.5e-3 / 3.5e-3  3.6e-3 / 3.6e-3  1.8e-3 / 1.8e-3  1.8e-4 / 1.8e-4  3.0e-3 / 3.0e-3  2.0e-4 / 2.0e-4
  mfma128     bf16    3.5e-3 / 3.5e-3  3.4e-3 / 3.4e-3  2.7e-3 / 2.7e-3  2.0e-3 / 2.0e-3  2.2e-4 / 2.2e-4  2.6e-3 / 2.6e-3  1.7e-4 / 1.7e-4
  mfma256     bf16    3.1e-3 / 3.1e-3  3.4e-3 / 3.4e-3  2.5e-3 / 2.5e-3  1.6e-3 / 1.6e-3  6.8e-4 / 6.8e-4  2.6e-3 / 2.6e-3  7.1e-5 / 7.1e-5
  blas1       bf16    3.1e-3 / 3.1e-3  3.5e-3 / 3.5e-3  2.8e-3 / 2.8e-3  2.0e-3 / 2.0e-3  9.5e-5 / 9.5e-5  2.6e-3 / 2.6e-3  1.2e-4 / 1.2e-4
  blas_slabs  bf16    3.1e-3 / 3.1e-3  3.5e-3 / 3.5e-3  3.7e-3 / 3.7e-3  1.8e-3 / 1.8e-3  7.6e-5 / 7.7e-5  2.7e-3 / 2.7e-3  1.1e-4 / 1.1e-4
  largest yardstick, fp32:   y 2.3e-7, dx 2.3e-7, dW 3.1e-6, db 2.1e-7, db0 4.4e-8, dbn 1.6e-6, bn 1.1e-7   -> FLOOR[F32]
  largest yardstick, bf16:   y 3.5e-3, dx 3.5e-3, dW 3.7e-3, db 2.0e-3, db0 6.8e-4, dbn 3.0e-3, bn 2.0e-4   -> FLOOR[BF16]
Activation pattern against the float64 block's own sign: fp32 no element of any case differs; bf16 at most
7.9e-4 of the elements, |z| <= 1.1e-2 rms.  (In bf16 both sides sit at the distance bf16 storage itself puts between the block
and exact arithmetic; what the bf16 rows add over the fp32 ones is the engine assertion, the accumulator bookkeeping and the
bit-equality of accumulated gradients.)  On a036c9f itself the 22 slab-engine cases fail, on the conv-bias gradient only
and only with weight accumulators: accumulators on every parameter -- nothing is added (eval mode: relative error 1.0;
training mode: caught by the bit comparison with the run without accumulators); weights only -- dvec[5] is never written
and Python returns what the buffer held (eval mode: error 1.0 .. 2.2; training mode: 2e-4 .. 1.4e-1 on the cancellation
scale against a bound of 1e-7).
"""
import contextlib
import math

import pytest
import torch

import block_reference as BR
from semigcn_amd import capi, functional as F_sg, synth
from semigcn_amd.graph import MeshGraph
from test_gpu_blocks import _block_module

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16

MESHES = {1200: (40, 30), 5000: (100, 50), 20480: (160, 128), 50000: (250, 200)}
MODES = ("none", "all", "weights", "bias_bn")
#: max(FLOOR, 2 x yardstick) bounds every kind.  fp32: the smallest power of ten above 2 x the largest float32-block error
#: of the kind over the whole matrix (table above); every one is below sqrt(rows) x 2^-24 x 8 -- a random-walk fp32 sum with
#: one digit of slack -- already at the smallest row count of the matrix (1.65e-5 at 1200 rows; 1.07e-4 at 50 000).
#: bf16: the same rule on the storage oracle's errors.  db0: the training-mode conv-bias gradient on its cancellation scale.
FLOOR = {F32: {"y": 1e-6, "dx": 1e-6, "dW": 1e-5, "db": 1e-6, "db0": 1e-7, "dbn": 1e-5, "bn": 1e-6},
         BF16: {"y": 1e-2, "dx": 1e-2, "dW": 1e-2, "db": 1e-2, "db0": 1e-2, "dbn": 1e-2, "bn": 1e-3}}
#: how far the prescribed pattern may sit from the float64 block's own sign: (fraction of the elements, largest |z| / rms z).
#: fp32: _assert_pattern_only_overridden_at_kinks' numbers.  bf16: the path STORES the BatchNorm input H in bf16, so its z is
#: off by up to half a bf16 ulp of H -- 2^-9 |H| / sigma_H x gamma, with |H| a few sigma and gamma <= 1.5 -- which no choice
#: of inputs avoids: a sign can differ wherever |z| is below that.  Fraction: the density of a unit normal at zero (0.4) x one
#: bf16 ulp (2^-8) x 1 = 1.6e-3; largest |z|: 8 x 2^-8 (|H| up to ~5 sigma x gamma 1.5, rounded up to a power of two).
PATTERN_CAP = {F32: (2e-5, 1e-3), BF16: (0.4 * 2.0 ** -8, 8 * 2.0 ** -8)}


def _case(rows, cin, cout, dtype, engine, K=3, knob=None, pool=None, graph="torus", seed=0):
    name = f"{engine}-{rows}-{cin}to{cout}-{'f32' if dtype == F32 else 'bf16'}" + (f"-K{K}" if K != 3 else "") + \
        (f"-knob{knob}" if knob is not None else "") + (f"-{pool}" if pool else "") + ("-asym" if graph != "torus" else "")
    return pytest.param(dict(rows=rows, cin=cin, cout=cout, dtype=dtype, engine=engine, K=K, knob=knob, pool=pool, graph=graph,
                             seed=seed), id=name)


CASES = [
    _case(1200, 4, 16, F32, "thin"), _case(1200, 4, 16, BF16, "thin"),
    _case(20480, 4, 16, F32, "thin"), _case(20480, 4, 16, BF16, "thin"),
    _case(20480, 16, 32, F32, "mid"), _case(20480, 32, 16, F32, "mid"),
    _case(20480, 6, 32, F32, "mid", K=2),
    _case(5000, 64, 128, F32, "split"), _case(20480, 64, 128, F32, "split"),
    _case(5000, 256, 128, F32, "split"), _case(20480, 256, 128, F32, "split"),
    _case(20480, 34, 64, F32, "split", K=2),
    _case(20480, 64, 128, BF16, "mfma128"), _case(20480, 32, 16, BF16, "mfma128"), _case(20480, 64, 16, BF16, "mfma128"),
    _case(20480, 256, 256, BF16, "mfma256"),
    _case(5000, 32, 32, F32, "blas1"), _case(5000, 4, 32, BF16, "blas1"),
    _case(20480, 32, 32, F32, "blas_slabs"), _case(50000, 32, 32, F32, "blas_slabs"),
    _case(20480, 4, 32, BF16, "blas_slabs"),
    _case(20480, 64, 128, F32, "blas_slabs", knob=1), _case(20480, 64, 128, F32, "blas_slabs", knob=8),
    _case(20480, 6, 32, F32, "blas_slabs"),
    _case(20480, 32, 32, F32, "blas_slabs", pool="pool"), _case(20480, 32, 32, F32, "blas_slabs", pool="unpool"),
    _case(20480, 64, 32, F32, "blas_slabs", K=1), _case(20480, 32, 32, F32, "blas_slabs", K=2),
    _case(20480, 32, 32, F32, "blas_slabs", graph="asym"),
]

_mesh_cache = {}


def _mesh(rows, graph):
    """(edge_index on the CPU, vertex count, pool hierarchy or None) -- built once per mesh."""
    key = (rows, graph)
    if key not in _mesh_cache:
        m = synth.torus_mesh(*MESHES[rows])
        V, ei = m.num_vertices, torch.from_numpy(m.edge_index)
        if graph == "asym":     # test_block_call_on_an_asymmetric_graph_with_isolated_vertices' graph
            gen = torch.Generator().manual_seed(48)
            keep = torch.rand(ei.shape[1], generator=gen) > 0.33
            keep |= ei[0] < ei[1]
            ei = ei[:, keep]
            lone = torch.randperm(V, generator=gen)[:7]
            ei = ei[:, ~(torch.isin(ei[0], lone) | torch.isin(ei[1], lone))]
            ei = torch.cat([ei, ei[:, :50], torch.arange(20).repeat(2, 1)], dim=1)
        _mesh_cache[key] = (ei, V, m)
    return _mesh_cache[key]


_pool_cache = {}


def _pool(rows):
    if rows not in _pool_cache:
        _, V, m = _mesh(rows, "torus")
        _pool_cache[rows] = synth.greedy_pool_hierarchy(m.edge_index, V, seed=7)
    return _pool_cache[rows]


@contextlib.contextmanager
def _knob(value):
    if value is None:
        yield
        return
    capi.tuning_set(capi.TUNE_F32_ENGINE, value)
    try:
        yield
    finally:
        capi.tuning_set(capi.TUNE_F32_ENGINE, 0)


def _engine_of(rec, M):
    """The ENGINE name of a "tn" trace record: the trace's engine refined by the library's own shape predicates."""
    e, N, Kp = rec["engine"], rec["b"], rec["c"]
    assert rec["a"] == M, (rec, M)
    if e == "thin":
        return "thin" if capi.thin_shape(N, Kp) else "mid"
    if e == "mfma":
        return "mfma256" if capi.gemm_tn_takes_big_tile(M, N, Kp, N, Kp) else "mfma128"
    if e == "blas":
        return "blas_slabs" if M // 4096 > 1 else "blas1"
    return e


def _params_of(seq):
    conv = seq[0]
    bn = [m for m in seq.modules() if isinstance(m, torch.nn.BatchNorm1d)][0]
    return conv, bn, [lin.weight for lin in conv.lins], [conv.bias, bn.weight, bn.bias]


def _hip(seq, g, x, r, train, mode, state, bystanders, trace=False):
    """One (mode "none") or two accumulated (the other modes, inside sink_param_grads()) forward/backward passes of the
    block on the HIP path, parameters and BatchNorm buffers restored before each.  Returns the tensors of the LAST pass and
    the parameter gradients as they stand in ``.grad`` afterwards."""
    conv, bn, weights, others = _params_of(seq)
    seq.train(train)
    with_acc = {"none": [], "all": weights + others, "weights": weights, "bias_bn": others}[mode]
    without = [p for p in weights + others if not any(p is q for q in with_acc)]
    for p in weights + others:
        p.grad = None
    for p in with_acc:
        p.grad = torch.zeros_like(p)
    acc_ptrs = {id(p): p.grad.data_ptr() for p in with_acc}
    watch = [b.clone() for b in bystanders]
    recs, routed = None, {}
    ctx = F_sg.sink_param_grads() if mode != "none" else contextlib.nullcontext()
    with ctx:
        for it in range(1 if mode == "none" else 2):
            seq.load_state_dict(state)
            xi = x.clone().requires_grad_(True)
            before = list(F_sg.block_calls)
            y = seq(xi, g)
            loss = (y.float() * r).sum()
            if trace and it == 0:
                with capi.LaunchTrace(64, kinds=("tn",)) as tr:
                    loss.backward()
                    torch.cuda.synchronize()
                    recs = tr.records()
            else:
                loss.backward()
            assert F_sg.block_calls == [before[0] + 1, before[1] + 1], "the block path did not serve this block"
            # a parameter WITHOUT an accumulator gets its gradient through autograd, which creates a .grad -- and with it an
            # accumulator for the next pass.  Taken away after every pass, so that both passes run in the mode asked for.
            for p in without:
                assert p.grad is not None, (mode, it)
                routed[id(p)] = p.grad.clone() if it == 0 else routed[id(p)] + p.grad
                p.grad = None
    for p in without:
        p.grad = routed[id(p)]
    torch.cuda.synchronize()
    # what the call must not touch: accumulators stay the tensors they were (added into in place); a parameter without one
    # got its gradient through autograd; accumulators of parameters of ANOTHER block are bit-identical
    for p in weights + others:
        assert p.grad is not None and p.grad.shape == p.shape, mode
        if id(p) in acc_ptrs:
            assert p.grad.data_ptr() == acc_ptrs[id(p)], mode
    for b, w in zip(bystanders, watch):
        assert torch.equal(b, w), "an accumulator of another block was written"
    got = {"y": y.detach().float(), "dx": xi.grad.float(), "dW": [w.grad.clone() for w in weights], "db": conv.bias.grad.clone(),
           "dgamma": bn.weight.grad.clone(), "dbeta": bn.bias.grad.clone(),
           "running_mean": bn.running_mean.clone(), "running_var": bn.running_var.clone()}
    assert int(bn.num_batches_tracked) == int(state[[k for k in state if k.endswith("num_batches_tracked")][0]]) + (1 if train else 0)
    return got, recs


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", CASES)
def test_block_gradients_against_float64_on_every_engine(case, train):
    c = case
    dtype, K, cin, cout = c["dtype"], c["K"], c["cin"], c["cout"]
    ei, V, _ = _mesh(c["rows"], c["graph"])
    pool_op, ph, V_in, V_out = None, None, V, V
    if c["pool"]:
        from semigcn_amd.meshnet import MeshPool, MeshUnpool, pool_hash_to_mask, unpool_hash_to_mask
        ph, ei_c, Vc = _pool(c["rows"])
        if c["pool"] == "pool":
            pool_op, V_out = MeshPool(pool_hash_to_mask(ph)), Vc
        else:
            pool_op, ei, V_in = MeshUnpool(unpool_hash_to_mask(ph)), torch.from_numpy(ei_c), Vc
    g = MeshGraph.from_edge_index(ei.to(DEV), V_in)
    seq = _block_module(cin, cout, pool=pool_op, seed=c["seed"], K=K)
    other = _block_module(cin, cout, seed=c["seed"] + 1, K=K)            # a bystander block with accumulators of its own
    bystanders = []
    for p in other.parameters():
        p.grad = torch.randn_like(p)
        bystanders.append(p.grad)
    conv, bn, weights, others = _params_of(seq)
    with torch.no_grad():
        bn.running_mean.normal_(0.0, 0.1)
        bn.running_var.uniform_(0.5, 1.5)
    gen = torch.Generator().manual_seed(1000 * cin + cout + K)
    x = torch.randn(V_in, cin, generator=gen)
    r = torch.randn(V_out, cout, generator=gen)
    if dtype == BF16:                                                    # bf16-representable on both sides
        x, r = x.bfloat16().float(), r.bfloat16().float()
    xd, rd = x.to(DEV).to(dtype), r.to(DEV)
    state = {k: v.clone() for k, v in seq.state_dict().items()}
    params = BR.BlockParams(weights, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, eps=bn.eps,
                            momentum=bn.momentum, slope=0.01)
    M_tn = V_in

    with _knob(c["knob"]):
        runs = {}
        for mode in MODES:
            runs[mode], recs = _hip(seq, g, xd, rd, train, mode, state, bystanders, trace=mode == "none")
            if mode == "none":
                tn = [t for t in recs if t["kind"] == "tn"]
                assert len(tn) == 1, recs
                assert _engine_of(tn[0], M_tn) == c["engine"], (tn[0], c["engine"])
                post = K >= 2 and cout < cin
                assert (tn[0]["b"], tn[0]["c"]) == ((K * cout, cin) if post else (cout, K * cin)), tn[0]
                if (cin, cout, dtype) == (64, 128, BF16):                # order 0 with T kept as K planes (the caller's choice,
                    blk = capi.sg_block()                                # which functional.py makes whenever the library agrees)
                    blk.graph, blk.dtype, blk.K, blk.V, blk.V_out = g.handle._h, capi._DTYPES[BF16], K, V_in, V_out
                    blk.Cin, blk.Cout, blk.order = cin, cout, 0
                    assert capi.block_planar(blk) and F_sg.USE_PLANES

    # the references: float64 with the HIP forward's pattern, and the yardstick on the same pattern -- once per case
    mask = (runs["none"]["y"] > 0).cpu()
    for mode in MODES[1:]:
        assert torch.equal(runs[mode]["y"], runs["none"]["y"]), f"{mode}: the forward pass is not reproducible"
    kw = dict(train=train, pool=c["pool"], pool_hash=ph)
    ref = BR.run_block(params, ei, x, r, mask=mask, **kw)
    flip_frac = ref["flips"] / ref["elements"]
    yard = BR.run_block(params, ei, x, r, mask=mask, dtype=F32, bf16_storage=dtype == BF16, threads=BR.YARDSTICK_THREADS, **kw)
    e_yard = BR.errors(yard, ref, train)
    print(f"\nCASE {c['engine']} rows={c['rows']} {cin}->{cout} K={K} {'f32' if dtype == F32 else 'bf16'} "
          f"{'train' if train else 'eval'} pool={c['pool']} knob={c['knob']} graph={c['graph']} "
          f"flips={ref['flips']} frac={flip_frac:.1e} max_flip_z={ref['max_flip_z']:.1e}")
    print("  YARD         " + " ".join(f"{k}={v:.2e}" for k, v in e_yard.items()))
    failures = []
    if flip_frac > PATTERN_CAP[dtype][0] or ref["max_flip_z"] > PATTERN_CAP[dtype][1]:
        failures.append(f"activation pattern overridden away from a kink: {ref['flips']} flips, max |z| / rms {ref['max_flip_z']:.2e}")
    for mode in MODES:
        scale = 1.0 if mode == "none" else 2.0
        e = BR.errors(runs[mode], ref, train, scale=scale)
        print(f"  HIP {mode:8s}" + " ".join(f"{k}={v:.2e}" for k, v in e.items()))
        for k, v in e.items():
            bound = max(FLOOR[dtype][k], 2.0 * e_yard[k])
            if not v <= bound:
                failures.append(f"{mode}: {k} error {v:.3e} > {bound:.1e} (yardstick {e_yard[k]:.2e})")
        if mode != "none":                                               # 0 + g + g == 2 g, bit for bit
            one, two = runs["none"], runs[mode]
            pairs = list(zip(two["dW"], one["dW"])) + [(two[k], one[k]) for k in ("db", "dgamma", "dbeta")]
            names = [f"dW{k}" for k in range(K)] + ["db", "dgamma", "dbeta"]
            for n, (a, b) in zip(names, pairs):
                if not torch.equal(a, 2 * b):
                    failures.append(f"{mode}: {n} accumulated over two passes is not twice the single gradient "
                                    f"(max |a - 2 b| = {float((a - 2 * b).abs().max()):.3e}, max |b| = {float(b.abs().max()):.3e})")
            for k in ("dx", "running_mean", "running_var"):
                if not torch.equal(two[k], one[k]):
                    failures.append(f"{mode}: {k} differs from the run without accumulators")
    assert not failures, "\n".join(failures)


def test_floors_are_below_the_random_walk_bound_of_an_fp32_sum():
    """The fp32 floors against sqrt(rows) x 2^-24 x 8 at the SMALLEST row count of the matrix (they are used at every one)."""
    assert all(v <= math.sqrt(min(MESHES)) * 2.0 ** -24 * 8 for v in FLOOR[F32].values())
