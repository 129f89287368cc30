"""tests/block_reference.py -- the float64 reference of one [ChebConv -> pool? -> BatchNorm1d -> LeakyReLU] block that
tests/test_gpu_block_gradients.py holds the HIP block path against -- pinned on the CPU: with its own sign pattern it IS the
plain composition of the oracle's modules, its analytic gradients pass torch.autograd.gradcheck in both BatchNorm modes, and
its error measures see a gradient that was never written."""
import numpy as np
import pytest
import torch

import block_reference as BR
from oracle import models as OM
from oracle.pyg_restatement import ChebConv
from semigcn_amd import synth


def _tiny(cin, cout, K, seed, pool=None):
    m = synth.torus_mesh(6, 5)
    ei, V = torch.from_numpy(m.edge_index), m.num_vertices
    ph = None
    V_in = V_out = V
    if pool is not None:
        ph, ei_c, Vc = synth.greedy_pool_hierarchy(m.edge_index, V, seed=7)
        if pool == "pool":
            V_out = Vc
        else:
            ei, V_in = torch.from_numpy(ei_c), Vc
    gen = torch.Generator().manual_seed(seed)
    a = (6.0 / (cin + cout)) ** 0.5
    p = BR.BlockParams([(torch.rand(cout, cin, generator=gen) * 2 - 1) * a for _ in range(K)],
                       torch.rand(cout, generator=gen) * 0.4 - 0.2, torch.rand(cout, generator=gen) + 0.5,
                       torch.rand(cout, generator=gen) * 0.6 - 0.3, torch.randn(cout, generator=gen) * 0.1,
                       torch.rand(cout, generator=gen) + 0.5)
    x = torch.randn(V_in, cin, generator=gen)
    dy = torch.randn(V_out, cout, generator=gen)
    return p, ei, x, dy, ph


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("pool", [None, "pool", "unpool"])
@pytest.mark.parametrize("K", [1, 3])
def test_reference_block_with_its_own_pattern_is_the_plain_composition(train, pool, K):
    p, ei, x, dy, ph = _tiny(5, 8, K, seed=K, pool=pool)
    got = BR.run_block(p, ei, x, dy, train=train, pool=pool, pool_hash=ph)
    conv = ChebConv(5, 8, K=K).double()
    bn = torch.nn.BatchNorm1d(8).double()
    with torch.no_grad():
        for lin, w in zip(conv.lins, p.weights):
            lin.weight.copy_(w)
        conv.bias.copy_(p.bias)
        bn.weight.copy_(p.gamma), bn.bias.copy_(p.beta)
        bn.running_mean.copy_(p.running_mean), bn.running_var.copy_(p.running_var)
    conv.train(train), bn.train(train)
    xd = x.double().requires_grad_(True)
    h = conv(xd, ei)
    if pool == "pool":
        h = OM.pool_mean(ph, h)
    elif pool == "unpool":
        h = OM.unpool_gather(ph, h)
    y = torch.nn.functional.leaky_relu(bn(h), 0.01)
    (y * dy.double()).sum().backward()
    assert got["flips"] == 0 and got["elements"] == y.numel()
    want = [y.detach(), xd.grad, conv.bias.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var] + \
        [lin.weight.grad for lin in conv.lins]
    have = [got["y"], got["dx"], got["db"], got["dgamma"], got["dbeta"], got["running_mean"], got["running_var"]] + got["dW"]
    for i, (a, b) in enumerate(zip(have, want)):
        assert a.dtype == torch.float64 and torch.equal(a, b), i
    assert torch.allclose(got["db"], got["dH"].sum(0), rtol=1e-12, atol=1e-14)      # d bias = column sums of dH
    if train and pool != "unpool":
        # behind a training-mode BatchNorm the bias gradient cancels to rounding: the measure reads ~1e-16, not ~1
        assert BR.bias_cancellation_error(got["db"], got) == 0.0
        assert float((got["db"].abs() / got["dH"].abs().sum(0)).max()) < 1e-14


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("pool", [None, "pool"])
def test_reference_block_passes_gradcheck(train, pool):
    p, ei, x, dy, ph = _tiny(3, 4, 3, seed=11, pool=pool)
    conv, bn = BR.build_modules(p, torch.float64)
    conv.train(train), bn.train(train)
    leaf = lambda t: t.double().clone().requires_grad_(True)      # noqa: E731
    args = [leaf(x)] + [leaf(w) for w in p.weights] + [leaf(p.bias), leaf(p.gamma), leaf(p.beta)]
    # a FIXED pattern (the block's own at the starting point) keeps the function linear across LeakyReLU's kink
    mask = BR.apply_block(conv, bn, args[0], args[1:4], *args[4:], ei, pool=pool, pool_hash=ph)[2].detach() > 0

    def f(x, w0, w1, w2, b, gamma, beta):
        return BR.apply_block(conv, bn, x, [w0, w1, w2], b, gamma, beta, ei, mask=mask, pool=pool, pool_hash=ph)[0]
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-6, rtol=1e-5)
    # and run_block returns exactly those analytic gradients
    got = BR.run_block(p, ei, x, dy, train=train, mask=mask, pool=pool, pool_hash=ph)
    grads = torch.autograd.grad((f(*args) * dy.double()).sum(), args)
    for a, b in zip([got["dx"]] + got["dW"] + [got["db"], got["dgamma"], got["dbeta"]], grads):
        assert torch.equal(a, b)


def test_float32_and_bf16_storage_runs_are_the_same_block_at_their_precision():
    p, ei, x, dy, _ = _tiny(8, 16, 3, seed=5)
    xb, dyb = x.bfloat16().float(), dy.bfloat16().float()
    ref = BR.run_block(p, ei, xb, dyb, train=True)
    f32 = BR.run_block(p, ei, xb, dyb, train=True, dtype=torch.float32, mask=ref["mask"], threads=1)
    b16 = BR.run_block(p, ei, xb, dyb, train=True, dtype=torch.float32, mask=ref["mask"], bf16_storage=True, threads=1)
    e32, e16 = BR.errors(f32, ref, True), BR.errors(b16, ref, True)
    assert f32["y"].dtype == torch.float32 and torch.equal(b16["y"], b16["y"].bfloat16().float())
    for k in ("y", "dx", "dW", "dbn", "bn"):
        assert e32[k] < 1e-5, (k, e32)
        assert 1e-5 < e16[k] < 3e-2 or k == "bn", (k, e16)
    assert e32["db0"] < 1e-6 and e16["db0"] < 1e-2


@pytest.mark.parametrize("train", [True, False])
def test_error_measures_see_a_gradient_that_was_never_written(train):
    """What the GPU matrix relies on: a conv-bias gradient that is stale, zero, uninitialised or not finite reads as a large
    error in BOTH BatchNorm modes (in training mode the true value is ~0, so a relative L2 could not tell)."""
    p, ei, x, dy, _ = _tiny(8, 16, 3, seed=9)
    ref = BR.run_block(p, ei, x, dy, train=train)
    f32 = BR.run_block(p, ei, x, dy, train=train, dtype=torch.float32, mask=ref["mask"], threads=1)
    key = "db0" if train else "db"
    assert BR.errors(f32, ref, train)[key] < 1e-6
    for bad in (torch.full_like(f32["db"], float("nan")), torch.randn(16), f32["db"] + 1e-3 * ref["dH"].abs().sum(0).float()):
        assert BR.errors(dict(f32, db=bad), ref, train)[key] > 5e-4
    if not train:       # eval mode: the gradient is a real quantity, and a missing accumulation (zero) is 100 % off
        assert BR.errors(dict(f32, db=torch.zeros(16)), ref, train)["db"] == pytest.approx(1.0)
    # gradients accumulated over two passes are held against twice the reference
    twice = dict(f32, dW=[2 * w for w in f32["dW"]], db=2 * f32["db"], dgamma=2 * f32["dgamma"], dbeta=2 * f32["dbeta"])
    e2, e1 = BR.errors(twice, ref, train, scale=2.0), BR.errors(f32, ref, train)
    assert all(e2[k] == pytest.approx(e1[k], rel=1e-6, abs=1e-12) for k in e1)
    assert np.isinf(BR.errors(dict(f32, dW=[w * float("nan") for w in f32["dW"]]), ref, train)["dW"])
