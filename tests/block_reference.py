"""ONE ``[ChebConv -> pool? -> BatchNorm1d -> LeakyReLU]`` block on the CPU with plain autograd: the independent reference
of ``sg_block_forward`` / ``sg_block_backward`` (tests/test_gpu_block_gradients.py).  TEST INFRASTRUCTURE ONLY.

Built from parts that are pinned elsewhere: ``oracle.pyg_restatement.ChebConv`` (golden g1, tests/test_oracle.py),
``oracle.models.pool_mean`` / ``unpool_gather``, ``torch.nn.BatchNorm1d`` in training or eval mode, and
``golden_util.PrescribedLeakyReLU`` -- an activation whose sign pattern is GIVEN, so that two evaluations of the block sit on
the same linear branch.  (LeakyReLU keeps the sign: the pattern of an implementation under test is ``y > 0`` of its output.)

  * ``dtype=torch.float64``: the reference;
  * ``dtype=torch.float32``: the same composition in the precision of the code under test -- its distance from the float64
    run is the YARDSTICK for everything fp32 rounding moves;
  * ``bf16_storage=True``: the composition with bf16 roundings at the stored rows (``oracle.bf16.ChebConvBf16``, the stored
    activation output, the stored pooled rows): the yardstick of the bf16-feature path.

``run_block`` returns y, dx, the K weight gradients, the conv-bias / gamma / beta gradients, the BatchNorm buffers after the
call, and dH -- the gradient that arrives at the conv output, whose column sums ARE the conv-bias gradient.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

import golden_util as GU
from oracle import bf16 as OB
from oracle import models as OM
from oracle.pyg_restatement import ChebConv

#: host threads of the float32 / bf16-storage yardstick runs: ATen splits its fp32 sums by the thread count, so the
#: yardstick is one fixed draw of that rounding noise (as BF16_BLOCK_ORACLE_THREADS in test_gpu_config_parity.py)
YARDSTICK_THREADS = 16


class BlockParams:
    """The parameters and buffers of one block as CPU float32 tensors (whatever device they came from)."""

    def __init__(self, weights: Sequence[torch.Tensor], bias: Optional[torch.Tensor], gamma, beta, running_mean, running_var,
                 eps: float = 1e-5, momentum: float = 0.1, slope: float = 0.01):
        cpu = lambda t: None if t is None else t.detach().cpu().float().clone()      # noqa: E731
        self.weights = [cpu(w) for w in weights]
        self.bias, self.gamma, self.beta = cpu(bias), cpu(gamma), cpu(beta)
        self.running_mean, self.running_var = cpu(running_mean), cpu(running_var)
        self.eps, self.momentum, self.slope = eps, momentum, slope

    @property
    def K(self):
        return len(self.weights)


def build_modules(p: BlockParams, dtype, bf16_storage: bool = False, post: bool = True):
    cout, cin = p.weights[0].shape
    conv = (OB.ChebConvBf16 if bf16_storage else ChebConv)(cin, cout, K=p.K, bias=p.bias is not None)
    if bf16_storage:
        conv.post_when_narrowing = post
    bn = torch.nn.BatchNorm1d(cout, eps=p.eps, momentum=p.momentum)
    with torch.no_grad():
        for lin, w in zip(conv.lins, p.weights):
            lin.weight.copy_(w)
        if p.bias is not None:
            conv.bias.copy_(p.bias)
        bn.weight.copy_(p.gamma)
        bn.bias.copy_(p.beta)
        bn.running_mean.copy_(p.running_mean)
        bn.running_var.copy_(p.running_var)
    return conv.to(dtype), bn.to(dtype)


def apply_block(conv, bn, x, weights, bias, gamma, beta, edge_index, *, mask=None, slope: float = 0.01, pool=None,
                pool_hash=None, store=lambda t: t):
    """The block as a FUNCTION of its input and parameters (``conv`` / ``bn`` supply structure, mode and buffers; their
    own parameters are not read): what run_block differentiates and what torch.autograd.gradcheck is run on.  Returns
    y, the conv output h, the BatchNorm output z and the activation module (its flip counters)."""
    pd = {f"lins.{k}.weight": w for k, w in enumerate(weights)}
    if bias is not None:
        pd["bias"] = bias
    h = torch.func.functional_call(conv, pd, (x, edge_index))
    hp = h
    if pool == "pool":
        hp = store(OM.pool_mean(pool_hash, h))
    elif pool == "unpool":
        hp = store(OM.unpool_gather(pool_hash, h))
    z = torch.func.functional_call(bn, {"weight": gamma, "bias": beta}, (hp,))
    if mask is None:
        mask = z.detach() > 0
    act = GU.PrescribedLeakyReLU([mask], negative_slope=slope)
    return store(act(z)), h, z, act


def run_block(p: BlockParams, edge_index: torch.Tensor, x: torch.Tensor, dy: torch.Tensor, *, train: bool,
              dtype=torch.float64, mask: Optional[torch.Tensor] = None, pool: Optional[str] = None,
              pool_hash: Optional[np.ndarray] = None, bf16_storage: bool = False, post: bool = True,
              threads: Optional[int] = None) -> Dict[str, object]:
    """Forward and backward of the block for the loss ``sum(y * dy)``.  ``mask`` (bool, y's shape): the activation
    pattern to apply; None: the block's own ``z > 0``.  ``pool``: None, "pool" or "unpool" with ``pool_hash`` [n, 2]
    (fine vertex, coarse vertex).  Returns a dict of CPU tensors of ``dtype`` plus the activation module's counters:
    ``flips`` / ``elements`` (pattern entries that differ from the block's own sign) and ``max_flip_z`` (their largest
    |z| / rms z)."""
    old = torch.get_num_threads()
    if threads is not None:
        torch.set_num_threads(threads)
    try:
        conv, bn = build_modules(p, dtype, bf16_storage, post)
        conv.train(train), bn.train(train)
        leaf = lambda t: None if t is None else t.detach().cpu().to(dtype).clone().requires_grad_(True)      # noqa: E731
        x, ws, b, gamma, beta = leaf(x), [leaf(w) for w in p.weights], leaf(p.bias), leaf(p.gamma), leaf(p.beta)
        y, h, z, act = apply_block(conv, bn, x, ws, b, gamma, beta, edge_index.cpu(), mask=None if mask is None else mask.cpu(),
                                   slope=p.slope, pool=pool, pool_hash=pool_hash, store=OB.round_st if bf16_storage else (lambda t: t))
        h.retain_grad()
        (y * dy.detach().cpu().to(dtype)).sum().backward()
        return {"y": y.detach(), "dx": x.grad, "dW": [w.grad for w in ws], "db": None if b is None else b.grad,
                "dgamma": gamma.grad, "dbeta": beta.grad,
                "running_mean": bn.running_mean.detach().clone(), "running_var": bn.running_var.detach().clone(),
                "dH": h.grad, "z": z.detach(), "mask": act.masks[0],
                "flips": act.flips, "elements": act.elements, "max_flip_z": act.max_flip_z}
    finally:
        torch.set_num_threads(old)


# ---- what is compared ------------------------------------------------------------------------------------------------------
def bias_cancellation_error(db: torch.Tensor, ref: Dict[str, object]) -> float:
    """The conv-bias gradient behind a TRAINING-mode BatchNorm is zero in exact arithmetic: a sum of dH entries that
    cancel.  Error = worst column of |db - db_ref| / sum |dH| (float64 reference): the rounding of the sum relative to what
    was summed.  A value that was never computed (stale or uninitialised memory, a missing accumulation) is O(1) or NaN on
    this scale, which NaN-propagating ``max`` turns into a failure."""
    dH = ref["dH"].double()
    scale = dH.abs().sum(0).clamp_min(1e-300)
    e = ((db.detach().cpu().double() - ref["db"].double()).abs() / scale)
    return float("inf") if not bool(torch.isfinite(e).all()) else float(e.max())


def errors(got: Dict[str, object], ref: Dict[str, object], train: bool, scale: float = 1.0) -> Dict[str, float]:
    """Per tensor KIND the worst error of ``got`` against the float64 ``ref`` (parameter gradients: against ``scale`` x
    the reference, for gradients accumulated over ``scale`` identical passes): relative L2, except the
    training-mode conv-bias gradient (bias_cancellation_error), which is a kind of its own.  Kinds: y, dx, dW (worst of
    the K matrices), db (eval mode) or db0 (training mode), dbn (worst of d gamma / d beta), bn (running statistics, worst
    relative max-norm)."""
    def rel(a, b, s=scale):
        a = a.detach().cpu().double()
        if not bool(torch.isfinite(a).all()):
            return float("inf")
        return GU.rel_l2(a.numpy(), (s * b.double()).numpy())
    out = {}
    if "y" in got:
        out["y"] = rel(got["y"], ref["y"], 1.0)
    if got.get("dx") is not None:
        out["dx"] = rel(got["dx"], ref["dx"], 1.0)
    out["dW"] = max(rel(a, b) for a, b in zip(got["dW"], ref["dW"]))
    if ref["db"] is not None:
        if train:
            scaled = dict(ref, db=scale * ref["db"].double(), dH=scale * ref["dH"].double())
            out["db0"] = bias_cancellation_error(got["db"], scaled)
        else:
            out["db"] = rel(got["db"], ref["db"])
    out["dbn"] = max(rel(got["dgamma"], ref["dgamma"]), rel(got["dbeta"], ref["dbeta"]))
    if "running_mean" in got:
        out["bn"] = max(float((got[k].detach().cpu().double() - ref[k].double()).abs().max() / ref[k].double().abs().max())
                        for k in ("running_mean", "running_var"))
    return out
