"""Training losses (reference tools/loss.py).

compute_loss: masked mean-L1 between estimated and ground-truth flow
(loss.py:34-38).  sequence_loss: exponentially weighted sum over the
per-iteration predictions, weight gamma^(T-1-i) (loss.py:8-11).
self_supervised_loss (absent in the reference): the same gamma weighting of
Chamfer distance + flow smoothness, which needs no ground-truth flow.
"""

from __future__ import annotations

from typing import List, Sequence, Union

import torch
from torch import Tensor


class _SeqLoss(torch.autograd.Function):
    """Fused gamma-weighted sequence loss (csrc/seq_loss.hip): one
    reduction kernel over all T flows + one backward kernel writing all T
    gradients, replacing ~5 (+6 backward) eager kernels per flow."""

    @staticmethod
    def forward(ctx, mask: Tensor, gt: Tensor, gamma: float, *flows):
        from pvraft_amd import _C

        loss, denom = _C.seq_loss_fwd(list(flows), gt, mask, float(gamma))
        ctx.save_for_backward(mask, gt, denom, *flows)
        ctx.gamma = float(gamma)
        return loss

    @staticmethod
    def backward(ctx, dloss: Tensor):
        from pvraft_amd import _C

        mask, gt, denom, *flows = ctx.saved_tensors
        grads = _C.seq_loss_bwd(
            list(flows), gt, mask, dloss.contiguous(), denom, ctx.gamma
        )
        return (None, None, None, *grads)


def _fused_loss(flows, batch, gamma: float):
    """HIP path when every flow is a contiguous fp32 GPU tensor."""
    from pvraft_amd import ops

    gt = batch["ground_truth"][1]
    mask = batch["ground_truth"][0]
    if not (gt.is_cuda and ops._use_hip(gt)) or len(flows) > 32:
        return None
    if gt.dtype != torch.float32 or mask.dtype != torch.float32:
        return None
    for f in flows:
        if not (f.is_cuda and f.dtype == torch.float32 and f.is_contiguous() and f.shape == gt.shape):
            return None
    return _SeqLoss.apply(mask.contiguous(), gt.contiguous(), float(gamma), *flows)


def compute_loss(est_flow: Tensor, batch) -> Tensor:
    fused = _fused_loss([est_flow], batch, 1.0)
    if fused is not None:
        return fused
    return _eager_loss(est_flow, batch)


def sequence_loss(est_flow: Sequence[Tensor], batch, gamma: float = 0.8) -> Tensor:
    n = len(est_flow)
    fused = _fused_loss(list(est_flow), batch, gamma)
    if fused is not None:
        return fused
    loss = 0.0
    for i in range(n):
        loss = loss + (gamma ** (n - i - 1)) * _eager_loss(est_flow[i], batch)
    return loss


def _eager_loss(est_flow: Tensor, batch) -> Tensor:
    mask = batch["ground_truth"][0][..., 0]
    true_flow = batch["ground_truth"][1]
    error = est_flow - true_flow
    # masked mean-L1 (identical to the reference's error[mask > 0].abs().mean(),
    # loss.py:34-38) written with static shapes so the training step is
    # hipGraph-capturable (boolean indexing has a data-dependent shape)
    m = (mask > 0).to(error.dtype)
    total = (error.abs() * m.unsqueeze(-1)).sum()
    count = m.sum() * error.shape[-1]
    return total / count.clamp(min=1)


def self_supervised_loss(
    est_flow: Union[Tensor, Sequence[Tensor]],
    batch,
    gamma: float = 0.8,
    chamfer_weight: float = 1.0,
    smooth_weight: float = 1.0,
    smooth_k: int = 9,
    graph=None,
) -> Tensor:
    """Label-free scene-flow objective over the T per-iteration flows,

      loss = sum_t gamma^(T-1-t) * (chamfer_weight * chamfer_t + smooth_weight * smooth_t)

    chamfer_t: Chamfer distance between pc1 + f_t and pc2 (ops.chamfer_loss);
    smooth_t: mean squared flow difference over pc1's smooth_k-NN graph
    (ops.flow_smoothness).  Reads only batch["sequence"]; ``graph`` may pass
    a prebuilt ``Graph`` of pc1.  ``est_flow`` is one flow or a sequence.
    """
    from pvraft_amd import ops
    from pvraft_amd.model.graph import Graph

    pc1, pc2 = batch["sequence"]
    flows = ops.reference.stack_flows(est_flow)
    if graph is None:
        graph = Graph.build(pc1.detach(), min(int(smooth_k), pc1.shape[1]))
    chamfer = ops.chamfer_loss(pc1, flows, pc2)
    smooth = ops.flow_smoothness(flows, graph)
    n = flows.shape[0]
    weights = torch.tensor(
        [gamma ** (n - 1 - t) for t in range(n)], dtype=chamfer.dtype, device=chamfer.device
    )
    return (weights * (chamfer_weight * chamfer + smooth_weight * smooth.to(chamfer.dtype))).sum()
