"""PointNet++/DGCNN-style edge convolution.

Capability parity with reference model/flot/gconv.py (SetConv): gather the k
neighbours' features, subtract the centre, concatenate the 3-d edge offset,
then Conv2d 1x1 -> GroupNorm(8) -> LeakyReLU(0.1) -> max over k ->
(Conv1d -> GN -> LReLU) x 2.  Channel rule gconv.py:21-24: mid = out//2 when
in is odd else (in+out)//2; all convs bias-free (gconv.py:26-33).

Parameter names (fc1/gn1/fc2/gn2/fc3/gn3) match the reference so its
checkpoints load directly.  The gather+concat runs through the fused HIP op
on GPU (ops.gather_edge_concat) instead of the flattened fancy-indexing of
gconv.py:64-66.
"""

from __future__ import annotations

import os

import torch
import torch.nn as nn
from torch import Tensor

from pvraft_amd import ops
from .graph import Graph
from .norm import FusedGroupNorm
from .pointwise import PwConv1d, PwConv2d


class SetConv(nn.Module):
    def __init__(self, in_ch: int, out_ch: int):
        super().__init__()
        mid = out_ch // 2 if in_ch % 2 != 0 else (out_ch + in_ch) // 2
        self.fc1 = PwConv2d(in_ch + 3, mid, 1, bias=False)
        self.gn1 = FusedGroupNorm(8, mid, act="lrelu", slope=0.1)
        self.fc2 = PwConv1d(mid, out_ch, 1, bias=False)
        self.gn2 = FusedGroupNorm(8, out_ch, act="lrelu", slope=0.1)
        self.fc3 = PwConv1d(out_ch, out_ch, 1, bias=False)
        self.gn3 = FusedGroupNorm(8, out_ch, act="lrelu", slope=0.1)

    def forward(self, feats: Tensor, graph: Graph) -> Tensor:
        """feats (B, N, C) -> (B, N, out_ch); both usually free views of
        channel-major tensors (see forward_cn)."""
        xyz_feats = feats is graph.xyz
        return self.forward_cn(
            feats.transpose(1, 2), graph, _xyz_feats=xyz_feats
        ).transpose(1, 2)

    def forward_cn(self, f_cn: Tensor, graph: Graph, _xyz_feats: bool = False) -> Tensor:
        """f_cn (B, C, N) -> (B, out_ch, N), channel-major in and out (the
        flow head calls this directly on the GRU state).

        Reference order gconv.py:71-83: conv -> GN -> lrelu (-> max over
        neighbours after stage 1).  LeakyReLU is fused into each GroupNorm.

        GPU path (stage 1): fc1 is linear in the edge vector and the edge
        vector is a difference of per-point [feats; xyz] vectors, so
            fc1(edge(n, j)) = Wg[idx[n, j]] - Wg[n],  Wg = fc1_W @ [feats; xyz]
        -- the GEMM runs over N points (not K*N edges, 32x less) and the
        gather-diff + GN + lrelu + max-pool fuse into the edge_gnmp kernels
        over the (B, N, mid) Wg tensor; the reference's (B, C+3, K, N) and
        (B, mid, K, N) tensors (gconv.py:64-68) never exist.  CPU /
        reference mode keeps the explicit composition.

        bf16 autocast: W @ [feats; xyz] = W[:, :C] @ feats + W[:, C:] @ xyz
        is one two-part pw_fused launch that stores Wg point-major from its
        epilogue, and edge_gnmp writes the pooled result channel-major --
        no cat and no transposes around stage 1.  The weight slices are
        views (of the parameter, of its bf16 mirror and of its .grad), so
        they cost no launches.  PVRAFT_SETCONV_LAYOUT=classic restores the
        cat + GEMM + transpose composition.
        """
        if (
            f_cn.is_cuda
            and ops.hip_available()
            and os.environ.get("PVRAFT_REF_OPS", "0") != "1"
        ):
            dt = (
                torch.get_autocast_dtype("cuda")
                if torch.is_autocast_enabled()
                else f_cn.dtype
            )
            if dt == torch.bfloat16 and torch.is_autocast_enabled() and ops.channel_major_layout():
                from . import pointwise
                from .pointwise import pw_fused

                C = f_cn.shape[1]
                w = self.fc1.weight.view(self.fc1.out_channels, -1)
                tf = tx = None
                if pointwise.wgrad_defer_active():
                    gw = pointwise._grad_buffer(self.fc1.weight).view(w.shape)
                    tf, tx = gw[:, :C], gw[:, C:]
                xyz_cn = graph.xyz_cn(dt)
                wg_t = pw_fused(
                    [(w[:, :C], xyz_cn if _xyz_feats else f_cn, tf),
                     (w[:, C:], xyz_cn, tx)],
                    out_point_major=True,
                )  # (B, N, mid)
                x = ops.edge_gnmp(
                    wg_t, graph.idx32, graph.csr(), self.gn1.num_groups,
                    self.gn1.weight, self.gn1.bias, self.gn1.eps,
                    act="lrelu", slope=0.1, channel_major_out=True,
                )  # (B, mid, N)
            else:
                g = torch.cat([f_cn.to(dt), graph.xyz.transpose(1, 2).to(dt)], dim=1)
                from .pointwise import pw_matmul

                wg = pw_matmul(self.fc1.weight.view(self.fc1.out_channels, -1), g,
                               targets=(self.fc1.weight, None))
                wg_t = ops.transpose_last2(wg)  # (B, N, mid)
                y_t = ops.edge_gnmp(
                    wg_t, graph.idx32, graph.csr(), self.gn1.num_groups,
                    self.gn1.weight, self.gn1.bias, self.gn1.eps,
                    act="lrelu", slope=0.1,
                )
                x = ops.transpose_last2(y_t)  # (B, mid, N)
        else:
            feats = f_cn.transpose(1, 2)
            x = ops.gather_edge_concat(feats, graph.idx, graph.xyz, csr=graph.csr())
            x = self.fc1(x)
            x = ops.group_norm_act_maxpool(
                x, self.gn1.num_groups, self.gn1.weight, self.gn1.bias,
                self.gn1.eps, act="lrelu", slope=0.1,
            )  # B, mid, N
        x = self.gn2(self.fc2(x))
        x = self.gn3(self.fc3(x))
        return x
