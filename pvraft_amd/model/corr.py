"""Point-voxel correlation fields (reference model/corr.py: CorrBlock).

The paper's core op.  Once per pair: the all-pair feature correlation
fmap1^T fmap2 / sqrt(C) is truncated to the top-K columns per row together
with the matching xyz2 positions (reference corr.py:31-42).  Per GRU
iteration the truncated field is queried at the current coords through two
branches (corr.py:44-93):

* voxel branch: 3-level voxel pyramid of mean correlations in a 3^3 cube
  (cell size base_scale * 2^i) -> Conv1d 81->128, GN(8), PReLU, Conv1d
  128->64.
* kNN branch: 32 nearest truncated candidates, [corr; rel-xyz] -> Conv2d
  4->64, GN(8), PReLU, max over k, Conv1d 64->64.

Redesign vs the reference: the truncated field is an explicit value object
(CorrField) returned by ``CorrBlock.build`` instead of mutable attributes
set by ``init_module`` (corr.py:31-42) -- stateless forward, safe under any
process/stream layout.  The scatter/gather math runs in single fused HIP
kernels on GPU (ops.voxel_corr / ops.knn_corr) with no torch_scatter and no
(B, N, K)-sized quantisation intermediates.

Parameter names (out_conv.0/1/2/3, knn_conv.0/1/2, knn_out) match the
reference so its checkpoints load directly.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn as nn
from torch import Tensor

from pvraft_amd import ops
from .norm import FusedGroupNorm, PReLUAny
from .pointwise import PwConv1d, PwConv2d


@dataclass
class CorrField:
    corr: Tensor  # (B, N, K) truncated correlation values (top-K SET,
    #               unordered: every consumer is order-invariant)
    xyz: Tensor   # (B, N, K, 3) positions of the selected candidates in pc2


class CorrBlock(nn.Module):
    def __init__(
        self,
        num_levels: int = 3,
        base_scale: float = 0.25,
        resolution: int = 3,
        truncate_k: int = 512,
        knn: int = 32,
    ):
        super().__init__()
        self.truncate_k = truncate_k
        self.num_levels = num_levels
        self.resolution = resolution
        self.base_scale = base_scale
        self.knn = knn
        self.out_conv = nn.Sequential(
            PwConv1d((resolution ** 3) * num_levels, 128, 1),
            FusedGroupNorm(8, 128),
            PReLUAny(),
            PwConv1d(128, 64, 1),
        )
        self.knn_conv = nn.Sequential(
            PwConv2d(4, 64, 1),
            FusedGroupNorm(8, 64),
            PReLUAny(),
        )
        self.knn_out = PwConv1d(64, 64, 1)

    def build(self, fmap1: Tensor, fmap2: Tensor, xyz2: Tensor) -> CorrField:
        """Compute the truncated correlation field (once per pair)."""
        # the index is not used here: take it as the kernels made it
        corr, _idx, txyz = ops.corr_truncate(
            fmap1, fmap2, xyz2, self.truncate_k, index_dtype=torch.int32
        )
        return CorrField(corr=corr, xyz=txyz)

    def forward(self, field: CorrField, coords: Tensor) -> Tensor:
        """Query the field at coords (B, N, 3) -> (B, 64, N).

        One fused kernel pass produces both raw lookups (voxel pyramid +
        kNN candidates); the two small conv pipelines then run on them.
        """
        vox, knn_raw = ops.pv_corr_lookup(
            field.corr, field.xyz, coords, self.base_scale, self.num_levels,
            self.knn, self.resolution,
        )
        return self._voxel_conv(vox) + self._knn_conv(knn_raw)

    def _voxel_feature(self, field: CorrField, coords: Tensor) -> Tensor:
        feat = ops.voxel_corr(
            field.corr, field.xyz, coords, self.base_scale, self.num_levels, self.resolution
        )  # B, L*R^3, N
        return self._voxel_conv(feat)

    def _voxel_conv(self, feat: Tensor) -> Tensor:
        # out_conv = Sequential(conv, GN, PReLU, conv) by state-dict layout;
        # executed with GN+PReLU fused (learnable slope = out_conv[2].weight)
        conv1, gn, prelu, conv2 = self.out_conv[0], self.out_conv[1], self.out_conv[2], self.out_conv[3]
        x = conv1(feat)
        x = ops.group_norm_act(
            x, gn.num_groups, gn.weight, gn.bias, gn.eps, act="prelu", slope_t=prelu.weight
        )
        return conv2(x)

    def _knn_feature(self, field: CorrField, coords: Tensor) -> Tensor:
        feat = ops.knn_corr(field.corr, field.xyz, coords, self.knn)  # B, 4, k, N
        return self._knn_conv(feat)

    def _knn_conv(self, feat: Tensor) -> Tensor:
        # knn_conv = Sequential(conv, GN, PReLU) + max over the k axis
        conv, gn, prelu = self.knn_conv[0], self.knn_conv[1], self.knn_conv[2]
        import os

        if (
            feat.is_cuda
            and ops.hip_available()
            and feat.dtype == torch.float32
            and conv.out_channels % 16 == 0
            and os.environ.get("PVRAFT_REF_OPS", "0") != "1"
            and os.environ.get("PVRAFT_NO_KNN_GNMP", "0") != "1"
        ):
            # one fused pipeline: the conv contraction is only 4-wide, so
            # it is evaluated inline with GN+PReLU+maxpool and the
            # (B, 64, k, N) activation never exists at all
            feat = ops.knn_gnmp(
                feat, conv.weight, conv.bias, gn.num_groups, gn.weight,
                gn.bias, gn.eps, prelu.weight,
            )  # B, 64, N
        else:
            feat = conv(feat)
            feat = ops.group_norm_act_maxpool(
                feat, gn.num_groups, gn.weight, gn.bias, gn.eps, act="prelu",
                slope_t=prelu.weight,
            )  # B, 64, N
        return self.knn_out(feat)
