"""Op dispatch layer.

Every hot op has two backends:

* ``pvraft_amd.ops.reference`` -- pure PyTorch, runs anywhere, numerics
  oracle for tests (CPU path).
* ``pvraft_amd._C``            -- hand-written CDNA4 HIP kernels (gfx950),
  built in-tree by ``pvraft_amd.ops.build``.

On a GPU tensor the HIP backend is mandatory: if the extension is missing we
raise instead of silently falling back (a silent eager fallback would fake
GPU coverage).  ``PVRAFT_REF_OPS=1`` explicitly forces the reference backend
(used for on-device A/B numerics tests only).
"""

from __future__ import annotations

import math
import os
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from . import reference

_EXT = None
_EXT_ERR: Optional[str] = None


def _load_ext():
    global _EXT, _EXT_ERR
    if _EXT is None and _EXT_ERR is None:
        try:
            from pvraft_amd import _C  # built in-tree (pvraft_amd/_C*.so)

            _EXT = _C
        except ImportError as e:  # pragma: no cover - exercised on GPU boxes
            _EXT_ERR = str(e)
    return _EXT


def _gn_defer_targets(weight, bias, slope_t, act):
    """fp32 grad-accumulation targets for a GN-family backward when the
    deferred-wgrad step is armed (GradReducer flat views), else None.
    Accumulating inside the extract kernel removes the per-call grad
    tensors and their AccumulateGrad add launches (~190/step)."""
    from pvraft_amd.model import pointwise

    # NOTE: checked in BACKWARD, where the engine runs custom Functions
    # with grad mode DISABLED -- an is_grad_enabled() condition here is
    # always False and silently reroutes every GN weight grad through
    # AccumulateGrad (whose nodes are pinned to the FIRST-backward
    # stream; inside a hipGraph capture that cross-stream write races at
    # replay -- measured 1e13 garbage grads, scripts/graph_step_gradcheck.py)
    if not pointwise._DEFER.on:
        return None
    for t in (weight, bias):
        if not (t.is_leaf and t.requires_grad and t.dtype == torch.float32):
            return None
    st = None
    if act == 2:
        if not (slope_t is not None and slope_t.is_leaf and slope_t.requires_grad):
            return None
        st = pointwise._grad_buffer(slope_t).view(-1)
    return (
        pointwise._grad_buffer(weight).view(-1),
        pointwise._grad_buffer(bias).view(-1),
        st,
    )


def _use_hip(*tensors: Tensor) -> bool:
    if os.environ.get("PVRAFT_REF_OPS", "0") == "1":
        return False
    if not tensors[0].is_cuda:
        return False
    ext = _load_ext()
    if ext is None:
        raise RuntimeError(
            "pvraft_amd HIP extension (pvraft_amd._C) is not built but an op "
            "was called on a GPU tensor. Build it with "
            "`python -m pvraft_amd.ops.build` (requires hipcc, gfx950). "
            f"Import error: {_EXT_ERR}"
        )
    return True


def hip_available() -> bool:
    return _load_ext() is not None


def channel_major_layout() -> bool:
    """SetConv stage 1 / kNN-branch head write their pooled output
    channel-major straight from the kernels; PVRAFT_SETCONV_LAYOUT=classic
    restores the point-major output + separate transpose composition."""
    return os.environ.get("PVRAFT_SETCONV_LAYOUT", "fused") != "classic"


def egnmp_classic() -> tuple:
    """(forward, backward) use the one-gather-per-iteration edge_gnmp
    kernels instead of the batched ones: PVRAFT_EGNMP=classic switches
    both, classic_fwd / classic_bwd one side only (paired A/B runs)."""
    mode = os.environ.get("PVRAFT_EGNMP", "batched")
    return (mode in ("classic", "classic_fwd"), mode in ("classic", "classic_bwd"))


# ---------------------------------------------------------------------------
# autograd wrappers around the HIP kernels
# ---------------------------------------------------------------------------


class _BatchedTranspose(torch.autograd.Function):
    """LDS-tiled (B, R, C) -> (B, C, R) transpose (ATen's strided copy
    path measured ~145 GB/s on this pattern)."""

    @staticmethod
    def forward(ctx, x: Tensor) -> Tensor:
        return _EXT.batched_transpose(x)

    @staticmethod
    def backward(ctx, dy: Tensor):
        return _EXT.batched_transpose(dy.contiguous())


def transpose_last2(x: Tensor) -> Tensor:
    """(B, R, C) -> (B, C, R), contiguous result."""
    # transpose-view of a contiguous tensor: the result IS the underlying
    if x.stride(1) == 1 and x.stride(2) == x.shape[1]:
        return x.transpose(1, 2)
    if (
        x.is_cuda
        and x.dtype in (torch.float32, torch.bfloat16)
        and x.stride(2) == 1
        and x.stride(1) == x.shape[2]
        and os.environ.get("PVRAFT_REF_OPS", "0") != "1"
        and _load_ext() is not None
    ):
        return _BatchedTranspose.apply(x)
    return x.transpose(1, 2).contiguous()


class _GatherEdgeConcat(torch.autograd.Function):
    """out (B,C+3,K,N) = concat(feat[nbr]-feat[center], xyz[nbr]-xyz[center]).

    Backward prefers the deterministic CSR path (inverse adjacency sorted
    by target node, no atomics); falls back to the fp32-atomic scatter when
    no CSR is provided (direct op calls outside a Graph).
    """

    @staticmethod
    def forward(ctx, feats: Tensor, idx: Tensor, xyz: Tensor, order, offsets) -> Tensor:
        ctx.save_for_backward(idx, order, offsets)
        ctx.C = feats.shape[2]
        return _EXT.gather_edge_concat_fwd(feats, idx, xyz)

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        idx, order, offsets = ctx.saved_tensors
        C = ctx.C
        grad_out = grad_out.contiguous()
        if order is not None:
            B, _, K, N = grad_out.shape
            # edge id = j*N + n: a plain last-two-dims transpose of the
            # (B, C, K*N) channel-slice view (LDS-tiled kernel)
            gT = _EXT.batched_transpose(grad_out[:, :C].reshape(B, C, K * N))
            g = _EXT.gather_edge_bwd_csr(gT, order, offsets, K)
        else:
            g = _EXT.gather_edge_concat_bwd(grad_out, idx, C)
        return g, None, None, None, None


class _VoxelCorr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, corr, xyz, coords, base_scale, num_levels, resolution):
        ctx.save_for_backward(xyz, coords)
        ctx.conf = (base_scale, num_levels, resolution)
        return _EXT.voxel_corr_fwd(corr, xyz, coords, base_scale, num_levels, resolution)

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        xyz, coords = ctx.saved_tensors
        base_scale, num_levels, resolution = ctx.conf
        g = _EXT.voxel_corr_bwd(grad_out.contiguous(), xyz, coords, base_scale, num_levels, resolution)
        return g, None, None, None, None, None


class _KnnCorr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, corr, xyz, coords, k):
        out, nbr = _EXT.knn_corr_fwd(corr, xyz, coords, k)
        ctx.save_for_backward(nbr)
        ctx.K = corr.shape[2]
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        (nbr,) = ctx.saved_tensors
        g = _EXT.knn_corr_bwd(grad_out.contiguous(), nbr, ctx.K)
        return g, None, None, None


class _GroupNormAct(torch.autograd.Function):
    """GroupNorm with fused LeakyReLU / learnable-PReLU (HIP, fp32/bf16 IO)."""

    @staticmethod
    def forward(ctx, x, num_groups, weight, bias, eps, act, slope, slope_t):
        w = weight.float().contiguous()
        b = bias.float().contiguous()
        st_ = slope_t.float().reshape(1).contiguous() if slope_t is not None else None
        y, mean, rstd = _EXT.group_norm_act_fwd(x, num_groups, w, b, eps, act, slope, st_)
        ctx.save_for_backward(x, mean, rstd, w, b, st_)
        ctx.conf = (num_groups, act, slope, weight.dtype)
        ctx.params = (weight, bias, slope_t)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, w, b, st_ = ctx.saved_tensors
        num_groups, act, slope, wdtype = ctx.conf
        tgt = _gn_defer_targets(*ctx.params, act)
        if tgt is not None:
            (dx,) = _EXT.group_norm_act_bwd(
                dy.contiguous(), x, mean, rstd, num_groups, w, b, act, slope,
                st_, tgt[0], tgt[1], tgt[2],
            )
            return dx, None, None, None, None, None, None, None
        dx, dw, db, dsl = _EXT.group_norm_act_bwd(
            dy.contiguous(), x, mean, rstd, num_groups, w, b, act, slope, st_,
            None, None, None,
        )
        dslope = dsl.to(wdtype) if act == 2 else None
        return dx, None, dw.to(wdtype), db.to(wdtype), None, None, None, dslope


def group_norm_act(
    x: Tensor,
    num_groups: int,
    weight: Tensor,
    bias: Tensor,
    eps: float = 1e-5,
    act: str = "none",
    slope: float = 0.1,
    slope_t: Optional[Tensor] = None,
) -> Tensor:
    """GroupNorm over (B, C, *spatial) with fused activation.

    act: "none", "lrelu" (constant slope) or "prelu" (learnable scalar
    slope tensor ``slope_t``, gradient included).
    GPU: single HIP pipeline (multi-workgroup reduction; ATen's GroupNorm
    uses one workgroup per (batch, group) which starves MI355X's 256 CUs).
    CPU / reference mode: F.group_norm (+ activation).
    """
    act_id = {"none": 0, "lrelu": 1, "prelu": 2}[act]
    if _use_hip(x):
        shape = x.shape
        y = _GroupNormAct.apply(
            x.reshape(shape[0], shape[1], -1).contiguous(),
            num_groups,
            weight,
            bias,
            eps,
            act_id,
            slope,
            slope_t,
        )
        return y.view(shape)
    y = torch.nn.functional.group_norm(x, num_groups, weight, bias, eps)
    if act_id == 1:
        y = torch.nn.functional.leaky_relu(y, slope)
    elif act_id == 2:
        y = torch.nn.functional.prelu(y, slope_t.to(y.dtype))
    return y


class _GroupNormActMaxpool(torch.autograd.Function):
    """GroupNorm + activation + max-pool over the K axis, fused (HIP).

    Stats over the full (K, N) spatial extent; output is the pooled
    (B, C, N) tensor -- the (B, C, K, N) activation never hits HBM.
    """

    @staticmethod
    def forward(ctx, x, num_groups, weight, bias, eps, act, slope, slope_t):
        w = weight.float().contiguous()
        b = bias.float().contiguous()
        st_ = slope_t.float().reshape(1).contiguous() if slope_t is not None else None
        y, am, mean, rstd = _EXT.group_norm_act_maxpool_fwd(x, num_groups, w, b, eps, act, slope, st_)
        ctx.save_for_backward(x, am, mean, rstd, w, b, st_)
        ctx.conf = (num_groups, act, slope, weight.dtype)
        ctx.params = (weight, bias, slope_t)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, am, mean, rstd, w, b, st_ = ctx.saved_tensors
        num_groups, act, slope, wdtype = ctx.conf
        tgt = _gn_defer_targets(*ctx.params, act)
        if tgt is not None:
            (dx,) = _EXT.group_norm_act_maxpool_bwd(
                dy.contiguous(), x, am, mean, rstd, num_groups, w, b, act,
                slope, st_, tgt[0], tgt[1], tgt[2],
            )
            return dx, None, None, None, None, None, None, None
        dx, dw, db, dsl = _EXT.group_norm_act_maxpool_bwd(
            dy.contiguous(), x, am, mean, rstd, num_groups, w, b, act, slope,
            st_, None, None, None,
        )
        dslope = dsl.to(wdtype) if act == 2 else None
        return dx, None, dw.to(wdtype), db.to(wdtype), None, None, None, dslope


def group_norm_act_maxpool(
    x: Tensor,
    num_groups: int,
    weight: Tensor,
    bias: Tensor,
    eps: float = 1e-5,
    act: str = "lrelu",
    slope: float = 0.1,
    slope_t: Optional[Tensor] = None,
) -> Tensor:
    """(B, C, K, N) -> (B, C, N): GroupNorm -> activation -> max over K."""
    act_id = {"none": 0, "lrelu": 1, "prelu": 2}[act]
    if _use_hip(x):
        return _GroupNormActMaxpool.apply(
            x.contiguous(), num_groups, weight, bias, eps, act_id, slope, slope_t
        )
    y = torch.nn.functional.group_norm(x, num_groups, weight, bias, eps)
    if act_id == 1:
        y = torch.nn.functional.leaky_relu(y, slope)
    elif act_id == 2:
        y = torch.nn.functional.prelu(y, slope_t.to(y.dtype))
    return y.max(dim=2)[0]


class _EdgeGNMP(torch.autograd.Function):
    """SetConv stage 1 on linearly-restructured operands (see
    csrc/edge_gnmp.hip): input wg (B, N, M) point-major = fc1-W @ [feats;
    xyz] per point; output = pooled max_j act(GN(wg[nbr] - wg[center]))
    (B, N, M).  The (B, M, K, N) edge tensors of the reference formulation
    (gconv.py:64-75) never exist, forward or backward; the backward is the
    deterministic CSR walk."""

    @staticmethod
    def forward(ctx, wg_t, idx, offsets, order_n, order_j, num_groups, weight, bias, eps, act, slope, slope_t,
                channel_major_out=False):
        w = weight.float().contiguous()
        b = bias.float().contiguous()
        st_ = slope_t.float().reshape(1).contiguous() if slope_t is not None else None
        y, am, vsel, vsum, mean, rstd = _EXT.edge_gnmp_fwd(
            wg_t, idx, num_groups, w, b, eps, act, slope, st_, channel_major_out,
            egnmp_classic()[0])
        ctx.save_for_backward(wg_t, idx, am, vsel, vsum, offsets, order_n, order_j, mean, rstd, w, b, st_)
        ctx.conf = (num_groups, act, slope, weight.dtype)
        ctx.channel_major_out = channel_major_out
        ctx.params = (weight, bias, slope_t)
        return y

    @staticmethod
    def backward(ctx, dy):
        (wg_t, idx, am, vsel, vsum, offsets, order_n, order_j, mean, rstd,
         w, b, st_) = ctx.saved_tensors
        num_groups, act, slope, wdtype = ctx.conf
        dy = dy.contiguous()
        if ctx.channel_major_out:
            # the backward kernels read dy point-major: one transpose, as
            # the autograd of the caller's output transpose did before
            dy = _EXT.batched_transpose(dy)
        tgt = _gn_defer_targets(*ctx.params, act)
        classic = egnmp_classic()[1]
        if tgt is not None:
            (dwg,) = _EXT.edge_gnmp_bwd(
                dy.contiguous(), wg_t, idx, am, vsel, vsum, offsets,
                order_n, order_j,
                mean, rstd, num_groups, w, b, act, slope, st_,
                tgt[0], tgt[1], tgt[2], classic,
            )
            return (dwg, None, None, None, None, None, None, None, None,
                    None, None, None, None)
        dwg, dw, db, dsl = _EXT.edge_gnmp_bwd(
            dy.contiguous(), wg_t, idx, am, vsel, vsum, offsets, order_n,
            order_j,
            mean, rstd, num_groups, w, b, act, slope, st_, None, None, None,
            classic,
        )
        dslope = dsl.to(wdtype) if act == 2 else None
        return (dwg, None, None, None, None, None, dw.to(wdtype),
                db.to(wdtype), None, None, None, dslope, None)


def edge_gnmp(
    wg_t: Tensor,
    idx: Tensor,
    csr,
    num_groups: int,
    weight: Tensor,
    bias: Tensor,
    eps: float = 1e-5,
    act: str = "lrelu",
    slope: float = 0.1,
    slope_t: Optional[Tensor] = None,
    channel_major_out: bool = False,
) -> Tensor:
    """(B, N, M) wg + (B, N, K) neighbours -> (B, N, M) pooled SetConv
    stage 1 (gather-diff -> GN -> act -> max over K), GPU only.
    ``channel_major_out``: the pooled result is written (B, M, N)."""
    if not _use_hip(wg_t):
        raise RuntimeError("edge_gnmp is a GPU-only fused op")
    act_id = {"none": 0, "lrelu": 1, "prelu": 2}[act]
    _order, offsets, order_n, order_j = csr
    return _EdgeGNMP.apply(
        wg_t.contiguous(), idx, offsets, order_n, order_j, num_groups,
        weight, bias, eps, act_id, slope, slope_t, channel_major_out,
    )


class _KnnGNMP(torch.autograd.Function):
    """Fused kNN-corr branch head: conv(4->C) + GN + PReLU + max over K
    (csrc/knn_gnmp.hip) -- the (B, C, K, N) conv activation never exists.
    fp32 compute (raw is fp32; the contraction is 4-wide), output in the
    autocast dtype."""

    @staticmethod
    def forward(ctx, raw, weight, cbias, num_groups, gamma, beta, eps, slope_t,
                channel_major_out=False):
        w = weight.view(weight.shape[0], 4).float().contiguous()
        cb = cbias.float().contiguous()
        ga = gamma.float().contiguous()
        be = beta.float().contiguous()
        st = slope_t.float().reshape(1).contiguous()
        out_bf16 = raw.is_cuda and torch.is_autocast_enabled() and (
            torch.get_autocast_dtype("cuda") == torch.bfloat16)
        y, am, vsel, mean, rstd = _EXT.knn_gnmp_fwd(
            raw, w, cb, num_groups, ga, be, eps, st, out_bf16,
            channel_major_out)
        ctx.save_for_backward(raw, w, cb, am, vsel, mean, rstd, ga, be, st)
        ctx.conf = (num_groups, weight.shape, weight.dtype, eps)
        ctx.channel_major_out = channel_major_out
        ctx.param_refs = (weight, cbias, gamma, beta, slope_t)
        return y

    @staticmethod
    def backward(ctx, dy):
        from pvraft_amd.model import pointwise

        raw, w, cb, am, vsel, mean, rstd, ga, be, st = ctx.saved_tensors
        num_groups, wshape, wdtype, eps = ctx.conf
        # the kernels read dy in the layout it arrives in: (B, C, N) for
        # the channel-major output, (B, N, C) otherwise
        dy = dy.contiguous()
        cm = ctx.channel_major_out
        params = ctx.param_refs
        if pointwise._DEFER.on and all(
            p.is_leaf and p.requires_grad for p in params
        ):
            # accumulate in-place on the CURRENT stream and return no
            # grads: an AccumulateGrad node pinned to the warmup side
            # stream mis-orders against the producing kernels under
            # hipGraph capture (replays read the grad workspaces before
            # they are written -- measured 1e13-garbage conv grads,
            # scripts/graph_step_gradcheck.py); every other weight grad
            # already rides the deferred/drain path for the same reason.
            bufs = [pointwise._grad_buffer(p) for p in params]
            if all(t.dtype == torch.float32 and t.is_contiguous()
                   for t in bufs):
                # the coefficient kernel adds into the buffers itself
                (draw,) = _EXT.knn_gnmp_bwd(
                    dy, raw, w, cb, am, vsel, mean, rstd, num_groups, ga,
                    be, st, eps, cm, *[t.view(-1) for t in bufs])
            else:
                draw, *grads = _EXT.knn_gnmp_bwd(
                    dy, raw, w, cb, am, vsel, mean, rstd, num_groups, ga,
                    be, st, eps, cm)
                for t, g in zip(bufs, grads):
                    t.view(-1).add_(g.view(-1))
            return (draw, None, None, None, None, None, None, None, None)
        draw, dW, dcb, dgamma, dbeta, dslope = _EXT.knn_gnmp_bwd(
            dy, raw, w, cb, am, vsel, mean, rstd, num_groups, ga, be, st, eps,
            cm)
        return (draw, dW.view(wshape).to(wdtype), dcb, None, dgamma, dbeta,
                None, dslope.reshape(1), None)


def knn_gnmp(raw: Tensor, weight: Tensor, cbias: Tensor, num_groups: int,
             gamma: Tensor, beta: Tensor, eps: float, slope_t: Tensor,
             channel_major_out: Optional[bool] = None) -> Tensor:
    """raw (B, 4, K, N) fp32 -> (B, C, N): conv -> GN -> PReLU -> max over
    K in one fused pipeline, GPU only."""
    if not _use_hip(raw):
        raise RuntimeError("knn_gnmp is a GPU-only fused op")
    if channel_major_out is None:
        channel_major_out = channel_major_layout()
    if channel_major_out:
        # the pick kernel writes (B, C, N) itself
        return _KnnGNMP.apply(raw.contiguous(), weight, cbias, num_groups,
                              gamma, beta, eps, slope_t, True)
    y = _KnnGNMP.apply(raw.contiguous(), weight, cbias, num_groups, gamma,
                       beta, eps, slope_t)
    return transpose_last2(y)  # (B, N, C) -> (B, C, N), narrow-R fast path


# ---------------------------------------------------------------------------
# public functional API (model code calls these)
# ---------------------------------------------------------------------------


_ARANGE_CACHE: dict = {}


def morton_order(xyz: Tensor, need_inv: bool = True):
    """(B, N, 3) -> (perm, inv) int64 (B, N): point relabeling along a
    30-bit Morton curve.  Gathers all over the model (SetConv neighbour
    rows, correlation lookups) touch random point ids on unordered
    clouds; Z-order relabeling makes kNN neighbourhoods id-local so those
    kernels L2/L1-hit.  ``xyz.gather(1, perm...)`` sorts; ``gather(1,
    inv...)`` restores the original order.  ``need_inv=False`` skips the
    inverse (pc2 never needs one)."""
    if not _use_hip(xyz):
        raise RuntimeError("morton_order is a GPU-only op")
    mn, mx = torch.aminmax(xyz, dim=1)
    mn = mn.contiguous()
    inv_ext = (1023.0 / (mx - mn).clamp_min(1e-9)).contiguous()
    keys = _EXT.morton_keys(xyz.contiguous(), mn, inv_ext)
    perm = keys.argsort(dim=1)
    inv = None
    if need_inv:
        B, N = perm.shape
        ck = (B, N, xyz.device.index)
        ar = _ARANGE_CACHE.get(ck)
        if ar is None:
            ar = torch.arange(N, device=xyz.device).expand(B, N).contiguous()
            _ARANGE_CACHE[ck] = ar
        inv = torch.empty_like(perm)
        inv.scatter_(1, perm, ar)  # one scatter instead of a second sort
    return perm, inv


def knn_graph_pair(xyz: Tensor, k: int) -> Tuple[Tensor, Optional[Tensor]]:
    """(B,N,3) -> ((B,N,k) int64 neighbour indices, the kernel's own int32
    result or None on the reference backend)."""
    xyz = xyz.contiguous().float()
    if _use_hip(xyz):
        idx32 = _EXT.knn_graph(xyz, k)
        return idx32.long(), idx32
    return reference.knn_idx(xyz, k), None


def knn_graph(xyz: Tensor, k: int) -> Tensor:
    """(B,N,3) -> (B,N,k) int64 neighbour indices (self included)."""
    return knn_graph_pair(xyz, k)[0]


def knn_csr(idx32: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(B,N,k) int32 -> inverse adjacency (order, offsets, order_n, order_j),
    edge ids j*N+n sorted by (target, id) (csrc/knn_csr.hip)."""
    if _load_ext() is None:
        raise RuntimeError(f"pvraft_amd._C is not built: {_EXT_ERR}")
    return tuple(_EXT.knn_csr(idx32.contiguous()))


class _KnnInterpolate(torch.autograd.Function):
    """Fused cross-set kNN + inverse-distance blend (csrc/knn_interp.hip).
    Neighbours and weights are constants to autograd; the backward is a
    scatter of w * dout into the selected support rows."""

    @staticmethod
    def forward(ctx, support_xyz, values, query_xyz, k, eps):
        out, idx32, w = _EXT.knn_interp_fwd(support_xyz, values, query_xyz, k, eps)
        idx = idx32.long()
        ctx.save_for_backward(idx, w)
        ctx.n_support = values.shape[1]
        ctx.mark_non_differentiable(idx, w)
        return out, idx, w

    @staticmethod
    def backward(ctx, dout, _didx, _dw):
        idx, w = ctx.saved_tensors
        B, M, ke = idx.shape
        C = dout.shape[2]
        # empty slots (-1, weight 0: non-finite coordinates) add zeros to row 0
        rows = (idx.clamp_min(0) + torch.arange(B, device=idx.device).view(B, 1, 1) * ctx.n_support).reshape(-1)
        contrib = (w.unsqueeze(-1) * dout.unsqueeze(2)).reshape(B * M * ke, C)
        dvalues = torch.zeros(B * ctx.n_support, C, dtype=dout.dtype, device=dout.device)
        dvalues.index_add_(0, rows, contrib)
        return None, dvalues.view(B, ctx.n_support, C), None, None, None


def knn_interpolate(
    support_xyz: Tensor, values: Tensor, query_xyz: Tensor, k: int = 3, eps: float = 1e-8
) -> Tuple[Tensor, Tensor, Tensor]:
    """Inverse-distance interpolation of ``values`` from a support cloud
    onto query points: (B,N,3),(B,N,C),(B,M,3) -> out (B,M,C), idx
    (B,M,k_eff) int64, w (B,M,k_eff), k_eff = min(k, N), 1 <= k <= 16.

    w_i = 1/(d2_i + eps) normalised over the k_eff nearest support points
    (idx ascending in distance), out = sum_i w_i * values[idx_i].  The
    (M, N) distance matrix is never materialised.  bf16/fp16 or
    non-contiguous inputs are upcast / made contiguous here.

    Autograd flows to ``values`` only; coordinates get no gradient.  On
    GPU the backward is an ``index_add_`` over the saved (idx, w), whose
    atomic accumulation order is NON-DETERMINISTIC (last-bit run-to-run
    differences in ``values.grad``).
    """
    if not 1 <= int(k) <= 16:
        raise ValueError(f"knn_interpolate requires 1 <= k <= 16, got {k}")
    if _use_hip(support_xyz):
        return _KnnInterpolate.apply(
            support_xyz.detach().float().contiguous(),
            values.float().contiguous(),
            query_xyz.detach().float().contiguous(),
            int(k),
            float(eps),
        )
    if not (support_xyz.dtype == values.dtype == query_xyz.dtype == torch.float64):
        support_xyz, values, query_xyz = support_xyz.float(), values.float(), query_xyz.float()
    return reference.knn_interpolate(
        support_xyz.detach().contiguous(), values.contiguous(), query_xyz.detach().contiguous(), int(k), float(eps)
    )


def gather_edge_concat(feats: Tensor, idx: Tensor, xyz: Tensor, csr=None) -> Tensor:
    """(B,N,C),(B,N,K),(B,N,3) -> (B,C+3,K,N) edge-conv input.

    ``csr`` = (order, offsets) from Graph.csr() selects the deterministic
    atomic-free backward.
    """
    if not feats.is_contiguous():
        if (
            feats.is_cuda
            and feats.dim() == 3
            and feats.stride(1) == 1
            and feats.stride(2) == feats.shape[1]
            and feats.dtype in (torch.float32, torch.bfloat16)
            and os.environ.get("PVRAFT_REF_OPS", "0") != "1"
            and _load_ext() is not None
        ):
            # (B, N, C) transpose-view of contiguous (B, C, N): transpose
            # through the LDS-tiled kernel instead of ATen's strided copy
            feats = _BatchedTranspose.apply(feats.transpose(1, 2))
        else:
            feats = feats.contiguous()
    if _use_hip(feats):
        if feats.dtype not in (torch.float32, torch.bfloat16):
            feats = feats.float()
        order, offsets = (csr[0], csr[1]) if csr is not None else (None, None)
        return _GatherEdgeConcat.apply(
            feats, idx.to(torch.int32).contiguous(), xyz.contiguous().float(),
            order, offsets,
        )
    return reference.gather_edge_concat(feats, idx, xyz)


class _CorrTruncate(torch.autograd.Function):
    """Truncated correlation with gather-based backward.

    Forward (no_grad): chunked rocBLAS GEMM + per-row top-K -- the N x M
    matrix exists only one row-chunk at a time and is NOT saved for
    backward (plain autograd through matmul+topk would retain all of it,
    reference corr.py:34-37 does exactly that).  Backward uses the saved
    top-K indices:
        d f1[:, n]  = scale * sum_k g[n, k] * f2[:, idx[n, k]]
        d f2[:, m] += scale * sum_{n,k: idx=m} g[n, k] * f1[:, n]
    which is O(N*K*C) instead of O(N*M*C).  (As executed: the sparse
    gradient is expanded to a dense (B, N, M) matrix, one pass of
    corr_grad_expand, and both sums run as dense MFMA GEMMs over it.)
    """

    CHUNK = 2048
    # corr_grad_expand keeps one row of the dense gradient in LDS
    EXPAND_ROW_BYTES = 64 * 1024

    @staticmethod
    def forward(ctx, fmap1: Tensor, fmap2: Tensor, xyz2: Tensor, truncate_k: int,
                index_dtype: torch.dtype = torch.int64):
        classic = corr_bwd_classic()
        # accumulation stays fp32 everywhere (selection quality follows the
        # reference, corr.py:95-99): the fused MFMA kernel accumulates fp32
        # from bf16 operands; the fp32 fallback disables autocast so the
        # bmm is a true fp32 GEMM
        with torch.no_grad(), torch.autocast("cuda", enabled=False):
            M = fmap2.shape[2]
            if (
                fmap1.is_cuda
                and fmap1.dtype == torch.bfloat16
                and fmap2.dtype == torch.bfloat16
                and fmap1.shape[1] % 32 == 0
                and fmap1.shape[1] <= 256
                and truncate_k <= 1024
                and _load_ext() is not None
            ):
                # fused MFMA GEMM + streaming top-K: the (N, M) matrix is
                # never materialised (csrc/corr_topk.hip)
                K = min(truncate_k, M)
                f1t = _EXT.batched_transpose(fmap1.contiguous())
                f2t = _EXT.batched_transpose(fmap2.contiguous())
                corr, idx = _EXT.corr_topk(f1t, f2t, K)
                B, _, N = fmap1.shape
                if classic or xyz2.dtype != torch.float32:
                    idx = idx.long()
                    txyz = xyz2.gather(
                        1, idx.reshape(B, N * K).unsqueeze(-1).expand(B, N * K, 3)
                    ).view(B, N, K, 3)
                else:
                    # int32 indices straight into the row gather and, saved,
                    # into the backward (csrc/corr_bwd.hip)
                    txyz = _EXT.corr_gather_xyz(idx, xyz2.contiguous())
            elif fmap1.is_cuda and M <= 8192 and _load_ext() is not None:
                corr, idx, txyz = _CorrTruncate._gpu_forward(
                    fmap1.float(), fmap2.float(), xyz2, truncate_k
                )
            else:
                corr, idx, txyz = reference.corr_truncate(
                    fmap1.float(), fmap2.float(), xyz2, truncate_k,
                    chunk=_CorrTruncate.CHUNK,
                )
        ctx.save_for_backward(fmap1, fmap2, idx)
        # backward GEMMs run bf16 when the surrounding step is bf16 autocast
        # (standard amp gradient precision; fp32 master weights untouched)
        ctx.bf16_bwd = fmap1.is_cuda and (
            torch.is_autocast_enabled() or fmap1.dtype == torch.bfloat16
        )
        # int64 unless the caller takes the kernels' int32 as it is; an
        # index that is already int64 is never narrowed
        idx_out = idx.long() if index_dtype == torch.int64 else idx
        return corr, idx_out, txyz

    @staticmethod
    def _gpu_forward(fmap1: Tensor, fmap2: Tensor, xyz2: Tensor, truncate_k: int):
        """Chunked rocBLAS GEMM + histogram-select top-K kernel (the
        torch.topk path sorts and was the next profiler hotspot; the top-K
        SET is order-free for every consumer)."""
        B, C, N = fmap1.shape
        M = fmap2.shape[2]
        K = min(truncate_k, M)
        scale = 1.0 / math.sqrt(C)
        f1t = fmap1.transpose(1, 2).contiguous()
        chunk = _CorrTruncate.CHUNK
        vals, idxs = [], []
        for s in range(0, N, chunk):
            c = torch.bmm(f1t[:, s : s + chunk], fmap2)
            c = c * scale
            n_rows = c.shape[1]
            v, i = _EXT.topk_rows(c.reshape(B * n_rows, M), K)
            vals.append(v.view(B, n_rows, K))
            idxs.append(i.view(B, n_rows, K))
        corr = torch.cat(vals, dim=1)
        idx = torch.cat(idxs, dim=1)
        if corr_bwd_classic() or xyz2.dtype != torch.float32:
            idx = idx.long()
            txyz = xyz2.gather(1, idx.reshape(B, N * K).unsqueeze(-1).expand(B, N * K, 3)).view(B, N, K, 3)
        else:
            txyz = _EXT.corr_gather_xyz(idx, xyz2.contiguous())
        return corr, idx, txyz

    @staticmethod
    def backward(ctx, g_corr: Tensor, _g_idx, _g_xyz):
        fmap1, fmap2, idx = ctx.saved_tensors
        B, C, N = fmap1.shape
        M = fmap2.shape[2]
        scale = 1.0 / math.sqrt(C)
        # top-K indices are unique within each row, so the sparse gradient
        # expands to a dense (B, N, M) buffer with a CONFLICT-FREE scatter
        # (no atomics), and both fmap gradients become plain rocBLAS GEMMs.
        dt = torch.bfloat16 if ctx.bf16_bwd else g_corr.dtype
        f1 = fmap1.to(dt)
        f2 = fmap2.to(dt)
        if (
            g_corr.is_cuda
            and not corr_bwd_classic()
            and dt in (torch.bfloat16, torch.float32)
            and M * dt.itemsize <= _CorrTruncate.EXPAND_ROW_BYTES
            and _load_ext() is not None
        ):
            # one pass writes every element of the dense matrix once
            # (csrc/corr_bwd.hip); the g1 GEMM reads the same buffer as a
            # transposed operand instead of a transposed copy (in the step
            # 100 us against 82 + 167 us at the flagship shape; multiplying
            # by the point-major fmap2 and transposing the result gave the
            # same step time, see profiles/README.md)
            gfull = _EXT.corr_grad_expand(
                g_corr.float().contiguous(), idx.to(torch.int32), scale, M,
                dt == torch.bfloat16,
            )
            g1 = torch.bmm(f2, gfull.transpose(1, 2)).float()  # (B,C,N)
            g2 = torch.bmm(f1, gfull).float()  # (B,C,M)
            return g1, g2, None, None, None
        gfull = torch.zeros(B, N, M, dtype=dt, device=g_corr.device)
        gfull.scatter_(2, idx.long(), (g_corr * scale).to(dt))
        if gfull.is_cuda and _load_ext() is not None:
            gfull_t = _EXT.batched_transpose(gfull)
        else:
            gfull_t = gfull.transpose(1, 2).contiguous()
        g1 = torch.bmm(f2, gfull_t).float()  # (B,C,N)
        g2 = torch.bmm(f1, gfull).float()  # (B,C,M)
        return g1, g2, None, None, None


def corr_bwd_classic() -> bool:
    """PVRAFT_CORR_BWD=classic (read per call) restores the composed
    truncated-correlation path: int64 indices + ATen gather in the forward,
    zeros + scatter_ + transposed copy in the backward."""
    return os.environ.get("PVRAFT_CORR_BWD", "") == "classic"


def corr_truncate(fmap1: Tensor, fmap2: Tensor, xyz2: Tensor, truncate_k: int,
                  index_dtype: torch.dtype = torch.int64):
    """(B,C,N),(B,C,M),(B,M,3) -> corr (B,N,K), idx (B,N,K), xyz (B,N,K,3).

    bf16 inputs (autocast) take the fused MFMA GEMM + streaming top-K
    kernel; fp32 falls back to the chunked rocBLAS bmm + topk_rows path.
    Values are always fp32 accumulate.  ``index_dtype=torch.int32`` hands
    out the kernels' own indices where the path has them, for callers that
    do not need ``idx`` as int64 (the conversion is a 64 MB write at the
    flagship shape); the reference paths return their int64 index as it
    is.
    """
    if fmap1.is_cuda and os.environ.get("PVRAFT_REF_OPS", "0") != "1":
        return _CorrTruncate.apply(fmap1, fmap2, xyz2, truncate_k, index_dtype)
    return reference.corr_truncate(fmap1.float(), fmap2.float(), xyz2, truncate_k)


def voxel_corr(
    corr: Tensor,
    xyz: Tensor,
    coords: Tensor,
    base_scale: float,
    num_levels: int,
    resolution: int = 3,
) -> Tensor:
    """(B,N,K),(B,N,K,3),(B,N,3) -> (B, num_levels*resolution^3, N)."""
    if _use_hip(corr):
        return _VoxelCorr.apply(
            corr.contiguous().float(),
            xyz.contiguous().float(),
            coords.contiguous().float(),
            float(base_scale),
            int(num_levels),
            int(resolution),
        )
    return reference.voxel_corr(corr, xyz, coords, base_scale, num_levels, resolution)


class _PVCorrFused(torch.autograd.Function):
    """Fused per-iteration lookup: voxel pyramid + kNN branch in one kernel
    pass over the truncated correlation field (see csrc/pv_corr_fused.hip)."""

    @staticmethod
    def forward(ctx, corr, xyz, coords, base_scale, num_levels, k):
        vox, knn, idx = _EXT.pv_corr_fused_fwd(corr, xyz, coords, base_scale, num_levels, k)
        ctx.save_for_backward(xyz, coords, idx)
        ctx.conf = (base_scale, num_levels, k)
        return vox, knn

    @staticmethod
    def backward(ctx, g_vox, g_knn):
        xyz, coords, idx = ctx.saved_tensors
        base_scale, num_levels, k = ctx.conf
        g = _EXT.pv_corr_fused_bwd(
            g_vox.contiguous(), g_knn.contiguous(), xyz, coords, idx, num_levels, k, base_scale
        )
        return g, None, None, None, None, None


def pv_corr_lookup(
    corr: Tensor,
    xyz: Tensor,
    coords: Tensor,
    base_scale: float,
    num_levels: int,
    k: int,
    resolution: int = 3,
):
    """(voxel (B, L*27, N), knn (B, 4, k, N)) in one fused pass on GPU."""
    if _use_hip(corr) and resolution == 3:
        return _PVCorrFused.apply(
            corr.contiguous().float(),
            xyz.contiguous().float(),
            coords.contiguous().float(),
            float(base_scale),
            int(num_levels),
            int(k),
        )
    return (
        reference.voxel_corr(corr, xyz, coords, base_scale, num_levels, resolution),
        reference.knn_corr(corr, xyz, coords, k),
    )


def knn_corr(corr: Tensor, xyz: Tensor, coords: Tensor, k: int) -> Tensor:
    """(B,N,K),(B,N,K,3),(B,N,3) -> (B,4,N,k)."""
    if _use_hip(corr):
        return _KnnCorr.apply(
            corr.contiguous().float(),
            xyz.contiguous().float(),
            coords.contiguous().float(),
            int(k),
        )
    return reference.knn_corr(corr, xyz, coords, k)


class _GruZR(torch.autograd.Function):
    """Fused GRU z/r gates (csrc/gru_gates.hip): one kernel for the
    sigmoid over the stacked z|r preactivations plus r*h (reference
    model/update.py:34-37), one kernel for the full backward."""

    @staticmethod
    def forward(ctx, pre: Tensor, h: Tensor):
        z, r, rh = _EXT.gru_zr_fwd(pre, h)
        ctx.save_for_backward(z, r, h)
        return z, rh

    @staticmethod
    def backward(ctx, dz: Tensor, drh: Tensor):
        z, r, h = ctx.saved_tensors
        if dz is None:
            dz = torch.zeros_like(z)
        if drh is None:
            drh = torch.zeros_like(z)
        dpre, dh = _EXT.gru_zr_bwd(dz.contiguous(), drh.contiguous(), z, r, h)
        return dpre, dh


class _GruQ(torch.autograd.Function):
    """Fused GRU candidate gate + blend: h' = (1-z) h + z tanh(pre_q)
    (reference model/update.py:38-40)."""

    @staticmethod
    def forward(ctx, pre: Tensor, z: Tensor, h: Tensor) -> Tensor:
        q, hnew = _EXT.gru_q_fwd(pre, z, h)
        ctx.save_for_backward(q, z, h)
        return hnew

    @staticmethod
    def backward(ctx, dhnew: Tensor):
        q, z, h = ctx.saved_tensors
        dpre, dz, dh = _EXT.gru_q_bwd(dhnew.contiguous(), q, z, h)
        return dpre, dz, dh


def gru_zr(pre_zr: Tensor, h: Tensor):
    """pre_zr (B,2H,N) stacked z|r preactivations, h (B,H,N) -> (z, r*h)."""
    if _use_hip(pre_zr) and os.environ.get("PVRAFT_NO_GRU_FUSION", "0") != "1":
        return _GruZR.apply(pre_zr.contiguous(), h.to(pre_zr.dtype).contiguous())
    hd = h.shape[1]
    zr = torch.sigmoid(pre_zr)
    return zr[:, :hd], zr[:, hd:] * h


def gru_q(pre_q: Tensor, z: Tensor, h: Tensor) -> Tensor:
    """h' = (1-z)*h + z*tanh(pre_q), all (B,H,N)."""
    if _use_hip(pre_q) and os.environ.get("PVRAFT_NO_GRU_FUSION", "0") != "1":
        return _GruQ.apply(
            pre_q.contiguous(), z.contiguous(), h.to(pre_q.dtype).contiguous()
        )
    return (1 - z) * h + z * torch.tanh(pre_q)


# ---------------------------------------------------------------------------
# self-supervised loss terms (csrc/chamfer.hip, csrc/flow_smooth.hip)
# ---------------------------------------------------------------------------


class _ChamferLoss(torch.autograd.Function):
    """Fused Chamfer distance of T warped clouds (csrc/chamfer.hip): one
    launch for all flows and both directions; the backward is a
    deterministic gather over the saved assignments."""

    @staticmethod
    def forward(ctx, pc1, flows, pc2):
        cham, _d1, i1, _d2, i2 = _EXT.chamfer_fwd(pc1, flows, pc2)
        ctx.save_for_backward(pc1, flows, pc2, i1, i2)
        return cham

    @staticmethod
    def backward(ctx, g):
        pc1, flows, pc2, i1, i2 = ctx.saved_tensors
        return None, _EXT.chamfer_bwd(pc1, flows, pc2, i1, i2, g.float().contiguous()), None


class _FlowSmoothness(torch.autograd.Function):
    """Fused smoothness of T flows over one kNN graph
    (csrc/flow_smooth.hip); the backward walks the graph's inverse
    adjacency, so it needs no atomics."""

    @staticmethod
    def forward(ctx, flows, idx32, offsets, order_n):
        ctx.save_for_backward(flows, idx32, offsets, order_n)
        return _EXT.flow_smooth_fwd(flows, idx32)

    @staticmethod
    def backward(ctx, g):
        flows, idx32, offsets, order_n = ctx.saved_tensors
        return _EXT.flow_smooth_bwd(flows, idx32, offsets, order_n, g.float().contiguous()), None, None, None


def _fp32_unless_all_fp64(*tensors: Tensor):
    if all(t.dtype == torch.float64 for t in tensors):
        return tensors
    return tuple(t.float() for t in tensors)


def chamfer_nn(query: Tensor, support: Tensor) -> Tuple[Tensor, Tensor]:
    """Nearest support point of every query: (B,Q,3), (B,S,3) -> d2 (B,Q),
    idx (B,Q) int64.  Squared distances from coordinate differences; ties go
    to the lowest index; a NaN or +INF distance never wins, and a query with
    no finite candidate gets idx -1 and d2 = +INF.  Not differentiable.
    The (Q, S) distance matrix is never materialised.  bf16/fp16 or
    non-contiguous inputs are upcast / made contiguous here.
    """
    if _use_hip(query):
        d2, idx32 = _EXT.chamfer_nn_fwd(
            query.detach().float().contiguous(), support.detach().float().contiguous()
        )
        return d2, idx32.long()
    query, support = _fp32_unless_all_fp64(query.detach(), support.detach())
    return reference.chamfer_nn(query.contiguous(), support.contiguous())


def chamfer_loss(pc1: Tensor, flows, pc2: Tensor) -> Tensor:
    """Chamfer distance between every warped cloud ``pc1 + f_t`` and
    ``pc2``: pc1 (B,N,3), flows = (T,B,N,3), a list of T (B,N,3) tensors or
    one (B,N,3) tensor, pc2 (B,M,3) -> (T,), 1 <= T <= 32,

      chamfer_t = mean_{b,i} min_j |w_t[b,i] - pc2[b,j]|^2
                + mean_{b,j} min_i |pc2[b,j] - w_t[b,i]|^2

    with the nearest-neighbour rules of ``chamfer_nn``.  Autograd flows to
    the flows only; coordinates get no gradient.  The GPU backward is
    deterministic (no atomics).
    """
    flows = reference.stack_flows(flows)
    if not 1 <= flows.shape[0] <= 32:
        raise ValueError(f"chamfer_loss supports 1..32 flows, got {flows.shape[0]}")
    if _use_hip(pc1):
        return _ChamferLoss.apply(
            pc1.detach().float().contiguous(), flows.float().contiguous(), pc2.detach().float().contiguous()
        )
    pc1, flows, pc2 = _fp32_unless_all_fp64(pc1.detach(), flows, pc2.detach())
    return reference.chamfer_loss(pc1.contiguous(), flows.contiguous(), pc2.contiguous())


def flow_smoothness(flows, graph) -> Tensor:
    """Mean squared flow difference along the edges of ``graph`` (a
    ``model.graph.Graph`` over pc1, self edges included): flows as in
    ``chamfer_loss`` -> (T,),

      smooth_t = mean_{b,i,j in idx[b,i]} |f_t[b,j] - f_t[b,i]|^2

    Autograd flows to the flows only; the GPU backward is deterministic.
    """
    flows = reference.stack_flows(flows)
    if not 1 <= flows.shape[0] <= 32:
        raise ValueError(f"flow_smoothness supports 1..32 flows, got {flows.shape[0]}")
    if _use_hip(flows):
        _, offsets, order_n, _ = graph.csr()
        return _FlowSmoothness.apply(flows.float().contiguous(), graph.idx32, offsets, order_n)
    if flows.dtype != torch.float64:
        flows = flows.float()
    return reference.flow_smoothness(flows.contiguous(), graph.idx)


# ---------------------------------------------------------------------------
# ego-motion from scene flow (csrc/rigid_fit.hip)
# ---------------------------------------------------------------------------


class EgoMotion(NamedTuple):
    """Result of ``ego_motion``: R (B,3,3), t (B,3), residual (B,N), static
    (B,N) bool, rigid_flow (B,N,3), ok (B,) bool."""

    R: Tensor
    t: Tensor
    residual: Tensor
    static: Tensor
    rigid_flow: Tensor
    ok: Tensor


def rigid_fit(
    src: Tensor, dst: Tensor, weights: Optional[Tensor] = None, thresh: float = 0.05, iters: int = 0
) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Robust rigid transform between two corresponding clouds: src (B,N,3),
    dst (B,N,3), optional prior weights (B,N) -> R (B,3,3), t (B,3),
    residual (B,N), ok (B,) bool, 0 <= iters <= 64, thresh > 0,

      w0_i = weights_i (1 without weights)
      for k = 0 .. iters:
          (R, t) = argmin sum_i w_i |R src_i + t - dst_i|^2,  det R = +1
          r_i    = |R src_i + t - dst_i|
          if k < iters:  w_i = w0_i / (1 + (r_i / thresh)^2)    (Cauchy)

    so ``iters=0`` is the plain weighted Kabsch fit.  ``residual`` belongs
    to the last fit.  A point with a non-finite coordinate is skipped and
    reports residual +INF; a point with a non-finite weight or a weight <= 0
    is skipped but still gets its residual.  ``ok`` is False when fewer than
    3 points carry positive weight or a sum is non-finite: then R = I and t
    is the w0-weighted mean of dst - src (0 when no point is usable); a
    cloud of fewer than 3 points is not an error.  Planar clouds get the
    proper rotation (never a reflection); for collinear clouds R is one of
    the minimisers.

    GPU: one fused launch for the whole loop (one workgroup per batch
    element, no host synchronisation), bit-reproducible run to run.
    Not differentiable: the outputs are detached.  bf16/fp16 or
    non-contiguous inputs are upcast / made contiguous here.
    """
    if not 0 <= int(iters) <= 64:
        raise ValueError(f"rigid_fit requires 0 <= iters <= 64, got {iters}")
    if not float(thresh) > 0:
        raise ValueError(f"rigid_fit requires thresh > 0, got {thresh}")
    if src.dim() != 3 or src.shape[-1] != 3 or dst.shape != src.shape:
        raise ValueError(f"rigid_fit needs src, dst (B,N,3), got {tuple(src.shape)}, {tuple(dst.shape)}")
    if weights is not None and weights.shape != src.shape[:2]:
        raise ValueError(f"rigid_fit needs weights (B,N), got {tuple(weights.shape)}")
    if _use_hip(src):
        w = None if weights is None else weights.detach().float().contiguous()
        R, t, res, ok = _EXT.rigid_fit(
            src.detach().float().contiguous(), dst.detach().float().contiguous(), w, float(thresh), int(iters)
        )
        return R, t, res, ok
    if weights is None:
        src, dst = _fp32_unless_all_fp64(src.detach(), dst.detach())
    else:
        src, dst, weights = _fp32_unless_all_fp64(src.detach(), dst.detach(), weights.detach())
    return reference.rigid_fit(src.contiguous(), dst.contiguous(), weights, float(thresh), int(iters))


def ego_motion(
    pc1: Tensor, flow: Tensor, thresh: float = 0.05, iters: int = 10, weights: Optional[Tensor] = None
) -> EgoMotion:
    """Ego-motion explained by a flow field: pc1 (B,N,3), flow (B,N,3) ->
    ``EgoMotion(R, t, residual, static, rigid_flow, ok)``.

    (R, t, residual, ok) = ``rigid_fit(pc1, pc1 + flow, weights, thresh,
    iters)``: the rigid motion of the static part of the scene, robust to
    independently moving points.  ``static`` (B,N) bool marks the points
    whose flow agrees with it (residual < thresh; never a point with a
    non-finite coordinate) and ``rigid_flow = pc1 @ R^T + t - pc1`` (B,N,3)
    is the flow that motion alone induces at every point.  Not
    differentiable; deterministic.
    """
    pc1 = pc1.detach()
    flow = flow.detach()
    R, t, residual, ok = rigid_fit(pc1, pc1 + flow, weights, thresh, iters)
    static = residual < thresh
    p = pc1.to(R.dtype)
    rigid_flow = p @ R.transpose(1, 2) + t.unsqueeze(1) - p
    return EgoMotion(R, t, residual, static, rigid_flow, ok)


# ---------------------------------------------------------------------------
# moving objects (csrc/cluster.hip, segmented fit in csrc/rigid_fit.hip)
# ---------------------------------------------------------------------------


class ObjectMotion(NamedTuple):
    """Result of ``object_motion``: labels (B,N) int32, num_objects (B,)
    int32, count (B,M) int32 from ``cluster_points``; R (B,M,3,3), t (B,M,3),
    ok (B,M) bool per object; residual (B,N) with respect to the point's own
    object (+INF outside objects); rigid_flow (B,N,3) piecewise-rigid flow;
    ego, the ``EgoMotion`` used."""

    labels: Tensor
    num_objects: Tensor
    count: Tensor
    R: Tensor
    t: Tensor
    ok: Tensor
    residual: Tensor
    rigid_flow: Tensor
    ego: EgoMotion


def cluster_points(
    xyz: Tensor, flow: Tensor, mask: Tensor, eps: float = 0.5, flow_eps: float = 0.1,
    min_points: int = 8, max_objects: int = 32,
) -> Tuple[Tensor, Tensor, Tensor]:
    """Euclidean + flow-consistency clustering: xyz (B,N,3), flow (B,N,3),
    mask (B,N) bool -> labels (B,N) int32, count (B,max_objects) int32,
    num_objects (B,) int32; eps >= 0, flow_eps >= 0 (``float('inf')``
    disables the flow test), min_points >= 3, 1 <= max_objects <= 256.

    A point is eligible if it is masked and its six numbers are finite.  Two
    eligible points are linked iff |xyz_i - xyz_j|^2 <= eps^2 and |flow_i -
    flow_j|^2 <= flow_eps^2 (fp32 sums of squared differences against the
    fp32 products; a pair within a few ulp of a threshold may fall either
    way).  The objects are the connected components of this exact radius
    graph with at least ``min_points`` members, ordered by (size descending,
    smallest member index ascending); only the first ``max_objects`` are
    kept.  ``labels`` is the rank of the point's object or -1 (unmasked,
    non-finite, small component, beyond ``max_objects``), ``count`` the
    object sizes (0 for unused slots).  The result is canonical: the same
    integers on every backend and in every run.

    GPU: lock-free union-find over all linked pairs (csrc/cluster.hip), five
    launches, no host synchronisation, no (N,N) tensor.  Every retry loop in
    the kernels is capped; should a cap ever be hit, that batch element comes
    back with all labels -1 and ``num_objects`` = -1 instead of a wrong
    partition.  Not differentiable.  bf16/fp16 or non-contiguous inputs are
    upcast / made contiguous here.
    """
    if xyz.dim() != 3 or xyz.shape[-1] != 3 or flow.shape != xyz.shape:
        raise ValueError(f"cluster_points needs xyz, flow (B,N,3), got {tuple(xyz.shape)}, {tuple(flow.shape)}")
    if mask.shape != xyz.shape[:2]:
        raise ValueError(f"cluster_points needs mask (B,N), got {tuple(mask.shape)}")
    if not float(eps) >= 0 or not float(flow_eps) >= 0:
        raise ValueError(f"cluster_points requires eps, flow_eps >= 0, got {eps}, {flow_eps}")
    if not int(min_points) >= 3:
        raise ValueError(f"cluster_points requires min_points >= 3, got {min_points}")
    if not 1 <= int(max_objects) <= 256:
        raise ValueError(f"cluster_points requires 1 <= max_objects <= 256, got {max_objects}")
    B, N = xyz.shape[:2]
    mask = mask.detach().bool()
    if _use_hip(xyz) and B > 0 and N > 0:
        return tuple(_EXT.cluster_points(
            xyz.detach().float().contiguous(), flow.detach().float().contiguous(), mask.contiguous(),
            float(eps), float(flow_eps), int(min_points), int(max_objects),
        ))
    xyz, flow = _fp32_unless_all_fp64(xyz.detach(), flow.detach())
    return reference.cluster_points(xyz.contiguous(), flow.contiguous(), mask, float(eps), float(flow_eps),
                                    int(min_points), int(max_objects))


def segmented_rigid_fit(
    src: Tensor, dst: Tensor, labels: Tensor, num_segments: int, weights: Optional[Tensor] = None,
    thresh: float = 0.05, iters: int = 0,
) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """One robust rigid fit per labelled segment: src, dst (B,N,3), labels
    (B,N) integer in [-1, num_segments) (anything else counts as -1),
    optional prior weights (B,N) -> R (B,M,3,3), t (B,M,3), residual (B,N),
    ok (B,M) bool with M = num_segments, 1 <= M <= 65535.

    Per segment this is exactly the loop of ``rigid_fit`` over that
    segment's points.  ``residual[b,i]`` belongs to i's own segment and is
    +INF for label -1 and for a non-finite coordinate.  An empty or
    under-determined segment has ok = False, R = I and t as ``rigid_fit``
    defines it.

    GPU: one launch, one workgroup per segment, which compacts its members in
    index order once and keeps up to ``_C.SEGMENTED_FIT_CAPACITY`` of them on
    chip, so a round costs in proportion to the segment, not to N; no
    atomics, no host synchronisation, bit-reproducible.  Not differentiable.
    """
    if not 0 <= int(iters) <= 64:
        raise ValueError(f"segmented_rigid_fit requires 0 <= iters <= 64, got {iters}")
    if not float(thresh) > 0:
        raise ValueError(f"segmented_rigid_fit requires thresh > 0, got {thresh}")
    if not 1 <= int(num_segments) <= 65535:
        raise ValueError(f"segmented_rigid_fit requires 1 <= num_segments <= 65535, got {num_segments}")
    if src.dim() != 3 or src.shape[-1] != 3 or dst.shape != src.shape:
        raise ValueError(f"segmented_rigid_fit needs src, dst (B,N,3), got {tuple(src.shape)}, {tuple(dst.shape)}")
    if labels.shape != src.shape[:2] or labels.is_floating_point() or labels.dtype == torch.bool:
        raise ValueError(f"segmented_rigid_fit needs integer labels (B,N), got {labels.dtype} {tuple(labels.shape)}")
    if weights is not None and weights.shape != src.shape[:2]:
        raise ValueError(f"segmented_rigid_fit needs weights (B,N), got {tuple(weights.shape)}")
    B, N = src.shape[:2]
    if _use_hip(src) and B > 0 and N > 0:
        w = None if weights is None else weights.detach().float().contiguous()
        lab = labels.detach()
        if lab.dtype != torch.int32:
            # out-of-range values of a wider type must not wrap into range
            lab = torch.where((lab >= 0) & (lab < int(num_segments)), lab, torch.full_like(lab, -1)).int()
        return tuple(_EXT.segmented_rigid_fit(
            src.detach().float().contiguous(), dst.detach().float().contiguous(), lab.contiguous(),
            int(num_segments), w, float(thresh), int(iters),
        ))
    if weights is None:
        src, dst = _fp32_unless_all_fp64(src.detach(), dst.detach())
    else:
        src, dst, weights = _fp32_unless_all_fp64(src.detach(), dst.detach(), weights.detach())
    return reference.segmented_rigid_fit(src.contiguous(), dst.contiguous(), labels.detach(), int(num_segments),
                                         weights, float(thresh), int(iters))


def object_motion(
    pc1: Tensor, flow: Tensor, ego: Optional[EgoMotion] = None, ego_thresh: float = 0.05, ego_iters: int = 10,
    eps: float = 0.5, flow_eps: float = 0.1, min_points: int = 8, max_objects: int = 32,
    thresh: float = 0.05, iters: int = 5,
) -> ObjectMotion:
    """Moving objects of a flow field: pc1 (B,N,3), flow (B,N,3) ->
    ``ObjectMotion``.

      ego    = ego or ego_motion(pc1, flow, ego_thresh, ego_iters)
      labels, count, num_objects = cluster_points(pc1, flow, ~ego.static,
                                       eps, flow_eps, min_points, max_objects)
      R, t, residual, ok = segmented_rigid_fit(pc1, pc1 + flow, labels,
                                       max_objects, thresh=thresh, iters=iters)

    ``rigid_flow`` is, per point, the flow its object's (R, t) induces where
    the point belongs to an object with ``ok``, ``ego.rigid_flow`` where the
    point is static, and the raw flow elsewhere.  The whole call only
    launches kernels: no host synchronisation.  Not differentiable.

    The defaults (link radii, min_points, thresholds) are untuned guesses at
    metric driving scenes: nobody has tuned them on real data.
    """
    pc1 = pc1.detach()
    flow = flow.detach()
    if ego is None:
        ego = ego_motion(pc1, flow, thresh=ego_thresh, iters=ego_iters)
    labels, count, num_objects = cluster_points(pc1, flow, ~ego.static, eps, flow_eps, min_points, max_objects)
    R, t, residual, ok = segmented_rigid_fit(pc1, pc1 + flow, labels, int(max_objects), None, thresh, iters)
    p = pc1.to(R.dtype)
    B, N = labels.shape
    slot = labels.clamp_min(0).long()
    Rp = R.gather(1, slot.view(B, N, 1, 1).expand(B, N, 3, 3))
    tp = t.gather(1, slot.view(B, N, 1).expand(B, N, 3))
    obj_flow = (Rp @ p.unsqueeze(-1)).squeeze(-1) + tp - p
    in_obj = (labels >= 0) & ok.gather(1, slot)
    rigid_flow = torch.where(ego.static.unsqueeze(-1), ego.rigid_flow, flow.to(R.dtype))
    rigid_flow = torch.where(in_obj.unsqueeze(-1), obj_flow, rigid_flow)
    return ObjectMotion(labels, num_objects, count, R, t, ok, residual, rigid_flow, ego)


# ---------------------------------------------------------------------------
# ground plane (csrc/plane_fit.hip)
# ---------------------------------------------------------------------------


class PlaneFit(NamedTuple):
    """Result of ``fit_plane``: normal (B,3) unit, ``normal . up > 0``;
    offset (B,), the plane is ``normal . p + offset = 0``; height (B,N) signed
    distance above the plane (+INF for a non-finite point); ground (B,N) bool
    ``height <= thresh``; inlier (B,N) bool ``|height| <= thresh``; count (B,)
    int32 inlier count of the winning hypothesis; best (B,) int32 its index or
    -1; rounds (B,) int32 accepted refinement rounds; ok (B,) bool."""

    normal: Tensor
    offset: Tensor
    height: Tensor
    ground: Tensor
    inlier: Tensor
    count: Tensor
    best: Tensor
    rounds: Tensor
    ok: Tensor


def _plane_inputs(name, xyz, mask):
    if xyz.dim() != 3 or xyz.shape[-1] != 3:
        raise ValueError(f"{name} needs xyz (B,N,3), got {tuple(xyz.shape)}")
    if mask is not None:
        if mask.shape != xyz.shape[:2]:
            raise ValueError(f"{name} needs mask (B,N), got {tuple(mask.shape)}")
        mask = mask.detach().bool().contiguous()
    return xyz.detach().float().contiguous(), mask


def plane_hypotheses(
    xyz: Tensor, mask: Optional[Tensor] = None, thresh: float = 0.2, hypotheses: int = 256,
    up=(0.0, 1.0, 0.0), max_tilt_deg: float = 20.0, seed: int = 0,
) -> Tuple[Tensor, Tensor]:
    """Stages A and B of ``fit_plane`` alone, for tests and debugging: the
    drawn point triples idx (B,H,3) int32 and their exact inlier counts
    count (B,H) int32; an invalid hypothesis has idx = -1 and count = -1.
    The same integers on every backend."""
    thresh, thresh2, cos2, up32, H, _, seed = reference.plane_params(thresh, hypotheses, up, max_tilt_deg, 0, seed)
    xyz, mask = _plane_inputs("plane_hypotheses", xyz, mask)
    B, N = xyz.shape[:2]
    if _use_hip(xyz) and B > 0 and N > 0:
        idx, count = _EXT.plane_fit(xyz, mask, thresh, thresh2, cos2, up32[0], up32[1], up32[2], H, -1, seed)
        return idx, count
    return reference.plane_hypotheses(xyz, mask, thresh2, cos2, up32, H, seed)


def fit_plane(
    xyz: Tensor, mask: Optional[Tensor] = None, thresh: float = 0.2, hypotheses: int = 256,
    up=(0.0, 1.0, 0.0), max_tilt_deg: float = 20.0, refine_iters: int = 3, seed: int = 0,
) -> PlaneFit:
    """Robust ground-plane fit of a cloud: xyz (B,N,3), optional mask (B,N)
    bool -> ``PlaneFit``.  1 <= hypotheses <= 4096, 0 <= refine_iters <= 16,
    0 < max_tilt_deg < 90, thresh > 0, ``up`` non-zero and finite; anything
    else raises ValueError.

    ``mask`` restricts which points FIT the plane (a point is eligible if it
    is masked in and its three coordinates are finite); every finite point
    still gets a height and its labels.  A point with a non-finite
    coordinate is never drawn and reports height +INF, both labels False.

    A. ``hypotheses`` planes through seeded point triples.  With unsigned
       32-bit arithmetic
         mix(x): x ^= x>>16; x *= 0x85EBCA6B; x ^= x>>13; x *= 0xC2B2AE35; x ^= x>>16
         key(b) = mix(seed ^ mix(b*0x9E3779B1 + 1))
         draw(b,h,j,t) = mix(key(b) ^ ((h*3 + j)*8 + t)) mod N
       slot j of hypothesis h takes the first of its 8 draws that is
       eligible.  n = (p1 - p0) x (p2 - p0) in fp32, every operation rounded
       on its own.  The hypothesis is invalid if a slot stays empty, two
       slots coincide, |n|^2 is zero or non-finite, or n is tilted more than
       ``max_tilt_deg`` away from ``up``: (n.up)^2 < cos^2(max_tilt) |n|^2.
    B. count[b,h] = number of eligible points with (n.(p - p0))^2 <=
       thresh^2 |n|^2, in the same fp32 rules: an exact integer.  The largest
       count wins, ties go to the smallest h.
    C. ``refine_iters`` rounds of reweighted least squares with the Tukey
       biweight w = (1 - (height/thresh)^2)^2 inside |height| < thresh: fp64
       sums over points centred on the winner's p0, the new normal is the
       eigenvector of the smallest eigenvalue of the weighted covariance,
       the new offset puts the weighted centroid on the plane.  A round is
       rejected (and the loop ends with the previous plane) when fewer than
       3 points carry weight, the two smallest eigenvalues are not separated
       (a collinear set) or the new normal violates the tilt limit.
    D. height = normal . p + offset evaluated in fp64, rounded to fp32.

    ``ok`` is False when no hypothesis is valid (fewer than 3 eligible
    points, only vertical structure, ...): then normal = up, offset = 0, all
    heights +INF, count = 0, best = -1, rounds = 0.

    GPU: four launches (csrc/plane_fit.hip), no host synchronisation,
    bit-reproducible run to run.  Not differentiable.  bf16/fp16/fp64 or
    non-contiguous inputs are converted to contiguous fp32 here.

    The defaults (0.2 m, 256 hypotheses, 20 degrees, 3 rounds) are untuned
    guesses at metric driving scenes with y up.
    """
    thresh, thresh2, cos2, up32, H, iters, seed = reference.plane_params(
        thresh, hypotheses, up, max_tilt_deg, refine_iters, seed)
    xyz, mask = _plane_inputs("fit_plane", xyz, mask)
    B, N = xyz.shape[:2]
    if _use_hip(xyz) and B > 0 and N > 0:
        return PlaneFit(*_EXT.plane_fit(xyz, mask, thresh, thresh2, cos2, up32[0], up32[1], up32[2], H, iters, seed))
    return PlaneFit(*reference.fit_plane(xyz, mask, thresh, thresh2, cos2, up32, H, iters, seed))


# ---------------------------------------------------------------------------
# voxel-stratified sampling (csrc/voxel_sample.hip)
# ---------------------------------------------------------------------------


class VoxelSample(NamedTuple):
    """Result of ``voxel_sample``: idx (B,m) int64 chosen point indices,
    ascending, padded with -1; count (B,) int32 ``min(m, eligible points)``,
    -1 if a kernel cap was hit; rank (B,N) int32, -1 for an ineligible point,
    else the number of grid levels (0..levels) at which the point represents
    its cell; occupied (B,levels) int32 occupied cells per grid level."""

    idx: Tensor
    count: Tensor
    rank: Tensor
    occupied: Tensor


def voxel_sample(
    xyz: Tensor, m: int, voxel: float = 0.1, levels: int = 10, mask: Optional[Tensor] = None, seed: int = 0,
) -> VoxelSample:
    """Spatially even, deterministic sample of exactly ``m`` point indices
    per cloud: xyz (B,N,3), optional mask (B,N) bool -> ``VoxelSample``.
    m >= 1, voxel > 0, 1 <= levels <= 16, N < 2**27; anything else raises
    ValueError.  The same integers on every backend and in every run.

    Cells.  ``inv = fp32(1) / fp32(voxel)`` is computed on the host; per
    coordinate ``q = floor(fp32(x * inv))``.  A point is eligible iff it is
    masked, its three coordinates are finite and -2**20 <= q < 2**20 for all
    three.  ``c0 = int(q)``; the level-l cell is ``c0 >> l`` (arithmetic
    shift: negative cells floor), so the grids are nested and level l has
    edge ``voxel * 2**l``.  A product ``x * inv`` that is a denormal fp32
    number is unspecified (it may or may not be flushed to zero).

    Tag.  With unsigned 32-bit arithmetic
      mix(x): x ^= x>>16; x *= 0x85EBCA6B; x ^= x>>13; x *= 0xC2B2AE35; x ^= x>>16
      key(b) = mix(seed ^ mix(b*0x9E3779B1 + 1)),  h_i = mix(key(b) ^ i)
    and ``tag_i = (h_i << 32) | i`` as an unsigned 64-bit number.  Two points
    can share a hash (from about N = 2**16 upward they do); the index makes
    the order total, all comparisons use the 64 bits.

    Representative and rank.  The representative of an occupied level-l cell
    is its eligible member with the smallest tag.  A minimum over a union is
    the minimum of the minima, so a level-l representative also represents
    its cell at every finer level.  ``rank_i`` counts the levels at which i
    is a representative (0..levels; -1 for an ineligible point) and
    ``occupied[l]`` is the number of points with rank >= l + 1.

    Selection.  The eligible points are ordered by (rank descending, tag
    ascending); the first ``m' = min(m, eligible)`` are taken and returned in
    ascending index order, padded with -1 up to m.

    Guarantee.  Let l* be the smallest level with ``occupied[l*] <= m'``.
    Every occupied level-l* cell then contains a selected point, so every
    eligible point is within ``sqrt(3) * voxel * 2**l*`` of a sample.  If no
    such level exists (the coarsest grid has more than m' cells) nothing is
    promised: raise ``levels`` or ``voxel``; ``occupied`` is returned so the
    caller can see it.

    GPU: csrc/voxel_sample.hip, no sort: hash-table minima per level with
    integer atomics, an exact radix select of the cut tag and a compaction;
    10 + levels launches, no host synchronisation, bit-reproducible.  Every
    probe loop is capped at the table size; should a cap ever be hit, that
    cloud comes back with count = -1, idx = -1 and rank = -1 instead of a
    wrong sample.  Not differentiable.  bf16/fp16/fp64 or non-contiguous
    inputs are converted to contiguous fp32 here.

    The defaults (0.1 m, 10 levels) are untuned guesses at metric driving
    scenes: nobody has tuned them on real data.
    """
    m, inv, levels, seed = reference.voxel_params(m, voxel, levels, seed)
    if xyz.dim() != 3 or xyz.shape[-1] != 3:
        raise ValueError(f"voxel_sample needs xyz (B,N,3), got {tuple(xyz.shape)}")
    B, N = xyz.shape[:2]
    if not N < (1 << 27):
        raise ValueError(f"voxel_sample requires N < 2**27, got {N}")
    if mask is not None:
        if mask.shape != xyz.shape[:2]:
            raise ValueError(f"voxel_sample needs mask (B,N), got {tuple(mask.shape)}")
        mask = mask.detach().bool().contiguous()
    xyz = xyz.detach().float().contiguous()
    if _use_hip(xyz) and B > 0 and N > 0:
        return VoxelSample(*_EXT.voxel_sample(xyz, mask, m, inv, levels, seed))
    return VoxelSample(*reference.voxel_sample(xyz, m, inv, levels, mask, seed))


# ---------------------------------------------------------------------------
# noise filter (csrc/noise_filter.hip)
# ---------------------------------------------------------------------------


class NoiseFilter(NamedTuple):
    """Result of ``noise_filter``: keep (B,N) bool, eligible and neither sparse
    nor far; count (B,N) int32 neighbours within the radius, -1 for an
    ineligible point (all -1 if a kernel cap was hit); mean_dist (B,N) fp32
    mean distance to the k nearest neighbours, +INF if count < k, k == 0 or the
    point is ineligible; mean, std, threshold (B,) float64 statistics of the
    finite mean_dist; ok (B,) bool, False only if a capped loop hit its cap
    (then keep is all False and count all -1)."""

    keep: Tensor
    count: Tensor
    mean_dist: Tensor
    mean: Tensor
    std: Tensor
    threshold: Tensor
    ok: Tensor


def noise_filter(
    xyz: Tensor, radius: float = 0.5, min_neighbors: int = 4, k: int = 8, std_ratio: float = 2.0,
    mask: Optional[Tensor] = None,
) -> NoiseFilter:
    """Flags isolated points of a cloud by two neighbour statistics: xyz
    (B,N,3), optional mask (B,N) bool -> ``NoiseFilter``.  radius > 0,
    min_neighbors >= 0, 0 <= k <= 16, std_ratio >= 0, N < 2**27; anything else
    raises ValueError.  The same ``count`` and ``mean_dist`` bits on every
    backend and in every run.

    Cells.  ``inv = fp32(1) / fp32(radius)`` is computed on the host; per
    coordinate ``q = floor(fp32(x * inv))``.  A point is eligible iff it is
    masked, its three coordinates are finite and -2**20 <= q < 2**20 for all
    three; its cell is ``c = int(q)``: the level-0 rules of ``voxel_sample``.
    A product ``x * inv`` that is a denormal fp32 number is unspecified.

    Neighbour.  j is a neighbour of i iff j != i, both are eligible points of
    the same cloud, ``max|c_i - c_j| <= 1`` and ``d2 <= r2`` with ``r2 =
    fp32(radius) * fp32(radius)`` rounded once and ``d2 = (dx*dx + dy*dy) +
    dz*dz``, ``dx = x_i - x_j``, every operation an fp32 operation rounded on
    its own.  The cell condition is part of the definition: two points within
    a rounding error of ``radius`` can land two cells apart, and making the
    27-cell stencil the rule keeps every backend on the same integers.  The
    relation is symmetric.

    ``count_i`` is the number of neighbours; i is sparse iff ``count_i <
    min_neighbors``.  For k >= 1 and ``count_i >= k``, ``mean_dist_i`` takes
    the k smallest d2 among the neighbours (a multiset), ascending, their
    correctly rounded fp32 square roots summed left to right in fp32, divided
    by fp32(k); it does not depend on the order the neighbours are visited.

    Statistics over S, the points with finite mean_dist, in float64: ``mean``,
    the population ``std = sqrt(mean((m - mean)**2))`` in two passes, and
    ``threshold = mean + std_ratio * std``; all 0.0 when S is empty or k == 0.
    i is far iff k >= 1 and (``count_i < k`` or ``float64(mean_dist_i) >
    threshold``), against the threshold this call returns.  ``keep_i =
    eligible_i and not sparse_i and not far_i``.

    GPU: csrc/noise_filter.hip: a hashed cell grid with edge ``radius`` built
    with integer atomics, a counting sort of the points by cell, one lane per
    point over its 27 cells with the k smallest d2 in registers, fixed-order
    float64 folds; 9 launches, no (N,N) tensor, no host synchronisation,
    bit-reproducible and equivariant under a permutation of the points.  All
    points in one cell cost O(N**2) tests.  Every probe loop is capped at the
    table size; should a cap ever be hit, that cloud comes back with ok =
    False, keep all False and count all -1.  Not differentiable.
    bf16/fp16/fp64 or non-contiguous inputs are converted to contiguous fp32
    here.

    The defaults (0.5 m, 4 neighbours, k = 8, 2 sigma) are untuned guesses at
    metric driving scenes: nobody has tuned them on real data.
    """
    inv, r2, min_neighbors, k, std_ratio = reference.noise_params(radius, min_neighbors, k, std_ratio)
    if xyz.dim() != 3 or xyz.shape[-1] != 3:
        raise ValueError(f"noise_filter needs xyz (B,N,3), got {tuple(xyz.shape)}")
    B, N = xyz.shape[:2]
    if not N < (1 << 27):
        raise ValueError(f"noise_filter requires N < 2**27, got {N}")
    if mask is not None:
        if mask.shape != xyz.shape[:2]:
            raise ValueError(f"noise_filter needs mask (B,N), got {tuple(mask.shape)}")
        mask = mask.detach().bool().contiguous()
    xyz = xyz.detach().float().contiguous()
    if _use_hip(xyz) and B > 0 and N > 0:
        keep, count, md, stats, ok = _EXT.noise_filter(xyz, mask, inv, r2, k, min_neighbors, std_ratio)
    else:
        keep, count, md, stats, ok = reference.noise_filter(xyz, inv, r2, min_neighbors, k, std_ratio, mask)
    return NoiseFilter(keep, count, md, stats[:, 0], stats[:, 1], stats[:, 2], ok)


# ---------------------------------------------------------------------------
# grid nearest-neighbour search and ICP refinement (csrc/grid_nn.hip)
# ---------------------------------------------------------------------------


class NearestInRadius(NamedTuple):
    """Result of ``nearest_in_radius``: idx (B,Nq) int32 index into support,
    -1 if none; d2 (B,Nq) fp32 squared distance, +INF if none; ok (B,) bool,
    False only if a capped probe loop hit its cap (then idx is all -1)."""

    idx: Tensor
    d2: Tensor
    ok: Tensor


class IcpRefine(NamedTuple):
    """Result of ``icp_refine``: R (B,3,3), t (B,3) fp32 with dst ~ R src + t;
    idx (B,N) int32 and d2 (B,N) fp32, the correspondences and squared
    distances UNDER THE RETURNED (R, t); matched (B,) int32, the number of idx
    >= 0; rounds (B,) int32, the fits performed; ok (B,) bool."""

    R: Tensor
    t: Tensor
    idx: Tensor
    d2: Tensor
    matched: Tensor
    rounds: Tensor
    ok: Tensor


def _cloud(op: str, name: str, x: Tensor) -> Tensor:
    if x.dim() != 3 or x.shape[-1] != 3:
        raise ValueError(f"{op} needs {name} (B,N,3), got {tuple(x.shape)}")
    if not x.shape[1] < (1 << 27):
        raise ValueError(f"{op} requires N < 2**27, got {x.shape[1]} points in {name}")
    return x.detach().float().contiguous()


def _cloud_mask(op: str, name: str, mask: Optional[Tensor], x: Tensor) -> Optional[Tensor]:
    if mask is None:
        return None
    if mask.shape != x.shape[:2]:
        raise ValueError(f"{op} needs {name} (B,N), got {tuple(mask.shape)}")
    return mask.detach().bool().contiguous()


def _pose(op: str, R: Optional[Tensor], t: Optional[Tensor], B: int, names=("R", "t")):
    if (R is None) != (t is None):
        raise ValueError(f"{op} needs {names[0]} and {names[1]} together")
    if R is None:
        return None, None
    if tuple(R.shape) != (B, 3, 3) or tuple(t.shape) != (B, 3):
        raise ValueError(
            f"{op} needs {names[0]} (B,3,3) and {names[1]} (B,3), got {tuple(R.shape)}, {tuple(t.shape)}"
        )
    return R.detach().float().contiguous(), t.detach().float().contiguous()


def nearest_in_radius(
    query: Tensor, support: Tensor, radius: float, query_mask: Optional[Tensor] = None,
    support_mask: Optional[Tensor] = None, R: Optional[Tensor] = None, t: Optional[Tensor] = None,
) -> NearestInRadius:
    """Nearest support point within a radius of every query point: query
    (B,Nq,3), support (B,M,3), radius > 0, optional masks (B,Nq) / (B,M) bool,
    optional R (B,3,3) and t (B,3) applied to the query first ->
    ``NearestInRadius(idx, d2, ok)``.  Nq, M < 2**27; anything else raises
    ValueError.  The same ``idx`` integers and ``d2`` bits on every backend and
    in every run.  R and t are read from device memory, so an earlier kernel's
    output can feed them without a host round trip.

    Mapping.  With R, t the query point becomes ``x' = ((R00*x + R01*y) +
    R02*z) + t0`` and likewise y', z', every operation an fp32 operation
    rounded on its own; without them the point is used as it is.

    Cells.  ``inv = fp32(1) / fp32(radius)`` is computed on the host; per
    coordinate ``q = floor(fp32(x * inv))``.  A support point is eligible iff
    it is masked, its three coordinates are finite and -2**20 <= q < 2**20 for
    all three; its cell is ``c = int(q)``: the rules of ``noise_filter``.  A
    query is eligible by the same rules applied to the mapped point.  A product
    ``x * inv`` that is a denormal fp32 number is unspecified.

    Candidate.  j is a candidate of query i iff j is an eligible support point
    of the same batch element, ``max|c_i - c_j| <= 1`` and ``d2 <= r2`` with
    ``r2 = fp32(radius) * fp32(radius)`` rounded once and ``d2 = (dx*dx +
    dy*dy) + dz*dz``, ``dx = x'_i - x_j``, every operation an fp32 operation
    rounded on its own.  The cell condition is part of the definition, as in
    ``noise_filter``: two points within a rounding error of ``radius`` can land
    two cells apart, and making the 27-cell stencil the rule keeps every
    backend on the same integers.

    ``idx_i`` is the candidate with the smallest d2; ties go to the smallest
    j.  With no candidate, or for an ineligible query, idx = -1 and d2 = +INF.

    GPU: csrc/grid_nn.hip: the hashed cell grid and counting sort of
    ``noise_filter`` over the support (integer atomics only), then one lane per
    query over its 27 cells with the running best (d2, index) in registers; 6
    launches, no (Nq,M) tensor, no host synchronisation, bit-reproducible and
    equivariant under a permutation of either cloud.  All support points in one
    cell cost O(Nq * M) tests.  Every probe loop is capped at the table size;
    should a cap ever be hit, that cloud comes back with ok = False and idx
    all -1.  Not differentiable.  bf16/fp16/fp64 or non-contiguous inputs are
    converted to contiguous fp32 here.
    """
    op = "nearest_in_radius"
    inv, r2 = reference.radius_params(op, radius)
    query, support = _cloud(op, "query", query), _cloud(op, "support", support)
    if support.shape[0] != query.shape[0]:
        raise ValueError(f"{op} needs the same batch size, got {query.shape[0]} and {support.shape[0]}")
    query_mask = _cloud_mask(op, "query_mask", query_mask, query)
    support_mask = _cloud_mask(op, "support_mask", support_mask, support)
    R, t = _pose(op, R, t, query.shape[0])
    if _use_hip(query) and min(query.shape[0], query.shape[1], support.shape[1]) > 0:
        return NearestInRadius(*_EXT.nearest_in_radius(query, support, query_mask, support_mask, R, t, inv, r2))
    return NearestInRadius(*reference.nearest_in_radius(query, support, inv, r2, query_mask, support_mask, R, t))


def icp_refine(
    src: Tensor, dst: Tensor, R0: Optional[Tensor] = None, t0: Optional[Tensor] = None,
    max_dist: float = 1.0, thresh: float = 0.1, iters: int = 10,
    src_mask: Optional[Tensor] = None, dst_mask: Optional[Tensor] = None,
) -> IcpRefine:
    """Point-to-point ICP of src (B,N,3) against dst (B,M,3), started from
    (R0, t0) ((B,3,3), (B,3); identity / zero by default) -> ``IcpRefine(R, t,
    idx, d2, matched, rounds, ok)`` with dst ~ R src + t.  0 <= iters <= 64,
    max_dist > 0, thresh > 0, N, M < 2**27; anything else raises ValueError.

      (R, t) = (R0, t0)
      for k in 0 .. iters-1:
          (idx, d2) = nearest_in_radius(src, dst, max_dist, src_mask, dst_mask, R, t)
          if fewer than 3 matches: stop (ok = False; R, t stay as they are)
          w_i = 1 / (1 + d2_i / thresh^2) for matched i, else 0          (Cauchy)
          (R, t) = rigid_fit(src, dst[idx], weights=w, iters=0)   # absolute, from the ORIGINAL src
      (idx, d2) = nearest_in_radius(src, dst, max_dist, src_mask, dst_mask, R, t)

    ``thresh^2 = fp32(thresh) * fp32(thresh)`` is computed on the host and the
    weight is formed in fp32, both divisions correctly rounded.  A fit that
    reports ok = False (a non-finite sum) stops its cloud like too few matches
    do.  ``rounds`` counts the fits whose result was taken; a stopped cloud
    keeps the (R, t) it had, and the returned correspondences are those under
    it.  ``ok`` is False if the cloud stopped early or the search reported a
    cap.  ``iters = 0`` returns (R0, t0) with the correspondences under it.

    GPU: csrc/grid_nn.hip: the grid over dst is built once per call; every
    round is the query kernel (which also writes the matched point and the
    weight), the one-launch ``rigid_fit`` kernel and a commit kernel of one lane
    per cloud: 5 + 3 * iters + 1 launches, fixed by ``iters``.  (R, t), the
    stop flag and the match counters live in device memory: no host
    synchronisation.  Bit-reproducible run to run.  Not differentiable.

    The defaults (1.0 m, 0.1 m, 10 rounds) are untuned guesses at metric
    driving scenes: nobody has tuned them on real data.
    """
    op = "icp_refine"
    try:
        iters = int(iters)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{op}: bad argument: {e}") from None
    if not 0 <= iters <= reference.ICP_MAX_ITERS:
        raise ValueError(f"{op} requires 0 <= iters <= {reference.ICP_MAX_ITERS}, got {iters}")
    inv, r2 = reference.radius_params(op, max_dist, "max_dist")
    _, th2 = reference.radius_params(op, thresh, "thresh")
    src, dst = _cloud(op, "src", src), _cloud(op, "dst", dst)
    if dst.shape[0] != src.shape[0]:
        raise ValueError(f"{op} needs the same batch size, got {src.shape[0]} and {dst.shape[0]}")
    src_mask = _cloud_mask(op, "src_mask", src_mask, src)
    dst_mask = _cloud_mask(op, "dst_mask", dst_mask, dst)
    R0, t0 = _pose(op, R0, t0, src.shape[0], ("R0", "t0"))
    if _use_hip(src) and min(src.shape[0], src.shape[1], dst.shape[1]) > 0:
        return IcpRefine(*_EXT.icp_refine(src, dst, src_mask, dst_mask, R0, t0, inv, r2, th2, iters))
    return IcpRefine(*reference.icp_refine(src, dst, inv, r2, th2, iters, src_mask, dst_mask, R0, t0))
