"""Inference wrapper: hipGraph-captured scene-flow prediction.

Evaluation/serving runs the backbone 32 GRU iterations per pair
(reference test.py:120) with fixed shapes (bs x max_points), so the whole
no-grad forward is captured once and replayed per sample -- the same
launch-collapse as the training step, applied to serving.

    pred = Predictor(model, points=8192, batch=1, iters=32)
    flow = pred(xyz1, xyz2)   # (B, N, 3)

    # flow for every point of full-resolution clouds (batch-1 predictors):
    dense = pred.predict_dense(pc1_full, pc2_full, k=3)   # (n1, 3)
    # ... of raw scans that still contain the ground:
    dense = pred.predict_dense(pc1_full, pc2_full, remove_ground=True)
    # ... that also contain isolated noise points:
    dense = pred.predict_dense(pc1_full, pc2_full, sampling="voxel", remove_noise=True)

    # flow plus the ego-motion it implies and a static/dynamic split:
    flow, ego = pred.predict_ego_motion(xyz1, xyz2)       # ego.R, ego.t, ...
    # ... refined by ICP against the full-resolution second scan:
    flow, ego, icp = pred.predict_ego_motion(xyz1, xyz2, icp=True, target=pc2_full)

    # flow plus the moving objects in it, each with its own rigid motion:
    flow, om = pred.predict_object_motion(xyz1, xyz2)     # om.labels, om.R, ...
"""

from __future__ import annotations

from typing import Optional

import torch


class Predictor:
    def __init__(self, model, points: int, batch: int = 1, iters: int = 32,
                 amp: bool = False, use_graph: bool = True):
        self.model = model.eval()
        self.iters = iters
        self.amp = amp
        self.device = next(model.parameters()).device
        # ROOT-CAUSED TOOLCHAIN BUG (round 2, profiles/README.md): hipGraph
        # replay of the inference forward at batch >= 5 faults in the ROCm
        # graph-pool page mapping -- the PURE-ATEN forward (PVRAFT_REF_OPS=1,
        # zero custom kernels) reproduces it identically ("write access to a
        # read-only page" / aperture violation on first replay), eager is
        # clean at every batch size under strict per-tensor allocation, and
        # batch <= 4 graphs are exercised throughout training/eval.
        # Repros: scripts/stress_graph_bs.py, scripts/graph_region_bisect.py.
        # Permanent guard: serve batch >= 5 eagerly on this toolchain.
        self.use_graph = use_graph and self.device.type == "cuda" and batch <= 4
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._in1 = torch.zeros(batch, points, 3, device=self.device)
        self._in2 = torch.zeros(batch, points, 3, device=self.device)
        self._flows = None
        self.last_flows = None

    def _forward(self):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.amp):
            flows = self.model([self._in1, self._in2], num_iters=self.iters)
        if not isinstance(flows, (list, tuple)):
            flows = [flows]
        return [f.float() for f in flows]

    def _capture(self) -> None:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._forward()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self._graph = torch.cuda.CUDAGraph()
        # capture on the warmup stream (see engine/graphed.py: nodes
        # pinned to another stream record cross-stream work that races
        # at replay)
        with torch.cuda.graph(self._graph, stream=s):
            self._flows = self._forward()

    @torch.no_grad()
    def __call__(self, xyz1: torch.Tensor, xyz2: torch.Tensor) -> torch.Tensor:
        """Returns the FINAL flow (B, N, 3); ``last_flows`` holds the whole
        per-iteration list (static graph outputs -- consume before the next
        call) for sequence-loss evaluation."""
        if not self.use_graph:
            self._in1, self._in2 = xyz1.to(self.device), xyz2.to(self.device)
            self.last_flows = self._forward()
            return self.last_flows[-1]
        if self._graph is None:
            self._in1.copy_(xyz1)
            self._in2.copy_(xyz2)
            self._capture()
        self._in1.copy_(xyz1, non_blocking=True)
        self._in2.copy_(xyz2, non_blocking=True)
        self._graph.replay()
        self.last_flows = self._flows
        return self._flows[-1].clone()

    @torch.no_grad()
    def predict_ego_motion(self, xyz1: torch.Tensor, xyz2: torch.Tensor,
                           thresh: float = 0.05, iters: int = 10, icp: bool = False,
                           icp_kw: Optional[dict] = None, target: Optional[torch.Tensor] = None):
        """(flow (B,N,3), ``ops.EgoMotion``): the usual forward (graph
        replay as in ``__call__``), then the robust rigid fit of the final
        flow -- one fused launch, run eagerly after the replay without
        draining the stream.  Works for any predictor batch.

        ``icp=True`` returns (flow, ego, ``ops.IcpRefine``): the fitted motion
        refined by point-to-point ICP of the static points of ``xyz1`` against
        ``target`` ((B,M,3), e.g. the full-resolution second scan; ``xyz2``
        when it is None), ``ops.icp_refine(xyz1, target, R0=ego.R, t0=ego.t,
        src_mask=ego.static, **icp_kw)``.  It reads ego.R / ego.t on the
        device: still no host synchronisation.  ``icp.d2`` is a per-point
        geometric residual that needs no ground truth.  Without ``icp`` the
        return value is the pair it always was."""
        from pvraft_amd import ops

        flow = self(xyz1, xyz2)
        pc1 = xyz1.to(self.device).float()
        ego = ops.ego_motion(pc1, flow, thresh=thresh, iters=iters)
        if not icp:
            return flow, ego
        dst = (xyz2 if target is None else target).to(self.device).float()
        refined = ops.icp_refine(pc1, dst, R0=ego.R, t0=ego.t, src_mask=ego.static, **(icp_kw or {}))
        return flow, ego, refined

    @torch.no_grad()
    def predict_object_motion(self, xyz1: torch.Tensor, xyz2: torch.Tensor, **kw):
        """(flow (B,N,3), ``ops.ObjectMotion``): the usual forward (graph
        replay as in ``__call__``), then ``ops.object_motion`` of the final
        flow (ego fit, clustering of the non-static points, one rigid fit
        per object), run eagerly after the replay without draining the
        stream.  Keyword arguments go to ``ops.object_motion``.  Works for
        any predictor batch."""
        from pvraft_amd import ops

        flow = self(xyz1, xyz2)
        om = ops.object_motion(xyz1.to(self.device).float(), flow, **kw)
        return flow, om

    @torch.no_grad()
    def predict_dense(self, pc1_full: torch.Tensor, pc2_full: torch.Tensor, k: int = 3,
                      generator: Optional[torch.Generator] = None,
                      return_sparse: bool = False, remove_ground: bool = False,
                      ground_kw: Optional[dict] = None, sampling: str = "random",
                      sample_kw: Optional[dict] = None, remove_noise: bool = False,
                      noise_kw: Optional[dict] = None):
        """Flow for EVERY point of ``pc1_full`` ((n1,3) or (1,n1,3)).

        Draws ``points`` indices without replacement from each full cloud
        (``torch.randperm`` with ``generator``, so a seeded generator makes
        the call reproducible), runs the fixed-shape forward on the samples
        (graph replay as in ``__call__``), then interpolates the sparse flow
        onto the full cloud with ``ops.knn_interpolate`` -- eagerly, outside
        the captured graph, because n1 differs per sample.

        Returns flow (n1, 3) in ``pc1_full``'s dtype on the predictor's
        device; with ``return_sparse`` the tuple (flow, idx1, flow_sub):
        idx1 (points,) int64 indices into pc1_full and the sparse flow
        flow_sub (points, 3) predicted at them.

        ``remove_ground=True`` is for raw scans that still contain the
        ground (the network was trained on clouds without it): each full
        cloud gets its own ``ops.fit_plane(cloud, **ground_kw)`` and the
        samples are drawn, with the same ``randperm`` mechanics, only among
        that cloud's non-ground points (``~fit.ground``: above the plane by
        more than ``thresh``).  The dense flow still covers every point of
        ``pc1_full``, ground included, and with ``return_sparse`` the tuple
        gains a fourth entry, the (n1,) bool ground mask of ``pc1_full``.
        Fewer than ``points`` non-ground points in a cloud raise ValueError.
        Compacting the non-ground indices reads their count on the host:
        one synchronisation per cloud, in this eager pre-phase only.

        ``sampling="voxel"`` replaces the uniform draw of each cloud by
        ``ops.voxel_sample(cloud, points, **sample_kw)``: spatially even,
        deterministic (``seed`` comes from ``sample_kw``; ``generator`` is
        not consumed) and ascending, so ``idx1`` is sorted.  With
        ``remove_ground`` the non-ground mask goes in as the sampler's
        ``mask`` (no compaction).  Reading the sampler's ``count`` to raise
        the ValueError for a cloud with fewer than ``points`` usable points
        is the one host synchronisation per cloud.  Any other ``sampling``
        than "random" or "voxel" raises ValueError.

        ``remove_noise=True`` keeps isolated points (flying pixels, returns
        from rain or dust) out of the samples: each full cloud gets its own
        ``ops.noise_filter(cloud, **noise_kw)`` on the WHOLE cloud (with
        ``remove_ground`` the ground is not masked out first: points just
        above it would lose their neighbours) and the usable points are
        ``keep``, and additionally ``~ground`` with ``remove_ground``.  With
        ``sampling="voxel"`` that goes in as the sampler's mask, with
        "random" it takes the compaction path of ``remove_ground``; the count
        checks, their messages and the one host synchronisation per cloud are
        the same.  The dense flow still covers every point, and with
        ``return_sparse`` the tuple gains a LAST entry, the (n1,) bool noise
        mask ``~keep`` of ``pc1_full``.
        """
        from pvraft_amd import ops

        if sampling not in ("random", "voxel"):
            raise ValueError(f'sampling must be "random" or "voxel", got {sampling!r}')
        batch, points = self._in1.shape[0], self._in1.shape[1]
        if batch != 1:
            raise ValueError(f"predict_dense needs a batch-1 Predictor, this one has batch={batch}")
        clouds = []
        for name, pc in (("pc1_full", pc1_full), ("pc2_full", pc2_full)):
            if pc.dim() == 3 and pc.shape[0] == 1:
                pc = pc[0]
            if pc.dim() != 2 or pc.shape[1] != 3:
                raise ValueError(f"{name} must be (n,3) or (1,n,3), got {tuple(pc.shape)}")
            if pc.shape[0] < points:
                raise ValueError(
                    f"{name} has {pc.shape[0]} points, fewer than the {points} the predictor samples"
                )
            clouds.append(pc.to(self.device))
        gdev = generator.device if generator is not None else torch.device("cpu")
        subs, idxs = [], []
        ground1 = None
        noise1 = None
        for name, pc in zip(("pc1_full", "pc2_full"), clouds):
            usable_mask = None  # (1, n) bool, None: every point
            if remove_ground:
                fit = ops.fit_plane(pc.float().unsqueeze(0), **(ground_kw or {}))
                if ground1 is None:
                    ground1 = fit.ground[0]
                usable_mask = ~fit.ground
            if remove_noise:
                nf = ops.noise_filter(pc.float().unsqueeze(0), **(noise_kw or {}))
                if noise1 is None:
                    noise1 = ~nf.keep[0]
                usable_mask = nf.keep if usable_mask is None else usable_mask & nf.keep
            if sampling == "voxel":
                vs = ops.voxel_sample(pc.float().unsqueeze(0), points, mask=usable_mask, **(sample_kw or {}))
                usable = int(vs.count[0])  # host sync: the count
                if usable < points:
                    raise ValueError(
                        f"{name} has {usable} points the voxel sampler can use, fewer than the {points} "
                        "the predictor samples"
                    )
                idx = vs.idx[0]
            elif usable_mask is not None:
                keep = usable_mask[0].nonzero().squeeze(1)  # host sync: the count
                if keep.numel() < points:
                    what = "non-ground" if not remove_noise else ("usable" if remove_ground else "non-noise")
                    raise ValueError(
                        f"{name} has {keep.numel()} {what} points, fewer than the {points} the predictor samples"
                    )
                sel = torch.randperm(keep.numel(), generator=generator, device=gdev)[:points].to(self.device)
                idx = keep[sel]
            else:
                idx = torch.randperm(pc.shape[0], generator=generator, device=gdev)[:points].to(self.device)
            idxs.append(idx)
            subs.append(pc[idx].float().unsqueeze(0))
        flow_sub = self(subs[0], subs[1])  # (1, points, 3)
        dense, _, _ = ops.knn_interpolate(subs[0], flow_sub, clouds[0].float().unsqueeze(0), k)
        dense = dense[0].to(pc1_full.dtype)
        if return_sparse:
            out = (dense, idxs[0], flow_sub[0])
            if remove_ground:
                out = out + (ground1,)
            if remove_noise:
                out = out + (noise1,)
            return out
        return dense
