"""Synthetic scene-flow pairs for benchmarking and tests.

Random point clouds with a smooth synthetic flow field, shaped exactly like
the FT3D samples (pc1/pc2 point-aligned, mask all ones, flow = pc2 - pc1).
Used when no real dataset is on disk (this environment has no network) --
bench.py and the plumbing tests run on these.
"""

from __future__ import annotations

import numpy as np
import torch

from .base import SceneFlowDataset
from .batch import Batch


class SyntheticSceneFlow(SceneFlowDataset):
    def __init__(self, nb_points: int, length: int = 256, seed: int = 0, extent: float = 10.0,
                 full_points=None, ground_fraction: float = 0.0, noise_fraction: float = 0.0):
        super().__init__(nb_points)
        if not 0.0 <= float(noise_fraction) < 1.0:
            raise ValueError(f"noise_fraction must be in [0, 1), got {noise_fraction}")
        # share of the points replaced in both clouds by points uniform in
        # the scene's bounding volume, with zero-flow ground truth that is
        # masked out; 0 keeps the historical stream
        self.noise_fraction = float(noise_fraction)
        if not 0.0 <= float(ground_fraction) < 1.0:
            raise ValueError(f"ground_fraction must be in [0, 1), got {ground_fraction}")
        # share of the points that lies on the plane y = -1.4 (2 cm noise)
        # and follows the same rigid motion; 0 keeps the historical stream
        self.ground_fraction = float(ground_fraction)
        self.length = length
        self.seed = seed
        self.extent = extent
        # clouds are generated with full_points points (>= nb_points) and
        # subsampled to nb_points; None keeps the historical stream
        self.full_points = full_points

    def __len__(self):
        return self.length

    def load_sequence(self, idx: int):
        rng = np.random.default_rng(self.seed * 1_000_003 + idx)
        n = self.nb_points if self.full_points is None else self.full_points
        pc1 = (rng.random((n, 3), dtype=np.float32) - 0.5) * self.extent
        # smooth flow: global translation + small rotation + noise
        t = rng.normal(0.0, 0.5, size=(1, 3)).astype(np.float32)
        ang = rng.normal(0.0, 0.02)
        c, s = np.cos(ang, dtype=np.float32), np.sin(ang, dtype=np.float32)
        rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32)
        noise = rng.normal(0.0, 0.01, size=(n, 3)).astype(np.float32)
        if self.ground_fraction > 0:
            # drawn after everything above: the default stream is untouched
            k = int(round(self.ground_fraction * n))
            sel = rng.permutation(n)[:k]
            pc1[sel, 1] = (-1.4 + rng.normal(0.0, 0.02, size=k)).astype(np.float32)
        pc2 = pc1 @ rot.T + t + noise
        ground_truth = [np.ones_like(pc1[:, 0:1]), pc2 - pc1]
        if self.noise_fraction > 0:
            # drawn after everything above: the default stream is untouched
            k = int(round(self.noise_fraction * n))
            sel = rng.permutation(n)[:k]
            lo = np.minimum(pc1.min(0), pc2.min(0))
            hi = np.maximum(pc1.max(0), pc2.max(0))
            pc1[sel] = (lo + rng.random((k, 3)) * (hi - lo)).astype(np.float32)
            pc2[sel] = (lo + rng.random((k, 3)) * (hi - lo)).astype(np.float32)
            ground_truth[0][sel] = 0.0
            ground_truth[1][sel] = 0.0
        return [pc1, pc2], ground_truth


def synthetic_batch(
    batch_size: int, nb_points: int, device="cpu", seed: int = 0
) -> Batch:
    ds = SyntheticSceneFlow(nb_points, length=batch_size, seed=seed)
    return Batch([ds[i] for i in range(batch_size)]).to(device)
