"""Scene-flow dataset base class (reference datasets/generic.py:69-215).

Each item: {"sequence": [pc1 (1,n,3), pc2 (1,m,3)],
            "ground_truth": [mask (1,n,1), flow (1,n,3)]}.
Point clouds are randomly subsampled to nb_points.  Samples with fewer
points than nb_points are skipped forward to the next index; unlike the
reference (generic.py:101-110, which can run off the end of the dataset)
the scan wraps around modulo len(self).
"""

from __future__ import annotations

import numpy as np
import torch
from torch.utils.data import Dataset


class SceneFlowDataset(Dataset):
    # opt-in: items also carry "full": [pc1_full (1,n,3), mask_full (1,n,1),
    # flow_full (1,n,3)], the first cloud and its ground truth BEFORE
    # subsampling (dense-flow evaluation)
    return_full = False
    # opt-in: items also carry "full2": [pc2_full (1,m,3)], the second cloud
    # BEFORE subsampling, under the same contract (a reference to the
    # pre-subsample array, no extra RNG draw): evaluation that draws its own
    # samples from both full clouds (ops.voxel_sample)
    return_full2 = False
    # opt-in: loaders that strip the ground with a fixed rule (Kitti: y < -1.4)
    # keep it, for users who segment the ground themselves (ops.fit_plane)
    keep_ground = False

    def __init__(self, nb_points: int):
        super().__init__()
        self.nb_points = nb_points

    def __getitem__(self, idx: int):
        for attempt in range(len(self)):
            data = self._load_item((idx + attempt) % len(self))
            n = data["sequence"][0].shape[1]
            m = data["sequence"][1].shape[1]
            if n == self.nb_points and m == self.nb_points:
                return data
        raise RuntimeError(
            f"No sample in {type(self).__name__} has >= {self.nb_points} points"
        )

    def _load_item(self, idx: int):
        sequence, ground_truth = self.load_sequence(idx)
        full = None
        if self.return_full:
            # references to the pre-subsample arrays (subsample_points
            # rebinds, never mutates); no extra RNG draw
            full = [sequence[0], ground_truth[0], ground_truth[1]]
        full2 = [sequence[1]] if self.return_full2 else None
        sequence, ground_truth = self.subsample_points(sequence, ground_truth)
        sequence, ground_truth = self.to_torch(sequence, ground_truth)
        data = {"sequence": sequence, "ground_truth": ground_truth}
        if full is not None:
            data["full"] = self.to_torch(full, [])[0]
        if full2 is not None:
            data["full2"] = self.to_torch(full2, [])[0]
        return data

    @staticmethod
    def to_torch(sequence, ground_truth):
        sequence = [torch.from_numpy(np.ascontiguousarray(s)).float().unsqueeze(0) for s in sequence]
        ground_truth = [torch.from_numpy(np.ascontiguousarray(g)).float().unsqueeze(0) for g in ground_truth]
        return sequence, ground_truth

    def subsample_points(self, sequence, ground_truth):
        ind1 = np.random.permutation(sequence[0].shape[0])[: self.nb_points]
        sequence[0] = sequence[0][ind1]
        ground_truth = [g[ind1] for g in ground_truth]
        ind2 = np.random.permutation(sequence[1].shape[0])[: self.nb_points]
        sequence[1] = sequence[1][ind2]
        return sequence, ground_truth

    def load_sequence(self, idx: int):
        """Return ([pc1 (N,3), pc2 (M,3)], [mask (N,1), flow (N,3)]) numpy arrays."""
        raise NotImplementedError
