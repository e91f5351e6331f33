"""Self-supervised training engine (absent in the reference).

Same skeleton as Trainer; differences:
* loss = self_supervised_loss (Chamfer distance of the warped cloud +
  flow smoothness over pc1's kNN graph) on every GRU iteration's flow with
  the sequence-loss gamma weighting; batch["ground_truth"] is never read
  by the loss, so unlabelled pairs can be trained on.
* train steps run EAGERLY: the loss adds a kNN-graph build and a CSR
  argsort to the step, and in-capture sorts disturb the graph-pool layout
  (see graphed.py), so the step is never captured into a hipGraph.
* validation is unchanged: the captured Predictor path, EPE / accuracy
  from the dataset's ground truth, best_checkpoint.params by val EPE.
"""

from __future__ import annotations

from pvraft_amd.data import Batch
from pvraft_amd.utils import self_supervised_loss

from .trainer import Trainer


class SelfSupTrainer(Trainer):
    def _loss(self, est_flow, batch):
        a = self.args
        return self_supervised_loss(
            est_flow,
            batch,
            gamma=a.gamma,
            chamfer_weight=getattr(a, "chamfer_weight", 1.0),
            smooth_weight=getattr(a, "smooth_weight", 1.0),
            smooth_k=getattr(a, "smooth_k", 9),
        )

    def _ensure_graph(self, batch: Batch) -> bool:
        """Never capture the train step (Trainer.train_step then runs it
        eagerly); _graph_enabled still lets validation use its graph."""
        return False
