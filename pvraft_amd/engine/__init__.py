from .trainer import Trainer, VAL_ITERS
from .refine_trainer import RefineTrainer
from .selfsup_trainer import SelfSupTrainer
from .predictor import Predictor
