from .losses import DiceLoss, DiceCELoss, TverskyLoss, CrossEntropyLoss, get_loss  # noqa: F401
from .metrics import (ConfusionMatrix, DiceMetric, HausdorffDistance, distance_transform_edt,  # noqa: F401
                      get_metrics)
from .optim import FlatAdamW  # noqa: F401
from .trainer import Trainer  # noqa: F401
