"""The optimizer, the learning-rate schedules and the settings of the MinkowskiNet CSN trainer.

Reference (marios2019/CSN):
  * ``initialize_optimizer`` / ``initialize_scheduler``, ``PolyLR`` / ``SquaredLR`` / ``ExpLR``     MinkowskiNet/lib/solvers.py:7-81
  * the settings and their defaults                                                              MinkowskiNet/lib/config.py:43-142

The lambda schedules count ITERATIONS (the trainer steps them once per ``optimizer.step()``); with s the step counter their
multipliers on the base rate are
    PolyLR      (1 - s / (max_iter + 1)) ** poly_power
    SquaredLR   (1 - s / (max_iter + 1)) ** 2
    ExpLR       exp_gamma ** (s / exp_step_size)
``StepLR`` and ``ReduceLROnPlateau`` are torch's classes.  Settings are data: ``TrainConfig`` restates the names and defaults of the
fields ``csn_amd.minkowski_trainer.CSNTrainer`` reads, nothing else of the reference's argument parser.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

from torch.optim import SGD, Adam
from torch.optim.lr_scheduler import LambdaLR, ReduceLROnPlateau, StepLR

OPTIMIZERS = ("SGD", "Adam")
SCHEDULERS = ("StepLR", "PolyLR", "SquaredLR", "ExpLR", "ReduceLROnPlateau")


@dataclass
class TrainConfig:
    """The settings the trainer uses, with config.py's defaults (``model``: config.py has None, the launch script passes
    ``HRNetSimCSN3S``)."""
    # optimizer
    lr: float = 1e-2
    optimizer: str = "SGD"
    sgd_momentum: float = 0.9
    sgd_dampening: float = 0.1
    weight_decay: float = 1e-4
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    # scheduler
    scheduler: str = "StepLR"
    max_iter: int = 60000
    poly_power: float = 0.9
    step_size: int = 10000
    step_gamma: float = 0.5
    exp_step_size: int = 445
    exp_gamma: float = 0.99
    # the loop
    max_epoch: int = 200
    iter_size: int = 1
    batch_size: int = 16
    k_neighbors: int = 1
    ignore_label: int = 255
    voxel_size: float = 0.05
    stat_freq: int = 40
    # checkpoints
    resume: Optional[str] = None
    resume_optimizer: bool = True
    log_dir: str = "outputs/default"
    model: str = "HRNetSimCSN3S"


def initialize_optimizer(params, cfg):
    """solvers.py:45-63: SGD (momentum, dampening, weight decay) or Adam (betas, weight decay); anything else is a ValueError."""
    if cfg.optimizer == "SGD":
        return SGD(params, lr=cfg.lr, momentum=cfg.sgd_momentum, dampening=cfg.sgd_dampening, weight_decay=cfg.weight_decay)
    if cfg.optimizer == "Adam":
        return Adam(params, lr=cfg.lr, betas=(cfg.adam_beta1, cfg.adam_beta2), weight_decay=cfg.weight_decay)
    raise ValueError(f"optimizer '{cfg.optimizer}' is not supported: one of {OPTIMIZERS}")


class _PolyFactor:
    """Module-level callables, not lambdas: a scheduler holding one pickles."""

    def __init__(self, max_iter, power):
        self.max_iter, self.power = max_iter, power

    def __call__(self, s):
        return (1 - s / (self.max_iter + 1)) ** self.power


class _ExpFactor:
    def __init__(self, step_size, gamma):
        self.step_size, self.gamma = step_size, gamma

    def __call__(self, s):
        return self.gamma ** (s / self.step_size)


class LambdaStepLR(LambdaLR):
    """``LambdaLR`` whose counter is named for what it counts here (solvers.py:7-19)."""

    def __init__(self, optimizer, lr_lambda, last_step=-1):
        super().__init__(optimizer, lr_lambda, last_step)

    @property
    def last_step(self):
        return self.last_epoch

    @last_step.setter
    def last_step(self, v):
        self.last_epoch = v


class PolyLR(LambdaStepLR):
    def __init__(self, optimizer, max_iter, power=0.9, last_step=-1):
        super().__init__(optimizer, _PolyFactor(max_iter, power), last_step)


class SquaredLR(LambdaStepLR):
    def __init__(self, optimizer, max_iter, last_step=-1):
        super().__init__(optimizer, _PolyFactor(max_iter, 2), last_step)


class ExpLR(LambdaStepLR):
    def __init__(self, optimizer, step_size, gamma=0.9, last_step=-1):
        super().__init__(optimizer, _ExpFactor(step_size, gamma), last_step)


def initialize_scheduler(optimizer, cfg, last_step=-1, factor=0.5, patience=10, cooldown=10):
    """solvers.py:66-80.  ``last_step >= 0`` continues a schedule at that step: torch then wants ``initial_lr`` in every parameter
    group, which is the group's current rate where it is not there yet — so set the rate to ``cfg.lr`` first, as the trainer does.
    ``factor`` / ``patience`` / ``cooldown`` reach ``ReduceLROnPlateau`` alone.  An unknown name is a ValueError (the reference logs
    and returns None)."""
    if last_step >= 0:
        for group in optimizer.param_groups:
            group.setdefault("initial_lr", group["lr"])
    if cfg.scheduler == "StepLR":
        return StepLR(optimizer, step_size=cfg.step_size, gamma=cfg.step_gamma, last_epoch=last_step)
    if cfg.scheduler == "PolyLR":
        return PolyLR(optimizer, max_iter=cfg.max_iter, power=cfg.poly_power, last_step=last_step)
    if cfg.scheduler == "SquaredLR":
        return SquaredLR(optimizer, max_iter=cfg.max_iter, last_step=last_step)
    if cfg.scheduler == "ExpLR":
        return ExpLR(optimizer, step_size=cfg.exp_step_size, gamma=cfg.exp_gamma, last_step=last_step)
    if cfg.scheduler == "ReduceLROnPlateau":
        return ReduceLROnPlateau(optimizer, patience=patience, cooldown=cooldown, factor=factor)
    raise ValueError(f"scheduler '{cfg.scheduler}' is not supported: one of {SCHEDULERS}")
