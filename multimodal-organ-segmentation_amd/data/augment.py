"""Device-side training augmentation: the reference's RandomFlip, RandomRotate90, RandomIntensityShift and
RandomGaussianNoise (src/data/transforms.py:32-139, composed by get_transforms, transforms.py:428-443) as
one HIP launch per sample (mmseg_augment, csrc/data.hip).

The random decisions are drawn on the host from a `random.Random` in exactly the order the reference
consumes Python's global `random` (draw_augment_params), so a seed gives the reference's flips, rotation
and per-channel intensity affine bit for bit.  Only the noise values come from a stream of our own (the
phantom generator's SplitMix64 counter stream): the reference takes them from numpy's global state, so the
noise has statistical parity only.  sample_rng keys the draws on (seed, epoch, global sample index), which
makes the augmentation independent of rank and world size under data parallelism.
"""
from __future__ import annotations

import ctypes
import random
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence

import torch

from .._lib import lib, ptr, stream_handle

NOISE_PROB, NOISE_MEAN, NOISE_SD = 0.2, 0.0, 0.05     # get_transforms: RandomGaussianNoise(std=0.05, prob=0.2)
_M64 = (1 << 64) - 1


@dataclass
class AugmentParams:
    """One sample's draws: flip per spatial axis (D, H, W), k quarter turns over (D, H), per-channel
    intensity affine (None = not fired), and the noise switch with its stream key."""
    flip: Sequence[bool] = (False, False, False)
    k: int = 0
    scale: Optional[List[float]] = None
    shift: Optional[List[float]] = None
    noise: bool = False
    noise_key: int = 0
    noise_mean: float = NOISE_MEAN
    noise_sd: float = NOISE_SD


def draw_augment_params(rng: random.Random, aug_cfg: Dict[str, Any], n_channels: int) -> AugmentParams:
    """Consume `rng` as get_transforms' train pipeline consumes `random` (transforms.py:428-443)."""
    p = AugmentParams()
    if aug_cfg.get("random_flip", True):
        p.flip = tuple(rng.random() < 0.5 for _ in range(3))
    if aug_cfg.get("random_rotate", 0) > 0:
        if rng.random() < 0.5:
            p.k = rng.randint(1, 3)
    s = aug_cfg.get("random_intensity", 0)
    if s > 0:
        if rng.random() < 0.3:
            p.shift, p.scale = [], []
            for _ in range(n_channels):
                p.shift.append(rng.uniform(-s, s))
                p.scale.append(rng.uniform(0.9, 1.1))
    p.noise = rng.random() < NOISE_PROB
    if p.noise:      # drawn last, so the reference's own sequence is undisturbed
        p.noise_key = rng.getrandbits(64)
    return p


def sample_rng(seed: int, epoch: int, index: int) -> random.Random:
    """The draw stream of global sample `index` in `epoch`: the same for every rank and world size."""
    return random.Random(((int(seed) & _M64) << 128) | ((int(epoch) & _M64) << 64) | (int(index) & _M64))


class DeviceAugment:
    """sample["image"] [C, D, H, W] fp32 and (optional) sample["label"] [D, H, W] int64 / uint8, both on the
    device, augmented out of place in one launch."""

    def __init__(self, aug_cfg: Optional[Dict[str, Any]] = None):
        self.cfg = dict(aug_cfg or {})

    def apply(self, sample: Dict[str, Any], params: AugmentParams) -> Dict[str, Any]:
        img = sample["image"]
        if img.device.type != "cuda":
            raise RuntimeError(f"DeviceAugment: the device data path needs ROCm tensors (got {img.device}); "
                               "there is no CPU path")
        if img.dim() != 4 or img.dtype != torch.float32:
            raise ValueError("DeviceAugment: image [C, D, H, W] float32")
        img = img.contiguous()
        C, D, H, W = img.shape
        Do, Ho = (H, D) if params.k % 2 else (D, H)
        out = torch.empty(C, Do, Ho, W, dtype=torch.float32, device=img.device)
        lab = sample.get("label")
        lab_out = None
        if lab is not None:
            if lab.device != img.device or tuple(lab.shape) != (D, H, W):
                raise ValueError("DeviceAugment: label [D, H, W] on the image's device")
            lab = lab.contiguous()
            lab_out = torch.empty(Do, Ho, W, dtype=lab.dtype, device=lab.device)
        scale = shift = None
        if params.scale is not None:
            if len(params.scale) != C or len(params.shift) != C:
                raise ValueError(f"DeviceAugment: {C} channels need {C} scales and shifts")
            scale = (ctypes.c_float * C)(*params.scale)
            shift = (ctypes.c_float * C)(*params.shift)
        key = ctypes.c_ulonglong(params.noise_key & _M64)
        flip_mask = sum(1 << a for a in range(3) if params.flip[a])
        lib().mmseg_augment(ptr(img), C, D, H, W, ptr(lab), lab.element_size() if lab is not None else 0,
                            flip_mask, int(params.k),
                            ctypes.addressof(scale) if scale is not None else None,
                            ctypes.addressof(shift) if shift is not None else None,
                            int(bool(params.noise)), float(params.noise_mean), float(params.noise_sd),
                            ctypes.addressof(key), ptr(out), ptr(lab_out), stream_handle())
        sample["image"] = out
        if lab is not None:
            sample["label"] = lab_out
        return sample

    def __call__(self, sample: Dict[str, Any], epoch: int, index: int, seed: int) -> Dict[str, Any]:
        params = draw_augment_params(sample_rng(seed, epoch, index), self.cfg, sample["image"].shape[0])
        return self.apply(sample, params)
