"""Device augmentation (mmseg_augment, csrc/data.hip, through data/augment.py) on the GPU: the geometry, the
two-rounding intensity affine and the label bit for bit against the numpy restatement (tests/augment_ref.py)
and against the reference's own output (tests/golden/augment.npz); the noise within 1e-6 of the restated
SplitMix64 stream (the bound test_phantom_matches_oracle uses for the same stream: the device's fp64 log / cos
differ from numpy's in the last bits); the loader wiring and two training steps on augmented batches."""
import copy
import functools
import random

import numpy as np
import pytest
import torch

import mmseg_amd  # noqa: F401
from mmseg_amd._lib import MmsegError
from mmseg_amd.data import AugmentParams, DeviceAugment, draw_augment_params, get_dataloader
from tests.augment_ref import apply_params
from tests.helpers import golden

pytestmark = pytest.mark.gpu
AUG = {"enabled": True, "random_flip": True, "random_rotate": 15, "random_intensity": 0.1}


@functools.lru_cache(maxsize=None)
def _volume(shape):
    rng = np.random.Generator(np.random.PCG64(sum(shape)))
    image = rng.standard_normal(shape, dtype=np.float32)
    label = rng.integers(0, 200, size=shape[1:]).astype(np.int64)
    image.setflags(write=False)
    label.setflags(write=False)
    return image, label


def _run(dev, image, label, p):
    sample = {"image": torch.from_numpy(np.array(image)).to(dev)}
    if label is not None:
        sample["label"] = torch.from_numpy(np.array(label)).to(dev)
    out = DeviceAugment().apply(sample, p)
    return out["image"].cpu().numpy(), out["label"].cpu().numpy() if label is not None else None


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("label_dtype", [np.int64, np.uint8])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("mask", range(8))
def test_geometry_all_flips_and_rotations(dev, mask, k, label_dtype):
    image, label = _volume((2, 5, 7, 9))
    label = label.astype(label_dtype)
    p = AugmentParams(flip=tuple(bool(mask >> a & 1) for a in range(3)), k=k)
    got_img, got_lab = _run(dev, image, label, p)
    ref_img, ref_lab = apply_params(image, label, p)
    assert _bits_equal(got_img, ref_img)
    assert got_lab.dtype == label_dtype and np.array_equal(got_lab, ref_lab)


def test_geometry_without_label(dev):
    image, _ = _volume((2, 5, 7, 9))
    p = AugmentParams(flip=(True, False, True), k=3)
    got_img, got_lab = _run(dev, image, None, p)
    assert got_lab is None and _bits_equal(got_img, apply_params(image, None, p)[0])


# rows longer than a block and not a multiple of 4 (scalar tail, reversed reads) | aligned vectors | short rows
@pytest.mark.parametrize("shape", [(1, 3, 2, 261), (2, 4, 6, 64), (3, 2, 3, 6)])
@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("xflip", [False, True])
def test_row_paths(dev, shape, k, xflip):
    image, label = _volume(shape)
    C = shape[0]
    p = AugmentParams(flip=(False, True, xflip), k=k, scale=[1.05 - 0.03 * c for c in range(C)],
                      shift=[0.07 * c - 0.05 for c in range(C)])
    for lab in (label, label.astype(np.uint8)):
        got_img, got_lab = _run(dev, image, lab, p)
        ref_img, ref_lab = apply_params(image, lab, p)
        assert _bits_equal(got_img, ref_img)
        assert np.array_equal(got_lab, ref_lab)


def test_reference_golden(dev):
    """Every fixture seed: the drawn parameters through the kernel, noise forced off, against what the
    reference's RandomFlip / RandomRotate90 / RandomIntensityShift produced -- bit-exact, so an affine fused
    into one FMA fails here."""
    g = golden("augment")
    cfg = dict(AUG, random_intensity=float(g["random_intensity"]))
    fired = 0
    for seed in g["seeds"]:
        p = draw_augment_params(random.Random(int(seed)), cfg, 2)
        p.noise = False
        fired += p.scale is not None
        got_img, got_lab = _run(dev, g["image_in"], g["label_in"], p)
        assert _bits_equal(got_img, g[f"image_{seed}"]), int(seed)
        assert np.array_equal(got_lab, g[f"label_{seed}"]), int(seed)
    assert fired >= 3


@pytest.mark.parametrize("shape", [(2, 5, 7, 9), (1, 3, 2, 261)])
def test_noise_matches_the_stream(dev, shape):
    image, label = _volume(shape)
    C = shape[0]
    p = AugmentParams(flip=(True, False, True), k=1, scale=[0.95] * C, shift=[0.02] * C, noise=True,
                      noise_key=0x9E3779B97F4A7C15)
    got, got_lab = _run(dev, image, label, p)
    ref, ref_lab = apply_params(image, label, p)
    clean = apply_params(image, label, p, noise=False)[0]
    err = np.abs(got - ref).max()
    print(f"noise {shape}: max |got - ref| = {err:.3e}, noise sd in the output = {(got - clean).std():.4f}")
    assert got.shape == ref.shape and err <= 1e-6 * max(1.0, np.abs(ref).max())
    assert np.array_equal(got_lab, ref_lab)
    assert 0.04 < (got - clean).std() < 0.06             # it is noise of sd 0.05, not zeros
    again, _ = _run(dev, image, label, p)
    assert _bits_equal(got, again)


def test_argument_checks(dev):
    aug = DeviceAugment()
    with pytest.raises(MmsegError):                      # C = 5 > 4 channels
        aug.apply({"image": torch.zeros(5, 4, 4, 8, device=dev)}, AugmentParams())
    with pytest.raises(MmsegError):                      # rot_k outside 0..3
        aug.apply({"image": torch.zeros(2, 4, 4, 8, device=dev)}, AugmentParams(k=4))
    with pytest.raises(MmsegError):                      # int32 labels have no kernel
        aug.apply({"image": torch.zeros(2, 4, 4, 8, device=dev),
                   "label": torch.zeros(4, 4, 8, dtype=torch.int32, device=dev)}, AugmentParams())
    with pytest.raises(RuntimeError, match="no CPU path"):
        aug.apply({"image": torch.zeros(2, 4, 4, 8)}, AugmentParams())


def _loader_cfg(mods=("CT", "PET"), augment=True):
    cfg = {"data": {"modalities": list(mods), "synthetic": {"n_train": 4, "n_val": 2, "size": 16, "device": True}},
           "model": {"out_channels": 3}, "training": {"batch_size": 2}, "hardware": {}}
    if augment:
        cfg["data"]["augmentation"] = dict(AUG)
    return cfg


def _epoch(loader):
    return [(b["image"].clone(), b["label"].clone()) for b in loader]


def test_loader_augments_training_only(dev):
    plain = _epoch(get_dataloader(_loader_cfg(augment=False), "train", shuffle=False))
    a, b = (get_dataloader(_loader_cfg(), "train", shuffle=False) for _ in range(2))
    first = _epoch(a)
    assert len(first) == len(plain) == 2
    for (xi, yi), (xp, yp) in zip(first, plain):
        assert xi.shape == xp.shape and xi.dtype == xp.dtype and xi.device == xp.device
        assert yi.shape == yp.shape and yi.dtype == yp.dtype
    assert any(not torch.equal(xi, xp) for (xi, _), (xp, _) in zip(first, plain))
    # same seed -> the same first epoch; the second epoch draws again
    assert all(torch.equal(x1, x2) and torch.equal(y1, y2) for (x1, y1), (x2, y2) in zip(first, _epoch(b)))
    second = _epoch(a)
    assert any(not torch.equal(x1, x2) for (x1, _), (x2, _) in zip(first, second))
    # validation is never augmented
    val_aug, val_plain = _epoch(get_dataloader(_loader_cfg(), "val")), _epoch(get_dataloader(_loader_cfg(augment=False), "val"))
    assert all(torch.equal(x1, x2) and torch.equal(y1, y2) for (x1, y1), (x2, y2) in zip(val_aug, val_plain))


def test_training_steps_on_augmented_batches(dev):
    """Two Trainer.train_step calls on a tiny UNet3D (16^3, 3 modalities) fed by the augmenting loader.
    Features 8..128: the engine's convolutions take channel counts that are multiples of 8 only
    (engine/layers.py), so this is the smallest five-level UNet it builds."""
    from bench import make_config
    from mmseg_amd.models.build import build_model
    from mmseg_amd.trainer.trainer import Trainer
    mods = ("CT", "PET", "MRI")
    cfg = make_config("unet", 2, "bf16", out_channels=3, modalities=mods, size=16)
    cfg["model"]["backbone"]["features"] = [8, 16, 32, 64, 128]
    cfg["data"].update(copy.deepcopy(_loader_cfg(mods)["data"]))
    torch.manual_seed(0)
    tr = Trainer(cfg, build_model(cfg))
    losses = [tr.train_step(batch, i) for i, batch in enumerate(get_dataloader(cfg, "train"))]
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses)
