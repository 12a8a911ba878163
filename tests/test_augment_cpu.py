"""Host side of the device augmentation (data/augment.py), no GPU: draw_augment_params consumes a
random.Random exactly as the reference's train pipeline consumes `random` (transforms.py:428-443), pinned by
tests/golden/augment.npz -- the reference's own RandomFlip / RandomRotate90 / RandomIntensityShift output per
seed, reproduced bit for bit by the drawn parameters through the numpy restatement (tests/augment_ref.py);
sample_rng keys the draws on (seed, epoch, global index); the host loader refuses to train un-augmented."""
import random

import numpy as np
import pytest

import mmseg_amd  # noqa: F401
from mmseg_amd.data import AugmentParams, draw_augment_params, get_dataloader, sample_rng
from tests.augment_ref import apply_params
from tests.helpers import golden

G = golden("augment")
CFG = {"enabled": True, "random_flip": True, "random_rotate": 15, "random_intensity": float(G["random_intensity"])}


@pytest.mark.parametrize("seed", [int(s) for s in G["seeds"]])
def test_draws_reproduce_the_reference(seed):
    p = draw_augment_params(random.Random(seed), CFG, 2)
    img, lab = apply_params(G["image_in"], G["label_in"], p, noise=False)
    ref_img, ref_lab = G[f"image_{seed}"], G[f"label_{seed}"]
    assert img.shape == ref_img.shape and lab.shape == ref_lab.shape
    assert np.array_equal(img.view(np.uint32), ref_img.view(np.uint32))
    assert np.array_equal(lab, ref_lab)
    assert p.noise == bool(G["noise_fired"][list(G["seeds"]).index(seed)])
    assert (p.noise_key != 0) == p.noise


def test_draw_order_with_transforms_switched_off():
    """A transform the config leaves out draws nothing (get_transforms does not build it)."""
    rng = random.Random(5)
    p = draw_augment_params(rng, {"random_flip": False}, 3)
    assert tuple(p.flip) == (False, False, False) and p.k == 0 and p.scale is None
    ref = random.Random(5)
    noise = ref.random() < 0.2                  # the only draw left: RandomGaussianNoise's
    assert p.noise == noise
    if noise:
        ref.getrandbits(64)
    assert rng.random() == ref.random()


def _as_tuple(p: AugmentParams):
    return (tuple(p.flip), p.k, None if p.scale is None else tuple(p.scale),
            None if p.shift is None else tuple(p.shift), p.noise, p.noise_key)


def test_sample_rng_keys_on_seed_epoch_index():
    draw = lambda s, e, i: [_as_tuple(draw_augment_params(sample_rng(s, e, i), CFG, 2))]  # noqa: E731
    many = lambda s, e, i: [r.random() for r in [sample_rng(s, e, i)] for _ in range(6)]  # noqa: E731
    assert draw(7, 3, 11) == draw(7, 3, 11) and many(7, 3, 11) == many(7, 3, 11)
    assert many(7, 3, 11) != many(7, 4, 11)
    assert many(7, 3, 11) != many(7, 3, 12)
    assert many(7, 3, 11) != many(8, 3, 11)
    assert many(7, 3, 11) != many(7, 11, 3)


def test_host_loader_refuses_augmentation():
    cfg = {"data": {"modalities": ["CT", "PET"], "synthetic": {"n_train": 4, "size": 16},
                    "augmentation": dict(CFG)},
           "model": {"out_channels": 3}, "training": {"batch_size": 2}, "hardware": {}}
    with pytest.raises(NotImplementedError, match="data.synthetic.device: true"):
        get_dataloader(cfg, "train")
    get_dataloader(cfg, "val")                  # validation is never augmented
    cfg["data"]["augmentation"]["enabled"] = False
    get_dataloader(cfg, "train")
