"""Generate tests/golden/augment.npz by running the REFERENCE's augmentation transforms
(wittyseok/multimodal-organ-segmentation, src/data/transforms.py:32-139) on the CPU, composed as
get_transforms composes them for training (transforms.py:428-443).

Run once where the reference is checked out (the reference never travels to the GPU box):

    MMSEG_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_augment.py

Only data is written (the input, and per seed the expected image / label and whether the noise fired); no
reference source is copied.  The reference is imported in place, with the same two-class `nibabel` stub as
make_golden.py (the package's trainer imports ask for it; no NIfTI I/O happens).

Per seed: random.seed(seed), then RandomFlip(0.5), RandomRotate90(0.5), RandomIntensityShift((-0.1, 0.1), 0.3)
on a [2, 5, 7, 9] float32 volume with an int64 label; image and label are stored at that point.  Then
RandomGaussianNoise(std=0.05, prob=0.2) runs and only "did the image change" is stored: its values come from
numpy's global state, which the device pass does not reproduce.
"""
from __future__ import annotations

import os
import random
import sys
import types

import numpy as np

REF = os.environ.get("MMSEG_REFERENCE")      # the reference checkout (read-only is enough)
OUT = os.path.dirname(os.path.abspath(__file__))
SEEDS = range(32)
SHAPE = (2, 5, 7, 9)
INTENSITY = 0.1


def _import_transforms():
    sys.dont_write_bytecode = True
    if "nibabel" not in sys.modules:
        nib = types.ModuleType("nibabel")
        nib.Nifti1Header = type("Nifti1Header", (), {})
        nib.Nifti1Image = type("Nifti1Image", (), {})
        sys.modules["nibabel"] = nib
    sys.path.insert(0, REF)
    import src.data.transforms as T  # noqa: E402
    return T


class _Recorder:
    """Stands in for the `random` module inside the reference's transforms: same draws, recorded."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(random, name)

        def call(*a):
            v = fn(*a)
            self.calls.append((name, v))
            return v
        return call


def main():
    if not REF:
        sys.exit("set MMSEG_REFERENCE to the reference checkout")
    T = _import_transforms()
    rec = T.random = _Recorder()
    rng = np.random.Generator(np.random.PCG64(2024))
    image = rng.standard_normal(SHAPE, dtype=np.float32)
    label = rng.integers(0, 6, size=SHAPE[1:]).astype(np.int64)
    geo = [T.RandomFlip(prob=0.5), T.RandomRotate90(prob=0.5)]
    inten = T.RandomIntensityShift(shift_range=(-INTENSITY, INTENSITY), prob=0.3)
    noise = T.RandomGaussianNoise(std=0.05, prob=0.2)
    out = {"image_in": image, "label_in": label, "seeds": np.array(list(SEEDS), dtype=np.int64),
           "random_intensity": np.float64(INTENSITY)}
    ks, flips, n_int, fired = set(), np.zeros(3, dtype=bool), 0, []
    for seed in SEEDS:
        rec.calls.clear()
        random.seed(seed)
        np.random.seed(seed)     # only the noise values depend on it, and they are not stored
        s = {"image": image.copy(), "label": label.copy()}
        for t in geo:
            s = t(s)
        g_img = s["image"].copy()
        s = inten(s)
        img, lab = s["image"].copy(), s["label"].copy()
        assert img.dtype == np.float32 and lab.dtype == np.int64
        s = noise(s)
        fired.append(not np.array_equal(s["image"], img))
        out[f"image_{seed}"], out[f"label_{seed}"] = img, lab
        # coverage bookkeeping from the recorded draws (RandomFlip draws first, once per axis; the only randint
        # is the rotation count), checked against the label the reference produced
        m = [v < 0.5 for _, v in rec.calls[:3]]
        k = next((v for n, v in rec.calls if n == "randint"), 0)
        ref = label
        for ax in range(3):
            if m[ax]:
                ref = np.flip(ref, axis=ax)
        assert np.array_equal(np.rot90(ref, k=k, axes=(0, 1)), lab), seed
        ks.add(k)
        flips |= np.array(m, dtype=bool)
        n_int += int(not np.array_equal(g_img, img))
    out["noise_fired"] = np.array(fired, dtype=bool)
    assert ks == {0, 1, 2, 3}, ks
    assert flips.all(), flips
    assert n_int >= 3, n_int
    assert sum(fired) >= 2, sum(fired)
    np.savez_compressed(os.path.join(OUT, "augment.npz"), **out)
    print("augment done: seeds", len(SEEDS), "rotations", sorted(ks), "intensity fired", n_int, "noise fired",
          sum(fired))


if __name__ == "__main__":
    main()
