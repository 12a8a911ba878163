"""Generate tests/golden/patch.npz by running the REFERENCE's RandomCrop and CenterCrop
(wittyseok/multimodal-organ-segmentation, src/data/transforms.py:142-212) on the CPU.

Run once where the reference is checked out (the reference never travels to the GPU box):

    MMSEG_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_patch.py

Only data is written (the inputs, and per seed and crop size the cropped image / label and the draws the
crop consumed); no reference source is copied.  The reference is imported in place, with the same two-class
`nibabel` stub as make_golden.py.

Per seed and size: random.seed(seed), one random.random() (the mode draw that mmseg_amd.data.patch.
draw_patch_params makes before the crop's draws), then RandomCrop(size) on a [2, 13, 11, 18] float32 volume
with an int64 label.  CenterCrop(size) once per size.  A second volume [2, 5, 9, 20], smaller than the
(8, 8, 16) crop along its first axis, records what the reference's slices give there (a [2, 5, 8, 16] crop:
the interior of the padded patch).
"""
from __future__ import annotations

import os
import random
import sys
import types

import numpy as np

REF = os.environ.get("MMSEG_REFERENCE")      # the reference checkout (read-only is enough)
OUT = os.path.dirname(os.path.abspath(__file__))
SEEDS = (0, 1, 2, 3, 4, 5)
SHAPE, SMALL = (2, 13, 11, 18), (2, 5, 9, 20)
SIZES = ((8, 8, 16), (6, 5, 7))


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
            self.calls.append((name, a, v))
            return v
        return call


def main():
    if not REF:
        sys.exit("set MMSEG_REFERENCE to the reference checkout")
    T = _import_transforms()
    rec = T.random = _Recorder()
    rng = np.random.Generator(np.random.PCG64(2025))
    out = {"seeds": np.array(SEEDS, dtype=np.int64), "sizes": np.array(SIZES, dtype=np.int64)}
    vols = {}
    for name, shape in (("a", SHAPE), ("b", SMALL)):
        image = rng.standard_normal(shape, dtype=np.float32)
        label = rng.integers(0, 4, size=shape[1:]).astype(np.int64)
        vols[name] = (image, label)
        out[f"image_{name}"], out[f"label_{name}"] = image, label
    for si, size in enumerate(SIZES):
        image, label = vols["a"]
        s = T.CenterCrop(size)({"image": image.copy(), "label": label.copy()})
        out[f"center_image_{si}"], out[f"center_label_{si}"] = s["image"], s["label"]
        for seed in SEEDS:
            rec.calls.clear()
            random.seed(seed)
            random.random()
            s = T.RandomCrop(size)({"image": image.copy(), "label": label.copy()})
            assert [c[0] for c in rec.calls] == ["randint"] * 3, rec.calls
            assert [c[1] for c in rec.calls] == [(0, image.shape[1 + a] - size[a]) for a in range(3)]
            draws = [c[2] for c in rec.calls]
            assert s["image"].shape == (2,) + tuple(size) and s["image"].dtype == np.float32
            assert s["label"].dtype == np.int64
            out[f"crop_image_{si}_{seed}"], out[f"crop_label_{si}_{seed}"] = s["image"], s["label"]
            out[f"draws_{si}_{seed}"] = np.array(draws, dtype=np.int64)
    # the volume smaller than the crop along axis 0: no draw for that axis, the slice keeps all 5 planes
    image, label = vols["b"]
    for seed in SEEDS[:2]:
        rec.calls.clear()
        random.seed(seed)
        random.random()
        s = T.RandomCrop(SIZES[0])({"image": image.copy(), "label": label.copy()})
        assert [c[1] for c in rec.calls] == [(0, 1), (0, 4)], rec.calls
        assert s["image"].shape == (2, 5, 8, 16)
        out[f"small_image_{seed}"], out[f"small_label_{seed}"] = s["image"], s["label"]
        out[f"small_draws_{seed}"] = np.array([c[2] for c in rec.calls], dtype=np.int64)
    s = T.CenterCrop(SIZES[0])({"image": image.copy(), "label": label.copy()})
    out["small_center_image"], out["small_center_label"] = s["image"], s["label"]
    np.savez_compressed(os.path.join(OUT, "patch.npz"), **out)
    print("patch done: seeds", len(SEEDS), "sizes", SIZES, "bytes", os.path.getsize(os.path.join(OUT, "patch.npz")))


if __name__ == "__main__":
    main()
