"""Generate tests/golden/metrics_boundary.npz by running the REFERENCE's HausdorffDistance and ConfusionMatrix
(wittyseok/multimodal-organ-segmentation, src/trainer/metrics.py:91-226) on the CPU.

Run once where the reference is checked out and scipy is installed (neither travels to the GPU box):

    MMSEG_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py

Only data is written; no reference source is copied.  The reference is imported in place, with the same
two-class `nibabel` stub as make_golden.py.

Hausdorff cases (`hd_cases` lists their names).  A case is one HausdorffDistance(percentile) instance, `nupd`
update calls and one compute():
    <case>.q, <case>.nupd, <case>.int64 (feed the masks as int64 rather than uint8),
    <case>.pred<u>, <case>.target<u> (uint8 [B, H, W, D]), <case>.spacing<u> (3 fp64; all zero = spacing omitted),
    <case>.distances (the instance's per-sample list), <case>.hd, <case>.hd_std (NaN = key absent).
Confusion cases (`cm_cases`): <case>.C, <case>.pred, <case>.target, <case>.matrix and every compute() value.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("MMSEG_REFERENCE")      # the reference checkout (read-only is enough)
OUT = os.path.dirname(os.path.abspath(__file__))
SPACINGS = {"unit": None, "a": (1.5, 1.5, 2.0), "b": (0.7, 1.3, 2.1)}


def _import_metrics():
    if not REF:
        raise SystemExit("set MMSEG_REFERENCE to the reference checkout")
    sys.dont_write_bytecode = True
    if "nibabel" not in sys.modules:
        nib = types.ModuleType("nibabel")
        nib.Nifti1Header = type("Nifti1Header", (), {})
        nib.Nifti1Image = type("Nifti1Image", (), {})
        sys.modules["nibabel"] = nib
    sys.path.insert(0, REF)
    import src.trainer.metrics as metrics
    return metrics


def blobs(rng, shape, nblob=3, speckle=0.01):
    """Random ellipsoids labelled 1..nblob plus `speckle` of the voxels redrawn from 0..nblob."""
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).astype(np.float64)
    m = np.zeros(shape, dtype=np.uint8)
    for k in range(nblob):
        c = rng.uniform(0.2, 0.8, 3) * np.array(shape)
        r = rng.uniform(0.15, 0.35, 3) * np.array(shape) + 1.0
        m[(((grid - c) / r) ** 2).sum(-1) <= 1.0] = k + 1
    flip = rng.random(shape) < speckle
    m[flip] = rng.integers(0, nblob + 1, size=int(flip.sum()), dtype=np.uint8)
    return m


def pair(rng, B, shape):
    """pred / target [B, *shape]: the target, and a pred made of other blobs that overlap it."""
    t = np.stack([blobs(rng, shape) for _ in range(B)])
    p = np.stack([np.where(rng.random(shape) < 0.7, t[b], blobs(rng, shape)) for b in range(B)]).astype(np.uint8)
    return p, t


def hd_cases():
    rng = np.random.Generator(np.random.PCG64(20240917))
    cases = {}

    def add(name, updates, q=95, int64=False):
        cases[name] = dict(q=q, int64=int64, updates=updates)

    s1, s2 = (9, 11, 13), (5, 7, 130)
    p1, t1 = pair(rng, 2, s1)
    p2, t2 = pair(rng, 2, s2)
    for sn, sp in SPACINGS.items():
        add(f"blobs_9x11x13_{sn}", [(p1, t1, sp)], int64=(sn == "unit"))
        add(f"blobs_5x7x130_{sn}", [(p2, t2, sp)], int64=(sn == "a"))
    for q in (50, 100):
        add(f"blobs_9x11x13_q{q}", [(p1, t1, None)], q=q)
        add(f"blobs_5x7x130_q{q}_b", [(p2, t2, SPACINGS["b"])], q=q, int64=True)
    # targets touching the h = 0 face / the h = H - 1 face: the rolled border wraps round
    H, W, D = s1
    lo_t, hi_t, box_p = (np.zeros((1, H, W, D), dtype=np.uint8) for _ in range(3))
    lo_t[0, 0:3, 2:8, 3:9] = 1
    hi_t[0, H - 3:H, 2:8, 3:9] = 2
    box_p[0, 2:6, 3:9, 2:10] = 1
    for sn, sp in SPACINGS.items():
        add(f"wrap_h0_{sn}", [(box_p, lo_t, sp)])
        add(f"wrap_hlast_{sn}", [(box_p, hi_t, sp)], int64=True)
    # B = 3: pred empty in sample 0, target empty in sample 1, sample 2 normal -> exactly one distance
    p3 = np.concatenate([np.zeros((1, *s1), np.uint8), p1[:1], p1[1:]])
    t3 = np.concatenate([t1[:1], np.zeros((1, *s1), np.uint8), t1[1:]])
    for sn, sp in SPACINGS.items():
        add(f"one_of_three_{sn}", [(p3, t3, sp)])
    add("all_foreground_pred", [(np.full((1, *s1), 3, np.uint8), t1[:1], None)])
    add("all_foreground_pred_a", [(np.full((1, *s1), 1, np.uint8), t1[:1], SPACINGS["a"])], int64=True)
    add("all_skipped", [(p3[:2], t3[:2], None)])
    # two update calls (two shapes, two spacings) before one compute
    add("two_updates", [(p1, t1, None), (p2, t2, None)], int64=True)
    add("two_updates_ab", [(p1, t1, SPACINGS["a"]), (box_p, hi_t, SPACINGS["b"])])
    return cases


def main():
    metrics = _import_metrics()
    out = {}
    names = []
    for name, c in hd_cases().items():
        hd = metrics.HausdorffDistance(percentile=c["q"])
        for u, (p, t, sp) in enumerate(c["updates"]):
            hd.update(torch.from_numpy(p.astype(np.int64)), torch.from_numpy(t.astype(np.int64)), spacing=sp)
            out[f"{name}.pred{u}"], out[f"{name}.target{u}"] = p, t
            out[f"{name}.spacing{u}"] = np.zeros(3) if sp is None else np.asarray(sp, dtype=np.float64)
        res = hd.compute()
        out[f"{name}.q"] = np.float64(c["q"])
        out[f"{name}.nupd"] = np.int64(len(c["updates"]))
        out[f"{name}.int64"] = np.bool_(c["int64"])
        out[f"{name}.distances"] = np.asarray(hd.distances, dtype=np.float64)
        out[f"{name}.hd"] = np.float64(res["hausdorff_distance"])
        out[f"{name}.hd_std"] = np.float64(res.get("hausdorff_distance_std", np.nan))
        assert set(res) <= {"hausdorff_distance", "hausdorff_distance_std"}
        names.append(name)
        print(f"{name}: {len(hd.distances)} distance(s), {res}")
    out["hd_cases"] = np.array(names)

    rng = np.random.Generator(np.random.PCG64(7))
    cm_names = []
    for C in (3, 6, 16):
        name = f"cm_C{C}"
        t = rng.integers(0, C, size=(2, 9, 11, 13)).astype(np.uint8)
        p = np.where(rng.random(t.shape) < 0.6, t, rng.integers(0, C, size=t.shape)).astype(np.uint8)
        if C == 6:
            p[p == 4] = 0       # a class that is never predicted: a zero column (precision 0 / 1e-8)
        cm = metrics.ConfusionMatrix(num_classes=C)
        cm.update(torch.from_numpy(p.astype(np.int64)), torch.from_numpy(t.astype(np.int64)))
        res = cm.compute()
        out[f"{name}.C"], out[f"{name}.pred"], out[f"{name}.target"] = np.int64(C), p, t
        out[f"{name}.matrix"] = cm.matrix
        for k, v in res.items():
            out[f"{name}.{k}"] = np.asarray(v, dtype=np.int64 if k == "confusion_matrix" else np.float64)
        cm_names.append(name)
    out["cm_cases"] = np.array(cm_names)
    path = os.path.join(OUT, "metrics_boundary.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
