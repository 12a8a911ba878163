"""Boundary and confusion metrics on the GPU (csrc/metrics.hip through trainer/metrics.py): the distance transform
against the brute-force numpy checker (tests/metrics_ref.py), HausdorffDistance and ConfusionMatrix against the
reference's own output (tests/golden/metrics_boundary.npz), and the Trainer's training.metrics wiring.

Tolerances: exact equality at unit spacing (every candidate distance is an exactly representable integer before
the one sqrt).  At the anisotropic spacings relative 1e-12: two candidates that tie in exact arithmetic can differ
by a few ulp of fp64 (about 1e-15) depending on which offsets win; 1e-12 is that with three orders of margin."""
import functools

import numpy as np
import pytest
import torch

import mmseg_amd  # noqa: F401
from mmseg_amd._lib import MmsegError
from mmseg_amd.data.synthetic import phantom
from mmseg_amd.models.build import build_model
from mmseg_amd.trainer import (ConfusionMatrix, DiceMetric, HausdorffDistance, Trainer, distance_transform_edt,
                               get_metrics)
from tests import metrics_ref as R
from tests.helpers import golden

pytestmark = pytest.mark.gpu
SPACINGS = [None, (1.5, 1.5, 2.0), (0.7, 1.3, 2.1)]
ANISO_RTOL = 1e-12


def _same(got, want, exact):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    if exact:
        return np.array_equal(got.view(np.uint64), want.view(np.uint64))
    fin = np.isfinite(want)
    return np.array_equal(got[~fin], want[~fin]) and bool(np.all(np.abs(got[fin] - want[fin])
                                                                 <= ANISO_RTOL * np.abs(want[fin])))


# ------------------------------------------------------------------------------------------------ distance transform
@functools.lru_cache(maxsize=None)
def _edt_mask(kind):
    rng = np.random.Generator(np.random.PCG64(len(kind) + 17))
    shapes = {"odd": (9, 11, 13), "long_d": (5, 7, 130), "long_h": (70, 6, 5), "long_w": (6, 70, 5)}
    if kind in shapes:
        m = (rng.random((2, *shapes[kind])) < 0.03).astype(np.uint8) * 2     # sparse: most lines hold no foreground
        m[1] = rng.random(shapes[kind]) < 0.4
    elif kind == "single_voxel":
        m = np.zeros((1, 9, 11, 13), dtype=np.uint8)
        m[0, 6, 2, 11] = 1
    elif kind == "all_foreground":
        m = np.ones((1, 9, 11, 13), dtype=np.uint8)
    else:
        assert kind == "all_background"
        m = np.zeros((2, 9, 11, 13), dtype=np.uint8)
        m[1, 4, 5, 6] = 1                    # the sample next to the empty one must not leak into it
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _edt_ref(kind, spacing):
    m = _edt_mask(kind)
    out = np.stack([R.edt(m[b] > 0, spacing or (1.0, 1.0, 1.0)) for b in range(len(m))])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("spacing", SPACINGS, ids=["unit", "a", "b"])
@pytest.mark.parametrize("kind", ["odd", "long_d", "long_h", "long_w", "single_voxel", "all_foreground",
                                  "all_background"])
def test_edt_matches_brute_force(dev, kind, spacing):
    m = _edt_mask(kind)
    t = torch.from_numpy(np.array(m)).to(dev)
    if kind in ("odd", "long_h"):
        t = t.long()
    got = distance_transform_edt(t, spacing)
    assert got.dtype == torch.float64 and got.shape == t.shape
    got = got.cpu().numpy()
    want = _edt_ref(kind, spacing)
    if kind == "all_background":
        assert np.all(np.isinf(got[0]))
    if kind == "all_foreground":
        assert not got.any()
    assert _same(got, want, exact=spacing is None)


def test_edt_three_dim_mask_and_argument_checks(dev):
    m = _edt_mask("single_voxel")
    got = distance_transform_edt(torch.from_numpy(np.array(m[0])).to(dev)).cpu().numpy()
    assert _same(got, _edt_ref("single_voxel", None)[0], exact=True)
    with pytest.raises(ValueError):
        distance_transform_edt(torch.zeros(4, 4, dtype=torch.uint8, device=dev))
    with pytest.raises(MmsegError):
        distance_transform_edt(torch.zeros(1, 1, 1, 40000, dtype=torch.uint8, device=dev))


# ------------------------------------------------------------------------------------------------ Hausdorff distance
def _hd_case(g, name):
    ups = []
    for u in range(int(g[f"{name}.nupd"])):
        sp = g[f"{name}.spacing{u}"]
        ups.append((g[f"{name}.pred{u}"], g[f"{name}.target{u}"], tuple(float(x) for x in sp) if sp.any() else None))
    return ups, float(g[f"{name}.q"]), bool(g[f"{name}.int64"])


HD_CASES = [str(n) for n in golden("metrics_boundary")["hd_cases"]]


def test_hd_case_list_is_complete():
    """The cases the fixture must hold; none may go missing from the parametrisation below."""
    need = ["blobs_9x11x13_", "blobs_5x7x130_", "wrap_h0_", "wrap_hlast_", "one_of_three_", "all_foreground_pred",
            "all_skipped", "two_updates", "_q50", "_q100"]
    for frag in need:
        assert any(frag in n for n in HD_CASES), frag
    g = golden("metrics_boundary")
    assert any(bool(g[f"{n}.int64"]) for n in HD_CASES) and not all(bool(g[f"{n}.int64"]) for n in HD_CASES)
    assert max(int(g[f"{n}.pred0"].max()) for n in HD_CASES) > 1       # labels > 1 collapse by `> 0`
    assert len(g["one_of_three_unit.distances"]) == 1 and len(g["all_skipped.distances"]) == 0


@pytest.mark.parametrize("name", HD_CASES)
def test_hausdorff_matches_reference(dev, name):
    g = golden("metrics_boundary")
    ups, q, as_int64 = _hd_case(g, name)
    exact = all(sp is None for _, _, sp in ups)
    hd = HausdorffDistance(percentile=q)
    for p, t, sp in ups:
        pt, tt = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
        if as_int64:
            pt, tt = pt.long(), tt.long()
        if sp is None:
            hd.update(pt, tt)
        else:
            hd.update(pt, tt, spacing=sp)
    res = hd.compute()
    want = g[f"{name}.distances"]
    print(f"\n{name}: distances {[float(d) for d in hd.distances]} vs {want.tolist()}; {res}")
    assert _same(hd.distances, want, exact)
    if len(want) == 0:
        assert res == {"hausdorff_distance": float("inf")}
        return
    assert set(res) == {"hausdorff_distance", "hausdorff_distance_std"}
    assert _same(res["hausdorff_distance"], g[f"{name}.hd"], exact)
    if exact:
        assert _same(res["hausdorff_distance_std"], g[f"{name}.hd_std"], True)
    else:   # a std of values each within rtol of the reference's: absolute bound rtol * the largest distance
        assert abs(res["hausdorff_distance_std"] - float(g[f"{name}.hd_std"])) <= ANISO_RTOL * float(np.max(want))
    assert hd.compute() == res                 # compute() drains once; a second call sees the same list
    hd.reset()
    assert hd.compute() == {"hausdorff_distance": float("inf")}


def test_hausdorff_mixed_dtypes_and_shape_checks(dev):
    g = golden("metrics_boundary")
    (p, t, _), = _hd_case(g, "blobs_9x11x13_unit")[0]
    hd = HausdorffDistance()
    hd.update(torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev).long())      # uint8 pred, int64 target
    hd.update(torch.from_numpy(p).to(dev).int(), torch.from_numpy(t).to(dev))       # int32 is widened
    want = g["blobs_9x11x13_unit.distances"]
    hd.compute()
    assert _same(hd.distances, np.concatenate([want, want]), True)
    with pytest.raises(ValueError):
        hd.update(torch.zeros(3, 3, 3, dtype=torch.uint8, device=dev), torch.zeros(3, 3, 3, dtype=torch.uint8,
                                                                                   device=dev))


# ------------------------------------------------------------------------------------------------ confusion matrix
@pytest.mark.parametrize("C", [3, 6, 16])
def test_confusion_matches_reference(dev, C):
    g = golden("metrics_boundary")
    name = f"cm_C{C}"
    p, t = g[f"{name}.pred"], g[f"{name}.target"]
    assert p.shape == (2, 9, 11, 13)
    cm = ConfusionMatrix(num_classes=C)
    cm.update(torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev).long())
    assert cm.matrix.dtype == np.int64 and np.array_equal(cm.matrix, R.confusion(p, t, C))
    assert np.array_equal(cm.matrix, g[f"{name}.matrix"]) and cm.invalid == 0
    res = cm.compute()
    assert set(res) == {"accuracy", "precision", "recall", "f1", "precision_per_class", "recall_per_class",
                        "f1_per_class", "confusion_matrix"}
    for k, v in res.items():
        want = g[f"{name}.{k}"]
        got = np.asarray(v, dtype=want.dtype)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), k
    cm.update(torch.from_numpy(p).to(dev).long(), torch.from_numpy(t).to(dev))      # accumulates over updates
    assert np.array_equal(cm.matrix, 2 * g[f"{name}.matrix"])
    cm.reset()
    assert not cm.matrix.any()


@pytest.mark.parametrize("label_dtype", [torch.int64, torch.uint8])
def test_confusion_from_logits_equals_update_of_argmax(dev, label_dtype):
    C = 6
    gen = torch.Generator().manual_seed(3)
    logits = torch.randn(2, C, 9, 11, 13, generator=gen)
    logits[0, 2, 1, 2, 3] = logits[0, 4, 1, 2, 3] = logits[0].max() + 1.0      # a tie: the first maximum wins
    logits[1, 3, 4, 5, 6] = float("nan")                                       # NaN counts as maximal
    target = torch.randint(0, C, (2, 9, 11, 13), generator=gen).to(label_dtype)
    pred = logits.argmax(1)
    assert pred[0, 1, 2, 3] == 2 and pred[1, 4, 5, 6] == 3
    a, b = ConfusionMatrix(C), ConfusionMatrix(C)
    a.update_from_logits(logits.to(dev), target.to(dev))
    b.update(pred.to(dev), target.to(dev))
    assert np.array_equal(a.matrix, b.matrix) and a.matrix.sum() == target.numel()
    assert np.array_equal(a.matrix, R.confusion(pred.numpy(), target.numpy(), C))
    assert a.compute() == b.compute()


def test_confusion_out_of_range_goes_to_invalid_only(dev):
    C = 3
    rng = np.random.Generator(np.random.PCG64(9))
    t = rng.integers(0, C, size=(2, 9, 11, 13))
    p = rng.integers(0, C, size=t.shape)
    clean = R.confusion(p, t, C)
    bad_t, bad_p = t.copy(), p.copy()
    bad_t[0, 0, 0, 0], bad_t[1, 8, 10, 12], bad_p[0, 3, 3, 3] = C, -1, 200
    keep = np.ones(t.shape, dtype=bool)
    keep[0, 0, 0, 0] = keep[1, 8, 10, 12] = keep[0, 3, 3, 3] = False
    cm = ConfusionMatrix(C)
    cm.update(torch.from_numpy(bad_p).to(dev), torch.from_numpy(bad_t).to(dev))
    assert cm.invalid == 3
    assert np.array_equal(cm.matrix, R.confusion(p[keep], t[keep], C)) and cm.matrix.sum() == clean.sum() - 3
    with pytest.raises(IndexError):
        cm.compute()
    lg = ConfusionMatrix(C)
    lg.update_from_logits(torch.randn(2, C, 9, 11, 13).to(dev), torch.from_numpy(bad_t).to(dev))
    assert lg.invalid == 2 and lg.matrix.sum() == t.size - 2
    with pytest.raises(MmsegError):
        ConfusionMatrix(17).update(torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev))


# ------------------------------------------------------------------------------------------------ Trainer
def _cfg(metrics=None):
    cfg = {
        "experiment": {"name": "metrics", "output_dir": "/tmp/mmseg_metrics", "seed": 42},
        "data": {"modalities": ["CT", "PET"]},
        "model": {"name": "unet", "in_channels": 2, "out_channels": 3,
                  "backbone": {"features": [8, 16, 32, 64, 128], "norm": "instance"}, "head": {"dropout": 0.0}},
        "training": {"epochs": 1, "batch_size": 1, "accumulation_steps": 1,
                     "optimizer": {"name": "adamw", "lr": 1e-3, "weight_decay": 1e-5, "betas": [0.9, 0.999]},
                     "scheduler": {"name": "none"},
                     "loss": {"name": "dice_ce", "dice_weight": 0.5, "ce_weight": 0.5, "class_weights": None},
                     "checkpoint": {"save_last": False, "save_best": False}},
        "hardware": {"device": "cuda", "mixed_precision": False, "engine_dtype": "float32"},
    }
    if metrics is not None:
        cfg["training"]["metrics"] = metrics
    return cfg


def _batch(seed, S=32):
    p = phantom(int(seed), S, 3, ["CT", "PET"])
    return {"image": torch.from_numpy(np.stack([p["CT"], p["PET"]]))[None], "label": torch.from_numpy(p["label"])[None]}


@functools.lru_cache(maxsize=None)
def _trained():
    """One Trainer over the tiny UNet after a few steps (so that the argmax is not one class everywhere), and its
    two validation batches."""
    torch.manual_seed(42)
    model = build_model(_cfg())
    val = [_batch(101), _batch(102)]
    tr = Trainer(_cfg(), model, val_loader=val)
    model.train()
    for i, s in enumerate((1, 2, 3, 4)):
        tr.train_step(_batch(s), i)
    return tr, model, val


def _evaluate(tr, metrics):
    tr.config["training"].pop("metrics", None)
    if metrics is not None:
        tr.config["training"]["metrics"] = metrics
    return tr.evaluate()


def test_trainer_validation_metrics(dev):
    tr, model, val = _trained()

    def evaluate(metrics):
        return _evaluate(tr, metrics)

    res_plain = evaluate(None)
    assert set(res_plain) == {"dice", "dice_per_class"}
    assert evaluate(["dice"]) == res_plain
    # the Dice path as it was: DiceMetric.update_from_logits on each batch's logits
    dm, hd, cm = DiceMetric(num_classes=3), HausdorffDistance(95), ConfusionMatrix(3)
    model.eval()
    with torch.no_grad():
        for b in val:
            out = model(b["image"].to(dev))
            dm.update_from_logits(out, b["label"].to(dev))
            pred = out.argmax(1)
            hd.update(pred, b["label"].to(dev))
            cm.update(pred, b["label"].to(dev))
    assert res_plain == dm.compute()
    full = evaluate(["dice", "hd95", "confusion"])
    want = {**dm.compute(), **hd.compute(), **cm.compute()}
    print(f"\nvalidation metrics: { {k: v for k, v in full.items() if k != 'confusion_matrix'} }")
    assert set(full) == set(want) and {"hausdorff_distance", "accuracy", "confusion_matrix"} <= set(full)
    for k in want:
        assert np.array_equal(np.asarray(full[k]), np.asarray(want[k])), k
    assert np.asarray(full["confusion_matrix"]).sum() == 2 * 32 ** 3
    only_hd = evaluate(["hd95"])
    assert set(only_hd) == set(dm.compute()) | set(hd.compute()) and only_hd["dice"] == res_plain["dice"]
    with pytest.raises(ValueError):
        evaluate(["dice", "hd96"])
    assert evaluate(None) == res_plain
    assert set(get_metrics(_cfg())) == {"dice", "confusion"}


def test_trainer_metrics_data_parallel_merge(dev, monkeypatch):
    """_validate's all-reduces with two ranks that saw the same batches (the all-reduce is replaced by a doubling):
    the int64 matrix doubles exactly, and HD95 from the summed [count, sum, sum of squares] has the single-rank mean
    and std to rounding."""
    from mmseg_amd.distributed import ddp
    tr, _, _ = _trained()
    single = _evaluate(tr, ["dice", "hd95", "confusion"])
    monkeypatch.setattr(ddp, "allreduce_sum_", lambda t: t.mul_(2))
    monkeypatch.setattr(tr, "world", 2)
    both = _evaluate(tr, ["dice", "hd95", "confusion"])
    assert np.array_equal(np.asarray(both["confusion_matrix"]), 2 * np.asarray(single["confusion_matrix"]))
    assert np.asarray(both["confusion_matrix"]).dtype == np.int64
    assert abs(both["hausdorff_distance"] - single["hausdorff_distance"]) <= 1e-12 * single["hausdorff_distance"]
    # sqrt(sum d^2 / n - mean^2): the subtraction cancels a few ulp of d^2, and the sqrt divides that by 2 std
    m, sd = float(single["hausdorff_distance"]), float(single["hausdorff_distance_std"])
    bound = 16 * np.finfo(np.float64).eps * (m + 3 * sd) ** 2 / (2 * max(sd, 1e-6))
    assert abs(both["hausdorff_distance_std"] - sd) <= bound
    assert abs(both["dice"] - single["dice"]) < 1e-6 and set(both) == set(single)
