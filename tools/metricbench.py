"""Time the validation metrics next to the validation forward they follow (config c3: DualEncoder, CT + PET,
2 x 96^3, bf16):

    python tools/metricbench.py [--iters 25] [--size 96] [--out FILE.json]

One HausdorffDistance.update, one ConfusionMatrix.update_from_logits, one DiceMetric.update_from_logits and one
model forward (eval, no_grad) per iteration, each between its own pair of HIP events, after --warmup untimed
iterations; the median over --iters (at least 20) is reported, with min and max.  The masks are a phantom's
labels against the same labels rolled by (2, 1, 3) voxels with 1 % speckle, so the borders are those of real
organs plus outliers.  "hd_kernels_us" is one update's launches summed per kernel from the library's launch
timing (mmseg_timing_*): which pass the time goes to.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cfg():
    return {"data": {"modalities": ["CT", "PET"]},
            "model": {"name": "dual_encoder", "out_channels": 6,
                      "backbone": {"features": [32, 64, 128, 256, 512], "norm": "instance"},
                      "fusion": {"type": "cross_attention"}, "head": {"dropout": 0.0}},
            "training": {"loss": {"name": "dice_ce"}},
            "hardware": {"device": "cuda", "mixed_precision": True, "engine_dtype": "bfloat16"}}


def _timed(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--out", help="also write the result line here")
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters: at least 20 timed iterations")
    import numpy as np
    import torch
    import mmseg_amd  # noqa: F401
    from mmseg_amd._lib import lib
    from mmseg_amd.data.synthetic import phantom
    from mmseg_amd.models.build import build_model
    from mmseg_amd.trainer.metrics import ConfusionMatrix, DiceMetric, HausdorffDistance

    dev = torch.device("cuda", 0)
    S, C = a.size, 6
    ph = [phantom(seed, S, C, ["CT", "PET"]) for seed in (11, 12)]
    target = torch.from_numpy(np.stack([p["label"] for p in ph])).to(dev)
    image = torch.from_numpy(np.stack([np.stack([p["CT"], p["PET"]]) for p in ph])).to(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    pred = torch.roll(target, (2, 1, 3), (1, 2, 3))
    speck = torch.rand(pred.shape, device=dev, generator=gen) < 0.01
    pred = torch.where(speck, torch.randint(0, C, pred.shape, device=dev, generator=gen), pred)
    logits = torch.randn(2, C, S, S, S, device=dev, generator=gen)
    logits.scatter_add_(1, pred[:, None], torch.full((2, 1, S, S, S), 4.0, device=dev))
    torch.manual_seed(0)
    model = build_model(_cfg()).to(dev).eval()

    hd, cm, dm = HausdorffDistance(95), ConfusionMatrix(C), DiceMetric(C, device=dev)

    def forward():
        with torch.no_grad():
            model(image)

    res = {"shape": [2, S, S, S], "iters": a.iters, "warmup": a.warmup,
           "forward_c3": _timed(forward, a.iters, a.warmup),
           "hd_update": _timed(lambda: hd.update(pred, target), a.iters, a.warmup),
           "confusion_update_from_logits": _timed(lambda: cm.update_from_logits(logits, target), a.iters, a.warmup),
           "dice_update_from_logits": _timed(lambda: dm.update_from_logits(logits, target), a.iters, a.warmup)}
    out = hd.compute()
    res["hd95"] = float(out["hausdorff_distance"])
    res["border_voxels"] = [int(r[0]) for r in _last_records(hd, pred, target)]
    L = lib()
    L.mmseg_timing_begin()
    hd.update(pred, target)
    torch.cuda.synchronize()
    L.mmseg_timing_end()
    ms, nm = ctypes.c_float(), ctypes.c_char_p()
    per = {}
    for i in range(L.mmseg_timing_count()):
        L.mmseg_timing_get(i, ctypes.addressof(ms), ctypes.addressof(nm))
        name = nm.value.decode()
        per[name] = round(per.get(name, 0.0) + ms.value * 1e3, 1)
    res["hd_kernels_us"] = per
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def _last_records(hd, pred, target):
    hd.reset()
    hd.update(pred, target)
    return hd._pending[-1].cpu().numpy()


if __name__ == "__main__":
    main()
