#!/usr/bin/env python3
"""Sliding-window blending at C = 6, roi 96^3, sw_batch 4 on a 512 x 512 x 256 volume: the batched
mmseg_window_blend (constant and Gaussian) against the compulsory bytes (read nb * C * roi predictions; read and
write each covered out and count voxel once), next to the four per-window mmseg_window_accum launches it stands
in for and a torch.Tensor.copy_ for scale; the fused mmseg_blend_argmax_encode against mmseg_window_finish +
mmseg_argmax_encode; and end-to-end prediction (windows, model, blend, mask) of one synthetic 256 x 256 x 128
case with the c6 UNet for constant blending, Gaussian, and Gaussian with 8 flips.  5 warm-ups, HIP events
around each launch, median of --reps.  Needs an MI355X.

    python tools/swbench.py [--out profiles/sw_blend_bench.json]      (DESIGN.md "Sliding-window inference")
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmseg_amd  # noqa: E402,F401
from bench import make_config  # noqa: E402
from mmseg_amd._lib import lib, ptr, stream_handle  # noqa: E402
from mmseg_amd.data.nifti import argmax_encode  # noqa: E402
from mmseg_amd.inference import (blend_argmax_encode, gaussian_tables, sliding_window_accumulate,  # noqa: E402
                                 sliding_window_inference)
from mmseg_amd.inference.sliding_window import _windows  # noqa: E402
from mmseg_amd.models.build import build_model  # noqa: E402


def timed(fn, warm, reps, flush=None):
    """flush: a buffer larger than the 256 MiB Infinity Cache, rewritten before each timed launch (cold operands)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        if flush is not None:
            flush.fill_(1.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}


def rate(r, nbytes):
    r["bytes"] = int(nbytes)
    r["GBps"] = nbytes / r["ms_median"] / 1e6
    return r


def bench_kernels(args, res):
    (D, H, W), C, roi, nb = args.shape, args.classes, [args.roi] * 3, args.sw_batch
    dev = torch.device("cuda", 0)
    L, s = lib(), stream_handle()
    rv = roi[0] * roi[1] * roi[2]
    _, wins = _windows(1, (D, H, W), roi, 0.5)
    wins = wins[:nb]                                   # the first predictor batch: neighbours along W, half overlapping
    win_host = torch.tensor(wins, dtype=torch.int32).reshape(-1)
    pred = torch.randn(nb, C, *roi, device=dev)
    out = torch.zeros(1, C, D, H, W, device=dev)
    count = torch.zeros(1, D, H, W, device=dev)
    tabs, wmin = gaussian_tables(roi, 0.125)
    tabs = [t.to(dev) for t in tabs]

    def blend(kind):
        L.mmseg_window_blend(ptr(pred), 1, C, D, H, W, win_host.data_ptr(), nb, *roi, kind,
                             ptr(tabs[0]) if kind else None, ptr(tabs[1]) if kind else None,
                             ptr(tabs[2]) if kind else None, wmin, ptr(out), ptr(count), s)

    blend(0)
    covered = int((count > 0).sum())
    nbytes = 4 * (nb * C * rv + 2 * (C + 1) * covered)
    res["windows"], res["covered_voxels"] = [list(w) for w in wins], covered
    # the batch's working set (about 200 MB) fits the Infinity Cache: timed back to back it is served from there, so
    # each figure is taken twice, warm and with the cache rewritten before every launch
    flush = torch.empty(1 << 28, device=dev)
    res["blend_constant"] = rate(timed(lambda: blend(0), 5, args.reps), nbytes)
    res["blend_gaussian"] = rate(timed(lambda: blend(1), 5, args.reps), nbytes)
    res["blend_constant_cold"] = rate(timed(lambda: blend(0), 5, args.reps, flush), nbytes)
    res["blend_gaussian_cold"] = rate(timed(lambda: blend(1), 5, args.reps, flush), nbytes)

    def per_window():
        for k, (n, z0, y0, x0) in enumerate(wins):
            L.mmseg_window_accum(ptr(pred) + 4 * k * C * rv, 1, C, D, H, W, n, z0, y0, x0, *roi, ptr(out), s)

    # the per-window launches read and write every window's voxels, overlapped ones once per window, and keep no count
    res["per_window_accum_x%d" % nb] = rate(timed(per_window, 5, args.reps), 4 * 3 * nb * C * rv)
    res["per_window_accum_x%d_cold" % nb] = rate(timed(per_window, 5, args.reps, flush), 4 * 3 * nb * C * rv)
    src = torch.empty(D * H * W, device=dev)
    res["copy_fp32"] = rate(timed(lambda: count.view(-1).copy_(src), 5, args.reps), 8 * D * H * W)
    res["copy_fp32_cold"] = rate(timed(lambda: count.view(-1).copy_(src), 5, args.reps, flush), 8 * D * H * W)
    del src, pred, flush

    # finish: fused with the argmax against out /= count followed by argmax_encode (count = 1 keeps out stable)
    V = D * H * W
    out.copy_(torch.randint(-1, 2, (1, C, D, H, W), device=dev))
    count.fill_(1.0)
    mask = torch.empty(V, dtype=torch.uint8, device=dev)
    res["fused_finish_argmax"] = rate(timed(lambda: L.mmseg_blend_argmax_encode(ptr(out), ptr(count), C, D, H, W,
                                                                                 ptr(mask), s), 5, args.reps),
                                      4 * (C + 1) * V + V)
    fused = mask.clone()

    def two_pass():
        L.mmseg_window_finish(ptr(out), ptr(count), 1, C, V, s)
        L.mmseg_argmax_encode(ptr(out), C, D, H, W, ptr(mask), s)

    res["finish_then_argmax"] = rate(timed(two_pass, 5, args.reps), 4 * (3 * C + 1) * V + V)
    assert torch.equal(mask, fused)


def bench_predict(args, res):
    dev = torch.device("cuda", 0)
    cfg = make_config("unet", 2, "bf16", out_channels=args.classes)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev)
    model.eval()
    x = torch.randn(1, 2, *args.case, generator=torch.Generator().manual_seed(1)).to(dev)
    roi, nb = (args.roi,) * 3, args.sw_batch
    calls = [0]

    def predictor(b):
        calls[0] += 1
        return model(b)

    canned = torch.randn(nb, args.classes, *roi, device=dev)

    def no_model(b):                                   # everything but the forwards: gathers, flips, blend, mask
        return canned[:b.shape[0]]

    def run(blend, flips, pred=predictor):
        if blend == "constant" and not flips:
            return argmax_encode(sliding_window_inference(x, roi, nb, pred, 0.5)[0])
        out, count = sliding_window_accumulate(x, roi, nb, pred, 0.5, blend=blend, tta_flips=flips)
        return blend_argmax_encode(out[0], count[0])

    def wall(blend, flips, pred):
        run(blend, flips, pred)
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            run(blend, flips, pred)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}

    with torch.no_grad():
        batch = torch.randn(nb, 2, *roi, device=dev)
        fwd = timed(lambda: model(batch), 3, 10)
        res["predict"] = {"case": list(args.case), "model_forward_batch%d" % nb: fwd}
        for name, blend, flips in (("constant", "constant", ()), ("gaussian", "gaussian", ()),
                                   ("gaussian_tta8", "gaussian", (0, 1, 2))):
            calls[0] = 0
            r = wall(blend, flips, predictor)
            r["model_calls"] = calls[0] // 4           # one warm-up and three timed runs
            r["without_model_ms"] = wall(blend, flips, no_model)["ms_median"]
            r["model_share"] = 1.0 - r["without_model_ms"] / r["ms_median"]
            res["predict"][name] = r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[512, 512, 256])
    ap.add_argument("--case", type=int, nargs=3, default=[256, 256, 128])
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--roi", type=int, default=96)
    ap.add_argument("--sw-batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"shape": args.shape, "classes": args.classes, "roi": args.roi, "sw_batch": args.sw_batch, "reps": args.reps}
    bench_kernels(args, res)
    torch.cuda.empty_cache()
    bench_predict(args, res)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
