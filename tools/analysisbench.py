#!/usr/bin/env python3
"""mmseg_suv_analyze at 512 x 512 x 256 (int16 SUV with slope / inter, uint8 mask): each kernel's own duration (the
library's launch timing), against its compulsory bytes (both volumes read once per pass; pass 3 also writes the three
masks), with a torch.Tensor.copy_ of the same volume bytes from the same run as the yardstick, and the wall time of
the numpy statement (tests/analysis_ref.py: SUV + TMTV + histogram statistics) on the same volume.  Warm-up, then
--reps calls; the median over the calls of each kernel's time.  Needs an MI355X.

    python tools/analysisbench.py [--out profiles/analysis_bench.json]      (DESIGN.md "Analysis")
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mmseg_amd  # noqa: E402,F401
from mmseg_amd._lib import lib, ptr, stream_handle  # noqa: E402
from mmseg_amd.analysis import core  # noqa: E402


def phantom(shape, seed=0):
    """int16 SUVs (stored = SUV / slope) around 1 with organs and lesions, and a uint8 mask of seven boxes."""
    X, Y, Z = shape
    rng = np.random.default_rng(seed)
    suv = rng.gamma(4.0, 100.0, shape).astype(np.int16)               # about 1 SUV at slope 0.0025
    seg = np.zeros(shape, dtype=np.uint8)
    for l in range(1, 8):
        x0, y0, z0 = (l * X) // 9, ((l * 3) % 7 * Y) // 9, ((l * 5) % 7 * Z) // 9
        seg[x0:x0 + X // 8, y0:y0 + Y // 6, z0:z0 + Z // 5] = l
        n = int((seg == l).sum())
        suv[seg == l] = rng.gamma(5.0, 100.0 + 40.0 * l, n).astype(np.int16)
    hot = (rng.random(shape) < 0.002) & (seg == 0)
    suv[hot] = rng.integers(1000, 5000, int(hot.sum()), dtype=np.int16)
    return suv, seg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[512, 512, 256])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ref-reps", type=int, default=3, help="runs of the numpy path (0 skips it)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    X, Y, Z = args.shape
    V = X * Y * Z
    dev = torch.device("cuda", 0)
    L, s = lib(), stream_handle()
    suv_h, seg_h = phantom((X, Y, Z))
    slope, inter = float(np.float32(0.0025)), float(np.float32(-0.25))
    suv = torch.from_numpy(suv_h.ravel(order="F").copy()).to(dev)
    seg = torch.from_numpy(seg_h.ravel(order="F").copy()).to(dev)
    crel, cabs = core.curve_thresholds()
    curves = torch.from_numpy(np.concatenate([crel, cabs])).to(dev)
    record = torch.empty(core.R_CELLS, dtype=torch.int64, device=dev)
    ws_bytes = int(L.mmseg_suv_ws_bytes(V))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    masks = torch.empty(3 * V, dtype=torch.uint8, device=dev)

    def call():
        L.mmseg_suv_analyze(ptr(suv), 4, 0, 1, slope, inter, ptr(seg), 2, 0, 0, 0.0, 0.0, X, Y, Z, 7, 5, 2.5, 0.4, 2.5,
                            ptr(curves), ptr(curves) + 8 * len(crel), len(crel), 100, ptr(masks), ptr(record), ptr(ws),
                            ws_bytes, s)

    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    whole, per = [], {}
    ms, nm = ctypes.c_float(), ctypes.c_char_p()
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        whole.append(a.elapsed_time(b))
    for _ in range(args.reps):
        L.mmseg_timing_begin()
        call()
        torch.cuda.synchronize()
        L.mmseg_timing_end()
        one = {}
        for i in range(L.mmseg_timing_count()):
            L.mmseg_timing_get(i, ctypes.addressof(ms), ctypes.addressof(nm))
            one.setdefault(nm.value.decode(), []).append(ms.value)
        for k, v in one.items():
            per.setdefault(k, []).append(v)
    in_bytes = V * 3
    res = {"shape": [X, Y, Z], "reps": args.reps, "ws_bytes": ws_bytes,
           "call": {"ms_median": statistics.median(whole), "ms_min": min(whole), "ms_max": max(whole)}}
    small = 0.0
    for k, runs in per.items():
        launches = len(runs[0])
        each = statistics.median([sum(r) / launches for r in runs])
        if k in ("suv_pass1_kernel", "suv_pass2_kernel", "suv_pass3_kernel", "suv_sel_hist_kernel"):
            nbytes = in_bytes + (3 * V if k == "suv_pass3_kernel" else 0)
            res[k] = {"launches": launches, "ms_median_each": each, "bytes": nbytes, "GBps": nbytes / each / 1e6}
        else:
            small += each * launches
    res["finalize_pick_peak_ms_total"] = small

    src = torch.empty(in_bytes, dtype=torch.uint8, device=dev)
    dst = torch.empty(in_bytes, dtype=torch.uint8, device=dev)
    for _ in range(5):
        dst.copy_(src)
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    cms = statistics.median(ts)
    res["copy_same_bytes"] = {"ms_median": cms, "bytes": 2 * in_bytes, "GBps": 2 * in_bytes / cms / 1e6}
    for k in ("suv_pass1_kernel", "suv_pass2_kernel", "suv_pass3_kernel", "suv_sel_hist_kernel"):
        if k in res:
            res[k]["of_copy_rate"] = res[k]["GBps"] / res["copy_same_bytes"]["GBps"]

    u = record.cpu().numpy().view(np.uint64)
    res["counts"] = {"absolute": int(u[core.R_ABS]), "liver": int(u[core.R_SLOT + 8 * 5]), "invalid": int(u[0])}
    if args.ref_reps > 0:
        import analysis_ref as AR
        vol = suv_h.astype(np.float64) * np.float64(np.float32(slope)) + np.float64(np.float32(inter))
        lab = seg_h.astype(np.int32)
        ts = []
        for _ in range(args.ref_reps):
            t0 = time.perf_counter()
            a = AR.suv_stats(vol, lab, np.float32(0.0045))
            t, _ = AR.tmtv_stats(vol, lab, np.float32(0.0045))
            AR.histogram_stats(vol, lab)
            ts.append(time.perf_counter() - t0)
        res["numpy_path_s"] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
        assert t["absolute"]["num_voxels"] == res["counts"]["absolute"]
        assert [r for r in a["organs"] if r["organ"] == "liver"][0]["volume_voxels"] == res["counts"]["liver"]
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
