#!/usr/bin/env python3
"""mmseg_nifti_decode (int16, slope / inter) and mmseg_argmax_encode (C = 6) at 512 x 512 x 256, against the
compulsory bytes (read raw + write fp32; read logits + write uint8), with a same-size fp32 copy and torch.argmax
for scale and the host path the decode replaces (np.frombuffer -> reshape "F" -> float64 scale -> float32 ->
ascontiguousarray).  Warm-up, HIP events around each launch, median of --reps.  Needs an MI355X.

    python tools/niftibench.py [--out profiles/nifti_bench.json]      (DESIGN.md "NIfTI volumes")
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmseg_amd  # noqa: E402,F401
from mmseg_amd._lib import lib, ptr, stream_handle  # noqa: E402


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[512, 512, 256])
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    (X, Y, Z), C = args.shape, args.classes
    N = X * Y * Z
    dev = torch.device("cuda", 0)
    L, s = lib(), stream_handle()
    raw_h = np.random.default_rng(0).integers(-1024, 3000, N, dtype=np.int16)
    slope, inter = float(np.float32(0.5)), float(np.float32(-1024.0))
    res = {"shape": [X, Y, Z], "classes": C, "reps": args.reps}

    raw = torch.from_numpy(raw_h).to(dev)
    out = torch.empty(X, Y, Z, dtype=torch.float32, device=dev)
    r = timed(lambda: L.mmseg_nifti_decode(ptr(raw), 4, 0, X, Y, Z, 1, slope, inter, ptr(out), s), 5, args.reps)
    r["bytes"] = N * 6
    r["GBps"] = r["bytes"] / r["ms_median"] / 1e6
    res["decode_int16_scaled"] = r
    ref = (raw_h.reshape((X, Y, Z), order="F")[:64, Y // 2, :].astype(np.float64) * slope + inter).astype(np.float32)
    assert np.array_equal(out[:64, Y // 2, :].cpu().numpy(), ref)
    src = torch.empty(N, dtype=torch.float32, device=dev)
    r = timed(lambda: out.view(-1).copy_(src), 5, args.reps)
    r["bytes"] = N * 8
    r["GBps"] = r["bytes"] / r["ms_median"] / 1e6
    res["copy_fp32"] = r
    del src, raw

    logits = torch.randint(-1, 2, (C, X, Y, Z), device=dev).float()
    mask = torch.empty(N, dtype=torch.uint8, device=dev)
    r = timed(lambda: L.mmseg_argmax_encode(ptr(logits), C, X, Y, Z, ptr(mask), s), 5, args.reps)
    r["bytes"] = C * N * 4 + N
    r["GBps"] = r["bytes"] / r["ms_median"] / 1e6
    res["argmax_encode"] = r
    assert torch.equal(mask.view(Z, Y, X)[:, Y // 2, :64].t(), torch.argmax(logits[:, :64, Y // 2, :], 0).to(torch.uint8))
    res["torch_argmax_int64"] = timed(lambda: torch.argmax(logits, 0), 2, 10)
    del logits

    blob = raw_h.tobytes()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        v = np.frombuffer(blob, dtype=np.int16).reshape((X, Y, Z), order="F")
        np.ascontiguousarray((v.astype(np.float64) * slope + inter).astype(np.float32))
        ts.append((time.perf_counter() - t0) * 1e3)
    res["host_path"] = {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
