"""Time the patch sampler's kernels (csrc/patch.hip):

    python tools/patchbench.py [--iters 40] [--out FILE.json]

2 channels, P = 4 patches of 96^3 out of a 256^3 volume, int64 labels: mmseg_patch_sample on its copy path and
on its affine path (15 degrees about every axis, scale 1.1), mmseg_patch_pick (foreground picks) and
mmseg_fg_count.  The measurement runs in a child process under a time limit (a failed or hung step ends the
run).  Every kernel's own duration comes from the library's launch timing (mmseg_timing_*): the median over
--iters launches.  GB/s = bytes written + bytes read over that duration, against the 8 TB/s HBM peak: for the
sampler the patches written and as many source bytes read (the affine path's 8 corners come out of the caches),
for mmseg_fg_count the label read once, for mmseg_patch_pick the counts and one chunk of the label per patch.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, S, PSZ, P = 2, 256, 96, 4
HBM_PEAK = 8.0e12


def _kernel_us(L, fn, iters):
    import torch
    L.mmseg_timing_begin()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    L.mmseg_timing_end()
    ms, nm = ctypes.c_float(), ctypes.c_char_p()
    durs = []
    for i in range(L.mmseg_timing_count()):
        L.mmseg_timing_get(i, ctypes.addressof(ms), ctypes.addressof(nm))
        durs.append(ms.value * 1e3)
    return statistics.median(durs), min(durs), max(durs)


def step(iters, warmup):
    import torch
    from mmseg_amd._lib import lib
    from mmseg_amd.data.patch import DevicePatchSampler, PatchParams, affine_matrix
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    img = torch.randn(C, S, S, S, device=dev, generator=g)
    lab = (torch.rand(S, S, S, device=dev, generator=g) < 0.05).long()
    sampler = DevicePatchSampler((PSZ,) * 3)
    L = lib()
    counts = sampler.fg_counts(lab)
    M = affine_matrix((15.0, 15.0, 15.0), 1.1)
    plain = [PatchParams(mode=1, u=(j + 0.5) / P, fallback_start=(0, 0, 0)) for j in range(P)]
    turned = [PatchParams(mode=1, u=(j + 0.5) / P, fallback_start=(0, 0, 0), affine=True, M=M) for j in range(P)]
    starts = sampler.pick(lab, counts, plain)
    steps = {"sample_copy": lambda: sampler.sample(img, lab, starts, plain),
             "sample_affine": lambda: sampler.sample(img, lab, starts, turned),
             "pick": lambda: sampler.pick(lab, counts, plain),
             "fg_count": lambda: sampler.fg_counts(lab)}
    pvox = P * PSZ ** 3
    nbytes = {"sample_copy": 2 * pvox * (C * 4 + 8), "sample_affine": 2 * pvox * (C * 4 + 8),
              "pick": counts.numel() * 4 + P * 4096 * 8 + P * 12, "fg_count": S ** 3 * 8 + counts.numel() * 4}
    r = {"volume": [C, S, S, S], "patch": [PSZ] * 3, "patches": P, "label": "int64", "iters": iters,
         "device": torch.cuda.get_device_name(0)}
    for name, fn in steps.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        med, lo, hi = _kernel_us(L, fn, iters)
        r[name] = {"kernel_us": round(med, 2), "min_us": round(lo, 2), "max_us": round(hi, 2),
                   "bytes": nbytes[name], "gbps": round(nbytes[name] / med / 1e3, 1),
                   "hbm_peak_share": round(nbytes[name] / (med * 1e-6) / HBM_PEAK, 4)}
    r["sampler_us_per_patch"] = {k: round((r[k]["kernel_us"] + r["pick"]["kernel_us"]) / P, 2)
                                 for k in ("sample_copy", "sample_affine")}
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step", action="store_true", help="measure in this process")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds for the child")
    ap.add_argument("--out", help="also write the result line here")
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters: at least 20 launches")
    if a.step:
        return step(a.iters, a.warmup)
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step",
           "--iters", str(a.iters), "--warmup", str(a.warmup)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        sys.exit(f"patchbench: the measurement ended with status {p.returncode}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(ln + "\n" for ln in p.stdout.splitlines() if ln.startswith("{")))


if __name__ == "__main__":
    main()
