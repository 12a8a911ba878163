"""Time the fused augmentation launch (mmseg_augment) against the same work as a torch composite, and the
device loader with augmentation on and off:

    python tools/augbench.py [--iters 40] [--rounds 5] [--out FILE.json]

Each measurement runs in a child process of its own under a time limit (a failed or hung step ends the
run; nothing is started after it).  Per sample shape (c3: [2, 96^3], c4: [2, 128^3], int64 label), with every
transform switched on (three flips, one quarter turn, per-channel affine, noise):

  fused      one mmseg_augment launch, outputs preallocated
  composite  torch.flip, torch.rot90(...).contiguous(), mul / add, randn and add, and flip / rot90 of the label

Both are timed with HIP events over --iters launches queued behind a spin kernel, so the events see the
GPU run them back to back and not the Python that enqueues them ("queued_us"; "host_bound" is set when
the enqueue outlasted the spin kernel and the figure is the host's pace instead).  fused and composite
alternate --rounds times in one process; medians are reported.  "kernel_us" is the fused kernel's own
duration from the library's launch timing (mmseg_timing_*), and GB/s = compulsory bytes (image and label,
read once and written once) over it, against the 8 TB/s HBM peak.  The loader step times an epoch of
get_dataloader(...) at 96^3 per sample, augmentation on and off, alternating.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"c3": (2, 96, 96, 96), "c4": (2, 128, 128, 128)}
HBM_PEAK = 8.0e12


def _queued_us(fn, iters, spin_cycles):
    """Median-free single window: iters calls of fn queued behind a spin kernel, event time per call."""
    import torch
    start, stop, s0 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    torch.cuda.synchronize()
    s0.record()
    torch.cuda._sleep(spin_cycles)
    start.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    host = time.perf_counter() - t0
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters, host * 1e3 > s0.elapsed_time(start)


def case(tag, iters, rounds, warmup):
    import torch
    from mmseg_amd._lib import lib, ptr, stream_handle
    dev = torch.device("cuda", 0)
    C, D, H, W = SHAPES[tag]
    g = torch.Generator(device=dev).manual_seed(0)
    img = torch.randn(C, D, H, W, device=dev, generator=g)
    lab = torch.randint(0, 6, (D, H, W), device=dev, generator=g)
    out, lab_out = torch.empty(C, H, D, W, device=dev), torch.empty(H, D, W, dtype=torch.int64, device=dev)
    scale_h, shift_h = [1.05, 0.95, 1.02, 0.98][:C], [0.03, -0.02, 0.01, -0.04][:C]
    scale_c, shift_c = (ctypes.c_float * C)(*scale_h), (ctypes.c_float * C)(*shift_h)
    key = ctypes.c_ulonglong(0x1234567887654321)
    L, s = lib(), stream_handle()

    def fused(noise=1):
        L.mmseg_augment(ptr(img), C, D, H, W, ptr(lab), 8, 7, 1, ctypes.addressof(scale_c),
                        ctypes.addressof(shift_c), noise, 0.0, 0.05, ctypes.addressof(key), ptr(out),
                        ptr(lab_out), s)

    scale_t = torch.tensor(scale_h, device=dev).view(C, 1, 1, 1)
    shift_t = torch.tensor(shift_h, device=dev).view(C, 1, 1, 1)

    def composite():
        x = torch.rot90(torch.flip(img, (1, 2, 3)), 1, (1, 2)).contiguous()
        x.mul_(scale_t).add_(shift_t)
        x.add_(torch.randn_like(x).mul_(0.05))
        y = torch.rot90(torch.flip(lab, (0, 1, 2)), 1, (0, 1)).contiguous()
        return x, y

    # the two do the same geometry (the composite's noise values are torch's own)
    fused(0)
    x, y = composite()
    assert torch.equal(lab_out, y) and (out - x).abs().max().item() < 0.5
    for _ in range(warmup):
        fused()
        fused(0)
        composite()
    spin = 20_000_000
    res = {"fused": [], "fused_no_noise": [], "composite": []}
    bound = {k: False for k in res}
    for _ in range(rounds):
        for name, fn in (("fused", fused), ("composite", composite), ("fused_no_noise", lambda: fused(0))):
            us, hb = _queued_us(fn, iters, spin)
            res[name].append(us)
            bound[name] |= hb
    # the fused kernel's own duration
    kern = {}
    for name, noise in (("fused", 1), ("fused_no_noise", 0)):
        L.mmseg_timing_begin()
        for _ in range(iters):
            fused(noise)
        torch.cuda.synchronize()
        L.mmseg_timing_end()
        ms, nm = ctypes.c_float(), ctypes.c_char_p()
        durs = []
        for i in range(L.mmseg_timing_count()):
            L.mmseg_timing_get(i, ctypes.addressof(ms), ctypes.addressof(nm))
            durs.append(ms.value * 1e3)
        kern[name] = statistics.median(durs)
    nbytes = 2 * (C * D * H * W * 4 + D * H * W * 8)
    r = {"case": tag, "shape": [C, D, H, W], "compulsory_bytes": nbytes, "iters": iters, "rounds": rounds}
    for name, v in res.items():
        r[name] = {"queued_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
                   "max_us": round(max(v), 2), "host_bound": bound[name]}
    for name, us in kern.items():
        r[name].update(kernel_us=round(us, 2), gbps=round(nbytes / us / 1e3, 1),
                       hbm_peak_share=round(nbytes / (us * 1e-6) / HBM_PEAK, 3))
    r["fused_over_composite"] = round(r["fused"]["queued_us"] / r["composite"]["queued_us"], 3)
    print(json.dumps(r), flush=True)


def loader(rounds):
    import torch
    from mmseg_amd.data import get_dataloader

    def cfg(aug):
        c = {"data": {"modalities": ["CT", "PET"], "synthetic": {"n_train": 8, "size": 96, "device": True}},
             "model": {"out_channels": 6}, "training": {"batch_size": 2}, "hardware": {}}
        if aug:
            c["data"]["augmentation"] = {"enabled": True, "random_flip": True, "random_rotate": 15,
                                         "random_intensity": 0.1}
        return c

    loaders = {"off": get_dataloader(cfg(False), "train"), "on": get_dataloader(cfg(True), "train")}
    times = {k: [] for k in loaders}
    for rnd in range(rounds + 1):          # round 0 warms up
        for name, ld in loaders.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = sum(b["image"].shape[0] for b in ld)
            torch.cuda.synchronize()
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e3 / n)
    r = {"case": "loader", "size": 96, "samples_per_epoch": 8, "rounds": rounds}
    for name, v in times.items():
        r[f"ms_per_sample_{name}"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3),
                                      "max": round(max(v), 3)}
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step", choices=list(SHAPES) + ["loader"], help="run one step in this process")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per child step")
    ap.add_argument("--out", help="also write the result lines here")
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters: at least 20 launches per window")
    if a.step in SHAPES:
        return case(a.step, a.iters, a.rounds, a.warmup)
    if a.step == "loader":
        return loader(a.rounds)
    lines = []
    for step in list(SHAPES) + ["loader"]:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step,
               "--iters", str(a.iters), "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.exit(f"augbench: step {step} ended with status {p.returncode}; nothing further is run")
        lines += [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
