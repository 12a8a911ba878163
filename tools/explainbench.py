"""Explainability timings (recorded in DESIGN.md "Explainability", not gated): Grad-CAM, Grad-CAM++, gradient-SHAP
and 50-step integrated gradients at c2 (UNet3D 96^3) and c3 (DualEncoder 96^3) on the HIP engine and on
`hardware.kernels: torch`, and the stem data gradient and each csrc/explain.hip kernel in GB/s against their
compulsory bytes.  Each step runs as a child process under its own time limit; nothing starts after a failure.

    python tools/explainbench.py [--out profiles/explain_bench.json] [--steps models,kernels]
    python tools/explainbench.py --child models --config c2 --kernels hip          (one step, in this process)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = {"c2": "configs/c2_unet_96_bf16.yaml", "c3": "configs/c3_dual_encoder_96_dp.yaml"}


def _time(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def child_models(config, kernels, ig_steps):
    import torch
    import mmseg_amd  # noqa: F401
    from mmseg_amd.explainability import GradCAM, GradCAMPlusPlus, SHAPAnalyzer
    from mmseg_amd.explainability.common import default_layer
    from mmseg_amd.models.build import build_model
    from mmseg_amd.utils import load_config
    cfg = load_config(os.path.join(ROOT, CONFIGS[config]))
    cfg["hardware"]["kernels"] = kernels
    torch.manual_seed(0)
    model = build_model(cfg).eval()
    M = len(cfg["data"]["modalities"])
    S = cfg["model"]["backbone"].get("img_size", [96, 96, 96])
    x = torch.randn(1, M, *S, device="cuda")
    bg = torch.randn(2, M, *S, device="cuda")
    layer = default_layer(model)
    sh = SHAPAnalyzer(model, background_samples=bg)
    res = {"config": config, "kernels": kernels, "layer": layer, "dtype": str(model.backbone.engine_dtype)}
    res["gradcam_ms"] = _time(lambda: GradCAM(model, [layer])(x, 1), 5)
    res["gradcampp_ms"] = _time(lambda: GradCAMPlusPlus(model, [layer])(x, 1), 5)
    res["gradient_shap_ms"] = _time(lambda: sh.compute_shap_values(x, 1, "gradient"), 5)
    res[f"integrated_gradients_{ig_steps}_ms"] = _time(
        lambda: sh.compute_shap_values(x, 1, "integrated_gradients", n_steps=ig_steps), 1)
    print("RESULT " + json.dumps(res), flush=True)


def child_kernels():
    import torch
    import mmseg_amd  # noqa: F401
    from mmseg_amd._lib import lib, stream_handle
    L, s = lib(), stream_handle()
    dev = torch.device("cuda", 0)
    S, C, ncls = 96, 32, 6
    V = S ** 3
    out = {}
    f32 = lambda *sh: torch.randn(*sh, device=dev)   # noqa: E731
    ws = torch.empty(L.mmseg_explain_ws_floats(), device=dev)
    logits, dl = f32(ncls * V), torch.empty(ncls * V, device=dev)
    for mode, tag in ((0, "seed_max"), (1, "seed_mean")):
        ms = _time(lambda: L.mmseg_explain_seed(logits.data_ptr(), ncls, V, 1, mode, dl.data_ptr(), ws.data_ptr(), s), 20)
        out[tag] = (ms, 4.0 * V * (ncls + (1 if mode == 0 else 0) + (1 if mode == 0 else 0)))
    for dt, code, es in ((torch.float32, 0, 4), (torch.bfloat16, 1, 2)):
        A = torch.randn(V * C, device=dev).clamp(min=0).to(dt)
        p1 = torch.randn(V * 2 * C, device=dev).to(dt)
        pd = torch.randn(V // 8 * C, device=dev).to(dt)
        idx = torch.randint(0, 8, (V // 8 * C,), device=dev, dtype=torch.uint8)
        w = torch.empty(C, device=dev)
        cws = torch.empty(L.mmseg_cam_ws_floats(V, C), device=dev)
        gbytes = V * C * es + V // 8 * C * (es + 1)
        for mode, tag, nb in ((0, "cam_weights", gbytes), (1, "cam_weights_pp", gbytes + 2 * V * C * es)):
            ms = _time(lambda: L.mmseg_cam_weights(A.data_ptr(), C, p1.data_ptr() + C * es, 2 * C, 1.0, pd.data_ptr(),
                                                   C, idx.data_ptr(), S, S, S, C, mode, w.data_ptr(), cws.data_ptr(),
                                                   code, s), 20)
            out[f"{tag}[{dt}]"] = (ms, float(nb))
        cam = torch.empty(V, device=dev)
        ms = _time(lambda: L.mmseg_cam_combine(A.data_ptr(), C, w.data_ptr(), V, C, cam.data_ptr(), code, s), 20)
        out[f"cam_combine[{dt}]"] = (ms, float(V * C * es + 4 * V))
        for ci in (1, 2):
            wt = f32(C * ci * 27)
            dx = torch.empty(ci * V, device=dev)
            ms = _time(lambda: L.mmseg_stem_dgrad(A.data_ptr(), C, C, wt.data_ptr(), ci, dx.data_ptr(), ci, 0, 1, S, S,
                                                  S, 0, code, s), 20)
            out[f"stem_dgrad_ci{ci}[{dt}]"] = (ms, float(V * C * es + 4 * ci * V))
    small = f32(12 ** 3).clamp(min=0)
    big = torch.empty(V, device=dev)
    ms = _time(lambda: L.mmseg_cam_upsample_norm(small.data_ptr(), 12, 12, 12, big.data_ptr(), S, S, S, ws.data_ptr(),
                                                 s), 20)
    out["cam_upsample_norm_x8"] = (ms, 4.0 * V * 3)
    x, b, g = f32(2 * V), f32(2 * V), f32(2 * V)
    o = torch.empty(2 * V, device=dev)
    ms = _time(lambda: L.mmseg_attr_lerp(x.data_ptr(), b.data_ptr(), 0.5, o.data_ptr(), 2 * V, s), 20)
    out["attr_lerp"] = (ms, 4.0 * 2 * V * 3)
    ms = _time(lambda: L.mmseg_attr_finish(x.data_ptr(), b.data_ptr(), g.data_ptr(), 1.0, o.data_ptr(), 2 * V, s), 20)
    out["attr_finish"] = (ms, 4.0 * 2 * V * 4)
    res = {k: {"us": round(ms * 1e3, 2), "GBps": round(nb / (ms * 1e-3) / 1e9, 1)} for k, (ms, nb) in out.items()}
    print("RESULT " + json.dumps({"kernels_96": res}), flush=True)


def run_child(argv, limit):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True,
                       timeout=limit, cwd=ROOT)
    sys.stderr.write(p.stderr[-2000:])
    if p.returncode != 0:
        raise SystemExit(f"step {argv} failed with status {p.returncode}: nothing further is started")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", default="models,kernels")
    ap.add_argument("--ig-steps", type=int, default=50)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child step")
    ap.add_argument("--child", default=None, choices=["models", "kernels"])
    ap.add_argument("--config", default="c2", choices=list(CONFIGS))
    ap.add_argument("--kernels", default="hip", choices=["hip", "torch"])
    args = ap.parse_args()
    if args.child == "models":
        return child_models(args.config, args.kernels, args.ig_steps)
    if args.child == "kernels":
        return child_kernels()
    results = []
    steps = args.steps.split(",")
    if "kernels" in steps:
        results.append(run_child(["--child", "kernels"], args.limit))
    if "models" in steps:
        for config in CONFIGS:
            for kernels in ("hip", "torch"):
                results.append(run_child(["--child", "models", "--config", config, "--kernels", kernels,
                                          "--ig-steps", str(args.ig_steps)], args.limit))
    for r in results:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
