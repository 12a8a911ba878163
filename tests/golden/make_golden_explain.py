"""Generate tests/golden/explain.npz by running the REFERENCE's own GradCAM / GradCAMPlusPlus / SHAPAnalyzer
(src/explainability/) on its own UNet3D and DualEncoder(fusion_type="mean"), in float64 on the CPU.

Run once where the reference is mounted (it never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_explain.py

Only data is written.  Per map: 4,096 seeded sample voxels, the sum and the abs-sum (as the model fixtures), and
the error of the same computation in float32 on the CPU (max-normwise: max |a - b| / max |b|).  Per model: the gap
between the largest and second-largest value of output[0, c] -- Grad-CAM differentiates output[0, c].max(), so the
selected voxel must not depend on rounding: the generator refuses a seed / class whose gap is below
1e-3 * max |logit| (1,000 times the engine's measured logit parity of ~1e-6).

The attributions differentiate output[0, c].mean(), whose gradient passes through every max-pool and ReLU
decision of the network: an input on which float32 and float64 take a different decision somewhere gives maps
that differ by ~1e-2 at a few voxels (5 of the 10 (seed, model) pairs probed differ by more than 1e-3), which says nothing about the code
under test.  The generator therefore also refuses an input whose gradient-SHAP map differs by more than 1e-4
between float32 and float64 on the CPU (the maps kept differ by ~1e-5).

The reference modules are loaded file by file: its src/explainability/__init__.py also imports the t-SNE and
attention visualisers, whose dependencies are absent here; matplotlib (imported by shap_analysis.py for its plot
helper only) is stubbed when missing.
"""
from __future__ import annotations

import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("MMSEG_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))

FEATURES = [8, 16, 32, 64, 128]
S, M, C = 32, 2, 3
CLS = 1
N_STEPS = 8
NSAMP = 4096
SEEDS = {"unet": 0, "dual": 0}          # model init seed; inputs come from INPUT_SEED
INPUT_SEED, BG_SEED, SAMPLE_SEED = 41, 12, 13
LAYERS = {"unet": ["init_conv", "encoders.0.conv", "encoders.3.conv", "decoders.0", "decoders.3"],
          "dual": ["encoders.0.init_conv", "encoders.1.blocks.3.conv", "decoder.3"]}


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _import_reference():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    try:
        import matplotlib.pyplot  # noqa: F401
    except Exception:
        mpl = types.ModuleType("matplotlib")
        mpl.pyplot = types.ModuleType("matplotlib.pyplot")
        sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, mpl.pyplot
    unet = _load("ref_unet", "src/models/backbones/unet.py")
    sys.modules.setdefault("src", types.ModuleType("src"))
    for pkg in ("src.models", "src.models.backbones"):
        sys.modules.setdefault(pkg, types.ModuleType(pkg))
    sys.modules["src.models.backbones.unet"] = unet
    dual = _load("ref_dual", "src/models/backbones/dual_encoder.py")
    cam = _load("ref_gradcam", "src/explainability/gradcam.py")
    shap = _load("ref_shap", "src/explainability/shap_analysis.py")
    return unet, dual, cam, shap


def inputs():
    g = torch.Generator().manual_seed(INPUT_SEED)
    x = torch.randn(1, M, S, S, S, generator=g)
    g = torch.Generator().manual_seed(BG_SEED)
    bg = torch.randn(3, M, S, S, S, generator=g)
    return x, bg


def sample_index(n):
    return np.random.default_rng(SAMPLE_SEED).choice(n, size=min(NSAMP, n), replace=False)


def max_normwise(a, b):
    d = np.abs(b).max()
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / (d if d > 0 else 1.0))


def maps(model, cam_mod, shap_mod, layers, x, bg):
    """Every map of one model, in the model's dtype."""
    dt = next(model.parameters()).dtype
    x, bg = x.to(dt), bg.to(dt)
    out = {}
    for tag, cls in (("gradcam", cam_mod.GradCAM), ("gradcampp", cam_mod.GradCAMPlusPlus)):
        m = copy.deepcopy(model)                      # (each instance leaves its hooks on the model)
        c = cls(m, list(layers), use_cuda=False)
        for layer in layers:
            out[f"{tag}__{layer}"] = np.asarray(c(x.clone(), CLS, layer))
    sh = shap_mod.SHAPAnalyzer(copy.deepcopy(model), background_samples=bg)
    out["shap_gradient"] = np.asarray(sh.compute_shap_values(x.clone(), CLS, "gradient"))
    out["shap_ig"] = np.asarray(sh._integrated_gradients(x.clone(), CLS, n_steps=N_STEPS))
    return out


def main():
    unet_mod, dual_mod, cam_mod, shap_mod = _import_reference()
    x, bg = inputs()
    store = {"features": np.array(FEATURES), "S": np.array(S), "M": np.array(M), "C": np.array(C),
             "cls": np.array(CLS), "n_steps": np.array(N_STEPS), "input_seed": np.array(INPUT_SEED),
             "bg_seed": np.array(BG_SEED)}
    for name in ("unet", "dual"):
        torch.manual_seed(SEEDS[name])
        if name == "unet":
            model = unet_mod.UNet3D(in_channels=M, out_channels=C, features=list(FEATURES))
        else:
            model = dual_mod.DualEncoder(num_modalities=M, out_channels=C, features=list(FEATURES),
                                         fusion_type="mean")
        model.eval()
        m64 = copy.deepcopy(model).double()
        with torch.no_grad():
            lg = m64(x.double())[0, CLS].flatten()
            top = torch.topk(lg, 2).values
            allmax = m64(x.double()).abs().max().item()
        gap = (top[0] - top[1]).item()
        if gap < 1e-3 * allmax:
            raise SystemExit(f"{name}: top-1 to top-2 gap {gap:.3e} of output[0, {CLS}] is below 1e-3 * max|logit| "
                             f"= {1e-3 * allmax:.3e}: choose another seed or class")
        store[f"{name}__seed"] = np.array(SEEDS[name])
        store[f"{name}__gap"] = np.array(gap)
        store[f"{name}__max_abs_logit"] = np.array(allmax)
        ref = maps(m64, cam_mod, shap_mod, LAYERS[name], x, bg)
        f32 = maps(model.float(), cam_mod, shap_mod, LAYERS[name], x, bg)
        for k, v in ref.items():
            flat = v.astype(np.float64).reshape(-1)
            idx = sample_index(flat.size)
            store[f"{name}__{k}__idx"] = idx.astype(np.int64)
            store[f"{name}__{k}__val"] = flat[idx]
            store[f"{name}__{k}__sum"] = np.array(flat.sum())
            store[f"{name}__{k}__abs"] = np.array(np.abs(flat).sum())
            store[f"{name}__{k}__max"] = np.array(np.abs(flat).max())
            store[f"{name}__{k}__shape"] = np.array(v.shape)
            store[f"{name}__{k}__err32"] = np.array(max_normwise(f32[k], v))
            if k == "shap_gradient" and store[f"{name}__{k}__err32"] > 1e-4:
                raise SystemExit(f"{name}: gradient-SHAP differs by {store[f'{name}__{k}__err32']:.2e} between float32 "
                                 "and float64 (a pool / ReLU decision flips): choose another input seed")
            print(f"{name} {k}: shape {v.shape} sum {flat.sum():.6e} fp32 err {store[f'{name}__{k}__err32']:.2e}")
        print(f"{name}: gap {gap:.4f} max|logit| {allmax:.3f}")
    np.savez_compressed(os.path.join(OUT, "explain.npz"), **store)


if __name__ == "__main__":
    main()
