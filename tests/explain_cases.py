"""Shared by the explainability tests: the fixture's models, inputs and comparisons (tests/golden/explain.npz,
written by tests/golden/make_golden_explain.py from the reference's own classes in float64)."""
import numpy as np
import torch

from mmseg_amd.models.build import build_model
from tests.helpers import golden
from tests.test_model_gpu import make_config

LAYERS = {"unet": ["init_conv", "encoders.0.conv", "encoders.3.conv", "decoders.0", "decoders.3"],
          "dual": ["encoders.0.init_conv", "encoders.1.blocks.3.conv", "decoder.3"]}
CAMS = [(m, tag, layer) for m in ("unet", "dual") for tag in ("gradcam", "gradcampp") for layer in LAYERS[m]]


def fixture():
    return golden("explain")


def inputs(g):
    gen = torch.Generator().manual_seed(int(g["input_seed"]))
    S, M = int(g["S"]), int(g["M"])
    x = torch.randn(1, M, S, S, S, generator=gen)
    gen = torch.Generator().manual_seed(int(g["bg_seed"]))
    bg = torch.randn(3, M, S, S, S, generator=gen)
    return x, bg


def build(g, name, device="cpu", kernels="torch", dtype="float32", fusion=None):
    """The fixture's model (the reference's weights: same seed, same RNG order) behind the product's wrapper."""
    kind = "unet" if name == "unet" else "dual_encoder"
    cfg = make_config(kind, ["CT", "PET"][:int(g["M"])], int(g["C"]), list(g["features"]),
                      fusion=fusion or "cross_attention", dtype=dtype)
    cfg["hardware"]["device"] = device
    cfg["hardware"]["kernels"] = kernels
    torch.manual_seed(int(g[f"{name}__seed"]))
    return build_model(cfg)


def fixture_err(g, key, got):
    """max |got - ref| / max |ref| over the fixture's sample voxels, plus the relative sum / abs-sum errors."""
    got = np.asarray(got)
    assert tuple(got.shape) == tuple(g[f"{key}__shape"]), (got.shape, g[f"{key}__shape"])
    assert got.dtype == np.float32
    flat = got.astype(np.float64).reshape(-1)
    mx = float(g[f"{key}__max"])
    err = np.abs(flat[g[f"{key}__idx"]] - g[f"{key}__val"]).max() / mx
    den = float(g[f"{key}__abs"])
    return float(err), abs(flat.sum() - float(g[f"{key}__sum"])) / den, abs(np.abs(flat).sum() - den) / den
