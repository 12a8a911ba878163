"""Shared by the CAM and SHAP classes: layer names, argument checks, the engine handle and the kernel calls."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from ..models.backbones.dual_encoder import DualEncoder
from ..models.backbones.unet import UNet3D

SEED_MAX, SEED_MEAN = 0, 1
CAM, CAM_PP = 0, 1


def backbone_of(model: nn.Module) -> nn.Module:
    """The network under the reference's pass-through wrapper (build.py MultiModalSegmentationModel), or itself."""
    bb = model.backbone if hasattr(model, "backbone") and isinstance(model.backbone, nn.Module) else model
    if not isinstance(bb, (UNet3D, DualEncoder)):
        raise NotImplementedError(f"explainability covers UNet3D and DualEncoder, not {type(bb).__name__} "
                                  "(SwinUNETR has no taps / data-only backward on the engine)")
    return bb


def valid_layers(model: nn.Module) -> List[str]:
    """Layer names the CAMs accept: the modules whose output is one tensor (the reference's hooks raise on
    `encoders.{i}`, whose DownBlock3D returns a tuple, and its default `encoder.layer4` matches no module)."""
    bb = backbone_of(model)
    nl = len(bb.features) - 1
    if isinstance(bb, UNet3D):
        return (["init_conv"] + [f"encoders.{i}.conv" for i in range(nl)]
                + [f"decoders.{j}{s}" for j in range(nl) for s in ("", ".conv")])
    names = []
    for m in range(bb.num_modalities):
        names += [f"encoders.{m}.init_conv"] + [f"encoders.{m}.blocks.{i}.conv" for i in range(nl)]
    return names + [f"decoder.{j}{s}" for j in range(nl) for s in ("", ".conv")]


def check_layer(model: nn.Module, name: str) -> str:
    """The layer's name relative to the backbone; ValueError listing the valid names otherwise."""
    n = name[len("backbone."):] if name.startswith("backbone.") else name
    valid = valid_layers(model)
    if n not in valid:
        raise ValueError(f"unknown explainability layer {name!r}; valid names (with or without a 'backbone.' "
                         f"prefix): {', '.join(valid)}")
    return n


def default_layer(model: nn.Module) -> str:
    """The bottleneck: the deepest encoder block of UNet3D, the first decoder block of DualEncoder."""
    bb = backbone_of(model)
    return f"encoders.{len(bb.features) - 2}.conv" if isinstance(bb, UNet3D) else "decoder.0"


def check_call(input_tensor: torch.Tensor, target_class: Optional[int], n_classes: int) -> int:
    if target_class is None:
        raise ValueError("target_class is required for volumetric outputs (the reference's argmax default yields "
                         "one class per voxel and fails there too)")
    if input_tensor.dim() != 5 or input_tensor.shape[0] != 1:
        raise ValueError(f"one sample per call: input [1, C, H, W, D], got {tuple(input_tensor.shape)}")
    c = int(target_class)
    if not 0 <= c < n_classes:
        raise ValueError(f"target_class {c} outside [0, {n_classes})")
    return c


def model_device(bb: nn.Module) -> torch.device:
    return next(bb.parameters()).device


# ------------------------------------------------------------------ HIP path
def engine_of(bb: nn.Module):
    from ..engine.engine import SegEngine
    eng = bb.__dict__.get("_engine")
    if eng is None:
        eng = SegEngine(bb, "unet" if isinstance(bb, UNet3D) else "dual_encoder")
        bb.__dict__["_engine"] = eng
    return eng


def _lib():
    from .._lib import lib, stream_handle
    return lib(), stream_handle()


def seed_fn(cls: int, mode: int):
    """logits -> the dense seed gradient of logits[0, cls].max() / .mean() (mmseg_explain_seed)."""
    def fn(logits: torch.Tensor) -> torch.Tensor:
        L, s = _lib()
        C, V = logits.shape[1], logits[0, 0].numel()
        out = torch.empty_like(logits)
        ws = torch.empty(L.mmseg_explain_ws_floats(), dtype=torch.float32, device=logits.device)
        L.mmseg_explain_seed(logits.data_ptr(), C, V, cls, mode, out.data_ptr(), ws.data_ptr(), s)
        return out
    return fn


def cam_weights(tap, mode: int) -> torch.Tensor:
    """Per-channel weights [C] of a tapped layer (mmseg_cam_weights)."""
    from .._lib import DTYPE_CODE
    L, s = _lib()
    d, h, w = tap.dims
    g = tap.grad
    dev = tap.act.device
    out = torch.empty(tap.C, dtype=torch.float32, device=dev)
    ws = torch.empty(L.mmseg_cam_ws_floats(d * h * w, tap.C), dtype=torch.float32, device=dev)
    pd = g.pool_dy
    L.mmseg_cam_weights(tap.act.data_ptr(), tap.C, g.p1.ptr if g.p1 is not None else None,
                        g.p1.ld if g.p1 is not None else 0, g.scale1, pd.ptr if pd is not None else None,
                        pd.ld if pd is not None else 0, g.pool_idx.data_ptr() if pd is not None else None, d, h, w,
                        tap.C, mode, out.data_ptr(), ws.data_ptr(), DTYPE_CODE[tap.act.dtype], s)
    return out


def cam_map(tap, mode: int, size: Tuple[int, int, int]) -> torch.Tensor:
    """The normalised heat map [size] of a tapped layer: weights, relu(sum_c w_c A_c), trilinear upsample, min-max
    normalisation -- all on the device."""
    from .._lib import DTYPE_CODE
    L, s = _lib()
    d, h, w = tap.dims
    dev = tap.act.device
    wts = cam_weights(tap, mode)
    cam = torch.empty(d * h * w, dtype=torch.float32, device=dev)
    L.mmseg_cam_combine(tap.act.data_ptr(), tap.C, wts.data_ptr(), d * h * w, tap.C, cam.data_ptr(),
                        DTYPE_CODE[tap.act.dtype], s)
    out = torch.empty(size, dtype=torch.float32, device=dev)
    ws = torch.empty(L.mmseg_explain_ws_floats(), dtype=torch.float32, device=dev)
    L.mmseg_cam_upsample_norm(cam.data_ptr(), d, h, w, out.data_ptr(), *size, ws.data_ptr(), s)
    return out
