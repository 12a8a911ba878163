"""GradCAM / GradCAMPlusPlus with the reference's call signatures (gradcam.py:21-247).

HIP backend: one SegEngine.explain call (eval forward, data-only backward of the seed d logits[0, c].max(), the
layer's activation and gradient sources) and the kernels of csrc/explain.hip; only the final map leaves the device.
Torch backend: the reference algorithm through a forward hook on `torch_forward`."""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import common as X


class GradCAM:
    mode = X.CAM

    def __init__(self, model: nn.Module, target_layers: List[str], use_cuda: bool = True):
        self.model = model
        self.backbone = X.backbone_of(model)
        self.target_layers = list(target_layers)
        if not self.target_layers:
            raise ValueError("target_layers is empty")
        for name in self.target_layers:
            X.check_layer(model, name)
        self.use_cuda = use_cuda and torch.cuda.is_available()

    def __call__(self, input_tensor: torch.Tensor, target_class: Optional[int] = None,
                 target_layer: Optional[str] = None) -> np.ndarray:
        """Heat map [H, W, D] (the input's spatial axes) in [0, 1], float32."""
        bb = self.backbone
        cls = X.check_call(input_tensor, target_class, bb.out_channels)
        layer = X.check_layer(self.model, target_layer if target_layer is not None else self.target_layers[0])
        dev = X.model_device(bb)
        x = input_tensor.detach().to(dev)
        if bb.kernels == "hip":
            res = X.engine_of(bb).explain(x, X.seed_fn(cls, X.SEED_MAX), taps=[layer])
            cam = X.cam_map(res.taps[layer], self.mode, tuple(x.shape[2:]))
            return cam.cpu().numpy()
        return self._torch_cam(x.to(next(bb.parameters()).dtype), cls, layer)

    # ------------------------------------------------------------- torch backend
    def _weights(self, act: torch.Tensor, grad: torch.Tensor) -> torch.Tensor:
        return grad.mean(dim=(2, 3, 4), keepdim=True)                      # gradcam.py:112-116

    def _torch_cam(self, x: torch.Tensor, cls: int, layer: str) -> np.ndarray:
        bb = self.backbone
        module = dict(bb.named_modules())[layer]
        kept = {}
        handle = module.register_forward_hook(lambda m, i, o: kept.__setitem__("act", o))
        was_training = bb.training
        bb.eval()
        try:
            with torch.enable_grad():
                out = bb.torch_forward(x)
                act = kept["act"]
                grad, = torch.autograd.grad(out[0, cls].max(), act)       # (no parameter gradient is formed)
        finally:
            handle.remove()
            bb.train(was_training)
        act = act.detach()
        cam = F.relu((self._weights(act, grad) * act).sum(dim=1, keepdim=True))
        cam = F.interpolate(cam, size=x.shape[2:], mode="trilinear", align_corners=False)[0, 0]
        cam = cam.cpu().numpy()
        cam = (cam - cam.min()) / (cam.max() - cam.min() + 1e-8)
        return cam.astype(np.float32)


class GradCAMPlusPlus(GradCAM):
    mode = X.CAM_PP

    def _weights(self, act: torch.Tensor, grad: torch.Tensor) -> torch.Tensor:
        g2, g3 = grad ** 2, grad ** 3                                      # gradcam.py:200-221
        alpha = g2 / (2 * g2 + act.sum(dim=(2, 3, 4), keepdim=True) * g3 + 1e-8)
        return (alpha * F.relu(grad)).sum(dim=(2, 3, 4), keepdim=True)
