"""SHAPAnalyzer with the reference's call signatures (shap_analysis.py:21-165): gradient x (input - baseline) and
integrated gradients of mean(output[0, c]).

HIP backend: the input gradient comes from SegEngine.explain (data-only backward + mmseg_stem_dgrad); the path
points and the final product are mmseg_attr_lerp / mmseg_attr_finish, and the n_steps + 1 gradients of integrated
gradients are summed on the device by the stem data gradient's accumulate flag.  Torch backend: autograd on
`torch_forward`.

A constant baseline (the zero default) meets InstanceNorm with zero variance: integrated gradients is then
ill-conditioned on these networks, so pass `background_samples` for that method."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import common as X


class SHAPAnalyzer:
    def __init__(self, model: nn.Module, background_samples: Optional[torch.Tensor] = None, n_samples: int = 100):
        self.model = model
        self.backbone = X.backbone_of(model)
        self.background = background_samples
        self.n_samples = n_samples

    def compute_shap_values(self, input_tensor: torch.Tensor, target_class: Optional[int] = None,
                            method: str = "gradient", n_steps: int = 50) -> np.ndarray:
        """Attributions [C_in, H, W, D], float32.  method: 'gradient' (also the reference's fallback for any other
        name) or 'integrated_gradients' (n_steps + 1 points on the line baseline -> input)."""
        bb = self.backbone
        cls = X.check_call(input_tensor, target_class, bb.out_channels)
        steps = int(n_steps) if method == "integrated_gradients" else 0
        if method == "integrated_gradients" and steps < 1:
            raise ValueError("n_steps must be at least 1")
        dev = X.model_device(bb)
        x = input_tensor.detach().to(dev)
        base = None
        if self.background is not None:
            base = self.background.detach().to(dev).to(x.dtype).mean(dim=0, keepdim=True)
            if base.shape != x.shape:
                raise ValueError(f"background samples {tuple(self.background.shape)} do not match the input "
                                 f"{tuple(x.shape)}")
        if bb.kernels == "hip":
            return self._hip(x.float().contiguous(), None if base is None else base.float().contiguous(), cls, steps)
        dt = next(bb.parameters()).dtype
        return self._torch(x.to(dt), None if base is None else base.to(dt), cls, steps)

    def _hip(self, x, base, cls, steps) -> np.ndarray:
        from .._lib import lib, stream_handle
        L, eng = lib(), X.engine_of(self.backbone)
        n, bptr = x.numel(), (base.data_ptr() if base is not None else None)
        kept = {}
        mean_seed = X.seed_fn(cls, X.SEED_MEAN)

        def seed(logits):            # 1 / V on the class: the same tensor at every path point
            if "g" not in kept:
                kept["g"] = mean_seed(logits)
            return kept["g"]
        out = torch.empty_like(x)
        if steps == 0:
            dx = eng.explain(x, seed, input_grad=True).dx
            L.mmseg_attr_finish(x.data_ptr(), bptr, dx.data_ptr(), 1.0, out.data_ptr(), n, stream_handle())
            return out[0].cpu().numpy()
        xt, dx = torch.empty_like(x), torch.empty_like(x)
        for i in range(steps + 1):
            L.mmseg_attr_lerp(x.data_ptr(), bptr, float(i) / steps, xt.data_ptr(), n, stream_handle())
            eng.explain(xt, seed, input_grad=True, dx=dx, accumulate=i > 0)
        L.mmseg_attr_finish(x.data_ptr(), bptr, dx.data_ptr(), 1.0 / (steps + 1), out.data_ptr(), n, stream_handle())
        return out[0].cpu().numpy()

    def _torch(self, x, base, cls, steps) -> np.ndarray:
        bb = self.backbone
        if base is None:
            base = torch.zeros_like(x)
        points = [x] if steps == 0 else [base + (float(i) / steps) * (x - base) for i in range(steps + 1)]
        was_training = bb.training
        bb.eval()
        try:
            grads = []
            for p in points:
                p = p.detach().clone().requires_grad_(True)
                with torch.enable_grad():
                    g, = torch.autograd.grad(bb.torch_forward(p)[0, cls].mean(), p)
                grads.append(g)
        finally:
            bb.train(was_training)
        attr = (x - base) * torch.stack(grads).mean(dim=0)
        return attr[0].cpu().numpy().astype(np.float32)
