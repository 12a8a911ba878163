"""Independent torch restatement of the three explainability algorithms (reference src/explainability/gradcam.py:61-247,
shap_analysis.py:63-165), for any module through hooks, in the dtype of the model it is given.  `forward` is the
callable that runs the network (a model, or a backbone's torch_forward)."""
import numpy as np
import torch
import torch.nn.functional as F


def tapped(module_root, forward, layer, x, score):
    """(activation, gradient of score(output) with respect to it, output) of the named module's output."""
    mod = dict(module_root.named_modules())[layer]
    box = {}

    def hook(m, i, o):
        box["a"] = o
    h = mod.register_forward_hook(hook)
    try:
        with torch.enable_grad():
            out = forward(x)
            score(out).backward(inputs=[box["a"]])        # (no parameter gradient is formed)
    finally:
        h.remove()
    return box["a"].detach(), box["a"].grad.detach(), out.detach()


def cam(module_root, forward, layer, x, cls, plus_plus=False):
    a, g, _ = tapped(module_root, forward, layer, x, lambda o: o[0, cls].max())
    if plus_plus:
        g2 = g * g
        alpha = g2 / (2 * g2 + a.sum(dim=(2, 3, 4), keepdim=True) * g2 * g + 1e-8)
        w = (alpha * g.clamp(min=0)).sum(dim=(2, 3, 4), keepdim=True)
    else:
        w = g.mean(dim=(2, 3, 4), keepdim=True)
    m = (w * a).sum(dim=1, keepdim=True).clamp(min=0)
    m = F.interpolate(m, size=x.shape[2:], mode="trilinear", align_corners=False)[0, 0].cpu().numpy()
    return (m - m.min()) / (m.max() - m.min() + 1e-8)


def input_grad(forward, x, cls):
    x = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        g, = torch.autograd.grad(forward(x)[0, cls].mean(), x)
    return g


def gradient_shap(forward, x, cls, background=None):
    base = background.mean(dim=0, keepdim=True) if background is not None else torch.zeros_like(x)
    return (input_grad(forward, x, cls) * (x - base))[0].cpu().numpy()


def integrated_gradients(forward, x, cls, background=None, n_steps=50):
    base = background.mean(dim=0, keepdim=True) if background is not None else torch.zeros_like(x)
    grads = [input_grad(forward, base + (float(i) / n_steps) * (x - base), cls) for i in range(n_steps + 1)]
    return ((x - base) * torch.stack(grads).mean(dim=0))[0].cpu().numpy()


def dense_grad(p1, scale1, pool_dy, pool_idx):
    """The gradient a DySpec stands for, dense [1, C, D, H, W]: scale1 * p1 plus the max-pool scatter of pool_dy
    [1, C, D/2, H/2, W/2] through the engine's argmax codes pool_idx [Vo][C] (code = (z&1)<<2 | (y&1)<<1 | x&1)."""
    g = p1.double() * scale1
    if pool_dy is not None:
        _, C, Do, Ho, Wo = pool_dy.shape
        code = pool_idx.view(Do, Ho, Wo, C).permute(3, 0, 1, 2).long()
        for sub in range(8):
            dz, dy, dx = (sub >> 2) & 1, (sub >> 1) & 1, sub & 1
            g[0, :, dz::2, dy::2, dx::2] += pool_dy[0].double() * (code == sub)
    return g
