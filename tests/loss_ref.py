"""Plain torch fp64 restatement of the segmentation losses and of the 1x1 head in front of them, the checker of the
loss / fused head + loss kernel tests (csrc/loss_head.hip).  Written from the formulas:

  p = softmax_C(z), t = one-hot(y); per (n, c): P = sum_v p, I = sum_v p t, T = sum_v t
  Dice     1 - (2 I + s) / (P + T + s), mean over N * (C - c0) entries (c0 = 1 without the background class)
  Tversky  1 - (I + s) / (I + a (P - I) + b (T - I) + s), mean over N * C entries
  CE       sum_v w_y (lse - z_y) / sum_v w_y
  Focal    ce_v = w_y (lse - z_y); mean_v (1 - exp(-ce_v))^gamma ce_v   (gamma rides in spec["alpha"])
  loss = dice_w * region + ce_w * CE

Label rules (label_state in loss_head.hip): a label in [0, C) is valid.  -100 is *ignored* by pure CE (region weight
0: no term, not in the denominator) and by focal (no term, but the plain mean still counts the voxel).  Every other
label outside [0, C) -- and -100 under a region loss -- is *invalid*: the loss is NaN and the voxel is counted.
Gradients come from autograd; tests/test_loss_ref_cpu.py pins all of it against the reference-produced golden losses
and against torch's own cross_entropy."""
import torch

TYPE_DICE, TYPE_TVERSKY, TYPE_FOCAL = 0, 1, 2


def label_masks(labels, C, spec):
    """(valid, ignored, invalid) boolean masks of `labels` under `spec`."""
    y = labels.long()
    valid = (y >= 0) & (y < C)
    skips = (spec["type"] == TYPE_DICE and spec["dice_w"] == 0.0) or spec["type"] == TYPE_FOCAL
    ignored = (y == -100) & ~valid if skips else torch.zeros_like(valid)
    return valid, ignored, ~valid & ~ignored


def loss_ref(logits64, labels, spec, class_w=None):
    """The loss scalar (fp64, differentiable in logits64) of logits64 [N, C, ...] and labels [N, ...]; NaN when a
    label is invalid."""
    N, C = logits64.shape[:2]
    z = logits64.double().reshape(N, C, -1)
    y = labels.long().reshape(N, -1)
    valid, ignored, invalid = label_masks(y, C, spec)
    if invalid.any():
        return torch.full((), float("nan"), dtype=torch.float64)
    m = valid.double()
    ys = torch.where(valid, y, torch.zeros_like(y))
    t = torch.zeros(N, C, y.shape[1], dtype=torch.float64).scatter_(1, ys[:, None], 1.0) * m[:, None]
    logp = torch.log_softmax(z, dim=1)
    w = torch.ones(C, dtype=torch.float64) if class_w is None else class_w.double().cpu()
    wy = w[ys] * m
    nll = -(logp * t).sum(1)                      # lse - z_y at valid voxels, 0 elsewhere
    loss = torch.zeros((), dtype=torch.float64)
    if spec["dice_w"] != 0.0:
        p = logp.exp() * m[:, None]
        P, I, T = p.sum(-1), (p * t).sum(-1), t.sum(-1)
        s = float(spec["smooth"])
        if spec["type"] == TYPE_TVERSKY:
            a, b = float(spec["alpha"]), float(spec["beta"])
            region = 1.0 - (I + s) / (I + a * (P - I) + b * (T - I) + s)
        else:
            region = 1.0 - (2.0 * I + s) / (P + T + s)
            if not spec["include_bg"]:
                region = region[:, 1:]
        loss = loss + float(spec["dice_w"]) * region.mean()
    if spec["ce_w"] != 0.0:
        if spec["type"] == TYPE_FOCAL:
            ce = wy * nll
            focal = (-torch.expm1(-ce)) ** float(spec["alpha"]) * ce
            term = focal.sum() / (valid | ignored).sum()
        else:
            term = (wy * nll).sum() / wy.sum()
        loss = loss + float(spec["ce_w"]) * term
    return loss


def head_input(x, norm, dtype):
    """The head's input h [N, Cin, D, H, W] as the kernels see it, in fp64: x rounded through the storage dtype or,
    with norm = (mean, rstd) [N, Cin], relu((x - mean) * rstd) in float32 (a subtraction, then a multiplication:
    HeadLoad::norm) rounded to the storage dtype."""
    xq = x.detach().cpu().to(dtype)
    if norm is None:
        return xq.double()
    mean, rstd = (s.detach().cpu().float()[:, :, None, None, None] for s in norm)
    h = xq.float() - mean
    h = h * rstd
    return torch.relu(h).to(dtype).double()


def head_loss_ref(x, W, b, dscale, norm, labels, spec, class_w, dtype, gout=1.0):
    """Dropout3d scale (dscale [N, Cin] or None) + 1x1 head (W [C, Cin], b [C]) + loss on h = head_input(x, norm,
    dtype).  Returns (loss, d/dh, dW, db), the gradients of gout * loss; d/dh is what the fused backward writes to
    dx (with the deferred norm: the gradient at the head's input, the norm's output)."""
    h = head_input(x, norm, dtype).requires_grad_(True)
    Wd = W.detach().cpu().double().reshape(W.shape[0], -1).requires_grad_(True)
    bd = b.detach().cpu().double().requires_grad_(True)
    hs = h if dscale is None else h * dscale.detach().cpu().double()[:, :, None, None, None]
    logits = torch.einsum("ncdhw,kc->nkdhw", hs, Wd) + bd[None, :, None, None, None]
    loss = loss_ref(logits, labels.cpu(), spec, class_w)
    if torch.isnan(loss):
        return loss.detach(), None, None, None
    (loss * gout).backward()
    return loss.detach(), h.grad, Wd.grad, bd.grad
