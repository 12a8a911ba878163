"""CPU restatement of weighted sliding-window blending and flip test-time augmentation, in plain torch and
without any package code (the second statement of DESIGN.md "Sliding-window inference"; MONAI is absent,
so parity against MONAI itself is unpinned).

importance_map : MONAI 1.3 compute_importance_map(mode="gaussian") with the 3-D map materialised and clamped
sliding_window : pad, windows in MONAI's order, out[idx] += w * pred, count[idx] += w, out / count, crop
tta_predictor  : torch.flip around the predictor, the sum over the 2 ** len(axes) mirrored passes written out

The predictor is called on its own device (as oracle/mmseg_oracle.py's restatement does); the blending runs
on the CPU, where torch's fp32 multiply and add are two rounded operations.
"""
import math

import torch
import torch.nn.functional as F


def gaussian_axis(r, sigma_scale):
    sigma = r * sigma_scale
    x = torch.arange(-(r - 1) / 2.0, (r - 1) / 2.0 + 1, dtype=torch.float32)
    return torch.exp(x ** 2 / (-2 * sigma ** 2))


def importance_map(roi, blend="constant", sigma_scale=0.125):
    """[r0, r1, r2] fp32 window weights: ones, or the clamped Gaussian."""
    if blend == "constant":
        return torch.ones(*roi, dtype=torch.float32)
    g = [gaussian_axis(r, sigma_scale) for r in roi]
    w = (g[0][:, None, None] * g[1][None, :, None]) * g[2][None, None, :]
    m = max(torch.min(w).item(), 1e-3)
    return torch.clamp(w, min=torch.tensor(m, dtype=torch.float32).item())


def flip_sets(tta_flips):
    """Entry m of the 2 ** len(A) passes mirrors axis A[k] of (D, H, W) when bit k of m is set, A sorted."""
    A = sorted(tta_flips)
    return [[A[k] for k in range(len(A)) if (m >> k) & 1] for m in range(2 ** len(A))]


def tta_predictor(predictor, tta_flips):
    sets = flip_sets(tta_flips)

    def first(t):
        return (t[0] if isinstance(t, (tuple, list)) else t).float()

    def wrapped(batch):
        acc = first(predictor(batch))
        for axes in sets[1:]:
            dims = [a + 2 for a in axes]
            acc = acc + torch.flip(first(predictor(torch.flip(batch, dims))), dims)
        return acc / len(sets)
    return wrapped


def window_starts(psize, roi, overlap):
    starts = []
    for d in range(3):
        interval = roi[d] if roi[d] == psize[d] else max(int(roi[d] * (1 - overlap)), 1)
        num = int(math.ceil(float(psize[d]) / interval))
        scan = next((i for i in range(num) if i * interval + roi[d] >= psize[d]), None)
        cnt = scan + 1 if scan is not None else 1
        starts.append([i * interval - max(i * interval + roi[d] - psize[d], 0) for i in range(cnt)])
    return starts


def sliding_window(inputs, roi_size, sw_batch_size, predictor, overlap=0.25, blend="constant", sigma_scale=0.125,
                   tta_flips=()):
    """inputs [N, M, D, H, W] (any device) -> blended logits [N, C, D, H, W] on the CPU."""
    if len(tuple(tta_flips)):
        predictor = tta_predictor(predictor, tta_flips)
    N = inputs.shape[0]
    size = list(inputs.shape[2:])
    roi = [r if r > 0 else s for r, s in zip(roi_size, size)]
    pad = []
    for k in (2, 1, 0):                                  # F.pad order: last dim first
        diff = max(roi[k] - size[k], 0)
        pad += [diff // 2, diff - diff // 2]
    x = F.pad(inputs.float().cpu(), pad, mode="constant", value=0.0)
    psize = list(x.shape[2:])
    starts = window_starts(psize, roi, overlap)
    wins = [(n, a, b, c) for n in range(N) for a in starts[0] for b in starts[1] for c in starts[2]]
    w = importance_map(roi, blend, sigma_scale)
    out = count = None
    for b0 in range(0, len(wins), sw_batch_size):
        chunk = wins[b0:b0 + sw_batch_size]
        batch = torch.stack([x[n, :, a:a + roi[0], b:b + roi[1], c:c + roi[2]] for n, a, b, c in chunk])
        pred = predictor(batch.to(inputs.device))
        pred = (pred[0] if isinstance(pred, (tuple, list)) else pred).float().cpu()
        if out is None:
            out = torch.zeros(N, pred.shape[1], *psize)
            count = torch.zeros(N, 1, *psize)
        for k, (n, a, b, c) in enumerate(chunk):
            out[n, :, a:a + roi[0], b:b + roi[1], c:c + roi[2]] += w * pred[k]
            count[n, :, a:a + roi[0], b:b + roi[1], c:c + roi[2]] += w
    out = out / count
    lo = [pad[4], pad[2], pad[0]]
    return out[:, :, lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]].contiguous()
