"""Sliding-window inference on device — the reference's Trainer._sliding_window_inference
(trainer.py:370-395) calls MONAI's `sliding_window_inference(image, roi_size, sw_batch_size,
predictor, overlap)` with the config's inference block (configs/default.yaml:127-133).  MONAI is
absent from this image, so its published algorithm (MONAI 1.3,
monai/inferers/utils.py sliding_window_inference, monai/data/utils.py dense_patch_slices) is
restated here for the arguments the reference passes: `mode` is not passed, so blending is
"constant" (the YAML's "gaussian" is dead config); padding is zeros.

Window cutting, accumulation and normalisation are HIP kernels (csrc/inference.hip); the
predictor is the engine model.  Windows are accumulated one at a time in MONAI's order, so each
output voxel is the same fp32 sum MONAI forms (parity is checked against the CPU restatement in
oracle/mmseg_oracle.py; against MONAI itself it is unpinned).

Two opt-in options the reference's YAML names but never passes (DESIGN.md "Sliding-window inference"):
`blend="gaussian"` weights each window by MONAI 1.3's compute_importance_map, and `tta_flips` averages
the logits over the mirrored copies of every window batch.  Either one takes the batched path: one
blend launch per predictor batch into `out` and a real `count` volume, then out / count.  The defaults
run exactly the calls above.
"""
from __future__ import annotations

import math
from typing import Callable, List, Sequence, Tuple

import torch

from .._lib import lib, ptr, stream_handle


def window_starts(size: int, roi: int, overlap: float) -> Tuple[List[int], int]:
    """Window starts along one axis in MONAI's padded frame, and the padding before it.
    (_get_scan_interval + dense_patch_slices of MONAI 1.3, one dimension.)"""
    padded = max(size, roi)
    pad_before = (padded - size) // 2
    if roi == padded:
        interval = roi
    else:
        interval = max(int(roi * (1 - overlap)), 1)
    num = int(math.ceil(float(padded) / interval))
    scan = next((d for d in range(num) if d * interval + roi >= padded), None)
    count = scan + 1 if scan is not None else 1
    starts = []
    for i in range(count):
        s = i * interval
        s -= max(s + roi - padded, 0)
        starts.append(s)
    return starts, pad_before


def _coverage(size: int, starts: List[int], pad_before: int, roi: int) -> torch.Tensor:
    c = torch.zeros(size, dtype=torch.float32)
    for s in starts:
        lo, hi = max(s - pad_before, 0), min(s - pad_before + roi, size)
        c[lo:hi] += 1.0
    return c


def gaussian_tables(roi: Sequence[int], sigma_scale: float = 0.125) -> Tuple[List[torch.Tensor], float]:
    """MONAI 1.3 compute_importance_map(mode="gaussian") as three per-axis tables and the clamp value:
    w[z, y, x] = max((g0[z] * g1[y]) * g2[x], m) with m = max(min(w), 1e-3) rounded to float32.  Every op is
    torch float32 on the host; fp32 rounding is monotone, so min(w) is the corner product and the 3-D map is
    never materialised."""
    if not sigma_scale > 0:
        raise ValueError("sigma_scale must be positive")
    tables = []
    for r in roi:
        sigma = r * sigma_scale
        x = torch.arange(-(r - 1) / 2.0, (r - 1) / 2.0 + 1, dtype=torch.float32)
        tables.append(torch.exp(x ** 2 / (-2 * sigma ** 2)))
    corner = (tables[0][0] * tables[1][0]) * tables[2][0]
    m = max(corner.item(), 1e-3)
    return tables, torch.tensor(m, dtype=torch.float32).item()


def flip_masks(tta_flips: Sequence[int]) -> List[int]:
    """The flip masks of test-time augmentation in the order they are summed: with A = sorted(tta_flips), entry m
    of the 2 ** len(A) mirrors axis A[k] (0, 1, 2 = D, H, W) when bit k of m is set.  Returned as kernel masks
    (bit d = axis d); entry 0 is the unflipped pass."""
    axes = list(tta_flips)
    if any(not isinstance(a, int) or isinstance(a, bool) or a < 0 or a > 2 for a in axes) or len(set(axes)) != len(axes):
        raise ValueError(f"tta_flips must be distinct axes out of 0, 1, 2 (got {axes})")
    A = sorted(axes)
    return [sum(1 << A[k] for k in range(len(A)) if (m >> k) & 1) for m in range(2 ** len(A))]


def _check_options(overlap: float, blend: str, sigma_scale: float, tta_flips: Sequence[int]) -> List[int]:
    if not 0 <= overlap < 1:
        raise ValueError("overlap must be >= 0 and < 1")
    if blend not in ("constant", "gaussian"):
        raise ValueError(f"blend must be 'constant' or 'gaussian' (got {blend!r})")
    if not sigma_scale > 0:
        raise ValueError("sigma_scale must be positive")
    return flip_masks(tta_flips)


def _windows(N: int, dims, roi, overlap: float):
    axes = [window_starts(s, r, overlap) for s, r in zip(dims, roi)]
    wins = []
    for n in range(N):                          # MONAI: windows image-major, then meshgrid "ij" order
        for z in axes[0][0]:
            for y in axes[1][0]:
                for xx in axes[2][0]:
                    wins.append((n, z - axes[0][1], y - axes[1][1], xx - axes[2][1]))
    return axes, wins


def sliding_window_accumulate(inputs: torch.Tensor, roi_size: Sequence[int], sw_batch_size: int,
                              predictor: Callable[[torch.Tensor], torch.Tensor], overlap: float = 0.25,
                              blend: str = "constant", sigma_scale: float = 0.125,
                              tta_flips: Sequence[int] = ()) -> Tuple[torch.Tensor, torch.Tensor]:
    """The batched path up to the division: (out [N, C, D, H, W], count [N, D, H, W]) with
    out = sum of w * pred and count = sum of w over the windows in MONAI's order.  pred is the predictor's
    output, or with tta_flips the mean of the un-flipped outputs over flip_masks(tta_flips)."""
    if inputs.dim() != 5 or inputs.device.type != "cuda":
        raise RuntimeError("sliding_window_inference runs on the ROCm device, input [N, M, D, H, W]")
    masks = _check_options(overlap, blend, sigma_scale, tta_flips)
    x = inputs.float().contiguous()
    N, M, D, H, W = x.shape
    roi = [r if r > 0 else s for r, s in zip(roi_size, (D, H, W))]     # fall_back_tuple
    _, wins = _windows(N, (D, H, W), roi, overlap)
    L, s = lib(), stream_handle()
    dev = x.device
    win_host = torch.tensor(wins, dtype=torch.int32).reshape(-1)
    win_dev = win_host.to(dev)
    gauss = blend == "gaussian"
    if gauss:
        tables, wmin = gaussian_tables(roi, sigma_scale)
        tables = [t.to(dev) for t in tables]
    else:
        tables, wmin = [None, None, None], 0.0
    out = count = acc = None
    for b0 in range(0, len(wins), sw_batch_size):
        nb = min(sw_batch_size, len(wins) - b0)
        batch = torch.empty(nb, M, *roi, dtype=torch.float32, device=dev)
        for i, mask in enumerate(masks):
            L.mmseg_window_gather_flip(ptr(x), N, M, D, H, W, ptr(win_dev) + 16 * b0, nb, roi[0], roi[1], roi[2], mask,
                                       ptr(batch), s)
            logits = predictor(batch)
            if isinstance(logits, (tuple, list)):
                logits = logits[0]
            logits = logits.float().contiguous()
            if len(masks) == 1:
                break
            if i == 0:
                acc = torch.empty_like(logits)
            L.mmseg_tta_accum(ptr(logits), nb * logits.shape[1], roi[0], roi[1], roi[2], mask, int(i == 0),
                              1.0 / len(masks) if i == len(masks) - 1 else 1.0, ptr(acc), s)
        pred = logits if len(masks) == 1 else acc
        if out is None:
            C = pred.shape[1]
            out = torch.zeros(N, C, D, H, W, dtype=torch.float32, device=dev)
            count = torch.zeros(N, D, H, W, dtype=torch.float32, device=dev)
        L.mmseg_window_blend(ptr(pred), N, C, D, H, W, win_host.data_ptr() + 16 * b0, nb, roi[0], roi[1], roi[2],
                             int(gauss), ptr(tables[0]), ptr(tables[1]), ptr(tables[2]), wmin, ptr(out), ptr(count), s)
    return out, count


def blend_argmax_encode(out: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
    """One volume's accumulators (out [C, X, Y, Z], count [X, Y, Z], fp32 on the device) -> the class mask of
    out / count as X*Y*Z uint8 in NIfTI file order (x fastest): data.nifti.argmax_encode of the finished logits,
    bit for bit, without writing them."""
    if out.device.type != "cuda" or count.device != out.device:
        raise RuntimeError("blend_argmax_encode runs on the ROCm device")
    if out.dim() != 4 or out.dtype != torch.float32 or count.dtype != torch.float32 or count.shape != out.shape[1:]:
        raise ValueError("blend_argmax_encode: out [C, X, Y, Z] and count [X, Y, Z] float32")
    out, count = out.contiguous(), count.contiguous()
    C, X, Y, Z = out.shape
    mask = torch.empty(X * Y * Z, dtype=torch.uint8, device=out.device)
    lib().mmseg_blend_argmax_encode(ptr(out), ptr(count), C, X, Y, Z, ptr(mask), stream_handle())
    return mask


def sliding_window_inference(inputs: torch.Tensor, roi_size: Sequence[int], sw_batch_size: int,
                             predictor: Callable[[torch.Tensor], torch.Tensor], overlap: float = 0.25,
                             blend: str = "constant", sigma_scale: float = 0.125,
                             tta_flips: Sequence[int] = ()) -> torch.Tensor:
    """inputs [N, M, D, H, W] fp32 on the device -> [N, C, D, H, W] fp32 (MONAI semantics).  blend "constant"
    with no tta_flips is MONAI's default call; "gaussian" (sigma_scale) and tta_flips (axes out of 0, 1, 2 =
    D, H, W) are the opt-in batched path."""
    masks = _check_options(overlap, blend, sigma_scale, tta_flips)
    if blend != "constant" or len(masks) > 1:
        out, count = sliding_window_accumulate(inputs, roi_size, sw_batch_size, predictor, overlap, blend,
                                               sigma_scale, tta_flips)
        N, C = out.shape[:2]
        lib().mmseg_window_finish(ptr(out), ptr(count), N, C, count[0].numel(), stream_handle())
        return out
    if inputs.dim() != 5 or inputs.device.type != "cuda":
        raise RuntimeError("sliding_window_inference runs on the ROCm device, input [N, M, D, H, W]")
    x = inputs.float().contiguous()
    N, M, D, H, W = x.shape
    dims = (D, H, W)
    roi = [r if r > 0 else s for r, s in zip(roi_size, dims)]     # fall_back_tuple
    axes, wins = _windows(N, dims, roi, overlap)
    L, s = lib(), stream_handle()
    dev = x.device
    win_dev = torch.tensor(wins, dtype=torch.int32).reshape(-1).to(dev)
    out = None
    C = None
    rv = roi[0] * roi[1] * roi[2]
    for b0 in range(0, len(wins), sw_batch_size):
        nb = min(sw_batch_size, len(wins) - b0)
        batch = torch.empty(nb, M, *roi, dtype=torch.float32, device=dev)
        L.mmseg_window_gather(ptr(x), N, M, D, H, W, ptr(win_dev) + 16 * b0, nb, roi[0], roi[1], roi[2], ptr(batch), s)
        logits = predictor(batch)
        if isinstance(logits, (tuple, list)):
            logits = logits[0]
        logits = logits.float().contiguous()
        if out is None:
            C = logits.shape[1]
            out = torch.zeros(N, C, D, H, W, dtype=torch.float32, device=dev)
        for k in range(nb):
            n, z0, y0, x0 = wins[b0 + k]
            L.mmseg_window_accum(ptr(logits) + 4 * k * C * rv, N, C, D, H, W, n, z0, y0, x0, roi[0], roi[1], roi[2],
                                 ptr(out), s)
    cov = [_coverage(sz, st, pb, r).to(dev) for sz, (st, pb), r in zip(dims, axes, roi)]
    L.mmseg_window_norm(ptr(out), N, C, D, H, W, ptr(cov[0]), ptr(cov[1]), ptr(cov[2]), s)
    return out
