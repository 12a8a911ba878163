"""Segmentation metrics on the MI355X engine — mirror of the reference's
DiceMetric (src/trainer/metrics.py:11-88), HausdorffDistance (91-162),
ConfusionMatrix (165-226) and get_metrics (229-244).

Counts are integer and exact on the device (mmseg_dice_counts*); each update's
counts are then added into fp32 accumulators exactly as the reference adds its
per-batch fp32 sums, so `compute()` is bit-identical to the reference's on the
same masks.  No per-batch host copy (the reference does .cpu() per update).

HausdorffDistance and ConfusionMatrix follow the same rule: `update` only
enqueues kernels (csrc/metrics.hip); `compute()` copies O(B) records (or the
C x C matrix) and finishes with the reference's own numpy arithmetic.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .._lib import lib, ptr, stream_handle


class DiceMetric:
    def __init__(self, num_classes: int, include_background: bool = False, reduction: str = "mean",
                 device: Optional[torch.device] = None):
        self.num_classes = num_classes
        self.include_background = include_background
        self.reduction = reduction
        self.device = device       # accumulators live here from the start (a rank with no batches still packs them)
        self.reset()

    def reset(self) -> None:
        self.intersection = torch.zeros(self.num_classes, device=self.device)
        self.union = torch.zeros(self.num_classes, device=self.device)
        self.count = 0
        self._counts: Optional[torch.Tensor] = None

    def _accumulate(self, counts: torch.Tensor) -> None:
        C = self.num_classes
        c = counts.to(torch.float32)
        if self.intersection.device != counts.device:
            self.intersection = self.intersection.to(counts.device)
            self.union = self.union.to(counts.device)
        self.intersection += c[:C]
        self.union += c[C:2 * C] + c[2 * C:]
        self.count += 1

    def _scratch(self, device) -> torch.Tensor:
        if self._counts is None or self._counts.device != device:
            self._counts = torch.zeros(3 * self.num_classes, dtype=torch.int64, device=device)
        else:
            self._counts.zero_()
        return self._counts

    def update(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        """pred / target: class-index masks [B, H, W, D] (reference metrics.py:42-67)."""
        if pred.device.type != "cuda":
            raise RuntimeError("HIP DiceMetric needs ROCm tensors; there is no CPU path")
        pred = pred.contiguous() if pred.dtype in (torch.int64, torch.uint8) else pred.long().contiguous()
        target = target.contiguous() if target.dtype in (torch.int64, torch.uint8) else target.long().contiguous()
        counts = self._scratch(pred.device)
        lib().mmseg_dice_counts_idx(ptr(pred), pred.element_size(), ptr(target), target.element_size(), pred.numel(),
                                    self.num_classes, ptr(counts), stream_handle())
        self._accumulate(counts)

    def update_from_logits(self, logits: torch.Tensor, target: torch.Tensor,
                           pred_out: Optional[torch.Tensor] = None) -> None:
        """Fused argmax(dim=1) + update (trainer.py:290-291) without materialising the mask; pred_out (optional,
        contiguous, target's dtype and shape) receives the argmax mask for the metrics that need it."""
        logits = logits.float().contiguous()
        target = target.contiguous() if target.dtype in (torch.int64, torch.uint8) else target.long().contiguous()
        N, C = logits.shape[:2]
        V = logits.numel() // (N * C)
        counts = self._scratch(logits.device)
        if pred_out is not None and (pred_out.dtype != target.dtype or pred_out.shape != target.shape
                                     or not pred_out.is_contiguous() or pred_out.device != logits.device):
            raise ValueError("pred_out must be a contiguous tensor of the target's dtype, shape and device")
        lib().mmseg_dice_counts(ptr(logits), ptr(target), target.element_size(), N, C, V, ptr(counts), ptr(pred_out),
                                stream_handle())
        self._accumulate(counts)

    def compute(self) -> Dict[str, Any]:
        smooth = 1e-5
        dpc = (2.0 * self.intersection.cpu() + smooth) / (self.union.cpu() + smooth)
        start = 0 if self.include_background else 1
        return {"dice": dpc[start:].mean().item(), "dice_per_class": dpc.tolist()}


def _index_mask(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous() if t.dtype in (torch.int64, torch.uint8) else t.long().contiguous()


# ------------------------------------------------------------------ percentile (host side, O(1) per sample)
def order_stat_indices(n: int, q: float) -> Tuple[int, int]:
    """(lo, hi): the two order statistics np.percentile(a, q) (method "linear") reads from n sorted values.
    numpy's virtual index is (n - 1) * (q / 100) -- the quotient first, in fp64 -- and at or above n - 1 it
    takes the last element for both."""
    vi = (n - 1) * np.true_divide(q, 100)
    if vi >= n - 1:
        return n - 1, n - 1
    lo = int(np.floor(vi))
    return lo, min(lo + 1, n - 1)


def percentile_from_order_stats(n: int, a_lo: float, a_hi: float, q: float) -> np.float64:
    """np.percentile(a, q) from n = len(a) and the two order statistics of order_stat_indices(n, q): numpy's
    gamma (virtual index minus the previous index, which is -1 in the "take the last element" case) and its
    _lerp, `t >= 0.5` branch included."""
    vi = np.float64((n - 1) * np.true_divide(q, 100))
    prev = np.float64(-1.0) if vi >= n - 1 else np.floor(vi)
    t = np.float64(vi - prev)
    a, b = np.float64(a_lo), np.float64(a_hi)
    diff = b - a
    if t >= 0.5:
        return b - diff * (1 - t)
    return a + diff * t


def percentile_linear(a: Sequence[float], q: float) -> np.float64:
    """np.percentile(a, q) through the two-order-statistic path the device takes (a sorted on the host here)."""
    srt = np.sort(np.asarray(a, dtype=np.float64))
    lo, hi = order_stat_indices(len(srt), q)
    return percentile_from_order_stats(len(srt), srt[lo], srt[hi], q)


def hd_moments(distances: Sequence[float]) -> np.ndarray:
    """[count, sum d, sum d^2] (fp64) of one rank's per-sample distances: what data parallelism all-reduces."""
    d = np.asarray(distances, dtype=np.float64)
    return np.array([float(d.size), d.sum(), (d * d).sum()], dtype=np.float64)


def hd_from_moments(m: Sequence[float]) -> Dict[str, float]:
    """HausdorffDistance.compute() from summed hd_moments.  The mean is sum / count and the std
    sqrt(sum d^2 / count - mean^2): equal to np.mean / np.std of the gathered list up to fp64 rounding
    (about 1e-15 relative for distances of comparable size), not bit-equal."""
    cnt, s1, s2 = float(m[0]), float(m[1]), float(m[2])
    if cnt == 0:
        return {"hausdorff_distance": float("inf")}
    mean = s1 / cnt
    return {"hausdorff_distance": mean, "hausdorff_distance_std": float(np.sqrt(max(s2 / cnt - mean * mean, 0.0)))}


def _spacing3(spacing) -> Tuple[float, float, float]:
    sp = tuple(float(x) for x in (spacing or (1.0, 1.0, 1.0)))
    if len(sp) != 3:
        raise ValueError("spacing: three values (H, W, D)")
    return sp


def _grown(buf: Optional[torch.Tensor], nbytes: int, device) -> torch.Tensor:
    if buf is None or buf.device != device or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
    return buf


def distance_transform_edt(mask: torch.Tensor, spacing: Optional[Sequence[float]] = None) -> torch.Tensor:
    """scipy.ndimage.distance_transform_edt(~(mask > 0), sampling=spacing) per sample of a [B, H, W, D] (or
    [H, W, D]) mask on the device: fp64, same shape; +inf throughout a sample with no foreground."""
    if mask.device.type != "cuda":
        raise RuntimeError("HIP distance_transform_edt needs ROCm tensors; there is no CPU path")
    if mask.dim() not in (3, 4):
        raise ValueError("mask: [B, H, W, D] or [H, W, D]")
    m = _index_mask(mask)
    B, H, W, D = (1, *m.shape) if m.dim() == 3 else m.shape
    s0, s1, s2 = _spacing3(spacing)
    out = torch.empty(m.shape, dtype=torch.float64, device=m.device)
    nbytes = lib().mmseg_edt_ws_bytes(B, H, W, D)
    ws = _grown(None, nbytes, m.device)
    lib().mmseg_edt(ptr(m), m.element_size(), B, H, W, D, s0, s1, s2, ptr(out), ptr(ws), nbytes, stream_handle())
    return out


class HausdorffDistance:
    """reference metrics.py:91-162 (binary foreground union, np.percentile of the two-way border distances).

    `update` enqueues the distance transforms, the border gather and the rank selection and keeps one [B, 4]
    fp64 record tensor {n, a[lo], a[hi], skipped} per call on the device; nothing is copied or synchronised.
    `compute()` copies those records, interpolates each non-skipped sample as np.percentile does and appends it
    to `self.distances`, then applies np.mean / np.std like the reference.  Updates share one workspace, so they
    must be issued on one stream."""

    def __init__(self, percentile: float = 95):
        self.percentile = percentile
        self._ws: Optional[torch.Tensor] = None
        self.reset()

    def reset(self) -> None:
        self.distances: List[Any] = []
        self._pending: List[torch.Tensor] = []

    def update(self, pred: torch.Tensor, target: torch.Tensor,
               spacing: Optional[Tuple[float, float, float]] = None) -> None:
        """pred / target: [B, H, W, D] class-index masks; foreground is `> 0`."""
        if pred.device.type != "cuda" or target.device.type != "cuda":
            raise RuntimeError("HIP HausdorffDistance needs ROCm tensors; there is no CPU path")
        if pred.dim() != 4 or pred.shape != target.shape:
            raise ValueError("pred / target: [B, H, W, D] masks of one shape")
        pred, target = _index_mask(pred), _index_mask(target)
        B, H, W, D = pred.shape
        s0, s1, s2 = _spacing3(spacing)
        nbytes = lib().mmseg_hd_ws_bytes(B, H, W, D)
        self._ws = _grown(self._ws, nbytes, pred.device)
        rec = torch.empty((B, 4), dtype=torch.float64, device=pred.device)
        lib().mmseg_hd_update(ptr(pred), pred.element_size(), ptr(target), target.element_size(), B, H, W, D,
                              s0, s1, s2, float(np.true_divide(self.percentile, 100)), ptr(rec), ptr(self._ws),
                              self._ws.numel(), stream_handle())
        self._pending.append(rec)

    def _drain(self) -> None:
        for rec in self._pending:
            for n, a_lo, a_hi, skipped in rec.cpu().numpy():
                if not skipped:
                    self.distances.append(percentile_from_order_stats(int(n), a_lo, a_hi, self.percentile))
        self._pending = []

    def moments(self) -> np.ndarray:
        self._drain()
        return hd_moments(self.distances)

    def compute(self) -> Dict[str, float]:
        self._drain()
        if len(self.distances) == 0:
            return {"hausdorff_distance": float("inf")}
        return {
            "hausdorff_distance": np.mean(self.distances),
            "hausdorff_distance_std": np.std(self.distances),
        }


class ConfusionMatrix:
    """reference metrics.py:165-226: matrix[t, p] counts, exact int64 on the device (allocated on the first
    update), and the reference's numpy arithmetic on the host copy in `compute()`.  A pair with a label outside
    [0, num_classes) is counted in `invalid` and not in the matrix; `compute()` then raises the IndexError the
    reference's update would have raised."""

    def __init__(self, num_classes: int):
        self.num_classes = num_classes
        self.reset()

    def reset(self) -> None:
        self._dev: Optional[torch.Tensor] = None      # [C * C + 1] int64: the matrix, then the invalid count

    def _buffers(self, device) -> torch.Tensor:
        if self._dev is None:
            self._dev = torch.zeros(self.num_classes * self.num_classes + 1, dtype=torch.int64, device=device)
        elif self._dev.device != device:
            raise RuntimeError("ConfusionMatrix: updates from more than one device")
        return self._dev

    def update(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        if pred.device.type != "cuda" or target.device.type != "cuda":
            raise RuntimeError("HIP ConfusionMatrix needs ROCm tensors; there is no CPU path")
        if pred.numel() != target.numel():
            raise ValueError("pred / target: masks of one size")
        pred, target = _index_mask(pred), _index_mask(target)
        dev = self._buffers(pred.device)
        C = self.num_classes
        lib().mmseg_confusion_counts_idx(ptr(pred), pred.element_size(), ptr(target), target.element_size(),
                                         pred.numel(), C, ptr(dev), dev.data_ptr() + 8 * C * C, stream_handle())

    def update_from_logits(self, logits: torch.Tensor, target: torch.Tensor) -> None:
        """update(argmax(logits, dim=1), target) without materialising the mask."""
        if logits.device.type != "cuda" or target.device.type != "cuda":
            raise RuntimeError("HIP ConfusionMatrix needs ROCm tensors; there is no CPU path")
        logits = logits.float().contiguous()
        target = _index_mask(target)
        N, C = logits.shape[:2]
        V = logits.numel() // (N * C)
        if C != self.num_classes or target.numel() != N * V:
            raise ValueError("logits [N, num_classes, ...] and target [N, ...] do not match")
        dev = self._buffers(logits.device)
        lib().mmseg_confusion_counts(ptr(logits), ptr(target), target.element_size(), N, C, V, ptr(dev),
                                     dev.data_ptr() + 8 * C * C, stream_handle())

    @property
    def matrix(self) -> np.ndarray:
        C = self.num_classes
        if self._dev is None:
            return np.zeros((C, C), dtype=np.int64)
        return self._dev[:C * C].cpu().numpy().reshape(C, C)

    @property
    def invalid(self) -> int:
        return 0 if self._dev is None else int(self._dev[-1].item())

    def compute(self) -> Dict[str, Any]:
        if self.invalid:
            raise IndexError(f"ConfusionMatrix: {self.invalid} voxel(s) with a label outside "
                             f"[0, {self.num_classes})")
        return confusion_summary(self.matrix)


def confusion_summary(matrix: np.ndarray) -> Dict[str, Any]:
    """reference metrics.py:205-226 on an int64 matrix."""
    tp = np.diag(matrix)
    fp = matrix.sum(axis=0) - tp
    fn = matrix.sum(axis=1) - tp
    precision = tp / (tp + fp + 1e-8)
    recall = tp / (tp + fn + 1e-8)
    f1 = 2 * precision * recall / (precision + recall + 1e-8)
    accuracy = tp.sum() / (matrix.sum() + 1e-8)
    return {
        "accuracy": accuracy,
        "precision": precision.mean(),
        "recall": recall.mean(),
        "f1": f1.mean(),
        "precision_per_class": precision.tolist(),
        "recall_per_class": recall.tolist(),
        "f1_per_class": f1.tolist(),
        "confusion_matrix": matrix.tolist(),
    }


def get_metrics(config: Dict[str, Any]) -> Dict[str, Any]:
    """reference metrics.py:229-244.  The ConfusionMatrix allocates on its first update: building it does no
    device work."""
    num_classes = config["model"]["out_channels"]
    return {"dice": DiceMetric(num_classes=num_classes), "confusion": ConfusionMatrix(num_classes=num_classes)}
