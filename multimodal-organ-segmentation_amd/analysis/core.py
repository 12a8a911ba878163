"""One case through mmseg_suv_analyze (csrc/analysis.hip) and the host helpers the three analyzers share.

The SUV volume and the segmentation go to the device as the files hold them (HostStager.upload of the raw voxel
block); every statistic comes back in one record block, read with one copy -- the case's only synchronisation --
and the TMTV masks, when asked for, as 3 * V bytes in file order.
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

ORGAN_LABELS = {1: "bladder", 2: "kidney_right", 3: "kidney_left", 4: "heart", 5: "liver", 6: "spleen", 7: "brain"}
ORGAN_MAX_LIMIT = 15
CURVE_POINTS = 50

# ---- the record's cells (include/mmseg_hip.h, mmseg_suv_analyze)
R_INVALID = 0
R_ABS = 1            # count, sum, max, mean
R_PCT_THR = 5
R_PCT = 6            # count, sum, max, mean
R_LIVER_PRESENT = 10
R_LIVER_THR = 11
R_LIV = 12           # count, sum, max, mean
R_LIVER_MEAN = 16
R_LIVER_STD = 17
R_ARG = 18
R_PEAK = 19
R_TUM = 20           # count, sum, max, mean, a_lo, a_hi
R_MAX_REGION = 26
R_SLOT = 32          # + 8 s: count, min, max, sum, mean, m2, std
R_ORG = 168          # + 8 o: n40, n50, n60, a_lo, a_hi, hist lo, hist hi
R_CREL = 288         # + 64 o + j
R_CABS = 1248
R_HIST = 2208        # + 256 o + i
R_CELLS = 6048
CURVE_STRIDE, HIST_STRIDE = 64, 256


def find_file(directory: Path, patterns: Sequence[str]) -> Optional[Path]:
    """The first pattern with a match below `directory` decides; of its matches the first in sorted order (the
    reference takes matches[0] of an rglob, which is in filesystem order)."""
    directory = Path(directory)
    for pattern in patterns:
        matches = sorted(directory.rglob(pattern))
        if matches:
            return matches[0]
    return None


def voxel_volume_ml(zooms) -> np.float32:
    """np.prod(header.get_zooms()) / 1000.0 as numpy 2 computes it for nibabel's float32 zooms: a float32 product,
    divided in float32.  A count times it is float64."""
    return np.prod(np.asarray(zooms, dtype=np.float32)) / 1000.0


def median_from_pair(n: int, lo: float, hi: float) -> float:
    """np.median from the two middle order statistics a[(n - 1) // 2] and a[n // 2]: numpy takes the mean of the
    middle element(s), which for two is (a + b) / 2 and for one the element itself."""
    if n < 1:
        raise ValueError("median of no values")
    if n % 2:
        return float(lo)
    return float((np.float64(lo) + np.float64(hi)) / 2.0)


def curve_thresholds() -> Tuple[np.ndarray, np.ndarray]:
    """_generate_threshold_curves' two grids: fractions of the organ's maximum, and absolute SUVs."""
    return np.linspace(0, 1, CURVE_POINTS), np.linspace(0, 20, CURVE_POINTS)


@dataclass
class CaseRecord:
    """The record of one case, parsed lazily: `u` the cells as uint64, `f` the same cells as float64."""
    u: np.ndarray
    f: np.ndarray
    shape: Tuple[int, int, int]
    organ_max: int
    liver_label: int
    bins: int
    curve_rel: np.ndarray
    curve_abs: np.ndarray
    abs_thr: float
    pct_thr: float
    tumor_thr: float
    has_seg: bool
    masks: Optional[np.ndarray] = None        # [3, X, Y, Z] uint8: absolute, percentage, liver-based

    def count(self, slot: int) -> int:
        return int(self.u[R_SLOT + 8 * slot])

    def slot(self, slot: int) -> Dict[str, float]:
        b = R_SLOT + 8 * slot
        return {"count": int(self.u[b]), "min": float(self.f[b + 1]), "max": float(self.f[b + 2]),
                "sum": float(self.f[b + 3]), "mean": float(self.f[b + 4]), "m2": float(self.f[b + 5]),
                "std": float(self.f[b + 6])}

    def organ(self, label: int) -> Dict[str, float]:
        """The organ's slot plus its threshold counts and its median."""
        d = self.slot(label)
        b = R_ORG + 8 * (label - 1)
        d["n40"], d["n50"], d["n60"] = int(self.u[b]), int(self.u[b + 1]), int(self.u[b + 2])
        d["a_lo"], d["a_hi"] = float(self.f[b + 3]), float(self.f[b + 4])
        d["median"] = median_from_pair(d["count"], d["a_lo"], d["a_hi"])
        d["hist_range"] = (float(self.f[b + 5]), float(self.f[b + 6]))
        return d

    def curve(self, label: int, absolute: bool = False) -> np.ndarray:
        b = (R_CABS if absolute else R_CREL) + CURVE_STRIDE * (label - 1)
        return self.u[b:b + len(self.curve_rel)].astype(np.int64)

    def histogram(self, label: int) -> Tuple[np.ndarray, np.ndarray]:
        """np.histogram(organ_suv, bins=self.bins): (counts int64 [B], edges float64 [B + 1])."""
        b = R_HIST + HIST_STRIDE * (label - 1)
        lo, hi = self.organ(label)["hist_range"]
        return self.u[b:b + self.bins].astype(np.int64), np.linspace(lo, hi, self.bins + 1)

    def masked(self, base: int) -> Dict[str, float]:
        return {"count": int(self.u[base]), "sum": float(self.f[base + 1]), "max": float(self.f[base + 2]),
                "mean": float(self.f[base + 3])}


def analyze_raw(suv_header, suv_raw, seg_header=None, seg_raw=None, *, organ_max: int = 7, liver_label: int = 5,
                abs_thr: float = 2.5, pct_thr: float = 0.4, tumor_thr: float = 2.5, bins: int = 100,
                want_masks: bool = False) -> CaseRecord:
    """suv_raw / seg_raw: the files' voxel blocks on the device (uint8 tensors of header.nbytes bytes)."""
    import torch

    from .._lib import lib, ptr, stream_handle
    from ..data.device import _require_device

    _require_device(suv_raw, "analyze_raw")
    if not 1 <= organ_max <= ORGAN_MAX_LIMIT:
        raise ValueError(f"organ_max in 1..{ORGAN_MAX_LIMIT} (got {organ_max})")
    if not 1 <= bins <= HIST_STRIDE:
        raise ValueError(f"analysis.histogram.bins in 1..{HIST_STRIDE} (got {bins})")
    if suv_raw.dtype != torch.uint8 or suv_raw.numel() != suv_header.nbytes or not suv_raw.is_contiguous():
        raise ValueError(f"analyze_raw: {suv_header.nbytes} contiguous raw SUV bytes expected (got {suv_raw.numel()})")
    has_seg = seg_header is not None
    if has_seg:
        if tuple(seg_header.shape) != tuple(suv_header.shape):
            raise ValueError(f"segmentation shape {tuple(seg_header.shape)} differs from the SUV volume's "
                             f"{tuple(suv_header.shape)}")
        if seg_raw.dtype != torch.uint8 or seg_raw.numel() != seg_header.nbytes or not seg_raw.is_contiguous():
            raise ValueError(f"analyze_raw: {seg_header.nbytes} contiguous raw segmentation bytes expected")
    L = lib()
    assert L.mmseg_suv_record_cells() == R_CELLS
    X, Y, Z = (int(v) for v in suv_header.shape)
    V = X * Y * Z
    dev = suv_raw.device
    crel, cabs = curve_thresholds()
    curves = torch.from_numpy(np.concatenate([crel, cabs])).to(dev)
    record = torch.empty(R_CELLS, dtype=torch.int64, device=dev)
    ws_bytes = int(L.mmseg_suv_ws_bytes(V))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    masks = torch.empty(3 * V, dtype=torch.uint8, device=dev) if want_masks else None

    def vol(h):
        return h.datatype, int(h.swapped), int(h.scaled), float(np.float32(h.scl_slope)), float(np.float32(h.scl_inter))

    seg_args = (ptr(seg_raw),) + vol(seg_header) if has_seg else (None, 2, 0, 0, 0.0, 0.0)
    L.mmseg_suv_analyze(ptr(suv_raw), *vol(suv_header), *seg_args, X, Y, Z, int(organ_max), int(liver_label),
                        float(abs_thr), float(pct_thr), float(tumor_thr), ptr(curves), ptr(curves) + 8 * len(crel),
                        len(crel), int(bins), ptr(masks), ptr(record), ptr(ws), ws_bytes, stream_handle())
    host_masks = None
    if want_masks:
        host_masks = np.stack([m.reshape((X, Y, Z), order="F") for m in masks.cpu().numpy().reshape(3, V)])
    u = record.cpu().numpy().view(np.uint64)          # the case's synchronisation
    rec = CaseRecord(u=u, f=u.view(np.float64), shape=(X, Y, Z), organ_max=int(organ_max), liver_label=int(liver_label),
                     bins=int(bins), curve_rel=crel, curve_abs=cabs, abs_thr=abs_thr, pct_thr=pct_thr,
                     tumor_thr=tumor_thr, has_seg=has_seg, masks=host_masks)
    invalid = int(u[R_INVALID])
    if invalid:
        raise ValueError(f"{invalid} non-finite SUV voxel(s): the statistics are undefined (the reference would "
                         "propagate NaN silently)")
    return rec


_STAGERS: Dict[str, object] = {}


def analyze_files(suv_path, seg_path=None, **kw) -> Tuple[CaseRecord, object]:
    """Read both files, upload their voxel blocks and run the kernels: (record, the SUV file's NiftiHeader)."""
    import torch

    from ..data.nifti import HostStager
    from ..utils.nifti import read_nifti_raw

    dev = torch.device("cuda", torch.cuda.current_device())
    stager = _STAGERS.setdefault(str(dev), HostStager(dev))
    h, raw = read_nifti_raw(suv_path)
    suv_dev = stager.upload(raw)
    sh, seg_dev = None, None
    if seg_path is not None:
        sh, sraw = read_nifti_raw(seg_path)
        if tuple(sh.shape) != tuple(h.shape):
            raise ValueError(f"{seg_path}: shape {tuple(sh.shape)} differs from {suv_path}'s {tuple(h.shape)}")
        seg_dev = stager.upload(sraw)
    return analyze_raw(h, suv_dev, sh, seg_dev, **kw), h


def write_csv(path: Path, rows: List[Dict], columns: Optional[List[str]] = None) -> List[str]:
    """DataFrame(rows).to_csv(index=False): the columns in order of first appearance, a missing value empty."""
    import csv
    if columns is None:
        columns = []
        for r in rows:
            for k in r:
                if k not in columns:
                    columns.append(k)
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=columns, restval="")
        w.writeheader()
        for r in rows:
            w.writerow(r)
    return columns
