"""SUV statistics per segmented organ: the reference's SUVAnalyzer (src/analysis/suv.py) on the device."""
from __future__ import annotations

from pathlib import Path
from typing import Any, Dict, List, Optional, Union

import numpy as np

from . import core

SUV_COLUMNS = ["organ", "label_id", "suv_max", "suv_mean", "suv_std", "suv_median", "suv_min", "volume_ml",
               "volume_voxels", "suv_40_volume", "suv_50_volume", "suv_60_volume"]


def organ_rows(rec: core.CaseRecord, voxel_volume, labels: Dict[int, str]) -> List[Dict[str, Any]]:
    """suv.py:76-105 from a record; `voxel_volume` in ml (the reference's float32 value, or a pinned one)."""
    rows = []
    for label_id, organ_name in labels.items():
        if label_id > rec.organ_max or rec.count(label_id) == 0:
            continue
        o = rec.organ(label_id)
        n = np.int64(o["count"])
        rows.append({
            "organ": organ_name,
            "label_id": label_id,
            "suv_max": o["max"],
            "suv_mean": o["mean"],
            "suv_std": o["std"],
            "suv_median": o["median"],
            "suv_min": o["min"],
            "volume_ml": float(n * voxel_volume),
            "volume_voxels": int(n),
            "suv_40_volume": float(np.int64(o["n40"]) * voxel_volume),
            "suv_50_volume": float(np.int64(o["n50"]) * voxel_volume),
            "suv_60_volume": float(np.int64(o["n60"]) * voxel_volume),
        })
    return rows


def tumor_result(rec: core.CaseRecord, voxel_volume, threshold) -> Dict[str, Any]:
    """suv.py:147-167: the voxels at or above `threshold` outside every organ (label <= 0)."""
    t = rec.masked(core.R_TUM)
    if t["count"] == 0:
        return {"num_lesions": 0, "total_volume_ml": 0, "max_suv": 0}
    n = np.int64(t["count"])
    return {
        "num_voxels": int(n),
        "volume_ml": float(n * voxel_volume),
        "suv_max": t["max"],
        "suv_mean": t["mean"],
        "suv_median": core.median_from_pair(int(n), float(rec.f[core.R_TUM + 4]), float(rec.f[core.R_TUM + 5])),
        "threshold_used": threshold,
    }


class SUVAnalyzer:
    """Analyze SUV values within segmented organs."""

    ORGAN_LABELS = dict(core.ORGAN_LABELS)

    def __init__(self, config: Dict[str, Any]):
        self.config = config
        self.analysis_config = config.get("analysis", {}).get("suv", {})
        self.organ_max = int(self.analysis_config.get("organ_max", max(self.ORGAN_LABELS)))
        self.liver_label = int(self.analysis_config.get("liver_label", 5))

    def analyze(self, input_path: Union[str, Path], output_path: Union[str, Path],
                voxel_volume: Optional[float] = None) -> Dict[str, Any]:
        input_path, output_path = Path(input_path), Path(output_path)
        output_path.mkdir(parents=True, exist_ok=True)
        suv_file = self._find_file(input_path, patterns=["*suv*.nii*", "*SUV*.nii*"])
        seg_file = self._find_file(input_path, patterns=["*seg*.nii*", "*label*.nii*", "*pred*.nii*"])
        if suv_file is None or seg_file is None:
            raise FileNotFoundError("SUV or segmentation file not found")
        rec, h = core.analyze_files(suv_file, seg_file, organ_max=self.organ_max, liver_label=self.liver_label)
        if voxel_volume is None:
            voxel_volume = core.voxel_volume_ml(h.zooms)
        results = organ_rows(rec, voxel_volume, self.ORGAN_LABELS)
        core.write_csv(output_path / "suv_analysis.csv", results, SUV_COLUMNS)
        return {
            "organs": results,
            "summary": {
                "num_organs_analyzed": len(results),
                "total_volume_ml": sum(r["volume_ml"] for r in results),
            },
        }

    def analyze_tumor(self, suv_path: Union[str, Path], seg_path: Union[str, Path], threshold: float = 2.5,
                      voxel_volume: Optional[float] = None) -> Dict[str, Any]:
        rec, h = core.analyze_files(suv_path, seg_path, organ_max=self.organ_max, liver_label=self.liver_label,
                                    tumor_thr=threshold)
        if voxel_volume is None:
            voxel_volume = core.voxel_volume_ml(h.zooms)
        return tumor_result(rec, voxel_volume, threshold)

    def _find_file(self, directory: Path, patterns: List[str]) -> Optional[Path]:
        return core.find_file(directory, patterns)
