"""Total metabolic tumour volume and total lesion glycolysis: the reference's TMTVAnalyzer
(src/analysis/tmtv.py) on the device, its irregular empty-mask dicts included."""
from __future__ import annotations

from pathlib import Path
from typing import Any, Dict, Optional, Union

import numpy as np

from . import core

SUV_PATTERNS = ["*suv*.nii*", "*SUV*.nii*", "*pet*.nii*", "*PET*.nii*"]
SEG_PATTERNS = ["*seg*.nii*", "*label*.nii*", "*pred*.nii*", "*mask*.nii*"]
MASK_FILES = ["tmtv_absolute.nii.gz", "tmtv_percentage.nii.gz", "tmtv_liver_based.nii.gz"]


def tmtv_results(rec: core.CaseRecord, voxel_volume, absolute_threshold, percentage_threshold) -> Dict[str, Any]:
    """tmtv.py:72-99 from a record; `voxel_volume` in ml."""
    f, results = rec.f, {}
    a = rec.masked(core.R_ABS)
    if a["count"] == 0:
        results["absolute"] = {"volume_ml": 0, "suv_max": 0, "suv_mean": 0, "threshold": absolute_threshold}
    else:
        results["absolute"] = {
            "volume_ml": float(np.int64(a["count"]) * voxel_volume),
            "suv_max": a["max"],
            "suv_mean": a["mean"],
            "suv_peak": float(f[core.R_PEAK]),
            "num_voxels": a["count"],
            "threshold": absolute_threshold,
        }
    p, pthr = rec.masked(core.R_PCT), f[core.R_PCT_THR]
    if p["count"] == 0:
        results["percentage"] = {"volume_ml": 0, "suv_max": 0, "suv_mean": 0, "threshold": np.float64(pthr),
                                 "percentage": percentage_threshold}
    else:
        results["percentage"] = {
            "volume_ml": float(np.int64(p["count"]) * voxel_volume),
            "suv_max": p["max"],
            "suv_mean": p["mean"],
            "num_voxels": p["count"],
            "threshold": float(pthr),
            "percentage": percentage_threshold,
        }
    if rec.has_seg:
        if not int(rec.u[core.R_LIVER_PRESENT]):
            results["liver_based"] = {"volume_ml": 0, "error": "Liver not found in segmentation"}
        else:
            v = rec.masked(core.R_LIV)
            tail = {"threshold": float(f[core.R_LIVER_THR]), "liver_mean": float(f[core.R_LIVER_MEAN]),
                    "liver_std": float(f[core.R_LIVER_STD])}
            if v["count"] == 0:
                results["liver_based"] = {"volume_ml": 0, "suv_max": 0, "suv_mean": 0, **tail}
            else:
                results["liver_based"] = {"volume_ml": float(np.int64(v["count"]) * voxel_volume), "suv_max": v["max"],
                                          "suv_mean": v["mean"], "num_voxels": v["count"], **tail}
    if a["count"] == 0:
        results["tlg"] = {"tlg": 0, "volume_ml": 0, "mean_suv": 0}
    else:
        volume_ml = np.int64(a["count"]) * voxel_volume
        mean_suv = np.float64(a["mean"])
        results["tlg"] = {"tlg": float(volume_ml * mean_suv), "volume_ml": float(volume_ml), "mean_suv": float(mean_suv)}
    return results


class TMTVAnalyzer:
    """Analyze Total Metabolic Tumor Volume from PET/SUV images."""

    def __init__(self, config: Dict[str, Any]):
        self.config = config
        self.tmtv_config = config.get("analysis", {}).get("tmtv", {})
        self.absolute_threshold = self.tmtv_config.get("absolute_threshold", 2.5)
        self.percentage_threshold = self.tmtv_config.get("percentage_threshold", 0.4)
        suv_cfg = config.get("analysis", {}).get("suv", {})
        self.organ_max = int(suv_cfg.get("organ_max", max(core.ORGAN_LABELS)))
        self.liver_label = int(suv_cfg.get("liver_label", 5))
        self.masks = None               # the last case's [3, X, Y, Z] masks

    def analyze(self, input_path: Union[str, Path], output_path: Union[str, Path],
                voxel_volume: Optional[float] = None) -> Dict[str, Any]:
        from ..utils.nifti import save_nifti
        input_path, output_path = Path(input_path), Path(output_path)
        output_path.mkdir(parents=True, exist_ok=True)
        suv_file = self._find_suv_file(input_path)
        seg_file = self._find_seg_file(input_path)
        if suv_file is None:
            raise FileNotFoundError("SUV file not found")
        rec, h = core.analyze_files(suv_file, seg_file, organ_max=self.organ_max, liver_label=self.liver_label,
                                    abs_thr=self.absolute_threshold, pct_thr=self.percentage_threshold,
                                    want_masks=True)
        if voxel_volume is None:
            voxel_volume = core.voxel_volume_ml(h.zooms)
        results = tmtv_results(rec, voxel_volume, self.absolute_threshold, self.percentage_threshold)
        self.masks = rec.masks
        for m, name in enumerate(MASK_FILES[:3 if rec.has_seg else 2]):
            save_nifti(rec.masks[m], output_path / name, affine=h.affine, header=h)
        core.write_csv(output_path / "tmtv_analysis.csv", [{"metric": k, **v} for k, v in results.items()])
        return results

    def _find_suv_file(self, directory: Path) -> Optional[Path]:
        return core.find_file(directory, SUV_PATTERNS)

    def _find_seg_file(self, directory: Path) -> Optional[Path]:
        return core.find_file(directory, SEG_PATTERNS)
