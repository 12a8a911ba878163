"""SUV distribution statistics, histogram counts and threshold-volume curves per organ: the numbers behind the
reference's HistogramAnalyzer (src/analysis/histogram.py); its matplotlib figures are not drawn."""
from __future__ import annotations

from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np

from . import core


def histogram_results(rec: core.CaseRecord, labels: Dict[int, str]) -> Dict[str, Any]:
    """histogram.py:103-143 (per_organ) and 202-242 (threshold_curves, the relative curve) from a record."""
    per_organ, curves = {}, {}
    for label_id, organ_name in labels.items():
        if label_id > rec.organ_max or rec.count(label_id) == 0:
            continue
        o = rec.organ(label_id)
        per_organ[organ_name] = {"mean": o["mean"], "std": o["std"], "median": o["median"], "max": o["max"],
                                 "min": o["min"]}
        total_volume = o["count"]
        volumes = [c / total_volume * 100 for c in rec.curve(label_id)]
        curves[organ_name] = list(zip(rec.curve_rel.tolist(), volumes))
    return {"per_organ": per_organ, "threshold_curves": curves}


class HistogramAnalyzer:
    """Generate histogram statistics for SUV distributions in organs."""

    ORGAN_LABELS = dict(core.ORGAN_LABELS)

    def __init__(self, config: Dict[str, Any]):
        self.config = config
        self.hist_config = config.get("analysis", {}).get("histogram", {})
        self.bins = self.hist_config.get("bins", 100)
        suv_cfg = config.get("analysis", {}).get("suv", {})
        self.organ_max = int(suv_cfg.get("organ_max", max(self.ORGAN_LABELS)))
        self.liver_label = int(suv_cfg.get("liver_label", 5))
        self._record: Optional[core.CaseRecord] = None

    def analyze(self, input_path: Union[str, Path], output_path: Union[str, Path]) -> Dict[str, Any]:
        input_path, output_path = Path(input_path), Path(output_path)
        output_path.mkdir(parents=True, exist_ok=True)
        suv_file = self._find_file(input_path, ["*suv*.nii*", "*SUV*.nii*"])
        seg_file = self._find_file(input_path, ["*seg*.nii*", "*label*.nii*", "*pred*.nii*"])
        if suv_file is None or seg_file is None:
            raise FileNotFoundError("SUV or segmentation file not found")
        self._record, _ = core.analyze_files(suv_file, seg_file, organ_max=self.organ_max,
                                             liver_label=self.liver_label, bins=int(self.bins))
        return histogram_results(self._record, self.ORGAN_LABELS)

    def histograms(self) -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
        """{organ: (counts int64 [bins], edges float64 [bins + 1])} of the last analyze(): np.histogram(organ_suv,
        bins=bins), what the reference's ax.hist draws."""
        if self._record is None:
            raise RuntimeError("histograms(): call analyze() first")
        return {name: self._record.histogram(label) for label, name in self.ORGAN_LABELS.items()
                if label <= self._record.organ_max and self._record.count(label) > 0}

    def absolute_curves(self) -> Dict[str, List[Tuple[float, float]]]:
        """The second panel of _generate_threshold_curves (histogram.py:252-274): volume percent at or above each
        absolute SUV threshold of np.linspace(0, 20, 50); the reference plots it and returns nothing."""
        if self._record is None:
            raise RuntimeError("absolute_curves(): call analyze() first")
        rec, out = self._record, {}
        for label, name in self.ORGAN_LABELS.items():
            if label <= rec.organ_max and rec.count(label) > 0:
                n = rec.count(label)
                out[name] = list(zip(rec.curve_abs.tolist(), [c / n * 100 for c in rec.curve(label, absolute=True)]))
        return out

    def _find_file(self, directory: Path, patterns: List[str]) -> Optional[Path]:
        return core.find_file(directory, patterns)
