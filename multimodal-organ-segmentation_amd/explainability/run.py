"""`main.py --mode eval --gradcam --shap`: heat maps of the first validation cases, written as NIfTI volumes on the
network grid under <output_dir>/explain/."""
from __future__ import annotations

from pathlib import Path
from typing import Any, Dict, List

import numpy as np

from ..utils.nifti import save_nifti
from .common import backbone_of, check_layer, default_layer
from .gradcam import GradCAM
from .shap_analysis import SHAPAnalyzer


def explain_config(config: Dict[str, Any]) -> Dict[str, Any]:
    """explainability.{gradcam, shap} with their defaults filled in (target_layers / target_classes: None = the
    bottleneck layer / every foreground class)."""
    ex = config.get("explainability") or {}
    gc, sh = dict(ex.get("gradcam") or {}), dict(ex.get("shap") or {})
    return {"gradcam": {"enabled": bool(gc.get("enabled", False)), "target_layers": gc.get("target_layers"),
                        "target_classes": gc.get("target_classes"), "num_cases": int(gc.get("num_cases", 1))},
            "shap": {"enabled": bool(sh.get("enabled", False)), "method": str(sh.get("method", "gradient")),
                     "n_steps": int(sh.get("n_steps", 50))}}


def run_explain(config: Dict[str, Any], model, loader, logger=None) -> List[Path]:
    """Grad-CAM per (layer, class) and SHAP per class for the first num_cases samples of `loader`; returns the
    files written."""
    cfg = explain_config(config)
    gc, sh = cfg["gradcam"], cfg["shap"]
    if not (gc["enabled"] or sh["enabled"]):
        return []
    bb = backbone_of(model)
    layers = gc["target_layers"] or [default_layer(model)]
    layers = [check_layer(model, n) for n in layers]
    classes = gc["target_classes"]
    if classes is None:
        classes = list(range(1, bb.out_channels))
    classes = [int(c) for c in classes]
    out_dir = Path(config["experiment"].get("output_dir", "outputs")) / config["experiment"]["name"] / "explain"
    out_dir.mkdir(parents=True, exist_ok=True)
    cam = GradCAM(model, layers) if gc["enabled"] else None
    shap = SHAPAnalyzer(model) if sh["enabled"] else None
    written: List[Path] = []
    done = 0
    for batch in loader:
        images, ids = batch["image"], batch["patient_id"]
        for i in range(images.shape[0]):
            if done >= gc["num_cases"]:
                return written
            x, pid = images[i:i + 1], str(ids[i])
            for c in classes:
                if cam is not None:
                    for layer in layers:
                        p = out_dir / f"{pid}_gradcam_{layer}_c{c}.nii.gz"
                        save_nifti(np.ascontiguousarray(cam(x, c, layer), dtype=np.float32), p)
                        written.append(p)
                if shap is not None:
                    vals = shap.compute_shap_values(x, c, method=sh["method"], n_steps=sh["n_steps"])
                    # one volume per class: the attributions summed over the input channels
                    p = out_dir / f"{pid}_shap_c{c}.nii.gz"
                    save_nifti(np.ascontiguousarray(vals.sum(axis=0), dtype=np.float32), p)
                    written.append(p)
            done += 1
            if logger is not None:
                logger.info(f"explain: {pid}: {len(written)} files under {out_dir}")
    return written
