"""The analysis pipeline of `main.py --mode analysis` (the reference's run_analysis, main.py:456-498)."""
from __future__ import annotations

import json
import os
from pathlib import Path
from typing import Any, Dict

import numpy as np

DEFAULTS = {"suv": {"enabled": True}, "tmtv": {"enabled": True, "absolute_threshold": 2.5, "percentage_threshold": 0.4},
            "histogram": {"enabled": True, "bins": 100}}


def analysis_config(config: Dict[str, Any]) -> Dict[str, Any]:
    """config["analysis"] with the reference's defaults filled in (configs/default.yaml:136-146); an absent block
    enables all three analyzers."""
    block = config.setdefault("analysis", {})
    for name, defaults in DEFAULTS.items():
        sub = block.setdefault(name, {})
        for k, v in defaults.items():
            sub.setdefault(k, v)
    return block


def _jsonable(o):
    if isinstance(o, np.ndarray):
        return o.tolist()
    if isinstance(o, np.generic):
        return o.item()
    raise TypeError(f"not JSON serialisable: {type(o)}")


def run_analysis(config: Dict[str, Any], logger) -> Dict[str, Any]:
    from ..distributed import ddp
    from .histogram import HistogramAnalyzer
    from .suv import SUVAnalyzer
    from .tmtv import TMTVAnalyzer

    args = config.get("_args", {})
    input_path = args.get("input")
    output_path = args.get("output") or "outputs/analysis"
    if input_path is None:
        raise ValueError("--input is required for analysis mode")
    block = analysis_config(config)
    if ddp.rank() != 0:          # one case, one GPU: rank 0 analyses, as it writes the predictions
        return {}
    logger.info("Starting analysis pipeline")
    logger.info(f"Input: {input_path}")
    logger.info(f"Output: {output_path}")
    os.makedirs(output_path, exist_ok=True)
    results: Dict[str, Any] = {}
    if block["suv"]["enabled"]:
        logger.info("Running SUV analysis")
        results["suv"] = SUVAnalyzer(config).analyze(input_path, output_path)
    if block["tmtv"]["enabled"]:
        logger.info("Running TMTV analysis")
        results["tmtv"] = TMTVAnalyzer(config).analyze(input_path, output_path)
    if block["histogram"]["enabled"]:
        logger.info("Generating histograms")
        hist = HistogramAnalyzer(config)
        results["histogram"] = hist.analyze(input_path, output_path)
        results["histogram_counts"] = {name: {"counts": c, "edges": e} for name, (c, e) in hist.histograms().items()}
    with open(Path(output_path) / "analysis.json", "w") as f:
        json.dump(results, f, indent=2, default=_jsonable)
    logger.info("Analysis completed")
    return results
