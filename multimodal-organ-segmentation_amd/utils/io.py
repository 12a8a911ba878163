"""YAML config loading (reference src/utils/io.py:15-33), safe loader only, and the reference's NIfTI
load / save interface (io.py:54-112) on the package's own reader / writer (utils/nifti.py)."""
from typing import Any, Dict

import yaml

from .nifti import load_nifti, save_nifti  # noqa: F401


def load_config(path: str) -> Dict[str, Any]:
    with open(path) as f:
        return yaml.safe_load(f)
