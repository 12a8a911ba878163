"""Grad-CAM, Grad-CAM++ and gradient attributions (reference src/explainability/gradcam.py, shap_analysis.py).

With `hardware.kernels: hip` the classes drive the engine's taps, data-only backward and input gradient
(SegEngine.explain) and the kernels of csrc/explain.hip; with `hardware.kernels: torch` they run the reference
algorithm through module hooks on `torch_forward` (DESIGN.md "Explainability").  The reference's matplotlib
helpers, AttentionVisualizer and TSNEVisualizer are out of scope."""
from .common import valid_layers
from .gradcam import GradCAM, GradCAMPlusPlus
from .run import explain_config, run_explain
from .shap_analysis import SHAPAnalyzer

__all__ = ["GradCAM", "GradCAMPlusPlus", "SHAPAnalyzer", "valid_layers", "explain_config", "run_explain"]
