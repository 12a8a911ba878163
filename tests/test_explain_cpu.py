"""Explainability on the torch backend (CPU): the public classes against the reference's own classes
(tests/golden/explain.npz, float64), the error cases, and the CLI keys.

The fixture was computed in float64, and float32 on the CPU differs from it by up to 1.2e-5 (the fixture records
that error per map), so the 1e-5 bound is checked with the model in float64: the torch path runs in the model's
dtype."""
import os

import numpy as np
import pytest
import torch

import mmseg_amd  # noqa: F401
from mmseg_amd.explainability import GradCAM, GradCAMPlusPlus, SHAPAnalyzer, explain_config, valid_layers
from tests import explain_ref
from tests.explain_cases import CAMS, LAYERS, build, fixture, fixture_err, inputs

torch.set_num_threads(min(8, torch.get_num_threads()))


@pytest.fixture(scope="module")
def fx():
    g = fixture()
    x, bg = inputs(g)
    models = {n: build(g, n).double().eval() for n in ("unet", "dual")}
    return g, x.double(), bg.double(), models


@pytest.mark.parametrize("name,tag,layer", CAMS)
def test_cam_matches_reference(fx, name, tag, layer):
    g, x, _, models = fx
    cls = GradCAM if tag == "gradcam" else GradCAMPlusPlus
    got = cls(models[name], ["backbone." + layer], use_cuda=False)(x, int(g["cls"]))
    err, esum, eabs = fixture_err(g, f"{name}__{tag}__{layer}", got)
    assert err < 1e-5 and esum < 1e-5 and eabs < 1e-5, (err, esum, eabs)
    # the maximum is r / (r + 1e-8) with r the range of the raw map (1.8e-5 for the smallest one here)
    assert got.min() == 0.0 and 0.999 < got.max() <= 1.0


@pytest.mark.parametrize("name", ["unet", "dual"])
def test_gradient_shap_matches_reference(fx, name):
    g, x, bg, models = fx
    got = SHAPAnalyzer(models[name], background_samples=bg).compute_shap_values(x, int(g["cls"]), "gradient")
    err, esum, eabs = fixture_err(g, f"{name}__shap_gradient", got)
    assert err < 1e-5 and eabs < 1e-5, (err, esum, eabs)


def test_integrated_gradients_matches_reference(fx):
    g, x, bg, models = fx
    got = SHAPAnalyzer(models["unet"], background_samples=bg).compute_shap_values(
        x, int(g["cls"]), "integrated_gradients", n_steps=int(g["n_steps"]))
    err, _, eabs = fixture_err(g, "unet__shap_ig", got)
    assert err < 1e-5 and eabs < 1e-5, (err, eabs)


def test_ref_restatement_matches_reference(fx):
    """tests/explain_ref.py (the GPU tests' reference for what the fixture does not hold) against the fixture."""
    g, x, bg, models = fx
    bb = models["unet"].backbone
    c = int(g["cls"])
    for pp, tag in ((False, "gradcam"), (True, "gradcampp")):
        m = explain_ref.cam(bb, bb.torch_forward, "encoders.3.conv", x, c, plus_plus=pp)
        assert fixture_err(g, f"unet__{tag}__encoders.3.conv", m.astype(np.float32))[0] < 1e-5
    s = explain_ref.gradient_shap(bb.torch_forward, x, c, bg)
    assert fixture_err(g, "unet__shap_gradient", s.astype(np.float32))[0] < 1e-5


def test_unwrapped_backbone_and_default_layer_names(fx):
    g, x, _, models = fx
    bb = models["unet"].backbone
    a = GradCAM(bb, ["encoders.3.conv"], use_cuda=False)(x, int(g["cls"]))
    b = GradCAM(models["unet"], ["backbone.encoders.3.conv"], use_cuda=False)(x, int(g["cls"]), "encoders.3.conv")
    assert np.array_equal(a, b)
    assert valid_layers(models["unet"])[:2] == ["init_conv", "encoders.0.conv"]
    assert "decoder.0.conv" in valid_layers(models["dual"]) and "encoders.1.blocks.3.conv" in valid_layers(models["dual"])
    for name in LAYERS["dual"]:
        assert name in valid_layers(models["dual"])


def test_no_parameter_gradient_is_left(fx):
    g, x, bg, models = fx
    m = models["unet"]
    m.zero_grad(set_to_none=True)
    GradCAM(m, ["decoders.0"], use_cuda=False)(x, int(g["cls"]))
    SHAPAnalyzer(m, background_samples=bg).compute_shap_values(x, int(g["cls"]))
    assert all(p.grad is None for p in m.parameters())


def test_error_cases(fx):
    g, x, _, models = fx
    m = models["unet"]
    cam = GradCAM(m, ["decoders.0"], use_cuda=False)
    with pytest.raises(ValueError, match="target_class is required"):
        cam(x, None)
    with pytest.raises(ValueError, match="one sample per call"):
        cam(torch.cat([x, x]), 1)
    with pytest.raises(ValueError, match="target_class is required"):
        SHAPAnalyzer(m).compute_shap_values(x, None)
    with pytest.raises(ValueError, match="one sample per call"):
        SHAPAnalyzer(m).compute_shap_values(torch.cat([x, x]), 1)
    for bad in ("encoders.0", "encoder.layer4", "backbone.encoders.0", "decoders.9"):
        with pytest.raises(ValueError, match="valid names"):
            GradCAM(m, [bad], use_cuda=False)
        with pytest.raises(ValueError, match="valid names"):
            cam(x, 1, bad)
    with pytest.raises(ValueError, match="valid names"):
        GradCAM(models["dual"], ["encoders.0"], use_cuda=False)
    with pytest.raises(ValueError):
        cam(x, 7)


def test_swin_unetr_is_not_covered():
    from mmseg_amd.models.backbones.swin_unetr import SwinUNETR
    net = SwinUNETR(img_size=(32, 32, 32), in_channels=1, out_channels=2, feature_size=24)
    with pytest.raises(NotImplementedError, match="SwinUNETR"):
        GradCAM(net, ["encoder1"], use_cuda=False)
    with pytest.raises(NotImplementedError, match="SwinUNETR"):
        SHAPAnalyzer(net)


def test_cli_keys_parse():
    import main
    from mmseg_amd.utils import load_config
    conf = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "c6_unet_nifti.yaml")
    args = main.parse_args(["--mode", "eval", "--config", conf])
    cfg = main.merge_config_with_args(load_config(args.config), args)
    ex = explain_config(cfg)
    assert ex["gradcam"] == {"enabled": False, "target_layers": None, "target_classes": None, "num_cases": 1}
    assert ex["shap"] == {"enabled": False, "method": "gradient", "n_steps": 50}
    args = main.parse_args(["--mode", "eval", "--config", conf, "--gradcam", "--shap"])
    cfg = main.merge_config_with_args(load_config(args.config), args)
    cfg["explainability"]["gradcam"].update(target_layers=["backbone.decoders.3"], target_classes=[2], num_cases=3)
    ex = explain_config(cfg)
    assert ex["gradcam"]["enabled"] and ex["shap"]["enabled"]
    assert ex["gradcam"]["target_layers"] == ["backbone.decoders.3"] and ex["gradcam"]["num_cases"] == 3
    assert explain_config({}) == explain_config({"explainability": None})


def test_run_explain_writes_heat_maps(fx, tmp_path):
    """The --mode eval --gradcam --shap writer: the first num_cases samples, one file per (layer, class) and class."""
    from mmseg_amd.explainability import run_explain
    from mmseg_amd.utils.nifti import load_nifti
    g, x, _, models = fx
    m = models["unet"]
    cfg = dict(m.config)
    cfg["experiment"] = dict(cfg["experiment"], output_dir=str(tmp_path), name="t")
    cfg["explainability"] = {"gradcam": {"enabled": True, "target_classes": [1], "num_cases": 1},
                             "shap": {"enabled": True}}
    files = run_explain(cfg, m, [{"image": torch.cat([x, x]), "patient_id": ["p0", "p1"]}])
    assert [f.name for f in files] == ["p0_gradcam_encoders.3.conv_c1.nii.gz", "p0_shap_c1.nii.gz"]
    assert all(f.parent == tmp_path / "t" / "explain" for f in files)
    cam = load_nifti(files[0], dtype=np.float32)
    assert cam.shape == (32, 32, 32) and cam.min() == 0.0 and 0.999 < cam.max() <= 1.0
    assert np.array_equal(cam, GradCAM(m, ["encoders.3.conv"], use_cuda=False)(x, 1))
    assert run_explain({"experiment": cfg["experiment"]}, m, []) == []
