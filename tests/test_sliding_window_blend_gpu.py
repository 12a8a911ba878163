"""Gaussian blending and flip test-time augmentation of the sliding windows (csrc/inference.hip,
inference/sliding_window.py, Trainer.predict, main.py --blend / --tta-flips) against the plain-torch restatement in
tests/sliding_window_ref.py with the SAME predictor on the device, so every comparison is torch.equal: the
window order, the rounded w * pred before each add, the count volume, the flip enumeration and the un-flip must
all agree to the bit.

The stand-in predictor is an arithmetic map that is not flip-symmetric and contains the voxel's in-window
position, so a wrong un-flip or a window read at the wrong offset shows.  Shapes are odd and non-cubic; they cover
clamped last windows, a batch spanning two images, a volume smaller than the roi (negative starts), one window,
the 16-byte path (W, roi and every start along W multiples of 4) with overlapping windows, batches that
alternate between the 16-byte and the scalar path, and more windows in one batch than one launch carries (32)."""
import copy

import numpy as np
import pytest
import torch
import yaml

import mmseg_amd  # noqa: F401
from mmseg_amd._lib import MmsegError, lib, ptr, stream_handle
from mmseg_amd.data.nifti import argmax_encode
from mmseg_amd.inference import (blend_argmax_encode, gaussian_tables, sliding_window_accumulate,
                                 sliding_window_inference)
from tests import nifti_ref as NR
from tests import sliding_window_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [
    ((1, 2, 11, 7, 13), (5, 7, 9), 0.5, 4),       # clamped last windows
    ((2, 2, 9, 9, 9), (5, 5, 5), 0.25, 3),        # a batch spanning two images
    ((1, 2, 3, 12, 8), (5, 8, 8), 0.5, 2),        # smaller than the roi along z: padding, negative starts
    ((1, 2, 8, 8, 8), (8, 8, 8), 0.5, 4),         # one window
    ((2, 2, 9, 10, 16), (5, 6, 8), 0.5, 5),       # 16-byte path: x starts 0, 4, 8; batches across both images
    ((1, 2, 6, 6, 16), (4, 4, 8), 0.3, 2),        # x starts 0, 5, 8: batches alternate 16-byte / scalar path
    ((2, 2, 9, 9, 9), (5, 5, 5), 0.25, 40),       # 54 windows, 40 in a batch: two launches for one batch
]
MODES = [("gaussian", ())] + [(b, f) for b in ("constant", "gaussian") for f in ((0,), (1, 2), (0, 1, 2))]


def standin(b):
    """[nb, 2, r0, r1, r2] -> [nb, 3, r0, r1, r2]; depends on the in-window position, not flip-symmetric."""
    r0, r1, r2 = b.shape[2:]
    f = dict(device=b.device, dtype=torch.float32)
    pos = ((torch.arange(r0, **f)[:, None, None] * 0.37 + torch.arange(r1, **f)[None, :, None] * 0.11)
           + torch.arange(r2, **f)[None, None, :] * 0.05)
    c0 = b[:, 0] * 1.5 + pos
    c1 = b[:, 1] - b[:, 0] * 0.25 + pos * pos * 0.01
    c2 = b[:, 0] * b[:, 1] - pos * 0.5
    return torch.stack([c0, c1, c2], dim=1)


def _volume(shape, dev, seed=3):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


@pytest.mark.parametrize("blend,flips", MODES)
@pytest.mark.parametrize("shape,roi,overlap,swb", SHAPES)
def test_standin_matches_restatement(dev, shape, roi, overlap, swb, blend, flips):
    x = _volume(shape, dev)
    got = sliding_window_inference(x, roi, swb, standin, overlap, blend=blend, tta_flips=flips)
    ref = R.sliding_window(x, roi, swb, standin, overlap, blend=blend, tta_flips=flips)
    assert got.shape == (shape[0], 3) + shape[2:]
    assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("sigma_scale", [0.125, 0.5])
def test_clamp_on_and_off(dev, sigma_scale):
    """roi 8: sigma_scale 0.5 leaves the clamp inactive (the corner weight is its own minimum), 0.125 clamps."""
    roi = (8, 8, 8)
    w = R.importance_map(roi, "gaussian", sigma_scale)
    g = R.gaussian_axis(8, sigma_scale)
    clamped = int((w > (g[:, None, None] * g[None, :, None]) * g[None, None, :]).sum())
    assert (clamped == 0) == (sigma_scale == 0.5)
    x = _volume((1, 2, 12, 8, 16), dev)
    got = sliding_window_inference(x, roi, 3, standin, 0.5, blend="gaussian", sigma_scale=sigma_scale)
    ref = R.sliding_window(x, roi, 3, standin, 0.5, blend="gaussian", sigma_scale=sigma_scale)
    assert torch.equal(got.cpu(), ref)


def _model(dev):
    from mmseg_amd.models.build import build_model
    cfg = {"data": {"modalities": ["CT", "PET"]},
           "model": {"name": "unet", "in_channels": 2, "out_channels": 3,
                     "backbone": {"features": [8, 16, 32, 64, 128]}, "head": {"dropout": 0.0}},
           "hardware": {"device": "cuda", "engine_dtype": "float32"}}
    torch.manual_seed(0)
    m = build_model(cfg).to(dev)
    m.eval()
    return m


def test_engine_model_gaussian_all_flips(dev):
    m = _model(dev)
    x = _volume((1, 2, 48, 40, 56), dev)
    with torch.no_grad():
        got = sliding_window_inference(x, (32, 32, 32), 4, m, 0.5, blend="gaussian", tta_flips=(0, 1, 2))
        ref = R.sliding_window(x, (32, 32, 32), 4, m, 0.5, blend="gaussian", tta_flips=(0, 1, 2))
    assert got.shape == (1, 3, 48, 40, 56)
    assert torch.equal(got.cpu(), ref)


def test_constant_predictor_gives_exactly_one(dev):
    """All-ones logits: out and count are the same sequence of fp32 additions, so the quotient is exactly 1."""
    def ones(b):
        return torch.ones(b.shape[0], 3, *b.shape[2:], device=b.device)
    for shape, roi, overlap, swb in SHAPES[:3] + SHAPES[4:5]:
        got = sliding_window_inference(_volume(shape, dev), roi, swb, ones, overlap, blend="gaussian")
        assert torch.equal(got, torch.ones_like(got))


@pytest.mark.parametrize("shape,roi,overlap,swb", SHAPES[:5])
def test_defaults_are_the_per_window_path(dev, shape, roi, overlap, swb):
    x = _volume(shape, dev)
    today = sliding_window_inference(x, roi, swb, standin, overlap)
    assert torch.equal(sliding_window_inference(x, roi, swb, standin, overlap, blend="constant", sigma_scale=0.125,
                                                tta_flips=()), today)
    # the batched kernels with constant weights form the same sums, and their count is the coverage product
    out, count = sliding_window_accumulate(x, roi, swb, standin, overlap)
    assert torch.equal(count, count.round()) and float(count.min()) >= 1.0
    lib().mmseg_window_finish(ptr(out), ptr(count), out.shape[0], out.shape[1], count[0].numel(), stream_handle())
    assert torch.equal(out, today)


@pytest.mark.parametrize("C", [2, 6])
def test_fused_finish_equals_finish_then_argmax(dev, C):
    """Accumulators with exact ties between classes, and pairs a > b whose quotients by the count round to the
    same float (so skipping the division would pick another class); 64 x 64 tiles with both remainders."""
    X, Y, Z = 70, 5, 67
    g = torch.Generator().manual_seed(11)
    out = torch.randint(0, 4, (C, X, Y, Z), generator=g).float()                  # many exact ties
    count = torch.tensor([0.3, 1.0, 3.0, 7.0, 0.001])[torch.randint(0, 5, (X, Y, Z), generator=g)]
    out[:, :, 1] = out[:, :, 1] * 0.37 + 1.0
    out[0, :, 2] += 1.0
    out[C - 1, :, 2] = torch.nextafter(out[0, :, 2], torch.tensor(float("inf")))  # a > b by one ulp
    out[:, :, 3] = out[0:1, :, 3]                                                 # every class ties
    want_logits = out / count                                                     # IEEE division on the host
    ties = int((want_logits[C - 1, :, 2] == want_logits[0, :, 2]).sum())
    assert 0 < ties < X * Z                                                       # the division decides
    out, count = out.to(dev), count.to(dev)
    got = blend_argmax_encode(out, count)
    finished = out.clone()
    lib().mmseg_window_finish(ptr(finished), ptr(count), 1, C, X * Y * Z, stream_handle())
    assert torch.equal(finished.cpu(), want_logits)
    assert torch.equal(got, argmax_encode(finished))
    want = torch.argmax(want_logits, dim=0).to(torch.uint8).permute(2, 1, 0).reshape(-1)
    assert torch.equal(got.cpu(), want) and len(torch.unique(want)) == C


# ------------------------------------------------------------------------------------ Trainer.predict and main.py
@pytest.fixture(scope="module")
def predict_setup(tmp_path_factory):
    """One 24 x 20 x 16 case (CT int16 with slope / inter, PET float32), a tiny model's checkpoint, a config
    with neither new key, and the mask the restatement gives with Gaussian blending over all eight flips."""
    from bench import make_config
    from mmseg_amd.models.build import build_model, save_checkpoint
    root = tmp_path_factory.mktemp("blend_predict")
    (root / "in" / "ct").mkdir(parents=True)
    (root / "in" / "pet").mkdir()
    rng = np.random.default_rng(59)
    shape = (24, 20, 16)
    ct = (1600 + rng.integers(-300, 300, shape)).astype(np.int16)
    pet = (1.0 + np.abs(rng.standard_normal(shape))).astype(np.float32)
    NR.write_nifti(root / "in" / "ct" / "caseA.nii.gz", ct, slope=0.5, inter=-1024.0)
    NR.write_nifti(root / "in" / "pet" / "caseA.nii", pet)
    raw = np.stack([NR.numpy_decode(ct, np.float32(0.5), np.float32(-1024.0)).astype(np.float32), pet])
    cfg = make_config("unet", 2, "fp32", out_channels=3)
    cfg["model"]["backbone"]["features"] = [8, 16, 32, 64, 128]
    cfg["model"]["backbone"]["img_size"] = [16, 16, 16]
    cfg["experiment"].update({"output_dir": str(root / "out"), "log_dir": str(root / "out" / "logs"),
                              "name": "blend", "seed": 5})
    cfg["inference"] = {"sliding_window": {"roi_size": [16, 16, 16], "overlap": 0.5}, "batch_size": 4}
    torch.manual_seed(0)
    model = build_model(cfg)
    save_checkpoint(model, None, 0, str(root / "model.pth"))
    with open(root / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    model = model.to(torch.device("cuda", 0))
    model.eval()
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(raw))[None].to(torch.device("cuda", 0))
        plain = R.sliding_window(x, (16, 16, 16), 4, model, 0.5)
        ref = R.sliding_window(x, (16, 16, 16), 4, model, 0.5, blend="gaussian", tta_flips=(0, 1, 2))
    want = torch.argmax(ref, dim=1)[0].numpy().astype(np.uint8)
    assert not torch.equal(ref, plain)
    return root, cfg, want


def _read_prediction(path):
    blob, gz = NR.read_file(path)
    assert gz
    return NR.parse_nifti(blob)["data"]


def test_trainer_predict_gaussian_tta(dev, predict_setup, tmp_path):
    from mmseg_amd.models.build import build_model, load_checkpoint
    from mmseg_amd.trainer.trainer import Trainer
    root, cfg, want = predict_setup
    cfg = copy.deepcopy(cfg)
    cfg["inference"]["sliding_window"]["blend"] = "gaussian"
    cfg["inference"]["tta_flips"] = [0, 1, 2]
    model = build_model(cfg)
    load_checkpoint(model, str(root / "model.pth"))
    Trainer(cfg, model).predict(root / "in", tmp_path / "pred")
    assert np.array_equal(_read_prediction(tmp_path / "pred" / "caseA_pred.nii.gz"), want)


def test_main_inference_blend_flags(dev, predict_setup, tmp_path):
    import main as entry
    root, cfg, want = predict_setup
    entry.main(["--mode", "inference", "--config", str(root / "config.yaml"), "--checkpoint", str(root / "model.pth"),
                "--input", str(root / "in"), "--output", str(tmp_path / "cli"), "--blend", "gaussian",
                "--tta-flips", "0", "1", "2"])
    assert np.array_equal(_read_prediction(tmp_path / "cli" / "caseA_pred.nii.gz"), want)


# ----------------------------------------------------------------------------------------------------- validation
def test_entry_points_validate(dev):
    L, s = lib(), stream_handle()
    vol = torch.zeros(1, 2, 8, 8, 8, device=dev)
    win = torch.zeros(4, dtype=torch.int32, device=dev)
    buf = torch.zeros(2 * 4 * 4 * 4, device=dev)
    acc = torch.zeros_like(buf)
    out, count = torch.zeros(1, 2, 8, 8, 8, device=dev), torch.zeros(1, 8, 8, 8, device=dev)
    tabs, wmin = gaussian_tables((4, 4, 4))
    tabs = [t.to(dev) for t in tabs]
    host = torch.zeros(4, dtype=torch.int32)

    def blend(win_host=host, nw=1, kind=1, tables=tabs):
        L.mmseg_window_blend(ptr(buf), 1, 2, 8, 8, 8, win_host.data_ptr(), nw, 4, 4, 4, kind, ptr(tables[0]),
                             ptr(tables[1]), ptr(tables[2]), wmin, ptr(out), ptr(count), s)

    blend()                                                                        # the valid call
    with pytest.raises(MmsegError, match="empty window set"):
        blend(nw=0)
    with pytest.raises(MmsegError, match="out of range"):
        blend(win_host=torch.tensor([1, 0, 0, 0], dtype=torch.int32))
    with pytest.raises(MmsegError, match="out of range"):
        blend(win_host=torch.tensor([-1, 0, 0, 0], dtype=torch.int32))
    with pytest.raises(MmsegError, match="does not touch"):
        blend(win_host=torch.tensor([0, 0, 8, 0], dtype=torch.int32))
    with pytest.raises(MmsegError, match="tables"):
        blend(tables=[tabs[0], None, tabs[2]])
    with pytest.raises(MmsegError, match="blend is"):
        blend(kind=2)
    blend(kind=0, tables=[None, None, None])                                       # constant needs no tables
    with pytest.raises(MmsegError, match="empty window set"):
        L.mmseg_window_gather_flip(ptr(vol), 1, 2, 8, 8, 8, ptr(win), 0, 4, 4, 4, 0, ptr(buf), s)
    with pytest.raises(MmsegError, match="bits above 2"):
        L.mmseg_window_gather_flip(ptr(vol), 1, 2, 8, 8, 8, ptr(win), 1, 4, 4, 4, 8, ptr(buf), s)
    with pytest.raises(MmsegError, match="bits above 2"):
        L.mmseg_tta_accum(ptr(buf), 2, 4, 4, 4, 8, 1, 1.0, ptr(acc), s)
    with pytest.raises(MmsegError, match="empty window set"):
        L.mmseg_tta_accum(ptr(buf), 0, 4, 4, 4, 0, 1, 1.0, ptr(acc), s)
    with pytest.raises(MmsegError):
        L.mmseg_window_finish(ptr(out), None, 1, 2, 512, s)
    with pytest.raises(MmsegError, match="C <= 255"):
        L.mmseg_blend_argmax_encode(ptr(out), ptr(count), 256, 8, 8, 8, ptr(buf), s)
    with pytest.raises(ValueError, match="count"):
        blend_argmax_encode(out[0], count)
    x = _volume((1, 2, 8, 8, 8), dev)
    with pytest.raises(ValueError, match="blend"):
        sliding_window_inference(x, (4, 4, 4), 2, standin, 0.5, blend="linear")
    with pytest.raises(ValueError, match="sigma_scale"):
        sliding_window_inference(x, (4, 4, 4), 2, standin, 0.5, blend="gaussian", sigma_scale=0.0)
    with pytest.raises(ValueError, match="tta_flips"):
        sliding_window_inference(x, (4, 4, 4), 2, standin, 0.5, tta_flips=(0, 0))
    with pytest.raises(ValueError, match="tta_flips"):
        sliding_window_inference(x, (4, 4, 4), 2, standin, 0.5, tta_flips=(3,))
