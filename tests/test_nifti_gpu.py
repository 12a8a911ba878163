"""NIfTI volumes on the device (csrc/nifti.hip, data/nifti.py, Trainer.predict, main.py --mode inference).

The kernels are held bitwise to numpy / torch on the host: decode to (raw.astype(f8) * slope + inter).astype(f4)
transposed to [X, Y, Z] C order, decode_label to the truncation toward zero, argmax_encode to torch.argmax in
Fortran order.  Shapes cover a tile interior (the tile is 64 x 64 over x, z), both remainders, a degenerate
axis in each position and odd row byte lengths for the 1- and 2-byte types.  Files are written by
tests/nifti_ref.py (struct.pack at the standard's offsets), and predictions are read back with its parser,
never with the package's own reader or writer.  Dataset samples are compared with the host path
load_nifti -> oracle modality_normalize -> resize at the tolerances tests/test_data_gpu.py holds those
kernels to (CT / PET bitwise, resize 2e-7 normwise, labels bitwise)."""
import copy
import sys

import numpy as np
import pytest
import torch
import yaml

import mmseg_amd  # noqa: F401
from mmseg_amd._lib import MmsegError, lib, ptr, stream_handle
from mmseg_amd.data.dataloader import get_dataloader, get_dataset
from mmseg_amd.data.device import DeviceLoader
from mmseg_amd.data.nifti import DeviceNiftiDataset
from mmseg_amd.utils.io import load_nifti
from oracle import data_oracle as DO
from tests import nifti_ref as NR

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (33, 5, 19), (64, 3, 65), (7, 70, 2), (130, 2, 37)]
SCALES = [None, (np.float32(0.5), np.float32(-1024.0)), (np.float32(1.7e-3), np.float32(3.25))]
PRE = {"ct": {"window_center": -100, "window_width": 700}, "pet": {"normalize": True}, "mri": {"normalize": True}}
# float64 inputs whose scaled value by SCALES[2] rounds to another float32 under a fused multiply-add
FMA_SENSITIVE = [1204630.25459469, 3960.195657174413, 1203395.9083334813]


def _file_order(swap):
    """The byte order of a file whose bytes are (swap = 1) or are not (0) swapped against this machine's."""
    native = "<" if sys.byteorder == "little" else ">"
    return native if not swap else (">" if native == "<" else "<")


def _values(code, shape, seed):
    """Seeded values of the type with its extremes (INT32_MIN / MAX, UINT32_MAX, ...) at the front."""
    t = np.dtype(NR.CODES[code])
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if t.kind == "f":
        v = (rng.standard_normal(n) * 1000).astype(t)
        ext = ([np.finfo(np.float32).max, -np.finfo(np.float32).max, np.finfo(np.float32).tiny, -0.0]
               if t == np.float32 else [1e30, -1e-300, 1e-42, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50]
               + FMA_SENSITIVE)
    else:
        info = np.iinfo(t)
        v = rng.integers(info.min, info.max, n, dtype=t, endpoint=True)
        ext = [info.min, info.max, info.max - 1]
    k = min(n, len(ext))
    v[:k] = ext[:k] if n > 1 else ext[1:2]           # a single voxel takes the maximum
    return v.reshape(shape, order="F")


def _upload(arr, code, swap, dev):
    blob = np.asarray(arr).astype(np.dtype(NR.CODES[code]).newbyteorder(_file_order(swap))).tobytes(order="F")
    return blob, torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)


@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("code", sorted(NR.CODES))
def test_decode_bitwise_numpy(dev, code, swap):
    L = lib()
    for si, shape in enumerate(SHAPES):
        arr = _values(code, shape, 100 * code + si)
        blob, raw = _upload(arr, code, swap, dev)
        X, Y, Z = shape
        for sc in SCALES:
            out = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
            slope, inter = (0.0, 0.0) if sc is None else (float(sc[0]), float(sc[1]))
            L.mmseg_nifti_decode(ptr(raw), code, swap, X, Y, Z, int(sc is not None), slope, inter, ptr(out),
                                 stream_handle())
            with np.errstate(over="ignore"):
                ref = NR.numpy_decode(arr, *(sc if sc is not None else (None, None))).astype(np.float32)
            got = out.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(ref).view(np.uint32)), (shape, sc)
        assert bytes(raw.cpu().numpy()) == blob                       # the input is not modified


def test_inputs_tell_two_roundings_from_a_fused_multiply_add():
    """What in test_decode_bitwise_numpy pins `raw * slope` then `+ inter` as two rounded operations.  With the
    24-bit slope 1.7e-3 the product of a uint32 (or a float64) is inexact in float64, so the fused result can be
    one float64 ulp off; the float32 output shows that only where the sum sits on a float32 rounding boundary.
    A search of the uint32 range found no such value for (1.7e-3, 3.25), so the float64 inputs carry FMA_SENSITIVE:
    there the two-rounding sum is an exact float32 tie and the correctly rounded fused sum is not."""
    from fractions import Fraction
    s, i = float(SCALES[2][0]), float(SCALES[2][1])
    big = np.array([0xFFFFFFFF, 0xFFFFFFFE, 0x80000001], dtype=np.float64)
    assert all(Fraction(float(a * s)) != Fraction(float(a)) * Fraction(s) for a in big)      # inexact products
    for v in FMA_SENSITIVE:
        two = np.float64(v) * np.float64(s) + np.float64(i)
        fused = float(Fraction(v) * Fraction(s) + Fraction(i))                  # one rounding of the exact value
        assert np.float32(two) != np.float32(fused)
    for shape in SHAPES[1:]:
        assert set(FMA_SENSITIVE) <= set(_values(64, shape, 0).ravel().tolist())


@pytest.mark.parametrize("label_bytes", [8, 1])
@pytest.mark.parametrize("code", [4, 2, 16])
def test_decode_label_truncates(dev, code, label_bytes):
    L = lib()
    special = {16: [2.9999, -0.5, 0.99999994, 3.0, 254.7, -1.5, 1e-30, 17.5],
               4: [-3, -2, -1, 0, 1, 2, 255, 32767, -32768], 2: [0, 1, 2, 5, 254, 255]}[code]
    odt = torch.int64 if label_bytes == 8 else torch.uint8
    for si, shape in enumerate(SHAPES):
        t = np.dtype(NR.CODES[code])
        rng = np.random.default_rng(7 * code + si)
        n = int(np.prod(shape))
        v = (rng.uniform(-4, 9, n).astype(t) if t.kind == "f" else rng.integers(0, 7, n).astype(t))
        k = min(n, len(special))
        v[:k] = np.asarray(special[:k], dtype=t)
        arr = v.reshape(shape, order="F")
        X, Y, Z = shape
        for swap in (0, 1):
            blob, raw = _upload(arr, code, swap, dev)
            for sc in (None, (np.float32(0.75), np.float32(-0.5))):
                out = torch.full(shape, 99, dtype=odt, device=dev)
                slope, inter = (0.0, 0.0) if sc is None else (float(sc[0]), float(sc[1]))
                L.mmseg_nifti_decode_label(ptr(raw), code, swap, X, Y, Z, int(sc is not None), slope, inter, ptr(out),
                                           label_bytes, stream_handle())
                ref = NR.numpy_decode(arr, *(sc if sc is not None else (None, None))).astype(np.int64)
                if label_bytes == 1:
                    ref = ref.astype(np.uint8)                        # the low byte of the truncated value
                assert np.array_equal(out.cpu().numpy(), ref), (shape, swap, sc)
            assert bytes(raw.cpu().numpy()) == blob


@pytest.mark.parametrize("C", [2, 6, 7])
def test_argmax_encode_first_maximum(dev, C):
    L = lib()
    ties = voxels = 0
    for si, shape in enumerate(SHAPES):
        g = torch.Generator().manual_seed(31 * C + si)
        logits = torch.randint(-1, 2, (C,) + shape, generator=g).float()          # {-1, 0, 1}: ties in most voxels
        X, Y, Z = shape
        n = X * Y * Z
        out = torch.full((n + 8,), 200, dtype=torch.uint8, device=dev)
        L.mmseg_argmax_encode(ptr(logits.to(dev)), C, X, Y, Z, ptr(out), stream_handle())
        ref = torch.argmax(logits, 0).numpy().astype(np.uint8).ravel(order="F")
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], ref), shape
        assert (got[n:] == 200).all()                                             # nothing written past the mask
        ties += int(((logits == logits.amax(0, keepdim=True)).sum(0) > 1).sum())
        voxels += n
    # ties are in fact present: two of three values agree with probability 1/3 (C = 2), the maximum of six or
    # seven draws is shared with probability > 0.8
    assert ties > (voxels // 4 if C == 2 else voxels // 2)


def test_argument_validation(dev):
    L = lib()
    raw = torch.zeros(64, dtype=torch.uint8, device=dev)
    out = torch.zeros(8, dtype=torch.float32, device=dev)
    s = stream_handle()
    with pytest.raises(MmsegError):
        L.mmseg_nifti_decode(None, 4, 0, 2, 2, 2, 0, 0.0, 0.0, ptr(out), s)
    with pytest.raises(MmsegError):
        L.mmseg_nifti_decode(ptr(raw), 4, 0, 2, 2, 2, 0, 0.0, 0.0, None, s)
    with pytest.raises(MmsegError, match="datatype"):
        L.mmseg_nifti_decode(ptr(raw), 32, 0, 2, 2, 2, 0, 0.0, 0.0, ptr(out), s)
    with pytest.raises(MmsegError):
        L.mmseg_nifti_decode(ptr(raw), 4, 0, 2, 0, 2, 0, 0.0, 0.0, ptr(out), s)
    with pytest.raises(MmsegError, match="datatype"):
        L.mmseg_nifti_decode_label(ptr(raw), 1024, 0, 2, 2, 2, 0, 0.0, 0.0, ptr(out), 8, s)
    with pytest.raises(MmsegError, match="out of place"):
        L.mmseg_nifti_decode_label(ptr(raw), 2, 0, 2, 2, 2, 0, 0.0, 0.0, ptr(raw), 1, s)
    with pytest.raises(MmsegError):
        L.mmseg_nifti_decode_label(ptr(raw), 2, 0, 2, 2, 2, 0, 0.0, 0.0, ptr(out), 4, s)
    with pytest.raises(MmsegError):
        L.mmseg_argmax_encode(None, 3, 2, 2, 2, ptr(raw), s)
    with pytest.raises(MmsegError, match="255"):
        L.mmseg_argmax_encode(ptr(out), 256, 2, 2, 2, ptr(raw), s)
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and int(raw.sum()) == 0                  # nothing was launched


# ------------------------------------------------------------------------------------------------ dataset
CASES = [("p0", (20, 18, 22)), ("p1", (24, 24, 16)), ("p2", (20, 18, 22)), ("p3", (17, 21, 19))]
CT_SCALE = (np.float32(0.5), np.float32(-1024.0))
AFFINE = np.array([[-0.9, 0.1, 0.0, 120.5], [0.05, 0.8, -0.2, -33.25], [0.0, 0.3, 2.5, 7.0], [0, 0, 0, 1]])


def _case_arrays(k, shape):
    rng = np.random.default_rng(50 + k)
    lab = np.zeros(shape, dtype=np.uint8)
    lab[shape[0] // 4: shape[0] // 2, 2:-2, 3:-3] = 1
    lab[shape[0] // 2: -2, shape[1] // 2:, 1:-1] = 2
    ct = (1600 + 400 * lab.astype(np.int16) + rng.integers(-300, 300, shape)).astype(np.int16)    # HU = raw/2 - 1024
    pet = (1.0 + 3.0 * lab + np.abs(rng.standard_normal(shape))).astype(np.float32)
    return ct, pet, lab


@pytest.fixture(scope="module")
def nifti_root(tmp_path_factory):
    """A data_root as the reference lays it out: CT int16 with slope / inter (.nii.gz), PET float32 big-endian
    (.nii), uint8 labels, train.csv with four cases of three sizes and val.csv with two."""
    root = tmp_path_factory.mktemp("nifti_root")
    for sub in ("ct", "pet", "label"):
        (root / sub).mkdir()
    rows = []
    for k, (pid, shape) in enumerate(CASES):
        ct, pet, lab = _case_arrays(k, shape)
        NR.write_nifti(root / "ct" / f"{pid}.nii.gz", ct, slope=float(CT_SCALE[0]), inter=float(CT_SCALE[1]),
                       sform=AFFINE)
        NR.write_nifti(root / "pet" / f"{pid}.nii", pet, byteorder=">")
        NR.write_nifti(root / "label" / f"{pid}.nii.gz", lab)
        rows.append(f"{pid},ct/{pid}.nii.gz,pet/{pid}.nii,label/{pid}.nii.gz\n")
    (root / "train.csv").write_text("patient_id,CT,PET,label\n" + "".join(rows))
    (root / "val.csv").write_text("patient_id,CT,PET,label\n" + "".join(rows[:2]))
    return root


def _config(root, out_dir, img_size=(16, 16, 16)):
    from bench import make_config
    cfg = make_config("unet", 2, "fp32", out_channels=3)
    cfg["model"]["backbone"]["features"] = [8, 16, 32, 64, 128]
    cfg["model"]["backbone"]["img_size"] = list(img_size)
    cfg["data"].update({"data_root": str(root), "train_csv": "train.csv", "val_csv": "val.csv",
                        "preprocessing": copy.deepcopy(PRE)})
    cfg["experiment"].update({"output_dir": str(out_dir), "log_dir": str(out_dir / "logs"), "name": "nifti", "seed": 5})
    cfg["training"]["checkpoint"] = {"save_last": True, "save_best": True}
    cfg["inference"] = {"sliding_window": {"roi_size": [16, 16, 16], "overlap": 0.5}, "batch_size": 4}
    return cfg


def _host_sample(root, pid):
    """The reference's host path for one case: load_nifti -> stack -> ModalitySpecificNormalize (oracle)."""
    ct = load_nifti(root / "ct" / f"{pid}.nii.gz", dtype=np.float32)
    pet = load_nifti(root / "pet" / f"{pid}.nii", dtype=np.float32)
    lab = load_nifti(root / "label" / f"{pid}.nii.gz", dtype=np.int64)
    return DO.modality_normalize(np.stack([ct, pet]).copy(), ["CT", "PET"], PRE), lab


def test_dataset_matches_host_path(dev, nifti_root, tmp_path):
    plain = get_dataset(_config(nifti_root, tmp_path, img_size=()), "val")       # no resize: img_size not 3 entries
    sized = get_dataset(_config(nifti_root, tmp_path), "val")
    assert isinstance(sized, DeviceNiftiDataset) and len(sized) == 2
    for i, (pid, shape) in enumerate(CASES[:2]):
        ref_img, ref_lab = _host_sample(nifti_root, pid)
        # the files hold what the test put there (the reader is checked in test_nifti_cpu.py; here it is the oracle)
        ct, pet, lab = _case_arrays(i, shape)
        assert np.array_equal(ref_lab, lab) and 0.0 <= ref_img[0].min() < ref_img[0].max() <= 1.0
        s = plain.get(i, 0)
        assert s["image"].shape == (2,) + shape and s["label"].dtype == torch.int64 and s["patient_id"] == pid
        got = s["image"].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ref_img.view(np.uint32))     # decode + CT window / PET max: bitwise
        assert np.array_equal(s["label"].cpu().numpy(), ref_lab)
        assert torch.equal(s["CT"], s["image"][0]) and torch.equal(s["PET"], s["image"][1])
        r = sized.get(i, 0)
        assert r["image"].shape == (2, 16, 16, 16) and r["label"].shape == (16, 16, 16)
        for m in range(2):
            ref = DO.resize_linear(ref_img[m], (16, 16, 16))
            assert np.abs(r["image"][m].cpu().numpy() - ref).max() <= 2e-7 * np.abs(ref).max()
        assert np.array_equal(r["label"].cpu().numpy(), DO.resize_nearest(ref_lab, (16, 16, 16)))
    cfg8 = _config(nifti_root, tmp_path)
    cfg8["data"]["label_dtype"] = "uint8"
    l8 = get_dataset(cfg8, "val").get(1, 0)["label"]
    assert l8.dtype == torch.uint8 and torch.equal(l8.long(), sized.get(1, 0)["label"])


def test_dataset_errors_name_the_path(dev, nifti_root, tmp_path):
    (tmp_path / "train.csv").write_text("patient_id,CT,PET,label\nx,ct/p0.nii.gz,pet/absent.nii,label/p0.nii.gz\n"
                                        "y,ct/p0.nii.gz,pet/p1.nii,label/p0.nii.gz\n"
                                        "z,ct/p0.nii.gz,pet/p0.nii,label/p1.nii.gz\n")
    cfg = _config(nifti_root, tmp_path)
    cfg["data"]["train_csv"] = str(tmp_path / "train.csv")                       # an absolute path replaces the root
    ds = get_dataset(cfg, "train")
    with pytest.raises(FileNotFoundError, match="absent.nii"):
        ds.get(0, 0)
    with pytest.raises(ValueError, match="p1.nii"):
        ds.get(1, 0)
    with pytest.raises(ValueError, match="label"):
        ds.get(2, 0)


def test_loader_batches_and_augmentation(dev, nifti_root, tmp_path):
    cfg = _config(nifti_root, tmp_path)
    ld = get_dataloader(cfg, "train")
    assert isinstance(ld, DeviceLoader) and len(ld) == 2
    b = next(iter(ld))
    assert set(b) == {"image", "label", "patient_id", "CT", "PET"}
    assert b["image"].shape == (2, 2, 16, 16, 16) and b["image"].is_cuda and b["image"].dtype == torch.float32
    assert b["label"].shape == (2, 16, 16, 16) and b["label"].dtype == torch.int64 and int(b["label"].max()) <= 2
    assert b["CT"].shape == (2, 1, 16, 16, 16) and set(b["patient_id"]) <= {c[0] for c in CASES}
    aug = copy.deepcopy(cfg)
    aug["data"]["augmentation"] = {"enabled": True, "random_flip": True, "random_rotate": 1, "random_intensity": 0.1}
    ds_a, ds_b, ds_p = get_dataset(aug, "train"), get_dataset(aug, "train"), get_dataset(cfg, "train")
    differs = 0
    for i in range(4):
        for epoch in (0, 1):
            a, b2, p = ds_a.get(i, epoch), ds_b.get(i, epoch), ds_p.get(i, epoch)
            assert torch.equal(a["image"], b2["image"]) and torch.equal(a["label"], b2["label"])   # same seed
            assert a["image"].shape == (2, 16, 16, 16)
            differs += int(not torch.equal(a["image"], p["image"]))
    assert differs >= 4
    val_a, val_p = get_dataset(aug, "val").get(0, 0), get_dataset(cfg, "val").get(0, 0)
    assert torch.equal(val_a["image"], val_p["image"])                          # validation is never augmented


def test_trainer_trains_on_nifti(dev, nifti_root, tmp_path):
    from mmseg_amd.models.build import build_model
    from mmseg_amd.trainer.trainer import Trainer
    cfg = _config(nifti_root, tmp_path)
    torch.manual_seed(0)
    tr = Trainer(cfg, build_model(cfg), train_loader=get_dataloader(cfg, "train"),
                 val_loader=get_dataloader(cfg, "val"))
    hist = tr.train()
    assert len(hist["train_loss"]) == 1 and np.isfinite(hist["train_loss"][0]) and np.isfinite(hist["val_loss"][0])
    assert 0.0 <= hist["val_dice"][0] <= 1.0
    assert (tmp_path / "nifti" / "last.pth").exists() and (tmp_path / "nifti" / "best.pth").exists()


# ------------------------------------------------------------------------------------------------ predict
@pytest.fixture(scope="module")
def predict_setup(tmp_path_factory):
    """An input folder with one complete 24 x 20 x 16 case and one that lacks its PET, the raw image the
    reference would feed, and the checkpoint of a tiny model."""
    from mmseg_amd.models.build import build_model, save_checkpoint
    root = tmp_path_factory.mktemp("predict")
    (root / "in" / "ct").mkdir(parents=True)
    (root / "in" / "pet").mkdir()
    ct, pet, _ = _case_arrays(9, (24, 20, 16))
    NR.write_nifti(root / "in" / "ct" / "caseA.nii.gz", ct, slope=float(CT_SCALE[0]), inter=float(CT_SCALE[1]),
                   sform=AFFINE)
    NR.write_nifti(root / "in" / "pet" / "caseA.nii", pet, byteorder=">")
    NR.write_nifti(root / "in" / "ct" / "caseB.nii.gz", ct)                     # no PET: skipped
    raw = np.stack([NR.numpy_decode(ct, *CT_SCALE).astype(np.float32), pet])
    cfg = _config(root, root / "out")
    torch.manual_seed(0)
    save_checkpoint(build_model(cfg), None, 0, str(root / "model.pth"))
    with open(root / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    return root, cfg, raw


def _trainer(cfg, root):
    from mmseg_amd.models.build import build_model, load_checkpoint
    from mmseg_amd.trainer.trainer import Trainer
    cfg = copy.deepcopy(cfg)
    model = build_model(cfg)
    load_checkpoint(model, str(root / "model.pth"))
    return Trainer(cfg, model)


def _expected_mask(trainer, image):
    trainer.model.eval()
    with torch.no_grad():
        logits = trainer._sliding_window_inference(torch.from_numpy(np.ascontiguousarray(image))[None].to(trainer.device))
    return torch.argmax(logits, dim=1)[0].cpu().numpy().astype(np.uint8)


def _read_prediction(path):
    blob, gz = NR.read_file(path)
    assert gz
    return NR.parse_nifti(blob)


def test_predict_writes_the_argmax_in_file_order(dev, predict_setup, tmp_path):
    root, cfg, raw = predict_setup
    tr = _trainer(cfg, root)
    tr.predict(root / "in", tmp_path / "raw")
    assert sorted(p.name for p in (tmp_path / "raw").iterdir()) == ["caseA_pred.nii.gz"]      # caseB lacks its PET
    f = _read_prediction(tmp_path / "raw" / "caseA_pred.nii.gz")
    want = _expected_mask(tr, raw)                                              # the RAW volume, as the reference
    assert f["datatype"] == 2 and f["dim"][:4] == [3, 24, 20, 16] and f["sform_code"] == 2
    assert np.array_equal(f["data"], want) and len(np.unique(want)) > 1
    assert np.array_equal(f["srow"], np.float32(AFFINE[:3]))
    # inference.normalize: true -> the windows see the normalised volume instead
    ncfg = copy.deepcopy(cfg)
    ncfg["inference"]["normalize"] = True
    tn = _trainer(ncfg, root)
    tn.predict(root / "in", tmp_path / "norm")
    normed = DO.modality_normalize(raw.copy(), ["CT", "PET"], PRE)
    assert not np.array_equal(normed, raw)
    fn = _read_prediction(tmp_path / "norm" / "caseA_pred.nii.gz")
    assert np.array_equal(fn["data"], _expected_mask(tn, normed))
    assert not np.array_equal(fn["data"], f["data"])


def test_main_inference_mode(dev, predict_setup, tmp_path):
    import main as entry
    root, cfg, raw = predict_setup
    with pytest.raises(ValueError, match="--checkpoint"):
        entry.main(["--mode", "inference", "--config", str(root / "config.yaml"), "--input", str(root / "in")])
    with pytest.raises(ValueError, match="--input"):
        entry.main(["--mode", "inference", "--config", str(root / "config.yaml"), "--checkpoint",
                    str(root / "model.pth")])
    entry.main(["--mode", "inference", "--config", str(root / "config.yaml"), "--checkpoint", str(root / "model.pth"),
                "--input", str(root / "in"), "--output", str(tmp_path / "cli")])
    f = _read_prediction(tmp_path / "cli" / "caseA_pred.nii.gz")
    assert np.array_equal(f["data"], _expected_mask(_trainer(cfg, root), raw))
    assert not (tmp_path / "cli" / "caseB_pred.nii.gz").exists()
