"""NIfTI datasets on the device data path: the counterpart of the reference's MultiModalDataset
(src/data/dataset.py:19-117) and get_dataset (dataset.py:179-217).

The host reads (and gunzips) each file and parses its header (utils/nifti.py); the voxel block goes to the
device as the file holds it -- 2 bytes per voxel for an int16 CT instead of 4 -- and mmseg_nifti_decode
(csrc/nifti.hip) unswaps, rescales, casts and permutes it into the [X, Y, Z] fp32 channel that
DeviceModalityNormalize -> DeviceAugment -> DeviceResize (get_transforms' order, transforms.py:407-451) take.
argmax_encode is the way back for a prediction: argmax over the classes fused with the permutation to file
order, so only X*Y*Z bytes return to the host.
"""
from __future__ import annotations

import csv
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

from .._lib import lib, ptr, stream_handle
from ..utils.nifti import NiftiHeader, read_nifti_raw
from .device import DeviceModalityNormalize, DeviceResize, _require_device

SUPPORTED_MODALITIES = ["CT", "PET", "MRI", "US"]
SPLIT_KEYS = {"train": "train_csv", "val": "val_csv", "test": "test_csv"}
LABEL_DTYPES = {"int64": torch.int64, "uint8": torch.uint8}


class HostStager:
    """Raw voxel blocks to the device through one pinned buffer that grows as needed.  The H2D copy is
    asynchronous, so the buffer is overwritten only after the event recorded behind the previous copy."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.buf: Optional[torch.Tensor] = None
        self.event: Optional[torch.cuda.Event] = None

    def upload(self, raw) -> torch.Tensor:
        """raw: a uint8 numpy array -> a uint8 device tensor holding the same bytes (the copy may be in flight;
        work queued on the current stream is ordered behind it)."""
        n = int(raw.size)
        if self.event is not None:
            self.event.synchronize()          # the previous copy has left the buffer
        if self.buf is None or self.buf.numel() < n:
            self.buf = torch.empty(max(n, 1 << 20), dtype=torch.uint8, pin_memory=True)
        self.buf.numpy()[:n] = raw
        dev = torch.empty(n, dtype=torch.uint8, device=self.device)
        dev.copy_(self.buf[:n], non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()
        return dev


def _decode_args(h: NiftiHeader):
    X, Y, Z = h.shape
    return h.datatype, int(h.swapped), X, Y, Z, int(h.scaled), float(h.scl_slope), float(h.scl_inter)


def decode_volume(h: NiftiHeader, raw_dev: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The file's voxel block (uint8 device tensor, h.nbytes bytes) -> [X, Y, Z] fp32 on the device, as
    load_nifti(path, dtype=np.float32) gives it.  `out`: a contiguous [X, Y, Z] fp32 tensor to fill."""
    _require_device(raw_dev, "decode_volume")
    if raw_dev.dtype != torch.uint8 or raw_dev.numel() != h.nbytes or not raw_dev.is_contiguous():
        raise ValueError(f"decode_volume: {h.nbytes} contiguous raw bytes expected (got {raw_dev.numel()})")
    if out is None:
        out = torch.empty(h.shape, dtype=torch.float32, device=raw_dev.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != tuple(h.shape) or not out.is_contiguous():
        raise ValueError(f"decode_volume: out must be a contiguous float32 {tuple(h.shape)}")
    lib().mmseg_nifti_decode(ptr(raw_dev), *_decode_args(h), ptr(out), stream_handle())
    return out


def decode_label(h: NiftiHeader, raw_dev: torch.Tensor, dtype=torch.int64) -> torch.Tensor:
    """As load_nifti(path, dtype=np.int64): the scaled double truncated toward zero, [X, Y, Z] int64 or uint8."""
    _require_device(raw_dev, "decode_label")
    if dtype not in (torch.int64, torch.uint8):
        raise ValueError("decode_label: int64 or uint8 labels")
    if raw_dev.dtype != torch.uint8 or raw_dev.numel() != h.nbytes or not raw_dev.is_contiguous():
        raise ValueError(f"decode_label: {h.nbytes} contiguous raw bytes expected (got {raw_dev.numel()})")
    out = torch.empty(h.shape, dtype=dtype, device=raw_dev.device)
    lib().mmseg_nifti_decode_label(ptr(raw_dev), *_decode_args(h), ptr(out), out.element_size(), stream_handle())
    return out


def argmax_encode(logits: torch.Tensor) -> torch.Tensor:
    """logits [C, X, Y, Z] fp32 on the device -> the class mask as X*Y*Z uint8 in NIfTI file order (x fastest)."""
    _require_device(logits, "argmax_encode")
    if logits.dim() != 4 or logits.dtype != torch.float32:
        raise ValueError("argmax_encode: logits [C, X, Y, Z] float32")
    logits = logits.contiguous()
    C, X, Y, Z = logits.shape
    out = torch.empty(X * Y * Z, dtype=torch.uint8, device=logits.device)
    lib().mmseg_argmax_encode(ptr(logits), C, X, Y, Z, ptr(out), stream_handle())
    return out


def load_modalities(paths: Sequence[Path], stager: HostStager) -> Tuple[torch.Tensor, NiftiHeader]:
    """One file per modality -> ([M, X, Y, Z] fp32 on the device, the first file's header)."""
    image, first = None, None
    for m, path in enumerate(paths):
        h, raw = read_nifti_raw(path)
        if first is None:
            first = h
            image = torch.empty((len(paths),) + tuple(h.shape), dtype=torch.float32, device=stager.device)
        elif h.shape != first.shape:
            raise ValueError(f"{path}: shape {h.shape} differs from {paths[0]}'s {first.shape}")
        decode_volume(h, stager.upload(raw), image[m])
    return image, first


def read_data_list(config: Dict[str, Any], split: str) -> List[Dict[str, str]]:
    """data_root/<split>_csv as a list of rows, with the reference's checks (dataset.py:62-69, 195-208)."""
    data = config["data"]
    if split not in SPLIT_KEYS:
        raise ValueError(f"Invalid split: {split}")
    if "data_root" not in data or SPLIT_KEYS[split] not in data:
        raise ValueError(f"data.data_root and data.{SPLIT_KEYS[split]} are needed for the '{split}' split "
                         "(or data.synthetic for phantoms)")
    csv_path = Path(data["data_root"]) / data[SPLIT_KEYS[split]]
    if not csv_path.exists():
        raise FileNotFoundError(f"Data list not found: {csv_path}")
    for mod in data["modalities"]:
        if mod not in SUPPORTED_MODALITIES:
            raise ValueError(f"Unsupported modality: {mod}. Supported: {SUPPORTED_MODALITIES}")
    with open(csv_path, newline="") as f:
        reader = csv.DictReader(f)
        columns = [c.strip() for c in (reader.fieldnames or [])]
        for col in ["patient_id"] + list(data["modalities"]) + ["label"]:
            if col not in columns:
                raise ValueError(f"Required column '{col}' not found in data_list ({csv_path})")
        return [{k.strip(): (v or "").strip() for k, v in row.items() if k is not None} for row in reader]


class DeviceNiftiDataset:
    """Sample i = row i of the split's CSV, decoded, normalised, augmented (training) and resized on the GPU,
    in the reference's batch format.  Serves DeviceLoader like DevicePhantomDataset (get, __len__, mods)."""

    def __init__(self, config: Dict[str, Any], rows: List[Dict[str, str]], mode: str = "train", device=None,
                 augment=None, resize: bool = True):
        data = config["data"]
        self.rows, self.mode, self.mods = list(rows), mode, list(data["modalities"])
        self.root = Path(data["data_root"])
        self._device = torch.device(device) if device is not None else None     # None: the current GPU, on first use
        self.seed = int(config.get("experiment", {}).get("seed", 0))
        name = str(data.get("label_dtype", "int64"))
        if name not in LABEL_DTYPES:
            raise ValueError(f"data.label_dtype: int64 (the reference's) or uint8 (got {name})")
        self.label_dtype = LABEL_DTYPES[name]
        self.norm = DeviceModalityNormalize(config)
        img_size = config["model"].get("backbone", {}).get("img_size", [96, 96, 96])
        # transforms.py:446-449; resize=False (data.patch.enabled): volumes keep their own size
        self.resize = DeviceResize(img_size) if resize and len(img_size) == 3 else None
        self.augment = augment if mode == "train" else None
        self._stager: Optional[HostStager] = None      # no GPU is touched before the first sample

    @property
    def device(self) -> torch.device:
        if self._device is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        return self._device

    @property
    def stager(self) -> HostStager:
        if self._stager is None:
            self._stager = HostStager(self.device)
        return self._stager

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, i: int) -> Dict[str, Any]:
        return self.get(i, 0)

    def _path(self, row: Dict[str, str], col: str) -> Path:
        p = self.root / row[col]
        if not p.exists():
            raise FileNotFoundError(f"{col} file of patient {row['patient_id']} not found: {p}")
        return p

    def volume(self, i: int) -> Tuple[torch.Tensor, torch.Tensor, str]:
        """Row i decoded and normalised at its own size: (image [M, X, Y, Z] fp32, label [X, Y, Z], patient_id)."""
        row = self.rows[i]
        paths = [self._path(row, mod) for mod in self.mods]
        image, first = load_modalities(paths, self.stager)
        lpath = self._path(row, "label")
        lh, lraw = read_nifti_raw(lpath)
        if lh.shape != first.shape:
            raise ValueError(f"{lpath}: label shape {lh.shape} differs from {paths[0]}'s {first.shape}")
        label = decode_label(lh, self.stager.upload(lraw), self.label_dtype)
        self.norm(image)
        return image, label, row["patient_id"]

    def get(self, i: int, epoch: int) -> Dict[str, Any]:
        row = self.rows[i]
        image, label, _ = self.volume(i)
        sample = {"image": image, "label": label}
        if self.augment is not None:
            sample = self.augment(sample, epoch, i, self.seed)
        if self.resize is not None:
            sample = self.resize(sample)
        sample["patient_id"] = row["patient_id"]
        for m, mod in enumerate(self.mods):
            sample[mod] = sample["image"][m]
        return sample


def find_cases(input_path: Path, modalities: Sequence[str]) -> List[Tuple[str, List[Path]]]:
    """The cases of a prediction folder (trainer.py:326-354): <input>/<modality.lower()>/<case>.nii[.gz];
    a case that lacks a modality is left out.  Sorted (the reference iterates a set)."""
    names = set()
    for mod in modalities:
        mod_dir = input_path / mod.lower()
        if mod_dir.is_dir():
            for f in mod_dir.iterdir():
                if f.name.endswith(".nii.gz"):
                    names.add(f.name[:-7])
                elif f.name.endswith(".nii"):
                    names.add(f.name[:-4])
    cases = []
    for name in sorted(names):
        paths = []
        for mod in modalities:
            p = input_path / mod.lower() / f"{name}.nii.gz"
            if not p.exists():
                p = input_path / mod.lower() / f"{name}.nii"
            if p.exists():
                paths.append(p)
        if len(paths) == len(modalities):
            cases.append((name, paths))
    return cases
