"""Patch-based training on the device: foreground-biased crops with rotation and scaling drawn from volumes at
their own resolution (csrc/patch.hip), instead of squeezing every volume to img_size with DeviceResize.

The reference has RandomCrop and CenterCrop (src/data/transforms.py:142-212) but never wires them in, and its
default.yaml promises random_rotate: 15 and random_scale: [0.9, 1.1] without running them.  Here
data.patch.enabled: true makes the training loader draw patches_per_volume patches of data.patch.size from
every volume; validation then runs the sliding windows of Trainer.predict over the full-size volume.

Draws (draw_patch_params) come from a `random.Random` per patch in a fixed order and a fixed count, so the
stream never depends on the outcome of an earlier draw:
  1. rng.random() < foreground_prob           -> mode 1 (centre the patch on a foreground voxel) or 0
  2. three rng.randint(0, max_a) if max_a > 0 else 0, max_a = max(0, n_a - P_a), axis 0, 1, 2: exactly what
     the reference's RandomCrop consumes (its H, W, D order) -> the uniform start, and mode 1's fallback
  3. u = rng.random()                         -> which foreground voxel (always drawn)
  4. if rotate_deg > 0 or scale is set: rng.random() < affine_prob, the gate of the two steps below
  5. if rotate_deg > 0: three rng.uniform(-deg, deg), the angles about array axis 0, 1, 2
  6. if scale is set: one rng.uniform(lo, hi)
Steps 5 and 6 are drawn whatever the gate says.

The stream of patch j of volume i in epoch e is patch_rng(seed, e, i, j), a key with a domain tag of its own, so
the streams of DeviceAugment (sample_rng) are untouched and nothing depends on rank or world size.  DeviceAugment
(flip / rot90 / intensity / noise) then runs on each patch, unchanged, with sample_rng(seed, e, i * P + j).
"""
from __future__ import annotations

import ctypes
import math
import random
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Any, Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .._lib import lib, ptr, stream_handle
from ..distributed import ddp

PATCH_DEFAULTS: Dict[str, Any] = {"enabled": False, "size": [96, 96, 96], "patches_per_volume": 4,
                                  "foreground_prob": 0.5, "rotate_deg": 0, "scale": None, "affine_prob": 1.0,
                                  "pad_value": 0.0, "cache_gb": 0}
MAX_PATCHES = 16                    # patches per launch (csrc/patch.hip)
_M64 = (1 << 64) - 1
_PATCH_TAG = 0x7061746368           # "patch": the domain of the patch streams


def patch_config(cfg: Optional[Dict[str, Any]]) -> Dict[str, Any]:
    """data.patch with the defaults filled in; unknown keys and values out of range raise."""
    cfg = dict(cfg or {})
    unknown = sorted(set(cfg) - set(PATCH_DEFAULTS))
    if unknown:
        raise ValueError(f"data.patch: unknown key(s) {unknown}; known: {sorted(PATCH_DEFAULTS)}")
    out = {**PATCH_DEFAULTS, **cfg}
    size = out["size"]
    if not isinstance(size, (list, tuple)) or len(size) != 3 or any(int(s) != s or s < 1 for s in size):
        raise ValueError(f"data.patch.size: three positive integers (got {size})")
    out["size"] = [int(s) for s in size]
    P = out["patches_per_volume"]
    if int(P) != P or not 1 <= P <= MAX_PATCHES:
        raise ValueError(f"data.patch.patches_per_volume: 1..{MAX_PATCHES} (got {P})")
    out["patches_per_volume"] = int(P)
    for key in ("foreground_prob", "affine_prob"):
        if not 0.0 <= float(out[key]) <= 1.0:
            raise ValueError(f"data.patch.{key}: a probability (got {out[key]})")
    if not 0 <= float(out["rotate_deg"]) <= 180:
        raise ValueError(f"data.patch.rotate_deg: 0..180 degrees (got {out['rotate_deg']})")
    sc = out["scale"]
    if sc is not None:
        if not isinstance(sc, (list, tuple)) or len(sc) != 2 or not 0 < float(sc[0]) <= float(sc[1]):
            raise ValueError(f"data.patch.scale: null or [lo, hi] with 0 < lo <= hi (got {sc})")
        out["scale"] = [float(sc[0]), float(sc[1])]
    pad = out["pad_value"]
    if isinstance(pad, (list, tuple)):
        out["pad_value"] = [float(v) for v in pad]
    else:
        out["pad_value"] = float(pad)
    if float(out["cache_gb"]) < 0:
        raise ValueError(f"data.patch.cache_gb: >= 0 (got {out['cache_gb']})")
    return out


def affine_matrix(angles_deg: Sequence[float], scale: float) -> np.ndarray:
    """M = Rz Ry Rx / s in fp64: the map from patch offsets q (about the patch centre) to volume offsets, so
    s > 1 magnifies.  Axes are the array's: Rx turns the (1, 2) plane about axis 0 of [D, H, W], Ry the (2, 0)
    plane about axis 1, Rz the (0, 1) plane about axis 2; angles_deg lists them in that order."""
    ax, ay, az = (math.radians(float(v)) for v in angles_deg)
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=np.float64)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=np.float64)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=np.float64)
    return (Rz @ Ry @ Rx) / np.float64(scale)


@dataclass
class PatchParams:
    """One patch's draws: mode (0 uniform start, 1 foreground-centred), the uniform / fallback start, u, and
    the affine switch with its angles (degrees about axis 0, 1, 2), scale and matrix M = Rz Ry Rx / s."""
    mode: int = 0
    fallback_start: Tuple[int, int, int] = (0, 0, 0)
    u: float = 0.0
    affine: bool = False
    angles: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    scale: float = 1.0
    M: np.ndarray = field(default_factory=lambda: np.eye(3, dtype=np.float64))


def draw_patch_params(rng: random.Random, patch_cfg: Dict[str, Any], shape: Sequence[int]) -> PatchParams:
    """Consume `rng` in the module docstring's order for one patch of a volume of spatial `shape`."""
    size = patch_cfg.get("size", PATCH_DEFAULTS["size"])
    p = PatchParams()
    p.mode = int(rng.random() < patch_cfg.get("foreground_prob", PATCH_DEFAULTS["foreground_prob"]))
    start = []
    for a in range(3):
        max_a = max(0, int(shape[a]) - int(size[a]))
        start.append(rng.randint(0, max_a) if max_a > 0 else 0)
    p.fallback_start = tuple(start)
    p.u = rng.random()
    deg, sc = patch_cfg.get("rotate_deg", 0) or 0, patch_cfg.get("scale")
    if deg > 0 or sc is not None:
        p.affine = rng.random() < patch_cfg.get("affine_prob", 1.0)
        if deg > 0:
            p.angles = tuple(rng.uniform(-deg, deg) for _ in range(3))
        if sc is not None:
            p.scale = rng.uniform(sc[0], sc[1])
        if p.affine:
            p.M = affine_matrix(p.angles, p.scale)
    return p


def patch_rng(seed: int, epoch: int, index: int, j: int) -> random.Random:
    """The draw stream of patch `j` of global volume `index` in `epoch`: the same for every rank and world size,
    and disjoint from augment.sample_rng's keys (those stay below 2^192)."""
    return random.Random((_PATCH_TAG << 256) | ((int(seed) & _M64) << 192) | ((int(epoch) & _M64) << 128)
                         | ((int(index) & _M64) << 64) | (int(j) & _M64))


class DevicePatchSampler:
    """The three entry points of csrc/patch.hip on device tensors: image [C, D, H, W] fp32, label [D, H, W] int64 /
    uint8.  Nothing is read back to the host: the crop starts stay on the device between pick and sample."""

    def __init__(self, size: Sequence[int], pad_value=0.0):
        self.size = tuple(int(s) for s in size)
        self.pad_value = pad_value

    @staticmethod
    def _check(image: Optional[torch.Tensor], label: Optional[torch.Tensor]):
        if image is not None:
            if image.device.type != "cuda":
                raise RuntimeError(f"DevicePatchSampler: the device data path needs ROCm tensors (got "
                                   f"{image.device}); there is no CPU path")
            if image.dim() != 4 or image.dtype != torch.float32 or not image.is_contiguous():
                raise ValueError("DevicePatchSampler: contiguous image [C, D, H, W] float32")
        if label is not None:
            if label.device.type != "cuda":
                raise RuntimeError(f"DevicePatchSampler: the device data path needs ROCm tensors (got "
                                   f"{label.device}); there is no CPU path")
            if label.dim() != 3 or label.dtype not in (torch.int64, torch.uint8) or not label.is_contiguous():
                raise ValueError("DevicePatchSampler: contiguous label [D, H, W] int64 or uint8")
            if image is not None and (label.device != image.device or tuple(label.shape) != tuple(image.shape[1:])):
                raise ValueError("DevicePatchSampler: label [D, H, W] on the image's device")

    def _pads(self, C: int):
        pad = self.pad_value
        vals = [float(v) for v in pad] if isinstance(pad, (list, tuple)) else [float(pad)] * C
        if len(vals) != C:
            raise ValueError(f"DevicePatchSampler: {C} channels need {C} pad values (got {len(vals)})")
        return (ctypes.c_float * C)(*vals)

    def fg_counts(self, label: torch.Tensor) -> torch.Tensor:
        """Foreground voxels per chunk of the label (int32, on the device): cache it with the volume."""
        self._check(None, label)
        D, H, W = label.shape
        n = lib().mmseg_fg_chunks(D * H * W)
        if n < 1:
            raise ValueError(f"DevicePatchSampler: empty or oversized label {tuple(label.shape)}")
        counts = torch.empty(n, dtype=torch.int32, device=label.device)
        lib().mmseg_fg_count(ptr(label), label.element_size(), D, H, W, ptr(counts), stream_handle())
        return counts

    def pick(self, label: Optional[torch.Tensor], counts: Optional[torch.Tensor], params: Sequence[PatchParams],
             size: Optional[Sequence[int]] = None, shape: Optional[Sequence[int]] = None,
             device=None) -> torch.Tensor:
        """The crop starts of len(params) patches: int32 [P, 3] on the device.  Without a label (every mode 0)
        the volume's `shape` and `device` stand in for it."""
        self._check(None, label)
        P = len(params)
        if not 1 <= P <= MAX_PATCHES:
            raise ValueError(f"DevicePatchSampler: 1..{MAX_PATCHES} patches per launch (got {P})")
        pd, ph, pw = size if size is not None else self.size
        D, H, W = label.shape if label is not None else shape
        device = label.device if label is not None else device
        if counts is not None and (label is None or counts.dtype != torch.int32 or counts.device != device
                                   or counts.numel() != lib().mmseg_fg_chunks(D * H * W)):
            raise ValueError("DevicePatchSampler: counts as fg_counts(label) returns them")
        mode = (ctypes.c_int * P)(*[int(p.mode) for p in params])
        u = (ctypes.c_double * P)(*[float(p.u) for p in params])
        fb = (ctypes.c_int * (3 * P))(*[int(v) for p in params for v in p.fallback_start])
        starts = torch.empty(P, 3, dtype=torch.int32, device=device)
        lib().mmseg_patch_pick(ptr(label), label.element_size() if label is not None else 1, D, H, W, ptr(counts),
                               P, pd, ph, pw, ctypes.addressof(mode), ctypes.addressof(u), ctypes.addressof(fb),
                               ptr(starts), stream_handle())
        return starts

    def sample(self, image: torch.Tensor, label: Optional[torch.Tensor], starts: torch.Tensor,
               params: Sequence[PatchParams], size: Optional[Sequence[int]] = None):
        """(patches [P, C, pd, ph, pw] fp32, labels [P, pd, ph, pw] or None) in one launch."""
        self._check(image, label)
        P = len(params)
        if starts.dtype != torch.int32 or tuple(starts.shape) != (P, 3) or starts.device != image.device \
                or not starts.is_contiguous():
            raise ValueError(f"DevicePatchSampler: starts int32 [{P}, 3] on the image's device")
        pd, ph, pw = size if size is not None else self.size
        C, D, H, W = image.shape
        out = torch.empty(P, C, pd, ph, pw, dtype=torch.float32, device=image.device)
        lab_out = None if label is None else torch.empty(P, pd, ph, pw, dtype=label.dtype, device=label.device)
        affine = (ctypes.c_int * P)(*[int(bool(p.affine)) for p in params])
        M = (ctypes.c_double * (9 * P))(*[float(v) for p in params
                                         for v in np.asarray(p.M, dtype=np.float64).reshape(9)])
        pads = self._pads(C)
        lib().mmseg_patch_sample(ptr(image), C, D, H, W, ptr(label), label.element_size() if label is not None else 0,
                                 ptr(starts), P, pd, ph, pw, ctypes.addressof(affine), ctypes.addressof(M),
                                 ctypes.addressof(pads), ptr(out), ptr(lab_out), stream_handle())
        return out, lab_out

    def __call__(self, image: torch.Tensor, label: torch.Tensor, counts: Optional[torch.Tensor],
                 params: Sequence[PatchParams]):
        return self.sample(image, label, self.pick(label, counts, params), params)

    def center_crop(self, sample: Dict[str, Any], size: Sequence[int]) -> Dict[str, Any]:
        """The reference's CenterCrop (transforms.py:184-212): start max(0, (n - size) // 2) per axis; an axis
        shorter than the crop keeps its length."""
        image = sample["image"].contiguous()
        label = sample.get("label")
        label = label.contiguous() if label is not None else None
        self._check(image, label)
        n_ax = image.shape[1:]
        out_size = [min(int(size[a]), int(n_ax[a])) for a in range(3)]
        p = PatchParams(mode=0, fallback_start=tuple(max(0, (int(n_ax[a]) - int(size[a])) // 2) for a in range(3)))
        # mode 0 reads no label: the pick only carries the start to the device
        starts = self.pick(None, None, [p], out_size, shape=n_ax, device=image.device)
        img, lab = self.sample(image, label, starts, [p], out_size)
        sample["image"] = img[0]
        if label is not None:
            sample["label"] = lab[0]
        return sample


class DevicePatchDataset:
    """patches_per_volume patches of every volume of `source` (a DeviceNiftiDataset or DevicePhantomDataset:
    volume(i), __len__, mods, seed).  data.patch.cache_gb > 0 keeps decoded, normalised volumes, their labels and
    their chunk counts resident on the device, least recently used first out; a hit skips the file read, the
    decode, the normalisation and mmseg_fg_count, and gives bitwise the patches a miss gives."""

    def __init__(self, source, patch_cfg: Dict[str, Any], augment=None, seed: Optional[int] = None):
        self.source, self.cfg = source, patch_config(patch_cfg)
        self.mods = list(source.mods)
        self.seed = int(source.seed if seed is None else seed)
        self.P = self.cfg["patches_per_volume"]
        self.sampler = DevicePatchSampler(self.cfg["size"], self.cfg["pad_value"])
        self.augment = augment
        size = self.cfg["size"]
        if augment is not None and augment.cfg.get("random_rotate", 0) > 0 and size[0] != size[1]:
            raise ValueError(f"data.patch.size {size}: the quarter turns of data.augmentation.random_rotate swap "
                             "the first two axes, so they must be equal for patches to stack into a batch")
        self.capacity = int(float(self.cfg["cache_gb"]) * (1 << 30))
        self._cache: "OrderedDict[int, tuple]" = OrderedDict()
        self._bytes = 0
        self.hits = self.misses = 0

    def __len__(self):
        return len(self.source)

    @staticmethod
    def _nbytes(entry) -> int:
        return sum(t.numel() * t.element_size() for t in entry[:3])

    def volume(self, i: int):
        """(image, label, counts, patient_id) of volume i, from the cache when it is there."""
        hit = self._cache.get(i)
        if hit is not None:
            self._cache.move_to_end(i)
            self.hits += 1
            return hit
        self.misses += 1
        image, label, pid = self.source.volume(i)
        image, label = image.contiguous(), label.contiguous()
        entry = (image, label, self.sampler.fg_counts(label), pid)
        nb = self._nbytes(entry)
        if 0 < nb <= self.capacity:
            while self._cache and self._bytes + nb > self.capacity:
                _, old = self._cache.popitem(last=False)
                self._bytes -= self._nbytes(old)
            self._cache[i] = entry
            self._bytes += nb
        return entry

    def patches(self, i: int, epoch: int) -> List[Dict[str, Any]]:
        """The P patches of volume i as epoch `epoch` sees them, each in the reference's sample format."""
        image, label, counts, pid = self.volume(i)
        params = [draw_patch_params(patch_rng(self.seed, epoch, i, j), self.cfg, image.shape[1:])
                  for j in range(self.P)]
        imgs, labs = self.sampler(image, label, counts, params)
        out = []
        for j in range(self.P):
            sample = {"image": imgs[j], "label": labs[j]}
            if self.augment is not None:
                sample = self.augment(sample, epoch, i * self.P + j, self.seed)
            sample["patient_id"] = pid
            for m, mod in enumerate(self.mods):
                sample[mod] = sample["image"][m]
            out.append(sample)
        return out


class PatchLoader:
    """Batches of batch_size patches in the reference's batch format.  One epoch visits each volume of the rank's
    shard once (sharded and shuffled as DeviceLoader does it); the patches of one volume are consecutive.
    len = (volumes * P) // batch_size: a ragged tail is dropped, as the training DeviceLoader drops it."""

    def __init__(self, ds: DevicePatchDataset, batch_size: int, shuffle: bool = True, seed: int = 0,
                 rank: Optional[int] = None, world: Optional[int] = None):
        self.ds, self.B, self.shuffle, self.seed = ds, int(batch_size), shuffle, seed
        self.epoch = 0
        r, w = ddp.rank() if rank is None else rank, ddp.world() if world is None else world
        self.idx = ddp.shard_indices(len(ds), r, w, pad=True) if w > 1 else list(range(len(ds)))

    def __len__(self):
        return (len(self.idx) * self.ds.P) // self.B

    def __iter__(self) -> Iterator[Dict[str, Any]]:
        order = list(self.idx)
        if self.shuffle:
            rng = np.random.Generator(np.random.PCG64(self.seed + self.epoch))
            order = [order[k] for k in rng.permutation(len(order))]
        epoch = self.epoch
        self.epoch += 1
        pending: List[Dict[str, Any]] = []
        left = len(self)
        for i in order:
            if left == 0:
                break
            pending.extend(self.ds.patches(i, epoch))
            while len(pending) >= self.B and left > 0:
                items, pending = pending[:self.B], pending[self.B:]
                left -= 1
                batch = {"image": torch.stack([it["image"] for it in items]),
                         "label": torch.stack([it["label"] for it in items]),
                         "patient_id": [it["patient_id"] for it in items]}
                for m, mod in enumerate(self.ds.mods):
                    batch[mod] = batch["image"][:, m:m + 1]
                yield batch
