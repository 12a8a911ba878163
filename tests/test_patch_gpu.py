"""Patch sampler on the device (csrc/patch.hip, mmseg_amd/data/patch.py).

mmseg_patch_pick is held bitwise to np.flatnonzero(label > 0)[k] plus the clamp rule (tests/patch_ref.py), the
copy path of mmseg_patch_sample bitwise to the reference's own RandomCrop / CenterCrop outputs
(tests/golden/patch.npz), and the affine path bitwise to the fp64 restatement that tests/test_patch_cpu.py holds
to scipy.  The loader tests pin rank independence, the volume cache and the opt-in; the last test trains and
validates end to end on NIfTI files."""
import copy
import os

import numpy as np
import pytest
import torch

import mmseg_amd  # noqa: F401
from mmseg_amd._lib import MmsegError, lib, ptr, stream_handle
from mmseg_amd.data.dataloader import get_dataloader
from mmseg_amd.data.device import DeviceLoader
from mmseg_amd.data.patch import DevicePatchDataset, DevicePatchSampler, PatchLoader, PatchParams
from tests import nifti_ref as NR
from tests import patch_cases as PC
from tests import patch_ref as PR

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "patch.npz"))
SIZES = [tuple(int(v) for v in s) for s in GOLD["sizes"]]
SEEDS = [int(s) for s in GOLD["seeds"]]
LABEL_DTYPES = {8: (torch.int64, np.int64), 1: (torch.uint8, np.uint8)}
US = [0.0, 2.0 ** -40, 0.5, 1.0 - 2.0 ** -53]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _labels(shape):
    """name -> label [D, H, W] int64: no foreground, one voxel (in the last chunk), only the last voxel, every
    voxel, and a sparse random one whose foreground spreads over every chunk."""
    V = int(np.prod(shape))
    out = {"none": np.zeros(V, dtype=np.int64), "one": np.zeros(V, dtype=np.int64),
           "last": np.zeros(V, dtype=np.int64), "all": np.full(V, 3, dtype=np.int64)}
    out["one"][(V * 7) // 8] = 2
    out["last"][V - 1] = 1
    rng = np.random.Generator(np.random.PCG64(V))
    out["sparse"] = (rng.random(V) < 0.03).astype(np.int64) * rng.integers(1, 4, V)
    return {k: v.reshape(shape) for k, v in out.items()}


@pytest.mark.parametrize("label_bytes", [8, 1])
@pytest.mark.parametrize("shape,sizes", [((7, 9, 11), [(4, 4, 6), (4, 12, 6), (9, 3, 11)]),
                                         ((40, 33, 29), [(16, 16, 16), (16, 40, 8), (48, 8, 32)])])
def test_pick_bitwise(dev, shape, sizes, label_bytes):
    tdt, ndt = LABEL_DTYPES[label_bytes]
    V = int(np.prod(shape))
    nchunks = lib().mmseg_fg_chunks(V)
    assert nchunks == -(-V // 4096) and (nchunks == 1) == (shape == (7, 9, 11))
    for name, lab in _labels(shape).items():
        lab = lab.astype(ndt)
        dlab = torch.from_numpy(lab).to(dev)
        n = int((lab > 0).sum())
        for size in sizes:
            sampler = DevicePatchSampler(size)
            counts = sampler.fg_counts(dlab)
            ref_counts = np.add.reduceat((lab.reshape(-1) > 0).astype(np.int32), np.arange(0, V, 4096))
            assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), ref_counts), (name, size)
            fb = tuple(max(0, shape[a] - size[a]) // 2 for a in range(3))
            top = tuple(max(0, shape[a] - size[a]) for a in range(3))
            params = [PatchParams(mode=1, u=u, fallback_start=fb) for u in US]
            params += [PatchParams(mode=1, u=k / 11.0 + 0.01, fallback_start=top) for k in range(11)]
            params += [PatchParams(mode=0, u=0.5, fallback_start=top)]
            assert len(params) == 16
            got = sampler.pick(dlab, counts, params).cpu().numpy()
            want = np.array([PR.pick_start(lab, size, p.mode, p.u, p.fallback_start) for p in params])
            assert got.dtype == np.int32 and np.array_equal(got, want), (name, size, got, want)
            if name == "all":      # u = 0 and the largest u clamp at the near and the far end of every axis
                for a in range(3):
                    if shape[a] >= size[a]:
                        assert got[0, a] == 0 and got[3, a] == shape[a] - size[a]
            if name in ("one", "last"):
                assert n == 1 and (got[:15] == got[0]).all()
            if name == "none":
                assert n == 0 and (got[:4] == np.array(PR.pick_start(lab, size, 0, 0.0, fb))).all()
            for a in range(3):
                if shape[a] < size[a]:
                    assert (got[:, a] == -((size[a] - shape[a]) // 2)).all()


def test_pick_on_an_unaligned_label_view(dev):
    """A label that does not start on a 16-byte boundary takes mmseg_fg_count's scalar path."""
    shape = (40, 33, 29)
    lab = _labels(shape)["sparse"].astype(np.uint8)
    buf = torch.zeros(lab.size + 16, dtype=torch.uint8, device=dev)
    view = buf[3:3 + lab.size].view(shape)
    view.copy_(torch.from_numpy(lab))
    assert view.data_ptr() % 16 != 0
    sampler = DevicePatchSampler((16, 16, 16))
    aligned = sampler.fg_counts(torch.from_numpy(lab).to(dev))
    assert torch.equal(sampler.fg_counts(view), aligned)
    p = [PatchParams(mode=1, u=u, fallback_start=(0, 0, 0)) for u in US]
    assert torch.equal(sampler.pick(view, aligned, p), sampler.pick(torch.from_numpy(lab).to(dev), aligned, p))


def _starts(dev, rows):
    return torch.tensor(rows, dtype=torch.int32, device=dev).reshape(-1, 3)


@pytest.mark.parametrize("label_bytes", [8, 1])
@pytest.mark.parametrize("si", range(len(SIZES)))
def test_copy_path_is_the_reference_crop(dev, si, label_bytes):
    tdt, ndt = LABEL_DTYPES[label_bytes]
    size = SIZES[si]
    image, label = GOLD["image_a"], GOLD["label_a"].astype(ndt)
    dimg, dlab = torch.from_numpy(image).to(dev), torch.from_numpy(label).to(dev)
    sampler = DevicePatchSampler(size, pad_value=[7.0, -7.0])
    params = [PatchParams(mode=0, fallback_start=tuple(int(v) for v in GOLD[f"draws_{si}_{seed}"]))
              for seed in SEEDS]
    img, lab = sampler(dimg, dlab, None, params)            # pick (mode 0) + sample, one launch each
    assert img.shape == (len(SEEDS), 2) + size and lab.shape == (len(SEEDS),) + size and lab.dtype == tdt
    for j, seed in enumerate(SEEDS):
        assert np.array_equal(_bits(img[j].cpu().numpy()), _bits(GOLD[f"crop_image_{si}_{seed}"])), seed
        assert np.array_equal(lab[j].cpu().numpy(), GOLD[f"crop_label_{si}_{seed}"].astype(ndt)), seed
    # starts 0 and max on every axis (what RandomCrop slices there), and the input is left alone
    top = [image.shape[1 + a] - size[a] for a in range(3)]
    corners = [(0, 0, 0), tuple(top), (top[0], 0, top[2]), (0, top[1], 0)]
    img, lab = sampler.sample(dimg, dlab, _starts(dev, corners), [PatchParams()] * 4)
    for j, st in enumerate(corners):
        sl = tuple(slice(st[a], st[a] + size[a]) for a in range(3))
        assert np.array_equal(_bits(img[j].cpu().numpy()), _bits(image[(slice(None),) + sl])), st
        assert np.array_equal(lab[j].cpu().numpy(), label[sl]), st
    assert np.array_equal(_bits(dimg.cpu().numpy()), _bits(image)) and np.array_equal(dlab.cpu().numpy(), label)
    # CenterCrop
    s = sampler.center_crop({"image": dimg, "label": dlab}, size)
    assert np.array_equal(_bits(s["image"].cpu().numpy()), _bits(GOLD[f"center_image_{si}"]))
    assert np.array_equal(s["label"].cpu().numpy(), GOLD[f"center_label_{si}"].astype(ndt))
    s = sampler.center_crop({"image": dimg}, size)           # no label
    assert np.array_equal(_bits(s["image"].cpu().numpy()), _bits(GOLD[f"center_image_{si}"])) and "label" not in s


@pytest.mark.parametrize("label_bytes", [8, 1])
def test_copy_path_pads_a_small_volume(dev, label_bytes):
    """(5, 9, 20) -> (8, 8, 16): rows of 80 bytes, so the starts 0 and 4 along W take the 16-byte vectors and 1..3
    the scalars; planes 0, 6 and 7 of the patch are padding."""
    tdt, ndt = LABEL_DTYPES[label_bytes]
    size, pad = SIZES[0], (2.5, -3.0)
    image, label = GOLD["image_b"], GOLD["label_b"].astype(ndt)
    dimg, dlab = torch.from_numpy(image).to(dev), torch.from_numpy(label).to(dev)
    sampler = DevicePatchSampler(size, pad_value=list(pad))
    fbs = [(0,) + tuple(int(v) for v in GOLD[f"small_draws_{seed}"]) for seed in SEEDS[:2]]
    fbs += [(0, 0, 0), (0, 1, 4), (0, 0, 1), (0, 1, 3)]
    params = [PatchParams(mode=0, fallback_start=fb) for fb in fbs]
    starts = sampler.pick(dlab, None, params)
    assert np.array_equal(starts.cpu().numpy(), np.array([(-1,) + fb[1:] for fb in fbs]))
    img, lab = sampler.sample(dimg, dlab, starts, params)
    for j, fb in enumerate(fbs):
        ref_img, ref_lab = PR.sample_copy(image, label, (-1,) + fb[1:], size, pad)
        assert np.array_equal(_bits(img[j].cpu().numpy()), _bits(ref_img)), fb
        assert np.array_equal(lab[j].cpu().numpy(), ref_lab), fb
    for j, seed in enumerate(SEEDS[:2]):                      # the reference's own slice is the interior
        assert np.array_equal(_bits(img[j, :, 1:6].cpu().numpy()), _bits(GOLD[f"small_image_{seed}"]))
        assert np.array_equal(lab[j, 1:6].cpu().numpy(), GOLD[f"small_label_{seed}"].astype(ndt))
    s = sampler.center_crop({"image": dimg, "label": dlab}, size)     # CenterCrop keeps the short axis short
    assert np.array_equal(_bits(s["image"].cpu().numpy()), _bits(GOLD["small_center_image"]))
    assert np.array_equal(s["label"].cpu().numpy(), GOLD["small_center_label"].astype(ndt))
    # a patch wholly outside, and one that sticks out at both ends of W
    far = _starts(dev, [(9, 0, 0), (0, 0, -3), (-1, -2, 9)])
    img, lab = sampler.sample(dimg, dlab, far, [PatchParams()] * 3)
    for j, st in enumerate([(9, 0, 0), (0, 0, -3), (-1, -2, 9)]):
        ref_img, ref_lab = PR.sample_copy(image, label, st, size, pad)
        assert np.array_equal(_bits(img[j].cpu().numpy()), _bits(ref_img)), st
        assert np.array_equal(lab[j].cpu().numpy(), ref_lab), st


@pytest.mark.parametrize("label_bytes", [8, 1])
def test_affine_path_bitwise_restatement(dev, label_bytes):
    tdt, ndt = LABEL_DTYPES[label_bytes]
    image, label = PC.volume()
    label = label.astype(ndt)
    dimg, dlab = torch.from_numpy(image).to(dev), torch.from_numpy(label).to(dev)
    cases = PC.affine_cases()
    sampler = DevicePatchSampler(PC.PATCH, pad_value=list(PC.PAD))
    params = [PatchParams(affine=True, M=M) for _, M in cases]
    img, lab = sampler.sample(dimg, dlab, _starts(dev, [st for st, _ in cases]), params)
    for j, (start, M) in enumerate(cases):
        ref = PR.sample_affine_image(image, start, PC.PATCH, M, PC.PAD)
        assert np.array_equal(_bits(img[j].cpu().numpy()), _bits(ref)), start
        assert np.array_equal(lab[j].cpu().numpy(), PR.sample_affine_label(label, start, PC.PATCH, M)), start
        inside = PR.sample_affine_image(image, start, PC.PATCH, M, (1e6, 1e6))
        assert (np.abs(inside) > 1e3).any() and (np.abs(inside) < 10).any()     # padding and volume both show
    # the identity matrix through the affine path is the copy
    eye = [PatchParams(affine=True, M=np.eye(3))] * 2
    st = _starts(dev, [PC.STARTS[0], PC.STARTS[1]])
    a_img, a_lab = sampler.sample(dimg, dlab, st, eye)
    c_img, c_lab = sampler.sample(dimg, dlab, st, [PatchParams()] * 2)
    assert torch.equal(a_img, c_img) and torch.equal(a_lab, c_lab)
    img_only, none = sampler.sample(dimg, None, _starts(dev, [st_ for st_, _ in cases]), params)
    assert none is None and torch.equal(img_only, img)


def test_one_launch_of_three_equals_three_launches(dev):
    image, label = PC.volume()
    dimg, dlab = torch.from_numpy(image).to(dev), torch.from_numpy(label).to(dev)
    cases = PC.affine_cases()
    sampler = DevicePatchSampler(PC.PATCH, pad_value=list(PC.PAD))
    params = [PatchParams(mode=1, u=0.37, fallback_start=(0, 0, 0)),
              PatchParams(mode=0, fallback_start=(5, 2, 8), affine=True, M=cases[0][1]),
              PatchParams(mode=1, u=0.91, fallback_start=(1, 1, 1), affine=True, M=cases[3][1])]
    counts = sampler.fg_counts(dlab)
    img, lab = sampler(dimg, dlab, counts, params)
    for j, p in enumerate(params):
        one_img, one_lab = sampler(dimg, dlab, counts, [p])
        assert torch.equal(one_img[0], img[j]) and torch.equal(one_lab[0], lab[j]), j
    assert not torch.equal(img[0], img[1]) and not torch.equal(img[1], img[2])


def test_argument_validation(dev):
    L, s = lib(), stream_handle()
    img = torch.zeros(2, 4, 4, 4, device=dev)
    lab = torch.zeros(4, 4, 4, dtype=torch.uint8, device=dev)
    out = torch.zeros(2, 2, 2, 2, device=dev)
    lout = torch.zeros(2, 2, 2, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    st = torch.zeros(3, dtype=torch.int32, device=dev)
    import ctypes
    one, zero = (ctypes.c_int * 1)(1), (ctypes.c_int * 1)(0)
    u, bad_u = (ctypes.c_double * 1)(0.5), (ctypes.c_double * 1)(1.0)
    fb, bad_fb = (ctypes.c_int * 3)(0, 0, 0), (ctypes.c_int * 3)(0, 3, 0)
    pad = (ctypes.c_float * 4)(0, 0, 0, 0)
    M = (ctypes.c_double * 9)(*([float("nan")] * 9))
    A = ctypes.addressof
    with pytest.raises(MmsegError, match="int64 or uint8"):
        L.mmseg_fg_count(ptr(lab), 4, 4, 4, 4, ptr(cnt), s)
    with pytest.raises(MmsegError):
        L.mmseg_fg_count(None, 1, 4, 4, 4, ptr(cnt), s)
    with pytest.raises(MmsegError, match="patches"):
        L.mmseg_patch_pick(ptr(lab), 1, 4, 4, 4, ptr(cnt), 17, 2, 2, 2, A(one), A(u), A(fb), ptr(st), s)
    with pytest.raises(MmsegError, match=r"u in \[0, 1\)"):
        L.mmseg_patch_pick(ptr(lab), 1, 4, 4, 4, ptr(cnt), 1, 2, 2, 2, A(one), A(bad_u), A(fb), ptr(st), s)
    with pytest.raises(MmsegError, match="leaves the volume"):
        L.mmseg_patch_pick(ptr(lab), 1, 4, 4, 4, ptr(cnt), 1, 2, 2, 2, A(zero), A(u), A(bad_fb), ptr(st), s)
    with pytest.raises(MmsegError, match="mode 1 needs"):
        L.mmseg_patch_pick(ptr(lab), 1, 4, 4, 4, None, 1, 2, 2, 2, A(one), A(u), A(fb), ptr(st), s)
    with pytest.raises(MmsegError, match="channels"):
        L.mmseg_patch_sample(ptr(img), 5, 4, 4, 4, None, 0, ptr(st), 1, 2, 2, 2, A(zero), None, A(pad), ptr(out),
                             None, s)
    with pytest.raises(MmsegError, match="matrix"):
        L.mmseg_patch_sample(ptr(img), 2, 4, 4, 4, None, 0, ptr(st), 1, 2, 2, 2, A(one), None, A(pad), ptr(out),
                             None, s)
    with pytest.raises(MmsegError, match="finite"):
        L.mmseg_patch_sample(ptr(img), 2, 4, 4, 4, None, 0, ptr(st), 1, 2, 2, 2, A(one), A(M), A(pad), ptr(out),
                             None, s)
    with pytest.raises(MmsegError, match="out of place"):
        L.mmseg_patch_sample(ptr(img), 2, 4, 4, 4, ptr(lab), 1, ptr(st), 1, 2, 2, 2, A(zero), None, A(pad),
                             ptr(out), ptr(lab), s)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DevicePatchSampler((2, 2, 2)).fg_counts(lab.cpu())
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and int(lout.sum()) == 0 and int(st.sum()) == 0     # nothing was launched


# ------------------------------------------------------------------------------------------------ loader
def _phantom_config(patch=None, n_train=4, batch=2):
    from bench import make_config
    cfg = make_config("unet", batch, "fp32", out_channels=3)
    cfg["data"]["synthetic"] = {"n_train": n_train, "n_val": 1, "size": 24, "seed": 77, "device": True}
    if patch is not None:
        cfg["data"]["patch"] = patch
    return cfg


PATCH = {"enabled": True, "size": [16, 16, 16], "patches_per_volume": 2, "foreground_prob": 0.5, "rotate_deg": 15,
         "scale": [0.9, 1.1], "affine_prob": 0.5}


def _by_patch(loader):
    """{(patient_id, position among that volume's patches): (image, label)} of one epoch."""
    out, seen = {}, {}
    for b in loader:
        assert set(b) == {"image", "label", "patient_id", "CT", "PET"}
        assert b["image"].shape == (2, 2, 16, 16, 16) and b["label"].shape == (2, 16, 16, 16)
        assert b["CT"].shape == (2, 1, 16, 16, 16) and torch.equal(b["PET"], b["image"][:, 1:2])
        for k, pid in enumerate(b["patient_id"]):
            j = seen[pid] = seen.get(pid, -1) + 1
            out[(pid, j)] = (b["image"][k].clone(), b["label"][k].clone())
    return out


def test_loader_is_independent_of_rank_and_world(dev):
    cfg = _phantom_config(PATCH)
    cfg["data"]["augmentation"] = {"enabled": True, "random_flip": True, "random_rotate": 1, "random_intensity": 0.1}
    ld = get_dataloader(cfg, "train")
    assert isinstance(ld, PatchLoader) and isinstance(ld.ds, DevicePatchDataset) and len(ld) == 4
    whole = _by_patch(ld)
    assert len(whole) == 8 and {k[1] for k in whole} == {0, 1}
    parts = {}
    for r in (0, 1):
        shard = PatchLoader(ld.ds, 2, shuffle=True, seed=ld.seed, rank=r, world=2)
        assert len(shard) == 2
        got = _by_patch(shard)
        assert not set(got) & set(parts)
        parts.update(got)
    assert set(parts) == set(whole)
    for k in whole:
        assert torch.equal(parts[k][0], whole[k][0]) and torch.equal(parts[k][1], whole[k][1]), k
    # the next epoch draws other patches, and another loader on the same config repeats this one
    second = _by_patch(ld)
    assert any(not torch.equal(second[k][0], whole[k][0]) for k in whole)
    again = _by_patch(get_dataloader(cfg, "train"))
    assert all(torch.equal(again[k][0], whole[k][0]) and torch.equal(again[k][1], whole[k][1]) for k in whole)
    # consecutive: both patches of a volume sit in one batch here (P == batch size)
    ld.epoch = 0
    assert all(b["patient_id"][0] == b["patient_id"][1] for b in ld)


def test_cached_epoch_equals_uncached_epoch(dev):
    plain = get_dataloader(_phantom_config(PATCH), "train")
    cached = get_dataloader(_phantom_config({**PATCH, "cache_gb": 0.5}), "train")
    want = _by_patch(plain)
    first = _by_patch(cached)
    assert cached.ds.misses == 4 and cached.ds.hits == 0 and plain.ds._bytes == 0 and len(plain.ds._cache) == 0
    cached.epoch = 0
    hit = _by_patch(cached)
    assert cached.ds.misses == 4 and cached.ds.hits == 4
    for k in want:
        for got in (first, hit):
            assert torch.equal(got[k][0], want[k][0]) and torch.equal(got[k][1], want[k][1]), k
    # least recently used out: room for two volumes (2 x 24^3 fp32 + 24^3 int64 + the counts, each)
    one = 2 * 24 ** 3 * 4 + 24 ** 3 * 8 + 4 * lib().mmseg_fg_chunks(24 ** 3)
    small = get_dataloader(_phantom_config({**PATCH, "cache_gb": (2 * one + 8) / 2 ** 30}), "train")
    ds = small.ds
    for i in (0, 1, 0, 2):
        ds.volume(i)
    assert list(ds._cache) == [0, 2] and ds._bytes == 2 * one and (ds.hits, ds.misses) == (1, 3)


def test_foreground_patches_hold_foreground(dev):
    cfg = _phantom_config({"enabled": True, "size": [8, 8, 8], "patches_per_volume": 8, "foreground_prob": 1.0},
                          batch=8)
    ld = get_dataloader(cfg, "train")
    n = 0
    for b in ld:
        assert b["label"].shape == (8, 8, 8, 8)
        assert (b["label"].reshape(8, -1) > 0).any(dim=1).all()
        n += 8
    assert n == 32
    # the uniform crops of these phantoms do miss it now and then: the bias is what the assertion above sees
    cfg["data"]["patch"]["foreground_prob"] = 0.0
    miss = sum(int((~(b["label"].reshape(8, -1) > 0).any(dim=1)).sum()) for b in get_dataloader(cfg, "train"))
    assert miss > 0


def test_without_enabled_the_loader_is_unchanged(dev):
    base = _phantom_config(None)
    off = _phantom_config({"size": [16, 16, 16], "patches_per_volume": 2})          # no `enabled`
    for split in ("train", "val"):
        a, b = get_dataloader(base, split), get_dataloader(off, split)
        assert type(a) is type(b) is DeviceLoader and len(a) == len(b)
        ba, bb = next(iter(a)), next(iter(b))
        assert ba["patient_id"] == bb["patient_id"] and ba["image"].shape[-3:] == (24, 24, 24)
        assert torch.equal(ba["image"], bb["image"]) and torch.equal(ba["label"], bb["label"])
    val = get_dataloader(_phantom_config(PATCH), "val")            # patch mode: full-size volumes one by one
    assert isinstance(val, DeviceLoader) and next(iter(val))["image"].shape == (1, 2, 24, 24, 24)


# ------------------------------------------------------------------------------------------------ end to end
def _phantom_arrays(k, S=40):
    rng = np.random.default_rng(90 + k)
    z, y, x = np.meshgrid(*[np.arange(S)] * 3, indexing="ij")
    lab = np.zeros((S, S, S), dtype=np.uint8)
    lab[(z - 14 - 3 * k) ** 2 + (y - 20) ** 2 + (x - 16) ** 2 <= 64] = 1
    lab[(z - 28) ** 2 / 30 + (y - 12 - 2 * k) ** 2 / 60 + (x - 27) ** 2 / 90 <= 1] = 2
    ct = (-100 + 150 * lab.astype(np.float32) + 20 * rng.standard_normal(lab.shape)).astype(np.int16)
    pet = (1.0 + 3.0 * lab + np.abs(rng.standard_normal(lab.shape))).astype(np.float32)
    return ct, pet, lab


def test_trains_on_patches_and_validates_on_windows(dev, tmp_path):
    from bench import make_config
    from mmseg_amd.models.build import build_model
    from mmseg_amd.trainer.metrics import DiceMetric
    from mmseg_amd.trainer.trainer import Trainer
    root = tmp_path / "data"
    for sub in ("ct", "pet", "label"):
        (root / sub).mkdir(parents=True)
    rows = []
    for k in range(2):
        ct, pet, lab = _phantom_arrays(k)
        NR.write_nifti(root / "ct" / f"p{k}.nii.gz", ct)
        NR.write_nifti(root / "pet" / f"p{k}.nii", pet)
        NR.write_nifti(root / "label" / f"p{k}.nii.gz", lab)
        rows.append(f"p{k},ct/p{k}.nii.gz,pet/p{k}.nii,label/p{k}.nii.gz\n")
    (root / "train.csv").write_text("patient_id,CT,PET,label\n" + "".join(rows))
    (root / "val.csv").write_text("patient_id,CT,PET,label\n" + rows[0])
    cfg = make_config("unet", 2, "fp32", out_channels=3)
    cfg["model"]["backbone"]["features"] = [8, 16, 32, 64, 128]
    cfg["model"]["backbone"]["img_size"] = [32, 32, 32]
    cfg["data"].update({"data_root": str(root), "train_csv": "train.csv", "val_csv": "val.csv",
                        "patch": {"enabled": True, "size": [32, 32, 32], "patches_per_volume": 2,
                                  "rotate_deg": 15, "scale": [0.9, 1.1]},
                        "augmentation": {"enabled": True, "random_flip": True, "random_rotate": 1,
                                         "random_intensity": 0.1}})
    cfg["experiment"].update({"output_dir": str(tmp_path), "log_dir": str(tmp_path / "logs"), "name": "patch",
                              "seed": 5})
    cfg["inference"] = {"sliding_window": {"roi_size": [32, 32, 32], "overlap": 0.5}, "batch_size": 4}
    torch.manual_seed(0)
    train, val = get_dataloader(cfg, "train"), get_dataloader(cfg, "val")
    assert isinstance(train, PatchLoader) and len(train) == 2 and len(val) == 1
    tr = Trainer(copy.deepcopy(cfg), build_model(cfg), train_loader=train, val_loader=val)
    before = [p.detach().clone() for p in tr.model.parameters()]
    hist = tr.train()                                           # two steps, then the windowed validation
    assert len(hist["train_loss"]) == 1 and np.isfinite(hist["train_loss"][0]) and np.isfinite(hist["val_loss"][0])
    assert any(not torch.equal(a, b) for a, b in zip(before, tr.model.parameters()))
    assert all(torch.isfinite(p).all() for p in tr.model.parameters())
    metrics = tr.evaluate()
    vol = next(iter(val))
    assert vol["image"].shape == (1, 2, 40, 40, 40) and vol["patient_id"] == ["p0"]
    tr.model.eval()
    with torch.no_grad():
        logits = tr._sliding_window_inference(vol["image"])
    assert logits.shape == (1, 3, 40, 40, 40)
    dm = DiceMetric(num_classes=3, device=tr.device)
    dm.update_from_logits(logits, vol["label"])
    by_hand = dm.compute()
    assert set(by_hand) <= set(metrics) and all(metrics[k] == by_hand[k] for k in by_hand), (metrics, by_hand)
    assert 0.0 <= metrics["dice"] <= 1.0 and metrics["dice"] == hist["val_dice"][0]
