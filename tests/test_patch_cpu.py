"""Patch sampler, host side (mmseg_amd/data/patch.py) and its numpy restatement (tests/patch_ref.py): no GPU.

The draws are held to the reference's own RandomCrop (tests/golden/patch.npz, made by make_golden_patch.py from
the reference's transforms), the restatement's copy path to the reference's crops bitwise, and its affine path
to scipy.ndimage.affine_transform in fp64.  The tolerance against scipy is 1e-12 x max|v|: both sides sum at
most 8 weighted fp64 terms of magnitude <= max|v| with weights in [0, 1] that carry a few ulps of their own, so
the difference is a few dozen ulps of max|v| (2.2e-16 each) at the very most."""
import os
import random

import numpy as np
import pytest
import scipy.ndimage as ndi

import mmseg_amd  # noqa: F401
from mmseg_amd.data.augment import sample_rng
from mmseg_amd.data.patch import (PATCH_DEFAULTS, affine_matrix, draw_patch_params, patch_config, patch_rng)
from tests import patch_cases as PC
from tests import patch_ref as PR

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "patch.npz"))
SIZES = [tuple(int(v) for v in s) for s in GOLD["sizes"]]
SEEDS = [int(s) for s in GOLD["seeds"]]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("si", range(len(SIZES)))
def test_draws_and_copy_match_reference_random_crop(si):
    size = SIZES[si]
    image, label = GOLD["image_a"], GOLD["label_a"]
    assert [tuple(int(v) for v in s) for s in GOLD["sizes"]] == [(8, 8, 16), (6, 5, 7)]
    assert image.shape == (2, 13, 11, 18)
    starts = set()
    for seed in SEEDS:
        p = draw_patch_params(random.Random(seed), {"size": size, "foreground_prob": 0}, image.shape[1:])
        assert p.mode == 0 and not p.affine
        assert list(p.fallback_start) == GOLD[f"draws_{si}_{seed}"].tolist()
        start = PR.pick_start(label, size, p.mode, p.u, p.fallback_start)
        assert start == list(p.fallback_start)
        img, lab = PR.sample_copy(image, label, start, size, (9.0, 9.0))
        assert np.array_equal(_bits(img), _bits(GOLD[f"crop_image_{si}_{seed}"]))
        assert np.array_equal(lab, GOLD[f"crop_label_{si}_{seed}"])
        starts.add(tuple(start))
    assert len(starts) >= 4          # the seeds do draw different crops
    centre = [max(0, (image.shape[1 + a] - size[a]) // 2) for a in range(3)]
    img, lab = PR.sample_copy(image, label, centre, size, (9.0, 9.0))
    assert np.array_equal(_bits(img), _bits(GOLD[f"center_image_{si}"]))
    assert np.array_equal(lab, GOLD[f"center_label_{si}"])


def test_volume_smaller_than_the_patch_is_centred_and_padded():
    """(5, 9, 20) -> (8, 8, 16): the reference's slice keeps the 5 planes, no draw for that axis; the patch holds
    them at planes 1..5 (start -((8 - 5) // 2) = -1) between padding."""
    image, label = GOLD["image_b"], GOLD["label_b"]
    size, pad = SIZES[0], (2.5, -3.0)
    for seed in SEEDS[:2]:
        p = draw_patch_params(random.Random(seed), {"size": size, "foreground_prob": 0}, image.shape[1:])
        assert list(p.fallback_start) == [0] + GOLD[f"small_draws_{seed}"].tolist()
        start = PR.pick_start(label, size, 0, p.u, p.fallback_start)
        assert start[0] == -1 and start[1:] == list(p.fallback_start[1:])
        img, lab = PR.sample_copy(image, label, start, size, pad)
        assert np.array_equal(_bits(img[:, 1:6]), _bits(GOLD[f"small_image_{seed}"]))
        assert np.array_equal(lab[1:6], GOLD[f"small_label_{seed}"])
        for c in range(2):
            assert (img[c, 0] == np.float32(pad[c])).all() and (img[c, 6:] == np.float32(pad[c])).all()
        assert (lab[0] == 0).all() and (lab[6:] == 0).all()


@pytest.mark.parametrize("fg", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("affine_prob", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("affine", ["none", "rotate", "scale", "both"])
def test_draw_count_is_fixed(fg, affine_prob, affine):
    cfg = {"size": [8, 6, 10], "foreground_prob": fg, "affine_prob": affine_prob,
           "rotate_deg": 15 if affine in ("rotate", "both") else 0,
           "scale": [0.9, 1.1] if affine in ("scale", "both") else None}
    shape = (13, 6, 18)              # no draw for axis 1: max_a == 0
    modes, fired = set(), set()
    for seed in range(24):
        rng, twin = random.Random(seed), random.Random(seed)
        p = draw_patch_params(rng, cfg, shape)
        twin.random()
        twin.randint(0, 5)
        twin.randint(0, 8)
        twin.random()
        if affine != "none":
            twin.random()
            for _ in range(3 if cfg["rotate_deg"] else 0):
                twin.uniform(-15, 15)
            if cfg["scale"]:
                twin.uniform(0.9, 1.1)
        assert rng.getstate() == twin.getstate(), (seed, p)
        assert p.fallback_start[1] == 0
        modes.add(p.mode)
        fired.add(p.affine)
        if p.affine:
            assert np.array_equal(p.M, affine_matrix(p.angles, p.scale))
            assert all(abs(a) <= cfg["rotate_deg"] for a in p.angles) and (p.scale == 1.0 or 0.9 <= p.scale <= 1.1)
        else:
            assert np.array_equal(p.M, np.eye(3))
    assert modes == ({0} if fg == 0 else {1} if fg == 1 else {0, 1})
    want = {False} if affine == "none" or affine_prob == 0 else {True} if affine_prob == 1 else {False, True}
    assert fired == want


def test_patch_streams_are_their_own():
    a = [patch_rng(3, 1, 5, j).random() for j in range(3)]
    assert len(set(a)) == 3
    assert patch_rng(3, 1, 5, 0).random() == a[0]
    others = {patch_rng(4, 1, 5, 0).random(), patch_rng(3, 2, 5, 0).random(), patch_rng(3, 1, 6, 0).random(),
              sample_rng(3, 1, 5).random(), sample_rng(3, 1, 5 * 4).random()}
    assert a[0] not in others and len(others) == 5


def test_affine_matrix_convention():
    """M = Rz Ry Rx / s; a turn about axis 0 alone leaves axis 0 alone and turns (1, 2)."""
    M = affine_matrix((30.0, 0.0, 0.0), 1.0)
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    assert np.allclose(M, [[1, 0, 0], [0, c, -s], [0, s, c]], atol=1e-15)
    assert np.allclose(affine_matrix((0.0, 30.0, 0.0), 1.0), [[c, 0, s], [0, 1, 0], [-s, 0, c]], atol=1e-15)
    assert np.allclose(affine_matrix((0.0, 0.0, 30.0), 1.0), [[c, -s, 0], [s, c, 0], [0, 0, 1]], atol=1e-15)
    for scale in PC.SCALES:
        M = affine_matrix(PC.ANGLES, scale)
        assert np.allclose(M, PR.rotation_scale_matrix(PC.ANGLES, scale), atol=1e-15)
        assert np.allclose(M @ M.T, np.eye(3) / scale ** 2, atol=1e-14)
        assert np.isclose(np.linalg.det(M), scale ** -3)


def _scipy_offset(start, M):
    half = (np.array(PC.PATCH, dtype=np.float64) - 1) * 0.5
    return np.array(start, dtype=np.float64) + half - M @ half


def test_restatement_image_is_scipy_grid_constant():
    image, _ = PC.volume()
    worst = 0.0
    for start, M in PC.affine_cases():
        got = PR.sample_affine_image(image, start, PC.PATCH, M, PC.PAD, dtype=np.float64)
        outside = 0
        for c in range(2):
            vol = image[c].astype(np.float64)
            ref = ndi.affine_transform(vol, M, offset=_scipy_offset(start, M), output_shape=PC.PATCH, order=1,
                                       mode="grid-constant", cval=PC.PAD[c])
            scale = max(np.abs(vol).max(), abs(PC.PAD[c]))
            err = np.abs(got[c] - ref).max() / scale
            worst = max(worst, err)
            assert err <= 1e-12, (start, c, err)
            other = ndi.affine_transform(vol, M, offset=_scipy_offset(start, M), output_shape=PC.PATCH, order=1,
                                         mode="constant", cval=PC.PAD[c])
            outside += int((np.abs(ref - other) > 1e-6).sum())
        assert outside > 0, start            # part of the patch does fall outside: the two modes differ there
    print("restatement vs scipy grid-constant: worst relative error", worst)


def test_restatement_label_is_scipy_order_0():
    _, label = PC.volume()
    for start, M in PC.affine_cases():
        ties = PR.label_ties(start, PC.PATCH, M, tol=1e-9)
        assert ties.mean() <= 0.01
        assert not ties.any()                # these angles put no voxel on a rounding boundary
        got = PR.sample_affine_label(label, start, PC.PATCH, M)
        ref = ndi.affine_transform(label.astype(np.float64), M, offset=_scipy_offset(start, M),
                                   output_shape=PC.PATCH, order=0, mode="grid-constant", cval=0.0)
        assert np.array_equal(got[~ties], ref[~ties].astype(np.int64)), start
        assert (got == 0).any() and (got > 0).any()


def test_pick_rule_restatement():
    label = np.zeros((7, 9, 11), dtype=np.int64)
    size = (4, 4, 6)
    assert PR.pick_start(label, size, 1, 0.3, (1, 2, 3)) == [1, 2, 3]           # no foreground: the fallback
    label[6, 8, 10] = 2
    assert PR.pick_start(label, size, 1, 0.99, (1, 2, 3)) == [3, 5, 5]          # clamped at the far end
    label[0, 0, 0] = 1
    assert PR.pick_start(label, size, 1, 0.0, (1, 2, 3)) == [0, 0, 0]           # clamped at the near end
    assert PR.pick_start(label, size, 1, 0.5, (1, 2, 3)) == [3, 5, 5]           # k = floor(0.5 * 2) = 1
    assert PR.pick_start(label, size, 1, 1 - 2.0 ** -53, (1, 2, 3)) == [3, 5, 5]
    assert PR.pick_start(label, (4, 12, 6), 0, 0.0, (1, 0, 3)) == [1, -1, 3]    # an axis smaller than the patch


def test_config_validation():
    assert patch_config(None) == PATCH_DEFAULTS and patch_config({})["enabled"] is False
    full = patch_config({"enabled": True, "size": (32, 32, 16), "patches_per_volume": 2, "scale": (0.9, 1.1),
                         "pad_value": [0, 1]})
    assert full["size"] == [32, 32, 16] and full["scale"] == [0.9, 1.1] and full["pad_value"] == [0.0, 1.0]
    with pytest.raises(ValueError, match="rotate_degrees"):
        patch_config({"rotate_degrees": 15})
    for bad in ({"size": [96, 96]}, {"size": [96, 0, 96]}, {"size": 96}, {"patches_per_volume": 0},
                {"patches_per_volume": 17}, {"foreground_prob": 1.5}, {"affine_prob": -0.1}, {"rotate_deg": -1},
                {"scale": [1.1, 0.9]}, {"scale": [0, 1]}, {"scale": 1.0}, {"cache_gb": -1}):
        with pytest.raises(ValueError, match="data.patch"):
            patch_config(bad)


def test_get_dataloader_rejects_a_bad_patch_block_and_the_host_path():
    from mmseg_amd.data.dataloader import get_dataloader
    cfg = {"data": {"modalities": ["CT"], "synthetic": {"n_train": 2, "size": 16}, "patch": {"enable": True}},
           "model": {"out_channels": 3}, "training": {"batch_size": 1}}
    with pytest.raises(ValueError, match="unknown key"):
        get_dataloader(cfg, "train")
    cfg["data"]["patch"] = {"enabled": True, "size": [8, 8, 8]}
    with pytest.raises(NotImplementedError, match="device data path"):
        get_dataloader(cfg, "train")
