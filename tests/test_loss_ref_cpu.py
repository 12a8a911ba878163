"""tests/loss_ref.py (the fp64 checker of the loss and fused head + loss kernel tests) against the reference-produced
golden losses and against torch's own cross_entropy.  CPU only."""
import math

import pytest
import torch
import torch.nn.functional as F

import mmseg_amd  # noqa: F401
from mmseg_amd.trainer.losses import CrossEntropyLoss, DiceCELoss, DiceLoss, FocalLoss, TverskyLoss
from tests.helpers import golden, rel
from tests.loss_ref import head_input, head_loss_ref, label_masks, loss_ref


def _golden_mods(cw):
    return {"dicece": DiceCELoss(), "dicece_w": DiceCELoss(0.3, 0.7, class_weights=cw), "dice": DiceLoss(),
            "dice_nobg": DiceLoss(include_background=False), "ce": CrossEntropyLoss(),
            "tversky": TverskyLoss(), "tversky_37": TverskyLoss(alpha=0.3, beta=0.7), "focal": FocalLoss(),
            "focal_w": FocalLoss(alpha=cw)}


@pytest.mark.parametrize("C", [3, 6, 7])
def test_loss_ref_matches_reference_golden(C):
    """All nine golden losses, value and gradient, to the bounds test_losses_vs_reference_golden holds the kernels
    to."""
    g = golden("losses")
    logits = torch.from_numpy(g[f"logits_C{C}"])
    labels = torch.from_numpy(g[f"labels_C{C}"])
    cw = torch.from_numpy(g[f"cw_C{C}"])
    for name, mod in _golden_mods(cw).items():
        z = logits.double().requires_grad_(True)
        loss = loss_ref(z, labels, mod._spec(), getattr(mod, "class_weights", None))
        loss.backward()
        want = float(g[f"{name}_C{C}"])
        assert abs(loss.item() - want) < 2e-6 * max(1.0, abs(want)), name
        assert rel(z.grad, torch.from_numpy(g[f"{name}_C{C}_grad"])) < 1e-5, name


def _edge_inputs(C):
    g = torch.Generator().manual_seed(21)
    logits = torch.randn(2, C, 6, 7, 8, generator=g) * 3
    y = torch.randint(0, C, (2, 6, 7, 8), generator=g)
    y[torch.rand(y.shape, generator=g) < 0.2] = -100
    return logits, y, torch.rand(C, generator=g) + 0.5


@pytest.mark.parametrize("C", [3, 5])
def test_ce_skips_minus_100_like_torch(C):
    logits, y, cw = _edge_inputs(C)
    for w in (None, cw):
        a = logits.double().requires_grad_(True)
        b = logits.double().requires_grad_(True)
        la = loss_ref(a, y, CrossEntropyLoss(weight=w)._spec(), w)
        lb = F.cross_entropy(b, y, weight=None if w is None else w.double())
        la.backward()
        lb.backward()
        assert abs(la.item() - lb.item()) < 1e-12
        assert rel(a.grad, b.grad) < 1e-12
        assert (a.grad.permute(0, 2, 3, 4, 1)[y == -100] == 0).all()


@pytest.mark.parametrize("C", [3, 6])
def test_focal_skips_minus_100_but_counts_it(C):
    """The formula test_focal_ignores_minus_100 holds the kernels to: cross_entropy(reduction='none') is 0 at -100
    and the plain mean still divides by every voxel."""
    logits, y, cw = _edge_inputs(C)
    for w in (None, cw):
        a = logits.double().requires_grad_(True)
        b = logits.double().requires_grad_(True)
        mod = FocalLoss(alpha=w)
        la = loss_ref(a, y, mod._spec(), mod.class_weights)
        ce = F.cross_entropy(b, y, weight=None if w is None else w.double(), reduction="none")
        lb = ((1 - torch.exp(-ce)) ** 2.0 * ce).mean()
        la.backward()
        lb.backward()
        assert abs(la.item() - lb.item()) < 1e-12
        assert rel(a.grad, b.grad) < 1e-10


def test_invalid_labels_give_nan_and_are_counted():
    C = 5
    logits, y, cw = _edge_inputs(C)
    n100 = int((y == -100).sum())
    assert n100 > 0
    bad = y.clone()
    bad[0, 1, 2, 3], bad[1, 0, 0, 0], bad[1, 5, 6, 4] = 255, C, -3
    extra = int((y[0, 1, 2, 3] == -100)) + int((y[1, 0, 0, 0] == -100)) + int((y[1, 5, 6, 4] == -100))
    for mod, count in ((CrossEntropyLoss(weight=cw), 3), (FocalLoss(), 3), (DiceCELoss(), 3 + n100 - extra),
                       (DiceLoss(), 3 + n100 - extra), (TverskyLoss(), 3 + n100 - extra)):
        spec = mod._spec()
        assert math.isnan(loss_ref(logits.double(), bad, spec, getattr(mod, "class_weights", None)).item())
        valid, ignored, invalid = label_masks(bad, C, spec)
        assert int(invalid.sum()) == count and int((valid | ignored | invalid).sum()) == bad.numel()
        assert not (valid & ignored).any() and not (valid & invalid).any() and not (ignored & invalid).any()
    # -100 under a region loss is invalid, not ignored
    assert math.isnan(loss_ref(logits.double(), y, DiceCELoss()._spec(), None).item())
    assert math.isfinite(loss_ref(logits.double(), y, CrossEntropyLoss()._spec(), None).item())


def test_absent_class_is_carried_by_smooth():
    """T_c = 0 and p_c -> 0: the (n, c) Dice / Tversky entry is 1 - s / s = 0, so a perfect prediction of the
    present classes has zero region loss."""
    y = torch.zeros(1, 2, 2, 2, dtype=torch.long)
    y[0, 0] = 1
    z = F.one_hot(y, 3).permute(0, 4, 1, 2, 3).double() * 200.0
    for mod in (DiceLoss(), TverskyLoss(0.3, 0.7)):
        assert abs(loss_ref(z, y, mod._spec()).item()) < 1e-12


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_head_loss_ref_is_conv3d_plus_loss(dtype):
    """head_loss_ref against F.conv3d + loss_ref on the same rounded input,
    with a Dropout3d scale, a deferred norm and an output-gradient scale."""
    g = torch.Generator().manual_seed(4)
    N, Cin, C = 2, 16, 5
    x = torch.randn(N, Cin, 3, 4, 5, generator=g) * 3
    W = torch.randn(C, Cin, generator=g) / 4
    b = torch.randn(C, generator=g)
    y = torch.randint(0, C, (N, 3, 4, 5), generator=g)
    cw = torch.rand(C, generator=g) + 0.5
    ds = (torch.rand(N, Cin, generator=g) > 0.3).float() / 0.7
    norm = (torch.randn(N, Cin, generator=g), torch.rand(N, Cin, generator=g) + 0.5)
    mod = DiceCELoss(0.3, 0.7, class_weights=cw)
    loss, dh, dW, db = head_loss_ref(x, W, b, ds, norm, y, mod._spec(), cw, dtype, gout=0.25)
    h = head_input(x, norm, dtype)
    want_h = torch.relu((x.to(dtype).float() - norm[0][:, :, None, None, None]) * norm[1][:, :, None, None, None])
    assert torch.equal(h, want_h.to(dtype).double())
    hh = h.clone().requires_grad_(True)
    Wd = W.double().requires_grad_(True)
    bd = b.double().requires_grad_(True)
    z = F.conv3d(hh * ds.double()[:, :, None, None, None], Wd[:, :, None, None, None], bd)
    ref = loss_ref(z, y, mod._spec(), cw)
    (ref * 0.25).backward()
    assert abs(loss.item() - ref.item()) < 1e-12
    assert rel(dh, hh.grad) < 1e-12 and rel(dW, Wd.grad) < 1e-12 and rel(db, bd.grad) < 1e-12
    assert (dh[0][ds[0] == 0] == 0).all()     # a dropped channel has no gradient
