"""Kernel-level parity: every HIP kernel family against a torch CPU fp64
restatement of the same op (the floating-point oracle for a single kernel),
on small odd shapes.  fp32 storage must agree to ~1e-5 normwise; bf16 storage
is compared against the op evaluated on the same bf16-rounded inputs."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mmseg_amd  # noqa: F401
from mmseg_amd.engine.layers import Conv3, ConvT2, DySpec, Head, Point, Block
from mmseg_amd.engine.runtime import Act, FlatParams, Runtime
from mmseg_amd._lib import lib, ptr, stream_handle
from tests.conv_fused_cases import VARIANTS, variant_names
from tests.helpers import from_ndhwc, golden, rel, to_ndhwc

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
@pytest.fixture(autouse=True)
def _brick2_small_volumes(monkeypatch):
    """These tests pin brick2-family kernels on small volumes; by default the engine sends conv launches of fewer
    than MMSEG_BRICK2_MINUNITS (4x8x8 brick, 64-column) units to the runtime-brick kernel instead
    (test_conv3_few_brick_units_take_runtime_brick covers that routing)."""
    monkeypatch.setenv("MMSEG_BRICK2_MINUNITS", "0")


TOL = {torch.float32: 2e-5, torch.bfloat16: 1.2e-2}
GTOL = {torch.float32: 2e-5, torch.bfloat16: 2e-3}   # fp32-accumulated gradient outputs


def _q(t, dtype):
    """round through the storage dtype, return fp64 CPU"""
    return t.detach().to(dtype).double().cpu()


def _act(x, dtype):
    N, C, D, H, W = x.shape
    return Act(to_ndhwc(x, dtype), 0, C, C, N, D, H, W)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout,shape", [
    (8, 32, (2, 5, 6, 7)), (32, 32, (1, 8, 8, 8)), (64, 32, (2, 6, 6, 6)), (32, 64, (1, 6, 7, 5)),
    (128, 64, (2, 4, 4, 4)), (256, 128, (1, 3, 2, 2)), (16, 8, (2, 4, 5, 6)),
    # shapes taken by the LDS-halo brick kernel (D%4, H%4, W%8, Cin%32): BN=32 / BN=64 / ragged Ncols
    (32, 32, (2, 4, 4, 8)), (64, 32, (1, 8, 4, 16)), (32, 64, (1, 4, 8, 8)), (256, 64, (2, 4, 4, 8)),
    (128, 128, (1, 8, 8, 8))])
def test_conv3_fwd_dgrad_wgrad(dev, dtype, cin, cout, shape):
    _check_conv3(dev, dtype, cin, cout, shape)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("knobs,cin,cout,shape", [row[:4] for row in VARIANTS])
def test_conv3_kernel_variants(dev, dtype, knobs, cin, cout, shape, monkeypatch):
    """Every kernel variant of the 3^3 conv against fp64, on the rows of tests/conv_fused_cases.py VARIANTS (each
    names the kernel it is for); the forward, data-gradient and weight-gradient kernels that ran are the row's
    (tests/test_conv_fused_plan_cpu.py holds the same names against the planning queries without a GPU)."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    ran = _check_conv3(dev, dtype, cin, cout, shape)
    assert ran == variant_names(knobs, cin, cout, shape)[0 if dtype == torch.float32 else 1]


def _planned_fwd(layer, x, y):
    """The kernel the library's planning query (mmseg_conv3_kernel) names for layer.fwd(x, y)."""
    L, M = lib(), x.N * x.V
    shape = (M, layer.ncols_f, layer.Cpad, layer.KG, layer.cpg_shift, x.D, x.H, x.W, x.ld, y.ld)
    ks = L.mmseg_conv3_splits(*shape, layer.rt.code)
    return L.mmseg_conv3_kernel(*shape, layer.kreal_f, ks, 0, layer.rt.code).decode()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout,shape,extra,kernel", [
    (64, 64, (2, 8, 16, 8), {"MMSEG_BRICK2_MINBLK": "0"}, "conv3_brick2_kernel<BN64,ZW1>"),
    (64, 64, (1, 12, 8, 24), {"MMSEG_BRICK2_MINBLK": "0"}, "conv3_brick2_kernel<BN64,ZW1>"),  # border bricks
    (256, 128, (2, 12, 12, 12), {}, "conv3_brickr_kernel"),        # runtime brick (3,6,12), split-K
    (512, 256, (1, 6, 6, 6), {}, "conv3_brickr_kernel"),           # compile-time 6x6x6 brick, 16 chunks
    # compile-time 4x8x8 brick (the grouped 48^3 / 24^3 levels); MMSEG_BRICK=3 skips the brick2 family
    (128, 64, (2, 8, 16, 16), {"MMSEG_BRICK": "3"}, "conv3_brickr_kernel"),   # BN64 in bf16
    (64, 32, (1, 8, 16, 24), {"MMSEG_BRICK": "3"}, "conv3_brickr_kernel<BN32>"),
])
def test_b32_halo_staging(dev, dtype, cin, cout, shape, extra, kernel, monkeypatch):
    """The 32-bit-offset halo staging of the bf16 brick2 / runtime-brick kernels (MMSEG_B32: buffer loads whose
    out-of-volume lanes read zeros) against the 64-bit staging (=0; the fp32 path's), on shapes with border bricks
    on every side: forward and data gradient bitwise equal (only the loads differ), and both against the fp64
    evaluation (_check_conv3).  (The 48-column brick2 variant is covered by the SwinUNETR tests, whose 48-channel
    layers are its only users.)"""
    for k, v in extra.items():
        monkeypatch.setenv(k, v)
    torch.manual_seed(cin + cout)
    conv = nn.Conv3d(cin, cout, 3, padding=1).to(dev)
    N, D, H, W = shape
    x = torch.randn(N, cin, D, H, W, device=dev)
    dy = torch.randn(N, cout, D, H, W, device=dev)
    res = []
    for b32 in ("1", "0"):
        monkeypatch.setenv("MMSEG_B32", b32)
        rt = Runtime(dev, dtype)
        flat = FlatParams(list(conv.parameters()))
        layer = Conv3(rt, conv, flat)
        layer.pack()
        xa = _act(x, dtype)
        ya = rt.act(N, D, H, W, cout)
        layer.fwd(xa, ya)
        torch.cuda.synchronize()
        assert lib().mmseg_last_kernel().decode().startswith(kernel)
        assert _planned_fwd(layer, xa, ya) == lib().mmseg_last_kernel().decode()
        dxa = rt.act(N, D, H, W, cin)
        layer.bwd(xa, _act(dy, dtype), dxa, accumulate=False)
        torch.cuda.synchronize()
        res.append((ya.buf.clone(), dxa.buf.clone()))
        if b32 == "1":
            _check_conv3(dev, dtype, cin, cout, shape)
    assert torch.equal(res[0][0], res[1][0]), "forward differs between 32-bit and 64-bit staging"
    assert torch.equal(res[0][1], res[1][1]), "data gradient differs between 32-bit and 64-bit staging"


def _check_conv3(dev, dtype, cin, cout, shape):
    """Forward, data gradient, weight and bias gradient of one Conv3 against fp64; returns the kernels that ran
    (forward, data gradient) and the weight-gradient kernel the library names for Conv3._bwd's arguments."""
    torch.manual_seed(cin + cout)
    conv = nn.Conv3d(cin, cout, 3, padding=1).to(dev)
    rt = Runtime(dev, dtype)
    flat = FlatParams(list(conv.parameters()))
    layer = Conv3(rt, conv, flat)
    N, D, H, W = shape
    x = torch.randn(N, cin, D, H, W, device=dev)
    xa = _act(x, dtype)
    ya = rt.act(N, D, H, W, cout)
    layer.pack()
    layer.fwd(xa, ya)
    ran_fwd = lib().mmseg_last_kernel().decode()
    xd = _q(x, dtype).requires_grad_(True)
    wd = _q(conv.weight, dtype).requires_grad_(True)
    bd = conv.bias.detach().double().cpu().requires_grad_(True)
    ref = F.conv3d(xd, wd, bd, padding=1)
    out = from_ndhwc(ya.buf, N, cout, D, H, W)
    assert rel(out, ref) < TOL[dtype]
    dy = torch.randn(ref.shape, device=dev)
    dya = _act(dy, dtype)
    dxa = rt.act(N, D, H, W, cin)
    layer.bwd(xa, dya, dxa, accumulate=False)
    ran_dgrad = lib().mmseg_last_kernel().decode()     # the data gradient is the backward's last launch
    (ref * _q(dy, dtype)).sum().backward()
    assert rel(from_ndhwc(dxa.buf, N, cin, D, H, W), xd.grad) < TOL[dtype]
    assert rel(flat.grad(conv.weight), wd.grad) < GTOL[dtype]
    assert rel(flat.grad(conv.bias), bd.grad) < GTOL[dtype]
    # the weight-gradient kernel: the name query with the arguments Conv3._bwd passes
    L, V = lib(), N * D * H * W
    wshape = (V, layer.Co, layer.Cip, layer.Ci, layer.cpg_shift, D, H, W, dya.ld, xa.ld)
    wsf = L.mmseg_conv3_wgrad_ws_floats(*wshape, rt.code)
    return ran_fwd, ran_dgrad, L.mmseg_conv3_wgrad_kernel(*wshape, wsf, 0, rt.code).decode()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cr,co,shape", [
    (2, 32, (2, 6, 8, 4)),                      # generic path (shape not brick-aligned)
    (1, 32, (2, 4, 8, 16)), (2, 32, (1, 8, 8, 8)), (3, 16, (1, 4, 16, 8)), (4, 32, (1, 4, 8, 8)),  # stem.hip
])
def test_conv3_stem_padded_input(dev, dtype, cr, co, shape):
    """first conv: 1-4 real input channels packed into an 8-channel NDHWC tile"""
    torch.manual_seed(5)
    conv = nn.Conv3d(cr, co, 3, padding=1).to(dev)
    rt = Runtime(dev, dtype)
    flat = FlatParams(list(conv.parameters()))
    layer = Conv3(rt, conv, flat, cin_pad=8, need_dgrad=False)
    N, D, H, W = shape
    x = torch.randn(N, cr, D, H, W, device=dev)
    xa = rt.act(N, D, H, W, 8)
    lib().mmseg_pack_input(ptr(x), cr, 0, cr, N, D * H * W, xa.ptr, rt.code, stream_handle())
    ya = rt.act(N, D, H, W, co)
    layer.pack()
    layer.fwd(xa, ya)
    xd = _q(x, dtype)
    wd = _q(conv.weight, dtype).requires_grad_(True)
    bd = conv.bias.detach().double().cpu().requires_grad_(True)
    ref = F.conv3d(xd, wd, bd, padding=1)
    assert rel(from_ndhwc(ya.buf, N, co, D, H, W), ref) < TOL[dtype]
    dy = torch.randn(ref.shape, device=dev)
    layer.bwd(xa, _act(dy, dtype), None, accumulate=False)
    (ref * _q(dy, dtype)).sum().backward()
    assert rel(flat.grad(conv.weight), wd.grad) < GTOL[dtype]
    assert rel(flat.grad(conv.bias), bd.grad) < GTOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout,shape", [(64, 32, (2, 3, 4, 5)), (128, 64, (1, 4, 4, 4)), (16, 8, (2, 2, 3, 2)),
                                            (512, 256, (2, 3, 3, 3)), (64, 32, (2, 16, 12, 12))])
def test_convT_fwd_dgrad_wgrad(dev, dtype, cin, cout, shape):
    """(the last shape runs the weight gradient over many voxel splits: the bias gradient then comes from the
    per-split, per-tap column sums folded by mmseg_colsum_reduce)"""
    torch.manual_seed(cin)
    up = nn.ConvTranspose3d(cin, cout, 2, stride=2).to(dev)
    rt = Runtime(dev, dtype)
    flat = FlatParams(list(up.parameters()))
    layer = ConvT2(rt, up, flat)
    N, D, H, W = shape
    x = torch.randn(N, cin, D, H, W, device=dev)
    xa = _act(x, dtype)
    # write into the first half of a 2*cout concat buffer, like the decoder does
    cat = rt.act(N, 2 * D, 2 * H, 2 * W, 2 * cout)
    layer.pack()
    layer.fwd(xa, cat.slot(0, cout))
    xd = _q(x, dtype).requires_grad_(True)
    wd = _q(up.weight, dtype).requires_grad_(True)
    bd = up.bias.detach().double().cpu().requires_grad_(True)
    ref = F.conv_transpose3d(xd, wd, bd, stride=2)
    out = from_ndhwc(cat.buf, N, cout, 2 * D, 2 * H, 2 * W, ld=2 * cout)
    assert rel(out, ref) < TOL[dtype]
    dy = torch.randn(ref.shape, device=dev)
    dyc = Act(to_ndhwc(dy, dtype, ld=2 * cout), 0, cout, 2 * cout, N, 2 * D, 2 * H, 2 * W)
    dxa = rt.act(N, D, H, W, cin)
    layer.bwd(xa, dyc, dxa, accumulate=False)
    (ref * _q(dy, dtype)).sum().backward()
    assert rel(from_ndhwc(dxa.buf, N, cin, D, H, W), xd.grad) < TOL[dtype]
    assert rel(flat.grad(up.weight), wd.grad) < GTOL[dtype]
    assert rel(flat.grad(up.bias), bd.grad) < GTOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_point_conv(dev, dtype):
    torch.manual_seed(3)
    conv = nn.Conv3d(96, 32, 1).to(dev)
    rt = Runtime(dev, dtype)
    flat = FlatParams(list(conv.parameters()))
    layer = Point(rt, conv, flat)
    N, D, H, W = 2, 3, 4, 5
    x = torch.randn(N, 96, D, H, W, device=dev)
    xa = _act(x, dtype)
    ya = rt.act(N, D, H, W, 32)
    layer.pack()
    layer.fwd(xa, ya)
    xd = _q(x, dtype).requires_grad_(True)
    wd = _q(conv.weight, dtype).requires_grad_(True)
    bd = conv.bias.detach().double().cpu().requires_grad_(True)
    ref = F.conv3d(xd, wd, bd)
    assert rel(from_ndhwc(ya.buf, N, 32, D, H, W), ref) < TOL[dtype]
    dy = torch.randn(ref.shape, device=dev)
    dxa = rt.act(N, D, H, W, 96)
    layer.bwd(xa, _act(dy, dtype), dxa, accumulate=False)
    (ref * _q(dy, dtype)).sum().backward()
    assert rel(from_ndhwc(dxa.buf, N, 96, D, H, W), xd.grad) < TOL[dtype]
    assert rel(flat.grad(conv.weight), wd.grad) < GTOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,shape", [(32, (2, 6, 8, 4)), (8, (1, 4, 4, 4)), (256, (2, 2, 4, 2)), (64, (2, 24, 24, 24))])
@pytest.mark.parametrize("small_v", ["16384", "0"])     # fused one-block-per-channel-group path / multi-pass path
def test_instnorm_relu_maxpool(dev, dtype, C, shape, small_v, monkeypatch):
    """IN+ReLU fwd, MaxPool3d fwd (argmax), IN+ReLU bwd with dy = skip + maxpool_bwd."""
    monkeypatch.setenv("MMSEG_IN_SMALL_V", small_v)
    torch.manual_seed(C)
    N, D, H, W = shape
    x = (torch.randn(N, C, D, H, W, device=dev) * 2 + 0.7)
    L, s, code = lib(), stream_handle(), (0 if dtype == torch.float32 else 1)
    xa = _act(x, dtype)
    ya = Act(torch.empty_like(xa.buf), 0, C, C, N, D, H, W)
    stats = torch.empty(2, N * C, device=dev)
    ws = torch.empty(L.mmseg_instnorm_ws_floats(N, D * H * W, C), device=dev)
    L.mmseg_instnorm_fwd(xa.ptr, C, ya.ptr, C, N, D * H * W, C, 1e-5, ptr(stats[0]), C, ptr(stats[1]), 1, ptr(ws),
                         code, s)
    xd = _q(x, dtype).requires_grad_(True)
    yref = torch.relu(F.instance_norm(xd, eps=1e-5))
    y = from_ndhwc(ya.buf, N, C, D, H, W)
    assert rel(y, yref) < TOL[dtype]
    # maxpool on the engine's own y (ties among ReLU zeros -> first index, like torch)
    pa = Act(torch.empty(N * D * H * W * C // 8, dtype=dtype, device=dev), 0, C, C, N, D // 2, H // 2, W // 2)
    idx = torch.empty(N * D * H * W * C // 8, dtype=torch.uint8, device=dev)
    L.mmseg_maxpool2_fwd(ya.ptr, C, pa.ptr, C, ptr(idx), N, D, H, W, C, code, s)
    yq = y.double().cpu().requires_grad_(True)
    pref, iref = F.max_pool3d(yq, 2, return_indices=True)
    assert rel(from_ndhwc(pa.buf, N, C, D // 2, H // 2, W // 2), pref) == 0.0
    # backward: dy = dskip + maxpool_bwd(dp)
    dskip = torch.randn(N, C, D, H, W, device=dev)
    dp = torch.randn(N, C, D // 2, H // 2, W // 2, device=dev)
    dpa = _act(dp, dtype)
    dxa = Act(torch.empty_like(xa.buf), 0, C, C, N, D, H, W)
    ws2 = torch.empty(L.mmseg_instnorm_ws_floats(N, D * H * W, C), device=dev)
    dska = _act(dskip, dtype)
    L.mmseg_instnorm_relu_bwd(xa.ptr, C, ptr(stats[0]), ptr(stats[1]), dska.ptr, C, 1.0, None, 0, None, 0,
                              dpa.ptr, C, ptr(idx), dxa.ptr, C, N, D, H, W, C, ptr(ws2), code, s)
    # reference: grads through relu(IN(x)), the pooled gradient routed by the engine's own argmax
    Do, Ho, Wo = D // 2, H // 2, W // 2
    it = idx.view(N, Do, Ho, Wo, C).permute(0, 4, 1, 2, 3).long().cpu()
    dpq = _q(dp, dtype)
    routed = torch.zeros(N, C, D, H, W, dtype=torch.float64)
    for t in range(8):
        a, b, c = t >> 2, (t >> 1) & 1, t & 1
        routed[:, :, a::2, b::2, c::2] += (it == t).double() * dpq
    yr = torch.relu(F.instance_norm(xd, eps=1e-5))
    (yr * (_q(dskip, dtype) + routed)).sum().backward()
    tol = 2e-4 if dtype == torch.float32 else 3e-2
    assert rel(from_ndhwc(dxa.buf, N, C, D, H, W), xd.grad) < tol


@pytest.mark.parametrize("shape", [(2, 4, 6, 8), (2, 16, 24, 20), (1, 9, 11, 13)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_head(dev, dtype, shape):
    """Head fwd/bwd vs fp64 conv3d; the larger shapes span several blocks of the 4-voxel-per-thread kernels
    (and a ragged tail: 1287 voxels)."""
    torch.manual_seed(1)
    conv = nn.Conv3d(32, 6, 1).to(dev)
    rt = Runtime(dev, dtype)
    flat = FlatParams(list(conv.parameters()))
    head = Head(rt, conv, flat)
    N, D, H, W = shape
    x = torch.randn(N, 32, D, H, W, device=dev)
    xa = _act(x, dtype)
    logits = torch.empty(N, 6, D, H, W, device=dev)
    head.fwd(xa, logits, None)
    xd = _q(x, dtype).requires_grad_(True)
    w = conv.weight.detach().double().cpu().requires_grad_(True)
    b = conv.bias.detach().double().cpu().requires_grad_(True)
    ref = F.conv3d(xd, w, b)
    assert rel(logits, ref) < 2e-6
    dl = torch.randn_like(logits)
    dxa = rt.act(N, D, H, W, 32)
    head.bwd(xa, dl, dxa, accumulate=False)
    (ref * dl.double().cpu()).sum().backward()
    assert rel(from_ndhwc(dxa.buf, N, 32, D, H, W), xd.grad) < TOL[dtype]
    assert rel(flat.grad(conv.weight), w.grad) < 2e-5
    assert rel(flat.grad(conv.bias), b.grad) < 2e-5


@pytest.mark.parametrize("C", [3, 6, 7])
def test_losses_vs_reference_golden(dev, C):
    from mmseg_amd.trainer.losses import CrossEntropyLoss, DiceCELoss, DiceLoss, FocalLoss, TverskyLoss
    g = golden("losses")
    logits = torch.from_numpy(g[f"logits_C{C}"]).to(dev)
    labels = torch.from_numpy(g[f"labels_C{C}"]).to(dev)
    cw = torch.from_numpy(g[f"cw_C{C}"])
    mods = {"dicece": DiceCELoss(), "dicece_w": DiceCELoss(0.3, 0.7, class_weights=cw), "dice": DiceLoss(),
            "dice_nobg": DiceLoss(include_background=False), "ce": CrossEntropyLoss(),
            "tversky": TverskyLoss(), "tversky_37": TverskyLoss(alpha=0.3, beta=0.7), "focal": FocalLoss(),
            "focal_w": FocalLoss(alpha=cw)}
    for name, mod in mods.items():
        lg = logits.clone().requires_grad_(True)
        loss = mod(lg, labels)
        loss.backward()
        assert abs(loss.item() - float(g[f"{name}_C{C}"])) < 2e-6 * max(1.0, abs(float(g[f"{name}_C{C}"]))), name
        assert rel(lg.grad, torch.from_numpy(g[f"{name}_C{C}_grad"])) < 1e-5, name


def test_loss_uint8_labels_and_scaled_grad(dev):
    from mmseg_amd.trainer.losses import DiceCELoss
    g = golden("losses")
    logits = torch.from_numpy(g["logits_C6"]).to(dev).requires_grad_(True)
    labels = torch.from_numpy(g["labels_C6"]).to(dev)
    (DiceCELoss()(logits, labels.to(torch.uint8)) / 4).backward()
    assert rel(logits.grad * 4, torch.from_numpy(g["dicece_C6_grad"])) < 1e-5


@pytest.mark.parametrize("C", [3, 6, 5])
def test_loss_out_of_range_labels(dev, C):
    """A label outside [0, C) makes the reference raise (F.one_hot / cross_entropy).  The kernels skip the
    voxel (no out-of-bounds class-weight read), count it and return a NaN loss; check_labels() and
    Trainer.train_step raise.  Pure CE ignores -100 like nn.CrossEntropyLoss (ignore_index default)."""
    import torch.nn.functional as F
    from mmseg_amd.trainer.losses import CrossEntropyLoss, DiceCELoss
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(2, C, 6, 7, 5, generator=g)
    labels = torch.randint(0, C, (2, 6, 7, 5), generator=g)
    cw = torch.rand(C, generator=g) + 0.5
    bad = labels.clone()
    bad[0, 1, 2, 3], bad[1, 0, 0, 0], bad[1, 5, 6, 4] = 255, C, -3
    for mod in (DiceCELoss(class_weights=cw), DiceCELoss(), CrossEntropyLoss(weight=cw)):
        lg = logits.to(dev).requires_grad_(True)
        loss = mod(lg, bad.to(dev))
        loss.backward()
        assert torch.isnan(loss).item() and mod.invalid_labels() == 3
        assert torch.isfinite(lg.grad).all()
        with pytest.raises(RuntimeError, match="outside"):
            mod.check_labels()
        assert mod(lg, labels.to(dev)).isfinite().item() and mod.invalid_labels() == 0
        mod.check_labels()
    # ignore_index -100 in pure CE: same value and gradient as torch's cross_entropy
    ign = labels.clone()
    ign[0, :2] = -100
    lg = logits.to(dev).requires_grad_(True)
    mod = CrossEntropyLoss(weight=cw)
    loss = mod(lg, ign.to(dev))
    loss.backward()
    ref_lg = logits.double().requires_grad_(True)
    ref = F.cross_entropy(ref_lg, ign, weight=cw.double())
    ref.backward()
    assert mod.invalid_labels() == 0 and abs(loss.item() - ref.item()) < 1e-5
    assert rel(lg.grad.cpu(), ref_lg.grad.float()) < 1e-5


@pytest.mark.parametrize("C", [3, 6])
def test_dice_metric_bit_identical(dev, C):
    from mmseg_amd.trainer.metrics import DiceMetric
    g = golden("dice_metric")
    dm = DiceMetric(num_classes=C)
    for p, t in zip(g[f"pred_C{C}"], g[f"tgt_C{C}"]):
        dm.update(torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev))
    res = dm.compute()
    assert np.array_equal(dm.intersection.cpu().numpy(), g[f"inter_C{C}"])
    assert np.array_equal(dm.union.cpu().numpy(), g[f"union_C{C}"])
    assert res["dice"] == float(g[f"dice_C{C}"])
    assert res["dice_per_class"] == list(g[f"dpc_C{C}"])


def test_dice_counts_from_logits_matches_argmax(dev):
    from mmseg_amd.trainer.metrics import DiceMetric
    torch.manual_seed(0)
    logits = torch.randn(2, 6, 7, 8, 9, device=dev)
    logits[:, 2, 0, 0, :] = logits[:, 4, 0, 0, :]  # exact ties -> first index
    labels = torch.randint(0, 6, (2, 7, 8, 9), device=dev)
    a, b = DiceMetric(6), DiceMetric(6)
    a.update_from_logits(logits, labels)
    b.update(logits.argmax(1), labels)
    assert torch.equal(a.intersection, b.intersection) and torch.equal(a.union, b.union)


@pytest.mark.parametrize("n0,n1", [(600, 400), (603, 402), (3, 0)])   # float4 body, + scalar tail, tail only
def test_adamw_matches_torch(dev, n0, n1):
    from mmseg_amd.trainer.optim import FlatAdamW
    torch.manual_seed(0)
    flat = torch.randn(n0 + n1, device=dev)
    gflat = torch.randn(n0 + n1, device=dev)
    params = [torch.nn.Parameter(flat[:n0].view(n0))] + ([torch.nn.Parameter(flat[n0:])] if n1 else [])
    params[0].grad = gflat[:n0].view(n0)
    if n1:
        params[1].grad = gflat[n0:]
    ref = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    for r, p in zip(ref, params):
        r.grad = p.grad.detach().cpu().clone()
    opt = FlatAdamW(params, lr=1e-3, weight_decay=1e-5)
    ropt = torch.optim.AdamW(ref, lr=1e-3, weight_decay=1e-5)
    for _ in range(3):
        opt.step()
        ropt.step()
    for r, p in zip(ref, params):
        assert rel(p, r) < 1e-6
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert rel(sd["state"][0]["exp_avg"], ropt.state_dict()["state"][0]["exp_avg"]) < 1e-6


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_conv3_pack_matches_per_layer_pack(dev, dtype):
    """mmseg_pack_conv3_batched (one launch, both operand images) == the per-layer element-wise pack, bitwise,
    for a stem (1 real channel padded to 8, no data-gradient image) and ragged / multi-chunk layers."""
    from mmseg_amd.engine.layers import Packer
    torch.manual_seed(3)
    rt = Runtime(dev, dtype)
    shapes = [(32, 1, 8, False), (64, 32, None, True), (32, 64, None, True), (256, 128, None, True),
              (16, 8, None, True)]
    convs = [nn.Conv3d(ci, co, 3, padding=1).to(dev) for co, ci, _, _ in shapes]
    flat = FlatParams([p for c in convs for p in c.parameters()])
    layers = [Conv3(rt, c, flat, cin_pad=cp, need_dgrad=nd) for c, (_, _, cp, nd) in zip(convs, shapes)]
    descs = [d for l in layers for d in l.descs()]
    Packer(rt, descs).run()
    got = [(l.wf.clone(), l.wd.clone() if l.need_dgrad else None) for l in layers]
    for l in layers:
        l.wf.fill_(7)
        if l.need_dgrad:
            l.wd.fill_(7)
        for d in l.descs():
            lib().mmseg_pack_weight(*d, rt.code, rt.stream)
    torch.cuda.synchronize()
    for l, (wf, wd) in zip(layers, got):
        ref_f = l.wf.clone()
        # the per-layer pack writes every entry (zeros in the padding): compare everything
        assert torch.equal(wf.view(torch.int16) if dtype == torch.bfloat16 else wf, ref_f.view(torch.int16) if dtype == torch.bfloat16 else ref_f)
        if wd is not None:
            assert torch.equal(wd, l.wd)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout,shape", [(48, 48, (1, 8, 8, 16)), (96, 48, (2, 4, 8, 8)), (48, 96, (1, 4, 8, 8)),
                                            (24, 24, (1, 4, 8, 8)), (48, 48, (1, 6, 6, 6)),
                                            # K-side padding skipped chunk-wise (96 of 128, 192 of 256 channels):
                                            # brick / runtime-brick forward, dgrad and weight-gradient kernels
                                            (96, 96, (1, 8, 8, 16)), (192, 96, (1, 4, 4, 4)),
                                            (384, 192, (2, 4, 4, 4))])
def test_conv3_channel_padded(dev, dtype, cin, cout, shape):
    """SwinUNETR's bias-free convs over channel-padded buffers (Conv3 cin_pad / cout_pad / pad_cols): 48-column
    brick tiles, padded K groups with zero weights (pack modes 0 / 6), staged Co-padded weight gradient."""
    from mmseg_amd.engine.swin import cpad
    torch.manual_seed(cin * 3 + cout)
    conv = nn.Conv3d(cin, cout, 3, padding=1, bias=False).to(dev)
    rt = Runtime(dev, dtype)
    flat = FlatParams(list(conv.parameters()))
    cip, cop = cpad(cin), cpad(cout)
    layer = Conv3(rt, conv, flat, cin_pad=cip, cout_pad=cop, pad_cols=True)
    N, D, H, W = shape
    x = torch.randn(N, cin, D, H, W, device=dev)
    xa = Act(to_ndhwc(x, dtype, ld=cip), 0, cin, cip, N, D, H, W)
    ya = Act(torch.zeros(N * D * H * W * cop, dtype=dtype, device=dev), 0, cout, cop, N, D, H, W)
    layer.pack()
    layer.fwd(xa, ya)
    xd = _q(x, dtype).requires_grad_(True)
    wd = _q(conv.weight, dtype).requires_grad_(True)
    ref = F.conv3d(xd, wd, padding=1)
    assert rel(from_ndhwc(ya.buf, N, cout, D, H, W, ld=cop), ref) < TOL[dtype]
    assert from_ndhwc(ya.buf, N, cop, D, H, W, ld=cop)[:, cout:].abs().max().item() == 0.0   # padding stays zero
    dy = torch.randn(ref.shape, device=dev)
    dya = Act(to_ndhwc(dy, dtype, ld=cop), 0, cout, cop, N, D, H, W)
    dxa = Act(torch.zeros(N * D * H * W * cip, dtype=dtype, device=dev), 0, cin, cip, N, D, H, W)
    layer.bwd(xa, dya, dxa, accumulate=False)
    (ref * _q(dy, dtype)).sum().backward()
    assert rel(from_ndhwc(dxa.buf, N, cin, D, H, W, ld=cip), xd.grad) < TOL[dtype]
    assert rel(flat.grad(conv.weight), wd.grad) < GTOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("knobs,cin,cout,shape", [
    ({}, 64, 32, (2, 8, 8, 16)),                                    # dgrad Ncols 64 (brick2 / brick3)
    ({"MMSEG_BRICK2_MINBLK": "0"}, 64, 32, (2, 8, 8, 16)),          # BN64 brick2
    ({}, 128, 64, (2, 4, 8, 8)),                                    # two 64-column tiles
    ({}, 256, 128, (2, 6, 6, 6)),                                   # runtime brick + split-K reduce
    ({}, 64, 32, (1, 3, 5, 7)),                                     # generic GEMM
])
def test_conv3_dgrad_split_output(dev, dtype, knobs, cin, cout, shape, monkeypatch):
    """mmseg_conv_gemm_split (the decoder's first-conv data gradient writing d(upsampled) and d(skip) as two
    dense tensors) gives bitwise the columns of the single [voxel][Cin] output, for every kernel family."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    torch.manual_seed(cin + cout)
    conv = nn.Conv3d(cin, cout, 3, padding=1).to(dev)
    rt = Runtime(dev, dtype)
    flat = FlatParams(list(conv.parameters()))
    layer = Conv3(rt, conv, flat)
    layer.pack()
    N, D, H, W = shape
    xa = _act(torch.randn(N, cin, D, H, W, device=dev), dtype)
    dya = _act(torch.randn(N, cout, D, H, W, device=dev), dtype)
    whole = rt.act(N, D, H, W, cin)
    layer.bwd(xa, dya, whole, accumulate=False)
    h = cin // 2
    buf = torch.zeros(2 * N * D * H * W * h, dtype=rt.dtype, device=dev)
    lo = Act(buf, 0, h, h, N, D, H, W)
    hi = Act(buf, N * D * H * W * h, h, h, N, D, H, W)
    layer.bwd(xa, dya, (lo, hi), accumulate=False)
    torch.cuda.synchronize()
    ref = whole.buf[: N * D * H * W * cin].view(-1, cin)
    assert torch.equal(buf[: N * D * H * W * h].view(-1, h), ref[:, :h])
    assert torch.equal(buf[N * D * H * W * h:].view(-1, h), ref[:, h:])


@pytest.mark.parametrize("cin,cout,shape,accumulate", [
    (64, 64, (2, 8, 12, 16), 0), (32, 128, (2, 8, 8, 16), 1), (64, 32, (2, 8, 4, 16), 0),
    (128, 64, (2, 8, 8, 16), 1), (32, 32, (2, 12, 8, 24), 0), (64, 64, (2, 24, 24, 24), 1)])
def test_wgrad_dma_fragment_partials(dev, cin, cout, shape, accumulate):
    """wgrad_dma's split partials in the accumulators' own layout (direct 16-B stores from registers; the reduce maps
    them to the torch order in a fixed split order): weight and bias gradients against fp64, bitwise repeatable."""
    N, D, H, W = shape
    V = N * D * H * W
    g = torch.Generator().manual_seed(cin + cout + V)
    dy = torch.randn(V, cout, generator=g).to(dev, torch.bfloat16).reshape(-1)
    x = torch.randn(V, cin, generator=g).to(dev, torch.bfloat16).reshape(-1)
    gw0 = torch.randn(cout * cin * 27, generator=g).to(dev) if accumulate else torch.zeros(cout * cin * 27, device=dev)
    gb0 = torch.ones(cout, device=dev) if accumulate else torch.zeros(cout, device=dev)
    L = lib()
    shift = int(np.log2(cin // 8))
    wsf = L.mmseg_conv3_wgrad_ws_floats(V, cout, cin, cin, shift, D, H, W, cout, cin, 1)
    assert wsf > 0, "single split: nothing to reduce"
    out = []
    for _ in range(2):
        ws = torch.full((wsf,), float("nan"), device=dev)
        gw, gb = gw0.clone(), gb0.clone()
        L.mmseg_conv3_wgrad(ptr(dy), cout, ptr(x), cin, ptr(gw), ptr(gb), cout, cin, cin, shift, V, D, H, W,
                            ptr(ws), wsf, accumulate, 1, stream_handle())
        assert L.mmseg_last_kernel().decode().startswith("wgrad_dma_kernel")
        assert L.mmseg_conv3_wgrad_kernel(V, cout, cin, cin, shift, D, H, W, cout, cin, wsf, 0,
                                          1).decode() == L.mmseg_last_kernel().decode()
        torch.cuda.synchronize()
        out.append((gw, gb))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    xr = x.double().cpu().reshape(N, D, H, W, cin).permute(0, 4, 1, 2, 3)
    dyr = dy.double().cpu().reshape(N, D, H, W, cout).permute(0, 4, 1, 2, 3)
    ref = torch.nn.grad.conv3d_weight(xr, (cout, cin, 3, 3, 3), dyr, padding=1).reshape(-1)
    got = out[1][0].double().cpu() - gw0.double().cpu()
    assert rel(got, ref) < GTOL[torch.bfloat16]
    assert rel(out[1][1].double().cpu() - gb0.double().cpu(), dyr.sum(dim=(0, 2, 3, 4))) < GTOL[torch.bfloat16]


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("cin,cout,shape,accumulate", [
    (32, 32, (2, 12, 8, 24), 0), (64, 32, (2, 8, 4, 16), 1), (32, 32, (1, 8, 8, 8), 1), (32, 32, (2, 24, 24, 24), 0)])
def test_wgrad_brick2_pipelined(dev, cin, cout, shape, accumulate, norm, monkeypatch):
    """The 32-co register-staged brick wgrad with its fragment reads software-pipelined (the 32-co layers whose W is
    not a multiple of 32; at 96^3 wgrad_row runs) against fp64 (the deferred norm: relu((x - mean) * rstd) of the bf16
    x, rounded to bf16), bitwise repeatable."""
    monkeypatch.setenv("MMSEG_WGRAD_DMA", "0")
    N, D, H, W = shape
    V = N * D * H * W
    g = torch.Generator().manual_seed(11 * cin + cout + V + norm)
    dy = torch.randn(V, cout, generator=g).to(dev, torch.bfloat16).reshape(-1)
    x = (torch.randn(V, cin, generator=g) * 2 + 0.5).to(dev, torch.bfloat16).reshape(-1)
    mean = (torch.randn(N, cin, generator=g) * 0.3 + 0.5).to(dev)
    rstd = (torch.rand(N, cin, generator=g) + 0.5).to(dev)
    gw0 = torch.randn(cout * cin * 27, generator=g).to(dev) if accumulate else torch.zeros(cout * cin * 27, device=dev)
    gb0 = torch.ones(cout, device=dev) if accumulate else torch.zeros(cout, device=dev)
    L = lib()
    shift = int(np.log2(cin // 8))
    if norm:
        assert L.mmseg_conv3_wgrad_norm_ok(V, cout, cin, cin, shift, D, H, W, cout, cin, 1)
    wsf = L.mmseg_conv3_wgrad_ws_floats(V, cout, cin, cin, shift, D, H, W, cout, cin, 1)
    out = {}
    for pipe in ("0", "1"):
        ws = torch.full((max(wsf, 1),), float("nan"), device=dev)
        gw, gb = gw0.clone(), gb0.clone()
        if norm:
            rc = L.mmseg_conv3_wgrad_norm(ptr(dy), cout, ptr(x), cin, ptr(mean), ptr(rstd), ptr(gw), ptr(gb), cout,
                                          cin, cin, shift, V, D, H, W, ptr(ws), wsf, accumulate, 1, stream_handle())
        else:
            rc = L.mmseg_conv3_wgrad(ptr(dy), cout, ptr(x), cin, ptr(gw), ptr(gb), cout, cin, cin, shift, V, D, H, W,
                                     ptr(ws), wsf, accumulate, 1, stream_handle())
        assert rc == 0
        assert L.mmseg_last_kernel().decode().startswith("wgrad_brick2_kernel<CO32,V3>")
        torch.cuda.synchronize()
        out[pipe] = (gw, gb)
    assert torch.equal(out["0"][0], out["1"][0]) and torch.equal(out["0"][1], out["1"][1])
    xd = x.double().cpu().reshape(N, D * H * W, cin)
    if norm:
        xd = torch.relu((xd - mean.double().cpu()[:, None, :]) * rstd.double().cpu()[:, None, :])
        xd = xd.to(torch.bfloat16).double()
    xr = xd.reshape(N, D, H, W, cin).permute(0, 4, 1, 2, 3)
    dyr = dy.double().cpu().reshape(N, D, H, W, cout).permute(0, 4, 1, 2, 3)
    ref = torch.nn.grad.conv3d_weight(xr, (cout, cin, 3, 3, 3), dyr, padding=1).reshape(-1)
    assert rel(out["1"][0].double().cpu() - gw0.double().cpu(), ref) < GTOL[torch.bfloat16]
    assert rel(out["1"][1].double().cpu() - gb0.double().cpu(), dyr.sum(dim=(0, 2, 3, 4))) < 1e-4


@pytest.mark.parametrize("cip,ci,cout,shape,accumulate", [
    (32, 32, 32, (2, 12, 8, 24), 0), (64, 48, 64, (1, 8, 8, 16), 1), (128, 96, 64, (1, 12, 12, 12), 0),
    (64, 64, 128, (2, 12, 12, 12), 1), (1024, 768, 64, (1, 8, 8, 8), 0)])
def test_wgrad_reduce_vec4(dev, cip, ci, cout, shape, accumulate, monkeypatch):
    """The split reduce of channel-major weight-gradient partials (brick2 / runtime-brick kernels) storing each
    thread's four sums as one 16-B store, padded input channels (ci < cip) dropped: against fp64, bitwise
    repeatable."""
    monkeypatch.setenv("MMSEG_WGRAD_DMA", "0")
    N, D, H, W = shape
    V = N * D * H * W
    g = torch.Generator().manual_seed(cip + ci + cout + V)
    dy = torch.randn(V, cout, generator=g).to(dev, torch.bfloat16).reshape(-1)
    x = torch.randn(V, cip, generator=g)
    x[:, ci:] = 0
    x = x.to(dev, torch.bfloat16).reshape(-1)
    gw0 = torch.randn(cout * ci * 27, generator=g).to(dev) if accumulate else torch.zeros(cout * ci * 27, device=dev)
    gb0 = torch.ones(cout, device=dev) if accumulate else torch.zeros(cout, device=dev)
    L = lib()
    shift = int(np.log2(cip // 8))
    wsf = L.mmseg_conv3_wgrad_ws_floats(V, cout, cip, ci, shift, D, H, W, cout, cip, 1)
    assert wsf > 0, "a direct single-split gradient has no reduce"
    out = {}
    for v4 in ("0", "1"):
        ws = torch.full((wsf,), float("nan"), device=dev)
        gw, gb = gw0.clone(), gb0.clone()
        assert L.mmseg_conv3_wgrad(ptr(dy), cout, ptr(x), cip, ptr(gw), ptr(gb), cout, cip, ci, shift, V, D, H, W,
                                   ptr(ws), wsf, accumulate, 1, stream_handle()) == 0
        assert not L.mmseg_last_kernel().decode().startswith("wgrad_dma")
        torch.cuda.synchronize()
        out[v4] = (gw, gb)
    assert torch.equal(out["0"][0], out["1"][0]) and torch.equal(out["0"][1], out["1"][1])
    xr = x.double().cpu().reshape(N, D, H, W, cip)[..., :ci].permute(0, 4, 1, 2, 3)
    dyr = dy.double().cpu().reshape(N, D, H, W, cout).permute(0, 4, 1, 2, 3)
    ref = torch.nn.grad.conv3d_weight(xr, (cout, ci, 3, 3, 3), dyr, padding=1).reshape(-1)
    assert rel(out["1"][0].double().cpu() - gw0.double().cpu(), ref) < GTOL[torch.bfloat16]
    assert rel(out["1"][1].double().cpu() - gb0.double().cpu(), dyr.sum(dim=(0, 2, 3, 4))) < GTOL[torch.bfloat16]


@pytest.mark.parametrize("cip,ci,cout,shape,accumulate", [
    (1024, 768, 64, (1, 4, 4, 4), 0), (1024, 768, 384, (1, 8, 8, 8), 1), (128, 96, 64, (1, 4, 4, 8), 1),
    (64, 32, 64, (1, 4, 4, 8), 0)])
def test_wgrad_direct_chunk_padded(dev, cip, ci, cout, shape, accumulate, monkeypatch):
    """A single-split brick weight gradient over chunk-padded input channels (ci % 32 == 0 < cip: SwinUNETR's 768 of
    1024) writes the torch-layout gradient itself at row pitch 27 ci (no workspace, no relayout reduce): against
    fp64, bitwise repeatable."""
    N, D, H, W = shape
    V = N * D * H * W
    g = torch.Generator().manual_seed(cip + ci + cout + V)
    dy = torch.randn(V, cout, generator=g).to(dev, torch.bfloat16).reshape(-1)
    x = torch.randn(V, cip, generator=g)
    x[:, ci:] = 0
    x = x.to(dev, torch.bfloat16).reshape(-1)
    gw0 = torch.randn(cout * ci * 27, generator=g).to(dev) if accumulate else torch.zeros(cout * ci * 27, device=dev)
    gb0 = torch.ones(cout, device=dev) if accumulate else torch.zeros(cout, device=dev)
    L = lib()
    shift = int(np.log2(cip // 8))
    out = {}
    for pd in ("0", "1"):
        wsf = L.mmseg_conv3_wgrad_ws_floats(V, cout, cip, ci, shift, D, H, W, cout, cip, 1)
        assert wsf == 0
        ws = torch.full((max(wsf, 1),), float("nan"), device=dev)
        gw, gb = gw0.clone(), gb0.clone()
        assert L.mmseg_conv3_wgrad(ptr(dy), cout, ptr(x), cip, ptr(gw), ptr(gb), cout, cip, ci, shift, V, D, H, W,
                                   ptr(ws) if wsf else None, wsf, accumulate, 1, stream_handle()) == 0
        torch.cuda.synchronize()
        out[pd] = (gw, gb)
    assert torch.equal(out["0"][0], out["1"][0]) and torch.equal(out["0"][1], out["1"][1])
    xr = x.double().cpu().reshape(N, D, H, W, cip)[..., :ci].permute(0, 4, 1, 2, 3)
    dyr = dy.double().cpu().reshape(N, D, H, W, cout).permute(0, 4, 1, 2, 3)
    ref = torch.nn.grad.conv3d_weight(xr, (cout, ci, 3, 3, 3), dyr, padding=1).reshape(-1)
    assert rel(out["1"][0].double().cpu() - gw0.double().cpu(), ref) < GTOL[torch.bfloat16]
    assert rel(out["1"][1].double().cpu() - gb0.double().cpu(), dyr.sum(dim=(0, 2, 3, 4))) < GTOL[torch.bfloat16]


@pytest.mark.parametrize("cip,ci,shape,accumulate", [
    (64, 48, (1, 16, 16, 16), 0), (128, 96, (1, 8, 16, 16), 1), (64, 48, (2, 8, 8, 16), 1), (64, 64, (1, 12, 8, 24), 0)])
def test_wgrad_pad16_rows_bitwise(dev, cip, ci, shape, accumulate, monkeypatch):
    """mmseg_conv3_wgrad_ex phase bit 8 (SwinUNETR's 48 real output channels in 64-row tiles): the LDS-DMA kernel
    multiplies 3 of its 4 row tiles (with the pipelined multiply).  Rows 0..47 of the weight and bias gradients are
    BITWISE those of the full 64-row launch; rows 48..63 receive zeros."""
    N, D, H, W = shape
    V = N * D * H * W
    co = 64
    g = torch.Generator().manual_seed(cip + ci + V + accumulate)
    dy = torch.randn(V, co, generator=g)
    dy[:, 48:] = 0
    dy = dy.to(dev, torch.bfloat16).reshape(-1)
    x = torch.randn(V, cip, generator=g)
    x[:, ci:] = 0
    x = x.to(dev, torch.bfloat16).reshape(-1)
    gw0 = torch.randn(co * ci * 27, generator=g).to(dev) if accumulate else torch.zeros(co * ci * 27, device=dev)
    gb0 = torch.ones(co, device=dev) if accumulate else torch.zeros(co, device=dev)
    L = lib()
    shift = int(np.log2(cip // 8))
    wsf = L.mmseg_conv3_wgrad_ws_floats(V, co, cip, ci, shift, D, H, W, co, cip, 1)
    out = {}
    for phase in (3, 11):
        ws = torch.full((max(wsf, 1),), float("nan"), device=dev)
        gw, gb = gw0.clone(), gb0.clone()
        args = (ptr(dy), co, ptr(x), cip, None, None, ptr(gw), ptr(gb), co, cip, ci, shift, V, D, H, W, ptr(ws), wsf,
                accumulate)
        assert L.mmseg_conv3_wgrad_ex(*args, phase & ~2, 1, stream_handle()) == 0   # the kernel
        assert L.mmseg_last_kernel().decode() == "wgrad_dma_kernel<CO64>"
        assert L.mmseg_conv3_wgrad_kernel(V, co, cip, ci, shift, D, H, W, co, cip, wsf, 16 if phase & 8 else 0,
                                          1).decode() == "wgrad_dma_kernel<CO64>"
        assert L.mmseg_conv3_wgrad_ex(*args, 2, 1, stream_handle()) == 0            # its split reduce
        torch.cuda.synchronize()
        out[phase] = (gw.view(co, -1), gb)
    r = 48
    assert torch.equal(out[3][0][:r], out[11][0][:r]) and torch.equal(out[3][1][:r], out[11][1][:r])
    assert torch.equal(out[11][0][r:], gw0.view(co, -1)[r:]) and torch.equal(out[11][1][r:], gb0[r:])
    xr = x.double().cpu().reshape(N, D, H, W, cip)[..., :ci].permute(0, 4, 1, 2, 3)
    dyr = dy.double().cpu().reshape(N, D, H, W, co).permute(0, 4, 1, 2, 3)
    ref = torch.nn.grad.conv3d_weight(xr, (co, ci, 3, 3, 3), dyr, padding=1).reshape(co, -1)
    assert rel(out[11][0][:r].double().cpu() - gw0.view(co, -1)[:r].double().cpu(), ref[:r]) < GTOL[torch.bfloat16]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout,shape", [(384, 384, (1, 8, 8, 8)), (768, 384, (1, 8, 8, 8)), (192, 192, (1, 16, 16, 16))])
def test_conv3_few_brick_units_take_runtime_brick(dev, dtype, cin, cout, shape, monkeypatch):
    """SwinUNETR's 8^3 / 16^3 convs (384 / 768 / 192 channels at pitch 512 / 1024 / 256) are 12-48 brick2 blocks for
    the whole chip; below MMSEG_BRICK2_MINUNITS (default 128) the plan takes the runtime-brick kernel with chunk
    splits.  Forward, data gradient and weight gradient against fp64 (as test_conv3_channel_padded)."""
    monkeypatch.delenv("MMSEG_BRICK2_MINUNITS", raising=False)
    from mmseg_amd.engine.swin import cpad
    torch.manual_seed(cin + cout)
    conv = nn.Conv3d(cin, cout, 3, padding=1, bias=False).to(dev)
    rt = Runtime(dev, dtype)
    flat = FlatParams(list(conv.parameters()))
    cip, cop = cpad(cin), cpad(cout)
    layer = Conv3(rt, conv, flat, cin_pad=cip, cout_pad=cop, pad_cols=True)
    N, D, H, W = shape
    x = torch.randn(N, cin, D, H, W, device=dev)
    xa = Act(to_ndhwc(x, dtype, ld=cip), 0, cin, cip, N, D, H, W)
    ya = Act(torch.zeros(N * D * H * W * cop, dtype=dtype, device=dev), 0, cout, cop, N, D, H, W)
    layer.pack()
    layer.fwd(xa, ya)
    torch.cuda.synchronize()
    assert lib().mmseg_last_kernel().decode().startswith("conv3_brickr_kernel")
    assert _planned_fwd(layer, xa, ya) == lib().mmseg_last_kernel().decode()
    xd = _q(x, dtype).requires_grad_(True)
    wd = _q(conv.weight, dtype).requires_grad_(True)
    ref = F.conv3d(xd, wd, padding=1)
    assert rel(from_ndhwc(ya.buf, N, cout, D, H, W, ld=cop), ref) < TOL[dtype]
    dy = torch.randn(ref.shape, device=dev)
    dya = Act(to_ndhwc(dy, dtype, ld=cop), 0, cout, cop, N, D, H, W)
    dxa = Act(torch.zeros(N * D * H * W * cip, dtype=dtype, device=dev), 0, cin, cip, N, D, H, W)
    layer.bwd(xa, dya, dxa, accumulate=False)
    (ref * _q(dy, dtype)).sum().backward()
    assert rel(from_ndhwc(dxa.buf, N, cin, D, H, W, ld=cip), xd.grad) < TOL[dtype]
    assert rel(flat.grad(conv.weight), wd.grad) < GTOL[dtype]


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("cin,shape,accumulate", [
    (32, (1, 8, 4, 32), 0), (32, (2, 28, 24, 64), 1), (64, (2, 28, 24, 64), 0), (32, (1, 12, 8, 96), 1),
    (64, (2, 8, 12, 32), 1)])
def test_wgrad_row_kernel(dev, cin, shape, accumulate, norm, monkeypatch):
    """The row-slab weight gradient (wgrad_row_kernel: 32 co, K-slabs of 32 consecutive x voxels, each halo-row
    fragment shared by the nine (kz, ky) taps of a wave, column segments walked along z; the c3 step's 96^3 32 -> 32
    and 64 -> 32 layers) against fp64 (the deferred norm: relu((x - mean) * rstd) of the bf16 x, rounded to bf16),
    with block step ranges that cross columns (2 x 28 x 24 x 64: 3 or 6 planes per block against D = 28) and
    single-plane blocks; bitwise repeatable; and against the brick kernel it replaces (MMSEG_WGRAD_ROW=0) within
    bf16 product-order noise."""
    N, D, H, W = shape
    V = N * D * H * W
    cout = 32
    g = torch.Generator().manual_seed(17 * cin + V + norm)
    dy = torch.randn(V, cout, generator=g).to(dev, torch.bfloat16).reshape(-1)
    x = (torch.randn(V, cin, generator=g) * 2 + 0.5).to(dev, torch.bfloat16).reshape(-1)
    mean = (torch.randn(N, cin, generator=g) * 0.3 + 0.5).to(dev)
    rstd = (torch.rand(N, cin, generator=g) + 0.5).to(dev)
    gw0 = torch.randn(cout * cin * 27, generator=g).to(dev) if accumulate else torch.zeros(cout * cin * 27, device=dev)
    gb0 = torch.ones(cout, device=dev) if accumulate else torch.zeros(cout, device=dev)
    L = lib()
    shift = int(np.log2(cin // 8))
    wsf = L.mmseg_conv3_wgrad_ws_floats(V, cout, cin, cin, shift, D, H, W, cout, cin, 1)

    def run():
        ws = torch.full((max(wsf, 1),), float("nan"), device=dev)
        gw, gb = gw0.clone(), gb0.clone()
        if norm:
            rc = L.mmseg_conv3_wgrad_norm(ptr(dy), cout, ptr(x), cin, ptr(mean), ptr(rstd), ptr(gw), ptr(gb), cout,
                                          cin, cin, shift, V, D, H, W, ptr(ws), wsf, accumulate, 1, stream_handle())
        else:
            rc = L.mmseg_conv3_wgrad(ptr(dy), cout, ptr(x), cin, ptr(gw), ptr(gb), cout, cin, cin, shift, V, D, H, W,
                                     ptr(ws), wsf, accumulate, 1, stream_handle())
        assert rc == 0, L.mmseg_last_error()
        name = L.mmseg_last_kernel().decode()
        assert L.mmseg_conv3_wgrad_kernel(V, cout, cin, cin, shift, D, H, W, cout, cin, wsf, 1 if norm else 0,
                                          1).decode() == name
        torch.cuda.synchronize()
        return gw, gb, name

    if norm:
        assert L.mmseg_conv3_wgrad_norm_ok(V, cout, cin, cin, shift, D, H, W, cout, cin, 1)
    gw, gb, name = run()
    assert name.startswith("wgrad_row_kernel<CO32"), name
    gw2, gb2, _ = run()
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)
    monkeypatch.setenv("MMSEG_WGRAD_ROW", "0")
    gwo, gbo, name_o = run()
    assert not name_o.startswith("wgrad_row"), name_o
    xd = x.double().cpu().reshape(N, D * H * W, cin)
    if norm:
        xd = torch.relu((xd - mean.double().cpu()[:, None, :]) * rstd.double().cpu()[:, None, :])
        xd = xd.to(torch.bfloat16).double()
    xr = xd.reshape(N, D, H, W, cin).permute(0, 4, 1, 2, 3)
    dyr = dy.double().cpu().reshape(N, D, H, W, cout).permute(0, 4, 1, 2, 3)
    ref = torch.nn.grad.conv3d_weight(xr, (cout, cin, 3, 3, 3), dyr, padding=1).reshape(-1)
    e_new = rel(gw.double().cpu() - gw0.double().cpu(), ref)
    e_old = rel(gwo.double().cpu() - gw0.double().cpu(), ref)
    print(f"\nwgrad_row {shape} cin {cin} norm {norm}: vs fp64 {e_new:.2e} (brick kernel {name_o} {e_old:.2e})")
    # exact bf16 products, fp32 sums in another order than fp64's; with the norm, the fp64 reference's own rounding
    # of relu((x - mean) * rstd) to bf16 differs from the fp32 one in a few elements (both kernels measure 1.2e-4)
    assert e_new < (GTOL[torch.bfloat16] if norm else 5e-5)
    assert rel(gb.double().cpu() - gb0.double().cpu(), dyr.sum(dim=(0, 2, 3, 4))) < 5e-5
    assert rel(gw.double().cpu(), gwo.double().cpu()) < 5e-5
