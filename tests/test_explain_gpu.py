"""Explainability on the HIP engine: every kernel of csrc/explain.hip and mmseg_stem_dgrad alone against float64
torch on small odd shapes, then the public classes on the fp32 engine against the reference's own classes
(tests/golden/explain.npz), the taps, the materialised tap gradients, side effects, determinism, the bf16 engine
and the fusion kinds.

Bounds: fp32 kernels 1e-5 max-normwise (sums of at most a few thousand fp32 terms against float64); bf16 inputs
2e-2, the project's bf16 bound; fp32 engine maps 1e-3, the project's standing fp32 parity bound; integrated
gradients max(1e-3, 4 x the fixture's own fp32-against-fp64 error).

Measured on an MI355X (max-normwise against the fixture): see DESIGN.md "Explainability"."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mmseg_amd  # noqa: F401
from mmseg_amd._lib import DTYPE_CODE, lib, stream_handle
from mmseg_amd.explainability import GradCAM, GradCAMPlusPlus, SHAPAnalyzer
from mmseg_amd.explainability import common as X
from tests import explain_ref
from tests.explain_cases import CAMS, LAYERS, build, fixture, fixture_err, inputs
from tests.helpers import rel

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-5, torch.bfloat16: 2e-2}
DTYPES = [torch.float32, torch.bfloat16]


def _ws(dev, n):
    return torch.empty(int(n), dtype=torch.float32, device=dev)


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("V", [5 * 6 * 7, 70001])
def test_seed_kernel_matches_autograd(dev, V):
    L, s = lib(), stream_handle()
    g = torch.Generator().manual_seed(V)
    x = torch.randn(1, 3, V, generator=g)
    top = x[0, 1].max().item() + 1.0
    x[0, 1, 3] = top
    x[0, 1, V - 2] = top                      # a two-way tie, in the first and the last block
    xr = x.clone().requires_grad_(True)
    xr[0, 1].max().backward()
    xd = x.to(dev)
    out = torch.full_like(xd, 7.0)
    ws = _ws(dev, L.mmseg_explain_ws_floats())
    L.mmseg_explain_seed(xd.data_ptr(), 3, V, 1, 0, out.data_ptr(), ws.data_ptr(), s)
    assert torch.equal(out.cpu(), xr.grad)
    assert out[0, 1, 3].item() == 0.5 and out[0, 1, V - 2].item() == 0.5
    xr = x.clone().requires_grad_(True)
    xr[0, 2].mean().backward()
    L.mmseg_explain_seed(xd.data_ptr(), 3, V, 2, 1, out.data_ptr(), ws.data_ptr(), s)
    assert rel(out, xr.grad) < 1e-6 and out[0, :2].abs().max().item() == 0.0


def _ndhwc(t, dtype, ld, off, dev):
    """[C, d, h, w] -> the engine layout [V][ld] with the channels at `off` (NaN elsewhere: never to be read)."""
    C = t.shape[0]
    buf = torch.full((t[0].numel(), ld), float("nan"), dtype=dtype, device=dev)
    buf[:, off:off + C] = t.reshape(C, -1).t().to(dev).to(dtype)
    return buf


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,dims,pool", [(8, (5, 6, 7), False), (32, (4, 6, 10), True), (8, (2, 2, 2), True),
                                         (24, (12, 10, 14), True), (32, (9, 11, 13), False)])
def test_cam_weights_kernel(dev, dtype, C, dims, pool):
    L, s = lib(), stream_handle()
    d, h, w = dims
    V = d * h * w
    g = torch.Generator().manual_seed(C + V)
    A = torch.randn(C, d, h, w, generator=g).clamp(min=0)
    p1 = torch.randn(C, d, h, w, generator=g)                      # both signs
    Ad, p1d = _ndhwc(A, dtype, C, 0, dev), _ndhwc(p1, dtype, 2 * C, C, dev)      # p1: a slot of a wider buffer
    sc = 0.5
    pdy = idx = None
    if pool:
        pdy = torch.randn(C, d // 2, h // 2, w // 2, generator=g)
        idx = torch.randint(0, 8, (V // 8, C), generator=g, dtype=torch.uint8)
        pdyd, idxd = _ndhwc(pdy, dtype, C, 0, dev), idx.to(dev)
    # float64 reference from the values as stored
    Ar = Ad.double().cpu().t().reshape(1, C, d, h, w)
    p1r = p1d[:, C:].double().cpu().t().reshape(1, C, d, h, w)
    pdr = pdyd.double().cpu().t().reshape(1, C, d // 2, h // 2, w // 2) if pool else None
    gr = explain_ref.dense_grad(p1r, sc, pdr, idx)
    out = torch.empty(C, dtype=torch.float32, device=dev)
    ws = _ws(dev, L.mmseg_cam_ws_floats(V, C))
    for mode in (0, 1):
        if mode == 0:
            ref = gr.mean(dim=(2, 3, 4))[0]
        else:
            g2 = gr * gr
            alpha = g2 / (2 * g2 + Ar.sum(dim=(2, 3, 4), keepdim=True) * g2 * gr + 1e-8)
            ref = (alpha * gr.clamp(min=0)).sum(dim=(2, 3, 4))[0]
        L.mmseg_cam_weights(Ad.data_ptr(), C, p1d.data_ptr() + C * p1d.element_size(), 2 * C, sc,
                            pdyd.data_ptr() if pool else None, C if pool else 0, idxd.data_ptr() if pool else None,
                            d, h, w, C, mode, out.data_ptr(), ws.data_ptr(), DTYPE_CODE[dtype], s)
        err = rel(out, ref)
        print(f"cam_weights C={C} dims={dims} pool={pool} {dtype} mode={mode}: {err:.2e}")
        assert err < TOL[dtype], (mode, err)
    if pool:        # the pool source alone (p1 null)
        L.mmseg_cam_weights(None, 0, None, 0, 1.0, pdyd.data_ptr(), C, idxd.data_ptr(), d, h, w, C, 0, out.data_ptr(),
                            ws.data_ptr(), DTYPE_CODE[dtype], s)
        ref = explain_ref.dense_grad(torch.zeros_like(p1r), 1.0, pdr, idx).mean(dim=(2, 3, 4))[0]
        assert rel(out, ref) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,V", [(8, 5 * 6 * 7), (32, 5 * 6 * 7), (24, 9 * 11 * 13), (128, 8)])
def test_cam_combine_kernel(dev, dtype, C, V):
    L, s = lib(), stream_handle()
    g = torch.Generator().manual_seed(C * V)
    A = torch.randn(C, V, 1, 1, generator=g)
    wts = torch.randn(C, generator=g).to(dev)
    Ad = _ndhwc(A, dtype, 2 * C, C, dev)
    out = torch.empty(V, dtype=torch.float32, device=dev)
    L.mmseg_cam_combine(Ad.data_ptr() + C * Ad.element_size(), 2 * C, wts.data_ptr(), V, C, out.data_ptr(),
                        DTYPE_CODE[dtype], s)
    ref = (Ad[:, C:].double().cpu() @ wts.double().cpu()).clamp(min=0)
    assert (ref > 0).any() and (ref == 0).any()
    assert rel(out, ref) < TOL[dtype]


@pytest.mark.parametrize("scale", [(2, 2, 2), (4, 4, 4), (1, 2, 4), (16, 8, 1)])
def test_cam_upsample_norm_kernel(dev, scale):
    L, s = lib(), stream_handle()
    d, h, w = 5, 6, 7
    D, H, W = d * scale[0], h * scale[1], w * scale[2]
    g = torch.Generator().manual_seed(sum(scale))
    cam = torch.randn(d, h, w, generator=g).clamp(min=0)
    out = torch.empty(D, H, W, dtype=torch.float32, device=dev)
    ws = _ws(dev, L.mmseg_explain_ws_floats())
    L.mmseg_cam_upsample_norm(cam.to(dev).data_ptr(), d, h, w, out.data_ptr(), D, H, W, ws.data_ptr(), s)
    up = F.interpolate(cam.double()[None, None], size=(D, H, W), mode="trilinear", align_corners=False)[0, 0]
    ref = (up - up.min()) / (up.max() - up.min() + 1e-8)
    assert rel(out, ref) < 1e-5
    assert out.min().item() == 0.0 and 0.999 < out.max().item() <= 1.0
    with pytest.raises(Exception, match="scale"):
        L.mmseg_cam_upsample_norm(cam.to(dev).data_ptr(), d, h, w, out.data_ptr(), 3 * d, H, W, ws.data_ptr(), s)


@pytest.mark.parametrize("with_base", [True, False])
def test_attr_kernels(dev, with_base):
    L, s = lib(), stream_handle()
    n = 2 * 5 * 6 * 7 + 1
    g = torch.Generator().manual_seed(n)
    x, b, gr = (torch.randn(n, generator=g).to(dev) for _ in range(3))
    bp = b.data_ptr() if with_base else None
    b64 = b.double() if with_base else torch.zeros(n, dtype=torch.float64, device=dev)
    out = torch.empty_like(x)
    for t in (0.0, 0.375, 1.0):
        L.mmseg_attr_lerp(x.data_ptr(), bp, t, out.data_ptr(), n, s)
        assert rel(out, b64 + t * (x.double() - b64)) < 1e-6
    L.mmseg_attr_lerp(x.data_ptr(), bp, 1.0, out.data_ptr(), n, s)
    L.mmseg_attr_finish(x.data_ptr(), bp, gr.data_ptr(), 0.25, out.data_ptr(), n, s)
    assert rel(out, (x.double() - b64) * gr.double() * 0.25) < 1e-6


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Ci,Co,dims", [(1, 8, (5, 6, 7)), (2, 32, (5, 6, 7)), (3, 16, (9, 5, 19)), (1, 24, (4, 4, 16)),
                                        (5, 8, (3, 9, 33))])
def test_stem_dgrad_kernel(dev, dtype, Ci, Co, dims):
    """Against torch.nn.grad.conv3d_input in float64: odd sizes (border voxels in every brick), more than one brick
    along each axis, a channel offset inside a wider dx, two samples, and accumulate over two calls."""
    L, s = lib(), stream_handle()
    D, H, W = dims
    N, Cx, c0 = 2, Ci + 2, 1
    g = torch.Generator().manual_seed(Ci * 100 + Co)
    gy = torch.randn(N, Co, D, H, W, generator=g)
    wt = torch.randn(Co, Ci, 3, 3, 3, generator=g).to(dev)
    gd = torch.stack([_ndhwc(gy[n], dtype, Co + 8, 8, dev) for n in range(N)])          # pitch Co + 8, offset 8
    gref = gd[:, :, 8:].double().cpu().permute(0, 2, 1).reshape(N, Co, D, H, W)
    ref = torch.nn.grad.conv3d_input((N, Ci, D, H, W), wt.double().cpu(), gref, padding=1)
    dx = torch.full((N, Cx, D, H, W), 3.0, dtype=torch.float32, device=dev)
    args = (gd.data_ptr() + 8 * gd.element_size(), Co + 8, Co, wt.data_ptr(), Ci, dx.data_ptr(), Cx, c0, N, D, H, W)
    L.mmseg_stem_dgrad(*args, 0, DTYPE_CODE[dtype], s)
    err = rel(dx[:, c0:c0 + Ci], ref)
    print(f"stem_dgrad Ci={Ci} Co={Co} dims={dims} {dtype}: {err:.2e}")
    assert err < TOL[dtype]
    border = torch.ones(D, H, W, dtype=torch.bool)
    border[1:-1, 1:-1, 1:-1] = False
    assert rel(dx[:, c0:c0 + Ci][..., border.to(dev)], ref[..., border]) < TOL[dtype]
    L.mmseg_stem_dgrad(*args, 1, DTYPE_CODE[dtype], s)
    assert rel(dx[:, c0:c0 + Ci], 2 * ref) < TOL[dtype]
    assert (dx[:, :c0] == 3.0).all() and (dx[:, c0 + Ci:] == 3.0).all()       # the other channels are not touched


# ------------------------------------------------------------------- models
@pytest.fixture(scope="module")
def fx(dev):
    g = fixture()
    x, bg = inputs(g)
    models = {n: build(g, n, device="cuda", kernels="hip").eval() for n in ("unet", "dual")}
    return g, x.to(dev), bg.to(dev), models


@pytest.fixture(scope="module")
def cpu_ref():
    """The fixture's models in float64 on the CPU (torch backend), for what the fixture does not hold."""
    g = fixture()
    x, bg = inputs(g)
    return g, x.double(), bg.double(), {n: build(g, n).double().eval() for n in ("unet", "dual")}


@pytest.mark.parametrize("name,tag,layer", CAMS)
def test_cam_matches_reference(fx, name, tag, layer):
    g, x, _, models = fx
    cls = GradCAM if tag == "gradcam" else GradCAMPlusPlus
    got = cls(models[name], ["backbone." + layer])(x, int(g["cls"]))
    err, esum, eabs = fixture_err(g, f"{name}__{tag}__{layer}", got)
    print(f"{name} {tag} {layer}: {err:.2e} (sum {esum:.2e}, abs-sum {eabs:.2e})")
    assert err < 1e-3 and esum < 1e-3 and eabs < 1e-3, (err, esum, eabs)
    assert got.min() == 0.0 and 0.999 < got.max() <= 1.0


@pytest.mark.parametrize("name", ["unet", "dual"])
def test_gradient_shap_matches_reference(fx, name):
    g, x, bg, models = fx
    got = SHAPAnalyzer(models[name], background_samples=bg).compute_shap_values(x, int(g["cls"]), "gradient")
    err, esum, eabs = fixture_err(g, f"{name}__shap_gradient", got)
    print(f"{name} gradient-SHAP: {err:.2e} (abs-sum {eabs:.2e})")
    assert err < 1e-3 and eabs < 1e-3, (err, esum, eabs)


@pytest.mark.parametrize("name", ["unet", "dual"])
def test_integrated_gradients_matches_reference(fx, name):
    g, x, bg, models = fx
    got = SHAPAnalyzer(models[name], background_samples=bg).compute_shap_values(
        x, int(g["cls"]), "integrated_gradients", n_steps=int(g["n_steps"]))
    err, _, eabs = fixture_err(g, f"{name}__shap_ig", got)
    bound = max(1e-3, 4.0 * float(g[f"{name}__shap_ig__err32"]))
    print(f"{name} integrated gradients: {err:.2e} (bound {bound:.2e}, abs-sum {eabs:.2e})")
    assert err < bound, (err, bound)


def _dense(a):
    """Sample 0 of an engine activation view as [1, C, D, H, W] float32 on the CPU (element (v, c) at
    buf[v * ld + off + c]; the decoder's split gradient views carry a whole-tensor offset in `off`)."""
    t = torch.as_strided(a.buf, (a.V, a.C), (a.ld, 1), a.buf.storage_offset() + a.off)
    return t.float().t().reshape(1, a.C, a.D, a.H, a.W).cpu()


def _hooked(bb, layers, x, cls):
    """One torch_forward + backward of output[0, cls].max(): {layer: (activation, gradient)}."""
    mods = dict(bb.named_modules())
    box, handles = {}, []
    for n in layers:
        handles.append(mods[n].register_forward_hook(lambda m, i, o, n=n: box.__setitem__(n, o)))
    try:
        with torch.enable_grad():
            out = bb.torch_forward(x)
            grads = torch.autograd.grad(out[0, cls].max(), [box[n] for n in layers])
    finally:
        for h in handles:
            h.remove()
    return {n: (box[n].detach(), gr) for n, gr in zip(layers, grads)}


@pytest.mark.parametrize("name", ["unet", "dual"])
def test_taps_and_dense_gradients_match_autograd(fx, cpu_ref, name):
    """Every valid layer: the tapped activation equals the torch backend's, and the tapped gradient sources,
    materialised (tests/explain_ref.dense_grad), equal autograd's."""
    g, x, _, models = fx
    _, x64, _, refs = cpu_ref
    bb = models[name].backbone
    layers = X.valid_layers(bb)
    cls = int(g["cls"])
    want = _hooked(refs[name].backbone, layers, x64, cls)
    res = X.engine_of(bb).explain(x, X.seed_fn(cls, X.SEED_MAX), taps=layers)
    for n in layers:
        tap = res.taps[n]
        d, h, w = tap.dims
        act = tap.act.float().t().reshape(1, tap.C, d, h, w)
        ea = rel(act, want[n][0])
        sp = tap.grad
        pdy = _dense(sp.pool_dy) if sp.pool_dy is not None else None
        idx = sp.pool_idx[: (d // 2) * (h // 2) * (w // 2) * tap.C].cpu().view(-1, tap.C) if pdy is not None else None
        dense = explain_ref.dense_grad(_dense(sp.p1), sp.scale1, pdy, idx)
        err = rel(dense, want[n][1])
        print(f"{name} tap {n}: activation {ea:.2e}, gradient {err:.2e}")
        assert ea < 1e-3 and err < 1e-3, (n, ea, err)
    # return_features reads the same level outputs
    with torch.no_grad():
        _, feats = bb(x, return_features=True)
    if name == "unet":
        t = res.taps["encoders.0.conv"]
        assert torch.equal(t.act.float().t().reshape(feats[1].shape), feats[1])
    else:
        t = res.taps["encoders.1.blocks.0.conv"]
        assert torch.equal(t.act.float().t().reshape(feats["encoder_features"][1][1].shape),
                           feats["encoder_features"][1][1])


def test_engine_error_cases(fx, dev):
    g, x, _, models = fx
    eng = X.engine_of(models["unet"].backbone)
    seed = X.seed_fn(1, X.SEED_MAX)
    for bad in ("encoders.0", "encoder.layer4", "decoder.0"):
        with pytest.raises(ValueError, match="valid names"):
            eng.explain(x, seed, taps=[bad])
    with pytest.raises(ValueError, match="one sample"):
        eng.explain(torch.cat([x, x]), seed, taps=["init_conv"])
    with pytest.raises(ValueError, match="dlogits"):
        eng.explain(x, torch.zeros(1, 2, 4, 4, 4, device=dev), taps=["init_conv"])
    from mmseg_amd.engine.engine import SegEngine
    with pytest.raises(NotImplementedError, match="SwinUNETR"):
        SegEngine(torch.nn.Identity(), "swin_unetr").explain(x, seed)


def _images(prog):
    """Every packed weight image of a UNet program."""
    out = []
    for blk in [prog.init] + prog.enc + prog.dec.blocks:
        for c in (blk.c1, blk.c2):
            out.append(c.wf)
            if c.need_dgrad:
                out.append(c.wd)
    for u in prog.dec.ups:
        out += [u.wf, u.wd]
    return out


def test_explain_has_no_side_effects(fx, dev):
    """After a training step an explain call launches no weight-gradient work and leaves every p.grad, the packed
    weight images and FlatParams.version() bitwise unchanged; the next training step is bitwise that of a run
    without the call."""
    from mmseg_amd.engine.profiler import TIMER
    from mmseg_amd.trainer.losses import get_loss
    g, x, bg, _ = fx
    gen = torch.Generator().manual_seed(5)
    xs = torch.randn(2, 2, int(g["M"]), 32, 32, 32, generator=gen).to(dev)
    ys = torch.randint(0, int(g["C"]), (2, 2, 32, 32, 32), generator=gen).to(dev)
    runs = []
    for with_explain in (False, True):
        m = build(g, "unet", device="cuda", kernels="hip").train()
        crit = get_loss(m.config)
        opt = torch.optim.SGD(m.parameters(), lr=1e-2)
        crit(m(xs[0]), ys[0]).backward()
        opt.step()
        with torch.no_grad():
            m(xs[0])            # (packs the weight images of the updated weights, in both runs)
        if with_explain:
            eng = m.backbone.__dict__["_engine"]
            before = ([p.grad.clone() for p in m.parameters()], [t.clone() for t in _images(eng.program)],
                      eng.flat.version(), eng.flat.grad_flat.clone())
            TIMER.start()
            try:
                GradCAMPlusPlus(m, ["encoders.3.conv"])(x, 1)
                SHAPAnalyzer(m, background_samples=bg).compute_shap_values(x, 1, "integrated_gradients", n_steps=2)
                names = [n for n, _ in TIMER.launches()]
            finally:
                TIMER.stop()
            assert names and any("stem_dgrad" in n for n in names)
            bad = [n for n in names if any(k in n for k in ("wgrad", "wred", "colsum", "adam"))]
            assert not bad, bad
            assert all(torch.equal(a, p.grad) for a, p in zip(before[0], m.parameters()))
            assert all(torch.equal(a, b) for a, b in zip(before[1], _images(eng.program)))
            assert eng.flat.version() == before[2] and torch.equal(before[3], eng.flat.grad_flat)
            assert m.training
        opt.zero_grad(set_to_none=True)
        out = m(xs[1])
        loss = crit(out, ys[1])
        loss.backward()
        runs.append((out.detach().clone(), loss.detach().clone(), [p.grad.clone() for p in m.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))


@pytest.mark.parametrize("name", ["unet", "dual"])
def test_maps_are_deterministic(fx, name):
    g, x, bg, models = fx
    layer = LAYERS[name][1]
    for make in (lambda: GradCAM(models[name], [layer])(x, 1), lambda: GradCAMPlusPlus(models[name], [layer])(x, 1),
                 lambda: SHAPAnalyzer(models[name], bg).compute_shap_values(x, 1, "integrated_gradients", n_steps=2)):
        assert np.array_equal(make(), make())


@pytest.mark.parametrize("name", ["unet", "dual"])
def test_bf16_engine_maps_are_sane(fx, name):
    """The bf16 engine: finite maps in [0, 1] whose maximum is r / (r + 1e-8) (r: the raw map's range).  The
    difference from the fp32 engine is printed (DESIGN.md records it), not asserted."""
    g, x, bg, models = fx
    m16 = build(g, name, device="cuda", kernels="hip", dtype="bfloat16").eval()
    for cls, tag in ((GradCAM, "gradcam"), (GradCAMPlusPlus, "gradcampp")):
        for layer in LAYERS[name]:
            a = cls(m16, [layer])(x, int(g["cls"]))
            assert np.isfinite(a).all() and a.min() == 0.0 and 0.99 < a.max() <= 1.0, (tag, layer)
            b = cls(models[name], [layer])(x, int(g["cls"]))
            print(f"bf16 vs fp32 {name} {tag} {layer}: max |diff| {np.abs(a - b).max():.3e}")
    s16 = SHAPAnalyzer(m16, background_samples=bg).compute_shap_values(x, int(g["cls"]))
    s32 = SHAPAnalyzer(models[name], background_samples=bg).compute_shap_values(x, int(g["cls"]))
    assert np.isfinite(s16).all()
    print(f"bf16 vs fp32 {name} gradient-SHAP: {np.abs(s16 - s32).max() / np.abs(s32).max():.3e} max-normwise")


@pytest.mark.parametrize("fusion", ["concat", "attention", "add"])
def test_fusion_kinds(fx, dev, fusion):
    """decoder.{j} taps work for every fusion kind and match the hook reference on the same weights in float64;
    the encoder taps of concat / attention fusion raise NotImplementedError naming the layer (add fusion serves
    them)."""
    g, x, _, _ = fx
    m = build(g, "dual", device="cuda", kernels="hip", fusion=fusion).eval()
    ref = copy.deepcopy(m.backbone).cpu().double()
    ref.__dict__.pop("_engine", None)
    layers = ["decoder.0", "decoder.3"] + (["encoders.1.blocks.2.conv"] if fusion == "add" else [])
    for layer in layers:
        for cls, pp in ((GradCAM, False), (GradCAMPlusPlus, True)):
            got = cls(m, [layer])(x, 1)
            want = explain_ref.cam(ref, ref.torch_forward, layer, x.cpu().double(), 1, plus_plus=pp)
            err = np.abs(got - want).max() / np.abs(want).max()
            assert err < 1e-3, (fusion, layer, pp, err)
    if fusion != "add":
        with pytest.raises(NotImplementedError, match="encoders.0.init_conv"):
            GradCAM(m, ["encoders.0.init_conv"])(x, 1)
        with pytest.raises(NotImplementedError, match="input gradient"):
            SHAPAnalyzer(m).compute_shap_values(x, 1)
