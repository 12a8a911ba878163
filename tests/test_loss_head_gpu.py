"""Loss and fused head + loss kernels (csrc/loss_head.hip) against the fp64 restatement in tests/loss_ref.py, driven
directly (no network around them) over the template space the whole-network tests do not reach: every class count
2..8 of the fused pair at Cin = 8 / 16 / 32 (class slots 3 / 6 / 8, with and without empty slots, classes 4..7 in
the second lane group), the runtime-C unfused kernels at C = 2, 4, 5, 8, 16, several voxel chunks with a ragged last
one, a class absent from a sample, saturated logits, both label types, the Dropout3d-scale and MMSEG_HEAD_BF16=0
instances, the deferred norm, padded pitches, dx = null / aliasing x, accumulation, the InstanceNorm-backward
partials and the label edges.

Volumes: (5, 7, 101) = 3535 voxels = 3 statistics chunks of 1179 and 2 backward chunks of 1768 (neither a multiple
of the 16-voxel tile; the last chunk is short), and (3, 3, 5) = 45 voxels (less than one wave step).  N = 2.

Bounds are the suite's existing ones for the same outputs: loss 2e-6 max(1, |loss|) in fp32 and 1e-5 max(1, |loss|)
with bf16 storage, dlogits 1e-5, dx TOL[dtype], gW / gb GTOL[dtype] (tests/test_kernels_gpu.py), all as
helpers.rel (max error over max reference) except the loss.

Largest errors observed on an MI355X over all cases of this file (every case prints its own as an "ERR" line; the
bf16 figures are first measurements on these shapes):

  output                      fp32 storage        bf16 storage
  loss / max(1, |loss|)       2.3e-7  (2e-6)      2.1e-6  (1e-5)
  dlogits (unfused)           1.4e-6  (1e-5)      --
  dx                          4.9e-6  (2e-5)      3.7e-3  (1.2e-2)   bf16: the rounding of dx itself
  gW                          2.6e-6  (2e-5)      7.0e-5  (2e-3)
  gb                          1.8e-6  (2e-5)      4.4e-5  (2e-3)
  inpart sum g   / sum |g|    2.3e-7  (1e-5)      1.8e-4  (2^-8)
  inpart sum g h / sum |g h|  2.2e-7  (1e-5)      2.4e-4  (2^-8)

(bound in parentheses).  The fp32 dx figure is at the saturated logits; torch evaluating the same head in float32
on the CPU is 5.5e-6 from fp64 there.
"""
import functools
import math

import pytest
import torch
import torch.nn as nn

import mmseg_amd  # noqa: F401
from mmseg_amd.engine.layers import Head
from mmseg_amd.engine.runtime import Act, FlatParams, Runtime
from mmseg_amd.trainer.losses import CrossEntropyLoss, DiceCELoss, DiceLoss, FocalLoss, TverskyLoss
from tests.helpers import from_ndhwc, rel, to_ndhwc
from tests.loss_ref import head_input, head_loss_ref, label_masks, loss_ref
from tests.test_kernels_gpu import GTOL, TOL

pytestmark = pytest.mark.gpu

N = 2
VOLS = {"v3535": (5, 7, 101), "v45": (3, 3, 5)}
DTYPES = [torch.float32, torch.bfloat16]
LTYPES = [torch.int64, torch.uint8]
GOUT = 0.25                 # the output gradient the backward is scaled by
SENTINEL = 7.25             # exact in bf16
LOSS_TOL = {torch.float32: 2e-6, torch.bfloat16: 1e-5}
IN_EPS = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -8}


def _ids(v):
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None


def _labels(g, C, vol):
    """Labels from [0, C - 1): class C - 1 is absent everywhere; sample 1 also lacks class 0 (unless C = 2)."""
    y = torch.randint(0, C - 1, (N, *vol), generator=g)
    if C > 2:
        y[1] = torch.randint(1, C - 1, vol, generator=g)
    return y


def _report(what, dtype, err, bound):
    print(f"ERR {what} {_ids(dtype)} {err:.3e} bound {bound:.1e}")
    assert err < bound, (what, err, bound)


def _check_loss(got, want, dtype, tag):
    bound = LOSS_TOL[dtype] * max(1.0, abs(want))
    print(f"ERR loss {_ids(dtype)} {abs(got - want) / max(1.0, abs(want)):.3e} bound {LOSS_TOL[dtype]:.1e}")
    assert math.isfinite(got) and abs(got - want) < bound, (tag, got, want)


# ------------------------------------------------------------------------------------------------ unfused losses
def _unfused_losses(cw):
    return {"dicece_w": DiceCELoss(0.3, 0.7, class_weights=cw), "dicece_nobg": DiceCELoss(include_background=False),
            "dice": DiceLoss(), "ce_w": CrossEntropyLoss(weight=cw), "tversky_37": TverskyLoss(0.3, 0.7),
            "focal": FocalLoss(), "focal_w": FocalLoss(alpha=cw)}


@functools.lru_cache(maxsize=None)
def _unfused_case(C, vname, scale):
    """Inputs and the fp64 loss / dlogits of every loss, computed once and shared by the label types."""
    vol = VOLS[vname]
    g = torch.Generator().manual_seed(1000 * C + 10 * len(vname) + scale)
    logits = torch.randn(N, C, *vol, generator=g) * scale
    y = _labels(g, C, vol)
    cw = torch.rand(C, generator=g) + 0.5
    refs = {}
    for name, mod in _unfused_losses(cw).items():
        z = logits.double().requires_grad_(True)
        loss = loss_ref(z, y, mod._spec(), getattr(mod, "class_weights", None))
        (loss * GOUT).backward()
        refs[name] = (loss.item(), z.grad)
    return logits, y, cw, refs


def _run_unfused(dev, C, vname, scale, ltype):
    logits, y, cw, refs = _unfused_case(C, vname, scale)
    assert int((y == C - 1).sum()) == 0 and (C == 2 or int((y[1] == 0).sum()) == 0)
    lab = y.to(ltype).to(dev)
    for name, mod in _unfused_losses(cw).items():
        lg = logits.to(dev).requires_grad_(True)
        loss = mod(lg, lab)
        (loss * GOUT).backward()
        want, dref = refs[name]
        _check_loss(loss.item(), want, torch.float32, (name, C, vname, scale))
        _report(f"dlogits[{name}]", torch.float32, rel(lg.grad, dref), 1e-5)
        assert mod.invalid_labels() == 0


@pytest.mark.parametrize("ltype", LTYPES, ids=_ids)
@pytest.mark.parametrize("scale", [3, 30])
@pytest.mark.parametrize("vname", list(VOLS))
@pytest.mark.parametrize("C", [2, 4, 5, 8, 16])
def test_unfused_losses_runtime_c(dev, C, vname, scale, ltype):
    """loss_stats_kernel<LT, 0> / loss_bwd_kernel<LT, 0> (runtime C, one voxel per thread) and the finalize pass."""
    _run_unfused(dev, C, vname, scale, ltype)


@pytest.mark.parametrize("ltype", LTYPES, ids=_ids)
@pytest.mark.parametrize("scale", [3, 30])
@pytest.mark.parametrize("C", [3, 6, 7])
def test_unfused_losses_fixed_c_multi_chunk(dev, C, scale, ltype):
    """The 4-voxels-per-thread instances over three chunks with a ragged last one."""
    _run_unfused(dev, C, "v3535", scale, ltype)


# ------------------------------------------------------------------------------------------- fused head + loss
def _fused_inputs(Cin, C, vname, wscale=1, seed=0):
    """Features of scale 3 and a head whose logits have standard deviation ~3 * wscale."""
    vol = VOLS[vname]
    g = torch.Generator().manual_seed(100000 * seed + 1000 * Cin + 10 * C + len(vname) + wscale)
    return dict(x=torch.randn(N, Cin, *vol, generator=g) * 3,
                W=torch.randn(C, Cin, generator=g) * (wscale / math.sqrt(Cin)), b=torch.randn(C, generator=g),
                y=_labels(g, C, vol), cw=torch.rand(C, generator=g) + 0.5,
                mean=torch.randn(N, Cin, generator=g), rstd=torch.rand(N, Cin, generator=g) + 0.5,
                dscale=(torch.rand(N, Cin, generator=g) > 0.3).float() / 0.7)


def _f32(t, dev):
    return None if t is None else t.to(dev, torch.float32).contiguous()


def _run_fused(dev, dtype, inp, spec, cw, labels, dscale=None, norm=None, ldx=None, lddx=None, dx="own", prior=None,
               inpart=False):
    """One fused forward + backward.  dx: "own" (a buffer of pitch lddx filled with SENTINEL), "none" or "alias"
    (the feature buffer itself); prior: gradient-arena contents to accumulate onto."""
    x, W, b = inp["x"], inp["W"], inp["b"]
    _, Cin, D, H, Wd = x.shape
    C = W.shape[0]
    conv = nn.Conv3d(Cin, C, 1).to(dev)
    with torch.no_grad():
        conv.weight.copy_(W.view(C, Cin, 1, 1, 1))
        conv.bias.copy_(b)
    rt = Runtime(dev, dtype)
    flat = FlatParams(list(conv.parameters()))
    head = Head(rt, conv, flat)
    ldx = ldx or Cin
    xbuf = to_ndhwc(x.to(dev), dtype, ld=ldx)
    if ldx > Cin:
        xbuf.view(-1, ldx)[:, Cin:] = float("nan")
    xa = Act(xbuf, 0, Cin, ldx, N, D, H, Wd)
    assert head.loss_ok(xa)
    nd = None if norm is None else (_f32(norm[0], dev), _f32(norm[1], dev))
    loss, ws = head.fwd_loss(xa, labels.to(dev), spec, _f32(cw, dev), _f32(dscale, dev), norm=nd)
    nch = head.in_chunks(xa)
    ip = None
    if inpart:
        assert nch > 0
        ip = torch.zeros(N, nch, Cin, 2, device=dev)
    dbuf = None
    if dx == "none":
        dxa = None
    elif dx == "alias":
        assert ldx == Cin
        dxa, dbuf, lddx = xa, xbuf, Cin
    else:
        lddx = lddx or Cin
        dbuf = torch.full((N * D * H * Wd * lddx,), SENTINEL, dtype=dtype, device=dev)
        dxa = Act(dbuf, 0, Cin, lddx, N, D, H, Wd)
    if prior is not None:
        flat.grad_flat.copy_(prior.to(dev))
    head.bwd_loss(xa, torch.tensor(GOUT, device=dev), dxa, accumulate=prior is not None, inpart=ip)
    torch.cuda.synchronize()
    out = dict(loss=loss.item(), bad=ws[-1].item(), in_chunks=nch,
               gW=flat.grad(conv.weight).reshape(C, Cin).cpu().clone(), gb=flat.grad(conv.bias).cpu().clone(),
               inpart=None if ip is None else ip.cpu())
    if dbuf is not None:
        out["dxbuf"] = dbuf.cpu().view(-1, lddx)
        out["dx"] = from_ndhwc(dbuf, N, Cin, D, H, Wd, ld=lddx).cpu()
    return out


def _check_fused(out, ref, dtype, tag):
    loss, dh, dW, db = ref
    _check_loss(out["loss"], loss.item(), dtype, tag)
    assert out["bad"] == 0
    if "dx" in out:
        _report("dx", dtype, rel(out["dx"], dh), TOL[dtype])
    _report("gW", dtype, rel(out["gW"], dW), GTOL[dtype])
    _report("gb", dtype, rel(out["gb"], db), GTOL[dtype])


def _absent_classes_ok(y, C):
    return int((y == C - 1).sum()) == 0 and (C == 2 or int((y[1] == 0).sum()) == 0)


PAIRS_A = [(cin, c) for cin in (8, 16, 32) for c in range(2, 9)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("idx", range(len(PAIRS_A)), ids=["cin%d_c%d" % p for p in PAIRS_A])
def test_fused_every_cin_and_class_count(dev, idx, dtype):
    """(Cin, C) over {8, 16, 32} x {2..8}: G = 1 / 2 / 4, NC = 3 / 6 / 8 full and with empty slots, weighted
    DiceCE; the label type alternates with the case."""
    Cin, C = PAIRS_A[idx]
    inp = _fused_inputs(Cin, C, "v3535")
    assert _absent_classes_ok(inp["y"], C)
    mod = DiceCELoss(0.3, 0.7, class_weights=inp["cw"])
    labels = inp["y"].to(LTYPES[idx % 2])
    out = _run_fused(dev, dtype, inp, mod._spec(), inp["cw"], labels)
    ref = head_loss_ref(inp["x"], inp["W"], inp["b"], None, None, inp["y"], mod._spec(), inp["cw"], dtype, GOUT)
    _check_fused(out, ref, dtype, (Cin, C))


def _fused_losses(cw):
    """The six losses of test_fused_head_loss_matches_unfused."""
    return {"dicece": DiceCELoss(), "dicece_w": DiceCELoss(0.3, 0.7, class_weights=cw), "dice": DiceLoss(),
            "ce_w": CrossEntropyLoss(weight=cw), "tversky": TverskyLoss(0.3, 0.7), "focal": FocalLoss()}


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("wscale", [1, 10])
@pytest.mark.parametrize("vname", list(VOLS))
@pytest.mark.parametrize("Cin,C", [(32, 6), (16, 5), (8, 2), (32, 8)])
def test_fused_every_loss(dev, Cin, C, vname, wscale, dtype):
    """Every loss type through the fused pair, at both volumes, with ordinary (std 3) and saturated (std 30)
    logits."""
    inp = _fused_inputs(Cin, C, vname, wscale, seed=1)
    for k, (name, mod) in enumerate(_fused_losses(inp["cw"]).items()):
        cw = getattr(mod, "class_weights", None)
        labels = inp["y"].to(LTYPES[k % 2])
        out = _run_fused(dev, dtype, inp, mod._spec(), cw, labels)
        ref = head_loss_ref(inp["x"], inp["W"], inp["b"], None, None, inp["y"], mod._spec(), cw, dtype, GOUT)
        _check_fused(out, ref, dtype, (name, Cin, C, vname, wscale))


ROWS = ["norm", "dscale", "head_bf16_off", "ldx_pad", "lddx_pad", "dx_none", "accumulate", "dx_alias"]
# MMSEG_HEAD_BF16 switches the logits of bf16 storage only: that row has no fp32 case
ROW_CASES = [(row, dtype) for row in ROWS for dtype in DTYPES if row != "head_bf16_off" or dtype == torch.bfloat16]


@pytest.mark.parametrize("row,dtype", ROW_CASES, ids=["%s-%s" % (r, _ids(d)) for r, d in ROW_CASES])
@pytest.mark.parametrize("Cin,C", [(32, 6), (16, 7), (8, 3)])
def test_fused_variants(dev, Cin, C, row, dtype, monkeypatch):
    """One template instance or pointer path per row, each against the fp64 reference and, where the row is about
    leaving something untouched, bit for bit against the plain run."""
    if row == "head_bf16_off":
        monkeypatch.setenv("MMSEG_HEAD_BF16", "0")
    inp = _fused_inputs(Cin, C, "v3535", seed=2)
    mod = DiceCELoss(0.3, 0.7, class_weights=inp["cw"])
    spec, cw, y = mod._spec(), inp["cw"], inp["y"]
    norm = (inp["mean"], inp["rstd"]) if row == "norm" else None
    dscale = inp["dscale"] if row == "dscale" else None
    if dscale is not None:
        assert (dscale == 0).any() and (dscale > 1).any()
    ref = head_loss_ref(inp["x"], inp["W"], inp["b"], dscale, norm, y, spec, cw, dtype, GOUT)
    run = functools.partial(_run_fused, dev, dtype, inp, spec, cw, y, dscale=dscale, norm=norm)
    if row in ("norm", "dscale", "head_bf16_off"):
        _check_fused(run(), ref, dtype, row)
        return
    base = run()
    _check_fused(base, ref, dtype, row)
    if row == "ldx_pad":        # NaN in the padding columns of x: never read
        out = run(ldx=Cin + 8)
        assert out["loss"] == base["loss"]
        for k in ("dxbuf", "gW", "gb"):
            assert torch.equal(out[k], base[k]), k
    elif row == "lddx_pad":     # the padding columns of dx: never written
        out = run(lddx=Cin + 8)
        pad = out["dxbuf"][:, Cin:]
        assert torch.equal(pad, torch.full_like(pad, SENTINEL))
        assert torch.equal(out["dxbuf"][:, :Cin], base["dxbuf"])
        assert torch.equal(out["gW"], base["gW"]) and torch.equal(out["gb"], base["gb"])
    elif row == "dx_none":
        out = run(dx="none")
        assert "dx" not in out and out["loss"] == base["loss"]
        assert torch.equal(out["gW"], base["gW"]) and torch.equal(out["gb"], base["gb"])
    elif row == "dx_alias":
        out = run(dx="alias")
        for k in ("dxbuf", "gW", "gb"):
            assert torch.equal(out[k], base[k]), k
    elif row == "accumulate":
        prior = torch.randn(C * Cin + C, generator=torch.Generator().manual_seed(9))
        out = run(prior=prior)
        got = torch.cat([out["gW"].reshape(-1), out["gb"]])
        fresh = torch.cat([base["gW"].reshape(-1), base["gb"]])
        ulp = 2.0 ** -23 * (prior.abs() + fresh.abs())
        assert ((got.double() - (prior.double() + fresh.double())).abs() <= ulp.double()).all()
        assert torch.equal(out["dxbuf"], base["dxbuf"])
    else:
        raise AssertionError(row)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("with_norm", [False, True])
@pytest.mark.parametrize("C", [3, 6, 8])
def test_fused_instnorm_partials(dev, C, with_norm, dtype):
    """inpart [N][in_chunks][32][2] summed over the chunks against fp64 sum_v g and sum_v g h, g = dx [h > 0].  The
    kernel sums dx as rounded to the storage type (at most 2^-9 per element in bf16; fp32 accumulation), hence
    |got - ref| <= eps sum_v |g| (|g h|), eps = 2^-8 in bf16 and 1e-5 in fp32."""
    inp = _fused_inputs(32, C, "v3535", seed=3)
    mod = DiceCELoss(0.3, 0.7, class_weights=inp["cw"])
    norm = (inp["mean"], inp["rstd"]) if with_norm else None
    out = _run_fused(dev, dtype, inp, mod._spec(), inp["cw"], inp["y"], norm=norm, inpart=True)
    ref = head_loss_ref(inp["x"], inp["W"], inp["b"], None, norm, inp["y"], mod._spec(), inp["cw"], dtype, GOUT)
    _check_fused(out, ref, dtype, ("inpart", C, with_norm))
    assert out["in_chunks"] == 2 and tuple(out["inpart"].shape) == (N, 2, 32, 2)
    h = head_input(inp["x"], norm, dtype)
    g = ref[1] * (h > 0)
    got = out["inpart"].double().sum(1)
    for k, (term, what) in enumerate(((g, "sum_g"), (g * h, "sum_gh"))):
        want, scale = term.sum((2, 3, 4)), term.abs().sum((2, 3, 4))
        assert (scale > 0).all()
        err = ((got[..., k] - want).abs() / scale).max().item()
        _report(f"inpart[{what}]", dtype, err, IN_EPS[dtype])


@pytest.mark.parametrize("Cin,with_dscale", [(8, False), (16, False), (32, True)])
def test_fused_instnorm_partials_unavailable(dev, Cin, with_dscale):
    """No partials for Cin = 8 / 16 or with a Dropout3d scale (in_chunks() == 0)."""
    inp = _fused_inputs(Cin, 3, "v45", seed=4)
    mod = DiceCELoss()
    out = _run_fused(dev, torch.float32, inp, mod._spec(), None, inp["y"],
                     dscale=inp["dscale"] if with_dscale else None)
    assert out["in_chunks"] == 0
    if Cin == 32:
        assert _run_fused(dev, torch.float32, inp, mod._spec(), None, inp["y"])["in_chunks"] == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("Cin,C", [(32, 6), (16, 5)])
def test_fused_label_edges(dev, Cin, C, dtype):
    """Three invalid labels (255, C, -3) and a 20 % share of -100.  Under DiceCE every one of them is invalid: NaN
    loss, exact count, finite gradients.  Pure CE and focal skip -100 (value and gradients of the reference, zero
    dx rows) and count only the three."""
    inp = _fused_inputs(Cin, C, "v3535", seed=5)
    g = torch.Generator().manual_seed(77)
    ign = inp["y"].clone()
    ign[torch.rand(ign.shape, generator=g) < 0.2] = -100
    bad = ign.clone()
    bad[0, 1, 2, 3], bad[1, 0, 0, 0], bad[1, 4, 6, 100] = 255, C, -3
    cw = inp["cw"]
    for mod in (DiceCELoss(0.3, 0.7, class_weights=cw), CrossEntropyLoss(weight=cw), FocalLoss(alpha=cw)):
        spec = mod._spec()
        out = _run_fused(dev, dtype, inp, spec, cw, bad)
        want_bad = int(label_masks(bad, C, spec)[2].sum())
        assert want_bad == (3 if spec["dice_w"] == 0 else int((bad == -100).sum()) + 3)
        assert math.isnan(out["loss"]) and out["bad"] == want_bad
        assert all(torch.isfinite(out[k]).all() for k in ("dx", "gW", "gb"))
        assert math.isnan(head_loss_ref(inp["x"], inp["W"], inp["b"], None, None, bad, spec, cw, dtype)[0].item())
    for mod in (CrossEntropyLoss(weight=cw), FocalLoss(alpha=cw)):
        spec = mod._spec()
        out = _run_fused(dev, dtype, inp, spec, cw, ign)
        ref = head_loss_ref(inp["x"], inp["W"], inp["b"], None, None, ign, spec, cw, dtype, GOUT)
        _check_fused(out, ref, dtype, ("ignore", type(mod).__name__))
        skipped = out["dx"].permute(0, 2, 3, 4, 1)[ign == -100]
        assert skipped.shape[0] > 0 and (skipped == 0).all()
