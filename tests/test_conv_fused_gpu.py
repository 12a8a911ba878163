"""The fused, grouped and stem-norm conv kernels, one kernel per test, against torch fp64 on the CPU evaluated on the
same storage-rounded inputs (tests/test_kernels_gpu.py is the pattern; TOL / GTOL are its bounds).  The rows and the
kernel each one must launch come from tests/conv_fused_cases.py; tests/test_conv_fused_plan_cpu.py holds the same
table against the planning queries without a GPU.

  1. ConvGroup (mmseg_conv_gemm_group / mmseg_conv3_wgrad_group) per group against fp64 conv3d;
  2. Conv3.fwd_norm (mmseg_conv3_fwd_norm) bitwise against the forward of the materialised norm, and against fp64;
  3. mmseg_conv3_dgrad_in: dx against fp64 and bitwise against the plain data gradient, the InstanceNorm-backward
     partials against fp64 sums;
  4. mmseg_stem_wgrad_inb against the fp64 weight / bias gradient for the norm's fp64 input gradient.

Every case prints its errors as "ERR" lines before it asserts.  Largest errors observed on an MI355X over all cases
of this file (bound in parentheses):

  1. grouped     out 3.3e-3, dx 3.7e-3 (1.2e-2); gW 3.6e-7, gb 8.0e-8 (2e-3), the same against twice the reference
                 after the accumulating run
  2. fwd_norm    bitwise equal on every row; 2.5e-3 from fp64 (1.2e-2)
  3. dgrad_in    dx bitwise equal to the plain data gradient, 3.4e-3 from fp64 (1.2e-2); partials sum g 9.9e-9 of
                 sum |g|, sum g h 2.9e-8 of sum |g h| (2e-5)
  4. stem inb    fp32: gW 2.4e-7 (2e-5), gb 4.5e-8 of sum |dx1| (1e-6; by helpers.rel it reads up to 9.1, see
                 STEM_GB_F32); bf16: gW 6.6e-7, gb 2.8e-4 (2e-3)
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mmseg_amd  # noqa: F401
from mmseg_amd._lib import lib, ptr, stream_handle
from mmseg_amd.engine.layers import IN_EPS, Conv3, ConvGroup
from mmseg_amd.engine.runtime import Act, FlatParams, Runtime
from tests import conv_fused_cases as C
from tests.helpers import from_ndhwc, rel, to_ndhwc
from tests.test_kernels_gpu import GTOL, TOL

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SENTINEL = 7.25            # exact in bf16 and fp32
PART_TOL = 2e-5            # the project's fp32 tolerance: fp32 sums of the stored rows against fp64 sums


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    """Only the row's knobs decide the routing; the fused rows need small volumes on the brick2 family."""
    for k in C.KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MMSEG_BRICK2_MINUNITS", "0")


def _set(monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def _q(t, dtype):
    """round through the storage dtype, return fp64 CPU"""
    return t.detach().to(dtype).double().cpu()


def _act(x, dtype, ld=None):
    N, Cx, D, H, W = x.shape
    return Act(to_ndhwc(x, dtype, ld=ld), 0, Cx, ld or Cx, N, D, H, W)


def _last():
    return lib().mmseg_last_kernel().decode()


def _report(what, err, bound):
    print(f"ERR {what} {err:.3e} bound {bound:.1e}")
    assert err < bound, (what, err, bound)


def _pow2(c):
    return 1 << (c - 1).bit_length()


def _prenorm(gen, N, Cx, D, H, W):
    """A pre-norm activation whose (sample, channel) slices differ in offset and scale, so the statistics matter
    and a kernel reading another sample's or channel's statistics is far off."""
    x = torch.randn(N, Cx, D, H, W, generator=gen)
    return x * (0.5 + 2.0 * torch.rand(N, Cx, 1, 1, 1, generator=gen)) + 1.5 * torch.randn(N, Cx, 1, 1, 1, generator=gen)


def _stats(rt, xa):
    """(mean, rstd) [N x C] of mmseg_instnorm_stats, as Block._norm_stats."""
    L = lib()
    st = torch.empty(2, xa.N * xa.C, dtype=torch.float32, device=rt.device)
    ws = torch.empty(max(L.mmseg_instnorm_ws_floats(xa.N, xa.V, xa.C), 1), dtype=torch.float32, device=rt.device)
    L.mmseg_instnorm_stats(xa.ptr, xa.ld, xa.N, xa.V, xa.C, IN_EPS, ptr(st[0]), xa.C, ptr(st[1]), ptr(ws), rt.code,
                           stream_handle())
    return st[0], st[1]


def _bc(t, N, Cx):
    """[N x C] statistics as fp64 CPU [N][C][1][1][1]"""
    return t.detach().double().cpu().view(N, Cx, 1, 1, 1)


# ------------------------------------------------------------------------------------------------ 1. grouped
def _group_case(G, N, vol, cin, cout):
    """Weights, inputs and the per-group fp64 results of a grouped row."""
    n = N // G
    convs = []
    for g in range(G):
        torch.manual_seed(100 * cin + cout + g)
        conv = nn.Conv3d(cin, cout, 3, padding=1)
        with torch.no_grad():
            conv.bias.add_(0.25 * (g + 1))
        convs.append(conv)
    gen = torch.Generator().manual_seed(cin + 3 * cout + N + vol[0])
    # a different scale per group: a group reading its neighbour's samples or weights is off by its ratio
    scale = torch.tensor([1.0 + 0.75 * g for g in range(G)]).repeat_interleave(n).view(N, 1, 1, 1, 1)
    x = torch.randn(N, cin, *vol, generator=gen) * scale
    dy = torch.randn(N, cout, *vol, generator=gen) * scale.flip(0)
    refs = []
    for g, conv in enumerate(convs):
        xd = _q(x[g * n:(g + 1) * n], BF16).requires_grad_(True)
        wd = _q(conv.weight, BF16).requires_grad_(True)
        bd = conv.bias.detach().double().requires_grad_(True)
        out = F.conv3d(xd, wd, bd, padding=1)
        (out * _q(dy[g * n:(g + 1) * n], BF16)).sum().backward()
        refs.append((out.detach(), xd.grad, wd.grad, bd.grad))
    return [c.state_dict() for c in convs], x, dy, refs


@pytest.mark.parametrize("row", C.GROUP_ROWS, ids=lambda r: f"G{r[0]}-N{r[1]}-{'x'.join(map(str, r[2]))}-{r[3]}-{r[4]}")
def test_grouped_conv_per_group_fp64(dev, row, monkeypatch):
    """ConvGroup forward and backward (accumulate False, then True on the same inputs) per group against fp64 conv3d
    (CPU) of the group's rounded samples and weights with its fp32 bias: the per-group weight stride, bias, split
    rounding and the gradient strides gw_gs / gb_gs.  The arena holds guard parameters before, between and after
    the convs' (the strides stay constant): none of their gradient floats may change."""
    G, N, vol, cin, cout, knobs, fname, _, dname, _, _, _ = row
    _set(monkeypatch, knobs)
    n, (D, H, W) = N // G, vol
    states, x, dy, refs = _group_case(G, N, vol, cin, cout)
    convs, params, guards = [], [], []
    for sd in states:
        conv = nn.Conv3d(cin, cout, 3, padding=1)
        conv.load_state_dict(sd)
        convs.append(conv.to(dev))
        guards.append(nn.Parameter(torch.zeros(24, device=dev)))
        params += [guards[-1]] + list(convs[-1].parameters())
    guards.append(nn.Parameter(torch.zeros(40, device=dev)))
    params.append(guards[-1])
    rt = Runtime(dev, BF16)
    flat = FlatParams(params)
    layers = [Conv3(rt, c, flat) for c in convs]
    for img in ("wf", "wd"):          # one combined buffer per image, as DualEncoderProgram.__init__
        ts = [getattr(l, img) for l in layers]
        comb = torch.zeros(G * ts[0].numel(), dtype=ts[0].dtype, device=dev)
        for k, l in enumerate(layers):
            setattr(l, img, comb[k * ts[0].numel():(k + 1) * ts[0].numel()])
    for l in layers:
        l.pack()
    grp = ConvGroup(layers)
    xa, dya = _act(x.to(dev), BF16), _act(dy.to(dev), BF16)
    ya, dxa = rt.act(N, D, H, W, cout), rt.act(N, D, H, W, cin)
    assert grp.layout_ok and grp.ok(xa, ya)
    grp.fwd(xa, ya)
    assert _last() == fname
    flat.grad_flat.fill_(SENTINEL)
    grp.bwd(xa, dya, dxa, accumulate=False)
    assert _last() == dname            # the data gradient is the last launch
    torch.cuda.synchronize()
    out, dx = from_ndhwc(ya.buf, N, cout, D, H, W), from_ndhwc(dxa.buf, N, cin, D, H, W)
    once = [(flat.grad(c.weight).clone(), flat.grad(c.bias).clone()) for c in convs]
    for gd in guards:
        assert (flat.grad(gd) == SENTINEL).all(), "a gradient float outside the convs' parameters changed"
    grp.bwd(xa, dya, dxa, accumulate=True)
    torch.cuda.synchronize()
    for gd in guards:
        assert (flat.grad(gd) == SENTINEL).all(), "a gradient float outside the convs' parameters changed"
    assert torch.equal(from_ndhwc(dxa.buf, N, cin, D, H, W), dx)
    for g, (conv, (oref, dxref, gwref, gbref)) in enumerate(zip(convs, refs)):
        s = slice(g * n, (g + 1) * n)
        _report(f"group{g} out", rel(out[s], oref), TOL[BF16])
        _report(f"group{g} dx", rel(dx[s], dxref), TOL[BF16])
        _report(f"group{g} gW", rel(once[g][0], gwref), GTOL[BF16])
        _report(f"group{g} gb", rel(once[g][1], gbref), GTOL[BF16])
        _report(f"group{g} gW x2", rel(flat.grad(conv.weight), 2 * gwref), GTOL[BF16])
        _report(f"group{g} gb x2", rel(flat.grad(conv.bias), 2 * gbref), GTOL[BF16])


# ----------------------------------------------------------------------------------- 2. deferred-norm forward
def _one_conv(dev, cin, cout, **kw):
    torch.manual_seed(7 * cin + cout)
    conv = nn.Conv3d(cin, cout, 3, padding=1).to(dev)
    rt = Runtime(dev, BF16)
    flat = FlatParams(list(conv.parameters()))
    layer = Conv3(rt, conv, flat, **kw)
    layer.pack()
    return conv, rt, flat, layer


def _fused_id(r):
    return f"N{r[0]}-{'x'.join(map(str, r[1]))}-{r[2]}-{r[3]}-blocks{r[4]}"


@pytest.mark.parametrize("row", C.NORM_ROWS, ids=_fused_id)
def test_fwd_norm_bitwise_and_fp64(dev, row, monkeypatch):
    """Conv3.fwd_norm(x) of a pre-norm x with mmseg_instnorm_stats' statistics is (a) bitwise the brick6 forward of
    y1 = mmseg_instnorm_relu_fwd(x) -- through the plain forward where that is brick6 too (not at 96 columns, whose
    plain forward takes 48-column brick2 tiles) and through fwd_norm(y1) with mean 0, rstd 1 (y1 >= 0 is staged
    unchanged) on every row -- and (b) within TOL of fp64 conv3d of the stored y1 with the rounded weights."""
    N, vol, cin, cout, blocks, plain = row
    _set(monkeypatch, C.knobs_of(blocks))
    D, H, W = vol
    conv, rt, flat, layer = _one_conv(dev, cin, cout, need_dgrad=False)
    L, ldo = lib(), _pow2(cout)
    gen = torch.Generator().manual_seed(N + cout)
    xa = _act(_prenorm(gen, N, cin, D, H, W).to(dev), BF16)
    mean, rstd = _stats(rt, xa)
    y1 = Act(torch.empty_like(xa.buf), 0, cin, cin, N, D, H, W)
    L.mmseg_instnorm_relu_fwd(xa.ptr, xa.ld, y1.ptr, y1.ld, N, xa.V, cin, ptr(mean), ptr(rstd), rt.code, rt.stream)
    outs = [Act(torch.zeros(N * xa.V * ldo, dtype=BF16, device=dev), 0, cout, ldo, N, D, H, W) for _ in range(3)]
    assert L.mmseg_conv3_norm_ok(N * xa.V, cout, layer.Cpad, layer.KG, layer.cpg_shift, D, H, W, xa.ld, ldo, rt.code)
    layer.fwd_norm(xa, mean, rstd, outs[0])
    assert _last() == C.BRICK6
    layer.fwd(y1, outs[1])
    assert _last() == plain
    layer.fwd_norm(y1, torch.zeros_like(mean), torch.ones_like(rstd), outs[2])
    assert _last() == C.BRICK6
    torch.cuda.synchronize()
    assert torch.equal(outs[0].buf, outs[2].buf), "fwd_norm(x) differs from the brick6 forward of the stored y1"
    if plain == C.BRICK6:
        assert torch.equal(outs[0].buf, outs[1].buf), "fwd_norm(x) differs from fwd(instnorm_relu_fwd(x))"
    ref = F.conv3d(from_ndhwc(y1.buf, N, cin, D, H, W).double().cpu(), _q(conv.weight, BF16),
                   conv.bias.detach().double().cpu(), padding=1)
    _report("fwd_norm", rel(from_ndhwc(outs[0].buf, N, cout, D, H, W, ld=ldo), ref), TOL[BF16])
    _report("fwd(y1)", rel(from_ndhwc(outs[1].buf, N, cout, D, H, W, ld=ldo), ref), TOL[BF16])


# ------------------------------------------------------------------- 3. data gradient with the IN partials
@pytest.mark.parametrize("row", C.INP_ROWS, ids=_fused_id)
def test_dgrad_in_partials(dev, row, monkeypatch):
    """mmseg_conv3_dgrad_in through Conv3._dgrad (Runtime.data_only: the data gradient alone): dx against fp64 and
    bitwise against the plain brick6 data gradient (MMSEG_DGRAD_IN_PART=0: only the epilogue differs), and the
    partials inpart [N][chunks][C][2], NaN before the launch so every slot must be written (the zeros of the samples
    a block does not touch included), summed over the chunks against sum_v g and sum_v g h.

    The brick6 INP epilogue sums the STORED rows: epi_inp reads eo[i][k], the bf16 values epi_row has just written
    (csrc/conv_brick6.hip), with g = dx [x > mean] and h = (x - mean) rstd, the product with rstd taken once per
    flush.  So the reference uses the kernel's own dx read back, and the bound is the fp32 summation's:
    |got - ref| <= 2e-5 sum_v |g| (resp. sum_v |g h|)."""
    N, vol, cin, cout, blocks, chunks = row
    _set(monkeypatch, C.knobs_of(blocks))
    D, H, W = vol
    conv, rt, flat, layer = _one_conv(dev, cin, cout)
    rt.data_only = True
    gen = torch.Generator().manual_seed(5 * N + cin + (int(blocks) if blocks else 0))
    xa = rt.act(N, D, H, W, cin)                       # the conv's input: only its shape is read
    dy = torch.randn(N, cout, D, H, W, generator=gen)
    dya = _act(dy.to(dev), BF16)
    xi = _prenorm(gen, N, cin, D, H, W)
    xia = _act(xi.to(dev), BF16)
    mean, rstd = _stats(rt, xia)
    layer._inpart = torch.full((N * chunks * cin * 2,), float("nan"), dtype=torch.float32, device=dev)
    nan_buf = layer._inpart
    dx1, dx0 = rt.act(N, D, H, W, cin), rt.act(N, D, H, W, cin)
    res = layer.bwd(xa, dya, dx1, False, inp=(xia, mean, rstd))
    assert _last() == C.BRICK6_INP
    assert res is not None and res[1] == chunks and res[0] is nan_buf
    monkeypatch.setenv("MMSEG_DGRAD_IN_PART", "0")
    assert layer.bwd(xa, dya, dx0, False, inp=(xia, mean, rstd)) is None
    assert _last() == C.BRICK6
    torch.cuda.synchronize()
    assert torch.equal(dx1.buf, dx0.buf), "dx differs between the INP and the plain brick6 data gradient"
    xd = torch.zeros(N, cin, D, H, W, dtype=torch.float64, requires_grad=True)
    (F.conv3d(xd, _q(conv.weight, BF16), None, padding=1) * _q(dy, BF16)).sum().backward()
    dx = from_ndhwc(dx1.buf, N, cin, D, H, W).double().cpu()
    _report("dx", rel(dx, xd.grad), TOL[BF16])
    part = res[0].view(N, chunks, cin, 2)
    assert torch.isfinite(part).all(), "a partial slot was not written"
    got = part.double().cpu().sum(1)
    xq, m, r = _q(xi, BF16), _bc(mean, N, cin), _bc(rstd, N, cin)
    h = (xq - m) * r
    g = dx * (xq > m)
    for k, (term, what) in enumerate(((g, "sum_g"), (g * h, "sum_gh"))):
        want, scale = term.sum((2, 3, 4)), term.abs().sum((2, 3, 4))
        assert (scale > 0).all()
        _report(f"inpart[{what}]", ((got[..., k] - want).abs() / scale).max().item(), PART_TOL)


# ------------------------------------------------ 4. stem weight gradient with the fused norm backward
def _stem_setup(dev, dtype, cr, co, shape):
    N, D, H, W = shape
    torch.manual_seed(5 + cr + co)
    conv = nn.Conv3d(cr, co, 3, padding=1).to(dev)
    rt = Runtime(dev, dtype)
    flat = FlatParams(list(conv.parameters()))
    layer = Conv3(rt, conv, flat, cin_pad=8, need_dgrad=False)
    gen = torch.Generator().manual_seed(cr + co + N * D)
    x = torch.randn(N, cr, D, H, W, generator=gen)
    xdev = x.to(dev)
    xa = rt.act(N, D, H, W, 8)
    L = lib()
    L.mmseg_pack_input(ptr(xdev), cr, 0, cr, N, D * H * W, xa.ptr, rt.code, stream_handle())
    x1 = _prenorm(gen, N, co, D, H, W)
    dy1 = torch.randn(N, co, D, H, W, generator=gen)
    x1a, dy1a = _act(x1.to(dev), dtype), _act(dy1.to(dev), dtype)
    mean, rstd = _stats(rt, x1a)
    coef = torch.empty(N * co * 2, dtype=torch.float32, device=dev)
    ws = torch.empty(max(L.mmseg_instnorm_ws_floats(N, x1a.V, co), 1), dtype=torch.float32, device=dev)
    # as Block.bwd with part = None
    L.mmseg_instnorm_bwd_coef(x1a.ptr, x1a.ld, ptr(mean), ptr(rstd), dy1a.ptr, dy1a.ld, N, D, H, W, co, 1, None, 0,
                              ptr(coef), ptr(ws), rt.code, stream_handle())
    # fp64: the norm's input gradient from the stored x1 / dy1 and the fp32 statistics, rounded through the
    # storage type (the contract is in_bwd_apply's values), then the conv's weight / bias gradient for it
    x1q, dyq, m, r = _q(x1, dtype), _q(dy1, dtype), _bc(mean, N, co), _bc(rstd, N, co)
    h = (x1q - m) * r
    g = dyq * (h > 0)
    dx1 = r * (g - g.mean((2, 3, 4), keepdim=True) - h * (g * h).mean((2, 3, 4), keepdim=True))
    dx1 = dx1.to(dtype).double()
    gw = torch.nn.grad.conv3d_weight(_q(x, dtype), (co, cr, 3, 3, 3), dx1, padding=1)
    return conv, rt, flat, layer, xa, x1a, dy1a, mean, rstd, coef, gw, dx1


# The stem bias gradient in fp32, as a fraction of sum_v |dx1|.  The bias gradient is sum_v dx1, and an InstanceNorm
# backward removes the mean of its gradient: the fp64 reference is what the rounding of dx1 to fp32 leaves of a sum
# that cancels, ~1e-6 to 1e-5 against sum_v |dx1| ~ 1e3.  Reference-side spread, measured on these shapes: the same
# reference with x1 and dy1 moved by one fp32 ulp (random direction, statistics held) moves by 0.07 to 0.43 of its
# own max (so helpers.rel at GTOL = 2e-5 cannot hold for any fp32 kernel) and by at most 7.0e-9 of sum_v |dx1|.  The
# bound is the rounding of an fp32 sum of n <= 1536 terms, sqrt(n) 2^-24 = 2.3e-6, taken at 1e-6: 140 x the
# reference's spread, 20 x the largest kernel error observed (4.5e-8).  bf16 keeps helpers.rel at GTOL: there the
# reference is the sum of dx1's bf16 rounding, ~0.1, which kernel and reference round alike.
STEM_GB_F32 = 1e-6


def _check_stem(tag, dtype, got_w, got_b, gw, dx1, times=1, prior=0.0):
    """gW by helpers.rel at GTOL; gb by helpers.rel at GTOL in bf16 and against sum_v |dx1| in fp32 (STEM_GB_F32).
    prior: what the bias gradient held before an accumulating run, on top of the earlier result."""
    _report(f"{tag} gW", rel(got_w, times * gw), GTOL[dtype])
    got_b = got_b.double().cpu() - prior
    ref_b, scale = times * dx1.sum((0, 2, 3, 4)), times * dx1.abs().sum((0, 2, 3, 4))
    if dtype == BF16:
        _report(f"{tag} gb", rel(got_b, ref_b), GTOL[dtype])
    else:
        print(f"INFO {tag} gb by helpers.rel {rel(got_b, ref_b):.3e} (max |ref| {ref_b.abs().max().item():.3e})")
        _report(f"{tag} gb / sum|dx1|", ((got_b - ref_b).abs() / scale).max().item(), STEM_GB_F32)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cr,co,shape", C.STEM_ROWS)
def test_stem_wgrad_inb(dev, dtype, cr, co, shape):
    """Conv3.bwd(inb=...) on the stem path (mmseg_stem_wgrad_inb + reduce), accumulate False then True, against
    fp64: dx1 = rstd (g - mean_v g - h mean_v (g h)), g = dy1 [h > 0], h = (x1 - mean) rstd, rounded through the
    storage type; the gradients are conv3d's for the output gradient dx1.  The gradients hold a sentinel before the
    first run (it must be overwritten); the bias gradient, whose true value is ~0, is raised by 1 before the
    accumulating run, so an overwrite there shows as a missing 1."""
    conv, rt, flat, layer, xa, x1a, dy1a, mean, rstd, coef, gw, dx1 = _stem_setup(dev, dtype, cr, co, shape)
    assert layer._stem(xa, dy1a.ld)
    flat.grad_flat.fill_(SENTINEL)
    layer.bwd(xa, dy1a, None, False, inb=(x1a, mean, rstd, coef))
    torch.cuda.synchronize()
    _check_stem("once", dtype, flat.grad(conv.weight), flat.grad(conv.bias), gw, dx1)
    flat.grad(conv.bias).add_(1.0)
    layer.bwd(xa, dy1a, None, True, inb=(x1a, mean, rstd, coef))
    torch.cuda.synchronize()
    _check_stem("accumulated", dtype, flat.grad(conv.weight), flat.grad(conv.bias), gw, dx1, times=2, prior=1.0)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
def test_stem_wgrad_inb_direct_ragged_split(dev, dtype):
    """mmseg_stem_wgrad_inb + mmseg_wgrad_reduce called directly with mmseg_stem_wgrad_splits(N, D, H, W, 2) = 2
    splits over 3 bricks (2 + 1: a ragged last split)."""
    cr, co, shape, want_ks = C.STEM_DIRECT
    N, D, H, W = shape
    conv, rt, flat, layer, xa, x1a, dy1a, mean, rstd, coef, gw, dx1 = _stem_setup(dev, dtype, cr, co, shape)
    L, s = lib(), stream_handle()
    ks, kp = L.mmseg_stem_wgrad_splits(N, D, H, W, 2), L.mmseg_stem_kp(cr)
    assert ks == want_ks
    part = torch.zeros(ks * co * kp + ks * co, dtype=torch.float32, device=dev)
    bpart = part.data_ptr() + ks * co * kp * 4
    L.mmseg_stem_wgrad_inb(dy1a.ptr, dy1a.ld, xa.ptr, xa.ld, cr, x1a.ptr, x1a.ld, ptr(mean), ptr(rstd), ptr(coef),
                           ptr(part), bpart, N, D, H, W, co, ks, rt.code, s)
    got_w, got_b = torch.full((co, cr, 3, 3, 3), SENTINEL, device=dev), torch.full((co,), SENTINEL, device=dev)
    L.mmseg_wgrad_reduce(ptr(part), ptr(got_w), bpart, ptr(got_b), co, kp, ks, cr, cr, 27, 0, s)
    torch.cuda.synchronize()
    _check_stem("direct", dtype, got_w, got_b, gw, dx1)
