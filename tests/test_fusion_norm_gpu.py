"""The DualEncoder fusion path's kernels (csrc/instnorm.hip, csrc/pool_fuse.hip) against the fp64 restatement
tests/fusion_ref.py: modality fusion forward (as stored and over pre-norm sources), max-pool over pre-norm sources,
the attention gate and its backward, the InstanceNorm forward through every kernel, and the InstanceNorm backward
with every source of its gathered dy.

Every input -- statistics, gate weights, argmax codes -- is built here from the reference side; only
test_attention_fusion_composite feeds kernels with kernel outputs.  Input rows are wider than C with the padding
filled (PAD), output buffers are pre-filled (SENT) and must keep that value outside the C channels written.
bf16: the reference is evaluated on the bf16-rounded inputs."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import mmseg_amd  # noqa: F401
from mmseg_amd._lib import MmsegError, lib, ptr, stream_handle
from tests import fusion_ref as R
from tests.helpers import rel

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
TOL = {torch.float32: 2e-5, torch.bfloat16: 1.2e-2}     # stored activations
GTOL = {torch.float32: 2e-5, torch.bfloat16: 2e-3}      # fp32-accumulated gradients (gate, beta, coef)
DXTOL = {torch.float32: 2e-4, torch.bfloat16: 3e-2}     # InstanceNorm-backward dx
SENT = 7.0       # pre-fill of every output buffer
PAD = 1.0e4      # input row padding (finite: a kernel that read it would be far off)
JUNK = 1.0e6     # the alpha / beta entries between the strided ones


def _code(dtype):
    return 0 if dtype == torch.float32 else 1


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[ptr(t) for t in ts])


def _ints(vs):
    return (ctypes.c_int * len(vs))(*vs)


def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def _rows(x, dtype, ld, dev):
    """NCDHW values (representable in dtype) -> [N*V][ld] device rows, the padding filled with PAD."""
    C = x.shape[1]
    buf = torch.full((x.numel() // C, ld), PAD, dtype=dtype)
    buf[:, :C] = x.permute(0, 2, 3, 4, 1).reshape(-1, C).to(dtype)
    return buf.to(dev)


def _unrows(buf, N, C, D, H, W, off=0):
    return buf[:, off:off + C].double().cpu().view(N, D, H, W, C).permute(0, 4, 1, 2, 3)


def _f32(t, dev):
    return t.float().contiguous().to(dev)


def _bc(s):
    return s.double()[:, :, None, None, None]


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _norm_input(dtype, N, C, shape, seed=0):
    """(x, mean, rstd): x fp64 NCDHW, representable in dtype; mean / rstd its fp64 InstanceNorm statistics cast to
    fp32 (what the kernels are given).  No |xhat| of the rounded input is below 1e-4, so the activation mask is the
    reference's own: offenders are pushed away from the mean and the statistics recomputed."""
    gen = _gen(11, dtype == torch.bfloat16, N, C, *shape, seed)
    x = torch.randn(N, C, *shape, generator=gen, dtype=torch.float64) * 2 + 0.7
    x = x * (0.5 + torch.rand(N, C, 1, 1, 1, generator=gen, dtype=torch.float64)) + torch.randn(
        N, C, 1, 1, 1, generator=gen, dtype=torch.float64)
    x = x.to(dtype).double()
    for _ in range(50):
        mean, rstd = (t.float() for t in R.in_stats(x))
        xhat = (x - _bc(mean)) * _bc(rstd)
        bad = xhat.abs() < 1e-3
        if not bad.any():
            break
        push = torch.where(xhat >= 0, 0.05, -0.05) / _bc(rstd)
        x = torch.where(bad, x + push, x).to(dtype).double()
    mean, rstd = (t.float() for t in R.in_stats(x))
    assert ((x - _bc(mean)) * _bc(rstd)).abs().min() >= 1e-4
    return x, mean, rstd


def _gate_params(pooled, M, C, gen):
    """fp32 gate weights for pooled [N, M*C] (fp32) whose fp64 hidden pre-activations all have magnitude >= 1e-3
    (the gate's ReLU sits on no kink) and take both signs."""
    MC, Hd = M * C, M * C // 4
    W1 = (torch.randn(Hd, MC, generator=gen) / math.sqrt(MC)).float()
    b1 = (torch.randn(Hd, generator=gen) * 0.5).float()
    # logits of order 0.5: a saturated softmax (w_m -> 1) makes dlogit_m = w_m (dw_m - sum_k w_k dw_k) a difference of
    # nearly equal numbers, which measures fp32 cancellation and not the kernel
    W2 = (torch.randn(M, Hd, generator=gen) * 0.5 / math.sqrt(Hd)).float()
    b2 = (torch.randn(M, generator=gen) * 0.3).float()
    for _ in range(100):
        pre = pooled.double() @ W1.double().t() + b1.double()
        bad = (pre.abs() < 2e-3).any(dim=0)
        if not bad.any():
            break
        b1 = torch.where(bad, b1 + 0.01, b1)
    pre = pooled.double() @ W1.double().t() + b1.double()
    assert pre.abs().min() >= 1e-3 and (pre > 0).any() and (pre < 0).any()
    assert R.gate(pooled, W1, b1, W2, b2)[1].min() > 0.05
    return W1, b1, W2, b2


# ---------------------------------------------------------- fusion forward
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 24, 32])
@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_fuse_fwd(dev, dtype, C, M):
    """mmseg_fuse_fwd and mmseg_fuse_norm_fwd (M = 2, 3: the compile-time-M kernel; 1, 4: the runtime-M one) with
    wconst = 1, wconst = 1 / M and per-sample weights whose rows do not sum to 1, against fusion_ref.fuse; source
    rows of C + 8, the output in the second half of 2C-wide rows."""
    N, (D, H, W) = 2, (4, 6, 10)
    V, ld, ldo = D * H * W, C + 8, 2 * C
    L, s = lib(), stream_handle()
    gen = _gen(21, dtype == torch.bfloat16, C, M)
    xs = [(torch.randn(N, C, D, H, W, generator=gen, dtype=torch.float64) * 2
           + torch.randn(N, C, 1, 1, 1, generator=gen, dtype=torch.float64)).to(dtype).double() for _ in range(M)]
    stats = [tuple(t.float() for t in R.in_stats(x)) for x in xs]
    wts = (torch.rand(N, M, generator=gen) * 0.3 + 1.1 / M).float()      # rows sum to 1.1 .. 1.1 + 0.3 M
    assert (wts.sum(dim=1) > 1.05).all()
    srcs = [_rows(x, dtype, ld, dev) for x in xs]
    means = [_f32(st[0], dev) for st in stats]
    rstds = [_f32(st[1], dev) for st in stats]
    wd = _f32(wts, dev)
    for norm in (False, True):
        for wconst, w in ((1.0, None), (1.0 / M, None), (1.0, wts)):
            out = torch.full((N * V, ldo), SENT, dtype=dtype, device=dev)
            slot = out.data_ptr() + C * out.element_size()
            if norm:
                L.mmseg_fuse_norm_fwd(_ptrs(srcs), _ints([ld] * M), _ptrs(means), _ptrs(rstds), M, wconst,
                                      ptr(wd) if w is not None else None, slot, ldo, N, V, C, _code(dtype), s)
            else:
                L.mmseg_fuse_fwd(_ptrs(srcs), _ints([ld] * M), M, wconst, ptr(wd) if w is not None else None, slot,
                                 ldo, N, V, C, _code(dtype), s)
            torch.cuda.synchronize()
            ref = R.fuse(xs, wconst=wconst, wts=w, stats=stats if norm else None, dtype=dtype)
            err = rel(_unrows(out, N, C, D, H, W, off=C), ref)
            print(f"fuse norm={norm} wconst={wconst:.3f} wts={w is not None}: {err:.3e}")
            assert err < TOL[dtype], (norm, wconst, w is not None)
            assert (out[:, :C] == SENT).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_wts", [False, True])
def test_fuse_norm_fwd_second_grid_stride_item(dev, dtype, with_wts):
    """fuse_norm_fwd_m keeps a thread's statistics across grid-stride iterations and reloads them when the sample
    changes.  N = 3, 32^3, C = 256, M = 2: N V C / 8 = 3 * 2^20 items against a stride of 8192 * 256 = 2^21, so the
    threads of sample 0 run a second item in sample 2.  The samples' statistics differ strongly (means +3 / 0 /
    -3, scales 0.5 / 1 / 2): statistics kept from sample 0 give zeros in sample 2.  The reference is the same fp64
    fusion_ref.fuse, evaluated on the device (25 M elements per source); the error is helpers.rel's metric."""
    N, C, M, (D, H, W) = 3, 256, 2, (32, 32, 32)
    V = D * H * W
    assert N * V * (C // 8) > 8192 * 256 and (N - 1) * V * (C // 8) >= 8192 * 256   # a second item, two samples on
    L, s = lib(), stream_handle()
    gen = torch.Generator(device=dev).manual_seed(31 + int(with_wts))
    off = torch.tensor([3.0, 0.0, -3.0], device=dev).view(N, 1, 1, 1, 1)
    sc = torch.tensor([0.5, 1.0, 2.0], device=dev).view(N, 1, 1, 1, 1)
    xs, srcs, stats = [], [], []
    for m in range(M):
        rows = (torch.randn(N, D, H, W, C, generator=gen, device=dev) * sc + off * (1 - 2 * m)
                + torch.randn(N, 1, 1, 1, C, generator=gen, device=dev) * 0.3).to(dtype)
        srcs.append(rows.view(N * V, C))
        xs.append(rows.permute(0, 4, 1, 2, 3))          # NCDHW view of the stored rows
        stats.append(tuple(t.float() for t in R.in_stats(xs[m])))
        assert (stats[m][0][0] - stats[m][0][2]).abs().min() > 4.0
    wts = torch.tensor([[0.7, 0.6], [0.2, 0.5], [0.9, 0.4]], device=dev) if with_wts else None
    out = torch.full((N * V, C), SENT, dtype=dtype, device=dev)
    L.mmseg_fuse_norm_fwd(_ptrs(srcs), _ints([C] * M), _ptrs([st[0] for st in stats]), _ptrs([st[1] for st in stats]),
                          M, 0.5, ptr(wts), ptr(out), C, N, V, C, _code(dtype), s)
    torch.cuda.synchronize()
    ref = R.fuse(xs, wconst=0.5, wts=wts, stats=stats, dtype=dtype)
    got = out.view(N, D, H, W, C).permute(0, 4, 1, 2, 3).double()
    for n in range(N):      # per sample, so that a sample of zeros cannot hide behind another sample's maximum
        err = ((got[n] - ref[n]).abs().max() / ref[n].abs().max()).item()
        print(f"fuse_norm large sample {n}: {err:.3e}")
        assert err < TOL[dtype], n


# ------------------------------------------------- max-pool over pre-norm x
NEG_WIN = (0, 0, 0)       # pooled voxel whose whole window is negative after the norm: all zeros, code 0
DUP_WIN = (1, 2, 1)       # pooled voxel with the same maximum at window positions 3 and 5: code 3
DUP_POS = (3, 5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(4, 6, 8), (12, 12, 12)])
@pytest.mark.parametrize("C", [8, 24])
def test_maxpool2_norm_fwd_exact(dev, dtype, shape, C):
    """mmseg_maxpool2_norm_fwd is stated as pooling in_relu_apply's output: fp32 h = (x - mean) * rstd, h > 0 ? h : 0,
    rounded (to nearest even) to the storage dtype, then the first maximum in z, y, x order.  The reference runs the
    same IEEE operations in the same order with torch in fp32, so values and codes must be equal, not close."""
    N, (D, H, W) = 2, shape
    Vo, ld, ldy = D * H * W // 8, C + 8, C + 8
    L, s = lib(), stream_handle()
    gen = _gen(41, dtype == torch.bfloat16, C, *shape)
    x = torch.randn(N, D, H, W, C, generator=gen) * 2 + 0.3
    mu = torch.randn(N, C, generator=gen) * 0.5
    rs = torch.rand(N, C, generator=gen) + 0.5
    z, y, xx = (2 * v for v in NEG_WIN)
    x[:, z:z + 2, y:y + 2, xx:xx + 2, :] = -50.0 - torch.rand(N, 2, 2, 2, C, generator=gen)
    z, y, xx = (2 * v for v in DUP_WIN)
    for t in DUP_POS:
        x[:, z + (t >> 2), y + ((t >> 1) & 1), xx + (t & 1), :] = 40.0
    xq = x.to(dtype)
    h = (xq.float() - mu[:, None, None, None, :]) * rs[:, None, None, None, :]
    a = torch.where(h > 0, h, torch.zeros_like(h)).to(dtype)
    pref, ind = F.max_pool3d(a.double().permute(0, 4, 1, 2, 3), 2, return_indices=True)
    cref = R.codes_from_indices(ind, H, W)
    assert (cref[(slice(None), slice(None)) + NEG_WIN] == 0).all() and (pref[(slice(None), slice(None)) + NEG_WIN] == 0).all()
    assert (cref[(slice(None), slice(None)) + DUP_WIN] == DUP_POS[0]).all()
    src = torch.full((N * D * H * W, ld), PAD, dtype=dtype)
    src[:, :C] = xq.reshape(-1, C)
    src = src.to(dev)
    yb = torch.full((N * Vo, ldy), SENT, dtype=dtype, device=dev)
    idx = torch.full((N * Vo * C,), 77, dtype=torch.uint8, device=dev)
    mud, rsd = mu.to(dev), rs.to(dev)
    L.mmseg_maxpool2_norm_fwd(ptr(src), ld, ptr(mud), ptr(rsd), ptr(yb), ldy, ptr(idx), N, D, H, W, C, _code(dtype), s)
    torch.cuda.synchronize()
    assert torch.equal(_unrows(yb, N, C, D // 2, H // 2, W // 2), pref)
    assert torch.equal(idx.cpu().view(N, D // 2, H // 2, W // 2, C).permute(0, 4, 1, 2, 3).long(), cref)
    assert (yb[:, C:] == SENT).all()


# ------------------------------------------------------------------- gate
GATE_CASES = [(2, 8, 2, (4, 4, 6)), (3, 8, 3, (8, 8, 10)), (2, 64, 2, (16, 16, 18)), (3, 32, 1, (32, 32, 40))]


def _dot_chunks(V, C):
    """chunks per sample of mmseg_attn_gate_bwd's dot pass (the host formula)"""
    want = 256 * 64
    nch = min((V * (C // 8) + want - 1) // want, 256)
    vpc = (V + nch - 1) // nch
    return (V + vpc - 1) // vpc


def test_gate_cases_span_many_dot_chunks():
    nch = [_dot_chunks(math.prod(shape), C) for _, C, _, shape in GATE_CASES]
    assert min(nch) == 1 and max(nch) >= 8, nch


@functools.lru_cache(maxsize=None)
def _gate_case(dtype, M, C, N, shape):
    """Sources as stored, their fp64 channel means, conditioned gate weights, a random dfused, and the reference's
    gate outputs and gradients: autograd of sum(dfused * fuse(srcs, wts = gate(pooled))) with respect to pooled and
    the Linear parameters."""
    gen = _gen(51, dtype == torch.bfloat16, M, C, N, *shape)
    xs = [(torch.randn(N, C, *shape, generator=gen, dtype=torch.float64)
           + torch.randn(N, C, 1, 1, 1, generator=gen, dtype=torch.float64)).to(dtype).double() for _ in range(M)]
    pooled64 = torch.cat([x.mean(dim=(2, 3, 4)) for x in xs], dim=1)
    pooled = pooled64.float()
    W1, b1, W2, b2 = _gate_params(pooled, M, C, gen)
    dfused = torch.randn(N, C, *shape, generator=gen, dtype=torch.float64).to(dtype).double()
    leaves = [t.double().requires_grad_(True) for t in (pooled, W1, b1, W2, b2)]
    h, w = R.gate(*leaves)
    (R.fuse(xs, wts=w) * dfused).sum().backward()
    V = math.prod(shape)
    grads = dict(beta=leaves[0].grad / V, gW1=leaves[1].grad, gb1=leaves[2].grad, gW2=leaves[3].grad,
                 gb2=leaves[4].grad)
    return dict(xs=xs, pooled64=pooled64, pooled=pooled, W1=W1, b1=b1, W2=W2, b2=b2, dfused=dfused, h=h.detach(),
                w=w.detach(), grads=grads)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C,N,shape", GATE_CASES)
def test_gate_channel_means(dev, dtype, M, C, N, shape):
    """mmseg_instnorm_stats as the gate calls it -- rstd NULL, eps 0, mean_ld = M C, the modality's columns at
    offset m C -- against the fp64 channel means; a call writes its own C columns only."""
    D, H, W = shape
    V, ld = D * H * W, C + 8
    L, s = lib(), stream_handle()
    case = _gate_case(dtype, M, C, N, shape)
    pooled = torch.full((N, M * C), SENT, device=dev)
    ws = torch.empty(L.mmseg_instnorm_ws_floats(N, V, C), device=dev)
    for m in range(M):
        src = _rows(case["xs"][m], dtype, ld, dev)
        L.mmseg_instnorm_stats(ptr(src), ld, N, V, C, 0.0, pooled.data_ptr() + m * C * 4, M * C, None, ptr(ws),
                               _code(dtype), s)
        torch.cuda.synchronize()
        assert (pooled[:, (m + 1) * C:] == SENT).all()
    err = rel(pooled, case["pooled64"])
    print(f"gate channel means: {err:.3e}")
    assert err < GTOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C,N,shape", GATE_CASES)
def test_attn_gate_fwd(dev, dtype, M, C, N, shape):
    """hbuf and wts of mmseg_attn_gate_fwd against fusion_ref.gate (the gate itself is fp32 for either dtype; the
    dtype picks the case's pooled values)."""
    L, s = lib(), stream_handle()
    case = _gate_case(dtype, M, C, N, shape)
    Hd = M * C // 4
    hbuf = torch.full((N * Hd + 8,), SENT, device=dev)
    wts = torch.full((N * M + 8,), SENT, device=dev)
    args = [_f32(case[k], dev) for k in ("pooled", "W1", "b1", "W2", "b2")]
    L.mmseg_attn_gate_fwd(*[ptr(a) for a in args], ptr(hbuf), ptr(wts), N, M * C, Hd, M, s)
    torch.cuda.synchronize()
    eh, ew = rel(hbuf[:N * Hd].view(N, Hd), case["h"]), rel(wts[:N * M].view(N, M), case["w"])
    print(f"gate fwd: h {eh:.3e} w {ew:.3e}")
    assert eh < GTOL[dtype] and ew < GTOL[dtype]
    assert (hbuf[N * Hd:] == SENT).all() and (wts[N * M:] == SENT).all()
    assert (wts[:N * M].view(N, M).sum(dim=1) - 1).abs().max() < 1e-5


def _run_gate_bwd(dev, dtype, M, C, N, shape, srcs, ld, dfused, ldd, pooled, W1, W2, hbuf, wts, accumulate, g0):
    L, s = lib(), stream_handle()
    Hd, V = M * C // 4, math.prod(shape)
    out = dict(beta=torch.full((N * M * C + 8,), SENT, device=dev))
    for k, n in (("gW1", Hd * M * C), ("gb1", Hd), ("gW2", M * Hd), ("gb2", M)):
        out[k] = torch.full((n + 8,), SENT, device=dev)
        out[k][:n] = g0[k].reshape(-1).to(dev) if g0 is not None else float("nan") if not accumulate else 0.0
    ws = torch.empty(4 * 256 * N, device=dev)
    L.mmseg_attn_gate_bwd(_ptrs(srcs), _ints([ld] * M), M, ptr(dfused), ldd, N, V, C, ptr(pooled), ptr(W1), ptr(W2),
                          ptr(hbuf), ptr(wts), ptr(out["beta"]), ptr(out["gW1"]), ptr(out["gb1"]), ptr(out["gW2"]),
                          ptr(out["gb2"]), Hd, ptr(ws), accumulate, _code(dtype), s)
    torch.cuda.synchronize()
    sizes = dict(beta=N * M * C, gW1=Hd * M * C, gb1=Hd, gW2=M * Hd, gb2=M)
    for k, n in sizes.items():
        assert (out[k][n:] == SENT).all(), k
    return {k: out[k][:n] for k, n in sizes.items()}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("M,C,N,shape", GATE_CASES)
def test_attn_gate_bwd(dev, dtype, M, C, N, shape, accumulate):
    """beta (= dpooled / V) and the Linear gradients of mmseg_attn_gate_bwd (its dot pass included: 1 to 10 chunks
    per sample) against autograd of fuse(srcs, wts = gate(pooled)) contracted with a random dfused.  pooled, hbuf and
    wts are the reference's; source and dfused rows are wider than C.  accumulate = 1 adds to gradients already in
    place (of the reference gradients' size); accumulate = 0 overwrites NaNs."""
    case = _gate_case(dtype, M, C, N, shape)
    ld, ldd = C + 8, C + 16
    srcs = [_rows(x, dtype, ld, dev) for x in case["xs"]]
    dfused = _rows(case["dfused"], dtype, ldd, dev)
    g0 = None
    if accumulate:
        gen = _gen(52, M, C, N)
        g0 = {k: (torch.randn(v.shape, generator=gen, dtype=torch.float64) * v.abs().max()).float()
              for k, v in case["grads"].items() if k != "beta"}
    got = _run_gate_bwd(dev, dtype, M, C, N, shape, srcs, ld, dfused, ldd, _f32(case["pooled"], dev),
                        _f32(case["W1"], dev), _f32(case["W2"], dev), _f32(case["h"], dev), _f32(case["w"], dev),
                        accumulate, g0)
    for k, ref in case["grads"].items():
        want = ref + g0[k].double() if accumulate and k != "beta" else ref
        err = rel(got[k].view(ref.shape), want)
        print(f"gate bwd {k}: {err:.3e}")
        assert err < GTOL[dtype], k


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C,N,shape", GATE_CASES[:2])
def test_attention_fusion_composite(dev, dtype, M, C, N, shape):
    """The attention fusion as the engine chains it -- channel means, gate forward, weighted fusion, gate backward,
    then mmseg_instnorm_relu_bwd per modality with alpha1 = wts + m (stride M) and beta = beta + m C (stride M C) --
    against autograd through fused = sum_m softmax(MLP(avgpool(cat y_m)))[m] * y_m, y_m = relu(IN(x_m)).  The one
    test where kernel outputs feed kernels.  The reference's forward sees y_m as stored (rounded to the dtype,
    straight-through for the gradient), as the kernels do."""
    D, H, W = shape
    V, Hd, ld = D * H * W, M * C // 4, C + 8
    L, s = lib(), stream_handle()
    ins = [_norm_input(dtype, N, C, shape, seed=100 + m) for m in range(M)]
    yq = [torch.relu((x - _bc(mean)) * _bc(rstd)).to(dtype).double() for x, mean, rstd in ins]
    gen = _gen(61, dtype == torch.bfloat16, M, C)
    W1, b1, W2, b2 = _gate_params(torch.cat([y.mean(dim=(2, 3, 4)) for y in yq], dim=1).float(), M, C, gen)
    dfused = torch.randn(N, C, D, H, W, generator=gen, dtype=torch.float64).to(dtype).double()
    # reference
    xs = [x.clone().requires_grad_(True) for x, _, _ in ins]
    ye = [torch.relu(F.instance_norm(x, eps=1e-5)) for x in xs]
    ys = [e + (q - e).detach() for e, q in zip(ye, yq)]
    params = [t.double().requires_grad_(True) for t in (W1, b1, W2, b2)]
    _, w = R.gate(torch.cat([y.mean(dim=(2, 3, 4)) for y in ys], dim=1), *params)
    fused = R.fuse(ys, wts=w)
    (fused * dfused).sum().backward()
    # kernels
    srcs = [_rows(y, dtype, ld, dev) for y in yq]
    pooled = torch.empty(N, M * C, device=dev)
    ws = torch.empty(L.mmseg_instnorm_ws_floats(N, V, C), device=dev)
    for m in range(M):
        L.mmseg_instnorm_stats(ptr(srcs[m]), ld, N, V, C, 0.0, pooled.data_ptr() + m * C * 4, M * C, None, ptr(ws),
                               _code(dtype), s)
    hbuf, wts = torch.empty(N, Hd, device=dev), torch.empty(N, M, device=dev)
    dW1, db1, dW2, db2 = (_f32(t, dev) for t in (W1, b1, W2, b2))
    L.mmseg_attn_gate_fwd(ptr(pooled), ptr(dW1), ptr(db1), ptr(dW2), ptr(db2), ptr(hbuf), ptr(wts), N, M * C, Hd, M, s)
    out = torch.full((N * V, ld), SENT, dtype=dtype, device=dev)
    L.mmseg_fuse_fwd(_ptrs(srcs), _ints([ld] * M), M, 1.0, ptr(wts), ptr(out), ld, N, V, C, _code(dtype), s)
    torch.cuda.synchronize()
    err = rel(_unrows(out, N, C, D, H, W), fused)
    print(f"composite fused: {err:.3e}")
    assert err < TOL[dtype] and (out[:, C:] == SENT).all()
    dfd = _rows(dfused, dtype, ld, dev)
    got = _run_gate_bwd(dev, dtype, M, C, N, shape, srcs, ld, dfd, ld, pooled, dW1, dW2, hbuf, wts, 0, None)
    for k, p in zip(("gW1", "gb1", "gW2", "gb2"), params):
        err = rel(got[k].view(p.shape), p.grad)
        print(f"composite {k}: {err:.3e}")
        assert err < GTOL[dtype], k
    for m in range(M):
        x, mean, rstd = ins[m]
        xr, md, rd, lddx = _rows(x, dtype, ld, dev), _f32(mean, dev), _f32(rstd, dev), C + 16
        dx = torch.full((N * V, lddx), SENT, dtype=dtype, device=dev)
        L.mmseg_instnorm_relu_bwd(ptr(xr), ld, ptr(md), ptr(rd), ptr(dfd), ld, 1.0,
                                  wts.data_ptr() + m * 4, M, got["beta"].data_ptr() + m * C * 4, M * C, None, 0, None,
                                  ptr(dx), lddx, N, D, H, W, C, ptr(ws), _code(dtype), s)
        torch.cuda.synchronize()
        err = rel(_unrows(dx, N, C, D, H, W), xs[m].grad)
        print(f"composite dx[{m}]: {err:.3e}")
        assert err < DXTOL[dtype], m
        assert (dx[:, C:] == SENT).all()


def test_attn_gate_bwd_rejects_more_rows_than_threads(dev):
    """attn_gate_bwd is one 256-thread block with a thread per (n, m): N M = 260 is refused before anything is
    launched (neither the dot pass nor the gate writes), and so is a gate whose (N M + N Hd) floats exceed the LDS."""
    L, s = lib(), stream_handle()
    C, V = 8, 8
    for N, M, Hd in ((65, 4, 8), (64, 4, 256)):
        srcs = [torch.ones(N * V, C, device=dev) for _ in range(M)]
        f = {k: torch.full((n,), SENT, device=dev) for k, n in
             (("pooled", N * M * C), ("W1", Hd * M * C), ("W2", M * Hd), ("hbuf", N * Hd), ("wts", N * M),
              ("beta", N * M * C), ("gW1", Hd * M * C), ("gb1", Hd), ("gW2", M * Hd), ("gb2", M),
              ("ws", 4 * 256 * N))}
        with pytest.raises(MmsegError):
            L.mmseg_attn_gate_bwd(_ptrs(srcs), _ints([C] * M), M, ptr(srcs[0]), C, N, V, C, ptr(f["pooled"]),
                                  ptr(f["W1"]), ptr(f["W2"]), ptr(f["hbuf"]), ptr(f["wts"]), ptr(f["beta"]),
                                  ptr(f["gW1"]), ptr(f["gb1"]), ptr(f["gW2"]), ptr(f["gb2"]), Hd, ptr(f["ws"]), 0, 0, s)
        torch.cuda.synchronize()
        assert all((t == SENT).all() for t in f.values()), (N, M, Hd)


# --------------------------------------------- InstanceNorm backward, gathered dy
IN_SHAPES = [(4, 6, 8), (8, 8, 10), (12, 12, 12), (16, 16, 18)]    # V = 192, 640, 1728, 4608
COMBOS = ("p1", "p1_alpha_beta", "beta_pool", "all")


def test_in_shapes_take_every_small_kernel():
    """V <= 256 (in_small_bwd_r<1>), <= 2048 (two sizes of in_small_bwd_r<8>, one the 12^3 level's), above
    (in_small_bwd); MMSEG_IN_SMALL_V = 0 sends all four to the partial / finalize / apply passes."""
    v = [math.prod(sh) for sh in IN_SHAPES]
    assert v[0] <= 256 < v[1] <= 2048 and 256 < v[2] <= 2048 < v[3] <= 16384


@functools.lru_cache(maxsize=None)
def _dy_sources(dtype, N, C, shape, nmod=0, seed=0):
    """The dy sources (values representable in dtype): p1 (nmod > 0: nmod samples that differ strongly), alpha [N],
    beta [N, C], pool_dy and random window codes 0..7 that no forward produced."""
    D, H, W = shape
    gen = _gen(71, dtype == torch.bfloat16, N, C, *shape, nmod, seed)
    n1 = nmod if nmod else N
    p1 = torch.randn(n1, C, D, H, W, generator=gen, dtype=torch.float64)
    if nmod:
        k = torch.arange(n1, dtype=torch.float64).view(n1, 1, 1, 1, 1)
        p1 = p1 * (1 + 2 * k) + 2 * k
    alpha = torch.rand(N, generator=gen) + 0.2
    beta = torch.randn(N, C, generator=gen) * 0.5
    pool_dy = torch.randn(N, C, D // 2, H // 2, W // 2, generator=gen, dtype=torch.float64)
    codes = torch.randint(0, 8, (N, C, D // 2, H // 2, W // 2), generator=gen)
    return p1.to(dtype).double(), alpha, beta, pool_dy.to(dtype).double(), codes


def _code_rows(codes, dev):
    """[N, C, Do, Ho, Wo] -> the kernels' [N][Vo][C] uint8"""
    return codes.permute(0, 2, 3, 4, 1).contiguous().to(torch.uint8).to(dev)


def _strided(vals, stride, off, dev, span):
    """vals [N, k] placed at buf[n * stride + off + j], JUNK elsewhere; (buffer, pointer to element off).  The buffer
    spans N * span + off elements, so a kernel that walked it with another of the test's strides reads JUNK, not
    memory outside it."""
    N, k = vals.shape
    buf = torch.full((N * max(stride, span) + off + k,), JUNK)
    for n in range(N):
        buf[n * stride + off:n * stride + off + k] = vals[n]
    buf = buf.to(dev)
    return buf, buf.data_ptr() + off * 4


# Worst error (tests.helpers.rel) of the kernels' fp32 mean / rstd against the fp64 statistics over the 96 cases of
# test_instnorm_fwd_every_kernel, measured on an MI355X with the library as it was before the InstanceNorm reductions
# got one definition each.  The bounds are 4x that: the fp32 rounding of a Welford pass depends on the input and
# moves either figure by a few ulp.
MEAN_MEASURED, RSTD_MEASURED = 2.276e-7, 2.281e-7
MEAN_TOL, RSTD_TOL = 4 * MEAN_MEASURED, 4 * RSTD_MEASURED


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("C", [8, 24, 64])
@pytest.mark.parametrize("small_v", ["16384", "0"])
@pytest.mark.parametrize("shape", IN_SHAPES)
def test_instnorm_fwd_every_kernel(dev, dtype, shape, small_v, C, relu, monkeypatch):
    """mmseg_instnorm_fwd through every forward kernel: in_small_fwd_r<1>, both sizes of in_small_fwd_r<8> and
    in_small_fwd (small_v 16384), or in_stats_partial / _finalize / in_relu_apply (small_v 0; C = 24 takes the
    partial kernels' serial reduction, 8 and 64 the shuffle tree), with and without the ReLU, on strided rows.
    y against the fp64 reference, mean / rstd against the fp64 statistics, nothing written past C -- and y equal bit
    for bit to what mmseg_instnorm_apply writes from the returned mean / rstd: every forward kernel normalises with
    in_relu_apply's expression."""
    monkeypatch.setenv("MMSEG_IN_SMALL_V", small_v)
    N, (D, H, W) = 2, shape
    V, ldx, ldy = D * H * W, C + 8, C + 16
    L, s = lib(), stream_handle()
    x = _norm_input(dtype, N, C, shape)[0]
    mean, rstd = R.in_stats(x)
    xr = _rows(x, dtype, ldx, dev)
    y = torch.full((N * V, ldy), SENT, dtype=dtype, device=dev)
    stats = torch.full((2, N * C + 8), SENT, device=dev)
    ws = torch.empty(L.mmseg_instnorm_ws_floats(N, V, C), device=dev)
    L.mmseg_instnorm_fwd(ptr(xr), ldx, ptr(y), ldy, N, V, C, 1e-5, ptr(stats[0]), C, ptr(stats[1]), relu, ptr(ws),
                         _code(dtype), s)
    torch.cuda.synchronize()
    ref = (x - _bc(mean)) * _bc(rstd)
    ey = rel(_unrows(y, N, C, D, H, W), torch.relu(ref) if relu else ref)
    em, er = rel(stats[0, :N * C].view(N, C), mean), rel(stats[1, :N * C].view(N, C), rstd)
    print(f"instnorm_fwd: y {ey:.3e}, mean {em:.3e}, rstd {er:.3e}")
    assert ey < TOL[dtype]
    assert (y[:, C:] == SENT).all() and (stats[:, N * C:] == SENT).all()
    assert em < MEAN_TOL and er < RSTD_TOL
    y2 = torch.full_like(y, SENT)
    L.mmseg_instnorm_apply(ptr(xr), ldx, ptr(y2), ldy, N, V, C, ptr(stats[0]), ptr(stats[1]), relu, _code(dtype), s)
    torch.cuda.synchronize()
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(y.view(bits), y2.view(bits))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("C", [8, 24, 64])
@pytest.mark.parametrize("small_v", ["16384", "0"])
@pytest.mark.parametrize("shape", IN_SHAPES)
def test_instnorm_bwd_gathered_dy(dev, dtype, shape, small_v, C, relu, monkeypatch):
    """mmseg_instnorm_relu_bwd / mmseg_instnorm_bwd (relu 0: the CrossAttentionFusion residual norm) with dy =
    scale1 alpha1[n] p1 + beta[n][c] + maxpool_bwd(pool_dy, pool_idx) in four source combinations -- p1 with scale1 =
    0.5 (mean fusion); p1, alpha (stride 3) and beta (stride 3 C) behind offset pointers (attention fusion); beta and
    pool_dy with p1 NULL; all four -- against fusion_ref.in_bwd(gather_dy).  Statistics are the fp64 reference's
    cast to fp32, the codes random; every row stride differs and is wider than C."""
    monkeypatch.setenv("MMSEG_IN_SMALL_V", small_v)
    N, (D, H, W) = 2, shape
    V = D * H * W
    ldx, ld1, pool_ld, lddx = C + 8, C + 16, C + 24, C + 32
    L, s = lib(), stream_handle()
    x, mean, rstd = _norm_input(dtype, N, C, shape)
    p1, alpha, beta, pool_dy, codes = _dy_sources(dtype, N, C, shape)
    xr, p1r, pdr, idx = _rows(x, dtype, ldx, dev), _rows(p1, dtype, ld1, dev), _rows(pool_dy, dtype, pool_ld, dev), \
        _code_rows(codes, dev)
    md, rd = _f32(mean, dev), _f32(rstd, dev)
    abuf, aptr = _strided(alpha.view(N, 1), 3, 1, dev, 3 * C)
    bbuf, bptr = _strided(beta, 3 * C, C, dev, 3 * C)
    ws = torch.empty(L.mmseg_instnorm_ws_floats(N, V, C), device=dev)
    for i, combo in enumerate(COMBOS):
        has_p1, has_ab, has_beta, has_pool = combo != "beta_pool", combo in ("p1_alpha_beta", "all"), combo != "p1", \
            combo in ("beta_pool", "all")
        scale1 = 1.0 if combo == "p1_alpha_beta" else 0.5
        dx = torch.full((N * V, lddx), SENT, dtype=dtype, device=dev)
        args = (ptr(xr), ldx, ptr(md), ptr(rd), ptr(p1r) if has_p1 else None, ld1 if has_p1 else 0, scale1,
                aptr if has_ab else None, 3 if has_ab else 0, bptr if has_beta else None, 3 * C if has_beta else 0,
                ptr(pdr) if has_pool else None, pool_ld if has_pool else 0, ptr(idx) if has_pool else None, ptr(dx),
                lddx, N, D, H, W, C)
        if relu and i % 2 == 0:
            L.mmseg_instnorm_relu_bwd(*args, ptr(ws), _code(dtype), s)
        else:
            L.mmseg_instnorm_bwd(*args, relu, ptr(ws), _code(dtype), s)
        torch.cuda.synchronize()
        dy = R.gather_dy(p1 if has_p1 else None, scale1, alpha if has_ab else None, beta if has_beta else None,
                         pool_dy if has_pool else None, codes if has_pool else None, shape=(N, C, D, H, W))
        err = rel(_unrows(dx, N, C, D, H, W), R.in_bwd(x, mean, rstd, dy, relu))
        print(f"in_bwd {combo}: {err:.3e}")
        assert err < DXTOL[dtype], combo
        assert (dx[:, C:] == SENT).all(), combo


@pytest.mark.parametrize("dtype", DTYPES)
def test_instnorm_act_bwd_zero_fills_channel_padding(dev, dtype, monkeypatch):
    """mmseg_instnorm_act_bwd (act 1) with Cw = C + 8 on the partial / apply path: dx against the reference, exact
    zeros in channels [C, Cw), nothing beyond Cw."""
    monkeypatch.setenv("MMSEG_IN_SMALL_V", "0")
    N, C, (D, H, W) = 2, 24, (8, 8, 10)
    V, ldx, ldg, lddx, Cw = D * H * W, C + 8, C + 16, C + 32, C + 8
    L, s = lib(), stream_handle()
    x, mean, rstd = _norm_input(dtype, N, C, (D, H, W))
    g = _dy_sources(dtype, N, C, (D, H, W))[0]
    dx = torch.full((N * V, lddx), SENT, dtype=dtype, device=dev)
    ws = torch.empty(L.mmseg_instnorm_ws_floats(N, V, C), device=dev)
    xr, md, rd, gr = _rows(x, dtype, ldx, dev), _f32(mean, dev), _f32(rstd, dev), _rows(g, dtype, ldg, dev)
    L.mmseg_instnorm_act_bwd(ptr(xr), ldx, ptr(md), ptr(rd), ptr(gr), ldg, ptr(dx), lddx, N, D, H, W, C, Cw, 1, 0.0,
                             None, 0, ptr(ws), _code(dtype), s)
    torch.cuda.synchronize()
    assert rel(_unrows(dx, N, C, D, H, W), R.in_bwd(x, mean, rstd, g, 1)) < DXTOL[dtype]
    assert (dx[:, C:Cw] == 0).all() and (dx[:, Cw:] == SENT).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("small_v", ["16384", "0"])
@pytest.mark.parametrize("with_pool", [False, True])
@pytest.mark.parametrize("N", [6, 4])
@pytest.mark.parametrize("C,shape", [(24, (8, 8, 10)), (8, (16, 16, 18))])
def test_instnorm_relu_bwd_group(dev, dtype, C, shape, N, with_pool, small_v, monkeypatch):
    """mmseg_instnorm_relu_bwd_group: N = G x 2 samples, sample n reads p1 sample n % 2 (G = 3 and 2; with the
    multi-pass kernels the blocks are chunk-major, DySrc::gsplit).  The two p1 samples differ in scale and offset, so
    a wrong sample map cannot pass."""
    monkeypatch.setenv("MMSEG_IN_SMALL_V", small_v)
    nmod, (D, H, W) = 2, shape
    V = D * H * W
    ldx, ld1, pool_ld, lddx = C + 8, C + 16, C + 24, C + 32
    L, s = lib(), stream_handle()
    x, mean, rstd = _norm_input(dtype, N, C, shape)
    p1, _, _, pool_dy, codes = _dy_sources(dtype, N, C, shape, nmod=nmod)
    dx = torch.full((N * V, lddx), SENT, dtype=dtype, device=dev)
    ws = torch.empty(L.mmseg_instnorm_ws_floats(N, V, C), device=dev)
    pdr, idx = _rows(pool_dy, dtype, pool_ld, dev), _code_rows(codes, dev)
    xr, md, rd, p1r = _rows(x, dtype, ldx, dev), _f32(mean, dev), _f32(rstd, dev), _rows(p1, dtype, ld1, dev)
    L.mmseg_instnorm_relu_bwd_group(ptr(xr), ldx, ptr(md), ptr(rd), ptr(p1r), ld1, 0.5, nmod,
                                    ptr(pdr) if with_pool else None,
                                    pool_ld if with_pool else 0, ptr(idx) if with_pool else None, ptr(dx), lddx, N, D,
                                    H, W, C, ptr(ws), _code(dtype), s)
    torch.cuda.synchronize()
    dy = R.gather_dy(p1, 0.5, None, None, pool_dy if with_pool else None, codes if with_pool else None, p1_nmod=nmod,
                     shape=(N, C, D, H, W))
    ref = R.in_bwd(x, mean, rstd, dy, 1)
    got = _unrows(dx, N, C, D, H, W)
    for n in range(N):      # per sample: the samples' gradients differ in size with their p1 sample
        err = rel(got[n], ref[n])
        print(f"in_bwd group sample {n}: {err:.3e}")
        assert err < DXTOL[dtype], n
    assert (dx[:, C:] == SENT).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("C", [8, 24, 64])
def test_instnorm_bwd_coef(dev, dtype, C, relu):
    """mmseg_instnorm_bwd_coef at V = 4608 (several chunks per sample): coef [N][C][2] = (mean g, mean g xhat)
    against fusion_ref.in_bwd_coef."""
    N, (D, H, W) = 2, IN_SHAPES[3]
    V, ldx, ld1 = D * H * W, C + 8, C + 16
    L, s = lib(), stream_handle()
    assert L.mmseg_instnorm_part_chunks(V, C) > 1
    x, mean, rstd = _norm_input(dtype, N, C, (D, H, W))
    # both means well away from zero (of a zero-mean p1 independent of x they would be sums that cancel)
    p1 = _dy_sources(dtype, N, C, (D, H, W))[0] + 0.25 + 0.3 * (x - _bc(mean)) * _bc(rstd)
    p1 = p1.to(dtype).double()
    coef = torch.full((N * C * 2 + 8,), SENT, device=dev)
    ws = torch.empty(L.mmseg_instnorm_ws_floats(N, V, C), device=dev)
    xr, md, rd, p1r = _rows(x, dtype, ldx, dev), _f32(mean, dev), _f32(rstd, dev), _rows(p1, dtype, ld1, dev)
    L.mmseg_instnorm_bwd_coef(ptr(xr), ldx, ptr(md), ptr(rd), ptr(p1r), ld1, N, D, H, W, C, relu, None, 0, ptr(coef),
                              ptr(ws), _code(dtype), s)
    torch.cuda.synchronize()
    ca, cb = R.in_bwd_coef(x, mean, rstd, p1, relu)
    got = coef[:N * C * 2].view(N, C, 2)
    ea, eb = rel(got[..., 0], ca), rel(got[..., 1], cb)
    print(f"in_bwd_coef: mean g {ea:.3e}, mean g xhat {eb:.3e}")
    assert ea < GTOL[dtype] and eb < GTOL[dtype]
    assert (coef[N * C * 2:] == SENT).all()
