"""The closed forms of tests/fusion_ref.py against torch autograd in fp64 (no GPU): the checker of
tests/test_fusion_norm_gpu.py has to be right before a kernel is measured against it."""
import pytest
import torch
import torch.nn.functional as F

from tests import fusion_ref as R

RTOL = 1e-10


def _close(a, b):
    d = b.abs().max().item()
    assert (a - b).abs().max().item() <= RTOL * (d if d > 0 else 1.0)


def _act(y, act, slope):
    return y if act == 0 else torch.relu(y) if act == 1 else F.leaky_relu(y, slope)


@pytest.mark.parametrize("act,slope", [(0, 0.0), (1, 0.0), (2, 0.01)])
def test_in_bwd_matches_autograd(act, slope):
    gen = torch.Generator().manual_seed(3 + act)
    x = (torch.randn(2, 5, 4, 6, 3, generator=gen, dtype=torch.float64) * 2 + 0.7).requires_grad_(True)
    dy = torch.randn(2, 5, 4, 6, 3, generator=gen, dtype=torch.float64)
    (_act(F.instance_norm(x, eps=1e-5), act, slope) * dy).sum().backward()
    mean, rstd = R.in_stats(x.detach())
    _close(R.in_bwd(x.detach(), mean, rstd, dy, act, slope), x.grad)
    ca, cb = R.in_bwd_coef(x.detach(), mean, rstd, dy, act, slope)
    xh = F.instance_norm(x.detach(), eps=1e-5).requires_grad_(True)
    g = torch.autograd.grad(_act(xh, act, slope), xh, dy)[0]     # the activation's own backward
    _close(ca, g.mean(dim=(2, 3, 4)))
    _close(cb, (g * xh.detach()).mean(dim=(2, 3, 4)))


def test_fuse_modes():
    gen = torch.Generator().manual_seed(5)
    xs = [torch.randn(2, 4, 2, 4, 6, generator=gen, dtype=torch.float64) for _ in range(3)]
    wts = torch.rand(2, 3, generator=gen, dtype=torch.float64) + 0.3
    _close(R.fuse(xs, wconst=1.0 / 3), torch.stack(xs).mean(dim=0))
    _close(R.fuse(xs, wts=wts), sum(wts[:, m].view(2, 1, 1, 1, 1) * xs[m] for m in range(3)))
    stats = [R.in_stats(x) for x in xs]
    _close(R.fuse(xs, wconst=1.0, stats=stats), sum(torch.relu(F.instance_norm(x, eps=1e-5)) for x in xs))
    # the materialised activation is rounded through the storage dtype before the sum
    yq = [torch.relu(F.instance_norm(x, eps=1e-5)).to(torch.bfloat16).double() for x in xs]
    _close(R.fuse(xs, wconst=0.5, stats=stats, dtype=torch.bfloat16), 0.5 * sum(yq))


@pytest.mark.parametrize("M", [2, 3])
def test_attention_fusion_wiring(M):
    """fused = sum_m softmax(MLP(avgpool(cat y_m)))[m] * y_m with y_m = relu(IN(x_m)): the backward the engine
    assembles -- dy_m = w[n, m] * dfused + dpooled[n, m*C + c] / V through gather_dy (alpha = w[:, m], beta = the
    modality's C columns of dpooled / V), then in_bwd -- equals autograd's y_m.grad and x_m.grad."""
    N, C, D, H, W = 2, 8, 4, 4, 6
    V, Hd = D * H * W, M * C // 4
    gen = torch.Generator().manual_seed(40 + M)
    xs = [(torch.randn(N, C, D, H, W, generator=gen, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
          for _ in range(M)]
    W1 = torch.randn(Hd, M * C, generator=gen, dtype=torch.float64, requires_grad=True)
    b1 = torch.randn(Hd, generator=gen, dtype=torch.float64, requires_grad=True)
    W2 = torch.randn(M, Hd, generator=gen, dtype=torch.float64, requires_grad=True)
    b2 = torch.randn(M, generator=gen, dtype=torch.float64, requires_grad=True)
    dfused = torch.randn(N, C, D, H, W, generator=gen, dtype=torch.float64)
    ys = [torch.relu(F.instance_norm(x, eps=1e-5)) for x in xs]
    for y in ys:
        y.retain_grad()
    # the reference's CrossModalAttention: cat on the channel axis, AdaptiveAvgPool3d(1), view(B, M*C)
    pooled = F.adaptive_avg_pool3d(torch.cat(ys, dim=1), 1).view(N, M * C)
    pooled.retain_grad()
    h, w = R.gate(pooled, W1, b1, W2, b2)
    assert (h > 0).any() and (h == 0).any()
    fused = R.fuse(ys, wts=w)
    _close(fused.detach(), sum(w[:, m].view(N, 1, 1, 1, 1) * ys[m] for m in range(M)).detach())
    (fused * dfused).sum().backward()
    for m in range(M):
        dy = R.gather_dy(dfused, 1.0, w.detach()[:, m], pooled.grad[:, m * C:(m + 1) * C] / V, None, None)
        _close(dy, ys[m].grad)
        mean, rstd = R.in_stats(xs[m].detach())
        _close(R.in_bwd(xs[m].detach(), mean, rstd, dy, 1, 0.0), xs[m].grad)


def test_gather_dy_routes_like_max_pool3d_backward():
    N, C, D, H, W = 2, 3, 4, 6, 8
    gen = torch.Generator().manual_seed(9)
    y = torch.randn(N, C, D, H, W, generator=gen, dtype=torch.float64).requires_grad_(True)   # no ties
    p, ind = F.max_pool3d(y, 2, return_indices=True)
    assert p.numel() * 8 == y.numel() and torch.unique(y.detach()).numel() == y.numel()
    dp = torch.randn(p.shape, generator=gen, dtype=torch.float64)
    (p * dp).sum().backward()
    codes = R.codes_from_indices(ind, H, W)
    assert codes.min() >= 0 and codes.max() <= 7
    _close(R.gather_dy(None, 1.0, None, None, dp, codes), y.grad)
    # with every other source too, and p1 shared by groups of samples
    p1 = torch.randn(1, C, D, H, W, generator=gen, dtype=torch.float64)
    alpha = torch.rand(N, generator=gen, dtype=torch.float64)
    beta = torch.randn(N, C, generator=gen, dtype=torch.float64)
    want = 0.5 * alpha.view(N, 1, 1, 1, 1) * p1 + beta.view(N, C, 1, 1, 1) + y.grad
    _close(R.gather_dy(p1, 0.5, alpha, beta, dp, codes, p1_nmod=1), want)
