"""Plain torch fp64 restatement of the DualEncoder fusion path, the checker of the fusion / gate / norm-backward
kernel tests: the weighted modality sum (reference dual_encoder.py:184-195), the CrossModalAttention gate
(dual_encoder.py:207-254), the gathered dy of the InstanceNorm backward (fusion backward + MaxPool3d backward,
unet.py:73) and the closed-form InstanceNorm3d(affine=False) + activation backward (unet.py:34-35).
Tensors are NCDHW, statistics [N, C]; everything is computed in fp64 on the device of its inputs
(tests/test_fusion_ref_cpu.py checks the closed forms against torch autograd)."""
import torch


def _bc(s):
    """[N, C] -> [N, C, 1, 1, 1]"""
    return s.double()[:, :, None, None, None]


def fuse(srcs, wconst=None, wts=None, stats=None, dtype=torch.float64):
    """wconst * sum_m a_m, or sum_m wts[n, m] * a_m (wts [N, M]).  a_m is srcs[m] as stored or, with stats =
    [(mean_m, rstd_m)] per source, relu((x_m - mean_m) * rstd_m) rounded through the storage dtype."""
    out = None
    for m, x in enumerate(srcs):
        a = x.double()
        if stats is not None:
            mean, rstd = stats[m]
            a = torch.relu((a - _bc(mean)) * _bc(rstd)).to(dtype).double()
        if wts is not None:
            a = a * wts.double()[:, m][:, None, None, None, None]
        out = a if out is None else out + a
    return out if wts is not None else out * (1.0 if wconst is None else wconst)


def gate(pooled, W1, b1, W2, b2):
    """(h, w): h = relu(pooled W1^T + b1) [N, Hd], w = softmax_M(h W2^T + b2) [N, M].  pooled[n, m*C + c] is the
    per-channel mean of source m -- the layout cat(dim=1) + AdaptiveAvgPool3d + view(B, M*C) gives; W1 [Hd, M*C]
    with Hd = M*C // 4, W2 [M, Hd]."""
    h = torch.relu(pooled.double() @ W1.double().t() + b1.double())
    return h, torch.softmax(h @ W2.double().t() + b2.double(), dim=1)


def gather_dy(p1, scale1, alpha, beta, pool_dy, pool_idx, p1_nmod=0, shape=None):
    """dy[n] = scale1 * alpha[n] * p1[n] + beta[n][c] + maxpool_bwd(pool_dy, pool_idx)[n]; any of p1 / alpha / beta /
    pool_dy may be None.  pool_idx holds the window codes t = (z&1)<<2 | (y&1)<<1 | (x&1) of the pooled voxels'
    maxima; sample n reads p1[n % p1_nmod] when p1_nmod > 0.  shape = (N, C, D, H, W) when neither p1 nor pool_dy
    gives it."""
    if pool_dy is not None:
        N, C, Do, Ho, Wo = pool_dy.shape
        shape = (N, C, 2 * Do, 2 * Ho, 2 * Wo)
    elif p1 is not None and p1_nmod == 0:
        shape = tuple(p1.shape)
    ref = next(t for t in (p1, beta, pool_dy) if t is not None)
    dy = torch.zeros(shape, dtype=torch.float64, device=ref.device)
    if p1 is not None:
        p = p1.double()
        if p1_nmod > 0:
            p = p[torch.arange(shape[0], device=p.device) % p1_nmod]
        if alpha is not None:
            p = p * alpha.double()[:, None, None, None, None]
        dy = dy + scale1 * p
    if beta is not None:
        dy = dy + _bc(beta)
    if pool_dy is not None:
        for t in range(8):
            z, y, x = t >> 2, (t >> 1) & 1, t & 1
            dy[:, :, z::2, y::2, x::2] += (pool_idx == t).double() * pool_dy.double()
    return dy


def _g_xhat(x, mean, rstd, dy, act, slope):
    xhat = (x.double() - _bc(mean)) * _bc(rstd)
    if act == 0:
        g = dy.double()
    else:
        g = torch.where(xhat > 0, dy.double(), dy.double() * (slope if act == 2 else 0.0))
    return g, xhat


def in_bwd_coef(x, mean, rstd, dy, act=1, slope=0.0):
    """(mean_v g, mean_v g * xhat), each [N, C]: g = act'(xhat) * dy, act 0 none, 1 ReLU, 2 LeakyReLU(slope)."""
    g, xhat = _g_xhat(x, mean, rstd, dy, act, slope)
    return g.mean(dim=(2, 3, 4)), (g * xhat).mean(dim=(2, 3, 4))


def in_bwd(x, mean, rstd, dy, act=1, slope=0.0):
    """Input gradient of act(InstanceNorm(x)) (no affine, biased variance) for the output gradient dy:
    dx = rstd * (g - mean_v(g) - xhat * mean_v(g * xhat))."""
    g, xhat = _g_xhat(x, mean, rstd, dy, act, slope)
    ca, cb = in_bwd_coef(x, mean, rstd, dy, act, slope)
    return _bc(rstd) * (g - _bc(ca) - xhat * _bc(cb))


def in_stats(x, eps=1e-5):
    """(mean, rstd) [N, C] of nn.InstanceNorm3d: biased variance, rstd = 1 / sqrt(var + eps)."""
    xd = x.double()
    mean = xd.mean(dim=(2, 3, 4))
    var = xd.var(dim=(2, 3, 4), unbiased=False)
    return mean, 1.0 / torch.sqrt(var + eps)


def codes_from_indices(indices, H, W):
    """Window codes of F.max_pool3d(..., 2, return_indices=True)'s flat input indices (z * H * W + y * W + x)."""
    z, y, x = indices // (H * W), (indices // W) % H, indices % W
    return ((z & 1) << 2) | ((y & 1) << 1) | (x & 1)
