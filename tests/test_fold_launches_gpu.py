"""Launch folding that must not move a bit: the fused fusion + max-pool pass (mmseg_fuse_pool_fwd) against the
separate fusion and max-pool kernels, and a whole DualEncoder training step with the pass on and off
(MMSEG_FUSE_POOL)."""
import ctypes

import pytest
import torch

import mmseg_amd  # noqa: F401
from mmseg_amd._lib import lib, ptr, stream_handle
from mmseg_amd.models.build import build_model
from mmseg_amd.trainer.trainer import Trainer

pytestmark = pytest.mark.gpu


def _bits(t):
    """The tensor's storage as integers: equality of these is bitwise (-0.0 != +0.0, NaN == NaN)."""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[ptr(t) for t in ts])


def _ints(vs):
    return (ctypes.c_int * len(vs))(*vs)


NEG_WIN = (0, 0, 0)       # pooled voxel whose whole window is negative after the norm (zero as stored, NORM off)
DUP_WIN = (1, 2, 1)       # pooled voxel with the same maximum at window positions 3 and 5
DUP_POS = (3, 5)


def _sources(dev, dtype, norm, M, N, C, D, H, W, ld):
    """M sources [N*V][ld] (row padding filled too), statistics [N][C] per source when `norm`."""
    gen = torch.Generator(device="cpu").manual_seed(1000 * M + 10 * C + D + int(norm))
    srcs, means, rstds = [], [], []
    for m in range(M):
        x = torch.randn(N, D, H, W, ld, generator=gen) * 2 + 0.3
        mu = torch.randn(N, C, generator=gen) * 0.5
        rs = torch.rand(N, C, generator=gen) + 0.5
        for n in range(N):
            z, y, xx = (2 * v for v in NEG_WIN)
            # NORM: far below every mean, so relu((x - mean) * rstd) is 0 in the whole window; as stored: exact zeros
            x[n, z:z + 2, y:y + 2, xx:xx + 2, :] = (-50.0 - torch.rand(2, 2, 2, ld, generator=gen)) if norm else 0.0
            z, y, xx = (2 * v for v in DUP_WIN)
            for t in DUP_POS:
                x[n, z + (t >> 2), y + ((t >> 1) & 1), xx + (t & 1), :] = 40.0
        srcs.append(x.to(dtype).reshape(N * D * H * W, ld).contiguous().to(dev))
        means.append(mu.to(dev))
        rstds.append(rs.to(dev))
    return srcs, means, rstds


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("shape", [(4, 6, 8), (8, 8, 8), (12, 12, 12)])
@pytest.mark.parametrize("C", [8, 24, 32])
@pytest.mark.parametrize("M", [2, 3])
def test_fuse_pool_bitwise(dev, dtype, norm, shape, C, M):
    """The fused tensor (in a concat slot: ldo = 2C), every source's pooled tensor and argmax codes equal the
    separate fusion and max-pool kernels' bit for bit, with source rows wider than C, a window of all-zero ties
    (code 0 wins) and a window with duplicate maxima (the first position wins)."""
    N = 2
    D, H, W = shape
    V, Vo = D * H * W, D * H * W // 8
    ld, ldo, ldy = C + 8, 2 * C, C + 8
    L, s, code = lib(), stream_handle(), (0 if dtype == torch.float32 else 1)
    srcs, means, rstds = _sources(dev, dtype, norm, M, N, C, D, H, W, ld)
    wconst = 1.0 / M
    res = []
    for fused in (False, True):
        out = torch.full((N * V, ldo), 7.0, dtype=dtype, device=dev)
        ys = [torch.full((N * Vo, ldy), 9.0, dtype=dtype, device=dev) for _ in range(M)]
        idxs = [torch.full((N * Vo * C,), 77, dtype=torch.uint8, device=dev) for _ in range(M)]
        slot = out.data_ptr() + C * out.element_size()      # the skip half of the decoder's concat rows
        if fused:
            L.mmseg_fuse_pool_fwd(_ptrs(srcs), _ints([ld] * M), _ptrs(means) if norm else None,
                                  _ptrs(rstds) if norm else None, M, wconst, slot, ldo, _ptrs(ys), _ints([ldy] * M),
                                  _ptrs(idxs), N, D, H, W, C, code, s)
        elif norm:
            L.mmseg_fuse_norm_fwd(_ptrs(srcs), _ints([ld] * M), _ptrs(means), _ptrs(rstds), M, wconst, None, slot,
                                  ldo, N, V, C, code, s)
            for m in range(M):
                L.mmseg_maxpool2_norm_fwd(ptr(srcs[m]), ld, ptr(means[m]), ptr(rstds[m]), ptr(ys[m]), ldy,
                                          ptr(idxs[m]), N, D, H, W, C, code, s)
        else:
            L.mmseg_fuse_fwd(_ptrs(srcs), _ints([ld] * M), M, wconst, None, slot, ldo, N, V, C, code, s)
            for m in range(M):
                L.mmseg_maxpool2_fwd(ptr(srcs[m]), ld, ptr(ys[m]), ldy, ptr(idxs[m]), N, D, H, W, C, code, s)
        torch.cuda.synchronize()
        res.append((out, ys, idxs))
    (out0, ys0, idx0), (out1, ys1, idx1) = res
    assert torch.equal(_bits(out0), _bits(out1))
    for m in range(M):
        assert torch.equal(_bits(ys0[m]), _bits(ys1[m])), m
        assert torch.equal(idx0[m], idx1[m]), m
        codes = idx1[m].view(N, D // 2, H // 2, W // 2, C)
        assert (codes[(slice(None),) + NEG_WIN] == 0).all()
        assert (codes[(slice(None),) + DUP_WIN] == DUP_POS[0]).all()
        pooled = ys1[m].view(N, D // 2, H // 2, W // 2, ldy)[..., :C]
        assert (pooled[(slice(None),) + NEG_WIN] == 0).all()
    # neither kernel wrote outside its rows: the other half of the concat rows and the pooled rows' padding
    assert (out1[:, :C] == 7.0).all() and all((y[:, C:] == 9.0).all() for y in ys1)


def test_fuse_pool_rejects_odd_dims(dev):
    from mmseg_amd._lib import MmsegError
    L, s = lib(), stream_handle()
    t = torch.zeros(2 * 4 * 6 * 7 * 8, device=dev)
    i = torch.zeros(2 * 4 * 6 * 7 * 8, dtype=torch.uint8, device=dev)
    with pytest.raises(MmsegError):
        L.mmseg_fuse_pool_fwd(_ptrs([t, t]), _ints([8, 8]), None, None, 2, 0.5, ptr(t), 8, _ptrs([t, t]),
                              _ints([8, 8]), _ptrs([i, i]), 2, 4, 6, 7, 8, 0, s)


def _config(modalities, fusion, dtype):
    return {
        "experiment": {"name": "t", "output_dir": "/tmp/mmseg_test_out", "seed": 0},
        "data": {"modalities": list(modalities)},
        "model": {"name": "dual_encoder", "in_channels": len(modalities), "out_channels": 3,
                  "backbone": {"features": [8, 16, 32, 64, 128], "norm": "instance"},
                  "fusion": {"type": fusion}, "head": {"dropout": 0.0}},
        "training": {"epochs": 1, "batch_size": 2, "accumulation_steps": 1,
                     "optimizer": {"name": "adamw", "lr": 1e-3, "weight_decay": 1e-5, "betas": [0.9, 0.999]},
                     "scheduler": {"name": "none"},
                     "loss": {"name": "dice_ce", "dice_weight": 0.5, "ce_weight": 0.5, "class_weights": None},
                     "checkpoint": {"save_last": False, "save_best": False}},
        "hardware": {"device": "cuda", "mixed_precision": False, "engine_dtype": dtype},
    }


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
@pytest.mark.parametrize("modalities,fusion", [(("CT", "PET"), "cross_attention"), (("CT", "PET", "MRI"), "cross_attention"),
                                               (("CT", "PET"), "add")])
def test_whole_step_bitwise(dev, modalities, fusion, dtype, monkeypatch):
    """One train_step of a small DualEncoder (features 8..128, 32^3, B = 2; mean fusion with 2 and 3 modalities, add
    fusion) with MMSEG_FUSE_POOL off and on: the loss, every gradient and every updated parameter are equal."""
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(2, len(modalities), 32, 32, 32, generator=gen)
    y = torch.randint(0, 3, (2, 32, 32, 32), generator=gen)
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("MMSEG_FUSE_POOL", flag)
        cfg = _config(modalities, fusion, dtype)
        torch.manual_seed(0)
        m = build_model(cfg)
        tr = Trainer(cfg, m)
        grads = {}
        opt_step = tr.optimizer.step

        def step(*a, _m=m, _grads=grads, _step=opt_step, **kw):   # (train_step clears the gradients after the update)
            _grads.update({n: p.grad.detach().clone() for n, p in _m.named_parameters() if p.grad is not None})
            return _step(*a, **kw)
        tr.optimizer.step = step
        loss = tr.train_step({"image": x, "label": y}, 0)
        torch.cuda.synchronize()
        assert m.backbone.__dict__["_engine"].program.fuse_pool == (flag == "1")
        params = {n: p.detach().clone() for n, p in m.named_parameters()}
        res[flag] = (loss, grads, params)
    assert res["0"][0] == res["1"][0]
    assert res["0"][1] and set(res["0"][1]) == set(res["1"][1])
    for k in (1, 2):
        diff = [n for n in res["0"][k] if not torch.equal(_bits(res["0"][k][n]), _bits(res["1"][k][n]))]
        assert not diff, diff
