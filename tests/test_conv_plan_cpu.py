"""Which kernel every 3^3 conv launch takes, checked without a GPU.

The library decides the kernel of a conv forward / data gradient in choose_gemm (csrc/conv_gemm.hip) and of a weight
gradient in choose_conv3_wgrad (csrc/conv_wgrad.hip); the planning queries and the name queries mmseg_conv3_kernel /
mmseg_conv3_wgrad_kernel are thin wrappers over them.  This file sweeps the queries for consistency and pins the
kernel and split count of the workloads' layers, so a routing change shows up here rather than rounds later as a
drift of a held-out metric ("The round-5 drift, named")."""
import hashlib
import itertools

import pytest

import mmseg_amd  # noqa: F401
from mmseg_amd import _lib

F32, BF16 = 0, 1
NORM, INPART, FP8, GROUPS, PAD16 = 1, 2, 4, 8, 16     # the name queries' flags
WS_CAP = 16 << 20                                      # the engine's weight-gradient workspace (floats)

CUBES = [(s, s, s) for s in (4, 6, 8, 12, 16, 24, 32, 48, 96)]
VOLUMES = CUBES + [(4, 8, 16), (12, 8, 24), (8, 16, 8), (28, 24, 64), (16, 8, 24)]
CHANNELS = (32, 48, 64, 96, 128, 256, 512)
KNOB_SETS = ({}, {"MMSEG_BRICK2_MINUNITS": "0", "MMSEG_BRICK4_BLOCKS": "3", "MMSEG_GROUP_FORCE_R": "0"})


def pow2(c):
    return 1 << (c - 1).bit_length()


def col_tile(n):
    return -(-n // (64 if n >= 64 else 32)) * (64 if n >= 64 else 32)


def conv_shape(N, vol, cin, cout):
    """(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo) of a cin -> cout conv on power-of-two padded pitches, as
    engine/layers.py Conv3 passes it; the data gradient is conv_shape(N, vol, cout, cin)."""
    D, H, W = vol
    cip = pow2(cin)
    return (N * D * H * W, cout, col_tile(cout), 27 * cip // 8, (cip // 8).bit_length() - 1, D, H, W, cip, pow2(cout))


def wgrad_shape(N, vol, cin, cout):
    """(V, Co, Cip, Ci, cpg_shift, D, H, W, lddy, ldx) of the same conv's weight gradient."""
    D, H, W = vol
    cip = pow2(cin)
    return (N * D * H * W, cout, cip, cin, (cip // 8).bit_length() - 1, D, H, W, pow2(cout), cip)


def fwd_name(L, shape, code, flags=0, ksplit=1, cin_real=0):
    return L.mmseg_conv3_kernel(*shape, cin_real, ksplit, flags, code).decode()


def wgrad_name(L, shape, code, flags=0, ws=WS_CAP):
    return L.mmseg_conv3_wgrad_kernel(*shape, ws, flags, code).decode()


def sweep_queries(L):
    """Every planning query that exists on both sides of the refactor, over the sweep: one tuple per shape."""
    out = []
    for N, vol, cin, cout, code in itertools.product((1, 2, 4), VOLUMES, CHANNELS, CHANNELS, (F32, BF16)):
        f, w = conv_shape(N, vol, cin, cout), wgrad_shape(N, vol, cin, cout)
        out.append((N, vol, cin, cout, code,
                    L.mmseg_conv3_splits(*f, code), L.mmseg_conv3_group_ok(*f, code),
                    L.mmseg_conv3_group_splits(*f, code), L.mmseg_conv3_norm_ok(*f, code),
                    L.mmseg_conv3_fp8_ok(*f), L.mmseg_conv3_dgrad_in_chunks(*f, code),
                    L.mmseg_conv3_wgrad_ws_floats(*w, code), L.mmseg_conv3_wgrad_norm_ok(*w, code),
                    L.mmseg_conv3_wgrad_group_ok(*w, code), L.mmseg_conv3_wgrad_group_ws_floats(*w, 2, code)))
    return out


def sweep_hash(rows):
    return hashlib.sha256(repr(rows).encode()).hexdigest()


@pytest.mark.parametrize("knobs", KNOB_SETS, ids=("default", "knobs"))
def test_queries_agree_with_the_kernel_names(knobs, monkeypatch):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    L = _lib.lib()
    rows = sweep_queries(L)
    assert len(rows) == 3 * len(VOLUMES) * len(CHANNELS) ** 2 * 2
    norm_capable = ("wgrad_row_kernel<CO32,NORM>", "wgrad_brick2_kernel<CO64,V3>", "wgrad_brick2_kernel<CO32,V3>")
    for (N, vol, cin, cout, code, ks, grp_ok, grp_ks, norm_ok, fp8_ok, in_chunks, ws, wnorm_ok, wgrp_ok,
         wgrp_ws) in rows:
        f, w, at = conv_shape(N, vol, cin, cout), wgrad_shape(N, vol, cin, cout), (N, vol, cin, cout, code)
        assert ks >= 1 and grp_ks >= 1 and ws >= 0 and wgrp_ws >= 0 and in_chunks >= 0, at
        assert {grp_ok, norm_ok, fp8_ok, wnorm_ok, wgrp_ok} <= {0, 1}, at
        assert bool(norm_ok) == fwd_name(L, f, code, NORM).startswith("conv3_brick6_kernel"), at
        # (mmseg_conv3_fp8_ok takes no dtype: the e4m3 forward is a bf16 launch)
        assert bool(fp8_ok) == fwd_name(L, f, BF16, FP8).startswith("conv3_brick6_kernel"), at
        assert (in_chunks > 0) == (fwd_name(L, f, code, INPART) == "conv3_brick6_kernel<BN32,INP>"), at
        if grp_ok:
            assert fwd_name(L, f, code, GROUPS, ksplit=grp_ks).startswith("conv3_brickr_kernel"), at
        if wnorm_ok:
            assert wgrad_name(L, w, code, NORM) in norm_capable, at
        if wgrp_ok:
            assert wgrad_name(L, w, code, GROUPS).startswith("wgrad_brickr_kernel"), at
        # every name is one of the families the launchers note
        for name in (fwd_name(L, f, code, 0, ks), wgrad_name(L, w, code)):
            assert name.split("<")[0].split("_kernel")[0] in FAMILIES, (at, name)


FAMILIES = {"conv3_brickr", "conv3_brick8", "conv3_brick2", "conv3_brick6", "conv3_brick4", "conv3_brick3",
            "conv3_brick", "conv_gemm", "wgrad_brickr", "wgrad_row", "wgrad_dma", "wgrad_brick2", "wgrad_brick",
            "wgrad"}


# ---------------------------------------------------------------- the workloads' layers, pinned
def layer_plan(L, N, vol, ci, co, cip=None, cop=None, code=BF16, grouped=False, flags=0):
    """(forward kernel, splits, data-gradient kernel, splits, weight-gradient kernel, splits) of one 3^3 conv as
    engine/layers.py (Conv3 / GroupedConv3) asks for it: channels ci -> co stored at pitches cip / cop, the channel
    padding skipped on the K side (cin_real), the weight gradient over cop rows when co is no multiple of 32
    (flag 16 when 16 of them are padding).  Weight-gradient splits 0: the kernel writes the gradient itself.
    flags: the deferred-norm forward / weight gradient (1) and the data gradient with IN-backward partials (2)."""
    D, H, W = vol
    cip, cop = cip or ci, cop or co
    M = N * D * H * W
    shift = lambda c: (c // 8).bit_length() - 1   # noqa: E731
    g = GROUPS if grouped else 0
    splits = L.mmseg_conv3_group_splits if grouped else L.mmseg_conv3_splits
    f = (M, co, col_tile(co), 27 * cip // 8, shift(cip), D, H, W, cip, cop)
    d = (M, ci, col_tile(ci), 27 * cop // 8, shift(cop), D, H, W, cop, cip)
    fks = 1 if flags & NORM else splits(*f, code)
    dks = 1 if flags & INPART else splits(*d, code)
    rows = cop if co % 32 and cop % 32 == 0 else co
    w = (M, rows, cip, ci, shift(cip), D, H, W, cop, cip)
    wflags = g | (flags & NORM) | (PAD16 if rows - co == 16 else 0)
    ws = (L.mmseg_conv3_wgrad_group_ws_floats(*w, 2, code) if grouped else L.mmseg_conv3_wgrad_ws_floats(*w, code))
    return (fwd_name(L, f, code, g | (flags & NORM), fks, ci if cip > ci else 0), fks,
            fwd_name(L, d, code, g | (flags & INPART), dks, co if cop > co else 0), dks,
            wgrad_name(L, w, code, wflags, ws), ws // (rows * 27 * cip + rows))


# ((N, cube side, Cin, Cout), layer_plan keywords, expected layer_plan).  bf16 unless code = 0.  The kernel names of
# the plain-conv rows were read from launches of the library before choose_gemm / choose_conv3_wgrad existed
# (tools/convbench.py --only fwd,fwdn,dgrad,dgradin,wgrad,wgradn prints the launched kernel per shape and op); the
# grouped rows and SwinUNETR's (feature_size 48, 128^3, B = 1, channels 48 / 96 / 192 / 384 / 768 at pitches 64 / 128
# / 256 / 512 / 1024 as engine/swin.py builds them) against the families of that library's per-launch timer dumps.
PINNED = [
    # DualEncoder / UNet3D at 96^3, B = 2 (c2, c3, c5): encoder and decoder levels
    ((2, 96, 32, 32), {},
     ('conv3_brick6_kernel<BN32>', 1, 'conv3_brick6_kernel<BN32>', 1, 'wgrad_row_kernel<CO32>', 256)),
    ((2, 96, 64, 32), {},
     ('conv3_brick8_kernel<BN32>', 1, 'conv3_brick2_kernel<BN64,ZW1>', 1, 'wgrad_row_kernel<CO32>', 128)),
    ((2, 48, 32, 64), {},
     ('conv3_brick2_kernel<BN64,ZW1>', 1, 'conv3_brick3_kernel<BN32>', 1, 'wgrad_dma_kernel<CO64>', 247)),
    ((2, 48, 64, 64), {},
     ('conv3_brick8_kernel<BN64>', 1, 'conv3_brick8_kernel<BN64>', 1, 'wgrad_dma_kernel<CO64>', 124)),
    ((2, 48, 128, 64), {},
     ('conv3_brick8_kernel<BN64>', 1, 'conv3_brick2_kernel<BN64,ZW1>', 1, 'wgrad_dma_kernel<CO64>', 64)),
    ((2, 24, 64, 128), {},
     ('conv3_brick3_kernel<BN32>', 1, 'conv3_brickr_kernel<BN32>', 2, 'wgrad_dma_kernel<CO64>', 54)),
    ((2, 24, 128, 128), {},
     ('conv3_brick3_kernel<BN32>', 1, 'conv3_brick3_kernel<BN32>', 1, 'wgrad_dma_kernel<CO64>', 31)),
    ((2, 24, 256, 128), {},
     ('conv3_brick3_kernel<BN32>', 1, 'conv3_brick3_kernel<BN32>', 1, 'wgrad_dma_kernel<CO64>', 16)),
    ((2, 12, 128, 256), {},
     ('conv3_brickr_kernel<BN32,KW2>', 2, 'conv3_brickr_kernel<BN32,KW2>', 4, 'wgrad_brickr_kernel<CO64,V3>', 8)),
    ((2, 12, 256, 256), {},
     ('conv3_brickr_kernel<BN32,KW2>', 2, 'conv3_brickr_kernel<BN32,KW2>', 2, 'wgrad_brickr_kernel<CO64,V3>', 8)),
    ((2, 12, 512, 256), {},
     ('conv3_brickr_kernel<BN32,KW2>', 2, 'conv3_brickr_kernel<BN32,KW2>', 1, 'wgrad_brickr_kernel<CO64,V3>', 4)),
    ((2, 6, 256, 512), {},
     ('conv3_brickr_kernel<BN32>', 8, 'conv3_brickr_kernel<BN32>', 16, 'wgrad_brickr_kernel<CO64,V3>', 0)),
    ((2, 6, 512, 512), {},
     ('conv3_brickr_kernel<BN32,KW2>', 8, 'conv3_brickr_kernel<BN32,KW2>', 8, 'wgrad_brickr_kernel<CO64,V3>', 0)),
    ((4, 24, 64, 128), {'grouped': True},
     ('conv3_brickr_kernel<BN64>', 1, 'conv3_brickr_kernel<BN32>', 1, 'wgrad_brickr_kernel<CO64,B448>', 62)),
    ((4, 24, 128, 128), {'grouped': True},
     ('conv3_brickr_kernel<BN64>', 1, 'conv3_brickr_kernel<BN64>', 1, 'wgrad_brickr_kernel<CO64,B448>', 30)),
    ((4, 24, 256, 128), {'grouped': True},
     ('conv3_brickr_kernel<BN64>', 1, 'conv3_brickr_kernel<BN64>', 1, 'wgrad_brickr_kernel<CO64,B448>', 16)),
    ((4, 12, 128, 256), {'grouped': True},
     ('conv3_brickr_kernel<BN32,KW2>', 1, 'conv3_brickr_kernel<BN32,KW2>', 2, 'wgrad_brickr_kernel<CO64,V3>', 16)),
    ((4, 12, 256, 256), {'grouped': True},
     ('conv3_brickr_kernel<BN32,KW2>', 1, 'conv3_brickr_kernel<BN32,KW2>', 1, 'wgrad_brickr_kernel<CO64,V3>', 8)),
    ((4, 12, 512, 256), {'grouped': True},
     ('conv3_brickr_kernel<BN32,KW2>', 1, 'conv3_brickr_kernel<BN64>', 1, 'wgrad_brickr_kernel<CO64,V3>', 4)),
    ((4, 6, 256, 512), {'grouped': True},
     ('conv3_brickr_kernel<BN32,KW2>', 4, 'conv3_brickr_kernel<BN32,KW2>', 8, 'wgrad_brickr_kernel<CO64,V3>', 0)),
    ((4, 6, 512, 512), {'grouped': True},
     ('conv3_brickr_kernel<BN32,KW2>', 4, 'conv3_brickr_kernel<BN32,KW2>', 4, 'wgrad_brickr_kernel<CO64,V3>', 0)),
    ((2, 96, 32, 32), {'flags': 3},
     ('conv3_brick6_kernel<BN32>', 1, 'conv3_brick6_kernel<BN32,INP>', 1, 'wgrad_row_kernel<CO32,NORM>', 256)),
    ((1, 64, 32, 32), {'code': 0},
     ('conv3_brick2_kernel<BN32,ZW1>', 1, 'conv3_brick2_kernel<BN32,ZW1>', 1, 'wgrad_brick_kernel', 512)),
    ((1, 32, 32, 64), {'code': 0},
     ('conv3_brick2_kernel<BN32,ZW1>', 1, 'conv3_brick2_kernel<BN32,ZW1>', 1, 'wgrad_brick_kernel', 256)),
    ((1, 32, 64, 64), {'code': 0},
     ('conv3_brick2_kernel<BN32,ZW1>', 1, 'conv3_brick2_kernel<BN32,ZW1>', 1, 'wgrad_brick_kernel', 128)),
    ((1, 16, 64, 128), {'code': 0},
     ('conv3_brickr_kernel<BN32>', 2, 'conv3_brickr_kernel<BN32>', 4, 'wgrad_brick_kernel', 32)),
    ((1, 16, 128, 128), {'code': 0},
     ('conv3_brickr_kernel<BN32>', 4, 'conv3_brickr_kernel<BN32>', 4, 'wgrad_brick_kernel', 32)),
    ((1, 8, 128, 256), {'code': 0},
     ('conv3_brickr_kernel<BN32>', 4, 'conv3_brickr_kernel<BN32>', 8, 'wgrad_brick_kernel', 4)),
    ((1, 8, 256, 256), {'code': 0},
     ('conv3_brickr_kernel<BN32>', 8, 'conv3_brickr_kernel<BN32>', 8, 'wgrad_brick_kernel', 4)),
    ((1, 4, 256, 512), {'code': 0},
     ('conv3_brickr_kernel<BN32>', 8, 'conv3_brickr_kernel<BN32>', 16, 'wgrad_kernel<conv3>', 1)),
    ((1, 4, 512, 512), {'code': 0},
     ('conv3_brickr_kernel<BN32>', 16, 'conv3_brickr_kernel<BN32>', 16, 'wgrad_kernel<conv3>', 1)),
    ((1, 8, 512, 256), {'code': 0},
     ('conv3_brickr_kernel<BN32>', 16, 'conv3_brickr_kernel<BN32>', 8, 'wgrad_brick_kernel', 4)),
    ((1, 16, 256, 128), {'code': 0},
     ('conv3_brickr_kernel<BN32>', 4, 'conv3_brickr_kernel<BN32>', 2, 'wgrad_brick_kernel', 16)),
    ((1, 32, 128, 64), {'code': 0},
     ('conv3_brick2_kernel<BN32,ZW1>', 1, 'conv3_brick2_kernel<BN32,ZW1>', 1, 'wgrad_brick_kernel', 64)),
    ((1, 64, 64, 32), {'code': 0},
     ('conv3_brick2_kernel<BN32,ZW1>', 1, 'conv3_brick2_kernel<BN64,ZW1>', 1, 'wgrad_brick_kernel', 293)),
    ((1, 128, 48, 48), {'cip': 64, 'cop': 64},
     ('conv3_brick2_kernel<BN48,ZW1>', 1, 'conv3_brick2_kernel<BN48,ZW1>', 1, 'wgrad_dma_kernel<CO64>', 128)),
    ((1, 64, 48, 48), {'cip': 64, 'cop': 64},
     ('conv3_brick2_kernel<BN48,ZW1>', 1, 'conv3_brick2_kernel<BN48,ZW1>', 1, 'wgrad_dma_kernel<CO64>', 128)),
    ((1, 32, 96, 96), {'cip': 128, 'cop': 128},
     ('conv3_brick2_kernel<BN48,ZW1>', 1, 'conv3_brick2_kernel<BN48,ZW1>', 1, 'wgrad_dma_kernel<CO32>', 26)),
    ((1, 16, 192, 192), {'cip': 256, 'cop': 256},
     ('conv3_brickr_kernel<BN32>', 3, 'conv3_brickr_kernel<BN32>', 3, 'wgrad_dma_kernel<CO64>', 11)),
    ((1, 4, 768, 768), {'cip': 1024, 'cop': 1024},
     ('conv3_brickr_kernel<BN32>', 11, 'conv3_brickr_kernel<BN32>', 11, 'wgrad_brickr_kernel<CO64>', 0)),
    ((1, 8, 768, 384), {'cip': 1024, 'cop': 512},
     ('conv3_brickr_kernel<BN32>', 11, 'conv3_brickr_kernel<BN32>', 6, 'wgrad_dma_kernel<CO64>', 0)),
    ((1, 8, 384, 384), {'cip': 512, 'cop': 512},
     ('conv3_brickr_kernel<BN32>', 8, 'conv3_brickr_kernel<BN32>', 8, 'wgrad_dma_kernel<CO64>', 2)),
    ((1, 16, 384, 192), {'cip': 512, 'cop': 256},
     ('conv3_brickr_kernel<BN32>', 3, 'conv3_brickr_kernel<BN32>', 2, 'wgrad_dma_kernel<CO64>', 6)),
    ((1, 32, 192, 96), {'cip': 256, 'cop': 128},
     ('conv3_brick2_kernel<BN48,ZW1>', 1, 'conv3_brick3_kernel<BN32>', 1, 'wgrad_dma_kernel<CO32>', 14)),
    ((1, 64, 96, 48), {'cip': 128, 'cop': 64},
     ('conv3_brick2_kernel<BN48,ZW1>', 1, 'conv3_brick2_kernel<BN48,ZW1>', 1, 'wgrad_dma_kernel<CO64>', 74)),
    ((1, 128, 96, 48), {'cip': 128, 'cop': 64},
     ('conv3_brick2_kernel<BN48,ZW1>', 1, 'conv3_brick2_kernel<BN48,ZW1>', 1, 'wgrad_dma_kernel<CO64>', 75)),
]


def test_workload_layers_take_the_pinned_kernels(monkeypatch):
    for knobs in KNOB_SETS[1:]:
        for k in knobs:
            monkeypatch.delenv(k, raising=False)
    L = _lib.lib()
    got = [(key, kw, layer_plan(L, key[0], (key[1],) * 3, key[2], key[3], **kw)) for key, kw, _ in PINNED]
    wrong = [(g, want) for g, (_, _, want) in zip(got, PINNED) if g[2] != want]
    assert not wrong, wrong
