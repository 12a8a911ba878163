"""The rows of tests/conv_fused_cases.py provably take the kernels they are for, checked without a GPU: for every row
the planning queries (tests/test_conv_plan_cpu.py describes them) must name the kernel, the split count and the
chunk count the table carries, under the row's knobs.  tests/test_conv_fused_gpu.py and test_conv3_kernel_variants
(tests/test_kernels_gpu.py) assert the launched kernel against the same table."""
import pytest

import mmseg_amd  # noqa: F401
from mmseg_amd import _lib
from tests import conv_fused_cases as C
from tests.test_conv_plan_cpu import (BF16, F32, GROUPS, INPART, NORM, conv_shape, fwd_name, wgrad_name,
                                      wgrad_shape)


@pytest.fixture(autouse=True)
def _clean_knobs(monkeypatch):
    for k in C.KNOBS + ("MMSEG_BRICK2_MINBLK", "MMSEG_BRICK3_BLOCKS", "MMSEG_BRICK8_MINBLK"):
        monkeypatch.delenv(k, raising=False)


def _set(monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("row", C.NORM_ROWS, ids=str)
def test_norm_rows_take_brick6(row, monkeypatch):
    N, vol, cin, cout, blocks, plain = row
    _set(monkeypatch, C.knobs_of(blocks))
    L, f = _lib.lib(), conv_shape(N, vol, cin, cout)
    assert L.mmseg_conv3_norm_ok(*f, BF16) == 1
    assert fwd_name(L, f, BF16, NORM) == C.BRICK6
    assert L.mmseg_conv3_splits(*f, BF16) == 1 and fwd_name(L, f, BF16) == plain
    # the fused forms are bf16-only
    assert L.mmseg_conv3_norm_ok(*f, F32) == 0 and not fwd_name(L, f, F32, NORM).startswith("conv3_brick6")


@pytest.mark.parametrize("row", C.NORM_REFUSED, ids=str)
def test_norm_refused(row, monkeypatch):
    N, vol, cin, cout, blocks = row
    _set(monkeypatch, C.knobs_of(blocks))
    L, f = _lib.lib(), conv_shape(N, vol, cin, cout)
    assert L.mmseg_conv3_norm_ok(*f, BF16) == 0 and not fwd_name(L, f, BF16, NORM).startswith("conv3_brick6")


@pytest.mark.parametrize("row", C.INP_ROWS, ids=str)
def test_inp_rows_take_brick6_inp(row, monkeypatch):
    N, vol, cin, cout, blocks, chunks = row
    _set(monkeypatch, C.knobs_of(blocks))
    L, d = _lib.lib(), conv_shape(N, vol, cout, cin)
    assert L.mmseg_conv3_splits(*d, BF16) == 1
    assert L.mmseg_conv3_dgrad_in_chunks(*d, BF16) == chunks
    assert fwd_name(L, d, BF16, INPART) == C.BRICK6_INP
    assert fwd_name(L, d, BF16) == C.BRICK6          # the plain data gradient the bitwise comparison runs
    assert L.mmseg_conv3_dgrad_in_chunks(*d, F32) == 0 and fwd_name(L, d, F32, INPART) != C.BRICK6_INP
    # the deferred norm needs one input chunk: the 64 -> 32 rows have the partials without it
    assert L.mmseg_conv3_norm_ok(*conv_shape(N, vol, cin, cout), BF16) == (1 if cin == 32 else 0)


@pytest.mark.parametrize("row", C.INP_REFUSED, ids=str)
def test_inp_refused(row, monkeypatch):
    N, vol, cin, cout, name = row
    _set(monkeypatch, C.BASE_KNOBS)
    L, d = _lib.lib(), conv_shape(N, vol, cout, cin)
    assert L.mmseg_conv3_dgrad_in_chunks(*d, BF16) == 0
    assert fwd_name(L, d, BF16, INPART) == fwd_name(L, d, BF16) == name


@pytest.mark.parametrize("row", C.GROUP_ROWS, ids=str)
def test_group_rows(row, monkeypatch):
    G, N, vol, cin, cout, knobs, fname, fks, dname, dks, wname, wsplits = row
    _set(monkeypatch, knobs)
    L = _lib.lib()
    f, d, w = conv_shape(N, vol, cin, cout), conv_shape(N, vol, cout, cin), wgrad_shape(N, vol, cin, cout)
    assert L.mmseg_conv3_group_ok(*f, BF16) == 1 and L.mmseg_conv3_group_ok(*d, BF16) == 1
    assert L.mmseg_conv3_wgrad_group_ok(*w, BF16) == 1
    assert L.mmseg_conv3_group_splits(*f, BF16) == fks and fwd_name(L, f, BF16, GROUPS, fks) == fname
    assert L.mmseg_conv3_group_splits(*d, BF16) == dks and fwd_name(L, d, BF16, GROUPS, dks) == dname
    ws = L.mmseg_conv3_wgrad_group_ws_floats(*w, G, BF16)
    assert wgrad_name(L, w, BF16, GROUPS, ws) == wname
    assert ws == wsplits * (cout * 27 * cin + cout) and wsplits % G == 0
    # fp32 has no grouped weight gradient, so ConvGroup.ok is False there.  (ConvGroup itself needs a device for its
    # Runtime and weight images; without one this asserts the query ConvGroup.ok returns False on.)
    assert L.mmseg_conv3_wgrad_group_ok(*w, F32) == 0


def test_stem_rows():
    L = _lib.lib()
    for cr, co, (N, D, H, W) in C.STEM_ROWS + [C.STEM_DIRECT[:3]]:
        assert L.mmseg_stem_ok(cr, co, D, H, W, 8, co) == 1, (cr, co, D, H, W)
    cr, co, (N, D, H, W), ks = C.STEM_DIRECT
    assert L.mmseg_stem_wgrad_splits(N, D, H, W, 2) == ks == 2      # 3 bricks: 2 + 1


@pytest.mark.parametrize("code", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(C.VARIANTS)))
def test_kernel_variant_rows(i, code, monkeypatch):
    """test_conv3_kernel_variants' rows: the forward / data-gradient / weight-gradient kernels Conv3 launches."""
    knobs, cin, cout, shape, names = C.VARIANTS[i]
    _set(monkeypatch, dict(C.BASE_KNOBS, **knobs))
    L, N, vol = _lib.lib(), shape[0], shape[1:]
    f, d, w = conv_shape(N, vol, cin, cout), conv_shape(N, vol, cout, cin), wgrad_shape(N, vol, cin, cout)
    got = (fwd_name(L, f, code, 0, L.mmseg_conv3_splits(*f, code)),
           fwd_name(L, d, code, 0, L.mmseg_conv3_splits(*d, code)),
           wgrad_name(L, w, code, 0, L.mmseg_conv3_wgrad_ws_floats(*w, code)))
    assert got == names[code]
