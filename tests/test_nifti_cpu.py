"""The NIfTI-1 reader / writer (utils/nifti.py, re-exported from utils/io.py) against the field layout of the
standard as tests/nifti_ref.py states it independently: the reader on struct-packed files, the writer by
unpacking what it wrote; and get_dataset over the reference's CSV lists, which needs no GPU until a sample is
fetched.  nibabel is absent, so parity with it is not pinned; its published rules (get_fdata scaling, affine
precedence) are what the cases spell out."""
import gzip
import itertools

import numpy as np
import pytest

import mmseg_amd  # noqa: F401
from mmseg_amd.data.dataloader import get_dataset
from mmseg_amd.utils.io import load_nifti, save_nifti
from tests import nifti_ref as NR

TYPES = sorted(NR.CODES)


def _values(code, shape, seed=0):
    """Seeded values of the type, its extremes included when there is room."""
    t = np.dtype(NR.CODES[code])
    rng = np.random.default_rng(seed + code)
    n = int(np.prod(shape))
    if t.kind == "f":
        v = (rng.standard_normal(n) * 1000).astype(t)
        ext = [np.finfo(t).max, -np.finfo(t).max, np.finfo(t).tiny, -0.0] if t == np.float32 else [1e30, -1e-300]
    else:
        info = np.iinfo(t)
        v = rng.integers(info.min, info.max, n, dtype=t, endpoint=True)
        ext = [info.min, info.max]
    if n >= len(ext):
        v[:len(ext)] = ext
    return v.reshape(shape, order="F")


@pytest.mark.parametrize("code,order", list(itertools.product(TYPES, "<>")))
@pytest.mark.parametrize("shape,ext", [((1, 1, 1), ".nii"), ((5, 4, 3), ".nii.gz")])
def test_reader_types_orders_shapes(tmp_path, code, order, shape, ext):
    arr = _values(code, shape)
    for k, (slope, inter) in enumerate([(0.0, 0.0), (0.5, -1024.0)]):
        p = tmp_path / f"v{k}{ext}"
        NR.write_nifti(p, arr, datatype=code, byteorder=order, slope=slope, inter=inter)
        got, hdr, aff = load_nifti(p, return_header=True)
        ref = NR.numpy_decode(arr, *( (slope, inter) if slope else (None, None)))
        assert got.dtype == np.float64 and got.shape == shape
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))
        assert hdr.datatype == code and hdr.shape == shape and hdr.byteorder == order
        assert np.array_equal(aff, np.eye(4))
        f32 = load_nifti(p, dtype=np.float32)
        assert f32.dtype == np.float32 and np.array_equal(f32.view(np.uint32), ref.astype(np.float32).view(np.uint32))


def test_reader_both_extensions_same_bytes(tmp_path):
    arr = _values(4, (5, 4, 3))
    NR.write_nifti(tmp_path / "a.nii", arr, slope=2.0, inter=1.0)
    NR.write_nifti(tmp_path / "a.nii.gz", arr, slope=2.0, inter=1.0)
    assert np.array_equal(load_nifti(tmp_path / "a.nii"), load_nifti(tmp_path / "a.nii.gz"))


def test_reader_trailing_singleton_and_offset(tmp_path):
    arr = _values(512, (5, 4, 3))
    NR.write_nifti(tmp_path / "t.nii", arr, dim=[4, 5, 4, 3, 1, 1, 1, 1], vox_offset=400)
    assert np.array_equal(load_nifti(tmp_path / "t.nii"), arr.astype(np.float64))
    NR.write_nifti(tmp_path / "t5.nii", arr, dim=[5, 5, 4, 3, 1, 1, 0, 0])
    assert load_nifti(tmp_path / "t5.nii").shape == (5, 4, 3)
    NR.write_nifti(tmp_path / "bad.nii", arr, dim=[4, 5, 4, 3, 2, 1, 1, 1])
    with pytest.raises(ValueError, match="past the third"):
        load_nifti(tmp_path / "bad.nii")
    NR.write_nifti(tmp_path / "two.nii", arr, dim=[2, 5, 4, 1, 1, 1, 1, 1])
    with pytest.raises(ValueError, match="dim"):
        load_nifti(tmp_path / "two.nii")


@pytest.mark.parametrize("slope", [0.0, float("nan"), float("inf"), float("-inf")])
def test_unscaled_slopes(tmp_path, slope):
    arr = _values(4, (5, 4, 3))
    NR.write_nifti(tmp_path / "s.nii", arr, slope=slope, inter=7.0)
    assert np.array_equal(load_nifti(tmp_path / "s.nii"), arr.astype(np.float64))
    NR.write_nifti(tmp_path / "n.nii", arr, slope=slope, inter=float("nan"))     # inter is not looked at
    assert np.array_equal(load_nifti(tmp_path / "n.nii"), arr.astype(np.float64))


@pytest.mark.parametrize("inter", [float("nan"), float("inf")])
def test_finite_slope_nonfinite_inter_is_an_error(tmp_path, inter):
    NR.write_nifti(tmp_path / "e.nii", _values(4, (5, 4, 3)), slope=2.0, inter=inter)
    with pytest.raises(ValueError, match="scl_inter"):
        load_nifti(tmp_path / "e.nii")


def test_scaling_is_two_roundings(tmp_path):
    """uint32 extremes with a 24-bit slope: the product is inexact in float64, so a fused multiply-add differs."""
    arr = np.array([0xFFFFFFFF, 0xFFFFFFFE, 0x80000001, 3], dtype=np.uint32).reshape(4, 1, 1)
    slope, inter = np.float32(1.7e-3), np.float32(3.25)
    NR.write_nifti(tmp_path / "u.nii", arr, slope=float(slope), inter=float(inter))
    ref = arr.astype(np.float64) * np.float64(slope) + np.float64(inter)
    assert np.array_equal(load_nifti(tmp_path / "u.nii"), ref)


def test_int64_truncates_toward_zero(tmp_path):
    arr = np.array([-3, -2, -1, 0, 1, 2, 3, 5], dtype=np.int16).reshape(2, 2, 2, order="F")
    NR.write_nifti(tmp_path / "l.nii", arr, slope=0.75, inter=-0.5)           # -2.75, -2, -1.25, -0.5, 0.25, ...
    got = load_nifti(tmp_path / "l.nii", dtype=np.int64)
    assert got.dtype == np.int64
    assert got.ravel(order="F").tolist() == [-2, -2, -1, 0, 0, 1, 1, 3]


def test_affine_precedence(tmp_path):
    arr = _values(2, (5, 4, 3))
    S = np.array([[-0.9, 0.1, 0.0, 120.5], [0.05, 0.8, -0.2, -33.25], [0.0, 0.3, 2.5, 7.0], [0, 0, 0, 1]])
    pix = [-1.0, 0.7, 0.8, 2.5, 0, 0, 0, 0]
    q = (0.0, 0.0, float(np.sqrt(0.5)), 10.0, -20.0, 30.0)
    NR.write_nifti(tmp_path / "sq.nii", arr, sform=S, qform=q, pixdim=pix)     # sform wins
    _, hdr, aff = load_nifti(tmp_path / "sq.nii", return_header=True)
    ref = np.eye(4)
    ref[:3] = np.float32(S[:3])
    assert aff.dtype == np.float64 and np.array_equal(aff, ref)
    assert hdr.zooms == tuple(float(np.float32(v)) for v in pix[1:4])
    NR.write_nifti(tmp_path / "p.nii", arr, pixdim=pix)                        # neither code set: pixdim only
    _, _, aff = load_nifti(tmp_path / "p.nii", return_header=True)
    assert np.array_equal(aff, np.diag([np.float32(0.7), np.float32(0.8), np.float32(2.5), 1.0]).astype(np.float64))
    NR.write_nifti(tmp_path / "s0.nii", arr, sform=S, sform_code=0, pixdim=pix)   # srow present but code 0
    _, _, aff = load_nifti(tmp_path / "s0.nii", return_header=True)
    assert np.array_equal(aff[:3, :3], np.diag([np.float32(0.7), np.float32(0.8), np.float32(2.5)]).astype(np.float64))


@pytest.mark.parametrize("bcd,qfac", [((0.0, 0.0, 0.0), 1.0), ((0.0, 0.0, float(np.sqrt(0.5))), 1.0),
                                      ((0.0, 0.0, 0.0), -1.0), ((0.1, -0.3, 0.5), -1.0), ((0.2, 0.4, -0.1), 0.0)])
def test_affine_from_qform(tmp_path, bcd, qfac):
    pix = [qfac, 0.7, 0.8, 2.5, 0, 0, 0, 0]
    off = (10.0, -20.5, 30.25)
    NR.write_nifti(tmp_path / "q.nii", _values(2, (5, 4, 3)), qform=bcd + off, pixdim=pix)
    _, hdr, aff = load_nifti(tmp_path / "q.nii", return_header=True)
    ref = NR.quaternion_matrix(*bcd, off, pix)
    assert np.abs(aff - ref).max() <= 1e-12
    if bcd == (0.0, 0.0, 0.0):
        assert np.array_equal(aff[:3, :3], np.diag([np.float32(0.7), np.float32(0.8),
                                                    np.float32(2.5) * (-1 if qfac < 0 else 1)]).astype(np.float64))
    if bcd[2] == float(np.sqrt(0.5)):          # a quarter turn about z: x -> y, y -> -x
        assert np.allclose(aff[:3, :3], [[0, -0.8, 0], [0.7, 0, 0], [0, 0, 2.5]], atol=1e-6)


def test_rejections(tmp_path):
    arr = _values(4, (5, 4, 3))
    NR.write_nifti(tmp_path / "pair.nii", arr, magic=b"ni1\0")
    with pytest.raises(ValueError, match="hdr/.img"):
        load_nifti(tmp_path / "pair.nii")
    NR.write_nifti(tmp_path / "n2.nii", arr, sizeof_hdr=540)
    with pytest.raises(ValueError, match="NIfTI-2"):
        load_nifti(tmp_path / "n2.nii")
    NR.write_nifti(tmp_path / "n2s.nii", arr, sizeof_hdr=540, byteorder=">")
    with pytest.raises(ValueError, match="NIfTI-2"):
        load_nifti(tmp_path / "n2s.nii")
    for code in (1, 32, 128, 1024, 1280, 1536, 1792, 2048):        # binary, complex64, rgb, int64, uint64, ...
        blob = bytearray(NR.build_nifti(arr))
        blob[70:72] = int(code).to_bytes(2, "little")
        (tmp_path / "dt.nii").write_bytes(bytes(blob))
        with pytest.raises(ValueError, match="datatype"):
            load_nifti(tmp_path / "dt.nii")
    blob = NR.build_nifti(arr)
    for cut, name in ((len(blob) - 1, "data.nii"), (352, "nodata.nii"), (200, "hdr.nii"), (0, "empty.nii")):
        (tmp_path / name).write_bytes(blob[:cut])
        with pytest.raises(ValueError, match="truncated"):
            load_nifti(tmp_path / name)
    gz = gzip.compress(blob)
    (tmp_path / "cut.nii.gz").write_bytes(gz[:len(gz) // 2])
    with pytest.raises(ValueError, match="truncated"):
        load_nifti(tmp_path / "cut.nii.gz")
    (tmp_path / "junk.nii").write_bytes(b"\x01" * 400)
    with pytest.raises(ValueError, match="not a NIfTI-1"):
        load_nifti(tmp_path / "junk.nii")
    NR.write_nifti(tmp_path / "off.nii", arr, vox_offset=352)
    blob = bytearray((tmp_path / "off.nii").read_bytes())
    blob[108:112] = np.float32(348).tobytes()
    (tmp_path / "off.nii").write_bytes(bytes(blob))
    with pytest.raises(ValueError, match="vox_offset"):
        load_nifti(tmp_path / "off.nii")
    with pytest.raises(FileNotFoundError):
        load_nifti(tmp_path / "absent.nii.gz")


@pytest.mark.parametrize("code", TYPES)
@pytest.mark.parametrize("ext", [".nii", ".nii.gz"])
def test_writer_fields(tmp_path, code, ext):
    arr = _values(code, (5, 4, 3), seed=3)
    A = np.array([[-0.9, 0.1, 0.0, 120.5], [0.05, 0.8, -0.2, -33.25], [0.0, 0.3, 2.5, 7.0], [0, 0, 0, 1]])
    p = tmp_path / f"w{ext}"
    save_nifti(arr, p, A)
    blob, gz = NR.read_file(p)
    assert gz == (ext == ".nii.gz")                                   # gzip framing follows the extension
    f = NR.parse_nifti(blob)                                          # native order = little-endian here
    assert f["sizeof_hdr"] == 348 and f["magic"] == b"n+1\0" and f["extension"] == b"\0\0\0\0"
    assert f["dim"] == [3, 5, 4, 3, 1, 1, 1, 1]
    assert f["datatype"] == code and f["bitpix"] == 8 * arr.dtype.itemsize
    assert f["vox_offset"] == 352.0 and f["trailing"] == 0
    assert f["scl_slope"] == 0.0 and f["scl_inter"] == 0.0
    assert f["sform_code"] == 2 and f["qform_code"] == 0 and f["xyzt_units"] == 2
    assert np.array_equal(f["srow"], np.float32(A[:3]))
    assert f["pixdim"][0] == 1.0
    assert np.array_equal(np.float32(f["pixdim"][1:4]), np.float32(np.sqrt((A[:3, :3] ** 2).sum(axis=0))))
    assert f["data_bytes"] == arr.tobytes(order="F")                  # bitwise, x fastest
    back, hdr, aff = load_nifti(p, return_header=True)               # round trip
    assert back.dtype == np.float64 and back.astype(arr.dtype).tobytes(order="F") == arr.tobytes(order="F")
    assert hdr.sform_code == 2 and hdr.zooms == tuple(float(np.float32(v)) for v in f["pixdim"][1:4])
    assert np.array_equal(aff[:3], np.float32(A[:3]).astype(np.float64)) and np.array_equal(aff[3], [0, 0, 0, 1])


def test_writer_defaults_and_errors(tmp_path):
    arr = _values(2, (3, 2, 4))
    save_nifti(arr, tmp_path / "sub" / "i.nii")                        # parent created, identity affine
    f = NR.parse_nifti(NR.read_file(tmp_path / "sub" / "i.nii")[0])
    assert np.array_equal(f["srow"], np.eye(4, dtype=np.float32)[:3]) and f["pixdim"][:4] == [1.0, 1.0, 1.0, 1.0]
    save_nifti(np.asfortranarray(arr), tmp_path / "f.nii")             # memory order does not matter
    assert NR.read_file(tmp_path / "f.nii")[0] == NR.read_file(tmp_path / "sub" / "i.nii")[0]
    with pytest.raises(ValueError, match="dtype"):
        save_nifti(arr.astype(np.int64), tmp_path / "x.nii")
    with pytest.raises(ValueError, match="3-D"):
        save_nifti(arr[0], tmp_path / "x.nii")
    with pytest.raises(ValueError, match=".nii"):
        save_nifti(arr, tmp_path / "x.img")


# ---------------------------------------------------------------- CSV lists
def _config(root, **data):
    d = {"modalities": ["CT", "PET"], "data_root": str(root), "train_csv": "train.csv", "val_csv": "val.csv"}
    d.update(data)
    return {"experiment": {"seed": 3}, "data": d, "model": {"out_channels": 3, "backbone": {"img_size": [16, 16, 16]}},
            "training": {"batch_size": 2}, "hardware": {}}


def test_get_dataset_reads_the_csv_lists(tmp_path):
    (tmp_path / "train.csv").write_text("patient_id,CT,PET,label\np1,ct/p1.nii.gz,pet/p1.nii.gz,label/p1.nii.gz\n"
                                        "p2,ct/p2.nii.gz,pet/p2.nii.gz,label/p2.nii.gz\n"
                                        "p3,ct/p3.nii.gz,pet/p3.nii.gz,label/p3.nii.gz\n")
    (tmp_path / "test.csv").write_text("patient_id,CT,PET,label\nq,ct/q.nii,pet/q.nii,label/q.nii\n")
    ds = get_dataset(_config(tmp_path), "train")
    assert len(ds) == 3 and ds.mods == ["CT", "PET"] and ds.rows[1]["patient_id"] == "p2"
    assert ds.rows[2]["PET"] == "pet/p3.nii.gz"
    with pytest.raises(FileNotFoundError, match="val.csv"):
        get_dataset(_config(tmp_path), "val")
    assert len(get_dataset(_config(tmp_path, test_csv="test.csv"), "test")) == 1       # the new split
    with pytest.raises(ValueError, match="Invalid split"):
        get_dataset(_config(tmp_path), "holdout")
    (tmp_path / "nolabel.csv").write_text("patient_id,CT,PET\np1,a,b\n")
    with pytest.raises(ValueError, match="'label'"):
        get_dataset(_config(tmp_path, train_csv="nolabel.csv"), "train")
    (tmp_path / "nopet.csv").write_text("patient_id,CT,label\np1,a,b\n")
    with pytest.raises(ValueError, match="'PET'"):
        get_dataset(_config(tmp_path, train_csv="nopet.csv"), "train")
    with pytest.raises(ValueError, match="Unsupported modality"):
        get_dataset(_config(tmp_path, modalities=["CT", "XRAY"]), "train")


def test_get_dataloader_over_csv_needs_no_gpu_to_build(tmp_path):
    from mmseg_amd.data.dataloader import get_dataloader
    from mmseg_amd.data.device import DeviceLoader
    rows = "".join(f"p{i},ct/p{i}.nii,pet/p{i}.nii,label/p{i}.nii\n" for i in range(5))
    (tmp_path / "train.csv").write_text("patient_id,CT,PET,label\n" + rows)
    (tmp_path / "val.csv").write_text("patient_id,CT,PET,label\n" + rows)
    ld = get_dataloader(_config(tmp_path), "train")
    assert isinstance(ld, DeviceLoader) and len(ld) == 2                # drop_last on the training split
    assert len(get_dataloader(_config(tmp_path), "val")) == 3
