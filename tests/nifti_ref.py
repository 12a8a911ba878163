"""An independent statement of the single-file NIfTI-1 layout (nifti1.h field offsets), for the NIfTI tests:
build_nifti packs a file's bytes with struct.pack, parse_nifti unpacks them again.  Neither touches the
package's reader or writer (utils/nifti.py) -- this file is the yardstick they are held to.

Offsets: sizeof_hdr 0 (int32) | dim 40 (8 x int16) | datatype 70, bitpix 72 (int16) | pixdim 76 (8 x float32) |
vox_offset 108, scl_slope 112, scl_inter 116 (float32) | xyzt_units 123 (byte) | descrip 148 (80 bytes) |
qform_code 252, sform_code 254 (int16) | quatern_b/c/d 256, qoffset_x/y/z 268 (float32) | srow_x/y/z 280
(3 x 4 float32) | magic 344 (4 bytes) | extension flag 348 (4 bytes) | voxel data at vox_offset, x fastest.
"""
import gzip
import struct

import numpy as np

CODES = {2: np.uint8, 4: np.int16, 8: np.int32, 16: np.float32, 64: np.float64, 256: np.int8, 512: np.uint16,
         768: np.uint32}
CODE_OF = {np.dtype(t): c for c, t in CODES.items()}


def build_nifti(array, datatype=None, byteorder="<", slope=0.0, inter=0.0, sform=None, qform=None, pixdim=None,
                vox_offset=352, dim=None, magic=b"n+1\0", sizeof_hdr=348, sform_code=None, qform_code=None):
    """The bytes of a NIfTI-1 file holding `array` ([X, Y, Z], stored as CODES[datatype] in `byteorder`).
    sform: [3 or 4, 4] matrix -> srow_* with sform_code 1; qform: (b, c, d, qoffset_x, qoffset_y, qoffset_z)
    with qform_code 1; pixdim: all eight (default [1, 1, 1, 1, 0, 0, 0, 0]); dim: all eight (default
    [3, X, Y, Z, 1, 1, 1, 1])."""
    o = byteorder
    array = np.asarray(array)
    datatype = CODE_OF[array.dtype.newbyteorder("=")] if datatype is None else datatype
    np_type = np.dtype(CODES[datatype])
    hdr = bytearray(int(vox_offset))
    struct.pack_into(o + "i", hdr, 0, sizeof_hdr)
    dim = [3, array.shape[0], array.shape[1], array.shape[2], 1, 1, 1, 1] if dim is None else list(dim)
    struct.pack_into(o + "8h", hdr, 40, *dim)
    struct.pack_into(o + "h", hdr, 70, datatype)
    struct.pack_into(o + "h", hdr, 72, 8 * np_type.itemsize)
    struct.pack_into(o + "8f", hdr, 76, *([1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0] if pixdim is None else pixdim))
    struct.pack_into(o + "f", hdr, 108, float(vox_offset))
    struct.pack_into(o + "f", hdr, 112, slope)
    struct.pack_into(o + "f", hdr, 116, inter)
    hdr[123] = 2
    if qform is not None:
        struct.pack_into(o + "h", hdr, 252, 1 if qform_code is None else qform_code)
        struct.pack_into(o + "6f", hdr, 256, *qform)
    if sform is not None:
        struct.pack_into(o + "h", hdr, 254, 1 if sform_code is None else sform_code)
        struct.pack_into(o + "12f", hdr, 280, *np.asarray(sform, dtype=np.float64)[:3].ravel())
    hdr[344:348] = magic
    body = np.asarray(array).astype(np_type.newbyteorder(o)).tobytes(order="F")
    return bytes(hdr) + body


def write_nifti(path, array, **kw):
    """build_nifti to a file; a name ending in .gz is gzipped."""
    blob = build_nifti(array, **kw)
    path = str(path)
    if path.endswith(".gz"):
        with gzip.open(path, "wb") as f:
            f.write(blob)
    else:
        with open(path, "wb") as f:
            f.write(blob)
    return blob


def parse_nifti(blob, byteorder="<"):
    """The header fields of a NIfTI-1 byte string and its data as [X, Y, Z] (raw stored values, unscaled)."""
    o = byteorder
    u = lambda fmt, off: struct.unpack_from(o + fmt, blob, off)  # noqa: E731
    f = {"sizeof_hdr": u("i", 0)[0], "dim": list(u("8h", 40)), "datatype": u("h", 70)[0], "bitpix": u("h", 72)[0],
         "pixdim": list(u("8f", 76)), "vox_offset": u("f", 108)[0], "scl_slope": u("f", 112)[0],
         "scl_inter": u("f", 116)[0], "xyzt_units": blob[123], "qform_code": u("h", 252)[0],
         "sform_code": u("h", 254)[0], "quatern": list(u("3f", 256)), "qoffset": list(u("3f", 268)),
         "srow": np.array(u("12f", 280), dtype=np.float32).reshape(3, 4), "magic": bytes(blob[344:348]),
         "extension": bytes(blob[348:352])}
    shape = tuple(f["dim"][1:4])
    dt = np.dtype(CODES[f["datatype"]]).newbyteorder(o)
    off = int(f["vox_offset"])
    n = shape[0] * shape[1] * shape[2]
    f["data_bytes"] = bytes(blob[off:off + n * dt.itemsize])
    f["trailing"] = len(blob) - (off + n * dt.itemsize)
    f["data"] = np.frombuffer(blob, dtype=dt, count=n, offset=off).reshape(shape, order="F")
    return f


def read_file(path):
    """A file's bytes (gunzipped for .gz) and whether it had gzip framing (magic 1f 8b)."""
    with open(path, "rb") as fh:
        raw = fh.read()
    gz = raw[:2] == b"\x1f\x8b"
    return (gzip.decompress(raw) if gz else raw), gz


def quaternion_matrix(b, c, d, qoffset, pixdim):
    """The qform matrix in closed form (nifti1.h, "METHOD 2"), float64 arithmetic on the stored float32 values."""
    b, c, d = (float(np.float32(v)) for v in (b, c, d))
    a = np.sqrt(max(1.0 - (b * b + c * c + d * d), 0.0))
    R = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                  [2 * (b * c + a * d), a * a + c * c - b * b - d * d, 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (c * d + a * b), a * a + d * d - b * b - c * c]])
    pd = [float(np.float32(v)) for v in pixdim]
    qfac = -1.0 if pd[0] < 0 else 1.0
    M = np.eye(4)
    M[:3, :3] = R @ np.diag([pd[1], pd[2], pd[3] * qfac])
    M[:3, 3] = [float(np.float32(v)) for v in qoffset]
    return M


def numpy_decode(raw, slope=None, inter=None):
    """numpy's statement of the decode: (raw.astype(f8) * slope + inter).astype(f4), or raw.astype(f8).astype(f4)."""
    v = np.asarray(raw).astype(np.float64)
    if slope is not None:
        v = v * np.float64(slope) + np.float64(inter)
    return v
