"""Single-file NIfTI-1 reader / writer on numpy, gzip and struct (nibabel is not a dependency).

load_nifti / save_nifti have the reference's signatures (src/utils/io.py:54-112) and nibabel's published
semantics where the reference relies on them: get_fdata() (float64, `raw * scl_slope + scl_inter` in two
roundings, slope 0 or non-finite = unscaled), the sform > qform > pixdim affine precedence, and a fresh
writer header with an sform only.  The contract is the NIfTI-1 field layout (nifti1.h); parity with nibabel
itself is not pinned, the package being absent wherever this project is built.

read_nifti_raw returns the parsed header and the voxel block exactly as the file holds it: the device data
path (data/nifti.py) uploads those bytes and unswaps, scales, casts and permutes them in one kernel.
"""
from __future__ import annotations

import gzip
import math
import struct
import sys
import zlib
from dataclasses import dataclass, field
from pathlib import Path
from typing import Optional, Tuple, Union

import numpy as np

HEADER_BYTES = 348
VOX_OFFSET = 352          # header + the four extension-flag bytes
# NIfTI-1 datatype code -> numpy type (native order)
DATATYPES = {2: np.uint8, 4: np.int16, 8: np.int32, 16: np.float32, 64: np.float64, 256: np.int8, 512: np.uint16,
             768: np.uint32}
_CODE_OF = {np.dtype(t): c for c, t in DATATYPES.items()}
_NATIVE = "<" if sys.byteorder == "little" else ">"


@dataclass
class NiftiHeader:
    """The parsed fields of a NIfTI-1 header (not a nibabel object)."""
    shape: Tuple[int, int, int]
    datatype: int
    dtype: np.dtype                     # numpy type of a voxel, native byte order
    byteorder: str                      # "<" or ">": the file's
    swapped: bool                       # the file's order is not this machine's
    vox_offset: int
    scl_slope: float
    scl_inter: float
    scaled: bool                        # get_fdata applies slope / inter
    pixdim: Tuple[float, ...]           # all eight; pixdim[0] is qfac
    zooms: Tuple[float, float, float]   # pixdim[1..3]
    qform_code: int
    sform_code: int
    quatern: Tuple[float, float, float]
    qoffset: Tuple[float, float, float]
    srow: np.ndarray                    # [3, 4] float64
    xyzt_units: int
    descrip: bytes = b""
    affine: np.ndarray = field(default_factory=lambda: np.eye(4))

    @property
    def nvox(self) -> int:
        return self.shape[0] * self.shape[1] * self.shape[2]

    @property
    def nbytes(self) -> int:
        return self.nvox * self.dtype.itemsize


def quaternion_affine(b: float, c: float, d: float, qoffset, pixdim) -> np.ndarray:
    """The qform matrix of the NIfTI-1 standard (nifti1.h "METHOD 2"), in float64: a from the unit norm,
    columns scaled by pixdim[1..3], the third also by qfac = pixdim[0] (0 counts as +1)."""
    b, c, d = float(b), float(c), float(d)
    a = 1.0 - (b * b + c * c + d * d)
    if a < 1e-7:                       # a 180 degree rotation: renormalise (b, c, d), a = 0
        s = 1.0 / math.sqrt(b * b + c * c + d * d)
        b, c, d, a = b * s, c * s, d * s, 0.0
    else:
        a = math.sqrt(a)
    R = np.array([[a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c],
                  [2 * b * c + 2 * a * d, a * a + c * c - b * b - d * d, 2 * c * d - 2 * a * b],
                  [2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a + d * d - c * c - b * b]], dtype=np.float64)
    qfac = -1.0 if float(pixdim[0]) < 0 else 1.0
    M = np.eye(4, dtype=np.float64)
    M[:3, :3] = R * np.array([float(pixdim[1]), float(pixdim[2]), float(pixdim[3]) * qfac], dtype=np.float64)
    M[:3, 3] = [float(v) for v in qoffset]
    return M


def parse_header(buf: bytes, path="<bytes>") -> NiftiHeader:
    if len(buf) < HEADER_BYTES:
        raise ValueError(f"{path}: truncated NIfTI file ({len(buf)} bytes, the header alone is {HEADER_BYTES})")
    order = None
    for o in ("<", ">"):
        size = struct.unpack_from(o + "i", buf, 0)[0]
        if size == HEADER_BYTES:
            order = o
            break
        if size == 540:
            raise ValueError(f"{path}: NIfTI-2 (sizeof_hdr 540) is not supported; single-file NIfTI-1 only")
    if order is None:
        raise ValueError(f"{path}: not a NIfTI-1 file (sizeof_hdr is neither 348 nor its byte swap)")
    magic = buf[344:348]
    if magic == b"ni1\0":
        raise ValueError(f"{path}: an .hdr/.img pair (magic 'ni1') is not supported; single-file NIfTI-1 only")
    if magic != b"n+1\0":
        raise ValueError(f"{path}: not a single-file NIfTI-1 (magic {magic!r}, expected b'n+1\\x00')")
    u = lambda fmt, off: struct.unpack_from(order + fmt, buf, off)  # noqa: E731
    dim = u("8h", 40)
    if dim[0] < 3 or dim[0] > 7:
        raise ValueError(f"{path}: dim[0] = {dim[0]}; a volume of at least three dimensions is needed")
    if any(v != 1 for v in dim[4:dim[0] + 1]):
        raise ValueError(f"{path}: dimensions past the third must be 1 (dim = {list(dim[1:dim[0] + 1])})")
    shape = tuple(int(v) for v in dim[1:4])
    if any(v < 1 for v in shape):
        raise ValueError(f"{path}: invalid dimensions {shape}")
    datatype = u("h", 70)[0]
    if datatype not in DATATYPES:
        raise ValueError(f"{path}: unsupported NIfTI datatype {datatype} (supported: {sorted(DATATYPES)})")
    pixdim = u("8f", 76)
    vox_offset = u("f", 108)[0]
    if not math.isfinite(vox_offset) or vox_offset < VOX_OFFSET or vox_offset != int(vox_offset):
        raise ValueError(f"{path}: vox_offset {vox_offset} (a single-file NIfTI-1 starts its data at {VOX_OFFSET} "
                         "or later)")
    slope, inter = u("2f", 112)
    scaled = slope != 0 and math.isfinite(slope)
    if scaled and not math.isfinite(inter):
        raise ValueError(f"{path}: scl_slope {slope} with a non-finite scl_inter {inter}")
    qform_code, sform_code = u("2h", 252)
    quatern, qoffset = u("3f", 256), u("3f", 268)
    srow = np.array(u("12f", 280), dtype=np.float64).reshape(3, 4)
    if sform_code > 0:
        affine = np.eye(4, dtype=np.float64)
        affine[:3] = srow
    elif qform_code > 0:
        affine = quaternion_affine(*quatern, qoffset, pixdim)
    else:
        affine = np.diag([float(pixdim[1]), float(pixdim[2]), float(pixdim[3]), 1.0])
    return NiftiHeader(shape=shape, datatype=int(datatype), dtype=np.dtype(DATATYPES[datatype]), byteorder=order,
                       swapped=order != _NATIVE, vox_offset=int(vox_offset), scl_slope=float(slope),
                       scl_inter=float(inter), scaled=scaled, pixdim=tuple(float(v) for v in pixdim),
                       zooms=tuple(float(v) for v in pixdim[1:4]), qform_code=int(qform_code),
                       sform_code=int(sform_code), quatern=tuple(float(v) for v in quatern),
                       qoffset=tuple(float(v) for v in qoffset), srow=srow, xyzt_units=buf[123],
                       descrip=bytes(buf[148:228]).rstrip(b"\0"), affine=affine)


def _read_bytes(path: Path) -> bytes:
    if not path.exists():
        raise FileNotFoundError(f"NIfTI file not found: {path}")
    name = path.name.lower()
    if name.endswith(".hdr") or name.endswith(".img"):
        raise ValueError(f"{path}: an .hdr/.img pair is not supported; single-file NIfTI-1 (.nii, .nii.gz) only")
    if name.endswith(".gz"):
        try:
            with gzip.open(path, "rb") as f:
                return f.read()
        except (EOFError, zlib.error, gzip.BadGzipFile) as e:
            raise ValueError(f"{path}: truncated or corrupt gzip stream ({e})") from None
    with open(path, "rb") as f:
        return f.read()


def read_nifti_raw(path: Union[str, Path]) -> Tuple[NiftiHeader, np.ndarray]:
    """(header, voxel block): the X*Y*Z elements as the file stores them (x fastest, the file's byte order),
    a read-only uint8 view of header.nbytes bytes."""
    path = Path(path)
    buf = _read_bytes(path)
    h = parse_header(buf, path)
    if len(buf) < h.vox_offset + h.nbytes:
        raise ValueError(f"{path}: truncated NIfTI file ({len(buf)} bytes; {h.shape} of {h.dtype} from offset "
                         f"{h.vox_offset} needs {h.vox_offset + h.nbytes})")
    return h, np.frombuffer(buf, dtype=np.uint8, count=h.nbytes, offset=h.vox_offset)


def load_nifti(file_path: Union[str, Path], return_header: bool = False, dtype=None):
    """The volume as nibabel's get_fdata() gives it: float64 [X, Y, Z], scaled when the header says so; then
    `.astype(dtype)`.  With return_header: (data, NiftiHeader, affine [4, 4] float64)."""
    h, raw = read_nifti_raw(file_path)
    vox = raw.view(h.dtype.newbyteorder(h.byteorder)).reshape(h.shape, order="F")
    data = vox.astype(np.float64)
    if h.scaled:
        data *= np.float64(np.float32(h.scl_slope))
        data += np.float64(np.float32(h.scl_inter))
    if dtype is not None:
        data = data.astype(dtype)
    if return_header:
        return data, h, h.affine
    return data


def save_nifti(data: np.ndarray, save_path: Union[str, Path], affine: Optional[np.ndarray] = None,
               header: Optional[NiftiHeader] = None) -> None:
    """Write a 3-D array as a native-endian single-file NIfTI-1 (.nii.gz gzipped, .nii plain): datatype from the
    array's dtype, no scaling, sform_code 2 with srow = float32(affine), no qform, pixdim[1..3] = the column norms
    of the affine's 3x3 part.  affine None = the header's, or identity.  A NiftiHeader contributes its affine
    (when none is given), xyzt_units and descrip; every other field follows the array and the affine."""
    save_path = Path(save_path)
    data = np.asarray(data)
    if data.ndim != 3:
        raise ValueError(f"save_nifti: a 3-D volume is needed (got shape {data.shape})")
    if any(n > 32767 for n in data.shape):
        raise ValueError(f"save_nifti: NIfTI-1 dimensions are 16-bit (got shape {data.shape})")
    code = _CODE_OF.get(data.dtype.newbyteorder("="))
    if code is None:
        raise ValueError(f"save_nifti: unsupported dtype {data.dtype} (supported: "
                         f"{[np.dtype(t).name for t in DATATYPES.values()]})")
    if affine is None:
        affine = header.affine if header is not None else np.eye(4)
    affine = np.asarray(affine, dtype=np.float64)
    if affine.shape != (4, 4):
        raise ValueError(f"save_nifti: affine must be 4x4 (got {affine.shape})")
    itemsize = data.dtype.itemsize
    zooms = np.sqrt((affine[:3, :3] ** 2).sum(axis=0))
    hdr = bytearray(VOX_OFFSET)          # the last four bytes: no extensions
    p = lambda fmt, off, *v: struct.pack_into("=" + fmt, hdr, off, *v)  # noqa: E731
    p("i", 0, HEADER_BYTES)
    p("8h", 40, 3, data.shape[0], data.shape[1], data.shape[2], 1, 1, 1, 1)
    p("h", 70, code)
    p("h", 72, 8 * itemsize)
    p("8f", 76, 1.0, zooms[0], zooms[1], zooms[2], 1.0, 1.0, 1.0, 1.0)
    p("f", 108, float(VOX_OFFSET))
    p("2f", 112, 0.0, 0.0)
    hdr[123] = header.xyzt_units if header is not None else 2          # NIFTI_UNITS_MM
    if header is not None and header.descrip:
        hdr[148:148 + min(len(header.descrip), 79)] = header.descrip[:79]
    p("2h", 252, 0, 2)                   # qform_code 0, sform_code 2 (aligned)
    p("12f", 280, *np.float32(affine[:3]).ravel())
    hdr[344:348] = b"n+1\0"
    body = np.asarray(data, dtype=data.dtype.newbyteorder("=")).tobytes(order="F")
    save_path.parent.mkdir(parents=True, exist_ok=True)
    if save_path.name.lower().endswith(".gz"):
        with gzip.open(save_path, "wb", compresslevel=6) as f:
            f.write(bytes(hdr))
            f.write(body)
    elif save_path.name.lower().endswith(".nii"):
        with open(save_path, "wb") as f:
            f.write(bytes(hdr))
            f.write(body)
    else:
        raise ValueError(f"save_nifti: {save_path} must end in .nii or .nii.gz")
