"""Generate tests/golden/analysis.npz by running the REFERENCE's SUVAnalyzer, TMTVAnalyzer and HistogramAnalyzer
(wittyseok/multimodal-organ-segmentation, src/analysis/suv.py, tmtv.py, histogram.py) on the CPU.

Run once where the reference is checked out and pandas and matplotlib are installed:

    MMSEG_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_analysis.py

Only data is written; no reference source is copied.  The reference is imported in place.  `nibabel` is a stub
whose load() is backed by this project's load_nifti (get_fdata(), header.get_zooms() as float32, affine) and whose
save() captures the mask array; DataFrame.to_excel is a no-op (openpyxl is absent) and matplotlib draws with Agg
into a scratch directory, so the three analyze() methods run unchanged.

Per case <c> (`cases` lists the names):
    <c>.suv, <c>.seg       the volumes as stored in the files ([X, Y, Z]; seg absent for a case without one)
    <c>.slope, <c>.inter   scl_slope / scl_inter of the SUV file (0, 0 = unscaled)
    <c>.zooms              pixdim[1..3] (float32)
    <c>.results            JSON text: {"suv", "tumor", "tmtv", "histogram"} -> the dicts the reference returned
    <c>.mask.<name>        the masks the reference saved (absolute, percentage, liver_based)
    <c>.hist.<organ>.counts / .edges    np.histogram(organ_suv, bins=100): what the reference's ax.hist computes
    <c>.abscurve.<organ>   counts of organ_suv >= t over np.linspace(0, 20, 50) (the reference plots these)
Precondition asserted here: no SUV voxel lies within relative 1e-9 of a case's liver-based threshold.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile
import types

import numpy as np

os.environ.setdefault("MPLBACKEND", "Agg")
REF = os.environ.get("MMSEG_REFERENCE")
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPE = (24, 20, 18)
SAVED = {}


def _install_stubs():
    import mmseg_amd  # noqa: F401
    from mmseg_amd.utils.nifti import load_nifti

    class Header:
        def __init__(self, h):
            self._h = h

        def get_zooms(self):
            return tuple(np.float32(z) for z in self._h.zooms)

    class Image:
        def __init__(self, data, affine, header=None):
            self._data, self.affine, self.header = data, affine, header

        def get_fdata(self):
            return np.asarray(self._data, dtype=np.float64)

    def load(path):
        data, h, affine = load_nifti(path, return_header=True)
        return Image(data, affine, Header(h))

    def save(img, path):
        SAVED[os.path.basename(str(path))] = np.array(img._data)

    nib = types.ModuleType("nibabel")
    nib.load, nib.save, nib.Nifti1Image, nib.Nifti1Header = load, save, Image, Header
    sys.modules["nibabel"] = nib
    import pandas as pd
    pd.DataFrame.to_excel = lambda self, *a, **k: None


def _import_reference():
    if not REF:
        raise SystemExit("set MMSEG_REFERENCE to the reference checkout")
    sys.dont_write_bytecode = True
    _install_stubs()
    sys.path.insert(0, REF)
    # the package's __init__ also imports its report generator, which needs python-docx: import the three analyzer
    # modules under an empty package of the same name and path instead
    import src
    pkg = types.ModuleType("src.analysis")
    pkg.__path__ = [os.path.join(REF, "src", "analysis")]
    sys.modules["src.analysis"] = src.analysis = pkg
    from src.analysis.histogram import HistogramAnalyzer
    from src.analysis.suv import SUVAnalyzer
    from src.analysis.tmtv import TMTVAnalyzer
    return SUVAnalyzer, TMTVAnalyzer, HistogramAnalyzer


def organ_boxes(seg, labels):
    """One box per organ label, placed on a fixed lattice of SHAPE."""
    spots = {1: (2, 2, 2), 2: (10, 2, 2), 3: (17, 2, 2), 4: (2, 11, 3), 5: (9, 10, 8), 6: (18, 11, 3), 7: (3, 3, 11)}
    sizes = {1: (5, 5, 4), 2: (4, 5, 5), 3: (5, 4, 3), 4: (5, 6, 5), 5: (8, 8, 7), 6: (4, 5, 6), 7: (5, 5, 5)}
    for l in labels:
        (x, y, z), (a, b, c) = spots[l], sizes[l]
        seg[x:x + a, y:y + b, z:z + c] = l


def phantom(seed):
    """A background of about 1 SUV; the cases paint organs and lesions over it."""
    rng = np.random.Generator(np.random.PCG64(seed))
    suv = rng.gamma(4.0, 0.25, SHAPE)
    return rng, suv


def make_cases():
    cases = {}
    # 1: float32 SUV, all seven organs, hot lesions, a label above organ_max
    rng, suv = phantom(101)
    seg = np.zeros(SHAPE, dtype=np.uint8)
    organ_boxes(seg, range(1, 8))
    for l in range(1, 8):
        suv[seg == l] = rng.gamma(6.0, 0.3 + 0.1 * l, int((seg == l).sum()))
    suv[20:23, 16:19, 12:16] = rng.uniform(3.0, 9.0, (3, 3, 4))
    suv[1:3, 17:19, 15:17] = rng.uniform(2.0, 6.0, (2, 2, 2))
    seg[12:14, 1:3, 14:16] = 9
    cases["seven_organs_f32"] = dict(suv=suv.astype(np.float32), seg=seg, slope=0.0, inter=0.0, zooms=(1.5, 1.5, 2.0))
    # 2: int16 SUV with slope / inter, no liver, a one-voxel organ, negative labels
    rng, suv = phantom(202)
    seg = np.zeros(SHAPE, dtype=np.int16)
    organ_boxes(seg, (1, 2, 4, 6))
    seg[20, 18, 16] = 3
    seg[0:2, 0:2, 16:18] = -1
    for l in (1, 2, 3, 4, 6):
        suv[seg == l] = rng.gamma(5.0, 0.5, int((seg == l).sum()))
    suv[12:15, 12:15, 1:4] = rng.uniform(2.0, 7.0, (3, 3, 3))
    slope, inter = float(np.float32(0.0025)), float(np.float32(-0.5))
    stored = np.clip(np.round((suv - inter) / slope), -32768, 32767).astype(np.int16)
    cases["int16_scaled_no_liver"] = dict(suv=stored, seg=seg, slope=slope, inter=inter, zooms=(0.7, 1.3, 2.1))
    # 3: nothing at or above the absolute threshold; the liver brighter than every background voxel
    rng, suv = phantom(303)
    suv = np.minimum(suv, 1.9)
    seg = np.zeros(SHAPE, dtype=np.uint8)
    organ_boxes(seg, (2, 5, 7))
    suv[seg == 5] = rng.uniform(2.0, 2.4, int((seg == 5).sum()))
    suv[seg == 2] = 1.25                      # min == max: the histogram's widened range
    cases["nothing_above_threshold"] = dict(suv=suv.astype(np.float32), seg=seg, slope=0.0, inter=0.0,
                                            zooms=(1.0, 1.0, 1.0))
    # 4: no segmentation file
    rng, suv = phantom(404)
    suv[5:9, 5:9, 5:9] = rng.uniform(2.0, 12.0, (4, 4, 4))
    cases["no_segmentation"] = dict(suv=suv.astype(np.float32), seg=None, slope=0.0, inter=0.0, zooms=(2.0, 2.0, 3.0))
    return cases


def write_case(d, c):
    """The case as files: <d>/case_suv.nii.gz and, with a segmentation, <d>/case_seg.nii.gz."""
    from nifti_ref import write_nifti
    pixdim = [1.0, *[float(np.float32(z)) for z in c["zooms"]], 0.0, 0.0, 0.0, 0.0]
    sform = np.diag([*c["zooms"], 1.0])
    write_nifti(os.path.join(d, "case_suv.nii.gz"), c["suv"], slope=c["slope"], inter=c["inter"], pixdim=pixdim,
                sform=sform)
    if c["seg"] is not None:
        write_nifti(os.path.join(d, "case_seg.nii.gz"), c["seg"], pixdim=pixdim, sform=sform)


def _jsonable(o):
    if isinstance(o, np.generic):
        return o.item()
    raise TypeError(type(o))


def main():
    SUVAnalyzer, TMTVAnalyzer, HistogramAnalyzer = _import_reference()
    from mmseg_amd.utils.nifti import load_nifti
    out, names = {}, []
    for name, c in make_cases().items():
        with tempfile.TemporaryDirectory() as d, tempfile.TemporaryDirectory() as o:
            write_case(d, c)
            SAVED.clear()
            res = {"tmtv": TMTVAnalyzer({}).analyze(d, o)}
            suv = load_nifti(os.path.join(d, "case_suv.nii.gz"))
            if c["seg"] is not None:
                res["suv"] = SUVAnalyzer({}).analyze(d, o)
                res["tumor"] = SUVAnalyzer({}).analyze_tumor(os.path.join(d, "case_suv.nii.gz"),
                                                             os.path.join(d, "case_seg.nii.gz"))
                res["histogram"] = HistogramAnalyzer({}).analyze(d, o)
                seg = c["seg"].astype(np.int32)
                for label, organ in SUVAnalyzer.ORGAN_LABELS.items():
                    v = suv[seg == label]
                    if v.size:
                        counts, edges = np.histogram(v, bins=100)
                        out[f"{name}.hist.{organ}.counts"], out[f"{name}.hist.{organ}.edges"] = counts, edges
                        out[f"{name}.abscurve.{organ}"] = np.array([(v >= t).sum() for t in np.linspace(0, 20, 50)])
                lb = res["tmtv"]["liver_based"]
                if "threshold" in lb:
                    gap = np.abs(suv - lb["threshold"]).min() / abs(lb["threshold"])
                    assert gap > 1e-9, f"{name}: a voxel within {gap:.1e} of the liver threshold; choose another seed"
            for fname, mask in SAVED.items():
                out[f"{name}.mask.{fname[len('tmtv_'):-len('.nii.gz')]}"] = mask.astype(np.uint8)
        out[f"{name}.suv"] = c["suv"]
        if c["seg"] is not None:
            out[f"{name}.seg"] = c["seg"]
        out[f"{name}.slope"], out[f"{name}.inter"] = np.float64(c["slope"]), np.float64(c["inter"])
        out[f"{name}.zooms"] = np.asarray(c["zooms"], dtype=np.float32)
        out[f"{name}.results"] = np.array(json.dumps(res, default=_jsonable))
        names.append(name)
        print(name, json.dumps(res["tmtv"], default=_jsonable)[:300])
    out["cases"] = np.array(names)
    path = os.path.join(OUT, "analysis.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
