"""Shared by the analysis tests: the goldens, case files, and the comparison with the derived tolerances.

Exact (==): counts, volume_voxels, num_voxels, suv_max, suv_min, suv_median, every *_volume and volume_ml (an exact
count times the pinned voxel volume), the absolute and percentage thresholds, threshold-curve values, histogram
counts and edges, masks.  Sums in another order: a mean over n values x is within (n - 1) 2^-53 sum|x| / n of the
exact mean whatever the order, so the device's and numpy's differ by at most twice that (mean_tol); a standard
deviation gets the variance's relative bound 2 (n + 4) 2^-53 (std_rtol), the mean's own error entering at second
order; the liver threshold the sum of its two parts' bounds; tlg its mean's bound times volume_ml.
"""
import json
import math
import os

import numpy as np

import analysis_ref as AR
from nifti_ref import write_nifti

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analysis.npz"))
U = 2.0 ** -53


def golden_cases():
    return [str(n) for n in GOLD["cases"]]


def golden_results(name):
    return json.loads(str(GOLD[f"{name}.results"]))


def decode(stored, slope=0.0, inter=0.0):
    """get_fdata(): float64, raw * slope + inter in two roundings when slope is set."""
    v = np.asarray(stored).astype(np.float64)
    if slope != 0.0:
        v = v * np.float64(np.float32(slope))
        v = v + np.float64(np.float32(inter))
    return v


def decoded(name):
    """(suv float64, seg int32 or None) of a golden case."""
    suv = decode(GOLD[f"{name}.suv"], float(GOLD[f"{name}.slope"]), float(GOLD[f"{name}.inter"]))
    seg = GOLD[f"{name}.seg"].astype(np.float64).astype(np.int32) if f"{name}.seg" in GOLD else None
    return suv, seg


def _item(o):
    if isinstance(o, np.generic):
        return o.item()
    raise TypeError(type(o))


def norm(d):
    """A result dict as JSON gives it back (tuples as lists, numpy scalars as Python's); floats survive exactly."""
    return json.loads(json.dumps(d, default=_item))


def write_case(d, suv, seg, zooms=(1.0, 1.0, 1.0), slope=0.0, inter=0.0, suv_order="<", seg_order="<", gz=True):
    """<d>/case_suv.nii[.gz] and, with a segmentation, <d>/case_pred.nii[.gz], as stored arrays."""
    from mmseg_amd.utils.nifti import save_nifti
    os.makedirs(d, exist_ok=True)
    ext = ".nii.gz" if gz else ".nii"
    pixdim = [1.0, *[float(np.float32(z)) for z in zooms], 0.0, 0.0, 0.0, 0.0]
    affine = np.diag([*[float(z) for z in zooms], 1.0])
    exact = all(float(np.float32(np.sqrt(float(z) ** 2))) == float(np.float32(z)) for z in zooms)
    if slope == 0.0 and suv_order == "<" and exact:
        save_nifti(suv, os.path.join(d, "case_suv" + ext), affine=affine)
    else:
        write_nifti(os.path.join(d, "case_suv" + ext), suv, slope=slope, inter=inter, pixdim=pixdim, sform=affine,
                    byteorder=suv_order)
    if seg is not None:
        if seg_order == "<" and exact:
            save_nifti(seg, os.path.join(d, "case_pred" + ext), affine=affine)
        else:
            write_nifti(os.path.join(d, "case_pred" + ext), seg, pixdim=pixdim, sform=affine, byteorder=seg_order)
    return d


# ---- tolerances
def mean_tol(v):
    v = np.asarray(v, dtype=np.float64).ravel()
    return 2.0 * (v.size - 1) * U * math.fsum(np.abs(v)) / v.size


def std_rtol(n):
    return 2.0 * (n + 4) * U


def close(got, want, tol, what):
    print(f"{what}: got {got!r} want {want!r} |diff| {abs(got - want):.3e} tol {tol:.3e}")
    assert abs(got - want) <= tol, what


def compare_suv(got, want, suv, seg):
    got, want = norm(got), norm(want)
    assert [r["organ"] for r in got["organs"]] == [r["organ"] for r in want["organs"]]
    for g, w in zip(got["organs"], want["organs"]):
        v = suv[seg == w["label_id"]]
        assert list(g) == list(w)
        for k in w:
            if k == "suv_mean":
                close(g[k], w[k], mean_tol(v), f"{w['organ']}.suv_mean")
            elif k == "suv_std":
                close(g[k], w[k], std_rtol(v.size) * w[k], f"{w['organ']}.suv_std")
            else:
                assert g[k] == w[k], (w["organ"], k, g[k], w[k])
    assert got["summary"] == want["summary"]


def compare_tumor(got, want, suv, seg, threshold=2.5):
    got, want = norm(got), norm(want)
    assert list(got) == list(want)
    for k in want:
        if k == "suv_mean":
            close(got[k], want[k], mean_tol(suv[(suv >= threshold) & (seg <= 0)]), "tumor.suv_mean")
        else:
            assert got[k] == want[k], (k, got[k], want[k])


def compare_tmtv(got, want, masks, suv, seg, liver_label=5):
    """masks: the expected {"absolute", "percentage", "liver"} masks, which say what each mean was taken over."""
    got, want = norm(got), norm(want)
    assert list(got) == list(want)
    liver = suv[seg == liver_label] if seg is not None else suv[:0]
    for method, mname in (("absolute", "absolute"), ("percentage", "percentage"), ("liver_based", "liver")):
        if method not in want:
            continue
        g, w = got[method], want[method]
        assert list(g) == list(w), method
        v = suv[masks[mname] == 1] if mname in masks else suv[:0]
        for k in w:
            if k == "suv_mean" and w[k] != 0:
                close(g[k], w[k], mean_tol(v), f"{method}.suv_mean")
            elif k == "suv_peak":
                c = AR.first_max_index(suv, masks["absolute"] == 1)
                box = suv[tuple(slice(max(0, i - 3), min(n, i + 4)) for i, n in zip(c, suv.shape))]
                close(g[k], w[k], mean_tol(box), "suv_peak")
            elif k == "liver_mean":
                close(g[k], w[k], mean_tol(liver), "liver_mean")
            elif k == "liver_std":
                close(g[k], w[k], std_rtol(liver.size) * w[k], "liver_std")
            elif k == "threshold" and method == "liver_based":
                close(g[k], w[k], mean_tol(liver) + 2.0 * std_rtol(liver.size) * w["liver_std"], "liver threshold")
            else:
                assert g[k] == w[k], (method, k, g[k], w[k])
    g, w = got["tlg"], want["tlg"]
    assert list(g) == list(w)
    if w["tlg"] == 0:
        assert g == w
    else:
        t = mean_tol(suv[masks["absolute"] == 1])
        assert g["volume_ml"] == w["volume_ml"]
        close(g["mean_suv"], w["mean_suv"], t, "tlg.mean_suv")
        close(g["tlg"], w["tlg"], t * w["volume_ml"], "tlg.tlg")


def compare_histogram(got, want, suv, seg, labels=AR.ORGANS):
    got, want = norm(got), norm(want)
    assert list(got["per_organ"]) == list(want["per_organ"])
    name_to_label = {n: l for l, n in labels.items()}
    for organ, w in want["per_organ"].items():
        g, v = got["per_organ"][organ], suv[seg == name_to_label[organ]]
        close(g["mean"], w["mean"], mean_tol(v), f"{organ}.mean")
        close(g["std"], w["std"], std_rtol(v.size) * w["std"], f"{organ}.std")
        for k in ("median", "max", "min"):
            assert g[k] == w[k], (organ, k, g[k], w[k])
    assert got["threshold_curves"] == want["threshold_curves"]
