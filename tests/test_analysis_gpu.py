"""--mode analysis on the device (csrc/analysis.hip through analysis/): the reference's goldens, and
tests/analysis_ref.py on the shapes, input types and values the goldens do not hold.

Tolerances are derived, none tuned (tests/analysis_cases.py states them in full).  Exact: counts, volume_voxels,
num_voxels, suv_max / min / median, every *_volume and volume_ml, the absolute and percentage thresholds, histogram
counts and edges, threshold curves, all masks.  A mean over n values: 2 (n - 1) 2^-53 sum|x| / n (numpy's error plus
the kernel's, either order of summation), computed per quantity from the inputs with math.fsum: suv_mean, liver_mean,
mean_suv, suv_peak.  suv_std, liver_std: relative 2 (n + 4) 2^-53.  The liver threshold: the sum of its two parts'
bounds.  tlg: its mean_suv bound times volume_ml.  The liver-based mask is exact because every case keeps its
voxels away from the liver threshold (asserted where the case is built).
"""
import json
import os

import numpy as np
import pytest

import analysis_ref as AR
from analysis_cases import (GOLD, compare_histogram, compare_suv, compare_tmtv, compare_tumor, decode, decoded,
                            golden_cases, golden_results, write_case)

pytestmark = pytest.mark.gpu


def analyzers(config=None):
    from mmseg_amd.analysis import HistogramAnalyzer, SUVAnalyzer, TMTVAnalyzer
    config = config or {}
    return SUVAnalyzer(config), TMTVAnalyzer(config), HistogramAnalyzer(config)


def liver_gap_ok(suv, seg, organ_max=7, liver_label=5):
    """The precondition of an exact liver-based mask and count: no tumor_region voxel (the only ones the threshold
    is applied to) within relative 1e-9 of mean + 2 std, which the device and numpy round differently."""
    v = suv[seg == liver_label] if seg is not None and liver_label <= organ_max else suv[:0]
    region = suv[AR.region(seg, suv.shape, organ_max)]
    if v.size == 0 or region.size == 0:
        return True
    thr = v.mean() + 2 * v.std()
    return np.abs(region - thr).min() > 1e-9 * abs(thr)


def run_and_compare(tmp_path, suv_stored, seg_stored, zooms=(1.0, 1.0, 1.0), slope=0.0, inter=0.0, want=None,
                    want_masks=None, config=None, gz=True, **orders):
    """The case through files and the three analyzers, against `want` (the goldens) or analysis_ref."""
    from mmseg_amd.analysis import voxel_volume_ml
    from mmseg_amd.utils.nifti import load_nifti
    config = config or {}
    organ_max = config.get("analysis", {}).get("suv", {}).get("organ_max", 7)
    liver_label = config.get("analysis", {}).get("suv", {}).get("liver_label", 5)
    bins = config.get("analysis", {}).get("histogram", {}).get("bins", 100)
    d, o = tmp_path / "in", tmp_path / "out"
    write_case(str(d), suv_stored, seg_stored, zooms, slope, inter, gz=gz, **orders)
    suv = decode(suv_stored, slope, inter)
    seg = None if seg_stored is None else np.asarray(seg_stored).astype(np.float64).astype(np.int32)
    assert liver_gap_ok(suv, seg, organ_max, liver_label)
    vv = voxel_volume_ml(np.float32(zooms))
    sa, ta, ha = analyzers(config)
    if want is None:
        want = {}
        want["tmtv"], want_masks = AR.tmtv_stats(suv, seg, vv, organ_max=organ_max, liver_label=liver_label)
        if seg is not None:
            want["suv"] = AR.suv_stats(suv, seg, vv, organ_max=organ_max)
            want["tumor"] = AR.tumor_stats(suv, seg, vv)
            want["histogram"], want_hists, want_abs = AR.histogram_stats(suv, seg, bins=bins, organ_max=organ_max)
    else:
        want_hists = want_abs = None
    got = ta.analyze(d, o)
    compare_tmtv(got, want["tmtv"], want_masks, suv, seg, liver_label)
    ext = ".nii.gz"
    for key, fname in (("absolute", "tmtv_absolute"), ("percentage", "tmtv_percentage"), ("liver", "tmtv_liver_based")):
        if key in want_masks:
            saved = load_nifti(o / (fname + ext), dtype=np.uint8)
            assert np.array_equal(saved, want_masks[key]), key
        else:
            assert not (o / (fname + ext)).exists()
    assert (o / "tmtv_analysis.csv").exists()
    if seg is None:
        with pytest.raises(FileNotFoundError):
            sa.analyze(d, o)
        with pytest.raises(FileNotFoundError):
            ha.analyze(d, o)
        return
    compare_suv(sa.analyze(d, o), want["suv"], suv, seg)
    assert (o / "suv_analysis.csv").exists()
    ext_in = ".nii.gz" if gz else ".nii"
    compare_tumor(sa.analyze_tumor(d / ("case_suv" + ext_in), d / ("case_pred" + ext_in)), want["tumor"], suv, seg)
    compare_histogram(ha.analyze(d, o), want["histogram"], suv, seg)
    hists = ha.histograms()
    assert list(hists) == list(want["histogram"]["per_organ"])
    return hists, ha, want_hists, want_abs


def check_hists(hists, ha, want_hists, want_abs):
    for organ, (counts, edges) in hists.items():
        assert counts.dtype == np.int64 and edges.dtype == np.float64
        assert np.array_equal(counts, want_hists[organ][0]), organ
        assert np.array_equal(edges, want_hists[organ][1]), organ
    for organ, curve in ha.absolute_curves().items():
        n = want_hists[organ][0].sum()
        assert [c for _, c in curve] == [c / n * 100 for c in want_abs[organ]], organ


# ------------------------------------------------------------------ goldens
@pytest.mark.parametrize("name", golden_cases())
def test_goldens(dev, tmp_path, name):
    want = golden_results(name)
    suv, seg = decoded(name)
    masks = {k: GOLD[f"{name}.mask.{g}"] for k, g in (("absolute", "absolute"), ("percentage", "percentage"),
                                                       ("liver", "liver_based")) if f"{name}.mask.{g}" in GOLD}
    r = run_and_compare(tmp_path, GOLD[f"{name}.suv"], GOLD[f"{name}.seg"] if seg is not None else None,
                        zooms=GOLD[f"{name}.zooms"], slope=float(GOLD[f"{name}.slope"]),
                        inter=float(GOLD[f"{name}.inter"]), want=want, want_masks=masks)
    if seg is not None:
        hists, ha, _, _ = r
        for organ, (counts, edges) in hists.items():
            assert np.array_equal(counts, GOLD[f"{name}.hist.{organ}.counts"]), organ
            assert np.array_equal(edges, GOLD[f"{name}.hist.{organ}.edges"]), organ
        for organ, curve in ha.absolute_curves().items():
            n = counts_of(GOLD, name, organ)
            assert [c for _, c in curve] == [c / n * 100 for c in GOLD[f"{name}.abscurve.{organ}"]], organ


def counts_of(gold, name, organ):
    return int(gold[f"{name}.hist.{organ}.counts"].sum())


# ------------------------------------------------------------------ shapes
def blob_case(shape, seed, dtype=np.float32, negative=False):
    """Random SUVs, organs 1..7 as boxes scaled to the shape, lesions in the background, a label above organ_max and
    negative labels."""
    rng = np.random.Generator(np.random.PCG64(seed))
    X, Y, Z = shape
    suv = rng.gamma(4.0, 0.25, shape)
    seg = np.zeros(shape, dtype=np.int16)
    for l in range(1, 8):
        x0, y0, z0 = (int(rng.integers(0, max(1, n - max(1, n // 3)))) for n in shape)
        seg[x0:x0 + max(1, X // 3), y0:y0 + max(1, Y // 3), z0:z0 + max(1, Z // 4)] = l
    for l in range(1, 8):
        k = int((seg == l).sum())
        suv[seg == l] = rng.gamma(5.0, 0.3 + 0.1 * l, k)
    hot = (rng.random(shape) < 0.01) & (seg == 0)
    suv[hot] = rng.uniform(2.0, 11.0, int(hot.sum()))
    seg[(rng.random(shape) < 0.002) & (seg == 0)] = 9
    seg[(rng.random(shape) < 0.002) & (seg == 0)] = -2
    if negative:
        suv -= 1.5
    return suv.astype(dtype), seg


@pytest.mark.parametrize("shape,gz", [((37, 29, 23), True), ((67, 45, 41), True), ((160, 96, 64), False),
                                      ((5, 3, 2), True)])
def test_shapes(dev, tmp_path, shape, gz):
    suv, seg = blob_case(shape, seed=sum(shape))
    check_hists(*run_and_compare(tmp_path, suv, seg, zooms=(1.5, 1.5, 2.0), gz=gz))


# ------------------------------------------------------------------ inputs
SMALL = (5, 3, 2)


def small_case(seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    seg = rng.integers(0, 4, SMALL).astype(np.uint8)
    seg[0, 0, 0], seg[1, 0, 0] = 5, 5
    return rng, seg


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32, np.float32, np.float64, np.int8, np.uint16, np.uint32])
def test_suv_datatypes(dev, tmp_path, dtype):
    rng, seg = small_case()
    if np.issubdtype(dtype, np.floating):
        suv = rng.normal(2.0, 2.0, SMALL).astype(dtype)
    else:
        info = np.iinfo(dtype)
        suv = rng.integers(max(info.min, -20), min(info.max, 20), SMALL).astype(dtype)
        suv[2, 1, 1], suv[4, 2, 1] = info.max, info.min
    suv[0, 0, 0], suv[1, 0, 0] = 3, 4          # the liver: mean + 2 std = 4.5, between the integer voxels
    check_hists(*run_and_compare(tmp_path, suv, seg))


@pytest.mark.parametrize("dtype", [np.int16, np.float64])
@pytest.mark.parametrize("scaled", [False, True])
def test_byte_swapped_and_scaled(dev, tmp_path, dtype, scaled):
    rng, seg = small_case(7)
    suv = (rng.normal(500.0, 400.0, SMALL)).astype(dtype)
    suv[0, 0, 0], suv[1, 0, 0] = 3, 4          # the liver: its threshold falls between the stored integers
    slope, inter = (float(np.float32(0.0123)), float(np.float32(-1.7))) if scaled else (0.0, 0.0)
    check_hists(*run_and_compare(tmp_path, suv, seg.astype(np.int16), slope=slope, inter=inter, suv_order=">",
                                 seg_order=">"))


@pytest.mark.parametrize("seg_dtype", [np.uint8, np.int16, np.float32])
def test_segmentation_datatypes(dev, tmp_path, seg_dtype):
    suv, seg = blob_case((37, 29, 23), seed=11)
    seg = np.where(seg < 0, 0, seg) if seg_dtype == np.uint8 else seg
    seg = seg.astype(seg_dtype)
    if seg_dtype == np.float32:
        seg[seg == 2] = 2.75           # truncated toward zero: still organ 2
        seg[seg == -2] = -0.5          # truncated to 0: tumor_region
    check_hists(*run_and_compare(tmp_path, suv, seg, slope=float(np.float32(0.5)), inter=float(np.float32(0.25))))


# ------------------------------------------------------------------ values
def trap_case():
    """float64 SUVs with negative values and the listed traps, on (37, 29, 23)."""
    shape = (37, 29, 23)
    suv, seg = blob_case(shape, seed=5, dtype=np.float64, negative=True)
    seg[seg == 9] = 0
    seg[3:10, 0:5, 0:14][seg[3:10, 0:5, 0:14] != 0] = 0          # room for the background's maxima
    # organ 7: one voxel; organ 6: two voxels; organ 3: min == max; organ 1 odd, organ 2 even counts
    seg[seg == 7] = 0
    seg[seg == 6] = 0
    seg[seg == 3] = 0
    seg[36, 28, 22] = 7
    seg[35, 28, 22], seg[35, 27, 22] = 6, 6
    seg[30:33, 0:2, 0:2] = 3
    suv[seg == 3] = -0.75
    for l in (1, 2):
        idx = np.argwhere(seg == l)
        if len(idx) % 2 != l % 2:
            seg[tuple(idx[0])] = 0
    assert (seg == 1).sum() % 2 == 1 and (seg == 2).sum() % 2 == 0
    # duplicated maxima inside organ 4
    idx = np.argwhere(seg == 4)
    suv[tuple(idx[3])] = suv[tuple(idx[-2])] = suv[seg == 4].max() + 0.5
    # the background's maximum twice: file order meets (6, 1, 2) first, C order (5, 1, 10)
    top = suv[(seg == 0) | (seg > 7)].max() + 1.0
    suv[5, 1, 10] = suv[6, 1, 2] = top
    bg = np.argwhere(seg == 0)
    free = [tuple(i) for i in bg if tuple(i) not in ((5, 1, 10), (6, 1, 2))]
    # a voxel exactly on the absolute threshold, the percentage threshold and the 40 / 50 / 60 % volume thresholds
    suv[free[10]] = 2.5
    suv[free[20]] = top * 0.4
    o5 = np.argwhere(seg == 5)
    m5 = suv[seg == 5].max()
    for j, f in enumerate((0.4, 0.5, 0.6)):
        suv[tuple(o5[j])] = m5 * f
    # and on a relative and an absolute curve threshold
    suv[tuple(o5[5])] = m5 * np.linspace(0, 1, 50)[17]
    suv[tuple(o5[6])] = np.linspace(0, 20, 50)[4]
    assert suv[seg == 5].max() == m5 and suv.min() < 0
    return suv, seg


def test_value_traps(dev, tmp_path):
    suv, seg = trap_case()
    hists, ha, want_hists, want_abs = run_and_compare(tmp_path, suv, seg, zooms=(0.7, 1.3, 2.1))
    check_hists(hists, ha, want_hists, want_abs)
    assert AR.first_max_index(suv, ((seg == 0) | (seg > 7)) & (suv >= 2.5)) == (5, 1, 10)
    assert {"brain", "spleen", "kidney_left"} <= set(hists)
    assert hists["kidney_left"][1][0] == -1.25 and hists["kidney_left"][1][-1] == -0.25


def test_every_voxel_in_an_organ(dev, tmp_path):
    """tumor_region is empty: the percentage threshold comes from the whole volume's maximum."""
    rng = np.random.Generator(np.random.PCG64(9))
    suv = rng.uniform(0.5, 9.0, SMALL).astype(np.float32)
    seg = rng.integers(1, 4, SMALL).astype(np.uint8)
    _, ta, _ = analyzers()
    check_hists(*run_and_compare(tmp_path, suv, seg))
    got = ta.analyze(tmp_path / "in", tmp_path / "out2")
    assert got["percentage"]["threshold"] == float(np.float64(suv.max()) * 0.4) and got["absolute"]["volume_ml"] == 0


def test_organ_max_and_liver_label_are_arguments(dev, tmp_path):
    suv, seg = blob_case((37, 29, 23), seed=21)
    config = {"analysis": {"suv": {"organ_max": 3, "liver_label": 2}, "histogram": {"bins": 37}}}
    hists, ha, want_hists, want_abs = run_and_compare(tmp_path, suv, seg, config=config)
    check_hists(hists, ha, want_hists, want_abs)
    assert list(hists) == ["bladder", "kidney_right", "kidney_left"] and len(hists["bladder"][0]) == 37


# ------------------------------------------------------------------ invalid, determinism, CLI
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_voxels_raise(dev, tmp_path, bad):
    suv, seg = blob_case((37, 29, 23), seed=31)
    dirty = suv.copy()
    dirty[7, 7, 7] = bad
    write_case(str(tmp_path / "dirty"), dirty, seg)
    for a in analyzers():
        with pytest.raises(ValueError, match="non-finite"):
            a.analyze(tmp_path / "dirty", tmp_path / "out")
    check_hists(*run_and_compare(tmp_path, suv, seg))


def test_two_calls_give_the_same_bits(dev, tmp_path):
    from mmseg_amd.analysis import analyze_files
    suv, seg = blob_case((67, 45, 41), seed=41)
    d = write_case(str(tmp_path / "in"), suv, seg)
    a, _ = analyze_files(d + "/case_suv.nii.gz", d + "/case_pred.nii.gz", want_masks=True)
    b, _ = analyze_files(d + "/case_suv.nii.gz", d + "/case_pred.nii.gz", want_masks=True)
    assert np.array_equal(a.u, b.u) and np.array_equal(a.masks, b.masks)
    assert a.masks.sum() > 0 and a.count(5) > 0


def test_main_analysis_mode(dev, tmp_path):
    import yaml

    import main as entry
    from mmseg_amd.utils import load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_config(os.path.join(root, "configs", "c6_unet_nifti.yaml"))
    cfg["experiment"]["log_dir"] = str(tmp_path / "logs")
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    suv, seg = blob_case((37, 29, 23), seed=51)
    write_case(str(tmp_path / "in"), suv, seg.astype(np.uint8) if seg.min() >= 0 else seg)
    with pytest.raises(ValueError, match="--input"):
        entry.main(["--mode", "analysis", "--config", str(tmp_path / "config.yaml")])
    out = tmp_path / "cli"
    entry.main(["--mode", "analysis", "--config", str(tmp_path / "config.yaml"), "--input", str(tmp_path / "in"),
                "--output", str(out)])
    for name in ("suv_analysis.csv", "tmtv_analysis.csv", "analysis.json", "tmtv_absolute.nii.gz",
                 "tmtv_percentage.nii.gz", "tmtv_liver_based.nii.gz"):
        assert (out / name).exists(), name
    with open(out / "analysis.json") as f:
        res = json.load(f)
    assert set(res) == {"suv", "tmtv", "histogram", "histogram_counts"}
    assert len(res["histogram_counts"]["liver"]["counts"]) == 100
    assert sum(res["histogram_counts"]["liver"]["counts"]) == int((seg == 5).sum())
