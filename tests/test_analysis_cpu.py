"""--mode analysis without a GPU: the numpy statement of the semantics (tests/analysis_ref.py) against the goldens
the reference produced (tests/golden/analysis.npz), the C ABI's declarations, and the host helpers of analysis/."""
import csv
import json
import logging

import numpy as np
import pytest

import analysis_ref as AR
import mmseg_amd  # noqa: F401
from mmseg_amd import _lib
from mmseg_amd.analysis import core
from mmseg_amd.analysis.suv import SUV_COLUMNS

from analysis_cases import GOLD, decoded, golden_cases, golden_results, norm


@pytest.mark.parametrize("name", golden_cases())
def test_ref_reproduces_the_reference(name):
    suv, seg = decoded(name)
    want = golden_results(name)
    vv = core.voxel_volume_ml(GOLD[f"{name}.zooms"])
    got_tmtv, masks = AR.tmtv_stats(suv, seg, vv)
    assert norm(got_tmtv) == want["tmtv"]
    for key, mname in (("absolute", "absolute"), ("percentage", "percentage"), ("liver_based", "liver")):
        if f"{name}.mask.{key}" in GOLD:
            assert np.array_equal(masks[mname], GOLD[f"{name}.mask.{key}"]), key
    assert (f"{name}.mask.liver_based" in GOLD) == (seg is not None)
    if seg is None:
        return
    assert norm(AR.suv_stats(suv, seg, vv)) == want["suv"]
    assert norm(AR.tumor_stats(suv, seg, vv)) == want["tumor"]
    res, hists, abs_counts = AR.histogram_stats(suv, seg)
    assert norm(res) == want["histogram"]
    assert hists
    for organ, (counts, edges) in hists.items():
        assert np.array_equal(counts, GOLD[f"{name}.hist.{organ}.counts"]), organ
        assert np.array_equal(edges, GOLD[f"{name}.hist.{organ}.edges"]), organ
        assert np.array_equal(abs_counts[organ], GOLD[f"{name}.abscurve.{organ}"]), organ


def test_goldens_cover_the_irregular_dicts():
    r = {n: golden_results(n)["tmtv"] for n in golden_cases()}
    assert any("error" in v.get("liver_based", {}) for v in r.values())
    assert any(v["absolute"]["volume_ml"] == 0 and "suv_peak" not in v["absolute"] for v in r.values())
    assert any("liver_based" not in v for v in r.values())
    assert any(v.get("liver_based", {}).get("volume_ml") == 0 and "liver_std" in v["liver_based"] for v in r.values())


def test_header_declares_the_entry_points():
    protos = _lib.parse_header()
    for fn in ("mmseg_suv_analyze", "mmseg_suv_ws_bytes", "mmseg_suv_record_cells"):
        assert fn in protos, fn
    assert "mmseg_suv_record_cells" in _lib._VALUE_FUNCS
    assert len(protos["mmseg_suv_analyze"][1]) == 29


def test_record_size_and_argument_validation():
    L = _lib.lib()
    assert L.mmseg_suv_record_cells() == core.R_CELLS
    assert L.mmseg_suv_ws_bytes(0) == 0 and L.mmseg_suv_ws_bytes(512 * 512 * 256) > 0
    ok = [256, 16, 0, 0, 0.0, 0.0, None, 2, 0, 0, 0.0, 0.0, 4, 4, 4, 7, 5, 2.5, 0.4, 2.5, 256, 256, 50, 100, None, 256,
          256, 1 << 30, None]

    def bad(**kw):
        names = ["suv", "sdt", "ssw", "ssc", "ssl", "sin", "seg", "gdt", "gsw", "gsc", "gsl", "gin", "X", "Y", "Z",
                 "organ_max", "liver", "abs", "pct", "tum", "crel", "cabs", "nc", "bins", "masks", "rec", "ws",
                 "wsb", "stream"]
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        with pytest.raises(_lib.MmsegError):
            L.mmseg_suv_analyze(*a)

    # every one of these is refused before any launch (the pointers above are not device memory)
    bad(sdt=3)
    bad(organ_max=16)
    bad(organ_max=0)
    bad(suv=None)
    bad(rec=None)
    bad(ws=None)
    bad(crel=None)
    bad(bins=257)
    bad(nc=64)
    bad(X=0)
    bad(wsb=16)
    bad(seg=256, gdt=5)
    bad(suv=257, sdt=4)


def test_median_from_the_order_statistic_pair():
    rng = np.random.Generator(np.random.PCG64(5))
    for n in range(1, 65):
        for ties in (False, True):
            v = rng.normal(size=n)
            if ties:
                v = np.round(v * 2) / 2
            a = np.sort(v)
            assert core.median_from_pair(n, a[(n - 1) // 2], a[n // 2]) == float(np.median(v)), (n, ties)
    with pytest.raises(ValueError):
        core.median_from_pair(0, 0.0, 0.0)


def test_file_discovery_is_sorted(tmp_path):
    (tmp_path / "b").mkdir()
    (tmp_path / "a").mkdir()
    for p in ("b/x_suv.nii.gz", "a/z_suv.nii", "a/y_SUV.nii.gz", "b/m_pred.nii.gz", "a/n_label.nii"):
        (tmp_path / p).write_bytes(b"")
    assert core.find_file(tmp_path, ["*suv*.nii*", "*SUV*.nii*"]) == tmp_path / "a" / "z_suv.nii"
    assert core.find_file(tmp_path, ["*SUV*.nii*"]) == tmp_path / "a" / "y_SUV.nii.gz"
    # the first pattern with a match decides, as in the reference
    assert core.find_file(tmp_path, ["*seg*.nii*", "*label*.nii*", "*pred*.nii*"]) == tmp_path / "a" / "n_label.nii"
    assert core.find_file(tmp_path, ["*mask*.nii*"]) is None


def test_float32_voxel_volume():
    vv = core.voxel_volume_ml((1.5, 1.5, 3.0))
    assert vv.dtype == np.float32
    z = np.float32([0.7, 1.3, 2.1])
    assert core.voxel_volume_ml((0.7, 1.3, 2.1)) == np.float32(np.float32(z[0] * z[1]) * z[2]) / np.float32(1000.0)
    # the issue's example: float32(0.0045) times 1000 voxels is not 4.5
    v = np.int64(1000) * np.float32(0.0045)
    assert v.dtype == np.float64 and 4.4999998 < v < 4.4999999


def test_csv_columns(tmp_path):
    rows = [{c: i for i, c in enumerate(SUV_COLUMNS)}]
    core.write_csv(tmp_path / "suv.csv", rows, SUV_COLUMNS)
    with open(tmp_path / "suv.csv", newline="") as f:
        assert next(csv.reader(f)) == ["organ", "label_id", "suv_max", "suv_mean", "suv_std", "suv_median", "suv_min",
                                       "volume_ml", "volume_voxels", "suv_40_volume", "suv_50_volume", "suv_60_volume"]
    tm = golden_results("int16_scaled_no_liver")["tmtv"]
    cols = core.write_csv(tmp_path / "tmtv.csv", [{"metric": k, **v} for k, v in tm.items()])
    assert cols == ["metric", "volume_ml", "suv_max", "suv_mean", "suv_peak", "num_voxels", "threshold", "percentage",
                    "error", "tlg", "mean_suv"]
    with open(tmp_path / "tmtv.csv", newline="") as f:
        got = list(csv.DictReader(f))
    assert [r["metric"] for r in got] == ["absolute", "percentage", "liver_based", "tlg"]
    assert got[2]["error"] == "Liver not found in segmentation" and got[2]["suv_max"] == ""


def test_cli_flags_and_missing_input():
    import main as entry
    a = entry.parse_args(["--mode", "analysis", "--input", "x", "--suv-analysis", "--histogram"])
    assert a.suv_analysis and a.histogram and not a.tmtv_analysis
    cfg = {"experiment": {}, "hardware": {}, "training": {}, "model": {}, "data": {},
           "analysis": {"suv": {"enabled": False}, "tmtv": {"enabled": False}}}
    cfg = entry.merge_config_with_args(cfg, a)
    assert cfg["analysis"]["suv"]["enabled"] and cfg["analysis"]["histogram"]["enabled"]
    assert not cfg["analysis"]["tmtv"]["enabled"]
    with pytest.raises(ValueError, match="--input"):
        entry.run_analysis({"_args": {"input": None, "output": None}}, logging.getLogger("test"))


def test_absent_analysis_block_enables_everything():
    from mmseg_amd.analysis import analysis_config
    block = analysis_config({})
    assert all(block[k]["enabled"] for k in ("suv", "tmtv", "histogram"))
    assert block["tmtv"]["absolute_threshold"] == 2.5 and block["tmtv"]["percentage_threshold"] == 0.4
    assert block["histogram"]["bins"] == 100
    assert not analysis_config({"analysis": {"tmtv": {"enabled": False}}})["tmtv"]["enabled"]
    assert json.loads(json.dumps(block)) == block
