"""Host side of the boundary metrics (trainer/metrics.py) without a GPU: the two-order-statistic percentile
against np.percentile bit for bit, the data-parallel merge of the per-sample distances, and the numpy checker
of the GPU tests (tests/metrics_ref.py) against the reference's own output (tests/golden/metrics_boundary.npz)."""
import numpy as np
import pytest

import mmseg_amd  # noqa: F401
from mmseg_amd.trainer import metrics as M
from tests import metrics_ref as R
from tests.helpers import golden

QS = (95, 50, 100, 0)


def _bits(x):
    return np.float64(x).view(np.uint64)


def _check(a, q):
    got, ref = M.percentile_linear(a, q), np.percentile(a, q)
    assert _bits(got) == _bits(ref), f"n={len(a)} q={q}: {got!r} != {ref!r}"


@pytest.mark.parametrize("q", QS)
def test_percentile_bitwise_every_n(q):
    """Every n in 1..4096: random fp64 values (signed, wide range) and non-negative distance-like values."""
    rng = np.random.Generator(np.random.PCG64(q))
    wide = rng.standard_normal(4096) * np.exp(rng.uniform(-20, 20, 4096))
    dist = np.sqrt(rng.integers(0, 400, 4096).astype(np.float64)) * 1.3
    for n in range(1, 4097):
        _check(wide[:n], q)
        _check(dist[4096 - n:], q)


@pytest.mark.parametrize("q", QS)
def test_percentile_bitwise_heavy_ties(q):
    """Arrays of two to four distinct values: the two order statistics are usually equal, sometimes straddle."""
    rng = np.random.Generator(np.random.PCG64(100 + q))
    for n in list(range(1, 200)) + [255, 256, 257, 1000, 4095, 4096]:
        for k in (2, 3, 4):
            vals = np.sort(rng.random(k) * 10.0)
            _check(vals[rng.integers(0, k, n)], q)
        _check(np.full(n, 1.4142135623730951), q)


def test_percentile_float_percentiles():
    rng = np.random.Generator(np.random.PCG64(5))
    a = rng.random(777)
    for q in (95.0, 97.5, 33.3, 99.9, 0.1):
        for n in (1, 2, 3, 10, 101, 777):
            _check(a[:n], q)


def test_order_stat_indices():
    assert M.order_stat_indices(1, 95) == (0, 0)
    assert M.order_stat_indices(10, 100) == (9, 9)
    assert M.order_stat_indices(10, 0) == (0, 1)
    assert M.order_stat_indices(21, 95) == (19, 20)     # vi = 20 * 0.95 = 19.0 exactly
    assert M.order_stat_indices(101, 50) == (50, 51)


def test_dp_merge_of_moments():
    """[count, sum d, sum d^2] summed over the ranks gives the mean / std of the concatenated lists to 1e-12."""
    rng = np.random.Generator(np.random.PCG64(11))
    for sizes in ((3, 5), (1, 0, 7, 2), (40, 40, 40, 40, 40, 40, 40, 40), (1,), (0, 1)):
        lists = [list(rng.uniform(0.0, 60.0, s)) for s in sizes]
        merged = M.hd_from_moments(np.sum([M.hd_moments(lst) for lst in lists], axis=0))
        allv = np.concatenate([np.asarray(lst, dtype=np.float64) for lst in lists])
        assert set(merged) == {"hausdorff_distance", "hausdorff_distance_std"}
        assert abs(merged["hausdorff_distance"] - np.mean(allv)) <= 1e-12
        assert abs(merged["hausdorff_distance_std"] - np.std(allv)) <= 1e-12
    assert M.hd_from_moments(M.hd_moments([]) + M.hd_moments([])) == {"hausdorff_distance": float("inf")}


def test_checker_reproduces_golden_at_unit_spacing():
    """tests/metrics_ref.py (brute-force EDT + roll border + np.percentile) == the reference (scipy EDT), bit for
    bit, on every unit-spacing case of the golden file."""
    g = golden("metrics_boundary")
    seen = 0
    for name in g["hd_cases"]:
        ups = [(g[f"{name}.pred{u}"], g[f"{name}.target{u}"], g[f"{name}.spacing{u}"])
               for u in range(int(g[f"{name}.nupd"]))]
        if any(sp.any() for _, _, sp in ups):
            continue
        dist, res = R.hausdorff([(p, t, None) for p, t, _ in ups], float(g[f"{name}.q"]))
        want = g[f"{name}.distances"]
        assert len(dist) == len(want) and np.array_equal(np.asarray(dist, dtype=np.float64).view(np.uint64),
                                                         want.view(np.uint64)), name
        assert _bits(res["hausdorff_distance"]) == _bits(g[f"{name}.hd"]), name
        if "hausdorff_distance_std" in res:
            assert _bits(res["hausdorff_distance_std"]) == _bits(g[f"{name}.hd_std"]), name
        else:
            assert np.isnan(g[f"{name}.hd_std"]), name
        seen += 1
    assert seen >= 8


def test_checker_confusion_matches_golden():
    g = golden("metrics_boundary")
    for name in g["cm_cases"]:
        C = int(g[f"{name}.C"])
        m = R.confusion(g[f"{name}.pred"], g[f"{name}.target"], C)
        assert np.array_equal(m, g[f"{name}.matrix"])
        res = M.confusion_summary(m)
        for k, v in res.items():
            want = g[f"{name}.{k}"]
            got = np.asarray(v, dtype=want.dtype)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), (name, k)


def test_cpu_tensors_raise():
    import torch
    m = torch.zeros(1, 3, 3, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        M.HausdorffDistance().update(m, m)
    with pytest.raises(RuntimeError):
        M.ConfusionMatrix(3).update(m, m)
    with pytest.raises(RuntimeError):
        M.distance_transform_edt(m)


def test_get_metrics_keys_and_lazy_buffers():
    ms = M.get_metrics({"model": {"out_channels": 3}})
    assert set(ms) == {"dice", "confusion"}
    assert ms["confusion"]._dev is None and ms["confusion"].invalid == 0
    assert np.array_equal(ms["confusion"].matrix, np.zeros((3, 3), dtype=np.int64))
