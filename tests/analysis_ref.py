"""Independent numpy statement of the analysis semantics (DESIGN.md "Analysis"): slots, thresholds, the histogram
edge rule and the SUVpeak box, on decoded float64 [X, Y, Z] volumes.  The goldens (tests/golden/analysis.npz, made
by the reference itself) pin it; the GPU tests use it for the shapes and values the goldens do not hold."""
import numpy as np

ORGANS = {1: "bladder", 2: "kidney_right", 3: "kidney_left", 4: "heart", 5: "liver", 6: "spleen", 7: "brain"}


def region(seg, shape, organ_max=7):
    """Slot 0: label 0 or above organ_max; everything when there is no segmentation."""
    if seg is None:
        return np.full(shape, True)
    return (seg == 0) | (seg > organ_max)


def ml(count, voxel_volume):
    return float(np.int64(count) * voxel_volume)


def suv_stats(suv, seg, voxel_volume, organ_max=7, organs=ORGANS):
    rows = []
    for label, name in organs.items():
        v = suv[seg == label] if label <= organ_max else suv[:0]
        if v.size == 0:
            continue
        top = float(v.max())
        row = dict(organ=name, label_id=label, suv_max=top, suv_mean=float(v.mean()), suv_std=float(v.std()),
                   suv_median=float(np.median(v)), suv_min=float(v.min()), volume_ml=ml(v.size, voxel_volume),
                   volume_voxels=int(v.size))
        for pct, frac in ((40, 0.4), (50, 0.5), (60, 0.6)):
            row[f"suv_{pct}_volume"] = ml(np.count_nonzero(v >= top * frac), voxel_volume)
        rows.append(row)
    return {"organs": rows, "summary": {"num_organs_analyzed": len(rows),
                                        "total_volume_ml": sum(r["volume_ml"] for r in rows)}}


def tumor_stats(suv, seg, voxel_volume, threshold=2.5):
    v = suv[(suv >= threshold) & (seg <= 0)]
    if v.size == 0:
        return {"num_lesions": 0, "total_volume_ml": 0, "max_suv": 0}
    return {"num_voxels": int(v.size), "volume_ml": ml(v.size, voxel_volume), "suv_max": float(v.max()),
            "suv_mean": float(v.mean()), "suv_median": float(np.median(v)), "threshold_used": threshold}


def first_max_index(suv, mask):
    """The C-order-first voxel of `mask` holding the mask's maximum."""
    flat = np.flatnonzero(mask.ravel(order="C") & (suv.ravel(order="C") == suv[mask].max()))
    return np.unravel_index(flat[0], suv.shape)


def suv_peak(suv, mask, radius=3):
    c = first_max_index(suv, mask)
    box = tuple(slice(max(0, i - radius), min(n, i + radius + 1)) for i, n in zip(c, suv.shape))
    return float(suv[box].mean())


def masked_stats(suv, mask, voxel_volume):
    v = suv[mask]
    return {"volume_ml": ml(v.size, voxel_volume), "suv_max": float(v.max()), "suv_mean": float(v.mean()),
            "num_voxels": int(v.size)}


def tmtv_stats(suv, seg, voxel_volume, abs_thr=2.5, pct=0.4, organ_max=7, liver_label=5):
    """(results, masks): masks = {"absolute", "percentage", "liver"} as uint8 [X, Y, Z]."""
    reg = region(seg, suv.shape, organ_max)
    empty = {"volume_ml": 0, "suv_max": 0, "suv_mean": 0}
    out, masks = {}, {}
    m_abs = reg & (suv >= abs_thr)
    masks["absolute"] = m_abs.astype(np.uint8)
    if m_abs.any():
        s = masked_stats(suv, m_abs, voxel_volume)
        out["absolute"] = {"volume_ml": s["volume_ml"], "suv_max": s["suv_max"], "suv_mean": s["suv_mean"],
                           "suv_peak": suv_peak(suv, m_abs), "num_voxels": s["num_voxels"], "threshold": abs_thr}
    else:
        out["absolute"] = {**empty, "threshold": abs_thr}
    top = suv[reg].max() if reg.any() else suv.max()
    pthr = top * pct
    m_pct = reg & (suv >= pthr)
    masks["percentage"] = m_pct.astype(np.uint8)
    if m_pct.any():
        out["percentage"] = {**masked_stats(suv, m_pct, voxel_volume), "threshold": float(pthr), "percentage": pct}
    else:
        out["percentage"] = {**empty, "threshold": pthr, "percentage": pct}
    if seg is not None:
        liver = suv[seg == liver_label] if 1 <= liver_label <= organ_max else suv[:0]
        if liver.size == 0:
            out["liver_based"] = {"volume_ml": 0, "error": "Liver not found in segmentation"}
            masks["liver"] = masks["absolute"].copy()
        else:
            mean, std = liver.mean(), liver.std()
            lthr = mean + 2 * std
            m_liv = reg & (suv >= lthr)
            masks["liver"] = m_liv.astype(np.uint8)
            tail = {"threshold": float(lthr), "liver_mean": float(mean), "liver_std": float(std)}
            out["liver_based"] = {**(masked_stats(suv, m_liv, voxel_volume) if m_liv.any() else empty), **tail}
    if m_abs.any():
        vol = np.int64(np.count_nonzero(m_abs)) * voxel_volume
        mean = suv[m_abs].mean()
        out["tlg"] = {"tlg": float(vol * mean), "volume_ml": float(vol), "mean_suv": float(mean)}
    else:
        out["tlg"] = {"tlg": 0, "volume_ml": 0, "mean_suv": 0}
    return out, masks


def histogram_edges(lo, hi, bins):
    """np.histogram's edges: linspace over (min, max), widened by 0.5 each way when they are equal."""
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    step = (hi - lo) / bins
    edges = np.arange(bins + 1, dtype=np.float64) * step + lo
    edges[-1] = hi
    return edges


def histogram_counts(v, bins):
    """The largest i with edge_i <= x, the last bin closed; stated by search, not by np.histogram's arithmetic."""
    edges = histogram_edges(float(v.min()), float(v.max()), bins)
    idx = np.searchsorted(edges, v, side="right") - 1
    idx[idx == bins] = bins - 1
    return np.bincount(idx, minlength=bins).astype(np.int64), edges


def histogram_stats(suv, seg, bins=100, organ_max=7, organs=ORGANS):
    """(results, {organ: (counts, edges)}, {organ: absolute-curve counts})."""
    per_organ, curves, hists, abs_counts = {}, {}, {}, {}
    rel, absolute = np.linspace(0, 1, 50), np.linspace(0, 20, 50)
    for label, name in organs.items():
        v = suv[seg == label] if label <= organ_max else suv[:0]
        if v.size == 0:
            continue
        per_organ[name] = {"mean": float(v.mean()), "std": float(v.std()), "median": float(np.median(v)),
                           "max": float(v.max()), "min": float(v.min())}
        top = v.max()
        curves[name] = [(float(t), np.count_nonzero(v >= top * t) / v.size * 100) for t in rel]
        abs_counts[name] = np.array([np.count_nonzero(v >= a) for a in absolute], dtype=np.int64)
        hists[name] = histogram_counts(v, bins)
    return {"per_organ": per_organ, "threshold_curves": curves}, hists, abs_counts
