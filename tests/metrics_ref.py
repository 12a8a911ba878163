"""numpy restatement of the reference's boundary metric (src/trainer/metrics.py:110-162), the checker of the
metric tests.  No scipy: the distance transform is the O(V^2) pairwise brute force -- for every voxel the minimum
over the foreground voxels of ((dh s0)^2 + (dw s1)^2) + (dd s2)^2, summed over the axes in order as scipy sums
its per-axis squares, then one sqrt.  At unit spacing every candidate is an exactly representable integer, so the
result equals scipy's bit for bit; at other spacings two candidates that tie in exact arithmetic may differ by a
few ulp."""
import numpy as np


def edt(fg, spacing=(1.0, 1.0, 1.0), chunk=512):
    """Distance of every voxel of a [H, W, D] boolean mask to its nearest foreground voxel (fp64); +inf
    everywhere when there is none (scipy's result is then not meaningful and the reference skips the sample)."""
    fg = np.asarray(fg, dtype=bool)
    out = np.full(fg.shape, np.inf)
    pts = np.argwhere(fg).astype(np.float64)
    if len(pts) == 0:
        return out
    sp = np.asarray(spacing, dtype=np.float64)
    vox = np.argwhere(np.ones(fg.shape, dtype=bool)).astype(np.float64)
    flat = out.reshape(-1)
    for i in range(0, len(vox), chunk):
        d = (vox[i:i + chunk, None, :] - pts[None, :, :]) * sp
        d *= d
        flat[i:i + chunk] = np.sqrt(((d[..., 0] + d[..., 1]) + d[..., 2]).min(axis=1))
    return out


def border(fg):
    """m ^ np.roll(m, 1, axis=0): row 0 is compared with row H - 1 (metrics.py:142-143)."""
    fg = np.asarray(fg, dtype=bool)
    return fg ^ np.roll(fg, 1, axis=0)


def sample_distances(pred, target, spacing=(1.0, 1.0, 1.0)):
    """The concatenated border distances of one sample, or None where the reference skips it."""
    p, t = np.asarray(pred) > 0, np.asarray(target) > 0
    if p.sum() == 0 or t.sum() == 0:
        return None
    both = np.concatenate([edt(t, spacing)[border(p)], edt(p, spacing)[border(t)]])
    return both if len(both) else None


def hausdorff(updates, percentile=95):
    """(distances, compute()) of HausdorffDistance(percentile) after update(pred, target, spacing) for every
    (pred [B, H, W, D], target, spacing) of `updates`."""
    distances = []
    for pred, target, spacing in updates:
        for b in range(len(pred)):
            d = sample_distances(pred[b], target[b], spacing if spacing is not None else (1.0, 1.0, 1.0))
            if d is not None:
                distances.append(np.percentile(d, percentile))
    if not distances:
        return distances, {"hausdorff_distance": float("inf")}
    return distances, {"hausdorff_distance": np.mean(distances), "hausdorff_distance_std": np.std(distances)}


def confusion(pred, target, num_classes):
    """matrix[t, p] += 1 over the flattened masks (metrics.py:192-196)."""
    m = np.zeros((num_classes, num_classes), dtype=np.int64)
    np.add.at(m, (np.asarray(target).reshape(-1).astype(np.int64), np.asarray(pred).reshape(-1).astype(np.int64)), 1)
    return m
