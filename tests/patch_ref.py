"""fp64 numpy restatement of the patch sampler (csrc/patch.hip): the pick rule of mmseg_patch_pick and both
paths of mmseg_patch_sample, with the kernels' expression order, so that the GPU tests can ask for the same bits.

numpy evaluates every elementwise product and sum as one rounded operation, which is what the kernels do with
floating-point contraction switched off (no fused multiply-add).
"""
from __future__ import annotations

import numpy as np


def pick_start(label, size, mode, u, fallback):
    """The crop start of one patch of `size` out of label [D, H, W] (see mmseg_patch_pick)."""
    n_ax = label.shape
    st = [int(v) for v in fallback]
    if mode == 1:
        fg = np.flatnonzero(label.reshape(-1) > 0)
        n = int(fg.size)
        if n > 0:
            k = min(int(np.floor(np.float64(u) * np.float64(n))), n - 1)
            v = np.unravel_index(int(fg[k]), n_ax)
            for a in range(3):
                if n_ax[a] >= size[a]:
                    st[a] = min(max(int(v[a]) - size[a] // 2, 0), n_ax[a] - size[a])
    for a in range(3):
        if n_ax[a] < size[a]:
            st[a] = -((size[a] - n_ax[a]) // 2)
    return st


def sample_copy(image, label, start, size, pad):
    """dst[o] = src[start + o]; pad[c] (labels: 0) outside the volume."""
    C = image.shape[0]
    out = np.empty((C,) + tuple(size), dtype=np.float32)
    for c in range(C):
        out[c] = np.float32(pad[c])
    lab = None if label is None else np.zeros(tuple(size), dtype=label.dtype)
    src, dst = [], []
    for a in range(3):
        lo, hi = max(start[a], 0), min(start[a] + size[a], image.shape[1 + a])
        if hi <= lo:
            return out, lab
        src.append(slice(lo, hi))
        dst.append(slice(lo - start[a], hi - start[a]))
    out[(slice(None),) + tuple(dst)] = image[(slice(None),) + tuple(src)]
    if label is not None:
        lab[tuple(dst)] = label[tuple(src)]
    return out, lab


def coords(start, size, M):
    """p [3][pd][ph][pw] fp64: p_a = ((M[a][0] q_0 + M[a][1] q_1) + M[a][2] q_2) + c_a with q = o - (P - 1) / 2
    and c = start + (P - 1) / 2."""
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    half = [np.float64(s - 1) * 0.5 for s in size]
    q = np.meshgrid(*[np.arange(s, dtype=np.float64) - h for s, h in zip(size, half)], indexing="ij")
    return np.stack([((M[a, 0] * q[0] + M[a, 1] * q[1]) + M[a, 2] * q[2]) + (np.float64(start[a]) + half[a])
                     for a in range(3)])


def sample_affine_image(image, start, size, M, pad, dtype=np.float32):
    """Trilinear over the 8 corners of floor(p), a corner outside contributing pad[c]; z, then y, then x as
    a * w0 + b * w1 in fp64; one rounding to fp32 (dtype=np.float64: the sum before that rounding)."""
    C, n_ax = image.shape[0], image.shape[1:]
    p = coords(start, size, M)
    fl = np.floor(p)
    t = p - fl
    w1, w0 = t, 1.0 - t
    i0 = [np.clip(fl[a], -2, n_ax[a]).astype(np.int64) for a in range(3)]
    out = np.empty((C,) + tuple(size), dtype=dtype)
    for c in range(C):
        vol = image[c].astype(np.float64)
        padv = np.float64(np.float32(pad[c]))

        def at(dz, dy, dx):
            z, y, x = i0[0] + dz, i0[1] + dy, i0[2] + dx
            ok = (z >= 0) & (z < n_ax[0]) & (y >= 0) & (y < n_ax[1]) & (x >= 0) & (x < n_ax[2])
            v = vol[np.clip(z, 0, n_ax[0] - 1), np.clip(y, 0, n_ax[1] - 1), np.clip(x, 0, n_ax[2] - 1)]
            return np.where(ok, v, padv)

        vy = [[at(0, i, j) * w0[0] + at(1, i, j) * w1[0] for j in range(2)] for i in range(2)]
        vx0 = vy[0][0] * w0[1] + vy[1][0] * w1[1]
        vx1 = vy[0][1] * w0[1] + vy[1][1] * w1[1]
        out[c] = (vx0 * w0[2] + vx1 * w1[2]).astype(dtype)
    return out


def label_ties(start, size, M, tol=1e-9):
    """Mask of the output voxels where some p_a + 0.5 lies within tol of an integer."""
    h = coords(start, size, M) + 0.5
    return (np.abs(h - np.round(h)) <= tol).any(axis=0)


def sample_affine_label(label, start, size, M):
    """The voxel at floor(p_a + 0.5) per axis, 0 outside."""
    n_ax = label.shape
    f = np.floor(coords(start, size, M) + 0.5)
    ok = np.ones(tuple(size), dtype=bool)
    idx = []
    for a in range(3):
        ok &= (f[a] >= 0) & (f[a] < n_ax[a])
        idx.append(np.clip(f[a], 0, n_ax[a] - 1).astype(np.int64))
    return np.where(ok, label[idx[0], idx[1], idx[2]], 0).astype(label.dtype)


def rotation_scale_matrix(angles_deg, scale):
    """M = Rz Ry Rx / s as mmseg_amd.data.patch.affine_matrix builds it, restated: Rx turns the (1, 2) plane
    about array axis 0, Ry the (2, 0) plane about axis 1, Rz the (0, 1) plane about axis 2."""
    ax, ay, az = [np.deg2rad(np.float64(v)) for v in angles_deg]
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=np.float64)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=np.float64)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=np.float64)
    return (Rz @ Ry @ Rx) / np.float64(scale)
