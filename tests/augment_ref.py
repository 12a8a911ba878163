"""numpy restatement of "apply AugmentParams" (data/augment.py), the checker of the augmentation tests:
np.flip on each flagged axis of the input, np.rot90(k) over the first two spatial axes (transforms.py:44-80),
the per-channel affine in two float32 roundings as the reference's numpy computes `image[c] * scale + shift`
(transforms.py:114), and the noise from oracle/data_oracle.py's SplitMix64 normal stream, element e = the
linear index into the output over all channels."""
import numpy as np

from oracle import data_oracle as DO


def apply_geometry(vol, flip, k, first_axis):
    """flip: 3 bools for the spatial axes; first_axis: 1 for a [C, D, H, W] image, 0 for a [D, H, W] label."""
    for ax in range(3):
        if flip[ax]:
            vol = np.flip(vol, axis=first_axis + ax)
    return np.ascontiguousarray(np.rot90(vol, k=k, axes=(first_axis, first_axis + 1)))


def apply_params(image, label, p, noise=None):
    """(image', label') of AugmentParams p on a float32 [C, D, H, W] image and an optional [D, H, W] label.
    noise: override p.noise (False = the reference's output before RandomGaussianNoise)."""
    img = apply_geometry(image.astype(np.float32), p.flip, p.k, 1)
    lab = None if label is None else apply_geometry(label, p.flip, p.k, 0)
    if p.scale is not None:
        for c in range(img.shape[0]):
            scaled = (img[c] * np.float32(p.scale[c])).astype(np.float32)       # rounding 1
            img[c] = (scaled + np.float32(p.shift[c])).astype(np.float32)       # rounding 2
    if p.noise if noise is None else noise:
        n = DO.normal_stream(int(p.noise_key), img.size).reshape(img.shape)
        sd = float(np.float32(p.noise_sd))
        img = (img + (float(p.noise_mean) + sd * n).astype(np.float32)).astype(np.float32)
    return img, lab
