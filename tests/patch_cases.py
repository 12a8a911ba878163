"""The affine cases shared by tests/test_patch_cpu.py (restatement against scipy) and tests/test_patch_gpu.py
(kernel against restatement): a 13 x 11 x 18 volume, an 8 x 6 x 10 patch turned by (10, -15, 7) degrees and
scaled by 0.9 and 1.1, at starts that leave part of the patch outside the volume."""
import numpy as np

from tests import patch_ref as PR

VOLUME = (13, 11, 18)
PATCH = (8, 6, 10)
ANGLES = (10.0, -15.0, 7.0)
SCALES = (0.9, 1.1)
STARTS = ((3, 4, 10), (-2, -1, 2))        # past the far end of W; before the near end of D and H
PAD = (0.75, -1.5)


def volume():
    rng = np.random.Generator(np.random.PCG64(7))
    image = rng.standard_normal((2,) + VOLUME, dtype=np.float32)
    label = rng.integers(0, 5, size=VOLUME).astype(np.int64)
    return image, label


def affine_cases():
    """(start, M) per case."""
    return [(start, PR.rotation_scale_matrix(ANGLES, s)) for s in SCALES for start in STARTS]
