from .sliding_window import (blend_argmax_encode, flip_masks, gaussian_tables, sliding_window_accumulate,
                             sliding_window_inference, window_starts)

__all__ = ["blend_argmax_encode", "flip_masks", "gaussian_tables", "sliding_window_accumulate",
           "sliding_window_inference", "window_starts"]
