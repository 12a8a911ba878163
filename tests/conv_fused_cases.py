"""Shared by tests/test_conv_fused_plan_cpu.py and tests/test_conv_fused_gpu.py: the shapes that drive the grouped
(ConvGroup), deferred-norm (mmseg_conv3_fwd_norm), IN-partial data-gradient (mmseg_conv3_dgrad_in) and fused stem
weight-gradient (mmseg_stem_wgrad_inb) kernels, with the kernel, split count and chunk count each shape is there
for.  The expected values were read from the planning queries of the library (csrc/conv_gemm.hip choose_gemm,
csrc/conv_wgrad.hip choose_conv3_wgrad) for bf16; the CPU test re-asks them for every row, so a routing change
shows up without a GPU, and the GPU tests assert the launched name against the same table.

Every fused row needs MMSEG_BRICK2_MINUNITS=0 (BASE_KNOBS): without it these small volumes route to the
runtime-brick kernel.  Shapes are (N, (D, H, W), Cin, Cout); a brick6 brick is 4 x 4 x 16 voxels but the family's
unit is the 4 x 8 x 8 footprint, so a (4, 8, 16) sample holds two bricks."""
BASE_KNOBS = {"MMSEG_BRICK2_MINUNITS": "0"}
KNOBS = ("MMSEG_BRICK2_MINUNITS", "MMSEG_BRICK4_BLOCKS", "MMSEG_BRICKR_SLOTS", "MMSEG_DGRAD_IN_PART",
         "MMSEG_DEFER_CONV_NORM", "MMSEG_GROUP_SMALL", "MMSEG_GROUP_FORCE_R", "MMSEG_BRICK", "MMSEG_BRICK8",
         "MMSEG_WGRAD_DMA", "MMSEG_WGRAD_BRICK")   # every knob the rows' routing depends on

BRICK6 = "conv3_brick6_kernel<BN32>"
BRICK6_INP = "conv3_brick6_kernel<BN32,INP>"
V = (4, 8, 16)


def knobs_of(blocks):
    return dict(BASE_KNOBS, **({"MMSEG_BRICK4_BLOCKS": blocks} if blocks else {}))


# ---------------------------------------------------------------- deferred-norm forward (mmseg_conv3_fwd_norm)
# (N, vol, Cin, Cout, MMSEG_BRICK4_BLOCKS or None, kernel of the PLAIN forward of the same shape).  All norm_ok in
# bf16, the norm forward is BRICK6.  With 3 samples of two bricks each: 1 block walks all three samples, 2 blocks of
# 3 bricks straddle sample 1, 4 -> 3 blocks of one sample each; 5 samples over 4 blocks: 3 + 3 + 3 + 1 bricks, every
# block but the last straddles.  32 -> 64 / 96: 2 / 3 column tiles (the plain 96-column forward takes 48-column
# brick2 tiles instead).
NORM_ROWS = [
    (3, V, 32, 32, None, BRICK6), (3, V, 32, 32, "1", BRICK6), (3, V, 32, 32, "2", BRICK6), (3, V, 32, 32, "4", BRICK6),
    (5, V, 32, 32, "4", BRICK6),
    (1, V, 32, 32, None, BRICK6),
    (2, (8, 8, 16), 32, 32, None, BRICK6),
    (2, V, 32, 64, None, BRICK6),
    (2, V, 32, 96, None, "conv3_brick2_kernel<BN48,ZW1>"),
]
# shapes the deferred norm refuses: two input chunks; W % 16 != 0
NORM_REFUSED = [(3, V, 64, 32, None), (3, (4, 8, 8), 32, 32, None)]

# ------------------------------------------------------ data gradient with IN-backward partials (conv3_dgrad_in)
# (N, vol, Cin, Cout, MMSEG_BRICK4_BLOCKS or None, chunks = blocks per column tile).  The data gradient of Cin -> Cout
# has Cin columns: the 64 -> 32 rows run two column tiles.
INP_ROWS = [
    (3, V, 32, 32, None, 6), (3, V, 32, 32, "1", 1), (3, V, 32, 32, "2", 2), (3, V, 32, 32, "4", 3),
    (3, V, 32, 32, "7", 6),
    (5, V, 32, 32, "4", 4),
    (1, V, 32, 32, None, 2),
    (2, (8, 8, 16), 32, 32, None, 8),
    (3, V, 64, 32, None, 6), (3, V, 64, 32, "4", 2), (3, V, 64, 32, "7", 3),
]
# data gradients with two input chunks: not the INP kernel (in_chunks 0), (N, vol, Cin, Cout, kernel that runs)
INP_REFUSED = [(2, V, 32, 64, "conv3_brick3_kernel<BN32>"), (2, V, 32, 96, "conv3_brick3_kernel<BN32>")]

# ---------------------------------------------------------------------------------- grouped launches (ConvGroup)
# (G, N = G x n samples, vol, Cin, Cout, knobs, forward kernel, splits, data-gradient kernel, splits,
#  weight-gradient kernel, weight-gradient splits over all groups; 0: one split per group, the kernel writes the
#  gradient itself).  The two 16^3 rows are the smallest shapes at which the 64-column rule of the runtime-brick
#  conv holds (bricks x Ncols / 64 >= 256): the dominant family of the dual-encoder step.
R32, R32K, R64 = "conv3_brickr_kernel<BN32>", "conv3_brickr_kernel<BN32,KW2>", "conv3_brickr_kernel<BN64>"
GROUP_ROWS = [
    (2, 4, (6, 6, 6), 64, 64, {}, R32, 2, R32, 2, "wgrad_brickr_kernel<CO64,V3>", 0),
    (2, 4, (6, 6, 6), 128, 64, {"MMSEG_BRICKR_SLOTS": "16"}, R32K, 2, R32K, 1, "wgrad_brickr_kernel<CO64,V3>", 0),
    (2, 4, (12, 12, 12), 64, 64, {}, R32, 2, R32, 2, "wgrad_brickr_kernel<CO64,V3>", 16),
    (2, 6, (8, 8, 8), 32, 32, {}, R32, 1, R32, 1, "wgrad_brickr_kernel<CO32,B448>", 6),
    (3, 6, (8, 8, 8), 32, 32, {}, R32, 1, R32, 1, "wgrad_brickr_kernel<CO32,B448>", 6),
    (2, 4, (8, 8, 16), 32, 64, {}, R32, 1, R32, 2, "wgrad_brickr_kernel<CO64,B448>", 8),
    (2, 4, (5, 6, 6), 64, 64, {}, R32, 2, R32, 2, "wgrad_brickr_kernel<CO64>", 0),
    (2, 4, (16, 16, 16), 32, 256, {}, R64, 1, R32, 4, "wgrad_brickr_kernel<CO64,B448>", 32),
    (2, 4, (16, 16, 16), 256, 32, {}, R32, 4, R64, 1, "wgrad_brickr_kernel<CO32,B448>", 32),
]

# ------------------------------------------------------- stem weight gradient with the fused norm backward
# (cr real input channels, Co, (N, D, H, W)): one 4 x 8 x 8 brick per sample; one sample of 4 bricks; 3 samples of
# two bricks.  STEM_DIRECT: 3 bricks over mmseg_stem_wgrad_splits(.., 2) = 2 splits, a ragged last split.
STEM_SHAPES = [(2, 4, 8, 8), (1, 8, 16, 8), (3, 4, 8, 16)]
STEM_ROWS = [(cr, co, shape) for cr in (1, 2, 4) for co in (16, 32) for shape in STEM_SHAPES]
STEM_DIRECT = (2, 32, (3, 4, 8, 8), 2)

# ------------------------------------- tests/test_kernels_gpu.py::test_conv3_kernel_variants, row by row
# (knobs, Cin, Cout, (N, D, H, W)) -> {dtype code: (forward kernel, data-gradient kernel, weight-gradient kernel)},
# dtype code 0 fp32 / 1 bf16 (fp32 ignores most knobs), under MMSEG_BRICK2_MINUNITS=0 and the row's knobs.
B2_32, B2_64 = "conv3_brick2_kernel<BN32,ZW1>", "conv3_brick2_kernel<BN64,ZW1>"
B3, B4, B8_32, B8_64 = ("conv3_brick3_kernel<BN32>", "conv3_brick4_kernel<BN32>", "conv3_brick8_kernel<BN32>",
                        "conv3_brick8_kernel<BN64>")
GEMM64, GEMM32 = "conv_gemm_kernel<conv3,128x64>", "conv_gemm_kernel<conv3,128x32>"
B1_64 = "conv3_brick_kernel<BN64>"
WB, WG, WD32, WD64, WROW = ("wgrad_brick_kernel", "wgrad_kernel<conv3>", "wgrad_dma_kernel<CO32>",
                            "wgrad_dma_kernel<CO64>", "wgrad_row_kernel<CO32>")
WB2_32, WB2_64 = "wgrad_brick2_kernel<CO32,V3>", "wgrad_brick2_kernel<CO64,V3>"
WR32, WR64 = "wgrad_brickr_kernel<CO32,V3>", "wgrad_brickr_kernel<CO64,V3>"
B8K = {"MMSEG_BRICK8": "2", "MMSEG_BRICK8_MINBLK": "0"}
VARIANTS = [
    # brick v2 variants (kernel choice is by grid size; the knobs force each one on a small grid)
    ({"MMSEG_BRICK2_MINBLK": "0"}, 64, 64, (2, 8, 16, 8),   # BN64 ZW1
     {0: (B2_64, B2_64, WB), 1: (B2_64, B2_64, WD64)}),
    ({"MMSEG_BRICK2_MINBLK": "0"}, 32, 128, (1, 4, 8, 16),   # BN64 ZW1, 2 column tiles
     {0: (B2_64, B2_32, WB), 1: (B2_64, B3, WD64)}),
    # brick v3 (bf16 BN32 default; f32 takes v2): persistent blocks over several bricks / column tiles
    ({"MMSEG_BRICK3_BLOCKS": "3"}, 64, 128, (1, 4, 16, 16),   # 4 col tiles x 4 bricks, ragged ranges
     {0: (B2_32, B2_32, WB), 1: (B3, B3, WD64)}),
    ({"MMSEG_BRICK3_BLOCKS": "0"}, 64, 32, (1, 12, 8, 24),   # one unit per block, border (2 chunks)
     {0: (B2_32, B2_32, WB), 1: (B3, B4, WD32)}),
    # brick v4 (bf16, Cin 32, W % 16 != 0, register-resident weights, double-buffered halo; f32 takes v2)
    ({"MMSEG_BRICK4_BLOCKS": "3"}, 32, 32, (2, 8, 16, 8),   # 8 bricks over 3 blocks, ragged ranges
     {0: (B2_32, B2_32, WB), 1: (B4, B4, WD32)}),
    ({"MMSEG_BRICK4_BLOCKS": "4"}, 32, 64, (1, 4, 16, 8),   # 2 column tiles x 2 blocks each
     {0: (B2_32, B2_32, WB), 1: (B4, B3, WD64)}),
    ({}, 32, 32, (1, 12, 8, 24),   # one brick per block, border bricks
     {0: (B2_32, B2_32, WB), 1: (B4, B4, WD32)}),
    # brick v6 (bf16, Cin 32, W % 16 == 0: 4x4x16 bricks, ky-shared A fragments, the staging interleaved between
    # the MFMAs)
    ({"MMSEG_BRICK4_BLOCKS": "1"}, 32, 32, (2, 8, 16, 16),   # one block over all 16 bricks of 2 samples
     {0: (B2_32, B2_32, WB), 1: (BRICK6, BRICK6, WD32)}),
    ({"MMSEG_BRICK4_BLOCKS": "3"}, 32, 32, (2, 8, 8, 32),   # 16 bricks over 3 blocks, ragged ranges
     {0: (B2_32, B2_32, WB), 1: (BRICK6, BRICK6, WROW)}),
    ({}, 32, 32, (1, 12, 16, 48),   # border bricks on every side (3 x 4 x 3 bricks)
     {0: (B2_32, B2_32, WB), 1: (BRICK6, BRICK6, WD32)}),
    ({"MMSEG_BRICK4_BLOCKS": "4"}, 32, 64, (1, 4, 8, 32),   # 2 column tiles
     {0: (B2_32, B2_32, WB), 1: (BRICK6, B3, WD64)}),
    ({"MMSEG_BRICK4_BLOCKS": "1"}, 32, 32, (2, 4, 8, 16),   # one block over both samples (two bricks each)
     {0: (B2_32, B2_32, WB), 1: (BRICK6, BRICK6, WD32)}),
    ({}, 128, 32, (1, 4, 16, 8),   # 4 input chunks: BN32 ZW1 in f32, brick v3 in bf16
     {0: (B2_32, B2_32, WB), 1: (B3, B4, WD32)}),
    # runtime brick: 12^3 and 6^3 both take the compile-time 6x6x6 brick (a tie with (3, 6, 12) goes to the smaller
    # halo); bf16 with >= 2 chunks per split runs the in-block K split over two 256-thread halves (KW2)
    ({}, 256, 128, (2, 12, 12, 12),   # chunk split-K, 4 / 2 splits
     {0: (R32, R32, WG), 1: (R32K, R32K, WR64)}),
    ({}, 512, 256, (1, 6, 6, 6),   # 16 chunks over 16 splits (one each: no KW2)
     {0: (R32, R32, WG), 1: (R32, R32, WR64)}),
    ({}, 256, 256, (4, 12, 12, 12),   # the grouped 12^3 shape (N = M x B = 4)
     {0: (R32, R32, WG), 1: (R32K, R32K, WR64)}),
    ({"MMSEG_BRICKR_SLOTS": "6"}, 256, 32, (2, 6, 6, 6),   # 8 chunks over 3 splits: 3 (2 + 1), 3, 2
     {0: (R32, R32, WG), 1: (R32K, R32, WR32)}),
    ({"MMSEG_BRICKR_SLOTS": "1"}, 128, 32, (2, 6, 6, 6),   # 4 chunks in one split
     {0: (R32, R32, WG), 1: (R32K, R32, WR32)}),
    ({"MMSEG_WGRAD_BRICK": "1"}, 64, 128, (2, 4, 8, 8),   # v1 brick wgrad (32 co per block)
     {0: (B2_32, B2_32, WB), 1: (B3, B3, WB)}),
    ({"MMSEG_WGRAD_BRICK": "0"}, 64, 64, (1, 4, 8, 8),   # generic wgrad
     {0: (B2_32, B2_32, WG), 1: (B3, B3, WG)}),
    # v2 brick wgrad, register-staged (bf16 with MMSEG_WGRAD_DMA=0; f32 takes the v1 brick wgrad)
    ({"MMSEG_WGRAD_DMA": "0"}, 32, 128, (1, 8, 4, 16),   # 2 row tiles of 64 co
     {0: (R32, R32, WB), 1: (R32, R32, WB2_64)}),
    ({"MMSEG_WGRAD_DMA": "0"}, 64, 32, (2, 4, 4, 16),   # 32 co per block
     {0: (R32, R32, WB), 1: (R32, R32, WB2_32)}),
    # v2 brick wgrad with LDS-DMA staging (the bf16 default; f32 keeps the register-staged kernel): 3-stage ring,
    # border halos, ragged brick ranges over the splits
    ({"MMSEG_WGRAD_DMA": "1"}, 32, 128, (1, 8, 4, 16),   # 64 co, 2 row tiles
     {0: (R32, R32, WB), 1: (R32, R32, WD64)}),
    ({"MMSEG_WGRAD_DMA": "1"}, 64, 32, (2, 4, 4, 16),   # 32 co, 2 input chunks
     {0: (R32, R32, WB), 1: (R32, R32, WD32)}),
    ({"MMSEG_WGRAD_DMA": "1"}, 32, 32, (2, 12, 8, 24),   # 32 co, 36 bricks
     {0: (B2_32, B2_32, WB), 1: (B4, B4, WD32)}),
    ({"MMSEG_WGRAD_DMA": "1"}, 64, 64, (1, 8, 12, 16),   # 64 co, 24 bricks
     {0: (R32, R32, WB), 1: (R32, R32, WD64)}),
    # MMSEG_BRICK = 1 / 0 on a small volume: the per-lane gather GEMM with 13 K splits (the v1 brick rows are at
    # the end of the table)
    ({"MMSEG_BRICK": "1"}, 64, 64, (2, 8, 8, 8),   # gather GEMM, split-K
     {0: (GEMM64, GEMM64, WB), 1: (GEMM64, GEMM64, WD64)}),
    ({"MMSEG_BRICK": "0"}, 64, 64, (2, 8, 8, 8),   # per-lane gather GEMM
     {0: (GEMM64, GEMM64, WB), 1: (GEMM64, GEMM64, WD64)}),
    # brick v8 (bf16; f32 ignores the knob): 8 waves over an 8x8x8 brick, LDS-DMA halo + double-buffered weights
    (B8K, 64, 64, (2, 8, 16, 8),   # 2 chunks (halo refill)
     {0: (B2_32, B2_32, WB), 1: (B8_64, B8_64, WD64)}),
    (B8K, 32, 64, (1, 16, 8, 24),   # 1 chunk, border bricks
     {0: (B2_32, B2_32, WB), 1: (B8_64, B8_32, WD64)}),
    (B8K, 128, 128, (1, 8, 8, 16),   # 4 chunks, 2 column tiles
     {0: (B2_32, B2_32, WB), 1: (B8_64, B8_64, WD64)}),
    (B8K, 64, 32, (1, 16, 8, 16),   # BN32: 2 planes per wave
     {0: (B2_32, B2_32, WB), 1: (B8_32, B8_64, WD32)}),
    (B8K, 128, 32, (2, 16, 16, 8),   # BN32, 4 chunks, border
     {0: (B2_32, B2_32, WB), 1: (B8_32, B8_64, WD32)}),
    # the shapes four rows above had before they were moved onto the kernels their comments name: H % 8 != 0 keeps
    # them off the 4 x 8 x 8 family, so they run the runtime-brick conv on a non-cubic brick
    ({}, 32, 32, (1, 12, 12, 16),   # border on every side
     {0: (R32, R32, WB), 1: (R32, R32, WD32)}),
    ({"MMSEG_BRICK4_BLOCKS": "4"}, 32, 64, (1, 4, 4, 32),   # 2 column tiles, 2 data-gradient splits
     {0: (R32, R32, WB), 1: (R32, R32, WD64)}),
    ({"MMSEG_BRICK4_BLOCKS": "1"}, 32, 32, (2, 4, 4, 16),   # 256 voxels per sample
     {0: (R32, R32, WB), 1: (R32, R32, WD32)}),
    # row 5's shape before it moved onto brick v4: brick v6 forward with 2 column tiles x 2 blocks at W = 16
    ({"MMSEG_BRICK4_BLOCKS": "4"}, 32, 64, (1, 4, 8, 16),
     {0: (B2_32, B2_32, WB), 1: (BRICK6, B3, WD64)}),
    # v1 brick (MMSEG_BRICK=1; 4 x 4 x 8 bricks): it needs ksplit 1, and the split query asks for splits below 512
    # (128-voxel x 64-column) tiles, so 16,384 voxels x 256 columns are the smallest launch that takes it -- the
    # forward of 32 -> 256 and the data gradient of 256 -> 32 (the other direction has 32 columns: gather GEMM)
    ({"MMSEG_BRICK": "1"}, 32, 256, (1, 16, 32, 32),   # v1 brick forward, 4 column tiles, 1 chunk
     {0: (B1_64, GEMM32, WB), 1: (B1_64, GEMM32, WD64)}),
    ({"MMSEG_BRICK": "1"}, 256, 32, (1, 16, 32, 32),   # v1 brick data gradient, 4 column tiles, 1 chunk
     {0: (GEMM32, B1_64, WB), 1: (GEMM32, B1_64, WROW)}),
]


def variant_names(knobs, cin, cout, shape):
    for k, ci, co, sh, names in VARIANTS:
        if (k, ci, co, sh) == (knobs, cin, cout, tuple(shape)):
            return names
    raise KeyError((knobs, cin, cout, shape))
