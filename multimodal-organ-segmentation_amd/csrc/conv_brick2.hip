// The 4 x 8 x 8-brick 3^3 conv family: conv3_brick_kernel (the first generation, 4 x 4 x 8 bricks) and
// conv3_brick2_kernel / conv3_brick3_kernel / conv3_brick4_kernel, which share Brick2Layout and the halo / weight
// staging, with their launcher.
#include "conv_common.h"

namespace {

// ------------------------------------------------------ brick conv (3^3)
// LDS-staged halo tiles for the 3x3x3 convolution (fwd, and dgrad with the
// flipped / transposed weights): a block owns a 4x4x8 output brick (128
// voxels, one sample) x BN output channels.  Per 32-channel input chunk the
// 6x6x10 input halo is staged ONCE into LDS and reused by all 27 taps (the
// per-lane gather kernel above re-reads it 27x through L1/L2), and the chunk's
// weights are staged one kz-plane (9 taps) at a time.  Register prefetch of
// the next stage overlaps its global loads with the current MFMAs.
// Wave w computes brick z-slice w (32 voxels = 2 row tiles) x BN columns.
template <typename T, int BN>
__global__ __launch_bounds__(256) void conv3_brick_kernel(GemmArgs g) {
  constexpr int EP = 16 / sizeof(T);
  constexpr int XP = CK + EP;                   // halo row pitch (elements)
  constexpr int WP = CK;                        // weight row pitch (elements)
  constexpr int RN = BN / 16;
  constexpr int XS = HLO_V * XP, WS = 9 * BN * WP;
  __shared__ __attribute__((aligned(16))) T lds[XS + WS];
  T* Xl = lds;
  T* Wl = lds + XS;
  constexpr int X_ITEMS = HLO_V * (CK / 8);     // V8 loads per halo stage
  constexpr int X_PER = (X_ITEMS + 255) / 256;
  constexpr int W_ITEMS = 9 * BN * (CK / 8);
  constexpr int W_PER = (W_ITEMS + 255) / 256;

  const T* A = reinterpret_cast<const T*>(g.a);
  const T* Bw = reinterpret_cast<const T*>(g.b);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bz_n = g.D / BRK_Z, by_n = g.H / BRK_Y, bx_n = g.W / BRK_X;
  const int nbrick = (g.M / (g.D * g.H * g.W)) * bz_n * by_n * bx_n;
  const int nt_n = (g.Ncols + BN - 1) / BN;
  const int tile = g.swz ? xcd_swizzle(blockIdx.x, nbrick * nt_n) : (int)blockIdx.x;
  int bidx = tile % nbrick;
  const int nt = tile / nbrick;
  const int bx = bidx % bx_n; bidx /= bx_n;
  const int by = bidx % by_n; bidx /= by_n;
  const int bz = bidx % bz_n;
  const int n = bidx / bz_n;
  const int z0 = bz * BRK_Z, y0 = by * BRK_Y, x0 = bx * BRK_X;
  const long long HW = (long long)g.H * g.W;
  const long long nbase = (long long)n * g.D * HW;
  const int n0 = nt * BN;
  const int cin = 8 << g.cpg_shift;             // channels of the A source
  const int nchunk = gemm_nchunk(g);
  const int nstage = nchunk * 3;

  V8<T> xr[X_PER], wr[W_PER];
  auto load_x = [&](int c) {
#pragma unroll
    for (int k = 0; k < X_PER; ++k) {
      const int e = tid + k * 256;
      if (e < X_ITEMS) {
        const int h = e >> 2, cg = e & 3;
        const int hx = h % HLO_X, hy = (h / HLO_X) % HLO_Y, hz = h / (HLO_X * HLO_Y);
        const int z = z0 - 1 + hz, y = y0 - 1 + hy, x = x0 - 1 + hx;
        if ((unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H && (unsigned)x < (unsigned)g.W)
          xr[k].load(A + (nbase + z * HW + (long long)y * g.W + x) * g.lda + c * CK + cg * 8);
        else
          xr[k].zero();
      }
    }
  };
  auto load_w = [&](int c, int kz) {
#pragma unroll
    for (int k = 0; k < W_PER; ++k) {
      const int e = tid + k * 256;
      if (e < W_ITEMS) {
        const int cg = e & 3, q = e >> 2;
        const int col = q % BN, t9 = q / BN;
        const int tap = kz * 9 + t9;
        const int kgi = tap * (cin / 8) + c * 4 + cg;
        wr[k].load(Bw + ((long long)kgi * g.Cpad + n0 + col) * 8);
      }
    }
  };
  auto store_x = [&]() {
#pragma unroll
    for (int k = 0; k < X_PER; ++k) {
      const int e = tid + k * 256;
      if (e < X_ITEMS) xr[k].store(Xl + (e >> 2) * XP + (e & 3) * 8);
    }
  };
  auto store_w = [&]() {
#pragma unroll
    for (int k = 0; k < W_PER; ++k) {
      const int e = tid + k * 256;
      if (e < W_ITEMS) {
        const int cg = e & 3, q = e >> 2;   // q = t9*BN + col
        wr[k].store(Wl + q * WP + cg * 8);
      }
    }
  };

  f32x4 acc[2][RN];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // lane's rows: row r = lane&15 of tile i -> brick voxel (wave, 2i + (r>>3), r&7)
  const int r16 = lane & 15, kg = lane >> 4;
  int hrow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) hrow[i] = (wave * HLO_Y + (2 * i + (r16 >> 3))) * HLO_X + (r16 & 7);

  load_x(0);
  load_w(0, 0);
  store_x();
  store_w();
  __syncthreads();
  for (int st = 0; st < nstage; ++st) {
    const int c = st / 3, kz = st - c * 3;
    const int sn = st + 1;
    const bool more = sn < nstage;
    const int cn = sn / 3, kzn = sn - cn * 3;
    if (more) {
      load_w(cn, kzn);
      if (kzn == 0) load_x(cn);
    }
#pragma unroll
    for (int t9 = 0; t9 < 9; ++t9) {
      const int ky = t9 / 3, kx = t9 - ky * 3;
      const int hoff = (kz * HLO_Y + ky) * HLO_X + kx;
      V8<T> af[2], bf[RN];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i].load(Xl + (hrow[i] + hoff) * XP + kg * 8);
#pragma unroll
      for (int j = 0; j < RN; ++j) bf[j].load(Wl + (t9 * BN + j * 16 + r16) * WP + kg * 8);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j) mfma_step<T>(acc[i][j], af[i], bf[j]);
    }
    __syncthreads();
    if (more) {
      store_w();
      if (kzn == 0) store_x();
      __syncthreads();
    }
  }

  T* O = reinterpret_cast<T*>(g.out);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) {
      const int col = n0 + j * 16 + r16;
      if (col >= g.Ncols) continue;
      const float bv = g.bias ? g.bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = kg * 4 + r;            // 0..15 within the tile
        const int y = y0 + 2 * i + (row >> 3), x = x0 + (row & 7), z = z0 + wave;
        const long long vox = nbase + z * HW + (long long)y * g.W + x;
        *out_at<T>(g, vox, col) = from_f<T>(acc[i][j][r] + bv);
      }
    }
}

// ------------------------------------------------- brick conv v2 (3^3)
// Same algorithm as conv3_brick_kernel with a 2x larger per-wave tile and
// bank-conflict-free LDS images:
//   * block = (4*ZW) x 8 x 8 output voxels x BN columns; wave w owns z-slices
//     [w*ZW, (w+1)*ZW) = 4*ZW row tiles of 16 voxels (two 8-voxel x-rows each),
//     so one B fragment feeds 4*ZW MFMAs and one A fragment feeds BN/16;
//   * halo image: 32 channels of a voxel = 4 consecutive 16-B quads, y-rows
//     padded to 42 quads.  A ds_read_b128 lane group then touches 16 distinct
//     bank quads for every tap shift (checked exhaustively on the host for
//     the lane groups of MI355X_MICROARCH.md §LDS);
//   * weight image: rows of 4 quads, quad index XOR-swizzled by bit 3 of the
//     column, which makes the 16-lane groups conflict-free as well;
//   * epilogue staged through LDS so every lane stores 16-B vectors.
// B32: the halo is staged with 32-bit offset buffer loads whose out-of-volume lanes read zeros (host: the A tensor
// spans < 2^31 bytes), instead of 64-bit address arithmetic and a bounds branch per item.
template <typename T, int BN, int ZW, bool PF = false, bool B32 = false>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 2 : 1) void conv3_brick2_kernel(GemmArgs g) {
  PROBE_BLOCK(false);
  PROBE_DECL();
  using L = Brick2Layout<T>;
  constexpr int BZ = 4 * ZW, HZ = BZ + 2;
  constexpr int RM = 4 * ZW, RN = BN / 16;
  constexpr int XQ = HZ * L::RZ;                      // halo quads
  constexpr int WQ = 9 * BN * L::QV;                  // weight quads (one kz plane)
  constexpr int EQ = (BZ * 64 * BN * (int)sizeof(T) + 15) / 16;   // epilogue tile quads
  constexpr int LQ = (XQ + WQ) > EQ ? (XQ + WQ) : EQ;
  __shared__ __attribute__((aligned(16))) float4 lds4[LQ];
  T* Xl = reinterpret_cast<T*>(lds4);
  T* Wl = reinterpret_cast<T*>(lds4 + XQ);
  constexpr int EPQ = 16 / sizeof(T);                 // elements per quad
  constexpr int HV = HZ * H2_Y * H2_X;
  constexpr int X_ITEMS = HV * 4;                     // 8-channel groups per halo stage
  constexpr int X_PER = (X_ITEMS + 255) / 256;
  constexpr int W_ITEMS = 9 * BN * 4;
  constexpr int W_PER = (W_ITEMS + 255) / 256;

  const T* A = reinterpret_cast<const T*>(g.a);
  const T* Bw = reinterpret_cast<const T*>(g.b);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bz_n = g.D / BZ, by_n = g.H / B2_Y, bx_n = g.W / B2_X;
  const int nbrick = (g.M / (g.D * g.H * g.W)) * bz_n * by_n * bx_n;
  const int nt_n = (g.Ncols + BN - 1) / BN;
  const int tile = g.swz ? xcd_swizzle(blockIdx.x, nbrick * nt_n) : (int)blockIdx.x;
  int bidx = tile % nbrick;
  const int nt = tile / nbrick;
  const int bx = bidx % bx_n; bidx /= bx_n;
  const int by = bidx % by_n; bidx /= by_n;
  const int bz = bidx % bz_n;
  const int n = bidx / bz_n;
  const int z0 = bz * BZ, y0 = by * B2_Y, x0 = bx * B2_X;
  const long long HW = (long long)g.H * g.W;
  const long long nbase = (long long)n * g.D * HW;
  const int n0 = nt * BN;
  const int cin = 8 << g.cpg_shift;
  const int nchunk = gemm_nchunk(g);
  const int nstage = nchunk * 3;

  V8<T> xr[X_PER], wr[W_PER];
  const int nvox = n * g.D * g.H * g.W;   // (B32 only: the host checked the extent)
  const __amdgpu_buffer_rsrc_t arsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(g.a), 0, B32 ? (int)((long long)g.M * g.lda * (int)sizeof(T)) : 0, 0x00020000);
  auto load_x = [&](int c) {
#pragma unroll
    for (int k = 0; k < X_PER; ++k) {
      const int e = tid + k * 256;
      if (e < X_ITEMS) {
        const int h = e >> 2, cg = e & 3;
        const int hx = h % H2_X, hy = (h / H2_X) % H2_Y, hz = h / (H2_X * H2_Y);
        const int z = z0 - 1 + hz, y = y0 - 1 + hy, x = x0 - 1 + hx;
        const bool ok = (unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H && (unsigned)x < (unsigned)g.W;
        if constexpr (B32) {
          const uint32_t off = ok ? (uint32_t)(((nvox + (z * g.H + y) * g.W + x) * g.lda + c * CK + cg * 8) *
                                               (int)sizeof(T))
                                  : 0x80000000u;
          buf_load_v8<T>(xr[k], arsrc, off);   // out-of-volume lanes read zeros
        } else {
          if (ok)
            xr[k].load(A + (nbase + z * HW + (long long)y * g.W + x) * g.lda + c * CK + cg * 8);
          else
            xr[k].zero();
        }
      }
    }
  };
  auto store_x = [&]() {
#pragma unroll
    for (int k = 0; k < X_PER; ++k) {
      const int e = tid + k * 256;
      if (e < X_ITEMS) {
        const int h = e >> 2, cg = e & 3;
        const int hx = h % H2_X, hy = (h / H2_X) % H2_Y, hz = h / (H2_X * H2_Y);
        xr[k].store(Xl + (hz * L::RZ + hy * L::RY + hx * L::QV + cg * L::QG) * EPQ);
      }
    }
  };
  auto load_w = [&](int c, int kz) {
#pragma unroll
    for (int k = 0; k < W_PER; ++k) {
      const int e = tid + k * 256;
      if (e < W_ITEMS) {
        const int cg = e & 3, q = e >> 2;
        const int col = q % BN, t9 = q / BN;
        const int kgi = (kz * 9 + t9) * (cin / 8) + c * 4 + cg;
        wr[k].load(Bw + ((long long)kgi * g.Cpad + n0 + col) * 8);
      }
    }
  };
  auto store_w = [&]() {
#pragma unroll
    for (int k = 0; k < W_PER; ++k) {
      const int e = tid + k * 256;
      if (e < W_ITEMS) {
        const int cg = e & 3, q = e >> 2;     // q = t9*BN + col
        wr[k].store(Wl + (q * L::QV + (cg ^ w2_swz(q)) * L::QG) * EPQ);
      }
    }
  };

  f32x4 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int r16 = lane & 15, kg = lane >> 4;
  int aq[RM];   // halo quad of the lane's row for tap (0,0,0), group kg
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    const int zs = wave * ZW + (i >> 2), yr = 2 * (i & 3) + (r16 >> 3), xr_ = r16 & 7;
    aq[i] = zs * L::RZ + yr * L::RY + xr_ * L::QV + kg * L::QG;
  }
  int bq[RN];
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    const int col = j * 16 + r16;
    bq[j] = col * L::QV + (kg ^ w2_swz(col)) * L::QG;
  }

  PROBE_T();
  load_x(0);
  load_w(0, 0);
  store_x();
  store_w();
  __syncthreads();
  PROBE_T();
  for (int st = 0; st < nstage; ++st) {
    const int c = st / 3, kz = st - c * 3;
    const int sn = st + 1;
    const bool more = sn < nstage;
    const int cn = sn / 3, kzn = sn - cn * 3;
    if (more) {
      load_w(cn, kzn);
      if (kzn == 0) load_x(cn);
    }
    if constexpr (PF) {
      // fragments of tap t+1 are read while tap t's MFMAs run (one wave per SIMD cannot hide the LDS latency
      // behind another wave's MFMAs)
      V8<T> af[2][RM], bf[2][RN];
      auto rd = [&](int t9, int b) {
        const int ky = t9 / 3, kx = t9 - ky * 3;
        const int hoff = kz * L::RZ + ky * L::RY + kx * L::QV;
#pragma unroll
        for (int j = 0; j < RN; ++j) bf[b][j].load(Wl + (t9 * BN * L::QV + bq[j]) * EPQ);
#pragma unroll
        for (int i = 0; i < RM; ++i) af[b][i].load(Xl + (aq[i] + hoff) * EPQ);
      };
      rd(0, 0);
#pragma unroll
      for (int t9 = 0; t9 < 9; ++t9) {
        if (t9 < 8) rd(t9 + 1, (t9 + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int j = 0; j < RN; ++j) mfma_step<T>(acc[i][j], af[t9 & 1][i], bf[t9 & 1][j]);
      }
    } else {
#pragma unroll
      for (int t9 = 0; t9 < 9; ++t9) {
        const int ky = t9 / 3, kx = t9 - ky * 3;
        const int hoff = kz * L::RZ + ky * L::RY + kx * L::QV;
        V8<T> af[RM], bf[RN];
#pragma unroll
        for (int j = 0; j < RN; ++j) bf[j].load(Wl + (t9 * BN * L::QV + bq[j]) * EPQ);
#pragma unroll
        for (int i = 0; i < RM; ++i) af[i].load(Xl + (aq[i] + hoff) * EPQ);
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int j = 0; j < RN; ++j) mfma_step<T>(acc[i][j], af[i], bf[j]);
      }
    }
    PROBE_T();
    __syncthreads();
    if (more) {
      store_w();
      if (kzn == 0) store_x();
      __syncthreads();
    }
    PROBE_T();
  }

  // epilogue: acc (+bias) -> LDS tile [BZ*64 voxels][BN] -> 16-B vector stores
  T* El = reinterpret_cast<T*>(lds4);
  constexpr int EP = BN + 8;   // padded pitch (elements)
  static_assert(BZ * 64 * (BN + 8) * sizeof(T) <= LQ * 16, "epilogue tile must fit");
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    const int col = j * 16 + r16;
    const float bv = (g.bias && n0 + col < g.Ncols) ? g.bias[n0 + col] : 0.f;
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int v = (wave * ZW + (i >> 2)) * 64 + (2 * (i & 3)) * 8 + kg * 4 + r;   // voxel in brick (z,y,x)
        El[v * EP + col] = from_f<T>(acc[i][j][r] + bv);
      }
  }
  __syncthreads();
  T* O = reinterpret_cast<T*>(g.out);
  constexpr int CG = BN / 8;                  // 8-column groups per voxel
  constexpr int O_ITEMS = BZ * 64 * CG;
  // zero groups past Ncols (whole-row hint), written by the last column tile's first groups
  const int zg = (g.zcols > g.Ncols && n0 + BN >= g.Ncols) ? (g.zcols - g.Ncols) >> 3 : 0;
#pragma unroll
  for (int k = 0; k < O_ITEMS / 256; ++k) {
    const int e = tid + k * 256;
    const int v = e / CG, cg = e % CG;
    const int col = n0 + cg * 8;
    const int z = z0 + (v >> 6), y = y0 + ((v >> 3) & 7), x = x0 + (v & 7);
    if (col < g.Ncols) {
      V8<T> o;
      o.load(El + v * EP + cg * 8);
      o.store(out_at<T>(g, nbase + z * HW + (long long)y * g.W + x, col));
    }
    for (int zc = cg; zc < zg; zc += CG) {
      V8<T> zv;
      zv.zero();
      zv.store(O + (nbase + z * HW + (long long)y * g.W + x) * g.ldo + g.Ncols + zc * 8);
    }
  }
  PROBE_T();
  PROBE_BLOCK(true);
}


// ------------------------------------------------- brick conv v3 (3^3)
// conv3_brick2_kernel (same 4x8x8-voxel brick, halo / weight LDS images and
// 9-tap stages) with the per-block fixed costs cut, which at Cin = 32 (one
// chunk, three stages per block) were ~5 VALU per MFMA (rocprofv3
// SQ_INSTS_VALU / SQ_INSTS_MFMA on the 96^3 layers):
//   * halo staging: thread t < 240 owns one (x, 8-channel group) column of the
//     halo and walks its 60 (z, y) rows 6 apart, so the voxel offset, the LDS
//     slot and the z / y bounds advance by block-uniform steps; the loads are
//     buffer loads whose out-of-volume lanes carry an offset past the buffer
//     end and read zeros (no branch, no zero fill);
//   * the MFMA computes the transposed tile W^T X (A and B swapped), so a lane
//     holds 4 consecutive output channels of one voxel: bias, bf16 packing and
//     an 8-B global store straight from the accumulators, no LDS epilogue.
// Measured and removed (round 6 knob pruning; numbers in DESIGN): a double-buffered weight stage (1 % slower),
// the next halo chunk loaded at the first stage of the current one (4 % slower on the bench), unconditional
// clamped weight loads, and sched_group_barrier interleaving of the fragment reads (8-13 % slower).
template <typename T, int BN>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 2 : 1) void conv3_brick3_kernel(GemmArgs g, int upb) {
  using L = Brick2Layout<T>;
  constexpr int BZ = 4, HZ = BZ + 2;
  constexpr int RM = 4, RN = BN / 16;
  constexpr int XQ = HZ * L::RZ;
  constexpr int WQ = 9 * BN * L::QV;
  __shared__ __attribute__((aligned(16))) float4 lds4[XQ + WQ];
  T* Xl = reinterpret_cast<T*>(lds4);
  T* Wl = reinterpret_cast<T*>(lds4 + XQ);
  constexpr int EPQ = 16 / sizeof(T);
  constexpr int XROWS = HZ * H2_Y;                    // 60 (z, y) halo rows
  constexpr int XK = XROWS / 6;                       // rows per thread (6 rows per pass of 240 threads)
  constexpr int W_ITEMS = 9 * BN * 4;
  constexpr int W_PER = (W_ITEMS + 255) / 256;
  static_assert(XROWS % 6 == 0, "halo rows per pass");

  const T* Bw = reinterpret_cast<const T*>(g.b);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bz_n = g.D / BZ, by_n = g.H / B2_Y, bx_n = g.W / B2_X;
  const int nbrick = (g.M / (g.D * g.H * g.W)) * bz_n * by_n * bx_n;
  const int nt_n = (g.Ncols + BN - 1) / BN;
  const int units = nbrick * nt_n;
  // this block's units: a contiguous range (consecutive units share halo columns in L2); unit = brick * nt_n + nt
  const int blk = g.swz ? xcd_swizzle(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int u_begin = blk * upb;
  const int u_end = u_begin + upb < units ? u_begin + upb : units;
  if (u_begin >= u_end) return;
  const int HW = g.H * g.W;
  const int cin = 8 << g.cpg_shift;
  const int nchunk = gemm_nchunk(g);
  const int nstage = nchunk * 3;
  const int ldb = g.lda * (int)sizeof(T);            // bytes per voxel
  const int vox_per_n = g.D * HW;

  // ---- halo column of this thread: (hx, cg) fixed, rows r0, r0+6, ... (hz = r / 10, hy = r % 10)
  const __amdgpu_buffer_rsrc_t arsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(g.a), 0, (int)((long long)(g.M / vox_per_n) * vox_per_n * ldb), 0x00020000);
  const bool xact = tid < 240;
  const int xq = tid % 40, r0 = tid / 40;
  const int hx = xq >> 2, cg = xq & 3;
  // row r0 + 6k -> (hz, hy) = divmod by 10 ((row * 205) >> 11 is exact for row < 1029); recomputed where
  // used rather than kept in 2 x XK registers (the BN64 instantiation is at the 256-VGPR cap)
  auto row_hz = [&](int k) { return ((r0 + 6 * k) * 205) >> 11; };
  const int xlds0 = (hx * L::QV + cg * L::QG) * EPQ;
  struct Unit { int n, z0, y0, x0, n0; };
  auto unit_of = [&](int u) {
    Unit r;
    const int nt = u % nt_n;
    int b = u / nt_n;
    const int bx = b % bx_n; b /= bx_n;
    const int by = b % by_n; b /= by_n;
    r.z0 = (b % bz_n) * BZ;
    r.n = b / bz_n;
    r.y0 = by * B2_Y;
    r.x0 = bx * B2_X;
    r.n0 = nt * BN;
    return r;
  };
  uint32_t xoff[XK];
  auto set_x = [&](const Unit& q) {    // per-unit halo offsets; out-of-volume lanes point past the buffer end
    const int xx = q.x0 - 1 + hx;
    const bool xok = xact && (unsigned)xx < (unsigned)g.W;
    const int vb = q.n * vox_per_n + xx;
#pragma unroll
    for (int k = 0; k < XK; ++k) {
      const int hz = row_hz(k), hy = r0 + 6 * k - 10 * hz;
      const int zz = q.z0 - 1 + hz, yy = q.y0 - 1 + hy;
      const bool ok = xok && (unsigned)zz < (unsigned)g.D && (unsigned)yy < (unsigned)g.H;
      xoff[k] = ok ? (uint32_t)((vb + zz * HW + yy * g.W) * ldb + cg * 8 * (int)sizeof(T)) : 0x80000000u;
    }
  };
  V8<T> xr[XK], wr[W_PER];
  auto load_x = [&](int c) {
    const uint32_t coff = (uint32_t)(c * CK * (int)sizeof(T));
#pragma unroll
    for (int k = 0; k < XK; ++k) buf_load_v8<T>(xr[k], arsrc, xoff[k] + coff);   // OOB lanes read 0
  };
  auto store_x = [&]() {
    if (xact) {
#pragma unroll
      for (int k = 0; k < XK; ++k) {
        const int hz = row_hz(k), hy = r0 + 6 * k - 10 * hz;
        xr[k].store(Xl + xlds0 + (hz * L::RZ + hy * L::RY) * EPQ);
      }
    }
  };
  // Every thread issues W_PER loads / stores unconditionally (items past the stage are clamped onto the
  // last item: a duplicate load and an identical store), so the compiler cannot sink a predicated load
  // past the tap loop, where its latency would be exposed right before store_w.
  auto load_w = [&](int n0, int c, int kz) {
#pragma unroll
    for (int k = 0; k < W_PER; ++k) {
      const int e0 = tid + k * 256;
      if (e0 < W_ITEMS) {
        const int e = e0;
        const int cgw = e & 3, q = e >> 2;
        const int col = q % BN, t9 = q / BN;
        const int kgi = (kz * 9 + t9) * (cin / 8) + c * 4 + cgw;
        wr[k].load(Bw + ((long long)kgi * g.Cpad + n0 + col) * 8);
      }
    }
  };
  auto store_w = [&]() {
    T* Wd = Wl;
#pragma unroll
    for (int k = 0; k < W_PER; ++k) {
      const int e0 = tid + k * 256;
      if (e0 < W_ITEMS) {
        const int e = e0;
        const int cgw = e & 3, q = e >> 2;
        wr[k].store(Wd + (q * L::QV + (cgw ^ w2_swz(q)) * L::QG) * EPQ);
      }
    }
  };

  const int r16 = lane & 15, kg = lane >> 4;
  int aq[RM];
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    const int yr = 2 * (i & 3) + (r16 >> 3), xr_ = r16 & 7;
    aq[i] = wave * L::RZ + yr * L::RY + xr_ * L::QV + kg * L::QG;
  }
  int bq[RN];
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    const int col = j * 16 + r16;
    bq[j] = col * L::QV + (kg ^ w2_swz(col)) * L::QG;
  }
  T* O = reinterpret_cast<T*>(g.out);

  Unit cur = unit_of(u_begin);
  set_x(cur);
  load_x(0);
  load_w(cur.n0, 0, 0);
  store_x();
  store_w();
  __syncthreads();
  for (int u = u_begin; u < u_end; ++u) {
    f32x4 acc[RM][RN];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int j = 0; j < RN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bool unext = u + 1 < u_end;
    Unit nxt = cur;
    if (unext) nxt = unit_of(u + 1);
    for (int st = 0; st < nstage; ++st) {
      const int c = st / 3, kz = st - c * 3;
      // next stage: (cn, kzn) of this unit, or stage 0 of the next unit
      const bool last = st + 1 == nstage;
      const bool more = !last || unext;
      const int sn = last ? 0 : st + 1;
      const int cn = sn / 3, kzn = sn - cn * 3;
      if (more) {
        if (last) set_x(nxt);
        load_w(last ? nxt.n0 : cur.n0, cn, kzn);
        if (kzn == 0) load_x(cn);
      }
#pragma unroll
      for (int t9 = 0; t9 < 9; ++t9) {
        const int ky = t9 / 3, kx = t9 - ky * 3;
        const int hoff = kz * L::RZ + ky * L::RY + kx * L::QV;
        V8<T> af[RM], bf[RN];
#pragma unroll
        for (int j = 0; j < RN; ++j) bf[j].load(Wl + (t9 * BN * L::QV + bq[j]) * EPQ);
#pragma unroll
        for (int i = 0; i < RM; ++i) af[i].load(Xl + (aq[i] + hoff) * EPQ);
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int j = 0; j < RN; ++j) mfma_step<T>(acc[i][j], bf[j], af[i]);   // transposed: rows = channels
      }
      __syncthreads();
      if (more) {
        store_w();
        if (kzn == 0) store_x();
        __syncthreads();
      }
    }
    // epilogue: lane holds channels n0 + j*16 + 4*kg + (0..3) of voxel r16 of row tile i
    const long long obase = (long long)cur.n * vox_per_n;
#pragma unroll
    for (int j = 0; j < RN; ++j) {
      const int col = cur.n0 + j * 16 + 4 * kg;
      if (col >= g.Ncols) continue;
      float bv[4] = {0.f, 0.f, 0.f, 0.f};
      if (g.bias) {
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[r] = g.bias[col + r];   // the bias view is only 4-B aligned
      }
#pragma unroll
      for (int i = 0; i < RM; ++i) {
        const int z = cur.z0 + wave, y = cur.y0 + 2 * (i & 3) + (r16 >> 3), x = cur.x0 + (r16 & 7);
        T* dst = out_at<T>(g, obase + (long long)(z * g.H + y) * g.W + x, col);
        if constexpr (sizeof(T) == 2) {
          typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
          bf16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = (bf16_t)(acc[i][j][r] + bv[r]);
          *reinterpret_cast<bf16x4*>(dst) = o;
        } else {
          *reinterpret_cast<float4*>(dst) = make_float4(acc[i][j][0] + bv[0], acc[i][j][1] + bv[1],
                                                        acc[i][j][2] + bv[2], acc[i][j][3] + bv[3]);
        }
      }
    }
    cur = nxt;
  }
}

// ------------------------------------------------- brick conv v4 (3^3, bf16, Cin = 32, Co tile 32)
// The 96^3 32 -> 32 layers.  v3 restages the 9-tap weight slab of every (brick, kz) stage through LDS and
// every wave re-reads the same B fragments: per tap and wave 4 A + 2 B ds_read_b128 for 8 MFMAs, plus
// 54 KB of weight and 38 KB of halo LDS writes per brick, and two barriers per stage.  v4:
//   * the whole 27-tap x 32-ci x 32-co weight tile of the block's column tile lives in the accumulator
//     register file (27 x 2 fragments = 216 AGPRs, loaded once per block straight from the packed
//     [KG][Cpad][8] image, which is already fragment-ordered; mfma_aw); LDS holds only halos;
//   * one block of 4 waves per CU (1 wave / SIMD), persistent over a contiguous brick range; the halo is
//     double-buffered: the next brick's halo is loaded into registers when a brick starts and written to the
//     other LDS buffer after 15 taps, so one barrier per brick;
//   * each tap's 4 A reads are issued two taps ahead of their MFMAs (sched_barrier; left alone, hipcc
//     issues them just before their MFMAs).
// Measured (s_memtime stamps, 96^3 B=2 forward): ~200 cycles per tap against 128 of MFMA issue, and the
// tap loop speeds up in proportion when the per-tap A reads are cut (half the reads: 146 cycles per tap):
// the LDS read stream, not latency, barriers or the halo loads, is what bounds this kernel.
// Requirements (host): bf16, one 32-channel K chunk, Ncols % 32 == 0, D % 4, H % 8, W % 8.

__global__ __launch_bounds__(256, 1) void conv3_brick4_kernel(GemmArgs g, int upb, int blocks_per_nt) {
  using T = bf16_t;
  using L = Brick2Layout<T>;
  constexpr int BZ = 4, HZ = BZ + 2;
  constexpr int RM = 4, RN = 2;
  constexpr int PF = 2;                               // A-fragment prefetch distance (taps)
  constexpr int XQ = HZ * L::RZ;
  __shared__ __attribute__((aligned(16))) float4 lds4[2 * XQ];
  T* Xl = reinterpret_cast<T*>(lds4);
  constexpr int EPQ = 8;
  constexpr int XROWS = HZ * H2_Y;                    // 60 (z, y) halo rows
  constexpr int XK = XROWS / 6;                       // rows per thread (6 rows per pass of 240 threads)

  const T* Bw = reinterpret_cast<const T*>(g.b);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bz_n = g.D / BZ, by_n = g.H / B2_Y, bx_n = g.W / B2_X;
  const int nbrick = (g.M / (g.D * g.H * g.W)) * bz_n * by_n * bx_n;
  const int blk_all = g.swz ? xcd_swizzle(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int nt = blk_all / blocks_per_nt, blk = blk_all - nt * blocks_per_nt;
  const int n0 = nt * 32;
  const int u_begin = blk * upb;
  const int u_end = u_begin + upb < nbrick ? u_begin + upb : nbrick;
  if (u_begin >= u_end || n0 >= g.Ncols) return;
  const int HW = g.H * g.W;
  const int cin = 8 << g.cpg_shift;
  const int ldb = g.lda * (int)sizeof(T);
  const int vox_per_n = g.D * HW;
  const int r16 = lane & 15, kg = lane >> 4;

  // ---- weights: fragment (tap, j) = 8 input channels kg*8.. of output column n0 + j*16 + r16
  V8<T> wf[27][RN];
#pragma unroll
  for (int t = 0; t < 27; ++t)
#pragma unroll
    for (int j = 0; j < RN; ++j)
      wf[t][j].load(Bw + ((long long)(t * (cin / 8) + kg) * g.Cpad + n0 + j * 16 + r16) * 8);
#pragma unroll
  for (int t = 0; t < 27; ++t) brick4_wfence(wf[t][0].v, wf[t][1].v);

  // ---- halo column of this thread: (hx, cg) fixed, rows r0, r0+6, ... (hz = r / 10, hy = r % 10)
  const __amdgpu_buffer_rsrc_t arsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(g.a), 0, (int)((long long)(g.M / vox_per_n) * vox_per_n * ldb), 0x00020000);
  const bool xact = tid < 240;
  const int xq = tid % 40, r0 = tid / 40;
  const int hx = xq >> 2, cg = xq & 3;
  auto row_hz = [&](int k) { return ((r0 + 6 * k) * 205) >> 11; };
  const int xlds0 = (hx * L::QV + cg * L::QG) * EPQ;
  struct Unit { int n, z0, y0, x0; };
  auto unit_of = [&](int b) {
    Unit r;
    const int bx = b % bx_n; b /= bx_n;
    const int by = b % by_n; b /= by_n;
    r.z0 = (b % bz_n) * BZ;
    r.n = b / bz_n;
    r.y0 = by * B2_Y;
    r.x0 = bx * B2_X;
    return r;
  };
  V8<T> xr[XK];
  auto load_x = [&](const Unit& q) {    // out-of-volume lanes point past the buffer end and read zeros
    const int xx = q.x0 - 1 + hx;
    const bool xok = xact && (unsigned)xx < (unsigned)g.W;
    const int vb = q.n * vox_per_n + xx;
#pragma unroll
    for (int k = 0; k < XK; ++k) {
      const int hz = row_hz(k), hy = r0 + 6 * k - 10 * hz;
      const int zz = q.z0 - 1 + hz, yy = q.y0 - 1 + hy;
      const bool ok = xok && (unsigned)zz < (unsigned)g.D && (unsigned)yy < (unsigned)g.H;
      const uint32_t off = ok ? (uint32_t)((vb + zz * HW + yy * g.W) * ldb + cg * 16) : 0x80000000u;
      buf_load_v8<T>(xr[k], arsrc, off);
    }
  };
  auto store_x = [&](int buf) {
    if (xact) {
#pragma unroll
      for (int k = 0; k < XK; ++k) {
        const int hz = row_hz(k), hy = r0 + 6 * k - 10 * hz;
        xr[k].store(Xl + buf * XQ * EPQ + xlds0 + (hz * L::RZ + hy * L::RY) * EPQ);
      }
    }
  };
  int aq[RM];
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    const int yr = 2 * i + (r16 >> 3), xr_ = r16 & 7;
    aq[i] = wave * L::RZ + yr * L::RY + xr_ * L::QV + kg * L::QG;
  }
  float bv[RN][4];
#pragma unroll
  for (int j = 0; j < RN; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[j][r] = g.bias ? g.bias[n0 + j * 16 + 4 * kg + r] : 0.f;
  T* O = reinterpret_cast<T*>(g.out);

  Unit cur = unit_of(u_begin);
  load_x(cur);
  store_x(0);
  __syncthreads();
  int b = 0;
  // (Storing each brick's outputs a few taps into the next brick, from a second accumulator set, measured
  // 25 % slower; loading the next halo in two halves, or storing it later, measured no faster.)
  for (int u = u_begin; u < u_end; ++u) {
    f32x4 acc[RM][RN];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int j = 0; j < RN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bool unext = u + 1 < u_end;
    Unit nxt = cur;
    if (unext) {
      nxt = unit_of(u + 1);
      load_x(nxt);
    }
    const T* Xb = Xl + b * XQ * EPQ;
    auto hoff = [](int t) { return (t / 9) * L::RZ + ((t / 3) % 3) * L::RY + (t % 3) * L::QV; };
    V8<T> af[PF + 1][RM];
#pragma unroll
    for (int p = 0; p < PF; ++p)
#pragma unroll
      for (int i = 0; i < RM; ++i) af[p][i].load(Xb + (aq[i] + hoff(p)) * EPQ);
#pragma unroll
    for (int t = 0; t < 27; ++t) {
      if (t == 15 && unext) store_x(b ^ 1);
      if (t + PF < 27) {
#pragma unroll
        for (int i = 0; i < RM; ++i) af[(t + PF) % (PF + 1)][i].load(Xb + (aq[i] + hoff(t + PF)) * EPQ);
      }
      __builtin_amdgcn_sched_barrier(0);   // keep the reads PF taps ahead of their MFMAs
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j) mfma_aw(acc[i][j], wf[t][j].v, af[t % (PF + 1)][i].v);   // rows = channels
    }
#pragma unroll
    for (int i = 0; i < RM; ++i) brick4_fence(acc[i][0], acc[i][1]);
    // epilogue: lane holds channels n0 + j*16 + 4*kg + (0..3) of voxel r16 of row tile i
    const long long obase = (long long)cur.n * vox_per_n;
#pragma unroll
    for (int j = 0; j < RN; ++j) {
      const int col = n0 + j * 16 + 4 * kg;
#pragma unroll
      for (int i = 0; i < RM; ++i) {
        const int z = cur.z0 + wave, y = cur.y0 + 2 * i + (r16 >> 3), x = cur.x0 + (r16 & 7);
        T* dst = out_at<T>(g, obase + (long long)(z * g.H + y) * g.W + x, col);
        typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (bf16_t)(acc[i][j][r] + bv[j][r]);
        *reinterpret_cast<bf16x4*>(dst) = o;
      }
    }
    __syncthreads();   // buffer b^1 is complete; buffer b is free for the brick after next
    b ^= 1;
    cur = nxt;
  }
}

// One instantiation per choice of the family, on the grid choose_gemm gave it.
template <typename T>
void launch_brick2_t(const GemmArgs& g, const GemmChoice& c, hipStream_t s) {
  const dim3 grid(c.grid), block(c.block);
  switch (c.kernel) {
    case GK_BRICK2_BN48:
      if (c.b32) MMSEG_LAUNCH((conv3_brick2_kernel<T, 48, 1, false, true>), grid, block, 0, s, g);
      else MMSEG_LAUNCH((conv3_brick2_kernel<T, 48, 1>), grid, block, 0, s, g);
      break;
    case GK_BRICK4:
      if constexpr (sizeof(T) == 2) MMSEG_LAUNCH(conv3_brick4_kernel, grid, block, 0, s, g, c.upb, c.bpn);
      break;
    case GK_BRICK3:
      MMSEG_LAUNCH((conv3_brick3_kernel<T, 32>), grid, block, 0, s, g, c.upb);
      break;
    case GK_BRICK2:
      if (c.bn == 64 && c.b32)
        MMSEG_LAUNCH((conv3_brick2_kernel<T, 64, 1, true, true>), grid, block, 0, s, g);
      else if (c.bn == 64)
        MMSEG_LAUNCH((conv3_brick2_kernel<T, 64, 1, true>), grid, block, 0, s, g);
      else
        MMSEG_LAUNCH((conv3_brick2_kernel<T, 32, 1>), grid, block, 0, s, g);
      break;
    case GK_BRICK1:
      if (c.bn == 64) MMSEG_LAUNCH((conv3_brick_kernel<T, 64>), grid, block, 0, s, g);
      else MMSEG_LAUNCH((conv3_brick_kernel<T, 32>), grid, block, 0, s, g);
      break;
  }
}

}  // namespace

MMSEG_LOCAL void launch_brick2(const GemmArgs& g, const GemmChoice& c, hipStream_t s) {
  if (c.tsize == 2) launch_brick2_t<bf16_t>(g, c, s);
  else launch_brick2_t<float>(g, c, s);
}

MMSEG_PROBE_SETTER(probe_set_brick2)
