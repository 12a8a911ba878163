// conv3_brick8_kernel: the 8-wave 8x8x8-brick 3^3 conv with LDS-DMA staging (bf16), and its launcher.
#include "conv_common.h"

namespace {

// ------------------------------------------------- brick conv v8 (3^3, bf16, 8 waves, LDS-DMA staging)
// conv3_brick2's BN-column tile with the block grown to an (8 ZP) x 8 x 8 brick: 8 waves, wave w owns z planes
// w ZP .. w ZP + ZP - 1 (64 voxels each = 4 row tiles of two 8-voxel x rows) x BN columns (BN 64 with ZP 1; BN 32
// with ZP 2, so a wave still runs 16 MFMAs per tap).  Both operands are staged by LDS-DMA
// (buffer_load ... lds): no staging registers and no ds_write pass, which in conv3_brick2 were ~2 VALU + 0.7 SALU
// per MFMA around a per-stage register round trip of the weights.  Per block:
//   * the halo image of one 32-channel input chunk: 10 x 10 rows of 10 voxels x 4 quads + 2 pad quads (the pad
//     keeps the 16-lane groups of the A-fragment ds_read_b128 on distinct banks), single buffer, re-filled
//     between chunks (that refill is the one exposed load: 1 of 3 * nchunk stages);
//   * the weight slice of one (chunk, kz) stage: 9 taps x BN columns x 32 channels in the B-operand order
//     [tap][col][4 quads, channel group kg at slot kg ^ w2_swz(col)], double buffered: stage s + 1's slice
//     lands while stage s is multiplied.
// The lane-linear DMA destination is matched by computing, per lane, the source of the quad that belongs at its
// LDS slot (pads and out-of-volume voxels read zeros through the OOB offset).  Each staged weight slice feeds
// 8 waves x 9 taps x 4 ZP x RN MFMAs (twice conv3_brick2's).  LDS 141 KB (BN 64) / 155 KB (BN 32): one block per
// CU, two waves per SIMD.  Requirements (host): bf16, Cin % 32 == 0, Ncols % BN == 0, D % 8 ZP, H % 8, W % 8, ksplit == 1, no
// deferred norm / IN partials, the A and B extents < 2^31 bytes.
template <int BN, int ZP>
__global__ __launch_bounds__(512, 1) void conv3_brick8_kernel(GemmArgs g) {
  PROBE_BLOCK(false);
  PROBE_DECL();
  typedef bf16_t T;
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  constexpr int QV = 4;                                  // 16-B quads per halo voxel (32 channels)
  constexpr int BZ = 8 * ZP;                            // z planes per brick (ZP per wave)
  constexpr int HXY = 10, HZ = BZ + 2;
  constexpr int RY = HXY * QV + 2, RZ = HXY * RY;        // 42 quads per halo row, 420 per plane
  constexpr int XQ = HZ * RZ;                            // 4200 (ZP 1) / 7560 (ZP 2)
  constexpr int XI = (XQ + 63) / 64, XK = (XI + 7) / 8;  // 66 / 119 wave-instructions
  constexpr int XQP = XI * 64;
  constexpr int WQ = 9 * BN * QV;                        // 2304 quads (BN 64)
  constexpr int WI = WQ / 64, WK = (WI + 7) / 8;         // 36, <= 5 per wave
  constexpr int RM = 4 * ZP, RN = BN / 16;
  constexpr int EPQ = 8;                                 // bf16 per quad
  static_assert(WQ % 64 == 0, "weight slice must be whole wave-instructions");
  __shared__ __attribute__((aligned(16))) float4 lds4[XQP + 2 * WQ];
  T* Xl = reinterpret_cast<T*>(lds4);
  T* Wl = reinterpret_cast<T*>(lds4 + XQP);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bz_n = g.D / BZ, by_n = g.H >> 3, bx_n = g.W >> 3;
  const int nbrick = (g.M / (g.D * g.H * g.W)) * bz_n * by_n * bx_n;
  const int nt_n = g.Ncols / BN;
  const int tile = g.swz ? xcd_swizzle(blockIdx.x, nbrick * nt_n) : (int)blockIdx.x;
  int bidx = tile % nbrick;
  const int nt = tile / nbrick;
  const int bx = bidx % bx_n; bidx /= bx_n;
  const int by = bidx % by_n; bidx /= by_n;
  const int bz = bidx % bz_n;
  const int n = bidx / bz_n;
  const int z0 = bz * BZ, y0 = by * 8, x0 = bx * 8;
  const int n0 = nt * BN;
  const int cin = 8 << g.cpg_shift;
  const int nchunk = gemm_nchunk(g);
  const int nstage = nchunk * 3;
  const long long HW = (long long)g.H * g.W;
  const long long nbase = (long long)n * g.D * HW;

  const wd_rsrc_t arsrc = wd_rsrc(g.a, (uint32_t)((long long)g.M * g.lda * 2));
  const int KGp = (g.KG + 3) & ~3;
  const wd_rsrc_t brsrc = wd_rsrc(g.b, (uint32_t)((long long)KGp * g.Cpad * 16));

  // per-lane halo sources: quad p = 64 m + lane of instruction m = wave + 8 kk, byte offset of chunk 0 or OOB
  uint32_t xo[XK];
#pragma unroll
  for (int kk = 0; kk < XK; ++kk) {
    const int p = (wave + 8 * kk) * 64 + lane;
    const int row = p / RY, qi = p - row * RY;
    const int hz = row / HXY, hy = row - hz * HXY, hx = qi >> 2, cg = qi & 3;
    const int z = z0 - 1 + hz, y = y0 - 1 + hy, x = x0 - 1 + hx;
    const bool ok = p < XQ && qi < HXY * QV && (unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H &&
                    (unsigned)x < (unsigned)g.W;
    xo[kk] = ok ? (uint32_t)((((n * g.D + z) * g.H + y) * g.W + x) * g.lda * 2 + cg * 16) : WD_OOB;
  }
  // per-lane weight sources: quad p = (t9 * BN + col) * 4 + slot, channel group slot ^ w2_swz(col)
  uint32_t wo[WK];
#pragma unroll
  for (int kk = 0; kk < WK; ++kk) {
    const int p = (wave + 8 * kk) * 64 + lane;
    const int q = p >> 2, col = q % BN, t9 = q / BN;
    const int cg = (p & 3) ^ w2_swz(col);
    wo[kk] = (uint32_t)(((t9 * (cin / 8) + cg) * g.Cpad + n0 + col) * 16);
  }
  const uint32_t xl_base = (uint32_t)(uintptr_t)(lds_ptr_t)Xl;
  const uint32_t wl_base = (uint32_t)(uintptr_t)(lds_ptr_t)Wl;
  auto issue_x = [&](int c) {
#pragma unroll
    for (int kk = 0; kk < XK; ++kk) {
      const int m = wave + 8 * kk;
      if (m < XI)
        wd_dma16(__builtin_amdgcn_readfirstlane((int)(xl_base + m * 1024)),
                 xo[kk] == WD_OOB ? WD_OOB : xo[kk] + c * 64, arsrc);
    }
  };
  auto issue_w = [&](int s, int buf) {
    const int c = s / 3, kz = s - c * 3;
    const uint32_t so = (uint32_t)((kz * 9 * (cin / 8) + c * 4) * g.Cpad * 16);
#pragma unroll
    for (int kk = 0; kk < WK; ++kk) {
      const int m = wave + 8 * kk;
      if (m < WI)
        wd_dma16(__builtin_amdgcn_readfirstlane((int)(wl_base + (buf * WQ + m * 64) * 16)), wo[kk] + so, brsrc);
    }
  };

  f32x4 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int r16 = lane & 15, kg = lane >> 4;
  int aq[RM];   // halo quad of the lane's row for tap (0,0,0), group kg: z plane wave * ZP + i / 4
#pragma unroll
  for (int i = 0; i < RM; ++i)
    aq[i] = (wave * ZP + (i >> 2)) * RZ + (2 * (i & 3) + (r16 >> 3)) * RY + (r16 & 7) * QV + kg;
  int bq[RN];
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    const int col = j * 16 + r16;
    bq[j] = col * QV + (kg ^ w2_swz(col));
  }

  PROBE_T();
  issue_x(0);
  issue_w(0, 0);
  __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): this wave's pieces have landed
  __syncthreads();
  PROBE_T();
  for (int s = 0; s < nstage; ++s) {
    const int kz = s % 3, b = s & 1;
    const bool more = s + 1 < nstage;
    if (more) issue_w(s + 1, b ^ 1);
    const T* Wb = Wl + b * WQ * EPQ;
    V8<T> af[2][RM], bf[2][RN];
    auto rd = [&](int t9, int k) {
      const int ky = t9 / 3, kx = t9 - ky * 3;
      const int hoff = kz * RZ + ky * RY + kx * QV;
#pragma unroll
      for (int j = 0; j < RN; ++j) bf[k][j].load(Wb + (t9 * BN * QV + bq[j]) * EPQ);
#pragma unroll
      for (int i = 0; i < RM; ++i) af[k][i].load(Xl + (aq[i] + hoff) * EPQ);
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
    if (more) {
      if ((s + 1) % 3 == 0) {           // next chunk: every wave is done with this halo, then refill it
        __syncthreads();
        issue_x((s + 1) / 3);
      }
      PROBE_T();
      __builtin_amdgcn_s_waitcnt(0x0f70);
      __syncthreads();
    }
    PROBE_T();
  }

  // epilogue: acc (+bias) -> LDS tile [512 ZP voxels][BN + 8] -> 16-B stores
  __syncthreads();
  T* El = reinterpret_cast<T*>(lds4);
  constexpr int EP = BN + 8;
  static_assert(512 * ZP * EP * 2 <= (XQP + 2 * WQ) * 16, "epilogue tile must fit");
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    const int col = j * 16 + r16;
    const float bv = (g.bias && n0 + col < g.Ncols) ? g.bias[n0 + col] : 0.f;
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        El[((wave * ZP + (i >> 2)) * 64 + 16 * (i & 3) + 4 * kg + r) * EP + col] = from_f<T>(acc[i][j][r] + bv);
  }
  __syncthreads();
  constexpr int CG = BN / 8;
#pragma unroll
  for (int k = 0; k < ZP * CG; ++k) {
    const int e = tid + k * 512;
    const int v = e / CG, cg = e % CG;
    const int z = z0 + (v >> 6), y = y0 + ((v >> 3) & 7), x = x0 + (v & 7);
    V8<T> o;
    o.load(El + v * EP + cg * 8);
    o.store(out_at<T>(g, nbase + z * HW + (long long)y * g.W + x, n0 + cg * 8));
  }
  PROBE_T();
  PROBE_BLOCK(true);
}

}  // namespace

MMSEG_LOCAL void launch_brick8(const GemmArgs& g, const GemmChoice& c, hipStream_t s) {
  const dim3 grid(c.grid), block(c.block);
  if (c.bn == 64) MMSEG_LAUNCH((conv3_brick8_kernel<64, 1>), grid, block, 0, s, g);
  else MMSEG_LAUNCH((conv3_brick8_kernel<32, 2>), grid, block, 0, s, g);
}

MMSEG_PROBE_SETTER(probe_set_brick8)
