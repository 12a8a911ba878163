// conv3_brickr_kernel: the runtime-brick 3^3 conv of the small volumes and the grouped launches, with its launcher.
#include "conv_common.h"

namespace {

// ------------------------------------- runtime-brick conv (small volumes)
// conv3_brick2_kernel for volumes whose sides are not multiples of 8 (the
// 12^3 and 6^3 levels): the brick (bz, by, bx), <= 256 voxels, is chosen on the
// host among divisors of (D, H, W), and the 27*Cin reduction can be split over
// 32-channel chunks (fp32 partials [ks][M][Ncols] + gemm_splitk_reduce) so that
// a handful of bricks still fills the chip.  Row r of the block (wave*64 + i*16
// + lane%16) is brick voxel r; rows >= bz*by*bx compute garbage and are never
// stored.
// CB* > 0: the brick is known at compile time (6x6x6 at the 12^3 / 6^3 levels), so the halo / epilogue index
// arithmetic divides by constants (mul-shift) instead of runtime integer divisions, which at one 32-channel
// chunk per block were most of the kernel's VALU work (8.6 VALU instructions per MFMA, rocprofv3 r02).
// B32 (bf16): the halo staged with 32-bit offset buffer loads, out-of-volume lanes reading zeros (conv3_brick2's B32).
// KW = 2 (12^3 / 6^3, r05): 512-thread blocks whose two 256-thread halves split the block's 32-channel chunks
// (half 0 the first ceil(n/2), half 1 the rest), each with its own halo / weight stage buffers, in lockstep through
// the same barriers; half 1's accumulators are added to half 0's through LDS (fixed order) before the epilogue.
// At these levels a launch has ~256 blocks, one per CU, so the KW = 1 form runs ONE wave per SIMD and nothing
// hides a wave's staging and LDS latency; two K-halves give every SIMD a second wave without a global split.
template <typename T, int BN, int CBZ = 0, int CBY = 0, int CBX = 0, bool PF = false, bool B32 = false, int KW = 1>
__global__ __launch_bounds__(256 * KW, (sizeof(T) == 2 && KW == 1) ? 2 : 1) void conv3_brickr_kernel(
    GemmArgs g, int bz_rt, int by_rt, int bx_rt) {
  const int bz = CBZ > 0 ? CBZ : bz_rt, by = CBY > 0 ? CBY : by_rt, bx = CBX > 0 ? CBX : bx_rt;
  using L = Brick2Layout<T>;
  constexpr int RM = 4, RN = BN / 16;
  constexpr int XQ = br_xq(sizeof(T));
  constexpr int WQ = 9 * BN * L::QV;
  constexpr int EQ = (256 * (BN + 4) * 4 + 15) / 16;   // fp32 epilogue tile
  constexpr int RQ = KW > 1 ? 256 * BN / 4 : 0;           // half 1's accumulators (fp32), after the epilogue tile
  constexpr int LQ = (KW * (XQ + WQ)) > (EQ + RQ) ? (KW * (XQ + WQ)) : (EQ + RQ);
  __shared__ __attribute__((aligned(16))) float4 lds4[LQ];
  const int half = KW > 1 ? (int)(threadIdx.x >> 8) : 0;
  T* Xl = reinterpret_cast<T*>(lds4 + half * (XQ + WQ));
  T* Wl = reinterpret_cast<T*>(lds4 + half * (XQ + WQ) + XQ);
  constexpr int EPQ = 16 / sizeof(T);
  constexpr int X_PER = (BR_MAXHV * 4 + 255) / 256;
  constexpr int W_ITEMS = 9 * BN * 4;
  constexpr int W_PER = (W_ITEMS + 255) / 256;

  const int HX = bx + 2, HY = by + 2, HZ = bz + 2;
  const int RY = HX * L::QV + 2, RZ = HY * RY;
  const int HV = HZ * HY * HX;
  const int X_ITEMS = HV * 4;
  const int rows = bz * by * bx;

  const T* A = reinterpret_cast<const T*>(g.a);
  const T* Bw = reinterpret_cast<const T*>(g.b);
  const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
  const int bz_n = g.D / bz, by_n = g.H / by, bx_n = g.W / bx;
  const int nbrick = (g.M / (g.D * g.H * g.W)) * bz_n * by_n * bx_n;
  const int nt_n = (g.Ncols + BN - 1) / BN;
  const int tile = g.swz ? xcd_swizzle(blockIdx.x, nbrick * nt_n * g.ksplit) : (int)blockIdx.x;
  int bidx = tile % nbrick;
  const int nt = (tile / nbrick) % nt_n;
  const int ks = tile / (nbrick * nt_n);
  const int bxi = bidx % bx_n; bidx /= bx_n;
  const int byi = bidx % by_n; bidx /= by_n;
  const int bzi = bidx % bz_n;
  const int n = bidx / bz_n;
  const int z0 = bzi * bz, y0 = byi * by, x0 = bxi * bx;
  const long long HW = (long long)g.H * g.W;
  const long long nbase = (long long)n * g.D * HW;
  const int grp = g.grp_n > 0 ? n / g.grp_n : 0;     // grouped launch: this brick's weight / bias group
  if (grp) Bw += (long long)grp * g.w_gstride;
  const float* biasp = (g.bias && grp) ? g.bias + grp * g.b_gstride : g.bias;
  const int n0 = nt * BN;
  const int cin = 8 << g.cpg_shift;
  const int nchunk = gemm_nchunk(g);
  const int cps = (nchunk + g.ksplit - 1) / g.ksplit;
  const int cb0 = ks * cps;
  const int ce0 = cb0 + cps < nchunk ? cb0 + cps : nchunk;
  // KW = 2: this half's chunks of the block's range (half 0 takes the larger share when it is odd)
  const int cmid = cb0 + (ce0 - cb0 + 1) / 2;
  const int c_begin = KW > 1 && half ? cmid : cb0;
  const int c_end = KW > 1 ? (half ? ce0 : cmid) : ce0;
  // iterations every thread of the block runs (the barriers inside the loop are block-wide): half 0's count
  const int n_iter = ((KW > 1 ? cmid : ce0) - cb0) * 3;

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
        const int hx = h % HX, t = h / HX;
        const int hy = t % HY, hz = t / HY;
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
        const int hx = h % HX, t = h / HX;
        const int hy = t % HY, hz = t / HY;
        xr[k].store(Xl + (hz * RZ + hy * RY + hx * L::QV + cg * L::QG) * EPQ);
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
        const int cg = e & 3, q = e >> 2;
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
  int aq[RM];
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    int rr = wave * 64 + i * 16 + r16;
    if (rr >= rows) rr = 0;   // padding rows read voxel 0's halo (never stored)
    const int rx = rr % bx, t = rr / bx;
    const int ry = t % by, rz = t / by;
    aq[i] = rz * RZ + ry * RY + rx * L::QV + kg * L::QG;
  }
  int bq[RN];
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    const int col = j * 16 + r16;
    bq[j] = col * L::QV + (kg ^ w2_swz(col)) * L::QG;
  }

  const int st_begin = c_begin * 3, st_end = c_end * 3;
  if (st_begin < st_end) {
    load_x(c_begin);
    load_w(c_begin, 0);
    store_x();
    store_w();
  }
  __syncthreads();
  for (int it = 0; it < n_iter; ++it) {
    const int st = st_begin + it;
    const bool active = st < st_end;   // (KW = 2: half 1 may own one chunk fewer; it still joins every barrier)
    const int kz = st % 3;
    const int sn = st + 1;
    const bool more = sn < st_end;
    const int cn = sn / 3, kzn = sn - cn * 3;
    if (more) {
      load_w(cn, kzn);
      if (kzn == 0) load_x(cn);
    }
    if (!active) {
    } else if constexpr (PF) {
      // fragments of tap t+1 are read while tap t's MFMAs run: at one block per CU (one wave per SIMD) nothing
      // else hides the LDS latency (s_memtime: ~4,200 cycles per 9-tap stage against 2,304 of MFMA)
      V8<T> af[2][RM], bf[2][RN];
      auto rd = [&](int t9, int b) {
        const int ky = t9 / 3, kx = t9 - ky * 3;
        const int hoff = kz * RZ + ky * RY + kx * L::QV;
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
    } else
#pragma unroll
    for (int t9 = 0; t9 < 9; ++t9) {
      const int ky = t9 / 3, kx = t9 - ky * 3;
      const int hoff = kz * RZ + ky * RY + kx * L::QV;
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
    __syncthreads();
    if (more) {
      store_w();
      if (kzn == 0) store_x();
    }
    if (KW > 1 || more) __syncthreads();   // (KW = 2: the halves' `more` may differ)
  }

  // KW = 2: half 1's accumulators added to half 0's (the loop ended with a barrier: the stage buffers are free)
  if constexpr (KW > 1) {
    f32x4* R4 = reinterpret_cast<f32x4*>(lds4 + EQ);
    if (half) {
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j) R4[((wave * RM + i) * RN + j) * 64 + lane] = acc[i][j];
    }
    __syncthreads();
    if (!half) {
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j) {
          const f32x4 o = R4[((wave * RM + i) * RN + j) * 64 + lane];
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i][j][r] += o[r];
        }
    }
  }
  // epilogue through LDS: rows < bz*by*bx only (KW = 2: half 0 fills the tile, all 512 threads store it)
  auto row_vox = [&](int rr) {
    const int rx = rr % bx, t = rr / bx;
    const int ry = t % by, rz = t / by;
    return nbase + (z0 + rz) * HW + (long long)(y0 + ry) * g.W + (x0 + rx);
  };
  const int etid = threadIdx.x;
  constexpr int ET = 256 * KW;
  if (g.ksplit == 1) {
    T* El = reinterpret_cast<T*>(lds4);
    constexpr int EP = BN + 8;
    if (!half) {
#pragma unroll
      for (int j = 0; j < RN; ++j) {
        const int col = j * 16 + r16;
        const float bv = (biasp && n0 + col < g.Ncols) ? biasp[n0 + col] : 0.f;
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) El[(wave * 64 + i * 16 + kg * 4 + r) * EP + col] = from_f<T>(acc[i][j][r] + bv);
      }
    }
    __syncthreads();
    T* O = reinterpret_cast<T*>(g.out);
    constexpr int CG = BN / 8;
    for (int e = etid; e < rows * CG; e += ET) {
      const int rr = e / CG, cg = e % CG;
      const int col = n0 + cg * 8;
      if (col < g.Ncols) {
        V8<T> o;
        o.load(El + rr * EP + cg * 8);
        o.store(out_at<T>(g, row_vox(rr), col));
      }
    }
  } else {
    float* El = reinterpret_cast<float*>(lds4);
    constexpr int EP = BN + 4;
    if (!half) {
#pragma unroll
      for (int j = 0; j < RN; ++j) {
        const int col = j * 16 + r16;
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) El[(wave * 64 + i * 16 + kg * 4 + r) * EP + col] = acc[i][j][r];
      }
    }
    __syncthreads();
    constexpr int CG = BN / 4;
    for (int e = etid; e < rows * CG; e += ET) {
      const int rr = e / CG, cg = e % CG;
      const int col = n0 + cg * 4;
      if (col < g.Ncols) {
        const float4 v = *reinterpret_cast<const float4*>(El + rr * EP + cg * 4);
        *reinterpret_cast<float4*>(g.part + ((long long)ks * g.M + row_vox(rr)) * g.Ncols + col) = v;
      }
    }
  }
}

// The instantiation for the brick, column tile and staging choose_gemm chose, on the grid it gave.
template <typename T>
void launch_brickr_t(const GemmArgs& g, const GemmChoice& c, hipStream_t s) {
  const dim3 grid(c.grid), block(c.block);
  // compile-time bricks: 6 x 6 x 6 (the 12^3 / 6^3 levels) and 4 x 8 x 8 (the grouped 48^3 / 24^3 levels)
  const bool b666 = c.bz == 6 && c.by == 6 && c.bx == 6;
  const bool b488 = c.bz == 4 && c.by == 8 && c.bx == 8;
  const bool rb32 = c.b32;
  if (c.bn == 64) {
    if constexpr (sizeof(T) == 2) {
      if (b666 && rb32)
        MMSEG_LAUNCH((conv3_brickr_kernel<T, 64, 6, 6, 6, false, true>), grid, block, 0, s, g, 6, 6, 6);
      else if (b666)
        MMSEG_LAUNCH((conv3_brickr_kernel<T, 64, 6, 6, 6>), grid, block, 0, s, g, 6, 6, 6);
      else if (b488 && rb32)
        MMSEG_LAUNCH((conv3_brickr_kernel<T, 64, 4, 8, 8, false, true>), grid, block, 0, s, g, 4, 8, 8);
      else if (b488)
        MMSEG_LAUNCH((conv3_brickr_kernel<T, 64, 4, 8, 8>), grid, block, 0, s, g, 4, 8, 8);
      else if (rb32)
        MMSEG_LAUNCH((conv3_brickr_kernel<T, 64, 0, 0, 0, false, true>), grid, block, 0, s, g, c.bz, c.by, c.bx);
      else
        MMSEG_LAUNCH((conv3_brickr_kernel<T, 64>), grid, block, 0, s, g, c.bz, c.by, c.bx);
    }
  } else if (c.kw2) {
    if constexpr (sizeof(T) == 2) {   // (the fp32 form's two stage sets exceed the LDS)
      const dim3 b2(c.block);
      if (rb32)
        MMSEG_LAUNCH((conv3_brickr_kernel<T, 32, 6, 6, 6, true, true, 2>), grid, b2, 0, s, g, 6, 6, 6);
      else
        MMSEG_LAUNCH((conv3_brickr_kernel<T, 32, 6, 6, 6, true, false, 2>), grid, b2, 0, s, g, 6, 6, 6);
    }
  } else if (b666 && rb32) {
    MMSEG_LAUNCH((conv3_brickr_kernel<T, 32, 6, 6, 6, true, true>), grid, block, 0, s, g, 6, 6, 6);
  } else if (b666) {
    MMSEG_LAUNCH((conv3_brickr_kernel<T, 32, 6, 6, 6>), grid, block, 0, s, g, 6, 6, 6);
  } else if (b488 && rb32) {
    MMSEG_LAUNCH((conv3_brickr_kernel<T, 32, 4, 8, 8, false, true>), grid, block, 0, s, g, 4, 8, 8);
  } else if (b488) {
    MMSEG_LAUNCH((conv3_brickr_kernel<T, 32, 4, 8, 8>), grid, block, 0, s, g, 4, 8, 8);
  } else if (rb32) {
    MMSEG_LAUNCH((conv3_brickr_kernel<T, 32, 0, 0, 0, false, true>), grid, block, 0, s, g, c.bz, c.by, c.bx);
  } else {
    MMSEG_LAUNCH((conv3_brickr_kernel<T, 32>), grid, block, 0, s, g, c.bz, c.by, c.bx);
  }
}

}  // namespace

MMSEG_LOCAL void launch_brickr(const GemmArgs& g, const GemmChoice& c, hipStream_t s) {
  if (c.tsize == 2) launch_brickr_t<bf16_t>(g, c, s);
  else launch_brickr_t<float>(g, c, s);
}
