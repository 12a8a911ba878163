// The weight gradients of the GEMM-shaped ops: the kernels, the chooser of the 3^3 weight gradient, their launcher
// and entry points, and the column sums of the bias gradient.
//
// wgrad (dW = sum over voxels) runs as a second kernel with K = voxels: both
// operands are staged through LDS transposed (channel-major) and reduced in a
// fixed-order split-K pass, so weight gradients are bitwise deterministic.
//
// Every weight-gradient kernel stays in this one source: wgrad_dma_kernel shares a device helper with
// wgrad_brick2_kernel and wgrad_brickr_kernel, and its <CO32> epilogue compiles differently in a source without them.
#include "conv_common.h"

#include <algorithm>
#include <type_traits>

namespace {

// ------------------------------------------------------------------ wgrad
// part[ks][row][col] = sum_{v in split ks} A[v][row] * Bgather[v][col]
//   CONV3 : A = dy (rows = Cout), B = x at v + off(tap), col = tap*Cin + ci
//   POINT : A = dy, B = x at v
//   CONVT : A = x (rows = Cin), B = dy at child(v, tap), col = tap*Cout + co
// Both operands are staged into LDS in their natural [voxel][channel] layout
// with 16-byte vector writes (double-buffered, one barrier per stage); the
// MFMA fragments (K = voxels) are read with the gfx950 transposed LDS read
// ds_read_b64_tr_b16 (bf16) or as single f32 elements (f32 path).
// bias_part (optional): the bias gradient partials.  A = dy (CONV3 / POINT): blocks of column tile 0 emit
// per-row sums of A, bias_part[ks][Ca].  CONVT: blocks of row tile 0 emit per-column sums of the gathered dy
// tile B, bias_part[ks][8 Cout] (col = tap*Cout + co), which mmseg_colsum_reduce folds over (ks, tap): the
// separate colsum pass over dy (113 MB at the 96^3 upconv) is not needed.
struct WgradArgs {
  const void* a;  int lda;
  const void* b;  int ldb;
  float* part;
  float* bias_part;
  int Ca, Ncols, cpg_shift;
  long long V;               // voxels in the a-grid
  int D, H, W;
  int ksplit;
  long long vox_per_split;   // multiple of KV
  int swz;
  int brick;                 // CONV3 only: ksplit splits the brick list instead of voxels
  // brick2 / brickr kernels (CONV3, bf16) write channel-major tiles (col = ci*27 + tap, the torch
  // order of grad[co][ci][3][3][3]); with ksplit == 1 and grad != null straight into the gradient.
  float* grad;
  float* bias_grad;
  int accumulate;
  int kchunks;               // CONV3 brick kernels: 32-channel chunks of x holding real channels (0 = all)
  // deferred InstanceNorm + ReLU of x (wgrad_brick2 only, mmseg_conv3_wgrad_norm): x holds the PRE-norm
  // activation, staged as relu((x - nmean[n][c]) * nrstd[n][c]) rounded to T
  const float* nmean;
  const float* nrstd;
  int frag;  // wgrad_dma: split partials in the fragment-native layout (Conv3WgradChoice::fmt, WReduceArgs::frag_mt)
  int groups;  // grouped launch (wgrad_brickr only): the bricks are `groups` equal sample groups, splits
               // [gi * ksplit / groups, (gi + 1) * ksplit / groups) cover group gi's bricks only
  // grouped with one split per group (ksplit == groups) and grad != null: split gi writes group gi's gradient
  // straight to grad + gi * grad_gstride (bias_grad + gi * bias_gstride), no partials and no reduce
  long long grad_gstride;
  int bias_gstride;
  int grad_ld;   // direct gradient row pitch (27 x real input channels; 0 = Ncols), wgrad_direct_ok
  int pad16;   // mmseg_conv3_wgrad_ex phase bit 8: rows [Ca - 16, Ca) are output-channel padding (48 real of 64: the
               // SwinUNETR 48-channel levels); wgrad_dma's 64-co tile then runs 3 of its 4 MFMA row tiles, zero rows
};

// the launch writes the gradient itself: one split, or one split per group of a grouped launch
__device__ __forceinline__ bool wgrad_direct(const WgradArgs& g) {
  return g.ksplit == 1 || (g.groups > 1 && g.ksplit == g.groups);
}

__host__ __device__ __forceinline__ int wgrad_nchunk(int cpg_shift, int kchunks) {
  const int n = (8 << cpg_shift) / 32;
  return (kchunks > 0 && kchunks < n) ? kchunks : n;
}

typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef short v8i16 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) v4i16 lds_v4i16;

__device__ __forceinline__ bf16x8 tr_frag(const bf16_t* p_lo, const bf16_t* p_hi) {
  v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(p_lo));
  v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(p_hi));
  v8i16 c = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, c);
}

template <int MODE>
__device__ __forceinline__ bool gather_src(long long vox, int kgi, int cpg_shift, const WgradArgs& g, long long& src,
                                           int& c8) {
  if (MODE == MODE_CONV3) {
    const int t = kgi >> cpg_shift;
    c8 = kgi & ((1 << cpg_shift) - 1);
    // 32-bit divisions (V < 2^31, checked by the host)
    const unsigned vu = (unsigned)vox;
    const unsigned q = vu / (unsigned)g.W, q2 = q / (unsigned)g.H;
    const int x = (int)(vu - q * (unsigned)g.W), y = (int)(q - q2 * (unsigned)g.H), z = (int)(q2 % (unsigned)g.D);
    int dz, dy, dx;
    tap_delta(t, dz, dy, dx);
    src = vox + ((long long)dz * g.H + dy) * g.W + dx;
    return (unsigned)(z + dz) < (unsigned)g.D && (unsigned)(y + dy) < (unsigned)g.H &&
           (unsigned)(x + dx) < (unsigned)g.W;
  } else if (MODE == MODE_CONVT_DGRAD) {
    const int t = kgi >> cpg_shift;
    c8 = kgi & ((1 << cpg_shift) - 1);
    const unsigned vu = (unsigned)vox;
    const unsigned q = vu / (unsigned)g.W, q2 = q / (unsigned)g.H, n = q2 / (unsigned)g.D;
    const unsigned x = vu - q * (unsigned)g.W, y = q - q2 * (unsigned)g.H, z = q2 - n * (unsigned)g.D;
    src = (((long long)n * 2LL * g.D + 2 * z + (t >> 2)) * 2LL * g.H + 2 * y + ((t >> 1) & 1)) * 2LL * g.W + 2 * x +
          (t & 1);
    return true;
  }
  c8 = kgi;
  src = vox;
  return true;
}

template <typename T, int MODE, int WM, int WN, int RM, int RN, int KV>
__global__ __launch_bounds__(256) void wgrad_kernel(WgradArgs g) {
  constexpr int BM = WM * RM * 16;
  constexpr int BN = WN * RN * 16;
  constexpr int EP = 16 / sizeof(T);
  constexpr int PA = BM + EP, PB = BN + EP;      // LDS row pitch (elements), 16-B aligned rows
  constexpr int AG = BM / 8, BG = BN / 8;
  constexpr int A_PER = KV * AG / 256, B_PER = KV * BG / 256;
  static_assert(A_PER >= 1 && B_PER >= 1 && (256 % AG) == 0 && (256 % BG) == 0, "tile/thread mismatch");
  constexpr int SA = KV * PA, SB = KV * PB;
  __shared__ __attribute__((aligned(16))) T lds[2 * (SA + SB)];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int ct_n = (g.Ncols + BN - 1) / BN, rt_n = (g.Ca + BM - 1) / BM;
  const int tile = g.swz ? xcd_swizzle(blockIdx.x, ct_n * rt_n * g.ksplit) : (int)blockIdx.x;
  const int ctile = tile % ct_n, rtile = (tile / ct_n) % rt_n, ks = tile / (ct_n * rt_n);
  const int row0 = rtile * BM;
  const int col0 = ctile * BN;
  const long long v_begin = ks * g.vox_per_split;
  long long v_end = v_begin + g.vox_per_split;
  if (v_end > g.V) v_end = g.V;
  const T* A = reinterpret_cast<const T*>(g.a);
  const T* B = reinterpret_cast<const T*>(g.b);
  constexpr bool BCOL = MODE == MODE_CONVT_DGRAD;   // bias = column sums of B (see above)
  const bool do_bias = g.bias_part != nullptr && (BCOL ? rtile == 0 : ctile == 0);

  // fixed per-thread column group (256 % BG == 0) -> fixed tap / channel group
  const int cga = tid % AG, cgb = tid % BG;
  const int kgi_b = (col0 >> 3) + cgb;
  const bool col_ok = kgi_b * 8 < g.Ncols;
  const bool row_ok = row0 + cga * 8 < g.Ca;

  f32x4 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bsum[8] = {0, 0, 0, 0, 0, 0, 0, 0};

  V8<T> ra[A_PER], rb[B_PER];
  // transposed conv: the thread's B voxels step by KV per stage, so their (n, z, y, x) are decomposed once and
  // stepped (gather_src's three runtime divisions per load were ~29 VALU per MFMA, r04i PMC)
  int cx[B_PER], cy[B_PER], cz[B_PER], cn[B_PER];
  const int t_b = kgi_b >> g.cpg_shift, c8_b = kgi_b & ((1 << g.cpg_shift) - 1);
  if constexpr (MODE == MODE_CONVT_DGRAD) {
#pragma unroll
    for (int k = 0; k < B_PER; ++k) {
      const unsigned vu = (unsigned)(v_begin + (tid + k * 256) / BG);
      const unsigned q = vu / (unsigned)g.W, q2 = q / (unsigned)g.H;
      cn[k] = (int)(q2 / (unsigned)g.D);
      cz[k] = (int)(q2 - (unsigned)cn[k] * (unsigned)g.D);
      cy[k] = (int)(q - q2 * (unsigned)g.H);
      cx[k] = (int)(vu - q * (unsigned)g.W);
    }
  }
  auto load_stage = [&](long long vb) {
#pragma unroll
    for (int k = 0; k < A_PER; ++k) {
      const int v = (tid + k * 256) / AG;
      const long long vox = vb + v;
      if (vox < v_end && row_ok) ra[k].load(A + vox * g.lda + row0 + cga * 8);
      else ra[k].zero();
    }
#pragma unroll
    for (int k = 0; k < B_PER; ++k) {
      const int v = (tid + k * 256) / BG;
      const long long vox = vb + v;
      if constexpr (MODE == MODE_CONVT_DGRAD) {
        const unsigned src = (((unsigned)cn[k] * 2u * g.D + 2u * cz[k] + (t_b >> 2)) * 2u * g.H + 2u * cy[k] +
                              ((t_b >> 1) & 1)) * 2u * g.W + 2u * cx[k] + (t_b & 1);
        if (vox < v_end && col_ok) rb[k].load(B + (long long)src * g.ldb + c8_b * 8);
        else rb[k].zero();
        // step to the voxel KV further on (the next stage): one division for the x carry (KV may span several
        // rows of a small grid), then y / z wrap at most a few times
        cx[k] += KV;
        if (cx[k] >= g.W) {
          const int qy = (int)((unsigned)cx[k] / (unsigned)g.W);
          cx[k] -= qy * g.W;
          cy[k] += qy;
          while (cy[k] >= g.H) {
            cy[k] -= g.H;
            if (++cz[k] == g.D) {
              cz[k] = 0;
              ++cn[k];
            }
          }
        }
      } else {
        long long src;
        int c8;
        const bool ok = vox < v_end && col_ok && gather_src<MODE>(vox, kgi_b, g.cpg_shift, g, src, c8);
        if (ok) rb[k].load(B + src * g.ldb + c8 * 8);
        else rb[k].zero();
      }
    }
  };
  auto write_stage = [&](int buf) {
    T* As = lds + buf * (SA + SB);
    T* Bs = As + SA;
#pragma unroll
    for (int k = 0; k < A_PER; ++k) {
      const int v = (tid + k * 256) / AG;
      ra[k].store(As + v * PA + cga * 8);
      if (!BCOL && do_bias) {
#pragma unroll
        for (int j = 0; j < 8; ++j) bsum[j] += ra[k].get(j);
      }
    }
#pragma unroll
    for (int k = 0; k < B_PER; ++k) {
      const int v = (tid + k * 256) / BG;
      rb[k].store(Bs + v * PB + cgb * 8);
      if (BCOL && do_bias) {
#pragma unroll
        for (int j = 0; j < 8; ++j) bsum[j] += rb[k].get(j);
      }
    }
  };

  const int g4 = lane >> 4, i16 = lane & 15, q = i16 >> 2, p4 = i16 & 3;
  int buf = 0;
  if (v_begin < v_end) {
    load_stage(v_begin);
    write_stage(0);
  }
  __syncthreads();
  for (long long vb = v_begin; vb < v_end; vb += KV) {
    const bool more = vb + KV < v_end;
    if (more) load_stage(vb + KV);
    const T* As = lds + buf * (SA + SB);
    const T* Bs = As + SA;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int kk = 0; kk < KV; kk += 32) {
        bf16x8 af[RM], bfr[RN];
#pragma unroll
        for (int i = 0; i < RM; ++i) {
          const bf16_t* base = (const bf16_t*)As + (kk + 8 * g4 + q) * PA + wm * RM * 16 + i * 16 + 4 * p4;
          af[i] = tr_frag(base, base + 4 * PA);
        }
#pragma unroll
        for (int j = 0; j < RN; ++j) {
          const bf16_t* base = (const bf16_t*)Bs + (kk + 8 * g4 + q) * PB + wn * RN * 16 + j * 16 + 4 * p4;
          bfr[j] = tr_frag(base, base + 4 * PB);
        }
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int j = 0; j < RN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
      }
    } else {
#pragma unroll 4
      for (int kk = 0; kk < KV; kk += 4) {
        float af[RM], bfr[RN];
#pragma unroll
        for (int i = 0; i < RM; ++i) af[i] = (float)As[(kk + g4) * PA + wm * RM * 16 + i * 16 + i16];
#pragma unroll
        for (int j = 0; j < RN; ++j) bfr[j] = (float)Bs[(kk + g4) * PB + wn * RN * 16 + j * 16 + i16];
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int j = 0; j < RN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bfr[j], acc[i][j], 0, 0, 0);
      }
    }
    if (more) write_stage(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) {
      const int col = col0 + wn * RN * 16 + j * 16 + (lane & 15);
      if (col >= g.Ncols) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + wm * RM * 16 + i * 16 + (lane >> 4) * 4 + r;
        if (row >= g.Ca) continue;
        g.part[((long long)ks * g.Ca + row) * g.Ncols + col] = acc[i][j][r];
      }
    }
  if (do_bias) {
    // fixed-order reduction of the per-thread row (column) sums: threads with equal tid % AG (tid % BG) share
    // rows (columns)
    float* red = reinterpret_cast<float*>(lds);
#pragma unroll
    for (int j = 0; j < 8; ++j) red[tid * 8 + j] = bsum[j];
    __syncthreads();
    if (BCOL) {
      if (tid < BN) {
        const int cg = tid >> 3, j = tid & 7;
        float sacc = 0.f;
        for (int t = cg; t < 256; t += BG) sacc += red[t * 8 + j];
        if (col0 + tid < g.Ncols) g.bias_part[(long long)ks * g.Ncols + col0 + tid] = sacc;
      }
    } else if (tid < BM) {
      const int cg = tid >> 3, j = tid & 7;
      float sacc = 0.f;
      for (int t = cg; t < 256; t += AG) sacc += red[t * 8 + j];
      if (row0 + tid < g.Ca) g.bias_part[(long long)ks * g.Ca + row0 + tid] = sacc;
    }
  }
}

// ------------------------------------------------------- brick wgrad (3^3)
// dW[co][tap][ci] partials with the input halo reused by all 27 taps: a block
// owns 32 output channels x one 32-channel input chunk x ALL 27 taps, and walks
// a contiguous range of 4x4x8 bricks.  Per brick it stages dy [128 vox][32 co]
// and the x halo [6x6x10][32 ci] into LDS; K = the brick's 128 voxels.  The
// MFMA operands are read with ds_read_b64_tr_b16 (K = voxels is the strided
// dimension of NDHWC): the A rows come from the dy tile, the B rows from halo
// rows shifted by the tap (4 arbitrary row addresses per 16-lane group).
// Wave w accumulates taps [7w, 7w+7) -> 2 x 7 x 2 MFMA tiles in registers.
template <typename T>
__global__ __launch_bounds__(256) void wgrad_brick_kernel(WgradArgs g) {
  constexpr int EP = 16 / sizeof(T);
  constexpr int DP = 32 + EP;                    // dy tile pitch
  constexpr int XP = CK + EP;                    // halo pitch
  constexpr int DS = 128 * DP, XS = HLO_V * XP;
  __shared__ __attribute__((aligned(16))) T lds[DS + XS];
  T* Dl = lds;
  T* Xl = lds + DS;
  constexpr int D_ITEMS = 128 * 4, X_ITEMS = HLO_V * 4;
  constexpr int D_PER = D_ITEMS / 256, X_PER = (X_ITEMS + 255) / 256;

  const T* Dy = reinterpret_cast<const T*>(g.a);
  const T* X = reinterpret_cast<const T*>(g.b);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cin = 8 << g.cpg_shift;
  const int nchunk = wgrad_nchunk(g.cpg_shift, g.kchunks), rt_n = g.Ca / 32;
  const int tile = blockIdx.x;
  const int ct = tile % nchunk, rt = (tile / nchunk) % rt_n, ks = tile / (nchunk * rt_n);
  const int bz_n = g.D / BRK_Z, by_n = g.H / BRK_Y, bx_n = g.W / BRK_X;
  const long long nbrick = (g.V / ((long long)g.D * g.H * g.W)) * bz_n * by_n * bx_n;
  const long long bpk = (nbrick + g.ksplit - 1) / g.ksplit;
  const long long b_begin = ks * bpk;
  const long long b_end = b_begin + bpk < nbrick ? b_begin + bpk : nbrick;
  const long long HW = (long long)g.H * g.W;
  const int row0 = rt * 32, c0 = ct * CK;
  const bool do_bias = g.bias_part != nullptr && ct == 0;
  const int t_begin = wave * 7, t_cnt = wave == 3 ? 6 : 7;

  f32x4 acc[2][7][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < 7; ++t)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bsum[8] = {0, 0, 0, 0, 0, 0, 0, 0};

  V8<T> dr[D_PER], xr[X_PER];
  auto brick_origin = [&](long long b, long long& nbase, int& z0, int& y0, int& x0) {
    int q = (int)b;   // brick index < V / 128 < 2^31 (mmseg_wgrad): 32-bit division
    const int bx = q % bx_n;
    q /= bx_n;
    const int by = q % by_n;
    q /= by_n;
    const int bz = q % bz_n;
    const long long n = q / bz_n;
    nbase = n * g.D * HW;
    z0 = bz * BRK_Z;
    y0 = by * BRK_Y;
    x0 = bx * BRK_X;
  };
  auto load = [&](long long b) {
    long long nbase;
    int z0, y0, x0;
    brick_origin(b, nbase, z0, y0, x0);
#pragma unroll
    for (int k = 0; k < D_PER; ++k) {
      const int e = tid + k * 256, v = e >> 2, cg = e & 3;
      const int z = z0 + (v >> 5), y = y0 + ((v >> 3) & 3), x = x0 + (v & 7);
      dr[k].load(Dy + (nbase + z * HW + (long long)y * g.W + x) * g.lda + row0 + cg * 8);
    }
#pragma unroll
    for (int k = 0; k < X_PER; ++k) {
      const int e = tid + k * 256;
      if (e < X_ITEMS) {
        const int h = e >> 2, cg = e & 3;
        const int hx = h % HLO_X, hy = (h / HLO_X) % HLO_Y, hz = h / (HLO_X * HLO_Y);
        const int z = z0 - 1 + hz, y = y0 - 1 + hy, x = x0 - 1 + hx;
        if ((unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H && (unsigned)x < (unsigned)g.W)
          xr[k].load(X + (nbase + z * HW + (long long)y * g.W + x) * g.ldb + c0 + cg * 8);
        else
          xr[k].zero();
      }
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int k = 0; k < D_PER; ++k) {
      const int e = tid + k * 256;
      dr[k].store(Dl + (e >> 2) * DP + (e & 3) * 8);
      if (do_bias) {
#pragma unroll
        for (int j = 0; j < 8; ++j) bsum[j] += dr[k].get(j);
      }
    }
#pragma unroll
    for (int k = 0; k < X_PER; ++k) {
      const int e = tid + k * 256;
      if (e < X_ITEMS) xr[k].store(Xl + (e >> 2) * XP + (e & 3) * 8);
    }
  };

  const int g4 = lane >> 4, i16 = lane & 15, q = i16 >> 2, p4 = i16 & 3;
  if (b_begin < b_end) {
    load(b_begin);
    store();
  }
  __syncthreads();
  for (long long b = b_begin; b < b_end; ++b) {
    const bool more = b + 1 < b_end;
    if (more) load(b + 1);
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int kk = 0; kk < 128; kk += 32) {
        bf16x8 af[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const bf16_t* base = (const bf16_t*)Dl + (kk + 8 * g4 + q) * DP + i * 16 + 4 * p4;
          af[i] = tr_frag(base, base + 4 * DP);
        }
        // B rows: voxels v = kk + 8*g4 + q (+4) -> halo row of (v) shifted by the tap
        const int v_lo = kk + 8 * g4 + q, v_hi = v_lo + 4;
        const int hlo = ((v_lo >> 5) * HLO_Y + ((v_lo >> 3) & 3)) * HLO_X + (v_lo & 7);
        const int hhi = ((v_hi >> 5) * HLO_Y + ((v_hi >> 3) & 3)) * HLO_X + (v_hi & 7);
#pragma unroll
        for (int t = 0; t < 7; ++t) {
          if (t < t_cnt) {
            const int tap = t_begin + t;
            const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
            const int hoff = (kz * HLO_Y + ky) * HLO_X + kx;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const bf16_t* pl = (const bf16_t*)Xl + (hlo + hoff) * XP + j * 16 + 4 * p4;
              const bf16_t* ph = (const bf16_t*)Xl + (hhi + hoff) * XP + j * 16 + 4 * p4;
              const bf16x8 bfr = tr_frag(pl, ph);
#pragma unroll
              for (int i = 0; i < 2; ++i)
                acc[i][t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr, acc[i][t][j], 0, 0, 0);
            }
          }
        }
      }
    } else {
      for (int kk = 0; kk < 128; kk += 4) {
        const int v = kk + g4;
        const int hv = ((v >> 5) * HLO_Y + ((v >> 3) & 3)) * HLO_X + (v & 7);
        float af[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) af[i] = (float)Dl[v * DP + i * 16 + i16];
#pragma unroll
        for (int t = 0; t < 7; ++t) {
          if (t < t_cnt) {
            const int tap = t_begin + t;
            const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
            const int hoff = (kz * HLO_Y + ky) * HLO_X + kx;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const float bv = (float)Xl[(hv + hoff) * XP + j * 16 + i16];
#pragma unroll
              for (int i = 0; i < 2; ++i)
                acc[i][t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bv, acc[i][t][j], 0, 0, 0);
            }
          }
        }
      }
    }
    __syncthreads();
    if (more) {
      store();
      __syncthreads();
    }
  }

  // partial layout [ks][Ca][Ncols], col = tap*cin + ci
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      if (t >= t_cnt) continue;
      const int tap = t_begin + t;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = tap * cin + c0 + j * 16 + i16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = row0 + i * 16 + g4 * 4 + r;
          g.part[((long long)ks * g.Ca + row) * g.Ncols + col] = acc[i][t][j][r];
        }
      }
    }
  if (do_bias) {
    float* red = reinterpret_cast<float*>(lds);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) red[tid * 8 + j] = bsum[j];
    __syncthreads();
    if (tid < 32) {
      const int cg = tid >> 3, j = tid & 7;
      float sacc = 0.f;
      for (int t = cg; t < 256; t += 4) sacc += red[t * 8 + j];
      g.bias_part[(long long)ks * g.Ca + row0 + tid] = sacc;
    }
  }
}


// Epilogue of the brick wgrad kernels (8 waves, acc[t][i][j] = rows i*16.., input channels j*16.., tap
// t_begin + t): the block's [MT*16 co][32 ci][27 taps] fp32 tile goes through LDS 16 co-rows at a time and
// leaves as contiguous float4 rows in channel-major order (torch grad[co][ci][tap] order), either into the
// split partial part[ks][Ca][Ncols] or, for a single split, straight into the gradient (= or +=).
// LDS pitch 868 floats: a ds_write_b32 lane group (two co-rows x 16 ci, ci stride 27) hits 32 distinct banks.
constexpr int WEP_P = 868;
// RP rows of the 16-row MFMA tile per LDS pass (16: 55.5 KB of staging; 8: half that, two passes)
template <int MT, int RP = 16>
__device__ __forceinline__ void wgrad_store_chmajor(const f32x4 (&acc)[4][MT][2], int t_begin, int t_cnt, float* L,
                                                    const WgradArgs& g, int ks, int row0, int c0) {
  const int tid = threadIdx.x, lane = tid & 63, g4 = lane >> 4, i16 = lane & 15;
  const bool direct = g.grad != nullptr && wgrad_direct(g);
  float* base = direct ? g.grad + (g.ksplit > 1 ? (long long)ks * g.grad_gstride : 0LL)
                       : g.part + (long long)ks * g.Ca * g.Ncols;
  const long long ldg = direct && g.grad_ld > 0 ? g.grad_ld : g.Ncols;   // gradient row pitch (real channels)
  const bool accum = direct && g.accumulate;
  constexpr int GP = RP / 4;   // lane groups per pass
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int hh = 0; hh < 16 / RP; ++hh) {
      __syncthreads();
      if (g4 / GP == hh) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (t >= t_cnt) continue;
          const int tap = t_begin + t;
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) L[((g4 % GP) * 4 + r) * WEP_P + (j * 16 + i16) * 27 + tap] = acc[t][i][j][r];
        }
      }
      __syncthreads();
      for (int e = tid; e < RP * 216; e += 512) {
        const int rr = e / 216, q = e - rr * 216;
        const float4 v = *reinterpret_cast<const float4*>(L + rr * WEP_P + q * 4);
        float4* d = reinterpret_cast<float4*>(base + (long long)(row0 + i * 16 + hh * RP + rr) * ldg + c0 * 27 +
                                              q * 4);
        if (accum) {
          const float4 o = *d;
          *d = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
        } else {
          *d = v;
        }
      }
    }
  }
}

template <int CG>
__device__ __forceinline__ void wgrad_store_bias(const float (&bsum)[8], float* red, const WgradArgs& g, int ks,
                                                 int row0) {
  constexpr int CO = CG * 8;
  const int tid = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; ++j) red[tid * 8 + j] = bsum[j];
  __syncthreads();
  if (tid < CO) {
    const int cg = tid >> 3, j = tid & 7;
    float sacc = 0.f;
    for (int t = cg; t < 512; t += CG) sacc += red[t * 8 + j];
    if (g.bias_grad != nullptr && wgrad_direct(g)) {
      float* bg = g.bias_grad + (g.ksplit > 1 ? ks * g.bias_gstride : 0) + row0 + tid;
      *bg = g.accumulate ? *bg + sacc : sacc;
    } else {
      g.bias_part[(long long)ks * g.Ca + row0 + tid] = sacc;
    }
  }
}

// ------------------------------------------------ brick wgrad v2 (3^3)
// 8 waves, 64 output channels x one 32-channel input chunk x all 27 taps per
// block (wgrad_brick_kernel has 32 x 32): each tap-shifted halo fragment now
// feeds 4 MFMAs instead of 2 and one staged halo serves twice the output
// channels, so LDS reads and L2 traffic per MAC drop by a third.  Taps are
// dealt 4,4,4,3,3,3,3,3 over the waves (acc: 4 taps x 4 x 2 tiles = 128
// VGPRs).  The two LDS stage buffers alternate, one barrier per brick.
// V = 3 (default): bank-conflict-free transposed reads.  A ds_read_b64_tr_b16 half-wave reads 8 tile rows
// x 16 columns; with the K order below those 8 rows are 8 consecutive voxels (one x-row of the brick: lane
// group g4, element j -> x = 4*(g4&1) + (j&3), y = 2*(g4>>1) + (j>>2)) in BOTH the dy tile and the halo, and
// with row pitches of 24 or 40 dwords (== 8 mod 16) 8 consecutive rows cover the 64 banks exactly once.
// V = 2: the previous K order (x = j&3 + 4*(j>>2), y = g4) with 20-dword pitches, 2-way conflicted
// (SQ_LDS_BANK_CONFLICT = half the LDS-active cycles at 96^3).
// NORM: x holds a pre-norm activation (g.nmean / g.nrstd, mmseg_conv3_wgrad_norm); a separate instantiation so
// the plain kernel does not carry the statistics' registers (256 VGPRs + spills for CO64 otherwise)
// PIPE (bf16, V = 3): the software-pipelined multiply of wgrad_dma_kernel's PIPE form -- halo fragments two
// (dy plane, tap) steps ahead in a ring of three, dy fragments one plane ahead -- instead of reading each tap's
// fragments into the registers the previous tap's MFMAs just released (read, wait, 4 MFMAs, per tap).
template <typename T, int MT, int V, bool NORM = false, bool PIPE = false>
__global__ __launch_bounds__(512, (MT == 2 && V == 2) ? 2 : 1) void wgrad_brick2_kernel(WgradArgs g) {
  static_assert(!PIPE || (V == 3 && sizeof(T) == 2), "PIPE: bf16 with the V = 3 fragment order");
  constexpr int EP = 16 / sizeof(T);
  constexpr int CO = MT * 16, CG = CO / 8;       // output channels per block, 8-channel groups
  constexpr int DP = V == 3 ? (MT == 2 ? 48 : 80) : CO + EP;   // dy tile pitch (elements)
  constexpr int XP = V == 3 ? 48 : CK + EP;                    // halo pitch
  constexpr int DS = 128 * DP, XS = HLO_V * XP;
  __shared__ __attribute__((aligned(16))) T lds[2 * (DS + XS)];
  constexpr int D_ITEMS = 128 * CG, X_ITEMS = HLO_V * 4;
  constexpr int D_PER = D_ITEMS / 512, X_PER = (X_ITEMS + 511) / 512;

  const T* Dy = reinterpret_cast<const T*>(g.a);
  const T* X = reinterpret_cast<const T*>(g.b);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cin = 8 << g.cpg_shift;
  const int nchunk = wgrad_nchunk(g.cpg_shift, g.kchunks), rt_n = g.Ca / CO;
  const int tile = g.swz ? xcd_swizzle(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int ct = tile % nchunk, rt = (tile / nchunk) % rt_n, ks = tile / (nchunk * rt_n);
  const int bz_n = g.D / BRK_Z, by_n = g.H / BRK_Y, bx_n = g.W / BRK_X;
  const long long nbrick = (g.V / ((long long)g.D * g.H * g.W)) * bz_n * by_n * bx_n;
  const long long bpk = (nbrick + g.ksplit - 1) / g.ksplit;
  const long long b_begin = ks * bpk;
  const long long b_end = b_begin + bpk < nbrick ? b_begin + bpk : nbrick;
  const long long HW = (long long)g.H * g.W;
  const int row0 = rt * CO, c0 = ct * CK;
  const bool do_bias = g.bias_part != nullptr && ct == 0;
  // wave-uniform (SGPRs): the per-tap halo offsets are scalar, and the pipelined multiply branches on t_cnt
  const int t_begin = __builtin_amdgcn_readfirstlane(wave < 3 ? 4 * wave : 12 + 3 * (wave - 3));
  const int t_cnt = __builtin_amdgcn_readfirstlane(wave < 3 ? 4 : 3);

  f32x4 acc[4][MT][2];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[t][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bsum[8] = {0, 0, 0, 0, 0, 0, 0, 0};

  V8<T> dr[D_PER], xr[X_PER];
  uint32_t xin = 0;    // bit k: xr[k] is an in-volume voxel (padding stays 0 under the deferred norm)
  int xn = 0;          // sample of the staged brick
  int norm_n = -1;     // sample whose deferred-norm statistics nmu / nrs hold
  float nmu[NORM ? 8 : 1], nrs[NORM ? 8 : 1];
  auto load_into = [&](long long b, auto& dr, auto& xr, uint32_t& xin, int& xn) {
    int q = (int)b;   // brick index < V / 128 < 2^31 (mmseg_wgrad): 32-bit division
    const int bx = q % bx_n;
    q /= bx_n;
    const int by = q % by_n;
    q /= by_n;
    const int bz = q % bz_n;
    xn = q / bz_n;
    const long long nbase = (long long)xn * g.D * HW;
    const int z0 = bz * BRK_Z, y0 = by * BRK_Y, x0 = bx * BRK_X;
    xin = 0;
#pragma unroll
    for (int k = 0; k < D_PER; ++k) {
      const int e = tid + k * 512, v = e / CG, cg = e % CG;
      const int z = z0 + (v >> 5), y = y0 + ((v >> 3) & 3), x = x0 + (v & 7);
      dr[k].load(Dy + (nbase + z * HW + (long long)y * g.W + x) * g.lda + row0 + cg * 8);
    }
#pragma unroll
    for (int k = 0; k < X_PER; ++k) {
      const int e = tid + k * 512;
      if (e < X_ITEMS) {
        const int h = e >> 2, cg = e & 3;
        const int hx = h % HLO_X, hy = (h / HLO_X) % HLO_Y, hz = h / (HLO_X * HLO_Y);
        const int z = z0 - 1 + hz, y = y0 - 1 + hy, x = x0 - 1 + hx;
        if ((unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H && (unsigned)x < (unsigned)g.W) {
          xr[k].load(X + (nbase + z * HW + (long long)y * g.W + x) * g.ldb + c0 + cg * 8);
          if constexpr (NORM) xin |= 1u << k;
        } else {
          xr[k].zero();
        }
      }
    }
  };
  auto store_from = [&](int buf, auto& dr, auto& xr, uint32_t xin, int xn) {
    T* Dl = lds + buf * (DS + XS);
    T* Xl = Dl + DS;
#pragma unroll
    for (int k = 0; k < D_PER; ++k) {
      const int e = tid + k * 512;
      dr[k].store(Dl + (e / CG) * DP + (e % CG) * 8);
      if (do_bias) {
#pragma unroll
        for (int j = 0; j < 8; ++j) bsum[j] += dr[k].get(j);
      }
    }
    if constexpr (NORM) {   // deferred InstanceNorm + ReLU of x: channels c0 + 8 (tid & 3) .. of sample xn
      if (xn != norm_n) {   // (the statistics change only when the brick range crosses into the next sample)
        norm_n = xn;
        const int cb = xn * cin + c0 + (tid & 3) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          nmu[j] = g.nmean[cb + j];
          nrs[j] = g.nrstd[cb + j];
        }
      }
#pragma unroll
      for (int k = 0; k < X_PER; ++k)
        if ((xin >> k) & 1u) norm_relu8<T>(xr[k], nmu, nrs);
    }
#pragma unroll
    for (int k = 0; k < X_PER; ++k) {
      const int e = tid + k * 512;
      if (e < X_ITEMS) xr[k].store(Xl + (e >> 2) * XP + (e & 3) * 8);
    }
  };

  const int g4 = lane >> 4, i16 = lane & 15, q = i16 >> 2, p4 = i16 & 3;
  auto compute = [&](int buf) {
    const T* Dl = lds + buf * (DS + XS);
    const T* Xl = Dl + DS;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int kk = 0; kk < 128; kk += 32) {
        bf16x8 af[MT];
        const int v_lo = V == 3 ? kk + 16 * (g4 >> 1) + 4 * (g4 & 1) + q : kk + 8 * g4 + q;
        const int v_hi = V == 3 ? v_lo + 8 : v_lo + 4;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const bf16_t* base = (const bf16_t*)Dl + v_lo * DP + i * 16 + 4 * p4;
          af[i] = tr_frag(base, base + (v_hi - v_lo) * DP);
        }
        const int hlo = ((v_lo >> 5) * HLO_Y + ((v_lo >> 3) & 3)) * HLO_X + (v_lo & 7);
        const int hhi = ((v_hi >> 5) * HLO_Y + ((v_hi >> 3) & 3)) * HLO_X + (v_hi & 7);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (t < t_cnt) {
            const int tap = t_begin + t;
            const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
            const int hoff = (kz * HLO_Y + ky) * HLO_X + kx;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const bf16_t* pl = (const bf16_t*)Xl + (hlo + hoff) * XP + j * 16 + 4 * p4;
              const bf16_t* ph = (const bf16_t*)Xl + (hhi + hoff) * XP + j * 16 + 4 * p4;
              const bf16x8 bfr = tr_frag(pl, ph);
#pragma unroll
              for (int i = 0; i < MT; ++i)
                acc[t][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr, acc[t][i][j], 0, 0, 0);
            }
          }
        }
      }
    } else {
      for (int kk = 0; kk < 128; kk += 4) {
        const int v = kk + g4;
        const int hv = ((v >> 5) * HLO_Y + ((v >> 3) & 3)) * HLO_X + (v & 7);
        float af[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) af[i] = (float)Dl[v * DP + i * 16 + i16];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (t < t_cnt) {
            const int tap = t_begin + t;
            const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
            const int hoff = (kz * HLO_Y + ky) * HLO_X + kx;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const float bv = (float)Xl[(hv + hoff) * XP + j * 16 + i16];
#pragma unroll
              for (int i = 0; i < MT; ++i)
                acc[t][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bv, acc[t][i][j], 0, 0, 0);
            }
          }
        }
      }
    }
  };

  // PIPE: steps s = (dy plane k4, tap t) over this wave's TC taps; lane rows v_lo = 32 k4 + v0 and v_lo + 8 (halo
  // rows hlo and hlo + HLO_X of the tap's shifted window)
  const int v0 = 16 * (g4 >> 1) + 4 * (g4 & 1) + q;
  const int hlo0 = ((v0 >> 3) & 3) * HLO_X + (v0 & 7);
  auto compute_pipe = [&](int buf, auto tcc) __attribute__((always_inline)) {
    if constexpr (PIPE) {
      constexpr int TC = decltype(tcc)::value;
      constexpr int PD = 3, NS = 4 * TC;
      const bf16_t* Dl = reinterpret_cast<const bf16_t*>(lds + buf * (DS + XS));
      const bf16_t* Xl = Dl + DS;
      bf16x8 af[2][MT], bf[PD][2];
      auto load_a = [&](int k4, bf16x8(&a)[MT]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const bf16_t* base = Dl + (32 * k4 + v0) * DP + i * 16 + 4 * p4;
          a[i] = tr_frag(base, base + 8 * DP);
        }
      };
      auto load_b = [&](int k4, int t, bf16x8(&b)[2]) __attribute__((always_inline)) {
        const int tap = t_begin + t;
        const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
        const int h = k4 * (HLO_Y * HLO_X) + hlo0 + (kz * HLO_Y + ky) * HLO_X + kx;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const bf16_t* pl = Xl + h * XP + j * 16 + 4 * p4;
          b[j] = tr_frag(pl, pl + HLO_X * XP);
        }
      };
      load_a(0, af[0]);
#pragma unroll
      for (int s0 = 0; s0 < PD - 1; ++s0)
        if (s0 < NS) load_b(s0 / TC, s0 % TC, bf[s0 % PD]);
#pragma unroll
      for (int sidx = 0; sidx < NS; ++sidx) {
        const int k4 = sidx / TC, t = sidx % TC;
        const int sn = sidx + PD - 1;
        if (sn < NS) load_b(sn / TC, sn % TC, bf[sn % PD]);
        if (t == 0 && k4 + 1 < 4) load_a(k4 + 1, af[(k4 + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < MT; ++i)
            acc[t][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[k4 & 1][i], bf[sidx % PD][j], acc[t][i][j], 0,
                                                                   0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };

  // PIPE: the brick loop is instantiated per tap count (a branch inside it would merge the two multiplies'
  // accumulator registers at every brick: copies, and 256 VGPRs with spills)
  auto brick_loop = [&](auto tcc) __attribute__((always_inline)) {
    int buf = 0;
    if (b_begin < b_end) {
      load_into(b_begin, dr, xr, xin, xn);
      store_from(0, dr, xr, xin, xn);
    }
    __syncthreads();
    for (long long b = b_begin; b < b_end; ++b) {
      const bool more = b + 1 < b_end;
      if (more) load_into(b + 1, dr, xr, xin, xn);
      if constexpr (PIPE)
        compute_pipe(buf, tcc);
      else
        compute(buf);
      if (more) store_from(buf ^ 1, dr, xr, xin, xn);
      __syncthreads();
      buf ^= 1;
    }
  };
  if (!PIPE || t_cnt == 4)
    brick_loop(std::integral_constant<int, 4>{});
  else
    brick_loop(std::integral_constant<int, 3>{});

  static_assert(sizeof(lds) >= 16 * WEP_P * sizeof(float) && sizeof(lds) >= 512 * 8 * sizeof(float),
                "epilogue staging must fit the stage buffers");
  wgrad_store_chmajor<MT>(acc, t_begin, t_cnt, reinterpret_cast<float*>(lds), g, ks, row0, c0);
  if (do_bias) wgrad_store_bias<CG>(bsum, reinterpret_cast<float*>(lds), g, ks, row0);
}

// ------------------------------------------ brick wgrad, LDS-DMA staging (3^3, bf16)
// wgrad_brick2_kernel<bf16, MT, 3> with the stage images filled by buffer_load ... lds (no staging registers,
// no ds_write) into THREE stage buffers: brick b + 2 is in flight while brick b is multiplied, so a load has two
// brick periods to land instead of one (the register-staged kernel spends about a third of its time waiting
// on its one-brick-ahead loads: 136 us with, 105 us without loads at 96^3 32->32).  The rows are unpadded and
// XOR-swizzled at 32-byte granules instead (the DMA writes 64 contiguous 16-B chunks per wave-instruction; the
// lane picks the global chunk that belongs at its LDS position), which keeps the transposed fragment reads
// conflict-free:
//   halo row (hz, hy, hx), 64 B:   granule j of channel half j lives at j ^ ((hx >> 2) & 1)
//   dy row v, 64 B (32 co):        granule i at i ^ ((v >> 2) & 1)
//   dy row v, 128 B (64 co):       granule i at i ^ ((v >> 1) & 3)
// (8 consecutive halo x positions, or 8 aligned dy rows, then cover the 64 banks once).  The bias gradient
// is one more MFMA chain against a ones fragment in wave 7's free tap slot.  NORM: the deferred InstanceNorm +
// ReLU is applied in place to the landed halo (each thread its fixed channel group), one extra barrier.
// (WD_OOB, wd_rsrc, wd_dma16: mmseg_common.h)

// PIPE: the fragment reads of the next (dy plane, tap) step are issued before the current step's MFMAs
// MTC < MT: only the first MTC 16-row tiles are multiplied (the rest are output-channel padding, WgradArgs::pad16);
// staging and the epilogue keep the MT-row layout, the skipped rows' accumulators stay zero
template <int MT, bool NORM = false, int NST = 3, bool PIPE = false, int MTC = MT>
__global__ __launch_bounds__(512, 1) void wgrad_dma_kernel(WgradArgs g) {
  typedef bf16_t T;
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  constexpr int CO = MT * 16;
  constexpr int DCH = CO / 8, XCH = CK / 8;             // 16-B chunks per dy / halo row
  constexpr int NDI = 128 * DCH / 64;                   // dy wave-instructions per brick (8 / 16)
  constexpr int NXI = (HLO_V * XCH + 63) / 64;          // halo wave-instructions (23, the last one half)
  constexpr int NI = NDI + NXI, KI = (NI + 7) / 8;      // per brick; per wave (8 waves)
  constexpr int DS = 128 * CO, XS = NXI * 64 * 8;       // elements per stage (halo padded to whole instructions)
  constexpr int SS = DS + XS;
  __shared__ __attribute__((aligned(16))) T st[NST * SS];   // ring of NST stage images

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cin = 8 << g.cpg_shift;
  const int nchunk = wgrad_nchunk(g.cpg_shift, g.kchunks), rt_n = g.Ca / CO;
  const int tile = g.swz ? xcd_swizzle(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int ct = tile % nchunk, rt = (tile / nchunk) % rt_n, ks = tile / (nchunk * rt_n);
  const int bz_n = g.D / BRK_Z, by_n = g.H / BRK_Y, bx_n = g.W / BRK_X;
  const int nbrick = (int)(g.V / ((long long)g.D * g.H * g.W)) * bz_n * by_n * bx_n;
  const int bpk = (nbrick + g.ksplit - 1) / g.ksplit;
  const int b_begin = ks * bpk;
  const int b_end = b_begin + bpk < nbrick ? b_begin + bpk : nbrick;
  const int HW = g.H * g.W;
  const int row0 = rt * CO, c0 = ct * CK;
  const bool do_bias = g.bias_part != nullptr && ct == 0;
  const int t_begin = wave < 3 ? 4 * wave : 12 + 3 * (wave - 3);
  const int t_cnt = wave < 3 ? 4 : 3;
  const bool bias_wave = do_bias && wave == 7;

  const wd_rsrc_t drsrc = wd_rsrc(g.a, (uint32_t)(g.V * g.lda * 2));
  const wd_rsrc_t xrsrc = wd_rsrc(g.b, (uint32_t)(g.V * g.ldb * 2));

  // per DMA slot k (wave-instruction m = wave + 8 k): the lane's byte offset from the brick origin and, for a
  // halo chunk, its halo position (hz, hy, hx packed; 0xff: no chunk)
  uint32_t rel[KI], hpos[KI];
  int nw = 0;
#pragma unroll
  for (int k = 0; k < KI; ++k) {
    const int m = wave + 8 * k;
    rel[k] = 0;
    hpos[k] = 0xffu;
    if (m < NDI) {
      const int p = m * 64 + lane, v = p / DCH, c = p % DCH;
      const int gi = (c >> 1) ^ (DCH == 4 ? (v >> 2) & 1 : (v >> 1) & 3), cc = (gi << 1) | (c & 1);
      rel[k] = (uint32_t)((((v >> 5) * HW + ((v >> 3) & 3) * g.W + (v & 7)) * g.lda + row0 + cc * 8) * 2);
      ++nw;
    } else if (m < NI) {
      const int p = (m - NDI) * 64 + lane, h = p >> 2, c = p & 3;
      if (h < HLO_V) {
        const int hx = h % HLO_X, hy = (h / HLO_X) % HLO_Y, hz = h / (HLO_X * HLO_Y);
        const int cc = (((c >> 1) ^ ((hx >> 2) & 1)) << 1) | (c & 1);
        rel[k] = (uint32_t)(((hz * HW + hy * g.W + hx) * g.ldb + c0 + cc * 8) * 2);
        hpos[k] = (uint32_t)(hz | (hy << 8) | (hx << 16));
      }
      ++nw;
    }
  }
  // brick b's origin: x fastest
  auto brick_at = [&](int b, int& n, int& z0, int& y0, int& x0) __attribute__((always_inline)) {
    int q = b;
    const int bx = q % bx_n;
    q /= bx_n;
    const int by = q % by_n;
    q /= by_n;
    const int bz = q % bz_n;
    n = q / bz_n;
    z0 = bz * BRK_Z, y0 = by * BRK_Y, x0 = bx * BRK_X;
  };
  auto issue = [&](T* dst, int b) __attribute__((always_inline)) {
    int n, z0, y0, x0;
    brick_at(b, n, z0, y0, x0);
    const int vb = (n * g.D + z0) * HW + y0 * g.W + x0;
    const int dbase = vb * g.lda * 2;
    const int xbase = (vb - HW - g.W - 1) * g.ldb * 2;
#pragma unroll
    for (int k = 0; k < KI; ++k) {
      const int m = wave + 8 * k;
      if (m < NDI) {
        wd_dma16(__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(lds_ptr_t)(dst + m * 512)),
                 (uint32_t)(dbase + (int)rel[k]), drsrc);
      } else if (m < NI) {
        const uint32_t hp = hpos[k];
        const int z = z0 - 1 + (int)(hp & 0xff), y = y0 - 1 + (int)((hp >> 8) & 0xff), x = x0 - 1 + (int)(hp >> 16);
        const bool ok = hp != 0xffu && (unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H &&
                        (unsigned)x < (unsigned)g.W;
        wd_dma16(__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(lds_ptr_t)(dst + DS + (m - NDI) * 512)),
                 ok ? (uint32_t)(xbase + (int)rel[k]) : WD_OOB, xrsrc);
      }
    }
  };
  // this wave's DMAs of all but the last brick issued have landed (vmcnt <= nw)
  // wait until at most `later` bricks' DMAs of this wave are in flight (vmcnt <= later * nw)
  auto wait_bricks = [&](int later) __attribute__((always_inline)) {
    switch (later * nw) {
#define MMSEG_WD_WAIT(N) \
  case N: __builtin_amdgcn_s_waitcnt(0x0f70 | N); break;
      MMSEG_WD_WAIT(1) MMSEG_WD_WAIT(2) MMSEG_WD_WAIT(3) MMSEG_WD_WAIT(4) MMSEG_WD_WAIT(5) MMSEG_WD_WAIT(6)
      MMSEG_WD_WAIT(7) MMSEG_WD_WAIT(8) MMSEG_WD_WAIT(9) MMSEG_WD_WAIT(10) MMSEG_WD_WAIT(11) MMSEG_WD_WAIT(12)
      MMSEG_WD_WAIT(13) MMSEG_WD_WAIT(14) MMSEG_WD_WAIT(15)
#undef MMSEG_WD_WAIT
      default: __builtin_amdgcn_s_waitcnt(0x0f70); break;
    }
  };
  // NORM: thread owns channel group cg = tid & 3 of halo rows (tid >> 2) + 128 k
  int norm_n = -1;
  float nmu[NORM ? 8 : 1], nrs[NORM ? 8 : 1];
  auto normalize = [&](T* dst, int b) __attribute__((always_inline)) {
    if constexpr (NORM) {
      int q = b;
      const int bx = q % bx_n;
      q /= bx_n;
      const int by = q % by_n;
      q /= by_n;
      const int bz = q % bz_n;
      const int n = q / bz_n;
      if (n != norm_n) {
        norm_n = n;
        const int cb = n * cin + c0 + (tid & 3) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          nmu[j] = g.nmean[cb + j];
          nrs[j] = g.nrstd[cb + j];
        }
      }
      const int z0 = bz * BRK_Z, y0 = by * BRK_Y, x0 = bx * BRK_X, cg = tid & 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int h = (tid >> 2) + 128 * k;
        if (h < HLO_V) {
          const int hx = h % HLO_X, hy = (h / HLO_X) % HLO_Y, hz = h / (HLO_X * HLO_Y);
          if ((unsigned)(z0 - 1 + hz) < (unsigned)g.D && (unsigned)(y0 - 1 + hy) < (unsigned)g.H &&
              (unsigned)(x0 - 1 + hx) < (unsigned)g.W) {
            const int c = (((cg >> 1) ^ ((hx >> 2) & 1)) << 1) | (cg & 1);
            T* p = dst + DS + h * CK + c * 8;
            V8<T> v;
            v.load(p);
            norm_relu8<T>(v, nmu, nrs);
            v.store(p);
          }
        }
      }
    }
  };

  f32x4 acc[4][MT][2];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[t][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // fragment addressing (bytes): dy rows v_lo = kk + 16 (g4 >> 1) + 4 (g4 & 1) + q and v_lo + 8 share the
  // swizzle; halo rows hlo + tap offset share hx's
  const int g4 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p4 = i16 & 3;
  const int v0 = 16 * (g4 >> 1) + 4 * (g4 & 1) + q4;
  const int dsw = DCH == 4 ? (v0 >> 2) & 1 : (v0 >> 1) & 3;
  const int hx0 = 4 * (g4 & 1) + q4;   // x of v_lo; y = 2 (g4 >> 1)
  const int hlo0 = (2 * (g4 >> 1)) * HLO_X + hx0;
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
  // halo row of tap (kz, ky, kx) for the lane's voxels in brick z-plane vz
  auto xrow = [&](const char* Xb, int sb, int vz, int kz, int ky, int kx) __attribute__((always_inline)) {
    (void)sb;
    return Xb + (hlo0 + (vz + kz) * (HLO_Y * HLO_X) + ky * HLO_X + kx) * (CK * 2);
  };
  auto compute = [&](const T* S, int sb) __attribute__((always_inline)) {
    const char* Db = reinterpret_cast<const char*>(S);
    const char* Xb = reinterpret_cast<const char*>(S + DS);
#pragma unroll
    for (int kk = 0; kk < 128; kk += 32) {
      bf16x8 af[MT];
#pragma unroll
      for (int i = 0; i < MTC; ++i) {
        const bf16_t* base = reinterpret_cast<const bf16_t*>(Db + (kk + v0) * (CO * 2) + 32 * (i ^ dsw) + 8 * p4);
        af[i] = tr_frag(base, base + 8 * CO);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < t_cnt) {
          const int tap = t_begin + t;
          const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
          const char* row = xrow(Xb, sb, kk >> 5, kz, ky, kx);
          const int xs = ((hx0 + kx) >> 2) & 1;
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const bf16_t* pl = reinterpret_cast<const bf16_t*>(row + 32 * (j ^ xs) + 8 * p4);
            const bf16x8 bfr = tr_frag(pl, pl + HLO_X * CK);
#pragma unroll
            for (int i = 0; i < MTC; ++i)
              acc[t][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr, acc[t][i][j], 0, 0, 0);
          }
        } else if (t == 3 && bias_wave) {
#pragma unroll
          for (int i = 0; i < MTC; ++i)
            acc[3][i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], ones, acc[3][i][0], 0, 0, 0);
        }
      }
    }
  };
  // software-pipelined: steps s = (kk, t) over this wave's TC taps, fragments double-buffered
  auto compute_pipe = [&](const T* S, int sb, auto tcc) __attribute__((always_inline)) {
    constexpr int TC = decltype(tcc)::value;
    const char* Db = reinterpret_cast<const char*>(S);
    const char* Xb = reinterpret_cast<const char*>(S + DS);
    constexpr int PD = 3;
    bf16x8 af[2][MT], bf[PD][2];
    auto load_a = [&](int kk, bf16x8(&a)[MT]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < MTC; ++i) {
        const bf16_t* base = reinterpret_cast<const bf16_t*>(Db + (kk + v0) * (CO * 2) + 32 * (i ^ dsw) + 8 * p4);
        a[i] = tr_frag(base, base + 8 * CO);
      }
    };
    auto load_b = [&](int kk, int t, bf16x8(&b)[2]) __attribute__((always_inline)) {
      const int tap = t_begin + t;
      const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
      const char* row = xrow(Xb, sb, kk >> 5, kz, ky, kx);
      const int xs = ((hx0 + kx) >> 2) & 1;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bf16_t* pl = reinterpret_cast<const bf16_t*>(row + 32 * (j ^ xs) + 8 * p4);
        b[j] = tr_frag(pl, pl + HLO_X * CK);
      }
    };
    // B fragments PD - 1 steps ahead (ring of PD), A one dy plane ahead
    constexpr int NS = 4 * TC;
    load_a(0, af[0]);
#pragma unroll
    for (int s0 = 0; s0 < PD - 1; ++s0)
      if (s0 < NS) load_b(32 * (s0 / TC), s0 % TC, bf[s0 % PD]);
#pragma unroll
    for (int sidx = 0; sidx < NS; ++sidx) {
      const int k4 = sidx / TC, t = sidx % TC;
      const int sn = sidx + PD - 1;
      if (sn < NS) load_b(32 * (sn / TC), sn % TC, bf[sn % PD]);
      if (t == 0 && k4 + 1 < 4) load_a(32 * (k4 + 1), af[(k4 + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < MTC; ++i)
          acc[t][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[k4 & 1][i], bf[sidx % PD][j], acc[t][i][j], 0, 0,
                                                                 0);
      if (TC == 3 && t == 2 && bias_wave) {
#pragma unroll
        for (int i = 0; i < MTC; ++i)
          acc[3][i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[k4 & 1][i], ones, acc[3][i][0], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // prologue: bricks b_begin .. b_begin + NST - 2 in flight, the first one landed
  for (int k = 0; k < NST - 1; ++k) {
    if (b_begin + k < b_end) issue(st + k * SS, b_begin + k);
  }
  {
    const int inflight = b_end - b_begin - 1 < NST - 2 ? b_end - b_begin - 1 : NST - 2;
    wait_bricks(inflight > 0 ? inflight : 0);
  }
  __syncthreads();
  if constexpr (NORM) {
    if (b_begin < b_end) {
      normalize(st, b_begin);
      __syncthreads();
    }
  }
  // PIPE: the brick loop is instantiated per tap count (a branch on t_cnt inside it merges the two multiplies'
  // accumulator registers at every brick: copies around every MFMA group)
  auto brick_loop = [&](auto tcc) __attribute__((always_inline)) {
  for (int b = b_begin, sc = 0; b < b_end; ++b, sc = sc + 1 == NST ? 0 : sc + 1) {
    // issue brick b + NST - 1 into the stage brick b - 1 used (every wave passed the barrier after it)
    const int sn = sc == 0 ? NST - 1 : sc - 1;
    if (b + NST - 1 < b_end) issue(st + sn * SS, b + NST - 1);
    const int sb = 0;
    if constexpr (PIPE)
      compute_pipe(st + sc * SS, sb, tcc);
    else
      compute(st + sc * SS, sb);
    // brick b + 1 has landed once at most min(NST - 2, bricks issued after it) bricks are in flight
    {
      const int after = b_end - b - 2 < NST - 2 ? b_end - b - 2 : NST - 2;
      wait_bricks(after > 0 ? after : 0);
    }
    __syncthreads();
    if constexpr (NORM) {
      if (b + 1 < b_end) {
        normalize(st + (sc + 1 == NST ? 0 : sc + 1) * SS, b + 1);
        __syncthreads();
      }
    }
  }
  };
  if (!PIPE || t_cnt == 4)
    brick_loop(std::integral_constant<int, 4>{});
  else
    brick_loop(std::integral_constant<int, 3>{});

  static_assert(sizeof(st) >= 16 * WEP_P * sizeof(float),
                "epilogue staging must fit the stage ring");
  if (g.frag && !(g.grad != nullptr && g.ksplit == 1)) {
    // split partials in the accumulators' own layout: every (tap, i, j) fragment is 1 KB contiguous (lane l's
    // f32x4 at 16 l), so each wave stores straight from registers with 16-B lanes -- no LDS transpose, no
    // barriers; wgrad_reduce_kernel (frag_mt) maps the layout to the torch order and sums in the same fixed
    // split order as before (bitwise the same gradient)
    float* base = g.part + (long long)ks * g.Ca * g.Ncols + (long long)(rt * nchunk + ct) * (CO * 27 * CK);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t >= t_cnt) continue;
      const int tap = t_begin + t;
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          *reinterpret_cast<f32x4*>(base + ((tap * MT + i) * 2 + j) * 256 + lane * 4) = acc[t][i][j];
    }
  } else {
    __syncthreads();
    wgrad_store_chmajor<MT>(acc, t_begin, t_cnt, reinterpret_cast<float*>(st),
                            g, ks, row0, c0);
  }
  if (bias_wave && i16 == 0) {
    // acc[3][i][0][r] = sum over the block's voxels of dy[.][row0 + 16 i + 4 g4 + r] (every column alike)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = row0 + 16 * i + 4 * g4 + r;
        const float s = acc[3][i][0][r];
        if (g.bias_grad != nullptr && g.ksplit == 1)
          g.bias_grad[co] = g.accumulate ? g.bias_grad[co] + s : s;
        else
          g.bias_part[(long long)ks * g.Ca + co] = s;
      }
  }
}

// ------------------------------------------- row-slab weight gradient (3^3, bf16, 32 co, W % 32 == 0)
// The 96^3 32-output-channel layers' weight gradient as long-lived blocks that walk columns of x rows.
// GEMM view: dW[co][ci][tap] = sum_v dy[v][co] x[v + tap][ci].  One MFMA K-slab is 32 CONSECUTIVE x voxels of one
// (z, y) row.  The B fragment of tap (kz, ky, kx) for the dy row at (z, y) is then the halo row at (z + kz - 1,
// y + ky - 1) shifted by kx: the same fragment serves every (dy row, kz, ky) pair that lands on the same halo row.
// A wave owns one kx, one 16-channel ci half and one 16-channel co half (12 waves) and ALL nine (kz, ky) of it, so
// each halo-row fragment it reads from LDS feeds up to nine MFMAs and each dy fragment (kept in registers while
// its plane is in the 3-plane tap window) up to nine: ~0.28 LDS fragments per MFMA against 0.65 for the brick
// kernels (wgrad_brick2 / wgrad_dma: each halo fragment feeds 2 MFMAs, DESIGN (d) 8a).
// A block owns a contiguous range of dy-plane steps: columns (sample n, RY = 6 y rows (4 where H % 6 != 0), 32 x)
// walked along z, so a halo plane is staged ONCE per column (8 rows x 34 voxels for 6 x 32 dy voxels: 1.4x the x
// bytes, against 2.8x for a 4 x 4 x 8 brick's halo).  Step u of a column segment stages halo plane z_a - 1 + u and dy plane z_a + u
// into one slot of a 4-slot LDS ring by LDS-DMA (buffer_load ... lds; the same 32-B XOR swizzle as wgrad_dma,
// conflict-free for every kx shift) three steps ahead; the multiply pairs the halo plane with the dy planes
// u, u - 1, u - 2 (kz = 0, 1, 2), whose fragments rotate through three register sets.  One barrier per step.
// NORM (deferred InstanceNorm + ReLU of x): each wave normalises, in place, the halo chunks its OWN DMA
// instructions brought in (its own vmcnt orders them), one step before they are multiplied: no extra barrier.
// Bias gradient: dy fragments times a ones fragment, dealt round-robin over the six waves of a co half.
// Partials: the fragment-native layout of wgrad_dma (WReduceArgs::frag_mt = 2), summed by the same reduce.
constexpr int WROW_HX = 34;                                  // voxels per halo row
constexpr int WROW_WAVES = 12;                               // (kx, ci half, co half)
constexpr int WROW_MAXN = 16;                                // samples whose norm statistics fit the LDS table
// per plane step of RY dy rows: halo rows, halo / dy DMA wave-instructions, slot geometry (bytes)
template <int RY>
struct WRowGeo {
  static constexpr int HY = RY + 2;
  static constexpr int HI = (HY * WROW_HX * 4 + 63) / 64;   // halo chunks (16 B) / 64 lanes (RY 4: 13)
  static constexpr int DI = RY * 32 * 4 / 64;                // dy (RY 4: 8)
  static constexpr int NI = HI + DI;
  static constexpr int KI = (NI + WROW_WAVES - 1) / WROW_WAVES;   // DMA instructions per wave per step (at most)
  static constexpr int DOFF = HI * 1024;                     // dy image offset in a slot
  static constexpr int SLOT = NI * 1024;
};

// a column segment of a block's step range: column col (sample, 4 y rows, 32 x), dy planes [za, za + L)
struct WRowSeg {
  int s, col, za, L;
};

// RY dy rows per step (4 or 6; 8 spills at 168 VGPRs), NST ring slots (DMA NST - 1 steps ahead)
template <bool NORM, int RY = 6, int NST = 4>
__global__ __launch_bounds__(768, 1) void wgrad_row_kernel(WgradArgs g) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef WRowGeo<RY> G;
  constexpr int WROW_RY = RY, WROW_HY = G::HY, WROW_HI = G::HI, WROW_NI = G::NI, WROW_DOFF = G::DOFF;
  constexpr int WROW_SLOT = G::SLOT, WROW_NST = NST, KI = G::KI;
  __shared__ __attribute__((aligned(16))) char ring[WROW_NST * WROW_SLOT];
  __shared__ __attribute__((aligned(16))) float ntab[NORM ? 2 * WROW_MAXN * CK : 4];
  __shared__ float bred[WROW_WAVES * 16];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kx = wave >> 2, jh = (wave >> 1) & 1, ih = wave & 1;   // the wave's tap column, ci half, co half
  const int cin = 8 << g.cpg_shift;
  const int nchunk = wgrad_nchunk(g.cpg_shift, g.kchunks);
  const int tile = g.swz ? xcd_swizzle(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int ct = tile % nchunk, ks = tile / nchunk;
  const int c0 = ct * CK;
  const int D = g.D, H = g.H, W = g.W;
  const int ncx = W / 32, ncol = (H / WROW_RY) * ncx;
  const int N = (int)(g.V / ((long long)D * H * W));
  const int s_tot = N * ncol * D;
  const int spb = (s_tot + g.ksplit - 1) / g.ksplit;
  const int s_begin = min(ks * spb, s_tot), s_end = min(s_begin + spb, s_tot);
  const bool do_bias = g.bias_part != nullptr && ct == 0;
  const wd_rsrc_t drsrc = wd_rsrc(g.a, (uint32_t)(g.V * g.lda * 2));
  const wd_rsrc_t xrsrc = wd_rsrc(g.b, (uint32_t)(g.V * g.ldb * 2));

  // segments and halo steps: a segment of L dy planes takes L + 2 halo steps
  auto seg_at = [&](int s) __attribute__((always_inline)) {
    WRowSeg q;
    q.s = s;
    q.col = s / D;
    q.za = s - q.col * D;
    q.L = min(D, s_end - q.col * D) - q.za;
    return q;
  };
  int h_tot = 0;
  for (int s = s_begin; s < s_end;) {
    const WRowSeg q = seg_at(s);
    h_tot += q.L + 2;
    s += q.L;
  }

  // the wave's DMA instructions (m = wave, wave + 12 < WROW_NI): m < WROW_HI halo chunks, else dy chunks.  Per
  // instruction: the lane's byte offset from the plane origin and its (y, x) position in the plane
  int nw = 0;
  int rel[KI], py[KI], px[KI], ncc[KI];
#pragma unroll
  for (int k = 0; k < KI; ++k) {
    const int m = wave + 12 * k;
    rel[k] = 0, py[k] = 0xff, px[k] = 0, ncc[k] = 0;
    if (m < WROW_HI) {
      const int p = m * 64 + lane, hy = p / (WROW_HX * 4), r = p - hy * (WROW_HX * 4), xh = r >> 2, cs = r & 3;
      const int cc = (((cs >> 1) ^ ((xh >> 2) & 1)) << 1) | (cs & 1);
      if (hy < WROW_HY) {
        rel[k] = ((hy * W + xh) * g.ldb + c0 + cc * 8) * 2;
        py[k] = hy, px[k] = xh, ncc[k] = cc;
      }
    } else if (m < WROW_NI) {
      const int p = (m - WROW_HI) * 64 + lane, ry = p >> 7, r = p & 127, x = r >> 2, cs = r & 3;
      const int cc = (((cs >> 1) ^ ((x >> 2) & 1)) << 1) | (cs & 1);
      rel[k] = ((ry * W + x) * g.lda + cc * 8) * 2;
    }
    if (m < WROW_NI) ++nw;
  }
  // DMA of halo step (segment q, step u) into ring slot `slot`
  auto issue = [&](int slot, const WRowSeg& q, int u) __attribute__((always_inline)) {
    const int n = q.col / ncol, cr = q.col - n * ncol, by = cr / ncx;
    const int y0 = by * WROW_RY, x0 = (cr - by * ncx) * 32;
    const int zh = q.za - 1 + u, zd = q.za + u;
    const bool zh_ok = (unsigned)zh < (unsigned)D, zd_ok = u < q.L;
    const int hb = (((n * D + zh) * H + (y0 - 1)) * W + (x0 - 1)) * g.ldb * 2;
    const int db = (((n * D + zd) * H + y0) * W + x0) * g.lda * 2;
    const uint32_t lbase = (uint32_t)(uintptr_t)(lds_ptr_t)(ring + slot * WROW_SLOT);
#pragma unroll
    for (int k = 0; k < KI; ++k) {
      const int m = wave + 12 * k;
      if (m < WROW_HI) {
        const int y = y0 - 1 + py[k], x = x0 - 1 + px[k];
        const bool ok = zh_ok && py[k] != 0xff && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        wd_dma16(__builtin_amdgcn_readfirstlane(lbase + m * 1024), ok ? (uint32_t)(hb + rel[k]) : WD_OOB, xrsrc);
      } else if (m < WROW_NI) {
        wd_dma16(__builtin_amdgcn_readfirstlane(lbase + m * 1024), zd_ok ? (uint32_t)(db + rel[k]) : WD_OOB, drsrc);
      }
    }
  };
  auto wait_cnt = [&](int cnt) __attribute__((always_inline)) {
    switch (cnt) {
#define MMSEG_WR_WAIT(N) \
  case N: __builtin_amdgcn_s_waitcnt(0x0f70 | N); break;
      MMSEG_WR_WAIT(1) MMSEG_WR_WAIT(2) MMSEG_WR_WAIT(3) MMSEG_WR_WAIT(4) MMSEG_WR_WAIT(5) MMSEG_WR_WAIT(6)
      MMSEG_WR_WAIT(7) MMSEG_WR_WAIT(8) MMSEG_WR_WAIT(9) MMSEG_WR_WAIT(10) MMSEG_WR_WAIT(11) MMSEG_WR_WAIT(12)
      MMSEG_WR_WAIT(13) MMSEG_WR_WAIT(14) MMSEG_WR_WAIT(15)
#undef MMSEG_WR_WAIT
      default: __builtin_amdgcn_s_waitcnt(0x0f70); break;
    }
  };
  // NORM: relu((x - mean) * rstd) of the in-volume halo chunks this wave's own DMA brought into `slot`
  auto normalize = [&](int slot, const WRowSeg& q, int u) __attribute__((always_inline)) {
    if constexpr (NORM) {
      const int n = q.col / ncol, cr = q.col - n * ncol, by = cr / ncx;
      const int y0 = by * WROW_RY, x0 = (cr - by * ncx) * 32;
      const int zh = q.za - 1 + u;
      if ((unsigned)zh >= (unsigned)D) return;
#pragma unroll
      for (int k = 0; k < KI; ++k) {
        const int m = wave + 12 * k;
        if (m < WROW_HI) {
          const int y = y0 - 1 + py[k], x = x0 - 1 + px[k];
          if (py[k] != 0xff && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
            bf16_t* p = reinterpret_cast<bf16_t*>(ring + slot * WROW_SLOT + m * 1024 + lane * 16);
            const float4* mu4 = reinterpret_cast<const float4*>(ntab + n * CK + ncc[k] * 8);
            const float4* rs4 = reinterpret_cast<const float4*>(ntab + WROW_MAXN * CK + n * CK + ncc[k] * 8);
            const float4 ma = mu4[0], mb = mu4[1], ra = rs4[0], rb = rs4[1];
            const float mu[8] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
            const float rs[8] = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w};
            V8<bf16_t> v;
            v.load(p);
            norm_relu8<bf16_t>(v, mu, rs);
            v.store(p);
          }
        }
      }
    }
  };

  // fragments: lane rows x = v0 and v0 + 8 of a 32-voxel row (wgrad_dma's lane order), granule swizzle (x >> 2) & 1
  const int g4 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p4 = i16 & 3;
  const int v0 = 16 * (g4 >> 1) + 4 * (g4 & 1) + q4;
  const int aoff = WROW_DOFF + v0 * 64 + 32 * (ih ^ (g4 & 1)) + 8 * p4;                      // + ry * 2048
  const int boff = (v0 + kx) * 64 + 32 * (jh ^ (((v0 + kx) >> 2) & 1)) + 8 * p4;            // + hy * 2176
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
  f32x4 acc[3][3], accb = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  bf16x8 areg[3][WROW_RY];   // dy fragments of the three dy planes in the tap window (register set = plane % 3)
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int r = 0; r < WROW_RY; ++r) areg[a][r] = ones;

  if (s_begin < s_end) {
    if constexpr (NORM) {
      for (int e = tid; e < N * CK; e += 768) {
        const int n = e / CK, c = e - n * CK;
        ntab[n * CK + c] = g.nmean[n * cin + c0 + c];
        ntab[WROW_MAXN * CK + n * CK + c] = g.nrstd[n * cin + c0 + c];
      }
      __syncthreads();
    }
    // prologue: halo steps 0 .. NST - 2 issued; the DMA cursor (dq, du) points at the next step to issue
    WRowSeg dq = seg_at(s_begin);
    int du = 0;
    auto dma_next = [&]() __attribute__((always_inline)) {
      if (++du == dq.L + 2) {
        du = 0;
        if (dq.s + dq.L < s_end) dq = seg_at(dq.s + dq.L);
      }
    };
    int h_iss = 0;
    for (; h_iss < WROW_NST - 1 && h_iss < h_tot; ++h_iss) {
      issue(h_iss % WROW_NST, dq, du);
      dma_next();
    }
    wait_cnt(nw * (min(h_tot - 1, WROW_NST - 2)));
    normalize(0, seg_at(s_begin), 0);
    __syncthreads();

    int h = 0;
    // one halo step: issue step h + NST - 1, multiply step h, normalise step h + 1, barrier
    auto step = [&](auto phc, const WRowSeg& q, int u) __attribute__((always_inline)) {
      constexpr int PH = decltype(phc)::value;
      if (h_iss < h_tot) {
        issue(h_iss % WROW_NST, dq, du);
        dma_next();
        ++h_iss;
      }
      const char* S = ring + (h % WROW_NST) * WROW_SLOT;
      bf16x8 bfr[WROW_HY];
#pragma unroll
      for (int hy = 0; hy < WROW_HY; ++hy) {
        const bf16_t* pl = reinterpret_cast<const bf16_t*>(S + hy * (WROW_HX * 64) + boff);
        bfr[hy] = tr_frag(pl, pl + 8 * 32);
      }
      const bool anew = u < q.L;
      if (anew) {
#pragma unroll
        for (int r = 0; r < WROW_RY; ++r) {
          const bf16_t* pa = reinterpret_cast<const bf16_t*>(S + r * (32 * 64) + aoff);
          areg[PH][r] = tr_frag(pa, pa + 8 * 32);
        }
      }
      auto mm = [&](auto kzc, const bf16x8(&a)[WROW_RY]) __attribute__((always_inline)) {
        constexpr int KZ = decltype(kzc)::value;
#pragma unroll
        for (int hy = 0; hy < WROW_HY; ++hy)
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) {
            const int ry = hy - ky;
            if (ry >= 0 && ry < WROW_RY)
              acc[KZ][ky] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ry], bfr[hy], acc[KZ][ky], 0, 0, 0);
          }
      };
      // kz = 2: dy plane u - 2 (register set (PH + 1) % 3), kz = 1: plane u - 1 ((PH + 2) % 3), kz = 0: plane u
      if (u >= 2) mm(std::integral_constant<int, 2>{}, areg[(PH + 1) % 3]);
      if (u >= 1 && u <= q.L) mm(std::integral_constant<int, 1>{}, areg[(PH + 2) % 3]);
      if (anew) {
        mm(std::integral_constant<int, 0>{}, areg[PH]);
        if (do_bias && h % 6 == kx * 2 + jh) {
#pragma unroll
          for (int r = 0; r < WROW_RY; ++r) accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(areg[PH][r], ones, accb, 0, 0, 0);
        }
      }
      // step h + 1 landed (this wave's part), normalised, then visible to all after the barrier
      wait_cnt(nw * (min(h_tot - 1, h + WROW_NST - 1) - (h + 1)));
      if (h + 1 < h_tot) {
        if (u + 1 < q.L + 2)
          normalize((h + 1) % WROW_NST, q, u + 1);
        else if (q.s + q.L < s_end)
          normalize((h + 1) % WROW_NST, seg_at(q.s + q.L), 0);
      }
      __syncthreads();
      ++h;
    };
    for (int s = s_begin; s < s_end;) {
      const WRowSeg q = seg_at(s);
      for (int u0 = 0; u0 < q.L + 2; u0 += 3) {
        step(std::integral_constant<int, 0>{}, q, u0);
        if (u0 + 1 < q.L + 2) step(std::integral_constant<int, 1>{}, q, u0 + 1);
        if (u0 + 2 < q.L + 2) step(std::integral_constant<int, 2>{}, q, u0 + 2);
      }
      s += q.L;
    }
  }

  // split partials in wgrad_dma's fragment-native layout: (tap, co tile, ci tile) fragments of 1 KB
  float* base = g.part + (long long)ks * g.Ca * g.Ncols + (long long)ct * (32 * 27 * CK);
#pragma unroll
  for (int kz = 0; kz < 3; ++kz)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int tap = kz * 9 + ky * 3 + kx;
      *reinterpret_cast<f32x4*>(base + ((tap * 2 + ih) * 2 + jh) * 256 + lane * 4) = acc[kz][ky];
    }
  if (do_bias) {
    // accb[r] on lanes i16 == 0: sum over this wave's share of the voxels of dy[.][16 ih + 4 g4 + r]
    if (i16 == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) bred[wave * 16 + 4 * g4 + r] = accb[r];
    }
    __syncthreads();
    if (tid < 32) {
      const int i = tid >> 4;
      float sacc = 0.f;
      for (int w = i; w < WROW_WAVES; w += 2) sacc += bred[w * 16 + (tid & 15)];
      g.bias_part[(long long)ks * g.Ca + tid] = sacc;
    }
  }
}

// ------------------------------------- runtime-brick wgrad (small volumes)
// wgrad_brick2_kernel for volumes whose sides are not multiples of (4, 4, 8)
// (the 12^3 and 6^3 levels): brick (bz, by, bx) chosen on the host, <= 128
// voxels (K of one brick, zero-padded to 128) and a halo of <= 384 voxels.
// The voxel -> halo-row map of a lane does not depend on the brick, so it is
// computed once (4 k-steps x 2 rows).
constexpr int WR_MAXHV = 384;

// CB* > 0: compile-time brick (3x6x6 at the 12^3 / 6^3 levels), see conv3_brickr_kernel.
template <typename T, int MT, int CBZ = 0, int CBY = 0, int CBX = 0>
__global__ __launch_bounds__(512) void wgrad_brickr_kernel(WgradArgs g, int bz_rt, int by_rt, int bx_rt) {
  const int bz = CBZ > 0 ? CBZ : bz_rt, by = CBY > 0 ? CBY : by_rt, bx = CBX > 0 ? CBX : bx_rt;
  constexpr int EP = 16 / sizeof(T);
  constexpr int CO = MT * 16, CG = CO / 8;
  constexpr int DP = CO + EP;
  constexpr int XP = CK + EP;
  constexpr int DS = 128 * DP, XS = WR_MAXHV * XP;
  __shared__ __attribute__((aligned(16))) T lds[2 * (DS + XS)];
  constexpr int D_ITEMS = 128 * CG, X_MAX = WR_MAXHV * 4;
  constexpr int D_PER = (D_ITEMS + 511) / 512, X_PER = (X_MAX + 511) / 512;

  const T* Dy = reinterpret_cast<const T*>(g.a);
  const T* X = reinterpret_cast<const T*>(g.b);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cin = 8 << g.cpg_shift;
  const int nchunk = wgrad_nchunk(g.cpg_shift, g.kchunks), rt_n = g.Ca / CO;
  const int tile = g.swz ? xcd_swizzle(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int ct = tile % nchunk, rt = (tile / nchunk) % rt_n, ks = tile / (nchunk * rt_n);
  const int HX = bx + 2, HY = by + 2, HZ = bz + 2;
  const int HV = HZ * HY * HX, rows = bz * by * bx;
  const int bz_n = g.D / bz, by_n = g.H / by, bx_n = g.W / bx;
  const long long nbrick = (g.V / ((long long)g.D * g.H * g.W)) * bz_n * by_n * bx_n;
  // grouped: group gi's bricks (contiguous, sample-major) over its own ksplit / groups splits
  const int ngrp = g.groups > 1 ? g.groups : 1;
  const int ks_g = g.ksplit / ngrp, gi = ks / ks_g, kl = ks - gi * ks_g;
  const long long nb_g = nbrick / ngrp;
  const long long bpk = (nb_g + ks_g - 1) / ks_g;
  const long long b_begin = gi * nb_g + kl * bpk;
  const long long b_end = b_begin + bpk < (gi + 1) * nb_g ? b_begin + bpk : (gi + 1) * nb_g;
  const long long HW = (long long)g.H * g.W;
  const int row0 = rt * CO, c0 = ct * CK;
  const bool do_bias = g.bias_part != nullptr && ct == 0;
  const int t_begin = wave < 3 ? 4 * wave : 12 + 3 * (wave - 3);
  const int t_cnt = wave < 3 ? 4 : 3;

  f32x4 acc[4][MT][2];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[t][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bsum[8] = {0, 0, 0, 0, 0, 0, 0, 0};

  auto vox_halo = [&](int v) {   // brick voxel -> halo row (tap 0); padding voxels map to row 0 (dy is 0 there)
    if (v >= rows) return 0;
    const int rx = v % bx, q = v / bx;
    return ((q / by) * HY + q % by) * HX + rx;
  };

  V8<T> dr[D_PER], xr[X_PER];
  auto load = [&](long long b) {
    int q = (int)b;   // brick index < V < 2^31 (mmseg_wgrad): 32-bit division
    const int bxi = q % bx_n;
    q /= bx_n;
    const int byi = q % by_n;
    q /= by_n;
    const int bzi = q % bz_n;
    const long long nbase = (long long)(q / bz_n) * g.D * HW;
    const int z0 = bzi * bz, y0 = byi * by, x0 = bxi * bx;
#pragma unroll
    for (int k = 0; k < D_PER; ++k) {
      const int e = tid + k * 512, v = e / CG, cg = e % CG;
      if (e < D_ITEMS) {
        if (v < rows) {
          const int rx = v % bx, qq = v / bx;
          const int ry = qq % by, rz = qq / by;
          dr[k].load(Dy + (nbase + (z0 + rz) * HW + (long long)(y0 + ry) * g.W + x0 + rx) * g.lda + row0 + cg * 8);
        } else {
          dr[k].zero();
        }
      }
    }
#pragma unroll
    for (int k = 0; k < X_PER; ++k) {
      const int e = tid + k * 512;
      if (e < HV * 4) {
        const int h = e >> 2, cg = e & 3;
        const int hx = h % HX, qq = h / HX;
        const int hy = qq % HY, hz = qq / HY;
        const int z = z0 - 1 + hz, y = y0 - 1 + hy, x = x0 - 1 + hx;
        if ((unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H && (unsigned)x < (unsigned)g.W)
          xr[k].load(X + (nbase + z * HW + (long long)y * g.W + x) * g.ldb + c0 + cg * 8);
        else
          xr[k].zero();
      }
    }
  };
  auto store = [&](int buf) {
    T* Dl = lds + buf * (DS + XS);
    T* Xl = Dl + DS;
#pragma unroll
    for (int k = 0; k < D_PER; ++k) {
      const int e = tid + k * 512;
      if (e < D_ITEMS) {
        dr[k].store(Dl + (e / CG) * DP + (e % CG) * 8);
        if (do_bias) {
#pragma unroll
          for (int j = 0; j < 8; ++j) bsum[j] += dr[k].get(j);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < X_PER; ++k) {
      const int e = tid + k * 512;
      if (e < HV * 4) xr[k].store(Xl + (e >> 2) * XP + (e & 3) * 8);
    }
  };

  const int g4 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p4 = i16 & 3;
  int hlo[4], hhi[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    hlo[s] = vox_halo(s * 32 + 8 * g4 + q4);
    hhi[s] = vox_halo(s * 32 + 8 * g4 + q4 + 4);
  }
  int toff[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int tap = t_begin + (t < t_cnt ? t : 0);
    toff[t] = ((tap / 9) * HY + (tap / 3) % 3) * HX + tap % 3;
  }
  int buf = 0;
  if (b_begin < b_end) {
    load(b_begin);
    store(0);
  }
  __syncthreads();
  for (long long b = b_begin; b < b_end; ++b) {
    const bool more = b + 1 < b_end;
    if (more) load(b + 1);
    const T* Dl = lds + buf * (DS + XS);
    const T* Xl = Dl + DS;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (s * 32 >= rows) break;
        bf16x8 af[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const bf16_t* base = (const bf16_t*)Dl + (s * 32 + 8 * g4 + q4) * DP + i * 16 + 4 * p4;
          af[i] = tr_frag(base, base + 4 * DP);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (t < t_cnt) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const bf16_t* pl = (const bf16_t*)Xl + (hlo[s] + toff[t]) * XP + j * 16 + 4 * p4;
              const bf16_t* ph = (const bf16_t*)Xl + (hhi[s] + toff[t]) * XP + j * 16 + 4 * p4;
              const bf16x8 bfr = tr_frag(pl, ph);
#pragma unroll
              for (int i = 0; i < MT; ++i)
                acc[t][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr, acc[t][i][j], 0, 0, 0);
            }
          }
        }
      }
    } else {
      for (int kk = 0; kk < rows; kk += 4) {
        const int v = kk + g4;
        const int hv = vox_halo(v);
        float af[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) af[i] = (float)Dl[v * DP + i * 16 + i16];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (t < t_cnt) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const float bv = (float)Xl[(hv + toff[t]) * XP + j * 16 + i16];
#pragma unroll
              for (int i = 0; i < MT; ++i)
                acc[t][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bv, acc[t][i][j], 0, 0, 0);
            }
          }
        }
      }
    }
    if (more) store(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  static_assert(sizeof(lds) >= 16 * WEP_P * sizeof(float) && sizeof(lds) >= 512 * 8 * sizeof(float),
                "epilogue staging must fit the stage buffers");
  wgrad_store_chmajor<MT>(acc, t_begin, t_cnt, reinterpret_cast<float*>(lds), g, ks, row0, c0);
  if (do_bias) wgrad_store_bias<CG>(bsum, reinterpret_cast<float*>(lds), g, ks, row0);
}

struct WBrick { int bz, by, bx; };

// Runtime brick for the small-volume wgrad: divisors of (D, H, W), <= 128 voxels,
// halo <= WR_MAXHV; the most voxels wins.  {0,0,0} = none.
WBrick plan_wgrad_brickr(int D, int H, int W) {
  WBrick best{0, 0, 0};
  int brows = 0;
  for (int bz = 1; bz <= D && bz <= 16; ++bz) {
    if (D % bz) continue;
    for (int by = 1; by <= H && by <= 16; ++by) {
      if (H % by) continue;
      for (int bx = 1; bx <= W && bx <= 16; ++bx) {
        if (W % bx) continue;
        const int rows = bz * by * bx;
        const int halo = (bz + 2) * (by + 2) * (bx + 2);
        if (rows > 128 || halo > WR_MAXHV) continue;
        // ties go to the smaller halo (12^3: 3x6x6, the compile-time kernel, over 3x3x12)
        const bool tie_better = rows == brows && halo < (best.bz + 2) * (best.by + 2) * (best.bx + 2);
        if (rows > brows || tie_better) {
          brows = rows;
          best = {bz, by, bx};
        }
      }
    }
  }
  return brows >= 32 ? best : WBrick{0, 0, 0};
}

// Column sums (bias gradient): db[c] = sum_v dy[v][c], split over voxels.
template <typename T>
__global__ void colsum_partial_kernel(const T* __restrict__ dy, int ld, int C, long long V, long long vps,
                                      float* __restrict__ part) {
  // block: 256 threads = (256/C8) voxel lanes x C8 channel groups (C8 = C/8 <= 64)
  const int C8 = C >> 3;
  const int lanes_v = 256 / C8;
  const int tid = threadIdx.x;
  const int cg = tid % C8, vl = tid / C8;
  const long long v0 = (long long)blockIdx.x * vps;
  long long v1 = v0 + vps;
  if (v1 > V) v1 = V;
  float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (vl < lanes_v) {
    for (long long v = v0 + vl; v < v1; v += lanes_v) {
      V8<T> x;
      x.load(dy + v * ld + cg * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += x.get(j);
    }
  }
  __shared__ float red[256 * 8];
#pragma unroll
  for (int j = 0; j < 8; ++j) red[tid * 8 + j] = s[j];
  __syncthreads();
  if (tid < C8) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int l = 0; l < lanes_v; ++l)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += red[(l * C8 + tid) * 8 + j];
#pragma unroll
    for (int j = 0; j < 8; ++j) part[(long long)blockIdx.x * C + tid * 8 + j] = acc[j];
  }
}

// one 256-thread block per channel: threads stride over the block partials (4 loads in flight), a fixed
// shuffle tree per wave, then the 4 waves in order (one wave per channel walked ~30 dependent loads per lane
// for the transposed conv's 8 x ksplit column-sum partials)
__global__ __launch_bounds__(256) void colsum_reduce_kernel(const float* __restrict__ part, int nblk, int C,
                                                            float* __restrict__ out, int accumulate) {
  const int c = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float v = 0.f;
#pragma unroll 4
  for (int b = threadIdx.x; b < nblk; b += 256) v += part[(long long)b * C + c];
  v = wave_sum(v);
  __shared__ float wred[4];
  if (lane == 0) wred[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = ((wred[0] + wred[1]) + wred[2]) + wred[3];
    out[c] = accumulate ? out[c] + t : t;
  }
}

// 64-co row tiles for the brick weight-gradient kernels (brick2 / LDS-DMA and runtime brick), else 32-co.
// A block's split partial is its whole tile, so at small volumes -- where the ~256 resident blocks each see a
// few bricks -- the partials outweigh the inputs (24^3: 54 MB written and re-read per launch against 35-65 MB
// of input); 32-co tiles halve them at the price of reading the halo once per row tile.  Below V voxels
// a threshold the 32-co tiles were tried below (r04: equal or slower at 24^3), so 64-co tiles throughout.
bool wgrad_co64(int Ca) { return Ca % 64 == 0; }

// 0: generic wgrad_kernel, 1: wgrad_brick_kernel (32 co), 2: wgrad_brick2_kernel (64 / 32 co),
// 3: wgrad_brickr_kernel (runtime brick, small volumes).
// (v2 / runtime brick are bf16 only: their two fp32 stage buffers would not fit in LDS)
int wgrad_brick_ok(int Ca, int cpg_shift, int D, int H, int W, int lda, int ldb, int dtype, bool force_r = false) {
  const int k = knob("MMSEG_WGRAD_BRICK", 2);
  if (!(k && Ca % 32 == 0 && (8 << cpg_shift) % CK == 0 && lda % 8 == 0 && ldb % 8 == 0)) return 0;
  if (force_r)   // grouped launches: only the runtime-brick weight gradient splits by sample group
    return (k >= 2 && dtype == MMSEG_BF16 && plan_wgrad_brickr(D, H, W).bz) ? 3 : 0;
  if (D % BRK_Z == 0 && H % BRK_Y == 0 && W % BRK_X == 0)
    return (k >= 2 && dtype == MMSEG_BF16) ? 2 : 1;
  if (k >= 2 && dtype == MMSEG_BF16 && plan_wgrad_brickr(D, H, W).bz) return 3;
  return 0;
}

// Split count of the CONV3 brick wgrad: enough blocks to fill the chip, capped by
// the caller's workspace (cap) and by one brick per split.
int brick_wgrad_splits(long long V, int cap, int Ca, int cpg_shift, int kind, int D, int H, int W,
                       int kchunks = 0) {
  const int nchunk = wgrad_nchunk(cpg_shift, kchunks);
  const int tiles = nchunk * (Ca / ((kind >= 2 && wgrad_co64(Ca)) ? 64 : 32));
  // v2 / runtime-brick kernels: one wave of resident blocks (256 CUs x blocks per CU: 2 for the 32-co brick2
  // kernel, 1 for the 64-co and runtime-brick kernels, whose stage buffers take > 80 KB of LDS), never more:
  // a partial second wave of 512-thread blocks costs a whole block time.
  long long ks;
  if (kind >= 2) {
    // (256 slots for the runtime-brick kernel too: 128 / 384 / 512 measured +0.04..0.15 ms per step, r04ah)
    ks = 256LL / tiles;
  } else {
    ks = (1024 + tiles - 1) / tiles;
  }
  if (ks > cap) ks = cap;
  long long nbrick = V / 128;
  if (kind == 3) {
    const WBrick wb = plan_wgrad_brickr(D, H, W);
    nbrick = V / (wb.bz * wb.by * wb.bx);
    // at least 4 bricks per split: at 6^3 (4 bricks) one split writes the gradient directly; two splits moved 2x
    // the 28 MB fp32 gradient of a 512->512 layer through partials and a reduce (41 -> 24 us, r02 convbench)
    const long long minb = 4;
    if (ks > nbrick / minb) ks = nbrick / minb;
  }
  if (ks > nbrick) ks = nbrick;
  if (ks < 1) ks = 1;
  const long long bpk = (nbrick + ks - 1) / ks;
  return (int)((nbrick + bpk - 1) / bpk);
}


int mmseg_wgrad_splits_impl(long long V, int ksplit) {
  long long vps = ((V + ksplit - 1) / ksplit + 63) / 64 * 64;
  return (int)((V + vps - 1) / vps);
}

// Real 32-channel chunks of a channel-padded x (Ci < Cip), 0 = all (the brick wgrad kernels skip the rest; the
// split reduction never reads the skipped columns' partials into the gradient).
int wgrad_kchunks(int Cip, int Ci) { return Ci < Cip ? (Ci + 31) / 32 : 0; }

// A single-split brick weight gradient writes the torch-layout gradient [co][ci][27] itself when its input
// channels are unpadded, or padded past whole real 32-channel chunks (Ci % 32 == 0: SwinUNETR's 768 of 1024): the
// kernel computes only the real chunks (wgrad_kchunks), whose rows then land at pitch 27 Ci (WgradArgs::grad_ld)
// -- no partial, no relayout reduce.
bool wgrad_direct_ok(int Cip, int Ci) {
  return Ci == Cip || (Ci % 32 == 0 && wgrad_kchunks(Cip, Ci) == Ci / 32);
}

// ---- the kernel choice of a 3^3 weight gradient (mmseg_conv3_wgrad and its forms).  choose_conv3_wgrad is the only
// place that decides it: conv3_wgrad_impl launches what it returns, and the planning queries (_ws_floats, _norm_ok,
// _group_ok, mmseg_conv3_wgrad_kernel) answer from it without a GPU.
enum WgradKernel { WK_GATHER, WK_BRICK1, WK_BRICK2, WK_DMA, WK_ROW, WK_BRICKR };
struct Conv3WgradChoice {
  int kind;          // wgrad_brick_ok
  int ksplit;
  int direct;        // the kernel writes the torch-layout gradient itself (brick2 / brickr, one split -- per group --,
                     // wgrad_direct_ok): no partials, no reduce
  long long ws;      // floats of split partials + bias partials otherwise
  int kernel;        // WgradKernel
  const char* name;  // the family noted for mmseg_last_kernel() / the per-kernel timer
  int co;            // output-channel rows of a block's tile
  int fmt;           // split partials: 0 row-major tiles, else fragment-native in fmt 16-row tiles
                     // (WgradArgs::frag, WReduceArgs::frag_mt)
  WBrick wb;         // WK_BRICKR: the brick
};

// ws_cap: the caller's workspace (floats), which caps the split.  groups > 1 (mmseg_conv3_wgrad_group): the
// runtime-brick kernel even where the (4, 8, 8)-brick family fits, the split count of the whole V rounded down to a
// multiple of `groups` (at least one split per group).  norm: x is staged through a deferred InstanceNorm + ReLU.
Conv3WgradChoice choose_conv3_wgrad(long long V, int Co, int Cip, int Ci, int cpg_shift, int D, int H, int W, int lda,
                                    int ldb, int dtype, long long ws_cap, int groups = 1, bool norm = false,
                                    bool pad16 = false) {
  Conv3WgradChoice p{};
  const long long ncols = 27LL * Cip;
  const long long per_split = (long long)Co * ncols + Co;
  int cap = (int)(ws_cap / per_split);
  if (cap < 1) cap = 1;
  p.kind = wgrad_brick_ok(Co, cpg_shift, D, H, W, lda, ldb, dtype, groups > 1);
  if (p.kind) {
    p.ksplit = brick_wgrad_splits(V, cap, Co, cpg_shift, p.kind, D, H, W, wgrad_kchunks(Cip, Ci));
  } else {
    const int bn = 64;
    const long long tiles = ((ncols + bn - 1) / bn) * ((Co + (Co % 64 == 0 ? 63 : 31)) / (Co % 64 == 0 ? 64 : 32));
    long long want = (1024 + tiles - 1) / tiles;
    if (want > V / 512) want = V / 512;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    p.ksplit = mmseg_wgrad_splits_impl(V, (int)want);
  }
  if (groups > 1) {
    p.ksplit = std::max(p.ksplit / groups * groups, groups);
    // one split per group (the deepest levels): each writes its group's gradient directly, as the ungrouped
    // single-split launch does -- a reduce would only copy 2 x 28 MB there (28.8 us, r04d)
    p.direct = p.kind >= 2 && p.ksplit == groups && Ci == Cip;
  } else {
    p.direct = p.kind >= 2 && p.ksplit == 1 && wgrad_direct_ok(Cip, Ci);
  }
  p.ws = p.direct ? 0 : p.ksplit * per_split;

  // both tensors within 31 bits of byte offset at 16-B rows (the LDS-DMA kernels; kinds 2 / 3 are bf16)
  const bool dma_ok = V * lda * 2 < (1LL << 31) && V * ldb * 2 < (1LL << 31) && lda % 8 == 0 && ldb % 8 == 0;
  p.co = wgrad_co64(Co) ? 64 : 32;
  if (p.kind == 3) {
    p.kernel = WK_BRICKR;
    p.wb = plan_wgrad_brickr(D, H, W);
    // (the compile-time bricks under their rocprofv3 family names, tools/rocprof_families.py)
    const bool b366 = p.wb.bz == 3 && p.wb.by == 6 && p.wb.bx == 6;
    const bool b448 = p.wb.bz == 4 && p.wb.by == 4 && p.wb.bx == 8;   // grouped 48^3 / 24^3
    p.name = p.co == 64 ? (b366 ? "wgrad_brickr_kernel<CO64,V3>" : b448 ? "wgrad_brickr_kernel<CO64,B448>"
                                                                         : "wgrad_brickr_kernel<CO64>")
                        : (b366 ? "wgrad_brickr_kernel<CO32,V3>" : b448 ? "wgrad_brickr_kernel<CO32,B448>"
                                                                         : "wgrad_brickr_kernel<CO32>");
  } else if (p.kind == 2 && knob("MMSEG_WGRAD_ROW", 1) && Co == 32 && W % 32 == 0 && H % 4 == 0 && (8 << cpg_shift) % CK == 0 &&
             groups <= 1 && !pad16 && p.ksplit > 1 && dma_ok && V / ((long long)D * H * W) <= WROW_MAXN) {
    // the row-slab weight gradient: 32 output channels, W % 32 == 0, H % 4 == 0, split partials (no direct gradient,
    // no groups, no padded rows), fragment-native partials only (2 co tiles of 16)
    p.kernel = WK_ROW;
    p.name = norm ? "wgrad_row_kernel<CO32,NORM>" : "wgrad_row_kernel<CO32>";
    p.fmt = 2;
  } else if (p.kind == 2 && knob("MMSEG_WGRAD_DMA", 1) && !norm && dma_ok) {
    // the LDS-DMA kernel (the deferred-norm variant keeps register staging by default: its in-place LDS pass and
    // extra barrier cost more than the DMA saves, 0.651 -> 0.682 ms/step for the 32-co family)
    p.kernel = WK_DMA;
    p.name = p.co == 64 ? "wgrad_dma_kernel<CO64>" : "wgrad_dma_kernel<CO32>";
    p.fmt = p.co / 16;
  } else if (p.kind == 2) {
    p.kernel = WK_BRICK2;
    p.name = p.co == 64 ? "wgrad_brick2_kernel<CO64,V3>" : "wgrad_brick2_kernel<CO32,V3>";
  } else if (p.kind == 1) {
    p.kernel = WK_BRICK1;
    p.name = "wgrad_brick_kernel";
    p.co = 32;
  } else {
    p.kernel = WK_GATHER;
    p.name = "wgrad_kernel<conv3>";
  }
  return p;
}

// Launch a weight gradient: what choose_conv3_wgrad chose (CONV3), or the gather kernel (WK_GATHER: the 1x1 and
// transposed-conv layers, and 3^3 shapes no brick kernel takes).
template <typename T, int MODE>
int launch_wgrad(const WgradArgs& g, const Conv3WgradChoice& c, hipStream_t s) {
  mmseg::note_kernel(c.name);
  const WBrick wb = c.wb;
  if (c.kernel != WK_GATHER) {
    const dim3 grid(wgrad_nchunk(g.cpg_shift, g.kchunks) * (g.Ca / c.co) * g.ksplit);   // (chunk, row tile, split)
    const bool b366 = wb.bz == 3 && wb.by == 6 && wb.bx == 6, b448 = wb.bz == 4 && wb.by == 4 && wb.bx == 8;
    if constexpr (sizeof(T) == 2) {   // (v2 / runtime brick are bf16 only: their fp32 stage buffers would not fit in LDS)
      if (c.kernel == WK_BRICKR && c.co == 64) {
        if (b366)
          MMSEG_LAUNCH((wgrad_brickr_kernel<T, 4, 3, 6, 6>), grid, dim3(512), 0, s, g, 3, 6, 6);
        else if (b448)
          MMSEG_LAUNCH((wgrad_brickr_kernel<T, 4, 4, 4, 8>), grid, dim3(512), 0, s, g, 4, 4, 8);
        else
          MMSEG_LAUNCH((wgrad_brickr_kernel<T, 4>), grid, dim3(512), 0, s, g, wb.bz, wb.by, wb.bx);
      } else if (c.kernel == WK_BRICKR) {
        if (b366)
          MMSEG_LAUNCH((wgrad_brickr_kernel<T, 2, 3, 6, 6>), grid, dim3(512), 0, s, g, 3, 6, 6);
        else if (b448)
          MMSEG_LAUNCH((wgrad_brickr_kernel<T, 2, 4, 4, 8>), grid, dim3(512), 0, s, g, 4, 4, 8);
        else
          MMSEG_LAUNCH((wgrad_brickr_kernel<T, 2>), grid, dim3(512), 0, s, g, wb.bz, wb.by, wb.bx);
      } else if (c.kernel == WK_ROW) {
        // rows per step: 6 where H allows (r06c, 96^3 B=2: 32 -> 32 deferred norm 128.6 -> 113.6 us, 64 -> 32
        // 196 -> 179 us against 4 rows; five ring slots or s_setprio for waves 6..11 measured no change), else 4
        auto run = [&](auto normc) {
          constexpr bool NRM = decltype(normc)::value;
          if (g.H % 6 == 0)
            MMSEG_LAUNCH((wgrad_row_kernel<NRM, 6>), grid, dim3(768), 0, s, g);
          else
            MMSEG_LAUNCH((wgrad_row_kernel<NRM, 4>), grid, dim3(768), 0, s, g);
        };
        if (g.nmean) run(std::true_type{});
        else run(std::false_type{});
      } else if (c.kernel == WK_DMA) {
        // 48 real rows of 64 (SwinUNETR's 48-channel levels): three row tiles, room for the pipelined multiply
        if (c.co == 64 && g.pad16 && g.Ca == 64)
          MMSEG_LAUNCH((wgrad_dma_kernel<4, false, 3, true, 3>), grid, dim3(512), 0, s, g);
        else if (c.co == 64)   // (fragment prefetch two steps ahead spills at 64 co: 59.5 -> 72.3 us)
          MMSEG_LAUNCH((wgrad_dma_kernel<4>), grid, dim3(512), 0, s, g);
        else
          MMSEG_LAUNCH((wgrad_dma_kernel<2, false, 3, true>), grid, dim3(512), 0, s, g);
      } else if (c.kernel == WK_BRICK2 && c.co == 64) {
        if (g.nmean)
          MMSEG_LAUNCH((wgrad_brick2_kernel<T, 4, 3, true>), grid, dim3(512), 0, s, g);
        else
          MMSEG_LAUNCH((wgrad_brick2_kernel<T, 4, 3>), grid, dim3(512), 0, s, g);
      } else if (c.kernel == WK_BRICK2) {
        // (fragment reads software-pipelined, r05: the deferred-norm 96^3 layers 136 -> 125 us before wgrad_row)
        if (g.nmean)
          MMSEG_LAUNCH((wgrad_brick2_kernel<T, 2, 3, true, true>), grid, dim3(512), 0, s, g);
        else
          MMSEG_LAUNCH((wgrad_brick2_kernel<T, 2, 3, false, true>), grid, dim3(512), 0, s, g);
      }
    }
    if (c.kernel == WK_BRICK1) MMSEG_LAUNCH((wgrad_brick_kernel<T>), grid, dim3(256), 0, s, g);
    return mmseg::check_launch(c.name);
  }
  // 1x1 weight gradients take 64-row tiles whatever the row count (rows past Ca are masked): every row tile re-reads
  // the whole B operand (x), and these launches are HBM-bound -- 48 / 144-row layers read x once / three times
  // instead of twice / five times with 32-row tiles
  const dim3 block(256);
  if (g.Ca % 64 == 0 || MODE == MODE_POINT) {
    dim3 grid(ceil_div(g.Ncols, 64) * ceil_div(g.Ca, 64) * g.ksplit);
    MMSEG_LAUNCH((wgrad_kernel<T, MODE, 2, 2, 2, 2, 64>), grid, block, 0, s, g);
  } else {
    dim3 grid(ceil_div(g.Ncols, 64) * ceil_div(g.Ca, 32) * g.ksplit);
    MMSEG_LAUNCH((wgrad_kernel<T, MODE, 1, 4, 2, 1, 64>), grid, block, 0, s, g);
  }
  return mmseg::check_launch(c.name);
}

template <typename T>
int launch_wgrad_mode(const WgradArgs& g, const Conv3WgradChoice& c, int mode, hipStream_t s) {
  switch (mode) {
    case MODE_CONV3: return launch_wgrad<T, MODE_CONV3>(g, c, s);
    case MODE_POINT: return launch_wgrad<T, MODE_POINT>(g, c, s);
    case MODE_CONVT_DGRAD: return launch_wgrad<T, MODE_CONVT_DGRAD>(g, c, s);
  }
  mmseg::set_error("wgrad: bad mode %d", mode);
  return 1;
}

}  // namespace

// =================================================================== C ABI
extern "C" {

// Weight-gradient partials of the 1x1 and transposed-conv layers: part[ksplit][Ca][Ncols] (fp32).
int mmseg_wgrad(const void* a, int lda, const void* b, int ldb, float* part, float* bias_part, int mode, int Ca,
                int Ncols, int cpg_shift, long long V, int D, int H, int W, int ksplit, int dtype, void* stream) {
  MMSEG_REQUIRE(Ca % 8 == 0, "wgrad: rows (%d) must be a multiple of 8", Ca);
  MMSEG_REQUIRE(Ncols % 8 == 0, "wgrad: cols (%d) must be a multiple of 8", Ncols);
  MMSEG_REQUIRE(V < (1LL << 31), "wgrad: voxel count %lld must fit 31 bits", V);
  MMSEG_REQUIRE(mode == MODE_POINT || mode == MODE_CONVT_DGRAD,
                "wgrad: mode %d: this entry takes the 1x1 (1) and transposed-conv (3) layers; the 3^3 weight gradient "
                "is mmseg_conv3_wgrad", mode);
  MMSEG_REQUIRE(ksplit >= 1, "wgrad: ksplit >= 1");
  const long long vps = ((V + ksplit - 1) / ksplit + 63) / 64 * 64;
  ksplit = (int)((V + vps - 1) / vps);
  WgradArgs g{a, lda, b, ldb, part, bias_part, Ca, Ncols, cpg_shift, V, D, H, W, ksplit, vps,
              1, 0, nullptr, nullptr, 0};
  Conv3WgradChoice c{};
  c.kernel = WK_GATHER;
  c.name = mode == MODE_POINT ? "wgrad_kernel<point>" : "wgrad_kernel<convT_dgrad>";
  hipStream_t s = (hipStream_t)stream;
  return dtype == MMSEG_BF16 ? launch_wgrad_mode<bf16_t>(g, c, mode, s) : launch_wgrad_mode<float>(g, c, mode, s);
}

// Effective split count the wgrad launcher will use (callers size `part` with it).
int mmseg_wgrad_splits(long long V, int ksplit) { return mmseg_wgrad_splits_impl(V, ksplit); }

// Weight (+ bias) gradient of a 3^3 conv straight into the torch-layout fp32 gradient
// grad[Co][Ci][27] (+ bias_grad[Co]), = or += (accumulate).  The library picks kernel and split;
// ws holds mmseg_conv3_wgrad_ws_floats() floats (more lets it split further, fewer is clamped).
long long mmseg_conv3_wgrad_ws_floats(long long V, int Co, int Cip, int Ci, int cpg_shift, int D, int H, int W,
                                      int lddy, int ldx, int dtype) {
  const long long cap = 16LL << 20;
  return choose_conv3_wgrad(V, Co, Cip, Ci, cpg_shift, D, H, W, lddy, ldx, dtype, cap).ws;
}

long long mmseg_conv3_wgrad_group_ws_floats(long long V, int Co, int Cip, int Ci, int cpg_shift, int D, int H, int W,
                                            int lddy, int ldx, int groups, int dtype) {
  const long long cap = 16LL << 20;
  return choose_conv3_wgrad(V, Co, Cip, Ci, cpg_shift, D, H, W, lddy, ldx, dtype, cap, groups).ws;
}

// The family name (mmseg_last_kernel()) the weight gradient of a 3^3 conv of this shape would launch with a
// workspace of ws_floats; flags: 1 deferred norm, 8 grouped, 16 last 16 rows padding (phase bit 8).
const char* mmseg_conv3_wgrad_kernel(long long V, int Co, int Cip, int Ci, int cpg_shift, int D, int H, int W,
                                     int lddy, int ldx, long long ws_floats, int flags, int dtype) {
  return choose_conv3_wgrad(V, Co, Cip, Ci, cpg_shift, D, H, W, lddy, ldx, dtype, ws_floats,
                            (flags & CF_GROUPS) ? 2 : 1, flags & CF_NORM, flags & CF_PAD16).name;
}

int conv3_wgrad_impl(const void* dy, int lddy, const void* x, int ldx, const float* nmean, const float* nrstd,
                     float* grad, float* bias_grad, int Co, int Cip, int Ci, int cpg_shift, long long V, int D, int H,
                     int W, float* ws, long long ws_floats, int accumulate, int dtype, void* stream, int phase = 3,
                     int groups = 1, long long grad_gstride = 0, int bias_gstride = 0);

// 1 when mmseg_conv3_wgrad_group takes this shape: the runtime-brick weight-gradient kernel (kind 3), as
// mmseg_conv3_group_ok (conv_gemm.hip) for the forward and the data gradient
int mmseg_conv3_wgrad_group_ok(long long V, int Co, int Cip, int Ci, int cpg_shift, int D, int H, int W, int lddy,
                               int ldx, int dtype) {
  if (!knob("MMSEG_GROUP_SMALL", 1)) return 0;
  if (choose_conv3_wgrad(V, Co, Cip, Ci, cpg_shift, D, H, W, lddy, ldx, dtype, 1LL << 40).kind == 3) return 1;
  return knob("MMSEG_GROUP_FORCE_R", 1) &&
         choose_conv3_wgrad(V, Co, Cip, Ci, cpg_shift, D, H, W, lddy, ldx, dtype, 1LL << 40, 2).kind == 3;
}

// The weight / bias gradients of `groups` same-shape 3^3 convs over equal sample groups of one activation pair
// (group gi: samples [gi N / groups, (gi + 1) N / groups) of dy / x, gradient at grad + gi * grad_gstride and
// bias_grad + gi * bias_gstride floats) in one weight-gradient launch and one reduce -- the modality encoders'
// small levels.  Runtime-brick weight-gradient shapes only; ws: mmseg_conv3_wgrad_group_ws_floats().
int mmseg_conv3_wgrad_group(const void* dy, int lddy, const void* x, int ldx, float* grad, float* bias_grad, int Co,
                            int Cip, int Ci, int cpg_shift, long long V, int D, int H, int W, float* ws,
                            long long ws_floats, int accumulate, int groups, long long grad_gstride,
                            int bias_gstride, int phase, int dtype, void* stream) {
  MMSEG_REQUIRE(groups >= 1 && V % ((long long)groups * D * H * W) == 0 && phase >= 1 && phase <= 7 && (phase & 3),
                "conv3_wgrad_group: V must hold groups x whole samples, phase bits 1 | 2 (| 4 defer)");
  return conv3_wgrad_impl(dy, lddy, x, ldx, nullptr, nullptr, grad, bias_grad, Co, Cip, Ci, cpg_shift, V, D, H, W, ws,
                          ws_floats, accumulate, dtype, stream, phase, groups, grad_gstride, bias_gstride);
}

int mmseg_conv3_wgrad(const void* dy, int lddy, const void* x, int ldx, float* grad, float* bias_grad, int Co, int Cip,
                      int Ci, int cpg_shift, long long V, int D, int H, int W, float* ws, long long ws_floats,
                      int accumulate, int dtype, void* stream) {
  return conv3_wgrad_impl(dy, lddy, x, ldx, nullptr, nullptr, grad, bias_grad, Co, Cip, Ci, cpg_shift, V, D, H, W, ws,
                          ws_floats, accumulate, dtype, stream);
}

// 1 when mmseg_conv3_wgrad_norm can run this shape: the brick2 weight-gradient kernel (the only one that applies
// a deferred InstanceNorm + ReLU to x), no channel padding, bf16.
int mmseg_conv3_wgrad_norm_ok(long long V, int Co, int Cip, int Ci, int cpg_shift, int D, int H, int W, int lddy,
                              int ldx, int dtype) {
  if (dtype != MMSEG_BF16 || Ci != Cip || !knob("MMSEG_DEFER_CONV_NORM", 1)) return 0;
  return choose_conv3_wgrad(V, Co, Cip, Ci, cpg_shift, D, H, W, lddy, ldx, dtype, 1LL << 40).kind == 2 ? 1 : 0;
}

// mmseg_conv3_wgrad with x the PRE-norm activation of an InstanceNorm + ReLU ([N][Cip] mean / rstd), applied on
// staging exactly as mmseg_instnorm_relu_fwd would write it (requires mmseg_conv3_wgrad_norm_ok).
int mmseg_conv3_wgrad_norm(const void* dy, int lddy, const void* x, int ldx, const float* nmean, const float* nrstd,
                           float* grad, float* bias_grad, int Co, int Cip, int Ci, int cpg_shift, long long V, int D,
                           int H, int W, float* ws, long long ws_floats, int accumulate, int dtype, void* stream) {
  MMSEG_REQUIRE(nmean && nrstd && mmseg_conv3_wgrad_norm_ok(V, Co, Cip, Ci, cpg_shift, D, H, W, lddy, ldx, dtype),
                "conv3_wgrad_norm: unsupported shape (mmseg_conv3_wgrad_norm_ok)");
  return conv3_wgrad_impl(dy, lddy, x, ldx, nmean, nrstd, grad, bias_grad, Co, Cip, Ci, cpg_shift, V, D, H, W, ws,
                          ws_floats, accumulate, dtype, stream);
}

// mmseg_conv3_wgrad in two phases (bit 1: the weight-gradient kernel, bit 2: the split reduce), so a caller can
// time the kernel alone; nmean / nrstd optional (deferred norm of x, see mmseg_conv3_wgrad_norm).
int mmseg_conv3_wgrad_ex(const void* dy, int lddy, const void* x, int ldx, const float* nmean, const float* nrstd,
                         float* grad, float* bias_grad, int Co, int Cip, int Ci, int cpg_shift, long long V, int D,
                         int H, int W, float* ws, long long ws_floats, int accumulate, int phase, int dtype,
                         void* stream) {
  MMSEG_REQUIRE(phase >= 1 && phase <= 15 && (phase & 3) && (!(phase & 8) || (Co >= 16 && Co % 16 == 0)),
                "conv3_wgrad_ex: phase %d: bits 1 | 2 (| 4 defer, | 8 last 16 rows padding)", phase);
  MMSEG_REQUIRE(!nmean || (nrstd && mmseg_conv3_wgrad_norm_ok(V, Co, Cip, Ci, cpg_shift, D, H, W, lddy, ldx, dtype)),
                "conv3_wgrad_ex: unsupported shape for the deferred norm (mmseg_conv3_wgrad_norm_ok)");
  return conv3_wgrad_impl(dy, lddy, x, ldx, nmean, nrstd, grad, bias_grad, Co, Cip, Ci, cpg_shift, V, D, H, W, ws,
                          ws_floats, accumulate, dtype, stream, phase);
}

int conv3_wgrad_impl(const void* dy, int lddy, const void* x, int ldx, const float* nmean, const float* nrstd,
                     float* grad, float* bias_grad, int Co, int Cip, int Ci, int cpg_shift, long long V, int D, int H,
                     int W, float* ws, long long ws_floats, int accumulate, int dtype, void* stream, int phase,
                     int groups, long long grad_gstride, int bias_gstride) {
  MMSEG_REQUIRE(Co % 8 == 0 && Cip % 8 == 0 && Ci <= Cip && (8 << cpg_shift) == Cip,
                "conv3_wgrad: Co=%d, Cip=%d must be multiples of 8, Ci=%d <= Cip, Cip = 8 << cpg_shift", Co, Cip, Ci);
  const Conv3WgradChoice p = choose_conv3_wgrad(V, Co, Cip, Ci, cpg_shift, D, H, W, lddy, ldx, dtype, ws_floats, groups,
                                                nmean != nullptr, (phase & 8) != 0);
  MMSEG_REQUIRE(!nmean || p.kind == 2, "conv3_wgrad: a deferred norm needs the brick2 weight-gradient kernel");
  MMSEG_REQUIRE(groups <= 1 || p.kind == 3, "conv3_wgrad_group: only the runtime-brick weight gradient is grouped");
  MMSEG_REQUIRE(p.ws <= ws_floats && (p.ws == 0 || ws != nullptr), "conv3_wgrad: workspace of %lld floats < %lld",
                ws_floats, p.ws);
  const int ncols = 27 * Cip;
  float* part = p.direct ? nullptr : ws;
  float* bpart = (p.direct || bias_grad == nullptr) ? nullptr : ws + (long long)p.ksplit * Co * ncols;
  const long long vps = ((V + p.ksplit - 1) / p.ksplit + 63) / 64 * 64;
  // XCD swizzle: each XCD walks a contiguous range of (split, row tile, channel chunk) tiles,
  // so the chunks of one brick range -- which all read the same dy -- and neighbouring brick ranges -- which share
  // halo planes -- meet in one L2 (r04e A/B: 6.38 -> 6.35 ms/step)
  WgradArgs g{dy, lddy, x, ldx, part, p.direct ? bias_grad : bpart, Co, ncols, cpg_shift, V, D, H, W, p.ksplit, vps,
              1, p.kind, p.direct ? grad : nullptr, p.direct ? bias_grad : nullptr,
              accumulate, wgrad_kchunks(Cip, Ci), nmean, nrstd};
  hipStream_t s = (hipStream_t)stream;
  g.frag = p.fmt > 0;
  g.groups = groups > 1 ? groups : 0;
  g.grad_gstride = grad_gstride;
  g.bias_gstride = bias_gstride;
  g.pad16 = (phase & 8) ? 1 : 0;
  g.grad_ld = p.direct ? 27 * Ci : 0;
  if (phase & 1) {
    const int rc = dtype == MMSEG_BF16 ? launch_wgrad_mode<bf16_t>(g, p, MODE_CONV3, s)
                                       : launch_wgrad_mode<float>(g, p, MODE_CONV3, s);
    if (rc) return rc;
  }
  if (p.direct || !(phase & 2)) return 0;
  const int ng = groups > 1 ? groups : 1;
  WReduceArgs r{part, grad, bpart, bias_grad, Co, ncols, p.ksplit / ng, Cip, Ci, 27, accumulate, p.kind >= 2 ? 1 : 0,
                p.fmt, wgrad_nchunk(cpg_shift, g.kchunks), grad_gstride, bias_gstride};
  r.vec4 = r.chmajor && !r.frag_mt && ((uintptr_t)grad & 15) == 0 &&
           (ng == 1 || grad_gstride % 4 == 0) && r.Ncols % 4 == 0 && ((long long)r.creal * r.ntap) % 4 == 0;
  if (phase & 4) {   // deferred: summed by the next mmseg_wgrad_reduce_flush on this stream
    return wred_push(r, ng, stream);
  }
  return launch_wgrad_reduce(r, stream, ng);
}

// Bias gradient: out[c] (+)= sum_v dy[v][c]; part must hold nblk*C floats.
int mmseg_colsum(const void* dy, int ld, int C, long long V, float* part, int nblk, float* out, int accumulate,
                 int dtype, void* stream) {
  MMSEG_REQUIRE(C % 8 == 0 && C / 8 <= 256, "colsum: C=%d must be a multiple of 8 and <= 2048", C);
  long long vps = (V + nblk - 1) / nblk;
  nblk = (int)((V + vps - 1) / vps);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MMSEG_BF16)
    MMSEG_LAUNCH(colsum_partial_kernel<bf16_t>, dim3(nblk), dim3(256), 0, s, (const bf16_t*)dy, ld, C, V, vps,
                       part);
  else
    MMSEG_LAUNCH(colsum_partial_kernel<float>, dim3(nblk), dim3(256), 0, s, (const float*)dy, ld, C, V, vps,
                       part);
  if (mmseg::check_launch("colsum_partial")) return 1;
  MMSEG_LAUNCH(colsum_reduce_kernel, dim3(C), dim3(256), 0, s, part, nblk, C, out, accumulate);
  return mmseg::check_launch("colsum_reduce");
}

// out[c] (=, or += with accumulate) = sum over b < nblk of part[b][c], fixed order; the transposed conv's bias
// gradient from mmseg_wgrad's CONVT column-sum partials is mmseg_colsum_reduce(bias_part, 8 * ksplit, Cout, ...).
int mmseg_colsum_reduce(const float* part, int nblk, int C, float* out, int accumulate, void* stream) {
  MMSEG_REQUIRE(nblk >= 1 && C >= 1, "colsum_reduce: nblk, C >= 1");
  MMSEG_LAUNCH(colsum_reduce_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, part, nblk, C, out,
                     accumulate);
  return mmseg::check_launch("colsum_reduce");
}

}  // extern "C"
