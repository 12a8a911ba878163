// HBM-bound kernels of the DownBlock3D / DualEncoder fusion path.
//
//   MaxPool3d(2) forward with argmax (ties -> first in z,y,x scan order)
//   modality fusion forward: weighted sum over M level tensors
//   CrossModalAttention gate (dual_encoder.py:207-254): pooled mean -> Linear ->
//       ReLU -> Linear -> softmax, and its backward.
//   Each forward also comes over a deferred InstanceNorm + ReLU of its sources (instnorm.hip's in_relu_apply values).
//
// All reductions are two-level and fixed-order (per-block partials, then a
// single-thread-per-output sweep), so results are bitwise reproducible.
#include "mmseg_common.h"
#include "instnorm_ops.h"

namespace {

// --------------------------------------------------------------- maxpool
// 2x2x2, stride 2.  idx = a*4 + b*2 + c (z,y,x), first maximum wins.
// NORM: x is the PRE-norm activation and the pooled values are relu((x - mean) * rstd) rounded to T, i.e.
// exactly in_relu_apply's output, so values and argmax (ties included) equal pooling the materialised
// InstanceNorm + ReLU output, which then never has to be written (DualEncoder mean / add fusion).
template <typename T, bool NORM = false>
__global__ void maxpool2_fwd(const T* __restrict__ x, int ldx, T* __restrict__ y, int ldy,
                             uint8_t* __restrict__ idx, int N, int D, int H, int W, int C,
                             const float* __restrict__ mean = nullptr, const float* __restrict__ rstd = nullptr) {
  const int C8 = C >> 3;
  const int Do = D >> 1, Ho = H >> 1, Wo = W >> 1;
  // 32-bit item index (the host requires N * Vo * C8 < 2^31): the former 64-bit divisions were most of the
  // kernel's VALU work
  const int total = N * Do * Ho * Wo * C8;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int cg = i % C8;
    int q = i / C8;
    const int xo = q % Wo;
    q /= Wo;
    const int yo = q % Ho;
    q /= Ho;
    const int zo = q % Do;
    const int n = q / Do;
    const long long in0 = ((long long)(n * D + 2 * zo) * H + 2 * yo) * (long long)W + 2 * xo;
    float best[8];
    uint8_t bi[8];
    float mu[8], rs[8];
    if constexpr (NORM) {
      load8f(mean + n * C + cg * 8, mu);
      load8f(rstd + n * C + cg * 8, rs);
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const long long vin = in0 + ((long long)(t >> 2) * H + ((t >> 1) & 1)) * W + (t & 1);
      V8<T> a;
      a.load(x + vin * ldx + cg * 8);
      if constexpr (NORM) norm_relu8(a, mu, rs);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // torch CPU max_pool3d: (val > maxval) || isnan(val) replaces
        const float v = a.get(j);
        if (t == 0 || v > best[j] || v != v) {
          best[j] = v;
          bi[j] = (uint8_t)t;
        }
      }
    }
    V8<T> o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.set(j, best[j]);
    const long long vo = ((long long)(n * Do + zo) * Ho + yo) * Wo + xo;
    o.store(y + vo * ldy + cg * 8);
    uint2 packed;
    packed.x = bi[0] | (bi[1] << 8) | (bi[2] << 16) | ((uint32_t)bi[3] << 24);
    packed.y = bi[4] | (bi[5] << 8) | (bi[6] << 16) | ((uint32_t)bi[7] << 24);
    *reinterpret_cast<uint2*>(idx + vo * C + cg * 8) = packed;
  }
}

// ---------------------------------------------------------------- fusion
// out[n,v,c] = sum_m w_m * src_m[n,v,c],  w_m = wconst or wts[n*M + m]
struct FuseSrc {
  const void* p[4];
  int ld[4];
  int M;
  float wconst;
  const float* wts;   // [N][M] or null
  const float* mean[4];   // NORM: per-source InstanceNorm statistics [N][C] (sources are pre-norm, + ReLU)
  const float* rstd[4];
};

template <typename T, bool NORM = false>
__global__ void fuse_fwd(FuseSrc s, T* __restrict__ out, int ldo, long long V, int N, int C) {
  const int C8 = C >> 3;
  const int total = N * (int)V * C8;   // < 2^31 (host check): 32-bit index math
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int cg = i % C8;
    const long long nv = i / C8;
    const int n = (int)(nv / (int)V);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int m = 0; m < s.M; ++m) {
      V8<T> a;
      a.load(reinterpret_cast<const T*>(s.p[m]) + nv * s.ld[m] + cg * 8);
      if constexpr (NORM) {   // in_relu_apply's value, rounded to T as the materialised output would be
        float mu[8], rs[8];
        load8f(s.mean[m] + n * C + cg * 8, mu);
        load8f(s.rstd[m] + n * C + cg * 8, rs);
        norm_relu8(a, mu, rs);
      }
      const float w = s.wts ? s.wts[n * s.M + m] : 1.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = s.wts ? fmaf(a.get(j), w, acc[j]) : acc[j] + a.get(j);
    }
    V8<T> o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.set(j, s.wts ? acc[j] : acc[j] * s.wconst);
    o.store(out + nv * ldo + cg * 8);
  }
}

// fuse_fwd<NORM> with the source count MM known at compile time: the MM feature loads of an item are issued
// together (the runtime-M loop waited a memory latency per source), and since the grid stride is a multiple of
// C / 8 a thread's channel group never changes, so the sources' statistics are loaded once per sample instead
// of once per item.  Same operations in the same order as fuse_fwd<NORM>: bitwise equal.
template <typename T, int MM>
__global__ void fuse_norm_fwd_m(FuseSrc s, T* __restrict__ out, int ldo, long long V, int N, int C) {
  const int C8 = C >> 3;
  const int total = N * (int)V * C8;   // < 2^31 (host check): 32-bit index math
  const int stride = gridDim.x * blockDim.x;   // a multiple of C8 (host check)
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = i % C8;
  int cur_n = -1;
  float mu[MM][8], rs[MM][8];
  for (; i < total; i += stride) {
    const long long nv = i / C8;
    const int n = (int)(nv / (int)V);
    V8<T> a[MM];
#pragma unroll
    for (int m = 0; m < MM; ++m) a[m].load(reinterpret_cast<const T*>(s.p[m]) + nv * s.ld[m] + cg * 8);
    if (n != cur_n) {
#pragma unroll
      for (int m = 0; m < MM; ++m) {
        load8f(s.mean[m] + n * C + cg * 8, mu[m]);
        load8f(s.rstd[m] + n * C + cg * 8, rs[m]);
      }
      cur_n = n;
    }
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int m = 0; m < MM; ++m) {
      // through a lambda: called directly, the bf16 MM = 2 kernel took 81 VGPRs, not 78 (5 waves per SIMD, not 6)
      [&] { norm_relu8(a[m], mu[m], rs[m]); }();
      const float w = s.wts ? s.wts[n * s.M + m] : 1.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = s.wts ? fmaf(a[m].get(j), w, acc[j]) : acc[j] + a[m].get(j);
    }
    V8<T> o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.set(j, s.wts ? acc[j] : acc[j] * s.wconst);
    o.store(out + nv * ldo + cg * 8);
  }
}

// Mean / add fusion and the MaxPool of every source in ONE pass over the sources: an encoder level's output is
// read by exactly these two consumers (fuse_norm_fwd_m / fuse_fwd and maxpool2_fwd per source), which ran as
// separate launches and each fetched the level again from HBM.  One thread owns one pooled voxel and 8 channels
// of one sample: it loads the window's 8 voxels of all MM sources (16-B loads, issued before use), writes the 8
// fused voxels, and per source the pooled voxel and the argmax codes.
// Same operations in the same order as the kernels it replaces, so every output is bitwise theirs: the value is
// relu((x - mean) * rstd) rounded to T (NORM) or the source as stored, the fusion is acc = 0 + a_0 + a_1 .. times
// wconst, and the pool takes the first maximum in z, y, x order (torch's rule: v > best or v is NaN replaces).
struct FusePoolSrc {
  const void* p[3];
  int ld[3];
  const float* mean[3];   // NORM: [N][C] per source
  const float* rstd[3];
  void* y[3];             // pooled [N][Vo] rows of ldy[m]
  int ldy[3];
  uint8_t* idx[3];        // argmax codes [N][Vo][C]
  float wconst;
};

template <typename T, int MM, bool NORM>
__global__ __launch_bounds__(256) void fuse_pool_fwd_m(FusePoolSrc s, T* __restrict__ out, int ldo, int N, int D,
                                                       int H, int W, int C) {
  const int C8 = C >> 3;
  const int Do = D >> 1, Ho = H >> 1, Wo = W >> 1;
  const int total = N * Do * Ho * Wo * C8;   // < 2^31 (host check)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int cg = i % C8;
  int q = i / C8;
  const int xo = q % Wo;
  q /= Wo;
  const int yo = q % Ho;
  q /= Ho;
  const int zo = q % Do;
  const int n = q / Do;
  const long long in0 = ((long long)(n * D + 2 * zo) * H + 2 * yo) * (long long)W + 2 * xo;
  const long long vo = ((long long)(n * Do + zo) * Ho + yo) * Wo + xo;
  // window voxels in flight at once: all 8 for 16-B vectors, fewer for fp32 (the registers of 8 x MM 32-B vectors
  // would spill)
  constexpr int TB = sizeof(T) == 2 ? 8 : (MM == 2 ? 4 : 2);
  float mu[MM][8], rs[MM][8];
  if constexpr (NORM) {
#pragma unroll
    for (int m = 0; m < MM; ++m) {
      load8f(s.mean[m] + n * C + cg * 8, mu[m]);
      load8f(s.rstd[m] + n * C + cg * 8, rs[m]);
    }
  }
  float best[MM][8];
  uint8_t bi[MM][8];
#pragma unroll
  for (int t0 = 0; t0 < 8; t0 += TB) {
    V8<T> a[TB][MM];
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      const int t = t0 + u;
      const long long vin = in0 + ((long long)(t >> 2) * H + ((t >> 1) & 1)) * W + (t & 1);
#pragma unroll
      for (int m = 0; m < MM; ++m) a[u][m].load(reinterpret_cast<const T*>(s.p[m]) + vin * s.ld[m] + cg * 8);
    }
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      const int t = t0 + u;
      const long long vin = in0 + ((long long)(t >> 2) * H + ((t >> 1) & 1)) * W + (t & 1);
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
      for (int m = 0; m < MM; ++m) {
        if constexpr (NORM) norm_relu8(a[u][m], mu[m], rs[m]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float v = a[u][m].get(j);
          acc[j] = acc[j] + v;
          if (t == 0 || v > best[m][j] || v != v) {
            best[m][j] = v;
            bi[m][j] = (uint8_t)t;
          }
        }
      }
      V8<T> o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o.set(j, acc[j] * s.wconst);
      o.store(out + vin * ldo + cg * 8);
    }
  }
#pragma unroll
  for (int m = 0; m < MM; ++m) {
    V8<T> o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.set(j, best[m][j]);
    o.store(reinterpret_cast<T*>(s.y[m]) + vo * s.ldy[m] + cg * 8);
    uint2 packed;
    packed.x = bi[m][0] | (bi[m][1] << 8) | (bi[m][2] << 16) | ((uint32_t)bi[m][3] << 24);
    packed.y = bi[m][4] | (bi[m][5] << 8) | (bi[m][6] << 16) | ((uint32_t)bi[m][7] << 24);
    *reinterpret_cast<uint2*>(s.idx[m] + vo * C + cg * 8) = packed;
  }
}

// dots[n][m] partial: sum_{v,c} dfused[n,v,c] * src_m[n,v,c]
template <typename T>
__global__ void fuse_dot_partial(FuseSrc s, const T* __restrict__ dfused, int ldd, long long V, int C, long long vpc,
                                 float* __restrict__ part) {
  const int n = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x;
  const int C8 = C >> 3;
  const int tid = threadIdx.x;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const long long v0 = (long long)chunk * vpc;
  long long v1 = v0 + vpc;
  if (v1 > V) v1 = V;
  const long long e0 = v0 * C8, e1 = v1 * C8;
  for (long long e = e0 + tid; e < e1; e += 256) {
    const long long v = e / C8;
    const int cg = (int)(e - v * C8);
    const long long nv = (long long)n * V + v;
    V8<T> d;
    d.load(dfused + nv * ldd + cg * 8);
    for (int m = 0; m < s.M; ++m) {
      V8<T> a;
      a.load(reinterpret_cast<const T*>(s.p[m]) + nv * s.ld[m] + cg * 8);
      float t = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) t = fmaf(a.get(j), d.get(j), t);
      acc[m] += t;
    }
  }
  __shared__ float red[4][4];
  const int lane = tid & 63, wave = tid >> 6;
  for (int m = 0; m < s.M; ++m) {
    float w = wave_sum(acc[m]);
    if (lane == 0) red[m][wave] = w;
  }
  __syncthreads();
  if (tid < s.M) part[((long long)n * nchunk + chunk) * 4 + tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
}

// ---------------------------------------------------- attention gate (SE)
// pooled [N][MC] -> h = relu(W1 pooled + b1) [N][Hd] -> logits = W2 h + b2 [N][M] -> w = softmax
__global__ void attn_gate_fwd(const float* __restrict__ pooled, const float* __restrict__ W1,
                              const float* __restrict__ b1, const float* __restrict__ W2, const float* __restrict__ b2,
                              float* __restrict__ hbuf, float* __restrict__ wts, int MC, int Hd, int M) {
  const int n = blockIdx.x;
  extern __shared__ float sh[];
  float* h = sh;  // Hd
  for (int k = threadIdx.x; k < Hd; k += blockDim.x) {
    float a = 0.f;
    for (int i = 0; i < MC; ++i) a = fmaf(W1[(long long)k * MC + i], pooled[(long long)n * MC + i], a);
    a += b1[k];
    a = a > 0.f ? a : 0.f;
    h[k] = a;
    hbuf[(long long)n * Hd + k] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float lg[4];
    float mx = -INFINITY;
    for (int m = 0; m < M; ++m) {
      float a = 0.f;
      for (int k = 0; k < Hd; ++k) a = fmaf(W2[m * Hd + k], h[k], a);
      lg[m] = a + b2[m];
      mx = fmaxf(mx, lg[m]);
    }
    float se = 0.f;
    for (int m = 0; m < M; ++m) {
      lg[m] = expf(lg[m] - mx);
      se += lg[m];
    }
    for (int m = 0; m < M; ++m) wts[n * M + m] = lg[m] / se;
  }
}

// Backward of the gate for all N (one block): inputs dots part -> dw[n][m];
// writes beta[n][MC] = dpooled / V and the Linear gradients (accumulated).
__global__ void attn_gate_bwd(const float* __restrict__ dot_part, int nchunk, const float* __restrict__ pooled,
                              const float* __restrict__ W1, const float* __restrict__ W2,
                              const float* __restrict__ hbuf, const float* __restrict__ wts, float* __restrict__ beta,
                              float* __restrict__ gW1, float* __restrict__ gb1, float* __restrict__ gW2,
                              float* __restrict__ gb2, int N, int MC, int Hd, int M, long long V, int accumulate) {
  extern __shared__ float sh[];
  float* dlog = sh;              // N*M
  float* dh = sh + N * M;        // N*Hd
  const int tid = threadIdx.x;
  if (tid < N * M) {
    const int n = tid / M, m = tid % M;
    // dw for (n, *) in fixed order
    float dw[4];
    float s = 0.f;
    for (int mm = 0; mm < M; ++mm) {
      float a = 0.f;
      for (int k = 0; k < nchunk; ++k) a += dot_part[((long long)n * nchunk + k) * 4 + mm];
      dw[mm] = a;
      s += wts[n * M + mm] * a;
    }
    dlog[tid] = wts[n * M + m] * (dw[m] - s);
  }
  __syncthreads();
  for (int e = tid; e < N * Hd; e += blockDim.x) {
    const int n = e / Hd, k = e % Hd;
    float a = 0.f;
    for (int m = 0; m < M; ++m) a = fmaf(W2[m * Hd + k], dlog[n * M + m], a);
    dh[e] = hbuf[e] > 0.f ? a : 0.f;
  }
  __syncthreads();
  // Linear2 grads
  for (int e = tid; e < M * Hd; e += blockDim.x) {
    const int m = e / Hd, k = e % Hd;
    float a = 0.f;
    for (int n = 0; n < N; ++n) a = fmaf(dlog[n * M + m], hbuf[n * Hd + k], a);
    gW2[e] = accumulate ? gW2[e] + a : a;
  }
  for (int m = tid; m < M; m += blockDim.x) {
    float a = 0.f;
    for (int n = 0; n < N; ++n) a += dlog[n * M + m];
    gb2[m] = accumulate ? gb2[m] + a : a;
  }
  // Linear1 grads and dpooled
  for (long long e = tid; e < (long long)Hd * MC; e += blockDim.x) {
    const int k = (int)(e / MC), i = (int)(e % MC);
    float a = 0.f;
    for (int n = 0; n < N; ++n) a = fmaf(dh[n * Hd + k], pooled[(long long)n * MC + i], a);
    gW1[e] = accumulate ? gW1[e] + a : a;
  }
  for (int k = tid; k < Hd; k += blockDim.x) {
    float a = 0.f;
    for (int n = 0; n < N; ++n) a += dh[n * Hd + k];
    gb1[k] = accumulate ? gb1[k] + a : a;
  }
  const float invV = 1.f / (float)V;
  for (long long e = tid; e < (long long)N * MC; e += blockDim.x) {
    const int n = (int)(e / MC), i = (int)(e % MC);
    float a = 0.f;
    for (int k = 0; k < Hd; ++k) a = fmaf(W1[(long long)k * MC + i], dh[n * Hd + k], a);
    beta[e] = a * invV;
  }
}

// Kernels with a 32-bit grid-stride index (maxpool2_fwd, fuse_fwd) step i by up to 8192 * 256 = 2^21: the
// item count must stay that far below INT_MAX so the last i += stride cannot wrap negative.
constexpr long long kGridStrideMax = 2147483647LL - 8192LL * 256;

// dynamic LDS a gate kernel may ask for (a launch over the 64 KB default limit fails)
constexpr long long kGateLdsBytes = 64 * 1024;

int grid_for(long long total) {
  long long b = (total + 255) / 256;
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

extern "C" {

int mmseg_maxpool2_fwd(const void* x, int ldx, void* y, int ldy, uint8_t* idx, int N, int D, int H, int W, int C,
                       int dtype, void* stream) {
  MMSEG_REQUIRE(C % 8 == 0 && ((D | H | W) & 1) == 0, "maxpool2: C%%8==0 and even dims required");
  MMSEG_REQUIRE((long long)N * (D / 2) * (H / 2) * (W / 2) * (C / 8) <= kGridStrideMax, "maxpool2: too many items");
  hipStream_t s = (hipStream_t)stream;
  const int grid = grid_for((long long)N * (D / 2) * (H / 2) * (W / 2) * (C / 8));
  by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    MMSEG_LAUNCH(maxpool2_fwd<T>, dim3(grid), dim3(256), 0, s, (const T*)x, ldx, (T*)y, ldy, idx, N, D, H, W, C,
                 (const float*)nullptr, (const float*)nullptr);
  });
  return mmseg::check_launch("maxpool2_fwd");
}

// mmseg_maxpool2_fwd over relu((x - mean) * rstd) (x pre-norm, mean / rstd [N][C]): equal to pooling the
// materialised InstanceNorm + ReLU output.
int mmseg_maxpool2_norm_fwd(const void* x, int ldx, const float* mean, const float* rstd, void* y, int ldy,
                            uint8_t* idx, int N, int D, int H, int W, int C, int dtype, void* stream) {
  MMSEG_REQUIRE(C % 8 == 0 && ((D | H | W) & 1) == 0, "maxpool2: C%%8==0 and even dims required");
  MMSEG_REQUIRE((long long)N * (D / 2) * (H / 2) * (W / 2) * (C / 8) <= kGridStrideMax, "maxpool2: too many items");
  hipStream_t s = (hipStream_t)stream;
  const int grid = grid_for((long long)N * (D / 2) * (H / 2) * (W / 2) * (C / 8));
  by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    MMSEG_LAUNCH((maxpool2_fwd<T, true>), dim3(grid), dim3(256), 0, s, (const T*)x, ldx, (T*)y, ldy, idx, N, D, H, W,
                 C, mean, rstd);
  });
  return mmseg::check_launch("maxpool2_norm_fwd");
}

// mmseg_fuse_fwd over relu((src_m - mean_m) * rstd_m) (pre-norm sources, statistics [N][C] per source)
int mmseg_fuse_norm_fwd(const void* const* srcs, const int* lds, const float* const* means, const float* const* rstds,
                        int M, float wconst, const float* wts, void* out, int ldo, int N, long long V, int C,
                        int dtype, void* stream) {
  MMSEG_REQUIRE(M >= 1 && M <= 4 && C % 8 == 0, "fuse: 1 <= M <= 4 and C%%8==0");
  MMSEG_REQUIRE((long long)N * V * (C / 8) <= kGridStrideMax, "fuse: too many items");
  FuseSrc s{};
  for (int m = 0; m < M; ++m) {
    s.p[m] = srcs[m];
    s.ld[m] = lds[m];
    s.mean[m] = means[m];
    s.rstd[m] = rstds[m];
  }
  s.M = M;
  s.wconst = wconst;
  s.wts = wts;
  hipStream_t st = (hipStream_t)stream;
  const int grid = grid_for((long long)N * V * (C / 8));
  // compile-time M for 2 and 3 sources (M = 4 spilled and stays runtime-M)
  const bool cm = M >= 2 && ((long long)grid * 256) % (C / 8) == 0;
  by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (cm && M == 2)
      MMSEG_LAUNCH((fuse_norm_fwd_m<T, 2>), dim3(grid), dim3(256), 0, st, s, (T*)out, ldo, V, N, C);
    else if (cm && M == 3)
      MMSEG_LAUNCH((fuse_norm_fwd_m<T, 3>), dim3(grid), dim3(256), 0, st, s, (T*)out, ldo, V, N, C);
    else
      MMSEG_LAUNCH((fuse_fwd<T, true>), dim3(grid), dim3(256), 0, st, s, (T*)out, ldo, V, N, C);
  });
  return mmseg::check_launch("fuse_norm_fwd");
}

// out = wconst * sum_m src_m   (wts == null)   or   sum_m wts[n][m] * src_m
int mmseg_fuse_fwd(const void* const* srcs, const int* lds, int M, float wconst, const float* wts, void* out, int ldo,
                   int N, long long V, int C, int dtype, void* stream) {
  MMSEG_REQUIRE(M >= 1 && M <= 4 && C % 8 == 0, "fuse: 1 <= M <= 4 and C%%8==0");
  MMSEG_REQUIRE((long long)N * V * (C / 8) <= kGridStrideMax, "fuse: too many items");
  FuseSrc s{};
  for (int m = 0; m < M; ++m) {
    s.p[m] = srcs[m];
    s.ld[m] = lds[m];
  }
  s.M = M;
  s.wconst = wconst;
  s.wts = wts;
  hipStream_t st = (hipStream_t)stream;
  const int grid = grid_for((long long)N * V * (C / 8));
  by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    MMSEG_LAUNCH(fuse_fwd<T>, dim3(grid), dim3(256), 0, st, s, (T*)out, ldo, V, N, C);
  });
  return mmseg::check_launch("fuse_fwd");
}

// mmseg_fuse_fwd (wts null; means null) or mmseg_fuse_norm_fwd (means / rstds given) into `out`, and per source
// mmseg_maxpool2_fwd / mmseg_maxpool2_norm_fwd into ys[m] / idxs[m], as one launch.
int mmseg_fuse_pool_fwd(const void* const* srcs, const int* lds, const float* const* means, const float* const* rstds,
                        int M, float wconst, void* out, int ldo, void* const* ys, const int* ldys,
                        uint8_t* const* idxs, int N, int D, int H, int W, int C, int dtype, void* stream) {
  MMSEG_REQUIRE((M == 2 || M == 3) && C % 8 == 0 && C > 0, "fuse_pool: M in {2, 3} and C%%8==0 required");
  MMSEG_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && ((D | H | W) & 1) == 0, "fuse_pool: even dims required");
  MMSEG_REQUIRE((means == nullptr) == (rstds == nullptr), "fuse_pool: means and rstds go together");
  const long long total = (long long)N * (D / 2) * (H / 2) * (W / 2) * (C / 8);
  // 32-bit item index, and n * D + z as an int in the kernel
  MMSEG_REQUIRE(total <= kGridStrideMax && (long long)N * D < 2147483647LL, "fuse_pool: too many items");
  FusePoolSrc s{};
  for (int m = 0; m < M; ++m) {
    MMSEG_REQUIRE(srcs[m] && ys[m] && idxs[m] && lds[m] >= C && ldys[m] >= C && lds[m] % 8 == 0 && ldys[m] % 8 == 0,
                  "fuse_pool: source / pooled rows of at least C, multiples of 8");
    s.p[m] = srcs[m];
    s.ld[m] = lds[m];
    if (means) {
      MMSEG_REQUIRE(means[m] && rstds[m], "fuse_pool: statistics of every source");
      s.mean[m] = means[m];
      s.rstd[m] = rstds[m];
    }
    s.y[m] = ys[m];
    s.ldy[m] = ldys[m];
    s.idx[m] = idxs[m];
  }
  MMSEG_REQUIRE(out && ldo >= C && ldo % 8 == 0, "fuse_pool: output rows of at least C, a multiple of 8");
  s.wconst = wconst;
  hipStream_t st = (hipStream_t)stream;
  const int grid = (int)((total + 255) / 256);
  by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (M == 2 && means)
      MMSEG_LAUNCH((fuse_pool_fwd_m<T, 2, true>), dim3(grid), dim3(256), 0, st, s, (T*)out, ldo, N, D, H, W, C);
    else if (M == 2)
      MMSEG_LAUNCH((fuse_pool_fwd_m<T, 2, false>), dim3(grid), dim3(256), 0, st, s, (T*)out, ldo, N, D, H, W, C);
    else if (means)
      MMSEG_LAUNCH((fuse_pool_fwd_m<T, 3, true>), dim3(grid), dim3(256), 0, st, s, (T*)out, ldo, N, D, H, W, C);
    else
      MMSEG_LAUNCH((fuse_pool_fwd_m<T, 3, false>), dim3(grid), dim3(256), 0, st, s, (T*)out, ldo, N, D, H, W, C);
  });
  return mmseg::check_launch("fuse_pool_fwd");
}

int mmseg_attn_gate_fwd(const float* pooled, const float* W1, const float* b1, const float* W2, const float* b2,
                        float* hbuf, float* wts, int N, int MC, int Hd, int M, void* stream) {
  MMSEG_REQUIRE(M >= 1 && M <= 4, "attn gate: M=%d outside [1, 4]", M);
  MMSEG_REQUIRE(N > 0 && MC > 0 && Hd > 0, "attn gate: N=%d, MC=%d, Hd=%d must be positive", N, MC, Hd);
  MMSEG_REQUIRE((long long)Hd * (long long)sizeof(float) <= kGateLdsBytes, "attn gate: Hd=%d floats exceed the LDS", Hd);
  MMSEG_REQUIRE(pooled && W1 && b1 && W2 && b2 && hbuf && wts, "attn gate: null operand");
  MMSEG_LAUNCH(attn_gate_fwd, dim3(N), dim3(256), Hd * sizeof(float), (hipStream_t)stream, pooled, W1, b1, W2,
                     b2, hbuf, wts, MC, Hd, M);
  return mmseg::check_launch("attn_gate_fwd");
}

// Backward of the attention fusion gate.  Computes dw from (dfused . src_m),
// then beta = dpooled / V (feed to instnorm_relu_bwd) and the Linear grads.
int mmseg_attn_gate_bwd(const void* const* srcs, const int* lds, int M, const void* dfused, int ldd, int N, long long V,
                        int C, const float* pooled, const float* W1, const float* W2, const float* hbuf,
                        const float* wts, float* beta, float* gW1, float* gb1, float* gW2, float* gb2, int Hd,
                        float* ws, int accumulate, int dtype, void* stream) {
  MMSEG_REQUIRE(M >= 1 && M <= 4 && C > 0 && C % 8 == 0, "attn gate bwd: M=%d outside [1, 4] or C=%d no multiple of 8", M,
                C);
  MMSEG_REQUIRE(N > 0 && V > 0 && Hd > 0, "attn gate bwd: N=%d, V=%lld, Hd=%d must be positive", N, V, Hd);
  // attn_gate_bwd is ONE 256-thread block: thread n * M + m owns dlogit[n][m], and dlogit / dh live in dynamic LDS
  MMSEG_REQUIRE((long long)N * M <= 256, "attn gate bwd: N*M=%lld exceeds the 256 threads of the gate block",
                (long long)N * M);
  MMSEG_REQUIRE(((long long)N * M + (long long)N * Hd) * (long long)sizeof(float) <= kGateLdsBytes,
                "attn gate bwd: (N*M + N*Hd) floats exceed the LDS (N=%d, M=%d, Hd=%d)", N, M, Hd);
  MMSEG_REQUIRE(srcs && lds && dfused && pooled && W1 && W2 && hbuf && wts && beta && gW1 && gb1 && gW2 && gb2 && ws,
                "attn gate bwd: null operand");
  for (int m = 0; m < M; ++m) MMSEG_REQUIRE(srcs[m], "attn gate bwd: source %d is null", m);
  FuseSrc s{};
  for (int m = 0; m < M; ++m) {
    s.p[m] = srcs[m];
    s.ld[m] = lds[m];
  }
  s.M = M;
  long long want = 256 * 64;
  long long nch = (V * (C / 8) + want - 1) / want;
  if (nch > 256) nch = 256;
  long long vpc = (V + nch - 1) / nch;
  nch = (V + vpc - 1) / vpc;
  hipStream_t st = (hipStream_t)stream;
  by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    MMSEG_LAUNCH(fuse_dot_partial<T>, dim3((int)nch, N), dim3(256), 0, st, s, (const T*)dfused, ldd, V, C, vpc, ws);
  });
  if (mmseg::check_launch("fuse_dot_partial")) return 1;
  const int MC = M * C;
  const size_t shm = (size_t)(N * M + N * Hd) * sizeof(float);
  MMSEG_LAUNCH(attn_gate_bwd, dim3(1), dim3(256), shm, st, ws, (int)nch, pooled, W1, W2, hbuf, wts, beta, gW1,
                     gb1, gW2, gb2, N, MC, Hd, M, V, accumulate);
  return mmseg::check_launch("attn_gate_bwd");
}

}  // extern "C"
