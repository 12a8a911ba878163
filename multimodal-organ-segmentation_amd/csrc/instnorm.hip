// InstanceNorm3d(affine=False, eps=1e-5, biased variance) + activation, forward and backward.
//
//   InstanceNorm3d + ReLU (reference unet.py:34-35,45,53-60)   -> instnorm_stats / _relu_fwd
//   its backward (+ ReLU mask)                    -> instnorm_relu_bwd_{reduce,apply}
//       with the MaxPool3d(2) backward (unet.py:73) and the fusion backward
//       (dual_encoder.py:193-195 mean / 184-186 add / 188-191 attention) fused
//       into the dy gather, so neither the pooled gradient nor the fused-level
//       gradient is ever materialised per modality.
//
// All reductions are two-level and fixed-order (per-block partials, then a
// single-thread-per-output sweep), so results are bitwise reproducible.  The per-element expressions are
// instnorm_ops.h's; the block-level reductions that kernels share are defined below, ahead of the kernels.
#include "mmseg_common.h"
#include "dy_gather.h"
#include "instnorm_ops.h"

#include <algorithm>

#include <stdlib.h>
#include <type_traits>

namespace {

// Block = (256 / C8) voxel lanes x C8 channel groups; a thread owns 8 channels
// of one sample and walks voxels v0+vl, v0+vl+lanes_v, ... of its chunk,
// issuing UNR independent 16-B loads before consuming them (the HBM latency is
// hidden by loads in flight, not by occupancy alone).
constexpr int UNR = 4;

// The small-volume kernels: one SMALL_T-thread block per (8-channel group, sample).
constexpr int SMALL_T = 256;

// --------------------------------------------------------- block reductions
// K per-thread sums of 8 channels each, over the voxel lanes of a (256 / C8) x C8 block: write(c, s) is called once
// per channel c of the block with its K sums.  Power-of-two C8: a shuffle tree over the voxel lanes of each wave
// (fixed order), then the 4 waves in order; otherwise one thread per channel adds the voxel lanes in order.
template <int K, typename F>
__device__ __forceinline__ void block_sum8(float (&acc)[K][8], int C, F&& write) {
  const int C8 = C >> 3, lanes_v = 256 / C8, tid = threadIdx.x;
  __shared__ float red[K][256 * 8];
  if ((C8 & (C8 - 1)) == 0 && C8 <= 32) {
    for (int o = 32; o >= C8; o >>= 1) {
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] += __shfl_down(acc[k][j], o, 64);
    }
    const int lane = tid & 63, wave = tid >> 6;
    if (lane < C8) {
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) red[k][(wave * C8 + lane) * 8 + j] = acc[k][j];
    }
    __syncthreads();
    if (tid < C) {
      const int g = tid >> 3, j = tid & 7;
      float s[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        s[k] = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) s[k] += red[k][(w * C8 + g) * 8 + j];
      }
      write(tid, s);
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) red[k][tid * 8 + j] = acc[k][j];
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    const int g = c >> 3, j = c & 7;
    float s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.f;
    for (int l = 0; l < lanes_v; ++l)
#pragma unroll
      for (int k = 0; k < K; ++k) s[k] += red[k][(l * C8 + g) * 8 + j];
    write(c, s);
  }
}

// Chan's merge of Welford state b into (cnt, mu, m2), 8 channels
__device__ __forceinline__ void chan_merge(float& cnt, float* mu, float* m2, float nb, const float* mb,
                                           const float* m2b) {
  const float na = cnt, nn = na + nb;
  if (nb > 0.f) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float dl = mb[j] - mu[j];
      mu[j] = mu[j] + dl * (nb / nn);
      m2[j] = m2[j] + m2b[j] + dl * dl * (na * nb / nn);
    }
    cnt = nn;
  }
}

// (mean g, mean g xhat) of a small-volume block from its threads' sums (8 channels, V voxels): wave_sum, then the 4
// waves in order through LDS; every thread gets all 8 pairs in ca / cb.
__device__ __forceinline__ void small_block_coef(float* ga, float* gb, int V, float* ca, float* cb) {
  __shared__ float sa[4][8], sb[4][8], sfin[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    ga[j] = wave_sum(ga[j]);
    gb[j] = wave_sum(gb[j]);
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sa[wave][j] = ga[j];
      sb[wave][j] = gb[j];
    }
  }
  __syncthreads();
  if (tid < 8) {
    sfin[tid] = (((sa[0][tid] + sa[1][tid]) + sa[2][tid]) + sa[3][tid]) / (float)V;
    sfin[8 + tid] = (((sb[0][tid] + sb[1][tid]) + sb[2][tid]) + sb[3][tid]) / (float)V;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    ca[j] = sfin[j];
    cb[j] = sfin[8 + j];
  }
}

// ------------------------------------------------------------------ stats
// Welford / Chan statistics: each thread keeps (n, mean, M2) for its 8
// channels; lanes are merged in a fixed order inside the block and chunks in a
// fixed order in the finalize (double).  A shifted-sums formulation is NOT
// used: convolution outputs are far from stationary near the volume border, so
// any single shift value can sit many sigmas from the channel mean and the
// E[x^2]-E[x]^2 cancellation then costs the gradients ~1e-2 accuracy.
template <typename T>
__global__ void in_stats_partial(const T* __restrict__ x, int ld, int V, int C, int vpc, float* __restrict__ part) {
  const int n = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x;
  const int C8 = C >> 3;
  const int lanes_v = 256 / C8;
  const int tid = threadIdx.x;
  const int cg = tid % C8, vl = tid / C8;
  const T* xn = x + (long long)n * V * ld + cg * 8;
  float mu[8], m2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = 0.f;
    m2[j] = 0.f;
  }
  float cnt = 0.f;
  const int v0 = chunk * vpc;
  const int v1 = v0 + vpc < V ? v0 + vpc : V;
  // through a lambda: called directly, the bf16 kernel was scheduled into 72 VGPRs, not 64 (7 waves per SIMD, not 8)
  auto upd = [&](const V8<T>& a) { welford8_update(cnt, mu, m2, a); };
  if (vl < lanes_v) {
    int v = v0 + vl;
    for (; v + (UNR - 1) * lanes_v < v1; v += UNR * lanes_v) {
      V8<T> a[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) a[u].load(xn + (long long)(v + u * lanes_v) * ld);
#pragma unroll
      for (int u = 0; u < UNR; ++u) upd(a[u]);
    }
    for (; v < v1; v += lanes_v) {
      V8<T> a;
      a.load(xn + (long long)v * ld);
      upd(a);
    }
  }
  // A Chan merge of (n, mean, M2) triples, not block_sum8's sums; and not the small-volume kernels' tree either: this one
  // is a one-sided shfl_down tree over the voxel lanes only whose mean update rounds as fmaf(delta, fb, mu), where
  // chan_merge rounds mu + dl * (nb / nn).
  __shared__ float red[2][256 * 8];
  __shared__ float rcnt[256];
  if ((C8 & (C8 - 1)) == 0 && C8 <= 32) {
    // power-of-two channel groups: the voxel lanes of a wave are merged by a
    // shuffle tree (lane l absorbs lane l+o, o = 32 .. C8: lower voxel lanes
    // stay first, fixed order), then lanes < C8 of the 4 waves go through LDS
    // and one thread per channel merges the 4 waves in order.  The serial
    // 64-lane merge below cost ~2 us per block at C = 32.
    for (int o = 32; o >= C8; o >>= 1) {
      const float nb = __shfl_down(cnt, o, 64);
      const float nn = cnt + nb;
      const float fb = nn > 0.f ? nb / nn : 0.f;
      const float fab = nn > 0.f ? cnt * fb : 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float mb = __shfl_down(mu[j], o, 64), sb = __shfl_down(m2[j], o, 64);
        const float delta = mb - mu[j];
        mu[j] = fmaf(delta, fb, mu[j]);
        m2[j] = m2[j] + sb + delta * delta * fab;
      }
      cnt = nn;
    }
    const int lane = tid & 63, wave = tid >> 6;
    if (lane < C8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        red[0][(wave * C8 + lane) * 8 + j] = mu[j];
        red[1][(wave * C8 + lane) * 8 + j] = m2[j];
      }
      rcnt[wave * C8 + lane] = cnt;
    }
    __syncthreads();
    if (tid < C) {
      const int g = tid >> 3, j = tid & 7;
      float na = 0.f, ma = 0.f, sa = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int t = w * C8 + g;
        const float nb = rcnt[t];
        if (nb == 0.f) continue;
        const float mb = red[0][t * 8 + j], sb = red[1][t * 8 + j];
        const float nn = na + nb;
        const float delta = mb - ma;
        ma = ma + delta * (nb / nn);
        sa = sa + sb + delta * delta * (na * nb / nn);
        na = nn;
      }
      float* p = part + (((long long)n * nchunk + chunk) * C + tid) * 2;
      p[0] = ma;
      p[1] = sa;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[0][tid * 8 + j] = mu[j];
    red[1][tid * 8 + j] = m2[j];
  }
  rcnt[tid] = (vl < lanes_v) ? cnt : 0.f;
  __syncthreads();
  // one thread per channel merges the voxel lanes in fixed order (Chan)
  for (int c = tid; c < C; c += 256) {
    const int g = c >> 3, j = c & 7;
    float na = 0.f, ma = 0.f, sa = 0.f;
    for (int l = 0; l < lanes_v; ++l) {
      const int t = l * C8 + g;
      const float nb = rcnt[t];
      if (nb == 0.f) continue;
      const float mb = red[0][t * 8 + j], sb = red[1][t * 8 + j];
      const float nn = na + nb;
      const float delta = mb - ma;
      ma = ma + delta * (nb / nn);
      sa = sa + sb + delta * delta * (na * nb / nn);
      na = nn;
    }
    float* p = part + (((long long)n * nchunk + chunk) * C + c) * 2;
    p[0] = ma;
    p[1] = sa;
  }
}

// one 256-thread block per (n, c): fixed-order Chan merge of the chunk partials in double
// (each thread its chunks in order, a fixed butterfly per wave, then the 4 waves in order;
// one wave per (n, c) walked ~14 dependent chunk loads per lane at 96^3)
template <typename T>
__global__ void in_stats_finalize(const T* __restrict__ x, int ld, long long V, int N, int C, int nchunk,
                                  long long vpc, const float* __restrict__ part, float eps, float* __restrict__ mean,
                                  int mean_ld, float* __restrict__ rstd) {
  const int idx = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = idx / C, c = idx - n * C;
  double na = 0.0, ma = 0.0, sa = 0.0;
  for (int k = threadIdx.x; k < nchunk; k += 256) {   // each thread: its chunks in order
    const float* p = part + (((long long)n * nchunk + k) * C + c) * 2;
    const long long v0 = (long long)k * vpc;
    const long long v1 = v0 + vpc < V ? v0 + vpc : V;
    const double nb = (double)(v1 - v0);
    if (nb <= 0) continue;
    const double nn = na + nb, delta = (double)p[0] - ma;
    ma += delta * (nb / nn);
    sa += (double)p[1] + delta * delta * (na * nb / nn);
    na = nn;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {          // fixed butterfly: deterministic Chan merge across lanes
    const double nb = __shfl_xor(na, o, 64), mb = __shfl_xor(ma, o, 64), sb = __shfl_xor(sa, o, 64);
    const double nn = na + nb;
    if (nn > 0) {
      // order the pair by lane id so both partners compute the bitwise-same result
      const bool lo = (lane & o) == 0;
      const double n1 = lo ? na : nb, m1 = lo ? ma : mb, s1 = lo ? sa : sb;
      const double n2 = lo ? nb : na, m2 = lo ? mb : ma, s2 = lo ? sb : sa;
      const double delta = m2 - m1;
      ma = m1 + delta * (n2 / nn);
      sa = s1 + s2 + delta * delta * (n1 * n2 / nn);
      na = nn;
    }
  }
  __shared__ double wred[4][3];
  if (lane == 0) {
    wred[wave][0] = na;
    wred[wave][1] = ma;
    wred[wave][2] = sa;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  na = 0.0; ma = 0.0; sa = 0.0;
  for (int w = 0; w < 4; ++w) {
    const double nb = wred[w][0];
    if (nb <= 0) continue;
    const double nn = na + nb, delta = wred[w][1] - ma;
    ma += delta * (nb / nn);
    sa += wred[w][2] + delta * delta * (na * nb / nn);
    na = nn;
  }
  const double var = sa / (double)V;
  mean[(long long)n * mean_ld + c] = (float)ma;
  if (rstd) rstd[idx] = (float)(1.0 / sqrt(var + (double)eps));
}

// y = relu((x - mean) * rstd); a thread owns 8 channels of one sample (their
// mean / rstd stay in registers) and UNR voxels per step; grid (chunks, N).
template <typename T, bool RELU = true>
__global__ void in_relu_apply(const T* __restrict__ x, int ldx, T* __restrict__ y, int ldy, int V, int C, int vpc,
                              const float* __restrict__ mean, const float* __restrict__ rstd) {
  const int n = blockIdx.y;
  const int C8 = C >> 3, lanes_v = 256 / C8;
  const int cg = threadIdx.x % C8, vl = threadIdx.x / C8;
  if (vl >= lanes_v) return;
  float mu[8], rs[8];
  load8f(mean + n * C + cg * 8, mu);
  load8f(rstd + n * C + cg * 8, rs);
  const T* xn = x + (long long)n * V * ldx + cg * 8;
  T* yn = y + (long long)n * V * ldy + cg * 8;
  const int v0 = blockIdx.x * vpc;
  const int v1 = v0 + vpc < V ? v0 + vpc : V;
  for (int vb = v0 + vl; vb < v1; vb += UNR * lanes_v) {
    V8<T> a[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u)
      if (vb + u * lanes_v < v1) a[u].load(xn + (long long)(vb + u * lanes_v) * ldx);
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (vb + u * lanes_v >= v1) break;
      norm_relu8<T, RELU>(a[u], mu, rs);
      a[u].store(yn + (long long)(vb + u * lanes_v) * ldy);
    }
  }
}

// ------------------------------------------------------------- dy gather
// (DySrc / DyCtx: dy_gather.h)

// (sample, chunk, chunks) of a partial / apply block (DySrc::gsplit)
__device__ __forceinline__ void in_block(const DySrc& s, int& n, int& chunk, int& nchunk) {
  if (s.gsplit > 1) {
    chunk = (int)blockIdx.x / s.gsplit;
    n = ((int)blockIdx.x % s.gsplit) * s.p1_nmod + (int)blockIdx.y;
    nchunk = (int)gridDim.x / s.gsplit;
  } else {
    n = (int)blockIdx.y;
    chunk = (int)blockIdx.x;
    nchunk = (int)gridDim.x;
  }
}

// 8 zeros into a row's channel padding (whole-row writes; see mmseg_instnorm_act_bwd)
template <typename T>
__device__ __forceinline__ void store_zero8(T* p) {
  V8<T> z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z.set(j, 0.f);
  z.store(p);
}

// partial sums of g and g*xhat, g = dy * [xhat > 0]
template <typename T, int ACT = 1>
__global__ void in_bwd_partial(const T* __restrict__ x, int ldx, const float* __restrict__ mean,
                               const float* __restrict__ rstd, DySrc s, int V, int C, int D, int H, int W, int vpc,
                               float* __restrict__ part) {
  int n, chunk, nchunk;
  in_block(s, n, chunk, nchunk);
  const int C8 = C >> 3;
  const int lanes_v = 256 / C8;
  const int tid = threadIdx.x;
  const int cg = tid % C8, vl = tid / C8;
  float acc[2][8], mu[8], rs[8];   // sum g, sum g xhat
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    acc[0][j] = 0.f;
    acc[1][j] = 0.f;
  }
  load8f(mean + n * C + cg * 8, mu);
  load8f(rstd + n * C + cg * 8, rs);
  const DyCtx<T> dc(s, n, V, cg, C, D, H, W);
  const T* xn = x + (long long)n * V * ldx + cg * 8;
  const int v0 = chunk * vpc;
  const int v1 = v0 + vpc < V ? v0 + vpc : V;
  if (vl < lanes_v) {
    for (int vb = v0 + vl; vb < v1; vb += UNR * lanes_v) {
      V8<T> a[UNR];
      typename DyCtx<T>::Raw r[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u)
        if (vb + u * lanes_v < v1) {
          a[u].load(xn + (long long)(vb + u * lanes_v) * ldx);
          dc.load(vb + u * lanes_v, r[u]);
        }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (vb + u * lanes_v >= v1) break;
        float dy[8];
        dc.combine(r[u], dy);
        in_bwd_sums8<T, ACT>(a[u], dy, mu, rs, s.slope, acc[0], acc[1]);
      }
    }
  }
  float* const p = part + ((long long)n * nchunk + chunk) * C * 2;
  block_sum8<2>(acc, C, [&](int c, const float* sum) {
    p[c * 2] = sum[0];
    p[c * 2 + 1] = sum[1];
  });
}

// one 256-thread block per (n, c): fixed-order double sums of the chunk partials
__global__ void in_bwd_finalize(const float* __restrict__ part, int N, int C, int nchunk, long long V,
                                float* __restrict__ coef) {
  const int idx = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = idx / C, c = idx - n * C;
  double a = 0.0, b = 0.0;
  for (int k = threadIdx.x; k < nchunk; k += 256) {
    const float* p = part + (((long long)n * nchunk + k) * C + c) * 2;
    a += p[0];
    b += p[1];
  }
  a = wave_sum_d(a);
  b = wave_sum_d(b);
  __shared__ double wred[4][2];
  if (lane == 0) {
    wred[wave][0] = a;
    wred[wave][1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = (wred[0][0] + wred[1][0]) + (wred[2][0] + wred[3][0]);
    b = (wred[0][1] + wred[1][1]) + (wred[2][1] + wred[3][1]);
    coef[idx * 2 + 0] = (float)(a / (double)V);
    coef[idx * 2 + 1] = (float)(b / (double)V);
  }
}

// dx = rstd * (g - mean(g) - xhat * mean(g * xhat)); same thread layout as the apply kernels
template <typename T, int ACT = 1, bool ZP = false>
__global__ void in_bwd_apply(const T* __restrict__ x, int ldx, const float* __restrict__ mean,
                             const float* __restrict__ rstd, DySrc s, const float* __restrict__ coef, T* __restrict__ dx,
                             int lddx, int V, int C, int D, int H, int W, int vpc, int npad) {
  int n, chunk, nchunk;
  in_block(s, n, chunk, nchunk);
  const int C8 = C >> 3, lanes_v = 256 / C8;
  const int cg = threadIdx.x % C8, vl = threadIdx.x / C8;
  if (vl >= lanes_v) return;
  float mu[8], rs[8], ca[8], cb[8];
  load8f(mean + n * C + cg * 8, mu);
  load8f(rstd + n * C + cg * 8, rs);
  {
    float t[16];
    load8f(coef + (n * C + cg * 8) * 2, t);
    load8f(coef + (n * C + cg * 8) * 2 + 8, t + 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ca[j] = t[2 * j];
      cb[j] = t[2 * j + 1];
    }
  }
  const DyCtx<T> dc(s, n, V, cg, C, D, H, W);
  const T* xn = x + (long long)n * V * ldx + cg * 8;
  T* dxn = dx + (long long)n * V * lddx + cg * 8;
  const int v0 = chunk * vpc;
  const int v1 = v0 + vpc < V ? v0 + vpc : V;
  for (int vb = v0 + vl; vb < v1; vb += UNR * lanes_v) {
    V8<T> a[UNR];
    typename DyCtx<T>::Raw r[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u)
      if (vb + u * lanes_v < v1) {
        a[u].load(xn + (long long)(vb + u * lanes_v) * ldx);
        dc.load(vb + u * lanes_v, r[u]);
      }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (vb + u * lanes_v >= v1) break;
      float dy[8];
      dc.combine(r[u], dy);
      in_bwd_dx8<T, ACT>(a[u], dy, mu, rs, s.slope, ca, cb).store(dxn + (long long)(vb + u * lanes_v) * lddx);
      if constexpr (ZP) {   // whole-row writes (a separate instantiation: the plain one keeps its code)
        if (cg < npad) store_zero8(dxn + (long long)(vb + u * lanes_v) * lddx + C);   // (dxn is at channel 8 cg)
      }
    }
  }
}

// The UnetResBlock tail's backward, first pass (y = lrelu(IN(xa) + IN(xb) | + residual)): g = dy * (y > 0 ? 1 :
// slope), stored (the norms' apply passes and the residual branch read it), and in the same pass the partial sums
// (sum g, sum g xhat) of the InstanceNorm backward of xa and, NX = 2, of xb -- over g as stored, with
// in_bwd_partial's chunks, per-thread voxel order and reduction tree, so the partials and everything after them
// are those of lrelu_bwd_kernel + in_bwd_partial bit for bit, without the separate passes over g.
template <typename T, int NX, bool ZP>
__global__ __launch_bounds__(256) void lrelu_bwd_in_partial(const T* __restrict__ y, int ldy,
                                                            const T* __restrict__ dy, int lddy, T* __restrict__ g,
                                                            int ldg, float slope, const T* __restrict__ xa, int lda,
                                                            const float* __restrict__ ma, const float* __restrict__ ra,
                                                            float* __restrict__ pa, const T* __restrict__ xb, int ldb,
                                                            const float* __restrict__ mb, const float* __restrict__ rb,
                                                            float* __restrict__ pb, int V, int C, int vpc,
                                                            int npad) {
  constexpr int K = 1 + NX;    // sum g, sum g xhat_a (, sum g xhat_b)
  const int n = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x;
  const int C8 = C >> 3, lanes_v = 256 / C8;
  const int tid = threadIdx.x, cg = tid % C8, vl = tid / C8;
  float acc[K][8], mua[8], rsa[8], mub[8], rsb[8];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
  load8f(ma + n * C + cg * 8, mua);
  load8f(ra + n * C + cg * 8, rsa);
  if constexpr (NX > 1) {
    load8f(mb + n * C + cg * 8, mub);
    load8f(rb + n * C + cg * 8, rsb);
  }
  const long long row0 = (long long)n * V;
  const int v0 = chunk * vpc;
  const int v1 = v0 + vpc < V ? v0 + vpc : V;
  if (vl < lanes_v) {
    for (int vb = v0 + vl; vb < v1; vb += UNR * lanes_v) {
      V8<T> vy[UNR], vd[UNR], va[UNR], vx[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u)
        if (vb + u * lanes_v < v1) {
          const long long t = row0 + vb + u * lanes_v;
          vy[u].load(y + t * ldy + cg * 8);
          vd[u].load(dy + t * lddy + cg * 8);
          va[u].load(xa + t * lda + cg * 8);
          if constexpr (NX > 1) vx[u].load(xb + t * ldb + cg * 8);
        }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (vb + u * lanes_v >= v1) break;
        const long long t = row0 + vb + u * lanes_v;
        V8<T> gv;
#pragma unroll
        for (int j = 0; j < 8; ++j) gv.set(j, vy[u].get(j) > 0.f ? vd[u].get(j) : vd[u].get(j) * slope);
        gv.store(g + t * ldg + cg * 8);
        if constexpr (ZP) {
          if (cg < npad) store_zero8(g + t * ldg + C + cg * 8);
        }
        // in_bwd_sums8 with ACT 0 over the stored g, the sum of g shared by both norms
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float gg = gv.get(j);
          acc[0][j] += gg;
          acc[1][j] = fmaf(gg, in_norm(va[u].get(j), mua[j], rsa[j]), acc[1][j]);
          if constexpr (NX > 1) acc[2][j] = fmaf(gg, in_norm(vx[u].get(j), mub[j], rsb[j]), acc[2][j]);
        }
      }
    }
  }
  float* const pout[2] = {pa + ((long long)n * nchunk + chunk) * C * 2,
                          NX > 1 ? pb + ((long long)n * nchunk + chunk) * C * 2 : nullptr};
  block_sum8<K>(acc, C, [&](int c, const float* sum) {
#pragma unroll
    for (int x = 0; x < NX; ++x) {
      pout[x][c * 2] = sum[0];
      pout[x][c * 2 + 1] = sum[1 + x];
    }
  });
}

// ------------------------------------------------- small-volume fused IN
// The 12^3 / 6^3 levels (V <= 4096 voxels per sample): one 256-thread block per (8-channel group, sample)
// holds the whole reduction, so InstanceNorm forward is ONE launch (statistics, then the normalised output
// from a second, L2-resident read) instead of partial + finalize + apply, and the backward likewise.
// Per-thread Welford / sums in fp32; the block merges run in a fixed order: deterministic.
// (The previous 1024-thread form with a 10-level LDS tree and 68 KB of LDS spent most of its time in the tree:
// ~1.7 voxels per thread.)
template <typename T, bool RELU>
__global__ __launch_bounds__(SMALL_T) void in_small_fwd(const T* __restrict__ x, int ldx, T* __restrict__ y, int ldy,
                                                       int V, int C, float eps, float* __restrict__ mean,
                                                       int mean_ld, float* __restrict__ rstd) {
  __shared__ float smu[4][8], sm2[4][8], scnt[4], sfin[16];
  const int cg = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const T* xn = x + (long long)n * V * ldx + cg * 8;
  float mu[8], m2[8], cnt = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) mu[j] = m2[j] = 0.f;
  // through a lambda, as in in_stats_partial: called directly, the compiler contracted other multiply-adds
  auto upd = [&](const V8<T>& a) { welford8_update(cnt, mu, m2, a); };
  int v = tid;
  for (; v + 3 * SMALL_T < V; v += 4 * SMALL_T) {   // 4 loads in flight
    V8<T> a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u].load(xn + (long long)(v + u * SMALL_T) * ldx);
#pragma unroll
    for (int u = 0; u < 4; ++u) upd(a[u]);
  }
  for (; v < V; v += SMALL_T) {
    V8<T> a;
    a.load(xn + (long long)v * ldx);
    upd(a);
  }
  // This block merge stays written out in in_small_fwd and in_small_fwd_r alike: as one shared function the compiler
  // contracted its multiply-adds differently and rstd moved in the last bit.  Lanes merge by a fixed xor-shuffle
  // tree, then the 4 waves in order through LDS.
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    float mb[8], m2b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mb[j] = __shfl_xor(mu[j], o, 64);
      m2b[j] = __shfl_xor(m2[j], o, 64);
    }
    chan_merge(cnt, mu, m2, __shfl_xor(cnt, o, 64), mb, m2b);
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      smu[wave][j] = mu[j];
      sm2[wave][j] = m2[j];
    }
    scnt[wave] = cnt;
  }
  __syncthreads();
  if (tid < 8) {   // channel tid: the 4 waves in order
    float c0 = scnt[0], m0 = smu[0][tid], q0 = sm2[0][tid];
    for (int w = 1; w < 4; ++w) {
      const float nb = scnt[w], nn = c0 + nb;
      if (nb > 0.f) {
        const float dl = smu[w][tid] - m0;
        m0 = m0 + dl * (nb / nn);
        q0 = q0 + sm2[w][tid] + dl * dl * (c0 * nb / nn);
        c0 = nn;
      }
    }
    const float rs = 1.f / sqrtf(q0 / (float)V + eps);
    sfin[tid] = m0;
    sfin[8 + tid] = rs;
    mean[(long long)n * mean_ld + cg * 8 + tid] = m0;
    rstd[n * C + cg * 8 + tid] = rs;
  }
  __syncthreads();
  float m[8], rs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    m[j] = sfin[j];
    rs[j] = sfin[8 + j];
  }
  T* yn = y + (long long)n * V * ldy + cg * 8;
  // 4 (L2-resident) loads in flight per thread before the stores: one latency per 4 voxels
  for (int v0 = tid; v0 < V; v0 += 4 * SMALL_T) {
    V8<T> a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (v0 + u * SMALL_T < V) a[u].load(xn + (long long)(v0 + u * SMALL_T) * ldx);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (v0 + u * SMALL_T >= V) break;
      norm_relu8<T, RELU>(a[u], m, rs);
      a[u].store(yn + (long long)(v0 + u * SMALL_T) * ldy);
    }
  }
}

template <typename T, int ACT>
__global__ __launch_bounds__(SMALL_T) void in_small_bwd(const T* __restrict__ x, int ldx, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, DySrc s, T* __restrict__ dx,
                                                       int lddx, int V, int C, int D, int H, int W) {
  const int cg = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  float mu[8], rs[8], ga[8], gb[8];
  load8f(mean + n * C + cg * 8, mu);
  load8f(rstd + n * C + cg * 8, rs);
#pragma unroll
  for (int j = 0; j < 8; ++j) ga[j] = gb[j] = 0.f;
  const DyCtx<T> dc(s, n, V, cg, C, D, H, W);
  const T* xn = x + (long long)n * V * ldx + cg * 8;
  // 4 voxels' loads in flight per thread, consumed in voxel order (the sums' order is unchanged)
  for (int v0 = tid; v0 < V; v0 += 4 * SMALL_T) {
    V8<T> a[4];
    typename DyCtx<T>::Raw r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (v0 + u * SMALL_T < V) {
        a[u].load(xn + (long long)(v0 + u * SMALL_T) * ldx);
        dc.load(v0 + u * SMALL_T, r[u]);
      }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (v0 + u * SMALL_T >= V) break;
      float dy[8];
      dc.combine(r[u], dy);
      in_bwd_sums8<T, ACT>(a[u], dy, mu, rs, s.slope, ga, gb);
    }
  }
  float ca[8], cb[8];
  small_block_coef(ga, gb, V, ca, cb);
  T* dxn = dx + (long long)n * V * lddx + cg * 8;
  for (int v0 = tid; v0 < V; v0 += 4 * SMALL_T) {
    V8<T> a[4];
    typename DyCtx<T>::Raw r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (v0 + u * SMALL_T < V) {
        a[u].load(xn + (long long)(v0 + u * SMALL_T) * ldx);
        dc.load(v0 + u * SMALL_T, r[u]);
      }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (v0 + u * SMALL_T >= V) break;
      float dy[8];
      dc.combine(r[u], dy);
      in_bwd_dx8<T, ACT>(a[u], dy, mu, rs, s.slope, ca, cb).store(dxn + (long long)(v0 + u * SMALL_T) * lddx);
    }
  }
}

// Register-resident forms for V <= VPT * 256 (the 12^3 and 6^3 levels): every voxel of the thread is loaded
// once, up front (one memory latency instead of one per pass and per 4 voxels), kept in registers through the
// statistics and applied from there.  The per-thread accumulation order (voxels tid, tid + 256, ...) and the
// block merges are those of in_small_fwd / in_small_bwd, so the results are bitwise the same.
template <typename T, bool RELU, int VPT>
__global__ __launch_bounds__(SMALL_T) void in_small_fwd_r(const T* __restrict__ x, int ldx, T* __restrict__ y,
                                                         int ldy, int V, int C, float eps, float* __restrict__ mean,
                                                         int mean_ld, float* __restrict__ rstd) {
  __shared__ float smu[4][8], sm2[4][8], scnt[4], sfin[16];
  const int cg = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const T* xn = x + (long long)n * V * ldx + cg * 8;
  V8<T> a[VPT];
#pragma unroll
  for (int u = 0; u < VPT; ++u)
    if (tid + u * SMALL_T < V) a[u].load(xn + (long long)(tid + u * SMALL_T) * ldx);
  float mu[8], m2[8], cnt = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) mu[j] = m2[j] = 0.f;
#pragma unroll
  for (int u = 0; u < VPT; ++u) {
    if (tid + u * SMALL_T >= V) break;
    welford8_update(cnt, mu, m2, a[u]);
  }
  // This block merge stays written out in in_small_fwd and in_small_fwd_r alike: as one shared function the compiler
  // contracted its multiply-adds differently and rstd moved in the last bit.  Lanes merge by a fixed xor-shuffle
  // tree, then the 4 waves in order through LDS.
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    float mb[8], m2b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mb[j] = __shfl_xor(mu[j], o, 64);
      m2b[j] = __shfl_xor(m2[j], o, 64);
    }
    chan_merge(cnt, mu, m2, __shfl_xor(cnt, o, 64), mb, m2b);
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      smu[wave][j] = mu[j];
      sm2[wave][j] = m2[j];
    }
    scnt[wave] = cnt;
  }
  __syncthreads();
  if (tid < 8) {   // channel tid: the 4 waves in order
    float c0 = scnt[0], m0 = smu[0][tid], q0 = sm2[0][tid];
    for (int w = 1; w < 4; ++w) {
      const float nb = scnt[w], nn = c0 + nb;
      if (nb > 0.f) {
        const float dl = smu[w][tid] - m0;
        m0 = m0 + dl * (nb / nn);
        q0 = q0 + sm2[w][tid] + dl * dl * (c0 * nb / nn);
        c0 = nn;
      }
    }
    const float rs = 1.f / sqrtf(q0 / (float)V + eps);
    sfin[tid] = m0;
    sfin[8 + tid] = rs;
    mean[(long long)n * mean_ld + cg * 8 + tid] = m0;
    rstd[n * C + cg * 8 + tid] = rs;
  }
  __syncthreads();
  float m[8], rs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    m[j] = sfin[j];
    rs[j] = sfin[8 + j];
  }
  T* yn = y + (long long)n * V * ldy + cg * 8;
#pragma unroll
  for (int u = 0; u < VPT; ++u) {
    if (tid + u * SMALL_T >= V) break;
    norm_relu8<T, RELU>(a[u], m, rs);
    a[u].store(yn + (long long)(tid + u * SMALL_T) * ldy);
  }
}

template <typename T, int ACT, int VPT>
__global__ __launch_bounds__(SMALL_T) void in_small_bwd_r(const T* __restrict__ x, int ldx,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         DySrc s, T* __restrict__ dx, int lddx, int V, int C, int D,
                                                         int H, int W) {
  const int cg = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const DyCtx<T> dc(s, n, V, cg, C, D, H, W);
  const T* xn = x + (long long)n * V * ldx + cg * 8;
  V8<T> a[VPT];
  float dy[VPT][8];
  {
    typename DyCtx<T>::Raw r[VPT];
#pragma unroll
    for (int u = 0; u < VPT; ++u)
      if (tid + u * SMALL_T < V) {
        a[u].load(xn + (long long)(tid + u * SMALL_T) * ldx);
        dc.load(tid + u * SMALL_T, r[u]);
      }
#pragma unroll
    for (int u = 0; u < VPT; ++u)
      if (tid + u * SMALL_T < V) dc.combine(r[u], dy[u]);
  }
  float mu[8], rs[8], ga[8], gb[8];
  load8f(mean + n * C + cg * 8, mu);
  load8f(rstd + n * C + cg * 8, rs);
#pragma unroll
  for (int j = 0; j < 8; ++j) ga[j] = gb[j] = 0.f;
#pragma unroll
  for (int u = 0; u < VPT; ++u) {
    if (tid + u * SMALL_T >= V) break;
    in_bwd_sums8<T, ACT>(a[u], dy[u], mu, rs, s.slope, ga, gb);
  }
  float ca[8], cb[8];
  small_block_coef(ga, gb, V, ca, cb);
  T* dxn = dx + (long long)n * V * lddx + cg * 8;
#pragma unroll
  for (int u = 0; u < VPT; ++u) {
    if (tid + u * SMALL_T >= V) break;
    in_bwd_dx8<T, ACT>(a[u], dy[u], mu, rs, s.slope, ca, cb).store(dxn + (long long)(tid + u * SMALL_T) * lddx);
  }
}

// ---------------------------------------------------------------- planners
int knob_small_v() {   // read per call (A/B runs and tests flip it in-process)
  const char* e = getenv("MMSEG_IN_SMALL_V");
  return e ? atoi(e) : 4096;
}

// at least 256 chunks per sample (down to 2 voxels per thread): the 48^3 / 24^3 levels otherwise ran 108..432
// blocks of 16 voxels per thread, latency-bound (128 / 512 measured within noise, r03u)
int knob_in_minch() { return 256; }

int chunks_for(long long V, int C, long long* vpc) {
  // reduction passes: ~16 voxels per thread (lanes_v = 256 / C8 voxel lanes), at most 1024 chunks
  const int lanes_v = 256 / (C >> 3);
  long long want = (long long)lanes_v * 16;
  long long nch = (V + want - 1) / want;
  const long long minch = std::min<long long>(knob_in_minch(), V / (2LL * lanes_v));
  if (nch < minch) nch = minch;
  if (nch > 1024) nch = 1024;
  if (nch < 1) nch = 1;
  *vpc = (V + nch - 1) / nch;
  return (int)((V + *vpc - 1) / *vpc);
}

int apply_chunks(long long V, int C, int* vpc) {
  // elementwise passes: 2 x UNR voxels per thread
  const int lanes_v = 256 / (C >> 3);
  long long want = (long long)lanes_v * 2 * UNR;
  long long nch = (V + want - 1) / want;
  const long long minch = std::min<long long>(knob_in_minch(), V / lanes_v);
  if (nch < minch) nch = minch;
  if (nch < 1) nch = 1;
  *vpc = (int)((V + nch - 1) / nch);
  return (int)((V + *vpc - 1) / *vpc);
}

// ---------------------------------------------------------------- backward
// One InstanceNorm backward as its entry points state it (host only: the kernels take DySrc).
struct InBwdArgs {
  const void* x;
  int ldx;
  const float* mean;
  const float* rstd;
  DySrc src;      // the dy sources, p1_nmod and slope (gsplit: set by the impl)
  void* dx;
  int lddx;
  int N, D, H, W, C;
  int act;        // 0 none, 1 ReLU, 2 LeakyReLU(src.slope)
  float* ws;
  int dtype;
  void* stream;
  const float* part_in = nullptr;   // partial sums a producer of dy emitted [N][nchunk_in][C][2], or null
  int nchunk_in = 0;
  int Cw = 0;     // dx's channels [C, Cw) are written as zeros on the partial / apply path; 0: C
};

int instnorm_bwd_impl(const InBwdArgs& a) {
  const int N = a.N, D = a.D, H = a.H, W = a.W, C = a.C;
  MMSEG_REQUIRE(a.act >= 0 && a.act <= 2, "instnorm_bwd: activation %d (0 none, 1 ReLU, 2 LeakyReLU)", a.act);
  const int Cw = a.Cw ? a.Cw : C;
  MMSEG_REQUIRE(Cw % 8 == 0 && Cw >= C && Cw <= 2 * C && Cw <= a.lddx,
                "instnorm_bwd: write extent Cw=%d outside [C, min(2 C, lddx)] or not a multiple of 8", Cw);
  const int npad = (Cw - C) / 8;
  MMSEG_REQUIRE(C % 8 == 0 && C <= 2048, "instnorm_bwd: C=%d must be a multiple of 8 and <= 2048", C);
  MMSEG_REQUIRE(!a.part_in || a.nchunk_in > 0, "instnorm_bwd: given partials need their chunk count");
  MMSEG_REQUIRE(!a.src.pool_dy || ((D | H | W) & 1) == 0, "instnorm_bwd: pooled gather needs even dims");
  const long long V = (long long)D * H * W;
  MMSEG_REQUIRE(V * std::max(a.ldx, a.lddx) < (1LL << 31) && V * std::max(a.src.ld1, a.src.pool_ld) < (1LL << 31),
                "instnorm_bwd: per-sample extent must fit int32");
  long long vpc;
  const int nch = chunks_for(V, C, &vpc);
  int avpc;
  const int anch = apply_chunks(V, C, &avpc);
  DySrc src = a.src;
  hipStream_t s = (hipStream_t)a.stream;
  float* part = a.ws;
  float* coef = a.part_in ? a.ws : a.ws + (long long)N * nch * C * 2;
  dim3 grid(nch, N), agrid(anch, N);
  if (src.p1_nmod > 0 && N / src.p1_nmod > 1) {   // modality groups sharing a p1 sample: chunk-major grids (DySrc::gsplit)
    src.gsplit = N / src.p1_nmod;
    grid = dim3(nch * src.gsplit, src.p1_nmod);
    agrid = dim3(anch * src.gsplit, src.p1_nmod);
  }
  const bool small = V <= knob_small_v() && !a.part_in;
  auto run = [&](auto tag, auto act_c) {
    using T = decltype(tag);
    constexpr int R = decltype(act_c)::value;
    const T* x = (const T*)a.x;
    T* dx = (T*)a.dx;
    auto launch_in_bwd_apply = [&] {
      if (npad)
        MMSEG_LAUNCH((in_bwd_apply<T, R, true>), agrid, dim3(256), 0, s, x, a.ldx, a.mean, a.rstd, src, coef, dx,
                     a.lddx, (int)V, C, D, H, W, avpc, npad);
      else
        MMSEG_LAUNCH((in_bwd_apply<T, R>), agrid, dim3(256), 0, s, x, a.ldx, a.mean, a.rstd, src, coef, dx, a.lddx,
                     (int)V, C, D, H, W, avpc, 0);
    };
    if (a.part_in) {
      MMSEG_LAUNCH(in_bwd_finalize, dim3(N * C), dim3(256), 0, s, a.part_in, N, C, a.nchunk_in, V, coef);
      launch_in_bwd_apply();
    } else if (small) {
      const dim3 sgrid(C / 8, N);
      if (V <= SMALL_T)
        MMSEG_LAUNCH((in_small_bwd_r<T, R, 1>), sgrid, dim3(SMALL_T), 0, s, x, a.ldx, a.mean, a.rstd, src, dx, a.lddx,
                     (int)V, C, D, H, W);
      else if (V <= 8 * SMALL_T)
        MMSEG_LAUNCH((in_small_bwd_r<T, R, 8>), sgrid, dim3(SMALL_T), 0, s, x, a.ldx, a.mean, a.rstd, src, dx, a.lddx,
                     (int)V, C, D, H, W);
      else
        MMSEG_LAUNCH((in_small_bwd<T, R>), sgrid, dim3(SMALL_T), 0, s, x, a.ldx, a.mean, a.rstd, src, dx, a.lddx,
                     (int)V, C, D, H, W);
    } else {
      MMSEG_LAUNCH((in_bwd_partial<T, R>), grid, dim3(256), 0, s, x, a.ldx, a.mean, a.rstd, src, (int)V, C, D, H, W,
                   (int)vpc, part);
      MMSEG_LAUNCH(in_bwd_finalize, dim3(N * C), dim3(256), 0, s, part, N, C, nch, V, coef);
      launch_in_bwd_apply();
    }
  };
  by_dtype(a.dtype, [&](auto tag) {
    if (a.act == 2) run(tag, std::integral_constant<int, 2>{});
    else if (a.act == 1) run(tag, std::integral_constant<int, 1>{});
    else run(tag, std::integral_constant<int, 0>{});
  });
  return mmseg::check_launch("instnorm_relu_bwd");
}

}  // namespace

extern "C" {

// Workspace (floats) the stats / bwd-reduce kernels need for N samples.
long long mmseg_instnorm_ws_floats(int N, long long V, int C) {
  long long vpc;
  int nch = chunks_for(V, C, &vpc);
  return (long long)N * nch * C * 2 + (long long)N * C * 2;
}

// mean[n*mean_ld + c], rstd[n*C + c] (rstd may be null: channel means only)
int mmseg_instnorm_stats(const void* x, int ldx, int N, long long V, int C, float eps, float* mean, int mean_ld,
                         float* rstd, float* ws, int dtype, void* stream) {
  MMSEG_REQUIRE(C % 8 == 0 && C <= 2048, "instnorm: C=%d must be a multiple of 8", C);
  MMSEG_REQUIRE(V * ldx < (1LL << 31), "instnorm: per-sample extent must fit int32");
  long long vpc;
  const int nch = chunks_for(V, C, &vpc);
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    MMSEG_LAUNCH(in_stats_partial<T>, dim3(nch, N), dim3(256), 0, s, (const T*)x, ldx, (int)V, C, (int)vpc, ws);
    MMSEG_LAUNCH(in_stats_finalize<T>, dim3(N * C), dim3(256), 0, s, (const T*)x, ldx, V, N, C, nch, vpc, ws, eps,
                 mean, mean_ld, rstd);
  });
  return mmseg::check_launch("instnorm_stats");
}

int mmseg_instnorm_apply(const void* x, int ldx, void* y, int ldy, int N, long long V, int C, const float* mean,
                         const float* rstd, int relu, int dtype, void* stream) {
  MMSEG_REQUIRE(C % 8 == 0 && C <= 2048, "instnorm_apply: C=%d must be a multiple of 8", C);
  MMSEG_REQUIRE(V * (ldx > ldy ? ldx : ldy) < (1LL << 31), "instnorm_apply: per-sample extent must fit int32");
  hipStream_t s = (hipStream_t)stream;
  int vpc;
  const dim3 grid(apply_chunks(V, C, &vpc), N);
  auto run = [&](auto tag, auto relu_c) {
    using T = decltype(tag);
    constexpr bool R = decltype(relu_c)::value;
    MMSEG_LAUNCH((in_relu_apply<T, R>), grid, dim3(256), 0, s, (const T*)x, ldx, (T*)y, ldy, (int)V, C, vpc, mean,
                 rstd);
  };
  by_dtype(dtype, [&](auto tag) {
    if (relu) run(tag, std::true_type{});
    else run(tag, std::false_type{});
  });
  return mmseg::check_launch("instnorm_apply");
}

int mmseg_instnorm_relu_fwd(const void* x, int ldx, void* y, int ldy, int N, long long V, int C, const float* mean,
                            const float* rstd, int dtype, void* stream) {
  return mmseg_instnorm_apply(x, ldx, y, ldy, N, V, C, mean, rstd, 1, dtype, stream);
}

int mmseg_instnorm_fwd(const void* x, int ldx, void* y, int ldy, int N, long long V, int C, float eps, float* mean,
                       int mean_ld, float* rstd, int relu, float* ws, int dtype, void* stream) {
  MMSEG_REQUIRE(C % 8 == 0 && C <= 2048, "instnorm_fwd: C=%d must be a multiple of 8", C);
  if (V > knob_small_v()) {
    if (mmseg_instnorm_stats(x, ldx, N, V, C, eps, mean, mean_ld, rstd, ws, dtype, stream)) return 1;
    MMSEG_REQUIRE(mean_ld == C, "instnorm_fwd: the apply pass reads mean with ld = C");
    return mmseg_instnorm_apply(x, ldx, y, ldy, N, V, C, mean, rstd, relu, dtype, stream);
  }
  MMSEG_REQUIRE(V * (ldx > ldy ? ldx : ldy) < (1LL << 31), "instnorm_fwd: per-sample extent must fit int32");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(C / 8, N);
  auto run = [&](auto tag, auto relu_c) {
    using T = decltype(tag);
    constexpr bool R = decltype(relu_c)::value;
    if (V <= SMALL_T)
      MMSEG_LAUNCH((in_small_fwd_r<T, R, 1>), grid, dim3(SMALL_T), 0, s, (const T*)x, ldx, (T*)y, ldy, (int)V, C,
                         eps, mean, mean_ld, rstd);
    else if (V <= 8 * SMALL_T)
      MMSEG_LAUNCH((in_small_fwd_r<T, R, 8>), grid, dim3(SMALL_T), 0, s, (const T*)x, ldx, (T*)y, ldy, (int)V, C,
                         eps, mean, mean_ld, rstd);
    else
      MMSEG_LAUNCH((in_small_fwd<T, R>), grid, dim3(SMALL_T), 0, s, (const T*)x, ldx, (T*)y, ldy, (int)V, C, eps,
                         mean, mean_ld, rstd);
  };
  by_dtype(dtype, [&](auto tag) {
    if (relu) run(tag, std::true_type{});
    else run(tag, std::false_type{});
  });
  return mmseg::check_launch("instnorm_fwd");
}

// mmseg_instnorm_bwd whose partial sums (g, g * xhat per chunk, [N][nchunk_in][C][2]) a producer of dy already
// emitted (the fused head + loss backward, mmseg_head_loss_bwd_in): the partial pass is skipped.
// dy sources: see DySrc.  Any of p1 / beta / pool_dy may be null.
int mmseg_instnorm_bwd_part(const void* x, int ldx, const float* mean, const float* rstd, const void* p1, int ld1,
                            float scale1, const float* alpha1, int alpha_stride, const float* beta, int beta_stride,
                            const void* pool_dy, int pool_ld, const uint8_t* pool_idx, void* dx, int lddx, int N,
                            int D, int H, int W, int C, int relu, const float* part_in, int nchunk_in, float* ws,
                            int dtype, void* stream) {
  InBwdArgs a{x, ldx, mean, rstd, DySrc{p1, ld1, scale1, alpha1, alpha_stride, beta, beta_stride, pool_dy, pool_ld,
                                        pool_idx},
              dx, lddx, N, D, H, W, C, relu, ws, dtype, stream};
  a.part_in = part_in;
  a.nchunk_in = nchunk_in;
  return instnorm_bwd_impl(a);
}

int mmseg_instnorm_bwd(const void* x, int ldx, const float* mean, const float* rstd, const void* p1, int ld1,
                            float scale1, const float* alpha1, int alpha_stride, const float* beta, int beta_stride,
                            const void* pool_dy, int pool_ld, const uint8_t* pool_idx, void* dx, int lddx, int N,
                            int D, int H, int W, int C, int relu, float* ws, int dtype, void* stream) {
  return mmseg_instnorm_bwd_part(x, ldx, mean, rstd, p1, ld1, scale1, alpha1, alpha_stride, beta, beta_stride, pool_dy,
                                 pool_ld, pool_idx, dx, lddx, N, D, H, W, C, relu, nullptr, 0, ws, dtype, stream);
}

int mmseg_instnorm_relu_bwd(const void* x, int ldx, const float* mean, const float* rstd, const void* p1, int ld1,
                            float scale1, const float* alpha1, int alpha_stride, const float* beta, int beta_stride,
                            const void* pool_dy, int pool_ld, const uint8_t* pool_idx, void* dx, int lddx, int N,
                            int D, int H, int W, int C, float* ws, int dtype, void* stream) {
  return mmseg_instnorm_bwd(x, ldx, mean, rstd, p1, ld1, scale1, alpha1, alpha_stride, beta, beta_stride, pool_dy,
                            pool_ld, pool_idx, dx, lddx, N, D, H, W, C, 1, ws, dtype, stream);
}

// The InstanceNorm + ReLU backward of G modality encoders' level outputs at once (N = G x n samples of one
// combined pre-norm tensor / statistics / pooled gradient): every sample reads the fused level's gradient p1 of
// its own sample index modulo p1_nmod = n -- once per fused sample for all G modalities (reference
// dual_encoder.py:193-195 mean / 184-186 add fusion backward, unet.py:34-35 InstanceNorm + ReLU).
int mmseg_instnorm_relu_bwd_group(const void* x, int ldx, const float* mean, const float* rstd, const void* p1,
                                  int ld1, float scale1, int p1_nmod, const void* pool_dy, int pool_ld,
                                  const uint8_t* pool_idx, void* dx, int lddx, int N, int D, int H, int W, int C,
                                  float* ws, int dtype, void* stream) {
  MMSEG_REQUIRE(p1_nmod >= 1 && N % p1_nmod == 0, "instnorm_relu_bwd_group: N=%d must be a multiple of p1_nmod=%d",
                N, p1_nmod);
  return instnorm_bwd_impl({x, ldx, mean, rstd, DySrc{p1, ld1, scale1, nullptr, 0, nullptr, 0, pool_dy, pool_ld,
                                                       pool_idx, p1_nmod},
                            dx, lddx, N, D, H, W, C, 1, ws, dtype, stream});
}

// The InstanceNorm backward (no affine) with the activation after the norm folded in (act 0 none, 1 ReLU, 2
// LeakyReLU(slope); g: the gradient of the activation's OUTPUT), dy = g: SwinUNETR's UnetResBlock norms (MONAI
// get_norm_layer("instance") + LeakyReLU(0.01) for conv1's, none for conv2 / conv3's, whose LeakyReLU follows the
// residual sum -- mmseg_lrelu_bwd_in_part).  part / nchunk: partial sums a producer of g emitted (finalize + apply
// only), or null.  Cw: dx's channels [C, Cw) are written as zeros (whole-row writes at pitch lddx > C) on the
// partial / apply path (V > the small-volume bound).
int mmseg_instnorm_act_bwd(const void* x, int ldx, const float* mean, const float* rstd, const void* g, int ldg,
                           void* dx, int lddx, int N, int D, int H, int W, int C, int Cw, int act, float slope,
                           const float* part, int nchunk, float* ws, int dtype, void* stream) {
  InBwdArgs a{x, ldx, mean, rstd, DySrc{g, ldg, 1.f, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, slope},
              dx, lddx, N, D, H, W, C, act, ws, dtype, stream};
  a.part_in = part;
  a.nchunk_in = nchunk;
  a.Cw = Cw;
  return instnorm_bwd_impl(a);
}

int mmseg_instnorm_part_chunks(long long V, int C) {
  long long vpc;
  return (C % 8 == 0 && C <= 2048 && V > 0) ? chunks_for(V, C, &vpc) : 0;
}

int mmseg_lrelu_bwd_in_part(const void* y, int ldy, const void* dy, int lddy, void* g, int ldg, float slope,
                            const void* xa, int lda, const float* ma, const float* ra, float* pa, const void* xb,
                            int ldb, const float* mb, const float* rb, float* pb, int N, long long V, int C, int Cw,
                            int dtype, void* stream) {
  MMSEG_REQUIRE(C % 8 == 0 && C <= 2048 && V > 0, "lrelu_bwd_in_part: C=%d must be a multiple of 8", C);
  MMSEG_REQUIRE(Cw % 8 == 0 && Cw >= C && Cw <= 2 * C && Cw <= ldg, "lrelu_bwd_in_part: C <= Cw <= min(2 C, ldg)");
  const int npad = (Cw - C) / 8;
  MMSEG_REQUIRE(y && dy && g && xa && ma && ra && pa, "lrelu_bwd_in_part: null operand");
  MMSEG_REQUIRE(!xb || (mb && rb && pb), "lrelu_bwd_in_part: xb needs its statistics and partial buffer");
  const int ldmax = std::max(std::max(ldy, lddy), std::max(std::max(ldg, lda), xb ? ldb : 0));
  MMSEG_REQUIRE(V * ldmax < (1LL << 31), "lrelu_bwd_in_part: per-sample extent must fit int32");
  MMSEG_REQUIRE(ldy % 8 == 0 && lddy % 8 == 0 && ldg % 8 == 0 && lda % 8 == 0 && (!xb || ldb % 8 == 0),
                "lrelu_bwd_in_part: pitches must be multiples of 8");
  long long vpc;
  const int nch = chunks_for(V, C, &vpc);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(nch, N);
  auto run = [&](auto tag, auto zp) {
    using T = decltype(tag);
    constexpr bool Z = decltype(zp)::value;
    if (xb)
      MMSEG_LAUNCH((lrelu_bwd_in_partial<T, 2, Z>), grid, dim3(256), 0, s, (const T*)y, ldy, (const T*)dy, lddy, (T*)g,
                   ldg, slope, (const T*)xa, lda, ma, ra, pa, (const T*)xb, ldb, mb, rb, pb, (int)V, C, (int)vpc,
                   npad);
    else
      MMSEG_LAUNCH((lrelu_bwd_in_partial<T, 1, Z>), grid, dim3(256), 0, s, (const T*)y, ldy, (const T*)dy, lddy, (T*)g,
                   ldg, slope, (const T*)xa, lda, ma, ra, pa, (const T*)nullptr, 0, nullptr, nullptr, nullptr, (int)V,
                   C, (int)vpc, npad);
  };
  by_dtype(dtype, [&](auto tag) {
    if (npad) run(tag, std::true_type{});
    else run(tag, std::false_type{});
  });
  return mmseg::check_launch("lrelu_bwd_in_part");
}

// The first half of mmseg_instnorm_bwd for dy = p1 (scale 1): the finalised coefficients coef [N][C][2] =
// (mean g, mean g xhat), from the partials a producer of dy emitted (part_in, nchunk_in) or from the partial pass
// (part_in null; ws: mmseg_instnorm_ws_floats).  The apply half then runs inside the norm's only consumer
// (mmseg_stem_wgrad_inb), which never writes the input gradient.
int mmseg_instnorm_bwd_coef(const void* x, int ldx, const float* mean, const float* rstd, const void* p1, int ld1,
                            int N, int D, int H, int W, int C, int relu, const float* part_in, int nchunk_in,
                            float* coef, float* ws, int dtype, void* stream) {
  MMSEG_REQUIRE(C % 8 == 0 && C <= 2048 && p1 && coef, "instnorm_bwd_coef: C=%d must be a multiple of 8", C);
  const long long V = (long long)D * H * W;
  MMSEG_REQUIRE(V * (ldx > ld1 ? ldx : ld1) < (1LL << 31), "instnorm_bwd_coef: per-sample extent must fit int32");
  hipStream_t s = (hipStream_t)stream;
  if (!part_in) {
    long long vpc;
    const int nch = chunks_for(V, C, &vpc);
    DySrc src{p1, ld1, 1.f, nullptr, 0, nullptr, 0, nullptr, 0, nullptr};
    const dim3 grid(nch, N);
    auto run = [&](auto tag, auto act_c) {
      using T = decltype(tag);
      constexpr int R = decltype(act_c)::value;
      MMSEG_LAUNCH((in_bwd_partial<T, R>), grid, dim3(256), 0, s, (const T*)x, ldx, mean, rstd, src, (int)V, C,
                         D, H, W, (int)vpc, ws);
    };
    by_dtype(dtype, [&](auto tag) {
      if (relu) run(tag, std::integral_constant<int, 1>{});
      else run(tag, std::integral_constant<int, 0>{});
    });
    part_in = ws;
    nchunk_in = nch;
  }
  MMSEG_LAUNCH(in_bwd_finalize, dim3(N * C), dim3(256), 0, s, part_in, N, C, nchunk_in, V, coef);
  return mmseg::check_launch("instnorm_bwd_coef");
}

}  // extern "C"
