// The per-element expressions of InstanceNorm (no affine), one definition each: the InstanceNorm kernels
// (instnorm.hip) and every kernel that applies a deferred norm to its input (pool_fuse.hip, the conv kernels through
// conv_common.h) use these, so a consumer of a deferred norm sees in_relu_apply's bits by construction.
#pragma once
#include "mmseg_common.h"

__device__ __forceinline__ void load8f(const float* p, float* d) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
  d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
}

// xhat, the normalised value
__device__ __forceinline__ float in_norm(float x, float mu, float rs) { return (x - mu) * rs; }

// The norm of 8 channels in place: (v - mu) * rs, through the ReLU (RELU), rounded to T -- in_relu_apply's output.
template <typename T, bool RELU = true>
__device__ __forceinline__ void norm_relu8(V8<T>& v, const float* mu, const float* rs) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float h = in_norm(v.get(j), mu[j], rs[j]);
    v.set(j, (!RELU || h > 0.f) ? h : 0.f);
  }
}

// One voxel into a thread's Welford state (count, mean, M2) of 8 channels.
template <typename T>
__device__ __forceinline__ void welford8_update(float& cnt, float* mu, float* m2, const V8<T>& a) {
  cnt += 1.f;
  const float inv = 1.f / cnt;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float xv = a.get(j), d = xv - mu[j];
    mu[j] = fmaf(d, inv, mu[j]);
    m2[j] = fmaf(d, xv - mu[j], m2[j]);
  }
}

// gradient through the activation that follows the norm (h: the normalised value; an activation keeps the sign,
// so h > 0 is where its output is > 0): ACT 0 none, 1 ReLU, 2 LeakyReLU
template <int ACT>
__device__ __forceinline__ float act_grad(float h, float dy, float slope) {
  if constexpr (ACT == 0) return dy;
  else if constexpr (ACT == 1) return h > 0.f ? dy : 0.f;
  else return h > 0.f ? dy : dy * slope;
}

// The backward's two passes over one voxel's 8 channels, g = act'(xhat) dy: the sums (g, g xhat) ...
template <typename T, int ACT>
__device__ __forceinline__ void in_bwd_sums8(const V8<T>& x, const float* dy, const float* mu, const float* rs,
                                             float slope, float* sg, float* sgx) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float h = in_norm(x.get(j), mu[j], rs[j]);
    const float g = act_grad<ACT>(h, dy[j], slope);
    sg[j] += g;
    sgx[j] = fmaf(g, h, sgx[j]);
  }
}
// ... and dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), rounded to T
template <typename T, int ACT>
__device__ __forceinline__ V8<T> in_bwd_dx8(const V8<T>& x, const float* dy, const float* mu, const float* rs,
                                            float slope, const float* ca, const float* cb) {
  V8<T> o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float h = in_norm(x.get(j), mu[j], rs[j]);
    const float g = act_grad<ACT>(h, dy[j], slope);
    o.set(j, rs[j] * (g - ca[j] - h * cb[j]));
  }
  return o;
}
