// The gathered gradient of an InstanceNorm + ReLU output (DySrc / DyCtx), shared by the norm backward kernels
// (instnorm.hip) and the Grad-CAM channel weights (explain.hip): one gather, one set of bits.
#pragma once
#include "mmseg_common.h"

// ------------------------------------------------------------- dy gather
// dy(n, v, c) = scale1 * alpha1[n] * p1[n,v,c] + beta[n,c]
//             + (pool_idx[n, pool(v), c] == sub(v) ? pool_dy[n, pool(v), c] : 0)
struct DySrc {
  const void* p1;
  int ld1;
  float scale1;
  const float* alpha1;   // [N] (stride alpha_stride) or null
  int alpha_stride;
  const float* beta;     // [N][C] (stride beta_stride per n) or null
  int beta_stride;
  const void* pool_dy;   // [N][Vo][C] with ld pool_ld, or null
  int pool_ld;
  const uint8_t* pool_idx;  // [N][Vo][C]
  int p1_nmod;           // > 0: p1 holds p1_nmod samples, sample n reads p1 sample n % p1_nmod (the fused level's
                         // gradient shared by the M modality groups of a grouped backward)
  float slope;           // ACT 2: the LeakyReLU's negative slope
  // > 1 (with p1_nmod): the partial / apply grids are (chunks x gsplit, p1_nmod) -- the gsplit modality samples
  // that read one p1 sample take adjacent blocks of each chunk, so the second read of that p1 chunk is served by
  // the Infinity Cache instead of HBM (launched sample-major, the re-read came ~2 samples = 240 MB later)
  int gsplit;
};

// Per-thread view of a DySrc for one sample and one 8-channel group: the
// scale, beta and base pointers are resolved once, the per-voxel work is the
// loads and the pool-window test.
template <typename T>
struct DyCtx {
  const T* p1;
  int ld1;
  float sc;
  float beta[8];
  bool has_beta;
  const T* pdy;
  int pool_ld;
  const uint8_t* pidx;
  int C, H, W, Ho, Wo, HWo;

  __device__ __forceinline__ DyCtx(const DySrc& s, int n, int V, int cg, int C_, int D, int H_, int W_) {
    C = C_;
    H = H_;
    W = W_;
    const int n1 = s.p1_nmod > 0 ? n % s.p1_nmod : n;
    p1 = s.p1 ? reinterpret_cast<const T*>(s.p1) + (long long)n1 * V * s.ld1 + cg * 8 : nullptr;
    ld1 = s.ld1;
    sc = s.scale1 * (s.alpha1 ? s.alpha1[n * s.alpha_stride] : 1.f);
    has_beta = s.beta != nullptr;
#pragma unroll
    for (int j = 0; j < 8; ++j) beta[j] = has_beta ? s.beta[n * s.beta_stride + cg * 8 + j] : 0.f;
    Ho = H >> 1;
    Wo = W >> 1;
    HWo = Ho * Wo;
    const long long Vo = (long long)(D >> 1) * HWo;
    pdy = s.pool_dy ? reinterpret_cast<const T*>(s.pool_dy) + (long long)n * Vo * s.pool_ld + cg * 8 : nullptr;
    pool_ld = s.pool_ld;
    pidx = s.pool_dy ? s.pool_idx + (long long)n * Vo * C + cg * 8 : nullptr;
  }

  // raw loads for voxel v (issued early), then combine
  struct Raw {
    V8<T> a, pd;
    uint2 id;
    uint8_t sub;
  };
  __device__ __forceinline__ void load(int v, Raw& r) const {
    if (p1) r.a.load(p1 + (long long)v * ld1);
    if (pdy) {
      const int x = v % W;
      const int q = v / W;
      const int y = q % H, z = q / H;
      const int vo = (z >> 1) * HWo + (y >> 1) * Wo + (x >> 1);
      r.sub = (uint8_t)(((z & 1) << 2) | ((y & 1) << 1) | (x & 1));
      r.pd.load(pdy + (long long)vo * pool_ld);
      r.id = *reinterpret_cast<const uint2*>(pidx + (long long)vo * C);
    }
  }
  __device__ __forceinline__ void combine(const Raw& r, float* dy) const {
#pragma unroll
    for (int j = 0; j < 8; ++j) dy[j] = (p1 ? r.a.get(j) * sc : 0.f) + beta[j];
    if (pdy) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t w = j < 4 ? r.id.x : r.id.y;
        const uint8_t id = (uint8_t)((w >> ((j & 3) * 8)) & 0xff);
        if (id == r.sub) dy[j] += r.pd.get(j);
      }
    }
  }
};
