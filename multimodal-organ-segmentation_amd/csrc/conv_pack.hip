// Weight packing: fp32 torch-layout weights into the MFMA B-operand images the conv kernels read, one layer or a
// whole table per launch, the fused AdamW + pack step, and the e4m3 image of the fp8 forward.
#include "mmseg_common.h"

namespace {

// ------------------------------------------------------------ weight pack
// dst[kgi][col][j] (T), KGp x Cpad x 8, from fp32 torch-layout weights.
//   0 CONV3_FWD  : W[Co][Ci][27]; kgi = tap*(Cip/8)+c8, col = co, ci = c8*8+j
//   1 CONV3_DGRAD: kgi = tap*(Co/8)+c8, col = ci, co = c8*8+j, tap' = 26-tap
//   2 POINT_FWD  : W[Co][Ci]; kgi = c8, col = co, ci = c8*8+j
//   3 POINT_DGRAD: kgi = c8, col = ci, co = c8*8+j
//   4 CONVT_FWD  : W[Ci][Co][8]; kgi = c8 (ci), col = tap*Co + co
//   5 CONVT_DGRAD: kgi = tap*(Co/8)+c8, col = ci, co = c8*8+j
//   6 / 7        : modes 1 / 5 with Cip = the padded output-channel count (rows co >= Co zero)
struct PackArgs {
  const float* w;
  void* dst;
  int Co, Ci, Cip;  // Cip: padded input channels (multiple of 8) for CONV3_FWD
  int KG, KGp, Cpad;
};

// Value of packed element (kgi, col, j) of a mode-`mode` image (0 outside the weight).
__device__ __forceinline__ float pack_value(const float* __restrict__ w, int mode, int Co, int Ci, int Cip, int kgi,
                                            int col, int j) {
  switch (mode) {
    case 0: {
      const int cpg = Cip >> 3, t = kgi / cpg, ci = (kgi % cpg) * 8 + j, co = col;
      if (co < Co && ci < Ci) return w[((long long)co * Ci + ci) * 27 + t];
    } break;
    case 1: {
      const int cpg = Co >> 3, t = kgi / cpg, co = (kgi % cpg) * 8 + j, ci = col;
      if (ci < Ci) return w[((long long)co * Ci + ci) * 27 + (26 - t)];
    } break;
    case 2: {
      const int ci = kgi * 8 + j, co = col;
      if (co < Co && ci < Ci) return w[(long long)co * Ci + ci];
    } break;
    case 3: {
      const int co = kgi * 8 + j, ci = col;
      if (ci < Ci && co < Co) return w[(long long)co * Ci + ci];
    } break;
    case 4: {
      const int ci = kgi * 8 + j;
      const int t = col / Co, co = col % Co;
      if (t < 8 && ci < Ci) return w[((long long)ci * Co + co) * 8 + t];
    } break;
    case 5: {
      const int cpg = Co >> 3, t = kgi / cpg, co = (kgi % cpg) * 8 + j, ci = col;
      if (ci < Ci) return w[((long long)ci * Co + co) * 8 + t];
    } break;
    case 6: {   // CONV3_DGRAD over Cop = Cip padded output channels (zero rows co >= Co)
      const int cpg = Cip >> 3, t = kgi / cpg, co = (kgi % cpg) * 8 + j, ci = col;
      if (ci < Ci && co < Co) return w[((long long)co * Ci + ci) * 27 + (26 - t)];
    } break;
    case 7: {   // CONVT_DGRAD over Cop = Cip padded output channels
      const int cpg = Cip >> 3, t = kgi / cpg, co = (kgi % cpg) * 8 + j, ci = col;
      if (ci < Ci && co < Co) return w[((long long)ci * Co + co) * 8 + t];
    } break;
  }
  return 0.f;
}

template <typename T>
__global__ void pack_weight_kernel(PackArgs g, int mode) {
  long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)g.KGp * g.Cpad * 8;
  if (idx >= total) return;
  const int j = (int)(idx & 7);
  const long long q = idx >> 3;
  const int col = (int)(q % g.Cpad);
  const int kgi = (int)(q / g.Cpad);
  const float v = kgi < g.KG ? pack_value(g.w, mode, g.Co, g.Ci, g.Cip, kgi, col, j) : 0.f;
  reinterpret_cast<T*>(g.dst)[idx] = from_f<T>(v);
}

// Batched 3^3 pack: one launch writes BOTH operand images of every 3^3 conv of
// a model (forward [27*Cip/8][Cpad][8] and flipped/transposed data-gradient
// [27*Co/8][Cpad_d][8]) from ONE coalesced read of the fp32 master weights.
// Block = (8 output channels, 32 input channels) of one layer: the 8 x 32 x 27
// source floats are contiguous runs per output channel, staged in LDS, then
// written as 16-B vectors (8 input channels for the forward image, 8 output
// channels for the data-gradient image).  Entries the block does not own
// (K padding, Cin padding of the stem) are zero from allocation.
struct Pack3Desc {
  const float* w;       // [Co][Ci][27]
  void* wf;             // forward image
  void* wd;             // data-gradient image or null
  int Co, Ci, Cip, Cpad, Cpad_d;
  int block_begin;      // first block of this layer in the launch
  int Cop;              // data-gradient reduction channels (pack mode 6: padded Co; 0 = Co)
  int pad1;
};

// The two operand images of one (8 co x 32 ci) tile of a 3^3 conv's weight staged in sw[co][ci][tap] (ci >= cis
// zero): forward image (tap, 8-ci group, co) and data-gradient image (tap s -> kgi = (26 - s) * Cop/8 + co0/8,
// column ci, 8 co per vector; rows co >= Co of a padded image are zero from allocation), 16-B stores.
template <typename T>
__device__ __forceinline__ void pack3_write(const float (*sw)[33][29], void* wfp, void* wdp, int Co, int Cip, int Cpad,
                                            int Cpad_d, int Cop, int co0, int ci0, int cis) {
  const int tid = threadIdx.x;
  const int cpg = Cip >> 3;
  const int ngrp = ((Cip - ci0) < 32 ? (Cip - ci0) : 32) >> 3;
  T* wf = reinterpret_cast<T*>(wfp);
  for (int e = tid; e < 27 * 4 * 8; e += 256) {
    const int co = e & 7, cg = (e >> 3) & 3, t = e >> 5;
    if (cg >= ngrp || co0 + co >= Co) continue;
    V8<T> v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v.set(j, sw[co][cg * 8 + j][t]);
    const long long kgi = (long long)t * cpg + (ci0 >> 3) + cg;
    v.store(wf + (kgi * Cpad + co0 + co) * 8);
  }
  if (wdp == nullptr) return;
  const int cpgd = (Cop > 0 ? Cop : Co) >> 3;
  T* wd = reinterpret_cast<T*>(wdp);
  for (int e = tid; e < 27 * 32; e += 256) {
    const int ci = e & 31, t = e >> 5;
    if (ci >= cis) continue;
    V8<T> v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v.set(j, sw[j][ci][t]);
    const long long kgi = (long long)(26 - t) * cpgd + (co0 >> 3);
    v.store(wd + (kgi * Cpad_d + ci0 + ci) * 8);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void pack_conv3_batched_kernel(const Pack3Desc* __restrict__ descs, int n) {
  __shared__ float sw[8][33][29];   // padded: conflict-free image reads (the [8][32][28] form was 32-way on the forward image)
  int lo = 0, hi = n - 1;
  const int b = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].block_begin <= b) lo = mid;
    else hi = mid - 1;
  }
  const Pack3Desc d = descs[lo];
  const int nci = (d.Ci + 31) / 32;
  const int lb = b - d.block_begin;
  const int co0 = (lb / nci) * 8, ci0 = (lb % nci) * 32;
  const int cis = d.Ci - ci0 < 32 ? d.Ci - ci0 : 32;
  const int tid = threadIdx.x;
  if (cis == 32 && co0 + 8 <= d.Co && (d.Ci & 3) == 0) {
    // full tile: each co row of the tile is 864 contiguous floats, 16-B aligned -> float4 loads
    for (int e = tid; e < 8 * 216; e += 256) {
      const int co = e / 216, r4 = (e - co * 216) * 4;
      const float4 v = *reinterpret_cast<const float4*>(d.w + ((long long)(co0 + co) * d.Ci + ci0) * 27 + r4);
      const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int r = r4 + k, ci = r / 27, t = r - ci * 27;
        sw[co][ci][t] = vv[k];
      }
    }
  } else {
    for (int e = tid; e < 8 * 32 * 27; e += 256) {
      const int co = e / (32 * 27), r = e - co * (32 * 27);
      const int ci = r / 27, t = r - ci * 27;
      sw[co][ci][t] = (ci < cis && co0 + co < d.Co) ? d.w[((long long)(co0 + co) * d.Ci + ci0) * 27 + r] : 0.f;
    }
  }
  __syncthreads();
  pack3_write<T>(sw, d.wf, d.wd, d.Co, d.Cip, d.Cpad, d.Cpad_d, d.Cop, co0, ci0, cis);
}

// Batched pack: one launch packs every layer of a model (descriptor table in device memory).
struct PackDesc {
  const float* w;
  void* dst;
  int mode, Co, Ci, Cip, KG, KGp, Cpad, pad0;
  long long begin;   // first element (of the virtual concatenation) owned by this descriptor
};

template <typename T>
__global__ void pack_weight_batched_kernel(const PackDesc* __restrict__ descs, int n, long long total) {
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {                    // last descriptor with begin <= idx
      const int mid = (lo + hi + 1) >> 1;
      if (descs[mid].begin <= idx) lo = mid;
      else hi = mid - 1;
    }
    const PackDesc d = descs[lo];
    const long long li = idx - d.begin;
    const int j = (int)(li & 7);
    const long long q = li >> 3;
    const int col = (int)(q % d.Cpad);
    const int kgi = (int)(q / d.Cpad);
    const float v = kgi < d.KG ? pack_value(d.w, d.mode, d.Co, d.Ci, d.Cip, kgi, col, j) : 0.f;
    reinterpret_cast<T*>(d.dst)[li] = from_f<T>(v);
  }
}

// ------------------------------------------------------------ fused AdamW + weight pack
// The captured training step's optimizer launch (mmseg_adamw_pack_dev): the AdamW update of the whole flat arena
// (adamw_one: mmseg_adamw_dev's per-element bits) with every packed weight's NEW value also written into its
// operand images -- what mmseg_pack_conv3_batched / mmseg_pack_weights_batched would write from the updated fp32
// weights at the next forward, which then skips its pack (one read of the fp32 weights and two launches less per
// step).  Blocks by descriptor kind:
//   0  3^3 conv: (8 co x 32 ci x 27 taps) tiles, pack_conv3_batched_kernel's tiles and image writes;
//   1  1x1 / token linear W[Co][Ci] (pack modes 2 / 3) or transposed conv W[Ci][Co][8] (modes 4 / 5 / 7):
//      8 source rows x up to AP_KT columns staged in LDS, written as 16-B vectors per image;
//   2  a plain range of the arena (biases, norm / LayerNorm parameters, tables): the update only.
// The host table (engine/layers.py Packer.adam_table) covers every arena element exactly once.  Entries no block
// owns (K / channel padding) stay zero from allocation, as with the batched packs.
constexpr int AP_KT = 512;      // kind-1 tile columns (a multiple of 64: whole 8-co groups of a transposed conv)
constexpr int AP_RANGE = 4096;  // kind-2 elements per block
struct AdamPackDesc {
  void* d0;            // kind 0: forward image; kind 1: the mode0 image
  void* d1;            // data-gradient image / the mode1 image (null: none)
  long long off;       // first arena element of the weight (kind 0 / 1) or of the range (kind 2)
  int kind, block_begin;
  int R, K;            // kind 1: source rows x columns; kind 2: K = the range's length
  int mode0, mode1;    // kind 1: pack modes of d0 / d1
  int Co, Ci, Cip, Cpad, Cpad_d, Cop;   // kind 0: Pack3Desc's fields; kind 1: the weight's Co, Ci, Cpad / Cpad_d
                                        // of d0 / d1, Cop of mode 7
};

// AdamW over `rows` runs of `len` arena elements (run r starts at a0 + r * stride); the new value of element
// (r, i) goes to put(r, i, value).  float4 lanes when every run is 16-B aligned.
template <typename PUT>
__device__ __forceinline__ void ap_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, long long a0, long long stride, int rows, int len,
                                          const AdamHyper& h, PUT&& put) {
  const int tid = threadIdx.x;
  if (((a0 | stride | (long long)len) & 3) == 0) {
    const int n4 = len >> 2, tot = rows * n4;
    for (int e = tid; e < tot; e += 256) {
      const int r = e / n4, q = e - r * n4;
      const long long k = ((a0 + r * stride) >> 2) + q;
      float4 pv = reinterpret_cast<const float4*>(p)[k];
      const float4 gv = reinterpret_cast<const float4*>(g)[k];
      float4 mv = reinterpret_cast<const float4*>(m)[k];
      float4 vv = reinterpret_cast<const float4*>(v)[k];
      adamw_one(pv.x, gv.x, mv.x, vv.x, h);
      adamw_one(pv.y, gv.y, mv.y, vv.y, h);
      adamw_one(pv.z, gv.z, mv.z, vv.z, h);
      adamw_one(pv.w, gv.w, mv.w, vv.w, h);
      reinterpret_cast<float4*>(p)[k] = pv;
      reinterpret_cast<float4*>(m)[k] = mv;
      reinterpret_cast<float4*>(v)[k] = vv;
      put(r, 4 * q, pv.x);
      put(r, 4 * q + 1, pv.y);
      put(r, 4 * q + 2, pv.z);
      put(r, 4 * q + 3, pv.w);
    }
  } else {
    const int tot = rows * len;
    for (int e = tid; e < tot; e += 256) {
      const int r = e / len, i = e - r * len;
      const long long k = a0 + r * stride + i;
      float pv = p[k], mv = m[k], vv = v[k];
      adamw_one(pv, g[k], mv, vv, h);
      p[k] = pv;
      m[k] = mv;
      v[k] = vv;
      put(r, i, pv);
    }
  }
}

// one image of a kind-1 tile: s[8][AP_KT + 1] rows r0 .. r0 + 7, columns k0 .. k0 + kt (kt8: kt rounded up to 8,
// zero past kt)
template <typename T>
__device__ __forceinline__ void ap_write1(const float (*s)[AP_KT + 1], int mode, void* dstp, int cpad, int Co, int Cop,
                                          int r0, int k0, int kt, int kt8) {
  const int tid = threadIdx.x;
  T* dst = reinterpret_cast<T*>(dstp);
  if (mode == 2) {            // 1x1 forward: (ci group, co) <- 8 ci of row co
    for (int e = tid; e < kt8; e += 256) {
      const int rr = e & 7, cg = e >> 3;
      V8<T> w;
#pragma unroll
      for (int j = 0; j < 8; ++j) w.set(j, s[rr][cg * 8 + j]);
      w.store(dst + ((long long)((k0 >> 3) + cg) * cpad + r0 + rr) * 8);
    }
  } else if (mode == 3) {     // 1x1 data gradient: (co group r0 / 8, ci) <- the tile's 8 rows of column ci
    for (int c = tid; c < kt; c += 256) {
      V8<T> w;
#pragma unroll
      for (int j = 0; j < 8; ++j) w.set(j, s[j][c]);
      w.store(dst + ((long long)(r0 >> 3) * cpad + k0 + c) * 8);
    }
  } else if (mode == 4) {     // transposed forward: (ci group r0 / 8, t Co + co) <- 8 rows of column co 8 + t
    const int ncol8 = kt >> 3;
    for (int e = tid; e < kt; e += 256) {
      const int t = e / ncol8, col = e - t * ncol8;
      V8<T> w;
#pragma unroll
      for (int j = 0; j < 8; ++j) w.set(j, s[j][col * 8 + t]);
      w.store(dst + ((long long)(r0 >> 3) * cpad + t * Co + (k0 >> 3) + col) * 8);
    }
  } else {                    // 5 / 7 transposed data gradient: (t Cop/8 + co group, ci) <- 8 co of row ci, tap t
    const int cpgd = (mode == 7 ? Cop : Co) >> 3, ngrp = kt >> 6;
    for (int e = tid; e < 64 * ngrp; e += 256) {
      const int rr = e & 7, t = (e >> 3) & 7, cg = e >> 6;
      V8<T> w;
#pragma unroll
      for (int j = 0; j < 8; ++j) w.set(j, s[rr][(cg * 8 + j) * 8 + t]);
      const int co = (k0 >> 3) + cg * 8;
      w.store(dst + ((long long)(t * cpgd + (co >> 3)) * cpad + r0 + rr) * 8);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void adamw_pack_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v,
                                                         const AdamPackDesc* __restrict__ descs, int n,
                                                         AdamHyper hv, const AdamHyper* __restrict__ hp,
                                                         const float* __restrict__ skip) {
  __shared__ float sw[8][33][29];
  AdamHyper h;
  if (!adamw_load(hv, hp, skip, h)) return;
  int lo = 0, hi = n - 1;
  const int b = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].block_begin <= b) lo = mid;
    else hi = mid - 1;
  }
  const AdamPackDesc d = descs[lo];
  const int lb = b - d.block_begin;
  const int tid = threadIdx.x;
  if (d.kind == 0) {
    const int nci = (d.Ci + 31) / 32;
    const int co0 = (lb / nci) * 8, ci0 = (lb % nci) * 32;
    const int cis = d.Ci - ci0 < 32 ? d.Ci - ci0 : 32;
    if (co0 >= d.Co) return;
    for (int e = tid; e < 8 * (32 - cis) * 27; e += 256) {   // the tile's channel padding reads as zero
      const int co = e / ((32 - cis) * 27), r = e - co * ((32 - cis) * 27);
      sw[co][cis + r / 27][r % 27] = 0.f;
    }
    ap_update(p, g, m, v, d.off + ((long long)co0 * d.Ci + ci0) * 27, (long long)d.Ci * 27, 8, cis * 27, h,
              [&](int r, int i, float x) __attribute__((always_inline)) {
                const int ci = i / 27;
                sw[r][ci][i - ci * 27] = x;
              });
    __syncthreads();
    pack3_write<T>(sw, d.d0, d.d1, d.Co, d.Cip, d.Cpad, d.Cpad_d, d.Cop, co0, ci0, cis);
  } else if (d.kind == 1) {
    float (*s)[AP_KT + 1] = reinterpret_cast<float (*)[AP_KT + 1]>(&sw[0][0][0]);
    const int nkt = (d.K + AP_KT - 1) / AP_KT;
    const int r0 = (lb / nkt) * 8, k0 = (lb % nkt) * AP_KT;
    const int kt = d.K - k0 < AP_KT ? d.K - k0 : AP_KT, kt8 = (kt + 7) & ~7;
    if (r0 >= d.R) return;
    for (int e = tid; e < 8 * (kt8 - kt); e += 256) s[e / (kt8 - kt)][kt + e % (kt8 - kt)] = 0.f;
    ap_update(p, g, m, v, d.off + (long long)r0 * d.K + k0, d.K, 8, kt, h,
              [&](int r, int i, float x) __attribute__((always_inline)) { s[r][i] = x; });
    __syncthreads();
    ap_write1<T>(s, d.mode0, d.d0, d.Cpad, d.Co, d.Cop, r0, k0, kt, kt8);
    if (d.d1 != nullptr) ap_write1<T>(s, d.mode1, d.d1, d.Cpad_d, d.Co, d.Cop, r0, k0, kt, kt8);
  } else {
    if (lb * AP_RANGE >= d.K) return;
    const long long a0 = d.off + (long long)lb * AP_RANGE;
    const int len = d.K - lb * AP_RANGE < AP_RANGE ? d.K - lb * AP_RANGE : AP_RANGE;
    ap_update(p, g, m, v, a0, 0, 1, len, h, [](int, int, float) __attribute__((always_inline)) {});
  }
}

}  // namespace

// e4m3 B-operand image of a 3^3 conv for brick6 F8 ([KGp][Cpad][8] bytes, the bf16 image's geometry): one block
// per output channel: s = 448 / max |w[co]| (1 for an all-zero row; 448 = e4m3fn's largest finite value), the
// entries w[co][ci][tap] * s rounded to e4m3 (v_cvt_pk_fp8_f32: round to nearest even), wdq[co] = 1 / s.
__global__ __launch_bounds__(256) void pack_conv3_fp8_kernel(const float* __restrict__ w, int Ci, int Cip, int Cpad,
                                                             unsigned char* __restrict__ dst, float* __restrict__ wdq) {
  const int co = blockIdx.x, tid = threadIdx.x;
  const int n = Ci * 27;
  const float* wr = w + (long long)co * n;
  float m = 0.f;
  for (int e = tid; e < n; e += 256) m = fmaxf(m, fabsf(wr[e]));
  __shared__ float red[4];
  m = fmaxf(m, __shfl_xor(m, 1, 64));
#pragma unroll
  for (int o = 2; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float sc = m > 0.f ? 448.f / m : 1.f;
  if (tid == 0) wdq[co] = 1.f / sc;
  for (int e = tid; e < n; e += 256) {
    const int ci = e / 27, tap = e - ci * 27;
    const int kgi = tap * (Cip / 8) + ci / 8;
    const int v = __builtin_amdgcn_cvt_pk_fp8_f32(wr[e] * sc, 0.f, 0, false);
    dst[((long long)kgi * Cpad + co) * 8 + (ci & 7)] = (unsigned char)(v & 0xff);
  }
}

// =================================================================== C ABI
extern "C" {

// Pack fp32 torch-layout weights into the MFMA B-operand layout [KGp][Cpad][8].
int mmseg_pack_weight(const float* w, void* dst, int mode, int Co, int Ci, int Cip, int KG, int KGp, int Cpad,
                      int dtype, void* stream) {
  PackArgs g{w, dst, Co, Ci, Cip, KG, KGp, Cpad};
  long long total = (long long)KGp * Cpad * 8;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MMSEG_BF16)
    MMSEG_LAUNCH(pack_weight_kernel<bf16_t>, dim3(ceil_div(total, 256)), dim3(256), 0, s, g, mode);
  else
    MMSEG_LAUNCH(pack_weight_kernel<float>, dim3(ceil_div(total, 256)), dim3(256), 0, s, g, mode);
  return mmseg::check_launch("pack_weight");
}

int mmseg_pack3_desc_bytes(void) { return (int)sizeof(Pack3Desc); }

int mmseg_adamw_pack_desc_bytes(void) { return (int)sizeof(AdamPackDesc); }

static int adamw_pack_launch(float* p, const float* g, float* m, float* v, const void* descs, int n, int nblocks,
                             const AdamHyper& hv, const AdamHyper* hp, const float* skip, int dtype,
                             hipStream_t s) {
  MMSEG_REQUIRE(n >= 1 && nblocks >= 1 && descs != nullptr, "adamw_pack: a descriptor table (Packer.adam_table)");
  MMSEG_REQUIRE(((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                  reinterpret_cast<uintptr_t>(v)) & 15) == 0, "adamw_pack: p, g, m, v must be 16-B aligned");
  if (dtype == MMSEG_BF16)
    MMSEG_LAUNCH(adamw_pack_kernel<bf16_t>, dim3(nblocks), dim3(256), 0, s, p, g, m, v, (const AdamPackDesc*)descs,
                 n, hv, hp, skip);
  else
    MMSEG_LAUNCH(adamw_pack_kernel<float>, dim3(nblocks), dim3(256), 0, s, p, g, m, v, (const AdamPackDesc*)descs,
                 n, hv, hp, skip);
  return mmseg::check_launch("adamw_pack");
}

// descs: device array of n AdamPackDesc sorted by block_begin, nblocks blocks in all (Packer.adam_table); the
// step's hyper-parameters by value (as mmseg_adamw) or as the 8 device floats of mmseg_adamw_hyper (as
// mmseg_adamw_dev); skip as there.  p / g / m / v: the flat arenas, 16-B aligned.
int mmseg_adamw_pack(float* p, const float* g, float* m, float* v, const void* descs, int n, int nblocks, float lr,
                     float beta1, float beta2, float eps, float wd, int step, const float* skip, int dtype,
                     void* stream) {
  MMSEG_REQUIRE(step >= 1, "adamw_pack: step counts from 1");
  return adamw_pack_launch(p, g, m, v, descs, n, nblocks, adamw_hyper(lr, beta1, beta2, eps, wd, step), nullptr, skip,
                           dtype, (hipStream_t)stream);
}

int mmseg_adamw_pack_dev(float* p, const float* g, float* m, float* v, const void* descs, int n, int nblocks,
                         const float* hyper, const float* skip, int dtype, void* stream) {
  MMSEG_REQUIRE(hyper != nullptr, "adamw_pack_dev: hyper (8 device floats from mmseg_adamw_hyper) required");
  return adamw_pack_launch(p, g, m, v, descs, n, nblocks, AdamHyper{}, reinterpret_cast<const AdamHyper*>(hyper),
                           skip, dtype, (hipStream_t)stream);
}

// descs: device array of n Pack3Desc sorted by block_begin; nblocks = total blocks
// (sum over layers of Co/8 * ceil(Ci/32)).  The images must be zero-initialised once.
int mmseg_pack_conv3_batched(const void* descs, int n, int nblocks, int dtype, void* stream) {
  MMSEG_REQUIRE(n >= 1 && nblocks >= 1, "pack_conv3_batched: empty table");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MMSEG_BF16)
    MMSEG_LAUNCH(pack_conv3_batched_kernel<bf16_t>, dim3(nblocks), dim3(256), 0, s, (const Pack3Desc*)descs, n);
  else
    MMSEG_LAUNCH(pack_conv3_batched_kernel<float>, dim3(nblocks), dim3(256), 0, s, (const Pack3Desc*)descs, n);
  return mmseg::check_launch("pack_conv3_batched");
}

// descs: device array of n PackDesc (64 B each, see mmseg_pack_desc_bytes); total = sum of KGp*Cpad*8.
int mmseg_pack_desc_bytes(void) { return (int)sizeof(PackDesc); }

int mmseg_pack_weights_batched(const void* descs, int n, long long total, int dtype, void* stream) {
  MMSEG_REQUIRE(n >= 1, "pack_weights_batched: n >= 1");
  hipStream_t s = (hipStream_t)stream;
  long long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (dtype == MMSEG_BF16)
    MMSEG_LAUNCH(pack_weight_batched_kernel<bf16_t>, dim3((int)blocks), dim3(256), 0, s, (const PackDesc*)descs,
                       n, total);
  else
    MMSEG_LAUNCH(pack_weight_batched_kernel<float>, dim3((int)blocks), dim3(256), 0, s, (const PackDesc*)descs,
                       n, total);
  return mmseg::check_launch("pack_weights_batched");
}

int mmseg_pack_conv3_fp8(const float* w, int Co, int Ci, int Cip, int KGp, int Cpad, void* dst, float* wdq,
                         void* stream) {
  MMSEG_REQUIRE(w && dst && wdq && Co > 0 && Co <= Cpad && Ci <= Cip && Cip % 8 == 0 && KGp * 8 >= 27 * Cip,
                "pack_conv3_fp8: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  hipMemsetAsync(dst, 0, (size_t)KGp * Cpad * 8, s);   // K / column padding stays e4m3 zero
  MMSEG_LAUNCH(pack_conv3_fp8_kernel, dim3(Co), dim3(256), 0, s, w, Ci, Cip, Cpad, (unsigned char*)dst, wdq);
  return mmseg::check_launch("pack_conv3_fp8");
}

}  // extern "C"
