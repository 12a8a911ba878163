// Explainability passes (reference src/explainability/gradcam.py, shap_analysis.py) over the engine's tapped
// activations and gradient sources.  All of them are memory-bound, run on the caller's stream, allocate nothing
// and reduce in a fixed order (per-block partials, then one ordered sweep), so two identical calls give the same
// bits; there are no float atomics.
//
//   explain_seed        d logits of logits[0, c].max() (ties share evenly, as torch's amax backward) or .mean()
//   cam_weights         per-channel weights of Grad-CAM (mean_v g) and Grad-CAM++ (sum_v alpha relu(g)), the
//                       gradient g gathered from its sources as the InstanceNorm backward gathers it (dy_gather.h)
//   cam_combine         relu(sum_c w_c A[v][c])
//   cam_upsample_norm   F.interpolate(trilinear, align_corners=False) + (x - min) / (max - min + 1e-8)
//   attr_lerp / finish  baseline + t (x - baseline)  /  (x - baseline) g scale   (gradient-SHAP, integrated gradients)
#include "mmseg_common.h"
#include "dy_gather.h"

#include <algorithm>

namespace {

constexpr int EX_BLOCK = 256;
constexpr int EX_MAXBLK = 1024;   // partial blocks of the seed / min-max reduces

inline int ex_grid(long long n, int per_block) {
  long long g = (n + per_block - 1) / per_block;
  return (int)std::max(1LL, std::min(g, (long long)EX_MAXBLK));
}

// ------------------------------------------------------------------ seed
// block b: (max, count of elements equal to it) over its contiguous range of logits[c]
__global__ void seed_max_partial(const float* __restrict__ x, long long V, long long per, float* __restrict__ part) {
  const long long v0 = (long long)blockIdx.x * per;
  const long long v1 = v0 + per < V ? v0 + per : V;
  float m = -INFINITY;
  float cnt = 0.f;
  for (long long v = v0 + threadIdx.x; v < v1; v += EX_BLOCK) {
    const float a = x[v];
    if (a > m) {
      m = a;
      cnt = 1.f;
    } else if (a == m) {
      cnt += 1.f;
    }
  }
  __shared__ float sm[EX_BLOCK], sc[EX_BLOCK];
  sm[threadIdx.x] = m;
  sc[threadIdx.x] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    float bm = -INFINITY, bc = 0.f;
    for (int i = 0; i < EX_BLOCK; ++i) {
      if (sm[i] > bm) {
        bm = sm[i];
        bc = sc[i];
      } else if (sm[i] == bm) {
        bc += sc[i];
      }
    }
    part[2 * blockIdx.x] = bm;
    part[2 * blockIdx.x + 1] = bc;
  }
}

// the partials in block order -> res[0] = max, res[1] = 1 / (number of maxima)
__global__ void seed_max_final(const float* __restrict__ part, int nblk, float* __restrict__ res) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float bm = -INFINITY, bc = 0.f;
  for (int i = 0; i < nblk; ++i) {
    const float m = part[2 * i], c = part[2 * i + 1];
    if (m > bm) {
      bm = m;
      bc = c;
    } else if (m == bm) {
      bc += c;
    }
  }
  res[0] = bm;
  res[1] = bc > 0.f ? 1.f / bc : 0.f;
}

// dlogits[ch][v]: zero off the class; on it 1/V (mode mean) or [x == max] / count (mode max)
__global__ void seed_fill(const float* __restrict__ x, int C, long long V, int cls, int mode,
                          const float* __restrict__ res, float inv_v, float* __restrict__ out) {
  const long long total = (long long)C * V;
  const float mx = mode == 0 ? res[0] : 0.f;
  const float share = mode == 0 ? res[1] : inv_v;
  for (long long i = (long long)blockIdx.x * EX_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * EX_BLOCK) {
    const long long ch = i / V;
    float g = 0.f;
    if (ch == cls) g = mode == 0 ? (x[i] == mx ? share : 0.f) : share;
    out[i] = g;
  }
}

// --------------------------------------------------------------- weights
// Block = (256 / C8) voxel lanes x C8 channel groups, a thread owns 8 channels (instnorm.hip's layout); chunk b of
// the voxels -> part[b][C].  MODE 0: sum_v g.  MODE 1: sum_v alpha g over g > 0, alpha = g^2 / (2 g^2 + S g^3 + 1e-8)
// with S = sum_v A per channel (suma).  MODE 2: sum_v A (Grad-CAM++'s first pass; no gradient read).
template <typename T, int MODE>
__global__ void cam_weights_partial(const T* __restrict__ A, int lda, DySrc s, const float* __restrict__ suma, int V,
                                    int C, int D, int H, int W, int vpc, float* __restrict__ part) {
  const int chunk = blockIdx.x;
  const int C8 = C >> 3;
  const int lanes_v = EX_BLOCK / C8;
  const int tid = threadIdx.x;
  const int cg = tid % C8, vl = tid / C8;
  float acc[8], sa[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    acc[j] = 0.f;
    sa[j] = 0.f;
  }
  const int v0 = chunk * vpc;
  const int v1 = v0 + vpc < V ? v0 + vpc : V;
  if (vl < lanes_v) {
    if constexpr (MODE == 2) {
      const T* an = A + cg * 8;
      for (int v = v0 + vl; v < v1; v += lanes_v) {
        V8<T> a;
        a.load(an + (long long)v * lda);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += a.get(j);
      }
    } else {
      if constexpr (MODE == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) sa[j] = suma[cg * 8 + j];
      }
      const DyCtx<T> dc(s, 0, V, cg, C, D, H, W);
      constexpr int U = 4;
      for (int vb = v0 + vl; vb < v1; vb += U * lanes_v) {
        typename DyCtx<T>::Raw r[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (vb + u * lanes_v < v1) dc.load(vb + u * lanes_v, r[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (vb + u * lanes_v >= v1) break;
          float g[8];
          dc.combine(r[u], g);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if constexpr (MODE == 0) {
              acc[j] += g[j];
            } else {
              const float g2 = g[j] * g[j];
              const float alpha = g2 / (2.f * g2 + sa[j] * (g2 * g[j]) + 1e-8f);
              acc[j] += g[j] > 0.f ? alpha * g[j] : 0.f;
            }
          }
        }
      }
    }
  }
  __shared__ float red[EX_BLOCK * 8];
#pragma unroll
  for (int j = 0; j < 8; ++j) red[tid * 8 + j] = vl < lanes_v ? acc[j] : 0.f;
  __syncthreads();
  for (int c = tid; c < C; c += EX_BLOCK) {
    const int g = c >> 3, j = c & 7;
    float a = 0.f;
    for (int l = 0; l < lanes_v; ++l) a += red[(l * C8 + g) * 8 + j];
    part[(long long)chunk * C + c] = a;
  }
}

// out[c] = scale * sum_b part[b][c], b in order
__global__ void cam_weights_final(const float* __restrict__ part, int nchunk, int C, float scale,
                                  float* __restrict__ out) {
  const int c = blockIdx.x * EX_BLOCK + threadIdx.x;
  if (c >= C) return;
  float a = 0.f;
  for (int b = 0; b < nchunk; ++b) a += part[(long long)b * C + c];
  out[c] = a * scale;
}

// --------------------------------------------------------------- combine
// cam[v] = relu(sum_c w[c] A[v][c]): a thread's 8 channels, then the channel groups of a voxel in order through LDS
template <typename T>
__global__ void cam_combine_kernel(const T* __restrict__ A, int lda, const float* __restrict__ w, long long V, int C,
                                   float* __restrict__ out) {
  const int C8 = C >> 3;
  const int lanes_v = EX_BLOCK / C8;
  const int tid = threadIdx.x;
  const int cg = tid % C8, vl = tid / C8;
  float wv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) wv[j] = vl < lanes_v ? w[cg * 8 + j] : 0.f;
  __shared__ float red[EX_BLOCK];
  for (long long vb = (long long)blockIdx.x * lanes_v; vb < V; vb += (long long)gridDim.x * lanes_v) {
    const long long v = vb + vl;
    float a = 0.f;
    if (vl < lanes_v && v < V) {
      V8<T> x;
      x.load(A + v * lda + cg * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) a = fmaf(wv[j], x.get(j), a);
    }
    red[tid] = a;
    __syncthreads();
    if (tid < lanes_v && vb + tid < V) {
      float t = 0.f;
      for (int g = 0; g < C8; ++g) t += red[tid * C8 + g];
      out[vb + tid] = t > 0.f ? t : 0.f;
    }
    __syncthreads();
  }
}

// -------------------------------------------------------------- upsample
// F.interpolate(mode="trilinear", align_corners=False): src = max(0, (dst + 0.5) in/out - 0.5)
__device__ __forceinline__ void lin_src(int o, float scale, int in, int& i0, int& i1, float& l1) {
  float s = ((float)o + 0.5f) * scale - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
}

__global__ void cam_upsample_kernel(const float* __restrict__ cam, int d, int h, int w, float* __restrict__ out, int D,
                                    int H, int W, float* __restrict__ part) {
  const long long total = (long long)D * H * W;
  const float sz = (float)d / (float)D, sy = (float)h / (float)H, sx = (float)w / (float)W;
  float mn = INFINITY, mx = -INFINITY;
  for (long long i = (long long)blockIdx.x * EX_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * EX_BLOCK) {
    const int x = (int)(i % W);
    const long long q = i / W;
    const int y = (int)(q % H), z = (int)(q / H);
    int z0, z1, y0, y1, x0, x1;
    float lz, ly, lx;
    lin_src(z, sz, d, z0, z1, lz);
    lin_src(y, sy, h, y0, y1, ly);
    lin_src(x, sx, w, x0, x1, lx);
    const float* p0 = cam + (long long)z0 * h * w;
    const float* p1 = cam + (long long)z1 * h * w;
    const float hz = 1.f - lz, hy = 1.f - ly, hx = 1.f - lx;
    const float v = hz * (hy * (hx * p0[y0 * w + x0] + lx * p0[y0 * w + x1]) +
                          ly * (hx * p0[y1 * w + x0] + lx * p0[y1 * w + x1])) +
                    lz * (hy * (hx * p1[y0 * w + x0] + lx * p1[y0 * w + x1]) +
                          ly * (hx * p1[y1 * w + x0] + lx * p1[y1 * w + x1]));
    out[i] = v;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  __shared__ float smn[EX_BLOCK], smx[EX_BLOCK];
  smn[threadIdx.x] = mn;
  smx[threadIdx.x] = mx;
  __syncthreads();
  for (int o = EX_BLOCK / 2; o > 0; o >>= 1) {   // (min / max: any order gives the same value)
    if (threadIdx.x < o) {
      smn[threadIdx.x] = fminf(smn[threadIdx.x], smn[threadIdx.x + o]);
      smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = smn[0];
    part[2 * blockIdx.x + 1] = smx[0];
  }
}

// every block folds the nblk partials itself (<= 8 KB from L2), then normalises its elements in place
__global__ void cam_norm_kernel(float* __restrict__ out, long long total, const float* __restrict__ part, int nblk) {
  __shared__ float smn[EX_BLOCK], smx[EX_BLOCK];
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < nblk; i += EX_BLOCK) {
    mn = fminf(mn, part[2 * i]);
    mx = fmaxf(mx, part[2 * i + 1]);
  }
  smn[threadIdx.x] = mn;
  smx[threadIdx.x] = mx;
  __syncthreads();
  for (int o = EX_BLOCK / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      smn[threadIdx.x] = fminf(smn[threadIdx.x], smn[threadIdx.x + o]);
      smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + o]);
    }
    __syncthreads();
  }
  mn = smn[0];
  const float den = (smx[0] - mn) + 1e-8f;
  for (long long i = (long long)blockIdx.x * EX_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * EX_BLOCK)
    out[i] = (out[i] - mn) / den;
}

// ----------------------------------------------------------- attribution
__global__ void attr_lerp_kernel(const float* __restrict__ x, const float* __restrict__ base, float t,
                                 float* __restrict__ out, long long n) {
  for (long long i = (long long)blockIdx.x * EX_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * EX_BLOCK) {
    const float b = base ? base[i] : 0.f;
    out[i] = b + t * (x[i] - b);
  }
}

__global__ void attr_finish_kernel(const float* __restrict__ x, const float* __restrict__ base,
                                   const float* __restrict__ g, float scale, float* __restrict__ out, long long n) {
  for (long long i = (long long)blockIdx.x * EX_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * EX_BLOCK) {
    const float b = base ? base[i] : 0.f;
    out[i] = (x[i] - b) * (g[i] * scale);
  }
}

inline int cam_chunks(long long V, int C) {
  const int lanes_v = EX_BLOCK / (C >> 3);
  long long n = (V + (long long)lanes_v * 16 - 1) / ((long long)lanes_v * 16);
  return (int)std::max(1LL, std::min(n, 1024LL));
}

}  // namespace

extern "C" {

long long mmseg_explain_ws_floats(void) { return 2 * EX_MAXBLK + 2; }

int mmseg_explain_seed(const float* logits, int C, long long V, int cls, int mode, float* dlogits, float* ws,
                       void* stream) {
  MMSEG_REQUIRE(logits && dlogits && ws && C >= 1 && V >= 1, "explain_seed: null pointer or empty shape");
  MMSEG_REQUIRE(cls >= 0 && cls < C, "explain_seed: class %d outside [0, %d)", cls, C);
  MMSEG_REQUIRE(mode == 0 || mode == 1, "explain_seed: mode 0 (max) or 1 (mean), got %d", mode);
  hipStream_t s = (hipStream_t)stream;
  float* res = ws + 2 * EX_MAXBLK;
  if (mode == 0) {
    const int nblk = ex_grid(V, EX_BLOCK * 16);
    const long long per = (V + nblk - 1) / nblk;
    MMSEG_LAUNCH(seed_max_partial, dim3(nblk), dim3(EX_BLOCK), 0, s, logits + (long long)cls * V, V, per, ws);
    MMSEG_LAUNCH(seed_max_final, dim3(1), dim3(64), 0, s, ws, nblk, res);
  }
  MMSEG_LAUNCH(seed_fill, dim3(ex_grid((long long)C * V, EX_BLOCK * 4)), dim3(EX_BLOCK), 0, s, logits, C, V, cls, mode,
               res, 1.f / (float)V, dlogits);
  return mmseg::check_launch("explain_seed");
}

long long mmseg_cam_ws_floats(long long V, int C) {
  if (C < 8 || C % 8 || C > 2048 || V < 1) return 0;
  return (long long)cam_chunks(V, C) * C + C;
}

int mmseg_cam_weights(const void* act, int lda, const void* p1, int ld1, float scale1, const void* pool_dy, int pool_ld,
                      const uint8_t* pool_idx, int D, int H, int W, int C, int mode, float* weights, float* ws,
                      int dtype, void* stream) {
  MMSEG_REQUIRE(weights && ws && (p1 || pool_dy), "cam_weights: null pointer (a gradient source is required)");
  MMSEG_REQUIRE(C >= 8 && C % 8 == 0 && C <= 2048, "cam_weights: C %d (a multiple of 8 up to 2048)", C);
  MMSEG_REQUIRE(D >= 1 && H >= 1 && W >= 1 && (long long)D * H * W < (1LL << 31), "cam_weights: volume");
  MMSEG_REQUIRE(mode == 0 || mode == 1, "cam_weights: mode 0 (Grad-CAM) or 1 (Grad-CAM++), got %d", mode);
  MMSEG_REQUIRE(mode == 0 || (act && lda >= C && lda % 8 == 0), "cam_weights: Grad-CAM++ reads the activation");
  MMSEG_REQUIRE(!p1 || (ld1 >= C && ld1 % 8 == 0), "cam_weights: ld1 %d", ld1);
  MMSEG_REQUIRE(!pool_dy || (pool_idx && pool_ld >= C && pool_ld % 8 == 0 && D % 2 == 0 && H % 2 == 0 && W % 2 == 0),
                "cam_weights: the pool source needs its argmax, pool_ld >= C and even dims");
  hipStream_t s = (hipStream_t)stream;
  const int V = D * H * W;
  const int nchunk = cam_chunks(V, C);
  const int vpc = (V + nchunk - 1) / nchunk;
  DySrc src{p1, ld1, scale1, nullptr, 0, nullptr, 0, pool_dy, pool_ld, pool_idx, 0, 0.f, 0};
  float* suma = ws + (long long)nchunk * C;
  const dim3 fgrid(ceil_div(C, EX_BLOCK));
  auto run = [&](auto tag) {
    using T = decltype(tag);
    const T* A = reinterpret_cast<const T*>(act);
    if (mode == 1) {
      MMSEG_LAUNCH((cam_weights_partial<T, 2>), dim3(nchunk), dim3(EX_BLOCK), 0, s, A, lda, src, nullptr, V, C, D, H,
                   W, vpc, ws);
      MMSEG_LAUNCH(cam_weights_final, fgrid, dim3(EX_BLOCK), 0, s, ws, nchunk, C, 1.f, suma);
      MMSEG_LAUNCH((cam_weights_partial<T, 1>), dim3(nchunk), dim3(EX_BLOCK), 0, s, A, lda, src, suma, V, C, D, H, W,
                   vpc, ws);
      MMSEG_LAUNCH(cam_weights_final, fgrid, dim3(EX_BLOCK), 0, s, ws, nchunk, C, 1.f, weights);
    } else {
      MMSEG_LAUNCH((cam_weights_partial<T, 0>), dim3(nchunk), dim3(EX_BLOCK), 0, s, A, lda, src, nullptr, V, C, D, H,
                   W, vpc, ws);
      MMSEG_LAUNCH(cam_weights_final, fgrid, dim3(EX_BLOCK), 0, s, ws, nchunk, C, 1.f / (float)V, weights);
    }
  };
  if (dtype == MMSEG_BF16) run(bf16_t{});
  else run(float{});
  return mmseg::check_launch("cam_weights");
}

int mmseg_cam_combine(const void* act, int lda, const float* weights, long long V, int C, float* cam, int dtype,
                      void* stream) {
  MMSEG_REQUIRE(act && weights && cam && V >= 1, "cam_combine: null pointer or empty shape");
  MMSEG_REQUIRE(C >= 8 && C % 8 == 0 && C <= 2048 && lda >= C && lda % 8 == 0, "cam_combine: C %d lda %d", C, lda);
  hipStream_t s = (hipStream_t)stream;
  const int lanes_v = EX_BLOCK / (C >> 3);
  const dim3 grid(ex_grid(V, lanes_v * 4));
  if (dtype == MMSEG_BF16)
    MMSEG_LAUNCH(cam_combine_kernel<bf16_t>, grid, dim3(EX_BLOCK), 0, s, (const bf16_t*)act, lda, weights, V, C, cam);
  else
    MMSEG_LAUNCH(cam_combine_kernel<float>, grid, dim3(EX_BLOCK), 0, s, (const float*)act, lda, weights, V, C, cam);
  return mmseg::check_launch("cam_combine");
}

int mmseg_cam_upsample_norm(const float* cam, int d, int h, int w, float* out, int D, int H, int W, float* ws,
                            void* stream) {
  MMSEG_REQUIRE(cam && out && ws, "cam_upsample_norm: null pointer");
  MMSEG_REQUIRE(d >= 1 && h >= 1 && w >= 1 && D >= d && H >= h && W >= w, "cam_upsample_norm: shape");
  for (int k = 0; k < 3; ++k) {
    const int i = k == 0 ? d : k == 1 ? h : w, o = k == 0 ? D : k == 1 ? H : W;
    const int r = o / i;
    MMSEG_REQUIRE(o % i == 0 && (r == 1 || r == 2 || r == 4 || r == 8 || r == 16),
                  "cam_upsample_norm: scale %d -> %d (1, 2, 4, 8 or 16 per axis)", i, o);
  }
  hipStream_t s = (hipStream_t)stream;
  const long long total = (long long)D * H * W;
  const int nblk = ex_grid(total, EX_BLOCK * 4);
  MMSEG_LAUNCH(cam_upsample_kernel, dim3(nblk), dim3(EX_BLOCK), 0, s, cam, d, h, w, out, D, H, W, ws);
  MMSEG_LAUNCH(cam_norm_kernel, dim3(nblk), dim3(EX_BLOCK), 0, s, out, total, ws, nblk);
  return mmseg::check_launch("cam_upsample_norm");
}

int mmseg_attr_lerp(const float* x, const float* baseline, float t, float* out, long long n, void* stream) {
  MMSEG_REQUIRE(x && out && n >= 1, "attr_lerp: null pointer or empty shape");
  MMSEG_LAUNCH(attr_lerp_kernel, dim3(ex_grid(n, EX_BLOCK * 4)), dim3(EX_BLOCK), 0, (hipStream_t)stream, x, baseline,
               t, out, n);
  return mmseg::check_launch("attr_lerp");
}

int mmseg_attr_finish(const float* x, const float* baseline, const float* grad, float scale, float* out, long long n,
                      void* stream) {
  MMSEG_REQUIRE(x && grad && out && n >= 1, "attr_finish: null pointer or empty shape");
  MMSEG_LAUNCH(attr_finish_kernel, dim3(ex_grid(n, EX_BLOCK * 4)), dim3(EX_BLOCK), 0, (hipStream_t)stream, x, baseline,
               grad, scale, out, n);
  return mmseg::check_launch("attr_finish");
}

}  // extern "C"
