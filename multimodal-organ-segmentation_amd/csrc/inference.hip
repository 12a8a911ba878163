// Sliding-window inference on device (reference trainer.py:370-395, which calls
// MONAI's sliding_window_inference with roi_size / overlap / sw_batch_size from
// configs/default.yaml:127-133; "mode" is not passed, so MONAI's default
// constant blending applies).
//
//   window_gather : windows [nw][M][r0][r1][r2] cut from the NCDHW volume,
//                   zero outside it (MONAI pads a volume smaller than the roi
//                   with zeros, symmetric; the host folds that padding into
//                   the window starts, which may be negative)
//   window_accum  : out[n][c][v] += logits of ONE window (launched per window
//                   in MONAI's window order, so every voxel's sum has the same
//                   fp32 addition order as MONAI's `output_image[idx] += pred`)
//   window_norm   : out /= count, count = per-axis coverage product (what
//                   MONAI's count_map holds for constant blending)
#include "mmseg_common.h"

namespace {

struct WinGeom {
  int N, C, D, H, W;     // volume (C = channels of the tensor being read / written)
  int r0, r1, r2;        // roi
};

__global__ void window_gather_kernel(const float* __restrict__ vol, WinGeom g, const int* __restrict__ win,
                                     int nw, float* __restrict__ out) {
  const long long rv = (long long)g.r0 * g.r1 * g.r2;
  const long long total = (long long)nw * g.C * rv;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(e % g.r2);
    long long q = e / g.r2;
    const int y = (int)(q % g.r1);
    q /= g.r1;
    const int z = (int)(q % g.r0);
    q /= g.r0;
    const int c = (int)(q % g.C);
    const int w = (int)(q / g.C);
    const int* s = win + 4 * w;    // (n, z0, y0, x0)
    const int zz = s[1] + z, yy = s[2] + y, xx = s[3] + x;
    float v = 0.f;
    if ((unsigned)zz < (unsigned)g.D && (unsigned)yy < (unsigned)g.H && (unsigned)xx < (unsigned)g.W)
      v = vol[(((long long)s[0] * g.C + c) * g.D + zz) * (long long)g.H * g.W + (long long)yy * g.W + xx];
    out[e] = v;
  }
}

__global__ void window_accum_kernel(const float* __restrict__ logits, WinGeom g, int n, int z0, int y0, int x0,
                                    float* __restrict__ out) {
  const long long rv = (long long)g.r0 * g.r1 * g.r2;
  const long long total = (long long)g.C * rv;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(e % g.r2);
    long long q = e / g.r2;
    const int y = (int)(q % g.r1);
    q /= g.r1;
    const int z = (int)(q % g.r0);
    const int c = (int)(q / g.r0);
    const int zz = z0 + z, yy = y0 + y, xx = x0 + x;
    if ((unsigned)zz < (unsigned)g.D && (unsigned)yy < (unsigned)g.H && (unsigned)xx < (unsigned)g.W) {
      float* o = out + (((long long)n * g.C + c) * g.D + zz) * (long long)g.H * g.W + (long long)yy * g.W + xx;
      *o = *o + logits[e];
    }
  }
}

__global__ void window_norm_kernel(float* __restrict__ out, WinGeom g, const float* __restrict__ cz,
                                   const float* __restrict__ cy, const float* __restrict__ cx) {
  const long long hw = (long long)g.H * g.W;
  const long long total = (long long)g.N * g.C * g.D * hw;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(e % g.W);
    const int y = (int)((e / g.W) % g.H);
    const int z = (int)((e / hw) % g.D);
    out[e] = out[e] / (cz[z] * cy[y] * cx[x]);
  }
}

int grid_for(long long total) {
  long long b = (total + 255) / 256;
  return (int)(b < 8192 ? (b < 1 ? 1 : b) : 8192);
}

// ---------------------------------------------------------------------------------------------------------
// Weighted blending and flip test-time augmentation (inference/sliding_window.py, blend / tta_flips).
//
//   window_gather_flip : window_gather, read mirrored along the axes of the flip mask (bit d = axis d); the
//                        zero padding belongs to the window, so it is mirrored with it
//   tta_accum          : acc (= | +=) the prediction of a flipped batch, mirrored back; the last flip also
//                        multiplies by 1 / flips (a power of two: exact)
//   window_blend       : out += w * pred and count += w for ALL windows of one predictor batch in one launch.
//                        A thread owns the output voxels it writes: voxel v of window k is handled by the thread
//                        at v of the FIRST window of the batch that covers it, which then walks every covering
//                        window in increasing index -- MONAI's per-voxel fp32 addition order with no atomics,
//                        although windows of one batch overlap
//   window_finish      : out /= count (count is a real [N][D][H][W] accumulator: Gaussian weights are not a
//                        per-axis coverage product)
//   blend_argmax       : argmax_encode of out / count without storing the quotient
// ---------------------------------------------------------------------------------------------------------
constexpr int BLEND_MAXW = 32;    // windows per launch: they travel as kernel arguments (uniform scalar tests)
constexpr int BLEND_PASS = 4;     // covering windows whose weights a thread keeps in registers at a time
struct BlendWins {
  int n[BLEND_MAXW], z0[BLEND_MAXW], y0[BLEND_MAXW], x0[BLEND_MAXW];
};

__global__ void window_gather_flip_kernel(const float* __restrict__ vol, WinGeom g, const int* __restrict__ win,
                                          int nw, int flip, float* __restrict__ out) {
  const long long rv = (long long)g.r0 * g.r1 * g.r2;
  const long long total = (long long)nw * g.C * rv;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    int x = (int)(e % g.r2);
    long long q = e / g.r2;
    int y = (int)(q % g.r1);
    q /= g.r1;
    int z = (int)(q % g.r0);
    q /= g.r0;
    const int c = (int)(q % g.C);
    const int w = (int)(q / g.C);
    if (flip & 1) z = g.r0 - 1 - z;
    if (flip & 2) y = g.r1 - 1 - y;
    if (flip & 4) x = g.r2 - 1 - x;
    const int* s = win + 4 * w;    // (n, z0, y0, x0)
    const int zz = s[1] + z, yy = s[2] + y, xx = s[3] + x;
    float v = 0.f;
    if ((unsigned)zz < (unsigned)g.D && (unsigned)yy < (unsigned)g.H && (unsigned)xx < (unsigned)g.W)
      v = vol[(((long long)s[0] * g.C + c) * g.D + zz) * (long long)g.H * g.W + (long long)yy * g.W + xx];
    out[e] = v;
  }
}

__global__ void tta_accum_kernel(const float* __restrict__ pred, long long rows, int r0, int r1, int r2, int flip,
                                 int assign, float scale, float* __restrict__ acc) {
  const long long rv = (long long)r0 * r1 * r2;
  const long long total = rows * rv;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    int x = (int)(e % r2);
    long long q = e / r2;
    int y = (int)(q % r1);
    q /= r1;
    int z = (int)(q % r0);
    const long long row = q / r0;
    if (flip & 1) z = r0 - 1 - z;
    if (flip & 2) y = r1 - 1 - y;
    if (flip & 4) x = r2 - 1 - x;
    const float p = pred[row * rv + ((long long)z * r1 + y) * r2 + x];
    const float s = assign ? p : acc[e] + p;
    acc[e] = s * scale;
  }
}

// importance_map * seg_prob, rounded, then output +=: hipcc would contract the pair to one v_fma_f32, whose
// result differs in the last bit
__device__ __forceinline__ float blend_add(float o, float w, float p) {
#pragma clang fp contract(off)
  const float t = w * p;
  return o + t;
}

template <int V> struct Vec;
template <> struct Vec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
};
template <> struct Vec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  }
  __device__ __forceinline__ void store(float* p) const {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};

// V = 4: W, r2 and every window's x0 are multiples of 4 (and the pointers 16-byte aligned), so a group of four
// voxels along W is aligned in the volume and in every window, and covered by a window as a whole.
// grid (blocks over a window's voxel groups, window k); pred [nw][C][r0][r1][r2].
template <int V>
__global__ __launch_bounds__(256) void window_blend_kernel(const float* __restrict__ pred, WinGeom g, BlendWins a,
                                                           int nw, int gaussian, const float* __restrict__ gz,
                                                           const float* __restrict__ gy, const float* __restrict__ gx,
                                                           float wmin, float* __restrict__ out,
                                                           float* __restrict__ count) {
  const int k = blockIdx.y;
  const int n = a.n[k];
  const int xg = g.r2 / V;
  const long long rv = (long long)g.r0 * g.r1 * g.r2;
  const long long dhw = (long long)g.D * g.H * g.W;
  const unsigned total = (unsigned)(g.r0 * g.r1 * xg);           // a window's voxels fit an int (checked by the host)
  for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int x = (int)(e % (unsigned)xg) * V;
    const unsigned q = e / (unsigned)xg;
    const int y = (int)(q % (unsigned)g.r1);
    const int z = (int)(q / (unsigned)g.r1);
    const int zz = a.z0[k] + z, yy = a.y0[k] + y, xx = a.x0[k] + x;
    if ((unsigned)zz >= (unsigned)g.D || (unsigned)yy >= (unsigned)g.H || (unsigned)xx >= (unsigned)g.W)
      continue;                                                    // the window's zero padding
    // windows of this image that cover the voxel group: bit j = window j
    uint32_t cover = 0;
    for (int j = 0; j < nw; ++j) {
      const bool in = a.n[j] == n && (unsigned)(zz - a.z0[j]) < (unsigned)g.r0 &&
                      (unsigned)(yy - a.y0[j]) < (unsigned)g.r1 && (unsigned)(xx - a.x0[j]) < (unsigned)g.r2;
      cover |= (in ? 1u : 0u) << j;
    }
    if (cover & ((1u << k) - 1u)) continue;                        // an earlier window's thread owns it
    const long long vox = ((long long)zz * g.H + yy) * g.W + xx;
    // the covering windows in increasing index, BLEND_PASS at a time: their weights and prediction offsets are
    // formed once and held in registers while the classes stream through (bits below k are clear: owned)
    for (uint32_t m = cover; m;) {
      float w[BLEND_PASS][V];
      long long po[BLEND_PASS];                                    // the group in window t's class 0, -1: no window
#pragma unroll
      for (int t = 0; t < BLEND_PASS; ++t) {
        po[t] = -1;
#pragma unroll
        for (int i = 0; i < V; ++i) w[t][i] = 1.f;
        if (m) {
          const int j = __ffs(m) - 1;
          m &= m - 1;
          const int lz = zz - a.z0[j], ly = yy - a.y0[j], lx = xx - a.x0[j];
          po[t] = (long long)j * g.C * rv + ((long long)lz * g.r1 + ly) * g.r2 + lx;
          if (gaussian) {
            const float wzy = gz[lz] * gy[ly];
#pragma unroll
            for (int i = 0; i < V; ++i) w[t][i] = fmaxf(wzy * gx[lx + i], wmin);
          }
        }
      }
      Vec<V> cnt;
      cnt.load(count + (long long)n * dhw + vox);
#pragma unroll
      for (int t = 0; t < BLEND_PASS; ++t)
        if (po[t] >= 0) {
#pragma unroll
          for (int i = 0; i < V; ++i) cnt.v[i] += w[t][i];
        }
      cnt.store(count + (long long)n * dhw + vox);
      for (int c = 0; c < g.C; ++c) {
        float* o = out + ((long long)n * g.C + c) * dhw + vox;
        Vec<V> acc;
        acc.load(o);
#pragma unroll
        for (int t = 0; t < BLEND_PASS; ++t)
          if (po[t] >= 0) {
            Vec<V> p;
            p.load(pred + po[t] + c * rv);
#pragma unroll
            for (int i = 0; i < V; ++i) acc.v[i] = blend_add(acc.v[i], w[t][i], p.v[i]);
          }
        acc.store(o);
      }
    }
  }
}

template <int V>
__global__ void window_finish_kernel(float* __restrict__ out, const float* __restrict__ count, int N, int C,
                                     long long vol) {
  const long long vg = vol / V;
  const long long total = (long long)N * C * vg;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long v = (e % vg) * V;
    const long long nc = e / vg;
    Vec<V> o, c;
    o.load(out + nc * vol + v);
    c.load(count + (nc / C) * vol + v);
#pragma unroll
    for (int i = 0; i < V; ++i) o.v[i] = o.v[i] / c.v[i];
    o.store(out + nc * vol + v);
  }
}

// argmax_encode (nifti.hip) over out[c] / count: 64 x 64 tiles over (x, z) of one y, read along z (contiguous
// in [X][Y][Z]), transposed through LDS, written along x (contiguous in file order)
constexpr int AT = 64, AW = 4;
__global__ __launch_bounds__(AT * AW) void blend_argmax_kernel(const float* __restrict__ acc,
                                                               const float* __restrict__ count, int C, int X, int Y,
                                                               int Z, int nbz, int nbx, uint8_t* __restrict__ out) {
  __shared__ uint32_t tile[AT][AT + 1];
  const int lane = threadIdx.x & (AT - 1), wave = threadIdx.x >> 6;
  unsigned b = blockIdx.x;
  const int bz = (int)(b % (unsigned)nbz);
  b /= (unsigned)nbz;
  const int bx = (int)(b % (unsigned)nbx), y = (int)(b / (unsigned)nbx);
  const int x0 = bx * AT, z0 = bz * AT;
  const size_t cs = (size_t)X * Y * Z;
  {
    const int z = z0 + lane;
    for (int r = wave; r < AT; r += AW) {
      const int x = x0 + r;
      if (x < X && z < Z) {
        const size_t v = ((size_t)x * Y + y) * Z + z;
        const float w = count[v];
        float best = acc[v] / w;       // the quotient decides: a > b does not order a / w and b / w after rounding
        uint32_t bi = 0;
        for (int c = 1; c < C; ++c) {
          const float t = acc[(size_t)c * cs + v] / w;
          if (t > best || (t != t && best == best)) {     // first maximum; a NaN counts as one (torch.argmax)
            best = t;
            bi = (uint32_t)c;
          }
        }
        tile[r][lane] = bi;
      }
    }
  }
  __syncthreads();
  const int x = x0 + lane;
#pragma unroll 4
  for (int r = wave; r < AT; r += AW) {
    const int z = z0 + r;
    if (x < X && z < Z) out[((size_t)z * Y + y) * X + x] = (uint8_t)tile[lane][r];
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" {

int mmseg_window_gather(const float* vol, int N, int C, int D, int H, int W, const int* win, int nw, int r0, int r1,
                        int r2, float* out, void* stream) {
  MMSEG_REQUIRE(nw >= 1 && r0 > 0 && r1 > 0 && r2 > 0, "window_gather: empty window set");
  WinGeom g{N, C, D, H, W, r0, r1, r2};
  MMSEG_LAUNCH(window_gather_kernel, dim3(grid_for((long long)nw * C * r0 * r1 * r2)), dim3(256), 0,
                     (hipStream_t)stream, vol, g, win, nw, out);
  return mmseg::check_launch("window_gather");
}

int mmseg_window_accum(const float* logits, int N, int C, int D, int H, int W, int n, int z0, int y0, int x0, int r0,
                       int r1, int r2, float* out, void* stream) {
  MMSEG_REQUIRE(n >= 0 && n < N, "window_accum: sample %d out of range", n);
  WinGeom g{N, C, D, H, W, r0, r1, r2};
  MMSEG_LAUNCH(window_accum_kernel, dim3(grid_for((long long)C * r0 * r1 * r2)), dim3(256), 0,
                     (hipStream_t)stream, logits, g, n, z0, y0, x0, out);
  return mmseg::check_launch("window_accum");
}

int mmseg_window_norm(float* out, int N, int C, int D, int H, int W, const float* cz, const float* cy, const float* cx,
                      void* stream) {
  WinGeom g{N, C, D, H, W, 1, 1, 1};
  MMSEG_LAUNCH(window_norm_kernel, dim3(grid_for((long long)N * C * D * H * W)), dim3(256), 0,
                     (hipStream_t)stream, out, g, cz, cy, cx);
  return mmseg::check_launch("window_norm");
}

int mmseg_window_gather_flip(const float* vol, int N, int C, int D, int H, int W, const int* win, int nw, int r0,
                             int r1, int r2, int flip, float* out, void* stream) {
  MMSEG_REQUIRE(vol != nullptr && win != nullptr && out != nullptr, "window_gather_flip: vol, win and out");
  MMSEG_REQUIRE(nw >= 1 && r0 > 0 && r1 > 0 && r2 > 0, "window_gather_flip: empty window set");
  MMSEG_REQUIRE(N >= 1 && C >= 1 && D >= 1 && H >= 1 && W >= 1, "window_gather_flip: empty volume");
  MMSEG_REQUIRE((flip & ~7) == 0, "window_gather_flip: flip mask %d has bits above 2", flip);
  WinGeom g{N, C, D, H, W, r0, r1, r2};
  MMSEG_LAUNCH(window_gather_flip_kernel, dim3(grid_for((long long)nw * C * r0 * r1 * r2)), dim3(256), 0,
               (hipStream_t)stream, vol, g, win, nw, flip, out);
  return mmseg::check_launch("window_gather_flip");
}

int mmseg_tta_accum(const float* pred, long long rows, int r0, int r1, int r2, int flip, int assign, float scale,
                    float* acc, void* stream) {
  MMSEG_REQUIRE(pred != nullptr && acc != nullptr && pred != acc, "tta_accum: pred and acc, out of place");
  MMSEG_REQUIRE(rows >= 1 && r0 > 0 && r1 > 0 && r2 > 0, "tta_accum: empty window set");
  MMSEG_REQUIRE((flip & ~7) == 0, "tta_accum: flip mask %d has bits above 2", flip);
  MMSEG_LAUNCH(tta_accum_kernel, dim3(grid_for(rows * r0 * r1 * r2)), dim3(256), 0, (hipStream_t)stream, pred, rows,
               r0, r1, r2, flip, assign != 0, scale, acc);
  return mmseg::check_launch("tta_accum");
}

int mmseg_window_blend(const float* pred, int N, int C, int D, int H, int W, const int* win_host, int nw, int r0,
                       int r1, int r2, int blend, const float* gz, const float* gy, const float* gx, float wmin,
                       float* out, float* count, void* stream) {
  MMSEG_REQUIRE(pred != nullptr && out != nullptr && count != nullptr && win_host != nullptr,
                "window_blend: pred, win_host, out and count");
  MMSEG_REQUIRE(nw >= 1 && r0 > 0 && r1 > 0 && r2 > 0, "window_blend: empty window set");
  MMSEG_REQUIRE(N >= 1 && C >= 1 && D >= 1 && H >= 1 && W >= 1, "window_blend: empty volume");
  MMSEG_REQUIRE((long long)r0 * r1 * r2 < (1LL << 30), "window_blend: roi %d x %d x %d is too large", r0, r1, r2);
  MMSEG_REQUIRE(blend == 0 || blend == 1, "window_blend: blend is 0 (constant) or 1 (gaussian), got %d", blend);
  MMSEG_REQUIRE(blend == 0 || (gz != nullptr && gy != nullptr && gx != nullptr),
                "window_blend: gaussian blending needs the three weight tables");
  bool vec = W % 4 == 0 && r2 % 4 == 0 && aligned16(pred) && aligned16(out) && aligned16(count);
  for (int k = 0; k < nw; ++k) {
    const int* s = win_host + 4 * k;
    MMSEG_REQUIRE(s[0] >= 0 && s[0] < N, "window_blend: window %d: sample %d out of range", k, s[0]);
    // a window lies within one roi of the volume (padding), which also keeps start + roi inside an int
    MMSEG_REQUIRE(s[1] > -r0 && s[1] < D && s[2] > -r1 && s[2] < H && s[3] > -r2 && s[3] < W,
                  "window_blend: window %d at (%d, %d, %d) does not touch the volume", k, s[1], s[2], s[3]);
    vec = vec && s[3] % 4 == 0;
  }
  WinGeom g{N, C, D, H, W, r0, r1, r2};
  const long long groups = (long long)r0 * r1 * (vec ? r2 / 4 : r2);
  // more windows than one launch carries: consecutive launches keep the window order
  for (int k0 = 0; k0 < nw; k0 += BLEND_MAXW) {
    const int nk = nw - k0 < BLEND_MAXW ? nw - k0 : BLEND_MAXW;
    BlendWins a = {};
    for (int k = 0; k < nk; ++k) {
      const int* s = win_host + 4 * (k0 + k);
      a.n[k] = s[0], a.z0[k] = s[1], a.y0[k] = s[2], a.x0[k] = s[3];
    }
    const float* p = pred + (long long)k0 * C * r0 * r1 * r2;
    const dim3 grid(grid_for(groups), nk);
    if (vec)
      MMSEG_LAUNCH(window_blend_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, p, g, a, nk, blend, gz, gy, gx, wmin,
                   out, count);
    else
      MMSEG_LAUNCH(window_blend_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p, g, a, nk, blend, gz, gy, gx, wmin,
                   out, count);
  }
  return mmseg::check_launch("window_blend");
}

int mmseg_window_finish(float* out, const float* count, int N, int C, long long V, void* stream) {
  MMSEG_REQUIRE(out != nullptr && count != nullptr, "window_finish: out and count");
  MMSEG_REQUIRE(N >= 1 && C >= 1 && V >= 1, "window_finish: empty volume");
  if (V % 4 == 0 && aligned16(out) && aligned16(count))
    MMSEG_LAUNCH(window_finish_kernel<4>, dim3(grid_for((long long)N * C * (V / 4))), dim3(256), 0, (hipStream_t)stream,
                 out, count, N, C, V);
  else
    MMSEG_LAUNCH(window_finish_kernel<1>, dim3(grid_for((long long)N * C * V)), dim3(256), 0, (hipStream_t)stream, out,
                 count, N, C, V);
  return mmseg::check_launch("window_finish");
}

int mmseg_blend_argmax_encode(const float* out, const float* count, int C, int X, int Y, int Z, unsigned char* mask,
                              void* stream) {
  MMSEG_REQUIRE(out != nullptr && count != nullptr && mask != nullptr, "blend_argmax_encode: out, count and mask");
  MMSEG_REQUIRE(C >= 1 && C <= 255, "blend_argmax_encode: 1 <= C <= 255 for a uint8 mask (got %d)", C);
  MMSEG_REQUIRE(X >= 1 && Y >= 1 && Z >= 1, "blend_argmax_encode: empty volume %d x %d x %d", X, Y, Z);
  const long long blocks = (long long)ceil_div(X, AT) * ceil_div(Z, AT) * Y;
  MMSEG_REQUIRE(blocks <= 0x7fffffffLL, "blend_argmax_encode: volume %d x %d x %d has too many tiles for one launch", X,
                Y, Z);
  MMSEG_LAUNCH(blend_argmax_kernel, dim3((unsigned)blocks), dim3(AT * AW), 0, (hipStream_t)stream, out, count, C, X, Y,
               Z, ceil_div(Z, AT), ceil_div(X, AT), mask);
  return mmseg::check_launch("blend_argmax_encode");
}

}  // extern "C"
