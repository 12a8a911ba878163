// Training-side patch sampler: foreground-biased crops with rotation and scaling, drawn from a volume that is
// resident on the device (data/patch.py).  The reference has RandomCrop / CenterCrop (src/data/transforms.py:
// 142-212) and promises random_rotate / random_scale in its default.yaml without running them.
//
//   fg_count      voxels with label > 0 per chunk of FG_CHUNK consecutive voxels (int32): depends on the label
//                 alone, so the caller may keep it with the volume
//   patch_pick    one wave per patch: total n of the chunk counts, k = min(floor(u n), n - 1), the chunk that holds
//                 the k-th foreground voxel from the exclusive prefix sum, the voxel inside it from a ballot /
//                 popcount scan, then the clamped crop start.  The starts stay on the device: no sync
//   patch_sample  all P patches of a volume in one launch.  affine == 0: a copy with padding (16-byte vectors along
//                 W where the source segment and the destination row are aligned and inside the volume, scalars
//                 elsewhere).  affine != 0: p = M q + c in fp64 with every product and sum rounded on its own (no FMA),
//                 trilinear over the 8 corners of floor(p) (a corner outside contributes pad_value: scipy's
//                 mode="grid-constant"), z then y then x; labels take the voxel at floor(p + 0.5)
// tests/patch_ref.py restates the pick rule and the sampler in numpy; the GPU tests hold the kernels to it bitwise.
#include "mmseg_common.h"

namespace {

constexpr int FG_CHUNK = 4096;      // voxels per count: 256 threads x one 16-byte vector of uint8 labels
constexpr int PATCH_MAXP = 16, PATCH_MAXC = 4;

template <typename L, int VN>
struct alignas(16) LabVec {
  L v[VN];
};

// one block per chunk; VEC: the label pointer is 16-byte aligned, so every full chunk reads 16-byte vectors
template <typename L, bool VEC>
__global__ __launch_bounds__(256) void fg_count_kernel(const L* __restrict__ label, long long V,
                                                       int* __restrict__ counts) {
  constexpr int VN = 16 / (int)sizeof(L);
  __shared__ int red[4];
  const long long base = (long long)blockIdx.x * FG_CHUNK;
  int c = 0;
  if (VEC && base + FG_CHUNK <= V) {
    const LabVec<L, VN>* p = reinterpret_cast<const LabVec<L, VN>*>(label + base);
    for (int j = threadIdx.x; j < FG_CHUNK / VN; j += 256) {
      const LabVec<L, VN> a = p[j];
#pragma unroll
      for (int i = 0; i < VN; ++i) c += a.v[i] > 0 ? 1 : 0;
    }
  } else {
    for (int j = threadIdx.x; j < FG_CHUNK; j += 256)
      if (base + j < V) c += label[base + j] > 0 ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);    // integers: any order gives the same count
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

struct PickArgs {
  int D, H, W, P;
  int psz[3];
  int nchunks;
  int mode[PATCH_MAXP];
  double u[PATCH_MAXP];
  int fallback[PATCH_MAXP][3];
};

__device__ __forceinline__ int pick_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one wave per patch
template <typename L>
__global__ __launch_bounds__(64) void patch_pick_kernel(PickArgs a, const L* __restrict__ label,
                                                        const int* __restrict__ counts, int* __restrict__ starts) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const int n_ax[3] = {a.D, a.H, a.W};
  int st[3] = {a.fallback[p][0], a.fallback[p][1], a.fallback[p][2]};
  if (a.mode[p] == 1) {
    // lane l owns chunks [l per, (l + 1) per): its sum, then an inclusive scan over the lanes
    const int per = (a.nchunks + 63) / 64;
    const int c0 = lane * per < a.nchunks ? lane * per : a.nchunks;
    const int c1 = c0 + per < a.nchunks ? c0 + per : a.nchunks;
    long long mine = 0;
    for (int c = c0; c < c1; ++c) mine += counts[c];
    long long incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    const long long n = __shfl(incl, 63, 64);
    if (n > 0) {
      long long k = (long long)floor(a.u[p] * (double)n);
      if (k > n - 1) k = n - 1;
      if (k < 0) k = 0;
      // the one lane whose range of the prefix sum holds k walks its chunks
      const long long excl = incl - mine;
      const bool owner = excl <= k && k < incl;
      int chunk = 0;
      long long rem = 0;
      if (owner) {
        long long before = excl;
        int c = c0;
        while (c < c1 - 1 && before + counts[c] <= k) before += counts[c++];
        chunk = c;
        rem = k - before;
      }
      const unsigned long long who = __ballot(owner);
      const int src = who ? __ffsll((long long)who) - 1 : 0;
      chunk = __shfl(chunk, src, 64);
      int r = (int)__shfl(rem, src, 64);
      // the r-th foreground voxel of the chunk: 64 voxels per step, in row-major order
      const long long V = (long long)a.D * a.H * a.W;
      const long long base = (long long)chunk * FG_CHUNK;
      long long found = -1;
      for (int it = 0; it < FG_CHUNK / 64; ++it) {
        const long long i = base + it * 64 + lane;
        const bool fg = i < V && label[i] > 0;
        const unsigned long long m = __ballot(fg);
        const int cnt = __popcll(m);
        if (r < cnt) {
          const int below = __popcll(m & ((1ull << lane) - 1ull));
          const unsigned long long hit = __ballot(fg && below == r);
          found = base + it * 64 + (__ffsll((long long)hit) - 1);
          break;
        }
        r -= cnt;
      }
      if (found >= 0) {      // always, when the counts belong to this label
        const int v[3] = {(int)(found / ((long long)a.H * a.W)), (int)((found / a.W) % a.H), (int)(found % a.W)};
#pragma unroll
        for (int x = 0; x < 3; ++x)
          if (n_ax[x] >= a.psz[x]) st[x] = pick_clamp(v[x] - a.psz[x] / 2, 0, n_ax[x] - a.psz[x]);
      }
    }
  }
#pragma unroll
  for (int x = 0; x < 3; ++x)
    if (n_ax[x] < a.psz[x]) st[x] = -((a.psz[x] - n_ax[x]) / 2);     // the volume centred in the patch
  if (lane < 3) starts[p * 3 + lane] = lane == 0 ? st[0] : (lane == 1 ? st[1] : st[2]);
}

struct SampleArgs {
  int C, D, H, W, P;
  int pd, ph, pw;
  int affine[PATCH_MAXP];
  double M[PATCH_MAXP][9];
  float pad[PATCH_MAXC];
};

// One output row of a plain crop: d[x] = s[sx + x] where 0 <= sx + x < W, fill elsewhere (row_ok false: the whole
// row lies outside the volume).  s points at the source row's first voxel.
template <typename T>
__device__ __forceinline__ void copy_row(const T* __restrict__ s, bool row_ok, int sx, int W, T* __restrict__ d,
                                         int pw, T fill) {
  constexpr int VN = 16 / (int)sizeof(T);
  typedef LabVec<T, VN> Vec;
  int nv = pw / VN;
  const bool aligned = row_ok && !(((uintptr_t)s + (long long)sx * (long long)sizeof(T)) & 15) &&
                       !(((uintptr_t)d) & 15);
  if (!aligned) nv = 0;
  for (int j = threadIdx.x; j < nv; j += blockDim.x) {
    const int x0 = sx + j * VN;
    Vec o;
    if (x0 >= 0 && x0 + VN <= W) {
      o = *reinterpret_cast<const Vec*>(s + x0);
    } else {
#pragma unroll
      for (int i = 0; i < VN; ++i) o.v[i] = (x0 + i >= 0 && x0 + i < W) ? s[x0 + i] : fill;
    }
    *reinterpret_cast<Vec*>(d + j * VN) = o;
  }
  for (int x = nv * VN + threadIdx.x; x < pw; x += blockDim.x) {
    const int xs = sx + x;
    d[x] = (row_ok && xs >= 0 && xs < W) ? s[xs] : fill;
  }
}

__device__ __forceinline__ double patch_lerp(double a, double b, double w0, double w1) {
  // plain operators under the pragma: __dadd_rn / __dmul_rn are inline functions around + and * that carry the
  // translation unit's contraction mode, so the compiler fuses them into one FMA after inlining
#pragma clang fp contract(off)
  return a * w0 + b * w1;
}

// source coordinate of output offset o along axis a: ((M[a][0] q0 + M[a][1] q1) + M[a][2] q2) + c_a
__device__ __forceinline__ double patch_coord(const double* __restrict__ m, double q0, double q1, double q2,
                                              double c) {
#pragma clang fp contract(off)
  return ((m[0] * q0 + m[1] * q1) + m[2] * q2) + c;
}

struct Corner {
  int i0;          // floor(p), held to [-2, n] so that both corners of anything outside stay outside
  double w0, w1;   // 1 - t, t with t = p - floor(p)
};

__device__ __forceinline__ Corner patch_corner(double p, int n) {
  Corner k;
  const double fl = floor(p);
  const double t = p - fl;
  k.w1 = t;
  k.w0 = 1.0 - t;
  k.i0 = fl >= (double)n ? n : (fl >= -2.0 ? (int)fl : -2);     // NaN: -2, everything outside
  return k;
}

// block (tx, ty): ty output rows (od, oh) per block, tx threads along each; blockIdx.y = channel, or C for the
// label; blockIdx.z = patch
template <typename L>
__global__ void patch_sample_kernel(SampleArgs a, const float* __restrict__ src, const L* __restrict__ lsrc,
                                    const int* __restrict__ starts, float* __restrict__ dst,
                                    L* __restrict__ ldst) {
  const int r = blockIdx.x * blockDim.y + threadIdx.y;
  if (r >= a.pd * a.ph) return;
  const int od = r / a.ph, oh = r - od * a.ph;
  const int p = blockIdx.z, c = blockIdx.y;
  const int sz = starts[p * 3], sy = starts[p * 3 + 1], sx = starts[p * 3 + 2];
  const long long pvox = (long long)a.pd * a.ph * a.pw;
  const long long plane = (long long)a.D * a.H * a.W;
  const long long drow = (long long)r * a.pw;
  const bool is_label = c == a.C;
  if (!a.affine[p]) {
    const int z = sz + od, y = sy + oh;
    const bool ok = z >= 0 && z < a.D && y >= 0 && y < a.H;
    const long long srow = ok ? ((long long)z * a.H + y) * a.W : 0;
    if (is_label)
      copy_row<L>(lsrc + srow, ok, sx, a.W, ldst + p * pvox + drow, a.pw, (L)0);
    else
      copy_row<float>(src + c * plane + srow, ok, sx, a.W, dst + ((long long)p * a.C + c) * pvox + drow, a.pw,
                      a.pad[c]);
    return;
  }
  const double* m = a.M[p];
  const double hz = (double)(a.pd - 1) * 0.5, hy = (double)(a.ph - 1) * 0.5, hx = (double)(a.pw - 1) * 0.5;
  const double cz = (double)sz + hz, cy = (double)sy + hy, cx = (double)sx + hx;     // exact: half-integers
  const double q0 = (double)od - hz, q1 = (double)oh - hy;
  for (int ox = threadIdx.x; ox < a.pw; ox += blockDim.x) {
    const double q2 = (double)ox - hx;
    const double pz = patch_coord(m, q0, q1, q2, cz), py = patch_coord(m + 3, q0, q1, q2, cy),
                 px = patch_coord(m + 6, q0, q1, q2, cx);
    if (is_label) {
      const double fz = floor(pz + 0.5), fy = floor(py + 0.5), fx = floor(px + 0.5);
      L v = (L)0;
      if (fz >= 0.0 && fz < (double)a.D && fy >= 0.0 && fy < (double)a.H && fx >= 0.0 && fx < (double)a.W)
        v = lsrc[((long long)(int)fz * a.H + (int)fy) * a.W + (int)fx];
      ldst[p * pvox + drow + ox] = v;
      continue;
    }
    const Corner kz = patch_corner(pz, a.D), ky = patch_corner(py, a.H), kx = patch_corner(px, a.W);
    const float* s = src + c * plane;
    const double pad = (double)a.pad[c];
    auto at = [&](int z, int y, int x) {
      return (z >= 0 && z < a.D && y >= 0 && y < a.H && x >= 0 && x < a.W)
                 ? (double)s[((long long)z * a.H + y) * a.W + x] : pad;
    };
    // axis 0 (z) first, then y, then x: the restatement's order
    double vy[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        vy[i][j] = patch_lerp(at(kz.i0, ky.i0 + i, kx.i0 + j), at(kz.i0 + 1, ky.i0 + i, kx.i0 + j), kz.w0, kz.w1);
    const double vx0 = patch_lerp(vy[0][0], vy[1][0], ky.w0, ky.w1);
    const double vx1 = patch_lerp(vy[0][1], vy[1][1], ky.w0, ky.w1);
    dst[((long long)p * a.C + c) * pvox + drow + ox] = (float)patch_lerp(vx0, vx1, kx.w0, kx.w1);
  }
}

}  // namespace

extern "C" {

int mmseg_fg_chunks(long long V) { return V >= 1 && V <= 0x7fffffffLL * 64 ? ceil_div(V, FG_CHUNK) : 0; }

int mmseg_fg_count(const void* label, int label_bytes, int D, int H, int W, int* counts, void* stream) {
  MMSEG_REQUIRE(D >= 1 && H >= 1 && W >= 1, "fg_count: empty shape");
  MMSEG_REQUIRE(label_bytes == 8 || label_bytes == 1, "fg_count: int64 or uint8 labels");
  MMSEG_REQUIRE(label != nullptr && counts != nullptr, "fg_count: label and counts");
  const long long V = (long long)D * H * W;
  const int nch = mmseg_fg_chunks(V);
  MMSEG_REQUIRE(nch >= 1, "fg_count: oversized volume");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = !(((uintptr_t)label) & 15);
#define FG_LAUNCH(L, VEC) \
  MMSEG_LAUNCH((fg_count_kernel<L, VEC>), dim3(nch), dim3(256), 0, s, (const L*)label, V, counts)
  if (label_bytes == 8) {
    if (vec) FG_LAUNCH(int64_t, true); else FG_LAUNCH(int64_t, false);
  } else {
    if (vec) FG_LAUNCH(uint8_t, true); else FG_LAUNCH(uint8_t, false);
  }
#undef FG_LAUNCH
  return mmseg::check_launch("fg_count");
}

int mmseg_patch_pick(const void* label, int label_bytes, int D, int H, int W, const int* counts, int P, int pd,
                     int ph, int pw, const int* mode, const double* u, const int* fallback_start, int* starts,
                     void* stream) {
  MMSEG_REQUIRE(D >= 1 && H >= 1 && W >= 1 && pd >= 1 && ph >= 1 && pw >= 1, "patch_pick: empty shape");
  MMSEG_REQUIRE(P >= 1 && P <= PATCH_MAXP, "patch_pick: 1 <= patches <= %d (got %d)", PATCH_MAXP, P);
  MMSEG_REQUIRE(label_bytes == 8 || label_bytes == 1, "patch_pick: int64 or uint8 labels");
  MMSEG_REQUIRE(mode != nullptr && u != nullptr && fallback_start != nullptr && starts != nullptr,
                "patch_pick: mode, u, fallback_start and starts");
  PickArgs a{};
  a.D = D; a.H = H; a.W = W; a.P = P;
  a.psz[0] = pd; a.psz[1] = ph; a.psz[2] = pw;
  a.nchunks = mmseg_fg_chunks((long long)D * H * W);
  MMSEG_REQUIRE(a.nchunks >= 1, "patch_pick: oversized volume");
  const int n_ax[3] = {D, H, W};
  bool any_fg = false;
  for (int p = 0; p < P; ++p) {
    MMSEG_REQUIRE(mode[p] == 0 || mode[p] == 1, "patch_pick: mode 0 (fallback start) or 1 (foreground), got %d",
                  mode[p]);
    MMSEG_REQUIRE(u[p] >= 0.0 && u[p] < 1.0, "patch_pick: u in [0, 1) (got %g)", u[p]);
    a.mode[p] = mode[p];
    a.u[p] = u[p];
    any_fg |= mode[p] == 1;
    for (int x = 0; x < 3; ++x) {
      const int f = fallback_start[p * 3 + x];
      MMSEG_REQUIRE(n_ax[x] < a.psz[x] || (f >= 0 && f <= n_ax[x] - a.psz[x]),
                    "patch_pick: fallback_start[%d][%d] = %d leaves the volume", p, x, f);
      a.fallback[p][x] = f;
    }
  }
  MMSEG_REQUIRE(!any_fg || (label != nullptr && counts != nullptr), "patch_pick: mode 1 needs the label and its counts");
  hipStream_t s = (hipStream_t)stream;
  if (label_bytes == 8)
    MMSEG_LAUNCH(patch_pick_kernel<int64_t>, dim3(P), dim3(64), 0, s, a, (const int64_t*)label, counts, starts);
  else
    MMSEG_LAUNCH(patch_pick_kernel<uint8_t>, dim3(P), dim3(64), 0, s, a, (const uint8_t*)label, counts, starts);
  return mmseg::check_launch("patch_pick");
}

int mmseg_patch_sample(const float* src, int C, int D, int H, int W, const void* label, int label_bytes,
                       const int* starts, int P, int pd, int ph, int pw, const int* affine, const double* M,
                       const float* pad_value, float* dst, void* label_dst, void* stream) {
  MMSEG_REQUIRE(C >= 1 && C <= PATCH_MAXC, "patch_sample: 1 <= channels <= %d (got %d)", PATCH_MAXC, C);
  MMSEG_REQUIRE(D >= 1 && H >= 1 && W >= 1 && pd >= 1 && ph >= 1 && pw >= 1 && (long long)pd * ph <= 0x7fffffffLL,
                "patch_sample: empty or oversized shape");
  MMSEG_REQUIRE(P >= 1 && P <= PATCH_MAXP, "patch_sample: 1 <= patches <= %d (got %d)", PATCH_MAXP, P);
  MMSEG_REQUIRE(src != nullptr && dst != nullptr && src != dst, "patch_sample: src and dst, out of place");
  MMSEG_REQUIRE(starts != nullptr && affine != nullptr && pad_value != nullptr,
                "patch_sample: starts, affine and pad_value");
  if (label != nullptr) {
    MMSEG_REQUIRE(label_bytes == 8 || label_bytes == 1, "patch_sample: int64 or uint8 labels");
    MMSEG_REQUIRE(label_dst != nullptr && label_dst != label, "patch_sample: label_dst, out of place");
  }
  SampleArgs a{};
  a.C = C; a.D = D; a.H = H; a.W = W; a.P = P;
  a.pd = pd; a.ph = ph; a.pw = pw;
  for (int p = 0; p < P; ++p) {
    a.affine[p] = affine[p] != 0;
    if (a.affine[p]) {
      MMSEG_REQUIRE(M != nullptr, "patch_sample: an affine patch needs its matrix");
      for (int k = 0; k < 9; ++k) {
        MMSEG_REQUIRE(M[p * 9 + k] == M[p * 9 + k] && M[p * 9 + k] < 1e6 && M[p * 9 + k] > -1e6,
                      "patch_sample: M[%d][%d] is not a finite rotation / scale entry", p, k);
        a.M[p][k] = M[p * 9 + k];
      }
    }
  }
  for (int c = 0; c < C; ++c) a.pad[c] = pad_value[c];
  // threads along a row: one per 16-byte vector when rows can be vectors at all, else one per element
  const int per_row = pw % 4 == 0 ? pw / 4 : pw;
  const int tx = per_row < 256 ? per_row : 256, ty = 256 / tx;
  const dim3 block(tx, ty), grid(ceil_div((long long)pd * ph, ty), C + (label != nullptr ? 1 : 0), P);
  hipStream_t s = (hipStream_t)stream;
  if (label_bytes == 1 && label != nullptr)
    MMSEG_LAUNCH(patch_sample_kernel<uint8_t>, grid, block, 0, s, a, src, (const uint8_t*)label, starts, dst,
                 (uint8_t*)label_dst);
  else
    MMSEG_LAUNCH(patch_sample_kernel<int64_t>, grid, block, 0, s, a, src, (const int64_t*)label, starts, dst,
                 (int64_t*)label_dst);
  return mmseg::check_launch("patch_sample");
}

}  // extern "C"
