// Boundary and confusion metrics on the device (reference src/trainer/metrics.py:91-226):
//   - exact Euclidean distance transform (scipy.ndimage.distance_transform_edt(~fg, sampling)), separable:
//     a scan along the contiguous axis, then two brute-force lower-envelope passes that carry the winning
//     INTEGER offsets, and one fp64 evaluation in scipy's order at the end;
//   - HausdorffDistance.update: roll-border extraction (np.roll(m, 1, axis=0), wrap included), gather of the
//     distances at the border voxels, and the two order statistics np.percentile interpolates between, by a
//     radix select over the fp64 bit patterns (no sort);
//   - ConfusionMatrix.update: exact int64 counts.
// Masks are [B][H][W][D] int64 or uint8, D contiguous; foreground = value > 0.  No float atomics anywhere.
#include "mmseg_common.h"

#include <math.h>

namespace {

constexpr int CMAX = 16;
constexpr int EDT_NONE = -1;      // "no foreground voxel in this line" offset sentinel
constexpr int ENV_TJ = 32;        // lines per block (consecutive in memory)
constexpr int ENV_TL = 8;         // output positions per block and step
constexpr int ENV_CH = 128;       // line positions staged in LDS at once
constexpr int SEL_BLOCKS = 128;   // blocks per sample of the select passes

struct short2_t {
  int16_t a, b;
};

// ------------------------------------------------------------------ distance transform
// pass 1: offset to the nearest foreground voxel along D of each line (b, h, w).  A block stages as many whole
// lines as it has threads for (one line when D >= blockDim.x) and each thread scans outwards within its line.
template <typename MT>
__global__ void edt_scan_kernel(const MT* __restrict__ mask, int D, long long lines, int16_t* __restrict__ o2) {
  extern __shared__ unsigned char fg[];
  const int nl = D >= (int)blockDim.x ? 1 : (int)blockDim.x / D;
  for (long long l0 = (long long)blockIdx.x * nl; l0 < lines; l0 += (long long)gridDim.x * nl) {
    const int cnt = (int)(lines - l0 < nl ? lines - l0 : nl) * D;
    const MT* m = mask + l0 * D;
    for (int e = threadIdx.x; e < cnt; e += blockDim.x) fg[e] = m[e] > 0 ? 1 : 0;
    __syncthreads();
    for (int e = threadIdx.x; e < cnt; e += blockDim.x) {
      const int ln = e / D, d = e - ln * D;
      const unsigned char* f = fg + ln * D;
      int o = EDT_NONE;
      for (int k = 0; k < D; ++k) {
        const bool lo_in = d - k >= 0, hi_in = d + k < D;
        if (!lo_in && !hi_in) break;
        if ((lo_in && f[d - k]) || (hi_in && f[d + k])) {
          o = k;
          break;
        }
      }
      o2[l0 * D + e] = (int16_t)o;
    }
    __syncthreads();
  }
}

// passes 2 and 3: lower envelope along one strided axis.  Element (outer, l, j) at (outer * L + l) * S + j,
// j in [0, S) contiguous.  PASS 2 (axis W, L = W, S = D): in = o2, out = (o1, o2).  PASS 3 (axis H, L = H,
// S = W * D): in = (o1, o2), out = the distance, formed once from the three winning offsets.
template <int PASS>
__global__ void __launch_bounds__(ENV_TJ* ENV_TL)
    edt_env_kernel(const void* __restrict__ in_, void* __restrict__ out_, int L, long long S, long long jtiles,
                   double s0, double s1, double s2) {
#pragma clang fp contract(off)
  __shared__ double carried[ENV_CH][ENV_TJ];
  const int16_t* in2 = (const int16_t*)in_;
  const short2_t* in3 = (const short2_t*)in_;
  const long long tile = blockIdx.x;
  const long long outer = tile / jtiles, jt = tile - outer * jtiles;
  const int tj = threadIdx.x % ENV_TJ, tl = threadIdx.x / ENV_TJ;
  const long long j = jt * ENV_TJ + tj;
  const bool jok = j < S;
  const long long base = outer * L * S + j;
  const double sa = PASS == 2 ? s1 : s0;
  const bool single = L <= ENV_CH;
  for (int lo0 = 0; lo0 < L; lo0 += ENV_TL) {
    const int lo = lo0 + tl;
    double best = INFINITY;
    int bl = -1;
    for (int c0 = 0; c0 < L; c0 += ENV_CH) {
      if (!single || lo0 == 0) {
        __syncthreads();
        for (int r = tl; r < ENV_CH; r += ENV_TL) {
          const int l = c0 + r;
          double v = INFINITY;
          if (l < L && jok) {
            if (PASS == 2) {
              const int o = in2[base + l * S];
              if (o >= 0) {
                const double t = (double)o * s2;
                v = t * t;
              }
            } else {
              const short2_t o = in3[base + l * S];
              if (o.a >= 0) {
                const double t1 = (double)o.a * s1, t2 = (double)o.b * s2;
                v = t1 * t1 + t2 * t2;
              }
            }
          }
          carried[r][tj] = v;
        }
        __syncthreads();
      }
      const int cn = L - c0 < ENV_CH ? L - c0 : ENV_CH;
      if (lo < L) {
        for (int r = 0; r < cn; ++r) {
          const double dl = (double)(c0 + r - lo) * sa;
          const double cand = dl * dl + carried[r][tj];
          if (cand < best) {
            best = cand;
            bl = c0 + r;
          }
        }
      }
    }
    if (lo < L && jok) {
      const long long oi = base + lo * S;
      const int oa = bl < 0 ? 0 : (bl > lo ? bl - lo : lo - bl);
      if (PASS == 2) {
        short2_t w;
        w.a = (int16_t)EDT_NONE;
        w.b = (int16_t)EDT_NONE;
        if (bl >= 0) {
          w.a = (int16_t)oa;
          w.b = in2[base + bl * S];
        }
        ((short2_t*)out_)[oi] = w;
      } else {
        double d = INFINITY;
        if (bl >= 0) {
          const short2_t o = in3[base + bl * S];
          const double t0 = (double)oa * s0, t1 = (double)o.a * s1, t2 = (double)o.b * s2;
          d = sqrt(((t0 * t0) + (t1 * t1)) + (t2 * t2));   // scipy: sum over the axes in order, then sqrt
        }
        ((double*)out_)[oi] = d;
      }
    }
  }
}

inline long long align256(long long x) { return (x + 255) / 256 * 256; }

struct EdtWs {
  int16_t* o2;
  short2_t* o12;
  long long bytes;
};
EdtWs edt_ws(void* ws, long long N) {
  EdtWs e;
  char* p = (char*)ws;
  e.o2 = (int16_t*)p;
  e.o12 = (short2_t*)(p + align256(N * 2));
  e.bytes = align256(N * 2) + align256(N * 4);
  return e;
}

int edt_check(const char* who, int mask_bytes, int B, int H, int W, int D) {
  MMSEG_REQUIRE(mask_bytes == 1 || mask_bytes == 8, "%s: masks are uint8 or int64", who);
  MMSEG_REQUIRE(B >= 1 && H >= 1 && W >= 1 && D >= 1 && H <= 32767 && W <= 32767 && D <= 32767,
                "%s: every dim in [1, 32767]", who);
  MMSEG_REQUIRE((long long)H * W * D < (1ll << 30), "%s: at most 2^30 - 1 voxels per sample", who);
  const long long tiles2 = (long long)B * H * (((long long)D + ENV_TJ - 1) / ENV_TJ);
  const long long tiles3 = (long long)B * (((long long)W * D + ENV_TJ - 1) / ENV_TJ);
  MMSEG_REQUIRE(tiles2 < (1ll << 31) && tiles3 < (1ll << 31), "%s: batch too large for one launch", who);
  return 0;
}

// the three passes of one mask; out [B][H][W][D] fp64 (+inf everywhere in a sample without foreground)
template <typename MT>
void edt_run(const MT* mask, int B, int H, int W, int D, double s0, double s1, double s2, double* out,
             const EdtWs& e, hipStream_t s) {
  const long long lines = (long long)B * H * W;
  const int nl = D >= 256 ? 1 : 256 / D;                          // as the kernel derives it from its 256 threads
  const long long blocks1 = (lines + nl - 1) / nl;
  const int grid1 = (int)(blocks1 < (1ll << 20) ? blocks1 : (1ll << 20));
  MMSEG_LAUNCH(edt_scan_kernel<MT>, dim3(grid1), dim3(256), (size_t)nl * D, s, mask, D, lines, e.o2);
  const long long jt2 = ((long long)D + ENV_TJ - 1) / ENV_TJ;
  MMSEG_LAUNCH(edt_env_kernel<2>, dim3((unsigned)((long long)B * H * jt2)), dim3(ENV_TJ * ENV_TL), 0, s,
               (const void*)e.o2, (void*)e.o12, W, (long long)D, jt2, s0, s1, s2);
  const long long S3 = (long long)W * D, jt3 = (S3 + ENV_TJ - 1) / ENV_TJ;
  MMSEG_LAUNCH(edt_env_kernel<3>, dim3((unsigned)((long long)B * jt3)), dim3(ENV_TJ * ENV_TL), 0, s,
               (const void*)e.o12, (void*)out, H, S3, jt3, s0, s1, s2);
}

// ------------------------------------------------------------------ border + gather
// ctr[b]: number of distances appended to buf[b][0 .. 2V).  grid (blocks, B): sample b = blockIdx.y, so the voxel
// index within the sample stays in 32 bits.  One slot-counter atomic per wave, its lanes placed by ballots.
template <typename PT, typename TT>
__global__ void hd_gather_kernel(const PT* __restrict__ pred, const TT* __restrict__ target,
                                 const double* __restrict__ dist_pred, const double* __restrict__ dist_target, int H,
                                 unsigned int WD, unsigned int V, double* __restrict__ buf,
                                 unsigned int* __restrict__ ctr) {
  const long long b = blockIdx.y, off = b * V;
  const unsigned int lane = threadIdx.x & 63u;
  const unsigned long long below = (1ull << lane) - 1ull;
  double* out = buf + 2 * off;
  for (unsigned int r0 = blockIdx.x * blockDim.x + (threadIdx.x - lane); r0 < V; r0 += gridDim.x * blockDim.x) {
    const unsigned int r = r0 + lane;
    bool pb = false, tb = false;
    const long long i = off + r;
    if (r < V) {
      const unsigned int h = r / WD;
      // np.roll(m, 1, axis=0): row h - 1, row 0 against row H - 1
      const long long ip = h == 0 ? i + (long long)(H - 1) * WD : i - (long long)WD;
      pb = (pred[i] > 0) != (pred[ip] > 0);
      tb = (target[i] > 0) != (target[ip] > 0);
    }
    const unsigned long long mp = __ballot(pb), mt = __ballot(tb);
    const int nwave = __popcll(mp) + __popcll(mt);
    unsigned int base = 0;
    if (lane == 0 && nwave) base = atomicAdd(&ctr[b], (unsigned int)nwave);
    base = __shfl(base, 0, 64);
    unsigned int slot = base + (unsigned int)(__popcll(mp & below) + __popcll(mt & below));
    if (pb) out[slot++] = dist_target[i];
    if (tb) out[slot] = dist_pred[i];
  }
}

// ------------------------------------------------------------------ rank selection
struct HdState {
  unsigned long long prefix, k, n, lo, cnt_le, min_gt;
  unsigned int hist[256];
};

__global__ void hd_sel_init_kernel(const unsigned int* __restrict__ ctr, double qfrac, HdState* __restrict__ st) {
#pragma clang fp contract(off)
  HdState& s = st[blockIdx.x];
  s.hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    const unsigned long long n = ctr[blockIdx.x];
    unsigned long long lo = 0;
    if (n > 0) {
      // numpy's "linear" virtual index (n - 1) * (q / 100); at or above n - 1 it takes the last element
      const double vi = (double)(n - 1) * qfrac;
      lo = vi >= (double)(n - 1) ? n - 1 : (unsigned long long)floor(vi);
    }
    s.prefix = 0;
    s.k = lo;
    s.n = n;
    s.lo = lo;
    s.cnt_le = 0;
    s.min_gt = ~0ull;
  }
}

// histogram of the digit at `shift` over the keys whose higher digits equal the prefix found so far
__global__ void hd_sel_hist_kernel(const double* __restrict__ buf, long long V, int shift, HdState* __restrict__ st) {
  __shared__ unsigned int lh[256];
  HdState& s = st[blockIdx.y];
  const unsigned long long* keys = (const unsigned long long*)(buf + (long long)blockIdx.y * 2 * V);
  const unsigned long long n = s.n, prefix = s.prefix;
  lh[threadIdx.x] = 0;
  __syncthreads();
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long key = keys[i];
    if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8)))
      atomicAdd(&lh[(unsigned int)(key >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (lh[threadIdx.x]) atomicAdd(&s.hist[threadIdx.x], lh[threadIdx.x]);
}

__global__ void hd_sel_pick_kernel(int shift, HdState* __restrict__ st) {
  __shared__ unsigned int lh[256];
  HdState& s = st[blockIdx.x];
  lh[threadIdx.x] = s.hist[threadIdx.x];
  __syncthreads();
  s.hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    unsigned long long k = s.k, cum = 0;
    int d = 0;
    for (; d < 255; ++d) {
      if (cum + lh[d] > k) break;
      cum += lh[d];
    }
    s.k = k >= cum ? k - cum : 0;
    s.prefix |= (unsigned long long)d << shift;
  }
}

// count(keys <= a_lo) and min(keys > a_lo)
__global__ void hd_sel_hi_kernel(const double* __restrict__ buf, long long V, HdState* __restrict__ st) {
  __shared__ unsigned int lcnt;
  __shared__ unsigned long long lmin;
  HdState& s = st[blockIdx.y];
  const unsigned long long* keys = (const unsigned long long*)(buf + (long long)blockIdx.y * 2 * V);
  const unsigned long long n = s.n, alo = s.prefix;
  if (threadIdx.x == 0) {
    lcnt = 0;
    lmin = ~0ull;
  }
  __syncthreads();
  unsigned int c = 0;
  unsigned long long m = ~0ull;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long key = keys[i];
    if (key <= alo) ++c;
    else if (key < m) m = key;
  }
  if (c) atomicAdd(&lcnt, c);
  if (m != ~0ull) atomicMin(&lmin, m);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (lcnt) atomicAdd(&s.cnt_le, (unsigned long long)lcnt);
    if (lmin != ~0ull) atomicMin(&s.min_gt, lmin);
  }
}

// records[b] = {n, a[lo], a[hi], skipped}
__global__ void hd_sel_final_kernel(const HdState* __restrict__ st, const double* __restrict__ dist_pred,
                                    const double* __restrict__ dist_target, long long V, int B,
                                    double* __restrict__ records) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const HdState& s = st[b];
  // a sample without foreground has no finite distance anywhere (the reference skips it, metrics.py:134)
  const bool skipped = isinf(dist_pred[b * V]) || isinf(dist_target[b * V]) || s.n == 0;
  const unsigned long long hi = s.cnt_le > s.lo + 1 || s.min_gt == ~0ull ? s.prefix : s.min_gt;
  records[b * 4 + 0] = (double)s.n;
  records[b * 4 + 1] = __longlong_as_double((long long)s.prefix);
  records[b * 4 + 2] = __longlong_as_double((long long)hi);
  records[b * 4 + 3] = skipped ? 1.0 : 0.0;
}

// ------------------------------------------------------------------ confusion matrix
// counts[t * C + p]; a pair with p or t outside [0, C) goes to *invalid instead
template <typename PT, typename LT>
__global__ void confusion_idx_kernel(const PT* __restrict__ pred, const LT* __restrict__ target, int C,
                                     long long total, unsigned long long* __restrict__ counts,
                                     unsigned long long* __restrict__ invalid) {
  __shared__ unsigned int sc[CMAX * CMAX + 1];
  for (int k = threadIdx.x; k <= C * C; k += blockDim.x) sc[k] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long p = (long long)pred[i], t = (long long)target[i];
    if (p >= 0 && p < C && t >= 0 && t < C) atomicAdd(&sc[(int)t * C + (int)p], 1u);
    else atomicAdd(&sc[C * C], 1u);
  }
  __syncthreads();
  for (int k = threadIdx.x; k <= C * C; k += blockDim.x)
    if (sc[k]) atomicAdd(k < C * C ? &counts[k] : invalid, (unsigned long long)sc[k]);
}

template <typename LT>
__global__ void confusion_logits_kernel(const float* __restrict__ logits, const LT* __restrict__ target, int C,
                                        long long V, long long total, unsigned long long* __restrict__ counts,
                                        unsigned long long* __restrict__ invalid) {
  __shared__ unsigned int sc[CMAX * CMAX + 1];
  for (int k = threadIdx.x; k <= C * C; k += blockDim.x) sc[k] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / V, v = i - n * V;
    const float* L = logits + n * C * V;
    int best = 0;
    float bv = L[v];
    for (int c = 1; c < C; ++c) {
      const float z = L[c * V + v];
      if (z > bv || (z != z && bv == bv)) {  // first maximum; NaN counts as maximal (torch.argmax), as dice_counts
        bv = z;
        best = c;
      }
    }
    const long long t = (long long)target[i];
    if (t >= 0 && t < C) atomicAdd(&sc[(int)t * C + best], 1u);
    else atomicAdd(&sc[C * C], 1u);
  }
  __syncthreads();
  for (int k = threadIdx.x; k <= C * C; k += blockDim.x)
    if (sc[k]) atomicAdd(k < C * C ? &counts[k] : invalid, (unsigned long long)sc[k]);
}

int count_grid(long long total) {
  long long b = (total + 255) / 256;
  return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

struct HdWs {
  EdtWs e;
  double *dist_pred, *dist_target, *buf;
  unsigned int* ctr;
  HdState* st;
  long long small_off, small_bytes, bytes;
};
HdWs hd_ws(void* ws, int B, long long V) {
  const long long N = (long long)B * V;
  HdWs h;
  h.e = edt_ws(ws, N);
  char* p = (char*)ws;
  long long off = h.e.bytes;
  h.dist_pred = (double*)(p + off);
  off += align256(N * 8);
  h.dist_target = (double*)(p + off);
  off += align256(N * 8);
  h.buf = (double*)(p + off);
  off += align256(2 * N * 8);
  h.small_off = off;
  h.ctr = (unsigned int*)(p + off);
  off += align256((long long)B * 4);
  h.st = (HdState*)(p + off);
  off += align256((long long)B * (long long)sizeof(HdState));
  h.small_bytes = off - h.small_off;
  h.bytes = off;
  return h;
}

}  // namespace

extern "C" {

long long mmseg_edt_ws_bytes(int B, int H, int W, int D) {
  if (B < 1 || H < 1 || W < 1 || D < 1) return 0;
  return edt_ws(nullptr, (long long)B * H * W * D).bytes;
}

int mmseg_edt(const void* mask, int mask_bytes, int B, int H, int W, int D, double s0, double s1, double s2,
              double* out, void* ws, long long ws_bytes, void* stream) {
  if (edt_check("edt", mask_bytes, B, H, W, D)) return 1;
  MMSEG_REQUIRE(mask && out && ws, "edt: null buffer");
  const EdtWs e = edt_ws(ws, (long long)B * H * W * D);
  MMSEG_REQUIRE(ws_bytes >= e.bytes, "edt: workspace of %lld bytes, %lld needed", ws_bytes, e.bytes);
  hipStream_t s = (hipStream_t)stream;
  if (mask_bytes == 8) edt_run((const int64_t*)mask, B, H, W, D, s0, s1, s2, out, e, s);
  else edt_run((const uint8_t*)mask, B, H, W, D, s0, s1, s2, out, e, s);
  return mmseg::check_launch("edt");
}

long long mmseg_hd_ws_bytes(int B, int H, int W, int D) {
  if (B < 1 || H < 1 || W < 1 || D < 1) return 0;
  return hd_ws(nullptr, B, (long long)H * W * D).bytes;
}

int mmseg_hd_update(const void* pred, int pred_bytes, const void* target, int target_bytes, int B, int H, int W, int D,
                    double s0, double s1, double s2, double qfrac, double* records, void* ws, long long ws_bytes,
                    void* stream) {
  if (edt_check("hd_update", pred_bytes, B, H, W, D) || edt_check("hd_update", target_bytes, B, H, W, D)) return 1;
  MMSEG_REQUIRE(pred && target && records && ws, "hd_update: null buffer");
  MMSEG_REQUIRE(qfrac >= 0.0 && qfrac <= 1.0, "hd_update: percentile / 100 in [0, 1]");
  MMSEG_REQUIRE(B <= 65535, "hd_update: at most 65535 samples per call");
  const long long V = (long long)H * W * D, N = (long long)B * V;
  const HdWs h = hd_ws(ws, B, V);
  MMSEG_REQUIRE(ws_bytes >= h.bytes, "hd_update: workspace of %lld bytes, %lld needed", ws_bytes, h.bytes);
  hipStream_t s = (hipStream_t)stream;
  MMSEG_REQUIRE(hipMemsetAsync((char*)ws + h.small_off, 0, (size_t)h.small_bytes, s) == hipSuccess,
                "hd_update: memset failed");
  if (pred_bytes == 8) edt_run((const int64_t*)pred, B, H, W, D, s0, s1, s2, h.dist_pred, h.e, s);
  else edt_run((const uint8_t*)pred, B, H, W, D, s0, s1, s2, h.dist_pred, h.e, s);
  if (target_bytes == 8) edt_run((const int64_t*)target, B, H, W, D, s0, s1, s2, h.dist_target, h.e, s);
  else edt_run((const uint8_t*)target, B, H, W, D, s0, s1, s2, h.dist_target, h.e, s);
  const dim3 ggrid((unsigned)count_grid(V), (unsigned)B);
#define HDG(PT, TT)                                                                                           \
  MMSEG_LAUNCH((hd_gather_kernel<PT, TT>), ggrid, dim3(256), 0, s, (const PT*)pred, (const TT*)target,        \
               (const double*)h.dist_pred, (const double*)h.dist_target, H, (unsigned int)((long long)W * D), \
               (unsigned int)V, h.buf, h.ctr)
  if (pred_bytes == 8 && target_bytes == 8) HDG(int64_t, int64_t);
  else if (pred_bytes == 8) HDG(int64_t, uint8_t);
  else if (target_bytes == 8) HDG(uint8_t, int64_t);
  else HDG(uint8_t, uint8_t);
#undef HDG
  MMSEG_LAUNCH(hd_sel_init_kernel, dim3(B), dim3(256), 0, s, (const unsigned int*)h.ctr, qfrac, h.st);
  long long sb = (2 * V + 1023) / 1024;
  const dim3 sgrid((unsigned)(sb > SEL_BLOCKS ? SEL_BLOCKS : sb), (unsigned)B);
  for (int shift = 56; shift >= 0; shift -= 8) {
    MMSEG_LAUNCH(hd_sel_hist_kernel, sgrid, dim3(256), 0, s, (const double*)h.buf, V, shift, h.st);
    MMSEG_LAUNCH(hd_sel_pick_kernel, dim3(B), dim3(256), 0, s, shift, h.st);
  }
  MMSEG_LAUNCH(hd_sel_hi_kernel, sgrid, dim3(256), 0, s, (const double*)h.buf, V, h.st);
  MMSEG_LAUNCH(hd_sel_final_kernel, dim3((B + 63) / 64), dim3(64), 0, s, (const HdState*)h.st,
               (const double*)h.dist_pred, (const double*)h.dist_target, V, B, records);
  return mmseg::check_launch("hd_update");
}

int mmseg_confusion_counts_idx(const void* pred, int pred_bytes, const void* target, int target_bytes, long long total,
                               int C, long long* counts, unsigned long long* invalid, void* stream) {
  MMSEG_REQUIRE(C >= 1 && C <= CMAX, "confusion_counts_idx: 1 <= C <= %d", CMAX);
  MMSEG_REQUIRE((pred_bytes == 8 || pred_bytes == 1) && (target_bytes == 8 || target_bytes == 1),
                "confusion_counts_idx: masks are uint8 or int64");
  MMSEG_REQUIRE(total >= 0 && pred && target && counts && invalid, "confusion_counts_idx: bad args");
  if (total == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int grid = count_grid(total);
#define CCI(PT, LT)                                                                                              \
  MMSEG_LAUNCH((confusion_idx_kernel<PT, LT>), dim3(grid), dim3(256), 0, s, (const PT*)pred, (const LT*)target, \
               C, total, (unsigned long long*)counts, invalid)
  if (pred_bytes == 8 && target_bytes == 8) CCI(int64_t, int64_t);
  else if (pred_bytes == 8) CCI(int64_t, uint8_t);
  else if (target_bytes == 8) CCI(uint8_t, int64_t);
  else CCI(uint8_t, uint8_t);
#undef CCI
  return mmseg::check_launch("confusion_counts_idx");
}

int mmseg_confusion_counts(const float* logits, const void* target, int target_bytes, int N, int C, long long V,
                           long long* counts, unsigned long long* invalid, void* stream) {
  MMSEG_REQUIRE(C >= 1 && C <= CMAX, "confusion_counts: 1 <= C <= %d", CMAX);
  MMSEG_REQUIRE(target_bytes == 8 || target_bytes == 1, "confusion_counts: labels are uint8 or int64");
  MMSEG_REQUIRE(N >= 0 && V >= 0 && logits && target && counts && invalid, "confusion_counts: bad args");
  const long long total = (long long)N * V;
  if (total == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int grid = count_grid(total);
  if (target_bytes == 8)
    MMSEG_LAUNCH(confusion_logits_kernel<int64_t>, dim3(grid), dim3(256), 0, s, logits, (const int64_t*)target, C, V,
                 total, (unsigned long long*)counts, invalid);
  else
    MMSEG_LAUNCH(confusion_logits_kernel<uint8_t>, dim3(grid), dim3(256), 0, s, logits, (const uint8_t*)target, C, V,
                 total, (unsigned long long*)counts, invalid);
  return mmseg::check_launch("confusion_counts");
}

}  // extern "C"
