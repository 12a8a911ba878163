// SUV statistics over a PET volume and its organ mask (analysis/: SUVAnalyzer, TMTVAnalyzer, HistogramAnalyzer;
// the reference's src/analysis/suv.py, tmtv.py, histogram.py).  Both volumes are read as the file holds them --
// raw voxel blocks in file order (x fastest), any of the eight NIfTI-1 types, either byte order, optional
// slope / inter -- and every voxel is decoded in registers exactly as nifti_decode_kernel decodes it
// (nifti_src.h), so no fp64 copy of the volume exists and nothing is transposed.
//
// Slots.  l = the decoded label truncated toward zero (get_fdata().astype(np.int32)):
//   slot l        1 <= l <= organ_max: the organ
//   slot 0        l == 0 or l > organ_max: the reference's tumor_region
//   slot NO + 1   l < 0: only its maximum is used (np.max(suv_data) when tumor_region is empty)
// and one more predicate, l <= 0 and x >= tumor_thr (SUVAnalyzer.analyze_tumor's mask).  A non-finite SUV voxel is
// counted in `invalid` and left out of every statistic.
//
// Passes over the volumes (each reads V * (bytes_suv + bytes_seg)); a pass reads its predecessor's results
// from the record in device memory:
//   pass1   per slot count, min, max, sum (min and max of +-0.0 come back as +0.0); slot-0 voxels at or above the absolute threshold; the tumour predicate
//   pass2   per organ sum (x - mean)^2, counts of x >= max f (f = 0.4, 0.5, 0.6), both threshold curves;
//           slot-0 voxels at or above max_region * percentage; first maximum of the absolute mask (np.argmax order)
//   pass3   slot-0 voxels at or above the liver threshold; the three TMTV masks; the per-organ histograms
//   select  8 x (digit histogram, pick): both middle order statistics of every organ and of the tumour predicate
//   peak    np.mean over the +-3 box around that first maximum
// Floating-point sums are per-thread, then a fixed shuffle tree, then per-block partials merged in block order
// by a one-block finalize (again a fixed tree): no float atomics, so two runs give the same bits.  Counts,
// histogram bins and the argmax index use integer atomics.
#include "mmseg_common.h"
#include "nifti_src.h"

namespace {

using namespace nifti_src;

constexpr int OMAX = 15;                 // organ_max at most
constexpr int NSLOT = OMAX + 2;          // slots 0 .. NO + 1
constexpr int NE1 = NSLOT + 2;           // pass1 entries: the slots, the absolute mask, the tumour predicate
constexpr int NV1 = NE1 * 4;             // {count, min, max, sum} each
constexpr int NV2 = OMAX + 3;            // pass2 values: m2 per organ, then count, sum, max of the percentage mask
constexpr int CSTR = 64;                 // cells per threshold curve (ncurve + 1 raw bins fit: ncurve <= 63)
constexpr int BMAX = 256;                // histogram bins at most
constexpr int NQ = 2 * (OMAX + 1);       // select queries: {lower, upper middle} x {organs, tumour predicate}
constexpr int NT = 256;                  // threads per block
constexpr int NW = NT / 64;
constexpr int MAX_BLOCKS = 2048;         // 8 blocks on each of the MI355X's 256 CUs
constexpr int PEAK_R = 3;                // _calculate_suv_peak's neighborhood_size

// ---- the record: 8-byte cells, doubles unless marked u64 (mmseg_hip.h repeats this layout)
enum {
  R_INVALID = 0,                                    // u64
  R_ABS_CNT = 1, R_ABS_SUM, R_ABS_MAX, R_ABS_MEAN,  // count u64
  R_PCT_THR = 5, R_PCT_CNT, R_PCT_SUM, R_PCT_MAX, R_PCT_MEAN,
  R_LIVER_PRESENT = 10,                             // u64
  R_LIVER_THR = 11, R_LIV_CNT, R_LIV_SUM, R_LIV_MAX, R_LIV_MEAN, R_LIVER_MEAN, R_LIVER_STD,
  R_ARG = 18,                                       // u64 C-order index, ~0 = the absolute mask is empty
  R_PEAK = 19,
  R_TUM_CNT = 20, R_TUM_SUM, R_TUM_MAX, R_TUM_MEAN, R_TUM_LO, R_TUM_HI,
  R_MAX_REGION = 26,
  R_SLOT = 32,                                      // [NSLOT][8]: count u64, min, max, sum, mean, m2, std, -
  R_ORG = R_SLOT + NSLOT * 8,                       // [OMAX][8]: n40, n50, n60 u64, a_lo, a_hi, hist lo, hist hi, -
  R_CREL = R_ORG + OMAX * 8,                        // [OMAX][CSTR] u64
  R_CABS = R_CREL + OMAX * CSTR,                    // [OMAX][CSTR] u64
  R_HIST = R_CABS + OMAX * CSTR,                    // [OMAX][BMAX] u64
  R_CELLS = R_HIST + OMAX * BMAX
};

struct Vol {
  const void* p;
  int dt, swap, scale;
  double slope, inter;
};

__device__ __forceinline__ double vox(const Vol& v, size_t i) {
  double x;
  switch (v.dt) {                        // wave-uniform
    case 2: x = Src<2>::get(v.p, i, v.swap); break;
    case 4: x = Src<4>::get(v.p, i, v.swap); break;
    case 8: x = Src<8>::get(v.p, i, v.swap); break;
    case 16: x = Src<16>::get(v.p, i, v.swap); break;
    case 64: x = Src<64>::get(v.p, i, v.swap); break;
    case 256: x = Src<256>::get(v.p, i, v.swap); break;
    case 512: x = Src<512>::get(v.p, i, v.swap); break;
    default: x = Src<768>::get(v.p, i, v.swap); break;
  }
  if (v.scale) x = scl(x, v.slope, v.inter);
  return x;
}
__device__ __forceinline__ int slot_of(int l, int NO) { return l < 0 ? NO + 1 : (l > NO ? 0 : l); }

// UNR voxels of one thread, a grid stride apart, loaded back to back (an index past the end reads voxel 0 and is
// marked not ok): the loads of a batch are in flight together, where one voxel per iteration waits out each load
constexpr int UNR = 4;
struct Batch {
  double x[UNR];
  int l[UNR];
  bool ok[UNR];
};
template <int DT>
__device__ __forceinline__ void load_t(const Vol& v, const size_t* j, double* out) {
#pragma unroll
  for (int u = 0; u < UNR; ++u) out[u] = Src<DT>::get(v.p, j[u], v.swap);
}
__device__ __forceinline__ void load_vol(const Vol& v, const size_t* j, double* out) {
  switch (v.dt) {                        // wave-uniform
    case 2: load_t<2>(v, j, out); break;
    case 4: load_t<4>(v, j, out); break;
    case 8: load_t<8>(v, j, out); break;
    case 16: load_t<16>(v, j, out); break;
    case 64: load_t<64>(v, j, out); break;
    case 256: load_t<256>(v, j, out); break;
    case 512: load_t<512>(v, j, out); break;
    default: load_t<768>(v, j, out); break;
  }
  if (v.scale) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) out[u] = scl(out[u], v.slope, v.inter);
  }
}
__device__ __forceinline__ void load_batch(const Vol& suv, const Vol& seg, size_t i0, size_t stride, size_t V,
                                           Batch& b) {
  size_t j[UNR];
#pragma unroll
  for (int u = 0; u < UNR; ++u) {
    const size_t i = i0 + (size_t)u * stride;
    b.ok[u] = i < V;
    j[u] = b.ok[u] ? i : 0;
  }
  load_vol(suv, j, b.x);
  if (seg.p) {
    double lv[UNR];
    load_vol(seg, j, lv);
#pragma unroll
    for (int u = 0; u < UNR; ++u) b.l[u] = (int)lv[u];        // get_fdata().astype(np.int32)
  } else {
#pragma unroll
    for (int u = 0; u < UNR; ++u) b.l[u] = 0;                 // no segmentation = label 0 everywhere
  }
}
__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN

__device__ __forceinline__ void put_d(unsigned long long* rec, int i, double v) {
  rec[i] = (unsigned long long)__double_as_longlong(v);
}
__device__ __forceinline__ double get_d(const unsigned long long* rec, int i) {
  return __longlong_as_double((long long)rec[i]);
}

// order-preserving key of a double (negative values included); -0.0 counts as +0.0, as it compares
__device__ __forceinline__ unsigned long long key_of(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x + 0.0);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double unkey(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

enum { OP_SUM = 0, OP_MIN = 1, OP_MAX = 2 };
__device__ __forceinline__ double red_op(double a, double b, int op) {
  return op == OP_SUM ? a + b : op == OP_MIN ? (b < a ? b : a) : (b > a ? b : a);
}
// the same value in every lane; a fixed butterfly, so a fixed order
__device__ __forceinline__ double wave_red(double x, int op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = red_op(x, __shfl_xor(x, o, 64), op);
  return x;
}
__device__ __forceinline__ int op_of1(int j) { return (j & 3) == 1 ? OP_MIN : (j & 3) == 2 ? OP_MAX : OP_SUM; }
__device__ __forceinline__ int op_of2(int j) { return j == OMAX + 2 ? OP_MAX : OP_SUM; }
__device__ __forceinline__ int op_of3(int j) { return j == 2 ? OP_MAX : OP_SUM; }

// tot[j] = the blocks' partials of value j merged in a fixed order: lane l of a wave folds blocks l, l + 64, ...
// in turn, then the butterfly; KIND picks the pass's operator table
template <int KIND> __device__ __forceinline__ int op_of(int j) {
  return KIND == 1 ? op_of1(j) : KIND == 2 ? op_of2(j) : op_of3(j);
}
template <int KIND, int NV>
__device__ __forceinline__ void merge_partials(const double* __restrict__ part, int nblk, double* tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < NV; j += NW) {
    const int op = op_of<KIND>(j);
    double v = op == OP_SUM ? 0.0 : op == OP_MIN ? __builtin_inf() : -__builtin_inf();
    for (int b = lane; b < nblk; b += 64) v = red_op(v, part[(size_t)b * NV + j], op);
    v = wave_red(v, op);
    if (lane == 0) tot[j] = v;
  }
}

// ------------------------------------------------------------------ pass 1
// A thread's voxels lie a grid stride apart, so they change slot rarely: the running {count, sum, min, max} of the
// thread's current slot stay in registers and are folded into LDS when the slot changes -- the sum into the
// thread's own cell of that slot (no atomics: every sum has one fixed order), count and extrema into the block's
// cells with integer atomics on ordered keys.  The absolute mask and the tumour predicate have registers of
// their own.
__global__ __launch_bounds__(NT) void suv_pass1_kernel(Vol suv, Vol seg, long long V, int NO, double abs_thr,
                                                       double tum_thr, double* __restrict__ part,
                                                       unsigned long long* __restrict__ rec) {
  __shared__ double c_sum[NSLOT][NT];
  __shared__ unsigned long long c_min[NSLOT], c_max[NSLOT];
  __shared__ unsigned int c_cnt[NSLOT];
  __shared__ double red[NW][6];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) c_sum[s][t] = 0.0;
  if (t < NSLOT) {
    c_min[t] = ~0ull;
    c_max[t] = 0ull;
    c_cnt[t] = 0u;
  }
  __syncthreads();
  int cs = 0;                                   // the current slot and its running values
  unsigned int c = 0;
  double sm = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
  unsigned int ac = 0, tc = 0, inv = 0;         // absolute mask, tumour predicate, invalid voxels
  double as = 0.0, amx = -__builtin_inf(), ts = 0.0, tmx = -__builtin_inf();
  auto flush = [&]() {
    if (c) {
      c_sum[cs][t] += sm;
      atomicAdd(&c_cnt[cs], c);
      atomicMin(&c_min[cs], key_of(mn));
      atomicMax(&c_max[cs], key_of(mx));
    }
    c = 0;
    sm = 0.0;
    mn = __builtin_inf();
    mx = -__builtin_inf();
  };
  const size_t stride = (size_t)gridDim.x * NT;
  for (size_t i0 = (size_t)blockIdx.x * NT + t; i0 < (size_t)V; i0 += UNR * stride) {
    Batch bt;
    load_batch(suv, seg, i0, stride, (size_t)V, bt);
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (!bt.ok[u]) continue;
      const double x = bt.x[u];
      const int l = bt.l[u];
      if (!finite_d(x)) {
        ++inv;
        continue;
      }
      const int slot = slot_of(l, NO);
      if (slot != cs) {
        flush();
        cs = slot;
      }
      ++c;
      sm += x;
      mn = x < mn ? x : mn;
      mx = x > mx ? x : mx;
      if (slot == 0 && x >= abs_thr) {
        ++ac;
        as += x;
        amx = x > amx ? x : amx;
      }
      if (l <= 0 && x >= tum_thr) {
        ++tc;
        ts += x;
        tmx = x > tmx ? x : tmx;
      }
    }
  }
  flush();
  {
    const double v0 = wave_red((double)ac, OP_SUM), v1 = wave_red(as, OP_SUM), v2 = wave_red(amx, OP_MAX),
                 v3 = wave_red((double)tc, OP_SUM), v4 = wave_red(ts, OP_SUM), v5 = wave_red(tmx, OP_MAX);
    if (lane == 0) {
      red[wave][0] = v0;
      red[wave][1] = v1;
      red[wave][2] = v2;
      red[wave][3] = v3;
      red[wave][4] = v4;
      red[wave][5] = v5;
    }
  }
  // invalid voxels: one integer atomic per wave
  const unsigned int winv = (unsigned int)wave_red((double)inv, OP_SUM);
  if (lane == 0 && winv) atomicAdd(&rec[R_INVALID], (unsigned long long)winv);
  __syncthreads();
  double* out = part + (size_t)blockIdx.x * NV1;
  for (int s = wave; s < NSLOT; s += NW) {      // a slot's sum: the threads' cells in a fixed tree
    double v = ((c_sum[s][lane] + c_sum[s][lane + 64]) + c_sum[s][lane + 128]) + c_sum[s][lane + 192];
    v = wave_red(v, OP_SUM);
    if (lane == 0) {
      const unsigned int n = c_cnt[s];
      out[s * 4 + 0] = (double)n;
      out[s * 4 + 1] = n ? unkey(c_min[s]) : __builtin_inf();
      out[s * 4 + 2] = n ? unkey(c_max[s]) : -__builtin_inf();
      out[s * 4 + 3] = v;
    }
  }
  if (t < 2) {                                  // entry NSLOT: the absolute mask; NSLOT + 1: the tumour predicate
    double n = red[0][3 * t], sum = red[0][3 * t + 1], top = red[0][3 * t + 2];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      n += red[w][3 * t];
      sum += red[w][3 * t + 1];
      top = red_op(top, red[w][3 * t + 2], OP_MAX);
    }
    out[(NSLOT + t) * 4 + 0] = n;
    out[(NSLOT + t) * 4 + 1] = __builtin_inf();
    out[(NSLOT + t) * 4 + 2] = top;
    out[(NSLOT + t) * 4 + 3] = sum;
  }
}

// merge the blocks' partials in block order; means, thresholds, histogram ranges, the select's ranks
__global__ __launch_bounds__(NT) void suv_fin1_kernel(const double* __restrict__ part, int nblk, int NO, double pct,
                                                      unsigned long long* __restrict__ rec,
                                                      unsigned long long* __restrict__ sel_k) {
  __shared__ double tot[NV1];
  merge_partials<1, NV1>(part, nblk, tot);
  __syncthreads();
  const int t = threadIdx.x;
  if (t < NO + 2) {
    const double c = tot[t * 4];
    unsigned long long* r = rec + R_SLOT + t * 8;
    r[0] = (unsigned long long)c;
    put_d(r, 1, tot[t * 4 + 1]);
    put_d(r, 2, tot[t * 4 + 2]);
    put_d(r, 3, tot[t * 4 + 3]);
    put_d(r, 4, c > 0.0 ? tot[t * 4 + 3] / c : 0.0);
    if (t >= 1 && t <= NO) {
      // np.histogram's range: (min, max), or (min - 0.5, max + 0.5) when they are equal
      double lo = tot[t * 4 + 1], hi = tot[t * 4 + 2];
      if (lo == hi) {
        lo -= 0.5;
        hi += 0.5;
      }
      put_d(rec, R_ORG + (t - 1) * 8 + 5, lo);
      put_d(rec, R_ORG + (t - 1) * 8 + 6, hi);
    }
  }
  if (t < 2 * (NO + 1)) {
    const int qs = t >> 1;
    const unsigned long long n = (unsigned long long)(qs < NO ? tot[(qs + 1) * 4] : tot[(NSLOT + 1) * 4]);
    sel_k[t] = n == 0 ? 0 : (t & 1) ? n / 2 : (n - 1) / 2;
  }
  if (t == 0) {
    const double ac = tot[NSLOT * 4], tc = tot[(NSLOT + 1) * 4];
    rec[R_ABS_CNT] = (unsigned long long)ac;
    put_d(rec, R_ABS_SUM, tot[NSLOT * 4 + 3]);
    put_d(rec, R_ABS_MAX, tot[NSLOT * 4 + 2]);
    put_d(rec, R_ABS_MEAN, ac > 0.0 ? tot[NSLOT * 4 + 3] / ac : 0.0);
    rec[R_TUM_CNT] = (unsigned long long)tc;
    put_d(rec, R_TUM_SUM, tot[(NSLOT + 1) * 4 + 3]);
    put_d(rec, R_TUM_MAX, tot[(NSLOT + 1) * 4 + 2]);
    put_d(rec, R_TUM_MEAN, tc > 0.0 ? tot[(NSLOT + 1) * 4 + 3] / tc : 0.0);
    // np.max(suv_data[tumor_region]) if tumor_region.any() else np.max(suv_data)
    double mr = tot[2];
    if (!(tot[0] > 0.0))
      for (int s = 1; s < NO + 2; ++s) mr = red_op(mr, tot[s * 4 + 2], OP_MAX);
    put_d(rec, R_MAX_REGION, mr);
    put_d(rec, R_PCT_THR, mr * pct);
    rec[R_ARG] = ~0ull;
  }
}

// ------------------------------------------------------------------ pass 2
__global__ __launch_bounds__(NT) void suv_pass2_kernel(Vol suv, Vol seg, long long V, int X, int Y, int Z, int NO,
                                                       double abs_thr, const double* __restrict__ curve_rel,
                                                       const double* __restrict__ curve_abs, int NC,
                                                       double* __restrict__ part, unsigned long long* __restrict__ rec) {
  __shared__ double s_mean[OMAX], s_thr3[OMAX * 3], s_rel[OMAX * CSTR], s_abs[CSTR];
  __shared__ unsigned int b_rel[OMAX * CSTR], b_abs[OMAX * CSTR], c3[OMAX * 3];
  __shared__ unsigned long long s_arg;
  __shared__ double red[NW][NV2];
  for (int j = threadIdx.x; j < OMAX * CSTR; j += NT) {
    b_rel[j] = 0;
    b_abs[j] = 0;
    const int o = j / CSTR, k = j % CSTR;
    // max_suv * thresh_pct: one multiply
    s_rel[j] = (o < NO && k < NC) ? get_d(rec, R_SLOT + (o + 1) * 8 + 2) * curve_rel[k] : 0.0;
  }
  if (threadIdx.x < CSTR) s_abs[threadIdx.x] = threadIdx.x < NC ? curve_abs[threadIdx.x] : 0.0;
  if (threadIdx.x < OMAX * 3) {
    const int o = threadIdx.x / 3, f = threadIdx.x % 3;
    c3[threadIdx.x] = 0;
    s_thr3[threadIdx.x] = o < NO ? get_d(rec, R_SLOT + (o + 1) * 8 + 2) * (f == 0 ? 0.4 : f == 1 ? 0.5 : 0.6) : 0.0;
  }
  if (threadIdx.x < OMAX) s_mean[threadIdx.x] = threadIdx.x < NO ? get_d(rec, R_SLOT + (threadIdx.x + 1) * 8 + 4) : 0.0;
  if (threadIdx.x == 0) s_arg = ~0ull;
  const double pct_thr = get_d(rec, R_PCT_THR), abs_max = get_d(rec, R_ABS_MAX);
  __syncthreads();

  double m2[OMAX];
#pragma unroll
  for (int o = 0; o < OMAX; ++o) m2[o] = 0.0;
  double pc = 0.0, ps = 0.0, pm = -__builtin_inf();
  const size_t stride = (size_t)gridDim.x * NT;
  for (size_t i0 = (size_t)blockIdx.x * NT + threadIdx.x; i0 < (size_t)V; i0 += UNR * stride) {
    Batch bt;
    load_batch(suv, seg, i0, stride, (size_t)V, bt);
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const size_t i = i0 + (size_t)u * stride;
      const double x = bt.x[u];
      if (!bt.ok[u] || !finite_d(x)) continue;
      const int slot = slot_of(bt.l[u], NO);
      if (slot >= 1 && slot <= NO) {
        const int o = slot - 1;
        double dd;
        {
#pragma clang fp contract(off)
          const double d = x - s_mean[o];
          dd = d * d;
        }
#pragma unroll
        for (int k = 0; k < OMAX; ++k)
          if (k < NO) m2[k] += (o == k) ? dd : 0.0;
#pragma unroll
        for (int f = 0; f < 3; ++f)
          if (x >= s_thr3[o * 3 + f]) atomicAdd(&c3[o * 3 + f], 1u);
        // bin = the number of thresholds <= x; the finalize turns the bins into counts of x >= threshold
        int kr = 0, ka = 0;
        for (int k = 0; k < NC; ++k) {
          kr += s_rel[o * CSTR + k] <= x ? 1 : 0;
          ka += s_abs[k] <= x ? 1 : 0;
        }
        atomicAdd(&b_rel[o * CSTR + kr], 1u);
        atomicAdd(&b_abs[o * CSTR + ka], 1u);
      } else if (slot == 0) {
        if (x >= pct_thr) {
          pc += 1.0;
          ps += x;
          pm = x > pm ? x : pm;
        }
        if (x >= abs_thr && x == abs_max) {
          // file index (z Y + y) X + x -> the reference's C-order index (x Y + y) Z + z
          const unsigned long long xx = i % (size_t)X, yy = (i / (size_t)X) % (size_t)Y, zz = i / ((size_t)X * Y);
          atomicMin(&s_arg, (xx * (unsigned long long)Y + yy) * (unsigned long long)Z + zz);
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 0; o < OMAX; ++o) {
    const double v = wave_red(m2[o], OP_SUM);
    if (lane == 0) red[wave][o] = v;
  }
  {
    const double a = wave_red(pc, OP_SUM), b = wave_red(ps, OP_SUM), c = wave_red(pm, OP_MAX);
    if (lane == 0) {
      red[wave][OMAX] = a;
      red[wave][OMAX + 1] = b;
      red[wave][OMAX + 2] = c;
    }
  }
  __syncthreads();
  if (threadIdx.x < NV2) {
    const int j = threadIdx.x, op = op_of2(j);
    double v = red[0][j];
#pragma unroll
    for (int w = 1; w < NW; ++w) v = red_op(v, red[w][j], op);
    part[(size_t)blockIdx.x * NV2 + j] = v;
  }
  for (int j = threadIdx.x; j < NO * CSTR; j += NT) {
    if (b_rel[j]) atomicAdd(&rec[R_CREL + j], (unsigned long long)b_rel[j]);
    if (b_abs[j]) atomicAdd(&rec[R_CABS + j], (unsigned long long)b_abs[j]);
  }
  if (threadIdx.x < NO * 3 && c3[threadIdx.x])
    atomicAdd(&rec[R_ORG + (threadIdx.x / 3) * 8 + threadIdx.x % 3], (unsigned long long)c3[threadIdx.x]);
  if (threadIdx.x == 0 && s_arg != ~0ull) atomicMin(&rec[R_ARG], s_arg);
}

__global__ __launch_bounds__(NT) void suv_fin2_kernel(const double* __restrict__ part, int nblk, int NO, int NC,
                                                      int liver_label, double abs_thr,
                                                      unsigned long long* __restrict__ rec) {
  __shared__ double tot[NV2];
  __shared__ unsigned long long bins[2 * OMAX][CSTR];
  merge_partials<2, NV2>(part, nblk, tot);
  for (int j = threadIdx.x; j < 2 * OMAX * CSTR; j += NT)
    bins[j / CSTR][j % CSTR] = rec[R_CREL + j];        // the R_CABS cells follow the R_CREL cells
  __syncthreads();
  const int t = threadIdx.x;
  if (t < NO) {
    const double n = (double)rec[R_SLOT + (t + 1) * 8];
    put_d(rec, R_SLOT + (t + 1) * 8 + 5, tot[t]);
    put_d(rec, R_SLOT + (t + 1) * 8 + 6, n > 0.0 ? sqrt(tot[t] / n) : 0.0);     // np.std: sqrt(sum(d^2) / n)
  }
  if (t < 2 * OMAX && (t % OMAX) < NO) {
    // bins[k] = voxels with exactly k thresholds <= x.  Ascending thresholds (max >= 0, and the absolute curve):
    // x >= thr_j iff k > j.  Descending ones (a negative max times an ascending fraction): iff k >= NC - j.
    const int o = t % OMAX;
    const bool desc = t < OMAX && get_d(rec, R_SLOT + (o + 1) * 8 + 2) < 0.0;
    unsigned long long* out = rec + (t < OMAX ? R_CREL : R_CABS) + o * CSTR;
    unsigned long long acc = 0;
    if (desc) {
      for (int j = 0; j < NC; ++j) {
        acc += bins[t][NC - j];
        out[j] = acc;
      }
    } else {
      for (int j = NC - 1; j >= 0; --j) {
        acc += bins[t][j + 1];
        out[j] = acc;
      }
    }
    out[NC] = 0;
  }
  if (t == 0) {
    const double c = tot[OMAX];
    rec[R_PCT_CNT] = (unsigned long long)c;
    put_d(rec, R_PCT_SUM, tot[OMAX + 1]);
    put_d(rec, R_PCT_MAX, tot[OMAX + 2]);
    put_d(rec, R_PCT_MEAN, c > 0.0 ? tot[OMAX + 1] / c : 0.0);
    const bool present = liver_label >= 1 && liver_label <= NO && rec[R_SLOT + liver_label * 8] > 0;
    rec[R_LIVER_PRESENT] = present ? 1 : 0;
    double thr = abs_thr;      // _create_tmtv_mask's fallback when the liver is absent
    if (present) {
#pragma clang fp contract(off)
      const double mean = get_d(rec, R_SLOT + liver_label * 8 + 4);
      const double n = (double)rec[R_SLOT + liver_label * 8];
      const double sd = sqrt(tot[liver_label - 1] / n);
      const double two_sd = 2.0 * sd;
      thr = mean + two_sd;
      put_d(rec, R_LIVER_MEAN, mean);
      put_d(rec, R_LIVER_STD, sd);
    }
    put_d(rec, R_LIVER_THR, thr);
  }
}

// ------------------------------------------------------------------ pass 3
__global__ __launch_bounds__(NT) void suv_pass3_kernel(Vol suv, Vol seg, long long V, int NO, double abs_thr, int B,
                                                       unsigned char* __restrict__ masks, double* __restrict__ part,
                                                       unsigned long long* __restrict__ rec) {
  __shared__ unsigned int hist[OMAX * BMAX];
  __shared__ double s_lo[OMAX], s_hi[OMAX], s_step[OMAX], s_scale[OMAX];
  __shared__ double red[NW][3];
  for (int j = threadIdx.x; j < OMAX * BMAX; j += NT) hist[j] = 0;
  if (threadIdx.x < OMAX) {
    const int o = threadIdx.x;
    const double lo = o < NO ? get_d(rec, R_ORG + o * 8 + 5) : 0.0, hi = o < NO ? get_d(rec, R_ORG + o * 8 + 6) : 1.0;
    s_lo[o] = lo;
    s_hi[o] = hi;
    s_step[o] = (hi - lo) / (double)B;          // np.linspace's step
    s_scale[o] = hi - lo;
  }
  const double pct_thr = get_d(rec, R_PCT_THR), liv_thr = get_d(rec, R_LIVER_THR);
  __syncthreads();
  double lc = 0.0, ls = 0.0, lm = -__builtin_inf();
  const size_t stride = (size_t)gridDim.x * NT;
  for (size_t i0 = (size_t)blockIdx.x * NT + threadIdx.x; i0 < (size_t)V; i0 += UNR * stride) {
    Batch bt;
    load_batch(suv, seg, i0, stride, (size_t)V, bt);
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (!bt.ok[u]) continue;
      const size_t i = i0 + (size_t)u * stride;
      const double x = bt.x[u];
      const int slot = slot_of(bt.l[u], NO);
      if (masks) {      // ((suv_data >= threshold) & tumor_region).astype(np.uint8), in file order
        masks[i] = (unsigned char)(slot == 0 && x >= abs_thr);
        masks[(size_t)V + i] = (unsigned char)(slot == 0 && x >= pct_thr);
        masks[2 * (size_t)V + i] = (unsigned char)(slot == 0 && x >= liv_thr);
      }
      if (!finite_d(x)) continue;
      if (slot == 0) {
        if (x >= liv_thr) {
          lc += 1.0;
          ls += x;
          lm = x > lm ? x : lm;
        }
      } else if (slot <= NO) {
        // np.histogram: the largest i with edge_i <= x, edge_i = i * step + lo (multiply, then add), edge_B = hi, the
        // last bin closed.  The first guess is numpy's own ((x - lo) / (hi - lo)) * B, then stepped onto the edges.
#pragma clang fp contract(off)
        const int o = slot - 1;
        const double lo = s_lo[o], hi = s_hi[o], step = s_step[o];
        const double f = ((x - lo) / s_scale[o]) * (double)B;
        int b = (int)f;
        b = b < 0 ? 0 : b > B - 1 ? B - 1 : b;
        while (b > 0 && x < (double)b * step + lo) --b;
        while (b < B - 1 && x >= ((b + 1 == B) ? hi : (double)(b + 1) * step + lo)) ++b;
        atomicAdd(&hist[o * BMAX + b], 1u);
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  {
    const double a = wave_red(lc, OP_SUM), b = wave_red(ls, OP_SUM), c = wave_red(lm, OP_MAX);
    if (lane == 0) {
      red[wave][0] = a;
      red[wave][1] = b;
      red[wave][2] = c;
    }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int j = threadIdx.x, op = op_of3(j);
    double v = red[0][j];
#pragma unroll
    for (int w = 1; w < NW; ++w) v = red_op(v, red[w][j], op);
    part[(size_t)blockIdx.x * 3 + j] = v;
  }
  for (int j = threadIdx.x; j < NO * BMAX; j += NT)
    if (hist[j]) atomicAdd(&rec[R_HIST + j], (unsigned long long)hist[j]);
}

// the liver-based mask's statistics, and SUVpeak: np.mean(suv_data[box]) around the absolute mask's first maximum
__global__ __launch_bounds__(NT) void suv_peak_kernel(Vol suv, int X, int Y, int Z, const double* __restrict__ part,
                                                      int nblk, unsigned long long* __restrict__ rec) {
  __shared__ double tot[3];
  __shared__ double red[NW];
  merge_partials<3, 3>(part, nblk, tot);
  __syncthreads();
  if (threadIdx.x == 0) {
    rec[R_LIV_CNT] = (unsigned long long)tot[0];
    put_d(rec, R_LIV_SUM, tot[1]);
    put_d(rec, R_LIV_MAX, tot[2]);
    put_d(rec, R_LIV_MEAN, tot[0] > 0.0 ? tot[1] / tot[0] : 0.0);
  }
  const unsigned long long arg = rec[R_ARG];
  if (arg == ~0ull) {
    if (threadIdx.x == 0) put_d(rec, R_PEAK, 0.0);
    return;
  }
  const int cz = (int)(arg % (unsigned long long)Z), cy = (int)((arg / (unsigned long long)Z) % (unsigned long long)Y),
            cx = (int)(arg / ((unsigned long long)Z * Y));
  const int x0 = max(0, cx - PEAK_R), x1 = min(X, cx + PEAK_R + 1), y0 = max(0, cy - PEAK_R),
            y1 = min(Y, cy + PEAK_R + 1), z0 = max(0, cz - PEAK_R), z1 = min(Z, cz + PEAK_R + 1);
  const int nx = x1 - x0, ny = y1 - y0, nz = z1 - z0, n = nx * ny * nz;
  double s = 0.0;
  for (int e = threadIdx.x; e < n; e += NT) {
    const int x = x0 + e % nx, y = y0 + (e / nx) % ny, z = z0 + e / (nx * ny);
    s += vox(suv, ((size_t)z * Y + y) * X + x);
  }
  s = wave_red(s, OP_SUM);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) v += red[w];
    put_d(rec, R_PEAK, v / (double)n);
  }
}

// ------------------------------------------------------------------ order statistics
// Query q = 2 qs + h: select slot qs (organ qs + 1, or the tumour predicate for qs == NO), h = 0 the element of
// rank (n - 1) / 2, h = 1 of rank n / 2.  One radix pass: the histogram of the digit at `shift` over the keys
// whose higher digits equal the query's prefix so far.
struct SelState {
  unsigned long long prefix[NQ], k[NQ];
  unsigned int hist[NQ * 256];
};

__global__ __launch_bounds__(NT) void suv_sel_hist_kernel(Vol suv, Vol seg, long long V, int NO, double tum_thr,
                                                          int shift, SelState* __restrict__ st) {
  __shared__ unsigned int lh[NQ * 256];
  __shared__ unsigned long long sp[NQ];
  for (int j = threadIdx.x; j < NQ * 256; j += NT) lh[j] = 0;
  if (threadIdx.x < NQ) sp[threadIdx.x] = st->prefix[threadIdx.x];
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * NT;
  for (size_t i0 = (size_t)blockIdx.x * NT + threadIdx.x; i0 < (size_t)V; i0 += UNR * stride) {
    Batch bt;
    load_batch(suv, seg, i0, stride, (size_t)V, bt);
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const double x = bt.x[u];
      if (!bt.ok[u] || !finite_d(x)) continue;
      const int l = bt.l[u];
      int qs;
      if (l >= 1 && l <= NO) qs = l - 1;
      else if (l <= 0 && x >= tum_thr) qs = NO;
      else continue;
      const unsigned long long key = key_of(x);
      const unsigned int digit = (unsigned int)(key >> shift) & 255u;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int q = 2 * qs + h;
        if (shift == 56 || (key >> (shift + 8)) == (sp[q] >> (shift + 8))) atomicAdd(&lh[q * 256 + digit], 1u);
      }
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < 2 * (NO + 1) * 256; j += NT)
    if (lh[j]) atomicAdd(&st->hist[j], lh[j]);
}

// the digit that holds rank k; after the last digit the prefix is the element's key
__global__ __launch_bounds__(NT) void suv_sel_pick_kernel(int shift, int NO, SelState* __restrict__ st,
                                                          unsigned long long* __restrict__ rec) {
  __shared__ unsigned int lh[NQ * 256];
  for (int j = threadIdx.x; j < NQ * 256; j += NT) {      // stage the histograms, and clear them for the next digit
    lh[j] = st->hist[j];
    st->hist[j] = 0;
  }
  __syncthreads();
  const int q = threadIdx.x;
  if (q < 2 * (NO + 1)) {
    const unsigned int* h = lh + q * 256;
    unsigned long long k = st->k[q], cum = 0;
    int d = 0;
    for (; d < 255; ++d) {
      if (cum + h[d] > k) break;
      cum += h[d];
    }
    st->k[q] = k >= cum ? k - cum : 0;
    const unsigned long long prefix = st->prefix[q] | ((unsigned long long)d << shift);
    st->prefix[q] = prefix;
    if (shift == 0) {
      const int qs = q >> 1;
      put_d(rec, qs < NO ? R_ORG + qs * 8 + 3 + (q & 1) : R_TUM_LO + (q & 1), unkey(prefix));
    }
  }
}

// ------------------------------------------------------------------ host
long long align256(long long n) { return (n + 255) & ~255ll; }

int suv_blocks(long long V) {
  const long long b = (V + (long long)NT * 4 - 1) / ((long long)NT * 4);
  return (int)(b < 1 ? 1 : b > MAX_BLOCKS ? MAX_BLOCKS : b);
}

struct SuvWs {
  double *part1, *part2, *part3;
  SelState* st;
  long long st_off, bytes;
};
SuvWs suv_ws(void* ws, long long V) {
  const long long nblk = suv_blocks(V);
  char* p = (char*)ws;
  SuvWs w;
  long long off = 0;
  w.part1 = (double*)(p + off);
  off += align256(nblk * NV1 * 8);
  w.part2 = (double*)(p + off);
  off += align256(nblk * NV2 * 8);
  w.part3 = (double*)(p + off);
  off += align256(nblk * 3 * 8);
  w.st_off = off;
  w.st = (SelState*)(p + off);
  off += align256((long long)sizeof(SelState));
  w.bytes = off;
  return w;
}

int check_vol(const char* what, const void* p, int dt, int swap) {
  MMSEG_REQUIRE(known_datatype(dt),
                "suv_analyze: %s NIfTI datatype %d (supported: 2 uint8, 4 int16, 8 int32, 16 float32, 64 float64, "
                "256 int8, 512 uint16, 768 uint32)", what, dt);
  MMSEG_REQUIRE(swap == 0 || swap == 1, "suv_analyze: %s swap is 0 or 1 (got %d)", what, swap);
  MMSEG_REQUIRE(((uintptr_t)p & (uintptr_t)(datatype_bytes(dt) - 1)) == 0,
                "suv_analyze: %s must be aligned to its %d-byte elements", what, datatype_bytes(dt));
  return 0;
}

}  // namespace

extern "C" {

int mmseg_suv_record_cells(void) { return R_CELLS; }

long long mmseg_suv_ws_bytes(long long V) {
  if (V < 1) return 0;
  return suv_ws(nullptr, V).bytes;
}

int mmseg_suv_analyze(const void* suv, int suv_datatype, int suv_swap, int suv_scale, double suv_slope,
                      double suv_inter, const void* seg, int seg_datatype, int seg_swap, int seg_scale,
                      double seg_slope, double seg_inter, int X, int Y, int Z, int organ_max, int liver_label,
                      double abs_thr, double pct_thr, double tumor_thr, const double* curve_rel,
                      const double* curve_abs, int ncurve, int bins, unsigned char* masks, void* record, void* ws,
                      long long ws_bytes, void* stream) {
  MMSEG_REQUIRE(suv != nullptr && record != nullptr && ws != nullptr, "suv_analyze: suv, record and ws");
  MMSEG_REQUIRE(X >= 1 && Y >= 1 && Z >= 1, "suv_analyze: empty volume %d x %d x %d", X, Y, Z);
  MMSEG_REQUIRE(organ_max >= 1 && organ_max <= OMAX, "suv_analyze: 1 <= organ_max <= %d (got %d)", OMAX, organ_max);
  MMSEG_REQUIRE(ncurve >= 1 && ncurve < CSTR && curve_rel != nullptr && curve_abs != nullptr,
                "suv_analyze: 1 <= ncurve <= %d thresholds per curve, both arrays given (got %d)", CSTR - 1, ncurve);
  MMSEG_REQUIRE(bins >= 1 && bins <= BMAX, "suv_analyze: 1 <= bins <= %d (got %d)", BMAX, bins);
  MMSEG_REQUIRE(((uintptr_t)record & 7) == 0 && ((uintptr_t)ws & 255) == 0,
                "suv_analyze: record 8-byte and ws 256-byte aligned");
  if (check_vol("suv", suv, suv_datatype, suv_swap)) return 1;
  if (seg != nullptr && check_vol("seg", seg, seg_datatype, seg_swap)) return 1;
  const long long V = (long long)X * Y * Z;
  MMSEG_REQUIRE(V < (1ll << 40), "suv_analyze: at most 2^40 voxels (a block counts its voxels in 32 bits)");
  const SuvWs w = suv_ws(ws, V);
  MMSEG_REQUIRE(ws_bytes >= w.bytes, "suv_analyze: workspace of %lld bytes, %lld needed", ws_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  const Vol vs = {suv, suv_datatype, suv_swap, suv_scale != 0, suv_slope, suv_inter};
  const Vol vg = {seg, seg_datatype, seg_swap, seg != nullptr && seg_scale != 0, seg_slope, seg_inter};
  unsigned long long* rec = (unsigned long long*)record;
  const int NO = organ_max, nblk = suv_blocks(V);
  MMSEG_REQUIRE(hipMemsetAsync(record, 0, (size_t)R_CELLS * 8, s) == hipSuccess &&
                    hipMemsetAsync((char*)ws + w.st_off, 0, sizeof(SelState), s) == hipSuccess,
                "suv_analyze: memset failed");
  const dim3 grid(nblk), block(NT), one(1);
  MMSEG_LAUNCH(suv_pass1_kernel, grid, block, 0, s, vs, vg, V, NO, abs_thr, tumor_thr, w.part1, rec);
  MMSEG_LAUNCH(suv_fin1_kernel, one, block, 0, s, (const double*)w.part1, nblk, NO, pct_thr, rec, w.st->k);
  MMSEG_LAUNCH(suv_pass2_kernel, grid, block, 0, s, vs, vg, V, X, Y, Z, NO, abs_thr, curve_rel, curve_abs, ncurve,
               w.part2, rec);
  MMSEG_LAUNCH(suv_fin2_kernel, one, block, 0, s, (const double*)w.part2, nblk, NO, ncurve, liver_label, abs_thr, rec);
  MMSEG_LAUNCH(suv_pass3_kernel, grid, block, 0, s, vs, vg, V, NO, abs_thr, bins, masks, w.part3, rec);
  MMSEG_LAUNCH(suv_peak_kernel, one, block, 0, s, vs, X, Y, Z, (const double*)w.part3, nblk, rec);
  for (int shift = 56; shift >= 0; shift -= 8) {
    MMSEG_LAUNCH(suv_sel_hist_kernel, grid, block, 0, s, vs, vg, V, NO, tumor_thr, shift, w.st);
    MMSEG_LAUNCH(suv_sel_pick_kernel, one, block, 0, s, shift, NO, w.st, rec);
  }
  return mmseg::check_launch("suv_analyze");
}

}  // extern "C"
