// The fixed-order split reduces of the weight gradients (split partials -> torch-layout gradient, WReduceArgs in
// conv_common.h), one launch per layer or several layers' deferred reduces in one (the queue g_wred_pending lives
// here, once), and their entry points.
#include "conv_common.h"

#include <algorithm>
#include <vector>

namespace {

// 256 threads = (256/S) float4 columns x S split slices: slice s sums splits
// k = s, s+S, ... with 16-B loads, then the S slice sums are added in slice
// order -> deterministic.  S follows ksplit (1 for a few splits, up to 64 for
// thousands), so every thread has a few independent loads in flight.  Bias
// partials ([ks][Ca], after the weight columns) are summed by the blocks past
// the weight range.
template <int U>
__device__ __forceinline__ void wred_body(WReduceArgs g, const int S, const int bx, const int gy, float4* red) {
  if (gy) {                                   // grouped: this group's splits and gradient
    const long long gi = gy;
    g.part += gi * g.ksplit * ((long long)g.Ca * g.Ncols);
    if (g.bias_part) g.bias_part += gi * g.ksplit * g.Ca;
    g.grad += gi * g.grad_gstride;
    if (g.bias_grad) g.bias_grad += gi * g.bias_gstride;
  }
  const int NC = 256 / S;                     // float4 columns per block
  const int col4 = threadIdx.x % NC, sl = threadIdx.x / NC;
  const long long total = (long long)g.Ca * g.Ncols;   // multiple of 4
  const long long e0 = ((long long)bx * NC + col4) * 4;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (e0 < total) {
    const float4* p = reinterpret_cast<const float4*>(g.part + e0);
    const long long stride4 = total / 4;
    // U loads in flight per thread (the sum order stays k = sl, sl + S, ...)
    for (int k0 = sl; k0 < g.ksplit; k0 += U * S) {
      float4 a[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u * S;
        if (k < g.ksplit) a[u] = p[(long long)k * stride4];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k0 + u * S < g.ksplit) {
          v.x += a[u].x; v.y += a[u].y; v.z += a[u].z; v.w += a[u].w;
        }
      }
    }
  } else if (g.bias_part) {
    const long long r0 = e0 - total;   // bias rows r0 .. r0+3
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (r0 + q >= g.Ca) break;
      float a = 0.f;
      for (int k = sl; k < g.ksplit; k += S) a += g.bias_part[(long long)k * g.Ca + r0 + q];
      (&v.x)[q] = a;
    }
  }
  if (S > 1) {
    // slice sums: a fixed pairwise tree (S = 16..64 made the former serial sweep of one thread per column the
    // kernel's critical path)
    red[sl * NC + col4] = v;
    __syncthreads();
#pragma unroll
    for (int h = S / 2; h > 0; h >>= 1) {
      if (sl < h) {
        const float4 a = red[(sl + h) * NC + col4];
        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
        red[sl * NC + col4] = v;
      }
      __syncthreads();
    }
    if (sl != 0) return;
  }
  // channel-major partials: the four sums are four consecutive gradient floats (col = c ntap + tap and the torch
  // offset (row creal + c) ntap + tap differ by row (Ncols - creal ntap), a multiple of 4, and the real-channel
  // boundary col = creal ntap is one too) -- one 16-B store instead of four 4-B ones
  if (g.vec4 && e0 < total && g.frag_mt == 0 && g.chmajor) {
    const long long row = e0 / g.Ncols;
    const long long col = e0 - row * g.Ncols;
    if (col >= (long long)g.creal * g.ntap) return;   // channel padding: dropped
    float4* d = reinterpret_cast<float4*>(g.grad + row * ((long long)g.creal * g.ntap) + col);
    if (g.accumulate) {
      const float4 o = *d;
      v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
    }
    *d = v;
    return;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long long idx = e0 + q;
    const float val = (&v.x)[q];
    if (idx >= total) {
      const long long row = idx - total;
      if (!g.bias_part || row >= g.Ca) continue;
      g.bias_grad[row] = g.accumulate ? g.bias_grad[row] + val : val;
      continue;
    }
    int row, tt, c;
    if (g.frag_mt > 0) {
      // tile (rt, ct) of CO x (27 taps x 32 channels), inside it ((tap * MT + i) * 2 + j) * 256 + lane * 4 + r
      const int CO = g.frag_mt * 16, tsz = CO * 27 * 32;
      const int tile = (int)(idx / tsz), loc = (int)(idx - (long long)tile * tsz);
      const int rt = tile / g.nchunk, ct = tile - rt * g.nchunk;
      const int f = loc >> 8, e = loc & 255, lane = e >> 2, r = e & 3;
      const int j = f & 1, i = (f >> 1) % g.frag_mt;
      tt = (f >> 1) / g.frag_mt;
      row = rt * CO + 16 * i + 4 * (lane >> 4) + r;
      c = ct * 32 + 16 * j + (lane & 15);
      if (row >= g.Ca || c >= g.creal) continue;   // past the tiles (channel padding): never written, sum dropped
      const long long dst = ((long long)row * g.creal + c) * g.ntap + tt;
      if (g.accumulate) g.grad[dst] += val;
      else g.grad[dst] = val;
      continue;
    }
    row = (int)(idx / g.Ncols);
    const int col = (int)(idx - (long long)row * g.Ncols);
    if (g.chmajor) {
      c = col / g.ntap;
      tt = col - c * g.ntap;
    } else {
      tt = col / g.cpad;
      c = col - tt * g.cpad;
    }
    if (c >= g.creal || tt >= g.ntap) continue;
    const long long dst = ((long long)row * g.creal + c) * g.ntap + tt;   // torch layout [row][c_real][tap]
    if (g.accumulate) g.grad[dst] += val;
    else g.grad[dst] = val;
  }
}

template <int S, int U = 4>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(WReduceArgs g) {
  __shared__ float4 red[256];
  wred_body<U>(g, S, blockIdx.x, blockIdx.y, red);
}

// Several layers' split reduces in one launch (mmseg_wgrad_reduce_flush): descriptor k owns blocks
// [blk0[k], blk0[k + 1]) = groups x nbx[k], each summed exactly as its own wgrad_reduce_kernel<S[k]> launch would
// (same slices, same fixed order: bitwise the same gradient).
constexpr int WRB_MAX = 30;
struct WReduceBatch {
  int n;
  int blk0[WRB_MAX + 1];
  int nbx[WRB_MAX];
  int S[WRB_MAX];
  WReduceArgs d[WRB_MAX];
};
__global__ __launch_bounds__(256) void wgrad_reduce_batch_kernel(WReduceBatch b) {
  __shared__ float4 red[256];
  const int bid = blockIdx.x;
  int k = 0;
  while (k + 1 < b.n && bid >= b.blk0[k + 1]) ++k;
  const int local = bid - b.blk0[k];
  wred_body<4>(b.d[k], b.S[k], local % b.nbx[k], local / b.nbx[k], red);
}

// split slices S of a reduce: about 8 split loads per thread, the slice sums a pairwise
// LDS tree; small gradients over many splits (the stem: 1,056 values x 1,024 splits) take more slices until the
// grid fills the chip, down to 2 loads per thread (S = 64 left it at 66 blocks, 12.8 us for 4 MB)
int wred_slices(const WReduceArgs& g) {
  const int ksplit = g.ksplit;
  const long long total = (long long)g.Ca * g.Ncols + (g.bias_part ? g.Ca : 0);
  int S = 1;
  while (S < 64 && ksplit / (2 * S) >= 8) S *= 2;
  while (S < 256 && (total * S + 1023) / 1024 < 512 && ksplit / (2 * S) >= 2) S *= 2;
  return S;
}

// reduces deferred by conv3_wgrad_impl (phase bit 4) until mmseg_wgrad_reduce_flush
struct PendingWred {
  WReduceArgs r;
  int groups;
  void* stream;
};
std::vector<PendingWred> g_wred_pending;

}  // namespace

// Queue a deferred reduce (summed by the next mmseg_wgrad_reduce_flush on its stream).  (Flushing early, once
// 60-240 MB of partials are queued so they are re-read from the Infinity Cache, measured +0.03..0.12 ms: r04.)
MMSEG_LOCAL int wred_push(const WReduceArgs& r, int groups, void* stream) {
  // a queued reduce reads its partials when the queue is flushed: a second weight-gradient kernel into the same
  // partial buffer before that would have overwritten them (the engine flushes first: Runtime.own_part)
  for (const auto& e : g_wred_pending)
    if (e.stream == stream && (e.r.part == r.part || (r.bias_part && e.r.bias_part == r.bias_part))) {
      mmseg::set_error("deferred weight-gradient reduce: its partial buffer is already queued on this stream "
                       "(flush the queue before reusing it)");
      return -1;
    }
  g_wred_pending.push_back({r, groups, stream});
  return 0;
}

MMSEG_LOCAL int launch_wgrad_reduce(WReduceArgs g, void* stream, int groups) {
  const long long total = (long long)g.Ca * g.Ncols + (g.bias_part ? g.Ca : 0);
  hipStream_t s = (hipStream_t)stream;
  const int S = wred_slices(g);
#define MMSEG_WRED(SS, NB)                                                                             \
  case SS:                                                                                             \
    MMSEG_LAUNCH((wgrad_reduce_kernel<SS, 4>), dim3(ceil_div(total, NB), groups), dim3(256), 0, s, g);  \
    break;
  switch (S) {
    MMSEG_WRED(256, 4)
    MMSEG_WRED(128, 8)
    MMSEG_WRED(64, 16)
    MMSEG_WRED(32, 32)
    MMSEG_WRED(16, 64)
    MMSEG_WRED(8, 128)
    MMSEG_WRED(4, 256)
    MMSEG_WRED(2, 512)
    default:
      MMSEG_WRED(1, 1024)
  }
#undef MMSEG_WRED
  return mmseg::check_launch("wgrad_reduce");
}

extern "C" {

int mmseg_wgrad_reduce(const float* part, float* grad, const float* bias_part, float* bias_grad, int Ca, int Ncols,
                       int ksplit, int cpad, int creal, int ntap, int accumulate, void* stream) {
  MMSEG_REQUIRE(((long long)Ca * Ncols) % 4 == 0 && (reinterpret_cast<uintptr_t>(part) & 15) == 0,
                "wgrad_reduce: Ca*Ncols %% 4 == 0 and a 16-B aligned partial buffer");
  WReduceArgs g{part, grad, bias_part, bias_grad, Ca, Ncols, ksplit, cpad, creal, ntap, accumulate, 0};
  return launch_wgrad_reduce(g, stream);
}

// mmseg_wgrad_reduce queued until mmseg_wgrad_reduce_flush(stream) (part must stay untouched until then)
int mmseg_wgrad_reduce_defer(const float* part, float* grad, const float* bias_part, float* bias_grad, int Ca,
                             int Ncols, int ksplit, int cpad, int creal, int ntap, int accumulate, void* stream) {
  MMSEG_REQUIRE(((long long)Ca * Ncols) % 4 == 0 && (reinterpret_cast<uintptr_t>(part) & 15) == 0,
                "wgrad_reduce: Ca*Ncols %% 4 == 0 and a 16-B aligned partial buffer");
  WReduceArgs g{part, grad, bias_part, bias_grad, Ca, Ncols, ksplit, cpad, creal, ntap, accumulate, 0};
  return wred_push(g, 1, stream);
}

// Launch the reduces deferred with phase bit 4 (in the order they were deferred, at most WRB_MAX per launch) on
// `stream`; each gradient is bitwise what its own reduce would have written.  Returns the number flushed.
int mmseg_wgrad_reduce_flush(void* stream) {
  int done = 0;
  std::vector<PendingWred> keep;
  std::vector<PendingWred> mine;
  for (auto& e : g_wred_pending) (e.stream == stream ? mine : keep).push_back(e);
  g_wred_pending.swap(keep);
  for (size_t i0 = 0; i0 < mine.size(); i0 += 0) {
    WReduceBatch b{};
    // at most WRB_MAX per launch, and a gradient written by two queued reduces (an accumulating second use) starts
    // a new launch, so the two stay ordered
    size_t i1 = i0;
    while (i1 < mine.size() && i1 - i0 < (size_t)WRB_MAX) {
      bool clash = false;
      for (size_t j = i0; j < i1; ++j)
        clash = clash || mine[j].r.grad == mine[i1].r.grad ||
                (mine[i1].r.bias_grad != nullptr && mine[j].r.bias_grad == mine[i1].r.bias_grad);
      if (clash) break;
      ++i1;
    }
    b.n = (int)(i1 - i0);
    int blk = 0;
    for (int k = 0; k < b.n; ++k) {
      const PendingWred& e = mine[i0 + k];
      const long long total = (long long)e.r.Ca * e.r.Ncols + (e.r.bias_part ? e.r.Ca : 0);
      b.d[k] = e.r;
      b.S[k] = wred_slices(e.r);
      b.nbx[k] = ceil_div(total, 1024 / b.S[k]);
      b.blk0[k] = blk;
      blk += b.nbx[k] * e.groups;
    }
    b.blk0[b.n] = blk;
    mmseg::note_kernel("wgrad_reduce_batch_kernel");
    MMSEG_LAUNCH(wgrad_reduce_batch_kernel, dim3(blk), dim3(256), 0, (hipStream_t)stream, b);
    if (mmseg::check_launch("wgrad_reduce_batch")) return -1;
    done += b.n;
    i0 = i1;
  }
  return done;
}

// number of deferred reduces not yet flushed (all streams)
int mmseg_wgrad_reduce_pending(void) { return (int)g_wred_pending.size(); }

// drop the deferred reduces of `stream` (a backward that failed half way); returns how many
int mmseg_wgrad_reduce_discard(void* stream) {
  const size_t n0 = g_wred_pending.size();
  g_wred_pending.erase(std::remove_if(g_wred_pending.begin(), g_wred_pending.end(),
                                      [&](const PendingWred& e) { return e.stream == stream; }),
                       g_wred_pending.end());
  return (int)(n0 - g_wred_pending.size());
}

}  // extern "C"
