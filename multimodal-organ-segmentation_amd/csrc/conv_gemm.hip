// Implicit-GEMM convolutions on CDNA4 MFMA (gfx950): the forward / data-gradient side.
//
// This source holds the per-lane gather GEMM (conv_gemm_kernel) and the split-K reduces, the chooser of every forward /
// data-gradient launch (choose_gemm, with gemm_shape / choose_conv3 for the planning queries), launch_gemm -- one call
// per brick family, whose kernels and launcher sit in conv_brick2.hip, conv_brick6.hip, conv_brick8.hip and
// conv_brickr.hip, plus the gather tiles -- and the forward / data-gradient entry points and planning queries.  The
// weight gradients, with their chooser, are conv_wgrad.hip.
//
// The gather GEMM covers every GEMM-shaped op of the UNet3D / DualEncoder
// training step (reference unet.py:26-27 Conv3d(3,pad 1), unet.py:95
// ConvTranspose3d(2,2), unet.py:163 / dual_encoder.py:75 1x1 Conv3d):
//
//   rows (M)  = voxels of a "row grid" (N x D x H x W, flattened)
//   cols (N)  = output channels (x 8 taps for the transposed conv)
//   K         = k-groups of 8 consecutive channels ("kgi"), each bound to a tap
//
// The A operand is gathered per lane straight from the NDHWC activation
// (8 contiguous channels = one 16 B bf16 / 32 B f32 load), with zero padding
// for out-of-volume taps.  The B operand is the weight tensor pre-packed as
// [KGp][Cpad][8] so that each lane's fragment is one contiguous vector.
//
// bf16: one v_mfma_f32_16x16x32_bf16 per k-step (lane l holds rows l&15,
//       k = 8*(l>>4)+j).
// f32 : eight v_mfma_f32_16x16x4f32 per k-step (exact fp32 FMA chain); lane
//       element j of k-group (l>>4) feeds MFMA j, so A and B agree on K order.
#include "conv_common.h"

#include <algorithm>

namespace {

// Per-lane row descriptor.
struct RowInfo {
  long long m;        // row index (voxel in row grid); -1 if out of range
  long long base;     // CONV3/POINT: m ; CONVT: child base voxel in 2x grid
  uint32_t tmask;     // CONV3: valid taps
};

template <int MODE>
__device__ __forceinline__ RowInfo make_row(long long m, const GemmArgs& g) {
  RowInfo r;
  r.m = m < g.M ? m : -1;
  r.base = m;
  r.tmask = 0;
  if (r.m < 0) return r;
  // 32-bit index arithmetic: M < 2^31 (the host checks M * lda), and 64-bit divisions cost ~100 VALU each
  if (MODE == MODE_CONV3) {
    const unsigned mu = (unsigned)m;
    const unsigned t = mu / (unsigned)g.W, x = mu - t * (unsigned)g.W;
    const unsigned t2 = t / (unsigned)g.H, y = t - t2 * (unsigned)g.H;
    const unsigned z = t2 % (unsigned)g.D;
    r.tmask = tap_valid_mask((int)z, (int)y, (int)x, g.D, g.H, g.W);
  } else if (MODE == MODE_CONVT_DGRAD) {
    const unsigned mu = (unsigned)m;
    const unsigned t = mu / (unsigned)g.W, x = mu - t * (unsigned)g.W;
    const unsigned t2 = t / (unsigned)g.H, y = t - t2 * (unsigned)g.H;
    const unsigned n = t2 / (unsigned)g.D, z = t2 - n * (unsigned)g.D;
    const long long H2 = 2LL * g.H, W2 = 2LL * g.W, D2 = 2LL * g.D;
    r.base = (((long long)n * D2 + 2 * z) * H2 + 2 * y) * W2 + 2 * x;
  }
  return r;
}

// Voxel offset of tap t relative to the row voxel (CONV3) or child (CONVT).
template <int MODE>
__device__ __forceinline__ long long tap_offset(int t, const GemmArgs& g) {
  if (MODE == MODE_CONV3) {
    int dz, dy, dx;
    tap_delta(t, dz, dy, dx);
    return ((long long)dz * g.H + dy) * g.W + dx;
  } else {   // 32-bit: the child grid's voxel count is < 2^31 (host: M * lda)
    const int a = t >> 2, b = (t >> 1) & 1, c = t & 1;
    return (long long)(a * (4 * g.H * g.W) + b * (2 * g.W) + c);
  }
}

template <typename T, int MODE>
__device__ __forceinline__ void load_a(V8<T>& v, const RowInfo& r, int kgi, const GemmArgs& g) {
  const T* A = reinterpret_cast<const T*>(g.a);
  bool ok = r.m >= 0 && kgi < g.KG;
  long long vox = 0;
  int c8 = kgi;
  if (MODE == MODE_CONV3) {
    int t = kgi >> g.cpg_shift;
    c8 = kgi & ((1 << g.cpg_shift) - 1);
    ok = ok && ((r.tmask >> t) & 1u);
    if (ok) vox = r.base + tap_offset<MODE_CONV3>(t, g);
  } else if (MODE == MODE_CONVT_DGRAD) {
    int t = kgi >> g.cpg_shift;
    c8 = kgi & ((1 << g.cpg_shift) - 1);
    vox = r.base + tap_offset<MODE_CONVT_DGRAD>(t, g);
  } else {
    vox = r.base;
  }
  if (ok) v.load(A + vox * g.lda + c8 * 8);
  else v.zero();
}

template <typename T>
__device__ __forceinline__ void load_b(V8<T>& v, int kgi, int col, const GemmArgs& g) {
  const T* B = reinterpret_cast<const T*>(g.b);
  v.load(B + ((long long)kgi * g.Cpad + col) * 8);
}

// Child voxel (2x grid) of input voxel `row` for transposed-conv tap t (32-bit divisions, see make_row).
__device__ __forceinline__ long long convt_child(long long row, int t, const GemmArgs& g) {
  const unsigned mu = (unsigned)row;
  const unsigned q = mu / (unsigned)g.W, x = mu - q * (unsigned)g.W;
  const unsigned q2 = q / (unsigned)g.H, y = q - q2 * (unsigned)g.H;
  const unsigned n = q2 / (unsigned)g.D, z = q2 - n * (unsigned)g.D;
  return (((long long)n * 2 * g.D + 2 * z + (t >> 2)) * 2LL * g.H + 2 * y + ((t >> 1) & 1)) * 2LL * g.W + 2 * x +
         (t & 1);
}

// Block = WM x WN waves; wave tile = (RM*16) x (RN*16).
template <typename T, int MODE, int WM, int WN, int RM, int RN>
__global__ __launch_bounds__(256) void conv_gemm_kernel(GemmArgs g) {
  constexpr int BM = WM * RM * 16;
  constexpr int BN = WN * RN * 16;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int mt_n = (g.M + BM - 1) / BM, nt_n = (g.Ncols + BN - 1) / BN;
  const int tile = g.swz ? xcd_swizzle(blockIdx.x, mt_n * nt_n * g.ksplit) : (int)blockIdx.x;
  const int mt = tile % mt_n, nt = (tile / mt_n) % nt_n, ks = tile / (mt_n * nt_n);
  const long long m0 = (long long)mt * BM + wm * RM * 16;
  const int n0 = nt * BN + wn * RN * 16;
  const int kg_begin = ks * g.kg_per_split;
  int kg_end = kg_begin + g.kg_per_split;
  const int KGp = (g.KG + 3) & ~3;
  if (kg_end > KGp) kg_end = KGp;

  RowInfo rows[RM];
#pragma unroll
  for (int i = 0; i < RM; ++i) rows[i] = make_row<MODE>(m0 + i * 16 + (lane & 15), g);

  f32x4 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int kq = lane >> 4;
  V8<T> ac[RM], bc[RN], an[RM], bn[RN];
  int kgi = kg_begin + kq;
  if (kg_begin < kg_end) {
#pragma unroll
    for (int i = 0; i < RM; ++i) load_a<T, MODE>(ac[i], rows[i], kgi, g);
#pragma unroll
    for (int j = 0; j < RN; ++j) load_b<T>(bc[j], kgi, n0 + j * 16 + (lane & 15), g);
  }
  for (int kb = kg_begin; kb < kg_end; kb += 4) {
    const int kn = kb + 4;
    if (kn < kg_end) {
      const int kgn = kn + kq;
#pragma unroll
      for (int i = 0; i < RM; ++i) load_a<T, MODE>(an[i], rows[i], kgn, g);
#pragma unroll
      for (int j = 0; j < RN; ++j) load_b<T>(bn[j], kgn, n0 + j * 16 + (lane & 15), g);
    }
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int j = 0; j < RN; ++j) mfma_step<T>(acc[i][j], ac[i], bc[j]);
    if (kn < kg_end) {
#pragma unroll
      for (int i = 0; i < RM; ++i) ac[i] = an[i];
#pragma unroll
      for (int j = 0; j < RN; ++j) bc[j] = bn[j];
    }
  }

  // epilogue: C/D layout col = lane&15, row = (lane>>4)*4 + r
  T* O = reinterpret_cast<T*>(g.out);
  const int Cout = (MODE == MODE_CONVT_FWD) ? (g.Ncols >> 3) : g.Ncols;
  if (g.ksplit > 1) {
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int j = 0; j < RN; ++j) {
        const int col = n0 + j * 16 + (lane & 15);
        if (col >= g.Ncols) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long row = m0 + i * 16 + (lane >> 4) * 4 + r;
          if (row < g.M) g.part[((long long)ks * g.M + row) * g.Ncols + col] = acc[i][j][r];
        }
      }
    return;
  }
  // stage the (BM x BN) tile through LDS so every lane stores 8 channels (16 B bf16) at once;
  // for the transposed conv an 8-column group is 8 channels of ONE child voxel (Cout % 8 == 0)
  constexpr int EPT = BN + 8;
  __shared__ __attribute__((aligned(16))) T El[BM * EPT];
  const long long mt0 = (long long)mt * BM;
  const int nt0 = nt * BN;
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) {
      const int lc = wn * RN * 16 + j * 16 + (lane & 15);
      const int col = nt0 + lc;
      float bv = 0.f;
      if (g.bias && col < g.Ncols) bv = g.bias[MODE == MODE_CONVT_FWD ? col % Cout : col];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = wm * RM * 16 + i * 16 + (lane >> 4) * 4 + r;
        El[lr * EPT + lc] = from_f<T>(acc[i][j][r] + bv);
      }
    }
  __syncthreads();
  constexpr int CG = BN / 8;
  const bool vec = g.ldo % 8 == 0 && g.Ncols % 8 == 0 && (reinterpret_cast<uintptr_t>(g.out) & 15) == 0;
  if (!vec) {   // odd strides: element-wise stores from the staged tile
    for (int e = threadIdx.x; e < BM * BN; e += 256) {
      const int lr = e / BN, lc = e % BN;
      const long long row = mt0 + lr;
      const int col = nt0 + lc;
      if (row >= g.M || col >= g.Ncols) continue;
      if (MODE == MODE_CONVT_FWD) {
        const int t = col / Cout, co = col - t * Cout;
        O[convt_child(row, t, g) * g.ldo + co] = El[lr * EPT + lc];
      } else {
        *out_at<T>(g, row, col) = El[lr * EPT + lc];
      }
    }
    return;
  }
  if constexpr (MODE == MODE_CONVT_FWD) {
    // a thread's 8-column group (tap t, channels co..co+7) is the same in every pass (256 % CG == 0) and its rows
    // step by 256 / CG: the child voxel's coordinates are decomposed once and then stepped, instead of three
    // runtime divisions per store (the epilogue was ~28 VALU per MFMA, r04i PMC)
    static_assert(256 % CG == 0, "fixed column group per thread");
    constexpr int LSTEP = 256 / CG;
    const int cg = threadIdx.x % CG;
    const int col = nt0 + cg * 8;
    if (col >= g.Ncols) return;
    const int t = col / Cout, co = col - t * Cout;
    const int tz = t >> 2, ty = (t >> 1) & 1, tx = t & 1;
    int lr = threadIdx.x / CG;
    const unsigned mu = (unsigned)(mt0 + lr);
    const unsigned q = mu / (unsigned)g.W, q2 = q / (unsigned)g.H;
    int x = (int)(mu - q * (unsigned)g.W), y = (int)(q - q2 * (unsigned)g.H);
    int n = (int)(q2 / (unsigned)g.D), z = (int)(q2 - (unsigned)n * (unsigned)g.D);
    const long long W2 = 2LL * g.W, H2 = 2LL * g.H, D2 = 2LL * g.D;
    for (; lr < BM; lr += LSTEP) {
      if (mt0 + lr >= g.M) break;
      V8<T> o;
      o.load(El + lr * EPT + cg * 8);
      const long long child = (((long long)n * D2 + 2 * z + tz) * H2 + 2 * y + ty) * W2 + 2 * x + tx;
      o.store(O + child * g.ldo + co);
      x += LSTEP;
      while (x >= g.W) {
        x -= g.W;
        if (++y == g.H) {
          y = 0;
          if (++z == g.D) {
            z = 0;
            ++n;
          }
        }
      }
    }
    return;
  }
  for (int e = threadIdx.x; e < BM * CG; e += 256) {
    const int lr = e / CG, cg = e % CG;
    const long long row = mt0 + lr;
    const int col = nt0 + cg * 8;
    if (row >= g.M || col >= g.Ncols) continue;
    V8<T> o;
    o.load(El + lr * EPT + cg * 8);
    if (MODE == MODE_POINT && g.res) {
      V8<T> rv;
      rv.load(reinterpret_cast<const T*>(g.res) + row * g.ldres + col);
#pragma unroll
      for (int j = 0; j < 8; ++j) o.set(j, o.get(j) + rv.get(j));
    }
    if (MODE == MODE_POINT && g.epi == 1) {
      V8<T> gv;
#pragma unroll
      for (int j = 0; j < 8; ++j) gv.set(j, mmseg_gelu(o.get(j)));
      gv.store(reinterpret_cast<T*>(g.aux_out) + row * g.ldo + col);
    } else if (MODE == MODE_POINT && g.epi == 2) {
      V8<T> hv;
      hv.load(reinterpret_cast<const T*>(g.aux) + row * g.ldo + col);
#pragma unroll
      for (int j = 0; j < 8; ++j) o.set(j, o.get(j) * mmseg_gelu_grad(hv.get(j)));
    }
    o.store(out_at<T>(g, row, col));
  }
}

// ---- the kernel choice of a forward / data-gradient GEMM launch.  choose_gemm is the only place that decides it:
// launch_gemm launches what it returns, and the planning queries (mmseg_conv3_splits, _group_ok, _norm_ok,
// _fp8_ok, _dgrad_in_chunks, mmseg_conv3_kernel) answer from it without a GPU.
// tsize: element bytes.  A grouped launch (g.grp_n > 0) takes the runtime-brick kernel even where the (4, 8, 8)-brick
// family fits: only it reads per-group weights (24^3 with MMSEG_GROUP_FORCE_R).  A deferred norm, IN-backward
// partials or e4m3 weights (g.nmean / g.inpart / g.wdq) are served by brick6 alone; the caller checks it got it.
GemmChoice choose_gemm(const GemmArgs& g, int mode, int tsize) {
  GemmChoice c{};
  c.block = 256;
  c.ksplit = g.ksplit;
  c.ks_want = 1;
  c.tsize = tsize;
  const bool bf16 = tsize == 2;
  if (mode == MODE_CONV3) {
    const int cin = 8 << g.cpg_shift, N = g.M / (g.D * g.H * g.W);
    const int brick = knob("MMSEG_BRICK", 2);
    const bool base_ok = cin % CK == 0 && g.lda % 8 == 0 && g.ldo % 8 == 0 && g.Ncols % 32 == 0;
    // 48-column multiples (SwinUNETR's feature_size 48) run the brick2 kernel with 48-column tiles
    const bool ok48 = cin % CK == 0 && g.lda % 8 == 0 && g.ldo % 8 == 0 && g.Ncols % 48 == 0;
    const bool out16 = g.ldo % 8 == 0 && (reinterpret_cast<uintptr_t>(g.out) & 15) == 0;   // 16-B output stores
    // 32-bit byte offsets into A; with them bf16 takes 32-bit offset halo staging (MMSEG_B32=0: the 64-bit staging)
    const bool a31 = (long long)g.M * g.lda * tsize < (1LL << 31);
    c.b32 = bf16 && knob("MMSEG_B32", 1) && a31;
    const int nb1 = N * (g.D / 4) * (g.H / B2_Y) * (g.W / B2_X);   // 4x8x8 bricks
    const bool fam = g.grp_n == 0 && brick == 2 && (base_ok || ok48) && g.D % 4 == 0 && g.H % B2_Y == 0 &&
                     g.W % B2_X == 0;
    // a brick2-family launch has one block per (4x8x8 brick, column tile): at SwinUNETR's 8^3 / 16^3 levels
    // (384 / 192 channels) that is 12-48 blocks for the whole chip (brick3 at 75-290 TF/s, r05m).  Below
    // MMSEG_BRICK2_MINUNITS such shapes take the runtime-brick kernel, whose chunk splits fill the CUs.
    const bool few = fam && base_ok && (long long)nb1 * ((g.Ncols + 63) / 64) < knob("MMSEG_BRICK2_MINUNITS", 128);
    if ((!fam || few) && brick >= 2 && base_ok) {
      int best = 0;
      for (int bz = 1; bz <= g.D && bz <= 8; ++bz) {
        if (g.D % bz) continue;
        for (int by = 1; by <= g.H && by <= 16; ++by) {
          if (g.H % by) continue;
          for (int bx = 1; bx <= g.W && bx <= 16; ++bx) {
            if (g.W % bx) continue;
            const int rows = bz * by * bx;
            const int halo = (bz + 2) * (by + 2) * (bx + 2);
            const int hq = (bz + 2) * (by + 2) * ((bx + 2) * 2 * tsize + 2);
            if (rows > 256 || halo > BR_MAXHV || hq > br_xq(tsize)) continue;
            const int score = rows * 4 + (bx % 8 == 0 ? 2 : 0) + (by % 8 == 0 ? 1 : 0);
            // ties go to the smaller halo (12^3: 6x6x6, 512 halo voxels and the compile-time kernel, over 3x6x12)
            const bool tie_better = score == best && halo < (c.bz + 2) * (c.by + 2) * (c.bx + 2);
            if (score > best || tie_better) {
              best = score;
              c.bz = bz; c.by = by; c.bx = bx;
            }
          }
        }
      }
      if (best >= 64 * 4) {   // at least a quarter of the 256-row tile in use
        c.kernel = GK_BRICKR;
        const int nb = N * (g.D / c.bz) * (g.H / c.by) * (g.W / c.bx);
        // 32-column tiles where 64-column ones leave fewer than 256 blocks: twice the blocks instead of a chunk split
        // (no fp32 partials, no reduce launch); 12^3 / 6^3 grouped: 2-8 us per launch (r04v convbench), -0.02 ms/step
        c.bn = (bf16 && g.Ncols % 64 == 0 && nb * (g.Ncols / 64) >= 256) ? 64 : 32;
        const int nt = (g.Ncols + c.bn - 1) / c.bn;
        const int slots = knob("MMSEG_BRICKR_SLOTS", 256);   // 512 measured 2-10 % slower at 12^3 / 6^3 (r02)
        const auto whole = [](int nchunk, int ks) {   // ks splits as equal ranges of whole chunks
          ks = std::max(1, std::min(ks, nchunk));
          const int cps = (nchunk + ks - 1) / ks;
          return (nchunk + cps - 1) / cps;
        };
        c.ks_want = whole(cin / CK, (slots + nb * nt - 1) / (nb * nt));
        const int nchunk = gemm_nchunk(g);
        c.ksplit = whole(nchunk, g.ksplit);
        // KW = 2: two waves per SIMD from an in-block split of the chunks (see the kernel); tap t + 1's fragments
        // read during tap t's MFMAs (PF: at 12^3 / 6^3 a CU holds one block; 5-10 % per launch, r04ab convbench)
        c.kw2 = bf16 && c.bn == 32 && c.bz == 6 && c.by == 6 && c.bx == 6 && (nchunk + c.ksplit - 1) / c.ksplit >= 2;
        c.name = c.bn == 64 ? "conv3_brickr_kernel<BN64>"
                 : c.kw2    ? "conv3_brickr_kernel<BN32,KW2>" : "conv3_brickr_kernel<BN32>";
        c.grid = nb * nt * c.ksplit;
        c.block = c.kw2 ? 512 : 256;
        c.reduce = c.ksplit > 1;
        return c;
      }
    }
    if (fam && g.ksplit == 1) {
      const int nchunk = gemm_nchunk(g);
      // launches only brick6 serves pass by brick8 and the 96-column rule on their way to it
      const bool only6 = g.nmean || g.inpart || g.wdq;
      // 8-wave 8x8x8 brick with LDS-DMA staging (conv3_brick8_kernel), bf16, 16-B output stores
      // (BN64: one 64-column tile over >= 2 input chunks, where it measured faster than brick2 BN64 -- 48^3
      // 64->64 fwd / dgrad 61 -> 55.5 us, 128->64 fwd 111 -> 98 us; with one chunk, or two column tiles, it was
      // slower: profiles/r03c_brick8_convbench.txt)
      const int b8 = knob("MMSEG_BRICK8", 1), nb8 = nb1 / 2;   // 8-deep bricks
      const bool b8_ok = bf16 && b8 && !only6 && g.H % 8 == 0 && g.W % 8 == 0 && out16 &&
                         (!g.out2 || g.ldo2 % 8 == 0) && a31 &&
                         (long long)((g.KG + 3) & ~3) * g.Cpad * 16 < (1LL << 31);
      c.kernel = GK_BRICK8;
      c.block = 512;
      if (b8_ok && g.Ncols % 64 == 0 && (b8 == 2 || (g.Ncols == 64 && nchunk >= 2)) && g.D % 8 == 0 &&
          nb8 * (g.Ncols / 64) >= knob("MMSEG_BRICK8_MINBLK", 256)) {
        c.name = "conv3_brick8_kernel<BN64>";
        c.bn = 64;
        c.grid = nb8 * (g.Ncols / 64);
        return c;
      }
      if (b8_ok && g.Ncols == 32 && g.D % 16 == 0 && nb8 / 2 >= knob("MMSEG_BRICK8_MINBLK", 256) && cin >= 64) {
        c.name = "conv3_brick8_kernel<BN32>";
        c.bn = 32;
        c.grid = nb8 / 2;
        return c;
      }
      c.block = 256;
      // v3 is bf16 only: its fp32 instantiation (f32 16x16x4 MFMA with swapped operands) returned the first
      // row of each 4-row accumulator group in all four registers (tools/diag_b3.py); the fp32 parity path
      // keeps the v2 kernel.
      const bool v3 = bf16 && a31;
      const bool wide = g.Ncols % 64 == 0 && nb1 * (g.Ncols / 64) >= knob("MMSEG_BRICK2_MINBLK", 512);
      // 48-column tiles also for multiples of 96 that are not of 64 (SwinUNETR's 96-column convs: two 48-column tiles
      // read the A halo twice, three 32-column brick3 tiles three times -- 128^3 96-column dgrad 0.74 ms at 706 TF/s
      // on brick3, r05c timer)
      if (g.Ncols % 32 != 0 || (!only6 && g.Ncols % 96 == 0 && g.Ncols % 64 != 0)) {   // a multiple of 48
        c.kernel = GK_BRICK2_BN48;
        c.name = "conv3_brick2_kernel<BN48,ZW1>";
        c.bn = 48;
        c.grid = nb1 * (g.Ncols / 48);
      } else if (v3 && nchunk == 1 && !wide) {
        // one persistent block per CU, each over a contiguous brick range of one 32-column tile; brick6 where its
        // 4x4x16 bricks divide the volume and the output takes 16-B stores
        const bool b6 = g.H % 4 == 0 && g.W % 16 == 0 && out16;
        const int nt_n = g.Ncols / 32;
        const int per_nt = std::max(1, knob("MMSEG_BRICK4_BLOCKS", 256) / nt_n);
        const int nb = b6 ? N * (g.D / 4) * (g.H / 4) * (g.W / 16) : nb1;
        c.kernel = b6 ? GK_BRICK6 : GK_BRICK4;
        c.name = !b6 ? "conv3_brick4_kernel<BN32>" : g.wdq ? "conv3_brick6_kernel<BN32,F8>"
                 : g.inpart ? "conv3_brick6_kernel<BN32,INP>" : "conv3_brick6_kernel<BN32>";
        c.bn = 32;
        c.upb = ceil_div(nb, std::min(per_nt, nb));
        c.bpn = ceil_div(nb, c.upb);
        c.grid = c.bpn * nt_n;
      } else if (v3 && !wide) {
        // persistent: at most one wave of resident blocks (2 per CU), each over a contiguous range of units
        const int units = nb1 * (g.Ncols / 32), maxblk = knob("MMSEG_BRICK3_BLOCKS", 512);
        c.kernel = GK_BRICK3;
        c.name = "conv3_brick3_kernel<BN32>";
        c.bn = 32;
        c.upb = maxblk > 0 ? ceil_div(units, maxblk) : 1;
        c.grid = ceil_div(units, c.upb);
      } else {
        // wide: each tap's fragments read while the previous tap's MFMAs run (2 % on the 48^3 64-channel layers, r02)
        c.kernel = GK_BRICK2;
        c.name = wide ? "conv3_brick2_kernel<BN64,ZW1>" : "conv3_brick2_kernel<BN32,ZW1>";
        c.bn = wide ? 64 : 32;
        c.grid = nb1 * (g.Ncols / c.bn);
      }
      return c;
    }
    // per-lane gather GEMM: enough (128 x 64|32) tiles to fill the chip
    const int tiles = ceil_div(g.M, 128) * ceil_div(g.Ncols, g.Ncols >= 64 ? 64 : 32);
    if (!fam && tiles < 512 && g.KG >= 32) c.ks_want = std::max(1, std::min(ceil_div(512, tiles), g.KG / 16));
    if (g.ksplit == 1 && brick == 1 && cin % CK == 0 && g.D % BRK_Z == 0 && g.H % BRK_Y == 0 && g.W % BRK_X == 0 &&
        g.lda % 8 == 0) {
      c.kernel = GK_BRICK1;
      c.bn = g.Ncols >= 64 ? 64 : 32;
      c.name = c.bn == 64 ? "conv3_brick_kernel<BN64>" : "conv3_brick_kernel<BN32>";
      c.grid = N * (g.D / BRK_Z) * (g.H / BRK_Y) * (g.W / BRK_X) * ceil_div(g.Ncols, c.bn);
      return c;
    }
  }
  // the gather GEMM's tiles (BM x BN)
  static const char* const nm32[4] = {"conv_gemm_kernel<conv3,128x32>", "conv_gemm_kernel<point,128x32>",
                                      "conv_gemm_kernel<convT_fwd,128x32>", "conv_gemm_kernel<convT_dgrad,128x32>"};
  static const char* const nm64[4] = {"conv_gemm_kernel<conv3,128x64>", "conv_gemm_kernel<point,128x64>",
                                      "conv_gemm_kernel<convT_fwd,128x64>", "conv_gemm_kernel<convT_dgrad,128x64>"};
  const bool point1 = mode == MODE_POINT && g.ksplit == 1;
  const auto pick = [&](int kernel, const char* name, int bn) { c.kernel = kernel; c.name = name; c.bn = bn; };
  int bm = 128;
  if (mode == MODE_CONVT_FWD && g.Ncols % 256 == 0) {
    // a block writes all 8 taps x 32 (or a quarter of 8 x 128 ...) output channels of its 64 input voxels, so
    // each input row is read by one block instead of by Ncols / 64 column tiles
    pick(GK_GEMM_64x256, "conv_gemm_kernel<convT_fwd,64x256>", 256);
    bm = 64;
  } else if (point1 && g.Ncols > 128 && g.Ncols <= 192 && g.Cpad >= 192) {
    // SwinUNETR's 144 / 192-column token linears (qkv, MLP fc1, fc2's data gradient) with every A row read by one
    // block -- 128x64 tiles re-read each K-wide row from L2 / HBM once per column tile
    pick(GK_GEMM_64x192, "conv_gemm_kernel<point,64x192>", 192);
    bm = 64;
  } else if (point1 && g.Ncols > 64 && g.Ncols <= 128 && g.Ncols % 96 != 0) {
    // 128-column outputs (the residual 1x1 convs' data gradients written as whole 96-of-128 rows) in one column
    // tile -- the 128x64 tile read every A row twice (the 128^3 decoder's: 295 us, r06k)
    pick(GK_GEMM_64x128, "conv_gemm_kernel<point,64x128>", 128);
    bm = 64;
  } else if (point1 && g.Ncols > 32 && g.Ncols <= 48 && g.Ncols % 16 == 0) {
    // the 48-column token linears / 1x1 convs (feature_size 48) in one column tile (BN=32 took two)
    pick(GK_GEMM_128x48, "conv_gemm_kernel<point,128x48>", 48);
  } else if (mode == MODE_POINT && g.Ncols % 96 == 0 && g.Ncols % 64 != 0) {
    // the 96 / 288 / 480-column 1x1 GEMMs (SwinUNETR's 96-channel stage, the 96 -> 48 residual conv's data
    // gradient) in whole tiles -- BN=64 left a half-empty last column tile that re-read every A row
    pick(GK_GEMM_128x96, "conv_gemm_kernel<point,128x96>", 96);
  } else if (g.Ncols < 64) {
    pick(GK_GEMM_128x32, nm32[mode], 32);
  } else {
    pick(GK_GEMM_128x64, nm64[mode], 64);
  }
  c.grid = ceil_div(g.M, bm) * ceil_div(g.Ncols, c.bn) * g.ksplit;
  c.reduce = g.ksplit > 1;
  return c;
}

// The shape fields of a launch's GemmArgs -- all choose_gemm reads besides the output pointers (null: 16-B aligned,
// unsplit) and the brick6-only inputs -- with the K range cut into ksplit ranges of whole groups of 4 k-groups.
GemmArgs gemm_shape(int M, int Ncols, int Cpad, int KG, int cpg_shift, int D, int H, int W, int lda, int ldo,
                    int ksplit = 1, int cin_real = 0) {
  GemmArgs g{};
  g.lda = lda; g.ldo = ldo; g.M = M; g.Ncols = Ncols; g.Cpad = Cpad; g.KG = KG; g.cpg_shift = cpg_shift;
  g.D = D; g.H = H; g.W = W;
  const int KGp = (KG + 3) & ~3;
  g.kg_per_split = ((ceil_div(KGp, ksplit) + 3) / 4) * 4;
  g.ksplit = ceil_div(KGp, g.kg_per_split);
  g.swz = 1;   // XCD-aware block remap
  g.kchunks = (cin_real + 31) / 32;
  return g;
}
// The planning queries: the choice of a 3^3 conv from its shape alone.  flags: what the launch would carry
// (ChoiceFlags, the bits of mmseg_conv3_kernel).
GemmChoice choose_conv3(int M, int Ncols, int Cpad, int KG, int cpg_shift, int D, int H, int W, int lda, int ldo,
                        int dtype, int flags = 0, int ksplit = 1, int cin_real = 0) {
  static float set = 0.f;   // any non-null address: choose_gemm only asks whether the launch carries these
  GemmArgs g = gemm_shape(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo, ksplit < 1 ? 1 : ksplit, cin_real);
  if (flags & CF_NORM) g.nmean = &set;
  if (flags & CF_INPART) g.inpart = &set;
  if (flags & CF_FP8) g.wdq = &set;
  g.grp_n = (flags & CF_GROUPS) ? 1 : 0;
  return choose_gemm(g, MODE_CONV3, dtype == MMSEG_BF16 ? 2 : 4);
}

// Every column tile of a conv launch reads weight columns [n0, n0 + BN) of the packed image [KGp][Cpad][8]: all of
// them must lie inside the image's pitch Cpad (the r05f GPU fault: a 192-column tile over a 96-column layer's
// 128-column image read 64 columns past it).  Checked on the host before each launch, with the kernel's name noted.
inline bool tile_in_pitch(const GemmArgs& g, int BN) { return (long long)((g.Ncols + BN - 1) / BN) * BN <= g.Cpad; }
#define MMSEG_TILE(G, NAME, BN)                                                                                   \
  do {                                                                                                           \
    MMSEG_REQUIRE(tile_in_pitch((G), (BN)), "%s: %d-column tiles over %d columns exceed the packed pitch %d", \
                  (const char*)(NAME), (int)(BN), (G).Ncols, (G).Cpad);                                          \
    mmseg::note_kernel(NAME);                                                                                    \
  } while (0)

// 4 consecutive columns per thread in gemm_splitk_reduce (for the transposed conv: 4 channels of one child voxel,
// Cout % 4 == 0)
template <int MODE>
__host__ __device__ __forceinline__ bool splitk_vec(const GemmArgs& g) {
  const bool al = (g.Ncols & 3) == 0 && (g.ldo & 3) == 0 && (reinterpret_cast<uintptr_t>(g.part) & 15) == 0;
  return MODE == MODE_CONVT_FWD ? al && ((g.Ncols >> 3) & 3) == 0 : al;
}
template <int MODE>
int splitk_reduce_blocks(const GemmArgs& g) {
  const long long total = (long long)g.M * g.Ncols;
  return ceil_div(splitk_vec<MODE>(g) ? (total + 3) / 4 : total, 256);
}

// Fixed-order split-K reduction for the forward GEMM: out = sum_k part[k] (+bias).
template <typename T, int MODE>
__global__ void gemm_splitk_reduce(GemmArgs g) {
  long long total = (long long)g.M * g.Ncols;
  if (MODE == MODE_CONVT_FWD && splitk_vec<MODE>(g)) {
    // 4 channels of one child voxel per thread: one child-index computation per 4 values (was one per value)
    const long long idx4 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (idx4 >= total) return;
    const long long row = idx4 / g.Ncols;
    const int col = (int)(idx4 - row * g.Ncols);
    const int Cout = g.Ncols >> 3, t = col / Cout, co = col - t * Cout;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4* p = reinterpret_cast<const float4*>(g.part + idx4);
    const long long st = total / 4;
#pragma unroll 4
    for (int k = 0; k < g.ksplit; ++k) {
      const float4 a = p[(long long)k * st];
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    }
    if (g.bias) {
      v.x += g.bias[co]; v.y += g.bias[co + 1]; v.z += g.bias[co + 2]; v.w += g.bias[co + 3];
    }
    T* O = reinterpret_cast<T*>(g.out) + convt_child(row, t, g) * g.ldo + co;
    O[0] = from_f<T>(v.x); O[1] = from_f<T>(v.y); O[2] = from_f<T>(v.z); O[3] = from_f<T>(v.w);
    return;
  }
  if (MODE != MODE_CONVT_FWD && splitk_vec<MODE>(g)) {
    // 4 consecutive columns per thread: 16-B partial loads, 4 splits' loads in flight, fixed split order
    const long long idx4 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (idx4 >= total) return;
    const long long row = idx4 / g.Ncols;
    const int col = (int)(idx4 - row * g.Ncols);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4* p = reinterpret_cast<const float4*>(g.part + idx4);
    const long long st = total / 4;
#pragma unroll 4
    for (int k = 0; k < g.ksplit; ++k) {
      const float4 a = p[(long long)k * st];
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    }
    if (g.bias) {
      const float* bp = g.grp_n > 0 ? g.bias + (int)(row / ((long long)g.D * g.H * g.W) / g.grp_n) * g.b_gstride
                                    : g.bias;
      v.x += bp[col]; v.y += bp[col + 1]; v.z += bp[col + 2]; v.w += bp[col + 3];
    }
    T* O = out_at<T>(g, row, col);
    O[0] = from_f<T>(v.x); O[1] = from_f<T>(v.y); O[2] = from_f<T>(v.z); O[3] = from_f<T>(v.w);
    return;
  }
  long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long long row = idx / g.Ncols;
  const int col = (int)(idx - row * g.Ncols);
  float v = 0.f;
  for (int k = 0; k < g.ksplit; ++k) v += g.part[(long long)k * total + idx];
  T* O = reinterpret_cast<T*>(g.out);
  if (MODE == MODE_CONVT_FWD) {
    const int Cout = g.Ncols >> 3;
    const int t = col / Cout, co = col - t * Cout;
    if (g.bias) v += g.bias[co];
    O[convt_child(row, t, g) * g.ldo + co] = from_f<T>(v);
  } else {
    if (g.bias)
      v += (g.grp_n > 0 ? g.bias + (int)(row / ((long long)g.D * g.H * g.W) / g.grp_n) * g.b_gstride : g.bias)[col];
    *out_at<T>(g, row, col) = from_f<T>(v);
  }
}

// Vectorised split-K reduce with the splits dealt over S slices of the block (256 / S float4 columns per
// block, ~4 splits per thread), slice sums a fixed pairwise LDS tree: at the small levels one thread per column
// walking 8..16 splits left the reduce latency-bound.  Same summation tree for every run (deterministic).
template <typename T, int S>
__global__ __launch_bounds__(256) void gemm_splitk_reduce_s(GemmArgs g) {
  constexpr int NC = 256 / S;
  __shared__ float4 red[S][NC];
  const long long total = (long long)g.M * g.Ncols;
  const int col4 = threadIdx.x % NC, sl = threadIdx.x / NC;
  const long long idx4 = ((long long)blockIdx.x * NC + col4) * 4;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (idx4 < total) {
    const float4* p = reinterpret_cast<const float4*>(g.part + idx4);
    const long long st = total / 4;
#pragma unroll 4
    for (int k = sl; k < g.ksplit; k += S) {
      const float4 a = p[(long long)k * st];
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    }
  }
  red[sl][col4] = v;
  __syncthreads();
#pragma unroll
  for (int h = S / 2; h > 0; h >>= 1) {
    if (sl < h) {
      const float4 a = red[sl + h][col4];
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
      red[sl][col4] = v;
    }
    __syncthreads();
  }
  if (sl != 0 || idx4 >= total) return;
  const long long row = idx4 / g.Ncols;
  const int col = (int)(idx4 - row * g.Ncols);
  if (g.bias) {
    const float* bp = g.grp_n > 0 ? g.bias + (int)(row / ((long long)g.D * g.H * g.W) / g.grp_n) * g.b_gstride
                                  : g.bias;
    v.x += bp[col]; v.y += bp[col + 1]; v.z += bp[col + 2]; v.w += bp[col + 3];
  }
  T* O = out_at<T>(g, row, col);
  O[0] = from_f<T>(v.x); O[1] = from_f<T>(v.y); O[2] = from_f<T>(v.z); O[3] = from_f<T>(v.w);
}

// ------------------------------------------------------------ host launch
template <typename T, int MODE>
int launch_splitk_reduce(const GemmArgs& g, hipStream_t s) {
  const long long total = (long long)g.M * g.Ncols;
  const bool vec = MODE != MODE_CONVT_FWD && splitk_vec<MODE>(g);   // (the sliced reduce: not the transposed conv)
  int S = 1;
  while (S < 16 && g.ksplit / (2 * S) >= 4) S *= 2;
  if (vec && S > 1) {
    const int nb = ceil_div(total / 4, 256 / S);
    if (S == 16) MMSEG_LAUNCH((gemm_splitk_reduce_s<T, 16>), dim3(nb), dim3(256), 0, s, g);
    else if (S == 8) MMSEG_LAUNCH((gemm_splitk_reduce_s<T, 8>), dim3(nb), dim3(256), 0, s, g);
    else if (S == 4) MMSEG_LAUNCH((gemm_splitk_reduce_s<T, 4>), dim3(nb), dim3(256), 0, s, g);
    else MMSEG_LAUNCH((gemm_splitk_reduce_s<T, 2>), dim3(nb), dim3(256), 0, s, g);
  } else {
    MMSEG_LAUNCH((gemm_splitk_reduce<T, MODE>), dim3(splitk_reduce_blocks<MODE>(g)), dim3(256), 0, s, g);
  }
  return mmseg::check_launch("gemm_splitk_reduce");
}

// Launch what choose_gemm chose (and the split-K reduce after it): one call per brick family, whose launcher sits
// next to its kernels, or the gather GEMM's tile.
template <typename T, int MODE>
int launch_gemm(GemmArgs g, hipStream_t s) {
  const GemmChoice c = choose_gemm(g, MODE, (int)sizeof(T));
  MMSEG_REQUIRE(!(g.nmean || g.inpart || g.wdq) || c.kernel == GK_BRICK6,
                "conv3 with a deferred norm, IN-backward partials or e4m3 weights needs the brick6 kernel for this "
                "shape (mmseg_conv3_norm_ok / _dgrad_in_chunks / _fp8_ok), not %s", c.name);
  MMSEG_REQUIRE(g.grp_n == 0 || c.kernel == GK_BRICKR,
                "grouped conv: only the runtime-brick kernel takes per-group weights (small volumes)");
  MMSEG_TILE(g, c.name, c.bn);
  g.ksplit = c.ksplit;
  const dim3 grid(c.grid), block(c.block);   // (the gather GEMM's cases)
  switch (c.kernel) {
    case GK_BRICKR:
      launch_brickr(g, c, s);
      break;
    case GK_BRICK8:
      if constexpr (sizeof(T) == 2) launch_brick8(g, c, s);
      break;
    case GK_BRICK6:
      launch_brick6(g, c, s);
      break;
    case GK_BRICK2_BN48:
    case GK_BRICK2:
    case GK_BRICK3:
    case GK_BRICK4:
    case GK_BRICK1:
      launch_brick2(g, c, s);
      break;
    case GK_GEMM_64x256:
      MMSEG_LAUNCH((conv_gemm_kernel<T, MODE, 1, 4, 4, 4>), grid, block, 0, s, g);
      break;
    case GK_GEMM_64x192:
      if constexpr (MODE == MODE_POINT) MMSEG_LAUNCH((conv_gemm_kernel<T, MODE, 1, 4, 4, 3>), grid, block, 0, s, g);
      break;
    case GK_GEMM_64x128:
      if constexpr (MODE == MODE_POINT) MMSEG_LAUNCH((conv_gemm_kernel<T, MODE, 1, 4, 4, 2>), grid, block, 0, s, g);
      break;
    case GK_GEMM_128x48:
      if constexpr (MODE == MODE_POINT) MMSEG_LAUNCH((conv_gemm_kernel<T, MODE, 4, 1, 2, 3>), grid, block, 0, s, g);
      break;
    case GK_GEMM_128x96:
      if constexpr (MODE == MODE_POINT) MMSEG_LAUNCH((conv_gemm_kernel<T, MODE, 2, 2, 4, 3>), grid, block, 0, s, g);
      break;
    case GK_GEMM_128x32:
      MMSEG_LAUNCH((conv_gemm_kernel<T, MODE, 4, 1, 2, 2>), grid, block, 0, s, g);
      break;
    case GK_GEMM_128x64:
      MMSEG_LAUNCH((conv_gemm_kernel<T, MODE, 2, 2, 4, 2>), grid, block, 0, s, g);
      break;
  }
  if (mmseg::check_launch(c.name)) return 1;
  return c.reduce ? launch_splitk_reduce<T, MODE>(g, s) : 0;
}

template <typename T>
int launch_gemm_mode(GemmArgs g, int mode, hipStream_t s) {
  switch (mode) {
    case MODE_CONV3: return launch_gemm<T, MODE_CONV3>(g, s);
    case MODE_POINT: return launch_gemm<T, MODE_POINT>(g, s);
    case MODE_CONVT_FWD: return launch_gemm<T, MODE_CONVT_FWD>(g, s);
    case MODE_CONVT_DGRAD: return launch_gemm<T, MODE_CONVT_DGRAD>(g, s);
  }
  mmseg::set_error("bad gemm mode %d", mode);
  return 1;
}

}  // namespace

// =================================================================== C ABI
extern "C" {

#ifdef MMSEG_TIMING_PROBES
// probe builds only (tools/convbench.py --probe): buffer of 8 * PROBE_NB + 32 * 16 * 64 longs, or null to stop
int mmseg_probe_set(long long* buf) {
  // (every source with probe points has its own g_probe; this one has none)
  return probe_set_brick2(buf) | probe_set_brick6(buf) | probe_set_brick8(buf);
}
#endif

// Generic implicit-GEMM: conv3 fwd / dgrad, 1x1, convT fwd / dgrad.
// cin_real: the A source's channels past cin_real are padding (zero weights), so the CONV3 brick kernels skip the
// 32-channel chunks wholly past it.  cin_real = 0: every channel is real.
int conv_gemm_impl(const void* a, int lda, const void* wpacked, const float* bias, void* out, int ldo, void* out2,
                   int ldo2, int split, float* splitk_ws, int mode, int M, int Ncols, int Cpad, int KG, int cpg_shift,
                   int D, int H, int W, int ksplit, int cin_real, int dtype, void* stream, int groups = 1,
                   long long w_gstride = 0, int b_gstride = 0, const void* res = nullptr, int ldres = 0,
                   int zcols = 0);

int mmseg_conv_gemm(const void* a, int lda, const void* wpacked, const float* bias, void* out, int ldo,
                    float* splitk_ws, int mode, int M, int Ncols, int Cpad, int KG, int cpg_shift, int D, int H, int W,
                    int ksplit, int dtype, void* stream) {
  return conv_gemm_impl(a, lda, wpacked, bias, out, ldo, nullptr, 0, 0, splitk_ws, mode, M, Ncols, Cpad, KG,
                        cpg_shift, D, H, W, ksplit, 0, dtype, stream);
}

// mmseg_conv_gemm over `groups` equal sample groups of A / out with their own packed weights (group gi:
// wpacked + gi * w_gstride elements) and bias (bias + gi * b_gstride): the modality encoders' small levels as one
// launch (+ one split-K reduce).  Runtime-brick CONV3 shapes only (small volumes).
int mmseg_conv_gemm_group(const void* a, int lda, const void* wpacked, const float* bias, void* out, int ldo,
                          float* splitk_ws, int mode, int M, int Ncols, int Cpad, int KG, int cpg_shift, int D, int H,
                          int W, int ksplit, int cin_real, int groups, long long w_gstride, int b_gstride, int dtype,
                          void* stream) {
  MMSEG_REQUIRE(mode == MODE_CONV3 && groups >= 1 && M % (groups * D * H * W) == 0,
                "conv_gemm_group: CONV3 over groups x whole samples");
  return conv_gemm_impl(a, lda, wpacked, bias, out, ldo, nullptr, 0, 0, splitk_ws, mode, M, Ncols, Cpad, KG, cpg_shift,
                        D, H, W, ksplit, cin_real, dtype, stream, groups, w_gstride, b_gstride);
}

// mmseg_conv_gemm (channel-padded A source: cin_real) with the whole-row output hint: columns [Ncols, zcols) of the
// output rows are written as zeros by the kernels that support it (the brick2 conv kernels), left alone by the others.
int mmseg_conv_gemm_zw(const void* a, int lda, const void* wpacked, const float* bias, void* out, int ldo,
                       float* splitk_ws, int mode, int M, int Ncols, int Cpad, int KG, int cpg_shift, int D, int H,
                       int W, int ksplit, int cin_real, int zcols, int dtype, void* stream) {
  return conv_gemm_impl(a, lda, wpacked, bias, out, ldo, nullptr, 0, 0, splitk_ws, mode, M, Ncols, Cpad, KG,
                        cpg_shift, D, H, W, ksplit, cin_real, dtype, stream, 1, 0, 0, nullptr, 0, zcols);
}

// 1x1 GEMM (MODE_POINT, ksplit 1) with the MLP's GELU in its epilogue: epi 1, out = h = A W^T + bias and gelu_out
// = gelu(h) (linear1 + GELU); epi 2, out = (A W^T) * gelu'(h) with h = gelu_in (linear2's data gradient through the
// GELU) -- bitwise the GEMM followed by mmseg_gelu_fwd / mmseg_gelu_bwd.  out, gelu_in / gelu_out at pitch ldo.
int mmseg_conv_gemm_gelu(const void* a, int lda, const void* wpacked, const float* bias, void* out, int ldo,
                         const void* gelu_in, void* gelu_out, int epi, int M, int Ncols, int Cpad, int KG, int dtype,
                         void* stream) {
  MMSEG_REQUIRE((epi == 1 && gelu_out && !gelu_in) || (epi == 2 && gelu_in && !gelu_out),
                "conv_gemm_gelu: epi 1 (forward, gelu_out) or 2 (backward, gelu_in)");
  MMSEG_REQUIRE(ldo % 8 == 0 && Ncols % 8 == 0 &&
                    ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(gelu_in) |
                      reinterpret_cast<uintptr_t>(gelu_out)) & 15) == 0,
                "conv_gemm_gelu: ldo, Ncols multiples of 8, 16-B aligned buffers");
  GemmArgs g = gemm_shape(M, Ncols, Cpad, KG, 0, 1, 1, 1, lda, ldo);
  g.a = a; g.b = wpacked; g.bias = bias; g.out = out;
  MMSEG_REQUIRE(lda % 8 == 0, "conv_gemm_gelu: lda must be a multiple of 8");
  MMSEG_REQUIRE(Cpad >= ((Ncols + (Ncols >= 64 ? 63 : 31)) / (Ncols >= 64 ? 64 : 32)) * (Ncols >= 64 ? 64 : 32),
                "conv_gemm_gelu: packed weights must be padded to the column tile (Cpad=%d, Ncols=%d)", Cpad, Ncols);
  g.epi = epi;
  g.aux = gelu_in;
  g.aux_out = gelu_out;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MMSEG_BF16) return launch_gemm<bf16_t, MODE_POINT>(g, s);
  return launch_gemm<float, MODE_POINT>(g, s);
}

// 1x1 GEMM (MODE_POINT, ksplit 1) whose epilogue adds a residual: out = round(round(A W^T + bias) + res), bitwise
// mmseg_conv_gemm into a temporary followed by mmseg_add(res, temporary, out); res may alias out.  The SwinUNETR
// residual sums (UnetResBlock input gradient dx += d(conv3 branch), the MLP residual x + fc2(.)) without a pass.
int mmseg_conv_gemm_res(const void* a, int lda, const void* wpacked, const float* bias, const void* res, int ldres,
                        void* out, int ldo, int M, int Ncols, int Cpad, int KG, int dtype, void* stream) {
  MMSEG_REQUIRE(res != nullptr, "conv_gemm_res: residual required");
  return conv_gemm_impl(a, lda, wpacked, bias, out, ldo, nullptr, 0, 0, nullptr, MODE_POINT, M, Ncols, Cpad, KG, 0, 1,
                        1, 1, 1, 0, dtype, stream, 1, 0, 0, res, ldres);
}

// mmseg_conv_gemm (channel-padded A source: cin_real) whose output columns [split, Ncols) go to a second tensor out2
// (row pitch ldo2) as columns 0..: the decoder's first-conv data gradient writes d(upsampled) and d(skip) dense.
int mmseg_conv_gemm_split(const void* a, int lda, const void* wpacked, const float* bias, void* out, int ldo,
                          void* out2, int ldo2, int split, float* splitk_ws, int mode, int M, int Ncols, int Cpad,
                          int KG, int cpg_shift, int D, int H, int W, int ksplit, int cin_real, int dtype,
                          void* stream) {
  MMSEG_REQUIRE(out2 && split > 0 && split < Ncols && split % 8 == 0 && ldo2 % 8 == 0 && ldo % 8 == 0 &&
                    (reinterpret_cast<uintptr_t>(out2) & 15) == 0 && mode != MODE_CONVT_FWD,
                "conv_gemm_split: split %d must be a multiple of 8 inside (0, %d), ldo / ldo2 multiples of 8, out2 "
                "16-B aligned", split, Ncols);
  return conv_gemm_impl(a, lda, wpacked, bias, out, ldo, out2, ldo2, split, splitk_ws, mode, M, Ncols, Cpad, KG,
                        cpg_shift, D, H, W, ksplit, cin_real, dtype, stream);
}

int conv_gemm_impl(const void* a, int lda, const void* wpacked, const float* bias, void* out, int ldo, void* out2,
                   int ldo2, int split, float* splitk_ws, int mode, int M, int Ncols, int Cpad, int KG, int cpg_shift,
                   int D, int H, int W, int ksplit, int cin_real, int dtype, void* stream, int groups,
                   long long w_gstride, int b_gstride, const void* res, int ldres, int zcols) {
  MMSEG_REQUIRE(zcols == 0 || (zcols >= Ncols && zcols % 8 == 0 && zcols <= ldo && !out2 && Ncols % 8 == 0 &&
                               zcols - Ncols <= 48),
                "conv_gemm: whole-row extent zcols=%d must lie in [Ncols, min(ldo, Ncols + 48)]", zcols);
  MMSEG_REQUIRE(!res || (mode == MODE_POINT && ksplit == 1 && !out2 && ldo % 8 == 0 && ldres % 8 == 0 &&
                         Ncols % 8 == 0 && ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(res)) &
                                            15) == 0),
                "conv_gemm_res: MODE_POINT, ksplit 1, pitches and Ncols multiples of 8, 16-B aligned out / res");
  MMSEG_REQUIRE(cin_real >= 0 && cin_real <= (8 << cpg_shift), "conv_gemm: cin_real %d outside [0, %d]", cin_real,
                8 << cpg_shift);
  MMSEG_REQUIRE(lda % 8 == 0 && ldo >= 1, "conv_gemm: lda must be a multiple of 8 (got %d)", lda);
  MMSEG_REQUIRE(Cpad >= ((Ncols + (Ncols >= 64 ? 63 : 31)) / (Ncols >= 64 ? 64 : 32)) * (Ncols >= 64 ? 64 : 32),
                "conv_gemm: packed weights must be padded to the column tile (Cpad=%d, Ncols=%d)", Cpad, Ncols);
  MMSEG_REQUIRE(ksplit >= 1, "conv_gemm: ksplit >= 1");
  MMSEG_REQUIRE(ksplit == 1 || splitk_ws != nullptr, "conv_gemm: split-K needs a workspace");
  GemmArgs g = gemm_shape(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo, ksplit, mode == MODE_CONV3 ? cin_real : 0);
  g.a = a; g.b = wpacked; g.bias = bias; g.out = out; g.part = splitk_ws;
  g.out2 = out2; g.ldo2 = ldo2; g.split = split;
  if (groups > 1) {
    g.grp_n = M / (D * H * W) / groups;
    g.w_gstride = w_gstride;
    g.b_gstride = b_gstride;
  }
  g.res = res;
  g.ldres = ldres;
  g.zcols = zcols;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MMSEG_BF16) return launch_gemm_mode<bf16_t>(g, mode, s);
  return launch_gemm_mode<float>(g, mode, s);
}

// 1 when mmseg_conv3_fwd_norm can run this shape (the brick6 kernel, the only conv forward that applies a
// deferred InstanceNorm + ReLU to its input): bf16, one 32-channel input chunk, 32 output columns, W % 16.
int mmseg_conv3_norm_ok(int M, int Ncols, int Cpad, int KG, int cpg_shift, int D, int H, int W, int lda, int ldo,
                        int dtype) {
  if (dtype != MMSEG_BF16 || !knob("MMSEG_DEFER_CONV_NORM", 1)) return 0;
  return choose_conv3(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo, dtype, CF_NORM).kernel == GK_BRICK6;
}

// 3^3 conv forward of an A source holding the PRE-norm activation of an InstanceNorm + ReLU: the kernel stages
// relu((a - nmean[n][c]) * nrstd[n][c]) rounded to bf16, exactly the values mmseg_instnorm_relu_fwd would
// write, so that output never has to be materialised (requires mmseg_conv3_norm_ok).
int mmseg_conv3_fwd_norm(const void* a, int lda, const float* nmean, const float* nrstd, const void* wpacked,
                         const float* bias, void* out, int ldo, int M, int Ncols, int Cpad, int KG, int cpg_shift,
                         int D, int H, int W, int dtype, void* stream) {
  MMSEG_REQUIRE(nmean && nrstd && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
                    mmseg_conv3_norm_ok(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo, dtype),
                "conv3_fwd_norm: unsupported shape (mmseg_conv3_norm_ok)");
  GemmArgs g = gemm_shape(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo);
  g.a = a; g.b = wpacked; g.bias = bias; g.out = out; g.nmean = nmean; g.nrstd = nrstd;
  return launch_gemm<bf16_t, MODE_CONV3>(g, (hipStream_t)stream);
}

// Mixed bf16/fp8 forward (config c5): the brick6 shapes of a 3^3 conv with e4m3 operands and fp32 accumulation.
int mmseg_conv3_fp8_ok(int M, int Ncols, int Cpad, int KG, int cpg_shift, int D, int H, int W, int lda, int ldo) {
  return choose_conv3(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo, MMSEG_BF16, CF_FP8).kernel == GK_BRICK6;
}

// out = conv3(A) with e4m3 operands (A: bf16 NDHWC, staged as e4m3; with nmean / nrstd: relu((a - mean) * rstd)
// first, as mmseg_conv3_fwd_norm), bf16 output; w8 / wdq from mmseg_pack_conv3_fp8 (requires mmseg_conv3_fp8_ok).
int mmseg_conv3_fwd_fp8(const void* a, int lda, const float* nmean, const float* nrstd, const void* w8,
                        const float* wdq, const float* bias, void* out, int ldo, int M, int Ncols, int Cpad, int KG,
                        int cpg_shift, int D, int H, int W, void* stream) {
  MMSEG_REQUIRE(a && w8 && wdq && out && (nmean == nullptr) == (nrstd == nullptr) &&
                    (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
                    mmseg_conv3_fp8_ok(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo),
                "conv3_fwd_fp8: unsupported shape (mmseg_conv3_fp8_ok)");
  GemmArgs g = gemm_shape(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo);
  g.a = a; g.b = w8; g.bias = bias; g.out = out; g.nmean = nmean; g.nrstd = nrstd; g.wdq = wdq;
  return launch_gemm<bf16_t, MODE_CONV3>(g, (hipStream_t)stream);
}

// Chunks per sample of the InstanceNorm-backward partials mmseg_conv3_dgrad_in writes for this CONV3 data-gradient
// shape (the brick6 kernel's blocks per column tile), or 0 when that kernel does not run it.
int mmseg_conv3_dgrad_in_chunks(int M, int Ncols, int Cpad, int KG, int cpg_shift, int D, int H, int W, int lda,
                                int ldo, int dtype) {
  const GemmChoice c = choose_conv3(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo, dtype, CF_INPART);
  return c.kernel == GK_BRICK6 ? c.bpn : 0;
}

// CONV3 data gradient (mmseg_conv_gemm, ksplit 1, no bias) whose output dy feeds the backward of an InstanceNorm +
// ReLU with pre-norm input inx (pitch ldinx) and statistics inmean / inrstd [N][Ncols]: the kernel also writes that
// backward's partial sums inpart [N][mmseg_conv3_dgrad_in_chunks()][Ncols][2] (the layout mmseg_instnorm_bwd_part
// reads), so its partial pass over x and dy is skipped.
int mmseg_conv3_dgrad_in(const void* a, int lda, const void* wpacked, void* out, int ldo, int M, int Ncols, int Cpad,
                         int KG, int cpg_shift, int D, int H, int W, const void* inx, int ldinx, const float* inmean,
                         const float* inrstd, float* inpart, int dtype, void* stream) {
  MMSEG_REQUIRE(inx && inmean && inrstd && inpart && ldinx % 8 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
                    mmseg_conv3_dgrad_in_chunks(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo, dtype) > 0,
                "conv3_dgrad_in: unsupported shape (mmseg_conv3_dgrad_in_chunks)");
  GemmArgs g = gemm_shape(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo);
  g.a = a; g.b = wpacked; g.out = out;
  g.inx = inx; g.ldinx = ldinx; g.inmean = inmean; g.inrstd = inrstd; g.inpart = inpart;
  return launch_gemm<bf16_t, MODE_CONV3>(g, (hipStream_t)stream);
}

// 1 when mmseg_conv_gemm_group takes this shape: the runtime-brick conv (mmseg_conv3_wgrad_group_ok, conv_wgrad.hip,
// answers for the weight gradient).
// (a grouped launch takes the runtime-brick kernels; MMSEG_GROUP_FORCE_R (default on) also groups shapes that would
// otherwise take the (4, 8, 8)-brick family -- the 24^3 / 48^3 levels: one launch over both modalities on the
// runtime-brick kernels beat two on the brick family there, r04j / r04l / r04n A/B -0.05..-0.07 ms per step)
int mmseg_conv3_group_ok(int M, int Ncols, int Cpad, int KG, int cpg_shift, int D, int H, int W, int lda, int ldo,
                         int dtype) {
  if (!knob("MMSEG_GROUP_SMALL", 1)) return 0;
  if (choose_conv3(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo, dtype).kernel == GK_BRICKR) return 1;
  return knob("MMSEG_GROUP_FORCE_R", 1) &&
         choose_conv3(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo, dtype, CF_GROUPS).kernel == GK_BRICKR;
}
// split count of a grouped conv (mmseg_conv_gemm_group): the runtime-brick kernel's
int mmseg_conv3_group_splits(int M, int Ncols, int Cpad, int KG, int cpg_shift, int D, int H, int W, int lda, int ldo,
                             int dtype) {
  const GemmChoice c = choose_conv3(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo, dtype, CF_GROUPS);
  return c.kernel == GK_BRICKR ? c.ks_want : 1;
}

// Number of K splits the CONV3 path wants for this shape (callers size the
// split-K workspace, ksplit*M*Ncols floats, with it and pass it as ksplit).
int mmseg_conv3_splits(int M, int Ncols, int Cpad, int KG, int cpg_shift, int D, int H, int W, int lda, int ldo,
                       int dtype) {
  return choose_conv3(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo, dtype).ks_want;
}

// The family name (mmseg_last_kernel()) a 3^3 conv forward / data gradient of this shape would launch with split
// count ksplit; flags: 1 deferred norm, 2 IN-backward partials, 4 e4m3 weights, 8 grouped.
const char* mmseg_conv3_kernel(int M, int Ncols, int Cpad, int KG, int cpg_shift, int D, int H, int W, int lda,
                               int ldo, int cin_real, int ksplit, int flags, int dtype) {
  return choose_conv3(M, Ncols, Cpad, KG, cpg_shift, D, H, W, lda, ldo, dtype, flags, ksplit, cin_real).name;
}

}  // extern "C"
