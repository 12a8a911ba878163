// conv3_brick6_kernel: the W % 16, one-input-chunk, 32-column 3^3 conv (the 96^3 32 -> 32 layers), with its
// deferred-norm, e4m3 and IN-backward-partial forms, and its launcher.
#include "conv_common.h"

namespace {

// ------------------------------------------------- brick conv v6 (3^3, bf16, Cin = 32, Co tile 32)
// brick4 with the A-read stream halved.  A row tile is 16 consecutive x voxels of ONE y row (brick 4 z x
// 4 y x 16 x, one z plane per wave), so the fragment of row tile i at tap ky is the fragment of halo row
// i + ky: per (kz, kx) the 12 (ky, i) fragments are 6 distinct halo rows, read once and used by 24 MFMAs
// (0.25 ds_read_b128 per MFMA instead of 0.5).  Halo image: voxel = 4 quads of 8 channels, the quad of
// channel group kg at slot kg ^ (((hx >> 2) & 1) << 1), which makes the 16-lane groups of ds_read_b128
// conflict-free for all three kx shifts; rows of 18 voxels, no padding.
// Requirements (host): bf16, one 32-channel K chunk, Ncols % 32 == 0, D % 4, H % 4, W % 16.
// Its predecessor v5 (same layout, same arithmetic, bitwise the same outputs; removed) measured ~8,000 cycles per
// brick against 3,456 of MFMA issue (r03s, 96^3 B=2 32->32 forward, one wave per SIMD).  hipcc emitted each group's
// halo staging (the deferred norm's VALU work and its ds_writes), the next group's fragment reads and the previous
// brick's epilogue as blocks BETWEEN the groups' MFMA runs, and an MFMA run at one wave per SIMD leaves only 8 of
// every 16 cycles to other instructions -- when those come as a block, the matrix pipe idles for the whole block.  v6
// cuts every group into 8 chunks of 3 MFMAs separated by sched_barrier(0), each chunk carrying a fixed share of the
// rest: one of the next group's 6 fragment reads, a row of the next brick's halo loads (groups 0-1), one 2-channel
// pair of a staged row's deferred norm (groups SG0..8, row written to LDS with its fourth pair) or one row of the
// previous brick's epilogue (group 0).  The steady state has no branches: NORM is a template parameter, out-of-volume
// rows are zeroed by a mask instead of a branch, the 40 threads without a halo column write a dummy LDS slot, the
// last brick re-stages itself, and the first brick's group-0 epilogue writes bias-only values that the next brick's
// epilogue (same lanes, same addresses) overwrites.
// INP (data gradient, no bias): the epilogue also sums the InstanceNorm-backward partials of its output
// (GemmArgs::inpart; fixed per-lane order); the x of a brick's output voxels is loaded in its group 4, its partial
// sums are formed in the next brick's group 1.
// F8 (forward only; mixed bf16/fp8 of config c5): the halo is staged as OCP e4m3 (the first 8 bytes of each 16-B
// quad, read by ds_read_b64), the weights come as e4m3 w * s[co] (mmseg_pack_conv3_fp8) and the MFMA is
// v_mfma_f32_16x16x32_fp8_fp8 with fp32 accumulation; the epilogue multiplies by g.wdq[co] = 1 / s[co].
template <bool NORM, int SG0 = 3, bool INP = false, bool F8 = false>
__global__ __launch_bounds__(256, 1) void conv3_brick6_kernel(GemmArgs g, int upb, int blocks_per_nt) {
  PROBE_BLOCK(false);
  using T = bf16_t;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  constexpr int BZ = 4, BY = 4, BX = 16;
  constexpr int HZ = BZ + 2, HY = BY + 2, HX = BX + 2;
  constexpr int RY = HX * 4, RZ = HY * RY;             // quads per halo row / plane
  constexpr int XQ = HZ * RZ;                          // 2592 quads = 41.5 KB
  constexpr int RN = 2;
  constexpr int XROWS = HZ * HY;                       // 36 (z, y) halo rows
  constexpr int XK = XROWS / 3;                        // rows per thread (3 rows per pass of 216 threads)
  constexpr int NSG = 9 - SG0;                         // groups that write staged rows
  constexpr int RPG = (XK + NSG - 1) / NSG;            // rows per such group
  constexpr int PPC = RPG / 2;                         // norm pairs per chunk (4 pairs per row, 8 chunks)
  static_assert(RPG % 2 == 0 && NSG * RPG >= XK && SG0 >= 2, "SG0: 3, 6 or 7");
  constexpr int EPQ = 8;
  __shared__ __attribute__((aligned(16))) float4 lds4[2 * XQ + 64];
  T* Xl = reinterpret_cast<T*>(lds4);

  const T* Bw = reinterpret_cast<const T*>(g.b);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bz_n = g.D / BZ, by_n = g.H / BY, bx_n = g.W / BX;
  const int nbrick = (g.M / (g.D * g.H * g.W)) * bz_n * by_n * bx_n;
  const int blk_all = g.swz ? xcd_swizzle(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int nt = blk_all / blocks_per_nt, blk = blk_all - nt * blocks_per_nt;
  const int n0 = nt * 32;
  const int u_begin = blk * upb;
  const int u_end = u_begin + upb < nbrick ? u_begin + upb : nbrick;
  // INP: zero partials for the samples outside the block's unit range [n_lo, n_hi] (the consumer sums every
  // block's slot of every sample; this replaces a memset of the whole partial buffer before the launch)
  auto inp_zero = [&](int n_lo, int n_hi) {
    if constexpr (INP) {
      const int nsamp = g.M / (g.D * g.H * g.W);
      if (tid < 32 && n0 + tid < g.Ncols)
        for (int n = 0; n < nsamp; ++n)
          if (n < n_lo || n > n_hi) {
            float* p = g.inpart + (((long long)n * blocks_per_nt + blk) * g.Ncols + n0 + tid) * 2;
            p[0] = 0.f;
            p[1] = 0.f;
          }
    }
  };
  if (u_begin >= u_end || n0 >= g.Ncols) {
    inp_zero(0, -1);
    return;
  }
  const int HW = g.H * g.W;
  const int cin = 8 << g.cpg_shift;
  const int ldb = g.lda * (int)sizeof(T);
  const int vox_per_n = g.D * HW;
  const int r16 = lane & 15, kg = lane >> 4;

  V8<T> wf[F8 ? 1 : 27][RN];
  long wf8[F8 ? 27 : 1][RN];
  if constexpr (F8) {
    const long* B8 = reinterpret_cast<const long*>(g.b);
#pragma unroll
    for (int t = 0; t < 27; ++t)
#pragma unroll
      for (int j = 0; j < RN; ++j)
        wf8[t][j] = B8[(long long)(t * (cin / 8) + kg) * g.Cpad + n0 + 8 * (r16 >> 2) + 4 * j + (r16 & 3)];
#pragma unroll
    for (int t = 0; t < 27; ++t) asm volatile("s_nop 2" : "+a"(wf8[t][0]), "+a"(wf8[t][1]));
  } else {
#pragma unroll
    for (int t = 0; t < 27; ++t)
#pragma unroll
      for (int j = 0; j < RN; ++j)
        wf[t][j].load(Bw + ((long long)(t * (cin / 8) + kg) * g.Cpad + n0 + 8 * (r16 >> 2) + 4 * j + (r16 & 3)) * 8);
#pragma unroll
    for (int t = 0; t < 27; ++t) brick4_wfence(wf[t][0].v, wf[t][1].v);
  }

  const __amdgpu_buffer_rsrc_t arsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(g.a), 0, (int)((long long)(g.M / vox_per_n) * vox_per_n * ldb), 0x00020000);
  const bool xact = tid < 216;
  const int xq = tid % 72, r0 = tid / 72;
  const int hx = xq >> 2, cg = xq & 3;
  const int xlds0 = (hx * 4 + (cg ^ (((hx >> 2) & 1) << 1))) * EPQ;
  // LDS destination of staged row k in buffer b: xs0 + b * xsb + k * xsk (idle threads: a dummy slot)
  const int xs0 = xact ? xlds0 + r0 * RY * EPQ : (2 * XQ + (tid & 63)) * EPQ;
  const int xsk = xact ? 3 * RY * EPQ : 0;
  const int xsb = xact ? XQ * EPQ : 0;
  struct Unit { int n, z0, y0, x0; };
  auto unit_of = [&](int b) {
    Unit r;
    const int bx = b % bx_n; b /= bx_n;
    const int by = b % by_n; b /= by_n;
    r.z0 = (b % bz_n) * BZ;
    r.n = b / bz_n;
    r.y0 = by * BY;
    r.x0 = bx * BX;
    return r;
  };
  V8<T> xr[XK];
  uint32_t rel[XK];
#pragma unroll
  for (int k = 0; k < XK; ++k) {
    const int row = r0 + 3 * k, hz = row / HY, hy = row - hz * HY;
    rel[k] = (uint32_t)((hz * HW + hy * g.W + hx) * ldb + cg * 16);
  }
  uint32_t xo[XK], om[XK];
  float nmu[8], nrs[8];
  int norm_n = -1;
  auto set_x = [&](const Unit& q) {
    if constexpr (NORM) {
      if (q.n != norm_n) {
        norm_n = q.n;
        const int cb = q.n * cin + cg * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          nmu[j] = g.nmean[cb + j];
          nrs[j] = g.nrstd[cb + j];
        }
      }
    }
    const int xx = q.x0 - 1 + hx;
    const bool xok = xact && (unsigned)xx < (unsigned)g.W;
    const int ob = ((q.n * g.D + q.z0 - 1) * g.H + q.y0 - 1) * g.W + q.x0 - 1;
    const uint32_t base = (uint32_t)(ob * ldb);
    if (q.z0 >= 1 && q.z0 + BZ < g.D && q.y0 >= 1 && q.y0 + BY < g.H) {
#pragma unroll
      for (int k = 0; k < XK; ++k) xo[k] = xok ? base + rel[k] : 0x80000000u;
    } else {
#pragma unroll
      for (int k = 0; k < XK; ++k) {
        const int row = r0 + 3 * k, hz = row / HY, hy = row - hz * HY;
        const int zz = q.z0 - 1 + hz, yy = q.y0 - 1 + hy;
        const bool ok = xok && (unsigned)zz < (unsigned)g.D && (unsigned)yy < (unsigned)g.H;
        xo[k] = ok ? base + rel[k] : 0x80000000u;
      }
    }
#pragma unroll
    for (int k = 0; k < XK; ++k) om[k] = xo[k] != 0x80000000u ? ~0u : 0u;
  };
  auto load_row = [&](int k) { buf_load_v8<T>(xr[k], arsrc, xo[k]); };
  // deferred norm of channels 2p, 2p+1 of staged row k: in_relu_apply's operations; out-of-volume rows stay 0
  u32x4 sv[RPG];
  auto norm_pair = [&](int k, int p, u32x4& o) {
    float ha = (xr[k].get(2 * p) - nmu[2 * p]) * nrs[2 * p];
    float hb = (xr[k].get(2 * p + 1) - nmu[2 * p + 1]) * nrs[2 * p + 1];
    ha = ha > 0.f ? ha : 0.f;
    hb = hb > 0.f ? hb : 0.f;
    if constexpr (F8) {   // pairs 0, 1 -> dword 0 (low, high word), 2, 3 -> dword 1
      if (p & 1) o[p >> 1] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(ha, hb, (int)o[p >> 1], true) & om[k];
      else o[p >> 1] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(ha, hb, 0, false);
    } else {
      const bf16x2 h2 = {(__bf16)ha, (__bf16)hb};
      o[p] = __builtin_bit_cast(uint32_t, h2) & om[k];
    }
  };
  auto to_f8 = [&](int k, u32x4& o) {   // raw staged row (no norm) -> e4m3 (out-of-volume lanes read 0 -> 0)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(xr[k].get(4 * d), xr[k].get(4 * d + 1), 0, false);
      o[d] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(xr[k].get(4 * d + 2), xr[k].get(4 * d + 3), lo, true);
    }
  };
  auto store_row = [&](int buf, int k, const u32x4& o) {
    if constexpr (F8) {
      typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
      *reinterpret_cast<u32x2*>(Xl + buf * xsb + xs0 + k * xsk) = (u32x2){o[0], o[1]};
    } else {
      *reinterpret_cast<u32x4*>(Xl + buf * xsb + xs0 + k * xsk) = o;
    }
  };
  auto stage_row = [&](int buf, int k) {   // whole row (prologue)
    u32x4 o;
    if constexpr (NORM) {
#pragma unroll
      for (int p = 0; p < 4; ++p) norm_pair(k, p, o);
    } else if constexpr (F8) {
      to_f8(k, o);
    } else {
      o = __builtin_bit_cast(u32x4, xr[k].v);
    }
    store_row(buf, k, o);
  };
  int ao[3];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
    const int h = r16 + kx;
    ao[kx] = wave * RZ + h * 4 + (kg ^ (((h >> 2) & 1) << 1));
  }
  float bv[RN][4], dq[F8 ? RN : 1][4];
#pragma unroll
  for (int j = 0; j < RN; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bv[j][r] = g.bias ? g.bias[n0 + 8 * kg + 4 * j + r] : 0.f;
      if constexpr (F8) dq[j][r] = g.wdq[n0 + 8 * kg + 4 * j + r];
    }

  f32x4 ev[BY][RN];
#pragma unroll
  for (int i = 0; i < BY; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) ev[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // row i of a finished brick: lane holds channels n0 + 8 kg + 4 j + (0..3) of voxel (z0 + wave, y0 + i, x0 + r16)
  bf16x8 eo[BY];   // the stored rows (INP: their partial sums follow one group later)
  auto epi_row = [&](const Unit& q, int i) {
    const long long obase = (long long)q.n * vox_per_n;
    const int z = q.z0 + wave, y = q.y0 + i, x = q.x0 + r16;
    T* dst = out_at<T>(g, obase + (long long)(z * g.H + y) * g.W + x, n0 + 8 * kg);
#pragma unroll
    for (int j = 0; j < RN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (F8) eo[i][4 * j + r] = (bf16_t)fmaf(ev[i][j][r], dq[j][r], bv[j][r]);
        else eo[i][4 * j + r] = (bf16_t)(ev[i][j][r] + bv[j][r]);
      }
    *reinterpret_cast<bf16x8*>(dst) = eo[i];
  };
  // InstanceNorm-backward partials (INP): per lane the sums over its voxels of g and g (x - mean) for channels
  // n0 + 8 kg + (0..7), g = dy if x > mean else 0 (times rstd at the flush); the first brick's epilogue runs on
  // zeroed accumulators and x and adds 0
  __shared__ float ired[INP ? 4 : 1][2][32];
  float isg[8], isgx[8], imu[8];
  int in_n = -1;
  V8<T> xin[BY];
  if constexpr (INP) {
#pragma unroll
    for (int k = 0; k < 8; ++k) isg[k] = isgx[k] = imu[k] = 0.f;
#pragma unroll
    for (int i = 0; i < BY; ++i) xin[i].zero();
  }
  auto in_flush = [&]() {
   if constexpr (INP) {   // (the 1-wave LDS array of the plain instantiations is never read)   // block-wide, fixed order: 16-lane tree, then waves 0..3
#pragma unroll
    for (int o = 1; o < 16; o <<= 1)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        isg[k] += __shfl_xor(isg[k], o, 64);
        isgx[k] += __shfl_xor(isgx[k], o, 64);
      }
    if (r16 == 0)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        ired[wave][0][8 * kg + k] = isg[k];
        ired[wave][1][8 * kg + k] = isgx[k];
      }
    __syncthreads();
    if (tid < 32) {
      const float a = ired[0][0][tid] + ired[1][0][tid] + ired[2][0][tid] + ired[3][0][tid];
      const float c = ired[0][1][tid] + ired[1][1][tid] + ired[2][1][tid] + ired[3][1][tid];
      float* p = g.inpart + (((long long)in_n * blocks_per_nt + blk) * g.Ncols + n0 + tid) * 2;
      p[0] = a;
      p[1] = c * g.inrstd[in_n * g.Ncols + n0 + tid];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) isg[k] = isgx[k] = 0.f;
   }
  };
  auto in_begin = [&](const Unit& q) {   // block-uniform: the sample of the epilogue's brick
    if constexpr (INP) {
      if (q.n != in_n) {
        if (in_n >= 0) in_flush();
        in_n = q.n;
#pragma unroll
        for (int k = 0; k < 8; ++k) imu[k] = g.inmean[in_n * g.Ncols + n0 + 8 * kg + k];
      }
    }
  };
  auto in_load_row = [&](const Unit& q, int i) {   // x of the lane's output voxel of row i
    const T* X = reinterpret_cast<const T*>(g.inx) + (long long)q.n * vox_per_n * g.ldinx + n0 + 8 * kg;
    xin[i].load(X + (long long)((q.z0 + wave) * g.H + q.y0 + i) * g.W * g.ldinx + (long long)(q.x0 + r16) * g.ldinx);
  };
  auto epi_inp = [&](int i, int half) {
#pragma unroll
    for (int k = 4 * half; k < 4 * half + 4; ++k) {
      const float d = xin[i].get(k) - imu[k];
      const float gg = d > 0.f ? (float)eo[i][k] : 0.f;
      isg[k] += gg;
      isgx[k] = fmaf(gg, d, isgx[k]);
    }
  };

  Unit cur = unit_of(u_begin), prev = cur;
  set_x(cur);
#pragma unroll
  for (int k = 0; k < XK; ++k) load_row(k);
#pragma unroll
  for (int k = 0; k < XK; ++k) stage_row(0, k);
  __syncthreads();
  int b = 0;
  for (int u = u_begin; u < u_end; ++u) {
    f32x4 acc[BY][RN];   // (first written by the C = 0 MFMAs of group 0)
    Unit nxt = cur;
    if (u + 1 < u_end) {   // (the last brick re-stages itself into the idle buffer)
      nxt.x0 += BX;
      if (nxt.x0 == g.W) {
        nxt.x0 = 0;
        nxt.y0 += BY;
        if (nxt.y0 == g.H) {
          nxt.y0 = 0;
          nxt.z0 += BZ;
          if (nxt.z0 == g.D) {
            nxt.z0 = 0;
            ++nxt.n;
          }
        }
      }
    }
    set_x(nxt);
    in_begin(prev);
    const T* Xb = Xl + b * XQ * EPQ;
    V8<T> af[F8 ? 1 : 2][HY];
    long af8[F8 ? 2 : 1][HY];
#pragma unroll
    for (int h = 0; h < HY; ++h) {
      if constexpr (F8) af8[0][h] = *reinterpret_cast<const long*>(Xb + (ao[0] + h * RY) * EPQ);
      else af[0][h].load(Xb + (ao[0] + h * RY) * EPQ);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      const int kz = q / 3, kx = q - kz * 3;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        if (q + 1 < 9 && c < HY) {     // fragment c of the next group
          const int qn = q + 1, kzn = qn / 3, kxn = qn - kzn * 3;
          if constexpr (F8) af8[qn & 1][c] = *reinterpret_cast<const long*>(Xb + (ao[kxn] + kzn * RZ + c * RY) * EPQ);
          else af[qn & 1][c].load(Xb + (ao[kxn] + kzn * RZ + c * RY) * EPQ);
        }
        if (q == 0) {
          load_row(c);                  // next brick's halo rows 0..7
          if ((c & 1) == 0) epi_row(prev, c >> 1);
        }
        if (q == 1 && c < XK - 8) load_row(8 + c);
        if constexpr (INP) {
          if (q == 1) epi_inp(c >> 1, c & 1);
          if (q == 4 && c < BY) in_load_row(cur, c);
        }
        if (q >= SG0) {
#pragma unroll
          for (int pp = 0; pp < PPC; ++pp) {
            const int pi = c * PPC + pp;            // pair index inside the group: row slot pi / 4, pair pi % 4
            const int k = (q - SG0) * RPG + pi / 4;
            if (k < XK) {
              if constexpr (NORM) norm_pair(k, pi % 4, sv[pi / 4]);
              else if constexpr (F8) { if (pi % 4 == 0) to_f8(k, sv[pi / 4]); }
              else if (pi % 4 == 0) sv[pi / 4] = __builtin_bit_cast(u32x4, xr[k].v);
              if (pi % 4 == 3) store_row(b ^ 1, k, sv[pi / 4]);
            }
          }
        }
#pragma unroll
        for (int m = 3 * c; m < 3 * c + 3; ++m) {
          const int ky = m >> 3, i = (m >> 1) & 3, j = m & 1;
          if constexpr (F8) {
            if (q == 0 && ky == 0) mfma_aw80(acc[i][j], wf8[kx][j], af8[0][i]);
            else mfma_aw8(acc[i][j], wf8[kz * 9 + ky * 3 + kx][j], af8[q & 1][i + ky]);
          } else {
            if (q == 0 && ky == 0) mfma_aw0(acc[i][j], wf[kx][j].v, af[0][i].v);
            else mfma_aw(acc[i][j], wf[kz * 9 + ky * 3 + kx][j].v, af[q & 1][i + ky].v);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // one MFMA-result hazard fence over all 8 accumulators before they are copied
    asm volatile("s_nop 7\n\ts_nop 7" : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[1][0]), "+a"(acc[1][1]),
                 "+a"(acc[2][0]), "+a"(acc[2][1]), "+a"(acc[3][0]), "+a"(acc[3][1]));
#pragma unroll
    for (int i = 0; i < BY; ++i)
#pragma unroll
      for (int j = 0; j < RN; ++j) ev[i][j] = acc[i][j];
    prev = cur;
    __syncthreads();   // buffer b^1 is complete; buffer b is free for the brick after next
    b ^= 1;
    cur = nxt;
  }
  in_begin(prev);
#pragma unroll
  for (int i = 0; i < BY; ++i) {
    epi_row(prev, i);
    if constexpr (INP) {
      epi_inp(i, 0);
      epi_inp(i, 1);
    }
  }
  if constexpr (INP) {
    in_flush();
    inp_zero(u_begin / (nbrick / (g.M / vox_per_n)), in_n);
  }
  PROBE_BLOCK(true);
}

}  // namespace

// The W % 16 one-chunk 32-column conv: brick6 (forward, deferred-norm forward, e4m3 forward, and the data gradient
// with the InstanceNorm-backward partials), on the grid choose_gemm gave it.
MMSEG_LOCAL void launch_brick6(const GemmArgs& g, const GemmChoice& c, hipStream_t s) {
  const dim3 grid(c.grid), block(c.block);
  if (g.wdq) {   // e4m3 forward (mmseg_conv3_fwd_fp8)
    if (g.nmean) MMSEG_LAUNCH((conv3_brick6_kernel<true, 6, false, true>), grid, block, 0, s, g, c.upb, c.bpn);
    else MMSEG_LAUNCH((conv3_brick6_kernel<false, 6, false, true>), grid, block, 0, s, g, c.upb, c.bpn);
  } else if (g.inpart) {   // mmseg_conv3_dgrad_in (no bias); the kernel zeroes the partials of samples a block does not touch
    MMSEG_LAUNCH((conv3_brick6_kernel<false, 6, true>), grid, block, 0, s, g, c.upb, c.bpn);
  } else if (g.nmean) {
    MMSEG_LAUNCH((conv3_brick6_kernel<true, 6>), grid, block, 0, s, g, c.upb, c.bpn);
  } else {
    MMSEG_LAUNCH((conv3_brick6_kernel<false, 6>), grid, block, 0, s, g, c.upb, c.bpn);
  }
}

MMSEG_PROBE_SETTER(probe_set_brick6)
