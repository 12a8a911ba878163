// Shared by the conv sources (conv_gemm.hip and the sources split off it: conv_brick2.hip, conv_brick6.hip,
// conv_brick8.hip, conv_brickr.hip, conv_wgrad.hip, wgrad_reduce.hip): the argument structs and the kernel choice that
// go from the choosers and entry points to the kernel families, the constants and device helpers more than one source
// uses, and the host functions that cross sources.
//
// The types sit in an anonymous namespace: a kernel's symbol carries the name of its argument struct
// ((anonymous namespace)::GemmArgs ...), and tools/rocprof_families.py, the recorded profiles and the name pins of
// tests/test_conv_plan_cpu.py depend on those symbols.  Every source therefore sees its own, identical copy of these
// types (the Makefile rebuilds every source that includes this header when it changes), and the host functions that
// cross sources are extern "C", whose linkage does not depend on their parameter types (MMSEG_LOCAL: hidden, not part
// of the library's ABI).  Keep them few: one launcher per kernel family.
#pragma once
#include "mmseg_common.h"
#include "instnorm_ops.h"   // norm_relu8: the deferred norm of staged channels

#include <stdlib.h>

#define MMSEG_LOCAL extern "C" __attribute__((visibility("hidden")))

namespace {

// Tuning knobs for in-process A/B runs (tools/kbench.py); defaults are the shipped choice.
int knob(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}

enum GatherMode { MODE_CONV3 = 0, MODE_POINT = 1, MODE_CONVT_FWD = 2, MODE_CONVT_DGRAD = 3 };

// the 4 x 4 x 8 brick and its halo (conv3_brick_kernel, the brick weight gradients), 32 input channels per chunk
constexpr int BRK_Z = 4, BRK_Y = 4, BRK_X = 8;
constexpr int HLO_Z = BRK_Z + 2, HLO_Y = BRK_Y + 2, HLO_X = BRK_X + 2;
constexpr int HLO_V = HLO_Z * HLO_Y * HLO_X;   // 360 halo voxels
constexpr int CK = 32;                          // input channels per chunk

// the (4 ZW) x 8 x 8 brick's y / x sides and the LDS halo image of conv3_brick2_kernel and its successors, which
// the runtime-brick kernel shares
constexpr int B2_Y = 8, B2_X = 8;
constexpr int H2_Y = B2_Y + 2, H2_X = B2_X + 2;

template <typename T>
struct Brick2Layout {
  static constexpr int QV = 2 * (int)sizeof(T);      // 16-B quads per voxel (32 channels): 4 bf16, 8 f32
  static constexpr int QG = QV / 4;                    // quads per 8-channel group
  static constexpr int RY = H2_X * QV + 2;             // quads per halo y-row (padded)
  static constexpr int RZ = H2_Y * RY;                 // quads per halo z-plane
};

// conv3_brickr_kernel's limits, which choose_gemm plans a brick within
constexpr int BR_MAXHV = 640;   // halo voxels staged per block (host guarantees)
// halo image quads available (host guarantees (bz+2)(by+2)((bx+2)*QV+2) <= this): 40 KB bf16 / 80 KB f32
__host__ __device__ constexpr int br_xq(int tsize) { return tsize == 2 ? 2560 : 5120; }

// Block timeline probe (diagnostics, built only with -DMMSEG_TIMING_PROBES; tools/convbench.py --probe).
// Per block b < PROBE_NB: [realtime start, realtime end, memtime start, memtime end, HW_ID, XCC_ID, -, -];
// then for blocks < 32, every wave's lane 0 records up to 64 memtime stamps (PROBE_T) at phase boundaries.
#ifdef MMSEG_TIMING_PROBES
constexpr int PROBE_NB = 16384;
__device__ long long* g_probe = nullptr;
__device__ __forceinline__ void probe_block(bool end) {
  long long* p = g_probe;
  if (p && threadIdx.x == 0 && blockIdx.x < PROBE_NB) {
    p += 8LL * blockIdx.x;
    p[end ? 1 : 0] = (long long)__builtin_amdgcn_s_memrealtime();
    p[end ? 3 : 2] = (long long)__builtin_amdgcn_s_memtime();
    if (!end) {
      p[4] = (long long)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID
      p[5] = (long long)(unsigned)__builtin_amdgcn_s_getreg((15 << 11) | 20);   // HW_REG_XCC_ID
    }
  }
}
__device__ __forceinline__ void probe_stamp(int& k) {
  long long* p = g_probe;
  if (p && (threadIdx.x & 63) == 0 && blockIdx.x < 32 && k < 64)
    p[8LL * PROBE_NB + ((blockIdx.x * 16 + (threadIdx.x >> 6)) * 64) + k] = (long long)__builtin_amdgcn_s_memtime();
  ++k;
}
#define PROBE_BLOCK(e) probe_block(e)
#define PROBE_T() probe_stamp(probe_k)
#define PROBE_DECL() int probe_k = 0
// There is no relocatable device code, so every source with probe points has its own g_probe and defines its setter
// with this; mmseg_probe_set (conv_gemm.hip) calls them all.
#define MMSEG_PROBE_SETTER(NAME)                                                            \
  MMSEG_LOCAL int NAME(long long* buf) {                                                    \
    return hipMemcpyToSymbol(HIP_SYMBOL(g_probe), &buf, sizeof(buf)) == hipSuccess ? 0 : 1; \
  }
#else
#define PROBE_BLOCK(e)
#define PROBE_T()
#define PROBE_DECL()
#define MMSEG_PROBE_SETTER(NAME)
#endif

struct GemmArgs {
  const void* a;  int lda;   // A source (NDHWC)
  const void* b;             // packed weights [KGp][Cpad][8]
  const float* bias;         // per output channel, or null
  void* out;      int ldo;   // output (NDHWC) for ksplit == 1
  float* part;               // [ksplit][M][Ncols] fp32 partials for ksplit > 1
  int M, Ncols, Cpad, KG, cpg_shift;
  int D, H, W;               // row grid
  int ksplit, kg_per_split;  // k-groups per split (multiple of 4)
  int swz;                   // XCD-aware block remap
  int kchunks;               // CONV3 brick kernels: 32-channel input chunks holding real channels (0 = all);
                             // the packed weights of the rest are zero (channel-padded K side), so they are skipped
  // deferred InstanceNorm + ReLU of the A source (brick6 only, mmseg_conv3_fwd_norm): A holds the PRE-norm
  // activation, the kernel stages relu((a - nmean[n][c]) * nrstd[n][c]) rounded to T (in_relu_apply's values)
  const float* nmean;
  const float* nrstd;
  // split output (mmseg_conv_gemm_split): columns >= split go to out2 (column - split, row pitch ldo2).  The
  // decoder's first-conv data gradient writes d(upsampled) and d(skip) as two dense tensors instead of one
  // [voxel][2F] tensor whose halves every later reader fetched at half a cache line per voxel.
  void* out2;
  int ldo2, split;
  // InstanceNorm-backward partials of the output (brick6 data gradient only, mmseg_conv3_dgrad_in): the output is
  // the gradient dy of an InstanceNorm + ReLU whose PRE-norm input is inx (pitch ldinx, statistics inmean /
  // inrstd [N][Ncols]); the kernel also writes inpart[n][block][col][2] = (sum g, sum g xhat), g = dy [xhat > 0]
  const void* inx;
  int ldinx;
  const float* inmean;
  const float* inrstd;
  float* inpart;
  // fp8 forward (brick6 F8, mmseg_conv3_fwd_fp8): b holds e4m3 weights w * s[co] (s = 448 / max |w[co]|), wdq[co] =
  // 1 / s[co] restores the scale in the epilogue; the staged activations are e4m3 at unit scale
  const float* wdq;
  // grouped launch (mmseg_conv_gemm_group, runtime-brick kernel only): the samples are grp_n-sample groups with
  // their own weights / bias -- group gi reads b + gi * w_gstride (elements) and bias + gi * b_gstride; the M
  // modality encoders' small levels run as ONE launch over M x N samples
  int grp_n;
  long long w_gstride;
  int b_gstride;
  // residual epilogue (MODE_POINT, ksplit 1, vector stores; mmseg_conv_gemm_res): out = round(round(acc + bias) +
  // res), the values of the GEMM followed by mmseg_add(res, out) -- a residual sum without its own pass (res may
  // alias out)
  const void* res;
  int ldres;
  // whole-row output hint (brick2 kernels; others ignore it): the last column tile also writes zeros into columns
  // [Ncols, zcols) (<= Ncols + BN) of the output rows -- SwinUNETR's 48 / 96-column outputs at pitch 64 / 128 are
  // then written in whole 128-B lines (partial-line writes ran at ~60 % of the whole-row rate, r05k)
  int zcols;
  // token-GEMM epilogue (MODE_POINT, ksplit 1, vector stores; mmseg_conv_gemm_gelu): epi 1 = GELU forward, out = h
  // (the pre-activation the backward reads) and aux_out = gelu(h); epi 2 = GELU backward, out = round(round(acc) *
  // gelu'(aux)) with aux = h -- the values of the GEMM followed by mmseg_gelu_fwd / mmseg_gelu_bwd (pitch ldo)
  int epi;
  const void* aux;
  void* aux_out;
};

// Output element (row voxel, column) of a GEMM (split-aware; split is a multiple of 8).
template <typename T>
__device__ __forceinline__ T* out_at(const GemmArgs& g, long long vox, int col) {
  if (g.out2 && col >= g.split) return reinterpret_cast<T*>(g.out2) + vox * g.ldo2 + (col - g.split);
  return reinterpret_cast<T*>(g.out) + vox * g.ldo + col;
}

// 32-channel K chunks a CONV3 brick kernel iterates: all of the (power-of-two) A source's, or only the
// leading ones that hold real channels.
__host__ __device__ __forceinline__ int gemm_nchunk(const GemmArgs& g) {
  const int n = (8 << g.cpg_shift) / 32;
  return (g.kchunks > 0 && g.kchunks < n) ? g.kchunks : n;
}

template <typename T>
__device__ __forceinline__ void mfma_step(f32x4& acc, const V8<T>& a, const V8<T>& b);

template <>
__device__ __forceinline__ void mfma_step<bf16_t>(f32x4& acc, const V8<bf16_t>& a, const V8<bf16_t>& b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mfma_step<float>(f32x4& acc, const V8<float>& a, const V8<float>& b) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b.v[j], acc, 0, 0, 0);
}

// weight image of the (4 ZW) x 8 x 8 brick kernels: quad slot swizzle by bit 3 of the column (conv3_brick2_kernel)
__device__ __forceinline__ int w2_swz(int col) { return ((col >> 3) & 1) << 1; }

// 8 channels of one voxel through a 32-bit offset buffer load (out-of-range offsets read zeros)
template <typename T>
__device__ __forceinline__ void buf_load_v8(V8<T>& v, __amdgpu_buffer_rsrc_t r, uint32_t off);
template <>
__device__ __forceinline__ void buf_load_v8<bf16_t>(V8<bf16_t>& v, __amdgpu_buffer_rsrc_t r, uint32_t off) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  const i32x4 t = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  v.v = __builtin_bit_cast(bf16x8, t);
}
// The whole vector is bit-cast at once.  Casting element by element (__builtin_bit_cast(float, a[j])) is
// miscompiled by hipcc (ROCm 7.2, gfx950): the b128 loads were narrowed to buffer_load_dword and element 0 was
// copied into all four registers (v173..v175 = v172 in the disassembly), which is why the fp32 instantiation
// of the 32-bit staging gave wrong results in r02 (tests/test_kernels_gpu.py::test_b32_halo_staging).
template <>
__device__ __forceinline__ void buf_load_v8<float>(V8<float>& v, __amdgpu_buffer_rsrc_t r, uint32_t off) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  typedef float f32x4v __attribute__((ext_vector_type(4)));
  const f32x4v a = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
  const f32x4v b = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(r, off + 16, 0, 0));
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v.v[j] = a[j];
    v.v[4 + j] = b[j];
  }
}

// MFMA with the weight fragment pinned to the accumulator file: hipcc otherwise keeps the 216 weight
// registers in VGPRs and, short of VGPRs, issues each tap's LDS reads just before their MFMAs.  The asm is one
// opaque instruction to hipcc: it inserts the lgkmcnt waits for x, but no MFMA hazard padding, which
// brick4_fence / brick4_wfence supply where the accumulators are read and after the weights are written.
__device__ __forceinline__ void mfma_aw(f32x4& acc, const bf16x8& w, const bf16x8& x) {
  asm("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "a"(w), "v"(x));
}
// e4m3 x e4m3 -> f32 (K = 32: a lane holds 8 fp8 = 8 bytes of A and of B, the bf16 form's lane map)
__device__ __forceinline__ void mfma_aw8(f32x4& acc, const long& w, const long& x) {
  asm("v_mfma_f32_16x16x32_fp8_fp8 %0, %1, %2, %0" : "+a"(acc) : "a"(w), "v"(x));
}
__device__ __forceinline__ void mfma_aw80(f32x4& acc, const long& w, const long& x) {
  asm("v_mfma_f32_16x16x32_fp8_fp8 %0, %1, %2, 0" : "=a"(acc) : "a"(w), "v"(x));
}
// first MFMA of an accumulation chain: C = 0 (no accumulator zeroing per brick)
__device__ __forceinline__ void mfma_aw0(f32x4& acc, const bf16x8& w, const bf16x8& x) {
  asm("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=a"(acc) : "a"(w), "v"(x));
}
__device__ __forceinline__ void brick4_fence(f32x4& a, f32x4& b) {
  asm volatile("s_nop 7\n\ts_nop 7" : "+a"(a), "+a"(b));
}
__device__ __forceinline__ void brick4_wfence(bf16x8& a, bf16x8& b) {
  asm volatile("s_nop 2" : "+a"(a), "+a"(b));
}

// ---- the kernel choice of a forward / data-gradient GEMM launch (choose_gemm, conv_gemm.hip)
enum GemmKernel {
  GK_BRICKR,   // conv3_brickr_kernel: runtime brick (small volumes, grouped launches), splits over 32-channel chunks
  GK_BRICK8,   // conv3_brick8_kernel: 8-wave 8x8x8 brick, LDS-DMA staging
  GK_BRICK2_BN48, GK_BRICK2,   // conv3_brick2_kernel: 4x8x8 brick, 48-column tiles; 64 / 32-column tiles
  GK_BRICK6,   // conv3_brick6_kernel: W % 16, one input chunk, 32 columns (deferred norm, e4m3, IN-backward partials)
  GK_BRICK4,   // conv3_brick4_kernel: one input chunk, 32 columns, persistent
  GK_BRICK3,   // conv3_brick3_kernel: 32-column tiles, persistent
  GK_BRICK1,   // conv3_brick_kernel: the first brick generation (MMSEG_BRICK=1)
  GK_GEMM_64x256, GK_GEMM_64x192, GK_GEMM_64x128, GK_GEMM_128x48, GK_GEMM_128x96, GK_GEMM_128x32, GK_GEMM_128x64
};
struct GemmChoice {
  int kernel;          // GemmKernel
  const char* name;    // the family noted for mmseg_last_kernel() / the per-kernel timer
  int bn;              // column tile
  int grid, block;
  int upb, bpn;        // persistent kernels (brick6 / brick4 / brick3): units per block, blocks per column tile
  int bz, by, bx;      // GK_BRICKR: the brick
  bool b32, kw2;       // 32-bit offset halo staging; GK_BRICKR: two waves per SIMD over an in-block chunk split
  int ksplit;          // the launch's split count (GK_BRICKR: clamped to whole chunk ranges)
  bool reduce;         // a split-K reduce follows
  int ks_want;         // CONV3: the split count this shape wants (mmseg_conv3_splits)
  int tsize;           // element bytes (2: bf16, 4: fp32): the element type of the instantiation a launcher takes
};
// The planning queries' flags: what the launch would carry (mmseg_conv3_kernel / mmseg_conv3_wgrad_kernel).
enum ChoiceFlags { CF_NORM = 1, CF_INPART = 2, CF_FP8 = 4, CF_GROUPS = 8, CF_PAD16 = 16 };

// part[ks][row][col] -> torch-layout gradient (fixed-order sum over ks).
//   CONV3 : grad[co][ci][tap]    row=co, col = tap*Cin_pad + ci, ci < Cin_real
//   POINT : grad[co][ci]         row=co, col = ci
//   CONVT : grad[ci][co][tap]    row=ci, col = tap*Cout + co
struct WReduceArgs {
  const float* part;
  float* grad;
  const float* bias_part;
  float* bias_grad;
  int Ca, Ncols, ksplit;
  int cpad, creal;    // per-tap channel count in cols (padded) and real count
  int ntap;           // 27 (CONV3), 1 (POINT), 8 (CONVT)
  int accumulate;
  int chmajor;        // cols are channel-major (col = c*ntap + tap, brick2/brickr partials) instead of tap-major
  int frag_mt;        // > 0: wgrad_dma's fragment-native partials (MT 16-row tiles per block), see wgrad_dma_kernel
  int nchunk;         // frag_mt > 0: 32-channel chunks per tile row
  // grouped (blockIdx.y = group gi < gridDim.y): splits [gi * ksplit, (gi + 1) * ksplit) of the partials (ksplit
  // counts one group's splits), written to grad + gi * grad_gstride / bias_grad + gi * bias_gstride
  long long grad_gstride;
  int bias_gstride;
  int vec4;           // host-set (wred_vec4): channel-major sums as 16-B stores
};

}  // namespace

// ---- per-family launchers: each maps a GemmChoice to the template instantiation next to its kernels and launches it
// on the grid the choice carries; launch_gemm (conv_gemm.hip) chooses, checks, calls one and checks the launch
MMSEG_LOCAL void launch_brickr(const GemmArgs& g, const GemmChoice& c, hipStream_t s);   // GK_BRICKR
MMSEG_LOCAL void launch_brick2(const GemmArgs& g, const GemmChoice& c, hipStream_t s);   // GK_BRICK2_BN48 / 2 / 3 / 4 / 1
MMSEG_LOCAL void launch_brick6(const GemmArgs& g, const GemmChoice& c, hipStream_t s);
MMSEG_LOCAL void launch_brick8(const GemmArgs& g, const GemmChoice& c, hipStream_t s);
#ifdef MMSEG_TIMING_PROBES
MMSEG_LOCAL int probe_set_brick2(long long* buf);
MMSEG_LOCAL int probe_set_brick6(long long* buf);
MMSEG_LOCAL int probe_set_brick8(long long* buf);
#endif
// the split reduce of a weight gradient now, or queued until mmseg_wgrad_reduce_flush (wgrad_reduce.hip)
MMSEG_LOCAL int launch_wgrad_reduce(WReduceArgs g, void* stream, int groups = 1);
MMSEG_LOCAL int wred_push(const WReduceArgs& r, int groups, void* stream);
