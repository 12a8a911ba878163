// NIfTI voxel blocks on the device (data/nifti.py, Trainer.predict): the file's raw
// voxel bytes are uploaded as they are and decoded here, and a prediction is
// encoded back into file order, so neither the float64 rescale nor the axis
// permutation of the reference's load_nifti / np.stack(...).copy() runs on the host.
//
//   nifti_decode        raw [Z][Y][X] (x fastest, any of the eight NIfTI-1 types,
//                       either byte order) -> fp32 [X][Y][Z] (z fastest): unswap,
//                       to double, optional slope / inter in two roundings, to float
//                       (bitwise numpy's (raw.astype(f8) * slope + inter).astype(f4))
//   nifti_decode_label  same read side, the double truncated toward zero -> int64 / uint8
//   argmax_encode       logits [C][X][Y][Z] -> uint8 [Z][Y][X]: first maximum over C
//                       (torch.argmax), written in file order
//
// All three transpose the fastest axis.  One block moves a 64 x 64 (x, z) tile of one y
// through LDS (rows padded by one element): the global loads run along the source's
// fastest axis and the stores along the destination's, both as whole rows of a wave.
#include "mmseg_common.h"
#include "nifti_src.h"

namespace {

using namespace nifti_src;     // Src<>, ld16 / ld32, scl, known_datatype

constexpr int NT = 64;            // tile edge = wave width
constexpr int NW = 4;             // waves per block: wave w moves tile rows w, w + 4, ...

// ---- the decoded double as the output type; the LDS tile holds at least a dword per element
template <typename O> struct Dst;
template <> struct Dst<float> {
  typedef float tile_t;
  static __device__ __forceinline__ tile_t put(double v) { return (float)v; }
};
template <> struct Dst<long long> {
  typedef long long tile_t;
  static __device__ __forceinline__ tile_t put(double v) { return (long long)v; }
};
template <> struct Dst<uint8_t> {
  typedef uint32_t tile_t;
  static __device__ __forceinline__ tile_t put(double v) { return (uint32_t)(uint8_t)(long long)v; }
};

// block b -> (tile along the source's fastest axis, tile along the other, y); the fastest-axis tile varies fastest
__device__ __forceinline__ void tile_of_block(int nfast, int nslow, int& tfast, int& tslow, int& y) {
  unsigned b = blockIdx.x;
  tfast = (int)(b % (unsigned)nfast);
  b /= (unsigned)nfast;
  tslow = (int)(b % (unsigned)nslow);
  y = (int)(b / (unsigned)nslow);
}

template <int DT, typename O>
__global__ __launch_bounds__(NT * NW) void nifti_decode_kernel(const void* __restrict__ raw, int swap, int X, int Y,
                                                                int Z, int nbx, int nbz, int scale, double slope,
                                                                double inter, O* __restrict__ out) {
  typedef typename Dst<O>::tile_t tile_t;
  __shared__ tile_t tile[NT][NT + 1];
  const int lane = threadIdx.x & (NT - 1), wave = threadIdx.x >> 6;
  int bx, bz, y;
  tile_of_block(nbx, nbz, bx, bz, y);
  const int x0 = bx * NT, z0 = bz * NT;
  {
    const int x = x0 + lane;
#pragma unroll 4
    for (int r = wave; r < NT; r += NW) {
      const int z = z0 + r;
      if (x < X && z < Z) {
        double v = Src<DT>::get(raw, ((size_t)z * Y + y) * X + x, swap);
        if (scale) v = scl(v, slope, inter);
        tile[r][lane] = Dst<O>::put(v);
      }
    }
  }
  __syncthreads();
  const int z = z0 + lane;
#pragma unroll 4
  for (int r = wave; r < NT; r += NW) {
    const int x = x0 + r;
    if (x < X && z < Z) out[((size_t)x * Y + y) * Z + z] = (O)tile[lane][r];
  }
}

__global__ __launch_bounds__(NT * NW) void argmax_encode_kernel(const float* __restrict__ logits, int C, int X, int Y,
                                                                 int Z, int nbz, int nbx, uint8_t* __restrict__ out) {
  __shared__ uint32_t tile[NT][NT + 1];
  const int lane = threadIdx.x & (NT - 1), wave = threadIdx.x >> 6;
  int bz, bx, y;
  tile_of_block(nbz, nbx, bz, bx, y);
  const int x0 = bx * NT, z0 = bz * NT;
  const size_t cs = (size_t)X * Y * Z;
  {
    const int z = z0 + lane;
    for (int r = wave; r < NT; r += NW) {
      const int x = x0 + r;
      if (x < X && z < Z) {
        const float* p = logits + ((size_t)x * Y + y) * Z + z;
        float best = p[0];
        uint32_t bi = 0;
        for (int c = 1; c < C; ++c) {
          const float t = p[(size_t)c * cs];
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
  for (int r = wave; r < NT; r += NW) {
    const int z = z0 + r;
    if (x < X && z < Z) out[((size_t)z * Y + y) * X + x] = (uint8_t)tile[lane][r];
  }
}

// blocks of a launch over the 64 x 64 tiles of every y; 0 when they do not fit a 1-D grid
long long tile_blocks(int X, int Y, int Z) {
  const long long n = (long long)ceil_div(X, NT) * ceil_div(Z, NT) * Y;
  return n <= 0x7fffffffLL ? n : 0;
}

template <typename O>
int launch_decode(const void* raw, int datatype, int swap, int X, int Y, int Z, int scale, double slope, double inter,
                  O* out, hipStream_t s) {
  const int nbx = ceil_div(X, NT), nbz = ceil_div(Z, NT);
  const dim3 grid((unsigned)tile_blocks(X, Y, Z)), block(NT * NW);
#define MMSEG_NIFTI_CASE(DT)                                                                                    \
  case DT:                                                                                                      \
    MMSEG_LAUNCH((nifti_decode_kernel<DT, O>), grid, block, 0, s, raw, swap, X, Y, Z, nbx, nbz, scale, slope, \
                 inter, out);                                                                                   \
    break;
  switch (datatype) {
    MMSEG_NIFTI_CASE(2)
    MMSEG_NIFTI_CASE(4)
    MMSEG_NIFTI_CASE(8)
    MMSEG_NIFTI_CASE(16)
    MMSEG_NIFTI_CASE(64)
    MMSEG_NIFTI_CASE(256)
    MMSEG_NIFTI_CASE(512)
    MMSEG_NIFTI_CASE(768)
  }
#undef MMSEG_NIFTI_CASE
  return 0;
}

int check_decode_args(const char* what, const void* raw, int datatype, int swap, int X, int Y, int Z, const void* out) {
  MMSEG_REQUIRE(raw != nullptr && out != nullptr && raw != out, "%s: raw and out, out of place", what);
  MMSEG_REQUIRE(known_datatype(datatype),
                "%s: NIfTI datatype %d (supported: 2 uint8, 4 int16, 8 int32, 16 float32, 64 float64, 256 int8, "
                "512 uint16, 768 uint32)", what, datatype);
  MMSEG_REQUIRE(swap == 0 || swap == 1, "%s: swap is 0 or 1 (got %d)", what, swap);
  MMSEG_REQUIRE(X >= 1 && Y >= 1 && Z >= 1, "%s: empty volume %d x %d x %d", what, X, Y, Z);
  MMSEG_REQUIRE(tile_blocks(X, Y, Z) > 0, "%s: volume %d x %d x %d has too many tiles for one launch", what, X, Y, Z);
  const int es = datatype_bytes(datatype);
  MMSEG_REQUIRE(((uintptr_t)raw & (uintptr_t)(es - 1)) == 0, "%s: raw must be aligned to its %d-byte elements", what, es);
  return 0;
}

}  // namespace

extern "C" {

int mmseg_nifti_decode(const void* raw, int datatype, int swap, int X, int Y, int Z, int scale, double slope,
                       double inter, float* out, void* stream) {
  if (check_decode_args("nifti_decode", raw, datatype, swap, X, Y, Z, out)) return 1;
  if (launch_decode<float>(raw, datatype, swap, X, Y, Z, scale != 0, slope, inter, out, (hipStream_t)stream)) return 1;
  return mmseg::check_launch("nifti_decode");
}

int mmseg_nifti_decode_label(const void* raw, int datatype, int swap, int X, int Y, int Z, int scale, double slope,
                             double inter, void* out, int label_bytes, void* stream) {
  if (check_decode_args("nifti_decode_label", raw, datatype, swap, X, Y, Z, out)) return 1;
  MMSEG_REQUIRE(label_bytes == 8 || label_bytes == 1, "nifti_decode_label: int64 or uint8 labels");
  hipStream_t s = (hipStream_t)stream;
  if (label_bytes == 8)
    launch_decode<long long>(raw, datatype, swap, X, Y, Z, scale != 0, slope, inter, (long long*)out, s);
  else
    launch_decode<uint8_t>(raw, datatype, swap, X, Y, Z, scale != 0, slope, inter, (uint8_t*)out, s);
  return mmseg::check_launch("nifti_decode_label");
}

int mmseg_argmax_encode(const float* logits, int C, int X, int Y, int Z, unsigned char* out, void* stream) {
  MMSEG_REQUIRE(logits != nullptr && out != nullptr, "argmax_encode: logits and out");
  MMSEG_REQUIRE(C >= 1 && C <= 255, "argmax_encode: 1 <= C <= 255 for a uint8 mask (got %d)", C);
  MMSEG_REQUIRE(X >= 1 && Y >= 1 && Z >= 1, "argmax_encode: empty volume %d x %d x %d", X, Y, Z);
  MMSEG_REQUIRE(tile_blocks(X, Y, Z) > 0, "argmax_encode: volume %d x %d x %d has too many tiles for one launch", X, Y, Z);
  MMSEG_LAUNCH(argmax_encode_kernel, dim3((unsigned)tile_blocks(X, Y, Z)), dim3(NT * NW), 0, (hipStream_t)stream, logits,
               C, X, Y, Z, ceil_div(Z, NT), ceil_div(X, NT), out);
  return mmseg::check_launch("argmax_encode");
}

}  // extern "C"
