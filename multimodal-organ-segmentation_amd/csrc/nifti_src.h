// One NIfTI-1 source element as a double, shared by the decode kernels (nifti.hip) and the SUV statistics
// (analysis.hip): both read the file's raw voxel block and must see the same bits get_fdata() gives.
#pragma once
#include "mmseg_common.h"

namespace nifti_src {

// ---- one source element as a double
template <int DT> struct Src;
template <> struct Src<2> {       // uint8
  static __device__ __forceinline__ double get(const void* p, size_t i, int) { return (double)((const uint8_t*)p)[i]; }
};
template <> struct Src<256> {     // int8
  static __device__ __forceinline__ double get(const void* p, size_t i, int) { return (double)((const int8_t*)p)[i]; }
};
__device__ __forceinline__ uint16_t ld16(const void* p, size_t i, int swap) {
  const uint16_t u = ((const uint16_t*)p)[i];
  return swap ? __builtin_bswap16(u) : u;
}
__device__ __forceinline__ uint32_t ld32(const void* p, size_t i, int swap) {
  const uint32_t u = ((const uint32_t*)p)[i];
  return swap ? __builtin_bswap32(u) : u;
}
template <> struct Src<4> {       // int16
  static __device__ __forceinline__ double get(const void* p, size_t i, int s) { return (double)(int16_t)ld16(p, i, s); }
};
template <> struct Src<512> {     // uint16
  static __device__ __forceinline__ double get(const void* p, size_t i, int s) { return (double)ld16(p, i, s); }
};
template <> struct Src<8> {       // int32
  static __device__ __forceinline__ double get(const void* p, size_t i, int s) { return (double)(int32_t)ld32(p, i, s); }
};
template <> struct Src<768> {     // uint32
  static __device__ __forceinline__ double get(const void* p, size_t i, int s) { return (double)ld32(p, i, s); }
};
template <> struct Src<16> {      // float32
  static __device__ __forceinline__ double get(const void* p, size_t i, int s) {
    return (double)__uint_as_float(ld32(p, i, s));
  }
};
template <> struct Src<64> {      // float64
  static __device__ __forceinline__ double get(const void* p, size_t i, int s) {
    const unsigned long long u = ((const unsigned long long*)p)[i];
    return __longlong_as_double((long long)(s ? __builtin_bswap64(u) : u));
  }
};

// raw * slope, then + inter, each rounded on its own (get_fdata's two numpy operations).  The contraction is
// switched off here: hipcc contracts by default and __dmul_rn / __dadd_rn are plain * and + to it, so without
// the pragma the pair becomes one v_fma_f64 and sums that sit on a float32 rounding boundary come out different.
__device__ __forceinline__ double scl(double v, double slope, double inter) {
#pragma clang fp contract(off)
  const double p = v * slope;
  return p + inter;
}

inline bool known_datatype(int dt) {
  return dt == 2 || dt == 4 || dt == 8 || dt == 16 || dt == 64 || dt == 256 || dt == 512 || dt == 768;
}
// bytes of one element of a known datatype
inline int datatype_bytes(int dt) {
  return dt == 2 || dt == 256 ? 1 : dt == 4 || dt == 512 ? 2 : dt == 64 ? 8 : 4;
}

}  // namespace nifti_src
