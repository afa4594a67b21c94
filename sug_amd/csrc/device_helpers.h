// Small device helpers shared by several .hip units (device code only; include after common.h).
#pragma once
#include <hip/hip_runtime.h>

// 16-byte load / store of four consecutive floats (p 16-byte aligned)
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// inclusive prefix sums over the lanes through the DPP paths (no LDS-crossbar shuffles): lanes without a source add 0
// (the reverse-list builds of knn.hip and reverse_tiled.hip)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned rev_dpp0(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ unsigned rev_row_scan(unsigned x) {          // over each row of 16 lanes
  x += rev_dpp0<0x111, 0xf>(x);                                         // row_shr:1
  x += rev_dpp0<0x112, 0xf>(x);                                         // row_shr:2
  x += rev_dpp0<0x114, 0xf>(x);                                         // row_shr:4
  x += rev_dpp0<0x118, 0xf>(x);                                         // row_shr:8
  return x;
}
__device__ __forceinline__ unsigned rev_wave_scan(unsigned x) {         // over the 64 lanes
  x = rev_row_scan(x);
  x += rev_dpp0<0x142, 0xa>(x);                                         // row_bcast:15 into rows 1, 3
  x += rev_dpp0<0x143, 0xc>(x);                                         // row_bcast:31 into rows 2, 3
  return x;
}
