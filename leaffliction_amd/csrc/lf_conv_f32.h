// libleafhip — what the fp32 convolution's two translation units share: lf_conv.hip (forward / dgrad) and
// lf_wgrad.hip (weight gradients, projection-shortcut backward).  Each pulls the names into its own unnamed
// namespace with `using namespace lf::conv_f32;`.
#pragma once
#include "lf_common.h"

namespace lf {
namespace conv_f32 {

constexpr int kThreads = 256;

constexpr int kMaxProC = 512;  // prologue scale/shift staged in LDS for this many channels at a time

inline bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

#if defined(__HIPCC__)
using lf::f32x16;
using lf::f32x4;

// Raw buffer loads: SGPR resource (base, byte size) + a 32-bit byte offset per lane; an offset
// at or beyond the size returns 0, which is how zero padding is fetched (no branches, no
// 64-bit address arithmetic per lane).
constexpr unsigned kBufOob = 0xffffffffu;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const float* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned off) {
    const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float buf_load1(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}
#endif

}  // namespace conv_f32
}  // namespace lf
