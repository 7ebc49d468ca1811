// mmidx_device_util.h -- the scalar / vector type names and the wave helpers that kernels of more than one unit use.
// Only typedefs and __device__ __forceinline__ functions: no __global__, so any kernel header may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef unsigned long long u64;
typedef unsigned int u32;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

// wave64 helpers that stay in the VALU (DPP / readlane): inside K3h's scan loop the LDS pipe is saturated
// by the table gather, and every ds_bpermute-based __shfl would queue behind it
__device__ __forceinline__ u32 wave_incl_scan_u32(u32 x) {
    u32 v = x;  // Hillis-Steele inside each row of 16 lanes, then the row totals (gfx9 row broadcasts)
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
    return v;
}
__device__ __forceinline__ u32 wave_read_u32(u32 x, int l) { return (u32)__builtin_amdgcn_readlane((int)x, l); }
