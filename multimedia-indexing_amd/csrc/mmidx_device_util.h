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

// ------------------------------------------------------------------------------------------------
// The certificate of the coarse and assignment filters, written once (derivation: DESIGN.md 5.1).
//   d~ = |c|^2 + |x|^2 - 2 S,  S = the filter's fp32 dot product of the row x and the centroid c;  claim: |d~ - d| <= eps.
// Every kernel that decides on d~ (K1d, K1f and its front ends, K6a, K6a', K8'') takes eps from here and certifies a row only
// where filter_norms_usable() holds, so the copies cannot drift apart.
//   xnorm, xn2: |x| and |x|^2 (rounded up);  cnorm_max, cn2_max: the largest |c| and |c|^2 (rounded up).
//
// filter_underflow_eps: the ABSOLUTE part.  The relative terms below assume that no fp32 (or bf16) result leaves the normal range;
// one that does carries an error of up to one subnormal step (gradual underflow) or up to the smallest normal number 2^-126 (a unit
// that flushes).  Which of the two a conversion, a matrix-core product or a VALU operation applies is not something the kernels
// control or the documentation settles for every step, so the bound takes the larger, U = 2^-126, per operation:
//   elements: fl32(x_j), its bf16 head and its bf16 tail, three roundings, |x_j - (xh_j + xl_j)| <= 2^-16 |x_j| + 3 U, so the dot
//             product moves by at most 3.01 U (sum |c_j| + sum |x_j|) <= 3.01 U sqrt(Dk) (|c| + |x|), twice that in d~: 8 U sqrt(Dk) sumn
//             (the fp32 dot product of K1c / K6a rounds each element once: a third of it);
//   products and partial sums: at most 3 Dk products and 3 Dk additions, U each, doubled in d~: 12 Dk U;
//   the epilogue: two norm copies, the operations that combine them with S, the stored value, borrowed mantissa bits: 16 U.
// At ordinary magnitudes the term is below half a unit in the last place of eps: the certified sets do not change.
__device__ __forceinline__ double filter_underflow_eps(int Dk, double sumn) {
    return (12.0 * (double)Dk + 16.0 + 8.0 * sqrt((double)Dk) * sumn) * 0x1p-126;
}
// bf16 head / tail split, three matrix-core products accumulated in fp32 over Dp padded dimensions (K1e, K6a', K8'');
// epi: the epilogue's relative roundings -- 2^-21 (K6a', K8''), 2^-21 + 2^-20 (K1e: three mantissa bits carry a position)
__device__ __forceinline__ double filter_eps_split16(int Dp, double epi, double xnorm, double xn2, double cnorm_max, double cn2_max) {
    const double sumn = cnorm_max + xnorm;
    return (2.0 * 3.1 * 0x1p-16 * xnorm * cnorm_max + 2.0 * (3.0 * (double)Dp + 16.0) * 0x1p-22 * xnorm * cnorm_max +
            1e-12 * (cn2_max + xn2) + epi * sumn * sumn + filter_underflow_eps(Dp, sumn)) * (1.0 + 1e-9);
}
// bf16 heads alone, ONE matrix-core product accumulated in fp32 over Dp padded dimensions (K1s, the screen of the one-probe
// certificate: DESIGN.md 5.1, "The screen"); epi as above.  Term by term:
//   dropped cross terms: q.c - qh.ch = (q - qh).c + qh.(c - ch), |x - xh| <= 2^-8 |x| elementwise (the fp32 copy's rounding and the
//             head's), |qh| <= (1 + 2^-8) |q|:  <= 2.01 * 2^-8 |q||c|, doubled in d~;
//   accumulation of Dp exact products, any order, 2^-22 relative per step: (Dp + 16) 2^-22 |qh||ch| <= 1.01 (Dp + 16) 2^-22 |q||c|, doubled;
//   the norms' 1e-12 and the epilogue's epi (|c| + |q|)^2: as the split's;
//   the absolute part, recounted from filter_underflow_eps: elements -- fl32(x_j) and its head, two roundings, the dot product moves
//             by at most 2.01 U sqrt(Dk) (|c| + |x|), twice that in d~: 6 U sqrt(Dk) sumn; Dk products and Dk additions, doubled: 4 Dk U;
//             the epilogue's 16 U unchanged.
__device__ __forceinline__ double filter_underflow_eps_head(int Dk, double sumn) {
    return (4.0 * (double)Dk + 16.0 + 6.0 * sqrt((double)Dk) * sumn) * 0x1p-126;
}
__device__ __forceinline__ double filter_eps_head16(int Dp, double epi, double xnorm, double xn2, double cnorm_max, double cn2_max) {
    const double sumn = cnorm_max + xnorm;
    return (2.0 * 2.01 * 0x1p-8 * xnorm * cnorm_max + 2.0 * 1.01 * ((double)Dp + 16.0) * 0x1p-22 * xnorm * cnorm_max +
            1e-12 * (cn2_max + xn2) + epi * sumn * sumn + filter_underflow_eps_head(Dp, sumn)) * (1.0 + 1e-9);
}
// fp32 fused multiply-add chain over D dimensions, fp64 epilogue, d~ stored as fp32 (K1c / K1d, K6a)
__device__ __forceinline__ double filter_eps_fp32(int D, double xnorm, double xn2, double cnorm_max, double cn2_max) {
    const double sumn = cnorm_max + xnorm;
    return (2.0 * (double)(D + 3) * 0x1p-24 * 1.01 * xnorm * cnorm_max + 1e-12 * (cn2_max + xn2) + 0x1p-23 * sumn * sumn +
            filter_underflow_eps(D, sumn)) * (1.0 + 1e-9);
}
// A row is certified only while the fp32 quantities of the filter mean something: at (|c|max + |x|)^2 >= 1e37 a square or a dot
// product may have overflowed (an infinite dot product would make a far centroid look nearest), and at <= 1e-37 every one of
// them is subnormal or zero (the absolute term above already exceeds any gap there; the guard says so outright).  NaN fails both.
__device__ __forceinline__ bool filter_norms_usable(double sumn) { return sumn * sumn < 1e37 && sumn * sumn > 1e-37; }
