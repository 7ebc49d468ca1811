// mmidx_split16.h -- the certified "bf16-split" dot product, written once: the pieces that K1e / K1e' / K1e'' (coarse stage),
// K6a' (assignment), K8'' (VLAD) and the Linear sweep are assembled from.  A kernel's body keeps its schedule -- how a tile
// reaches LDS, which barriers and waits surround the products -- and takes everything else from here.
//
// Device only: __device__ __forceinline__ functions and constants, no __global__ and no __shared__ definition, so -- unlike a
// kernel header -- any number of units may include it.
//
// ------------------------------------------------------------------------------------------------
// K1e + K1f: the same certified selection without materialising the [nq][C] matrix of d~.
//
// K1c writes 4 bytes per (query, centroid) and K1d reads them back -- 1 GiB of HBM traffic per 16384
// queries at C = 8192 -- although only ~w+3 entries per row matter.  Here the dot products run on the
// bf16 matrix cores with a two-term split (x = xh + xl + O(2^-16 x); q.c ~ qh.ch + qh.cl + ql.ch, each
// product exact in fp32), 16x the fp32 MFMA rate, and the epilogue keeps, per group of 8 centroids (the 8
// columns one lane holds for a row: no cross-lane work), the smallest d~, its position and the runner-up
// (K1e: [nq][C/8] float2, a quarter of the traffic).  K1f then
//   * takes tau = (w+1)-th smallest of its 256 per-thread minima + eps16: w+1 distinct centroids have an
//     exact distance <= their d~ + eps16, so tau bounds the (w+1)-th smallest exact distance;
//   * nominates the minimum of every group with d~ <= tau + eps16 (any centroid with exact distance <= tau
//     satisfies that), and all 8 members of a group whose runner-up passes too (rare: 8 (w+1) / C);
//   * hands the nominees to the shared exact second half.
// Error bound of the split dot product (|x - xh - xl| <= 2^-16 |x| elementwise, |xl| <= 2^-8 |x|):
//   |q.c - (qh.ch + qh.cl + ql.ch)| <= 3.1 * 2^-16 |q||c|   (dropped terms, Cauchy-Schwarz)
//   accumulation of 3D exact products in fp32, any order, at most 2^-22 relative per step (twice the IEEE
//   unit roundoff: the MFMA's internal summation order and rounding are not documented)
//                                   <= (3D + 16) 2^-22 |q||c|
//   d~ = |c|^2 + |q|^2 - 2 S evaluated in fp32 from fp32 copies of the norms: 2^-21 (|c| + |q|)^2
// ------------------------------------------------------------------------------------------------
//
// Conventions of every function below.  A wave owns 32 rows (queries / vectors) [q0, q0 + 32) as two 16-row A tiles;
// fr = lane & 15, fg = lane >> 4.  Fragments of v_mfma_f32_16x16x32_bf16: lane l holds A[row l & 15][k = 8 (l >> 4) ..] and
// B[k = 8 (l >> 4) ..][col l & 15]; result register r of lane l is (row 4 (l >> 4) + r, col l & 15).  Rows past n are clamped
// for the loads (in bounds) and never stored.
#pragma once
#include "mmidx_device_util.h"
#include "mmidx_host.h"  // G16_BC, G16_KC, G16_STRIDE

constexpr int SPLIT16_HROWS = G16_BC / 2;                  // centroids per half tile of the LDS-DMA kernels
constexpr int SPLIT16_HBYTES = SPLIT16_HROWS * G16_KC * 2;  // 16 KiB per part (head / tail) of a half tile: 128 bf16 = 256 B = 16 units per row

// f -> (head, tail)
__device__ __forceinline__ void split16_head_tail(const float f, __bf16 &h, __bf16 &l) {
    h = (__bf16)f;
    l = (__bf16)(f - (float)h);  // f - h is exact in fp32
}

// row-wise minimum over the 16 lanes that share lane >> 4 (all of them receive it); VALU only
__device__ __forceinline__ float row16_min(float v) {
    float o;
    o = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
    v = o < v ? o : v;
    o = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
    v = o < v ? o : v;
    o = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xf, 0xf, true));  // row_half_mirror
    v = o < v ? o : v;
    o = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xf, 0xf, true));  // row_mirror
    v = o < v ? o : v;
    return v;
}
// one DPP step of the merge below
template <int CTRL>
__device__ __forceinline__ void row16_best2_step(float &m1, int &ix, float &m2) {
    const float o1 = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(m1), CTRL, 0xf, 0xf, true));
    const float o2 = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(m2), CTRL, 0xf, 0xf, true));
    const int oi = __builtin_amdgcn_mov_dpp(ix, CTRL, 0xf, 0xf, true);
    const bool take = o1 < m1 || (o1 == m1 && oi < ix);
    const float hi1 = take ? m1 : o1;  // the larger of the two bests
    const float lo2 = o2 < m2 ? o2 : m2;
    m2 = hi1 < lo2 ? hi1 : lo2;
    ix = take ? oi : ix;
    m1 = take ? o1 : m1;
}
// (best, its index, second best) merged over the same 16 lanes, the smaller index winning a tie; the steps of row16_min
__device__ __forceinline__ void row16_best2_merge(float &m1, int &ix, float &m2) {
    row16_best2_step<0xB1>(m1, ix, m2);
    row16_best2_step<0x4E>(m1, ix, m2);
    row16_best2_step<0x141>(m1, ix, m2);
    row16_best2_step<0x140>(m1, ix, m2);
}

// the centroid tiles [t_lo, t_hi) of block y of ny (gridDim.y, blockIdx.y: unsigned, so the division is)
__device__ __forceinline__ void split16_tile_range(const int ntiles, const unsigned ny, const unsigned y, int &t_lo, int &t_hi) {
    const int t_per = (ntiles + ny - 1) / ny;
    t_lo = y * t_per;
    t_hi = (t_lo + t_per < ntiles) ? t_lo + t_per : ntiles;
}

// the squared norms of the eight rows a lane holds results for, as fp32; zero past n.
// UNCOND (K1e''): the load itself is unconditional, from a clamped row: a load under a condition is branched around and waited
// for on its own, eight round trips in a row
template <bool UNCOND = false, typename IDX>
__device__ __forceinline__ void split16_row_norms(float (&qn_r)[2][4], const double *__restrict__ qn, const IDX q0, const IDX n, const int fg) {
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const IDX q = q0 + rt * 16 + 4 * fg + r;
            if constexpr (UNCOND) {
                const float v = (float)qn[q < n ? q : n - 1];
                qn_r[rt][r] = q < n ? v : 0.0f;
            } else {
                qn_r[rt][r] = q < n ? (float)qn[q] : 0.0f;
            }
        }
}

// A fragments of the k chunk that starts at kbase, from the bf16 copies: [row tile][k step of 32].
// ZFILL: zeros past Dp (a short last chunk); off for the kernels whose chunks are always whole (Dp a multiple of 128)
template <bool ZFILL, typename IDX>
__device__ __forceinline__ void split16_load_a(bf16x8 (&ah)[2][4], bf16x8 (&al)[2][4], const __bf16 *__restrict__ Qh, const __bf16 *__restrict__ Ql,
                                               const IDX q0, const IDX n, const int Dp, const int kbase, const int fr, const int fg) {
#pragma unroll
    for (int rt = 0; rt < 2; rt++) {
        IDX q = q0 + rt * 16 + fr;
        q = q < n ? q : n - 1;
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
            const int k = kbase + ks * 32 + fg * 8;
            bf16x8 h = {}, l = {};
            if (!ZFILL || k < Dp) {
                h = *(const bf16x8 *)(Qh + (size_t)q * Dp + kbase + ks * 32 + fg * 8);
                l = *(const bf16x8 *)(Ql + (size_t)q * Dp + kbase + ks * 32 + fg * 8);
            }
            ah[rt][ks] = h;
            al[rt][ks] = l;
        }
    }
}

// A fragments straight from the fp64 rows X[n][D] (D a multiple of 8, one k chunk: D <= 32 KS; zeros past D) -- head / tail
// split in registers -- with xrow[rt] = ||x||^2 (rounded up) of row rt * 16 + fr, in all four lanes that share fr, and its fp32
// copies for the rows a lane holds results for
template <int KS, typename IDX>
__device__ __forceinline__ void split16_load_a_fp64(bf16x8 (&ah)[2][KS], bf16x8 (&al)[2][KS], double (&xrow)[2], float (&xn_r)[2][4],
                                                    const double *__restrict__ X, const IDX q0, const IDX n, const int D, const int fr, const int fg) {
#pragma unroll
    for (int rt = 0; rt < 2; rt++) {
        IDX q = q0 + rt * 16 + fr;
        q = q < n ? q : n - 1;
        double pn = 0.0;
#pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            const int k = ks * 32 + fg * 8;
            bf16x8 h = {}, l = {};
            if (k < D) {  // (D a multiple of 8: a lane's eight values are all inside the row or all padding)
                const double2 *xp = (const double2 *)(X + (size_t)q * D + k);
                const double2 v0 = xp[0], v1 = xp[1], v2 = xp[2], v3 = xp[3];
                const double vv[8] = {v0.x, v0.y, v1.x, v1.y, v2.x, v2.y, v3.x, v3.y};
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const float f = (float)vv[e];
                    const __bf16 hh = (__bf16)f;
                    h[e] = hh;
                    l[e] = (__bf16)(f - (float)hh);  // f - head is exact in fp32
                    pn += vv[e] * vv[e];
                }
            }
            ah[rt][ks] = h;
            al[rt][ks] = l;
        }
        pn += __shfl_xor(pn, 16);
        pn += __shfl_xor(pn, 32);
        xrow[rt] = pn * (1.0 + 1e-12);  // only ever used inside error bounds: round up (as k_split_bf16)
#pragma unroll
        for (int r = 0; r < 4; r++) xn_r[rt][r] = (float)__shfl(xrow[rt], 4 * fg + r);
    }
}

// The three products of one accumulator for one k step.  THE BIT-LEVEL CONTRACT of the split: every accumulator sees
// h.h, h.l, l.h in this order, k steps ascending; the certificate and the equality of K1e' and K1e'' rest on it.
__device__ __forceinline__ void split16_mma_one(f32x4 &acc, const bf16x8 &ah, const bf16x8 &al, const bf16x8 &bh, const bf16x8 &bl) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
}
// The products of NCT column tiles x 2 row tiles for k step ks: acc[rt][ct0 .. ct0 + NCT) += A x B, all h.h, then all h.l,
// then all l.h (2 NCT independent accumulators between dependent matrix instructions) -- per accumulator the order of the
// contract above.
template <int NCT, int NACC, int KS>
__device__ __forceinline__ void split16_mma_step(f32x4 (&acc)[2][NACC], const int ct0, const bf16x8 (&ah)[2][KS], const bf16x8 (&al)[2][KS],
                                                 const int ks, const bf16x8 (&bh)[NCT], const bf16x8 (&bl)[NCT]) {
#pragma unroll
    for (int u = 0; u < NCT; u++)
#pragma unroll
        for (int rt = 0; rt < 2; rt++) acc[rt][ct0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[rt][ks], bh[u], acc[rt][ct0 + u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < NCT; u++)
#pragma unroll
        for (int rt = 0; rt < 2; rt++) acc[rt][ct0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[rt][ks], bl[u], acc[rt][ct0 + u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < NCT; u++)
#pragma unroll
        for (int rt = 0; rt < 2; rt++) acc[rt][ct0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[rt][ks], bh[u], acc[rt][ct0 + u], 0, 0, 0);
}
__device__ __forceinline__ void split16_zero_acc(f32x4 (&acc)[2][8]) {
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int ct = 0; ct < 8; ct++) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---- a tile staged global -> registers -> padded LDS rows of G16_STRIDE bytes (K1e, K6a') ----
// One k chunk (kbase, upr 16-byte units per row) of the 128 centroids from c0, head and tail, by a block of MMIDX_BLOCK threads.
__device__ __forceinline__ void split16_stage_tile(unsigned char *Bh, unsigned char *Bl, const __bf16 *__restrict__ Ch, const __bf16 *__restrict__ Cl,
                                                   const int c0, const int Dp, const int kbase, const int upr, const int tid) {
    if (upr == 16) {  // full-width chunk: all 16 loads of the thread in flight, then the LDS stores
        uint4 vh[8], vl[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int u = tid + i * 256, row = u >> 4, cu = u & 15;
            const size_t src = (size_t)(c0 + row) * Dp + kbase + cu * 8;
            vh[i] = *(const uint4 *)(Ch + src);
            vl[i] = *(const uint4 *)(Cl + src);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int u = tid + i * 256, row = u >> 4, cu = u & 15;
            *(uint4 *)(Bh + row * G16_STRIDE + cu * 16) = vh[i];
            *(uint4 *)(Bl + row * G16_STRIDE + cu * 16) = vl[i];
        }
    } else {
        for (int u = tid; u < G16_BC * upr; u += 256) {
            const int row = u / upr, cu = u - row * upr;
            const size_t src = (size_t)(c0 + row) * Dp + kbase + cu * 8;
            *(uint4 *)(Bh + row * G16_STRIDE + cu * 16) = *(const uint4 *)(Ch + src);
            *(uint4 *)(Bl + row * G16_STRIDE + cu * 16) = *(const uint4 *)(Cl + src);
        }
    }
}
__device__ __forceinline__ int split16_stage_frag_offset(const int row, const int ks, const int fg) { return row * G16_STRIDE + (ks * 32 + fg * 8) * 2; }
// the products of a staged chunk of kw columns (a multiple of 32) with all eight column tiles
__device__ __forceinline__ void split16_stage_products(f32x4 (&acc)[2][8], const bf16x8 (&ah)[2][4], const bf16x8 (&al)[2][4], const unsigned char *Bh,
                                                       const unsigned char *Bl, const int kw, const int fr, const int fg) {
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        if (ks * 32 < kw) {  // block-uniform
            // two column tiles at a time: four independent accumulators between dependent MFMAs
#pragma unroll
            for (int ct = 0; ct < 8; ct += 2) {
                bf16x8 bh[2], bl[2];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const int off = split16_stage_frag_offset((ct + u) * 16 + fr, ks, fg);
                    bh[u] = *(const bf16x8 *)(Bh + off);
                    bl[u] = *(const bf16x8 *)(Bl + off);
                }
                split16_mma_step<2>(acc, ct, ah, al, ks, bh, bl);
            }
        }
    }
}

// ---- a half tile by LDS-DMA (K1e', K1e'', K1e' for long vectors) ----
// The DMA writes lane-linear (wave-uniform base + lane x 16 B), so the rows cannot be padded; the 16-byte units of a row are
// XOR-swizzled instead -- unit u of row r is FETCHED into slot u ^ (r & 15) by choosing the lane's global address, and read back
// from that slot: the 16 lanes of a fragment read (rows r .. r + 15, same u) hit 16 different slots = all 64 banks.
// k chunk kbase of the 64 centroids from row0 into buf (head) and buf + SPLIT16_HBYTES (tail): 2 x (16 / NWAVES)
// wave-instructions of 1 KiB (4 rows) per wave
template <int NWAVES>
__device__ __forceinline__ void split16_dma_half(unsigned char *buf, const __bf16 *__restrict__ Ch, const __bf16 *__restrict__ Cl, const int row0,
                                                 const int Dp, const int kbase, const int wave, const int lane) {
#pragma unroll
    for (int i = 0; i < 16 / NWAVES; i++) {
        const int pu = (i * NWAVES + wave) * 64 + lane;  // 16-byte slot of the part this lane fills
        const int row = pu >> 4, slot = pu & 15;
        const size_t src = ((size_t)(row0 + row) * Dp + (size_t)kbase + (size_t)((slot ^ (row & 15)) * 8)) * 2;  // bytes
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)((const unsigned char *)Ch + src),
                                         (__attribute__((address_space(3))) void *)(buf + (i * NWAVES + wave) * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)((const unsigned char *)Cl + src),
                                         (__attribute__((address_space(3))) void *)(buf + SPLIT16_HBYTES + (i * NWAVES + wave) * 1024), 16, 0, 0);
    }
}
// the head part alone (k_coarse_screen16): 16 / NWAVES wave-instructions per wave, the same swizzle, buf holds SPLIT16_HBYTES
template <int NWAVES>
__device__ __forceinline__ void split16_dma_half_head(unsigned char *buf, const __bf16 *__restrict__ Ch, const int row0, const int Dp, const int kbase,
                                                      const int wave, const int lane) {
#pragma unroll
    for (int i = 0; i < 16 / NWAVES; i++) {
        const int pu = (i * NWAVES + wave) * 64 + lane;
        const int row = pu >> 4, slot = pu & 15;
        const size_t src = ((size_t)(row0 + row) * Dp + (size_t)kbase + (size_t)((slot ^ (row & 15)) * 8)) * 2;  // bytes
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)((const unsigned char *)Ch + src),
                                         (__attribute__((address_space(3))) void *)(buf + (i * NWAVES + wave) * 1024), 16, 0, 0);
    }
}
// where the fragment of (row, k step ks) lies in such a half (fr == row & 15)
__device__ __forceinline__ int split16_dma_frag_offset(const int row, const int ks, const int fg, const int fr) {
    return row * (G16_KC * 2) + (((ks * 4 + fg) ^ fr) * 16);
}
// the products of a half with its four column tiles: acc[rt][ct0 .. ct0 + 3] += A x B
__device__ __forceinline__ void split16_dma_products(f32x4 (&acc)[2][8], const int ct0, const bf16x8 (&ah)[2][4], const bf16x8 (&al)[2][4],
                                                     const unsigned char *buf, const int fr, const int fg) {
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
#pragma unroll
        for (int cp = 0; cp < 4; cp += 2) {
            bf16x8 bh[2], bl[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int off = split16_dma_frag_offset((cp + u) * 16 + fr, ks, fg, fr);
                bh[u] = *(const bf16x8 *)(buf + off);
                bl[u] = *(const bf16x8 *)(buf + SPLIT16_HBYTES + off);
            }
            split16_mma_step<2>(acc, ct0 + cp, ah, al, ks, bh, bl);
        }
    }
}

// ---- K1e's epilogue ----
// the +inf norm of a padding centroid as a finite "far"
__device__ __forceinline__ float split16_clamp_norm(const float cf) { return cf < 3.0e38f ? cf : 3.0e38f; }
// the clamped fp32 norms of the columns a lane holds of the tile at c0
__device__ __forceinline__ void split16_tile_norms(float (&cn_c)[8], const double *__restrict__ cn, const int c0, const int fr) {
#pragma unroll
    for (int ct = 0; ct < 8; ct++) cn_c[ct] = split16_clamp_norm((float)cn[c0 + ct * 16 + fr]);
}
// epilogue of tile t: d~ = |c|^2 + |q|^2 - 2 S.  A group = the 8 columns one lane holds for a row
// (c0 + fr + 16 ct, ct = 0..7): its two smallest d~ and the position of the smallest, no cross-lane work.
// The epilogue's VALU work was half of this kernel's time (timing experiment: 155 us with, 48 us without), so
// it is four instructions per value: t = fma(-2, S, |c|^2) (|q|^2, constant along the row, is added to the two
// survivors only), the column index packed into t's three low mantissa bits (v_and_or_b32: the minimum then
// carries its own position), runner-up = med3(best, runner-up, t), best = min(best, t).
// Roundings: fp32 copies of the norms, the fma, the final addition (4 x 2^-24) and the three borrowed bits
// (2^-20, on either survivor) -- inside eps16's last term (2^-21 + 2^-20)(|c| + |q|)^2.  Nothing here can
// overflow or produce a NaN: K1f sends rows with (|c|max + |q|)^2 >= 1e37 to the exact path before it looks at
// these values, and the +inf norms of the padding centroids are clamped to a finite "far".
// Output: gpair[q][G] = (smallest, second smallest | position of the smallest) of group 16 t + fr.
__device__ __forceinline__ void split16_gmin_store(const f32x4 (&acc)[2][8], const float (&cn_c)[8], const float (&qn_r)[2][4], const int q0, const int nq,
                                                   float2 *__restrict__ gpair, const int G, const int t, const int fr, const int fg) {
#pragma unroll
    for (int rt = 0; rt < 2; rt++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float m1 = __int_as_float(0x7f7ffff8), m2 = m1;  // (largest finite value with the position bits clear)
#pragma unroll
            for (int ct = 0; ct < 8; ct++) {
                const float tv = __builtin_fmaf(-2.0f, acc[rt][ct][r], cn_c[ct]);
                const float tp = __int_as_float((__float_as_int(tv) & ~7) | ct);
                m2 = __builtin_amdgcn_fmed3f(m1, m2, tp);
                // min(m1, tp) as the median with a value below everything (|t| < 1e37 here): a minnum of a value
                // assembled from bits would be preceded by a canonicalising v_max, a fifth instruction per value
                m1 = __builtin_amdgcn_fmed3f(m1, tp, -3.0e38f);
            }
            const int a1 = __float_as_int(m1) & 7;
            const float d1 = m1 + qn_r[rt][r];
            float d2 = m2 + qn_r[rt][r];
            d2 = d2 < 0.0f ? 0.0f : d2;
            // the position of the minimum rides in the 3 low mantissa bits of the runner-up (masked off by the reader)
            const float m2p = __int_as_float((__float_as_int(d2) & ~7) | a1);
            const int q = q0 + rt * 16 + 4 * fg + r;
            if (q < nq) gpair[(size_t)q * G + (size_t)t * 16 + fr] = make_float2(d1, m2p);
        }
    }
}
