// mmidx_learn_kernels.h -- kernels of the batched product-quantizer learner (mmidx_pq_learn_device).
// Included by mmidx_learn.hip alone.
//
// A "job" is a (sub-space, k-means seed) pair: all jobs have the same shape (n points of dsub doubles, ks centres), so every
// kernel here serves a list of jobs in one launch -- blockIdx.y walks the list.  A PlSlot names the job a list entry stands for.
// Every floating-point result is a function of its own job alone (fixed tile sizes, fixed summation orders, integer atomics
// only), so neither the other jobs of a launch nor the grouping of the jobs changes a bit of it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#define PL_BLOCK 256
#define PL_IPT 8                       // consecutive items a thread scans
#define PL_TILE (PL_BLOCK * PL_IPT)    // items per scan tile
#define PL_PPT 4                       // points per thread in the assignment (one broadcast read serves four chains)
#define PL_APTS (PL_BLOCK * PL_PPT)    // points per assignment block
#define PL_MAX_DSUB 16

struct PlSlot {
    int32_t jl;     // job, local to the group: row of the per-job arrays
    int32_t sub;    // its sub-space: which [n][dsub] slab of the data
    int32_t k_eff;  // centres it has left
    int32_t force;  // 1 = every point counts as moved (first iteration, or the numbering changed after a drop)
};

// ---- prep ---------------------------------------------------------------------------------------------------------------------
// residual (centroid - x, IVFPQ.java:645) -> transform (permutation out[i] = r[perm[i]]; rotation sum_i r[i] rot[i][j], i ascending:
// the arithmetic of k_encode_pq) -> sub-space-major Y[m][n][dsub].  One thread per output element.
__global__ __launch_bounds__(PL_BLOCK) void k_pl_prep(const double *__restrict__ X, const int32_t *__restrict__ cell,
                                                      const double *__restrict__ coarse, const int32_t *__restrict__ perm,
                                                      const double *__restrict__ rot, double *__restrict__ Y, long long n, int D, int dsub,
                                                      int transform, int ivf) {
    const long long e = (long long)blockIdx.x * PL_BLOCK + threadIdx.x;
    if (e >= n * D) return;
    const long long v = e / D;
    const int j = (int)(e - v * D);
    const double *x = X + (size_t)v * D;
    const double *c = ivf ? coarse + (size_t)cell[v] * D : nullptr;
    double val;
    if (transform == 1) {
        double total = 0.0;
        for (int i = 0; i < D; i++) {
            const double r = ivf ? c[i] - x[i] : x[i];
            total += r * rot[(size_t)i * D + j];
        }
        val = total;
    } else {
        const int i = transform == 2 ? perm[j] : j;
        val = ivf ? c[i] - x[i] : x[i];
    }
    const int s = j / dsub;
    Y[((size_t)s * n + (size_t)v) * dsub + (j - s * dsub)] = val;
}

// per attribute minimum / maximum of Y[m][n][dsub]: one block per attribute (sub-space s, dimension jj), mn / mx [m * dsub]
__global__ __launch_bounds__(PL_BLOCK) void k_pl_minmax(const double *__restrict__ Y, long long n, int dsub, double *__restrict__ mn,
                                                        double *__restrict__ mx) {
    const int s = blockIdx.x / dsub, jj = blockIdx.x - s * dsub;
    const double *col = Y + (size_t)s * n * dsub + jj;
    double lo = __longlong_as_double(0x7FF0000000000000ll), hi = -lo;
    for (long long i = threadIdx.x; i < n; i += PL_BLOCK) {
        const double v = col[(size_t)i * dsub];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    __shared__ double s_lo[PL_BLOCK], s_hi[PL_BLOCK];
    s_lo[threadIdx.x] = lo;
    s_hi[threadIdx.x] = hi;
    __syncthreads();
    for (int off = PL_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            s_lo[threadIdx.x] = s_lo[threadIdx.x + off] < s_lo[threadIdx.x] ? s_lo[threadIdx.x + off] : s_lo[threadIdx.x];
            s_hi[threadIdx.x] = s_hi[threadIdx.x + off] > s_hi[threadIdx.x] ? s_hi[threadIdx.x + off] : s_hi[threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        mn[blockIdx.x] = s_lo[0];
        mx[blockIdx.x] = s_hi[0];
    }
}

// (y - min) / (max - min), 0 for a constant attribute (weka.core.NormalizableDistance.norm)
__global__ __launch_bounds__(PL_BLOCK) void k_pl_normalize(const double *__restrict__ Y, double *__restrict__ Yn, const double *__restrict__ mn,
                                                           const double *__restrict__ mx, long long n, int dsub, long long total) {
    const long long e = (long long)blockIdx.x * PL_BLOCK + threadIdx.x;
    if (e >= total) return;
    const long long row = e / dsub;  // s * n + i
    const int a = (int)(row / n) * dsub + (int)(e - row * dsub);
    const double r = mx[a] - mn[a];
    Yn[e] = r > 0.0 ? (Y[e] - mn[a]) / r : 0.0;
}

// ---- k-means++ seeding ----------------------------------------------------------------------------------------------------------
// Inclusive sum of one tile: v[0..8) of thread t are items t * 8 .. t * 8 + 7 on entry and their inclusive sums within the tile on
// return.  Thread-sequential, then a shuffle scan of the 64 thread totals of a wave, then the waves in order: one fixed order,
// whatever the tile holds.  The tile's total is v[7] of the last thread.  s_wave: 4 doubles of LDS.
__device__ __forceinline__ void pl_tile_scan(double (&v)[PL_IPT], double *s_wave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 1; k < PL_IPT; k++) v[k] = v[k - 1] + v[k];
    double inc = v[PL_IPT - 1];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(inc, off);
        if (lane >= off) inc = o + inc;
    }
    double exc = __shfl_up(inc, 1);
    if (lane == 0) exc = 0.0;
    __syncthreads();  // (a caller's earlier reads of s_wave)
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    double base = 0.0;
    for (int w = 0; w < wave; w++) base += s_wave[w];
    const double pre = base + exc;
#pragma unroll
    for (int k = 0; k < PL_IPT; k++) v[k] = pre + v[k];
}

// one seeding step, first half: mind2[i] = min(mind2[i], |x_i - centre|^2) for the centre picked last (pick[jl][c - 1]), the sum
// over the dimensions sequential; and the sum of the tile.  grid (tiles, jobs)
__global__ __launch_bounds__(PL_BLOCK) void k_pl_pp_update(const double *__restrict__ W, const PlSlot *__restrict__ slots,
                                                           const int32_t *__restrict__ pick, double *__restrict__ mind2,
                                                           double *__restrict__ tsum, long long n, int dsub, int ks, int c, long long ntl) {
    __shared__ double s_c[PL_MAX_DSUB];
    __shared__ double s_wave[4];
    const PlSlot S = slots[blockIdx.y];
    const double *data = W + (size_t)S.sub * n * dsub;
    if ((int)threadIdx.x < dsub) s_c[threadIdx.x] = data[(size_t)pick[(size_t)S.jl * ks + (c - 1)] * dsub + threadIdx.x];
    __syncthreads();
    double *md = mind2 + (size_t)S.jl * n;
    const long long i0 = (long long)blockIdx.x * PL_TILE + (long long)threadIdx.x * PL_IPT;
    double v[PL_IPT];
#pragma unroll
    for (int k = 0; k < PL_IPT; k++) {
        const long long i = i0 + k;
        v[k] = 0.0;
        if (i < n) {
            const double *x = data + (size_t)i * dsub;
            double acc = 0.0;
            for (int j = 0; j < dsub; j++) {
                const double df = x[j] - s_c[j];
                acc += df * df;
            }
            const double old = md[i];
            v[k] = (c == 1 || acc < old) ? acc : old;
            md[i] = v[k];
        }
    }
    pl_tile_scan(v, s_wave);
    if (threadIdx.x == PL_BLOCK - 1) tsum[(size_t)S.jl * ntl + blockIdx.x] = v[PL_IPT - 1];
}

// second half: the inclusive sums of the job's tile sums (tinc), target = prob * total formed here, the first tile whose sum passes
// the target, and inside it the first point whose cumulative sum does: pick[jl][c].  No point passes it: n - 1.  One block per job.
__global__ __launch_bounds__(PL_BLOCK) void k_pl_pp_pick(const double *__restrict__ mind2, const double *__restrict__ tsum,
                                                         double *__restrict__ tinc, const double *__restrict__ prob,
                                                         const PlSlot *__restrict__ slots, int32_t *__restrict__ pick, long long n, int ks,
                                                         int c, long long ntl) {
    __shared__ double s_wave[4];
    __shared__ double s_carry;
    __shared__ long long s_min;
    const PlSlot S = slots[blockIdx.x];
    const double *ts = tsum + (size_t)S.jl * ntl;
    double *ti = tinc + (size_t)S.jl * ntl;
    const double *md = mind2 + (size_t)S.jl * n;
    const long long none = 0x7fffffffffffffffll;
    double carry = 0.0;
    double v[PL_IPT];
    for (long long t0 = 0; t0 < ntl; t0 += PL_TILE) {
        const long long b = t0 + (long long)threadIdx.x * PL_IPT;
#pragma unroll
        for (int k = 0; k < PL_IPT; k++) v[k] = b + k < ntl ? ts[b + k] : 0.0;
        pl_tile_scan(v, s_wave);
#pragma unroll
        for (int k = 0; k < PL_IPT; k++)
            if (b + k < ntl) ti[b + k] = carry + v[k];
        if (threadIdx.x == PL_BLOCK - 1) s_carry = carry + v[PL_IPT - 1];
        __syncthreads();
        carry = s_carry;
        __syncthreads();
    }
    const double target = prob[(size_t)S.jl * (ks - 1) + (c - 1)] * carry;
    if (threadIdx.x == 0) s_min = none;
    __syncthreads();  // (also: the tinc written above is visible to the whole block)
    for (long long t = threadIdx.x; t < ntl; t += PL_BLOCK)
        if (ti[t] > target) {
            atomicMin((unsigned long long *)&s_min, (unsigned long long)t);
            break;
        }
    __syncthreads();
    const long long tsel = s_min;
    __syncthreads();
    long long idx = n - 1;
    if (tsel != none) {
        const double base = tsel > 0 ? ti[tsel - 1] : 0.0;
        const long long i0 = tsel * PL_TILE + (long long)threadIdx.x * PL_IPT;
#pragma unroll
        for (int k = 0; k < PL_IPT; k++) v[k] = i0 + k < n ? md[i0 + k] : 0.0;
        pl_tile_scan(v, s_wave);
        if (threadIdx.x == 0) s_min = none;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PL_IPT; k++)
            if (i0 + k < n && base + v[k] > target) {
                atomicMin((unsigned long long *)&s_min, (unsigned long long)(i0 + k));
                break;
            }
        __syncthreads();
        const long long last = (tsel + 1) * PL_TILE - 1;
        idx = s_min != none ? s_min : (last < n - 1 ? last : n - 1);
    }
    if (threadIdx.x == 0) pick[(size_t)S.jl * ks + c] = (int32_t)idx;
}

// the picked rows -> the job's table Ctab[jl][ks][dsub].  grid (ceil(ks * dsub / 256), jobs)
__global__ __launch_bounds__(PL_BLOCK) void k_pl_gather_seeds(const double *__restrict__ W, const PlSlot *__restrict__ slots,
                                                              const int32_t *__restrict__ pick, double *__restrict__ Ctab, long long n,
                                                              int dsub, int ks) {
    const int e = blockIdx.x * PL_BLOCK + threadIdx.x;
    if (e >= ks * dsub) return;
    const PlSlot S = slots[blockIdx.y];
    const int c = e / dsub, j = e - c * dsub;
    Ctab[(size_t)S.jl * ks * dsub + e] = W[((size_t)S.sub * n + (size_t)pick[(size_t)S.jl * ks + c]) * dsub + j];
}

__global__ __launch_bounds__(PL_BLOCK) void k_pl_iota_mod(int32_t *__restrict__ v, long long n, long long total) {
    const long long e = (long long)blockIdx.x * PL_BLOCK + threadIdx.x;
    if (e < total) v[e] = (int32_t)(e % n);
}

// ---- Lloyd: assignment ------------------------------------------------------------------------------------------------------------
// grid (ceil(n / PL_APTS), active jobs).  The block stages its job's table (k_eff x dsub doubles) in LDS; a thread keeps PL_PPT
// points in registers and walks the table with broadcast reads (every lane reads the same address): df = c - x; acc += df * df,
// dimension ascending, unfused; strict <, so the first minimum wins.  It writes the assignment in place, the sort key
// slot * ks + cluster, and counts the points that moved and the members per cluster: integers, an LDS histogram per block.
// dynamic LDS: k_eff * dsub doubles + k_eff ints.  DS = dsub rounded up to 4, 8 or 16 (the register array's length).
template <int DS>
__global__ __launch_bounds__(PL_BLOCK) void k_pl_assign(const double *__restrict__ W, const PlSlot *__restrict__ slots,
                                                        const double *__restrict__ Ctab, int32_t *__restrict__ assign,
                                                        uint32_t *__restrict__ keys, int32_t *__restrict__ counts,
                                                        uint32_t *__restrict__ changed, long long n, int dsub, int ks) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pl_smem[];
    const int slot = blockIdx.y;
    const PlSlot S = slots[slot];
    const int k_eff = S.k_eff;
    double *tab = (double *)pl_smem;
    int *hist = (int *)(tab + (size_t)k_eff * dsub);
    const double *ct = Ctab + (size_t)S.jl * ks * dsub;
    for (int e = threadIdx.x; e < k_eff * dsub; e += PL_BLOCK) tab[e] = ct[e];
    for (int e = threadIdx.x; e < k_eff; e += PL_BLOCK) hist[e] = 0;
    const double *data = W + (size_t)S.sub * n * dsub;
    const long long i0 = (long long)blockIdx.x * PL_APTS + threadIdx.x;
    double x[PL_PPT][DS], best[PL_PPT];
    int bi[PL_PPT];
#pragma unroll
    for (int p = 0; p < PL_PPT; p++) {
        long long i = i0 + (long long)p * PL_BLOCK;
        i = i < n ? i : n - 1;
#pragma unroll
        for (int j = 0; j < DS; j++) x[p][j] = j < dsub ? data[(size_t)i * dsub + j] : 0.0;
        best[p] = __longlong_as_double(0x7FF0000000000000ll);
        bi[p] = 0;
    }
    __syncthreads();
    for (int c = 0; c < k_eff; c++) {
        const double *row = tab + (size_t)c * dsub;
        double acc[PL_PPT];
#pragma unroll
        for (int p = 0; p < PL_PPT; p++) acc[p] = 0.0;
#pragma unroll
        for (int j = 0; j < DS; j++) {
            if (j < dsub) {
                const double cj = row[j];
#pragma unroll
                for (int p = 0; p < PL_PPT; p++) {
                    const double df = cj - x[p][j];
                    acc[p] += df * df;
                }
            }
        }
#pragma unroll
        for (int p = 0; p < PL_PPT; p++)
            if (acc[p] < best[p]) {
                best[p] = acc[p];
                bi[p] = c;
            }
    }
    int32_t *a = assign + (size_t)S.jl * n;
    uint32_t *kk = keys + (size_t)slot * n;
    unsigned moved = 0;
#pragma unroll
    for (int p = 0; p < PL_PPT; p++) {
        const long long i = i0 + (long long)p * PL_BLOCK;
        if (i < n) {
            const int old = S.force ? -1 : a[i];
            a[i] = bi[p];
            kk[i] = (uint32_t)slot * (uint32_t)ks + (uint32_t)bi[p];
            atomicAdd(hist + bi[p], 1);
            moved += old != bi[p];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) moved += __shfl_down(moved, off);
    if ((threadIdx.x & 63) == 0 && moved) atomicAdd(changed + slot, moved);
    __syncthreads();
    for (int e = threadIdx.x; e < k_eff; e += PL_BLOCK)
        if (hist[e]) atomicAdd(counts + (size_t)slot * ks + e, hist[e]);
}

// ---- Lloyd: means -----------------------------------------------------------------------------------------------------------------
// sorted[] holds the point indices of every listed slot grouped by (slot, cluster), ascending inside a group (a stable sort of the
// keys).  One thread per (surviving cluster t, dimension j): the members' values added up in that order from 0.0, divided by
// their number -- 64 / dsub clusters to a wave.  rng_a / rng_b [slot][t]: the group's range in sorted[], survivors in their order,
// so the table comes out compacted.  lst (may be null: the slots 0 .. gridDim.y) names the slots to serve.
// grid (ceil(ks * dsub / 256), slots)
__global__ __launch_bounds__(PL_BLOCK) void k_pl_means(const double *__restrict__ data_all, const PlSlot *__restrict__ slots,
                                                       const int32_t *__restrict__ lst, const int32_t *__restrict__ sorted,
                                                       const int32_t *__restrict__ rng_a, const int32_t *__restrict__ rng_b,
                                                       const int32_t *__restrict__ kept, double *__restrict__ Cout, long long n, int dsub,
                                                       int ks) {
    const int slot = lst ? lst[blockIdx.y] : (int)blockIdx.y;
    const int e = blockIdx.x * PL_BLOCK + threadIdx.x;
    const int t = e / dsub, j = e - t * dsub;
    if (t >= kept[slot]) return;
    const PlSlot S = slots[slot];
    const double *data = data_all + (size_t)S.sub * n * dsub + j;
    const int a = rng_a[(size_t)slot * ks + t], b = rng_b[(size_t)slot * ks + t];
    double acc = 0.0;
    int q = a;
    for (; q + 4 <= b; q += 4) {
        const int i0 = sorted[q], i1 = sorted[q + 1], i2 = sorted[q + 2], i3 = sorted[q + 3];
        const double v0 = data[(size_t)i0 * dsub], v1 = data[(size_t)i1 * dsub], v2 = data[(size_t)i2 * dsub], v3 = data[(size_t)i3 * dsub];
        acc += v0;
        acc += v1;
        acc += v2;
        acc += v3;
    }
    for (; q < b; q++) acc += data[(size_t)sorted[q] * dsub];
    Cout[((size_t)S.jl * ks + t) * dsub + j] = acc / (double)(b - a);
}

// ---- final ------------------------------------------------------------------------------------------------------------------------
// |x_i - C[remap[a_i]]|^2 per point of the listed slots (remap: cluster -> its row in the compacted table).  grid (ceil(n / 256), slots)
__global__ __launch_bounds__(PL_BLOCK) void k_pl_sqerr(const double *__restrict__ W, const PlSlot *__restrict__ slots,
                                                       const int32_t *__restrict__ lst, const double *__restrict__ Ctab,
                                                       const int32_t *__restrict__ assign, const int32_t *__restrict__ remap,
                                                       double *__restrict__ perr, long long n, int dsub, int ks) {
    const long long i = (long long)blockIdx.x * PL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int slot = lst[blockIdx.y];
    const PlSlot S = slots[slot];
    const double *x = W + ((size_t)S.sub * n + (size_t)i) * dsub;
    const double *c = Ctab + ((size_t)S.jl * ks + remap[(size_t)slot * ks + assign[(size_t)S.jl * n + i]]) * dsub;
    double acc = 0.0;
    for (int j = 0; j < dsub; j++) {
        const double df = x[j] - c[j];
        acc += df * df;
    }
    perr[(size_t)S.jl * n + i] = acc;
}

// the per-point values of a job added up in index order from 0.0 (one chain: thread 0 walks tiles the block stages in LDS).
// One block per listed slot.
__global__ __launch_bounds__(PL_BLOCK) void k_pl_seqsum(const double *__restrict__ perr, const PlSlot *__restrict__ slots,
                                                        const int32_t *__restrict__ lst, double *__restrict__ sse, long long n) {
    __shared__ double buf[PL_TILE];
    const PlSlot S = slots[lst[blockIdx.x]];
    const double *pe = perr + (size_t)S.jl * n;
    double s = 0.0;
    for (long long i0 = 0; i0 < n; i0 += PL_TILE) {
        const int cnt = (int)(n - i0 < PL_TILE ? n - i0 : PL_TILE);
        for (int e = threadIdx.x; e < cnt; e += PL_BLOCK) buf[e] = pe[i0 + e];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int e = 0; e < cnt; e++) s += buf[e];
        __syncthreads();
    }
    if (threadIdx.x == 0) sse[S.jl] = s;
}
