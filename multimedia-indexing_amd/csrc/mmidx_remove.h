// mmidx_remove.h -- K13: records taken back out of the list-major arrays (mmidx_remove).
//
// A stable stream compaction over the n records in list-major order: one global compaction keeps the order of the lists and the
// arrival order inside every list, and a list's new start is the number of survivors in front of its old start.  Five launches, none
// of which waits for another block:
//   K13a k_rm_mark     one bit per requested iid in a bitmap over [0, inv_size); found[i] from the iid -> position table
//   K13b k_rm_flags    a wave loads 64 ids, tests the bitmap, writes the ballot as one 64-bit keep word; a tile writes its survivor count
//   K13c k_rm_scan     one block walks the tile counts: exclusive prefix, total at [ntiles]
//   K13d k_rm_offsets  one thread per list boundary: tile prefix + popcounts of the keep words in front of it inside its tile
//   K13e k_rm_compact  rank inside the wave = popcount of the keep word below the lane, + the words in front, + the tile prefix;
//                      the id and the record's bytes move as V-sized pieces (V = the widest type that divides the record)
// Included by mmidx_remove.hip alone (mmidx_host.h: one .hip per kernel header).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#define RM_TILE 2048                 // records per block: a power of two, at most 8192
#define RM_NT 256                    // threads per block (4 waves)
#define RM_WORDS (RM_TILE / 64)      // keep words per tile
#define RM_WPW (RM_WORDS / (RM_NT / 64))  // keep words (rounds of 64 records) per wave
#define RM_SCAN_NT 1024
static_assert((RM_TILE & (RM_TILE - 1)) == 0 && RM_TILE <= 8192 && RM_TILE >= RM_NT, "the tile is a power of two of at most 8192 records");
static_assert(RM_WORDS <= 64 * (RM_NT / 64) && RM_WORDS % (RM_NT / 64) == 0 && RM_WORDS <= 128, "a wave sums the words in front of it in two steps at most");

typedef unsigned long long rm_u64;

// K13a: req[nreq] -> bits; found (may be null) = 1 where the id was stored before the call.  An id outside [0, inv_size) sets nothing.
__global__ void k_rm_mark(const int32_t *__restrict__ req, long long nreq, const int32_t *__restrict__ inv, long long inv_size, long long n_csr,
                          unsigned *__restrict__ bits, int32_t *__restrict__ found) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nreq) return;
    const int32_t id = req[i];
    int f = 0;
    if (id >= 0 && id < inv_size) {
        const int32_t pos = inv[id];
        f = pos >= 0 && pos < n_csr;
        if (f) atomicOr(&bits[id >> 5], 1u << (id & 31));
    }
    if (found) found[i] = f;
}

// K13b: keep[w] bit l = record 64 w + l survives (bits past n are 0); tile_cnt[t] = survivors of tile t
__global__ __launch_bounds__(RM_NT) void k_rm_flags(const int32_t *__restrict__ ids, long long n, const unsigned *__restrict__ bits, long long inv_size,
                                                    rm_u64 *__restrict__ keep, unsigned *__restrict__ tile_cnt) {
    __shared__ unsigned s_cnt[RM_NT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w0 = (long long)blockIdx.x * RM_WORDS + (long long)wave * RM_WPW;
    unsigned cnt = 0;
    for (int r = 0; r < RM_WPW; r++) {
        const long long pos = (w0 + r) * 64 + lane;
        int k = 0;
        if (pos < n) {
            const int32_t id = ids[pos];
            k = 1;
            if (id >= 0 && id < inv_size) k = !((bits[id >> 5] >> (id & 31)) & 1u);
        }
        const rm_u64 word = __ballot(k);
        if (lane == 0 && (w0 + r) * 64 < n) keep[w0 + r] = word;
        cnt += (unsigned)__popcll(word);
    }
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int w = 0; w < RM_NT / 64; w++) t += s_cnt[w];
        tile_cnt[blockIdx.x] = t;
    }
}

// K13c: one block; pre[t] = survivors in tiles 0 .. t - 1, pre[ntiles] = all of them
__global__ __launch_bounds__(RM_SCAN_NT) void k_rm_scan(const unsigned *__restrict__ tile_cnt, long long ntiles, long long *__restrict__ pre) {
    __shared__ long long s_w[RM_SCAN_NT / 64];
    __shared__ long long s_carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (long long base = 0; base < ntiles; base += RM_SCAN_NT) {
        const long long t = base + threadIdx.x;
        const long long v = t < ntiles ? (long long)tile_cnt[t] : 0;
        long long inc = v;  // inclusive scan inside the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        long long front = s_carry;
        for (int w = 0; w < wave; w++) front += s_w[w];
        if (t < ntiles) pre[t] = front + inc - v;
        __syncthreads();
        if (threadIdx.x == RM_SCAN_NT - 1) s_carry = front + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) pre[ntiles] = s_carry;
}

// survivors among the records of tile `tile` in front of position p (p inside the tile, or its end)
__device__ __forceinline__ long long rm_rank_in_tile(const rm_u64 *__restrict__ keep, long long tile, long long p) {
    const long long wfirst = tile * RM_WORDS, wp = p >> 6;
    long long r = 0;
    for (long long w = wfirst; w < wp; w++) r += __popcll(keep[w]);
    const int b = (int)(p & 63);
    if (b) r += __popcll(keep[wp] & ((1ull << b) - 1ull));
    return r;
}

// K13d: off_new[c] for c = 0 .. nlists
__global__ void k_rm_offsets(const long long *__restrict__ off_old, int nlists, long long n, const rm_u64 *__restrict__ keep,
                             const long long *__restrict__ pre, long long ntiles, long long *__restrict__ off_new) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > nlists) return;
    const long long p = off_old[c];
    if (p >= n) {
        off_new[c] = pre[ntiles];
        return;
    }
    const long long tile = p / RM_TILE;
    off_new[c] = pre[tile] + rm_rank_in_tile(keep, tile, p);
}

// K13e: the survivors to their new places.  V: the widest of uint4 / uint2 / unsigned / unsigned short / unsigned char that divides
// the record's rb bytes (16-byte records: one load and one store per lane; 6-byte records: three shorts); nv = rb / sizeof(V).
// The arrays start on hipMalloc's alignment, so record e starts on a multiple of sizeof(V).
template <typename V>
__global__ __launch_bounds__(RM_NT) void k_rm_compact(const int32_t *__restrict__ ids, const V *__restrict__ codes, long long n, int nv,
                                                      const rm_u64 *__restrict__ keep, const long long *__restrict__ pre, int32_t *__restrict__ ids_new,
                                                      V *__restrict__ codes_new) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long wtile = (long long)blockIdx.x * RM_WORDS;
    const long long nwords = (n + 63) >> 6;
    // survivors of this tile in front of the wave's first word
    int front = 0;
    for (int w = lane; w < wave * RM_WPW; w += 64)
        if (wtile + w < nwords) front += __popcll(keep[wtile + w]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) front += __shfl_xor(front, d);
    long long dst0 = pre[blockIdx.x] + front;
    for (int r = 0; r < RM_WPW; r++) {
        const long long w = wtile + (long long)wave * RM_WPW + r;
        if (w >= nwords) break;  // (uniform over the wave)
        const rm_u64 word = keep[w];
        if ((word >> lane) & 1ull) {
            const long long src = w * 64 + lane;
            const long long dst = dst0 + __popcll(word & ((1ull << lane) - 1ull));
            ids_new[dst] = ids[src];
            const V *s = codes + src * nv;
            V *d = codes_new + dst * nv;
            for (int t = 0; t < nv; t++) d[t] = s[t];
        }
        dst0 += __popcll(word);
    }
}
