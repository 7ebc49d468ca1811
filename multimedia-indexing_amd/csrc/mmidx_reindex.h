// mmidx_reindex.h -- K12: truncate rows to up to eight lengths and L2-normalise them, in one pass.
//
// The arithmetic is Normalization.normalizeL2 (Normalization.java:21-37) literally: s = 0; s += y[i] * y[i] for i ascending, the
// product rounded before the add (-ffp-contract=off, and the product is a statement of its own), norm = sqrt(s), y[i] / norm, a zero
// norm -> every entry 1.0.  sqrt and / on fp64 are the correctly rounded forms under the build's flags (-fno-fast-math): the same two
// operations k_rows_normalize_l2 has always been compared bit for bit with the oracle on.  fp64 subnormals are never flushed on gfx950.
//
// A row's chain is sequential, so the parallelism is across rows: a block owns TRL_ROWS = 64 consecutive rows, and in the summing
// phase lane r of wave 0 walks row r column by column.  One chain serves every target: the running sum after entry T - 1 is the
// squared norm of the length-T target, so the walk stops at L = max(lens) and records sqrt(s) wherever a normalised target ends.
//
// HBM side: all 256 threads stage tiles of 64 rows x TRL_CT = 32 columns into LDS -- a lane loads 16 bytes (two doubles; 8-byte loads
// where ld is odd or the base is not 16-byte aligned), 16 lanes a contiguous 256-byte row segment -- into registers first, so that
// the loads of tile ct + 1 are in flight while wave 0 sums tile ct.  In LDS a row has an odd stride in doubles (33 for a staged tile):
// the 32-lane groups of wave 0's ds_read_b64 land on 32 distinct even banks.
//   CACHED   the block keeps all its truncated rows, [64][32 nct + 1] doubles: the scaled outputs are produced from LDS and every
//            source element is read from HBM once.  One barrier per tile (a tile is written once, nothing is overwritten).
//   streamed two staging tiles [2][64][33]: tile ct + 2 overwrites tile ct only after the barrier wave 0 reaches when it has summed
//            tile ct.  The outputs re-read the rows from HBM: twice in all.
// Outputs: the 64 rows of a target are one contiguous piece of its dense array, written once, consecutive lanes consecutive doubles.
#pragma once
#include <hip/hip_runtime.h>

#define TRL_NT 256     // threads per block
#define TRL_ROWS 64    // rows per block: one per lane of the summing wave
#define TRL_CT 32      // columns per staged tile
#define TRL_TS 33      // doubles per row of a staged tile
#define TRL_MAX_T 8    // targets per launch
#define TRL_NORM_BYTES (TRL_ROWS * TRL_MAX_T * 8)
#define TRL_STREAM_LDS (TRL_NORM_BYTES + 2 * TRL_ROWS * TRL_TS * 8)
#define TRL_LDS_MAX (160 * 1024)
#define TRL_CACHED_FIT 288  // longest row (columns) the CACHED form can keep: 64 rows of 32 * 9 + 1 doubles beside the norms fit TRL_LDS_MAX
#define TRL_CACHED_MAX 128  // ... and the longest it keeps by default: two blocks per CU.  Beyond, one block of four waves per CU with one
                            // summing wave loses to the streamed form's four blocks by 1.36 - 1.56 x, measured
#define TRL_MAX_DEV 64      // devices whose LDS limit is remembered as raised

struct TrlArgs {
    double *y[TRL_MAX_T];  // [n][len[t]], dense
    int len[TRL_MAX_T];
    int norm[TRL_MAX_T];   // 1 = normalise (the three modes are resolved on the host)
    int nt, maxlen;
};

// LDS bytes of the CACHED form for rows of L = max(lens) columns
static inline size_t trl_cached_lds(int L) {
    const size_t nct = ((size_t)L + TRL_CT - 1) / TRL_CT;
    return TRL_NORM_BYTES + (size_t)TRL_ROWS * (nct * TRL_CT + 1) * 8;
}

template <bool CACHED, bool VEC>
__global__ __launch_bounds__(TRL_NT) void k_truncate_l2(const double *__restrict__ X, long long n, long long ld, TrlArgs a) {
    extern __shared__ double trl_lds[];
    double *nrm = trl_lds;                          // [64][8] norms of the normalised targets
    double *tile = trl_lds + TRL_ROWS * TRL_MAX_T;  // CACHED: [64][S]; else [2][64][33]
    const int tid = threadIdx.x;
    const int L = a.maxlen;
    const int nct = (L + TRL_CT - 1) / TRL_CT;
    const int S = CACHED ? nct * TRL_CT + 1 : TRL_TS;
    const long long row0 = (long long)blockIdx.x * TRL_ROWS;
    const int rows = (int)(n - row0 < TRL_ROWS ? n - row0 : TRL_ROWS);
    const int lr = tid >> 4, lc = 2 * (tid & 15);  // this thread's row (+ 16 i) and column pair within a tile

    double v[4][2];
    auto load_tile = [&](int ct) {
        const int c = ct * TRL_CT + lc;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = lr + 16 * i;
            v[i][0] = 0.0;
            v[i][1] = 0.0;
            if (r < rows && c < L) {  // (columns from L on are never read)
                const double *p = X + (size_t)(row0 + r) * (size_t)ld + c;
                if (VEC && c + 1 < L) {
                    const double2 t = *reinterpret_cast<const double2 *>(p);
                    v[i][0] = t.x;
                    v[i][1] = t.y;
                } else {
                    v[i][0] = p[0];
                    if (c + 1 < L) v[i][1] = p[1];
                }
            }
        }
    };

    // the chain of row `tid` (wave 0 only) and the next column count at which a normalised target ends
    double s = 0.0;
    int nextb = 0x7fffffff;
    for (int t = 0; t < a.nt; t++)
        if (a.norm[t] && a.len[t] < nextb) nextb = a.len[t];

    load_tile(0);
    for (int ct = 0; ct < nct; ct++) {
        double *dst = CACHED ? tile + ct * TRL_CT : tile + (ct & 1) * (TRL_ROWS * TRL_TS);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            dst[(lr + 16 * i) * S + lc] = v[i][0];
            dst[(lr + 16 * i) * S + lc + 1] = v[i][1];
        }
        if (ct + 1 < nct) load_tile(ct + 1);  // in flight while wave 0 sums tile ct
        __syncthreads();
        if (tid < TRL_ROWS) {
            const double *src = dst + tid * S;
            const int c0 = ct * TRL_CT;
            const int jn = L - c0 < TRL_CT ? L - c0 : TRL_CT;
            for (int j = 0; j < jn; j++) {
                const double x = src[j];
                const double p = x * x;  // rounded before the add
                s = s + p;
                if (c0 + j + 1 == nextb) {  // (uniform)
                    const double nv = sqrt(s);
                    int nb2 = 0x7fffffff;
                    for (int t = 0; t < a.nt; t++) {
                        if (!a.norm[t]) continue;
                        if (a.len[t] == nextb) nrm[tid * TRL_MAX_T + t] = nv;
                        else if (a.len[t] > nextb && a.len[t] < nb2) nb2 = a.len[t];
                    }
                    nextb = nb2;
                }
            }
        }
    }
    __syncthreads();

    // the outputs: target t's rows row0 .. row0 + rows - 1 are rows * T consecutive doubles
    for (int t = 0; t < a.nt; t++) {
        const unsigned T = (unsigned)a.len[t];
        const unsigned total = (unsigned)rows * T;
        const bool nz = a.norm[t] != 0;
        double *Y = a.y[t] + (size_t)row0 * T;
        for (unsigned e = tid; e < total; e += TRL_NT) {
            const unsigned r = e / T, c = e - r * T;
            double x = CACHED ? tile[r * S + c] : X[(size_t)(row0 + r) * (size_t)ld + c];
            if (nz) {
                const double nv = nrm[r * TRL_MAX_T + t];
                x = nv == 0.0 ? 1.0 : x / nv;
            }
            Y[e] = x;
        }
    }
}
