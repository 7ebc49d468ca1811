/*
 * mmidx.h -- C ABI of the MI355X-native PQ / IVFPQ search engine (libmmidx_hip.so).
 *
 * This is the drop-in boundary for the search path of MKLab-ITI/multimedia-indexing
 * (gr.iti.mklab.visual.datastructures.{PQ,IVFPQ}).  The reference is pure Java and has no FFI
 * layer; its seam is the Template-Method contract of AbstractSearchStructure (5 protected hooks,
 * AbstractSearchStructure.java:267,305,342,729,755).  Each entry point below states the
 * reference method(s) whose body it replaces.  Citations are relative to the reference root,
 * J/ = src/main/java/gr/iti/mklab/visual/.  INTEGRATION.md shows the JNI stub and the Java
 * subclasses (GpuIVFPQ / GpuPQ) that bind these symbols.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types.  Every call returns an int status
 *     (MMIDX_OK == 0); mmidx_last_error() returns the message for the calling thread.  Status
 *     codes map 1:1 onto the reference's exceptions (see the enum).  Native code never exits.
 *   - vectors are row-major IEEE binary64, exactly the Java double[] contents.
 *   - PQ codes cross the boundary in the reference's stored form: for numProductCentroids <= 256
 *     one int8 per sub-quantizer holding (index - 128) (PQ.transformToByte, J/datastructures/
 *     PQ.java:552-558); otherwise one int16 per sub-quantizer holding the index
 *     (PQ.transformToShort, PQ.java:544-550).
 *   - internal ids (iid) are int32, as in the reference (loadCounter, ASS:65).
 *   - "_device" variants take pointers into the HBM of the handle's GPU and run asynchronously on
 *     the given hipStream_t (passed as void*; NULL = the HIP default stream, which is also what
 *     PyTorch's default stream is).  Host variants stage through HBM on a private stream and
 *     are synchronous.
 *   - threading: adds are serialised per handle (indexVector / indexPQCode are `synchronized`,
 *     ASS:229, IVFPQ.java:357); searches may run concurrently with each other but not with adds
 *     (the reference offers no reader/writer exclusion either).
 *   - arithmetic: all distances are fp64, accumulated in the reference's left-to-right order
 *     without FMA contraction; returned ids are bit-exact w.r.t. the reference restatement and
 *     distances are bit-equal (tolerance promised to callers: 1e-5).
 */
#ifndef MMIDX_H
#define MMIDX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMIDX_ABI_VERSION 8

typedef struct mmidx_index mmidx_index; /* opaque handle: one index on one GPU */

enum mmidx_status {
    MMIDX_OK = 0,
    MMIDX_ERR_INVALID_SUBVECTORS = 1, /* "The given number of subvectors is not valid!"  IVFPQ.java:181-183, PQ.java:148-150 */
    MMIDX_ERR_WRONG_DIM = 2,          /* "The dimensionality of the vector is wrong!"    IVFPQ.java:310-312, PQ.java:233-235 */
    MMIDX_ERR_NOT_IN_MEMORY = 3,      /* "Cannot execute query because the index is not loaded in memory!" ASS:282-284 */
    MMIDX_ERR_BYTE_OVERFLOW = 4,      /* "Byte is not sufficient to enumerate the centroids of the product quantizer!" IVFPQ.java:358-361 */
    MMIDX_ERR_CAPACITY = 5,           /* "Maximum index capacity reached..." (return false) ASS:232-235 */
    MMIDX_ERR_INVALID_ARG = 6,        /* null pointer, k < 1 (LingPipe queue ctor), w outside 1..C (NPE at IVFPQ.java:597-599) */
    MMIDX_ERR_NOT_READY = 7,          /* quantizers not loaded (NullPointerException in the reference) */
    MMIDX_ERR_NO_DEVICE = 8,          /* no usable MI355X / HIP runtime: the product path has NO CPU fallback */
    MMIDX_ERR_HIP = 9,                /* HIP runtime error; message carries hipGetErrorString */
    MMIDX_ERR_UNSUPPORTED = 10,       /* configuration outside the kernel envelope (see DESIGN.md limits) */
    MMIDX_ERR_NOT_CONVERGED = 11      /* mmidx_pca_learn_compute: max_iter reached above tol; the message carries the residual */
};

enum mmidx_kind { MMIDX_KIND_PQ = 1, MMIDX_KIND_IVFPQ = 2 };
/* PQ.TransformationType ordinals, J/datastructures/PQ.java:78-80 */
enum mmidx_transform { MMIDX_TR_NONE = 0, MMIDX_TR_ROTATION = 1, MMIDX_TR_PERMUTATION = 2 };

const char *mmidx_last_error(void);
int mmidx_abi_version(void);
/* number of visible HIP devices (0 when there is no GPU / runtime) */
int mmidx_device_count(void);

/* ---- lifecycle ------------------------------------------------------------------------------
 * Replaces the in-memory half of the constructors IVFPQ.java:174-237 / PQ.java:142-174 (the
 * BDB half stays in Java).  D = vectorLength, m = numSubVectors, ks = numProductCentroids,
 * C = numCoarseCentroids (ignored for PQ).  transform PERMUTATION: perm = D int32 indices
 * (RandomPermutation, J/utilities/RandomPermutation.java:29-56; pass NULL to have the library
 * derive RandomPermutation(seed = 1, D) with the JDK LCG, IVFPQ.java:136,193).  transform
 * ROTATION: rot = D*D row-major doubles computed by the Java side with EJML
 * (J/utilities/RandomRotation.java:30-35; the EJML stream cannot be re-derived natively).
 * Default w = (int)(0.1 * C), IVFPQ.java:188. */
int mmidx_create(int kind, int D, int m, int ks, int C, int transform, const int32_t *perm,
                 const double *rot, int device, mmidx_index **out);
int mmidx_destroy(mmidx_index *h); /* closeInternal, IVFPQ.java:888-890 */

/* loadCoarseQuantizer IVFPQ.java:297-300 : coarse[C][D] */
int mmidx_set_coarse(mmidx_index *h, const double *coarse);
/* loadProductQuantizer IVFPQ.java:275-288 / PQ.java:210-223 : pq[m][ks][D/m], file order */
int mmidx_set_pq(mmidx_index *h, const double *pq);
/* setW IVFPQ.java:95-97 */
int mmidx_set_w(mmidx_index *h, int w);
int mmidx_get_w(const mmidx_index *h, int *w_out);
/* loadCounter (ASS:65): number of indexed codes */
int mmidx_size(const mmidx_index *h, int64_t *n_out);
/* outputItemsPerList IVFPQ.java:654-673 : sizes[C] (sizes[1] for PQ) */
int mmidx_list_sizes(mmidx_index *h, int32_t *sizes_out);

/* ---- indexing -------------------------------------------------------------------------------
 * mmidx_encode: the arithmetic of indexVectorInternal, IVFPQ.java:309-335 (+computeNearest-
 * CoarseIndex :547-564, computeResidualVector :642-648, computeNearestProductIndex :613-631) /
 * PQ.java:232-252, for n vectors X[n][D], WITHOUT appending.  cell_out[n] (-1 for PQ),
 * code_out[n][m] in stored form (int8 or int16, see above).  Lets the Java side persist the
 * record to BDB exactly as appendPersistentIndex does (IVFPQ.java:760-792). */
int mmidx_encode(mmidx_index *h, int64_t n, const double *X, int32_t *cell_out, void *code_out);
/* mmidx_add_vectors: indexVectorInternal for a batch: encode + append with the given iids
 * (iids == NULL: iid = current size + i, i.e. loadCounter semantics ASS:244-251).  cell_out /
 * code_out may be NULL. */
int mmidx_add_vectors(mmidx_index *h, int64_t n, const double *X, const int32_t *iids,
                      int32_t *cell_out, void *code_out);
/* mmidx_add_codes: append precomputed records -- serves indexPQCode (IVFPQ.java:357-386) and
 * loadIndexInMemory (IVFPQ.java:680-728, PQ.java:436-483).  cells may be NULL for PQ. */
int mmidx_add_codes(mmidx_index *h, int64_t n, const int32_t *iids, const int32_t *cells,
                    const void *codes);
/* device-resident bulk variants (X, iids, cells, codes in HBM). */
int mmidx_add_vectors_device(mmidx_index *h, int64_t n, const double *dX, const int32_t *d_iids,
                             int32_t iid0, void *stream);
int mmidx_add_codes_device(mmidx_index *h, int64_t n, const int32_t *d_iids,
                           const int32_t *d_cells, const void *d_codes, void *stream);
int mmidx_encode_device(mmidx_index *h, int64_t n, const double *dX, int32_t *d_cell_out,
                        void *d_code_out, void *stream);
/* build the device-side inverted-list layout now (otherwise done lazily by the next search) */
int mmidx_sync_index(mmidx_index *h);
/* snapshot of the in-memory index in list-major order -- the arrays loadIndexInMemory builds
 * (invertedLists / pqByteCodes, IVFPQ.java:680-728; the per-id getters getPQCodeByte :801,
 * getInvertedListId :865 read the same records from BDB): list_off_out[nlists+1],
 * iids_out[n], codes_out[n][m] in stored form.  iids_out / codes_out may be NULL. */
int mmidx_export(mmidx_index *h, int64_t *list_off_out, int32_t *iids_out, void *codes_out);
/* native flat snapshot for fast restart alongside BDB (ABI 8).  mmidx_save writes what mmidx_export returns -- header
 * (magic "MMIDXSN1", version, kind, D, m, ks, C, code width, transform, n), list_off[nlists + 1], iids[n], codes[n][m] in stored
 * form, little-endian -- to `path` (through path.tmp + rename).  mmidx_load fills an EMPTY handle of the same shape (quantizers set
 * as after the constructor) from such a file: the work of loadIndexInMemory (IVFPQ.java:680-728, PQ.java:436-483) without the
 * BDB cursor; every list keeps its arrival order.  A shape mismatch, a damaged file or a non-empty index is MMIDX_ERR_INVALID_ARG.
 * Ids (String <-> iid) stay where they are: in the Java side's BDB. */
int mmidx_save(mmidx_index *h, const char *path);
int mmidx_load(mmidx_index *h, const char *path);

/* ---- per-id utilities of IVFPQ / PQ ----------------------------------------------------------------
 * mmidx_get_dims: the constructor arguments of the handle (vectorLength, numSubVectors, numProductCentroids,
 *   numCoarseCentroids) and the bytes per stored code entry (1: byte codes, 2: short codes); any pointer may be NULL.
 *   (Lets a binding check array lengths before it hands them over.)
 * mmidx_get_codes: getInvertedListId (IVFPQ.java:865-880) and getPQCodeByte / getPQCodeShort (:801-855) for n internal
 *   ids: cell_out[n] (-1 for PQ) and code_out[n][m] in stored form (int8 or int16).  An id that was never indexed fails
 *   with MMIDX_ERR_INVALID_ARG, message "Id does not exist!" (IVFPQ.java:803-805).  Either output may be NULL.
 * mmidx_distance: computeDistanceIVFADC(double[] qVector, String existingVecId), IVFPQ.java:464-497, for n (query, id) pairs:
 *   residual of Q[i] w.r.t. the cell of iids[i] (:470), the handle's transformation (:473-477), then the sum over the
 *   sub-quantizers of the lookup-table entries the stored code selects (:482-495), in the reference's order -- bit-equal to
 *   the distance a search reports for that candidate.  For a PQ handle the query itself takes the place of the residual. */
int mmidx_get_dims(const mmidx_index *h, int *D, int *m, int *ks, int *C, int *code_bytes);
int mmidx_get_codes(mmidx_index *h, int64_t n, const int32_t *iids, int32_t *cell_out, void *code_out);
int mmidx_distance(mmidx_index *h, int64_t n, const double *Q, const int32_t *iids, double *dist_out);

/* ---- search ---------------------------------------------------------------------------------
 * computeNearestNeighborsInternal(k, double[]) : computeKnnIVFADC IVFPQ.java:408-450 /
 * computeKnnADC PQ.java:290-322, for nq queries Q[nq][D].  Row i of iid_out / dist_out holds
 * count_out[i] = min(k, #candidates) results, best first: ascending squared distance, equal
 * distances in the bounded queue's order (ASS.lookUp, ASS:345-358).  Unused tail entries are
 * iid -1 / +inf.  k must be in 1..4095 (the reference's queue has no bound, IVFPQ.java:409; here the per-block
 * candidate buffers share the 160 KiB LDS with the lookup table: larger k -> MMIDX_ERR_INVALID_ARG).
 * mmidx_search may be called from any number of threads (computeNearestNeighbors is not synchronized,
 * ASS:281-291): callers that arrive while a batch is running are served together as one device batch
 * (same k), each with the answer of its own call. */
int mmidx_search(mmidx_index *h, int k, int64_t nq, const double *Q, int32_t *iid_out,
                 double *dist_out, int32_t *count_out);
int mmidx_search_device(mmidx_index *h, int k, int64_t nq, const double *dQ, int32_t *d_iid_out,
                        double *d_dist_out, int32_t *d_count_out, void *stream);
/* computeNearestNeighborsInternal(k, int iid) of PQ: computeKnnSDC, PQ.java:334-374 -- the query is
 * the stored code of the vector with internal id iids[i]; distances are code-to-code (one sequential
 * chain over all D dimensions).  PQ with byte codes only: IVFPQ.computeKnnIVFSDC returns null in the
 * reference (IVFPQ.java:509-511) -> MMIDX_ERR_UNSUPPORTED. */
int mmidx_search_sdc(mmidx_index *h, int k, int64_t nq, const int32_t *iids, int32_t *iid_out,
                     double *dist_out, int32_t *count_out);

/* ---- queries by indexed id on IVFPQ and PQ, and the vectors behind the records ------------------------------
 * An extension of the reference, which has no id query on IVFPQ (computeKnnIVFSDC returns null) and no getVector on a
 * quantized index.  The stored record (list, code) of an internal id decodes to the vector the index holds for it:
 *   z[s * dsub + t] = pq[s][code[s]][t];   y = z, or y[perm[i]] = z[i] (RandomPermutation), or
 *   y[i] = sum_j z[j] * R[i][j] (RandomRotation, R orthogonal: fp64 from 0.0, j ascending, every product rounded before its add);
 *   x = coarse[list] - y for IVFPQ (the residual is centroid - vector, IVFPQ.java:645), x = y for PQ.
 * mmidx_reconstruct: X_out[n][D] for n internal ids, host arrays.  An unknown or negative id fails the call with
 *   MMIDX_ERR_INVALID_ARG, message "Id does not exist!" (as mmidx_get_codes); X_out is then not written.
 * mmidx_reconstruct_device: the same on device pointers, asynchronous on `stream`.  d_found_out[n] (may be NULL) is 1 for a
 *   stored id and 0 for an unknown one, whose row is zeros.
 * mmidx_search_ids: computeKnnIVFADC(k, x) (IVFPQ) / computeKnnADC(k, x) (PQ) with x the decoded vector of iids[i], on the search
 *   path the handle would take for any vector; outputs as mmidx_search.  The query's own record is among the answers (as in
 *   PQ.computeKnnSDC); its distance is rounding residue, not necessarily 0.  Every id is checked before any output is written:
 *   an unknown id -> MMIDX_ERR_INVALID_ARG, "Id does not exist!".  The decoded vectors never visit the host.
 * mmidx_search_ids_device: as mmidx_search_device.  The row of an unknown id comes back with count -1, ids -1 and distances
 *   +inf; the other rows are unaffected.
 * All four: IVFPQ and PQ handles, byte and short codes, every transformation, k as for mmidx_search; the quantizers must be
 * loaded (MMIDX_ERR_NOT_READY); a sharded handle answers MMIDX_ERR_UNSUPPORTED. */
int mmidx_reconstruct(mmidx_index *h, int64_t n, const int32_t *iids, double *X_out);
int mmidx_reconstruct_device(mmidx_index *h, int64_t n, const int32_t *d_iids, double *dX_out, int32_t *d_found_out, void *stream);
int mmidx_search_ids(mmidx_index *h, int k, int64_t nq, const int32_t *iids, int32_t *iid_out, double *dist_out,
                     int32_t *count_out);
int mmidx_search_ids_device(mmidx_index *h, int k, int64_t nq, const int32_t *d_iids, int32_t *d_iid_out,
                            double *d_dist_out, int32_t *d_count_out, void *stream);

/* ---- removing records ---------------------------------------------------------------------
 * An extension of the reference, which can only index: a record leaves its collection there by a rebuilt BDB environment.
 * mmidx_remove takes n internal ids (host array) and removes every stored record that carries one of them:
 *   - pending records are folded into the lists first, so a record appended a moment ago can be removed;
 *   - mmidx_add_codes does not forbid two records with one iid: all of them go; an iid given twice in the request is one removal;
 *   - found_out[n] (may be NULL): 1 where iids[i] was stored before the call, else 0 -- every occurrence of a repeated iid gets
 *     the same answer.  A negative id, one beyond the largest stored id or one that is simply absent is no error: found 0;
 *   - removed_out (may be NULL) counts records, not request entries;
 *   - n == 0 is MMIDX_OK and touches nothing; so does a request none of whose ids is stored (no array moves);
 *   - the survivors keep their list and their arrival order inside it (the order equal distances are resolved in): afterwards
 *     the index is, array for array as mmidx_export returns them (list_off, ids, codes), the index that would exist had the
 *     removed records never been added;
 *   - all or nothing: the new arrays are built beside the old ones and swapped in at the end, so a failure before the swap
 *     leaves the index as it was.  Peak extra device memory: one copy of the survivors' codes and ids, plus one bit per id of the
 *     id space, one bit per record and a counter per 2048 records;
 *   - mmidx_size, mmidx_list_sizes, mmidx_export and mmidx_save report the smaller index; a later mmidx_add_* may use a removed
 *     iid again.  The per-code norms of the matrix-core pass B and the iid -> position table are rebuilt on their next use.
 * mmidx_remove_device: the ids (and d_found_out) are device pointers.  The call orders itself after `stream`, runs on the
 *   handle's own stream and SYNCHRONISES before it returns (the host copy of the list offsets must be current): d_found_out is
 *   complete on return, removed_out is a host pointer.
 * Both take the handle as an add that rebuilds the lists does (one at a time, never under a search of another thread or stream);
 * IVFPQ and PQ handles, byte and short codes.  A sharded handle answers MMIDX_ERR_UNSUPPORTED before anything is launched. */
int mmidx_remove(mmidx_index *h, int64_t n, const int32_t *iids, int32_t *found_out, int64_t *removed_out);
int mmidx_remove_device(mmidx_index *h, int64_t n, const int32_t *d_iids, int32_t *d_found_out, int64_t *removed_out, void *stream);

/* computeNearestCoarseIndex (IVFPQ.java:547-564) for n device-resident vectors: d_cell_out[i] = the exact
 * fp64 argmin cell, first index wins ties.  Needs only the coarse quantizer (used by the codebook learner). */
int mmidx_assign_device(mmidx_index *h, int64_t n, const double *dX, int32_t *d_cell_out, void *stream);

/* ---- sharded search, building blocks (one process per GPU over torch.distributed / MPI; the single-process form is
 * mmidx_create_sharded below, which drives these same phases itself) ---------------------
 * mmidx_coarse_device: computeNearestCoarseIndices IVFPQ.java:575-601 for nq queries ->
 *   d_cells_out[nq][w] (nearest first) and, when d_cdist_out is not NULL, the exact squared distance
 *   of every selected cell, d_cdist_out[nq][w] (what pass B's coarse bound needs: ranks that did not
 *   run the coarse stage for a query receive it with the all-gather of the cells).
 * mmidx_search_partial_device: scan of this shard's lists for the given probe cells; writes the
 *   shard's best k+1 candidates per query, sorted: d_pdist[nq][k+1] (fp64), d_pkey[nq][k+1]
 *   (int64 = probe_rank << 32 | iid -- the reference's offer order), d_pcount[nq].
 * mmidx_merge_partials_device: merges nshards partial lists into final results; no index handle
 *   needed.  Layout: dense [nshards][nq][k+1] (d_poff NULL), or ragged -- only the d_pcount[s][q] valid
 *   entries of every list, concatenated, list (s, q) starting at element d_poff[s * nq + q] (what a
 *   variable-size all-to-all delivers). */
int mmidx_coarse_device(mmidx_index *h, int64_t nq, const double *dQ, int32_t *d_cells_out,
                        double *d_cdist_out, void *stream);
int mmidx_search_partial_device(mmidx_index *h, int k, int64_t nq, const double *dQ,
                                const int32_t *d_cells, double *d_pdist, int64_t *d_pkey,
                                int32_t *d_pcount, void *stream);
/* Two-phase form of the partial search, so that shards can share their thresholds:
 *   pass A scans probe rank 0 of every query on this shard and exports the shard's threshold per
 *   query (the (k+1)-th best distance so far as a double, +inf when there are fewer candidates);
 *   the host MIN-all-reduces that array over ranks; pass B imports it, drops every probe whose
 *   coarse bound exceeds it, scans the rest and writes the sorted partial lists.  pass B must follow
 *   pass A on the same handle with the same (k, nq, dQ, d_cells).  d_cdist (may be NULL: the bound
 *   is then evaluated from the centroids) = the distances mmidx_coarse_device delivered. */
int mmidx_shard_pass_a_device(mmidx_index *h, int k, int64_t nq, const double *dQ,
                              const int32_t *d_cells, double *d_T_out, void *stream);
int mmidx_shard_pass_b_device(mmidx_index *h, int k, int64_t nq, const double *dQ,
                              const int32_t *d_cells, const double *d_cdist, const double *d_T_in,
                              double *d_pdist, int64_t *d_pkey, int32_t *d_pcount, void *stream);
/* dense partial lists [nq][k+1] -> ragged (list q = its d_pcount[q] valid entries at element d_poff[q]):
 * what a rank sends through the variable-size all-to-all */
int mmidx_compact_partials_device(int device, int k, int64_t nq, const double *d_pdist,
                                  const int64_t *d_pkey, const int32_t *d_pcount, const int64_t *d_poff,
                                  double *d_out_dist, int64_t *d_out_key, void *stream);
int mmidx_merge_partials_device(int device, int k, int64_t nq, int nshards, const double *d_pdist,
                                const int64_t *d_pkey, const int32_t *d_pcount, const int64_t *d_poff,
                                int32_t *d_iid_out, double *d_dist_out, int32_t *d_count_out,
                                int32_t *d_flag_out, void *stream);
/* Straddling ties across shards (ABI version 4).  mmidx_merge_partials_device sets d_flag_out[q] = 1 (d_flag_out may be NULL)
 * when the k-th and (k+1)-th merged distances are equal: which of the equal candidates the reference's single bounded queue
 * (IVFPQ.java:409, :445) keeps depends on the offer order over ALL probed lists, which no rank sees alone.  The owner collects
 * the flagged queries (d_fq[nf] = query index into dQ / d_cells, -1 = unused slot; d_tau[nf] = the k-th distance) and every
 * rank runs three passes over its own lists with a reduction over ranks in between:
 *   phase 0  d_counts[nf][w][2] (zeroed by the caller) <- per local list: offers with d <= tau, offers with d == tau;  SUM all-reduce
 *   phase 1  d_pB[nf] (zeroed) <- ties among the first offers of the list that holds the k-th "d <= tau" offer;          SUM all-reduce
 *   phase 2  d_tie_iids[nf][k] (filled with -1) <- iids of this rank's kept ties at their answer slots;                 MAX all-reduce
 * after which the owner overwrites answer slot s of a flagged query with d_tie_iids[f][s] wherever that is >= 0.  The result is
 * the single queue's (the same closed form k_tie_resolve applies on one GPU).  Within a list, entries are replayed in list
 * position = arrival order, as the reference appends them. */
int mmidx_shard_tie_phase_device(mmidx_index *h, int phase, int k, int64_t nf, const double *dQ, const int32_t *d_cells,
                                 const int32_t *d_fq, const double *d_tau, int32_t *d_counts, int32_t *d_pB,
                                 int32_t *d_tie_iids, void *stream);

/* ---- one index over several GPUs, ONE process (ABI version 5) --------------------------------------------------------------
 * The reference's caller is a single JVM that holds the whole index and queries it through one object
 * (YFCC100MExample.java:93-99, :155; Example.java:96-110).  mmidx_create_sharded makes that object span n_dev GPUs of one node:
 * whole inverted lists are partitioned (list c lives on shard c mod n_dev -- invertedLists[c] / pqByteCodes[c], IVFPQ.java:72-83,
 * stay intact, so the offer order inside a list is the reference's), the codebooks are replicated, and every entry point that
 * takes host pointers works on the returned handle exactly as on a plain one:
 *   mmidx_set_coarse / mmidx_set_pq / mmidx_set_w / mmidx_set_option / mmidx_set_profiling   applied to every shard
 *   mmidx_encode / mmidx_add_vectors     the batch is encoded 1/n_dev per GPU, each record goes to the shard that owns its list
 *   mmidx_add_codes                      indexPQCode / loadIndexInMemory: records routed by list id
 *   mmidx_search                         computeKnnIVFADC over all shards (below); concurrent callers are combined as usual
 *   mmidx_size / mmidx_list_sizes / mmidx_export / mmidx_get_codes / mmidx_distance / mmidx_get_stats / mmidx_sync_index
 * Search, per round of queries: shard r owns 1/n_dev of the queries; RCCL all-gather of the query vectors and of the probe cells
 * (each shard runs the coarse stage for its own queries), pass A on every shard's local lists, RCCL all-reduce (MIN) of the
 * thresholds, pass B under the global thresholds, every sorted partial top-(k+1) list stored straight into its owner's buffers
 * over xGMI (peer access; option "shard_exchange" = 1: ncclSend / ncclRecv of the dense lists instead), merge at the owner,
 * cross-shard replay of the bounded queue for queries whose k-th and (k+1)-th distances tie (RCCL all-reduces).  Results are
 * those of a plain handle holding the same records: ids bit-exact, distances bit-equal, ties included.
 * devs[i] = HIP device of shard i.  Pairwise distinct devices (the production form, n_dev = 1 included) use RCCL
 * (ncclCommInitAll, one communicator per device, one host thread per device); a device listed more than once makes virtual
 * shards on it with in-process collectives (RCCL refuses duplicate devices): the functional test form on a one-GPU box.
 * The _device entry points of a plain handle take ONE device's pointers and are refused on a sharded handle
 * (MMIDX_ERR_UNSUPPORTED); the _sliced_device forms below are their counterparts: slice r lives in the HBM of shard r's device.
 *   mmidx_search_sliced_device   shard r hands in nq_per_shard queries dQ[r][nq_per_shard][D] and receives their answers in
 *                                d_iid_out[r] / d_dist_out[r] / d_count_out[r] (synchronous: the answers are complete on return)
 *   mmidx_add_vectors_sliced_device   the batch is the concatenation of the slices dX[r][n_per_shard[r]][D]; row i of it gets
 *                                iid0 + i (arrival order = batch order, as indexVector calls in that order would give)
 *   mmidx_shard_count / mmidx_shard_info   number of shards (1 for a plain handle); a shard's device, its number of records,
 *                                and whether the group's collectives run on RCCL */
int mmidx_create_sharded(int kind, int D, int m, int ks, int C, int transform, const int32_t *perm, const double *rot, int n_dev,
                         const int *devs, mmidx_index **out);
int mmidx_shard_count(const mmidx_index *h, int *n_out);
int mmidx_shard_info(const mmidx_index *h, int shard, int *device_out, int64_t *size_out, int *uses_rccl_out);
int mmidx_search_sliced_device(mmidx_index *h, int k, int64_t nq_per_shard, const double *const *dQ, int32_t *const *d_iid_out,
                               double *const *d_dist_out, int32_t *const *d_count_out);
int mmidx_add_vectors_sliced_device(mmidx_index *h, const int64_t *n_per_shard, const double *const *dX, int32_t iid0);

/* ---- Linear: exhaustive exact search (J/datastructures/Linear.java; BASELINE config 1) ------------------------
 * add = indexVectorInternal (:111-122), search = computeNearestNeighborsInternal(k, double[]) (:138-163): exact
 * sequential fp64 squared distances, bounded-queue order and ties, ids = insertion order; get_vector = getVector
 * (:253-263).  The vectors live in HBM in arrival order; an append moves and prepares the new rows only.  While
 * n <= 16384 and k + 1 <= 256 a search is the certified coarse stage of a hidden index handle whose "centroids" the
 * vectors are; beyond that it is the certified scan of csrc/mmidx_linear_scan.h: a matrix-core filter
 * with an error bound, exact fp64 for the survivors, and the exact path (fp64 distances to every row + the bounded
 * queue's selection) for the queries the scan hands back -- a tie between the k-th and (k + 1)-th distance, norms
 * outside the filter's range, a full survivor list.  Every path returns the reference's bits.
 *   mmidx_linear_add_device      indexVectorInternal (:111-122) for n rows already in the handle's HBM
 *   mmidx_linear_search_device   computeNearestNeighborsInternal(k, double[]) (:138-163) on device pointers: ids [nq][k]
 *                                (-1 beyond the count), distances [nq][k] (+inf beyond it), counts [nq]; asynchronous on
 *                                `stream` except for one read-back per call (the number of handed-back queries)
 *   mmidx_linear_search_ids      computeNearestNeighborsInternal(k, int iid) (:181-184): the stored vector is the query;
 *                                host arrays, the rows are gathered on the device
 *   mmidx_linear_copy_rows_device  rows iid0 .. iid0+n-1 into a device buffer (the walk of IndexTransformation.java:113-122)
 *   mmidx_linear_set_option      switches for measurements and tests; none changes a result.  An unknown name is
 *                                MMIDX_ERR_INVALID_ARG.
 *        "exact" = 1       every search beyond the small path goes through the exact path
 *        "mfma_qcap" = n   capacity of the scan's survivor record list (0 = sized from the call)
 *        "debug_sync" = 1  stage times in the stats (HIP events, one wait per segment)
 *   mmidx_linear_get_stats       figures of the last search (and of the last add: uploaded_rows) */
typedef struct mmidx_linear mmidx_linear;
typedef struct mmidx_linear_stats {
    int32_t path;          /* what served the last search: 1 coarse stage (small index), 2 exact, 3 scan */
    int32_t segments;      /* sweep launches of the scan */
    int64_t rows_scanned;  /* rows the scan went over (seed included), summed over its rounds of queries */
    int64_t survivors;     /* (query, row) records verified exactly */
    int64_t redo_queries;  /* queries the scan handed back to the exact path */
    int64_t uploaded_rows; /* rows the last add moved and produced side data for */
    double scan_ms, verify_ms; /* sweep / verification + pool reduction, only with "debug_sync" */
} mmidx_linear_stats;
int mmidx_linear_create(int D, int64_t capacity, int device, mmidx_linear **out);
int mmidx_linear_destroy(mmidx_linear *l);
int mmidx_linear_add(mmidx_linear *l, int64_t n, const double *X);
int mmidx_linear_add_device(mmidx_linear *l, int64_t n, const double *dX, void *stream);
int mmidx_linear_size(const mmidx_linear *l, int64_t *n_out);
int mmidx_linear_get_dim(const mmidx_linear *l, int *D_out); /* vectorLength of the handle (bindings check array lengths against it) */
int mmidx_linear_get_vector(const mmidx_linear *l, int64_t iid, double *out);
int mmidx_linear_search(mmidx_linear *l, int k, int64_t nq, const double *Q, int32_t *iid_out, double *dist_out,
                        int32_t *count_out);
int mmidx_linear_search_device(mmidx_linear *l, int k, int64_t nq, const double *dQ, int32_t *d_iid_out,
                               double *d_dist_out, int32_t *d_count_out, void *stream);
/* computeNearestNeighborsInternal(k, int iid), Linear.java:181-184: the stored vector is the query */
int mmidx_linear_search_ids(mmidx_linear *l, int k, int64_t nq, const int32_t *iids, int32_t *iid_out,
                            double *dist_out, int32_t *count_out);
/* rows iid0 .. iid0+n-1 into a device buffer (the walk of IndexTransformation.java:113-122) */
int mmidx_linear_copy_rows_device(mmidx_linear *l, int64_t iid0, int64_t n, double *d_out, void *stream);
int mmidx_linear_set_option(mmidx_linear *l, const char *name, int value);
int mmidx_linear_get_stats(mmidx_linear *l, mmidx_linear_stats *out);

/* ---- exact re-ranking of a PQ / IVFPQ answer against a Linear handle ---------------------------------
 * An extension of the reference, whose deployment keeps both structures: IndexTransformation.java:61-125 walks a full-vector
 * Linear index into a PQ / IVFPQ one, and Example.java:155-182 compares their answers.  Identity contract: the record with
 * internal id i of the compressed handle h is row i of the Linear handle l, which is what that walk produces (:113-122).
 * refine(k, R, q), for nq queries:
 *   1. the candidates are exactly the answer of mmidx_search(h, R, q): at most R records, ascending code distance, the bounded
 *      queue's order among equal ones;
 *   2. a candidate whose internal id is outside [0, size(l)) is dropped and counted in `missing`; its row is never read;
 *   3. every other candidate gets d = sum_j (q[j] - x[j])^2 from row iid of l: fp64, j ascending, uncontracted (Linear.java:147-149);
 *   4. the pairs (iid, d) are offered in the candidates' order to a bounded queue of size k under ASS.lookUp's rule (ASS:345-358):
 *      a candidate equal to the worst kept is rejected, a better one evicts the earliest-inserted of the equal-worst.
 * Row i of iid_out / dist_out holds count_out[i] = min(k, candidates kept) results, nearest first by exact squared distance, the
 * later-offered first among equal distances; unused tail entries are iid -1 / +inf, as mmidx_search pads.  *missing_out (may be
 * NULL) is the number of dropped candidates summed over the call.  With R = size and w = C on tie-free data the answer is
 * mmidx_linear_search's, bit for bit.
 *   mmidx_search_refine          host arrays, synchronous, in rounds on the index handle's stream
 *   mmidx_search_refine_device   device pointers, asynchronous on `stream`; nothing is read back.  d_missing_out (may be NULL) is
 *                                one int64 in HBM, zeroed and then added to by the call.  The Linear handle orders the call
 *                                against its adds on other streams, as its own _device calls do.
 *   mmidx_search_refine_ids      computeNearestNeighbors(k, String id) in exact form (Linear.java:181-184): the query is row
 *                                iids[q] of l, gathered on the device, then refined like any other.  An id outside [0, size(l))
 *                                gives count 0 and a padded row, and adds nothing to `missing`.
 * Refused before any launch, the message naming the offending value: a null handle, k < 1, R < k, R > 4095 (the k of
 * mmidx_search), vector lengths of h and l that differ, handles on different devices -- MMIDX_ERR_INVALID_ARG; a sharded h --
 * MMIDX_ERR_UNSUPPORTED.  nq == 0 is MMIDX_OK and writes nothing but *missing_out = 0 (host forms).  An empty l is legal: every
 * candidate is missing and the counts are 0.  Locks: the index handle first, then the Linear handle. */
int mmidx_search_refine(mmidx_index *h, mmidx_linear *l, int k, int R, int64_t nq, const double *Q, int32_t *iid_out,
                        double *dist_out, int32_t *count_out, int64_t *missing_out);
int mmidx_search_refine_device(mmidx_index *h, mmidx_linear *l, int k, int R, int64_t nq, const double *dQ,
                               int32_t *d_iid_out, double *d_dist_out, int32_t *d_count_out, int64_t *d_missing_out,
                               void *stream);
int mmidx_search_refine_ids(mmidx_index *h, mmidx_linear *l, int k, int R, int64_t nq, const int32_t *iids, int32_t *iid_out,
                            double *dist_out, int32_t *count_out, int64_t *missing_out);

/* ---- re-indexing a Linear index: project, truncate, renormalise -------------------------------------------
 * The two drivers of the reference that turn one index into another, as one native walk: IndexTransformation.java:61-125 (a full
 * Linear index into a shorter Linear, a PQ or an IVFPQ one) and PCAProjectionExample.java:74-88 (project every row once, index
 * several truncations).  It produces what mmidx_search_refine's identity contract (above) asks for.
 *
 * mmidx_truncate_l2_device reads rows x_r = dX[r * ld .. r * ld + ncols), ld >= ncols.  lens, normalize and dY are HOST arrays of
 * nt entries (1 <= nt <= 8); dY[t] is a device pointer to [n][lens[t]], dense.  For every target t with T = lens[t], 1 <= T <= ncols:
 *   y = x_r[0..T);  normalize[t] = 0: never normalise; 1: always (PCAProjectionExample.java:83-85); 2: if and only if T < ncols
 *   (IndexTransformation.java:118-120).  Normalising is Normalization.normalizeL2 (Normalization.java:21-37) literally:
 *     s = 0; for i in 0..T-1: s += y[i] * y[i]   (fp64, the product rounded before the add, index order)
 *     norm = sqrt(s), correctly rounded;  norm == 0: every entry becomes 1.0;  otherwise y[i] = y[i] / norm (IEEE division).
 *   A target that is not normalised is a bit copy.  Columns from max(lens) on are never read.  No NaN inputs.
 * Asynchronous on `stream`; nothing is read back.  Refusals (MMIDX_ERR_INVALID_ARG, before any launch): nt outside 1..8, n < 0,
 * ncols < 1, ld < ncols, a null array, a length outside 1..ncols, a normalize value outside 0..2, a null dX / dY[t] with n > 0.
 *
 * mmidx_linear_reindex handles rows iid0 .. iid0 + n - 1 of src in chunks of chunk_rows rows (0 = 2^25 / W rows, W the widest row
 * the walk buffers: nc with a pca, else the longest target, the stored rows being read in place; i.e. 256 MiB of such rows, kept
 * within 4096 .. 2^20 and rounded down to a multiple of 64).  Without pca the chunk is the
 * stored rows (ncols = D_src), read in place; with pca it is mmidx_pca_project_device of them (ncols = nc, whitening included as
 * that call does it, PCA.java:199-204).  The chunk goes through mmidx_truncate_l2_device's kernel once for all targets, lens[t]
 * being the target handle's own vector length, and each output is appended to its target in row order:
 *   kinds[t] = 0   targets[t] is a mmidx_linear, appended as mmidx_linear_add_device does;
 *   kinds[t] = 1   targets[t] is a mmidx_index (PQ or IVFPQ, any transformation), appended as mmidx_add_vectors_device does with
 *                  the internal ids iid0 + i.
 * Synchronous: on return every target is complete.  Nothing leaves HBM.
 * Identity is checked, not assumed: every target must hold exactly iid0 records / rows when the call starts, so that record i of
 * every target is row i of src.  An index that has grown is brought up to date by a second call with iid0 = the old size.
 * Refusals, all before any launch, the message naming the offending value, no target changed:
 *   MMIDX_ERR_INVALID_ARG   a null src, targets or targets[t]; nt outside 1..8; a kinds[t] outside 0..1 or normalize[t] outside
 *                           0..2; n < 0; chunk_rows < 0; iid0 < 0 (all of these before any handle is looked into); the same handle
 *                           twice, or src among the targets; iid0 + n > size(src); a target longer than ncols; a pca whose sample
 *                           size is not D_src; a target whose size is not iid0; a target whose remaining capacity is below n;
 *                           handles on different devices
 *   MMIDX_ERR_NOT_READY     an index target without its codebooks
 *   MMIDX_ERR_UNSUPPORTED   a sharded target
 * n == 0 is MMIDX_OK after the checks.  A HIP failure in the middle of the walk can leave targets of different sizes; their sizes
 * say which chunks arrived.  Locks, held for the whole call: every index target first (its add lock, then its search lock, as
 * mmidx_add_vectors_device takes them), then the Linear handles, src and the Linear targets alike; within each class in ascending
 * address order, so that the argument order of two concurrent walks does not matter.  This is mmidx_search_refine's order (index
 * handle first, then the Linear handle): a refine over a pair that a walk is filling runs before or after the walk, never across
 * it.  Searches and adds on any handle of the walk wait until it returns. */
int mmidx_truncate_l2_device(int device, int64_t n, int ncols, int64_t ld, const double *dX, int nt, const int32_t *lens,
                             const int32_t *normalize, double *const *dY, void *stream);
struct mmidx_pca; /* the PCA handle of the front end, below */
int mmidx_linear_reindex(mmidx_linear *src, int64_t iid0, int64_t n, struct mmidx_pca *pca, int nt, const int32_t *kinds,
                         void *const *targets, const int32_t *normalize, int64_t chunk_rows);

/* ---- codebook learning (J/visual/quantization/AbstractQuantizerLearning.java:39-81) ------
 * k-means on the GPU in place of Weka's SimpleKMeans, which the reference calls with setSeed(seed),
 * setNumClusters(k), setMaxIterations(max_iter) and, optionally, k-means++ seeding.  flags:
 *   MMIDX_KMEANS_PLUS_PLUS  k-means++ seeding (else SimpleKMeans' default random seeding, which skips a drawn
 *                           instance equal to a centre already taken: fewer than k centres when X has fewer
 *                           than k distinct rows),
 *   MMIDX_KMEANS_NORMALIZE  min-max attribute normalisation inside the distance (Weka's default).
 * init_centroids (host, [k][d], may be NULL) overrides the seeding.  Empty clusters are dropped as Weka does:
 * *k_out <= k centroids are written to centroids_out (host, room for [k][d]); assign_out[i] indexes them.
 * 1 <= k <= n < 2^31, else MMIDX_ERR_INVALID_ARG.
 * sse = squared error in the space the clustering ran in.  Weka is an absent third-party dependency: the
 * algorithm is restated, its random stream and summation order are not reproduced (parity unpinned). */
enum mmidx_kmeans_flags { MMIDX_KMEANS_PLUS_PLUS = 1, MMIDX_KMEANS_NORMALIZE = 2 };
int mmidx_kmeans_device(int device, int64_t n, int d, int k, int max_iter, int64_t seed, int flags,
                        const double *dX, const double *init_centroids, double *centroids_out,
                        int32_t *d_assign_out, double *sse_out, int32_t *iters_out, int32_t *k_out,
                        void *stream);
int mmidx_kmeans(int device, int64_t n, int d, int k, int max_iter, int64_t seed, int flags,
                 const double *X, const double *init_centroids, double *centroids_out,
                 int32_t *assign_out, double *sse_out, int32_t *iters_out, int32_t *k_out);

/* The whole product quantizer in one device-resident call (ProductQuantizationLearning.java:247-305):
 * residual w.r.t. the nearest coarse centroid (centroid - x; coarse = NULL, C = 0: flat PQ, no residual), the transformation (perm /
 * rot as for mmidx_create), then for each of the m sub-spaces k-means++ with the seeds 1..repeats, keeping the repeat of lowest
 * squared error (a later repeat replaces the kept one only on sse < best).  Each (sub-space, seed) pair runs the algorithm of
 * mmidx_kmeans with MMIDX_KMEANS_PLUS_PLUS, bit for bit the same centroids; all pairs share every kernel launch, and the host waits
 * at most once per Lloyd iteration.  flags accepts MMIDX_KMEANS_NORMALIZE only.
 * pq_out (host, [m][ks][dsub], the order of the product quantizer file): clusters that came out empty are rows of 1000.0
 * (:285-302).  sse_out / seed_out / k_out / iters_out ([m] each, may be NULL): squared error, seed, number of real centroids and
 * Lloyd iterations of the kept repeat.
 * Refusals, all before any device call, pq_out untouched: a null dX or pq_out, a non-positive size, ks > n, n >= 2^31, other flags,
 * a transformation without its perm / rot -> MMIDX_ERR_INVALID_ARG; D % m != 0 -> MMIDX_ERR_INVALID_SUBVECTORS.
 * Envelope: dsub = D / m <= 16 and ks * dsub * 8 <= 64 KiB (a job's table lives in LDS), else MMIDX_ERR_UNSUPPORTED: such callers
 * keep mmidx_kmeans per sub-space.  When all m * repeats pairs do not fit the memory (or 2^31 - 1 sort items) at once they run in
 * groups, which changes no bit of the result; the environment variable MMIDX_PQ_LEARN_GROUP caps the pairs per group (tests). */
int mmidx_pq_learn_device(int device, int64_t n, int D, int m, int ks, int max_iter, int repeats, int flags,
                          const double *dX, int C, const double *coarse, int transform, const int32_t *perm,
                          const double *rot, double *pq_out, double *sse_out, int32_t *seed_out, int32_t *k_out,
                          int32_t *iters_out, void *stream);
int mmidx_pq_learn(int device, int64_t n, int D, int m, int ks, int max_iter, int repeats, int flags,
                   const double *X, int C, const double *coarse, int transform, const int32_t *perm,
                   const double *rot, double *pq_out, double *sse_out, int32_t *seed_out, int32_t *k_out,
                   int32_t *iters_out);

/* ---- instrumentation -------------------------------------------------------------------------
 * Per-handle statistics accumulated over the search calls since the last mmidx_get_stats, measured
 * with HIP events recorded on the stream the kernels are launched on (no host synchronisation
 * until mmidx_get_stats).  scan_ms = time inside the list-scan kernel (the HBM-bound
 * kernel of the path), scan_codes = sum over (query, probed list) of list lengths (algorithmic
 * bytes = m * scan_codes), launches = number of scan launches. */
typedef struct mmidx_stats {
    double total_ms, coarse_ms, scan_ms, merge_ms;
    int64_t scan_codes;
    int32_t scan_launches;
    int32_t tie_fallbacks;
    /* pass A alone (the dominant kernel: the exact scan of every query's nearest list): time between the events around
     * its launches, the codes of the probe-rank-0 lists, the number of calls that ran it (ABI version 3) */
    double passa_ms;
    int64_t passa_codes;
    int32_t passa_launches;
    /* (query, probe) pairs of the most recent search call that survived the coarse bound and went through pass B
     * (-1: unknown); read from the pinned word the device writes for the launch-size hint */
    int32_t passb_items_last;
    /* codes of pass B that survived the lower-bound filter and had their exact distance computed (ABI version 4) */
    int64_t verified_codes;
    /* K3m, the matrix-core lower bound of pass B (csrc/mmidx_scan_mfma.h; ABI version 6): (query, code) pairs its bound could not
     * drop (each verified exactly: they are part of verified_codes), and queries it handed back to K3f (no finite threshold yet, a
     * full survivor list or pool) */
    int64_t mfma_survivors;
    int64_t mfma_redo_queries;
    /* ... and, with full profiling, the launch durations of its scan kernel (k_scan_mfma) and of the exact verification
     * (k_mfma_verify) from HIP events around them, summed over mfma_launches calls */
    double mfma_scan_ms, mfma_verify_ms;
    int32_t mfma_launches;
    int32_t reserved0;
    /* K3ma, pass A on the matrix cores (csrc/mmidx_scan_mfma_a.h; ABI version 7): calls whose pass A went through it, and with full
     * profiling the durations of its four stages (HIP events): sweep 1 (k_scan_mfma<.., 1>), threshold selection (k_a1_select),
     * sweep 2 (k_scan_mfma<.., 2>) and the exact verification (k_a1_verify), summed over those calls.  Its verified codes count in
     * verified_codes / mfma_survivors, the queries it handed to the exact kernels in mfma_redo_queries. */
    int64_t passa_mfma_launches;
    double passa_mfma_sweep1_ms, passa_mfma_select_ms, passa_mfma_sweep2_ms, passa_mfma_verify_ms;
} mmidx_stats;
/* enabled: 0 off; 1 full (six events per search call and the code counters: every field below); 2 light (only the two
 * events around pass A: passa_ms / passa_launches -- an event record is a ~5 us bubble in the stream, so a throughput
 * run carries as few as its roofline figure needs) */
int mmidx_set_profiling(mmidx_index *h, int enabled);
/* Runtime switches for measurements and tests, by name.  None of them changes a result (DESIGN.md section 5 describes the
 * devices they switch).  An unknown name is MMIDX_ERR_INVALID_ARG.  One line per name, the text of the table kOptions of
 * csrc/mmidx_api.hip; "(env MMIDX_X)" marks the ones mmidx_create also reads from the environment.
 *   "exhaustive": sets no_filter and no_bound together: every probed code is read and summed in fp64
 *   "no_filter": exact scan only, no lower-bound filter (from the environment it also sets no_bound) (env MMIDX_NO_FILTER)
 *   "no_bound": no coarse-bound pruning of probes (env MMIDX_NO_BOUND)
 *   "exact_coarse": coarse stage and assignment by fp64 distances to every centroid (K1a/K1b) (env MMIDX_EXACT_COARSE)
 *   "debug_sync": synchronise after every stage, report the first failing one and per-stage figures on stderr (env MMIDX_DEBUG_SYNC)
 *   "combine": concurrent mmidx_search callers are served together (default 1)
 *   "host_slots": large host-pointer requests: up to three callers in flight (default 1); 0 = one at a time through the combiner's queue
 *   "coarse_v1": coarse stage by K1c/K1d (fp32 MFMA, full distance matrix) instead of K1e/K1f (env MMIDX_COARSE_V1)
 *   "coarse_fused": K1f as one kernel (front end + selection)
 *   "coarse_dma_kc": K1e with LDS-DMA also for vectors of several k chunks, Dp a multiple of 128 (default 1)
 *   "coarse_groups": K1e for Dp = 128 as two staggered wave groups, a block of 256 queries per CU (default 1); 0 = the four-wave K1e' with two half-tile buffers
 *   "coarse_wave_sel": the coarse stage's exact selection by one wave per query where its tile applies (default 1); 0 = always a block per query
 *   "passa_q": pass A by K3q: 1 always (where the shape allows), 0 never, -1 = from 1.25 queries per non-empty list of a long-list index (default); K3q is tested before passa_hist, so passa_q = 0 is needed for passa_hist to take effect on long-list m = 16 indexes
 *   "passa_mfma": pass A by K3ma: 1 always (where the shape allows), 0 never, -1 = from 8 queries per list of a long-list index (default)
 *   "passa_mfma_wide": K3ma's small items through the eight-wave instance (default 1); 0 = the four-wave instance alone
 *   "passa_mfma_icnt_sat": where K3ma's record prefix saturates (0 = 0xFFFFFFFF); tests force the overflow path
 *   "passa_hist": pass A by K3h: 1 always, 0 never, -1 = lists of >= 4096 codes on average (default) (env MMIDX_PASSA_HIST)
 *   "passa_wide": K3h with 512-thread blocks (env MMIDX_PASSA_WIDE)
 *   "passa_item_min": fewest queries per call for a shard's pass A to launch over the queries with a non-empty nearest list only (default 4096)
 *   "passa_item_margin": blocks that launch takes beyond 1.15 x the expected count (default 1024; tests: 0)
 *   "smin_pre": K3s (k_pair_smin) in front of pass B's counting sort: 1 always, 0 never, -1 = by the device-reported figures of the call before (default)
 *   "smin_bf16": K3s's bf16 first stage for 16-dimensional sub-quantizers (default 1); 0 = fp32 only
 *   "smin_valu": K3s with packed VALU FMAs instead of the matrix cores
 *   "no_mfma": no matrix-core bounds: pass B through K3g / K3f instead of K3m, and no K3ma in pass A
 *   "no_grp": pass B through K3f (one block per query and list) instead of the grouped K3g
 *   "no_union": K3g without the per-query histogram that lowers thresholds from the union over lists; -1 = with it always
 *   "no_split_table": m = 128: the table-in-global-scratch kernels instead of k_scan_split
 *   "passb_small": pass B through K3f when the like call before kept at most 64 pairs (default 1)
 *   "passb_main_grid": > 0: fixed size of K3f's main launch (tests force the looping tail kernel)
 *   "mfma_sub": codes per K3m item (0 = sized from the call)
 *   "mfma_qcap": survivor records per K3m launch (0 = sized from the call); tests force the redo path
 *   "mfma_blocks": persistent blocks of K3m (0 = occupancy x CUs)
 *   "mfma_kc_v1": K3mk without LDS-DMA (k_scan_mfma_kc) also where k_scan_mfma_kc2 applies
 *   "mfma_kc_tpw": code tiles per wave of K3mk: 8 (default) or 16
 *   "flat_chunk": codes per chunk of a flat PQ list, from 4096 (0 = sized from the batch)
 *   "sub_batch": > 0: at most this many queries per sub-batch of a search call (0 = from the memory caps alone); tests split small calls
 *   "coarse_near": the coarse stage's one-probe certificate: -1 = wherever its conditions hold (default), 0 = off (every query gets its exact far ranking)
 *   "coarse_screen": the head-only bf16 screen in front of that certificate (K1s): -1 = where it applies, resting seven calls
 *        after one that handed on more than a quarter of its queries (default), 0 = off, 1 = wherever it applies
 * A sharded handle passes these on to every shard and has options of its own (csrc/mmidx_sharded.h):
 *   "shard_exchange": 0 = partial lists stored into the owners' buffers over xGMI, 1 = ncclSend / ncclRecv
 *   "tie_slots": flagged queries per owner and replay round (0 = no replay)
 *   "shard_max_round": queries per collective round
 *   "combine": as above, for the group's own combiner
 *   "shard_route_host": 1 = mmidx_add_vectors_sliced_device sends its records through the host instead of routing them between the devices
 *   "shard_pipeline": 1 = the query exchange on a second stream / communicator (the default for in-process shards; off by default on two or more physical devices) */
int mmidx_set_option(mmidx_index *h, const char *name, int value);
int mmidx_get_stats(mmidx_index *h, mmidx_stats *out);
/* Which kernel family served each stage of the most recent search sub-batch of this handle (ABI version 7), as text:
 * "coarse=<K1..>;pass_a=<K3 | K3h | K3ma | ..>;pre=<K3s | ->;pass_b=<K3m | K3mk | K3g | K3f.. | ->;coarse_mm=<groups | dma | dma_kc | staged | ->"
 * (coarse_mm: the form of K1e's matrix kernel, "-" where the coarse stage is not K1e; DESIGN.md section 5.0 lists the gates;
 * tests/test_gpu_dispatch.py asserts the table).  pass_a names the kernel launch_scan took: "K3(table in two halves)" only where
 * k_scan_split ran, "K3(table in global scratch)" for every other table beyond the LDS.  pass_b names the exact scan where the
 * filtered one fell back to it: "K3(exact scan: no K3f instance for this shape)", or "K3(exact scan: symmetric distances)" after
 * mmidx_search_sdc on an index of several chunks (tests/test_gpu_sdc.py).  Three fields follow them for the build path (the "build" table of section 5.0;
 * tests/test_gpu_build.py asserts it):
 *   ";assign=<K6a'(rows) | K6a'(copies) | K6a | exact | ->"   the kernel of the most recent assignment: K6a' fed from the fp64 rows,
 *        K6a' fed from k_split_bf16's copies, the fp32 K6a, the exact kernel alone; "-" for a flat PQ or before any assignment
 *   ";encode=<K6b' | K6b | ->"   the product quantisation kernel of the most recent encode
 *   ";flagged=<count | ->"   vectors that the most recent mmidx_encode / _add_vectors / _assign_device / _encode_device /
 *        _add_vectors_device call sent to the exact redo, summed over its internal chunks; "-" where no certified kernel ran in it
 *   ";screened=<count | ->"   queries of that search sub-batch the screen's certificate served (option "coarse_screen"; the others went on to
 *        the split kernels); "-" where the screen did not run; read from the device by this call
 *   ";near_only=<count>"   queries of that search sub-batch the coarse stage answered with the nearest cell alone (the one-probe
 *        certificate; option "coarse_near"); read from the device by this call
 * A sharded handle reports its first shard.  Diagnostic: not a stable format. */
int mmidx_get_dispatch(mmidx_index *h, char *out, int cap);

/* Measured ceilings for the rooflines bench.py reports (csrc/mmidx_probe.hip; SURVEY 8d "secondary: LDS gather rate", A5):
 * mmidx_probe_lds_gather: the gather of the exact scan alone -- per code m random 8-byte LDS reads over 2 KiB rows, summed
 *   in fp64, `chains` (1 or 3) codes in flight per lane, 256-thread blocks at the scan kernel's occupancy; m in {8, 16, 32}.
 *   out[0] = wave-level ds_read_b64 per second, out[1] = GB/s of "algorithmic bytes" (codes x m), out[2] = blocks per CU,
 *   out[3] = seconds.
 * mmidx_probe_split_gather: the m = 16 loop with the last kg (1, 2 or 4) rows gathered through the vector-memory path (a
 *   per-block copy in global memory, L1-resident) and the others from the LDS -- the experiment behind DESIGN section 9's
 *   "share the gather between the two pipes"; out as mmidx_probe_lds_gather.
 * mmidx_probe_f64_mfma: back-to-back v_mfma_f64_16x16x4_f64 on every SIMD; out[0] = TFLOP/s, out[1] = seconds.
 * mmidx_probe_sym_eig: the PCA learners' device eigen-solver alone (cyclic Jacobi, csrc/mmidx_dense_solve.h), 1 <= b <= 1056.  T is
 *   a host matrix [b][b] (symmetrised as (T + T^T) / 2); lam_out[b] descending, Wt_out[b][b] with row i the unit eigenvector of
 *   lam_out[i] (the layout of the host solver), *sweeps_out the Jacobi sweeps run.  A non-finite entry: MMIDX_ERR_INVALID_ARG,
 *   nothing written. */
int mmidx_probe_lds_gather(int device, int m, int chains, double *out);
int mmidx_probe_split_gather(int device, int kg, double *out);
int mmidx_probe_f64_mfma(int device, double *out);
int mmidx_probe_sym_eig(int device, int b, const double *T, double *lam_out, double *Wt_out, int32_t *sweeps_out);

/* ---- front end of BASELINE config 5 ----------------------------------------------------------
 * PCA projection: PCA.loadPCAFromFile (J/dimreduction/PCA.java:257-318) + sampleToEigenSpace
 * (:188-208).  means[ss] = line 1 of the PCA file, eig[nc] = line 2 (used iff whitening: the
 * library folds W = diag(eig^-0.5) into V_t exactly as :283-313 does), Vt[nc][ss] = the component
 * lines.  project: Y[n][nc] = V_t (X[n] - means), L2-normalised iff whitening (:203-204).  This is
 * the one dense contraction of the path and runs on the f64 matrix cores; results agree with the
 * reference to 1e-12 (relative to the row norm), not bit-for-bit (EJML summation order, A2). */
typedef struct mmidx_pca mmidx_pca;
int mmidx_pca_create(int nc, int ss, int whitening, const double *means, const double *eig,
                     const double *Vt, int device, mmidx_pca **out);
int mmidx_pca_destroy(mmidx_pca *p);
int mmidx_pca_get_dims(const mmidx_pca *p, int *nc_out, int *ss_out); /* numComponents, sampleSize of the handle */
int mmidx_pca_project(mmidx_pca *p, int64_t n, const double *X, double *Y);
int mmidx_pca_project_device(mmidx_pca *p, int64_t n, const double *dX, double *dY, void *stream);

/* Learning the PCA basis: PCA.addSample / computeBasis (J/dimreduction/PCA.java:120-177; driver PCALearningExample.java:36-55).
 * create = the constructor (:101-111): room for num_samples rows of ss doubles in HBM, where the samples stay until destroy, as
 * the reference keeps them in A (:109).  add = addSample for n rows at once, in arrival order (host rows, or rows already in the
 * HBM of the learner's device; the _device form is asynchronous on `stream`).  compute = computeBasis:
 *   means_out[ss]   the reference's loop (:142-153): every column summed in arrival order into a zero-initialised double, one
 *                   division by num_samples -- BIT-EXACT, also when the samples arrived in several add calls;
 *   sv_out[nc]      the largest nc SINGULAR VALUES OF THE CENTRED SAMPLE MATRIX, descending, NOT divided by n or n - 1: this is what
 *                   savePCAToFile writes on line 2 (W.get(i, i), :234-237) and what the loader whitens with value^-0.5 (:283-285);
 *   Vt_out[nc][ss]  the matching orthonormal right singular vectors, one per row.  Sign: in every row the entry of largest
 *                   magnitude (lowest index on a tie) is positive.  EJML's SVD is an absent third-party dependency whose
 *                   arithmetic and row signs cannot be reproduced (assumption A2): the contract is mathematical.
 * Method: Gram matrix of the centred samples on the f64 matrix cores, then blocked subspace iteration with Rayleigh-Ritz (block
 * nc + 32) until max_i ||G v_i - sv_i^2 v_i||_2 <= tol * sv_1^2 over the nc components; *iters_out = iterations run,
 * *residual_out = the achieved value of that ratio.  Not converged within max_iter: MMIDX_ERR_NOT_CONVERGED, the message carries the
 * residual, all outputs are still written.  The Gram route squares the condition number: components with sv below ~1e-8 sv_1 are
 * not resolved.  Deterministic (fixed start block, no atomics).  Any output pointer may be NULL.
 * Envelope: 1 <= nc <= ss <= 16384, nc <= 1024, num_samples < 2^31 (else MMIDX_ERR_UNSUPPORTED).  Errors as the reference's, all
 * MMIDX_ERR_INVALID_ARG and raised before any device call: nc > ss "More components requested than the data's length." (:102-104);
 * more than num_samples rows "Too many samples" (:121-122); compute before all rows "Not all the data has been added" (:136-137);
 * nc > num_samples "More data needed to compute the desired number of components" (:138-140). */
typedef struct mmidx_pca_learner mmidx_pca_learner;
int mmidx_pca_learn_create(int nc, int64_t num_samples, int ss, int device, mmidx_pca_learner **out);
int mmidx_pca_learn_add(mmidx_pca_learner *l, int64_t n, const double *X);
int mmidx_pca_learn_add_device(mmidx_pca_learner *l, int64_t n, const double *dX, void *stream);
int mmidx_pca_learn_compute(mmidx_pca_learner *l, double tol, int max_iter, double *means_out, double *sv_out,
                            double *Vt_out, int32_t *iters_out, double *residual_out);
int mmidx_pca_learn_destroy(mmidx_pca_learner *l);

/* The same basis from a STREAM of samples: no num_samples, rows are folded into the Gram matrix as they arrive and are not kept.
 * This is the learner for the flagship front end (4 x 128 SURF centroids, a 32768-long VLAD vector, 32768 -> 1024), whose samples
 * do not fit a device.  add / add_device as above; count = rows so far; compute = computeBasis over the rows so far, with the
 * outputs, sign rule, determinism and MMIDX_ERR_NOT_CONVERGED behaviour of mmidx_pca_learn_compute:
 *   means_out   BIT-EXACT: the reference's sequential column sums (:142-153) kept running across add calls, one division by the count;
 *   sv_out, Vt_out   as above, for the Gram matrix centred by the exact mean of the rows (it differs from the resident learner's,
 *               centred by the rounded sequential mean, by n delta delta^T: second order in the rounding of the mean).  One step
 *               more than the resident learner: every row of Vt_out is divided by its 2-norm, so |v| = 1 to an ulp where the
 *               resident learner's rows are unit to the 10-20 eps that V = Q W leaves (its output bytes are kept as they were).
 * THE RESULT BYTES DO NOT DEPEND ON HOW THE ROWS WERE SPLIT OVER add CALLS: rows wait in a staging block of R rows, R fixed by ss
 * alone (2^25 / ss rounded down to a multiple of 64, within 64 .. 4096: at most 256 MiB), and a full block is folded in one launch:
 * Gt += (X - m0)^T (X - m0) on the f64 matrix cores and st += sum (x - m0), where the shift m0 is the first row; compute folds the
 * tail and finalises G = Gt - st st^T / n.  (Accumulating uncentred X^T X and subtracting n mu mu^T would cancel catastrophically
 * for data with an offset.)  After compute the Gram matrix is final: add is MMIDX_ERR_INVALID_ARG; compute may be called again, for
 * example with another tol or after MMIDX_ERR_NOT_CONVERGED.  MMIDX_PCA_STREAM_ROWS (read at create; a multiple of 8, at least 8)
 * overrides R for tests.
 * Device memory: ss^2 * 8 bytes for the Gram matrix (8 GiB at 32768) + R * ss * 8 for the staging block (256 MiB) + 4 * ss * 8
 * (column sums, shift, shifted sums, a zero vector) from create to destroy; during compute 5 * ss * b * 8 + nc * ss * 8 for the
 * iteration's blocks (b = min(ss, nc + 32): 1.6 GiB at 32768 -> 1024), 2 * b^2 * 8 for S and the factor, and with the device solves
 * 6 * b^2 * 8 more (two copies each of T and Wt, the unpolished eigenvectors, the polish factor: 51 MiB at b = 1056).
 * A device call that fails in the middle of an add or of the finalisation leaves the running sums unusable: every later add or
 * compute on that handle returns MMIDX_ERR_HIP; destroy it.
 * Envelope: 1 <= nc <= ss <= 32768, nc <= 1024, fewer than 2^31 rows in all (else MMIDX_ERR_UNSUPPORTED).  MMIDX_ERR_INVALID_ARG
 * before any device call: nc > ss "More components requested than the data's length."; compute with fewer rows than nc "More data
 * needed to compute the desired number of components"; add after compute.
 * Both learners solve the b x b eigenproblems of an iteration on the device (cyclic Jacobi) for
 * 256 < b <= 512 and on the host otherwise: below as always, above until the device form has been measured to win there;
 * MMIDX_PCA_LEARN_SOLVE=host|device, read by compute, forces either at any b. */
typedef struct mmidx_pca_stream mmidx_pca_stream;
int mmidx_pca_stream_create(int nc, int ss, int device, mmidx_pca_stream **out);
int mmidx_pca_stream_add(mmidx_pca_stream *s, int64_t n, const double *X);
int mmidx_pca_stream_add_device(mmidx_pca_stream *s, int64_t n, const double *dX, void *stream);
int mmidx_pca_stream_count(const mmidx_pca_stream *s, int64_t *n_out);
int mmidx_pca_stream_compute(mmidx_pca_stream *s, double tol, int max_iter, double *means_out, double *sv_out,
                             double *Vt_out, int32_t *iters_out, double *residual_out);
int mmidx_pca_stream_destroy(mmidx_pca_stream *s);

/* VLAD aggregation: VladAggregator.aggregateInternal (J/aggregation/VladAggregator.java:56-70) with
 * computeNearestCentroid (AbstractFeatureAggregator.java:136-155), and the multi-vocabulary wrapper
 * with power + L2 normalisation (VladAggregatorMultipleVocabularies.java:84-101).  codebooks =
 * the nvocab codebooks concatenated, ncent[i] centroids of dl doubles each.  desc_off[nimg+1]
 * delimits each image's descriptors in descs[total][dl].  out[nimg][sum ncent*dl].  Without
 * normalisation the output is bit-exact (accumulation in descriptor order); with it, 1e-12. */
typedef struct mmidx_vlad mmidx_vlad;
int mmidx_vlad_create(int nvocab, const int32_t *ncent, int dl, const double *codebooks,
                      int normalizations_on, int device, mmidx_vlad **out);
/* "exact" = 1: the one-kernel form (fp64 brute-force nearest centroid inside the image's block) instead of the default -- the
 * nearest centroid of every descriptor of the call by the encoder's certified bf16-MFMA argmin (identical result: first index wins,
 * AFA:136-155; flagged descriptors redone in fp64), then the ordered accumulation.  A/B and test switch (ABI version 6).
 * "two_pass" = 1 (ABI version 7): assignment and accumulation as two kernels (K8') also where the default one-kernel form K8''
 * (k_vlad_fused: 64-dimensional descriptors, vocabularies of <= 128 centroids -- one pass over the descriptors, no host
 * synchronisation inside mmidx_vlad_aggregate_device) applies.
 * Envelope of "exact": the block keeps the codebook in LDS beside its lists,
 *   ncent * dl * 8 + 2 * 4 * max(2, max_desc rounded up to even) + 4 * ((ncent + 2) & ~1) + 32 bytes <= 160 KiB,
 * else the call returns MMIDX_ERR_UNSUPPORTED ("codebook N x DL plus M descriptors per image exceed the 160 KiB LDS") before any
 * launch for that vocabulary, and the handle stays usable: 128 x 128 fits, 256 x 128 and 128 x 192 do not.
 * The _device forms: d_desc_off[nimg + 1] holds ABSOLUTE row offsets into d_descs, so images i0 .. i0 + n of a batch are passed as
 * (n, d_desc_off + i0) with the same d_descs; the forms that assign as a stage of their own read d_desc_off[nimg] back (one wait on
 * `stream`) and assign rows 0 .. d_desc_off[nimg].  max_desc may be overstated (it sizes LDS lists only), never understated.
 * Alignment: d_descs and d_out need the alignment of a double (8 bytes) and no more.  A d_descs that is also 16-byte aligned --
 * any allocation's base, and every row offset from it when dl is even -- lets the one-kernel form K8'' and the assignment's
 * single-chunk form load rows as double2; otherwise K8' with single-double loads serves the call, with identical results. */
int mmidx_vlad_set_option(mmidx_vlad *v, const char *name, int value);
int mmidx_vlad_destroy(mmidx_vlad *v);
int mmidx_vlad_vector_length(const mmidx_vlad *v, int *len_out);
int mmidx_vlad_descriptor_length(const mmidx_vlad *v, int *dl_out);
int mmidx_vlad_aggregate(mmidx_vlad *v, int64_t nimg, const int64_t *desc_off, const double *descs,
                         double *out);
int mmidx_vlad_aggregate_device(mmidx_vlad *v, int64_t nimg, const int64_t *d_desc_off,
                                const double *d_descs, int max_desc, double *d_out, void *stream);

/* ImageVectorization.transformToVector (J/vectorization/ImageVectorization.java:169-208) for a batch of images:
 * aggregate (VLAD) then PCA.sampleToEigenSpace in one call; the VLAD vectors stay on the device.  out[nimg][nc]. */
int mmidx_vectorize(mmidx_vlad *v, mmidx_pca *p, int64_t nimg, const int64_t *desc_off, const double *descs,
                    double *out);
int mmidx_vectorize_device(mmidx_vlad *v, mmidx_pca *p, int64_t nimg, const int64_t *d_desc_off,
                           const double *d_descs, int max_desc, double *d_out, void *stream);

/* Bag-of-words aggregation: BowAggregator.aggregateInternal (J/aggregation/BowAggregator.java:39-74) for a batch of images.
 * codebook[nc][dl] = the vocabulary; desc_off[nimg+1] delimits each image's descriptors in descs[total][dl], exactly as for
 * mmidx_vlad_aggregate; out[nimg][nc] (getVectorLength() == numCentroids), raw counts, no normalisation.
 *   k == 1 (hard)  bow[computeNearestCentroid(d)]++ per descriptor (AbstractFeatureAggregator.java:136-155; strict `<`: the first
 *                  of several equally near centroids wins).
 *   k  > 1 (soft)  nn = computeKNearestCentroids(d, k) (AFA:193-220), then bow[nn[j]]++ descriptorLength TIMES for each of the k
 *                  indices (the inner loop BowAggregator.java:47-51, sic): every (descriptor, neighbour) hit adds dl -- reproduced,
 *                  not "fixed".  Only the set of the k indices matters; which of several centroids tied at the k-th position
 *                  belongs to it follows the bounded queue, i.e. assumption A1, as in mmidx_coarse_device (whose loop,
 *                  IVFPQ.java:575-601, is AFA:193-220 line for line and which serves this path).
 * All values are integers far below 2^53: the output is BIT-EXACT.  Counters are 32-bit hit counts (the x dl weight is applied once
 * at the end): one word may take up to 2^32 - 1 hits of one image.
 * create: MMIDX_ERR_INVALID_ARG, raised before any device call, for a null pointer, nc < 1, dl < 1, k < 1 (the LingPipe queue
 * constructor throws) and k > nc (AFA:214-217 polls an emptied queue: NullPointerException); k > 5459 is MMIDX_ERR_UNSUPPORTED, also
 * before any device call (the coarse stage's exact selection keeps k + 1 entries of 12 bytes in a 64 KiB LDS block); a null handle is refused the same way
 * by every call but destroy.  The descriptor-length check of aggregate (AFA:72-79, "Descriptor length is incompatible with codebook centroid
 * length!") belongs to the binding, which sees the arrays: mmidx_bow_get_dims (any pointer may be NULL) gives it the lengths.
 * set_option: "exact" = 1: the assignment through the hidden handle's "exact_coarse" (fp64, no matrix-core bound); "hist_global" = 1:
 * the global-memory histogram also where the LDS form applies (up to 40960 words); "chunk_images" = n: the host form takes n images
 * per round (0 = automatic: the dense [chunk][nc] workspace stays under 1 GiB).  None of them changes a result.
 * aggregate_device: asynchronous on `stream` except for two read-backs: the descriptor range of the call (desc_off[0],
 * desc_off[nimg]: 16 bytes into pinned memory, one wait) and, for k == 1, the count inside mmidx_assign_device.
 * threading: every call on a handle takes the handle's mutex, so calls from several threads are served one after the other; a
 * _device call holds it while its work is enqueued, and a call on another stream than the one before first waits for that stream
 * (the workspaces are shared).  max_desc (largest descriptor count of an image) is
 * accepted for symmetry with mmidx_vlad_aggregate_device; no workspace is sized by it. */
typedef struct mmidx_bow mmidx_bow;
int mmidx_bow_create(int nc, int dl, int k, const double *codebook, int device, mmidx_bow **out);
int mmidx_bow_destroy(mmidx_bow *b);
int mmidx_bow_get_dims(const mmidx_bow *b, int *nc, int *dl, int *k);
int mmidx_bow_set_option(mmidx_bow *b, const char *name, int value);
int mmidx_bow_aggregate(mmidx_bow *b, int64_t nimg, const int64_t *desc_off, const double *descs, double *out);
int mmidx_bow_aggregate_device(mmidx_bow *b, int64_t nimg, const int64_t *d_desc_off, const double *d_descs, int max_desc,
                               double *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
