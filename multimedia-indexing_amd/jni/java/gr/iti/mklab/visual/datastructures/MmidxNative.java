package gr.iti.mklab.visual.datastructures;

/**
 * JNI declarations for libmmidx_jni.so (mmidx_jni.c) -> libmmidx_hip.so (include/mmidx.h). The shim checks the length of
 * every array against the handle's dimensions before it touches it; codes travel as byte[] when numProductCentroids <= 256
 * and as short[] otherwise (IVFPQ.java:342-354), and the wrong variant throws.
 */
public final class MmidxNative {
	static {
		System.loadLibrary("mmidx_jni");
	}

	public static final int KIND_PQ = 1, KIND_IVFPQ = 2;

	public static native long create(int kind, int vectorLength, int numSubVectors, int numProductCentroids,
			int numCoarseCentroids, int transformationOrdinal, int[] permutation, double[] rotation, int device)
			throws Exception;

	/**
	 * mmidx_create_sharded: one index over the GPUs listed in devices (inverted list c lives on devices[c % devices.length]); every
	 * other method takes the returned handle unchanged. One JVM drives all of them, as the reference's caller holds the whole
	 * index in one process.
	 */
	public static native long createSharded(int kind, int vectorLength, int numSubVectors, int numProductCentroids,
			int numCoarseCentroids, int transformationOrdinal, int[] permutation, double[] rotation, int[] devices)
			throws Exception;

	public static native void destroy(long handle);

	public static native void setCoarse(long handle, double[] flatCoarse) throws Exception;

	public static native void setPq(long handle, double[] flatProductQuantizer) throws Exception;

	public static native void setW(long handle, int w) throws Exception;

	/** mmidx_add_vectors for one vector; cellOut[0] and codeOut[numSubVectors] receive the record */
	public static native void addVector(long handle, int iid, double[] vector, int[] cellOut, byte[] codeOut)
			throws Exception;

	public static native void addVectorShort(long handle, int iid, double[] vector, int[] cellOut, short[] codeOut)
			throws Exception;

	/** mmidx_add_codes: n records; cells == null for PQ */
	public static native void addCodes(long handle, int n, int[] iids, int[] cells, byte[] codes) throws Exception;

	public static native void addCodesShort(long handle, int n, int[] iids, int[] cells, short[] codes) throws Exception;

	/** mmidx_get_codes: list ids and stored codes of iids.length internal ids; either output may be null */
	public static native void getCodes(long handle, int[] iids, int[] cellsOut, byte[] codesOut) throws Exception;

	public static native void getCodesShort(long handle, int[] iids, int[] cellsOut, short[] codesOut) throws Exception;

	/** mmidx_distance: computeDistanceIVFADC for iids.length (query, internal id) pairs, queries row-major */
	public static native void distance(long handle, double[] queries, int[] iids, double[] out) throws Exception;

	public static native void search(long handle, int k, int nq, double[] queries, int[] iidOut, double[] distOut,
			int[] countOut) throws Exception;

	/** mmidx_search_sdc: queries are internal ids (PQ.computeKnnSDC, PQ.java:334-374) */
	public static native void searchSdc(long handle, int k, int nq, int[] queryIids, int[] iidOut, double[] distOut,
			int[] countOut) throws Exception;

	/**
	 * mmidx_search_ids: queries are internal ids of an IVFPQ or PQ index; each id's stored record is decoded on the device and
	 * searched as any vector (computeKnnIVFADC / computeKnnADC). An unknown id throws "Id does not exist!".
	 */
	public static native void searchIds(long handle, int k, int nq, int[] queryIids, int[] iidOut, double[] distOut,
			int[] countOut) throws Exception;

	/**
	 * mmidx_search_refine: the R best records of the compressed answer (exactly search(handle, R, ...)) re-ranked by their exact
	 * squared distances from the rows of the Linear handle, the k best kept under the bounded queue's rule. Record iid of the
	 * index must be row iid of the Linear index (IndexTransformation.java:113-122). Returns the number of candidates without a row.
	 */
	public static native long searchRefine(long handle, long linearHandle, int k, int R, int nq, double[] queries, int[] iidOut,
			double[] distOut, int[] countOut) throws Exception;

	/** mmidx_search_refine_ids: the same with the rows queryIids[q] of the Linear handle as the queries (Linear.java:181-184) */
	public static native long searchRefineIds(long handle, long linearHandle, int k, int R, int nq, int[] queryIids, int[] iidOut,
			double[] distOut, int[] countOut) throws Exception;

	/** mmidx_reconstruct: out[iids.length * vectorLength] = the vectors the index holds for the given internal ids */
	public static native void reconstruct(long handle, int[] iids, double[] out) throws Exception;

	/**
	 * mmidx_remove: every stored record with one of these internal ids leaves the index (the survivors keep their list and their
	 * order inside it); found[n] (may be null) = 1 where the id was stored; returns the number of records removed
	 */
	public static native long remove(long handle, int[] iids, int[] found) throws Exception;

	public static native void listSizes(long handle, int[] out) throws Exception;

	/** mmidx_save / mmidx_load (ABI 8): the native flat snapshot -- list offsets, iids and stored codes as loadIndexInMemory builds them */
	public static native void saveSnapshot(long handle, String path) throws Exception;

	public static native void loadSnapshot(long handle, String path) throws Exception;

	/** mmidx_get_stats as {total_ms, coarse_ms, scan_ms, merge_ms, scan_codes, scan_launches, tie_fallbacks} */
	public static native void stats(long handle, double[] out7) throws Exception;

	public static native void setProfiling(long handle, int mode) throws Exception;

	/* ---- Linear (mmidx_linear_*) ---- */
	public static native long linearCreate(int vectorLength, long maxNumVectors, int device) throws Exception;

	public static native void linearDestroy(long handle);

	public static native void linearAdd(long handle, int n, int vectorLength, double[] flatVectors) throws Exception;

	public static native void linearSearch(long handle, int k, int nq, int vectorLength, double[] queries, int[] iidOut,
			double[] distOut, int[] countOut) throws Exception;

	/** computeNearestNeighborsInternal(k, int iid), Linear.java:181-184: the stored vectors are the queries */
	public static native void linearSearchIds(long handle, int k, int nq, int[] iids, int[] iidOut, double[] distOut,
			int[] countOut) throws Exception;

	/** "exact", "mfma_qcap", "debug_sync" (include/mmidx.h, Linear section) */
	public static native void linearSetOption(long handle, String name, int value) throws Exception;

	/**
	 * mmidx_linear_reindex: rows iid0 .. iid0 + n - 1 of the Linear handle src, projected through the PCA handle pca (0 = none),
	 * truncated to every target's vector length, L2-normalised (normalize[t]: 0 never, 1 always, 2 where truncated) and appended
	 * to the targets in one pass on the GPU (IndexTransformation.java:111-123, PCAProjectionExample.java:74-88). kinds[t] = 0:
	 * targets[t] is a Linear handle, 1: a PQ / IVFPQ handle. Every target must hold exactly iid0 vectors. chunkRows 0 = default.
	 */
	public static native void linearReindex(long src, long iid0, long n, long pca, int[] kinds, long[] targets, int[] normalize,
			long chunkRows) throws Exception;

	/* ---- front end (mmidx_pca_*, mmidx_vlad_*, mmidx_vectorize) ---- */
	public static native long pcaCreate(int numComponents, int sampleSize, boolean whitening, double[] means,
			double[] eigenvalues, double[] components, int device) throws Exception;

	public static native void pcaDestroy(long pca);

	public static native void pcaProject(long pca, int n, int sampleSize, int numComponents, double[] samples,
			double[] projected) throws Exception;

	/* ---- learning the PCA basis (mmidx_pca_learn_*): PCA.addSample / computeBasis ---- */
	public static native long pcaLearnCreate(int numComponents, int numSamples, int sampleSize, int device)
			throws Exception;

	public static native void pcaLearnDestroy(long learner);

	public static native void pcaLearnAdd(long learner, int n, int sampleSize, double[] samples) throws Exception;

	/** returns the iterations run; residualOut[0] = achieved residual; throws when maxIter is reached above tol */
	public static native int pcaLearnCompute(long learner, int numComponents, int sampleSize, double tol, int maxIter,
			double[] means, double[] singularValues, double[] components, double[] residualOut) throws Exception;

	/* ---- the same from a stream of samples that are not kept (mmidx_pca_stream_*): sampleSize up to 32768 ---- */
	public static native long pcaStreamCreate(int numComponents, int sampleSize, int device) throws Exception;

	public static native void pcaStreamDestroy(long stream);

	public static native void pcaStreamAdd(long stream, int n, int sampleSize, double[] samples) throws Exception;

	public static native long pcaStreamCount(long stream) throws Exception;

	/** as pcaLearnCompute, over the rows added so far; afterwards the stream takes no more samples */
	public static native int pcaStreamCompute(long stream, int numComponents, int sampleSize, double tol, int maxIter,
			double[] means, double[] singularValues, double[] components, double[] residualOut) throws Exception;

	/**
	 * mmidx_pq_learn: the whole product quantizer in one call. vectors[n * D]; coarse[C * D] or null (flat PQ); perm[D] / rot[D * D]
	 * or null as the transformation (0 none, 1 rotation, 2 permutation) wants; pq[m * ks * (D / m)]; sse / seed / k / iterations [m]
	 * each, of the kept repeat, any may be null
	 */
	public static native void pqLearn(int device, int n, int vectorLength, int m, int numProductCentroids, int maxIterations,
			int numKmeansRepeats, boolean normalize, double[] vectors, int numCoarseCentroids, double[] coarse, int transformation,
			int[] perm, double[] rot, double[] pq, double[] sse, int[] seed, int[] k, int[] iterations) throws Exception;

	public static native long vladCreate(int[] numCentroids, int descriptorLength, double[] codebooks,
			boolean normalizationsOn, int device) throws Exception;

	public static native void vladDestroy(long vlad);

	public static native int vladVectorLength(long vlad) throws Exception;

	/** pca == 0: aggregate only (outLen = VLAD length); else aggregate + sampleToEigenSpace (outLen = components) */
	public static native void vladAggregate(long vlad, long pca, int descriptorLength, int outLen, long[] descOff,
			double[] descriptors, double[] out) throws Exception;

	/* ---- bag of words (mmidx_bow_*): BowAggregator.aggregateInternal, k = 1 hard, k > 1 soft ---- */
	public static native long bowCreate(int numCentroids, int descriptorLength, int k, double[] codebook, int device)
			throws Exception;

	public static native void bowDestroy(long bow);

	/** out[nimg][numCentroids]; descriptorLength and outLen are checked against the native object */
	public static native void bowAggregate(long bow, int descriptorLength, int outLen, long[] descOff,
			double[] descriptors, double[] out) throws Exception;

	private MmidxNative() {
	}
}
