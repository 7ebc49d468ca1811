package gr.iti.mklab.visual.datastructures;

import gr.iti.mklab.visual.utilities.Result;

import com.aliasi.util.BoundedPriorityQueue;
import com.sleepycat.bind.tuple.IntegerBinding;
import com.sleepycat.bind.tuple.TupleBinding;
import com.sleepycat.bind.tuple.TupleInput;
import com.sleepycat.bind.tuple.TupleOutput;
import com.sleepycat.je.Cursor;
import com.sleepycat.je.Database;
import com.sleepycat.je.DatabaseConfig;
import com.sleepycat.je.DatabaseEntry;
import com.sleepycat.je.OperationStatus;

/**
 * Drop-in for {@link Linear} (exhaustive exact search, Linear.java:138-163) over libmmidx_hip.so: same constructors, the
 * BDB store ("vlad" database, one record of vectorLength doubles per iid, Linear.java:225-236) stays in Java, the
 * in-memory vectors and the search live on the GPU (mmidx_linear_*).  Not compiled here (no JDK in the build image).
 */
public class GpuLinear extends AbstractSearchStructure {

	private final long handle;
	private final Database iidToVectorDB;

	public GpuLinear(int vectorLength, int maxNumVectors, boolean readOnly, String BDBEnvHome, boolean loadIndexInMemory,
			boolean countSizeOnLoad, int loadCounter) throws Exception {
		super(vectorLength, maxNumVectors, readOnly, countSizeOnLoad, loadCounter, loadIndexInMemory);
		handle = MmidxNative.linearCreate(vectorLength, maxNumVectors, Integer.getInteger("mmidx.device", 0));
		createOrOpenBDBEnvAndDbs(BDBEnvHome);
		DatabaseConfig dbConf = new DatabaseConfig();
		dbConf.setReadOnly(readOnly);
		dbConf.setTransactional(transactional);
		dbConf.setAllowCreate(true);
		iidToVectorDB = dbEnv.openDatabase(null, "vlad", dbConf); // Linear.java:78
		if (loadIndexInMemory) {
			loadIndexInMemory();
		}
	}

	public GpuLinear(int vectorLength, int maxNumVectors, boolean readOnly, String BDBEnvHome) throws Exception {
		this(vectorLength, maxNumVectors, readOnly, BDBEnvHome, true, true, 0);
	}

	/** the native handle, for the calls that pair this index with a compressed one (GpuIVFPQ / GpuPQ.computeNearestNeighborsRefined) */
	long nativeHandle() {
		return handle;
	}

	/**
	 * The walks of IndexTransformation.java:111-123 and PCAProjectionExample.java:74-88 as one native call (mmidx_linear_reindex):
	 * the rows of this index from the targets' common size up to its own, through the PCA handle pcaHandle (0 = none;
	 * GpuPCA.nativeHandle()), truncated to every target's vectorLength, L2-normalised by normalize[t] (0 never, 1 always, 2 where
	 * truncated) and appended to the in-memory part of the targets (GpuLinear, GpuPQ or GpuIVFPQ), without leaving the GPU. The ids
	 * are carried over here, on the Java side (getId(i) -> createMapping, as :114 and :121 do). Checked before the native call, with
	 * the reference's messages: a target whose maxNumVectors would be passed, an id a target already holds. The targets'
	 * persistent record stores are not written: a target filled this way is kept with saveSnapshot, or re-walked after a restart.
	 * Returns the number of vectors moved.
	 */
	public synchronized int reindexInto(AbstractSearchStructure[] targets, long pcaHandle, int[] normalize, long chunkRows)
			throws Exception {
		if (targets.length == 0 || normalize.length != targets.length) {
			throw new Exception("One normalization mode per target is needed!");
		}
		int iid0 = targets[0].loadCounter;
		int[] kinds = new int[targets.length];
		long[] handles = new long[targets.length];
		for (int t = 0; t < targets.length; t++) {
			if (targets[t].loadCounter != iid0) {
				throw new Exception("The target indices hold different numbers of vectors!");
			}
			if (targets[t] instanceof GpuLinear) {
				handles[t] = ((GpuLinear) targets[t]).handle;
			} else if (targets[t] instanceof GpuIVFPQ) {
				kinds[t] = 1;
				handles[t] = ((GpuIVFPQ) targets[t]).nativeHandle();
			} else if (targets[t] instanceof GpuPQ) {
				kinds[t] = 1;
				handles[t] = ((GpuPQ) targets[t]).nativeHandle();
			} else {
				throw new Exception("Unsupported index transformation type!");
			}
		}
		int n = loadCounter - iid0;
		String[] ids = new String[Math.max(n, 0)];
		for (int i = 0; i < n; i++) {
			ids[i] = getId(iid0 + i);
		}
		for (AbstractSearchStructure target : targets) {
			if (iid0 + n > target.maxNumVectors) {
				throw new Exception("Maximum index capacity reached, no more vectors can be indexed!");
			}
			for (int i = 0; i < n; i++) {
				if (ids[i] != null && target.isIndexed(ids[i])) {
					throw new Exception("Vector '" + ids[i] + "' already indexed!");
				}
			}
		}
		MmidxNative.linearReindex(handle, iid0, n, pcaHandle, kinds, handles, normalize, chunkRows); // -> mmidx_linear_reindex
		for (AbstractSearchStructure target : targets) {
			synchronized (target) {
				for (int i = 0; i < n; i++) {
					if (ids[i] != null) { // (a source row without an id gets none, as in Linear.reindex of the Python mirror)
						target.createMapping(ids[i]); // maps ids[i] <-> target.loadCounter
					}
					target.loadCounter++;
				}
			}
		}
		return n;
	}

	protected void indexVectorInternal(double[] vector) throws Exception { // Linear.java:111-122
		if (vector.length != vectorLength) {
			throw new Exception("The dimensionality of the vector is wrong!");
		}
		TupleOutput output = new TupleOutput();
		for (int i = 0; i < vectorLength; i++) {
			output.writeDouble(vector[i]);
		}
		DatabaseEntry data = new DatabaseEntry();
		TupleBinding.outputToEntry(output, data);
		DatabaseEntry key = new DatabaseEntry();
		IntegerBinding.intToEntry(loadCounter, key);
		iidToVectorDB.put(null, key, data);
		if (loadIndexInMemory) {
			MmidxNative.linearAdd(handle, 1, vectorLength, vector);
		}
	}

	protected BoundedPriorityQueue<Result> computeNearestNeighborsInternal(int k, double[] queryVector) throws Exception {
		int[] iids = new int[k];
		double[] dists = new double[k];
		int[] count = new int[1];
		MmidxNative.linearSearch(handle, k, 1, vectorLength, queryVector, iids, dists, count); // -> mmidx_linear_search
		BoundedPriorityQueue<Result> nn = new BoundedPriorityQueue<Result>(new Result(), k);
		for (int i = count[0] - 1; i >= 0; i--)
			nn.offer(new Result(iids[i], dists[i])); // worst first keeps the tie order
		return nn;
	}

	protected BoundedPriorityQueue<Result> computeNearestNeighborsInternal(int k, int iid) throws Exception {
		// Linear.java:181-184: the stored vector is the query; it is read in HBM, not fetched from the BDB store
		int[] iids = new int[k];
		double[] dists = new double[k];
		int[] count = new int[1];
		MmidxNative.linearSearchIds(handle, k, 1, new int[] { iid }, iids, dists, count); // -> mmidx_linear_search_ids
		BoundedPriorityQueue<Result> nn = new BoundedPriorityQueue<Result>(new Result(), k);
		for (int i = count[0] - 1; i >= 0; i--)
			nn.offer(new Result(iids[i], dists[i])); // worst first keeps the tie order
		return nn;
	}

	/** measurement and test switches of the native Linear: "exact", "mfma_qcap", "debug_sync" */
	public void setOption(String name, int value) throws Exception {
		MmidxNative.linearSetOption(handle, name, value);
	}

	public double[] getVector(int iid) { // Linear.java:253-280 (disk-based branch)
		DatabaseEntry key = new DatabaseEntry();
		IntegerBinding.intToEntry(iid, key);
		DatabaseEntry data = new DatabaseEntry();
		if (iidToVectorDB.get(null, key, data, null) != OperationStatus.SUCCESS) {
			return null;
		}
		TupleInput input = TupleBinding.entryToInput(data);
		double[] vector = new double[vectorLength];
		for (int i = 0; i < vectorLength; i++) {
			vector[i] = input.readDouble();
		}
		return vector;
	}

	private void loadIndexInMemory() throws Exception { // Linear.java:191-222, batched
		final int B = 4096;
		double[] buf = new double[B * vectorLength];
		int n = 0, counter = 0;
		DatabaseEntry key = new DatabaseEntry(), data = new DatabaseEntry();
		Cursor cursor = iidToVectorDB.openCursor(null, null);
		while (cursor.getNext(key, data, null) == OperationStatus.SUCCESS && counter < maxNumVectors) {
			TupleInput input = TupleBinding.entryToInput(data);
			for (int i = 0; i < vectorLength; i++) {
				buf[n * vectorLength + i] = input.readDouble();
			}
			n++;
			counter++;
			if (n == B) {
				MmidxNative.linearAdd(handle, n, vectorLength, buf);
				n = 0;
			}
		}
		if (n > 0) {
			MmidxNative.linearAdd(handle, n, vectorLength, java.util.Arrays.copyOf(buf, n * vectorLength));
		}
		cursor.close();
	}

	protected void outputIndexingTimesInternal() {
	}

	protected void closeInternal() {
		iidToVectorDB.close();
		MmidxNative.linearDestroy(handle);
	}
}
