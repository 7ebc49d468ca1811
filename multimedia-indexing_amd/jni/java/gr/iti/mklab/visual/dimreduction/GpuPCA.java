package gr.iti.mklab.visual.dimreduction;

import gr.iti.mklab.visual.datastructures.MmidxNative;

import java.io.BufferedReader;
import java.io.BufferedWriter;
import java.io.FileReader;
import java.io.FileWriter;

/**
 * {@link PCA} on an MI355X: loadPCAFromFile (PCA.java:257-318) + sampleToEigenSpace (PCA.java:188-208), plus a batch overload
 * (one f64-MFMA GEMM for n samples); results agree with EJML to 1e-12 relative to the row norm, not bit for bit (summation order).
 * Learning: addSample / computeBasis / savePCAToFile (PCA.java:120-177, :219-247). The means are the reference's, bit for bit; the
 * components and singular values come from a Gram matrix on the f64 matrix cores and a subspace iteration instead of EJML's SVD:
 * the same quantities mathematically, with our own sign rule (in every row the entry of largest magnitude is positive; EJML's
 * row signs are arbitrary), which changes no distance computed after projection. Line 2 of the file holds the singular values of
 * the centred sample matrix, not divided by n, exactly as the reference writes W.get(i, i).
 */
public class GpuPCA {

	private final int numComponents, sampleSize;
	private int numSamples; // streaming: the count at computeBasis
	private final boolean doWhitening, streaming;
	private long handle;
	// learning side
	private long learner;
	private int sampleIndex;
	private double[] means, singularValues, components;
	private int iterations;
	private double residual;

	public GpuPCA(int numComponents, int numTrainingSamples, int sampleSize, boolean doWhitening) { // PCA.java:75-111
		if (numComponents > sampleSize) {
			throw new IllegalArgumentException("More components requested than the data's length.");
		}
		this.numComponents = numComponents;
		this.numSamples = numTrainingSamples;
		this.sampleSize = sampleSize;
		this.doWhitening = doWhitening;
		this.streaming = false;
	}

	/**
	 * A PCA that learns from a stream of samples (mmidx_pca_stream_*): no numTrainingSamples, the samples are folded into the Gram
	 * matrix as they arrive and are not kept, sampleSize up to 32768 (the 32768 to 1024 basis of the four-vocabulary SURF VLAD).
	 * computeBasis works on the samples added so far; after it no more are taken. The result does not depend on how the samples
	 * were split over addSample / addSamples calls.
	 */
	public GpuPCA(int numComponents, int sampleSize, boolean doWhitening) {
		if (numComponents > sampleSize) {
			throw new IllegalArgumentException("More components requested than the data's length.");
		}
		this.numComponents = numComponents;
		this.numSamples = 0;
		this.sampleSize = sampleSize;
		this.doWhitening = doWhitening;
		this.streaming = true;
	}

	private void ensureLearner() throws Exception {
		if (learner != 0)
			return;
		int device = Integer.getInteger("mmidx.device", 0);
		learner = streaming ? MmidxNative.pcaStreamCreate(numComponents, sampleSize, device)
				: MmidxNative.pcaLearnCreate(numComponents, numSamples, sampleSize, device);
	}

	public void addSample(double[] sampleData) throws Exception { // PCA.java:120-130
		if (!streaming && sampleIndex >= numSamples)
			throw new IllegalArgumentException("Too many samples");
		if (sampleData.length != sampleSize)
			throw new IllegalArgumentException("Unexpected sample size");
		addSamples(sampleData, 1);
	}

	/** n samples row-major, in arrival order */
	public void addSamples(double[] samples, int n) throws Exception {
		if (n < 0 || (!streaming && (long) sampleIndex + n > numSamples))
			throw new IllegalArgumentException("Too many samples");
		if (samples.length != (long) n * sampleSize)
			throw new IllegalArgumentException("Unexpected sample size");
		ensureLearner();
		if (streaming)
			MmidxNative.pcaStreamAdd(learner, n, sampleSize, samples);
		else
			MmidxNative.pcaLearnAdd(learner, n, sampleSize, samples);
		sampleIndex += n;
	}

	public void computeBasis() throws Exception { // PCA.java:135-177
		computeBasis(1e-12, 200);
	}

	/** stops when max_i ||G v_i - sv_i^2 v_i|| <= tol * sv_1^2; throws (results kept) when maxIter is reached first */
	public void computeBasis(double tol, int maxIter) throws Exception {
		if (streaming)
			numSamples = sampleIndex;
		if (sampleIndex != numSamples)
			throw new IllegalArgumentException("Not all the data has been added");
		if (numComponents > numSamples)
			throw new IllegalArgumentException("More data needed to compute the desired number of components");
		ensureLearner();
		means = new double[sampleSize];
		singularValues = new double[numComponents];
		components = new double[numComponents * sampleSize];
		double[] res = new double[1];
		iterations = maxIter; // (what a not-converged call, which throws, has run)
		try {
			iterations = streaming
					? MmidxNative.pcaStreamCompute(learner, numComponents, sampleSize, tol, maxIter, means, singularValues,
							components, res)
					: MmidxNative.pcaLearnCompute(learner, numComponents, sampleSize, tol, maxIter, means, singularValues,
							components, res);
		} finally {
			residual = res[0]; // written back by the shim on both paths
		}
	}

	/** PCA.java:320-322 selects one of EJML's two SVD forms; there is a single method here: a no-op kept for drop-in callers */
	public void setCompact(boolean compact) {
	}

	public void savePCAToFile(String PCAFileName) throws Exception { // PCA.java:219-247
		if (handle != 0) {
			throw new Exception("Cannot save, PCA is initialized!");
		}
		if (components == null) {
			throw new Exception("Cannot save to file, PCA matrix is null!");
		}
		BufferedWriter out = new BufferedWriter(new FileWriter(PCAFileName));
		for (int i = 0; i < sampleSize - 1; i++)
			out.write(means[i] + " ");
		out.write(means[sampleSize - 1] + "\n");
		for (int i = 0; i < numComponents - 1; i++)
			out.write(singularValues[i] + " ");
		out.write(singularValues[numComponents - 1] + "\n");
		for (int i = 0; i < numComponents; i++) {
			for (int j = 0; j < sampleSize - 1; j++)
				out.write(components[i * sampleSize + j] + " ");
			out.write(components[i * sampleSize + sampleSize - 1] + "\n");
		}
		out.close();
	}

	/** samples the basis was computed from (streaming: the count at computeBasis) */
	public int getNumSamples() {
		return numSamples;
	}

	public int getIterations() {
		return iterations;
	}

	public double getResidual() {
		return residual;
	}

	public void loadPCAFromFile(String PCAFileName) throws Exception { // PCA.java:257-318
		BufferedReader in = new BufferedReader(new FileReader(PCAFileName));
		String[] meanString = in.readLine().trim().split(" ");
		if (meanString.length != sampleSize) {
			in.close();
			throw new Exception("Means line is wrong!");
		}
		double[] means = new double[sampleSize];
		for (int i = 0; i < sampleSize; i++)
			means[i] = Double.parseDouble(meanString[i]);
		String line = in.readLine();
		double[] eig = null;
		if (doWhitening) {
			String[] eigString = line.trim().split(" ");
			eig = new double[numComponents];
			for (int i = 0; i < numComponents; i++)
				eig[i] = Double.parseDouble(eigString[i]);
		}
		double[] vt = new double[numComponents * sampleSize];
		for (int i = 0; i < numComponents; i++) {
			String[] comp = in.readLine().trim().split(" ");
			for (int j = 0; j < sampleSize; j++)
				vt[i * sampleSize + j] = Double.parseDouble(comp[j]);
		}
		in.close();
		// the whitening matrix diag(eig^-0.5) is folded into V_t natively, as PCA.java:283-313 does
		handle = MmidxNative.pcaCreate(numComponents, sampleSize, doWhitening, means, eig, vt,
				Integer.getInteger("mmidx.device", 0));
	}

	public double[] sampleToEigenSpace(double[] sampleData) throws Exception { // PCA.java:188-208
		if (handle == 0) {
			throw new Exception("PCA is not correctly initialized!");
		}
		if (sampleData.length != sampleSize) {
			throw new IllegalArgumentException("Unexpected vector length!");
		}
		double[] out = new double[numComponents];
		MmidxNative.pcaProject(handle, 1, sampleSize, numComponents, sampleData, out);
		return out;
	}

	/** n samples row-major -> n projected vectors row-major */
	public double[] samplesToEigenSpace(double[] samples, int n) throws Exception {
		double[] out = new double[n * numComponents];
		MmidxNative.pcaProject(handle, n, sampleSize, numComponents, samples, out);
		return out;
	}

	long nativeHandle() {
		return handle;
	}

	public void close() {
		if (handle != 0)
			MmidxNative.pcaDestroy(handle);
		handle = 0;
		if (learner != 0) {
			if (streaming)
				MmidxNative.pcaStreamDestroy(learner);
			else
				MmidxNative.pcaLearnDestroy(learner);
		}
		learner = 0;
	}
}
