package gr.iti.mklab.visual.aggregation;

import java.util.ArrayList;

import gr.iti.mklab.visual.datastructures.MmidxNative;

/**
 * {@link BowAggregator} on an MI355X: aggregateInternal of BowAggregator.java:39-74. k = 1 counts every descriptor at its nearest
 * centroid (computeNearestCentroid, AbstractFeatureAggregator.java:136-155); k &gt; 1 counts it at its k nearest centroids
 * (computeKNearestCentroids, AFA:193-220), each hit adding descriptorLength as the reference's inner loop does (:47-51). The
 * vectors are raw counts, bit-exact; a batch overload serves many images in one call.
 */
public class GpuBowAggregator {

	private final long handle;
	private final int numCentroids, descriptorLength;

	/** hard assignment, BowAggregator(double[][] codebook) */
	public GpuBowAggregator(double[][] codebook) throws Exception {
		this(codebook, 1);
	}

	/** soft assignment to the k nearest centroids, BowAggregator(double[][] codebook, int k) */
	public GpuBowAggregator(double[][] codebook, int k) throws Exception {
		if (codebook == null || codebook.length == 0 || codebook[0] == null || codebook[0].length == 0)
			throw new IllegalArgumentException("the codebook is empty");
		numCentroids = codebook.length;
		descriptorLength = codebook[0].length;
		if ((long) numCentroids * descriptorLength > Integer.MAX_VALUE)
			throw new IllegalArgumentException("the codebook does not fit a Java array");
		double[] flat = new double[numCentroids * descriptorLength];
		int o = 0;
		for (double[] c : codebook) {
			if (c == null || c.length != descriptorLength)
				throw new IllegalArgumentException("codebook rows differ in length");
			System.arraycopy(c, 0, flat, o, descriptorLength);
			o += descriptorLength;
		}
		handle = MmidxNative.bowCreate(numCentroids, descriptorLength, k, flat, Integer.getInteger("mmidx.device", 0));
	}

	public int getVectorLength() {
		return numCentroids;
	}

	public int getNumCentroids() {
		return numCentroids;
	}

	public int getDescriptorLength() {
		return descriptorLength;
	}

	public double[] aggregate(double[][] descriptors) throws Exception {
		return aggregate(new double[][][] { descriptors })[0];
	}

	public double[] aggregate(ArrayList<double[]> descriptors) throws Exception {
		return aggregate(descriptors.toArray(new double[descriptors.size()][]));
	}

	/** one call for a batch of images */
	public double[][] aggregate(double[][][] images) throws Exception {
		long[] off = new long[images.length + 1];
		for (int i = 0; i < images.length; i++)
			off[i + 1] = off[i] + images[i].length;
		// (both products in long: a batch beyond a Java array is refused, not wrapped around)
		if (off[images.length] * descriptorLength > Integer.MAX_VALUE || (long) images.length * numCentroids > Integer.MAX_VALUE)
			throw new IllegalArgumentException("the batch does not fit a Java array: aggregate it in smaller parts");
		double[] descs = new double[(int) (off[images.length] * descriptorLength)];
		int o = 0;
		for (double[][] img : images)
			for (double[] d : img) {
				if (d == null || d.length != descriptorLength) // AbstractFeatureAggregator.java:72-79
					throw new Exception("Descriptor length is incompatible with codebook centroid length!");
				System.arraycopy(d, 0, descs, o, descriptorLength);
				o += descriptorLength;
			}
		double[] out = new double[images.length * numCentroids];
		MmidxNative.bowAggregate(handle, descriptorLength, numCentroids, off, descs, out);
		double[][] res = new double[images.length][];
		for (int i = 0; i < images.length; i++)
			res[i] = java.util.Arrays.copyOfRange(out, i * numCentroids, (i + 1) * numCentroids);
		return res;
	}

	public void close() {
		MmidxNative.bowDestroy(handle);
	}
}
