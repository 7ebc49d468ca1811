package gr.iti.mklab.visual.quantization;

import gr.iti.mklab.visual.datastructures.MmidxNative;
import gr.iti.mklab.visual.datastructures.PQ.TransformationType;
import gr.iti.mklab.visual.utilities.RandomPermutation;

import java.io.BufferedWriter;
import java.io.FileWriter;
import java.util.Random;

/**
 * {@link ProductQuantizationLearning} on an MI355X: the residuals, the transformation and the m x numKmeansRepeats k-means problems
 * of ProductQuantizationLearning.java:225-305 in one native call (mmidx_pq_learn), every kernel launch shared by all of them. The
 * clustering restates SimpleKMeans (k-means++ with the seeds 1..numKmeansRepeats, min-max normalised attributes, empty clusters
 * dropped); Weka's own random stream and summation order are not reproduced. Sub-vectors of at most 16 values and tables of at most
 * 64 KiB (numProductCentroids x subVectorLength doubles); anything else throws.
 */
public class GpuProductQuantizationLearning {

	private GpuProductQuantizationLearning() {
	}

	/** the kept repeat per sub-quantizer, filled by the last {@link #learn}: squared error, seed, real centroids, iterations */
	public static double[] lastSse;
	public static int[] lastSeed, lastNumCentroids, lastIterations;

	/**
	 * @param vectors
	 *            the learning vectors, [numVectors][vectorLength]
	 * @param coarseQuantizer
	 *            [numCoarseCentroids][vectorLength] for IVFADC (residuals are learned), null for ADC
	 * @param BDBpath
	 *            where the file is written, under the reference's name (ProductQuantizationLearning.java:189-199); null writes none
	 * @return the product quantizer [m][numProductCentroids][vectorLength / m]; missing centroids are rows of 1000
	 */
	public static double[][][] learn(double[][] vectors, int m, int numProductCentroids, int maxIterations, int numKmeansRepeats,
			double[][] coarseQuantizer, TransformationType transformation, String BDBpath) throws Exception {
		int numVectors = vectors.length;
		int vectorLength = vectors[0].length;
		if (vectorLength % m != 0) { // ProductQuantizationLearning.java:168-170
			throw new Exception("d is not a multiple of m");
		}
		int subVectorLength = vectorLength / m;
		if ((long) numVectors * vectorLength > Integer.MAX_VALUE || (long) numProductCentroids * vectorLength > Integer.MAX_VALUE) {
			throw new Exception("The learning vectors or the product quantizer exceed a Java array (2^31 - 1 values)");
		}
		double[] flat = new double[numVectors * vectorLength];
		for (int i = 0; i < numVectors; i++) {
			System.arraycopy(vectors[i], 0, flat, i * vectorLength, vectorLength);
		}
		int numCoarseCentroids = coarseQuantizer == null ? 0 : coarseQuantizer.length;
		double[] coarse = null;
		if (coarseQuantizer != null) {
			coarse = new double[numCoarseCentroids * vectorLength];
			for (int i = 0; i < numCoarseCentroids; i++) {
				System.arraycopy(coarseQuantizer[i], 0, coarse, i * vectorLength, vectorLength);
			}
		}
		int[] perm = null;
		double[] rot = null;
		if (transformation == TransformationType.RandomPermutation) { // RandomPermutation(1, d), :178
			double[] identity = new double[vectorLength];
			for (int i = 0; i < vectorLength; i++) {
				identity[i] = i;
			}
			double[] permuted = new RandomPermutation(1, vectorLength).permute(identity); // permuted[i] = perm[i]
			perm = new int[vectorLength];
			for (int i = 0; i < vectorLength; i++) {
				perm[i] = (int) permuted[i];
			}
		} else if (transformation == TransformationType.RandomRotation) { // RandomRotation(1, d), :176
			rot = org.ejml.ops.RandomMatrices.createOrthogonal(vectorLength, vectorLength, new Random(1)).getData();
		}
		double[] pq = new double[numProductCentroids * vectorLength];
		lastSse = new double[m];
		lastSeed = new int[m];
		lastNumCentroids = new int[m];
		lastIterations = new int[m];
		MmidxNative.pqLearn(Integer.getInteger("mmidx.device", 0), numVectors, vectorLength, m, numProductCentroids, maxIterations,
				numKmeansRepeats, true, flat, numCoarseCentroids, coarse, transformation.ordinal(), perm, rot, pq, lastSse, lastSeed,
				lastNumCentroids, lastIterations);

		double[][][] out = new double[m][numProductCentroids][subVectorLength];
		for (int s = 0; s < m; s++) {
			for (int j = 0; j < numProductCentroids; j++) {
				System.arraycopy(pq, (s * numProductCentroids + j) * subVectorLength, out[s][j], 0, subVectorLength);
			}
		}
		if (BDBpath != null) {
			// pq_<d>_<m>x<log2 ks>_<vectors>[_rr | _rp][_ivf_c<C>].csv, the name the reference's loaders are pointed at
			int bits = (int) (Math.log(numProductCentroids) / Math.log(2));
			String tr = transformation == TransformationType.RandomRotation ? "_rr"
					: transformation == TransformationType.RandomPermutation ? "_rp" : "";
			String ivf = coarseQuantizer == null ? "" : "_ivf_c" + numCoarseCentroids;
			String name = BDBpath + "/pq_" + vectorLength + "_" + m + "x" + bits + "_" + numVectors + tr + ivf + ".csv";
			BufferedWriter w = new BufferedWriter(new FileWriter(name));
			try {
				for (int s = 0; s < m; s++) {
					for (int j = 0; j < numProductCentroids; j++) {
						StringBuilder line = new StringBuilder();
						for (int t = 0; t < subVectorLength; t++) {
							line.append(out[s][j][t]).append(t + 1 < subVectorLength ? "," : "\n");
						}
						w.write(line.toString());
					}
				}
			} finally {
				w.close();
			}
		}
		return out;
	}
}
