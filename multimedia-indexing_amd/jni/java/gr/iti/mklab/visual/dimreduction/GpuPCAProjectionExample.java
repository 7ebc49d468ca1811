package gr.iti.mklab.visual.dimreduction;

import gr.iti.mklab.visual.datastructures.GpuLinear;

/**
 * {@link PCAProjectionExample} on an MI355X, with the same argument list (PCAProjectionExample.java:38-49): every vector is projected
 * once to the largest length, and each shorter length is a truncation of that projection (:79-82), L2-normalised on request
 * (:83-85) and indexed in a Linear index of its own (:86). Here projection, truncations, normalisations and appends are one call,
 * GpuLinear.reindexInto, with all target indices filled from a single pass over the rows. Not compiled here (no JDK in the build image).
 *
 * <pre>
 * args[0] folder of the full-length Linear index   args[1] its vector length   args[2] maximum number of vectors
 * args[3] PCA file   args[4] whitening (true | false)   args[5] L2 normalisation after PCA (true | false)
 * args[6] the projection lengths, increasing, comma separated (at most eight)
 * </pre>
 */
public class GpuPCAProjectionExample {

	public static void main(String[] args) throws Exception {
		String fullFolder = args[0];
		int fullLength = Integer.parseInt(args[1]), maxVectors = Integer.parseInt(args[2]);
		String pcaFile = args[3];
		boolean whitening = Boolean.parseBoolean(args[4]), l2 = Boolean.parseBoolean(args[5]);
		String[] fields = args[6].split(",");
		int[] lengths = new int[fields.length];
		for (int j = 0; j < fields.length; j++) {
			lengths[j] = Integer.parseInt(fields[j].trim());
		}

		GpuLinear fullVectors = new GpuLinear(fullLength, maxVectors, true, fullFolder, true, true, 0);
		int numVectors = Math.min(fullVectors.getLoadCounter(), maxVectors);

		GpuPCA pca = new GpuPCA(lengths[lengths.length - 1], 1, fullLength, whitening); // the largest length (:62-64)
		pca.loadPCAFromFile(pcaFile);

		GpuLinear[] projected = new GpuLinear[lengths.length];
		int[] normalize = new int[lengths.length];
		for (int j = 0; j < lengths.length; j++) {
			String folder = fullFolder + "to" + lengths[j] + (whitening ? "w" : "") + (l2 ? "_l2" : ""); // (:69-76)
			projected[j] = new GpuLinear(lengths[j], numVectors, false, folder, true, true, 0);
			normalize[j] = l2 ? 1 : 0; // always, also at the full projection length (:83-85)
		}

		int moved = fullVectors.reindexInto(projected, pca.nativeHandle(), normalize, 0);
		System.out.println(moved + " vectors projected to " + args[6]);
		for (GpuLinear p : projected) {
			p.close();
		}
		fullVectors.close();
	}
}
