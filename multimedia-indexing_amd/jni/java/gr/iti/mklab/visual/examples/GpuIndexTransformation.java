package gr.iti.mklab.visual.examples;

import gr.iti.mklab.visual.datastructures.AbstractSearchStructure;
import gr.iti.mklab.visual.datastructures.GpuIVFPQ;
import gr.iti.mklab.visual.datastructures.GpuLinear;
import gr.iti.mklab.visual.datastructures.GpuPQ;
import gr.iti.mklab.visual.datastructures.PQ.TransformationType;

/**
 * {@link IndexTransformation} on an MI355X, with the same argument list (IndexTransformation.java:61-66, :86-89, :104-105): the
 * getVector / copyOf / normalizeL2 / indexVector loop of :111-123 is one call, GpuLinear.reindexInto, which truncates, renormalises
 * and encodes every vector on the GPU. Not compiled here (no JDK in the build image).
 *
 * <pre>
 * args[0] folder of the full-length Linear index      args[1] folder of the target index
 * args[2] its vector length                           args[3] the target vector length
 * args[4] maximum number of vectors                   args[5] small | pq | ivfpq
 * pq, ivfpq:  args[6] product quantizer file   args[7] m   args[8] k_s   args[9] no | rr | rp
 * ivfpq:      args[10] coarse quantizer file   args[11] k_c
 * </pre>
 */
public class GpuIndexTransformation {

	static TransformationType transformation(String s) throws Exception {
		switch (s) {
		case "no":
			return TransformationType.None;
		case "rr":
			return TransformationType.RandomRotation;
		case "rp":
			return TransformationType.RandomPermutation;
		default:
			throw new Exception("Wrong transformation type given!");
		}
	}

	public static void main(String[] args) throws Exception {
		String fromFolder = args[0], toFolder = args[1];
		int fromLength = Integer.parseInt(args[2]), toLength = Integer.parseInt(args[3]);
		int maxVectors = Integer.parseInt(args[4]);
		String kind = args[5].toLowerCase();

		// the source lives in HBM for the walk (the reference reads it from disk vector by vector, :75-76)
		GpuLinear fromIndex = new GpuLinear(fromLength, maxVectors, true, fromFolder, true, true, 0);
		AbstractSearchStructure toIndex;
		if (kind.equals("small")) {
			toIndex = new GpuLinear(toLength, maxVectors, false, toFolder, true, true, 0);
		} else if (kind.equals("pq")) {
			GpuPQ pq = new GpuPQ(toLength, maxVectors, false, toFolder, Integer.parseInt(args[7]), Integer.parseInt(args[8]),
					transformation(args[9]), 512);
			pq.loadProductQuantizer(args[6]);
			toIndex = pq;
		} else if (kind.equals("ivfpq")) {
			GpuIVFPQ ivfpq = new GpuIVFPQ(toLength, maxVectors, false, toFolder, Integer.parseInt(args[7]),
					Integer.parseInt(args[8]), transformation(args[9]), Integer.parseInt(args[11]), 512);
			ivfpq.loadCoarseQuantizer(args[10]);
			ivfpq.loadProductQuantizer(args[6]);
			toIndex = ivfpq;
		} else {
			throw new Exception("Unsupported index transformation type!");
		}

		// normalisation mode 2: renormalise if and only if the vector was truncated (:118-120)
		int moved = fromIndex.reindexInto(new AbstractSearchStructure[] { toIndex }, 0, new int[] { 2 }, 0);
		System.out.println(moved + " vectors re-indexed, " + fromLength + " -> " + toLength + " (" + kind + ")");
		toIndex.close();
		fromIndex.close();
	}
}
