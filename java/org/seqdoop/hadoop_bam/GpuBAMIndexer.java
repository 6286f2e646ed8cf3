// Copyright (c) the hadoop-bam_amd authors.  MIT license (as Hadoop-BAM).
//
// The BAM index (.bai, SAM spec 5.2) of a coordinate-sorted BAM, computed on
// the MI355X (hbam_build_bai): the file is streamed through HBM window by
// window and every record's bin, chunk and 16 kbp windows come out of the
// kernels.  Hadoop-BAM has no class of this kind (its users index with
// htsjdk's BAMIndexer or samtools); this one closes the loop for the GPU
// path: with the .bai it writes, BAMInputFormat.setIntervals (-L) and the BAI
// split calculator need no index made elsewhere.
//
// The index follows the SAM specification; it is not claimed to be
// byte-identical to the file htsjdk's BAMIndexer writes for the same BAM.
//
//   createIndex(bam, out, conf)   the .bai of bam written to out, with the
//       metadata pseudo-bins unless hadoopbam.gpu.bai-metadata is false
//   main(BAM files...)            each file indexed into file + ".bai"
//
// Not compiled in this repository (no JDK in the build image).
package org.seqdoop.hadoop_bam;

import java.io.IOException;
import java.io.OutputStream;
import org.apache.hadoop.conf.Configuration;
import org.apache.hadoop.fs.Path;
import org.seqdoop.hadoop_bam.gpu.HbamFiles;
import org.seqdoop.hadoop_bam.gpu.HbamNative;

public final class GpuBAMIndexer {
  public static final String OUTPUT_FILE_EXTENSION = ".bai";
  /** false: leave out the pseudo-bins 37450 and the count of records without coordinates. */
  public static final String METADATA_PROPERTY = "hadoopbam.gpu.bai-metadata";

  private GpuBAMIndexer() {}

  /**
   * Writes the index of bam (a file of any of conf's file systems) to out
   * (created or overwritten).  The records are validated under the configured
   * stringency, as a read of the file is.
   *
   * @throws htsjdk.samtools.SAMFormatException if bam is not coordinate-sorted
   */
  public static void createIndex(final Path bam, final Path out, final Configuration conf) throws IOException {
    final byte[] index;
    try (HbamFiles.Handle h = HbamFiles.open(bam, conf, GpuBAMRecordReader.device(conf),
                                             GpuBAMRecordReader.stringencyCode(GpuBAMRecordReader.stringencyOf(conf)),
                                             conf.getLong(GpuBAMRecordReader.WINDOW_BYTES_PROPERTY, 0L))) {
      index = HbamNative.buildBai(h.ctx, conf.getBoolean(METADATA_PROPERTY, true));
    }
    try (OutputStream os = out.getFileSystem(conf).create(out, true)) {
      os.write(index);
    }
  }

  public static void main(String[] args) {
    if (args.length == 0) {
      System.out.println("Usage: GpuBAMIndexer [BAM files...]\n\n"
                         + "Writes the BAM index of each coordinate-sorted BAM file into [filename].bai.");
      return;
    }
    final Configuration conf = new Configuration();
    for (final String arg : args) {
      final Path bam = new Path(arg);
      System.out.printf("Indexing %s...", bam);
      try {
        createIndex(bam, bam.suffix(OUTPUT_FILE_EXTENSION), conf);
        System.out.println(" done.");
      } catch (IOException | RuntimeException e) {
        System.out.println(" FAILED!");
        e.printStackTrace();
      }
    }
  }
}
