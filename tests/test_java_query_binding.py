"""CPU: the Java drop-in reads bounded traversal through the GPU query entry
points (textual, as tests/test_java_binding.py: no JDK here).

GpuBAMInputFormat hands bounded-traversal splits to GpuBAMRecordReader while
their planning stays the stock BAMInputFormat.filterByInterval
(BAMInputFormat.java:532-634); GpuBAMRecordReader.initialize has the three-way
branch of BAMRecordReader.java:170-183."""
import os
import re

from test_java_binding import JAVA, JNI, _natives, _strip_comments


def _src(name):
    return _strip_comments(open(os.path.join(JAVA, name)).read())


def _method(src, head):
    """The body of the method whose declaration starts with `head`."""
    i = src.index(head)
    j = src.index("{", i)
    depth, k = 1, j + 1
    while depth:
        depth += src[k] == "{"
        depth -= src[k] == "}"
        k += 1
    return src[j:k]


def test_reader_gate_admits_bounded_traversal():
    src = _src("GpuBAMInputFormat.java")
    gate = _method(src, "static boolean gpuEnabled(Configuration conf)")
    assert "!isBoundedTraversal" not in gate and "isBoundedTraversal" not in gate
    assert "GPU_ENABLE_PROPERTY" in gate and "nativeAvailable()" in gate
    reader = _method(src, "public RecordReader<LongWritable, SAMRecordWritable> createRecordReader(")
    assert "gpuEnabled(" in reader and "new GpuBAMRecordReader()" in reader and "isBoundedTraversal" not in reader


def test_get_splits_keeps_the_stock_planner_for_bounded_traversal():
    src = _src("GpuBAMInputFormat.java")
    body = _method(src, "public List<InputSplit> getSplits(List<InputSplit> splits, Configuration cfg)")
    m = re.search(r"if \(([^;]*)\) return super\.getSplits\(splits, cfg\);", body)
    assert m and "isBoundedTraversal(cfg)" in m.group(1) and "!isBoundedTraversal" not in m.group(1)
    # before any GPU planning
    assert body.index("super.getSplits(splits, cfg)") < body.index("addFileSplits(")


def test_reader_has_the_three_way_branch():
    src = _src("GpuBAMRecordReader.java")
    init = _method(src, "public void initialize(InputSplit spl, TaskAttemptContext tctx)")
    for s in ("BAMInputFormat.isBoundedTraversal(conf)", "BAMInputFormat.getIntervals(conf)",
              "BAMInputFormat.prepareQueryIntervals(", "getIntervalFilePointers()", "HbamNative.queryIntervals(",
              "HbamNative.queryUnmapped("):
        assert s in init, s
    assert init.index("getIntervalFilePointers() != null") < init.index("HbamNative.queryIntervals(") < \
        init.index("HbamNative.queryUnmapped(")
    assert "getStartOfLastLinearBin()" in src
    # batches of a bounded read come from the query, the others from the split
    batch = _method(src, "private void nextBatch()")
    assert "HbamNative.queryNext(" in batch and "HbamNative.decodeSpan(" in batch
    # no per-batch writable bytes and no read-ahead stream position in bounded mode
    assert "encode = !bounded &&" in src
    progress = _method(src, "public float getProgress()")
    assert progress.index("if (bounded)") < progress.index("HbamNative.readerPosition(")


def test_query_natives_and_their_jni_functions():
    natives = _natives()
    assert natives["queryIntervals"] == 3 and natives["queryUnmapped"] == 2 and natives["queryNext"] == 2
    jni = _strip_comments(open(JNI).read())
    for fn, call in (("queryIntervals", "hbam_query_intervals("), ("queryUnmapped", "hbam_query_unmapped("),
                     ("queryNext", "hbam_query_next(")):
        m = re.search(r"FN\(%s\)\([^)]*\)\s*\{" % fn, jni)
        assert m, fn
        assert call in jni[m.end():jni.index("JNIEXPORT", m.end())], fn
