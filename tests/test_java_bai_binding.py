"""CPU: the Java side of the BAM index entry points (textual, as
tests/test_java_query_binding.py: no JDK here): the natives buildBai,
baiSummary and baiQuery with their JNI functions, each calling its hbam_* entry
point, and GpuBAMIndexer's createIndex and main."""
import os
import re

from test_java_binding import JAVA, JNI, _natives, _public_signatures, _strip_comments
from test_java_query_binding import _method, _src


def test_bai_natives_and_their_jni_functions():
    natives = _natives()
    assert natives["buildBai"] == 2 and natives["baiSummary"] == 1 and natives["baiQuery"] == 2
    jni = _strip_comments(open(JNI).read())
    for fn, call in (("buildBai", "hbam_build_bai("), ("baiSummary", "hbam_bai_summarize("),
                     ("baiQuery", "hbam_bai_query(")):
        m = re.search(r"FN\(%s\)\([^)]*\)\s*\{" % fn, jni)
        assert m, fn
        body = jni[m.end():jni.index("JNIEXPORT", m.end())]
        assert call in body, fn
        # the library's buffers go back to it; the ctx-less calls report through hbam_last_error(NULL)
        if fn != "baiSummary":
            assert "hbam_free(" in body, fn
        assert ("hbam_last_error(CTX(h))" if fn == "buildBai" else "hbam_last_error(NULL)") in body, fn
    native_src = _strip_comments(open(os.path.join(JAVA, "gpu", "HbamNative.java")).read())
    assert "public static native byte[] buildBai(long ctx, boolean metadata)" in native_src
    assert "public static native long[] baiSummary(byte[] bai)" in native_src
    assert "public static native long[] baiQuery(byte[] bai, int[] intervals)" in native_src


def test_gpu_bam_indexer_surface():
    src = _src("GpuBAMIndexer.java")
    assert "package org.seqdoop.hadoop_bam;" in src and "public final class GpuBAMIndexer" in src
    have = _public_signatures(src)
    assert ("createIndex", ("Path", "Path", "Configuration")) in have
    assert ("main", ("String[]",)) in have
    assert "public static void createIndex(final Path bam, final Path out, final Configuration conf)" in src
    body = _method(src, "public static void createIndex(")
    assert "HbamFiles.open(bam, conf" in body and "HbamNative.buildBai(h.ctx" in body
    assert body.index("HbamNative.buildBai(") < body.index(".create(out")  # nothing is written when the build fails
    assert "createIndex(" in _method(src, "public static void main(String[] args)")


def test_input_format_planning_is_untouched():
    # bounded traversal keeps the stock planner in the drop-in (tests/test_java_query_binding.py pins it)
    src = _src("GpuBAMInputFormat.java")
    assert "baiQuery" not in src and "buildBai" not in src
