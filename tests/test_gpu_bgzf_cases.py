"""The BGZF write path on the GPU (k_deflate_blocks + k_dfl_crc + k_dfl_frame)
against zlib on the inputs of bgzf_cases.py: several lanes of one wave at work
(more than 5,120 blocks in a batch), zlib's rare encoder paths, every CRC regime
at every payload alignment, and levels 7 and 8.  test_bgzf_cases.py shows, from
zlib's output alone, that each input reaches the path it is named for, and runs
the host build of the same code on all but W."""
import pytest

import bgzf_cases as bc


def first_difference(got, want, block_lens):
    """Where two BGZF files part: the block (by want's framing) and the byte in it."""
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    p, blk = 0, 0
    while p + 18 <= len(want):
        bs = int.from_bytes(want[p + 16:p + 18], "little") + 1
        if k < p + bs:
            break
        p += bs
        blk += 1
    n = block_lens[blk] if blk < len(block_lens) else 0  # past the list: the EOF block
    part = "header" if k - p < 18 else "cdata" if k - p < bs - 8 else "crc32" if k - p < bs - 4 else "isize"
    return ("sizes %d / %d; first difference at byte %d = block %d (payload %d bytes), byte %d of its %d (%s)"
            % (len(got), len(want), k, blk, n, k - p, bs, part))


def check(name, level):
    import hbam
    c = bc.get(name)
    want = bc.want(name, level)
    got = hbam.bgzf_compress(c.payload, block_lens=c.block_lens, level=level, eof=True)
    assert got == want, "%s level %d: %s" % (name, level, first_difference(got, want, c.block_lens))


@pytest.mark.gpu
@pytest.mark.parametrize("name,level", bc.params(bc.SMALL))
def test_gpu_matches_zlib(name, level):
    check(name, level)


@pytest.mark.gpu
@pytest.mark.parametrize("name,level", bc.params(["W1", "W2"]))
def test_gpu_matches_zlib_with_shared_waves(name, level, monkeypatch):
    """One batch: 2 (W1) and 3 (W2) live lanes per wave, the last wave with one."""
    monkeypatch.delenv("HBAM_DFL_MAX_LANES", raising=False)
    check(name, level)


@pytest.mark.gpu
def test_gpu_second_batch_reuses_the_arenas(monkeypatch):
    """5,121 arenas for 5,421 blocks: a first batch at 2 lanes per wave, then
    300 blocks over arenas and slots that hold the first batch's state."""
    monkeypatch.setenv("HBAM_DFL_MAX_LANES", "5121")
    check("W1", 5)
    check("W1b", 5)


def test_first_difference_names_block_and_byte():
    want = bc.want("R", 1)
    lens = bc.get("R").block_lens
    first = int.from_bytes(want[16:18], "little") + 1
    bad = bytearray(want)
    bad[first + 20] ^= 1
    assert "= block 1 (payload 259 bytes), byte 20 of" in first_difference(bytes(bad), want, lens)
    assert "(cdata)" in first_difference(bytes(bad), want, lens)
    assert "block 20 (payload 0 bytes), byte 0" in first_difference(want[:-28], want, lens)
