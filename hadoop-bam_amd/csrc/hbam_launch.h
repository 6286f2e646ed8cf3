// hbam_launch.h -- host-callable launch wrappers for the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hbam_device.h"

namespace hbam {

struct ChainArgs {
  const uint8_t* u;
  const BlockInfo* blocks;
  uint64_t e_inf, e_true, p0, q_end;
  const uint64_t* dead;
  uint32_t ndead;
  int32_t n_ref;
  uint32_t k0, k1;
  int validate;            // reader mode: 0 SILENT, 1 LENIENT (decode structure only), 2 STRICT (SAMRecord.isValid)
  const int32_t* ref_len;  // n_ref reference lengths (nullptr: alignment-start bound not checked)
  // per-block scratch (indexed by k - k0)
  uint64_t *g, *x, *entry, *summary, *base;
  uint64_t* x2;        // parallel link: y (walk exits)
  void* scan_tmp;      // parallel link: hipcub temp storage
  size_t scan_bytes;
  uint32_t* cnt;
  int32_t* err;
  unsigned long long* need;
  // outputs
  uint64_t *rec_pos, *rec_voff;
  // lane-per-block walks + per-block record lists
  uint64_t* cand;       // first plausible record start per block
  uint64_t* force;      // re-walk requests (kNone = keep)
  uint32_t* wcnt;       // records listed per block
  uint16_t* list;       // kListCap u16 offsets (from ustart) per block
  uint32_t* counters;   // [0] hard link violations, [1] blocks to re-walk, [2] list overflow (zeroed per pass);
                        // [kChainCtr..]: cumulative path counters (zeroed once, hbam_chain_counters)
  // fused check + output (launch_rec_check_out)
  uint64_t* fuse_bad;    // = ~0: min (i << kFusedBadShift | records up to i's stop) over blocks that stop early
  uint32_t* fuse_flags;  // [0] first failing block = ~0
};
constexpr uint32_t kListCap = 2048;              // >= 65536 / 36 + 2: every reader-mode record start
constexpr uint64_t kForceEmpty = ~0ull - 1;      // force[]: the block holds no record start
// ChainArgs::counters words past the per-pass ones: written only on the rare
// paths they count, never zeroed after the buffer's allocation
constexpr uint32_t kChainCtr = 4;          // first cumulative word
constexpr uint32_t kChainCtrSearched = 4;  // blocks handed to k_rec_search (first candidate's walk failed)
constexpr uint32_t kChainCtrRewalked = 5;  // blocks the link check re-walks from a forced entry
constexpr uint32_t kChainCtrDropped = 6;   // stray walks the link check drops (kForceEmpty)
constexpr uint32_t kChainCtrWords = 8;     // the buffer's size in words

// launch_chain stages
enum ChainStage : int {
  kStageSerialLink = 1,  // exact serial link over the walk exits (entry[] + summary)
  kStageCount = 2,       // per-block count + validation by walking (list overflow path)
  kStageEmit = 3,        // per-block positions + voffs by walking (list overflow path)
  kStageWalkLane = 4,    // candidates (k_rec_cand) + lane-per-block walks: kStageWalk's result, the A/B of it
  kStageWalk = 5,        // candidates + walks, a wave per block (k_rec_walk_wave), then the search
  kStageLinkCheck = 6,   // max-scan link check with re-walk requests
  kStageRewalk = 7,      // re-walk the requested blocks (entries validated)
  kStageRewalkAll = 8,   // re-walk every block off the serial link's entry[]
};
// ---- hbam_locate.hip: BGZF block discovery
// candidates in [lo, hi); file + buf_base is the (aligned) device buffer start
hipError_t launch_bgzf_scan(const uint8_t* file, uint64_t buf_base, uint64_t lo, uint64_t hi, uint64_t* cand,
                            uint32_t cap, uint32_t* count, hipStream_t s);
// partial != 0: bytes past hi are not part of the window; a block cut by hi
// ends the range (verify: flags[2] = 1; walk: out[2..3] = its start, status OK)
hipError_t launch_bgzf_verify(const uint8_t* file, uint64_t lo, uint64_t hi, const uint64_t* cand, uint32_t n,
                              BlockInfo* blocks, uint32_t* flags, uint32_t partial, hipStream_t s);
hipError_t launch_bgzf_walk(const uint8_t* file, uint64_t lo, uint64_t hi, BlockInfo* blocks, uint32_t cap,
                            uint32_t* out, uint32_t partial, hipStream_t s);
// Anchored locate of [lo, hi), lo a block start, in nseg segments of seg bytes
// (per-segment scratch: anchor, exitp, cnt, offs).  res[0] != 0: declined (run
// the scan path); else res[1] = the blocks of the range, and
// launch_bgzf_seg_emit writes their n starts to out in file order.
hipError_t launch_bgzf_anchor_walk(const uint8_t* file, uint64_t lo, uint64_t hi, uint64_t seg, uint32_t nseg,
                                   uint32_t partial, uint64_t* anchor, uint64_t* exitp, uint32_t* cnt, uint32_t* offs,
                                   uint32_t* res, hipStream_t s);
hipError_t launch_bgzf_seg_emit(const uint8_t* file, const uint64_t* anchor, const uint32_t* cnt,
                                const uint32_t* offs, uint32_t nseg, uint32_t n, uint64_t* out, hipStream_t s);
// ustart = base + exclusive scan of ISIZE
hipError_t launch_block_ustart(BlockInfo* blocks, uint32_t n, uint64_t* tmp_isize, uint64_t* tmp_ustart,
                               void* scan_tmp, size_t* scan_bytes, uint64_t base, hipStream_t s);
hipError_t sort_u64(void* tmp, size_t* tmp_bytes, uint64_t* keys_in, uint64_t* keys_out, uint32_t n,
                    hipStream_t s);
hipError_t scan_u32_to_u64(void* tmp, size_t* tmp_bytes, const uint32_t* in, uint64_t* out, uint32_t n,
                           hipStream_t s);
// ---- hbam_kernels.hip: inflate phase A
// inflate phase A in two launches: the first DEFLATE block's header + tables
// of every block of a chunk (k_huff_tables), then the decode reading them
// (round 0: the header at each block's start; round r > 0: where decode
// round r-1 left the block kHuffPending)
hipError_t launch_huff_tables(const uint8_t* file, const BlockInfo* blocks, uint32_t b0, uint32_t nb,
                              uint8_t* tables, HuffTableInfo* tinfo, const HuffOut* hout, uint32_t round,
                              hipStream_t s);
// (defer: stop a block before its next DEFLATE header, kHuffPending, for
// the next round; the last round decodes every remaining header inline)
// Round 0, two launches: the lean instance over the chunk, then the fallback
// over the blocks it handed over.  A later round, three: the lean instance
// 128 lanes wide over the chunk, the 256-lane one over the blocks whose window
// the narrow stage does not hold, the fallback.  flist: the chunk's lists
// (huff_list_words(nb) words, the kHuffListHdr header words zeroed before
// round 0); pstats: kPathStatWords path counters.
hipError_t launch_inflate_huff_prebuilt(const uint8_t* file, const BlockInfo* blocks, uint32_t b0, uint32_t nb,
                                        uint64_t chunk_ustart, uint32_t* tokens, HuffOut* hout,
                                        const uint8_t* tables, const HuffTableInfo* tinfo, uint32_t round,
                                        uint32_t defer, uint32_t* flist, uint32_t* pstats, hipStream_t s);
// resident workgroups per CU the runtime reports for the lean instance
hipError_t huff_lean_occupancy(int* workgroups_per_cu);
// the same for the narrow instance, and the bytes of window its stage holds
hipError_t huff_narrow_occupancy(int* workgroups_per_cu, uint32_t* stage_cap_bytes);
// ---- hbam_inflate_lz77.hip: inflate phase B
hipError_t launch_inflate_lz77(const BlockInfo* blocks, uint32_t b0, uint32_t nb, uint64_t chunk_ustart,
                               const uint32_t* tokens, const HuffOut* hout, uint8_t* u, hipStream_t s);
// ---- hbam_chain.hip: the record chain
hipError_t launch_chain(const ChainArgs& a, int mode, int stage, hipStream_t s);
// a.cnt[i] = the records block i's list holds (0 off the chain): scanned into
// a.base, the offsets launch_rec_check_out writes at
hipError_t launch_list_counts(const ChainArgs& a, hipStream_t s);
// the record rules, long-cigar validation and output of the listed records
// (k_rec_check_out): cnt / err / need per block, outputs at a.base[i] (the
// scanned list counts), a.fuse_bad / a.fuse_flags as documented there; cap =
// the rec_pos / rec_voff / column capacity
hipError_t launch_rec_check_out(const ChainArgs& a, int mode, bool decode, const Columns& col, uint64_t cap,
                                hipStream_t s);
constexpr int kFusedBadShift = 40;
hipError_t link_scan_bytes(uint32_t nb, size_t* bytes);
hipError_t launch_first_error_hout(const HuffOut* hout, uint32_t b0, uint32_t nb, uint32_t* first, hipStream_t s);
hipError_t launch_records_after(const uint32_t* cnt, uint32_t nb, uint32_t k, uint32_t* flag, hipStream_t s);
hipError_t launch_first_error_i32(const int32_t* err, uint32_t nb, uint32_t* first, hipStream_t s);
hipError_t launch_truncate_counts(uint32_t* cnt, uint32_t nb, const uint32_t* cut, hipStream_t s);
// ---- hbam_records.hip: record output and the SAMRecordWritable codec
hipError_t launch_rec_decode(const uint8_t* u, const uint64_t* rec_pos, uint64_t n, const Columns& col,
                             hipStream_t s);
// .splitting-bai entries of records with global ordinals o0 .. o0+n-1
// (ordinals k*g - 1): ent[j] for the j-th such ordinal of the span
hipError_t launch_sbi_emit(const uint64_t* voff, uint64_t n, uint32_t g, uint64_t o0, uint64_t* ent, hipStream_t s);
// *out = the chain successor of the last of n records (p0 when n == 0)
// gate_* (optional): a speculative launch, skipped on the device unless
// *gate_bad == ~0 and *gate_need <= gate_e_inf (k_rec_check_out's verdict)
hipError_t launch_next_pos(const uint8_t* u, const uint64_t* rec_pos, uint64_t n, uint64_t p0, int mode,
                           uint64_t* out, hipStream_t s, const unsigned long long* gate_bad = nullptr,
                           const unsigned long long* gate_need = nullptr, uint64_t gate_e_inf = 0);
// drop-in batches: records [0, n) of a decoded span -> an export slot
// (ColLayout with rec_pos; positions rebased by base, dst_pos[n] = nbytes);
// m > 0: also batch-major column blocks of m records at `packed`
// (k_export_records)
hipError_t launch_export_records(const Columns& src, const uint64_t* src_pos, const Columns& dst, uint64_t* dst_pos,
                                 uint64_t n, uint64_t base, uint64_t nbytes, uint8_t* packed, uint64_t m,
                                 hipStream_t s);
// n bytes device -> page-locked host by a kernel (no copy engine)
hipError_t launch_readback(void* dst, const void* src, uint64_t n, hipStream_t s);
// dst <- the rests of a span's records [0, n) back to back (record i's at
// rest_off[i] - p0 - 36 (i + 1)); u = the stream rest_off indexes; dst holds
// the rests' total + 16 bytes, u is readable 32 bytes past the last rest
hipError_t launch_pack_rests(const uint8_t* u, const uint64_t* rest_off, const uint32_t* rest_len, uint64_t n,
                             uint64_t p0, uint8_t* dst, hipStream_t s);
// dst[i] <- *src[i], i < n <= kGatherMax (dst: page-locked host or device)
constexpr int kGatherMax = 8;
hipError_t launch_gather_u64(uint64_t* dst, const uint64_t* const* src, int n, hipStream_t s);
// out[0] ^= xor of keys (if keys), out[1] += sum of voffs, out[2..3] += the
// order-sensitive key / voff digests (see k_digest)
hipError_t launch_digest(const int64_t* keys, const uint64_t* voffs, uint64_t n, uint64_t* out, hipStream_t s);
// keys deferred by decode_record (rest > kLongHash bytes): one wave per record
hipError_t launch_long_hash(const uint8_t* u, const uint64_t* rec_pos, const Columns& col, hipStream_t s,
                            const unsigned long long* gate_bad = nullptr, const unsigned long long* gate_need = nullptr,
                            uint64_t gate_e_inf = 0);
// SAMRecordWritable.write of a span's records: u[p0, p0+nbytes) -> dst
// (16 B-aligned, room for nbytes rounded up to 16) + bin patches (refID < 0)
hipError_t launch_wr_encode(const uint8_t* u, uint64_t p0, uint64_t nbytes, const uint64_t* rec_pos,
                            const int32_t* ref_id, const uint16_t* bin, uint64_t n, uint8_t* dst, hipStream_t s);
// SAMRecordWritable.readFields of n framed values; *bad = min((i << 8) | status)
hipError_t launch_wr_decode(const uint8_t* buf, uint64_t len, const uint64_t* offs, uint64_t n, const Columns& col,
                            uint64_t* rec_pos, unsigned long long* bad, hipStream_t s);
// ---- hbam_sort.hip
// Sorted SAMRecordWritable.write of a span's records (hbam_sort.hip), n < 2^31 - 1.
// order: kSortKey = ascending signed key, kSortCoordinate = ascending
// (uint32 refID, pos + 1); both stable.
enum : int { kSortKey = 0, kSortCoordinate = 1 };
// temporary storage of the radix sort of n pairs and of the scan over n + 1 lengths
hipError_t sort_tmp_bytes(uint64_t n, size_t* bytes);
// perm[j] = the span index of the j-th record in sorted order (word, word_sorted:
// n u64; len: n u32 = the records' encoded lengths; iota, perm: n u32)
hipError_t launch_sort_perm(void* tmp, size_t tmp_bytes, const Columns& col, uint64_t n, int order, uint64_t* word,
                            uint64_t* word_sorted, uint32_t* len, uint32_t* iota, uint32_t* perm, hipStream_t s);
// doff[j] = the output start of the j-th sorted record, doff[n] = the output's bytes (slen, doff: n + 1 u64)
hipError_t launch_sort_offsets(void* tmp, size_t tmp_bytes, const uint32_t* len, const uint32_t* perm, uint64_t n,
                               uint64_t* slen, uint64_t* doff, hipStream_t s);
// dst[doff[j], doff[j + 1]) = record perm[j]'s bytes at u + rec_pos[perm[j]], indexBin
// 0 when its refID < 0; total = doff[n]; dst holds total rounded up to 16, u is
// readable 16 bytes past its last record
hipError_t launch_sort_gather(const uint8_t* u, const uint64_t* rec_pos, const int32_t* ref_id, const uint32_t* perm,
                              const uint64_t* doff, uint64_t n, uint64_t total, uint8_t* dst, hipStream_t s);
// k_sort_words alone: the sort words, encoded lengths and iota of n decoded records
hipError_t launch_sort_words(const Columns& col, uint64_t n, int order, uint64_t* word, uint32_t* len, uint32_t* iota,
                             hipStream_t s);
// ---- hbam_samtext.hip
// SAM text of a span's records (hbam_samtext.hip), n < 2^31 - 1: one line per
// record in batch order.  The reference names: ref_bytes back to back, name r =
// [ref_off[r], ref_off[r + 1]) (n_ref + 1 u32).
// temporary storage of the scan over n + 1 lengths
hipError_t sam_tmp_bytes(uint64_t n, size_t* bytes);
// head_len[i] = the bytes of line i up to and with the tab behind TLEN, llen[i]
// = the line's bytes (llen: n + 1 u64, the last 0); *bad (preset ~0) = the first
// record whose fields do not fit its rest or whose aux fields are malformed
hipError_t launch_sam_measure(const uint8_t* u, const uint64_t* rec_pos, const Columns& col, uint64_t n,
                              const uint32_t* ref_off, const uint8_t* ref_bytes, int32_t n_ref, uint32_t* head_len,
                              uint64_t* llen, unsigned long long* bad, hipStream_t s);
// doff = the exclusive sum of llen over n + 1 entries: the line starts, doff[n] = the text's bytes
hipError_t launch_sam_offsets(void* tmp, size_t tmp_bytes, const uint64_t* llen, uint64_t n, uint64_t* doff,
                              hipStream_t s);
// dst[doff[i], doff[i + 1]) = line i; total = doff[n]; dst is 16 B-aligned.  Only
// after a launch_sam_measure of the same records that left *bad = ~0.
hipError_t launch_sam_write(const uint8_t* u, const uint64_t* rec_pos, const Columns& col, uint64_t n,
                            const uint32_t* ref_off, const uint8_t* ref_bytes, int32_t n_ref,
                            const uint32_t* head_len, const uint64_t* doff, uint64_t total, uint8_t* dst,
                            hipStream_t s);
// ---- hbam_samparse.hip
// SAM text into BAM records (hbam_samparse.hip).  text: device, 16 B-aligned,
// zero from len up to the next multiple of 16 at least; every line ends in
// '\n' (the host appends the one a final last line lacks).
// the 4 KiB pieces of len text bytes (one workgroup and one count each)
uint64_t samp_pieces(uint64_t len);
// temporary storage of an exclusive sum over m u64 entries
hipError_t samp_scan_bytes(uint64_t m, size_t* bytes);
hipError_t launch_samp_scan(void* tmp, size_t tmp_bytes, const uint64_t* in, uint64_t m, uint64_t* out,
                            hipStream_t s);
// cnt[p] = the '\n's of piece p, cnt[samp_pieces(len)] = 0
hipError_t launch_samp_count(const uint8_t* text, uint64_t len, uint64_t* cnt, hipStream_t s);
// first = the exclusive sum of cnt; start[0] = 0, start[k + 1] = the byte behind the k-th '\n' (n + 1 u64)
hipError_t launch_samp_starts(const uint8_t* text, uint64_t len, const uint64_t* first, uint64_t* start,
                              hipStream_t s);
// The dictionary: dict_n names sorted as unsigned bytes (a prefix first), name j
// = dict_bytes[dict_off[j], dict_off[j + 1]), dict_idx[j] = its reference index.
// rlen[i] = the bytes of line i's record (rlen: n + 1 u64, the last 0); *bad
// (preset ~0) = line << 8 | field of the first malformed line (atomicMin: the
// lowest line, and its lowest field code; samp_field_name names it)
hipError_t launch_samp_measure(const uint8_t* text, const uint64_t* start, uint64_t n, const uint32_t* dict_off,
                               const uint8_t* dict_bytes, const int32_t* dict_idx, int32_t dict_n, uint64_t* rlen,
                               unsigned long long* bad, hipStream_t s);
// dst[roff[i], roff[i + 1]) = line i's record; roff = the exclusive sum of rlen.
// Only after a launch_samp_measure of the same text that left *bad = ~0.
hipError_t launch_samp_write(const uint8_t* text, const uint64_t* start, uint64_t n, const uint32_t* dict_off,
                             const uint8_t* dict_bytes, const int32_t* dict_idx, int32_t dict_n, const uint64_t* roff,
                             uint8_t* dst, hipStream_t s);
const char* samp_field_name(uint32_t field);
// ---- hbam_names.hip
// Queryname order (hbam_names.hip): the name = name_len bytes at base +
// name_pos, zero-extended and compared as unsigned bytes, then the tie word
// (2 * mate rank + secondary/supplementary, from the flag), then the input
// order.  An LSD radix sort over the name's 8-byte big-endian chunks.
enum : int { kSortQueryname = 3 };  // (2 is not an order)
constexpr uint32_t kNameChunks = 32;  // ceil(255 / 8): l_read_name is a byte
// the census buffer: two halves (OR-like words preset 0, AND-like words preset
// ~0) of kNameChunks chunk words, the tie word and the most / fewest chunks
constexpr uint32_t kNameCensusTie = kNameChunks, kNameCensusChunks = kNameChunks + 1;
constexpr uint32_t kNameCensusHalf = kNameChunks + 2, kNameCensusWords = 2 * kNameCensusHalf;
struct NameOrderStats {
  uint64_t chunks_present = 0;  // the most chunks of a name
  uint64_t chunks_sorted = 0;   // chunk indices in which the names differ: one radix sort each
  uint64_t bits_sorted = 0;     // the bits those sorts cover (the tie word's pass is not counted)
};
// device -> host copy of `bytes` that has landed when it returns (Pipeline::rb + rb_sync)
typedef hipError_t (*NameReadback)(void* ctx, void* dst, const void* src, size_t bytes, hipStream_t s);
// name_pos = rec_pos + 36, name_len = min(l_read_name, rest_len), tie = the flag's tie word, of n decoded
// records; len (nullptr or n u32) = their encoded lengths, 36 + rest_len
hipError_t launch_name_refs(const uint64_t* rec_pos, const Columns& col, uint64_t n, uint64_t* name_pos,
                            uint8_t* name_len, uint8_t* tie, uint32_t* len, hipStream_t s);
// perm[j] = the index of the j-th record in queryname order.  tmp: sort_tmp_bytes(n);
// word, word2: n u64; scratch, perm: n u32; census: kNameCensusWords u64.  Every
// aligned 8-byte word that holds a byte of a name must be readable.
// Measurement: full = sort every chunk present over all 64 bits (the census
// still runs; the order is the same); after_census / after_tie (or nullptr) are
// recorded behind the census read-back and behind the tie word's pass.
hipError_t launch_name_order(void* tmp, size_t tmp_bytes, const uint8_t* base, const uint64_t* name_pos,
                             const uint8_t* name_len, const uint8_t* tie, uint64_t n, uint64_t* word,
                             uint64_t* word2, uint32_t* scratch, uint32_t* perm, uint64_t* census,
                             NameReadback rb, void* rb_ctx, NameOrderStats* stats, hipStream_t s, bool full = false,
                             hipEvent_t after_census = nullptr, hipEvent_t after_tie = nullptr);
// *bad (preset ~0) = min over the records i > 0 whose (name, tie) is below record i - 1's
hipError_t launch_name_sorted(const uint8_t* base, const uint64_t* name_pos, const uint8_t* name_len,
                              const uint8_t* tie, uint64_t n, unsigned long long* bad, hipStream_t s);
// at = the exclusive sum of name_len over n + 1 entries (at[n] = the names' bytes); len64, at: n + 1 u64
hipError_t launch_name_starts(void* tmp, size_t tmp_bytes, const uint8_t* name_len, uint64_t n, uint64_t* len64,
                              uint64_t* at, hipStream_t s);
// the names copied back to back: dst[dst_base + at[i] ..) = the name at src + name_pos[i]; name_pos[i] = dst_base + at[i]
hipError_t launch_name_pack(const uint8_t* src, uint64_t* name_pos, const uint8_t* name_len, const uint64_t* at,
                            uint64_t n, uint8_t* dst, uint64_t dst_base, hipStream_t s);
// ---- hbam_merge.hip
// Merge of k sorted runs of SAMRecordWritable encodings (hbam_merge.hip), total
// records n < 2^31 - 1.  A record's global index is run-major: run_base[r] + i
// (run_base: k + 1 u64).  Every run's n_r + 1 offsets lie back to back in one
// array, run r's at run_base[r] + r.
constexpr uint64_t kMergeMinRecord = 36;  // block_size + the fixed fields
// temporary storage of the radix sort of n pairs and of the scans over n + 1 entries
hipError_t merge_tmp_bytes(uint64_t n, size_t* bytes);
// one run: rlen[i] = offs[i + 1] - offs[i]; bad[0] = the first record whose
// framing is not an increasing pair >= kMergeMinRecord apart inside len,
// bad[1] = the first record whose word is below its predecessor's (word ==
// nullptr: not checked); both preset to ~0 by the caller
hipError_t launch_merge_check(const uint64_t* offs, uint64_t n, uint64_t len, const uint64_t* word, uint32_t* rlen,
                              unsigned long long* bad, hipStream_t s);
// perm[j] = the global index of the j-th output record (stable; idx: n u32 of scratch)
hipError_t launch_merge_perm(void* tmp, size_t tmp_bytes, const uint64_t* word, uint64_t* word_sorted, uint32_t* idx,
                             uint32_t* perm, uint64_t n, hipStream_t s);
// flag[j] = output record j starts a part (doff[j] / part_bytes differs from
// its predecessor's), num = the exclusive sum of flag over n + 1 entries: num[n] = the parts
hipError_t launch_merge_heads(void* tmp, size_t tmp_bytes, const uint64_t* doff, uint64_t n, uint64_t part_bytes,
                              uint32_t* flag, uint32_t* num, hipStream_t s);
// part_first / part_start (parts + 1 entries: the first record / output byte of
// each part, the last = n / doff[n]), rank (n u32: the inverse of perm) and
// cut[p * k + r], p <= parts: the records of run r before part p; cut_off = the
// offset in run r at which they end (off: the runs' offsets as described above)
hipError_t launch_merge_cuts(const uint32_t* flag, const uint32_t* num, const uint64_t* doff, const uint32_t* perm,
                             uint64_t n, const uint64_t* run_base, uint32_t k, uint64_t parts, uint32_t* part_first,
                             uint64_t* part_start, uint32_t* rank, const uint64_t* off, uint32_t* cut,
                             uint64_t* cut_off, hipStream_t s);
// one part of n records (perm, doff: its first entries; dbase = doff[0]):
// src_pos[j] = slice_base[run] + the record's offset in its run, src_id[j] =
// run << 32 | record, part_offs[j] = doff[j] - dbase (n + 1 entries)
hipError_t launch_merge_src(const uint32_t* perm, const uint64_t* doff, uint64_t n, uint64_t dbase,
                            const uint64_t* run_base, uint32_t k, const uint64_t* off, const uint64_t* slice_base,
                            uint64_t* src_pos, uint64_t* src_id, uint64_t* part_offs, hipStream_t s);
// dst[doff[j] - dbase, doff[j + 1] - dbase) = the bytes at u + src_pos[j]
// (k_sort_gather without perm and bin patch); total = doff[n] - dbase; dst holds
// total rounded up to 16, u is readable 16 bytes past its last record
hipError_t launch_merge_gather(const uint8_t* u, const uint64_t* src_pos, const uint64_t* doff, uint64_t n,
                               uint64_t dbase, uint64_t total, uint8_t* dst, hipStream_t s);

}  // namespace hbam
