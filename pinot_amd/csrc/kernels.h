// kernels.h — the host-callable launchers of kernels.hip and derive.hip. host.cpp and both definition files
// include this, so the compiler checks each definition against the one declaration.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "device_types.h"

namespace pamd {
// kernels.hip
hipError_t launch_init_acc(uint64_t* d_acc, const DevQuery& q, int64_t num_keys, hipStream_t st);
hipError_t launch_sext_hi(uint64_t* d_acc, int64_t n, const int32_t* arrs, int32_t narr, hipStream_t st);
hipError_t launch_raw_int_minmax(const uint8_t* be, int type, int64_t n, long long* out, hipStream_t st);
hipError_t launch_fingerprint(const void* p, size_t bytes, unsigned long long* out, hipStream_t st);
hipError_t launch_for_pack(const uint8_t* be, int type, int64_t n, unsigned long long base, int lo_bits, int hi_bits,
                           uint8_t* lo, uint8_t* hi, hipStream_t st);
hipError_t launch_trim(const unsigned long long* keys, int64_t cap, int nw_seg, const uint64_t* acc, int fd_acc,
                       int32_t nsegs, int64_t limit, const int64_t* bucket_base, uint32_t* hist,
                       unsigned long long* seg_distinct, int64_t* bstar, int64_t* rank, unsigned long long* bitmap,
                       int64_t* dstar, unsigned long long* limit_reached, hipStream_t st);
hipError_t launch_hash_merge(const unsigned long long* skeys, int64_t scap, int nw, int has_seg, const uint64_t* sacc,
                             unsigned long long* fkeys, int64_t fcap, uint64_t* facc, const DevQuery& q, int fd_acc,
                             const int64_t* dstar, unsigned long long* overflow, hipStream_t st,
                             const SegSelStage* sst = nullptr, int nst = 0, const int32_t* sdone = nullptr,
                             const uint64_t* scut = nullptr);
hipError_t launch_segsel(const unsigned long long* keys, int64_t cap, int nw, const uint64_t* acc, int fd_acc,
                         const int64_t* dstar, const DevQuery& q, const SegSelStage* sst, int nst, int32_t nsegs,
                         int64_t keep, unsigned long long* cnt, int64_t* want, int32_t* done, uint64_t* prefix,
                         uint64_t* cut, uint32_t* hist, hipStream_t st);
hipError_t launch_admit(uint32_t* first, int64_t nk, const uint32_t* seen, const unsigned long long* seen_n, int64_t cap,
                        int32_t nsegs, int64_t limit, const int64_t* bucket_base, int64_t max_buckets, uint32_t* hist,
                        int64_t* bstar, int64_t* rank, unsigned long long* bitmap, int64_t* dstar,
                        unsigned long long* limit_reached, int phase, uint32_t* admit, int64_t words, hipStream_t st);
hipError_t launch_presence_bitset(const uint64_t* count, int64_t n, unsigned long long* bits, hipStream_t st);
hipError_t launch_seg_cut(const unsigned long long* bits, int64_t words, int32_t nsegs, int64_t limit,
                          unsigned long long* cut, hipStream_t st);
hipError_t launch_spill_direct_prep(const int64_t* offs, const int64_t* part_begin, const uint32_t* hist, int P,
                                    int64_t grid, int64_t* dbase, uint32_t* dcnt, int64_t* pbeg, hipStream_t st);
hipError_t launch_spill_agg(const DevHash& H, int nw, const unsigned long long* sorted, const int64_t* part_begin,
                            const DevQuery& q, uint64_t* acc, int agg_grid, int S, uint32_t narrow, hipStream_t st);
hipError_t launch_spill_passes(const DevHash& H, int nw, int64_t grid, const uint32_t* hist_unused, int64_t* offs,
                               int64_t* part_begin, unsigned long long* sorted, const DevQuery& q, uint64_t* acc,
                               int agg_grid, int S, int sorted_scatter, uint32_t narrow, hipStream_t st);
hipError_t launch_gather_groups(const int32_t* slots, int64_t ngroups, const unsigned long long* keys, int nw,
                                int64_t cap, const uint64_t* acc, int32_t nacc, uint64_t* out_keys, uint64_t* out_acc,
                                hipStream_t st);
hipError_t launch_export_groups(const int32_t* slots, int64_t ngroups, const unsigned long long* hkeys, int64_t cap,
                                const uint64_t* acc, int32_t nacc_out, const DevKeyPack& kp, uint64_t* out_keys,
                                uint64_t* out_acc, hipStream_t st);
hipError_t launch_merge_rows(const uint64_t* keys, const uint64_t* acc, int64_t n, int nw, int nacc_in,
                             unsigned long long* fkeys, int64_t fcap, uint64_t* facc, const DevQuery& q,
                             unsigned long long* overflow, hipStream_t st);
hipError_t launch_distinct_fold_count(const uint64_t* ckeys, int64_t nrows, const DevKeyPack& kc, const DevKeyPack& kb,
                                      const uint64_t* bkeys, int64_t nbase, int cbits, uint32_t* cnt, uint64_t* pair,
                                      unsigned long long* miss, hipStream_t st);
hipError_t launch_hll_fold(const uint64_t* ckeys, const uint64_t* cacc, int nacc, int acc_word, int64_t nrows,
                           const DevKeyPack& kc, const DevKeyPack& kb, const uint64_t* bkeys, int64_t nbase, int log2m,
                           uint8_t* regs, unsigned long long* sz, unsigned long long* miss, unsigned long long* bad,
                           hipStream_t st);
hipError_t launch_distinct_fold_fill(const uint64_t* sorted, int64_t nrows, int cbits, const uint32_t* cnt, int64_t nbase,
                                     int64_t* off, int32_t* values, hipStream_t st);
hipError_t launch_value_count_scan(const uint64_t* counts, int64_t n, int64_t* bsum, int64_t* cum, hipStream_t st);
hipError_t launch_percentile_select(const int64_t* off, const int64_t* cum, const int32_t* values, int64_t ngroups,
                                    const double* pct, int np, int32_t* out, hipStream_t st);
int64_t distinct_fold_sum_tiles(int64_t nrows);
hipError_t launch_distinct_fold_sum(const uint64_t* sorted, int64_t nrows, int cbits, const int64_t* off, int64_t nbase,
                                    const double* dictd, const int64_t* dicti, double* sumd, uint64_t* sumi,
                                    double* partd, uint64_t* parti, hipStream_t st);
hipError_t launch_read_dict_ids(const uint8_t* packed, int bits, int64_t start, int64_t len, int32_t* out,
                                hipStream_t st);
hipError_t launch_pack_dict_ids(const int32_t* values, int64_t n, int bits, uint8_t* packed, hipStream_t st);
hipError_t launch_read_raw(const uint8_t* raw, int type, int64_t start, int64_t len, uint8_t* out, hipStream_t st);
hipError_t launch_chunk_decompress(const uint8_t* src, uint8_t* dst, const void* jobs, int32_t njobs, int32_t* status,
                                   hipStream_t st);
hipError_t launch_bitset_binop(const uint64_t* a, const uint64_t* b, uint64_t* out, int64_t n, int op,
                               hipStream_t st);
hipError_t launch_bitset_not(const uint64_t* a, uint64_t* out, int64_t num_docs, hipStream_t st);
int64_t compact_num_chunks(int64_t num_docs);
hipError_t launch_bitset_count(const uint64_t* bits, int64_t num_docs, int64_t* d_chunk_counts, int64_t* d_total,
                               hipStream_t st);
hipError_t launch_bitset_compact(const uint64_t* bits, int64_t num_docs, const int64_t* d_chunk_offsets,
                                 int32_t* out, hipStream_t st);
// ... stopped at the first `limit` set bits (out holds min(limit, set bits) ascending indices)
hipError_t launch_bitset_compact_limit(const uint64_t* bits, int64_t num_bits, const int64_t* d_chunk_offsets,
                                       int64_t limit, uint32_t* out, hipStream_t st);
hipError_t launch_expand_jobs(const void* d_jobs, int32_t njobs, int64_t total_items, hipStream_t st);
hipError_t launch_roaring_select(const void* d_jobs, const void* d_fs, int32_t nfs, int64_t total_items, const void* d_segs,
                                 int32_t nleaves, int32_t nclauses, unsigned long long* sel_entries,
                                 unsigned long long* sel_count, int64_t sel_cap, unsigned long long* matched_out, int clause,
                                 hipStream_t st);
hipError_t launch_pack_sel(const void* conts, const int32_t* sel, int64_t n, int group, unsigned long long* out,
                           hipStream_t st);
int expand_group();
hipError_t launch_partition_offsets(const uint32_t* d_hist, int32_t nparts, int64_t nblocks, int64_t* d_offs,
                                    int64_t* d_part_begin, hipStream_t st);
hipError_t launch_allot_prefix(const uint32_t* d_hist, int32_t P, int64_t G, int mode, int64_t stride, double scale,
                               int64_t limit, int64_t* d_ptot, int64_t* d_out, hipStream_t st);
hipError_t launch_selection_count(const uint64_t* sorted, int W, int64_t n, int64_t K, int32_t nsegs, uint32_t* cnt,
                                  hipStream_t st);
hipError_t launch_selection_cut(const uint64_t* sorted, int W, int64_t n, int64_t K, int32_t nsegs, const int64_t* off,
                                int64_t total, uint32_t* out_seg, uint32_t* out_doc, hipStream_t st);
hipError_t launch_selection_gather(const SelCol* cols, int32_t ncols, const uint32_t* row_seg, const uint32_t* row_doc,
                                   int64_t nrows, int64_t* out, hipStream_t st);
// dict_regex_match_kernel: one STRING dictionary of a batch. bytes: the values' UTF-8 bytes concatenated in dictId
// order (dword-aligned, pinot_amd_required_padding() bytes of slack behind them); offs: card + 1 byte offsets
struct DevRegexDict {
  const uint32_t* bytes;
  const int32_t* offs;
  int64_t first_wave;  // waves (64 values each) of the descriptors before this one
  int64_t out_word0;   // this dictionary's first 64-bit word in the mask buffer (one word per wave)
  int32_t card, pad;
};
// dfa_words: the 256-byte class map, then the table's uint16 row offsets (regex_dfa.h), padded to a dword
hipError_t launch_dict_regex_match(const DevRegexDict* d_descs, int32_t ndesc, int64_t total_waves,
                                   const uint32_t* d_dfa_words, int32_t dfa_nwords, int32_t num_classes, uint32_t start,
                                   unsigned long long* d_masks, hipStream_t st);

// derive.hip
// A GROUP BY key transform as the transform kernel takes it (by value): pinot_amd_key_transform_spec after
// validation, the granularity already in milliseconds. Units are java.util.concurrent.TimeUnit ordinals.
struct DevKeyTransform {
  int32_t kind;        // pinot_amd_key_transform
  int32_t trunc_unit;  // pinot_amd_trunc_unit (DATETRUNC)
  int32_t in_unit, out_unit;
  int32_t gran_unit;   // DATETIMECONVERT: the granularity's unit when its size is 1 (a constant divisor), else -1
  int64_t in_size, out_size;
  int64_t gran_ms;     // DATETIMECONVERT: G.toMillis(g) > 0
};
// how derive_dictionary's source values are stored
enum DeriveSource { DERIVE_SRC_BE = 0 /* staged raw column: big-endian values of `type` */,
                    DERIVE_SRC_LE64 = 1 /* int64 in host order (a dictionary's values) */ };
size_t derive_dictionary_scratch(int64_t n);
hipError_t derive_dictionary(const uint8_t* d_src, int type, int src, const DevKeyTransform* tf, int64_t n,
                             void* d_scratch, int32_t* d_ids, uint8_t* d_dict_be, int64_t* h_card, hipStream_t st);
hipError_t launch_remap_dict_ids(int32_t* ids, int64_t n, const int32_t* map, int64_t card, hipStream_t st);
hipError_t launch_sorted_dict_ids(const int32_t* starts, int64_t card, int64_t n, const int32_t* map, int32_t* ids,
                                  hipStream_t st);
// DISTINCTCOUNTHLL twins (hll_hash_kernel): how the n values to hash are stored
enum HllSource { HLL_SRC_BE32 = 0 /* staged raw INT / FLOAT */, HLL_SRC_BE64 = 1 /* staged raw LONG / DOUBLE */,
                 HLL_SRC_LE64 = 2 /* an INT / LONG dictionary as int64, a DOUBLE one as doubles, host order */,
                 HLL_SRC_LE64_F32 = 3 /* a FLOAT dictionary as doubles */,
                 HLL_SRC_STRING = 4 /* a STRING dictionary's bytes, offs its n + 1 byte offsets */ };
hipError_t launch_hll_hash(const void* src, const int32_t* offs, int src_kind, int64_t n, int log2m, int32_t* idx,
                           int32_t* rank, hipStream_t st);
// Multi-value columns. A staged dictionary-encoded MV forward index (FixedBitMVForwardIndexWriter's file, all
// big-endian): `words` is the 4-byte aligned file; the start-bit bitmap begins at dword bm_word0 (MSB-first, bit i
// set = value i starts a doc), the fixed-bit dictId stream at bit raw_bit0 of the file. tile_first_doc[t] = start bits
// before value t * kMvTileValues: the only derived index.
constexpr int kMvTileValues = 4096;
struct DevMvColumn {
  const uint32_t* words;
  int64_t bm_word0, raw_bit0;
  int64_t num_values, num_docs;
  const int32_t* tile_first_doc;
  int32_t bits, pad;
};
// An ANY-match predicate's resolved dictId set
enum : int32_t { MV_SET_RANGE = 0 /* lo <= dictId < hi */, MV_SET_ACCEPT = 1 /* bit dictId of accept, card <= 64 */,
                 MV_SET_LDS = 2 /* bit dictId of set, staged in LDS */, MV_SET_HBM = 3 /* ... read in place */ };
struct DevMvSet {
  int32_t mode, set_words;
  int64_t lo, hi, card;
  uint64_t accept;
  const uint32_t* set;
};
enum : int32_t { MV_RED_COUNT = 0, MV_RED_SUM_I64 = 1, MV_RED_SUM_F64 = 2, MV_RED_MIN = 3, MV_RED_MAX = 4 };
int64_t mv_num_tiles(int64_t num_values);
// tile_first_doc: mv_num_tiles(num_values) entries (at least one allocated); total[0] = the bitmap's popcount
hipError_t launch_mv_index(const DevMvColumn& c, int32_t* tile_first_doc, long long* total, hipStream_t st);
// flags |= 1: bit 0 unset, 4: a chunk offset header entry disagrees with the bitmap's rank, 8: a doc longer than
// max_values
hipError_t launch_mv_validate(const DevMvColumn& c, int32_t docs_per_chunk, int32_t num_chunks, int32_t max_values,
                              uint32_t* flags, hipStream_t st);
hipError_t launch_mv_read(const DevMvColumn& c, int32_t* offsets, int32_t* ids, hipStream_t st);
// ORs the docs with a matching value into `bitset` (32-bit words of the dense docId bitset, zeroed by the caller)
hipError_t launch_mv_match(const DevMvColumn& c, const DevMvSet& s, uint32_t* bitset, hipStream_t st);
// one word per doc (mv_reduce_kernel); dict: the column's little-endian dictionary of `type`
hipError_t launch_mv_reduce(const DevMvColumn& c, const void* dict, int type, int op, unsigned long long* out,
                            hipStream_t st);
size_t sort_rows_scratch(int64_t n);
hipError_t sort_rows_by_key(const uint64_t* keys, int nwk, const int* word_bits, const uint64_t* acc, int nacc, int64_t n,
                            void* scratch, uint64_t* keys_out, uint64_t* acc_out, hipStream_t st);
}  // namespace pamd
