/*
 * pinot_amd.h — C ABI of the MI355X segment-execution library (libpinot_amd.so).
 *
 * This is the drop-in boundary for Pinot's server-side segment execution hot path:
 * forward-index scan, filter (scan + inverted index), aggregation, group-by and selection
 * (SELECT columns [ORDER BY ...] LIMIT n) over immutable segments staged in HBM. Every entry point takes plain pointers and sizes
 * (no torch or Java types), so a JNI / Panama FFM binding in pinot-core can call it
 * directly; INTEGRATION.md shows the Java-side binding.
 *
 * Each entry point names the reference interface it replaces (paths relative to the
 * reference checkout root; "core" = pinot-core/src/main/java/org/apache/pinot/core,
 * "local" = pinot-segment-local/src/main/java/org/apache/pinot/segment/local).
 *
 * Conventions
 *   - Return value: 0 on success, a negative PINOT_AMD_E* code on failure; the message is
 *     available from pinot_amd_last_error() (thread-local). Invalid arguments fail loudly;
 *     nothing falls back to a CPU path.
 *   - "stream" is a hipStream_t passed as void* (NULL = the null stream). Calls that
 *     return results to host memory synchronise that stream.
 *   - Device pointers are marked d_. Host pointers are marked h_.
 */
#ifndef PINOT_AMD_H
#define PINOT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PINOT_AMD_ABI_VERSION 1

/* error codes */
#define PINOT_AMD_OK 0
#define PINOT_AMD_EINVAL (-1)     /* bad argument (IllegalArgumentException / IllegalStateException) */
#define PINOT_AMD_EUNSUPPORTED (-2) /* format or query shape not supported by this build */
#define PINOT_AMD_EHIP (-3)       /* HIP runtime error */
#define PINOT_AMD_ENOMEM (-4)     /* device allocation failed */
#define PINOT_AMD_EOVERFLOW (-5)  /* result capacity exceeded */

/* FieldSpec.DataType stored types on the path (pinot-spi/.../data/FieldSpec.java) */
enum pinot_amd_data_type { PINOT_AMD_INT = 0, PINOT_AMD_LONG = 1, PINOT_AMD_FLOAT = 2, PINOT_AMD_DOUBLE = 3,
                           PINOT_AMD_STRING = 4 };

/* Forward-index encodings (local/segment/index/forward/ForwardIndexReaderFactory.java:75-115) */
enum pinot_amd_fwd_encoding {
  PINOT_AMD_FWD_FIXED_BIT = 0, /* dict-encoded SV, unsorted: FixedBitSVForwardIndexReaderV2 */
  PINOT_AMD_FWD_RAW = 1,       /* raw fixed-width SV: FixedBytePower2ChunkSV / FixedByteChunkSV (PASS_THROUGH) */
  PINOT_AMD_FWD_SORTED = 2,    /* dict-encoded SV, sorted: SortedIndexReaderImpl */
  PINOT_AMD_FWD_FIXED_BIT_MV = 3 /* dict-encoded MV: FixedBitMVForwardIndexReader (pinot_amd_segment_add_mv_column) */
};

/* Predicate types (pinot-common/.../request/context/predicate/Predicate.java Type) */
enum pinot_amd_predicate_type { PINOT_AMD_EQ = 0, PINOT_AMD_NOT_EQ = 1, PINOT_AMD_IN = 2, PINOT_AMD_NOT_IN = 3,
                                PINOT_AMD_RANGE = 4,
                                /* RegexpLikePredicate on a STRING column: the pattern is h_values_s[0], num_values 1;
                                 * _CI is match parameter 'i' (CASE_INSENSITIVE | UNICODE_CASE). A LIKE is the
                                 * REGEXP_LIKE_CI of pinot_amd_like_to_regexp's pattern. */
                                PINOT_AMD_REGEXP_LIKE = 5, PINOT_AMD_REGEXP_LIKE_CI = 6 };

/* Aggregation functions (pinot-segment-spi/.../AggregationFunctionType.java) */
enum pinot_amd_agg_type { PINOT_AMD_AGG_COUNT = 0, PINOT_AMD_AGG_SUM = 1, PINOT_AMD_AGG_MIN = 2,
                          PINOT_AMD_AGG_MAX = 3, PINOT_AMD_AGG_SUMLONG = 4, PINOT_AMD_AGG_AVG = 5,
                          /* MinMaxRangeAggregationFunction: (min, max) pair built with < / > (NaN never
                           * enters it); final result max - min */
                          PINOT_AMD_AGG_MINMAXRANGE = 6,
                          /* DistinctCountAggregationFunction: per group the set of distinct values of the
                           * column (value identity = its id in the batch's merged dictionary: FLOAT/DOUBLE by
                           * floatToIntBits / doubleToLongBits, one NaN, -0.0 != 0.0); final result the set's
                           * size. See "DISTINCTCOUNT results" below. */
                          PINOT_AMD_AGG_DISTINCTCOUNT = 7,
                          /* The other aggregations answered from DISTINCTCOUNT's value-set query, whose rows
                           * with their COUNT are each group's histogram over the column's distinct values in
                           * merged-dictionary order (added with pinot_amd_query_add_aggregation_param; one INT /
                           * LONG / FLOAT / DOUBLE column). See "DISTINCTCOUNT results" below.
                           * PercentileAggregationFunction.java:79-131,207-252: the group's values as doubles
                           * over every matching doc, sorted as Arrays.sort(double[]) does (-0.0 < 0.0, NaN
                           * greatest: the merged dictionary's order); n values: the last for p = 100, else the
                           * one at index (int) ((double) n * p / 100.0); no matching doc: -inf. */
                          PINOT_AMD_AGG_PERCENTILE = 8,
                          /* DistinctSumAggregationFunction.java:83-95: the sum of DISTINCTCOUNT's set as doubles
                           * (an empty set: 0.0), summed on the device in a fixed order: two executions return
                           * the same bits. An INT / LONG column is also summed exactly: while the sum fits int64
                           * the result is that integer rounded once (equal to the reference's sum while its
                           * partial sums stay below 2^53); FLOAT / DOUBLE: within 1e-12 relative. */
                          PINOT_AMD_AGG_DISTINCTSUM = 9,
                          /* DistinctAvgAggregationFunction.java:83-95: that sum over the set's size (0.0 / 0 =
                           * NaN for an empty set) */
                          PINOT_AMD_AGG_DISTINCTAVG = 10,
                          /* The multi-value aggregations (CountMV / SumMV / MinMV / MaxMV / AvgMV /
                           * MinMaxRangeMVAggregationFunction: the aggregateMV bodies of their SV parents) over one
                           * multi-value INT / LONG / FLOAT / DOUBLE column: every value of a matching doc counts.
                           * Added with pinot_amd_query_add_aggregation_mv (they take no literal). COUNTMV: the
                           * number of values; SUMMV: their sum as doubles; MINMV / MAXMV: value < min / value > max
                           * from +inf / -inf (NaN never enters, with and without GROUP BY); AVGMV: the AvgPair (sum
                           * of values, count of values); MINMAXRANGEMV: the pair (min, max), final max - min. No
                           * matching doc: 0, 0.0, +inf, -inf, -inf, -inf. See "Multi-value columns" below. */
                          PINOT_AMD_AGG_COUNTMV = 11, PINOT_AMD_AGG_SUMMV = 12, PINOT_AMD_AGG_MINMV = 13,
                          PINOT_AMD_AGG_MAXMV = 14, PINOT_AMD_AGG_AVGMV = 15, PINOT_AMD_AGG_MINMAXRANGEMV = 16,
                          /* DistinctCountHLLAggregationFunction.java over one single-value column: per group a
                           * stream-lib HyperLogLog(log2m) offered every matching doc's value (MurmurHash.hash of the
                           * boxed value; a dictionary column offers each distinct value once: the same registers);
                           * merge = element-wise maximum of the registers, final = HyperLogLog.cardinality() as a
                           * LONG, 0 without a matching doc. Registers and estimate equal Pinot's bit for bit. Added
                           * with pinot_amd_query_add_aggregation_hll (it takes log2m). */
                          PINOT_AMD_AGG_DISTINCTCOUNTHLL = 17 };

/* ------------------------------------------------------------------------------------------------
 * Runtime
 * --------------------------------------------------------------------------------------------- */
int pinot_amd_abi_version(void);
const char* pinot_amd_last_error(void);
/* hipSetDevice for the calling thread; one process drives one GPU. */
int pinot_amd_set_device(int device);
/* Diagnostic: generate and hipRTC-compile a spread of query-specialised scan kernels (no device
 * needed). Returns 0 when every shape compiles; verbose != 0 prints each shape (and failures). */
int pinot_amd_jit_selftest(int verbose);
/* Bytes of slack the kernels may read past the end of a column buffer handed to the
 * low-level entry points (segments staged by pinot_amd_segment_* are padded internally). */
size_t pinot_amd_required_padding(void);

/* ------------------------------------------------------------------------------------------------
 * Segment staging: ImmutableSegmentLoader + PinotDataBuffer, HBM edition.
 * Replaces the mmap of a segment's column buffers (local/segment/index/loader/ImmutableSegmentLoader.java,
 * pinot-segment-spi/.../memory/PinotDataBuffer.java). The host buffers are the exact bytes of the
 * segment's index files (V1 files or V3 columns.psf slices); they are copied to HBM once and may be
 * released by the caller after the call returns.
 * --------------------------------------------------------------------------------------------- */
typedef struct pinot_amd_segment pinot_amd_segment;

typedef struct pinot_amd_column_spec {
  const char* name;
  int32_t stored_type;        /* pinot_amd_data_type (value type; dictionary value type for dict columns) */
  int32_t encoding;           /* pinot_amd_fwd_encoding */
  int32_t cardinality;        /* ColumnMetadata.getCardinality (dict columns) */
  int32_t bits_per_element;   /* ColumnMetadata.getBitsPerElement (fixed-bit) */
  const void* h_fwd;          /* forward index buffer */
  size_t fwd_size;
  const void* h_dictionary;   /* dictionary buffer (BE fixed width; strings NUL padded), or NULL */
  size_t dictionary_size;
  const void* h_inverted;     /* bitmap inverted index buffer (BitmapInvertedIndexWriter layout), or NULL */
  size_t inverted_size;
} pinot_amd_column_spec;

int pinot_amd_segment_create(const char* name, int64_t num_docs, pinot_amd_segment** out);
/* Raw (no-dictionary) forward indexes may use any ChunkCompressionType (ChunkCompressionType.java:22):
 * PASS_THROUGH chunks are copied; LZ4, LZ4_LENGTH_PREFIXED, SNAPPY, DELTA and DELTADELTA chunks are
 * decoded on the device (one wave per chunk, BaseChunkForwardIndexReader.decompressChunk); ZSTANDARD
 * and GZIP chunks are inflated on the host with the system libzstd / zlib. Malformed chunks fail
 * with PINOT_AMD_EINVAL. */
int pinot_amd_segment_add_column(pinot_amd_segment* seg, const pinot_amd_column_spec* spec);
/* Multi-value columns: a dictionary-encoded MV forward index as FixedBitMVForwardIndexWriter writes it
 * (local/io/writer/impl/FixedBitMVForwardIndexWriter.java:36-101,143-158, read by FixedBitMVForwardIndexReader.java:66-141),
 * all big-endian: numChunks int32 chunk offsets (docsPerChunk = ceil(2048 / (float) (totalNumValues / numDocs)), the
 * inner division Java's int division; entry k = the value index where doc k * docsPerChunk starts), a bitmap of
 * ceil(totalNumValues / 8) bytes, MSB-first (bit i set = value i starts a doc; every doc has at least one value), and
 * the fixed-bit dictId stream of ceil(totalNumValues * bits / 8) bytes. spec->encoding is PINOT_AMD_FWD_FIXED_BIT_MV,
 * h_dictionary is required and h_fwd / fwd_size are that whole file (V1 <col>.mv.fwd, V3 <col>.forward_index);
 * total_num_values / max_num_values_per_doc are ColumnMetadata's totalNumberOfEntries / maxNumberOfMultiValues. The
 * bytes are copied (padded) and validated on the device: EINVAL when the sizes do not match the formula, the bitmap's
 * popcount is not numDocs, bit 0 is unset, a chunk offset disagrees with the bitmap's rank, or a doc is longer than
 * max_num_values_per_doc. The one derived index is the rank of the first value of every 4096-value tile (one int32 per
 * tile). A segment of 0 docs takes an empty forward index. h_inverted: EUNSUPPORTED (inverted indexes on MV columns are
 * not on the path); raw (no-dictionary) MV forward indexes cannot be staged. pinot_amd_segment_add_column with
 * PINOT_AMD_FWD_FIXED_BIT_MV: EINVAL (use this call).
 *
 * Queries over an MV column:
 *   filters        EQ / IN / RANGE match a doc iff any of its values matches; NOT_EQ / NOT_IN (and negate = 1 on an
 *                  EQ / IN leaf) iff no value is in the excluded set (BaseDictionaryBasedPredicateEvaluator.applyMV,
 *                  PredicateType.isExclusive); leaves are independent (c > 5 AND c < 2 matches a doc holding 1 and 7).
 *                  Each MV leaf becomes a dense docId bitset per segment, built inside the execution where the
 *                  inverted-index expansion runs (pinot_amd_execute_again and last_kernel_ms cover it);
 *                  algorithmic_bytes adds total_values * (bits + 1) / 8 and the bitset written and read once.
 *   aggregations   the six *MV functions above, FILTER lanes included. Each segment gets, at the first query that
 *                  needs them, raw single-value twins of the per-doc count / sum / min / max ("<col>$mvcount",
 *                  "$mvsum" (LONG, exact, when max values x the dictionary's largest magnitude fits int64 in every
 *                  segment of the batch; else "$mvsumd", DOUBLE, summed in value order), "$mvmin", "$mvmax"), which
 *                  count in pinot_amd_segment_device_bytes; the query then aggregates those columns.
 *   fetch          h_values the final double; h_values_i64 the exact COUNTMV and the integer SUMMV when it fits
 *   fetch_intermediate   AVGMV: (sum, value count); MINMAXRANGEMV: (min, max); the others (final, 0)
 * From pinot_amd_execute, naming the column: EUNSUPPORTED for an SV aggregation (SUMLONG, expressions, DISTINCTCOUNT,
 * PERCENTILE, DISTINCTSUM, DISTINCTAVG included) or a key transform over an MV column, an *MV function over an SV
 * column, GROUP BY an MV column, an MV column selected or ordered by in a selection query, and
 * pinot_amd_query_set_group_key_values on an MV column; EINVAL for an *MV function over a STRING column and for a
 * column that is MV in some segments of the batch and SV in others. */
int pinot_amd_segment_add_mv_column(pinot_amd_segment* seg, const pinot_amd_column_spec* spec, int64_t total_num_values,
                                    int32_t max_num_values_per_doc);
/* 1 for a multi-value column (filling totalNumberOfEntries / maxNumberOfMultiValues; either may be NULL), 0 for a
 * single-value column, < 0 on error. */
int pinot_amd_segment_column_mv_info(const pinot_amd_segment* seg, const char* column, int64_t* total_values,
                                     int32_t* max_values);
int pinot_amd_segment_destroy(pinot_amd_segment* seg);
int64_t pinot_amd_segment_num_docs(const pinot_amd_segment* seg);
/* HBM bytes held by the segment (forward indexes + dictionaries + inverted indexes + directories). */
int64_t pinot_amd_segment_device_bytes(const pinot_amd_segment* seg);
/* Device pointer to a staged column's forward-index values (fixed-bit stream, raw values at
 * rawDataStart, or sorted pairs; a multi-value column: its whole forward index file) — for the low-level entry
 * points below. */
const void* pinot_amd_segment_column_fwd(const pinot_amd_segment* seg, const char* column);
/* The packed twin staging built for a raw INT / LONG column (value - base bit-packed in two planes; the
 * streaming scan kernels read it instead of the raw bytes, PINOT_AMD_PACKED=0 builds none). Returns 1 and fills
 * the low plane's bits per doc (0, 16, 32), the high plane's (0..16), the base (the column's minimum) and the
 * twin's HBM bytes (padding included; they count in pinot_amd_segment_device_bytes); 0 when the column has no
 * twin; < 0 on error. Any out pointer may be NULL. */
int pinot_amd_segment_column_packed_info(const pinot_amd_segment* seg, const char* column, int32_t* lo_bits,
                                         int32_t* hi_bits, int64_t* base, int64_t* twin_bytes);

/* ------------------------------------------------------------------------------------------------
 * Low-level operators (one per reference class), device in / device out.
 * --------------------------------------------------------------------------------------------- */

/* FixedBitSVForwardIndexReaderV2.readDictIds over a contiguous docId range
 * (local/segment/index/readers/forward/FixedBitSVForwardIndexReaderV2.java:64-103, FixedBitIntReader.read32).
 * d_packed: big-endian MSB-first bit stream; writes length int32 dictIds to d_out. */
int pinot_amd_fwd_read_dict_ids(const void* d_packed, int32_t bits, int64_t start_doc, int64_t length,
                                int32_t* d_out, void* stream);

/* FixedBitMVForwardIndexReader.getDictIdMV for the whole column (FixedBitMVForwardIndexReader.java:66-141): d_fwd is
 * the MV forward index file in device memory (4-byte aligned, pinot_amd_required_padding() bytes of slack behind it;
 * pinot_amd_segment_column_fwd of a staged MV column is one). Writes d_offsets[num_docs + 1] (doc d's values are
 * [d_offsets[d], d_offsets[d + 1])) and the num_values dictIds in value order; either output may be NULL. */
int pinot_amd_fwd_read_dict_ids_mv(const void* d_fwd, int64_t num_docs, int64_t num_values, int32_t bits,
                                   int32_t* d_offsets, int32_t* d_dict_ids, void* stream);

/* FixedBitSVForwardIndexWriter (local/io/writer/impl/FixedBitSVForwardIndexWriter.java) — packs
 * num_values int32 dictIds into the big-endian bit stream (ceil(n*bits/8) bytes written). */
int pinot_amd_fwd_pack_dict_ids(const int32_t* d_values, int64_t num_values, int32_t bits, void* d_packed,
                                void* stream);

/* FixedBytePower2ChunkSVForwardIndexReader.readValuesSV on a PASS_THROUGH buffer
 * (local/segment/index/readers/forward/FixedBytePower2ChunkSVForwardIndexReader.java:48-90):
 * big-endian values at d_raw (rawDataStart) -> native little-endian values in d_out. */
int pinot_amd_fwd_read_raw(const void* d_raw, int32_t stored_type, int64_t start_doc, int64_t length, void* d_out,
                           void* stream);

/* Dense docId bitsets: bit d of word d/64 set <=> doc d matches (MutableRoaringBitmap in
 * core/operator/docidsets, expanded). num_words = ceil(num_docs / 64). */
int pinot_amd_bitset_and(const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, int64_t num_words, void* stream);
int pinot_amd_bitset_or(const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, int64_t num_words, void* stream);
int pinot_amd_bitset_not(const uint64_t* d_a, uint64_t* d_out, int64_t num_docs, void* stream);
/* BlockDocIdIterator materialisation (core/operator/dociditerators): ascending docIds of the set
 * bits, compacted with wavefront ballot + prefix sums. h_count receives the count. d_out must hold
 * num_docs int32. */
int pinot_amd_bitset_to_doc_ids(const uint64_t* d_bitset, int64_t num_docs, int32_t* d_out, int64_t* h_count,
                                void* stream);
int pinot_amd_bitset_count(const uint64_t* d_bitset, int64_t num_docs, int64_t* h_count, void* stream);

/* RegexpLikePredicateEvaluatorFactory.DictIdBasedRegexpLikePredicateEvaluator
 * (core/operator/filter/predicate/RegexpLikePredicateEvaluatorFactory.java): the dictIds of a STRING column whose
 * values the pattern matches, as java.util.regex's Matcher.find() over the value would (flags 0, or
 * CASE_INSENSITIVE | UNICODE_CASE when case_insensitive is set). h_mask_words receives bit d of 32-bit word d / 32
 * for dictId d (mask_words >= ceil(cardinality / 32); the words behind the dictionary are zeroed), num_matching
 * the count; either may be NULL. The pattern is compiled to a DFA that the device walks one lane per dictionary value
 * or the host walks value by value: PINOT_AMD_REGEX_DEVICE=always|never|auto (auto: the device at 16384 values and
 * above, the measured break-even). A pattern outside the supported subset fails with PINOT_AMD_EUNSUPPORTED and the construct's name, one that
 * java.util.regex rejects too with PINOT_AMD_EINVAL, a column that is not STRING with PINOT_AMD_EINVAL. */
int pinot_amd_segment_regexp_match_dictionary(pinot_amd_segment* seg, const char* column, const char* pattern,
                                              int32_t case_insensitive, uint32_t* h_mask_words, int64_t mask_words,
                                              int64_t* num_matching);
/* Compiles the pattern and drops the automaton: 0, or the error pinot_amd_query_add_predicate would return. */
int pinot_amd_regexp_check(const char* pattern, int32_t case_insensitive);
/* RegexpPatternConverterUtils.likeToRegexpLike: the REGEXP_LIKE pattern of a LIKE pattern, written NUL-terminated to
 * h_out. Returns the pattern's length (without the NUL); when that is >= capacity nothing is written. */
int64_t pinot_amd_like_to_regexp(const char* like, char* h_out, int64_t capacity);

/* ------------------------------------------------------------------------------------------------
 * Query plan: FilterPlanNode + AggregationPlanNode / GroupByPlanNode + CombinePlanNode.
 * A query is compiled once on the host (predicate evaluation per segment mirrors
 * core/operator/filter/predicate/PredicateEvaluatorProvider.java) and executed over a batch of
 * segments in one device pass (replaces ServerQueryExecutorV1Impl -> InstancePlanMakerImplV2 ->
 * per-segment operators -> GroupByCombineOperator / AggregationCombineOperator).
 * --------------------------------------------------------------------------------------------- */
typedef struct pinot_amd_query pinot_amd_query;

typedef struct pinot_amd_predicate_spec {
  const char* column;
  int32_t type;               /* pinot_amd_predicate_type */
  int32_t num_values;         /* EQ/NOT_EQ/REGEXP_LIKE[_CI]: 1; IN/NOT_IN: n; RANGE: unused */
  const int64_t* h_values_i;  /* values for INT/LONG columns */
  const double* h_values_d;   /* values for FLOAT/DOUBLE columns */
  const char* const* h_values_s; /* values for STRING columns; REGEXP_LIKE[_CI]: the pattern (UTF-8) */
  /* RANGE (RangePredicate): bounds in the column's value domain */
  int32_t lower_unbounded, upper_unbounded, lower_inclusive, upper_inclusive;
  int64_t lower_i, upper_i;
  double lower_d, upper_d;
  const char* lower_s;
  const char* upper_s;
  int32_t use_inverted_index; /* 1: evaluate through the bitmap inverted index (BitmapBasedFilterOperator) */
} pinot_amd_predicate_spec;

int pinot_amd_query_create(pinot_amd_query** out);
int pinot_amd_query_destroy(pinot_amd_query* q);
/* Filter in conjunctive normal form: clause c is the OR of its predicates; the filter is the AND of
 * all clauses (an AND/OR/NOT tree is normalised to CNF by the caller; NOT on a leaf = NOT_EQ/NOT_IN
 * or negate=1). */
int pinot_amd_query_add_predicate(pinot_amd_query* q, int32_t clause, const pinot_amd_predicate_spec* p,
                                  int32_t negate);
/* GROUP BY on dictionary-encoded columns (DictionaryBasedGroupKeyGenerator.java:116-180) or on raw
 * INT/LONG/FLOAT/DOUBLE columns (NoDictionarySingleColumnGroupKeyGenerator.java:98-143,
 * NoDictionaryMultiColumnGroupKeyGenerator: one group per distinct value, FLOAT/DOUBLE told apart by
 * floatToIntBits/doubleToLongBits). A raw column gets a derived dictionary twin staged on its segment
 * at the first such query (kept for later queries). */
int pinot_amd_query_add_group_by(pinot_amd_query* q, const char* column);
/* GROUP BY on a time bucket: one of three transform functions of a single-value INT / LONG column (raw,
 * dictionary-encoded or sorted; the encoding may differ between the segments of a batch). All arithmetic is
 * Java long; the key is a LONG: its values, their order and the group identity are those of a LONG column holding
 * the transformed values.
 *   DATETRUNC (DateTruncTransformFunction.java:132-142, DateTimeUtils.getTimestampField, UTC only):
 *     out = out_unit.convert(roundFloor_trunc_unit(MILLISECONDS.convert(v, in_unit)), MILLISECONDS); roundFloor is
 *     Joda's (a true floor: instants before 1970 round toward -inf), week floors to Monday 00:00, month / quarter /
 *     year to the first instant of the civil month / quarter / year (ISOChronology: proleptic Gregorian, UTC).
 *   TIMECONVERT (TimeConversionTransformFunction, JavaTimeUnitTransformer.java:37-41):
 *     out = out_unit.convert(v, in_unit).
 *   DATETIMECONVERT, EPOCH -> EPOCH without a bucketing time zone (EpochToEpochTransformer.java:44-46,
 *     BaseDateTimeTransformer.java:208-243): ms = in_unit.toMillis(v * in_size) (the product wraps, toMillis
 *     saturates); q = (ms / G) * G with G = gran_unit.toMillis(gran_size), the division truncating toward zero;
 *     out = out_unit.convert(q, MILLISECONDS) / out_size.
 * TimeUnit.convert is the JDK's: scaling down divides truncating toward zero, scaling up multiplies and saturates at
 * Long.MIN_VALUE / Long.MAX_VALUE. */
enum pinot_amd_time_unit { /* java.util.concurrent.TimeUnit, in its order */
  PINOT_AMD_NANOSECONDS = 0, PINOT_AMD_MICROSECONDS = 1, PINOT_AMD_MILLISECONDS = 2, PINOT_AMD_SECONDS = 3,
  PINOT_AMD_MINUTES = 4, PINOT_AMD_HOURS = 5, PINOT_AMD_DAYS = 6 };
enum pinot_amd_trunc_unit { /* the units of DateTimeUtils.getTimestampField */
  PINOT_AMD_TRUNC_MILLISECOND = 0, PINOT_AMD_TRUNC_SECOND = 1, PINOT_AMD_TRUNC_MINUTE = 2, PINOT_AMD_TRUNC_HOUR = 3,
  PINOT_AMD_TRUNC_DAY = 4, PINOT_AMD_TRUNC_WEEK = 5, PINOT_AMD_TRUNC_MONTH = 6, PINOT_AMD_TRUNC_QUARTER = 7,
  PINOT_AMD_TRUNC_YEAR = 8 };
enum pinot_amd_key_transform { PINOT_AMD_KEY_DATETRUNC = 0, PINOT_AMD_KEY_TIMECONVERT = 1,
                               PINOT_AMD_KEY_DATETIMECONVERT = 2 };
typedef struct pinot_amd_key_transform_spec {
  int32_t kind;        /* pinot_amd_key_transform */
  int32_t trunc_unit;  /* pinot_amd_trunc_unit; DATETRUNC only */
  int32_t in_unit;     /* pinot_amd_time_unit of the column's values */
  int64_t in_size;     /* DATETIMECONVERT only: 'in_size:in_unit:EPOCH' */
  int32_t out_unit;    /* pinot_amd_time_unit of the key */
  int64_t out_size;    /* DATETIMECONVERT only: 'out_size:out_unit:EPOCH' */
  int32_t gran_unit;   /* DATETIMECONVERT only: 'gran_size:gran_unit' */
  int64_t gran_size;
} pinot_amd_key_transform_spec;
/* Appends a GROUP BY key in order with pinot_amd_query_add_group_by: its index (pinot_amd_query_add_order_by kind 0,
 * the key columns of fetch / export_groups) is its position. A NULL argument, an enum out of range, a size <= 0 or a
 * granularity below one millisecond (DATETIMECONVERT; the fields marked "only" are not read otherwise): EINVAL here.
 * A STRING column: EINVAL, a FLOAT / DOUBLE column: EUNSUPPORTED, both from pinot_amd_execute. Time zones other than
 * UTC, the WEEKS / MONTHS / YEARS outputs of CustomTimeUnitTransformer and SIMPLE_DATE_FORMAT / TIMESTAMP formats
 * have no spec: callers refuse them. Every segment gets, at the first query that needs it, a dictionary-encoded
 * twin of the transformed values (built on the device, kept staged per (column, spec), counted in
 * pinot_amd_segment_device_bytes); the query then runs as a GROUP BY on that fixed-bit column. The spec is part of
 * the query's identity: queries that differ only in it never share a prepared plan. */
int pinot_amd_query_add_group_by_transform(pinot_amd_query* q, const char* column,
                                           const pinot_amd_key_transform_spec* spec);
/* An arithmetic expression over single-value INT / LONG / FLOAT / DOUBLE columns (raw, fixed-bit dictionary or sorted,
 * per segment) and numeric literals, as a postfix tree. Every node's value is a Java double: columns are read as
 * transformToDoubleValuesSV reads them (LONG is (double) v), the result is DOUBLE. Evaluation, in this order
 * (pinot-core/.../operator/transform/function/):
 *   ADD (n >= 2)      acc = 0.0 + the literal arguments in order, then acc += each other argument in order
 *                     (AdditionTransformFunction: plus(x, y) of two -0.0 is 0.0)
 *   MULT (n >= 2)     acc = 1.0 * the literal arguments, then acc *= each other argument (MultiplicationTransformFunction)
 *   SUB, DIV, MOD     first - second, first / second (IEEE: x / 0 = +-inf, 0 / 0 = NaN), Java % = fmod
 *   ABS CEIL FLOOR SQRT SIGN   Math.abs / ceil / floor / sqrt / signum of one non-literal argument
 *   LEAST, GREATEST (n >= 2)   a left fold of Math.min / Math.max (NaN propagates, -0.0 < 0.0)
 * The device result is bit-identical to Java's (no fused multiply-add, no flushed denormals; every NaN is one value).
 * num_args is read for the operator nodes, `column` for COLUMN, `literal` for LITERAL.
 * *out_name is the name of a virtual single-value DOUBLE column of this query, owned by the query; it contains '$'.
 * It is accepted wherever a raw DOUBLE column's name is: pinot_amd_query_add_predicate, _add_aggregation,
 * _add_aggregation_param, _add_aggregation_filter_predicate, _add_group_by, _add_selection and
 * _add_selection_order_by. Equal trees -- the same operators, columns and literal bits after the literal folding
 * above -- get one name, and a segment one twin column per name: built on the device at the first query that needs it,
 * kept staged beside the sources, counted in pinot_amd_segment_device_bytes. The name is part of the query wherever
 * it is used, so queries that differ in a literal share no prepared plan.
 * EINVAL here: more than 32 nodes or 8 distinct columns, a malformed postfix, an arity the list above does not
 * allow, ABS .. SIGN of a literal, an expression without a column. EUNSUPPORTED here: a kind outside the enum (exp,
 * ln, power, round, CASE, CAST ... have none: their libm / BigDecimal results are not bit-reproducible). From
 * pinot_amd_execute: a STRING source EINVAL, a multi-value source EUNSUPPORTED. pinot_amd_query_add_group_by_transform
 * and pinot_amd_query_set_group_key_values of an expression: EUNSUPPORTED.
 * Expression twins (and the "$dict" twins GROUP BY derives from them) are bounded per device by
 * PINOT_AMD_EXPR_TWIN_BYTES (default: 1/8 of the device's memory): building one beyond the budget first drops the
 * least recently used twins no live result reads (with the idle prepared plans over their segments); when none can
 * go the budget is exceeded -- no query fails because of it. */
enum pinot_amd_xnode_kind { PINOT_AMD_X_COLUMN, PINOT_AMD_X_LITERAL, PINOT_AMD_X_ADD, PINOT_AMD_X_SUB, PINOT_AMD_X_MULT,
                            PINOT_AMD_X_DIV, PINOT_AMD_X_MOD, PINOT_AMD_X_ABS, PINOT_AMD_X_CEIL, PINOT_AMD_X_FLOOR,
                            PINOT_AMD_X_SQRT, PINOT_AMD_X_SIGN, PINOT_AMD_X_LEAST, PINOT_AMD_X_GREATEST };
typedef struct pinot_amd_xnode { int32_t kind; int32_t num_args; const char* column; double literal; } pinot_amd_xnode;
int pinot_amd_query_define_expression(pinot_amd_query* q, const pinot_amd_xnode* postfix, int32_t n, const char** out_name);
/* Aggregation function (column NULL or "*" for COUNT(*)). Returns the aggregation index via out_index.
 * PINOT_AMD_AGG_DISTINCTCOUNT takes a column of any stored type, STRING included (EINVAL for NULL / "*").
 * Types above PINOT_AMD_AGG_DISTINCTCOUNT: EINVAL (pinot_amd_query_add_aggregation_param adds the value-set
 * functions, pinot_amd_query_add_aggregation_mv the *MV functions). */
int pinot_amd_query_add_aggregation(pinot_amd_query* q, int32_t agg_type, const char* column, int32_t* out_index);
/* The same for every aggregation type, with the function's literal argument: `param` is the percentile of
 * PINOT_AMD_AGG_PERCENTILE, 0 <= param <= 100 (anything else, NaN included: EINVAL;
 * AggregationFunctionFactory.java:143,191,534-536), and is ignored for the other types. PERCENTILE, DISTINCTSUM and
 * DISTINCTAVG take one column (EINVAL for NULL / "*"; a STRING column: EINVAL from pinot_amd_execute). The
 * percentile is part of no cached plan's identity: queries that differ only in it run the same plans. */
int pinot_amd_query_add_aggregation_param(pinot_amd_query* q, int32_t agg_type, const char* column, double param,
                                          int32_t* out_index);
/* A multi-value aggregation, PINOT_AMD_AGG_COUNTMV .. PINOT_AMD_AGG_MINMAXRANGEMV, over one multi-value column (EINVAL
 * for another type and for NULL / "*"). The two entry points above keep refusing every type beyond the ones they took
 * before (EINVAL), so the *MV functions have their own. The aggregation may carry FILTER lanes
 * (pinot_amd_query_add_aggregation_filter_predicate) like its single-value counterpart. */
int pinot_amd_query_add_aggregation_mv(pinot_amd_query* q, int32_t agg_type, const char* column, int32_t* out_index);
/* DISTINCTCOUNTHLL(column [, log2m]) (DistinctCountHLLAggregationFunction's constructor: one column, an optional
 * integer literal, CommonConstants.Helix.DEFAULT_HYPERLOGLOG_LOG2M = 8 without it). 4 <= log2m <= 16, anything else:
 * EINVAL; NULL / "*" for the column: EINVAL; an arithmetic expression or a transformed key as the column:
 * EUNSUPPORTED. The three entry points above refuse PINOT_AMD_AGG_DISTINCTCOUNTHLL (EINVAL). The aggregation takes no
 * FILTER lanes and no multi-value column (EUNSUPPORTED at pinot_amd_execute, naming the column). */
int pinot_amd_query_add_aggregation_hll(pinot_amd_query* q, const char* column, int32_t log2m, int32_t* out_index);
/* Aggregation over a binary arithmetic transform of two columns (SUM / MIN / MAX / AVG):
 * MultiplicationTransformFunction (times), SubtractionTransformFunction (minus),
 * AdditionTransformFunction (plus) in core/operator/transform/function/. Pinot evaluates these in
 * double; with two INT operands the device sums the exact int64 value (equal to the reference's
 * double sum while partial sums stay below 2^53), otherwise it computes in double as the
 * reference does. Needs the query-specialised (hipRTC) kernel; EUNSUPPORTED without it.
 * DISTINCTCOUNT, PERCENTILE, DISTINCTSUM or DISTINCTAVG over an expression: EUNSUPPORTED. */
enum pinot_amd_expr_op { PINOT_AMD_EXPR_COLUMN = 0, PINOT_AMD_EXPR_MUL = 1, PINOT_AMD_EXPR_SUB = 2,
                         PINOT_AMD_EXPR_ADD = 3 };
int pinot_amd_query_add_aggregation_expr(pinot_amd_query* q, int32_t agg_type, int32_t expr_op, const char* column_a,
                                         const char* column_b, int32_t* out_index);
/* Filtered aggregation, AGG(x) FILTER (WHERE f): one leaf of the CNF of the filter of aggregation `agg_index` (what
 * pinot_amd_query_add_aggregation* returned); clauses and leaves as in pinot_amd_query_add_predicate, the clauses
 * numbered from 0 per aggregation. The aggregation takes exactly the docs matching the main filter AND f
 * (AggregationFunctionUtils.buildFilteredAggregationInfos, java:386-477; an aggregation without a filter takes the
 * main filter's docs). Replaces FilteredGroupByOperator / FilteredAggregationOperator: aggregations with equal
 * filters share one "lane" of the one scan, which evaluates every lane's clauses beside the main filter's. GROUP BY:
 * the groups are the main filter's, also when every aggregation is filtered (java:462-474); a group without a doc
 * in some lane has that function's empty value there (COUNT 0, SUM 0, MIN +inf, MAX / AVG / MINMAXRANGE -inf), and
 * pinot_amd_result_num_docs_matched stays the docs matching the main filter.
 * Limits: the main filter's and every lane's leaves together at most 16, their clauses at most 16, the accumulators
 * (a filtered COUNT and the count of a filtered AVG are accumulators of their lane) at most 16: EUNSUPPORTED here
 * where it is knowable, else at pinot_amd_execute. pinot_amd_execute also returns EUNSUPPORTED for a filtered query
 * where a segment may reach numGroupsLimit (the reference admits groups across lanes in a HashMap's iteration
 * order there: unspecified), with a segment-level trim (pinot_amd_query_set_server_options /
 * pinot_amd_query_set_segment_trim) and with DISTINCTCOUNT / PERCENTILE / DISTINCTSUM / DISTINCTAVG in the query;
 * EINVAL for a selection query and for pinot_amd_execute_filter. */
int pinot_amd_query_add_aggregation_filter_predicate(pinot_amd_query* q, int32_t agg_index, int32_t clause,
                                                     const pinot_amd_predicate_spec* p, int32_t negate);
/* QueryOptions filteredAggregationsSkipEmptyGroups (default 0). Non-zero and no aggregation without a filter: a
 * group exists iff some doc matches the main filter AND (f1 OR ... OR fn), and pinot_amd_result_num_docs_matched
 * counts those docs (FilteredGroupByOperator.java:116-180). With an unfiltered aggregation it changes nothing. */
int pinot_amd_query_set_filtered_aggregations_skip_empty_groups(pinot_amd_query* q, int32_t skip);
/* Install the group key space of group-by column `column` (values in the column's stored type, any
 * order; duplicates ignored): the union of the dictionaries of every server's segments, so that the
 * dense accumulator tables of all servers index groups identically and can be merged in place
 * (the broker merges by value: GroupByDataTableReducer.java:258). Must hold every dictionary value of
 * the segments executed (EINVAL otherwise). Without it the key space is the union over the batch.
 * EUNSUPPORTED when `column` is the column of a transformed key (pinot_amd_query_add_group_by_transform) and not a
 * plain GROUP BY column of the query: a transformed key's space is always the union over the batch. */
int pinot_amd_query_set_group_key_values(pinot_amd_query* q, const char* column, int32_t stored_type, int64_t n,
                                         const int64_t* h_values_i, const double* h_values_d,
                                         const char* const* h_values_s);
/* QueryOptions numGroupsLimit (InstancePlanMakerImplV2.DEFAULT_NUM_GROUPS_LIMIT = 100000). */
int pinot_amd_query_set_num_groups_limit(pinot_amd_query* q, int64_t limit);
/* The server's combine table (GroupByUtils.createIndexedTableForCombineOperator, GroupByUtils.java:104-149;
 * IndexedTable.finish): with no ORDER BY the result keeps LIMIT groups (the table stops accepting new
 * ones; here the first LIMIT in ascending key order); with ORDER BY the top
 * trimSize = max(5 * LIMIT, min_server_group_trim_size) groups by the ORDER BY, sorted (ties in ascending
 * key order). min_server_group_trim_size <= 0 disables the trim (every group kept when ordered). Replaces
 * the server-side IndexedTable of GroupByCombineOperator; not set: every group is returned. */
int pinot_amd_query_set_result_limit(pinot_amd_query* q, int64_t limit, int64_t min_server_group_trim_size,
                                     int64_t group_trim_threshold);
/* Query options of the server result's size (defaults 0 / 10000): serverReturnFinalResult (with ORDER BY and
 * no HAVING the table keeps LIMIT groups, GroupByUtils.java:134-139) and sortAggregateLimitThreshold. With
 * ORDER BY keys = GROUP BY keys (safe trim, QueryContext.java:568-580,746-747) and LIMIT below the threshold,
 * Pinot's sorted combine (CombinePlanNode.java:150-154) keeps the top LIMIT groups, exact; at or above it each
 * segment keeps its top LIMIT groups by the ORDER BY (GroupByOperator.java:157-175) and the combine table the
 * top trimSize of their union -- restated for dense key spaces (a presence pass over ORDER BY ranks, each
 * segment's LIMIT-th rank as the cutoff its docs are aggregated within) and over hash-table key spaces (the
 * (key, segment) scan table, each segment's top LIMIT entries by a radix selection over the ORDER BY). */
int pinot_amd_query_set_server_options(pinot_amd_query* q, int32_t server_return_final_result,
                                       int64_t sort_aggregate_limit_threshold);
/* QueryOptions minSegmentGroupTrimSize (default -1: CommonConstants.java:1436). With ORDER BY not equal to the
 * GROUP BY keys (an unsafe trim) and a positive value, each segment keeps its top max(value, 5 x LIMIT) groups
 * by the ORDER BY, aggregation values included (QueryContext.java:575-578, GroupByUtils.java:63-66): the (key,
 * segment) hash plan, each segment's top entries by a radix selection over the ORDER BY's final values (ties in
 * ascending group key; TableResizer leaves them unspecified). Under a safe trim the segment trim size is LIMIT
 * whatever this value (pinot_amd_query_set_server_options). */
int pinot_amd_query_set_segment_trim(pinot_amd_query* q, int64_t min_segment_group_trim_size);
/* ORDER BY key of the server table, in order of precedence: kind 0 = group-by column `index` (value
 * order), kind 1 = aggregation `index` (final value, Double.compare); ascending != 0 for ASC. */
int pinot_amd_query_add_order_by(pinot_amd_query* q, int32_t kind, int32_t index, int32_t ascending);

/* ------------------------------------------------------------------------------------------------
 * Selection queries: SELECT a, b FROM t WHERE ... [ORDER BY c DESC, ...] LIMIT n [OFFSET m]
 * (core/plan/SelectionPlanNode.java -> core/operator/query/SelectionOnlyOperator.java /
 * SelectionOrderByOperator.java per segment -> core/operator/combine/SelectionOrderByCombineOperator.java).
 * A query with at least one selection column is a selection query: pinot_amd_execute runs the filter and, in the
 * same pass, keeps each segment's best offset + limit rows on the device (SelectionOrderByOperator.java:112: the
 * server keeps offset + limit rows, the broker applies the offset), gathers their columns by docId
 * (SelectionOrderByOperator.java:270-330, the second-round projection) and combines the segments' rows.
 *   - Columns: plain single-value columns of any stored type, STRING included. The result's columns are the
 *     selection columns in the order added; the caller arranges them into the server's schema -- the ORDER BY
 *     columns first (core/query/selection/SelectionOperatorUtils.java:83-125) -- and expands SELECT *.
 *   - ORDER BY compares by value: INT / LONG numerically, FLOAT / DOUBLE as Float.compare / Double.compare
 *     (-0.0 < 0.0, NaN greatest), STRING as String.compareTo; descending reverses it. Pinot leaves ties unspecified
 *     (SelectionOperatorUtils.java:630-637 evicts an arbitrary worst row; the combine is multi-threaded): here ties
 *     are broken by ascending (index of the segment in the batch, docId), one of Pinot's possible answers, so
 *     results are deterministic. The key is at most two 64-bit words (a dictionary column, INT or FLOAT takes 32
 *     bits, a raw LONG or DOUBLE 64): a wider ORDER BY is EUNSUPPORTED.
 *   - Without ORDER BY the rows are the first offset + limit matching docs in (segment index, docId) order
 *     (SelectionOnlyOperator takes docs in docId order; Pinot's combine takes whichever segments answer first).
 *     Segments are scanned in batch order in groups of 1, 2, 4, ... and the scan stops once enough rows are held.
 *   - LIMIT 0: the ORDER BY is ignored and no row is returned (EmptySelectionOperator); the schema is valid.
 *   - offset + limit up to half the scan's LDS buffer (2048 rows without ORDER BY, 1024 with) is pruned on the
 *     device as it scans (kernel_info "jit-topk"); above that every matching doc's record is written and sorted
 *     ("jit-topk-sort"), within PINOT_AMD_TOPK_SORT_MAX_BYTES (default 4 GiB) and offset + limit <= 2^20, beyond
 *     which the query is EUNSUPPORTED.
 * A query with selection columns and any aggregation or GROUP BY fails pinot_amd_execute with EINVAL;
 * pinot_amd_execute_filter ignores the selection fields.
 *
 * The result calls on a selection result:
 *   pinot_amd_result_num_docs_matched   with ORDER BY every matching doc; without, the rows returned
 *   pinot_amd_execute_again             re-runs the passes; last_kernel_ms covers them (the scan, the candidate
 *                                       sort, the cut and the gather)
 *   kernel_info                         "jit-topk" or "jit-topk-sort", " xN" for N launches run
 *   algorithmic_bytes                   the filter and ORDER BY columns streamed once, plus the gathered columns of
 *                                       the rows fetched
 *   check_word                          reads 0
 *   num_groups, fetch, fetch_intermediate, fetch_distinct_values, fetch_value_counts: EINVAL
 *   accumulators, export_groups, merge_groups: EUNSUPPORTED
 * --------------------------------------------------------------------------------------------- */
/* An output column; out_index (optional) receives its index among the result's columns. */
int pinot_amd_query_add_selection(pinot_amd_query* q, const char* column, int32_t* out_index);
/* An ORDER BY column, in order of precedence (ascending != 0 for ASC); it need not be selected. */
int pinot_amd_query_add_selection_order_by(pinot_amd_query* q, const char* column, int32_t ascending);
/* LIMIT and OFFSET, both >= 0 (EINVAL otherwise). Not set: LIMIT 10 (Pinot's default), OFFSET 0. */
int pinot_amd_query_set_selection_limit(pinot_amd_query* q, int64_t limit, int64_t offset);

/* ------------------------------------------------------------------------------------------------
 * Distinct queries: SELECT DISTINCT a, b FROM t WHERE ... [ORDER BY a DESC, ...] LIMIT n
 * (core/plan/DistinctPlanNode.java -> core/operator/query/DistinctOperator.java /
 * DictionaryBasedDistinctOperator.java per segment -> core/operator/combine/DistinctCombineOperator.java, with
 * core/query/distinct/DistinctExecutorFactory.java and core/query/distinct/table/MultiColumnDistinctTable.java).
 * pinot_amd_query_set_distinct turns a query into a distinct query: its distinct columns are the keys added with
 * pinot_amd_query_add_group_by / _add_group_by_transform, in order; its ORDER BY the pinot_amd_query_add_order_by
 * entries of kind 0; `limit` its LIMIT (Pinot's default is 10). The scan records one presence bit per matching
 * doc -- no accumulator, no COUNT cell -- in a bitmap indexed by the row's rank in the result order, so the answer
 * is the bitmap's first LIMIT set bits.
 *   - Columns: single-value columns of any stored type, dictionary, sorted or raw, an expression
 *     (pinot_amd_query_define_expression) or a time-bucket transform, exactly as GROUP BY keys. Values are
 *     identified as group keys are (FLOAT / DOUBLE by floatToIntBits / doubleToLongBits: one NaN, -0.0 != 0.0).
 *     A multi-value column is EUNSUPPORTED (DistinctExecutorFactory's processMV is not restated).
 *   - Result: the distinct rows over every doc matching the filter in every segment of the batch, cut to LIMIT.
 *   - With ORDER BY (only distinct columns can be named: Pinot asserts it) the first LIMIT rows in that order.
 *     Values compare as the server table compares group columns (numerically, Double.compare, String.compareTo;
 *     DESC reverses). Rows equal on the ORDER BY columns are ordered by ascending global group key; Pinot leaves
 *     such ties to a hash set's iteration order, so this is one of its possible answers.
 *   - Without ORDER BY Pinot keeps whichever LIMIT rows it meets first and stops scanning
 *     (DistinctTable.addWithoutOrderBy returns true, DistinctOperator breaks). Here the segments are scanned in
 *     batch order in groups of 1, 2, 4, ... segments (as a selection without ORDER BY); the scan stops after the
 *     first group that leaves at least LIMIT distinct rows held, or after the last segment, and the result is the
 *     first LIMIT held rows in ascending global key order. A hash plan scans the whole batch.
 *   - LIMIT 0: no row, a valid schema, nothing scanned. numGroupsLimit does not apply (a DistinctTable knows
 *     only its limit).
 *   - One dictionary-encoded or sorted column and no filter (DictionaryBasedDistinctOperator): the first LIMIT
 *     values of the batch's merged dictionary, the last LIMIT with ORDER BY ... DESC; no kernel runs;
 *     num_docs_matched is the sum over the segments of min(LIMIT, cardinality), as that operator reports.
 *   - Plans: key spaces up to 2^31 keys take the bitmap -- in a 256-thread block's LDS up to 327 680 keys, in one
 *     CU-wide block's LDS up to about 1.3 M keys (LDS bitmaps are OR-ed into the HBM bitmap once per block), in HBM
 *     above that; larger key spaces, or PINOT_AMD_GROUP_PLAN=hash, take the COUNT-only hash plan, whose groups are
 *     cut to LIMIT by the ordered table. PINOT_AMD_DISTINCT_PLAN=lds|wide|hbm|hash pins the kind (tests).
 * pinot_amd_execute fails with EINVAL for a distinct query without a key, with an aggregation, a selection
 * column, an ORDER BY of kind 1, or with pinot_amd_query_set_result_limit / _set_server_options /
 * _set_segment_trim called on it; with EUNSUPPORTED, naming the column, for a multi-value key and for
 * pinot_amd_query_set_group_key_values (there is no multi-GPU merge of distinct results).
 * pinot_amd_execute_filter ignores the distinct flag and limit; both are part of a prepared plan's identity.
 *
 * The result calls on a distinct result:
 *   pinot_amd_result_num_groups         the rows held, at most LIMIT
 *   pinot_amd_result_fetch              the rows' values as a GROUP BY fetch returns keys, in result order;
 *                                       h_values / h_values_i64 may be NULL (there are no aggregations)
 *   pinot_amd_result_string_key         as for a group-by result
 *   pinot_amd_result_num_docs_matched   the docs matching the filter in the segments actually scanned
 *   pinot_amd_execute_again             re-zeroes the bitmap and re-runs every pass; last_kernel_ms covers them
 *   kernel_info                         "jit-distinct-lds", "jit-distinct-wide", "jit-distinct-hbm" (" xN" for N
 *                                       launches run, when N != 1), the hash plan's name, or "distinct-dictionary"
 *   algorithmic_bytes                   the filter and distinct columns of the scanned segments, streamed once
 *   check_word                          reads 0
 *   fetch_intermediate, fetch_distinct_values, fetch_value_counts: EINVAL
 *   accumulators, export_groups, merge_groups: EUNSUPPORTED
 * --------------------------------------------------------------------------------------------- */
/* limit >= 0 (EINVAL otherwise). */
int pinot_amd_query_set_distinct(pinot_amd_query* q, int64_t limit);

/* ------------------------------------------------------------------------------------------------
 * Execution and results (IntermediateResultsBlock / AggregationGroupByResult equivalents).
 * --------------------------------------------------------------------------------------------- */
typedef struct pinot_amd_result pinot_amd_result;

/* Execute q over n segments as one batched device pass on `stream`; results stay in HBM until
 * fetched. The group key space across segments is the union of their dictionaries. */
int pinot_amd_execute(pinot_amd_query* q, pinot_amd_segment* const* segs, int32_t n, void* stream,
                      pinot_amd_result** out);
/* FilterPlanNode -> BlockDocIdSet for each segment: evaluates only q's filter and keeps, per segment,
 * a dense docId bitset in HBM (bit d of word d/64 set <=> doc d matches), readable with
 * pinot_amd_result_bitset and convertible to ascending docIds with pinot_amd_bitset_to_doc_ids. */
int pinot_amd_execute_filter(pinot_amd_query* q, pinot_amd_segment* const* segs, int32_t n, void* stream,
                             pinot_amd_result** out);
/* Device pointer and word count of segment `segment_index`'s docId bitset of a filter-only result. */
int pinot_amd_result_bitset(pinot_amd_result* r, int32_t segment_index, const uint64_t** h_d_bitset,
                            int64_t* h_num_words);
/* Re-run a query whose plan was compiled by pinot_amd_execute on the same segments (no host work
 * beyond the launches): the benchmarked step. */
int pinot_amd_execute_again(pinot_amd_result* r, void* stream);
/* Release a result after synchronising its stream. Its plan is kept (idle, up to PINOT_AMD_PLAN_CACHE_BYTES of
 * plan device memory) for the next pinot_amd_execute of the same query -- every field, the same segments, the
 * same device and planner overrides -- which then only runs it; destroying a segment drops the plans over it. */
int pinot_amd_result_destroy(pinot_amd_result* r);
/* Number of docs that matched the filter across all segments (numDocsScanned). */
int pinot_amd_result_num_docs_matched(pinot_amd_result* r, int64_t* h_out);
/* Number of groups with >= 1 matching doc (1 for an aggregation-only query). */
int pinot_amd_result_num_groups(pinot_amd_result* r, int64_t* h_out);
/* numGroupsLimitReached (GroupByOperator / GroupByResultsBlock metadata): 1 when some segment reached
 * the query's numGroupsLimit. As in Pinot, each segment admits only the first numGroupsLimit groups
 * it sees in docId order (DictionaryBasedGroupKeyGenerator.java:351-363); later groups of that
 * segment are dropped, and the combine keeps the union of the admitted groups. */
int pinot_amd_result_num_groups_limit_reached(pinot_amd_result* r, int32_t* h_out);
/* Fetch up to cap groups: h_keys[g*num_group_by + j] = group-by column j's value as int64 (INT/LONG),
 * its double bits (FLOAT/DOUBLE) or its index into the merged STRING dictionary
 * (pinot_amd_result_string_key); h_values[g*num_aggs + a] = final result as double
 * (COUNT, SUM, MIN, MAX, AVG, SUMLONG, MINMAXRANGE as double; SUM of integers is the exact 128-bit
 * sum rounded once); h_values_i64 (optional) = exact COUNT / SUMLONG, and SUM on integer columns when
 * it fits int64 (INT64_MIN otherwise). Groups are ordered by ascending global key. */
int pinot_amd_result_fetch(pinot_amd_result* r, int64_t cap, int64_t* h_keys, double* h_values,
                           int64_t* h_values_i64, int64_t* h_num_fetched);
/* AggregationFunction.extractAggregationResult: the intermediate result of every aggregation, two
 * doubles per (group, aggregation) in fetch order — AVG: AvgPair (sum, count); MINMAXRANGE:
 * MinMaxRangePair (min, max); every other function: (final value, 0). What a server hands the broker
 * for the cross-server merge. */
int pinot_amd_result_fetch_intermediate(pinot_amd_result* r, int64_t cap, double* h_pairs, int64_t* h_num_fetched);
/* String value of merged-dictionary id `id` for group-by column j. */
const char* pinot_amd_result_string_key(pinot_amd_result* r, int32_t j, int64_t id);
/* The execution's self-check word (device address of one uint64; 0 = the check held). Partitioned plans
 * verify that every doc past the filter became exactly one record and reached the aggregation
 * (DefaultGroupByExecutor.java:192-219 folds each doc once); a nonzero word voids the result: every read
 * of its groups or matched count fails with PINOT_AMD_EINVAL. A multi-GPU merge carries the word through
 * its collectives (every rank then fails, none returns a table a failed rank contributed to). */
int pinot_amd_result_check_word(pinot_amd_result* r, void** h_d_word);
/* Executions of this process whose self-check failed (each also failed its result with PINOT_AMD_EINVAL). */
int64_t pinot_amd_selfcheck_failures(void);
/* Device view of the dense accumulators for a multi-GPU merge (RCCL all-reduce in place):
 * per aggregation slot an array of num_key_slots 8-byte words; op per slot: 0 = sum(int64),
 * 1 = sum(double), 2 = min(uint64 ordered), 3 = max(uint64 ordered), 4 / 5 = low / high word of an
 * exact 128-bit integer sum. EUNSUPPORTED for hash-table plans (merge those by value). */
int pinot_amd_result_accumulators(pinot_amd_result* r, int32_t* h_num_slots, int64_t* h_num_key_slots,
                                  void** h_slot_ptrs, int32_t* h_slot_ops);
/* Cross-GPU merge by value (replaces the broker's GroupByDataTableReducer merge of server DataTables,
 * pinot-core/.../query/reduce/GroupByDataTableReducer.java:258, and IndexedTable.upsert's
 * AggregationFunction.merge): for GROUP BY results of any plan (dense, partitioned, hash, trimmed).
 * export_groups writes the result's groups to device memory: h_key_words 64-bit words per group (the
 * merged key space's ids packed <= 63 bits per word) at d_keys[g * key_words], h_num_acc accumulator
 * words per group at d_acc[g * num_acc] (the library's encoding). d_keys / d_acc NULL: only the three
 * sizes. Every rank exports the same layout once the same global key space is installed
 * (pinot_amd_query_set_group_key_values). merge_groups folds n such rows (a rank's share of every
 * rank's rows, exchanged over RCCL) into one device hash table with the accumulator ops; until the next
 * execution the result's groups (num_groups / fetch / fetch_intermediate / export_groups) are the merged
 * ones, so a key-partitioned merge can export its merged share again. `stream` (NULL: the result's
 * stream) is ordered after the result's own stream by the library and used for this call only. */
int pinot_amd_result_export_groups(pinot_amd_result* r, uint64_t* d_keys, uint64_t* d_acc, int64_t cap,
                                   int32_t* h_key_words, int32_t* h_num_acc, int64_t* h_num_groups, void* stream);
int pinot_amd_result_merge_groups(pinot_amd_result* r, const uint64_t* d_keys, const uint64_t* d_acc, int64_t n,
                                  void* stream);
/* ------------------------------------------------------------------------------------------------
 * DISTINCTCOUNT results (DistinctCountAggregationFunction / BaseDistinctAggregateAggregationFunction in
 * core/query/aggregation/function/: per-group dictId bitmaps, convertToValueSet, merge = union, final = size).
 * pinot_amd_execute of a query with at least one PINOT_AMD_AGG_DISTINCTCOUNT runs, inside the library and on the
 * caller's stream, the base query (the query without its DISTINCTCOUNTs, or with COUNT(*) when nothing else is
 * left) and one value-set query per distinct DISTINCTCOUNT column c: the same predicates and installed key spaces,
 * GROUP BY g..., c, COUNT(*) only, no server table, numGroupsLimit raised to 2^30. Their groups are folded on the
 * device into per-group value sets when the result's groups are first read. The result's groups are the base
 * query's: with numGroupsLimit only the groups the base admitted are kept, each with all its values over the batch
 * (Pinot would also drop, per segment, the docs of the groups that segment did not admit). DISTINCTCOUNT of a
 * GROUP BY column is 1 per group and runs no value-set query. EUNSUPPORTED: kMaxGroupCols (16) GROUP BY columns
 * already, and the segment-level trims (ORDER BY = GROUP BY with LIMIT >= sortAggregateLimitThreshold and no
 * serverReturnFinalResult; minSegmentGroupTrimSize > 0 with another ORDER BY). The server table
 * (pinot_amd_query_set_result_limit / add_order_by) may order by a DISTINCTCOUNT: its final value is the count.
 *
 * The result calls on such a result:
 *   pinot_amd_execute_again            re-runs the base and the value-set queries
 *   last_kernel_ms, algorithmic_bytes  summed over the base and the value-set queries
 *   kernel_info                        the base's, then " +distinct(<column>:<value-set query's kernel_info>)" each
 *   num_docs_matched, num_groups, num_groups_limit_reached, string_key, check_word: the base's
 *   fetch                              a DISTINCTCOUNT's h_values = the count as double, h_values_i64 = the count
 *   fetch_intermediate                 (count, 0); the set itself comes from fetch_distinct_values
 *   accumulators, export_groups, merge_groups: EUNSUPPORTED (sets merge by union, not by accumulator op)
 * Every read fails with EINVAL when the self-check of the base or of a value-set query failed, or when a
 * (group, value) pair belongs to no group of a base query that could not have trimmed.
 *
 * PERCENTILE, DISTINCTSUM and DISTINCTAVG are answered from the same value-set query (every such aggregation on
 * one column shares it, whatever the percentile: kernel_info keeps one " +distinct(<column>:...)" per column), with
 * the same rules (groups, numGroupsLimit, kMaxGroupCols, segment-level trims, the result calls above). The
 * value-set query's COUNT rides through the fold: a percentile is a rank selection in each group's cumulative doc
 * counts, DISTINCTSUM a segmented sum of the dictionary's values over the group's ids, both on the device; one
 * word per group and PERCENTILE (two per column for the sums) cross PCIe with the distinct counts.
 *   fetch               h_values = the final double. h_values_i64 = the selected value of a PERCENTILE of an INT /
 *                       LONG column (exact beyond 2^53), the integer sum of a DISTINCTSUM of an INT / LONG column
 *                       when it fits int64, INT64_MIN otherwise
 *   fetch_intermediate  (final value, 0); the histogram comes from fetch_value_counts
 *   the server table    may order by any of them
 * Of a GROUP BY column each is the key's own value.
 *
 * DistinctCountAggregationFunction.extractGroupByResult: the value sets, CSR over the groups in fetch
 * order (after a server table: its kept groups, in its order). h_offsets[ngroups + 1];
 * h_values[h_offsets[g] .. h_offsets[g+1]) = group g's distinct values of aggregation agg_index, ascending
 * merged-dictionary id, each as fetch's key encoding (int64 / double bits / index for
 * pinot_amd_result_distinct_string). h_offsets may be NULL. h_values NULL: sizes only (h_num_values = the total).
 * More than cap values: EOVERFLOW. EINVAL when agg_index is not a DISTINCTCOUNT, PERCENTILE, DISTINCTSUM or
 * DISTINCTAVG of the result.
 * --------------------------------------------------------------------------------------------- */
int pinot_amd_result_fetch_distinct_values(pinot_amd_result* r, int32_t agg_index, int64_t cap, int64_t* h_offsets,
                                           int64_t* h_values, int64_t* h_num_values);
/* The same CSR with h_counts[i] = the matching docs holding h_values[i]: each group's histogram, the
 * intermediate result a server hands on for PERCENTILE (PercentileAggregationFunction's DoubleArrayList, sorted
 * and run-length encoded). Same conventions (h_values NULL: sizes only; EOVERFLOW; after a server table its kept
 * groups in its order); h_values without h_counts: EINVAL. Valid for all four value-set aggregation types; when
 * no PERCENTILE of the column made the fold carry the doc counts, the first such call folds once more with them. */
int pinot_amd_result_fetch_value_counts(pinot_amd_result* r, int32_t agg_index, int64_t cap, int64_t* h_offsets,
                                        int64_t* h_values, int64_t* h_counts, int64_t* h_num_values);
/* String value of merged-dictionary id `id` of aggregation agg_index's value-set column (NULL when it is
 * not a STRING column or id is out of range). */
const char* pinot_amd_result_distinct_string(pinot_amd_result* r, int32_t agg_index, int64_t id);

/* The registers of aggregation agg_index, a PINOT_AMD_AGG_DISTINCTCOUNTHLL of the result: the intermediate result
 * a server hands on (DistinctCountHLLAggregationFunction.extractAggregationResult / extractGroupByResult: the
 * HyperLogLog itself; here its RegisterSet as one byte per register, 2^log2m per group, not the library's serialised
 * form). Groups in pinot_amd_result_fetch's order (after a server table: its kept groups in its order);
 * *out_log2m and *out_groups are always set; h_registers NULL: sizes only; fewer than groups << log2m bytes of
 * capacity: EOVERFLOW. pinot_amd_result_fetch returns the estimate (exact in h_values_i64),
 * pinot_amd_result_fetch_intermediate (estimate, 0). */
int pinot_amd_result_fetch_hll(pinot_amd_result* r, int32_t agg_index, int64_t cap_bytes, uint8_t* h_registers,
                               int32_t* out_log2m, int64_t* out_groups);

/* Selection results (DataSchema + rows of SelectionResultsBlock). EINVAL on any other result. */
int pinot_amd_result_selection_num_columns(pinot_amd_result* r, int32_t* h_out);
/* Column j's name (owned by the result) and stored type (pinot_amd_data_type); either out pointer may be NULL. */
int pinot_amd_result_selection_column(pinot_amd_result* r, int32_t j, const char** h_name, int32_t* h_stored_type);
/* Rows of the last execution: at most offset + limit. */
int pinot_amd_result_num_rows(pinot_amd_result* r, int64_t* h_out);
/* The rows in result order: h_values[row * num_columns + j] encoded as pinot_amd_result_fetch encodes keys -- the
 * value as int64 (INT / LONG), its double bits (DOUBLE; a FLOAT widened to double), or an id for
 * pinot_amd_result_selection_string (STRING). h_segment / h_doc_id (optional) receive each row's origin: the
 * index of its segment in the batch and its docId. More rows than cap: EOVERFLOW. */
int pinot_amd_result_fetch_rows(pinot_amd_result* r, int64_t cap, int32_t* h_segment, int32_t* h_doc_id, int64_t* h_values,
                                int64_t* h_num_fetched);
/* String of id `id` of STRING column j of the fetched rows (NULL when out of range); valid until the next
 * execution of the result. */
const char* pinot_amd_result_selection_string(pinot_amd_result* r, int32_t j, int64_t id);

/* The device plan: "jit" (fused scan), "jit-partitioned", "jit-hash", "jit-hash-trim"; then "-select" /
 * "-wselect" / "-fwselect" for a selection-vector plan (filter on 4-doc tiles / on 64-doc bitset words /
 * fused with the inverted-index expansion), "+admit-seq" / "+admit" for numGroupsLimit admission
 * (sequential / first-doc), and " xN" when the batch ran as N shape launches; "jit-topk" /
 * "jit-topk-sort" for a selection query. */
const char* pinot_amd_result_kernel_info(pinot_amd_result* r);
/* Algorithmic HBM bytes of the last execution (the roofline numerator): every decoded column once
 * (fixed-bit columns at their bit width, raw columns at their value width, or at their packed twin's width
 * where the plan streams the twin: pinot_amd_result_packed_info); under an inverted-index
 * gate only the rows that pass it; selection-vector plans: the filter columns of every doc, 16 B per
 * vector entry (written + read) and the gathered columns of the matches; plus, per inverted-index leaf,
 * the selected bitmaps' serialized bytes and -- only when the expansion writes one -- the dense docId
 * bitset written and read once (the fused -fwselect plan writes none); plus, per leaf on a multi-value column, its
 * total_values * (bits + 1) / 8 bytes of dictIds and start bits and the dense docId bitset written and read once. */
int pinot_amd_result_algorithmic_bytes(pinot_amd_result* r, double* h_bytes);
/* Which raw columns the plan's streaming kernels read through their packed twins: "column:lo+hi" (plane bits
 * per doc) per column and shape launch, launches separated by ";", "" when none. Such columns count in
 * pinot_amd_result_algorithmic_bytes at (lo + hi) / 8 bytes per row. */
const char* pinot_amd_result_packed_info(pinot_amd_result* r);
/* Host planning time of the execute that built this result, per phase, as "phase=ms;..." (raw_keys:
 * derived dictionaries of raw GROUP BY columns; leaves: per-segment predicate resolution; keys_probe:
 * merged key space + the plan-time match-count probe; plan: accumulators, plan kind, descriptors;
 * jit_alloc: kernel lookup / hipRTC compile, launch descriptors and buffers; launch: enqueueing the first
 * execution). Diagnostics for cold / cached query latency. */
const char* pinot_amd_result_plan_timing(pinot_amd_result* r);
/* Kernel timing of the last execute: device milliseconds of the fused scan kernel, measured with
 * HIP events on the execution stream. */
int pinot_amd_result_last_kernel_ms(pinot_amd_result* r, double* h_ms);

#ifdef __cplusplus
}
#endif
#endif /* PINOT_AMD_H */
