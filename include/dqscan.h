/*
 * dqscan.h -- C ABI of libdqscan.so, the MI355X (gfx950) replacement for Deequ's fused
 * single-pass metric scan.
 *
 * Reference interface this replaces (paths relative to src/main/scala/com/amazon/deequ/):
 *   AnalysisRunner.runScanningAnalyzers            analyzers/runners/AnalysisRunner.scala:279-326
 *     -> data.agg(aggregations...).collect().head   analyzers/runners/AnalysisRunner.scala:303
 *   ScanShareableAnalyzer.aggregationFunctions /
 *     fromAggregationResult(row, offset)           analyzers/Analyzer.scala:159-187
 *   State.sum / Analyzers.merge                    analyzers/Analyzer.scala:34-48, 343-362
 *   DeequHyperLogLogPlusPlusUtils.count            analyzers/catalyst/StatefulHyperloglogPlus.scala:210-257
 *   HdfsStateProvider persist / load byte images   analyzers/StateProvider.scala:176-294
 *
 * Call pattern of a drop-in shim (Scala/JNI, C++, or the Python host in deequ_amd/):
 *   dq_plan_create(specs, schema, predicate IR)    <- the GPU-eligible ScanShareableAnalyzers
 *   dq_scan(plan, columns, n_rows, chunk) ...      <- one or more row chunks, HBM-resident buffers
 *   dq_finish(plan, states)                        <- one aggregation "Row" slot set per spec
 *   dq_state_* / dq_hll_estimate                   <- state algebra for StateLoader/Persister merges
 *
 * All functions return DQ_OK (0) or a negative dq_status; dq_last_error() (thread-local) holds the
 * message.  A shim maps ANY failure of plan/scan/finish to a failure metric on every GPU-routed
 * analyzer, as runScanningAnalyzers does for an aggregation exception (AnalysisRunner.scala:310-313).
 * Plans are not thread-safe: one plan per calling thread.  State functions are pure and reentrant.
 */
#ifndef DQSCAN_H
#define DQSCAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DQ_ABI_VERSION 6  /* 2: dq_state.reserved[0] = integral flag + Sum / Mean int64 partials; ingestion, pool and state-array entry points;
                             3: dq_plan_create_opts (predicate-pass mode), dq_plan_create_time, dq_plan_explain, dq_quantile_digest;
                             4: any number of analyzers / columns per plan (split into fused plans over the
                                per-plan capacities), AUTO compiles the predicate kernel in the background,
                                dq_plan_pred_wait;
                             5: column types F32 / I16 / I8 / BOOL / DATE32 / TIMESTAMP (scan, predicates, Arrow import);
                             6: DECIMAL128 (type codes carry precision / scale, dq_state Sum / Mean decimal partials);
                                dq_cast_utf8, the dq_cat_hist_* entry points, the dq_schema_* / dq_take_* / dq_split_*
                                entry points and dq_pred_jit_drain are additions under 6 (nothing existing changed its layout or meaning);
                                so are dq_freq_materialize / _self_contained / _to_bytes / _from_bytes / _take_values /
                                _mutual_information (self-contained frequency tables) and the row-level results:
                                dq_row_program_* / dq_row_outcomes (per-row predicate outcomes as bitmaps),
                                dq_freq_unique_rows (the rows whose group has count 1); arithmetic operands of
                                predicates: DQ_PRED_EXPR, dq_pred_pool_num_exprs / _expr, dq_expr_eval / _host; uploads into
                                caller-owned buffers: dq_upload_to / _payload / _stage; referential integrity:
                                dq_freq_contains_rows (the rows whose tuple is a group of another table's key set);
                                binned histograms: dq_bins_create / _destroy, dq_bin_count; row selections for the grouping,
                                histogram and quantile entry points: dq_freq_build_where / _unique_rows_where,
                                dq_dict_count_where, dq_bin_count_where, dq_approx_quantiles_where,
                                dq_quantile_digest_where, dq_mutual_information_where; dataset match:
                                dq_freq_lookup_rows (which group a row hit), dq_rows_match (a row's other columns
                                against the reference row of its group); distribution drift: dq_freq_distance
                                (L-infinity / total variation / Jensen-Shannon between two frequency tables),
                                dq_freq_ks (their two-sample Kolmogorov-Smirnov statistic) */

typedef int32_t dq_status;
#define DQ_OK 0
#define DQ_E_INVALID (-1)     /* bad argument / malformed spec */
#define DQ_E_TYPE (-2)        /* column type not valid for the analyzer (preconditions) */
#define DQ_E_UNSUPPORTED (-3) /* predicate outside the GPU grammar: route to the fallback */
#define DQ_E_HIP (-4)         /* HIP runtime / kernel failure */
#define DQ_E_OOM (-5)         /* device allocation failed */
#define DQ_E_STATE (-6)       /* state algebra misuse (op mismatch, bad byte image) */

/* Column physical types (Arrow layouts) and the Spark SQL types they carry.  The numeric types are the ones
 * Preconditions.isNumeric accepts (analyzers/Analyzer.scala:322-334): F64 / F32 / I64 / I32 / I16 / I8 /
 * DECIMAL128.  Values are converted to double as Spark casts them (exactly, or for a decimal correctly rounded:
 * Decimal.toDouble; Sum of an integral type is Spark's wrapping LongType sum, of a decimal the exact decimal sum
 * cast at the end); ApproxCountDistinct hashes each type as Spark 2.2's XxHash64Function does: hashLong for
 * LongType / TimestampType / DoubleType (doubleToLongBits) / DecimalType of precision <= 18 (the unscaled long),
 * hashInt for IntegerType / ShortType / ByteType / DateType (the value widened to int), FloatType
 * (floatToIntBits) and BooleanType (1 / 0), hashUnsafeBytes of BigInteger.toByteArray for a wider DecimalType.
 * BOOL / DATE32 / TIMESTAMP are not numeric: Completeness, Size, ApproxCountDistinct, DataType and IS [NOT] NULL
 * atoms (BOOL also = / != against TRUE / FALSE).  A DECIMAL128 type code carries its precision (1..38) and scale
 * (0..precision): DQ_DECIMAL128(p, s); every other code is its enum value alone. */
enum dq_type {
  DQ_TYPE_F64 = 1,        /* DoubleType: 8-byte values */
  DQ_TYPE_I64 = 2,        /* LongType: 8-byte values */
  DQ_TYPE_I32 = 3,        /* IntegerType: 4-byte values */
  DQ_TYPE_UTF8 = 4,       /* StringType: int32 offsets[n+1] + data bytes */
  DQ_TYPE_LARGE_UTF8 = 5, /* StringType with int64 offsets[n+1] (chunks > 2 GiB) */
  DQ_TYPE_F32 = 6,        /* FloatType: 4-byte values */
  DQ_TYPE_I16 = 7,        /* ShortType: 2-byte values */
  DQ_TYPE_I8 = 8,         /* ByteType: 1-byte values */
  DQ_TYPE_BOOL = 9,       /* BooleanType: LSB-first bit-packed values (Arrow `b`), bit 0 = row 0 of the chunk */
  DQ_TYPE_DATE32 = 10,    /* DateType: int32 days since 1970-01-01 (Arrow `tdD`) */
  DQ_TYPE_TIMESTAMP = 11, /* TimestampType: int64 microseconds since the epoch (Arrow `tsu:<timezone>`) */
  DQ_TYPE_DECIMAL128 = 12,/* DecimalType(p, s): 16-byte little-endian two's-complement unscaled values (Arrow
                             `d:p,s` / `d:p,s,128`); use the code DQ_DECIMAL128(p, s) */
  DQ_TYPE_DICT_UTF8 = 13  /* StringType carried as int32 indices into a dictionary of strings (Arrow dictionary
                             arrays).  The dictionary's bytes never reach dq_scan: a view passes the indices in
                             `values`, their bitmap in `validity`, the dictionary's entry words (dq_dict_entries,
                             uint32 each, device) in `offsets` and the number of entries in `reserved`.  A plan
                             takes such a column as col_a of COMPLETENESS / APPROX_COUNT_DISTINCT / DATATYPE (with
                             or without a `where` over other columns); any other use is DQ_E_UNSUPPORTED: decode
                             it (dq_dict_decode) and pass the UTF8 column */
};
#define DQ_TYPE_MAX 13
#define DQ_DECIMAL128(p, s) (DQ_TYPE_DECIMAL128 | ((p) << 8) | ((s) << 16))
#define DQ_TYPE_BASE(t) ((t) & 0xFF)
#define DQ_DECIMAL_PRECISION(t) (((t) >> 8) & 0xFF)
#define DQ_DECIMAL_SCALE(t) (((t) >> 16) & 0xFF)

/* Analyzer ops: the GPU-eligible ScanShareableAnalyzers. */
enum dq_op {
  DQ_OP_SIZE = 1,                 /* analyzers/Size.scala:36-48 */
  DQ_OP_COMPLETENESS = 2,         /* analyzers/Completeness.scala:26-46 */
  DQ_OP_COMPLIANCE = 3,           /* analyzers/Compliance.scala:37-53 */
  DQ_OP_SUM = 4,                  /* analyzers/Sum.scala:36-52 */
  DQ_OP_MEAN = 5,                 /* analyzers/Mean.scala:36-54 */
  DQ_OP_STDDEV = 6,               /* analyzers/StandardDeviation.scala:47-73 */
  DQ_OP_MIN = 7,                  /* analyzers/Minimum.scala:36-53 */
  DQ_OP_MAX = 8,                  /* analyzers/Maximum.scala:36-53 */
  DQ_OP_CORRELATION = 9,          /* analyzers/Correlation.scala:65-105 */
  DQ_OP_APPROX_COUNT_DISTINCT = 10,/* analyzers/ApproxCountDistinct.scala:47-64 */
  DQ_OP_DATATYPE = 11,            /* analyzers/DataType.scala:152-183, catalyst/StatefulDataType.scala:26-83 */
  DQ_OP_PATTERN_MATCH = 12        /* analyzers/PatternMatch.scala:37-56: pred_root = a DQ_PRED_REGEX node
                                     (mode DQ_REGEX_EXTRACT_NONEMPTY); state NumMatchesAndCount */
};

typedef struct dq_column_desc {
  int32_t type;     /* enum dq_type */
  int32_t nullable; /* 0: validity bitmaps are ignored (may be NULL) */
} dq_column_desc;

/* One analyzer instance (a Scala case class).  Unused fields = -1. */
typedef struct dq_analyzer_spec {
  int32_t op;         /* enum dq_op */
  int32_t col_a;      /* column index (COMPLETENESS..MAX, ACD, DATATYPE, CORRELATION first column) */
  int32_t col_b;      /* CORRELATION second column */
  int32_t pred_root;  /* COMPLIANCE predicate: root index into the predicate node pool */
  int32_t where_root; /* optional `where` filter root, -1 = none */
} dq_analyzer_spec;

/* Predicate IR: a pool of nodes, referenced by index.  This is the lowered form of the Spark SQL
 * expressions deequ builds with expr(...) (Check.scala:538-548, 670-871): comparisons with SQL
 * three-valued logic, AND / OR / NOT, IS [NOT] NULL, COALESCE(column, literal).  Literal typing
 * follows Spark 2.2: `3` -> LIT_INT, `3.0` -> LIT_DECIMAL (exact), `3e0` -> LIT_DOUBLE. */
enum dq_pred_kind {
  DQ_PRED_COLUMN = 1,      /* a = column index */
  DQ_PRED_LIT_INT = 2,     /* i64 */
  DQ_PRED_LIT_DECIMAL = 3, /* i64 = unscaled value, cmp = scale (value = i64 / 10^scale) */
  DQ_PRED_LIT_DOUBLE = 4,  /* f64 */
  DQ_PRED_LIT_NULL = 5,
  DQ_PRED_LIT_BOOL = 6,    /* i64 = 0 / 1 */
  DQ_PRED_CMP = 7,         /* a CMP b, cmp = enum dq_cmp */
  DQ_PRED_AND = 8,         /* a AND b */
  DQ_PRED_OR = 9,          /* a OR b */
  DQ_PRED_NOT = 10,        /* NOT a */
  DQ_PRED_IS_NULL = 11,    /* a IS NULL */
  DQ_PRED_IS_NOT_NULL = 12,/* a IS NOT NULL */
  DQ_PRED_COALESCE = 13,   /* COALESCE(a, b): a = COLUMN node, b = literal node */
  DQ_PRED_REGEX = 14,      /* regex over a UTF8 column: a = COLUMN node, i64 = index into the plan's
                              patterns (dq_plan_create_ex), cmp = enum dq_regex_mode;
                              string equality / IN lists lower to mode DQ_REGEX_FULL */
  DQ_PRED_EXPR = 15        /* an arithmetic operand (dq_pred_pool_add only): a = index into the pool's expression
                              list (dq_pred_pool_expr), cmp = its result type (enum dq_type).  A plan never sees
                              this kind: the caller materialises the expression as a derived column (dq_expr_eval)
                              and hands the node over as DQ_PRED_COLUMN of that column */
};
/* DQ_PRED_REGEX semantics (java.util.regex Matcher.find on the value's code points):
 *   DQ_REGEX_RLIKE            `col RLIKE p`: NULL on a NULL value, else TRUE iff find() succeeds;
 *   DQ_REGEX_EXTRACT_NONEMPTY `CASE WHEN regexp_extract(col, p, 0) != '' THEN 1 ELSE 0` as PatternMatch
 *                             builds it (PatternMatch.scala:48-49): FALSE on NULL, never NULL; patterns
 *                             that can match the empty string are DQ_E_UNSUPPORTED (fallback). */
enum dq_regex_mode { DQ_REGEX_RLIKE = 0, DQ_REGEX_EXTRACT_NONEMPTY = 1, DQ_REGEX_FULL = 2 };
/*   DQ_REGEX_FULL             the whole value is in L(p) (no search, no `^` / `$` handling): string
 *                             equality `col = 'v'` / `col IN ('a', 'b')` lowered to p = (?:a|b) with
 *                             escaped literals; NULL on a NULL value. */
enum dq_cmp { DQ_CMP_LT = 1, DQ_CMP_LE = 2, DQ_CMP_GT = 3, DQ_CMP_GE = 4, DQ_CMP_EQ = 5, DQ_CMP_NE = 6 };

typedef struct dq_pred_node {
  int32_t kind;
  int32_t a;
  int32_t b;
  int32_t cmp;
  int64_t i64;
  double f64;
} dq_pred_node;

/* One column of one row chunk.  All pointers are DEVICE pointers (HBM-resident, e.g. uploaded
 * Spark/Arrow batches).  values: 16-byte aligned; validity: Arrow LSB-first bitmap, 4-byte
 * aligned, bit 0 = row 0 of the chunk, NULL when the column has no nulls.  UTF8 columns pass the
 * data bytes in `values` and the offsets (n_rows + 1 entries) in `offsets`. */
typedef struct dq_column_view {
  const void* values;
  const uint8_t* validity;
  const void* offsets;
  int64_t reserved; /* must be 0 (DQ_TYPE_DICT_UTF8: the number of dictionary entries) */
} dq_column_view;

/* ---- Dictionary-encoded string columns (DQ_TYPE_DICT_UTF8) ----
 * dq_dict_entries: one pass over a dictionary's n_entries strings (dict: a DQ_TYPE_UTF8 / DQ_TYPE_LARGE_UTF8 view
 * of them, device pointers; validity NULL = no NULL entry) that writes one uint32 entry word per entry to
 * entries_out (device, 4-byte aligned), asynchronously on hip_stream:
 *   bits 0..8    the entry's HLL register index: the top 9 bits of XXH64(bytes, seed 42)
 *   bits 9..14   its rank pw (1..56) as StatefulHyperloglogPlus computes it from the same hash
 *   bits 15..17  its StatefulDataType class: 1 FRACTIONAL, 2 INTEGRAL, 3 BOOLEAN, 4 STRING
 *   bit 18       1 for a non-NULL entry; a NULL entry's word is 0
 *   bits 19..31  reserved, written 0
 * The word does not depend on a plan: compute a dictionary's table once and pass it to every plan and chunk that
 * sees the dictionary.  In dq_scan a row of such a column is NULL iff its validity bit is 0, its entry is NULL or
 * its index lies outside [0, reserved) (such a row's entry is never loaded; validate indices on the host --
 * dq_dict_check_indices); entries no row refers to influence nothing, duplicate entries are harmless.
 * dq_dict_decode: the plain string column (of dict_type) a dictionary column stands for, in the layout dq_take_rows
 * writes: out_offsets n_rows + 1 offsets of dict's width, out_values the bytes (values_capacity = its size),
 * out_validity (NULL: not wanted) ceil(n_rows / 64) 64-bit words.  indices: values = int32 indices, validity = their
 * bitmap or NULL.  With out_values NULL the call writes the offsets and *data_bytes only (the sizing call).
 * Synchronises hip_stream.
 * dq_dict_count: the grouping of a dictionary column from its indices alone.  indices: a DQ_TYPE_DICT_UTF8 view as
 * dq_scan takes it (int32 indices, their bitmap or NULL, the entry words in `offsets`, the number of entries D in
 * `reserved`); counts: int64[D] on the device, 8-byte aligned.  Adds to counts[e] the number of rows among the
 * n_rows (< 2^31) that carry index e; a row counts when it is non-NULL by dq_scan's rule above (validity bit set,
 * index inside [0, D), entry non-NULL) -- any other row is counted nowhere, and nothing outside counts[0, D) is
 * written.  The call ACCUMULATES: the caller zeroes counts once, and the chunks that share a dictionary add into one
 * array.  Asynchronous on hip_stream.  dq_freq_build_weighted over the dictionary's entries with these counts as
 * weights is the frequency table dq_freq_build makes of the decoded column.
 * Measurement hook, not for production: with the environment variable DQ_DICT_COUNT_AB=global (exactly that value,
 * read on every call) a dictionary of at most 4096 entries is counted with global atomic adds, as larger ones are,
 * instead of in LDS -- the same counts, 17x to 1500x slower.  Any other value, or no variable, changes
 * nothing. */
dq_status dq_dict_count(const dq_column_view* indices, int64_t n_rows, int64_t* counts, int32_t device,
                        void* hip_stream);
dq_status dq_dict_entries(int32_t dict_type, const dq_column_view* dict, int64_t n_entries, uint32_t* entries_out,
                          int32_t device, void* hip_stream);
dq_status dq_dict_decode(int32_t dict_type, const dq_column_view* dict, int64_t n_entries,
                         const dq_column_view* indices, int64_t n_rows, void* out_values, int64_t values_capacity,
                         uint8_t* out_validity, void* out_offsets, int64_t* data_bytes, int32_t device,
                         void* hip_stream);

/* ---- Binned histograms: a numeric column counted into declared bins (additions under ABI 6) ----
 * dq_bins_create: edges (host): n_edges = k + 1 finite, strictly increasing binary64 numbers giving k bins,
 * 1 <= k <= 4096; the handle keeps a device copy of them on `device`.  Fewer than 2 edges, a non-finite edge
 * ("edges[i] is not finite") or one not above its predecessor ("edges[i] is not greater than edges[i-1]") is
 * DQ_E_INVALID; more than 4096 bins is DQ_E_UNSUPPORTED.  dq_bins_destroy frees the handle (NULL: nothing); it waits
 * for the device's outstanding work, so a dq_bin_count still running has finished with the edges.
 * dq_bin_count: counts: int64[n_edges + 2] on the device, 8-byte aligned, the slots [below, bin 0 .. bin k-1, above,
 * nan].  Adds to counts[slot] the number of rows among the n_rows (< 2^31) of col (a view of `type`: values, validity
 * bitmap or NULL) in that slot.  The slot rule: a value is converted to binary64 as Spark's cast does (f32 widens
 * exactly, integers round to nearest-even, a decimal is the correctly rounded quotient), then, with e the stored edges,
 *     e[i] <= x < e[i+1]            bin i
 *     x == e[k]                     the last bin, which is closed on the right
 *     x < e[0], including -inf      below
 *     x > e[k], including +inf      above
 *     NaN                           nan
 * -0.0 compares as 0.0.  NULL rows are in no slot.  The bin of a value is defined only by comparisons against the
 * stored edges, never by a division.
 * The call ACCUMULATES, as dq_dict_count does: the caller zeroes counts once and the chunks of a column add into one
 * array; nothing outside counts[0, n_edges + 2) is written.  Asynchronous on hip_stream.  n_rows == 0: DQ_OK, no
 * launch.  type: DQ_TYPE_F64 / F32 / I64 / I32 / I16 / I8 or DQ_DECIMAL128(p, s) of any precision; BOOL, DATE32,
 * TIMESTAMP, the string types and DICT_UTF8 are DQ_E_UNSUPPORTED with the type named, before any launch.  A device
 * other than the handle's, a NULL or misaligned buffer, reserved != 0: DQ_E_INVALID.  dq_freq_build_weighted over a
 * string column of the k + 3 slot labels with these counts as weights is the frequency table Spark's groupBy over a
 * binning UDF returning those labels builds. */
typedef struct dq_bins dq_bins;
dq_status dq_bins_create(const double* edges, int32_t n_edges, int32_t device, dq_bins** out);
void dq_bins_destroy(dq_bins* bins);
dq_status dq_bin_count(const dq_bins* bins, int32_t type, const dq_column_view* col, int64_t n_rows, int64_t* counts,
                       int32_t device, void* hip_stream);

/* Host: widen n indices of index_type (DQ_TYPE_I8 / I16 / I32, or the unsigned widths as -DQ_TYPE_I8 / -DQ_TYPE_I16)
 * to int32 in out (may be NULL: check only) and check 0 <= index < n_entries for every row whose validity bit
 * (LSB-first bitmap starting at bit validity_bit of validity[0]; NULL: every row) is set.  DQ_E_INVALID names the
 * first offending row. */
dq_status dq_dict_check_indices(int32_t index_type, const void* indices, int64_t n, const uint8_t* validity,
                                int32_t validity_bit, int64_t n_entries, int32_t* out);

/* ---- Host ingestion: Arrow C Data Interface batches -> device chunks (no JVM in the data path) ----
 * The Arrow C Data Interface ABI (arrow.apache.org/docs/format/CDataInterface.html), as exported by
 * Spark's Arrow conversion, pyarrow (Array._export_to_c), arrow-rs / arrow-cpp. */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
#define ARROW_FLAG_DICTIONARY_ORDERED 1
#define ARROW_FLAG_NULLABLE 2
#define ARROW_FLAG_MAP_KEYS_SORTED 4
struct ArrowSchema {
  const char* format;
  const char* name;
  const char* metadata;
  int64_t flags;
  int64_t n_children;
  struct ArrowSchema** children;
  struct ArrowSchema* dictionary;
  void (*release)(struct ArrowSchema*);
  void* private_data;
};
struct ArrowArray {
  int64_t length;
  int64_t null_count;
  int64_t offset;
  int64_t n_buffers;
  int64_t n_children;
  const void** buffers;
  struct ArrowArray** children;
  struct ArrowArray* dictionary;
  void (*release)(struct ArrowArray*);
  void* private_data;
};
#endif /* ARROW_C_DATA_INTERFACE */

/* One column's HOST buffers (what dq_arrow_import finds in an ArrowArray; the caller keeps the Arrow
 * array alive until dq_upload returns).  Byte counts are the bytes dq_upload writes to the device. */
typedef struct dq_host_column {
  int32_t type;            /* enum dq_type */
  int32_t nullable;        /* 1 iff validity != NULL */
  int64_t n_rows;
  const void* values;      /* fixed-width values / UTF8 data bytes (from the first string's first byte) */
  const uint8_t* validity; /* LSB-first bitmap: row 0 is bit validity_bit of byte 0; NULL = no nulls */
  const void* offsets;     /* UTF8: n_rows + 1 offsets; offsets[0] == offset_base */
  int64_t value_bytes, validity_bytes, offset_bytes;
  int64_t offset_base;     /* subtracted from every offset by dq_upload (an Arrow slice's first offset) */
  int32_t validity_bit;    /* 0..7: dq_upload shifts the bitmap so that row 0 lands on bit 0 */
  int32_t reserved;
} dq_host_column;
/* Map an exported Arrow array (formats g = float64, f = float32, l = int64, i = int32, s = int16, c = int8,
 * b = boolean, tdD = date32, tsu:<tz> = timestamp[us], d:p,s[,128] = decimal128 (precision <= 38, scale 0..p),
 * u = utf8, U = large_utf8) to host column buffers; slices
 * at any row offset are rebased by dq_upload (a boolean slice's value bits are shifted like its validity:
 * validity_bit holds the slice's bit offset of both bitmaps).  DQ_E_UNSUPPORTED: other
 * types, nested / dictionary arrays.  DQ_E_INVALID: a required buffer is NULL (an empty array may
 * export NULL buffers: it maps to an empty column). */
dq_status dq_arrow_import(const struct ArrowSchema* schema, const struct ArrowArray* array, dq_host_column* out);
/* A dictionary-encoded Arrow array is two columns.  *indices (index formats c, s, i, C, S; slices honoured as above):
 * a host column of type DQ_TYPE_DICT_UTF8 whose `values` are the Arrow index bytes, `reserved` their type as
 * dq_dict_check_indices names it (DQ_TYPE_I8 / I16 / I32, negated for the unsigned formats), `offset_base` the number
 * of dictionary entries and value_bytes = 4 * n_rows: dq_upload widens the indices to int32 while it copies them into
 * the pinned slot and, in that loop, checks 0 <= index < entries for every valid row -- a violation is DQ_E_INVALID
 * naming the row, and nothing is uploaded.  The device view dq_upload returns holds the int32 indices and their
 * validity; the caller adds the entry table (`offsets`) and the entry count (`reserved`).  *dictionary (value formats
 * u, U; a sliced dictionary included): an ordinary UTF8 / LARGE_UTF8 host column of the entries, uploaded once per
 * dictionary.  DQ_E_UNSUPPORTED: other index widths, other value types, a nested dictionary. */
dq_status dq_arrow_import_dictionary(const struct ArrowSchema* schema, const struct ArrowArray* array,
                                     dq_host_column* indices, dq_host_column* dictionary);
/* Pinned, n-buffered host -> device upload.  dq_upload copies one chunk's columns (CPU threads: host ->
 * pinned slot; DMA on the uploader's own stream: pinned -> device slot) and returns device views of the
 * slot, valid until the slot is reused n_slots uploads later.  Before scanning, make the scan stream wait
 * for the copy (dq_upload_fence); after enqueueing the scan, record the slot's release on that stream
 * (dq_upload_release) -- the DMA of a later chunk into the same slot waits for it.  So with n_slots = 2 the
 * upload of chunk k + 1 overlaps the scan of chunk k.  host_threads <= 0: up to 16 CPU threads. */
typedef struct dq_uploader dq_uploader;
dq_status dq_uploader_create(int32_t device, int32_t n_slots, int64_t slot_bytes, int32_t host_threads,
                             dq_uploader** out);
dq_status dq_upload(dq_uploader* u, const dq_host_column* cols, int32_t n_cols, dq_column_view* dev_views);
dq_status dq_upload_fence(dq_uploader* u, void* hip_stream);
dq_status dq_upload_release(dq_uploader* u, void* hip_stream);
dq_status dq_upload_sync(dq_uploader* u);
void dq_uploader_destroy(dq_uploader* u);
/* Upload into buffers the caller owns (additions under ABI 6).  dq_upload_to copies one chunk's columns through the
 * uploader's next pinned slot -- the same CPU threads and the same copy stream as dq_upload -- and DMAs every buffer
 * to its destination: device memory the caller allocated (one dq_upload_dest per column: the addresses and the WHOLE
 * sizes of its values / validity / offsets buffers, padding included; a NULL address = the column has no such
 * buffer).  No device slot is used and nothing is copied on the device afterwards; dq_upload_fence orders a stream
 * behind the copy as it does for dq_upload, dq_upload_release is not needed (both kinds of upload may share an
 * uploader).  What arrives is the canonical column image, not the producer's bytes:
 *   - a NULL row's value is 0, a NULL boolean false, a NULL string empty (bytes under a NULL slot are dropped and the
 *     offsets rebuilt), a NULL row's dictionary index 0;
 *   - bitmap bits past the last row are 0; a destination with a validity buffer whose source has none gets all ones;
 *     a destination without one whose source holds a NULL is DQ_E_INVALID naming column and row;
 *   - every byte of a destination behind its rows is 0;
 *   - dictionary indices are widened and range-checked as by dq_upload; a DECIMAL128 value of a valid row with
 *     |unscaled| >= 10^precision is DQ_E_INVALID naming the column and the first such row (dq_arrow_import and
 *     dq_upload do not check it).  On an error nothing is uploaded.
 * dq_upload_payload gives, per column, the value bytes the rows need (a string column: the bytes of its non-NULL rows;
 * otherwise value_bytes), and checks each column's byte counts and string offsets (ascending, inside the data), so a
 * caller can size the destinations.  dq_upload_stage is dq_upload_to's host half with no device in it: it writes
 * every destination's image into `staging` (host memory of staging_bytes) at positions[3 * c + {0 values, 1 validity,
 * 2 offsets}] (-1: no such buffer; each 256-byte aligned, dests[c]'s sizes long; the destination addresses are only
 * tested for NULL) and the bytes used to *staged_bytes.  host_threads <= 0: up to 16 CPU threads. */
typedef struct dq_upload_dest {
  void* values;
  void* validity;
  void* offsets;
  int64_t value_bytes, validity_bytes, offset_bytes;
} dq_upload_dest;
dq_status dq_upload_payload(const dq_host_column* cols, int32_t n_cols, int64_t* value_bytes);
dq_status dq_upload_stage(const dq_host_column* cols, int32_t n_cols, const dq_upload_dest* dests, void* staging,
                          int64_t staging_bytes, int32_t host_threads, int64_t* positions, int64_t* staged_bytes);
dq_status dq_upload_to(dq_uploader* u, const dq_host_column* cols, int32_t n_cols, const dq_upload_dest* dests);

/* The aggregation-result slots of one analyzer (the reference's Row slice at its offset,
 * SURVEY §8b).  has_value[i] = SQL non-null flag of slot i; single-slot analyzers mirror slot 0
 * into has_value[1].  fromAggregationResult yields Some(state) iff both flags are 1 (and, for
 * StandardDeviation / Correlation, n > 0). */
typedef struct dq_state {
  int32_t op;           /* enum dq_op */
  uint8_t has_value[2];
  uint8_t integral;     /* SUM / MEAN of an integral column (1): `partial` holds Spark's int64 partial-aggregate
                           sum (wraps like Spark's LongType sum); dq_state_combine adds the partials and
                           casts, so row shards combine exactly as Spark's partial -> final merge.  Of a
                           DECIMAL128 column (2): `partial` / `partial_hi` hold the exact decimal sum (128-bit,
                           unscaled at scale `dec_scale`), `guard` the fp64 sum of the values (it tells a sum
                           past 2^127 from its wrapped image); an unscaled sum of 10^dec_digits or more (Spark
                           2.2's sum type DecimalType(min(38, p + 10), s) overflows: a NULL sum) makes the state
                           undefined */
  uint8_t reserved;
  union {
    struct { int64_t num_matches; } size;                     /* NumMatches */
    struct { int64_t num_matches; int64_t count; } ratio;     /* NumMatchesAndCount (Completeness, Compliance, PatternMatch) */
    struct { double sum; int64_t partial; int64_t partial_hi; double guard; int32_t dec_scale, dec_digits; } sum;
    /* SumState (+ integral / decimal partial) */
    struct { double sum; int64_t count; int64_t partial; int64_t partial_hi; double guard; int32_t dec_scale, dec_digits; } mean;
    /* MeanState (+ partial) */
    struct { double n, avg, m2; } stddev;                     /* StandardDeviationState */
    struct { double value; } minmax;                          /* MinState / MaxState */
    struct { double n, x_avg, y_avg, ck, x_mk, y_mk; } corr;  /* CorrelationState */
    struct { int64_t words[52]; } hll;                        /* ApproxCountDistinctState */
    struct { int64_t num_null, num_fractional, num_integral, num_boolean, num_string; } dtype;  /* DataTypeHistogram */
  } u;
} dq_state;

typedef struct dq_plan dq_plan;

/* Library identity. */
int32_t dq_abi_version(void);
const char* dq_last_error(void);

/* Plan: validate + dedup the analyzers, lower predicates, allocate device partial states. */
dq_status dq_plan_create(const dq_analyzer_spec* specs, int32_t n_specs, const dq_column_desc* schema,
                         int32_t n_cols, const dq_pred_node* pred_pool, int32_t n_pred, int32_t device,
                         dq_plan** out);
/* As dq_plan_create, plus the UTF-8 regex patterns DQ_PRED_REGEX nodes refer to (i64 = index).
 * Each pattern is compiled on the host into a byte-level search DFA (java.util.regex subset:
 * literals, `.`, classes, \d \s \w, groups, alternation, greedy / lazy quantifiers, leading `^`,
 * trailing `$`); backreferences, look-around, \b and inline flags are DQ_E_UNSUPPORTED. */
dq_status dq_plan_create_ex(const dq_analyzer_spec* specs, int32_t n_specs, const dq_column_desc* schema,
                            int32_t n_cols, const dq_pred_node* pred_pool, int32_t n_pred,
                            const char* const* patterns, int32_t n_patterns, int32_t device, dq_plan** out);
/* How the predicate pass of a plan runs (dq_plan_options.pred_pass).  AUTO: the kernel generated and
 * compiled for the plan's program when the generator takes it (numeric comparisons; Spark's whole-stage
 * code generation of the same expressions), else -- or when the compile fails -- the interpreter, with
 * the reason in dq_plan_pred_compiled's note.  A kernel not yet in the process's cache is obtained (from the
 * disk code-object cache, else compiled by hipRTC) on a background thread: plan creation does not wait for
 * it, the scan runs the interpreter until the kernel is ready and the compiled kernel from the next chunk on
 * (bit-identical results either way; dq_plan_pred_wait blocks for it).  INTERPRETER: always the interpreter (the reference
 * implementation the compiled kernel is tested against).  COMPILED: the compiled kernel (plan creation
 * waits for the compile) or DQ_E_UNSUPPORTED from dq_plan_create_opts (reason in dq_last_error) -- no
 * silent fallback. */
enum dq_pred_pass { DQ_PRED_PASS_AUTO = 0, DQ_PRED_PASS_INTERPRETER = 1, DQ_PRED_PASS_COMPILED = 2 };
typedef struct dq_plan_options {
  int32_t struct_size;  /* sizeof(dq_plan_options) as the caller was compiled (fields past it: defaults) */
  int32_t pred_pass;    /* enum dq_pred_pass */
  int32_t reserved[6];  /* 0 */
} dq_plan_options;
/* As dq_plan_create_ex with options (NULL = all defaults).  Replaces AnalysisRunner.runScanningAnalyzers'
 * plan step (AnalysisRunner.scala:279-326): one plan per run, created before the first chunk.
 * Like the reference's single data.agg (AnalysisRunner.scala:293-303) a plan takes any number of analyzers.
 * One fused pass holds at most 64 columns, 32 distinct predicates (Compliance predicates, `where` filters,
 * Completeness-with-`where` NOT NULL tests), 32 predicate counters, 8 distinct `where` filters of value
 * analyzers (Sum ... ApproxCountDistinct, Correlation), 256 column tasks and a 96-instruction predicate
 * program; a larger set is split -- analyzers grouped by their columns -- into several fused passes over
 * the same chunks, each reading only its own columns (dq_plan_explain shows the split).  Only a spec that
 * exceeds a limit by itself (e.g. a predicate over more than 64 columns or nested deeper than the
 * 16-entry operand stack) fails, with DQ_E_UNSUPPORTED: route it to the fallback set. */
dq_status dq_plan_create_opts(const dq_analyzer_spec* specs, int32_t n_specs, const dq_column_desc* schema,
                              int32_t n_cols, const dq_pred_node* pred_pool, int32_t n_pred,
                              const char* const* patterns, int32_t n_patterns, const dq_plan_options* opts,
                              int32_t device, dq_plan** out);
/* Compile a pattern without a GPU: DFA size (or the DQ_E_UNSUPPORTED reason in dq_last_error), and
 * the host walk of the same DFA over n values (UTF-8 bytes data[offsets[r] .. offsets[r + 1]))
 * for tests of the compiler; out[r] = 1 iff the value matches under `mode` (NULLs are the caller's). */
dq_status dq_regex_info(const char* pattern, int32_t mode, int32_t* n_states, int32_t* n_classes);
dq_status dq_regex_match_host(const char* pattern, int32_t mode, const uint8_t* data, const int64_t* offsets,
                              int64_t n, uint8_t* out);
/* Predicate compiler: Spark SQL predicate text -> the IR above, on the host (replaces Spark's expr(...)
 * parse of the strings deequ builds: Analyzer.scala:385-408 `where`, Check.scala:538-548, 670-871).
 * A pool holds the table's columns (name, enum dq_type; node column indices are positions in that list)
 * and accumulates the nodes and regex patterns of every root of one plan, ready for dq_plan_create_ex.
 * Grammar: OR / AND / NOT, comparisons < <= > >= = == != <>, IS [NOT] NULL, COALESCE(a, b), parentheses,
 * numeric literals typed as Spark 2.2 (`3` int, `3.0` exact decimal, `3e0` double), NULL / TRUE / FALSE,
 * string (in)equality and [NOT] IN ('a', ...) on a string column (lowered to a DQ_REGEX_FULL node), and arithmetic
 * (+ - * / %, unary minus) on each side of a comparison and under IS [NOT] NULL ("Arithmetic operands" below).
 * dq_pred_pool_add: DQ_E_UNSUPPORTED (reason in dq_last_error) for text outside that grammar -- string
 * ordering, a numeric comparison of a string column, LIKE / RLIKE / BETWEEN, function calls, typed literal
 * suffixes, escapes -- i.e. route the analyzer to the Spark fallback; DQ_E_INVALID "no such column: x" for
 * an unknown column.  A failed add leaves the pool unchanged.  dq_pred_pool_add_regex appends a
 * DQ_PRED_REGEX root over `column` (PatternMatch; DQ_E_UNSUPPORTED outside the DFA subset).  Node and
 * pattern arrays stay valid until the next add or destroy. */
typedef struct dq_pred_pool dq_pred_pool;
dq_status dq_pred_pool_create(const char* const* names, const int32_t* types, int32_t n_cols, dq_pred_pool** out);
dq_status dq_pred_pool_add(dq_pred_pool* pool, const char* sql, int32_t* root);
dq_status dq_pred_pool_add_regex(dq_pred_pool* pool, int32_t column, const char* pattern, int32_t mode, int32_t* root);
int32_t dq_pred_pool_size(const dq_pred_pool* pool);
const dq_pred_node* dq_pred_pool_nodes(const dq_pred_pool* pool);
int32_t dq_pred_pool_num_patterns(const dq_pred_pool* pool);
const char* const* dq_pred_pool_patterns(const dq_pred_pool* pool);
void dq_pred_pool_destroy(dq_pred_pool* pool);

/* ---- Arithmetic operands: + - * / % over numeric columns (additions under ABI 6) ----
 * Each side of a comparison, and the operand of IS [NOT] NULL, is an arithmetic expression:
 *     operand := sum
 *     sum     := term ( (+ | -) term )*
 *     term    := unary ( (* | / | %) unary )*
 *     unary   := - unary | primary
 *     primary := column | `column` | number | ( sum ) | the other operands of the grammar above
 * A primary alone lowers exactly as before, and `- number` stays a literal.  An operand with at least one operator
 * and at least one column becomes one DQ_PRED_EXPR node whose `a` indexes the pool's expression list; equal canonical
 * texts (fully parenthesised, columns in backticks) share one entry within a pool.  The caller evaluates every
 * entry once per chunk with dq_expr_eval into a derived column and passes the node to the plan as DQ_PRED_COLUMN of
 * that column, so every comparison rule of the plan applies to the result unchanged.
 *
 * Semantics (Spark 2.2, non-ANSI):
 *   types      Byte < Short < Int < Long < Float < Double (I8 < I16 < I32 < I64 < F32 < F64)
 *   literals   an integer literal is IntegerType if it fits, else LongType; `3e0` is Double; a decimal literal
 *              (`2.5`) next to a Float or Double operand is cast to Double
 *   + - * %    both sides are cast to the wider type, which is the result type
 *   integral   results wrap in two's complement at the result width: Byte 127 + 1 = -128, Int MIN % -1 = 0
 *   Float      binary32 arithmetic, rounded after each operation; Double: binary64.  No contraction: a * b + c is
 *              two roundings, never an FMA
 *   /          both sides are cast to Double (7 / 2 = 3.5); a divisor == 0, of either sign of zero, gives NULL
 *   %          NULL on a zero divisor; integrals: Java's truncated remainder; Float / Double: Java %, i.e. fmod
 *   unary -    keeps the type and wraps
 *   NULL       any NULL operand gives NULL
 *   result     a column of the result type (I8 I16 I32 I64 F32 F64), nullable whenever an input is or when the
 *              program contains / or %
 * DQ_E_UNSUPPORTED, each with the reason in dq_last_error: a non-numeric operand (bool, date, timestamp, string),
 * a decimal(p,s) column inside arithmetic, a decimal literal combined with an integral operand or another decimal
 * literal (decimal arithmetic), COALESCE or NULL inside arithmetic, an operator expression without a column,
 * function calls, BETWEEN, IN over numbers or over an expression, an expression used as a boolean, and a program
 * beyond the limits below.
 *
 * A program is postfix over a value stack.  Every instruction carries the type it produces: COL pushes column
 * `arg` of the program's column list (type = the column's), LIT pushes literal `arg` (I32 / I64 / F64), CAST widens
 * the top of the stack to `type`, NEG negates it at `type`; ADD SUB MUL MOD pop b then a, both of `type`, and push
 * a op b; DIV the same with `type` = F64.  The compiler emits every cast, so an evaluator needs no type rules. */
#define DQ_EXPR_MAX_COLUMNS 8   /* distinct source columns of one expression */
#define DQ_EXPR_MAX_INSTRS 32   /* program length */
#define DQ_EXPR_MAX_LITERALS 16 /* literals of one program (the program length binds first) */
#define DQ_EXPR_MAX_STACK 8     /* value-stack depth (the kernel holds the stack in registers) */
enum dq_expr_op {
  DQ_EXPR_COL = 1, DQ_EXPR_LIT = 2, DQ_EXPR_CAST = 3, DQ_EXPR_NEG = 4,
  DQ_EXPR_ADD = 5, DQ_EXPR_SUB = 6, DQ_EXPR_MUL = 7, DQ_EXPR_DIV = 8, DQ_EXPR_MOD = 9
};
typedef struct dq_expr_instr {
  int32_t op;   /* enum dq_expr_op */
  int32_t arg;  /* COL: index into columns[]; LIT: index into literals[]; else 0 */
  int32_t type; /* enum dq_type of the value the instruction leaves on the stack */
  int32_t reserved;
} dq_expr_instr;
typedef struct dq_expr_literal {
  int32_t type; /* DQ_TYPE_I32 / DQ_TYPE_I64: i64; DQ_TYPE_F64: f64 */
  int32_t reserved;
  int64_t i64;
  double f64;
} dq_expr_literal;
typedef struct dq_expr_program {
  int32_t n_instrs, n_columns, n_literals;
  int32_t result_type;  /* enum dq_type: I8 I16 I32 I64 F32 F64 */
  int32_t stack_depth;  /* the deepest the value stack gets */
  int32_t divides;      /* 1: the program holds / or %, so the result is nullable whatever the inputs are */
  dq_expr_instr instrs[DQ_EXPR_MAX_INSTRS];
  int32_t columns[DQ_EXPR_MAX_COLUMNS];      /* positions in the pool's column list, in first-use order */
  int32_t column_types[DQ_EXPR_MAX_COLUMNS]; /* their enum dq_type */
  dq_expr_literal literals[DQ_EXPR_MAX_LITERALS];
  const char* text;     /* canonical text; the pool's (dq_pred_pool_expr), unused by dq_expr_eval */
} dq_expr_program;
/* The expressions the pool's DQ_PRED_EXPR nodes refer to; a program stays valid until the pool is destroyed. */
int32_t dq_pred_pool_num_exprs(const dq_pred_pool* pool);
const dq_expr_program* dq_pred_pool_expr(const dq_pred_pool* pool, int32_t index);
/* Evaluate one program over n_rows rows into a derived column.  cols: prog->n_columns views, in the order of
 * prog->columns, of the fixed-width types prog->column_types names (values 16-byte aligned, n_rows elements;
 * validity NULL: no NULL row; offsets unused, reserved 0).  out_values: n_rows elements of the result type (16-byte
 * aligned); out_validity: ceil(n_rows / 64) 64-bit words (8-byte aligned; bits past n_rows are written 0); both
 * device, caller-allocated; every value and every word of the n_rows rows is written (a NULL row's value is 0),
 * nothing beyond them.  *nulls_out (host) = the NULL rows; the call synchronises hip_stream.  n_rows = 0: DQ_OK,
 * nothing written.  The program is checked first (limits, indices, the stack discipline and the type of every
 * operand): a malformed one, a NULL or misaligned buffer, n_rows < 0 or reserved != 0 are DQ_E_INVALID, a column
 * or result type outside the six numeric ones is DQ_E_UNSUPPORTED, and nothing is launched. */
dq_status dq_expr_eval(const dq_expr_program* prog, const dq_column_view* cols, int64_t n_rows, void* out_values,
                       uint64_t* out_validity, int32_t device, void* hip_stream, int64_t* nulls_out);
/* The same evaluation on the CPU, no device (tests of the compiler and of the rules): cols[k] = host pointers. */
dq_status dq_expr_eval_host(const dq_expr_program* prog, const dq_column_view* cols, int64_t n_rows, void* out_values,
                            uint64_t* out_validity, int64_t* nulls_out);
/* Launch on this hipStream_t from now on (NULL = the device null stream).  A new plan launches on its
   own non-blocking stream, which does not order against other streams: set the producer's stream. */
dq_status dq_plan_set_stream(dq_plan* plan, void* hip_stream);
/* Scan one chunk of rows (asynchronous on the plan's stream).  chunk_index must increase by one
 * per call starting at 0: chunk results are merged in that order, so results are deterministic. */
dq_status dq_scan(dq_plan* plan, const dq_column_view* cols, int64_t n_rows, int64_t chunk_index);
/* Synchronise and write one dq_state per spec (caller-allocated, n_specs entries).  The plan's device
 * accumulators come back through a small pinned host buffer the plan allocates on its first finish
 * (hipHostMalloc; freed by dq_plan_destroy). */
dq_status dq_finish(dq_plan* plan, dq_state* out_states);
/* Forget all scanned chunks (keeps allocations). */
dq_status dq_plan_reset(dq_plan* plan);
void dq_plan_destroy(dq_plan* plan);
/* Algorithmic HBM bytes one scan of n_rows reads (each needed buffer counted once; UTF8 data
 * bytes are data-dependent and reported by the caller). */
int64_t dq_plan_bytes_per_row_x1000(const dq_plan* plan);
/* Number of kernel launches one dq_scan issues. */
int32_t dq_plan_num_launches(const dq_plan* plan);
/* Optional per-kernel timing (hipEvents recorded on the launch stream around every launch).
 * kernel: 0 = predicate pass, 1 = all column-pass launches, 2 = pair (correlation) pass,
 * 3 = finalize, 4 = the dictionary row pass (DQ_TYPE_DICT_UTF8 columns; not part of 1),
 * 16 + v = column-pass launches of variant v (see deequ_amd/csrc/dq_device.h).
 * dq_plan_kernel_time synchronises, then returns the summed duration and launch count since
 * timing was (re-)enabled. */
dq_status dq_plan_enable_timing(dq_plan* plan, int32_t on);
dq_status dq_plan_kernel_time(dq_plan* plan, int32_t kernel, double* total_ms, int64_t* launches);
/* Algorithmic bytes per row (x1000) the column-pass launch of variant v reads (excl. UTF8 data). */
int64_t dq_plan_variant_bytes_per_row_x1000(const dq_plan* plan, int32_t variant);
/* The same per timing kernel id (0 = predicate pass: its atoms' columns, 2 = pair pass: its columns,
 * 16 + v = variant v); UTF8 data bytes excluded. */
int64_t dq_plan_kernel_bytes_per_row_x1000(const dq_plan* plan, int32_t kernel);
/* 1 when the plan's predicate pass runs as a kernel compiled for its program (the Compliance / where
 * programs of numeric comparisons: whole-stage code generation as Spark does for the same expressions,
 * hipRTC for the device's gfx950 target), 0 when the interpreter runs it (or the plan has no predicates);
 * note (optional, cap bytes incl. the terminator) receives the reason the interpreter runs, or -- when
 * compiled -- where the code object came from ("hiprtc", "disk cache", "process cache"). */
int32_t dq_plan_pred_compiled(const dq_plan* plan, char* note, int32_t cap);
/* Wait up to timeout_ms (< 0: until done) for a background compile of the plan's predicate kernel (AUTO);
 * then 1 when the next dq_scan runs the compiled kernel, 0 when the interpreter runs it (compile failed, not
 * eligible, no predicates), or a negative dq_status. */
int32_t dq_plan_pred_wait(dq_plan* plan, int32_t timeout_ms);
/* Join every background compile still running.  A host program calls it before the process starts to exit: hipRTC
 * loads its compiler on first use, so at exit that compiler is torn down before this library's own join runs, and a
 * compile still in flight would run into it.  deequ_amd registers it with Python's atexit. */
void dq_pred_jit_drain(void);
/* EXPLAIN of the plan dq_plan_create_opts would build, on the host only (no device, no allocation, no
 * compile): the launches per scan, the column-pass variants, the pair pass, the predicate program and -- when
 * the predicate pass would be compiled -- the generated kernel source.  Writes at most cap bytes (incl. the
 * terminator) to out and returns the full text's size incl. the terminator (call with cap 0 to size the
 * buffer), or a negative dq_status (planning errors as dq_plan_create reports them). */
int64_t dq_plan_explain(const dq_analyzer_spec* specs, int32_t n_specs, const dq_column_desc* schema, int32_t n_cols,
                        const dq_pred_node* pred_pool, int32_t n_pred, const char* const* patterns, int32_t n_patterns,
                        const dq_plan_options* opts, char* out, int64_t cap);
/* Host wall time dq_plan_create* spent on the plan (ms), and the part of it spent obtaining the compiled
 * predicate kernel (hipRTC compile, or a code-object cache lookup); 0 for the latter without one. */
dq_status dq_plan_create_time(const dq_plan* plan, double* total_ms, double* pred_jit_ms);

/* Grouping analyzers (analyzers/GroupingAnalyzers.scala:44-82, 118-138): the frequencies
 * SELECT cols, COUNT(*) FROM data WHERE cols IS NOT NULL GROUP BY cols on the GPU (sort-based), and
 * the summary Uniqueness / Distinctness / CountDistinct / Entropy / UniqueValueRatio compute from.
 * cols: n_chunks x n_cols views, chunk-major (device pointers).  A single numeric column groups by
 * its exact value (NaN canonical, -0.0 != 0.0 as Spark 2.2); strings / several columns group by a
 * 64-bit tuple hash whose equal-hash neighbours are compared exactly (a collision between distinct
 * tuples is DQ_E_UNSUPPORTED, never a silent merge).  dq_freq_merge is FrequenciesAndNumRows.sum
 * (outer join adding counts).  Hashed tables carry a second, independently seeded hash per group, so a
 * merge of two tables whose distinct tuples share a first hash is DQ_E_UNSUPPORTED, not a silent
 * merge; more than 2^31 - 1 groups in the two tables together is DQ_E_UNSUPPORTED. */
typedef struct dq_freq_table dq_freq_table;
typedef struct dq_freq_summary {
  int64_t num_groups;  /* rows of the frequencies table (CountDistinct) */
  int64_t num_unique;  /* groups with count == 1 */
  int64_t num_values;  /* rows with every grouping column non-null */
  double entropy;      /* sum over groups of -(c / num_rows) * ln(c / num_rows) (Entropy.scala:31-37) */
} dq_freq_summary;
dq_status dq_freq_build(const int32_t* types, int32_t n_cols, const dq_column_view* cols, const int64_t* chunk_rows,
                        int32_t n_chunks, int32_t device, void* hip_stream, dq_freq_table** out);
/* dq_freq_build of rows that each stand for several: weights[k] is chunk k's device array of chunk_rows[k] int64
 * weights, row r of the chunk counts weights[k][r] times, and a row whose weight is <= 0 is not part of the data (it
 * makes no group).  Keys, group order, the exact check, the second hashes and the representative rows (ids into
 * these chunks) are dq_freq_build's, the counts and num_values are sums of weights; the table is what dq_freq_build
 * makes of the data with every row repeated weight times.  For the groupings keyed by a tuple hash (a string or
 * decimal column, several columns); a single fixed-width column is DQ_E_UNSUPPORTED.  Used with dq_dict_count: the
 * chunks are dictionaries' entries, the weights their counts. */
dq_status dq_freq_build_weighted(const int32_t* types, int32_t n_cols, const dq_column_view* cols,
                                 const int64_t* chunk_rows, const int64_t* const* weights, int32_t n_chunks,
                                 int32_t device, void* hip_stream, dq_freq_table** out);
dq_status dq_freq_merge(const dq_freq_table* a, const dq_freq_table* b, dq_freq_table** out);
dq_status dq_freq_summarize(const dq_freq_table* t, int64_t num_rows, dq_freq_summary* out);
int64_t dq_freq_num_groups(const dq_freq_table* t);
dq_status dq_freq_export(const dq_freq_table* t, uint64_t* keys, int64_t* counts, int64_t cap);
void dq_freq_destroy(dq_freq_table* t);
/* Self-contained frequency tables (the state of the grouping analyzers as Deequ's State / StatePersister /
 * StateLoader model needs it).  A hashed table built from data names every group's value only by a row id into the
 * caller's chunks.  dq_freq_materialize gathers those representative tuples into a store the table owns: per grouping
 * column exactly n_groups entries in group order and no validity (groups hold no NULL) -- a dense array for
 * fixed-width types (16 bytes per DECIMAL128, one byte per BOOL), int64 offsets[n_groups + 1] plus the bytes for
 * UTF8 / LARGE_UTF8.  cols / chunk_rows / n_chunks: the views the table was built from.  A second call and a call on
 * an unhashed table (its keys are its values) do nothing; a hashed table with groups but no representative rows (a
 * merge of tables without values) is DQ_E_STATE; chunks that do not cover the stored row ids are DQ_E_INVALID.
 * dq_freq_self_contained: 1 for an unhashed table or one with a store.
 * dq_freq_merge of two self-contained tables gives a self-contained table (each group's tuple from either input) and
 * compares groups of equal first hash value by value (distinct tuples: DQ_E_UNSUPPORTED); with either input not
 * self-contained the second hash decides and the output carries no values.
 * dq_freq_to_bytes / dq_freq_from_bytes: the table's byte image, the library's own format (returns the length, or a
 * negative dq_status; writes nothing when out is NULL or cap too small).  A table that is not self-contained is
 * DQ_E_STATE.  dq_freq_from_bytes checks the whole image on the host before it allocates or copies (wrong magic /
 * version / byte order, truncation, sizes beyond n, n_groups >= 2^31, keys not strictly ascending, a count < 1, counts
 * not adding up to n_values, bad string offsets, an unknown type code: DQ_E_STATE with a message) and rebuilds the
 * table on `device` / `hip_stream`.  The image, every integer little-endian:
 *   u8[4] "DQFT"; u32 version = 1; u32 0x01020304 (byte-order marker); i32 n_cols;
 *   i32 types[n_cols] (a DECIMAL128 code carries precision and scale), one zero i32 when n_cols is odd;
 *   i32 hashed; i32 0; i64 n_groups; i64 n_values;
 *   u64 keys[n_groups]; i64 counts[n_groups]; hashed tables: u64 keys2[n_groups];
 *   hashed tables, per column: the n_groups values zero-padded to 8 bytes, or for strings i64 n_bytes,
 *   i64 offsets[n_groups + 1], the n_bytes bytes zero-padded to 8 bytes.
 * dq_freq_take_values: the stored values of column `col` for the groups with the given keys (e.g. dq_freq_top's), in
 * that order: *values_bytes = their length; copied to `values` when values_cap holds them (call with values = NULL
 * for the size); a string column also fills offsets[n + 1].  A key that is no group: DQ_E_INVALID.
 * dq_freq_mutual_information: MutualInformation of a self-contained two-column table, marginals and sum as
 * dq_mutual_information takes them, N = num_rows; *defined = 0 for an empty table. */
dq_status dq_freq_materialize(dq_freq_table* t, const dq_column_view* cols, const int64_t* chunk_rows,
                              int32_t n_chunks);
int32_t dq_freq_self_contained(const dq_freq_table* t);
int64_t dq_freq_to_bytes(const dq_freq_table* t, uint8_t* out, int64_t cap);
dq_status dq_freq_from_bytes(const uint8_t* bytes, int64_t n, int32_t device, void* hip_stream, dq_freq_table** out);
dq_status dq_freq_take_values(const dq_freq_table* t, const uint64_t* keys, int32_t n, int32_t col, void* values,
                              int64_t values_cap, int64_t* offsets, int64_t* values_bytes);
dq_status dq_freq_mutual_information(const dq_freq_table* t, int64_t num_rows, double* value, int32_t* defined);
/* ColumnProfiler.computeHistograms (profiles/ColumnProfiler.scala:518-565): the counts of every value of n_cols
 * low-cardinality columns in one pass over the data -- what one dq_freq_build per column gives, without its sort,
 * for columns the profiler's first pass found to hold few distinct values.  types: DQ_TYPE_UTF8 / LARGE_UTF8 / BOOL
 * (anything else DQ_E_UNSUPPORTED: the profiler targets string and boolean columns, :498-511); cols: n_chunks x
 * n_cols views, chunk-major, as dq_freq_build; n_cols at most 1024.  Every row counts once per column: a NULL row
 * into n_null (the caller adds it to Histogram.NullFieldReplacement's bin), any other under its exact bytes (the
 * empty string is a value) or its boolean value.  A string column holds at most dq_cat_hist_capacity() distinct
 * non-null values: one with more has status 1 (over capacity), its counts are dropped (use dq_freq_build for it) and
 * the other columns of the call are unaffected.  Strings are keyed by dq_freq_build's 64-bit tuple hash and every
 * counted row's bytes are compared with its group's representative, within a chunk and across chunks: distinct
 * values under one key fail the whole call with DQ_E_UNSUPPORTED and dq_freq_build's message, never a silent merge.
 * dq_cat_hist_export: a column's n_values counts with, for a string column, one representative row id each (chunk
 * << 40 | row: the value's first row, in ascending order, so two runs export the same arrays) whose bytes the caller
 * renders; for a boolean column rep_rows holds the value itself, 0 (false) then 1 (true), present values only.
 * No chunks, no rows or no columns give an empty, valid handle.  Synchronises hip_stream. */
typedef struct dq_cat_hist dq_cat_hist;
int32_t dq_cat_hist_capacity(void); /* distinct non-null values per column the fused pass holds */
dq_status dq_cat_hist_build(const int32_t* types, int32_t n_cols, const dq_column_view* cols, const int64_t* chunk_rows,
                            int32_t n_chunks, int32_t device, void* hip_stream, dq_cat_hist** out);
dq_status dq_cat_hist_column(const dq_cat_hist* h, int32_t col, int32_t* status /* 0 ok, 1 over capacity */,
                             int64_t* n_null, int32_t* n_values);
dq_status dq_cat_hist_export(const dq_cat_hist* h, int32_t col, int64_t* counts, uint64_t* rep_rows /* chunk << 40 | row */,
                             int32_t cap);
void dq_cat_hist_destroy(dq_cat_hist* h);
/* ApproxQuantile / ApproxQuantiles (analyzers/ApproxQuantile.scala:49-103, ApproxQuantiles.scala:30-105;
 * replaces their DeequFunctions.stateful_approx_quantile aggregation + PercentileDigest.getPercentiles).
 * One numeric column (DQ_TYPE_F64 / I64 / I32) over n_chunks chunk views; per quantile the exact order
 * statistic of rank ceil(q * n) over the non-null values (rank 1 if q <= relative_error, n if
 * q >= 1 - relative_error, as Spark 2.2's QuantileSummaries.query), which is inside the GK error bound
 * the reference guarantees.  NaN sorts last (java.lang.Double.compare), -0.0 before 0.0.  *count = the
 * number of non-null values (0: no digest, out untouched).  Parameters outside [0, 1] are DQ_E_INVALID
 * with the reference's MetricCalculationException message in dq_last_error(). */
#define DQ_MAX_QUANTILES 8
dq_status dq_approx_quantiles(int32_t type, const dq_column_view* cols, const int64_t* chunk_rows, int32_t n_chunks,
                              const double* quantiles, int32_t n_q, double relative_error, int32_t device,
                              void* hip_stream, double* out, int64_t* count);
/* ApproxQuantileState's digest (ApproxQuantile.scala:28-35, 69-80), every sample rank in two passes over the
 * column: the order keys (Double.compare order: NaN largest, -0.0 < 0.0) counted per bucket against splitters
 * from an evenly spaced sample, then only the buckets holding a sample rank compacted and radix-sorted; the
 * values at the 1-based ranks 1, 1 + s, 1 + 2 s, ..., n with s = max(1, floor(2 relative_error n)) -- the samples of a
 * QuantileSummaries with exact ranks (g = rank gaps, delta = 0; deequ_amd/quantiles.py).  *count = n
 * (0: every value NULL, no samples); *n_samples = the number of samples; DQ_E_INVALID when it exceeds cap
 * (call again with a larger buffer; relative_error 0 samples every value). */
dq_status dq_quantile_digest(int32_t type, const dq_column_view* cols, const int64_t* chunk_rows, int32_t n_chunks,
                             double relative_error, int32_t device, void* hip_stream, double* values, int64_t* ranks,
                             int64_t cap, int64_t* n_samples, int64_t* count);
/* Cast(StringType -> LongType | DoubleType), Spark 2.2: the ColumnProfiler's castNumericStringColumns
 * (profiles/ColumnProfiler.scala:133-141, 330-339, 399-417), materialised as withColumn(... cast ...) does so that
 * every analyzer above reads the result as an ordinary I64 / F64 column.  to_type: DQ_TYPE_I64 or DQ_TYPE_F64.
 * src: a DQ_TYPE_UTF8 / DQ_TYPE_LARGE_UTF8 view of n_rows.  out_values: 8 * n_rows bytes (16-byte aligned),
 * out_validity: 8 * ceil(n_rows / 64) bytes (8-byte aligned; bits past n_rows are written 0); both device,
 * caller-allocated.  Row r of the result is NULL (value 0) iff the source row is NULL or the cast fails;
 * *null_count (host, optional) = NULL rows of the result.
 * To long (UTF8String.toLong, raw bytes, no trimming): [+-]digits[.digits], the fraction dropped, Java's overflow
 * checks (-9223372036854775808 is a value, 9223372036854775808 NULL); "", a lone sign and any other byte are NULL.
 * To double (java.lang.Double.parseDouble): blanks (<= U+0020) trimmed, [+-] then NaN | Infinity | a decimal with
 * optional exponent | a Java hex float, the last two with an optional fFdD suffix; correctly rounded (nearest
 * even), overflow to +-Infinity, underflow through subnormals to +-0; everything else NULL.  Values outside the
 * device's exact fast tier (more than 38 significant digits, large exponents, hex floats) are converted on the host
 * and patched in before the call returns: every row is exact.  Synchronises hip_stream. */
dq_status dq_cast_utf8(int32_t src_type, const dq_column_view* src, int64_t n_rows, int32_t to_type,
                       void* out_values, uint8_t* out_validity, int32_t device, void* hip_stream,
                       int64_t* null_count);
/* String lengths: length(col) of a string column materialised as an I32 column, which MinLength / MaxLength read
 * as DQ_OP_MIN / DQ_OP_MAX through dq_scan like any other column (additions under ABI 6).
 * The length of a value is the number of its bytes b with (b & 0xC0) != 0x80.  On well-formed UTF-8 that is its
 * number of code points, what Spark 2.2's UTF8String.numChars returns; on ill-formed bytes it is simply this rule
 * (Spark walks lead bytes and skips by the length each announces, so the two can differ there: a lone continuation
 * byte counts 1 for Spark and 0 here, a truncated sequence may swallow the bytes behind it for Spark).
 * dq_utf8_length: src: a DQ_TYPE_UTF8 (int32 offsets) / DQ_TYPE_LARGE_UTF8 (int64 offsets) view of n_rows, values
 * 16-byte aligned and readable up to the 4-byte boundary behind the last value; src->validity NULL: no NULL row.
 * lengths: int32[n_rows]; validity_out: ceil(n_rows / 64) 64-bit words (8-byte aligned; bits past n_rows are written
 * 0); both device, caller-allocated, and every length and every word of the n_rows rows is written.  A NULL source
 * row gives a NULL row of length 0 whatever bytes its slot holds.  A LARGE_UTF8 value of 2^31 code points or more
 * is stored as INT32_MAX (a UTF8 column cannot hold one).  *nulls_out (host, optional) = the NULL rows; with it the
 * call synchronises hip_stream, without it the call is asynchronous on hip_stream.  n_rows = 0: DQ_OK, nothing
 * written.  Another source type is DQ_E_UNSUPPORTED; a NULL or misaligned buffer, n_rows < 0, reserved != 0 are
 * DQ_E_INVALID.
 * dq_utf8_length_host: the same rule on the CPU, no device (tests): data, int64 offsets[n + 1], validity an LSB-first
 * bitmap or NULL; out[r] = the length, 0 for a NULL row.
 * dq_dict_take_i32: the per-row gather of a dictionary column: indices->values int32 indices, indices->validity
 * their bitmap or NULL (the view's other fields are not read); out[r] = entry_values[index[r]] (device,
 * int32[n_entries]) and row r is valid iff its index row is valid -- and, so that the call is total, its index lies
 * inside [0, n_entries) and the entry's value is not negative (a negative value marks a NULL entry); any other row is
 * NULL with value 0.  The index of a NULL row is neither loaded nor used to address memory.  out: int32[n_rows],
 * validity_out: ceil(n_rows / 64) 64-bit words (8-byte aligned), every one written.  Asynchronous on hip_stream. */
dq_status dq_utf8_length(int32_t src_type, const dq_column_view* src, int64_t n_rows, int32_t* lengths,
                         uint64_t* validity_out, int32_t device, void* hip_stream, int64_t* nulls_out);
dq_status dq_utf8_length_host(const uint8_t* data, const int64_t* offsets, int64_t n, const uint8_t* validity,
                              int32_t* out);
dq_status dq_dict_take_i32(const dq_column_view* indices, int64_t n_rows, const int32_t* entry_values,
                           int64_t n_entries, int32_t* out, uint64_t* validity_out, int32_t device, void* hip_stream);
/* RowLevelSchemaValidator (schema/RowLevelSchemaValidator.scala:25-282): a declared schema over string columns,
 * the per-row verdict m = toCNF(schema) (:225-281, a three-valued SQL boolean), the conforming rows cast to the
 * declared types and the other rows untouched.  One dq_schema_column per ColumnDefinition, in the schema's order:
 *   DQ_SCHEMA_STRING     has_min / has_max: minLength / maxLength against length(c) (UTF-8 characters);
 *                        text: `matches` (NULL = none), tested as regexp_extract(c, p, 0) != "" (DQ_REGEX_EXTRACT_NONEMPTY)
 *   DQ_SCHEMA_INT        has_min / has_max: minValue / maxValue against Cast(c, IntegerType) = UTF8String.toInt
 *   DQ_SCHEMA_DECIMAL    precision, scale (0 <= scale <= precision <= 38): Cast(c, DecimalType(p, s)) IS NOT NULL
 *   DQ_SCHEMA_TIMESTAMP  text: the SimpleDateFormat mask; unix_timestamp(c, mask) IS NOT NULL, session time zone UTC.
 *                        Masks: fields y (3 letters or more), M (at most 2), d, H, m, s, each followed by a literal
 *                        (a non-letter, non-digit ASCII character or 'quoted text') or the end of the mask
 * nullable = 0 adds the clause c IS NOT NULL.  A row is TRUE, FALSE or -- only when no clause is FALSE and an INT
 * column with has_min is NULL in it (:246 is `FALSE OR v >= min`) -- UNKNOWN; an UNKNOWN row belongs to neither
 * output, as in the reference.  dq_schema_plan_create needs no device; DQ_E_UNSUPPORTED (reason in dq_last_error) for
 * a regex outside the DFA subset or a mask outside the subset above.
 * dq_schema_validate: one chunk.  types / cols: the chunk's n_cols columns (device views; a definition reads column
 * `column`, which must be UTF8 / LARGE_UTF8).  valid_bitmap / invalid_bitmap: ceil(n_rows / 64) 64-bit words each
 * (device, 8-byte aligned): bit r of the first is set iff m is TRUE for row r, of the second iff m is FALSE; bits
 * past n_rows are written 0.  cast_values[d] / cast_validity[d] (device; NULL entries or NULL arrays: not
 * materialised; ignored for STRING) receive definition d's cast of every row: int32, 16-byte unscaled decimal or
 * int64 microseconds per row (16-byte aligned) and ceil(n_rows / 64) validity words.  A row's cast is its value for
 * every TRUE row; a row past its first FALSE clause may hold 0 / NULL instead.  *num_valid / *num_invalid (host):
 * the TRUE and FALSE rows.  Synchronises hip_stream.
 * dq_schema_check_host: the same rules over host bytes, no device (tests): per column c data[c], int64 offsets[c]
 * (n_rows + 1) and valid[c] (one byte per row; NULL array or entry: no NULL rows); verdict[r] = 1 TRUE, 0 FALSE,
 * 2 UNKNOWN; cast_values[d] as above, cast_ok[d] one byte per row (NULL entries: skipped); every definition's cast
 * is evaluated for every row. */
enum dq_schema_kind { DQ_SCHEMA_STRING = 1, DQ_SCHEMA_INT = 2, DQ_SCHEMA_DECIMAL = 3, DQ_SCHEMA_TIMESTAMP = 4 };
typedef struct dq_schema_column {
  int32_t kind;       /* enum dq_schema_kind */
  int32_t column;     /* index into the views of a chunk */
  int32_t nullable;   /* isNullable */
  int32_t has_min, has_max;
  int32_t min_value, max_value;
  int32_t precision, scale;
  int32_t reserved;   /* 0 */
  const char* text;   /* UTF-8: STRING `matches` or NULL; TIMESTAMP mask */
} dq_schema_column;
typedef struct dq_schema_plan dq_schema_plan;
dq_status dq_schema_plan_create(const dq_schema_column* defs, int32_t n_defs, dq_schema_plan** out);
void dq_schema_plan_destroy(dq_schema_plan* plan);
dq_status dq_schema_validate(dq_schema_plan* plan, const int32_t* types, const dq_column_view* cols, int32_t n_cols,
                             int64_t n_rows, uint64_t* valid_bitmap, uint64_t* invalid_bitmap, void* const* cast_values,
                             uint8_t* const* cast_validity, int32_t device, void* hip_stream, int64_t* num_valid,
                             int64_t* num_invalid);
dq_status dq_schema_check_host(const dq_schema_plan* plan, const uint8_t* const* data, const int64_t* const* offsets,
                               const uint8_t* const* valid, int32_t n_cols, int64_t n_rows, uint8_t* verdict,
                               void* const* cast_values, uint8_t* const* cast_ok);
/* Stable row compaction ("take"): the rows a bitmap selects, in source order.  dq_take_index: index[k] (device,
 * n_selected entries) = the k-th selected row of selection (device, ceil(n_rows / 64) 64-bit words); n_selected must
 * be the bitmap's popcount over the n_rows (DQ_E_INVALID otherwise, nothing written).  dq_take_rows: one column of
 * any dq_type through such an index.  out_values: fixed-width types n_selected values (BOOL: ceil(n_selected / 64)
 * 64-bit words), strings the bytes; values_capacity = its size in bytes.  out_validity (NULL: not wanted):
 * ceil(n_selected / 64) 64-bit words, all set when src has no validity.  Strings: out_offsets receives n_selected + 1
 * offsets of src's width and *data_bytes the bytes selected; with out_values NULL the call stops there (the sizing
 * call).  All output buffers are device memory, values 16-byte and bitmaps / offsets 8-byte aligned; bytes past the
 * result (the padding a column carries) are the caller's to clear.  Both synchronise hip_stream. */
dq_status dq_take_index(const uint64_t* selection, int64_t n_rows, int64_t n_selected, int64_t* index, int32_t device,
                        void* hip_stream);
dq_status dq_take_rows(int32_t type, const dq_column_view* src, int64_t n_rows, const int64_t* index, int64_t n_selected,
                       void* out_values, int64_t values_capacity, uint8_t* out_validity, void* out_offsets,
                       int64_t* data_bytes, int32_t device, void* hip_stream);
/* Row-level results (Deequ's VerificationResult.rowLevelResultsAsDataFrame): which rows pass, as bitmaps in the layout
 * dq_take_index reads (64-bit words, LSB first, bit r = row r of the chunk, bits past n_rows written 0).
 * A row program is a predicate program that keeps its rows: dq_row_program_create takes the column descriptors, the
 * predicate pool and the regex patterns as dq_plan_create_ex does, plus n_out outputs (pred_root, where_root or -1).
 * It lowers on the host and needs no device.  At most dq_row_max_outputs() outputs and as many distinct roots
 * (predicates and `where` filters together), 64 columns and the fused pass's program length and DFA budget; a
 * longer list is DQ_E_UNSUPPORTED: split it into several programs.  A root outside the GPU grammar is
 * DQ_E_UNSUPPORTED as in dq_plan_create; a predicate over a DQ_TYPE_DICT_UTF8 column too (decode it).
 * dq_row_outcomes evaluates one chunk of n_rows (< 2^31) on `device`, enqueued on hip_stream: cols are the chunk's
 * views as dq_scan takes them (only the columns the program reads are looked at).  Output k writes
 *   pass[k]      ceil(n_rows / 64) words: bit r = 1 iff pred is TRUE on row r and (no where, or where is TRUE on r);
 *   applies[k]   (the array or an entry may be NULL: not wanted) bit r = 1 iff no where, or where is TRUE on row r;
 *   num_pass[k] / num_applies[k] (host, either array may be NULL): the set bits of the two.
 * A NULL predicate result is not a pass (Compliance's CASE WHEN p THEN 1 ELSE 0); a row whose where is NULL or FALSE
 * neither passes nor applies.  No byte past ceil(n_rows / 64) * 8 of a bitmap is touched; pass / applies buffers
 * are device memory, 8-byte aligned.  n_rows = 0: DQ_OK, nothing written (the counts are 0).  Invalid arguments are
 * rejected before any launch.  Synchronises hip_stream.  Interpreted evaluator only (no compiled kernel).
 * dq_row_program_info: the outputs, the distinct roots after deduplication and the program's instructions. */
typedef struct dq_row_output {
  int32_t pred_root;  /* root index into the predicate node pool */
  int32_t where_root; /* optional `where` filter root, -1 = none */
} dq_row_output;
typedef struct dq_row_program dq_row_program;
int32_t dq_row_max_outputs(void);
dq_status dq_row_program_create(const dq_column_desc* schema, int32_t n_cols, const dq_pred_node* pred_pool,
                                int32_t n_pred, const char* const* patterns, int32_t n_patterns,
                                const dq_row_output* outputs, int32_t n_out, dq_row_program** out);
dq_status dq_row_program_info(const dq_row_program* prog, int32_t* n_outputs, int32_t* n_roots, int32_t* n_instr);
void dq_row_program_destroy(dq_row_program* prog);
dq_status dq_row_outcomes(dq_row_program* prog, const dq_column_view* cols, int64_t n_rows, uint64_t* const* pass,
                          uint64_t* const* applies, int32_t device, void* hip_stream, int64_t* num_pass,
                          int64_t* num_applies);
/* The unique rows of one chunk from a frequency table built (dq_freq_build / _build_weighted / _merge) from data that
 * holds the chunk, over the table's grouping columns C.  cols: the chunk's views of C in the table's order; types:
 * their type codes, or NULL for the table's own (a string column may have the other offset width: the key hashes
 * bytes and length, so a dictionary column's table built from its entries is probed with the decoded column).
 * unique: bit r = 1 iff every column of C is non-null in row r and the row's group has count 1; grouped (NULL: not
 * wanted): bit r = 1 iff every column of C is non-null in row r (the row took part in the grouping).  Both in the
 * bitmap layout above; *num_unique / *num_grouped (host, optional) their set bits.  A value that occurs once in
 * this chunk and once in another chunk of the table's data is not unique.  Keys are computed as the build computed
 * them and looked up in the table's sorted keys; the build verified that equal keys are equal tuples.  A row whose
 * key the table lacks means the table was not built from this data: DQ_E_INVALID (the bitmaps' contents are then
 * unspecified).  Runs on the table's device, enqueued on hip_stream, and synchronises it. */
dq_status dq_freq_unique_rows(const dq_freq_table* t, const int32_t* types, const dq_column_view* cols, int64_t n_rows,
                              uint64_t* unique, uint64_t* grouped, void* hip_stream, int64_t* num_unique,
                              int64_t* num_grouped);
/* Referential integrity: the rows of one chunk whose tuple over the key columns C is a group of the frequency table
 * t, a key set built from OTHER data (dq_freq_build of the reference table's columns, then dq_freq_materialize) --
 * SQL's `C IN (SELECT keys)` / a left semi-join, per row.  A key the table lacks is the answer here, never an error.
 * cols: the chunk's views of C in the table's column order (the table's arity is the number of views read); types:
 * their type codes, or NULL for the table's own.  A string column may have the other offset width, as in
 * dq_freq_unique_rows; any other difference -- a decimal of another precision or scale included -- is DQ_E_INVALID
 * naming the column and both type codes.  Nothing is widened implicitly: an i32 column is never matched against i64
 * keys; cast it first.
 * filter (NULL: every row): a bitmap in the layout above, the rows to look at (a `where`).
 * contained: bit r = 1 iff filter is NULL or has bit r set, AND every column of C is non-null in row r, AND the
 * row's tuple is a group of t.  A NULL in any key column is "not contained" (SQL IN / semi-join: NULL matches
 * nothing) and the row still counts in the denominator.  applies (NULL: not wanted): bit r = 1 iff filter is NULL or
 * has bit r set.  Bitmap layout, zero tail bits, 8-byte alignment (filter too), n_rows = 0 (DQ_OK, nothing written),
 * the n_rows < 2^31 limit and the synchronisation of hip_stream are dq_freq_unique_rows's; *num_contained /
 * *num_applies (host, optional) are the set bits.  The table's counts are ignored: only membership matters.
 * An unhashed table (one fixed-width column): membership is equality of the grouping's value bits -- NaN canonical,
 * -0.0 and 0.0 distinct.  A hashed table (strings, decimals, several columns) must be self-contained
 * (dq_freq_self_contained), else DQ_E_STATE: nothing has verified that a found hash is the row's tuple, so the row is
 * contained only if its tuple equals the group's stored tuple column by column (string bytes and length, a decimal's
 * 16 bytes, value bits otherwise); a found hash with a different tuple is "not contained", never the collision
 * error.  Arguments are checked before anything is launched: n_rows, the bitmaps' alignment, NULL contained / cols /
 * table, the table's state, the types, the views' buffers. */
dq_status dq_freq_contains_rows(const dq_freq_table* t, const int32_t* types, const dq_column_view* cols,
                                int64_t n_rows, const uint64_t* filter, uint64_t* contained, uint64_t* applies,
                                void* hip_stream, int64_t* num_contained, int64_t* num_applies);
/* Dataset match: does a row equal the reference table's row with the same key?  Two calls per chunk.
 * dq_freq_lookup_rows is dq_freq_contains_rows that says WHICH group a row hit: group (device, n_rows int32, 4-byte
 * aligned) receives for row r the index of its group in t's sorted keys (0 .. G-1; the keys ascend as unsigned 64-bit
 * words -- an unhashed integer column's negative values after the others, a hashed table in hash order -- so the
 * index is an identifier of the group, dq_freq_export's position, not a rank of the value) when the filter keeps the row,
 * every key column is non-null and the tuple is a group of t, else -1.  The membership rule, the type rule, the
 * DQ_E_STATE of a hashed table that is not self-contained and the by-value comparison of a found hash (a different
 * tuple: -1, never the collision error) are dq_freq_contains_rows's: it is the same search.  *num_found (host,
 * optional): the entries >= 0.  A table of more than 2^31 - 1 groups is DQ_E_UNSUPPORTED.  Arguments are checked
 * before anything is launched, in dq_freq_contains_rows's order; n_rows = 0: DQ_OK, nothing written.
 * dq_rows_match compares n_cols (1 .. 16) columns of the chunk with the reference's payload: payload row g
 * (0 <= g < n_payload_rows) holds the compare columns of the reference row whose key is group g.  types / cols: the
 * chunk's n_cols columns of n_rows rows; payload_types / payload: the payload's.  Column c of both must have the same
 * type code (a decimal's precision and scale included) or both be string columns (UTF8 / LARGE_UTF8, in any pairing);
 * any other difference -- DQ_TYPE_DICT_UTF8 included: decode it -- is DQ_E_INVALID naming the column and both codes.
 * Outputs in the bitmap layout above (zero tail bits, 8-byte aligned, no byte past ceil(n_rows / 64) * 8 touched):
 *   matched  bit r = 1 iff the filter (NULL: every row) keeps r, group[r] is a payload row, and every column is equal;
 *   found    (NULL: not wanted) bit r = 1 iff the filter keeps r and group[r] is a payload row;
 *   applies  (NULL: not wanted) bit r = 1 iff the filter keeps r.
 * A group[r] < 0 or >= n_payload_rows is "not found" and addresses nothing.  Equality per column is null-safe:
 * NULL equals NULL, NULL differs from every value, and the bytes under a NULL slot are never read.  Values compare as
 * grouping keys do: fixed-width types by their value bits (every NaN the same, -0.0 and 0.0 distinct), BOOL by its
 * bit, DECIMAL128 by its 16 bytes, strings by length and bytes.  *num_matched / *num_found / *num_applies (host,
 * optional): the set bits; num_mismatch (host, n_cols entries, or NULL): entry c = the found rows whose column c
 * differs -- with it every column of a found row is judged, without it a row stops at its first difference.
 * n_rows < 2^31; n_rows = 0: DQ_OK, no bitmap written, the counts 0.  Arguments are checked before anything is
 * launched.  Runs on `device`, enqueued on hip_stream, and synchronises it. */
dq_status dq_freq_lookup_rows(const dq_freq_table* t, const int32_t* types, const dq_column_view* cols, int64_t n_rows,
                              const uint64_t* filter, int32_t* group, void* hip_stream, int64_t* num_found);
dq_status dq_rows_match(const int32_t* types, const dq_column_view* cols, const int32_t* payload_types,
                        const dq_column_view* payload, int32_t n_cols, int64_t n_rows, int64_t n_payload_rows,
                        const int32_t* group, const uint64_t* filter, uint64_t* matched, uint64_t* found,
                        uint64_t* applies, int32_t device, void* hip_stream, int64_t* num_matched, int64_t* num_found,
                        int64_t* num_applies, int64_t* num_mismatch);
/* Distribution drift: how far is the distribution of one frequency table from another's?  (Additions under ABI 6.)
 * a is the data's table, b the reference's; both stay on the device and neither is changed.  N_a / N_b are the tables'
 * n_values (the sums of their counts: NULL rows are part of neither distribution).  For a group g,
 * p = (double)count_a(g) / (double)N_a and q likewise for b; a group a table lacks has probability 0 there.
 * A group of a and a group of b are the same group when their key words are equal and, for hashed tables (strings,
 * decimals, several columns), their stored tuples are equal by value -- string length and bytes, a decimal's 16 bytes,
 * value bits otherwise: dq_freq_contains_rows' comparison.  Equal hashes with different tuples are two groups, one
 * only in a and one only in b: never the collision error, never a match.  An unhashed table's key is its value's
 * bits: every NaN one group, -0.0 and 0.0 two.
 * dq_freq_distance, over the union of the groups:
 *   linf = max |p - q|;  tv = 1/2 sum |p - q|;
 *   js = 1/2 sum [p ln(p / m) + q ln(q / m)], m = (p + q) / 2, natural logarithm, a zero p (or q) contributing 0:
 *        a value in [0, ln 2];
 *   n_common / n_only_a / n_only_b: the groups in both tables, in a alone, in b alone; count_only_a / count_only_b:
 *        the rows (counts) of a in groups b lacks, and of b in groups a lacks;
 *   linf_key / linf_side: the key word of the group attaining linf and the table that holds its value (0 = a, also for
 *        a group of both; 1 = b alone).  Ties go to the smaller unsigned key word, then to side a.
 * Both tables must be self-contained (dq_freq_self_contained), else DQ_E_STATE.  They need the same number of columns
 * and per column the same type code (a decimal's precision and scale are part of it; the string offset width is
 * free); any other difference is DQ_E_INVALID naming the column and both codes; tables on different devices are
 * DQ_E_INVALID.  All of that is checked before anything is launched.  Either table with n_values = 0: DQ_OK,
 * defined = 0, every other member 0, nothing launched.
 * Arithmetic is binary64 without contraction and with correctly rounded division: linf is bit for bit
 * max |c_a / N_a - c_b / N_b| evaluated per group in IEEE doubles.  No floating-point atomics: a thread, a wave, a
 * workgroup and one final pass sum in a fixed order that depends on the group counts alone, so two calls on the same
 * tables return identical bits.  tv and js carry the roundings of their G terms (G = the union's size): within
 * 16 (G + 1) 2^-53 of the exact sums.
 * dq_freq_ks: the exact two-sample Kolmogorov-Smirnov statistic of two unhashed single-column tables of one type among
 * F64 / F32 / I64 / I32 / I16 / I8 / DATE32 / TIMESTAMP; BOOL and every hashed table are DQ_E_UNSUPPORTED, different
 * types DQ_E_INVALID.  Values order numerically; floats with -0.0 immediately below 0.0 (two groups, as the grouping
 * has them), -inf and +inf in their numeric places and the canonical NaN greatest.  F_a(x) = (the counts of a's groups
 * <= x, an exact integer) / N_a, one division; *ks = max over every group value x of either table of
 * |F_a(x) - F_b(x)|, bit for bit that expression in IEEE doubles.  *defined = 0 (and *ks = 0) when either table has
 * n_values = 0.  A table of more than 2^31 - 2 groups is DQ_E_UNSUPPORTED.
 * Both run on the tables' device, enqueued on hip_stream, take their scratch from the grouping arena and synchronise
 * the stream; nothing but the result goes to the host. */
typedef struct dq_freq_distance_result {
  int32_t defined;    /* 0: a table without values; everything below is 0 */
  int32_t linf_side;  /* 0 = the linf group is a group of a, 1 = of b alone */
  double linf, tv, js;
  uint64_t linf_key;
  int64_t n_common, n_only_a, n_only_b, count_only_a, count_only_b;
} dq_freq_distance_result;
dq_status dq_freq_distance(const dq_freq_table* a, const dq_freq_table* b, void* hip_stream,
                           dq_freq_distance_result* out);
dq_status dq_freq_ks(const dq_freq_table* a, const dq_freq_table* b, void* hip_stream, double* ks, int32_t* defined);
/* Segmented metrics: the scan analyzers' states per group of a key column.  (Additions under ABI 6.)
 * seg (device, n_rows int32) is dq_freq_lookup_rows' output against the key set of the segment columns: the row's
 * segment 0 .. G - 1, or -1 for a row with a NULL key, which belongs to the trailing NULL segment G.
 * dq_segment_order: perm (device, n_rows int32) receives the row numbers sorted stably by segment -- the rows of a
 * segment ascend -- and offsets (device, G + 2 int64) the segments' first positions in perm; offsets[G + 1] = n_rows.
 * n_rows < 2^31; n_rows = 0: DQ_OK, offsets all 0.  G + 1 beyond int32 is DQ_E_UNSUPPORTED.  Once per chunk, shared
 * by every slot.
 * dq_segment_scan: slots (host, 1 .. DQ_SEGMENT_MAX_SLOTS) over the G1 = G + 1 segments of perm / offsets; out
 * (device, n_slots x G1 dq_segment_state, slot-major) receives per (slot, segment):
 *   applies    the segment's rows the filter keeps (filter NULL: its rows);
 *   count      of those, the rows whose validity bit is set (col.validity NULL: all of them);
 * and for DQ_SEG_STATS (type F64 / F32 / I64 / I32 / I16 / I8 / DATE32 / TIMESTAMP; col.values not NULL) over those
 * count rows what the column scan keeps for a column: n / mean / m2 (NaN values included, +-inf values counted in
 * pinf_count / ninf_count instead), sum (floating types; without the +-inf values) or isum (integral types: the
 * wrapping int64 sum), fmin / fmax over the values that are not NaN (v_min_f64 / v_max_f64: -0.0 below 0.0), nan_count.
 * A segment without rows gets the empty state (n = 0, count = 0, fmin = +inf, fmax = -inf).  DQ_SEG_COUNT reads no
 * value and ignores type.  The reduction is a function of offsets alone -- tiles of dq_segment_tile() rows from a
 * segment's first row, each reduced in one order, merged in ascending tile order -- so equal inputs give equal bits;
 * no floating-point atomics.  An unknown op or type, a NULL argument, n_slots or G1 out of range: DQ_E_INVALID before
 * any launch; a valid type without segmented statistics (strings, BOOL, DECIMAL128): DQ_E_UNSUPPORTED.  Both calls
 * run on the current device, enqueue on hip_stream and synchronise it. */
#define DQ_SEGMENT_MAX_SLOTS 64
#define DQ_SEGMENT_TILE 256
enum dq_segment_op { DQ_SEG_COUNT = 1, DQ_SEG_STATS = 2 };
typedef struct dq_segment_slot {
  dq_column_view col;
  int32_t type;            /* enum dq_type (DQ_SEG_STATS) */
  int32_t op;              /* enum dq_segment_op */
  const uint64_t* filter;  /* device bitmap of the chunk's rows (bit r = row r), or NULL: every row */
} dq_segment_slot;
typedef struct dq_segment_state {
  double n, mean, m2, sum;
  int64_t isum, count, nan_count;
  double fmin, fmax;
  int64_t pinf_count, ninf_count, applies;
} dq_segment_state;
int32_t dq_segment_tile(void);
dq_status dq_segment_order(const int32_t* seg, int64_t n_rows, int64_t G, int32_t* perm, int64_t* offsets,
                           void* hip_stream);
dq_status dq_segment_scan(const dq_segment_slot* slots, int32_t n_slots, const int32_t* perm, const int64_t* offsets,
                          int64_t G1, dq_segment_state* out, void* hip_stream);
/* Row-level random split (the train / test split of suggestions/ConstraintSuggestionRunner.scala:127-148).  Row r of
 * the chunk has the global index g = row0 + r; h = XXH64 of g's 8 little-endian bytes under `seed`,
 * u = (h >> 11) * 2^-53, and the row is a test row iff u < test_ratio, else a training row: a pure function of
 * (seed, g), so a table splits the same way however it is chunked.  (Spark's randomSplit depends on the
 * partitioning and is not reproduced.)  train_bitmap / test_bitmap: ceil(n_rows / 64) 64-bit words each (device,
 * 8-byte aligned), LSB first, bits past n_rows written 0 -- the layout dq_take_index reads.  *num_train + *num_test
 * (host) = n_rows.  n_rows = 0: DQ_OK, nothing written; test_ratio outside ]0, 1[ or NaN, row0 < 0: DQ_E_INVALID.
 * Synchronises hip_stream.  dq_split_rows_host: the same draw on the CPU, no device (tests): is_test[r] = 1 / 0. */
dq_status dq_split_rows(int64_t n_rows, int64_t row0, uint64_t seed, double test_ratio, uint64_t* train_bitmap,
                        uint64_t* test_bitmap, int32_t device, void* hip_stream, int64_t* num_train,
                        int64_t* num_test);
dq_status dq_split_rows_host(int64_t n_rows, int64_t row0, uint64_t seed, double test_ratio, uint8_t* is_test);
/* Histogram (analyzers/Histogram.scala:33-99): the n largest groups by count (ties in key order):
 * key, count and -- for a table built from data with hashed keys (strings) -- one representative row
 * id (chunk << 40 | row) whose value the caller renders; ~0 when not available (merged tables). */
dq_status dq_freq_top(const dq_freq_table* t, int32_t n, uint64_t* keys, int64_t* counts, uint64_t* rep_rows,
                      int32_t* n_out);
/* MutualInformation(a, b) (analyzers/MutualInformation.scala:32-72): joint frequencies of the two
 * columns, their marginals summed from the joint counts, and
 * sum (pxy / N) * ln((pxy / N) / ((px / N) * (py / N))) with N = num_rows.  cols: n_chunks x 2 views.
 * *defined = 0 when no row has both values (the SQL sum is NULL -> EmptyStateException). */
dq_status dq_mutual_information(const int32_t* types, const dq_column_view* cols, const int64_t* chunk_rows,
                                int32_t n_chunks, int64_t num_rows, int32_t device, void* hip_stream, double* value,
                                int32_t* defined);

/* ---- Row selections (`where`) for the grouping, histogram and quantile entry points (additions under ABI 6) ----
 * X_where(..., selection, ...) is X over the data that holds exactly the selected rows, in their order: an unselected
 * row is no part of the data -- it makes no group, is in no slot, has no rank, and does not count as a NULL either.
 * A selection is a device bitmap of ceil(n_rows / 64) uint64_t words, LSB first, 8-byte aligned: the layout
 * dq_take_index reads and dq_row_outcomes writes.  Bits past n_rows are ignored.  A NULL selection means every row
 * (the unfiltered kernel runs); a misaligned one is DQ_E_INVALID before any launch.  Where the entry point takes
 * chunks, `selection` is an array of n_chunks such pointers (host array, each entry NULL or a device bitmap), or NULL
 * for no selection at all.  No entry point copies the selected values out: the selection joins the validity in the
 * row test of the first pass, and everything after it sees selected rows only.
 * dq_freq_build_where: dq_freq_build; the representative row ids are ids into the caller's unfiltered chunks, so
 * dq_freq_materialize / _top / _take_values / _unique_rows_where take the same chunks.  The caller passes the number
 * of selected rows, not the chunks', to dq_freq_summarize.
 * dq_freq_unique_rows_where: unique / grouped bits of unselected rows are 0; the table is one built with the same
 * selection (or from data that holds the selected rows).
 * dq_dict_count_where / dq_bin_count_where: selection is the one chunk's bitmap.  *n_selected of dq_bin_count_where
 * (device int64, 8-byte aligned, NULL: not wanted) ACCUMULATES the number of selected rows, NULL rows included, as
 * counts accumulates; with a NULL selection it adds n_rows.
 * dq_approx_quantiles_where / dq_quantile_digest_where: ranks and *count run over the selected non-null values.
 * dq_mutual_information_where: num_rows is the number of selected rows. */
dq_status dq_freq_build_where(const int32_t* types, int32_t n_cols, const dq_column_view* cols, const int64_t* chunk_rows,
                              const uint64_t* const* selection, int32_t n_chunks, int32_t device, void* hip_stream,
                              dq_freq_table** out);
dq_status dq_freq_unique_rows_where(const dq_freq_table* t, const int32_t* types, const dq_column_view* cols,
                                    int64_t n_rows, const uint64_t* selection, uint64_t* unique, uint64_t* grouped,
                                    void* hip_stream, int64_t* num_unique, int64_t* num_grouped);
dq_status dq_dict_count_where(const dq_column_view* indices, int64_t n_rows, const uint64_t* selection, int64_t* counts,
                              int32_t device, void* hip_stream);
dq_status dq_bin_count_where(const dq_bins* bins, int32_t type, const dq_column_view* col, int64_t n_rows,
                             const uint64_t* selection, int64_t* counts, int64_t* n_selected, int32_t device,
                             void* hip_stream);
dq_status dq_approx_quantiles_where(int32_t type, const dq_column_view* cols, const int64_t* chunk_rows,
                                    const uint64_t* const* selection, int32_t n_chunks, const double* quantiles,
                                    int32_t n_q, double relative_error, int32_t device, void* hip_stream, double* out,
                                    int64_t* count);
dq_status dq_quantile_digest_where(int32_t type, const dq_column_view* cols, const int64_t* chunk_rows,
                                   const uint64_t* const* selection, int32_t n_chunks, double relative_error,
                                   int32_t device, void* hip_stream, double* values, int64_t* ranks, int64_t cap,
                                   int64_t* n_samples, int64_t* count);
dq_status dq_mutual_information_where(const int32_t* types, const dq_column_view* cols, const int64_t* chunk_rows,
                                      const uint64_t* const* selection, int32_t n_chunks, int64_t num_rows,
                                      int32_t device, void* hip_stream, double* value, int32_t* defined);

/* State algebra.
 * dq_state_merge:   Analyzers.merge / State.sum on Option[State] (Analyzer.scala:343-362):
 *                   None + x = x; Min/Max merge with java.lang.Math.min/max.
 * dq_state_combine: Spark partial-aggregate merge of two aggregation-result slot sets (row
 *                   shards of one scan: GPUs, chunks): SQL null-skipping per slot, NaN-as-largest
 *                   min/max ordering.  Used for the multi-GPU allgather merge. */
dq_status dq_state_merge(const dq_state* a, const dq_state* b, dq_state* out);
dq_status dq_state_combine(const dq_state* a, const dq_state* b, dq_state* out);
/* Element-wise over n slot sets (a whole run's analyzers in one call: the fixed rank-order merge of the
 * multi-GPU all-gather, the incremental StateLoader append).  out may alias a or b. */
dq_status dq_state_merge_n(const dq_state* a, const dq_state* b, int32_t n, dq_state* out);
dq_status dq_state_combine_n(const dq_state* a, const dq_state* b, int32_t n, dq_state* out);
/* 1 if fromAggregationResult would produce Some(state). */
int32_t dq_state_is_defined(const dq_state* s);
/* metricValue() of a defined state (DoubleMetric analyzers; DATATYPE has a histogram, not a double:
   DQ_E_STATE). */
dq_status dq_state_metric(const dq_state* s, double* out);
/* HLL++ estimate of 52 packed words, bit-exact with DeequHyperLogLogPlusPlusUtils.count. */
dq_status dq_hll_estimate(const int64_t* words52, double* out);

/* HdfsStateProvider byte images (Java DataOutputStream, big-endian).  Returns the image length,
 * or a negative dq_status; writes nothing when buf is NULL / cap too small (returns length). */
int64_t dq_state_to_bytes(const dq_state* s, uint8_t* buf, int64_t cap);
dq_status dq_state_from_bytes(int32_t op, const uint8_t* buf, int64_t len, dq_state* out);
/* HdfsStateProvider.toIdentifier: MurmurHash3.stringHash(analyzer.toString, 42) of UTF-8 text. */
int32_t dq_state_identifier(const char* analyzer_to_string_utf8);

#ifdef __cplusplus
}
#endif

#endif /* DQSCAN_H */
