/*
 * cobrix_hip.h -- C ABI of the MI355X (gfx950) Cobrix record decoder (libcobrix_hip.so).
 *
 * Drop-in boundary: replaces, per BATCH of records, the per-record
 *   RecordExtractors.extractRecord(ast, data, offsetBytes, ...)            (CP/reader/extractors/record/RecordExtractors.scala:49-183)
 *   + Primitive.decodeTypeValue / DecoderSelector decoder closures        (CP/parser/ast/Primitive.scala:102-128,
 *                                                                            CP/parser/decoders/DecoderSelector.scala:54-290)
 * that sit under
 *   FixedLenReader.getRowIterator(binaryData)                              (SC/reader/FixedLenReader.scala:23-25)
 *   VarLenReader.getRowIterator(stream, startingFileOffset, fileNumber, startingRecordIndex)
 *                                                                          (SC/reader/VarLenReader.scala:44-60)
 * and, for RDW files, the sequential header walk of
 *   VRLRecordReader.fetchRecordUsingRdwHeaders / RecordHeaderParserRDW     (CP/reader/iterator/VRLRecordReader.scala:151-186,
 *                                                                            CP/parser/headerparsers/RecordHeaderParserRDW.scala:44-85)
 *   IndexGenerator.sparseIndexGenerator                                   (CP/reader/index/IndexGenerator.scala:33-127)
 * (CP = cobol-parser/src/main/scala/za/co/absa/cobrix/cobol/, SC = spark-cobol/src/main/scala/za/co/absa/cobrix/spark/cobol/)
 *
 * The JVM side flattens the parsed `Copybook` AST into the cbx_field / cbx_array tables below
 * (what the Scala/Python host does in cobrix_amd/plan.py) and calls this library through
 * JNI or Panama FFM with device (or pinned host) pointers.  Plain C types only.
 *
 * Error convention (mirrors the reference): data errors never fail a call -- a malformed value
 * decodes to null (validity bit 0), as DecoderSelector.scala:283-290 does.  Structural errors
 * return a negative status: CBX_E_ARGUMENT ~ IllegalArgumentException, CBX_E_STATE ~
 * IllegalStateException (bad RDW), with the detail in cbx_last_error().
 */
#ifndef COBRIX_HIP_H
#define COBRIX_HIP_H
#ifndef __HIPCC_RTC__
#include <stdint.h>
#else   /* compiled by hipRTC (the library's copybook-specialised kernels): its fixed-width types */
typedef __hip_internal::int8_t int8_t;
typedef __hip_internal::uint8_t uint8_t;
typedef __hip_internal::int16_t int16_t;
typedef __hip_internal::uint16_t uint16_t;
typedef __hip_internal::int32_t int32_t;
typedef __hip_internal::uint32_t uint32_t;
typedef __hip_internal::int64_t int64_t;
typedef __hip_internal::uint64_t uint64_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define CBX_ABI_VERSION 25

/* status codes */
#define CBX_OK 0
#define CBX_E_ARGUMENT (-1)   /* IllegalArgumentException */
#define CBX_E_STATE (-2)      /* IllegalStateException (e.g. RDW length 0 or > 100 MiB) */
#define CBX_E_CAPACITY (-3)   /* caller buffer too small; required size reported */
#define CBX_E_HIP (-4)        /* HIP runtime failure */
#define CBX_E_UNSUPPORTED (-5)

/* field decode kinds (one per DecoderSelector branch) */
enum cbx_kind {
    CBX_K_STRING = 1,      /* EBCDIC string via code page, trimmed   StringDecoders.decodeEbcdicString */
    CBX_K_STRING_ASCII = 2,/* ASCII string                            StringDecoders.decodeAsciiString  */
    CBX_K_HEX = 3,         /* debug HEX string                        StringDecoders.decodeHex          */
    CBX_K_RAW = 4,         /* debug RAW bytes                         StringDecoders.decodeRaw          */
    CBX_K_BCD = 5,         /* COMP-3                                  BCDNumberDecoders                 */
    CBX_K_BINARY = 6,      /* COMP / COMP-4 / COMP-5 / COMP-9         BinaryNumberDecoders, BinaryUtils */
    CBX_K_ZONED = 7,       /* EBCDIC DISPLAY numeric                  StringDecoders.decodeEbcdicNumber */
    CBX_K_ASCII_NUM = 8,   /* ASCII DISPLAY numeric                   StringDecoders.decodeAsciiNumber  */
    CBX_K_FLOAT = 9,       /* COMP-1                                  FloatingPointDecoders             */
    CBX_K_DOUBLE = 10,     /* COMP-2                                  FloatingPointDecoders             */
    CBX_K_RECORD_ID = 11,  /* generated Record_Id (long)              RecordExtractors.scala:409-451    */
    CBX_K_FILE_ID = 12,    /* generated File_Id (int)                                                   */
    CBX_K_UTF16_BE = 13,   /* PIC N, is_utf16_big_endian=true         StringDecoders.decodeUtf16String  */
    CBX_K_UTF16_LE = 14    /* PIC N, is_utf16_big_endian=false                                          */
};

/* output (Spark) types -- SC/schema/CobolSchema.scala:144-173 */
enum cbx_out {
    CBX_O_I32 = 1, CBX_O_I64 = 2, CBX_O_DEC64 = 3, CBX_O_DEC128 = 4,
    CBX_O_F32 = 5, CBX_O_F64 = 6, CBX_O_STRING = 7, CBX_O_BINARY = 8
};

/* cbx_field.flags */
#define CBX_F_SIGNED 0x1        /* PIC has a sign (signPosition.isDefined) */
#define CBX_F_BIG_ENDIAN 0x2    /* binary: COMP/COMP-4/COMP-5 (COMP-9 is little-endian) */
#define CBX_F_EXPLICIT_DOT 0x4  /* DISPLAY with explicit decimal point */
#define CBX_F_INTEGRAL 0x8      /* AST type is Integral (else Decimal) */
#define CBX_F_IBM 0x10          /* COMP-1/2 in IBM hex float (else IEEE-754) */
#define CBX_F_LITTLE_ENDIAN_FP 0x20
#define CBX_F_DEPENDEE 0x40     /* an OCCURS DEPENDING ON source (isDependee) */
#define CBX_F_LIST 0x80         /* element of a list-layout OCCURS DEPENDING ON array (cbx_array.offsets_column) */

/* string trimming (StringTrimmingPolicy) */
#define CBX_TRIM_NONE 1
#define CBX_TRIM_LEFT 2
#define CBX_TRIM_RIGHT 3
#define CBX_TRIM_BOTH 4

#define CBX_MAX_DIMS 4

/* One decoded leaf (a Primitive of the AST, each OCCURS element flattened into "slots").
 * Offsets are static (variable_size_occurs = false): element (i0..ik) of the field lives at
 *   offset + sum_k i_k * dim_stride[k]  relative to the record decode base. */
typedef struct {
    int32_t kind;          /* cbx_kind */
    int32_t out_type;      /* cbx_out */
    int32_t offset;        /* binaryProperties.offset */
    int32_t size;          /* binaryProperties.dataSize (bytes per element) */
    int32_t precision, scale, scale_factor;   /* AST type */
    int32_t out_precision, out_scale;         /* Spark DecimalType(p, s) */
    int32_t flags;
    int32_t trim;          /* CBX_TRIM_* for strings */
    int32_t n_dims;        /* enclosing OCCURS levels, outermost first */
    int32_t dim_count[CBX_MAX_DIMS];   /* arrayMaxSize per level */
    int32_t dim_stride[CBX_MAX_DIMS];  /* bytes per element of that level */
    int32_t dim_array[CBX_MAX_DIMS];   /* index into the cbx_array table per level */
    int32_t segment;       /* segment-redefine group this field is under, -1 if none */
    int32_t column;        /* output column */
} cbx_field;

/* One OCCURS node. Element count per record (extractArray, RecordExtractors.scala:66-114):
 *   dependee < 0 ? max : (dependee value v valid && min <= v <= max ? v : max) */
typedef struct {
    int32_t max_count, min_count;
    int32_t dependee;      /* index into the field table, -1 for a fixed OCCURS */
    int32_t segment;       /* segment of the array node, -1 if none */
    int32_t count_column;  /* output column receiving the per-record element count (int32) */
    int32_t n_dims;        /* enclosing OCCURS levels (outer arrays of this array) */
    int32_t parent;        /* enclosing array index or -1 */
    int32_t offsets_column;/* list layout (fields flagged CBX_F_LIST): output column receiving each
                              record's int64 child offset, -1 for the slot-major layout */
} cbx_array;

/* Segment ids (the `segment_field` of a multisegment file) and everything keyed by them:
 *   - segment-redefine selection (FixedLenNestedRowIterator.getSegmentId + redefine map,
 *     CP/reader/iterator/FixedLenNestedRowIterator.scala:64-99, VarLenNestedIterator.scala:91-93),
 *   - Seg_IdN generation (segment_id_level0.., SegmentIdAccumulator.scala:19-86),
 *   - segment_filter and root-reached filtering (VarLenNestedIterator.scala:138-147),
 *   - root-segment index cuts (IndexGenerator.scala:89-113).
 * A record's segment id is extractPrimitiveField(field).toString.trim (VRLRecordReader.scala:188-198):
 * for a string field the trimmed decoded text (compared with the UTF-8 key bytes), for an integral
 * field the decimal text of its value (keys that are canonical integers are compared by value:
 * key_is_int / key_int).  Each distinct key carries everything the options say about it. */
#define CBX_MAX_SEG_KEYS 32
#define CBX_MAX_SEG_KEY_LEN 32
#define CBX_MAX_SEG_LEVELS 8
#define CBX_MAX_SEG_PREFIX 64
typedef struct {
    int32_t field_offset, field_size;   /* segment-id field (relative to decode base) */
    int32_t n_keys;
    int32_t key_len[CBX_MAX_SEG_KEYS];
    uint16_t key[CBX_MAX_SEG_KEYS][CBX_MAX_SEG_KEY_LEN];  /* UTF-16 code units */
    int32_t key_segment[CBX_MAX_SEG_KEYS];   /* redefine segment the key activates, -1 none */
    int32_t key_level[CBX_MAX_SEG_KEYS];     /* first segment_id_level listing the key (0 also for a hierarchical
                                                file's root ids: index cuts, no Seg_Id column), -1 none */
    int32_t key_in_filter[CBX_MAX_SEG_KEYS]; /* 1: listed in segment_filter */
    int32_t key_is_int[CBX_MAX_SEG_KEYS];    /* integral segment field: key is a canonical integer */
    int64_t key_int[CBX_MAX_SEG_KEYS];
    int32_t field;           /* index of the segment-id field in the field table */
    int32_t field_is_int;    /* the segment-id field is integral (compared by value) */
    int32_t n_levels;        /* segment_id_level count = Seg_IdN columns */
    int32_t has_filter;      /* segment_filter given */
    int32_t level_column[CBX_MAX_SEG_LEVELS];   /* output string column of Seg_Id<l>, -1 none */
    int32_t prefix_len;
    uint8_t prefix[CBX_MAX_SEG_PREFIX];       /* segment_id_prefix, UTF-8 */
} cbx_segment_map;

typedef struct {
    int32_t n_columns;      /* value columns + count columns */
    int32_t file_id;        /* File_Id value for CBX_K_FILE_ID */
    int32_t has_segments;   /* segment map valid */
    int32_t window_bytes;   /* LDS window per record (0 = default) */
    int32_t segment_column; /* column receiving the active segment index per record, -1 none */
    int32_t jit_min_records;/* batches of at least this many records run a kernel
                               specialised for the copybook (compiled once with hipRTC);
                               0 = default (262144), < 0 = never */
    int32_t string_views;   /* string/binary columns in the Arrow string-view layout (below) */
    int32_t direct_decode;  /* 1: decode calls run the direct kernel (one lane per record, every field
                               read straight from the record's bytes -- for a plan holding a few fields of
                               a wide record, a column projection) when the plan is eligible
                               (cbx_plan_direct_eligible), the staged kernels otherwise; 0 = never */
    uint32_t lut[256];      /* code page: UTF-8 bytes (0-23), length (24-25), trimmable (31) */
    cbx_segment_map segments;
} cbx_plan_options;

/* Output column buffers (caller-owned, device memory).  Every column is n_slots(c) slot rows
 * of pitch = 64 * ceil(n_rec / 64) values (one row per OCCURS element; 1 row without OCCURS):
 * value (slot s, record r) is element s * pitch + r; elements r >= n_rec are padding the
 * kernels may overwrite.  Validity is an Arrow bitmap per slot row, 64-bit words:
 *   bit r of row s = validity[s * (pitch / 64) + r / 64] >> (r % 64).
 * Strings/binary: every slot is its own Arrow large-string array.  Slot s owns the payload
 * region data[s * data_capacity, (s + 1) * data_capacity) and the offsets
 * offsets[s * (pitch + 1) + r], r = 0 .. n_rec (absolute byte positions in `data`; entries past
 * n_rec are padding).  data_capacity = cbx_string_bound(...) always suffices; a smaller
 * capacity (e.g. from cbx_string_sizes_*) is honoured: payload never overflows its region, an
 * overflow is reported by cbx_plan_check.
 *
 * List layout of an OCCURS DEPENDING ON array (cbx_array.offsets_column >= 0; its fields flagged
 * CBX_F_LIST, numeric, one OCCURS level; Arrow ListView): a field's `values` / `validity` hold
 * the CHILD elements -- tile t of 64 records owns elements [t * 64 * M, (t + 1) * 64 * M) with
 * M = max_count rounded up to 64, record r's elements start at its offsets-column value (a
 * multiple of 64) and its count column gives their number (none where the count is null: the
 * array's segment is not the record's); the run is padded to a multiple of 64 (padding values
 * unspecified, validity bits 0) and nothing past it is written.  All CBX_F_LIST fields of an
 * array share its segment.  values need ceil(n_rec / 64) * 64 * M elements, validity
 * ceil(n_rec / 64) * M words.  The elements are decoded by a second, element-parallel kernel
 * (64 consecutive elements of one record per wave step) after the record kernel.
 *
 * String-view layout (cbx_plan_options.string_views != 0; Arrow Utf8View / BinaryView): `values`
 * holds n_slots * pitch views of 16 bytes (value (s, r) at view s * pitch + r): int32 length, then
 * the UTF-8 bytes inline when length <= 12 (zero padded), else their first 4 bytes, an int32
 * data-buffer index and an int32 offset into that buffer.  `data` holds n_slots regions of
 * data_capacity bytes; a region is cut into data buffers of buffer_bytes (the last one shorter):
 * buffer k of slot s starts at data + s * data_capacity + k * buffer_bytes
 * (cbx_string_view_geometry: a power-of-two number of whole tiles, at most 1 GiB unless one tile
 * is larger).  Long payloads start at 4-byte-aligned positions of their tile.  Every tile of 64 records owns tile_bytes of its slot's region,
 * so a value is written once, where the decode kernel produces it -- no scan over the batch and
 * no placement pass.  data_capacity must be at least ceil(n_rec / 64) * tile_bytes
 * (cbx_string_bound returns that in this layout; a smaller one fails the call with
 * CBX_E_CAPACITY).  `offsets` and `data_sizes` are unused. */
typedef struct {
    void* values;          /* fixed-width values (NULL for strings) */
    uint64_t* validity;
    int64_t* offsets;      /* strings: n_slots * (pitch + 1) entries */
    uint8_t* data;         /* strings: UTF-8 payload, n_slots regions of data_capacity bytes */
    int64_t data_capacity; /* strings: bytes per slot region */
    int64_t* data_sizes;   /* strings: device array [n_slots] receiving each slot's payload bytes (may be NULL) */
} cbx_column;

typedef struct cbx_plan cbx_plan;

int32_t cbx_abi_version(void);

/* Pipelined Arrow Utf8 batches: two plans of the same layout decoding alternate batches on two
 * streams.  Each cbx_decode_fixed / cbx_decode_var call of a linked plan (Utf8 layout) makes its
 * stream wait for the peer plan's last count pass + scan before its own, and marks its own end, so
 * one plan's count pass (HBM-read bound) runs beside the other's decode (issue bound) instead of
 * after it; count_blocks_per_cu / decode_blocks_per_cu (0: the default occupancy) cap the resident
 * workgroups per CU of the two kernels so both fit on a CU at once.  B = NULL unlinks A. */
int cbx_plan_pipeline(cbx_plan* a, cbx_plan* b, int32_t count_blocks_per_cu, int32_t decode_blocks_per_cu);
const char* cbx_last_error(void);

/* Build a plan from the flattened copybook.  Copies the tables to device memory. */
int cbx_plan_create(const cbx_field* fields, int32_t n_fields, const cbx_array* arrays,
                    int32_t n_arrays, const cbx_plan_options* opts, cbx_plan** out_plan);
void cbx_plan_destroy(cbx_plan* plan);

/* Upper bound of a string column's payload per slot for n_rec records (n_rec * field size *
 * widest UTF-8 expansion of the code page; string-view layout: ceil(n_rec / 64) * tile_bytes);
 * out_bytes[n_columns] (0 for non-string columns). */
int cbx_string_bound(const cbx_plan* plan, int64_t n_rec, int64_t* out_bytes);

/* String-view layout geometry per column (0 for non-string columns): tile_bytes[n_columns] =
 * bytes of a slot region owned by one tile of 64 records, buffer_bytes[n_columns] = bytes per
 * Arrow data buffer of a slot (a whole number of tiles, at most 1 GiB). */
int cbx_string_view_geometry(const cbx_plan* plan, int64_t* tile_bytes, int64_t* buffer_bytes);

/* Exact payload sizes (optional pre-pass, synchronous): out_sizes[n_columns] receives, per
 * string column, the largest slot payload of the batch (0 for non-string columns). */
int cbx_string_sizes_fixed(cbx_plan* plan, const uint8_t* d_records, int64_t n_rec,
                           int32_t rec_stride, int32_t start_offset, int64_t* out_sizes, void* stream);

/* Fixed-length batch: record i occupies d_records[i*rec_stride, (i+1)*rec_stride) and is
 * decoded at +start_offset (CobolScanners.buildScanForFixedLength; record_start_offset).
 * Bounds rules of Primitive.decodeTypeValue apply against rec_stride.  Asynchronous on
 * `stream` (one kernel launch); calls on one plan must be issued in order on one stream. */
int cbx_decode_fixed(cbx_plan* plan, const uint8_t* d_records, int64_t n_rec, int32_t rec_stride,
                     int32_t start_offset, int64_t first_record_id, cbx_column* columns, void* stream);

/* Variable-length batch: record i is d_data[rec_off[i], rec_off[i] + rec_len[i]) (payload
 * without RDW), decoded at +start_offset; shorter records yield null numerics / truncated strings. */
int cbx_decode_var(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, const int64_t* d_rec_off,
                   const int32_t* d_rec_len, int64_t n_rec, int32_t start_offset,
                   int64_t first_record_id, cbx_column* columns, void* stream);
int cbx_string_sizes_var(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, const int64_t* d_rec_off,
                         const int32_t* d_rec_len, int64_t n_rec, int32_t start_offset,
                         int64_t* out_sizes, void* stream);

/* Multi-GPU shards of one variable-length file: d_base is a device int64 (e.g. the
 * exclusive prefix of the ranks' framed record counts, all-gathered on the device) that every later
 * decode call of the plan adds to its first_record_id when it writes Record_Id -- the shard's base
 * never visits the host.  NULL clears it.  The pointer must stay valid while calls are in flight.
 * Replaces the startingRecordIndex a Spark task passes to VarLenNestedReader.getRowIterator
 * (SC/reader/VarLenNestedReader.scala:52-81). */
int cbx_plan_set_record_base(cbx_plan* plan, const int64_t* d_base);

/* Hierarchical records (segment-children): OCCURS DEPENDING ON counts the caller resolved itself.
 * d_counts: device int32[n_arrays][pitch] -- entry (a, r) the element count of the plan's array a in
 * record r of the following decode calls (cbx_decode_selected / cbx_decode_var / cbx_decode_fixed),
 * < 0: the count the record's own dependee gives.  Replaces the dependFields map that
 * RecordExtractors.extractHierarchicalRecord shares between the segments of one hierarchical record
 * (CP/reader/extractors/record/RecordExtractors.scala:224-245): a child segment's array depending on
 * a field of its parent segment (or of a segment decoded earlier in the record) takes the value
 * registered there.  NULL clears it; the pointer must stay valid while calls are in flight.
 * CBX_E_UNSUPPORTED on a record-walk plan. */
int cbx_plan_set_odo_counts(cbx_plan* plan, const int32_t* d_counts, int64_t pitch);

/* Synchronise `stream` and report device-side errors of the plan's earlier decode calls
 * (CBX_E_CAPACITY: a string payload exceeded data_capacity). */
int cbx_plan_check(cbx_plan* plan, void* stream);

/* Optional kernel timing with HIP events on the call's stream (bench / profiling): while
 * enabled, every decode call records events around its decode kernel and around its post
 * passes (fixup of deferred values, string scan + placement), without synchronising.
 * cbx_plan_kernel_times waits for the recorded events, returns up to max_calls per-call
 * durations in ms (oldest first, *n_calls of them) and clears the record. */
int cbx_plan_set_profiling(cbx_plan* plan, int32_t enable);
int cbx_plan_kernel_times(cbx_plan* plan, float* decode_ms, float* post_ms, int32_t max_calls, int32_t* n_calls);

/* Which decode kernel the plan's last decode call ran: *kind = 0 the table-driven kernel,
 * 2 the record walk (cbx_plan_set_walk), 3 its copybook-specialised form,
 * 1 the copybook-specialised kernel, 4 the direct kernel (cbx_plan_options.direct_decode).  If
 * specialisation was attempted and failed, *kind = 0 and the reason is in cbx_last_error() (the call
 * itself succeeded on the table-driven kernel). */
int cbx_plan_kernel_kind(cbx_plan* plan, int32_t* kind);

/* How the plan's last decode call launched its decode kernel: the kernel kind, the way a tile's
 * records were staged into LDS and the launch geometry (read-only; tests pin the dispatch with it).
 * The staging fields describe the staged kernels (kind 0 / 1); the record walk and the direct kernel
 * (kind 2 / 3 / 4) report the kind alone, the other fields zero. */
typedef struct cbx_launch_info {
    int32_t kind;          /* as cbx_plan_kernel_kind */
    int32_t staging;       /* 0 windowed, 1 contiguous, 2 span */
    int32_t coop;          /* cooperative tiles: one tile per workgroup */
    int32_t kp;            /* 16-byte chunks per lane (contiguous / span), else 0 */
    int32_t padded_rows;   /* contiguous: LDS rows padded to an odd dword pitch (pitch != stride) */
    int32_t n_windows;     /* windows of the op set used */
    int32_t global_window; /* the op set has a global (HBM) window with fields in it */
    int32_t count_kernel;  /* Utf8 count pass: 0 none, 1 specialised, 2 table-driven mode 1 */
    int32_t base_shift;    /* data pointer & 15 */
    int32_t reserved;
    int64_t grid, blocks_needed;   /* workgroups launched / workgroups that cover every tile once */
} cbx_launch_info;
int cbx_plan_launch_info(cbx_plan* plan, cbx_launch_info* out);

/* How the plan's last decode call launched the record walk (cbx_plan_set_walk; read-only, tests pin the
 * dispatch with it).  CBX_E_STATE when the plan's last decode call was not a walk (kind 2 / 3).  Whether
 * a given tile was staged depends on the data: a tile whose records span lo..hi bytes of the data is
 * staged when hi - lo + ((data + lo) & 15) <= stage_cap, and read from HBM otherwise. */
typedef struct cbx_walk_info {
    int32_t kind;          /* 2 the table-driven walk, 3 its copybook-specialised form */
    int32_t stage_cap;     /* LDS bytes per wave for a tile's record span (0: CBX_WALK_NO_STAGE) */
    int32_t vlds;          /* validity words and string cursors accumulate in LDS (0: global atomics) */
    int32_t wave_lds;      /* LDS bytes per wave: frame stack + stage + (vlds) words and cursors */
    int32_t depth;         /* frame-stack depth of the copybook */
    int32_t stack_lds;     /* LDS bytes of the frame stack per wave (0 for kind 3: frames in registers) */
    int32_t n_vslots;      /* validity words per tile: every slot of every column */
    int32_t n_sslots;      /* string column slots (one payload cursor each) */
    int64_t grid, n_tiles; /* workgroups launched (4 waves each) / tiles of 64 records */
} cbx_walk_info;
int cbx_plan_walk_info(cbx_plan* plan, cbx_walk_info* out);

/* Whether decode calls of the plan would run the direct kernel with direct_decode = 1: *eligible = 1,
 * or 0 with the reason in cbx_last_error().  Eligible: no record walk, no OCCURS array, no list
 * layout, no Seg_Id level column, string columns absent or in the string-view layout, no pipeline
 * peer (cbx_plan_pipeline).  An ineligible plan runs the staged kernels; that is not an error. */
int cbx_plan_direct_eligible(const cbx_plan* plan, int32_t* eligible);

/* Which step the plan's last cbx_frame_var_occurs call walked records with: *kind = 0 the
 * table-driven walk_length, 1 its copybook-specialised form (hipRTC, from jit_min_records records
 * estimated at the copybook's largest record; same records, tested on both). */
int cbx_plan_frame_kind(cbx_plan* plan, int32_t* kind);

/* The copybook-specialised kernel of a plan (its contiguous fixed-length variant when the layout
 * has one, else the windowed variant): writes its HIP source
 * (NUL-terminated, truncated to source_cap) and its length; with compile != 0 also compiles it
 * for gfx950 with hipRTC (no device needed) and reports a failure with the compiler log in
 * cbx_last_error().  Decode calls build and use it on their own (cbx_plan_options.jit_min_records);
 * this entry point is for inspection, ahead-of-time warm-up and tests. */
int cbx_plan_specialize(cbx_plan* plan, char* source, int64_t source_cap, int64_t* source_len, int32_t compile);

/* RDW header walk on the GPU (RecordHeaderParserRDW + VRLRecordReader), seeded by sparse-index
 * entry points: seeds[k] is a known record-header offset (offsetFrom of an index entry), the
 * chain from seeds[k] is walked up to seeds[k+1] (or n_bytes).  Writes payload offsets/lengths
 * of valid records in file order; *n_records receives the count. */
typedef struct {
    int32_t big_endian;         /* is_rdw_big_endian */
    int32_t adjustment;         /* rdw_adjustment (+ -4 if is_rdw_part_of_record_length) */
    int32_t file_header_bytes;  /* file_start_offset */
    int32_t file_footer_bytes;  /* file_end_offset */
} cbx_rdw_params;

int cbx_frame_rdw(const uint8_t* d_data, int64_t n_bytes, const int64_t* seeds, int32_t n_seeds,
                  const cbx_rdw_params* params, int64_t* d_rec_off, int32_t* d_rec_len,
                  int64_t capacity, int64_t* n_records, void* stream);

/* The same walk with no host wait: everything is enqueued on `stream` and the outcome stays on the
 * device in d_state (int64[3]): [0] the record count, [1] the first header error (-1: none; else
 * offset << 2 | kind, kind 2 = zero-length header, 3 = header above 100 MB), [2] flags (1: more
 * records than capacity).  max_rounds parallel fix rounds (0 = 3) run before a one-wave pass on the
 * device settles whatever they left (a no-op when the last round changed nothing).  A
 * multi-GPU step all-gathers d_state[0] on the device (the Record_Id bases) and decodes with the
 * count its index run predicts; cbx_frame_rdw_state reads d_state afterwards (one host wait) and
 * returns the error cbx_frame_rdw would have returned, *n_records the count.
 * (Replaces the host out-parameter of VRLRecordReader's sequential count, VarLenNestedIterator.scala:80-147,
 * for the all-gather RCCL performs) */
int cbx_frame_rdw_async(const uint8_t* d_data, int64_t n_bytes, const int64_t* seeds, int32_t n_seeds,
                        const cbx_rdw_params* params, int64_t* d_rec_off, int32_t* d_rec_len,
                        int64_t capacity, int64_t* d_state, int32_t max_rounds, void* stream);
int cbx_frame_rdw_state(const int64_t* d_state, int64_t* n_records, void* stream);

/* ---- variable-length record streams: sparse index, record selection, selected decode ----
 *
 * Sparse index (IndexGenerator.sparseIndexGenerator, CP/reader/index/IndexGenerator.scala:33-157,
 * called by VarLenNestedReader.generateIndex, CP/reader/VarLenNestedReader.scala:125-180) over a
 * file already framed on the GPU (cbx_frame_rdw over the whole file, or fixed-length records).
 * Entries are cut every records_per_entry records, or by size: bytes_per_entry with
 * subtract_size != 0 (input_split_size_mb / HDFS block size: the split size is subtracted, not
 * reset), or the 100 MB default (reset); with `hierarchical` only at records whose segment id is
 * a level-0 key of the plan's segment map.  The first entry is (0, -1, file_id, 0); the last
 * entry's offset_to is -1.  record_index counts every header read (the file header record too).
 * start_bytes: IndexGenerator's bytesInChunk as of the first framed record, which is taken as an entry
 * already cut -- 0 for a whole file; for a piece of a file that starts at one of the file's entries, that
 * entry's residual under the subtracting size split (its header offset minus the split size times the
 * cuts up to it): the piece's entries are then the file's (shard.index_chain). */
typedef struct {
    int64_t offset_from, offset_to;
    int64_t record_index;
    int32_t file_id;
    int32_t reserved;
} cbx_index_entry;

typedef struct {
    int64_t records_per_entry;  /* input_split_records; 0 = split by size */
    int64_t bytes_per_entry;    /* split size in bytes when records_per_entry == 0 */
    int32_t subtract_size;      /* isSplitBySize: an explicit MB size (subtracted) vs the default (reset) */
    int32_t header_bytes;       /* record header length: 4 (RDW) or 0 (fixed-length record parser) */
    int32_t has_file_header;    /* a file-header record precedes the first framed record */
    int32_t hierarchical;       /* cut only at level-0 segment records (segment levels given) */
    int32_t file_id;
    int32_t reserved;
    int64_t start_bytes;        /* bytesInChunk at the first framed record (0: a whole file) */
} cbx_index_params;

int cbx_sparse_index(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, const int64_t* d_rec_off,
                     const int32_t* d_rec_len, int64_t n_rec, const cbx_index_params* params,
                     cbx_index_entry* entries, int64_t capacity, int64_t* n_entries, void* stream);

/* Record selection over framed records (VarLenNestedIterator.fetchNext + VRLRecordReader record
 * numbering, CP/reader/iterator/VarLenNestedIterator.scala:80-147, VRLRecordReader.scala:55-74):
 * records are numbered per index entry (Record_Id = entry.record_index + ordinal inside the entry;
 * entries = NULL: one entry (0, -1, file_id, 0)), Seg_IdN state is accumulated per entry,
 * records before the first root of an entry (when segment levels are given) and records outside
 * segment_filter are dropped.  Output arrays (device, capacity n_rec each) receive the selected
 * records in file order; seg_state holds (1 + n_levels) int64 per record: the root record id
 * (-1: no root seen in the entry) then per level -2 (null) or the level counter. */
typedef struct {
    int64_t* rec_off;          /* payload offsets */
    int32_t* rec_len;          /* payload lengths */
    int64_t* record_id;        /* Record_Id */
    int32_t* segment;          /* active segment redefine index, -1 none */
    int64_t* seg_state;        /* [n][1 + n_levels], may be NULL when the plan has no levels */
    int32_t file_id;           /* File_Id of the batch (written by cbx_decode_selected) */
    int32_t footer_bytes;      /* in: file_end_offset -- the reference bounds each entry's stream to
                                  offset_to and its header parser then reads records within
                                  file_end_offset of that bound as the footer: they are dropped */
} cbx_selection;

int cbx_select_records(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, const int64_t* d_rec_off,
                       const int32_t* d_rec_len, int64_t n_rec, int32_t start_offset,
                       const cbx_index_entry* entries, int32_t n_entries, cbx_selection* out,
                       int64_t* n_selected, void* stream);

/* Decode selected records: as cbx_decode_var, with Record_Id and the active segment taken from
 * the selection and the Seg_IdN string columns written from its seg_state
 * (SegmentIdAccumulator.getSegmentLevelId: prefix_fileId_rootRecordId[_L<level>_<counter>]). */
int cbx_decode_selected(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, const cbx_selection* sel,
                        int64_t n_rec, int32_t start_offset, cbx_column* columns, void* stream);

/* ---- row filters pushed down to the GPU ----
 *
 * What Spark's PrunedFilteredScan.buildScan(requiredColumns, filters) hands a relation, evaluated before
 * the decode so that only surviving records are decoded and written (the reference filters rows after
 * RecordExtractors.extractRecord, on a lazy iterator).  cbx_filter is a predicate table in conjunctive
 * normal form: terms of one `group` are OR-ed, groups are AND-ed; terms are listed with non-decreasing
 * group; an empty table keeps every record.  A term compares one field of the plan's cbx_field table
 * with its literals [lit_begin, lit_begin + lit_count).
 * SQL three-valued logic: a comparison with a null value is unknown, a record is kept only when the
 * whole filter is true.  A field is null exactly where the decode makes it null: a malformed value, a
 * numeric reaching past the record's end, a field of a segment redefine that is not the record's
 * active segment (and a string starting past the record's end); a string cut by a short record
 * compares as the truncated value.  Negated comparisons are ops of their own (no NOT node: under
 * three-valued logic NOT(a < b) and a >= b keep the same rows).
 * Numerics compare as the column's output value (int32 / int64 / the unscaled decimal at the Spark
 * scale, 128-bit signed for precision > 18) with literals given as 128-bit two's complement at that
 * scale; strings compare as the decoded UTF-8 bytes (code page, trimming) in unsigned byte order
 * (UTF8String.compareTo) with literals held in `pool`. */
#define CBX_FILTER_MAX_TERMS 32
#define CBX_FILTER_MAX_LITERALS 64
#define CBX_FILTER_POOL_BYTES 1024
enum cbx_filter_op {
    CBX_OP_EQ = 1, CBX_OP_NE = 2, CBX_OP_LT = 3, CBX_OP_LE = 4, CBX_OP_GT = 5, CBX_OP_GE = 6,
    CBX_OP_IN = 7, CBX_OP_NOT_IN = 8,              /* any / none of lit_count literals equal */
    CBX_OP_IS_NULL = 9, CBX_OP_IS_NOT_NULL = 10,   /* no literal */
    CBX_OP_STARTS_WITH = 11, CBX_OP_NOT_STARTS_WITH = 12,  /* strings, one literal */
    /* (additive extension of ABI 25; cbx_filter_max_op tells whether the library evaluates them)
     * strings, one literal: the literal's bytes are a suffix of / occur in the decoded UTF-8 bytes, compared
     * byte-wise as UTF8String.endsWith / contains do (a literal may begin or end inside a character).  An
     * empty literal is true for every non-null value; a null value is unknown for the op and its negation. */
    CBX_OP_ENDS_WITH = 13, CBX_OP_NOT_ENDS_WITH = 14,
    CBX_OP_CONTAINS = 15, CBX_OP_NOT_CONTAINS = 16
};
typedef struct {
    uint64_t lo, hi;       /* numeric fields: two's complement 128-bit value at the field's output scale */
    int32_t str_off;       /* string fields: UTF-8 bytes pool[str_off, str_off + str_len) */
    int32_t str_len;
} cbx_filter_literal;
typedef struct {
    int32_t field;         /* index into the plan's cbx_field table */
    int32_t op;            /* cbx_filter_op */
    int32_t group;         /* terms of one group are OR-ed, groups AND-ed */
    int32_t lit_begin, lit_count;
    int32_t reserved;
} cbx_filter_term;
typedef struct {
    int32_t n_terms, n_literals, pool_bytes, reserved;
    cbx_filter_term terms[CBX_FILTER_MAX_TERMS];
    cbx_filter_literal literals[CBX_FILTER_MAX_LITERALS];
    uint8_t pool[CBX_FILTER_POOL_BYTES];
} cbx_filter;

/* The records of one source that `filter` keeps, in source order, as a selection cbx_decode_selected
 * takes.  Sources (exactly one):
 *   in != NULL:          the n_rec rows of a selection (cbx_select_records): record ids, active segment
 *                        and seg_state are carried over;
 *   d_rec_off/d_rec_len: framed records (payload offsets / lengths);
 *   rec_stride > 0:      fixed-length records, record i at d_data + i * rec_stride.
 * For the last two Record_Id = first_record_id + i and the active segment comes from the plan's segment
 * map as cbx_select_records takes it (-1 without one); a plan with Seg_Id levels needs a selection.
 * out's arrays (capacity n_rec each, distinct from in's) receive the kept rows; *n_selected their count
 * (one host wait).  Three passes on `stream`: test (one lane per record: the terms' fields are decoded
 * from the record's bytes, a keep bit per record and a count per 64 records stored), scan of the
 * counts, emit.
 * CBX_E_UNSUPPORTED (reason in cbx_last_error): a field inside an OCCURS; a record-walk plan
 * (data-dependent offsets); a comparison on COMP-1 / COMP-2 (IS_NULL / IS_NOT_NULL are fine); UTF-16,
 * HEX and RAW fields; generated columns.  CBX_E_ARGUMENT: a malformed table. */
int cbx_filter_records(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, const cbx_selection* in,
                       const int64_t* d_rec_off, const int32_t* d_rec_len, int64_t n_rec, int32_t rec_stride,
                       int32_t start_offset, int64_t first_record_id, const cbx_filter* filter,
                       cbx_selection* out, int64_t* n_selected, void* stream);

/* Durations in ms of the three passes of the plan's last cbx_filter_records call, measured with HIP
 * events on its stream while cbx_plan_set_profiling is on (zeros otherwise). */
int cbx_filter_pass_times(cbx_plan* plan, float* test_ms, float* scan_ms, float* emit_ms);

/* The highest cbx_filter_op this library evaluates (16: CBX_OP_NOT_CONTAINS); a term with a higher op is
 * CBX_E_ARGUMENT "unknown op".  ABI-25 libraries without this symbol evaluate ops up to
 * CBX_OP_NOT_STARTS_WITH: enum values add no symbol, so this is how a caller tells the two apart. */
int32_t cbx_filter_max_op(void);

/* ---- aggregate pushdown ----
 *
 * What Spark's SupportsPushDownAggregates.pushAggregation hands a data source: COUNT(*), COUNT(col),
 * MIN, MAX and SUM over the rows a filter keeps, computed from the records' bytes -- no selection and no
 * column is written.  cbx_aggregate lists up to CBX_AGG_MAX_TERMS terms, each one field of the plan's
 * cbx_field table with a bit mask of functions (a field is decoded once however many functions are
 * asked of it; a field appears in one term only; an empty table is COUNT(*) alone).
 * The value aggregated is exactly the one the filter compares: null where the decode makes the field
 * null (a malformed value, a numeric reaching past the record's end, a field of a segment redefine that
 * is not the record's active segment, a string starting past the record's end), else the column's
 * output value (int32 / int64 / the unscaled decimal at the Spark scale) as a signed 128-bit number.
 * Nulls are skipped, as SQL aggregates skip them.
 * Result: n_rows is the number of records the filter keeps (COUNT(*)); per term `count` is the number
 * of non-null values of its field (kept whatever the mask), min / max are 128-bit two's complement and
 * sum is 192-bit two's complement in three little-endian limbs -- |value| < 2^127 and fewer than 2^63
 * records, so the sum is exact and does not depend on the order of addition.  min, max and sum are
 * meaningful only when count > 0 and their function was asked for, and are zero otherwise.  Two
 * results over disjoint records merge by adding n_rows, count and sum and taking the smaller min /
 * larger max of the sides with count > 0. */
#define CBX_AGG_MAX_TERMS 16
enum cbx_aggregate_func { CBX_AGG_COUNT = 1, CBX_AGG_MIN = 2, CBX_AGG_MAX = 4, CBX_AGG_SUM = 8 };
typedef struct {
    int32_t field;         /* index into the plan's cbx_field table */
    int32_t funcs;         /* cbx_aggregate_func bits, not empty */
} cbx_aggregate_term;
typedef struct {
    int32_t n_terms, reserved;
    cbx_aggregate_term terms[CBX_AGG_MAX_TERMS];
} cbx_aggregate;
typedef struct {
    int64_t count;
    uint64_t min_lo, min_hi, max_lo, max_hi;
    uint64_t sum[3];
} cbx_aggregate_value;
typedef struct {
    int64_t n_rows;
    cbx_aggregate_value values[CBX_AGG_MAX_TERMS];   /* values[t]: term t; zeros past n_terms */
} cbx_aggregate_result;

/* Aggregate the records of one source that `filter` keeps (NULL: every record) into *result (host
 * memory).  Sources (exactly one) as for cbx_filter_records: a selection, framed records, or
 * fixed-length records; the active segment comes from the selection or from the plan's segment map.
 * Unlike the filter a plan with Seg_Id levels needs no selection: no seg_state is carried.
 * n_rec == 0 gives a zeroed result and launches nothing.  Otherwise two launches on `stream`: the
 * accumulate pass, a grid-stride loop over tiles of 64 records run by at most max_workgroups
 * workgroups (0: the library's choice; a caller that shares the device gives fewer), each storing one
 * partial result, and the combine pass, one workgroup that merges them; then one host wait for the
 * copy of the result.  The result does not depend on max_workgroups.
 * CBX_E_UNSUPPORTED (reason in cbx_last_error): a field inside an OCCURS; a record-walk plan; UTF-16,
 * HEX and RAW fields; generated columns; MIN, MAX or SUM on COMP-1 / COMP-2 (a float sum depends on
 * the order, NaN ordering is not modelled) or on a string field (COUNT is fine for both); and whatever
 * cbx_filter_records refuses in `filter`.  CBX_E_ARGUMENT: a malformed table, a repeated field, an
 * empty function mask, max_workgroups < 0. */
int cbx_aggregate_records(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, const cbx_selection* in,
                          const int64_t* d_rec_off, const int32_t* d_rec_len, int64_t n_rec, int32_t rec_stride,
                          int32_t start_offset, const cbx_filter* filter, const cbx_aggregate* aggregate,
                          int32_t max_workgroups, cbx_aggregate_result* result, void* stream);

/* Durations in ms of the two passes of the plan's last cbx_aggregate_records call, measured with HIP
 * events on its stream while cbx_plan_set_profiling is on (zeros otherwise). */
int cbx_aggregate_pass_times(cbx_plan* plan, float* accumulate_ms, float* combine_ms);

/* ---- grouped aggregates (GROUP BY): an additive extension of ABI 24 ----
 *
 * SELECT k1..kK, COUNT(*), f(c).. FROM records WHERE filter GROUP BY k1..kK, what pushAggregation hands a
 * data source when Aggregation.groupByExpressions is not empty.  No structure and no entry point above
 * changes, so CBX_ABI_VERSION stays 24; a caller checks for the three entry points below.
 * A key's value is the column's output value exactly as the filter and the aggregates see it: a numeric
 * key is the signed 128-bit value at the column's scale, a string key the UTF-8 bytes of the trimmed field
 * through the plan's code page.  Keys group by that decoded value, never by the record's bytes: the sign
 * nibbles of a COMP-3 zero, the overpunch spellings of one zoned number, strings that differ in trimmed
 * padding or in two source bytes with one code-page image are one group.  NULL (a malformed numeric, a
 * numeric reaching past the record's end, a field of an inactive segment redefine, a string starting past
 * the record's end) is a key value of its own; the empty string is another.
 * Keys: up to CBX_GROUP_MAX_KEYS distinct fields, numeric (COMP-3, binary, zoned, ASCII numeric, any output
 * type) or EBCDIC / ASCII strings of at most 32 bytes; a key may also be aggregated.
 * Per group: n_rows (COUNT(*)) and per term a cbx_aggregate_value with the meaning it has above.  The
 * order of the groups is unspecified.  The result does not depend on max_workgroups or on timing.
 * max_groups >= 1 bounds the number of distinct keys: the call gives the exact result when there are at
 * most max_groups of them, and otherwise sets header->overflow (status CBX_OK): no group data is to be
 * trusted then.  The workspace is a table of `capacity` slots (the power of two >= 2 * max_groups) of
 * 16 + 64 * n_terms bytes plus device copies of the output arrays; CBX_E_ARGUMENT when it would exceed
 * CBX_GROUP_MAX_WORKSPACE_BYTES. */
#define CBX_GROUP_MAX_KEYS 4
#define CBX_GROUP_MAX_WORKSPACE_BYTES 0x40000000ll   /* 1 GiB */
typedef struct {
    int32_t n_keys;                        /* 1 .. CBX_GROUP_MAX_KEYS */
    int32_t fields[CBX_GROUP_MAX_KEYS];    /* indices into the plan's cbx_field table, no repeats */
    int32_t reserved[3];
} cbx_group_by;
typedef struct {
    uint64_t lo, hi;       /* numeric key: 128-bit two's complement at the column's scale; zero otherwise */
    int32_t is_null;
    int32_t str_len;       /* string key: UTF-8 bytes at key_bytes[g * str_stride + str_off[k]]; else 0 */
} cbx_group_key;
typedef struct {
    int32_t str_stride;                    /* bytes of key_bytes per group (3 per source byte of every string key) */
    int32_t str_off[CBX_GROUP_MAX_KEYS];   /* where key k's bytes start inside a group's stride */
    int32_t reserved[3];
    int64_t capacity;                      /* slots of the table */
    int64_t workspace_bytes;               /* device memory the call allocates from the stream's pool */
} cbx_group_strides;
typedef struct {
    int64_t* n_rows;                 /* [max_groups] */
    cbx_aggregate_value* values;     /* [max_groups][n_terms], NULL when n_terms == 0 */
    cbx_group_key* keys;             /* [max_groups][n_keys] */
    uint8_t* key_bytes;              /* [max_groups][str_stride], NULL when str_stride == 0 */
} cbx_group_output;
typedef struct {
    int64_t n_rows;        /* records the filter keeps (the sum of the groups' n_rows) */
    int64_t n_groups;
    int32_t overflow;      /* more than max_groups distinct keys: nothing else is to be trusted */
    int32_t reserved;
} cbx_group_header;

/* The strides and the workspace size of a grouped call: validates the tables as the call itself does. */
int cbx_group_layout(cbx_plan* plan, const cbx_group_by* group_by, const cbx_aggregate* aggregate,
                     int64_t max_groups, cbx_group_strides* strides);

/* As cbx_aggregate_records, per distinct key of `group_by`: out's host arrays (sized by max_groups and the
 * strides above) receive header->n_groups groups.  n_rec == 0 launches nothing and gives zero groups.
 * Otherwise, on `stream`: the table's init, the accumulate pass (one lane per record finds or claims its
 * key's slot -- a slot names a representative record, its key is that record's key -- and the tile's values
 * go through a wave-private cache of running accumulators to device-scope 64-bit atomics), the emit pass
 * (one lane per slot); then a host wait for the header and one for the copies of exactly n_groups groups.
 * CBX_E_UNSUPPORTED (reason in cbx_last_error): whatever cbx_aggregate_records refuses for a field or in
 * `filter`; a COMP-1 / COMP-2 key; a string key longer than 32 bytes; MIN or MAX of a DEC128 column (there
 * is no 128-bit atomic; COUNT and SUM of it are fine).  CBX_E_ARGUMENT: a malformed table, a repeated key,
 * max_groups < 1, a workspace above the limit. */
int cbx_aggregate_grouped(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, const cbx_selection* in,
                          const int64_t* d_rec_off, const int32_t* d_rec_len, int64_t n_rec, int32_t rec_stride,
                          int32_t start_offset, const cbx_filter* filter, const cbx_aggregate* aggregate,
                          const cbx_group_by* group_by, int64_t max_groups, int32_t max_workgroups,
                          const cbx_group_output* out, cbx_group_header* header, void* stream);

/* Durations in ms of the passes of the plan's last cbx_aggregate_grouped call (init, accumulate, emit),
 * measured with HIP events on its stream while cbx_plan_set_profiling is on (zeros otherwise). */
int cbx_group_pass_times(cbx_plan* plan, float* init_ms, float* accumulate_ms, float* emit_ms);

/* ---- Top-N (ORDER BY .. LIMIT n) and LIMIT: an additive extension of ABI 25 ----
 *
 * SELECT .. WHERE filter ORDER BY k1 [DESC], .. LIMIT n, what SupportsPushDownTopN.pushTopN and
 * SupportsPushDownLimit.pushLimit hand a data source.  No structure and no entry point above changes, so
 * CBX_ABI_VERSION stays 25; a caller checks for the three entry points below.
 * Of the rows `filter` keeps (NULL: every row) the call returns the min(limit, kept) rows that come first
 * under `order`; rows equal on every key are taken by source position, the lower index first.  The rows are
 * written IN SOURCE ORDER as a selection for cbx_decode_selected (record ids, active segment and seg_state
 * carried as cbx_filter_records carries them): a caller that merges several batches, index entries or
 * shards orders and limits the union itself (Spark: isPartiallyPushed() == true).  n_keys == 0 is the plain
 * LIMIT: the first `limit` kept rows.  limit >= kept returns what cbx_filter_records returns.  The result
 * does not depend on max_workgroups or on timing.
 * Keys: up to CBX_TOPN_MAX_KEYS distinct fields.  A key's value is the column's output value exactly as the
 * filter and the aggregates see it: a numeric key the signed value at the column's scale (128 bits for a
 * precision above 18), a string key the UTF-8 bytes of the trimmed field through the plan's code page,
 * compared as unsigned bytes (UTF8String.compareTo); a string cut by a short record orders as the cut
 * value.  A key is NULL where the filter finds the field null.  Default per key: ascending, NULLS FIRST.
 * Method (cbx_topn.h): an exact radix select over the records' composite sort key, 64 bits of it at a time.
 * Workspace from the stream's pool: 8 bytes per source record (the current level's key words), two 64-bit
 * words and two counts per 64 records, 2 bytes per record when the active segment comes from the plan's
 * segment map, and 24 bytes per record of the tie class level 0 leaves (two buffers, allocated when a
 * further level runs).  Host waits: one per level that runs (a level decides all but the records equal on
 * its 64 bits; the last level is the source index, which always decides), plus one for the final count.
 * limit == 0 or n_rec == 0 launches nothing.
 * CBX_E_UNSUPPORTED (reason in cbx_last_error): whatever cbx_filter_records refuses for a field or in
 * `filter`; a COMP-1 / COMP-2 key; a string key longer than 32 source bytes.  CBX_E_ARGUMENT: a malformed
 * table, a repeated field, unknown flag bits, limit < 0, max_workgroups < 0, n_rec > INT32_MAX, the
 * argument errors of cbx_filter_records (sources, Seg_Id levels without a selection, shared arrays). */
#define CBX_TOPN_MAX_KEYS 4
enum cbx_sort_flags { CBX_SORT_DESC = 1, CBX_SORT_NULLS_LAST = 2 };
typedef struct {
    int32_t field;         /* index into the plan's cbx_field table */
    int32_t flags;         /* cbx_sort_flags bits */
} cbx_sort_key;
typedef struct {
    int32_t n_keys;        /* 0 .. CBX_TOPN_MAX_KEYS */
    int32_t reserved;
    cbx_sort_key keys[CBX_TOPN_MAX_KEYS];
} cbx_sort_order;
typedef struct cbx_topn_info {
    int64_t n_live;               /* rows the filter kept; -1 when the call launched nothing for limit == 0 */
    int64_t ties_after_level0;    /* records equal to the threshold on the first 64 key bits that went to level 1 */
    int64_t ties_max;             /* the largest tie class handed to a further level */
    int64_t grid;                 /* workgroups of the select passes (0: no select ran) */
    int32_t levels_run;           /* select levels run (0: limit >= n_rec, or nothing launched) */
    int32_t levels_total;         /* 64-bit words of the composite key, the source index included */
    int32_t words_per_key[CBX_TOPN_MAX_KEYS];   /* words of the composite key that hold bytes of key k */
} cbx_topn_info;

/* Sources (exactly one) and `out` as for cbx_filter_records.  max_workgroups bounds the grids of the select
 * passes for a caller that shares the device (0: the library's choice). */
int cbx_top_n_records(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, const cbx_selection* in,
                      const int64_t* d_rec_off, const int32_t* d_rec_len, int64_t n_rec, int32_t rec_stride,
                      int32_t start_offset, int64_t first_record_id, const cbx_filter* filter,
                      const cbx_sort_order* order, int64_t limit, int32_t max_workgroups, cbx_selection* out,
                      int64_t* n_selected, void* stream);

/* How the plan's last Top-N call ran (host code only, no GPU work). */
int cbx_top_n_info(cbx_plan* plan, cbx_topn_info* out);

/* Durations in ms of the plan's last Top-N call: the key pass, the select levels (host waits between them
 * included) and count + scan + emit, measured with HIP events while cbx_plan_set_profiling is on. */
int cbx_top_n_pass_times(cbx_plan* plan, float* key_ms, float* select_ms, float* emit_ms);

/* ---- key-set filters (semi-join pushdown): an additive extension of ABI 25 ----
 *
 * WHERE (k1..kK) IN (<a set of tuples>) and WHERE k NOT IN (<a set of values>) for sets past the 64 literals of a
 * cbx_filter: what Spark's dynamic partition pruning and runtime filters hand a relation as In sets of hundreds
 * to millions of keys.  No structure and no entry point above changes, so CBX_ABI_VERSION stays 25; a caller
 * checks for the four entry points below.
 * A key set is built once over 1 to CBX_GROUP_MAX_KEYS distinct key fields of one plan from n_values >= 0 tuples
 * of key values, lives on the device until it is destroyed, and is probed by any number of keyed filter calls
 * of that plan on any stream.  A key value is exactly what the grouped aggregate emits for a group (cbx_group_key
 * without the null flag): a numeric key the signed 128-bit value at the column's output scale, a string key the
 * UTF-8 bytes of the trimmed field through the plan's code page.  The accepted and refused key fields are those
 * of the grouped aggregate, with its reasons.  Duplicate tuples are one member; a set has no null member (a
 * cbx_key_value has no null flag: what a null in the caller's list means is the caller's matter).
 * The keyed filter keeps a record when all of these hold: its cbx_filter is true, if one is given; for every set
 * with negate == 0 every key field of the record is non-null and the tuple is a member; for every set with
 * negate != 0 the key is non-null and its value is not a member (single-column sets only).  A key is null exactly
 * where the grouped aggregate makes it null, and a record with a null key component is kept by neither form (SQL
 * three-valued logic: unknown is not true).  The result depends neither on the order of the values nor on timing.
 * Table (cbx_keyset.h): open addressing with linear probing over `capacity` slots, the power of two at or above
 * 2 * max(1, n_values); a slot is one 64-bit word, 0 when empty, else a 32-bit fingerprint of the key's hash in
 * the high half and the value's index + 1 in the low half; the uploaded value array is the key storage. */
typedef struct {
    uint64_t lo, hi;       /* numeric key: 128-bit two's complement at the column's scale; zero for a string key */
    int32_t str_len;       /* string key: UTF-8 bytes at h_bytes[v * str_stride + str_off[k]]; else 0 */
    int32_t reserved;
} cbx_key_value;
typedef struct cbx_key_set cbx_key_set;
typedef struct cbx_keyset_info {
    int64_t n_values;      /* tuples given */
    int64_t n_distinct;    /* members (duplicates are one) */
    int64_t capacity;      /* slots of the table */
    int64_t device_bytes;  /* device memory the set holds until it is destroyed */
    int64_t max_probe;     /* the longest probe sequence of the build, in slots visited */
    float build_ms;        /* the build launch, from HIP events while cbx_plan_set_profiling is on (else 0) */
    int32_t n_keys;
} cbx_keyset_info;

/* Build a set over `keys` from host arrays: h_values[n_values][n_keys], and for string keys h_bytes[n_values]
 * [str_stride] with key k's bytes at str_off[k], the layout cbx_group_layout reports for key_bytes (3 bytes per
 * source byte of each string key; h_bytes and str_off may be NULL when no key is a string).  Uploads them and
 * builds the table on `stream` (one lane per value: hash, probe, one device-scope 64-bit compare-and-swap per
 * claim; an occupied slot with an equal fingerprint is compared against the occupant's tuple in the uploaded
 * array), then waits for the stream, so the set may be probed from any stream afterwards.
 * CBX_E_UNSUPPORTED (reason in cbx_last_error): a key field the grouped aggregate refuses.  CBX_E_ARGUMENT: a
 * malformed key table, repeated or out-of-range fields, n_values < 0, a str_len below 0 or above 3 x the field
 * size, strides other than the group layout's, device memory above CBX_GROUP_MAX_WORKSPACE_BYTES. */
int cbx_key_set_create(cbx_plan* plan, const cbx_group_by* keys, const cbx_key_value* h_values, const uint8_t* h_bytes,
                       int32_t str_stride, const int32_t* str_off, int64_t n_values, void* stream, cbx_key_set** out);

/* What the build of the set found (host code only, no GPU work). */
int cbx_key_set_info(const cbx_key_set* set, cbx_keyset_info* out);

/* Frees the set's device memory; no call that probes it may still be running.  NULL is allowed. */
void cbx_key_set_destroy(cbx_key_set* set);

/* As cbx_filter_records (sources, `out`, *n_selected, the three passes and one host wait), with `filter` allowed
 * to be NULL and 1 to CBX_GROUP_MAX_KEYS key sets: sets[s] is probed as IN when negate[s] == 0 and as NOT IN
 * otherwise (negate == NULL: all IN).  The test pass evaluates the cbx_filter first and probes the sets for the
 * lanes still kept: fingerprint before key, numerics as (hi, lo), strings streamed through the code page against
 * the stored bytes.  n_rec == 0 launches nothing.  cbx_filter_pass_times reports this call's passes too.
 * CBX_E_ARGUMENT: n_sets outside 1..4, a NULL set, a set built on another plan, a negated set of more than one
 * column, and the argument errors of cbx_filter_records. */
int cbx_filter_records_keyed(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, const cbx_selection* in,
                             const int64_t* d_rec_off, const int32_t* d_rec_len, int64_t n_rec, int32_t rec_stride,
                             int32_t start_offset, int64_t first_record_id, const cbx_filter* filter,
                             const cbx_key_set* const* sets, const int32_t* negate, int32_t n_sets,
                             cbx_selection* out, int64_t* n_selected, void* stream);

/* ---- key sets built from the records of a second file: an additive extension of ABI 25 ----
 *
 * The semi join of a fact file against the keys of a dimension file without a trip of the keys through the host:
 * the set of `probe_plan` over `probe_keys` is built on the device from the `source_keys` of the records of a
 * second file, read through `source_plan` (its own copybook, code page, trimming policy and row filter).  No
 * structure and no entry point above changes, so CBX_ABI_VERSION stays 25; a caller checks for the symbol.
 * Over decoded values: take the source rows `source_filter` keeps (NULL: all; the record sources are those of
 * cbx_aggregate_grouped -- a selection, framed records or fixed-length records, exactly one); decode the
 * source_keys tuple of each as the grouped aggregate does; skip tuples with a NULL component (n_null_rows counts
 * those rows); take the distinct tuples that remain (n_source_keys); keep the ones the probe_keys columns can hold
 * (the others are counted in n_dropped: a decimal probe column holds |v| < 10^precision, an integer one the signed
 * 32- / 64-bit range, a string one at most 3 x its size in UTF-8 bytes and at most its size in characters).  The
 * set is what cbx_key_set_create(probe_plan, probe_keys, <those tuples>) builds: it belongs to probe_plan, and
 * cbx_key_set_info, cbx_key_set_destroy and cbx_filter_records_keyed treat it like any other set (its
 * capacity is the one of n_values tuples; only device_bytes may be larger, the block being laid out for
 * n_source_keys tuples before the drops are known).  cbx_keyset_info.n_values is n_source_keys - n_dropped; the order of the
 * values in the device array is unspecified.  Members, n_distinct and the four counts depend neither on
 * max_workgroups (a bound on the distinct pass's grid; 0: the library's choice) nor on timing.
 * Columns, checked before anything is launched: both key tables have the same n_keys; each pair is string / string
 * or numeric / numeric (else CBX_E_ARGUMENT); a numeric pair has one output scale, an integral column counting as
 * scale 0 -- precision, width, encoding and output type may differ, since the canonical key is the signed 128-bit
 * value at the column's scale (different scales: CBX_E_UNSUPPORTED, "key k: scales 2 and 3 differ"; nothing is
 * rescaled on the device).  Each side is otherwise refused as the grouped aggregate refuses a key, the reason
 * prefixed with "probe: " or "source: ".  A string key is the UTF-8 bytes of the trimmed source field through the
 * SOURCE plan's code page and trimming policy, compared as bytes with what the probe plan makes of its own field.
 * max_values >= 1 bounds the distinct source keys: with more, the call returns CBX_E_CAPACITY, sets
 * info->overflow, leaves *out NULL and holds no device memory (a partial set would silently drop rows of the
 * join).  The distinct table (cbx_keyset_from.h) has source_capacity = the power of two >= 2 * max_values slots of
 * 8 bytes, taken from the stream's memory pool and returned before the call ends; CBX_E_ARGUMENT when it or the
 * set's block for max_values values would exceed CBX_GROUP_MAX_WORKSPACE_BYTES.  n_rec == 0 launches no pass over
 * records and gives an empty set.
 * Passes: distinct (one pass over the source records: filter, key hash, find or claim a slot of bare 64-bit words),
 * convert (one lane per slot: the representative's key, the probe columns' limits, a dense index into the new set's
 * value array), then cbx_key_set_create's build over that array.  Host waits: three -- after the distinct pass (it
 * sizes the set's block), after the convert pass (the number of values the build takes), and the build's own. */
typedef struct cbx_keyset_source_info {
    int64_t n_rows;        /* source records the source filter kept */
    int64_t n_null_rows;   /* of those, records with a null key component (never members) */
    int64_t n_source_keys; /* distinct non-null source key tuples */
    int64_t n_dropped;     /* of those, tuples the probe columns can never hold (not members) */
    int64_t source_capacity, workspace_bytes;  /* the distinct table: slots, bytes from the stream's pool */
    int32_t overflow;      /* more than max_values distinct source keys: no set was built */
    int32_t reserved;
    float distinct_ms, convert_ms;   /* HIP events while cbx_plan_set_profiling(source_plan) is on, else 0 */
} cbx_keyset_source_info;

int cbx_key_set_create_from_records(cbx_plan* probe_plan, const cbx_group_by* probe_keys, cbx_plan* source_plan,
                                    const cbx_group_by* source_keys, const uint8_t* d_data, int64_t n_bytes,
                                    const cbx_selection* in, const int64_t* d_rec_off, const int32_t* d_rec_len,
                                    int64_t n_rec, int32_t rec_stride, int32_t start_offset,
                                    const cbx_filter* source_filter, int64_t max_values, int32_t max_workgroups,
                                    void* stream, cbx_key_set** out, cbx_keyset_source_info* info /* may be NULL */);

/* ---- lookup joins: key maps and the join stage: an additive extension of ABI 25 ----
 *
 * The question after the semi join: "and give me the dimension's columns beside each fact row".  A key map is a key
 * set whose members remember the dimension row they came from; the join stage is the keyed filter stage that also
 * emits, per kept fact row, the matching dimension row; cbx_select_ordinals turns those rows into a selection of the
 * dimension file that cbx_decode_selected takes.  No structure and no entry point above changes, so CBX_ABI_VERSION
 * stays 25; a caller checks for the six symbols below.
 * Key map, over decoded values.  Let S be the set cbx_key_set_create_from_records builds from the same arguments: the
 * accepted record sources, the pairing rules of the key columns, the scale rule, the drop rules, max_values, the
 * overflow behaviour, the refusals and their messages are that call's, unchanged.  Number the records of the source's
 * record source 0 .. n_rec - 1 (the position in the source handed to the call, not the position among the kept rows).
 * For every member v of S, first_row[v] is the smallest ordinal among the source rows source_filter keeps whose key
 * equals v, and n_rows[v] is the number of such rows.  n_duplicate_keys is the number of members with n_rows > 1,
 * max_rows_per_key the largest n_rows (0 for an empty map).  None of this depends on timing, on max_workgroups or on
 * which lane claimed a slot: first_row is a minimum, not the distinct pass's representative.
 * Passes: those of cbx_key_set_create_from_records, then fill (one more pass over the source records: the source
 * filter, then every kept record probes the finished set through the SOURCE plan's key program and, on a hit, does
 * one 64-bit atomic min on first_row and one 64-bit atomic add on n_rows, relaxed, device scope) and stats (one lane
 * per value).  Host waits: four -- the set's three and one after the stats pass for the two numbers.  An empty set
 * launches neither pass and does not wait again.  The map holds the set's device memory and 16 bytes per value.
 * Join.  K(r): the cbx_filter is true for r and every set's verdict is true for r, exactly as cbx_filter_records_keyed
 * decides it (here n_sets may be 0 and filter NULL: then K is true).  m(r): first_row of the member equal to r's key
 * over the map's probe columns, -1 when a key component is null or the key is no member.  CBX_JOIN_INNER keeps r when
 * K(r) and m(r) >= 0; CBX_JOIN_LEFT keeps r when K(r).  `out` is the selection of the kept rows in source order --
 * for INNER bit-identical to cbx_filter_records_keyed with the map's set added as one more IN set --, *n_selected
 * their number, d_match[j] (device, capacity n_rec) m of the j-th kept row, d_match_rows[j] (device, capacity n_rec;
 * may be NULL) n_rows of that member, 0 where m = -1.
 * THIS IS A LOOKUP JOIN: it equals SQL's inner / left join exactly when n_duplicate_keys == 0.  With duplicate
 * dimension keys it returns the first matching dimension row, and d_match_rows says how many there were.
 * Passes: test (the keyed test pass, then the map probe for lanes still kept: one value-index lookup, one 8-byte
 * load and one 8-byte store per kept row into a per-input-record array from the stream's pool), the filter stage's
 * scan, emit (filter_emit_kernel unchanged, then the compaction of the match arrays with the same keep words).
 * Host waits: one, as cbx_filter_records.  n_rec == 0 launches nothing. */
#define CBX_JOIN_INNER 0
#define CBX_JOIN_LEFT 1
typedef struct cbx_key_map cbx_key_map;
typedef struct cbx_keymap_info {
    int64_t n_rows;        /* as cbx_keyset_source_info, field by field ... */
    int64_t n_null_rows;
    int64_t n_source_keys;
    int64_t n_dropped;
    int64_t source_capacity, workspace_bytes;
    int32_t overflow;
    int32_t reserved;
    float distinct_ms, convert_ms;
    int64_t n_duplicate_keys;   /* ... then: members with more than one source row */
    int64_t max_rows_per_key;   /* the largest number of source rows of one member */
    float fill_ms;              /* init + fill + stats, HIP events while cbx_plan_set_profiling(source_plan) is on */
    int32_t reserved2;
} cbx_keymap_info;

/* The arguments of cbx_key_set_create_from_records.  On any error *out is NULL and no device memory is held. */
int cbx_key_map_create_from_records(cbx_plan* probe_plan, const cbx_group_by* probe_keys, cbx_plan* source_plan,
                                    const cbx_group_by* source_keys, const uint8_t* d_data, int64_t n_bytes,
                                    const cbx_selection* in, const int64_t* d_rec_off, const int32_t* d_rec_len,
                                    int64_t n_rec, int32_t rec_stride, int32_t start_offset,
                                    const cbx_filter* source_filter, int64_t max_values, int32_t max_workgroups,
                                    void* stream, cbx_key_map** out, cbx_keymap_info* info /* may be NULL */);

/* What the build of the map found (host code only, no GPU work). */
int cbx_key_map_info(const cbx_key_map* map, cbx_keymap_info* out);

/* Frees the map, its set included; no call that probes either may still be running.  NULL is allowed. */
void cbx_key_map_destroy(cbx_key_map* map);

/* The member set S: owned by the map and valid until cbx_key_map_destroy.  It is a set of probe_plan like any other
 * (cbx_key_set_info, cbx_filter_records_keyed), but it MUST NOT be passed to cbx_key_set_destroy.  NULL for NULL. */
const cbx_key_set* cbx_key_map_set(const cbx_key_map* map);

/* As cbx_filter_records_keyed with 0 to CBX_GROUP_MAX_KEYS sets (sets / negate may be NULL when n_sets == 0), one
 * key map of `plan` and a join type.  CBX_E_ARGUMENT: a NULL map, a map built for another probe plan, a join_type
 * other than the two, a NULL d_match, and whatever cbx_filter_records_keyed refuses. */
int cbx_join_records(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, const cbx_selection* in,
                     const int64_t* d_rec_off, const int32_t* d_rec_len, int64_t n_rec, int32_t rec_stride,
                     int32_t start_offset, int64_t first_record_id, const cbx_filter* filter,
                     const cbx_key_set* const* sets, const int32_t* negate, int32_t n_sets, const cbx_key_map* map,
                     int32_t join_type, cbx_selection* out, int64_t* n_selected, int64_t* d_match,
                     int64_t* d_match_rows /* may be NULL */, void* stream);

/* Rows of a record source by ordinal (independent of maps): row j of `out` (capacity n) is exactly the row
 * filter_emit_kernel writes for record d_ordinals[j] (device, n values) of the record source, which is given as to
 * cbx_filter_records.  With an `in` selection its rec_off, rec_len, record_id, segment and seg_state are carried
 * over; otherwise the row has the framed or fixed-length offset and length, first_record_id + ordinal, and the
 * segment from the plan's segment map or -1.  Ordinals may repeat and come in any order.  An ordinal outside
 * [0, n_rec) gives a zero-length record at offset 0 (record id -1, segment -1): the host cannot check this without a
 * wait, so the call does not.  One launch, no host wait: `out` is complete when `stream` reaches this point. */
int cbx_select_ordinals(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, const cbx_selection* in,
                        const int64_t* d_rec_off, const int32_t* d_rec_len, int64_t n_rec, int32_t rec_stride,
                        int32_t start_offset, int64_t first_record_id, const int64_t* d_ordinals, int64_t n,
                        cbx_selection* out, void* stream);

/* Durations in ms of the plan's last cbx_join_records call: test, scan, emit (both emit launches), measured with HIP
 * events while cbx_plan_set_profiling is on. */
int cbx_join_pass_times(cbx_plan* plan, float* test_ms, float* scan_ms, float* emit_ms);

/* ---- fan-out joins: one output row per match (an additive extension of ABI 25; cbx_keymap_rows.h) ----
 *
 * Row lists.  cbx_key_map_index_rows gives an existing map, for every member v, rows[row_start[v] .. row_start[v+1]):
 * the ordinals of ALL source rows source_filter keeps whose key is v, ASCENDING, numbered as first_row is.  So
 * rows[row_start[v]] == first_row[v], row_start[v+1] - row_start[v] == n_rows[v] and row_start[n_values] is the sum
 * of n_rows.  Nothing depends on the grid, on max_workgroups or on timing.  The map does not keep its source: the
 * caller presents it again -- source_plan, source_keys, the record source and source_filter exactly as
 * cbx_key_map_create_from_records took them.  source_plan and n_rec must be the map's (CBX_E_ARGUMENT, no launch);
 * a source that differs otherwise never writes outside a member's segment and is found by the check pass:
 * CBX_E_STATE "source differs from the one the map was built from", the lists are freed and the map stays a valid
 * lookup map.  A second call on a map with lists is CBX_OK and launches nothing; so is a call on an empty map.
 * Passes: a 64-bit exclusive scan of n_rows; scatter (the fill pass's geometry and probe, one 64-bit atomic add on a
 * per-member cursor per hit); sort -- segments of up to short_max ordinals by one lane each, up to lds_max by one
 * workgroup through LDS, longer ones by one workgroup in global memory (slow, never refused); check (one lane per
 * value).  Host waits: one.  Memory: 8 bytes per kept source row plus 8 per value, owned by the map, freed by
 * cbx_key_map_destroy; 24 bytes per value from the stream's pool during the call.
 *
 * Expand.  cbx_join_records_expand takes cbx_join_records' arguments; K(r) and the member j(r) are as there, L(r) is
 * that member's row list (empty when j(r) = -1).  INNER: c(r) = |L(r)| when K(r), else 0.  LEFT: c(r) = max(|L(r)|, 1)
 * when K(r), else 0.  T = sum of c(r), in 64 bits.  The outputs of r occupy [B(r), B(r) + c(r)), B the exclusive
 * prefix of c in source order; output row B(r) + q has the selection row filter_emit_kernel writes for r (`out`),
 * d_match = L(r)[q] or -1 for the single row of an unmatched LEFT row, and d_fact_row (may be NULL) = r's ordinal in
 * the input.  *n_out = T, *n_kept = the number of r with c(r) > 0.  On a map with n_duplicate_keys == 0, `out`,
 * *n_out and d_match are bit-identical to cbx_join_records' out, *n_selected and d_match.  WITH ROW LISTS THIS IS
 * SQL'S INNER / LEFT JOIN.  T > out_capacity: CBX_E_CAPACITY with *n_out = T and *n_kept set, both numbers in the
 * message, and NO output array written (the emit is not launched).  out == NULL with out_capacity == 0 is the
 * count-only form (the join's COUNT(*)): the two numbers, CBX_OK, d_match / d_fact_row unused.  A map without row
 * lists: CBX_E_STATE.  Every other refusal is cbx_join_records' own, message for message.  n_rec == 0 launches
 * nothing.
 * Passes: test (keymap_test_kernel, unchanged: per input record the start and length of its member's list); scan
 * (the uint32 scan of the tile counts, the compaction to kept rows, a 64-bit scan over the kept rows whose grid is
 * sized from n_rec and which reads the kept count on the device); emit (lane = output row: a wave finds the kept row
 * of its first output by one binary search and each lane its own within the next 64 kept rows in 6 cross-lane
 * steps, so a wave's work is bounded by its 64 outputs).  Host waits: one, for T and n_kept together (a second one
 * after the emit only while profiling is on, to read its duration). */
typedef struct cbx_keymap_rows_info {
    int64_t n_indexed_rows;     /* row_start[n_values] */
    int64_t n_short, n_lds, n_global;   /* members each sort path took */
    int32_t has_rows;
    int32_t short_max, lds_max; /* the two boundaries: longest segment of the lane path / of the LDS path */
    float index_ms;             /* all passes, HIP events while cbx_plan_set_profiling(source_plan) is on */
} cbx_keymap_rows_info;

typedef struct cbx_expand_info {
    int64_t n_kept, n_out;
    int64_t max_fanout;         /* the largest c(r) */
    int64_t emit_grid;          /* workgroups of the emit pass (0: not launched) */
    int32_t outputs_per_workgroup;
    int32_t host_waits;
} cbx_expand_info;

int cbx_key_map_index_rows(cbx_key_map* map, cbx_plan* source_plan, const cbx_group_by* source_keys, const uint8_t* d_data,
                           int64_t n_bytes, const cbx_selection* in, const int64_t* d_rec_off, const int32_t* d_rec_len,
                           int64_t n_rec, int32_t rec_stride, int32_t start_offset, const cbx_filter* source_filter,
                           int32_t max_workgroups, void* stream, cbx_keymap_rows_info* info /* may be NULL */);

/* Host code only, no GPU work. */
int cbx_key_map_rows_info(const cbx_key_map* map, cbx_keymap_rows_info* out);

/* The lists as device pointers (row_start: n_values + 1 entries), valid until cbx_key_map_destroy; NULLs before the
 * lists exist and for an empty map. */
int cbx_key_map_rows(const cbx_key_map* map, const int64_t** d_row_start, const int64_t** d_rows);

int cbx_join_records_expand(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, const cbx_selection* in,
                            const int64_t* d_rec_off, const int32_t* d_rec_len, int64_t n_rec, int32_t rec_stride,
                            int32_t start_offset, int64_t first_record_id, const cbx_filter* filter,
                            const cbx_key_set* const* sets, const int32_t* negate, int32_t n_sets, const cbx_key_map* map,
                            int32_t join_type, cbx_selection* out, int64_t out_capacity, int64_t* n_out, int64_t* n_kept,
                            int64_t* d_match, int64_t* d_fact_row /* may be NULL */, void* stream);

/* How the plan's last cbx_join_records_expand call ran (host code only). */
int cbx_join_expand_info(cbx_plan* plan, cbx_expand_info* out);

/* Durations in ms of the plan's last cbx_join_records_expand call: test, scan (both scans and the compaction), emit,
 * measured with HIP events while cbx_plan_set_profiling is on. */
int cbx_join_expand_pass_times(cbx_plan* plan, float* test_ms, float* scan_ms, float* emit_ms);

/* ---- the record walk with data-dependent offsets ----
 *
 * Layouts the static-offset tables above cannot express run through a per-record walk of the
 * copybook (RecordExtractors.extractRecord restated per lane, cbx_walk.h): variable_size_occurs =
 * true (an OCCURS DEPENDING ON array consumes only its present elements, RecordExtractors.scala:
 * 109-113), DEPENDING ON a field inside an OCCURS, DEPENDING ON a string field through
 * occurs_mappings (dependingOnHandlers).  cbx_plan_set_walk attaches the copybook's node table to a
 * plan; every later decode call on the plan walks.  Output columns are as above, with two
 * differences: a count column of an array nested in OCCURS has one slot per enclosing element
 * (n_slots = product of the enclosing max counts), and string columns must use the string-view
 * layout.  Requires zeroed validity buffers. */
#define CBX_W_GROUP 0
#define CBX_W_PRIM 1
#define CBX_W_REDEFINED 0x1   /* isRedefined: the node does not advance the offset */
#define CBX_W_REDEFINES 0x2   /* redefines another node: a group advances by its static size */
typedef struct {
    int32_t kind;          /* CBX_W_GROUP / CBX_W_PRIM */
    int32_t next, child;   /* next sibling, first child (groups); -1 none */
    int32_t field;         /* primitive: cbx_field index, -1 when not decoded (FILLER) */
    int32_t array;         /* OCCURS node: cbx_array index, -1 */
    int32_t flags;         /* CBX_W_* */
    int32_t data_size;     /* bytes per element (binaryProperties.dataSize) */
    int32_t actual_size;   /* bytes of the whole node (binaryProperties.actualSize) */
    int32_t segment;       /* group: segment redefine index, -1 */
    int32_t dep_slot;      /* DEPENDING ON source: its dependee slot (one per name, < 8), -1 */
} cbx_walk_node;
typedef struct {
    int32_t dep_slot;      /* dependee slot of the array's DEPENDING ON name, -1: fixed OCCURS */
    int32_t h_begin, h_end;/* its occurs_mappings handlers (cbx_walk_handler range) */
    int32_t reserved;
} cbx_walk_array;
typedef struct {
    int32_t key_id;        /* distinct key strings share an id */
    int32_t key_len;       /* UTF-8 bytes */
    int32_t value;         /* element count the key stands for */
    int32_t reserved;
    uint8_t key[64];
} cbx_walk_handler;

int cbx_plan_set_walk(cbx_plan* plan, const cbx_walk_node* nodes, int32_t n_nodes, int32_t root,
                      const cbx_walk_array* arrays, const cbx_walk_handler* handlers, int32_t n_handlers,
                      int32_t variable_size_occurs);

/* VarOccursRecordExtractor (CP/reader/extractors/raw/VarOccursRecordExtractor.scala:30-154): record
 * boundaries of a file whose record size follows from its OCCURS DEPENDING ON values (no RDW, no
 * length field), from first_offset on.  A record starts where the previous one ends; the stream is
 * framed chunk-parallel (speculated chunk entries corrected until they agree with the sequential walk,
 * cbx_chain.h), with the sequential walk's results.  A short read at the end is zero-filled by
 * the reference: the last record may reach past n_bytes, up to *virtual_bytes (the buffer must hold
 * zeros there before decoding).  Needs a plan with cbx_plan_set_walk.  From jit_min_records records
 * (estimated at the copybook's largest record) the step is the copybook-specialised walk_length
 * (hipRTC; cbx_plan_frame_kind).  Device scratch, stream-ordered (hipMallocAsync, freed by the call):
 * a bitmap of one bit per byte of [first_offset, n_bytes) -- n_bytes / 8, 125 MB per GB framed --
 * plus ~60 bytes per chunk of >= 16 KiB; cbx_frame_length_field takes the same (chunks >= 1 KiB). */
int cbx_frame_var_occurs(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, int64_t first_offset,
                         int64_t* d_rec_off, int32_t* d_rec_len, int64_t capacity, int64_t* n_records,
                         int64_t* virtual_bytes, void* stream);

/* Record length field framing (record_length_field, not is_record_sequence):
 * VRLRecordReader.fetchRecordUsingRecordLengthField (CP/reader/iterator/VRLRecordReader.scala:114-149).
 * From byte 0, each record is start_offset + lfb bytes (lfb = the field's offset + size; `field` indexes
 * the plan's cbx_field table) plus max(0, value + adjustment - lfb + end_offset) more, fewer at the end
 * of the data, which ends the walk; a stream holding fewer than start_offset + lfb bytes has no further
 * record.  The field must be a primitive Integral one (ReaderParametersValidator.getLengthField); its
 * value is decoded as extractPrimitiveField does (Int / Long -> toInt) and a null or BigDecimal value
 * fails with CBX_E_STATE (the reference's IllegalStateException).  rec_off / rec_len receive
 * the record starts and lengths (decode them with cbx_decode_var at start_offset).  Framed
 * chunk-parallel like cbx_frame_var_occurs (cbx_chain.h); the error reported is the first one on the
 * record chain. */
int cbx_frame_length_field(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, int32_t field,
                           int32_t start_offset, int32_t end_offset, int32_t adjustment, int64_t* d_rec_off,
                           int32_t* d_rec_len, int64_t capacity, int64_t* n_records, void* stream);

/* ---- hierarchical records (`segment-children`) ----
 *
 * Replaces VarLenHierarchicalIterator + the structure walk of RecordExtractors.extractHierarchicalRecord
 * (CP/reader/iterator/VarLenHierarchicalIterator.scala:43-162, RecordExtractors.scala:211-385): the
 * framed records of a stream are grouped by root segment (records before the first root dropped) and
 * each record is placed under its parent instance (extractChildren's rule, :298-322: the children of
 * type C of a parent p are the C records after p up to the first record of p's segment or of one of
 * its ancestors).  With one segment id per segment that has children the reference's rule depends on
 * types only (parallel passes over the records); else flags bit 0 selects the general walk.  At most
 * 16 segments.
 *
 * Output: one cbx_selection of rows in table order -- table 0 = the root records (one row per
 * hierarchical record, Record_Id = first_record_id + the index of the next root record or n_rec,
 * VarLenHierarchicalIterator.scala:107-133), then table 1 + s = the records of segment s placed in
 * the tree, each table in record order (Record_Id = first_record_id + record index, unused by the
 * reference).  parent_row[row] = the row of the record's parent instance (-1 for roots).  Decode
 * the rows with cbx_decode_selected (segment = the record's own segment: its redefine decodes); the
 * list of segment-C children of every parent row is a contiguous run of table 1 + C
 * (cbx_hier_list_offsets).  table_rows (host, n_segments + 1 entries) receives the row count per
 * table.  Output arrays need capacity n_rec.
 * record_start_offset: extractHierarchicalRecord decodes the root at the start offset but each child
 * segment at its group's own offset, without it (RecordExtractors.scala:308-310, :376) -- the host
 * decodes the child rows as records starting start_offset bytes earlier.  The dependFields map the
 * reference shares between the segments of a hierarchical record (:224-245: a child's array DEPENDING
 * ON a field of its parent segment or of the common header, or on a null field of its own segment)
 * is resolved on the device by cbx_hier_dependee_counts and applied with cbx_plan_set_odo_counts.
 * Several segment ids mapped to one segment that has children: flags bit 0 (the general walk: one
 * thread per hierarchical record runs extractChildren's recursion with its id-based break rule).
 * The counts are resolved BEFORE the decode (one decode): cbx_hier_dependee_values decodes each
 * DEPENDING ON field from every row's bytes, cbx_hier_dependee_counts replays the walk.
 * Record-walk plans (string dependees through occurs_mappings, variable_size_occurs) take the map per
 * row instead of counts (cbx_hier_walk.seeds -> cbx_plan_set_dep_seed).
 * Not covered (reported by the host, CBX_E_UNSUPPORTED, never decoded differently): a segment group
 * placed before the root segment's that has child segments, with a cross-segment DEPENDING ON (the
 * root's record walk extracts that group's children too); on a record-walk plan, a cross-segment
 * DEPENDING ON field inside an OCCURS or behind a variable-size one. */
typedef struct {
    int32_t n_segments;               /* segment redefines (cbx_field.segment / key_segment indices) */
    int32_t root_segment;             /* the segment without a parent */
    int32_t parent[CBX_MAX_SEG_KEYS]; /* parent segment of each segment, -1 for the root */
    int64_t first_record_id;          /* startRecordId of the stream (entry.record_index) */
    int32_t start_offset;             /* record_start_offset: the segment id is read past it (VRLRecordReader) */
    int32_t flags;                    /* bit 0: the general walk -- a segment with children mapped from several
                                       * segment ids (one record can then sit under several parents: rows may
                                       * outnumber n_rec; CBX_E_CAPACITY with *n_rows / table_rows set when they
                                       * do not fit, call again with that capacity) */
    int64_t row_capacity;             /* rows the outputs hold (0: n_rec) */
} cbx_hier_params;

int cbx_hier_select(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, const int64_t* d_rec_off,
                    const int32_t* d_rec_len, int64_t n_rec, const cbx_hier_params* params, cbx_selection* out,
                    int64_t* d_parent_row, int64_t* table_rows, int64_t* n_rows, void* stream);

/* Arrow list offsets (int32, n_parent + 1 entries) of one child table over its parent table:
 * offsets[k] = rows of the child table [child_begin, child_begin + n_child) whose parent row is
 * below parent_begin + k.  Asynchronous on `stream`. */
int cbx_hier_list_offsets(const int64_t* d_parent_row, int64_t child_begin, int64_t n_child, int64_t parent_begin,
                          int64_t n_parent, int32_t* d_offsets, void* stream);

/* A DEPENDING ON field (plan field `field`: integral COMP-3 / binary / DISPLAY) decoded from each of
 * n_rows rows' own bytes -- at rec_off + start_offset + its offset, null past rec_len or when malformed,
 * whatever the row's segment (the root record decodes every segment group from its own bytes,
 * RecordExtractors.scala:365-372) -- into d_values (int64 Number.intValue) and d_validity (one bit per
 * row, a word per 64 rows).  The dependee columns of cbx_hier_dependee_counts (out_type CBX_O_I64),
 * so the counts exist before the rows are decoded.  Asynchronous on `stream`. */
int cbx_hier_dependee_values(cbx_plan* plan, const uint8_t* d_data, int64_t n_bytes, const int64_t* d_rec_off,
                             const int32_t* d_rec_len, int64_t n_rows, int32_t start_offset, int32_t field,
                             int64_t* d_values, uint64_t* d_validity, void* stream);

/* The dependFields map extractHierarchicalRecord shares between the segments of one hierarchical
 * record (RecordExtractors.scala:224-245, walk order :324-370), on the device: one thread per
 * hierarchical record walks its rows as the reference does -- the root, then per child segment in
 * copybook order (getParentToChildrenMap, CopybookParser.scala:702-727) each child row followed by
 * its own subtree -- replaying at every row its segment's events in field order: a numeric DEPENDING
 * ON field registers its value (Number.intValue) when the row decodes it non-null; an array takes the
 * value registered last (its maximum when none is, or the value is outside [min, max]).
 * counts (device, [n_arrays_out][pitch] int32) receives the count of every array event's rows, root
 * rows included, and *d_changed (device int32) is set to 1 when some count differs from first_counts
 * (when given); apply with cbx_plan_set_odo_counts to the decode.  Rows as cbx_hier_select emits them.
 * Root-record registrations that precede the root segment's group (the common header, a segment group
 * placed before it, decoded from the root's bytes) are events[CBX_HIER_MAX_SEG]. */
#define CBX_HIER_MAX_SEG 16       /* segments of a hierarchical layout (cbx_hier_select's limit) */
#define CBX_HIER_MAX_EVENTS 32    /* events per segment */
#define CBX_HIER_MAX_DEPS 16      /* dependees and arrays of one cbx_hier_dependee_counts call */
typedef struct {
    const void* values;               /* device: the dependee column's values, slot 0 (row-indexed) */
    const uint64_t* validity;         /* device: its validity words, slot 0 */
    int32_t out_type;                 /* CBX_O_I32 / CBX_O_I64 / CBX_O_DEC128; CBX_O_STRING: int64 values are the
                                       * occurs_mappings key id + 1 of a string dependee (cbx_hier_dependee_values) */
    int32_t walk_slot;                /* its dependee slot in the plan's record walk (seeds), -1 none */
} cbx_hier_dependee;

typedef struct {
    int32_t dependee;                 /* index into the dependee table */
    int32_t out_row;                  /* row of `counts` receiving this array's counts (the plan array index) */
    int32_t min_count, max_count;
    const int32_t* first_counts;      /* device: the first decode's counts of the array (row-indexed), may be NULL */
} cbx_hier_odo_array;

typedef struct {
    int32_t n_segments;
    int32_t root_segment;
    int64_t table_base[CBX_HIER_MAX_SEG + 1];        /* first row of table t (0: roots, 1 + s: segment s) */
    int64_t table_rows[CBX_HIER_MAX_SEG + 1];
    const int32_t* child_offsets[CBX_HIER_MAX_SEG];  /* device: segment s's list offsets over its parent table */
    int8_t children[CBX_HIER_MAX_SEG][CBX_HIER_MAX_SEG]; /* child segments of s in copybook order, -1 ends */
    /* events of a row of segment s in field order (s = CBX_HIER_MAX_SEG: the root record's common-header
     * registrations before the root segment's group): e >= 0 registers dependee e, e < 0 resolves
     * array -e - 1; -32768 ends */
    int16_t events[CBX_HIER_MAX_SEG + 1][CBX_HIER_MAX_EVENTS];
    /* device, or NULL: [8][pitch] int64, each row's record-walk dependee slots as the walk leaves the map
     * before the row (after the root's registrations that precede the root segment's group, for a root
     * row): kind << 32 | value, kind 0 unseen, 1 Left(int), 2 Right(key id + 1) -- cbx_plan_set_dep_seed */
    int64_t* seeds;
} cbx_hier_walk;

/* Record-walk plans (cbx_plan_set_walk: variable_size_occurs, string dependees through occurs_mappings,
 * DEPENDING ON inside an OCCURS): the walk resolves a row's counts itself from its dependFields map; for
 * hierarchical rows that map starts as the walk of the hierarchical record left it (cbx_hier_walk.seeds),
 * and a child row registers no common-header dependee (it decodes its own segment group only,
 * RecordExtractors.scala:300-322).  d_seed = NULL clears it.  Asynchronous use by later decode calls. */
int cbx_plan_set_dep_seed(cbx_plan* plan, const int64_t* d_seed, int64_t pitch, int32_t root_segment);

int cbx_hier_dependee_counts(const cbx_hier_walk* walk, const cbx_hier_dependee* deps, int32_t n_deps,
                             const cbx_hier_odo_array* arrays, int32_t n_arrays, int32_t* d_counts, int64_t pitch,
                             int32_t* d_changed, void* stream);

/* One string slot in the string-view layout (Utf8View: 16-byte views, long payloads in data buffers of
 * buffer_bytes each starting at region, cbx_string_view_geometry) -> Arrow Utf8 (int32 offsets
 * [n + 1] + the payload written contiguously into data, data_capacity bytes).  The record walk
 * (cbx_plan_set_walk: data-dependent offsets, one pass) writes views; this converts its columns for a
 * consumer of the Utf8 layout the reference's StringType maps to (SC/schema/CobolSchema.scala:
 * StringType).  Validity is unchanged (null values are empty).  *d_size (device int64) receives the
 * payload bytes; CBX_E_CAPACITY when they exceed data_capacity or an int32 offset (Arrow's limit). */
int cbx_views_to_utf8(const uint8_t* d_views, int64_t n, const uint8_t* d_region, int64_t buffer_bytes,
                      int32_t* d_offsets, uint8_t* d_data, int64_t data_capacity, int64_t* d_size, void* stream);

/* Text record framing (is_text = true) on the GPU: replaces TextRecordExtractor
 * (cobol-parser/.../reader/extractors/raw/TextRecordExtractor.scala:26-108, chosen by
 * VarLenNestedReader.scala:69-70).  Records end at LF or CR LF (payload without the line
 * ending) inside a window of record_size + 2 bytes (record_size = copybook.getRecordSize); a
 * window without one gives a forced record.  Writes payload offsets/lengths in file order.
 * *virtual_bytes receives the stream length the reference decodes against: its read helper
 * treats a short last read as a full window of zero bytes, so records may reach past n_bytes
 * (by at most record_size + 2); the buffer must hold zeros there before records are decoded
 * (pass *virtual_bytes as n_bytes to cbx_decode_var). */
int cbx_frame_text(const uint8_t* d_data, int64_t n_bytes, int32_t record_size, int64_t* d_rec_off,
                   int32_t* d_rec_len, int64_t capacity, int64_t* n_records, int64_t* virtual_bytes,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
