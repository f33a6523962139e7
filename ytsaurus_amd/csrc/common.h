/* Internal structures shared between the host evaluator and the HIP kernels.
 * Product code (libytql_gpu.so). Not part of the public C-ABI
 * (see /root/repo/include/ytql_gpu.h for the boundary).
 */
#pragma once
#include <stdint.h>

namespace ytql {

/* Resolved device-side segment descriptor. The kernel parses the sub-blob
 * offsets itself from the 8-byte bit-pack headers
 * (reference layout: bit_packed_unsigned_vector-inl.h:34-45 header word =
 * count(56b)|width(8b); segment assembly integer_column_writer.cpp:66-116,
 * 394-489). */
struct DevSeg {
    int32_t type;        /* YT_SEG_* */
    int32_t is_signed;   /* 1 = int64 (zigzag), 0 = uint64; 2 = string column */
    int64_t start_row;   /* first chunk row covered */
    int32_t row_count;
    int32_t col;         /* owning column index */
    uint64_t min_value;
    const uint64_t* blob;
    int64_t blob_bytes;
};

/* Parsed per-segment sub-blob map (built on device by k_parse_segments). */
struct SegEx {
    uint32_t w_values;
    uint32_t w_ids;
    uint32_t w_starts;
    uint32_t run_count;       /* RLE run count / dictionary id count */
    uint32_t dict_size;
    uint32_t flags;
    int64_t off_values_words; /* first data word of the values vector (past header) */
    int64_t off_bitmap_bytes; /* null bitmap (direct formats) */
    int64_t off_ids_words;    /* dictionary ids / RLE ids data words */
    int64_t off_starts_words; /* RLE run-start data words */
    int64_t off_doubles_bytes;
};

/* Postfix expression program; mirrors the oracle's eval_expr semantics
 * (cg_fragment_compiler.cpp arithmetic/relational/logical codegen). */
enum POp : int32_t {
    P_COL = 0, P_LIT_I64 = 1, P_LIT_NULL = 2, P_LIT_DOUBLE = 3,
    /* a YT_EX_LIT_I64 that faces a UINT64 operand (include/ytql_gpu.h,
     * expression typing): the same bits, typed UINT64. No YT_EX_* node. */
    P_LIT_U64 = 5,
    P_ADD = 10, P_SUB = 11, P_MUL = 12, P_DIV = 13, P_MOD = 14,
    P_EQ = 20, P_NE = 21, P_LT = 22, P_LE = 23, P_GT = 24, P_GE = 25,
    P_AND = 30, P_OR = 31, P_NOT = 32,
    /* one whole string-predicate leaf (a STRING column against a literal):
     * col = the column; bits = predicate index (low 8 bits) | kSpNullRes /
     * kSpNullIsNull = the answer for a null text | kSpConst / kSpConstRes =
     * the answer for every non-null text is a constant (comparison with the
     * null literal), no bitmap. Otherwise the answer for entry id is bit
     * sp_base[pred][seg]*64 + id-1 of sp_bits[pred] (k_strpred_entries). */
    P_STR_PRED = 50,
    /* a whole projection that is one STRING column of the primary chunk
     * (plain scans only): col = the column. Yields type YT_VT_STRING, or null,
     * and bits = (global DevSeg index << 32) | (entry id - 1): the entry that
     * dict_entry() resolves to the value's bytes (StrGatherRec.ref). */
    P_STR_REF = 51,
    /* numeric YT_EX_IN, postfix: pops the operand, pushes a non-null
     * boolean. bits = set index (low 8 bits) | kInNullRes = the list holds
     * null (the answer for a null operand). The set is DevPlan in_tab /
     * in_mask / in_empty (inlist.h inlist_probe_u64). */
    P_IN_NUM = 52,
};

constexpr uint64_t kSpNullRes = 1ULL << 8;
constexpr uint64_t kSpNullIsNull = 1ULL << 9;
constexpr uint64_t kSpConst = 1ULL << 10;
constexpr uint64_t kSpConstRes = 1ULL << 11;
constexpr uint64_t kInNullRes = 1ULL << 8;

struct PInst {
    int32_t op;
    int32_t col;
    uint64_t bits;     /* literal payload */
};

constexpr int kMaxProg = 48;
/* slots of eval_prog's value stack. A leaf needs 1, NOT and IN what their
 * operand needs, a binary node max(need(a), 1 + need(b)): compile_expr
 * refuses a program that needs more, so no thread indexes past the array. */
constexpr int kEvalStack = 12;
constexpr int kMaxCols = 8;
constexpr int kMaxAggs = 4;
constexpr int kMaxStrPreds = 4;    /* string predicates with a bitmap per filter */
constexpr int kMaxInSets = 4;      /* numeric IN lists per plan */

/* The scalar words of the chunk setup (k_parse_segments, k_scan_nullflags,
 * the kernels' error word) in one block: one H2D copy of a host image sets
 * them, one D2H copy brings them back. */
struct SetupWords {
    unsigned col_null[kMaxCols];          /* bit0 nulls seen, bit1 unknown */
    unsigned maxw;                        /* widest value vector */
    unsigned err[3];                      /* [0] kernel error, [1] join dups */
    unsigned long long zzmin[kMaxCols];   /* image: ~0 */
    unsigned long long zzmax[kMaxCols];   /* image: 0 */
};

/* One compiled plan for the device: programs are concatenated postfix
 * streams with (offset,len) per role. */
constexpr int kMaxProj = 8;

constexpr int kMaxPackKeys = 4;

struct DevPlan {
    int32_t ncols;
    uint8_t col_types[kMaxCols];       /* YT_VT_* */
    /* composite packed group key (key_count > 1): each component column's
     * zigzag-space value is biased by kp_base and offset by 1 (0 = null),
     * then packed at kp_shift. Total width <= 62 bits so the table's empty
     * (0x8000...) sentinel can never collide; key_bits == 0 (all-null key)
     * rides the existing side-accumulator path. A STRING component packs
     * its string id (StrKeyDev below). */
    int32_t kp_count;
    int32_t kp_col[kMaxPackKeys];
    int32_t kp_signed[kMaxPackKeys];
    int32_t kp_shift[kMaxPackKeys];
    int32_t kp_bits[kMaxPackKeys];
    uint64_t kp_base[kMaxPackKeys];
    /* log2(rows per segment) when the column's interior segments are all
     * exactly 1<<shift rows (the writer's 128Ki cap makes this the norm):
     * row→segment is then a shift instead of a binary search. 0 = ragged. */
    int32_t col_uniform_shift[kMaxCols];
    int32_t filter_off, filter_len;    /* -1 len 0 = none */
    int32_t key_off, key_len;          /* key_count==1 only; len 0 = global agg */
    int32_t agg_count;
    int32_t agg_func[kMaxAggs];        /* YT_AGG_* */
    int32_t agg_off[kMaxAggs], agg_len[kMaxAggs];
    int32_t proj_count;                /* scan-without-aggregation mode */
    int32_t proj_off[kMaxProj], proj_len[kMaxProj];
    PInst prog[kMaxProg];
    int32_t prog_len;
    /* string predicates (P_STR_PRED): per predicate the entry-answer bitmap
     * and, per kept segment of its column, the bitmap's first 64-bit word.
     * Device pointers, filled by the host after the segment parse. */
    int32_t sp_count;
    const uint64_t* sp_bits[kMaxStrPreds];
    const int64_t* sp_base[kMaxStrPreds];
    /* numeric IN sets (P_IN_NUM): open-addressing tables of the lists'
     * distinct values, device pointers filled by the host (inlist.h); the
     * program alone says how many are in use */
    const uint64_t* in_tab[kMaxInSets];
    uint64_t in_mask[kMaxInSets];
    uint64_t in_empty[kMaxInSets];
};

/* STRING components of the composite key (col_types[kp_col[i]] is
 * YT_VT_STRING): the code of a non-null value is 1 + its string id,
 * kmap[i][kbase[i][seg] + id in seg - 1] (k_strkey_*: one id per distinct
 * string of the column's kept segments); kp_base is 0 and kp_bits holds
 * codes 0..D. Device pointers, filled by the host after the segment parse.
 * An argument of k_scan_generic alone: DevPlan, which every interpreter
 * kernel copies, stays as it was. */
struct StrKeyDev {
    const uint32_t* kmap[kMaxPackKeys];
    const int64_t* kbase[kMaxPackKeys];
};

/* Equi-join device context (one join item — see include/ytql_gpu.h
 * YtJoin). The hash table is open-addressing with the
 * row index as the claim word (hrow -1 = empty); duplicate keys are
 * detected by a post-build verify kernel, so inserts never read other
 * slots' keys (no publish race). Probes run in later kernels only. */
struct JoinDev {
    int32_t active;
    int32_t is_left;
    int32_t pkey_col;             /* primary key column */
    int32_t primary_ncols;        /* P: plan columns >= P are foreign */
    int32_t fval_col[kMaxCols];   /* foreign column per appended slot */
    int32_t f_shift[kMaxCols];    /* uniform row->segment shift per slot */
    int32_t fkey_shift;
    int32_t fkey_col;
    const DevSeg* fsegs;
    const SegEx* fsegex;
    const int32_t* f_off;         /* per FOREIGN column: first segment */
    const int32_t* f_cnt;
    const uint64_t* hkey;
    const int64_t* hrow;          /* -1 = empty (slot claim; dup keys may
                                     occupy several slots — probes stop at
                                     the FIRST matching slot, whose chead
                                     holds the match list) */
    uint64_t hmask;
    int64_t null_row;             /* head of the null-key chain, or -1 */
    int64_t frows;
    /* duplicate foreign keys (registry.cpp MultiJoinOpHelper cross-product
     * expansion): per-slot match-list head + per-foreign-row next links */
    const int64_t* chead;         /* [nslots] chain head row, -1 */
    const int64_t* fnext;         /* [frows] next same-key row, -1 */
    int32_t has_dups;             /* any key (incl. null) with >1 row */
    /* 0: int64/uint64/boolean keys, hkey = the key's bits, rows probe the
     * table. 1: STRING keys (strjoin.h), hkey = the byte hash; the table is
     * probed once per ENTRY of the primary key column's kept segments
     * (k_strjoin_entries) and a row reads jmap[jbase[seg] + id - 1]: the
     * head of its key's match list, or -1. */
    int32_t key_kind;
    const int32_t* jmap;
    const int64_t* jbase;         /* per kept key segment: first jmap index */
};

/* versioned scan-format read: per-segment device
 * descriptor; ts_data/val_data point at device copies of the encoded
 * segment blobs (layouts in include/ytql_gpu.h) */
struct VSegDev {
    int64_t row_start;
    int64_t row_count;
    uint64_t base_timestamp;
    uint32_t exp_w, exp_d, exp_v;
    uint32_t vtype;      /* YT_VSEG_* (include/ytql_gpu.h) */
    uint32_t vflags;     /* YT_VSEG_F_* */
    uint32_t pad_;
    uint64_t base_value;
    const char* ts_data;
    const char* val_data;
};

/* device output value for the scan+project path (16 B). A YT_VT_STRING
 * value holds its entry reference in bits (P_STR_REF) as the interpreter
 * leaves it; after the compaction / length pass pad_ = its length in bytes,
 * and in the rows sent to the host bits = its byte offset in the pool. */
struct DevOutVal {
    uint64_t bits;
    uint32_t type;     /* YT_VT_*; YT_VT_NULL for null */
    uint32_t pad_;
};

/* scan+project with STRING projections (kernels.hip k_proj_*, k_str_*).
 * The window is compacted on the device in tiles of kProjTile rows; a tile's
 * total is {passing rows, bytes of their non-null string values}. */
constexpr int kProjTile = 2048;
struct ProjTot {
    unsigned long long rows;
    unsigned long long bytes;
};

/* one string value to copy: entry `ref` (P_STR_REF bits) -> pool[dst, dst+len).
 * ref == kStrRefNull stands for a null value: len 0, nothing copied. */
constexpr uint64_t kStrRefNull = ~0ULL;
struct StrGatherRec {
    uint64_t ref;
    uint64_t dst;
    uint32_t len;
    uint32_t pad_;
};

/* Group hash-table slot layout (generic path):
 *   u64 key_bits | u64 cnt | per-agg { u64 bits, u64 nonnull }
 * stride_u64 = 2 + 2*agg_count. key_bits == 0 means EMPTY; real key 0 and
 * null key live in the side accumulators of TableHdr. */
struct TableHdr {
    uint64_t nslots;          /* power of two */
    uint64_t mask;
    /* side groups: [0] = the in-table empty-sentinel key (bits in
     * side_key_bits[0]), [1] = null key */
    uint64_t side_used[2];    /* 0/1 */
    uint64_t side_key_bits[2];
    uint64_t side_cnt[2];
    uint64_t side_agg[2][2 * kMaxAggs];  /* bits, nonnull per agg */
    unsigned long long ngroups;          /* inserted (excl. side) */
    uint64_t overflow;        /* set when probe failed / group limit hit */
    int64_t group_limit;      /* 0 = unlimited */
};

/* Compacted output record (device→host), generic path */
struct OutGroup {
    uint64_t key_bits;
    uint64_t key_meta;        /* bit0 null-key */
    uint64_t cnt;
    uint64_t agg_bits[kMaxAggs];
    uint64_t agg_nonnull[kMaxAggs];
};

/* Compacted output record of the partitioned path when the whole query runs
 * in one call (yt_gpu_query_execute): that family has one int64 key, at most
 * one sum and an optional sum(1), and its null key is a side slot, so 32 of
 * OutGroup's 88 bytes say everything. The D2H of the groups is the largest
 * copy of the step. */
struct SlimGroup {
    uint64_t key_bits;
    uint64_t cnt;
    uint64_t sum_bits;        /* the one sum; 0 without */
    uint64_t sum_nonnull;
};
static_assert(sizeof(SlimGroup) == 32, "two 16-byte stores per group");

/* Fast-shape descriptor (analysed by the host):
 * filter: optional int64 range on one column; key: direct column or none;
 * aggs: sum(direct col) and/or sum(1). */
struct FastShape {
    int32_t valid;
    int32_t ragged;           /* the shape fits but segment row counts differ:
                                 the partitioned path only (its tiles are
                                 masked per segment), never k_scan_fast */
    int32_t filter_col;       /* -1 = none */
    int64_t filter_lo, filter_hi;   /* inclusive */
    int32_t key_col;          /* -1 = global */
    int32_t nsum;             /* number of sum(col) aggs */
    int32_t sum_col[kMaxAggs];
    int32_t sum_slot[kMaxAggs];     /* agg index of each sum */
    int32_t have_sum1;
};

/* fast-kernel launch descriptors */
struct FastCol {
    int32_t seg_off;      /* into segs/segex: first segment of this column */
    int32_t seg_cnt;
};

struct FastParams {
    int32_t nused;               /* staged columns */
    int32_t tile_rows;
    int32_t tiles_per_seg;       /* uniform by the 128Ki interior-segment cap */
    int32_t filter_idx;          /* index into used cols; -1 none */
    int32_t key_idx;             /* -1 = global aggregate */
    int32_t nsum;
    int32_t sum_idx[kMaxAggs];   /* used-col index of each sum arg */
    int32_t sum_slot[kMaxAggs];  /* agg slot in table layout */
    int32_t agg_count;           /* table stride basis */
    int64_t filter_lo, filter_hi;
    int64_t row_count;
    int32_t nsegs_per_col;
    int32_t ntiles;
    int32_t stage_bm_mask;       /* bit u: used col u has nulls — stage+check */
    int32_t pad2_;
};

/* two-phase partitioned group-by (BASELINE configs 3/4 family):
 * Phase A (k_scan_partition): fused decode+filter; every row is decoded once
 * into an 8-byte packed or 16-byte {key,val} record and partitioned into kNB
 * buckets (mirrors the reference's in-process shuffle partition,
 * shuffling_reader.cpp:40-42, pushed down to the row level so aggregation
 * can run in LDS). A workgroup gathers a tile's records bucket-major in an
 * LDS scratch and copies each bucket's run out as contiguous stores.
 * Phase B (k_bucket_agg / k_bucket_agg_direct): one workgroup per bucket
 * aggregates its records in an LDS table and emits compacted OutGroups or
 * SlimGroups. Both flush through bucket_flush: ranks by ballot and popcount,
 * ONE reservation per workgroup on out_counter and th->ngroups, groups
 * stored at base + rank in slot order. The direct kernel's table is
 * 1 << dshift slots of {cnt | nonnull << 32, sum}, an array each, and the
 * flush's scan words behind them (64 KiB + 64 B at dshift 12: the launcher
 * raises the kernel's dynamic LDS limit). */
constexpr int kNB = 1024;          /* partition buckets */
constexpr int kHSlots = 2048;      /* LDS table slots per bucket (48 KB -> 3 WGs/CU) */
constexpr uint64_t kEmptyKey = 0x8000000000000000ULL;  /* INT64_MIN bits */
/* k_bucket_agg_direct: a full pass of a workgroup over a sub-region of
 * packed records is eight 16-byte loads per lane, two records each; what is
 * left below a full pass goes in turns of one load per lane. k_bucket_agg's
 * full pass is eight records per lane, half as many. */
constexpr int kBucketPassRecords = 256 * 8 * 2;

/* phase-A geometry: a thread holds up to 16 rows of a tile (8 with 16-byte
 * records), a compile-time constant so the tile's records and (bucket, rank)
 * words stay in registers. Either way a tile's records fill a 64 KiB LDS
 * scratch; with the three kNB-word histograms that is 76 KiB, two
 * 512-thread workgroups per CU.
 * A (bucket, XCD sub) region must hold one whole tile whatever the key skew
 * (bucket_stride's fixed slack is 4096 records for that reason), so packed
 * records tile kPartTileMax rows only once bucket_stride reaches that, and
 * kPartTileMin below; the kernel masks the rows a tile does not use. */
constexpr int kPartThreads = 512;
constexpr int kPartTileMax = 16 * kPartThreads;    /* packed records, large inputs */
constexpr int kPartTileMin = 8 * kPartThreads;     /* 16-byte records; small inputs */
constexpr size_t kPartScratchBytes = (size_t)kPartTileMax * 8;
constexpr size_t kPartLdsBytes = kPartScratchBytes + 3 * kNB * 4 + 64;

struct PartParams {
    int32_t tile_rows;            /* kPartTileMax or kPartTileMin */
    int32_t tiles_per_seg;        /* the rows, or whole tiles, past a segment's
                                     end are masked */
    int32_t ntiles;
    int32_t filter_idx;           /* used-col index; -1 none */
    int32_t key_idx;              /* used-col index (required) */
    int32_t val_idx;              /* used-col index of the sum arg; -1 none */
    int32_t nused;
    int32_t has_val_nulls;        /* value-null rows go to the null stream */
    int32_t has_key_nulls;
    int32_t has_filter_nulls;
    int32_t sum_slot;             /* agg slot of the sum; -1 none */
    int32_t agg_count;
    int64_t filter_lo, filter_hi;
    int64_t bucket_stride;        /* record capacity per (bucket, XCD sub) region */
    int64_t nbucket_stride;       /* null-stream capacity per region */
    /* 8-byte packed records: when the key and value zigzag spans fit 64
     * bits together, a record is (kzz - gmin_k) | (vzz - gmin_v) << bits_k
     * — half the partition traffic of {key,val} pairs. */
    int32_t packed_mode;
    int32_t bits_k;
    uint64_t gmin_k, gmin_v;
    /* direct-span mode (small key zigzag span): buckets are key-RANGE
     * slices (bucket = krel >> dshift) and phase B indexes an LDS array
     * directly — no hash probe, no CAS, no stored keys. The copy-out of
     * phase A re-derives a record's bucket the same way. */
    int32_t direct_mode;
    int32_t dshift;               /* per-bucket key-slot range = 1 << dshift */
    /* the plain decode (kernels.hip part_decode_plain): packed_mode and
     * direct_mode, a value column, no filter, no nulls in key or value,
     * every key segment at most 32 bits wide and the key column's zigzag
     * maximum below UINT64_MAX, so that no row is a side row (INT64_MIN has
     * zz = UINT64_MAX). The widths are bounded through the segment headers'
     * range, so a header range that saturates at UINT64_MAX rules it out
     * too, whatever an exact scan found. The launcher picks the
     * instantiation by it. */
    int32_t plain_mode;
    int32_t pad_;
};

/* which k_scan_partition a launch ran (yt_gpu_debug_partition_variant) */
constexpr int kPartVariantPacked = 1;
constexpr int kPartVariantPlain = 2;   /* set together with packed */

/* string-keyed GROUP BY (BASELINE config 5 family): dictionary-encoded
 * string key segments aggregate by per-segment dictionary id into dense
 * per-segment accumulators, then dictionary entries merge across segments
 * in a global table keyed by (hash, byte-exact string compare). */
struct StrGroupParams {
    int32_t key_seg_off;          /* key column segments */
    int32_t key_seg_cnt;
    int32_t val_seg_off;          /* sum-arg column segments; -1 = none */
    int32_t val_seg_cnt;
    int32_t val_is_double;
    int32_t sum_slot;             /* agg slot of the sum; -1 = none */
    int32_t agg_count;
    int32_t tile_rows;
    int32_t tiles_per_seg;
    int32_t ntiles;
    int32_t has_val_nulls;
    int64_t row_count;
};

/* merge-table slot of every string-key merge. The protocol below is written
 * once, in kernels.hip strslot_find_or_claim; what differs per merge is the
 * Key it is given. rep names the slot's owner, 0 = empty:
 *   dictionary entry (k_strgrp_merge, k_strgen_merge)  (seg+1)<<32 | 1-based id
 *   exchanged state  (k_strst_merge)                   state index + 1
 * The owner's hash is NOT stored: readers recompute it from the
 * precomputed per-key hash array via rep, which avoids any publication
 * ordering between the claim and a hash field.
 * 64-byte slot, one cache line: rep claims the slot (CAS); the claimer
 * then publishes the key identity in-slot with RELAXED agent stores —
 * ident = hash48|len16, pfx = the key's first 16 bytes. Readers verify
 * with relaxed loads; a stale (zero / partially visible) identity only
 * demotes the probe to the exact owner-array compare, never a wrong
 * accept: ident mismatch is exact (FNV48+len of equal strings always
 * match), ident match with len <= 16 is decided by pfx (the FULL bytes),
 * len > 16 falls back to the byte compare against the owner's bytes
 * (Key::equals_owner). */
struct StrSlot {
    unsigned long long rep;       /* names the owner (above); 0 = empty */
    uint64_t ident;               /* hash48<<16 | len; 0 = unpublished */
    uint64_t pfx[2];              /* first 16 key bytes, zero-padded */
    uint64_t sum_bits;
    uint64_t cnt;                 /* low 32 = row count, high 32 = nonnull */
    uint64_t pad0_;
    uint64_t pad_;
};
static_assert(sizeof(StrSlot) == 64, "one cache line per slot");

/* one distinct string of a multi-key GROUP BY's STRING key column
 * (kernels.hip k_strkey_*), index = its dense id. Brought to the host once
 * per query with the byte pool: D records, not one per group. */
struct StrKeyId {
    uint64_t off_len;             /* pool offset << 24 | length */
    unsigned long long rep;       /* claim word of the owner entry (StrSlot) */
};
/* kmap word of an entry without an id (a null entry of a direct layout) */
constexpr uint32_t kStrKeyNoId = 0xFFFFFFFFu;

/* ORDER BY ... LIMIT k-selection (see kernels.hip k_topk_*).
 * Range-adaptive digits: candidates are mapped keys in [lo, hi]; digit =
 * (m - lo) >> shift (< 2048 by host choice of shift). Pass 0 also reduces
 * the data min/max so the next pass bins the ACTUAL key range instead of
 * stepping fixed 11-bit prefixes through constant high bits. */
struct TopkPass {
    int32_t order_proj;       /* projection index whose value is the order key */
    int32_t desc;             /* invert mapped key */
    int32_t level0;           /* count nulls + reduce min/max on this pass */
    int32_t shift;
    uint64_t lo, hi;          /* inclusive candidate interval */
};
struct TopkGather {
    int32_t order_proj;
    int32_t desc;
    int32_t all_nonnull;      /* 1 = every non-null row is a strict hit */
    int32_t pad_;
    uint64_t lo, hi;          /* strict: m < lo; tie: lo <= m <= hi */
    int64_t cap_strict;       /* rows the histograms counted below lo */
    int64_t cap_tie;
    int64_t cap_null;
};

/* merged string-state group (device→host) for the string-keyed two-phase
 * front query: counts are full u64 (multi-rank accumulation can exceed the
 * 32-bit halves the single-pass path packs). */
struct OutStrState {
    uint64_t off_len;             /* out_pool offset<<24 | len */
    uint64_t sum_bits;
    uint64_t cnt;
    uint64_t nonnull;
};

/* compacted string group (device→host). 24 B: this array is the bulk of
 * the query's D2H at 100 M groups, so the key ref packs off|len (pool is
 * bounded by the dict blob bytes << 2^48) and counts stay in the slot's
 * cnt|nonnull 32-bit-halves encoding. */
struct OutStrGroup {
    uint64_t off_len;             /* pool_off<<24 | len (len cap 16 MB =
                                     the reference MaxStringValueLength) */
    uint64_t sum_bits;
    uint64_t cnt_nonnull;         /* low 32 = row count, high 32 = nonnull */
};

/* general string-keyed GROUP BY (kernels.hip k_strgen_*): what the merge
 * needs to fold one accumulator record {rows, {bits, nonnull} per agg} into
 * a slot's record of the same layout. */
struct StrGenAggs {
    int32_t count;
    int32_t func[kMaxAggs];       /* YT_AGG_* */
    int32_t is_double[kMaxAggs];  /* sum/avg state is a double */
};

/* per-group aggregates of the general string path (device→host), index-
 * aligned with the OutStrGroup array that carries the keys; full 64-bit
 * counts, finalized on the host by finalize_row */
struct OutStrAgg {
    uint64_t cnt;
    uint64_t agg_bits[kMaxAggs];
    uint64_t agg_nonnull[kMaxAggs];
};

struct KernelTimes {
    float scan_ms;
    int64_t scan_launches;
    float other_ms;
};

} /* namespace ytql */
