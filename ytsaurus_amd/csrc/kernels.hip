/* kernels.hip — hand-written CDNA4 (gfx950) kernels for the YTsaurus
 * dynamic-table query hot path: fused columnar decode → filter →
 * hash-aggregate, plus state partition/merge for the 8-GPU exchange.
 *
 * The compute semantics restate (MI355X-native, not ported):
 *   - bit-unpack:   reference bit_packed_unsigned_vector-inl.h:108-186
 *   - int64 decode: integer_column_reader.cpp:19-127,391-449 (zigzag-space
 *                   frame of reference: v = ZigZagDecode64(min + packed))
 *   - filter:       cg_fragment_compiler.cpp:3460-3510 (here fused into the
 *                   decode loop instead of a row-at-a-time branch)
 *   - group insert: cg_routines/registry.cpp:1783-1834 (open addressing; our
 *                   table is a device CAS-claimed linear-probe table; the
 *                   reference's hash function is internal and not mirrored —
 *                   results are order-free)
 *   - aggregates:   udf/sum.c (null-propagating; int64 wraps mod 2^64, so
 *                   unordered atomic u64 adds are bit-exact)
 *   - merge/shuffle: engine/coordinator.cpp:420-505 + shuffling_reader.cpp:21-88
 *
 * Everything is HBM-bandwidth-bound integer work — no MFMA on this path.
 * All tables are accessed with device-scope atomics (per-XCD L2s are not
 * coherent; see MI355X microarch notes).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "common.h"
#include "strpred.h"
#include "inlist.h"
#include "strjoin.h"
#include "launch.h"
#include "../../include/ytql_gpu.h"

namespace ytql {

/* ------------------------------------------------------------------ */
/* device helpers                                                      */

__device__ __forceinline__ int64_t zz_dec(uint64_t n)
{
    return (int64_t)((n >> 1) ^ (~(n & 1) + 1));
}

__device__ __forceinline__ uint64_t mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

/* must match oracle yto_partition_hash */
__device__ __forceinline__ uint64_t partition_hash(uint64_t key_bits, int key_null)
{
    return mix64(key_bits ^ (key_null ? 0xDEADBEEF12345678ULL : 0));
}

struct DVal {
    uint64_t bits;
    uint8_t type;    /* YT_VT_* */
    uint8_t null_;
};

__device__ __forceinline__ uint64_t bp_get(const uint64_t* data, uint32_t width, uint64_t index)
{
    if (width == 0) return 0;
    if (width == 64) return data[index];
    uint64_t bit = index * width;
    const uint64_t* word = data + (bit >> 6);
    unsigned off = (unsigned)(bit & 63);
    uint64_t w1 = *word >> off;
    if (off + width > 64) {
        uint64_t w2 = (word[1] & ((1ULL << ((off + width) & 63)) - 1)) << (64 - off);
        w1 |= w2;
    } else {
        w1 &= (1ULL << width) - 1;
    }
    return w1;
}

__device__ __forceinline__ int bm_get(const uint8_t* bm, uint64_t index)
{
    return (bm[index >> 3] >> (index & 7)) & 1;
}

/* extract value `index` (absolute in segment) from an LDS window that holds
 * words [w0, ...] of the packed vector */
__device__ __forceinline__ uint64_t bp_get_win(const uint64_t* win, uint32_t width,
                                               uint64_t index, uint64_t w0)
{
    if (width == 0) return 0;
    uint64_t bit = index * width;
    uint64_t wi = (bit >> 6) - w0;
    unsigned off = (unsigned)(bit & 63);
    if (width == 64) return win[wi];
    uint64_t w1 = win[wi] >> off;
    if (off + width > 64) {
        w1 |= (win[wi + 1] & ((1ULL << ((off + width) & 63)) - 1)) << (64 - off);
    } else {
        w1 &= (1ULL << width) - 1;
    }
    return w1;
}


/* staging copy with explicit memory-level parallelism: 8 independent global
 * loads in flight per thread before the LDS writes (a simple
 * `for(i=tid;...) dst[i]=src[i]` loop serializes on each load's s_waitcnt —
 * measured 83% WAIT_ANY on the fused scan) */
__device__ __forceinline__ void stage_copy(uint64_t* dst, const uint64_t* src,
                                           int64_t nwords, int tid)
{
    int64_t base = tid;
    for (; base + 256 * 7 < nwords; base += 256 * 8) {
        uint64_t r0 = src[base];
        uint64_t r1 = src[base + 256];
        uint64_t r2 = src[base + 512];
        uint64_t r3 = src[base + 768];
        uint64_t r4 = src[base + 1024];
        uint64_t r5 = src[base + 1280];
        uint64_t r6 = src[base + 1536];
        uint64_t r7 = src[base + 1792];
        dst[base] = r0;
        dst[base + 256] = r1;
        dst[base + 512] = r2;
        dst[base + 768] = r3;
        dst[base + 1024] = r4;
        dst[base + 1280] = r5;
        dst[base + 1536] = r6;
        dst[base + 1792] = r7;
    }
    if (base + 256 * 3 < nwords) {
        uint64_t r0 = src[base];
        uint64_t r1 = src[base + 256];
        uint64_t r2 = src[base + 512];
        uint64_t r3 = src[base + 768];
        dst[base] = r0;
        dst[base + 256] = r1;
        dst[base + 512] = r2;
        dst[base + 768] = r3;
        base += 256 * 4;
    }
    if (base + 256 < nwords) {
        uint64_t r0 = src[base];
        uint64_t r1 = src[base + 256];
        dst[base] = r0;
        dst[base + 256] = r1;
        base += 256 * 2;
    }
    for (; base < nwords; base += 256) dst[base] = src[base];
}

/* branchless global-memory funnel extraction; safe to read one word past
 * the packed vector (the segment's null bitmap follows it) */
__device__ __forceinline__ uint64_t bp_gl(const uint64_t* base, uint64_t mask,
                                          uint32_t width, uint64_t index)
{
    uint64_t bit = index * width;
    unsigned off = (unsigned)(bit & 63);
    uint64_t lo = base[bit >> 6] >> off;
    uint64_t hi = off ? (base[(bit >> 6) + 1] << (64 - off)) : 0;
    return (lo | hi) & mask;
}

/* the same from n words staged in LDS; never reads past them: a value that
 * ends in the last word takes nothing from the clamped one */
__device__ __forceinline__ uint64_t bp_lds(const uint64_t* words, uint32_t n, uint64_t mask,
                                           uint32_t width, uint32_t index)
{
    const uint32_t bit = index * width;
    const unsigned off = bit & 63;
    const uint32_t wi = bit >> 6;
    const uint64_t lo = words[wi] >> off;
    const uint64_t hi = (words[wi + 1 < n ? wi + 1 : wi] << 1) << (63 - off);
    return (lo | hi) & mask;
}

/* ------------------------------------------------------------------ */
/* segment header parsing (one thread per segment)                     */

/* fills e from the segment's headers. Returns false for a STRING column's
 * segment, which takes no part in the per-column words; otherwise true, with
 * *nullbits = the bits the segment adds to its column's null flags. */
__device__ __forceinline__ bool parse_segment(const DevSeg& s, SegEx& e,
                                              unsigned* nullbits)
{
    const uint64_t* b = s.blob;
    *nullbits = 0;
    if (s.type == YT_SEG_DOUBLE) {
        /* [u64 count][doubles][null bitmap]. The blob's own count places the
         * bitmap: input_row_limit may have clamped s.row_count below it. */
        e.off_doubles_bytes = 8;
        e.off_bitmap_bytes = 8 + 8 * (int64_t)b[0];
        e.w_values = 64;
    } else if (s.is_signed == 2) {
        /* STRING column — string_column_writer.cpp dump layouts.
         * off_values_words = offsets vector data; off_doubles_bytes = blob
         * byte offset of the string data; dict_size = dictionary entries. */
        uint64_t h0 = b[0];
        uint64_t n0 = h0 & ((1ULL << 56) - 1);
        uint32_t w0 = (uint32_t)(h0 >> 56);
        int64_t words0 = 1 + (int64_t)((w0 * n0 + 63) >> 6);
        switch (s.type) {
        case YT_SEG_DICTIONARY_DENSE: {
            /* [ids][offsets][data] */
            e.w_ids = w0;
            e.run_count = (uint32_t)n0;
            e.off_ids_words = 1;
            uint64_t h1 = b[words0];
            e.w_values = (uint32_t)(h1 >> 56);
            e.dict_size = (uint32_t)(h1 & ((1ULL << 56) - 1));
            e.off_values_words = words0 + 1;
            int64_t words1 = 1 + (int64_t)(((uint64_t)e.w_values * e.dict_size + 63) >> 6);
            e.off_doubles_bytes = (words0 + words1) * 8;
            e.flags |= 8;   /* dictionary string segment */
            break;
        }
        case YT_SEG_DICTIONARY_RLE: {
            /* [row starts][ids][offsets][data] */
            e.w_starts = w0;
            e.run_count = (uint32_t)n0;
            e.off_starts_words = 1;
            uint64_t h1 = b[words0];
            e.w_ids = (uint32_t)(h1 >> 56);
            uint32_t nids = (uint32_t)(h1 & ((1ULL << 56) - 1));
            e.run_count = nids;
            e.off_ids_words = words0 + 1;
            int64_t words1 = 1 + (int64_t)(((uint64_t)e.w_ids * nids + 63) >> 6);
            uint64_t h2 = b[words0 + words1];
            e.w_values = (uint32_t)(h2 >> 56);
            e.dict_size = (uint32_t)(h2 & ((1ULL << 56) - 1));
            e.off_values_words = words0 + words1 + 1;
            int64_t words2 = 1 + (int64_t)(((uint64_t)e.w_values * e.dict_size + 63) >> 6);
            e.off_doubles_bytes = (words0 + words1 + words2) * 8;
            e.flags |= 8;
            break;
        }
        case YT_SEG_DIRECT_DENSE: {
            /* [offsets, diff-from-expected][null bitmap][data]
             * (string_column_writer.cpp DumpDirectValues). As a GROUP key
             * this rides the dictionary machinery with an IDENTITY
             * dictionary: entry j = row j's string, null rows skipped via
             * the bitmap (their accumulators stay zero). */
            e.w_values = w0;
            e.dict_size = (uint32_t)n0;      /* = row_count */
            e.off_values_words = 1;
            e.off_bitmap_bytes = words0 * 8;
            /* one bitmap bit per stored row (n0), not per kept row:
             * input_row_limit may have clamped s.row_count */
            int64_t bm = (((int64_t)n0 + 7) / 8 + 7) & ~(int64_t)7;
            e.off_doubles_bytes = words0 * 8 + bm;
            e.flags |= 32;  /* direct-dense string segment */
            break;
        }
        case YT_SEG_DIRECT_RLE: {
            /* [run starts][run END offsets, diff-from-expected]
             * [run null bitmap][run data] (string_column_writer.cpp
             * DumpDirectRleData). As a GROUP key this is an identity
             * dictionary over RUNS: entry j = run j's string, row -> run by
             * binary search on the starts, null runs by the bitmap (their
             * entries are empty and their accumulators stay zero). */
            e.w_starts = w0;
            e.run_count = (uint32_t)n0;
            e.off_starts_words = 1;
            uint64_t h1 = b[words0];
            e.w_values = (uint32_t)(h1 >> 56);
            e.dict_size = e.run_count;
            e.off_values_words = words0 + 1;
            int64_t words1 = 1 + (int64_t)(((uint64_t)e.w_values * e.run_count + 63) >> 6);
            e.off_bitmap_bytes = (words0 + words1) * 8;
            int64_t bm = (((int64_t)e.run_count + 7) / 8 + 7) & ~(int64_t)7;
            e.off_doubles_bytes = e.off_bitmap_bytes + bm;
            e.flags |= 64;  /* direct-RLE string segment */
            break;
        }
        default:
            e.flags |= 16;  /* unknown string layout: no GPU key path */
            break;
        }
        return false;
    } else if (s.type == YT_SEG_BOOLEAN) {
        /* [u64 count][value bitmap][null bitmap], both 8-aligned */
        e.off_doubles_bytes = 8;     /* value bitmap */
        e.off_bitmap_bytes = 8 + (((int64_t)b[0] + 7) / 8 + 7) / 8 * 8;
        e.w_values = 1;
    } else {
        uint64_t h0 = b[0];
        uint64_t n0 = h0 & ((1ULL << 56) - 1);
        uint32_t w0 = (uint32_t)(h0 >> 56);
        int64_t words0 = 1 + (int64_t)((w0 * n0 + 63) >> 6);
        switch (s.type) {
        case YT_SEG_DIRECT_DENSE: {
            e.w_values = w0;
            e.off_values_words = 1;
            e.off_bitmap_bytes = words0 * 8;
            break;
        }
        case YT_SEG_DICTIONARY_DENSE: {
            e.w_values = w0;                 /* dictionary vector */
            e.dict_size = (uint32_t)n0;
            e.off_values_words = 1;
            uint64_t h1 = b[words0];
            e.w_ids = (uint32_t)(h1 >> 56);
            e.run_count = (uint32_t)(h1 & ((1ULL << 56) - 1));
            e.off_ids_words = words0 + 1;
            break;
        }
        case YT_SEG_DIRECT_RLE: {
            e.w_values = w0;
            e.run_count = (uint32_t)n0;
            e.off_values_words = 1;
            e.off_bitmap_bytes = words0 * 8;
            int64_t bm_bytes = ((int64_t)n0 + 7) / 8;
            bm_bytes = (bm_bytes + 7) & ~(int64_t)7;
            int64_t starts_word = words0 + bm_bytes / 8;
            uint64_t h2 = b[starts_word];
            e.w_starts = (uint32_t)(h2 >> 56);
            e.off_starts_words = starts_word + 1;
            break;
        }
        case YT_SEG_DICTIONARY_RLE: {
            e.w_values = w0;
            e.dict_size = (uint32_t)n0;
            e.off_values_words = 1;
            uint64_t h1 = b[words0];
            e.w_ids = (uint32_t)(h1 >> 56);
            e.run_count = (uint32_t)(h1 & ((1ULL << 56) - 1));
            int64_t words1 = 1 + (int64_t)(((uint64_t)e.w_ids * e.run_count + 63) >> 6);
            e.off_ids_words = words0 + 1;
            int64_t starts_word = words0 + words1;
            uint64_t h2 = b[starts_word];
            e.w_starts = (uint32_t)(h2 >> 56);
            e.off_starts_words = starts_word + 1;
            break;
        }
        }
    }
    if (s.type != YT_SEG_DIRECT_DENSE && s.type != YT_SEG_DOUBLE) {
        /* dictionary/RLE null presence is unknown without an id scan —
         * be conservative (fast paths only run on DirectDense anyway) */
        *nullbits = 2u;
    }
    return true;
}

/* The per-column words (null flags, zigzag min / max) and the widest value
 * vector are combined within the wave before the global atomics: segments
 * arrive in column order, so a wave holds one or two distinct columns and
 * issues a handful of atomics where every thread used to issue four on the
 * same few addresses. */
__global__ void k_parse_segments(const DevSeg* segs, int nsegs, SegEx* out,
                                 unsigned* max_width_out,
                                 unsigned* col_null_flags /* kMaxCols words */,
                                 unsigned long long* col_zzmin /* kMaxCols, init ~0 */,
                                 unsigned long long* col_zzmax /* kMaxCols, init 0 */)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int col = -1;               /* -1: nothing to contribute */
    unsigned nullbits = 0, width = 0;
    unsigned long long lo = ~0ULL, hi = 0;
    if (i < nsegs) {
        const DevSeg& s = segs[i];
        SegEx e = {};
        const bool counts = parse_segment(s, e, &nullbits);
        out[i] = e;
        if (counts) {
            col = s.col;
            width = e.w_values;
            /* per-column zigzag-space range, from segment meta alone
             * (value = min_value + packed, packed < 2^w) */
            lo = (unsigned long long)s.min_value;
            unsigned long long span = (e.w_values >= 64) ? ~0ULL
                                    : ((1ULL << e.w_values) - 1);
            hi = lo + span;   /* may wrap for degenerate metas */
            if (hi < lo) hi = ~0ULL;
        }
    }
    unsigned wmax = width;
    for (int sh = 32; sh >= 1; sh >>= 1)
        wmax = max(wmax, (unsigned)__shfl_xor((int)wmax, sh, 64));
    unsigned long long todo = __ballot(col >= 0);
    if (lane == 0 && todo) atomicMax(max_width_out, wmax);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int c = __shfl(col, leader, 64);
        const bool mine = (col == c);
        unsigned nb = mine ? nullbits : 0u;
        unsigned long long mn = mine ? lo : ~0ULL;
        unsigned long long mx = mine ? hi : 0ULL;
        for (int sh = 32; sh >= 1; sh >>= 1) {
            nb |= (unsigned)__shfl_xor((int)nb, sh, 64);
            mn = min(mn, (unsigned long long)__shfl_xor((long long)mn, sh, 64));
            mx = max(mx, (unsigned long long)__shfl_xor((long long)mx, sh, 64));
        }
        if (lane == leader) {
            if (nb) atomicOr(&col_null_flags[c], nb);
            atomicMin(&col_zzmin[c], mn);
            atomicMax(&col_zzmax[c], mx);
        }
        todo &= ~__ballot(mine);
    }
}

/* k_scan_zzrange's stream over one segment's packed words (width 1..64; T
 * holds a value: uint32_t up to width 32). A thread takes whole words, 256
 * apart, and extracts the values that START in its word (v = the first of
 * them, sb = its bit in the word); a value that runs over the word's end
 * takes its top bits from the next word, which may be the one past the
 * vector. Stepping 256 words = 16384 bits = q * w + r moves (v, sb) without
 * dividing. Rows from n on do not count. */
template <typename T>
__device__ __forceinline__ void zz_stream(const uint64_t* words, const uint64_t* bm64,
                                          uint32_t n, uint32_t w, uint32_t tid,
                                          T& mn, T& mx)
{
    const T mask = (w >= 8 * sizeof(T)) ? (T)~(T)0 : (T)(((T)1 << w) - 1);
    const int64_t nwords = ((int64_t)n * w + 63) >> 6;
    const uint32_t q = 16384u / w, r = 16384u % w;
    uint32_t v = (64u * tid + w - 1) / w;
    uint32_t sb = v * w - 64u * tid;
    auto take = [&](uint64_t lo, uint64_t hi) {
        if (v < n) {
            uint64_t nb = 0;
            if (bm64) {
                /* null bits of the rows from v on: 64 cover a word's values */
                const unsigned sh = v & 63;
                nb = bm64[v >> 6] >> sh;
                const uint32_t last = min(v + (63u - sb) / w, n - 1);
                if ((last >> 6) != (v >> 6)) nb |= bm64[last >> 6] << (64 - sh);
            }
            /* a word starts at most 64 values: with 64 rows left, no row check */
            const uint32_t bend = (n - v >= 64u) ? 64u : min(64u, sb + (n - v) * w);
            for (uint32_t b = sb; b < bend; b += w, nb >>= 1) {
                T z = (T)(lo >> b);
                if (b + w > 64) z |= (T)((T)hi << (64 - b));
                z &= mask;
                if (!(nb & 1)) { mn = min(mn, z); mx = max(mx, z); }
            }
        }
        /* the next word of this thread, 16384 bits on */
        if (sb >= r) { v += q; sb -= r; }
        else { v += q + 1; sb += w - r; }
    };
    int64_t i = tid;
    for (; i + 768 < nwords; i += 1024) {
        /* eight independent loads in flight before the first use */
        const uint64_t a0 = words[i], b0 = words[i + 1];
        const uint64_t a1 = words[i + 256], b1 = words[i + 257];
        const uint64_t a2 = words[i + 512], b2 = words[i + 513];
        const uint64_t a3 = words[i + 768], b3 = words[i + 769];
        take(a0, b0);
        take(a1, b1);
        take(a2, b2);
        take(a3, b3);
    }
    for (; i < nwords; i += 256) take(words[i], words[i + 1]);
}

/* exact zigzag-space min/max of one DirectDense int64 column (non-null
 * values): k_parse_segments' meta-only bound rounds every segment up to
 * min_value + 2^w - 1, which can overstate the span by one bit — enough to
 * disable packed records / direct-span mode on data that
 * actually fits (the headline config: 21+41 = 62 real bits, 22+42 = 64 by
 * meta). One workgroup per segment; out[0] = min (init ~0), out[1] = max
 * (init 0); no update when every value is null. The packed words are
 * streamed: each is loaded about once, coalesced, and every value is taken
 * from registers (a load pair per VALUE, as bp_gl does it, left the kernel
 * bound by load instructions at a third of the HBM rate). */
__global__ void __launch_bounds__(256)
k_scan_zzrange(const DevSeg* segs, const SegEx* segex, int seg_off,
               int has_nulls, unsigned long long* out)
{
    __shared__ unsigned long long red[8];   /* 4 waves x {min,max} */
    const int si = seg_off + blockIdx.x;
    const DevSeg& s = segs[si];
    const SegEx& e = segex[si];
    const uint64_t* words = s.blob + e.off_values_words;
    const uint32_t w = e.w_values;
    const uint8_t* bm = has_nulls
        ? (const uint8_t*)s.blob + e.off_bitmap_bytes : nullptr;
    const uint64_t* bm64 = (const uint64_t*)bm;   /* 8-aligned, zero-padded to 8 */
    uint64_t mn = ~0ULL, mx = 0;
    const uint32_t n = (uint32_t)s.row_count;
    if (w == 0) {
        /* every packed value is 0: the range is {0} once one row is non-null */
        bool any = false;
        if (!bm) any = n > 0;
        else for (uint32_t j = threadIdx.x; j < n; j += 256) any |= !bm_get(bm, j);
        if (any) { mn = 0; mx = 0; }
    } else {
        /* widths up to 32 keep their values, minimum and maximum in 32 bits */
        if (w <= 32) {
            uint32_t mn32 = ~0u, mx32 = 0;
            zz_stream<uint32_t>(words, bm64, n, w, threadIdx.x, mn32, mx32);
            if (mn32 <= mx32) { mn = mn32; mx = mx32; }   /* saw a value */
        } else {
            zz_stream<uint64_t>(words, bm64, n, w, threadIdx.x, mn, mx);
        }
    }
    for (int sh = 32; sh >= 1; sh >>= 1) {
        mn = min(mn, (uint64_t)__shfl_down((long long)mn, sh, 64));
        mx = max(mx, (uint64_t)__shfl_down((long long)mx, sh, 64));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave * 2] = mn; red[wave * 2 + 1] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mn = min(min(red[0], red[2]), min(red[4], red[6]));
        mx = max(max(red[1], red[3]), max(red[5], red[7]));
        if (mn != ~0ULL) {
            atomicMin(&out[0], s.min_value + mn);
            atomicMax(&out[1], s.min_value + mx);
        }
    }
}

/* null-presence scan: one workgroup per DirectDense segment, threads stride
 * the null bitmap words, wave-OR reduce (writer zero-pads to 8 bytes,
 * bitmap.h) */
__global__ void __launch_bounds__(256)
k_scan_nullflags(const DevSeg* segs, const SegEx* segex, int nsegs,
                 unsigned* col_null_flags)
{
    int seg = blockIdx.x;
    if (seg >= nsegs) return;
    const DevSeg& s = segs[seg];
    if (s.type != YT_SEG_DIRECT_DENSE && s.type != YT_SEG_DOUBLE) return;
    const SegEx& e = segex[seg];
    const uint64_t* bm = (const uint64_t*)((const uint8_t*)s.blob + e.off_bitmap_bytes);
    int64_t words = ((int64_t)s.row_count + 63) / 64;
    uint64_t any = 0;
    for (int64_t i = threadIdx.x; i < words; i += 256) any |= bm[i];
    any = (uint64_t)__any((long long)any != 0);
    __shared__ int found;
    if (threadIdx.x == 0) found = 0;
    __syncthreads();
    if (any && (threadIdx.x & 63) == 0) found = 1;
    __syncthreads();
    if (threadIdx.x == 0 && found) atomicOr(&col_null_flags[s.col], 1u);
}

/* ------------------------------------------------------------------ */
/* generic row-at-a-time value fetch (correctness path; any segment)   */

__device__ DVal seg_value_at(const DevSeg& s, const SegEx& e, int64_t row_in_seg,
                             uint8_t vt)
{
    DVal v;
    v.type = vt;
    v.null_ = 0;
    const uint64_t* b = s.blob;
    switch (s.type) {
    case YT_SEG_DOUBLE: {
        const uint8_t* bm = (const uint8_t*)b + e.off_bitmap_bytes;
        if (bm_get(bm, row_in_seg)) { v.null_ = 1; v.bits = 0; return v; }
        v.bits = ((const uint64_t*)((const uint8_t*)b + e.off_doubles_bytes))[row_in_seg];
        return v;
    }
    case YT_SEG_BOOLEAN: {
        const uint8_t* bm = (const uint8_t*)b + e.off_bitmap_bytes;
        if (bm_get(bm, row_in_seg)) { v.null_ = 1; v.bits = 0; return v; }
        v.bits = (uint64_t)bm_get((const uint8_t*)b + e.off_doubles_bytes, row_in_seg);
        return v;
    }
    case YT_SEG_DIRECT_DENSE: {
        const uint8_t* bm = (const uint8_t*)b + e.off_bitmap_bytes;
        if (bm_get(bm, row_in_seg)) { v.null_ = 1; v.bits = 0; return v; }
        uint64_t data = s.min_value + bp_get(b + e.off_values_words, e.w_values, row_in_seg);
        v.bits = s.is_signed ? (uint64_t)zz_dec(data) : data;
        return v;
    }
    case YT_SEG_DICTIONARY_DENSE: {
        uint64_t id = bp_get(b + e.off_ids_words, e.w_ids, row_in_seg);
        if (id == 0) { v.null_ = 1; v.bits = 0; return v; }
        uint64_t data = s.min_value + bp_get(b + e.off_values_words, e.w_values, id - 1);
        v.bits = s.is_signed ? (uint64_t)zz_dec(data) : data;
        return v;
    }
    case YT_SEG_DIRECT_RLE:
    case YT_SEG_DICTIONARY_RLE: {
        /* binary search the run whose start <= row; starts are sorted
         * (run starts, integer_column_writer.cpp:403-419) */
        const uint64_t* starts = b + e.off_starts_words;
        uint32_t lo = 0, hi = e.run_count;   /* first run with start > row, minus 1 */
        while (lo + 1 < hi) {
            uint32_t mid = (lo + hi) / 2;
            if (bp_get(starts, e.w_starts, mid) <= (uint64_t)row_in_seg) lo = mid;
            else hi = mid;
        }
        uint32_t run = lo;
        if (s.type == YT_SEG_DIRECT_RLE) {
            const uint8_t* bm = (const uint8_t*)b + e.off_bitmap_bytes;
            if (bm_get(bm, run)) { v.null_ = 1; v.bits = 0; return v; }
            uint64_t data = s.min_value + bp_get(b + e.off_values_words, e.w_values, run);
            v.bits = s.is_signed ? (uint64_t)zz_dec(data) : data;
        } else {
            uint64_t id = bp_get(b + e.off_ids_words, e.w_ids, run);
            if (id == 0) { v.null_ = 1; v.bits = 0; return v; }
            uint64_t data = s.min_value + bp_get(b + e.off_values_words, e.w_values, id - 1);
            v.bits = s.is_signed ? (uint64_t)zz_dec(data) : data;
        }
        return v;
    }
    }
    v.null_ = 1;
    v.bits = 0;
    return v;
}

/* ------------------------------------------------------------------ */
/* postfix expression interpreter — same semantics as the oracle        */
/* (cg_fragment_compiler.cpp: arithmetic null-propagating :1440-1540,  */
/*  relational non-canonical :1601-1720, logical Kleene :1547-1599)    */

struct ColCtx {
    const DevSeg* segs;        /* all columns' segments, concatenated */
    const SegEx* segex;
    const int32_t* col_seg_off;   /* per column: first segment index */
    const int32_t* col_seg_cnt;
    int64_t row;                  /* chunk row */
    uint32_t error;               /* YT_ERR_* */
    /* equi-join state: jrow_for caches which row the probe resolved.
     * jt = join item 0 (may have duplicate keys — the cross-product
     * machinery binds c.jrow per match); jt2 = item 1 (unique keys). */
    const JoinDev* jt = nullptr;
    int64_t jrow = -1;
    int64_t jrow_for = -1;
    const JoinDev* jt2 = nullptr;
    int64_t jrow2 = -1;
    int64_t jrow2_for = -1;
};

__device__ int64_t join_resolve(const DevPlan& p, ColCtx& c);
__device__ int64_t join_resolve2(const DevPlan& p, ColCtx& c);
__device__ DVal jforeign_at(const JoinDev& jt, int fcol, int shift,
                            int64_t frow, uint8_t vt);
__device__ DVal str_entry_at(const DevSeg& s, const SegEx& e, int64_t j, int seg);

__device__ DVal col_value(const DevPlan& p, ColCtx& c, int col)
{
    /* join item 1's columns sit ABOVE item 0's (primary_ncols of item 1 =
     * primary + item-0 values), so check it first */
    if (c.jt2 && c.jt2->active && col >= c.jt2->primary_ncols) {
        int slot = col - c.jt2->primary_ncols;
        int64_t frow = join_resolve2(p, c);
        if (frow < 0) {
            DVal v;
            v.type = p.col_types[col];
            v.null_ = 1;
            v.bits = 0;
            return v;
        }
        return jforeign_at(*c.jt2, c.jt2->fval_col[slot], c.jt2->f_shift[slot],
                           frow, p.col_types[col]);
    }
    if (c.jt && c.jt->active && col >= c.jt->primary_ncols) {
        int slot = col - c.jt->primary_ncols;
        int64_t frow = join_resolve(p, c);
        if (frow < 0) {
            DVal v;
            v.type = p.col_types[col];
            v.null_ = 1;
            v.bits = 0;
            return v;
        }
        return jforeign_at(*c.jt, c.jt->fval_col[slot], c.jt->f_shift[slot],
                           frow, p.col_types[col]);
    }
    int off = c.col_seg_off[col];
    int cnt = c.col_seg_cnt[col];
    int lo;
    if (p.col_uniform_shift[col]) {
        lo = (int)(c.row >> p.col_uniform_shift[col]);
    } else {
        /* binary search segment by start_row */
        int hi = cnt;
        lo = 0;
        while (lo + 1 < hi) {
            int mid = (lo + hi) / 2;
            if (c.segs[off + mid].start_row <= c.row) lo = mid;
            else hi = mid;
        }
    }
    const DevSeg& s = c.segs[off + lo];
    /* a STRING column has no 64-bit value: its entry stands for it */
    if (s.is_signed == 2)
        return str_entry_at(s, c.segex[off + lo], c.row - s.start_row, lo);
    return seg_value_at(s, c.segex[off + lo], c.row - s.start_row, p.col_types[col]);
}

/* fetch a FOREIGN chunk value (row, column index into the foreign chunk) */
__device__ DVal jforeign_at(const JoinDev& jt, int fcol, int shift,
                            int64_t frow, uint8_t vt)
{
    int off = jt.f_off[fcol];
    int cnt = jt.f_cnt[fcol];
    int lo;
    if (shift) {
        lo = (int)(frow >> shift);
    } else {
        int hi = cnt;
        lo = 0;
        while (lo + 1 < hi) {
            int mid = (lo + hi) / 2;
            if (jt.fsegs[off + mid].start_row <= frow) lo = mid;
            else hi = mid;
        }
    }
    const DevSeg& s = jt.fsegs[off + lo];
    return seg_value_at(s, jt.fsegex[off + lo], frow - s.start_row, vt);
}

__device__ DVal col_value(const DevPlan& p, ColCtx& c, int col);

/* resolve the join match for the current row (cached per row); returns the
 * foreign row index or -1. null primary keys join the null foreign key —
 * the reference eq-comparer treats null == null
 * (cg_fragment_compiler.cpp:425-447). */
__device__ int64_t join_resolve(const DevPlan& p, ColCtx& c)
{
    const JoinDev& jt = *c.jt;
    if (c.jrow_for == c.row) return c.jrow;
    c.jrow_for = c.row;
    c.jrow = -1;
    DVal k = col_value(p, c, jt.pkey_col);
    if (k.null_) {
        c.jrow = jt.null_row;
        return c.jrow;
    }
    if (jt.key_kind) {
        /* STRING key: k is its entry (str_entry_at), probed by k_strjoin_entries */
        c.jrow = jt.jmap[jt.jbase[k.bits >> 32] + (int64_t)(k.bits & 0xFFFFFFFFu)];
        return c.jrow;
    }
    uint64_t h = mix64(k.bits) & jt.hmask;
    for (;;) {
        int64_t r = jt.hrow[h];
        if (r < 0) break;
        if (jt.hkey[h] == k.bits) { c.jrow = jt.chead[h]; break; }
        h = (h + 1) & jt.hmask;
    }
    return c.jrow;
}

/* item-1 resolver: its key column may be one of item 0's appended values
 * (col_value recursion handles the chain; key col < jt2->primary_ncols so
 * it can never recurse back into item 1) */
__device__ int64_t join_resolve2(const DevPlan& p, ColCtx& c)
{
    const JoinDev& jt = *c.jt2;
    if (c.jrow2_for == c.row) return c.jrow2;
    c.jrow2_for = c.row;
    c.jrow2 = -1;
    DVal k = col_value(p, c, jt.pkey_col);
    if (k.null_) {
        c.jrow2 = jt.null_row;
        return c.jrow2;
    }
    if (jt.key_kind) {
        c.jrow2 = jt.jmap[jt.jbase[k.bits >> 32] + (int64_t)(k.bits & 0xFFFFFFFFu)];
        return c.jrow2;
    }
    uint64_t h = mix64(k.bits) & jt.hmask;
    for (;;) {
        int64_t r = jt.hrow[h];
        if (r < 0) break;
        if (jt.hkey[h] == k.bits) { c.jrow2 = jt.chead[h]; break; }
        h = (h + 1) & jt.hmask;
    }
    return c.jrow2;
}

/* INNER-join row gate: call once per row before evaluating expressions */
__device__ __forceinline__ bool join_row_ok(const DevPlan& p, ColCtx& c)
{
    if (c.jt && c.jt->active && !c.jt->is_left) {
        if (join_resolve(p, c) < 0) return false;
    }
    if (c.jt2 && c.jt2->active && !c.jt2->is_left) {
        if (join_resolve2(p, c) < 0) return false;
    }
    return true;
}

__device__ __forceinline__ uint64_t str_key_id(const DevSeg& sk, const SegEx& ek,
                                               int64_t j);

/* P_STR_PRED: the row's answer to one string predicate (common.h). The
 * predicate was evaluated once per ENTRY of the column's segments by
 * k_strpred_entries; a row looks its entry id up and reads one bit. Kept
 * out of line: inlined into eval_prog it cost k_topk_materialize 9 VGPRs and
 * one wave of occupancy; out of line every interpreter kernel keeps the
 * register count it had before this instruction existed. */
__device__ __noinline__ DVal str_pred_row(const DevPlan& p, const ColCtx& c, const PInst& in)
{
    const int off = c.col_seg_off[in.col];
    int lo;
    if (p.col_uniform_shift[in.col]) {
        lo = (int)(c.row >> p.col_uniform_shift[in.col]);
    } else {
        int hi = c.col_seg_cnt[in.col];
        lo = 0;
        while (lo + 1 < hi) {
            int mid = (lo + hi) / 2;
            if (c.segs[off + mid].start_row <= c.row) lo = mid;
            else hi = mid;
        }
    }
    const DevSeg& s = c.segs[off + lo];
    const uint64_t id = str_key_id(s, c.segex[off + lo], c.row - s.start_row);
    DVal v;
    v.type = YT_VT_BOOLEAN;
    v.null_ = 0;
    if (id == 0) {
        if (in.bits & kSpNullIsNull) { v.type = YT_VT_NULL; v.null_ = 1; v.bits = 0; }
        else v.bits = (in.bits & kSpNullRes) != 0;
    } else if (in.bits & kSpConst) {
        v.bits = (in.bits & kSpConstRes) != 0;
    } else {
        const int pi = (int)(in.bits & 0xFF);
        const uint64_t bit = (uint64_t)p.sp_base[pi][lo] * 64 + (id - 1);
        v.bits = (p.sp_bits[pi][bit >> 6] >> (bit & 63)) & 1;
    }
    return v;
}

/* The value col_value gives for a row of a STRING column: a reference to its
 * entry, (index of the segment in its column) << 32 | id - 1, or null. Only
 * a STRING-key join reads it (join_resolve: one jmap word per entry, filled by
 * k_strjoin_entries); expressions over string columns never compile to P_COL.
 * Out of line for the reason given at str_pred_row. */
__device__ __noinline__ DVal str_entry_at(const DevSeg& s, const SegEx& e, int64_t j,
                                          int seg)
{
    const uint64_t id = str_key_id(s, e, j);
    DVal v;
    v.type = YT_VT_STRING;
    v.null_ = id == 0;
    v.bits = id ? (((uint64_t)seg << 32) | (id - 1)) : 0;
    return v;
}

/* The code of a non-null STRING component of the composite group key
 * (StrKeyDev): ref is the row's entry as str_entry_at gives it, the code is
 * 1 + the string id of that entry (k_strkey_*). Out of line for the reason
 * given at str_pred_row. */
__device__ __noinline__ uint64_t strkey_code(const uint32_t* kmap, const int64_t* kbase,
                                             uint64_t ref)
{
    return 1 + (uint64_t)kmap[kbase[ref >> 32] + (int64_t)(ref & 0xFFFFFFFFu)];
}

/* P_STR_REF: the row's value of a projected STRING column, as a reference to
 * its entry (common.h). Out of line for the reason given at str_pred_row. */
__device__ __noinline__ DVal str_ref_row(const DevPlan& p, const ColCtx& c, const PInst& in)
{
    const int off = c.col_seg_off[in.col];
    int lo;
    if (p.col_uniform_shift[in.col]) {
        lo = (int)(c.row >> p.col_uniform_shift[in.col]);
    } else {
        int hi = c.col_seg_cnt[in.col];
        lo = 0;
        while (lo + 1 < hi) {
            int mid = (lo + hi) / 2;
            if (c.segs[off + mid].start_row <= c.row) lo = mid;
            else hi = mid;
        }
    }
    const DevSeg& s = c.segs[off + lo];
    const uint64_t id = str_key_id(s, c.segex[off + lo], c.row - s.start_row);
    DVal v;
    v.type = YT_VT_STRING;
    v.null_ = id == 0;
    v.bits = id ? (((uint64_t)(off + lo) << 32) | (id - 1)) : 0;
    return v;
}

/* P_IN_NUM: is the operand in the numeric IN set (common.h)? A mix64 probe
 * loop over the set's open-addressing table, like join_resolve's; a null
 * operand answers with the list's null flag. The result is never null. Out
 * of line for the reason given at str_pred_row. */
__device__ __noinline__ void in_num_row(const DevPlan& p, const PInst& in, DVal& v)
{
    if (v.null_) {
        v.bits = (in.bits & kInNullRes) != 0;
    } else {
        const int si = (int)(in.bits & 0xFF);
        v.bits = (uint64_t)inlist_probe_u64(p.in_tab[si], p.in_mask[si],
                                            p.in_empty[si], v.bits);
    }
    v.type = YT_VT_BOOLEAN;
    v.null_ = 0;
}

__device__ DVal eval_prog(const DevPlan& p, ColCtx& c, int off, int len)
{
    /* the host refuses a program that needs more slots (compile_expr) */
    DVal stk[kEvalStack];
    int sp = 0;
    for (int i = 0; i < len; i++) {
        const PInst& in = p.prog[off + i];
        switch (in.op) {
        case P_COL:
            stk[sp++] = col_value(p, c, in.col);
            break;
        case P_LIT_I64:
        case P_LIT_U64: {
            DVal v; v.bits = in.bits; v.null_ = 0;
            v.type = in.op == P_LIT_I64 ? YT_VT_INT64 : YT_VT_UINT64;
            stk[sp++] = v;
            break;
        }
        case P_LIT_DOUBLE: {
            DVal v; v.bits = in.bits; v.type = YT_VT_DOUBLE; v.null_ = 0;
            stk[sp++] = v;
            break;
        }
        case P_LIT_NULL: {
            DVal v; v.bits = 0; v.type = YT_VT_NULL; v.null_ = 1;
            stk[sp++] = v;
            break;
        }
        case P_NOT: {
            DVal a = stk[--sp];
            if (!a.null_) { a.bits = !a.bits; a.type = YT_VT_BOOLEAN; }
            stk[sp++] = a;
            break;
        }
        case P_STR_PRED:
            stk[sp++] = str_pred_row(p, c, in);
            break;
        case P_STR_REF:
            stk[sp++] = str_ref_row(p, c, in);
            break;
        case P_IN_NUM:
            in_num_row(p, in, stk[sp - 1]);
            break;
        default: {
            DVal b = stk[--sp];
            DVal a = stk[--sp];
            DVal r; r.bits = 0; r.type = YT_VT_NULL; r.null_ = 1;
            if (in.op >= P_ADD && in.op <= P_MOD) {
                if (!a.null_ && !b.null_) {
                    if (a.type == YT_VT_DOUBLE) {
                        double x = __longlong_as_double(a.bits);
                        double y = __longlong_as_double(b.bits);
                        double z = 0;
                        switch (in.op) {
                        case P_ADD: z = x + y; break;
                        case P_SUB: z = x - y; break;
                        case P_MUL: z = x * y; break;
                        case P_DIV: z = x / y; break;
                        default: c.error = YT_ERR_UNSUPPORTED; break;
                        }
                        r.bits = __double_as_longlong(z);
                        r.type = YT_VT_DOUBLE; r.null_ = 0;
                    } else {
                        uint64_t x = a.bits, y = b.bits, z = 0;
                        int sgn = (a.type == YT_VT_INT64);
                        switch (in.op) {
                        case P_ADD: z = x + y; break;
                        case P_SUB: z = x - y; break;
                        case P_MUL: z = x * y; break;
                        case P_DIV:
                        case P_MOD:
                            if (y == 0) { c.error = YT_ERR_DIV_ZERO; }
                            else if (sgn) {
                                int64_t sx = (int64_t)x, sy = (int64_t)y;
                                if (sx == INT64_MIN && sy == -1) {
                                    z = (in.op == P_DIV) ? (uint64_t)INT64_MIN : 0;
                                } else {
                                    z = (uint64_t)((in.op == P_DIV) ? sx / sy : sx % sy);
                                }
                            } else {
                                z = (in.op == P_DIV) ? x / y : x % y;
                            }
                            break;
                        }
                        r.bits = z; r.type = a.type; r.null_ = 0;
                    }
                }
            } else if (in.op >= P_EQ && in.op <= P_GE) {
                int lt, eq;
                int force_true = 0;
                if (a.null_ || b.null_) {
                    unsigned ln = a.null_, rn = b.null_;
                    lt = rn < ln;
                    eq = ln == rn;
                } else if (a.type == YT_VT_DOUBLE) {
                    double x = __longlong_as_double(a.bits);
                    double y = __longlong_as_double(b.bits);
                    int unordered = (x != x) || (y != y);
                    lt = unordered || (x < y);
                    eq = unordered || (x == y);
                    force_true = unordered;   /* FCmpU*: NaN → true */
                } else if (a.type == YT_VT_INT64) {
                    int64_t x = (int64_t)a.bits, y = (int64_t)b.bits;
                    lt = x < y; eq = x == y;
                } else {
                    lt = a.bits < b.bits; eq = a.bits == b.bits;
                }
                int res = 1;
                if (!force_true) {
                    switch (in.op) {
                    case P_EQ: res = eq; break;
                    case P_NE: res = !eq; break;
                    case P_LT: res = lt; break;
                    case P_LE: res = lt || eq; break;
                    case P_GT: res = !(lt || eq); break;
                    case P_GE: res = !lt; break;
                    }
                }
                r.bits = (uint64_t)res; r.type = YT_VT_BOOLEAN; r.null_ = 0;
            } else if (in.op == P_AND || in.op == P_OR) {
                int an = a.null_, bn = b.null_;
                int av = an ? 0 : (a.bits != 0), bv = bn ? 0 : (b.bits != 0);
                if (in.op == P_AND) {
                    if ((!an && !av) || (!bn && !bv)) { r.bits = 0; r.type = YT_VT_BOOLEAN; r.null_ = 0; }
                    else if (!an && !bn) { r.bits = 1; r.type = YT_VT_BOOLEAN; r.null_ = 0; }
                } else {
                    if ((!an && av) || (!bn && bv)) { r.bits = 1; r.type = YT_VT_BOOLEAN; r.null_ = 0; }
                    else if (!an && !bn) { r.bits = 0; r.type = YT_VT_BOOLEAN; r.null_ = 0; }
                }
            } else {
                c.error = YT_ERR_UNSUPPORTED;
            }
            stk[sp++] = r;
            break;
        }
        }
    }
    return stk[0];
}

/* ------------------------------------------------------------------ */
/* group table update                                                  */

/* order-preserving map to u64 with 0 as the min/max identity (the table is
 * zero-initialized; emptiness is distinguished by nonnull == 0):
 *   MAX: m(x) such that x < y  <=>  m(x) < m(y); store max m(x)
 *   MIN: store max of ~m(x) (order reversed)                            */
__device__ __forceinline__ uint64_t ord_map(uint64_t bits, uint8_t type)
{
    if (type == YT_VT_DOUBLE) {
        /* IEEE754 total-order map */
        return (bits & 0x8000000000000000ULL) ? ~bits : (bits | 0x8000000000000000ULL);
    }
    if (type == YT_VT_INT64) return bits ^ 0x8000000000000000ULL;
    return bits;   /* uint64 / boolean */
}

__device__ __forceinline__ uint64_t ord_unmap(uint64_t m, uint8_t type)
{
    if (type == YT_VT_DOUBLE)
        return (m & 0x8000000000000000ULL) ? (m & ~0x8000000000000000ULL)
                                           : ~m;
    if (type == YT_VT_INT64) return m ^ 0x8000000000000000ULL;
    return m;
}

__device__ __forceinline__ void agg_update_slot(unsigned long long* aggp,
                                                const DevPlan& p, int a,
                                                DVal v)
{
    /* aggp -> { bits, nonnull } for agg a; semantics udf/sum.c, min.c, max.c */
    if (v.null_) return;
    int f = p.agg_func[a];
    if (f == YT_AGG_SUM || f == YT_AGG_AVG) {
        /* avg state = {sum (arg-typed; int wraps, double fadd), count} —
         * builtin_function_profiler.cpp avg codegen; count rides the
         * nonnull word */
        if (v.type == YT_VT_DOUBLE) {
            atomicAdd((double*)aggp, __longlong_as_double(v.bits));
        } else {
            atomicAdd(aggp, (unsigned long long)v.bits);
        }
    } else if (f == YT_AGG_MAX) {
        atomicMax(aggp, (unsigned long long)ord_map(v.bits, v.type));
    } else if (f == YT_AGG_MIN) {
        atomicMax(aggp, (unsigned long long)~ord_map(v.bits, v.type));
    } else if (f == YT_AGG_FIRST) {
        /* FirstIteration (registry.cpp:3642-3663): keep the first non-null;
         * the CAS winner owns the bits word (read only after kernel end) */
        if (atomicCAS(aggp + 1, 0ULL, 1ULL) == 0ULL) aggp[0] = v.bits;
        return;
    }
    atomicAdd(aggp + 1, 1ULL);
}

/* group-row-limit mark (overflow = 2, incomplete output). It must never
 * replace a capacity mark (overflow = 1), on which the host discards the
 * table and re-runs: a plain store of 2 after a 1 would pass a partial
 * table off as a finished one. */
__device__ __forceinline__ void mark_group_limit(TableHdr* th)
{
    if (th->overflow == 0)
        atomicCAS((unsigned long long*)&th->overflow, 0ULL, 2ULL);
}

/* returns pointer to slot (stride u64s) for key, claiming if new; nullptr on
 * overflow. side groups handled by caller. */
__device__ unsigned long long* table_probe(TableHdr* th, unsigned long long* slots,
                                           int stride, uint64_t key_bits)
{
    uint64_t h = mix64(key_bits);
    uint64_t mask = th->mask;
    uint64_t s = h & mask;
    for (uint64_t iter = 0; iter <= mask; iter++) {
        unsigned long long* slot = slots + s * stride;
        /* relaxed agent-scope load first: on the hot path the group exists,
         * and a read is far cheaper than an RMW (probe measurement V5) */
        unsigned long long cur = __hip_atomic_load(slot, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
        if (cur == (unsigned long long)key_bits) return slot;
        if (cur != 0ULL) { s = (s + 1) & mask; continue; }
        unsigned long long old = atomicCAS(slot, 0ULL, (unsigned long long)key_bits);
        if (old == 0ULL) {
            unsigned long long ticket = atomicAdd(&th->ngroups, 1ULL);
            if (th->group_limit > 0 && (int64_t)ticket >= th->group_limit) {
                mark_group_limit(th);   /* group row limit — incomplete output */
            }
            return slot;
        }
        if (old == (unsigned long long)key_bits) return slot;
        s = (s + 1) & mask;
    }
    th->overflow = 1;
    return nullptr;
}

__device__ void table_update_generic(TableHdr* th, unsigned long long* slots,
                                     const DevPlan& p, DVal key, DVal* aggv)
{
    int stride = 2 + 2 * p.agg_count;
    unsigned long long* aggp;
    unsigned long long* cntp;
    if (key.null_ || key.bits == 0) {
        int side = key.null_ ? 1 : 0;
        th->side_used[side] = 1;
        cntp = (unsigned long long*)&th->side_cnt[side];
        aggp = (unsigned long long*)&th->side_agg[side][0];
    } else {
        unsigned long long* slot = table_probe(th, slots, stride, key.bits);
        if (!slot) return;
        cntp = slot + 1;
        aggp = slot + 2;
    }
    atomicAdd(cntp, 1ULL);
    for (int a = 0; a < p.agg_count; a++) {
        if (p.agg_func[a] != YT_AGG_SUM1) {
            agg_update_slot(aggp + 2 * a, p, a, aggv[a]);
        }
        /* YT_AGG_SUM1: cnt covers it */
    }
}

/* ------------------------------------------------------------------ */
/* versioned scan-format read-at-timestamp           */
/* One thread per row. Layout + semantics: include/ytql_gpu.h.          */

struct VVecRef {
    const uint64_t* data;
    uint32_t width;
    uint64_t size;
};

__device__ __forceinline__ VVecRef vvec_parse(const char** cursor)
{
    const uint64_t* p = (const uint64_t*)*cursor;
    VVecRef v;
    v.size = p[0] & ((1ULL << 56) - 1);
    v.width = (uint32_t)(p[0] >> 56);
    v.data = p + 1;
    *cursor += (1 + (((uint64_t)v.width * v.size + 63) >> 6)) * 8;
    return v;
}

__device__ __forceinline__ uint64_t vvec_get(const VVecRef& v, uint64_t i)
{
    if (v.width == 0) return 0;
    uint64_t mask = v.width >= 64 ? ~0ULL : ((1ULL << v.width) - 1);
    return bp_gl(v.data, mask, v.width, (int64_t)i);
}

__device__ __forceinline__ uint64_t vcum_dev(const VVecRef& diffs,
                                             uint32_t expected, int64_t i)
{
    if (i < 0) return 0;
    uint32_t zz = (uint32_t)vvec_get(diffs, i);
    int32_t diff = (int32_t)((zz >> 1) ^ (~(zz & 1) + 1));
    return (uint64_t)expected * (uint64_t)(i + 1) + (uint64_t)(int64_t)diff;
}

/* sparse value index: [vb,ve) = the contiguous run of values whose packed
 * row index equals r (column_writer_detail.cpp sparse branch emits row
 * indexes sorted ascending) */
__device__ __forceinline__ void vsparse_range(const VVecRef& ridx, int64_t r,
                                              uint64_t* vb, uint64_t* ve)
{
    uint64_t lo = 0, hi = ridx.size;
    while (lo < hi) {   /* first j with ridx[j] >= r */
        uint64_t mid = (lo + hi) >> 1;
        if ((int64_t)vvec_get(ridx, mid) < r) lo = mid + 1; else hi = mid;
    }
    *vb = lo;
    hi = ridx.size;
    while (lo < hi) {   /* first j with ridx[j] > r */
        uint64_t mid = (lo + hi) >> 1;
        if ((int64_t)vvec_get(ridx, mid) <= r) lo = mid + 1; else hi = mid;
    }
    *ve = lo;
}

__global__ void __launch_bounds__(256)
k_versioned_read(const VSegDev* segs, int nseg, int64_t total_rows,
                 uint64_t timestamp,
                 uint64_t* out_bits, uint8_t* out_null, uint8_t* out_vis,
                 uint8_t* out_agg)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < total_rows; g += stride) {
        int lo = 0, hi = nseg;
        while (lo + 1 < hi) {
            int mid = (lo + hi) / 2;
            if (segs[mid].row_start <= g) lo = mid;
            else hi = mid;
        }
        const VSegDev& S = segs[lo];
        int64_t r = g - S.row_start;

        const char* tp = S.ts_data;
        VVecRef dict = vvec_parse(&tp);
        VVecRef wids = vvec_parse(&tp);
        VVecRef dids = vvec_parse(&tp);
        VVecRef wdiffs = vvec_parse(&tp);
        VVecRef ddiffs = vvec_parse(&tp);
        const char* vp = S.val_data;
        const bool sparse = (S.vtype & 2) != 0;   /* *_SPARSE codes */
        const bool is_str = S.vtype >= YT_VSEG_STR_DIRECT_DENSE;
        const bool is_dbl = !is_str && S.vtype >= YT_VSEG_DOUBLE_DENSE;
        const bool is_dict = !is_dbl && !is_str && (S.vtype & 1) != 0;
        const bool is_sdict = is_str && (S.vtype & 1) != 0;
        VVecRef vindex = vvec_parse(&vp);         /* dense offsets | sparse row idx */
        VVecRef tsids = vvec_parse(&vp);
        const uint8_t* vaggbm = nullptr;
        if (S.vflags & YT_VSEG_F_AGGREGATE) {
            vaggbm = (const uint8_t*)vp;
            vp += ((tsids.size + 7) / 8 + 7) & ~(uint64_t)7;
        }
        VVecRef vvals = {};                       /* int direct values | dictionary */
        VVecRef vids = {};                        /* dictionary ids */
        const double* ddata = nullptr;
        const uint8_t* vnull = nullptr;
        const char* sdata = nullptr;              /* string / dict bytes */
        if (is_str) {
            /* string_column_writer.cpp layouts (see include/ytql_gpu.h):
             * direct = [END offsets diff][null bitmap][bytes];
             * dict   = [ids 0=null][dict END offsets diff][bytes] */
            if (is_sdict) {
                vids = vvec_parse(&vp);
                vvals = vvec_parse(&vp);          /* dictionary offsets */
                sdata = vp;
            } else {
                vvals = vvec_parse(&vp);          /* value END offsets */
                vnull = (const uint8_t*)vp;
                vp += ((vvals.size + 7) / 8 + 7) & ~(uint64_t)7;
                sdata = vp;
            }
        } else if (is_dbl) {
            uint64_t cnt = *(const uint64_t*)vp;
            ddata = (const double*)(vp + 8);
            vnull = (const uint8_t*)(vp + 8 + cnt * 8);
        } else if (is_dict) {
            vvals = vvec_parse(&vp);              /* dictionary (value - base) */
            vids = vvec_parse(&vp);               /* 0 = null, 1-based */
        } else {
            vvals = vvec_parse(&vp);
            vnull = (const uint8_t*)vp;
        }

        out_vis[g] = 0;
        out_null[g] = 1;
        out_bits[g] = 0;
        if (out_agg) out_agg[g] = 0;

        uint64_t wb = vcum_dev(wdiffs, S.exp_w, r - 1);
        uint64_t we = vcum_dev(wdiffs, S.exp_w, r);
        uint64_t db = vcum_dev(ddiffs, S.exp_d, r - 1);
        uint64_t de = vcum_dev(ddiffs, S.exp_d, r);

        uint64_t delete_ts = 0;
        for (uint64_t i = db; i < de; i++) {
            uint64_t ts = S.base_timestamp + vvec_get(dict, vvec_get(dids, i));
            if (ts <= timestamp) { delete_ts = ts; break; }
        }
        int64_t wcount = (int64_t)(we - wb);
        int64_t lower = wcount, upper = wcount;
        for (int64_t i = 0; i < wcount; i++) {
            uint64_t ts = S.base_timestamp + vvec_get(dict, vvec_get(wids, wb + i));
            if (lower == wcount && ts <= timestamp) lower = i;
            if (ts <= delete_ts) { upper = i; break; }
        }
        if (upper < lower) upper = lower;
        if (lower >= upper) continue;
        out_vis[g] = 1;

        uint64_t vb, ve;
        if (sparse) {
            vsparse_range(vindex, r, &vb, &ve);
        } else {
            vb = vcum_dev(vindex, S.exp_v, r - 1);
            ve = vcum_dev(vindex, S.exp_v, r);
        }
        for (uint64_t j = vb; j < ve; j++) {
            int64_t ti = (int64_t)vvec_get(tsids, j);
            if (ti < lower) continue;
            if (ti >= upper) break;
            int nul;
            uint64_t bits = 0;
            if (is_str) {
                /* bits = (byte offset within the value blob) << 24 | len */
                if (is_sdict) {
                    uint64_t id = vvec_get(vids, j);
                    nul = (id == 0);
                    if (!nul) {
                        uint64_t e2 = vcum_dev(vvals, (uint32_t)S.base_value,
                                               (int64_t)id - 1);
                        uint64_t b2 = vcum_dev(vvals, (uint32_t)S.base_value,
                                               (int64_t)id - 2);
                        bits = ((uint64_t)(sdata - S.val_data + b2) << 24)
                             | (e2 - b2);
                    }
                } else {
                    nul = (vnull[j / 8] >> (j % 8)) & 1;
                    if (!nul) {
                        uint64_t e2 = vcum_dev(vvals, (uint32_t)S.base_value,
                                               (int64_t)j);
                        uint64_t b2 = vcum_dev(vvals, (uint32_t)S.base_value,
                                               (int64_t)j - 1);
                        bits = ((uint64_t)(sdata - S.val_data + b2) << 24)
                             | (e2 - b2);
                    }
                }
            } else if (is_dict) {
                uint64_t id = vvec_get(vids, j);
                nul = (id == 0);
                if (!nul)
                    bits = (uint64_t)zz_dec(S.base_value + vvec_get(vvals, id - 1));
            } else {
                nul = (vnull[j / 8] >> (j % 8)) & 1;
                if (!nul) {
                    bits = is_dbl
                        ? ((const uint64_t*)ddata)[j]
                        : (uint64_t)zz_dec(S.base_value + vvec_get(vvals, j));
                }
            }
            if (!nul) {
                out_null[g] = 0;
                out_bits[g] = bits;
            }
            /* the aggregate flag belongs to the chosen value, null or not
             * (TVersionedColumnWriterBase::AddValues appends it per value) */
            if (out_agg && vaggbm)
                out_agg[g] = (vaggbm[j / 8] >> (j % 8)) & 1;
            break;
        }
    }
}

/* decode one unversioned DirectDense int64 column into per-row
 * (decoded bits, null) arrays — the key-column side of the versioned
 * table bridge (keys in the scan format are plain unversioned segments,
 * rowset_builder.cpp key readers) */
__global__ void __launch_bounds__(256)
k_unvcol_to_arrays(const DevSeg* segs, const SegEx* segex,
                   int seg_off, int seg_cnt, int64_t n,
                   uint64_t* out_bits, uint8_t* out_null,
                   unsigned* error_out)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < n; g += stride) {
        int lo = 0, hi = seg_cnt;
        while (lo + 1 < hi) {
            int mid = (lo + hi) / 2;
            if (segs[seg_off + mid].start_row <= g) lo = mid;
            else hi = mid;
        }
        const DevSeg& sg = segs[seg_off + lo];
        const SegEx& e = segex[seg_off + lo];
        if (sg.is_signed == 2) { *error_out = 1; return; }   /* string keys: not yet */
        int64_t r = g - sg.start_row;
        DVal v = seg_value_at(sg, e, r, YT_VT_INT64);
        out_null[g] = (uint8_t)v.null_;
        out_bits[g] = v.null_ ? 0 : v.bits;
    }
}

/* versioned → unversioned chunk bridge: compact the visible rows of a
 * read-at-timestamp into reference-layout DirectDense width-64 segments
 * (min_value = 0, values in zigzag space) that the query engine scans
 * directly. Stable two-pass block compaction (pass A per-block counts,
 * host scans the ≤4096 block sums, pass B scatters). */
__global__ void __launch_bounds__(256)
k_vis_count(const uint8_t* vis, int64_t n, unsigned long long* block_counts)
{
    __shared__ unsigned long long s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    int64_t per = (n + gridDim.x - 1) / gridDim.x;
    int64_t b0 = (int64_t)blockIdx.x * per;
    int64_t b1 = b0 + per > n ? n : b0 + per;
    unsigned long long c = 0;
    for (int64_t i = b0 + threadIdx.x; i < b1; i += blockDim.x)
        c += vis[i];
    #pragma unroll
    for (int d = 32; d; d >>= 1) c += __shfl_down(c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt;
}

__global__ void __launch_bounds__(256)
k_vis_scatter(const uint8_t* vis, const uint8_t* nulls, const uint64_t* bits,
              int64_t n, const unsigned long long* block_bases,
              uint64_t seg_rows_cap,
              const int64_t* seg_blob_off,   /* byte offset of each segment */
              char* out_blob, int is_double)
{
    __shared__ unsigned long long s_wcnt[16];
    __shared__ unsigned long long s_run;
    const int lane = threadIdx.x & 63;
    const int wid = (int)(threadIdx.x >> 6);
    const int nw = (int)(blockDim.x >> 6);

    int64_t per = (n + gridDim.x - 1) / gridDim.x;
    int64_t b0 = (int64_t)blockIdx.x * per;
    int64_t b1 = b0 + per > n ? n : b0 + per;
    if (threadIdx.x == 0) s_run = block_bases[blockIdx.x];
    __syncthreads();

    for (int64_t base = b0; base < b1; base += blockDim.x) {
        int64_t i = base + threadIdx.x;
        int v = (i < b1) ? vis[i] : 0;
        unsigned long long mask = __ballot(v != 0);
        unsigned long long run = v;
        #pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            unsigned long long x = __shfl_up(run, d, 64);
            if (lane >= d) run += x;
        }
        if (lane == 63) s_wcnt[wid] = run;
        __syncthreads();
        if (v) {
            unsigned long long woff = 0;
            for (int w = 0; w < wid; w++) woff += s_wcnt[w];
            uint64_t idx = s_run + woff + (run - v);
            uint64_t seg = idx / seg_rows_cap;
            uint64_t j = idx - seg * seg_rows_cap;
            char* sb = out_blob + seg_blob_off[seg];
            /* int64: [bitpack header][values w64 zigzag][null bitmap];
             * double: [u64 count][raw doubles][null bitmap] — identical
             * offsets, only the header/types differ (host writes them) */
            uint64_t stored;
            if (is_double) {
                stored = bits[i];
            } else {
                int64_t v64 = (int64_t)bits[i];
                stored = ((uint64_t)v64 << 1) ^ (uint64_t)(v64 >> 63);
            }
            ((uint64_t*)(sb + 8))[j] = nulls[i] ? 0 : stored;
            if (nulls[i]) {
                uint64_t rows_here = 0;   /* bitmap offset needs seg rows */
                (void)rows_here;
                /* bitmap starts after the per-segment value words; the host
                 * passes per-segment offsets so compute from the NEXT
                 * segment boundary: bitmap_off = 8 + seg_rows*8 where
                 * seg_rows = min(cap, total - seg*cap); the host encodes
                 * seg_rows in the header it wrote BEFORE this kernel runs */
                uint64_t hdr = *(const uint64_t*)sb;
                uint64_t rows = hdr & ((1ULL << 56) - 1);   /* both layouts */
                uint32_t* bm = (uint32_t*)(sb + 8 + rows * 8);
                atomicOr(&bm[j >> 5], 1u << (j & 31));
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int w = 0; w < nw; w++) s_run += s_wcnt[w];
        __syncthreads();
    }
}

/* ------------------------------------------------------------------ */
/* equi-join foreign-table build + unique-key verify                    */

__global__ void k_join_build(JoinDev jt, int64_t frows,
                             uint64_t* hkey, long long* hrow,
                             unsigned long long* null_row_plus1,
                             unsigned* error_out)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < frows; r += stride) {
        DVal k = jforeign_at(jt, jt.fkey_col, jt.fkey_shift, r, YT_VT_INT64);
        if (k.null_) {
            /* null-key rows chain off null_row (null joins null) */
            unsigned long long prev = atomicExch(null_row_plus1,
                                                 (unsigned long long)(r + 1));
            ((int64_t*)jt.fnext)[r] = (int64_t)prev - 1;
            if (prev != 0ULL) atomicOr(error_out + 1, 1u);   /* has_dups */
            continue;
        }
        uint64_t h = mix64(k.bits) & jt.hmask;
        for (;;) {
            unsigned long long prev = atomicCAS(
                (unsigned long long*)&hrow[h],
                (unsigned long long)(long long)-1,
                (unsigned long long)r);
            if (prev == (unsigned long long)(long long)-1) {
                hkey[h] = k.bits;
                break;
            }
            h = (h + 1) & jt.hmask;
        }
    }
}

/* all inserts are visible now: push every row onto the match list of its
 * key's CANONICAL slot (first matching slot in probe order — duplicate
 * keys may have claimed later slots too; those stay as tombstones that
 * only lengthen probes). error_out[1] = has_dups. */
__global__ void k_join_chain(JoinDev jt, int64_t frows, unsigned* error_out)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < frows; r += stride) {
        DVal k = jforeign_at(jt, jt.fkey_col, jt.fkey_shift, r, YT_VT_INT64);
        if (k.null_) continue;
        uint64_t h = mix64(k.bits) & jt.hmask;
        for (;;) {
            int64_t rr = jt.hrow[h];
            if (rr < 0) break;                        /* unreachable */
            if (jt.hkey[h] == k.bits) {
                int64_t prev = (int64_t)atomicExch(
                    (unsigned long long*)&((int64_t*)jt.chead)[h],
                    (unsigned long long)r);
                ((int64_t*)jt.fnext)[r] = prev;
                if (prev >= 0) atomicOr(error_out + 1, 1u);   /* has_dups */
                break;
            }
            h = (h + 1) & jt.hmask;
        }
    }
}

/* ------------------------------------------------------------------ */
/* generic fused scan (any segment types / expressions)                */

__global__ void __launch_bounds__(256)
k_scan_generic(DevPlan p, const DevSeg* segs, const SegEx* segex,
               const int32_t* col_seg_off, const int32_t* col_seg_cnt,
               int64_t row_count, JoinDev jd, JoinDev jd2,
               TableHdr* th, unsigned long long* slots,
               unsigned* error_out, StrKeyDev sk)
{
    ColCtx c;
    c.segs = segs;
    c.segex = segex;
    c.col_seg_off = col_seg_off;
    c.col_seg_cnt = col_seg_cnt;
    c.error = 0;
    c.jt = &jd;
    c.jt2 = jd2.active ? &jd2 : nullptr;

    DVal aggv[kMaxAggs];

    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < row_count; r += stride) {
        c.row = r;
        /* duplicate foreign keys: one pass per match in the key's chain
         * (registry.cpp MultiJoinOpHelper cross-product); unjoined plans
         * and unique keys run the single pass they always did */
        const bool joined = jd.active != 0;
        int64_t m = -1;
        if (joined) {
            m = join_resolve(p, c);
            if (m < 0 && !jd.is_left) continue;
        }
        for (;;) {
        if (joined) { c.jrow = m; c.jrow_for = r; c.jrow2_for = -9; }
        bool pass = true;
        /* INNER gate for join item 1 (its key may depend on item 0's match,
         * so it re-resolves per match pass) */
        if (c.jt2 && c.jt2->active && !c.jt2->is_left &&
            join_resolve2(p, c) < 0)
            pass = false;
        if (pass && p.filter_len) {
            DVal f = eval_prog(p, c, p.filter_off, p.filter_len);
            if (f.null_ || f.bits == 0) pass = false;
        }
        if (pass) {
        DVal key;
        if (p.kp_count) {
            /* composite packed key (see DevPlan kp_*) */
            uint64_t kb = 0;
            for (int i = 0; i < p.kp_count; i++) {
                DVal v = col_value(p, c, p.kp_col[i]);
                uint64_t enc = 0;
                if (!v.null_ && v.type == YT_VT_STRING) {
                    enc = strkey_code(sk.kmap[i], sk.kbase[i], v.bits);
                } else if (!v.null_) {
                    uint64_t z = p.kp_signed[i]
                        ? (((uint64_t)v.bits << 1)
                           ^ (uint64_t)(((int64_t)v.bits) >> 63))
                        : v.bits;
                    enc = 1 + (z - p.kp_base[i]);
                }
                kb |= enc << p.kp_shift[i];
            }
            key.bits = kb;
            key.type = YT_VT_UINT64;
            key.null_ = 0;
        } else if (p.key_len) {
            key = eval_prog(p, c, p.key_off, p.key_len);
        } else {
            key.bits = 1; key.type = YT_VT_INT64; key.null_ = 0;  /* single group, side-stepped below */
        }
        for (int a = 0; a < p.agg_count; a++) {
            if (p.agg_func[a] != YT_AGG_SUM1) {
                aggv[a] = eval_prog(p, c, p.agg_off[a], p.agg_len[a]);
            }
        }
        if (c.error) { atomicMax(error_out, c.error); return; }
        table_update_generic(th, slots, p, key, aggv);
        }   /* pass */
        if (!joined || m < 0) break;
        m = jd.fnext[m];
        if (m < 0) break;
        }   /* match loop */
    }
    if (c.error) atomicMax(error_out, c.error);
}

/* scan + filter + project (no aggregation): preserves input row order —
 * MakeCodegenProjectOp + WriteOpHelper semantics (registry.cpp:1999-2047)
 * with row-at-a-time evaluation replaced by one thread per row. Rows that
 * fail the filter leave pass[j] = 0; the host compacts in row order. */
__global__ void __launch_bounds__(256)
k_scan_project(DevPlan p, const DevSeg* segs, const SegEx* segex,
               const int32_t* col_seg_off, const int32_t* col_seg_cnt,
               int64_t row_base, int64_t row_count,
               JoinDev jd, JoinDev jd2,
               DevOutVal* out, uint8_t* pass, unsigned* error_out)
{
    /* [row_base, row_base+row_count) window: out/pass are window-local so
     * the host can STREAM arbitrarily large scans through a bounded
     * materialization buffer */
    ColCtx c;
    c.segs = segs;
    c.segex = segex;
    c.col_seg_off = col_seg_off;
    c.col_seg_cnt = col_seg_cnt;
    c.error = 0;
    c.jt = &jd;
    c.jt2 = jd2.active ? &jd2 : nullptr;

    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < row_count; r += stride) {
        c.row = row_base + r;
        pass[r] = 0;
        if (!join_row_ok(p, c)) continue;
        if (p.filter_len) {
            DVal f = eval_prog(p, c, p.filter_off, p.filter_len);
            if (f.null_ || f.bits == 0) continue;
        }
        pass[r] = 1;
        for (int pj = 0; pj < p.proj_count; pj++) {
            DVal v = eval_prog(p, c, p.proj_off[pj], p.proj_len[pj]);
            DevOutVal o;
            o.bits = v.bits;
            o.type = v.null_ ? YT_VT_NULL : v.type;
            o.pad_ = 0;
            out[r * p.proj_count + pj] = o;
        }
        if (c.error) { atomicMax(error_out, c.error); return; }
    }
    if (c.error) atomicMax(error_out, c.error);
}

/* ------------------------------------------------------------------ */
/* ORDER BY ... LIMIT: histogram k-selection over an order-isomorphic  */
/* u64 key mapping (TTopCollector semantics; the host drives the digit */
/* refinement and finishes with the exact comparer on ≤cap candidates) */

/* map a value to u64 preserving the reference comparer order
 * (cg_fragment_compiler.cpp:400-530): int64 signed, uint64/boolean
 * unsigned, double by value (NaN -> error), null handled by caller */
__device__ __forceinline__ bool topk_map(const DVal& v, int desc,
                                         uint64_t* mk, unsigned* error_out)
{
    uint64_t m;
    switch (v.type) {
    case YT_VT_INT64:
        m = v.bits ^ 0x8000000000000000ULL;
        break;
    case YT_VT_UINT64:
    case YT_VT_BOOLEAN:
        m = v.bits;
        break;
    case YT_VT_DOUBLE: {
        double d = __longlong_as_double((long long)v.bits);
        if (isnan(d)) { atomicMax(error_out, 100u); return false; }
        m = (v.bits >> 63) ? ~v.bits : (v.bits | 0x8000000000000000ULL);
        break;
    }
    default:
        atomicMax(error_out, (unsigned)YT_ERR_UNSUPPORTED);
        return false;
    }
    *mk = desc ? ~m : m;
    return true;
}

__global__ void __launch_bounds__(256)
k_topk_hist(DevPlan p, const DevSeg* segs, const SegEx* segex,
            const int32_t* col_seg_off, const int32_t* col_seg_cnt,
            int64_t row_count, JoinDev jd, JoinDev jd2, TopkPass tp,
            unsigned long long* bins,           /* 2048 */
            unsigned long long* misc,           /* null_cnt, mmin, mmax */
            unsigned* error_out)
{
    __shared__ unsigned lh[2048];
    for (int i = threadIdx.x; i < 2048; i += blockDim.x) lh[i] = 0;
    __syncthreads();

    ColCtx c;
    c.segs = segs;
    c.segex = segex;
    c.col_seg_off = col_seg_off;
    c.col_seg_cnt = col_seg_cnt;
    c.error = 0;
    c.jt = &jd;
    c.jt2 = jd2.active ? &jd2 : nullptr;
    unsigned long long nulls = 0;
    uint64_t mmin = ~0ULL, mmax = 0;

    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < row_count; r += stride) {
        c.row = r;
        if (!join_row_ok(p, c)) continue;
        if (p.filter_len) {
            DVal f = eval_prog(p, c, p.filter_off, p.filter_len);
            if (f.null_ || f.bits == 0) continue;
        }
        DVal v = eval_prog(p, c, p.proj_off[tp.order_proj],
                           p.proj_len[tp.order_proj]);
        if (c.error) break;
        if (v.null_) { nulls++; continue; }
        uint64_t m;
        if (!topk_map(v, tp.desc, &m, error_out)) continue;
        if (tp.level0) {
            if (m < mmin) mmin = m;
            if (m > mmax) mmax = m;
        }
        if (m < tp.lo || m > tp.hi) continue;
        atomicAdd(&lh[(m - tp.lo) >> tp.shift], 1u);
    }
    if (c.error) atomicMax(error_out, c.error);
    __syncthreads();
    for (int i = threadIdx.x; i < 2048; i += blockDim.x) {
        if (lh[i]) atomicAdd(&bins[i], (unsigned long long)lh[i]);
    }
    if (tp.level0) {
        if (nulls) atomicAdd(&misc[0], nulls);
        if (mmin != ~0ULL) atomicMin(&misc[1], mmin);
        if (mmax || mmin != ~0ULL) atomicMax(&misc[2], mmax);
    }
}

__global__ void __launch_bounds__(256)
k_topk_gather(DevPlan p, const DevSeg* segs, const SegEx* segex,
              const int32_t* col_seg_off, const int32_t* col_seg_cnt,
              int64_t row_count, JoinDev jd, JoinDev jd2, TopkGather tg,
              int64_t* rows_strict, unsigned long long* ctr_strict,
              int64_t* rows_tie, unsigned long long* ctr_tie,
              int64_t* rows_null, unsigned long long* ctr_null,
              unsigned* error_out)
{
    ColCtx c;
    c.segs = segs;
    c.segex = segex;
    c.col_seg_off = col_seg_off;
    c.col_seg_cnt = col_seg_cnt;
    c.error = 0;
    c.jt = &jd;
    c.jt2 = jd2.active ? &jd2 : nullptr;

    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < row_count; r += stride) {
        c.row = r;
        if (!join_row_ok(p, c)) continue;
        if (p.filter_len) {
            DVal f = eval_prog(p, c, p.filter_off, p.filter_len);
            if (f.null_ || f.bits == 0) continue;
        }
        DVal v = eval_prog(p, c, p.proj_off[tg.order_proj],
                           p.proj_len[tg.order_proj]);
        if (c.error) break;
        if (v.null_) {
            unsigned long long j = atomicAdd(ctr_null, 1ULL);
            if ((int64_t)j < tg.cap_null) rows_null[j] = r;
            continue;
        }
        uint64_t m;
        if (!topk_map(v, tg.desc, &m, error_out)) continue;
        if (tg.all_nonnull || m < tg.lo) {
            unsigned long long j = atomicAdd(ctr_strict, 1ULL);
            if ((int64_t)j < tg.cap_strict) rows_strict[j] = r;
        } else if (m <= tg.hi) {
            unsigned long long j = atomicAdd(ctr_tie, 1ULL);
            if ((int64_t)j < tg.cap_tie) rows_tie[j] = r;
        }
    }
    if (c.error) atomicMax(error_out, c.error);
}

/* fast selection passes for the common shape: no filter, no join, order key
 * = a plain DirectDense int64/uint64 column with uniform segmentation. The
 * generic pass pays interpreter + one dependent load chain per row-thread
 * (~570 GB/s); here each thread keeps 4 strided rows in flight. */
__device__ __forceinline__ uint64_t topk_map_int(uint64_t raw, int is_signed,
                                                 int desc)
{
    uint64_t m = is_signed
        ? ((uint64_t)zz_dec(raw) ^ 0x8000000000000000ULL) : raw;
    return desc ? ~m : m;
}

__global__ void __launch_bounds__(256)
k_topk_hist_fast(const DevSeg* segs, const SegEx* segex, int seg_off,
                 int shift, int64_t row_count, int has_nulls, int is_signed,
                 TopkPass tp, unsigned long long* bins,
                 unsigned long long* misc)
{
    __shared__ unsigned lh[2048];
    for (int i = threadIdx.x; i < 2048; i += blockDim.x) lh[i] = 0;
    __syncthreads();
    unsigned long long nulls = 0;
    uint64_t mmin = ~0ULL, mmax = 0;

    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t base = tid0; base < row_count; base += 4 * stride) {
        #pragma unroll
        for (int u = 0; u < 4; u++) {
            int64_t r = base + (int64_t)u * stride;
            if (r >= row_count) break;
            int seg = (int)(r >> shift);
            const DevSeg& sg = segs[seg_off + seg];
            const SegEx& e = segex[seg_off + seg];
            int64_t j = r - sg.start_row;
            if (has_nulls &&
                bm_get((const uint8_t*)sg.blob + e.off_bitmap_bytes, j)) {
                nulls++;
                continue;
            }
            uint32_t w = e.w_values;
            uint64_t mask = (w >= 64) ? ~0ULL : ((1ULL << w) - 1);
            uint64_t raw = sg.min_value
                + bp_gl(sg.blob + e.off_values_words, mask, w, j);
            uint64_t m = topk_map_int(raw, is_signed, tp.desc);
            if (tp.level0) {
                if (m < mmin) mmin = m;
                if (m > mmax) mmax = m;
            }
            if (m < tp.lo || m > tp.hi) continue;
            atomicAdd(&lh[(m - tp.lo) >> tp.shift], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2048; i += blockDim.x) {
        if (lh[i]) atomicAdd(&bins[i], (unsigned long long)lh[i]);
    }
    if (tp.level0) {
        if (nulls) atomicAdd(&misc[0], nulls);
        if (mmin != ~0ULL) atomicMin(&misc[1], mmin);
        if (mmax || mmin != ~0ULL) atomicMax(&misc[2], mmax);
    }
}

__global__ void __launch_bounds__(256)
k_topk_gather_fast(const DevSeg* segs, const SegEx* segex, int seg_off,
                   int shift, int64_t row_count, int has_nulls, int is_signed,
                   TopkGather tg,
                   int64_t* rows_strict, unsigned long long* ctr_strict,
                   int64_t* rows_tie, unsigned long long* ctr_tie,
                   int64_t* rows_null, unsigned long long* ctr_null)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t base = tid0; base < row_count; base += 4 * stride) {
        #pragma unroll
        for (int u = 0; u < 4; u++) {
            int64_t r = base + (int64_t)u * stride;
            if (r >= row_count) break;
            int seg = (int)(r >> shift);
            const DevSeg& sg = segs[seg_off + seg];
            const SegEx& e = segex[seg_off + seg];
            int64_t j = r - sg.start_row;
            if (has_nulls &&
                bm_get((const uint8_t*)sg.blob + e.off_bitmap_bytes, j)) {
                unsigned long long q = atomicAdd(ctr_null, 1ULL);
                if ((int64_t)q < tg.cap_null) rows_null[q] = r;
                continue;
            }
            uint32_t w = e.w_values;
            uint64_t mask = (w >= 64) ? ~0ULL : ((1ULL << w) - 1);
            uint64_t raw = sg.min_value
                + bp_gl(sg.blob + e.off_values_words, mask, w, j);
            uint64_t m = topk_map_int(raw, is_signed, tg.desc);
            if (tg.all_nonnull || m < tg.lo) {
                unsigned long long q = atomicAdd(ctr_strict, 1ULL);
                if ((int64_t)q < tg.cap_strict) rows_strict[q] = r;
            } else if (m <= tg.hi) {
                unsigned long long q = atomicAdd(ctr_tie, 1ULL);
                if ((int64_t)q < tg.cap_tie) rows_tie[q] = r;
            }
        }
    }
}

/* decode the full projected row for each selected chunk row */
__global__ void __launch_bounds__(256)
k_topk_materialize(DevPlan p, const DevSeg* segs, const SegEx* segex,
                   const int32_t* col_seg_off, const int32_t* col_seg_cnt,
                   JoinDev jd, JoinDev jd2, const int64_t* rows, int64_t m, DevOutVal* out,
                   unsigned* error_out)
{
    ColCtx c;
    c.segs = segs;
    c.segex = segex;
    c.col_seg_off = col_seg_off;
    c.col_seg_cnt = col_seg_cnt;
    c.error = 0;
    c.jt = &jd;
    c.jt2 = jd2.active ? &jd2 : nullptr;

    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < m; i += stride) {
        c.row = rows[i];
        for (int pj = 0; pj < p.proj_count; pj++) {
            DVal v = eval_prog(p, c, p.proj_off[pj], p.proj_len[pj]);
            DevOutVal o;
            o.bits = v.bits;
            o.type = v.null_ ? YT_VT_NULL : v.type;
            o.pad_ = 0;
            out[i * p.proj_count + pj] = o;
        }
        if (c.error) break;
    }
    if (c.error) atomicMax(error_out, c.error);
}

/* ------------------------------------------------------------------ */
/* fast fused kernel — DirectDense segments, direct-column shapes      */
/*                                                                     */
/* One workgroup (256 threads) per tile of `tile_rows` rows inside one */
/* segment. Packed words of every used column + null bitmaps staged in */
/* LDS via coalesced loads; per-thread strided extraction; aggregation */
/* either into registers (global aggregate: wave shfl-reduce → LDS →   */
/* one atomic per WG) or the shared table (group by).                  */

/* global accumulators for the no-key path:
 * [0] = row count (pass filter), [1 + 2a], [2 + 2a] = sum bits / nonnull */
__global__ void __launch_bounds__(256)
k_scan_fast(FastParams fp, const DevSeg* segs, const SegEx* segex,
            const FastCol* cols,
            TableHdr* th, unsigned long long* slots,
            unsigned long long* gaccum)
{
    /* No LDS staging: every value is decoded straight from global memory
     * with a branchless two-word funnel; the L1/L2 absorb the window
     * overlap between lanes and the unrolled row loop supplies enough
     * loads in flight to reach streaming bandwidth (a staged-LDS version
     * of this loop measured 83% WAIT_ANY — phases serialized).
     * Canonical column slots: 0 = filter, 1..4 = sum args, 5 = key. */
    __shared__ uint64_t red[64];
    const int tid = threadIdx.x;
    const bool has_filter = fp.filter_idx >= 0;
    const bool has_key = fp.key_idx >= 0;

    uint64_t acc_sum[kMaxAggs] = {0, 0, 0, 0};
    uint64_t acc_nn[kMaxAggs] = {0, 0, 0, 0};
    uint64_t acc_cnt = 0;

    for (int tile = blockIdx.x; tile < fp.ntiles; tile += gridDim.x) {
        const int seg_idx = tile / fp.tiles_per_seg;
        const int tile_in_seg = tile % fp.tiles_per_seg;
        const int64_t t0 = (int64_t)tile_in_seg * fp.tile_rows;
        const int32_t seg_rows = segs[cols[1].seg_off + seg_idx].row_count;
        int64_t t1 = t0 + fp.tile_rows;
        if (t1 > seg_rows) t1 = seg_rows;

        /* per-tile uniform column state, all constant-indexed */
        const uint64_t* fwords = nullptr;
        const uint8_t* fbm = nullptr;
        uint32_t fwd = 0;
        uint64_t fmask = 0, fmin = 0;
        if (has_filter) {
            const DevSeg& sg = segs[cols[0].seg_off + seg_idx];
            const SegEx& e = segex[cols[0].seg_off + seg_idx];
            fwords = sg.blob + e.off_values_words;
            fwd = e.w_values;
            fmask = (fwd >= 64) ? ~0ULL : ((1ULL << fwd) - 1);
            fmin = sg.min_value;
            if ((fp.stage_bm_mask >> 0) & 1)
                fbm = (const uint8_t*)sg.blob + e.off_bitmap_bytes;
        }
        const uint64_t* swords_[4] = {nullptr, nullptr, nullptr, nullptr};
        const uint8_t* sbm_[4] = {nullptr, nullptr, nullptr, nullptr};
        uint32_t swd_[4] = {0, 0, 0, 0};
        uint64_t smask_[4] = {0, 0, 0, 0};
        uint64_t smin_[4] = {0, 0, 0, 0};
        #pragma unroll
        for (int a = 0; a < kMaxAggs; a++) {
            if (a >= fp.nsum) break;
            const DevSeg& sg = segs[cols[1 + a].seg_off + seg_idx];
            const SegEx& e = segex[cols[1 + a].seg_off + seg_idx];
            swords_[a] = sg.blob + e.off_values_words;
            swd_[a] = e.w_values;
            smask_[a] = (swd_[a] >= 64) ? ~0ULL : ((1ULL << swd_[a]) - 1);
            smin_[a] = sg.min_value;
            if ((fp.stage_bm_mask >> (1 + a)) & 1)
                sbm_[a] = (const uint8_t*)sg.blob + e.off_bitmap_bytes;
        }
        const uint64_t* kwords = nullptr;
        const uint8_t* kbm = nullptr;
        uint32_t kwd = 0;
        uint64_t kmask = 0, kmin = 0;
        if (has_key) {
            const DevSeg& sg = segs[cols[5].seg_off + seg_idx];
            const SegEx& e = segex[cols[5].seg_off + seg_idx];
            kwords = sg.blob + e.off_values_words;
            kwd = e.w_values;
            kmask = (kwd >= 64) ? ~0ULL : ((1ULL << kwd) - 1);
            kmin = sg.min_value;
            if ((fp.stage_bm_mask >> 5) & 1)
                kbm = (const uint8_t*)sg.blob + e.off_bitmap_bytes;
        }

        const int R = (fp.tile_rows + 255) / 256;
        #pragma unroll 4
        for (int i = 0; i < R; i++) {
            int64_t j = t0 + (int64_t)i * 256 + tid;
            if (j >= t1) continue;

            if (has_filter) {
                if (fbm && bm_get(fbm, j)) continue;
                int64_t v = zz_dec(fmin + bp_gl(fwords, fmask, fwd, j));
                if (v < fp.filter_lo || v > fp.filter_hi) continue;
            }

            if (!has_key) {
                acc_cnt++;
                #pragma unroll
                for (int a = 0; a < kMaxAggs; a++) {
                    if (a >= fp.nsum) break;
                    if (sbm_[a] && bm_get(sbm_[a], j)) continue;
                    acc_sum[a] += (uint64_t)zz_dec(smin_[a] + bp_gl(swords_[a], smask_[a], swd_[a], j));
                    acc_nn[a]++;
                }
            } else {
                DVal key;
                if (kbm && bm_get(kbm, j)) {
                    key.null_ = 1; key.bits = 0; key.type = YT_VT_INT64;
                } else {
                    key.bits = (uint64_t)zz_dec(kmin + bp_gl(kwords, kmask, kwd, j));
                    key.null_ = 0; key.type = YT_VT_INT64;
                }
                unsigned long long* cntp;
                unsigned long long* aggp;
                int stride = 2 + 2 * fp.agg_count;
                if (key.null_ || key.bits == 0) {
                    int side = key.null_ ? 1 : 0;
                    th->side_used[side] = 1;
                    cntp = (unsigned long long*)&th->side_cnt[side];
                    aggp = (unsigned long long*)&th->side_agg[side][0];
                } else {
                    unsigned long long* slot = table_probe(th, slots, stride, key.bits);
                    if (!slot) continue;
                    cntp = slot + 1;
                    aggp = slot + 2;
                }
                atomicAdd(cntp, 1ULL);
                #pragma unroll
                for (int a = 0; a < kMaxAggs; a++) {
                    if (a >= fp.nsum) break;
                    if (sbm_[a] && bm_get(sbm_[a], j)) continue;
                    uint64_t v = (uint64_t)zz_dec(smin_[a] + bp_gl(swords_[a], smask_[a], swd_[a], j));
                    unsigned long long* ap = aggp + 2 * fp.sum_slot[a];
                    atomicAdd(ap, (unsigned long long)v);
                    atomicAdd(ap + 1, 1ULL);
                }
            }
        }
    }

    /* one block-level reduction + one set of atomics per WORKGROUP (not per
     * tile): accumulators persist across the block's tiles */
    if (!has_key) {
        const int lane = tid & 63;
        const int wave = tid >> 6;
        for (int a = 0; a < 2 * fp.nsum + 1; a++) {
            uint64_t v = (a == 0) ? acc_cnt
                       : (a & 1) ? acc_sum[a >> 1]
                                 : acc_nn[(a >> 1) - 1];
            for (int sh = 32; sh >= 1; sh >>= 1) {
                v += (uint64_t)__shfl_down((long long)v, sh, 64);
            }
            if (lane == 0) red[wave * 16 + a] = v;
        }
        __syncthreads();
        if (tid == 0) {
            for (int a = 0; a < 2 * fp.nsum + 1; a++) {
                uint64_t v = red[a] + red[16 + a] + red[32 + a] + red[48 + a];
                if (a == 0) {
                    atomicAdd(&gaccum[0], (unsigned long long)v);
                } else if (a & 1) {
                    int slot = fp.sum_slot[a >> 1];
                    atomicAdd(&gaccum[1 + 2 * slot], (unsigned long long)v);
                } else {
                    int slot = fp.sum_slot[(a >> 1) - 1];
                    atomicAdd(&gaccum[2 + 2 * slot], (unsigned long long)v);
                }
            }
        }
    }
}


/* ------------------------------------------------------------------ */
/* two-phase partitioned group-by (see common.h PartParams)            */

__device__ __forceinline__ uint64_t zz_enc64(int64_t v)
{
    return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63);
}

/* per-row state word of k_scan_partition: bucket in bits 0..9, rank within
 * the tile's bucket run in bits 10..23, class in the top bits */
constexpr unsigned kRowInvalid = 0xFFFFFFFFu;   /* masked, filtered out, or done */
constexpr unsigned kRowSide = 0x80000000u;      /* | side (bit 0) | val_null << 1 */
constexpr unsigned kRowNullVal = 0x40000000u;   /* goes to the null-value stream */

/* The plain decode of k_scan_partition: packed records, direct span, a value
 * column, no filter, no nulls, key fields of at most 32 bits and no
 * INT64_MIN key in the column (PartParams::plain_mode). Nothing is tested per
 * row: rb[i] is the row's bucket, or kRowInvalid past the tile's end.
 *   - A field is cut from a window of dwords that starts at the dword
 *     holding its first bit: two adjacent dwords (one LDS read with two
 *     offsets, 4-byte aligned) for a field of up to 32 bits, three for a
 *     value of 33..64 bits (WIDE), then v_alignbit by the bit's low five
 *     bits and one mask. The window is not clamped: its last dword may lie
 *     one dword past the staged words. That dword is still inside the
 *     workgroup's LDS (the key's words are followed by the value's, the
 *     scratch by the histograms) and every bit it brings is masked away.
 *   - The key stays in 32 bits: the tile's kmin - gmin_k is added to the raw
 *     field (mod 2^32; the column's span is below 2^22) and the bucket is a
 *     32-bit shift. The value gets the tile's vmin - gmin_v in 64 bits.
 *   - A thread's row i lies 512 w bits behind its row i - 1, so positions
 *     advance by addition; a position past the tile's last row is held at
 *     that row, as the general decode holds the row index.
 *   - The LDS reads of eight rows are issued before the first use. */
template <bool WIDE, int R>
__device__ __forceinline__ void part_decode_plain(const uint32_t* sk, const uint32_t* sv,
        uint32_t kwd, uint32_t vwd, uint32_t trows, uint32_t kadd, uint64_t vadd,
        unsigned bits_k, unsigned dshift, uint32_t tid,
        uint64_t (&rx)[R], unsigned (&rb)[R])
{
    constexpr int G = 8;
    static_assert(R % G == 0, "whole groups of rows");
    const uint32_t kmask = kwd >= 32 ? ~0u : (1u << kwd) - 1;
    const uint32_t vtop = WIDE ? vwd - 32 : vwd;   /* bits of the value's masked dword */
    const uint32_t vmask = vtop >= 32 ? ~0u : (1u << vtop) - 1;
    const uint32_t klast = (trows - 1) * kwd, vlast = (trows - 1) * vwd;
    const uint32_t kstep = kPartThreads * kwd, vstep = kPartThreads * vwd;
    uint32_t kbit = tid * kwd, vbit = tid * vwd, jt = tid;
    #pragma unroll
    for (int i0 = 0; i0 < R; i0 += G) {
        uint32_t k0[G], k1[G], v0[G], v1[G], v2[WIDE ? G : 1], ks[G], vs[G];
        #pragma unroll
        for (int i = 0; i < G; i++) {
            ks[i] = kbit < klast ? kbit : klast;
            vs[i] = vbit < vlast ? vbit : vlast;
            const uint32_t* pk = sk + (ks[i] >> 5);
            const uint32_t* pv = sv + (vs[i] >> 5);
            k0[i] = pk[0];
            k1[i] = pk[1];
            v0[i] = pv[0];
            v1[i] = pv[1];
            if constexpr (WIDE) v2[i] = pv[2];
            kbit += kstep;
            vbit += vstep;
        }
        /* the group's reads stay ahead of its first use: the scheduler
         * otherwise pairs them off two rows at a time */
        __builtin_amdgcn_sched_barrier(0);
        #pragma unroll
        for (int i = 0; i < G; i++) {
            const uint32_t krel = (__builtin_amdgcn_alignbit(k1[i], k0[i], ks[i]) & kmask) + kadd;
            uint32_t lo = __builtin_amdgcn_alignbit(v1[i], v0[i], vs[i]), hi = 0;
            if constexpr (WIDE) hi = __builtin_amdgcn_alignbit(v2[i], v1[i], vs[i]) & vmask;
            else lo &= vmask;
            const uint64_t vrel = (((uint64_t)hi << 32) | lo) + vadd;
            rx[i0 + i] = (uint64_t)krel | (vrel << bits_k);
            rb[i0 + i] = jt < trows ? krel >> dshift : kRowInvalid;
            jt += kPartThreads;
        }
    }
}

/* Phase A. Canonical column slots: 0 = filter, 1 = key, 2 = value.
 * A tile is R rows per thread, R a compile-time constant, so the decoded
 * records and their (bucket, rank) words stay in registers and every row is
 * decoded ONCE, straight from global memory:
 *   1. zero the per-tile histograms;
 *   2. decode all R rows (loads first, rows past the segment end masked),
 *      then rank each row in its bucket with a returning LDS add;
 *   3. one block scan of the histogram gives each bucket's offset in the
 *      tile, one global add per non-empty bucket reserves its run in the
 *      (bucket, XCD sub) region. The cursors lie [sub][bucket], so a
 *      wave's adds fall on 1 KiB of adjacent words, and they are only
 *      ISSUED here;
 *   4. records go to an LDS scratch at off[b] + rank, bucket-major, while
 *      the adds are in flight; then their returned bases give delta[] and
 *      the capacity guard, which gates step 5 alone;
 *   5. the scratch is copied out with every lane busy: lane r re-derives
 *      its record's bucket and stores to base[b] + (r - off[b]), so a
 *      bucket's run leaves as contiguous stores from adjacent lanes.
 * Null-value rows (key only, rare) go straight to their own stream, from
 * registers, in step 5.
 * PLAIN (PartParams::plain_mode) replaces step 2's decode by
 * part_decode_plain and compiles the side pass and the null stream out;
 * steps 3 to 5 are the same code. */
template <bool PACKED, bool PLAIN>
__global__ void __launch_bounds__(kPartThreads, 4)
k_scan_partition(PartParams pp, const DevSeg* segs, const SegEx* segex,
                 const FastCol* cols, TableHdr* th,
                 unsigned long long* cursors,        /* 8 x kNB main: [sub][bucket] */
                 ulonglong2* recs,
                 unsigned long long* ncursors,       /* 8 x kNB null-value stream */
                 uint64_t* nrecs)
{
    static_assert(PACKED || !PLAIN, "the plain decode writes packed records");
    constexpr int R = (PACKED ? kPartTileMax : kPartTileMin) / kPartThreads;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;

    uint64_t* scratch8 = (uint64_t*)smem;         /* the tile's records, bucket-major */
    ulonglong2* scratch16 = (ulonglong2*)smem;
    unsigned* hist = (unsigned*)(smem + kPartScratchBytes);  /* counts, then off[] */
    unsigned* delta = hist + kNB;                 /* run base - off[] (mod 2^32) */
    unsigned* nhist = delta + kNB;                /* null stream: counts, then bases */
    unsigned* misc = nhist + kNB;                 /* [0] guard flag, [1] tile total, [2..] wave sums */

    const bool has_filter = pp.filter_idx >= 0;
    const bool has_val = pp.val_idx >= 0;
    /* per-XCD sub-buckets: workgroups on different XCDs write disjoint
     * record regions (cross-XCD partial-line sharing measured 3.7x write
     * amplification) */
    const int sub = blockIdx.x & 7;
    const uint64_t recmask = (pp.bits_k >= 64) ? ~0ULL : ((1ULL << pp.bits_k) - 1);
    uint64_t* recs8 = (uint64_t*)recs;

    for (int tile = blockIdx.x, half = 0; tile < pp.ntiles; ) {
        const int seg_idx = tile / pp.tiles_per_seg;
        const int tile_in_seg = tile % pp.tiles_per_seg;
        const int64_t ts = (int64_t)tile_in_seg * pp.tile_rows;
        const int32_t seg_rows = segs[cols[1].seg_off + seg_idx].row_count;
        if (ts >= seg_rows) { tile += gridDim.x; continue; }   /* a tile past a short segment's end */
        int64_t te = ts + pp.tile_rows;   /* <= R rows per thread */
        if (te > seg_rows) te = seg_rows;

        const uint64_t* fwords = nullptr;
        const uint8_t* fbm = nullptr;
        uint32_t fwd = 0;
        uint64_t fmask = 0, fmin = 0;
        if (has_filter) {
            const DevSeg& sg = segs[cols[0].seg_off + seg_idx];
            const SegEx& e = segex[cols[0].seg_off + seg_idx];
            fwords = sg.blob + e.off_values_words;
            fwd = e.w_values;
            fmask = (fwd >= 64) ? ~0ULL : ((1ULL << fwd) - 1);
            fmin = sg.min_value;
            if (pp.has_filter_nulls)
                fbm = (const uint8_t*)sg.blob + e.off_bitmap_bytes;
        }
        const DevSeg& sgk = segs[cols[1].seg_off + seg_idx];
        const SegEx& ek = segex[cols[1].seg_off + seg_idx];
        const uint32_t kwd = ek.w_values;
        const uint64_t kmask = (kwd >= 64) ? ~0ULL : ((1ULL << kwd) - 1);
        const uint64_t kmin = sgk.min_value;
        const uint8_t* kbm = pp.has_key_nulls
            ? (const uint8_t*)sgk.blob + ek.off_bitmap_bytes : nullptr;
        const uint64_t* kwords = sgk.blob + ek.off_values_words;
        const uint64_t* vwords = nullptr;
        const uint8_t* vbm = nullptr;
        uint32_t vwd = 0;
        uint64_t vmask = 0, vmin = 0;
        if (has_val) {
            const DevSeg& sg = segs[cols[2].seg_off + seg_idx];
            const SegEx& e = segex[cols[2].seg_off + seg_idx];
            vwords = sg.blob + e.off_values_words;
            vwd = e.w_values;
            vmask = (vwd >= 64) ? ~0ULL : ((1ULL << vwd) - 1);
            vmin = sg.min_value;
            if (pp.has_val_nulls)
                vbm = (const uint8_t*)sg.blob + e.off_bitmap_bytes;
        }

        /* The tile's packed key and value words are staged in the scratch,
         * which is idle until step 4. A tile of kw + vw bits per row fits the
         * 64 KiB whenever its records do; where a segment is written wider
         * than its column's span and a large tile does not fit, the tile is
         * taken as two small ones, which always fit: its second half is the
         * loop's next turn. */
        int64_t step = pp.tile_rows;
        {
            const uint32_t n = (uint32_t)(te - ts);
            if ((((n * kwd + 63) >> 6) + 1 & ~1u) + (((n * vwd + 63) >> 6) + 1 & ~1u) > kPartScratchBytes / 8)
                step = kPartTileMin;
        }
        const int64_t t0 = half ? ts + step : ts;
        const int64_t t1 = t0 + step < te ? t0 + step : te;

        for (int i = tid; i < kNB; i += kPartThreads) { hist[i] = 0; nhist[i] = 0; }
        if (tid == 0) misc[0] = 0;

        /* one straight-line group of coalesced 16-byte loads that the
         * hardware writes straight into LDS (lane l of a wave to the wave's
         * base + 16 l): no registers, each word read once, at most the one
         * word that follows a vector read with it (a tile starts on a word:
         * its first row is a multiple of 64). The value words start on an
         * even word. */
        const uint32_t trows = (uint32_t)(t1 - t0);
        const uint32_t nkw = (trows * kwd + 63) >> 6;
        const uint32_t nvw = (trows * vwd + 63) >> 6;
        const uint32_t nkwp = (nkw + 1) & ~1u;
        {
            typedef const uint64_t __attribute__((address_space(1))) gword;
            typedef __attribute__((address_space(3))) char lchar;
            gword* kg = (gword*)(kwords + (((uint64_t)t0 * kwd) >> 6));
            gword* vg = (gword*)(vwords + (((uint64_t)t0 * vwd) >> 6));
            const uint32_t npairs = (nkwp + nvw + 1) >> 1;
            const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane(tid & ~63);
            constexpr int NS = (int)(kPartScratchBytes / 16) / kPartThreads;
            #pragma unroll
            for (int k = 0; k < NS; k++) {
                const uint32_t p0 = k * kPartThreads + wave0;   /* the wave's first pair */
                const uint32_t wi = 2 * (p0 + (tid & 63));
                if (wi < 2 * npairs)
                    __builtin_amdgcn_global_load_lds(wi < nkwp ? kg + wi : vg + (wi - nkwp),
                                                     (lchar*)smem + 16 * p0, 16, 0, 0);
            }
            __builtin_amdgcn_s_waitcnt(0x0F70);   /* vmcnt(0): this wave's words are in LDS */
        }
        __syncthreads();

        /* decode once, from the staged words. A row past the tile or segment
         * end re-reads the last row and is marked invalid (with the small
         * tile of packed records that is half of a thread's rows: small
         * inputs only). The filter column keeps the per-value global loads.
         * Side rows keep the decoded value in rx. */
        uint64_t rx[R];
        uint64_t ry[PACKED ? 1 : R];
        unsigned rb[R];
        if constexpr (PLAIN) {
            const uint32_t* sk = (const uint32_t*)smem;
            const uint32_t* sv = sk + 2 * nkwp;
            const uint32_t kadd = (uint32_t)(kmin - pp.gmin_k);
            const uint64_t vadd = vmin - pp.gmin_v;
            if (vwd > 32)   /* uniform, per tile */
                part_decode_plain<true, R>(sk, sv, kwd, vwd, trows, kadd, vadd,
                                           pp.bits_k, pp.dshift, tid, rx, rb);
            else
                part_decode_plain<false, R>(sk, sv, kwd, vwd, trows, kadd, vadd,
                                            pp.bits_k, pp.dshift, tid, rx, rb);
        } else {
            #pragma unroll
            for (int i = 0; i < R; i++) {
                const uint32_t jt = (uint32_t)(i * kPartThreads + tid);
                const uint32_t jr = jt < trows ? jt : trows - 1;
                const int64_t jj = t0 + jr;
                bool keep = jt < trows;
                if (has_filter) {
                    int64_t f = zz_dec(fmin + bp_gl(fwords, fmask, fwd, jj));
                    keep = keep && f >= pp.filter_lo && f <= pp.filter_hi;
                    if (fbm) keep = keep && !bm_get(fbm, jj);
                }
                const uint64_t kzz = kmin + bp_lds(scratch8, nkw, kmask, kwd, jr);
                const bool key_null = kbm && bm_get(kbm, jj);
                uint64_t vzz = 0;
                bool val_null = true;
                if (has_val) {
                    vzz = vmin + bp_lds(scratch8 + nkwp, nvw, vmask, vwd, jr);
                    val_null = vbm && bm_get(vbm, jj);
                }
                const uint64_t key = (uint64_t)zz_dec(kzz);
                const unsigned b = pp.direct_mode
                    ? (unsigned)((kzz - pp.gmin_k) >> pp.dshift)
                    : (unsigned)(mix64(key) >> 40) & (kNB - 1);
                unsigned cls;
                uint64_t x, y = 0;
                if (key_null || key == kEmptyKey) {
                    cls = kRowSide | (key_null ? 1u : 0u) | (val_null ? 2u : 0u);
                    x = (uint64_t)zz_dec(vzz);
                } else if (has_val && val_null) {
                    cls = kRowNullVal | b;
                    x = key;
                } else if constexpr (PACKED) {
                    cls = b;
                    x = kzz - pp.gmin_k;
                    if (has_val) x |= (vzz - pp.gmin_v) << pp.bits_k;
                } else {
                    cls = b;
                    x = key;
                    y = has_val ? (uint64_t)zz_dec(vzz) : 0;
                }
                rb[i] = keep ? cls : kRowInvalid;
                rx[i] = x;
                if constexpr (!PACKED) ry[i] = y;
            }
        }
        /* side rows (null key, INT64_MIN key) update their slots in a pass
         * of their own and drop out; almost no wave has one. The plain
         * decode has none. */
        if constexpr (!PLAIN) {
            bool side = false;
            #pragma unroll
            for (int i = 0; i < R; i++)
                side = side || (rb[i] != kRowInvalid && (rb[i] & kRowSide));
            if (__any(side)) {
                #pragma unroll
                for (int i = 0; i < R; i++) {
                    const unsigned c = rb[i];
                    if (c == kRowInvalid || !(c & kRowSide)) continue;
                    const int sd = c & 1;
                    th->side_used[sd] = 1;
                    atomicAdd((unsigned long long*)&th->side_cnt[sd], 1ULL);
                    if (pp.sum_slot >= 0 && !(c & 2)) {
                        atomicAdd((unsigned long long*)&th->side_agg[sd][2 * pp.sum_slot], rx[i]);
                        atomicAdd((unsigned long long*)&th->side_agg[sd][2 * pp.sum_slot + 1], 1ULL);
                    }
                    rb[i] = kRowInvalid;
                }
            }
        }
        /* rank each row in its bucket. No branch: a row that is out adds 0
         * to a word of its thread's own, so the returning LDS adds issue
         * back to back and their results are taken in a second loop */
        {
            unsigned rk[R];
            #pragma unroll
            for (int i = 0; i < R; i++) {
                const unsigned c = rb[i];
                const bool in = c != kRowInvalid;
                unsigned* h = ((!PLAIN && (c & kRowNullVal)) ? nhist : hist) + (c & (kNB - 1));
                rk[i] = atomicAdd(in ? h : &hist[tid], in ? 1u : 0u);
            }
            #pragma unroll
            for (int i = 0; i < R; i++)
                if (rb[i] != kRowInvalid) rb[i] |= rk[i] << 10;
        }
        __syncthreads();

        /* exclusive block scan of hist -> off[] (two buckets per thread,
         * wave scan + wave sums), and one reservation per non-empty
         * bucket in this workgroup's (sub, bucket) cursor. The reservations
         * are issued here and their bases taken after the scratch fill,
         * which needs off[] alone. */
        constexpr int BPT = kNB / kPartThreads;   /* thread t: buckets t and t + 512 */
        static_assert(BPT == 2 && kPartTileMax < (1 << 16), "two 16-bit scan fields");
        unsigned cnt[BPT], ncnt[BPT], boff[BPT];
        unsigned long long mbase[BPT], nbase[BPT];
        {
            /* both halves are scanned at once, as two 16-bit fields of one
             * word: a tile's rows never carry out of the low field */
            const int lane = tid & 63, wave = tid >> 6;
            cnt[0] = hist[tid];
            cnt[1] = hist[tid + kPartThreads];
            const unsigned local = cnt[0] | (cnt[1] << 16);
            unsigned pre = local;
            for (int sh = 1; sh < 64; sh <<= 1) {
                unsigned o = (unsigned)__shfl_up((int)pre, sh, 64);
                if (lane >= sh) pre += o;
            }
            {
                unsigned wv = wave;   /* its LDS address is formed here, as co below */
                asm volatile("" : "+v"(wv));
                if (lane == 63) misc[2 + wv] = pre;
            }
            __syncthreads();
            unsigned excl = pre - local, all = 0;
            #pragma unroll
            for (int w2 = 0; w2 < kPartThreads / 64; w2++) {
                const unsigned ws = misc[2 + w2];
                all += ws;
                if (w2 < wave) excl += ws;
            }
            if (tid == 0) misc[1] = (all & 0xFFFFu) + (all >> 16);
            #pragma unroll
            for (int h = 0; h < BPT; h++) {
                /* the cursor and histogram addresses are formed here, per
                 * tile: kept across the tile loop they cost a dozen registers
                 * and spill */
                unsigned b = tid + h * kPartThreads;
                asm volatile("" : "+v"(b));
                const unsigned co = (unsigned)(sub * kNB) + b;
                const unsigned off = h ? (all & 0xFFFFu) + (excl >> 16) : (excl & 0xFFFFu);
                boff[h] = off;
                mbase[h] = 0;
                if (cnt[h])
                    mbase[h] = atomicAdd(&cursors[co], (unsigned long long)cnt[h]);
                hist[b] = off;
                ncnt[h] = 0;
                nbase[h] = 0;
                if (!PLAIN && pp.has_val_nulls) {
                    ncnt[h] = nhist[b];
                    if (ncnt[h])
                        nbase[h] = atomicAdd(&ncursors[co], (unsigned long long)ncnt[h]);
                }
            }
        }
        __syncthreads();

        /* the scratch fill runs while the reservations are in flight; a tile
         * whose guard trips below has filled its scratch for nothing */
        {
            /* off[] of eight rows' buckets are read together */
            #pragma unroll
            for (int i0 = 0; i0 < R; i0 += 8) {
                unsigned ro[8];
                #pragma unroll
                for (int i = 0; i < 8; i++) ro[i] = hist[rb[i0 + i] & (kNB - 1)];
                #pragma unroll
                for (int i = 0; i < 8; i++) {
                    const unsigned c = rb[i0 + i];
                    if (c == kRowInvalid || (c & kRowNullVal)) continue;
                    const unsigned at = ro[i] + ((c >> 10) & 0x3FFFu);
                    if constexpr (PACKED) {
                        scratch8[at] = rx[i0 + i];
                    } else {
                        scratch16[at] = make_ulonglong2(rx[i0 + i], ry[i0 + i]);
                    }
                }
            }
        }
        /* the returned bases: delta[], the null stream's bases, the guard */
        #pragma unroll
        for (int h = 0; h < BPT; h++) {
            unsigned b = tid + h * kPartThreads;
            asm volatile("" : "+v"(b));
            if (cnt[h]) {
                unsigned long long base = mbase[h];
                if ((int64_t)(base + cnt[h]) > pp.bucket_stride) { th->overflow = 1; misc[0] = 1; base = 0; }
                delta[b] = (unsigned)base - boff[h];
            }
            if (ncnt[h]) {
                unsigned long long base = nbase[h];
                if ((int64_t)(base + ncnt[h]) > pp.nbucket_stride) { th->overflow = 1; misc[0] = 1; base = 0; }
                nhist[b] = (unsigned)base;
            }
        }
        __syncthreads();

        if (misc[0] != 1) {   /* LDS flag: uniform across the block */
            if (!PLAIN && pp.has_val_nulls) {
                #pragma unroll
                for (int i = 0; i < R; i++) {
                    const unsigned c = rb[i];
                    if (c == kRowInvalid || !(c & kRowNullVal)) continue;
                    const unsigned b = c & (kNB - 1);
                    const unsigned rank = (c >> 10) & 0x3FFFu;
                    nrecs[((int64_t)b * 8 + sub) * pp.nbucket_stride + nhist[b] + rank] = rx[i];
                }
            }
            const unsigned total = misc[1];
            for (unsigned r = tid; r < total; r += kPartThreads) {
                if constexpr (PACKED) {
                    const uint64_t rec = scratch8[r];
                    const uint64_t krel = rec & recmask;
                    const unsigned b = pp.direct_mode
                        ? (unsigned)(krel >> pp.dshift)
                        : (unsigned)(mix64((uint64_t)zz_dec(pp.gmin_k + krel)) >> 40) & (kNB - 1);
                    recs8[((int64_t)b * 8 + sub) * pp.bucket_stride + (unsigned)(delta[b] + r)] = rec;
                } else {
                    const ulonglong2 rec = scratch16[r];
                    const unsigned b = pp.direct_mode
                        ? (unsigned)((zz_enc64((int64_t)rec.x) - pp.gmin_k) >> pp.dshift)
                        : (unsigned)(mix64(rec.x) >> 40) & (kNB - 1);
                    recs[((int64_t)b * 8 + sub) * pp.bucket_stride + (unsigned)(delta[b] + r)] = rec;
                }
            }
        }
        __syncthreads();
        if (t1 < te) half = 1;
        else { half = 0; tile += gridDim.x; }
    }
}



/* Phase B's flush, one for both kernels: the workgroup counts its non-empty
 * slots (ballot + popcount per wave, wave sums in LDS), ONE thread reserves
 * the whole run with one add on out_counter and one on th->ngroups, and
 * every lane stores its group at base + rank. Wave w owns the w-th quarter
 * of the 64-slot chunks, so ranks follow slot order and a bucket's groups
 * leave as contiguous stores of adjacent lanes. A workgroup without a group
 * issues no add. The group-limit mark is set iff a ticket of the run reaches
 * group_limit (base + n > group_limit); a group whose index reaches out_cap
 * sets overflow = 1 and is not written.
 * Slots: occupied(i), and read(i, key, cnt, nonnull, sum) for an occupied
 * slot. scanw: kFlushScanWords words of LDS that nothing else uses from the
 * barrier before the flush on. Called by all 256 threads. */
constexpr int kFlushScanWords = 8;      /* 4 wave counts, the base, 3 spare */
/* the direct kernel's largest request: two 8-byte words per slot at dshift
 * 12 (a key span of 22 bits) and the scan words */
constexpr size_t kBucketDirectLdsMax =
    ((size_t)16 << 12) + kFlushScanWords * sizeof(unsigned long long);

template <class Slots>
__device__ __forceinline__ void bucket_flush(const Slots sl, int nslots,
        unsigned long long* scanw, OutGroup* out, unsigned long long* out_counter,
        int64_t out_cap, int slim, TableHdr* th, int sum_slot, int agg_count)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int nchunks = (nslots + 63) >> 6;
    const int cpw = (nchunks + 3) >> 2;
    const int c0 = wave * cpw;
    const int c1 = c0 + cpw < nchunks ? c0 + cpw : nchunks;

    unsigned mine = 0;
    for (int c = c0; c < c1; c++) {
        const int i = c * 64 + lane;
        mine += __popcll(__ballot(i < nslots && sl.occupied(i)));
    }
    if (lane == 0) scanw[wave] = mine;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long n = scanw[0] + scanw[1] + scanw[2] + scanw[3];
        unsigned long long idx = 0;
        if (n) {
            idx = atomicAdd(out_counter, n);
            const unsigned long long t = atomicAdd(&th->ngroups, n);
            if (th->group_limit > 0 && (int64_t)(t + n) > th->group_limit)
                mark_group_limit(th);
        }
        scanw[4] = idx;
    }
    __syncthreads();
    unsigned long long at = scanw[4];
    for (int w = 0; w < wave; w++) at += scanw[w];
    for (int c = c0; c < c1; c++) {
        const int i = c * 64 + lane;
        const bool occ = i < nslots && sl.occupied(i);
        const unsigned long long b = __ballot(occ);
        const unsigned long long idx = at + __popcll(b & ((1ULL << lane) - 1));
        at += __popcll(b);
        if (!occ) continue;
        if ((int64_t)idx >= out_cap) { th->overflow = 1; continue; }
        uint64_t key, cnt, nonnull, sum;
        sl.read(i, key, cnt, nonnull, sum);
        if (slim) {
            ulonglong2* g2 = (ulonglong2*)((SlimGroup*)out + idx);
            g2[0] = make_ulonglong2(key, cnt);
            g2[1] = sum_slot >= 0 ? make_ulonglong2(sum, nonnull)
                                  : make_ulonglong2(0, 0);
            continue;
        }
        OutGroup& g = out[idx];
        g.key_bits = key;
        g.key_meta = 0;
        g.cnt = cnt;
        for (int a = 0; a < agg_count; a++) {
            g.agg_bits[a] = 0;
            g.agg_nonnull[a] = 0;
        }
        if (sum_slot >= 0) {
            g.agg_bits[sum_slot] = sum;
            g.agg_nonnull[sum_slot] = nonnull;
        }
    }
}

/* the hash kernel's table: {key, cnt | nonnull << 32, sum} */
struct HashSlots {
    const unsigned long long* tab;
    __device__ __forceinline__ bool occupied(int i) const
    {
        return tab[i * 3] != (unsigned long long)kEmptyKey;
    }
    __device__ __forceinline__ void read(int i, uint64_t& key, uint64_t& cnt,
                                         uint64_t& nonnull, uint64_t& sum) const
    {
        key = tab[i * 3];
        const uint64_t cn = tab[i * 3 + 1];
        cnt = cn & 0xFFFFFFFFULL;
        nonnull = cn >> 32;
        sum = tab[i * 3 + 2];
    }
};

/* Phase B: one workgroup per bucket. LDS table slot = {key, cnt|nonnull<<32
 * packed, sum}; per-workgroup counts stay < 2^32 because a bucket's rows do.
 * Emits compacted OutGroups directly (buckets are key-disjoint), or
 * SlimGroups (out then points at those) when the launcher sets slim. */
__global__ void __launch_bounds__(256)
k_bucket_agg(const ulonglong2* recs, const unsigned long long* cursors,
             int64_t bucket_stride,
             const uint64_t* nrecs, const unsigned long long* ncursors,
             int64_t nbucket_stride,
             OutGroup* out, unsigned long long* out_counter, int64_t out_cap,
             int slim, TableHdr* th, int sum_slot, int agg_count,
             int packed_mode, int bits_k, uint64_t gmin_k, uint64_t gmin_v,
             int nsub)
{
    __shared__ unsigned long long tab[kHSlots * 3];
    __shared__ unsigned long long scanw[kFlushScanWords];
    const int tid = threadIdx.x;
    const int bucket = blockIdx.x;

    /* a capacity guard tripped in phase A: its cursors then count records
     * that were never written and run past their regions, and the host
     * discards this pass anyway — read nothing */
    __shared__ int skip;
    if (tid == 0) skip = (th->overflow == 1);
    __syncthreads();
    if (skip) return;

    for (int i = tid; i < kHSlots; i += 256) {
        tab[i * 3] = kEmptyKey;
        tab[i * 3 + 1] = 0;
        tab[i * 3 + 2] = 0;
    }
    __syncthreads();

    const uint64_t kmask = (bits_k >= 64) ? ~0ULL : ((1ULL << bits_k) - 1);
    bool full = false;
    for (int sub = 0; sub < nsub && !full; sub++) {
    int64_t n = (int64_t)cursors[(int64_t)sub * kNB + bucket];
    const ulonglong2* rows = recs + ((int64_t)bucket * nsub + sub) * bucket_stride;
    const uint64_t* rows8 = (const uint64_t*)recs + ((int64_t)bucket * nsub + sub) * bucket_stride;
    /* 4 records per thread per pass: independent probes overlap LDS latency */
    int64_t i = tid;
    /* real INT64_MIN keys are side-slotted in phase A and never enter the
     * streams, so kEmptyKey is free to mark an empty table slot */
    #define LOADKV(kv, idx)                                                  \
        ulonglong2 kv;                                                       \
        if (packed_mode) {                                                   \
            uint64_t r_ = rows8[idx];                                        \
            kv.x = (uint64_t)zz_dec(gmin_k + (r_ & kmask));                  \
            kv.y = (uint64_t)zz_dec(gmin_v + (r_ >> bits_k));                \
        } else {                                                             \
            kv = rows[idx];                                                  \
        }
    for (; i + 1792 < n; i += 2048) {
        LOADKV(kv0, i)
        LOADKV(kv1, i + 256)
        LOADKV(kv2, i + 512)
        LOADKV(kv3, i + 768)
        LOADKV(kv4, i + 1024)
        LOADKV(kv5, i + 1280)
        LOADKV(kv6, i + 1536)
        LOADKV(kv7, i + 1792)
        uint64_t s0 = mix64(kv0.x) & (kHSlots - 1);
        uint64_t s1 = mix64(kv1.x) & (kHSlots - 1);
        uint64_t s2 = mix64(kv2.x) & (kHSlots - 1);
        uint64_t s3 = mix64(kv3.x) & (kHSlots - 1);
        #define PROBE(kv, sv_)                                               \
        if (kv.x != (unsigned long long)kEmptyKey) {                         \
            uint64_t sp = sv_;                                               \
            int found = 0;                                                   \
            for (int it = 0; it < kHSlots; it++) {                           \
                unsigned long long k = tab[sp * 3];                          \
                if (k == (unsigned long long)kv.x) { found = 1; break; }     \
                if (k == (unsigned long long)kEmptyKey) {                    \
                    k = atomicCAS(&tab[sp * 3], (unsigned long long)kEmptyKey,\
                                  (unsigned long long)kv.x);                 \
                    if (k == (unsigned long long)kEmptyKey ||                \
                        k == (unsigned long long)kv.x) { found = 1; break; } \
                }                                                            \
                sp = (sp + 1) & (kHSlots - 1);                               \
            }                                                                \
            if (!found) { full = true; }                                     \
            else {                                                           \
                atomicAdd(&tab[sp * 3 + 1], 1ULL | (1ULL << 32));            \
                if (sum_slot >= 0)                                           \
                    atomicAdd(&tab[sp * 3 + 2], (unsigned long long)kv.y);   \
            }                                                                \
        }
        uint64_t s4 = mix64(kv4.x) & (kHSlots - 1);
        uint64_t s5 = mix64(kv5.x) & (kHSlots - 1);
        uint64_t s6 = mix64(kv6.x) & (kHSlots - 1);
        uint64_t s7 = mix64(kv7.x) & (kHSlots - 1);
        PROBE(kv0, s0)
        PROBE(kv1, s1)
        PROBE(kv2, s2)
        PROBE(kv3, s3)
        PROBE(kv4, s4)
        PROBE(kv5, s5)
        PROBE(kv6, s6)
        PROBE(kv7, s7)
        if (full) break;
    }
    for (; i < n && !full; i += 256) {
        LOADKV(kv, i)
        uint64_t s0 = mix64(kv.x) & (kHSlots - 1);
        PROBE(kv, s0)
    }
    }   /* sub-stream loop */
    #undef PROBE
    #undef LOADKV
    if (nrecs) {
        for (int sub = 0; sub < 8 && !full; sub++) {
        int64_t nn = (int64_t)ncursors[sub * kNB + bucket];
        const uint64_t* nrows = nrecs + ((int64_t)bucket * 8 + sub) * nbucket_stride;
        for (int64_t i = tid; i < nn && !full; i += 256) {
            uint64_t key = nrows[i];
            uint64_t s = mix64(key) & (kHSlots - 1);
            int found = 0;
            for (int it = 0; it < kHSlots; it++) {
                unsigned long long k = tab[s * 3];
                if (k == (unsigned long long)key) { found = 1; break; }
                if (k == (unsigned long long)kEmptyKey) {
                    k = atomicCAS(&tab[s * 3], (unsigned long long)kEmptyKey,
                                  (unsigned long long)key);
                    if (k == (unsigned long long)kEmptyKey ||
                        k == (unsigned long long)key) { found = 1; break; }
                }
                s = (s + 1) & (kHSlots - 1);
            }
            if (!found) { full = true; break; }
            atomicAdd(&tab[s * 3 + 1], 1ULL);   /* cnt only; sum stays null-contributing */
        }
        }   /* sub-stream loop */
    }
    if (full) th->overflow = 1;
    __syncthreads();

    /* flush compacted groups */
    bucket_flush(HashSlots{tab}, kHSlots, scanw, out, out_counter, out_cap,
                 slim, th, sum_slot, agg_count);
}


/* the direct kernel's table: cnt | nonnull << 32 and sum in an array each;
 * the slot index IS the key (zz-relative to key0) */
struct DirectSlots {
    const unsigned long long* cntnn;
    const unsigned long long* sums;
    uint64_t key0;
    __device__ __forceinline__ bool occupied(int i) const { return cntnn[i] != 0; }
    __device__ __forceinline__ void read(int i, uint64_t& key, uint64_t& cnt,
                                         uint64_t& nonnull, uint64_t& sum) const
    {
        key = (uint64_t)zz_dec(key0 + (uint64_t)i);
        cnt = cntnn[i] & 0xFFFFFFFFULL;
        nonnull = cntnn[i] >> 32;
        sum = sums[i];
    }
};

/* Phase B, direct-span mode: buckets are key-RANGE slices, so the LDS
 * "table" is a dense array indexed by (krel - bucket<<dshift) — no hash,
 * no probe loop, no CAS, no stored keys. Slot = {cnt|nonnull<<32, sum}; the
 * flush's scan words lie behind the two arrays.
 * Semantics identical to k_bucket_agg (registry.cpp:1783-1834 insert +
 * udf/sum.c null-propagating sum); only the table organisation differs. */
__global__ void __launch_bounds__(256)
k_bucket_agg_direct(const ulonglong2* recs, const unsigned long long* cursors,
                    int64_t bucket_stride,
                    const uint64_t* nrecs, const unsigned long long* ncursors,
                    int64_t nbucket_stride,
                    OutGroup* out, unsigned long long* out_counter, int64_t out_cap,
                    int slim, TableHdr* th, int sum_slot, int agg_count,
                    int packed_mode, int bits_k, uint64_t gmin_k, uint64_t gmin_v,
                    int dshift, int nsub)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int SL = 1 << dshift;
    unsigned long long* cntnn = (unsigned long long*)smem;   /* lo cnt, hi nonnull */
    unsigned long long* sums = cntnn + SL;
    const int tid = threadIdx.x;
    const int bucket = blockIdx.x;

    /* a capacity guard tripped in phase A: its cursors then count records
     * that were never written and run past their regions, and the host
     * discards this pass anyway — read nothing. The flag goes through
     * cntnn[0], which the zeroing below takes back. */
    if (tid == 0) cntnn[0] = (th->overflow == 1);
    __syncthreads();
    const bool skip = cntnn[0] != 0;
    __syncthreads();
    if (skip) return;

    for (int i = tid; i < SL; i += 256) { cntnn[i] = 0; sums[i] = 0; }
    __syncthreads();

    const uint64_t kmask = (bits_k >= 64) ? ~0ULL : ((1ULL << bits_k) - 1);
    const uint64_t base_rel = (uint64_t)bucket << dshift;
    const bool has_sum = sum_slot >= 0;

    for (int sub = 0; sub < nsub; sub++) {
        int64_t n = (int64_t)cursors[(int64_t)sub * kNB + bucket];
        const ulonglong2* rows = recs + ((int64_t)bucket * nsub + sub) * bucket_stride;
        const uint64_t* rows8 = (const uint64_t*)recs + ((int64_t)bucket * nsub + sub) * bucket_stride;
        int64_t i = tid;
        /* a packed record with bit 63 set, or a 16-byte one with key
         * kEmptyKey, is skipped: phase A stores neither (direct mode is only
         * chosen with bit 63 spare, INT64_MIN keys are side-slotted), so the
         * skips are never taken */
        #define DACCR(r_)                                                    \
            {                                                                \
                uint64_t k_ = ((int64_t)(r_) < 0 && packed_mode)             \
                    ? ~0ULL : ((r_) & kmask) - base_rel;                     \
                if (k_ != ~0ULL) {                                           \
                    atomicAdd(&cntnn[k_], 1ULL | (1ULL << 32));              \
                    if (has_sum)                                             \
                        atomicAdd(&sums[k_],                                 \
                                  (uint64_t)zz_dec(gmin_v + ((r_) >> bits_k))); \
                }                                                            \
            }
        if (packed_mode) {
            /* 16B paired loads: 8 in flight = 16 records per thread pass */
            const ulonglong2* rows2 = (const ulonglong2*)rows8;
            int64_t n2 = n >> 1;
            for (; i + 1792 < n2; i += 2048) {
                ulonglong2 p0 = rows2[i];
                ulonglong2 p1 = rows2[i + 256];
                ulonglong2 p2 = rows2[i + 512];
                ulonglong2 p3 = rows2[i + 768];
                ulonglong2 p4 = rows2[i + 1024];
                ulonglong2 p5 = rows2[i + 1280];
                ulonglong2 p6 = rows2[i + 1536];
                ulonglong2 p7 = rows2[i + 1792];
                DACCR(p0.x) DACCR(p0.y) DACCR(p1.x) DACCR(p1.y)
                DACCR(p2.x) DACCR(p2.y) DACCR(p3.x) DACCR(p3.y)
                DACCR(p4.x) DACCR(p4.y) DACCR(p5.x) DACCR(p5.y)
                DACCR(p6.x) DACCR(p6.y) DACCR(p7.x) DACCR(p7.y)
            }
            for (; i < n2; i += 256) {
                ulonglong2 pz = rows2[i];
                DACCR(pz.x) DACCR(pz.y)
            }
            if ((n & 1) && tid == 0) {
                uint64_t r_ = rows8[n - 1];
                DACCR(r_)
            }
        } else {
            for (; i < n; i += 256) {
                ulonglong2 kv = rows[i];
                uint64_t k_ = (kv.x == kEmptyKey) ? ~0ULL
                     : (zz_enc64((int64_t)kv.x) - gmin_k) - base_rel;
                if (k_ != ~0ULL) {
                    atomicAdd(&cntnn[k_], 1ULL | (1ULL << 32));
                    if (has_sum) atomicAdd(&sums[k_], kv.y);
                }
            }
        }
        #undef DACCR
    }
    if (nrecs) {
        for (int sub = 0; sub < 8; sub++) {
            int64_t nn = (int64_t)ncursors[sub * kNB + bucket];
            const uint64_t* nrows = nrecs + ((int64_t)bucket * 8 + sub) * nbucket_stride;
            for (int64_t i = tid; i < nn; i += 256) {
                uint64_t key = nrows[i];
                if (key == kEmptyKey) continue;         /* never stored: side-slotted */
                uint64_t idx = (zz_enc64((int64_t)key) - gmin_k) - base_rel;
                atomicAdd(&cntnn[idx], 1ULL);           /* cnt only: null value */
            }
        }
    }
    __syncthreads();

    /* flush: slot index IS the key (zz-relative) */
    bucket_flush(DirectSlots{cntnn, sums, gmin_k + base_rel}, SL,
                 (unsigned long long*)smem + 2 * SL, out, out_counter, out_cap,
                 slim, th, sum_slot, agg_count);
}


/* ------------------------------------------------------------------ */
/* string-keyed GROUP BY (config-5 family; see common.h StrGroupParams) */

/* string dictionary entry bounds — string_column_reader.cpp:39-42:
 * offset(i) = expected_length*(i+1) + ZigZagDecode32(packed[i]) */
__device__ __forceinline__ int32_t zz_dec32(uint32_t n)
{
    return (int32_t)((n >> 1) ^ (~(n & 1) + 1));
}

__device__ __forceinline__ uint64_t str_off(const uint64_t* offs, uint32_t w,
                                            uint64_t expected, int64_t i)
{
    if (i < 0) return 0;
    return expected * (uint64_t)(i + 1)
         + (uint64_t)(int64_t)zz_dec32((uint32_t)bp_get(offs, w, i));
}

/* dictionary entry j (0-BASED index = id-1) of a parsed string segment →
 * (ptr, len): spans [offset(j-1), offset(j)), offset(-1) = 0
 * (string_column_reader.cpp:44-66) */
__device__ __forceinline__ const char* dict_entry(const DevSeg& s, const SegEx& e,
                                                  int64_t j, uint32_t* len)
{
    const uint64_t* offs = s.blob + e.off_values_words;
    uint64_t b = str_off(offs, e.w_values, s.min_value, j - 1);
    uint64_t en = str_off(offs, e.w_values, s.min_value, j);
    *len = (uint32_t)(en - b);
    return (const char*)s.blob + e.off_doubles_bytes + b;
}

/* S1: accumulate rows into per-segment per-dictionary-id accumulators
 * acc[base + id-1] = { cnt|nonnull<<32 (u32 pair, bounded by the 128Ki
 * segment row cap), sum bits }. Null ids go to the null-key side group. */
__global__ void __launch_bounds__(256)
k_strgrp_accum(StrGroupParams sp, const DevSeg* segs, const SegEx* segex,
               const int64_t* acc_base, unsigned long long* acc,
               TableHdr* th)
{
    /* XCD-affine schedule: workgroups land on XCD blockIdx%8 (round-robin,
     * MI355X_MICROARCH.md), so striding segments by 8 from blockIdx&7 keeps
     * ALL tiles of a segment — and therefore all atomics into its ~1.3 MB
     * accumulator region — inside one XCD's 4 MB L2 instead of ping-ponging
     * the lines across eight of them. */
    const bool affine = gridDim.x >= 64;
    const int xcd = blockIdx.x & 7;
    const int sub = blockIdx.x >> 3;
    const int nsub = gridDim.x >> 3;
    const int nwork = affine
        ? ((sp.key_seg_cnt + 7) >> 3) * sp.tiles_per_seg   /* per-XCD upper bound */
        : sp.ntiles;
    for (int w = affine ? sub : blockIdx.x; w < nwork;
         w += affine ? nsub : gridDim.x) {
        int seg_idx, tile_in_seg;
        if (affine) {
            seg_idx = xcd + 8 * (w / sp.tiles_per_seg);
            tile_in_seg = w % sp.tiles_per_seg;
            if (seg_idx >= sp.key_seg_cnt) continue;
            if (seg_idx * sp.tiles_per_seg + tile_in_seg >= sp.ntiles) continue;
        } else {
            seg_idx = w / sp.tiles_per_seg;
            tile_in_seg = w % sp.tiles_per_seg;
        }
        const DevSeg& sk = segs[sp.key_seg_off + seg_idx];
        const SegEx& ek = segex[sp.key_seg_off + seg_idx];
        const int64_t t0 = (int64_t)tile_in_seg * sp.tile_rows;
        int64_t t1 = t0 + sp.tile_rows;
        if (t1 > sk.row_count) t1 = sk.row_count;
        unsigned long long* seg_acc = acc + 2 * acc_base[seg_idx];

        const DevSeg* sv = sp.val_seg_off >= 0 ? &segs[sp.val_seg_off + seg_idx] : nullptr;
        const SegEx* ev = sp.val_seg_off >= 0 ? &segex[sp.val_seg_off + seg_idx] : nullptr;
        const uint8_t* vbm = nullptr;
        uint64_t vmask = 0, vmin = 0;
        uint32_t vwd = 0;
        const uint64_t* vwords = nullptr;
        if (sv) {
            vwords = sv->blob + ev->off_values_words;
            vwd = ev->w_values;
            vmask = (vwd >= 64) ? ~0ULL : ((1ULL << vwd) - 1);
            vmin = sv->min_value;
            if (sp.has_val_nulls)
                vbm = (const uint8_t*)sv->blob + ev->off_bitmap_bytes;
        }

        const bool is_rle = (sk.type == YT_SEG_DICTIONARY_RLE);
        const bool is_direct = (ek.flags & 32) != 0;
        const uint8_t* kbm = (const uint8_t*)sk.blob + ek.off_bitmap_bytes;
        const uint64_t* ids = sk.blob + ek.off_ids_words;
        const uint64_t* starts = sk.blob + ek.off_starts_words;
        const int R = (sp.tile_rows + 255) / 256;
        for (int i = 0; i < R; i++) {
            int64_t j = t0 + (int64_t)i * 256 + threadIdx.x;
            if (j >= t1) continue;
            uint64_t id;
            if (is_direct) {
                /* identity dictionary: row j IS entry j; nulls by bitmap */
                id = bm_get(kbm, j) ? 0 : (uint64_t)(j + 1);
            } else if (is_rle) {
                uint32_t lo = 0, hi = ek.run_count;
                while (lo + 1 < hi) {
                    uint32_t mid = (lo + hi) / 2;
                    if (bp_get(starts, ek.w_starts, mid) <= (uint64_t)j) lo = mid;
                    else hi = mid;
                }
                id = bp_get(ids, ek.w_ids, lo);
            } else {
                id = bp_get(ids, ek.w_ids, j);
            }
            int val_null = 1;
            uint64_t vbits = 0;
            double vdbl = 0;
            if (sv) {
                if (sv->type == YT_SEG_DOUBLE ||
                    (sv->type == YT_SEG_DIRECT_DENSE && sv->is_signed != 2)) {
                    val_null = vbm && bm_get(vbm, j);
                    if (!val_null) {
                        if (sv->type == YT_SEG_DOUBLE) {
                            vbits = ((const uint64_t*)((const uint8_t*)sv->blob
                                     + ev->off_doubles_bytes))[j];
                            vdbl = __longlong_as_double(vbits);
                        } else {
                            uint64_t pv = bp_gl(vwords, vmask, vwd, j);
                            vbits = (uint64_t)zz_dec(vmin + pv);
                        }
                    }
                } else {
                    /* dictionary / RLE value segments: generic per-row
                     * fetch (handles the layout's own null encoding) */
                    DVal dv = seg_value_at(*sv, *ev, j,
                                           sp.val_is_double ? YT_VT_DOUBLE
                                                            : YT_VT_INT64);
                    val_null = dv.null_;
                    vbits = dv.bits;
                    if (sp.val_is_double) vdbl = __longlong_as_double(dv.bits);
                }
            }
            if (id == 0) {
                /* null string key → side group (registry.cpp group-key null) */
                th->side_used[1] = 1;
                atomicAdd((unsigned long long*)&th->side_cnt[1], 1ULL);
                if (sp.sum_slot >= 0 && !val_null) {
                    if (sp.val_is_double)
                        atomicAdd((double*)&th->side_agg[1][2 * sp.sum_slot], vdbl);
                    else
                        atomicAdd((unsigned long long*)&th->side_agg[1][2 * sp.sum_slot], vbits);
                    atomicAdd((unsigned long long*)&th->side_agg[1][2 * sp.sum_slot + 1], 1ULL);
                }
                continue;
            }
            unsigned long long* a = seg_acc + 2 * (id - 1);
            atomicAdd(a, 1ULL | ((unsigned long long)(!val_null) << 32));
            if (sp.sum_slot >= 0 && !val_null) {
                if (sp.val_is_double) atomicAdd((double*)(a + 1), vdbl);
                else atomicAdd(a + 1, vbits);
            }
        }
    }
}

/* ---- shared by every string-key merge (common.h StrSlot) ---- */

__device__ __forceinline__ uint64_t fnv1a_bytes(const char* p, uint32_t len)
{
    uint64_t h = 0xCBF29CE484222325ULL;
    for (uint32_t k = 0; k < len; k++)
        h = (h ^ (uint8_t)p[k]) * 0x100000001B3ULL;
    return h;
}

/* the segment that owns global entry g: the last s with base[s] <= g */
__device__ __forceinline__ int seg_of(const int64_t* base, int nsegs, int64_t g)
{
    int lo = 0, hi = nsegs;
    while (lo + 1 < hi) {
        int mid = (lo + hi) / 2;
        if (base[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

/* what the merges stream per key: the FNV-1a hash, the slot identity
 * (hash48|len16) and the first 16 bytes, zero-padded */
__device__ __forceinline__ void str_key_identity(const char* p, uint32_t len,
                                                 uint64_t* hash, uint64_t* ident,
                                                 ulonglong2* pfx)
{
    const uint64_t h = fnv1a_bytes(p, len);
    ulonglong2 pf;
    pf.x = 0; pf.y = 0;
    const uint32_t npfx = len < 16 ? len : 16;
    for (uint32_t k = 0; k < npfx; k++)
        ((char*)&pf)[k] = p[k];
    *hash = h;
    *ident = ((h >> 16) << 16) | (uint64_t)(len & 0xFFFF);
    *pfx = pf;
}

/* exclusive scan of (a, b) over the 256 threads of a block, in thread
 * order; *ta, *tb = the block totals (the same in every thread) */
__device__ __forceinline__ void block_excl_scan2(uint64_t& a, uint64_t& b,
                                                 uint64_t* ta, uint64_t* tb,
                                                 uint64_t (*wsum)[2] /* [4] LDS */)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t ia = a, ib = b;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t xa = (uint64_t)__shfl_up((unsigned long long)ia, d, 64);
        const uint64_t xb = (uint64_t)__shfl_up((unsigned long long)ib, d, 64);
        if (lane >= d) { ia += xa; ib += xb; }
    }
    __syncthreads();            /* wsum may still be read from the last call */
    if (lane == 63) { wsum[wave][0] = ia; wsum[wave][1] = ib; }
    __syncthreads();
    uint64_t ba = 0, bb = 0, sa = 0, sb = 0;
    for (int w = 0; w < 4; w++) {
        if (w < wave) { ba += wsum[w][0]; bb += wsum[w][1]; }
        sa += wsum[w][0];
        sb += wsum[w][1];
    }
    a = ba + ia - a;
    b = bb + ib - b;
    *ta = sa;
    *tb = sb;
}

/* The slot identity protocol, once. Find the slot that holds key's string
 * or claim an empty one for it; nullptr when the probe gave up (table too
 * small: the caller raises th->overflow and the host retries at 4x, never a
 * wrong result). *claimed = this call created the group.
 *
 * Everything the hot path needs is STREAMED (hash, ident, pfx are read in
 * key order) — the only random memory is the slot line itself, read as ONE
 * 32-byte load (rep|ident|pfx share the line's first half). What a Key
 * resolves lazily — its claim word, the owner's bytes — is paid only by the
 * ~1/dup-factor claimers and the rare fallbacks.
 *
 * A Key supplies:
 *   hash(), ident(), pfx()  from the streamed arrays
 *   rep()                   the nonzero claim word that names this key,
 *                           computed on first use and cached
 *   equals_owner(cur)       exact: are this key's bytes those of the key
 *                           that claim word cur names */
template <typename Key>
__device__ __forceinline__ StrSlot* strslot_find_or_claim(StrSlot* slots, uint64_t mask,
                                                          Key& key, bool* claimed)
{
    const uint64_t h = key.hash();
    const uint64_t my_ident = key.ident();
    const uint32_t my_len = (uint32_t)(my_ident & 0xFFFF);
    const ulonglong2 pf = key.pfx();
    *claimed = false;
    uint64_t sidx = mix64(h) & mask;
    /* probe chains this long only happen when the table is (nearly) full —
     * give up early so a too-small table overflows in bounded time */
    const uint64_t max_probe = mask < 8192 ? mask : 8192;
    for (uint64_t it = 0; it <= max_probe; it++, sidx = (sidx + 1) & mask) {
        StrSlot* cand = &slots[sidx];
        const ulonglong4 v = *(const ulonglong4*)cand;
        unsigned long long cur = v.x;
        uint64_t oident = v.y;
        if (cur == 0ULL) {
            cur = atomicCAS(&cand->rep, 0ULL, key.rep());
            if (cur == 0ULL) {
                /* claimed: publish the identity (relaxed agent stores;
                 * readers that catch it unpublished fall back to the exact
                 * compare) */
                __hip_atomic_store(&cand->pfx[0], pf.x,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&cand->pfx[1], pf.y,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&cand->ident, my_ident,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                *claimed = true;
                return cand;
            }
            /* lost the race: cand belongs to someone else now and its
             * identity may be unpublished — treat as oident 0 */
            oident = 0;
        }
        if (oident != 0 && oident != my_ident) continue;
        if (oident == my_ident && my_len <= 16
            && v.z == pf.x && v.w == pf.y) return cand;
        /* unpublished identity, long key, or prefix mismatch on an ident
         * match: decide exactly from the owner's bytes (rare) */
        if (key.equals_owner(cur)) return cand;
    }
    return nullptr;
}

/* Key: global dictionary entry g of the key column. rep = (seg+1)<<32 |
 * 1-based id in that segment. The segment search is lazy: only claimers
 * and fallbacks pay it (and the dictionary reads behind it). kEagerRep runs
 * it in the constructor instead, where it overlaps the streamed loads:
 * k_strgen_merge's choice, about 4 % faster there at one claimer in five
 * entries (profiles/r06); k_strgrp_merge keeps the lazy form config 5 was tuned on. */
template <bool kEagerRep>
struct DictEntryKey {
    const DevSeg* segs;
    const SegEx* segex;
    int key_seg_off, nsegs;
    const int64_t* acc_base;
    const uint64_t* hashes;
    const uint64_t* idents;
    const ulonglong2* pfxs;
    int64_t g;
    uint64_t h;
    int seg;                        /* valid once rep_ != 0 */
    unsigned long long rep_;

    __device__ __forceinline__
    DictEntryKey(const DevSeg* segs_, const SegEx* segex_, int key_seg_off_,
                 int nsegs_, const int64_t* acc_base_, const uint64_t* hashes_,
                 const uint64_t* idents_, const ulonglong2* pfxs_, int64_t g_)
        : segs(segs_), segex(segex_), key_seg_off(key_seg_off_), nsegs(nsegs_),
          acc_base(acc_base_), hashes(hashes_), idents(idents_), pfxs(pfxs_),
          g(g_), h(hashes_[g_]), seg(0), rep_(0)
    {
        if (kEagerRep) (void)rep();
    }

    __device__ __forceinline__ uint64_t hash() const { return h; }
    __device__ __forceinline__ uint64_t ident() const { return idents[g]; }
    __device__ __forceinline__ ulonglong2 pfx() const { return pfxs[g]; }
    __device__ __forceinline__ unsigned long long rep()
    {
        if (!rep_) {
            seg = seg_of(acc_base, nsegs, g);
            rep_ = ((unsigned long long)(seg + 1) << 32)
                 | (unsigned long long)(g - acc_base[seg] + 1);
        }
        return rep_;
    }
    __device__ __forceinline__ bool equals_owner(unsigned long long cur)
    {
        const int oseg = (int)(cur >> 32) - 1;
        const int64_t oid = (int64_t)(cur & 0xFFFFFFFFULL);
        if (hashes[acc_base[oseg] + oid - 1] != h) return false;
        (void)rep();
        uint32_t mlen, olen;
        const char* mp = dict_entry(segs[key_seg_off + seg], segex[key_seg_off + seg],
                                    g - acc_base[seg], &mlen);
        const char* op = dict_entry(segs[key_seg_off + oseg],
                                    segex[key_seg_off + oseg], oid - 1, &olen);
        if (olen != mlen) return false;
        uint32_t k = 0;
        while (k < mlen && op[k] == mp[k]) k++;
        return k == mlen;
    }
};

/* Key: exchanged state i, its bytes in the concatenated pool at absoff[i]
 * (offset << 24 | length). rep = i + 1. */
struct PoolStateKey {
    const char* pool;
    const uint64_t* absoff;
    const uint64_t* hashes;
    const uint64_t* idents;
    const ulonglong2* pfxs;
    int64_t i;
    uint64_t h;

    __device__ __forceinline__
    PoolStateKey(const char* pool_, const uint64_t* absoff_, const uint64_t* hashes_,
                 const uint64_t* idents_, const ulonglong2* pfxs_, int64_t i_)
        : pool(pool_), absoff(absoff_), hashes(hashes_), idents(idents_),
          pfxs(pfxs_), i(i_), h(hashes_[i_]) {}

    __device__ __forceinline__ uint64_t hash() const { return h; }
    __device__ __forceinline__ uint64_t ident() const { return idents[i]; }
    __device__ __forceinline__ ulonglong2 pfx() const { return pfxs[i]; }
    __device__ __forceinline__ unsigned long long rep() const
    {
        return (unsigned long long)(i + 1);
    }
    __device__ __forceinline__ bool equals_owner(unsigned long long cur) const
    {
        const int64_t oi = (int64_t)cur - 1;
        if (hashes[oi] != h) return false;
        const uint64_t mab = absoff[i], oab = absoff[oi];
        const uint32_t mlen = (uint32_t)(mab & 0xFFFFFF);
        if ((uint32_t)(oab & 0xFFFFFF) != mlen) return false;
        const char* mp = pool + (mab >> 24);
        const char* op = pool + (oab >> 24);
        uint32_t k = 0;
        while (k < mlen && op[k] == mp[k]) k++;
        return k == mlen;
    }
};

/* Claims are counted per block in LDS (*s_claims) and folded into
 * th->ngroups ONCE per block — a per-claim global atomicAdd on that single
 * address serializes (~160 M/s measured, tools/probe_strcompact) and
 * throttled the whole merge at 100 M distinct keys. The group-limit check
 * sits on the fold. Every thread of the block calls this, after its loop. */
__device__ __forceinline__ void strslot_fold_claims(const unsigned long long* s_claims,
                                                    TableHdr* th)
{
    __syncthreads();
    if (threadIdx.x == 0 && *s_claims) {
        unsigned long long t = atomicAdd(&th->ngroups, *s_claims);
        if (th->group_limit > 0 && (int64_t)(t + *s_claims) > th->group_limit)
            mark_group_limit(th);
    }
}

/* S2: hash, slot identity and 16-byte prefix of every dictionary entry. This
 * kernel already streams every dictionary byte, so capturing them here lets
 * the merge's hot path touch ONLY its streaming arrays and the slot line
 * (no dict reads, no binary search). */
__global__ void k_strgrp_hash(const DevSeg* segs, const SegEx* segex,
                              int key_seg_off, int nsegs,
                              const int64_t* acc_base, uint64_t* hashes,
                              uint64_t* idents, ulonglong2* pfxs)
{
    int64_t total = acc_base[nsegs];
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int s = seg_of(acc_base, nsegs, g);
        uint32_t len;
        const char* p = dict_entry(segs[key_seg_off + s], segex[key_seg_off + s],
                                   g - acc_base[s], &len);
        str_key_identity(p, len, &hashes[g], &idents[g], &pfxs[g]);
    }
}

/* S3: merge dictionary entries across segments by exact string identity.
 * One thread per dictionary entry with a nonzero count. */
__global__ void k_strgrp_merge(const DevSeg* segs, const SegEx* segex,
                               int key_seg_off, int nsegs,
                               const int64_t* acc_base,
                               const unsigned long long* acc,
                               const uint64_t* hashes,
                               const uint64_t* idents, const ulonglong2* pfxs,
                               StrSlot* slots, uint64_t nslots,
                               int val_is_double, TableHdr* th)
{
    int64_t total = acc_base[nsegs];
    __shared__ unsigned long long s_claims;
    if (threadIdx.x == 0) s_claims = 0;
    __syncthreads();
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < total; g += (int64_t)gridDim.x * blockDim.x) {
        unsigned long long cn = acc[2 * g];
        if (cn == 0) continue;
        DictEntryKey<false> key(segs, segex, key_seg_off, nsegs, acc_base, hashes,
                         idents, pfxs, g);
        bool claimed;
        StrSlot* slot = strslot_find_or_claim(slots, nslots - 1, key, &claimed);
        if (!slot) { th->overflow = 1; continue; }
        if (claimed) atomicAdd(&s_claims, 1ULL);
        /* one packed atomic: cnt in the low half, nonnull in the high half
         * (both < 2^32 — segment row caps; carries cannot cross) */
        atomicAdd((unsigned long long*)&slot->cnt, cn);
        unsigned long long nn = cn >> 32;
        if (nn) {
            if (val_is_double)
                atomicAdd((double*)&slot->sum_bits,
                          __longlong_as_double(acc[2 * g + 1]));
            else
                atomicAdd((unsigned long long*)&slot->sum_bits, acc[2 * g + 1]);
        }
    }
    strslot_fold_claims(&s_claims, th);
}

/* S4: compact occupied slots; copy each group's key string into the device
 * pool. Two-pass block compaction: counter/pool_cursor are single hot
 * addresses and single-address atomic RMW serializes at ~160 M/s (probe
 * tools/probe_strcompact.hip: per-group atomics = 39 ms, wave-aggregated
 * still 78 ms at 2.4 % slot occupancy — 78 % of waves contain an occupied
 * slot — while the raw 6.4 GB slot scan is 1.1 ms at 5.9 TB/s). So: each
 * block scans its contiguous slot range twice — pass A counts groups and
 * key bytes and claims space with ONE atomic pair per block, pass B emits
 * in slot order with an in-block prefix per 256-slot tile.
 *   src.bytes(rep, &len)            the key bytes of the slot's owner
 *   wr.write(idx, off_len, slot)    output record idx; key at off_len
 * 256 threads per block (block_excl_scan2). */
template <typename Src, typename Writer>
__device__ __forceinline__ void strslot_compact(const StrSlot* slots, uint64_t nslots,
                                                const Src& src, const Writer& wr,
                                                unsigned long long* counter,
                                                char* pool,
                                                unsigned long long* pool_cursor,
                                                uint64_t pool_cap, TableHdr* th)
{
    __shared__ uint64_t wsum[4][2];
    __shared__ unsigned long long s_cbase, s_pbase;

    uint64_t per = (nslots + gridDim.x - 1) / gridDim.x;
    uint64_t b0 = (uint64_t)blockIdx.x * per;
    if (b0 > nslots) b0 = nslots;
    uint64_t b1 = b0 + per;
    if (b1 > nslots) b1 = nslots;

    /* pass A: count occupied slots + total key bytes in [b0, b1) */
    uint64_t c = 0, l = 0, tc, tl;
    for (uint64_t i = b0 + threadIdx.x; i < b1; i += blockDim.x) {
        unsigned long long rep = slots[i].rep;
        if (rep) {
            uint32_t len;
            (void)src.bytes(rep, &len);
            c++;
            l += len;
        }
    }
    block_excl_scan2(c, l, &tc, &tl, wsum);
    if (threadIdx.x == 0) {
        s_cbase = tc ? atomicAdd(counter, (unsigned long long)tc) : 0;
        s_pbase = tl ? atomicAdd(pool_cursor, (unsigned long long)tl) : 0;
    }
    __syncthreads();
    uint64_t cbase = s_cbase, pbase = s_pbase;

    /* pass B: ordered emit */
    for (uint64_t base = b0; base < b1; base += blockDim.x) {
        uint64_t i = base + threadIdx.x;
        uint64_t occ = 0, off = 0;
        uint32_t len = 0;
        const char* p = nullptr;
        if (i < b1) {
            unsigned long long rep = slots[i].rep;
            if (rep) {
                occ = 1;
                p = src.bytes(rep, &len);
                off = len;
            }
        }
        uint64_t idx = occ;
        block_excl_scan2(idx, off, &tc, &tl, wsum);
        if (occ) {
            idx += cbase;
            off += pbase;
            if (off + len > pool_cap) {
                th->overflow = 1;
            } else {
                for (uint32_t k = 0; k < len; k++) pool[off + k] = p[k];
                wr.write(idx, ((unsigned long long)off << 24) | len, slots[i]);
            }
        }
        cbase += tc;
        pbase += tl;
    }
}

struct DictEntrySrc {
    const DevSeg* segs;
    const SegEx* segex;
    int key_seg_off;
    __device__ __forceinline__ const char* bytes(unsigned long long rep,
                                                 uint32_t* len) const
    {
        const int seg = (int)(rep >> 32) - 1;
        const int64_t id = (int64_t)(rep & 0xFFFFFFFFULL);
        return dict_entry(segs[key_seg_off + seg], segex[key_seg_off + seg],
                          id - 1, len);
    }
};

struct StrGroupWriter {
    OutStrGroup* out;
    __device__ __forceinline__ void write(uint64_t idx, unsigned long long off_len,
                                          const StrSlot& sl) const
    {
        OutStrGroup& g = out[idx];
        g.off_len = off_len;
        g.sum_bits = sl.sum_bits;
        g.cnt_nonnull = sl.cnt;
    }
};

__global__ void __launch_bounds__(256)
k_strgrp_compact(const DevSeg* segs, const SegEx* segex, int key_seg_off,
                 const StrSlot* slots, uint64_t nslots,
                 OutStrGroup* out, unsigned long long* counter,
                 char* pool, unsigned long long* pool_cursor,
                 uint64_t pool_cap, TableHdr* th)
{
    strslot_compact(slots, nslots, DictEntrySrc{segs, segex, key_seg_off},
                    StrGroupWriter{out}, counter, pool, pool_cursor, pool_cap, th);
}

/* ------------------------------------------------------------------ */
/* string ids of a multi-key GROUP BY's STRING key column (common.h
 * StrKeyId): one dense id per distinct string over the
 * entries of the column's kept segments, so that the composite packer takes
 * the column as one more integer component. k_strgrp_hash gives every entry
 * its hash, ident and prefix; then
 *   k_strkey_claim   one lane per entry: find or claim the string's slot,
 *                    kmap[entry] = slot index
 *   k_strkey_compact occupied slots -> ids 0..D-1 in slot order, bytes into
 *                    the pool in id order; the id is left in the slot
 *   k_strkey_remap   kmap[entry] = the id its slot was given
 * Null entries exist in the direct layouts only (an entry is a row or a
 * run there, null by the segment's bitmap): they claim nothing and keep
 * kStrKeyNoId, which no row reads, because a null row never looks up. */

__global__ void __launch_bounds__(256)
k_strkey_claim(const DevSeg* segs, const SegEx* segex, int key_seg_off, int nsegs,
               const int64_t* kbase, const uint64_t* hashes,
               const uint64_t* idents, const ulonglong2* pfxs,
               StrSlot* slots, uint64_t nslots, uint32_t* kmap, TableHdr* th)
{
    const int64_t total = kbase[nsegs];
    __shared__ unsigned long long s_claims;
    if (threadIdx.x == 0) s_claims = 0;
    __syncthreads();
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int s = seg_of(kbase, nsegs, g);
        const DevSeg& sk = segs[key_seg_off + s];
        const SegEx& ek = segex[key_seg_off + s];
        if ((ek.flags & (32 | 64)) &&
            bm_get((const uint8_t*)sk.blob + ek.off_bitmap_bytes, g - kbase[s])) {
            kmap[g] = kStrKeyNoId;
            continue;
        }
        DictEntryKey<false> key(segs, segex, key_seg_off, nsegs, kbase, hashes,
                                idents, pfxs, g);
        bool claimed;
        StrSlot* slot = strslot_find_or_claim(slots, nslots - 1, key, &claimed);
        if (!slot) {
            th->overflow = 1;
            kmap[g] = kStrKeyNoId;
            continue;
        }
        if (claimed) atomicAdd(&s_claims, 1ULL);
        kmap[g] = (uint32_t)(slot - slots);
    }
    strslot_fold_claims(&s_claims, th);
}

/* id idx: the owner's claim word and where its bytes went; the slot keeps
 * the id (sum_bits, unused by this table) for k_strkey_remap */
struct StrKeyIdWriter {
    StrKeyId* out;
    StrSlot* slots;
    __device__ __forceinline__ void write(uint64_t idx, unsigned long long off_len,
                                          const StrSlot& sl) const
    {
        out[idx].off_len = off_len;
        out[idx].rep = sl.rep;
        slots[&sl - slots].sum_bits = idx;
    }
};

__global__ void __launch_bounds__(256)
k_strkey_compact(const DevSeg* segs, const SegEx* segex, int key_seg_off,
                 StrSlot* slots, uint64_t nslots, StrKeyId* out,
                 unsigned long long* counter, char* pool,
                 unsigned long long* pool_cursor, uint64_t pool_cap, TableHdr* th)
{
    strslot_compact(slots, nslots, DictEntrySrc{segs, segex, key_seg_off},
                    StrKeyIdWriter{out, slots}, counter, pool, pool_cursor,
                    pool_cap, th);
}

__global__ void __launch_bounds__(256)
k_strkey_remap(const StrSlot* slots, uint32_t* kmap, int64_t total)
{
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t si = kmap[g];
        if (si != kStrKeyNoId) kmap[g] = (uint32_t)slots[si].sum_bits;
    }
}

/* ------------------------------------------------------------------ */
/* general string-keyed GROUP BY (common.h StrGenAggs): any filter, the
 * whole aggregate family, all four key layouts, ragged segmentation. Same
 * three stages as the specialised kernels above — dense per-(segment,
 * dictionary id) accumulators, identity merge into StrSlot, compact — with
 * a wider accumulator record and a per-slot aggregate array beside the
 * slot table. k_strgrp_hash, the slot probe (strslot_find_or_claim over a
 * DictEntryKey) and k_strgrp_compact are shared as they are. */

/* 1-based dictionary id of row j of a string key segment; 0 = null key */
__device__ __forceinline__ uint64_t str_key_id(const DevSeg& sk, const SegEx& ek,
                                               int64_t j)
{
    if (ek.flags & 32)      /* direct dense: entry j is row j */
        return bm_get((const uint8_t*)sk.blob + ek.off_bitmap_bytes, j)
            ? 0 : (uint64_t)(j + 1);
    if (ek.flags & 8) {
        const uint64_t* ids = sk.blob + ek.off_ids_words;
        if (sk.type == YT_SEG_DICTIONARY_DENSE) return bp_get(ids, ek.w_ids, j);
    } else if (!(ek.flags & 64)) {
        return 0;           /* unknown layout: refused by the host */
    }
    /* RLE forms: the run whose start <= j (seg_value_at's search) */
    const uint64_t* starts = sk.blob + ek.off_starts_words;
    uint32_t lo = 0, hi = ek.run_count;
    while (lo + 1 < hi) {
        uint32_t mid = (lo + hi) / 2;
        if (bp_get(starts, ek.w_starts, mid) <= (uint64_t)j) lo = mid;
        else hi = mid;
    }
    if (ek.flags & 64)      /* direct RLE: entry = run, null by run bitmap */
        return bm_get((const uint8_t*)sk.blob + ek.off_bitmap_bytes, lo)
            ? 0 : (uint64_t)lo + 1;
    return bp_get(sk.blob + ek.off_ids_words, ek.w_ids, lo);
}

/* String predicate entry pass (common.h P_STR_PRED): evaluate ONE predicate
 * (op, escape, literal) on every entry of every segment of its column and
 * leave one answer bit per entry — bit id-1 of the segment's bitmap, which
 * starts at word pred_base[seg]. One wave64 owns one 64-bit word: a lane per
 * entry, __ballot assembles the word, lane 0 stores it. Every word of
 * [0, pred_base[nsegs]) is written exactly once, so the buffer needs no
 * memset and no atomics; lanes past dict_size contribute 0. Null entries
 * (direct layouts) get an arbitrary bit: null rows never look it up. */
__global__ void __launch_bounds__(256)
k_strpred_entries(const DevSeg* segs, const SegEx* segex, int seg_off, int nsegs,
                  const int64_t* pred_base, int op, int escape,
                  const char* lit, int64_t lit_len, uint64_t* bits)
{
    const int lane = threadIdx.x & 63;
    const int64_t nwords = pred_base[nsegs];
    const int64_t wstride = (int64_t)gridDim.x * 4;
    for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < nwords;
         w += wstride) {
        /* the last segment whose first word <= w: segments without entries
         * own no word and are stepped over */
        int lo = 0, hi = nsegs;
        while (lo + 1 < hi) {
            int mid = (lo + hi) / 2;
            if (pred_base[mid] <= w) lo = mid;
            else hi = mid;
        }
        const DevSeg& s = segs[seg_off + lo];
        const SegEx& e = segex[seg_off + lo];
        const int64_t j = (w - pred_base[lo]) * 64 + lane;
        int res = 0;
        if (j < (int64_t)e.dict_size) {
            uint32_t len;
            const char* t = dict_entry(s, e, j, &len);
            res = strpred_eval(op, escape, t, (int64_t)len, lit, lit_len) > 0;
        }
        const unsigned long long word = __ballot(res);
        if (lane == 0) bits[w] = word;
    }
}

/* String IN entry pass (YT_EX_IN over a STRING column): the shape of
 * k_strpred_entries — one wave64 per 64-bit answer word, a lane per entry,
 * __ballot assembles the word, lane 0 stores it; no memset, no atomics —
 * with the predicate "the entry's bytes are in the list". Each lane hashes
 * its entry (inlist.h inlist_str_hash) and probes the list's slot table; a
 * hash hit is confirmed on length and bytes. kLds: the table has at most
 * kInStrLdsSlots slots and the workgroup copies it into LDS first (16-byte
 * slots, one ds_read_b128 per probe step); otherwise the probes read global
 * memory. The list's bytes stay in global memory either way. */
template <bool kLds>
__global__ void __launch_bounds__(256)
k_inlist_str_entries(const DevSeg* segs, const SegEx* segex, int seg_off, int nsegs,
                     const int64_t* pred_base, const InStrSlot* slots,
                     uint64_t mask, const char* list_bytes, uint64_t* bits)
{
    __shared__ InStrSlot lds[kLds ? kInStrLdsSlots : 1];
    const InStrSlot* tab = slots;
    if (kLds) {
        for (uint32_t i = threadIdx.x; i <= (uint32_t)mask && i < kInStrLdsSlots;
             i += 256)
            lds[i] = slots[i];
        __syncthreads();
        tab = lds;
    }
    const int lane = threadIdx.x & 63;
    const int64_t nwords = pred_base[nsegs];
    const int64_t wstride = (int64_t)gridDim.x * 4;
    for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < nwords;
         w += wstride) {
        int lo = 0, hi = nsegs;
        while (lo + 1 < hi) {
            int mid = (lo + hi) / 2;
            if (pred_base[mid] <= w) lo = mid;
            else hi = mid;
        }
        const DevSeg& s = segs[seg_off + lo];
        const SegEx& e = segex[seg_off + lo];
        const int64_t j = (w - pred_base[lo]) * 64 + lane;
        int res = 0;
        if (j < (int64_t)e.dict_size) {
            uint32_t len;
            const char* t = dict_entry(s, e, j, &len);
            res = inlist_probe_str(tab, mask, list_bytes,
                                   inlist_str_hash(t, len), t, len);
        }
        const unsigned long long word = __ballot(res);
        if (lane == 0) bits[w] = word;
    }
}

/* ------------------------------------------------------------------ */
/* STRING-key equi-join (common.h JoinDev.key_kind = 1, strjoin.h): the   */
/* foreign table over byte hashes, and one probe per primary entry.      */

/* the key of foreign row frow: its bytes, or nullptr for a null key */
__device__ __forceinline__ const char* jforeign_str(const JoinDev& jt, int64_t frow,
                                                    uint32_t* len)
{
    const int off = jt.f_off[jt.fkey_col];
    int lo;
    if (jt.fkey_shift) {
        lo = (int)(frow >> jt.fkey_shift);
    } else {
        int hi = jt.f_cnt[jt.fkey_col];
        lo = 0;
        while (lo + 1 < hi) {
            int mid = (lo + hi) / 2;
            if (jt.fsegs[off + mid].start_row <= frow) lo = mid;
            else hi = mid;
        }
    }
    const DevSeg& s = jt.fsegs[off + lo];
    const SegEx& e = jt.fsegex[off + lo];
    const uint64_t id = str_key_id(s, e, frow - s.start_row);
    if (id == 0) return nullptr;
    return dict_entry(s, e, (int64_t)(id - 1), len);
}

/* strjoin_probe_slot's view of a slot's owner row */
struct JForeignOwner {
    const JoinDev& jt;
    __device__ const char* operator()(int64_t row, uint32_t* len) const
    {
        return jforeign_str(jt, row, len);
    }
};

/* k_join_build for STRING keys: a row claims a slot by CAS on hrow, walking
 * from its byte hash, and stores the hash in hkey. Inserts never read another
 * slot's key, so there is no publish race. The empty string is a key like any
 * other; null keys chain off null_row. inserted += the slots claimed, one
 * atomic per wave. */
__global__ void __launch_bounds__(256)
k_strjoin_build(JoinDev jt, int64_t frows, uint64_t* hkey, long long* hrow,
                unsigned long long* null_row_plus1, unsigned* error_out,
                unsigned long long* inserted)
{
    unsigned mine = 0;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < frows; r += stride) {
        uint32_t len = 0;
        const char* t = jforeign_str(jt, r, &len);
        if (!t) {
            unsigned long long prev = atomicExch(null_row_plus1,
                                                 (unsigned long long)(r + 1));
            ((int64_t*)jt.fnext)[r] = (int64_t)prev - 1;
            if (prev != 0ULL) atomicOr(error_out + 1, 1u);   /* has_dups */
            continue;
        }
        const uint64_t hash = inlist_str_hash(t, len);
        uint64_t h = hash & jt.hmask;
        for (;;) {
            unsigned long long prev = atomicCAS(
                (unsigned long long*)&hrow[h],
                (unsigned long long)(long long)-1,
                (unsigned long long)r);
            if (prev == (unsigned long long)(long long)-1) {
                hkey[h] = hash;
                mine++;
                break;
            }
            h = (h + 1) & jt.hmask;
        }
    }
    for (int sh = 32; sh >= 1; sh >>= 1) mine += __shfl_xor((int)mine, sh, 64);
    if ((threadIdx.x & 63) == 0 && mine)
        atomicAdd(inserted, (unsigned long long)mine);
}

/* k_join_chain for STRING keys, after all inserts are visible: every row
 * finds its key's canonical slot (strjoin_probe_slot: equal hash AND the
 * owner's length and bytes) and pushes itself on that slot's match list. A
 * row always finds a slot: its own lies on its probe path. */
__global__ void __launch_bounds__(256)
k_strjoin_chain(JoinDev jt, int64_t frows, unsigned* error_out)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < frows; r += stride) {
        uint32_t len = 0;
        const char* t = jforeign_str(jt, r, &len);
        if (!t) continue;
        const int64_t h = strjoin_probe_slot(jt.hkey, jt.hrow, jt.hmask,
                                             inlist_str_hash(t, len), t, len,
                                             JForeignOwner{jt});
        if (h < 0) continue;                          /* unreachable */
        int64_t prev = (int64_t)atomicExch(
            (unsigned long long*)&((int64_t*)jt.chead)[h],
            (unsigned long long)r);
        ((int64_t*)jt.fnext)[r] = prev;
        if (prev >= 0) atomicOr(error_out + 1, 1u);   /* has_dups */
    }
}

/* String join entry pass: the shape of k_strpred_entries with a 32-bit answer
 * per entry and not a bit. Entry id-1 of kept key segment seg owns
 * jmap[jbase[seg] + id-1]; a lane takes one entry, hashes its bytes, probes
 * the foreign table and stores the head of the match list (chead of the
 * canonical slot) or -1. Consecutive lanes store consecutive words, every
 * word of [0, jbase[nsegs]) exactly once: no memset, no atomics. Null entries
 * of the direct layouts get the answer of whatever bytes their offsets span
 * (none): null rows never look them up. */
__global__ void __launch_bounds__(256)
k_strjoin_entries(const DevSeg* segs, const SegEx* segex, int seg_off, int nsegs,
                  const int64_t* jbase, JoinDev jt, int32_t* jmap)
{
    const int64_t total = jbase[nsegs];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += stride) {
        /* the last segment whose first entry <= i: segments without entries
         * own no word and are stepped over */
        int lo = 0, hi = nsegs;
        while (lo + 1 < hi) {
            int mid = (lo + hi) / 2;
            if (jbase[mid] <= i) lo = mid;
            else hi = mid;
        }
        const DevSeg& s = segs[seg_off + lo];
        const SegEx& e = segex[seg_off + lo];
        uint32_t len;
        const char* t = dict_entry(s, e, i - jbase[lo], &len);
        const int64_t h = strjoin_probe_slot(jt.hkey, jt.hrow, jt.hmask,
                                             inlist_str_hash(t, len), t, len,
                                             JForeignOwner{jt});
        jmap[i] = h < 0 ? -1 : (int32_t)jt.chead[h];
    }
}

/* ------------------------------------------------------------------ */
/* scan + project with STRING projections: stable device compaction of  */
/* one window and the byte gather (common.h ProjTot, StrGatherRec).     */
/* k_scan_project has left out[r * np + pj] and pass[r]; a string value */
/* holds its entry reference (P_STR_REF). Reduce-then-scan in three     */
/* launches — no workgroup ever waits on another:                       */
/*   k_proj_tile_totals  lengths into pad_, {rows, bytes} per tile      */
/*   k_proj_scan_tiles   one workgroup: exclusive scan of the tile      */
/*                       totals, looping over them 256 at a time        */
/*   k_proj_scatter      per-tile rescan; survivors written densely in  */
/*                       row order, one gather record per string slot   */
/* A thread owns 8 CONSECUTIVE rows of its tile, so thread order is row */
/* order and the scan is stable by construction.                        */

constexpr int kProjRowsPerThread = kProjTile / 256;

/* length of the entry a P_STR_REF value points at */
__device__ __forceinline__ uint32_t str_ref_len(const DevSeg* segs, const SegEx* segex,
                                                uint64_t ref)
{
    const uint32_t seg = (uint32_t)(ref >> 32);
    uint32_t len;
    (void)dict_entry(segs[seg], segex[seg], (int64_t)(ref & 0xFFFFFFFFu), &len);
    return len;
}

__global__ void __launch_bounds__(256)
k_proj_tile_totals(const DevSeg* segs, const SegEx* segex, DevOutVal* out,
                   const uint8_t* pass, int64_t row_count, int np,
                   unsigned str_mask, ProjTot* tile_tot)
{
    __shared__ uint64_t wsum[4][2];
    const int64_t r0 = (int64_t)blockIdx.x * kProjTile
                     + (int64_t)threadIdx.x * kProjRowsPerThread;
    uint64_t rows = 0, bytes = 0;
    for (int i = 0; i < kProjRowsPerThread; i++) {
        const int64_t r = r0 + i;
        if (r >= row_count || !pass[r]) continue;
        rows++;
        for (int pj = 0; pj < np; pj++) {
            if (!((str_mask >> pj) & 1)) continue;
            DevOutVal& o = out[r * np + pj];
            if (o.type != YT_VT_STRING) continue;
            const uint32_t len = str_ref_len(segs, segex, o.bits);
            o.pad_ = len;
            bytes += len;
        }
    }
    uint64_t ta, tb;
    block_excl_scan2(rows, bytes, &ta, &tb, wsum);
    if (threadIdx.x == 0) {
        tile_tot[blockIdx.x].rows = ta;
        tile_tot[blockIdx.x].bytes = tb;
    }
}

/* ONE workgroup. tile_tot becomes the exclusive prefix, in place;
 * totals[0] = {all rows, all bytes} of the window. */
__global__ void __launch_bounds__(256)
k_proj_scan_tiles(ProjTot* tile_tot, int ntiles, ProjTot* totals)
{
    __shared__ uint64_t wsum[4][2];
    uint64_t ca = 0, cb = 0;            /* carry: uniform across the block */
    for (int base = 0; base < ntiles; base += 256) {
        const int i = base + (int)threadIdx.x;
        uint64_t a = 0, b = 0;
        if (i < ntiles) { a = tile_tot[i].rows; b = tile_tot[i].bytes; }
        uint64_t ta, tb;
        block_excl_scan2(a, b, &ta, &tb, wsum);
        if (i < ntiles) {
            tile_tot[i].rows = ca + a;
            tile_tot[i].bytes = cb + b;
        }
        ca += ta;
        cb += tb;
    }
    if (threadIdx.x == 0) { totals[0].rows = ca; totals[0].bytes = cb; }
}

/* Survivors to cout[(dense row) * np + pj], in input row order. A string
 * value becomes bits = byte offset in the window pool, pad_ = length; every
 * string slot of a surviving row gets record (dense row) * nstr + (rank of
 * pj among the string projections), a null one with len 0. */
__global__ void __launch_bounds__(256)
k_proj_scatter(const DevOutVal* out, const uint8_t* pass, int64_t row_count,
               int np, unsigned str_mask, int nstr, const ProjTot* tile_off,
               DevOutVal* cout, StrGatherRec* recs)
{
    __shared__ uint64_t wsum[4][2];
    const int64_t r0 = (int64_t)blockIdx.x * kProjTile
                     + (int64_t)threadIdx.x * kProjRowsPerThread;
    uint64_t rows = 0, bytes = 0;
    for (int i = 0; i < kProjRowsPerThread; i++) {
        const int64_t r = r0 + i;
        if (r >= row_count || !pass[r]) continue;
        rows++;
        for (int pj = 0; pj < np; pj++) {
            if (!((str_mask >> pj) & 1)) continue;
            const DevOutVal& o = out[r * np + pj];
            if (o.type == YT_VT_STRING) bytes += o.pad_;
        }
    }
    uint64_t ta, tb;
    block_excl_scan2(rows, bytes, &ta, &tb, wsum);
    uint64_t drow = tile_off[blockIdx.x].rows + rows;
    uint64_t dbyte = tile_off[blockIdx.x].bytes + bytes;
    for (int i = 0; i < kProjRowsPerThread; i++) {
        const int64_t r = r0 + i;
        if (r >= row_count || !pass[r]) continue;
        int sidx = 0;
        for (int pj = 0; pj < np; pj++) {
            DevOutVal o = out[r * np + pj];
            if ((str_mask >> pj) & 1) {
                StrGatherRec g;
                g.ref = kStrRefNull;
                g.dst = 0;
                g.len = 0;
                g.pad_ = 0;
                if (o.type == YT_VT_STRING) {
                    g.ref = o.bits;
                    g.dst = dbyte;
                    g.len = o.pad_;
                    o.bits = dbyte;
                    dbyte += o.pad_;
                }
                recs[drow * nstr + sidx] = g;
                sidx++;
            }
            cout[drow * np + pj] = o;
        }
        drow++;
    }
}

/* lengths for host-built records (scan + ORDER BY): len from ref */
__global__ void __launch_bounds__(256)
k_str_reclen(const DevSeg* segs, const SegEx* segex, StrGatherRec* recs, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t ref = recs[i].ref;
    recs[i].len = ref == kStrRefNull ? 0 : str_ref_len(segs, segex, ref);
}

/* Byte gather: record i's entry bytes -> pool[dst, dst + len). One wave64
 * per 64 records. When every length in the wave is at most kGatherSmall each
 * lane copies its own string; otherwise the wave takes the records one at a
 * time, pointer and length broadcast by __shfl, all 64 lanes copying
 * lane-strided — a multi-KB string is 64 bytes per step instead of one lane's
 * serial loop, and the byte accesses of one step share cache lines. Plain
 * byte loads and stores: source and destination alignments are unrelated.
 * A record that would end past pool_bytes is skipped (cannot happen for
 * records whose dst came from a prefix sum of these same lengths). */
constexpr uint32_t kGatherSmall = 32;

__global__ void __launch_bounds__(256)
k_str_gather(const DevSeg* segs, const SegEx* segex, const StrGatherRec* recs,
             int64_t n, char* pool, uint64_t pool_bytes)
{
    const int lane = threadIdx.x & 63;
    const int64_t wstride = (int64_t)gridDim.x * 4;
    const int64_t nwaves = (n + 63) / 64;
    for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < nwaves;
         w += wstride) {
        const int64_t i = w * 64 + lane;
        uint32_t len = 0;
        const char* src = nullptr;
        char* dst = nullptr;
        if (i < n) {
            const StrGatherRec g = recs[i];
            if (g.ref != kStrRefNull && g.len &&
                g.dst + g.len <= pool_bytes) {
                const uint32_t seg = (uint32_t)(g.ref >> 32);
                uint32_t elen;
                src = dict_entry(segs[seg], segex[seg],
                                 (int64_t)(g.ref & 0xFFFFFFFFu), &elen);
                len = g.len < elen ? g.len : elen;
                dst = pool + g.dst;
            }
        }
        if (!__any(len > kGatherSmall)) {
            for (uint32_t b = 0; b < len; b++) dst[b] = src[b];
            continue;
        }
        for (int k = 0; k < 64; k++) {
            const uint32_t kl = (uint32_t)__shfl((int)len, k, 64);
            if (!kl) continue;                         /* wave-uniform */
            const char* ks = (const char*)(uintptr_t)
                __shfl((unsigned long long)(uintptr_t)src, k, 64);
            char* kd = (char*)(uintptr_t)
                __shfl((unsigned long long)(uintptr_t)dst, k, 64);
            for (uint32_t b = lane; b < kl; b += 64) kd[b] = ks[b];
        }
    }
}

/* G1: per row — filter, aggregate arguments (eval_prog), then
 * agg_update_slot into the row's record
 *   acc[stride * (acc_base[seg] + id-1)] = { rows, {bits, nonnull} per agg }
 * with stride = 1 + 2*agg_count. Null keys go to TableHdr side group 1, as
 * in table_update_generic. Blocks take whole 2048-row tiles so a block's
 * atomics stay inside one key segment's accumulator region. */
constexpr int kStrGenTile = 2048;

__global__ void __launch_bounds__(256)
k_strgen_accum(DevPlan p, const DevSeg* segs, const SegEx* segex,
               const int32_t* col_seg_off, const int32_t* col_seg_cnt,
               int key_col, int64_t row_count, const int64_t* acc_base,
               unsigned long long* acc, TableHdr* th, unsigned* error_out)
{
    ColCtx c;
    c.segs = segs;
    c.segex = segex;
    c.col_seg_off = col_seg_off;
    c.col_seg_cnt = col_seg_cnt;
    c.error = 0;
    const int koff = col_seg_off[key_col];
    const int kcnt = col_seg_cnt[key_col];
    const int kshift = p.col_uniform_shift[key_col];
    const int stride = 1 + 2 * p.agg_count;
    DVal aggv[kMaxAggs];

    const int64_t ntiles = (row_count + kStrGenTile - 1) / kStrGenTile;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        for (int i = threadIdx.x; i < kStrGenTile; i += 256) {
            const int64_t r = t * kStrGenTile + i;
            if (r >= row_count) break;
            c.row = r;
            if (p.filter_len) {
                DVal f = eval_prog(p, c, p.filter_off, p.filter_len);
                if (c.error) { atomicMax(error_out, c.error); return; }
                if (f.null_ || f.bits == 0) continue;
            }
            for (int a = 0; a < p.agg_count; a++) {
                if (p.agg_func[a] != YT_AGG_SUM1)
                    aggv[a] = eval_prog(p, c, p.agg_off[a], p.agg_len[a]);
            }
            if (c.error) { atomicMax(error_out, c.error); return; }
            /* key row -> segment, the way col_value does it */
            int ks;
            if (kshift) {
                ks = (int)(r >> kshift);
            } else {
                int hi = kcnt;
                ks = 0;
                while (ks + 1 < hi) {
                    int mid = (ks + hi) / 2;
                    if (segs[koff + mid].start_row <= r) ks = mid;
                    else hi = mid;
                }
            }
            const DevSeg& sk = segs[koff + ks];
            const uint64_t id = str_key_id(sk, segex[koff + ks], r - sk.start_row);
            unsigned long long* cntp;
            unsigned long long* aggp;
            if (id == 0) {
                th->side_used[1] = 1;
                cntp = (unsigned long long*)&th->side_cnt[1];
                aggp = (unsigned long long*)&th->side_agg[1][0];
            } else {
                cntp = acc + (uint64_t)stride * (uint64_t)(acc_base[ks] + (int64_t)id - 1);
                aggp = cntp + 1;
            }
            atomicAdd(cntp, 1ULL);
            for (int a = 0; a < p.agg_count; a++) {
                if (p.agg_func[a] != YT_AGG_SUM1)
                    agg_update_slot(aggp + 2 * a, p, a, aggv[a]);
            }
        }
    }
}

/* G2: fold every dictionary entry that kept at least one row into its
 * slot's aggregate record slot_aggs[stride * slot index] (same layout as
 * the accumulator record; counts are full 64-bit words). The slot comes from
 * the same strslot_find_or_claim over a DictEntryKey as in k_strgrp_merge.
 * An entry whose rows were all filtered out is skipped, so it creates no
 * group. The claimer leaves the slot's own index in StrSlot.sum_bits:
 * k_strgrp_compact copies that word into OutStrGroup.sum_bits, which is how
 * k_strgen_gather finds each compacted group's record. */
__global__ void __launch_bounds__(256)
k_strgen_merge(const DevSeg* segs, const SegEx* segex, int key_seg_off, int nsegs,
               const int64_t* acc_base, const unsigned long long* acc,
               StrGenAggs ag, const uint64_t* hashes, const uint64_t* idents,
               const ulonglong2* pfxs, StrSlot* slots, uint64_t nslots,
               unsigned long long* slot_aggs, TableHdr* th)
{
    const int64_t total = acc_base[nsegs];
    const int stride = 1 + 2 * ag.count;
    __shared__ unsigned long long s_claims;
    if (threadIdx.x == 0) s_claims = 0;
    __syncthreads();
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long* rec = acc + (uint64_t)stride * (uint64_t)g;
        if (rec[0] == 0) continue;
        DictEntryKey<true> key(segs, segex, key_seg_off, nsegs, acc_base, hashes,
                         idents, pfxs, g);
        bool claimed;
        StrSlot* slot = strslot_find_or_claim(slots, nslots - 1, key, &claimed);
        if (!slot) { th->overflow = 1; continue; }
        const uint64_t sidx = (uint64_t)(slot - slots);
        if (claimed) {
            slot->sum_bits = sidx;
            atomicAdd(&s_claims, 1ULL);
        }
        unsigned long long* sa = slot_aggs + (uint64_t)stride * sidx;
        atomicAdd(sa, rec[0]);
        for (int a = 0; a < ag.count; a++) {
            const unsigned long long bits = rec[1 + 2 * a];
            const unsigned long long nn = rec[2 + 2 * a];
            const int f = ag.func[a];
            if (f == YT_AGG_SUM1 || nn == 0) continue;
            unsigned long long* ap = sa + 1 + 2 * a;
            if (f == YT_AGG_FIRST) {
                if (atomicCAS(ap + 1, 0ULL, 1ULL) == 0ULL) ap[0] = bits;
                continue;
            }
            if (f == YT_AGG_MIN || f == YT_AGG_MAX) {
                atomicMax(ap, bits);            /* already ord_map'ped */
            } else if (ag.is_double[a]) {
                atomicAdd((double*)ap, __longlong_as_double(bits));
            } else {
                atomicAdd(ap, bits);
            }
            atomicAdd(ap + 1, nn);
        }
    }
    strslot_fold_claims(&s_claims, th);
}

/* G3: after k_strgrp_compact — fetch each compacted group's aggregate
 * record through the slot index left in OutStrGroup.sum_bits. With
 * pack_state (two-phase bottom query, one sum + sum(1)s) the group is also
 * rewritten in place into the specialised path's {sum_bits, cnt|nonnull}
 * form, which is what the k_strst_* partition kernels read. */
__global__ void __launch_bounds__(256)
k_strgen_gather(OutStrGroup* groups, int64_t n, const unsigned long long* slot_aggs,
                uint64_t nslots, int agg_count, OutStrAgg* out,
                int pack_state, int sum_slot)
{
    const int stride = 1 + 2 * agg_count;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t sidx = groups[i].sum_bits;
        if (sidx >= nslots) continue;
        const unsigned long long* sa = slot_aggs + (uint64_t)stride * sidx;
        OutStrAgg o;
        o.cnt = sa[0];
        for (int a = 0; a < kMaxAggs; a++) {
            o.agg_bits[a] = a < agg_count ? sa[1 + 2 * a] : 0;
            o.agg_nonnull[a] = a < agg_count ? sa[2 + 2 * a] : 0;
        }
        out[i] = o;
        if (pack_state) {
            groups[i].sum_bits = sum_slot >= 0 ? o.agg_bits[sum_slot] : 0;
            groups[i].cnt_nonnull = (o.cnt & 0xFFFFFFFFULL)
                | ((sum_slot >= 0 ? o.agg_nonnull[sum_slot] : 0) << 32);
        }
    }
}

/* ------------------------------------------------------------------ */
/* table compaction / partition / merge                                */

__global__ void k_compact(TableHdr* th, const unsigned long long* slots,
                          int agg_count, OutGroup* out,
                          unsigned long long* counter)
{
    int stride = 2 + 2 * agg_count;
    uint64_t nslots = th->nslots;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < nslots; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long* slot = slots + i * stride;
        uint64_t key = slot[0];
        if (key == 0) continue;
        unsigned long long idx = atomicAdd(counter, 1ULL);
        OutGroup& g = out[idx];
        g.key_bits = key;
        g.key_meta = 0;
        g.cnt = slot[1];
        for (int a = 0; a < agg_count; a++) {
            g.agg_bits[a] = slot[2 + 2 * a];
            g.agg_nonnull[a] = slot[3 + 2 * a];
        }
    }
}

/* partition counting + scatter of compacted groups into YtStateRow buckets.
 * Mirrors the reference's in-process shuffle hash partition
 * (shuffling_reader.cpp:40-42: destination = hash(key) % destinationCount). */
/* per-block LDS reduction first: single-address global atomics serialize
 * at ~160 M/s (tools/probe_strcompact), and nparts is 1..64 — a per-row
 * global atomicAdd made this pair ~24 ms at 1M groups */
constexpr int kMaxParts = 64;
__global__ void k_part_count(const OutGroup* groups, int64_t n, int nparts,
                             int sum_slot, unsigned long long* counts)
{
    __shared__ unsigned lc[kMaxParts];
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) lc[i] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t h = partition_hash(groups[i].key_bits, (int)(groups[i].key_meta & 1));
        atomicAdd(&lc[h % (uint64_t)nparts], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nparts; i += blockDim.x)
        if (lc[i]) atomicAdd(&counts[i], (unsigned long long)lc[i]);
}

/* block-chunked: count my chunk, claim one global range per partition,
 * then place rows at block-local claims (order within a partition is
 * arbitrary — the merge is order-free) */
__global__ void k_part_scatter(const OutGroup* groups, int64_t n, int nparts,
                               int sum_slot, int sum_is_double, int state_func,
                               unsigned long long* cursors,
                               YtStateRow* out)
{
    __shared__ unsigned lcnt[kMaxParts];
    __shared__ unsigned lclaim[kMaxParts];
    __shared__ unsigned long long lbase[kMaxParts];
    const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    int64_t hi = lo + chunk;
    if (hi > n) hi = n;
    if (lo >= hi) return;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) { lcnt[i] = 0; lclaim[i] = 0; }
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        uint64_t h = partition_hash(groups[i].key_bits, (int)(groups[i].key_meta & 1));
        atomicAdd(&lcnt[h % (uint64_t)nparts], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nparts; i += blockDim.x)
        lbase[i] = lcnt[i] ? atomicAdd(&cursors[i], (unsigned long long)lcnt[i]) : 0;
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const OutGroup& g = groups[i];
        int knull = (int)(g.key_meta & 1);
        uint64_t h = partition_hash(g.key_bits, knull);
        int p = (int)(h % (uint64_t)nparts);
        unsigned long long pos = lbase[p] + atomicAdd(&lclaim[p], 1u);
        YtStateRow& sr = out[pos];
        sr.key_bits = g.key_bits;
        /* meta bits 8+ carry the EXACT non-null count (needed for avg; any
         * value >0 means a non-null sum) */
        uint64_t nonnull = (sum_slot >= 0) ? g.agg_nonnull[sum_slot] : 0;
        sr.meta = (uint64_t)knull | (nonnull << 8)
                | (sum_is_double ? 2ULL : 0ULL);
        uint64_t sb = (sum_slot >= 0) ? g.agg_bits[sum_slot] : 0;
        if (sum_slot >= 0 && nonnull &&
            (state_func == YT_AGG_MIN || state_func == YT_AGG_MAX)) {
            /* the table stores min/max in the order-preserving mapped space
             * (ord_map above); the exchanged STATE carries the RAW value so
             * oracle- and GPU-produced states are interchangeable */
            uint8_t vt = sum_is_double ? YT_VT_DOUBLE : YT_VT_INT64;
            sb = ord_unmap(state_func == YT_AGG_MIN ? ~sb : sb, vt);
        }
        sr.sum_bits = sb;
        sr.row_count = g.cnt;
    }
}

/* ---- string-keyed two-phase exchange (§8e; shuffling_reader.cpp key
 * shuffle applied to string group keys) ----
 * The 32-byte YtStateRow is reused with key_bits = (byte offset within the
 * state's own partition pool slice) << 24 | length; the pool slices travel
 * beside the states in the all-to-all. Partition = splitmix64(FNV-1a(key
 * bytes) [^ null marker]) % world — the byte-level mirror of
 * partition_hash, matching the oracle bit-for-bit. */
__global__ void k_strst_count(const OutStrGroup* groups, int64_t n,
                              const char* pool, int nparts,
                              unsigned long long* counts,
                              unsigned long long* byte_counts)
{
    __shared__ unsigned long long lc[kMaxParts], lb[kMaxParts];
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) { lc[i] = 0; lb[i] = 0; }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t ol = groups[i].off_len;
        uint32_t len = (uint32_t)(ol & 0xFFFFFF);
        uint64_t h = mix64(fnv1a_bytes(pool + (ol >> 24), len));
        int p = (int)(h % (uint64_t)nparts);
        atomicAdd(&lc[p], 1ULL);
        atomicAdd(&lb[p], (unsigned long long)len);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
        if (lc[i]) atomicAdd(&counts[i], lc[i]);
        if (lb[i]) atomicAdd(&byte_counts[i], lb[i]);
    }
}

/* block-chunked scatter (rows AND bytes claimed per block, order within a
 * partition arbitrary — the merge is order-free) */
__global__ void k_strst_scatter(const OutStrGroup* groups, int64_t n,
                                const char* pool, int nparts,
                                int sum_is_double,
                                unsigned long long* cursors,   /* global row idx */
                                unsigned long long* bcursors,  /* slice-local bytes */
                                YtStateRow* states, char* out_pool,
                                const unsigned long long* pool_base)
{
    __shared__ unsigned lcnt[kMaxParts], lclaim[kMaxParts];
    __shared__ unsigned long long lbytes[kMaxParts], lbclaim[kMaxParts];
    __shared__ unsigned long long lbase[kMaxParts], lbbase[kMaxParts];
    const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    int64_t hi = lo + chunk;
    if (hi > n) hi = n;
    if (lo >= hi) return;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
        lcnt[i] = 0; lclaim[i] = 0; lbytes[i] = 0; lbclaim[i] = 0;
    }
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        uint64_t ol = groups[i].off_len;
        uint32_t len = (uint32_t)(ol & 0xFFFFFF);
        uint64_t h = mix64(fnv1a_bytes(pool + (ol >> 24), len));
        int p = (int)(h % (uint64_t)nparts);
        atomicAdd(&lcnt[p], 1u);
        atomicAdd(&lbytes[p], (unsigned long long)len);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
        lbase[i] = lcnt[i] ? atomicAdd(&cursors[i], (unsigned long long)lcnt[i]) : 0;
        lbbase[i] = lbytes[i] ? atomicAdd(&bcursors[i], lbytes[i]) : 0;
    }
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const OutStrGroup& g = groups[i];
        uint64_t ol = g.off_len;
        uint32_t len = (uint32_t)(ol & 0xFFFFFF);
        const char* src = pool + (ol >> 24);
        uint64_t h = mix64(fnv1a_bytes(src, len));
        int p = (int)(h % (uint64_t)nparts);
        unsigned long long pos = lbase[p] + atomicAdd(&lclaim[p], 1u);
        unsigned long long boff = lbbase[p] + atomicAdd(&lbclaim[p],
                                                        (unsigned long long)len);
        char* dst = out_pool + pool_base[p] + boff;
        for (uint32_t k = 0; k < len; k++) dst[k] = src[k];
        YtStateRow& sr = states[pos];
        sr.key_bits = (boff << 24) | len;       /* slice-local reference */
        uint64_t nonnull = (g.cnt_nonnull >> 32) ? 1 : 0;
        sr.meta = (nonnull << 8) | (sum_is_double ? 2ULL : 0ULL);
        sr.sum_bits = g.sum_bits;
        sr.row_count = g.cnt_nonnull & 0xFFFFFFFFULL;
    }
}

/* merge side: per-state hash/ident/prefix + absolute pool offsets (the
 * received slices are concatenated; a state's slice is found by its row
 * segment) */
__global__ void k_strst_hash(const YtStateRow* states, int64_t n,
                             const int64_t* seg_row_base,
                             const unsigned long long* seg_pool_base,
                             int nsegin, const char* pool,
                             uint64_t* hashes, uint64_t* idents,
                             ulonglong2* pfxs, uint64_t* absoff)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int s = seg_of(seg_row_base, nsegin, i);
        uint64_t ol = states[i].key_bits;
        uint32_t len = (uint32_t)(ol & 0xFFFFFF);
        uint64_t ab = seg_pool_base[s] + (ol >> 24);
        absoff[i] = (ab << 24) | len;
        if (states[i].meta & 1) { idents[i] = 0; hashes[i] = 0; continue; }
        str_key_identity(pool + ab, len, &hashes[i], &idents[i], &pfxs[i]);
    }
}

/* front-query merge over string states: strslot_find_or_claim over a
 * PoolStateKey; counts are FULL u64 (slot->cnt = rows, slot->pad0_ =
 * nonnull) */
__global__ void k_strst_merge(const YtStateRow* states, int64_t n,
                              const char* pool, const uint64_t* hashes,
                              const uint64_t* idents, const ulonglong2* pfxs,
                              const uint64_t* absoff, int sum_slot,
                              StrSlot* slots, uint64_t nslots, TableHdr* th)
{
    __shared__ unsigned long long s_claims;
    if (threadIdx.x == 0) s_claims = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const YtStateRow sr = states[i];
        if (sr.meta & 1) {
            /* null-key state → side accumulator (k_merge_states pattern) */
            th->side_used[1] = 1;
            atomicAdd((unsigned long long*)&th->side_cnt[1],
                      (unsigned long long)sr.row_count);
            if (sum_slot >= 0 && (sr.meta >> 8)) {
                if (sr.meta & 2)
                    atomicAdd((double*)&th->side_agg[1][2 * sum_slot],
                              __longlong_as_double((long long)sr.sum_bits));
                else
                    atomicAdd((unsigned long long*)&th->side_agg[1][2 * sum_slot],
                              (unsigned long long)sr.sum_bits);
                atomicAdd((unsigned long long*)&th->side_agg[1][2 * sum_slot + 1],
                          (unsigned long long)(sr.meta >> 8));
            }
            continue;
        }
        PoolStateKey key(pool, absoff, hashes, idents, pfxs, i);
        bool claimed;
        StrSlot* slot = strslot_find_or_claim(slots, nslots - 1, key, &claimed);
        if (!slot) { th->overflow = 1; continue; }
        if (claimed) atomicAdd(&s_claims, 1ULL);
        atomicAdd((unsigned long long*)&slot->cnt,
                  (unsigned long long)sr.row_count);
        if (sum_slot >= 0 && (sr.meta >> 8)) {
            if (sr.meta & 2)
                atomicAdd((double*)&slot->sum_bits,
                          __longlong_as_double((long long)sr.sum_bits));
            else
                atomicAdd((unsigned long long*)&slot->sum_bits,
                          (unsigned long long)sr.sum_bits);
            atomicAdd((unsigned long long*)&slot->pad0_,
                      (unsigned long long)(sr.meta >> 8));
        }
    }
    strslot_fold_claims(&s_claims, th);
}

/* compact the merged string-state table (strslot_compact); strings come from
 * the exchanged pool via the owner state's absolute offset */
struct PoolStateSrc {
    const uint64_t* absoff;
    const char* pool;
    __device__ __forceinline__ const char* bytes(unsigned long long rep,
                                                 uint32_t* len) const
    {
        const uint64_t ab = absoff[rep - 1];
        *len = (uint32_t)(ab & 0xFFFFFF);
        return pool + (ab >> 24);
    }
};

struct StrStateWriter {
    OutStrState* out;
    __device__ __forceinline__ void write(uint64_t idx, unsigned long long off_len,
                                          const StrSlot& sl) const
    {
        OutStrState& g = out[idx];
        g.off_len = off_len;
        g.sum_bits = sl.sum_bits;
        g.cnt = sl.cnt;
        g.nonnull = sl.pad0_;
    }
};

__global__ void __launch_bounds__(256)
k_strst_compact(const StrSlot* slots, uint64_t nslots,
                const uint64_t* absoff, const char* pool,
                OutStrState* out, unsigned long long* counter,
                char* out_pool, unsigned long long* pool_cursor,
                uint64_t pool_cap, TableHdr* th)
{
    strslot_compact(slots, nslots, PoolStateSrc{absoff, pool},
                    StrStateWriter{out}, counter, out_pool, pool_cursor,
                    pool_cap, th);
}

/* merge state rows into a (fresh) table — front-query Merge semantics
 * (cg_fragment_compiler.cpp:4116-4134 + udf/sum.c sum_merge). */
__global__ void k_merge_states(const YtStateRow* states, int64_t n,
                               int agg_count, int sum_slot, int state_func,
                               TableHdr* th, unsigned long long* slots)
{
    int stride = 2 + 2 * agg_count;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const YtStateRow& sr = states[i];
        int knull = (int)(sr.meta & 1);
        unsigned long long* cntp;
        unsigned long long* aggp;
        if (knull || sr.key_bits == 0) {
            int side = knull ? 1 : 0;
            th->side_used[side] = 1;
            cntp = (unsigned long long*)&th->side_cnt[side];
            aggp = (unsigned long long*)&th->side_agg[side][0];
        } else {
            unsigned long long* slot = table_probe(th, slots, stride, sr.key_bits);
            if (!slot) continue;
            cntp = slot + 1;
            aggp = slot + 2;
        }
        atomicAdd(cntp, (unsigned long long)sr.row_count);
        if (sum_slot >= 0 && (sr.meta >> 8)) {
            if (state_func == YT_AGG_FIRST) {
                /* FirstIteration merge: the first ARRIVING non-null state
                 * claims the slot via CAS on the nonnull word (same idiom
                 * as the single-pass agg_update_slot FIRST case) */
                if (atomicCAS(aggp + 2 * sum_slot + 1, 0ULL,
                              (unsigned long long)(sr.meta >> 8)) == 0ULL)
                    aggp[2 * sum_slot] = sr.sum_bits;
                continue;
            }
            if (state_func == YT_AGG_MIN || state_func == YT_AGG_MAX) {
                /* states carry RAW values; the table accumulates in the
                 * mapped space (same convention as the single-pass table) */
                uint8_t vt = (sr.meta & 2) ? YT_VT_DOUBLE : YT_VT_INT64;
                uint64_t m = ord_map(sr.sum_bits, vt);
                atomicMax(aggp + 2 * sum_slot,
                          (unsigned long long)(state_func == YT_AGG_MIN ? ~m : m));
            } else if (sr.meta & 2) {
                /* double sum state: FP merge (udf/sum.c:27-35) */
                atomicAdd((double*)(aggp + 2 * sum_slot),
                          __longlong_as_double((long long)sr.sum_bits));
            } else {
                atomicAdd(aggp + 2 * sum_slot, (unsigned long long)sr.sum_bits);
            }
            /* states carry EXACT non-null counts (avg = sum/count) */
            atomicAdd(aggp + 2 * sum_slot + 1,
                      (unsigned long long)(sr.meta >> 8));
        }
    }
}

} /* namespace ytql */

/* ------------------------------------------------------------------ */
/* extern-C launch wrappers (called from evaluator.cpp)                */

using namespace ytql;

extern "C" {

hipError_t ytql_launch_parse_segments(const DevSeg* segs, int nsegs, SegEx* out,
                                      unsigned* max_width, unsigned* col_null_flags,
                                      unsigned long long* col_zzmin,
                                      unsigned long long* col_zzmax,
                                      hipStream_t st)
{
    int block = 256;
    int grid = (nsegs + block - 1) / block;
    hipLaunchKernelGGL(k_parse_segments, dim3(grid), dim3(block), 0, st,
                       segs, nsegs, out, max_width, col_null_flags,
                       col_zzmin, col_zzmax);
    return hipGetLastError();
}

hipError_t ytql_launch_scan_nullflags(const DevSeg* segs, const SegEx* segex,
                                      int nsegs, unsigned* col_null_flags,
                                      hipStream_t st)
{
    hipLaunchKernelGGL(k_scan_nullflags, dim3(nsegs), dim3(256), 0, st,
                       segs, segex, nsegs, col_null_flags);
    return hipGetLastError();
}

hipError_t ytql_launch_scan_zzrange(const DevSeg* segs, const SegEx* segex,
                                    int seg_off, int seg_cnt, int has_nulls,
                                    unsigned long long* out, hipStream_t st)
{
    hipLaunchKernelGGL(k_scan_zzrange, dim3(seg_cnt), dim3(256), 0, st,
                       segs, segex, seg_off, has_nulls, out);
    return hipGetLastError();
}

hipError_t ytql_launch_scan_partition(const PartParams* pp, const DevSeg* segs,
                                      const SegEx* segex, const FastCol* cols,
                                      TableHdr* th,
                                      unsigned long long* cursors, void* recs,
                                      unsigned long long* ncursors, uint64_t* nrecs,
                                      int grid, hipStream_t st)
{
    /* 64 KiB record scratch + histograms: above the 64 KiB a launch may
     * request by default, so raise the kernel's limit first, once per
     * device and instantiation */
    static std::atomic<bool> raised[3][64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (pp->plain_mode && !pp->packed_mode) return hipErrorInvalidValue;
    const int inst = pp->plain_mode ? 2 : pp->packed_mode ? 1 : 0;
    if (dev < 0 || dev >= 64 || !raised[inst][dev].load(std::memory_order_acquire)) {
        const void* fn = inst == 2 ? (const void*)k_scan_partition<true, true>
                       : inst == 1 ? (const void*)k_scan_partition<true, false>
                                   : (const void*)k_scan_partition<false, false>;
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kPartLdsBytes);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) raised[inst][dev].store(true, std::memory_order_release);
    }
    if (inst == 2)
        hipLaunchKernelGGL((k_scan_partition<true, true>), dim3(grid), dim3(kPartThreads),
                           kPartLdsBytes, st, *pp, segs, segex, cols, th, cursors,
                           (ulonglong2*)recs, ncursors, nrecs);
    else if (inst == 1)
        hipLaunchKernelGGL((k_scan_partition<true, false>), dim3(grid), dim3(kPartThreads),
                           kPartLdsBytes, st, *pp, segs, segex, cols, th, cursors,
                           (ulonglong2*)recs, ncursors, nrecs);
    else
        hipLaunchKernelGGL((k_scan_partition<false, false>), dim3(grid), dim3(kPartThreads),
                           kPartLdsBytes, st, *pp, segs, segex, cols, th, cursors,
                           (ulonglong2*)recs, ncursors, nrecs);
    return hipGetLastError();
}

hipError_t ytql_launch_bucket_agg(const void* recs, const unsigned long long* cursors,
                                  int64_t bucket_stride,
                                  const uint64_t* nrecs, const unsigned long long* ncursors,
                                  int64_t nbucket_stride,
                                  OutGroup* out, unsigned long long* out_counter,
                                  int64_t out_cap, int slim,
                                  TableHdr* th, int sum_slot, int agg_count,
                                  int packed_mode, int bits_k,
                                  uint64_t gmin_k, uint64_t gmin_v,
                                  int nsub, hipStream_t st)
{
    hipLaunchKernelGGL(k_bucket_agg, dim3(kNB), dim3(256), 0, st,
                       (const ulonglong2*)recs, cursors, bucket_stride,
                       nrecs, ncursors, nbucket_stride,
                       out, out_counter, out_cap, slim, th, sum_slot, agg_count,
                       packed_mode, bits_k, gmin_k, gmin_v, nsub);
    return hipGetLastError();
}

hipError_t ytql_launch_bucket_agg_direct(const void* recs, const unsigned long long* cursors,
                                         int64_t bucket_stride,
                                         const uint64_t* nrecs, const unsigned long long* ncursors,
                                         int64_t nbucket_stride,
                                         OutGroup* out, unsigned long long* out_counter,
                                         int64_t out_cap, int slim,
                                         TableHdr* th, int sum_slot, int agg_count,
                                         int packed_mode, int bits_k,
                                         uint64_t gmin_k, uint64_t gmin_v,
                                         int dshift, int nsub, hipStream_t st)
{
    /* the table and the flush's scan words: at dshift 12 that is 64 KiB + 64
     * bytes, above what a launch may request by default, so raise the
     * kernel's limit first, once per device */
    static std::atomic<bool> raised[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !raised[dev].load(std::memory_order_acquire)) {
        e = hipFuncSetAttribute((const void*)k_bucket_agg_direct,
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kBucketDirectLdsMax);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) raised[dev].store(true, std::memory_order_release);
    }
    size_t lds = ((size_t)16 << dshift) + kFlushScanWords * sizeof(unsigned long long);
    if (lds > kBucketDirectLdsMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bucket_agg_direct, dim3(kNB), dim3(256), lds, st,
                       (const ulonglong2*)recs, cursors, bucket_stride,
                       nrecs, ncursors, nbucket_stride,
                       out, out_counter, out_cap, slim, th, sum_slot, agg_count,
                       packed_mode, bits_k, gmin_k, gmin_v, dshift, nsub);
    return hipGetLastError();
}

hipError_t ytql_launch_topk_hist(const DevPlan* p, const DevSeg* segs,
                                 const SegEx* segex,
                                 const int32_t* col_seg_off,
                                 const int32_t* col_seg_cnt,
                                 int64_t row_count, const JoinDev* jd,
                                 const JoinDev* jd2, const TopkPass* tp,
                                 unsigned long long* bins,
                                 unsigned long long* null_cnt,
                                 unsigned* error_out, hipStream_t st)
{
    int block = 256;
    int64_t want = (row_count + block - 1) / block;
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_topk_hist, dim3(grid), dim3(block), 0, st,
                       *p, segs, segex, col_seg_off, col_seg_cnt, row_count,
                       *jd, *jd2, *tp, bins, null_cnt, error_out);
    return hipGetLastError();
}

hipError_t ytql_launch_topk_hist_fast(const DevSeg* segs, const SegEx* segex,
                                      int seg_off, int shift, int64_t n,
                                      int has_nulls, int is_signed,
                                      const TopkPass* tp,
                                      unsigned long long* bins,
                                      unsigned long long* misc, hipStream_t st)
{
    int block = 256;
    int64_t want = (n + 4 * block - 1) / (4 * block);
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_topk_hist_fast, dim3(grid), dim3(block), 0, st,
                       segs, segex, seg_off, shift, n, has_nulls, is_signed,
                       *tp, bins, misc);
    return hipGetLastError();
}

hipError_t ytql_launch_topk_gather_fast(const DevSeg* segs, const SegEx* segex,
                                        int seg_off, int shift, int64_t n,
                                        int has_nulls, int is_signed,
                                        const TopkGather* tg,
                                        int64_t* rows_strict, unsigned long long* ctr_strict,
                                        int64_t* rows_tie, unsigned long long* ctr_tie,
                                        int64_t* rows_null, unsigned long long* ctr_null,
                                        hipStream_t st)
{
    int block = 256;
    int64_t want = (n + 4 * block - 1) / (4 * block);
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_topk_gather_fast, dim3(grid), dim3(block), 0, st,
                       segs, segex, seg_off, shift, n, has_nulls, is_signed,
                       *tg, rows_strict, ctr_strict, rows_tie, ctr_tie,
                       rows_null, ctr_null);
    return hipGetLastError();
}

hipError_t ytql_launch_versioned_read(const VSegDev* segs, int nseg,
                                      int64_t total_rows, uint64_t timestamp,
                                      uint64_t* out_bits, uint8_t* out_null,
                                      uint8_t* out_vis, uint8_t* out_agg,
                                      hipStream_t st)
{
    int block = 256;
    int64_t want = (total_rows + block - 1) / block;
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_versioned_read, dim3(grid), dim3(block), 0, st,
                       segs, nseg, total_rows, timestamp,
                       out_bits, out_null, out_vis, out_agg);
    return hipGetLastError();
}

hipError_t ytql_launch_unvcol_to_arrays(const DevSeg* segs, const SegEx* segex,
                                        int seg_off, int seg_cnt, int64_t n,
                                        uint64_t* out_bits, uint8_t* out_null,
                                        unsigned* error_out, hipStream_t st)
{
    int block = 256;
    int64_t want = (n + block - 1) / block;
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_unvcol_to_arrays, dim3(grid), dim3(block), 0, st,
                       segs, segex, seg_off, seg_cnt, n, out_bits, out_null,
                       error_out);
    return hipGetLastError();
}

hipError_t ytql_launch_vis_count(const uint8_t* vis, int64_t n,
                                 unsigned long long* block_counts, int grid,
                                 hipStream_t st)
{
    hipLaunchKernelGGL(k_vis_count, dim3(grid), dim3(256), 0, st,
                       vis, n, block_counts);
    return hipGetLastError();
}

hipError_t ytql_launch_vis_scatter(const uint8_t* vis, const uint8_t* nulls,
                                   const uint64_t* bits, int64_t n,
                                   const unsigned long long* block_bases,
                                   uint64_t seg_rows_cap,
                                   const int64_t* seg_blob_off,
                                   char* out_blob, int is_double,
                                   int grid, hipStream_t st)
{
    hipLaunchKernelGGL(k_vis_scatter, dim3(grid), dim3(256), 0, st,
                       vis, nulls, bits, n, block_bases, seg_rows_cap,
                       seg_blob_off, out_blob, is_double);
    return hipGetLastError();
}

hipError_t ytql_launch_join_build(const JoinDev* jd, int64_t frows,
                                  uint64_t* hkey, long long* hrow,
                                  unsigned long long* null_row_plus1,
                                  unsigned* error_out, hipStream_t st)
{
    int block = 256;
    int64_t want = (frows + block - 1) / block;
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_join_build, dim3(grid), dim3(block), 0, st,
                       *jd, frows, hkey, hrow, null_row_plus1, error_out);
    return hipGetLastError();
}

hipError_t ytql_launch_join_chain(const JoinDev* jd, int64_t frows,
                                   unsigned* error_out, hipStream_t st)
{
    int block = 256;
    int64_t want = (frows + block - 1) / block;
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_join_chain, dim3(grid), dim3(block), 0, st,
                       *jd, frows, error_out);
    return hipGetLastError();
}

hipError_t ytql_launch_strjoin_build(const JoinDev* jd, int64_t frows,
                                     uint64_t* hkey, long long* hrow,
                                     unsigned long long* null_row_plus1,
                                     unsigned* error_out,
                                     unsigned long long* inserted, hipStream_t st)
{
    int block = 256;
    int64_t want = (frows + block - 1) / block;
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_strjoin_build, dim3(grid), dim3(block), 0, st,
                       *jd, frows, hkey, hrow, null_row_plus1, error_out, inserted);
    return hipGetLastError();
}

hipError_t ytql_launch_strjoin_chain(const JoinDev* jd, int64_t frows,
                                     unsigned* error_out, hipStream_t st)
{
    int block = 256;
    int64_t want = (frows + block - 1) / block;
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_strjoin_chain, dim3(grid), dim3(block), 0, st,
                       *jd, frows, error_out);
    return hipGetLastError();
}

/* entries = jbase[nsegs], the length of jmap */
hipError_t ytql_launch_strjoin_entries(const DevSeg* segs, const SegEx* segex,
                                       int seg_off, int nsegs,
                                       const int64_t* jbase, int64_t entries,
                                       const JoinDev* jd, int32_t* jmap,
                                       hipStream_t st)
{
    int64_t want = (entries + 255) / 256;
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_strjoin_entries, dim3(grid), dim3(256), 0, st,
                       segs, segex, seg_off, nsegs, jbase, *jd, jmap);
    return hipGetLastError();
}

hipError_t ytql_launch_topk_gather(const DevPlan* p, const DevSeg* segs,
                                   const SegEx* segex,
                                   const int32_t* col_seg_off,
                                   const int32_t* col_seg_cnt,
                                   int64_t row_count, const JoinDev* jd,
                                   const JoinDev* jd2, const TopkGather* tg,
                                   int64_t* rows_strict, unsigned long long* ctr_strict,
                                   int64_t* rows_tie, unsigned long long* ctr_tie,
                                   int64_t* rows_null, unsigned long long* ctr_null,
                                   unsigned* error_out, hipStream_t st)
{
    int block = 256;
    int64_t want = (row_count + block - 1) / block;
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_topk_gather, dim3(grid), dim3(block), 0, st,
                       *p, segs, segex, col_seg_off, col_seg_cnt, row_count,
                       *jd, *jd2, *tg, rows_strict, ctr_strict, rows_tie, ctr_tie,
                       rows_null, ctr_null, error_out);
    return hipGetLastError();
}

hipError_t ytql_launch_topk_materialize(const DevPlan* p, const DevSeg* segs,
                                        const SegEx* segex,
                                        const int32_t* col_seg_off,
                                        const int32_t* col_seg_cnt,
                                        const JoinDev* jd,
                                        const JoinDev* jd2,
                                        const int64_t* rows, int64_t m,
                                        DevOutVal* out, unsigned* error_out,
                                        hipStream_t st)
{
    int block = 256;
    int64_t want = (m + block - 1) / block;
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_topk_materialize, dim3(grid), dim3(block), 0, st,
                       *p, segs, segex, col_seg_off, col_seg_cnt, *jd, *jd2,
                       rows, m, out, error_out);
    return hipGetLastError();
}

hipError_t ytql_launch_scan_project(const DevPlan* p, const DevSeg* segs,
                                    const SegEx* segex,
                                    const int32_t* col_seg_off,
                                    const int32_t* col_seg_cnt,
                                    int64_t row_base,
                                    int64_t row_count, const JoinDev* jd,
                                    const JoinDev* jd2, DevOutVal* out,
                                    uint8_t* pass, unsigned* error_out,
                                    hipStream_t st)
{
    int block = 256;
    int64_t want = (row_count + block - 1) / block;
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_scan_project, dim3(grid), dim3(block), 0, st,
                       *p, segs, segex, col_seg_off, col_seg_cnt, row_base,
                       row_count, *jd, *jd2, out, pass, error_out);
    return hipGetLastError();
}

/* the two reduce-then-scan launches over one scan+project window: per-tile
 * totals, then the scan of the tile totals (tile_tot needs
 * ceil(row_count / kProjTile) entries; totals one) */
hipError_t ytql_launch_proj_offsets(const DevSeg* segs, const SegEx* segex,
                                    DevOutVal* out, const uint8_t* pass,
                                    int64_t row_count, int np, unsigned str_mask,
                                    ProjTot* tile_tot, ProjTot* totals,
                                    hipStream_t st)
{
    const int ntiles = (int)((row_count + kProjTile - 1) / kProjTile);
    hipLaunchKernelGGL(k_proj_tile_totals, dim3(ntiles), dim3(256), 0, st,
                       segs, segex, out, pass, row_count, np, str_mask, tile_tot);
    hipLaunchKernelGGL(k_proj_scan_tiles, dim3(1), dim3(256), 0, st,
                       tile_tot, ntiles, totals);
    return hipGetLastError();
}

hipError_t ytql_launch_proj_scatter(const DevOutVal* out, const uint8_t* pass,
                                    int64_t row_count, int np, unsigned str_mask,
                                    int nstr, const ProjTot* tile_off,
                                    DevOutVal* cout, StrGatherRec* recs,
                                    hipStream_t st)
{
    const int ntiles = (int)((row_count + kProjTile - 1) / kProjTile);
    hipLaunchKernelGGL(k_proj_scatter, dim3(ntiles), dim3(256), 0, st,
                       out, pass, row_count, np, str_mask, nstr, tile_off,
                       cout, recs);
    return hipGetLastError();
}

hipError_t ytql_launch_str_reclen(const DevSeg* segs, const SegEx* segex,
                                  StrGatherRec* recs, int64_t n, hipStream_t st)
{
    const int grid = (int)((n + 255) / 256);
    hipLaunchKernelGGL(k_str_reclen, dim3(grid), dim3(256), 0, st,
                       segs, segex, recs, n);
    return hipGetLastError();
}

hipError_t ytql_launch_str_gather(const DevSeg* segs, const SegEx* segex,
                                  const StrGatherRec* recs, int64_t n,
                                  char* pool, uint64_t pool_bytes, hipStream_t st)
{
    const int64_t want = (n + 255) / 256;       /* 4 waves of 64 records */
    const int grid = (int)(want > 8192 ? 8192 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_str_gather, dim3(grid), dim3(256), 0, st,
                       segs, segex, recs, n, pool, pool_bytes);
    return hipGetLastError();
}

hipError_t ytql_launch_scan_generic(const DevPlan* p, const DevSeg* segs,
                                    const SegEx* segex,
                                    const int32_t* col_seg_off,
                                    const int32_t* col_seg_cnt,
                                    int64_t row_count, const JoinDev* jd,
                                    const JoinDev* jd2,
                                    TableHdr* th, unsigned long long* slots,
                                    unsigned* error_out, const StrKeyDev* sk,
                                    hipStream_t st)
{
    int block = 256;
    int64_t want = (row_count + block - 1) / block;
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_scan_generic, dim3(grid), dim3(block), 0, st,
                       *p, segs, segex, col_seg_off, col_seg_cnt, row_count,
                       *jd, *jd2, th, slots, error_out, *sk);
    return hipGetLastError();
}

hipError_t ytql_launch_scan_fast(const FastParams* fp, const DevSeg* segs,
                                 const SegEx* segex, const FastCol* cols,
                                 TableHdr* th, unsigned long long* slots,
                                 unsigned long long* gaccum,
                                 size_t lds_bytes, int grid, hipStream_t st)
{
    hipLaunchKernelGGL(k_scan_fast, dim3(grid), dim3(256), lds_bytes, st,
                       *fp, segs, segex, cols, th, slots, gaccum);
    return hipGetLastError();
}

hipError_t ytql_launch_compact(TableHdr* th_host_nslots, TableHdr* th,
                               const unsigned long long* slots, int agg_count,
                               OutGroup* out, unsigned long long* counter,
                               uint64_t nslots, hipStream_t st)
{
    int block = 256;
    uint64_t want = (nslots + block - 1) / block;
    int grid = (int)(want > 2048 ? 2048 : (want ? want : 1));
    hipLaunchKernelGGL(k_compact, dim3(grid), dim3(block), 0, st,
                       th, slots, agg_count, out, counter);
    return hipGetLastError();
}

hipError_t ytql_launch_part_count(const OutGroup* groups, int64_t n, int nparts,
                                  int sum_slot, unsigned long long* counts,
                                  hipStream_t st)
{
    int block = 256;
    int64_t want = (n + block - 1) / block;
    int grid = (int)(want > 2048 ? 2048 : (want ? want : 1));
    hipLaunchKernelGGL(k_part_count, dim3(grid), dim3(block), 0, st,
                       groups, n, nparts, sum_slot, counts);
    return hipGetLastError();
}

hipError_t ytql_launch_part_scatter(const OutGroup* groups, int64_t n, int nparts,
                                    int sum_slot, int sum_is_double,
                                    int state_func,
                                    unsigned long long* cursors,
                                    YtStateRow* out, hipStream_t st)
{
    int block = 256;
    int64_t want = (n + block - 1) / block;
    int grid = (int)(want > 2048 ? 2048 : (want ? want : 1));
    hipLaunchKernelGGL(k_part_scatter, dim3(grid), dim3(block), 0, st,
                       groups, n, nparts, sum_slot, sum_is_double, state_func,
                       cursors, out);
    return hipGetLastError();
}

hipError_t ytql_launch_strgrp_accum(const StrGroupParams* sp, const DevSeg* segs,
                                    const SegEx* segex, const int64_t* acc_base,
                                    unsigned long long* acc, TableHdr* th,
                                    hipStream_t st)
{
    int grid = sp->ntiles < 2048 ? (sp->ntiles ? sp->ntiles : 1) : 2048;
    hipLaunchKernelGGL(k_strgrp_accum, dim3(grid), dim3(256), 0, st,
                       *sp, segs, segex, acc_base, acc, th);
    return hipGetLastError();
}

hipError_t ytql_launch_strgrp_hash(const DevSeg* segs, const SegEx* segex,
                                   int key_seg_off, int nsegs,
                                   const int64_t* acc_base, uint64_t* hashes,
                                   uint64_t* idents, ulonglong2* pfxs,
                                   int64_t total, hipStream_t st)
{
    int64_t want = (total + 255) / 256;
    int grid = (int)(want > 4096 ? 4096 : (want ? want : 1));
    hipLaunchKernelGGL(k_strgrp_hash, dim3(grid), dim3(256), 0, st,
                       segs, segex, key_seg_off, nsegs, acc_base, hashes,
                       idents, pfxs);
    return hipGetLastError();
}

hipError_t ytql_launch_strgrp_merge(const DevSeg* segs, const SegEx* segex,
                                    int key_seg_off, int nsegs,
                                    const int64_t* acc_base,
                                    const unsigned long long* acc,
                                    const uint64_t* hashes,
                                    const uint64_t* idents, const ulonglong2* pfxs,
                                    StrSlot* slots, uint64_t nslots,
                                    int val_is_double, TableHdr* th,
                                    int64_t total, hipStream_t st)
{
    int64_t want = (total + 255) / 256;
    int grid = (int)(want > 4096 ? 4096 : (want ? want : 1));
    hipLaunchKernelGGL(k_strgrp_merge, dim3(grid), dim3(256), 0, st,
                       segs, segex, key_seg_off, nsegs, acc_base, acc, hashes,
                       idents, pfxs, slots, nslots, val_is_double, th);
    return hipGetLastError();
}

hipError_t ytql_launch_strgrp_compact(const DevSeg* segs, const SegEx* segex,
                                      int key_seg_off,
                                      const StrSlot* slots, uint64_t nslots,
                                      OutStrGroup* out, unsigned long long* counter,
                                      char* pool, unsigned long long* pool_cursor,
                                      uint64_t pool_cap, TableHdr* th,
                                      hipStream_t st)
{
    uint64_t want = (nslots + 255) / 256;
    int grid = (int)(want > 2048 ? 2048 : (want ? want : 1));
    hipLaunchKernelGGL(k_strgrp_compact, dim3(grid), dim3(256), 0, st,
                       segs, segex, key_seg_off, slots, nslots, out, counter,
                       pool, pool_cursor, pool_cap, th);
    return hipGetLastError();
}

hipError_t ytql_launch_strkey_claim(const DevSeg* segs, const SegEx* segex,
                                    int key_seg_off, int nsegs,
                                    const int64_t* kbase, const uint64_t* hashes,
                                    const uint64_t* idents, const ulonglong2* pfxs,
                                    StrSlot* slots, uint64_t nslots,
                                    uint32_t* kmap, TableHdr* th,
                                    int64_t total, hipStream_t st)
{
    int64_t want = (total + 255) / 256;
    int grid = (int)(want > 4096 ? 4096 : (want ? want : 1));
    hipLaunchKernelGGL(k_strkey_claim, dim3(grid), dim3(256), 0, st,
                       segs, segex, key_seg_off, nsegs, kbase, hashes, idents,
                       pfxs, slots, nslots, kmap, th);
    return hipGetLastError();
}

hipError_t ytql_launch_strkey_compact(const DevSeg* segs, const SegEx* segex,
                                      int key_seg_off,
                                      StrSlot* slots, uint64_t nslots,
                                      StrKeyId* out, unsigned long long* counter,
                                      char* pool, unsigned long long* pool_cursor,
                                      uint64_t pool_cap, TableHdr* th,
                                      hipStream_t st)
{
    uint64_t want = (nslots + 255) / 256;
    int grid = (int)(want > 2048 ? 2048 : (want ? want : 1));
    hipLaunchKernelGGL(k_strkey_compact, dim3(grid), dim3(256), 0, st,
                       segs, segex, key_seg_off, slots, nslots, out, counter,
                       pool, pool_cursor, pool_cap, th);
    return hipGetLastError();
}

hipError_t ytql_launch_strkey_remap(const StrSlot* slots, uint32_t* kmap,
                                    int64_t total, hipStream_t st)
{
    int64_t want = (total + 255) / 256;
    int grid = (int)(want > 4096 ? 4096 : (want ? want : 1));
    hipLaunchKernelGGL(k_strkey_remap, dim3(grid), dim3(256), 0, st,
                       slots, kmap, total);
    return hipGetLastError();
}

hipError_t ytql_launch_strpred_entries(const DevSeg* segs, const SegEx* segex,
                                       int seg_off, int nsegs,
                                       const int64_t* pred_base,
                                       int64_t nwords, int op, int escape,
                                       const char* lit, int64_t lit_len,
                                       uint64_t* bits, hipStream_t st)
{
    int64_t want = (nwords + 3) / 4;      /* one wave64 per word */
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_strpred_entries, dim3(grid), dim3(256), 0, st,
                       segs, segex, seg_off, nsegs, pred_base, op, escape,
                       lit, lit_len, bits);
    return hipGetLastError();
}

/* use_lds != 0 needs mask + 1 <= kInStrLdsSlots */
hipError_t ytql_launch_inlist_str_entries(const DevSeg* segs, const SegEx* segex,
                                          int seg_off, int nsegs,
                                          const int64_t* pred_base,
                                          int64_t nwords, const InStrSlot* slots,
                                          uint64_t mask, const char* list_bytes,
                                          int use_lds, uint64_t* bits,
                                          hipStream_t st)
{
    int64_t want = (nwords + 3) / 4;      /* one wave64 per word */
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    if (use_lds && mask + 1 > kInStrLdsSlots) return hipErrorInvalidValue;
    if (use_lds)
        hipLaunchKernelGGL(k_inlist_str_entries<true>, dim3(grid), dim3(256), 0, st,
                           segs, segex, seg_off, nsegs, pred_base, slots, mask,
                           list_bytes, bits);
    else
        hipLaunchKernelGGL(k_inlist_str_entries<false>, dim3(grid), dim3(256), 0, st,
                           segs, segex, seg_off, nsegs, pred_base, slots, mask,
                           list_bytes, bits);
    return hipGetLastError();
}

hipError_t ytql_launch_strgen_accum(const DevPlan* p, const DevSeg* segs,
                                    const SegEx* segex,
                                    const int32_t* col_seg_off,
                                    const int32_t* col_seg_cnt,
                                    int key_col, int64_t row_count,
                                    const int64_t* acc_base,
                                    unsigned long long* acc, TableHdr* th,
                                    unsigned* error_out, hipStream_t st)
{
    int64_t want = (row_count + kStrGenTile - 1) / kStrGenTile;
    int grid = (int)(want > 4096 ? 4096 : (want > 0 ? want : 1));
    hipLaunchKernelGGL(k_strgen_accum, dim3(grid), dim3(256), 0, st,
                       *p, segs, segex, col_seg_off, col_seg_cnt, key_col,
                       row_count, acc_base, acc, th, error_out);
    return hipGetLastError();
}

hipError_t ytql_launch_strgen_merge(const DevSeg* segs, const SegEx* segex,
                                    int key_seg_off, int nsegs,
                                    const int64_t* acc_base,
                                    const unsigned long long* acc,
                                    const StrGenAggs* ag,
                                    const uint64_t* hashes,
                                    const uint64_t* idents, const ulonglong2* pfxs,
                                    StrSlot* slots, uint64_t nslots,
                                    unsigned long long* slot_aggs, TableHdr* th,
                                    int64_t total, hipStream_t st)
{
    int64_t want = (total + 255) / 256;
    int grid = (int)(want > 4096 ? 4096 : (want ? want : 1));
    hipLaunchKernelGGL(k_strgen_merge, dim3(grid), dim3(256), 0, st,
                       segs, segex, key_seg_off, nsegs, acc_base, acc, *ag,
                       hashes, idents, pfxs, slots, nslots, slot_aggs, th);
    return hipGetLastError();
}

hipError_t ytql_launch_strgen_gather(OutStrGroup* groups, int64_t n,
                                     const unsigned long long* slot_aggs,
                                     uint64_t nslots, int agg_count,
                                     OutStrAgg* out, int pack_state,
                                     int sum_slot, hipStream_t st)
{
    int64_t want = (n + 255) / 256;
    int grid = (int)(want > 2048 ? 2048 : (want ? want : 1));
    hipLaunchKernelGGL(k_strgen_gather, dim3(grid), dim3(256), 0, st,
                       groups, n, slot_aggs, nslots, agg_count, out,
                       pack_state, sum_slot);
    return hipGetLastError();
}

hipError_t ytql_launch_strst_count(const OutStrGroup* groups, int64_t n,
                                   const char* pool, int nparts,
                                   unsigned long long* counts,
                                   unsigned long long* byte_counts,
                                   hipStream_t st)
{
    int64_t want = (n + 255) / 256;
    int grid = (int)(want > 2048 ? 2048 : (want ? want : 1));
    hipLaunchKernelGGL(k_strst_count, dim3(grid), dim3(256), 0, st,
                       groups, n, pool, nparts, counts, byte_counts);
    return hipGetLastError();
}

hipError_t ytql_launch_strst_scatter(const OutStrGroup* groups, int64_t n,
                                     const char* pool, int nparts,
                                     int sum_is_double,
                                     unsigned long long* cursors,
                                     unsigned long long* bcursors,
                                     YtStateRow* states, char* out_pool,
                                     const unsigned long long* pool_base,
                                     hipStream_t st)
{
    int64_t want = (n + 255) / 256;
    int grid = (int)(want > 2048 ? 2048 : (want ? want : 1));
    hipLaunchKernelGGL(k_strst_scatter, dim3(grid), dim3(256), 0, st,
                       groups, n, pool, nparts, sum_is_double, cursors,
                       bcursors, states, out_pool, pool_base);
    return hipGetLastError();
}

hipError_t ytql_launch_strst_hash(const YtStateRow* states, int64_t n,
                                  const int64_t* seg_row_base,
                                  const unsigned long long* seg_pool_base,
                                  int nsegin, const char* pool,
                                  uint64_t* hashes, uint64_t* idents,
                                  ulonglong2* pfxs, uint64_t* absoff,
                                  hipStream_t st)
{
    int64_t want = (n + 255) / 256;
    int grid = (int)(want > 2048 ? 2048 : (want ? want : 1));
    hipLaunchKernelGGL(k_strst_hash, dim3(grid), dim3(256), 0, st,
                       states, n, seg_row_base, seg_pool_base, nsegin, pool,
                       hashes, idents, pfxs, absoff);
    return hipGetLastError();
}

hipError_t ytql_launch_strst_merge(const YtStateRow* states, int64_t n,
                                   const char* pool, const uint64_t* hashes,
                                   const uint64_t* idents,
                                   const ulonglong2* pfxs,
                                   const uint64_t* absoff, int sum_slot,
                                   StrSlot* slots, uint64_t nslots,
                                   TableHdr* th, hipStream_t st)
{
    int64_t want = (n + 255) / 256;
    int grid = (int)(want > 4096 ? 4096 : (want ? want : 1));
    hipLaunchKernelGGL(k_strst_merge, dim3(grid), dim3(256), 0, st,
                       states, n, pool, hashes, idents, pfxs, absoff,
                       sum_slot, slots, nslots, th);
    return hipGetLastError();
}

hipError_t ytql_launch_strst_compact(const StrSlot* slots, uint64_t nslots,
                                     const uint64_t* absoff, const char* pool,
                                     OutStrState* out,
                                     unsigned long long* counter,
                                     char* out_pool,
                                     unsigned long long* pool_cursor,
                                     uint64_t pool_cap, TableHdr* th,
                                     hipStream_t st)
{
    uint64_t want = (nslots + 255) / 256;
    int grid = (int)(want > 2048 ? 2048 : (want ? want : 1));
    hipLaunchKernelGGL(k_strst_compact, dim3(grid), dim3(256), 0, st,
                       slots, nslots, absoff, pool, out, counter, out_pool,
                       pool_cursor, pool_cap, th);
    return hipGetLastError();
}

hipError_t ytql_launch_merge_states(const YtStateRow* states, int64_t n,
                                    int agg_count, int sum_slot, int state_func,
                                    TableHdr* th, unsigned long long* slots,
                                    hipStream_t st)
{
    int block = 256;
    int64_t want = (n + block - 1) / block;
    int grid = (int)(want > 2048 ? 2048 : (want ? want : 1));
    hipLaunchKernelGGL(k_merge_states, dim3(grid), dim3(block), 0, st,
                       states, n, agg_count, sum_slot, state_func, th, slots);
    return hipGetLastError();
}

} /* extern C */
