/* inlist.h — lookup tables of YT_EX_IN (include/ytql_gpu.h), shared by the
 * kernels (kernels.hip in_num_row, k_inlist_str_entries), by the host that
 * builds them (evaluator.cpp) and by the host test entries
 * (yt_inlist_eval_i64 / yt_inlist_eval_str), which build a table exactly as
 * the product does and probe it on the CPU.
 *
 * Numeric form: an open-addressing table of uint64_t keys, load <= 0.5,
 * linear probing from mix64(key). The empty marker is a value outside the
 * list, picked by the builder.
 *
 * String form: slots {hash64, byte offset, length} over one buffer of the
 * list's bytes; hash = splitmix64(FNV-1a(bytes)), the byte hash of the
 * string-key exchange. An equal hash is not equality: a hit is confirmed on
 * length and bytes. An empty slot has len == kInStrEmpty.
 *
 * Both tables hold DISTINCT values only and at least one empty slot, so
 * every probe loop ends. "The list holds null" is not in the table: it is a
 * flag beside it (the answer for a null operand).
 */
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include <algorithm>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YT_IN_HD __host__ __device__ inline
#else
#define YT_IN_HD inline
#endif

namespace ytql {

struct InStrSlot {
    uint64_t hash;
    uint32_t off;          /* into the list's byte buffer */
    uint32_t len;          /* kInStrEmpty = empty slot */
};
static_assert(sizeof(InStrSlot) == 16, "one 16-byte load per slot");

constexpr uint32_t kInStrEmpty = 0xFFFFFFFFu;

/* values per list after the host removed duplicates */
constexpr int64_t kInListMax = 1 << 20;

/* k_inlist_str_entries stages the slot table in LDS when it fits this many
 * bytes. The entry kernels run 256-thread workgroups at 8 waves/SIMD, that
 * is 8 workgroups per CU; 160 KiB of LDS per CU over 8 workgroups is 20 KiB
 * each, and 16 KiB is the largest power-of-two table below that (32 KiB
 * would leave 5 workgroups, 5 waves/SIMD). 1024 slots: lists of up to 512
 * distinct strings. */
constexpr uint32_t kInStrLdsBytes = 16 * 1024;
constexpr uint32_t kInStrLdsSlots = kInStrLdsBytes / sizeof(InStrSlot);

/* splitmix64: kernels.hip mix64, evaluator.cpp splitmix64_host */
YT_IN_HD uint64_t inlist_mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

YT_IN_HD uint64_t inlist_str_hash(const char* p, uint32_t len)
{
    uint64_t h = 0xCBF29CE484222325ULL;
    for (uint32_t k = 0; k < len; k++)
        h = (h ^ (uint8_t)p[k]) * 0x100000001B3ULL;
    return inlist_mix64(h);
}

/* is key in the table? */
YT_IN_HD int inlist_probe_u64(const uint64_t* tab, uint64_t mask, uint64_t empty,
                              uint64_t key)
{
    if (key == empty) return 0;
    uint64_t h = inlist_mix64(key) & mask;
    for (;;) {
        const uint64_t k = tab[h];
        if (k == key) return 1;
        if (k == empty) return 0;
        h = (h + 1) & mask;
    }
}

/* is the text (hash h = inlist_str_hash of it) in the table? */
YT_IN_HD int inlist_probe_str(const InStrSlot* slots, uint64_t mask,
                              const char* bytes, uint64_t h,
                              const char* t, uint32_t tn)
{
    uint64_t i = h & mask;
    for (;;) {
        const InStrSlot s = slots[i];
        if (s.len == kInStrEmpty) return 0;
        if (s.hash == h && s.len == tn) {
            const char* l = bytes + s.off;
            uint32_t k = 0;
            while (k < tn && l[k] == t[k]) k++;
            if (k == tn) return 1;
        }
        i = (i + 1) & mask;
    }
}

/* ---- host builders ---- */

inline uint64_t inlist_slots_for(uint64_t n)
{
    uint64_t p = 2;
    while (p < n * 2) p <<= 1;
    return p;
}

/* sorted: the list's distinct non-null values as raw 64-bit patterns,
 * ascending as uint64_t. Fills tab (a power of two of slots, load <= 0.5)
 * and picks *empty outside the list. */
inline void inlist_build_u64(const std::vector<uint64_t>& sorted,
                             std::vector<uint64_t>* tab, uint64_t* mask,
                             uint64_t* empty)
{
    uint64_t e = 0x8000000000000000ULL;
    while (std::binary_search(sorted.begin(), sorted.end(), e)) e++;
    const uint64_t nslots = inlist_slots_for(sorted.size());
    tab->assign(nslots, e);
    for (uint64_t k : sorted) {
        uint64_t h = inlist_mix64(k) & (nslots - 1);
        while ((*tab)[h] != e) h = (h + 1) & (nslots - 1);
        (*tab)[h] = k;
    }
    *mask = nslots - 1;
    *empty = e;
}

/* The list's non-null strings (ptr[i], len[i]), duplicates allowed: copies
 * the distinct ones into *bytes and fills *slots. Returns the number of
 * distinct strings, or -1 when their bytes pass 4 GiB (offsets are 32-bit). */
inline int64_t inlist_build_str(const char* const* ptr, const uint32_t* len,
                                int64_t n, std::vector<char>* bytes,
                                std::vector<InStrSlot>* slots, uint64_t* mask)
{
    InStrSlot none;
    none.hash = 0; none.off = kInStrEmpty; none.len = kInStrEmpty;
    /* a table sized for the whole list finds the duplicates; the table that
     * is kept is sized for the distinct values alone */
    uint64_t nslots = inlist_slots_for((uint64_t)n);
    slots->assign(nslots, none);
    bytes->clear();
    std::vector<InStrSlot> kept;
    for (int64_t i = 0; i < n; i++) {
        const uint64_t h = inlist_str_hash(ptr[i], len[i]);
        if (inlist_probe_str(slots->data(), nslots - 1, bytes->data(), h,
                             ptr[i], len[i]))
            continue;
        if (bytes->size() + (uint64_t)len[i] >= 0xFFFFFFFFull) return -1;
        uint64_t s = h & (nslots - 1);
        while ((*slots)[s].len != kInStrEmpty) s = (s + 1) & (nslots - 1);
        (*slots)[s].hash = h;
        (*slots)[s].off = (uint32_t)bytes->size();
        (*slots)[s].len = len[i];
        kept.push_back((*slots)[s]);
        bytes->insert(bytes->end(), ptr[i], ptr[i] + len[i]);
    }
    if (inlist_slots_for(kept.size()) < nslots) {
        nslots = inlist_slots_for(kept.size());
        slots->assign(nslots, none);
        for (const InStrSlot& k : kept) {
            uint64_t s = k.hash & (nslots - 1);
            while ((*slots)[s].len != kInStrEmpty) s = (s + 1) & (nslots - 1);
            (*slots)[s] = k;
        }
    }
    *mask = nslots - 1;
    return (int64_t)kept.size();
}

} /* namespace ytql */
