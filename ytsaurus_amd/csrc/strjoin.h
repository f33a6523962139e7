/* strjoin.h — the slot probe of a STRING-key equi-join's foreign table,
 * shared by the kernels (kernels.hip k_strjoin_chain, k_strjoin_entries) and
 * by the host test entry (evaluator.cpp yt_strjoin_eval), which builds a
 * table on the CPU by the same rules and probes it.
 *
 * The table is JoinDev's (common.h): open addressing, linear probing, the
 * foreign ROW index as the claim word (hrow, -1 = empty) and the row's
 * 64-bit byte hash (inlist.h inlist_str_hash) in hkey. Every non-null
 * foreign row claims a slot of its own, so rows with one key hold several
 * slots; the key's CANONICAL slot is the first one in probe order whose hash
 * equals the key's and whose owner row has the key's length and bytes. Its
 * chead holds the match list. An equal hash is not equality: the bytes
 * decide. The table keeps load <= 0.5, so every probe loop ends.
 *
 * The probe takes the hash as an argument and does not compute it: the host
 * test entry passes hashes cut to a few bits, so that nearly every probe
 * meets an equal hash over different bytes — a branch that whole 64-bit
 * hashes never reach in a test.
 */
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YT_SJ_HD __host__ __device__ inline
#else
#define YT_SJ_HD inline
#endif

namespace ytql {

/* the probe found no slot */
constexpr int64_t kStrJoinAbsent = -1;

/* Canonical slot of the text (t, tn) whose hash is h, or kStrJoinAbsent.
 * owner(row, &len) yields the bytes of foreign row `row`'s key; it is asked
 * about slot owners only, which are never null-key rows. */
template <class OwnerBytes>
YT_SJ_HD int64_t strjoin_probe_slot(const uint64_t* hkey, const int64_t* hrow,
                                    uint64_t mask, uint64_t h,
                                    const char* t, uint32_t tn,
                                    const OwnerBytes& owner)
{
    uint64_t i = h & mask;
    for (;;) {
        const int64_t r = hrow[i];
        if (r < 0) return kStrJoinAbsent;
        if (hkey[i] == h) {
            uint32_t ln = 0;
            const char* l = owner(r, &ln);
            if (ln == tn) {
                uint32_t k = 0;
                while (k < tn && l[k] == t[k]) k++;
                if (k == tn) return (int64_t)i;
            }
        }
        i = (i + 1) & mask;
    }
}

} /* namespace ytql */
