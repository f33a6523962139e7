/* strpred.h — byte-wise string predicate matchers, shared by the device
 * entry pass (kernels.hip k_strpred_entries) and the host test entry
 * (yt_strpred_eval). One text against one literal; the text is non-null.
 *
 * Plain loops only: no recursion and no per-thread arrays, so the device
 * build keeps everything in registers.
 *
 * op is a YT_EX_* code: EQ..GE compare text with the literal (memcmp over
 * the shorter length, then the shorter string is less; bytes unsigned — the
 * oracle's string comparer), IS_PREFIX / IS_SUBSTR take the literal as the
 * prefix / pattern, LIKE takes the literal as the pattern.
 */
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YT_SP_HD __host__ __device__ inline
#else
#define YT_SP_HD inline
#endif

namespace ytql {

/* the YT_EX_* codes of include/ytql_gpu.h, restated so that this header
 * stands alone */
enum {
    SP_EQ = 20, SP_NE = 21, SP_LT = 22, SP_LE = 23, SP_GT = 24, SP_GE = 25,
    SP_IS_PREFIX = 40, SP_IS_SUBSTR = 41, SP_LIKE = 42,
};

/* -1 / 0 / +1: text against literal */
YT_SP_HD int strpred_cmp(const char* t, int64_t tn, const char* l, int64_t ln)
{
    const int64_t n = tn < ln ? tn : ln;
    for (int64_t i = 0; i < n; i++) {
        const unsigned a = (unsigned char)t[i], b = (unsigned char)l[i];
        if (a != b) return a < b ? -1 : 1;
    }
    return tn < ln ? -1 : (tn > ln ? 1 : 0);
}

YT_SP_HD int strpred_prefix(const char* t, int64_t tn, const char* l, int64_t ln)
{
    if (ln > tn) return 0;
    for (int64_t i = 0; i < ln; i++)
        if (t[i] != l[i]) return 0;
    return 1;
}

/* naive O(n*m) search; the empty pattern is found everywhere */
YT_SP_HD int strpred_substr(const char* t, int64_t tn, const char* l, int64_t ln)
{
    for (int64_t s = 0; s + ln <= tn; s++) {
        int64_t i = 0;
        while (i < ln && t[s + i] == l[i]) i++;
        if (i == ln) return 1;
    }
    return 0;
}

/* does the pattern end in a lone escape byte? (an invalid plan) */
YT_SP_HD int strpred_like_bad_pattern(const char* p, int64_t pn, int escape)
{
    if (escape < 0) return 0;
    for (int64_t i = 0; i < pn; i++) {
        if ((unsigned char)p[i] == (unsigned)escape) {
            if (i + 1 >= pn) return 1;
            i++;
        }
    }
    return 0;
}

/* LIKE, anchored to the whole text: '%' any byte sequence, '_' exactly one
 * byte, escape + byte = that byte literally (escape < 0: none). The
 * two-pointer matcher with ONE backtrack point: after a '%', a mismatch
 * resumes behind that '%' with the text advanced by one byte. The pattern
 * must have passed strpred_like_bad_pattern. */
YT_SP_HD int strpred_like(const char* t, int64_t tn, const char* p, int64_t pn,
                          int escape)
{
    int64_t ti = 0, pi = 0;
    int64_t star_p = -1, star_t = 0;
    while (ti < tn) {
        int ok = 0;
        if (pi < pn) {
            const unsigned c = (unsigned char)p[pi];
            if (escape >= 0 && c == (unsigned)escape) {
                /* pi + 1 < pn by validation */
                if ((unsigned char)p[pi + 1] == (unsigned char)t[ti]) {
                    pi += 2; ti++; ok = 1;
                }
            } else if (c == '%') {
                star_p = ++pi;
                star_t = ti;
                ok = 1;
            } else if (c == '_' || c == (unsigned char)t[ti]) {
                pi++; ti++; ok = 1;
            }
        }
        if (!ok) {
            if (star_p < 0) return 0;
            pi = star_p;
            ti = ++star_t;
        }
    }
    /* text consumed: only '%'s may remain (an escaped '%' is a literal) */
    while (pi < pn && p[pi] == '%' && !(escape == '%')) pi++;
    return pi == pn;
}

/* 0 / 1, or -1 for an unknown op. LIKE patterns must be pre-validated. */
YT_SP_HD int strpred_eval(int op, int escape, const char* t, int64_t tn,
                          const char* l, int64_t ln)
{
    switch (op) {
    case SP_EQ: return strpred_cmp(t, tn, l, ln) == 0;
    case SP_NE: return strpred_cmp(t, tn, l, ln) != 0;
    case SP_LT: return strpred_cmp(t, tn, l, ln) < 0;
    case SP_LE: return strpred_cmp(t, tn, l, ln) <= 0;
    case SP_GT: return strpred_cmp(t, tn, l, ln) > 0;
    case SP_GE: return strpred_cmp(t, tn, l, ln) >= 0;
    case SP_IS_PREFIX: return strpred_prefix(t, tn, l, ln);
    case SP_IS_SUBSTR: return strpred_substr(t, tn, l, ln);
    case SP_LIKE: return strpred_like(t, tn, l, ln, escape);
    default: return -1;
    }
}

} /* namespace ytql */
