/* evaluator.cpp — host side of the MI355X query executor: the C-ABI
 * implementation of the IEvaluator::Run seam (reference
 * engine/evaluator.cpp:51-105), plan compilation (AOT replacement of the
 * LLVM codegen in folding_profiler.cpp / cg_fragment_compiler.cpp), device
 * orchestration, limits and statistics (TExecutionContext /
 * TQueryStatistics, engine_api/evaluation_helpers.h:251-280).
 *
 * Product code. No CPU fallback: without a HIP device every execute entry
 * returns YT_ERR_NO_GPU / YT_ERR_HIP.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include <algorithm>
#include <mutex>
#include <chrono>
#include <thread>
#include <atomic>
#include <memory>

#include "common.h"
#include "strpred.h"
#include "inlist.h"
#include "strjoin.h"
#include "launch.h"
#include "../../include/ytql_gpu.h"

using namespace ytql;

/* must match kernels.hip mix64 and the oracle's splitmix64 */
static inline uint64_t splitmix64_host(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

/* partition-output request for run_string_group (string-keyed bottom
 * query): when set, the compacted groups are hash-partitioned into
 * state rows + pool slices instead of being emitted as a rowset. */
struct StrPartialOut {
    int32_t partition_count;
    YtStateRow* states_device;
    int64_t capacity_rows;
    char* pool_device;
    int64_t pool_capacity;
    int64_t* part_counts;        /* out */
    int64_t* part_pool_bytes;    /* out */
};

/* ------------------------------------------------------------------ */
/* device/pinned buffer pool: query executions reuse large allocations
 * across calls (the reference's evaluator similarly reuses codegen and
 * memory-chunk pools per query class, evaluator.cpp:256, TExpressionContext
 * chunk providers). Freed via yt_gpu_pool_trim(). */

namespace {

struct Pool {
    struct Blk { void* p; size_t sz; bool used; bool host; };
    std::mutex m;
    std::vector<Blk> blks;

    hipError_t get(size_t sz, bool host, void** out)
    {
        std::lock_guard<std::mutex> g(m);
        Blk* best = nullptr;
        for (auto& b : blks) {
            if (!b.used && b.host == host && b.sz >= sz &&
                (!best || b.sz < best->sz)) {
                best = &b;
            }
        }
        if (best && best->sz <= sz * 2 + (64 << 20)) {
            best->used = true;
            *out = best->p;
            return hipSuccess;
        }
        void* p = nullptr;
        hipError_t e = host ? hipHostMalloc(&p, sz) : hipMalloc(&p, sz);
        if (e != hipSuccess) {
            /* retry after trimming the pool */
            for (auto& b : blks) {
                if (!b.used) {
                    if (b.host) { (void)hipHostFree(b.p); } else { (void)hipFree(b.p); }
                    b.p = nullptr;
                    b.sz = 0;
                }
            }
            blks.erase(std::remove_if(blks.begin(), blks.end(),
                                      [](const Blk& b) { return !b.p; }),
                       blks.end());
            e = host ? hipHostMalloc(&p, sz) : hipMalloc(&p, sz);
            if (e != hipSuccess) return e;
        }
        blks.push_back({p, sz, true, host});
        *out = p;
        return hipSuccess;
    }

    void put(void* p)
    {
        if (!p) return;
        std::lock_guard<std::mutex> g(m);
        for (auto& b : blks) {
            if (b.p == p) { b.used = false; return; }
        }
    }

    void trim()
    {
        std::lock_guard<std::mutex> g(m);
        for (auto& b : blks) {
            if (!b.used) {
                if (b.host) { (void)hipHostFree(b.p); } else { (void)hipFree(b.p); }
                b.p = nullptr;
            }
        }
        blks.erase(std::remove_if(blks.begin(), blks.end(),
                                  [](const Blk& b) { return !b.p; }),
                   blks.end());
    }

    uint64_t in_use()
    {
        std::lock_guard<std::mutex> g(m);
        uint64_t n = 0;
        for (auto& b : blks) n += b.used;
        return n;
    }
};

Pool g_pool;

/* The owner of what a call takes from g_pool and of the events it creates:
 * the destructor destroys the events, then puts every block back, so no exit
 * has a list to repeat. The call sites keep their raw pointers. */
struct PoolScope {
    std::vector<void*> blks;
    std::vector<hipEvent_t> evs;

    PoolScope() = default;
    PoolScope(const PoolScope&) = delete;
    PoolScope& operator=(const PoolScope&) = delete;

    ~PoolScope()
    {
        for (hipEvent_t e : evs) (void)hipEventDestroy(e);
        for (void* b : blks) g_pool.put(b);
    }

    template <class T>
    hipError_t dev(T** p, size_t bytes) { return take((void**)p, bytes, false); }

    template <class T>
    hipError_t host(T** p, size_t bytes) { return take((void**)p, bytes, true); }

    /* put one block back early; null and unknown pointers are ignored */
    void release(void* p) { if (forget(p)) g_pool.put(p); }

    /* the block outlives the call: its new owner puts it back */
    void detach(void* p) { (void)forget(p); }

    hipError_t event(hipEvent_t* e, unsigned flags = hipEventDefault)
    {
        hipError_t err = hipEventCreateWithFlags(e, flags);
        if (err == hipSuccess) evs.push_back(*e);
        return err;
    }

private:
    hipError_t take(void** p, size_t bytes, bool host)
    {
        hipError_t err = g_pool.get(bytes, host, p);
        if (err == hipSuccess) blks.push_back(*p);
        return err;
    }

    bool forget(void* p)
    {
        auto it = p ? std::find(blks.begin(), blks.end(), p) : blks.end();
        if (it == blks.end()) return false;
        blks.erase(it);
        return true;
    }
};

/* joins its threads on every way out of the scope that holds it */
struct ThreadJoiner {
    std::vector<std::thread> ths;

    ThreadJoiner() = default;
    ThreadJoiner(const ThreadJoiner&) = delete;
    ThreadJoiner& operator=(const ThreadJoiner&) = delete;
    ~ThreadJoiner() { join(); }

    void join()
    {
        for (auto& t : ths) if (t.joinable()) t.join();
        ths.clear();
    }
};

double now_ms()
{
    return std::chrono::duration<double, std::milli>(
        std::chrono::steady_clock::now().time_since_epoch()).count();
}

} /* namespace */

extern "C" void yt_gpu_pool_trim(void)
{
    g_pool.trim();
}

/* diagnostic: pool blocks taken and not yet put back */
extern "C" uint64_t yt_gpu_debug_pool_blocks_in_use(void)
{
    return g_pool.in_use();
}

static void set_err(char* errbuf, size_t errlen, const char* msg)
{
    if (errbuf && errlen) snprintf(errbuf, errlen, "%s", msg);
}

#define HIP_CHECK(call)                                                     \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) {                                             \
            if (errbuf) snprintf(errbuf, errlen, "HIP error %s at %s:%d",   \
                                 hipGetErrorString(e_), __FILE__, __LINE__);\
            return YT_ERR_HIP;                                              \
        }                                                                   \
    } while (0)

extern "C" int yt_gpu_available(char* errbuf, size_t errlen)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        set_err(errbuf, errlen, "no HIP device");
        return YT_ERR_NO_GPU;
    }
    return YT_OK;
}

/* ------------------------------------------------------------------ */
/* plan compilation: YtExpr tree → postfix DevPlan program              */

struct StrPreds;
static int compile_in_num(const YtExpr* e, DevPlan* p, StrPreds* sp, int* len,
                          char* errbuf, size_t errlen, int* need);

/* ---- expression typing (include/ytql_gpu.h, the comment above YtExpr) ----
 * Decided from static types, before any kernel runs: check_plan_types
 * refuses what the rules refuse, compile_expr emits an adopting integer
 * literal in its adopted type, and expr_static_type gives an arithmetic
 * node the common type of its operands. */

static inline bool op_is_arith(int op) { return op >= YT_EX_ADD && op <= YT_EX_MOD; }
static inline bool op_is_rel(int op) { return op >= YT_EX_EQ && op <= YT_EX_GE; }

/* the type operand e, of static type `own`, has beside an operand of static
 * type `other`: an integer literal takes a DOUBLE or UINT64 neighbour's */
static inline uint8_t adopt_type(const YtExpr* e, uint8_t own, uint8_t other)
{
    if (e->op == YT_EX_LIT_I64 && (other == YT_VT_DOUBLE || other == YT_VT_UINT64))
        return other;
    return own;
}

static uint8_t expr_static_type(const YtExpr* e, const uint8_t* col_types);

/* The device stack one more operand takes: a binary node evaluates a, keeps
 * its value and evaluates b. */
static int need_check(int need, char* errbuf, size_t errlen)
{
    if (need <= kEvalStack) return YT_OK;
    if (errbuf && errlen)
        snprintf(errbuf, errlen,
                 "expression nested too deep: it needs %d evaluation stack "
                 "slots, the limit is %d", need, kEvalStack);
    return YT_ERR_UNSUPPORTED;
}

/* *need (optional) = the evaluation stack slots the program of e takes; a
 * program over kEvalStack is refused at the node that exceeds it */
static int compile_expr(const YtExpr* e, DevPlan* p, StrPreds* sp, int* len,
                        char* errbuf, size_t errlen, int* need = nullptr)
{
    if (!e) { set_err(errbuf, errlen, "null expr"); return YT_ERR_INVALID_PLAN; }
    int need_here = 1;
    switch (e->op) {
    case YT_EX_COLUMN:
    case YT_EX_LIT_I64:
    case YT_EX_LIT_NULL:
    case YT_EX_LIT_DOUBLE:
        break;
    case YT_EX_IN:
        /* one operand and a literal list: the operand, then P_IN_NUM */
        return compile_in_num(e, p, sp, len, errbuf, errlen, need);
    case YT_EX_NOT: {
        int rc = compile_expr(e->a, p, sp, len, errbuf, errlen, &need_here);
        if (rc) return rc;
        break;
    }
    default: {
        int na = 1, nb = 1;
        int rc = compile_expr(e->a, p, sp, len, errbuf, errlen, &na);
        if (rc) return rc;
        const int ia = p->prog_len - 1;
        rc = compile_expr(e->b, p, sp, len, errbuf, errlen, &nb);
        if (rc) return rc;
        const int ib = p->prog_len - 1;
        need_here = std::max(na, 1 + nb);
        rc = need_check(need_here, errbuf, errlen);
        if (rc) return rc;
        if (op_is_arith(e->op) || op_is_rel(e->op)) {
            /* an integer literal operand is the one instruction just
             * emitted for it: retype it beside a DOUBLE or UINT64 operand
             * (check_plan_types has refused a negative one beside UINT64) */
            const uint8_t ta = expr_static_type(e->a, p->col_types);
            const uint8_t tb = expr_static_type(e->b, p->col_types);
            const YtExpr* side[2] = {e->a, e->b};
            const uint8_t to[2] = {adopt_type(e->a, ta, tb), adopt_type(e->b, tb, ta)};
            const int at[2] = {ia, ib};
            for (int s = 0; s < 2; s++) {
                if (side[s]->op != YT_EX_LIT_I64) continue;
                PInst& li = p->prog[at[s]];
                if (to[s] == YT_VT_DOUBLE) {
                    const double d = (double)side[s]->lit_i64;
                    li.op = P_LIT_DOUBLE;
                    memcpy(&li.bits, &d, 8);
                } else if (to[s] == YT_VT_UINT64) {
                    li.op = P_LIT_U64;
                }
            }
        }
        break;
    }
    }
    if (need) *need = need_here;
    if (p->prog_len >= kMaxProg) {
        if (errbuf && errlen)
            snprintf(errbuf, errlen,
                     "expression too long: a plan's programs hold at most %d "
                     "instructions", kMaxProg);
        return YT_ERR_INVALID_PLAN;
    }
    PInst& in = p->prog[p->prog_len++];
    in.op = e->op;     /* YT_EX_* values coincide with P_* by construction */
    in.col = e->col;
    in.bits = 0;
    if (e->op == YT_EX_LIT_I64) in.bits = (uint64_t)e->lit_i64;
    if (e->op == YT_EX_LIT_DOUBLE) memcpy(&in.bits, &e->lit_dbl, 8);
    if (e->op == YT_EX_COLUMN && (e->col < 0 || e->col >= p->ncols)) {
        set_err(errbuf, errlen, "column index out of range");
        return YT_ERR_INVALID_PLAN;
    }
    (*len)++;
    return YT_OK;
}

/* static result type of an expression: aggregate state and output types, IN
 * operand typing, rowset column types. An arithmetic node has the common
 * type of its operands after literal adoption: a null operand leaves the
 * other one's type, BOOLEAN beside an integer keeps the left one's. */
static uint8_t expr_static_type(const YtExpr* e, const uint8_t* col_types)
{
    switch (e->op) {
    case YT_EX_COLUMN: return col_types[e->col];
    case YT_EX_LIT_I64: return YT_VT_INT64;
    case YT_EX_LIT_DOUBLE: return YT_VT_DOUBLE;
    case YT_EX_LIT_NULL: return YT_VT_NULL;
    case YT_EX_LIT_STRING: return YT_VT_STRING;
    case YT_EX_NOT: return YT_VT_BOOLEAN;
    case YT_EX_IN: return YT_VT_BOOLEAN;
    default: {
        if (e->op >= YT_EX_EQ) return YT_VT_BOOLEAN;   /* cmp / and / or */
        const uint8_t ta = expr_static_type(e->a, col_types);
        const uint8_t tb = expr_static_type(e->b, col_types);
        const uint8_t xa = adopt_type(e->a, ta, tb);
        return xa == YT_VT_NULL ? adopt_type(e->b, tb, ta) : xa;
    }
    }
}

/* Refuses a tree that breaks the typing rules; types[0..ntypes) are the
 * static types of the columns it reads. Strings keep their own rules
 * (compile_filter): a node with a STRING operand passes here. */
static int check_expr_types(const YtExpr* e, const uint8_t* types, int ntypes,
                            char* errbuf, size_t errlen)
{
    if (!e) { set_err(errbuf, errlen, "null expr"); return YT_ERR_INVALID_PLAN; }
    switch (e->op) {
    case YT_EX_COLUMN:
        if (e->col < 0 || e->col >= ntypes) {
            set_err(errbuf, errlen, "column index out of range");
            return YT_ERR_INVALID_PLAN;
        }
        return YT_OK;
    case YT_EX_LIT_I64:
    case YT_EX_LIT_DOUBLE:
    case YT_EX_LIT_NULL:
    case YT_EX_LIT_STRING:
        return YT_OK;
    case YT_EX_NOT:
    case YT_EX_IN:                  /* one operand; the list has its own check */
        return check_expr_types(e->a, types, ntypes, errbuf, errlen);
    default:
        break;
    }
    int rc = check_expr_types(e->a, types, ntypes, errbuf, errlen);
    if (rc) return rc;
    rc = check_expr_types(e->b, types, ntypes, errbuf, errlen);
    if (rc) return rc;
    if (!op_is_arith(e->op) && !op_is_rel(e->op)) return YT_OK;
    const uint8_t ta = expr_static_type(e->a, types);
    const uint8_t tb = expr_static_type(e->b, types);
    if (ta == YT_VT_STRING || tb == YT_VT_STRING) return YT_OK;
    const uint8_t xa = adopt_type(e->a, ta, tb), xb = adopt_type(e->b, tb, ta);
    for (const YtExpr* s : {e->a, e->b}) {
        if (s->op == YT_EX_LIT_I64 && s->lit_i64 < 0 &&
            (s == e->a ? xa : xb) == YT_VT_UINT64) {
            set_err(errbuf, errlen,
                    "type mismatch: a negative integer literal beside a "
                    "UINT64 operand");
            return YT_ERR_INVALID_PLAN;
        }
    }
    if ((xa == YT_VT_DOUBLE && xb != YT_VT_DOUBLE && xb != YT_VT_NULL) ||
        (xb == YT_VT_DOUBLE && xa != YT_VT_DOUBLE && xa != YT_VT_NULL)) {
        set_err(errbuf, errlen,
                "type mismatch: a DOUBLE operand beside one that is neither "
                "DOUBLE nor null (litf() writes a double literal)");
        return YT_ERR_INVALID_PLAN;
    }
    if ((xa == YT_VT_INT64 && xb == YT_VT_UINT64) ||
        (xa == YT_VT_UINT64 && xb == YT_VT_INT64)) {
        set_err(errbuf, errlen,
                "type mismatch: an INT64 operand beside a UINT64 operand");
        return YT_ERR_INVALID_PLAN;
    }
    if (e->op == YT_EX_MOD && (xa == YT_VT_DOUBLE || xb == YT_VT_DOUBLE)) {
        set_err(errbuf, errlen, "modulo over DOUBLE operands: unsupported");
        return YT_ERR_UNSUPPORTED;
    }
    return YT_OK;
}

/* Every expression of the plan: filter, keys, aggregate arguments and a plain
 * scan's projections against the input column types, a grouped plan's
 * projections and HAVING against the types of its rows [keys, aggregates]. */
static int check_plan_types(const YtPlan* plan, const uint8_t* col_types, int ncols,
                            char* errbuf, size_t errlen)
{
    int rc;
    if (plan->filter) {
        rc = check_expr_types(plan->filter, col_types, ncols, errbuf, errlen);
        if (rc) return rc;
    }
    uint8_t row[kMaxPackKeys + kMaxAggs];
    int nrow = 0;
    const bool grouped = plan->key_count > 0 || plan->agg_count > 0;
    if (plan->key_count > kMaxPackKeys || plan->agg_count > kMaxAggs)
        return YT_OK;               /* refused by the entry that compiles it */
    for (int k = 0; k < plan->key_count; k++) {
        rc = check_expr_types(plan->keys[k], col_types, ncols, errbuf, errlen);
        if (rc) return rc;
        row[nrow++] = expr_static_type(plan->keys[k], col_types);
    }
    for (int a = 0; a < plan->agg_count; a++) {
        const int f = plan->aggs[a]->func;
        uint8_t t = YT_VT_INT64;
        if (f != YT_AGG_SUM1) {
            rc = check_expr_types(plan->aggs[a]->arg, col_types, ncols, errbuf, errlen);
            if (rc) return rc;
            t = expr_static_type(plan->aggs[a]->arg, col_types);
        }
        row[nrow++] = f == YT_AGG_AVG ? (uint8_t)YT_VT_DOUBLE : t;
    }
    for (int pj = 0; pj < plan->project_count; pj++) {
        rc = check_expr_types(plan->projects[pj], grouped ? row : col_types,
                              grouped ? nrow : ncols, errbuf, errlen);
        if (rc) return rc;
    }
    if (plan->having && grouped) {
        rc = check_expr_types(plan->having, row, nrow, errbuf, errlen);
        if (rc) return rc;
    }
    return YT_OK;
}

static bool expr_is_col(const YtExpr* e, int* col);
static void hexpr_cols(const YtExpr* e, uint64_t* mask);

/* does the expression read a STRING column? The device interpreter decodes
 * integer, boolean and double layouts only; it would misread a string blob
 * as packed integers. */
static bool expr_reads_string(const YtExpr* e, const uint8_t* col_types, int ncols)
{
    if (!e) return false;
    if (e->op == YT_EX_COLUMN)
        return e->col >= 0 && e->col < ncols && col_types[e->col] == YT_VT_STRING;
    if (e->op == YT_EX_LIT_I64 || e->op == YT_EX_LIT_NULL ||
        e->op == YT_EX_LIT_DOUBLE || e->op == YT_EX_LIT_STRING)
        return false;
    if (e->op == YT_EX_IN)          /* one operand; b is unused */
        return expr_reads_string(e->a, col_types, ncols);
    return expr_reads_string(e->a, col_types, ncols) ||
           (e->op != YT_EX_NOT && expr_reads_string(e->b, col_types, ncols));
}

/* does an IN list hold a string value? (a numeric IN is no string node) */
static bool in_list_has_string(const YtExpr* e)
{
    if (!e->list) return false;
    for (int64_t i = 0; i < e->list_len; i++)
        if (e->list[i].type == YT_VT_STRING) return true;
    return false;
}

/* does the expression hold a string literal or a string function? Only a
 * filter's string-predicate leaves may (compile_filter). */
static bool expr_has_strlit(const YtExpr* e)
{
    if (!e) return false;
    if (e->op == YT_EX_LIT_STRING ||
        (e->op >= YT_EX_IS_PREFIX && e->op <= YT_EX_LIKE))
        return true;
    if (e->op == YT_EX_COLUMN || e->op == YT_EX_LIT_I64 ||
        e->op == YT_EX_LIT_NULL || e->op == YT_EX_LIT_DOUBLE)
        return false;
    if (e->op == YT_EX_IN)
        return in_list_has_string(e) || expr_has_strlit(e->a);
    return expr_has_strlit(e->a) ||
           (e->op != YT_EX_NOT && expr_has_strlit(e->b));
}

/* ------------------------------------------------------------------ */
/* string predicates: a STRING column against a literal, in the filter.
 * A leaf depends on the column's ENTRY only (dictionary entry, run or row,
 * kernels.hip str_key_id), so it is evaluated once per entry into a bitmap
 * (k_strpred_entries) and each row reads one bit (P_STR_PRED). */

struct StrPredDesc {
    int op;                /* YT_EX_EQ..GE (column on the left), IS_PREFIX,
                              IS_SUBSTR, LIKE, or YT_EX_IN (the list is
                              StrPreds::il of the same index) */
    int escape;            /* LIKE: 0..255, or -1 */
    int col;
    const char* lit;       /* the plan's bytes; alive for the whole call */
    int64_t lit_len;
};

/* a string IN list as the entry kernel reads it (inlist.h) */
struct InStrList {
    std::vector<char> bytes;
    std::vector<InStrSlot> slots;
    uint64_t mask = 0;
};

/* a numeric IN list: the distinct non-null values as raw 64-bit patterns,
 * ascending; the device table is built from it (setup_string_preds) and
 * heval searches it */
struct InNumSet {
    const YtExpr* e = nullptr;
    std::vector<uint64_t> sorted;
    bool has_null = false;
    uint8_t type = 0;      /* YT_VT_* of the values; 0 = nulls only */
};

/* what a plan's filter (string predicates) and expressions (numeric IN
 * sets) need on the device beside the program */
struct StrPreds {
    int count = 0;                  /* leaves that need a bitmap */
    bool any = false;               /* any leaf, bitmap-less ones included */
    int primary_ncols = 0;          /* columns below this are the chunk's own */
    StrPredDesc d[kMaxStrPreds];
    InStrList il[kMaxStrPreds];     /* d[i].op == YT_EX_IN */
    int in_count = 0;               /* numeric IN sets */
    InNumSet in[kMaxInSets];
    PoolScope ps;                   /* pooled device buffers of this run */
    std::vector<int64_t> h_base[kMaxStrPreds];   /* upload sources */
    std::vector<uint64_t> h_intab[kMaxInSets];
};

static thread_local uint64_t t_last_strpred_entries = 0;
static thread_local uint64_t t_last_strjoin_inserted = 0;
static thread_local uint64_t t_last_strjoin_entries = 0;
static thread_local uint64_t t_last_strkey_entries = 0;
static thread_local uint64_t t_last_strkey_distinct = 0;
static thread_local int32_t t_last_inlist_mode = 0;

/* is component i of the composite key a STRING column (packs a string id)? */
static inline bool kp_is_str(const DevPlan* dp, int i)
{
    return dp->col_types[dp->kp_col[i]] == YT_VT_STRING;
}

/* the distinct strings of one STRING key column on the host: id -> bytes */
struct StrKeyTab {
    std::vector<StrKeyId> ids;
    std::vector<char> pool;
};

extern "C" uint64_t yt_gpu_debug_last_strpred_entries(void)
{
    return t_last_strpred_entries;
}

extern "C" int32_t yt_gpu_debug_last_inlist_mode(void)
{
    return t_last_inlist_mode;
}

/* the list of a YT_EX_IN node is well formed */
static int in_list_shape(const YtExpr* e, char* errbuf, size_t errlen)
{
    if (e->list_len < 0 || (e->list_len > 0 && !e->list)) {
        set_err(errbuf, errlen, "IN: negative list_len, or a list without values");
        return YT_ERR_INVALID_PLAN;
    }
    if (e->b) {
        set_err(errbuf, errlen, "IN over a tuple operand: not this round");
        return YT_ERR_UNSUPPORTED;
    }
    return YT_OK;
}

static int in_list_too_long(char* errbuf, size_t errlen)
{
    if (errbuf && errlen)
        snprintf(errbuf, errlen,
                 "IN list longer than %lld distinct values: unsupported",
                 (long long)kInListMax);
    return YT_ERR_UNSUPPORTED;
}

/* sort and deduplicate a numeric list whose values have type vt (or are
 * null); a boolean is its truth value */
static int in_num_prepare(const YtExpr* e, uint8_t vt, InNumSet* s,
                          char* errbuf, size_t errlen)
{
    s->e = e;
    s->type = vt;
    s->has_null = false;
    s->sorted.clear();
    s->sorted.reserve((size_t)e->list_len);
    for (int64_t i = 0; i < e->list_len; i++) {
        const YtValue& v = e->list[i];
        if (v.type == YT_VT_NULL) { s->has_null = true; continue; }
        if (v.type != vt) {
            set_err(errbuf, errlen,
                    "type mismatch: an IN list value has another type than "
                    "the operand");
            return YT_ERR_INVALID_PLAN;
        }
        s->sorted.push_back(vt == YT_VT_BOOLEAN ? (uint64_t)(v.data.bits != 0)
                                                : v.data.bits);
    }
    std::sort(s->sorted.begin(), s->sorted.end());
    s->sorted.erase(std::unique(s->sorted.begin(), s->sorted.end()),
                    s->sorted.end());
    if ((int64_t)s->sorted.size() > kInListMax)
        return in_list_too_long(errbuf, errlen);
    return YT_OK;
}

static int emit_inst(DevPlan* p, int op, int col, uint64_t bits,
                     char* errbuf, size_t errlen)
{
    if (p->prog_len >= kMaxProg) { set_err(errbuf, errlen, "expression too long"); return YT_ERR_INVALID_PLAN; }
    PInst& in = p->prog[p->prog_len++];
    in.op = op;
    in.col = col;
    in.bits = bits;
    return YT_OK;
}

/* numeric YT_EX_IN: the operand's program, then one P_IN_NUM, which answers
 * in the operand's stack slot */
static int compile_in_num(const YtExpr* e, DevPlan* p, StrPreds* sp, int* len,
                          char* errbuf, size_t errlen, int* need)
{
    int rc = in_list_shape(e, errbuf, errlen);
    if (rc) return rc;
    if (!e->a) { set_err(errbuf, errlen, "null expr"); return YT_ERR_INVALID_PLAN; }
    if (e->a->op == YT_EX_COLUMN && (e->a->col < 0 || e->a->col >= p->ncols)) {
        set_err(errbuf, errlen, "column index out of range");
        return YT_ERR_INVALID_PLAN;
    }
    const uint8_t vt = expr_static_type(e->a, p->col_types);
    if (vt == YT_VT_DOUBLE) {
        set_err(errbuf, errlen, "IN over a DOUBLE operand: not this round");
        return YT_ERR_UNSUPPORTED;
    }
    if (vt == YT_VT_STRING) {
        set_err(errbuf, errlen,
                "IN: a string operand must be a plain string column of the "
                "primary chunk, in the filter");
        return YT_ERR_UNSUPPORTED;
    }
    if (vt != YT_VT_INT64 && vt != YT_VT_UINT64 && vt != YT_VT_BOOLEAN) {
        set_err(errbuf, errlen,
                "type mismatch: IN takes an int64, uint64 or boolean operand");
        return YT_ERR_INVALID_PLAN;
    }
    if (!sp || sp->in_count >= kMaxInSets) {
        set_err(errbuf, errlen,
                "more than 4 numeric IN lists in one plan: not this round");
        return YT_ERR_UNSUPPORTED;
    }
    /* the operand may hold an IN of its own: take the index first */
    const int idx = sp->in_count++;
    rc = in_num_prepare(e, vt, &sp->in[idx], errbuf, errlen);
    if (rc) return rc;
    rc = compile_expr(e->a, p, sp, len, errbuf, errlen, need);
    if (rc) return rc;
    rc = emit_inst(p, P_IN_NUM, 0,
                   (uint64_t)idx | (sp->in[idx].has_null ? kInNullRes : 0),
                   errbuf, errlen);
    if (rc) return rc;
    (*len)++;
    return YT_OK;
}

extern "C" int yt_inlist_eval_i64(const uint64_t* list, int64_t n, int has_null,
                                  const uint64_t* values, const uint8_t* nulls,
                                  int64_t m, uint8_t* out)
{
    if (n < 0 || m < 0 || (n && !list) || (m && (!values || !out)))
        return YT_ERR_INVALID_PLAN;
    std::vector<uint64_t> sorted(list, list + n);
    std::sort(sorted.begin(), sorted.end());
    sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
    if ((int64_t)sorted.size() > kInListMax) return YT_ERR_UNSUPPORTED;
    std::vector<uint64_t> tab;
    uint64_t mask = 0, empty = 0;
    inlist_build_u64(sorted, &tab, &mask, &empty);
    for (int64_t i = 0; i < m; i++)
        out[i] = (nulls && nulls[i])
            ? (uint8_t)(has_null != 0)
            : (uint8_t)inlist_probe_u64(tab.data(), mask, empty, values[i]);
    return YT_OK;
}

extern "C" int yt_inlist_eval_str(const char* list_bytes, const int64_t* list_ends,
                                  const uint8_t* list_nulls, int64_t n,
                                  const char* text_bytes, const int64_t* text_ends,
                                  const uint8_t* text_nulls, int64_t m,
                                  uint8_t* out)
{
    if (n < 0 || m < 0 || (n && !list_ends) || (m && (!text_ends || !out)))
        return YT_ERR_INVALID_PLAN;
    std::vector<const char*> ptr;
    std::vector<uint32_t> len;
    bool has_null = false;
    for (int64_t i = 0; i < n; i++) {
        const int64_t b = i ? list_ends[i - 1] : 0;
        if (list_nulls && list_nulls[i]) { has_null = true; continue; }
        ptr.push_back(list_bytes + b);
        len.push_back((uint32_t)(list_ends[i] - b));
    }
    InStrList il;
    const int64_t distinct = inlist_build_str(ptr.data(), len.data(),
                                              (int64_t)ptr.size(), &il.bytes,
                                              &il.slots, &il.mask);
    if (distinct < 0 || distinct > kInListMax) return YT_ERR_UNSUPPORTED;
    for (int64_t i = 0; i < m; i++) {
        const int64_t b = i ? text_ends[i - 1] : 0;
        const uint32_t tn = (uint32_t)(text_ends[i] - b);
        out[i] = (text_nulls && text_nulls[i])
            ? (uint8_t)has_null
            : (uint8_t)inlist_probe_str(il.slots.data(), il.mask, il.bytes.data(),
                                        inlist_str_hash(text_bytes + b, tn),
                                        text_bytes + b, tn);
    }
    return YT_OK;
}

/* strjoin_probe_slot's view of a slot's owner row, over packed host strings */
struct HostOwnerBytes {
    const char* bytes;
    const int64_t* ends;
    const char* operator()(int64_t row, uint32_t* len) const
    {
        const int64_t b = row ? ends[row - 1] : 0;
        *len = (uint32_t)(ends[row] - b);
        return bytes + b;
    }
};

extern "C" int yt_strjoin_eval(const char* f_bytes, const int64_t* f_ends,
                               const uint8_t* f_nulls, int64_t n,
                               const char* p_bytes, const int64_t* p_ends,
                               const uint8_t* p_nulls, int64_t m, int hash_bits,
                               int64_t* out_head_row, int64_t* out_chain_next)
{
    if (n < 0 || m < 0 || hash_bits < 1 || hash_bits > 64 ||
        (n && (!f_ends || !out_chain_next)) || (m && (!p_ends || !out_head_row)))
        return YT_ERR_INVALID_PLAN;
    const uint64_t hmask = hash_bits >= 64 ? ~0ULL : ((1ULL << hash_bits) - 1);
    /* setup_join_item's table: load <= 0.5, at least 2048 slots */
    uint64_t cap = 2048;
    while (cap < (uint64_t)(n ? n : 1) * 2) cap <<= 1;
    const uint64_t mask = cap - 1;
    std::vector<uint64_t> hkey(cap, 0);
    std::vector<int64_t> hrow(cap, -1), chead(cap, -1);
    const HostOwnerBytes owner{f_bytes, f_ends};
    int64_t null_row = -1;
    /* k_strjoin_build: every non-null row claims the first free slot from
     * its hash; null rows chain off null_row */
    for (int64_t r = 0; r < n; r++) {
        out_chain_next[r] = -1;
        if (f_nulls && f_nulls[r]) {
            out_chain_next[r] = null_row;
            null_row = r;
            continue;
        }
        uint32_t len = 0;
        const char* t = owner(r, &len);
        const uint64_t hash = inlist_str_hash(t, len) & hmask;
        uint64_t h = hash & mask;
        while (hrow[h] >= 0) h = (h + 1) & mask;
        hrow[h] = r;
        hkey[h] = hash;
    }
    /* k_strjoin_chain: push every row on its key's canonical slot */
    for (int64_t r = 0; r < n; r++) {
        if (f_nulls && f_nulls[r]) continue;
        uint32_t len = 0;
        const char* t = owner(r, &len);
        const int64_t h = strjoin_probe_slot(hkey.data(), hrow.data(), mask,
                                             inlist_str_hash(t, len) & hmask,
                                             t, len, owner);
        if (h < 0) return YT_ERR_INVALID_CHUNK;   /* unreachable */
        out_chain_next[r] = chead[h];
        chead[h] = r;
    }
    /* k_strjoin_entries + join_resolve: one probe per text, null joins null */
    for (int64_t i = 0; i < m; i++) {
        if (p_nulls && p_nulls[i]) { out_head_row[i] = null_row; continue; }
        const int64_t b = i ? p_ends[i - 1] : 0;
        const uint32_t tn = (uint32_t)(p_ends[i] - b);
        const int64_t h = strjoin_probe_slot(hkey.data(), hrow.data(), mask,
                                             inlist_str_hash(p_bytes + b, tn) & hmask,
                                             p_bytes + b, tn, owner);
        out_head_row[i] = h < 0 ? -1 : chead[h];
    }
    return YT_OK;
}

extern "C" int yt_strpred_eval(int op, int escape, const char* text,
                               int64_t text_len, const char* lit,
                               int64_t lit_len)
{
    if (text_len < 0 || lit_len < 0 || (text_len && !text) || (lit_len && !lit))
        return -1;
    if (op == YT_EX_LIKE) {
        if (escape < -1 || escape > 255) return -1;
        if (strpred_like_bad_pattern(lit, lit_len, escape)) return -2;
    }
    return strpred_eval(op, escape, text, text_len, lit, lit_len);
}

static bool is_string_col(const YtExpr* e, const DevPlan* p)
{
    return e && e->op == YT_EX_COLUMN && e->col >= 0 && e->col < p->ncols &&
           p->col_types[e->col] == YT_VT_STRING;
}

/* recognise one string-predicate leaf and compile it into one P_STR_PRED;
 * *matched = 0 when e is no such leaf (and nothing was emitted) */
static int compile_str_leaf(const YtExpr* e, DevPlan* p, StrPreds* sp,
                            int* matched, char* errbuf, size_t errlen)
{
    *matched = 0;
    StrPredDesc d;
    memset(&d, 0, sizeof(d));
    d.escape = -1;
    const YtExpr* lit = nullptr;
    if (e->op == YT_EX_IN) {
        const bool str_operand = is_string_col(e->a, p) ||
                                 (e->a && e->a->op == YT_EX_LIT_STRING);
        if (!str_operand) return YT_OK;       /* numeric form, or a mismatch */
        int rc = in_list_shape(e, errbuf, errlen);
        if (rc) return rc;
        if (e->a->op != YT_EX_COLUMN || e->a->col >= sp->primary_ncols) {
            set_err(errbuf, errlen,
                    "IN: a string operand must be a plain string column of "
                    "the primary chunk, in the filter");
            return YT_ERR_UNSUPPORTED;
        }
        std::vector<const char*> ptr;
        std::vector<uint32_t> len;
        bool has_null = false;
        for (int64_t i = 0; i < e->list_len; i++) {
            const YtValue& v = e->list[i];
            if (v.type == YT_VT_NULL) { has_null = true; continue; }
            if (v.type != YT_VT_STRING) {
                set_err(errbuf, errlen,
                        "type mismatch: an IN list value has another type "
                        "than the operand");
                return YT_ERR_INVALID_PLAN;
            }
            if (v.length > 0 && !v.data.str) {
                set_err(errbuf, errlen, "string literal without bytes");
                return YT_ERR_INVALID_PLAN;
            }
            ptr.push_back(v.data.str);
            len.push_back(v.length);
        }
        sp->any = true;
        *matched = 1;
        if (ptr.empty()) {
            /* no value to match: false for every text, the list's null flag
             * for a null text — constants, no bitmap */
            return emit_inst(p, P_STR_PRED, e->a->col,
                             kSpConst | (has_null ? kSpNullRes : 0),
                             errbuf, errlen);
        }
        if (sp->count >= kMaxStrPreds) {
            set_err(errbuf, errlen,
                    "more than 4 string predicates in one filter: not this round");
            return YT_ERR_UNSUPPORTED;
        }
        InStrList& il = sp->il[sp->count];
        const int64_t distinct = inlist_build_str(ptr.data(), len.data(),
                                                  (int64_t)ptr.size(), &il.bytes,
                                                  &il.slots, &il.mask);
        if (distinct < 0 || distinct > kInListMax)
            return in_list_too_long(errbuf, errlen);
        d.op = YT_EX_IN;
        d.col = e->a->col;
        const uint64_t bits = (uint64_t)sp->count | (has_null ? kSpNullRes : 0);
        sp->d[sp->count++] = d;
        return emit_inst(p, P_STR_PRED, d.col, bits, errbuf, errlen);
    }
    if (e->op >= YT_EX_EQ && e->op <= YT_EX_GE) {
        int op = e->op;
        const YtExpr* colx = nullptr;
        if (is_string_col(e->a, p)) {
            colx = e->a; lit = e->b;
        } else if (is_string_col(e->b, p)) {
            /* literal on the left: flip the operator */
            colx = e->b; lit = e->a;
            switch (op) {
            case YT_EX_LT: op = YT_EX_GT; break;
            case YT_EX_LE: op = YT_EX_GE; break;
            case YT_EX_GT: op = YT_EX_LT; break;
            case YT_EX_GE: op = YT_EX_LE; break;
            default: break;
            }
        } else {
            return YT_OK;
        }
        if (!lit || (lit->op != YT_EX_LIT_STRING && lit->op != YT_EX_LIT_NULL))
            return YT_OK;
        d.op = op;
        d.col = colx->col;
        if (lit->op == YT_EX_LIT_NULL) {
            /* null < any value, null == null: a constant per null and per
             * non-null text — no bitmap */
            const int lt_null = 0, eq_null = 1;      /* null text vs null */
            const int lt_val = 0, eq_val = 0;        /* value vs null */
            auto res = [&](int lt, int eq) -> bool {
                switch (op) {
                case YT_EX_EQ: return eq;
                case YT_EX_NE: return !eq;
                case YT_EX_LT: return lt;
                case YT_EX_LE: return lt || eq;
                case YT_EX_GT: return !(lt || eq);
                default: return !lt;
                }
            };
            uint64_t bits = kSpConst;
            if (res(lt_null, eq_null)) bits |= kSpNullRes;
            if (res(lt_val, eq_val)) bits |= kSpConstRes;
            sp->any = true;
            *matched = 1;
            return emit_inst(p, P_STR_PRED, d.col, bits, errbuf, errlen);
        }
    } else if (e->op == YT_EX_IS_PREFIX || e->op == YT_EX_IS_SUBSTR) {
        if (!e->a || e->a->op != YT_EX_LIT_STRING || !is_string_col(e->b, p)) {
            set_err(errbuf, errlen,
                    "type mismatch: is_prefix / is_substr take (string "
                    "literal, plain string column)");
            return YT_ERR_INVALID_PLAN;
        }
        d.op = e->op;
        d.col = e->b->col;
        lit = e->a;
    } else if (e->op == YT_EX_LIKE) {
        if (!e->b || e->b->op != YT_EX_LIT_STRING || !is_string_col(e->a, p)) {
            set_err(errbuf, errlen,
                    "type mismatch: LIKE takes (plain string column, string "
                    "literal)");
            return YT_ERR_INVALID_PLAN;
        }
        if (e->lit_i64 < -1 || e->lit_i64 > 255) {
            set_err(errbuf, errlen, "LIKE: escape must be one byte or -1");
            return YT_ERR_INVALID_PLAN;
        }
        d.op = e->op;
        d.col = e->a->col;
        d.escape = (int)e->lit_i64;
        lit = e->b;
    } else {
        return YT_OK;
    }
    if (lit->lit_len < 0 || (lit->lit_len > 0 && !lit->lit_str)) {
        set_err(errbuf, errlen, "string literal without bytes");
        return YT_ERR_INVALID_PLAN;
    }
    d.lit = lit->lit_str;
    d.lit_len = lit->lit_len;
    if (d.op == YT_EX_LIKE &&
        strpred_like_bad_pattern(d.lit, d.lit_len, d.escape)) {
        set_err(errbuf, errlen, "LIKE: pattern ends in a lone escape");
        return YT_ERR_INVALID_PLAN;
    }
    if (sp->count >= kMaxStrPreds) {
        set_err(errbuf, errlen,
                "more than 4 string predicates in one filter: not this round");
        return YT_ERR_UNSUPPORTED;
    }
    /* a null text: the relational ops answer by the null rule (null < any
     * value), the functions answer null */
    uint64_t bits = (uint64_t)sp->count;
    if (d.op >= YT_EX_EQ && d.op <= YT_EX_GE) {
        if (d.op == YT_EX_NE || d.op == YT_EX_LT || d.op == YT_EX_LE)
            bits |= kSpNullRes;
    } else {
        bits |= kSpNullIsNull;
    }
    sp->d[sp->count++] = d;
    sp->any = true;
    *matched = 1;
    return emit_inst(p, P_STR_PRED, d.col, bits, errbuf, errlen);
}

/* the filter: AND/OR/NOT over string-predicate leaves and ordinary
 * subexpressions; sp == nullptr refuses every string predicate */
static int compile_filter(const YtExpr* e, DevPlan* p, StrPreds* sp,
                          char* errbuf, size_t errlen, int* need = nullptr)
{
    if (!e) { set_err(errbuf, errlen, "null expr"); return YT_ERR_INVALID_PLAN; }
    if (e->op == YT_EX_AND || e->op == YT_EX_OR || e->op == YT_EX_NOT) {
        /* stack slots as in compile_expr */
        int na = 1, nb = 0;
        int rc = compile_filter(e->a, p, sp, errbuf, errlen, &na);
        if (rc) return rc;
        if (e->op != YT_EX_NOT) {
            rc = compile_filter(e->b, p, sp, errbuf, errlen, &nb);
            if (rc) return rc;
            na = std::max(na, 1 + nb);
            rc = need_check(na, errbuf, errlen);
            if (rc) return rc;
        }
        if (need) *need = na;
        return emit_inst(p, e->op, e->col, 0, errbuf, errlen);
    }
    if (need) *need = 1;            /* a string-predicate leaf pushes one value */
    if (sp) {
        int matched = 0;
        int rc = compile_str_leaf(e, p, sp, &matched, errbuf, errlen);
        if (rc || matched) return rc;
    }
    if (expr_has_strlit(e)) {
        set_err(errbuf, errlen,
                "type mismatch: a string literal compares with a plain "
                "string column only");
        return YT_ERR_INVALID_PLAN;
    }
    if (expr_reads_string(e, p->col_types, p->ncols)) {
        set_err(errbuf, errlen,
                "string column inside a filter or key expression: "
                "unsupported on the GPU (string predicates take one plain "
                "string column and one literal)");
        return YT_ERR_UNSUPPORTED;
    }
    int len = 0;
    return compile_expr(e, p, sp, &len, errbuf, errlen, need);
}

static int build_devplan(const YtPlan* plan, const YtChunk* chunk, DevPlan* p,
                         StrPreds* sp, char* errbuf, size_t errlen)
{
    memset(p, 0, sizeof(*p));
    p->ncols = chunk->column_count;
    if (sp) sp->primary_ncols = chunk->column_count;
    for (const YtJoin* J = plan->join; J; J = J->next)
        p->ncols += J->foreign_value_count;
    if (p->ncols > kMaxCols) { set_err(errbuf, errlen, "too many columns"); return YT_ERR_UNSUPPORTED; }
    for (int c = 0; c < chunk->column_count; c++) p->col_types[c] = (uint8_t)chunk->columns[c].value_type;
    {
        int at = chunk->column_count;
        for (const YtJoin* J = plan->join; J; J = J->next)
            for (int j = 0; j < J->foreign_value_count; j++)
                p->col_types[at++] =
                    (uint8_t)J->foreign->columns[J->foreign_value_cols[j]].value_type;
    }
    {
        /* the typing rules, before anything is compiled or launched */
        int trc = check_plan_types(plan, p->col_types, p->ncols, errbuf, errlen);
        if (trc) return trc;
    }
    for (int c = 0; c < chunk->column_count; c++) {
        const YtColumn& col = chunk->columns[c];
        int shift = 0;
        if (col.segment_count > 0) {
            int32_t r0 = col.segments[0].row_count;
            if (r0 > 0 && (r0 & (r0 - 1)) == 0) {
                int ok = 1;
                for (int i = 0; i + 1 < col.segment_count; i++)
                    if (col.segments[i].row_count != r0) { ok = 0; break; }
                if (ok && col.segments[col.segment_count - 1].row_count <= r0) {
                    while ((1 << (shift + 1)) <= r0) shift++;
                    if ((1 << shift) != r0) shift = 0;
                }
            }
        }
        p->col_uniform_shift[c] = shift;
    }

    if (plan->key_count > 1) {
        /* composite packed key: plain int64/uint64/boolean key columns,
         * widths resolved after segment parse (see pack_group_key) */
        if (plan->key_count > kMaxPackKeys) {
            set_err(errbuf, errlen, "GPU path: at most 4 group keys this round");
            return YT_ERR_UNSUPPORTED;
        }
        p->kp_count = plan->key_count;
        for (int i = 0; i < plan->key_count; i++) {
            int c;
            if (!expr_is_col(plan->keys[i], &c) || c >= p->ncols) {
                set_err(errbuf, errlen,
                        "multi-key GROUP BY: plain key columns this round");
                return YT_ERR_UNSUPPORTED;
            }
            if (c >= chunk->column_count) {
                set_err(errbuf, errlen,
                        "multi-key GROUP BY over joined columns: not this round");
                return YT_ERR_UNSUPPORTED;
            }
            uint8_t vt = p->col_types[c];
            if (vt != YT_VT_INT64 && vt != YT_VT_UINT64 && vt != YT_VT_BOOLEAN &&
                vt != YT_VT_STRING) {
                set_err(errbuf, errlen,
                        "multi-key GROUP BY: int64/uint64/boolean/string keys "
                        "this round");
                return YT_ERR_UNSUPPORTED;
            }
            p->kp_col[i] = c;
            p->kp_signed[i] = vt == YT_VT_INT64;
            /* a STRING key packs its string id (setup_strkey_ids) */
            if (vt != YT_VT_STRING) continue;
            if (plan->join) {
                set_err(errbuf, errlen,
                        "multi-key GROUP BY: a string key beside a join: not "
                        "this round");
                return YT_ERR_UNSUPPORTED;
            }
            if (plan->project_count) {
                set_err(errbuf, errlen,
                        "multi-key GROUP BY: post-projections on a plan with a "
                        "string key: not this round");
                return YT_ERR_UNSUPPORTED;
            }
            uint64_t hmask = 0;
            hexpr_cols(plan->having, &hmask);
            if ((hmask >> i) & 1) {
                set_err(errbuf, errlen, "HAVING over string values: not this round");
                return YT_ERR_UNSUPPORTED;
            }
        }
    }
    if (plan->agg_count == 0 && plan->key_count == 0) {
        if (plan->project_count < 1 || plan->project_count > kMaxProj) {
            set_err(errbuf, errlen, "scan mode needs 1..8 projections");
            return YT_ERR_UNSUPPORTED;
        }
    } else if (plan->agg_count > 0)
    if (plan->agg_count < 1 || plan->agg_count > kMaxAggs) { set_err(errbuf, errlen, "need 1..4 aggregates"); return YT_ERR_UNSUPPORTED; }
    for (int a = 0; a < plan->agg_count; a++) {
        int f = plan->aggs[a]->func;
        if (f < YT_AGG_SUM || f > YT_AGG_AVG) {
            set_err(errbuf, errlen, "unsupported aggregate");
            return YT_ERR_UNSUPPORTED;
        }
    }

    int rc;
    if (plan->key_count == 1 && plan->keys[0]->op != YT_EX_COLUMN &&
        (expr_reads_string(plan->keys[0], p->col_types, p->ncols) ||
         expr_has_strlit(plan->keys[0]))) {
        set_err(errbuf, errlen,
                "string column inside a filter or key expression: "
                "unsupported on the GPU (string predicates belong to the "
                "filter)");
        return YT_ERR_UNSUPPORTED;
    }
    if (plan->filter) {
        p->filter_off = p->prog_len;
        rc = compile_filter(plan->filter, p, sp, errbuf, errlen);
        if (rc) return rc;
        p->filter_len = p->prog_len - p->filter_off;
        if (sp && sp->any && plan->join) {
            set_err(errbuf, errlen,
                    "string predicate beside a join: not this round");
            return YT_ERR_UNSUPPORTED;
        }
    }
    if (plan->key_count == 1) {
        p->key_off = p->prog_len;
        rc = compile_expr(plan->keys[0], p, sp, &p->key_len, errbuf, errlen);
        if (rc) return rc;
        p->key_len = p->prog_len - p->key_off;
    }
    p->agg_count = plan->agg_count;
    for (int a = 0; a < plan->agg_count; a++) {
        p->agg_func[a] = plan->aggs[a]->func;
        if (plan->aggs[a]->func < YT_AGG_SUM ||
            plan->aggs[a]->func > YT_AGG_AVG) {
            set_err(errbuf, errlen, "unknown aggregate function");
            return YT_ERR_UNSUPPORTED;
        }
        if (plan->aggs[a]->func == YT_AGG_FIRST ||
            plan->aggs[a]->func == YT_AGG_AVG) {
            /* no packed state format for these: strings can't live in one
             * slot word (first), and avg-of-avgs is wrong (totals fold) */
            uint8_t at = expr_static_type(plan->aggs[a]->arg, p->col_types);
            if (plan->aggs[a]->func == YT_AGG_AVG &&
                at != YT_VT_INT64 && at != YT_VT_UINT64 && at != YT_VT_DOUBLE) {
                set_err(errbuf, errlen, "avg: int64/uint64/double argument only");
                return YT_ERR_UNSUPPORTED;
            }
            if (plan->aggs[a]->func == YT_AGG_FIRST && at == YT_VT_STRING) {
                set_err(errbuf, errlen,
                        "first(): string argument is oracle-only this round");
                return YT_ERR_UNSUPPORTED;
            }
            if (plan->aggs[a]->func == YT_AGG_AVG && plan->with_totals) {
                set_err(errbuf, errlen, "avg: WITH TOTALS not this round");
                return YT_ERR_UNSUPPORTED;
            }
        }
        if (plan->aggs[a]->func != YT_AGG_SUM1 &&
            (expr_reads_string(plan->aggs[a]->arg, p->col_types, p->ncols) ||
             expr_has_strlit(plan->aggs[a]->arg))) {
            set_err(errbuf, errlen,
                    "string column inside an aggregate argument: "
                    "unsupported on the GPU");
            return YT_ERR_UNSUPPORTED;
        }
        if (plan->aggs[a]->func != YT_AGG_SUM1) {
            p->agg_off[a] = p->prog_len;
            rc = compile_expr(plan->aggs[a]->arg, p, sp, &p->agg_len[a], errbuf, errlen);
            if (rc) return rc;
            p->agg_len[a] = p->prog_len - p->agg_off[a];
        }
    }
    if (plan->agg_count == 0) {
        p->proj_count = plan->project_count;
        for (int pj = 0; pj < plan->project_count; pj++) {
            if (expr_has_strlit(plan->projects[pj])) {
                set_err(errbuf, errlen,
                        "string literal or predicate inside a projection: "
                        "unsupported on the GPU");
                return YT_ERR_UNSUPPORTED;
            }
            p->proj_off[pj] = p->prog_len;
            int sc;
            if (expr_is_col(plan->projects[pj], &sc) && sc >= 0 &&
                sc < p->ncols && p->col_types[sc] == YT_VT_STRING) {
                /* a bare STRING column: one P_STR_REF, plain scans only */
                const char* why = nullptr;
                if (sc >= chunk->column_count)
                    why = "foreign string column in a projection: not this round";
                else if (plan->join)
                    why = "string projection beside a join: not this round";
                else if (plan->key_count > 0)
                    why = "string projection outside a plain scan: unsupported "
                          "on the GPU";
                for (int i = 0; !why && i < plan->order_count; i++)
                    if (plan->order_cols && plan->order_cols[i] == pj)
                        why = "ORDER BY on a string column in a plain scan: "
                              "not this round";
                if (why) {
                    set_err(errbuf, errlen, why);
                    return YT_ERR_UNSUPPORTED;
                }
                rc = emit_inst(p, P_STR_REF, sc, 0, errbuf, errlen);
                if (rc) return rc;
                p->proj_len[pj] = 1;
                continue;
            }
            if (expr_reads_string(plan->projects[pj], p->col_types, p->ncols)) {
                set_err(errbuf, errlen,
                        "string column inside a projection expression: "
                        "unsupported on the GPU (a projection may be one plain "
                        "string column)");
                return YT_ERR_UNSUPPORTED;
            }
            rc = compile_expr(plan->projects[pj], p, sp, &p->proj_len[pj], errbuf, errlen);
            if (rc) return rc;
            p->proj_len[pj] = p->prog_len - p->proj_off[pj];
        }
    }
    return YT_OK;
}

/* fast-shape analysis: filter = none | cmp(col, lit) | AND of two bounds;
 * key = direct int64 column | none; sum args = direct int64 columns */
static bool expr_is_col(const YtExpr* e, int* col)
{
    if (e && e->op == YT_EX_COLUMN) { *col = e->col; return true; }
    return false;
}

static bool match_bound(const YtExpr* e, const uint8_t* col_types,
                        int* col, int64_t* lo, int64_t* hi)
{
    /* col cmp lit / lit cmp col, int64 only */
    int c;
    int64_t k;
    int op = e->op;
    if (op < YT_EX_EQ || op > YT_EX_GE || op == YT_EX_NE) return false;
    if (expr_is_col(e->a, &c) && e->b && e->b->op == YT_EX_LIT_I64) {
        k = e->b->lit_i64;
    } else if (expr_is_col(e->b, &c) && e->a && e->a->op == YT_EX_LIT_I64) {
        k = e->a->lit_i64;
        /* mirror: lit cmp col → col cmp' lit */
        switch (op) {
        case YT_EX_LT: op = YT_EX_GT; break;
        case YT_EX_LE: op = YT_EX_GE; break;
        case YT_EX_GT: op = YT_EX_LT; break;
        case YT_EX_GE: op = YT_EX_LE; break;
        default: break;
        }
    } else {
        return false;
    }
    if (col_types[c] != YT_VT_INT64) return false;
    *col = c;
    *lo = INT64_MIN; *hi = INT64_MAX;
    switch (op) {
    case YT_EX_EQ: *lo = *hi = k; break;
    case YT_EX_LT: if (k == INT64_MIN) return false; *hi = k - 1; break;
    case YT_EX_LE: *hi = k; break;
    case YT_EX_GT: if (k == INT64_MAX) return false; *lo = k + 1; break;
    case YT_EX_GE: *lo = k; break;
    default: return false;
    }
    return true;
}

static void analyze_fast(const YtPlan* plan, const YtChunk* chunk, FastShape* fs)
{
    memset(fs, 0, sizeof(*fs));
    fs->filter_col = -1;
    fs->key_col = -1;
    if (plan->join) return;           /* joined plans run the generic path */

    const uint8_t* ct = nullptr;
    static uint8_t types[kMaxCols];
    for (int c = 0; c < chunk->column_count && c < kMaxCols; c++)
        types[c] = (uint8_t)chunk->columns[c].value_type;
    ct = types;

    /* all segments of all columns must be DirectDense int64 and cut at the
     * same rows; k_scan_fast also needs uniform interior row counts, the
     * partitioned path masks its tiles per segment and takes any (ragged) */
    int32_t seg_cnt0 = chunk->columns[0].segment_count;
    int32_t rows0 = seg_cnt0 ? chunk->columns[0].segments[0].row_count : 0;
    bool ragged = false;
    for (int c = 0; c < chunk->column_count; c++) {
        const YtColumn& col = chunk->columns[c];
        if (col.value_type != YT_VT_INT64) return;
        if (col.segment_count != seg_cnt0) return;
        for (int s = 0; s < col.segment_count; s++) {
            if (col.segments[s].type != YT_SEG_DIRECT_DENSE) return;
            if (col.segments[s].row_count != chunk->columns[0].segments[s].row_count) return;
            if (s < col.segment_count - 1 && col.segments[s].row_count != rows0) ragged = true;
            if (col.segments[s].row_count > rows0) ragged = true;
        }
    }
    if (seg_cnt0 == 0) return;

    if (plan->filter) {
        int64_t lo, hi;
        int col;
        if (match_bound(plan->filter, ct, &col, &lo, &hi)) {
            fs->filter_col = col; fs->filter_lo = lo; fs->filter_hi = hi;
        } else if (plan->filter->op == YT_EX_AND) {
            int c1, c2;
            int64_t lo1, hi1, lo2, hi2;
            if (!match_bound(plan->filter->a, ct, &c1, &lo1, &hi1)) return;
            if (!match_bound(plan->filter->b, ct, &c2, &lo2, &hi2)) return;
            if (c1 != c2) return;
            fs->filter_col = c1;
            fs->filter_lo = std::max(lo1, lo2);
            fs->filter_hi = std::min(hi1, hi2);
        } else {
            return;
        }
    }
    if (plan->key_count == 1) {
        int col;
        if (!expr_is_col(plan->keys[0], &col)) return;
        if (ct[col] != YT_VT_INT64) return;
        fs->key_col = col;
    } else if (plan->key_count > 1) {
        return;
    }
    fs->nsum = 0;
    for (int a = 0; a < plan->agg_count; a++) {
        if (plan->aggs[a]->func == YT_AGG_SUM1) { fs->have_sum1 = 1; continue; }
        if (plan->aggs[a]->func != YT_AGG_SUM) return;
        int col;
        if (!expr_is_col(plan->aggs[a]->arg, &col)) return;
        if (ct[col] != YT_VT_INT64) return;
        if (fs->nsum >= kMaxAggs) return;
        fs->sum_col[fs->nsum] = col;
        fs->sum_slot[fs->nsum] = a;
        fs->nsum++;
    }
    if (fs->nsum == 0 && fs->filter_col < 0 && fs->key_col < 0) {
        return;   /* pure row count with no staged column — generic path */
    }
    fs->valid = ragged ? 0 : 1;
    fs->ragged = ragged ? 1 : 0;
}

/* ------------------------------------------------------------------ */
/* host-side projection evaluation over a finalized group row           */
/* (mirrors MakeCodegenProjectOp over [keys..., aggregates...])        */

struct HVal { uint8_t type; uint64_t bits; };

static int heval(const YtExpr* e, const HVal* row, int nrow, HVal* out);

/* The numeric IN lists of the expression heval is running (HAVING), sorted
 * by hin_prepare on the calling thread; a node that is not among them is
 * compared value by value. */
static thread_local const std::vector<InNumSet>* t_hin = nullptr;

static int hin_collect(const YtExpr* e, std::vector<InNumSet>* sets,
                       char* errbuf, size_t errlen)
{
    if (!e) return YT_OK;
    if (e->op == YT_EX_IN) {
        int rc = in_list_shape(e, errbuf, errlen);
        if (rc) return rc;
        uint8_t vt = 0;
        for (int64_t i = 0; i < e->list_len && !vt; i++)
            if (e->list[i].type != YT_VT_NULL) vt = e->list[i].type;
        if (vt == YT_VT_DOUBLE) {
            set_err(errbuf, errlen, "IN over a DOUBLE operand: not this round");
            return YT_ERR_UNSUPPORTED;
        }
        if (vt && vt != YT_VT_INT64 && vt != YT_VT_UINT64 && vt != YT_VT_BOOLEAN) {
            set_err(errbuf, errlen,
                    "type mismatch: IN takes an int64, uint64 or boolean operand");
            return YT_ERR_INVALID_PLAN;
        }
        sets->emplace_back();
        rc = in_num_prepare(e, vt, &sets->back(), errbuf, errlen);
        if (rc) return rc;
        return hin_collect(e->a, sets, errbuf, errlen);
    }
    int rc = hin_collect(e->a, sets, errbuf, errlen);
    if (rc) return rc;
    return hin_collect(e->b, sets, errbuf, errlen);
}

/* YT_EX_IN on the host: the operand equals one of the values; null matches
 * null; the result is never null */
static int heval_in(const YtExpr* e, const HVal* row, int nrow, HVal* out)
{
    if (!e->a || e->b || e->list_len < 0 || (e->list_len > 0 && !e->list))
        return YT_ERR_INVALID_PLAN;
    HVal a;
    int rc = heval(e->a, row, nrow, &a);
    if (rc) return rc;
    if (a.type == YT_VT_DOUBLE || a.type == YT_VT_STRING) return YT_ERR_UNSUPPORTED;
    const uint64_t abits = a.type == YT_VT_BOOLEAN ? (uint64_t)(a.bits != 0) : a.bits;
    out->type = YT_VT_BOOLEAN;
    out->bits = 0;
    if (t_hin) {
        for (const InNumSet& s : *t_hin) {
            if (s.e != e) continue;
            if (a.type == YT_VT_NULL) { out->bits = s.has_null; return YT_OK; }
            if (s.type && s.type != a.type) return YT_ERR_INVALID_PLAN;
            out->bits = std::binary_search(s.sorted.begin(), s.sorted.end(), abits);
            return YT_OK;
        }
    }
    for (int64_t i = 0; i < e->list_len; i++) {
        const YtValue& v = e->list[i];
        if (v.type == YT_VT_NULL) {
            if (a.type == YT_VT_NULL) out->bits = 1;
            continue;
        }
        if (a.type == YT_VT_NULL) continue;
        if (v.type != a.type) return YT_ERR_INVALID_PLAN;
        const uint64_t vb = v.type == YT_VT_BOOLEAN ? (uint64_t)(v.data.bits != 0)
                                                    : v.data.bits;
        if (vb == abits) out->bits = 1;
    }
    return YT_OK;
}

/* An integer literal operand beside the value `other`: the adoption
 * compile_expr does from static types. check_plan_types has passed, so a
 * non-null value has its node's static type, and reading the neighbour's type
 * off its value decides the same; beside a null neighbour the literal's type
 * changes no result. */
static inline void hval_adopt(const YtExpr* e, HVal* v, const HVal& other)
{
    if (e->op != YT_EX_LIT_I64) return;
    if (other.type == YT_VT_DOUBLE) {
        const double d = (double)e->lit_i64;
        v->type = YT_VT_DOUBLE;
        memcpy(&v->bits, &d, 8);
    } else if (other.type == YT_VT_UINT64) {
        v->type = YT_VT_UINT64;
    }
}

static int heval(const YtExpr* e, const HVal* row, int nrow, HVal* out)
{
    switch (e->op) {
    case YT_EX_IN:
        return heval_in(e, row, nrow, out);
    case YT_EX_COLUMN:
        if (e->col < 0 || e->col >= nrow) return YT_ERR_INVALID_PLAN;
        *out = row[e->col];
        return YT_OK;
    case YT_EX_LIT_I64: out->type = YT_VT_INT64; out->bits = (uint64_t)e->lit_i64; return YT_OK;
    case YT_EX_LIT_DOUBLE: out->type = YT_VT_DOUBLE; memcpy(&out->bits, &e->lit_dbl, 8); return YT_OK;
    case YT_EX_LIT_NULL: out->type = YT_VT_NULL; out->bits = 0; return YT_OK;
    case YT_EX_NOT: {
        HVal a;
        int rc = heval(e->a, row, nrow, &a);
        if (rc) return rc;
        if (a.type == YT_VT_NULL) { *out = a; return YT_OK; }
        out->type = YT_VT_BOOLEAN; out->bits = !a.bits;
        return YT_OK;
    }
    default: break;
    }
    HVal a, b;
    int rc = heval(e->a, row, nrow, &a);
    if (rc) return rc;
    rc = heval(e->b, row, nrow, &b);
    if (rc) return rc;
    if (op_is_arith(e->op) || op_is_rel(e->op)) {
        hval_adopt(e->a, &a, b);
        hval_adopt(e->b, &b, a);
    }
    out->type = YT_VT_NULL; out->bits = 0;
    if (e->op >= YT_EX_ADD && e->op <= YT_EX_MOD) {
        if (a.type == YT_VT_NULL || b.type == YT_VT_NULL) return YT_OK;
        if (a.type == YT_VT_DOUBLE) {
            double x, y, z = 0;
            memcpy(&x, &a.bits, 8);
            memcpy(&y, &b.bits, 8);
            switch (e->op) {
            case YT_EX_ADD: z = x + y; break;
            case YT_EX_SUB: z = x - y; break;
            case YT_EX_MUL: z = x * y; break;
            case YT_EX_DIV: z = x / y; break;
            default: return YT_ERR_UNSUPPORTED;
            }
            out->type = YT_VT_DOUBLE;
            memcpy(&out->bits, &z, 8);
            return YT_OK;
        }
        uint64_t x = a.bits, y = b.bits, z = 0;
        int sgn = (a.type == YT_VT_INT64);
        switch (e->op) {
        case YT_EX_ADD: z = x + y; break;
        case YT_EX_SUB: z = x - y; break;
        case YT_EX_MUL: z = x * y; break;
        case YT_EX_DIV:
        case YT_EX_MOD:
            if (y == 0) return YT_ERR_DIV_ZERO;
            if (sgn) {
                int64_t sx = (int64_t)x, sy = (int64_t)y;
                if (sx == INT64_MIN && sy == -1) z = (e->op == YT_EX_DIV) ? (uint64_t)INT64_MIN : 0;
                else z = (uint64_t)((e->op == YT_EX_DIV) ? sx / sy : sx % sy);
            } else {
                z = (e->op == YT_EX_DIV) ? x / y : x % y;
            }
            break;
        }
        out->type = a.type;
        out->bits = z;
        return YT_OK;
    }
    if (e->op >= YT_EX_EQ && e->op <= YT_EX_GE) {
        int lt, eq, force_true = 0;
        if (a.type == YT_VT_NULL || b.type == YT_VT_NULL) {
            unsigned ln = (a.type == YT_VT_NULL), rn = (b.type == YT_VT_NULL);
            lt = rn < ln; eq = ln == rn;
        } else if (a.type == YT_VT_DOUBLE) {
            double x, y;
            memcpy(&x, &a.bits, 8);
            memcpy(&y, &b.bits, 8);
            int unordered = (x != x) || (y != y);
            lt = unordered || (x < y);
            eq = unordered || (x == y);
            force_true = unordered;
        } else if (a.type == YT_VT_INT64) {
            int64_t x = (int64_t)a.bits, y = (int64_t)b.bits;
            lt = x < y; eq = x == y;
        } else {
            lt = a.bits < b.bits; eq = a.bits == b.bits;
        }
        int r = 1;
        if (!force_true) {
            switch (e->op) {
            case YT_EX_EQ: r = eq; break;
            case YT_EX_NE: r = !eq; break;
            case YT_EX_LT: r = lt; break;
            case YT_EX_LE: r = lt || eq; break;
            case YT_EX_GT: r = !(lt || eq); break;
            case YT_EX_GE: r = !lt; break;
            }
        }
        out->type = YT_VT_BOOLEAN;
        out->bits = (uint64_t)r;
        return YT_OK;
    }
    if (e->op == YT_EX_AND || e->op == YT_EX_OR) {
        int an = (a.type == YT_VT_NULL), bn = (b.type == YT_VT_NULL);
        int av = an ? 0 : (a.bits != 0), bv = bn ? 0 : (b.bits != 0);
        if (e->op == YT_EX_AND) {
            if ((!an && !av) || (!bn && !bv)) { out->type = YT_VT_BOOLEAN; out->bits = 0; }
            else if (!an && !bn) { out->type = YT_VT_BOOLEAN; out->bits = 1; }
        } else {
            if ((!an && av) || (!bn && bv)) { out->type = YT_VT_BOOLEAN; out->bits = 1; }
            else if (!an && !bn) { out->type = YT_VT_BOOLEAN; out->bits = 0; }
        }
        return YT_OK;
    }
    return YT_ERR_UNSUPPORTED;
}

/* ------------------------------------------------------------------ */
/* device chunk setup                                                  */

struct DeviceRun {
    /* string ids of the composite key's STRING components (setup_strkey_ids) */
    StrKeyDev strkeys = {};
    std::vector<DevSeg> h_segs;
    std::vector<int32_t> h_off, h_cnt;
    DevSeg* d_segs = nullptr;
    SegEx* d_segex = nullptr;
    int32_t* d_off = nullptr;
    int32_t* d_cnt = nullptr;
    /* d_maxw, d_err, d_colnull and d_zzrange point into d_setup */
    SetupWords* d_setup = nullptr;
    SetupWords* h_setup = nullptr;     /* pinned: the image, then the readback */
    unsigned* d_maxw = nullptr;
    unsigned* d_err = nullptr;
    TableHdr* d_th = nullptr;
    unsigned long long* d_slots = nullptr;
    OutGroup* d_groups = nullptr;
    unsigned long long* d_counter = nullptr;
    unsigned long long* d_gaccum = nullptr;
    FastCol* d_fastcols = nullptr;
    unsigned* d_colnull = nullptr;
    unsigned long long* d_zzrange = nullptr;   /* [0..kMaxCols) min, [kMaxCols..) max */
    unsigned long long* d_cursors = nullptr;
    void* d_recs = nullptr;
    unsigned long long* d_ncursors = nullptr;
    uint64_t* d_nrecs = nullptr;
    uint64_t nslots = 0;
    int nsegs = 0;
    int64_t groups_capacity = 0;
    bool groups_compacted = false;     /* d_groups already holds final groups */
    /* set by yt_gpu_query_execute alone: the partitioned path may leave
     * SlimGroups in d_groups. groups_slim says that it did. */
    bool want_slim = false;
    bool groups_slim = false;
    /* the table header as run_partitioned last read it (pinned); valid
     * while th_valid, so the caller need not fetch it again */
    TableHdr* h_th = nullptr;
    bool th_valid = false;
    unsigned col_null_flags[kMaxCols] = {0};
    uint64_t col_zzmin[kMaxCols] = {0};
    uint64_t col_zzmax[kMaxCols] = {0};
    hipStream_t stream = 0;
    PoolScope ps;                      /* owns every block above */
};

/* diagnostic: which scan path the last query on this thread took
 * (YT_SCAN_PATH_* bits); written by run_partitioned / run_scan /
 * run_string_group, and by the plain-scan dispatch (0, or
 * YT_SCAN_PATH_PROJ_COMPACT from run_scan_project) */
static thread_local uint32_t t_last_scan_path = 0;

extern "C" uint32_t yt_gpu_debug_last_scan_path(void)
{
    return t_last_scan_path;
}

/* diagnostic: YT_TOPK_* bits of this thread's last query; only run_scan_topk
 * writes it */
static thread_local uint32_t t_last_topk = 0;

extern "C" uint32_t yt_gpu_debug_last_topk(void)
{
    return t_last_topk;
}

extern "C" int32_t yt_gpu_debug_partition_tile_rows(int large)
{
    return large ? kPartTileMax : kPartTileMin;
}

/* diagnostic: kPartVariant* bits of the process's last phase-A launch; only
 * run_partitioned writes it */
static std::atomic<int32_t> g_last_part_variant{0};

extern "C" int32_t yt_gpu_debug_partition_variant(void)
{
    return g_last_part_variant.load(std::memory_order_relaxed);
}

extern "C" int32_t yt_gpu_debug_bucket_pass_records(void)
{
    return kBucketPassRecords;
}

static uint64_t next_pow2(uint64_t x)
{
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

/* builds device segment descriptors; returns YT status.
 * input_row_limit > 0 truncates the scan to the first N rows — exactly the
 * reference's InputRowLimit interrupt semantics (rows are consumed in row
 * order; registry.cpp:259-265, TInterruptedIncompleteException). */
static int setup_chunk(const YtChunk* chunk, DeviceRun* R, unsigned* maxw_out,
                       int64_t input_row_limit, int* clamped,
                       char* errbuf, size_t errlen)
{
    int ncols = chunk->column_count;
    if (clamped) *clamped = 0;
    R->h_off.resize(ncols);
    R->h_cnt.resize(ncols);
    for (int c = 0; c < ncols; c++) {
        const YtColumn& col = chunk->columns[c];
        R->h_off[c] = (int32_t)R->h_segs.size();
        int32_t kept = 0;
        int64_t row = 0;
        for (int s = 0; s < col.segment_count; s++) {
            const YtSegment& seg = col.segments[s];
            int32_t rows_here = seg.row_count;
            if (input_row_limit > 0) {
                if (row >= input_row_limit) {
                    if (clamped) *clamped = 1;
                    row += seg.row_count;
                    continue;
                }
                if (row + rows_here > input_row_limit) {
                    rows_here = (int32_t)(input_row_limit - row);
                    if (clamped) *clamped = 1;
                }
            }
            DevSeg d;
            d.type = seg.type;
            d.is_signed = (col.value_type == YT_VT_STRING) ? 2
                        : (col.value_type == YT_VT_INT64);
            d.start_row = row;
            d.row_count = rows_here;
            d.col = c;
            d.min_value = seg.min_value;
            d.blob = (const uint64_t*)seg.data;
            d.blob_bytes = seg.data_size;
            R->h_segs.push_back(d);
            kept++;
            row += seg.row_count;
        }
        R->h_cnt[c] = kept;
        if (row != chunk->row_count) {
            set_err(errbuf, errlen, "segment row counts do not sum to chunk rows");
            return YT_ERR_INVALID_CHUNK;
        }
    }
    R->nsegs = (int)R->h_segs.size();
    if (R->nsegs == 0) return YT_OK;

    HIP_CHECK(R->ps.dev(&R->d_segs, sizeof(DevSeg) * R->nsegs));
    HIP_CHECK(R->ps.dev(&R->d_segex, sizeof(SegEx) * R->nsegs));
    HIP_CHECK(R->ps.dev(&R->d_off, sizeof(int32_t) * ncols));
    HIP_CHECK(R->ps.dev(&R->d_cnt, sizeof(int32_t) * ncols));
    /* the scalar words: one block, set by one copy of a pinned host image
     * and read back into it by one copy (it was five fills and four copies
     * into pageable memory) */
    HIP_CHECK(R->ps.dev(&R->d_setup, sizeof(SetupWords)));
    HIP_CHECK(R->ps.host(&R->h_setup, sizeof(SetupWords)));
    R->d_maxw = &R->d_setup->maxw;
    R->d_err = R->d_setup->err;
    R->d_colnull = R->d_setup->col_null;
    R->d_zzrange = R->d_setup->zzmin;
    static_assert(offsetof(SetupWords, zzmax) ==
                  offsetof(SetupWords, zzmin) + sizeof(uint64_t) * kMaxCols,
                  "d_zzrange: kMaxCols minima, then kMaxCols maxima");
    memset(R->h_setup, 0, sizeof(SetupWords));
    memset(R->h_setup->zzmin, 0xFF, sizeof(R->h_setup->zzmin));
    HIP_CHECK(hipMemcpyAsync(R->d_setup, R->h_setup, sizeof(SetupWords),
                             hipMemcpyHostToDevice, R->stream));
    HIP_CHECK(hipMemcpyAsync(R->d_segs, R->h_segs.data(), sizeof(DevSeg) * R->nsegs,
                             hipMemcpyHostToDevice, R->stream));
    HIP_CHECK(hipMemcpyAsync(R->d_off, R->h_off.data(), sizeof(int32_t) * ncols,
                             hipMemcpyHostToDevice, R->stream));
    HIP_CHECK(hipMemcpyAsync(R->d_cnt, R->h_cnt.data(), sizeof(int32_t) * ncols,
                             hipMemcpyHostToDevice, R->stream));
    HIP_CHECK(ytql_launch_parse_segments(R->d_segs, R->nsegs, R->d_segex, R->d_maxw,
                                         R->d_colnull, R->d_zzrange,
                                         R->d_zzrange + kMaxCols, R->stream));
    HIP_CHECK(ytql_launch_scan_nullflags(R->d_segs, R->d_segex, R->nsegs,
                                         R->d_colnull, R->stream));
    HIP_CHECK(hipMemcpyAsync(R->h_setup, R->d_setup, sizeof(SetupWords),
                             hipMemcpyDeviceToHost, R->stream));
    HIP_CHECK(hipStreamSynchronize(R->stream));
    *maxw_out = R->h_setup->maxw;
    memcpy(R->col_null_flags, R->h_setup->col_null, sizeof(R->col_null_flags));
    memcpy(R->col_zzmin, R->h_setup->zzmin, sizeof(R->col_zzmin));
    memcpy(R->col_zzmax, R->h_setup->zzmax, sizeof(R->col_zzmax));
    return YT_OK;
}

/* String predicates, after setup_chunk: for every predicate read back its
 * column's parsed segments (the KEPT ones — input_row_limit truncates the
 * list), lay the per-segment bitmaps out on 64-bit word boundaries, run the
 * entry pass on the run's stream and hand bitmap + bases to the plan. The
 * buffers live in sp until the run ends. */
static int setup_string_preds(StrPreds* sp, DeviceRun* R, DevPlan* dp,
                              char* errbuf, size_t errlen)
{
    PoolScope ps;                   /* the two timing events */
    uint64_t entries = 0;
    const bool timing = getenv("YTQL_TIMING") != nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    t_last_strpred_entries = 0;
    t_last_inlist_mode = 0;
    dp->sp_count = sp->count;
    /* numeric IN sets: one open-addressing table each (inlist.h) */
    for (int i = 0; i < sp->in_count && R->nsegs != 0; i++) {
        std::vector<uint64_t>& tab = sp->h_intab[i];
        inlist_build_u64(sp->in[i].sorted, &tab, &dp->in_mask[i], &dp->in_empty[i]);
        uint64_t* d_tab = nullptr;
        HIP_CHECK(sp->ps.dev(&d_tab, sizeof(uint64_t) * tab.size()));
        HIP_CHECK(hipMemcpyAsync(d_tab, tab.data(), sizeof(uint64_t) * tab.size(),
                                 hipMemcpyHostToDevice, R->stream));
        dp->in_tab[i] = d_tab;
    }
    if (sp->count == 0 || R->nsegs == 0) return YT_OK;
    if (timing) {
        HIP_CHECK(ps.event(&e0));
        HIP_CHECK(ps.event(&e1));
        HIP_CHECK(hipEventRecord(e0, R->stream));
    }
    for (int i = 0; i < sp->count; i++) {
        const StrPredDesc& d = sp->d[i];
        const int off = R->h_off[d.col], cnt = R->h_cnt[d.col];
        if (cnt == 0) continue;
        std::vector<SegEx> ex(cnt);
        HIP_CHECK(hipMemcpy(ex.data(), R->d_segex + off, sizeof(SegEx) * cnt,
                            hipMemcpyDeviceToHost));
        std::vector<int64_t>& base = sp->h_base[i];
        base.resize(cnt + 1);
        int64_t words = 0;
        for (int sg = 0; sg < cnt; sg++) {
            if (!(ex[sg].flags & (8 | 32 | 64))) {
                set_err(errbuf, errlen,
                        "string predicate: unknown string segment layout");
                return YT_ERR_UNSUPPORTED;
            }
            base[sg] = words;
            words += ((int64_t)ex[sg].dict_size + 63) / 64;
            entries += ex[sg].dict_size;
        }
        base[cnt] = words;
        int64_t* d_base = nullptr;
        uint64_t* d_bits = nullptr;
        char* d_lit = nullptr;
        HIP_CHECK(sp->ps.dev(&d_base, sizeof(int64_t) * (cnt + 1)));
        HIP_CHECK(sp->ps.dev(&d_bits, sizeof(uint64_t) * (words ? words : 1)));
        HIP_CHECK(hipMemcpyAsync(d_base, base.data(), sizeof(int64_t) * (cnt + 1),
                                 hipMemcpyHostToDevice, R->stream));
        if (d.op == YT_EX_IN) {
            /* the list's slot table and bytes, then the IN entry kernel */
            const InStrList& il = sp->il[i];
            InStrSlot* d_slots = nullptr;
            char* d_bytes = nullptr;
            const size_t nb = il.bytes.size();
            HIP_CHECK(sp->ps.dev(&d_slots, sizeof(InStrSlot) * il.slots.size()));
            HIP_CHECK(sp->ps.dev(&d_bytes, nb ? nb : 1));
            HIP_CHECK(hipMemcpyAsync(d_slots, il.slots.data(),
                                     sizeof(InStrSlot) * il.slots.size(),
                                     hipMemcpyHostToDevice, R->stream));
            if (nb)
                HIP_CHECK(hipMemcpyAsync(d_bytes, il.bytes.data(), nb,
                                         hipMemcpyHostToDevice, R->stream));
            const int use_lds = il.slots.size() <= kInStrLdsSlots;
            if (words) {
                HIP_CHECK(ytql_launch_inlist_str_entries(
                    R->d_segs, R->d_segex, off, cnt, d_base, words, d_slots,
                    il.mask, d_bytes, use_lds, d_bits, R->stream));
                if (!use_lds) t_last_inlist_mode = 2;
                else if (t_last_inlist_mode == 0) t_last_inlist_mode = 1;
            }
            dp->sp_bits[i] = d_bits;
            dp->sp_base[i] = d_base;
            continue;
        }
        HIP_CHECK(sp->ps.dev(&d_lit, (size_t)(d.lit_len ? d.lit_len : 1)));
        if (d.lit_len)
            HIP_CHECK(hipMemcpyAsync(d_lit, d.lit, (size_t)d.lit_len,
                                     hipMemcpyHostToDevice, R->stream));
        if (words)
            HIP_CHECK(ytql_launch_strpred_entries(R->d_segs, R->d_segex, off, cnt,
                                                  d_base, words, d.op, d.escape,
                                                  d_lit, d.lit_len, d_bits,
                                                  R->stream));
        dp->sp_bits[i] = d_bits;
        dp->sp_base[i] = d_base;
    }
    t_last_strpred_entries = entries;
    if (timing) {
        float ms = 0;
        HIP_CHECK(hipEventRecord(e1, R->stream));
        HIP_CHECK(hipEventSynchronize(e1));
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        fprintf(stderr, "[ytql timing] string predicates: %d, %llu entries, "
                        "entry pass %.3fms\n",
                sp->count, (unsigned long long)entries, ms);
    }
    return YT_OK;
}

static int setup_table(DeviceRun* R, int agg_count, int64_t max_groups,
                       int64_t group_limit, char* errbuf, size_t errlen)
{
    R->nslots = next_pow2((uint64_t)(max_groups > 0 ? max_groups : (1 << 20)) * 2);
    if (R->nslots < 2048) R->nslots = 2048;
    HIP_CHECK(R->ps.dev(&R->d_th, sizeof(TableHdr)));
    TableHdr hh;
    memset(&hh, 0, sizeof(hh));
    hh.nslots = R->nslots;
    hh.mask = R->nslots - 1;
    hh.group_limit = group_limit;
    HIP_CHECK(hipMemcpyAsync(R->d_th, &hh, sizeof(hh), hipMemcpyHostToDevice, R->stream));
    return YT_OK;
}

/* the direct-table slot array is only needed on the non-partitioned paths */
static int ensure_slots(DeviceRun* R, int agg_count, char* errbuf, size_t errlen)
{
    if (R->d_slots) return YT_OK;
    int stride = 2 + 2 * agg_count;
    HIP_CHECK(R->ps.dev(&R->d_slots, sizeof(uint64_t) * R->nslots * stride));
    HIP_CHECK(hipMemsetAsync(R->d_slots, 0, sizeof(uint64_t) * R->nslots * stride, R->stream));
    return YT_OK;
}

/* Two-phase partitioned group-by for the {1 direct int64 key, <=1 direct
 * sum, sum(1), optional range filter} family. On success sets *done and
 * leaves COMPACTED groups in R->d_groups (+ counter in R->d_counter);
 * sets *done=false (no error) when a capacity guard tripped so the caller
 * falls back to the direct-table kernel. */
static int run_partitioned(const YtPlan* plan, const YtChunk* chunk,
                           const YtExecOptions* options, DeviceRun* R,
                           const FastShape* fs, unsigned maxw,
                           YtStatistics* stats, bool* done,
                           int force_hash, bool* tried_direct,
                           char* errbuf, size_t errlen)
{
    int rc = YT_OK;
    *done = false;
    PoolScope ps;                   /* the events; the blocks are R's */
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    uint32_t path = YT_SCAN_PATH_PARTITIONED
                  | (force_hash ? YT_SCAN_PATH_HASH_RETRY : 0);

    PartParams pp;
    memset(&pp, 0, sizeof(pp));
    /* canonical slots: 0 = filter, 1 = key, 2 = value (see kernel comment) */
    int used[3];
    used[0] = fs->filter_col >= 0 ? fs->filter_col : fs->key_col;
    used[1] = fs->key_col;
    used[2] = fs->nsum == 1 ? fs->sum_col[0] : fs->key_col;
    int nused = 3;
    pp.filter_idx = fs->filter_col >= 0 ? 0 : -1;
    pp.key_idx = 1;
    pp.val_idx = fs->nsum == 1 ? 2 : -1;
    pp.nused = nused;
    pp.sum_slot = fs->nsum == 1 ? fs->sum_slot[0] : -1;
    pp.agg_count = plan->agg_count;
    pp.filter_lo = fs->filter_lo;
    pp.filter_hi = fs->filter_hi;
    pp.has_key_nulls = (R->col_null_flags[fs->key_col] != 0);
    pp.has_val_nulls = pp.val_idx >= 0 && (R->col_null_flags[fs->sum_col[0]] != 0);
    pp.has_filter_nulls = pp.filter_idx >= 0 && (R->col_null_flags[fs->filter_col] != 0);

    /* 8-byte packed records when the combined zigzag spans fit 64 bits */
    {
        auto bits_of = [](uint64_t span) -> int {
            int b = 0;
            while (span) { b++; span >>= 1; }
            return b;
        };
        auto exact_range = [&](int col) -> int {
            /* refine the meta-only span (rounded up to min+2^w-1 per
             * segment) by an exact device scan of the column */
            uint64_t* d_ex = nullptr;
            int rc2 = ps.dev(&d_ex, 2 * sizeof(uint64_t));
            if (rc2 != YT_OK) return rc2;
            uint64_t init[2] = { ~0ULL, 0 };
            hipError_t e;
            if ((e = hipMemcpyAsync(d_ex, init, sizeof(init),
                                    hipMemcpyHostToDevice, R->stream)) ||
                (e = ytql_launch_scan_zzrange(R->d_segs, R->d_segex,
                                              R->h_off[col], R->h_cnt[col],
                                              R->col_null_flags[col] != 0,
                                              (unsigned long long*)d_ex, R->stream)) ||
                (e = hipMemcpyAsync(init, d_ex, sizeof(init),
                                    hipMemcpyDeviceToHost, R->stream)) ||
                (e = hipStreamSynchronize(R->stream))) {
                ps.release(d_ex);
                set_err(errbuf, errlen, hipGetErrorString(e));
                return YT_ERR_HIP;
            }
            ps.release(d_ex);
            if (init[0] <= init[1]) {   /* any non-null value seen */
                R->col_zzmin[col] = init[0];
                R->col_zzmax[col] = init[1];
            }
            return YT_OK;
        };
        uint64_t span_k = R->col_zzmax[fs->key_col] - R->col_zzmin[fs->key_col];
        int bk = bits_of(span_k);
        int bv = 0;
        uint64_t gmin_v = 0;
        if (pp.val_idx >= 0) {
            uint64_t span_v = R->col_zzmax[fs->sum_col[0]] - R->col_zzmin[fs->sum_col[0]];
            bv = bits_of(span_v);
            gmin_v = R->col_zzmin[fs->sum_col[0]];
        }
        /* the meta bound overstates each span by at most one bit; scan
         * exactly when that one bit could enable direct-span mode or the
         * spare bit 63 it needs (cheap: one streaming read of the column) */
        if ((bk >= 1 && bk <= 23) && !(bk <= 22 && bk + bv <= 63)) {
            rc = exact_range(fs->key_col);
            if (rc != YT_OK) return rc;
            path |= YT_SCAN_PATH_KEY_EXACT;
            span_k = R->col_zzmax[fs->key_col] - R->col_zzmin[fs->key_col];
            bk = bits_of(span_k);
        }
        if (pp.val_idx >= 0 && bk + bv >= 64 && bk + bv <= 65) {
            rc = exact_range(fs->sum_col[0]);
            if (rc != YT_OK) return rc;
            path |= YT_SCAN_PATH_VAL_EXACT;
            uint64_t span_v = R->col_zzmax[fs->sum_col[0]] - R->col_zzmin[fs->sum_col[0]];
            bv = bits_of(span_v);
            gmin_v = R->col_zzmin[fs->sum_col[0]];
        }
        /* a 64-bit key span beside a sum (bv is 0 then: one constant value)
         * would make bits_k 64, and the kernels shift the value by bits_k —
         * no valid shift count; such a plan keeps 16-byte records */
        if (bk + bv <= 64 && !(bk == 64 && pp.val_idx >= 0)) {
            pp.packed_mode = 1;
            pp.bits_k = bk ? bk : 1;
            /* only bk == 0 with bv == 64 gets here (one distinct key, full-
             * range values): the key then takes no record bits at all */
            if (pp.bits_k + bv > 64) pp.bits_k = bk;
            pp.gmin_k = R->col_zzmin[fs->key_col];
            pp.gmin_v = gmin_v;
        }
        /* direct-span mode asks for bit 63 of a packed record to be spare
         * (bk + bv <= 63; 16-byte records always qualify). The padded claims
         * that used the bit are gone and nothing sets it any more; the
         * condition stays only so that the mode lattice, which
         * tests/test_partition_modes.py pins, does not move */
        int spare_bit = (!pp.packed_mode || pp.bits_k + bv <= 63) ? 1 : 0;
        /* direct-span mode: when the key zigzag span is small, partition by
         * key RANGE and index phase B's per-bucket array directly (the
         * headline config — 1M distinct keys — spans 21 bits). */
        pp.gmin_k = R->col_zzmin[fs->key_col];
        if (bk <= 22 && spare_bit && !force_hash && !getenv("YTQL_NO_DIRECT")) {
            pp.direct_mode = 1;
            pp.dshift = bk > 10 ? bk - 10 : 0;
            if (tried_direct) *tried_direct = true;
        }
        /* the plain decode (common.h PartParams::plain_mode). The column's
         * zigzag maximum, from the headers or exact, bounds every row: below
         * UINT64_MAX no key is INT64_MIN. The headers' own range is
         * min(min_value) .. max(min_value + 2^w - 1) over the key's
         * segments, saturated at UINT64_MAX: unsaturated and narrower than
         * 2^32 it holds every segment's width w to 32 bits. A saturated
         * header range therefore keeps the general decode even where an
         * exact scan found a lower maximum: the widths are unknown then.
         * (Direct mode itself needs a header span of at most 23 bits, the
         * widest the exact key scan runs for, so no segment wider than 23
         * bits gets here today; the 32 is the kernel's own limit.) */
        if (pp.packed_mode && pp.direct_mode && pp.filter_idx < 0 && pp.val_idx >= 0 &&
            !pp.has_key_nulls && !pp.has_val_nulls && R->h_setup &&
            R->col_zzmax[fs->key_col] != UINT64_MAX) {
            const uint64_t hlo = R->h_setup->zzmin[fs->key_col];
            const uint64_t hhi = R->h_setup->zzmax[fs->key_col];
            if (hhi != UINT64_MAX && hhi >= hlo && hhi - hlo < (1ULL << 32))
                pp.plain_mode = 1;
        }
        if (pp.direct_mode) path |= YT_SCAN_PATH_DIRECT;
        if (pp.packed_mode) path |= YT_SCAN_PATH_PACKED;
        if (pp.has_val_nulls) path |= YT_SCAN_PATH_NULL_STREAM;
        /* a hash retry keeps what the direct-span attempt recorded */
        t_last_scan_path = (force_hash ? t_last_scan_path : 0) | path;
    }

    int64_t rows = chunk->row_count;
    if (options->input_row_limit > 0 && options->input_row_limit < rows)
        rows = options->input_row_limit;

    const int nsub = 8;
    /* per (bucket, XCD) sub-streams: 8x more cursors, 1/8 the rows each */
    pp.bucket_stride = rows / (kNB * 8) + (rows / (kNB * 8)) / 2 + 4096;
    pp.bucket_stride = (pp.bucket_stride + 7) & ~(int64_t)7;
    pp.nbucket_stride = pp.has_val_nulls ? pp.bucket_stride : 0;

    /* a region holds one whole tile whatever the key skew (common.h); a
     * segment takes as many tiles as its longest sibling needs, and the
     * kernel masks the rows, or whole tiles, past its end */
    const int tile_rows = (pp.packed_mode && pp.bucket_stride >= kPartTileMax)
        ? kPartTileMax : kPartTileMin;
    pp.tile_rows = tile_rows;
    const int nseg = R->h_cnt[fs->key_col];
    int32_t max_seg_rows = 1;
    for (int s = 0; s < nseg; s++)
        max_seg_rows = std::max(max_seg_rows, R->h_segs[R->h_off[fs->key_col] + s].row_count);
    pp.tiles_per_seg = (max_seg_rows + tile_rows - 1) / tile_rows;
    {
        int32_t last_rows = R->h_segs[R->h_off[fs->key_col] + nseg - 1].row_count;
        pp.ntiles = (nseg - 1) * pp.tiles_per_seg + (last_rows + tile_rows - 1) / tile_rows;
    }
    /* two workgroups fit a CU; a grid of 512, 1024 or 2048 measured alike
     * (YTQL_GRID: sweeps only) */
    int grid = pp.ntiles < 2048 ? (pp.ntiles ? pp.ntiles : 1) : 2048;
    {
        const char* gv = getenv("YTQL_GRID");   /* perf experiments only */
        if (gv && atoi(gv) >= 8 && atoi(gv) < grid) grid = atoi(gv) & ~7;
        if (grid < 1) grid = 1;
    }

    std::vector<FastCol> fc(nused);
    for (int u = 0; u < nused; u++) {
        fc[u].seg_off = R->h_off[used[u]];
        fc[u].seg_cnt = R->h_cnt[used[u]];
    }

    HIP_CHECK(R->ps.dev(&R->d_fastcols, sizeof(FastCol) * nused));
    HIP_CHECK(hipMemcpyAsync(R->d_fastcols, fc.data(), sizeof(FastCol) * nused,
                             hipMemcpyHostToDevice, R->stream));
    HIP_CHECK(R->ps.dev(&R->d_cursors, sizeof(uint64_t) * kNB * nsub));
    HIP_CHECK(hipMemsetAsync(R->d_cursors, 0, sizeof(uint64_t) * kNB * nsub, R->stream));
    HIP_CHECK(R->ps.dev(&R->d_recs,
                         (size_t)kNB * nsub * pp.bucket_stride * (pp.packed_mode ? 8 : 16)));
    if (pp.has_val_nulls) {
        HIP_CHECK(R->ps.dev(&R->d_ncursors, sizeof(uint64_t) * kNB * 8));
        HIP_CHECK(hipMemsetAsync(R->d_ncursors, 0, sizeof(uint64_t) * kNB * 8, R->stream));
        HIP_CHECK(R->ps.dev(&R->d_nrecs, (size_t)kNB * 8 * pp.nbucket_stride * 8));
    }
    /* the partitioned path's in-table sentinel is INT64_MIN bits */
    uint64_t sk = kEmptyKey;
    HIP_CHECK(hipMemcpyAsync((char*)R->d_th + offsetof(TableHdr, side_key_bits),
                             &sk, 8, hipMemcpyHostToDevice, R->stream));

    int64_t cap_groups = (int64_t)kNB * kHSlots;
    if (options->max_groups_hint > 0) {
        int64_t want = options->max_groups_hint * 2 + 4096;
        if (want < cap_groups) cap_groups = want;
    }
    if (cap_groups > rows + 16) cap_groups = rows + 16;
    R->groups_capacity = cap_groups;
    const int slim = R->want_slim ? 1 : 0;
    HIP_CHECK(R->ps.dev(&R->d_groups,
                         (slim ? sizeof(SlimGroup) : sizeof(OutGroup)) * cap_groups));
    if (!R->h_th) HIP_CHECK(R->ps.host(&R->h_th, sizeof(TableHdr)));
    R->th_valid = false;
    HIP_CHECK(R->ps.dev(&R->d_counter, sizeof(unsigned long long)));
    HIP_CHECK(hipMemsetAsync(R->d_counter, 0, sizeof(unsigned long long), R->stream));

    HIP_CHECK(ps.event(&ev0));
    HIP_CHECK(ps.event(&ev1));
    HIP_CHECK(ps.event(&ev2));
    HIP_CHECK(hipEventRecord(ev0, R->stream));
    HIP_CHECK(ytql_launch_scan_partition(&pp, R->d_segs, R->d_segex, R->d_fastcols,
                                         R->d_th, R->d_cursors, R->d_recs,
                                         R->d_ncursors, R->d_nrecs,
                                         grid, R->stream));
    g_last_part_variant.store((pp.packed_mode ? kPartVariantPacked : 0) |
                              (pp.plain_mode ? kPartVariantPlain : 0),
                              std::memory_order_relaxed);
    HIP_CHECK(hipEventRecord(ev1, R->stream));
    if (pp.direct_mode) {
        HIP_CHECK(ytql_launch_bucket_agg_direct(R->d_recs, R->d_cursors, pp.bucket_stride,
                                         R->d_nrecs, R->d_ncursors, pp.nbucket_stride,
                                         R->d_groups, R->d_counter, cap_groups, slim,
                                         R->d_th, pp.sum_slot, pp.agg_count,
                                         pp.packed_mode, pp.bits_k,
                                         pp.gmin_k, pp.gmin_v, pp.dshift, nsub, R->stream));
    } else {
        HIP_CHECK(ytql_launch_bucket_agg(R->d_recs, R->d_cursors, pp.bucket_stride,
                                         R->d_nrecs, R->d_ncursors, pp.nbucket_stride,
                                         R->d_groups, R->d_counter, cap_groups, slim,
                                         R->d_th, pp.sum_slot, pp.agg_count,
                                         pp.packed_mode, pp.bits_k,
                                         pp.gmin_k, pp.gmin_v, nsub, R->stream));
    }
    HIP_CHECK(hipEventRecord(ev2, R->stream));
    /* the header rides the synchronisation that the events need anyway */
    HIP_CHECK(hipMemcpyAsync(R->h_th, R->d_th, sizeof(TableHdr),
                             hipMemcpyDeviceToHost, R->stream));
    HIP_CHECK(hipStreamSynchronize(R->stream));
    float msA = 0, msB = 0;
    HIP_CHECK(hipEventElapsedTime(&msA, ev0, ev1));
    HIP_CHECK(hipEventElapsedTime(&msB, ev1, ev2));
    if (stats) {
        stats->kernel_scan_ms += msA;
        stats->kernel_scan_launches += 1;
        stats->kernel_other_ms += msB;
    }
    /* overflow==1 → capacity guard; retry on the direct path */
    if (R->h_th->overflow == 1) {
        /* reset and fall back */
        R->ps.release(R->d_groups); R->d_groups = nullptr;
        R->ps.release(R->d_counter); R->d_counter = nullptr;
        R->ps.release(R->d_recs); R->d_recs = nullptr;
        R->ps.release(R->d_cursors); R->d_cursors = nullptr;
        R->ps.release(R->d_nrecs); R->d_nrecs = nullptr;
        R->ps.release(R->d_ncursors); R->d_ncursors = nullptr;
        R->ps.release(R->d_fastcols); R->d_fastcols = nullptr;
        TableHdr hh;
        memset(&hh, 0, sizeof(hh));
        hh.nslots = R->nslots;
        hh.mask = R->nslots - 1;
        hh.group_limit = options->group_row_limit;
        HIP_CHECK(hipMemcpyAsync(R->d_th, &hh, sizeof(hh), hipMemcpyHostToDevice, R->stream));
        *done = false;
    } else {
        R->groups_compacted = true;
        R->groups_slim = slim != 0;
        R->th_valid = true;
        *done = true;
    }
    return YT_OK;
}

/* run the scan (fast when possible), leaving results in the table/gaccum.
 * Fills stats->kernel_scan_* from device events. */
static int run_scan(const YtPlan* plan, const YtChunk* chunk,
                    const YtExecOptions* options, DeviceRun* R,
                    const DevPlan* dp, const JoinDev* jd,
                    const JoinDev* jd2,
                    const FastShape* fs, unsigned maxw,
                    YtStatistics* stats, char* errbuf, size_t errlen)
{
    int rc = YT_OK;
    PoolScope ps;                   /* the events; the blocks are R's */
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool partitioned = false;

    if ((fs->valid || fs->ragged) && fs->key_col >= 0 && fs->nsum <= 1) {
        bool done = false;
        partitioned = true;
        bool tried_direct = false;
        rc = run_partitioned(plan, chunk, options, R, fs, maxw, stats, &done,
                             0, &tried_direct, errbuf, errlen);
        if (rc != YT_OK) return rc;
        /* direct-span mode overflows on range-clustered key skew; the
         * hash-partitioned layout spreads those — retry before giving up */
        if (!done && tried_direct) {
            rc = run_partitioned(plan, chunk, options, R, fs, maxw, stats, &done,
                                 1, nullptr, errbuf, errlen);
            if (rc != YT_OK) return rc;
        }
        if (done) return YT_OK;
        /* else: capacity guard tripped — fall through to the direct path */
    }

    t_last_scan_path = (partitioned ? t_last_scan_path : 0)
        | (fs->valid ? YT_SCAN_PATH_FAST : YT_SCAN_PATH_GENERIC);
    for (int i = 0; dp && i < dp->kp_count; i++)
        if (kp_is_str(dp, i)) t_last_scan_path |= YT_SCAN_PATH_STR_IDS;

    rc = ensure_slots(R, plan->agg_count, errbuf, errlen);
    if (rc != YT_OK) return rc;

    HIP_CHECK(ps.event(&ev0));
    HIP_CHECK(ps.event(&ev1));

    HIP_CHECK(R->ps.dev(&R->d_gaccum, sizeof(uint64_t) * (1 + 2 * kMaxAggs)));
    HIP_CHECK(hipMemsetAsync(R->d_gaccum, 0, sizeof(uint64_t) * (1 + 2 * kMaxAggs), R->stream));

    if (fs->valid) {
        /* fast fused kernel — canonical slots: 0 = filter, 1..4 = sum args,
         * 5 = key (see k_scan_fast) */
        FastParams fp;
        memset(&fp, 0, sizeof(fp));
        int used[6];
        used[0] = fs->filter_col >= 0 ? fs->filter_col : 0;
        for (int a = 0; a < kMaxAggs; a++) {
            used[1 + a] = (a < fs->nsum) ? fs->sum_col[a] : 0;
        }
        used[5] = fs->key_col >= 0 ? fs->key_col : 0;
        int nused = 6;
        fp.filter_idx = fs->filter_col >= 0 ? 0 : -1;
        fp.key_idx = fs->key_col >= 0 ? 5 : -1;
        fp.nsum = fs->nsum;
        for (int a = 0; a < fs->nsum; a++) {
            fp.sum_idx[a] = 1 + a;
            fp.sum_slot[a] = fs->sum_slot[a];
        }
        fp.nused = nused;
        fp.agg_count = plan->agg_count;
        fp.filter_lo = fs->filter_lo;
        fp.filter_hi = fs->filter_hi;
        fp.row_count = chunk->row_count;
        fp.nsegs_per_col = chunk->columns[0].segment_count;
        fp.stage_bm_mask = 0;
        if (fs->filter_col >= 0 && R->col_null_flags[fs->filter_col]) fp.stage_bm_mask |= 1;
        for (int a = 0; a < fs->nsum; a++) {
            if (R->col_null_flags[fs->sum_col[a]]) fp.stage_bm_mask |= 1 << (1 + a);
        }
        if (fs->key_col >= 0 && R->col_null_flags[fs->key_col]) fp.stage_bm_mask |= 1 << 5;

        int32_t seg0_rows = R->h_segs[R->h_off[used[1]]].row_count;

        /* no LDS staging: tile size only shapes the grid */
        size_t lds = 0;
        int tile_rows = 8192;
        if (tile_rows > seg0_rows) {
            while (tile_rows > 256 && tile_rows > seg0_rows) tile_rows >>= 1;
        }
        fp.tile_rows = tile_rows;
        fp.tiles_per_seg = (seg0_rows + tile_rows - 1) / tile_rows;
        {
            int nseg = R->h_cnt[used[1]];
            int32_t last_rows = R->h_segs[R->h_off[used[1]] + nseg - 1].row_count;
            fp.ntiles = (nseg - 1) * fp.tiles_per_seg + (last_rows + tile_rows - 1) / tile_rows;
        }

        std::vector<FastCol> fc(nused);
        for (int u = 0; u < nused; u++) {
            fc[u].seg_off = R->h_off[used[u]];
            fc[u].seg_cnt = R->h_cnt[used[u]];
        }
        HIP_CHECK(R->ps.dev(&R->d_fastcols, sizeof(FastCol) * nused));
        HIP_CHECK(hipMemcpyAsync(R->d_fastcols, fc.data(), sizeof(FastCol) * nused,
                                 hipMemcpyHostToDevice, R->stream));

        int grid = fp.ntiles < 2048 ? (fp.ntiles ? fp.ntiles : 1) : 2048;
        HIP_CHECK(hipEventRecord(ev0, R->stream));
        HIP_CHECK(ytql_launch_scan_fast(&fp, R->d_segs, R->d_segex, R->d_fastcols,
                                        R->d_th, R->d_slots, R->d_gaccum,
                                        lds, grid, R->stream));
        HIP_CHECK(hipEventRecord(ev1, R->stream));
    } else {
        HIP_CHECK(hipEventRecord(ev0, R->stream));
        int64_t gen_rows = chunk->row_count;
        if (options->input_row_limit > 0 && options->input_row_limit < gen_rows)
            gen_rows = options->input_row_limit;
        HIP_CHECK(ytql_launch_scan_generic(dp, R->d_segs, R->d_segex, R->d_off, R->d_cnt,
                                           gen_rows, jd, jd2, R->d_th, R->d_slots,
                                           R->d_err, &R->strkeys, R->stream));
        HIP_CHECK(hipEventRecord(ev1, R->stream));
    }
    HIP_CHECK(hipStreamSynchronize(R->stream));
    {
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
        if (stats) {
            stats->kernel_scan_ms += ms;
            stats->kernel_scan_launches += 1;
        }
    }
    if (!fs->valid) {
        unsigned kerr = 0;
        HIP_CHECK(hipMemcpy(&kerr, R->d_err, sizeof(unsigned), hipMemcpyDeviceToHost));
        if (kerr) {
            set_err(errbuf, errlen, kerr == YT_ERR_DIV_ZERO ? "Division by zero" : "expression error");
            return (int)kerr;
        }
    }
    return YT_OK;
}

static inline int64_t h_zz_dec(uint64_t z)
{
    return (int64_t)(z >> 1) ^ -(int64_t)(z & 1);
}

/* resolve composite-key packing widths from the parsed per-column
 * zigzag-space ranges (k_parse_segments min/max atomics) */
static int pack_group_key(DevPlan* dp, const DeviceRun* R,
                          char* errbuf, size_t errlen,
                          const StrKeyTab* strtabs = nullptr)
{
    int shift = 0;
    for (int i = 0; i < dp->kp_count; i++) {
        int c = dp->kp_col[i];
        uint64_t lo = R->col_zzmin[c], hi = R->col_zzmax[c];
        uint64_t span = hi >= lo ? hi - lo : 0;
        if (kp_is_str(dp, i)) {
            /* string ids 0..D-1 (setup_strkey_ids): codes 0 (null) .. D */
            const uint64_t D = strtabs ? strtabs[i].ids.size() : 0;
            lo = 0;
            span = D ? D - 1 : 0;
        }
        /* codes are 0 (null) .. span+1: smallest bits with span+1 < 2^bits */
        int bits = 1;
        while (bits < 64 && ((span + 1) >> bits) != 0) bits++;
        dp->kp_base[i] = lo;
        dp->kp_bits[i] = bits;
        dp->kp_shift[i] = shift;
        shift += bits;
    }
    if (shift > 62) {
        set_err(errbuf, errlen,
                "multi-key GROUP BY: composite key wider than 62 bits this round");
        return YT_ERR_UNSUPPORTED;
    }
    return YT_OK;
}

/* finalize a group (OutGroup record or side accumulator) into HVal row
 * [keys..., aggs...] */
static void finalize_row(const YtPlan* plan, uint8_t key_type,
                         uint8_t sum_type[kMaxAggs],
                         uint64_t key_bits, int key_null, uint64_t cnt,
                         const uint64_t* agg_bits, const uint64_t* agg_nonnull,
                         HVal* row, int* nrow, int has_key)
{
    int n = 0;
    if (has_key) {
        row[n].type = key_null ? YT_VT_NULL : key_type;
        row[n].bits = key_null ? 0 : key_bits;
        n++;
    }
    for (int a = 0; a < plan->agg_count; a++) {
        if (plan->aggs[a]->func == YT_AGG_SUM1) {
            row[n].type = YT_VT_INT64;
            row[n].bits = cnt;
        } else if (agg_nonnull[a] == 0) {
            row[n].type = YT_VT_NULL;
            row[n].bits = 0;
        } else if (plan->aggs[a]->func == YT_AGG_AVG) {
            /* finalize: double(sum)/count (profiler avg Finalize; count —
             * the nonnull word — is nonzero here) */
            double sum;
            if (sum_type[a] == YT_VT_DOUBLE) {
                memcpy(&sum, &agg_bits[a], 8);
            } else if (sum_type[a] == YT_VT_UINT64) {
                sum = (double)agg_bits[a];
            } else {
                sum = (double)(int64_t)agg_bits[a];
            }
            double r = sum / (double)agg_nonnull[a];
            row[n].type = YT_VT_DOUBLE;
            memcpy(&row[n].bits, &r, 8);
        } else {
            row[n].type = sum_type[a];
            uint64_t bits = agg_bits[a];
            int f = plan->aggs[a]->func;
            if (f == YT_AGG_MIN || f == YT_AGG_MAX) {
                /* undo the order-preserving map (kernels.hip ord_map):
                 * MIN stored ~m(x); then m inverse per type */
                uint64_t m = (f == YT_AGG_MIN) ? ~bits : bits;
                const uint64_t SIGN = 0x8000000000000000ULL;
                if (sum_type[a] == YT_VT_DOUBLE) {
                    bits = (m & SIGN) ? (m & ~SIGN) : ~m;
                } else if (sum_type[a] == YT_VT_INT64) {
                    bits = m ^ SIGN;
                } else {
                    bits = m;
                }
            }
            row[n].bits = bits;
        }
        n++;
    }
    *nrow = n;
}

/* SlimGroups on their way to the host: the copy was queued in `count` slices
 * of `per` groups each (the last one shorter), with an event after every
 * slice. A reader waits for the event of a slice before it touches it. */
constexpr int kGroupSlices = 8;
struct SlimSlices {
    hipEvent_t ev[kGroupSlices];
    int count;
    int64_t per;
};

/* `groups` holds OutGroups, or, when `slim` is given, is null and `slim`
 * holds the SlimGroups of the partitioned path; `slices` (slim only) is null
 * when the records have already landed. */
static int emit_rows(const YtPlan* plan, const YtChunk* chunk,
                     const DevPlan* dp,
                     const OutGroup* groups, int64_t ngroups,
                     const TableHdr& th, int has_any_row_global,
                     const uint64_t* gaccum, int used_fast_global,
                     int64_t output_row_limit, int* out_limited,
                     YtRowset* output, char* errbuf, size_t errlen,
                     const SlimGroup* slim = nullptr,
                     const SlimSlices* slices = nullptr,
                     const StrKeyTab* strtabs = nullptr)
{
    uint8_t col_types[kMaxCols];
    memset(col_types, YT_VT_INT64, sizeof(col_types));
    if (dp) {
        /* dp carries the EXTENDED column space (primary + joined foreign) */
        for (int c = 0; c < dp->ncols && c < kMaxCols; c++)
            col_types[c] = dp->col_types[c];
    } else {
        for (int c = 0; c < chunk->column_count && c < kMaxCols; c++)
            col_types[c] = (uint8_t)chunk->columns[c].value_type;
    }

    const int kp = dp ? dp->kp_count : 0;
    /* STRING components of the composite key: their bytes go to the rowset's
     * string pool as rows are emitted, one row after the other */
    bool kp_any_str = false;
    for (int i = 0; i < kp; i++) kp_any_str |= kp_is_str(dp, i);
    if (kp_any_str) {
        if (!strtabs) return YT_ERR_INVALID_PLAN;
        output->string_pool_used = 0;   /* rowsets reusable across queries */
    }
    uint8_t key_type = YT_VT_INT64;
    int has_key = plan->key_count == 1;
    if (has_key) key_type = expr_static_type(plan->keys[0], col_types);
    uint8_t sum_type[kMaxAggs];
    for (int a = 0; a < plan->agg_count; a++) {
        sum_type[a] = (plan->aggs[a]->func != YT_AGG_SUM1)
            ? expr_static_type(plan->aggs[a]->arg, col_types) : YT_VT_INT64;
        if (sum_type[a] == YT_VT_NULL) sum_type[a] = YT_VT_INT64;
    }

    int base_cols = (kp ? kp : (has_key ? 1 : 0)) + plan->agg_count;
    int out_cols = plan->project_count ? plan->project_count : base_cols;

    auto emit_at = [&](YtValue* dst, uint64_t key_bits, int key_null,
                       uint64_t cnt, const uint64_t* ab, const uint64_t* an) -> int {
        HVal row[kMaxPackKeys + 1 + kMaxAggs];
        uint32_t slen[kMaxPackKeys] = {0, 0, 0, 0};
        int nrow = 0;
        if (kp) {
            /* unpack the composite key (DevPlan kp_*; code 0 = null) */
            for (int i = 0; i < kp; i++) {
                uint64_t mask = dp->kp_bits[i] >= 64
                    ? ~0ULL : ((1ULL << dp->kp_bits[i]) - 1);
                uint64_t code = (key_bits >> dp->kp_shift[i]) & mask;
                if (code == 0) {
                    row[nrow].type = YT_VT_NULL;
                    row[nrow].bits = 0;
                } else if (kp_is_str(dp, i)) {
                    /* string id code-1: bits = where its bytes went */
                    const StrKeyTab& T = strtabs[i];
                    if (code - 1 >= T.ids.size()) return YT_ERR_HIP;
                    const uint64_t ol = T.ids[code - 1].off_len;
                    const uint32_t len = (uint32_t)(ol & 0xFFFFFF);
                    if (len && (!output->string_pool ||
                                (uint64_t)output->string_pool_used + len >
                                    (uint64_t)output->string_pool_capacity)) {
                        set_err(errbuf, errlen, "string pool too small");
                        return YT_ERR_CAPACITY;
                    }
                    char* kdst = output->string_pool
                        ? output->string_pool + output->string_pool_used : nullptr;
                    if (len) memcpy(kdst, T.pool.data() + (ol >> 24), len);
                    output->string_pool_used += len;
                    slen[i] = len;
                    row[nrow].type = YT_VT_STRING;
                    row[nrow].bits = (uint64_t)(uintptr_t)kdst;
                } else {
                    uint64_t z = code - 1 + dp->kp_base[i];
                    row[nrow].type = col_types[dp->kp_col[i]];
                    row[nrow].bits = dp->kp_signed[i]
                        ? (uint64_t)h_zz_dec(z) : z;
                }
                nrow++;
            }
            int an_ = 0;
            finalize_row(plan, key_type, sum_type, 0, 0, cnt, ab, an,
                         row + nrow, &an_, /*has_key=*/0);
            nrow += an_;
        } else
        finalize_row(plan, key_type, sum_type, key_bits, key_null, cnt, ab, an,
                     row, &nrow, has_key);
        if (plan->project_count) {
            for (int p = 0; p < plan->project_count; p++) {
                HVal v;
                int rc = heval(plan->projects[p], row, nrow, &v);
                if (rc) return rc;
                dst[p].id = (uint16_t)p;
                dst[p].type = v.type;
                dst[p].flags = 0;
                dst[p].length = 0;
                dst[p].data.bits = v.bits;
            }
        } else {
            for (int i = 0; i < nrow; i++) {
                dst[i].id = (uint16_t)i;
                dst[i].type = row[i].type;
                dst[i].flags = 0;
                dst[i].length = i < kp ? slen[i] : 0;
                dst[i].data.bits = row[i].bits;
            }
        }
        return YT_OK;
    };
    auto emit = [&](uint64_t key_bits, int key_null, uint64_t cnt,
                    const uint64_t* ab, const uint64_t* an) -> int {
        if (output_row_limit > 0 && output->row_count >= output_row_limit) {
            /* OutputRowLimit: soft stop — registry.cpp:297-305 WriteRow */
            if (out_limited) *out_limited = 1;
            return -1;
        }
        if (output->row_count >= output->capacity_rows) return YT_ERR_CAPACITY;
        int rc_ = emit_at(output->values + output->row_count * out_cols,
                          key_bits, key_null, cnt, ab, an);
        if (rc_ == YT_OK) output->row_count++;
        return rc_;
    };

    /* a SlimGroup row. Without projections the family's values are written
     * straight into the rowset: key, then per aggregate sum(1) = cnt or the
     * one sum (NULL when no argument was non-null) — what finalize_row
     * yields for them. Anything else goes the general way. */
    bool slim_direct = slim && !plan->project_count && !kp && has_key;
    for (int a = 0; a < plan->agg_count; a++) {
        int f = plan->aggs[a]->func;
        if (f != YT_AGG_SUM && f != YT_AGG_SUM1) slim_direct = false;
    }
    auto emit_slim_at = [&](YtValue* dst, const SlimGroup& g) -> int {
        if (!slim_direct) {
            uint64_t ab[kMaxAggs], an[kMaxAggs];
            for (int a = 0; a < kMaxAggs; a++) {
                ab[a] = g.sum_bits;
                an[a] = g.sum_nonnull;
            }
            return emit_at(dst, g.key_bits, 0, g.cnt, ab, an);
        }
        dst[0].id = 0;
        dst[0].type = key_type;
        dst[0].flags = 0;
        dst[0].length = 0;
        dst[0].data.bits = g.key_bits;
        for (int a = 0; a < plan->agg_count; a++) {
            YtValue& v = dst[1 + a];
            v.id = (uint16_t)(1 + a);
            v.flags = 0;
            v.length = 0;
            if (plan->aggs[a]->func == YT_AGG_SUM1) {
                v.type = YT_VT_INT64;
                v.data.bits = g.cnt;
            } else if (g.sum_nonnull == 0) {
                v.type = YT_VT_NULL;
                v.data.bits = 0;
            } else {
                v.type = sum_type[a];
                v.data.bits = g.sum_bits;
            }
        }
        return YT_OK;
    };

    output->row_count = 0;
    output->column_count = out_cols;
    int rc = YT_OK;

    if (!has_key && !kp) {
        /* global aggregate: one row iff any row passed the filter */
        uint64_t cnt;
        uint64_t ab[kMaxAggs] = {0}, an[kMaxAggs] = {0};
        if (used_fast_global) {
            cnt = gaccum[0];
            for (int a = 0; a < plan->agg_count; a++) {
                ab[a] = gaccum[1 + 2 * a];
                an[a] = gaccum[2 + 2 * a];
            }
            if (cnt == 0) return YT_OK;
        } else {
            /* generic path routed rows to synthetic key bits=1 */
            if (ngroups == 0) return YT_OK;
            cnt = groups[0].cnt;
            for (int a = 0; a < plan->agg_count; a++) {
                ab[a] = groups[0].agg_bits[a];
                an[a] = groups[0].agg_nonnull[a];
            }
        }
        (void)has_any_row_global;
        rc = emit(0, 0, cnt, ab, an);
        return rc == -1 ? YT_OK : rc;
    }

    {
        const int64_t total_sides = (int64_t)(th.side_used[0] != 0)
                                  + (int64_t)(th.side_used[1] != 0);
        const bool par_ok = ngroups >= 65536 && !kp_any_str
            && (output_row_limit <= 0 ||
                output_row_limit >= ngroups + total_sides)
            && ngroups + total_sides <= output->capacity_rows;
        if (par_ok) {
            /* row i is group i — emit in parallel (group order preserved;
             * the host loop was 5.5 ms of the 31 ms step at 1M groups) */
            std::atomic<int> arc{YT_OK};
            int nt = (int)std::min<int64_t>(std::thread::hardware_concurrency(),
                                            (ngroups + 131071) / 131072);
            if (nt > 32) nt = 32;
            if (nt < 1) nt = 1;
            ThreadJoiner tj;
            for (int t = 0; t < nt; t++) {
                tj.ths.emplace_back([&, t]() {
                    int64_t lo = ngroups * t / nt, hi = ngroups * (t + 1) / nt;
                    if (slim) {
                        /* slice by slice behind the copy: rows [lo, hi) */
                        const int64_t per = slices ? slices->per : ngroups;
                        for (int64_t a = lo; a < hi; ) {
                            const int64_t sl = a / per;
                            const int64_t b = std::min(hi, (sl + 1) * per);
                            if (slices &&
                                hipEventSynchronize(slices->ev[sl]) != hipSuccess) {
                                arc.store(YT_ERR_HIP);
                                return;
                            }
                            for (int64_t i = a; i < b; i++) {
                                int r2 = emit_slim_at(output->values + i * out_cols,
                                                      slim[i]);
                                if (r2 != YT_OK) { arc.store(r2); return; }
                            }
                            a = b;
                        }
                        return;
                    }
                    for (int64_t i = lo; i < hi; i++) {
                        const OutGroup& g = groups[i];
                        int r2 = emit_at(output->values + i * out_cols,
                                         g.key_bits, (int)(g.key_meta & 1),
                                         g.cnt, g.agg_bits, g.agg_nonnull);
                        if (r2 != YT_OK) { arc.store(r2); return; }
                    }
                });
            }
            tj.join();
            if (arc.load() != YT_OK) return arc.load();
            output->row_count = ngroups;
        } else if (slim) {
            /* serial: output_row_limit, few groups, or a rowset too short */
            if (slices && slices->count > 0 &&
                hipEventSynchronize(slices->ev[slices->count - 1]) != hipSuccess)
                return YT_ERR_HIP;
            for (int64_t i = 0; i < ngroups; i++) {
                if (output_row_limit > 0 && output->row_count >= output_row_limit) {
                    if (out_limited) *out_limited = 1;
                    return YT_OK;
                }
                if (output->row_count >= output->capacity_rows) return YT_ERR_CAPACITY;
                rc = emit_slim_at(output->values + output->row_count * out_cols,
                                  slim[i]);
                if (rc) return rc;
                output->row_count++;
            }
        } else {
            for (int64_t i = 0; i < ngroups; i++) {
                const OutGroup& g = groups[i];
                rc = emit(g.key_bits, (int)(g.key_meta & 1), g.cnt,
                          g.agg_bits, g.agg_nonnull);
                if (rc == -1) return YT_OK;
                if (rc) return rc;
            }
        }
    }
    /* side groups: the in-table sentinel key, then the null key */
    for (int side = 0; side < 2; side++) {
        if (!th.side_used[side]) continue;
        uint64_t ab[kMaxAggs], an[kMaxAggs];
        for (int a = 0; a < plan->agg_count; a++) {
            ab[a] = th.side_agg[side][2 * a];
            an[a] = th.side_agg[side][2 * a + 1];
        }
        rc = emit(th.side_key_bits[side], side == 1, th.side_cnt[side], ab, an);
        if (rc == -1) return YT_OK;
        if (rc) return rc;
    }
    (void)errbuf; (void)errlen;
    return rc;
}


/* ---- ORDER BY ... LIMIT ----
 * Comparer mirrors the reference codegen universal comparer
 * (cg_fragment_compiler.cpp:400-530): null < any, int64 signed,
 * uint64/boolean unsigned, double by value (NaN comparison = error), string
 * memcmp + length tiebreak; a descending key inverts the outcome. The
 * collector contract is TTopCollector's (top_collector-inl.h AddRow +
 * OrderOpHelper registry.cpp:1948-1997): keep the (offset+limit) least
 * rows, emit sorted ascending from offset. */
static int ord_cmp_vals(const YtPlan* plan, const YtValue* a, const YtValue* b,
                        int* nan_err)
{
    for (int i = 0; i < plan->order_count; i++) {
        int c = plan->order_cols[i];
        const YtValue* x = &a[c];
        const YtValue* y = &b[c];
        int xn = x->type == YT_VT_NULL, yn = y->type == YT_VT_NULL;
        int r = 0;
        if (xn || yn) {
            r = (xn == yn) ? 0 : (xn ? -1 : 1);
        } else if (x->type == YT_VT_DOUBLE) {
            double xv = x->data.dbl, yv = y->data.dbl;
            if (xv != xv || yv != yv) { *nan_err = 1; return 0; }
            r = xv < yv ? -1 : (xv > yv ? 1 : 0);
        } else if (x->type == YT_VT_STRING) {
            uint32_t lx = x->length, ly = y->length, m = lx < ly ? lx : ly;
            int mc = m ? memcmp(x->data.str, y->data.str, m) : 0;
            r = mc ? (mc < 0 ? -1 : 1) : (lx < ly ? -1 : (lx > ly ? 1 : 0));
        } else if (x->type == YT_VT_INT64) {
            r = x->data.i64 < y->data.i64 ? -1 : (x->data.i64 > y->data.i64 ? 1 : 0);
        } else {
            r = x->data.u64 < y->data.u64 ? -1 : (x->data.u64 > y->data.u64 ? 1 : 0);
        }
        if (plan->order_desc && plan->order_desc[i]) r = -r;
        if (r) return r;
    }
    return 0;
}

static int ord_validate_plan(const YtPlan* plan, int ncols, char* errbuf,
                             size_t errlen)
{
    if (plan->order_limit <= 0) {
        set_err(errbuf, errlen, "ORDER BY requires LIMIT");
        return YT_ERR_INVALID_PLAN;
    }
    for (int i = 0; i < plan->order_count; i++) {
        if (!plan->order_cols || plan->order_cols[i] < 0 ||
            plan->order_cols[i] >= ncols) {
            set_err(errbuf, errlen, "ORDER BY column out of range");
            return YT_ERR_INVALID_PLAN;
        }
    }
    return YT_OK;
}

/* sort the already-materialized rowset and keep [offset, offset+limit) —
 * used for grouped output, where the group count is already bounded */
static int apply_order_host(const YtPlan* plan, YtRowset* out,
                            char* errbuf, size_t errlen)
{
    int ncols = out->column_count;
    int rc = ord_validate_plan(plan, ncols, errbuf, errlen);
    if (rc != YT_OK) return rc;
    int64_t n = out->row_count;
    std::vector<const YtValue*> idx((size_t)n);
    for (int64_t i = 0; i < n; i++) idx[i] = out->values + i * ncols;
    int nan_err = 0;
    std::sort(idx.begin(), idx.end(),
              [&](const YtValue* a, const YtValue* b) {
                  return ord_cmp_vals(plan, a, b, &nan_err) < 0;
              });
    if (nan_err) {
        set_err(errbuf, errlen, "NaN in ORDER BY comparison");
        return YT_ERR_LIMIT;
    }
    int64_t b = plan->order_offset < n ? plan->order_offset : n;
    int64_t e = b + plan->order_limit;
    if (e > n) e = n;
    std::vector<YtValue> tmp((size_t)(e - b) * ncols);
    for (int64_t i = b; i < e; i++)
        memcpy(tmp.data() + (i - b) * ncols, idx[i], sizeof(YtValue) * ncols);
    memcpy(out->values, tmp.data(), sizeof(YtValue) * (e - b) * ncols);
    out->row_count = e - b;
    return YT_OK;
}

/* WITH TOTALS + ORDER BY finishing pass over a fully-materialized group
 * rowset: totals (null keys + aggregates over ALL grouped rows — the
 * reference's EStreamTag::Totals, registry.cpp FlushTotals) are computed
 * BEFORE the order/limit slice and appended after it, flagged in
 * YtRowset.totals_row. */
static int column_uniform_shift(const YtColumn& col)
{
    if (col.segment_count == 0) return 0;
    int32_t r0 = col.segments[0].row_count;
    if (r0 <= 0 || (r0 & (r0 - 1)) != 0) return 0;
    for (int i = 0; i + 1 < col.segment_count; i++)
        if (col.segments[i].row_count != r0) return 0;
    if (col.segments[col.segment_count - 1].row_count > r0) return 0;
    int shift = 0;
    while ((1 << (shift + 1)) <= r0) shift++;
    return (1 << shift) == r0 ? shift : 0;
}

/* equi-join runtime: parsed foreign chunk + unique-key hash table in HBM */
struct JoinRun {
    DeviceRun Rf;
    JoinDev jd;
    uint64_t* d_hkey = nullptr;
    long long* d_hrow = nullptr;
    unsigned long long* d_misc = nullptr;

    long long* d_chead = nullptr;
    long long* d_fnext = nullptr;

    JoinRun() { memset(&jd, 0, sizeof(jd)); }
};

/* one join item: the primary side is the row AS EXTENDED SO FAR
 * (row_types/row_ncols — primary columns plus earlier items' values, so a
 * later item can key on an earlier item's output). */
static int setup_join_item(const YtJoin* J, const uint8_t* row_types,
                           int row_ncols, int primary_ncols, JoinRun* JR,
                           hipStream_t stream, char* errbuf, size_t errlen)
{
    int rc = YT_OK;
    const YtChunk* fc = J->foreign;
    if (J->primary_key_col < 0 || J->primary_key_col >= row_ncols ||
        J->foreign_key_col < 0 || J->foreign_key_col >= fc->column_count) {
        set_err(errbuf, errlen, "join: key column out of range");
        return YT_ERR_INVALID_PLAN;
    }
    auto intish = [](int vt) {
        return vt == YT_VT_INT64 || vt == YT_VT_UINT64 || vt == YT_VT_BOOLEAN;
    };
    const int pvt = row_types[J->primary_key_col];
    const int fvt = fc->columns[J->foreign_key_col].value_type;
    const bool str_key = pvt == YT_VT_STRING && fvt == YT_VT_STRING;
    if ((pvt == YT_VT_STRING) != (fvt == YT_VT_STRING)) {
        set_err(errbuf, errlen, "join: key type mismatch");
        return YT_ERR_INVALID_PLAN;
    }
    if (!str_key && (!intish(pvt) || !intish(fvt))) {
        set_err(errbuf, errlen,
                "join: int64/uint64/boolean key columns this round");
        return YT_ERR_UNSUPPORTED;
    }
    /* a string key is looked up through the entries of a primary segment
     * (setup_strjoin_maps). An earlier item's appended value has none; string
     * foreign values are refused below, so no plan gets this far today, but
     * this is the bound that keeps the jmap lookup off foreign columns. */
    if (str_key && J->primary_key_col >= primary_ncols) {
        set_err(errbuf, errlen,
                "join: a string key must be a column of the primary chunk");
        return YT_ERR_UNSUPPORTED;
    }
    if (str_key && fc->row_count >= ((int64_t)1 << 31)) {
        set_err(errbuf, errlen,
                "join: string keys take foreign chunks below 2^31 rows");
        return YT_ERR_UNSUPPORTED;
    }
    for (int j = 0; j < J->foreign_value_count; j++) {
        int cjf = J->foreign_value_cols[j];
        if (cjf < 0 || cjf >= fc->column_count) {
            set_err(errbuf, errlen, "join: foreign value column out of range");
            return YT_ERR_INVALID_PLAN;
        }
        if (fc->columns[cjf].value_type == YT_VT_STRING) {
            set_err(errbuf, errlen, "join: string foreign values not this round");
            return YT_ERR_UNSUPPORTED;
        }
    }

    JR->Rf.stream = stream;
    unsigned mw = 0;
    int cl = 0;
    rc = setup_chunk(fc, &JR->Rf, &mw, 0, &cl, errbuf, errlen);
    if (rc) return rc;

    int64_t fn = fc->row_count;
    uint64_t cap = next_pow2((uint64_t)(fn ? fn : 1) * 2);
    if (cap < 2048) cap = 2048;
    JoinDev& jd = JR->jd;
    unsigned long long nr1 = 0;
    unsigned kerr = 0;
    HIP_CHECK(JR->Rf.ps.dev(&JR->d_hkey, sizeof(uint64_t) * cap));
    HIP_CHECK(JR->Rf.ps.dev(&JR->d_hrow, sizeof(long long) * cap));
    HIP_CHECK(JR->Rf.ps.dev(&JR->d_misc, sizeof(unsigned long long) * 3));
    HIP_CHECK(JR->Rf.ps.dev(&JR->d_chead, sizeof(long long) * cap));
    HIP_CHECK(JR->Rf.ps.dev(&JR->d_fnext, sizeof(long long) * (fn ? fn : 1)));
    HIP_CHECK(hipMemsetAsync(JR->d_hrow, 0xFF, sizeof(long long) * cap, stream));
    HIP_CHECK(hipMemsetAsync(JR->d_chead, 0xFF, sizeof(long long) * cap, stream));
    HIP_CHECK(hipMemsetAsync(JR->d_fnext, 0xFF, sizeof(long long) * (fn ? fn : 1), stream));
    HIP_CHECK(hipMemsetAsync(JR->d_misc, 0, sizeof(unsigned long long) * 3, stream));

    jd.active = 1;
    jd.is_left = J->is_left ? 1 : 0;
    jd.pkey_col = J->primary_key_col;
    jd.primary_ncols = row_ncols;
    jd.fkey_col = J->foreign_key_col;
    jd.fkey_shift = column_uniform_shift(fc->columns[J->foreign_key_col]);
    for (int j = 0; j < J->foreign_value_count; j++) {
        jd.fval_col[j] = J->foreign_value_cols[j];
        jd.f_shift[j] = column_uniform_shift(fc->columns[J->foreign_value_cols[j]]);
    }
    jd.fsegs = JR->Rf.d_segs;
    jd.fsegex = JR->Rf.d_segex;
    jd.f_off = JR->Rf.d_off;
    jd.f_cnt = JR->Rf.d_cnt;
    jd.hkey = JR->d_hkey;
    jd.hrow = (const int64_t*)JR->d_hrow;
    jd.hmask = cap - 1;
    jd.null_row = -1;
    jd.frows = fn;
    jd.chead = (const int64_t*)JR->d_chead;
    jd.fnext = (const int64_t*)JR->d_fnext;
    jd.has_dups = 0;
    jd.key_kind = str_key ? 1 : 0;
    jd.jmap = nullptr;
    jd.jbase = nullptr;

    if (str_key && fn > 0 && JR->Rf.nsegs > 0) {
        /* str_key_id answers "null" for a layout it does not know */
        const int off = JR->Rf.h_off[jd.fkey_col], cnt = JR->Rf.h_cnt[jd.fkey_col];
        std::vector<SegEx> ex(cnt);
        HIP_CHECK(hipMemcpy(ex.data(), JR->Rf.d_segex + off, sizeof(SegEx) * cnt,
                            hipMemcpyDeviceToHost));
        for (int sg = 0; sg < cnt; sg++)
            if (!(ex[sg].flags & (8 | 32 | 64))) {
                set_err(errbuf, errlen, "join: unknown string segment layout");
                return YT_ERR_UNSUPPORTED;
            }
        /* the string table (strjoin.h): same claim word, byte hashes in
         * hkey. The chain kernel does not read null_row, so the two launches
         * need no readback between them. */
        const bool timing = getenv("YTQL_TIMING") != nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (timing) {
            HIP_CHECK(JR->Rf.ps.event(&e0));
            HIP_CHECK(JR->Rf.ps.event(&e1));
            HIP_CHECK(hipEventRecord(e0, stream));
        }
        HIP_CHECK(hipMemsetAsync(JR->Rf.d_err, 0, sizeof(unsigned), stream));
        HIP_CHECK(ytql_launch_strjoin_build(&jd, fn, JR->d_hkey, JR->d_hrow,
                                            JR->d_misc, (unsigned*)(JR->d_misc + 1),
                                            JR->d_misc + 2, stream));
        HIP_CHECK(ytql_launch_strjoin_chain(&jd, fn, (unsigned*)(JR->d_misc + 1), stream));
        if (timing) HIP_CHECK(hipEventRecord(e1, stream));
        unsigned long long misc[3] = {0, 0, 0};
        HIP_CHECK(hipMemcpy(misc, JR->d_misc, sizeof(misc), hipMemcpyDeviceToHost));
        jd.null_row = misc[0] ? (int64_t)(misc[0] - 1) : -1;
        jd.has_dups = ((unsigned*)&misc[1])[1] != 0;
        t_last_strjoin_inserted += misc[2];
        if (timing) {
            float ms = 0;
            HIP_CHECK(hipEventSynchronize(e1));
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            fprintf(stderr, "[ytql timing] string join: %lld foreign rows, %llu "
                            "inserted, build %.3fms\n",
                    (long long)fn, misc[2], ms);
        }
    } else if (fn > 0 && JR->Rf.nsegs > 0) {
        /* d_err[0] = decode error, d_err[1] = has_dups flag (two words) */
        HIP_CHECK(hipMemsetAsync(JR->Rf.d_err, 0, sizeof(unsigned), stream));
        HIP_CHECK(hipMemsetAsync(JR->d_misc + 1, 0, sizeof(unsigned long long), stream));
        HIP_CHECK(ytql_launch_join_build(&jd, fn, JR->d_hkey, JR->d_hrow,
                                         JR->d_misc, (unsigned*)(JR->d_misc + 1), stream));
        HIP_CHECK(hipMemcpy(&nr1, JR->d_misc, sizeof(unsigned long long),
                            hipMemcpyDeviceToHost));
        jd.null_row = nr1 ? (int64_t)(nr1 - 1) : -1;
        HIP_CHECK(ytql_launch_join_chain(&jd, fn, (unsigned*)(JR->d_misc + 1), stream));
        unsigned long long dupw = 0;
        HIP_CHECK(hipMemcpy(&dupw, JR->d_misc + 1, sizeof(unsigned long long),
                            hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(&kerr, JR->Rf.d_err, sizeof(unsigned),
                            hipMemcpyDeviceToHost));
        jd.has_dups = ((unsigned*)&dupw)[1] != 0;
        if (kerr) {
            set_err(errbuf, errlen, "join: foreign decode error");
            return (int)kerr;
        }
        HIP_CHECK(hipMemsetAsync(JR->Rf.d_err, 0, sizeof(unsigned), stream));
    }
    return YT_OK;
}

/* diagnostic: the string-key joins of this thread's last query — foreign
 * rows that claimed a slot of a string table, and primary entries probed by
 * the entry pass (both summed over the join items) */
extern "C" void yt_gpu_debug_last_strjoin(uint64_t* inserted, uint64_t* entries)
{
    if (inserted) *inserted = t_last_strjoin_inserted;
    if (entries) *entries = t_last_strjoin_entries;
}

/* String-key join items, after setup_chunk of the primary: read back the key
 * column's parsed segments (the KEPT ones — input_row_limit truncates the
 * list), give every entry one jmap word, run the entry pass on the run's
 * stream and hand jmap + jbase to a COPY of the item's JoinDev in store[];
 * *jd / *jd2 are repointed at the copies. The buffers are R's. */
static int setup_strjoin_maps(DeviceRun* R, const JoinDev** jd, const JoinDev** jd2,
                              JoinDev store[2], char* errbuf, size_t errlen)
{
    const JoinDev** items[2] = {jd, jd2};
    for (int it = 0; it < 2; it++) {
        const JoinDev* src = *items[it];
        if (!src || !src->active || !src->key_kind || R->nsegs == 0) continue;
        const bool timing = getenv("YTQL_TIMING") != nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        const int off = R->h_off[src->pkey_col], cnt = R->h_cnt[src->pkey_col];
        std::vector<SegEx> ex(cnt ? cnt : 1);
        if (cnt)
            HIP_CHECK(hipMemcpy(ex.data(), R->d_segex + off, sizeof(SegEx) * cnt,
                                hipMemcpyDeviceToHost));
        std::vector<int64_t> base(cnt + 1);
        int64_t entries = 0;
        for (int sg = 0; sg < cnt; sg++) {
            if (!(ex[sg].flags & (8 | 32 | 64))) {
                set_err(errbuf, errlen, "join: unknown string segment layout");
                return YT_ERR_UNSUPPORTED;
            }
            base[sg] = entries;
            entries += ex[sg].dict_size;
        }
        base[cnt] = entries;
        int64_t* d_base = nullptr;
        int32_t* d_map = nullptr;
        HIP_CHECK(R->ps.dev(&d_base, sizeof(int64_t) * (cnt + 1)));
        HIP_CHECK(R->ps.dev(&d_map, sizeof(int32_t) * (entries ? entries : 1)));
        /* base is pageable: the copy has left it when the call returns */
        HIP_CHECK(hipMemcpyAsync(d_base, base.data(), sizeof(int64_t) * (cnt + 1),
                                 hipMemcpyHostToDevice, R->stream));
        if (timing) {
            HIP_CHECK(R->ps.event(&e0));
            HIP_CHECK(R->ps.event(&e1));
            HIP_CHECK(hipEventRecord(e0, R->stream));
        }
        if (entries)
            HIP_CHECK(ytql_launch_strjoin_entries(R->d_segs, R->d_segex, off, cnt,
                                                  d_base, entries, src, d_map,
                                                  R->stream));
        t_last_strjoin_entries += (uint64_t)entries;
        if (timing) {
            float ms = 0;
            HIP_CHECK(hipEventRecord(e1, R->stream));
            HIP_CHECK(hipEventSynchronize(e1));
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            fprintf(stderr, "[ytql timing] string join: %lld entries, entry "
                            "pass %.3fms\n", (long long)entries, ms);
        }
        store[it] = *src;
        store[it].jmap = d_map;
        store[it].jbase = d_base;
        *items[it] = &store[it];
    }
    return YT_OK;
}

/* diagnostic: the string-id passes of this thread's last query — entries
 * covered and distinct strings found, summed over the plan's STRING key
 * columns (a column that is a key twice is numbered once) */
extern "C" void yt_gpu_debug_last_strkey(uint64_t* entries, uint64_t* distinct)
{
    if (entries) *entries = t_last_strkey_entries;
    if (distinct) *distinct = t_last_strkey_distinct;
}

/* STRING components of a multi-key plan, after setup_chunk: number the
 * distinct strings of each such column over the entries of its KEPT segments
 * (the set setup_strjoin_maps walks) — hash, claim, compact, remap
 * (kernels.hip k_strkey_*) on the run's stream — and hand kmap + kbase to the
 * plan. The id table and its bytes come to the host once, for emit_rows.
 * kmap and kbase are R's; the pass's scratch goes back before it returns. */
static int setup_strkey_ids(DeviceRun* R, const DevPlan* dp,
                            StrKeyTab tabs[kMaxPackKeys],
                            char* errbuf, size_t errlen)
{
    const bool timing = getenv("YTQL_TIMING") != nullptr;
    for (int i = 0; i < dp->kp_count; i++) {
        if (!kp_is_str(dp, i)) continue;
        const int col = dp->kp_col[i];
        int same = -1;
        for (int j = 0; j < i; j++)
            if (dp->kp_col[j] == col) { same = j; break; }
        if (same >= 0) {
            R->strkeys.kmap[i] = R->strkeys.kmap[same];
            R->strkeys.kbase[i] = R->strkeys.kbase[same];
            tabs[i] = tabs[same];
            continue;
        }
        const int off = R->h_off[col], cnt = R->h_cnt[col];
        std::vector<SegEx> ex(cnt ? cnt : 1);
        if (cnt)
            HIP_CHECK(hipMemcpy(ex.data(), R->d_segex + off, sizeof(SegEx) * cnt,
                                hipMemcpyDeviceToHost));
        std::vector<int64_t> base(cnt + 1);
        int64_t entries = 0;
        uint64_t pool_cap = 0;
        for (int sg = 0; sg < cnt; sg++) {
            if (!(ex[sg].flags & (8 | 32 | 64))) {
                set_err(errbuf, errlen, "string keys: unknown key segment layout");
                return YT_ERR_UNSUPPORTED;
            }
            base[sg] = entries;
            entries += ex[sg].dict_size;
            /* a segment's blob bounds the bytes of its entries */
            pool_cap += (uint64_t)R->h_segs[off + sg].blob_bytes;
        }
        base[cnt] = entries;
        if (entries >= ((int64_t)1 << 30)) {
            set_err(errbuf, errlen,
                    "multi-key GROUP BY: string key column with 2^30 entries "
                    "or more: not this round");
            return YT_ERR_UNSUPPORTED;
        }
        if (pool_cap < 1024) pool_cap = 1024;
        const size_t ne = (size_t)(entries ? entries : 1);

        PoolScope ps;               /* the pass's scratch */
        int64_t* d_base = nullptr;
        uint32_t* d_map = nullptr;
        uint64_t* d_hashes = nullptr;
        uint64_t* d_idents = nullptr;
        ulonglong2* d_pfxs = nullptr;
        TableHdr* d_kth = nullptr;
        StrSlot* d_slots = nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        HIP_CHECK(R->ps.dev(&d_base, sizeof(int64_t) * (cnt + 1)));
        HIP_CHECK(R->ps.dev(&d_map, sizeof(uint32_t) * ne));
        HIP_CHECK(ps.dev(&d_hashes, sizeof(uint64_t) * ne));
        HIP_CHECK(ps.dev(&d_idents, sizeof(uint64_t) * ne));
        HIP_CHECK(ps.dev(&d_pfxs, sizeof(ulonglong2) * ne));
        HIP_CHECK(ps.dev(&d_kth, sizeof(TableHdr)));
        /* base is pageable: the copy has left it when the call returns */
        HIP_CHECK(hipMemcpyAsync(d_base, base.data(), sizeof(int64_t) * (cnt + 1),
                                 hipMemcpyHostToDevice, R->stream));
        HIP_CHECK(hipMemsetAsync(d_kth, 0, sizeof(TableHdr), R->stream));
        if (timing) {
            HIP_CHECK(ps.event(&e0));
            HIP_CHECK(ps.event(&e1));
            HIP_CHECK(hipEventRecord(e0, R->stream));
        }
        /* the table: as run_string_group sizes it — half the entries to
         * start with, 4x on overflow up to twice the entries */
        uint64_t nslots_cap = next_pow2((uint64_t)ne * 2);
        if (nslots_cap < 2048) nslots_cap = 2048;
        uint64_t nslots = next_pow2((uint64_t)ne / 2 + 1);
        if (nslots < 2048) nslots = 2048;
        if (nslots > nslots_cap) nslots = nslots_cap;
        TableHdr kth;
        memset(&kth, 0, sizeof(kth));
        if (entries) {
            HIP_CHECK(ytql_launch_strgrp_hash(R->d_segs, R->d_segex, off, cnt, d_base,
                                              d_hashes, d_idents, d_pfxs, entries,
                                              R->stream));
            for (;;) {
                HIP_CHECK(ps.dev(&d_slots, sizeof(StrSlot) * nslots));
                HIP_CHECK(hipMemsetAsync(d_slots, 0, sizeof(StrSlot) * nslots,
                                         R->stream));
                HIP_CHECK(ytql_launch_strkey_claim(R->d_segs, R->d_segex, off, cnt,
                                                   d_base, d_hashes, d_idents,
                                                   d_pfxs, d_slots, nslots, d_map,
                                                   d_kth, entries, R->stream));
                HIP_CHECK(hipMemcpyAsync(&kth, d_kth, sizeof(kth),
                                         hipMemcpyDeviceToHost, R->stream));
                HIP_CHECK(hipStreamSynchronize(R->stream));
                if (kth.overflow != 1 || nslots >= nslots_cap) break;
                ps.release(d_slots);
                d_slots = nullptr;
                nslots *= 4;
                if (nslots > nslots_cap) nslots = nslots_cap;
                HIP_CHECK(hipMemsetAsync(d_kth, 0, sizeof(TableHdr), R->stream));
            }
            if (kth.overflow == 1) {
                set_err(errbuf, errlen, "string key id table overflow");
                return YT_ERR_CAPACITY;
            }
        }
        const int64_t D = (int64_t)kth.ngroups;
        StrKeyTab& T = tabs[i];
        T.ids.resize((size_t)D);
        if (D > 0) {
            StrKeyId* d_ids = nullptr;
            char* d_pool = nullptr;
            unsigned long long* d_ctr = nullptr;
            unsigned long long hctr[2] = {0, 0};
            HIP_CHECK(ps.dev(&d_ids, sizeof(StrKeyId) * D));
            HIP_CHECK(ps.dev(&d_pool, pool_cap));
            HIP_CHECK(ps.dev(&d_ctr, 2 * sizeof(unsigned long long)));
            HIP_CHECK(hipMemsetAsync(d_ctr, 0, 2 * sizeof(unsigned long long),
                                     R->stream));
            HIP_CHECK(ytql_launch_strkey_compact(R->d_segs, R->d_segex, off, d_slots,
                                                 nslots, d_ids, d_ctr, d_pool,
                                                 d_ctr + 1, pool_cap, d_kth,
                                                 R->stream));
            HIP_CHECK(ytql_launch_strkey_remap(d_slots, d_map, entries, R->stream));
            HIP_CHECK(hipMemcpyAsync(&kth, d_kth, sizeof(kth), hipMemcpyDeviceToHost,
                                     R->stream));
            HIP_CHECK(hipMemcpyAsync(hctr, d_ctr, sizeof(hctr), hipMemcpyDeviceToHost,
                                     R->stream));
            HIP_CHECK(hipMemcpyAsync(T.ids.data(), d_ids, sizeof(StrKeyId) * D,
                                     hipMemcpyDeviceToHost, R->stream));
            HIP_CHECK(hipStreamSynchronize(R->stream));
            if (kth.overflow == 1 || hctr[0] != (unsigned long long)D ||
                hctr[1] > pool_cap) {
                set_err(errbuf, errlen, "string key id pool overflow");
                return YT_ERR_CAPACITY;
            }
            T.pool.resize((size_t)(hctr[1] ? hctr[1] : 1));
            if (hctr[1])
                HIP_CHECK(hipMemcpy(T.pool.data(), d_pool, (size_t)hctr[1],
                                    hipMemcpyDeviceToHost));
        }
        t_last_strkey_entries += (uint64_t)entries;
        t_last_strkey_distinct += (uint64_t)D;
        if (timing) {
            float ms = 0;
            HIP_CHECK(hipEventRecord(e1, R->stream));
            HIP_CHECK(hipEventSynchronize(e1));
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            fprintf(stderr, "[ytql timing] string key ids: %lld entries, %lld "
                            "distinct, entry pass %.3fms\n",
                    (long long)entries, (long long)D, ms);
        }
        HIP_CHECK(hipStreamSynchronize(R->stream));
        R->strkeys.kmap[i] = d_map;
        R->strkeys.kbase[i] = d_base;
    }
    return YT_OK;
}

/* drive the join chain (2 items max this round; duplicate foreign keys on
 * the FIRST item only — the cross-product machinery binds item 0) */
static int setup_join_chain(const YtPlan* plan, const YtChunk* chunk,
                            JoinRun* JR, JoinDev const** jd0,
                            JoinDev const** jd1,
                            hipStream_t stream, char* errbuf, size_t errlen)
{
    static const JoinDev kNone = {};
    *jd0 = &kNone;
    *jd1 = &kNone;
    uint8_t rt[kMaxCols];
    int rn = chunk->column_count;
    if (rn > kMaxCols) { set_err(errbuf, errlen, "too many columns"); return YT_ERR_UNSUPPORTED; }
    for (int c = 0; c < rn; c++) rt[c] = (uint8_t)chunk->columns[c].value_type;
    int nj = 0;
    for (const YtJoin* J = plan->join; J; J = J->next) {
        if (nj >= 2) {
            set_err(errbuf, errlen, "join: more than two join items not this round");
            return YT_ERR_UNSUPPORTED;
        }
        int rc = setup_join_item(J, rt, rn, chunk->column_count, &JR[nj], stream,
                                 errbuf, errlen);
        if (rc != YT_OK) return rc;
        if (nj == 1 && JR[1].jd.has_dups) {
            set_err(errbuf, errlen,
                    "join: duplicate foreign keys on a non-first join item "
                    "not this round");
            return YT_ERR_UNSUPPORTED;
        }
        for (int j = 0; j < J->foreign_value_count; j++) {
            if (rn >= kMaxCols) { set_err(errbuf, errlen, "too many columns"); return YT_ERR_UNSUPPORTED; }
            rt[rn++] = (uint8_t)J->foreign->columns[J->foreign_value_cols[j]].value_type;
        }
        nj++;
    }
    if (nj >= 1) *jd0 = &JR[0].jd;
    if (nj >= 2) *jd1 = &JR[1].jd;
    return YT_OK;
}

static void fold_totals_rows(const YtPlan* plan, const YtRowset* out,
                             std::vector<YtValue>& tot)
{
    int kc = plan->key_count, ac = plan->agg_count;
    int ncols = out->column_count;
    tot.assign(ac, YtValue());
    for (int a = 0; a < ac; a++) {
        tot[a].id = (uint16_t)(kc + a);
        tot[a].type = YT_VT_NULL;
    }
    for (int64_t r = 0; r < out->row_count; r++) {
        const YtValue* row = out->values + r * ncols;
        for (int a = 0; a < ac; a++) {
            const YtValue& v = row[kc + a];
            if (v.type == YT_VT_NULL) continue;
            YtValue& t = tot[a];
            int f = plan->aggs[a]->func;
            if (t.type == YT_VT_NULL) {
                t.type = v.type;
                t.data.bits = v.data.bits;
                continue;
            }
            if (f == YT_AGG_SUM || f == YT_AGG_SUM1) {
                if (v.type == YT_VT_DOUBLE) t.data.dbl += v.data.dbl;
                else t.data.bits += v.data.bits;   /* mod 2^64, udf/sum.c */
            } else if (f == YT_AGG_FIRST) {
                /* keep the first non-null (already in t) */
            } else {
                bool take;
                if (v.type == YT_VT_DOUBLE)
                    take = (f == YT_AGG_MAX) ? (v.data.dbl > t.data.dbl)
                                             : (v.data.dbl < t.data.dbl);
                else if (v.type == YT_VT_INT64)
                    take = (f == YT_AGG_MAX) ? (v.data.i64 > t.data.i64)
                                             : (v.data.i64 < t.data.i64);
                else
                    take = (f == YT_AGG_MAX) ? (v.data.u64 > t.data.u64)
                                             : (v.data.u64 < t.data.u64);
                if (take) t.data.bits = v.data.bits;
            }
        }
    }
}

static void hexpr_cols(const YtExpr* e, uint64_t* mask)
{
    if (!e) return;
    if (e->op == YT_EX_COLUMN && e->col >= 0 && e->col < 64)
        *mask |= 1ULL << e->col;
    hexpr_cols(e->a, mask);
    hexpr_cols(e->b, mask);
}

/* totals(BeforeHaving) → HAVING → totals(AfterHaving) → ORDER/limit →
 * append totals row (folding_profiler.cpp:1810-1815 Process() order;
 * parser.ypp:469-481 totals modes) */
static int finish_output(const YtPlan* plan, YtRowset* out,
                         char* errbuf, size_t errlen)
{
    std::vector<YtValue> tot;
    const bool after = plan->totals_mode == 2;
    /* all-null group keys are forbidden on the INTERMEDIATE stream (WITH
     * TOTALS re-folds rows) and in the group-combined-with-order op —
     * registry.cpp ValidateGroupKeyIsNotNull:1460-1476, call sites
     * :1795,:1820; pinned by GroupByWithTotalsNulls ql_query_ut.cpp:3989 */
    if (plan->with_totals || plan->order_count > 0) {
        const int kc0 = plan->key_count;
        const int nc0 = out->column_count;
        for (int64_t r = 0; r < out->row_count; r++) {
            const YtValue* row = out->values + r * nc0;
            bool allnull = kc0 > 0;
            for (int k = 0; k < kc0; k++)
                if (row[k].type != YT_VT_NULL) { allnull = false; break; }
            if (allnull) {
                set_err(errbuf, errlen, "Null values are forbidden in group key");
                return YT_ERR_INVALID_PLAN;
            }
        }
    }
    const int64_t had_group_rows = out->row_count;
    if (plan->with_totals && !after) fold_totals_rows(plan, out, tot);
    if (plan->having) {
        if (expr_has_strlit(plan->having)) {
            set_err(errbuf, errlen, "HAVING over string values: not this round");
            return YT_ERR_UNSUPPORTED;
        }
        int ncols = out->column_count;
        uint64_t mask = 0;
        hexpr_cols(plan->having, &mask);
        /* IN lists: sorted once, binary-searched per group row */
        std::vector<InNumSet> hin;
        int hrc = hin_collect(plan->having, &hin, errbuf, errlen);
        if (hrc) return hrc;
        struct HinScope {
            HinScope(const std::vector<InNumSet>* s) { t_hin = s; }
            ~HinScope() { t_hin = nullptr; }
        } hin_scope(&hin);
        int64_t w = 0;
        HVal hrow[32];
        for (int64_t r = 0; r < out->row_count; r++) {
            YtValue* row = out->values + r * ncols;
            for (int i = 0; i < ncols && i < 32; i++) {
                if (((mask >> i) & 1) && row[i].type == YT_VT_STRING) {
                    set_err(errbuf, errlen,
                            "HAVING over string values: not this round");
                    return YT_ERR_UNSUPPORTED;
                }
                hrow[i].type = row[i].type;
                hrow[i].bits = row[i].data.bits;
            }
            HVal h;
            int rc = heval(plan->having, hrow, ncols, &h);
            if (rc) { set_err(errbuf, errlen, "HAVING expression error"); return rc; }
            if (h.type == YT_VT_NULL || h.bits == 0) continue;
            if (w != r)
                memmove(out->values + w * ncols, row, sizeof(YtValue) * ncols);
            w++;
        }
        out->row_count = w;
    }
    if (plan->with_totals && after) fold_totals_rows(plan, out, tot);
    if (plan->order_count > 0) {
        int rc = apply_order_host(plan, out, errbuf, errlen);
        if (rc) return rc;
    }
    if (plan->with_totals && had_group_rows > 0) {
        int kc = plan->key_count, ac = plan->agg_count;
        int ncols = out->column_count;
        if (out->row_count >= out->capacity_rows) {
            set_err(errbuf, errlen, "rowset too small for the totals row");
            return YT_ERR_CAPACITY;
        }
        YtValue* dst = out->values + out->row_count * ncols;
        for (int k = 0; k < kc; k++) {
            dst[k].id = (uint16_t)k;
            dst[k].type = YT_VT_NULL;
            dst[k].flags = 0;
            dst[k].length = 0;
            dst[k].data.bits = 0;
        }
        for (int a = 0; a < ac; a++) {
            dst[kc + a] = tot[a];
            if (plan->aggs[a]->func == YT_AGG_SUM1 &&
                dst[kc + a].type == YT_VT_NULL) {
                dst[kc + a].type = YT_VT_INT64;   /* sum(1) over zero rows */
                dst[kc + a].data.bits = 0;
            }
        }
        out->row_count++;
        out->totals_row = 1;
    }
    return YT_OK;
}

static unsigned string_proj_mask(const DevPlan* dp);
static void emit_proj_value(YtValue* dst, int pj, const DevOutVal& v,
                            char* pool_base);

/* scan + ORDER BY ... LIMIT without materializing the scan: histogram
 * k-selection on an order-isomorphic u64 mapping of the first order key
 * (digits of 11 bits, host-driven refinement), then exact candidate gather
 * and a full-comparer host sort of the <=(K + tie-cap) survivors.
 * Selection runs the same expression program as the projection, so any
 * filter/projection the generic path supports works here. */
static int run_scan_topk(const YtPlan* plan, const YtChunk* chunk,
                         const YtExecOptions* options, const DevPlan* dp,
                         StrPreds* sp,
                         const JoinDev* jd, const JoinDev* jd2,
                         YtRowset* output, YtStatistics* stats, double tw0,
                         char* errbuf, size_t errlen)
{
    int rc = YT_OK;
    const int np = plan->project_count;
    rc = ord_validate_plan(plan, np, errbuf, errlen);
    if (rc != YT_OK) return rc;
    const int64_t K = plan->order_offset + plan->order_limit;
    if (K > ((int64_t)1 << 24)) {
        set_err(errbuf, errlen, "ORDER BY LIMIT capped at 16M rows this round");
        return YT_ERR_UNSUPPORTED;
    }

    DeviceRun R2;
    PoolScope ps;
    DevPlan dpl = *dp;      /* + this run's string-predicate bitmaps */
    R2.stream = (hipStream_t)(uintptr_t)options->stream;
    unsigned mw = 0;
    int in_clamped = 0;
    rc = setup_chunk(chunk, &R2, &mw, options->input_row_limit, &in_clamped,
                     errbuf, errlen);
    if (rc) return rc;
    rc = setup_string_preds(sp, &R2, &dpl, errbuf, errlen);
    if (rc) return rc;
    JoinDev jstr[2];        /* + this run's string-join maps */
    rc = setup_strjoin_maps(&R2, &jd, &jd2, jstr, errbuf, errlen);
    if (rc) return rc;
    dp = &dpl;
    if (stats) stats->decode_time_ms = now_ms() - tw0;   /* setup phase */
    int64_t n = chunk->row_count;
    if (options->input_row_limit > 0 && options->input_row_limit < n)
        n = options->input_row_limit;
    output->row_count = 0;
    output->column_count = np;
    if (n == 0 || R2.nsegs == 0) return YT_OK;
    if (in_clamped && stats) stats->incomplete_input = 1;

    const int ord0 = plan->order_cols[0];
    const int desc0 = plan->order_desc ? plan->order_desc[0] : 0;
    const int64_t CAPB = (int64_t)1 << 17;

    /* fast selection passes: plain DirectDense int column key, no filter,
     * no join, uniform segmentation (k_topk_*_fast — 4 rows in flight per
     * thread, no interpreter) */
    int fast_col = -1, fast_signed = 0, fast_nulls = 0, fast_shift = 0;
    {
        int kcol;
        if (!plan->filter && !plan->join &&
            expr_is_col(plan->projects[ord0], &kcol) &&
            kcol < chunk->column_count &&
            (chunk->columns[kcol].value_type == YT_VT_INT64 ||
             chunk->columns[kcol].value_type == YT_VT_UINT64) &&
            dp->col_uniform_shift[kcol] != 0) {
            bool all_dd = true;
            for (int i = 0; i < chunk->columns[kcol].segment_count; i++) {
                if (chunk->columns[kcol].segments[i].type != YT_SEG_DIRECT_DENSE) {
                    all_dd = false;
                    break;
                }
            }
            if (all_dd) {
                fast_col = kcol;
                fast_signed = chunk->columns[kcol].value_type == YT_VT_INT64;
                fast_nulls = R2.col_null_flags[kcol] != 0;
                fast_shift = dp->col_uniform_shift[kcol];
            }
        }
    }

    unsigned long long* d_bins = nullptr;   /* 2048 bins + misc(3) + ctrs(3) */
    HIP_CHECK(ps.dev(&d_bins, sizeof(unsigned long long) * (2048 + 8)));
    unsigned long long* d_misc = d_bins + 2048;   /* null_cnt, mmin, mmax */
    unsigned long long* d_ctrs = d_bins + 2051;   /* strict, tie, null */
    HIP_CHECK(hipMemsetAsync(R2.d_err, 0, sizeof(unsigned), R2.stream));

    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_CHECK(ps.event(&e0));
    HIP_CHECK(ps.event(&e1));
    HIP_CHECK(hipEventRecord(e0, R2.stream));

    TopkPass tp;
    tp.order_proj = ord0;
    tp.desc = desc0;
    tp.level0 = 1;
    tp.shift = 53;
    tp.lo = 0;
    tp.hi = ~0ULL;

    uint64_t lo = 0, hi = ~0ULL;
    int shift = 53;
    int64_t S = 0, T = 0, nonnull = 0, k_nonnull = 0;
    unsigned long long null_cnt = 0;
    bool all_nonnull = false, only_nulls = false;
    std::vector<unsigned long long> h_bins(2051);
    int launches = 0;

    for (;;) {
        HIP_CHECK(hipMemsetAsync(d_bins, 0,
                                 sizeof(unsigned long long) * 2049, R2.stream));
        if (tp.level0) {
            /* mmin = ~0, mmax = 0 */
            HIP_CHECK(hipMemsetAsync(d_misc + 1, 0xFF,
                                     sizeof(unsigned long long), R2.stream));
            HIP_CHECK(hipMemsetAsync(d_misc + 2, 0,
                                     sizeof(unsigned long long), R2.stream));
        }
        if (fast_col >= 0) {
            HIP_CHECK(ytql_launch_topk_hist_fast(
                R2.d_segs, R2.d_segex, R2.h_off[fast_col], fast_shift, n,
                fast_nulls, fast_signed, &tp, d_bins, d_misc, R2.stream));
        } else {
            HIP_CHECK(ytql_launch_topk_hist(dp, R2.d_segs, R2.d_segex,
                                            R2.d_off, R2.d_cnt, n, jd,
                                            jd2, &tp,
                                            d_bins, d_misc,
                                            R2.d_err, R2.stream));
        }
        launches++;
        HIP_CHECK(hipMemcpy(h_bins.data(), d_bins,
                            sizeof(unsigned long long) * 2051,
                            hipMemcpyDeviceToHost));
        unsigned kerr = 0;
        HIP_CHECK(hipMemcpy(&kerr, R2.d_err, sizeof(unsigned),
                            hipMemcpyDeviceToHost));
        if (kerr) {
            if (kerr == 100) {
                set_err(errbuf, errlen, "NaN in ORDER BY comparison");
                return YT_ERR_LIMIT;
            }
            set_err(errbuf, errlen, "unsupported ORDER BY key type");
            return (int)kerr;
        }
        uint64_t mmin = h_bins[2049], mmax = h_bins[2050];
        if (tp.level0) {
            null_cnt = h_bins[2048];
            nonnull = 0;
            for (int i = 0; i < 2048; i++) nonnull += (int64_t)h_bins[i];
            const bool nulls_first = !desc0;
            int64_t null_take = nulls_first
                ? ((int64_t)null_cnt < K ? (int64_t)null_cnt : K)
                : (K - nonnull > 0 ? K - nonnull : 0);
            k_nonnull = K - (nulls_first ? null_take : 0);
            if (!nulls_first && k_nonnull > nonnull) k_nonnull = nonnull;
            if (k_nonnull <= 0) { only_nulls = true; break; }
            if (k_nonnull >= nonnull) { all_nonnull = true; S = nonnull; break; }
        }
        int64_t cum = 0;
        int t = -1;
        for (int i = 0; i < 2048; i++) {
            if (S + cum + (int64_t)h_bins[i] >= k_nonnull) { t = i; break; }
            cum += (int64_t)h_bins[i];
        }
        if (t < 0) {   /* cannot happen: counts shrank between passes */
            set_err(errbuf, errlen, "ORDER BY selection internal error");
            return YT_ERR_HIP;
        }
        S += cum;
        T = (int64_t)h_bins[t];
        /* shrink [lo, hi] to the chosen bin (∩ data bounds on pass 0) */
        uint64_t nlo = lo + ((uint64_t)t << shift);
        uint64_t span = (uint64_t)(t + 1) << shift;
        uint64_t nhi = (span == 0 || nlo + (span - ((uint64_t)t << shift)) - 1 < nlo)
            ? hi : nlo + (((uint64_t)1 << shift) - 1);
        if (nhi > hi) nhi = hi;
        if (tp.level0) {
            if (mmin > nlo) nlo = mmin;
            if (mmax < nhi) nhi = mmax;
        }
        lo = nlo;
        hi = nhi;
        if (T <= CAPB || shift == 0 || lo >= hi) break;
        uint64_t range = hi - lo;     /* >= 1 */
        shift = 0;
        while ((range >> shift) >= 2048) shift++;
        tp.lo = lo;
        tp.hi = hi;
        tp.shift = shift;
        tp.level0 = 0;
    }

    /* refinement stops above CAPB only on one key value (shift == 0 bins are
     * single values, lo >= hi is one) */
    const bool big_tie = !all_nonnull && !only_nulls && T > CAPB;
    t_last_topk = (fast_col >= 0 ? YT_TOPK_FAST : 0)
        | (only_nulls ? YT_TOPK_ONLY_NULLS : 0)
        | (all_nonnull ? YT_TOPK_ALL_NONNULL : 0)
        | (big_tie ? YT_TOPK_BIG_TIE : 0)
        | ((uint32_t)(launches > 255 ? 255 : launches) << YT_TOPK_PASSES_SHIFT);

    if (big_tie && plan->order_count > 1) {
        set_err(errbuf, errlen,
                "order-key tie set too large for multi-key ORDER BY this round");
        return YT_ERR_UNSUPPORTED;
    }
    const int64_t CAPN = K + CAPB;
    {
        const bool nulls_first = !desc0;
        int64_t null_take = nulls_first
            ? ((int64_t)null_cnt < K ? (int64_t)null_cnt : K)
            : (K - nonnull > 0 ? K - nonnull : 0);
        if ((int64_t)null_cnt > CAPN && plan->order_count > 1 &&
            null_take > 0 && null_take < (int64_t)null_cnt) {
            set_err(errbuf, errlen,
                    "null order-key set too large for multi-key ORDER BY this round");
            return YT_ERR_UNSUPPORTED;
        }
    }

    /* gather candidates: strict (exactly S), ties (cap), nulls (cap) */
    TopkGather tg;
    tg.order_proj = ord0;
    tg.desc = desc0;
    tg.all_nonnull = all_nonnull ? 1 : 0;
    tg.pad_ = 0;
    /* only_nulls: nothing strict (strict is m < lo, so lo = 0 matches
     * no row — a mapped key CAN be 0, e.g. INT64_MIN ascending, and S is
     * 0 here) and at most the capped tie bucket */
    tg.lo = only_nulls ? 0 : lo;
    tg.hi = only_nulls ? 0 : hi;
    /* the ties still owed are k_nonnull - S; above CAPB that is one key
     * value (big_tie), and with a single order key any k_nonnull - S of its
     * rows are a correct answer (more keys were refused above) */
    int64_t cap_tie = CAPB;
    if (big_tie && k_nonnull - S > cap_tie) cap_tie = k_nonnull - S;
    tg.cap_strict = S;
    tg.cap_tie = cap_tie;
    tg.cap_null = CAPN;
    int64_t* d_rows_strict = nullptr;
    int64_t* d_rows_tie = nullptr;
    int64_t* d_rows_null = nullptr;
    HIP_CHECK(ps.dev(&d_rows_strict, sizeof(int64_t) * (S ? S : 1)));
    HIP_CHECK(ps.dev(&d_rows_tie, sizeof(int64_t) * cap_tie));
    HIP_CHECK(ps.dev(&d_rows_null, sizeof(int64_t) * CAPN));
    HIP_CHECK(hipMemsetAsync(d_ctrs, 0, 3 * sizeof(unsigned long long),
                             R2.stream));
    if (fast_col >= 0) {
        HIP_CHECK(ytql_launch_topk_gather_fast(
            R2.d_segs, R2.d_segex, R2.h_off[fast_col], fast_shift, n,
            fast_nulls, fast_signed, &tg,
            d_rows_strict, d_ctrs, d_rows_tie, d_ctrs + 1,
            d_rows_null, d_ctrs + 2, R2.stream));
    } else {
        HIP_CHECK(ytql_launch_topk_gather(dp, R2.d_segs, R2.d_segex,
                                          R2.d_off, R2.d_cnt, n, jd,
                                          jd2, &tg,
                                          d_rows_strict, d_ctrs,
                                          d_rows_tie, d_ctrs + 1,
                                          d_rows_null, d_ctrs + 2,
                                          R2.d_err, R2.stream));
    }
    launches++;
    unsigned long long hctrs[3];
    HIP_CHECK(hipMemcpy(hctrs, d_ctrs, 3 * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost));
    int64_t nS = (int64_t)hctrs[0];
    if (nS != S) {   /* cannot happen: the gather counts what the passes did */
        set_err(errbuf, errlen, "ORDER BY selection internal error");
        return YT_ERR_HIP;
    }
    int64_t nB = (int64_t)hctrs[1] < cap_tie ? (int64_t)hctrs[1] : cap_tie;
    int64_t nN = (int64_t)hctrs[2] < CAPN ? (int64_t)hctrs[2] : CAPN;
    int64_t M = nS + nB + nN;

    /* pack the three lists and materialize the projected rows */
    int64_t* d_rows_all = nullptr;
    DevOutVal* d_vals = nullptr;
    DevOutVal* h_vals = nullptr;
    HIP_CHECK(ps.dev(&d_rows_all, sizeof(int64_t) * (M ? M : 1)));
    if (nS) HIP_CHECK(hipMemcpyAsync(d_rows_all, d_rows_strict,
                                     sizeof(int64_t) * nS,
                                     hipMemcpyDeviceToDevice, R2.stream));
    if (nB) HIP_CHECK(hipMemcpyAsync(d_rows_all + nS, d_rows_tie,
                                     sizeof(int64_t) * nB,
                                     hipMemcpyDeviceToDevice, R2.stream));
    if (nN) HIP_CHECK(hipMemcpyAsync(d_rows_all + nS + nB, d_rows_null,
                                     sizeof(int64_t) * nN,
                                     hipMemcpyDeviceToDevice, R2.stream));
    HIP_CHECK(ps.dev(&d_vals, sizeof(DevOutVal) * (M ? M : 1) * np));
    HIP_CHECK(ps.host(&h_vals, sizeof(DevOutVal) * (M ? M : 1) * np));
    if (M) {
        HIP_CHECK(ytql_launch_topk_materialize(dp, R2.d_segs, R2.d_segex,
                                               R2.d_off, R2.d_cnt, jd, jd2,
                                               d_rows_all, M, d_vals,
                                               R2.d_err, R2.stream));
        launches++;
        HIP_CHECK(hipMemcpyAsync(h_vals, d_vals, sizeof(DevOutVal) * M * np,
                                 hipMemcpyDeviceToHost, R2.stream));
    }
    HIP_CHECK(hipEventRecord(e1, R2.stream));
    HIP_CHECK(hipStreamSynchronize(R2.stream));
    if (stats) stats->kernel_other_ms = now_ms() - tw0;  /* pre-emit wall */
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    unsigned kerr = 0;
    HIP_CHECK(hipMemcpy(&kerr, R2.d_err, sizeof(unsigned),
                        hipMemcpyDeviceToHost));
    if (kerr) {
        if (kerr == 100) {
            set_err(errbuf, errlen, "NaN in ORDER BY comparison");
            return YT_ERR_LIMIT;
        }
        set_err(errbuf, errlen,
                kerr == YT_ERR_DIV_ZERO ? "Division by zero" : "expression error");
        return (int)kerr;
    }

    /* host: full-comparer sort of the candidates, emit the slice */
    std::vector<int64_t> idx((size_t)M);
    for (int64_t i = 0; i < M; i++) idx[i] = i;
    int nan_err = 0;
    auto cmp_cand = [&](int64_t ia, int64_t ib) {
        const DevOutVal* a = h_vals + ia * np;
        const DevOutVal* b = h_vals + ib * np;
        for (int i = 0; i < plan->order_count; i++) {
            int c = plan->order_cols[i];
            const DevOutVal& x = a[c];
            const DevOutVal& y = b[c];
            int xn = x.type == YT_VT_NULL, yn = y.type == YT_VT_NULL;
            int r = 0;
            if (xn || yn) {
                r = (xn == yn) ? 0 : (xn ? -1 : 1);
            } else if (x.type == YT_VT_DOUBLE) {
                double xv, yv;
                memcpy(&xv, &x.bits, 8);
                memcpy(&yv, &y.bits, 8);
                if (xv != xv || yv != yv) { nan_err = 1; return false; }
                r = xv < yv ? -1 : (xv > yv ? 1 : 0);
            } else if (x.type == YT_VT_INT64) {
                int64_t xv = (int64_t)x.bits, yv = (int64_t)y.bits;
                r = xv < yv ? -1 : (xv > yv ? 1 : 0);
            } else {
                r = x.bits < y.bits ? -1 : (x.bits > y.bits ? 1 : 0);
            }
            if (plan->order_desc && plan->order_desc[i]) r = -r;
            if (r) return r < 0;
        }
        return false;
    };
    std::sort(idx.begin(), idx.end(), cmp_cand);
    if (nan_err) {
        set_err(errbuf, errlen, "NaN in ORDER BY comparison");
        return YT_ERR_LIMIT;
    }
    int64_t b = plan->order_offset < M ? plan->order_offset : M;
    int64_t e = b + plan->order_limit;
    if (e > M) e = M;
    int out_limited = 0;
    char* pool_base = nullptr;
    if (const unsigned str_mask = string_proj_mask(dp)) {
        /* only the emitted slice needs bytes: its string values become
         * gather records (row order of the slice), the device fills in
         * the lengths, the host lays them out, k_str_gather copies */
        int64_t ne = e - b;
        if (options->output_row_limit > 0 && ne > options->output_row_limit)
            ne = options->output_row_limit;    /* the loop below flags it */
        if (ne > output->capacity_rows) return YT_ERR_CAPACITY;
        std::vector<StrGatherRec> recs;
        std::vector<DevOutVal*> owner;
        for (int64_t i = b; i < b + ne; i++)
            for (int pj = 0; pj < np; pj++) {
                DevOutVal* v = h_vals + idx[i] * np + pj;
                if (!((str_mask >> pj) & 1) || v->type != YT_VT_STRING)
                    continue;
                StrGatherRec g;
                g.ref = v->bits;
                g.dst = 0;
                g.len = 0;
                g.pad_ = 0;
                recs.push_back(g);
                owner.push_back(v);
            }
        if (!recs.empty()) {
            const int64_t nr = (int64_t)recs.size();
            StrGatherRec* d_recs = nullptr;
            char* d_spool = nullptr;
            rc = YT_OK;
            uint64_t bytes = 0;
            hipError_t he = ps.dev(&d_recs, sizeof(StrGatherRec) * nr);
            if (he == hipSuccess)
                he = hipMemcpy(d_recs, recs.data(), sizeof(StrGatherRec) * nr,
                               hipMemcpyHostToDevice);
            if (he == hipSuccess)
                he = ytql_launch_str_reclen(R2.d_segs, R2.d_segex, d_recs, nr,
                                            R2.stream);
            if (he == hipSuccess) he = hipStreamSynchronize(R2.stream);
            if (he == hipSuccess)
                he = hipMemcpy(recs.data(), d_recs, sizeof(StrGatherRec) * nr,
                               hipMemcpyDeviceToHost);
            if (he == hipSuccess) {
                for (int64_t i = 0; i < nr; i++) {
                    recs[i].dst = bytes;
                    owner[i]->bits = bytes;      /* offset in this slice */
                    owner[i]->pad_ = recs[i].len;
                    bytes += recs[i].len;
                }
                if (bytes > 0 &&
                    (!output->string_pool ||
                     (uint64_t)output->string_pool_used + bytes >
                         (uint64_t)output->string_pool_capacity)) {
                    set_err(errbuf, errlen, "string pool too small");
                    rc = YT_ERR_CAPACITY;
                }
            }
            if (he == hipSuccess && rc == YT_OK && bytes) {
                pool_base = output->string_pool + output->string_pool_used;
                he = ps.dev(&d_spool, (size_t)bytes);
                if (he == hipSuccess)
                    he = hipMemcpy(d_recs, recs.data(),
                                   sizeof(StrGatherRec) * nr,
                                   hipMemcpyHostToDevice);
                if (he == hipSuccess)
                    he = ytql_launch_str_gather(R2.d_segs, R2.d_segex, d_recs,
                                                nr, d_spool, bytes, R2.stream);
                if (he == hipSuccess) he = hipStreamSynchronize(R2.stream);
                if (he == hipSuccess)
                    he = hipMemcpy(pool_base, d_spool, (size_t)bytes,
                                   hipMemcpyDeviceToHost);
                launches += 2;
            }
            ps.release(d_recs);
            ps.release(d_spool);
            if (he != hipSuccess) {
                if (errbuf) snprintf(errbuf, errlen, "HIP error %s (string gather)",
                                     hipGetErrorString(he));
                rc = YT_ERR_HIP;
            }
            if (rc != YT_OK) return rc;
            output->string_pool_used += (int64_t)bytes;
        }
    }
    for (int64_t i = b; i < e; i++) {
        if (options->output_row_limit > 0 &&
            output->row_count >= options->output_row_limit) {
            out_limited = 1;
            break;
        }
        if (output->row_count >= output->capacity_rows) return YT_ERR_CAPACITY;
        const DevOutVal* src = h_vals + idx[i] * np;
        YtValue* dst = output->values + output->row_count * np;
        for (int pj = 0; pj < np; pj++)
            emit_proj_value(dst + pj, pj, src[pj], pool_base);
        output->row_count++;
    }
    if (stats) {
        stats->rows_read = n;
        stats->rows_written = output->row_count;
        stats->incomplete_output = out_limited;
        stats->kernel_scan_ms += ms;
        stats->kernel_scan_launches += launches;
        stats->execute_time_ms = now_ms() - tw0;
    }
    return YT_OK;
}

/* bit pj set = projection pj is one P_STR_REF (a plain STRING column) */
static unsigned string_proj_mask(const DevPlan* dp)
{
    unsigned m = 0;
    for (int pj = 0; pj < dp->proj_count; pj++)
        if (dp->proj_len[pj] == 1 && dp->prog[dp->proj_off[pj]].op == P_STR_REF)
            m |= 1u << pj;
    return m;
}

/* one emitted value of a scan with string projections: v is the device
 * value, for a string with bits = byte offset inside this call's slice of
 * the pool (which starts at pool_base) and pad_ = length */
static void emit_proj_value(YtValue* dst, int pj, const DevOutVal& v,
                            char* pool_base)
{
    dst->id = (uint16_t)pj;
    dst->type = (uint8_t)v.type;
    dst->flags = 0;
    dst->length = 0;
    dst->data.bits = v.bits;
    if (v.type == YT_VT_STRING) {
        dst->length = v.pad_;
        dst->data.bits = 0;
        dst->data.str = pool_base ? pool_base + v.bits : nullptr;
    }
}

/* scan + filter + project with at least one STRING projection (DESIGN.md
 * §12): per window k_scan_project, then a stable device compaction — row and
 * byte offsets by reduce-then-scan, scatter of the survivors, byte gather
 * into a window pool — so that only surviving rows and their bytes cross to
 * the host. R is the set-up chunk, dp carries the string-predicate bitmaps. */
static int scan_project_compact(const YtPlan* plan, const YtExecOptions* options,
                                const DevPlan* dp, DeviceRun* R, int64_t n,
                                unsigned str_mask,
                                const JoinDev* jd, const JoinDev* jd2,
                                YtRowset* output, YtStatistics* stats, double tw0,
                                char* errbuf, size_t errlen)
{
    const int np = plan->project_count;
    int nstr = 0;
    for (int pj = 0; pj < np; pj++) nstr += (str_mask >> pj) & 1;
    const bool timing = getenv("YTQL_TIMING") != nullptr;
    int64_t kWin = (int64_t)1 << 24;
    if (const char* wv = getenv("YTQL_PROJ_WINDOW")) {    /* tests: small windows */
        long long w = atoll(wv);
        if (w < 64) w = 64;
        if (w < kWin) kWin = w;
    }
    const int64_t win = n < kWin ? n : kWin;
    const int64_t max_tiles = (win + kProjTile - 1) / kProjTile;
    DevOutVal* d_out = nullptr;
    uint8_t* d_pass = nullptr;
    ProjTot* d_tiles = nullptr;      /* [max_tiles] + the window totals */
    DevOutVal* d_cout = nullptr;
    StrGatherRec* d_recs = nullptr;
    char* d_pool = nullptr;
    DevOutVal* h_out = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float t_scan = 0, t_off = 0, t_scat = 0, t_gath = 0;
    double t_host = 0;
    int windows = 0;
    PoolScope ps;
    auto put_win = [&]() {
        ps.release(d_cout); ps.release(d_recs); ps.release(d_pool);
        ps.release(h_out);
        d_cout = nullptr; d_recs = nullptr; d_pool = nullptr; h_out = nullptr;
    };
    HIP_CHECK(ps.dev(&d_out, sizeof(DevOutVal) * win * np));
    HIP_CHECK(ps.dev(&d_pass, (size_t)win));
    HIP_CHECK(ps.dev(&d_tiles, sizeof(ProjTot) * (max_tiles + 1)));
    for (int i = 0; i < 5; i++) HIP_CHECK(ps.event(&ev[i]));
    HIP_CHECK(hipMemsetAsync(R->d_err, 0, sizeof(unsigned), R->stream));
    for (int64_t w0 = 0; w0 < n; w0 += win) {
        const int64_t wlen = (w0 + win <= n) ? win : (n - w0);
        const int ntiles = (int)((wlen + kProjTile - 1) / kProjTile);
        ProjTot* d_totals = d_tiles + ntiles;
        windows++;
        HIP_CHECK(hipEventRecord(ev[0], R->stream));
        HIP_CHECK(ytql_launch_scan_project(dp, R->d_segs, R->d_segex, R->d_off,
                                           R->d_cnt, w0, wlen, jd, jd2, d_out,
                                           d_pass, R->d_err, R->stream));
        HIP_CHECK(hipEventRecord(ev[1], R->stream));
        HIP_CHECK(ytql_launch_proj_offsets(R->d_segs, R->d_segex, d_out, d_pass,
                                           wlen, np, str_mask, d_tiles, d_totals,
                                           R->stream));
        HIP_CHECK(hipEventRecord(ev[2], R->stream));
        ProjTot tot;
        unsigned kerr = 0;
        HIP_CHECK(hipMemcpyAsync(&tot, d_totals, sizeof(tot),
                                 hipMemcpyDeviceToHost, R->stream));
        HIP_CHECK(hipMemcpyAsync(&kerr, R->d_err, sizeof(unsigned),
                                 hipMemcpyDeviceToHost, R->stream));
        HIP_CHECK(hipStreamSynchronize(R->stream));
        if (kerr) {
            set_err(errbuf, errlen, kerr == YT_ERR_DIV_ZERO ? "Division by zero" : "expression error");
            return (int)kerr;
        }
        const int64_t wrows = (int64_t)tot.rows;
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        t_scan += ms;
        HIP_CHECK(hipEventElapsedTime(&ms, ev[1], ev[2]));
        t_off += ms;
        if (wrows == 0) continue;

        /* limits, in the order of the uncompacted path: output_row_limit
         * stops the emit, then the rowset capacity, then the pool */
        int64_t take = wrows;
        bool limited = false;
        if (options->output_row_limit > 0 &&
            output->row_count + take > options->output_row_limit) {
            take = options->output_row_limit - output->row_count;
            limited = true;
        }
        if (output->row_count + take > output->capacity_rows) {
            set_err(errbuf, errlen, "rowset too small");
            return YT_ERR_CAPACITY;
        }
        if (take > 0) {
            HIP_CHECK(ps.dev(&d_cout, sizeof(DevOutVal) * wrows * np));
            HIP_CHECK(ps.dev(&d_recs, sizeof(StrGatherRec) * wrows * nstr));
            HIP_CHECK(ps.dev(&d_pool, (size_t)(tot.bytes ? tot.bytes : 1)));
            HIP_CHECK(ps.host(&h_out, sizeof(DevOutVal) * take * np));
            HIP_CHECK(hipEventRecord(ev[2], R->stream));
            HIP_CHECK(ytql_launch_proj_scatter(d_out, d_pass, wlen, np, str_mask,
                                               nstr, d_tiles, d_cout, d_recs,
                                               R->stream));
            HIP_CHECK(hipEventRecord(ev[3], R->stream));
            /* records are in row order: the first take * nstr of them are
             * the emitted rows', and their bytes a prefix of the pool */
            if (tot.bytes)
                HIP_CHECK(ytql_launch_str_gather(R->d_segs, R->d_segex, d_recs,
                                                 take * nstr, d_pool, tot.bytes,
                                                 R->stream));
            HIP_CHECK(hipEventRecord(ev[4], R->stream));
            HIP_CHECK(hipMemcpyAsync(h_out, d_cout, sizeof(DevOutVal) * take * np,
                                     hipMemcpyDeviceToHost, R->stream));
            HIP_CHECK(hipStreamSynchronize(R->stream));
            HIP_CHECK(hipEventElapsedTime(&ms, ev[2], ev[3]));
            t_scat += ms;
            HIP_CHECK(hipEventElapsedTime(&ms, ev[3], ev[4]));
            t_gath += ms;
            const double th0 = now_ms();
            uint64_t bytes = tot.bytes;
            if (take < wrows) {
                bytes = 0;
                for (int64_t i = 0; i < take * np; i++)
                    if (h_out[i].type == YT_VT_STRING) bytes += h_out[i].pad_;
            }
            if (bytes > 0 &&
                (!output->string_pool ||
                 (uint64_t)output->string_pool_used + bytes >
                     (uint64_t)output->string_pool_capacity)) {
                set_err(errbuf, errlen, "string pool too small");
                return YT_ERR_CAPACITY;
            }
            char* pool_base = output->string_pool
                ? output->string_pool + output->string_pool_used : nullptr;
            if (bytes)
                HIP_CHECK(hipMemcpy(pool_base, d_pool, (size_t)bytes,
                                    hipMemcpyDeviceToHost));
            YtValue* dst = output->values + output->row_count * np;
            for (int64_t i = 0; i < take; i++)
                for (int pj = 0; pj < np; pj++)
                    emit_proj_value(dst + i * np + pj, pj, h_out[i * np + pj],
                                    pool_base);
            output->row_count += take;
            output->string_pool_used += (int64_t)bytes;
            t_host += now_ms() - th0;
            put_win();
        }
        if (limited) {
            if (stats) stats->incomplete_output = 1;
            break;
        }
        if (options->output_row_limit > 0 &&
            output->row_count >= options->output_row_limit)
            break;
    }
    if (stats) {
        stats->rows_read = n;
        stats->rows_written = output->row_count;
        stats->kernel_scan_ms += t_scan + t_off + t_scat + t_gath;
        stats->kernel_scan_launches += 1;
        stats->execute_time_ms = now_ms() - tw0;
    }
    if (timing)
        fprintf(stderr, "[ytql timing] scan+project compact: %d window(s), "
                        "%lld rows out, %lld pool bytes: scan %.3fms offsets "
                        "%.3fms scatter %.3fms gather %.3fms D2H+emit %.3fms\n",
                windows, (long long)output->row_count,
                (long long)output->string_pool_used, t_scan, t_off, t_scat,
                t_gath, t_host);
    return YT_OK;
}

/* scan + filter + project: order-preserving (MakeCodegenProjectOp +
 * WriteOpHelper, registry.cpp:1999-2047). The device writes per-row values
 * and a pass mask; the host compacts in row order. Plans with a STRING
 * projection take scan_project_compact instead. */
static int run_scan_project(const YtPlan* plan, const YtChunk* chunk,
                            const YtExecOptions* options, const DevPlan* dp,
                            StrPreds* sp,
                            const JoinDev* jd, const JoinDev* jd2,
                            YtRowset* output, YtStatistics* stats, double tw0,
                            char* errbuf, size_t errlen)
{
    int rc = YT_OK;
    DeviceRun R2;
    PoolScope ps;
    DevPlan dpl = *dp;      /* + this run's string-predicate bitmaps */
    R2.stream = (hipStream_t)(uintptr_t)options->stream;
    unsigned mw = 0;
    int in_clamped = 0;
    rc = setup_chunk(chunk, &R2, &mw, options->input_row_limit, &in_clamped,
                     errbuf, errlen);
    if (rc) return rc;
    rc = setup_string_preds(sp, &R2, &dpl, errbuf, errlen);
    if (rc) return rc;
    JoinDev jstr[2];        /* + this run's string-join maps */
    rc = setup_strjoin_maps(&R2, &jd, &jd2, jstr, errbuf, errlen);
    if (rc) return rc;
    dp = &dpl;
    (void)in_clamped;
    int64_t n = chunk->row_count;
    if (options->input_row_limit > 0 && options->input_row_limit < n)
        n = options->input_row_limit;
    output->row_count = 0;
    output->column_count = plan->project_count;
    if (const unsigned str_mask = string_proj_mask(dp)) {
        t_last_scan_path = YT_SCAN_PATH_PROJ_COMPACT;
        if (n == 0 || R2.nsegs == 0) return YT_OK;
        return scan_project_compact(plan, options, dp, &R2, n, str_mask, jd, jd2,
                                    output, stats, tw0, errbuf, errlen);
    }
    if (n == 0 || R2.nsegs == 0) return YT_OK;
    /* stream the scan through bounded windows: the per-row
     * materialization buffer is at most kWin rows, so arbitrarily
     * large inputs need only bounded device/host memory */
    const int64_t kWin = (int64_t)1 << 24;
    const int64_t win = n < kWin ? n : kWin;
    DevOutVal* d_out = nullptr;
    uint8_t* d_pass = nullptr;
    DevOutVal* h_out = nullptr;
    uint8_t* h_pass = nullptr;
    HIP_CHECK(ps.dev(&d_out, sizeof(DevOutVal) * win * plan->project_count));
    HIP_CHECK(ps.dev(&d_pass, (size_t)win));
    HIP_CHECK(ps.host(&h_out, sizeof(DevOutVal) * win * plan->project_count));
    HIP_CHECK(ps.host(&h_pass, (size_t)win));
    HIP_CHECK(hipMemsetAsync(R2.d_err, 0, sizeof(unsigned), R2.stream));
    float ms = 0;
    int np = plan->project_count;
    hipEvent_t e0 = nullptr, e1 = nullptr;      /* reused by every window */
    HIP_CHECK(ps.event(&e0));
    HIP_CHECK(ps.event(&e1));
    for (int64_t w0 = 0; w0 < n; w0 += win) {
        const int64_t wlen = (w0 + win <= n) ? win : (n - w0);
        HIP_CHECK(hipEventRecord(e0, R2.stream));
        HIP_CHECK(ytql_launch_scan_project(dp, R2.d_segs, R2.d_segex, R2.d_off,
                                           R2.d_cnt, w0, wlen, jd, jd2, d_out,
                                           d_pass, R2.d_err, R2.stream));
        HIP_CHECK(hipEventRecord(e1, R2.stream));
        HIP_CHECK(hipMemcpyAsync(h_out, d_out, sizeof(DevOutVal) * wlen * plan->project_count,
                                 hipMemcpyDeviceToHost, R2.stream));
        HIP_CHECK(hipMemcpyAsync(h_pass, d_pass, (size_t)wlen,
                                 hipMemcpyDeviceToHost, R2.stream));
        HIP_CHECK(hipStreamSynchronize(R2.stream));
        float wms = 0;
        HIP_CHECK(hipEventElapsedTime(&wms, e0, e1));
        ms += wms;
        unsigned kerr = 0;
        HIP_CHECK(hipMemcpy(&kerr, R2.d_err, sizeof(unsigned), hipMemcpyDeviceToHost));
        if (kerr) {
            set_err(errbuf, errlen, kerr == YT_ERR_DIV_ZERO ? "Division by zero" : "expression error");
            return (int)kerr;
        }
        for (int64_t r2 = 0; r2 < wlen; r2++) {
            if (!h_pass[r2]) continue;
            if (options->output_row_limit > 0 &&
                output->row_count >= options->output_row_limit) {
                if (stats) stats->incomplete_output = 1;
                break;
            }
            if (output->row_count >= output->capacity_rows) return YT_ERR_CAPACITY;
            YtValue* dst = output->values + output->row_count * np;
            for (int pj = 0; pj < np; pj++) {
                const DevOutVal& o = h_out[r2 * np + pj];
                dst[pj].id = (uint16_t)pj;
                dst[pj].type = (uint8_t)o.type;
                dst[pj].flags = 0;
                dst[pj].length = 0;
                dst[pj].data.bits = o.bits;
            }
            output->row_count++;
        }
        if (options->output_row_limit > 0 &&
            output->row_count >= options->output_row_limit)
            break;
    }
    if (stats) {
        stats->rows_read = n;
        stats->rows_written = output->row_count;
        stats->kernel_scan_ms += ms;
        stats->kernel_scan_launches += 1;
        stats->execute_time_ms = now_ms() - tw0;
    }
    return YT_OK;
}


/* general string path: emit [key(string), aggs...] rows from the compacted
 * key refs (hgroups: pool offset|len) and their aggregate records (haggs),
 * then the null-key side group; aggregates finalize through finalize_row
 * exactly as on the int-key paths. */
static int emit_string_general(const YtPlan* plan, const uint8_t* sum_type,
                               const OutStrGroup* hgroups,
                               const OutStrAgg* haggs, int64_t ngroups,
                               const char* pool, const TableHdr& th,
                               int64_t output_row_limit, int* out_limited,
                               YtRowset* output, char* errbuf, size_t errlen)
{
    const int ncols = 1 + plan->agg_count;
    uint8_t st[kMaxAggs];
    memcpy(st, sum_type, sizeof(st));
    for (int64_t gI = 0; gI < ngroups + 1; gI++) {
        const int knull = gI == ngroups;
        if (knull && !th.side_used[1]) break;
        if (output_row_limit > 0 && output->row_count >= output_row_limit) {
            *out_limited = 1;
            break;
        }
        if (output->row_count >= output->capacity_rows) {
            set_err(errbuf, errlen, "rowset too small");
            return YT_ERR_CAPACITY;
        }
        YtValue* dst = output->values + output->row_count * ncols;
        HVal row[kMaxAggs];
        int nrow = 0;
        if (knull) {
            /* side_agg interleaves {bits, nonnull} per aggregate */
            uint64_t ab[kMaxAggs], an[kMaxAggs];
            for (int a = 0; a < plan->agg_count; a++) {
                ab[a] = th.side_agg[1][2 * a];
                an[a] = th.side_agg[1][2 * a + 1];
            }
            finalize_row(plan, YT_VT_STRING, st, 0, 1, th.side_cnt[1], ab, an,
                         row, &nrow, 0);
            dst[0].type = YT_VT_NULL;
            dst[0].length = 0;
            dst[0].data.bits = 0;
        } else {
            const OutStrGroup& g = hgroups[gI];
            const uint32_t klen = (uint32_t)(g.off_len & 0xFFFFFF);
            finalize_row(plan, YT_VT_STRING, st, 0, 0, haggs[gI].cnt,
                         haggs[gI].agg_bits, haggs[gI].agg_nonnull, row, &nrow, 0);
            if (output->string_pool_used + klen > output->string_pool_capacity) {
                set_err(errbuf, errlen, "string pool too small");
                return YT_ERR_CAPACITY;
            }
            char* kdst = output->string_pool + output->string_pool_used;
            if (klen) memcpy(kdst, pool + (g.off_len >> 24), klen);
            dst[0].type = YT_VT_STRING;
            dst[0].length = klen;
            dst[0].data.str = kdst;
            output->string_pool_used += klen;
        }
        dst[0].id = 0;
        dst[0].flags = 0;
        for (int a = 0; a < nrow; a++) {
            YtValue& v = dst[1 + a];
            v.id = (uint16_t)(1 + a);
            v.type = row[a].type;
            v.flags = 0;
            v.length = 0;
            v.data.bits = row[a].bits;
        }
        output->row_count++;
    }
    return YT_OK;
}

/* one [key(string), aggs...] row of the specialised {sum, sum(1)} shape; a
 * key_type of YT_VT_NULL writes the null-key row */
static inline void write_str_sum_row(YtValue* dst, int agg_count,
                                     uint8_t key_type, uint32_t key_len,
                                     const char* key, uint64_t cnt,
                                     uint64_t nonnull, uint64_t sum_bits,
                                     const int* agg_is_sum1, int val_is_double)
{
    dst[0].id = 0;
    dst[0].type = key_type;
    dst[0].flags = 0;
    dst[0].length = key_len;
    if (key_type == YT_VT_STRING) dst[0].data.str = key;
    else dst[0].data.bits = 0;
    for (int a = 0; a < agg_count; a++) {
        YtValue& v = dst[1 + a];
        v.id = (uint16_t)(1 + a);
        v.flags = 0;
        v.length = 0;
        if (agg_is_sum1[a]) {
            v.type = YT_VT_INT64;
            v.data.bits = cnt;
        } else if (nonnull == 0) {
            v.type = YT_VT_NULL;
            v.data.bits = 0;
        } else {
            v.type = val_is_double ? YT_VT_DOUBLE : YT_VT_INT64;
            v.data.bits = sum_bits;
        }
    }
}

/* the null-key row of that shape, from the table header's side group */
static inline void write_str_sum_null_row(YtValue* dst, int agg_count,
                                          const TableHdr& th, int sum_slot,
                                          const int* agg_is_sum1,
                                          int val_is_double)
{
    write_str_sum_row(dst, agg_count, YT_VT_NULL, 0, nullptr, th.side_cnt[1],
                      sum_slot >= 0 ? th.side_agg[1][2 * sum_slot + 1] : 0,
                      sum_slot >= 0 ? th.side_agg[1][2 * sum_slot] : 0,
                      agg_is_sum1, val_is_double);
}

/* memcpy in 64 MB pieces, one thread each */
static void copy_parallel(char* dst, const char* src, size_t bytes)
{
    const int ct = (int)std::min<size_t>(std::thread::hardware_concurrency(),
                                         (bytes + (64 << 20) - 1) / (64 << 20));
    if (ct <= 1) {
        if (bytes) memcpy(dst, src, bytes);
        return;
    }
    ThreadJoiner cth;
    const size_t per = (bytes + ct - 1) / ct;
    for (int t = 0; t < ct; t++) {
        const size_t b = (size_t)t * per;
        const size_t e = std::min(bytes, b + per);
        if (b >= e) break;
        cth.ths.emplace_back([=] { memcpy(dst + b, src + b, e - b); });
    }
}

/* what run_string_group learns from the plan and the host-visible segment
 * meta before it touches the device */
struct StrGroupShape {
    bool general;
    int sum_slot, sum_col, val_is_double;
    uint8_t col_types[kMaxCols];
};

/* which of the two kernel sets the plan takes, and the refusals that need no
 * device; `partial` is the bottom query (the state row carries one sum) */
static int classify_string_group(const YtPlan* plan, const YtChunk* chunk,
                                 int key_col, bool partial, StrGroupShape* sh,
                                 char* errbuf, size_t errlen)
{
    sh->sum_slot = -1;
    sh->sum_col = -1;
    sh->val_is_double = 0;
    bool general = plan->filter != nullptr;
    memset(sh->col_types, YT_VT_INT64, sizeof(sh->col_types));
    for (int c = 0; c < chunk->column_count && c < kMaxCols; c++)
        sh->col_types[c] = (uint8_t)chunk->columns[c].value_type;
    for (int a = 0; a < plan->agg_count; a++) {
        int f = plan->aggs[a]->func;
        if (f == YT_AGG_SUM) {
            int c;
            if (sh->sum_slot >= 0) {
                if (partial) {
                    set_err(errbuf, errlen,
                            "partial_str: the string state row carries one sum");
                    return YT_ERR_UNSUPPORTED;
                }
                general = true;
                continue;
            }
            sh->sum_slot = a;
            if (expr_is_col(plan->aggs[a]->arg, &c) && c >= 0 &&
                c < chunk->column_count && c < kMaxCols) {
                sh->sum_col = c;
                sh->val_is_double = sh->col_types[c] == YT_VT_DOUBLE;
                if (!sh->val_is_double && sh->col_types[c] != YT_VT_INT64)
                    general = true;
            } else {
                general = true;     /* sum(<expression>) */
            }
        } else if (f != YT_AGG_SUM1) {
            if (partial) {
                set_err(errbuf, errlen,
                        "partial_str: min/max/avg/first are not exchanged for "
                        "string keys (the state row carries sum and sum(1))");
                return YT_ERR_UNSUPPORTED;
            }
            general = true;
        }
    }
    if (plan->project_count) {
        set_err(errbuf, errlen, "string keys: no post-projection this round");
        return YT_ERR_UNSUPPORTED;
    }
    /* key layout and segmentation decide too (host-visible segment meta) */
    const YtColumn& kcol = chunk->columns[key_col];
    for (int i = 0; i < kcol.segment_count; i++) {
        if (kcol.segments[i].type == YT_SEG_DIRECT_RLE) general = true;
        if (i + 1 < kcol.segment_count &&
            kcol.segments[i].row_count != kcol.segments[0].row_count)
            general = true;
    }
    if (!general && sh->sum_col >= 0) {
        const YtColumn& vcol = chunk->columns[sh->sum_col];
        if (vcol.segment_count != kcol.segment_count) general = true;
        for (int i = 0; !general && i < kcol.segment_count; i++)
            if (vcol.segments[i].row_count != kcol.segments[i].row_count)
                general = true;
    }
    sh->general = general;
    return YT_OK;
}

/* bottom query: hash-partition the compacted groups + the null side group
 * into state rows and per-partition pool slices (key_bits = slice-local
 * offset<<24 | len); *state_rows = rows written */
static int partition_string_groups(PoolScope& ps, StrPartialOut* po,
                                   hipStream_t stream, const OutStrGroup* d_out,
                                   int64_t ngroups, const char* d_pool,
                                   const TableHdr& th, int sum_slot,
                                   int val_is_double, int64_t* state_rows,
                                   char* errbuf, size_t errlen)
{
    const int np = po->partition_count;
    const int p_null = (int)(splitmix64_host(
        0xCBF29CE484222325ULL ^ 0xDEADBEEF12345678ULL) % (uint64_t)np);
    unsigned long long* d_pc = nullptr;   /* [np] counts, [np] bytes,
                                             [np] cursors, [np] bcursors,
                                             [np] pool_base */
    HIP_CHECK(ps.dev(&d_pc, sizeof(unsigned long long) * np * 5));
    HIP_CHECK(hipMemsetAsync(d_pc, 0, sizeof(unsigned long long) * np * 5,
                             stream));
    if (ngroups > 0) {
        HIP_CHECK(ytql_launch_strst_count(d_out, ngroups, d_pool, np,
                                          d_pc, d_pc + np, stream));
    }
    std::vector<unsigned long long> pc(2 * np);
    HIP_CHECK(hipMemcpyAsync(pc.data(), d_pc,
                             sizeof(unsigned long long) * 2 * np,
                             hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    if (th.side_used[1]) pc[p_null] += 1;
    unsigned long long rrun = 0, brun = 0;
    std::vector<unsigned long long> rcur(np), pbase(np);
    for (int p = 0; p < np; p++) {
        rcur[p] = rrun;
        pbase[p] = brun;
        rrun += pc[p];
        brun += pc[np + p];
    }
    if ((int64_t)rrun > po->capacity_rows
        || (int64_t)brun > po->pool_capacity) {
        set_err(errbuf, errlen, "partial_str: state/pool buffer too small");
        return YT_ERR_CAPACITY;
    }
    HIP_CHECK(hipMemcpyAsync(d_pc + 2 * np, rcur.data(),
                             sizeof(unsigned long long) * np,
                             hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemsetAsync(d_pc + 3 * np, 0,
                             sizeof(unsigned long long) * np, stream));
    HIP_CHECK(hipMemcpyAsync(d_pc + 4 * np, pbase.data(),
                             sizeof(unsigned long long) * np,
                             hipMemcpyHostToDevice, stream));
    if (ngroups > 0) {
        HIP_CHECK(ytql_launch_strst_scatter(d_out, ngroups, d_pool, np,
                                            val_is_double,
                                            d_pc + 2 * np, d_pc + 3 * np,
                                            po->states_device, po->pool_device,
                                            d_pc + 4 * np, stream));
    }
    HIP_CHECK(hipStreamSynchronize(stream));
    if (th.side_used[1]) {
        unsigned long long pos = 0;
        HIP_CHECK(hipMemcpy(&pos, d_pc + 2 * np + p_null,
                            sizeof(pos), hipMemcpyDeviceToHost));
        YtStateRow sr;
        memset(&sr, 0, sizeof(sr));
        sr.key_bits = 0;
        uint64_t nn = sum_slot >= 0 ? th.side_agg[1][2 * sum_slot + 1] : 0;
        sr.meta = 1ULL | (val_is_double ? 2ULL : 0ULL) | (nn << 8);
        sr.sum_bits = sum_slot >= 0 ? th.side_agg[1][2 * sum_slot] : 0;
        sr.row_count = th.side_cnt[1];
        HIP_CHECK(hipMemcpy(po->states_device + pos, &sr, sizeof(sr),
                            hipMemcpyHostToDevice));
    }
    for (int p = 0; p < np; p++) {
        po->part_counts[p] = (int64_t)pc[p];
        po->part_pool_bytes[p] = (int64_t)pc[np + p];
    }
    *state_rows = (int64_t)rrun;
    return YT_OK;
}

/* specialised path: emit [key(string), aggs...] rows from the compacted
 * groups in d_out and their key bytes in d_pool (pool_bytes of them), then
 * the null-key side group. hgroups is the pinned landing area for d_out. */
static int emit_string_sums(PoolScope& ps, const YtPlan* plan,
                            const YtExecOptions* options, hipStream_t stream,
                            const OutStrGroup* d_out, OutStrGroup* hgroups,
                            int64_t ngroups, const char* d_pool,
                            uint64_t pool_bytes, const TableHdr& th,
                            int sum_slot, int val_is_double, int* out_limited,
                            YtRowset* output, char* errbuf, size_t errlen)
{
    const int nagg = plan->agg_count;
    const int ncols = 1 + nagg;
    const int has_null_row = th.side_used[1] ? 1 : 0;
    int agg_is_sum1[kMaxAggs];
    for (int a = 0; a < nagg; a++)
        agg_is_sum1[a] = plan->aggs[a]->func == YT_AGG_SUM1;

    /* Fast path (no output limit, everything fits): copy the device key pool
     * wholesale — compact's pool_off values are global offsets into it — and
     * fill the YtValue rows with host threads. */
    if (options->output_row_limit == 0 &&
        ngroups + has_null_row <= output->capacity_rows &&
        pool_bytes <= (unsigned long long)output->string_pool_capacity &&
        (output->string_pool != nullptr || pool_bytes == 0)) {
        /* pipeline: pool D2H first, then hgroups in slices — the
         * parallel host copies/emits of slice s overlap slice s+1's
         * D2H (the serial tail was D2H then copy then emit) */
        char* stage = nullptr;
        if (pool_bytes) {
            HIP_CHECK(ps.host(&stage, pool_bytes));
            HIP_CHECK(hipMemcpyAsync(stage, d_pool, pool_bytes,
                                     hipMemcpyDeviceToHost, stream));
        }
        const int kSlices = (ngroups >= (1 << 21)) ? 8 : 1;
        std::vector<hipEvent_t> sl_ev(kSlices, nullptr);
        const int64_t per_sl = (ngroups + kSlices - 1) / kSlices;
        for (int s2 = 0; s2 < kSlices; s2++) {
            int64_t b = (int64_t)s2 * per_sl;
            int64_t e = std::min<int64_t>(ngroups, b + per_sl);
            if (b >= e) break;
            HIP_CHECK(hipMemcpyAsync(hgroups + b, d_out + b,
                                     sizeof(OutStrGroup) * (e - b),
                                     hipMemcpyDeviceToHost, stream));
            HIP_CHECK(ps.event(&sl_ev[s2]));
            HIP_CHECK(hipEventRecord(sl_ev[s2], stream));
        }
        ThreadJoiner tj;        /* before the checks that run beside threads */
        if (pool_bytes) {
            /* pool D2H was queued first — wait for the FIRST slice event
             * (>= pool completion), then copy to the caller's pool off
             * the critical path */
            hipEvent_t after_pool = sl_ev[0];
            if (!after_pool) {
                HIP_CHECK(hipStreamSynchronize(stream));
            }
            const size_t total_b = (size_t)pool_bytes;
            char* dst_pool = output->string_pool;
            tj.ths.emplace_back([stage, dst_pool, total_b, after_pool] {
                if (after_pool) (void)hipEventSynchronize(after_pool);
                copy_parallel(dst_pool, stage, total_b);
            });
        }
        output->string_pool_used = pool_bytes;
        auto emit_range = [&](int64_t b, int64_t e) {
            for (int64_t gI = b; gI < e; gI++) {
                const OutStrGroup& g = hgroups[gI];
                write_str_sum_row(output->values + gI * ncols, nagg,
                                  YT_VT_STRING, (uint32_t)(g.off_len & 0xFFFFFF),
                                  output->string_pool + (g.off_len >> 24),
                                  g.cnt_nonnull & 0xFFFFFFFFULL,
                                  g.cnt_nonnull >> 32, g.sum_bits,
                                  agg_is_sum1, val_is_double);
            }
        };
        int nt = (int)std::thread::hardware_concurrency();
        if (nt < 1) nt = 1;
        if (nt > 64) nt = 64;
        if (ngroups < (1 << 16)) nt = 1;
        for (int s2 = 0; s2 < kSlices; s2++) {
            int64_t sb = (int64_t)s2 * per_sl;
            int64_t se = std::min<int64_t>(ngroups, sb + per_sl);
            if (sb >= se) break;
            if (sl_ev[s2]) HIP_CHECK(hipEventSynchronize(sl_ev[s2]));
            if (nt == 1) {
                emit_range(sb, se);
                continue;
            }
            int kt = nt / kSlices > 0 ? nt / kSlices : 1;
            int64_t per = (se - sb + kt - 1) / kt;
            for (int t = 0; t < kt; t++) {
                int64_t b = sb + (int64_t)t * per, e = b + per;
                if (b >= se) break;
                if (e > se) e = se;
                tj.ths.emplace_back(emit_range, b, e);
            }
        }
        tj.join();
        output->row_count = ngroups;
        if (has_null_row) {
            write_str_sum_null_row(output->values + output->row_count * ncols,
                                   nagg, th, sum_slot, agg_is_sum1, val_is_double);
            output->row_count++;
        }
        return YT_OK;
    }

    /* limited path: output_row_limit, or a rowset or pool that may be too
     * small — one copy each of the pool and the groups, rows one by one */
    std::vector<char> pool(pool_bytes ? pool_bytes : 1);
    if (pool_bytes) {
        HIP_CHECK(hipMemcpy(pool.data(), d_pool, pool_bytes, hipMemcpyDeviceToHost));
    }
    if (ngroups > 0) {
        HIP_CHECK(hipMemcpy(hgroups, d_out, sizeof(OutStrGroup) * ngroups,
                            hipMemcpyDeviceToHost));
    }
    for (int64_t gI = 0; gI < ngroups + 1; gI++) {
        const int knull = gI == ngroups;
        if (knull && !has_null_row) break;
        if (options->output_row_limit > 0 &&
            output->row_count >= options->output_row_limit) {
            *out_limited = 1;
            break;
        }
        if (output->row_count >= output->capacity_rows) return YT_ERR_CAPACITY;
        YtValue* dst = output->values + output->row_count * ncols;
        if (knull) {
            write_str_sum_null_row(dst, nagg, th, sum_slot, agg_is_sum1,
                                   val_is_double);
        } else {
            const OutStrGroup& g = hgroups[gI];
            const uint32_t klen = (uint32_t)(g.off_len & 0xFFFFFF);
            if (output->string_pool_used + klen > output->string_pool_capacity) {
                set_err(errbuf, errlen, "string pool too small");
                return YT_ERR_CAPACITY;
            }
            char* kdst = output->string_pool + output->string_pool_used;
            memcpy(kdst, pool.data() + (g.off_len >> 24), klen);
            write_str_sum_row(dst, nagg, YT_VT_STRING, klen, kdst,
                              g.cnt_nonnull & 0xFFFFFFFFULL, g.cnt_nonnull >> 32,
                              g.sum_bits, agg_is_sum1, val_is_double);
            output->string_pool_used += klen;
        }
        output->row_count++;
    }
    return YT_OK;
}

/* string-keyed GROUP BY (config-5 family). Dense per-segment dictionary-id
 * accumulators, then an exact cross-segment merge (hash gate + byte
 * compare), then device-side key materialization into the caller's string
 * pool. Two kernel sets share that pipeline:
 *  - the specialised one (YT_SCAN_PATH_STR_DENSE): no filter, at most one
 *    sum over a plain int64/double column plus sum(1)s, uniform key
 *    segments that the value column shares, no DirectRle key segment;
 *  - the general one (YT_SCAN_PATH_STR_GENERAL): everything else — filter,
 *    min/max/avg/first, expression arguments, ragged segmentation, DirectRle
 *    keys (k_strgen_* in kernels.hip). */
static int run_string_group(const YtPlan* plan, const YtChunk* chunk,
                            const YtExecOptions* options, int key_col,
                            YtRowset* output, YtStatistics* stats, double tw0,
                            char* errbuf, size_t errlen,
                            StrPartialOut* po = nullptr)
{
    StrGroupShape sh;
    int rc = classify_string_group(plan, chunk, key_col, po != nullptr, &sh,
                                   errbuf, errlen);
    if (rc) return rc;
    const bool general = sh.general;
    const int sum_slot = sh.sum_slot, sum_col = sh.sum_col;
    int val_is_double = sh.val_is_double;
    DevPlan dp;
    StrPreds SP;
    uint8_t sum_type[kMaxAggs];
    if (general) {
        /* the interpreter's plan: compiles filter + aggregate arguments and
         * carries its refusals (string columns in expressions, avg + WITH
         * TOTALS, more than kMaxAggs aggregates, ...) */
        rc = build_devplan(plan, chunk, &dp, &SP, errbuf, errlen);
        if (rc) return rc;
        for (int a = 0; a < plan->agg_count; a++) {
            sum_type[a] = (plan->aggs[a]->func != YT_AGG_SUM1)
                ? expr_static_type(plan->aggs[a]->arg, sh.col_types)
                : (uint8_t)YT_VT_INT64;
            if (sum_type[a] == YT_VT_NULL) sum_type[a] = YT_VT_INT64;
        }
        if (sum_slot >= 0) {
            val_is_double = sum_type[sum_slot] == YT_VT_DOUBLE;
            if (po && !val_is_double && sum_type[sum_slot] != YT_VT_INT64) {
                set_err(errbuf, errlen,
                        "partial_str: the string state row carries an int64 "
                        "or double sum");
                return YT_ERR_UNSUPPORTED;
            }
        }
    } else {
        /* no program to compile; HAVING still runs on the host */
        rc = check_plan_types(plan, sh.col_types,
                              std::min(chunk->column_count, kMaxCols),
                              errbuf, errlen);
        if (rc) return rc;
    }
    t_last_scan_path = general ? YT_SCAN_PATH_STR_GENERAL : YT_SCAN_PATH_STR_DENSE;

    DeviceRun R;
    PoolScope ps;
    R.stream = (hipStream_t)(uintptr_t)options->stream;
    unsigned mw = 0;
    int in_clamped = 0;
    rc = setup_chunk(chunk, &R, &mw, options->input_row_limit, &in_clamped,
                     errbuf, errlen);
    if (rc) return rc;
    if (output) {
        output->row_count = 0;
        output->string_pool_used = 0;   /* rowsets reusable across queries */
        output->column_count = 1 + plan->agg_count;
    }
    if (chunk->row_count == 0 || R.nsegs == 0) {
        if (po) {
            for (int p = 0; p < po->partition_count; p++) {
                po->part_counts[p] = 0;
                po->part_pool_bytes[p] = 0;
            }
        }
        return YT_OK;
    }
    rc = setup_table(&R, plan->agg_count, options->max_groups_hint,
                     options->group_row_limit, errbuf, errlen);
    if (rc) return rc;
    if (general) {
        rc = setup_string_preds(&SP, &R, &dp, errbuf, errlen);
        if (rc) return rc;
    }

    /* read back the parsed key-column segments: dictionary sizes + layout */
    const int knseg = R.h_cnt[key_col];
    const int koff = R.h_off[key_col];
    std::vector<SegEx> ksegex(knseg);
    TableHdr th;
    int64_t total_dict = 0;
    HIP_CHECK(hipMemcpy(ksegex.data(), R.d_segex + koff,
                        sizeof(SegEx) * knseg, hipMemcpyDeviceToHost));
    for (int i = 0; i < knseg; i++) {
        if (!(ksegex[i].flags & (general ? (8 | 32 | 64) : (8 | 32)))) {
            set_err(errbuf, errlen, "string keys: unknown key segment layout");
            return YT_ERR_UNSUPPORTED;
        }
    }
    const int32_t rows0 = R.h_segs[koff].row_count;
    /* accumulator record: {cnt|nonnull<<32, sum} on the specialised
     * path, {rows, {bits, nonnull} per aggregate} on the general one */
    const int acc_stride = general ? 1 + 2 * plan->agg_count : 2;
    /* rows actually scanned (input_row_limit clamps the segment list) */
    const int64_t scan_rows = R.h_segs[koff + knseg - 1].start_row
                            + R.h_segs[koff + knseg - 1].row_count;
    if (general && po && scan_rows >= ((int64_t)1 << 32)) {
        set_err(errbuf, errlen, "partial_str: chunk too large (2^32 rows)");
        return YT_ERR_UNSUPPORTED;
    }

    std::vector<int64_t> acc_base(knseg + 1);
    for (int i = 0; i < knseg; i++) {
        acc_base[i] = total_dict;
        total_dict += ksegex[i].dict_size;
    }
    acc_base[knseg] = total_dict;

    StrGroupParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.key_seg_off = koff;
    sp.key_seg_cnt = knseg;
    sp.val_seg_off = sum_col >= 0 ? R.h_off[sum_col] : -1;
    sp.val_seg_cnt = sum_col >= 0 ? R.h_cnt[sum_col] : 0;
    sp.val_is_double = val_is_double;
    sp.sum_slot = sum_slot;
    sp.agg_count = plan->agg_count;
    sp.has_val_nulls = sum_col >= 0 && (R.col_null_flags[sum_col] != 0);
    sp.tile_rows = 8192;
    if (sp.tile_rows > rows0) sp.tile_rows = rows0 > 256 ? rows0 : 256;
    sp.tiles_per_seg = (rows0 + sp.tile_rows - 1) / sp.tile_rows;
    const int32_t last_rows = R.h_segs[koff + knseg - 1].row_count;
    sp.ntiles = (knseg - 1) * sp.tiles_per_seg
              + (last_rows + sp.tile_rows - 1) / sp.tile_rows;
    sp.row_count = chunk->row_count;

    int64_t* d_accbase = nullptr;
    unsigned long long* d_acc = nullptr;
    uint64_t* d_hashes = nullptr;
    StrSlot* d_slots = nullptr;
    HIP_CHECK(ps.dev(&d_accbase, sizeof(int64_t) * (knseg + 1)));
    HIP_CHECK(hipMemcpyAsync(d_accbase, acc_base.data(),
                             sizeof(int64_t) * (knseg + 1),
                             hipMemcpyHostToDevice, R.stream));
    HIP_CHECK(ps.dev(&d_acc, sizeof(uint64_t) * acc_stride * (total_dict ? total_dict : 1)));
    HIP_CHECK(hipMemsetAsync(d_acc, 0, sizeof(uint64_t) * acc_stride * (total_dict ? total_dict : 1), R.stream));
    HIP_CHECK(ps.dev(&d_hashes, sizeof(uint64_t) * (total_dict ? total_dict : 1)));
    /* per-entry identity + prefix arrays: filled by the hash kernel so
     * the merge's hot path reads them as a stream */
    uint64_t* d_idents = nullptr;
    ulonglong2* d_pfxs = nullptr;
    HIP_CHECK(ps.dev(&d_idents, sizeof(uint64_t) * (total_dict ? total_dict : 1)));
    HIP_CHECK(ps.dev(&d_pfxs, sizeof(ulonglong2) * (total_dict ? total_dict : 1)));
    /* Table sized for the worst case (every dict entry distinct).
     * Measured: an 8×-smaller table holding just the ~6 M live keys is
     * NOT faster — the merge's scattered atomics then fight over hot
     * cachelines across XCDs (59 ms vs 47 ms at 86 M entries), while
     * the oversized cold table costs only compact-scan time, which the
     * two-pass compact already made cheap. The grow-on-overflow loop
     * below is kept as a safety net (never triggers at this size). */
    uint64_t nslots_cap = next_pow2((uint64_t)(total_dict ? total_dict : 1) * 2);
    if (nslots_cap < 2048) nslots_cap = 2048;
    /* Start smaller than the every-entry-distinct worst case: the 64 B/slot
     * table is memset before the merge and scanned by the compact, so an
     * oversized table costs real milliseconds per step. With a caller
     * hint, kSlotsPerHintedGroup x the hint; otherwise half the entry count
     * (cross-segment duplication >= 2x in any chunk where a GROUP BY is the
     * right plan). The grow-on-overflow loop below keeps correctness for
     * adversarial cardinalities (one 4x retry reaches 2x entries). */
    constexpr uint64_t kSlotsPerHintedGroup = 4;
    uint64_t nslots = options->max_groups_hint > 0
        ? next_pow2((uint64_t)options->max_groups_hint * kSlotsPerHintedGroup)
        : next_pow2((uint64_t)(total_dict ? total_dict : 1) / 2 + 1);
    if (nslots < 2048) nslots = 2048;
    if (nslots > nslots_cap) nslots = nslots_cap;
    HIP_CHECK(ps.dev(&d_slots, sizeof(StrSlot) * nslots));
    HIP_CHECK(hipMemsetAsync(d_slots, 0, sizeof(StrSlot) * nslots, R.stream));
    /* general path: one aggregate record per slot, beside the slot table
     * (the slot line itself stays 64 B) */
    unsigned long long* d_slotaggs = nullptr;
    OutStrAgg* d_oaggs = nullptr;
    OutStrAgg* haggs = nullptr;
    StrGenAggs ag;
    memset(&ag, 0, sizeof(ag));
    if (general) {
        ag.count = plan->agg_count;
        for (int a = 0; a < plan->agg_count; a++) {
            ag.func[a] = plan->aggs[a]->func;
            ag.is_double[a] = sum_type[a] == YT_VT_DOUBLE;
        }
        HIP_CHECK(ps.dev(&d_slotaggs, sizeof(uint64_t) * acc_stride * nslots));
        HIP_CHECK(hipMemsetAsync(d_slotaggs, 0,
                                 sizeof(uint64_t) * acc_stride * nslots, R.stream));
    }

    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, ea = nullptr, eh = nullptr;
    HIP_CHECK(ps.event(&e0));
    HIP_CHECK(ps.event(&e1));
    HIP_CHECK(ps.event(&e2));
    HIP_CHECK(ps.event(&ea));
    HIP_CHECK(ps.event(&eh));
    HIP_CHECK(hipEventRecord(e0, R.stream));
    if (general) {
        HIP_CHECK(ytql_launch_strgen_accum(&dp, R.d_segs, R.d_segex, R.d_off,
                                           R.d_cnt, key_col, scan_rows,
                                           d_accbase, d_acc, R.d_th, R.d_err,
                                           R.stream));
    } else {
        HIP_CHECK(ytql_launch_strgrp_accum(&sp, R.d_segs, R.d_segex, d_accbase,
                                           d_acc, R.d_th, R.stream));
    }
    HIP_CHECK(hipEventRecord(ea, R.stream));
    HIP_CHECK(ytql_launch_strgrp_hash(R.d_segs, R.d_segex, koff, knseg,
                                      d_accbase, d_hashes, d_idents, d_pfxs,
                                      total_dict, R.stream));
    HIP_CHECK(hipEventRecord(eh, R.stream));
    for (;;) {
        if (general) {
            HIP_CHECK(ytql_launch_strgen_merge(R.d_segs, R.d_segex, koff, knseg,
                                               d_accbase, d_acc, &ag, d_hashes,
                                               d_idents, d_pfxs, d_slots, nslots,
                                               d_slotaggs, R.d_th, total_dict,
                                               R.stream));
        } else {
            HIP_CHECK(ytql_launch_strgrp_merge(R.d_segs, R.d_segex, koff, knseg,
                                               d_accbase, d_acc, d_hashes,
                                               d_idents, d_pfxs,
                                               d_slots, nslots, val_is_double,
                                               R.d_th, total_dict, R.stream));
        }
        HIP_CHECK(hipMemcpy(&th, R.d_th, sizeof(th), hipMemcpyDeviceToHost));
        if (th.overflow != 1 || nslots >= nslots_cap) break;
        ps.release(d_slots);
        d_slots = nullptr;
        nslots *= 4;
        if (nslots > nslots_cap) nslots = nslots_cap;
        HIP_CHECK(ps.dev(&d_slots, sizeof(StrSlot) * nslots));
        HIP_CHECK(hipMemsetAsync(d_slots, 0, sizeof(StrSlot) * nslots, R.stream));
        if (general) {
            ps.release(d_slotaggs);
            d_slotaggs = nullptr;
            HIP_CHECK(ps.dev(&d_slotaggs, sizeof(uint64_t) * acc_stride * nslots));
            HIP_CHECK(hipMemsetAsync(d_slotaggs, 0,
                                     sizeof(uint64_t) * acc_stride * nslots,
                                     R.stream));
        }
        th.ngroups = 0;
        th.overflow = 0;
        HIP_CHECK(hipMemcpy(R.d_th, &th, sizeof(th), hipMemcpyHostToDevice));
    }
    HIP_CHECK(hipEventRecord(e1, R.stream));
    if (general) {
        /* expression errors raised by the accumulate kernel */
        unsigned kerr = 0;
        HIP_CHECK(hipMemcpy(&kerr, R.d_err, sizeof(unsigned), hipMemcpyDeviceToHost));
        if (kerr) {
            set_err(errbuf, errlen, kerr == YT_ERR_DIV_ZERO
                    ? "Division by zero" : "expression error");
            return (int)kerr;
        }
    }

    /* compact + materialize keys into a device pool */
    const int64_t ngroups = (int64_t)th.ngroups;
    uint64_t pool_cap = 0;
    for (int i = 0; i < knseg; i++) {
        /* dictionary blob bytes upper-bound the key bytes */
        pool_cap += (uint64_t)R.h_segs[koff + i].blob_bytes;
    }
    if (pool_cap < 1024) pool_cap = 1024;
    OutStrGroup* d_out = nullptr;
    char* d_pool = nullptr;
    unsigned long long* d_ctr = nullptr;
    HIP_CHECK(ps.dev(&d_out, sizeof(OutStrGroup) * (ngroups ? ngroups : 1)));
    HIP_CHECK(ps.dev(&d_pool, pool_cap));
    HIP_CHECK(ps.dev(&d_ctr, 2 * sizeof(unsigned long long)));
    HIP_CHECK(hipMemsetAsync(d_ctr, 0, 2 * sizeof(unsigned long long), R.stream));
    if (ngroups > 0) {
        HIP_CHECK(ytql_launch_strgrp_compact(R.d_segs, R.d_segex, koff,
                                             d_slots, nslots, d_out, d_ctr,
                                             d_pool, d_ctr + 1, pool_cap,
                                             R.d_th, R.stream));
    }
    if (general) {
        /* compact copied each slot's index (left in StrSlot.sum_bits by
         * the merge) into OutStrGroup.sum_bits: gather the aggregate
         * records in group order. The bottom query also packs them back
         * into the {sum, cnt|nonnull} form the partition kernels read —
         * 32-bit halves, so it needs the chunk below 2^32 rows. */
        HIP_CHECK(ps.dev(&d_oaggs, sizeof(OutStrAgg) * (ngroups ? ngroups : 1)));
        HIP_CHECK(ps.host(&haggs, sizeof(OutStrAgg) * (ngroups ? ngroups : 1)));
        if (ngroups > 0) {
            HIP_CHECK(ytql_launch_strgen_gather(d_out, ngroups, d_slotaggs,
                                                nslots, plan->agg_count,
                                                d_oaggs, po ? 1 : 0, sum_slot,
                                                R.stream));
            HIP_CHECK(hipMemcpyAsync(haggs, d_oaggs, sizeof(OutStrAgg) * ngroups,
                                     hipMemcpyDeviceToHost, R.stream));
        }
    }
    OutStrGroup* hgroups = nullptr;
    HIP_CHECK(ps.host(&hgroups, sizeof(OutStrGroup) * (ngroups ? ngroups : 1)));
    unsigned long long hctr[2] = {0, 0};
    /* the fast emit path streams hgroups in SLICES so the host emit
     * overlaps the remaining D2H; the limited path copies in one go */
    HIP_CHECK(hipMemcpyAsync(hctr, d_ctr, 2 * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, R.stream));
    HIP_CHECK(hipEventRecord(e2, R.stream));
    HIP_CHECK(hipStreamSynchronize(R.stream));
    float ms = 0, ms_other = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    HIP_CHECK(hipEventElapsedTime(&ms_other, e1, e2));
    if (getenv("YTQL_TIMING")) {
        float ms_acc = 0, ms_hash = 0;
        HIP_CHECK(hipEventElapsedTime(&ms_acc, e0, ea));
        HIP_CHECK(hipEventElapsedTime(&ms_hash, ea, eh));
        fprintf(stderr, "[ytql timing] strgrp%s: accum %.2fms hash %.2fms "
                "merge %.2fms compact+D2H %.2fms\n",
                general ? " (general)" : "",
                ms_acc, ms_hash, ms - ms_acc - ms_hash, ms_other);
    }
    HIP_CHECK(hipMemcpy(&th, R.d_th, sizeof(th), hipMemcpyDeviceToHost));
    if (th.overflow == 1) {
        set_err(errbuf, errlen, "string merge table/pool overflow");
        return YT_ERR_CAPACITY;
    }

    if (po) {
        int64_t state_rows = 0;
        rc = partition_string_groups(ps, po, R.stream, d_out, ngroups, d_pool,
                                     th, sum_slot, val_is_double, &state_rows,
                                     errbuf, errlen);
        if (rc) return rc;
        if (stats) {
            stats->rows_read = chunk->row_count;
            stats->grouped_row_count = state_rows;
            stats->incomplete_input = in_clamped;
            stats->incomplete_output = (th.overflow == 2);
            stats->kernel_scan_ms += ms;
            stats->kernel_scan_launches += 1;
            stats->kernel_other_ms += ms_other;
            stats->execute_time_ms = now_ms() - tw0;
        }
        return YT_OK;
    }

    int out_limited = 0;
    if (general) {
        std::vector<char> pool(hctr[1] ? hctr[1] : 1);
        if (hctr[1]) {
            HIP_CHECK(hipMemcpy(pool.data(), d_pool, hctr[1], hipMemcpyDeviceToHost));
        }
        if (ngroups > 0) {
            HIP_CHECK(hipMemcpy(hgroups, d_out, sizeof(OutStrGroup) * ngroups,
                                hipMemcpyDeviceToHost));
        }
        rc = emit_string_general(plan, sum_type, hgroups, haggs, ngroups,
                                 pool.data(), th, options->output_row_limit,
                                 &out_limited, output, errbuf, errlen);
    } else {
        rc = emit_string_sums(ps, plan, options, R.stream, d_out, hgroups,
                              ngroups, d_pool, hctr[1], th, sum_slot,
                              val_is_double, &out_limited, output, errbuf, errlen);
    }
    if (stats) {
        stats->rows_read = chunk->row_count;
        stats->rows_written = output->row_count;
        stats->grouped_row_count = ngroups + (th.side_used[1] ? 1 : 0);
        stats->incomplete_input = in_clamped;
        stats->incomplete_output = out_limited || (th.overflow == 2);
        stats->kernel_scan_ms += ms;
        stats->kernel_scan_launches += 1;
        stats->kernel_other_ms += ms_other;   /* compact + result D2H */
        stats->execute_time_ms = now_ms() - tw0;
    }
    return rc;
}

/* ------------------------------------------------------------------ */
/* public entries                                                      */

extern "C" int yt_gpu_versioned_read(
    const YtVersionedColumn* col, uint64_t timestamp,
    uint64_t* out_bits, uint8_t* out_null, uint8_t* out_visible,
    uint8_t* out_agg, uint64_t stream, char* errbuf, size_t errlen)
{
    int rc = yt_gpu_available(errbuf, errlen);
    if (rc != YT_OK) return rc;
    hipStream_t st = (hipStream_t)(uintptr_t)stream;
    int nseg = col->ts_seg_count;
    if (nseg == 0) return YT_OK;
    if (col->val_seg_count != nseg) {
        set_err(errbuf, errlen, "versioned: segment count mismatch");
        return YT_ERR_INVALID_CHUNK;
    }
    std::vector<VSegDev> h_segs((size_t)nseg);
    PoolScope ps;
    int64_t total_rows = 0;
    for (int i = 0; i < nseg; i++) {
        const YtTimestampSeg& T = col->ts_segs[i];
        const YtVersionedValueSeg& V = col->val_segs[i];
        char* d_t = nullptr;
        char* d_v = nullptr;
        /* +8 pad: bp_gl may read one word past the last vector */
        HIP_CHECK(ps.dev(&d_t, (size_t)T.data_size + 8));
        HIP_CHECK(ps.dev(&d_v, (size_t)V.data_size + 8));
        HIP_CHECK(hipMemcpyAsync(d_t, T.data, (size_t)T.data_size,
                                 hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_v, V.data, (size_t)V.data_size,
                                 hipMemcpyHostToDevice, st));
        VSegDev& S = h_segs[i];
        S.row_start = total_rows;
        S.row_count = T.row_count;
        S.base_timestamp = T.base_timestamp;
        S.exp_w = T.expected_writes_per_row;
        S.exp_d = T.expected_deletes_per_row;
        S.exp_v = V.expected_values_per_row;
        S.vtype = V.type;
        S.vflags = V.flags;
        S.base_value = V.base_value;
        S.ts_data = d_t;
        S.val_data = d_v;
        total_rows += T.row_count;
    }
    VSegDev* d_segs = nullptr;
    HIP_CHECK(ps.dev(&d_segs, sizeof(VSegDev) * nseg));
    HIP_CHECK(hipMemcpyAsync(d_segs, h_segs.data(), sizeof(VSegDev) * nseg,
                             hipMemcpyHostToDevice, st));
    HIP_CHECK(ytql_launch_versioned_read(d_segs, nseg, total_rows,
                                         timestamp, out_bits, out_null,
                                         out_visible, out_agg, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return YT_OK;
}

namespace {
struct ScanChunkHandle {
    char* blob = nullptr;              /* device */
    YtSegment* segs = nullptr;         /* host heap */
    YtColumn* col = nullptr;           /* host heap */

    /* the blob is the pool's: yt_gpu_scan_chunk_free puts it back */
    ~ScanChunkHandle() { free(segs); free(col); }
};
} /* namespace */

extern "C" int yt_gpu_versioned_scan_table(
    const YtVersionedColumn* const* vcols, int nvcols,
    const YtChunk* key_chunk, uint64_t timestamp,
    YtChunk* out_chunk, void** out_handle,
    uint64_t stream, char* errbuf, size_t errlen);

extern "C" int yt_gpu_versioned_scan_chunk(
    const YtVersionedColumn* col, uint64_t timestamp,
    YtChunk* out_chunk, void** out_handle,
    uint64_t stream, char* errbuf, size_t errlen)
{
    /* single-column case of the table bridge below */
    const YtVersionedColumn* arr[1] = { col };
    return yt_gpu_versioned_scan_table(arr, 1, nullptr, timestamp,
                                       out_chunk, out_handle, stream,
                                       errbuf, errlen);
}

/* Versioned TABLE bridge: N versioned value
 * columns sharing one timestamp layout + optional unversioned KEY columns
 * (keys in the scan format are plain unversioned segments —
 * rowset_builder.cpp key readers), read at T and compacted into one
 * device-resident unversioned chunk [keys..., values...] that
 * yt_gpu_query_execute scans directly. Int64 and double value columns. */
extern "C" int yt_gpu_versioned_scan_table(
    const YtVersionedColumn* const* vcols, int nvcols,
    const YtChunk* key_chunk, uint64_t timestamp,
    YtChunk* out_chunk, void** out_handle,
    uint64_t stream, char* errbuf, size_t errlen)
{
    int rc = yt_gpu_available(errbuf, errlen);
    if (rc != YT_OK) return rc;
    hipStream_t st = (hipStream_t)(uintptr_t)stream;
    memset(out_chunk, 0, sizeof(*out_chunk));
    *out_handle = nullptr;
    if (nvcols < 1 || !vcols) { set_err(errbuf, errlen, "scan_table: need >=1 versioned column"); return YT_ERR_INVALID_PLAN; }

    int64_t n = 0;
    for (int i = 0; i < vcols[0]->ts_seg_count; i++)
        n += vcols[0]->ts_segs[i].row_count;
    for (int j = 1; j < nvcols; j++) {
        int64_t nj = 0;
        for (int i = 0; i < vcols[j]->ts_seg_count; i++)
            nj += vcols[j]->ts_segs[i].row_count;
        if (nj != n) { set_err(errbuf, errlen, "scan_table: column row counts differ"); return YT_ERR_INVALID_CHUNK; }
    }
    const int nkey = key_chunk ? key_chunk->column_count : 0;
    if (key_chunk && key_chunk->row_count != n) {
        set_err(errbuf, errlen, "scan_table: key chunk row count differs");
        return YT_ERR_INVALID_CHUNK;
    }
    for (int c = 0; c < nkey; c++) {
        if (key_chunk->columns[c].value_type != YT_VT_INT64) {
            set_err(errbuf, errlen, "scan_table: int64 key columns this round");
            return YT_ERR_UNSUPPORTED;
        }
    }
    for (int j = 0; j < nvcols; j++) {
        for (int i = 0; i < vcols[j]->val_seg_count; i++) {
            if (vcols[j]->val_segs[i].type >= YT_VSEG_STR_DIRECT_DENSE) {
                set_err(errbuf, errlen,
                        "scan_table: versioned string value columns are "
                        "readable (yt_gpu_versioned_read) but not yet "
                        "bridged into engine chunks");
                return YT_ERR_UNSUPPORTED;
            }
        }
    }
    const int ncols = nkey + nvcols;

    std::unique_ptr<ScanChunkHandle> H(new ScanChunkHandle());
    PoolScope ps;
    std::vector<uint64_t*> d_bits(ncols, nullptr);
    std::vector<uint8_t*> d_null(ncols, nullptr);
    uint8_t* d_vis = nullptr;
    uint8_t* d_vis2 = nullptr;
    unsigned long long* d_blk = nullptr;
    int64_t* d_off = nullptr;
    const int64_t kSegCap = 128 * 1024;
    int grid = (int)((n + 255) / 256);
    if (grid > 2048) grid = 2048;
    if (grid < 1) grid = 1;
    std::vector<int> col_is_dbl(ncols, 0);
    std::vector<unsigned long long> blk((size_t)grid);
    std::vector<int64_t> seg_rows, seg_bytes;
    int64_t total = 0, col_bytes = 0, blob_bytes = 0;
    int nseg = 0;
    if (n == 0) { *out_handle = H.release(); return YT_OK; }

    for (int c = 0; c < ncols; c++) {
        HIP_CHECK(ps.dev(&d_bits[c], sizeof(uint64_t) * n));
        HIP_CHECK(ps.dev(&d_null[c], (size_t)n));
    }
    HIP_CHECK(ps.dev(&d_vis, (size_t)n));
    HIP_CHECK(ps.dev(&d_vis2, (size_t)n));
    HIP_CHECK(ps.dev(&d_blk, sizeof(unsigned long long) * grid));

    /* key columns: decode unversioned DirectDense int64 */
    if (nkey) {
        DeviceRun R2;
        R2.stream = st;
        unsigned maxw = 0;
        int clamped = 0;
        rc = setup_chunk(key_chunk, &R2, &maxw, 0, &clamped, errbuf, errlen);
        if (rc != YT_OK) return rc;
        HIP_CHECK(hipMemsetAsync(R2.d_err, 0, sizeof(unsigned), st));
        for (int c = 0; c < nkey; c++) {
            HIP_CHECK(ytql_launch_unvcol_to_arrays(R2.d_segs, R2.d_segex,
                                                   R2.h_off[c], R2.h_cnt[c], n,
                                                   d_bits[c], d_null[c],
                                                   R2.d_err, st));
        }
        unsigned kerr = 0;
        HIP_CHECK(hipMemcpy(&kerr, R2.d_err, sizeof(unsigned), hipMemcpyDeviceToHost));
        if (kerr) {
            set_err(errbuf, errlen, "scan_table: string key columns not bridged this round");
            return YT_ERR_UNSUPPORTED;
        }
    }
    /* value columns: read at T (col 0 supplies the visibility mask — the
     * write/delete timestamp lists are row-level, shared by every column) */
    for (int j = 0; j < nvcols; j++) {
        const YtVersionedColumn* vc = vcols[j];
        int dbl = 0;
        for (int i = 0; i < vc->val_seg_count; i++)
            if (vc->val_segs[i].type >= YT_VSEG_DOUBLE_DENSE) dbl = 1;
        col_is_dbl[nkey + j] = dbl;
        rc = yt_gpu_versioned_read(vc, timestamp, d_bits[nkey + j],
                                   d_null[nkey + j], j == 0 ? d_vis : d_vis2,
                                   nullptr, stream, errbuf, errlen);
        if (rc != YT_OK) return rc;
    }

    HIP_CHECK(ytql_launch_vis_count(d_vis, n, d_blk, grid, st));
    HIP_CHECK(hipMemcpy(blk.data(), d_blk, sizeof(unsigned long long) * grid,
                        hipMemcpyDeviceToHost));
    {
        unsigned long long run = 0;
        for (int i = 0; i < grid; i++) { unsigned long long c = blk[i]; blk[i] = run; run += c; }
        total = (int64_t)run;
    }
    nseg = (int)((total + kSegCap - 1) / kSegCap);
    if (total == 0) {
        *out_handle = H.release();
        return YT_OK;
    }
    HIP_CHECK(hipMemcpyAsync(d_blk, blk.data(), sizeof(unsigned long long) * grid,
                             hipMemcpyHostToDevice, st));

    /* one blob: per column, per segment [header][values w64][null bitmap] */
    seg_rows.resize(nseg);
    seg_bytes.resize(nseg);
    for (int i = 0; i < nseg; i++) {
        seg_rows[i] = i + 1 < nseg ? kSegCap : total - (int64_t)i * kSegCap;
        int64_t bm = (((seg_rows[i] + 7) / 8) + 7) & ~(int64_t)7;
        seg_bytes[i] = 8 + seg_rows[i] * 8 + bm;
        col_bytes += seg_bytes[i];
    }
    blob_bytes = col_bytes * ncols;
    HIP_CHECK(ps.dev(&H->blob, (size_t)blob_bytes + 8));
    HIP_CHECK(hipMemsetAsync(H->blob, 0, (size_t)blob_bytes, st));
    HIP_CHECK(ps.dev(&d_off, sizeof(int64_t) * nseg));

    H->segs = (YtSegment*)calloc((size_t)nseg * ncols, sizeof(YtSegment));
    H->col = (YtColumn*)calloc(ncols, sizeof(YtColumn));
    for (int c = 0; c < ncols; c++) {
        std::vector<int64_t> off(nseg);
        int64_t at = (int64_t)c * col_bytes;
        for (int i = 0; i < nseg; i++) {
            off[i] = at;
            /* int: bitpack header rows|64<<56; double: [u64 count] */
            uint64_t hdr = col_is_dbl[c] ? (uint64_t)seg_rows[i]
                                         : ((uint64_t)seg_rows[i] | (64ULL << 56));
            HIP_CHECK(hipMemcpyAsync(H->blob + at, &hdr, 8,
                                     hipMemcpyHostToDevice, st));
            YtSegment& sg = H->segs[c * nseg + i];
            sg.type = col_is_dbl[c] ? YT_SEG_DOUBLE : YT_SEG_DIRECT_DENSE;
            sg.row_count = (int32_t)seg_rows[i];
            sg.min_value = 0;
            sg.data = H->blob + at;
            sg.data_size = seg_bytes[i];
            at += seg_bytes[i];
        }
        HIP_CHECK(hipMemcpyAsync(d_off, off.data(), sizeof(int64_t) * nseg,
                                 hipMemcpyHostToDevice, st));
        HIP_CHECK(ytql_launch_vis_scatter(d_vis, d_null[c], d_bits[c], n, d_blk,
                                          (uint64_t)kSegCap, d_off,
                                          H->blob, col_is_dbl[c], grid, st));
        HIP_CHECK(hipStreamSynchronize(st));
        YtColumn& C2 = H->col[c];
        C2.value_type = col_is_dbl[c] ? YT_VT_DOUBLE : YT_VT_INT64;
        C2.segment_count = nseg;
        C2.segments = &H->segs[c * nseg];
    }
    out_chunk->row_count = total;
    out_chunk->column_count = ncols;
    out_chunk->columns = H->col;
    ps.detach(H->blob);         /* the handle's from here on */
    *out_handle = H.release();
    return YT_OK;
}

extern "C" void yt_gpu_scan_chunk_free(YtChunk* chunk, void* handle)
{
    auto* H = (ScanChunkHandle*)handle;
    if (!H) return;
    g_pool.put(H->blob);
    delete H;
    if (chunk) memset(chunk, 0, sizeof(*chunk));
}

extern "C" int yt_gpu_query_execute(
    const YtPlan* plan, const YtChunk* chunk, const YtExecOptions* options,
    YtRowset* output, YtStatistics* stats, char* errbuf, size_t errlen)
{
    int rc = yt_gpu_available(errbuf, errlen);
    if (rc != YT_OK) return rc;
    if (!plan || !chunk || !output) { set_err(errbuf, errlen, "null argument"); return YT_ERR_INVALID_PLAN; }

    double tw0 = now_ms();
    double tp0 = 0, tp1 = 0, tp2 = 0;   /* phase checkpoints (YTQL_TIMING) */
    YtExecOptions defopt;
    memset(&defopt, 0, sizeof(defopt));
    if (!options) options = &defopt;
    if (stats) memset(stats, 0, sizeof(*stats));

    if (plan->agg_count == 0 && plan->project_count == 0 &&
        plan->key_count == 0) {
        set_err(errbuf, errlen, "empty plan");
        return YT_ERR_INVALID_PLAN;
    }
    output->totals_row = 0;
    t_last_strpred_entries = 0;
    t_last_strjoin_inserted = 0;
    t_last_strjoin_entries = 0;
    t_last_strkey_entries = 0;
    t_last_strkey_distinct = 0;
    t_last_inlist_mode = 0;
    t_last_topk = 0;
    if (plan->having && expr_has_strlit(plan->having)) {
        set_err(errbuf, errlen, "HAVING over string values: not this round");
        return YT_ERR_UNSUPPORTED;
    }
    if (plan->with_totals || plan->having) {
        if (plan->key_count == 0) {
            set_err(errbuf, errlen, "WITH TOTALS / HAVING requires GROUP BY");
            return YT_ERR_INVALID_PLAN;
        }
        if (plan->project_count) {
            set_err(errbuf, errlen,
                    "WITH TOTALS / HAVING with projections: not this round");
            return YT_ERR_UNSUPPORTED;
        }
        if (options->output_row_limit > 0) {
            set_err(errbuf, errlen,
                    "WITH TOTALS / HAVING with OutputRowLimit: not this round");
            return YT_ERR_UNSUPPORTED;
        }
    }

    {
        int kc;
        if (plan->key_count == 1 && plan->agg_count > 0 &&
            expr_is_col(plan->keys[0], &kc) && kc < chunk->column_count &&
            chunk->columns[kc].value_type == YT_VT_STRING) {
            if (plan->join) {
                set_err(errbuf, errlen,
                        "join with string group keys: not this round");
                return YT_ERR_UNSUPPORTED;
            }
            rc = run_string_group(plan, chunk, options, kc, output, stats,
                                  tw0, errbuf, errlen);
            if (rc == YT_OK && (plan->order_count > 0 || plan->with_totals ||
                                plan->having)) {
                rc = finish_output(plan, output, errbuf, errlen);
                if (rc == YT_OK && stats)
                    stats->rows_written = output->row_count;
            }
            return rc;
        }
    }

    DevPlan dp;
    StrPreds SP;
    rc = build_devplan(plan, chunk, &dp, &SP, errbuf, errlen);
    if (rc) return rc;

    JoinRun JR[2];
    const JoinDev* jd = nullptr;
    const JoinDev* jd2 = nullptr;
    rc = setup_join_chain(plan, chunk, JR, &jd, &jd2,
                          (hipStream_t)(uintptr_t)options->stream,
                          errbuf, errlen);
    if (rc) return rc;
    if (jd->active && jd->has_dups &&
        (plan->order_count > 0 || plan->agg_count == 0)) {
        /* the ORDER BY / scan-project machinery tracks candidates by
         * primary row id; a one-to-many join breaks that identity —
         * grouped plans take the cross-product path instead */
        set_err(errbuf, errlen,
                "join: duplicate foreign keys with ORDER BY / plain scan "
                "not this round (GROUP BY plans supported)");
        return YT_ERR_UNSUPPORTED;
    }

    if (plan->agg_count == 0 && plan->key_count == 0) {
        /* a plain scan reports YT_SCAN_PATH_PROJ_COMPACT or nothing */
        t_last_scan_path = 0;
        if (plan->order_count > 0) {
            /* scan + ORDER BY ... LIMIT: k-selection, no full materialization */
            return run_scan_topk(plan, chunk, options, &dp, &SP, jd, jd2,
                                 output, stats, tw0, errbuf, errlen);
        }
        return run_scan_project(plan, chunk, options, &dp, &SP, jd, jd2,
                                output, stats, tw0, errbuf, errlen);
    }

    FastShape fs;
    analyze_fast(plan, chunk, &fs);
    /* a string predicate runs in the interpreter only. analyze_fast refuses
     * any chunk that holds a non-int64 column, so this never fires; it is
     * stated so that it does not depend on that */
    if (SP.any) fs.valid = fs.ragged = 0;
    /* so does a packed STRING key; a multi-key plan is no fast shape either */
    for (int i = 0; i < dp.kp_count; i++)
        if (kp_is_str(&dp, i)) fs.valid = fs.ragged = 0;

    DeviceRun R;
    R.stream = (hipStream_t)(uintptr_t)options->stream;
    /* the groups go straight to the host from here: 32-byte records do */
    R.want_slim = true;
    if (options->device) {
        hipError_t e = hipSetDevice(options->device);
        if (e != hipSuccess) { set_err(errbuf, errlen, "bad device"); return YT_ERR_HIP; }
    }

    unsigned maxw = 0;
    int in_clamped = 0;
    rc = setup_chunk(chunk, &R, &maxw, options->input_row_limit, &in_clamped,
                     errbuf, errlen);
    if (rc) return rc;
    StrKeyTab strtabs[kMaxPackKeys];
    if (dp.kp_count && chunk->row_count > 0 && R.nsegs > 0) {
        rc = setup_strkey_ids(&R, &dp, strtabs, errbuf, errlen);
        if (rc) return rc;
        rc = pack_group_key(&dp, &R, errbuf, errlen, strtabs);
        if (rc) return rc;
    }

    if (chunk->row_count == 0 || R.nsegs == 0) {
        /* zero groups -> single final flush emits nothing (registry.cpp:1481) */
        output->row_count = 0;
        output->string_pool_used = 0;
        output->column_count = plan->project_count ? plan->project_count
            : (plan->key_count + plan->agg_count);
        return YT_OK;
    }

    rc = setup_table(&R, plan->agg_count,
                     options->max_groups_hint,
                     options->group_row_limit, errbuf, errlen);
    if (rc) return rc;
    rc = setup_string_preds(&SP, &R, &dp, errbuf, errlen);
    if (rc) return rc;
    JoinDev jstr[2];
    rc = setup_strjoin_maps(&R, &jd, &jd2, jstr, errbuf, errlen);
    if (rc) return rc;

    const bool timing = getenv("YTQL_TIMING") != nullptr;   /* phase breakdown to stderr */
    tp0 = now_ms();
    rc = run_scan(plan, chunk, options, &R, &dp, jd, jd2, &fs, maxw, stats,
                  errbuf, errlen);
    if (rc) return rc;
    tp1 = now_ms();

    /* compact + readback (pinned staging from the pool) */
    TableHdr th;
    int64_t ngroups = 0;
    {
        /* the staging buffers and slice events live as long as this block;
         * `drain` is declared after `ps`, so on every way out the stream is
         * idle before the pool takes the pinned staging back */
        PoolScope ps;
        struct Drain {
            hipStream_t st;
            bool armed;
            ~Drain() { if (armed) (void)hipStreamSynchronize(st); }
        } drain{R.stream, false};
        OutGroup* hgroups = nullptr;
        SlimGroup* hslim = nullptr;
        SlimSlices slices;
        slices.count = 0;
        slices.per = 0;
        /* the partitioned path already brought the header back */
        if (R.th_valid) th = *R.h_th;
        else HIP_CHECK(hipMemcpy(&th, R.d_th, sizeof(th), hipMemcpyDeviceToHost));
        if (th.overflow == 1) { set_err(errbuf, errlen, "group table overflow — raise max_groups_hint"); return YT_ERR_CAPACITY; }
        ngroups = (int64_t)th.ngroups;
        if (ngroups > 0 && !R.groups_compacted) {
            HIP_CHECK(R.ps.dev(&R.d_groups, sizeof(OutGroup) * ngroups));
            HIP_CHECK(R.ps.dev(&R.d_counter, sizeof(unsigned long long)));
            HIP_CHECK(hipMemsetAsync(R.d_counter, 0, sizeof(unsigned long long), R.stream));
            HIP_CHECK(ytql_launch_compact(nullptr, R.d_th, R.d_slots, plan->agg_count,
                                          R.d_groups, R.d_counter, R.nslots, R.stream));
        }
        if (ngroups > 0 && R.groups_compacted && R.groups_slim) {
            /* 32-byte records; from 65,536 groups on (where emit_rows may
             * run its workers) in slices, so that the emit of one slice
             * overlaps the copy of the next */
            const SlimGroup* d_slim = (const SlimGroup*)R.d_groups;
            HIP_CHECK(ps.host(&hslim, sizeof(SlimGroup) * ngroups));
            drain.armed = true;
            const int want = ngroups >= 65536 ? kGroupSlices : 1;
            slices.per = (ngroups + want - 1) / want;
            for (int64_t a = 0; a < ngroups; a += slices.per) {
                const int64_t cnt = std::min(slices.per, ngroups - a);
                HIP_CHECK(hipMemcpyAsync(hslim + a, d_slim + a, sizeof(SlimGroup) * cnt,
                                         hipMemcpyDeviceToHost, R.stream));
                hipEvent_t ev = nullptr;
                HIP_CHECK(ps.event(&ev, hipEventDisableTiming));
                slices.ev[slices.count++] = ev;
                HIP_CHECK(hipEventRecord(ev, R.stream));
            }
        } else if (ngroups > 0) {
            HIP_CHECK(ps.host(&hgroups, sizeof(OutGroup) * ngroups));
            drain.armed = true;
            HIP_CHECK(hipMemcpyAsync(hgroups, R.d_groups, sizeof(OutGroup) * ngroups,
                                     hipMemcpyDeviceToHost, R.stream));
            HIP_CHECK(hipStreamSynchronize(R.stream));
        }
        tp2 = now_ms();
        std::vector<uint64_t> gaccum(1 + 2 * kMaxAggs, 0);
        if (fs.valid && fs.key_col < 0) {
            HIP_CHECK(hipMemcpy(gaccum.data(), R.d_gaccum,
                                sizeof(uint64_t) * (1 + 2 * kMaxAggs), hipMemcpyDeviceToHost));
        }
        int out_limited = 0;
        rc = emit_rows(plan, chunk, &dp, hgroups, ngroups, th, 0, gaccum.data(),
                       fs.valid && fs.key_col < 0,
                       options->output_row_limit, &out_limited,
                       output, errbuf, errlen, hslim, hslim ? &slices : nullptr,
                       strtabs);
        if (hslim) {
            /* emit_rows can return before the last slice has landed */
            hipError_t es = hipStreamSynchronize(R.stream);
            if (es != hipSuccess && rc == YT_OK) {
                set_err(errbuf, errlen, hipGetErrorString(es));
                rc = YT_ERR_HIP;
            }
        }
        drain.armed = false;
        if (rc) return rc;
        if (out_limited && stats) stats->incomplete_output = 1;
    }
    if (timing) {
        double tp3 = now_ms();
        fprintf(stderr, "[ytql timing] pre-scan %.2fms scan-wall %.2fms compact+D2H %.2fms emit %.2fms\n",
                tp0 - tw0, tp1 - tp0, tp2 - tp1, tp3 - tp2);
    }
    if (plan->order_count > 0 || plan->with_totals || plan->having) {
        /* grouped output is already bounded: order/totals/having on the host
         * (combined group+order mode, registry.cpp:1677-1699) */
        rc = finish_output(plan, output, errbuf, errlen);
        if (rc) return rc;
        if (stats) stats->rows_written = output->row_count;
    }
    if (stats) {
        stats->rows_read = (options->input_row_limit > 0 &&
                            options->input_row_limit < chunk->row_count)
            ? options->input_row_limit : chunk->row_count;
        stats->incomplete_input = in_clamped;
        int64_t bytes = 0;
        for (int c = 0; c < chunk->column_count; c++)
            for (int s = 0; s < chunk->columns[c].segment_count; s++)
                bytes += chunk->columns[c].segments[s].data_size;
        stats->data_weight_read = bytes;
        stats->rows_written = output->row_count;
        stats->grouped_row_count = (int64_t)th.ngroups
            + (plan->key_count ? (int64_t)(th.side_used[0] + th.side_used[1]) : 0);
        stats->incomplete_output |= (th.overflow == 2);
        stats->execute_time_ms = now_ms() - tw0;
    }
    return YT_OK;
}

static int query_partial_impl(
    const YtPlan* plan, const YtChunk* chunk, const YtExecOptions* options,
    int32_t partition_count, void* states_device, int64_t capacity_rows,
    int64_t* part_counts,
    const uint64_t* key_zzmin, const uint64_t* key_zzmax,
    YtStatistics* stats, char* errbuf, size_t errlen)
{
    int rc = yt_gpu_available(errbuf, errlen);
    if (rc != YT_OK) return rc;
    if (plan->key_count < 1 || plan->key_count > kMaxPackKeys) {
        set_err(errbuf, errlen, "partial: 1..4 group keys");
        return YT_ERR_UNSUPPORTED;
    }
    if (plan->key_count > 1 && (!key_zzmin || !key_zzmax)) {
        set_err(errbuf, errlen,
                "partial: multi-key sharding needs the common key ranges "
                "(yt_gpu_key_ranges + cross-rank min/max reduce)");
        return YT_ERR_UNSUPPORTED;
    }
    if (partition_count < 1 || partition_count > 64) { set_err(errbuf, errlen, "partial: 1..64 partitions"); return YT_ERR_UNSUPPORTED; }
    for (int i = 0; plan->key_count > 1 && i < plan->key_count; i++) {
        int kc;
        if (expr_is_col(plan->keys[i], &kc) && kc >= 0 && kc < chunk->column_count &&
            chunk->columns[kc].value_type == YT_VT_STRING) {
            set_err(errbuf, errlen,
                    "partial: multi-key GROUP BY with a string key: string ids "
                    "are local to one chunk and cannot be exchanged");
            return YT_ERR_UNSUPPORTED;
        }
    }
    /* join at the bottom query (the reference's coordinated split keeps
     * JoinClause in the bottom, coordinator.cpp:130-170: the dimension
     * table is available on every node) — each rank builds the foreign
     * hash table from its own copy of the dimension chunk and the generic
     * scan probes it while producing partial states. Multi-key packing
     * would need zigzag ranges of foreign columns; deferred. */
    if (plan->join && plan->key_count > 1) {
        set_err(errbuf, errlen,
                "partial: join with multi-key GROUP BY not this round");
        return YT_ERR_UNSUPPORTED;
    }
    /* the 32-byte state carries ONE running {sum, nonnull-count} slot plus
     * the row count: sum(x) or avg(x) (the reference's coordinated avg is
     * exactly {count,sum}: GroupByWithAvgCoordinated ql_query_ut.cpp:2760) */
    int sum_slot = -1;
    int state_func = YT_AGG_SUM;
    for (int a = 0; a < plan->agg_count; a++) {
        int f = plan->aggs[a]->func;
        if (f == YT_AGG_SUM || f == YT_AGG_AVG || f == YT_AGG_MIN ||
            f == YT_AGG_MAX || f == YT_AGG_FIRST) {
            if (sum_slot >= 0) { set_err(errbuf, errlen, "partial: one value-carrying agg max this round"); return YT_ERR_UNSUPPORTED; }
            sum_slot = a;
            state_func = f;
        } else if (f != YT_AGG_SUM1) {
            set_err(errbuf, errlen, "partial: sum/avg/min/max/first/sum(1) only");
            return YT_ERR_UNSUPPORTED;
        }
    }

    YtExecOptions defopt;
    memset(&defopt, 0, sizeof(defopt));
    if (!options) options = &defopt;
    if (stats) memset(stats, 0, sizeof(*stats));

    double tw0 = now_ms();
    t_last_strpred_entries = 0;
    t_last_strjoin_inserted = 0;
    t_last_strjoin_entries = 0;
    t_last_strkey_entries = 0;
    t_last_strkey_distinct = 0;
    t_last_inlist_mode = 0;
    t_last_topk = 0;
    DevPlan dp;
    StrPreds SP;
    rc = build_devplan(plan, chunk, &dp, &SP, errbuf, errlen);
    if (rc) return rc;
    FastShape fs;
    analyze_fast(plan, chunk, &fs);
    if (SP.any) fs.valid = fs.ragged = 0;   /* interpreter only, as in yt_gpu_query_execute */

    DeviceRun R;
    R.stream = (hipStream_t)(uintptr_t)options->stream;

    unsigned maxw = 0;
    int in_clamped = 0;
    rc = setup_chunk(chunk, &R, &maxw, options->input_row_limit, &in_clamped,
                     errbuf, errlen);
    if (rc) return rc;
    if (chunk->row_count == 0 || R.nsegs == 0) {
        for (int p = 0; p < partition_count; p++) part_counts[p] = 0;
        return YT_OK;
    }
    if (dp.kp_count && key_zzmin && key_zzmax) {
        /* pack the composite with the COMMON cross-rank ranges so every
         * rank's key_bits agree (partition hash + merge identity) */
        for (int i = 0; i < dp.kp_count; i++) {
            int c = dp.kp_col[i];
            R.col_zzmin[c] = key_zzmin[i];
            R.col_zzmax[c] = key_zzmax[i];
        }
        rc = pack_group_key(&dp, &R, errbuf, errlen);
        if (rc) return rc;
    } else if (dp.kp_count) {
        rc = pack_group_key(&dp, &R, errbuf, errlen);
        if (rc) return rc;
    }
    rc = setup_table(&R, plan->agg_count, options->max_groups_hint,
                     options->group_row_limit, errbuf, errlen);
    if (rc) return rc;
    rc = setup_string_preds(&SP, &R, &dp, errbuf, errlen);
    if (rc) return rc;
    double tq0 = now_ms();
    JoinRun JRp[2];
    const JoinDev* pjd = nullptr;
    const JoinDev* pjd2 = nullptr;
    rc = setup_join_chain(plan, chunk, JRp, &pjd, &pjd2,
                          (hipStream_t)(uintptr_t)options->stream,
                          errbuf, errlen);
    if (rc) return rc;
    JoinDev jstr[2];
    rc = setup_strjoin_maps(&R, &pjd, &pjd2, jstr, errbuf, errlen);
    if (rc) return rc;
    /* dup foreign keys on item 0 are fine here: a partial is always grouped */
    rc = run_scan(plan, chunk, options, &R, &dp, pjd, pjd2, &fs, maxw, stats,
                  errbuf, errlen);
    if (rc) return rc;
    if (getenv("YTQL_TIMING"))
        fprintf(stderr, "[ytql timing] partial: setup %.2fms scan %.2fms\n",
                tq0 - tw0, now_ms() - tq0);

    TableHdr th;
    double tq15 = now_ms();
    HIP_CHECK(hipMemcpy(&th, R.d_th, sizeof(th), hipMemcpyDeviceToHost));
    if (th.overflow == 1) { set_err(errbuf, errlen, "group table overflow"); return YT_ERR_CAPACITY; }
    int64_t ngroups = (int64_t)th.ngroups;
    int64_t total = ngroups + th.side_used[0] + th.side_used[1];
    if (total > capacity_rows) { set_err(errbuf, errlen, "state buffer too small"); return YT_ERR_CAPACITY; }

    if (!R.groups_compacted) {
        /* compact table into OutGroups (device) */
        HIP_CHECK(R.ps.dev(&R.d_groups, sizeof(OutGroup) * (total ? total : 1)));
        HIP_CHECK(R.ps.dev(&R.d_counter, sizeof(unsigned long long)));
        HIP_CHECK(hipMemsetAsync(R.d_counter, 0, sizeof(unsigned long long), R.stream));
        if (ngroups > 0) {
            HIP_CHECK(ytql_launch_compact(nullptr, R.d_th, R.d_slots, plan->agg_count,
                                          R.d_groups, R.d_counter, R.nslots, R.stream));
        }
    } else if (R.groups_capacity < total) {
        set_err(errbuf, errlen, "state buffer too small");
        return YT_ERR_CAPACITY;
    }
    /* append side groups from host */
    int64_t pos = ngroups;
    for (int side = 0; side < 2; side++) {
        if (!th.side_used[side]) continue;
        OutGroup g;
        memset(&g, 0, sizeof(g));
        g.key_bits = th.side_key_bits[side];
        g.key_meta = (side == 1);
        g.cnt = th.side_cnt[side];
        for (int a = 0; a < plan->agg_count; a++) {
            g.agg_bits[a] = th.side_agg[side][2 * a];
            g.agg_nonnull[a] = th.side_agg[side][2 * a + 1];
        }
        HIP_CHECK(hipMemcpyAsync(R.d_groups + pos, &g, sizeof(g),
                                 hipMemcpyHostToDevice, R.stream));
        pos++;
    }

    /* partition counts → host prefix → scatter */
    double tq2 = now_ms();
    unsigned long long* d_counts = nullptr;
    HIP_CHECK(R.ps.dev(&d_counts, sizeof(unsigned long long) * partition_count));
    HIP_CHECK(hipMemsetAsync(d_counts, 0, sizeof(unsigned long long) * partition_count, R.stream));
    HIP_CHECK(ytql_launch_part_count(R.d_groups, total, partition_count, sum_slot,
                                     d_counts, R.stream));
    std::vector<unsigned long long> counts(partition_count);
    HIP_CHECK(hipMemcpyAsync(counts.data(), d_counts,
                             sizeof(unsigned long long) * partition_count,
                             hipMemcpyDeviceToHost, R.stream));
    HIP_CHECK(hipStreamSynchronize(R.stream));
    std::vector<unsigned long long> cursors(partition_count);
    unsigned long long run = 0;
    for (int p = 0; p < partition_count; p++) { cursors[p] = run; run += counts[p]; }
    HIP_CHECK(hipMemcpyAsync(d_counts, cursors.data(),
                             sizeof(unsigned long long) * partition_count,
                             hipMemcpyHostToDevice, R.stream));
    int sum_is_double = 0;
    if (sum_slot >= 0) {
        /* dp.col_types already appends the joined foreign columns */
        int at = expr_static_type(plan->aggs[sum_slot]->arg, dp.col_types);
        sum_is_double = at == YT_VT_DOUBLE;
        if ((state_func == YT_AGG_MIN || state_func == YT_AGG_MAX) &&
            at != YT_VT_INT64 && at != YT_VT_DOUBLE) {
            set_err(errbuf, errlen,
                    "partial: min/max over int64/double args this round");
            return YT_ERR_UNSUPPORTED;
        }
    }
    HIP_CHECK(ytql_launch_part_scatter(R.d_groups, total, partition_count, sum_slot,
                                       sum_is_double, state_func,
                                       d_counts, (YtStateRow*)states_device, R.stream));
    HIP_CHECK(hipStreamSynchronize(R.stream));
    for (int p = 0; p < partition_count; p++) part_counts[p] = (int64_t)counts[p];
    if (getenv("YTQL_TIMING"))
        fprintf(stderr, "[ytql timing] partial total %.2fms (compact+sides %.2fms count/scatter %.2fms)\n",
                now_ms() - tw0, tq2 - tq15, now_ms() - tq2);
    if (stats) {
        stats->rows_read = chunk->row_count;
        stats->grouped_row_count = total;
        stats->incomplete_output = (th.overflow == 2);
    }
    return YT_OK;
}

extern "C" int yt_gpu_query_partial(
    const YtPlan* plan, const YtChunk* chunk, const YtExecOptions* options,
    int32_t partition_count, void* states_device, int64_t capacity_rows,
    int64_t* part_counts, YtStatistics* stats, char* errbuf, size_t errlen)
{
    if (plan && plan->key_count != 1) {
        set_err(errbuf, errlen, "partial: need exactly 1 key (use _mk)");
        return YT_ERR_UNSUPPORTED;
    }
    return query_partial_impl(plan, chunk, options, partition_count,
                              states_device, capacity_rows, part_counts,
                              nullptr, nullptr, stats, errbuf, errlen);
}

extern "C" int yt_gpu_query_partial_mk(
    const YtPlan* plan, const YtChunk* chunk, const YtExecOptions* options,
    int32_t partition_count, void* states_device, int64_t capacity_rows,
    int64_t* part_counts,
    const uint64_t* key_zzmin, const uint64_t* key_zzmax,
    YtStatistics* stats, char* errbuf, size_t errlen)
{
    return query_partial_impl(plan, chunk, options, partition_count,
                              states_device, capacity_rows, part_counts,
                              key_zzmin, key_zzmax, stats, errbuf, errlen);
}

/* STRING-keyed bottom query: the local string group-by (run_string_group)
 * followed by a hash partition of the groups into YtStateRow records +
 * per-partition key-byte pool slices. The caller all-to-alls BOTH buffers
 * (counts and byte counts per partition are returned); each received
 * state's key_bits is an offset within its own slice. Mirrors the
 * reference's key shuffle (shuffling_reader.cpp:40-42) applied to string
 * group keys. */
extern "C" int yt_gpu_query_partial_str(
    const YtPlan* plan, const YtChunk* chunk, const YtExecOptions* options,
    int32_t partition_count, void* states_device, int64_t capacity_rows,
    void* pool_device, int64_t pool_capacity,
    int64_t* part_counts, int64_t* part_pool_bytes,
    YtStatistics* stats, char* errbuf, size_t errlen)
{
    int rc = yt_gpu_available(errbuf, errlen);
    if (rc != YT_OK) return rc;
    if (!plan || !chunk) { set_err(errbuf, errlen, "null argument"); return YT_ERR_INVALID_PLAN; }
    if (partition_count < 1 || partition_count > 64) { set_err(errbuf, errlen, "partial_str: 1..64 partitions"); return YT_ERR_UNSUPPORTED; }
    int kc = -1;
    if (!(plan->key_count == 1 && plan->agg_count > 0 &&
          expr_is_col(plan->keys[0], &kc) && kc < chunk->column_count &&
          chunk->columns[kc].value_type == YT_VT_STRING)) {
        set_err(errbuf, errlen, "partial_str: needs one string key column + aggregates");
        return YT_ERR_UNSUPPORTED;
    }
    if (plan->join) { set_err(errbuf, errlen, "partial_str: join with string keys not this round"); return YT_ERR_UNSUPPORTED; }
    YtExecOptions defopt;
    memset(&defopt, 0, sizeof(defopt));
    if (!options) options = &defopt;
    if (stats) memset(stats, 0, sizeof(*stats));
    t_last_strpred_entries = 0;
    t_last_strjoin_inserted = 0;
    t_last_strjoin_entries = 0;
    t_last_strkey_entries = 0;
    t_last_strkey_distinct = 0;
    t_last_inlist_mode = 0;
    t_last_topk = 0;
    StrPartialOut po;
    po.partition_count = partition_count;
    po.states_device = (YtStateRow*)states_device;
    po.capacity_rows = capacity_rows;
    po.pool_device = (char*)pool_device;
    po.pool_capacity = pool_capacity;
    po.part_counts = part_counts;
    po.part_pool_bytes = part_pool_bytes;
    return run_string_group(plan, chunk, options, kc, nullptr, stats,
                            now_ms(), errbuf, errlen, &po);
}

/* per-rank key-column zigzag ranges for the cross-rank reduce (meta-only
 * bound: conservative is fine, the reduce of bounds is a bound) */
extern "C" int yt_gpu_key_ranges(
    const YtPlan* plan, const YtChunk* chunk,
    uint64_t* key_zzmin, uint64_t* key_zzmax,
    uint64_t stream, char* errbuf, size_t errlen)
{
    int rc = yt_gpu_available(errbuf, errlen);
    if (rc != YT_OK) return rc;
    if (plan->key_count < 1 || plan->key_count > kMaxPackKeys) {
        set_err(errbuf, errlen, "key_ranges: 1..4 group keys");
        return YT_ERR_UNSUPPORTED;
    }
    DeviceRun R;
    R.stream = (hipStream_t)(uintptr_t)stream;
    unsigned maxw = 0;
    int cl = 0;
    rc = setup_chunk(chunk, &R, &maxw, 0, &cl, errbuf, errlen);
    if (rc) return rc;
    for (int i = 0; i < plan->key_count; i++) {
        int c;
        if (!expr_is_col(plan->keys[i], &c) || c >= chunk->column_count) {
            set_err(errbuf, errlen, "key_ranges: plain key columns only");
            return YT_ERR_UNSUPPORTED;
        }
        if (plan->key_count > 1 && chunk->columns[c].value_type == YT_VT_STRING) {
            set_err(errbuf, errlen,
                    "key_ranges: multi-key GROUP BY with a string key: string "
                    "ids are local to one chunk and cannot be exchanged");
            return YT_ERR_UNSUPPORTED;
        }
        key_zzmin[i] = R.col_zzmin[c];
        key_zzmax[i] = R.col_zzmax[c];
    }
    return YT_OK;
}

static int merge_states_impl(
    const YtPlan* plan, const void* states_device, int64_t state_row_count,
    const uint8_t* col_types,
    const uint64_t* key_zzmin, const uint64_t* key_zzmax,
    const YtExecOptions* options, YtRowset* output, YtStatistics* stats,
    char* errbuf, size_t errlen)
{
    int rc = yt_gpu_available(errbuf, errlen);
    if (rc != YT_OK) return rc;
    if (plan->key_count < 1 || plan->key_count > kMaxPackKeys) {
        set_err(errbuf, errlen, "merge: 1..4 group keys");
        return YT_ERR_UNSUPPORTED;
    }
    if (plan->key_count > 1 && (!key_zzmin || !key_zzmax)) {
        set_err(errbuf, errlen, "merge: multi-key needs the common key ranges");
        return YT_ERR_UNSUPPORTED;
    }
    for (int i = 0; plan->key_count > 1 && col_types && i < plan->key_count; i++) {
        int kc;
        if (expr_is_col(plan->keys[i], &kc) && kc >= 0 && kc < kMaxCols &&
            col_types[kc] == YT_VT_STRING) {
            set_err(errbuf, errlen,
                    "merge: multi-key GROUP BY with a string key: string ids "
                    "are local to one chunk and cannot be exchanged");
            return YT_ERR_UNSUPPORTED;
        }
    }
    if (col_types && plan->agg_count <= kMaxAggs) {
        /* the front query evaluates HAVING and projections on the host; the
         * typing rules need the bottom query's column types */
        rc = check_plan_types(plan, col_types, kMaxCols, errbuf, errlen);
        if (rc) return rc;
    }
    output->totals_row = 0;
    int sum_slot = -1;
    int state_func = YT_AGG_SUM;
    for (int a = 0; a < plan->agg_count; a++) {
        int f = plan->aggs[a]->func;
        if (f == YT_AGG_SUM || f == YT_AGG_AVG || f == YT_AGG_MIN ||
            f == YT_AGG_MAX || f == YT_AGG_FIRST) { sum_slot = a; state_func = f; }
    }

    YtExecOptions defopt;
    memset(&defopt, 0, sizeof(defopt));
    if (!options) options = &defopt;
    if (stats) memset(stats, 0, sizeof(*stats));

    double tw0 = now_ms();
    DeviceRun R;
    R.stream = (hipStream_t)(uintptr_t)options->stream;
    rc = setup_table(&R, plan->agg_count, options->max_groups_hint, 0, errbuf, errlen);
    if (rc) return rc;
    rc = ensure_slots(&R, plan->agg_count, errbuf, errlen);
    if (rc) return rc;
    double tq1 = now_ms();

    HIP_CHECK(ytql_launch_merge_states((const YtStateRow*)states_device, state_row_count,
                                       plan->agg_count, sum_slot, state_func,
                                       R.d_th, R.d_slots, R.stream));
    HIP_CHECK(hipStreamSynchronize(R.stream));
    if (getenv("YTQL_TIMING"))
        fprintf(stderr, "[ytql timing] merge: setup %.2fms kernel %.2fms\n",
                tq1 - tw0, now_ms() - tq1);
    TableHdr th;
    HIP_CHECK(hipMemcpy(&th, R.d_th, sizeof(th), hipMemcpyDeviceToHost));
    if (th.overflow == 1) { set_err(errbuf, errlen, "merge table overflow"); return YT_ERR_CAPACITY; }
    int64_t ngroups = (int64_t)th.ngroups;
    OutGroup* hgroups = nullptr;
    if (ngroups > 0) {
        HIP_CHECK(R.ps.dev(&R.d_groups, sizeof(OutGroup) * ngroups));
        HIP_CHECK(R.ps.dev(&R.d_counter, sizeof(unsigned long long)));
        HIP_CHECK(hipMemsetAsync(R.d_counter, 0, sizeof(unsigned long long), R.stream));
        HIP_CHECK(ytql_launch_compact(nullptr, R.d_th, R.d_slots, plan->agg_count,
                                      R.d_groups, R.d_counter, R.nslots, R.stream));
        HIP_CHECK(R.ps.host(&hgroups, sizeof(OutGroup) * ngroups));
        HIP_CHECK(hipMemcpyAsync(hgroups, R.d_groups, sizeof(OutGroup) * ngroups,
                                 hipMemcpyDeviceToHost, R.stream));
        HIP_CHECK(hipStreamSynchronize(R.stream));
    }
    /* fabricate a single-int64-column chunk view for type inference:
     * the key static type is carried by plan->keys[0] over col types.
     * Merge callers use the same chunk schema as partial; we only need
     * col_types for expr_static_type — rebuild from the key expr columns
     * is not possible here, so default key/sum types to int64. */
    YtColumn col;
    memset(&col, 0, sizeof(col));
    col.value_type = YT_VT_INT64;
    col.segment_count = 0;
    std::vector<YtColumn> cols(kMaxCols, col);
    if (col_types) {
        for (int c2 = 0; c2 < kMaxCols; c2++)
            cols[c2].value_type = col_types[c2];
    }
    YtChunk fake;
    fake.row_count = 0;
    fake.column_count = kMaxCols;
    fake.columns = cols.data();
    /* multi-key: rebuild the composite packing from the COMMON ranges
     * (identical math to every rank's partial — pack_group_key) so
     * emit unpacks the key components */
    DevPlan dpk;
    DevPlan* dpk_p = nullptr;
    if (plan->key_count > 1) {
        memset(&dpk, 0, sizeof(dpk));
        dpk.ncols = kMaxCols;
        for (int c2 = 0; c2 < kMaxCols; c2++)
            dpk.col_types[c2] = col_types ? col_types[c2] : YT_VT_INT64;
        dpk.kp_count = plan->key_count;
        DeviceRun R2;   /* host-side ranges only */
        for (int i = 0; i < plan->key_count; i++) {
            int c2;
            if (!expr_is_col(plan->keys[i], &c2) || c2 >= kMaxCols) {
                set_err(errbuf, errlen, "merge: plain key columns only");
                return YT_ERR_UNSUPPORTED;
            }
            dpk.kp_col[i] = c2;
            dpk.kp_signed[i] = dpk.col_types[c2] == YT_VT_INT64;
            R2.col_zzmin[c2] = key_zzmin[i];
            R2.col_zzmax[c2] = key_zzmax[i];
        }
        rc = pack_group_key(&dpk, &R2, errbuf, errlen);
        if (rc) return rc;
        dpk_p = &dpk;
    }
    int out_limited = 0;
    rc = emit_rows(plan, &fake, dpk_p, hgroups, ngroups, th, 0,
                   nullptr, 0, options->output_row_limit, &out_limited,
                   output, errbuf, errlen);
    if (rc) return rc;
    if (out_limited && stats) stats->incomplete_output = 1;
    if (plan->order_count > 0 || plan->with_totals || plan->having) {
        /* ORDER BY / WITH TOTALS / HAVING apply at the front query */
        rc = finish_output(plan, output, errbuf, errlen);
        if (rc) return rc;
    }
    if (stats) {
        stats->rows_written = output->row_count;
        stats->grouped_row_count = ngroups + th.side_used[0] + th.side_used[1];
    }
    return YT_OK;
}

extern "C" int yt_gpu_merge_states(
    const YtPlan* plan, const void* states_device, int64_t state_row_count,
    const uint8_t* col_types,
    const YtExecOptions* options, YtRowset* output, YtStatistics* stats,
    char* errbuf, size_t errlen)
{
    if (plan && plan->key_count != 1) {
        set_err(errbuf, errlen, "merge: need exactly 1 key (use _mk)");
        return YT_ERR_UNSUPPORTED;
    }
    return merge_states_impl(plan, states_device, state_row_count, col_types,
                             nullptr, nullptr, options, output, stats,
                             errbuf, errlen);
}

extern "C" int yt_gpu_merge_states_mk(
    const YtPlan* plan, const void* states_device, int64_t state_row_count,
    const uint8_t* col_types,
    const uint64_t* key_zzmin, const uint64_t* key_zzmax,
    const YtExecOptions* options, YtRowset* output, YtStatistics* stats,
    char* errbuf, size_t errlen)
{
    return merge_states_impl(plan, states_device, state_row_count, col_types,
                             key_zzmin, key_zzmax, options, output, stats,
                             errbuf, errlen);
}

/* STRING-keyed front query: merge exchanged state rows (key_bits =
 * slice-local pool reference) whose pool slices were concatenated in
 * segment order on the receiver. seg_counts / seg_pool_bytes give each
 * segment's row and byte extent; states and pool are DEVICE buffers. */
extern "C" int yt_gpu_merge_states_str(
    const YtPlan* plan, const void* states_device, const int64_t* seg_counts,
    int32_t nseg_in, const void* pool_device, const int64_t* seg_pool_bytes,
    const uint8_t* col_types,      /* original chunk column types (sum arg) */
    const YtExecOptions* options, YtRowset* output, YtStatistics* stats,
    char* errbuf, size_t errlen)
{
    int rc = yt_gpu_available(errbuf, errlen);
    if (rc != YT_OK) return rc;
    if (!plan || !output || nseg_in < 1) { set_err(errbuf, errlen, "merge_str: bad arguments"); return YT_ERR_INVALID_PLAN; }
    if (plan->key_count != 1) { set_err(errbuf, errlen, "merge_str: one string key"); return YT_ERR_UNSUPPORTED; }
    if (plan->with_totals || plan->having || plan->order_count) {
        set_err(errbuf, errlen, "merge_str: totals/having/order not this round");
        return YT_ERR_UNSUPPORTED;
    }
    int sum_slot = -1;
    for (int a = 0; a < plan->agg_count; a++) {
        if (plan->aggs[a]->func == YT_AGG_SUM) {
            if (sum_slot >= 0) { set_err(errbuf, errlen, "merge_str: one sum agg max"); return YT_ERR_UNSUPPORTED; }
            sum_slot = a;
        } else if (plan->aggs[a]->func != YT_AGG_SUM1) {
            set_err(errbuf, errlen, "merge_str: sum/sum(1) only");
            return YT_ERR_UNSUPPORTED;
        }
    }
    int sum_is_double = 0;
    if (sum_slot >= 0) {
        uint8_t ct2[kMaxCols];
        memset(ct2, YT_VT_INT64, sizeof(ct2));
        if (col_types) {
            for (int c2 = 0; c2 < kMaxCols; c2++) ct2[c2] = col_types[c2];
        }
        sum_is_double =
            expr_static_type(plan->aggs[sum_slot]->arg, ct2) == YT_VT_DOUBLE;
    }
    YtExecOptions defopt;
    memset(&defopt, 0, sizeof(defopt));
    if (!options) options = &defopt;
    if (stats) memset(stats, 0, sizeof(*stats));
    hipStream_t st = (hipStream_t)(uintptr_t)options->stream;
    double tw0 = now_ms();

    int64_t n = 0, pool_total = 0;
    std::vector<int64_t> row_base(nseg_in);
    std::vector<unsigned long long> pool_base(nseg_in);
    for (int s = 0; s < nseg_in; s++) {
        row_base[s] = n;
        pool_base[s] = (unsigned long long)pool_total;
        n += seg_counts[s];
        pool_total += seg_pool_bytes[s];
    }
    output->row_count = 0;
    output->string_pool_used = 0;
    output->column_count = 1 + plan->agg_count;
    if (n == 0) return YT_OK;

    int64_t* d_rowb = nullptr;
    unsigned long long* d_poolb = nullptr;
    uint64_t* d_hashes = nullptr;
    uint64_t* d_idents = nullptr;
    ulonglong2* d_pfxs = nullptr;
    uint64_t* d_absoff = nullptr;
    StrSlot* d_slots = nullptr;
    TableHdr* d_th = nullptr;
    OutStrState* d_out = nullptr;
    char* d_opool = nullptr;
    unsigned long long* d_ctr = nullptr;
    OutStrState* hgroups = nullptr;
    char* hpool = nullptr;
    PoolScope ps;
    HIP_CHECK(ps.dev(&d_rowb, sizeof(int64_t) * nseg_in));
    HIP_CHECK(ps.dev(&d_poolb, sizeof(unsigned long long) * nseg_in));
    HIP_CHECK(hipMemcpyAsync(d_rowb, row_base.data(),
                             sizeof(int64_t) * nseg_in,
                             hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_poolb, pool_base.data(),
                             sizeof(unsigned long long) * nseg_in,
                             hipMemcpyHostToDevice, st));
    HIP_CHECK(ps.dev(&d_hashes, sizeof(uint64_t) * n));
    HIP_CHECK(ps.dev(&d_idents, sizeof(uint64_t) * n));
    HIP_CHECK(ps.dev(&d_pfxs, sizeof(ulonglong2) * n));
    HIP_CHECK(ps.dev(&d_absoff, sizeof(uint64_t) * n));
    uint64_t nslots_cap = next_pow2((uint64_t)n * 2);
    if (nslots_cap < 2048) nslots_cap = 2048;
    uint64_t nslots = options->max_groups_hint > 0
        ? next_pow2((uint64_t)options->max_groups_hint * 2)
        : nslots_cap;
    if (nslots < 2048) nslots = 2048;
    if (nslots > nslots_cap) nslots = nslots_cap;
    HIP_CHECK(ps.dev(&d_th, sizeof(TableHdr)));
    HIP_CHECK(ytql_launch_strst_hash((const YtStateRow*)states_device, n,
                                     d_rowb, d_poolb, nseg_in,
                                     (const char*)pool_device,
                                     d_hashes, d_idents, d_pfxs, d_absoff, st));
    TableHdr th;
    for (;;) {
        HIP_CHECK(ps.dev(&d_slots, sizeof(StrSlot) * nslots));
        HIP_CHECK(hipMemsetAsync(d_slots, 0, sizeof(StrSlot) * nslots, st));
        memset(&th, 0, sizeof(th));
        th.group_limit = options->group_row_limit;
        HIP_CHECK(hipMemcpyAsync(d_th, &th, sizeof(th),
                                 hipMemcpyHostToDevice, st));
        HIP_CHECK(ytql_launch_strst_merge((const YtStateRow*)states_device, n,
                                          (const char*)pool_device, d_hashes,
                                          d_idents, d_pfxs, d_absoff, sum_slot,
                                          d_slots, nslots, d_th, st));
        HIP_CHECK(hipMemcpy(&th, d_th, sizeof(th), hipMemcpyDeviceToHost));
        if (th.overflow != 1 || nslots >= nslots_cap) break;
        ps.release(d_slots);
        d_slots = nullptr;
        nslots *= 4;
        if (nslots > nslots_cap) nslots = nslots_cap;
    }
    if (th.overflow == 1) {
        set_err(errbuf, errlen, "merge_str: table overflow");
        return YT_ERR_CAPACITY;
    }
    int64_t ngroups = (int64_t)th.ngroups;
    int has_null = th.side_used[1] ? 1 : 0;
    if (ngroups + has_null > output->capacity_rows) {
        set_err(errbuf, errlen, "merge_str: output rowset too small");
        return YT_ERR_CAPACITY;
    }
    uint64_t opool_cap = (uint64_t)(pool_total ? pool_total : 1);
    HIP_CHECK(ps.dev(&d_out, sizeof(OutStrState) * (ngroups ? ngroups : 1)));
    HIP_CHECK(ps.dev(&d_opool, opool_cap));
    HIP_CHECK(ps.dev(&d_ctr, 2 * sizeof(unsigned long long)));
    HIP_CHECK(hipMemsetAsync(d_ctr, 0, 2 * sizeof(unsigned long long), st));
    if (ngroups > 0) {
        HIP_CHECK(ytql_launch_strst_compact(d_slots, nslots, d_absoff,
                                            (const char*)pool_device, d_out,
                                            d_ctr, d_opool, d_ctr + 1,
                                            opool_cap, d_th, st));
    }
    unsigned long long hctr[2] = {0, 0};
    HIP_CHECK(ps.host(&hgroups,
                              sizeof(OutStrState) * (ngroups ? ngroups : 1)));
    if (ngroups > 0) {
        HIP_CHECK(hipMemcpyAsync(hgroups, d_out,
                                 sizeof(OutStrState) * ngroups,
                                 hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipMemcpyAsync(hctr, d_ctr, 2 * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if ((unsigned long long)hctr[1] > (unsigned long long)output->string_pool_capacity
        || (output->string_pool == nullptr && hctr[1] != 0)) {
        set_err(errbuf, errlen, "merge_str: string pool too small");
        return YT_ERR_CAPACITY;
    }
    if (hctr[1]) {
        HIP_CHECK(ps.host(&hpool, hctr[1]));
        HIP_CHECK(hipMemcpyAsync(hpool, d_opool, hctr[1],
                                 hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        copy_parallel(output->string_pool, hpool, (size_t)hctr[1]);
    }
    output->string_pool_used = hctr[1];
    int ncols = 1 + plan->agg_count;
    int agg_is_sum1[kMaxAggs];
    for (int a = 0; a < plan->agg_count; a++)
        agg_is_sum1[a] = plan->aggs[a]->func == YT_AGG_SUM1;
    auto emit_range = [&](int64_t b, int64_t e) {
        for (int64_t g = b; g < e; g++) {
            const OutStrState& gg = hgroups[g];
            write_str_sum_row(output->values + g * ncols, plan->agg_count,
                              YT_VT_STRING, (uint32_t)(gg.off_len & 0xFFFFFF),
                              output->string_pool + (gg.off_len >> 24),
                              gg.cnt, gg.nonnull, gg.sum_bits,
                              agg_is_sum1, sum_is_double);
        }
    };
    if (ngroups >= 65536) {
        int nt = (int)std::min<int64_t>(std::thread::hardware_concurrency(),
                                        (ngroups + 65535) / 65536);
        ThreadJoiner tj;
        int64_t per = (ngroups + nt - 1) / nt;
        for (int t2 = 0; t2 < nt; t2++) {
            int64_t b = (int64_t)t2 * per;
            int64_t e = std::min<int64_t>(ngroups, b + per);
            if (b >= e) break;
            tj.ths.emplace_back(emit_range, b, e);
        }
    } else {
        emit_range(0, ngroups);
    }
    output->row_count = ngroups;
    if (has_null) {
        write_str_sum_null_row(output->values + output->row_count * ncols,
                               plan->agg_count, th, sum_slot, agg_is_sum1,
                               sum_is_double);
        output->row_count++;
    }
    if (stats) {
        stats->rows_written = output->row_count;
        stats->grouped_row_count = ngroups + has_null;
        stats->incomplete_output = (th.overflow == 2);
        stats->execute_time_ms = now_ms() - tw0;
    }
    return YT_OK;
}
