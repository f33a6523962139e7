/* probe: where does phase B (k_bucket_agg_direct) spend its time at the
 * headline's shapes? 1024 buckets x 8 sub-regions x 122,070 packed 8-byte
 * records (random 11-bit slot | 42-bit value << 11), cursors [sub][bucket],
 * one workgroup per bucket, a 2048-slot table in 32 KiB of LDS. Variants, at
 * 1024 x 256 threads unless named otherwise, three repetitions each:
 *   L    the r2 loop's loads only (eight 16-byte loads per lane in the full
 *        passes, then up to seven single-load turns per sub-region); every
 *        lane xor-reduces what it loaded and stores once
 *   A2   the LDS adds only: records made in registers from a counter hash,
 *        two ds_add_u64 per record (cnt|nonnull<<32, sum)
 *   A1   as A2 with a ds_add_u32 for the count and a ds_add_u64 for the sum
 *   S    the r2 loop whole: L's loads, A2's adds
 *   P    the candidate loop: every turn in the eight-load form (indices past
 *        the end clamped, their adds masked), the next turn's loads (crossing
 *        sub-regions) issued before this turn's adds, A1's adds
 *   P512 P with 512 threads per workgroup
 *   F0   the flush alone, 1024 non-empty slots of 2048 per workgroup (1 M
 *        groups of 32 bytes): a returning add on each of two words per group
 *   F1   the flush alone: ballot/popcount ranks, one reservation per
 *        workgroup, stores by rank
 * Prints us and TB/s (or G adds/s, M groups/s) per variant and repetition.
 * Every variant is checked: the tables sum to the number of records, the
 * flushes deliver every group once.
 * hipcc --offload-arch=gfx950 -O3 -o probe_bucket probe_bucket.hip */
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>

#define CHK(x) do { hipError_t e=(x); if(e){printf("HIP %s @%d\n", hipGetErrorString(e), __LINE__); exit(1);} } while(0)

constexpr int kNB = 1024, kSub = 8, kSlots = 2048, kSlotBits = 11;
constexpr int kRegion = 122070;                 /* records per (bucket, sub) */
constexpr int64_t kStride = (kRegion + 7) & ~7; /* records between regions */
constexpr int64_t kRecords = (int64_t)kNB * kSub * kRegion;

__host__ __device__ inline uint64_t mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

/* slot in bits 0..10, value in bits 11..52 */
__device__ inline uint64_t make_rec(uint64_t n) { return mix64(n) >> 11; }

__global__ void k_fill(uint64_t* recs, unsigned long long* cursors)
{
    const int64_t region = blockIdx.x;          /* bucket * 8 + sub */
    uint64_t* r = recs + region * kStride;
    for (int i = threadIdx.x; i < kStride; i += blockDim.x)
        r[i] = make_rec((uint64_t)region * kStride + i);
    if (threadIdx.x == 0)
        cursors[(region & 7) * kNB + (region >> 3)] = kRegion;
}

struct Slot { unsigned long long sum; unsigned nonnull, nullcnt; };

__device__ inline void add2(unsigned long long* cntnn, unsigned long long* sums, uint64_t r)
{
    const unsigned k = (unsigned)r & (kSlots - 1);
    atomicAdd(&cntnn[k], 1ULL | (1ULL << 32));
    atomicAdd(&sums[k], (unsigned long long)(r >> kSlotBits));
}

__device__ inline void add1(Slot* tab, uint64_t r)
{
    Slot* s = tab + ((unsigned)r & (kSlots - 1));
    atomicAdd(&s->nonnull, 1u);
    atomicAdd(&s->sum, (unsigned long long)(r >> kSlotBits));
}

/* per-workgroup total of the counts, for the host's check */
template <int T>
__device__ inline void report(const unsigned long long* words, int stride, int shift,
                              unsigned long long* wg_counts, unsigned long long* red)
{
    unsigned long long c = 0;
    for (int i = threadIdx.x; i < kSlots; i += T)
        c += shift ? (words[i * stride] & 0xFFFFFFFFULL) : (unsigned)words[i * stride];
    if (threadIdx.x == 0) red[0] = 0;
    __syncthreads();
    atomicAdd(&red[0], c);
    __syncthreads();
    if (threadIdx.x == 0) wg_counts[blockIdx.x] = red[0];
}

/* V: 0 = L, 1 = S */
template <int V>
__global__ void __launch_bounds__(256)
k_shipped(const uint64_t* recs, const unsigned long long* cursors,
          unsigned long long* wg_counts, unsigned long long* sink)
{
    __shared__ unsigned long long tab[2 * kSlots];
    __shared__ unsigned long long red[1];
    unsigned long long* cntnn = tab;
    unsigned long long* sums = tab + kSlots;
    const int tid = threadIdx.x, bucket = blockIdx.x;
    for (int i = tid; i < 2 * kSlots; i += 256) tab[i] = 0;
    __syncthreads();
    uint64_t x = 0;
    #define ACC(r_) { if (V == 0) x ^= (r_); else add2(cntnn, sums, (r_)); }
    for (int sub = 0; sub < kSub; sub++) {
        const int64_t n = (int64_t)cursors[sub * kNB + bucket];
        const uint64_t* rows8 = recs + ((int64_t)bucket * kSub + sub) * kStride;
        const ulonglong2* rows2 = (const ulonglong2*)rows8;
        const int64_t n2 = n >> 1;
        int64_t i = tid;
        for (; i + 1792 < n2; i += 2048) {
            ulonglong2 p0 = rows2[i], p1 = rows2[i + 256], p2 = rows2[i + 512],
                       p3 = rows2[i + 768], p4 = rows2[i + 1024], p5 = rows2[i + 1280],
                       p6 = rows2[i + 1536], p7 = rows2[i + 1792];
            ACC(p0.x) ACC(p0.y) ACC(p1.x) ACC(p1.y) ACC(p2.x) ACC(p2.y) ACC(p3.x) ACC(p3.y)
            ACC(p4.x) ACC(p4.y) ACC(p5.x) ACC(p5.y) ACC(p6.x) ACC(p6.y) ACC(p7.x) ACC(p7.y)
        }
        for (; i < n2; i += 256) {
            ulonglong2 pz = rows2[i];
            ACC(pz.x) ACC(pz.y)
        }
        if ((n & 1) && tid == 0) { uint64_t r = rows8[n - 1]; ACC(r) }
    }
    #undef ACC
    __syncthreads();
    if (V == 0) {
        if (x == 0x123456789ULL) sink[0] = x;   /* keeps the loads live */
        if (tid == 0) wg_counts[bucket] = (unsigned long long)kSub * kRegion;
    } else {
        report<256>(cntnn, 1, 1, wg_counts, red);
    }
}

/* V: 2 = A2, 3 = A1; each lane makes 16 records per turn, as many turns as
 * cover the bucket's records, the surplus of the last turn masked */
template <int V>
__global__ void __launch_bounds__(256)
k_adds(unsigned long long* wg_counts)
{
    __shared__ __attribute__((aligned(16))) unsigned long long tab[2 * kSlots];
    __shared__ unsigned long long red[1];
    const int tid = threadIdx.x, bucket = blockIdx.x;
    for (int i = tid; i < 2 * kSlots; i += 256) tab[i] = 0;
    __syncthreads();
    const int64_t total = (int64_t)kSub * kRegion;
    for (int64_t base = 0; base < total; base += 4096) {
        uint64_t r[16];
        #pragma unroll
        for (int j = 0; j < 16; j++)
            r[j] = make_rec(((uint64_t)bucket << 32) + base + tid + 256 * j);
        #pragma unroll
        for (int j = 0; j < 16; j++) {
            if (base + tid + 256 * j >= total) continue;
            if (V == 2) add2(tab, tab + kSlots, r[j]);
            else add1((Slot*)tab, r[j]);
        }
    }
    __syncthreads();
    if (V == 2) report<256>(tab, 1, 1, wg_counts, red);
    else report<256>(tab + 1, 2, 0, wg_counts, red);
}

/* the candidate loop */
__device__ inline int pick8(const int (&m)[8], int s)
{
    int r = 0;
    #pragma unroll
    for (int t = 0; t < 8; t++) r = (t == s) ? m[t] : r;
    return r;
}

template <int T>
__device__ inline void next_turn(const int (&m)[8], int& s, int& i, int& ms)
{
    i += T * 8;
    if (i < ms) return;
    i = 0;
    do { s++; ms = pick8(m, s); } while (s < 8 && ms == 0);
}

template <int T>
__device__ inline void load_turn(ulonglong2 (&q)[8], const ulonglong2* p, int i, int ms)
{
    #pragma unroll
    for (int j = 0; j < 8; j++) {
        const int idx = i + (int)threadIdx.x + T * j;
        q[j] = p[idx < ms ? idx : ms - 1];
    }
}

template <int T>
__device__ inline void acc_turn(Slot* tab, const ulonglong2 (&q)[8], int i, int ms)
{
    #pragma unroll
    for (int j = 0; j < 8; j++)
        if (i + (int)threadIdx.x + T * j < ms) { add1(tab, q[j].x); add1(tab, q[j].y); }
}

template <int T>
__global__ void __launch_bounds__(T)
k_candidate(const uint64_t* recs, const unsigned long long* cursors,
            unsigned long long* wg_counts)
{
    __shared__ __attribute__((aligned(16))) unsigned long long tabw[2 * kSlots];
    __shared__ unsigned long long red[1];
    Slot* tab = (Slot*)tabw;
    const int tid = threadIdx.x, bucket = blockIdx.x;
    for (int i = tid; i < 2 * kSlots; i += T) tabw[i] = 0;
    __syncthreads();
    const uint64_t* region0 = recs + (int64_t)bucket * kSub * kStride;
    int m[8];
    #pragma unroll
    for (int s = 0; s < 8; s++) m[s] = (int)cursors[s * kNB + bucket] >> 1;
    ulonglong2 a[8], b[8];
    int s0 = -1, i0 = 0, m0 = 0;
    next_turn<T>(m, s0, i0, m0);
    if (s0 < 8) {
        load_turn<T>(a, (const ulonglong2*)(region0 + s0 * kStride), i0, m0);
        for (;;) {
            int s1 = s0, i1 = i0, m1 = m0;
            next_turn<T>(m, s1, i1, m1);
            const bool more1 = s1 < 8;
            if (!more1) { s1 = s0; i1 = i0; m1 = m0; }
            load_turn<T>(b, (const ulonglong2*)(region0 + s1 * kStride), i1, m1);
            acc_turn<T>(tab, a, i0, m0);
            if (!more1) break;
            s0 = s1; i0 = i1; m0 = m1;
            next_turn<T>(m, s0, i0, m0);
            const bool more0 = s0 < 8;
            if (!more0) { s0 = s1; i0 = i1; m0 = m1; }
            load_turn<T>(a, (const ulonglong2*)(region0 + s0 * kStride), i0, m0);
            acc_turn<T>(tab, b, i1, m1);
            if (!more0) break;
        }
    }
    if (tid < kSub) {
        const int64_t n = (int64_t)cursors[tid * kNB + bucket];
        if (n & 1) add1(tab, (region0 + tid * kStride)[n - 1]);
    }
    __syncthreads();
    report<T>(tabw + 1, 2, 0, wg_counts, red);
}

/* the flushes: slot i of workgroup b is non-empty iff i is even; a group is
 * {key, cnt, sum, nonnull}, 32 bytes */
__global__ void __launch_bounds__(256)
k_flush0(ulonglong2* out, unsigned long long* counter, unsigned long long* ngroups, int64_t cap)
{
    __shared__ unsigned long long cntnn[kSlots], sums[kSlots];
    const int tid = threadIdx.x;
    for (int i = tid; i < kSlots; i += 256) { cntnn[i] = (i & 1) ? 0 : (1ULL | 1ULL << 32); sums[i] = i; }
    __syncthreads();
    for (int i = tid; i < kSlots; i += 256) {
        const uint64_t cn = cntnn[i];
        if (!cn) continue;
        const unsigned long long idx = atomicAdd(counter, 1ULL);
        const unsigned long long t = atomicAdd(ngroups, 1ULL);
        if ((int64_t)idx >= cap || t == ~0ULL) continue;
        out[2 * idx] = make_ulonglong2((uint64_t)blockIdx.x * kSlots + i, cn & 0xFFFFFFFFULL);
        out[2 * idx + 1] = make_ulonglong2(sums[i], cn >> 32);
    }
}

__global__ void __launch_bounds__(256)
k_flush1(ulonglong2* out, unsigned long long* counter, unsigned long long* ngroups, int64_t cap)
{
    __shared__ unsigned long long cntnn[kSlots], sums[kSlots];
    __shared__ unsigned long long scanw[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < kSlots; i += 256) { cntnn[i] = (i & 1) ? 0 : (1ULL | 1ULL << 32); sums[i] = i; }
    __syncthreads();
    constexpr int cpw = kSlots / 64 / 4;
    unsigned mine = 0;
    for (int c = wave * cpw; c < (wave + 1) * cpw; c++)
        mine += __popcll(__ballot(cntnn[c * 64 + lane] != 0));
    if (lane == 0) scanw[wave] = mine;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long n = scanw[0] + scanw[1] + scanw[2] + scanw[3];
        unsigned long long idx = 0;
        if (n) { idx = atomicAdd(counter, n); atomicAdd(ngroups, n); }
        scanw[4] = idx;
    }
    __syncthreads();
    unsigned long long at = scanw[4];
    for (int w = 0; w < wave; w++) at += scanw[w];
    for (int c = wave * cpw; c < (wave + 1) * cpw; c++) {
        const int i = c * 64 + lane;
        const uint64_t cn = cntnn[i];
        const unsigned long long bal = __ballot(cn != 0);
        const unsigned long long idx = at + __popcll(bal & ((1ULL << lane) - 1));
        at += __popcll(bal);
        if (!cn || (int64_t)idx >= cap) continue;
        out[2 * idx] = make_ulonglong2((uint64_t)blockIdx.x * kSlots + i, cn & 0xFFFFFFFFULL);
        out[2 * idx + 1] = make_ulonglong2(sums[i], cn >> 32);
    }
}

struct Bufs {
    uint64_t* recs; unsigned long long *cursors, *wg_counts, *sink, *counter, *ngroups;
    ulonglong2* groups;
};
constexpr int64_t kGroups = (int64_t)kNB * kSlots / 2;

static float timed(int v, const Bufs& b)
{
    hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    CHK(hipMemset(b.wg_counts, 0, 8 * kNB));
    CHK(hipMemset(b.counter, 0, 8)); CHK(hipMemset(b.ngroups, 0, 8));
    CHK(hipMemset(b.groups, 0xFF, 32 * kGroups));
    CHK(hipEventRecord(e0, 0));
    switch (v) {
    case 0: hipLaunchKernelGGL(k_shipped<0>, dim3(kNB), dim3(256), 0, 0, b.recs, b.cursors, b.wg_counts, b.sink); break;
    case 1: hipLaunchKernelGGL(k_adds<2>, dim3(kNB), dim3(256), 0, 0, b.wg_counts); break;
    case 2: hipLaunchKernelGGL(k_adds<3>, dim3(kNB), dim3(256), 0, 0, b.wg_counts); break;
    case 3: hipLaunchKernelGGL(k_shipped<1>, dim3(kNB), dim3(256), 0, 0, b.recs, b.cursors, b.wg_counts, b.sink); break;
    case 4: hipLaunchKernelGGL(k_candidate<256>, dim3(kNB), dim3(256), 0, 0, b.recs, b.cursors, b.wg_counts); break;
    case 5: hipLaunchKernelGGL(k_candidate<512>, dim3(kNB), dim3(512), 0, 0, b.recs, b.cursors, b.wg_counts); break;
    case 6: hipLaunchKernelGGL(k_flush0, dim3(kNB), dim3(256), 0, 0, b.groups, b.counter, b.ngroups, kGroups); break;
    default: hipLaunchKernelGGL(k_flush1, dim3(kNB), dim3(256), 0, 0, b.groups, b.counter, b.ngroups, kGroups); break;
    }
    CHK(hipGetLastError());
    CHK(hipEventRecord(e1, 0));
    CHK(hipDeviceSynchronize());
    float ms; CHK(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0); hipEventDestroy(e1);
    if (v < 6) {
        std::vector<unsigned long long> h(kNB);
        CHK(hipMemcpy(h.data(), b.wg_counts, 8 * kNB, hipMemcpyDeviceToHost));
        unsigned long long s = 0;
        for (unsigned long long c : h) s += c;
        if (s != (unsigned long long)kRecords) { printf("variant %d: %llu records counted, %lld expected\n", v, s, (long long)kRecords); exit(1); }
    } else {
        unsigned long long c[2];
        CHK(hipMemcpy(&c[0], b.counter, 8, hipMemcpyDeviceToHost));
        CHK(hipMemcpy(&c[1], b.ngroups, 8, hipMemcpyDeviceToHost));
        std::vector<ulonglong2> g(2 * kGroups);
        CHK(hipMemcpy(g.data(), b.groups, 32 * kGroups, hipMemcpyDeviceToHost));
        std::vector<unsigned char> seen((size_t)kNB * kSlots, 0);
        bool ok = c[0] == (unsigned long long)kGroups && c[1] == c[0];
        for (int64_t i = 0; ok && i < kGroups; i++) {
            const uint64_t key = g[2 * i].x;
            ok = key < (uint64_t)kNB * kSlots && !(key & 1) && !seen[key] && g[2 * i].y == 1
                 && g[2 * i + 1].x == (key & (kSlots - 1)) && g[2 * i + 1].y == 1;
            if (ok) seen[key] = 1;
        }
        if (!ok) { printf("variant %d: groups wrong\n", v); exit(1); }
    }
    return ms;
}

int main()
{
    Bufs b;
    CHK(hipMalloc(&b.recs, (size_t)kNB * kSub * kStride * 8));
    CHK(hipMalloc(&b.cursors, 8 * kNB * kSub));
    CHK(hipMalloc(&b.wg_counts, 8 * kNB));
    CHK(hipMalloc(&b.sink, 8));
    CHK(hipMalloc(&b.counter, 8));
    CHK(hipMalloc(&b.ngroups, 8));
    CHK(hipMalloc(&b.groups, 32 * kGroups));
    hipLaunchKernelGGL(k_fill, dim3(kNB * kSub), dim3(256), 0, 0, b.recs, b.cursors);
    CHK(hipDeviceSynchronize());
    const char* name[8] = {"L    r2 loop, loads only", "A2   adds only, 2 x u64", "A1   adds only, u32 + u64",
                           "S    r2 loop", "P    candidate loop", "P512 candidate, 512 threads",
                           "F0   flush, add per group", "F1   flush, add per workgroup"};
    const double bytes = (double)kRecords * 8;
    for (int rep = 0; rep < 3; rep++) {
        for (int v = 0; v < 8; v++) {
            const float ms = timed(v, b);
            if (v == 1 || v == 2)
                printf("rep %d  %-30s %9.1f us  %7.2f G adds/s\n", rep, name[v], ms * 1e3, 2.0 * kRecords / (ms * 1e6));
            else if (v >= 6)
                printf("rep %d  %-30s %9.1f us  %7.1f M groups/s\n", rep, name[v], ms * 1e3, kGroups / (ms * 1e3));
            else
                printf("rep %d  %-30s %9.1f us  %7.2f TB/s\n", rep, name[v], ms * 1e3, bytes / (ms * 1e9));
        }
    }
    return 0;
}
