/* probe: what do phase A's per-tile reservations cost? 2048 workgroups of 512
 * threads; a workgroup does `tiles` rounds of 1024 returning adds (two per
 * thread, one per bucket) into a cursor table of 1024 buckets x 8 subs, a
 * barrier per round as in k_scan_partition. Variants:
 *   a   [bucket][sub] u64, thread t on buckets 2t, 2t+1, a wait after each add
 *   b   the same addresses, both adds issued, then one wait
 *   c   [sub][bucket] u64, thread t on buckets t, t+512: a wave on adjacent words
 *   c2  [sub][bucket] u64, thread t on buckets 2t, 2t+1: a wave on 1 KiB
 *   d   c with u32 cursors
 * Prints ms, adds/s and us per round of a resident workgroup (512 resident).
 * hipcc --offload-arch=gfx950 -O3 -o probe_reserve probe_reserve.hip */
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHK(x) do { hipError_t e=(x); if(e){printf("HIP %s @%d\n", hipGetErrorString(e), __LINE__); exit(1);} } while(0)

constexpr int kNB = 1024, kSub = 8, kThreads = 512, kGrid = 2048;

template <int V>
__global__ void __launch_bounds__(kThreads)
k_reserve(unsigned long long* cur, unsigned* cur32, int tiles, unsigned long long* sink)
{
    const int t = threadIdx.x, sub = blockIdx.x & 7;
    unsigned long long acc = 0;
    for (int i = 0; i < tiles; i++) {
        if (V == 0) {
            unsigned long long r0 = atomicAdd(&cur[(2 * t) * kSub + sub], 1ULL);
            /* the second add's operand needs the first one's result */
            unsigned long long r1 = atomicAdd(&cur[(2 * t + 1) * kSub + sub], 1ULL + (r0 >> 63));
            acc += r0 + r1;
        } else if (V == 1) {
            unsigned long long r0 = atomicAdd(&cur[(2 * t) * kSub + sub], 1ULL);
            unsigned long long r1 = atomicAdd(&cur[(2 * t + 1) * kSub + sub], 1ULL);
            acc += r0 + r1;
        } else if (V == 2) {
            unsigned long long r0 = atomicAdd(&cur[sub * kNB + t], 1ULL);
            unsigned long long r1 = atomicAdd(&cur[sub * kNB + t + kThreads], 1ULL);
            acc += r0 + r1;
        } else if (V == 3) {
            unsigned long long r0 = atomicAdd(&cur[sub * kNB + 2 * t], 1ULL);
            unsigned long long r1 = atomicAdd(&cur[sub * kNB + 2 * t + 1], 1ULL);
            acc += r0 + r1;
        } else {
            unsigned r0 = atomicAdd(&cur32[sub * kNB + t], 1u);
            unsigned r1 = atomicAdd(&cur32[sub * kNB + t + kThreads], 1u);
            acc += r0 + r1;
        }
        __syncthreads();
    }
    if (acc == ~0ULL) sink[0] = acc;   /* keeps the results live; never true */
}

template <int V>
static float run1(unsigned long long* cur, unsigned* cur32, int tiles, unsigned long long* sink)
{
    hipEvent_t a, b; CHK(hipEventCreate(&a)); CHK(hipEventCreate(&b));
    CHK(hipMemset(cur, 0, sizeof(unsigned long long) * kNB * kSub));
    CHK(hipMemset(cur32, 0, sizeof(unsigned) * kNB * kSub));
    CHK(hipEventRecord(a, 0));
    hipLaunchKernelGGL(k_reserve<V>, dim3(kGrid), dim3(kThreads), 0, 0, cur, cur32, tiles, sink);
    CHK(hipEventRecord(b, 0));
    CHK(hipDeviceSynchronize());
    float ms; CHK(hipEventElapsedTime(&ms, a, b));
    hipEventDestroy(a); hipEventDestroy(b);
    /* every add must have landed: the table sums to the number of adds */
    std::vector<unsigned long long> h(kNB * kSub);
    std::vector<unsigned> h32(kNB * kSub);
    CHK(hipMemcpy(h.data(), cur, h.size() * 8, hipMemcpyDeviceToHost));
    CHK(hipMemcpy(h32.data(), cur32, h32.size() * 4, hipMemcpyDeviceToHost));
    unsigned long long s = 0;
    for (size_t i = 0; i < h.size(); i++) s += h[i] + h32[i];
    if (s != (unsigned long long)kGrid * kNB * tiles) { printf("variant %d: sum %llu wrong\n", V, s); exit(1); }
    return ms;
}

int main(int argc, char** argv)
{
    const int tiles = argc > 1 ? atoi(argv[1]) : 60;   /* 122,880 rounds in all */
    unsigned long long *cur, *sink; unsigned* cur32;
    CHK(hipMalloc(&cur, sizeof(unsigned long long) * kNB * kSub));
    CHK(hipMalloc(&cur32, sizeof(unsigned) * kNB * kSub));
    CHK(hipMalloc(&sink, 8));
    const char* name[5] = {"a  [b][sub] u64, wait each", "b  [b][sub] u64, one wait",
                           "c  [sub][b] u64, t / t+512", "c2 [sub][b] u64, 2t / 2t+1",
                           "d  [sub][b] u32, t / t+512"};
    for (int rep = 0; rep < 3; rep++) {
        float ms[5] = {run1<0>(cur, cur32, tiles, sink), run1<1>(cur, cur32, tiles, sink),
                       run1<2>(cur, cur32, tiles, sink), run1<3>(cur, cur32, tiles, sink),
                       run1<4>(cur, cur32, tiles, sink)};
        for (int v = 0; v < 5; v++) {
            double adds = (double)kGrid * kNB * tiles;
            printf("rep %d  %-28s %8.3f ms  %7.2f G adds/s  %6.2f us/round\n", rep, name[v],
                   ms[v], adds / (ms[v] * 1e6), ms[v] * 1e3 * 512 / ((double)kGrid * tiles));
        }
    }
    return 0;
}
