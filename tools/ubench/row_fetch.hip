// What does the SHAPE of the fused launch's row fetch cost?  Every block of a launch pulls the whole partial table of the launch before it
// (256 rows x 32 doubles = 64 KB) and sums it per column in a fixed order before anything else can happen (stage_pending).  Three forms
// of the same fetch, same sums:
//   A  all 16 waves, thread = (row group q = t / 32, value v = t % 32), 8 x 8-byte loads 8 KB apart          (128 wave requests of 512 B per CU)
//   B  waves 0-7, thread = (q = t / 16, value pair t % 16), 8 x 16-byte loads, scalar base + 32-bit offset    (64 requests of 1 KB)
//   C  a j-fastest table, table[q][v][j] (row = q + 32 j): all 16 waves, 4 x 16-byte loads of 64 consecutive bytes per thread
//      (64 requests of 1 KB ... as 4-KB-contiguous wave accesses); the producer's row store becomes 32 eight-byte stores at 64 B stride
//   N  no fetch at all (the stand-in pass alone)
// 256 blocks x 1024 threads; each block fetches + sums, spins ~10 us (a stand-in for the pass), then stores its row.  Back-to-back launches
// on ping-pong tables; time per launch from HIP events, and per block the time from kernel start to "sums in LDS" (s_memrealtime, 100 MHz,
// written to a buffer of its own; mean / max over the blocks of the last launch).
// build + run on the GPU box:  hipcc --offload-arch=gfx950 -O3 -o tools/ubench/row_fetch tools/ubench/row_fetch.hip && tools/ubench/row_fetch
#include <hip/hip_runtime.h>

#include <cstdio>

constexpr int kThreads = 1024, kVals = 32, kRows = 256, kGroups = 32, kBatches = kRows / kGroups;

struct alignas(16) D2 { double x, y; };

__device__ __forceinline__ double add_lane_xor(double v, const bool rows16) {      // v(lane) + v(lane ^ 32), or v(lane) + v(lane ^ 16)
    int lo = __double2loint(v), hi = __double2hiint(v), lo2 = lo, hi2 = hi;
    if (rows16) {
        asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(lo), "+v"(lo2));
        asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(hi), "+v"(hi2));
    } else {
        asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(lo), "+v"(lo2));
        asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(hi), "+v"(hi2));
    }
    return __hiloint2double(hi, lo) + __hiloint2double(hi2, lo2);
}

template <int FORM>      // 0: A, 1: B, 2: C, 3: N
__global__ __launch_bounds__(kThreads) void k_iter(const double* __restrict__ rows_in, double* __restrict__ rows_out,
                                                   unsigned* __restrict__ stamps, int spin_ticks, double* __restrict__ sink) {
    __shared__ double red[kThreads / 64][kVals];
    __shared__ double tot[kVals];
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
    const int tid = threadIdx.x;
    if (FORM == 0) {
        const int v = tid % kVals, q = tid / kVals;
        double tmp[kBatches];
#pragma unroll
        for (int j = 0; j < kBatches; ++j) tmp[j] = rows_in[(size_t)(q + kGroups * j) * kVals + v];
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < kBatches; ++j) s += tmp[j];
        const double pair = add_lane_xor(s, false);
        if ((tid & 63) < kVals) red[tid >> 6][tid & 31] = pair;
    } else if (FORM == 1) {
        if (__builtin_amdgcn_readfirstlane(tid) < kThreads / 2) {
            D2 tmp[kBatches];
#pragma unroll
            for (int j = 0; j < kBatches; ++j) {
                unsigned step = j * (kGroups * kVals * 8), off = (unsigned)tid * 16u;      // (the asm statements: see stage_pending)
                asm("" : "+s"(step));
                asm("" : "+v"(off));
                tmp[j] = *reinterpret_cast<const D2*>(reinterpret_cast<const char*>(rows_in) + step + off);
            }
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int j = 0; j < kBatches; ++j) { s0 += tmp[j].x; s1 += tmp[j].y; }
            const double p0 = add_lane_xor(s0, true), p1 = add_lane_xor(s1, true);
            if ((tid & 16) == 0) {
                red[tid >> 5][2 * (tid & 15)] = p0;
                red[tid >> 5][2 * (tid & 15) + 1] = p1;
            }
        }
    } else if (FORM == 2) {
        const D2* p = reinterpret_cast<const D2*>(rows_in) + (size_t)tid * (kBatches / 2);      // (q, v) = (tid / 32, tid % 32): 64 consecutive bytes
        D2 tmp[kBatches / 2];
#pragma unroll
        for (int j = 0; j < kBatches / 2; ++j) tmp[j] = p[j];
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < kBatches / 2; ++j) { s += tmp[j].x; s += tmp[j].y; }
        const double pair = add_lane_xor(s, false);
        if ((tid & 63) < kVals) red[tid >> 6][tid & 31] = pair;
    } else {
        if ((tid & 63) < kVals) red[tid >> 6][tid & 31] = 1.0;
    }
    __syncthreads();
    if (tid == 0) stamps[blockIdx.x] = (unsigned)(__builtin_amdgcn_s_memrealtime() - t_start);      // sums in LDS, on every wave
    if (tid < kVals) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < kThreads / 64; ++k) t += red[k][tid];
        tot[tid] = t;
    }
    __syncthreads();
    const double pose = tot[0] + tot[5] + tot[31];
    // the "pass"
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned long long)spin_ticks) __builtin_amdgcn_s_sleep(4);
    if (tid < kVals) {
        const double val = pose * 1e-9 + (double)(blockIdx.x + tid);
        const int b = blockIdx.x;
        if (FORM == 2) rows_out[((size_t)(b % kGroups) * kVals + tid) * kBatches + b / kGroups] = val;      // table[q][v][j]
        else rows_out[(size_t)b * kVals + tid] = val;
    }
    if (blockIdx.x == 0 && tid == 0) *sink = pose;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <int FORM>
static int run(const char* name, int spin_us, double* const rows[2], unsigned* stamps, double* sink, hipEvent_t e0, hipEvent_t e1) {
    const int iters = 2000;
    float best = 1e30f;
    for (int rep = 0; rep < 4; ++rep) {      // the first repetition warms up
        CK(hipEventRecord(e0));
        for (int it = 0; it < iters; ++it)
            hipLaunchKernelGGL(k_iter<FORM>, dim3(kRows), dim3(kThreads), 0, 0, rows[it & 1], rows[(it + 1) & 1], stamps, spin_us * 100, sink);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep && ms < best) best = ms;
    }
    unsigned h[kRows];
    CK(hipMemcpy(h, stamps, sizeof(h), hipMemcpyDeviceToHost));
    double mean = 0.0;
    unsigned mx = 0;
    for (int b = 0; b < kRows; ++b) { mean += h[b]; mx = h[b] > mx ? h[b] : mx; }
    printf("pass stand-in %2d us | form %s | %7.3f us / launch | kernel start -> sums in LDS: mean %.3f us, max %.2f us over %d blocks\n", spin_us, name,
           best * 1e3 / iters, mean / kRows / 100.0, mx / 100.0, kRows);
    return 0;
}

int main() {
    double *rows[2], *sink;
    unsigned* stamps;
    for (int k = 0; k < 2; ++k) { CK(hipMalloc(&rows[k], kRows * kVals * 8)); CK(hipMemset(rows[k], 0, kRows * kVals * 8)); }
    CK(hipMalloc(&stamps, kRows * sizeof(unsigned)));
    CK(hipMalloc(&sink, 8));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int round = 0; round < 3; ++round) {      // the forms in turns: a drift of the clocks shows as a drift of all four
        for (int spin_us : {10, 0}) {
            if (run<0>("A  16 waves x 8 x  8 B", spin_us, rows, stamps, sink, e0, e1)) return 1;
            if (run<1>("B   8 waves x 8 x 16 B", spin_us, rows, stamps, sink, e0, e1)) return 1;
            if (run<2>("C  16 waves x 4 x 16 B", spin_us, rows, stamps, sink, e0, e1)) return 1;
            if (run<3>("N  no fetch           ", spin_us, rows, stamps, sink, e0, e1)) return 1;
        }
    }
    return 0;
}
