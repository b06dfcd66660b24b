// LDS integer atomics on gfx950: clocks per wave-instruction per CU (whole-workgroup timing: 16 waves, one workgroup, as lds.hip), no-return
// ds_add_u32 / ds_add_u64 / ds_max_u32 at four address patterns -- what a histogram in LDS meets:
//   spread   every lane its own element (conflict-free)
//   32 bins  lane % 32: two lanes an address, the addresses side by side -- a diffuse stereo field
//   3 bins   lane % 3: real music, most frames in two or three sectors
//   1 bin    every lane the same address -- an all-mono file
// Every wave of the workgroup uses the same table (TABLES = 1) or a table of its own (TABLES = 16).
//   hipcc --offload-arch=gfx950 -O3 -o tools/ubench/lds_atomics tools/ubench/lds_atomics.hip && tools/ubench/lds_atomics
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>
#define REP16(X) X X X X X X X X X X X X X X X X
template <int OP, int PATTERN, int TABLES>
__global__ void __launch_bounds__(1024) k(long long *clk, unsigned *out)
{
    extern __shared__ unsigned lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned width = OP == 1 ? 8 : 4;
    const unsigned element = PATTERN == 0 ? unsigned(lane) : PATTERN == 1 ? unsigned(lane % 32) : PATTERN == 2 ? unsigned(lane % 3) : 0u;
    const unsigned addr = (TABLES == 1 ? 0u : unsigned(wave) * 64u * width) + element * width;
    const unsigned v = unsigned(tid) + 1u;
    const unsigned long long v2 = (unsigned long long)(tid) + 1ull;
    for (int i = tid; i < 16384; i += 1024) lds[i] = 0u;
    __syncthreads();
    const long long t0 = __builtin_readcyclecounter();
#pragma unroll 1
    for (int it = 0; it < 64; ++it) {
        if (OP == 0) { REP16(asm volatile("ds_add_u32 %0, %1" :: "v"(addr), "v"(v) : "memory");) }
        if (OP == 1) { REP16(asm volatile("ds_add_u64 %0, %1" :: "v"(addr), "v"(v2) : "memory");) }
        if (OP == 2) { REP16(asm volatile("ds_max_u32 %0, %1" :: "v"(addr), "v"(v) : "memory");) }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const long long t1 = __builtin_readcyclecounter();
    if (lane == 0) { clk[2 * wave] = t0; clk[2 * wave + 1] = t1; }
    __syncthreads();
    out[tid] = lds[tid];
}
template <int OP, int PATTERN, int TABLES>
static void run(const char *name, long long *d_clk, unsigned *d_out)
{
    static const char *patterns[] = {"spread", "32 bins", "3 bins", "1 bin"};
    std::vector<long long> h(32);
    double best = 1e30;
    for (int rep = 0; rep < 5; ++rep) {
        hipLaunchKernelGGL((k<OP, PATTERN, TABLES>), dim3(1), dim3(1024), 65536, 0, d_clk, d_out);
        hipDeviceSynchronize();
        hipMemcpy(h.data(), d_clk, 32 * sizeof(long long), hipMemcpyDeviceToHost);
        long long lo = h[0], hi = h[1];
        for (int w = 0; w < 16; ++w) { lo = std::min(lo, h[2 * w]); hi = std::max(hi, h[2 * w + 1]); }
        best = std::min(best, double(hi - lo));
    }
    printf("%-12s %-8s %2d table(s) %8.2f clk / wave-instruction / CU\n", name, patterns[PATTERN], TABLES, best / (64.0 * 16 * 16));
}
template <int OP>
static void all(const char *name, long long *d_clk, unsigned *d_out)
{
    run<OP, 0, 1>(name, d_clk, d_out); run<OP, 1, 1>(name, d_clk, d_out); run<OP, 2, 1>(name, d_clk, d_out); run<OP, 3, 1>(name, d_clk, d_out);
    run<OP, 0, 16>(name, d_clk, d_out); run<OP, 1, 16>(name, d_clk, d_out); run<OP, 2, 16>(name, d_clk, d_out); run<OP, 3, 16>(name, d_clk, d_out);
}
int main()
{
    long long *d_clk; unsigned *d_out;
    hipMalloc(&d_clk, 32 * sizeof(long long)); hipMalloc(&d_out, 1024 * sizeof(unsigned));
    all<0>("ds_add_u32", d_clk, d_out);
    all<1>("ds_add_u64", d_clk, d_out);
    all<2>("ds_max_u32", d_clk, d_out);
    return 0;
}
