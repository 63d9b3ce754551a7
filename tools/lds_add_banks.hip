// lds_add_banks.hip -- how gfx950 banks a no-return LDS add of a double (ds_add_f64), the add
// k_pr_pull_units spends its LDS time in.  Stand-alone:
//   hipcc --offload-arch=gfx950 -O3 tools/lds_add_banks.hip -o lds_add_banks && ./lds_add_banks
// One workgroup of 1024 threads per CU adds 1.0 into 16 Ki LDS doubles in a timed loop, every
// lane to the row a lane -> row map names (each wave inside its own 1024 rows), and prints the
// s_memtime ticks per wave-instruction and CU for each map, beside what three hypotheses predict
// in LDS-array cycles:
//   H16  groups of 16 contiguous lanes, slot = row mod 16, equal addresses serialise
//   H16b the same, equal addresses combine
//   H32  groups of 32 contiguous lanes, slot = row mod 32 (as ds_read_b64), equal addresses serialise
// Ticks are not LDS cycles; the identity map gives the scale (4 cycles under H16, 2 under H32).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                              \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                      \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

constexpr int kBS = 1024, kWave = 64, kRows = 16384, kUnroll = 8;

struct Map {
    const char *name;
    int (*row)(int lane);
};

// rows below 1024 for every lane
static const Map kMaps[] = {
    {"identity                       r = l", [](int l) { return l; }},
    {"one slot, 64 rows              r = 16 l", [](int l) { return 16 * l; }},
    {"2-way per group                r = (l & 7) + 16 (l >> 3)", [](int l) { return (l & 7) + 16 * (l >> 3); }},
    {"4-way per group                r = (l & 3) + 16 (l >> 2)", [](int l) { return (l & 3) + 16 * (l >> 2); }},
    {"stride 2                       r = 2 l", [](int l) { return 2 * l; }},
    {"stride 4                       r = 4 l", [](int l) { return 4 * l; }},
    {"stride 8                       r = 8 l", [](int l) { return 8 * l; }},
    {"lanes l, l + 16 share a slot   r = (l & 15) + 16 (l >> 4)", [](int l) { return (l & 15) + 16 * (l >> 4); }},
    {"lanes l, l + 32 share a slot   r = (l & 31) + 32 (l >> 5)", [](int l) { return (l & 31) + 32 * (l >> 5); }},
    {"neighbours share a slot        r = (l >> 2) + 16 (l & 3)", [](int l) { return (l >> 2) + 16 * (l & 3); }},
    {"rows r, r + 16 alternate       r = (l >> 1) + 16 (l & 1)", [](int l) { return (l >> 1) + 16 * (l & 1); }},
    {"same address, 2 lanes          r = l >> 1", [](int l) { return l >> 1; }},
    {"same address, 4 lanes          r = l >> 2", [](int l) { return l >> 2; }},
    {"same address, 16 lanes         r = l >> 4", [](int l) { return l >> 4; }},
    {"same address, all lanes        r = 0", [](int) { return 0; }},
};

// LDS-array cycles of one wave-instruction: per group of G lanes, the largest number of accesses
// one slot (row mod S) serves; equal rows count once when `combine`.
static int predict(const int *row, int G, int S, bool combine) {
    int cycles = 0;
    for (int g0 = 0; g0 < kWave; g0 += G) {
        int worst = 0;
        for (int s = 0; s < S; s++) {
            std::vector<int> seen;
            for (int l = g0; l < g0 + G; l++)
                if (row[l] % S == s && !(combine && std::count(seen.begin(), seen.end(), row[l]))) seen.push_back(row[l]);
            worst = std::max<int>(worst, (int)seen.size());
        }
        cycles += std::max(worst, 1);
    }
    return cycles;
}

__global__ __launch_bounds__(kBS) void k_lds_add(const int *__restrict__ rowmap, int iters, unsigned long long *ticks, double *sink) {
    extern __shared__ double acc[];
    const int tid = threadIdx.x;
    for (int i = tid; i < kRows; i += kBS) acc[i] = 0.0;
    double *mine = acc + (tid / kWave) * (kRows / (kBS / kWave)) + rowmap[tid & (kWave - 1)];
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int u = 0; u < kUnroll; u++) atomicAdd(mine, 1.0);   // result unused: the no-return add
    }
    __syncthreads();   // every wave's adds have been served (lgkmcnt(0) before the barrier)
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (tid == 0) ticks[blockIdx.x] = t1 - t0;
    if (tid < kWave) sink[(size_t)blockIdx.x * kWave + tid] = acc[tid];   // keeps the adds observable
}

int main(int argc, char **argv) {
    const int iters = argc > 1 ? std::max(1, std::atoi(argv[1])) : 2048;
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    const size_t lds = (size_t)kRows * sizeof(double);
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_lds_add), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int *d_map = nullptr;
    unsigned long long *d_ticks = nullptr;
    double *d_sink = nullptr;
    CHECK(hipMalloc(&d_map, kWave * sizeof(int)));
    CHECK(hipMalloc(&d_ticks, (size_t)cus * sizeof(unsigned long long)));
    CHECK(hipMalloc(&d_sink, (size_t)cus * kWave * sizeof(double)));
    std::printf("%s, %d CUs, %d iterations x %d adds per lane, %d waves per CU\n", prop.gcnArchName, cus, iters, kUnroll,
                kBS / kWave);
    std::printf("%-60s %10s %10s   %4s %4s %4s\n", "lane -> row map", "ticks/inst", "x identity", "H16", "H16b", "H32");
    double ident = 0.0;
    for (size_t m = 0; m < sizeof kMaps / sizeof kMaps[0]; m++) {
        int row[kWave];
        for (int l = 0; l < kWave; l++) {
            row[l] = kMaps[m].row(l);
            if (row[l] < 0 || row[l] >= kRows / (kBS / kWave)) {   // inside the wave's rows
                std::fprintf(stderr, "map %zu: row %d out of range\n", m, row[l]);
                return 1;
            }
        }
        CHECK(hipMemcpy(d_map, row, sizeof row, hipMemcpyHostToDevice));
        std::vector<unsigned long long> t(cus);
        double best = 0.0;
        for (int rep = 0; rep < 3; rep++) {   // the first launch warms the clocks; the fastest counts
            hipLaunchKernelGGL(k_lds_add, dim3(cus), dim3(kBS), lds, 0, d_map, iters, d_ticks, d_sink);
            CHECK(hipGetLastError());
            CHECK(hipDeviceSynchronize());
            CHECK(hipMemcpy(t.data(), d_ticks, t.size() * sizeof t[0], hipMemcpyDeviceToHost));
            std::sort(t.begin(), t.end());
            const double per = (double)t[t.size() / 2] / ((double)iters * kUnroll * (kBS / kWave));   // median CU
            if (rep == 0 || per < best) best = per;
        }
        if (m == 0) ident = best;
        std::printf("%-60s %10.3f %10.2f   %4d %4d %4d\n", kMaps[m].name, best, best / ident, predict(row, 16, 16, false),
                    predict(row, 16, 16, true), predict(row, 32, 32, false));
    }
    CHECK(hipFree(d_map));
    CHECK(hipFree(d_ticks));
    CHECK(hipFree(d_sink));
    return 0;
}
