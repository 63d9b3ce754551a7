// gx_lcc.h -- what the LCC files share: the tier constants and the packed-entry masks, the
// orientation / work-item / cache types, the knobs and the host functions that cross files.
// gx_lcc.hip is the driver (work items, the triangle tiers, gx_lcc), gx_lcc_orient.hip the
// orientation and its transpose, gx_lcc_dense.hip the dense core on the matrix cores,
// gx_lcc_part.hip the partitioned entry points (gx_lcc_part_*).
#pragma once

#include <string>
#include <vector>

#include "gx_device.h"

namespace gx {

constexpr int kLccBlock = 256;
constexpr int kWavesPerBlock = kLccBlock / kWave;
constexpr int kWaveMax = 256;          // wave tiers: |O(u)| <= 256 (512-slot tables) ...
constexpr int kWave2Max = 512;         // ... and <= 512 (1024-slot tables)
constexpr int kBlockMax = 8192;        // workgroup tier: table sized to the tier's largest |O(u)|
constexpr int kBlockSlots = 16384;     //   (dynamic LDS, at most 128 KiB)
constexpr uint32_t kVMask = (1u << 29) - 1;     // in-orientation entry: dense bit 31 | v << 2 | popcount
constexpr uint32_t kDenseBit = 1u << 31;

// Oriented entries are packed as (vertex << 2) | popcount(flag), so n < 2^29; `fn` is the entry
// point's name.
inline int lcc_check_size(uint64_t n, const char *fn) {
    if (n >= (1ull << 29))
        return fail(GX_NOT_IMPLEMENTED, std::string(fn) + ": more than 2^29 vertices (packed oriented entries)");
    return GX_SUCCESS;
}

// Degree-ordered orientation O of the closure S (CSR orp / ocode) and its transpose I
// (irp / icode, entries (v << 2) | popcount of the v -> u entry).
struct LccOrient {
    int64_t m = 0;
    DBuf<int64_t> orp, irp;
    DBuf<uint32_t> ocode, icode;
};

// The work items of the middle vertices in [v0, v1), by tier (k_lcc_items).
struct LccItems {
    DBuf<uint64_t> items0, items1, items2;
    DBuf<int32_t> big;
    std::vector<int32_t> h_big;
    uint32_t hc[5] = {0, 0, 0, 0, 0};   // items per tier, then the largest workgroup-tier |O(u)|
};

// What gx_lcc keeps on the graph between calls (gx_graph::lcc), next to the cached closure
// it is derived from: the orientation O, its transpose I and the work items (~2.2 ms of
// sorts, scans and host round trips per call on SYN-cit when rebuilt).
struct LccCache {
    LccOrient O;
    LccItems L;
    DBuf<unsigned long long> tc;
    DBuf<double> out;
    // dense core (GX_LCC_CORE = its largest size; 0: none)
    int32_t K = 0, Kp = 0;
    DBuf<int32_t> coreidx, corev;
    DBuf<int8_t> W, B;
    DBuf<uint8_t> tmask;
    DBuf<unsigned long long> tcore;
};

// The knobs, read by lcc_knobs (gx_lcc.hip) once at the top of an entry call and nowhere else.
// GX_LCC_WAVE_MAX / GX_LCC_WAVE2_MAX / GX_LCC_BLOCK_MAX can only lower kWaveMax / kWave2Max /
// kBlockMax (clamped to [1, the compile-time value], then wave <= wave2 <= block), so the static
// wave tables and the kBlockSlots cap hold whatever is set.  Tests use them to reach the
// workgroup tier and the merge fallback on small graphs.  gx_lcc hands the knobs to its cache
// build only, so they are latched with the cache; gx_lcc_part_counts cuts its items, and so
// applies the limits, at every call.
struct LccKnobs {
    int32_t wave_max, wave2_max, block_max;
    int32_t core;   // GX_LCC_CORE: the dense core's largest size (unset or 0: none)
};
LccKnobs lcc_knobs();

// gx_lcc_orient.hip
int lcc_orient(gx_graph *g, LccOrient &O, hipStream_t s);

// gx_lcc.hip
int lcc_items(const LccOrient &O, int64_t v0, int64_t v1, const LccKnobs &kn, LccItems &L, hipStream_t s);
// Adds the contributions of every triangle whose middle vertex is one of the items' into tc
// (n counters).
int lcc_count_items(gx_graph *g, const LccOrient &O, const LccItems &L, unsigned long long *tc, hipStream_t s);
// out[v] = tc[v] / (k (k - 1)) with k the closure degree srp[v + 1] - srp[v]; 0 when k < 2.
int lcc_finish(const int64_t *srp, const unsigned long long *tc, int64_t n, double *out, hipStream_t s);

// gx_lcc_dense.hip
int lcc_dense_build(gx_graph *g, LccCache &C, int32_t kmax, hipStream_t s);
int lcc_dense_count(gx_graph *g, LccCache &C, unsigned long long *tc, hipStream_t s);

}  // namespace gx
