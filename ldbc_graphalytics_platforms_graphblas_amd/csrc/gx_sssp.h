// gx_sssp.h -- what the two SSSP files share: the bucket constants and device helpers, the knobs
// and the per-graph rules (mean weight, non-isolated vertices, bucket width, pull threshold,
// fusion bound).  gx_sssp.hip is the single-device driver with its kernels and defines the
// functions declared here; gx_sssp_split.hip is the 1-D split (one rank's slice and rounds).
// Where the two paths differ, the difference is written down at the knob's field below.
#pragma once

#include <algorithm>
#include <cstdlib>

#include "gx_device.h"

namespace gx {

constexpr int kRing = 32;     // bucket ring slots
constexpr int kChunk = 256;   // edges per relax item (vertex << 32 | chunk)

// Distances are non-negative fp64 kept as their IEEE bit patterns (unsigned order = numeric order).
__device__ __forceinline__ unsigned long long dbits(double d) {
    return (unsigned long long)__double_as_longlong(d);
}
__device__ __forceinline__ double bitsd(unsigned long long b) { return __longlong_as_double((long long)b); }

// bucket(d) = floor(d / delta), clamped: an infinite or huge distance stays a valid int64
constexpr long long kMaxBucket = 4000000000000000000ll;
__device__ __forceinline__ int64_t bucket_of(double d, double inv_delta) {
    const double q = d * inv_delta;
    return q < 4.0e18 ? (int64_t)q : (int64_t)kMaxBucket;
}

// A bucket number as a per-vertex stamp: its low 31 bits, so never negative.  A vertex is stamped
// only for buckets of the current ring window, and a later stamp names a lower bucket that is
// still ahead of `cur`, so two stamps of one vertex lie fewer than 2 kRing buckets apart and 31
// bits tell them apart.  The "never stamped" state is a word no bucket produces: negative on the
// single path (bstamp -1, the bucket half of nsw all ones), 0 on the split, whose tags are
// ~stamp_of(b), always negative.
__device__ __forceinline__ int32_t stamp_of(int64_t b) { return (int32_t)((uint32_t)b & 0x7FFFFFFFu); }

// Relax items of a row part of `len` edges: gx_sssp queues none for an empty part, the split one.
__device__ __forceinline__ uint32_t chunks_of(int64_t len) { return (uint32_t)((len + kChunk - 1) / kChunk); }
__device__ __forceinline__ uint32_t chunks_min1(int64_t len) {
    return (uint32_t)max<int64_t>(1, (len + kChunk - 1) / kChunk);
}

// The SSSP knobs, read by sssp_knobs() and nowhere else: gx_sssp reads them at every call (tests
// flip them within one process), the split when it builds (gx_sssp_split_create, and the rebuild
// on the hub-first copy in the first gx_sssp_split_run) and, for split_verbose, at every run.
// Any positive bucket width and any grouping of buckets gives the same distances; the knobs only
// trade rounds for re-relaxations.  "split" below is gx_sssp_split.hip, "single" gx_sssp().
struct SsspKnobs {
    bool split;          // which path's defaults the fields hold
    double delta;        // GX_SSSP_DELTA: the bucket width itself; unset or not positive: sssp_delta's rule
    // GX_SSSP_DSCALE: the rule's scale, delta = dscale x mean weight / mean degree.  Directed: 0.5
    // on both paths.  Undirected, single: 2 -- measured on the SYN stand-ins with bucket fusion
    // (DESIGN.md 4): 2 for undirected graphs, whose big early buckets are pulled (round 5 re-sweep
    // after the dense opening, profiles/r05_sssp_dscale_sweep.txt: against 3, SYN-8_5 5.88 -> 5.61
    // ms, SYN-g500-22 3.56 -> 3.01, SYN-7_5 1.91 -> 1.80; round 3 had chosen 3 over 4).
    // Undirected, split: 3 -- SYN-8_5 N = 1: 9.3-9.4 ms at 3, 9.7 at 4.
    double dscale;
    // GX_SSSP_PULL: 0 a heavy phase is never pulled by its targets, 1 from pull_frac's threshold
    // (default), 2 always.  Directed graphs never pull: the field is 0.  Any other value reads as 0
    // on single and as 1 on the split.
    int pull;
    // GX_SSSP_PULL_FRAC (single only; default 8; not positive: never pull): a heavy phase whose
    // settled list holds at least 1 / pull_frac of the non-isolated vertices (rounded up) is
    // pulled.  8 rather than 4: the same times at the default bucket width, and no cliff below it
    // (a scale of 2-2.5 left SYN-8_5's first bucket short of 1/4 and pushed it: 14.8 ms; 8.2 at
    // 1/8).  The split does not read the variable: always 8, rounded down.
    double pull_frac;
    // GX_SSSP_FUSE: bucket fusion opens further ring buckets with the first non-empty one while
    // their entries together stay within this bound.  Single: unset the whole window (no bound),
    // 0 one bucket at a time.  Split: unset max(1024, n / 16), and 0 is clamped to 1 (which also
    // opens one bucket at a time: a non-empty bucket holds an entry).  sssp_fuse() resolves it.
    bool fuse_set;
    long long fuse;
    int32_t fuse_max;    // GX_SSSP_FUSE_MAX (single only): at most this many buckets fused, 1..kRing (default kRing)
    // GX_SSSP_DENSE (single only; default 16; 0 never): an opening of more than n / dense_div
    // entries scans the bucket stamps instead of the entries (k_sssp_advance).
    uint32_t dense_div;
    bool graph;          // GX_SSSP_GRAPH=0 (single only): batched launches instead of the replayed step graph
    // GX_SSSP_VERBOSE (single only): unset 0; set 1, a summary line per call on stderr; >= 2 also
    // one step per batch and a line per step (tools/sssp_steps.py).  1 and 2 run without the
    // replayed step graph.
    int verbose;
    bool split_verbose;  // GX_SPLIT_VERBOSE set (split only): gx_sssp_split_run prints its rounds per mode and the mode log
};

inline SsspKnobs sssp_knobs(bool directed, bool split) {
    auto real = [](const char *name, double dflt) {
        const char *e = std::getenv(name);
        return e ? std::atof(e) : dflt;
    };
    auto integer = [](const char *name, long long dflt) {
        const char *e = std::getenv(name);
        return e ? std::strtoll(e, nullptr, 10) : dflt;
    };
    SsspKnobs k;
    k.split = split;
    k.delta = real("GX_SSSP_DELTA", 0.0);
    k.dscale = real("GX_SSSP_DSCALE", directed ? 0.5 : split ? 3.0 : 2.0);
    const long long pull = integer("GX_SSSP_PULL", 1);
    k.pull = directed || pull == 0 ? 0 : pull == 2 ? 2 : (split || pull == 1) ? 1 : 0;
    k.pull_frac = split ? 8.0 : real("GX_SSSP_PULL_FRAC", 8.0);
    k.fuse_set = std::getenv("GX_SSSP_FUSE") != nullptr;
    k.fuse = integer("GX_SSSP_FUSE", 0);
    k.fuse_max = (int32_t)std::max<long long>(1, std::min<long long>(kRing, integer("GX_SSSP_FUSE_MAX", kRing)));
    k.dense_div = (uint32_t)integer("GX_SSSP_DENSE", 16);
    k.graph = integer("GX_SSSP_GRAPH", 1) != 0;
    k.verbose = !std::getenv("GX_SSSP_VERBOSE") ? 0 : integer("GX_SSSP_VERBOSE", 0) >= 2 ? 2 : 1;
    k.split_verbose = std::getenv("GX_SPLIT_VERBOSE") != nullptr;
    return k;
}

// Fills g->mean_w and g->nonisolated once per graph object (a hub-first copy has its own, summed
// in its own entry order, so a path's width does not depend on which path ran first).
int sssp_graph_stats(gx_graph *g, hipStream_t s);
// The one bucket-width rule; needs sssp_graph_stats.
double sssp_delta(const gx_graph *g, const SsspKnobs &k);
// Settled-list size from which a heavy phase is pulled (SsspState / SplitState::pull_min; never:
// single 0xFFFFFFFF, split 0); needs sssp_graph_stats.
uint32_t sssp_pull_min(const gx_graph *g, const SsspKnobs &k);
// Bucket fusion's entry bound (SsspState / SplitState::fuse).
uint32_t sssp_fuse(const gx_graph *g, const SsspKnobs &k);

}  // namespace gx
