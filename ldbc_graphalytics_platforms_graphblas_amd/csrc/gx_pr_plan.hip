// gx_pr_plan.hip -- the plan of the column-sorted PageRank iteration (pr_plan_sorted).
//
// This file owns what runs once per plan: the key, sort and pack kernels behind sci / spk / gbase,
// the orders inside a block (k_bank_order, k_sorted_laneperm), the cost, split, fill and emit
// kernels of the three code regions (runs, pairs, narrow), the launch simulation that picks the
// unit size, and pr_plan_sorted, a list of stages over one PlanCtx.  The tables' layout and the
// kernels that read them (k_pr_pull_units) are gx_pr_sorted.hip; gx_pr.h holds what both need.
#include <algorithm>
#include <cmath>
#include <functional>
#include <queue>
#include <thread>
#include <type_traits>
#include <cstdio>
#include <cstdlib>

#include "gx_pr.h"
#include "gx_pr_runs.h"
#include "gx_pr_bank.h"

namespace gx {
namespace {

// The plan's one radix sort.  The rows are cut into segments, in row order: the sorted blocks
// and each LONG row (a sorted block's rows, or one LONG row).  Entry e of local row i gets key
// (segment << colbits) | column and value i - (its segment's first row); sorted, every
// segment's entries keep its CSR range [rp[row_begin], rp[row_end]) and come out in column
// order.  Local row i is row order[i] of the source CSR with columns renamed perm[c]
// (gx_pagerank's hub-first relabelling, never materialised), or row i itself (order / perm
// null).  Sixteen entries per thread, the row found once by a binary search of the row
// pointers.
struct KeySrc {
    const int64_t *rp;          // local row pointers (the plan's, row order)
    int64_t rows;
    const int64_t *srp;         // source CSR
    const int32_t *sci;
    const int32_t *order;       // null: identity
    const int32_t *perm;        // null: columns as stored
    const int32_t *seg_row;     // nseg + 1 segment row starts
    int32_t nseg;
    int colbits;
    int32_t segmask;            // segment bits kept in the key (its sort group's share)
};

// The segment of every local row (one workgroup per segment; rows of skipped empty blocks fall
// in the segment before them and are never looked up: they hold no entry).
__global__ __launch_bounds__(256) void k_row_seg(const int32_t *__restrict__ seg_row, int32_t nseg, int32_t *rowseg) {
    for (int32_t sg = blockIdx.x; sg < nseg; sg += gridDim.x)
        for (int32_t r = seg_row[sg] + threadIdx.x; r < seg_row[sg + 1]; r += 256) rowseg[r] = sg;
}

// One wave per kKeyU 64-entry slabs of the plan's rows, lane = entry (coalesced key / row writes
// and row-contiguous column reads; the row by the slab shuffle search, gx_device.h
// slab_row_of, the segment from rowseg).  The slabs' chains (row -> source row -> column ->
// renamed column) are issued side by side: one slab at a time this kernel was a chain of
// ~15 dependent loads per slab (a binary search of the segments among them), ~10 ms on SYN-8_5.
constexpr int kKeyU = 4;

template <typename K>
__global__ __launch_bounds__(256) void k_sorted_keys(KeySrc k, int64_t nnz, const int64_t *__restrict__ srow,
                                                     int64_t nslabs, const int32_t *__restrict__ rowseg,
                                                     K *__restrict__ keys, uint16_t *__restrict__ vals) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t nw = (int64_t)gridDim.x * (256 / kWave);
    const int64_t nch = (nslabs + kKeyU - 1) / kKeyU;
    for (int64_t ch = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kWave; ch < nch; ch += nw) {
        int32_t i[kKeyU], sg[kKeyU], c0[kKeyU];
        int64_t rpi[kKeyU], sp[kKeyU];
        const int64_t e0 = ch * kKeyU * kWave + lane;   // lane's entry of slab u: e0 + u * kWave
#pragma unroll
        for (int u = 0; u < kKeyU; u++) {
            const int64_t sl = min(ch * kKeyU + u, nslabs - 1);
            i[u] = (int32_t)slab_row_of(k.rp, srow, k.rows, sl, min(e0 + u * kWave, nnz - 1), lane);
        }
#pragma unroll
        for (int u = 0; u < kKeyU; u++) {
            sg[u] = rowseg[i[u]];
            rpi[u] = k.rp[i[u]];
            sp[u] = k.srp[k.order ? k.order[i[u]] : i[u]];
        }
#pragma unroll
        for (int u = 0; u < kKeyU; u++) c0[u] = k.sci[sp[u] + (min(e0 + u * kWave, nnz - 1) - rpi[u])];
#pragma unroll
        for (int u = 0; u < kKeyU; u++) {
            const uint32_t c = (uint32_t)(k.perm ? k.perm[c0[u]] : c0[u]);
            const int64_t e = e0 + u * kWave;
            if (e < nnz) {
                keys[e] = ((K)(sg[u] & k.segmask) << k.colbits) | (K)c;
                vals[e] = (uint16_t)(i[u] - k.seg_row[sg[u]]);
            }
        }
    }
}

// The key pass from the source side (PrPart::job): the source entries [e0, e1) of one uploaded
// chunk, one wave per 64-entry slab of the SOURCE CSR, lane = entry.  Source row u is local row
// perm[u] (the single plan's hub-first relabelling: order and perm are inverse), so entry e of
// row u lands at local position rp[perm[u]] + (e - srp[u]), the position the gather pass
// (k_sorted_keys) gives it: the sort that follows sees the same keys in the same places.  Each
// chunk runs as soon as its copy has landed, under the copies of the later chunks.
template <typename K>
__global__ __launch_bounds__(256) void k_scatter_keys(KeySrc k, int64_t n_src, const int64_t *__restrict__ ssrow,
                                                      int64_t sl0, int64_t sl1, int64_t nnz,
                                                      const int32_t *__restrict__ rowseg, K *__restrict__ keys,
                                                      uint16_t *__restrict__ vals) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t nw = (int64_t)gridDim.x * (256 / kWave);
    const int64_t nslabs_src = (nnz + kWave - 1) / kWave;
    for (int64_t sl = sl0 + ((int64_t)blockIdx.x * 256 + threadIdx.x) / kWave; sl < sl1; sl += nw) {
        const int64_t e = sl * kWave + lane;
        const int64_t ee = min(e, nnz - 1);
        const int64_t u = slab_row_of(k.srp, ssrow, n_src, min(sl, nslabs_src - 1), ee, lane);
        const int32_t i = k.perm[u];
        const int32_t sg = rowseg[i];
        const int64_t dst = k.rp[i] + (ee - k.srp[u]);
        const uint32_t c = (uint32_t)k.perm[k.sci[ee]];
        if (e < nnz) {
            keys[dst] = ((K)(sg & k.segmask) << k.colbits) | (K)c;
            vals[dst] = (uint16_t)(i - k.seg_row[sg]);
        }
    }
}

// sci / spk / gbase from the sorted (key, row) pairs: every entry's column into sci (the LONG
// path and the escape supergroups read it), and for the sorted blocks (segments with gseg >= 0)
// the packed entries and the base column of each 256-entry supergroup, aligned to the block's
// first entry (the kernel's rounds).
struct SegDesc {
    int64_t z0, z1;
    int32_t gseg;   // the block's first supergroup in gbase, -1 for a LONG row
    int32_t pad;
};

// A workgroup per kPackChunk entries of one segment (host-built list: no search per entry); the
// chunks start on the segment's 256-entry supergroups, so each of a thread's 16 entries lies in
// one supergroup whose base / last keys every thread of the workgroup reads alike.
constexpr int64_t kPackChunk = 4096;
struct PackChunk {
    int64_t z0;
    int32_t seg;
    int32_t pad;
};

template <typename K>
__global__ __launch_bounds__(256) void k_sorted_pack(const SegDesc *__restrict__ segs, const PackChunk *__restrict__ chunks,
                                                     int64_t nchunks, const K *__restrict__ keys,
                                                     const uint16_t *__restrict__ vals, uint32_t colmask,
                                                     int32_t *__restrict__ sci, uint32_t *__restrict__ spk,
                                                     uint32_t *__restrict__ gbase) {
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const PackChunk pc = chunks[c];
        const SegDesc sg = segs[pc.seg];
        const int64_t z1 = min(pc.z0 + kPackChunk, sg.z1);
#pragma unroll 4
        for (int64_t g0 = pc.z0; g0 < z1; g0 += 256) {
            const int64_t e = g0 + threadIdx.x;
            const bool in = e < z1;
            const uint32_t col = in ? (uint32_t)keys[e] & colmask : 0u;
            if (in) sci[e] = (int32_t)col;
            if (sg.gseg < 0 || !in) continue;
            const int64_t q = (g0 - sg.z0) >> 8;
            const uint32_t base = (uint32_t)keys[g0] & colmask;
            const uint32_t lastc = (uint32_t)keys[min(g0 + 255, sg.z1 - 1)] & colmask;
            const bool esc = lastc - base >= (1u << (32 - kRowBits));
            const uint32_t row = vals[e];
            spk[e] = esc ? row : ((col - base) << kRowBits) | row;
            if (threadIdx.x == 0) gbase[sg.gseg + q] = esc ? (base | 0x80000000u) : base;
        }
    }
}

// LDS bank spreading: inside every full 64-entry group of a sorted block, the 64 entries are
// permuted so that each of the four LDS-add wave-instructions of the X4 layout (instruction j
// adds the entries at positions 4s + j, s < 16, of the group: one per lane of the group's 16
// lanes) gets entries whose rows differ mod 16 wherever possible -- the banks of a 64-bit LDS
// address a are (a/4) mod 32, so rows r and r' collide on a 16-lane group iff r = r' mod 16.
// The entries are ranked by (row mod 16, bit 4 of the row, position) and entry k of that order
// goes to instruction k mod 4, slot k / 4: a residue held by m <= 4 entries lands in m
// different instructions.  The group keeps its column set, so its gathers touch the same lines.
// One wave per group.
// Only the wide part of the block (from its narrow prefix nsplit[block] supergroups on).
__global__ __launch_bounds__(256) void k_sorted_laneperm(const RowBlock *__restrict__ blocks, const uint32_t *__restrict__ nsplit,
                                                         uint32_t *spk, int32_t *sci) {
    const RowBlock b = blocks[blockIdx.y];
    const int64_t z0 = b.nz_begin + 256 * (int64_t)nsplit[blockIdx.y], ngroups = (b.nz_end - z0) >> 6;   // full groups only
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
    const int64_t waves = (int64_t)gridDim.x * blockDim.x / kWave;
    for (int64_t g = wave; g < ngroups; g += waves) {
        const int64_t e = z0 + (g << 6) + lane;
        const uint32_t p = spk[e];
        const int32_t c = sci[e];
        const uint32_t row = p & ((1u << kRowBits) - 1);
        const uint32_t key = ((row & 15u) << 1) | ((row >> 4) & 1u);
        // rank = entries with a smaller key + entries with my key at a lower lane
        uint32_t rank = 0;
        for (uint32_t k = 0; k < 32; k++) {
            const uint64_t m = __ballot(key == k);
            if (k < key) rank += (uint32_t)__popcll(m);
            else if (k == key) rank += (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        }
        const int64_t dst = z0 + (g << 6) + 4 * (rank >> 2) + (rank & 3);
        spk[dst] = p;
        sci[dst] = c;
    }
}

// Bank-aware order inside column runs (GX_PR_BANK_ORDER; gx_pr_bank.h), for the run region
// (supergroups below rsplit[block]: runs of one column pair, in plain positions: a run's codes
// are consecutive from a group's start), the pair prefix
// (supergroups below qsplit[block]: runs of one column pair) and the narrow prefix (up to
// nsplit[block]: runs of one column) of every sorted block, before their codes are emitted.  In
// all three layouts a 16-lane group of an LDS add covers 16 consecutive codes (slots), and a run has no
// filler inside it, so consecutive entries of a run meet in a group.  Each piece of a run inside
// a tile of kBankTile entries is dealt round-robin over its rows' classes (row mod 16), in place.
// A piece keeps its entries (row and column move together), so the block's multiset of
// (row, column), the runs' boundaries, hence every step, filler and junk half, are unchanged.
// One 256-thread workgroup per tile, thread t holding entries 8 t .. 8 t + 7.  A long run is
// dealt 2 Ki entries at a time, which leaves its classes' counts nearly even; dealt 64 at a time
// (one wave per tile, ballots only) a class of random rows holds 4 +- 2 entries and the fullest
// class sets the cycles of the piece's last groups: the model's conflict cycles x 0.79 against
// x 0.63, 584 against 577 us per launch.  A piece's ends come from two scans over
// the workgroup (the last head at or before an entry, the first after it); an entry's rank in
// its class from an LDS counter of its piece and class (pieces of two or more entries start at
// least 2 apart, so start / 2 names them; two 16-bit counters per word), in arrival order:
// which of two rows of one class and run comes first is not fixed run to run, and does not
// matter to the banks.  A tile may straddle the end of the pair prefix; a piece does not.  The
// words of spk keep the column offset of the supergroup they came from, which neither prefix reads.
constexpr int kBankTile = 2048, kBankBS = 256, kBankPer = kBankTile / kBankBS;
__global__ __launch_bounds__(kBankBS) void k_bank_order(const RowBlock *__restrict__ blocks, const uint32_t *__restrict__ rsplit,
                                                        const uint32_t *__restrict__ qsplit,
                                                        const uint32_t *__restrict__ nsplit, uint32_t *spk, int32_t *sci) {
    __shared__ uint32_t cnt2[kBankTile / 2][kBankClasses / 2];   // 32 KiB
    __shared__ int32_t wred[2][kBankBS / kWave];
    const RowBlock b = blocks[blockIdx.y];
    const int64_t z0 = b.nz_begin, N = b.nz_end - z0;
    const int64_t Nq = min(N, (int64_t)qsplit[blockIdx.y] << 8), Np = min(N, (int64_t)nsplit[blockIdx.y] << 8);
    const int64_t Nr = min(N, (int64_t)rsplit[blockIdx.y] << 8);   // run region: keyed by pair, plain positions
    const int64_t ntiles = (Np + kBankTile - 1) / kBankTile;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    for (int64_t g = blockIdx.x; g < ntiles; g += gridDim.x) {
        const int64_t t0 = g * kBankTile;
        const int32_t nin = (int32_t)min<int64_t>(kBankTile, Np - t0);   // entries of the tile
        uint32_t p[kBankPer], key[kBankPer];
        int32_t c[kBankPer], s0[kBankPer], s1[kBankPer];
        bool head[kBankPer];
        for (int w = tid; w < kBankTile / 2 * (kBankClasses / 2); w += kBankBS) (&cnt2[0][0])[w] = 0u;
        // the entry before the thread's first, for its head flag
        const int32_t i0 = tid * kBankPer;
        uint32_t prevkey = 0;
        if (i0 > 0 && i0 < nin) {
            const int64_t e = t0 + i0 - 1;
            prevkey = e < Nq ? (uint32_t)sci[z0 + e] >> 1 : (uint32_t)sci[z0 + e];
        }
#pragma unroll
        for (int j = 0; j < kBankPer; j++) {
            const int32_t i = i0 + j;
            const bool in = i < nin;
            p[j] = in ? spk[z0 + t0 + i] : 0u;
            c[j] = in ? sci[z0 + t0 + i] : 0;
            key[j] = t0 + i < Nq ? (uint32_t)c[j] >> 1 : (uint32_t)c[j];
        }
        int32_t last = -1;
#pragma unroll
        for (int j = 0; j < kBankPer; j++) {
            const int32_t i = i0 + j;
            // the tile's first entry, the pair or narrow prefix's first, an entry past the prefix, a new key
            head[j] = i == 0 || i >= nin || t0 + i == Nq || t0 + i == Nr || key[j] != (j ? key[j - 1] : prevkey);
            if (head[j]) last = i;
            s0[j] = last;
        }
        int32_t first = kBankTile;
#pragma unroll
        for (int j = kBankPer - 1; j >= 0; j--) {
            s1[j] = first;
            if (head[j]) first = i0 + j;
        }
        // the last head of the threads before mine, the first head of the threads after mine
        int32_t m0 = last, m1 = first;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int32_t v0 = __shfl_up(m0, d, kWave), v1 = __shfl_down(m1, d, kWave);
            if (lane >= d) m0 = max(m0, v0);
            if (lane + d < kWave) m1 = min(m1, v1);
        }
        if (lane == kWave - 1) wred[0][wave] = m0;
        if (lane == 0) wred[1][wave] = m1;
        int32_t before = __shfl_up(m0, 1, kWave), after = __shfl_down(m1, 1, kWave);
        if (lane == 0) before = -1;
        if (lane == kWave - 1) after = kBankTile;
        __syncthreads();   // wred written, cnt2 zeroed
        for (int w = 0; w < kBankBS / kWave; w++) {
            if (w < wave) before = max(before, wred[0][w]);
            if (w > wave) after = min(after, wred[1][w]);
        }
        uint32_t rank[kBankPer];
#pragma unroll
        for (int j = 0; j < kBankPer; j++) {
            if (s0[j] < 0) s0[j] = before;   // entry 0 of the tile is a head, so before >= 0 here
            s1[j] = min(s1[j], after);
            rank[j] = 0;
            if (s1[j] - s0[j] > 1) {
                const uint32_t cls = p[j] & (uint32_t)(kBankClasses - 1);
                const uint32_t old = atomicAdd(&cnt2[s0[j] >> 1][cls >> 1], 1u << (16 * (cls & 1)));
                rank[j] = (old >> (16 * (cls & 1))) & 0xffffu;
            }
        }
        __syncthreads();   // every entry counted, and every load of the tile done
#pragma unroll
        for (int j = 0; j < kBankPer; j++) {
            const uint32_t n = (uint32_t)(s1[j] - s0[j]);
            if (n <= 1) continue;
            uint32_t cnt[kBankClasses];
#pragma unroll
            for (int k = 0; k < kBankClasses / 2; k++) {
                const uint32_t w = cnt2[s0[j] >> 1][k];
                cnt[2 * k] = w & 0xffffu;
                cnt[2 * k + 1] = w >> 16;
            }
            const uint32_t k = bank_deal_pos(cnt, p[j] & (uint32_t)(kBankClasses - 1), rank[j]);
            const bool pairs = t0 + s0[j] < Nq, runs = t0 + s0[j] < Nr;
            const int64_t dst = z0 + t0 + s0[j] + (pairs && !runs ? bank_pair_pos(k, n) : k);
            spk[dst] = p[j];
            if (pairs) sci[dst] = c[j];   // a narrow run is one column
        }
        __syncthreads();   // cnt2 and wred are rewritten by the next tile
    }
}

// ---- narrow codes (gather_narrow).  A sorted block's entries are column-sorted; its prefix of
// supergroups where 2-byte codes (fillers included) take fewer bytes than the 4-byte entries is
// recoded, chosen per block to minimise the index bytes: supergroup g costs 2 (n_g + D_g) bytes
// narrow against 4 n_g wide, D_g = the fillers its column steps need (a step s > 3 takes
// ceil(s / 3) - 1).  SYN-8_5: 95 % of the entries, 2.5 % fillers, index bytes 2.51 -> 1.35 GB.

// fillers of the step from the previous entry of the block to entry e (0 for its first)
__device__ __forceinline__ uint32_t narrow_fillers(const int32_t *sci, int64_t z0, int64_t e, uint32_t *step) {
    const uint32_t c = (uint32_t)sci[e];
    const uint32_t s0 = e > z0 ? c - (uint32_t)sci[e - 1] : 0u;
    *step = s0;
    return s0 > 3 ? (s0 + 2) / 3 - 1 : 0u;
}

__device__ __forceinline__ uint32_t wave_total(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_incl(v), kWave - 1);
}

// D_g of every 256-entry supergroup of every sorted block (grid.y = block) from the end of its
// pair prefix qsplit[block] on (the narrow codes start afresh there), one wave each.
__global__ __launch_bounds__(256) void k_narrow_cost(const RowBlock *__restrict__ blocks, const int32_t *__restrict__ sci,
                                                     const uint32_t *__restrict__ qsplit, uint32_t *__restrict__ fill) {
    const RowBlock b = blocks[blockIdx.y];
    const int64_t z0 = b.nz_begin, N = b.nz_end - z0, ng = (N + 255) >> 8;
    const int64_t Q = qsplit[blockIdx.y], zq = z0 + (Q << 8);
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t waves = (int64_t)gridDim.x * blockDim.x / kWave;
    for (int64_t g = Q + ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave; g < ng; g += waves) {
        uint32_t d = 0, st;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t e = (g << 8) + 4 * lane + j;
            if (e < N) d += narrow_fillers(sci, zq, z0 + e, &st);
        }
        d = wave_total(d);
        if (lane == 0) fill[b.seg + g] = d;
    }
}

// Per block (one 1024-thread workgroup): the narrow prefix P (supergroups) maximising
// sum_{Q<=g<P} (n_g - D_g) (Q when `enable` is off; Q = qsplit[block], the end of the pair
// prefix, or 0 when qsplit is null), the code offset of every supergroup inside the block's
// narrow run (exclusive prefix of n_g + D_g), and the block's code count.
// The pair prefix is chosen by the same kernel (k_pair_cost's counts): `codes` then holds the
// slots of each supergroup (null: n_g + D_g) and a filler weighs w4 / 4 entries (narrow: 4).
__global__ __launch_bounds__(1024) void k_narrow_split(const RowBlock *__restrict__ blocks, const uint32_t *__restrict__ fill,
                                                       const uint32_t *__restrict__ codes, int w4,
                                                       const uint32_t *__restrict__ qsplit,
                                                       int enable, int64_t min_entries, uint32_t *__restrict__ nsplit,
                                                       uint32_t *__restrict__ ncode,
                                                       uint32_t *__restrict__ noff) {
    __shared__ int64_t sben[1024], scod[1024];
    __shared__ int64_t bestv[1024];
    __shared__ int32_t besti[1024];
    const RowBlock b = blocks[blockIdx.x];
    const int64_t N = b.nz_end - b.nz_begin, ng = (N + 255) >> 8;
    const int t = threadIdx.x;
    const int64_t per = (ng + 1023) / 1024, g0 = min(ng, t * per), g1 = min(ng, g0 + per);
    const int64_t Q = qsplit ? (int64_t)qsplit[blockIdx.x] : 0;
    auto cnt = [&](int64_t g) { return min<int64_t>(256, N - (g << 8)); };
    auto benefit = [&](int64_t g) { return g < Q ? 0 : 4 * cnt(g) - (int64_t)w4 * (int64_t)fill[b.seg + g]; };
    auto ncodes = [&](int64_t g) {
        return g < Q ? 0 : codes ? (int64_t)codes[b.seg + g] : cnt(g) + (int64_t)fill[b.seg + g];
    };
    int64_t ben = 0, cod = 0;
    for (int64_t g = g0; g < g1; g++) {
        ben += benefit(g);
        cod += ncodes(g);
    }
    sben[t] = ben;
    scod[t] = cod;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {   // inclusive scans (Hillis-Steele)
        const int64_t a1 = t >= o ? sben[t - o] : 0, a2 = t >= o ? scod[t - o] : 0;
        __syncthreads();
        sben[t] += a1;
        scod[t] += a2;
        __syncthreads();
    }
    int64_t pb = sben[t] - ben, pc = scod[t] - cod;
    int64_t bv = 0;
    int32_t bi = (int32_t)Q;   // P = Q (no code) is always allowed
    for (int64_t g = g0; g < g1; g++) {
        noff[b.seg + g] = (uint32_t)pc;
        pb += benefit(g);
        pc += ncodes(g);
        if (pb > bv) {
            bv = pb;
            bi = (int32_t)(g + 1);
        }
    }
    bestv[t] = bv;
    besti[t] = bi;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {   // max value, then the smallest prefix
        if (t < o) {
            const int64_t v2 = bestv[t + o];
            const int32_t i2 = besti[t + o];
            if (v2 > bestv[t] || (v2 == bestv[t] && i2 < besti[t])) {
                bestv[t] = v2;
                besti[t] = i2;
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        const int32_t P = (enable && N >= min_entries) ? besti[0] : (int32_t)Q;
        nsplit[blockIdx.x] = (uint32_t)P;
        // codes of the prefix: the offset of supergroup P, or all of them
        ncode[blockIdx.x] = P == Q ? 0u : (uint32_t)(P < ng ? noff[b.seg + P] : (uint32_t)scod[1023]);
    }
}

// Padding codes everywhere (step 0, a junk row by lane) and the null supergroup's base.
__global__ void k_narrow_fill(uint16_t *__restrict__ npk, uint64_t ncodes, uint32_t *__restrict__ nbase, uint32_t null_sg,
                              uint32_t zero_col) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < ncodes; p += (uint64_t)gridDim.x * blockDim.x)
        npk[p] = (uint16_t)(kJunkRow + ((p >> 3) & (kWave - 1)));
    if (blockIdx.x == 0 && threadIdx.x == 0) nbase[null_sg] = zero_col;
}

// The codes of the narrow prefix: one wave per 256-entry supergroup g < P of each block; lane
// l emits entries 4l .. 4l+3, each preceded by its fillers, at the block's run + noff[g] + the
// lane's exclusive scan of code counts.  Whoever emits the last code of a 512-code supergroup
// stores the next one's base (the column reached); the block's first base is its first column.
__global__ __launch_bounds__(256) void k_narrow_emit(const RowBlock *__restrict__ blocks, const int32_t *__restrict__ sci,
                                                     const uint32_t *__restrict__ spk, const uint32_t *__restrict__ qsplit,
                                                     const uint32_t *__restrict__ nsplit,
                                                     const uint32_t *__restrict__ ncode, const uint32_t *__restrict__ noff,
                                                     const int64_t *__restrict__ nbeg, uint16_t *__restrict__ npk,
                                                     uint32_t *__restrict__ nbase) {
    const RowBlock b = blocks[blockIdx.y];
    const int64_t z0 = b.nz_begin, N = b.nz_end - z0, P = nsplit[blockIdx.y];
    const int64_t Q = qsplit[blockIdx.y], zq = z0 + (Q << 8);   // the narrow codes follow the pair prefix
    const int64_t nb = nbeg[blockIdx.y], C = ncode[blockIdx.y];
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t waves = (int64_t)gridDim.x * blockDim.x / kWave;
    if (P > Q && blockIdx.x == 0 && threadIdx.x == 0) nbase[nb / kNSg] = (uint32_t)sci[zq];
    for (int64_t g = Q + ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave; g < P; g += waves) {
        uint32_t fl[4], st[4], n = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t e = (g << 8) + 4 * lane + j;
            fl[j] = e < N ? narrow_fillers(sci, zq, z0 + e, &st[j]) : 0u;
            n += e < N ? fl[j] + 1 : 0u;
        }
        int64_t pos = nb + noff[b.seg + g] + (wave_scan_incl(n) - n);   // absolute code index
        // stored lane-major inside the 512-code supergroup: code e of it at (e mod 64) * 8 + e / 64
        auto put = [&](uint32_t step, uint32_t row, uint32_t col_after) {
            npk[(pos & ~(int64_t)(kNSg - 1)) + (pos & (kWave - 1)) * 8 + ((pos >> 6) & 7)] = (uint16_t)((step << kRowBits) | row);
            const int64_t rel = pos - nb + 1;   // codes of the block up to and including this one
            if ((rel & (kNSg - 1)) == 0 && rel < C) nbase[(pos + 1) / kNSg] = col_after;
            pos++;
        };
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t e = (g << 8) + 4 * lane + j;
            if (e >= N) continue;
            const uint32_t c = (uint32_t)sci[z0 + e];
            uint32_t at = c - st[j];
            for (uint32_t f = 0; f < fl[j]; f++) {
                at += 3;
                put(3u, (uint32_t)(kJunkRow + (pos & (kWave - 1))), at);   // the lane's own junk row
            }
            put(c - at, spk[z0 + e] & ((1u << kRowBits) - 1), c);
        }
    }
}

// ---- pair slots (gather_pairs).  The first Q 256-entry supergroups of a block's column-sorted
// entries are recoded in slots of two entries of one column pair (columns 2p, 2p + 1).  The
// entries of a pair are consecutive (a run); entry k of its run leads a slot when k is even and
// takes entry k + 1 as the slot's second half, or a junk row when the run (or the prefix) ends
// there.  A run whose pair lies more than 3 pairs past the previous run's is preceded by
// ceil(step / 3) - 1 filler slots.  So the slots of a supergroup do not depend on Q; only whether
// the slot led by the prefix's last entry has a second half does.

// The lane's four entries 4 lane .. 4 lane + 3 of supergroup g of a block (z0, N entries, the
// first Nq of them in the prefix), one wave per supergroup.
struct PairLane {
    uint32_t pair[4], col[4], next[4];   // the entry's pair and column, the next entry's column
    uint32_t step[4], sf[4];             // a run's first entry: the slot's step and the filler slots before it
    bool in[4], start[4], lead[4], half[4];
};

// The first entry of the column-pair run that holds entry f of a block (z0): f itself, or, when
// the run starts before it, found by binary search (the entries are column-sorted).  Uniform over
// the wave when f is.
__device__ __forceinline__ int64_t pair_run_start(const int32_t *__restrict__ sci, int64_t z0, int64_t f) {
    const uint32_t pf = (uint32_t)sci[z0 + f] >> 1;
    if (f == 0 || ((uint32_t)sci[z0 + f - 1] >> 1) != pf) return f;
    int64_t lo = 0, hi = f;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (((uint32_t)sci[z0 + mid] >> 1) >= pf) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ void pair_lane(const int32_t *__restrict__ sci, int64_t z0, int64_t N, int64_t Nq, int64_t g,
                                          int lane, PairLane &o) {
    const int64_t i0 = (g << 8) + 4 * lane;
    uint32_t c[6];   // the entry before, the four, the entry after
#pragma unroll
    for (int j = 0; j < 6; j++) c[j] = (uint32_t)sci[z0 + min(max(i0 + j - 1, (int64_t)0), N - 1)];
    const int64_t f = g << 8;
    const int64_t gs = pair_run_start(sci, z0, f);
    int32_t ls = -1;   // the last run start among the lane's entries (supergroup-relative)
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t i = i0 + j;
        o.in[j] = i < Nq;
        o.col[j] = c[j + 1];
        o.next[j] = c[j + 2];
        o.pair[j] = c[j + 1] >> 1;
        o.start[j] = o.in[j] && (i == 0 || (c[j] >> 1) != o.pair[j]);
        if (o.start[j]) ls = 4 * lane + j;
    }
    int32_t m = ls;   // inclusive max scan over the lanes
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int32_t v = __shfl_up(m, d, kWave);
        if (lane >= d) m = max(m, v);
    }
    int32_t before = __shfl_up(m, 1, kWave);
    if (lane == 0) before = -1;
    int64_t rs = before >= 0 ? f + before : gs;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t i = i0 + j;
        if (o.start[j]) rs = i;
        o.lead[j] = o.in[j] && (((i - rs) & 1) == 0);
        o.half[j] = o.lead[j] && (i + 1 >= Nq || (o.next[j] >> 1) != o.pair[j]);
        const uint32_t s0 = (o.start[j] && i > 0) ? o.pair[j] - (c[j] >> 1) : 0u;
        o.sf[j] = s0 > 3 ? (s0 + 2) / 3 - 1 : 0u;
        o.step[j] = s0 - 3 * o.sf[j];
    }
}

// Slots and filler halves of every 256-entry supergroup of every sorted block from the end of its
// run region rsplit[block] on (the slots start afresh there).
__global__ __launch_bounds__(256) void k_pair_cost(const RowBlock *__restrict__ blocks, const int32_t *__restrict__ sci,
                                                   const uint32_t *__restrict__ rsplit, uint32_t *__restrict__ slots,
                                                   uint32_t *__restrict__ fill) {
    const RowBlock b = blocks[blockIdx.y];
    const int64_t R = rsplit[blockIdx.y];
    const int64_t z0 = b.nz_begin + (R << 8), N = b.nz_end - z0, ng = (N + 255) >> 8;   // past the run region
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t waves = (int64_t)gridDim.x * blockDim.x / kWave;
    for (int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave; g < ng; g += waves) {
        PairLane pl;
        pair_lane(sci, z0, N, N, g, lane, pl);
        uint32_t ns = 0, nf = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            ns += (pl.lead[j] ? 1u : 0u) + (pl.start[j] ? pl.sf[j] : 0u);
            nf += (pl.half[j] ? 1u : 0u) + (pl.start[j] ? 2 * pl.sf[j] : 0u);
        }
        ns = wave_total(ns);
        nf = wave_total(nf);
        if (lane == 0) {
            slots[b.seg + R + g] = ns;
            fill[b.seg + R + g] = nf;
        }
    }
}

// Padding slots everywhere (step 0, both halves the lane's junk row, sel 0: in the null
// supergroup x's zero slot) and the null supergroup's base, the pair holding x's zero slot.
__global__ void k_pair_fill(uint32_t *__restrict__ ppk, uint64_t nslots, uint32_t *__restrict__ pbase, uint32_t null_sg,
                            uint32_t zero_pair) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nslots; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t junk = (uint32_t)(kJunkRow + ((p >> 2) & (kWave - 1)));
        ppk[p] = (junk << 15) | junk;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) pbase[null_sg] = zero_pair;
}

// The slots of the pair prefix: one wave per 256-entry supergroup R <= g < Q of each block; lane l
// emits the slots led by entries 4l .. 4l+3, each run's first preceded by its filler slots, at
// the block's run + poff[g] + the lane's exclusive scan of slot counts.  Whoever emits the last
// slot of a 256-slot supergroup stores the next one's base (the pair reached); the block's first
// base is its first pair.  nfill: the filler halves written (statistics).
__global__ __launch_bounds__(256) void k_pair_emit(const RowBlock *__restrict__ blocks, const int32_t *__restrict__ sci,
                                                   const uint32_t *__restrict__ spk, const uint32_t *__restrict__ rsplit,
                                                   const uint32_t *__restrict__ qsplit,
                                                   const uint32_t *__restrict__ pcount, const uint32_t *__restrict__ poff,
                                                   const int64_t *__restrict__ pbeg, uint32_t *__restrict__ ppk,
                                                   uint32_t *__restrict__ pbase, unsigned long long *__restrict__ nfill) {
    const RowBlock b = blocks[blockIdx.y];
    // supergroups and entries counted from the end of the run region
    const int64_t R = rsplit[blockIdx.y];
    const int64_t z0 = b.nz_begin + (R << 8), N = b.nz_end - z0, Q = (int64_t)qsplit[blockIdx.y] - R;
    const int64_t Nq = min(N, Q << 8);
    const int64_t pb = pbeg[blockIdx.y], C = pcount[blockIdx.y];
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t waves = (int64_t)gridDim.x * blockDim.x / kWave;
    constexpr uint32_t kRowMask = (1u << kRowBits) - 1;
    if (Q > 0 && blockIdx.x == 0 && threadIdx.x == 0) pbase[pb / kPSg] = (uint32_t)sci[z0] >> 1;
    for (int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave; g < Q; g += waves) {
        PairLane pl;
        pair_lane(sci, z0, N, Nq, g, lane, pl);
        uint32_t n = 0, nf = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            n += (pl.lead[j] ? 1u : 0u) + (pl.start[j] ? pl.sf[j] : 0u);
            nf += (pl.half[j] ? 1u : 0u) + (pl.start[j] ? 2 * pl.sf[j] : 0u);
        }
        int64_t pos = pb + poff[b.seg + R + g] + (wave_scan_incl(n) - n);   // absolute slot index
        nf = wave_total(nf);
        if (lane == 0 && nf) atomicAdd(nfill, (unsigned long long)nf);
        // stored lane-major inside the 256-slot supergroup: slot e of it at (e mod 64) * 4 + e / 64
        auto put = [&](uint32_t step, uint32_t ha, uint32_t hb, uint32_t pair_after) {
            ppk[(pos & ~(int64_t)(kPSg - 1)) + (pos & (kWave - 1)) * 4 + ((pos >> 6) & 3)] = (step << 30) | (ha << 15) | hb;
            const int64_t rel = pos - pb + 1;   // slots of the block up to and including this one
            if ((rel & (kPSg - 1)) == 0 && rel < C) pbase[(pos + 1) / kPSg] = pair_after;
            pos++;
        };
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (!pl.lead[j]) continue;
            const int64_t e = (g << 8) + 4 * lane + j;
            uint32_t step = 0;
            if (pl.start[j]) {
                uint32_t at = pl.pair[j] - pl.step[j] - 3 * pl.sf[j];
                for (uint32_t f = 0; f < pl.sf[j]; f++) {
                    at += 3;
                    const uint32_t junk = (uint32_t)(kJunkRow + (pos & (kWave - 1)));   // the lane's own junk row
                    put(3u, junk, junk, at);
                }
                step = pl.step[j];
            }
            const uint32_t ha = ((pl.col[j] & 1u) << kRowBits) | (spk[z0 + e] & kRowMask);
            const uint32_t hb = pl.half[j] ? (uint32_t)(kJunkRow + (pos & (kWave - 1)))
                                           : ((pl.next[j] & 1u) << kRowBits) | (spk[z0 + e + 1] & kRowMask);
            put(step, ha, hb, pl.pair[j]);
        }
    }
}

// ---- run groups (gather_runs, gx_pr_runs.h).  The first R 256-entry supergroups of a block's
// column-sorted entries are recoded as 2-byte run codes.  The entries of a column pair are
// consecutive (a run); a run's codes start on a group of 64 and the run is followed by
// run_pad(its length) padding codes, so the entry at sorted position e takes code position
// e + (the padding of the runs that end before e).  The padding of a run is counted in the
// supergroup that holds its last entry, so a supergroup's count does not depend on R; the run
// that R cuts is padded like the others (run_region_codes).

// The lane's four entries 4 lane .. 4 lane + 3 of supergroup g of a block (z0, N entries, the
// first Nr of them in the region), one wave per supergroup: where a run ends (or the region cuts
// it), the run's length.
struct RunLane {
    uint32_t pair[4], col[4], len[4];   // len: the run's entries at its last entry, 0 elsewhere
    bool in[4];
};

__device__ __forceinline__ void run_lane(const int32_t *__restrict__ sci, int64_t z0, int64_t N, int64_t Nr, int64_t g,
                                         int lane, RunLane &o) {
    const int64_t i0 = (g << 8) + 4 * lane;
    uint32_t c[6];   // the entry before, the four, the entry after
#pragma unroll
    for (int j = 0; j < 6; j++) c[j] = (uint32_t)sci[z0 + min(max(i0 + j - 1, (int64_t)0), N - 1)];
    const int64_t f = g << 8;
    const int64_t gs = pair_run_start(sci, z0, f);
    bool start[4];
    int32_t ls = -1;   // the last run start among the lane's entries (supergroup-relative)
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t i = i0 + j;
        o.in[j] = i < Nr;
        o.col[j] = c[j + 1];
        o.pair[j] = c[j + 1] >> 1;
        start[j] = o.in[j] && (i == 0 || (c[j] >> 1) != o.pair[j]);
        if (start[j]) ls = 4 * lane + j;
    }
    int32_t m = ls;   // inclusive max scan over the lanes
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int32_t v = __shfl_up(m, d, kWave);
        if (lane >= d) m = max(m, v);
    }
    int32_t before = __shfl_up(m, 1, kWave);
    if (lane == 0) before = -1;
    int64_t rs = before >= 0 ? f + before : gs;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t i = i0 + j;
        if (start[j]) rs = i;
        const bool end = o.in[j] && (i + 1 >= Nr || (c[j + 2] >> 1) != o.pair[j]);
        o.len[j] = end ? (uint32_t)(i - rs + 1) : 0u;
    }
}

// Padding codes of every 256-entry supergroup of every sorted block.
__global__ __launch_bounds__(256) void k_run_cost(const RowBlock *__restrict__ blocks, const int32_t *__restrict__ sci,
                                                  uint32_t *__restrict__ fill) {
    const RowBlock b = blocks[blockIdx.y];
    const int64_t z0 = b.nz_begin, N = b.nz_end - z0, ng = (N + 255) >> 8;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t waves = (int64_t)gridDim.x * blockDim.x / kWave;
    for (int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave; g < ng; g += waves) {
        RunLane rl;
        run_lane(sci, z0, N, N, g, lane, rl);
        RunCursor cur{0};   // the padding of the runs that end among the lane's entries
#pragma unroll
        for (int j = 0; j < 4; j++) cur.end_run(rl.len[j]);
        const uint32_t nf = wave_total((uint32_t)cur.pad);
        if (lane == 0) fill[b.seg + g] = nf;
    }
}

// Padding codes everywhere (sel 0, a junk row by lane) and every group's pair the one holding x's
// zero slot: the groups after a block's last run and the null supergroup gather 0.0.
__global__ void k_run_fill(uint16_t *__restrict__ rpk, uint64_t ncodes, uint32_t *__restrict__ rpair, uint32_t zero_pair) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < ncodes; p += (uint64_t)gridDim.x * blockDim.x) {
        rpk[p] = (uint16_t)(kJunkRow + ((p / kRunSgGroups) & (kWave - 1)));
        if ((p & (kRunGroup - 1)) == 0) rpair[p / kRunGroup] = zero_pair;
    }
}

// The codes of the run region: one wave per 256-entry supergroup g < R of each block; lane l
// emits entries 4l .. 4l+3 at the block's run + roff[g] (the codes before the supergroup's first
// entry) + the entry's offset + the padding of the runs that end in the supergroup before it.  The
// entry whose code opens a group stores the group's pair, so no header past the block's last
// group is written.
__global__ __launch_bounds__(256) void k_run_emit(const RowBlock *__restrict__ blocks, const int32_t *__restrict__ sci,
                                                  const uint32_t *__restrict__ spk, const uint32_t *__restrict__ rsplit,
                                                  const uint32_t *__restrict__ roff, const int64_t *__restrict__ rbeg,
                                                  uint16_t *__restrict__ rpk, uint32_t *__restrict__ rpair) {
    const RowBlock b = blocks[blockIdx.y];
    const int64_t z0 = b.nz_begin, N = b.nz_end - z0, R = rsplit[blockIdx.y];
    const int64_t Nr = min(N, R << 8);
    const int64_t rb = rbeg[blockIdx.y];
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t waves = (int64_t)gridDim.x * blockDim.x / kWave;
    for (int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave; g < R; g += waves) {
        RunLane rl;
        run_lane(sci, z0, N, Nr, g, lane, rl);
        RunCursor lanepad{0};
#pragma unroll
        for (int j = 0; j < 4; j++) lanepad.end_run(rl.len[j]);
        const uint32_t n = (uint32_t)lanepad.pad;
        // the padding before the lane's first entry: the block's codes before the supergroup's first
        // entry, less those entries themselves, and the runs that end in the lanes before
        RunCursor cur{(uint64_t)roff[b.seg + g] - (uint64_t)(g << 8) + (wave_scan_incl(n) - n)};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t e = (g << 8) + 4 * lane + j;
            if (!rl.in[j]) continue;
            const uint64_t pos = (uint64_t)rb + cur.place((uint64_t)e);   // absolute code index
            rpk[run_slot(pos)] = (uint16_t)(((rl.col[j] & 1u) << kRowBits) | (spk[z0 + e] & ((1u << kRowBits) - 1)));
            if ((pos & (kRunGroup - 1)) == 0) rpair[run_group_of(pos)] = rl.pair[j];
            cur.end_run(rl.len[j]);
        }
    }
}

// Simulated duration (us) of one k_pr_pull_units launch: the units of every sorted block
// (entries ents[i], rows rws[i]) cut at unit size t, and the LONG segments (lsegs), dealt
// largest first to one workgroup slot per CU, each slot taking the next unit when it frees
// (list scheduling; the grid is issued in that order).  Per-unit cost from the per-workgroup
// timestamps (tools/unit_times.py on SYN-7_5): ~2,900 entries/us of gathers, ~2 ns per row
// (zeroing, epilogue, slab store), ~1.5 us fixed, and the last arriver's slab reads.  It
// picks the unit size on large graphs, so that the units of the large blocks land in as few
// waves as the CUs allow.
struct UnitCost {
    // entries per us, us per row, us fixed, us per row and slab (GX_PR_SIM_RATE, GX_PR_SIM_ROW_PS,
    // GX_PR_SIM_SLAB_PS override: entries / us and ps)
    double rate = 2900.0, row = 0.002, fixed = 1.5, slab = 0.0005;
    // model 1 (GX_PR_SIM_MODEL=1): a multi-unit block's units each store their slab (slab per
    // row), and only the last arriver pays the combine, one round trip (rt us, GX_PR_SIM_RT_NS)
    // per 16 Ki slab entries
    int model = 0;
    double rt = 2.0;
};

double pr_unit_makespan(const std::vector<int64_t> &ents, const std::vector<int64_t> &effs, const std::vector<int64_t> &rws,
                        const std::vector<int64_t> &lsegs, int64_t t, int cus, bool by_cost, const UnitCost &uc) {
    const double kRate = uc.rate, kRow = uc.row, kFixed = uc.fixed, kSlab = uc.slab;
    std::vector<double> cost;
    for (size_t i = 0; i < ents.size(); i++) {
        const int64_t E = ents[i];
        // units by cost, not entries: a block of mostly wide (sparse-tail) entries runs at about
        // half the hub blocks' entry rate, so it is cut into more units (pr_unit_count)
        const int64_t k = std::max<int64_t>(1, std::min((E + kRound - 1) / kRound, ((by_cost ? effs[i] : E) + t - 1) / t));
        // (model 0: every unit pays the k slabs' reads; model 1: its own slab's store, the last the combine)
        const double c = (double)effs[i] / (double)k / kRate + kRow * (double)rws[i] + kFixed +
                         (k > 1 ? kSlab * (double)rws[i] * (uc.model == 1 ? 1.0 : (double)k) : 0.0);
        for (int64_t j = 0; j < k; j++) cost.push_back(c);
        if (uc.model == 1 && k > 1)
            cost.back() = c + uc.rt * std::ceil((double)k * (double)rws[i] / (double)(1 << kRowBits));
    }
    for (int64_t e : lsegs) cost.push_back((double)e / kRate + kFixed);
    std::sort(cost.begin(), cost.end(), std::greater<double>());
    std::priority_queue<double, std::vector<double>, std::greater<double>> slots;
    for (int i = 0; i < std::max(1, cus); i++) slots.push(0.0);
    double span = 0.0;
    for (double c : cost) {
        const double f = slots.top() + c;
        slots.pop();
        slots.push(f);
        span = std::max(span, f);
    }
    return span;
}

// Every GX_PR_* knob of the plan, read once at the top of every plan (tests flip them between
// plans in one process).  The knobs that PrPart itself keeps for the launch (sorted_rows,
// sorted_nnz, long_nnz, cache_policy, nt_col, comb_kernel, queue_on) are stored there.  The
// measurements behind the defaults are in DESIGN.md 4.
struct PlanKnobs {
    bool huge, piece, runs_on, pairs_on, bank_order, laneperm, wide_keys;
    int64_t B;                                                        // entries per sorted block
    int narrow_on, sort_group_bits, run_fill_cost, pair_fill_cost, verbose;
    int64_t run_min, pair_min, narrow_min;                            // smallest block that gets the region
    int64_t wide_cost4, fill_cost4, pair_cost4, run_cost4, row_cost;  // eff_entries, the unit order
    bool cost_codes, unit_by_cost, iso_closed, unit_sim, unit_nnz_set;
    int64_t unit_nnz;
    UnitCost uc;
};

PlanKnobs plan_knobs(PrPart *p, uint64_t nnz, int64_t cus) {
    PlanKnobs k;
    // Sorted blocks of up to block_nnz entries and sorted_rows rows; rows longer than block_nnz / 4
    // take the LONG path.  block_nnz = 1 Mi with 4 Ki rows, 4 Mi once nnz / CUs passes 384 Ki, 32 Mi
    // with 16 Ki rows once it passes 2 Mi (the huge plan, or GX_PR_HUGE=1 / force_huge: a rank of a
    // block partition cuts its rows as the whole graph's plan does), at most 4x (16x when huge) the
    // power of two nearest nnz / CUs so that a small partition keeps about 4 units per block.
    // Larger blocks cut the x line requests (tools/pr_line_model.py) but give the last arriver more
    // slabs per row.  GX_PR_BLOCK_NNZ, GX_PR_SORTED_ROWS, GX_PR_LONG_NNZ override.
    const double per_cu = std::max(1.0, (double)nnz / (double)cus);
    const bool huge = k.huge = per_cu > (double)(2 << 20) || env_int("GX_PR_HUGE", 0, 0, 1) == 1 || p->force_huge;
    // a rank of a block partition: the whole graph's 32 Mi-entry blocks dealt whole, and the unit
    // cost model fitted to its pieces (below)
    const bool piece = k.piece = huge && p->nranks > 1;
    const int rmax = kMaxBlockRows;   // rows per block (LDS accumulators: 16 Ki rows = 128 KiB, the top 64 junk)
    p->sorted_rows = env_int("GX_PR_SORTED_ROWS", huge ? rmax : 4096, 64, rmax);
    int64_t pow2 = 1 << 14;
    while (pow2 < (1 << 24) && (double)(2 * pow2) <= per_cu * 1.41421356) pow2 *= 2;
    const int64_t bdef = piece ? kPlanBlockNnz
                       : huge ? std::min<int64_t>(32 << 20, 16 * pow2)
                              : std::min<int64_t>(per_cu > 384.0 * 1024 ? 4 << 20 : 1 << 20, 4 * pow2);
    k.B = env_int("GX_PR_BLOCK_NNZ", (int)bdef, 1024, 1 << 30);
    p->long_nnz = env_int("GX_PR_LONG_NNZ", (int)std::max<int64_t>(k.B / 4, kRound), 1024, 1 << 30);
    p->sorted_nnz = (int)k.B;
    // Cache policy, when x is larger than the 32 MiB of all eight L2s: the index stream, read once
    // per launch, loaded non-temporally (bit 0: SYN-8_5 898 -> 871-877 us per launch), and so are
    // the gathers of the narrow supergroups from column nt_col on (bit 2: 780 -> 757-760 us), so
    // the XCD's L2 keeps the hub lines.  Wide gathers stay cached (non-temporal: 965 us), and
    // SYN-7_5 (8 MB of x) keeps plain loads (83 -> 91 us with bit 0).  GX_PR_CP = 0 / 1 / 5.
    const uint64_t xbytes = (uint64_t)p->chunk * (uint64_t)std::max(1, p->nranks) * sizeof(double);
    p->cache_policy = env_int("GX_PR_CP", xbytes >= (32ull << 20) ? 5 : 0, 0, 5);
    if (p->cache_policy != 0 && p->cache_policy != 1) p->cache_policy = 5;
    p->nt_col = (uint32_t)env_int("GX_PR_NT_COL", 65536, 0, 1 << 30);
    // Pair slots, run groups and the bank-aware order inside the runs of the prefixes: on by
    // default for a huge graph's single plan only, where they were measured to win
    const int single_huge = huge && !piece ? 1 : 0;
    k.pairs_on = env_int("GX_PR_PAIRS", single_huge, 0, 1) == 1;
    k.runs_on = env_int("GX_PR_RUNS", single_huge, 0, 1) == 1;
    k.bank_order = env_int("GX_PR_BANK_ORDER", single_huge, 0, 1) == 1;
    k.wide_keys = env_int("GX_PR_WIDE_KEYS", 0, 0, 1) != 0;
    k.sort_group_bits = env_int("GX_PR_SORT_GROUP_BITS", 32, 1, 32);
    // a region's prefix of a block maximises entries - w fillers: w = GX_PR_RUN_FILL_COST / 4 per
    // padding code, GX_PR_PAIR_FILL_COST / 4 per filler half, 1 per narrow filler (GX_PR_NARROW=0: none)
    k.run_fill_cost = env_int("GX_PR_RUN_FILL_COST", kRunFillCost, 0, 1 << 20);
    k.run_min = env_int("GX_PR_RUN_MIN", 65536, 0, 1 << 30);
    k.pair_fill_cost = env_int("GX_PR_PAIR_FILL_COST", 48, 0, 1 << 20);
    k.pair_min = env_int("GX_PR_PAIR_MIN", 0, 0, 1 << 30);
    k.narrow_on = env_int("GX_PR_NARROW", 1, 0, 1);
    k.narrow_min = env_int("GX_PR_NARROW_MIN", 0, 0, 1 << 30);
    k.laneperm = env_int("GX_PR_LANEPERM", 1, 0, 1) != 0;   // 0 keeps every group in column order
    // The cost of a block's entries in the unit order and the launch simulation, in quarters of a
    // narrow entry's: a wide (sparse-tail) entry GX_PR_WIDE_COST (its x lines are shared by fewer
    // entries; 6x on huge graphs with the units cut by this cost, 2.7x on pieces), a narrow filler
    // GX_PR_FILL_COST where the codes are priced (GX_PR_COST_CODES, pieces: a mid-density block needs
    // up to one filler per entry), a pair-slot entry GX_PR_PAIR_COST, a run code GX_PR_RUN_COST
    k.wide_cost4 = env_int("GX_PR_WIDE_COST", piece ? 11 : huge ? 24 : 4, 4, 64);
    k.cost_codes = env_int("GX_PR_COST_CODES", piece ? 1 : 0, 0, 1) == 1;
    k.fill_cost4 = env_int("GX_PR_FILL_COST", 4, 0, 64);
    k.pair_cost4 = env_int("GX_PR_PAIR_COST", 4, 1, 64);
    k.run_cost4 = env_int("GX_PR_RUN_COST", kRunCost, 1, 64);
    k.row_cost = env_int("GX_PR_ROW_COST", 4, 0, 1024);
    // huge graphs: units per block by weighted entries (GX_PR_UNIT_BY_COST=0: by entries)
    k.unit_by_cost = env_int("GX_PR_UNIT_BY_COST", huge ? 1 : 0, 0, 1) == 1;
    // GX_PR_COMBINE=1: the multi-unit blocks combined by k_pr_combine (stripes), not by their last unit
    p->comb_kernel = env_int("GX_PR_COMBINE", piece ? 1 : 0, 0, 1) == 1;
    k.iso_closed = env_int("GX_PR_ISO_CLOSED", 1, 0, 1) == 1;
    k.unit_nnz_set = std::getenv("GX_PR_UNIT_NNZ") != nullptr;
    k.unit_nnz = env_int("GX_PR_UNIT_NNZ", 65536, 1024, 1 << 30);
    k.unit_sim = env_int("GX_PR_UNIT_SIM", 0, 0, 1) != 0;
    // a piece: the fit to the unit stamps of SYN-8_5's 8 pieces (8.3 us + 177 ps per narrow entry;
    // model 1); the combine kernel leaves the units only their slab stores
    UnitCost &uc = k.uc;
    if (piece) uc = {5650.0, 0.0, 8.3, 0.0002, 1, p->comb_kernel ? 0.0 : 2.0};
    uc.rate = (double)env_int("GX_PR_SIM_RATE", (int)uc.rate, 100, 1 << 20);
    uc.row = 1e-6 * (double)env_int("GX_PR_SIM_ROW_PS", (int)(uc.row * 1e6), 0, 1 << 20);
    uc.slab = 1e-6 * (double)env_int("GX_PR_SIM_SLAB_PS", (int)(uc.slab * 1e6), 0, 1 << 20);
    uc.model = env_int("GX_PR_SIM_MODEL", uc.model, 0, 1);
    uc.rt = 1e-3 * (double)env_int("GX_PR_SIM_RT_NS", (int)(uc.rt * 1e3), 0, 1 << 20);
    uc.fixed = 1e-3 * (double)env_int("GX_PR_SIM_FIXED_NS", (int)(uc.fixed * 1e3), 0, 1 << 20);
    // work queue: on (1), off (0), or (default) when the launch has at least two items per CU
    p->queue_on = env_int("GX_PR_QUEUE", -1, -1, 1);
    k.verbose = env_int("GX_PR_VERBOSE", 0, 0, 3);
    return k;
}

// One code region of the sorted blocks (runs, pairs, narrow): per 256-entry supergroup its
// fillers and code offset, per block the supergroup where the region ends (split), its codes
// (code) and its first code in the region's table (beg, a multiple of the supergroup size sg).
struct Region {
    int sg;
    DBuf<uint32_t> fill, off, split, code;
    DBuf<int64_t> beg;
    std::vector<uint32_t> h_split, h_code;
    std::vector<int64_t> h_beg;
    uint64_t total = 0;   // codes of all blocks, each block's rounded up to whole supergroups
    int32_t sgs(size_t i) const { return (int32_t)(((int64_t)h_code[i] + sg - 1) / sg); }
    void resize(size_t nblocks) { h_split.assign(nblocks, 0), h_code.assign(nblocks, 0), h_beg.assign(nblocks, 0); }
};

// What the stages of one plan share: the host block lists, the regions, and the device temporaries
// with the host arrays copied into them asynchronously; all live until the plan returns.
struct PlanCtx {
    PrPart *p;
    HostView<int64_t> h_rp;
    HostView<int32_t> h_outdeg;
    const int64_t rows, cus;
    const uint64_t nnz;
    const hipStream_t s;
    const PlanKnobs k;
    PlanClock clk;
    std::vector<RowBlock> longb, sortb, all;   // LONG segments, sorted blocks, both (PrPart::blocks)
    std::vector<int32_t> lfirst, lnseg, seg_row;
    std::vector<std::pair<int64_t, int32_t>> longrows;   // (length, row)
    std::vector<SegDesc> segd;
    std::vector<PackChunk> pch;
    int32_t nsegs = 0;
    int64_t ngroups = 0, T = 0;                // 256-entry supergroups of the sorted blocks; entries per unit
    const RowBlock *d_sort = nullptr;          // the sorted blocks on the device
    Region run{kRunSg}, pair{kPSg}, nar{kNSg};
    DBuf<uint32_t> pslots;                     // pairs: slots per supergroup (k_pair_cost)
    DBuf<unsigned long long> npfill;
    DBuf<int32_t> d_seg_row, d_rowseg;
    DBuf<SegDesc> d_segd;
    DBuf<int64_t> srow;
    DBuf<PackChunk> d_pch;
    bool long_dangling = false;
    std::vector<CombStripe> stripes;
    std::vector<char> multi;                   // per block of `all`: cut into several units

    PlanCtx(PrPart *part, HostView<int64_t> rp, HostView<int32_t> outdeg)
        : p(part), h_rp(rp), h_outdeg(outdeg), rows((int64_t)rp.size() - 1), cus(std::max(1, part->ctx->num_cus)),
          nnz((uint64_t)rp[rp.size() - 1]), s(part->ctx->stream), k(plan_knobs(part, nnz, cus)), clk("sorted", s) {}

    int64_t entries(size_t i) const { return sortb[i].nz_end - sortb[i].nz_begin; }
    // entries of sorted block i up to the end of region r
    int64_t upto(const Region &r, size_t i) const { return std::min<int64_t>(entries(i), 256 * (int64_t)r.h_split[i]); }
    int64_t eff_entries(size_t i) const;
    bool iso_block(const RowBlock &b) const;
    template <typename K>
    int key_pass(const KeySrc &ks, int64_t nslabs, K *keys, uint16_t *vals);
    template <typename CostLaunch>
    int split_region(Region &r, const Region *prev, bool on, CostLaunch launch_cost, const char *cost_name,
                     const char *split_name, const uint32_t *codes, int w4, int enable, int64_t min_entries);
    void print_plan(int32_t parts, int64_t slab) const;
    int cut_blocks(), upload_blocks(), sort_columns(), build_regions(), choose_unit_size(), cut_units(),
        assign_dangling_slots();
};

// The cost of block i's entries in the unit order and the launch simulation (PlanKnobs).
int64_t PlanCtx::eff_entries(size_t i) const {
    const int64_t E = entries(i), Er = upto(run, i), Erp = upto(pair, i), Enp = upto(nar, i);
    const int64_t Ep = Erp - Er, En = Enp - Erp;
    const int64_t fill = k.cost_codes ? std::max<int64_t>(0, (int64_t)nar.h_code[i] - En) : 0;
    const int64_t pent = k.cost_codes ? std::max<int64_t>(Ep, 2 * (int64_t)pair.h_code[i]) : Ep;
    return (int64_t)run.h_code[i] * k.run_cost4 / 4 + pent * k.pair_cost4 / 4 + En + fill * k.fill_cost4 / 4 +
           (E - Enp) * k.wide_cost4 / 4;
}

// LONG rows (longest first, a block per kSegNnz-entry segment) and the sorted blocks: runs of the
// other rows of at most B entries and sorted_rows rows.
int PlanCtx::cut_blocks() {
    const int64_t R = p->sorted_rows, LT = std::max<int64_t>(p->long_nnz, 1), B = k.B;
    for (int64_t r = 0; r < rows;) {
        const int64_t len = h_rp[r + 1] - h_rp[r];
        if (len > LT) {
            longrows.push_back({len, (int32_t)r});
            r++;
            continue;
        }
        const int64_t start = r;
        if (p->rows_desc) {
            // lengths non-increasing (the LONG rows are a prefix): the same cut as below by binary
            // search, the row limit or the last row pointer within B of the start (3.5 ms less on SYN-8_5)
            const int64_t lim = std::min<int64_t>(rows, start + R), limit = h_rp[start] + B;
            int64_t lo = start + 1, hi = lim + 1;   // first e in (start, lim] with h_rp[e] > limit
            while (lo < hi) {
                const int64_t mid = (lo + hi) / 2;
                if (h_rp[mid] > limit) hi = mid;
                else lo = mid + 1;
            }
            r = std::max<int64_t>(start + 1, lo - 1);
        } else {
            int64_t nz = 0;
            while (r < rows && r - start < R) {
                const int64_t l = h_rp[r + 1] - h_rp[r];
                if (l > LT || nz + l > B) break;
                nz += l;
                r++;
            }
        }
        sortb.push_back({h_rp[start], h_rp[r], (int32_t)start, (int32_t)r, -1, 0});
    }
    int64_t maxrows = 1;   // LDS accumulators
    for (const RowBlock &b : sortb) maxrows = std::max<int64_t>(maxrows, b.row_end - b.row_begin);
    p->sorted_lds = (int)(maxrows * sizeof(double));
    // seg of a sorted block = index of its first 256-entry supergroup in gbase
    for (RowBlock &b : sortb) {
        b.seg = (int32_t)ngroups;
        ngroups += (b.nz_end - b.nz_begin + 255) / 256;
    }
    std::stable_sort(longrows.begin(), longrows.end(), [](const auto &x, const auto &y) { return x.first > y.first; });
    for (const auto &lr : longrows) {
        const int32_t row = lr.second;
        const int32_t nseg = (int32_t)((lr.first + kSegNnz - 1) / kSegNnz);
        const int32_t sp = (int32_t)lfirst.size();
        lfirst.push_back(nsegs);
        lnseg.push_back(nseg);
        for (int32_t sgm = 0; sgm < nseg; sgm++) {
            const int64_t zb = h_rp[row] + (int64_t)sgm * kSegNnz;
            longb.push_back({zb, std::min(zb + kSegNnz, h_rp[row + 1]), row, row + 1, sp, sgm});
        }
        nsegs += nseg;
    }
    all = longb;
    all.insert(all.end(), sortb.begin(), sortb.end());
    return GX_SUCCESS;
}

int PlanCtx::upload_blocks() {
    p->nblocks = (uint32_t)all.size();
    p->nlong_blocks = (uint32_t)longb.size();
    p->nlong = (uint32_t)lfirst.size();
    p->nsegs = (uint32_t)nsegs;
    GX_TRY(p->blocks.alloc(std::max<size_t>(all.size(), 1)));
    GX_TRY(p->long_first.alloc(std::max<size_t>(lfirst.size(), 1)));
    GX_TRY(p->long_nseg.alloc(std::max<size_t>(lnseg.size(), 1)));
    GX_TRY(p->long_part.alloc(std::max<size_t>(nsegs, 1)));
    GX_TRY(p->long_ticket.alloc(std::max<size_t>(lfirst.size(), 1)));
    if (!all.empty())
        GX_HIP_TRY(hipMemcpy(p->blocks.p, all.data(), all.size() * sizeof(RowBlock), hipMemcpyHostToDevice));
    if (!lfirst.empty()) {
        GX_HIP_TRY(hipMemcpy(p->long_first.p, lfirst.data(), lfirst.size() * 4, hipMemcpyHostToDevice));
        GX_HIP_TRY(hipMemcpy(p->long_nseg.p, lnseg.data(), lnseg.size() * 4, hipMemcpyHostToDevice));
    }
    GX_HIP_TRY(hipMemset(p->long_ticket.p, 0, p->long_ticket.n * 4));
    d_sort = p->blocks.p + longb.size();
    return GX_SUCCESS;
}

// The key pass: over the local rows (gather), or chunk by chunk from the source side while the
// source columns are still being uploaded (PrPart::job, gx_pagerank_csr).
template <typename K>
int PlanCtx::key_pass(const KeySrc &ks, int64_t nslabs, K *keys, uint16_t *vals) {
    if (!p->job) {
        const unsigned kgrid = grid_for((uint64_t)((nslabs + kKeyU - 1) / kKeyU) * kWave, 256, 16384);
        hipLaunchKernelGGL(k_sorted_keys<K>, dim3(kgrid), dim3(256), 0, s, ks, (int64_t)nnz, srow.p, nslabs,
                           d_rowseg.p, keys, vals);
        return check_launch("k_sorted_keys");
    }
    const int64_t n_src = (int64_t)p->n_global;
    DBuf<int64_t> ssrow;
    GX_TRY(ssrow.alloc(nslabs + 1));
    GX_TRY(slab_rows(p->src_rp, n_src, nslabs, ssrow.p, s));
    UploadJob *job = p->job;
    for (size_t c = 0; c < job->ev.size(); c++) {
        GX_TRY(job->wait_chunk((int)c));
        GX_HIP_TRY(hipStreamWaitEvent(s, job->ev[c], 0));
        const int64_t e0 = c ? job->end[c - 1] : 0, e1 = job->end[c];
        const int64_t sl0 = e0 / kWave, sl1 = (e1 + kWave - 1) / kWave;   // chunks are 64-aligned
        hipLaunchKernelGGL(k_scatter_keys<K>, dim3(grid_for((uint64_t)(sl1 - sl0) * kWave, 256, 4096)), dim3(256),
                           0, s, ks, n_src, ssrow.p, sl0, sl1, (int64_t)nnz, d_rowseg.p, keys, vals);
        GX_TRY(check_launch("k_scatter_keys"));
    }
    GX_TRY(job->join());
    GX_HIP_TRY(hipStreamSynchronize(s));   // ssrow is freed on return
    return GX_SUCCESS;
}

// sci / spk / gbase: block-sorted columns and packed entries, by one radix sort of (segment,
// column) keys.
int PlanCtx::sort_columns() {
    GX_TRY(p->sci.alloc(std::max<uint64_t>(nnz, 1), 16));
    GX_TRY(p->spk.alloc(std::max<uint64_t>(nnz, 1), 16));
    GX_TRY(p->gbase.alloc(std::max<int64_t>(ngroups, 1), 16));
    // pair slots and run groups need an even chunk: a pair never straddles two ranks' chunks, and
    // x's zero slot chunk - 2 shares its pair with the dangling slot only
    if (k.pairs_on && (p->chunk & 1)) return fail(GX_INVALID_VALUE, "pr_plan_sorted: pair slots need an even chunk");
    if (k.runs_on && (p->chunk & 1)) return fail(GX_INVALID_VALUE, "pr_plan_sorted: run groups need an even chunk");
    if (nnz == 0) return GX_SUCCESS;
    // segments in row order: the sorted blocks and the LONG rows
    std::vector<std::pair<int32_t, int32_t>> order_;   // (first row, index: block i >= 0, LONG row -1 - j)
    for (size_t i = 0; i < sortb.size(); i++) order_.push_back({sortb[i].row_begin, (int32_t)i});
    for (size_t j = 0; j < longrows.size(); j++) order_.push_back({longrows[j].second, -1 - (int32_t)j});
    std::sort(order_.begin(), order_.end());
    for (const auto &o : order_) {
        const int32_t r0 = o.first;
        const bool blk = o.second >= 0;
        const int32_t r1 = blk ? sortb[o.second].row_end : r0 + 1;
        if (h_rp[r0] == h_rp[r1]) continue;   // no entries: no key names it (fewer segment bits)
        seg_row.push_back(r0);
        segd.push_back({h_rp[r0], h_rp[r1], blk ? sortb[o.second].seg : -1, 0});
    }
    seg_row.push_back((int32_t)rows);
    // column bits from the columns that occur: one rank's plan holds vertex ids < n (the
    // chunk's padding slots are never a column), a partition's the chunk layout
    int colbits = 1;
    const uint64_t ncols = p->nranks == 1 ? std::max<uint64_t>(p->n_global, 1) : p->chunk * (uint64_t)p->nranks;
    while ((1ull << colbits) < ncols) colbits++;
    int segbits = 1;
    while ((1ull << segbits) < segd.size()) segbits++;
    GX_TRY(d_seg_row.alloc(seg_row.size()));
    GX_TRY(d_segd.alloc(segd.size()));
    GX_HIP_TRY(hipMemcpyAsync(d_seg_row.p, seg_row.data(), seg_row.size() * 4, hipMemcpyHostToDevice, s));
    GX_HIP_TRY(hipMemcpyAsync(d_segd.p, segd.data(), segd.size() * sizeof(SegDesc), hipMemcpyHostToDevice, s));
    // 4-byte keys whenever the columns leave room: segments are contiguous entry ranges, so
    // groups of 2^(32 - colbits) of them sort independently with the segment's low bits in
    // the key (SYN-8_5: 556 segments x 2^23 columns = 33 bits, two groups of 32-bit keys, not one
    // 64-bit sort; one rocPRIM segmented sort of column-only keys ran 494 ms against 16 ms)
    const bool narrow = colbits <= 31 && !k.wide_keys;
    const int gbits = narrow ? std::min({segbits, 32 - colbits, k.sort_group_bits}) : segbits;
    const KeySrc ks{p->rp, rows, p->src_rp, p->src_ci, p->src_order, p->src_perm, d_seg_row.p,
                    (int32_t)segd.size(), colbits, (int32_t)((1ll << gbits) - 1)};
    const int64_t nslabs = (int64_t)((nnz + kWave - 1) / kWave);
    GX_TRY(srow.alloc(nslabs + 1));
    GX_TRY(slab_rows(p->rp, rows, nslabs, srow.p, s));
    GX_TRY(d_rowseg.alloc(std::max<int64_t>(rows, 1)));
    hipLaunchKernelGGL(k_row_seg, dim3((unsigned)std::min<size_t>(segd.size(), 65535)), dim3(256), 0, s, d_seg_row.p,
                       (int32_t)segd.size(), d_rowseg.p);
    GX_TRY(check_launch("k_row_seg"));
    // the pack's chunks: kPackChunk entries of one segment each, from the segment's start
    for (size_t g = 0; g < segd.size(); g++)
        for (int64_t z = segd[g].z0; z < segd[g].z1; z += kPackChunk) pch.push_back({z, (int32_t)g, 0});
    GX_TRY(d_pch.alloc(std::max<size_t>(pch.size(), 1)));
    if (!pch.empty())
        GX_HIP_TRY(hipMemcpyAsync(d_pch.p, pch.data(), pch.size() * sizeof(PackChunk), hipMemcpyHostToDevice, s));
    clk.mark("segments + slab rows");
    const unsigned pgrid = (unsigned)std::min<size_t>(std::max<size_t>(pch.size(), 1), 1u << 20);
    const uint32_t colmask = (uint32_t)((1ull << colbits) - 1);
    // keys and values in the kept plan scratch: [k0 | k1 | v0 | v1]
    const size_t kb = narrow ? 4 : 8, align = 256;
    auto up = [&](size_t x) { return (x + align - 1) / align * align; };
    const size_t kbytes = up((size_t)nnz * kb), vbytes = up((size_t)nnz * 2);
    char *scr = nullptr;
    GX_TRY(plan_scratch(2 * kbytes + 2 * vbytes, reinterpret_cast<void **>(&scr)));
    uint16_t *v0 = reinterpret_cast<uint16_t *>(scr + 2 * kbytes), *v1 = reinterpret_cast<uint16_t *>(scr + 2 * kbytes + vbytes);
    clk.mark("key buffers");
    auto pack = [&](auto *k1) {
        using K = std::remove_pointer_t<decltype(k1)>;
        hipLaunchKernelGGL(k_sorted_pack<K>, dim3(pgrid), dim3(256), 0, s, d_segd.p, d_pch.p, (int64_t)pch.size(), k1, v1,
                           colmask, p->sci.p, p->spk.p, p->gbase.p);
    };
    if (narrow) {
        uint32_t *k0 = reinterpret_cast<uint32_t *>(scr), *k1 = reinterpret_cast<uint32_t *>(scr + kbytes);
        GX_TRY(key_pass(ks, nslabs, k0, v0));
        clk.mark("keys");
        const size_t G = (size_t)1 << gbits;
        for (size_t g0 = 0; g0 < segd.size(); g0 += G) {
            const size_t g1 = std::min(segd.size(), g0 + G) - 1;
            const int64_t z0 = segd[g0].z0, z1 = segd[g1].z1;
            GX_TRY(sort_pairs_u32_u16(k0 + z0, k1 + z0, v0 + z0, v1 + z0, (size_t)(z1 - z0), gbits + colbits, s));
        }
        clk.mark("sort");
        pack(k1);
    } else {
        uint64_t *k0 = reinterpret_cast<uint64_t *>(scr), *k1 = reinterpret_cast<uint64_t *>(scr + kbytes);
        GX_TRY(key_pass(ks, nslabs, k0, v0));
        GX_TRY(sort_pairs_u64_u16(k0, k1, v0, v1, (size_t)nnz, segbits + colbits, s));
        pack(k1);
    }
    GX_TRY(check_launch("k_sorted_pack"));
    clk.mark("keys + sort + pack");
    return GX_SUCCESS;
}

// What the three regions do alike: the per-block buffers, the region's cost kernel (launch_cost,
// filling r.fill), then k_narrow_split from the end of the region before it (prev, null: the
// block's start), and split and code on their way back to the host.  Off: an empty region.
template <typename CostLaunch>
int PlanCtx::split_region(Region &r, const Region *prev, bool on, CostLaunch launch_cost, const char *cost_name,
                          const char *split_name, const uint32_t *codes, int w4, int enable, int64_t min_entries) {
    const unsigned nsb = (unsigned)sortb.size();
    const uint32_t *q = prev ? prev->split.p : nullptr;
    GX_TRY(r.split.alloc(nsb));
    GX_TRY(r.code.alloc(nsb));
    GX_TRY(r.beg.alloc(nsb));
    if (!on) {
        if (q) GX_HIP_TRY(hipMemcpyAsync(r.split.p, q, nsb * 4, hipMemcpyDeviceToDevice, s));
        else GX_HIP_TRY(hipMemsetAsync(r.split.p, 0, nsb * 4, s));
        return GX_SUCCESS;
    }
    GX_TRY(r.fill.alloc(std::max<int64_t>(ngroups, 1)));
    GX_TRY(r.off.alloc(std::max<int64_t>(ngroups, 1)));
    launch_cost();
    GX_TRY(check_launch(cost_name));
    hipLaunchKernelGGL(k_narrow_split, dim3(nsb), dim3(1024), 0, s, d_sort, r.fill.p, codes, w4, q, enable, min_entries,
                       r.split.p, r.code.p, r.off.p);
    GX_TRY(check_launch(split_name));
    GX_HIP_TRY(hipMemcpyAsync(r.h_split.data(), r.split.p, nsb * 4, hipMemcpyDeviceToHost, s));
    GX_HIP_TRY(hipMemcpyAsync(r.h_code.data(), r.code.p, nsb * 4, hipMemcpyDeviceToHost, s));
    return GX_SUCCESS;
}

// A block's column-sorted entries recoded from the front: the run region R, the pair prefix from
// R to Q, the narrow prefix from Q, in bank-aware order; then the wide rest's lane permutation.
int PlanCtx::build_regions() {
    const unsigned nsb = (unsigned)sortb.size();
    for (Region *r : {&run, &pair, &nar}) r->resize(nsb);
    p->ncodes = p->nnarrow = p->npair = p->npfill = p->npslots = p->nrun = p->nrpad = p->nrcodes = 0;
    if (nnz == 0 || sortb.empty()) return GX_SUCCESS;
    const dim3 per_block(64, nsb);
    GX_TRY(npfill.alloc(1));
    GX_HIP_TRY(hipMemsetAsync(npfill.p, 0, sizeof(unsigned long long), s));
    GX_TRY(split_region(run, nullptr, k.runs_on,
                        [&] { hipLaunchKernelGGL(k_run_cost, per_block, dim3(256), 0, s, d_sort, p->sci.p, run.fill.p); },
                        "k_run_cost", "k_narrow_split (runs)", nullptr, k.run_fill_cost, 1, k.run_min));
    if (k.pairs_on) GX_TRY(pslots.alloc(std::max<int64_t>(ngroups, 1)));
    GX_TRY(split_region(pair, &run, k.pairs_on,
                        [&] {
                            hipLaunchKernelGGL(k_pair_cost, per_block, dim3(256), 0, s, d_sort, p->sci.p, run.split.p,
                                               pslots.p, pair.fill.p);
                        },
                        "k_pair_cost", "k_narrow_split (pairs)", pslots.p, k.pair_fill_cost, 1, k.pair_min));
    GX_TRY(split_region(nar, &pair, true,
                        [&] {
                            hipLaunchKernelGGL(k_narrow_cost, per_block, dim3(256), 0, s, d_sort, p->sci.p, pair.split.p,
                                               nar.fill.p);
                        },
                        "k_narrow_cost", "k_narrow_split", nullptr, 4, k.narrow_on, k.narrow_min));
    GX_HIP_TRY(hipStreamSynchronize(s));
    if (!k.pairs_on) pair.h_split = run.h_split;   // (without pair slots the pair prefix is empty: Q = R)
    for (size_t i = 0; i < nsb; i++) {
        // the run region's codes: the run that R cuts is padded like the others
        run.h_code[i] = (uint32_t)run_region_codes(run.h_code[i]);
        for (Region *r : {&run, &pair, &nar}) {
            r->h_beg[i] = (int64_t)r->total;
            r->total += (uint64_t)r->sgs(i) * r->sg;
        }
        const int64_t Er = upto(run, i), Ep = upto(pair, i);   // in run codes; run codes + pair slots
        p->nrun += (uint64_t)Er;
        p->nrpad += (uint64_t)run.h_code[i] - (uint64_t)Er;
        p->npair += (uint64_t)(Ep - Er);
        p->nnarrow += (uint64_t)(upto(nar, i) - Ep);
    }
    // the order inside the runs of both prefixes, now that they are known, before their codes
    if (k.bank_order) {
        clk.mark("prefix splits");
        hipLaunchKernelGGL(k_bank_order, per_block, dim3(kBankBS), 0, s, d_sort, run.split.p, pair.split.p, nar.split.p,
                           p->spk.p, p->sci.p);
        GX_TRY(check_launch("k_bank_order"));
        clk.mark("bank order");
    }
    // each region's table: padding everywhere and a null supergroup at the end, then each block's codes
    const uint32_t zero_pair = (uint32_t)((p->chunk - 2) >> 1);
    if (k.runs_on) {
        p->rnull_sg = (uint32_t)(run.total / kRunSg);
        p->nrcodes = run.total + kRunSg;
        GX_TRY(p->rpk.alloc(p->nrcodes, 16));
        GX_TRY(p->rpair.alloc(p->nrcodes / kRunGroup));
        hipLaunchKernelGGL(k_run_fill, dim3(grid_for(p->nrcodes, 256, 16384)), dim3(256), 0, s, p->rpk.p, p->nrcodes,
                           p->rpair.p, zero_pair);
        GX_TRY(check_launch("k_run_fill"));
        if (p->nrun) {
            GX_HIP_TRY(hipMemcpyAsync(run.beg.p, run.h_beg.data(), nsb * 8, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_run_emit, per_block, dim3(256), 0, s, d_sort, p->sci.p, p->spk.p, run.split.p, run.off.p,
                               run.beg.p, p->rpk.p, p->rpair.p);
            GX_TRY(check_launch("k_run_emit"));
        }
        clk.mark("run codes");
    }
    p->pnull_sg = (uint32_t)(pair.total / kPSg);
    p->npslots = pair.total + kPSg;
    GX_TRY(p->ppk.alloc(p->npslots, 16));
    GX_TRY(p->pbase.alloc(p->npslots / kPSg));
    hipLaunchKernelGGL(k_pair_fill, dim3(grid_for(p->npslots, 256, 16384)), dim3(256), 0, s, p->ppk.p, p->npslots,
                       p->pbase.p, p->pnull_sg, zero_pair);
    GX_TRY(check_launch("k_pair_fill"));
    if (p->npair) {
        GX_HIP_TRY(hipMemcpyAsync(pair.beg.p, pair.h_beg.data(), nsb * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_pair_emit, per_block, dim3(256), 0, s, d_sort, p->sci.p, p->spk.p, run.split.p, pair.split.p,
                           pair.code.p, pair.off.p, pair.beg.p, p->ppk.p, p->pbase.p, npfill.p);
        GX_TRY(check_launch("k_pair_emit"));
        unsigned long long nf = 0;
        GX_HIP_TRY(hipMemcpyAsync(&nf, npfill.p, sizeof nf, hipMemcpyDeviceToHost, s));
        GX_HIP_TRY(hipStreamSynchronize(s));
        p->npfill = nf;
    }
    p->null_sg = (uint32_t)(nar.total / kNSg);
    p->ncodes = nar.total + kNSg;
    GX_TRY(p->npk.alloc(p->ncodes, 16));
    GX_TRY(p->nbase.alloc(p->ncodes / kNSg));
    GX_HIP_TRY(hipMemcpyAsync(nar.beg.p, nar.h_beg.data(), nsb * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_narrow_fill, dim3(grid_for(p->ncodes, 256, 16384)), dim3(256), 0, s, p->npk.p, p->ncodes,
                       p->nbase.p, p->null_sg, (uint32_t)(p->chunk - 2));
    GX_TRY(check_launch("k_narrow_fill"));
    hipLaunchKernelGGL(k_narrow_emit, per_block, dim3(256), 0, s, d_sort, p->sci.p, p->spk.p, pair.split.p, nar.split.p,
                       nar.code.p, nar.off.p, nar.beg.p, p->npk.p, p->nbase.p);
    GX_TRY(check_launch("k_narrow_emit"));
    clk.mark("narrow codes");
    if (k.laneperm) {
        hipLaunchKernelGGL(k_sorted_laneperm, per_block, dim3(256), 0, s, d_sort, nar.split.p, p->spk.p, p->sci.p);
        GX_TRY(check_launch("k_sorted_laneperm"));
    }
    return GX_SUCCESS;
}

// T, the entries per unit: GX_PR_UNIT_NNZ, a quarter block, or (huge graphs, GX_PR_UNIT_SIM=1)
// the size whose simulated launch is shortest.  Host work, under the region kernels.
int PlanCtx::choose_unit_size() {
    if (k.unit_nnz_set || (!k.huge && !k.unit_sim)) {
        // a quarter block: measured best on SYN-7_5 (256 Ki of 1 Mi: 100 us per launch;
        // 232 Ki: 130) and on its 1/8 partition (32 Ki of 128 Ki: 33.5 us; 24 Ki: 38.8; 64 Ki: 47.7)
        T = k.unit_nnz_set ? k.unit_nnz : std::max<int64_t>(kRound, (k.B / 4 + kRound - 1) / kRound * kRound);
        return GX_SUCCESS;
    }
    std::vector<int64_t> ents, effs, rws, lsegs;
    for (size_t i = 0; i < sortb.size(); i++) {
        ents.push_back(entries(i));
        effs.push_back(eff_entries(i));
        rws.push_back(sortb[i].row_end - sortb[i].row_begin);
    }
    for (const RowBlock &b : longb) lsegs.push_back(b.nz_end - b.nz_begin);
    double best = 0.0;
    const int64_t emax = *std::max_element(ents.begin(), ents.end());
    // candidates: every round up to 64 rounds, then 4 % apart (the makespan curve is flat there),
    // simulated on up to 8 host threads (13 ms on one thread for SYN-8_5), then scanned in order
    std::vector<int64_t> cand;
    for (int64_t t = kRound; t <= std::max<int64_t>(kRound, emax);
         t = t < 64 * kRound ? t + kRound : (t + t / 25 + kRound - 1) / kRound * kRound)
        cand.push_back(t);
    std::vector<double> span(cand.size());
    const int nth = (int)std::max<size_t>(1, std::min<size_t>({8, cand.size(),
                                                               (size_t)std::max(1u, std::thread::hardware_concurrency())}));
    std::vector<std::thread> th;
    for (int w = 0; w < nth; w++)
        th.emplace_back([&, w]() {
            for (size_t i = (size_t)w; i < cand.size(); i += (size_t)nth)
                span[i] = pr_unit_makespan(ents, effs, rws, lsegs, cand[i], (int)cus, k.unit_by_cost, k.uc);
        });
    for (auto &x : th) x.join();
    for (size_t i = 0; i < cand.size(); i++)
        if (T == 0 || span[i] < best * 0.999) {
            best = span[i];
            T = cand[i];
        }
    if (k.verbose) std::fprintf(stderr, "[gx_pr] unit size %lld: simulated launch %.1f us\n", (long long)T, best);
    if (k.verbose >= 2) {
        // the blocks whose units cost most at the chosen size
        std::vector<std::pair<double, size_t>> top;
        for (size_t i = 0; i < ents.size(); i++)
            top.push_back({pr_unit_makespan({ents[i]}, {effs[i]}, {rws[i]}, {}, T, 1 << 14, k.unit_by_cost, k.uc), i});
        std::sort(top.begin(), top.end(), std::greater<>());
        for (size_t q = 0; q < std::min<size_t>(8, top.size()); q++) {
            const size_t i = top[q].second;
            std::fprintf(stderr, "[gx_pr]   block %zu: entries %lld eff %lld rows %lld -> longest unit %.1f us\n", i,
                         (long long)ents[i], (long long)effs[i], (long long)rws[i], top[q].first);
        }
    }
    return GX_SUCCESS;
}

// Isolated rows in closed form (GX_PR_ISO_CLOSED=0: off), with the fused dangling sum only.  A
// block without entries whose rows all have out-degree 0 holds vertices without any edge: score
// teleport, x never gathered, dangling mass rows * teleport.  Such rows are known without a look at
// every out-degree where they lie past `live` (a partition's xd rows) or inside the plan's one
// range of dangling rows (the hub-first single plan).  These blocks' units and slots go last;
// every launch but a run's last leaves them out (pr_step_sorted).
bool PlanCtx::iso_block(const RowBlock &b) const {
    if (!k.iso_closed || p->nd == 0 || long_dangling) return false;
    if (b.nz_begin != b.nz_end || b.row_end <= b.row_begin) return false;
    if ((uint64_t)b.row_begin >= p->live) return true;
    return p->d_range && b.row_begin >= p->d0 && b.row_end <= p->d0 + (int64_t)p->nd;
}

// GX_PR_VERBOSE: the plan's totals, then the pair and run prefixes (blocks that have one and its
// mean length in supergroups, counted from the end of the region before it).
void PlanCtx::print_plan(int32_t parts, int64_t slab) const {
    std::fprintf(stderr, "[gx_pr] plan: rows %lld nnz %llu unit_nnz %lld block_nnz %d "
                 "long_nnz %d: %zu sorted blocks, %u LONG blocks (%u rows), %u units, %d multi-unit blocks, "
                 "slab %lld doubles; narrow %llu entries in %llu codes\n",
                 (long long)rows, (unsigned long long)nnz, (long long)T,
                 p->sorted_nnz, p->long_nnz, sortb.size(), p->nlong_blocks, p->nlong, p->nunits, parts,
                 (long long)slab, (unsigned long long)p->nnarrow, (unsigned long long)p->ncodes);
    size_t nq = 0;
    auto mean = [&](const Region &r, const Region *prev) {
        uint64_t sum = 0;
        nq = 0;
        for (size_t i = 0; i < sortb.size(); i++) {
            const uint32_t q = r.h_split[i] - (prev ? prev->h_split[i] : 0u);
            nq += q > 0;
            sum += q;
        }
        return nq ? (double)sum / (double)nq : 0.0;
    };
    const double mq = mean(pair, &run);
    if (k.pairs_on)
        std::fprintf(stderr, "[gx_pr] pairs: %llu entries and %llu filler halves in %llu slots (padding included); "
                     "%zu of %zu blocks with a pair prefix, mean Q %.1f supergroups\n",
                     (unsigned long long)p->npair, (unsigned long long)p->npfill, (unsigned long long)p->npslots, nq,
                     sortb.size(), mq);
    const double mr = mean(run, nullptr);
    std::fprintf(stderr, "[gx_pr] runs: %llu entries and %llu padding codes in %llu codes (supergroup padding "
                 "included); %zu of %zu blocks with a run prefix, mean R %.1f supergroups\n",
                 (unsigned long long)p->nrun, (unsigned long long)p->nrpad, (unsigned long long)p->nrcodes, nq,
                 sortb.size(), mr);
}

// Units of the sorted blocks (ceil(weighted entries / T) per block, at most one per round), the
// slabs and stripes of the multi-unit blocks, the units' launch order and the closed-form counts.
int PlanCtx::cut_units() {
    std::vector<SortedUnit> units;
    int64_t slab = 0;
    int32_t parts = 0;
    for (size_t i = 0; i < sortb.size(); i++) {
        const RowBlock &b = sortb[i];
        const int64_t E = entries(i);
        const int64_t rounds = (E + kRound - 1) / kRound;
        // units per block: by weighted entries (eff_entries; = E unless the plan weights wide
        // entries, GX_PR_WIDE_COST), as the simulation that picked T counts them
        const int64_t Ek = k.unit_by_cost ? eff_entries(i) : E;
        const int32_t nu = (int32_t)std::max<int64_t>(1, std::min<int64_t>(rounds, (Ek + T - 1) / T));
        const int64_t rows_b = b.row_end - b.row_begin;
        const int64_t wide = b.nz_begin + 256 * (int64_t)nar.h_split[i];   // the wide part's first entry
        // lo, hi, step, slab, nbeg, nsg, blk, part, unit, nunits, then the block's seg, z0, z1, r0, r1,
        // then pbeg, psg, rsg, rbeg
        for (int32_t j = 0; j < nu; j++)
            units.push_back({wide + (int64_t)kRound * j, b.nz_end, (int64_t)kRound * nu, nu > 1 ? slab : 0, nar.h_beg[i],
                             nar.sgs(i), (int32_t)(longb.size() + i), nu > 1 ? parts : -1, j, nu, b.seg, b.nz_begin,
                             b.nz_end, b.row_begin, b.row_end, pair.h_beg[i], pair.sgs(i), run.sgs(i), run.h_beg[i]});
        if (k.verbose == 3)
            std::fprintf(stderr, "[gx_pr blk] %zu E %lld En %lld codes %u eff %lld k %d rows %lld\n", i, (long long)E,
                         (long long)(upto(nar, i) - upto(pair, i)), nar.h_code[i], (long long)eff_entries(i), nu,
                         (long long)rows_b);
        if (nu > 1) {
            if (p->comb_kernel)
                for (int64_t s0 = 0; s0 < rows_b; s0 += kCombBS)
                    stripes.push_back({slab, b.row_begin, (int32_t)rows_b, (int32_t)s0,
                                       (int32_t)std::min<int64_t>(rows_b, s0 + kCombBS), nu, -1});
            multi[longb.size() + i] = 1;
            slab += (int64_t)nu * rows_b;
            parts++;
        }
    }
    // Largest units first: the launch lasts as long as the unit that finishes last, so the
    // big units start in the first wave and the small ones fill the gaps at the end.  Cost ~
    // entries + 4 per row (zeroing, epilogue).  Ties keep block order, so a block's units
    // stay adjacent.
    auto cost = [&](const SortedUnit &u) {
        const size_t i = (size_t)u.blk - longb.size();
        return (eff_entries(i) + u.nunits - 1) / u.nunits + k.row_cost * (sortb[i].row_end - sortb[i].row_begin);
    };
    auto iso_unit = [&](const SortedUnit &u) { return iso_block(sortb[u.blk - longb.size()]); };
    std::stable_sort(units.begin(), units.end(), [&](const SortedUnit &x, const SortedUnit &y) {
        const bool ix = iso_unit(x), iy = iso_unit(y);
        if (ix != iy) return iy;   // the closed-form blocks last, whatever their cost
        return cost(x) > cost(y);
    });
    for (const SortedUnit &u : units)
        if (iso_unit(u)) {
            p->iso_units++;
            p->iso_rows += (uint64_t)(u.r1 - u.r0);
        }
    // something has to run to write the sum: a graph of isolated rows alone keeps its items
    if (p->nlong_pad + (uint32_t)units.size() == p->iso_units) {
        p->iso_units = 0;
        p->iso_rows = 0;
    }
    // (Smallest first, or largest and smallest alternating, ran 88 and 120 us against 72 on SYN-7_5:
    // a block's interleaved units must run together.  Co-scheduling similar units on one XCD cut
    // the fabric reads of SYN-8_5 by 9 % and still ran slower)
    p->nunits = (uint32_t)units.size();
    if (k.verbose) print_plan(parts, slab);
    GX_TRY(p->units.alloc(units.size()));
    GX_HIP_TRY(hipMemcpy(p->units.p, units.data(), units.size() * sizeof(SortedUnit), hipMemcpyHostToDevice));
    GX_TRY(p->uslab.alloc(std::max<int64_t>(slab, 1)));
    GX_TRY(p->uticket.alloc(std::max<int32_t>(parts, 1)));
    GX_HIP_TRY(hipMemset(p->uticket.p, 0, p->uticket.n * 4));
    return GX_SUCCESS;
}

// Fused dangling sum: every dangling row in a sorted block (none in a LONG block), one slot per
// block (or stripe of a combined block) holding dangling rows; then the stripes' upload.
int PlanCtx::assign_dangling_slots() {
    std::vector<int32_t> slot(all.size(), -1);
    uint32_t nd = 0;
    auto dangling_in = [&](int64_t r0, int64_t r1) {
        if (p->d_range)   // the dangling rows are [d0, d0 + nd)
            return p->nd > 0 && r0 < p->d0 + (int64_t)p->nd && r1 > p->d0;
        for (int64_t r2 = r0; r2 < r1; r2++)
            if (h_outdeg[r2] == 0) return true;
        return false;
    };
    for (size_t i = longb.size(); i < all.size(); i++) {
        if (p->comb_kernel && multi[i]) continue;   // its stripes publish instead
        if (p->iso_units && iso_block(all[i])) continue;   // the last slots, below
        if (dangling_in(all[i].row_begin, all[i].row_end)) slot[i] = (int32_t)nd++;
    }
    for (CombStripe &c : stripes)
        if (dangling_in((int64_t)c.r0 + c.s0, (int64_t)c.r0 + c.s1)) c.dslot = (int32_t)nd++;
    // the closed-form blocks' slots last: a launch without them sums the slots before
    for (size_t i = longb.size(); i < all.size() && p->iso_units; i++)
        if (iso_block(all[i])) {
            slot[i] = (int32_t)nd++;
            p->iso_dblocks++;
        }
    p->fused_dangling = p->nd > 0 && nd > 0 && !long_dangling;
    p->ndblocks = nd;
    if (k.verbose)
        std::fprintf(stderr, "[gx_pr] closed-form isolated rows: %u of %u units, %llu rows, %u of %u dangling slots\n",
                     p->iso_units, p->nunits, (unsigned long long)p->iso_rows, p->iso_dblocks, nd);
    if (p->fused_dangling) {
        GX_TRY(p->dslot.alloc(std::max<size_t>(all.size(), 1)));
        GX_TRY(p->fdpart.alloc(nd));
        GX_TRY(p->fdticket.alloc(1));
        if (!all.empty()) GX_HIP_TRY(hipMemcpy(p->dslot.p, slot.data(), all.size() * 4, hipMemcpyHostToDevice));
        GX_HIP_TRY(hipMemset(p->fdticket.p, 0, 4));
    }
    p->ncstripes = (uint32_t)stripes.size();
    if (!stripes.empty()) {
        GX_TRY(p->cstripes.alloc(stripes.size()));
        GX_HIP_TRY(hipMemcpy(p->cstripes.p, stripes.data(), stripes.size() * sizeof(CombStripe), hipMemcpyHostToDevice));
    }
    return GX_SUCCESS;
}

}  // namespace

// Plan: rows longer than long_nnz -> LONG segment blocks (longest first); runs of the other
// rows with entries -> blocks of <= block_nnz entries and <= sorted_rows rows, entries sorted
// by column and cut into units; the trailing rows without entries -> row-range workgroups.
int pr_plan_sorted(PrPart *p, HostView<int64_t> h_rp, HostView<int32_t> h_outdeg) {
    PlanCtx c(p, h_rp, h_outdeg);
    GX_TRY(c.cut_blocks());
    GX_TRY(c.upload_blocks());
    c.clk.mark("blocks (host)");
    GX_TRY(c.sort_columns());
    GX_TRY(c.build_regions());
    p->ci = p->sci.p;   // the LONG rows read their (column-sorted) entries there
    c.clk.mark("laneperm");
    p->nsorted = (uint32_t)c.sortb.size();
    p->nlong_pad = (p->nlong_blocks + 7u) & ~7u;
    p->nunits = p->iso_units = p->iso_dblocks = 0;
    p->iso_rows = 0;
    for (const RowBlock &b : c.longb) c.long_dangling |= h_outdeg[b.row_begin] == 0;
    c.multi.assign(c.all.size(), 0);
    // the host search runs while the region kernels execute (the temporaries go when c does)
    if (!c.sortb.empty()) GX_TRY(c.choose_unit_size());
    GX_HIP_TRY(hipStreamSynchronize(c.s));
    if (!c.sortb.empty()) {
        c.clk.mark("unit size");
        GX_TRY(c.cut_units());
    }
    p->unit_nnz = c.T;
    GX_TRY(p->queue.alloc(2));
    GX_HIP_TRY(hipMemset(p->queue.p, 0, 2 * sizeof(uint32_t)));
    c.clk.mark("units");
    GX_TRY(c.assign_dangling_slots());
    c.clk.mark("dangling slots");
    return GX_SUCCESS;
}

}  // namespace gx

GX_MODULE_WARMER(pr_plan)
