// match_plan.hpp -- what the matcher's launch functions decide between their kernel launches: which knn2 kernel runs on how many
// splits of the train set, how the scratch buffers of SearchForInitialization and of the projection searches are sized and carved,
// the dynamic LDS of k_search_by_projection_batch, and the growth rules of the overflow-and-repeat contract.  Pure host arithmetic,
// no HIP (sbp_lds_offsets alone is also called by the kernel): csrc/match_kernels.hip asks for a plan or layout and then only ensures
// buffers and launches, tests/test_match_plan_cpu.py compiles this header with g++ and pins the rules as literals.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>

#include "../../include/orbfe.h"
#include "../../include/orbfe_math.h"   // ORBFE_HD

namespace orbfe {

// ---- constants the kernels and the plans share (their one definition)
constexpr int KNN_TILE = 256;      // k_knn2_tiles / k_knn2_merge: queries per workgroup, train descriptors per LDS tile
constexpr int KM_WAVES = 8;        // k_knn2_mfma: waves per workgroup, 32 queries each
constexpr int KM_CHUNK = 128;      // k_knn2_mfma: train descriptors spread into LDS at a time
constexpr int GRID_COLS = 64;      // FRAME_GRID_COLS / FRAME_GRID_ROWS of the reference's Frame
constexpr int GRID_ROWS = 48;
constexpr int SFI_MAXL0 = 1024;    // level-0 keypoints of a frame SearchForInitialization holds
constexpr int SFI_CURSOR_PAD = 64; // ints between two pairs' pool cursors: one cursor per 256 bytes
constexpr int SBP_CELLS = GRID_COLS * GRID_ROWS;
constexpr size_t MATCH_LDS_LIMIT = 150 * 1024;   // dynamic LDS the projection search asks for at most (a CU has 160 KB)
static_assert(KM_WAVES * 32 == KNN_TILE, "k_knn2_merge's query tiles are those of k_knn2_mfma: one x dimension for both grids");

// the switches of orbfe_debug_control: "knn2_path" 0 = the matrix cores wherever they apply, 1 = the VALU kernel, 2 = as 0
struct MatchSwitches {
    int knn2_path = 0;
};

struct Grid3 { int x = 0, y = 0, z = 0; };

// ---- knn2: all-pairs best / second-best
struct Knn2Plan {
    bool mfma = false;      // k_knn2_mfma, else k_knn2_tiles
    int nsplit = 1;         // parts of the train set; above 1 the scan writes partials and k_knn2_merge folds them in split order
    int chunk = 0;          // train descriptors per part, a multiple of the kernel's tile
    Grid3 scan;             // (query tiles, pairs, nsplit)
    int scan_block = 0;
    Grid3 merge;            // (query tiles, pairs, 1); x == 0: no merge
    size_t part_bytes = 0;  // each of the three partial buffers [pair][split][max_nq]; 0 with one split
};

inline Knn2Plan plan_knn2(int max_nq, int max_nt, int npairs, int init, const MatchSwitches& sw)
{
    Knn2Plan p;
    // the matrix-core kernel holds a train index in 16 bits of its keys and needs a finite `init`
    p.mfma = max_nt <= 65535 && init > 0 && sw.knn2_path != 1;
    // split the train set when there are too few (query-tile, pair) workgroups to fill 256 CUs
    const int qtiles = (max_nq + KNN_TILE - 1) / KNN_TILE;
    const long long wgs = (long long)qtiles * npairs;
    const int tile = p.mfma ? KM_CHUNK : KNN_TILE;
    const int max_split = (max_nt + tile - 1) / tile;
    int nsplit = 1;
    if (p.mfma) {
        // k_knn2_mfma: 8 waves of ~110 registers -> two workgroups per CU, 512 resident; the split aims at ONE round of them (a second,
        // half-empty round costs as much as a full one), in whole 128-descriptor chunks
        if (wgs < 512) nsplit = (int)std::max<long long>(1, std::min<long long>(512 / wgs, max_split));
    } else {
        // k_knn2_tiles: 1024 workgroups of 256 threads, in whole 256-descriptor tiles
        if (wgs < 1024) nsplit = (int)std::max<long long>(1, std::min<long long>((1024 + wgs - 1) / wgs, max_split));
    }
    p.chunk = (max_nt + nsplit - 1) / nsplit;
    p.chunk = std::max(tile, (p.chunk + tile - 1) / tile * tile);
    p.nsplit = std::max(1, (max_nt + p.chunk - 1) / p.chunk);   // whole chunks may cover the train set in fewer parts
    p.scan.x = qtiles; p.scan.y = npairs; p.scan.z = p.nsplit;
    p.scan_block = p.mfma ? KM_WAVES * 64 : KNN_TILE;
    if (p.nsplit > 1) {
        p.merge.x = qtiles; p.merge.y = npairs; p.merge.z = 1;
        p.part_bytes = (size_t)npairs * p.nsplit * max_nq * 4;
    }
    return p;
}

// ---- SearchForInitialization: a pair's candidate rows share one dense pool; a pool that turns out too small is flagged, grown by the
// status call (or the host wrapper) and the batch repeated.  16 K entries hold a 640 x 480 / 1000-feature pair at window 100 more
// than twice.
constexpr int SFI_POOL_MIN = 16384;
inline int sfi_pool_floor(int now) { return std::max((now + 3) / 4 * 4, SFI_POOL_MIN); }
// the pool after a pair needed `needed` entries
inline int sfi_pool_after(int now, int needed) { return needed > now ? (needed + 1023) / 1024 * 1024 : now; }

// What the two flag words -- [0] level-0 keypoints of a frame beyond SFI_MAXL0, [1] pool entries a pair needed -- mean: the level-0
// count goes with the error, also when a pool overflowed in the same batch (the pool is grown all the same).
struct SfiFlagsDecision {
    int need = 0;        // 0, the level-0 count that does not fit, or the pool size a pair needed
    int err = ORBFE_OK;  // ORBFE_ERR_CAPACITY for the level-0 count
    int pool = 0;        // the pool size from here on
    bool clear = false;  // a flag was raised: zero the words behind the read
};
inline SfiFlagsDecision sfi_flags_decision(int level0, int pool_needed, int pool_now)
{
    SfiFlagsDecision d;
    d.clear = level0 || pool_needed;
    d.pool = sfi_pool_after(pool_now, pool_needed);
    d.need = level0 > SFI_MAXL0 ? level0 : pool_needed;
    d.err = level0 > SFI_MAXL0 ? ORBFE_ERR_CAPACITY : ORBFE_OK;
    return d;
}

struct SfiLayout {
    int nframes = 0, pool = 0;   // frames of the batch; pool entries per pair after the floor rule
    size_t cnt_bytes = 0, idx_bytes = 0, dist_bytes = 0, scratch_bytes = 0;   // csr_cnt, csr_idx, csr_dist, scratch
    // SfiGrid's arrays.  In csr_cnt, as int offsets: nl0 | nq | one cursor per pair, SFI_CURSOR_PAD ints apart
    size_t nl0 = 0, nq = 0, cursor = 0;
    // in csr_idx, as byte offsets: [frame][SFI_MAXL0] each, widest element first, so every array is aligned to its element
    size_t desc = 0, xy = 0, sorted = 0, qxy = 0, ang = 0, query = 0;
};

inline SfiLayout plan_sfi(int npairs, int pool_entries_now)
{
    SfiLayout l;
    l.nframes = npairs + 1;
    l.pool = sfi_pool_floor(pool_entries_now);
    const size_t nf = (size_t)l.nframes, F = nf * SFI_MAXL0;
    l.nl0 = 0; l.nq = nf; l.cursor = 2 * nf;
    l.cnt_bytes = nf * (2 + SFI_CURSOR_PAD) * 4 + 64;
    size_t b = 0;
    l.desc = b; b += F * 32;     // uint4 x 2
    l.xy = b; b += F * 8;        // float2
    l.sorted = b; b += F * 4;    // uint32_t
    l.qxy = b; b += F * 8;       // float2
    l.ang = b; b += F * 4;       // float
    l.query = b; b += F * 2;     // uint16_t
    l.idx_bytes = b + 256;
    // k_sfi_accept prefetches a row's next 64 entries unconditionally: up to 63 entries past the last pool
    l.dist_bytes = (size_t)npairs * l.pool * 4 + 512;
    l.scratch_bytes = (size_t)npairs * SFI_MAXL0 * 4;
    return l;
}

// ---- the projection searches (k_search_by_projection_batch): a frame's grid lives in dynamic LDS, sized by the keypoint capacity
// rounded up to a power of two (ncap); the candidate rows live in HBM at the workspace's stride.
struct SbpLdsOffsets { int sorted, xy, cell0, lvl, taken, end; };   // bytes from the start of the dynamic LDS

// The one statement of that LDS: the launcher sizes it from `end`, sbp_frame carves it by the five offsets.  Signed ints, as the
// pointer steps they stand for were: the kernel's address arithmetic is then the compiler's own for `s_sorted + ncap` and so on
// (unsigned offsets fold differently).  ncap <= 8192 here, far from any overflow.
ORBFE_HD SbpLdsOffsets sbp_lds_offsets(int ncap)
{
    SbpLdsOffsets o;
    o.sorted = 0;                             // uint32_t[ncap]: (cell << 16) | index, ascending
    o.xy = o.sorted + ncap * 4;               // float2[ncap], by rank
    o.cell0 = o.xy + ncap * 8;                // uint16_t[SBP_CELLS + 2]: first rank of every cell, SBP_CELLS + 1 entries in use
    o.lvl = o.cell0 + (SBP_CELLS + 2) * 2;    // uint8_t[ncap], by rank
    o.taken = o.lvl + ncap;                   // uint8_t[ncap], by rank
    o.end = o.taken + ncap;
    return o;
}

constexpr int SBP_STRIDE_MIN = 128;
// the longest candidate list of a search that overflowed decides the row stride of the next one
inline int sbp_stride_after(int now, int overflow) { return overflow > now ? (overflow + 63) / 64 * 64 : now; }

struct SbpLayout {
    int err = ORBFE_OK;   // ORBFE_OK, or why this capacity is refused (then nothing else below is meaningful)
    char msg[96] = "";
    int ncap = 0;         // power of two >= capacity, at least 64
    SbpLdsOffsets lds{};  // the carving
    size_t lds_bytes = 0; // what the launch asks for
    int stride = 0;       // candidate row stride after the floor rule
    size_t rank_bytes = 0, dist_bytes = 0, cnt_bytes = 0;   // the rows' ranks (u16), distances (u8) and lengths (int)
};

inline SbpLayout plan_sbp(int capacity, int qcapacity, int nframes, int stride_now)
{
    SbpLayout l;
    if (capacity > 65535) {
        l.err = ORBFE_ERR_INVALID;
        snprintf(l.msg, sizeof l.msg, "more than 65535 keypoints per frame are unsupported");
        return l;
    }
    l.ncap = 64;
    while (l.ncap < capacity) l.ncap <<= 1;
    l.lds = sbp_lds_offsets(l.ncap);
    l.lds_bytes = (size_t)l.lds.end + 64;
    if (l.lds_bytes > MATCH_LDS_LIMIT) {
        l.err = ORBFE_ERR_CAPACITY;
        snprintf(l.msg, sizeof l.msg, "%d keypoints do not fit the grid kernel's LDS", capacity);
        return l;
    }
    l.stride = std::max(stride_now, SBP_STRIDE_MIN);
    const size_t NQ = (size_t)nframes * qcapacity;
    l.rank_bytes = NQ * l.stride * 2;
    l.dist_bytes = NQ * l.stride;
    l.cnt_bytes = NQ * 4;
    return l;
}

// ---- orbfe_fuse_search_batch_device: the projected queries, and `obest`: the result arrays nobody asked for and the two count arrays
struct FuseBatchLayout {
    size_t q_bytes = 0, obest_bytes = 0;
    // int offsets into obest: four arrays of nkf * nmp, then nq[nkf], nmatches[nkf]
    size_t best_level = 0, second_dist = 0, second_level = 0, match = 0, nq = 0, nmatches = 0;
};

inline FuseBatchLayout plan_fuse_batch(int nkf, int nmp)
{
    FuseBatchLayout l;
    const size_t NQ = (size_t)nkf * nmp;
    l.q_bytes = NQ * sizeof(orbfe_window_query);
    l.best_level = 0; l.second_dist = NQ; l.second_level = 2 * NQ; l.match = 3 * NQ;
    l.nq = 4 * NQ; l.nmatches = l.nq + nkf;
    l.obest_bytes = (l.nmatches + nkf) * 4 + 256;
    return l;
}

} // namespace orbfe
