// C entry points over csrc/match_plan.hpp for tests/test_match_plan_cpu.py (built with g++ by tests/match_plan_build.py: the header
// has no HIP in it).  With -DMATCH_PLAN_MAIN the same source is a program that runs the knn2 sweep and walks the layouts, for a run
// under AddressSanitizer and UBSan.  Test infrastructure only.
#include <cstdio>
#include <cstring>

#include "../orb_slam2_aruco_amd/csrc/match_plan.hpp"

using namespace orbfe;

extern "C" {

// out: KNN_TILE, KM_WAVES, KM_CHUNK, SFI_MAXL0, SFI_CURSOR_PAD, GRID_COLS, GRID_ROWS, SBP_CELLS, MATCH_LDS_LIMIT
void mplan_constants(long long* out)
{
    const long long v[9] = {KNN_TILE, KM_WAVES, KM_CHUNK, SFI_MAXL0, SFI_CURSOR_PAD, GRID_COLS, GRID_ROWS, SBP_CELLS, (long long)MATCH_LDS_LIMIT};
    memcpy(out, v, sizeof v);
}

// out: mfma, nsplit, chunk, scan x y z, scan_block, merge x y z, part_bytes
void mplan_knn2(int max_nq, int max_nt, int npairs, int init, int knn2_path, long long* out)
{
    MatchSwitches sw;
    sw.knn2_path = knn2_path;
    const Knn2Plan p = plan_knn2(max_nq, max_nt, npairs, init, sw);
    const long long v[11] = {p.mfma, p.nsplit, p.chunk, p.scan.x, p.scan.y, p.scan.z, p.scan_block, p.merge.x, p.merge.y, p.merge.z, (long long)p.part_bytes};
    memcpy(out, v, sizeof v);
}

// out: nframes, pool, cnt_bytes, idx_bytes, dist_bytes, scratch_bytes, nl0, nq, cursor, desc, xy, sorted, qxy, ang, query
void mplan_sfi(int npairs, int pool_now, long long* out)
{
    const SfiLayout l = plan_sfi(npairs, pool_now);
    const long long v[15] = {l.nframes, l.pool, (long long)l.cnt_bytes, (long long)l.idx_bytes, (long long)l.dist_bytes, (long long)l.scratch_bytes,
                             (long long)l.nl0, (long long)l.nq, (long long)l.cursor, (long long)l.desc, (long long)l.xy, (long long)l.sorted,
                             (long long)l.qxy, (long long)l.ang, (long long)l.query};
    memcpy(out, v, sizeof v);
}

int mplan_sfi_pool_after(int now, int needed) { return sfi_pool_after(now, needed); }

// out: need, err, pool, clear
void mplan_sfi_flags(int level0, int pool_needed, int pool_now, int* out)
{
    const SfiFlagsDecision d = sfi_flags_decision(level0, pool_needed, pool_now);
    const int v[4] = {d.need, d.err, d.pool, d.clear};
    memcpy(out, v, sizeof v);
}

// out: sorted, xy, cell0, lvl, taken, end
void mplan_sbp_lds_offsets(int ncap, int* out)
{
    const SbpLdsOffsets o = sbp_lds_offsets(ncap);
    const int v[6] = {o.sorted, o.xy, o.cell0, o.lvl, o.taken, o.end};
    memcpy(out, v, sizeof v);
}

// out: err, ncap, lds_bytes, the six offsets, stride, rank_bytes, dist_bytes, cnt_bytes;  msg: the refusal's text
void mplan_sbp(int capacity, int qcapacity, int nframes, int stride_now, long long* out, char* msg, int msg_cap)
{
    const SbpLayout l = plan_sbp(capacity, qcapacity, nframes, stride_now);
    const long long v[13] = {l.err, l.ncap, (long long)l.lds_bytes, l.lds.sorted, l.lds.xy, l.lds.cell0, l.lds.lvl, l.lds.taken, l.lds.end,
                             l.stride, (long long)l.rank_bytes, (long long)l.dist_bytes, (long long)l.cnt_bytes};
    memcpy(out, v, sizeof v);
    if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "%s", l.msg);
}

int mplan_sbp_stride_after(int now, int overflow) { return sbp_stride_after(now, overflow); }

// out: q_bytes, obest_bytes, best_level, second_dist, second_level, match, nq, nmatches (the last six in ints)
void mplan_fuse_batch(int nkf, int nmp, long long* out)
{
    const FuseBatchLayout l = plan_fuse_batch(nkf, nmp);
    const long long v[8] = {(long long)l.q_bytes, (long long)l.obest_bytes, (long long)l.best_level, (long long)l.second_dist,
                            (long long)l.second_level, (long long)l.match, (long long)l.nq, (long long)l.nmatches};
    memcpy(out, v, sizeof v);
}

// The sweep of tests/test_match_plan_cpu.py: plans whose splits do not cover the train set exactly once, or whose chunk is no positive
// multiple of the kernel's tile.  *plans = how many were made.
int mplan_knn2_sweep(int* plans)
{
    static const int NQ[] = {1, 255, 256, 257, 1000, 5000};
    static const int NT[] = {0, 1, 127, 128, 129, 255, 256, 257, 1000, 5000, 65535, 65536};
    static const int NP[] = {1, 2, 7, 64, 511, 512, 513, 1024, 1025};
    int bad = 0, n = 0;
    for (int nq : NQ)
        for (int nt : NT)
            for (int np : NP)
                for (int path = 0; path < 3; path++) {
                    MatchSwitches sw;
                    sw.knn2_path = path;
                    const Knn2Plan p = plan_knn2(nq, nt, np, 256, sw);
                    const int tile = p.mfma ? KM_CHUNK : KNN_TILE;
                    const bool covers = (long long)p.nsplit * p.chunk >= nt;
                    const bool no_empty_split = p.nsplit == 1 || (long long)(p.nsplit - 1) * p.chunk < nt;
                    const bool whole_tiles = p.chunk > 0 && p.chunk % tile == 0;
                    if (!covers || !no_empty_split || !whole_tiles) bad++;
                    n++;
                }
    if (plans) *plans = n;
    return bad;
}

} // extern "C"

#ifdef MATCH_PLAN_MAIN
#include <vector>

// Walks every layout the way its user does: an array per part, every byte of every part written once (a byte claimed twice, or one
// outside the buffer, is counted; the sanitizers see the writes).
static int claim(std::vector<unsigned char>& buf, size_t off, size_t bytes)
{
    int twice = 0;
    for (size_t i = 0; i < bytes; i++) twice += buf.at(off + i)++ != 0;
    return twice;
}

int main()
{
    int plans = 0;
    const int bad = mplan_knn2_sweep(&plans);
    printf("knn2 sweep: %d plans, %d violations\n", plans, bad);
    int overlaps = 0;
    for (int npairs : {1, 2, 7}) {
        const SfiLayout l = plan_sfi(npairs, 0);
        const size_t F = (size_t)l.nframes * SFI_MAXL0;
        std::vector<unsigned char> idx(l.idx_bytes, 0), cnt(l.cnt_bytes, 0);
        overlaps += claim(idx, l.desc, F * 32) + claim(idx, l.xy, F * 8) + claim(idx, l.sorted, F * 4) + claim(idx, l.qxy, F * 8) +
                    claim(idx, l.ang, F * 4) + claim(idx, l.query, F * 2);
        overlaps += claim(cnt, l.nl0 * 4, (size_t)l.nframes * 4) + claim(cnt, l.nq * 4, (size_t)l.nframes * 4);
        for (int p = 0; p < npairs; p++) overlaps += claim(cnt, (l.cursor + (size_t)p * SFI_CURSOR_PAD) * 4, 4);
    }
    for (int capacity : {1, 64, 65, 1000, 8192}) {
        const SbpLayout l = plan_sbp(capacity, 100, 2, 0);
        const size_t n = (size_t)l.ncap;
        std::vector<unsigned char> lds(l.lds_bytes, 0);
        overlaps += claim(lds, l.lds.sorted, n * 4) + claim(lds, l.lds.xy, n * 8) + claim(lds, l.lds.cell0, (SBP_CELLS + 2) * 2) +
                    claim(lds, l.lds.lvl, n) + claim(lds, l.lds.taken, n);
    }
    {
        const int nkf = 3, nmp = 500;
        const FuseBatchLayout l = plan_fuse_batch(nkf, nmp);
        const size_t NQ = (size_t)nkf * nmp;
        std::vector<unsigned char> ob(l.obest_bytes, 0);
        for (size_t part : {l.best_level, l.second_dist, l.second_level, l.match}) overlaps += claim(ob, part * 4, NQ * 4);
        overlaps += claim(ob, l.nq * 4, (size_t)nkf * 4) + claim(ob, l.nmatches * 4, (size_t)nkf * 4);
    }
    printf("layouts: %d bytes claimed twice\n", overlaps);
    return bad || overlaps ? 1 : 0;
}
#endif
