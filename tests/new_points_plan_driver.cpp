// C entry points over csrc/new_points_plan.hpp for tests/test_new_points_cpu.py (built with g++ through tests/ref_build.py: the
// header has no HIP in it).  With -DNEW_POINTS_PLAN_MAIN the same source is a program that walks every layout and every chain step,
// for a run under AddressSanitizer and UBSan.  Test infrastructure only.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../orb_slam2_aruco_amd/csrc/new_points_plan.hpp"

using namespace orbfe;

extern "C" {

// out: NMP_THREADS, NMP_MAX_CAPACITY, NMP_MAX_LEVELS, NMP_SEARCH_LAUNCHES, NMP_INSPECT_FLOATS, sizeof pair record, sizeof result record
void nplan_constants(long long* out)
{
    const long long v[7] = {NMP_THREADS, NMP_MAX_CAPACITY, NMP_MAX_LEVELS, NMP_SEARCH_LAUNCHES, NMP_INSPECT_FLOATS,
                            (long long)sizeof(orbfe_new_points_pair), (long long)sizeof(orbfe_new_points_result)};
    memcpy(out, v, sizeof v);
}

// returns the error code; msg receives the message
int nplan_check_common(int capacity, int npairs, int have_pair1, int have_pair2, const float* K4, char* msg, int msg_len)
{
    static const int32_t dummy = 0;
    const NmpCheck c = nmp_check_common("call", capacity, npairs, have_pair1 ? &dummy : nullptr, have_pair2 ? &dummy : nullptr, K4);
    snprintf(msg, (size_t)msg_len, "%s", c.msg);
    return c.err;
}

int nplan_check_levels(const float* scale, const float* sigma2, int nlevels, float ratio_factor, char* msg, int msg_len)
{
    const NmpCheck c = nmp_check_levels("call", scale, sigma2, nlevels, ratio_factor);
    snprintf(msg, (size_t)msg_len, "%s", c.msg);
    return c.err;
}

// out: prepare x y block, triangulate x y block, chain launches
void nplan_geometry(int capacity, int npairs, long long* out)
{
    const NmpGrid p = nmp_prepare_grid(npairs), t = nmp_triangulate_grid(capacity, npairs);
    const long long v[7] = {p.x, p.y, p.block, t.x, t.y, t.block, nmp_chain_launches(npairs)};
    memcpy(out, v, sizeof v);
}

// out: pair, frame, index, per_feature, fv_offset, per_frame, tcw
void nplan_chain_step(int p, int have_index, int capacity, long long* out)
{
    const NmpChainStep s = nmp_chain_step(p, have_index != 0);
    const NmpFrameOffsets o = nmp_frame_offsets(s, capacity);
    const long long v[7] = {(long long)s.pair, (long long)s.frame, (long long)s.index, (long long)o.per_feature, (long long)o.fv_offset,
                            (long long)o.per_frame, (long long)o.tcw};
    memcpy(out, v, sizeof v);
}

// out: 23 offsets in declaration order, then split, down, end
void nplan_host_layout(int cap, int with_search, int with_inspect, long long* out)
{
    const NmpHostLayout l = nmp_host_layout(cap, with_search != 0, with_inspect != 0);
    const size_t v[26] = {l.kps, l.desc, l.n, l.fn, l.fo, l.ff, l.nf, l.tcw, l.x3Dw, l.valid, l.free_, l.F12, l.epipole, l.prep, l.m12, l.m21,
                          l.nm, l.status, l.x3D, l.normal, l.dist, l.res, l.inspect, l.io.split, l.io.down(), l.io.end()};
    for (int i = 0; i < 26; i++) out[i] = (long long)v[i];
}

} // extern "C"

#ifdef NEW_POINTS_PLAN_MAIN
// every array of every layout is written in a buffer of exactly end() bytes; every chain step addresses blocks inside the batch
int main()
{
    long checked = 0;
    for (int cap : {1, 2, 63, 64, 65, 255, 256, 257, 512, 1000, 4096})
        for (int search = 0; search < 2; search++)
            for (int inspect = 0; inspect < 2; inspect++) {
                const NmpHostLayout l = nmp_host_layout(cap, search != 0, inspect != 0);
                std::vector<unsigned char> buf(l.io.end());
                const size_t C = (size_t)cap, S = search ? C : 0;
                const size_t off[23] = {l.kps, l.desc, l.n, l.fn, l.fo, l.ff, l.nf, l.tcw, l.x3Dw, l.valid, l.free_, l.F12, l.epipole, l.prep, l.m12,
                                        l.m21, l.nm, l.status, l.x3D, l.normal, l.dist, l.res, l.inspect};
                const size_t len[23] = {2 * C * sizeof(orbfe_keypoint), 2 * S * 32, 8, 2 * S * 4, search ? 2 * (C + 1) * 4 : 0, 2 * S * 4, 8, 96,
                                        2 * C * 12, 2 * C, 2 * C, 36, 8, sizeof(orbfe_new_points_pair), C * 4, S * 4, 4, C, C * 12, C * 12, C * 8,
                                        sizeof(orbfe_new_points_result), inspect ? C * NMP_INSPECT_FLOATS * 4 : 0};
                for (int i = 0; i < 23; i++) {
                    if (off[i] % 256 != 0) { printf("unaligned array %d at capacity %d\n", i, cap); return 1; }
                    if (i && off[i] < off[i - 1] + len[i - 1]) { printf("overlap at array %d, capacity %d\n", i, cap); return 1; }
                    memset(buf.data() + off[i], i, len[i]);
                    checked++;
                }
                if (l.io.down() != l.x3Dw || l.io.split != l.F12) { printf("in-out range misplaced\n"); return 1; }
            }
    for (int cap : {1, 64, 512, 4096})
        for (int npairs : {1, 2, 6, 20})
            for (int have = 0; have < 2; have++) {
                const size_t frames = have ? 3 : (size_t)npairs + 1;
                std::vector<unsigned char> per_feature(frames * cap), fvo(frames * ((size_t)cap + 1)), per_pair((size_t)npairs * cap);
                for (int p = 0; p < npairs; p++) {
                    const NmpChainStep s = nmp_chain_step(p, have != 0);
                    const NmpFrameOffsets o = nmp_frame_offsets(s, cap);
                    // a batch of one pair reads frames 0 and 1 of the advanced blocks when there is no index array
                    const size_t last = have ? 0 : 1;
                    per_feature[o.per_feature + last * cap + cap - 1] = 1;
                    fvo[o.fv_offset + last * ((size_t)cap + 1) + cap] = 1;
                    per_pair[s.pair * cap + cap - 1] = 1;
                    checked++;
                }
                const NmpGrid g = nmp_triangulate_grid(cap, npairs);
                if ((long)g.x * g.block < cap || (long)(g.x - 1) * g.block >= cap || g.y != npairs) { printf("grid does not cover %d\n", cap); return 1; }
            }
    printf("new_points_plan: %ld checks ok\n", checked);
    return 0;
}
#endif
