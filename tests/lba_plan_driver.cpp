// C entry points over csrc/lba_plan.hpp and csrc/ba_camera.hpp for tests/test_lba_plan_cpu.py (built with g++ by
// tests/lba_plan_build.py: the headers have no HIP in them).  With -DLBA_PLAN_MAIN the same source is a program that writes every array
// of both layouts and runs the validation on arrays of exactly their lengths, for a run under AddressSanitizer and UBSan.  Test
// infrastructure only.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../orb_slam2_aruco_amd/csrc/lba_plan.hpp"

using namespace orbfe;

namespace {

LbaSizes sizes_of(const int* n) { return LbaSizes{n[0], n[1], n[2], n[3], n[4]}; }

int give(const BaCheck& c, char* msg, int msg_len)
{
    if (msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "%s", c.msg);
    return c.err;
}

constexpr int N_SCRATCH = 37, N_IO = 14;

void scratch_offsets(const LbaLayout& l, size_t* o)
{
    const size_t v[N_SCRATCH] = {l.ctl, l.xv, l.xl, l.e_chi2, l.m_chi2, l.e_level, l.m_level, l.pose[0], l.pose[1], l.pt[0], l.pt[1], l.e_kf, l.e_pt,
                                 l.e_ox, l.e_oy, l.e_info, l.e_use, l.e_blk, l.mo_marker, l.m_use, l.m_blk, l.Hll, l.bl, l.Dinv, l.p_active, l.Hpp,
                                 l.bp, l.vmax, l.v_active, l.v_kf, l.kf_free, l.tbl, l.S, l.bs, l.chi_part, l.scale_part, l.max_part};
    memcpy(o, v, sizeof v);
}

// what the kernels of local_ba.hip index in each array, in bytes, in the order of scratch_offsets: the test's own statement
void scratch_lengths(const LbaSizes& n, size_t* o)
{
    const size_t K = (size_t)std::max(n.nkf, 1), P = (size_t)std::max(n.np, 1), E = (size_t)std::max(n.nobs, 1), M = (size_t)std::max(n.nma, 1),
                 MO = (size_t)std::max(n.nmobs, 1), ME = 4 * MO, NB = (size_t)std::max((n.np + 63) / 64 + (4 * n.nmobs + 63) / 64, 1);
    const size_t v[N_SCRATCH] = {sizeof(LbaCtl), 384 * 8, P * 24, E * 8, ME * 8, E, ME, (K + M) * 64, (K + M) * 64, P * 24, P * 24, E * 4, E * 4,
                                 E * 4, E * 4, E * 4, E, E * 45 * 8, MO * 4, ME, ME * 90 * 8, P * 48, P * 24, P * 72, P, 64 * 36 * 8,
                                 384 * 8, 64 * 8, 64 * 4, 64 * 4, K * 4, K * P * 4, (size_t)384 * 384 * 8, 384 * 8, NB * 8, NB * 8, NB * 8};
    memcpy(o, v, sizeof v);
}

void io_offsets(const LbaHostIo& l, size_t* o)
{
    const size_t v[N_IO] = {l.fixed, l.off, l.kf, l.xy, l.oct, l.mloc, l.moff, l.mkf, l.mcor, l.T, l.X, l.M, l.erase, l.res};
    memcpy(o, v, sizeof v);
}

// what lba_stage copies into, or a kernel writes, in each array of the staging block
void io_lengths(const LbaSizes& n, size_t* o)
{
    const size_t K = (size_t)std::max(n.nkf, 1), P = (size_t)std::max(n.np, 1), E = (size_t)std::max(n.nobs, 1), M = (size_t)std::max(n.nma, 1),
                 MO = (size_t)std::max(n.nmobs, 1);
    const size_t v[N_IO] = {K, (P + 1) * 4, E * 4, E * 8, E * 4, M * 48, (M + 1) * 4, MO * 4, MO * 32, K * 48, P * 12, M * 48, E, sizeof(orbfe_lba_result)};
    memcpy(o, v, sizeof v);
}

} // namespace

extern "C" {

// out: LBA_MAXV, LBA_N, LBA_PT, LBA_MAX_LEVELS, LBA_EBLK, LBA_MBLK, LBA_SE3_BYTES, LBA_SOLVE_LDS, sizeof LbaCtl, sizeof the record
void lplan_constants(long long* out)
{
    const long long v[10] = {LBA_MAXV, LBA_N, LBA_PT, LBA_MAX_LEVELS, LBA_EBLK, LBA_MBLK, (long long)LBA_SE3_BYTES, (long long)LBA_SOLVE_LDS,
                             (long long)sizeof(LbaCtl), (long long)sizeof(orbfe_lba_result)};
    memcpy(out, v, sizeof v);
}

int lplan_sizes_ok(const int* n) { return lba_sizes_ok(sizes_of(n)); }

// the host calls' checks; returns the error code, msg receives the message
int lplan_check_host(const int* n, float* Tcw, const uint8_t* kf_fixed, float* x3Dw, const int32_t* obs_offset, const int32_t* obs_kf, const float* obs_xy,
                     const int32_t* obs_octave, float* Twm, const float* marker_local, const int32_t* mobs_offset, const int32_t* mobs_kf,
                     const float* mobs_corners, int nlevels, int use_markers, char* msg, int msg_len)
{
    const LbaProblem pb{sizes_of(n), Tcw, kf_fixed, x3Dw, obs_offset, obs_kf, obs_xy, obs_octave, nullptr, nullptr, 0,
                        Twm, marker_local, mobs_offset, mobs_kf, mobs_corners};
    return give(lba_check_host(pb, nlevels, use_markers, "call"), msg, msg_len);
}

// The device call's checks in its order: the arguments, then the scratch size.  a: 17 addresses, never read -- Tcw, kf_fixed, x3Dw,
// obs_offset, obs_kf, obs_xy, obs_octave, obs_feature, kps, Twm, marker_local, mobs_offset, mobs_kf, mobs_corners, erase, res, scratch
int lplan_check_device(const int* n, const unsigned long long* a, int capacity, unsigned long long scratch_bytes, char* msg, int msg_len)
{
    auto at = [&](int i) { return (uintptr_t)a[i]; };
    const LbaProblem d{sizes_of(n), (float*)at(0), (const uint8_t*)at(1), (float*)at(2), (const int32_t*)at(3), (const int32_t*)at(4),
                       (const float*)at(5), (const int32_t*)at(6), (const int32_t*)at(7), (const orbfe_keypoint*)at(8), capacity,
                       (float*)at(9), (const float*)at(10), (const int32_t*)at(11), (const int32_t*)at(12), (const float*)at(13)};
    const BaCheck c = lba_check_device(d, (const void*)at(14), (const void*)at(15), (const void*)at(16), "call");
    return give(c.err ? c : lba_check_scratch(d.n, (size_t)scratch_bytes, "call"), msg, msg_len);
}

// out: the 37 offsets in declaration order, then zero_end, tbl_bytes, end;  len: this driver's lengths of the 37 arrays
void lplan_scratch(const int* n, long long* out, long long* len)
{
    LbaLayout l;
    const LbaExtent x = lba_scratch(l, sizes_of(n));
    size_t o[N_SCRATCH], b[N_SCRATCH];
    scratch_offsets(l, o);
    scratch_lengths(sizes_of(n), b);
    for (int i = 0; i < N_SCRATCH; i++) { out[i] = (long long)o[i]; len[i] = (long long)b[i]; }
    out[N_SCRATCH] = (long long)x.zero_end; out[N_SCRATCH + 1] = (long long)x.tbl_bytes; out[N_SCRATCH + 2] = (long long)x.end;
}

unsigned long long lplan_scratch_bytes(const int* n) { return lba_scratch_bytes(sizes_of(n)); }

// out: the 14 offsets in declaration order, then split, down, end;  len: this driver's lengths
void lplan_host_io(const int* n, long long* out, long long* len)
{
    const LbaHostIo l = lba_host_io(sizes_of(n));
    size_t o[N_IO], b[N_IO];
    io_offsets(l, o);
    io_lengths(sizes_of(n), b);
    for (int i = 0; i < N_IO; i++) { out[i] = (long long)o[i]; len[i] = (long long)b[i]; }
    out[N_IO] = (long long)l.io.split; out[N_IO + 1] = (long long)l.io.down(); out[N_IO + 2] = (long long)l.io.end();
}

// out: npb, nb, g_setup, g_pass, g_points, g_edges, vmax, lds_rows, tri_bytes, rounds, maxit[0], maxit[1], trials, launches
void lplan_schedule(const int* n, int use_markers, int inspect, unsigned long long lds_limit, long long* out)
{
    const LbaSchedule s = lba_schedule(sizes_of(n), use_markers != 0, inspect != 0, (size_t)lds_limit);
    const long long v[14] = {s.npb, s.nb, s.g_setup, s.g_pass, s.g_points, s.g_edges, s.vmax, s.lds_rows, (long long)s.tri_bytes, s.rounds,
                             s.maxit[0], s.maxit[1], s.trials, s.launches};
    memcpy(out, v, sizeof v);
}

// the step pose_optimizer.hip and local_ba.hip share.  out: fx, fy, cx, cy, marker_info, then the 32 table entries
int lplan_camera(const char* name, const float* K4, const float* inv_sigma2, int nlevels, float marker_info, float* out, double* delta, int* nlevels_out,
                 char* msg, int msg_len)
{
    BaCamera c{};
    const BaCheck chk = ba_camera(c, K4, inv_sigma2, nlevels, marker_info, name);
    const float v[5] = {c.fx, c.fy, c.cx, c.cy, c.marker_info};
    memcpy(out, v, sizeof v);
    memcpy(out + 5, c.inv_sigma2, sizeof c.inv_sigma2);
    *delta = c.delta;
    *nlevels_out = c.nlevels;
    return give(chk, msg, msg_len);
}

} // extern "C"

#ifdef LBA_PLAN_MAIN
#include <limits>

namespace {

long checked = 0;

// a problem whose arrays are allocated at exactly their lengths: a check that reads one entry too many is the sanitizer's
struct Pb {
    std::vector<float> Tcw, x3Dw, obs_xy, Twm, mlocal, mcorners;
    std::vector<uint8_t> fixed;
    std::vector<int32_t> off, kf, oct, moff, mkf;
    int nlevels = 2, use_markers = 1;
    LbaSizes n() const
    {
        return LbaSizes{(int)fixed.size(), (int)x3Dw.size() / 3, (int)kf.size(), (int)Twm.size() / 12, (int)mkf.size()};
    }
};

template <class T> T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

// nkf keyframes (the first fixed), the points' observation counts, markers with their observation counts
Pb make(int nkf, std::vector<int> per_point, std::vector<int> per_marker)
{
    Pb p;
    p.Tcw.assign((size_t)nkf * 12, 0.5f);
    p.fixed.assign((size_t)nkf, 0);
    if (nkf) p.fixed[0] = 1;
    p.x3Dw.assign(per_point.size() * 3, 1.f);
    if (!per_point.empty()) p.off.push_back(0);
    for (int c : per_point) {
        for (int k = 0; k < c; k++) { p.kf.push_back(k % std::max(nkf, 1)); p.oct.push_back(k % 2); }
        p.off.push_back((int32_t)p.kf.size());
    }
    p.obs_xy.assign(p.kf.size() * 2, 10.f);
    p.Twm.assign(per_marker.size() * 12, 0.25f);
    p.mlocal.assign(per_marker.size() * 12, 0.1f);
    if (!per_marker.empty()) p.moff.push_back(0);
    for (int c : per_marker) {
        for (int k = 0; k < c; k++) p.mkf.push_back(k % std::max(nkf, 1));
        p.moff.push_back((int32_t)p.mkf.size());
    }
    p.mcorners.assign(p.mkf.size() * 8, 20.f);
    return p;
}

BaCheck run(Pb& p, const LbaSizes* sizes = nullptr)
{
    const LbaProblem pb{sizes ? *sizes : p.n(), ptr(p.Tcw), ptr(p.fixed), ptr(p.x3Dw), ptr(p.off), ptr(p.kf), ptr(p.obs_xy), ptr(p.oct), nullptr, nullptr, 0,
                        ptr(p.Twm), ptr(p.mlocal), ptr(p.moff), ptr(p.mkf), ptr(p.mcorners)};
    return lba_check_host(pb, p.nlevels, p.use_markers, "call");
}

bool expect(const char* what, const BaCheck& c, int err, const char* text)
{
    checked++;
    if (c.err == err && strstr(c.msg, text)) return true;
    printf("%s: code %d \"%s\", expected %d with \"%s\"\n", what, c.err, c.msg, err, text);
    return false;
}

// every array of a layout written at its length in a buffer of exactly `end` bytes
bool write_all(const char* what, const size_t* off, const size_t* len, int count, size_t end)
{
    std::vector<unsigned char> buf(end);
    for (int i = 0; i < count; i++) {
        if (off[i] % 256 != 0 || (i && off[i] < off[i - 1] + len[i - 1])) { printf("%s: array %d misplaced\n", what, i); return false; }
        memset(buf.data() + off[i], i + 1, len[i]);
        checked++;
    }
    return true;
}

} // namespace

int main()
{
    bool ok = true;
    static const int SIZES[][5] = {{0, 0, 0, 0, 0}, {1, 1, 1, 0, 0}, {3, 40, 80, 1, 3}, {3, 257, 514, 0, 0}, {64, 70, 4480, 0, 0}, {256, 12, 3072, 0, 0},
                                   {40, 3000, 42000, 2, 5}};
    for (const auto& t : SIZES) {
        const LbaSizes n = sizes_of(t);
        size_t off[N_SCRATCH], len[N_SCRATCH];
        LbaLayout l;
        const LbaExtent x = lba_scratch(l, n);
        scratch_offsets(l, off);
        scratch_lengths(n, len);
        ok = ok && write_all("scratch", off, len, N_SCRATCH, x.end);
        // the same list gives the kernels' pointers: each at its offset of the base
        struct { unsigned char *ctl, *xv, *xl, *e_chi2, *m_chi2, *e_level, *m_level, *pose[2], *pt[2], *e_kf, *e_pt, *e_ox, *e_oy, *e_info, *e_use, *e_blk,
                     *mo_marker, *m_use, *m_blk, *Hll, *bl, *Dinv, *p_active, *Hpp, *bp, *vmax, *v_active, *v_kf, *kf_free, *tbl, *S, *bs, *chi_part,
                     *scale_part, *max_part; } p;
        std::vector<unsigned char> base(x.end);
        lba_scratch(p, n, base.data());
        if (p.ctl != base.data() || p.pose[1] != base.data() + l.pose[1] || p.tbl != base.data() + l.tbl ||
            p.max_part != base.data() + l.max_part) { printf("pointers and offsets disagree\n"); ok = false; }
        checked++;
        const LbaHostIo io = lba_host_io(n);
        size_t ioff[N_IO], ilen[N_IO];
        io_offsets(io, ioff);
        io_lengths(n, ilen);
        ok = ok && write_all("staging", ioff, ilen, N_IO, io.io.end());
        if (io.io.down() != io.T || io.io.split != io.erase) { printf("in-out range misplaced\n"); ok = false; }
    }

    const float nan = std::numeric_limits<float>::quiet_NaN();
    const int INV = ORBFE_ERR_INVALID, CAP = ORBFE_ERR_CAPACITY;
    // 2 keyframes, 2 points with 2 and 1 observations, 1 marker with 1 observation
    auto base = [] { return make(2, {2, 1}, {1}); };
    { Pb p = base(); ok &= expect("valid", run(p), ORBFE_OK, ""); }
    { Pb p = base(); LbaSizes n = p.n(); n.nkf = -1; ok &= expect("negative size", run(p, &n), INV, "invalid argument"); }
    // each array absent while its size says it is there
    { Pb p = base(); LbaSizes n = p.n(); p.Tcw.clear(); ok &= expect("no Tcw", run(p, &n), INV, "invalid argument"); }
    { Pb p = base(); LbaSizes n = p.n(); p.fixed.clear(); ok &= expect("no kf_fixed", run(p, &n), INV, "invalid argument"); }
    { Pb p = base(); LbaSizes n = p.n(); p.x3Dw.clear(); ok &= expect("no x3Dw", run(p, &n), INV, "invalid argument"); }
    { Pb p = base(); LbaSizes n = p.n(); p.off.clear(); ok &= expect("no obs_offset", run(p, &n), INV, "invalid argument"); }
    { Pb p = base(); LbaSizes n = p.n(); p.kf.clear(); ok &= expect("no obs_kf", run(p, &n), INV, "invalid argument"); }
    { Pb p = base(); LbaSizes n = p.n(); p.obs_xy.clear(); ok &= expect("no obs_xy", run(p, &n), INV, "invalid argument"); }
    { Pb p = base(); LbaSizes n = p.n(); p.oct.clear(); ok &= expect("no obs_octave", run(p, &n), INV, "invalid argument"); }
    { Pb p = base(); LbaSizes n = p.n(); n.np = 0; ok &= expect("observations without points", run(p, &n), INV, "invalid argument"); }
    { Pb p = base(); LbaSizes n = p.n(); p.Twm.clear(); ok &= expect("no Twm", run(p, &n), INV, "invalid argument"); }
    { Pb p = base(); LbaSizes n = p.n(); p.mlocal.clear(); ok &= expect("no marker_local", run(p, &n), INV, "invalid argument"); }
    { Pb p = base(); LbaSizes n = p.n(); p.moff.clear(); ok &= expect("no mobs_offset", run(p, &n), INV, "invalid argument"); }
    { Pb p = base(); LbaSizes n = p.n(); p.mkf.clear(); ok &= expect("no mobs_kf", run(p, &n), INV, "invalid argument"); }
    { Pb p = base(); LbaSizes n = p.n(); p.mcorners.clear(); ok &= expect("no mobs_corners", run(p, &n), INV, "invalid argument"); }
    { Pb p = base(); LbaSizes n = p.n(); n.nma = 0; ok &= expect("marker observations without markers", run(p, &n), INV, "invalid argument"); }
    // a non-finite value in the last entry of each of the six float arrays
    { Pb p = base(); p.Tcw.back() = nan; ok &= expect("Tcw", run(p), INV, "not finite"); }
    { Pb p = base(); p.x3Dw.back() = nan; ok &= expect("x3Dw", run(p), INV, "not finite"); }
    { Pb p = base(); p.obs_xy.back() = nan; ok &= expect("obs_xy", run(p), INV, "not finite"); }
    { Pb p = base(); p.Twm.back() = nan; ok &= expect("Twm", run(p), INV, "not finite"); }
    { Pb p = base(); p.mlocal.back() = nan; ok &= expect("marker_local", run(p), INV, "not finite"); }
    { Pb p = base(); p.mcorners.back() = nan; ok &= expect("mobs_corners", run(p), INV, "not finite"); }
    // the offset tables
    { Pb p = base(); p.off = {1, 2, 3}; ok &= expect("obs_offset[0]", run(p), INV, "obs_offset does not span"); }
    { Pb p = base(); p.off = {0, 2, 2}; ok &= expect("obs_offset[np]", run(p), INV, "obs_offset does not span"); }
    { Pb p = base(); p.off = {0, 4, 3}; ok &= expect("obs_offset decreases", run(p), INV, "obs_offset decreases at point 1"); }
    { Pb p = base(); p.moff = {1, 1}; ok &= expect("mobs_offset[0]", run(p), INV, "mobs_offset does not span"); }
    { Pb p = base(); p.moff = {0, 2}; ok &= expect("mobs_offset[nma]", run(p), INV, "mobs_offset does not span"); }
    { Pb p = make(2, {2, 1}, {1, 0}); p.moff = {0, 2, 1}; ok &= expect("mobs_offset decreases", run(p), INV, "mobs_offset decreases at marker 1"); }
    // indices
    { Pb p = base(); p.kf.back() = 2; ok &= expect("keyframe 2 of 2", run(p), INV, "observation 2 names keyframe 2 of 2"); }
    { Pb p = base(); p.kf[0] = -1; ok &= expect("keyframe -1", run(p), INV, "observation 0 names keyframe -1"); }
    { Pb p = base(); p.oct.back() = 2; ok &= expect("octave 2 of 2", run(p), INV, "octave 2"); }
    { Pb p = base(); p.oct[0] = -1; ok &= expect("octave -1", run(p), INV, "octave -1"); }
    { Pb p = base(); p.mkf.back() = 2; ok &= expect("marker keyframe", run(p), INV, "marker observation 0 names keyframe 2 of 2"); }
    { Pb p = base(); p.kf = {1, 1, 0}; ok &= expect("twice", run(p), INV, "keyframe 1 observes point 0 twice"); }
    // the bounds
    { Pb p = make(64, {}, {0}); p.fixed[0] = 0; ok &= expect("65 free", run(p), CAP, "ORBFE_LBA_MAX_FREE_POSES"); }
    { Pb p = make(64, {}, {0}); p.fixed[0] = 0; p.use_markers = 0; ok &= expect("64 free, marker unused", run(p), ORBFE_OK, ""); }
    { Pb p = make(257, {257}, {}); p.fixed.assign(257, 1); ok &= expect("257 observations", run(p), CAP, "ORBFE_LBA_MAX_OBSERVATIONS"); }
    { Pb p = make(256, {256}, {}); p.fixed.assign(256, 1); ok &= expect("256 observations", run(p), ORBFE_OK, ""); }
    { Pb p = make(0, {}, {}); ok &= expect("empty", run(p), ORBFE_OK, ""); }

    // the camera step on arrays of exactly 4 and nlevels entries
    {
        std::vector<float> K{500.f, 500.f, 320.f, 240.f}, sig{1.f, 0.5f};
        BaCamera c{};
        ok &= expect("camera", ba_camera(c, K.data(), sig.data(), 2, 25.f, "call"), ORBFE_OK, "");
        if (c.inv_sigma2[1] != 0.5f || c.inv_sigma2[2] != 0.f || c.inv_sigma2[31] != 0.f || c.nlevels != 2) { printf("sigma table not padded\n"); ok = false; }
        std::vector<float> sig32(32, 1.f);
        ok &= expect("32 levels", ba_camera(c, K.data(), sig32.data(), 32, 25.f, "call"), ORBFE_OK, "");
        ok &= expect("33 levels", ba_camera(c, K.data(), sig32.data(), 33, 25.f, "call"), INV, "invalid K4 / sigma table");
        K[3] = nan;
        ok &= expect("K", ba_camera(c, K.data(), sig.data(), 2, 25.f, "call"), INV, "K is not finite");
    }
    if (!ok) return 1;
    printf("lba_plan: %ld checks ok\n", checked);
    return 0;
}
#endif
