// orb_extractor.hip -- host side of the ORB extractor behind the C ABI (include/orbfe.h).
//
// Mirrors ORB_SLAM2::ORBextractor (include/ORBextractor.h:45-113): the constructor builds the same tables
// (src/ORBextractor.cc:410-470) with the same float/double arithmetic, operator() becomes orbfe_extract*(), and
// the image work runs as the gfx950 kernels of orb_kernels.hip on a batch of frames.  There is no CPU path: if
// no HIP device is usable every entry point fails with ORBFE_ERR_NO_DEVICE.
#include <algorithm>
#include <cmath>

#include "orb_kernels.hpp"
#include <map>
#include <mutex>

#include "orbfe_common.hpp"
#include "orbfe_tables.inc"

namespace orbfe {

thread_local char g_err[512] = "";

int use_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(ORBFE_ERR_NO_DEVICE, "no usable HIP device (%s); liborbfe has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(ORBFE_ERR_INVALID, "device %d out of range (have %d)", device, n);
    ORBFE_HIP(hipSetDevice(device));
    return ORBFE_OK;
}

int ensure_dyn_lds(const void* fn, size_t bytes)
{
    // per device: the attribute belongs to the function object of the current device's code object
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> done;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    size_t& have = done[std::make_pair(dev, fn)];
    if (have >= bytes && have != 0) return ORBFE_OK;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError(); // do not leave the error for the next call to trip over
        return fail(ORBFE_ERR_CAPACITY, "a kernel needs %zu bytes of dynamic LDS (plus its static LDS): more than a workgroup can have (%s)",
                    bytes, hipGetErrorString(e));
    }
    have = bytes;
    return ORBFE_OK;
}

static inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

} // namespace orbfe

using namespace orbfe;

struct orbfe_extractor {
    // --- reference members (ORBextractor.h:92-112)
    int nfeatures, nlevels, iniThFAST, minThFAST;
    double scaleFactor;
    std::vector<float> mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2;
    std::vector<int> mnFeaturesPerLevel, umax;
    // --- device state
    int device = 0;
    hipStream_t own_stream = nullptr, aux_stream = nullptr;
    PinnedBuf pinned;               // staging of the host-pointer entry points
    orbfe_aruco* paired = nullptr;  // orbfe_extractor_pair_detector
    hipEvent_t ev_up = nullptr;     // the image of the host-pointer call is on the device
    hipStream_t user_aux = nullptr; // orbfe_extractor_set_aux_stream: run the blur there instead of on aux_stream
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // orbfe_extractor_follow: this handle's batches start behind a stage of ANOTHER handle's latest batch (two engine sets of a
    // pipeline hold a fixed phase that way instead of whatever the contention of the moment settles on)
    orbfe_extractor* follow = nullptr;
    int follow_stage = 0;                // 1 = the other's FAST, 2 = its quadtree, 3 = its descriptors (the whole batch), 4 = its resize chain
    int follow_fast_stage = 0;           // a second gate in front of this handle's FAST (0 = none): the resize chain may run earlier
    hipEvent_t ev_stage[4] = {nullptr, nullptr, nullptr, nullptr};   // after FAST, the quadtree, the descriptors; [3] = after the resize chain (FAST starts)
    bool stage_recorded = false;         // a batch's front part has been enqueued.  A stage's event is created when the stage is first
                                         // enqueued -- the descriptors may come a step later (extractor_defer_describe) -- and a wait skips
                                         // an event that does not exist yet
    // queue on `st` a wait for stage k (1 .. 4 as in follow_stage; 0 = no gate) of h's newest batch.  No wait when h is null or is
    // `self` (a handle is not gated by itself), nor before h's front part has been enqueued once.
    static int wait_stage(const orbfe_extractor* h, int k, hipStream_t st, const orbfe_extractor* self = nullptr)
    {
        if (h && h != self && h->stage_recorded && k >= 1 && k <= 4 && h->ev_stage[k - 1]) ORBFE_HIP(hipStreamWaitEvent(st, h->ev_stage[k - 1], 0));
        return ORBFE_OK;
    }
    int rows = 0, cols = 0; // geometry currently built
    int batch_cap = 0;
    std::vector<LevelGeom> geom;
    int ncells_total = 0, ntiles = 0, out_total = 0, max_out_cap = 0, max_wcell = 0, max_hcell = 0;
    size_t pyr_fbytes = 0, blur_fbytes = 0, slots_fu32 = 0, keys_fu32 = 0;
    int keycap_lds = 0, nodecap = 0, veccap = 0;
    std::vector<char> resize_tab_ok; // per level >= 1: k_resize_tab's 8-byte windows fit
    std::vector<size_t> tab_off; // per level >= 1: offsets (in ints) of xofs, xalpha, yofs, ybeta in d_tabs
    DevBuf d_geom, d_cellinfo, d_tiles, d_tabs, d_pattern, d_umax;
    DevBuf d_pyr, d_blur, d_slots, d_cellcnt, d_keys, d_lvlout, d_lvlcnt, d_lvloff, d_lvlncand, d_overflow, d_fallback,
        d_flatkv, d_flatlvl, d_worklist;
    bool gaussian_ed = false;            // orbfe_extractor_set_gaussian_taps: 18 34 48 56 48 34 18 instead of 18 34 49 55 49 34 18
    // workgroups per CU the VALU-bound kernels may occupy (0 = what the hardware allows): the launch asks for LDS it does not use
    // so that the other engine's latency-bound kernels (8 waves and 50-77 KB of LDS per workgroup) always find room on every CU
    // k_orient_describe2 (two keypoints per wave: 227 instead of 342 VALU instructions per keypoint, 238 instead of 256 us alone at C2)
    // is NOT the default: with the detector running the C2 step was 1.62 ms with it and 1.61 without (four interleaved runs each)
    // (rounds 2 - 3 capped the VALU-bound kernels' workgroups per CU with an LDS request they did not use -- ORBFE_OCC_FAST / _BLUR /
    // _ORIENT -- so that the detector's 65 - 77 KB workgroups always found room: noise at best, slower when tighter; the switches went in round 5)
    bool force_general_quadtree = false; // test hook: run the general kernel for every level
    int force_pyramid_depth = 0;         // test hook: shallow count pyramid so that levels fall back
    DevBuf d_in, d_kps, d_desc, d_nout; // staging for the host-pointer entry points
    KernelTimer timer;
    int last_nframes = 0;
    ImgView last_src0{};

    ~orbfe_extractor()
    {
        for (DevBuf* b : {&d_geom, &d_cellinfo, &d_tiles, &d_tabs, &d_pattern, &d_umax, &d_bstrips, &d_btabs, &d_btab2, &d_pyr, &d_blur, &d_slots,
                          &d_cellcnt, &d_keys, &d_lvlout, &d_lvlcnt, &d_lvloff, &d_lvlncand, &d_overflow, &d_fallback, &d_flatkv,
                          &d_flatlvl, &d_worklist, &d_in,
                          &d_kps, &d_desc, &d_nout})
            b->release();
        if (own_stream) (void)hipStreamDestroy(own_stream);
        if (aux_stream) (void)hipStreamDestroy(aux_stream);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (ev_up) (void)hipEventDestroy(ev_up);
        for (hipEvent_t e : ev_stage) if (e) (void)hipEventDestroy(e);
    }

    // ORBextractor::ORBextractor, src/ORBextractor.cc:410-470
    void build_tables()
    {
        mvScaleFactor.resize(nlevels);
        mvLevelSigma2.resize(nlevels);
        mvScaleFactor[0] = 1.0f;
        mvLevelSigma2[0] = 1.0f;
        for (int i = 1; i < nlevels; i++) {
            mvScaleFactor[i] = (float)(mvScaleFactor[i - 1] * scaleFactor);
            mvLevelSigma2[i] = mvScaleFactor[i] * mvScaleFactor[i];
        }
        mvInvScaleFactor.resize(nlevels);
        mvInvLevelSigma2.resize(nlevels);
        for (int i = 0; i < nlevels; i++) {
            mvInvScaleFactor[i] = 1.0f / mvScaleFactor[i];
            mvInvLevelSigma2[i] = 1.0f / mvLevelSigma2[i];
        }
        mnFeaturesPerLevel.resize(nlevels);
        float factor = (float)(1.0f / scaleFactor);
        float nDesired = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nlevels));
        int sum = 0;
        for (int level = 0; level < nlevels - 1; level++) {
            mnFeaturesPerLevel[level] = orbfe_round_f(nDesired);
            sum += mnFeaturesPerLevel[level];
            nDesired *= factor;
        }
        mnFeaturesPerLevel[nlevels - 1] = std::max(nfeatures - sum, 0);
        const int HP = 15;
        umax.assign(HP + 1, 0);
        int v, v0, vmax = orbfe_floor_d(HP * std::sqrt(2.f) / 2 + 1);
        int vmin = orbfe_ceil_d(HP * std::sqrt(2.f) / 2);
        const double hp2 = HP * HP;
        for (v = 0; v <= vmax; ++v) umax[v] = orbfe_round_d(std::sqrt(hp2 - v * v));
        for (v = HP, v0 = 0; v >= vmin; --v) {
            while (umax[v0] == umax[v0 + 1]) ++v0;
            umax[v] = v0;
            ++v0;
        }
    }

    // Tables of k_orient_describe: the 256 rBRIEF tests (x0, y0, x1, y1 as int8 -- the pattern copied at ORBextractor.cc:448-450),
    // and per row v = -15 .. 15 of the r = 15 patch of IC_Angle the weights of its 32 bytes: byte index i = u + 15 inside
    // |u| <= umax[|v|] (:454-469), and ones for the same bytes (d_umax keeps its name: it holds umax in this form).
    int upload_describe_tables()
    {
        std::vector<uint32_t> w(31 * 16, 0u);
        for (int row = 0; row < 31; row++) {
            const int um = umax[row < 15 ? 15 - row : row - 15];
            for (int i = 0; i <= 30; i++) {
                const int u = i - 15;
                if (u < -um || u > um) continue;
                w[row * 16 + i / 4] |= (uint32_t)i << (8 * (i & 3));
                w[row * 16 + 8 + i / 4] |= 1u << (8 * (i & 3));
            }
        }
        int rc;
        if ((rc = d_pattern.ensure(1024)) || (rc = d_umax.ensure(w.size() * 4))) return rc;
        ORBFE_HIP(hipMemcpy(d_pattern.p, ORBFE_BIT_PATTERN_31, 1024, hipMemcpyHostToDevice));
        ORBFE_HIP(hipMemcpy(d_umax.p, w.data(), w.size() * 4, hipMemcpyHostToDevice));
        return ORBFE_OK;
    }

    int max_keypoints() const
    {
        int t = 0;
        for (int l = 0; l < nlevels; l++) t += mnFeaturesPerLevel[l] + 3;
        return t + 8;
    }

    // Level geometry for a rows x cols input: pyramid sizes (:1112), cell grid (:767-787), quadtree roots (:543-558),
    // plus the HBM layout of every per-frame block.
    int build_geometry(int rows_, int cols_)
    {
        if (rows_ == rows && cols_ == cols && !geom.empty()) return ORBFE_OK;
        geom.assign(nlevels, LevelGeom{});
        std::vector<uint32_t> cellinfo, tiles;
        std::vector<int> tabs;
        tab_off.assign((size_t)nlevels * 4, 0);
        resize_tab_ok.assign((size_t)nlevels, 0);
        size_t pyr = 0, blur = 0, slots = 0, cand = 0;
        int out = 0, maxcap = 0, mwc = 0, mhc = 0;
        for (int l = 0; l < nlevels; l++) {
            LevelGeom& g = geom[l];
            const float scale = mvInvScaleFactor[l];
            g.w = orbfe_round_f((float)cols_ * scale);
            g.h = orbfe_round_f((float)rows_ * scale);
            // the reference's own limit: its cell grid needs nCols = (w - 32) / 30 >= 1 (ORBextractor.cc:780-784; below that it divides by zero)
            if (g.w < 32 + 30 || g.h < 32 + 30)
                return fail(ORBFE_ERR_INVALID, "level %d is %dx%d: too small for a FAST cell grid (62 pixels a side)", l, g.w, g.h);
            // a keypoint travels as x | y << 12 | score << 24 relative to the 16-px border
            if (g.w - 32 > 4095 || g.h - 32 > 4095)
                return fail(ORBFE_ERR_INVALID, "level %d is %dx%d: images above 4127 px a side are unsupported", l, g.w, g.h);
            g.pitch = align_up(g.w, 64);
            g.bpitch = align_up(g.w, 64);
            g.img_off = (long long)pyr;
            if (l > 0) pyr += (size_t)g.pitch * g.h;
            g.blur_off = (long long)blur;
            blur += (size_t)g.bpitch * g.h;
            g.maxBX = g.w - 19 + 3;
            g.maxBY = g.h - 19 + 3;
            const float width = (float)(g.maxBX - 16), height = (float)(g.maxBY - 16);
            g.nCols = (int)(width / 30.f);
            g.nRows = (int)(height / 30.f);
            g.wCell = (int)std::ceil(width / g.nCols);
            g.hCell = (int)std::ceil(height / g.nRows);
            if (g.wCell > 60 || g.hCell > 60) return fail(ORBFE_ERR_INVALID, "cell larger than 60 px");
            mwc = std::max(mwc, g.wCell); mhc = std::max(mhc, g.hCell);
            g.cell_first = (int)cellinfo.size();
            for (int i = 0; i < g.nRows; i++) {
                const float iniY = (float)(16 + i * g.hCell);
                if (iniY >= g.maxBY - 3) continue;
                for (int j = 0; j < g.nCols; j++) {
                    const float iniX = (float)(16 + j * g.wCell);
                    if (iniX >= g.maxBX - 6) continue;
                    cellinfo.push_back((uint32_t)l | ((uint32_t)i << 4) | ((uint32_t)j << 14));
                }
            }
            g.ncells = (int)cellinfo.size() - g.cell_first;
            g.cell_cap = ((g.wCell + 1) / 2) * ((g.hCell + 1) / 2);
            g.slot_off = (long long)slots;
            g.cand_cap = g.ncells * g.cell_cap;
            slots += (size_t)g.cand_cap;
            g.cand_off = (long long)cand;
            cand += (size_t)g.cand_cap;
            g.quota = mnFeaturesPerLevel[l];
            g.nIni = (int)std::round(static_cast<float>(g.maxBX - 16) / (g.maxBY - 16));
            if (g.nIni < 1 || g.nIni > QT_MAXROOTS)
                return fail(ORBFE_ERR_INVALID, "aspect ratio gives %d quadtree roots (supported: 1..%d)", g.nIni, QT_MAXROOTS);
            g.hX = static_cast<float>(g.maxBX - 16) / g.nIni;
            g.out_cap = std::max(g.quota + 3, 4 * g.nIni) + 5;
            g.out_off = out;
            out += g.out_cap;
            maxcap = std::max(maxcap, g.out_cap);
            g.scale = mvScaleFactor[l];
            g.kp_size = (float)(int)(31 * mvScaleFactor[l]);
            for (int tx = 0; tx < (g.w + 63) / 64; tx++) // k_blur7: one workgroup per 64-column strip, long strips first
                tiles.push_back((uint32_t)l | ((uint32_t)tx << 4));
            if (l > 0) {
                // cv::resize(INTER_LINEAR) coefficient tables, OpenCV 3.4
                const int sw = geom[l - 1].w, sh = geom[l - 1].h, dw = g.w, dh = g.h;
                const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
                const int dwp = align_up(dw, 4);
                std::vector<int> xofs(dwp), xal(dwp), ytab((size_t)dh * 4);   // ytab: per row {source row, the row below (both clipped), b0 << 12, b1 << 12}
                for (int dx = 0; dx < dw; dx++) {
                    float fx = (float)((dx + 0.5) * scale_x - 0.5);
                    int sx = orbfe_floor_d(fx);
                    fx -= sx;
                    if (sx < 0) { fx = 0; sx = 0; }
                    if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
                    const int a0 = (short)orbfe_round_f((1.f - fx) * 2048.f), a1 = (short)orbfe_round_f(fx * 2048.f);
                    xofs[dx] = sx;
                    xal[dx] = (a0 & 0xffff) | (a1 << 16);
                }
                for (int dx = dw; dx < dwp; dx++) { xofs[dx] = xofs[dw - 1]; xal[dx] = xal[dw - 1]; }
                // k_resize_tab reads columns sx[0] .. sx[3]+1 of a source row with one 8-byte load
                bool ok = sw >= 8;
                for (int x4 = 0; ok && x4 < dwp / 4; x4++) {
                    const int w0 = std::min(xofs[x4 * 4], sw - 8);
                    for (int k = 0; k < 4; k++)
                        ok = ok && xofs[x4 * 4 + k] >= w0 && std::min(xofs[x4 * 4 + k] + 1, sw - 1) - w0 <= 7;
                }
                resize_tab_ok[l] = ok;
                for (int dy = 0; dy < dh; dy++) {
                    float fy = (float)((dy + 0.5) * scale_y - 0.5);
                    int sy = orbfe_floor_d(fy);
                    fy -= sy;
                    const int b0 = (short)orbfe_round_f((1.f - fy) * 2048.f), b1 = (short)orbfe_round_f(fy * 2048.f);
                    // rows are NOT clamped like columns: cv::resize keeps the fractional weight and clips the row index
                    ytab[(size_t)dy * 4 + 0] = std::min(std::max(sy, 0), sh - 1);
                    ytab[(size_t)dy * 4 + 1] = std::min(std::max(sy + 1, 0), sh - 1);
                    ytab[(size_t)dy * 4 + 2] = (b0 & 0xffff) << 12;
                    ytab[(size_t)dy * 4 + 3] = (b1 & 0xffff) << 12;
                }
                while (tabs.size() % 4) tabs.push_back(0); // k_resize_tab loads xofs/xal as int4
                tab_off[l * 4 + 0] = tabs.size(); tabs.insert(tabs.end(), xofs.begin(), xofs.end());
                tab_off[l * 4 + 1] = tabs.size(); tabs.insert(tabs.end(), xal.begin(), xal.end());
                while (tabs.size() % 4) tabs.push_back(0); // ... and ytab as int4
                tab_off[l * 4 + 2] = tabs.size(); tabs.insert(tabs.end(), ytab.begin(), ytab.end());
                tab_off[l * 4 + 3] = 0;
            }
        }
        rows = rows_; cols = cols_;
        ncells_total = (int)cellinfo.size();
        ntiles = (int)tiles.size();
        out_total = out;
        max_out_cap = maxcap;
        max_wcell = mwc; max_hcell = mhc;
        pyr_fbytes = pyr + 64;
        blur_fbytes = blur + 64;
        slots_fu32 = slots;
        keys_fu32 = 2 * cand;
        nodecap = maxcap + 8;
        veccap = 1;
        while (veccap < nodecap) veccap <<= 1;
        keycap_lds = 6144;
        {   // the general kernel's key buffers share LDS with the node lists: large quotas leave less room (levels whose candidates do
            // not fit work out of the HBM key scratch)
            const long long room = (long long)160 * 1024 - 3072 - (long long)qt_lds_bytes(0, nodecap, veccap);
            keycap_lds = (int)std::max<long long>(0, std::min<long long>(6144, room / 8)) & ~63;
        }
        {
            // the node lists of DistributeOctTree live in LDS, sized by the largest per-level quota: say so here, not at launch
            int max_ini = 1;
            for (const LevelGeom& g : geom) max_ini = std::max(max_ini, g.nIni);
            const size_t need = std::max(qp_lds_bytes(max_ini, max_ini <= 4 ? 5 : 4, nodecap, veccap), qt_lds_bytes(keycap_lds, nodecap, veccap));
            if (need + 2048 > (size_t)160 * 1024)
                return fail(ORBFE_ERR_CAPACITY, "a pyramid level's quota of %d keypoints (nfeatures %d over %d levels at scale %.3f) needs %zu bytes "
                            "of LDS for the quadtree: more than a workgroup has (about 2700 keypoints per level fit)", maxcap, nfeatures, nlevels,
                            (double)scaleFactor, need);
        }
        batch_cap = 0; // force workspace re-allocation
        if (tabs.empty()) tabs.push_back(0);
        int rc;
        if ((rc = d_geom.ensure(geom.size() * sizeof(LevelGeom)))) return rc;
        if ((rc = d_cellinfo.ensure(cellinfo.size() * 4))) return rc;
        if ((rc = d_tiles.ensure(tiles.size() * 4))) return rc;
        if ((rc = d_tabs.ensure(tabs.size() * 4))) return rc;
        ORBFE_HIP(hipMemcpy(d_geom.p, geom.data(), geom.size() * sizeof(LevelGeom), hipMemcpyHostToDevice));
        ORBFE_HIP(hipMemcpy(d_cellinfo.p, cellinfo.data(), cellinfo.size() * 4, hipMemcpyHostToDevice));
        ORBFE_HIP(hipMemcpy(d_tiles.p, tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice));
        ORBFE_HIP(hipMemcpy(d_tabs.p, tabs.data(), tabs.size() * 4, hipMemcpyHostToDevice));
        return ORBFE_OK;
    }

    // Tables of k_blur7_mfma for the geometry and the taps in force: the strips (level-major), per strip the two pass-1 tap matrices in the
    // B-operand layout of v_mfma_i32_32x32x32_i8 (lane (n, half) holds B[16 half + i][n], i = 0 .. 15, as 16 bytes), BORDER_REFLECT_101
    // folded in, and the two pass-2 matrices whose K index runs over a block's rows in the order pass 1 leaves them in a lane's registers.
    DevBuf d_bstrips, d_btabs, d_btab2;
    int n_bstrips = 0, blur_tabs_ed = -1, blur_tabs_rows = 0, blur_tabs_cols = 0;
    bool blur_mfma_ok = false;
    bool blur_mfma = true;               // test hook (debug key "blur_mfma" = 0): k_blur7 instead
    int build_blur_tables()
    {
        if (blur_tabs_ed == (int)gaussian_ed && blur_tabs_rows == rows && blur_tabs_cols == cols) return ORBFE_OK;
        static const int T0[7] = {18, 34, 49, 55, 49, 34, 18}, T1[7] = {18, 34, 48, 56, 48, 34, 18};
        const int* t = gaussian_ed ? T1 : T0;
        std::vector<BlurStrip> st;
        std::vector<uint8_t> tabs;
        bool ok = true;
        auto refl = [](int p, int n) { while (p < 0 || p >= n) p = (p < 0) ? -p : 2 * (n - 1) - p; return p; };
        for (int l = 0; l < nlevels && ok; l++) {
            const int w = geom[l].w, rowbytes = l == 0 ? w : geom[l].pitch;
            if (w < 48 || rowbytes < 16) { ok = false; break; }
            for (int X = 0; X < w; X += 32) {
                BlurStrip S{};
                S.level = l; S.x0 = X; S.tab = (int)(tabs.size() / 1024);
                auto cl = [&](int c) { return std::min(std::max(c, 0), rowbytes - 16); };
                S.c0 = cl(X - 4); S.c1 = cl(X + 12); S.c2 = cl(X + 28);
                const int cs[3] = {S.c0, S.c1, S.c2};
                // weight of input column xin for output column n
                std::vector<int> W((size_t)w * 32, 0);
                for (int n = 0; n < 32; n++) {
                    if (X + n >= w) continue;
                    for (int u = 0; u < 7; u++) W[(size_t)refl(X + n + u - 3, w) * 32 + n] += t[u];
                }
                std::vector<int> owner((size_t)w, -1);
                for (int x = 0; x < w; x++)
                    for (int pz = 0; pz < 3 && owner[x] < 0; pz++)
                        if (x >= cs[pz] && x < cs[pz] + 16) owner[x] = pz;
                for (int x = 0; x < w && ok; x++)
                    for (int n = 0; n < 32; n++)
                        if (W[(size_t)x * 32 + n] && (owner[x] < 0 || W[(size_t)x * 32 + n] > 127)) ok = false;
                const size_t base = tabs.size();
                tabs.resize(base + 2048, 0);
                for (int ab = 0; ab < 2; ab++)
                    for (int lane = 0; lane < 64; lane++) {
                        const int n = lane & 31, half = lane >> 5;
                        const int piece = ab == 0 ? half : (half == 0 ? 2 : -1);
                        if (piece < 0) continue;
                        for (int i = 0; i < 16; i++) {
                            const int x = cs[piece] + i;
                            if (x < 0 || x >= w || owner[x] != piece) continue;
                            tabs[base + (size_t)ab * 1024 + (size_t)lane * 16 + i] = (uint8_t)(int8_t)W[(size_t)x * 32 + n];
                        }
                    }
                st.push_back(S);
            }
        }
        blur_mfma_ok = ok && !st.empty();
        blur_tabs_ed = (int)gaussian_ed; blur_tabs_rows = rows; blur_tabs_cols = cols;
        if (!blur_mfma_ok) return ORBFE_OK;   // (k_blur7 does such a geometry)
        std::vector<uint8_t> t2(2048, 0);
        for (int ab = 0; ab < 2; ab++)
            for (int lane = 0; lane < 64; lane++) {
                const int n = lane & 31, half = lane >> 5;
                for (int i = 0; i < 16; i++) {
                    const int q = 4 * half + (i & 3) + 8 * (i >> 2);
                    const int u = ab == 0 ? q - n - 1 : q - n + 31;
                    if (u >= 0 && u <= 6) t2[(size_t)ab * 1024 + (size_t)lane * 16 + i] = (uint8_t)t[u];
                }
            }
        n_bstrips = (int)st.size();
        int rc;
        if ((rc = d_bstrips.ensure(st.size() * sizeof(BlurStrip))) || (rc = d_btabs.ensure(tabs.size())) || (rc = d_btab2.ensure(t2.size()))) return rc;
        ORBFE_HIP(hipMemcpy(d_bstrips.p, st.data(), st.size() * sizeof(BlurStrip), hipMemcpyHostToDevice));
        ORBFE_HIP(hipMemcpy(d_btabs.p, tabs.data(), tabs.size(), hipMemcpyHostToDevice));
        ORBFE_HIP(hipMemcpy(d_btab2.p, t2.data(), t2.size(), hipMemcpyHostToDevice));
        return ORBFE_OK;
    }

    int ensure_workspace(int B)
    {
        if (B <= batch_cap) return ORBFE_OK;
        int rc;
        if ((rc = d_pyr.ensure(pyr_fbytes * B))) return rc;
        if ((rc = d_blur.ensure(blur_fbytes * B))) return rc;
        if ((rc = d_slots.ensure(slots_fu32 * 4 * B))) return rc;
        if ((rc = d_cellcnt.ensure((size_t)ncells_total * 4 * B))) return rc;
        if ((rc = d_keys.ensure(keys_fu32 * 4 * B))) return rc;
        if ((rc = d_lvlout.ensure((size_t)out_total * 4 * B))) return rc;
        if ((rc = d_lvlcnt.ensure((size_t)nlevels * 4 * B))) return rc;
        if ((rc = d_lvloff.ensure((size_t)nlevels * 4 * B))) return rc;
        if ((rc = d_lvlncand.ensure((size_t)nlevels * 4 * B))) return rc;
        if ((rc = d_fallback.ensure((size_t)nlevels * 4 * B))) return rc;
        // work list of the levels the count-pyramid quadtree gives up on: [0] = their number (zeroed here, and by k_level_offsets behind
        // every batch), [4 ..] = frame * nlevels + level
        if ((rc = d_worklist.ensure(((size_t)nlevels * B + 4) * 4))) return rc;
        ORBFE_HIP(hipMemset(d_worklist.p, 0, 16));
        if (!d_overflow.p) { // zeroed here and whenever it is read: no memset launch per batch
            if ((rc = d_overflow.ensure(16))) return rc;
            ORBFE_HIP(hipMemset(d_overflow.p, 0, 16));
        }
        batch_cap = B;
        return ORBFE_OK;
    }

    // The batched pipeline: every launch covers all frames.  Asynchronous on `s`.
    int run_device(const uint8_t* d_imgs, int B, size_t frame_stride, int rows_, int cols_, size_t step,
                   orbfe_keypoint* d_kps_out, uint8_t* d_desc_out, int capacity, int32_t* d_n, hipStream_t s, int flag_word = 0)
    {
        // flag_word: 0 = the sticky flag of the device-pointer batches (orbfe_extractor_batch_status), 1 = the host-pointer entry
        // points' own word (they own their whole call, so a device batch's unread flag must not fail them)
        int rc;
        // a batch whose descriptors are still owed (the pipeline defers them by a step) gets them before its buffers are used again
        if (late.pending && (rc = describe_deferred(nullptr, 0))) return rc;
        if ((rc = build_geometry(rows_, cols_))) return rc;
        if ((rc = ensure_workspace(B))) return rc;
        if ((rc = build_blur_tables())) return rc;
        ImgView src0{d_imgs, nullptr, frame_stride, (int)step};
        ImgView pyr{d_pyr.as<uint8_t>(), d_pyr.as<uint8_t>(), pyr_fbytes, 0};
        ImgView blur{d_blur.as<uint8_t>(), d_blur.as<uint8_t>(), blur_fbytes, 0};
        const LevelGeom* dg = d_geom.as<LevelGeom>();
        last_nframes = B;
        last_src0 = src0;
        timer.begin();
        if ((rc = wait_stage(follow, follow_stage, s, this))) return rc;
        timer.mark(s, "start");
        for (int r16_ = 0; r16_ < ORBFE_REPS_ORB(16); r16_++)
        for (int l = 1; l < nlevels; l++) {
            const LevelGeom& g = geom[l];
            const LevelGeom& gp = geom[l - 1];
            ImgView sv = (l == 1) ? src0 : ImgView{pyr.base + gp.img_off, nullptr, pyr_fbytes, gp.pitch};
            ImgView dv{pyr.base + g.img_off, pyr.base_w + g.img_off, pyr_fbytes, g.pitch};
            const int dw4 = (g.w + 3) / 4;
            if (resize_tab_ok[l]) {
                const int nthreads = dw4 * ((g.h + RS_ROWS - 1) / RS_ROWS);
                const int* tb = d_tabs.as<int>();
                const int nx = (nthreads + 255) / 256;
                hipLaunchKernelGGL(k_resize_tab, dim3(xcd_grid(nx * B)), dim3(256), 0, s, sv, dv, gp.w, gp.h, dw4,
                                   g.h, nthreads, tb + tab_off[l * 4 + 0], tb + tab_off[l * 4 + 1],
                                   reinterpret_cast<const int4*>(tb + tab_off[l * 4 + 2]), nx, nx * B);
            } else {
                dim3 grid((dw4 + 63) / 64, (g.h + 7) / 8, B);
                const double scale_x = 1. / ((double)g.w / gp.w), scale_y = 1. / ((double)g.h / gp.h);
                hipLaunchKernelGGL(k_resize_level, grid, dim3(256), 0, s, sv, dv, gp.w, gp.h, dw4, g.h, scale_x, scale_y,
                                   g.w);
            }
        }
        timer.mark(s, "resize");
        {   // stage 4: the pyramid is there, FAST starts
            if (!ev_stage[3]) ORBFE_HIP(hipEventCreateWithFlags(&ev_stage[3], hipEventDisableTiming));
            ORBFE_HIP(hipEventRecord(ev_stage[3], s));
        }
        // The blur only needs the pyramid, and only k_orient_describe needs the blur: it runs on a second stream, forked in front of
        // FAST.  Measured on the C2 batch (step time with the detector running / extractor alone, ms): fork in front of FAST 1.83 /
        // 1.76, fork after FAST (blur next to the quadtree) 1.88 / 1.76, no fork 1.97 / 1.75 (again in round 6: tools/sweeps.md).
        hipStream_t aux_stream = user_aux ? user_aux : this->aux_stream;
        // strips [first, first + count) of the strip list (level-major: level 0's strips come first)
        auto blur_strips = [&](int first, int count) {
            if (count <= 0) return;
            if (gaussian_ed)
                hipLaunchKernelGGL(k_blur7<true>, dim3(xcd_grid(count * B)), dim3(256), 0, aux_stream, src0, pyr, blur, dg,
                                   d_tiles.as<uint32_t>() + first, count, count * B);
            else
                hipLaunchKernelGGL(k_blur7<false>, dim3(xcd_grid(count * B)), dim3(256), 0, aux_stream, src0, pyr, blur, dg,
                                   d_tiles.as<uint32_t>() + first, count, count * B);
        };
        auto launch_blur = [&]() -> int {
            ORBFE_HIP(hipEventRecord(ev_fork, s));
            ORBFE_HIP(hipStreamWaitEvent(aux_stream, ev_fork, 0));
            timer.mark(aux_stream, "blur7 starts", true);
            for (int r_ = 0; r_ < ORBFE_REPS_ORB(8); r_++) {
                if (blur_mfma && blur_mfma_ok) {   // the matrix-core kernel (a wave per 32-column strip, four to a workgroup)
                    const int T = gaussian_ed ? 256 : 257, nxb = (n_bstrips + 3) / 4;
                    hipLaunchKernelGGL(k_blur7_mfma, dim3(xcd_grid(nxb * B)), dim3(256), 0, aux_stream, src0, pyr, blur, dg, d_bstrips.as<BlurStrip>(),
                                       d_btabs.as<uint4>(), d_btab2.as<uint4>(), 128 * T * T + 32768, n_bstrips, nxb, nxb * B);
                } else
                    blur_strips(0, ntiles);
            }
            timer.mark(aux_stream, "blur7");
            ORBFE_HIP(hipEventRecord(ev_join, aux_stream));
            return ORBFE_OK;
        };
        if ((rc = launch_blur())) return rc;
        if ((rc = wait_stage(follow, follow_fast_stage, s, this))) return rc;
        {
            // LDS per wave: ROI (cell + 6), score map (cell + 2), one u16 list of cell pixels
            const int roi_pitch = align_up(max_wcell + 6 + 4, 4) + 8, roi_rows = max_hcell + 6; // +1 byte shift, +2 dwords read past a row (8-pixel groups)
            const int map_pitch = max_wcell + 2, map_rows = max_hcell + 2;
            const int list_cap = max_wcell * max_hcell;
            auto a16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
            const size_t lds = 4 * (a16((size_t)roi_pitch * roi_rows) + a16((size_t)map_pitch * map_rows) +
                                    a16((size_t)list_cap * 2));
            if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&k_fast_cells), lds))) return rc;
            const int nx = (ncells_total + 3) / 4;   // (every level has at least one cell: build_geometry)
            for (int r_ = 0; r_ < ORBFE_REPS_ORB(1); r_++) hipLaunchKernelGGL(k_fast_cells, dim3(xcd_grid(nx * B)), dim3(256), lds, s, src0, pyr, dg,
                               d_cellinfo.as<uint32_t>(), d_slots.as<uint32_t>(), slots_fu32,
                               d_cellcnt.as<int32_t>(), ncells_total, iniThFAST, minThFAST, roi_pitch, roi_rows,
                               map_pitch, map_rows, list_cap, nx, nx * B, 0, ncells_total);
        }
        timer.mark(s, "fast_cells");
        auto stage_event = [&](int k) -> int {
            if (!ev_stage[k]) ORBFE_HIP(hipEventCreateWithFlags(&ev_stage[k], hipEventDisableTiming));
            ORBFE_HIP(hipEventRecord(ev_stage[k], s));
            return ORBFE_OK;
        };
        if ((rc = stage_event(0))) return rc;
        {
            // fast path: count-pyramid quadtree (no keypoint movement); general kernel only for flagged levels
            int max_ini = 1;
            for (const LevelGeom& g : geom) max_ini = std::max(max_ini, g.nIni);
            // depth of the count pyramid: 1024 (2048) leaves for a level's 217 (434) nodes.  Its LDS decides how many of the
            // nlevels x B workgroups are resident at once, and this kernel sits alone on the extractor's critical path: with six
            // levels (4096 leaves, 54 KB, two workgroups per CU) the 2400 workgroups of a C2 batch ran in five rounds, 225 us;
            // a level that needs more depth is flagged and redone by the general kernel
            const int D = force_pyramid_depth ? force_pyramid_depth : max_ini <= 4 ? 5 : 4;
            const size_t lds_p = qp_lds_bytes(max_ini, D, nodecap, veccap);
            { int rc_lds_ = ensure_dyn_lds(reinterpret_cast<const void*>(&k_distribute_pyr), (size_t)(lds_p)); if (rc_lds_) return rc_lds_; }
            const int by_level = 0;   // (frames x levels, every frame's level 0 first: 1.419 against 1.420 ms per C2 step, ten interleaved runs each)
            for (int r_ = 0; r_ < ORBFE_REPS_ORB(2); r_++) hipLaunchKernelGGL(k_distribute_pyr, by_level ? dim3(B, nlevels) : dim3(nlevels, B), dim3(QP_THREADS), lds_p, s, dg, d_slots.as<uint32_t>(),
                               slots_fu32, d_cellcnt.as<int32_t>(), ncells_total, d_lvlout.as<uint32_t>(), out_total,
                               d_lvlcnt.as<int32_t>(), nlevels, d_lvlncand.as<int32_t>(), d_fallback.as<int32_t>(), D,
                               nodecap, veccap, d_worklist.as<int32_t>() + 4, d_worklist.as<int32_t>(), by_level);
            // (the work-list launch keeps its keys in the HBM scratch: a workgroup that asks for 50 KB of LDS it will almost never use
            //  waits for the CU's other tenants -- 87 us behind the detector's threshold kernel, with an EMPTY list)
            const int qcap = force_general_quadtree ? keycap_lds : 0;
            const size_t lds = qt_lds_bytes(qcap, nodecap, veccap);
            { int rc_lds_ = ensure_dyn_lds(reinterpret_cast<const void*>(&k_distribute), qt_lds_bytes(keycap_lds, nodecap, veccap)); if (rc_lds_) return rc_lds_; }
            // the general kernel drains the work list with a small grid (a launch of nlevels x B workgroups of this much LDS that found
            // nothing to do cost the chain 73 us); the test hook runs it for every level, a workgroup each
            const dim3 qgrid = force_general_quadtree ? dim3(nlevels, B) : dim3(std::min(nlevels * B, 128));
            hipLaunchKernelGGL(k_distribute, qgrid, dim3(64), lds, s, dg, d_slots.as<uint32_t>(), slots_fu32,
                               d_cellcnt.as<int32_t>(), ncells_total, d_keys.as<uint32_t>(), keys_fu32,
                               d_lvlout.as<uint32_t>(), out_total, d_lvlcnt.as<int32_t>(), nlevels,
                               d_lvlncand.as<int32_t>(), qcap, nodecap, veccap,
                               force_general_quadtree ? nullptr : d_worklist.as<int32_t>() + 4, d_worklist.as<int32_t>());
        }
        timer.mark(s, "distribute");
        if ((rc = stage_event(1))) return rc;
        {
            int rc2;
            if ((rc2 = d_flatkv.ensure((size_t)B * capacity * 4)) || (rc2 = d_flatlvl.ensure((size_t)B * capacity))) return rc2;
        }
        hipLaunchKernelGGL(k_level_offsets, dim3(B), dim3(256), 0, s, d_lvlcnt.as<int32_t>(), d_lvloff.as<int32_t>(),
                           d_n, nlevels, B, capacity, d_overflow.as<int32_t>() + flag_word, dg, d_lvlout.as<uint32_t>(), out_total,
                           d_flatkv.as<uint32_t>(), d_flatlvl.as<uint8_t>(), d_worklist.as<int32_t>());
        ORBFE_HIP(hipStreamWaitEvent(s, ev_join, 0));
        stage_recorded = true;
        // the descriptors: here, or -- extractor_defer_describe(), the batched pipeline -- when the caller says so (describe_deferred())
        late = Late{true, src0, B, capacity, d_kps_out, d_desc_out, d_n, s};
        if (defer_describe) return ORBFE_OK;
        return describe_deferred(nullptr, 0);
    }

    // k_orient_describe2 of the newest batch, behind stage `gate_stage` of `gate`'s newest batch if one is named
    struct Late { bool pending; ImgView src0; int B, capacity; orbfe_keypoint* kps; uint8_t* desc; int32_t* n; hipStream_t s; };
    Late late{};
    bool defer_describe = false;
    int describe_deferred(orbfe_extractor* gate, int gate_stage)
    {
        if (!late.pending) return ORBFE_OK;
        late.pending = false;
        hipStream_t s = late.s;
        int rc;
        if ((rc = wait_stage(gate, gate_stage, s, this))) return rc;
        ImgView pyr{d_pyr.as<uint8_t>(), d_pyr.as<uint8_t>(), pyr_fbytes, 0};
        ImgView blur{d_blur.as<uint8_t>(), d_blur.as<uint8_t>(), blur_fbytes, 0};
        const int kcap_ = std::min(late.capacity, max_keypoints());
        const int okx = (kcap_ + 7) / 8;   // workgroups per frame: 4 waves of two keypoints
        for (int r_ = 0; r_ < ORBFE_REPS_ORB(4); r_++) hipLaunchKernelGGL(k_orient_describe2, dim3(xcd_grid(okx * late.B)), dim3(256), 0, s, late.src0, pyr, blur, d_geom.as<LevelGeom>(),
                           d_flatkv.as<uint32_t>(), d_flatlvl.as<uint8_t>(), late.n, nlevels, d_pattern.as<uint32_t>(),
                           d_umax.as<uint4>(), late.kps, late.desc, late.capacity, okx, okx * late.B);
        timer.mark(s, "orient_describe");
        if (!ev_stage[2]) ORBFE_HIP(hipEventCreateWithFlags(&ev_stage[2], hipEventDisableTiming));
        ORBFE_HIP(hipEventRecord(ev_stage[2], s));
        ORBFE_HIP(hipGetLastError());
        return ORBFE_OK;
    }
};

namespace orbfe {
void extractor_defer_describe(orbfe_extractor* h, bool on) { if (h) h->defer_describe = on; }
int extractor_describe_now(orbfe_extractor* h, orbfe_extractor* gate, int gate_stage) { return h ? h->describe_deferred(gate, gate_stage) : ORBFE_OK; }
}

extern "C" {

const char* orbfe_last_error(void) { return g_err; }
#ifdef ORBFE_ABLATION
const char* orbfe_version(void) { return "orbfe 0.2 (gfx950) +ablation"; } // diagnosis build: launches can be skipped
#else
const char* orbfe_version(void) { return "orbfe 0.2 (gfx950)"; }
#endif
int orbfe_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

orbfe_extractor* orbfe_extractor_create(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST,
                                        int device)
{
    if (nfeatures <= 0 || nlevels < 1 || nlevels > 15 || !(scaleFactor > 1.0f) || iniThFAST < 1 || minThFAST < 1 ||
        iniThFAST > 254 || minThFAST > 254) {
        fail(ORBFE_ERR_INVALID, "invalid extractor parameters");
        return nullptr;
    }
    if (use_device(device) != ORBFE_OK) return nullptr;
    orbfe_extractor* h = new orbfe_extractor();
    h->nfeatures = nfeatures; h->nlevels = nlevels; h->iniThFAST = iniThFAST; h->minThFAST = minThFAST;
    h->scaleFactor = scaleFactor;
    h->device = device;
    h->build_tables();
    if (hipStreamCreate(&h->own_stream) != hipSuccess || hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess || h->upload_describe_tables() != ORBFE_OK) {
        fail(ORBFE_ERR_HIP, "extractor device initialisation failed");
        delete h;
        return nullptr;
    }
    return h;
}

void orbfe_extractor_destroy(orbfe_extractor* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->paired) { aruco_speculation_wait(h->paired); aruco_unpair_notice(h->paired); } // it reads this handle's buffers (a paired detector outlives the pairing: orbfe.h)
    delete h;
}

int orbfe_extractor_get_levels(const orbfe_extractor* h) { return h ? h->nlevels : ORBFE_ERR_INVALID; }
float orbfe_extractor_get_scale_factor(const orbfe_extractor* h) { return h ? (float)h->scaleFactor : 0.f; }
static int copy_vec(const orbfe_extractor* h, const std::vector<float>& v, float* out)
{
    if (!h || !out) return fail(ORBFE_ERR_INVALID, "null argument");
    memcpy(out, v.data(), v.size() * sizeof(float));
    return (int)v.size();
}
int orbfe_extractor_get_scale_factors(const orbfe_extractor* h, float* out) { return h ? copy_vec(h, h->mvScaleFactor, out) : ORBFE_ERR_INVALID; }
int orbfe_extractor_get_inverse_scale_factors(const orbfe_extractor* h, float* out) { return h ? copy_vec(h, h->mvInvScaleFactor, out) : ORBFE_ERR_INVALID; }
int orbfe_extractor_get_scale_sigma_squares(const orbfe_extractor* h, float* out) { return h ? copy_vec(h, h->mvLevelSigma2, out) : ORBFE_ERR_INVALID; }
int orbfe_extractor_get_inverse_scale_sigma_squares(const orbfe_extractor* h, float* out) { return h ? copy_vec(h, h->mvInvLevelSigma2, out) : ORBFE_ERR_INVALID; }
int orbfe_extractor_get_features_per_level(const orbfe_extractor* h, int32_t* out)
{
    if (!h || !out) return fail(ORBFE_ERR_INVALID, "null argument");
    for (int i = 0; i < h->nlevels; i++) out[i] = h->mnFeaturesPerLevel[i];
    return h->nlevels;
}
int orbfe_extractor_max_keypoints(const orbfe_extractor* h) { return h ? h->max_keypoints() : ORBFE_ERR_INVALID; }

int orbfe_extract_batch_device(orbfe_extractor* h, const uint8_t* d_imgs, int nframes, size_t frame_stride, int rows,
                               int cols, size_t step, orbfe_keypoint* d_kps, uint8_t* d_desc, int capacity,
                               int32_t* d_n_out, void* stream)
{
    if (!h || !d_imgs || !d_kps || !d_desc || !d_n_out || nframes <= 0 || rows <= 0 || cols <= 0 ||
        step < (size_t)cols || capacity <= 0)
        return fail(ORBFE_ERR_INVALID, "orbfe_extract_batch_device: invalid argument");
    int rc = use_device(h->device);
    if (rc) return rc;
    return h->run_device(d_imgs, nframes, frame_stride, rows, cols, step, d_kps, d_desc, capacity, d_n_out,
                         (hipStream_t)stream);
}

int orbfe_extractor_batch_status(orbfe_extractor* h, int32_t* overflow)
{
    if (!h || !overflow) return fail(ORBFE_ERR_INVALID, "orbfe_extractor_batch_status: null argument");
    *overflow = 0;
    if (!h->d_overflow.p) return ORBFE_OK; // no batch yet
    int rc = use_device(h->device);
    if (rc) return rc;
    ORBFE_HIP(hipDeviceSynchronize());
    ORBFE_HIP(hipMemcpy(overflow, h->d_overflow.p, 4, hipMemcpyDeviceToHost));
    if (*overflow) ORBFE_HIP(hipMemset(h->d_overflow.p, 0, 4)); // sticky until read
    return ORBFE_OK;
}

int orbfe_extract_batch(orbfe_extractor* h, const uint8_t* imgs, int nframes, size_t frame_stride, int rows, int cols,
                        size_t step, orbfe_keypoint* kps, uint8_t* desc, int capacity, int32_t* n_out)
{
    if (!h || !n_out) return fail(ORBFE_ERR_INVALID, "orbfe_extract_batch: null argument");
    if (!imgs || rows <= 0 || cols <= 0 || nframes <= 0) { // empty image: ORBextractor.cc:1046
        for (int f = 0; f < nframes; f++) n_out[f] = 0;
        return ORBFE_OK;
    }
    if (!kps || !desc || step < (size_t)cols || capacity <= 0)
        return fail(ORBFE_ERR_INVALID, "orbfe_extract_batch: invalid argument");
    int rc = use_device(h->device);
    if (rc) return rc;
    const int cap = h->max_keypoints();
    const size_t dpitch = (size_t)align_up(cols, 64), dframe = dpitch * rows;
    if ((rc = h->d_in.ensure(dframe * nframes + 64))) return rc;
    if ((rc = h->d_kps.ensure((size_t)cap * nframes * sizeof(orbfe_keypoint)))) return rc;
    if ((rc = h->d_desc.ensure((size_t)cap * nframes * 32))) return rc;
    if ((rc = h->d_nout.ensure((size_t)nframes * 4))) return rc;
    // page-locked staging: [frames in, row pitch dpitch] then [n per frame | flag | keypoints | descriptors] out
    const size_t o_n = (dframe * (size_t)nframes + 255) / 256 * 256, o_flag = o_n + ((size_t)nframes * 4 + 63) / 64 * 64, o_kps = o_flag + 64; // (size_t: a batch of 2 GiB and more)
    const size_t o_desc = o_kps + (size_t)cap * nframes * sizeof(orbfe_keypoint), o_end = o_desc + (size_t)cap * nframes * 32;
    if ((rc = h->pinned.ensure(o_end))) return rc;
    uint8_t* hp = h->pinned.as<uint8_t>();
    hipStream_t s = h->own_stream;
    for (int f = 0; f < nframes; f++)
        for (int y = 0; y < rows; y++) memcpy(hp + f * dframe + (size_t)y * dpitch, imgs + f * frame_stride + (size_t)y * step, (size_t)cols);
    if (h->paired) aruco_speculation_wait(h->paired); // the detector may still be reading the previous frame in d_in
    ORBFE_HIP(hipMemcpyAsync(h->d_in.p, hp, dframe * nframes, hipMemcpyHostToDevice, s));
    if (h->paired && nframes == 1) { // the paired detector starts on the same device copy, on its own stream, next to the launches below
        if (!h->ev_up) ORBFE_HIP(hipEventCreateWithFlags(&h->ev_up, hipEventDisableTiming));
        ORBFE_HIP(hipEventRecord(h->ev_up, s));
        // a frame the detector refuses, or a workspace it cannot get, is the detector's own call's business: the extraction runs
        // "as if nothing had been started" (orbfe.h), and aruco_speculate() leaves no speculation pending when it fails
        if (aruco_speculate(h->paired, h->d_in.as<uint8_t>(), dframe, rows, cols, dpitch, h->ev_up, hp, dpitch) != ORBFE_OK) (void)hipGetLastError();
    }
    if ((rc = h->run_device(h->d_in.as<uint8_t>(), nframes, dframe, rows, cols, dpitch, h->d_kps.as<orbfe_keypoint>(),
                            h->d_desc.as<uint8_t>(), cap, h->d_nout.as<int32_t>(), s, /*flag_word*/ 1)))
        return rc;
    // the results: queued behind the kernels, one wait (blocking copies cost a round trip each: 4 x ~40 us per frame).  A single
    // frame's four arrays go out in one launch that writes the page-locked staging buffer (OutPack); a batch by the copy engine.
    if ((size_t)cap * nframes * 60 <= ((size_t)1 << 20)) {
        OutPack op;
        op.add(hp + o_n, h->d_nout.p, (size_t)nframes * 4);
        op.add(hp + o_flag, h->d_overflow.as<int32_t>() + 1, 4);
        op.add(hp + o_kps, h->d_kps.p, (size_t)cap * nframes * sizeof(orbfe_keypoint));
        op.add(hp + o_desc, h->d_desc.p, (size_t)cap * nframes * 32);
        if ((rc = op.flush<0>(s))) return rc;
    } else {
        ORBFE_HIP(hipMemcpyAsync(hp + o_n, h->d_nout.p, (size_t)nframes * 4, hipMemcpyDeviceToHost, s));
        ORBFE_HIP(hipMemcpyAsync(hp + o_flag, h->d_overflow.as<int32_t>() + 1, 4, hipMemcpyDeviceToHost, s));
        ORBFE_HIP(hipMemcpyAsync(hp + o_kps, h->d_kps.p, (size_t)cap * nframes * sizeof(orbfe_keypoint), hipMemcpyDeviceToHost, s));
        ORBFE_HIP(hipMemcpyAsync(hp + o_desc, h->d_desc.p, (size_t)cap * nframes * 32, hipMemcpyDeviceToHost, s));
    }
    ORBFE_HIP(hipStreamSynchronize(s));
    const int32_t ovf = *reinterpret_cast<const int32_t*>(hp + o_flag);
    if (ovf) ORBFE_HIP(hipMemset(h->d_overflow.as<int32_t>() + 1, 0, 4));
    memcpy(n_out, hp + o_n, (size_t)nframes * 4);
    if (ovf) return fail(ORBFE_ERR_CAPACITY, "internal keypoint capacity exceeded (%d)", ovf);
    for (int f = 0; f < nframes; f++) {
        if (n_out[f] > capacity)
            return fail(ORBFE_ERR_CAPACITY, "frame %d has %d keypoints, capacity is %d", f, n_out[f], capacity);
        if (n_out[f] == 0) continue;
        memcpy(kps + (size_t)f * capacity, hp + o_kps + (size_t)f * cap * sizeof(orbfe_keypoint), (size_t)n_out[f] * sizeof(orbfe_keypoint));
        memcpy(desc + (size_t)f * capacity * 32, hp + o_desc + (size_t)f * cap * 32, (size_t)n_out[f] * 32);
    }
    return ORBFE_OK;
}

int orbfe_extract(orbfe_extractor* h, const uint8_t* img, int rows, int cols, size_t step, orbfe_keypoint* kps,
                  uint8_t* desc, int capacity, int32_t* n_out)
{
    return orbfe_extract_batch(h, img, 1, 0, rows, cols, step, kps, desc, capacity, n_out);
}

int orbfe_extractor_debug_level_size(orbfe_extractor* h, int level, int* w, int* hgt)
{
    if (!h || level < 0 || level >= h->nlevels || h->geom.empty()) return fail(ORBFE_ERR_INVALID, "no geometry");
    *w = h->geom[level].w;
    *hgt = h->geom[level].h;
    return ORBFE_OK;
}

int orbfe_extractor_debug_level_image(orbfe_extractor* h, int frame, int level, int stage, uint8_t* out)
{
    if (!h || !out || level < 0 || level >= h->nlevels || frame < 0 || frame >= h->last_nframes)
        return fail(ORBFE_ERR_INVALID, "debug_level_image: invalid argument");
    int rc = use_device(h->device);
    if (rc) return rc;
    const LevelGeom& g = h->geom[level];
    const uint8_t* src;
    size_t pitch;
    if (stage == 1) { src = h->d_blur.as<uint8_t>() + frame * h->blur_fbytes + g.blur_off; pitch = g.bpitch; }
    else if (level == 0) { src = h->last_src0.base + frame * h->last_src0.fstride; pitch = h->last_src0.pitch; }
    else { src = h->d_pyr.as<uint8_t>() + frame * h->pyr_fbytes + g.img_off; pitch = g.pitch; }
    ORBFE_HIP(hipDeviceSynchronize());
    ORBFE_HIP(hipMemcpy2D(out, g.w, src, pitch, g.w, g.h, hipMemcpyDeviceToHost));
    return ORBFE_OK;
}

int orbfe_extractor_debug_level_keypoints(orbfe_extractor* h, int frame, int level, int stage, orbfe_keypoint* out,
                                          int capacity, int32_t* n)
{
    if (!h || !n || level < 0 || level >= h->nlevels || frame < 0 || frame >= h->last_nframes)
        return fail(ORBFE_ERR_INVALID, "debug_level_keypoints: invalid argument");
    int rc = use_device(h->device);
    if (rc) return rc;
    ORBFE_HIP(hipDeviceSynchronize());
    const LevelGeom& g = h->geom[level];
    std::vector<uint32_t> keys;
    if (stage == 2) { // raw per-level candidate counter written by k_distribute (instrumented builds pack timings here)
        ORBFE_HIP(hipMemcpy(n, h->d_lvlncand.as<int32_t>() + frame * h->nlevels + level, 4, hipMemcpyDeviceToHost));
        return ORBFE_OK;
    }
    if (stage == 3) { // 1 if the level fell back from the count-pyramid quadtree to the general kernel
        ORBFE_HIP(hipMemcpy(n, h->d_fallback.as<int32_t>() + frame * h->nlevels + level, 4, hipMemcpyDeviceToHost));
        return ORBFE_OK;
    }
    if (stage == 0) {
        std::vector<int32_t> cnt(g.ncells);
        ORBFE_HIP(hipMemcpy(cnt.data(), h->d_cellcnt.as<int32_t>() + (size_t)frame * h->ncells_total + g.cell_first,
                            (size_t)g.ncells * 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> slots((size_t)g.cand_cap);
        ORBFE_HIP(hipMemcpy(slots.data(), h->d_slots.as<uint32_t>() + (size_t)frame * h->slots_fu32 + g.slot_off,
                            slots.size() * 4, hipMemcpyDeviceToHost));
        for (int c = 0; c < g.ncells; c++)
            for (int k = 0; k < cnt[c]; k++) keys.push_back(slots[(size_t)c * g.cell_cap + k]);
    } else {
        int32_t c = 0;
        ORBFE_HIP(hipMemcpy(&c, h->d_lvlcnt.as<int32_t>() + frame * h->nlevels + level, 4, hipMemcpyDeviceToHost));
        keys.resize(c);
        if (c)
            ORBFE_HIP(hipMemcpy(keys.data(), h->d_lvlout.as<uint32_t>() + (size_t)frame * h->out_total + g.out_off,
                                (size_t)c * 4, hipMemcpyDeviceToHost));
    }
    *n = (int32_t)keys.size();
    const int add = stage == 0 ? 0 : 16;
    for (int i = 0; i < (int)keys.size() && i < capacity; i++) {
        const uint32_t kv = keys[i];
        out[i].x = (float)((int)(kv & 0xfff) + add);
        out[i].y = (float)((int)((kv >> 12) & 0xfff) + add);
        out[i].size = stage == 0 ? 7.f : g.kp_size;
        out[i].angle = -1.f;
        out[i].response = (float)(kv >> 24);
        out[i].octave = stage == 0 ? 0 : level;
        out[i].class_id = -1;
    }
    return ORBFE_OK;
}

int orbfe_extractor_set_gaussian_taps(orbfe_extractor* h, int mode)
{
    if (!h || (mode != 0 && mode != 1)) return fail(ORBFE_ERR_INVALID, "orbfe_extractor_set_gaussian_taps: mode is 0 or 1");
    h->gaussian_ed = mode == 1;
    return ORBFE_OK;
}

int orbfe_extractor_set_aux_stream(orbfe_extractor* h, void* stream)
{
    if (!h) return fail(ORBFE_ERR_INVALID, "null handle");
    h->user_aux = (hipStream_t)stream;
    return ORBFE_OK;
}

int orbfe_extractor_pair_detector(orbfe_extractor* h, orbfe_aruco* detector)
{
    if (!h) return fail(ORBFE_ERR_INVALID, "null handle");
    if (detector && aruco_device_of(detector) != h->device)   // the detector is started on the extractor's device copy of the frame
        return fail(ORBFE_ERR_INVALID, "orbfe_extractor_pair_detector: extractor on device %d, detector on device %d", h->device, aruco_device_of(detector));
    if (h->paired) { aruco_speculation_wait(h->paired); aruco_unpair_notice(h->paired); }
    h->paired = detector;
    return ORBFE_OK;
}

int orbfe_extractor_follow(orbfe_extractor* h, orbfe_extractor* other, int stage)
{
    if (!h || stage < 0 || stage % 10 > 4 || stage / 10 > 4 || (other && other->device != h->device)) return fail(ORBFE_ERR_INVALID, "orbfe_extractor_follow: invalid argument");
    // stage = start gate + 10 * gate in front of FAST (either may be 0)
    h->follow = stage ? other : nullptr;
    h->follow_stage = stage % 10;
    h->follow_fast_stage = stage / 10;
    return ORBFE_OK;
}

int orbfe_extractor_stage_wait(orbfe_extractor* h, int stage, void* stream)
{
    if (!h || stage < 1 || stage > 4) return fail(ORBFE_ERR_INVALID, "orbfe_extractor_stage_wait: invalid argument");
    int rc = use_device(h->device);
    if (rc) return rc;
    return orbfe_extractor::wait_stage(h, stage, (hipStream_t)stream);
}

int orbfe_extractor_debug_control(orbfe_extractor* h, const char* key, int value)
{
    if (!h || !key) return fail(ORBFE_ERR_INVALID, "orbfe_extractor_debug_control: null argument");
    const bool on_off = value == 0 || value == 1;
    if (!strcmp(key, "kernel_timing") && on_off) { h->timer.enabled = value; h->timer.reset_history(); }
    else if (!strcmp(key, "general_quadtree") && on_off) h->force_general_quadtree = value;
    else if (!strcmp(key, "pyramid_depth") && value >= 0 && value <= 6) h->force_pyramid_depth = value;   // 0 = by the levels' node counts
    else if (!strcmp(key, "blur_mfma") && on_off) h->blur_mfma = value;   // the blur on the matrix cores (default) / k_blur7
    else return fail(ORBFE_ERR_INVALID, "orbfe_extractor_debug_control: unknown key \"%s\" or value %d", key, value);
    return ORBFE_OK;
}

int orbfe_extractor_debug_kernel_times(orbfe_extractor* h, float* out_us, int capacity)
{
    if (!h || !out_us) return fail(ORBFE_ERR_INVALID, "orbfe_extractor_debug_kernel_times: null argument");
    if (capacity < 0) return h->timer.collect_median(out_us, -capacity, nullptr);
    return h->timer.collect(out_us, capacity);
}

} // extern "C"
