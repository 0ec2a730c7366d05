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
    // --- configuration and test hooks
    int device = 0;
    orbfe_aruco* paired = nullptr;       // orbfe_extractor_pair_detector
    bool gaussian_ed = false;            // orbfe_extractor_set_gaussian_taps: 18 34 48 56 48 34 18 instead of 18 34 49 55 49 34 18
    bool defer_describe = false;         // extractor_defer_describe: a batch's descriptors wait for describe_deferred()
    bool force_general_quadtree = false; // test hook: run the general kernel for every level
    int force_pyramid_depth = 0;         // test hook: shallow count pyramid so that levels fall back
    KernelTimer timer;
    // --- streams and events
    hipStream_t own_stream = nullptr, aux_stream = nullptr;
    hipStream_t user_aux = nullptr;      // orbfe_extractor_set_aux_stream: run the blur there instead of on aux_stream
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_up = nullptr;          // the image of the host-pointer call is on the device
    // orbfe_extractor_follow: this handle's batches start behind a stage of ANOTHER handle's latest batch (two engine sets of a
    // pipeline hold a fixed phase that way instead of whatever the contention of the moment settles on)
    orbfe_extractor* follow = nullptr;
    int follow_stage = 0;                // 1 = the other's FAST, 2 = its quadtree, 3 = its descriptors (the whole batch), 4 = its resize chain
    int follow_fast_stage = 0;           // a second gate in front of this handle's FAST (0 = none): the resize chain may run earlier
    hipEvent_t ev_stage[4] = {nullptr, nullptr, nullptr, nullptr};   // after FAST, the quadtree, the descriptors; [3] = after the resize chain (FAST starts)
    bool stage_recorded = false;         // a batch's front part has been enqueued.  A stage's event is created when the stage is first
                                         // enqueued -- the descriptors may come a step later (extractor_defer_describe) -- and a wait skips
                                         // an event that does not exist yet
    // --- the plan of the input size in force (extractor_plan.hpp) and what a batch of it launches
    ExtractorPlan plan;
    int batch_cap = 0;                   // frames the workspace holds
    int last_nframes = 0;
    ImgView last_src0{};
    struct BatchPlan {
        int blur_K2 = 0, blur_nx = 0;    // k_blur7_mfma: its rounding constant for the taps' sum, workgroups (four strips each) per frame
        int roi_pitch = 0, roi_rows = 0, map_pitch = 0, map_rows = 0, list_cap = 0, fast_nx = 0;   // k_fast_cells: LDS layout of a wave, workgroups per frame
        size_t fast_lds = 0;
        int D = 0;                       // k_distribute_pyr: depth of the count pyramid
        size_t qp_lds = 0;
        int qcap = 0;                    // k_distribute: keys it holds in LDS, its LDS and its grid
        size_t qt_lds = 0;
        dim3 qgrid;
        int okx = 0;                     // k_orient_describe2: workgroups per frame
    };
    // --- device buffers: the plan's tables, the describe tables, the per-batch workspace, staging of the host-pointer entry points
    DevBuf d_geom, d_cellinfo, d_tabs, d_bstrips, d_btabs, d_btab2;
    DevBuf d_pattern, d_umax;
    DevBuf d_pyr, d_blur, d_slots, d_cellcnt, d_keys, d_lvlout, d_lvlcnt, d_lvloff, d_lvlncand, d_overflow, d_fallback,
        d_flatkv, d_flatlvl, d_worklist;
    DevBuf d_in, d_kps, d_desc, d_nout;
    PinnedBuf pinned;
    // --- the newest batch's descriptors, owed while extractor_defer_describe is on
    struct Late { bool pending; ImgView src0; int B, capacity, okx; orbfe_keypoint* kps; uint8_t* desc; int32_t* n; hipStream_t s; };
    Late late{};

    // (orbfe_extractor_destroy selects the device; the buffers release themselves behind this body)
    ~orbfe_extractor()
    {
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

    template <class T> static int upload(DevBuf& d, const std::vector<T>& v)
    {
        if (int rc = d.ensure(v.size() * sizeof(T))) return rc;
        if (!v.empty()) ORBFE_HIP(hipMemcpy(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return ORBFE_OK;
    }
    // The plan for a rows x cols input with the taps in force.  A size the plan refuses leaves the handle as it was; a failed upload
    // leaves it without a plan (the next batch starts over) rather than with host tables that disagree with the device's.
    int ensure_plan(int rows_, int cols_)
    {
        if (rows_ == plan.rows && cols_ == plan.cols && gaussian_ed == plan.gaussian_ed) return ORBFE_OK;
        ExtractorPlan fresh = plan_extractor(rows_, cols_, nlevels, mvScaleFactor.data(), mvInvScaleFactor.data(), mnFeaturesPerLevel.data(), gaussian_ed);
        if (fresh.err) return fail(fresh.err, "%s", fresh.msg);
        const bool resized = rows_ != plan.rows || cols_ != plan.cols;
        plan = ExtractorPlan{};
        last_nframes = 0;
        int rc;
        if ((rc = upload(d_geom, fresh.geom)) || (rc = upload(d_cellinfo, fresh.cellinfo)) || (rc = upload(d_tabs, fresh.resize_tabs)) ||
            (rc = upload(d_bstrips, fresh.blur_strips)) || (rc = upload(d_btabs, fresh.blur_tabs)) || (rc = upload(d_btab2, fresh.blur_tab2)))
            return rc;
        if (resized) batch_cap = 0;   // the per-frame blocks have other sizes: the workspace is allocated again
        plan = std::move(fresh);
        return ORBFE_OK;
    }

    int ensure_workspace(int B)
    {
        if (B <= batch_cap) return ORBFE_OK;
        int rc;
        if ((rc = d_pyr.ensure(plan.pyr_fbytes * B))) return rc;
        if ((rc = d_blur.ensure(plan.blur_fbytes * B))) return rc;
        if ((rc = d_slots.ensure(plan.slots_fu32 * 4 * B))) return rc;
        if ((rc = d_cellcnt.ensure((size_t)plan.ncells_total * 4 * B))) return rc;
        if ((rc = d_keys.ensure(plan.keys_fu32 * 4 * B))) return rc;
        if ((rc = d_lvlout.ensure((size_t)plan.out_total * 4 * B))) return rc;
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

    // What a batch of B frames launches, decided once; and everything that can fail -- the workspace, the flat keypoint list of
    // `capacity` a frame, the kernels' dynamic LDS -- before the batch's first launch
    int plan_batch(int B, int capacity, BatchPlan& p)
    {
        const int T = gaussian_ed ? 256 : 257;
        p.blur_K2 = 128 * T * T + 32768;
        p.blur_nx = ((int)plan.blur_strips.size() + 3) / 4;
        // FAST, LDS per wave: ROI (cell + 6), score map (cell + 2), one u16 list of cell pixels
        p.roi_pitch = align_up(plan.max_wcell + 6 + 4, 4) + 8; p.roi_rows = plan.max_hcell + 6; // +1 byte shift, +2 dwords read past a row (8-pixel groups)
        p.map_pitch = plan.max_wcell + 2; p.map_rows = plan.max_hcell + 2;
        p.list_cap = plan.max_wcell * plan.max_hcell;
        auto a16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
        p.fast_lds = 4 * (a16((size_t)p.roi_pitch * p.roi_rows) + a16((size_t)p.map_pitch * p.map_rows) + a16((size_t)p.list_cap * 2));
        p.fast_nx = (plan.ncells_total + 3) / 4;   // (every level has at least one cell: plan_levels)
        // depth of the count pyramid: 1024 (2048) leaves for a level's 217 (434) nodes.  Its LDS decides how many of the
        // nlevels x B workgroups are resident at once, and this kernel sits alone on the extractor's critical path: with six
        // levels (4096 leaves, 54 KB, two workgroups per CU) the 2400 workgroups of a C2 batch ran in five rounds, 225 us;
        // a level that needs more depth is flagged and redone by the general kernel
        p.D = force_pyramid_depth ? force_pyramid_depth : plan.max_ini <= 4 ? 5 : 4;
        p.qp_lds = qp_lds_bytes(plan.max_ini, p.D, plan.nodecap, plan.veccap);
        // (the work-list launch keeps its keys in the HBM scratch: a workgroup that asks for 50 KB of LDS it will almost never use
        //  waits for the CU's other tenants -- 87 us behind the detector's threshold kernel, with an EMPTY list)
        p.qcap = force_general_quadtree ? plan.keycap_lds : 0;
        p.qt_lds = qt_lds_bytes(p.qcap, plan.nodecap, plan.veccap);
        // the general kernel drains the work list with a small grid (a launch of nlevels x B workgroups of this much LDS that found
        // nothing to do cost the chain 73 us); the test hook runs it for every level, a workgroup each
        p.qgrid = force_general_quadtree ? dim3(nlevels, B) : dim3(std::min(nlevels * B, 128));
        p.okx = (std::min(capacity, max_keypoints()) + 7) / 8;   // 4 waves of two keypoints
        int rc;
        if ((rc = ensure_workspace(B)) || (rc = d_flatkv.ensure((size_t)B * capacity * 4)) || (rc = d_flatlvl.ensure((size_t)B * capacity))) return rc;
        if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&k_fast_cells), p.fast_lds)) ||
            (rc = ensure_dyn_lds(reinterpret_cast<const void*>(&k_distribute_pyr), p.qp_lds)) ||
            (rc = ensure_dyn_lds(reinterpret_cast<const void*>(&k_distribute), qt_lds_bytes(plan.keycap_lds, plan.nodecap, plan.veccap))))
            return rc;
        return ORBFE_OK;
    }

    // queue on `st` a wait for stage k (1 .. 4 as in follow_stage; 0 = no gate) of h's newest batch.  No wait when h is null or is
    // `self` (a handle is not gated by itself), nor before h's front part has been enqueued once.
    static int wait_stage(const orbfe_extractor* h, int k, hipStream_t st, const orbfe_extractor* self = nullptr)
    {
        if (h && h != self && h->stage_recorded && k >= 1 && k <= 4 && h->ev_stage[k - 1]) ORBFE_HIP(hipStreamWaitEvent(st, h->ev_stage[k - 1], 0));
        return ORBFE_OK;
    }
    // stage k (as in follow_stage) of the batch being enqueued is complete at this point of `s`
    int stage_event(int k, hipStream_t s)
    {
        if (!ev_stage[k - 1]) ORBFE_HIP(hipEventCreateWithFlags(&ev_stage[k - 1], hipEventDisableTiming));
        ORBFE_HIP(hipEventRecord(ev_stage[k - 1], s));
        return ORBFE_OK;
    }

    // The batched pipeline: every launch covers all frames.  Asynchronous on `s`.
    // flag_word: 0 = the sticky flag of the device-pointer batches (orbfe_extractor_batch_status), 1 = the host-pointer entry
    // points' own word (they own their whole call, so a device batch's unread flag must not fail them)
    int run_device(const uint8_t* d_imgs, int B, size_t frame_stride, int rows_, int cols_, size_t step,
                   orbfe_keypoint* d_kps_out, uint8_t* d_desc_out, int capacity, int32_t* d_n, hipStream_t s, int flag_word = 0)
    {
        int rc;
        // a batch whose descriptors are still owed (the pipeline defers them by a step) gets them before its buffers are used again
        if (late.pending && (rc = describe_deferred(nullptr, 0))) return rc;
        BatchPlan p;
        if ((rc = ensure_plan(rows_, cols_)) || (rc = plan_batch(B, capacity, p))) return rc;
        const ImgView src0{d_imgs, nullptr, frame_stride, (int)step};
        last_nframes = B;
        last_src0 = src0;
        timer.begin();
        if ((rc = wait_stage(follow, follow_stage, s, this))) return rc;
        timer.mark(s, "start");
        for (int r_ = 0; r_ < ORBFE_REPS_ORB(16); r_++) resize_chain(src0, B, s);
        timer.mark(s, "resize");
        if ((rc = stage_event(4, s))) return rc;   // the pyramid is there, FAST starts
        if ((rc = blur_fork(p, src0, B, s))) return rc;
        if ((rc = wait_stage(follow, follow_fast_stage, s, this))) return rc;
        for (int r_ = 0; r_ < ORBFE_REPS_ORB(1); r_++) fast(p, src0, B, s);
        timer.mark(s, "fast_cells");
        if ((rc = stage_event(1, s))) return rc;
        quadtree(p, B, s);
        timer.mark(s, "distribute");
        if ((rc = stage_event(2, s))) return rc;
        level_offsets(B, capacity, d_n, flag_word, s);
        ORBFE_HIP(hipStreamWaitEvent(s, ev_join, 0));   // the blur joins: the descriptors read it
        stage_recorded = true;
        // the descriptors: here, or -- extractor_defer_describe(), the batched pipeline -- when the caller says so (describe_deferred())
        late = Late{true, src0, B, capacity, p.okx, d_kps_out, d_desc_out, d_n, s};
        return defer_describe ? ORBFE_OK : describe_deferred(nullptr, 0);
    }

    ImgView pyr_view() const { return ImgView{d_pyr.as<uint8_t>(), d_pyr.as<uint8_t>(), plan.pyr_fbytes, 0}; }
    ImgView blur_view() const { return ImgView{d_blur.as<uint8_t>(), d_blur.as<uint8_t>(), plan.blur_fbytes, 0}; }

    // the pyramid: level l from level l - 1, a launch each
    void resize_chain(const ImgView& src0, int B, hipStream_t s)
    {
        const ImgView pyr = pyr_view();
        for (int l = 1; l < nlevels; l++) {
            const LevelGeom& g = plan.geom[l];
            const LevelGeom& gp = plan.geom[l - 1];
            ImgView sv = (l == 1) ? src0 : ImgView{pyr.base + gp.img_off, nullptr, plan.pyr_fbytes, gp.pitch};
            ImgView dv{pyr.base + g.img_off, pyr.base_w + g.img_off, plan.pyr_fbytes, g.pitch};
            const int dw4 = (g.w + 3) / 4;
            if (plan.resize_tab_ok[l]) {
                const int nthreads = dw4 * ((g.h + RS_ROWS - 1) / RS_ROWS);
                const int* tb = d_tabs.as<int>();
                const int nx = (nthreads + 255) / 256;
                hipLaunchKernelGGL(k_resize_tab, dim3(xcd_grid(nx * B)), dim3(256), 0, s, sv, dv, gp.w, gp.h, dw4,
                                   g.h, nthreads, tb + plan.tab_off[l * 3 + 0], tb + plan.tab_off[l * 3 + 1],
                                   reinterpret_cast<const int4*>(tb + plan.tab_off[l * 3 + 2]), nx, nx * B);
            } else {
                dim3 grid((dw4 + 63) / 64, (g.h + 7) / 8, B);
                const double scale_x = 1. / ((double)g.w / gp.w), scale_y = 1. / ((double)g.h / gp.h);
                hipLaunchKernelGGL(k_resize_level, grid, dim3(256), 0, s, sv, dv, gp.w, gp.h, dw4, g.h, scale_x, scale_y,
                                   g.w);
            }
        }
    }

    // The blur only needs the pyramid, and only k_orient_describe2 needs the blur: it runs on a second stream, forked in front of
    // FAST (run_device joins it in front of the descriptors).  Measured on the C2 batch (step time with the detector running /
    // extractor alone, ms): fork in front of FAST 1.83 / 1.76, fork after FAST (blur next to the quadtree) 1.88 / 1.76, no fork
    // 1.97 / 1.75 (again in round 6: tools/sweeps.md).  The matrix-core kernel: a wave per 32-column strip, four to a workgroup.
    int blur_fork(const BatchPlan& p, const ImgView& src0, int B, hipStream_t s)
    {
        hipStream_t aux = user_aux ? user_aux : aux_stream;
        ORBFE_HIP(hipEventRecord(ev_fork, s));
        ORBFE_HIP(hipStreamWaitEvent(aux, ev_fork, 0));
        timer.mark(aux, "blur7 starts", true);
        for (int r_ = 0; r_ < ORBFE_REPS_ORB(8); r_++)
            hipLaunchKernelGGL(k_blur7_mfma, dim3(xcd_grid(p.blur_nx * B)), dim3(256), 0, aux, src0, pyr_view(), blur_view(), d_geom.as<LevelGeom>(),
                               d_bstrips.as<BlurStrip>(), d_btabs.as<uint4>(), d_btab2.as<uint4>(), p.blur_K2, (int)plan.blur_strips.size(),
                               p.blur_nx, p.blur_nx * B);
        timer.mark(aux, "blur7");
        ORBFE_HIP(hipEventRecord(ev_join, aux));
        return ORBFE_OK;
    }

    void fast(const BatchPlan& p, const ImgView& src0, int B, hipStream_t s)
    {
        hipLaunchKernelGGL(k_fast_cells, dim3(xcd_grid(p.fast_nx * B)), dim3(256), p.fast_lds, s, src0, pyr_view(), d_geom.as<LevelGeom>(),
                           d_cellinfo.as<uint32_t>(), d_slots.as<uint32_t>(), plan.slots_fu32,
                           d_cellcnt.as<int32_t>(), plan.ncells_total, iniThFAST, minThFAST, p.roi_pitch, p.roi_rows,
                           p.map_pitch, p.map_rows, p.list_cap, p.fast_nx, p.fast_nx * B, 0, plan.ncells_total);
    }

    // fast path: count-pyramid quadtree (no keypoint movement); general kernel only for flagged levels (the work list)
    void quadtree(const BatchPlan& p, int B, hipStream_t s)
    {
        const LevelGeom* dg = d_geom.as<LevelGeom>();
        // (grid = levels x frames; frames x levels, every frame's level 0 first: 1.419 against 1.420 ms per C2 step, ten interleaved runs each)
        for (int r_ = 0; r_ < ORBFE_REPS_ORB(2); r_++)
            hipLaunchKernelGGL(k_distribute_pyr, dim3(nlevels, B), dim3(QP_THREADS), p.qp_lds, s, dg, d_slots.as<uint32_t>(),
                               plan.slots_fu32, d_cellcnt.as<int32_t>(), plan.ncells_total, d_lvlout.as<uint32_t>(), plan.out_total,
                               d_lvlcnt.as<int32_t>(), nlevels, d_lvlncand.as<int32_t>(), d_fallback.as<int32_t>(), p.D,
                               plan.nodecap, plan.veccap, d_worklist.as<int32_t>() + 4, d_worklist.as<int32_t>(), /*by_level*/ 0);
        hipLaunchKernelGGL(k_distribute, p.qgrid, dim3(64), p.qt_lds, s, dg, d_slots.as<uint32_t>(), plan.slots_fu32,
                           d_cellcnt.as<int32_t>(), plan.ncells_total, d_keys.as<uint32_t>(), plan.keys_fu32,
                           d_lvlout.as<uint32_t>(), plan.out_total, d_lvlcnt.as<int32_t>(), nlevels,
                           d_lvlncand.as<int32_t>(), p.qcap, plan.nodecap, plan.veccap,
                           force_general_quadtree ? nullptr : d_worklist.as<int32_t>() + 4, d_worklist.as<int32_t>());
    }

    // per frame: the levels' offsets in the output, the keypoint count, the flat (key, level) list of the descriptor kernel
    void level_offsets(int B, int capacity, int32_t* d_n, int flag_word, hipStream_t s)
    {
        hipLaunchKernelGGL(k_level_offsets, dim3(B), dim3(256), 0, s, d_lvlcnt.as<int32_t>(), d_lvloff.as<int32_t>(),
                           d_n, nlevels, B, capacity, d_overflow.as<int32_t>() + flag_word, d_geom.as<LevelGeom>(), d_lvlout.as<uint32_t>(),
                           plan.out_total, d_flatkv.as<uint32_t>(), d_flatlvl.as<uint8_t>(), d_worklist.as<int32_t>());
    }

    // k_orient_describe2 of the newest batch, behind stage `gate_stage` of `gate`'s newest batch if one is named
    int describe_deferred(orbfe_extractor* gate, int gate_stage)
    {
        if (!late.pending) return ORBFE_OK;
        late.pending = false;
        hipStream_t s = late.s;
        int rc;
        if ((rc = wait_stage(gate, gate_stage, s, this))) return rc;
        for (int r_ = 0; r_ < ORBFE_REPS_ORB(4); r_++)
            hipLaunchKernelGGL(k_orient_describe2, dim3(xcd_grid(late.okx * late.B)), dim3(256), 0, s, late.src0, pyr_view(), blur_view(),
                               d_geom.as<LevelGeom>(), d_flatkv.as<uint32_t>(), d_flatlvl.as<uint8_t>(), late.n, nlevels, d_pattern.as<uint32_t>(),
                               d_umax.as<uint4>(), late.kps, late.desc, late.capacity, late.okx, late.okx * late.B);
        timer.mark(s, "orient_describe");
        if ((rc = stage_event(3, s))) return rc;
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
    if (!h || !d_imgs || !d_kps || !d_desc || !d_n_out || nframes <= 0 || rows <= 0 || cols <= 0 || capacity <= 0)
        return fail(ORBFE_ERR_INVALID, "orbfe_extract_batch_device: invalid argument");
    char why[192];   // level 0 is read from the caller's buffer as it lies: what the kernels' offsets cannot address is refused here
    if (plan_input_layout(rows, cols, step, frame_stride, nframes, why, sizeof(why))) return fail(ORBFE_ERR_INVALID, "orbfe_extract_batch_device: %s", why);
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
    if (!h || level < 0 || level >= h->nlevels || h->plan.geom.empty()) return fail(ORBFE_ERR_INVALID, "no geometry");
    *w = h->plan.geom[level].w;
    *hgt = h->plan.geom[level].h;
    return ORBFE_OK;
}

int orbfe_extractor_debug_level_image(orbfe_extractor* h, int frame, int level, int stage, uint8_t* out)
{
    if (!h || !out || level < 0 || level >= h->nlevels || frame < 0 || frame >= h->last_nframes)
        return fail(ORBFE_ERR_INVALID, "debug_level_image: invalid argument");
    int rc = use_device(h->device);
    if (rc) return rc;
    const LevelGeom& g = h->plan.geom[level];
    ORBFE_HIP(hipDeviceSynchronize());
    if (stage == 1) {   // the blurred level is tiled (extractor_plan.hpp): its tiles as they lie, put in rows here
        std::vector<uint8_t> tiles((size_t)g.btrow * blur_tiles_y(g.h));
        ORBFE_HIP(hipMemcpy(tiles.data(), h->d_blur.as<uint8_t>() + frame * h->plan.blur_fbytes + g.blur_off, tiles.size(), hipMemcpyDeviceToHost));
        for (int y = 0; y < g.h; y++)
            for (int x = 0; x < g.w; x++) out[(size_t)y * g.w + x] = tiles[blur_tile_off(g.btrow, x, y)];
        return ORBFE_OK;
    }
    const uint8_t* src;
    size_t pitch;
    if (level == 0) { src = h->last_src0.base + frame * h->last_src0.fstride; pitch = h->last_src0.pitch; }
    else { src = h->d_pyr.as<uint8_t>() + frame * h->plan.pyr_fbytes + g.img_off; pitch = g.pitch; }
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
    const LevelGeom& g = h->plan.geom[level];
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
        ORBFE_HIP(hipMemcpy(cnt.data(), h->d_cellcnt.as<int32_t>() + (size_t)frame * h->plan.ncells_total + g.cell_first,
                            (size_t)g.ncells * 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> slots((size_t)g.cand_cap);
        ORBFE_HIP(hipMemcpy(slots.data(), h->d_slots.as<uint32_t>() + (size_t)frame * h->plan.slots_fu32 + g.slot_off,
                            slots.size() * 4, hipMemcpyDeviceToHost));
        for (int c = 0; c < g.ncells; c++)
            for (int k = 0; k < cnt[c]; k++) keys.push_back(slots[(size_t)c * g.cell_cap + k]);
    } else {
        int32_t c = 0;
        ORBFE_HIP(hipMemcpy(&c, h->d_lvlcnt.as<int32_t>() + frame * h->nlevels + level, 4, hipMemcpyDeviceToHost));
        keys.resize(c);
        if (c)
            ORBFE_HIP(hipMemcpy(keys.data(), h->d_lvlout.as<uint32_t>() + (size_t)frame * h->plan.out_total + g.out_off,
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
