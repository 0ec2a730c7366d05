// aruco_detector.hip -- host side of the ArUco marker detector behind the C ABI (include/orbfe.h).
//
// Mirrors aruco::MarkerDetector as configured by the reference at src/Frame.cc:129-142:
//   setDictionary(name), setDetectionMode(DM_NORMAL), setCornerRefinementMethod(CORNER_LINES), detect(gray).
// Effective parameters: adaptive threshold window max(3, 15*W/1920) made odd, C = 7, one
// threshold image, contours longer than 70 points, approxPolyDP eps 5 %, markerWarpPixSize 5, pyrfactor 2,
// borderDistThres 0.015, error correction off.  Pose estimation (step 12) is not part of this path yet.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <limits>
#include <map>

#include "aruco_kernels.hpp"
#include "aruco_pose.hpp"
#include "detector_plan.hpp"
#include "host_stage.hpp"
#include "orbfe_common.hpp"
#include "orbfe_tables.inc"

using namespace orbfe;

// What a run of the device pipeline does differently from the configuration of Frame.cc:135-137 (aruco_modes.hip)
struct ModeRun {
    const uint8_t* d_full = nullptr; // minSize > 0: the full-resolution frames (pyramid, warps, cornerUpsample); d_imgs is the reduction
    size_t full_fstride = 0, full_step = 0;
    int full_rows = 0, full_cols = 0;
    int fixed_thr = -1;              // THRES_AUTO_FIXED: the global threshold (-1: adaptive)
    uint32_t* d_hist = nullptr;      // THRES_AUTO_FIXED: per frame, 256 bins over the accepted candidates' patches
    std::function<int(hipStream_t)> before_finalize; // trackingMinDetections: the host looks at the decode results and may adopt rejected candidates
};

// the window of cv::cornerSubPix for half size w, (2 w + 1)^2 weights: exp(-y^2) exp(-x^2) in float, by the host's expf like the reference
static void subpix_window(int w, float* mk)
{
    for (int i = 0; i < 2 * w + 1; i++)
        for (int j = 0; j < 2 * w + 1; j++) {
            const float y = (float)(i - w) / w, x = (float)(j - w) / w;
            mk[i * (2 * w + 1) + j] = (float)(std::exp(-y * y) * std::exp(-x * x));
        }
}

// the handle's streams and events: a base of the handle, so that they are destroyed after its members -- the device buffers, which
// release themselves
struct DetectorQueues {
    hipStream_t own_stream = nullptr, aux_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    ~DetectorQueues()
    {
        if (own_stream) (void)hipStreamDestroy(own_stream);
        if (aux_stream) (void)hipStreamDestroy(aux_stream);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
    }
};

struct orbfe_aruco : DetectorQueues {
    int device = 0;
    std::string dict_name;
    int nbits = 0, nb = 0, S = 0, ncodes = 0;
    hipStream_t user_aux = nullptr; // orbfe_aruco_set_aux_stream: run the pyramid there instead of on aux_stream
    // every switch of how a batch runs (detector_plan.hpp): environment at creation, then orbfe_aruco_debug_control / _set_big_frames
    DetectorSwitches sw;
    // what the kernels are told about the input size in force (detector_plan.hpp); swapped in whole by build_geometry
    DetectorGeometry geo;
    int batch_cap = 0;
    DevBuf d_twork, d_trect, d_tctr; // k_tail_prep -> k_tail_approx -> k_tail_finish: work list, 4-gon flags, list length
    DevBuf d_rstate, d_lut; // k_contours_relay -> k_contours_small: per-frame grid shift and pool fill; the walks' step table
    DevBuf d_segs, d_tailkeys, d_tailoff, d_small, d_hint; // d_hint: the relay kernel's grid spacing of the previous batch
    PinnedBuf pinned; // staging of the host-pointer entry points
    DevBuf d_poses;   // orbfe_aruco_detect_poses
    // speculation for a paired extractor (orbfe_extractor_pair_detector; orbfe_common.hpp)
    struct Spec {
        bool pending = false, has_pose = false; // work enqueued and not consumed yet; poses were computed with `cam` / `size`
        int rows = 0, cols = 0;
        const uint8_t* host_copy = nullptr; // the extractor's staged frame (orbfe_common.hpp)
        size_t host_pitch = 0;
        PoseCamera cam{};
        float size = 0.f;
    } spec;
    bool last_cam_valid = false; // camera and marker size of the last detect-with-poses call: what the speculation assumes
    PoseCamera last_cam{};
    float last_size = 0.f;
    DevBuf d_dwork, d_dctr, d_ditems, d_dhist, d_dpatch; // k_prefilter -> k_decode_warp / _otsu / _vote: the batch's candidates
    bool decode_dirty = false; // the decode work-list counter may be non-zero
    bool tail_dirty = false;   // the work-list counters may be non-zero (set while the tail's three launches are being enqueued)
    int n_escalations = 0;     // batches done again on the next contour path (orbfe_aruco_debug_contour_retries: the tests assert 0 for ordinary frames)
    DevBuf d_ctmlist;
    bool ct_dirty = true;      // the per-frame counters of the walk kernel may be non-zero (first use; a batch abandoned before k_ct_lists)
    unsigned ct_gen = 0;       // generation tag of the hash table's entries (16 bits; the table is cleared when it wraps and before first use)
    bool ct_tab_dirty = true;
    DevBuf d_ctseg, d_cthtab, d_ctelem, d_ctstate, d_ctitemsA, d_ctitemsB, d_ctnitems, d_ctcodes;
    DevBuf d_tstrips, d_ttabs, d_ttab2;
    ThresholdTables ttab;   // the tables of k_threshold_mfma on the device (detector_plan.hpp)
    template <class T> static int upload(DevBuf& d, const std::vector<T>& v)
    {
        if (int rc = d.ensure(v.size() * sizeof(T))) return rc;
        if (!v.empty()) ORBFE_HIP(hipMemcpy(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return ORBFE_OK;
    }
    // For a batch whose plan says Thr::mfma (plan_batch: threshold_tables_apply).  A failed upload leaves the handle without tables
    // (the next batch that wants them starts over)
    int ensure_threshold_tables()
    {
        if (ttab.cols == geo.cols && ttab.win == geo.win) return ORBFE_OK;
        ThresholdTables fresh = plan_threshold_tables(geo.cols, geo.win);
        ttab = ThresholdTables{};
        if (!fresh.ok) return fail(ORBFE_ERR_INVALID, "matrix-core threshold tables refused a %d-pixel row at window %d", geo.cols, geo.win);
        int rc;
        if ((rc = upload(d_tstrips, fresh.strips)) || (rc = upload(d_ttabs, fresh.tabs)) || (rc = upload(d_ttab2, fresh.tab2))) return rc;
        ttab = std::move(fresh);
        return ORBFE_OK;
    }
    bool specks_ran = false;   // the last batch's contour kernels read d_bitsc
    DevBuf d_bitsc;
    DevBuf d_codes, d_levels, d_bits, d_pyr, d_candq, d_pool, d_kept, d_rects, d_counts, d_candidx, d_ncand,
        d_result, d_gpad;
    DevBuf d_in, d_out, d_nout;
    // MarkerDetector::Params the ABI exposes (markerdetector.h:96-214): error_correction_rate, cornerRefinementM
    float error_rate = 0.0f;
    int max_corr = 0, tau = 0, nsorted = 0; // int(tau * error_rate); the dictionary's code map in std::map order
    int corner_method = 1;                  // aruco::CornerRefinementMethod: 0 CORNER_SUBPIX, 1 CORNER_LINES, 2 CORNER_NONE
    DevBuf d_scodes, d_sids, d_msrc;        // d_msrc: rectangle (= contour) of every output marker of the last batch
    // MarkerDetector::Params outside the configuration of Frame.cc:135-137 (markerdetector.h:158-196; kernels in aruco_modes.hip)
    int detect_mode = 0;         // DM_NORMAL 0, DM_FAST 1, DM_VIDEO_FAST 2
    int thres_method = 0;        // THRES_ADAPTIVE 0, THRES_AUTO_FIXED 1
    int thres_value = 7;         // Params::ThresHold: the adaptive constant C, or the global threshold carried from frame to frame
    int n_attempts_auto_fix = 3; // Params::NAttemptsAutoThresFix
    float min_size = 0.f;        // Params::minSize as setDetectionMode / the automatic size estimation leave it
    bool auto_size = false;      // Params::autoSize (DM_VIDEO_FAST)
    float ts = 0.25f;
    bool enclosed = false;       // Params::enclosedMarker (detectEnclosedMarkers, markerdetector.h:126)
    // Params::trackingMinDetections (markerdetector.h:187; markerdetector_impl.cpp:7107-7890): a marker found in that many calls and
    // missing now is looked for among the candidates the dictionary rejected, inside its last outline
    int tracking_min = 0;
    std::map<int, int> marker_counts;         // id -> calls it was found in (one less per call without it)
    std::vector<orbfe_marker> prev_markers;   // what the previous call returned
    int last_tracked = 0;
    int gray_bits15 = 0;         // BGR2GRAY with 15 fractional bits (OpenCV 3.4.2+) instead of 14
    int last_attempts = 0, last_work_rows = 0, last_work_cols = 0;
    size_t rl_static = 0;
    DevBuf d_red, d_mhist, d_masks, d_bgr, d_bits2;
    // batch(floor, &ran) enqueues the pipeline on the contour paths from `floor` on and the copy of its nframes x 4 counts to `counts`;
    // done again on the next path while a frame exceeded a capacity (escalate(); not while "legacy_contours" pins the single walker)
    template <class Batch> int with_retries(Batch&& batch, const int32_t* counts, int nframes)
    {
        for (Contours floor = Contours::tiled;;) {
            Contours ran = Contours::none; int flags_or = 0, rc;
            if ((rc = batch(floor, &ran))) return rc;
            ORBFE_HIP(hipStreamSynchronize(own_stream));
            for (int f = 0; f < nframes; f++) flags_or |= counts[f * 4 + 2];
            if (sw.force_legacy || (floor = escalate(ran, flags_or, geo.relay_tbits != 0)) == Contours::none) return ORBFE_OK;
            n_escalations++;
        }
    }
    bool stateful() const { return thres_method == 1 || auto_size || tracking_min > 0; } // a frame's result depends on the frames before it
    KernelTimer timer;
    int last_nframes = 0;

    int set_dictionary(const char* name)
    {
        for (int i = 0; i < ORBFE_NDICTS; i++)
            if (!strcmp(ORBFE_DICTS[i].name, name)) {
                const orbfe_dict_entry& d = ORBFE_DICTS[i];
                if (d.nbits > 36) return fail(ORBFE_ERR_DICT, "dictionary %s: %d-bit codes are not supported", name, d.nbits);
                dict_name = name;
                nbits = d.nbits;
                nb = (int)std::sqrt((double)nbits);
                S = 5 * (nb + 2); // getMarkerWarpSize(): markerWarpPixSize * nSubdivisions (markerdetector_impl.cpp:1199-1292)
                ncodes = d.ncodes;
                int rc = d_codes.ensure((size_t)std::max(ncodes, 1) * 8);
                if (rc) return rc;
                if (ncodes) ORBFE_HIP(hipMemcpy(d_codes.p, d.codes, (size_t)ncodes * 8, hipMemcpyHostToDevice));
                // Dictionary::getMapCode() for the error-correction pass: std::map<uint64_t, uint16_t> = codes ascending, the FIRST id of
                // a duplicated code (map.insert does not overwrite, dictionary.cpp:99-103)
                std::vector<std::pair<unsigned long long, int>> m;
                for (int k = 0; k < ncodes; k++) m.push_back({d.codes[k], k});
                std::stable_sort(m.begin(), m.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
                std::vector<unsigned long long> sc;
                std::vector<int32_t> si;
                for (size_t k = 0; k < m.size(); k++)
                    if (k == 0 || m[k].first != m[k - 1].first) { sc.push_back(m[k].first); si.push_back(m[k].second); }
                nsorted = (int)sc.size();
                if ((rc = d_scodes.ensure((size_t)std::max(nsorted, 1) * 8)) || (rc = d_sids.ensure((size_t)std::max(nsorted, 1) * 4))) return rc;
                if (nsorted) {
                    ORBFE_HIP(hipMemcpy(d_scodes.p, sc.data(), (size_t)nsorted * 8, hipMemcpyHostToDevice));
                    ORBFE_HIP(hipMemcpy(d_sids.p, si.data(), (size_t)nsorted * 4, hipMemcpyHostToDevice));
                }
                tau = d.tau;
                max_corr = (int)((float)tau * error_rate); // dictionary_based.cpp: static_cast<int>(static_cast<float>(tau()) * rate)
                invalidate_geometry(); // pyramid depth depends on S
                return ORBFE_OK;
            }
        // the reference treats an unknown name as a file path and throws (dictionary.cpp:44-62)
        return fail(ORBFE_ERR_DICT, "unknown dictionary '%s'", name);
    }

    void invalidate_geometry() { geo = DetectorGeometry{}; }   // an input of the plan other than the sizes changed: the next batch plans again
    // rows_ x cols_: the image that is thresholded and traced; prows x pcols: the frame the /2 pyramid is built from.  The plan is made
    // on the host and its level table uploaded to a buffer of its own before either replaces the handle's: a size the plan refuses and
    // a failed allocation or upload leave the handle answering for the geometry it had.
    int build_geometry(int rows_, int cols_, int prows, int pcols)
    {
        if (geo.matches(rows_, cols_, prows, pcols)) return ORBFE_OK;
        if (!rl_static) {   // static LDS of the relay kernels, asked from the runtime (detector_plan.hpp)
            size_t most = 0;
            const void* fns[4] = {reinterpret_cast<const void*>(k_contours_relay), reinterpret_cast<const void*>(k_contours_relay8),
                                  reinterpret_cast<const void*>(k_contours_relay8g), reinterpret_cast<const void*>(k_contours_relay_wide)};
            for (const void* fn : fns) {
                hipFuncAttributes fa{};
                ORBFE_HIP(hipFuncGetAttributes(&fa, fn));
                most = std::max(most, (size_t)fa.sharedSizeBytes);
            }
            rl_static = most + 256;
        }
        DetectorGeometry fresh = plan_detector(rows_, cols_, prows, pcols, S, sw.specks_inkernel, sw.lcap, rl_static);
        if (fresh.err) return fail(fresh.err, "%s", fresh.msg);
        DevBuf lv;
        if (int rc = upload(lv, fresh.levels)) return rc;
        std::swap(d_levels.p, lv.p); std::swap(d_levels.bytes, lv.bytes);
        geo = std::move(fresh);
        batch_cap = 0;
        return ORBFE_OK;
    }

    int ensure_workspace(int B)
    {
        if (B <= batch_cap) return ORBFE_OK;
        int rc;
        if ((rc = d_bits.ensure(geo.bits_fu32 * 4 * B)) || (rc = d_pyr.ensure(geo.pyr_fbytes * B)) ||   // (d_bitsc: when the speck launch runs)
            (rc = d_candq.ensure(geo.candq_fu32 * 4 * B)) || (rc = d_pool.ensure(geo.pool_fu32 * 4 * B)) ||
            (rc = d_kept.ensure((size_t)AR_MAX_KEPT_BIG * sizeof(ArKept) * B)) ||
            (rc = d_rects.ensure((size_t)AR_MAX_RECTS * sizeof(ArRect) * B)) || (rc = d_counts.ensure((size_t)16 * B)) ||
            (rc = d_candidx.ensure((size_t)AR_MAX_RECTS * 4 * B)) || (rc = d_ncand.ensure((size_t)4 * B)) ||
            (rc = d_result.ensure((size_t)AR_MAX_RECTS * 8 * B)) || (rc = d_msrc.ensure((size_t)AR_MAX_RECTS * 4 * B)) ||
            (rc = d_gpad.ensure(std::max<size_t>(geo.gpad_fu32 * 4 * B, 16))) ||
            (rc = d_segs.ensure(std::max<size_t>(((size_t)sizeof(RelaySeg) << geo.relay_tbits) * B, 16))) ||
            (rc = d_tailkeys.ensure((size_t)geo.relay_kcap * 8 * B)) || (rc = d_tailoff.ensure((size_t)geo.relay_kcap * 4 * B)) ||
            (rc = d_small.ensure((size_t)geo.relay_kcap * 16 * B)) || (rc = d_rstate.ensure((size_t)8 * B)) ||
            (rc = d_twork.ensure((size_t)geo.relay_kcap * 32 * B)) || (rc = d_trect.ensure((size_t)geo.relay_kcap * B)))
            return rc;
        if (sw.tiled != 0) {
            const size_t elem_words = (size_t)geo.ct_segcap + ((size_t)geo.ct_segcap + 3) / 4; // u64 elements + u16 next ids, per frame
            if ((rc = d_ctseg.ensure((size_t)5 * geo.ct_segcap * 4 * B)) || (rc = d_cthtab.ensure(((size_t)8 << geo.ct_hbits) * B)) ||
                (rc = d_ctelem.ensure(elem_words * 8 * B)) || (rc = d_ctstate.ensure((size_t)CT_STATE_INTS * 4 * B)) ||
                (rc = d_ctitemsA.ensure((size_t)geo.ct_items_per_frame * 16 * B)) || (rc = d_ctitemsB.ensure((size_t)geo.ct_items_per_frame * 8 * B)) ||
                (rc = d_ctnitems.ensure((size_t)4 * B)) || (rc = d_ctcodes.ensure((size_t)geo.ct_segcap * CT_CODE_WORDS * 4 * B)) ||
                (rc = d_ctmlist.ensure((size_t)CTB_MCAP * 4 * ((geo.rows + 31) / 32) * B)))   // (one list per band; at most one band per cell row)
                return rc;
            ct_dirty = true; ct_tab_dirty = true;
        }
        if (!d_hint.p) {
            if ((rc = d_hint.ensure(16))) return rc;
            ORBFE_HIP(hipMemset(d_hint.p, 0, 16));
        }
        {
            const size_t items = (size_t)B * AR_MAX_RECTS;
            if ((rc = d_dwork.ensure(items * 4)) || (rc = d_ditems.ensure(items * sizeof(DcItem))) || (rc = d_dhist.ensure(items * 512)) ||
                (rc = d_dpatch.ensure(items * DC_PATCH_BYTES)))
                return rc;
        }
        if (!d_dctr.p) {   // [0]: k_finalize leaves the counter at zero for the next batch; [2], [3]: flagged frames and the union of their
                           // flags over every batch since aruco_flags_since_read last cleared them (k_finalize adds to them)
            if ((rc = d_dctr.ensure(16))) return rc;
            ORBFE_HIP(hipMemset(d_dctr.p, 0, 16));
        }
        if (!d_tctr.p) {   // k_tail_finish leaves the two counters at zero for the next batch
            if ((rc = d_tctr.ensure(16))) return rc;
            ORBFE_HIP(hipMemset(d_tctr.p, 0, 16));
        }
        if (!d_lut.p) {
            if ((rc = d_lut.ensure(2048 * 2))) return rc;
            hipLaunchKernelGGL(k_relay_lut, dim3(8), dim3(256), 0, 0, d_lut.as<uint16_t>());
            ORBFE_HIP(hipDeviceSynchronize());
        }
        batch_cap = B;
        return ORBFE_OK;
    }

    // window tables of cv::cornerSubPix for half sizes 1 .. 8
    int ensure_subpix_masks()
    {
        if (d_masks.p) return ORBFE_OK;
        std::vector<float> m((size_t)8 * 17 * 17, 0.f);
        for (int w = 1; w <= 8; w++) subpix_window(w, m.data() + (size_t)(w - 1) * 17 * 17);
        if (int rc = d_masks.ensure(m.size() * 4)) return rc;
        ORBFE_HIP(hipMemcpy(d_masks.p, m.data(), m.size() * 4, hipMemcpyHostToDevice));
        return ORBFE_OK;
    }

    // A batch: the pipeline on the first contour path from `floor` on that may run; *ran = the one it took (escalate())
    int run_device(const uint8_t* d_imgs, int B, size_t frame_stride, int rows_, int cols_, size_t step, orbfe_marker* d_out_m, int capacity,
                   int32_t* d_n, hipStream_t s, const ModeRun* mr = nullptr, Contours floor = Contours::tiled, Contours* ran = nullptr)
    {
        int rc;
        const bool reduced = mr && mr->d_full;
        if ((rc = build_geometry(rows_, cols_, reduced ? mr->full_rows : rows_, reduced ? mr->full_cols : cols_))) return rc;
        if ((rc = ensure_workspace(B))) return rc;
        if ((reduced || corner_method == 0) && (rc = ensure_subpix_masks())) return rc;
        last_nframes = B;
        const ImgView srcW{d_imgs, nullptr, frame_stride, (int)step}; // what is thresholded and traced
        // the frame the pyramid starts from and the patches are warped from (level 0)
        const ImgView src0 = reduced ? ImgView{mr->d_full, nullptr, mr->full_fstride, (int)mr->full_step} : srcW;
        timer.begin();
        timer.mark(s, "start");
        const BatchPlan p = plan_batch(geo, B, BatchMode{!(mr && mr->fixed_thr >= 0), reduced, thres_value}, floor, sw);
        if (p.thr == Thr::mfma && (rc = ensure_threshold_tables())) return rc;
        if (ran) *ran = p.contours;
        // the /2 pyramid is only needed by k_decode: it runs on a second stream next to threshold + contours (what the threshold kernel
        // leaves of it: behind that kernel, in line)
        hipStream_t aux = p.nfuse ? s : user_aux ? user_aux : aux_stream;
        if (!p.nfuse) { ORBFE_HIP(hipEventRecord(ev_fork, s)); ORBFE_HIP(hipStreamWaitEvent(aux, ev_fork, 0)); }
        timer.mark(aux, "pyramid starts", true);
        if (!p.nfuse) pyramid(1, src0, B, aux);
        timer.mark(aux, "pyramid");
        if (!p.nfuse) ORBFE_HIP(hipEventRecord(ev_join, aux));
        int enlarge_k = geo.win;   // detectEnclosedMarkers: the candidates grow by half the adaptive window, or half the erosion size
        if ((rc = threshold(p, srcW, src0, mr ? mr->fixed_thr : -1, B, s, &enlarge_k))) return rc;
        timer.mark(s, "threshold");
        ORBFE_HIP(hipGetLastError());
        if ((rc = speck_pass(p, B, s))) return rc;
        const uint32_t* cbits = (p.specks ? d_bitsc : d_bits).as<uint32_t>();
        bool finish_in_prefilter = false;   // k_tail_finish's work inside k_prefilter (set where the tail kernels are launched)
        for (int r_ = 0; p.contours <= Contours::relay && r_ < ORBFE_REPS_ARUCO(1); r_++)
            if ((rc = p.contours == Contours::tiled ? contours_tiled(p, B, cbits, s) : contours_relay(p, B, cbits, s)) || (rc = relay_tail(B, s, &finish_in_prefilter))) return rc;
        if (p.contours >= Contours::walker && (rc = contours_single_walker(p, B, cbits, s))) return rc;
        timer.mark(s, "contours");
        ORBFE_HIP(hipGetLastError());
        if ((rc = prefilter_decode(p, B, s, src0, enlarge_k, finish_in_prefilter))) return rc;
        timer.mark(s, "decode");
        if ((rc = finalize(B, s, src0, mr, d_out_m, capacity, d_n))) return rc;
        timer.mark(s, "finalize");
        ORBFE_HIP(hipGetLastError());
        decode_dirty = false;   // k_finalize leaves the work-list length at zero
        return ORBFE_OK;
    }

    ImgView pyr_view() { return ImgView{d_pyr.as<uint8_t>(), d_pyr.as<uint8_t>(), geo.pyr_fbytes, 0}; }
    // the /2 pyramid from level `first` on; which kernel makes a level: plan_pyramid_kernels (detector_plan.hpp)
    void pyramid(int first, const ImgView& src0, int B, hipStream_t st)
    {
        const ImgView pyr = pyr_view();
        const std::vector<PyrKernel> K = plan_pyramid_kernels(geo, first, (unsigned)((uintptr_t)src0.base & 15), src0.pitch, src0.fstride, sw.half_pyr);
        if (first == 1 && first < geo.npyr && (K[1] == PyrKernel::half_pyr4 || K[1] == PyrKernel::half_pyr3)) {
            // the leading exact halvings in one launch (k_half_pyr): four from 16 x 16 source blocks, or three from 8 x 8
            const int nf = K[1] == PyrKernel::half_pyr4 ? 4 : 3, bs = 1 << nf;
            HalfPyrDst P{};
            P.base = pyr.base_w; P.fstride = geo.pyr_fbytes;
            for (int p = 1; p <= nf; p++) { P.off[p - 1] = (uint32_t)geo.levels[p].off; P.pitch[p - 1] = geo.levels[p].pitch; }
            const int bw = geo.levels[0].w / bs, nblocks = bw * (geo.levels[0].h / bs);
            if (nf == 4) hipLaunchKernelGGL(k_half_pyr<4>, dim3((nblocks + 255) / 256, B), dim3(256), 0, st, src0, P, bw, nblocks);
            else hipLaunchKernelGGL(k_half_pyr<3>, dim3((nblocks + 255) / 256, B), dim3(256), 0, st, src0, P, bw, nblocks);
            first = nf + 1;
        }
        for (int p = first; p < geo.npyr; p++) {
            const ArLevel &L = geo.levels[p], &Lp = geo.levels[p - 1];
            ImgView sv = (p == 1) ? src0 : ImgView{pyr.base + Lp.off, nullptr, geo.pyr_fbytes, Lp.pitch};
            ImgView dv{pyr.base + L.off, pyr.base_w + L.off, geo.pyr_fbytes, L.pitch};
            if (K[p] == PyrKernel::half_area4) {
                const int dw4 = (L.w + 3) / 4, nthreads = dw4 * ((L.h + 1) / 2);   // reads 8 * dw4 bytes of a source row: within a pitch that is a multiple of 8
                hipLaunchKernelGGL(k_half_area4, dim3((nthreads + 255) / 256, B), dim3(256), 0, st, sv, dv, dw4, L.h);
            } else if (K[p] == PyrKernel::half_area) {
                hipLaunchKernelGGL(k_half_area, dim3((L.w + 63) / 64, (L.h + 3) / 4, B), dim3(256), 0, st, sv, dv, L.w, L.h);
            } else {
                const int dw4 = (L.w + 3) / 4;
                const double scale_x = 1. / ((double)L.w / Lp.w), scale_y = 1. / ((double)L.h / Lp.h);
                hipLaunchKernelGGL(k_resize_level, dim3((dw4 + 63) / 64, (L.h + 7) / 8, B), dim3(256), 0, st, sv, dv,
                                   Lp.w, Lp.h, dw4, L.h, scale_x, scale_y, L.w);
            }
        }
    }
    // the instance of k_threshold_pyr for the window (it is built for windows 5, 7, 11 and 15)
    template <class K> K by_window(K k5, K k7, K k11, K k15) const { return geo.win == 5 ? k5 : geo.win == 7 ? k7 : geo.win == 11 ? k11 : k15; }
    // the bit image d_bits (k_threshold_pyr: and the pyramid, its first levels in the kernel and the rest behind it)
    int threshold(const BatchPlan& p, const ImgView& srcW, const ImgView& src0, int fixed_thr, int B, hipStream_t s, int* enlarge_k)
    {
        for (int r_ = 0; r_ < ORBFE_REPS_ARUCO(8); r_++) {
            const int ntx = (geo.cols + 63) / 64, ntl = ntx * ((geo.rows + 63) / 64);
            const dim3 tg(ntx, (geo.rows + 63) / 64, B), tg1(xcd_grid(ntl * B));
            uint32_t* bp = d_bits.as<uint32_t>();
            if (p.thr == Thr::fixed) {   // THRES_AUTO_FIXED: cv::threshold(THRESH_BINARY_INV) at the carried-over threshold
                if (enclosed) {               // detectEnclosedMarkers: the inner edge band of the thresholded regions (erode + xor)
                    if (int rc = d_bits2.ensure(geo.bits_fu32 * 4 * B)) return rc;
                    const int k = *enlarge_k = int(std::max(3.0, 3. / 1920. * float(geo.cols))) | 1;   // (made odd)
                    if (k / 2 > 15) return fail(ORBFE_ERR_INVALID, "detectEnclosedMarkers: frame too wide (erosion size %d)", k);
                }
                hipLaunchKernelGGL(k_fixed_threshold, dim3((geo.wpr * geo.rows + 255) / 256, B), dim3(256), 0, s, srcW, geo.cols, geo.rows, fixed_thr, enclosed ? d_bits2.as<uint32_t>() : bp, geo.bits_fu32, geo.wpr);
                if (enclosed) hipLaunchKernelGGL(k_erode_cross_xor, dim3((geo.wpr * geo.rows + 255) / 256, B), dim3(256), 0, s, d_bits2.as<uint32_t>(), bp, geo.bits_fu32, geo.wpr, geo.cols, geo.rows, *enlarge_k / 2);
            } else if (p.thr == Thr::mfma) {
                const int n2 = geo.win * geo.win, n_tstrips = (int)ttab.strips.size(), nxs = (n_tstrips + 3) / 4;
                hipLaunchKernelGGL(k_threshold_mfma, dim3(xcd_grid(nxs * B)), dim3(256), 0, s, srcW, geo.cols, geo.rows, ttab.rb, -(n2 * thres_value - n2 / 2),
                                   d_tstrips.as<ThrStrip>(), d_ttabs.as<uint4>(), d_ttab2.as<uint4>(), bp, geo.bits_fu32, geo.wpr, n_tstrips, nxs, nxs * B, n2 > 127 ? 1 : 0);
            } else if (p.thr == Thr::pyr) {
                ThrPyr P{};
                P.n = p.nfuse;
                for (int l = 1; l <= p.nfuse; l++) { P.w[l - 1] = geo.levels[l].w; P.h[l - 1] = geo.levels[l].h; P.pitch[l - 1] = geo.levels[l].pitch; P.off[l - 1] = geo.levels[l].off; }
                hipLaunchKernelGGL(by_window(k_threshold_pyr<5>, k_threshold_pyr<7>, k_threshold_pyr<11>, k_threshold_pyr<15>), tg1, dim3(256), 0, s,
                                   srcW, geo.cols, geo.rows, p.thr_kk, bp, geo.bits_fu32, geo.wpr, ntx, ntl, ntl * B, pyr_view(), P);
                if (p.nfuse && r_ == 0) pyramid(p.nfuse + 1, src0, B, s);
            } else if (geo.win <= 15) hipLaunchKernelGGL(k_adaptive_threshold<7>, tg, dim3(256), 0, s, srcW, geo.cols, geo.rows, geo.win, thres_value, 1.0 / (geo.win * geo.win), bp, geo.bits_fu32, geo.wpr);
            else hipLaunchKernelGGL(k_adaptive_threshold<15>, tg, dim3(256), 0, s, srcW, geo.cols, geo.rows, geo.win, thres_value, 1.0 / (geo.win * geo.win), bp, geo.bits_fu32, geo.wpr);
        }
        return ORBFE_OK;
    }
    // the speck passes as a launch of their own: d_bits -> d_bitsc
    int speck_pass(const BatchPlan& p, int B, hipStream_t s)
    {
        int rc;
        const size_t spk_lds = speck_lds_bytes(geo.cols);
        if (!(specks_ran = p.specks)) return ORBFE_OK;
        if ((rc = d_bitsc.ensure(geo.bits_fu32 * 4 * batch_cap)) || (rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_speck_clean), spk_lds))) return rc;
        hipLaunchKernelGGL(k_speck_clean, dim3((geo.rows + SPK_ROWS - 1) / SPK_ROWS, B), dim3(SPK_THREADS), spk_lds, s, d_bits.as<uint32_t>(), geo.bits_fu32, geo.wpr,
                           geo.cols, geo.rows, d_bitsc.as<uint32_t>());
        return ORBFE_OK;
    }
    // the tiled relay formulation (aruco_tiles.hip): k_ct_band or k_ct_walk, k_ct_lists, k_ct_points
    int contours_tiled(const BatchPlan& p, int B, const uint32_t* cbits, hipStream_t s)
    {
        int rc;
        const int cw = p.tile_w, ncols = (geo.cols + cw - 1) / cw, nbands = (geo.rows + 31) / 32, total_tiles = ncols * nbands * B;
        const int wave_bytes = ctw_wave_lds_bytes(cw), wlds = wave_bytes * (CTW_THREADS / 64);
        const int walk_wgs = std::max(1, std::min((total_tiles / p.tpw + CTW_THREADS / 64 - 1) / (CTW_THREADS / 64), 256 * 8));
        const size_t llds = (size_t)geo.ct_lcap * 8 + 16;
        if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_ct_walk), (size_t)wlds)) || (rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_ct_lists), llds))) return rc;
        if (ct_dirty) ORBFE_HIP(hipMemsetAsync(d_ctstate.p, 0, (size_t)CT_STATE_INTS * 4 * B, s)); // first use, or a batch abandoned before k_ct_lists (which leaves them at zero)
        ct_gen = (ct_gen + 1) & 0xffffu;
        if (ct_gen == 0) { ct_gen = 1; ct_tab_dirty = true; }
        if (ct_tab_dirty) { ORBFE_HIP(hipMemsetAsync(d_cthtab.p, 0, d_cthtab.bytes, s)); ct_tab_dirty = false; }
        ct_dirty = true;
        if (p.band) {
            const int nb = ((geo.rows + 31) / 32 + p.band_rows - 1) / p.band_rows;
            const size_t blds = ctb_lds_bytes(geo.cols, p.band_rows);
            if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_ct_band), blds))) return rc;
            hipLaunchKernelGGL(k_ct_band, dim3(nb, B), dim3(CTB_THREADS), blds, s, cbits, geo.bits_fu32, geo.wpr, geo.cols, geo.rows, 70,
                               d_lut.as<uint16_t>(), p.band_rows, d_ctmlist.as<uint32_t>(), CTB_MCAP, d_cthtab.as<unsigned long long>(), geo.ct_hbits, ct_gen,
                               d_ctseg.as<uint32_t>(), (size_t)5 * geo.ct_segcap, geo.ct_segcap, d_ctstate.as<int32_t>(), d_pool.as<uint32_t>(), geo.pool_fu32,
                               (int)geo.pool_fu32, geo.relay_kcap, d_tailkeys.as<unsigned long long>(), d_tailoff.as<int32_t>(), d_ctcodes.as<uint4>());
        } else
            hipLaunchKernelGGL(k_ct_walk, dim3(walk_wgs), dim3(CTW_THREADS), wlds, s, cbits, geo.bits_fu32, geo.wpr, geo.cols, geo.rows, 70,
                               d_lut.as<uint16_t>(), cw, ncols, nbands, total_tiles, d_cthtab.as<unsigned long long>(), geo.ct_hbits, ct_gen,
                               d_ctseg.as<uint32_t>(), (size_t)5 * geo.ct_segcap, geo.ct_segcap, d_ctstate.as<int32_t>(), d_pool.as<uint32_t>(), geo.pool_fu32,
                               (int)geo.pool_fu32, geo.relay_kcap, d_tailkeys.as<unsigned long long>(), d_tailoff.as<int32_t>(), wave_bytes,
                               d_ctcodes.as<uint4>());
        hipLaunchKernelGGL(k_ct_lists, dim3(B), dim3(geo.ct_lcap > 4096 ? 1024 : 512), llds, s, d_ctseg.as<uint32_t>(), (size_t)5 * geo.ct_segcap, geo.ct_segcap,
                           d_ctstate.as<int32_t>(), d_cthtab.as<unsigned long long>(), geo.ct_hbits, ct_gen, d_ctelem.as<unsigned long long>(), geo.ct_lcap, 70,
                           (int)geo.pool_fu32, geo.relay_kcap, d_tailkeys.as<unsigned long long>(), d_tailoff.as<int32_t>(), d_counts.as<int32_t>(),
                           d_rstate.as<int32_t>(), d_ctitemsA.as<uint4>(), d_ctitemsB.as<uint2>(), geo.ct_items_per_frame, d_ctnitems.as<int32_t>());
        if (hipPeekAtLastError() == hipSuccess) ct_dirty = false;
        hipLaunchKernelGGL(k_ct_points, dim3(geo.ct_items_per_frame >= 8192 ? 32 : 8, B), dim3(256), 0, s, d_ctitemsA.as<uint4>(), d_ctitemsB.as<uint2>(),
                           geo.ct_items_per_frame, d_ctnitems.as<int32_t>(), d_ctcodes.as<uint32_t>(), geo.ct_segcap, d_pool.as<uint32_t>(), geo.pool_fu32);
        return ORBFE_OK;
    }
    // the one-workgroup relay kernels (a workgroup per frame), then k_contours_small
    int contours_relay(const BatchPlan& p, int B, const uint32_t* cbits, hipStream_t s)
    {
        const size_t rlds = relay_lds_bytes(geo.relay_global ? 0 : geo.lds_bits_words, geo.relay_kcap, geo.relay_tbits);
        // (round 2 launched the large-frame kernels, whose workgroups take a CU's whole LDS, in chunks of N frames: no gain at 128 / 192,
        // worse below -- profiles/r02_relay_chunks.txt; one launch since round 5)
        if (p.relay == Relay::relay8g) {
            if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_contours_relay8g), rlds)) return rc;
            hipLaunchKernelGGL(k_contours_relay8g, dim3(B), dim3(RL_THREADS_BIG), rlds, s, cbits, geo.bits_fu32, geo.wpr,
                               geo.cols, geo.rows, 0, 70, geo.relay_kshift, geo.relay_tbits, d_segs.as<RelaySeg>(),
                               d_pool.as<uint32_t>(), geo.pool_fu32, (int)geo.pool_fu32, d_kept.as<ArKept>(), geo.relay_kcap, geo.relay_kcap,
                               d_tailkeys.as<unsigned long long>(), d_tailoff.as<int32_t>(), d_counts.as<int32_t>(), d_hint.as<int32_t>(),
                               d_small.as<uint4>(), d_rstate.as<int32_t>(), d_gpad.as<uint32_t>(), geo.gpad_fu32, d_lut.as<uint16_t>(), 0);
        } else {
            auto rfn = p.relay == Relay::relay8 ? k_contours_relay8 : p.relay == Relay::wide ? k_contours_relay_wide : k_contours_relay;
            if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(rfn), rlds)) return rc;
            hipLaunchKernelGGL(rfn, dim3(B), dim3(p.relay == Relay::relay ? RL_THREADS : RL_THREADS_BIG), rlds, s, cbits, geo.bits_fu32, geo.wpr,
                               geo.cols, geo.rows, geo.lds_bits_words, 70, geo.relay_kshift, geo.relay_tbits, d_segs.as<RelaySeg>(),
                               d_pool.as<uint32_t>(), geo.pool_fu32, (int)geo.pool_fu32, d_kept.as<ArKept>(), geo.relay_kcap, geo.relay_kcap,
                               d_tailkeys.as<unsigned long long>(), d_tailoff.as<int32_t>(), d_counts.as<int32_t>(), d_hint.as<int32_t>(),
                               d_small.as<uint4>(), d_rstate.as<int32_t>(), (p.small_separate ? 1 : 0) | (sw.specks_inkernel && !p.specks && !p.small_separate ? 2 : 0),
                               d_lut.as<uint16_t>(), 0, d_candq.as<uint32_t>(), geo.candq_fu32);
        }
        // the borders that touch no grid line, for frames done with a grid by a relay kernel that leaves them out (the
        // HBM-resident one: its bands fit LDS here; for LDS-resident frames the separate launch halves the relay kernel's time
        // but issues twice the instructions of the in-kernel phase -- measured 1.85 -> 1.98 ms per C2 step -- so those keep
        // phase (c) inside): bands of K rows, K >= 2^relay_kshift
        if (p.small_separate) {
            const int nwaves = ((geo.cols >> RS_BLOCK_SHIFT) + 1) * ((geo.rows >> geo.relay_kshift) + 1); // blocks of the finest grid
            hipLaunchKernelGGL(k_contours_small, dim3((nwaves + RS_THREADS / 64 - 1) / (RS_THREADS / 64), B), dim3(RS_THREADS), 0, s,
                               cbits, geo.bits_fu32, geo.wpr, geo.cols, geo.rows, 70, d_lut.as<uint16_t>(), d_rstate.as<int32_t>(),
                               d_pool.as<uint32_t>(), geo.pool_fu32, (int)geo.pool_fu32, geo.relay_kcap, d_tailkeys.as<unsigned long long>(),
                               d_tailoff.as<int32_t>(), d_counts.as<int32_t>());
        }
        return ORBFE_OK;
    }
    // (g) of the tiled and relay paths: sort + rank per frame, approxPolyDP by persistent waves over the whole batch's borders, rectangles per frame
    int relay_tail(int B, hipStream_t s, bool* finish_in_prefilter)
    {
        int rc;
        const int pts = RT_PTS, tail_wgs = std::min(RT_WGS, B * 128);   // pts: LDS point buffer per wave; longer borders are read from the pool
        const size_t alds = tail_approx_lds_bytes(pts);
        if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_tail_prep), tail_prep_lds_bytes(geo.relay_kcap))) || (rc = ensure_dyn_lds(reinterpret_cast<const void*>(k_tail_approx), alds))) return rc;
        if (tail_dirty) ORBFE_HIP(hipMemsetAsync(d_tctr.p, 0, 16, s));   // a previous batch was abandoned between prep and finish
        tail_dirty = true;
        hipLaunchKernelGGL(k_tail_prep, dim3(B), dim3(geo.relay_global ? 1024 : 256), tail_prep_lds_bytes(geo.relay_kcap), s,
                           d_tailkeys.as<unsigned long long>(), d_tailoff.as<int32_t>(), geo.relay_kcap, d_counts.as<int32_t>(),
                           d_twork.as<uint4>(), (size_t)geo.relay_kcap * B, d_tctr.as<int32_t>());
        hipLaunchKernelGGL(k_tail_approx, dim3(tail_wgs), dim3(256), alds, s, geo.relay_kcap, d_twork.as<uint4>(), (size_t)geo.relay_kcap * B, d_tctr.as<int32_t>(),
                           d_pool.as<uint32_t>(), geo.pool_fu32, d_kept.as<ArKept>(), geo.relay_kcap, d_trect.as<uint8_t>(), pts);
        // (the rectangle lists: a launch of their own only when the enclosed-marker pass sits between them and k_prefilter)
        if ((*finish_in_prefilter = !enclosed)) return ORBFE_OK;
        hipLaunchKernelGGL(k_tail_finish, dim3(B), dim3(64), 0, s, geo.relay_kcap, d_trect.as<uint8_t>(), d_kept.as<ArKept>(), geo.relay_kcap,
                           d_rects.as<ArRect>(), AR_MAX_RECTS, d_counts.as<int32_t>(), d_tctr.as<int32_t>());
        if (hipPeekAtLastError() == hipSuccess) tail_dirty = false;   // k_tail_finish leaves the list lengths at zero
        return ORBFE_OK;
    }
    // the single-walker kernel: images whose bit image does not fit LDS next to the relay kernel's tables, big-frame mode, or forced
    int contours_single_walker(const BatchPlan& p, int B, const uint32_t* cbits, hipStream_t s)
    {
        const int kcap = p.walker_hbm ? AR_MAX_KEPT_BIG : AR_MAX_KEPT, ldsw = p.walker_hbm ? 0 : geo.lds_bits_words;
        const size_t lds = contours_lds_bytes(ldsw, kcap);
        auto kfn = p.walker_hbm ? k_contours_t<false> : k_contours_t<true>;
        if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(kfn), lds)) return rc;
        if (!ORBFE_SKIP_ARUCO(1))
            hipLaunchKernelGGL(kfn, dim3(B), dim3(CT_PROBE_THREADS), lds, s, cbits, geo.bits_fu32, geo.wpr, geo.cols, geo.rows, ldsw, 70, d_candq.as<uint32_t>(),
                               geo.candq_fu32, (int)geo.candq_fu32, d_pool.as<uint32_t>(), geo.pool_fu32, (int)geo.pool_fu32, d_kept.as<ArKept>(), kcap,
                               d_rects.as<ArRect>(), AR_MAX_RECTS, d_counts.as<int32_t>(), d_gpad.as<uint32_t>(), geo.gpad_fu32, 0);
        return ORBFE_OK;
    }
    // prefilterCandidates, then the batch's candidates decoded as one work list: a wave per candidate (persistent: 32 candidates per
    // frame is more than the streams here produce, a busier batch loops), 64 candidates per Otsu wave
    int prefilter_decode(const BatchPlan& p, int B, hipStream_t s, const ImgView& src0, int enlarge_k, bool finish_in_prefilter)
    {
        if (enclosed)   // enlargeMarkerCandidate on every rectangle, before prefilterCandidates sees them (:3560-3590)
            hipLaunchKernelGGL(k_enlarge_candidates, dim3(B), dim3(AR_MAX_RECTS), 0, s, d_rects.as<ArRect>(), AR_MAX_RECTS, d_counts.as<int32_t>(),
                               (int)(float(enlarge_k) / 2.));
        if (decode_dirty) ORBFE_HIP(hipMemsetAsync(d_dctr.p, 0, 4, s));   // a previous batch was abandoned between prefilter and finalize (the counter only: [2], [3] are the sticky flags)
        decode_dirty = true;
        const TailFinish tf = finish_in_prefilter ? TailFinish{geo.relay_kcap, d_trect.as<uint8_t>(), d_kept.as<ArKept>(), geo.relay_kcap, d_tctr.as<int32_t>()} : TailFinish{};
        hipLaunchKernelGGL(k_prefilter, dim3(B), dim3(256), 0, s, d_rects.as<ArRect>(), AR_MAX_RECTS,
                           d_counts.as<int32_t>(), geo.cols, geo.rows, geo.win, d_candidx.as<int32_t>(), d_ncand.as<int32_t>(),
                           d_dwork.as<uint32_t>(), d_dctr.as<int32_t>(), tf);
        if (finish_in_prefilter && hipPeekAtLastError() == hipSuccess) tail_dirty = false;   // (it leaves the tail's list lengths at zero)
        if (!p.nfuse) ORBFE_HIP(hipStreamWaitEvent(s, ev_join, 0));   // the pyramid of the aux stream
        const int max_items = B * AR_MAX_RECTS, wgs = std::max(1, std::min((B * 32 + DC_WAVES - 1) / DC_WAVES, 4096));
        for (int r_ = 0; r_ < ORBFE_REPS_ARUCO(2); r_++) {
            hipLaunchKernelGGL(k_decode_warp, dim3(wgs), dim3(DC_WAVES * 64), 0, s, src0, pyr_view(), d_levels.as<ArLevel>(), geo.npyr,
                               d_rects.as<ArRect>(), AR_MAX_RECTS, d_candidx.as<int32_t>(), S, geo.cols, d_dwork.as<uint32_t>(),
                               d_dctr.as<int32_t>(), d_ditems.as<DcItem>(), d_dhist.as<uint16_t>(), d_dpatch.as<uint8_t>());
            hipLaunchKernelGGL(k_decode_otsu, dim3((max_items + 63) / 64), dim3(64), 0, s, d_dctr.as<int32_t>(), d_ditems.as<DcItem>(),
                               d_dhist.as<uint16_t>(), S);
            hipLaunchKernelGGL(k_decode_vote, dim3(wgs), dim3(DC_WAVES * 64), 0, s, src0, pyr_view(), d_levels.as<ArLevel>(), AR_MAX_RECTS, S, nb,
                               d_codes.as<unsigned long long>(), ncodes, d_scodes.as<unsigned long long>(), d_sids.as<int32_t>(),
                               nsorted, max_corr, d_dwork.as<uint32_t>(), d_dctr.as<int32_t>(), d_ditems.as<DcItem>(),
                               d_dpatch.as<uint8_t>(), d_result.as<int32_t>());
        }
        return ORBFE_OK;
    }
    // the mode runs' histogram and corner upsampling, sort / dedupe into the marker records (k_finalize), cornerSubPix
    int finalize(int B, hipStream_t s, const ImgView& src0, const ModeRun* mr, orbfe_marker* d_out_m, int capacity, int32_t* d_n)
    {
        const bool reduced = mr && mr->d_full;
        if (mr && mr->d_hist)   // the pixels of the accepted candidates: the next frame's threshold is Otsu over them
            hipLaunchKernelGGL(k_marker_hist, dim3(B), dim3(256), 0, s, d_dwork.as<uint32_t>(), d_dctr.as<int32_t>(), d_result.as<int32_t>(),
                               AR_MAX_RECTS, d_dhist.as<uint16_t>(), mr->d_hist);
        if (reduced) {   // cornerUpsample: before sort / dedupe, whose perimeters are those of the upsampled corners
            int start = 0;
            for (int i = 0; i < geo.npyr && geo.cols < geo.levels[i].w; i++) start = i;
            const int wgs = std::max(1, std::min((B * 32 * 4 + 3) / 4, 2048));
            hipLaunchKernelGGL(k_upsample_corners, dim3(wgs), dim3(256), 0, s, src0, pyr_view(), d_levels.as<ArLevel>(), start, geo.cols,
                               d_rects.as<ArRect>(), AR_MAX_RECTS, d_candidx.as<int32_t>(), d_dwork.as<uint32_t>(), d_dctr.as<int32_t>(),
                               d_result.as<int32_t>(), d_masks.as<float>());
        }
        if (int rc = mr && mr->before_finalize ? mr->before_finalize(s) : ORBFE_OK) return rc;
        // corner refinement applies only when the input was not reduced (:8420): CORNER_LINES inside k_finalize, CORNER_SUBPIX after it
        // (a measuring build that repeats the launch counts a flagged frame into the sticky words once per repeat; the shipped build runs it once)
        for (int r_ = 0; r_ < ORBFE_REPS_ARUCO(4); r_++) hipLaunchKernelGGL(k_finalize, dim3(B), dim3(256), 0, s, d_rects.as<ArRect>(), AR_MAX_RECTS,
                           d_candidx.as<int32_t>(), d_ncand.as<int32_t>(), d_result.as<int32_t>(),
                           d_pool.as<uint32_t>(), geo.pool_fu32, d_out_m, capacity, d_n, (corner_method == 1 && !reduced) ? 1 : 0, d_msrc.as<int32_t>(),
                           d_dctr.as<int32_t>(), d_counts.as<int32_t>());
        if (corner_method == 0 && !reduced)   // cornerSubPix(grey, Size(4, 4), TermCriteria(MAX_ITER | EPS, 12, 0.005)) (:8511)
            hipLaunchKernelGGL(k_corner_subpix_markers, dim3(16, B), dim3(256), 0, s, src0, geo.cols, geo.rows, d_out_m, d_n, capacity, 4, 12,
                               0.005 * 0.005, d_masks.as<float>() + (size_t)3 * 17 * 17);
        return ORBFE_OK;
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// Marker pose (reference detect :8720-8780 -> Marker::calculateExtrinsics, and Frame.cc:170): TWO lanes per marker record, one per IPPE
// solution -- both compute the homography and the two rotations (the same instructions on both lanes), then each its own translation,
// reprojection error (Rodrigues with a double sine and cosine, four distorted projections) and rotation vector; the pair exchanges
// seven floats.  The same operations on the same values as one lane doing both; the kernel is one serial chain of double arithmetic
// at the end of the detector's launches, and this takes 40 % off it.  32 markers per 64-thread workgroup.
__global__ __launch_bounds__(64) void k_marker_poses(const orbfe_marker* __restrict__ markers, const int32_t* __restrict__ d_n,
                                                    int capacity, float marker_size, PoseCamera cam,
                                                    orbfe_marker_pose* __restrict__ poses)
{
    const int f = blockIdx.y, lane = threadIdx.x, i = blockIdx.x * 32 + (lane >> 1), which = lane & 1;
    const int n = d_n ? min(d_n[f], capacity) : capacity;
    if (i >= n) return;   // (both lanes of a pair: the exchange below is between lanes of one pair)
    const orbfe_marker m = markers[(size_t)f * capacity + i];
    float e, r[3], t[3];
    pose::solve_marker_half(m.corners, marker_size, cam, which, &e, r, t);
    // the partner's solution
    const float eo = __shfl_xor(e, 1);
    float ro[3], to[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { ro[k] = __shfl_xor(r[k], 1); to[k] = __shfl_xor(t[k], 1); }
    if (which == 0) {
        const bool a_first = e < eo; // ippe.cpp:786 (this lane holds solution a)
        orbfe_marker_pose out;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            out.rvec[k] = a_first ? r[k] : ro[k]; out.tvec[k] = a_first ? t[k] : to[k];
            out.rvec2[k] = a_first ? ro[k] : r[k]; out.tvec2[k] = a_first ? to[k] : t[k];
        }
        out.err[0] = a_first ? e : eo;
        out.err[1] = a_first ? eo : e;
        poses[(size_t)f * capacity + i] = out;
    }
}

static int pose_camera(const float* K4, const float* dist, int ndist, float marker_size, PoseCamera& c, const char* who)
{
    if (!(marker_size > 0.0f)) return fail(ORBFE_ERR_INVALID, "%s: markerSize<=0: invalid markerSize", who); // marker.cpp:328-329
    if (!K4 || ndist < 0 || ndist > 12 || (ndist && !dist) || !(K4[0] != 0.0f) || !(K4[1] != 0.0f))
        return fail(ORBFE_ERR_INVALID, "%s: invalid camera (K = {fx, fy, cx, cy} with fx, fy != 0; at most 12 coefficients)", who);
    c.fx = K4[0]; c.fy = K4[1]; c.cx = K4[2]; c.cy = K4[3];
    for (int i = 0; i < 12; i++) c.k[i] = i < ndist ? (double)dist[i] : 0.0;
    c.has_dist = ndist > 0;
    return ORBFE_OK;
}

static thread_local ThreadWorkspaces<HostStage> tl_host_ws; // orbfe_marker_poses and orbfe_corner_subpix, per (thread, device)

// ---- trackingMinDetections: host logic, as in the reference (it walks two short lists; the device supplies the candidates) ----
namespace {
struct TrackQuad { // marker_analyzer (markerdetector_impl.h:2460-2530): centre, area, inside test
    float c[4][2], cx, cy, area;
    void set(const float q[4][2])
    {
        memcpy(c, q, sizeof c);
        const float a1 = std::fabs((c[1][0] - c[0][0]) * (c[3][1] - c[0][1]) - (c[1][1] - c[0][1]) * (c[3][0] - c[0][0]));
        const float a2 = std::fabs((c[1][0] - c[2][0]) * (c[3][1] - c[2][1]) - (c[1][1] - c[2][1]) * (c[3][0] - c[2][0]));
        area = (a2 + a1) / 2.f;
        float sx = 0, sy = 0;
        for (int k = 0; k < 4; k++) { sx += c[k][0]; sy += c[k][1]; }
        cx = (float)(sx * (1. / 4.)); cy = (float)(sy * (1. / 4.));
    }
    bool is_into(float px, float py) const
    {
        for (int k = 0; k < 4; k++) {
            const float* p1 = c[k];
            const float* p2 = c[(k + 1) % 4];
            const float d = ((p1[1] - p2[1]) * px + (p2[0] - p1[0]) * py + (p1[0] * p2[1] - p2[0] * p1[1])) /
                            std::sqrt((p2[0] - p1[0]) * (p2[0] - p1[0]) + (p2[1] - p1[1]) * (p2[1] - p1[1]));
            if (d < 0) return false;
        }
        return true;
    }
};
// agreement of the first sides' directions (:7700-7760)
float track_side_agreement(const float a[4][2], const float b[4][2])
{
    float ux = a[1][0] - a[0][0], uy = a[1][1] - a[0][1], vx = b[1][0] - b[0][0], vy = b[1][1] - b[0][1];
    const double nu = 1. / std::sqrt((double)ux * ux + (double)uy * uy), nv = 1. / std::sqrt((double)vx * vx + (double)vy * vy);
    ux = (float)(ux * nu); uy = (float)(uy * nu);
    vx = (float)(vx * nv); vy = (float)(vy * nv);
    return ux * vx + uy * vy;
}
} // namespace

// The tracking block of detect() on the decode results of one frame: `ids[slot]` (-1 = rejected) and the candidates' corners.  Adopted
// candidates get the missing marker's id and the corner rotation that best continues its previous orientation (written back as
// the (id, nRot) pair k_finalize understands).  Returns the number of adopted candidates.
static int track_missing_markers(orbfe_aruco* h, int ncand, int32_t* result /* ncand x (id, nRot) */, const float (*corners)[4][2])
{
    auto found = [&](int id) { for (int s = 0; s < ncand; s++) if (result[2 * s] == id) return true; return false; };
    for (auto& mc : h->marker_counts)
        if (!found(mc.first)) mc.second = std::max(mc.second - 1, 0);
    struct Info { TrackQuad q; int best = -1; double dist = std::numeric_limits<double>::max(); const orbfe_marker* prev = nullptr; };
    std::map<int, Info> need;
    for (const orbfe_marker& m : h->prev_markers)
        if (!found(m.id) && h->marker_counts.count(m.id) != 0 && h->marker_counts.at(m.id) >= h->tracking_min && !need.count(m.id)) {
            Info in; in.q.set(m.corners); in.prev = &m;
            need.insert({m.id, in});
        }
    struct Adopt { int slot, id, nrot; };
    std::vector<Adopt> adopt;
    if (!need.empty()) {
        for (int s = 0; s < ncand; s++) {
            if (result[2 * s] >= 0) continue; // only what the dictionary rejected
            TrackQuad qc; qc.set(corners[s]);
            for (auto& kv : need) {
                Info& in = kv.second;
                if (!in.q.is_into(qc.cx, qc.cy)) continue;
                const float dx = in.q.cx - qc.cx, dy = in.q.cy - qc.cy;
                const double dist = std::sqrt((double)dx * dx + (double)dy * dy);
                const float size_diff = std::fabs(in.q.area - qc.area) / in.q.area;
                if (size_diff < 0.3f && dist < in.dist) { in.best = s; in.dist = dist; }
            }
        }
        std::vector<char> used((size_t)std::max(ncand, 1), 0);
        for (auto& kv : need) {
            Info& in = kv.second;
            if (in.best == -1 || used[in.best]) continue; // (a candidate claimed twice: undefined in the reference; the first claim wins)
            int best_r = 0;
            double best_s = -1;
            for (int r = 0; r < 4; r++) {
                float rot[4][2];
                for (int k = 0; k < 4; k++) { rot[k][0] = corners[in.best][(k + r) % 4][0]; rot[k][1] = corners[in.best][(k + r) % 4][1]; }
                const float sc = track_side_agreement(in.prev->corners, rot);
                if (sc > best_s) { best_r = r; best_s = sc; }
            }
            used[in.best] = 1;
            // k_finalize rotates the corners by 4 - nRot: a left rotation by r is nRot = (4 - r) % 4
            adopt.push_back(Adopt{in.best, kv.first, (4 - best_r) % 4});
        }
        for (const Adopt& a : adopt) { result[2 * a.slot] = a.id; result[2 * a.slot + 1] = a.nrot; } // (after the loop: found() above saw the dictionary's results only)
    }
    const int adopted = (int)adopt.size();
    for (int s = 0; s < ncand; s++)
        if (result[2 * s] >= 0) {
            const int id = result[2 * s];
            if (h->marker_counts.count(id) == 0) h->marker_counts[id] = 1;
            else h->marker_counts[id]++;
        }
    return adopted;
}

// The image detect() works on (markerdetector_impl.cpp:5990-6090): with Params::minSize > 0 markers smaller than minSize * max(cols,
// rows) need not be found, so the frame is reduced until such a marker would be lowResMarkerSize = 20 pixels.
static int work_size(const orbfe_aruco* h, int rows, int cols, int* wr, int* wc)
{
    *wr = rows; *wc = cols;
    const int maxdim = std::max(cols, rows);
    const int minpix = (int)(static_cast<float>(h->min_size) * static_cast<float>(maxdim)); // getMinMarkerSizePix, minSize_pix = -1
    if (20 < minpix) {
        const float scale = float(20) / float(minpix);
        if (scale < 0.9) {
            int w = float(cols) * scale + 0.5, hh = float(rows) * scale + 0.5;
            if (w % 2 != 0) w++;
            if (hh % 2 != 0) hh++;
            // cornerUpsample's cornerSubPix window is int(0.5 + 2.5 * width ratio to the pyramid level above): tables up to 8
            if (w < 64 || hh < 48)
                return fail(ORBFE_ERR_INVALID, "minMarkerSize %g reduces a %d x %d frame to %d x %d: working images below 64 x 48 are not supported",
                            (double)h->min_size, cols, rows, w, hh);
            *wr = hh; *wc = w;
        }
    }
    return ORBFE_OK;
}

// a batch on a reduced working image: INTER_NEAREST into the handle's buffer, then the pipeline (mode run `mr`) with the full frames for
// the pyramid, the warps and cornerUpsample
static int reduced_batch(orbfe_aruco* h, const uint8_t* d_imgs, int B, size_t frame_stride, int rows, int cols, size_t step, int wr, int wc,
                         orbfe_marker* d_out, int capacity, int32_t* d_n, hipStream_t s, ModeRun mr = {}, Contours floor = Contours::tiled, Contours* ran = nullptr)
{
    const size_t rpitch = (size_t)(wc + 63) / 64 * 64, rframe = rpitch * wr;
    int rc = h->d_red.ensure(rframe * B + 64);
    if (rc) return rc;
    const double ifx = 1. / ((double)wc / cols), ify = 1. / ((double)wr / rows);
    hipLaunchKernelGGL(k_resize_nearest, dim3((wc + 63) / 64, (wr + 3) / 4, B), dim3(256), 0, s, ImgView{d_imgs, nullptr, frame_stride, (int)step},
                       ImgView{h->d_red.as<uint8_t>(), h->d_red.as<uint8_t>(), rframe, (int)rpitch}, cols, rows, wc, wr, ifx, ify);
    mr.d_full = d_imgs; mr.full_fstride = frame_stride; mr.full_step = step; mr.full_rows = rows; mr.full_cols = cols;
    return h->run_device(h->d_red.as<uint8_t>(), B, rframe, wr, wc, rpitch, d_out, capacity, d_n, s, &mr, floor, ran);
}

// The threshold of the next frame: Otsu's criterion over the normalised float histogram of the detected markers' pixels, every
// split evaluated from scratch in single precision as markerdetector_impl.cpp:6121-6380 does (host logic there as here: 2 x 256 x 255
// additions).  -1: no split has both classes above 1e-4 (an empty histogram turns into NaNs and ends here too).
static int otsu_of_marker_histogram(const uint32_t* counts)
{
    float hist[256], total = 0;
    for (int v = 0; v < 256; v++) { hist[v] = (float)counts[v]; total += hist[v]; } // counts < 2^24: exact, like the reference's ++
    const float inv = 1. / total;
    for (int v = 0; v < 256; v++) hist[v] *= inv;
    float best = 0;
    int best_t = -1;
    for (int t = 1; t < 256; t++) {
        float wlo = 0, whi = 0, mlo = 0, mhi = 0;
        for (int v = 0; v < t; v++) { wlo += hist[v]; mlo += float(v) * hist[v]; }
        for (int v = t; v < 256; v++) { whi += hist[v]; mhi += hist[v] * float(v); }
        if (!(wlo > 1e-4 && whi > 1e-4)) continue;
        mlo /= wlo;
        mhi /= whi;
        const float between = wlo * whi * (mlo - mhi) * (mlo - mhi);
        if (between > best) { best = between; best_t = t; }
    }
    return best_t;
}

extern "C" {

orbfe_aruco* orbfe_aruco_create(const char* dictionary, int device)
{
    if (!dictionary) { fail(ORBFE_ERR_INVALID, "null dictionary name"); return nullptr; }
    if (use_device(device) != ORBFE_OK) return nullptr;
    orbfe_aruco* h = new orbfe_aruco();
    h->device = device;
    read_detector_env(h->sw, [](const char* name) -> const char* { return getenv(name); });   // every ORBFE_ARUCO_* variable, here and nowhere else
    if (hipStreamCreate(&h->own_stream) != hipSuccess ||
        hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess) {
        fail(ORBFE_ERR_HIP, "hipStreamCreate failed");
        delete h;
        return nullptr;
    }
    if (h->set_dictionary(dictionary) != ORBFE_OK) { delete h; return nullptr; }
    return h;
}

void orbfe_aruco_destroy(orbfe_aruco* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->spec.pending) (void)hipStreamSynchronize(h->own_stream); // work started for a paired extractor (unpair before destroying)
    delete h;
}

// A setter that changes what detect() returns ends a speculation started with the old parameters (orbfe_extractor_pair_detector:
// the extractor's call may have run this detector on its frame already): the detector's next call then runs by itself.
static void end_speculation(orbfe_aruco* h)
{
    if (h->spec.pending) { (void)hipStreamSynchronize(h->own_stream); h->spec.pending = false; }
}

int orbfe_aruco_set_dictionary(orbfe_aruco* h, const char* dictionary)
{
    if (!h || !dictionary) return fail(ORBFE_ERR_INVALID, "null argument");
    int rc = use_device(h->device);
    if (rc) return rc;
    end_speculation(h);
    return h->set_dictionary(dictionary);
}

int orbfe_aruco_max_markers(const orbfe_aruco* h) { return h ? AR_MAX_RECTS : ORBFE_ERR_INVALID; }

int orbfe_aruco_set_error_correction_rate(orbfe_aruco* h, float rate)
{
    if (!h || !(rate >= 0.0f && rate <= 1.0f)) return fail(ORBFE_ERR_INVALID, "orbfe_aruco_set_error_correction_rate: rate must be in [0, 1]");
    end_speculation(h);
    h->error_rate = rate;
    h->max_corr = (int)((float)h->tau * rate);
    return ORBFE_OK;
}

int orbfe_aruco_set_detection_mode(orbfe_aruco* h, int mode, float min_marker_size)
{
    if (!h) return fail(ORBFE_ERR_INVALID, "null handle");
    // Params::setDetectionMode (markerdetector.cpp:374-391).  DM_NORMAL = 0: adaptive threshold, C = 7 (Frame.cc:136); DM_FAST = 1:
    // THRES_AUTO_FIXED, the global threshold starts at 100; DM_VIDEO_FAST = 2: the same plus the automatic size estimation with
    // ts = 0.3.  minMarkerSize (Params::minSize, a fraction of the larger image side) > 0 makes detect() work on a reduced frame.
    if (mode < 0 || mode > 2) return fail(ORBFE_ERR_INVALID, "detection mode %d: DM_NORMAL 0, DM_FAST 1, DM_VIDEO_FAST 2", mode);
    if (!(min_marker_size >= 0.0f && min_marker_size <= 1.0f))
        return fail(ORBFE_ERR_INVALID, "minMarkerSize %g: a fraction of the image size in [0, 1]", (double)min_marker_size);
    end_speculation(h);
    h->detect_mode = mode;
    h->min_size = min_marker_size;
    if (mode == 0) { h->auto_size = false; h->ts = 0.25f; h->thres_method = 0; h->thres_value = 7; }
    else if (mode == 1) { h->auto_size = false; h->ts = 0.25f; h->thres_method = 1; h->thres_value = 100; }
    else { h->thres_method = 1; h->thres_value = 100; h->auto_size = true; h->ts = 0.3f; }
    return ORBFE_OK;
}

int orbfe_aruco_set_corner_refinement(orbfe_aruco* h, int method)
{
    if (!h) return fail(ORBFE_ERR_INVALID, "null handle");
    // aruco::CornerRefinementMethod (markerdetector.h:62): CORNER_SUBPIX = 0 (cv::cornerSubPix), CORNER_LINES = 1, CORNER_NONE = 2.
    // Params::setCornerRefinementMethod (markerdetector.cpp:392-395): anything but CORNER_SUBPIX resets minSize to 0.
    if (method < 0 || method > 2) return fail(ORBFE_ERR_INVALID, "corner refinement method %d: CORNER_SUBPIX 0, CORNER_LINES 1, CORNER_NONE 2", method);
    end_speculation(h);
    h->corner_method = method;
    if (method != 0) h->min_size = 0.f;
    return ORBFE_OK;
}

int orbfe_aruco_set_enclosed_markers(orbfe_aruco* h, int on)
{
    if (!h) return fail(ORBFE_ERR_INVALID, "null handle");
    end_speculation(h);
    h->enclosed = on != 0;
    return ORBFE_OK;
}

int orbfe_aruco_set_tracking(orbfe_aruco* h, int min_detections)
{
    if (!h || min_detections < 0) return fail(ORBFE_ERR_INVALID, "orbfe_aruco_set_tracking: trackingMinDetections >= 0");
    end_speculation(h);
    h->tracking_min = min_detections;
    h->marker_counts.clear();
    h->prev_markers.clear();
    h->last_tracked = 0;
    return ORBFE_OK;
}

int orbfe_aruco_last_tracked(const orbfe_aruco* h) { return h ? h->last_tracked : ORBFE_ERR_INVALID; }

int orbfe_aruco_set_gray_conversion(orbfe_aruco* h, int fractional_bits)
{
    if (!h || (fractional_bits != 14 && fractional_bits != 15))
        return fail(ORBFE_ERR_INVALID, "orbfe_aruco_set_gray_conversion: 14 (OpenCV <= 3.4.1) or 15 (3.4.2 and later) fractional bits");
    end_speculation(h);
    h->gray_bits15 = fractional_bits == 15;
    return ORBFE_OK;
}

int orbfe_aruco_get_state(const orbfe_aruco* h, int32_t* threshold, float* min_size, int32_t* attempts, int32_t* work_rows, int32_t* work_cols)
{
    if (!h) return fail(ORBFE_ERR_INVALID, "null handle");
    if (threshold) *threshold = h->thres_value;
    if (min_size) *min_size = h->min_size;
    if (attempts) *attempts = h->last_attempts;
    if (work_rows) *work_rows = h->last_work_rows;
    if (work_cols) *work_cols = h->last_work_cols;
    return ORBFE_OK;
}

int orbfe_aruco_marker_contour(orbfe_aruco* h, int frame, int marker, int32_t* xy, int capacity, int32_t* n)
{
    if (!h || !n || frame < 0 || frame >= h->last_nframes || marker < 0 || marker >= AR_MAX_RECTS || (capacity > 0 && !xy))
        return fail(ORBFE_ERR_INVALID, "orbfe_aruco_marker_contour: invalid argument");
    int rc = use_device(h->device);
    if (rc) return rc;
    ORBFE_HIP(hipDeviceSynchronize());
    int32_t src = -1;
    ORBFE_HIP(hipMemcpy(&src, h->d_msrc.as<int32_t>() + (size_t)frame * AR_MAX_RECTS + marker, 4, hipMemcpyDeviceToHost));
    if (src < 0 || src >= AR_MAX_RECTS) return fail(ORBFE_ERR_INVALID, "orbfe_aruco_marker_contour: no such marker in the last batch");
    ArRect r;
    ORBFE_HIP(hipMemcpy(&r, h->d_rects.as<ArRect>() + (size_t)frame * AR_MAX_RECTS + src, sizeof r, hipMemcpyDeviceToHost));
    *n = r.len;
    const int m = std::min(r.len, capacity);
    if (m > 0) {
        std::vector<uint32_t> p(m);
        ORBFE_HIP(hipMemcpy(p.data(), h->d_pool.as<uint32_t>() + (size_t)frame * h->geo.pool_fu32 + r.off, (size_t)m * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < m; i++) { xy[2 * i] = (int32_t)(p[i] & 0xffff); xy[2 * i + 1] = (int32_t)(p[i] >> 16); }
    }
    return ORBFE_OK;
}

int orbfe_aruco_marker_contours(orbfe_aruco* h, int frame, int nmarkers, int32_t* xy, int capacity, int32_t* offsets)
{
    if (!h || !offsets || frame < 0 || frame >= h->last_nframes || nmarkers < 0 || nmarkers > AR_MAX_RECTS || (capacity > 0 && !xy))
        return fail(ORBFE_ERR_INVALID, "orbfe_aruco_marker_contours: invalid argument");
    int rc = use_device(h->device);
    if (rc) return rc;
    offsets[0] = 0;
    if (nmarkers == 0) return ORBFE_OK;
    ORBFE_HIP(hipDeviceSynchronize());
    std::vector<int32_t> src((size_t)nmarkers);
    std::vector<ArRect> rects(AR_MAX_RECTS);
    ORBFE_HIP(hipMemcpy(src.data(), h->d_msrc.as<int32_t>() + (size_t)frame * AR_MAX_RECTS, (size_t)nmarkers * 4, hipMemcpyDeviceToHost));
    ORBFE_HIP(hipMemcpy(rects.data(), h->d_rects.as<ArRect>() + (size_t)frame * AR_MAX_RECTS, sizeof(ArRect) * AR_MAX_RECTS, hipMemcpyDeviceToHost));
    // the borders of a frame's markers lie in one pool: fetch the span that covers them once, then cut it up
    uint32_t lo = ~0u, hi = 0;
    for (int i = 0; i < nmarkers; i++) {
        if (src[i] < 0 || src[i] >= AR_MAX_RECTS) return fail(ORBFE_ERR_INVALID, "orbfe_aruco_marker_contours: no marker %d in the last batch", i);
        const ArRect& r = rects[(size_t)src[i]];
        offsets[i + 1] = offsets[i] + r.len;
        if (r.len > 0) { lo = std::min(lo, (uint32_t)r.off); hi = std::max(hi, (uint32_t)(r.off + r.len)); }
    }
    if (offsets[nmarkers] > capacity || hi <= lo) return ORBFE_OK; // the caller reads the total from offsets and comes back with room
    std::vector<uint32_t> p((size_t)(hi - lo));
    ORBFE_HIP(hipMemcpy(p.data(), h->d_pool.as<uint32_t>() + (size_t)frame * h->geo.pool_fu32 + lo, p.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < nmarkers; i++) {
        const ArRect& r = rects[(size_t)src[i]];
        int32_t* o = xy + 2 * (size_t)offsets[i];
        for (int k = 0; k < r.len; k++) { const uint32_t v = p[(size_t)(r.off - lo) + k]; o[2 * k] = (int32_t)(v & 0xffff); o[2 * k + 1] = (int32_t)(v >> 16); }
    }
    return ORBFE_OK;
}

int orbfe_aruco_detect_batch_device(orbfe_aruco* h, const uint8_t* d_imgs, int nframes, size_t frame_stride, int rows,
                                    int cols, size_t step, orbfe_marker* d_out, int capacity, int32_t* d_n_out,
                                    void* stream)
{
    if (!h || !d_imgs || !d_out || !d_n_out || nframes <= 0 || rows <= 0 || cols <= 0 || capacity <= 0)
        return fail(ORBFE_ERR_INVALID, "orbfe_aruco_detect_batch_device: invalid argument");
    char why[192];   // level 0 is read from the caller's buffer as it lies: what the kernels' offsets cannot address is refused here
    if (plan_input_layout(rows, cols, step, frame_stride, nframes, why, sizeof(why))) return fail(ORBFE_ERR_INVALID, "orbfe_aruco_detect_batch_device: %s", why);
    int rc = use_device(h->device);
    if (rc) return rc;
    if (h->spec.pending) { ORBFE_HIP(hipStreamSynchronize(h->own_stream)); h->spec.pending = false; } // the handle's buffers are in use
    // THRES_AUTO_FIXED and the automatic size estimation carry state from one frame to the next and decide on the host (retry with
    // a random threshold): frames must go one at a time through the host-pointer entry points
    if (h->stateful())
        return fail(ORBFE_ERR_INVALID, "orbfe_aruco_detect_batch_device: DM_FAST / DM_VIDEO_FAST are frame-sequential (use orbfe_aruco_detect)");
    int wr, wc;
    if ((rc = work_size(h, rows, cols, &wr, &wc))) return rc;
    if (wc != cols) return reduced_batch(h, d_imgs, nframes, frame_stride, rows, cols, step, wr, wc, d_out, capacity, d_n_out, (hipStream_t)stream);
    return h->run_device(d_imgs, nframes, frame_stride, rows, cols, step, d_out, capacity, d_n_out, (hipStream_t)stream);
}

} // extern "C"

// staging layout of a one-frame host call (page-locked): [frame in] [n] [counts x 4] [marker records] [poses]
struct DetOffsets { size_t n, cnt, mk, ps, end; };
static DetOffsets det_offsets(size_t dframe, int nframes, bool with_pose)
{
    DetOffsets o;
    o.n = (dframe * nframes + 255) / 256 * 256;
    o.cnt = o.n + ((size_t)nframes * 4 + 63) / 64 * 64;
    o.mk = o.cnt + ((size_t)nframes * 16 + 63) / 64 * 64;
    o.ps = o.mk + (size_t)AR_MAX_RECTS * nframes * sizeof(orbfe_marker);
    o.end = o.ps + (with_pose ? (size_t)AR_MAX_RECTS * nframes * sizeof(orbfe_marker_pose) : 0);
    return o;
}

static bool same_camera(const PoseCamera& a, const PoseCamera& b) { return memcmp(&a, &b, sizeof(PoseCamera)) == 0; }

namespace orbfe {

// is `img` byte for byte the frame the paired extractor staged?
static bool same_frame(const uint8_t* img, size_t step, const uint8_t* copy, size_t pitch, int rows, int cols)
{
    if (!copy) return false;
    for (int y = 0; y < rows; y++)
        if (memcmp(img + (size_t)y * step, copy + (size_t)y * pitch, (size_t)cols) != 0) return false;
    return true;
}

int aruco_speculate(orbfe_aruco* h, const uint8_t* d_img, size_t dframe, int rows, int cols, size_t dpitch, hipEvent_t uploaded,
                    const uint8_t* host_copy, size_t host_pitch)
{
    h->spec.pending = false;
    if (h->sw.big_mode) return ORBFE_OK; // the rare big-frame mode is left to the detector's own call
    if (h->stateful() || h->min_size > 0.f) return ORBFE_OK; // frame-sequential modes (aruco_modes.hip): the detector's own call too
    int rc;
    if ((rc = h->d_out.ensure((size_t)AR_MAX_RECTS * sizeof(orbfe_marker))) || (rc = h->d_nout.ensure(4))) return rc;
    const bool pose = h->last_cam_valid;
    const DetOffsets o = det_offsets(dframe, 1, true);
    if ((rc = h->pinned.ensure(o.end)) || (rc = h->d_poses.ensure((size_t)AR_MAX_RECTS * sizeof(orbfe_marker_pose)))) return rc;
    uint8_t* hp = h->pinned.as<uint8_t>();
    hipStream_t s = h->own_stream;
    ORBFE_HIP(hipStreamWaitEvent(s, uploaded, 0));
    if ((rc = h->run_device(d_img, 1, dframe, rows, cols, dpitch, h->d_out.as<orbfe_marker>(), AR_MAX_RECTS, h->d_nout.as<int32_t>(), s))) return rc;
    OutPack op;   // (one launch for the call's results: orbfe_common.hpp)
    op.add(hp + o.n, h->d_nout.p, 4);
    op.add(hp + o.cnt, h->d_counts.p, 16);
    op.add(hp + o.mk, h->d_out.p, (size_t)AR_MAX_RECTS * sizeof(orbfe_marker));
    if (pose) {
        hipLaunchKernelGGL(k_marker_poses, dim3((AR_MAX_RECTS + 31) / 32, 1), dim3(64), 0, s, h->d_out.as<orbfe_marker>(), h->d_nout.as<int32_t>(),
                           AR_MAX_RECTS, h->last_size, h->last_cam, h->d_poses.as<orbfe_marker_pose>());
        op.add(hp + o.ps, h->d_poses.p, (size_t)AR_MAX_RECTS * sizeof(orbfe_marker_pose));
    }
    if ((rc = op.flush<1>(s))) return rc;
    h->spec.pending = true; h->spec.rows = rows; h->spec.cols = cols; h->spec.host_copy = host_copy; h->spec.host_pitch = host_pitch;
    h->spec.has_pose = pose; h->spec.cam = h->last_cam; h->spec.size = h->last_size;
    return ORBFE_OK;
}

void aruco_speculation_wait(orbfe_aruco* h)
{
    if (h && h->spec.pending) { (void)hipStreamSynchronize(h->own_stream); h->spec.pending = false; }
}

void aruco_unpair_notice(orbfe_aruco* h)
{
    if (h) h->spec.pending = false;
}

int aruco_device_of(const orbfe_aruco* h) { return h ? h->device : -1; }

int aruco_flags_since_read(orbfe_aruco* h, int32_t* nflagged, int32_t* flags_or)
{
    *nflagged = 0; *flags_or = 0;
    if (!h || !h->d_dctr.p) return ORBFE_OK; // no batch yet
    int rc = use_device(h->device);
    if (rc) return rc;
    ORBFE_HIP(hipDeviceSynchronize());
    int32_t w[2] = {0, 0};
    ORBFE_HIP(hipMemcpy(w, h->d_dctr.as<int32_t>() + 2, 8, hipMemcpyDeviceToHost));
    if (w[0] || w[1]) ORBFE_HIP(hipMemset(h->d_dctr.as<int32_t>() + 2, 0, 8)); // sticky until read
    *nflagged = w[0]; *flags_or = w[1];
    return ORBFE_OK;
}


} // namespace orbfe

// The modes whose frames go one at a time (THRES_AUTO_FIXED and the automatic size estimation carry state from frame to frame and
// decide on the host; a reduced working image or a BGR frame just take this path too): upload, BGR -> grey, the pipeline -- again
// with a random threshold when nothing was found (markerdetector_impl.cpp:6903-6990; rand() is the process's own sequence, as in
// the reference) --, the next frame's threshold and minimum size (:7003-7040, :8790-8880), the poses.
static int detect_frames_modes(orbfe_aruco* h, const uint8_t* imgs, int nframes, size_t frame_stride, int rows, int cols, size_t step,
                               int channels, orbfe_marker* out, int capacity, int32_t* n_out, const PoseCamera* cam, float marker_size,
                               orbfe_marker_pose* poses_out)
{
    int rc;
    if (h->spec.pending) { ORBFE_HIP(hipStreamSynchronize(h->own_stream)); h->spec.pending = false; }
    const size_t dpitch = (size_t)(cols + 63) / 64 * 64, dframe = dpitch * rows;
    const size_t in_bytes = channels == 3 ? (size_t)cols * 3 * rows : dframe;
    // page-locked: [frame in] [n | counts | histogram | markers | poses] out
    const size_t o_n = (in_bytes + 255) / 256 * 256, o_cnt = o_n + 64, o_h = o_cnt + 64, o_mk = o_h + 1024,
                 o_ps = o_mk + (size_t)AR_MAX_RECTS * sizeof(orbfe_marker), o_tk = o_ps + (size_t)AR_MAX_RECTS * sizeof(orbfe_marker_pose),
                 o_tci = o_tk + 64, o_trc = o_tci + (size_t)AR_MAX_RECTS * 4, o_trs = o_trc + (size_t)AR_MAX_RECTS * sizeof(ArRect),
                 o_end = o_trs + (size_t)AR_MAX_RECTS * 8; // trackingMinDetections: candidate count, indices, rectangles, decode results
    if ((rc = h->pinned.ensure(o_end)) || (rc = h->d_in.ensure(dframe + 64)) || (rc = h->d_out.ensure((size_t)AR_MAX_RECTS * sizeof(orbfe_marker))) ||
        (rc = h->d_nout.ensure(4)) || (rc = h->d_mhist.ensure(1024)) || (cam && (rc = h->d_poses.ensure((size_t)AR_MAX_RECTS * sizeof(orbfe_marker_pose)))) ||
        (channels == 3 && (rc = h->d_bgr.ensure(in_bytes + 64))))
        return rc;
    uint8_t* hp = h->pinned.as<uint8_t>();
    hipStream_t s = h->own_stream;
    const int32_t* counts = reinterpret_cast<const int32_t*>(hp + o_cnt);
    const int32_t* np = reinterpret_cast<const int32_t*>(hp + o_n);
    const orbfe_marker* mk = reinterpret_cast<const orbfe_marker*>(hp + o_mk);
    for (int f = 0; f < nframes; f++) {
        const uint8_t* img = imgs + (size_t)f * frame_stride;
        if (channels == 3) {
            for (int y = 0; y < rows; y++) memcpy(hp + (size_t)y * cols * 3, img + (size_t)y * step, (size_t)cols * 3);
            ORBFE_HIP(hipMemcpyAsync(h->d_bgr.p, hp, in_bytes, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_bgr_to_gray, dim3((cols + 63) / 64, (rows + 3) / 4, 1), dim3(256), 0, s, h->d_bgr.as<uint8_t>(), (size_t)0, (size_t)cols * 3,
                               ImgView{h->d_in.as<uint8_t>(), h->d_in.as<uint8_t>(), dframe, (int)dpitch}, cols, rows, h->gray_bits15);
        } else {
            for (int y = 0; y < rows; y++) memcpy(hp + (size_t)y * dpitch, img + (size_t)y * step, (size_t)cols);
            ORBFE_HIP(hipMemcpyAsync(h->d_in.p, hp, dframe, hipMemcpyHostToDevice, s));
        }
        int wr, wc;
        if ((rc = work_size(h, rows, cols, &wr, &wc))) return rc;
        h->last_work_rows = wr; h->last_work_cols = wc;
        int attempts = 0;
        h->last_attempts = 0;
        h->last_tracked = 0;
        // trackingMinDetections (:7107-7890): between the dictionary's verdicts and sort / dedupe the host looks at the frame's
        // candidates (2 KB of results, 10 KB of rectangles) and may hand a rejected one the id of a marker that has gone missing
        int pre_detected = -1;
        const std::map<int, int> counts_at_start = h->marker_counts;
        std::function<int(hipStream_t)> track_hook;
        if (h->tracking_min > 0)
            track_hook = [&](hipStream_t st) -> int {
                ORBFE_HIP(hipMemcpyAsync(hp + o_tk, h->d_ncand.p, 4, hipMemcpyDeviceToHost, st));
                ORBFE_HIP(hipMemcpyAsync(hp + o_tci, h->d_candidx.p, (size_t)AR_MAX_RECTS * 4, hipMemcpyDeviceToHost, st));
                ORBFE_HIP(hipMemcpyAsync(hp + o_trc, h->d_rects.p, (size_t)AR_MAX_RECTS * sizeof(ArRect), hipMemcpyDeviceToHost, st));
                ORBFE_HIP(hipMemcpyAsync(hp + o_trs, h->d_result.p, (size_t)AR_MAX_RECTS * 8, hipMemcpyDeviceToHost, st));
                ORBFE_HIP(hipStreamSynchronize(st));
                const int ncand = std::min(*reinterpret_cast<const int32_t*>(hp + o_tk), (int32_t)AR_MAX_RECTS);
                const int32_t* cidx = reinterpret_cast<const int32_t*>(hp + o_tci);
                const ArRect* rc_ = reinterpret_cast<const ArRect*>(hp + o_trc);
                int32_t* res = reinterpret_cast<int32_t*>(hp + o_trs);
                pre_detected = 0;
                for (int q = 0; q < ncand; q++) pre_detected += res[2 * q] >= 0;
                // a pass that will be repeated with another threshold: the tracking block runs once, after the last pass
                if (pre_detected == 0 && h->thres_method == 1 && attempts + 1 < h->n_attempts_auto_fix) return ORBFE_OK;
                h->marker_counts = counts_at_start;
                std::vector<std::array<std::array<float, 2>, 4>> cs((size_t)std::max(ncand, 1));
                for (int q = 0; q < ncand; q++) memcpy(&cs[q], rc_[cidx[q]].c, sizeof(float) * 8);
                h->last_tracked = track_missing_markers(h, ncand, res, reinterpret_cast<const float (*)[4][2]>(cs.data()));
                if (h->last_tracked) ORBFE_HIP(hipMemcpyAsync(h->d_result.p, res, (size_t)AR_MAX_RECTS * 8, hipMemcpyHostToDevice, st));
                return ORBFE_OK;
            };
        for (;;) {
            h->last_attempts++;
            ModeRun mr;   // THRES_AUTO_FIXED: the carried-over threshold and the histogram of the markers found with it
            mr.fixed_thr = h->thres_method == 1 ? h->thres_value : -1; mr.d_hist = h->thres_method == 1 ? h->d_mhist.as<uint32_t>() : nullptr; mr.before_finalize = track_hook;
            rc = h->with_retries([&](Contours floor, Contours* ran) -> int {
                if (int e = wc != cols ? reduced_batch(h, h->d_in.as<uint8_t>(), 1, dframe, rows, cols, dpitch, wr, wc, h->d_out.as<orbfe_marker>(),
                                                       AR_MAX_RECTS, h->d_nout.as<int32_t>(), s, mr, floor, ran)
                                       : h->run_device(h->d_in.as<uint8_t>(), 1, dframe, rows, cols, dpitch, h->d_out.as<orbfe_marker>(), AR_MAX_RECTS,
                                                       h->d_nout.as<int32_t>(), s, &mr, floor, ran))
                    return e;
                ORBFE_HIP(hipMemcpyAsync(hp + o_n, h->d_nout.p, 4, hipMemcpyDeviceToHost, s));
                ORBFE_HIP(hipMemcpyAsync(hp + o_cnt, h->d_counts.p, 16, hipMemcpyDeviceToHost, s));
                if (mr.d_hist) ORBFE_HIP(hipMemcpyAsync(hp + o_h, mr.d_hist, 1024, hipMemcpyDeviceToHost, s));
                ORBFE_HIP(hipMemcpyAsync(hp + o_mk, h->d_out.p, (size_t)AR_MAX_RECTS * sizeof(orbfe_marker), hipMemcpyDeviceToHost, s));
                return ORBFE_OK;
            }, counts, 1);
            if (rc) return rc;
            if (counts[2]) return fail(ORBFE_ERR_CAPACITY, "frame %d: internal detector capacity exceeded (flags 0x%x)", f, counts[2]);
            // (the retry is decided on what the dictionary found, before the tracking block adds anything: :6903)
            if ((h->tracking_min > 0 ? pre_detected : np[0]) == 0 && h->thres_method == 1 && ++attempts < h->n_attempts_auto_fix) {
                h->thres_value = 10 + rand() % 230;
                continue;
            }
            break;
        }
        const int n = np[0];
        if (h->thres_method == 1) {
            const int t = otsu_of_marker_histogram(reinterpret_cast<const uint32_t*>(hp + o_h));
            if (t > 0) h->thres_value = t;
        }
        // the smallest marker of this frame sets the minimum size the next frame looks for (:8790-8880)
        float shortest = std::numeric_limits<float>::max();
        for (int i = 0; i < n && i < AR_MAX_RECTS; i++) {
            float per = 0;
            for (int c = 0; c < 4; c++) {
                const float dx = mk[i].corners[c][0] - mk[i].corners[(c + 1) % 4][0], dy = mk[i].corners[c][1] - mk[i].corners[(c + 1) % 4][1];
                per += std::sqrt((double)dx * dx + (double)dy * dy);
            }
            if (shortest > per) shortest = per;
        }
        const float marker_min = shortest != std::numeric_limits<float>::max() ? shortest / (4 * std::max(cols, rows)) : 0.f;
        if (h->auto_size) h->min_size = marker_min * (1 - h->ts);
        if (h->tracking_min > 0) h->prev_markers.assign(mk, mk + std::min(n, (int)AR_MAX_RECTS));
        n_out[f] = n;
        if (n > capacity) return fail(ORBFE_ERR_CAPACITY, "frame %d has %d markers, capacity is %d", f, n, capacity);
        if (n) memcpy(out + (size_t)f * capacity, mk, (size_t)n * sizeof(orbfe_marker));
        if (n && cam) {
            hipLaunchKernelGGL(k_marker_poses, dim3((AR_MAX_RECTS + 31) / 32, 1), dim3(64), 0, s, h->d_out.as<orbfe_marker>(), h->d_nout.as<int32_t>(),
                               AR_MAX_RECTS, marker_size, *cam, h->d_poses.as<orbfe_marker_pose>());
            ORBFE_HIP(hipMemcpyAsync(hp + o_ps, h->d_poses.p, (size_t)n * sizeof(orbfe_marker_pose), hipMemcpyDeviceToHost, s));
            ORBFE_HIP(hipStreamSynchronize(s));
            memcpy(poses_out + (size_t)f * capacity, hp + o_ps, (size_t)n * sizeof(orbfe_marker_pose));
        }
    }
    return ORBFE_OK;
}

// detect (+ the IPPE pose of every marker when a camera is given: one call, one wait, instead of a detect call and a pose call)
static int detect_batch_impl(orbfe_aruco* h, const uint8_t* imgs, int nframes, size_t frame_stride, int rows, int cols,
                             size_t step, orbfe_marker* out, int capacity, int32_t* n_out, const PoseCamera* cam, float marker_size,
                             orbfe_marker_pose* poses_out, int channels = 1)
{
    if (!h || !n_out) return fail(ORBFE_ERR_INVALID, "orbfe_aruco_detect_batch: null argument");
    if (!imgs || rows <= 0 || cols <= 0 || nframes <= 0) {
        for (int f = 0; f < nframes; f++) n_out[f] = 0;
        return ORBFE_OK;
    }
    if (!out || step < (size_t)cols * channels || capacity <= 0) return fail(ORBFE_ERR_INVALID, "orbfe_aruco_detect_batch: invalid argument");
    int rc = use_device(h->device);
    if (rc) return rc;
    {
        int wr, wc;
        if ((rc = work_size(h, rows, cols, &wr, &wc))) return rc;
        if (h->stateful() || wc != cols || channels == 3)
            return detect_frames_modes(h, imgs, nframes, frame_stride, rows, cols, step, channels, out, capacity, n_out, cam, marker_size, poses_out);
        h->last_attempts = 1; h->last_work_rows = rows; h->last_work_cols = cols;
    }
    const size_t dpitch = (size_t)(cols + 63) / 64 * 64, dframe = dpitch * rows;
    if (cam) { h->last_cam = *cam; h->last_size = marker_size; h->last_cam_valid = true; } // what a paired extractor's speculation assumes
    // A paired extractor has started this detector on the image it was given (aruco_speculate): if this call is handed the same
    // image, the work is done or under way on the device -- wait for it and take the results (and the poses, when the camera is the
    // one of the last call); anything else -- another image, a capacity flag -- and the call runs as if nothing had happened.
    if (h->spec.pending && nframes != 1) { ORBFE_HIP(hipStreamSynchronize(h->own_stream)); h->spec.pending = false; }
    if (h->spec.pending && nframes == 1) {
        h->spec.pending = false;
        const bool match = h->spec.rows == rows && h->spec.cols == cols && same_frame(imgs, step, h->spec.host_copy, h->spec.host_pitch, rows, cols);
        hipStream_t s = h->own_stream;
        if (!match) ORBFE_HIP(hipStreamSynchronize(s)); // its buffers are about to be reused
        else {
            const DetOffsets o = det_offsets(dframe, 1, true);
            uint8_t* hp = h->pinned.as<uint8_t>();
            const bool pose_ready = cam && h->spec.has_pose && h->spec.size == marker_size && same_camera(h->spec.cam, *cam);
            if (cam && !pose_ready) { // same markers, another camera: only the poses are still to do
                hipLaunchKernelGGL(k_marker_poses, dim3((AR_MAX_RECTS + 31) / 32, 1), dim3(64), 0, s, h->d_out.as<orbfe_marker>(),
                                   h->d_nout.as<int32_t>(), AR_MAX_RECTS, marker_size, *cam, h->d_poses.as<orbfe_marker_pose>());
                ORBFE_HIP(hipMemcpyAsync(hp + o.ps, h->d_poses.p, (size_t)AR_MAX_RECTS * sizeof(orbfe_marker_pose), hipMemcpyDeviceToHost, s));
            }
            ORBFE_HIP(hipStreamSynchronize(s));
            const int32_t* counts = reinterpret_cast<const int32_t*>(hp + o.cnt);
            const int32_t n = *reinterpret_cast<const int32_t*>(hp + o.n);
            if (!counts[2] && n <= capacity) { // no capacity flag: the speculated run is the result
                n_out[0] = n;
                if (n) memcpy(out, hp + o.mk, (size_t)n * sizeof(orbfe_marker));
                if (n && cam) memcpy(poses_out, hp + o.ps, (size_t)n * sizeof(orbfe_marker_pose));
                return ORBFE_OK;
            }
        }
    }
    if ((rc = h->d_in.ensure(dframe * nframes + 64)) || (rc = h->d_out.ensure((size_t)AR_MAX_RECTS * nframes * sizeof(orbfe_marker))) ||
        (rc = h->d_nout.ensure((size_t)nframes * 4)))
        return rc;
    // page-locked staging: [frames in] then [n per frame | counts (4 per frame) | marker records] out -- three copies queued behind
    // the kernels and one wait instead of a blocking copy per array
    const DetOffsets o_ = det_offsets(dframe, nframes, cam != nullptr);
    const size_t o_n = o_.n, o_cnt = o_.cnt, o_mk = o_.mk, o_ps = o_.ps, o_end = o_.end;
    if ((rc = h->pinned.ensure(o_end))) return rc;
    if (cam && (rc = h->d_poses.ensure((size_t)AR_MAX_RECTS * nframes * sizeof(orbfe_marker_pose)))) return rc;
    uint8_t* hp = h->pinned.as<uint8_t>();
    hipStream_t s = h->own_stream;
    for (int f = 0; f < nframes; f++)
        for (int y = 0; y < rows; y++) memcpy(hp + f * dframe + (size_t)y * dpitch, imgs + f * frame_stride + (size_t)y * step, (size_t)cols);
    ORBFE_HIP(hipMemcpyAsync(h->d_in.p, hp, dframe * nframes, hipMemcpyHostToDevice, s));
    const int32_t* counts = reinterpret_cast<const int32_t*>(hp + o_cnt);
    // a frame with more segments than the tiled path's lists hold: the batch is done again by the relay kernels; one with more kept
    // borders (or border points) than those hold: by the single-walker kernel with its tables sized for AR_MAX_KEPT_BIG
    rc = h->with_retries([&](Contours floor, Contours* ran) -> int {
        if (int e = h->run_device(h->d_in.as<uint8_t>(), nframes, dframe, rows, cols, dpitch, h->d_out.as<orbfe_marker>(),
                                  AR_MAX_RECTS, h->d_nout.as<int32_t>(), s, nullptr, floor, ran))
            return e;
        if (cam)
            hipLaunchKernelGGL(k_marker_poses, dim3((AR_MAX_RECTS + 31) / 32, nframes), dim3(64), 0, s, h->d_out.as<orbfe_marker>(),
                               h->d_nout.as<int32_t>(), AR_MAX_RECTS, marker_size, *cam, h->d_poses.as<orbfe_marker_pose>());
        if (nframes <= 16) {   // a frame or a few: the results in one launch that writes the staging buffer (OutPack, orbfe_common.hpp)
            OutPack op;
            op.add(hp + o_n, h->d_nout.p, (size_t)nframes * 4);
            op.add(hp + o_cnt, h->d_counts.p, (size_t)nframes * 16);
            op.add(hp + o_mk, h->d_out.p, (size_t)AR_MAX_RECTS * nframes * sizeof(orbfe_marker));
            if (cam) op.add(hp + o_ps, h->d_poses.p, (size_t)AR_MAX_RECTS * nframes * sizeof(orbfe_marker_pose));
            if (int e = op.flush<2>(s)) return e;
        } else {
            ORBFE_HIP(hipMemcpyAsync(hp + o_n, h->d_nout.p, (size_t)nframes * 4, hipMemcpyDeviceToHost, s));
            ORBFE_HIP(hipMemcpyAsync(hp + o_cnt, h->d_counts.p, (size_t)nframes * 16, hipMemcpyDeviceToHost, s));
            ORBFE_HIP(hipMemcpyAsync(hp + o_mk, h->d_out.p, (size_t)AR_MAX_RECTS * nframes * sizeof(orbfe_marker), hipMemcpyDeviceToHost, s));
            if (cam) ORBFE_HIP(hipMemcpyAsync(hp + o_ps, h->d_poses.p, (size_t)AR_MAX_RECTS * nframes * sizeof(orbfe_marker_pose), hipMemcpyDeviceToHost, s));
        }
        return ORBFE_OK;
    }, counts, nframes);
    if (rc) return rc;
    memcpy(n_out, hp + o_n, (size_t)nframes * 4);
    for (int f = 0; f < nframes; f++) {
        if (counts[f * 4 + 2])
            return fail(ORBFE_ERR_CAPACITY, "frame %d: internal detector capacity exceeded (flags 0x%x)", f, counts[f * 4 + 2]);
        if (n_out[f] > capacity) return fail(ORBFE_ERR_CAPACITY, "frame %d has %d markers, capacity is %d", f, n_out[f], capacity);
        if (n_out[f])
            memcpy(out + (size_t)f * capacity, hp + o_mk + (size_t)f * AR_MAX_RECTS * sizeof(orbfe_marker), (size_t)n_out[f] * sizeof(orbfe_marker));
        if (n_out[f] && cam)
            memcpy(poses_out + (size_t)f * capacity, hp + o_ps + (size_t)f * AR_MAX_RECTS * sizeof(orbfe_marker_pose),
                   (size_t)n_out[f] * sizeof(orbfe_marker_pose));
    }
    return ORBFE_OK;
}

extern "C" {

int orbfe_aruco_detect_batch(orbfe_aruco* h, const uint8_t* imgs, int nframes, size_t frame_stride, int rows, int cols,
                             size_t step, orbfe_marker* out, int capacity, int32_t* n_out)
{
    return detect_batch_impl(h, imgs, nframes, frame_stride, rows, cols, step, out, capacity, n_out, nullptr, 0.f, nullptr);
}

int orbfe_aruco_detect_poses(orbfe_aruco* h, const uint8_t* img, int rows, int cols, size_t step, orbfe_marker* out,
                             orbfe_marker_pose* poses, int capacity, int32_t* n_out, float marker_size, const float* K4,
                             const float* dist, int ndist)
{
    if (!poses) return fail(ORBFE_ERR_INVALID, "orbfe_aruco_detect_poses: null argument");
    PoseCamera c;
    int rc = pose_camera(K4, dist, ndist, marker_size, c, "orbfe_aruco_detect_poses");
    if (rc) return rc;
    return detect_batch_impl(h, img, 1, 0, rows, cols, step, out, capacity, n_out, &c, marker_size, poses);
}

int orbfe_aruco_detect(orbfe_aruco* h, const uint8_t* img, int rows, int cols, size_t step, orbfe_marker* out,
                       int capacity, int32_t* n_out)
{
    return orbfe_aruco_detect_batch(h, img, 1, 0, rows, cols, step, out, capacity, n_out);
}

int orbfe_aruco_detect_bgr(orbfe_aruco* h, const uint8_t* bgr, int rows, int cols, size_t step, orbfe_marker* out, int capacity, int32_t* n_out)
{
    return detect_batch_impl(h, bgr, 1, 0, rows, cols, step, out, capacity, n_out, nullptr, 0.f, nullptr, 3);
}

int orbfe_aruco_detect_poses_bgr(orbfe_aruco* h, const uint8_t* bgr, int rows, int cols, size_t step, orbfe_marker* out,
                                 orbfe_marker_pose* poses, int capacity, int32_t* n_out, float marker_size, const float* K4,
                                 const float* dist, int ndist)
{
    if (!poses) return fail(ORBFE_ERR_INVALID, "orbfe_aruco_detect_poses_bgr: null argument");
    PoseCamera c;
    int rc = pose_camera(K4, dist, ndist, marker_size, c, "orbfe_aruco_detect_poses_bgr");
    if (rc) return rc;
    return detect_batch_impl(h, bgr, 1, 0, rows, cols, step, out, capacity, n_out, &c, marker_size, poses, 3);
}

int orbfe_corner_subpix(const uint8_t* img, int rows, int cols, size_t step, float* pts, int n, int win, int max_iters, double eps, int device)
{
    if (!img || rows <= 0 || cols <= 0 || step < (size_t)cols || n < 0 || (n && !pts) || win < 1 || win > 8 || max_iters < 1 || !(eps >= 0.0))
        return fail(ORBFE_ERR_INVALID, "orbfe_corner_subpix: invalid argument (window half size 1 .. 8, max_iters >= 1, eps >= 0)");
    if (n == 0) return ORBFE_OK;
    int rc = use_device(device);
    if (rc) return rc;
    // the markers kernel without a detector: the corners as n / 4 "markers" (padded with the first corner), one frame
    const int nm = (n + 3) / 4;
    const size_t pitch = (size_t)(cols + 63) / 64 * 64;
    HostStage& w = tl_host_ws.get();
    IoLayout l;
    const size_t i_img = l.take(pitch * rows + 64), i_mask = l.take(17 * 17 * 4), i_n = l.take(4);
    l.inout();
    const size_t io_mk = l.take((size_t)nm * sizeof(orbfe_marker));
    l.outputs();
    if ((rc = w.begin(l))) return rc;
    for (int y = 0; y < rows; y++) w.put(i_img + (size_t)y * pitch, img + (size_t)y * step, (size_t)cols);
    subpix_window(win, w.host<float>(i_mask));
    w.put(i_n, &nm, 4);
    orbfe_marker* mk = w.host<orbfe_marker>(io_mk);
    memset(mk, 0, (size_t)nm * sizeof(orbfe_marker));
    for (int i = 0; i < 4 * nm; i++) { const int s = i < n ? i : 0; mk[i >> 2].corners[i & 3][0] = pts[2 * s]; mk[i >> 2].corners[i & 3][1] = pts[2 * s + 1]; }
    if ((rc = w.upload())) return rc;
    hipLaunchKernelGGL(k_corner_subpix_markers, dim3(std::max(1, std::min(nm, 256)), 1), dim3(256), 0, w.stream,
                       ImgView{w.dev<uint8_t>(i_img), nullptr, 0, (int)pitch}, cols, rows, w.dev<orbfe_marker>(io_mk), w.dev<int32_t>(i_n), nm, win,
                       std::min(max_iters, 100), eps * eps, w.dev<float>(i_mask));
    ORBFE_HIP(hipGetLastError());
    if ((rc = w.download()) || (rc = w.sync())) return rc;
    for (int i = 0; i < n; i++) { pts[2 * i] = mk[i >> 2].corners[i & 3][0]; pts[2 * i + 1] = mk[i >> 2].corners[i & 3][1]; }
    return ORBFE_OK;
}

int orbfe_aruco_debug_image(orbfe_aruco* h, int frame, int stage, uint8_t* out)
{
    if (!h || !out || frame < 0 || frame >= h->last_nframes) return fail(ORBFE_ERR_INVALID, "debug_image: invalid argument");
    int rc = use_device(h->device);
    if (rc) return rc;
    ORBFE_HIP(hipDeviceSynchronize());
    if (stage == 0 || stage == 104) { // the threshold image; 104: the bit image the contour kernels of the last batch read (after the speck passes, if they ran)
        std::vector<uint32_t> bits(h->geo.bits_fu32);
        ORBFE_HIP(hipMemcpy(bits.data(), (stage == 104 && h->specks_ran ? h->d_bitsc : h->d_bits).as<uint32_t>() + (size_t)frame * h->geo.bits_fu32, bits.size() * 4,
                            hipMemcpyDeviceToHost));
        for (int y = 0; y < h->geo.rows; y++)
            for (int x = 0; x < h->geo.cols; x++)
                out[(size_t)y * h->geo.cols + x] = ((bits[(size_t)y * h->geo.wpr + (x >> 5)] >> (x & 31)) & 1) ? 255 : 0;
        return ORBFE_OK;
    }
    if (stage >= 1 && stage < h->geo.npyr + 1 && stage - 1 >= 1) { // pyramid level stage-1 (>= 1)
        const ArLevel& L = h->geo.levels[stage - 1];
        ORBFE_HIP(hipMemcpy2D(out, L.w, h->d_pyr.as<uint8_t>() + (size_t)frame * h->geo.pyr_fbytes + L.off, L.pitch, L.w, L.h,
                              hipMemcpyDeviceToHost));
        return ORBFE_OK;
    }
    if (stage == 100) { // counts: nkept, nrect, flags, ncand as 4 int32
        ORBFE_HIP(hipMemcpy(out, h->d_counts.as<int32_t>() + frame * 4, 16, hipMemcpyDeviceToHost));
        return ORBFE_OK;
    }
    if (stage == 101) { // rectangle candidates: AR_MAX_RECTS x ArRect (40 B)
        ORBFE_HIP(hipMemcpy(out, h->d_rects.as<ArRect>() + (size_t)frame * AR_MAX_RECTS, sizeof(ArRect) * AR_MAX_RECTS,
                            hipMemcpyDeviceToHost));
        return ORBFE_OK;
    }
    if (stage == 102) { // tail of the kept array (phase timing words of instrumented builds), 96 bytes
        ORBFE_HIP(hipMemcpy(out, h->d_kept.as<ArKept>() + (size_t)frame * AR_MAX_KEPT + AR_MAX_KEPT - 4, 96,
                            hipMemcpyDeviceToHost));
        return ORBFE_OK;
    }
    if (stage == 103) { // decode results of the frame, raw: AR_MAX_RECTS x (id, rotations)
        ORBFE_HIP(hipMemcpy(out, h->d_result.as<int32_t>() + (size_t)frame * AR_MAX_RECTS * 2, (size_t)AR_MAX_RECTS * 8,
                            hipMemcpyDeviceToHost));
        return ORBFE_OK;
    }
    return fail(ORBFE_ERR_INVALID, "debug_image: unknown stage %d", stage);
}

int orbfe_aruco_batch_status(orbfe_aruco* h, int32_t* nflagged, int32_t* flags_or)
{
    if (!h || !nflagged) return fail(ORBFE_ERR_INVALID, "orbfe_aruco_batch_status: null argument");
    int rc = use_device(h->device);
    if (rc) return rc;
    *nflagged = 0;
    if (flags_or) *flags_or = 0;
    if (h->last_nframes <= 0) return ORBFE_OK;
    ORBFE_HIP(hipDeviceSynchronize());
    std::vector<int32_t> counts((size_t)h->last_nframes * 4);
    ORBFE_HIP(hipMemcpy(counts.data(), h->d_counts.p, counts.size() * 4, hipMemcpyDeviceToHost));
    for (int f = 0; f < h->last_nframes; f++)
        if (counts[f * 4 + 2]) { (*nflagged)++; if (flags_or) *flags_or |= counts[f * 4 + 2]; }
    return ORBFE_OK;
}

int orbfe_aruco_set_big_frames(orbfe_aruco* h, int on)
{
    if (!h) return fail(ORBFE_ERR_INVALID, "null handle");
    end_speculation(h);
    h->sw.big_mode = on != 0;
    return ORBFE_OK;
}

int orbfe_aruco_set_aux_stream(orbfe_aruco* h, void* stream)
{
    if (!h) return fail(ORBFE_ERR_INVALID, "null handle");
    h->user_aux = (hipStream_t)stream;
    return ORBFE_OK;
}

int orbfe_aruco_debug_control(orbfe_aruco* h, const char* key, int value)
{
    if (!h || !key) return fail(ORBFE_ERR_INVALID, "orbfe_aruco_debug_control: null argument");
    const bool on_off = value == 0 || value == 1, by_rule = on_off || value == -1;
    if (!strcmp(key, "kernel_timing") && on_off) { h->timer.enabled = value; h->timer.reset_history(); }
    else if (!strcmp(key, "legacy_contours") && on_off) h->sw.force_legacy = value;
    else if (!strcmp(key, "tiled_contours") && by_rule) {
        if (h->sw.tiled == 0 && value != 0) h->batch_cap = 0;   // the tiled path's workspace is only allocated while it can run: allocate on the next batch
        h->sw.tiled = value;
    }
    else if (!strcmp(key, "speck_passes") && on_off) h->sw.specks = value;
    else if (!strcmp(key, "speck_passes_in_kernel") && on_off) { h->sw.specks_inkernel = value; h->invalidate_geometry(); }   // (the queue's size depends on it: geometry rebuilt)
    else if (!strcmp(key, "threshold_pyr") && on_off) h->sw.thr_pyr = value;
    else if (!strcmp(key, "threshold_mfma") && by_rule) { h->sw.thr_mfma = value != 0; h->sw.thr_mfma_auto = value == -1; }
    else if (!strcmp(key, "half_pyr") && on_off) h->sw.half_pyr = value;
    else return fail(ORBFE_ERR_INVALID, "orbfe_aruco_debug_control: unknown key \"%s\" or value %d", key, value);
    return ORBFE_OK;
}

int orbfe_aruco_debug_contour_retries(const orbfe_aruco* h)
{
    if (!h) return fail(ORBFE_ERR_INVALID, "null handle");
    return h->n_escalations;
}

int orbfe_aruco_debug_kernel_times(orbfe_aruco* h, float* out_us, int capacity)
{
    if (!h || !out_us) return fail(ORBFE_ERR_INVALID, "orbfe_aruco_debug_kernel_times: null argument");
    if (capacity < 0) return h->timer.collect_median(out_us, -capacity, nullptr);
    return h->timer.collect(out_us, capacity);
}

int orbfe_camera_resize(const float* K4, int cam_width, int cam_height, int img_width, int img_height, float* K4_out)
{
    if (!K4 || !K4_out || cam_width <= 0 || cam_height <= 0 || img_width <= 0 || img_height <= 0)
        return fail(ORBFE_ERR_INVALID, "orbfe_camera_resize: invalid argument");
    float k[4] = {K4[0], K4[1], K4[2], K4[3]};
    if (!(img_width == cam_width && img_height == cam_height)) { // cameraparameters.cpp:162-172
        const float ax = float(img_width) / float(cam_width), ay = float(img_height) / float(cam_height);
        k[0] *= ax; k[2] *= ax; k[1] *= ay; k[3] *= ay;
    }
    for (int i = 0; i < 4; i++) K4_out[i] = k[i];
    return ORBFE_OK;
}

int orbfe_marker_poses_batch_device(const orbfe_marker* d_markers, const int32_t* d_n, int capacity, int nframes,
                                    float marker_size, const float* K4, const float* dist, int ndist,
                                    orbfe_marker_pose* d_poses, void* stream)
{
    if (nframes < 0 || capacity < 0 || (nframes && capacity && (!d_markers || !d_poses)))
        return fail(ORBFE_ERR_INVALID, "orbfe_marker_poses_batch_device: invalid argument");
    PoseCamera c;
    int rc = pose_camera(K4, dist, ndist, marker_size, c, "orbfe_marker_poses_batch_device");
    if (rc) return rc;
    if (nframes == 0 || capacity == 0) return ORBFE_OK;
    hipLaunchKernelGGL(k_marker_poses, dim3((capacity + 31) / 32, nframes), dim3(64), 0, (hipStream_t)stream, d_markers, d_n,
                       capacity, marker_size, c, d_poses);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

int orbfe_marker_poses(const orbfe_marker* markers, int n, float marker_size, const float* K4, const float* dist, int ndist,
                       orbfe_marker_pose* poses, int device)
{
    if (n < 0 || (n && (!markers || !poses))) return fail(ORBFE_ERR_INVALID, "orbfe_marker_poses: invalid argument");
    PoseCamera c;
    int rc = pose_camera(K4, dist, ndist, marker_size, c, "orbfe_marker_poses");
    if (rc || (rc = use_device(device))) return rc;
    if (n == 0) return ORBFE_OK;
    HostStage& w = tl_host_ws.get();
    const size_t pb = (size_t)n * sizeof(orbfe_marker_pose);
    IoLayout l;
    const size_t i_mk = l.take((size_t)n * sizeof(orbfe_marker));
    l.outputs();
    const size_t o_p = l.take(pb);
    if ((rc = w.begin(l))) return rc;
    w.put(i_mk, markers, (size_t)n * sizeof(orbfe_marker));
    if ((rc = w.upload())) return rc;
    hipLaunchKernelGGL(k_marker_poses, dim3((n + 31) / 32, 1), dim3(64), 0, w.stream, w.dev<const orbfe_marker>(i_mk), (const int32_t*)nullptr,
                       n, marker_size, c, w.dev<orbfe_marker_pose>(o_p));
    ORBFE_HIP(hipGetLastError());
    if ((rc = w.download()) || (rc = w.sync())) return rc;
    memcpy(poses, w.host<uint8_t>(o_p), pb);
    return ORBFE_OK;
}

} // extern "C"
