/*
 * orbfe.h -- C ABI of the MI355X-native per-frame front-end for ORB_SLAM2_aruco.
 *
 * One shared library (liborbfe.so, built by hipcc for gfx950) exports exactly the
 * entry points below.  Plain pointers and sizes only: no C++ types, no torch
 * types, nothing thrown across the boundary (status codes instead; the C++ shim
 * classes in include/shims/ re-raise to keep reference behaviour).
 *
 * Each group names the reference interface it replaces (file:line in the
 * reference tree, CarminLiu/ORB_SLAM2_aruco):
 *
 *   orbfe_extractor_*   ORB_SLAM2::ORBextractor            include/ORBextractor.h:45-113
 *                       ctor                               src/ORBextractor.cc:410-470
 *                       operator()(image, mask, kps, desc) src/ORBextractor.cc:1043-1105
 *                       Get{Levels,ScaleFactor(s),...}     include/ORBextractor.h:63-83
 *                       called from Frame::ExtractORB      src/Frame.cc:200-206
 *   orbfe_aruco_*       aruco::MarkerDetector              Thirdparty/aruco/aruco/markerdetector.h:96-312
 *                       setDictionary / setDetectionMode / setCornerRefinementMethod / detect
 *                       configured + called at             src/Frame.cc:129-142
 *   orbfe_hamming*,     ORBmatcher::DescriptorDistance     src/ORBmatcher.cc:1651-1667
 *   orbfe_knn2*,        best/second-best inner loop of every SearchBy*  
 *   orbfe_search_for_initialization   ORBmatcher::SearchForInitialization  src/ORBmatcher.cc:409-524
 *   orbfe_initialize*   ORB_SLAM2::Initializer::Initialize src/Initializer.cc:44-121  (called from Tracking.cc:497-680)
 *                       Initializer::InitializeUseAruco    src/Initializer.cc:124-189 (Tracking.cc:632)
 *   orbfe_pose_*        Optimizer::PoseOptimizationByAruco src/Optimizer.cc:522-770 (Tracking.cc:940, 1025, 1200, 1256, 1843)
 *                       Optimizer::PoseOptimization        src/Optimizer.cc:308-520, monocular
 *   orbfe_sim3_*        ORB_SLAM2::Sim3Solver              src/Sim3Solver.cc (LoopClosing.cc:402-425, :489-600)
 *   orbfe_optimize_sim3* Optimizer::OptimizeSim3           src/Optimizer.cc:1544-1739 (LoopClosing.cc:425, :580)
 *   orbfe_create_new_map_points*, orbfe_new_points_*, orbfe_triangulate_matches_batch_device
 *                       LocalMapping::CreateNewMapPoints   src/LocalMapping.cc:222-467, monocular (+ ComputeF12, :904-921)
 *
 * Memory convention: functions without a suffix take HOST pointers (drop-in for
 * the reference's call sites, which hand over cv::Mat / std::vector storage) and
 * do their own H2D/D2H staging.  Functions ending in _device take DEVICE pointers
 * (hipMalloc'd, e.g. torch CUDA tensors) and a hipStream_t passed as void*; they
 * launch asynchronously on that stream and are the batched-video path.
 *
 * Threading: an extractor / detector handle is a stateful, non-re-entrant object
 * like the classes it replaces (one handle per stream of frames).  The
 * matching functions are thread-safe (device scratch per calling thread, device and stream, released when the thread
 * exits); so is orbfe_vocabulary_transform on one shared
 * vocabulary handle, and it does not serialise the callers (ComputeBoW runs on the Tracking, LocalMapping and LoopClosing
 * threads: the handle is read-only, each thread stages in its own scratch).  orbfe_corner_subpix: scratch per (thread, device).
 */
#ifndef ORBFE_H
#define ORBFE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* liborbfe.so is built with -fvisibility=hidden: what is declared between here and the matching pop is its whole dynamic symbol table */
/* the four opaque handles (their members are not part of the ABI: declared before the push, so that the library's own definitions
 * of them keep hidden visibility) */
typedef struct orbfe_extractor orbfe_extractor;   /* ORB_SLAM2::ORBextractor */
typedef struct orbfe_aruco orbfe_aruco;           /* aruco::MarkerDetector */
typedef struct orbfe_vocabulary orbfe_vocabulary; /* DBoW2 ORBVocabulary */
typedef struct orbfe_pipeline orbfe_pipeline;     /* the batched-video mode */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* status codes (0 = ok, <0 = error; orbfe_last_error() holds the message of the calling thread) */
#define ORBFE_OK 0
#define ORBFE_ERR_INVALID (-1)   /* bad argument (null pointer, non-positive size, ...) */
#define ORBFE_ERR_NO_DEVICE (-2) /* no gfx950 device / HIP runtime unusable: the product path has NO CPU fallback */
#define ORBFE_ERR_HIP (-3)       /* a HIP call failed */
#define ORBFE_ERR_CAPACITY (-4)  /* caller-provided output capacity too small */
#define ORBFE_ERR_DICT (-5)      /* unknown dictionary name */

/* cv::KeyPoint layout (pt.x, pt.y, size, angle, response, octave, class_id) = 28 bytes;
 * fields are set as at src/ORBextractor.cc:822-846,:477 */
typedef struct orbfe_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orbfe_keypoint;

/* aruco::Marker essentials (marker.h:42-56): id + 4 refined corners (x,y) in detection order */
typedef struct orbfe_marker {
    int32_t id;
    float corners[4][2];
} orbfe_marker;

const char* orbfe_last_error(void);
const char* orbfe_version(void);
int orbfe_device_count(void); /* number of usable HIP devices, 0 if none */

/* ------------------------------------------------------------------ ORB extractor -- */

/* ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST); device = HIP device ordinal. NULL on error. */
orbfe_extractor* orbfe_extractor_create(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST,
                                        int device);
void orbfe_extractor_destroy(orbfe_extractor* h);

int orbfe_extractor_get_levels(const orbfe_extractor* h);                                 /* GetLevels */
float orbfe_extractor_get_scale_factor(const orbfe_extractor* h);                         /* GetScaleFactor */
int orbfe_extractor_get_scale_factors(const orbfe_extractor* h, float* out);              /* GetScaleFactors */
int orbfe_extractor_get_inverse_scale_factors(const orbfe_extractor* h, float* out);      /* GetInverseScaleFactors */
int orbfe_extractor_get_scale_sigma_squares(const orbfe_extractor* h, float* out);        /* GetScaleSigmaSquares */
int orbfe_extractor_get_inverse_scale_sigma_squares(const orbfe_extractor* h, float* out);/* GetInverseScaleSigmaSquares */
int orbfe_extractor_get_features_per_level(const orbfe_extractor* h, int32_t* out);       /* mnFeaturesPerLevel */
/* upper bound on keypoints per frame (the quadtree may overshoot a level quota by a few nodes,
 * src/ORBextractor.cc:730): size kps/desc buffers with this */
int orbfe_extractor_max_keypoints(const orbfe_extractor* h);

/* operator()(image, mask(ignored), keypoints, descriptors) for one CV_8UC1 frame in host memory.
 * img: rows x cols bytes with row stride `step`.  kps: capacity records; desc: capacity x 32 bytes, row i belongs to
 * kps[i].  *n_out = number of keypoints.  Empty image (rows==0 || cols==0 || img==NULL) -> ORBFE_OK with *n_out
 * untouched semantics of :1046 mapped to *n_out = 0.
 * Frame geometry this implementation accepts (ORBFE_ERR_INVALID otherwise): every pyramid level at least 62 pixels in both
 * directions (below that the reference's cell grid has no column, ORBextractor.cc:780-784); levels up to 4127 pixels (a keypoint travels as 12 + 12 bits inside the kernels);
 * 1 to 16 quadtree roots per level, nIni = round(width / height) of the border-less level (ORBextractor.cc:544): portrait frames give
 * nIni = 0, on which the reference divides by zero and indexes an empty vector; frames wider than 16.5 : 1 are a capacity limit of
 * the quadtree kernels; a level's keypoint quota (mnFeaturesPerLevel) up to about 2700 -- its node lists live in LDS -- i.e.
 * nfeatures up to ~12000 at 8 levels and scale 1.2 (ORBFE_ERR_CAPACITY beyond). */
int orbfe_extract(orbfe_extractor* h, const uint8_t* img, int rows, int cols, size_t step, orbfe_keypoint* kps,
                  uint8_t* desc, int capacity, int32_t* n_out);

/* Batched video mode, host buffers: nframes images `frame_stride` bytes apart; outputs are nframes blocks of
 * `capacity` records; n_out[nframes]. */
int orbfe_extract_batch(orbfe_extractor* h, const uint8_t* imgs, int nframes, size_t frame_stride, int rows, int cols,
                        size_t step, orbfe_keypoint* kps, uint8_t* desc, int capacity, int32_t* n_out);

/* Batched video mode, device buffers, asynchronous on `stream` (hipStream_t). d_n_out: int32[nframes] on device.
 * LAYOUT OF DEVICE FRAMES (this call, orbfe_aruco_detect_batch_device, orbfe_pipeline_step): the kernels read the frames where they
 * lie, so a ROI of a larger device frame or a pitched allocation is passed as it is --
 *   - d_imgs may sit at any byte: no alignment is asked of the base, the step or the frame stride;
 *   - step: any value >= cols and below 2^23 (8388608), with (rows - 1) * step + cols below 2^31: rows are addressed with 24-bit
 *     multiplies and 32-bit offsets inside a frame (frames themselves with 64 bits);
 *   - frame_stride: any value >= (rows - 1) * step + cols (not looked at when nframes is 1);
 *   - the bytes between a row's last pixel and the next row, and between frames, are never written and their content has no
 *     influence on any result.  They may be READ: every row, the last row of the last frame included, has to be followed by
 *     readable memory up to `step` bytes from its first pixel.  (The one reader of such bytes is the detector's /2 pyramid where base,
 *     step and frame stride are all multiples of 8: it loads a row in 8-byte pieces, up to 6 bytes past the pixels and never past
 *     `step`.  No other kernel reads a byte behind the last row's last pixel; the requirement is not meant to grow.)
 * Anything else is ORBFE_ERR_INVALID before a kernel is enqueued (orbfe_last_error names the bound). */
int orbfe_extract_batch_device(orbfe_extractor* h, const uint8_t* d_imgs, int nframes, size_t frame_stride, int rows,
                               int cols, size_t step, orbfe_keypoint* d_kps, uint8_t* d_desc, int capacity,
                               int32_t* d_n_out, void* stream);
/* The 8-bit taps of the extractor's GaussianBlur(7x7, sigma 2) (ORBextractor.cc:1086) depend on the OpenCV release the
 * reference is built against.  mode 0 (default): every tap rounded on its own, 18 34 49 55 49 34 18 (sum 257) -- OpenCV 2.4 / 3.2
 * (what CMakeLists.txt:32-38 asks for) and the first fixed-point GaussianBlur of 3.4.  mode 1: the later bit-exact kernel
 * (rounding error carried from tap to tap, the centre tap takes the remainder), 18 34 48 56 48 34 18 (sum 256) -- late 3.4.x, 4.x.
 * Output is sat_u8((sum + 2^15) >> 16) either way. */
int orbfe_extractor_set_gaussian_taps(orbfe_extractor* h, int mode);

/* The device-pointer entry point is asynchronous and cannot return a capacity error: a frame whose keypoint total exceeds
 * `capacity` is clamped to it.  A clamped frame holds a PREFIX of its full result: records and descriptor rows 0 .. capacity - 1 of
 * what a sufficient capacity gives, byte for byte (the output is the concatenation of the levels in ascending order, cut at
 * `capacity`: level 0 comes first, the coarsest levels are what is cut); d_n_out[f] = capacity, slots of other frames and slots past
 * d_n_out[f] are not written.  After the batch (synchronises the device): *overflow = 0, or the largest per-frame total
 * that did not fit -- the batch's records are then incomplete and the call must be repeated with capacity >= *overflow
 * (orbfe_extractor_max_keypoints() always suffices).  The flag covers every batch since it was last read (reading clears it).
 * The host-pointer calls keep a flag of their own: they return ORBFE_ERR_CAPACITY themselves, never show here, and an unread
 * flag of a device batch does not fail them. */
int orbfe_extractor_batch_status(orbfe_extractor* h, int32_t* overflow);

/* Stage read-back for parity tests (valid after an extract call; `frame` indexes the last batch).
 * stage 0: pyramid level image, 1: blurred level image -> out must hold w*h bytes (tightly packed). */
int orbfe_extractor_debug_level_size(orbfe_extractor* h, int level, int* w, int* hgt);
int orbfe_extractor_debug_level_image(orbfe_extractor* h, int frame, int level, int stage, uint8_t* out);
/* stage 0: FAST candidates handed to the quadtree (x,y relative to the 16-px border, response=score),
 * stage 1: keypoints kept by the quadtree (level coordinates).  Returns count in *n (<= capacity copied). */
int orbfe_extractor_debug_level_keypoints(orbfe_extractor* h, int frame, int level, int stage, orbfe_keypoint* out,
                                          int capacity, int32_t* n);
/* per-kernel timing of the last batch call on this handle, microseconds, in launch order; returns number written (0 while timing is
 * off: orbfe_extractor_debug_control "kernel_timing"; out_us == NULL is ORBFE_ERR_INVALID).  capacity < 0:
 * the per-interval MEDIAN over the batches recorded since timing was switched on (the newest 64 at most), -capacity slots --
 * what bench.py reports, because one batch's events are not the steady state of a pipelined run. */
/* The extractor forks one launch (the blur, which only needs the pyramid) onto a second stream so that it overlaps with
 * FAST and the quadtree.  By default that is a stream the handle owns; an application that already has a lightly
 * loaded stream (bench.py: the matching stream) can lend it instead -- ROCm maps streams onto a few hardware queues, and
 * two busy streams on one queue serialise.  NULL restores the internal stream.  Ordering is by events either way. */
int orbfe_extractor_set_aux_stream(orbfe_extractor* h, void* stream);
/* Phase lock between the extractor handles of a pipeline (device-pointer batches): every batch of `h` starts behind a stage of the
 * latest batch enqueued on `other` -- stage 1 = its FAST, 2 = its quadtree, 3 = its descriptors, 4 = its resize chain (FAST starts); 0 or
 * other == NULL: free running.
 * Two engine sets that follow each other run a fixed half-period apart instead of in whatever phase contention leaves them
 * (bench.py: measured).  stage + 10 * g adds a second gate: the handle's FAST waits for stage g of `other` (with stage
 * % 10 == 0 the resize chain starts freely; measured slower in every combination, docs/history/DESIGN_rounds_1-4.md §6b).  `other` must outlive the
 * relation.  Results do not depend on it. */
int orbfe_extractor_follow(orbfe_extractor* h, orbfe_extractor* other, int stage);
/* The same relation for any other work of the pipeline: whatever is enqueued on `stream` after this call starts behind stage 1 .. 4
 * of the latest batch enqueued on `h` (nothing to wait for before its first batch). */
int orbfe_extractor_stage_wait(orbfe_extractor* h, int stage, void* stream);

/* Pairing for the drop-in path.  The reference builds a Frame by calling ORBextractor::operator() and then
 * MarkerDetector::detect on the SAME grey image (Frame.cc:91 / :200-206, then :142), one after the other on the Tracking thread; the
 * two are independent.  With a detector paired to an extractor, a one-frame orbfe_extract uploads the image once and starts the
 * detector on that device copy on the detector's own stream, next to its own launches; the following orbfe_aruco_detect /
 * orbfe_aruco_detect_poses call, if it is handed the same image (rows, cols and every pixel, compared with the copy the extractor
 * staged), waits for that
 * work and returns its results -- poses included when camera and marker size are those of the detector's previous call.  Any
 * other image, a batch call, or a capacity flag: the call runs as if nothing had been started.  Results are identical either way.
 * detector == NULL unpairs; unpair (or destroy the extractor) before destroying the detector.  Both handles on one device. */
int orbfe_extractor_pair_detector(orbfe_extractor* h, struct orbfe_aruco* detector);
int orbfe_extractor_debug_kernel_times(orbfe_extractor* h, float* out_us, int capacity);

/* ------------------------------------------------------------------ descriptor matching -- */
/* Debug/test switch.  "knn2_path": 0 = the matrix-core kernel wherever it applies -- at most 65535 train descriptors and init > 0 --
 * and the VALU tile kernel otherwise (default), 1 = the VALU tile kernel always, 2 = as 0.
 * Both kernels give identical results.  No key of the shipped library skips work ("orb_skip" / "aruco_skip" exist only in
 * the -DORBFE_ABLATION diagnosis build, whose orbfe_version() says "+ablation"; here they are ORBFE_ERR_INVALID). */
int orbfe_debug_control(const char* key, int value);
/* The same for one engine handle.  An unknown key or a value outside its range is ORBFE_ERR_INVALID and changes nothing.
 * Extractor:  "kernel_timing" 0 / 1 (event timing off / on; either clears the history), "general_quadtree" 0 / 1 (the general
 *   quadtree kernel for every level), "pyramid_depth" 0 .. 6 (depth of the quadtree count pyramid; 0 = by the levels' node counts).
 * Detector:  "kernel_timing" 0 / 1, "legacy_contours" 0 / 1 (the single-walker contour kernel for every frame), "tiled_contours"
 *   -1 / 0 / 1 (the tiled contour path by frame and batch size, the default / never / always), "speck_passes" 0 / 1 (as a launch of
 *   their own: never / wherever their tile fits LDS), "speck_passes_in_kernel" 0 / 1 (inside the one-workgroup relay kernels),
 *   "threshold_pyr" 1 / 0 (k_threshold_pyr where it applies, the default / k_adaptive_threshold_t), "threshold_mfma" -1 / 0 / 1
 *   (k_threshold_mfma for calls of 8 frames and more, the default / never / wherever it applies), "half_pyr" 1 / 0 (k_half_pyr, the
 *   default / a launch per level).  ORBFE_ARUCO_TILED and ORBFE_ARUCO_SPECKS set the same switches when the handle is created.
 * Results do not depend on any of them. */
int orbfe_extractor_debug_control(orbfe_extractor* h, const char* key, int value);
int orbfe_aruco_debug_control(orbfe_aruco* h, const char* key, int value);

/* popcount(a XOR b) over 256 bits, host pointers (ORBmatcher::DescriptorDistance) */
int orbfe_hamming(const uint8_t* a, const uint8_t* b);
/* Two more host-side scalar helpers for the reference's protected members (the device searches carry their own copies):
 * ComputeThreeMaxima (ORBmatcher.cc:1605-1646) on L bin populations -> ind3[0..2], -1 where the 10 % rule drops a runner-up;
 * CheckDistEpipolarLine (ORBmatcher.cc:139-157): 1 if keypoint 2 lies within 3.84 sigma^2 of the epipolar line of keypoint 1
 * (F12 row-major 3 x 3, level_sigma2 = mvLevelSigma2[kp2.octave]). */
void orbfe_three_maxima(const int32_t* counts, int L, int32_t* ind3);
int orbfe_epipolar_distance_ok(float x1, float y1, float x2, float y2, const float* F12, float level_sigma2);

/* All-pairs best / second-best of nq query descriptors against nt train descriptors (32 B rows), rule of App. D:
 *   if d<best {second=best; best=d; idx=t} else if d<second {second=d}   (first candidate wins ties)
 * best and second start at `init` (256 or INT_MAX in the reference). idx = -1 when nt == 0. Host pointers. */
int orbfe_knn2(const uint8_t* Q, int nq, const uint8_t* T, int nt, int init, int32_t* best_idx, int32_t* best_dist,
               int32_t* second_dist, int device);

/* The same rule over per-query candidate lists in CSR form (offsets[nq + 1] starting at 0, idx[offsets[nq]] rows of T):
 * the inner loop of the guided searches whose candidates the caller builds (SearchByBoW node lists, ORBmatcher.cc:159-292;
 * Fuse; SearchForTriangulation).  Candidates are visited in list order.  Host pointers. */
int orbfe_knn2_csr(const uint8_t* Q, int nq, const uint8_t* T, int nt, const int32_t* offsets, const int32_t* idx, int init,
                   int32_t* best_idx, int32_t* best_dist, int32_t* second_dist, int device);

/* Batched device variant: npairs independent (Q,T) problems. Q/T: device pointers to descriptor blocks,
 * block p at Q + p*q_stride bytes with d_nq[p] valid rows (<= max_nq), same for T. Outputs blocks of max_nq.
 * d_nq == NULL: every pair has max_nq queries.  t_stride = 0 (q_stride = 0): one train (query) block shared by all pairs.  Strides
 * are multiples of 16 bytes.  The counts are the caller's duty, 0 <= d_nq[p] <= max_nq and 0 <= d_nt[p] <= max_nt: they are not
 * clamped.  Rows past d_nq[p] of a block are neither read nor written, rows past d_nt[p] are not read; d_nt[p] == 0 gives
 * idx = -1 and both distances `init`.  Asynchronous on `stream`. */
int orbfe_knn2_batch_device(const uint8_t* d_Q, const int32_t* d_nq, size_t q_stride, int max_nq, const uint8_t* d_T,
                            const int32_t* d_nt, size_t t_stride, int max_nt, int npairs, int init,
                            int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_second_dist, void* stream);

/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize).  The keypoints are the
 * UNDISTORTED ones (mvKeysUn).  bounds = {mnMinX, mnMinY, mnMaxX, mnMaxY} of the undistorted image
 * (Frame::ComputeImageBounds, Frame.cc:418-451): the 64 x 48 Frame grid spans them (Frame.cc:112-113); NULL = a camera
 * without distortion, 0, 0, cols, rows (Frame.cc:440-446).  prev_matched: n1 x 2 floats, updated in place like
 * vbPrevMatched; matches12: n1 ints (-1 = none).  Returns ORBFE_OK and the match count in *nmatches. */
int orbfe_search_for_initialization(const orbfe_keypoint* kps1, const uint8_t* desc1, int n1,
                                    const orbfe_keypoint* kps2, const uint8_t* desc2, int n2, int cols, int rows,
                                    const float* bounds, float* prev_matched, int32_t* matches12, int window_size, float nnratio,
                                    int check_orientation, int32_t* nmatches, int device);

/* The matching loop of ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (ORBmatcher.cc:45-129) on
 * flat arrays; the projection of the map points, the viewing-cosine radius and the MapPoint bookkeeping stay with the
 * caller.  Query q = a map point in view: window centre (x, y), radius r (already times the scale factor of the predicted
 * level, :71), octave range [min_level, max_level] (:71 passes predicted-1 .. predicted; max_level < 0 = no upper bound,
 * both <= 0 / < 0 = no octave test, as Frame::GetFeaturesInArea, Frame.cc:280-333), 32-byte descriptor.  Candidates are
 * GetFeaturesInArea's, in its order.  taken[i] != 0: keypoint i already carries a map point with observations (:91-93).
 *   mode 0: best / second-best distance and octave per query (:84-118), no state between queries -- also the inner loop
 *           of the (CurrentFrame, LastFrame) and (CurrentFrame, KeyFrame) variants (:1413-1433, :1551-1571);
 *           best_idx = -1, distances 256, levels -1 when there is no candidate.  match / nmatches may be NULL.
 *   mode 1: the whole loop: accept when best <= th_high (TH_HIGH = 100) and not (same octave and best > nnratio*second)
 *           (:121-128); an accepted keypoint is taken for the queries after it when the map point it received is observed
 *           (q_observed[q] = pMP->Observations() > 0, the test of :91-93; NULL = all observed).  match[q] = keypoint index or
 *           -1 (a keypoint assigned twice keeps the later query, as F.mvpMapPoints[bestIdx] = pMP does), *nmatches =
 *           accepted count, taken[] updated in place.  The raw outputs may be NULL.
 * Host pointers.  bounds as for orbfe_search_for_initialization; mono (no right-image test). */
typedef struct orbfe_window_query {
    float x, y, r;
    int32_t min_level, max_level;
} orbfe_window_query;
int orbfe_search_by_projection(const orbfe_keypoint* kps, const uint8_t* desc, int n, int cols, int rows, const float* bounds,
                               const orbfe_window_query* queries, const uint8_t* qdesc, int nq, uint8_t* taken, const uint8_t* q_observed,
                               int mode, int th_high, float nnratio, int32_t* best_idx, int32_t* best_dist, int32_t* best_level,
                               int32_t* second_dist, int32_t* second_level, int32_t* match, int32_t* nmatches, int device);

/* The same loop over the frames of a batch resident on the device (no host round trip per call): frame f owns block f of
 * `capacity` keypoint records (d_n[f] valid, the layout of orbfe_extract_batch_device) and block f of `qcapacity` queries
 * (d_nq[f] valid) with their descriptors, flags and outputs.  mode 0 / 1 as above; mode 2 = the best-only loop of
 * orbfe_search_by_projection_best (d_q_angle, factor, check_orientation, d_match_cur[f][keypoint] = query or -1; d_q_observed
 * plays q_blocks).  d_taken (may be NULL) is updated in place.  Asynchronous on `stream`; a candidate row that overflowed the
 * per-stream scratch truncates silently, so ask orbfe_search_by_projection_batch_status afterwards: *overflow = 0, or the
 * longest candidate list -- the scratch has then been grown and repeating the call succeeds.  The flag is sticky like the extractor's
 * and SearchForInitialization's: it covers every _batch_device search / fuse call on this stream since it was last read (reading
 * clears it), so two batches may be enqueued before one status call.  After a truncated search the caller restores d_taken before
 * it repeats the call: the first attempt has marked keypoints.
 * Counts are clamped: a frame searches its first min(d_n[f], capacity) keypoints with its first min(d_nq[f], qcapacity) queries,
 * a negative count is 0.  Nothing past those rows is read or written: the per-query outputs get nq entries, d_match_cur and
 * d_taken n.  mode 0 writes only the five raw outputs (d_match is required but stays untouched, as does d_nmatches); modes 1 and
 * 2 write d_match, d_nmatches[f] and, where given, the raw outputs; mode 2 also d_match_cur.  A frame without keypoints answers
 * every query with best_idx = -1, distances 256, levels -1, match = -1. */
int orbfe_search_by_projection_batch_device(const orbfe_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int capacity, int nframes,
                                            int cols, int rows, const float* bounds, const orbfe_window_query* d_queries,
                                            const uint8_t* d_qdesc, const int32_t* d_nq, int qcapacity, uint8_t* d_taken,
                                            const uint8_t* d_q_observed, const float* d_q_angle, int mode, int th_high, float nnratio,
                                            float factor, int check_orientation, int32_t* d_best_idx, int32_t* d_best_dist,
                                            int32_t* d_best_level, int32_t* d_second_dist, int32_t* d_second_level, int32_t* d_match,
                                            int32_t* d_match_cur, int32_t* d_nmatches, void* stream);
int orbfe_search_by_projection_batch_status(void* stream, int32_t* overflow);

/* Scratch of the matching entry points is kept per (calling thread, device, stream) so that Tracking / LocalMapping / LoopClosing
 * calls do not serialise on each other.  Reuse a small fixed set of streams: at most 16 (device, stream) slots are kept per thread,
 * least recently used first out.  Before destroying a stream that was handed to a `_device` matching call, release its scratch
 * (grown candidate strides, unread overflow flags) so that a new stream at the same address starts clean.  Synchronises `stream`.
 * The host-pointer matching calls run on a stream of their own and keep their scratch under it: releasing NULL (the null stream)
 * does not drop it, it goes when the calling thread exits. */
int orbfe_release_stream_scratch(void* stream);

/* ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) (src/ORBmatcher.cc:1332-1474; what
 * TrackWithMotionModel runs every frame), monocular, whole on the device: the projection of the last frame's map points
 * with the current pose (:1362-1389), the window search on the Frame grid (levels octave +- 1, :1396), best match <= th_high
 * (TH_HIGH = 100, :1421), the blocking of keypoints that received an observed map point (:1397-1399), the rotation
 * histogram (factor 1/HISTO_LENGTH, :1341) and ComputeThreeMaxima (:1440-1471).
 * Per feature i of the last frame: valid_last[i] = has a map point and is not an outlier (NULL = all); x3Dw = its world
 * position (n_last x 3); mp_desc = MapPoint::GetDescriptor() (n_last x 32); mp_observed[i] = Observations() > 0 (NULL = all).
 * taken_cur[i2] = the keypoint already holds an observed map point (NULL = none).  Tcw = 3x4 row-major [Rcw | tcw]
 * (CurrentFrame.mTcw), K4 = fx fy cx cy, scale_factors = mvScaleFactors.  match_cur[i2] = i (the keypoint receives the
 * map point of last-frame feature i) or -1; *nmatches = the return value.  Host pointers. */
int orbfe_search_by_projection_last_frame(const orbfe_keypoint* kps_cur, const uint8_t* desc_cur, int n_cur, const uint8_t* taken_cur,
                                          int cols, int rows, const float* bounds, const orbfe_keypoint* kps_last, int n_last,
                                          const uint8_t* valid_last, const float* x3Dw, const uint8_t* mp_desc, const uint8_t* mp_observed,
                                          const float* Tcw, const float* K4, const float* scale_factors, int nlevels, float th, int th_high,
                                          int check_orientation, int32_t* match_cur, int32_t* nmatches, int device);
/* The same loop for queries projected by the caller -- SearchByProjection(CurrentFrame, KeyFrame, sAlreadyFound, th, ORBdist)
 * (:1476-1603: th_high = ORBdist, levels nPredictedLevel +- 1 from MapPoint::PredictScale, q_blocks = NULL) and the other
 * best-only variants: queries (r < 0 = skip) with their descriptors, q_angle = the source keypoints' angles, factor = the
 * histogram factor of the variant. */
int orbfe_search_by_projection_best(const orbfe_keypoint* kps, const uint8_t* desc, int n, int cols, int rows, const float* bounds,
                                    const orbfe_window_query* queries, const float* q_angle, const uint8_t* qdesc, const uint8_t* q_blocks,
                                    int nq, const uint8_t* taken, int th_high, int check_orientation, float factor, int32_t* match_cur,
                                    int32_t* nmatches, int device);

/* The matching part of ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:829-970; chi2 = 5.99) and of Fuse(pKF, Scw,
 * vpPoints, th, vpReplacePoint) (:972-1104; chi2 = 0, Tcw / Ow from the decomposed Scw) on the device: per map point the
 * projection and gates (positive depth, KeyFrame::IsInImage, scale-invariance range, viewing angle < 60 deg), PredictScale,
 * the window search on the keyframe grid at levels [predicted - 1, predicted], the reprojection gate and the best
 * descriptor distance.  valid[i] = "pMP && !isBad() && !IsInKeyFrame(pKF)" resp. "!isBad() && !alreadyFound" (NULL = all);
 * min_dist / max_dist = the map point's mfMinDistance / mfMaxDistance: the range gate applies the 0.8f / 1.2f of
 * Get{Min,Max}DistanceInvariance() (MapPoint.cc:402-412) and MapPoint::PredictScale divides mfMaxDistance itself (:419) -- the
 * two are not recoverable from the getters' values bit-exactly, so the members are what every guided search here takes;
 * normal = GetNormal() (nmp x 3), mp_desc = GetDescriptor().
 * Tcw = 3x4 row-major [Rcw | tcw], Ow = camera centre (3).  best_idx[i] = keypoint or -1, best_dist[i] = its distance (256
 * if none); the caller applies bestDist <= TH_LOW and does the map bookkeeping (Replace / AddObservation, :943-964). */
int orbfe_fuse_search(const orbfe_keypoint* kps, const uint8_t* desc, int n, int cols, int rows, const float* bounds, const float* p3Dw,
                      const uint8_t* valid, const float* min_dist, const float* max_dist, const float* normal, const uint8_t* mp_desc, int nmp,
                      const float* Tcw, const float* Ow, const float* K4, const float* scale_factors, const float* inv_level_sigma2, int nlevels,
                      float log_scale_factor, float th, double chi2, int32_t* best_idx, int32_t* best_dist, int device);

/* The same over several keyframes resident on the device: LocalMapping::SearchInNeighbors fuses the current keyframe's map points
 * into every neighbour (`matcher.Fuse(pKFi, vpMapPointMatches)` in a loop, src/LocalMapping.cc:850-858) -- one call instead of a
 * host round trip per keyframe.  Keyframe k owns block k of `capacity` keypoint records / descriptors (d_n[k] valid; the layout of
 * orbfe_extract_batch_device); the nmp map points (device arrays) are shared, d_valid (may be NULL) is [nkf][nmp] because
 * IsInKeyFrame(pKF) depends on the keyframe; Tcw / Ow are HOST arrays of nkf poses (12 / 3 floats each).  Outputs [nkf][nmp].
 * Asynchronous on `stream`; a candidate row that overflowed the per-stream scratch truncates silently:
 * orbfe_search_by_projection_batch_status(stream) reports it (and grows the scratch for a repeat).  Keyframe k searches its first
 * min(d_n[k], capacity) keypoints (a negative count is 0); all nmp entries of both output blocks are written, -1 / 256 for a point
 * that is not valid, does not project or has no candidate -- hence for every point of a keyframe without keypoints. */
int orbfe_fuse_search_batch_device(const orbfe_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int capacity, int nkf, int cols, int rows,
                                   const float* bounds, const float* d_p3Dw, const uint8_t* d_valid, const float* d_min_dist,
                                   const float* d_max_dist, const float* d_normal, const uint8_t* d_mp_desc, int nmp, const float* Tcw,
                                   const float* Ow, const float* K4, const float* scale_factors, const float* inv_level_sigma2, int nlevels,
                                   float log_scale_factor, float th, double chi2, int32_t* d_best_idx, int32_t* d_best_dist, void* stream);
/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cc:1106-1330): the map points of
 * each keyframe are carried into the other camera (world -> own camera -> sR | t of the similarity, each stage rounded to
 * float), gated (positive depth, IsInImage, distance in the scale-invariance range of the FINAL camera coordinates),
 * PredictScale, window search at levels [predicted - 1, predicted], best distance <= th_high (TH_HIGH = 100); pairs that
 * agree in both directions are returned.  Feature i of keyframe k carries p3Dw_k[i], min/max_dist_k[i], mp_desc_k[i];
 * valid_k[i] = "map point exists, is not bad, is not already matched" (:1148-1155, :1230-1236; NULL = all).  T1w / T2w =
 * 3x4 row-major [R | t]; sT12 = [s12 R12 | t12], sT21 = [(1/s12) R12' | t21] as the caller computes them (:1123-1126).
 * match12[i1] = i2 or -1 (vpMatches12[i1] = vpMapPoints2[i2]); *nfound = the return value. */
int orbfe_search_by_sim3(const orbfe_keypoint* kps1, const uint8_t* desc1, int n1, const orbfe_keypoint* kps2, const uint8_t* desc2, int n2,
                         int cols, int rows, const float* bounds, const float* p3Dw1, const uint8_t* valid1, const float* min_dist1,
                         const float* max_dist1, const uint8_t* mp_desc1, const float* p3Dw2, const uint8_t* valid2, const float* min_dist2,
                         const float* max_dist2, const uint8_t* mp_desc2, const float* T1w, const float* T2w, const float* sT12,
                         const float* sT21, const float* K4, const float* scale_factors, int nlevels, float log_scale_factor, float th,
                         int th_high, int32_t* match12, int32_t* nfound, int device);

/* ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:294-407, loop closing): map points
 * projected with the similarity's rigid part (Tcw = [Rcw | tcw], Ow as computed at :303-308), gated as in Fuse incl. the viewing
 * angle, searched at levels [predicted - 1, predicted] among keypoints not yet matched (matched[i] = vpMatched[i] != NULL; a
 * keypoint that receives a point is matched for the points after it), best distance <= TH_LOW.  valid[i] = "!isBad() && not
 * in vpMatched".  match_kf[i] = index of the map point the keypoint received or -1; *nmatches = the return value. */
int orbfe_search_by_projection_sim3(const orbfe_keypoint* kps, const uint8_t* desc, int n, int cols, int rows, const float* bounds,
                                    const uint8_t* matched, const float* p3Dw, const uint8_t* valid, const float* min_dist,
                                    const float* max_dist, const float* normal, const uint8_t* mp_desc, int nmp, const float* Tcw,
                                    const float* Ow, const float* K4, const float* scale_factors, int nlevels, float log_scale_factor, int th,
                                    int32_t* match_kf, int32_t* nmatches, int device);

/* Only the projection + gates + PredictScale, as window queries for orbfe_search_by_projection / _best: r < 0 = not searched,
 * min_level = predicted - level_below, max_level = predicted + level_above.  normal == NULL: no viewing-angle gate.
 * keyframe_variant != 0: the projection of Fuse / SearchBySim3 / SearchByProjection(pKF, Scw, ...) (:321-358, :848-893): positive
 * depth, invz = 1 / z in float, u = fx * (xc * invz) + cx, KeyFrame::IsInImage (u < mnMaxX).  keyframe_variant == 0: the
 * projection of SearchByProjection(CurrentFrame, pKF, ...) (:1503-1512): NO depth gate, invzc = 1.0 / z in double,
 * u = (fx * xc) * invzc + cx, the Frame bounds test (u <= mnMaxX). */
int orbfe_project_map_points(const float* p3Dw, const uint8_t* valid, const float* min_dist, const float* max_dist, const float* normal, int n,
                             const float* Tcw, const float* Ow, const float* K4, int cols, int rows, const float* bounds, int keyframe_variant,
                             const float* scale_factors, int nlevels, float log_scale_factor, float th, int level_below, int level_above,
                             orbfe_window_query* queries, int device);

/* ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
 * (src/ORBmatcher.cc:1476-1603; Tracking::Relocalization calls it with (10, 100) and (3, 64), Tracking.cc:1858, :1875), whole on
 * the device: the projection above (keyframe_variant = 0), the distance gate, PredictScale, the window search at levels
 * predicted - 1 .. predicted + 1 among keypoints without a map point (taken_cur[i2] = CurrentFrame.mvpMapPoints[i2] != NULL; a
 * keypoint that receives a point is taken for the points after it), best distance <= orb_dist, rotation histogram (factor
 * 1 / HISTO_LENGTH) and ComputeThreeMaxima.  Per feature i of the keyframe: valid[i] = "has a map point that is not bad and
 * not in sAlreadyFound" (NULL = all), p3Dw, min_dist / max_dist, mp_desc as below, kf_angle[i] = pKF->mvKeysUn[i].angle.
 * Ow = -Rcw' tcw (:1482).  match_cur[i2] = i or -1; *nmatches = the return value. */
int orbfe_search_by_projection_keyframe(const orbfe_keypoint* kps_cur, const uint8_t* desc_cur, int n_cur, const uint8_t* taken_cur, int cols,
                                        int rows, const float* bounds, int n_kf, const float* kf_angle, const uint8_t* valid, const float* p3Dw,
                                        const float* min_dist, const float* max_dist, const uint8_t* mp_desc, const float* Tcw, const float* Ow,
                                        const float* K4, const float* scale_factors, int nlevels, float log_scale_factor, float th, int orb_dist,
                                        int check_orientation, int32_t* match_cur, int32_t* nmatches, int device);

/* Batched device variant over npairs frame pairs (frame t vs t-1 of a stream); all arrays are blocks of `capacity`
 * records per frame; pair p matches frame p (as F1) against frame p+1 (as F2). prev_matched == NULL means
 * "start from F1's own keypoint positions" (what Tracking does on the first call, src/Tracking.cc:520-523).
 * The counts are the caller's duty, 0 <= d_n[f] <= capacity <= 65535: they are not clamped.  Records past d_n[f] are not read.
 * d_matches12 block p gets d_n[p] entries, the entries from there to `capacity` are not written; d_nmatches[p] is always written
 * (0 when either frame is empty).  Asynchronous on `stream`. */
int orbfe_search_for_initialization_batch_device(const orbfe_keypoint* d_kps, const uint8_t* d_desc,
                                                 const int32_t* d_n, int capacity, int npairs, int cols, int rows, const float* bounds,
                                                 int window_size, float nnratio, int check_orientation,
                                                 int32_t* d_matches12, int32_t* d_nmatches, void* stream);
/* The batch entry point cannot return a capacity error either (the host-pointer one retries by itself): the candidate rows of a
 * frame pair live in one pool, and a pair that needs more entries than the pool holds loses rows.  After a batch issued by THIS
 * thread on `stream` (synchronises the stream): *overflow = 0, or the number of pool entries the fullest pair needed -- the batch's
 * matches are then incomplete; the per-stream pool has been grown, so repeating the batch call succeeds.  Only the pairs that
 * needed more than the pool are incomplete: every pair has a pool of its own.  More than 1024 level-0 keypoints in a frame:
 * ORBFE_ERR_CAPACITY (*overflow = that count, also when a pool overflowed in the same batch; only the pairs that frame belongs to
 * are wrong).  The flag covers every batch since it was last read (reading clears it, an error included). */
int orbfe_search_for_initialization_batch_status(void* stream, int32_t* overflow);

/* ------------------------------------------------------------ monocular two-view initializer -- */
/* ORB_SLAM2::Initializer (src/Initializer.cc), constructed as Initializer(frame1, sigma, iterations) and called with frame 2.
 * Keypoints are the UNDISTORTED ones (mvKeysUn) of the two frames, as for orbfe_search_for_initialization; matches12 is its
 * output (n1 entries, -1 = none: vMatches12).  K4 = fx, fy, cx, cy (mK).
 *
 * Random sets: the reference seeds rand() once per process (DUtils::Random::SeedRandOnce(0)) and draws iterations * 8 values;
 * rand_words holds them as rand() returned them, in draw order, and the call maps each through RandomInt(0, size - 1) with the
 * swap-with-back removal of Initializer.cc:80-97.  The rand() state stays with the caller.
 *
 * Deviations from the reference, where it has undefined behaviour:
 *   - fewer than 8 matches (RandomInt(0, -1)): ORBFE_OK, initialized = 0, best_h = best_f = -1, every other field 0;
 *   - the F branch taken with no F hypothesis of positive score (RH <= 0.40 or SH = SF = 0: ReconstructF would read an empty
 *     inlier vector): ORBFE_OK, initialized = 0, no motion checked.
 * p3d (n1 x 3) / triangulated (n1) are written exactly when the reference assigns vP3D / vbTriangulated: when the call
 * initializes.  On a failed reconstruction ReconstructH and ReconstructF leave both untouched, and so does this call.  Where they
 * are written, p3d is 0 for every keypoint CheckRT did not count.  Either may be NULL.  A matches12 entry outside [-1, n2) is
 * ORBFE_ERR_INVALID.  Host pointers. */
typedef struct orbfe_init_result {
    int32_t initialized;        /* Initialize()'s return value */
    int32_t model;              /* 0 = homography branch (RH > 0.40), 1 = fundamental; 2 = orbfe_initialize_check_poses */
    float   SH, SF, RH;
    int32_t best_h, best_f;     /* winning RANSAC iteration of each model (first strict maximum), -1 = none; check_poses: best_h = bestIdA */
    float   H21[9], F21[9];     /* the winning models, row-major, as FindHomography / FindFundamental return them (0 when none) */
    float   R21[9], t21[3];     /* valid when initialized; zero otherwise */
    int32_t n_good;             /* CheckRT's nGood of the accepted motion (or of the best one when not accepted) */
    float   parallax;           /* degrees, as CheckRT computes it, of that motion */
} orbfe_init_result;

int orbfe_initialize(const orbfe_keypoint* kps1, int n1, const orbfe_keypoint* kps2, int n2, const int32_t* matches12, const float* K4,
                     float sigma, int iterations, const int32_t* rand_words, orbfe_init_result* res, float* p3d, uint8_t* triangulated,
                     int device);

/* The batched device variant over npairs frame pairs, in the pair convention of orbfe_search_for_initialization_batch_device:
 * pair p is frame p (side 1) against frame p + 1 (side 2); d_kps / d_n / capacity are that call's blocks (npairs + 1 frames) and
 * d_matches12 its output (block p of `capacity` entries; an entry outside [-1, d_n[p+1]) counts as no match).  d_rand_words:
 * npairs x iterations x 8 (a word outside 0 .. RAND_MAX is clamped to the ends of the index range).  Outputs: d_res[npairs], d_p3d blocks of capacity x 3, d_triangulated blocks of capacity, written as
 * orbfe_initialize writes them (untouched for a pair that does not initialize).  K4 is read at the call.  Runs on `stream`,
 * no host synchronisation; scratch per (thread, device, stream). */
int orbfe_initialize_batch_device(const orbfe_keypoint* d_kps, const int32_t* d_n, int capacity, int npairs, const int32_t* d_matches12,
                                  const float* K4, float sigma, int iterations, const int32_t* d_rand_words, orbfe_init_result* d_res,
                                  float* d_p3d, uint8_t* d_triangulated, void* stream);

/* Initializer::InitializeUseAruco (src/Initializer.cc:124-189): CheckRT of npose caller-given motions (poses: npose x 12 floats,
 * R row-major then t) with every match an inlier and th2 = 4 sigma^2.  res->best_h = bestIdA (the first strict maximum of nGood,
 * -1 when no pose counts a point), n_good / parallax of it, initialized = !(bestGood < 0.7 N), R21 / t21 = that pose when
 * initialized; model = 2.  p3d / triangulated are those of bestIdA whenever there is one (the reference assigns them inside the
 * loop, also when it then returns false); npose = 0 returns at once (initialized = 0).  Host pointers. */
int orbfe_initialize_check_poses(const orbfe_keypoint* kps1, int n1, const orbfe_keypoint* kps2, int n2, const int32_t* matches12,
                                 const float* K4, float sigma, const float* poses, int npose, orbfe_init_result* res, float* p3d,
                                 uint8_t* triangulated, int device);

/* DIAGNOSTIC / TEST INTERFACE, no stability promise (its arguments may change with the kernels): orbfe_initialize with its
 * intermediate results (the parity tests): nmatches = N; sets: iterations x 8 match indices; T12: T1 then
 * T2 (row-major); pn1 / pn2: the normalised points of every keypoint (n1 x 2, n2 x 2); models: iterations x 27 (H21, H12, F21);
 * scores: SH of every iteration, then SF of every iteration.  sets / models / scores are left untouched when N < 8. */
int orbfe_initialize_inspect(const orbfe_keypoint* kps1, int n1, const orbfe_keypoint* kps2, int n2, const int32_t* matches12,
                             const float* K4, float sigma, int iterations, const int32_t* rand_words, orbfe_init_result* res,
                             int32_t* nmatches, int32_t* sets, float* T12, float* pn1, float* pn2, float* models, float* scores, int device);

/* ------------------------------------------------------------ Sim3 RANSAC of loop closing -- */
/* ORB_SLAM2::Sim3Solver (src/Sim3Solver.cc), the step of LoopClosing::ComputeSim3 between SearchByBoW(KF, KF) and SearchBySim3
 * (src/LoopClosing.cc:402-425, :489-600): RANSAC over closed-form Horn alignments of 3 correspondences.
 * Side k: kps = mvKeysUn (n entries), x3Dw[i] = world position of feature i's map point (n x 3), valid[i] != 0 = "feature i has a
 * map point, it is not bad, and its index in this keyframe is i" (Sim3Solver.cc:66-79; valid1 and valid2 both NULL = all),
 * Tcw = the keyframe's pose, 3 x 4 row-major, K4 = fx, fy, cx, cy.  match12[i1] = i2 or -1: what orbfe_search_by_bow returns.
 * level_sigma2 = mvLevelSigma2 (nlevels <= 32 entries, read at the call).  probability, min_inliers, max_iterations:
 * SetRansacParameters' arguments; the result's max_iterations is mRansacMaxIts after it.
 *
 * One call = one iterate(n_iterations, ...): the window [first_iteration, first_iteration + n_iterations) clipped to
 * mRansacMaxIts, with best_inliers_in = mnBestInliers on entry.  The library holds no state between calls: the caller carries
 * mnIterations (found + 1 after a success, else the end of the window) and mnBestInliers (best_inliers), and keeps the model it
 * holds when best = -1.  first_iteration = 0, n_iterations = max_iterations, best_inliers_in = 0 is find().  rand_words:
 * n_iterations x 3 values as rand() returned them, in draw order (RandomInt(0, size - 1) and the swap-with-back removal of
 * :163-177 are applied here); words past the clipped window are not read.  Every hypothesis of the window is computed, the
 * first that iterate() would return decides (the reference stops there; the words after it are the caller's to account for).
 * inliers12 (n1 bytes) = vbInliers: all 0 unless found >= 0.
 * The chi-square gates are (size_t)(9.210 * level_sigma2[octave]): the reference keeps them in a std::vector<size_t>.
 *
 * Where the reference is undefined:
 *   - N < 3 with min_inliers <= N (RandomInt(0, -1)): as N < min_inliers -- no_more = 1, found = -1, no word read;
 *   - a hypothesis whose quaternion has no imaginary part (0 / 0 at :280, a NaN model in OpenCV): zero inliers, a zero model,
 *     and it is never `best`;
 *   - a point with z = 0: its projection is inf / NaN, it is never an inlier;
 *   - an iteration count that is not finite or below 1 (log of a negative number when N < min_inliers; min_inliers = 0): 1.
 * ORBFE_ERR_INVALID: NULL pointers, a match12 entry outside [-1, n2), an octave outside [0, nlevels) on a kept correspondence,
 * a negative word, probability outside (0, 1), min_inliers < 0, best_inliers_in < 0, iteration counts outside 1 .. 100000.
 * Host pointers. */
typedef struct orbfe_sim3_result {
    int32_t n;                  /* N: correspondences the constructor kept */
    int32_t max_iterations;     /* mRansacMaxIts after SetRansacParameters */
    int32_t no_more;            /* bNoMore of this call */
    int32_t found;              /* global iteration index (0-based) of the hypothesis iterate() returned, -1 = none in this window */
    int32_t n_inliers;          /* nInliers (0 when found < 0) */
    int32_t best, best_inliers; /* mnBestInliers and the iteration that holds it, after this window (best = -1: no hypothesis of
                                   the window reached best_inliers_in; best_inliers = best_inliers_in then, the model fields 0) */
    float   s12, R12[9], t12[3];/* of `best` (== found on success): GetEstimatedScale / Rotation / Translation */
    float   T12[16];            /* mBestT12, row-major */
    int32_t status;             /* ORBFE_OK; the batch call: ORBFE_ERR_INVALID for a problem it skipped (see there) */
} orbfe_sim3_result;

int orbfe_sim3_solve(const orbfe_keypoint* kps1, int n1, const float* x3Dw1, const uint8_t* valid1, const float* Tcw1, const float* K4_1,
                     const orbfe_keypoint* kps2, int n2, const float* x3Dw2, const uint8_t* valid2, const float* Tcw2, const float* K4_2,
                     const int32_t* match12, const float* level_sigma2, int nlevels, int fix_scale, double probability, int min_inliers,
                     int max_iterations, int first_iteration, int n_iterations, int best_inliers_in, const int32_t* rand_words,
                     orbfe_sim3_result* res, uint8_t* inliers12, int device);

/* npairs whole runs (find()) on resident data, in the conventions of orbfe_search_by_bow_batch_device: per-frame blocks of
 * `capacity` entries of d_kps, d_x3Dw (x 3), d_valid (may be NULL) and d_n, d_Tcw 12 floats a frame; problem p is frame
 * d_pair1[p] (side 1) against frame d_pair2[p] (NULL index arrays: p and p + 1); d_match12 block p of `capacity` = that call's
 * output (an entry outside [-1, d_n[pair2]) counts as no match), so the two chain on one stream without a download.  One K4 for
 * both sides.  d_rand_words: npairs x max_iterations x 3 (a word outside 0 .. RAND_MAX is clamped to the ends of the index
 * range).  Outputs: d_res[npairs]; d_inliers12 blocks of `capacity`, the first d_n[pair1] entries written.  A problem with an
 * octave outside [0, nlevels) on a kept correspondence is skipped: its record has status ORBFE_ERR_INVALID and every other field
 * 0, its inliers are not written.  Four launches whatever npairs is; asynchronous on `stream`, no host synchronisation; scratch
 * per (thread, device, stream). */
int orbfe_sim3_solve_batch_device(const orbfe_keypoint* d_kps, const int32_t* d_n, int capacity, const float* d_x3Dw, const uint8_t* d_valid,
                                  const float* d_Tcw, const int32_t* d_pair1, const int32_t* d_pair2, int npairs, const int32_t* d_match12,
                                  const float* K4, const float* level_sigma2, int nlevels, int fix_scale, double probability,
                                  int min_inliers, int max_iterations, const int32_t* d_rand_words, orbfe_sim3_result* d_res,
                                  uint8_t* d_inliers12, void* stream);

/* DIAGNOSTIC / TEST INTERFACE, no stability promise: orbfe_sim3_solve with its intermediate results (the parity tests).
 * *n = N; per kept correspondence (n1 entries of capacity, the first N written, the rest 0): indices1, X3Dc1 / X3Dc2 (x 3),
 * P1im1 / P2im2 (x 2), maxError1 / maxError2; per iteration of the window (n_iterations entries; those the window does not
 * run are 0): sets (x 3 correspondence indices), models (x 13: s12, R12 row-major, t12), counts (inliers of the hypothesis). */
int orbfe_sim3_inspect(const orbfe_keypoint* kps1, int n1, const float* x3Dw1, const uint8_t* valid1, const float* Tcw1, const float* K4_1,
                       const orbfe_keypoint* kps2, int n2, const float* x3Dw2, const uint8_t* valid2, const float* Tcw2, const float* K4_2,
                       const int32_t* match12, const float* level_sigma2, int nlevels, int fix_scale, double probability, int min_inliers,
                       int max_iterations, int first_iteration, int n_iterations, int best_inliers_in, const int32_t* rand_words,
                       orbfe_sim3_result* res, uint8_t* inliers12, int32_t* n, int32_t* indices1, float* X3Dc1, float* X3Dc2, float* P1im1,
                       float* P2im2, float* maxError1, float* maxError2, int32_t* sets, float* models, int32_t* counts, int device);

/* ------------------------------------------------------------ Sim3 refinement of loop closing -- */
/* Optimizer::OptimizeSim3 (src/Optimizer.cc:1544-1739), the step of LoopClosing::ComputeSim3 between SearchBySim3 and
 * SearchByProjection(pKF, Scw, ...) (src/LoopClosing.cc:425, :580; its return value decides the loop): Levenberg-Marquardt on the
 * 7-DoF similarity S12 (g2o as ORB_SLAM2 vendors it, in double) over two reprojection edges per correspondence, optimize(5), a
 * chi2 > th2 check that removes pairs, then optimize(10 or 5) on what is left and a second check.
 * The sides are those of orbfe_sim3_solve: kps = mvKeysUn, x3Dw (n x 3), valid (both NULL = all), Tcw 3 x 4 row-major, K4 = fx, fy,
 * cx, cy.  match12[i1] = i2 or -1 = vpMatches1 as orbfe_search_by_sim3 / orbfe_sim3_solve leave it.  Correspondence i is kept
 * when match12[i] = i2 >= 0, valid1[i] and valid2[i2]; its points are P3Dkc = Rkw x + tkw in CV_32F (the Mat product of the Sim3
 * solver), widened to double.  Edges, in this order per correspondence: e12 = obs1 - cam_map1(project(S12.map(P2c))), information
 * inv_level_sigma2[octave of kps1[i]] * I; e21 = obs2 - cam_map2(project(S12.inverse().map(P1c))), information
 * inv_level_sigma2[octave of kps2[i2]] * I (inv_level_sigma2 = mvInvLevelSigma2, nlevels <= 32 entries, floats widened).  Huber,
 * delta = (double)sqrtf(th2), in both rounds.  The Jacobian is g2o's numeric one (central differences, delta = 1e-9, through
 * Sim3(update) * estimate); with fix_scale the update's 7th component is zeroed, column 6 of every Jacobian is exactly 0 and
 * H(6, 6) is lambda alone.  A pair is bad when either chi2 > (double)th2, read from the errors the edges cached last -- those of
 * a rejected trial when the round ended on one (stale_mask).  The initial similarity is g2o::Sim3(R12, t12, s12) of the floats:
 * both call sites build it from float cv::Mats.
 *
 * Outputs: match12_out (n1 entries, may be match12 itself) = match12 with -1 where the reference sets vpMatches1 to NULL; the
 * record.  When fewer than 10 pairs survive the first check the reference returns 0 at once: n_inliers = 0, more_iterations = 0,
 * the pairs already removed stay removed, and the similarity in the record is the one given (g2oS12 is not written back).
 *
 * Where the reference is undefined:
 *   - a projected point with z = 0 (an error or a numeric Jacobian that is not finite): that edge adds nothing to chi2, H and b in
 *     the pass where it happens, and a pair one of whose chi2 is not finite at a check is bad (never an inlier);
 *   - no kept correspondence (N = 0): no iteration runs (iterations[0] = -1), the early return, the similarity as given.
 * ORBFE_ERR_INVALID: NULL pointers, a match12 entry outside [-1, n2), an octave outside [0, nlevels) on a kept correspondence,
 * th2 <= 0, th2, K, the similarity, a pose, or a kept correspondence's point or observation not finite.  ORBFE_ERR_CAPACITY:
 * max(n1, n2) above the bound of the batch call.  Host pointers. */
typedef struct orbfe_sim3_opt_result {
    int32_t n_inliers;          /* the return value: nIn of the second check (0 on the early return) */
    int32_t n_correspondences;  /* nCorrespondences: the pairs kept */
    int32_t n_bad;              /* nBad of the first check */
    int32_t more_iterations;    /* nMoreIterations of the second optimize(): 10, 5, or 0 on the early return */
    int32_t iterations[2];      /* DIAGNOSTIC: LM iterations of each optimize() run (-1: no active edge) */
    int32_t stale_mask;         /* DIAGNOSTIC: bit r = optimize() r ended on a rejected trial (the check read that trial's errors) */
    int32_t status;             /* ORBFE_OK; the batch call: ORBFE_ERR_INVALID for a problem it skipped (see there) */
    double  s12, q12[4], t12[3];/* g2oS12 after the call: scale, rotation (x, y, z, w; not normalised, as g2o::Sim3 keeps it), translation */
} orbfe_sim3_opt_result;

int orbfe_optimize_sim3(const orbfe_keypoint* kps1, int n1, const float* x3Dw1, const uint8_t* valid1, const float* Tcw1, const float* K4_1,
                        const orbfe_keypoint* kps2, int n2, const float* x3Dw2, const uint8_t* valid2, const float* Tcw2, const float* K4_2,
                        const int32_t* match12, const float* inv_level_sigma2, int nlevels, float s12, const float* R12, const float* t12,
                        float th2, int fix_scale, int32_t* match12_out, orbfe_sim3_opt_result* res, int device);

/* npairs problems on resident data, in the layout of orbfe_sim3_solve_batch_device: per-frame blocks of `capacity` entries of
 * d_kps, d_x3Dw (x 3), d_valid (may be NULL) and d_n (clamped to the block), d_Tcw 12 floats a frame; problem p is frame d_pair1[p]
 * against frame d_pair2[p] (NULL index arrays: p and p + 1); d_match12 / d_match12_out blocks of `capacity` (the same array works
 * in place; the first d_n[pair1] entries are written, an input entry outside [-1, d_n[pair2]) counts as no match and is copied as
 * it is).  One K4 for both sides.  Problem p's initial similarity is the 13 floats s12, R12 (row-major), t12 at
 * (char*)d_sim12 + p * sim12_stride: d_sim12 = &d_res[0].s12 of orbfe_sim3_result with sim12_stride = sizeof(orbfe_sim3_result)
 * chains this call after orbfe_sim3_solve_batch_device on one stream without a download (stride and base multiples of 4, stride
 * >= 52).  A problem with an octave outside [0, nlevels) on a kept correspondence is skipped: its record has status
 * ORBFE_ERR_INVALID and every other field 0, its matches are not written.  One launch whatever npairs is; asynchronous on
 * `stream`, no host synchronisation, no scratch beyond the caller's buffers.  A problem is staged in its workgroup's LDS:
 * capacity x 53 B + 4 KB must fit (ORBFE_ERR_CAPACITY otherwise: capacity <= about 3 000 features a keyframe on gfx950's 160 KB). */
int orbfe_optimize_sim3_batch_device(const orbfe_keypoint* d_kps, const int32_t* d_n, int capacity, const float* d_x3Dw,
                                     const uint8_t* d_valid, const float* d_Tcw, const int32_t* d_pair1, const int32_t* d_pair2, int npairs,
                                     const int32_t* d_match12, const float* K4, const float* inv_level_sigma2, int nlevels,
                                     const void* d_sim12, size_t sim12_stride, float th2, int fix_scale, int32_t* d_match12_out,
                                     orbfe_sim3_opt_result* d_res, void* stream);

/* ------------------------------------------------------------ motion-only pose optimization -- */
/* Optimizer::PoseOptimizationByAruco(Frame*) (src/Optimizer.cc:522-770; every tracking path of Tracking.cc ends in it) and
 * Optimizer::PoseOptimization(Frame*) without its stereo branch (:308-520; nm = 0): four rounds of 10 Levenberg-Marquardt iterations
 * of the 6-DoF camera pose (g2o as ORB_SLAM2 vendors it, in double), each from the initial pose, with chi2 > 5.991 outlier
 * classification of the monocular edges after every round and their Huber kernel (delta = sqrt(5.991)) dropped after round 2.
 * Monocular edge i (has_mp[i] != 0): kps[i] = mvKeysUn[i] (x, y observed; octave picks inv_level_sigma2 = mvInvLevelSigma2),
 * x3Dw[i] = the map point's world position (n x 3).  Marker edges (Frame::mbUArucoIni, and only for markers with !mvbOldAruco,
 * mvbArucoGood and a MapAruco): four per marker record, corner k = mvArucoUn[4i + k] against Twm * get3DPointsLocalRefSystem(k),
 * information marker_info * I (the reference's wei = 25), Huber in every round, numeric Jacobian (g2o's central differences).
 * Poses are 3 x 4 row-major [R | t] floats (Tcw_in = mTcw, Tcw_out = what SetPose receives; they may be the same array).
 * outlier[i] = mvbOutlier[i] for every i with has_mp[i]; entries without a map point are not written.  chi2 (may be NULL) = the
 * chi2 of each monocular edge at the last classification (the value compared with 5.991).  With fewer than 3 monocular edges the
 * call returns n_good = 0, writes outlier[i] = 0 for them and copies Tcw_in to Tcw_out (the reference leaves the pose untouched).
 * An octave outside [0, nlevels) on an observation with a map point is ORBFE_ERR_INVALID.  nlevels <= 32.  Host pointers. */
typedef struct orbfe_pose_marker {
    float corners[8];           /* the four undistorted corners (x, y), mvArucoUn[4i .. 4i + 3] */
    float Twm[12];              /* MapAruco::GetTwm(), 3 x 4 row-major */
    float local[12];            /* get3DPointsLocalRefSystem(0 .. 3), the corners in the marker frame */
} orbfe_pose_marker;

typedef struct orbfe_pose_result {
    int32_t n_good;             /* the return value: n_initial - nBad of the last round run (0 when n_initial < 3) */
    int32_t n_initial;          /* nInitialCorrespondences: observations with a map point */
    int32_t n_marker_edges;     /* 4 x the marker records used (0 when n_initial < 3) */
    int32_t rounds;             /* rounds run: 4, 1 (fewer than 10 edges in all) or 0 (n_initial < 3) */
    int32_t n_bad[4];           /* nBad of each round run */
    int32_t iterations[4];      /* DIAGNOSTIC: LM iterations of each round run (-1: no active edge, optimize() returned -1) */
    int32_t stale_mask;         /* DIAGNOSTIC: bit r = round r ended on a rejected trial (its inliers' chi2 read that trial's errors) */
    int32_t status;             /* ORBFE_OK; the batch call: ORBFE_ERR_INVALID for a problem it skipped (see there) */
} orbfe_pose_result;

int orbfe_pose_optimization(const orbfe_keypoint* kps, int n, const uint8_t* has_mp, const float* x3Dw, const float* inv_level_sigma2,
                            int nlevels, const float* K4, const orbfe_pose_marker* markers, int nm, float marker_info, const float* Tcw_in,
                            float* Tcw_out, uint8_t* outlier, float* chi2, orbfe_pose_result* res, int device);

/* The same over nframes problems resident on the device, one launch.  Frame f owns block f of `capacity` entries of d_kps (the
 * layout of orbfe_extract_batch_device, d_n[f] valid), d_has_mp, d_x3Dw (x 3), d_outlier and d_chi2 (may be NULL), and block f
 * of `mcapacity` marker records (d_nm[f] valid; d_markers / d_nm may be NULL when mcapacity = 0).  d_Tcw_in / d_Tcw_out: 12
 * floats a frame (the same array works in place).  inv_level_sigma2, K4 and marker_info are read at the call.  A frame with an
 * octave outside [0, nlevels) on an observation with a map point is skipped: its result record has status ORBFE_ERR_INVALID and
 * every other field 0, its pose is copied, its outlier / chi2 entries are not written.  d_n / d_nm are clamped to the blocks.
 * capacity x 25 B + mcapacity x 160 B + 2 KB must fit in a workgroup's LDS (ORBFE_ERR_CAPACITY otherwise: about 6 000 keypoints
 * a frame on gfx950).  Asynchronous on `stream`; no scratch beyond the caller's buffers. */
int orbfe_pose_optimization_batch_device(const orbfe_keypoint* d_kps, const int32_t* d_n, int capacity, int nframes, const uint8_t* d_has_mp,
                                         const float* d_x3Dw, const orbfe_pose_marker* d_markers, const int32_t* d_nm, int mcapacity,
                                         const float* inv_level_sigma2, int nlevels, const float* K4, float marker_info,
                                         const float* d_Tcw_in, float* d_Tcw_out, uint8_t* d_outlier, float* d_chi2,
                                         orbfe_pose_result* d_res, void* stream);

/* The inputs of the batch call from what mode 2 of orbfe_search_by_projection_batch_device leaves on the device: for frame f and
 * keypoint i < d_n[f], m = d_match_cur[f][i]; has_mp = 0 <= m < d_nq[f], x3Dw = d_q_x3Dw[f][m] (the world point of query m, blocks
 * of qcapacity x 3 floats: the points the caller projected); entries without a match and those from d_n[f] to capacity get
 * has_mp = 0, x3Dw = 0.  Asynchronous on `stream`. */
int orbfe_pose_gather_device(const int32_t* d_match_cur, const int32_t* d_n, int capacity, int nframes, const float* d_q_x3Dw,
                             const int32_t* d_nq, int qcapacity, uint8_t* d_has_mp, float* d_x3Dw, void* stream);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:270-333; called after every new observation by Tracking,
 * LocalMapping and LoopClosing): for every map point, among the descriptors it was observed with (CSR: point p owns rows
 * offsets[p] .. offsets[p + 1] of desc, in the order of its observation map), the one with the least median Hamming distance
 * to the others -- median = sorted row[(int)(0.5 * (N - 1))], first row wins ties.  best_idx[p] = its index inside the point's
 * list (-1 for a point without descriptors, which the reference leaves untouched); best_desc (may be NULL) receives the chosen
 * descriptor (npoints x 32).  At most 256 observations per point.  Host pointers / device pointers + stream.
 * The host call checks the offsets (start at 0, non-decreasing) and returns ORBFE_ERR_CAPACITY for a point with more than 256
 * observations.  The device call cannot look at them: the offsets are the caller's duty, and a point with more than 256
 * observations is answered from its FIRST 256 -- best_idx in [0, 256) is what the call returns for those rows alone, the later
 * rows are not read.  best_desc of a point without descriptors is not written. */
int orbfe_distinctive_descriptors(const uint8_t* desc, const int32_t* offsets, int npoints, int32_t* best_idx, uint8_t* best_desc, int device);
int orbfe_distinctive_descriptors_device(const uint8_t* d_desc, const int32_t* d_offsets, int npoints, int32_t* d_best_idx, uint8_t* d_best_desc,
                                         void* stream);

/* ------------------------------------------------------------------ DBoW2 vocabulary transform -- */
/* ORBVocabulary (= DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>, include/ORBVocabulary.h) as Frame::ComputeBoW and
 * KeyFrame::ComputeBoW use it (src/Frame.cc:348-355, src/KeyFrame.cc): transform(descriptors, BowVector, FeatureVector, 4).
 * The handle owns the tree in HBM.  scoring / weighting are DBoW2's enums (BowVector.h:37-55): weighting 0 TF_IDF, 1 TF,
 * 2 IDF, 3 BINARY; scoring 0 L1_NORM .. 5 DOT_PRODUCT (decides the normalisation, ScoringObject.h:74-91). */

/* TemplatedVocabulary::loadFromTextFile (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1425; System.cc loads
 * ORBvoc.txt with it): "k L scoring weighting" then one line per node "parent isLeaf d0..d31 weight".  An empty line --
 * the one the reference's `while(!f.eof())` reads after the file's last newline -- becomes a node exactly as there (child of
 * the root, no word, weight 0; its descriptor, left unset by the reference, is zero here).  NULL + orbfe_last_error() on failure. */
orbfe_vocabulary* orbfe_vocabulary_load_text(const char* filename, int device);
/* The same tree from arrays: nodes 1..nnodes in file order (the root, node 0, is implicit; parent[i] refers to node ids, so
 * parent[i] <= i); descriptors nnodes x 32 bytes; weights as parsed. */
orbfe_vocabulary* orbfe_vocabulary_create(int k, int L, int scoring, int weighting, int nnodes, const int32_t* parent,
                                          const uint8_t* is_leaf, const uint8_t* descriptors, const double* weights, int device);
void orbfe_vocabulary_destroy(orbfe_vocabulary* v);
int orbfe_vocabulary_info(const orbfe_vocabulary* v, int32_t* out6); /* k, L, scoring, weighting, nodes (incl. root), words */

/* transform(features, v, fv, levelsup) (TemplatedVocabulary.h:1127-1194) for one frame, host pointers.  Per feature
 * (each may be NULL): word_id, node_id (the ancestor at level L - levelsup, :1218-1259), weight.  The two vectors (all
 * seven pointers or none): BowVector as *nbow (word id ascending, value) pairs; FeatureVector as *nfv node ids ascending
 * with fv_offset[0..*nfv] into fv_feature (feature indices ascending within a node).  Capacity of every array: n
 * (fv_offset: n + 1).  Bit-exact doubles: weights are added and normalised in the reference's map order.
 * n > 4096 with vectors is ORBFE_ERR_CAPACITY. */
int orbfe_vocabulary_transform(orbfe_vocabulary* v, const uint8_t* desc, int n, int levelsup, int32_t* word_id, int32_t* node_id,
                               double* weight, uint32_t* bow_word, double* bow_value, int32_t* nbow, uint32_t* fv_node,
                               int32_t* fv_offset, uint32_t* fv_feature, int32_t* nfv);
/* Batch on the device over the extractor's output (blocks of `capacity` records per frame, d_n[f] valid; fv_offset
 * blocks are capacity + 1).  d_word / d_node / d_weight are required (scratch for the vector kernel).
 * A frame transforms its first min(d_n[f], capacity) descriptors, a negative count is 0.  Written per frame: that many entries of
 * d_word / d_node / d_weight, d_nbow[f] entries of the BowVector, d_nfv[f] node ids, d_nfv[f] + 1 offsets and
 * d_fv_offset[f][d_nfv[f]] feature indices; everything behind them in a block is left alone.  An empty frame gives
 * d_nbow[f] = d_nfv[f] = 0 and d_fv_offset[f][0] = 0.  Asynchronous on `stream`. */
int orbfe_vocabulary_transform_batch_device(orbfe_vocabulary* v, const uint8_t* d_desc, const int32_t* d_n, int capacity, int nframes,
                                            int levelsup, int32_t* d_word, int32_t* d_node, double* d_weight, uint32_t* d_bow_word,
                                            double* d_bow_value, int32_t* d_nbow, uint32_t* d_fv_node, int32_t* d_fv_offset,
                                            uint32_t* d_fv_feature, int32_t* d_nfv, void* stream);

/* ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (src/ORBmatcher.cc:159-292) and SearchByBoW(KeyFrame*,
 * KeyFrame*, vpMatches12) (:526-659) on flat arrays: side 1 = the keyframe whose map points are looked for, side 2 = the
 * frame / second keyframe, each with the FeatureVector orbfe_vocabulary_transform returned.  valid1[i] != 0 = "feature i has
 * a map point that is not bad" (:196-201; NULL = all); valid2 the same for side 2 (the KF-KF variant, :583-590; NULL = the
 * KF-Frame variant).  The variants also differ in accept_max (best <= TH_LOW = 50, :233, vs best < TH_LOW, :608 -> 49) and
 * factor (this fork's HISTO_LENGTH / 360.0f, :174, vs 1.0f / HISTO_LENGTH, :546).  match12[i1] = i2 or -1 and match21[i2] =
 * i1 or -1 (vpMapPointMatches[i2] = map point of match21[i2]; vpMatches12[i1] = map point of match12[i1]); *nmatches is the
 * return value.  At most 4096 features per side.  Host pointers. */
int orbfe_search_by_bow(const orbfe_keypoint* kps1, const uint8_t* desc1, const uint8_t* valid1, int n1, const uint32_t* fv_node1,
                        const int32_t* fv_offset1, const uint32_t* fv_feature1, int nfv1, const orbfe_keypoint* kps2,
                        const uint8_t* desc2, const uint8_t* valid2, int n2, const uint32_t* fv_node2, const int32_t* fv_offset2,
                        const uint32_t* fv_feature2, int nfv2, float nnratio, int check_orientation, int accept_max, float factor,
                        int32_t* match12, int32_t* match21, int32_t* nmatches, int device);
/* Batch over npairs pairs of frames of one set of per-frame blocks (the layouts of orbfe_extract_batch_device and
 * orbfe_vocabulary_transform_batch_device; d_valid may be NULL): pair p matches frame d_pair1[p] (side 1) with frame
 * d_pair2[p] (side 2); NULL index arrays mean p and p + 1.  use_valid2 != 0 applies d_valid to side 2 as well.
 * d_match12 / d_match21 are blocks of `capacity` per pair: min(d_n[f], capacity) entries are written for the pair's side-1 resp.
 * side-2 frame (a negative count is 0), the rest of a block is left alone; d_nmatches[p] is always written.  A frame may be paired
 * with itself and a pair may occur twice.  Asynchronous on `stream`. */
int orbfe_search_by_bow_batch_device(const orbfe_keypoint* d_kps, const uint8_t* d_desc, const uint8_t* d_valid, const int32_t* d_n,
                                     const uint32_t* d_fv_node, const int32_t* d_fv_offset, const uint32_t* d_fv_feature,
                                     const int32_t* d_nfv, int capacity, const int32_t* d_pair1, const int32_t* d_pair2, int npairs,
                                     int use_valid2, float nnratio, int check_orientation, int accept_max, float factor,
                                     int32_t* d_match12, int32_t* d_match21, int32_t* d_nmatches, void* stream);

/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo = false) (src/ORBmatcher.cc:661-827),
 * monocular: features of the two keyframes without a map point (has_mp* != 0 = skip, :710-714, :731-735; NULL = none has
 * one), paired per vocabulary node, distance <= TH_LOW, not within 10 px * sqrt(scale) of the epipole (ex, ey) (:752-757,
 * the caller computes it, :669-675), within the 3.84 sigma^2 band of the epipolar line x1' F12 (CheckDistEpipolarLine,
 * :139-157; F12 3x3 row-major), rotation histogram with factor 1/HISTO_LENGTH.  scale_factors2 / level_sigma2_2 =
 * pKF2->mvScaleFactors / mvLevelSigma2.  match12[i1] = i2 or -1: vMatchedPairs = the pairs in ascending i1. */
int orbfe_search_for_triangulation(const orbfe_keypoint* kps1, const uint8_t* desc1, const uint8_t* has_mp1, int n1, const uint32_t* fv_node1,
                                   const int32_t* fv_offset1, const uint32_t* fv_feature1, int nfv1, const orbfe_keypoint* kps2,
                                   const uint8_t* desc2, const uint8_t* has_mp2, int n2, const uint32_t* fv_node2, const int32_t* fv_offset2,
                                   const uint32_t* fv_feature2, int nfv2, const float* F12, float ex, float ey, const float* scale_factors2,
                                   const float* level_sigma2_2, int nlevels, int check_orientation, int32_t* match12, int32_t* nmatches,
                                   int device);
/* Batch over pairs of frames as orbfe_search_by_bow_batch_device; d_free[i] != 0 = "feature i has no map point" (NULL = all),
 * d_F12 npairs x 9 and d_epipole npairs x 2 on the device, the level tables on the host; d_scratch21 = capacity ints per pair.
 * Counts and written rows as there.  An all-zero F12 has no epipolar line: 0 matches. */
int orbfe_search_for_triangulation_batch_device(const orbfe_keypoint* d_kps, const uint8_t* d_desc, const uint8_t* d_free, const int32_t* d_n,
                                                const uint32_t* d_fv_node, const int32_t* d_fv_offset, const uint32_t* d_fv_feature,
                                                const int32_t* d_nfv, int capacity, const int32_t* d_pair1, const int32_t* d_pair2, int npairs,
                                                const float* d_F12, const float* d_epipole, const float* scale_factors,
                                                const float* level_sigma2, int nlevels, int check_orientation, int32_t* d_match12,
                                                int32_t* d_scratch21, int32_t* d_nmatches, void* stream);

/* ------------------------------------------------------------ local mapping: CreateNewMapPoints -- */
/* LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:222-467), monocular: the geometry between the covisibility query and the
 * object-graph lines :449-464.  Per neighbour keyframe: the baseline / median-depth gate (:259-276), ComputeF12 (:904-921), the
 * epipole of SearchForTriangulation (src/ORBmatcher.cc:668-674), that search, and per match (:306-446) the ray-parallax gate, the
 * 4 x 4 DLT (cv::SVD, CV_32F), two cheirality gates, two chi-square gates (5.991 sigma2) and the scale-consistency gate; for a point
 * that passes, MapPoint::UpdateNormalAndDepth of a two-observation point whose reference keyframe is the current one
 * (src/MapPoint.cc:359-400).  Numerics: OpenCV 3.4's for CV_32F -- Mat products and dot products accumulate in double and round
 * once, cv::norm is a double sum of float squares and a double square root, 3 x 3 inverses are cofactor formulas in double, "m / s"
 * multiplies by (float)(1. / s); a float error is compared against the double product 5.991 * sigma2.  OpenCV itself is not part
 * of the tests: parity is against a CPU restatement of the same conventions (tests/new_points_ref.cpp).
 *
 * Resident layout, as the Sim3 and the triangulation-search calls: per-frame blocks of `capacity` entries of d_kps (mvKeysUn),
 * d_x3Dw (x 3), d_valid ("has a map point"), d_free ("has no map point": the flags of the search) and d_n (clamped to the block, a
 * negative count is 0); d_Tcw 12 floats a frame (3 x 4 row-major); pair p is the current keyframe d_pair1[p] (side 1) against the
 * neighbour d_pair2[p] (NULL index arrays: p and p + 1); K4 = fx, fy, cx, cy, one for both sides; the level tables
 * (mvScaleFactors, mvLevelSigma2, nlevels <= 16) on the host.
 *
 * Status byte per side-1 feature (ORBFE_NMP_*): 0 no match, 1 created, 2 parallax gate (!(cos > 0 && cos < 0.9998)), 3 w == 0,
 * 4 a point that is not finite, 5 z1 <= 0, 6 z2 <= 0, 7 reprojection error in keyframe 1, 8 in keyframe 2, 9 a zero distance,
 * 10 scale consistency.
 *
 * Where the reference is undefined:
 *   - a neighbour with no map point (the reference reads vDepths[-1 / 2] of an empty vector): the pair is skipped, median_depth 0;
 *   - a triangulated point that is not finite would pass every comparison (NaN compares false) and become a map point: it is
 *     rejected with status 4.  A STATED DEVIATION from the reference;
 *   - an octave outside [0, nlevels) on a matched feature: the pair's record has status ORBFE_ERR_INVALID and every other field 0,
 *     nothing else of that pair is written (status bytes, outputs, map state); the other pairs of the call are unaffected;
 *   - a match12 entry outside [-1, d_n[f2]) counts as no match. */
#define ORBFE_NMP_NO_MATCH 0
#define ORBFE_NMP_CREATED 1
#define ORBFE_NMP_PARALLAX 2
#define ORBFE_NMP_W_ZERO 3
#define ORBFE_NMP_NOT_FINITE 4
#define ORBFE_NMP_Z1 5
#define ORBFE_NMP_Z2 6
#define ORBFE_NMP_REPROJECTION1 7
#define ORBFE_NMP_REPROJECTION2 8
#define ORBFE_NMP_ZERO_DISTANCE 9
#define ORBFE_NMP_SCALE 10

typedef struct orbfe_new_points_pair {
    float   baseline;           /* cv::norm(Ow2 - Ow1) */
    float   median_depth;       /* pKF2->ComputeSceneMedianDepth(2): the (m - 1) / 2-th smallest depth; 0 when m = 0 */
    int32_t n_depths;           /* m: features of the neighbour with a map point */
    int32_t skipped;            /* 1: baseline / median_depth < 0.01 (the reference's `continue`), or m = 0 */
} orbfe_new_points_pair;

typedef struct orbfe_new_points_result {
    int32_t n_matches;          /* entries of the pair's match12 inside [0, d_n[f2]): vMatchedIndices.size() */
    int32_t n_new;              /* nnew of this neighbour: status bytes equal to 1 */
    int32_t status;             /* ORBFE_OK, or ORBFE_ERR_INVALID for a pair that was not processed (see above) */
} orbfe_new_points_result;

/* The gate and the inputs of the search, for npairs pairs in one launch (one workgroup per pair): d_prep[p], d_F12 (npairs x 9,
 * row-major) and d_epipole (npairs x 2) as orbfe_search_for_triangulation_batch_device reads them.  The depths are
 * z = (float)(Tcw2 row 2 . x3Dw in double + (double)zcw) over the neighbour's features with d_valid != 0 (NULL = all); the gate
 * compares (double)(baseline / median_depth) < 0.01.  A skipped pair gets an all-zero F12 and epipole: the search then finds no match
 * and the triangulation has nothing to do, so a chain needs no host decision.  Asynchronous on `stream`, no scratch. */
int orbfe_new_points_prepare_batch_device(const int32_t* d_n, int capacity, const float* d_x3Dw, const uint8_t* d_valid, const float* d_Tcw,
                                          const int32_t* d_pair1, const int32_t* d_pair2, int npairs, const float* K4, float* d_F12,
                                          float* d_epipole, orbfe_new_points_pair* d_prep, void* stream);

/* Lines :306-446 for every match of npairs pairs in one launch (one thread per side-1 feature).  d_match12: blocks of `capacity`
 * per pair, match12[i1] = i2 or -1, as the search writes them.  Outputs, blocks of `capacity` per pair, slot i1 (ascending i1 is
 * the reference's creation order, ORBmatcher.cc:816-824): d_status (the first d_n[f1] bytes are written), and for status 1 d_x3D (x 3),
 * d_normal (x 3: mNormalVector) and d_dist (x 2: mfMaxDistance, mfMinDistance); the slots of other codes are left alone.  d_res[p]
 * is always written.
 * The map state is updated in place where status is 1, and nowhere else: d_free[f1][i1] = d_free[f2][i2] = 0, d_valid[..] = 1,
 * d_x3Dw[..] = x3D (the three arrays are all given or all NULL: outputs only).  Within one pair i1 and i2 are each unique, so these
 * writes do not race.  ALL PAIRS OF ONE CALL SEE THE MATCH LISTS AS THEY WERE GIVEN: two pairs of one call that share a frame may
 * both create a point on the same feature, and which of the two the state arrays then hold is not defined.  The reference's
 * sequential order -- a feature that received a point from neighbour p is no longer free for neighbour p + 1 -- is what
 * orbfe_create_new_map_points_device is for.  The call itself does not read the state arrays.
 * Asynchronous on `stream` (one memset of d_res and one launch), no host synchronisation, no scratch. */
int orbfe_triangulate_matches_batch_device(const orbfe_keypoint* d_kps, const int32_t* d_n, int capacity, float* d_x3Dw, uint8_t* d_valid,
                                           uint8_t* d_free, const float* d_Tcw, const int32_t* d_pair1, const int32_t* d_pair2, int npairs,
                                           const int32_t* d_match12, const float* K4, const float* scale_factors, const float* level_sigma2,
                                           int nlevels, float ratio_factor, uint8_t* d_status, float* d_x3D, float* d_normal, float* d_dist,
                                           orbfe_new_points_result* d_res, void* stream);

/* The product call: CreateNewMapPoints of resident keyframes.  One orbfe_new_points_prepare_batch_device over all pairs (on the
 * state at entry), then STRICTLY IN LIST ORDER, per pair: orbfe_search_for_triangulation_batch_device on that one pair (with d_free
 * as it is by then) and the triangulation of that pair, which clears d_free where it created a point -- the reference's skip of
 * ORBmatcher.cc:710-714 for the next neighbour.  Everything is enqueued on `stream` with no host synchronisation:
 * 1 + npairs x (1 search launch + 1) kernel launches (41 for 20 neighbours), one memset.  The per-frame arrays of the search
 * (d_desc, the FeatureVector blocks d_fv_node / d_fv_offset (capacity + 1 a frame) / d_fv_feature / d_nfv) and its outputs
 * d_match12, d_scratch21 (capacity ints a pair) and d_nmatches are those of that call; every other argument is that of the two
 * calls above.  The caller ends the pair list where CheckNewKeyFrames() would return, and passes ratio_factor = 1.5f * mfScaleFactor. */
int orbfe_create_new_map_points_device(const orbfe_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, const uint32_t* d_fv_node,
                                       const int32_t* d_fv_offset, const uint32_t* d_fv_feature, const int32_t* d_nfv, int capacity,
                                       float* d_x3Dw, uint8_t* d_valid, uint8_t* d_free, const float* d_Tcw, const int32_t* d_pair1,
                                       const int32_t* d_pair2, int npairs, const float* K4, const float* scale_factors,
                                       const float* level_sigma2, int nlevels, float ratio_factor, int check_orientation, float* d_F12,
                                       float* d_epipole, orbfe_new_points_pair* d_prep, int32_t* d_match12, int32_t* d_scratch21,
                                       int32_t* d_nmatches, uint8_t* d_status, float* d_x3D, float* d_normal, float* d_dist,
                                       orbfe_new_points_result* d_res, void* stream);

/* One neighbour, host pointers: both keyframes are staged once, prepare, search and triangulation run on the stage, one download.
 * Side k: kps, descriptors, its FeatureVector (orbfe_vocabulary_transform), x3Dw (n x 3) and valid (n; 1 = has a map point) -- both
 * IN / OUT: a created point is written to both sides -- and Tcw.  Outputs, n1 entries: match12, status, x3D, normal, dist (x 2);
 * F12 (9), epipole (2), prep and res.  The caller walks the neighbours in order and hands the current keyframe's x3Dw / valid from
 * call to call: that is the sequence of the device chain. */
int orbfe_create_new_map_points(const orbfe_keypoint* kps1, const uint8_t* desc1, int n1, const uint32_t* fv_node1, const int32_t* fv_offset1,
                                const uint32_t* fv_feature1, int nfv1, float* x3Dw1, uint8_t* valid1, const float* Tcw1,
                                const orbfe_keypoint* kps2, const uint8_t* desc2, int n2, const uint32_t* fv_node2, const int32_t* fv_offset2,
                                const uint32_t* fv_feature2, int nfv2, float* x3Dw2, uint8_t* valid2, const float* Tcw2, const float* K4,
                                const float* scale_factors, const float* level_sigma2, int nlevels, float ratio_factor, int check_orientation,
                                float* F12, float* epipole, orbfe_new_points_pair* prep, int32_t* match12, uint8_t* status, float* x3D,
                                float* normal, float* dist, orbfe_new_points_result* res, int device);

/* DIAGNOSTIC / TEST INTERFACE, no stability promise: the triangulation of one pair's given match list with its gate quantities
 * (the parity tests).  No map state.  quantities: n1 x 6 = cosParallaxRays, the squared reprojection errors in keyframe 1 and 2,
 * dist1, dist2, ratioOctave; a quantity behind the gate that rejected the match is 0.  The other outputs as above. */
int orbfe_new_points_inspect(const orbfe_keypoint* kps1, int n1, const float* Tcw1, const orbfe_keypoint* kps2, int n2, const float* Tcw2,
                             const int32_t* match12, const float* K4, const float* scale_factors, const float* level_sigma2, int nlevels,
                             float ratio_factor, uint8_t* status, float* x3D, float* normal, float* dist, float* quantities,
                             orbfe_new_points_result* res, int device);

/* ------------------------------------------------------------ LocalBundleAdjustment (local mapping) -- */
/* Optimizer::LocalBundleAdjustment(KeyFrame*, bool*, Map*) (src/Optimizer.cc:772-1242) behind its collect step (:777-888), on flat
 * arrays: g2o's Levenberg-Marquardt with BlockSolver_6_3 restated in double -- optimize(5) over all edges with Huber
 * (delta = (double)sqrtf(5.991f)), the first check (a monocular edge whose cached chi2 > 5.991 or whose depth is not positive, and a
 * marker edge whose chi2 > 5.991, go to level 1; Huber comes off every edge), optimize(10) on level 0 from the first round's
 * estimates, the second check (the erase list) and the write-back.
 *
 * The problem:
 *   - pose vertices 0 .. nkf-1: Tcw (12 floats each, 3 x 4 row-major, IN / OUT) and kf_fixed[k] (1 = lFixedCameras and the keyframe
 *     with mnId 0; 0 = the other local keyframes).  The caller's order is the local keyframes in list order, then the fixed ones;
 *   - points 0 .. np-1: x3Dw (np x 3 floats, IN / OUT);
 *   - observations in CSR by point (obs_offset[np + 1], starting at 0, non-decreasing), in the point's GetObservations() order (the
 *     order g2o adds the edges).  Two forms: obs_kf / obs_xy (x, y) / obs_octave, or -- the device call only, d_obs_xy == NULL --
 *     obs_kf / obs_feature into d_kps blocks of `capacity` keypoints a keyframe (the layout of orbfe_extract_batch_device), so that
 *     the call chains behind orbfe_create_new_map_points_device without repacking keypoints.  A keyframe observes a point once;
 *   - one K4 = fx, fy, cx, cy; inv_level_sigma2[nlevels] = mvInvLevelSigma2, nlevels <= 32;
 *   - markers 0 .. nma-1: Twm (12 floats, IN / OUT) and marker_local (12 floats: get3DPointsLocalRefSystem(0 .. 3)), as in
 *     orbfe_pose_marker; their observations in CSR by marker (mobs_offset[nma + 1]) in GetObservations() order, each a keyframe index
 *     and the 8 floats of mvArucoUn[4 idx .. 4 idx + 3]; four EdgeMarker edges an observation, information marker_info * I (the
 *     reference's wei = 25);
 *   - use_markers = Frame::mbUArucoIni: with 0 no marker vertex or edge exists and Twm is not written.
 * EdgeSE3ProjectXYZ has g2o's analytic Jacobians; EdgeMarker (error = obs - pi((Tcw Twm) p)) g2o's numeric ones on both vertices:
 * central differences, delta = 1e-9, through exp(+-delta e_d) T, none for a fixed vertex.  A fixed vertex has no Hessian block.
 * LM as g2o runs it: lambda0 = 1e-5 x the largest diagonal entry over pose and point blocks, lambda on both, up to 10 trials an
 * iteration, rho = dchi2 / (sum x (lambda x + b) + 1e-3) over all vertices, g2o's lambda / nu and stop rules (and the vendored
 * "three iterations that gain less than 0.1 %" rule), lambda anew in each optimize().  The point blocks are marginalised:
 * S = Hpp - sum Hpl Hll^-1 Hpl^T (Hll^-1 by cofactors, as Eigen inverts a 3 x 3), the dense S is factorised L L^T without pivoting
 * (a pivot that is not positive and finite fails the solve: a failed trial with chi2 = DBL_MAX, the update of the last solve that
 * succeeded applied as in g2o), the points follow by back-substitution.  A vertex all of whose edges are at level 1 is not part of
 * the system and does not move; neither does a free keyframe without observations.
 * Where the reference is undefined: an edge whose error or Jacobian is not finite adds nothing to H and b in that pass (its chi2
 * still enters the sums, so that trial is rejected); a chi2 that is not finite at a check is bad.
 *
 * Outputs: Tcw of the keyframes with kf_fixed = 0 (floats as Converter::toCvMat(SE3Quat) makes them; the fixed ones are left as they
 * are -- SetPose of the mnId 0 keyframe with its own pose is the shim's), x3Dw, Twm (use_markers), erase[e] = 1 for observation slot e
 * of the erase list (one byte per slot, CSR order: vToErase is the slots with 1 in ascending order) and the record.
 * MapPoint::UpdateNormalAndDepth is NOT done here: it needs the reference keyframe, the observations' levels and the scale factors of
 * every observing keyframe, which the device function of new_map_points.hip (two observations, fresh point) does not take; it stays
 * the shim's host call.
 *
 * stop (the reference's pbStopFlag, may be NULL): read at the call -- nonzero returns ORBFE_OK with status ORBFE_LBA_STOPPED and
 * nothing else written (the reference returns before initializeOptimization) -- and, by the device call, at the start of every LM
 * iteration, trial and round (d_stop must then stay readable by the device: device memory or mapped host memory): a set flag ends
 * that optimize(), skips round 2 (bDoMore = false), and the second check and the write-back still run.  LIMITATION, to be lifted:
 * the host call reads it at the call only (the flag is the caller's host byte, which the kernels cannot see; a caller that needs
 * the abort inside a call uses the device call with a mapped byte).  Only the set-before-the-call case can be tested
 * deterministically.
 *
 * ORBFE_ERR_CAPACITY: free pose vertices (keyframes with kf_fixed = 0, plus the markers when use_markers) above
 * ORBFE_LBA_MAX_FREE_POSES, or a point with more than ORBFE_LBA_MAX_OBSERVATIONS observations.  ORBFE_ERR_INVALID: NULLs, offsets
 * that do not start at 0 or decrease, a keyframe or feature index out of range, a keyframe that observes a point twice, an octave
 * outside [0, nlevels), inputs that are not finite.  The host call returns these; the device call, which cannot look at device
 * data without synchronising, returns them for what it can see on the host and writes the rest to d_res->status, and then writes
 * nothing else.  iterations and stale_mask are diagnostics as in orbfe_pose_result.
 *
 * Scaling: the (keyframe, point) -> edge index is a dense table of nkf x np ints in the scratch (nkf x np < 2^30, ORBFE_ERR_INVALID
 * beyond; orbfe_lba_scratch_bytes says what that costs: 0.5 MB of its 18 MB at 40 keyframes x 3 000 points), and the kernels that
 * build a pose block or a block of the reduced system walk all np points once per block, whatever the number of observations.
 * That is sized for local mapping (tens of keyframes, thousands of points); a map-sized problem is orbfe_global_bundle_adjustment's (lists by
 * vertex and by covisible pair, a block-sparse reduced system). */
#define ORBFE_LBA_MAX_FREE_POSES 64
#define ORBFE_LBA_MAX_OBSERVATIONS 256
#define ORBFE_LBA_STOPPED 1

typedef struct orbfe_lba_result {
    int32_t n_edges_mono;       /* EdgeSE3ProjectXYZ edges = observation slots */
    int32_t n_edges_marker;     /* EdgeMarker edges: 4 x marker observations (0 without use_markers) */
    int32_t n_level1[2];        /* edges the first check sent to level 1: monocular, marker */
    int32_t n_erase;            /* entries of the erase list */
    int32_t iterations[2];      /* DIAGNOSTIC: LM iterations of the two optimize() calls */
    int32_t stale_mask;         /* DIAGNOSTIC: bit r = round r ended on a rejected trial (the check after it read that trial's errors) */
    int32_t status;             /* ORBFE_OK, ORBFE_LBA_STOPPED, or the device call's ORBFE_ERR_INVALID / ORBFE_ERR_CAPACITY (see above) */
} orbfe_lba_result;

/* Bytes of scratch orbfe_local_bundle_adjustment_device needs for a problem of these sizes (0 for negative sizes). */
size_t orbfe_lba_scratch_bytes(int nkf, int np, int nobs, int nma, int nmobs);

/* Host pointers; one upload, the chain below, one download, one synchronisation.  Gives the bits of the device call. */
int orbfe_local_bundle_adjustment(float* Tcw, const uint8_t* kf_fixed, int nkf, float* x3Dw, int np, const int32_t* obs_offset,
                                  const int32_t* obs_kf, const float* obs_xy, const int32_t* obs_octave, int nobs, const float* K4,
                                  const float* inv_level_sigma2, int nlevels, float* Twm, const float* marker_local, int nma,
                                  const int32_t* mobs_offset, const int32_t* mobs_kf, const float* mobs_corners, int nmobs, float marker_info,
                                  int use_markers, const uint8_t* stop, uint8_t* erase, orbfe_lba_result* res, int device);

/* Device pointers (K4 and inv_level_sigma2 are host arrays read at the call).  The call allocates nothing: d_scratch holds
 * scratch_bytes >= orbfe_lba_scratch_bytes(...) bytes, 256-byte aligned.  Everything is enqueued on `stream` with no host
 * synchronisation between entry and the last launch.  The LM state -- lambda, nu, both copies of the estimates, the "accepted / done /
 * solve failed" flags, the counters -- lives in the scratch, and the sequence of launches does not depend on the problem: a launch
 * that finds its step already decided returns at once.  Two memsets, then 1 launch of setup, per round 1 + iterations x (3 +
 * 10 trials x 5) launches (5 and 10 iterations), a check behind each round and 1 launch of write-back: 1 + 2 x 1 + 15 x 53 + 2 + 1 =
 * 801 launches whatever the problem.  Every sum has an order that depends on the problem's sizes alone (no floating-point atomics). */
int orbfe_local_bundle_adjustment_device(float* d_Tcw, const uint8_t* d_kf_fixed, int nkf, float* d_x3Dw, int np, const int32_t* d_obs_offset,
                                         const int32_t* d_obs_kf, const float* d_obs_xy, const int32_t* d_obs_octave,
                                         const int32_t* d_obs_feature, const orbfe_keypoint* d_kps, int capacity, int nobs, const float* K4,
                                         const float* inv_level_sigma2, int nlevels, float* d_Twm, const float* d_marker_local, int nma,
                                         const int32_t* d_mobs_offset, const int32_t* d_mobs_kf, const float* d_mobs_corners, int nmobs,
                                         float marker_info, int use_markers, const uint8_t* d_stop, uint8_t* d_erase, orbfe_lba_result* d_res,
                                         void* d_scratch, size_t scratch_bytes, void* stream);

/* DIAGNOSTIC / TEST INTERFACE, no stability promise: one linearisation at the given estimates (all edges, Huber) and the first LM
 * trial.  Host pointers; the problem as above, nothing of it is written.  *nv = free pose vertices (keyframes in order, then markers);
 * b (6 nv, then 3 np), Hpp (nv x 36, the diagonal blocks row-major), Hll (np x 6: the upper triangle xx xy xz yy yz zz), chi2 (the
 * robust chi2 and lambda0), x (6 nv, then 3 np: the first trial's update).  Arrays sized for ORBFE_LBA_MAX_FREE_POSES vertices. */
int orbfe_lba_inspect(const float* Tcw, const uint8_t* kf_fixed, int nkf, const float* x3Dw, int np, const int32_t* obs_offset,
                      const int32_t* obs_kf, const float* obs_xy, const int32_t* obs_octave, int nobs, const float* K4,
                      const float* inv_level_sigma2, int nlevels, const float* Twm, const float* marker_local, int nma,
                      const int32_t* mobs_offset, const int32_t* mobs_kf, const float* mobs_corners, int nmobs, float marker_info,
                      int use_markers, int32_t* nv, double* b, double* Hpp, double* Hll, double* chi2, double* x, int device);

/* ------------------------------------------------------------ OptimizeEssentialGraph (loop closing's pose graph) -- */
/* Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1245-1542, called by LoopClosing::CorrectLoopByAruco with bFixScale = true)
 * behind its collect step: Sim3 vertices, EdgeSim3 edges with identity information, g2o's Levenberg-Marquardt with
 * setUserLambdaInit(1e-16), then the SE3 recovery of every keyframe and the correction of every map point.  Flat arrays in the
 * reference's vpKFs order ("positions" 0 .. nkf - 1; bad keyframes are left out by the caller), nothing pointer-shaped.
 *   keyframes   kf_id[nkf] (mnId; read for the messages of orbfe_last_error alone, may be NULL), Tcw[nkf][12] (3 x 4 row-major),
 *               fixed (the position of pLoopKF), corrected_pos[nc] + corrected[nc][8] (CorrectedSim3) and noncorrected_pos[nn] +
 *               noncorrected[nn][8] (NonCorrectedSim3): quaternion x y z w, t, s in double, as g2o::Sim3 holds them; a position
 *               at most once in each list.  vScw of a keyframe is its CorrectedSim3 entry, else Sim3(Rcw, tcw, 1)
 *   edges       in the order the reference adds them: edge_i[ne] (vertex 0), edge_j[ne] (vertex 1), edge_kind[ne].  Kind 0
 *               (LoopConnections, :1316-1344) measures vScw[j] * vScw[i]^-1; kind 1 (spanning tree, old loop edges, covisibility,
 *               :1347-1447) measures the same with the NonCorrectedSim3 entry of a keyframe that has one.  Two edges on one pair
 *               are legal and both count
 *   points      x3Dw[np][3], point_ref[np]: the position of the keyframe whose id the reference calls nIDr (:1487-1496), -1
 *               leaves the point as it is
 *   options     iterations (the reference: 20, at most 20), fix_scale, leaf_vertices (the elimination plan's leaf size, 0 = default)
 * Outputs: Tcw_out[nkf][12] (the corrected Siw as [R t/s], :1462-1473), x3Dw_out[np][3] (correctedSwr.map(Srw.map(P)) in double,
 * then float), Siw_out[nkf][8] (may be NULL), the record.  nkf == 1 or ne == 0 is a legal call that returns its inputs.
 * ORBFE_ERR_INVALID: NULLs, positions out of range, a self edge, an edge kind other than 0 / 1, a pose, similarity or point that is
 * not finite, `fixed` out of range, a scale <= 0.  ORBFE_ERR_CAPACITY: more than ORBFE_EG_MAX_KEYFRAMES keyframes or
 * ORBFE_EG_MAX_EDGES edges (at these the scratch is 0.9 GB), or a graph whose elimination fronts need more than the 768 MB of
 * scratch set aside for them (a graph that dense is no essential graph).  A refused call writes nothing. */
#define ORBFE_EG_MAX_KEYFRAMES 4096
#define ORBFE_EG_MAX_EDGES 65536

typedef struct orbfe_eg_result {
    int32_t status;       /* ORBFE_OK, or the device call's ORBFE_ERR_INVALID (values it could only check on the device) */
    int32_t iterations;   /* iterations run */
    int32_t trials;       /* LM trials run over all iterations */
    int32_t pad;
    double chi2_first, chi2_last, lambda_last;
} orbfe_eg_result;

/* bytes of device scratch a problem of these sizes needs, whatever its graph; 0: sizes out of range */
size_t orbfe_essential_graph_scratch_bytes(int nkf, int nedges, int npoints, int leaf_vertices);

/* host pointers, one call, synchronous */
int orbfe_optimize_essential_graph(const int32_t* kf_id, const float* Tcw, int nkf, int fixed, const int32_t* corrected_pos,
                                   const double* corrected, int nc, const int32_t* noncorrected_pos, const double* noncorrected, int nn,
                                   const int32_t* edge_i, const int32_t* edge_j, const int32_t* edge_kind, int ne, const float* x3Dw,
                                   const int32_t* point_ref, int np, int iterations, int fix_scale, int leaf_vertices, float* Tcw_out,
                                   float* x3Dw_out, double* Siw_out, orbfe_eg_result* res, int device);

/* The values on the device (d_*), the graph -- kf_id, edge_i, edge_j, edge_kind -- on the host: the elimination plan is made from it
 * before anything is enqueued.  Everything runs on `stream` with no host synchronisation (a second call on one stream waits, on the
 * host, until the first one's tables have left their staging block); the worst case of 20 x 10 trials is enqueued and decided steps
 * fall through.  d_scratch: scratch_bytes >= orbfe_essential_graph_scratch_bytes(...) bytes, 256-byte aligned.  What only the device
 * can check (values that are not finite, scales, positions of the similarity lists and of point_ref) comes back as d_res->status,
 * with no output written. */
int orbfe_optimize_essential_graph_device(const int32_t* kf_id, const float* d_Tcw, int nkf, int fixed, const int32_t* d_corrected_pos,
                                          const double* d_corrected, int nc, const int32_t* d_noncorrected_pos, const double* d_noncorrected,
                                          int nn, const int32_t* edge_i, const int32_t* edge_j, const int32_t* edge_kind, int ne,
                                          const float* d_x3Dw, const int32_t* d_point_ref, int np, int iterations, int fix_scale,
                                          int leaf_vertices, float* d_Tcw_out, float* d_x3Dw_out, double* d_Siw_out, orbfe_eg_result* d_res,
                                          void* d_scratch, size_t scratch_bytes, void* stream);

/* DIAGNOSTIC / TEST INTERFACE, no stability promise: one linearisation and one solve at lambda0.  err (ne x 7), Ji and Jj (ne x 49,
 * row-major 7 x 7; zeros for the fixed vertex), Hd (nkf x 49, the diagonal blocks) and b (nkf x 7) in the caller's positions, chi2
 * (chi2, lambda0, 1 when every pivot was positive), x (nkf x 7, caller's positions), tree (2 + 2 nkf + 4 nodes, at most 10 nkf + 10
 * entries: nodes, levels; node and place in the elimination order of every vertex, -1 the fixed one; parent, level, own and boundary
 * vertices of every node). */
int orbfe_essential_graph_inspect(const int32_t* kf_id, const float* Tcw, int nkf, int fixed, const int32_t* corrected_pos,
                                  const double* corrected, int nc, const int32_t* noncorrected_pos, const double* noncorrected, int nn,
                                  const int32_t* edge_i, const int32_t* edge_j, const int32_t* edge_kind, int ne, int fix_scale,
                                  int leaf_vertices, double* err, double* Ji, double* Jj, double* Hd, double* b, double* chi2, double* x,
                                  int32_t* tree, int device);

/* ------------------------------------------------------------ GlobalBundleAdjustment (map-wide BA, sparse Schur) -- */
/* Optimizer::BundleAdjustment (src/Optimizer.cc:49-307; GlobalBundleAdjustemnt above it collects the whole map and calls it) behind
 * its collect step: ONE optimize(iterations) of g2o's Levenberg-Marquardt with BlockSolver_6_3 over keyframes, map points and this
 * fork's marker poses, in double.  The reference calls it from Tracking::CreateInitialMapMonocular (20 iterations, robust, two
 * keyframes) and from LoopClosing::RunGlobalBundleAdjustment (10 iterations, not robust), the step behind
 * orbfe_optimize_essential_graph.  Flat arrays laid out as orbfe_local_bundle_adjustment's, nothing pointer-shaped:
 *   keyframes   Tcw[nkf][12] (IN / OUT) and kf_fixed[nkf] (the shim sets it for mnId == 0).  Any number of fixed keyframes is legal,
 *               none included: keyframe 0 may be bad and left out
 *   points      x3Dw[np][3] (IN / OUT) with their observations in CSR by point (obs_offset, obs_kf and obs_xy / obs_octave, or -- the
 *               device call only -- obs_feature into d_kps blocks of `capacity` keypoints a keyframe), in GetObservations() order
 *   markers     Twm[nma][12] (IN / OUT), marker_local, mobs_offset, mobs_kf, mobs_corners, marker_info (the reference's wei = 25)
 *               and use_markers (Frame::mbUArucoIni), as in orbfe_local_bundle_adjustment
 *   camera      K4, inv_level_sigma2[nlevels], nlevels <= 32
 *   options     iterations (1 .. 20), robust (bRobust), stop (pbStopFlag, may be NULL), leaf_vertices (the elimination plan's leaf
 *               size, 0 = default, as in orbfe_optimize_essential_graph)
 * What differs from the local bundle adjustment, from the reference's lines:
 *   - one round: no levels, no chi2 checks, no erase list; the output is the estimates and the record;
 *   - robust != 0 puts Huber on every monocular edge with delta = (double)(float)sqrt(5.99) (5.99 here, :91, not 5.991);
 *   - the four EdgeMarker edges of a marker observation always carry Huber with that delta, whatever robust says (:218-220); their
 *     Jacobians are g2o's numeric ones;
 *   - a point without observations is no vertex (:157-161): its x3Dw is not written, and it counts in n_points_left_out.
 * As there: a free keyframe or marker without an edge is not part of the system and keeps its bits (a deviation: g2o would solve a
 * block that holds lambda alone and leave the estimate where it is, rounded through the quaternion); LM as g2o runs it
 * (lambda0 = 1e-5 x the largest diagonal entry over pose and point blocks, up to 10 trials an iteration, rho, the stop rules, a
 * failed solve as a trial with chi2 = DBL_MAX); an edge whose error or Jacobian is not finite adds nothing to H and b in that pass
 * while its chi2 still enters the sum, so the trial is rejected.
 *
 * The solve.  Lists index the blocks, not a dense (keyframe, point) table: the edges of every vertex, and the covisible pairs of
 * free vertices -- joined by a point or by a marker edge -- each with its items.  The reduced camera system S = Hpp - sum W D^-1 W^T
 * has one 6 x 6 block per covisible pair and is kept that way; it is factored L L^T without pivoting along the elimination tree of a
 * nested dissection on the caller's keyframe order (the essential graph's plan, 6 rows a vertex), one workgroup per front, with the
 * markers as own vertices of the root so that a marker seen along the whole trajectory pulls no keyframe into a separator.  No
 * kernel's work grows with nkf x np.  Every sum has an order fixed by the plan (no floating-point atomics): the host call, the device
 * call and a repeat give equal bits.
 *
 * stop: read at the call -- nonzero returns ORBFE_OK with status ORBFE_GBA_STOPPED and nothing else written -- and, by the device
 * call, at every iteration and trial (d_stop must then stay readable by the device): a set flag ends the optimize() and the
 * estimates of the last accepted trial are written.  The choice between SetPose and mTcwGBA / mPosGBA / mnBAGlobalForKF (nLoopKF,
 * :251-285) and MapPoint::UpdateNormalAndDepth are the shim's.
 *
 * ORBFE_ERR_CAPACITY: nkf + nma above ORBFE_GBA_MAX_POSES (checked by the sizes alone), a point with more than
 * ORBFE_GBA_MAX_OBSERVATIONS observations (the per-point kernels need no bound; the one on the pair items of the device call's
 * scratch, sized from the sizes alone, does), a scratch smaller than orbfe_gba_scratch_bytes says, or a covisibility graph whose
 * fronts need more than GBA_FRONT_BUDGET = 768 MB of scratch.  ORBFE_ERR_INVALID: the cases of orbfe_local_bundle_adjustment, and
 * iterations outside [1, 20].  The host call returns all of these; the device call returns what the host can see (the sizes, the
 * graph, the plan) and writes what only the device can check (values that are not finite, an octave or feature out of range) to
 * d_res->status, and then writes nothing else.  A refused call writes nothing. */
#define ORBFE_GBA_MAX_POSES 4096          /* keyframes plus markers: the value of ORBFE_EG_MAX_KEYFRAMES */
#define ORBFE_GBA_MAX_OBSERVATIONS 256    /* observations of one point: the value of ORBFE_LBA_MAX_OBSERVATIONS */
#define ORBFE_GBA_STOPPED 1

typedef struct orbfe_gba_result {
    int32_t status;             /* ORBFE_OK, ORBFE_GBA_STOPPED, or the device call's ORBFE_ERR_INVALID (see above) */
    int32_t iterations;         /* DIAGNOSTIC: LM iterations run */
    int32_t trials;             /* DIAGNOSTIC: LM trials run over all iterations */
    int32_t n_edges_mono;       /* EdgeSE3ProjectXYZ edges = observation slots */
    int32_t n_edges_marker;     /* EdgeMarker edges: 4 x marker observations (0 without use_markers) */
    int32_t n_points_left_out;  /* points without observations: no vertex, not written */
    double chi2_first, chi2_last, lambda_last;   /* the robust chi2 of the first linearisation and of the last accepted estimate */
} orbfe_gba_result;

/* bytes of device scratch orbfe_global_bundle_adjustment_device needs for a problem of these sizes, whatever its graph; 0: sizes out
 * of range */
size_t orbfe_gba_scratch_bytes(int nkf, int np, int nobs, int nma, int nmobs, int leaf_vertices);

/* host pointers, one call, synchronous */
int orbfe_global_bundle_adjustment(float* Tcw, const uint8_t* kf_fixed, int nkf, float* x3Dw, int np, const int32_t* obs_offset,
                                   const int32_t* obs_kf, const float* obs_xy, const int32_t* obs_octave, int nobs, const float* K4,
                                   const float* inv_level_sigma2, int nlevels, float* Twm, const float* marker_local, int nma,
                                   const int32_t* mobs_offset, const int32_t* mobs_kf, const float* mobs_corners, int nmobs, float marker_info,
                                   int use_markers, int iterations, int robust, const uint8_t* stop, int leaf_vertices, orbfe_gba_result* res,
                                   int device);

/* The values on the device (d_*), the graph -- kf_fixed, obs_offset, obs_kf, mobs_offset, mobs_kf -- on the host: the pair lists and
 * the elimination plan are made from it before anything is enqueued (K4 and inv_level_sigma2 are host arrays read at the call).
 * Everything runs on `stream` with no host synchronisation (a second call on one stream waits, on the host, until the first one's
 * tables have left their staging block); the worst case of iterations x 10 trials is enqueued and decided steps fall through.
 * d_scratch: scratch_bytes >= orbfe_gba_scratch_bytes(...) bytes, 256-byte aligned. */
int orbfe_global_bundle_adjustment_device(float* d_Tcw, const uint8_t* kf_fixed, int nkf, float* d_x3Dw, int np, const int32_t* obs_offset,
                                          const int32_t* obs_kf, const float* d_obs_xy, const int32_t* d_obs_octave,
                                          const int32_t* d_obs_feature, const orbfe_keypoint* d_kps, int capacity, int nobs, const float* K4,
                                          const float* inv_level_sigma2, int nlevels, float* d_Twm, const float* d_marker_local, int nma,
                                          const int32_t* mobs_offset, const int32_t* mobs_kf, const float* d_mobs_corners, int nmobs,
                                          float marker_info, int use_markers, int iterations, int robust, const uint8_t* d_stop,
                                          int leaf_vertices, orbfe_gba_result* d_res, void* d_scratch, size_t scratch_bytes, void* stream);

/* DIAGNOSTIC / TEST INTERFACE, no stability promise: one linearisation at the given estimates and the first LM trial.  Host pointers;
 * nothing of the problem is written.  *nv = free pose vertices (free keyframes in order, then the markers); b (6 nv, then 3 np), Hpp
 * (nv x 36, the diagonal blocks row-major), Hll (np x 6: the upper triangle xx xy xz yy yz zz), chi2 (the robust chi2, lambda0, 1
 * when every pivot was positive), x (6 nv, then 3 np: the first trial's update), tree (2 + 2 nv + 4 nodes entries, at most
 * 10 (nkf + nma) + 10: nodes, levels; node and place in the elimination order of every free vertex; parent, level, own and boundary
 * vertices of every node).  Arrays sized for nkf + nma vertices. */
int orbfe_gba_inspect(const float* Tcw, const uint8_t* kf_fixed, int nkf, const float* x3Dw, int np, const int32_t* obs_offset,
                      const int32_t* obs_kf, const float* obs_xy, const int32_t* obs_octave, int nobs, const float* K4,
                      const float* inv_level_sigma2, int nlevels, const float* Twm, const float* marker_local, int nma,
                      const int32_t* mobs_offset, const int32_t* mobs_kf, const float* mobs_corners, int nmobs, float marker_info,
                      int use_markers, int robust, int leaf_vertices, int32_t* nv, double* b, double* Hpp, double* Hll, double* chi2, double* x,
                      int32_t* tree, int device);

/* ------------------------------------------------------------ KeyFrameDatabase: candidate queries -- */
/* KeyFrameDatabase::DetectLoopCandidates(pKF, minScore) (src/KeyFrameDatabase.cc:76-197, called by LoopClosing::DetectLoop) and
 * KeyFrameDatabase::DetectRelocalizationCandidates(F) (:199-309, called by Tracking::Relocalization) on flat arrays, with DBoW2's
 * L1 score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).  Every output is the reference's bit for bit: the score is additions,
 * subtractions and fabs in double in ascending word order, everything behind it float comparisons and short float sums.
 *
 * The database is K keyframes in the order they were add()ed ("positions" 0 .. K-1), each with its BowVector (word ids strictly
 * ascending, values) and an `active` flag (0 = erase()d: the keyframe is never met, as a keyframe or as a neighbour; NULL = all
 * active).  neigh[k][0 .. 9] = GetBestCovisibilityKeyFrames(10) of keyframe k as positions, in order; a negative entry is skipped
 * (fewer than ten neighbours, or a neighbour that is not in the database).  The steps, in the reference's order:
 *   1. the sharing list: every active keyframe that holds a word of the query -- in loop mode except the positions of `connected`
 *      (GetConnectedKeyFrames()) -- ordered as the walk over the inverted file meets them: ascending (first common word, position).
 *      common[k] = the number of query words keyframe k holds (mnLoopWords / mnRelocWords) for the keyframes of the list, 0 elsewhere;
 *   2. min_common_words = (int)(max_common_words * 0.8f); a keyframe of the list with common > min_common_words is scored:
 *      si = (float)L1Scoring::score(query, keyframe), and scores[k] = si (mLoopScore / mRelocScore).  No other entry of scores
 *      is written.  Loop mode keeps the scored keyframes with si >= min_score, relocalization mode all of them;
 *   3. for each kept keyframe in list order: accScore = si + the scores of its neighbours that count, in neighbour order, in
 *      float; pBestKF = the keyframe or the neighbour with the strictly greatest score.  A neighbour counts in loop mode when it
 *      is in the sharing list and was scored in this call; in relocalization mode when it is in the sharing list, scored or not:
 *      one that was not scored contributes scores[k] AS THE CALLER PASSED IT (the reference reads the mRelocScore an earlier
 *      query left, or an uninitialised float).  That is why scores is in/out; loop mode never reads what it did not write;
 *   4. best_acc_score = the greatest accScore, starting from min_score (loop) or 0; entries with accScore > 0.75f * best_acc_score
 *      give their pBestKF, first occurrences only: candidates[0 .. n_candidates), in the reference's order.
 * The reference's early returns (no sharing keyframe; nothing kept) give n_candidates = 0 and zero in the fields behind them.
 * scoring is DBoW2's enum (0 = L1_NORM, what ORBvoc.txt declares); anything else is ORBFE_ERR_INVALID. */
#define ORBFE_KFDB_LOOP 0
#define ORBFE_KFDB_RELOC 1
#define ORBFE_KFDB_NEIGHBOURS 10
#define ORBFE_KFDB_MAX_KEYFRAMES 8192  /* K of one call */
#define ORBFE_KFDB_MAX_WORDS 4096      /* words of a query BowVector (the bound of the vocabulary transform) */

typedef struct orbfe_kfdb_result {
    int32_t n_sharing;          /* lKFsSharingWords.size() */
    int32_t max_common_words, min_common_words;
    int32_t n_scored;           /* nscores */
    int32_t n_kept;             /* lScoreAndMatch.size() */
    int32_t n_candidates;       /* size of the returned vector */
    float   best_acc_score, min_score_to_retain; /* 0 when the function returned early */
    int32_t status;             /* ORBFE_OK; the batch call: ORBFE_ERR_INVALID for a query it skipped (see there) */
} orbfe_kfdb_result;

/* One query, host pointers.  Query: q_word / q_value, nbow entries.  Database: CSR, keyframe k owns entries offsets[k] ..
 * offsets[k + 1] of word / value.  connected / nconn and min_score are read in loop mode only.  candidates: K entries of room,
 * n_candidates are written; common (K entries, all written) may be NULL; scores: K entries, see above.
 * ORBFE_ERR_INVALID: NULL pointers, an unknown mode or scoring, words not strictly ascending, offsets that do not start at 0 or
 * decrease, a position outside [0, K) in connected, a neigh entry >= K, a value or min_score that is not finite.
 * ORBFE_ERR_CAPACITY: K > ORBFE_KFDB_MAX_KEYFRAMES or nbow > ORBFE_KFDB_MAX_WORDS.  Nothing is written on an error.  K = 0 is an
 * empty database: the zero record.  The call uploads the whole database: a caller with many queries keeps it on the device and
 * uses the batch call. */
int orbfe_detect_candidates(int mode, int scoring, const uint32_t* q_word, const double* q_value, int nbow, const int32_t* offsets,
                            const uint32_t* word, const double* value, const uint8_t* active, int K, const int32_t* neigh,
                            const int32_t* connected, int nconn, float min_score, float* scores, int32_t* candidates, int32_t* common,
                            orbfe_kfdb_result* res, int device);

/* nq queries against one resident database.  BowVectors in the layout orbfe_vocabulary_transform_batch_device writes: blocks of
 * `capacity` entries of d_bow_word / d_bow_value per frame, d_nbow[f] valid (clamped to the block; capacity <=
 * ORBFE_KFDB_MAX_WORDS).  Keyframe k of the database is frame d_db[k] (NULL: frame k), query q is frame d_query[q] of the same
 * blocks; a negative frame index is an empty BowVector.  d_active[K] may be NULL; d_neigh as above (an entry >= K is skipped like
 * a negative one).  Loop mode: query q's connected positions are d_conn[d_conn_offsets[q] .. d_conn_offsets[q + 1]) and its
 * min_score is d_min_score[q], read ON THE DEVICE (orbfe_bow_min_score_batch_device in front of this call produces it).
 * Relocalization mode reads none of the three (they may be NULL).
 * d_scores[nq][K], in/out: row q is the score state query q sees and updates.  The queries of one call run side by side, each
 * on its own row.  The reference's state is sequential -- a query sees what the queries before it left: a caller who wants
 * exactly that runs ONE query a call, every call on the same row.
 * Outputs: d_candidates[nq][K] (n_candidates entries of row q are written, the rest of the row is left alone), d_common[nq][K]
 * (required: it is the call's scratch too; every entry is written), d_res[nq].  d_scratch: nq x K uint32 of scratch.
 * A query frame that is itself in the database and not in its connected list finds itself, with every word in common: leaving
 * it out (d_active, the connected list, or adding it afterwards as LoopClosing does) is the caller's duty.
 * A query whose connected range decreases or holds a position outside [0, K) is skipped: status ORBFE_ERR_INVALID, every other
 * field 0, its row of d_common zero, nothing else written.  Word order and finite values are the caller's duty here.
 * K <= ORBFE_KFDB_MAX_KEYFRAMES (ORBFE_ERR_CAPACITY above; also for capacity > ORBFE_KFDB_MAX_WORDS and nq > 65535).  Two launches
 * whatever nq is; asynchronous on `stream`, no host synchronisation, no scratch beyond the caller's buffers.
 * Candidate positions become the next step's pair list as they are when d_db is NULL: d_pair2 = the candidates row, d_pair1 =
 * the query frame repeated (orbfe_search_by_bow_batch_device, orbfe_sim3_solve_batch_device).  Those calls index their blocks by
 * d_pair2 unchecked, and the entries of a row behind n_candidates are NOT written here: a caller who launches the next step over a
 * fixed number of rows without reading n_candidates back MUST fill each row of d_candidates with a valid frame index (the query
 * frame, say) before this call; the rows behind n_candidates then pair the query with that frame and are ignored afterwards. */
int orbfe_detect_candidates_batch_device(int mode, int scoring, const uint32_t* d_bow_word, const double* d_bow_value, const int32_t* d_nbow,
                                         int capacity, const int32_t* d_db, const uint8_t* d_active, int K, const int32_t* d_query, int nq,
                                         const int32_t* d_neigh, const int32_t* d_conn_offsets, const int32_t* d_conn,
                                         const float* d_min_score, float* d_scores, int32_t* d_candidates, int32_t* d_common,
                                         uint32_t* d_scratch, orbfe_kfdb_result* d_res, void* stream);

/* DetectLoop's minScore (src/LoopClosing.cc:232-246) for nq queries: d_min_score[q] = the least (float)score(query q, keyframe)
 * over query q's connected positions, starting from 1.0f; arguments as above.  A position outside [0, K) and an inactive keyframe
 * are skipped (SetBadFlag erases a keyframe from the database: the reference's isBad() skip).  Asynchronous on `stream`. */
int orbfe_bow_min_score_batch_device(int scoring, const uint32_t* d_bow_word, const double* d_bow_value, const int32_t* d_nbow, int capacity,
                                     const int32_t* d_db, const uint8_t* d_active, int K, const int32_t* d_query, int nq,
                                     const int32_t* d_conn_offsets, const int32_t* d_conn, float* d_min_score, void* stream);

/* The raw scores: scores[p] = (float)L1Scoring::score(frame pair1[p], frame pair2[p]).  Host call: nframes BowVectors in CSR
 * (ORBFE_ERR_INVALID as in orbfe_detect_candidates, and for a pair outside [0, nframes)).  Device call: the block layout above,
 * without the bound on capacity; frame indices are the caller's duty (a negative one is an empty vector: score -0.0f). */
int orbfe_bow_score(int scoring, const int32_t* offsets, const uint32_t* word, const double* value, int nframes, const int32_t* pair1,
                    const int32_t* pair2, int npairs, float* scores, int device);
int orbfe_bow_score_batch_device(int scoring, const uint32_t* d_bow_word, const double* d_bow_value, const int32_t* d_nbow, int capacity,
                                 const int32_t* d_pair1, const int32_t* d_pair2, int npairs, float* d_scores, void* stream);

/* ------------------------------------------------------------------ Frame glue: undistortion -- */
/* cv::undistortPoints(src, dst, K, distCoeffs, noArray(), K) (OpenCV 3.4: 5 fixed-point iterations in double) on n
 * (x, y) float pairs -- what Frame::UndistortKeyPoints (src/Frame.cc:357-387) and Frame::UndistortArucoCorners
 * (:389-416) run over mvKeys / the 4*NA marker corners.  K4 = {fx, fy, cx, cy}; dist = k1 k2 p1 p2 [k3 [k4 k5 k6
 * [s1 s2 s3 s4]]] (ORB_SLAM2's mDistCoef has 4 or 5).  Always undistorts (the callers' "mDistCoef[0] == 0 -> copy"
 * shortcut is the caller's, see the batch variant).  Host pointers; src may equal dst. */
int orbfe_undistort_points(const float* src, int n, const float* K4, const float* dist, int ndist, float* dst, int device);

/* Frame::UndistortKeyPoints over a batch of extractor outputs on the device: frame f's first min(d_n[f], capacity)
 * records get undistorted (x, y), every other field is kept (Frame.cc:379-386); with ndist == 0 or dist[0] == 0 the
 * records are copied unchanged (:359-363).  d_kps_un may equal d_kps.  A negative count is 0.  With coefficients the records
 * from min(d_n[f], capacity) to `capacity` of d_kps_un are not written; the copy of ndist == 0 / dist[0] == 0 is of whole blocks, so
 * there d_kps_un receives those records of d_kps as well, bit for bit.  Asynchronous on `stream`. */
int orbfe_undistort_keypoints_batch_device(const orbfe_keypoint* d_kps, const int32_t* d_n, int capacity, int nframes,
                                           const float* K4, const float* dist, int ndist, orbfe_keypoint* d_kps_un, void* stream);

/* Frame::ComputeImageBounds (src/Frame.cc:418-451): bounds = {mnMinX, mnMinY, mnMaxX, mnMaxY}, the `bounds` argument
 * of the search entry points above.  {0, 0, cols, rows} when dist[0] == 0. */
int orbfe_compute_image_bounds(int cols, int rows, const float* K4, const float* dist, int ndist, float* bounds, int device);

/* ------------------------------------------------------------------ on-disk keyframe features -- */
/* The feature records of the reference's binary map files (src/Map.cc:297-321 SaveKeyFrame, :478-511 LoadKeyFrame): per
 * feature pt.x pt.y size angle response (f32) octave (i32) | mDescriptors.cols (i32 = 32) | 32 descriptor bytes | map
 * point index (u64, ULONG_MAX = none) = 68 bytes, packed back to back after each keyframe header (id u64, timestamp f64,
 * quaternion 4 x f32, translation 3 x f32, N i32).  class_id is not stored; unpack sets -1 (cv::KeyPoint's default). */
#define ORBFE_KF_FEATURE_BYTES 68
/* n records <-> arrays, host pointers.  mp_index may be NULL (pack: ULONG_MAX everywhere; unpack: not returned).
 * unpack fails with ORBFE_ERR_INVALID when a record's descriptor length is not 32 (LoadKeyFrame would read a
 * different number of bytes there, Map.cc:492-495). */
int orbfe_keyframe_features_pack(const orbfe_keypoint* kps, const uint8_t* desc, const uint64_t* mp_index, int n, uint8_t* out, int device);
int orbfe_keyframe_features_unpack(const uint8_t* in, int n, orbfe_keypoint* kps, uint8_t* desc, uint64_t* mp_index, int device);
/* A whole map file image resident on the device: segment s = the features of one keyframe, starting at byte
 * d_seg_offset[s] of d_file (4-byte aligned, as every offset of the format is) and occupying output indices
 * d_seg_first[s] .. d_seg_first[s + 1].  NULL offsets = one segment at offset 0 of max_records_per_segment records.
 * *d_bad counts records whose descriptor length is not 32 (zero it first). */
int orbfe_keyframe_features_unpack_device(const uint8_t* d_file, const uint64_t* d_seg_offset, const int32_t* d_seg_first, int nsegments,
                                          int max_records_per_segment, orbfe_keypoint* d_kps, uint8_t* d_desc, uint64_t* d_mp_index,
                                          int32_t* d_bad, void* stream);
int orbfe_keyframe_features_pack_device(const orbfe_keypoint* d_kps, const uint8_t* d_desc, const uint64_t* d_mp_index,
                                        const uint64_t* d_seg_offset, const int32_t* d_seg_first, int nsegments,
                                        int max_records_per_segment, uint8_t* d_file, void* stream);

/* ------------------------------------------------------------------ ArUco marker detector -- */

/* MarkerDetector + setDictionary(dict) + setDetectionMode(DM_NORMAL) +
 * setCornerRefinementMethod(CORNER_LINES): the configuration of src/Frame.cc:135-137. NULL on error. */
orbfe_aruco* orbfe_aruco_create(const char* dictionary, int device);
void orbfe_aruco_destroy(orbfe_aruco* h);
int orbfe_aruco_set_dictionary(orbfe_aruco* h, const char* dictionary);
int orbfe_aruco_max_markers(const orbfe_aruco* h);
/* MarkerDetector::Params the shim forwards (markerdetector.h:96-214).
 *   setDictionary(name, error_correction_rate) / MarkerDetector(dict, rate): rate in [0, 1]; > 0 enables the error-correction pass
 *     of DictionaryBased::detect (a code closer than int(tau * rate) bits to a dictionary entry is accepted; default 0 = exact).
 *   setDetectionMode(dm, minMarkerSize) (markerdetector.cpp:374-391): DM_NORMAL (0, Frame.cc:136), DM_FAST (1) and DM_VIDEO_FAST (2).
 *     The fast modes threshold with THRES_AUTO_FIXED: one global threshold, carried from frame to frame (Otsu over the pixels of the
 *     markers just found, markerdetector_impl.cpp:7003-7040) and replaced by 10 + rand() % 230 -- the process's own rand() sequence,
 *     as in the reference -- when a frame yields nothing (:6903-6990); DM_VIDEO_FAST also derives the next frame's minMarkerSize from
 *     the smallest marker of this one (:8790-8880).  Such a handle is frame-sequential: the host-pointer entry points take its frames
 *     one at a time in order, orbfe_aruco_detect_batch_device refuses it.  minMarkerSize in [0, 1] (Params::minSize, a fraction of
 *     the larger image side) > 0 detects on an INTER_NEAREST reduction of the frame and brings the corners back through the /2
 *     pyramid with cv::cornerSubPix (cornerUpsample, :14028-14220); reductions below 64 x 48 pixels are refused.
 *   setCornerRefinementMethod(m): CORNER_SUBPIX (0: cv::cornerSubPix, window 4, 12 iterations, eps 0.005, :8511), CORNER_LINES
 *     (1, default here, Frame.cc:137) and CORNER_NONE (2); anything but CORNER_SUBPIX resets minMarkerSize to 0 (markerdetector.cpp:392-395).
 *   orbfe_aruco_get_state: Params::ThresHold and Params::minSize as the last call left them, the threshold passes of the last call
 *     and the size of the image it worked on (any pointer may be NULL). */
int orbfe_aruco_set_error_correction_rate(orbfe_aruco* h, float rate);
int orbfe_aruco_set_detection_mode(orbfe_aruco* h, int mode, float min_marker_size);
int orbfe_aruco_set_corner_refinement(orbfe_aruco* h, int method);
/* Params::detectEnclosedMarkers (markerdetector.h:126): markers whose corners touch other dark squares (chessboard-like boards).
 * With THRES_AUTO_FIXED the thresholded image is replaced by its inner edge band (erode with a cross, xor); in every mode each
 * rectangle candidate is enlarged by half the threshold window along its diagonals (markerdetector_impl.cpp:2871-2950, :10620-10690). */
int orbfe_aruco_set_enclosed_markers(orbfe_aruco* h, int on);
/* Params::trackingMinDetections (markerdetector.h:187; 0 = off, the default): a marker that was found in that many calls and is
 * missing from this one is looked for among the rectangle candidates the dictionary rejected -- centre inside its last outline,
 * area within 30 %, nearest centre -- and returned with its id and the corner order that continues its previous orientation
 * (markerdetector_impl.cpp:7107-7890).  Host logic over two short lists, as in the reference; the handle becomes frame-sequential.
 * Setting it resets the history.  orbfe_aruco_last_tracked: markers the last call recovered that way. */
int orbfe_aruco_set_tracking(orbfe_aruco* h, int min_detections);
int orbfe_aruco_last_tracked(const orbfe_aruco* h);
int orbfe_aruco_get_state(const orbfe_aruco* h, int32_t* threshold, float* min_size, int32_t* attempts, int32_t* work_rows,
                          int32_t* work_cols);
/* cvtColor(BGR2GRAY) of the CV_8UC3 entry points: 14 fractional bits (OpenCV <= 3.4.1: B 1868, G 9617, R 4899; default) or 15
 * (3.4.2 and later: 3735, 19235, 9798). */
int orbfe_aruco_set_gray_conversion(orbfe_aruco* h, int fractional_bits);
/* aruco::Marker::contourPoints (marker.h:56) of marker `marker` (index into the output of the last detect / batch call) of frame
 * `frame`: the full border the rectangle came from, (x, y) int32 pairs.  *n = its length; min(*n, capacity) points are written.
 * Host pointers; synchronises the device. */
int orbfe_aruco_marker_contour(orbfe_aruco* h, int frame, int marker, int32_t* xy, int capacity, int32_t* n);
/* The same for the first `nmarkers` markers of the frame in ONE round trip: offsets[0 .. nmarkers] are filled in any case (marker i owns
 * points offsets[i] .. offsets[i+1]); the (x, y) pairs are written only when offsets[nmarkers] <= capacity (points), so a caller
 * asks once with capacity 0 for the total or, simply, passes a generous buffer. */
int orbfe_aruco_marker_contours(orbfe_aruco* h, int frame, int nmarkers, int32_t* xy, int capacity, int32_t* offsets);

/* detect(image) -> markers sorted by id, corners refined by contour lines. Host pointers, one CV_8UC1 frame.
 * Frames up to 4095 pixels wide (adaptive-threshold windows up to 31, markerdetector_impl.cpp:3765-3809). */
int orbfe_aruco_detect(orbfe_aruco* h, const uint8_t* img, int rows, int cols, size_t step, orbfe_marker* out,
                       int capacity, int32_t* n_out);
/* detect() on a CV_8UC3 (BGR) frame (markerdetector_impl.cpp:5892: cvtColor(BGR2GRAY) first); `step` in bytes, >= 3 * cols. */
int orbfe_aruco_detect_bgr(orbfe_aruco* h, const uint8_t* bgr, int rows, int cols, size_t step, orbfe_marker* out, int capacity,
                           int32_t* n_out);
int orbfe_aruco_detect_batch(orbfe_aruco* h, const uint8_t* imgs, int nframes, size_t frame_stride, int rows, int cols,
                             size_t step, orbfe_marker* out, int capacity, int32_t* n_out);
/* Flag of orbfe_aruco_batch_status / orbfe_pipeline_status: the frame has more markers than the caller's `capacity` (the pipeline's
 * marker_capacity) records.  Not an internal capacity: no other contour path helps, the batch is repeated with more records. */
#define ORBFE_ARUCO_FLAG_TRUNCATED 128
/* device frames: any base byte, step and frame stride within the bounds given at orbfe_extract_batch_device (LAYOUT OF DEVICE FRAMES).
 * Frame f writes its first min(markers, capacity) records in id order -- a frame with more markers than `capacity` holds a prefix of
 * its id-sorted list, d_n_out[f] = capacity, and is flagged ORBFE_ARUCO_FLAG_TRUNCATED in orbfe_aruco_batch_status; slots past
 * d_n_out[f] are not written.  capacity = orbfe_aruco_max_markers() always suffices. */
int orbfe_aruco_detect_batch_device(orbfe_aruco* h, const uint8_t* d_imgs, int nframes, size_t frame_stride, int rows,
                                    int cols, size_t step, orbfe_marker* d_out, int capacity, int32_t* d_n_out,
                                    void* stream);
/* The batch entry point on device pointers cannot report a frame that exceeded the detector's internal capacities (more
 * than 1024 contours longer than 70 points in a frame that the LDS-resident contour kernels handle; the host-pointer
 * entry points retry such a batch with the big-frame kernel themselves), nor one with more markers than the caller's `capacity`
 * (the host-pointer entry points return ORBFE_ERR_CAPACITY for that).  After the batch: *nflagged = frames of the last
 * batch whose results are incomplete, *flags_or = the union of their capacity flags (synchronises the device).  A frame that was
 * only cut at the caller's capacity carries ORBFE_ARUCO_FLAG_TRUNCATED and nothing else: repeat with capacity up to
 * orbfe_aruco_max_markers(), which always suffices; any other bit is an internal capacity.
 * orbfe_aruco_set_big_frames(h, 1) selects the big-frame contour kernel (bit image in HBM, 4096 kept contours) for all
 * following batches. */
int orbfe_aruco_batch_status(orbfe_aruco* h, int32_t* nflagged, int32_t* flags_or);
int orbfe_aruco_set_big_frames(orbfe_aruco* h, int on);
/* stage read-back for parity tests: 0 = thresholded image (rows x cols bytes, 0/255) of `frame`; 104 = the bit image the contour
 * kernels read from HBM: the thresholded image minus the specks that cannot have a border of more than 70 points where the speck
 * passes ran as a launch (the default in front of the one-workgroup kernels of a full batch), the thresholded image itself otherwise
 * -- also when the passes run INSIDE the relay kernels (ORBFE_ARUCO_SPECKS=2): their cleaned image only ever exists in LDS */
int orbfe_aruco_debug_image(orbfe_aruco* h, int frame, int stage, uint8_t* out);
/* As orbfe_extractor_set_aux_stream, for the detector's forked launches (the /2 pyramid). */
int orbfe_aruco_set_aux_stream(orbfe_aruco* h, void* stream);
int orbfe_aruco_debug_kernel_times(orbfe_aruco* h, float* out_us, int capacity);
/* How many batches of this handle were done again on the next contour path (tiled -> one workgroup -> single walker) because a
 * frame exceeded a capacity of the one they ran on. */
int orbfe_aruco_debug_contour_retries(const orbfe_aruco* h);

/* ------------------------------------------------------------------ marker pose (IPPE) -- */
/* Marker pose: what MarkerDetector::detect adds to every marker when it is given camera parameters and a marker size
 * (markerdetector_impl.cpp:8720-8780 -> Marker::calculateExtrinsics, marker.cpp:322-344 -> aruco::solvePnP, ippe.cpp:91-100)
 * and what Frame.cc:170-174 asks for again to judge the ambiguity (aruco::solvePnP returning both IPPE solutions,
 * ippe.cpp:72-89): rvec/tvec = the solution with the lower reprojection error (Marker::Rvec / Tvec as CV_32F), rvec2/tvec2
 * the other one, err = their reprojection errors in pixels (Frame.cc:172: mvbArucoGood = err[0] / err[1] < 0.7).
 * Object frame: marker centre, corners (-s/2, s/2, 0) (s/2, s/2, 0) (s/2, -s/2, 0) (-s/2, -s/2, 0) (marker.cpp:358-369).
 * For a marker within about 1e-3 rad of fronto-parallel, rvec and err carry the error of the reference's rot2vec (eps / (pi - angle)^2), and the
 * rvec and err of a solution, or the whole record, can be NaN; tvec and tvec2 are unaffected. */
typedef struct orbfe_marker_pose {
    float rvec[3], tvec[3];
    float rvec2[3], tvec2[3];
    float err[2];
} orbfe_marker_pose;

/* CameraParameters::resize (cameraparameters.cpp:158-173): detect() rescales the camera matrix when the image size is not
 * CamSize (markerdetector_impl.cpp:1110-1172; Frame.cc:132 fixes CamSize = 1280x720).  K4 = {fx, fy, cx, cy}. Host only. */
int orbfe_camera_resize(const float* K4, int cam_width, int cam_height, int img_width, int img_height, float* K4_out);

/* Poses of n markers (host pointers).  marker_size in metres (Frame.cc:131: 0.187); marker_size <= 0 or an empty camera
 * matrix is ORBFE_ERR_INVALID (the reference throws cv::Exception 9004, marker.cpp:325-331).  dist as orbfe_undistort_points. */
int orbfe_marker_poses(const orbfe_marker* markers, int n, float marker_size, const float* K4, const float* dist, int ndist,
                       orbfe_marker_pose* poses, int device);

/* The same over the detector's batch output on the device: frame f's first min(d_n[f], capacity) records of d_markers get
 * a pose in the same slot of d_poses.  d_n == NULL: all `capacity` records of every frame. */
int orbfe_marker_poses_batch_device(const orbfe_marker* d_markers, const int32_t* d_n, int capacity, int nframes,
                                    float marker_size, const float* K4, const float* dist, int ndist,
                                    orbfe_marker_pose* d_poses, void* stream);
/* detect(image, CameraParameters, markerSize) in ONE call (markerdetector.h:276-283: what Frame.cc:142 calls): the markers of
 * orbfe_aruco_detect plus poses[i] of markers[i] as orbfe_marker_poses would give them, with one upload, one wait and one set of
 * result copies instead of two of each.  K4 = {fx, fy, cx, cy} for THIS image size (orbfe_camera_resize when CamSize differs). */
int orbfe_aruco_detect_poses(orbfe_aruco* h, const uint8_t* img, int rows, int cols, size_t step, orbfe_marker* out,
                             orbfe_marker_pose* poses, int capacity, int32_t* n_out, float marker_size, const float* K4,
                             const float* dist, int ndist);
/* The same on a CV_8UC3 (BGR) frame. */
int orbfe_aruco_detect_poses_bgr(orbfe_aruco* h, const uint8_t* bgr, int rows, int cols, size_t step, orbfe_marker* out,
                                 orbfe_marker_pose* poses, int capacity, int32_t* n_out, float marker_size, const float* K4,
                                 const float* dist, int ndist);
/* cv::cornerSubPix(image, corners, Size(win, win), Size(-1, -1), TermCriteria(MAX_ITER | EPS, max_iters, eps)) on a CV_8UC1 image
 * (what the detector's CORNER_SUBPIX mode and its cornerUpsample run, markerdetector_impl.cpp:8511, :14182): pts = n (x, y) pairs,
 * refined in place; window half size 1 .. 8.  Host pointers. */
int orbfe_corner_subpix(const uint8_t* img, int rows, int cols, size_t step, float* pts, int n, int win, int max_iters, double eps,
                        int device);

/* ------------------------------------------------------------------ the batched-video mode -- */
/* What the reference's Tracking thread does per frame -- ORBextractor::operator() (Frame.cc:200-206), MarkerDetector::detect(image,
 * camera, 0.187) (Frame.cc:142), frame t matched against t-1 (Tracking.cc:531-532: all-pairs knn2 + SearchForInitialization) -- for
 * a STREAM of same-sized frames handed over in batches resident on the device (BASELINE north_star).  The pipeline
 * owns the engines (two extractor sets that alternate batches, phase-locked; one detector), its HIP streams and events, `record_sets`
 * result sets in rotation, and -- on N > 1 ranks -- the batch's one collective: the gather of the record set to rank `dst` by RCCL
 * send / recv on the pipeline's matching stream.  orbfe_pipeline_step only ENQUEUES (a few hundred microseconds of host time per
 * 300-frame batch) and returns the record set the batch is written to; a batch's matching (and gather) is enqueued one step late
 * where that shortens the step (frames up to 640 x 480), so call orbfe_pipeline_flush before waiting for the newest batch.
 *
 * A record set is ONE contiguous device buffer (orbfe_record_layout), array by array over the frames; the keypoint arrays carry one
 * slot in front of the batch (`halo` = 1): the last frame of the previous batch, so that the first frame of a batch is matched
 * against its predecessor in the stream too.  Frame f of the batch is slot f + halo.  Matching outputs of the newest batch: pair p
 * = slot p (queries, F1) against slot p + 1 (train, F2), p = 0 .. frames - 1; pair 0 is the pair across the batch boundary (no
 * keypoints on the F1 side for the first batch of a stream). */
typedef struct orbfe_pipeline_config {
    int32_t frames, rows, cols;        /* frames per batch; frame size */
    int32_t nfeatures, nlevels;        /* ORBextractor(nfeatures, scale_factor, nlevels, ini_th_fast, min_th_fast) */
    float scale_factor;
    int32_t ini_th_fast, min_th_fast;
    char dictionary[32];               /* MarkerDetector::setDictionary */
    int32_t device;
    int32_t marker_capacity;           /* marker (+ pose) records per frame in a record set (<= orbfe_aruco_max_markers; a frame with more: orbfe_pipeline_status) */
    int32_t use_orb, use_aruco;        /* 0 leaves an engine out (diagnostics) */
    float marker_size;                 /* metres (Frame.cc:131: 0.187) */
    float K[4], dist[12];              /* camera of the marker poses FOR THIS FRAME SIZE (orbfe_camera_resize), ndist coefficients */
    int32_t ndist;
    int32_t window_size;               /* SearchForInitialization: 100 */
    float nnratio;                     /* 0.9 */
    int32_t check_orientation;         /* 1 */
    /* scheduling; -1 = the measured default for the frame size: extractor engine sets, result sets in rotation,
     * phase lock of the engine sets (orbfe_extractor_follow stage), stage of the extractor's previous batch the detector's batch starts
     * behind, matching enqueued one step late, the detector's /2 pyramid in line on its stream.  They change the order of work, never
     * the results.  With two or more engine sets a batch's descriptor kernel is enqueued one step late (ORBFE_DESCRIBE_LATE, on by
     * default), and that forces defer_post on whatever was asked for -- an explicit defer_post = 0 here or ORBFE_DEFER_POST=0 included;
     * only turning the late describe off (ORBFE_DESCRIBE_LATE=0, one engine set, a stage-3 lock) gives it back.  A lock on stage 3, the descriptors (phase_pin % 10 == 3,
     * phase_pin / 10 == 3 or det_pin % 10 == 3), turns the late describe off.  (The whole rule: plan_schedule, csrc/pipeline_plan.hpp.)  orbfe_pipeline_engine_sets reads back the six fields in
     * effect; whether the late describe is on is not reported (above 640 x 480, where defer_post defaults to 0, it shows there). */
    int32_t engine_sets, record_sets, phase_pin, det_pin, defer_post, det_nofork;
} orbfe_pipeline_config;
typedef struct orbfe_record_layout {
    int32_t frames, capacity, marker_capacity, halo;
    uint64_t off_kps, off_desc, off_n;                 /* (frames + halo) x capacity x 28 B | x 32 B | (frames + halo) x int32 */
    uint64_t off_markers, off_nmarkers, off_poses;     /* frames x marker_capacity x 36 B | frames x int32 | frames x marker_capacity x 56 B */
    uint64_t nbytes;
} orbfe_record_layout;

/* the defaults of BASELINE configs[1]: nfeatures 1000, 8 levels, 1.2, FAST 20 / 7, "ARUCO", 64 marker records, both engines, marker
 * size 0.187, TUM1 camera (Examples/Monocular/TUM1.yaml) rescaled from 1280 x 720 (Frame.cc:132), window 100, ratio 0.9; scheduling -1 */
int orbfe_pipeline_config_default(orbfe_pipeline_config* cfg, int frames, int rows, int cols);
orbfe_pipeline* orbfe_pipeline_create(const orbfe_pipeline_config* cfg);
void orbfe_pipeline_destroy(orbfe_pipeline* p);
int orbfe_pipeline_layout(const orbfe_pipeline* p, orbfe_record_layout* out);
/* One batch: d_imgs = frames x rows x pitch bytes on the pipeline's device (any base byte, any pitch >= cols within the bounds of LAYOUT
 * OF DEVICE FRAMES at orbfe_extract_batch_device, frames rows * pitch apart; the frames have to stay valid and unchanged
 * until orbfe_pipeline_input_done for the batch, or orbfe_pipeline_synchronize, has returned: a kernel of the batch may be enqueued
 * after this call).  *record_set = index of the set the batch is written to. */
int orbfe_pipeline_step(orbfe_pipeline* p, const uint8_t* d_imgs, size_t pitch, int32_t* record_set);
/* The same with the frames in HOST memory (rows of `step` bytes, frames contiguous; page-locked -- orbfe_host_alloc -- for the copy to
 * overlap): the pipeline uploads the batch into a ring of three device buffers on a copy stream of its own, ahead of the engines,
 * and copies every batch's record set back to page-locked host memory on a second copy stream behind the batch's post-work; both
 * overlap with the engines of the neighbouring batches.  h_imgs must stay valid and unchanged until orbfe_pipeline_input_done for
 * the batch, or orbfe_pipeline_synchronize, has returned.
 * orbfe_pipeline_host_records: the host copy of record set `set` (waits for its copy; valid until the set is written again, R steps on). */
int orbfe_pipeline_step_host(orbfe_pipeline* p, const uint8_t* h_imgs, size_t step, int32_t* record_set);
int orbfe_pipeline_host_records(orbfe_pipeline* p, int set, const uint8_t** h_records);
/* after steps from host memory: out[0] = microseconds the newest uploads took on the copy stream (mean over the input ring), out[1] =
 * the newest read-back of a record set.  Synchronises. */
int orbfe_pipeline_host_copy_us(orbfe_pipeline* p, float out[2]);
/* The HIP stream priority of the upload / read-back streams of orbfe_pipeline_step_host and the range the device offers (numerically
 * larger = lower).  They are created with the LOWEST one so that they come out of another pool of hardware queues than the engines'
 * streams; lowest == highest means the device has no second pool and uploads queue behind the engines (a warning is printed once). */
int orbfe_pipeline_copy_stream_priority(orbfe_pipeline* p, int* priority, int* lowest, int* highest);
void* orbfe_host_alloc(size_t bytes);                        /* page-locked host memory (hipHostMalloc) / NULL */
void orbfe_host_free(void* p);
/* Device memory for a caller without a HIP toolchain of its own (the Python wrapper, a host language over FFI): zeroed memory on
 * `device` / NULL, a blocking upload of `nrows` rows of `width` bytes (source rows `spitch` apart, destination rows `dpitch`), a
 * blocking download of `bytes`.  The pointers are ordinary HIP device pointers of the library's runtime. */
void* orbfe_device_alloc(int device, size_t bytes);
void orbfe_device_free(void* d);
int orbfe_device_upload_rows(void* d_dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t nrows);
int orbfe_device_download(void* dst, const void* d_src, size_t bytes);
int orbfe_pipeline_flush(orbfe_pipeline* p);                 /* enqueue the held-back post-work (matching, gather) of the newest batch */
int orbfe_pipeline_synchronize(orbfe_pipeline* p);           /* flush + wait for everything enqueued */
/* wait until the engines of the batch written to `record_set` have read their frames: the call that releases the caller's input buffer,
 * device frames and host frames alike.  The batch's descriptor kernel may still be held back (the late describe of the next step): for
 * the newest batch this call enqueues it first, so nothing has to be flushed before. */
int orbfe_pipeline_input_done(orbfe_pipeline* p, int record_set);
/* capacity flags since the last call (synchronises): out[0] extractor overflow, [1] SearchForInitialization pool overflow (the pool
 * has been grown: repeat), [2] frames the detector flagged, [3] the union of their flags.  All zero = results complete.
 * All four cover EVERY step since the last call (reading clears them), the detector's as well: [2] counts the flagged frames of all
 * those steps.  ORBFE_ARUCO_FLAG_TRUNCATED in [3]: a frame had more markers than marker_capacity and its record holds the first
 * marker_capacity of them in id order (with their poses) -- create the pipeline with a larger marker_capacity, up to
 * orbfe_aruco_max_markers(), which always suffices; the other bits are as in orbfe_aruco_batch_status. */
int orbfe_pipeline_status(orbfe_pipeline* p, int32_t out[4]);
int orbfe_pipeline_set_big_frames(orbfe_pipeline* p, int on); /* orbfe_aruco_set_big_frames on the pipeline's detector */
/* device pointers: record set `set`; the matching outputs of the newest batch ([frames][capacity] each, nmatches [frames]) */
int orbfe_pipeline_records(orbfe_pipeline* p, int set, uint8_t** d_records);
int orbfe_pipeline_matches(orbfe_pipeline* p, int32_t** d_best_idx, int32_t** d_best_dist, int32_t** d_second_dist, int32_t** d_matches12,
                           int32_t** d_nmatches);
/* a new stream: the next batch has no predecessor (the halo slots are emptied) */
int orbfe_pipeline_reset_stream(orbfe_pipeline* p);
/* the engines (for their debug entry points / kernel timers): extractor of engine set `set` (NULL past the last), the detector */
orbfe_extractor* orbfe_pipeline_extractor(orbfe_pipeline* p, int set);
orbfe_aruco* orbfe_pipeline_detector(orbfe_pipeline* p);
int orbfe_pipeline_engine_sets(const orbfe_pipeline* p, int32_t* engine_sets, int32_t* record_sets, int32_t* phase_pin, int32_t* det_pin,
                               int32_t* defer_post, int32_t* det_nofork);
/* launch timing of the matching / gather (HIP events on the matching stream; off by default).  timing_us: medians over the steps
 * since timing was switched on (the newest 64): out[0] knn2, [1] SearchForInitialization, [2] gather (0 without one); last != 0: the
 * newest step's instead.  Synchronises. */
int orbfe_pipeline_enable_timing(orbfe_pipeline* p, int on);
int orbfe_pipeline_timing_us(orbfe_pipeline* p, int last, float out[3]);
/* The ORBFE_* environment variables the pipeline and the engines read, with their defaults, as "NAME=default;NAME=default;..."
 * ("size" = decided by the frame size): what bench.py checks the environment against. */
const char* orbfe_pipeline_env_defaults(void);

/* Multi-GPU (one process per GPU): the batch's gather over RCCL (librccl is opened at run time; ORBFE_ERR_HIP when it is missing).
 * Either hand over a communicator the application owns (set_comm; ncclComm_t as void*), or let the pipeline create one:
 * comm_unique_id on one rank (ncclGetUniqueId, 128 bytes), the bytes sent to all ranks by the application's own means, then
 * comm_init on every rank (ncclCommInitRank).  From then on every batch's record set is gathered to rank `dst` behind the batch's
 * matching.  `dst` receives block r of rank r (its own too) in buffers allocated once: ONE SET OF BLOCKS PER RECORD SET -- the batch
 * written to record set s (orbfe_pipeline_step's *record_set) lands in block set s, which is written again record_sets batches later --
 * so a consumer on `dst` (one Tracking thread per stream, src/Tracking.cc:163-190) reads batch i while the following batches arrive:
 *     orbfe_pipeline_gathered_wait(p, s)          block until the gather of the batch last written to set s is complete (its deferred
 *                                                 post-work is flushed first if it was still held back); ORBFE_ERR_INVALID while no batch has
 *                                                 been gathered into s yet
 *     orbfe_pipeline_gathered_batch(p, s, &b)     which batch (step number of this pipeline, from 0) the newest gather into set s carries:
 *                                                 a consumer that expects batch i and reads b = i + record_sets has been overtaken
 *     orbfe_pipeline_gathered_set(p, s, r, &ptr)  rank r's block of set s (device pointer, layout = orbfe_pipeline_layout)
 *     orbfe_pipeline_gathered_release(p, s, st)   optional: the reads of set s enqueued on the consumer's HIP stream `st` so far (NULL: the
 *                                                 null stream) must finish before the set is received into again; without it the set is
 *                                                 simply overwritten record_sets batches later.  Call it BEFORE the step that writes set s
 *                                                 again is enqueued: a release that comes later delays the gather after that one instead
 * orbfe_pipeline_gathered(p, r, &ptr) = block r of the newest gather that was enqueued.  world == 1 runs the same branch with a send /
 * recv to itself.  ORBFE_RCCL_LIB names a library to bind in place of librccl (tests/fake_rccl.cpp). */
int orbfe_pipeline_comm_unique_id(uint8_t id[128]);
int orbfe_pipeline_comm_init(orbfe_pipeline* p, const uint8_t id[128], int rank, int world, int dst);
int orbfe_pipeline_set_comm(orbfe_pipeline* p, void* nccl_comm, int rank, int world, int dst);
int orbfe_pipeline_gathered(orbfe_pipeline* p, int rank, uint8_t** d_block);
int orbfe_pipeline_gathered_set(orbfe_pipeline* p, int record_set, int rank, uint8_t** d_block);
int orbfe_pipeline_gathered_wait(orbfe_pipeline* p, int record_set);
int orbfe_pipeline_gathered_release(orbfe_pipeline* p, int record_set, void* stream);
int orbfe_pipeline_gathered_batch(orbfe_pipeline* p, int record_set, long long* batch);
/* The transport operations one batch's gather consists of on rank `rank`, in issue order (csrc/gather_plan.hpp: the function the
 * pipeline itself executes with ncclRecv / ncclSend / a device copy).  Host logic only -- no device is touched -- so the N-rank control
 * flow (who receives what into which of the rotating blocks) can be driven over any transport: tests/test_multigpu_cpu.py runs it
 * between two gloo ranks on the CPU.  Returns the number of operations written to ops[0 .. capacity), or ORBFE_ERR_INVALID. */
#define ORBFE_GATHER_RECV 0      /* receive rank `peer`'s record set into the block buffer at byte `offset` */
#define ORBFE_GATHER_SEND 1      /* send this rank's record set to rank `peer` */
#define ORBFE_GATHER_COPY_OWN 2  /* this rank's own record set into the block buffer at byte `offset` */
typedef struct orbfe_gather_op { int32_t kind, peer; unsigned long long offset; } orbfe_gather_op;
int orbfe_pipeline_gather_plan(int rank, int world, int dst, int record_set, int record_sets, size_t nbytes, orbfe_gather_op* ops, int capacity);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* ORBFE_H */
