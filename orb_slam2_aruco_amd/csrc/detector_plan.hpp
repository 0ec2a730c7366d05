// detector_plan.hpp -- what the ArUco detector's kernels are told about an input size: the adaptive-threshold window, the bit image,
// the /2 pyramid, the per-frame block sizes, which contour kernels fit LDS, the matrix-core threshold tables.  Pure host arithmetic,
// no HIP: csrc/aruco_detector.hip computes a geometry per input size and swaps it into the handle once its tables are on the device,
// tests/test_detector_plan_cpu.py compiles this header with g++ and checks it against the oracle.  A geometry is a value:
// plan_detector() returns either a complete one or an error (err, msg).
// Below it: the detector's switches (DetectorSwitches, read from the environment once per handle by read_detector_env) and what a
// batch launches on a geometry (plan_batch, escalate): pure functions of plain inputs, pinned by the same CPU tests.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/orbfe.h"
#include "aruco_trace.hpp"
#include "input_layout.hpp"   // plan_input_layout: the layouts of a caller's device frames the kernels can address

namespace orbfe {

#define AR_MAX_KEPT 1024
#define AR_MAX_KEPT_BIG 4096 // the single-walker kernel with the bit image in HBM: LDS has room for this many kept borders
#define RL_KCAP AR_MAX_KEPT  // kept borders per frame (k_contours_relay + k_contours_tail)
#define CTW_MAX_CW 480           // tile width limit: the marker pixels of all relay columns of a tile (31 x (cw / 32 + 1)) fit the queue
// a frame's flag word (counts[f * 4 + 2]; ORBFE_ARUCO_FLAG_TRUNCATED, include/orbfe.h, is its bit 128): the two capacity bits every
// contour kernel sets (as the literals 2 and 4), and the relay formulation's own
#define AR_FLAG_KEPT 2          // more kept borders than the path's list holds
#define AR_FLAG_POOL 4          // the frame's point pool (or a kernel's staging arena in it) is full
#define AR_CAPACITY_FLAGS (AR_FLAG_KEPT | AR_FLAG_POOL)
#define RL_FLAG_TABLE 32        // (kernel-internal) markers did not fit: coarsen the grid
#define RL_FLAG_BUG 64          // an invariant of the relay formulation failed: redone by k_contours_t as well
#define RL_FALLBACK_FLAGS (RL_FLAG_TABLE | RL_FLAG_BUG)

// one level of the detector's /2 pyramid
struct ArLevel {
    int w, h, pitch;
    long long off; // byte offset inside a frame's pyramid block (level 0 is the input image)
};

// the speck passes ("FEWER WALKS" (2)): bit image -> the bit image the contour kernels are handed
#define SPK_THREADS 256
#define SPK_ROWS 48   // output rows per workgroup (+ ORBFE_SPECK_REACH above and below)
inline size_t speck_lds_bytes(int cols) { return (size_t)4 * (SPK_ROWS + 2 * ORBFE_SPECK_REACH) * (((cols + 2 + 31) >> 5) + 1) * 4; }
// Per-frame scratch of the relay kernels behind the long-walk queue words of d_candq: [start-candidate queue | rim masks and anchors
// of the two speck passes when they run inside the kernel (speck_pass_frame): 3 arrays a pass, each (padded rows + 2 * (H + 1)) rows]
ORBFE_HD int relay_queue_words(int W, int H) { return (W * H) / 16 + 64; }
ORBFE_HD int speck_frame_rows(int H, int HH) { return H + 2 + 2 * (HH + 1); }
ORBFE_HD size_t speck_frame_scratch_words(int W, int H)
{
    const size_t pw = (size_t)((W + 2 + 31) >> 5);
    return 3 * pw * (size_t)speck_frame_rows(H, ORBFE_SPECK_H1) + 3 * pw * (size_t)speck_frame_rows(H, ORBFE_SPECK_H2);
}

#define CT_THREADS 256          // threads that run the whole kernel
#define CT_WAVES (CT_THREADS / 64)
#define AP_STACK 64
#define AP_OUT 64

// LDS of k_contours_relay: region R (bit image | list arrays) followed by the marker keys
ORBFE_HD size_t relay_region_bytes(int lds_bits_words, int kcap, int tbits)
{
    const size_t bits = ((size_t)lds_bits_words * 4 + 15) & ~(size_t)15;
    const size_t lists = (size_t)kcap * 12 + ((size_t)8 << tbits);
    size_t r = bits > lists ? bits : lists;
    return (r + 15) & ~(size_t)15;
}
inline size_t relay_lds_bytes(int lds_bits_words, int kcap, int tbits)
{
    return relay_region_bytes(lds_bits_words, kcap, tbits) + ((size_t)4 << tbits);
}

inline size_t contours_lds_bytes(int lds_bits_words, int kept_cap)
{
    size_t b = ((size_t)lds_bits_words * 4 + 15) & ~(size_t)15;
    b += (size_t)kept_cap * 8;      // keys
    b += (size_t)kept_cap * 4 * 4;  // arena offsets, len, off, rect flag (the last three double as the long-walk queue)
    b += (size_t)CT_WAVES * AP_OUT * 8;
    b += (size_t)CT_WAVES * AP_STACK * 8;
    b += (size_t)kept_cap * 2; // length ranking
    return b + 16;
}

#define AR_MAX_WIN 31   // windows up to 31 (k_adaptive_threshold<15>): frames up to 4095 pixels wide

struct DetectorGeometry {
    int err = ORBFE_OK;               // ORBFE_OK, or why this input is refused (then nothing else below is meaningful)
    char msg[256] = "";
    // what it was planned for: the image that is thresholded and traced, the frame the /2 pyramid starts from (the working image is
    // smaller when minSize > 0).  rows == 0: no geometry.
    int rows = 0, cols = 0, pyr_rows = 0, pyr_cols = 0;
    // Adaptive-threshold window.  The threshold kernels compare box sums as integers, mean = (s + n / 2) / n with n = win^2: n is odd,
    // so the rounding has no ties and equals the reference's rint(s * (1.0 / n)) for every box sum of every window admitted here
    // (tests/test_detector_plan_cpu.py runs through them all).
    int win = 0;
    int wpr = 0;                      // words per row of the bit image
    size_t bits_fu32 = 0;
    int npyr = 0;
    std::vector<ArLevel> levels;
    std::vector<int> lvl_exact;       // 1 if level p is an exact 2x reduction of level p-1
    size_t pyr_fbytes = 0, candq_fu32 = 0, pool_fu32 = 0, gpad_fu32 = 0;
    int lds_bits_words = 0;           // the padded bit image where it fits LDS next to k_contours_t's arrays (0: it does not)
    int relay_tbits = 0;              // hash-table size of the relay kernels (0: they cannot run at this image size)
    int relay_kshift = 5;             // their initial grid spacing (log2)
    bool relay_global = false;        // k_contours_relay8g: the bit image stays in HBM (it does not fit LDS)
    int relay_kcap = RL_KCAP;         // kept borders per frame the relay kernels and their tail hold
    int ct_segcap = 0, ct_hbits = 0, ct_lcap = 0, ct_items_per_frame = 0;   // tiled path
    bool matches(int rows_, int cols_, int prows, int pcols) const { return rows && rows_ == rows && cols_ == cols && prows == pyr_rows && pcols == pyr_cols; }
};

inline int plan_fail(DetectorGeometry& g, int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g.msg, sizeof(g.msg), fmt, ap);
    va_end(ap);
    return g.err = code;
}

// rows x cols: the image that is thresholded and traced; prows x pcols: the frame the /2 pyramid is built from; S: the dictionary's
// warp size; lcap_override > 0: list elements k_ct_lists keeps in LDS (a measurement switch); rl_static: static LDS of the relay
// kernels (step table, counters) as the runtime reports it -- a constant here once fell behind the kernels and frames whose tables
// only just fitted (1582 x 619: 156,976 B dynamic) failed at launch
inline DetectorGeometry plan_detector(int rows, int cols, int prows, int pcols, int S, bool specks_inkernel, int lcap_override, size_t rl_static)
{
    DetectorGeometry g;
    if (cols > 8000 || rows > 8000) { plan_fail(g, ORBFE_ERR_INVALID, "image larger than 8000 px"); return g; }
    int w = std::max(3, int(15 * float(cols) / 1920.)); // :3765-3809
    if (w % 2 == 0) w++;
    if (w > AR_MAX_WIN) { plan_fail(g, ORBFE_ERR_INVALID, "threshold window %d too large", w); return g; }
    g.rows = rows; g.cols = cols; g.pyr_rows = prows; g.pyr_cols = pcols;
    g.win = w;
    g.wpr = (cols + 31) / 32;
    g.bits_fu32 = (size_t)g.wpr * rows;
    // buildPyramid (:1299-1488): halve while width > 2 * S; inexact levels go through k_resize_level
    int lw = pcols, lh = prows;
    size_t off = 0;
    g.levels.push_back(ArLevel{lw, lh, 0, 0});
    g.lvl_exact.push_back(1);
    int n = 1, tw = pcols;
    while (tw > 2 * S) { tw /= 2; n++; }
    for (int p = 1; p < n; p++) {
        const int sw = lw, sh = lh;
        lw /= 2; lh /= 2;
        if (lw < 1 || lh < 1) break;
        const ArLevel L{lw, lh, (lw + 63) / 64 * 64, (long long)off};
        off += (size_t)L.pitch * lh;
        g.levels.push_back(L);
        g.lvl_exact.push_back(sw == 2 * lw && sh == 2 * lh);
    }
    g.npyr = (int)g.levels.size();
    g.pyr_fbytes = off + 64;
    // HBM overflow of the single-walker kernel's long-walk queue / the relay kernels' start-candidate queue, + their speck scratch
    // (the speck scratch -- four times the queue at 640 x 480 -- only where the in-kernel passes are switched on)
    g.candq_fu32 = ((size_t)relay_queue_words(cols, rows) + (specks_inkernel ? speck_frame_scratch_words(cols, rows) : 0) + 63) / 64 * 64;
    g.pool_fu32 = (size_t)CT_THREADS * std::max(4096, rows * cols / 48); // one private arena per lane of k_contours
    const int pw = (cols + 2 + 31) / 32;
    const size_t padded_words = (size_t)pw * (rows + 2) + 2; // + spare words for ring8()
    // the padded bit image goes to LDS when it fits next to the other arrays (160 KiB per workgroup)
    g.lds_bits_words = (contours_lds_bytes((int)padded_words, AR_MAX_KEPT) + 256 <= 160 * 1024) ? (int)padded_words : 0;
    g.gpad_fu32 = padded_words; // always there: big_mode uses the HBM variant at any size
    // k_contours_relay needs the bit image AND its marker table in LDS; otherwise k_contours_t does all frames.
    // 4096 marker slots on a 32-pixel grid for ordinary frames (a 2048-slot table on a 64-pixel grid would let two workgroups
    // share a CU, but its longer segments cost more than the sharing wins: 857 vs 726 us).  Large frames have more grid
    // crossings than 4096 slots hold and would be coarsened to a 128-pixel grid, which doubles the kernel's time (640 x 480:
    // 463 / 592 / 949 us at 32 / 64 / 128 pixels): they get 8192 slots (k_contours_relay8) when the LDS allows.
    const bool large = (size_t)rows * cols > (size_t)640 * 480 * 3 / 2;
    if (g.lds_bits_words && large && relay_lds_bytes(g.lds_bits_words, RL_KCAP, 13) + rl_static <= 160 * 1024) g.relay_tbits = 13;
    else if (g.lds_bits_words && relay_lds_bytes(g.lds_bits_words, RL_KCAP, 12) + rl_static <= 160 * 1024) g.relay_tbits = 12;
    // frames whose bit image does not fit LDS: the relay formulation with the bit image in HBM (k_contours_relay8g)
    // (and room for as many kept borders as the single-walker kernel's big-frame mode: busy 1920 x 1080 frames have > 1024)
    // (also frames whose bit image fits LDS for the single-walker kernel but not next to a marker table)
    // (round 2: the HBM-image formulation also for frames that fit LDS -- 45 KB workgroups instead of 151 KB -- was slower, 5.50 against 4.62 ms at C3)
    g.relay_global = !g.relay_tbits && relay_lds_bytes(0, AR_MAX_KEPT_BIG, 13) + rl_static <= 160 * 1024;
    if (g.relay_global) { g.relay_tbits = 13; g.relay_kcap = AR_MAX_KEPT_BIG; }
    // tiled path: segments per frame the lists hold (a 640 x 480 frame of the synthetic streams has ~2000, salt noise ~15 k; ids
    // are 16 bits), hash slots (twice that), segments whose list arrays k_ct_lists keeps in LDS (more: the same arrays in HBM)
    int sc = 4096;
    while (sc < rows * cols / 32 && sc < 65536) sc <<= 1;
    g.ct_segcap = std::min(sc, 65535);
    g.ct_hbits = 1;
    while ((1 << g.ct_hbits) < 2 * sc) g.ct_hbits++;
    g.ct_lcap = std::min(g.ct_segcap, lcap_override > 0 ? lcap_override : large ? 16384 : 4096);   // list elements k_ct_lists keeps in LDS (8 B each)
    g.ct_items_per_frame = std::max(4096, g.ct_segcap / 4);
    return g;
}

// Which kernel writes a level of the /2 pyramid.  Level 1 is read from the caller's frames, whose alignment decides: k_half_pyr and
// k_half_area4 cast the source rows to uint4 / uint2, k_half_area reads bytes, k_resize_level makes the inexact levels.
enum class PyrKernel : int { none = 0, half_pyr4, half_pyr3, half_area4, half_area, resize_level };

// The kernels of levels first .. npyr - 1 (entries below `first`: none).  src_align = the low four bits of the address of level 0's
// first byte, src_pitch / src_fstride = its row and frame strides (the caller's); levels >= 2 are read from the detector's own
// pyramid block, whose allocation is aligned and whose frames are pyr_fbytes apart.  half_pyr: the switch of the same name.
//   k_half_pyr<4> / <3> (only from level 1: levels 1 .. 4 / 1 .. 3 in one launch, from 16 x 16 / 8 x 8 source blocks): those levels
//     exact halvings of a level 0 that divides into the blocks; base, pitch and frame stride multiples of 16 / 8;
//   k_half_area4: an exact level whose source base, pitch and frame stride are multiples of 8 (it reads 8 * ceil(w / 4) bytes of a row:
//     up to 6 past the source's pixels, inside a pitch that is a multiple of 8);
//   k_half_area: any other exact level;  k_resize_level: an inexact one.
inline std::vector<PyrKernel> plan_pyramid_kernels(const DetectorGeometry& geo, int first, unsigned src_align, int src_pitch, size_t src_fstride, bool half_pyr)
{
    std::vector<PyrKernel> k((size_t)std::max(geo.npyr, 0), PyrKernel::none);
    if (first == 1 && half_pyr)
        for (int nf = 4; nf >= 3 && first == 1; nf--) {
            const int bs = 1 << nf, al0 = bs == 16 ? 16 : 8;
            bool ok = geo.npyr > nf && geo.levels[0].w % bs == 0 && geo.levels[0].h % bs == 0 && src_pitch % al0 == 0 && src_fstride % al0 == 0 &&
                      (src_align & (unsigned)(al0 - 1)) == 0 && geo.pyr_fbytes % 8 == 0;
            for (int p = 1; ok && p <= nf; p++) {
                const int al = bs >> p;   // bytes a thread stores per row of level p
                ok = geo.lvl_exact[p] && geo.levels[p].w == geo.levels[0].w >> p && geo.levels[p].h == geo.levels[0].h >> p && geo.levels[p].pitch % al == 0 &&
                     geo.levels[p].off % al == 0 && geo.levels[p].pitch >= geo.levels[p].w;
            }
            if (!ok) continue;
            for (int p = 1; p <= nf; p++) k[(size_t)p] = nf == 4 ? PyrKernel::half_pyr4 : PyrKernel::half_pyr3;
            first = nf + 1;
        }
    for (int p = std::max(first, 1); p < geo.npyr; p++) {
        const ArLevel &L = geo.levels[(size_t)p], &Lp = geo.levels[(size_t)p - 1];
        const bool own = p > 1;   // the source is the detector's pyramid block
        const int spitch = own ? Lp.pitch : src_pitch;
        const size_t sfstride = own ? geo.pyr_fbytes : src_fstride;
        const unsigned salign = own ? (unsigned)(Lp.off & 15) : src_align;
        if (!geo.lvl_exact[(size_t)p]) k[(size_t)p] = PyrKernel::resize_level;
        else if (spitch % 8 == 0 && sfstride % 8 == 0 && (salign & 7) == 0 && L.pitch % 4 == 0 && L.pitch >= 4 * ((L.w + 3) / 4)) k[(size_t)p] = PyrKernel::half_area4;
        else k[(size_t)p] = PyrKernel::half_area;
    }
    return k;
}

// k_threshold_mfma: a 32-column strip per wave; c0 / c1 / c2 = byte columns of the three 16-byte pieces of a row it loads, tab = index
// (units of 64 uint4) of the strip's four pass-1 matrices
struct ThrStrip { int x0, c0, c1, c2, tab; };

// Tables of k_threshold_mfma: per 32-column strip the pass-1 matrices (box K blocks a / b, selection a / b) in the B-operand layout of
// v_mfma_i32_32x32x32_i8, BORDER_REPLICATE folded in; the pass-2 matrices (box over the previous / this block, centre x -WIN^2).
struct ThresholdTables {
    int cols = 0, win = 0;   // what they were built for (0: none)
    bool ok = false;         // false: the kernel does not apply (windows above 15, frames narrower than 48 pixels); the rest is void
    int rb = 0;              // rows / columns of halo in front of a block: 4 for radii up to 3, else 8
    std::vector<ThrStrip> strips;
    std::vector<uint8_t> tabs, tab2;
};

// Where k_threshold_mfma applies: windows up to 15 and frames at least 48 pixels wide.  plan_batch chooses the kernel by this, the
// handle builds and uploads the tables afterwards (tests/test_detector_plan_cpu.py: the tables of every such width and window come out ok)
inline bool threshold_tables_apply(int cols, int win) { return win / 2 <= 7 && cols >= 48; }

inline ThresholdTables plan_threshold_tables(int cols, int win)
{
    ThresholdTables t;
    t.cols = cols; t.win = win;
    const int R = win / 2, n2 = win * win, W = cols, rb = R <= 3 ? 4 : 8;
    if (!threshold_tables_apply(cols, win)) return t;
    t.tabs.reserve((size_t)(W + 31) / 32 * 4096);
    for (int X = 0; X < W; X += 32) {
        ThrStrip S{};
        S.x0 = X; S.tab = (int)(t.tabs.size() / 1024);
        auto cl = [&](int c) { return std::min(std::max(c, 0), W - 16); };
        S.c0 = cl(X - rb); S.c1 = cl(X - rb + 16); S.c2 = cl(X - rb + 32);
        const int cs[3] = {S.c0, S.c1, S.c2};
        // the piece that supplies input column x: the first that holds it (-1: none)
        auto owner = [&](int x) {
            for (int pz = 0; pz < 3; pz++)
                if (x >= cs[pz] && x < cs[pz] + 16) return pz;
            return -1;
        };
        const size_t base = t.tabs.size();
        t.tabs.resize(base + 4096, 0);
        // matrices a hold pieces 0 (lanes 0 .. 31) and 1 (lanes 32 .. 63), matrices b piece 2 (lanes 0 .. 31); lane = output column
        auto entry = [&](int m, int n, int piece, int x) -> uint8_t& {
            return t.tabs[base + (size_t)(m + (piece == 2)) * 1024 + (size_t)(n + 32 * (piece == 1)) * 16 + (x - cs[piece])];
        };
        for (int n = 0; n < 32 && X + n < W; n++) {
            for (int u = -R; u <= R; u++) {   // the taps of output column X + n, folded by BORDER_REPLICATE
                const int x = std::min(std::max(X + n + u, 0), W - 1), piece = owner(x);
                if (piece < 0) return t;      // an input column the strip's windows reach comes with none of the three pieces
                entry(0, n, piece, x) += 1;
            }
            entry(2, n, owner(X + n), X + n) = 1;
        }
        t.strips.push_back(S);
    }
    t.tab2.assign(6144, 0);
    const int cw1 = n2 <= 127 ? n2 : 113, cw2 = n2 - cw1;   // the centre's weight -n2 in one signed byte, or in two
    for (int m = 0; m < 6; m++)   // box over the previous block, over this block, centre in the previous block, in this block (x 2)
        for (int lane = 0; lane < 64; lane++) {
            const int n = lane & 31, half = lane >> 5;
            for (int i = 0; i < 16; i++) {
                const int q = 4 * half + (i & 3) + 8 * (i >> 2);
                const int d = ((m & 1) ? 32 : 0) + q - rb - n;   // the row's offset from the output row
                int v = 0;
                if (m < 2) v = (d >= -R && d <= R) ? 1 : 0;
                else v = d == 0 ? -(m < 4 ? cw1 : cw2) : 0;
                t.tab2[(size_t)m * 1024 + (size_t)lane * 16 + i] = (uint8_t)(int8_t)v;
            }
        }
    t.rb = rb;
    t.ok = true;
    return t;
}

// ---- the detector's switches: what a handle may be told about HOW it runs (never about what it computes: every path is bit-exact).
// The handle keeps one of these; read_detector_env fills the environment-driven fields once, at creation, and
// orbfe_aruco_debug_control / orbfe_aruco_set_big_frames change the fields that have a key.  plan_batch reads nothing else.
struct DetectorSwitches {
    // the tiled relay formulation (aruco_tiles.hip: k_ct_band or k_ct_walk / k_ct_lists / k_ct_points).  -1 = by frame and batch size:
    // frames for which the one-workgroup relay kernel needs its 8192-slot table and a CU to itself (1280 x 720: 300-frame step 4.09 -
    // 4.13 -> 3.96 - 4.07 ms) or whose bit image does not fit LDS at all (1920 x 1080: 100-frame step 4.88 -> 3.41 ms), and batches of
    // up to 32 frames (a frame's walks spread over ~40 CUs instead of one); full batches of 640 x 480 frames keep the one-workgroup
    // kernel, whose single launch costs the pipeline less than band + lists + points (1.32 - 1.34 against 1.45 - 1.62 ms per step).
    // ORBFE_ARUCO_TILED = 0 / 1 (debug key "tiled_contours") forces it off / on for every batch (tests, A/B)
    int tiled = -1;
    // the walks of the tiled path by BANDS of cell rows, a workgroup of eight waves each (k_ct_band), instead of a wave per tile
    // (k_ct_walk): -1 = by frame / batch size, 0 / 1 forced (ORBFE_ARUCO_BANDED)
    int banded = -1;
    int band_rows = 0;   // ORBFE_ARUCO_BAND_ROWS = cell rows per band (0: what fits ~36 KB of LDS, at most 8)
    int tile_w = 0;      // ORBFE_ARUCO_TILE_W = tile width in pixels of k_ct_walk, ORBFE_ARUCO_TPW = its tiles per wave: measurement
    int tpw = 0;         // switches (0: by batch size)
    int lcap = 0;        // ORBFE_ARUCO_LCAP > 0: list elements k_ct_lists keeps in LDS (a measurement switch; an input of plan_detector)
    // The speck passes (aruco_trace.hpp "FEWER WALKS" (2)): result-neutral, a quarter of the contour stage's start candidates and walks
    // gone -- and OFF by default, because neither way of running them pays in the pipeline:
    //   = 1: as a launch of their own between threshold and contours (k_speck_clean), for every contour path: the contour stage of
    //     300 x 640 x 480 alone 462 -> 408 us, but one more launch on the detector's chain costs the pipeline more than that (C2 step
    //     1.40 - 1.46 against 1.34 - 1.38 ms, single-frame detect 0.357 against 0.358 ms; profiles/r05_contour_reductions_ab.txt);
    //   = 2: inside the one-workgroup relay kernels, on the bit image they hold in LDS anyway (speck_pass_frame; batches of more than
    //     32 frames whose image fits LDS): 462 -> 440 us alone and 140 -> 120 us of VALU issue, the C2 step unchanged (1.343 against
    //     1.333 ms, four interleaved runs) -- and the rim masks and anchors of a frame (120 KB) go through scratch in HBM, which
    //     doubles the stage's HBM traffic (148 -> 268 MB per step).
    // ORBFE_ARUCO_SPECKS = 0 (default) / 1 / 2.  Debug keys "speck_passes": the launch on / off, "speck_passes_in_kernel": inside.
    // Tested either way (tests/test_aruco_gpu.py, tests/test_stress_gpu.py).
    // the speck passes as a launch between threshold and contours: -1 = where they pay (full batches on the one-workgroup relay kernels:
    // 1.246 against 1.263 ms per C2 step with them, round 6; on the tiled paths 3.99 against 3.74 ms at 1280 x 720, 3.53 against 3.21 at
    // 1920 x 1080), 0 / 1 = never / wherever their tile fits LDS
    int specks = -1;
    bool specks_inkernel = false;   // (an input of plan_detector: the relay kernels' scratch grows by the passes' rim masks)
    bool relay_wide = true;   // k_contours_relay_wide for up to 32 frames that fit the 4096-slot table (ORBFE_ARUCO_RELAY_WIDE=0: k_contours_relay)
    // phase (c) of LDS-resident frames as its own launch (k_contours_small): -1 = by batch size (a few frames leave most of the chip
    // idle, so the many small workgroups of the separate kernel shorten the call: 0.62 -> 0.57 ms for one 640 x 480 frame; a full
    // batch issues more instructions that way and the pipeline is bound by those: 1.85 -> 1.98 ms per C2 step), 0 / 1 = forced
    // (ORBFE_ARUCO_SMALL_SEPARATE)
    int small_separate = -1;
    bool thr_mfma = true;        // k_threshold_mfma where it applies (windows up to 15; debug key "threshold_mfma" = 1 / 0)
    bool thr_mfma_auto = true;   // ... but k_threshold_pyr for calls of fewer than 8 frames ("threshold_mfma" = 1 forces the matrix-core kernel, -1 = this rule again)
    bool thr_pyr = true;         // k_threshold_pyr where it applies (debug key "threshold_pyr": the tests run both threshold kernels)
    bool half_pyr = true;        // the leading exact pyramid levels in one launch (k_half_pyr; debug key "half_pyr")
    bool force_legacy = false;   // debug key "legacy_contours": always k_contours_t, and no retry on another path
    bool big_mode = false;       // orbfe_aruco_set_big_frames: every batch on Contours::big (a retry passes its path to plan_batch instead)
};

// The ORBFE_ARUCO_* variables, each looked up once (the library passes getenv, a test a table).  A variable that is not set leaves
// its field as it is.
typedef const char* (*EnvLookup)(const char* name);
inline void read_detector_env(DetectorSwitches& sw, EnvLookup env)
{
    auto num = [&](const char* name, int unset) { const char* v = env(name); return v ? atoi(v) : unset; };
    auto tri = [&](const char* name, int unset) { const char* v = env(name); return v ? (atoi(v) ? 1 : 0) : unset; };
    sw.relay_wide = num("ORBFE_ARUCO_RELAY_WIDE", 1) != 0;
    sw.small_separate = num("ORBFE_ARUCO_SMALL_SEPARATE", sw.small_separate);
    sw.tiled = tri("ORBFE_ARUCO_TILED", sw.tiled);
    sw.banded = tri("ORBFE_ARUCO_BANDED", sw.banded);
    sw.band_rows = num("ORBFE_ARUCO_BAND_ROWS", sw.band_rows);
    sw.tile_w = num("ORBFE_ARUCO_TILE_W", sw.tile_w);
    sw.tpw = num("ORBFE_ARUCO_TPW", sw.tpw);
    sw.lcap = num("ORBFE_ARUCO_LCAP", sw.lcap);
    if (const char* v = env("ORBFE_ARUCO_SPECKS")) { sw.specks = atoi(v) == 1; sw.specks_inkernel = atoi(v) == 2; }
}

// The contour paths: tiled (aruco_tiles.hip), the one-workgroup relay kernels, k_contours_t where neither can run or forced ("walker"),
// k_contours_t in big-frame mode (bit image in HBM, AR_MAX_KEPT_BIG kept borders).  A batch with a frame over a capacity of its path is
// done again on the next (escalate(): tiled -> relay, which coarsen their grid -> (kept borders / pool) big); plan_batch takes the first.
enum class Contours : int8_t { tiled, relay, walker, big, none };
enum class Thr : int8_t { fixed, mfma, pyr, box };   // k_fixed_threshold, k_threshold_mfma, k_threshold_pyr<WIN>, k_adaptive_threshold<R>
enum class Relay : int8_t { relay, relay8, wide, relay8g }; // k_contours_relay, _relay8, _relay_wide, _relay8g

// The path a batch is done again on: `ran` = the one it took, flags_or = the union of its frames' flag words, relay_ok = the relay
// kernels can run at this image size (DetectorGeometry::relay_tbits).  Contours::none: the batch stands.
inline Contours escalate(Contours ran, int flags_or, bool relay_ok)
{
    const bool was_tiled = ran == Contours::tiled;
    // from the tiled path any exceeded capacity (segment lists, kept borders, pool) goes to the one-workgroup relay kernels first:
    // they coarsen their grid and follow what is left whole, and get through frames of dense noise that neither the tiles nor the
    // single-walker kernel's per-lane arenas hold (480 x 640 with +-40 grey levels of noise: 203 kept borders, no flag)
    if (was_tiled && (flags_or & (AR_CAPACITY_FLAGS | RL_FALLBACK_FLAGS)) && relay_ok) return Contours::relay;
    return ran != Contours::big && (flags_or & (AR_CAPACITY_FLAGS | (was_tiled ? RL_FALLBACK_FLAGS : 0))) ? Contours::big : Contours::none;
}

// What a run of the pipeline is asked for besides its frames: THRES_AUTO_FIXED instead of the adaptive threshold, a reduced working
// image under the full frame's pyramid (minSize > 0), Params::ThresHold
struct BatchMode {
    bool adaptive = true, reduced = false;
    int thres_value = 7;
};

// What run_device launches for a batch: every choice of kernel, variant and size, made once before its first launch
struct BatchPlan {
    Thr thr = Thr::box; uint32_t thr_kk = 0;   // the threshold kernel; k_threshold_pyr: K | K << 16
    int nfuse = 0;                // pyramid levels k_threshold_pyr writes, the rest in line behind it (0: the pyramid on the aux stream)
    bool specks = false;          // k_speck_clean between threshold and contours
    Contours contours = Contours::tiled;   // the path that runs; its variants:
    bool band = false; int band_rows = 0, tile_w = 0, tpw = 0;   // tiled: k_ct_band, band_rows cell rows a band (else k_ct_walk: tile_w-pixel tiles, tpw tiles a wave)
    Relay relay = Relay::relay;   // relay: the kernel, and k_contours_small behind it or not
    bool small_separate = false, walker_hbm = false;   // walker: k_contours_t with its bit image in HBM and AR_MAX_KEPT_BIG kept borders
};

// The plan of a batch of B frames on geometry `geo`: the first contour path from `floor` on that may run (escalate()), and every
// choice that depends on the batch size.  Host arithmetic only: Thr::mfma means the tables apply, the handle uploads them afterwards.
inline BatchPlan plan_batch(const DetectorGeometry& geo, int B, const BatchMode& m, Contours floor, const DetectorSwitches& sw)
{
    BatchPlan p;
    // The threshold kernel of the batched configuration writes the pyramid levels its 64 x 64 tiles hold whole (k_threshold_pyr): the
    // exact halvings, at most four, when the pyramid starts from the thresholded frame itself and n v + K stays within 16 bits
    const long n2 = (long)geo.win * geo.win, K = n2 * m.thres_value - n2 / 2;
    const bool win_t = geo.win == 5 || geo.win == 7 || geo.win == 11 || geo.win == 15;
    const bool fused_ok = m.adaptive && sw.thr_pyr && win_t && K >= 0 && n2 * 255 + K <= 65535;
    // A call of a few frames (the drop-in call: one) is a chain of launches that each wait for the one before: there the kernel that
    // also writes the pyramid (one launch instead of five) is the shorter chain -- detect 0.333 -> 0.303 ms per 640 x 480 frame;
    // a batch has the pyramid next to the contour kernels on a stream of its own and takes the matrix-core kernel
    const bool try_mfma = m.adaptive && sw.thr_mfma && K > -(1 << 20) && K < (1 << 20) && !(fused_ok && !m.reduced && B < 8 && sw.thr_mfma_auto);
    p.thr = !m.adaptive ? Thr::fixed : try_mfma && threshold_tables_apply(geo.cols, geo.win) ? Thr::mfma : fused_ok ? Thr::pyr : Thr::box;
    if (p.thr == Thr::pyr) p.thr_kk = (uint32_t)K | ((uint32_t)K << 16);
    for (int l = 1; p.thr == Thr::pyr && !m.reduced && l < geo.npyr && l <= 4; l++) {
        if (!geo.lvl_exact[l] || geo.levels[l].pitch % 4 != 0 || geo.levels[l].pitch < 4 * ((geo.levels[l].w + 3) / 4)) break;
        p.nfuse = l;
    }
    // the first contour path from `floor` on that may run (big_mode: orbfe_aruco_set_big_frames; the tiled rule: at `tiled`)
    if (sw.big_mode || floor >= Contours::big) p.contours = Contours::big;
    else if (!sw.force_legacy && floor <= Contours::tiled && (sw.tiled > 0 || (sw.tiled < 0 && (geo.relay_global || !geo.relay_tbits || geo.relay_tbits > 12 || B <= 32))))
        p.contours = Contours::tiled;
    else p.contours = !sw.force_legacy && floor <= Contours::relay && geo.relay_tbits ? Contours::relay : Contours::walker;
    // the bit image the contour kernels read: after the speck passes, unless switched off or the frame is too wide for their LDS tile
    p.specks = (sw.specks > 0 || (sw.specks < 0 && p.contours == Contours::relay && !geo.relay_global && B > 32)) && speck_lds_bytes(geo.cols) <= 150 * 1024;
    // Tile width and waves.  k_ct_walk's waves are persistent and overlap their tiles, so a wave wants several tiles (its
    // lanes always find work) and a SIMD wants several waves (a step is a chain of dependent LDS reads): narrow tiles for a
    // batch -- ORBFE_ARUCO_TILE_W / ORBFE_ARUCO_TPW (tiles per wave) are measurement switches --, and for a few frames as many
    // waves as there are tiles.
    const int target = sw.tile_w > 0 ? sw.tile_w : (B <= 32 ? 192 : 480), ncols0 = std::max(1, (geo.cols + target - 1) / target);
    p.tile_w = std::min(CTW_MAX_CW, std::max(32, ((geo.cols + ncols0 - 1) / ncols0 + 31) / 32 * 32));
    p.tpw = sw.tpw > 0 ? sw.tpw : (B <= 32 ? 1 : 2);
    // bands for full batches (eight waves level each other's load through the band's ticket counters) and, one cell row each, for
    // up to four frames (single-frame call 0.385 -> 0.355 ms: the waves of a band share its start candidates, where a wave of
    // k_ct_walk has its tile's to itself); a wave per tile in between
    p.band = sw.banded > 0 || (sw.banded < 0 && (B > 32 || B <= 4));
    const int pw = (geo.cols + 2 + 31) / 32, rb = sw.band_rows > 0 ? sw.band_rows : B <= 4 ? 1 : std::max(1, std::min(8, (int)((36 * 1024 / (pw * 4) - 3) / 32)));
    p.band_rows = std::max(1, std::min(rb, (geo.rows + 31) / 32));
    const bool wide = geo.relay_tbits <= 12 && B <= 32 && sw.relay_wide;   // few frames: 16 waves per frame (see k_contours_relay_wide)
    p.relay = geo.relay_global ? Relay::relay8g : geo.relay_tbits > 12 ? Relay::relay8 : wide ? Relay::wide : Relay::relay;
    p.small_separate = geo.relay_global || (sw.small_separate < 0 ? B <= 32 : sw.small_separate != 0);   // (always behind relay8g)
    p.walker_hbm = p.contours == Contours::big || !geo.lds_bits_words;
    return p;
}

} // namespace orbfe
