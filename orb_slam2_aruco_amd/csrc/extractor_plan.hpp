// extractor_plan.hpp -- what the ORB extractor's kernels are told about a rows x cols input: the level geometry, the cv::resize
// coefficient tables, the blur kernel's strips and tap matrices, the quadtree's LDS capacities.  Pure host arithmetic, no HIP:
// csrc/orb_extractor.hip computes a plan per input size and uploads it, tests/test_extractor_plan_cpu.py compiles this header with
// g++ and checks it against the oracle.  A plan is a value: plan_extractor() returns either a complete one or an error (err, msg).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../include/orbfe.h"
#include "../../include/orbfe_math.h"
#include "input_layout.hpp"   // plan_input_layout: the layouts of a caller's device frames the kernels can address

namespace orbfe {

// Geometry of one pyramid level, computed on the host with the reference's own float arithmetic
// (ORBextractor.cc:767-787, :546-558) and read by every kernel.
struct LevelGeom {
    int w, h;            // level image size (:1112)
    int pitch;           // row pitch of the level inside the pyramid block (levels >= 1)
    int btrow;           // bytes from one row of tiles to the next inside the blurred block (blur_tile_off)
    long long img_off;   // byte offset of the level inside a frame's pyramid block (levels >= 1)
    long long blur_off;  // byte offset inside a frame's blurred block
    int nCols, nRows, wCell, hCell; // FAST cell grid (:784-787)
    int maxBX, maxBY;    // maxBorderX/Y (:774-775); minBorder is 16
    int cell_first;      // index of the level's first active cell in the frame's cell array
    int ncells;          // active cells (rows/cols skipped at :795,:804 are not materialised)
    int cell_cap;        // candidate slots per cell: ceil(wCell/2)*ceil(hCell/2) (no two NMS survivors are adjacent)
    long long slot_off;  // u32 offset of the level's slots inside a frame's slot block
    int cand_cap;        // ncells * cell_cap
    long long cand_off;  // u32 offset (per ping-pong half) inside a frame's key scratch
    int quota;           // mnFeaturesPerLevel[level] (:435-446)
    int out_cap;         // slots for the level's distributed keypoints
    int out_off;         // u32 offset inside a frame's lvl_out block
    int nIni;            // root nodes (:543)
    float hX;            // (:545)
    float scale;         // mvScaleFactor[level]
    float kp_size;       // (float)(int)(31 * scale) (:837)
};

// The blurred pyramid is stored in tiles of 128 bytes, one cache line each: BLUR_TW bytes of BLUR_TH consecutive rows, the tiles of a
// level row-major, every level a whole number of tiles.  Its writer (k_blur7_mfma, 32-column strips) and its reader (k_orient_describe2,
// a 37 x 37 window per keypoint) both work on 2-D pieces: a window lies in 15 - 24 lines instead of the 37 - 74 of a row-major level,
// and a store instruction of the blur (256 bytes) writes two whole lines.  blur_tile_off is the one place that knows the layout: the
// two kernels and the host's de-tiling (orbfe_extractor_debug_level_image) call it.  16 bytes at a column that is a multiple of 16 are
// contiguous.  Padding columns and rows inside a level's last tiles hold whatever the blur computed there; nothing reads them.
constexpr int BLUR_TW = 16, BLUR_TH = 8;   // (32 x 4 measured equal at 640 x 480: tools/sweeps.md; a window lies in fewer of these)
static_assert(BLUR_TW * BLUR_TH == 128 && BLUR_TW % 16 == 0, "a tile is one 128-byte line of whole 16-byte chunks");

// byte offset of pixel (x, y), both >= 0, inside a level whose rows of tiles are `trow` bytes apart (LevelGeom::btrow)
ORBFE_HD uint32_t blur_tile_off(int trow, int x, int y)
{
    const uint32_t ux = (uint32_t)x, uy = (uint32_t)y;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t rows = __umul24(uy / BLUR_TH, (uint32_t)trow);
#else
    const uint32_t rows = uy / BLUR_TH * (uint32_t)trow;
#endif
    return rows + ux / BLUR_TW * 128u + (uy % BLUR_TH * BLUR_TW + ux % BLUR_TW);
}
inline int blur_tiles_x(int w) { return (w + BLUR_TW - 1) / BLUR_TW; }
inline int blur_tiles_y(int h) { return (h + BLUR_TH - 1) / BLUR_TH; }
// (level geometry, x, y) -> byte offset inside a frame's blurred block
template <class Geom> ORBFE_HD long long blur_pixel_off(const Geom& g, int x, int y) { return g.blur_off + (long long)blur_tile_off(g.btrow, x, y); }

// k_blur7_mfma: a 32-column strip of a level per wave; c0 / c1 / c2 = byte columns of the three 16-byte pieces of a row it loads, tab =
// index (units of 64 uint4) of the strip's two pass-1 tap matrices in operand layout (plan_blur_level)
struct BlurStrip { int level, x0, c0, c1, c2, tab; };

#define QT_MAXROOTS 16   // root nodes of DistributeOctTree (nIni = round(width / height), ORBextractor.cc:544) the kernels hold

// dynamic LDS of k_distribute_pyr (count pyramid of depth D over nIni roots) and of k_distribute (keycap_lds keys in LDS)
inline size_t qp_lds_bytes(int nIni, int D, int nodecap, int veccap)
{
    const size_t nleaf = (size_t)nIni << (2 * D);
    const size_t T = (size_t)nIni * (((1u << (2 * (D + 1))) - 1) / 3);
    size_t b = nleaf * 4 + (size_t)veccap * 16 + (size_t)nodecap * 24;
    b += 2 * (((size_t)nodecap * 2 + 15) & ~(size_t)15);
    b += (T / 2 + 4) * 4;
    return b + 32;
}
inline size_t qt_lds_bytes(int keycap_lds, int nodecap, int veccap)
{
    size_t b = (size_t)veccap * 16;                 // vec + vprev
    b += (size_t)nodecap * 12;                      // begin, count, seq
    b += (size_t)nodecap * 14;                      // x0,y0,x1,y1,next,prev,free
    b += ((size_t)nodecap + 15) & ~(size_t)15;      // flags
    b = (b + 15) & ~(size_t)15;
    b += (size_t)keycap_lds * 8;                    // two key buffers
    return b + 16;
}

struct ExtractorPlan {
    int err = ORBFE_OK;              // ORBFE_OK, or why this input is refused (then nothing else below is meaningful)
    char msg[256] = "";
    int rows = 0, cols = 0;
    bool gaussian_ed = false;        // the blur taps the tables were built for
    // level geometry, and the layout of every per-frame block
    std::vector<LevelGeom> geom;
    std::vector<uint32_t> cellinfo;  // per active cell: level | row << 4 | column << 14
    int ncells_total = 0, out_total = 0, max_out_cap = 0, max_wcell = 0, max_hcell = 0, max_ini = 1;
    size_t pyr_fbytes = 0, blur_fbytes = 0, slots_fu32 = 0, keys_fu32 = 0;
    // cv::resize tables of levels >= 1
    std::vector<int> resize_tabs;
    std::vector<size_t> tab_off;     // per level: offsets (in ints) of xofs, xalpha, ytab in resize_tabs
    std::vector<char> resize_tab_ok; // per level >= 1: k_resize_tab's 8-byte windows fit
    // k_blur7_mfma: the strips (level-major), per strip two pass-1 tap matrices, and the two pass-2 matrices
    std::vector<BlurStrip> blur_strips;
    std::vector<uint8_t> blur_tabs, blur_tab2;
    // quadtree: node and vector capacities of a workgroup, and how many keys of the general kernel fit LDS next to them
    int nodecap = 0, veccap = 0, keycap_lds = 0;
};

inline int plan_fail(ExtractorPlan& p, int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(p.msg, sizeof(p.msg), fmt, ap);
    va_end(ap);
    return p.err = code;
}

inline int plan_align_up(int v, int a) { return (v + a - 1) / a * a; }

// Level geometry for p.rows x p.cols: pyramid sizes (:1112), cell grid (:767-787), quadtree roots (:543-558), plus the HBM layout of
// every per-frame block.
inline int plan_levels(ExtractorPlan& p, int nlevels, const float* mvScaleFactor, const float* mvInvScaleFactor, const int* mnFeaturesPerLevel)
{
    p.geom.assign(nlevels, LevelGeom{});
    size_t pyr = 0, blur = 0, slots = 0, cand = 0;
    for (int l = 0; l < nlevels; l++) {
        LevelGeom& g = p.geom[l];
        const float scale = mvInvScaleFactor[l];
        g.w = orbfe_round_f((float)p.cols * scale);
        g.h = orbfe_round_f((float)p.rows * scale);
        // the reference's own limit: its cell grid needs nCols = (w - 32) / 30 >= 1 (ORBextractor.cc:780-784; below that it divides by zero)
        if (g.w < 32 + 30 || g.h < 32 + 30)
            return plan_fail(p, ORBFE_ERR_INVALID, "level %d is %dx%d: too small for a FAST cell grid (62 pixels a side)", l, g.w, g.h);
        // a keypoint travels as x | y << 12 | score << 24 relative to the 16-px border
        if (g.w - 32 > 4095 || g.h - 32 > 4095)
            return plan_fail(p, ORBFE_ERR_INVALID, "level %d is %dx%d: images above 4127 px a side are unsupported", l, g.w, g.h);
        g.pitch = plan_align_up(g.w, 64);
        g.btrow = blur_tiles_x(g.w) * 128;
        g.img_off = (long long)pyr;
        if (l > 0) pyr += (size_t)g.pitch * g.h;
        g.blur_off = (long long)blur;
        blur += (size_t)g.btrow * blur_tiles_y(g.h);
        g.maxBX = g.w - 19 + 3;
        g.maxBY = g.h - 19 + 3;
        const float width = (float)(g.maxBX - 16), height = (float)(g.maxBY - 16);
        g.nCols = (int)(width / 30.f);
        g.nRows = (int)(height / 30.f);
        g.wCell = (int)std::ceil(width / g.nCols);
        g.hCell = (int)std::ceil(height / g.nRows);
        if (g.wCell > 60 || g.hCell > 60) return plan_fail(p, ORBFE_ERR_INVALID, "cell larger than 60 px");
        p.max_wcell = std::max(p.max_wcell, g.wCell); p.max_hcell = std::max(p.max_hcell, g.hCell);
        g.cell_first = (int)p.cellinfo.size();
        for (int i = 0; i < g.nRows; i++) {
            const float iniY = (float)(16 + i * g.hCell);
            if (iniY >= g.maxBY - 3) continue;
            for (int j = 0; j < g.nCols; j++) {
                const float iniX = (float)(16 + j * g.wCell);
                if (iniX >= g.maxBX - 6) continue;
                p.cellinfo.push_back((uint32_t)l | ((uint32_t)i << 4) | ((uint32_t)j << 14));
            }
        }
        g.ncells = (int)p.cellinfo.size() - g.cell_first;
        g.cell_cap = ((g.wCell + 1) / 2) * ((g.hCell + 1) / 2);
        g.slot_off = (long long)slots;
        g.cand_cap = g.ncells * g.cell_cap;
        slots += (size_t)g.cand_cap;
        g.cand_off = (long long)cand;
        cand += (size_t)g.cand_cap;
        g.quota = mnFeaturesPerLevel[l];
        g.nIni = (int)std::round(static_cast<float>(g.maxBX - 16) / (g.maxBY - 16));
        if (g.nIni < 1 || g.nIni > QT_MAXROOTS)
            return plan_fail(p, ORBFE_ERR_INVALID, "aspect ratio gives %d quadtree roots (supported: 1..%d)", g.nIni, QT_MAXROOTS);
        p.max_ini = std::max(p.max_ini, g.nIni);
        g.hX = static_cast<float>(g.maxBX - 16) / g.nIni;
        g.out_cap = std::max(g.quota + 3, 4 * g.nIni) + 5;
        g.out_off = p.out_total;
        p.out_total += g.out_cap;
        p.max_out_cap = std::max(p.max_out_cap, g.out_cap);
        g.scale = mvScaleFactor[l];
        g.kp_size = (float)(int)(31 * mvScaleFactor[l]);
    }
    p.ncells_total = (int)p.cellinfo.size();
    p.pyr_fbytes = pyr + 64;
    p.blur_fbytes = blur + 128;   // (a frame's block stays a whole number of lines; k_orient_describe2 reads nothing outside a level's tiles)
    p.slots_fu32 = slots;
    p.keys_fu32 = 2 * cand;
    return ORBFE_OK;
}

// cv::resize(INTER_LINEAR) coefficient tables of every level >= 1, OpenCV 3.4
inline void plan_resize_tables(ExtractorPlan& p)
{
    const int nlevels = (int)p.geom.size();
    std::vector<int>& tabs = p.resize_tabs;
    p.tab_off.assign((size_t)nlevels * 3, 0);
    p.resize_tab_ok.assign((size_t)nlevels, 0);
    for (int l = 1; l < nlevels; l++) {
        const int sw = p.geom[l - 1].w, sh = p.geom[l - 1].h, dw = p.geom[l].w, dh = p.geom[l].h;
        const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
        const int dwp = plan_align_up(dw, 4);
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
        p.resize_tab_ok[l] = ok;
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
        p.tab_off[l * 3 + 0] = tabs.size(); tabs.insert(tabs.end(), xofs.begin(), xofs.end());
        p.tab_off[l * 3 + 1] = tabs.size(); tabs.insert(tabs.end(), xal.begin(), xal.end());
        while (tabs.size() % 4) tabs.push_back(0); // ... and ytab as int4
        p.tab_off[l * 3 + 2] = tabs.size(); tabs.insert(tabs.end(), ytab.begin(), ytab.end());
    }
}

inline const int* blur_taps(bool gaussian_ed)   // orbfe_extractor_set_gaussian_taps: 18 34 48 56 48 34 18 instead of 18 34 49 55 49 34 18
{
    static const int T0[7] = {18, 34, 49, 55, 49, 34, 18}, T1[7] = {18, 34, 48, 56, 48, 34, 18};
    return gaussian_ed ? T1 : T0;
}

// Strips and pass-1 tap matrices of k_blur7_mfma for one level of width w whose rows hold `rowbytes` readable bytes (level 0: w, the
// caller's image; levels >= 1: the pitch): per strip the two matrices in the B-operand layout of v_mfma_i32_32x32x32_i8 (lane (n, half)
// holds B[16 half + i][n], i = 0 .. 15, as 16 bytes), BORDER_REFLECT_101 folded in.  False if a strip's taps do not fit the kernel: an
// input column outside the three 16-byte pieces it loads, or a folded weight above 127.
inline bool plan_blur_level(int l, int w, int rowbytes, const int* t, std::vector<BlurStrip>& st, std::vector<uint8_t>& tabs)
{
    if (w < 48 || rowbytes < 16) return false;
    auto refl = [](int p, int n) { while (p < 0 || p >= n) p = (p < 0) ? -p : 2 * (n - 1) - p; return p; };
    for (int X = 0; X < w; X += 32) {
        BlurStrip S{};
        S.level = l; S.x0 = X; S.tab = (int)(tabs.size() / 1024);
        auto cl = [&](int c) { return std::min(std::max(c, 0), rowbytes - 16); };
        S.c0 = cl(X - 4); S.c1 = cl(X + 12); S.c2 = cl(X + 28);
        const int cs[3] = {S.c0, S.c1, S.c2};
        // weight of input column xlo + i for output column X + n: the strip's 32 outputs read columns X - 3 .. X + 34, folded into the image
        const int xlo = std::max(0, X - 3), nx = std::min(w, X + 35) - xlo;
        std::vector<int> W((size_t)nx * 32, 0), owner((size_t)nx, -1);
        for (int n = 0; n < 32; n++) {
            if (X + n >= w) continue;
            for (int u = 0; u < 7; u++) W[(size_t)(refl(X + n + u - 3, w) - xlo) * 32 + n] += t[u];
        }
        for (int i = 0; i < nx; i++)
            for (int pz = 0; pz < 3 && owner[i] < 0; pz++)
                if (xlo + i >= cs[pz] && xlo + i < cs[pz] + 16) owner[i] = pz;
        for (int i = 0; i < nx; i++)
            for (int n = 0; n < 32; n++)
                if (W[(size_t)i * 32 + n] && (owner[i] < 0 || W[(size_t)i * 32 + n] > 127)) return false;
        const size_t base = tabs.size();
        tabs.resize(base + 2048, 0);
        for (int ab = 0; ab < 2; ab++)
            for (int lane = 0; lane < 64; lane++) {
                const int n = lane & 31, half = lane >> 5;
                const int piece = ab == 0 ? half : (half == 0 ? 2 : -1);
                if (piece < 0) continue;
                for (int i = 0; i < 16; i++) {
                    const int x = cs[piece] + i;
                    if (x < xlo || x >= xlo + nx || owner[x - xlo] != piece) continue;
                    tabs[base + (size_t)ab * 1024 + (size_t)lane * 16 + i] = (uint8_t)(int8_t)W[(size_t)(x - xlo) * 32 + n];
                }
            }
        st.push_back(S);
    }
    return true;
}

// Tables of k_blur7_mfma for the geometry and the taps: plan_blur_level for every level, and the two pass-2 matrices whose K index runs
// over a block's rows in the order pass 1 leaves them in a lane's registers.
inline int plan_blur_tables(ExtractorPlan& p)
{
    const int* t = blur_taps(p.gaussian_ed);
    for (int l = 0; l < (int)p.geom.size(); l++)
        if (!plan_blur_level(l, p.geom[l].w, l == 0 ? p.geom[l].w : p.geom[l].pitch, t, p.blur_strips, p.blur_tabs))
            return plan_fail(p, ORBFE_ERR_INVALID, "level %d is %d pixels wide: its blur taps do not fit the matrix-core kernel's strips", l, p.geom[l].w);
    p.blur_tab2.assign(2048, 0);
    for (int ab = 0; ab < 2; ab++)
        for (int lane = 0; lane < 64; lane++) {
            const int n = lane & 31, half = lane >> 5;
            for (int i = 0; i < 16; i++) {
                const int q = 4 * half + (i & 3) + 8 * (i >> 2);
                const int u = ab == 0 ? q - n - 1 : q - n + 31;
                if (u >= 0 && u <= 6) p.blur_tab2[(size_t)ab * 1024 + (size_t)lane * 16 + i] = (uint8_t)t[u];
            }
        }
    return ORBFE_OK;
}

// The node lists of DistributeOctTree live in LDS, sized by the largest per-level quota: refuse here what would not fit, not at launch
inline int plan_quadtree_capacity(ExtractorPlan& p)
{
    p.nodecap = p.max_out_cap + 8;
    p.veccap = 1;
    while (p.veccap < p.nodecap) p.veccap <<= 1;
    // the general kernel's key buffers share LDS with the node lists: large quotas leave less room (levels whose candidates do not fit
    // work out of the HBM key scratch)
    const long long room = (long long)160 * 1024 - 3072 - (long long)qt_lds_bytes(0, p.nodecap, p.veccap);
    p.keycap_lds = (int)std::max<long long>(0, std::min<long long>(6144, room / 8)) & ~63;
    const size_t need = std::max(qp_lds_bytes(p.max_ini, p.max_ini <= 4 ? 5 : 4, p.nodecap, p.veccap), qt_lds_bytes(p.keycap_lds, p.nodecap, p.veccap));
    if (need + 2048 > (size_t)160 * 1024)
        return plan_fail(p, ORBFE_ERR_CAPACITY, "a pyramid level's quota of %d keypoints needs %zu bytes of LDS for the quadtree: more than a "
                         "workgroup has (about 2700 keypoints per level fit)", p.max_out_cap, need);
    return ORBFE_OK;
}

// The plan of a rows x cols input for an extractor with the constructor's tables (ORBextractor.cc:410-446) and blur taps
inline ExtractorPlan plan_extractor(int rows, int cols, int nlevels, const float* mvScaleFactor, const float* mvInvScaleFactor,
                                    const int* mnFeaturesPerLevel, bool gaussian_ed)
{
    ExtractorPlan p;
    p.rows = rows; p.cols = cols; p.gaussian_ed = gaussian_ed;
    if (plan_levels(p, nlevels, mvScaleFactor, mvInvScaleFactor, mnFeaturesPerLevel) || plan_quadtree_capacity(p)) return p;
    plan_resize_tables(p);
    plan_blur_tables(p);
    return p;
}

} // namespace orbfe
