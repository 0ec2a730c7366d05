// C entry points over csrc/extractor_plan.hpp for tests/test_extractor_plan_cpu.py (built with g++ by tests/extractor_plan_build.py:
// the header has no HIP in it).  Test infrastructure only.
#include <cstring>

#include "../orb_slam2_aruco_amd/csrc/extractor_plan.hpp"

using namespace orbfe;

extern "C" {

// The plan of a rows x cols input.  levels: 12 ints per level (w, h, nCols, nRows, wCell, hCell, ncells, quota, nIni, out_cap,
// resize_tab_ok, number of blur strips); scalars: nodecap, veccap, keycap_lds, max_wcell, max_hcell, max_ini, ncells_total, out_total.
// Returns the plan's error code; msg receives its message.
int xplan_make(int rows, int cols, int nlevels, const float* scale, const float* inv_scale, const int* quota, int gaussian_ed,
               int* levels, int* scalars, char* msg, int msgcap)
{
    const ExtractorPlan p = plan_extractor(rows, cols, nlevels, scale, inv_scale, quota, gaussian_ed != 0);
    snprintf(msg, (size_t)msgcap, "%s", p.msg);
    if (p.err) return p.err;
    for (int l = 0; l < nlevels; l++) {
        const LevelGeom& g = p.geom[(size_t)l];
        int strips = 0;
        for (const BlurStrip& s : p.blur_strips) strips += s.level == l;
        const int v[12] = {g.w, g.h, g.nCols, g.nRows, g.wCell, g.hCell, g.ncells, g.quota, g.nIni, g.out_cap, p.resize_tab_ok[(size_t)l], strips};
        memcpy(levels + 12 * l, v, sizeof(v));
    }
    const int s[8] = {p.nodecap, p.veccap, p.keycap_lds, p.max_wcell, p.max_hcell, p.max_ini, p.ncells_total, p.out_total};
    memcpy(scalars, s, sizeof(s));
    return ORBFE_OK;
}

// plan_blur_level for every width w_first .. w_last, both tap sets, both row-length rules (level 0: w readable bytes a row; levels >= 1:
// w rounded up to 64).  Returns how many of the (w, taps, rule) combinations the matrix-core tables refuse; first_bad = the first one.
// Every accepted strip is checked against the blur itself: the weights a strip's matrices hold for an output column, summed per input
// column, are the 7 taps folded by BORDER_REFLECT_101.
int xplan_blur_sweep(int w_first, int w_last, int* first_bad)
{
    int bad = 0;
    for (int w = w_first; w <= w_last; w++)
        for (int ed = 0; ed < 2; ed++)
            for (int rule = 0; rule < 2; rule++) {
                std::vector<BlurStrip> st;
                std::vector<uint8_t> tabs;
                const int rowbytes = rule == 0 ? w : plan_align_up(w, 64);
                bool ok = plan_blur_level(rule, w, rowbytes, blur_taps(ed != 0), st, tabs) && (int)st.size() == (w + 31) / 32;
                for (size_t k = 0; ok && k < st.size(); k++) {
                    const BlurStrip& S = st[k];
                    const int cs[3] = {S.c0, S.c1, S.c2};
                    const int lo = std::min(S.c0, std::max(0, S.x0 - 3)), span = 96;   // the input columns a strip may touch
                    for (int n = 0; ok && n < 32 && S.x0 + n < w; n++) {
                        int got[span] = {0}, want[span] = {0};
                        for (int piece = 0; piece < 3; piece++)
                            for (int i = 0; i < 16; i++) {
                                const int lane = n + 32 * (piece == 1), ab = piece == 2, x = cs[piece] + i;
                                const int v = (int8_t)tabs[(size_t)S.tab * 1024 + (size_t)ab * 1024 + (size_t)lane * 16 + i];
                                ok = ok && cs[piece] >= 0 && cs[piece] + 16 <= rowbytes && x - lo >= 0 && x - lo < span && (x < w || v == 0);
                                if (ok) got[x - lo] += v;
                            }
                        for (int u = 0; ok && u < 7; u++) {
                            int x = S.x0 + n + u - 3;
                            x = x < 0 ? -x : x >= w ? 2 * (w - 1) - x : x;
                            ok = x - lo >= 0 && x - lo < span;
                            if (ok) want[x - lo] += blur_taps(ed != 0)[u];
                        }
                        ok = ok && !memcmp(got, want, sizeof(got));
                    }
                }
                if (!ok && !bad++) { first_bad[0] = w; first_bad[1] = ed; first_bad[2] = rule; }
            }
    return bad;
}

// plan_input_layout (csrc/input_layout.hpp) as the extractor's plan header carries it: the error code, the reason in msg
int xplan_input_layout(int rows, int cols, unsigned long long step, unsigned long long frame_stride, int nframes, char* msg, int msgcap)
{
    return plan_input_layout(rows, cols, (size_t)step, (size_t)frame_stride, nframes, msg, (size_t)msgcap);
}

// The byte column behind the last one a level-0 load of k_blur7_mfma touches, over all strips of a `cols`-wide level 0 (its three
// 16-byte pieces are planned with rowbytes = cols: level 0 is the caller's buffer, whose rows may end with their last pixel); -1 if
// the tables are refused
int xplan_level0_read_end(int cols, int gaussian_ed)
{
    std::vector<BlurStrip> st;
    std::vector<uint8_t> tabs;
    if (!plan_blur_level(0, cols, cols, blur_taps(gaussian_ed != 0), st, tabs)) return -1;
    int end = 0;
    for (const BlurStrip& S : st) end = std::max(end, std::max(S.c0, std::max(S.c1, S.c2)) + 16);
    return end;
}

} // extern "C"
