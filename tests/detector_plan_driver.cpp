// C entry points over csrc/detector_plan.hpp for tests/test_detector_plan_cpu.py (built with g++ by tests/detector_plan_build.py:
// the header has no HIP in it).  Test infrastructure only.
#include <cmath>
#include <cstring>

#include "../orb_slam2_aruco_amd/csrc/detector_plan.hpp"

using namespace orbfe;

extern "C" {

// The geometry of a rows x cols working image whose pyramid starts from prows x pcols.  scalars: win, wpr, npyr, lds_bits_words,
// relay_tbits, relay_kshift, relay_global, relay_kcap, ct_segcap, ct_hbits, ct_lcap, ct_items_per_frame; sizes: bits_fu32, pyr_fbytes,
// candq_fu32, pool_fu32, gpad_fu32; levels: (w, h, pitch, exact) per level, at most maxlevels.  Returns the plan's error code; msg
// receives its message.
int dplan_make(int rows, int cols, int prows, int pcols, int S, int specks_inkernel, int lcap_override, long long rl_static, int* scalars,
               long long* sizes, int* levels, int maxlevels, char* msg, int msgcap)
{
    const DetectorGeometry g = plan_detector(rows, cols, prows, pcols, S, specks_inkernel != 0, lcap_override, (size_t)rl_static);
    snprintf(msg, (size_t)msgcap, "%s", g.msg);
    if (g.err) return g.err;
    const int s[12] = {g.win, g.wpr, g.npyr, g.lds_bits_words, g.relay_tbits, g.relay_kshift, g.relay_global, g.relay_kcap,
                       g.ct_segcap, g.ct_hbits, g.ct_lcap, g.ct_items_per_frame};
    memcpy(scalars, s, sizeof(s));
    const long long z[5] = {(long long)g.bits_fu32, (long long)g.pyr_fbytes, (long long)g.candq_fu32, (long long)g.pool_fu32, (long long)g.gpad_fu32};
    memcpy(sizes, z, sizeof(z));
    if (g.npyr != (int)g.levels.size() || g.npyr != (int)g.lvl_exact.size() || g.npyr > maxlevels) return -100;
    for (int l = 0; l < g.npyr; l++) {
        const ArLevel& L = g.levels[(size_t)l];
        // a level's rows lie inside the frame's pyramid block, behind the level before
        if (l > 0 && (L.pitch < L.w || L.off < 0 || (size_t)L.off + (size_t)L.pitch * L.h > g.pyr_fbytes)) return -101;
        if (l > 1 && L.off < g.levels[(size_t)l - 1].off + (long long)g.levels[(size_t)l - 1].pitch * g.levels[(size_t)l - 1].h) return -101;
        const int v[4] = {L.w, L.h, L.pitch, g.lvl_exact[(size_t)l]};
        memcpy(levels + 4 * l, v, sizeof(v));
    }
    return ORBFE_OK;
}

// The box mean of the threshold kernels for a window of n pixels: for how many box sums s = 0 .. 255 n the integer mean
// (s + n / 2) / n, or its multiply-shift form (s + n / 2) * ceil(2^32 / n) >> 32, is not the reference's rint(s * (1.0 / n))
int dplan_mean_mismatches(int n)
{
    const uint32_t magic = (uint32_t)((0x100000000ull + (unsigned)n - 1) / (unsigned)n);
    int bad = 0;
    for (int s = 0; s <= 255 * n; s++) {
        const int want = (int)std::rint((double)s * (1.0 / n));
        bad += (int)(((unsigned long long)(s + n / 2) * magic) >> 32) != want || (s + n / 2) / n != want;
    }
    return bad;
}

// plan_threshold_tables for every width w_first .. w_last at window `win`.  Returns how many widths the matrix-core tables refuse
// or get wrong; first_bad = the first one.  Every accepted strip is checked against the box filter itself: the weights its pass-1 box
// matrices hold for an output column, summed per input column, are the `win` taps folded by BORDER_REPLICATE, its selection
// matrices pick the column itself, and every 16-byte piece it loads lies inside the row.  (A strip whose windows stay clear of both
// image borders and whose pieces lie where the last such strip's lay, relative to its first column, is compared with that one's
// matrices byte by byte instead: the same weights at the same places.)
int dplan_threshold_sweep(int w_first, int w_last, int win, int* first_bad)
{
    int bad = 0;
    const int R = win / 2;
    for (int w = w_first; w <= w_last; w++) {
        const ThresholdTables t = plan_threshold_tables(w, win);
        bool ok = t.ok && t.cols == w && t.win == win && (int)t.strips.size() == (w + 31) / 32 && t.tabs.size() == t.strips.size() * 4096 &&
                  t.tab2.size() == 6144 && t.rb == (R <= 3 ? 4 : 8);
        const ThrStrip* ref = nullptr;   // the last interior strip that went through the full check
        for (size_t k = 0; ok && k < t.strips.size(); k++) {
            const ThrStrip& S = t.strips[k];
            const int cs[3] = {S.c0, S.c1, S.c2};
            ok = S.x0 == (int)k * 32 && S.tab == (int)k * 4;
            const bool interior = S.x0 - R >= 0 && S.x0 + 31 + R <= w - 1;
            if (ok && interior && ref && S.c0 - S.x0 == ref->c0 - ref->x0 && S.c1 - S.x0 == ref->c1 - ref->x0 && S.c2 - S.x0 == ref->c2 - ref->x0) {
                ok = !memcmp(&t.tabs[(size_t)S.tab * 1024], &t.tabs[(size_t)ref->tab * 1024], 4096);
                continue;
            }
            const int lo = std::min(S.c0, std::max(0, S.x0 - R)), span = 64;   // the input columns a strip may touch
            for (int n = 0; ok && n < 32; n++) {
                int8_t box[span] = {0}, sel[span] = {0}, wbox[span] = {0}, wsel[span] = {0};
                for (int piece = 0; piece < 3; piece++)
                    for (int i = 0; i < 16; i++) {
                        const int lane = n + 32 * (piece == 1), ab = piece == 2, x = cs[piece] + i;
                        const uint8_t* m = &t.tabs[(size_t)S.tab * 1024 + (size_t)ab * 1024 + (size_t)lane * 16 + i];
                        ok = ok && cs[piece] >= 0 && cs[piece] + 16 <= w && x - lo >= 0 && x - lo < span;
                        if (ok) { box[x - lo] += (int8_t)m[0]; sel[x - lo] += (int8_t)m[2048]; }
                    }
                // (matrix b's lanes 32 .. 63 have no piece: they stay zero)
                for (int i = 0; ok && i < 16; i++)
                    ok = !t.tabs[(size_t)S.tab * 1024 + 1024 + (size_t)(n + 32) * 16 + i] && !t.tabs[(size_t)S.tab * 1024 + 3072 + (size_t)(n + 32) * 16 + i];
                if (S.x0 + n < w) {
                    for (int u = -R; ok && u <= R; u++) {
                        const int x = std::min(std::max(S.x0 + n + u, 0), w - 1);
                        ok = x - lo >= 0 && x - lo < span;
                        if (ok) wbox[x - lo] += 1;
                    }
                    if (ok) wsel[S.x0 + n - lo] = 1;
                }
                ok = ok && !memcmp(box, wbox, sizeof(box)) && !memcmp(sel, wsel, sizeof(sel));
            }
            if (ok && interior) ref = &S;
        }
        if (!ok && !bad++) *first_bad = w;
    }
    return bad;
}

// 1 if plan_threshold_tables(cols, win) says "not applicable"
int dplan_threshold_refused(int cols, int win) { return plan_threshold_tables(cols, win).ok ? 0 : 1; }

// plan_input_layout (csrc/input_layout.hpp) as the detector's plan header carries it: the error code, the reason in msg
int dplan_input_layout(int rows, int cols, unsigned long long step, unsigned long long frame_stride, int nframes, char* msg, int msgcap)
{
    return plan_input_layout(rows, cols, (size_t)step, (size_t)frame_stride, nframes, msg, (size_t)msgcap);
}

// The byte column behind the last one a load of k_threshold_mfma touches, over all strips of a `cols`-wide frame (the caller's rows may
// end with their last pixel); -1 if the tables do not apply
int dplan_threshold_read_end(int cols, int win)
{
    const ThresholdTables t = plan_threshold_tables(cols, win);
    if (!t.ok) return -1;
    int end = 0;
    for (const ThrStrip& S : t.strips) end = std::max(end, std::max(S.c0, std::max(S.c1, S.c2)) + 16);
    return end;
}

// plan_pyramid_kernels for the geometry of a rows x cols frame (pyramid from the frame itself) whose level 0 lies at an address with
// the low bits src_align, rows src_pitch and frames src_fstride apart: out[p] = the PyrKernel of level p (0: none).  Returns the
// number of levels, or the plan's error code.
int dplan_pyramid_kernels(int rows, int cols, int S, int first, int src_align, int src_pitch, unsigned long long src_fstride, int half_pyr, int* out, int maxlevels)
{
    const DetectorGeometry g = plan_detector(rows, cols, rows, cols, S, false, 0, 4352);
    if (g.err) return g.err;
    if (g.npyr > maxlevels) return -100;
    const std::vector<PyrKernel> k = plan_pyramid_kernels(g, first, (unsigned)src_align, src_pitch, (size_t)src_fstride, half_pyr != 0);
    for (int p = 0; p < g.npyr; p++) out[p] = (int)k[(size_t)p];
    return g.npyr;
}

// ---- the switches, the environment reader and the batch plan

// DetectorSwitches as 16 ints, in the order of detector_plan_build.SWITCH_FIELDS
static void switches_out(const DetectorSwitches& w, int* o)
{
    const int v[16] = {w.tiled, w.banded, w.band_rows, w.tile_w, w.tpw, w.lcap, w.specks, w.specks_inkernel, w.relay_wide, w.small_separate,
                       w.thr_mfma, w.thr_mfma_auto, w.thr_pyr, w.half_pyr, w.force_legacy, w.big_mode};
    memcpy(o, v, sizeof(v));
}
static DetectorSwitches switches_in(const int* v)
{
    DetectorSwitches w;
    w.tiled = v[0]; w.banded = v[1]; w.band_rows = v[2]; w.tile_w = v[3]; w.tpw = v[4]; w.lcap = v[5]; w.specks = v[6]; w.specks_inkernel = v[7] != 0;
    w.relay_wide = v[8] != 0; w.small_separate = v[9]; w.thr_mfma = v[10] != 0; w.thr_mfma_auto = v[11] != 0; w.thr_pyr = v[12] != 0;
    w.half_pyr = v[13] != 0; w.force_legacy = v[14] != 0; w.big_mode = v[15] != 0;
    return w;
}

// An environment that is a table: `n` (name, value) pairs.  Every name a reader asks for is appended to `asked` ("NAME;"), set or not.
// (The readers take a plain function pointer, so the table of the call in progress is file-static.)
static const char* const* g_env_names = nullptr;
static const char* const* g_env_values = nullptr;
static int g_env_n = 0, g_asked_cap = 0;
static char* g_asked = nullptr;
static const char* table_lookup(const char* name)
{
    if (g_asked && strlen(g_asked) + strlen(name) + 2 <= (size_t)g_asked_cap) { strcat(g_asked, name); strcat(g_asked, ";"); }
    for (int i = 0; i < g_env_n; i++)
        if (!strcmp(g_env_names[i], name)) return g_env_values[i];
    return nullptr;
}
static void table_set(const char* const* names, const char* const* values, int n, char* asked, int asked_cap)
{
    g_env_names = names; g_env_values = values; g_env_n = n; g_asked = asked; g_asked_cap = asked_cap;
    if (asked && asked_cap > 0) asked[0] = 0;
}

// the defaults (no environment at all), and read_detector_env over a table on top of them
void dplan_switch_defaults(int* out) { switches_out(DetectorSwitches{}, out); }
void dplan_read_env(const char* const* names, const char* const* values, int n, int* out, char* asked, int asked_cap)
{
    DetectorSwitches w;
    table_set(names, values, n, asked, asked_cap);
    read_detector_env(w, table_lookup);
    table_set(nullptr, nullptr, 0, nullptr, 0);
    switches_out(w, out);
}

// plan_batch for B frames of a rows x cols working image (pyramid from prows x pcols; specks_inkernel and lcap go into the geometry as
// the handle passes them).  out: thr, thr_kk, nfuse, specks, contours, band, band_rows, tile_w, tpw, relay, small_separate, walker_hbm.
// Returns the geometry's error code.
int dplan_batch(int rows, int cols, int prows, int pcols, int S, long long rl_static, int B, int adaptive, int reduced, int thres_value, int floor,
                const int* switches, long long* out)
{
    const DetectorSwitches w = switches_in(switches);
    const DetectorGeometry g = plan_detector(rows, cols, prows, pcols, S, w.specks_inkernel, w.lcap, (size_t)rl_static);
    if (g.err) return g.err;
    BatchMode m;
    m.adaptive = adaptive != 0; m.reduced = reduced != 0; m.thres_value = thres_value;
    const BatchPlan p = plan_batch(g, B, m, (Contours)floor, w);
    const long long v[12] = {(int)p.thr, (long long)p.thr_kk, p.nfuse, p.specks, (int)p.contours, p.band, p.band_rows, p.tile_w, p.tpw, (int)p.relay,
                             p.small_separate, p.walker_hbm};
    memcpy(out, v, sizeof(v));
    return ORBFE_OK;
}

// Whether a batch gets the speck launch when it is forced on ("speck_passes" = 1) and the frame is `cols` wide: the geometry of a
// 480 x 640 frame with its width replaced, because plan_detector admits no frame wide enough for the tile not to fit
int dplan_forced_speck_launch(int cols, int B)
{
    DetectorGeometry g = plan_detector(480, 640, 480, 640, 35, false, 0, 4352);
    g.cols = cols;
    DetectorSwitches w;
    w.specks = 1;
    return plan_batch(g, B, BatchMode{}, Contours::tiled, w).specks;
}

int dplan_escalate(int ran, int flags_or, int relay_ok) { return (int)escalate((Contours)ran, flags_or, relay_ok != 0); }

// 1 where threshold_tables_apply(cols, win) and plan_threshold_tables(cols, win).ok disagree
int dplan_threshold_predicate_differs(int cols, int win) { return threshold_tables_apply(cols, win) != plan_threshold_tables(cols, win).ok; }

} // extern "C"
