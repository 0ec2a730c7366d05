// C entry points over the blurred pyramid's tiled layout (csrc/extractor_plan.hpp: blur_tile_off, blur_pixel_off, LevelGeom::btrow /
// blur_off, blur_fbytes) for tests/test_blur_layout_cpu.py and tests/test_blur_tiles_gpu.py; built with g++ by
// tests/blur_layout_build.py.  With -DBLUR_LAYOUT_MAIN it is a program of its own (for a sanitizer build): it plans the three bench
// geometries, fills every level of a frame block through the address function and reads it back.  Test infrastructure only.
#include <cstring>

#include "../orb_slam2_aruco_amd/csrc/extractor_plan.hpp"

using namespace orbfe;

// the ORB-SLAM2 constructor's tables (ORBextractor.cc:410-446) for a scale factor of 1.2: what plan_extractor is given
static ExtractorPlan plan_for(int rows, int cols, int nfeatures, int nlevels)
{
    std::vector<float> sc((size_t)nlevels), inv((size_t)nlevels);
    std::vector<int> quota((size_t)nlevels);
    sc[0] = 1.f;
    for (int l = 1; l < nlevels; l++) sc[(size_t)l] = sc[(size_t)l - 1] * 1.2f;
    for (int l = 0; l < nlevels; l++) inv[(size_t)l] = 1.f / sc[(size_t)l];
    const float factor = 1.f / 1.2f;
    float per = nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int l = 0; l < nlevels - 1; l++) {
        quota[(size_t)l] = orbfe_round_f(per);
        sum += quota[(size_t)l];
        per *= factor;
    }
    quota[(size_t)nlevels - 1] = std::max(nfeatures - sum, 0);
    return plan_extractor(rows, cols, nlevels, sc.data(), inv.data(), quota.data(), false);
}

// the most bytes a load of k_orient_describe2 reads from a pixel's offset on: one 16-byte chunk
static const long long OVER_READ = 16;

// Checks the layout of a rows x cols plan.  Returns 0, or the number of the first check that fails:
//   1 the plan is refused     2 a level is not a whole number of 128-byte tiles, or its offset is not line-aligned
//   3 two pixels (of one level or of two) share an offset     4 an offset + OVER_READ passes blur_fbytes
//   5 the 16 bytes of a chunk-aligned column are not contiguous     6 a level's pixels leave its own tiles
static int check_layout(const ExtractorPlan& p)
{
    if (p.err) return 1;
    std::vector<uint8_t> seen(p.blur_fbytes, 0);
    for (size_t l = 0; l < p.geom.size(); l++) {
        const LevelGeom& g = p.geom[l];
        const long long bytes = (long long)g.btrow * blur_tiles_y(g.h);
        if (g.btrow != blur_tiles_x(g.w) * 128 || g.blur_off % 128 || bytes % 128) return 2;
        for (int y = 0; y < g.h; y++)
            for (int x = 0; x < g.w; x++) {
                const long long o = blur_pixel_off(g, x, y);
                if (o < g.blur_off || o >= g.blur_off + bytes) return 6;
                if (o + OVER_READ > (long long)p.blur_fbytes) return 4;
                if (seen[(size_t)o]++) return 3;
                if (x % 16 == 0)
                    for (int k = 1; k < 16 && x + k < g.w; k++)
                        if (blur_pixel_off(g, x + k, y) != o + k) return 5;
            }
    }
    return 0;
}

extern "C" {

int blur_layout_check(int rows, int cols, int nfeatures, int nlevels) { return check_layout(plan_for(rows, cols, nfeatures, nlevels)); }

void blur_layout_tile(int* tw, int* th) { *tw = BLUR_TW; *th = BLUR_TH; }

// fills every level of a frame's blurred block with a function of (level, x, y) through the address function, reads it back the same
// way (what orbfe_extractor_debug_level_image does with a level's tiles); returns the number of pixels that differ, -1: no plan
long long blur_layout_roundtrip(int rows, int cols, int nfeatures, int nlevels)
{
    const ExtractorPlan p = plan_for(rows, cols, nfeatures, nlevels);
    if (p.err) return -1;
    std::vector<uint8_t> block(p.blur_fbytes, 0);
    auto val = [](size_t l, int x, int y) { return (uint8_t)(x * 7 + y * 13 + (int)l * 29 + 1); };
    for (size_t l = 0; l < p.geom.size(); l++)
        for (int y = 0; y < p.geom[l].h; y++)
            for (int x = 0; x < p.geom[l].w; x++) block[(size_t)blur_pixel_off(p.geom[l], x, y)] = val(l, x, y);
    long long bad = 0;
    for (size_t l = 0; l < p.geom.size(); l++) {
        const LevelGeom& g = p.geom[l];
        std::vector<uint8_t> tiles(block.begin() + g.blur_off, block.begin() + g.blur_off + (long long)g.btrow * blur_tiles_y(g.h));
        std::vector<uint8_t> out((size_t)g.w * g.h);
        for (int y = 0; y < g.h; y++)
            for (int x = 0; x < g.w; x++) out[(size_t)y * g.w + x] = tiles[blur_tile_off(g.btrow, x, y)];
        for (int y = 0; y < g.h; y++)
            for (int x = 0; x < g.w; x++) bad += out[(size_t)y * g.w + x] != val(l, x, y);
    }
    return bad;
}

} // extern "C"

#ifdef BLUR_LAYOUT_MAIN
int main()
{
    const int cases[3][4] = {{480, 640, 1000, 8}, {720, 1280, 2000, 8}, {1080, 1920, 4000, 12}};
    for (const auto& c : cases) {
        const int rc = blur_layout_check(c[0], c[1], c[2], c[3]);
        const long long bad = blur_layout_roundtrip(c[0], c[1], c[2], c[3]);
        printf("%dx%d / %d levels: check %d, %lld pixels differ\n", c[1], c[0], c[3], rc, bad);
        if (rc || bad) return 1;
    }
    return 0;
}
#endif
