// C entry points over csrc/pipeline_plan.hpp for tests/test_pipeline_plan_cpu.py (built with g++ by tests/pipeline_plan_build.py:
// the header has no HIP in it).  Test infrastructure only.
#include <cstring>

#include "../orb_slam2_aruco_amd/csrc/pipeline_plan.hpp"

using namespace orbfe;

// An environment that is a table: `n` (name, value) pairs.  Every name plan_schedule asks for is appended to `asked` ("NAME;"), set
// or not.  (It takes a plain function pointer, so the table of the call in progress is file-static.)
static const char* const* g_names = nullptr;
static const char* const* g_values = nullptr;
static int g_n = 0, g_asked_cap = 0;
static char* g_asked = nullptr;
static const char* table_lookup(const char* name)
{
    if (g_asked && strlen(g_asked) + strlen(name) + 2 <= (size_t)g_asked_cap) { strcat(g_asked, name); strcat(g_asked, ";"); }
    for (int i = 0; i < g_n; i++)
        if (!strcmp(g_names[i], name)) return g_values[i];
    return nullptr;
}

extern "C" {

// cfg: engine_sets, record_sets, phase_pin, det_pin, defer_post, det_nofork;  out: D, R, phase_pin, det_pin, defer_post, det_nofork,
// describe_late, gather_stream
void pplan_schedule(int rows, int cols, int use_orb, const int* cfg, const char* const* names, const char* const* values, int n, int* out,
                    char* asked, int asked_cap)
{
    g_names = names; g_values = values; g_n = n; g_asked = asked; g_asked_cap = asked_cap;
    if (asked && asked_cap > 0) asked[0] = 0;
    const Schedule s = plan_schedule(rows, cols, use_orb != 0, ScheduleConfig{cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], cfg[5]}, table_lookup);
    g_names = g_values = nullptr; g_n = 0; g_asked = nullptr;
    const int v[8] = {s.D, s.R, s.phase_pin, s.det_pin, s.defer_post, s.det_nofork, s.describe_late, s.gather_stream};
    memcpy(out, v, sizeof(v));
}

const char* pplan_env_defaults() { return pipeline_env_defaults(); }

} // extern "C"
