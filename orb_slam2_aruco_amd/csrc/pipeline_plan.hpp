// pipeline_plan.hpp -- the batched pipeline's schedule: how many extractor and record sets, which locks between the engines, what
// runs a step late.  Pure host arithmetic of the frame size, the configuration and the environment, no HIP:
// orbfe_pipeline_create (csrc/pipeline.hip) calls plan_schedule once and then only creates resources,
// tests/test_pipeline_plan_cpu.py compiles this header with g++ and pins the defaults and their interactions.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <cstdlib>

namespace orbfe {

typedef const char* (*EnvLookup)(const char* name);   // getenv, or a test's table

// One list for the pipeline and the engines: bench.py marks a line as diagnostic when one of these is set to something else.
// Every ORBFE_* variable plan_schedule and read_detector_env (detector_plan.hpp) look up is here, and nothing else but
// ORBFE_RCCL_LIB, which pipeline.hip reads where it binds the library (tests/test_pipeline_plan_cpu.py holds both directions).
inline const char* pipeline_env_defaults()
{
    return "ORBFE_ENGINE_SETS=2;ORBFE_RECORD_SETS=4;ORBFE_PHASE_PIN=size;ORBFE_DET_PIN=4;ORBFE_DEFER_POST=size;ORBFE_DET_NOFORK=size;"
           "ORBFE_ARUCO_RELAY_WIDE=1;"
           "ORBFE_ARUCO_SPECKS=size;ORBFE_DESCRIBE_LATE=1;ORBFE_ARUCO_SMALL_SEPARATE=size;ORBFE_ARUCO_TILED=size;ORBFE_ARUCO_TILE_W=0;ORBFE_ARUCO_TPW=0;ORBFE_ARUCO_BANDED=size;ORBFE_ARUCO_BAND_ROWS=0;ORBFE_ARUCO_LCAP=0;"
           "ORBFE_GATHER_STREAM=0;ORBFE_RCCL_LIB=";
}

// the six fields of orbfe_pipeline_config that steer the schedule (include/orbfe.h): -1 = the default by frame size
struct ScheduleConfig {
    int engine_sets = -1, record_sets = -1, phase_pin = -1, det_pin = -1, defer_post = -1, det_nofork = -1;
};

struct Schedule {
    int D = 0, R = 0;              // extractor sets, record sets
    int phase_pin = 0, det_pin = 0;   // the locks: extractor set on extractor set, detector on extractor (orbfe_extractor_follow's stages)
    bool defer_post = false, det_nofork = false;
    bool describe_late = false;    // a batch's descriptor kernel one step late, behind the next batch's resize chain
    bool gather_stream = false;    // the gather on a low-priority stream of its own
};

// an empty variable counts as unset
inline int env_or(EnvLookup env, const char* name, int v) { const char* e = env(name); return e && *e ? atoi(e) : v; }

// Defaults by frame size, each overridable by the configuration and, for measurements, by the environment (env over configuration
// over size default).
inline Schedule plan_schedule(int rows, int cols, bool use_orb, const ScheduleConfig& cfg, EnvLookup env)
{
    Schedule s;
    const bool vga = (size_t)rows * cols <= (size_t)640 * 480;
    auto pick = [&](int cfgv, const char* name, int dflt) { return env_or(env, name, cfgv >= 0 ? cfgv : dflt); };
    // two extractor sets (1.4955 against 1.5288 ms per C2 step in round 3; 1920 x 1080 lost then, 4.84 -> 5.00, while its contour
    // stage held whole CUs -- with the banded contour kernels it gains: 3.58 against 3.64 ms, three interleaved runs each)
    s.D = std::max(1, pick(cfg.engine_sets, "ORBFE_ENGINE_SETS", 2));
    if (!use_orb) s.D = 1;
    s.R = std::max(2, pick(cfg.record_sets, "ORBFE_RECORD_SETS", 4));
    // the extractor sets' lock: behind the other set's quadtree up to 1280 x 720; behind its FAST above (1920 x 1080 with the banded contour
    // kernels, four runs each: 3.15 - 3.19 ms per step, no lock at all 3.16 - 3.18, behind the quadtree 3.33 - 3.37, tools/r04_pins35b.sh)
    const bool above_720p = (size_t)rows * cols > (size_t)1280 * 720;
    s.phase_pin = pick(cfg.phase_pin, "ORBFE_PHASE_PIN", above_720p ? 1 : 2);
    s.det_pin = pick(cfg.det_pin, "ORBFE_DET_PIN", 4);
    s.defer_post = pick(cfg.defer_post, "ORBFE_DEFER_POST", vga ? 1 : 0) != 0;
    s.det_nofork = pick(cfg.det_nofork, "ORBFE_DET_NOFORK", vga ? 1 : 0) != 0;
    s.gather_stream = env_or(env, "ORBFE_GATHER_STREAM", 0) != 0;
    // A batch's descriptor kernel one step late, behind the NEXT batch's resize chain (round 6).  Both live on the CU's vector memory
    // path -- unaligned 8- and 16-byte lane loads -- and next to each other the resize chain, which is on the step's critical chain,
    // took 400 - 450 us (200 alone); next to FAST, which is VALU-bound, the descriptors cost less than they gave back at 640 x 480:
    // 1.308 against 1.338 ms per C2 step (twelve interleaved runs each; resize 294 - 336 us, FAST 810 - 890 instead of 610 - 690).
    // With the blur on the matrix cores (k_blur7_mfma) FAST has the vector ALUs more to itself and every size gains: C2 1.265
    // against 1.327, 1280 x 720 3.70 against 3.74, 1920 x 1080 3.13 against 3.21 ms.
    // A lock on stage 3 -- the descriptors of a batch -- would be circular with it: the descriptors of batch i - 1 wait for the
    // resize chain of batch i.  Such a lock turns it off.
    // It forces defer_post, an explicit defer_post = 0 of the configuration or the environment included (include/orbfe.h says so).
    const bool stage3_lock = s.phase_pin % 10 == 3 || s.phase_pin / 10 == 3 || s.det_pin % 10 == 3;
    s.describe_late = use_orb && env_or(env, "ORBFE_DESCRIBE_LATE", 1) != 0 && s.D > 1 && !stage3_lock;
    if (s.describe_late) s.defer_post = true;
    return s;
}

} // namespace orbfe
