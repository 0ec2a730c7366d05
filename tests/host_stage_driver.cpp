// C entry point over the IoLayout of csrc/host_stage.hpp for tests/test_host_stage_cpu.py (built with g++ by
// tests/host_stage_build.py: that half of the header has no HIP in it).  Test infrastructure only.
#include "../orb_slam2_aruco_amd/csrc/host_stage.hpp"

extern "C" {

// Takes in[0 .. n_in) as the inputs, io[0 .. n_io) as the arrays that travel both ways (n_io < 0: inout() is not called) and
// out[0 .. n_out) as the outputs of one layout.  offsets: the offsets take() returned, in order; ranges: upload begin, upload end,
// download begin, download end.
void iolayout_run(const long long* in, int n_in, const long long* io, int n_io, const long long* out, int n_out, long long* offsets,
                  long long* ranges)
{
    orbfe::IoLayout l;
    for (int i = 0; i < n_in; i++) *offsets++ = (long long)l.take((size_t)in[i]);
    if (n_io >= 0) l.inout();
    for (int i = 0; i < n_io; i++) *offsets++ = (long long)l.take((size_t)io[i]);
    l.outputs();
    for (int i = 0; i < n_out; i++) *offsets++ = (long long)l.take((size_t)out[i]);
    ranges[0] = 0;
    ranges[1] = (long long)l.split;
    ranges[2] = (long long)l.down();
    ranges[3] = (long long)l.end();
}

} // extern "C"
