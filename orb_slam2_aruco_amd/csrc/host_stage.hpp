// host_stage.hpp -- what the host-pointer entry points of the geometry solvers (initializer.hip, sim3_solver.hip, pose_optimizer.hip,
// orbfe_marker_poses, orbfe_corner_subpix) and of the matcher (match_kernels.hip, bow_vocabulary.hip, keyframe_io.hip) share: the
// layout of one staging block and the workspace that moves it.  Host code only.  IoLayout alone is what the HIP-free plan headers
// take from here: new_points_plan.hpp for its staging block, lba_plan.hpp for the staging block and the scratch of local_ba.hip.
#pragma once
#include <cstddef>

namespace orbfe {

// Offsets of the arrays of one block, each 256-byte aligned, in the order they are taken: [inputs] inout() [in-out] outputs()
// [outputs]; inout() is optional.  The scratch of a solver is a block without outputs(): only take() and end() mean something there.
struct IoLayout {
    size_t off = 0, split = 0, back = (size_t)-1;
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }
    void inout() { back = off; }      // what is taken from here to outputs() goes up and comes back (flags a kernel updates, a word it counts in)
    void outputs() { split = off; }   // what was taken so far goes up, what is taken from here on comes down
    size_t down() const { return back < split ? back : split; }
    size_t end() const { return off; }   // upload range [0, split), download range [down(), end())
};

} // namespace orbfe

#ifdef __HIPCC__
#include "orbfe_common.hpp"
#include <cstring>
#include <vector>

namespace orbfe {

// The workspace of a host-pointer call, one per (thread, device) through ThreadWorkspaces: the call stages its inputs in `pinned`,
// sends them to `io` in ONE copy, runs its kernels on `stream`, fetches the outputs in ONE copy and synchronises once.
struct HostStage {
    // the RANSAC solvers: the batch entry point runs on the caller's stream, the host entry points on `stream`.  Each has scratch of
    // its own, so that a host call never overwrites the scratch of a batch still running on the caller's stream of the same thread
    DevBuf scratch, host_scratch, io;
    PinnedBuf pinned;
    hipStream_t stream = nullptr;   // not the null stream: that one synchronises with every blocking stream of the process
    IoLayout lay;
    ~HostStage() { if (stream) (void)hipStreamDestroy(stream); }
    int begin(const IoLayout& l)
    {
        lay = l;
        int rc;
        if ((rc = io.ensure(l.end())) || (rc = pinned.ensure(l.end()))) return rc;
        if (!stream) ORBFE_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return ORBFE_OK;
    }
    template <class T> T* dev(size_t o) const { return (T*)(io.as<uint8_t>() + o); }
    template <class T> T* host(size_t o) const { return (T*)(pinned.as<uint8_t>() + o); }
    // a host array that is absent (NULL) or empty is not copied, in either direction
    void put(size_t o, const void* src, size_t bytes) { if (src && bytes) memcpy(host<uint8_t>(o), src, bytes); }
    void get(void* dst, size_t o, size_t bytes) const { if (dst && bytes) memcpy(dst, host<uint8_t>(o), bytes); }
    int upload() { ORBFE_HIP(hipMemcpyAsync(io.p, pinned.p, lay.split, hipMemcpyHostToDevice, stream)); return ORBFE_OK; }
    int download()
    {
        const size_t b = lay.down();
        ORBFE_HIP(hipMemcpyAsync(host<uint8_t>(b), dev<uint8_t>(b), lay.end() - b, hipMemcpyDeviceToHost, stream));
        return ORBFE_OK;
    }
    int sync() { ORBFE_HIP(hipStreamSynchronize(stream)); return ORBFE_OK; }
};

// A plan's tables on their way to the device (essential_graph.hip, global_ba.hip), one page-locked block per (thread, device,
// stream).  A call overwrites the block of the call before it on the same stream, so it first waits until that call's copy has left
// the block (an event behind the copy).
struct TablesStage {
    PinnedBuf pinned;
    hipEvent_t ev = nullptr;
    bool pending = false;
    ~TablesStage() { if (ev) (void)hipEventDestroy(ev); }
    int send(const std::vector<unsigned char>& blob, void* dst, hipStream_t s)
    {
        if (pending) ORBFE_HIP(hipEventSynchronize(ev));
        if (!ev) ORBFE_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        const int rc = pinned.ensure(blob.size());
        if (rc) return rc;
        memcpy(pinned.p, blob.data(), blob.size());
        ORBFE_HIP(hipMemcpyAsync(dst, pinned.p, blob.size(), hipMemcpyHostToDevice, s));
        ORBFE_HIP(hipEventRecord(ev, s));
        pending = true;
        return ORBFE_OK;
    }
};

// The stage of the matcher's host-pointer calls, one per (thread, device): defined in match_kernels.hip, shared with
// bow_vocabulary.hip and keyframe_io.hip.  The caller has selected the device already.
HostStage& match_host_stage();

} // namespace orbfe
#endif
