// ransac_sets.hpp -- the device helpers the RANSAC drivers share (initializer.hip: sets of 8 indices, sim3_solver.hip: of 3).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace orbfe {

// a frame's keypoint count as the kernels use it: a count outside 0 .. capacity (a device entry point cannot check it) is clamped
__device__ __forceinline__ int clampn(int n, int cap) { return n < 0 ? 0 : n > cap ? cap : n; }

// One minimal set as the reference draws it (Initializer.cc:80-97, Sim3Solver.cc:163-177): for j = 0 .. K-1,
// RandomInt(0, size - 1) on the caller's rand() word w[j] with size = N - j, the index taken from the list of available indices
// (initially 0 .. N-1) and replaced there by the list's last entry.  N >= K.  Only the positions of the list that differ from the
// identity are kept (at most K), so a set costs no memory of size N.
template <int K>
__device__ __forceinline__ void decode_set(const int32_t* w, int N, int32_t* out)
{
    int pos[K], val[K], nov = 0;
    for (int j = 0; j < K; j++) {
        const int size = N - j;
        // rand() returns 0 .. RAND_MAX; a word outside that range (a device entry point cannot check it) is clamped, so that
        // every index stays inside the list
        int randi = (int)(((double)w[j] / ((double)2147483647 + 1.0)) * size);
        randi = randi < 0 ? 0 : randi >= size ? size - 1 : randi;
        int idx = randi, back = size - 1;
        for (int q = 0; q < nov; q++) { if (pos[q] == randi) idx = val[q]; }
        for (int q = 0; q < nov; q++) { if (pos[q] == size - 1) back = val[q]; }
        out[j] = idx;
        int q = 0;
        while (q < nov && pos[q] != randi) q++;
        pos[q] = randi; val[q] = back;
        if (q == nov) nov++;
    }
}

} // namespace orbfe
