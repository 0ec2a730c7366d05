// input_layout.hpp -- which layouts of a caller's device frames the image kernels can address.  Pure host arithmetic, no HIP: the three
// entry points that read pyramid level 0 from the caller's buffer (orbfe_extract_batch_device, orbfe_aruco_detect_batch_device,
// orbfe_pipeline_step) ask plan_input_layout() before they enqueue anything, tests/test_input_layout_cpu.py compiles it with g++ through
// both plan headers.
//
// The kernels place no condition on alignment: the base may sit at any byte and the row step may be any value >= cols (every load of
// level 0 is declared unaligned, or chosen by the host from the alignment it finds: the detector's pyramid()).  What bounds a layout is
// their offset arithmetic, row * step + column off a frame's first byte (frames are 64-bit: base + frame * frame_stride):
//   * row * step is a 24-bit multiply (__mul24: off24() in orb_kernels.hip -- k_resize_tab, k_blur7_mfma, k_orient_describe2, the ROI
//     staging of k_fast_cells; k_threshold_pyr, k_threshold_mfma in aruco_kernels.hip).  It sign-extends bit 23 of both operands, so
//     the step has to be below 2^23; the row is (rows <= 8000).
//   * the product and the column are added in 32 bits (int, then read as uint32_t) and carried to the pointer as one 32-bit lane offset.
//     The largest offset a kernel forms is the last row's, (rows - 1) * step, plus a column below cols; a load reaches at most 16 bytes
//     further.  With the frame's span (rows - 1) * step + cols below 2^31 no signed sum overflows, and the unsigned ones stay far
//     below 2^32.
//   * the kernels that multiply in 64 bits (k_half_area*, k_half_pyr, k_resize_level, k_resize_nearest, the decoders, the sub-pixel
//     pass) hold the step as int (ImgView::pitch): below 2^23 it is.
// A frame has to hold its last row's pixels: frame_stride >= (rows - 1) * step + cols wherever a second frame follows.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cstdio>

#include "../../include/orbfe.h"

namespace orbfe {

constexpr size_t kMaxInputStep = (size_t)1 << 23;         // exclusive
constexpr uint64_t kMaxInputFrameSpan = (uint64_t)1 << 31; // exclusive: (rows - 1) * step + cols

// ORBFE_OK, or ORBFE_ERR_INVALID with the reason in msg (may be null)
inline int plan_input_layout(int rows, int cols, size_t step, size_t frame_stride, int nframes, char* msg, size_t msgcap)
{
    // what: the quantity that is out of bounds, is: its value, rule: the bound it misses
    auto refuse = [&](const char* what, unsigned long long is, const char* rule, unsigned long long bound) {
        if (msg && msgcap) snprintf(msg, msgcap, "input layout: %s %llu %s %llu", what, is, rule, bound);
        return ORBFE_ERR_INVALID;
    };
    if (rows <= 0 || cols <= 0 || nframes <= 0) {
        if (msg && msgcap) snprintf(msg, msgcap, "input layout: no frame (%d frames of %d rows, %d columns)", nframes, rows, cols);
        return ORBFE_ERR_INVALID;
    }
    if (step < (size_t)cols) return refuse("row step", step, "is less than the columns,", (unsigned long long)cols);
    if (step >= kMaxInputStep) return refuse("row step", step, "is not below the limit of the 24-bit row offsets,", kMaxInputStep);
    const uint64_t span = (uint64_t)(rows - 1) * step + (uint64_t)cols;   // (rows < 2^31, step < 2^23: no overflow)
    if (span >= kMaxInputFrameSpan) return refuse("bytes a frame spans,", span, "are not below the limit of the 32-bit offsets inside a frame,", kMaxInputFrameSpan);
    if (nframes > 1 && frame_stride < span) return refuse("frame stride", frame_stride, "is less than the bytes a frame spans,", span);
    return ORBFE_OK;
}

} // namespace orbfe
