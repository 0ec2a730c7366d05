// orb_kernels.hpp -- device-side structs and kernel declarations of the ORB extractor.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbfe.h"
#include "../../include/orbfe_math.h"
#include "extractor_plan.hpp"   // LevelGeom, BlurStrip, QT_MAXROOTS, qp_lds_bytes / qt_lds_bytes: what the host plans and the kernels read

namespace orbfe {

// A batch of same-sized images: frame f starts at base + f * fstride, rows are `pitch` bytes apart.
struct ImgView {
    const uint8_t* base;
    uint8_t* base_w; // same memory, writable (null for read-only views)
    size_t fstride;
    int pitch;
};

// The hardware hands workgroups to the 8 XCDs round-robin by linear workgroup id, and every XCD has its own L2.
// Kernels whose workgroups of one frame read overlapping image regions are launched as a 1-D grid of
// xcd_grid(nx * nframes) workgroups and call xcd_remap() for (bx, f): consecutive logical ids -- a frame's nx
// workgroups -- then run on the same XCD and share its L2 instead of fetching the same lines into all eight.
inline int xcd_grid(int total) { return ((total + 7) / 8) * 8; }
#if defined(__HIPCC__)
__device__ __forceinline__ bool xcd_remap(int nx, int total, int& bx, int& f)
{
    const int wg = blockIdx.x, per = (total + 7) >> 3;
    const int logical = (wg & 7) * per + (wg >> 3);
    if (logical >= total) return false;
    f = logical / nx;
    bx = logical - f * nx;
    return true;
}
#endif

__global__ void k_resize_level(ImgView src, ImgView dst, int sw, int sh, int dw4, int dh, double scale_x,
                               double scale_y, int dw);
#define RS_ROWS 8
__global__ void k_resize_tab(ImgView src, ImgView dst, int sw, int sh, int dw4, int dh, int nthreads, const int* xofs,
                             const int* xal, const int4* ytab, int nx, int total);
__global__ void k_fast_cells(ImgView src0, ImgView pyr, const LevelGeom* geom, const uint32_t* cellinfo,
                             uint32_t* slots, size_t slots_fstride, int32_t* cellcnt, int ncells_total, int iniTh,
                             int minTh, int roi_pitch, int roi_rows, int map_pitch, int map_rows, int list_cap, int nx, int total,
                             int cell_base, int cell_end);
__global__ void k_distribute(const LevelGeom* geom, const uint32_t* slots, size_t slots_fstride,
                             const int32_t* cellcnt, int ncells_total, uint32_t* keyscratch, size_t keys_fstride,
                             uint32_t* lvl_out, int out_fstride, int32_t* lvl_cnt, int nlevels, int32_t* lvl_ncand,
                             int keycap_lds, int nodecap, int veccap, const int32_t* worklist, const int32_t* worklist_n);
#define QP_THREADS 256
__global__ void k_distribute_pyr(const LevelGeom* geom, const uint32_t* slots, size_t slots_fstride,
                                 const int32_t* cellcnt, int ncells_total, uint32_t* lvl_out, int out_fstride,
                                 int32_t* lvl_cnt, int nlevels, int32_t* lvl_ncand, int32_t* fallback, int D,
                                 int nodecap, int veccap, int32_t* worklist, int32_t* worklist_n, int by_level);

__global__ void k_level_offsets(const int32_t* lvl_cnt, int32_t* lvl_off, int32_t* n_out, int nlevels, int nframes,
                                int capacity, int32_t* overflow, const LevelGeom* geom, const uint32_t* lvl_out,
                                int out_fstride, uint32_t* flat_kv, uint8_t* flat_lvl, int32_t* worklist_n);
__global__ void k_blur7_mfma(ImgView src0, ImgView pyr, ImgView blur, const LevelGeom* geom, const BlurStrip* strips, const uint4* tabs,
                             const uint4* tab2, int K2, int nstrips, int nx, int total);
#ifndef OD2_LDS_PAD
#define OD2_LDS_PAD 8192   // k_orient_describe2: unused LDS that caps its workgroups at seven a CU (see the kernel)
#endif
__global__ void k_orient_describe2(ImgView src0, ImgView pyr, ImgView blur, const LevelGeom* geom,
                                  const uint32_t* flat_kv, const uint8_t* flat_lvl, const int32_t* n_out, int nlevels,
                                  const uint32_t* pattern32, const uint4* icw, orbfe_keypoint* kps, uint8_t* desc,
                                  int capacity, int nx, int total);

} // namespace orbfe
