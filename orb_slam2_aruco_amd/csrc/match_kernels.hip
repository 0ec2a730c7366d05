// match_kernels.hip -- descriptor matching on gfx950 behind the C ABI (include/orbfe.h, "descriptor matching").
//
//   k_knn2_tiles / k_knn2_merge    all-pairs best / second-best Hamming with the reference update rule
//                                  (inner loop of every ORBmatcher::SearchBy*)
//   k_sfi_grid / _rows / _accept   ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:409-524) incl. the Frame
//                                  grid (src/Frame.cc:183-198, 280-345): a sort per frame, a wave per query for the candidate
//                                  rows, one wave per frame pair for the coupled accept loop
//
// Bound: integer VALU issue (XOR + v_bcnt_u32_b32), not HBM: 1000 x 1000 descriptors are 64 KB of traffic for
// 16 M lane-ops.  Train descriptors are staged through LDS and broadcast to all lanes of a wave.
#include <climits>

#include "host_stage.hpp"
#include "match_plan.hpp"
#include "orbfe_common.hpp"
#include "wave_dpp.hpp"

namespace orbfe {

__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1)
{
    int d = __popc(a0.x ^ b0.x);
    d += __popc(a0.y ^ b0.y);
    d += __popc(a0.z ^ b0.z);
    d += __popc(a0.w ^ b0.w);
    d += __popc(a1.x ^ b1.x);
    d += __popc(a1.y ^ b1.y);
    d += __popc(a1.z ^ b1.z);
    d += __popc(a1.w ^ b1.w);
    return d;
}

// grid: (ceil(max_nq/256), npairs, nsplit).  Split s handles train rows [s*chunk, (s+1)*chunk).
// Partial results go to part_* [pair][split][max_nq]; with nsplit == 1 they are the final arrays.
__global__ __launch_bounds__(256) void k_knn2_tiles(const uint8_t* __restrict__ Q, const int32_t* __restrict__ nq_arr,
                                                    size_t q_stride, int max_nq, const uint8_t* __restrict__ T,
                                                    const int32_t* __restrict__ nt_arr, size_t t_stride, int chunk,
                                                    int init, int32_t* __restrict__ best_idx,
                                                    int32_t* __restrict__ best_dist, int32_t* __restrict__ second_dist)
{
    __shared__ uint4 st[KNN_TILE * 2];
    const int pair = blockIdx.y, split = blockIdx.z, nsplit = gridDim.z;
    const int nq = nq_arr ? nq_arr[pair] : max_nq;
    const int nt = nt_arr[pair];
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 >= nq) return;
    const uint4* Qp = reinterpret_cast<const uint4*>(Q + (size_t)pair * q_stride);
    const uint4* Tp = reinterpret_cast<const uint4*>(T + (size_t)pair * t_stride);
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    if (q < nq) { a0 = Qp[2 * q]; a1 = Qp[2 * q + 1]; }
    int best = init, second = init, idx = -1;
    const int t_begin = split * chunk, t_end = min(nt, t_begin + chunk);
    for (int t0 = t_begin; t0 < t_end; t0 += KNN_TILE) {
        const int m = min(KNN_TILE, t_end - t0);
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * m; i += 256) st[i] = Tp[2 * t0 + i];
        __syncthreads();
        for (int t = 0; t < m; t++) {
            const int d = hamming256(a0, a1, st[2 * t], st[2 * t + 1]);
            if (d < best) { second = best; best = d; idx = t0 + t; }
            else if (d < second) second = d;
        }
    }
    if (q < nq) {
        const size_t o = ((size_t)pair * nsplit + split) * max_nq + q;
        best_idx[o] = idx; best_dist[o] = best; second_dist[o] = second;
    }
}

// ---- all-pairs Hamming distances on the matrix cores.
// For bit vectors a, b:  |a ^ b| = |a| + |b| - 2 a.b, and a.b over 256 bits is an int8 dot product of the bits spread to
// bytes -- an (nq x 256) x (256 x nt) GEMM, which is what MFMA is for.  v_mfma_i32_32x32x32_i8 does a 32 x 32 tile of
// dot products over 32 bits per instruction; eight of them finish a tile.  Per pair the VALU only has to fold the
// result into the running (best, second) keys: one mad, one med3, one min.
//   workgroup = KM_WAVES waves x 32 queries; the train descriptors are spread to bytes once per workgroup and chunk
//   (KM_CHUNK descriptors) in LDS and shared by all waves; the queries' A fragments stay in registers.
// Operand layout: lane l supplies row/column l & 31 and the 16 k-values of half l >> 5; A and B are loaded with the
// same rule, so the order of the k-values inside the instruction does not matter (a.b is a sum over k).
// C layout (cdna4 ISA, 32 x 32): column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
#define KM_ROWB 272 // bytes per spread descriptor in LDS: 256 + 16 keeps the 16-byte reads of adjacent rows on distinct banks
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// middle value of three (the compiler emits v_med3_i32)
__device__ __forceinline__ int med3i(int a, int b, int c) { return max(min(a, b), min(max(a, b), c)); }
// 4 bits -> 4 bytes (bit i -> byte i)
__device__ __forceinline__ int spread4(uint32_t x) { return (int)(__umul24(x & 15u, 0x00204081u) & 0x01010101u); }
// x * 255 for words of 0 / 1 bytes as (x << 8) - x, the shift written as the instruction (the compiler folds the pair back into a
// v_mul_lo_u32 by 255: 5.3 cycles per wave against 2 x 3.4 - 4.5 for the pair, tools/valu_rate.hip -- a wash, kept for the shorter chain).
__device__ __forceinline__ int x255_1(int x)
{
    int t;
    asm("v_lshlrev_b32 %0, 8, %1" : "=v"(t) : "v"(x));
    return t - x;
}
__device__ __forceinline__ v4i x255(v4i p)
{
    v4i r;
    r.x = x255_1(p.x); r.y = x255_1(p.y); r.z = x255_1(p.z); r.w = x255_1(p.w);
    return r;
}
__device__ __forceinline__ v4i spread16(uint32_t bits)
{
    v4i r;
    r.x = spread4(bits); r.y = spread4(bits >> 4); r.z = spread4(bits >> 8); r.w = spread4(bits >> 12);
    return r;
}

__global__ __launch_bounds__(KM_WAVES * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_knn2_mfma(const uint8_t* __restrict__ Q, const int32_t* __restrict__ nq_arr,
                                                             size_t q_stride, int max_nq, const uint8_t* __restrict__ T,
                                                             const int32_t* __restrict__ nt_arr, size_t t_stride, int chunk,
                                                             int init, int32_t* __restrict__ best_idx,
                                                             int32_t* __restrict__ best_dist,
                                                             int32_t* __restrict__ second_dist)
{
    // grid: (query tiles, pairs, nsplit).  Split z handles train rows [z * chunk, (z + 1) * chunk) and writes partials
    // [pair][split][max_nq] for k_knn2_merge, exactly as k_knn2_tiles does; with one split they are the final arrays.
    // the spread train descriptors of the current chunk and, after the loop, the cross-lane merge of the keys share one region:
    // 35 KB per workgroup instead of 69 (the footprint is a cost of its own: it decides what else fits on the CU)
    constexpr int KM_LDS = KM_CHUNK * KM_ROWB > KM_WAVES * 32 * 33 * 4 ? KM_CHUNK * KM_ROWB : KM_WAVES * 32 * 33 * 4;
    __shared__ __align__(16) unsigned char s_u[KM_LDS];
    unsigned char* s_t = s_u;
    int (*s_red)[32][33] = reinterpret_cast<int (*)[32][33]>(s_u);
    __shared__ int s_pt[KM_CHUNK];                                  // their popcounts
    const int pair = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int nq = nq_arr ? nq_arr[pair] : max_nq;
    const int split = blockIdx.z, nsplit = gridDim.z;
    const int t_begin = split * chunk, nt = min(nt_arr[pair], t_begin + chunk);
    const int q0 = blockIdx.x * (KM_WAVES * 32);
    if (q0 >= nq) return;
    const uint32_t* Qp = reinterpret_cast<const uint32_t*>(Q + (size_t)pair * q_stride);
    const uint32_t* Tp = reinterpret_cast<const uint32_t*>(T + (size_t)pair * t_stride);
    const int col = lane & 31, half = lane >> 5;
    const int ie = min(init, 257); // distances are <= 256: any larger start value behaves like 257

    // A fragments: query row (q0 + 32 wid + col), k-step s = dword s of the descriptor, this lane's 16-bit half.  A set bit is
    // the byte -1, so the accumulator holds -(q.t) and a pair's key is ONE v_lshl_add_u32 (with +1 bytes the compiler needs a
    // shift and a subtraction)
    const int qa = q0 + 32 * wid + col;
    v4i a[8];
    {
        const uint4* qrow = reinterpret_cast<const uint4*>(Qp) + (size_t)min(qa, nq - 1) * 2; // clamped, not predicated
        const uint4 d0 = qrow[0], d1 = qrow[1];
        const uint32_t w[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
        for (int s2 = 0; s2 < 8; s2++) {
            const v4i p = spread16((qa < nq ? w[s2] : 0u) >> (16 * half));
            a[s2] = x255(p); // 0x01 -> 0xff per byte, no carries
        }
    }
    // the 16 rows this lane accumulates: row(reg) = (reg & 3) + 8 * (reg >> 2) + 4 * half.  Keys are ((|t| - 2 q.t) << 16) | j: the
    // order of a row's candidates by (distance, index) without the row's own |q|; "accepted iff d < init" is applied when the
    // row is written, so the running keys simply start above every real key
    int bestk[16], secondk[16];
#pragma unroll
    for (int r = 0; r < 16; r++) bestk[r] = secondk[r] = 0x7fffffff;

    // A thread's part of a chunk: dwords 2 p, 2 p + 1 of train row (tid >> 2), p = tid & 3.  The NEXT chunk's part is loaded
    // before the current chunk's tiles are computed and waited for after them: global latency (and with two workgroups per CU
    // in the same rhythm there is nothing else to hide it) is off the chunk's critical path.
    const int ctr = tid >> 2, cpart = tid & 3;
    const uint2* Tp2 = reinterpret_cast<const uint2*>(Tp);
    uint2 nxt = make_uint2(0u, 0u);
    if (t_begin < nt) nxt = Tp2[(size_t)min(t_begin + ctr, nt - 1) * 4 + cpart];
    for (int t0 = t_begin; t0 < nt; t0 += KM_CHUNK) {
        const int m = min(KM_CHUNK, nt - t0);
        uint2 w = nxt;
        if (ctr >= m) w = make_uint2(0u, 0u); // rows past the end: zero bytes, popcount 0
        __syncthreads();                      // every wave is done with the previous chunk
        {
            v4i* dst = reinterpret_cast<v4i*>(s_t + ctr * KM_ROWB + cpart * 64);
            dst[0] = spread16(w.x);
            dst[1] = spread16(w.x >> 16);
            dst[2] = spread16(w.y);
            dst[3] = spread16(w.y >> 16);
            int pc = __popc(w.x) + __popc(w.y);                // |t|: sum over the row's four threads (one quad)
            pc += ORBFE_DPP(0, pc, 0xb1, 0xf);                 // quad_perm [1, 0, 3, 2]
            pc += ORBFE_DPP(0, pc, 0x4e, 0xf);                 // quad_perm [2, 3, 0, 1]
            if (cpart == 0) s_pt[ctr] = pc;
        }
        if (t0 + KM_CHUNK < nt) nxt = Tp2[(size_t)min(t0 + KM_CHUNK + ctr, nt - 1) * 4 + cpart];
        __syncthreads();
        // all four tiles of the chunk, straight-line (rows past the end are zero bytes and get the never-accepted key): one basic
        // block, so that a tile's matrix instructions can be scheduled under the previous tile's key updates
#pragma unroll
        for (int tt = 0; tt < KM_CHUNK; tt += 32) {
            v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            const unsigned char* brow = s_t + (tt + col) * KM_ROWB + 16 * half;
            v4i b[8];
#pragma unroll
            for (int s2 = 0; s2 < 8; s2++) b[s2] = *reinterpret_cast<const v4i*>(brow + 32 * s2); // all eight reads in flight
            const int pt = s_pt[tt + col];
#pragma unroll
            for (int s2 = 0; s2 < 8; s2++) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s2], b[s2], acc, 0, 0, 0);
            // this lane's column is train t0 + tt + col; a column past the end has zero bytes (acc = 0) and a key above every real one
            const uint32_t cj = (tt + col < m) ? (((uint32_t)pt << 16) | (uint32_t)(t0 + tt + col)) : 0x7fffffffu;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int key = (int)(((uint32_t)acc[r] << 17) + cj); // ((|t| - 2 q.t) << 16) | j
                secondk[r] = med3i(bestk[r], secondk[r], key);       // middle of the three
                bestk[r] = min(bestk[r], key);
            }
        }
    }
    // merge the 32 column classes of every row through LDS: s_red[wave][row][column class]
    __syncthreads(); // every wave has read the last chunk: the region changes hands
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; r++) s_red[wid][(r & 3) + 8 * (r >> 2) + 4 * half][col] = pass == 0 ? bestk[r] : secondk[r];
        __builtin_amdgcn_wave_barrier();
        // lane = (row = col, half h): scans 16 column classes
        int b1 = 0x7fffffff, b2 = 0x7fffffff; // two smallest keys of the scanned entries
#pragma unroll
        for (int c = 0; c < 16; c++) {
            const int key = s_red[wid][col][16 * half + c];
            b2 = med3i(b1, b2, key);
            b1 = min(b1, key);
        }
        // combine the two halves of the row (lanes l and l ^ 32)
        const int o1 = __shfl_xor(b1, 32), o2 = __shfl_xor(b2, 32);
        const int n1 = min(b1, o1);
        const int n2 = min(max(b1, o1), min(b2, o2));
        if (pass == 0) { bestk[0] = n1; bestk[1] = n2; }       // two smallest "best" keys of the row
        else { secondk[0] = n1; }                              // smallest "second" key of the row
    }
    // row's best = smallest best key; row's second = min(second smallest best key, smallest second key)
    if (half == 0) {
        const int qr = q0 + 32 * wid + col;
        if (qr < nq) {
            uint4 d0 = reinterpret_cast<const uint4*>(Qp)[(size_t)qr * 2], d1 = reinterpret_cast<const uint4*>(Qp)[(size_t)qr * 2 + 1];
            const int pq = __popc(d0.x) + __popc(d0.y) + __popc(d0.z) + __popc(d0.w) + __popc(d1.x) + __popc(d1.y) + __popc(d1.z) + __popc(d1.w);
            const int kb = bestk[0], ks = min(bestk[1], secondk[0]);
            int bd = (kb >> 16) + pq, sd = (ks >> 16) + pq, bi = kb & 0xffff;
            if (bd >= ie) { bd = init; bi = -1; }
            if (sd >= ie) sd = init;
            const size_t o = ((size_t)pair * nsplit + split) * max_nq + qr;
            best_idx[o] = bi; best_dist[o] = bd; second_dist[o] = sd;
        }
    }
}

// Merge the per-split partials in ascending split order (earlier candidates win ties, as in the serial loop).
__global__ void k_knn2_merge(const int32_t* __restrict__ pidx, const int32_t* __restrict__ pbest,
                             const int32_t* __restrict__ psecond, int nsplit, int max_nq,
                             const int32_t* __restrict__ nq_arr, int32_t* __restrict__ best_idx,
                             int32_t* __restrict__ best_dist, int32_t* __restrict__ second_dist)
{
    const int pair = blockIdx.y;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const int nq = nq_arr ? nq_arr[pair] : max_nq;
    if (q >= nq) return;
    int best = INT_MAX, second = INT_MAX, idx = -1;
    for (int s = 0; s < nsplit; s++) {
        const size_t o = ((size_t)pair * nsplit + s) * max_nq + q;
        const int b = pbest[o], sc = psecond[o], i = pidx[o];
        if (s == 0) { best = b; second = sc; idx = i; continue; }
        if (b < best) { second = min(best, sc); best = b; idx = i; }
        else second = min(second, b);
    }
    const size_t o = (size_t)pair * max_nq + q;
    best_idx[o] = idx; best_dist[o] = best; second_dist[o] = second;
}

// ---------------------------------------------------------------------------- SearchForInitialization ----------

// One workgroup (256 threads) per frame pair p: F1 = frame p, F2 = frame p+1 of a stream.
// Phase A: F2's level-0 keypoints sorted by (grid column, grid row, index) in LDS.  That is exactly the order in which
//   Frame::GetFeaturesInArea walks the 64x48 grid (ix outer, iy inner, push_back order inside a cell), and
//   SearchForInitialization only ever asks for level 0 (minLevel = maxLevel = 0), so a query's candidate list is the
//   sub-sequence of this list whose cell lies in the query's cell rectangle and which passes the |dx|,|dy| < r test.
// Phase B (parallel, one wave per query): candidate indices + Hamming distances into a fixed-stride scratch row.
// Phase C (wave 0, serial over i1 as in the reference because vMatchedDistance couples the queries): best /
//   second-best with the "already matched better" skip, ratio + TH_LOW tests, mutual-uniqueness bookkeeping,
//   rotation histogram, ComputeThreeMaxima, final vbPrevMatched update.
// Three launches (round 3; before: one 1024-thread workgroup + 55 KB of LDS per frame pair, fifteen of its sixteen waves parked
// while one wave ran the serial loop -- 146 us alone, 640 us next to the other engines' kernels):
//   k_sfi_grid    workgroup per FRAME: what a frame contributes in either role.  As F2: its level-0 keypoints inside the Frame
//                 grid sorted by (grid column, grid row, index) -- the order in which GetFeaturesInArea walks the 64 x 48 grid
//                 (Frame.cc:183-198, :280-345) -- with position, angle and descriptor laid out by rank; as F1: its level-0
//                 keypoints in index order (the queries).  A frame of a batch is F2 of one pair and F1 of the next.
//   k_sfi_rows    wave per query, all pairs of the batch in one grid (a throughput kernel): window test against F2's sorted
//                 list, Hamming distance of every candidate, one contiguous row (distance << 16 | rank, candidate order) per
//                 query in the pair's pool; rows are placed by an atomic cursor, so a pool is dense and any order.
//   k_sfi_accept  ONE WAVE per pair (64-thread workgroups): the reference's serial loop -- the "already matched better" skip and
//                 the mutual-uniqueness bookkeeping couple the queries (ORBmatcher.cc:448-449, :467-475) -- out of LDS, then the
//                 rotation histogram, ComputeThreeMaxima and the vbPrevMatched update.
struct SfiGrid { // [frame][SFI_MAXL0] arrays in HBM, written by k_sfi_grid
    int32_t* nl0;     // [frames] level-0 keypoints inside the grid (role F2), clamped to SFI_MAXL0
    int32_t* nq;      // [frames] level-0 keypoints (role F1), clamped to SFI_MAXL0
    uint32_t* sorted; // (cell << 16) | index, ascending
    float2* xy;       // by rank
    float* ang;       // by rank
    uint4* desc;      // by rank, two per keypoint
    uint16_t* query;  // by query position: keypoint index
    float2* qxy;      // by query position: the keypoint's own position (the window centre unless vbPrevMatched is given)
    int32_t* cursor;  // [pairs * SFI_CURSOR_PAD] next free pool entry (zeroed here, advanced by k_sfi_rows); one per 256 bytes, so that
                      //   the 65 k atomics of a batch do not queue on a handful of cache lines of one L2 channel
};
#define SFI_GRID_THREADS 256
#define SFI_ROWS_BX 64         // workgroups per pair in k_sfi_rows (4 waves each, one query per wave and trip)
#define SFI_POOL_LDS 6144      // pool entries k_sfi_accept stages in LDS (24 KB); later ones are read from the pool in HBM
#define SFI_ROW_BITS 11        // row record = offset << 11 | count (count <= SFI_MAXL0 = 1024)

__global__ __launch_bounds__(SFI_GRID_THREADS) void k_sfi_grid(const orbfe_keypoint* __restrict__ kps, const uint8_t* __restrict__ desc,
                                                               const int32_t* __restrict__ nkp, int capacity, int nframes, float4 bnd,
                                                               SfiGrid G, int32_t* __restrict__ overflow)
{
    __shared__ __align__(16) uint32_t s_key[SFI_MAXL0 + 4];
    __shared__ int s_nl0;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const orbfe_keypoint* k = kps + (size_t)f * capacity;
    const uint8_t* d = desc + (size_t)f * capacity * 32;
    const int n = nkp[f];
    // bounds of the undistorted image (Frame::ComputeImageBounds; 0, 0, cols, rows without distortion) and Frame.cc:112-113
    const float mnMinX = bnd.x, mnMinY = bnd.y;
    const float invW = __fdiv_rn((float)GRID_COLS, bnd.z - bnd.x);
    const float invH = __fdiv_rn((float)GRID_ROWS, bnd.w - bnd.y);
    if (tid == 0) { s_nl0 = 0; if (f < nframes - 1) G.cursor[(size_t)f * SFI_CURSOR_PAD] = 0; }
    __syncthreads();
    // role F2: level-0 keypoints that fall inside the grid (Frame.cc:183-198, :335-345)
    for (int i = tid; i < n; i += SFI_GRID_THREADS) {
        const orbfe_keypoint kp = k[i];
        if (kp.octave != 0) continue;
        const int px = (int)roundf(__fmul_rn(kp.x - mnMinX, invW));
        const int py = (int)roundf(__fmul_rn(kp.y - mnMinY, invH));
        if (px >= 0 && px < GRID_COLS && py >= 0 && py < GRID_ROWS) {
            const int e = atomicAdd(&s_nl0, 1);
            if (e < SFI_MAXL0) s_key[e] = ((uint32_t)(px * GRID_ROWS + py) << 16) | (uint32_t)i;
        }
    }
    // role F1: level-0 keypoints in index order (ORBmatcher.cc:425-428), wave 0 by ballots
    if (wid == 0) {
        int nq = 0;
        uint16_t* qo = G.query + (size_t)f * SFI_MAXL0;
        float2* qp = G.qxy + (size_t)f * SFI_MAXL0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            orbfe_keypoint kp;
            kp.octave = 1;
            if (i < n) kp = k[i];
            const bool isq = i < n && kp.octave <= 0;
            const unsigned long long m = __ballot(isq);
            const int pos = nq + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
            if (isq && pos < SFI_MAXL0) { qo[pos] = (uint16_t)i; qp[pos] = make_float2(kp.x, kp.y); }
            nq += __popcll(m);
        }
        if (lane == 0) {
            if (nq > SFI_MAXL0) { atomicMax(overflow, nq); nq = SFI_MAXL0; }
            G.nq[f] = nq;
        }
    }
    __syncthreads();
    int nl0 = s_nl0;
    if (nl0 > SFI_MAXL0) { if (tid == 0) atomicMax(overflow, nl0); nl0 = SFI_MAXL0; }
    if (tid == 0) G.nl0[f] = nl0;
    if (tid < 4) s_key[nl0 + tid] = 0xffffffffu; // the counting loop reads whole uint4s
    __syncthreads();
    // sort by counting: the keys are distinct (the index is part of them), so an entry's rank is the number of smaller keys --
    // broadcast LDS reads, no barrier; the rank-ordered record goes straight to HBM
    const uint4* k4 = reinterpret_cast<const uint4*>(s_key);
    for (int e = tid; e < nl0; e += SFI_GRID_THREADS) {
        const uint32_t key = s_key[e];
        int r = 0;
        for (int j = 0; j < (nl0 + 3) / 4; j++) {
            const uint4 v = k4[j];
            r += (v.x < key) + (v.y < key) + (v.z < key) + (v.w < key);
        }
        const int i2 = key & 0xffff;
        const orbfe_keypoint kp = k[i2];
        const size_t o = (size_t)f * SFI_MAXL0 + r;
        G.sorted[o] = key;
        G.xy[o] = make_float2(kp.x, kp.y);
        G.ang[o] = kp.angle;
        G.desc[2 * o] = reinterpret_cast<const uint4*>(d)[2 * i2];
        G.desc[2 * o + 1] = reinterpret_cast<const uint4*>(d)[2 * i2 + 1];
    }
}

// Candidates of one query among four 64-entry chunks (c0 .. c0 + 3) of F2's sorted list: window test, then the Hamming distances
// with all loads of the four chunks in flight together.  keys[k] = distance << 20 | position in the row << 10 | rank (0x7fffffff:
// no candidate); returns the number of candidates found (wave-uniform).
struct SfiWindow { float x, y, r; int minx, maxx, miny, maxy; };
__device__ __forceinline__ int sfi_chunks4(const SfiGrid& G, size_t g2, int nl0, int c0, int lane, const SfiWindow& W, const uint4& a0,
                                           const uint4& a1, int base, int* keys)
{
    uint32_t cell[4];
    float2 xy[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int j = (c0 + k) * 64 + lane;
        cell[k] = 0xffffffffu; xy[k] = make_float2(0.f, 0.f);
        if (j < nl0) { cell[k] = G.sorted[g2 + j] >> 16; xy[k] = G.xy[g2 + j]; }
    }
    bool ok[4];
    uint4 b0[4], b1[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        // Frame::GetFeaturesInArea (Frame.cc:280-333): the cell range of the window, then |dx| < r and |dy| < r
        const int cx = (int)(cell[k] / GRID_ROWS), cy = (int)(cell[k] - (uint32_t)cx * GRID_ROWS);
        ok[k] = cell[k] != 0xffffffffu && cx >= W.minx && cx <= W.maxx && cy >= W.miny && cy <= W.maxy && fabsf(xy[k].x - W.x) < W.r &&
                fabsf(xy[k].y - W.y) < W.r;
        if (ok[k]) { const size_t o = 2 * (g2 + (size_t)((c0 + k) * 64 + lane)); b0[k] = G.desc[o]; b1[k] = G.desc[o + 1]; }
    }
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned long long m = __ballot(ok[k]);
        keys[k] = 0x7fffffff;
        if (ok[k]) {
            const int pos = base + n + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
            const int dd = hamming256(a0, a1, b0[k], b1[k]); // 256 only for exact complements; 255 is far above TH_LOW as well
            keys[k] = (min(dd, 255) << 20) | (pos << 10) | ((c0 + k) * 64 + lane);
        }
        n += (int)__popcll(m);
    }
    return n;
}

#define SFI_ROWS_WAVES 4
__global__ __launch_bounds__(SFI_ROWS_WAVES * 64) void k_sfi_rows(const orbfe_keypoint* __restrict__ kps, const uint8_t* __restrict__ desc,
                                                                  int capacity, float4 bnd, float window, const float* __restrict__ prev_in,
                                                                  SfiGrid G, uint32_t* __restrict__ pool, int pool_cap,
                                                                  uint32_t* __restrict__ rowrec, int32_t* __restrict__ overflow)
{
    __shared__ int s_keys[SFI_ROWS_WAVES][SFI_MAXL0]; // the wave's row, by candidate position, for the rank-by-counting sort
    const int p = blockIdx.y, lane = threadIdx.x & 63, wid = wave_id();
    const int nq = G.nq[p], nl0 = G.nl0[p + 1];
    const size_t g1 = (size_t)p * SFI_MAXL0, g2 = (size_t)(p + 1) * SFI_MAXL0;
    const uint8_t* d1 = desc + (size_t)p * capacity * 32;
    const float* prev = prev_in ? prev_in + (size_t)p * capacity * 2 : nullptr;
    uint32_t* pl = pool + (size_t)p * pool_cap;
    const float mnMinX = bnd.x, mnMinY = bnd.y;
    const float invW = __fdiv_rn((float)GRID_COLS, bnd.z - bnd.x);
    const float invH = __fdiv_rn((float)GRID_ROWS, bnd.w - bnd.y);
    int* row = s_keys[wid];
    (void)kps;
    for (int q = blockIdx.x * SFI_ROWS_WAVES + wid; q < nq; q += gridDim.x * SFI_ROWS_WAVES) {
        const int i1 = __builtin_amdgcn_readfirstlane((int)G.query[g1 + q]);
        float2 c = G.qxy[g1 + q];
        if (prev) c = make_float2(prev[2 * i1], prev[2 * i1 + 1]);
        SfiWindow W;
        W.x = c.x; W.y = c.y; W.r = window;
        W.minx = max(0, (int)floorf(__fmul_rn(c.x - mnMinX - W.r, invW)));
        W.maxx = min(GRID_COLS - 1, (int)ceilf(__fmul_rn(c.x - mnMinX + W.r, invW)));
        W.miny = max(0, (int)floorf(__fmul_rn(c.y - mnMinY - W.r, invH)));
        W.maxy = min(GRID_ROWS - 1, (int)ceilf(__fmul_rn(c.y - mnMinY + W.r, invH)));
        const bool any = !(W.minx >= GRID_COLS || W.maxx < 0 || W.miny >= GRID_ROWS || W.maxy < 0);
        const uint4 a0 = reinterpret_cast<const uint4*>(d1)[2 * i1];
        const uint4 a1 = reinterpret_cast<const uint4*>(d1)[2 * i1 + 1];
        int count = 0;
        if (any)
            for (int c0 = 0; c0 * 64 < nl0; c0 += 4) { // the row in candidate order, wave-private LDS
                int keys[4];
                const int n = sfi_chunks4(G, g2, nl0, c0, lane, W, a0, a1, count, keys);
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (keys[k] != 0x7fffffff) row[(keys[k] >> 10) & 0x3ff] = keys[k];
                count += n;
            }
        int off = 0;
        if (lane == 0 && count > 0) off = atomicAdd(&G.cursor[(size_t)p * SFI_CURSOR_PAD], count);
        // sorted by (distance, position): the accept loop then takes the first two candidates that are not skipped instead of
        // reducing the row.  Rank by counting (the keys are distinct), broadcast LDS reads; the first 64 entries are ranked while
        // the cursor's atomic is in flight.
        auto rank_of = [&](int e, int& key) {
            key = e < count ? row[e] : 0x7fffffff;
            int r = 0;
            for (int t = 0; t < count; t++) r += row[t] < key;
            return r;
        };
        int key0 = 0x7fffffff;
        const int r0 = count > 0 ? rank_of(lane, key0) : 0;
        off = __builtin_amdgcn_readfirstlane(off);
        bool fits = true;
        if (count > 0 && off + count > pool_cap) { // the pool is too small: flagged, the host grows it and the batch is repeated
            if (lane == 0) atomicMax(overflow + 1, off + count);
            fits = false;
        }
        if (lane == 0) rowrec[g1 + q] = fits ? ((uint32_t)off << SFI_ROW_BITS) | (uint32_t)count : 0u;
        if (count == 0 || !fits) continue;
        if (lane < count) pl[off + r0] = ((uint32_t)(key0 >> 20) << 16) | (uint32_t)(key0 & 0x3ff);
        for (int e0 = 64; e0 < count; e0 += 64) {
            int key;
            const int r = rank_of(e0 + lane, key);
            if (e0 + lane < count) pl[off + r] = ((uint32_t)(key >> 20) << 16) | (uint32_t)(key & 0x3ff);
        }
    }
}

// The serial loop of k_sfi_accept (see there).  IN_LDS: the pair's whole pool is staged in LDS -- no global path, hence no
// branch and no vmcnt wait inside the loop.
template <bool IN_LDS>
__device__ __forceinline__ void sfi_accept_loop(int nq, int lane, float nnratio, const uint32_t* s_pool, uint32_t* s_state,
                                                const uint32_t* s_row, uint16_t* s_acc, uint16_t* s_held, const uint32_t* __restrict__ pl)
{
    constexpr int NIL = 0xffff;
    auto rfl = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
    constexpr uint32_t CNT = (1u << SFI_ROW_BITS) - 1;
    auto entry = [&](int o) { return IN_LDS || o < SFI_POOL_LDS ? s_pool[min(o, SFI_POOL_LDS - 1)] : pl[o]; };
    // rows longer than a wave whose first 64 entries did not settle best and second: the later chunks, in order
    auto long_row = [&](int e, int off, int& bestDist, int& bestRank, uint32_t& bestState, int& bestDist2) {
        for (int j0 = 64; j0 < e; j0 += 64) {
            const uint32_t en = j0 + lane < e ? entry(off + j0 + lane) : 0u;
            const int rk = (int)(en & 0x3ffu), dd = (int)(en >> 16);
            const uint32_t st = s_state[rk];
            unsigned long long open = __ballot(j0 + lane < e && (int)(st >> 16) > dd);
            if (open && bestDist < 0) {
                const int b = __builtin_ctzll(open);
                bestDist = __builtin_amdgcn_readlane(dd, b);
                bestRank = __builtin_amdgcn_readlane(rk, b);
                bestState = (uint32_t)__builtin_amdgcn_readlane((int)st, b);
                open &= open - 1;
            }
            if (open) { bestDist2 = __builtin_amdgcn_readlane(dd, __builtin_ctzll(open)); return; }
        }
    };
    uint32_t rr = nq > 0 ? rfl(s_row[0]) : 0u, rr1 = nq > 1 ? rfl(s_row[1]) : 0u;
    uint32_t ent = entry((int)(rr >> SFI_ROW_BITS) + lane);
    for (int q = 0; q < nq; q++) {
        const int e = (int)(rr & CNT), off = (int)(rr >> SFI_ROW_BITS);
        const int rk = (int)(ent & 0x3ffu), dd = (int)(ent >> 16);
        const uint32_t st = s_state[rk];                                        // the loop-carried read
        const uint32_t ent1 = entry((int)(rr1 >> SFI_ROW_BITS) + lane);         // row q + 1
        const uint32_t rr2 = s_row[min(q + 2, SFI_MAXL0 - 1)];                  // record of row q + 2
        unsigned long long open = __ballot(lane < e && (int)(st >> 16) > dd);
        int bestDist = -1, bestRank = 0, bestDist2 = INT_MAX;
        uint32_t bestState = 0;
        if (open) {
            const int b = __builtin_ctzll(open);
            bestDist = __builtin_amdgcn_readlane(dd, b);
            bestRank = __builtin_amdgcn_readlane(rk, b);
            bestState = (uint32_t)__builtin_amdgcn_readlane((int)st, b);
            open &= open - 1;
            if (open) bestDist2 = __builtin_amdgcn_readlane(dd, __builtin_ctzll(open));
        }
        if (e > 64 && !open) long_row(e, off, bestDist, bestRank, bestState, bestDist2);
        if (bestDist >= 0 && bestDist <= 50 && (float)bestDist < __fmul_rn((float)bestDist2, nnratio)) { // TH_LOW, ratio test
            if (lane == 0) {
                const int old = (int)(bestState & 0xffffu) - 1;
                if (old >= 0) s_held[old] = NIL;      // the earlier query loses the keypoint (:467-471)
                s_state[bestRank] = ((uint32_t)bestDist << 16) | (uint32_t)(q + 1);
                s_held[q] = (uint16_t)bestRank;
                s_acc[q] = (uint16_t)bestRank;
            }
            __builtin_amdgcn_wave_barrier();
        }
        rr = rr1; rr1 = q + 2 < nq ? rfl(rr2) : 0u; ent = ent1;
    }
}

__global__ __launch_bounds__(64) void k_sfi_accept(const orbfe_keypoint* __restrict__ kps, const int32_t* __restrict__ nkp, int capacity,
                                                   float nnratio, int check_ori, const float* __restrict__ prev_in,
                                                   float* __restrict__ prev_out, int32_t* __restrict__ matches12,
                                                   int32_t* __restrict__ nmatches_out, SfiGrid G, const uint32_t* __restrict__ pool,
                                                   int pool_cap, const uint32_t* __restrict__ rowrec)
{
    __builtin_amdgcn_s_setprio(2); // latency-bound: one wave per pair goes first when a VALU-bound kernel shares the CU
    __shared__ __align__(16) uint32_t s_pool[SFI_POOL_LDS];
    __shared__ uint32_t s_state[SFI_MAXL0]; // vMatchedDistance << 16 | (position of the query in vnMatches21 + 1), indexed by the RANK
                                            //   of an F2 keypoint (only level-0 keypoints of F2 inside the grid can ever be matched)
    __shared__ uint32_t s_row[SFI_MAXL0];   // per query: pool offset << 11 | candidates
    __shared__ uint16_t s_acc[SFI_MAXL0];   // per query: rank accepted with, or NIL
    __shared__ uint16_t s_held[SFI_MAXL0];  // per query: rank still held, or NIL
    __shared__ signed char s_rotbin[SFI_MAXL0]; // per query: histogram bin or -1
    __shared__ int s_hist[30];
    const int p = blockIdx.x, lane = threadIdx.x;
    const orbfe_keypoint* k1 = kps + (size_t)p * capacity;
    const orbfe_keypoint* k2 = kps + (size_t)(p + 1) * capacity;
    const int n1 = nkp[p];
    const int nq = G.nq[p], nl0 = G.nl0[p + 1];
    const size_t g1 = (size_t)p * SFI_MAXL0, g2 = (size_t)(p + 1) * SFI_MAXL0;
    const uint16_t* qi = G.query + g1;
    int32_t* m12 = matches12 + (size_t)p * capacity;
    const float* prev = prev_in ? prev_in + (size_t)p * capacity * 2 : nullptr;
    float* prevo = prev_out ? prev_out + (size_t)p * capacity * 2 : nullptr;
    const uint32_t* pl = pool + (size_t)p * pool_cap;
    constexpr int NIL = 0xffff;

    // the pair's candidate rows -> LDS (dense pool: a flat copy), the per-query and per-keypoint state.  All of it without
    // predicated loads -- a load under `if (i < n)` becomes a branch with a full wait behind it, one L2 round trip per trip -- the
    // buffers are sized so that whole batches may be read: the pool holds >= 16 K entries per pair (SFI_POOL_LDS are copied), the
    // row records SFI_MAXL0 per pair.
#ifdef ORBFE_SFI_TIMING // diagnosis build (tools/build_timing.sh): phase clocks of one pair, s_memrealtime ticks of 10 ns
    const unsigned long long t_0 = wall_clock64();
#endif
    const int total = min(G.cursor[(size_t)p * SFI_CURSOR_PAD], pool_cap);
    {
        const uint4* src = reinterpret_cast<const uint4*>(pl); // pool_cap is a multiple of 4
        uint4* dst = reinterpret_cast<uint4*>(s_pool);
        const int n4 = (min(total, SFI_POOL_LDS) + 3) / 4;
        static_assert(SFI_POOL_LDS % (4 * 64 * 8) == 0, "whole batches");
        for (int i0 = 0; i0 < n4; i0 += 64 * 8) { // eight loads in flight per lane
            uint4 v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = src[i0 + k * 64 + lane];
#pragma unroll
            for (int k = 0; k < 8; k++) dst[i0 + k * 64 + lane] = v[k];
        }
        for (int i0 = 0; i0 < nq; i0 += 64 * 4) {
            uint32_t v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = rowrec[g1 + i0 + k * 64 + lane];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int i = i0 + k * 64 + lane;
                s_row[i] = i < nq ? v[k] : 0u; s_acc[i] = NIL; s_held[i] = NIL; s_rotbin[i] = -1;
            }
        }
    }
    for (int i = lane; i < SFI_MAXL0; i += 64) s_state[i] = 0xffff0000u;
    if (lane < 30) s_hist[lane] = 0;
    for (int i = lane; i < n1; i += 64) m12[i] = -1;
    __builtin_amdgcn_wave_barrier();

    // ---- the serial matching loop (ORBmatcher.cc:423-490).  It carries only what couples the queries -- vMatchedDistance /
    // vnMatches21 per F2 keypoint and which query currently holds it; everything else (vnMatches12 in HBM, the rotation bins) is
    // written by all lanes after the loop from two per-query records: the rank a query was accepted with (rotHist keeps it even
    // if the match is stolen later, :470-488) and the rank it still holds.
    // A query's row is sorted by (distance, candidate position), so "best = first minimum among the candidates whose
    // vMatchedDistance exceeds their distance (:448-449), second = the next smallest" is: the first two candidates of the row that
    // are not skipped -- one gather of the keypoints' state words, one ballot, two scalar bit scans; no wave reduction on the
    // loop-carried chain.  One LDS round trip on that chain per query: the gather is issued first, the row of query q + 1 and the
    // row record of query q + 2 behind it (LDS answers in order, so the wait for the gather does not wait for them); every LDS
    // read of the loop is unconditional (clamped addresses), only the ballot looks at the row length.
    const float factor = 1.0f / 30; // HISTO_LENGTH; the upstream "1/30" quirk is kept (App. D)
#ifdef ORBFE_SFI_TIMING
    const unsigned long long t_1 = wall_clock64();
#endif
    if (total <= SFI_POOL_LDS) sfi_accept_loop<true>(nq, lane, nnratio, s_pool, s_state, s_row, s_acc, s_held, pl);
    else sfi_accept_loop<false>(nq, lane, nnratio, s_pool, s_state, s_row, s_acc, s_held, pl); // rows beyond the staged part of the pool
    __builtin_amdgcn_wave_barrier();
#ifdef ORBFE_SFI_TIMING
    const unsigned long long t_2 = wall_clock64();
#endif
    int nmatches = 0;
    for (int q0 = 0; q0 < nq; q0 += 4 * 64) {   // four queries a lane and trip: their index, match and angle loads in flight together
        int rr[4], ra[4], qidx[4];
        bool in[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int q = q0 + 64 * k + lane, qc = min(q, nq - 1);
            in[k] = q < nq;
            rr[k] = s_held[qc]; ra[k] = s_acc[qc];
            qidx[k] = qi[qc];
        }
        uint32_t srt[4];
        float a1[4], a2[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            srt[k] = G.sorted[g2 + (rr[k] != NIL ? rr[k] : 0)];
            a1[k] = k1[qidx[k]].angle;
            a2[k] = G.ang[g2 + (ra[k] != NIL ? ra[k] : 0)];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int q = q0 + 64 * k + lane;
            const bool held = in[k] && rr[k] != NIL;
            if (held) m12[qidx[k]] = (int)(srt[k] & 0xffff);
            if (in[k] && check_ori && ra[k] != NIL) {
                float rot = a1[k] - a2[k];
                if (rot < 0.0f) rot += 360.0f;
                int bin = (int)roundf(__fmul_rn(rot, factor));
                if (bin == 30) bin = 0;
                s_rotbin[q] = (signed char)bin; // rotHist[bin].push_back(i1): stays even if un-matched later
            }
            nmatches += (int)__popcll(__ballot(held));
        }
    }
    __threadfence_block();
    if (check_ori) {
        // histogram sizes count every push_back, including i1 whose match was later stolen (as in the reference)
        for (int i = lane; i < nq; i += 64)
            if (s_rotbin[i] >= 0) atomicAdd(&s_hist[s_rotbin[i]], 1);
        __builtin_amdgcn_wave_barrier();
        int ind1 = -1, ind2 = -1, ind3 = -1, max1 = 0, max2 = 0, max3 = 0;
        for (int i = 0; i < 30; i++) { // ComputeThreeMaxima, ORBmatcher.cc:1605-1646
            const int sz = s_hist[i];
            if (sz > max1) { max3 = max2; max2 = max1; max1 = sz; ind3 = ind2; ind2 = ind1; ind1 = i; }
            else if (sz > max2) { max3 = max2; max2 = sz; ind3 = ind2; ind2 = i; }
            else if (sz > max3) { max3 = sz; ind3 = i; }
        }
        if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
        else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
        int removed = 0;
        for (int q0 = 0; q0 < nq; q0 += 4 * 64) {
            int qidx[4];
#pragma unroll
            for (int k = 0; k < 4; k++) qidx[k] = qi[min(q0 + 64 * k + lane, nq - 1)];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int q = q0 + 64 * k + lane;
                bool rm = false;
                if (q < nq) {
                    const int bin = s_rotbin[q];
                    rm = bin >= 0 && bin != ind1 && bin != ind2 && bin != ind3 && s_held[q] != NIL;
                    if (rm) m12[qidx[k]] = -1;
                }
                removed += (int)__popcll(__ballot(rm));
            }
        }
        nmatches -= removed;
    }
    __threadfence_block();
    if (prevo)
        for (int i0 = 0; i0 < n1; i0 += 4 * 64) {   // four entries a lane, their loads in flight together (they were a round trip each:
            float x[4], y[4];                        //   the match, then the keypoint it names, sixteen times over for one pair)
            int m[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int i = min(i0 + 64 * k + lane, n1 - 1);
                x[k] = prev ? prev[2 * i] : k1[i].x; y[k] = prev ? prev[2 * i + 1] : k1[i].y;
                m[k] = m12[i];
            }
            float mx[4], my[4];
#pragma unroll
            for (int k = 0; k < 4; k++) { const int mm = max(m[k], 0); mx[k] = k2[mm].x; my[k] = k2[mm].y; }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int i = i0 + 64 * k + lane;
                if (i < n1) {
                    prevo[2 * i] = m[k] >= 0 ? mx[k] : x[k];
                    prevo[2 * i + 1] = m[k] >= 0 ? my[k] : y[k];
                }
            }
        }
    if (lane == 0) nmatches_out[p] = nmatches;
#ifdef ORBFE_SFI_TIMING
    if (lane == 0 && (p == 7 || p == 150))
        printf("k_sfi_accept pair %d: nq %d nl0 %d pool %d | stage %llu loop %llu epilogue %llu (x 10 ns)\n", p, nq, nl0, total, t_1 - t_0,
               t_2 - t_1, wall_clock64() - t_2);
#endif
}

// ---------------------------------------------------------------------------- guided knn2 (CSR) ----------------
// Best / second-best of every query over ITS candidate list (CSR: offsets[nq + 1], idx[]) -- the inner loop of the guided
// searches whose candidates the caller builds (SearchByBoW node lists ORBmatcher.cc:159-292, Fuse, SearchForTriangulation).
// One wave per query; strict '<', the first candidate in list order wins ties.
__global__ __launch_bounds__(256) void k_knn2_csr(const uint8_t* __restrict__ Q, int nq, const uint8_t* __restrict__ T,
                                                  const int32_t* __restrict__ offsets, const int32_t* __restrict__ idx,
                                                  int init, int32_t* __restrict__ best_idx, int32_t* __restrict__ best_dist,
                                                  int32_t* __restrict__ second_dist)
{
    const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const uint4 a0 = reinterpret_cast<const uint4*>(Q)[2 * q], a1 = reinterpret_cast<const uint4*>(Q)[2 * q + 1];
    const int b = offsets[q], e = offsets[q + 1];
    unsigned long long bestk = ~0ull, secondk = ~0ull; // (distance << 32) | position in the list
    for (int j0 = b; j0 < e; j0 += 64) {
        const int j = j0 + lane;
        unsigned long long key = ~0ull;
        if (j < e) {
            const int t = idx[j];
            const int d = hamming256(a0, a1, reinterpret_cast<const uint4*>(T)[2 * t], reinterpret_cast<const uint4*>(T)[2 * t + 1]);
            if (d < init) key = ((unsigned long long)d << 32) | (unsigned)(j - b);
        }
        const unsigned long long m1 = wave_min_u64(key);
        const unsigned long long k2 = wave_min_u64(key == m1 ? ~0ull : key);
        if (m1 < bestk) { secondk = min(bestk, k2); bestk = m1; }
        else secondk = min(secondk, m1);
    }
    if (lane == 0) {
        best_idx[q] = bestk != ~0ull ? idx[b + (int)(bestk & 0xffffffffu)] : -1;
        best_dist[q] = bestk != ~0ull ? (int)(bestk >> 32) : init;
        second_dist[q] = secondk != ~0ull ? (int)(secondk >> 32) : init;
    }
}

// ---------------------------------------------------------------------------- SearchByProjection ---------------
// The matching loop of ORBmatcher::SearchByProjection (ORBmatcher.cc:45-129) on flat arrays; see include/orbfe.h.
// One workgroup (16 waves) per frame.
//   A  the Frame grid (Frame.cc:183-198, :335-345): keypoints sorted by (cell, index); cell start offsets; per-rank
//      position / octave / taken flag in LDS.  Sorted order inside a run of cells of one grid column IS the order in
//      which GetFeaturesInArea (Frame.cc:280-333) walks them, so a query's candidates are one contiguous range per column.
//   B  one wave per query: candidates that pass the octave and window tests, with their Hamming distances, as a row
//      (rank u16, distance u8) in scratch, in candidate order.
//   C  mode 0: one wave per query resolves best / second-best over the row (strict '<', first candidate wins);
//      mode 1: ONE wave walks the queries in order, because an accepted keypoint is taken for the queries after it.
//      mode 2: the loop of SearchByProjection(CurrentFrame, LastFrame, th, mono) (ORBmatcher.cc:1355-1471): best only,
//              accept best <= th_high, the accepted keypoint is taken when the query's map point has observations, rotation
//              histogram + ComputeThreeMaxima; the result is per keypoint of the frame (match_cur[i2] = query or -1).
#define SBP_THREADS 1024
struct SbpQuery { float x, y, r; int32_t min_level, max_level; }; // r < 0: no search (the point did not project into the frame)
struct SbpBest { // mode 2 only (q_blocks: modes 1 and 2)
    const float* q_angle;     // LastFrame.mvKeysUn[i].angle per query
    const uint8_t* q_blocks;  // "the query's map point has Observations() > 0" (:91-93, :1397-1399); NULL = all
    float factor;             // rotation histogram factor (:1341)
    int check_ori;
    int32_t* match_cur;       // n entries
    int32_t* qbin;            // nq entries of scratch
    // any mode: the reprojection gate of Fuse (ORBmatcher.cc:925-931): skip a candidate when e2 * inv_sigma2[level] > chi2
    double chi2;              // 0 = no gate
    const float* inv_sigma2;  // 16 entries (the kernel argument's: a copy here would live in scratch)
};

__device__ __forceinline__ void sbp_frame(
    const orbfe_keypoint* __restrict__ kps, const uint8_t* __restrict__ desc, int n, int ncap /*pow2 >= n*/, float4 bnd,
    const SbpQuery* __restrict__ queries, const uint8_t* __restrict__ qdesc, int nq, uint8_t* __restrict__ taken, int mode,
    int th_high, float nnratio, uint16_t* __restrict__ row_rank, uint8_t* __restrict__ row_dist, int32_t* __restrict__ row_cnt,
    int row_stride, int32_t* __restrict__ best_idx, int32_t* __restrict__ best_dist, int32_t* __restrict__ best_level,
    int32_t* __restrict__ second_dist, int32_t* __restrict__ second_level, int32_t* __restrict__ match,
    int32_t* __restrict__ nmatches_out, int32_t* __restrict__ overflow, SbpBest bo)
{
    extern __shared__ __align__(16) unsigned char sbp_smem[];
    __shared__ int s_nin;
    __shared__ int s_hist[30];
    const SbpLdsOffsets lo = sbp_lds_offsets(ncap);            // the layout sbp_launch sized (match_plan.hpp)
    uint32_t* s_sorted = (uint32_t*)(sbp_smem + lo.sorted);    // (cell << 16) | index, ascending; ncap entries
    float2* s_xy = (float2*)(sbp_smem + lo.xy);                // by rank
    uint16_t* s_cell0 = (uint16_t*)(sbp_smem + lo.cell0);      // first rank of every cell, SBP_CELLS + 1 entries
    uint8_t* s_lvl = sbp_smem + lo.lvl;                        // by rank
    uint8_t* s_taken = sbp_smem + lo.taken;                    // by rank
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // bounds of the undistorted image (Frame::ComputeImageBounds; 0, 0, cols, rows without distortion) and Frame.cc:112-113
    const float mnMinX = bnd.x, mnMinY = bnd.y;
    const float invW = __fdiv_rn((float)GRID_COLS, bnd.z - bnd.x);
    const float invH = __fdiv_rn((float)GRID_ROWS, bnd.w - bnd.y);

    // ---- A
    if (tid == 0) s_nin = 0;
    if (tid < 30) s_hist[tid] = 0;
    if (mode == 2)
        for (int i = tid; i < n; i += SBP_THREADS) bo.match_cur[i] = -1;
    __syncthreads();
    for (int i = tid; i < n; i += SBP_THREADS) {
        const orbfe_keypoint kp = kps[i];
        const int px = (int)roundf(__fmul_rn(kp.x - mnMinX, invW));
        const int py = (int)roundf(__fmul_rn(kp.y - mnMinY, invH));
        if (px >= 0 && px < GRID_COLS && py >= 0 && py < GRID_ROWS) {
            const int k = atomicAdd(&s_nin, 1);
            s_sorted[k] = ((uint32_t)(px * GRID_ROWS + py) << 16) | (uint32_t)i;
        }
    }
    __syncthreads();
    const int nin = s_nin;
    {
        int P = 1;
        while (P < nin) P <<= 1;
        for (int i = nin + tid; i < P; i += SBP_THREADS) s_sorted[i] = 0xffffffffu;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (P >> 1); t += SBP_THREADS) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    const int l = i | j;
                    const uint32_t a = s_sorted[i], b = s_sorted[l];
                    const bool up = ((i & k) == 0);
                    if ((a > b) == up) { s_sorted[i] = b; s_sorted[l] = a; }
                }
                __syncthreads();
            }
    }
    for (int c = tid; c <= SBP_CELLS; c += SBP_THREADS) { // lower bound of (c << 16)
        const uint32_t key = (uint32_t)c << 16;
        int lo = 0, hi = nin;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_sorted[mid] < key) lo = mid + 1; else hi = mid;
        }
        s_cell0[c] = (uint16_t)lo;
    }
    for (int i = tid; i < nin; i += SBP_THREADS) {
        const int idx = s_sorted[i] & 0xffff;
        const orbfe_keypoint kp = kps[idx];
        s_xy[i] = make_float2(kp.x, kp.y);
        s_lvl[i] = (uint8_t)kp.octave;
        s_taken[i] = taken ? taken[idx] : 0;
    }
    __syncthreads();

    // ---- B
    for (int q = wid; q < nq; q += SBP_THREADS / 64) {
        const SbpQuery Q = queries[q];
        const float x = Q.x, y = Q.y, r = Q.r;
        int count = 0;
        const int nMinCellX = max(0, (int)floorf(__fmul_rn(x - mnMinX - r, invW)));
        const int nMaxCellX = min(GRID_COLS - 1, (int)ceilf(__fmul_rn(x - mnMinX + r, invW)));
        const int nMinCellY = max(0, (int)floorf(__fmul_rn(y - mnMinY - r, invH)));
        const int nMaxCellY = min(GRID_ROWS - 1, (int)ceilf(__fmul_rn(y - mnMinY + r, invH)));
        if (!(r < 0.0f) && !(nMinCellX >= GRID_COLS || nMaxCellX < 0 || nMinCellY >= GRID_ROWS || nMaxCellY < 0)) {
            const bool check_levels = (Q.min_level > 0) || (Q.max_level >= 0);
            const uint4 a0 = reinterpret_cast<const uint4*>(qdesc)[2 * q];
            const uint4 a1 = reinterpret_cast<const uint4*>(qdesc)[2 * q + 1];
            uint16_t* rr = row_rank + (size_t)q * row_stride;
            uint8_t* rd = row_dist + (size_t)q * row_stride;
            for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
                const int j_begin = s_cell0[ix * GRID_ROWS + nMinCellY], j_end = s_cell0[ix * GRID_ROWS + nMaxCellY + 1];
                for (int j0 = j_begin; j0 < j_end; j0 += 64) {
                    const int j = j0 + lane;
                    bool ok = false;
                    if (j < j_end) {
                        const int lv = s_lvl[j];
                        ok = !check_levels || (lv >= Q.min_level && (Q.max_level < 0 || lv <= Q.max_level));
                        if (ok) {
                            const float2 p = s_xy[j];
                            ok = fabsf(p.x - x) < r && fabsf(p.y - y) < r;
                            if (ok && bo.chi2 > 0.0) {
                                const float ex = x - p.x, ey = y - p.y;
                                const float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
                                ok = !((double)__fmul_rn(e2, bo.inv_sigma2[min(lv, 15)]) > bo.chi2);
                            }
                        }
                    }
                    const unsigned long long m = __ballot(ok);
                    if (ok) {
                        const int pos = count + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
                        if (pos < row_stride) {
                            const int i2 = s_sorted[j] & 0xffff;
                            const uint4 b0 = reinterpret_cast<const uint4*>(desc)[2 * i2];
                            const uint4 b1 = reinterpret_cast<const uint4*>(desc)[2 * i2 + 1];
                            const int d = hamming256(a0, a1, b0, b1);
                            rr[pos] = (uint16_t)j;
                            rd[pos] = (uint8_t)(d > 255 ? 255 : d); // 256 only for exact complements: never accepted
                        }
                    }
                    count += __popcll(m);
                }
            }
        }
        if (lane == 0) {
            if (count > row_stride) atomicMax(overflow, count);
            row_cnt[q] = min(count, row_stride);
        }
    }
    __threadfence_block();
    __syncthreads();

    // ---- C: best / second-best over a row; returns keys (d << 32 | position << 16 | rank), ~0 = none
    auto resolve = [&](int q, unsigned long long& bestk, unsigned long long& secondk) {
        const int e = row_cnt[q];
        const uint16_t* rr = row_rank + (size_t)q * row_stride;
        const uint8_t* rd = row_dist + (size_t)q * row_stride;
        bestk = ~0ull; secondk = ~0ull;
        for (int j0 = 0; j0 < e; j0 += 64) {
            const int j = j0 + lane;
            unsigned long long key = ~0ull;
            if (j < e) {
                const int rk = rr[j];
                if (!s_taken[rk]) key = ((unsigned long long)rd[j] << 32) | ((unsigned long long)j << 16) | (unsigned)rk;
            }
            const unsigned long long m1 = wave_min_u64(key);
            const unsigned long long k2 = wave_min_u64(key == m1 ? ~0ull : key);
            if (m1 < bestk) { secondk = min(bestk, k2); bestk = m1; }
            else secondk = min(secondk, m1);
        }
    };
    auto write_raw = [&](int q, unsigned long long bestk, unsigned long long secondk) {
        if (lane == 0 && best_idx) {
            const bool hb = bestk != ~0ull, hs = secondk != ~0ull;
            best_idx[q] = hb ? (int)(s_sorted[bestk & 0xffff] & 0xffff) : -1;
            best_dist[q] = hb ? (int)(bestk >> 32) : 256;
            best_level[q] = hb ? (int)s_lvl[bestk & 0xffff] : -1;
            second_dist[q] = hs ? (int)(secondk >> 32) : 256;
            second_level[q] = hs ? (int)s_lvl[secondk & 0xffff] : -1;
        }
    };
    if (mode == 0) {
        for (int q = wid; q < nq; q += SBP_THREADS / 64) {
            unsigned long long bk, sk;
            resolve(q, bk, sk);
            write_raw(q, bk, sk);
        }
        return;
    }
    if (wid != 0) return;
    int nmatches = 0;
    if (mode == 2) {
        for (int q = 0; q < nq; q++) {
            unsigned long long bk, sk;
            resolve(q, bk, sk);
            write_raw(q, bk, sk);
            int m = -1, bin = -1;
            if (bk != ~0ull && (int)(bk >> 32) <= th_high) { // :1421
                const int bestRank = (int)(bk & 0xffff);
                m = (int)(s_sorted[bestRank] & 0xffff);
                if (bo.check_ori) {
                    float rot = bo.q_angle[q] - kps[m].angle;
                    if (rot < 0.0f) rot += 360.0f;
                    bin = (int)roundf(__fmul_rn(rot, bo.factor));
                    if (bin == 30) bin = 0;
                    bin = min(max(bin, 0), 29);
                }
                if (lane == 0) {
                    bo.match_cur[m] = q; // CurrentFrame.mvpMapPoints[bestIdx2] = pMP (:1423)
                    if (!bo.q_blocks || bo.q_blocks[q]) { s_taken[bestRank] = 1; if (taken) taken[m] = 1; }
                }
                nmatches++;
            }
            if (lane == 0) { match[q] = m; bo.qbin[q] = bin; }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        if (bo.check_ori) { // :1440-1471: every push_back counts, also for a keypoint that was assigned twice
            __threadfence_block();
            for (int q = lane; q < nq; q += 64)
                if (match[q] >= 0) atomicAdd(&s_hist[bo.qbin[q]], 1);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            int ind1 = -1, ind2 = -1, ind3 = -1, max1 = 0, max2 = 0, max3 = 0;
            for (int i = 0; i < 30; i++) { // ComputeThreeMaxima, ORBmatcher.cc:1605-1646
                const int sz = s_hist[i];
                if (sz > max1) { max3 = max2; max2 = max1; max1 = sz; ind3 = ind2; ind2 = ind1; ind1 = i; }
                else if (sz > max2) { max3 = max2; max2 = sz; ind3 = ind2; ind2 = i; }
                else if (sz > max3) { max3 = sz; ind3 = i; }
            }
            if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
            else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
            int removed = 0;
            for (int q0 = 0; q0 < nq; q0 += 64) {
                const int q = q0 + lane;
                bool rm = false;
                if (q < nq && match[q] >= 0) {
                    const int bin = bo.qbin[q];
                    rm = bin != ind1 && bin != ind2 && bin != ind3;
                    if (rm) bo.match_cur[match[q]] = -1;
                }
                removed += __popcll(__ballot(rm));
            }
            nmatches -= removed;
        }
        if (lane == 0) *nmatches_out = nmatches;
        return;
    }
    for (int q = 0; q < nq; q++) {
        unsigned long long bk, sk;
        resolve(q, bk, sk);
        write_raw(q, bk, sk);
        int m = -1;
        if (bk != ~0ull) {
            const int bestDist = (int)(bk >> 32), bestRank = (int)(bk & 0xffff);
            // a second-best of 256 (none) has level -1, which never equals the best's level
            const int bestDist2 = sk != ~0ull ? (int)(sk >> 32) : 256;
            const int bestLevel = s_lvl[bestRank], bestLevel2 = sk != ~0ull ? (int)s_lvl[sk & 0xffff] : -1;
            if (bestDist <= th_high && !(bestLevel == bestLevel2 && (float)bestDist > __fmul_rn(nnratio, (float)bestDist2))) {
                m = (int)(s_sorted[bestRank] & 0xffff);
                // the keypoint blocks later queries only if the map point it received is observed (:91-93)
                if (lane == 0 && (!bo.q_blocks || bo.q_blocks[q])) { s_taken[bestRank] = 1; if (taken) taken[m] = 1; }
                nmatches++;
            }
        }
        if (lane == 0) match[q] = m;
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) *nmatches_out = nmatches;
}

// The search over the frames of a batch resident on the device: workgroup f = frame f of blocks of `capacity` keypoint
// records and `qcapacity` query records (the layouts of orbfe_extract_batch_device).  n / nq NULL: every frame holds `capacity`
// keypoints / `qcapacity` queries (the host-pointer searches: one frame whose counts are known on the host).
struct SbpBatch {
    const orbfe_keypoint* kps; const uint8_t* desc; const int32_t* n; int capacity;
    const SbpQuery* queries; const uint8_t* qdesc; const int32_t* nq; int qcapacity;
    uint8_t* taken; const uint8_t* q_observed; const float* q_angle;
    uint16_t* row_rank; uint8_t* row_dist; int32_t* row_cnt; int row_stride;
    int32_t *best_idx, *best_dist, *best_level, *second_dist, *second_level, *match, *nmatches, *overflow;
    int32_t *match_cur, *qbin;
    int qdesc_shared;     // every frame's queries use the same descriptor block (the same map points into several keyframes: Fuse)
    double chi2;          // > 0: reprojection gate of Fuse (SbpBest::chi2)
    float inv_sigma2[16];
};
__global__ __launch_bounds__(SBP_THREADS) void k_search_by_projection_batch(SbpBatch B, int ncap, float4 bnd, int mode, int th_high,
                                                                            float nnratio, float factor, int check_ori)
{
    const size_t f = blockIdx.x, ko = f * B.capacity, qo = f * B.qcapacity;
    const int n = B.n ? min(B.n[f], B.capacity) : B.capacity, nq = B.nq ? min(B.nq[f], B.qcapacity) : B.qcapacity;
    SbpBest bo{};
    bo.q_angle = B.q_angle ? B.q_angle + qo : nullptr;
    bo.q_blocks = B.q_observed ? B.q_observed + qo : nullptr;
    bo.factor = factor; bo.check_ori = check_ori;
    bo.match_cur = B.match_cur ? B.match_cur + ko : nullptr;
    bo.qbin = B.qbin ? B.qbin + qo : nullptr;
    bo.chi2 = B.chi2;
    bo.inv_sigma2 = B.inv_sigma2;
    sbp_frame(B.kps + ko, B.desc + ko * 32, n, ncap, bnd, B.queries + qo, B.qdesc + (B.qdesc_shared ? 0 : qo * 32), nq, B.taken ? B.taken + ko : nullptr, mode, th_high,
              nnratio, B.row_rank + qo * B.row_stride, B.row_dist + qo * B.row_stride, B.row_cnt + qo, B.row_stride,
              B.best_idx ? B.best_idx + qo : nullptr, B.best_dist ? B.best_dist + qo : nullptr, B.best_level ? B.best_level + qo : nullptr,
              B.second_dist ? B.second_dist + qo : nullptr, B.second_level ? B.second_level + qo : nullptr, B.match + qo, B.nmatches + f,
              B.overflow, bo);
}

// ---------------------------------------------------------------------------------------------------------------------
// Frame glue: cv::undistortPoints with P = K (Frame.cc:357-451).  One point per lane, double arithmetic
// (orbfe_undistort_point in include/orbfe_math.h is the numerics contract); the 12 coefficients come by value.
struct UndistortParams {
    double fx, fy, cx, cy;
    double k[12];
};

// points: n (x, y) float pairs, src -> dst (may alias)
__global__ __launch_bounds__(256) void k_undistort_points(const float2* __restrict__ src, int n, UndistortParams P,
                                                          float2* __restrict__ dst)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float2 p = src[i];
    float2 o;
    orbfe_undistort_point(p.x, p.y, P.fx, P.fy, P.cx, P.cy, P.k, &o.x, &o.y);
    dst[i] = o;
}

// keypoint records of a batch: frame = blockIdx.y, in place on (x, y) (mvKeysUn keeps the other fields, Frame.cc:379-386)
__global__ __launch_bounds__(256) void k_undistort_keypoints(const orbfe_keypoint* __restrict__ kin, const int32_t* __restrict__ d_n,
                                                             int capacity, UndistortParams P, orbfe_keypoint* __restrict__ kout)
{
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= min(d_n[f], capacity)) return;
    orbfe_keypoint kp = kin[(size_t)f * capacity + i];
    orbfe_undistort_point(kp.x, kp.y, P.fx, P.fy, P.cx, P.cy, P.k, &kp.x, &kp.y);
    kout[(size_t)f * capacity + i] = kp;
}

static int undistort_params(const float* K4, const float* dist, int ndist, UndistortParams& P, const char* who)
{
    if (!K4 || ndist < 0 || ndist > 12 || (ndist && !dist) || !(K4[0] != 0.0f) || !(K4[1] != 0.0f))
        return fail(ORBFE_ERR_INVALID, "%s: invalid camera (K = {fx, fy, cx, cy} with fx, fy != 0; at most 12 coefficients)", who);
    P.fx = K4[0]; P.fy = K4[1]; P.cx = K4[2]; P.cy = K4[3];
    for (int i = 0; i < 12; i++) P.k[i] = i < ndist ? (double)dist[i] : 0.0;
    return ORBFE_OK;
}

// The projection of SearchByProjection(CurrentFrame, LastFrame) (ORBmatcher.cc:1362-1389): one lane per feature of the last
// frame.  x3Dc = Rcw * x3Dw + tcw is OpenCV's 3x3 float product (a row is summed left to right in float) plus the float
// translation; invzc is a double division rounded to float (:1371).  A query that is skipped gets r = -1.
__global__ __launch_bounds__(256) void k_project_last_frame(const float* __restrict__ x3Dw, const uint8_t* __restrict__ valid,
                                                            const orbfe_keypoint* __restrict__ kps_last, int n, const float* __restrict__ Tcw,
                                                            float4 K, float4 bnd, const float* __restrict__ scale, int nlevels, float th,
                                                            SbpQuery* __restrict__ queries, float* __restrict__ q_angle)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    SbpQuery Q{0.0f, 0.0f, -1.0f, 0, 0};
    const orbfe_keypoint kp = kps_last[i];
    q_angle[i] = kp.angle;
    if (!valid || valid[i]) {
        const float X = x3Dw[3 * i], Y = x3Dw[3 * i + 1], Z = x3Dw[3 * i + 2];
        const float xc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(Tcw[0], X), __fmul_rn(Tcw[1], Y)), __fmul_rn(Tcw[2], Z)), Tcw[3]);
        const float yc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(Tcw[4], X), __fmul_rn(Tcw[5], Y)), __fmul_rn(Tcw[6], Z)), Tcw[7]);
        const float zc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(Tcw[8], X), __fmul_rn(Tcw[9], Y)), __fmul_rn(Tcw[10], Z)), Tcw[11]);
        const float invzc = (float)(1.0 / (double)zc);
        if (!(invzc < 0)) {
            const float u = __fadd_rn(__fmul_rn(__fmul_rn(K.x, xc), invzc), K.z);
            const float v = __fadd_rn(__fmul_rn(__fmul_rn(K.y, yc), invzc), K.w);
            // NaN coordinates (zc == 0 with xc == 0) are dropped here; the reference would index the grid with them
            if (u >= bnd.x && u <= bnd.z && v >= bnd.y && v <= bnd.w) {
                const int oct = min(max(kp.octave, 0), nlevels - 1);
                Q = SbpQuery{u, v, __fmul_rn(th, scale[oct]), kp.octave - 1, kp.octave + 1}; // mono: :1396
            }
        }
    }
    queries[i] = Q;
}

// The projection and visibility gates shared by Fuse (ORBmatcher.cc:848-893 and :1008-1049) and the keyframe variants of
// SearchByProjection (:321-358, :1497-1530): camera coordinates (OpenCV's 3x3 float product + float translation), positive
// depth, inside the image, distance inside the scale-invariance range [0.8f * mfMinDistance, 1.2f * mfMaxDistance]
// (MapPoint::Get{Min,Max}DistanceInvariance, MapPoint.cc:402-412), optional viewing-angle gate (P - Ow) . n >= 0.5 d
// (cv::Mat::dot and cv::norm accumulate in double), MapPoint::PredictScale (MapPoint.cc:414-446: mfMaxDistance / dist, and --
// TemplatedVocabulary.h:36 puts `using namespace std` in front of MapPoint.cc -- std::log(float), float division, std::ceil(float);
// the float log here is the correctly rounded one), search radius th * scale[level].  One lane per map point; a point that is
// not searched gets r = -1.
// frame_variant: the relocalisation search SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) projects with other
// arithmetic (:1503-1512): NO depth gate, invzc = 1.0 / zc evaluated in double, u = (fx * xc) * invzc + cx, Frame bounds (<=).
struct ProjectParams {
    float T[12], Ow[3], K[4], bnd[4], scale[16];
    int nlevels, strict_max, level_below, level_above;
    float log_scale, th;
    // SearchBySim3 (ORBmatcher.cc:1158-1159, :1238-1239): a second transform applied to the camera coordinates of the first, each
    // stage rounded to float as the two cv::Mat expressions are; the distance is then the norm of the final camera coordinates
    int use_T2;
    float T2[12];
    int frame_variant;
};

__global__ __launch_bounds__(256) void k_project_map_points(const float* __restrict__ p3Dw, const uint8_t* __restrict__ valid,
                                                            const float* __restrict__ min_dist, const float* __restrict__ max_dist,
                                                            const float* __restrict__ normal, int n, ProjectParams P,
                                                            SbpQuery* __restrict__ queries)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    SbpQuery Q{0.0f, 0.0f, -1.0f, 0, 0};
    if (!valid || valid[i]) {
        const float X = p3Dw[3 * i], Y = p3Dw[3 * i + 1], Z = p3Dw[3 * i + 2];
        float xc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(P.T[0], X), __fmul_rn(P.T[1], Y)), __fmul_rn(P.T[2], Z)), P.T[3]);
        float yc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(P.T[4], X), __fmul_rn(P.T[5], Y)), __fmul_rn(P.T[6], Z)), P.T[7]);
        float zc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(P.T[8], X), __fmul_rn(P.T[9], Y)), __fmul_rn(P.T[10], Z)), P.T[11]);
        if (P.use_T2) {
            const float a = xc, b = yc, c = zc;
            xc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(P.T2[0], a), __fmul_rn(P.T2[1], b)), __fmul_rn(P.T2[2], c)), P.T2[3]);
            yc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(P.T2[4], a), __fmul_rn(P.T2[5], b)), __fmul_rn(P.T2[6], c)), P.T2[7]);
            zc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(P.T2[8], a), __fmul_rn(P.T2[9], b)), __fmul_rn(P.T2[10], c)), P.T2[11]);
        }
        float u = 0.0f, v = 0.0f;
        bool inside = false;
        if (P.frame_variant) {
            const float invzc = (float)(1.0 / (double)zc);
            u = __fadd_rn(__fmul_rn(__fmul_rn(P.K[0], xc), invzc), P.K[2]);
            v = __fadd_rn(__fmul_rn(__fmul_rn(P.K[1], yc), invzc), P.K[3]);
            // NaN coordinates (zc == 0 with xc == 0) fail every comparison and are dropped; the reference would index the grid with them
            inside = u >= P.bnd[0] && u <= P.bnd[2] && v >= P.bnd[1] && v <= P.bnd[3];
        } else if (!(zc < 0.0f)) {
            const float invz = __fdiv_rn(1.0f, zc);
            u = __fadd_rn(__fmul_rn(P.K[0], __fmul_rn(xc, invz)), P.K[2]);
            v = __fadd_rn(__fmul_rn(P.K[1], __fmul_rn(yc, invz)), P.K[3]);
            inside = P.strict_max ? (u >= P.bnd[0] && u < P.bnd[2] && v >= P.bnd[1] && v < P.bnd[3])  // KeyFrame::IsInImage
                                  : (u >= P.bnd[0] && u <= P.bnd[2] && v >= P.bnd[1] && v <= P.bnd[3]);
        }
        if (inside) {
            const float px = P.use_T2 ? xc : X - P.Ow[0], py = P.use_T2 ? yc : Y - P.Ow[1], pz = P.use_T2 ? zc : Z - P.Ow[2];
            const float dist3D = (float)sqrt((double)px * px + (double)py * py + (double)pz * pz);
            const float mfMax = max_dist[i];
            bool ok = !(dist3D < __fmul_rn(0.8f, min_dist[i]) || dist3D > __fmul_rn(1.2f, mfMax));
            if (ok && normal) {
                const double dot = (double)px * normal[3 * i] + (double)py * normal[3 * i + 1] + (double)pz * normal[3 * i + 2];
                ok = !(dot < 0.5 * (double)dist3D);
            }
            if (ok) {
                const float ratio = __fdiv_rn(mfMax, dist3D);
                int lvl = (int)ceilf(__fdiv_rn((float)log((double)ratio), P.log_scale));
                if (lvl < 0) lvl = 0;
                else if (lvl >= P.nlevels) lvl = P.nlevels - 1;
                Q = SbpQuery{u, v, __fmul_rn(P.th, P.scale[lvl]), lvl - P.level_below, lvl + P.level_above};
            }
        }
    }
    queries[i] = Q;
}

// ---------------------------------------------------------------------------------------------------------------------
// MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:270-333): among the N descriptors a map point was observed with,
// the one with the least MEDIAN Hamming distance to the others -- median = sorted row[(int)(0.5 * (N - 1))], the first row wins
// ties (`median < BestMedian`).  One wave per map point, N <= 256: lane l keeps descriptors l, l + 64, l + 128, l + 192 in
// registers; row i's descriptor comes by v_readlane from the lane that owns it; the k-th smallest of a row's distances (all in
// 0 .. 256) is found by bisection on the VALUE with one ballot + popcount per chunk and step -- no sort, no LDS.
#define DD_MAXN 256
__global__ __launch_bounds__(256) void k_distinctive(const uint8_t* __restrict__ desc, const int32_t* __restrict__ offsets, int npoints,
                                                     int32_t* __restrict__ best_idx, uint8_t* __restrict__ best_desc)
{
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= npoints) return;
    const int o0 = offsets[p], N = min(offsets[p + 1] - o0, DD_MAXN);
    if (N <= 0) {
        if (lane == 0) best_idx[p] = -1;
        return;
    }
    const uint4* D = reinterpret_cast<const uint4*>(desc) + (size_t)o0 * 2;
    uint32_t w[4][8];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int j = lane + 64 * c;
        uint4 a = make_uint4(0, 0, 0, 0), b = a;
        if (j < N) { a = D[2 * j]; b = D[2 * j + 1]; }
        w[c][0] = a.x; w[c][1] = a.y; w[c][2] = a.z; w[c][3] = a.w; w[c][4] = b.x; w[c][5] = b.y; w[c][6] = b.z; w[c][7] = b.w;
    }
    const int k = (int)(0.5 * (double)(N - 1)); // index of the median in the sorted row
    int best_median = 0x7fffffff, best = 0;
    for (int i = 0; i < N; i++) {
        uint32_t r[8];
        const int src_lane = i & 63, src_c = i >> 6;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const uint32_t v = src_c == 0 ? w[0][q] : src_c == 1 ? w[1][q] : src_c == 2 ? w[2][q] : w[3][q];
            r[q] = (uint32_t)__builtin_amdgcn_readlane((int)v, src_lane);
        }
        int d[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            int s_ = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) s_ += __popc(w[c][q] ^ r[q]);
            d[c] = s_;
        }
        int lo = 0, hi = 256; // smallest m with #(d <= m) >= k + 1
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            int cnt = 0;
#pragma unroll
            for (int c = 0; c < 4; c++) cnt += __popcll(__ballot(lane + 64 * c < N && d[c] <= mid));
            if (cnt >= k + 1) hi = mid; else lo = mid + 1;
        }
        if (lo < best_median) { best_median = lo; best = i; }
    }
    if (lane == 0) best_idx[p] = best;
    if (best_desc && lane < 8) reinterpret_cast<uint32_t*>(best_desc)[(size_t)p * 8 + lane] = reinterpret_cast<const uint32_t*>(D)[(size_t)best * 8 + lane];
}

// The kernels' scratch: the partials of knn2_launch, the grid records and pools of sfi_launch, the rows of sbp_launch.
struct MatchWorkspace {
    DevBuf pidx, pbest, psecond, csr_cnt, csr_idx, csr_dist, scratch;
    DevBuf sbp_batch_overflow; // flag of the _batch_device searches: sticky until orbfe_search_by_projection_batch_status reads it
    DevBuf sfi_overflow;  // SearchForInitialization's two flag words: zeroed when allocated and whenever they are read (no memset launch per batch)
    DevBuf q, obest;      // orbfe_fuse_search_batch_device: the projected queries, the result arrays nobody asked for
    int csr_per_pair = 0; // candidate pool entries per frame pair of SearchForInitialization (grown on overflow)
    int sbp_stride = 0;   // candidate row stride of k_search_by_projection_batch (grown on overflow)
};
// one workspace per (thread, device, stream): see ThreadWorkspaces.  A _batch_device call takes the one of the caller's stream, a
// host-pointer call the one of its stage's stream, so the two never share buffers, pool size or row stride.
static thread_local ThreadWorkspaces<MatchWorkspace> tl_ws;
static MatchWorkspace& ws(hipStream_t s) { return tl_ws.get(s); }
// the stage of the host-pointer calls of this file, bow_vocabulary.hip and keyframe_io.hip (host_stage.hpp)
static thread_local ThreadWorkspaces<HostStage> tl_stage;
HostStage& match_host_stage() { return tl_stage.get(); }
// a capacity flag that is zeroed once, when it is allocated, and again only by the status call that reads it
static int ensure_sticky_flag(DevBuf& b)
{
    if (b.p) return ORBFE_OK;
    int rc = b.ensure(16);
    if (rc) return rc;
    ORBFE_HIP(hipMemset(b.p, 0, 16));
    return ORBFE_OK;
}

// orbfe_debug_control sets them
static MatchSwitches g_match_switches;
#ifdef ORBFE_ABLATION
int g_orb_skip = 0, g_aruco_skip = 0;
#endif

static int knn2_launch(const uint8_t* d_Q, const int32_t* d_nq, size_t q_stride, int max_nq, const uint8_t* d_T,
                       const int32_t* d_nt, size_t t_stride, int max_nt, int npairs, int init, int32_t* d_best_idx,
                       int32_t* d_best_dist, int32_t* d_second_dist, hipStream_t s)
{
    const Knn2Plan p = plan_knn2(max_nq, max_nt, npairs, init, g_match_switches);
    // with one split the scan writes the caller's arrays; the partials of more are merged in split order
    int32_t *o_idx = d_best_idx, *o_best = d_best_dist, *o_second = d_second_dist;
    if (p.nsplit > 1) {
        MatchWorkspace& w = ws(s);
        int rc;
        if ((rc = w.pidx.ensure(p.part_bytes)) || (rc = w.pbest.ensure(p.part_bytes)) || (rc = w.psecond.ensure(p.part_bytes))) return rc;
        o_idx = w.pidx.as<int32_t>(); o_best = w.pbest.as<int32_t>(); o_second = w.psecond.as<int32_t>();
    }
    const auto k_scan = p.mfma ? k_knn2_mfma : k_knn2_tiles;
    hipLaunchKernelGGL(k_scan, dim3(p.scan.x, p.scan.y, p.scan.z), dim3(p.scan_block), 0, s, d_Q, d_nq, q_stride, max_nq, d_T, d_nt, t_stride,
                       p.chunk, init, o_idx, o_best, o_second);
    if (p.nsplit > 1)
        hipLaunchKernelGGL(k_knn2_merge, dim3(p.merge.x, p.merge.y), dim3(KNN_TILE), 0, s, o_idx, o_best, o_second, p.nsplit, max_nq, d_nq,
                           d_best_idx, d_best_dist, d_second_dist);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

static float4 frame_bounds(int cols, int rows, const float* bounds)
{
    return bounds ? make_float4(bounds[0], bounds[1], bounds[2], bounds[3]) : make_float4(0.f, 0.f, (float)cols, (float)rows);
}

static int sfi_launch(const orbfe_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int capacity, int npairs,
                      float4 bnd, int window, float nnratio, int check_ori, const float* d_prev_in,
                      float* d_prev_out, int32_t* d_m12, int32_t* d_nm, hipStream_t s, MatchWorkspace& w)
{
    if (capacity > 65535) return fail(ORBFE_ERR_INVALID, "capacity above 65535 keypoints per frame is unsupported");
    const SfiLayout l = plan_sfi(npairs, w.csr_per_pair);   // sizes and carves the grid records and the pairs' candidate pools
    const int pool_cap = w.csr_per_pair = l.pool, nframes = l.nframes;
    int rc;
    if ((rc = w.csr_cnt.ensure(l.cnt_bytes)) || (rc = w.csr_idx.ensure(l.idx_bytes)) || (rc = w.csr_dist.ensure(l.dist_bytes)) ||
        (rc = w.scratch.ensure(l.scratch_bytes)))
        return rc;
    if ((rc = ensure_sticky_flag(w.sfi_overflow))) return rc;
    SfiGrid G;
    int32_t* cnt = w.csr_cnt.as<int32_t>();
    G.nl0 = cnt + l.nl0; G.nq = cnt + l.nq; G.cursor = cnt + l.cursor;
    uint8_t* b = w.csr_idx.as<uint8_t>();
    G.desc = reinterpret_cast<uint4*>(b + l.desc);
    G.xy = reinterpret_cast<float2*>(b + l.xy);
    G.sorted = reinterpret_cast<uint32_t*>(b + l.sorted);
    G.qxy = reinterpret_cast<float2*>(b + l.qxy);
    G.ang = reinterpret_cast<float*>(b + l.ang);
    G.query = reinterpret_cast<uint16_t*>(b + l.query);
    int32_t* ovf = w.sfi_overflow.as<int32_t>(); // [0]: level-0 keypoints beyond SFI_MAXL0, [1]: pool entries a pair needed
    hipLaunchKernelGGL(k_sfi_grid, dim3(nframes), dim3(SFI_GRID_THREADS), 0, s, d_kps, d_desc, d_n, capacity, nframes, bnd, G, ovf);
    // a wave per query for frames of up to 256 level-0 keypoints (ORB-SLAM's 1000 features at 640 x 480 have ~217), more per wave above
    hipLaunchKernelGGL(k_sfi_rows, dim3(SFI_ROWS_BX, npairs), dim3(SFI_ROWS_WAVES * 64), 0, s, d_kps, d_desc, capacity, bnd, (float)window, d_prev_in, G,
                       w.csr_dist.as<uint32_t>(), pool_cap, w.scratch.as<uint32_t>(), ovf);
    hipLaunchKernelGGL(k_sfi_accept, dim3(npairs), dim3(64), 0, s, d_kps, d_n, capacity, nnratio, check_ori, d_prev_in, d_prev_out, d_m12,
                       d_nm, G, w.csr_dist.as<uint32_t>(), pool_cap, w.scratch.as<uint32_t>());
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

// takes the two flag words f, read after stream s has drained, and clears them behind it; *need = 0, the level-0 count that does not
// fit (an error), or the pool size a pair needed (the pool is grown: repeat the call)
static int sfi_take_flags(MatchWorkspace& w, const int32_t* f, hipStream_t s, int32_t* need)
{
    const SfiFlagsDecision d = sfi_flags_decision(f[0], f[1], w.csr_per_pair);
    if (d.clear) ORBFE_HIP(hipMemsetAsync(w.sfi_overflow.p, 0, 8, s)); // sticky until read
    w.csr_per_pair = d.pool; // the next batch on this stream has the room
    *need = d.need;
    if (d.err) return fail(d.err, "%d level-0 keypoints in a frame exceed the supported %d", d.need, SFI_MAXL0);
    return ORBFE_OK;
}

// Every projection search is this launch: nframes workgroups over B, whose candidate rows (row_*) it sizes at the workspace's
// stride.  A frame's grid lives in LDS, sized by the keypoint capacity.
static int sbp_launch(MatchWorkspace& w, SbpBatch B, int nframes, float4 bnd, int mode, int th_high, float nnratio, float factor,
                      int check_ori, hipStream_t s)
{
    const SbpLayout l = plan_sbp(B.capacity, B.qcapacity, nframes, w.sbp_stride);
    if (l.err) return fail(l.err, "%s", l.msg);
    w.sbp_stride = l.stride;
    int rc;
    if ((rc = w.csr_idx.ensure(l.rank_bytes)) || (rc = w.csr_dist.ensure(l.dist_bytes)) || (rc = w.csr_cnt.ensure(l.cnt_bytes)) ||
        (rc = ensure_dyn_lds(reinterpret_cast<const void*>(&k_search_by_projection_batch), l.lds_bytes)))
        return rc;
    B.row_rank = w.csr_idx.as<uint16_t>(); B.row_dist = w.csr_dist.as<uint8_t>(); B.row_cnt = w.csr_cnt.as<int32_t>(); B.row_stride = l.stride;
    hipLaunchKernelGGL(k_search_by_projection_batch, dim3(nframes), dim3(SBP_THREADS), l.lds_bytes, s, B, l.ncap, bnd, mode, th_high, nnratio,
                       factor, check_ori);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

// One host-pointer search of one frame (orbfe_search_by_projection and the entry points after it).  Host arrays: a NULL input is
// absent, a NULL output is not copied back.
struct SbpHostCall {
    const orbfe_keypoint* kps; const uint8_t* desc; int n; float4 bnd;
    const uint8_t* taken;          // the frame's taken flags
    int nq; const uint8_t* qdesc; const uint8_t* q_observed; const float* q_angle;
    // the queries: the caller's windows, or map points x3Dw (valid: which exist) projected on the device by k_project_last_frame
    // (kps_last != NULL, whose angles become q_angle) or by k_project_map_points (P != NULL)
    const orbfe_window_query* window;
    const float* x3Dw; const uint8_t* valid;
    const orbfe_keypoint* kps_last; const float* Tcw; const float* K4; const float* scale; int nlevels; float th;
    const ProjectParams* P; const float* min_dist; const float* max_dist; const float* normal;
    int mode, th_high; float nnratio, factor; int check_ori;
    double chi2; const float* inv_sigma2; // Fuse's gate: chi2 > 0, nlevels entries
    int32_t *best_idx, *best_dist, *best_level, *second_dist, *second_level, *match, *match_cur, *nmatches;
    uint8_t* taken_out;            // the taken flags after the search
};

// stages the call in the matcher's stage, builds or uploads the queries, searches and fetches the results: one upload, the kernels,
// one download, one synchronisation.  The taken flags and the two count words travel both ways: a search marks keypoints taken and
// raises the overflow word, which goes up as zero.  After an overflow the whole sequence runs a second time with a longer row
// stride, from the caller's flags again.
static int sbp_host_run(const SbpHostCall& c)
{
    HostStage& w = match_host_stage();
    const size_t n = (size_t)c.n, nq = (size_t)c.nq, kb = sizeof(orbfe_keypoint);
    IoLayout l;
    const size_t s_kps = l.take(n * kb), s_desc = l.take(n * 32), s_q = l.take(nq * sizeof(SbpQuery)), s_qdesc = l.take(nq * 32);
    const size_t s_obs = l.take(nq), s_angle = l.take(nq * 4), s_x3 = l.take(nq * 12), s_valid = l.take(nq);
    const size_t s_last = l.take(c.kps_last ? nq * kb : 0), s_cam = l.take(c.kps_last ? (12 + 16) * 4 : 0);
    const size_t s_min = l.take(c.P ? nq * 4 : 0), s_max = l.take(c.P ? nq * 4 : 0), s_nrm = l.take(c.P ? nq * 12 : 0);
    l.inout();
    const size_t s_taken = l.take(n), s_cnt = l.take(8); // nmatches, overflow
    l.outputs();
    const size_t s_cur = l.take(n * 4), s_out = l.take(nq * 4 * 7); // best_idx .. second_level, match, qbin
    int rc = w.begin(l);
    if (rc) return rc;
    const hipStream_t s = w.stream;
    MatchWorkspace& m = ws(s);
    int32_t* o = w.dev<int32_t>(s_out);
    SbpBatch B{};
    B.kps = w.dev<const orbfe_keypoint>(s_kps); B.desc = w.dev<const uint8_t>(s_desc); B.capacity = c.n;
    B.queries = w.dev<const SbpQuery>(s_q); B.qdesc = w.dev<const uint8_t>(s_qdesc); B.qcapacity = c.nq;
    B.taken = c.taken ? w.dev<uint8_t>(s_taken) : nullptr; B.q_observed = c.q_observed ? w.dev<const uint8_t>(s_obs) : nullptr;
    B.q_angle = c.q_angle || c.kps_last ? w.dev<const float>(s_angle) : nullptr;
    if (c.best_idx) { B.best_idx = o; B.best_dist = o + nq; B.best_level = o + 2 * nq; B.second_dist = o + 3 * nq; B.second_level = o + 4 * nq; }
    B.match = o + 5 * nq; B.qbin = o + 6 * nq; B.match_cur = w.dev<int32_t>(s_cur);
    B.nmatches = w.dev<int32_t>(s_cnt); B.overflow = B.nmatches + 1;
    if (c.chi2 > 0.0) { B.chi2 = c.chi2; for (int l = 0; l < 16; l++) B.inv_sigma2[l] = c.inv_sigma2[std::min(l, c.nlevels - 1)]; }
    w.put(s_kps, c.kps, n * kb); w.put(s_desc, c.desc, n * 32);
    w.put(s_q, c.window, nq * sizeof(orbfe_window_query)); w.put(s_qdesc, c.qdesc, nq * 32);
    w.put(s_obs, c.q_observed, nq); w.put(s_angle, c.q_angle, nq * 4);
    w.put(s_x3, c.x3Dw, nq * 12); w.put(s_valid, c.valid, nq);
    if (c.P) { w.put(s_min, c.min_dist, nq * 4); w.put(s_max, c.max_dist, nq * 4); w.put(s_nrm, c.normal, nq * 12); }
    else if (c.kps_last) {
        float cam[12 + 16]; // Tcw, the scale factors
        memcpy(cam, c.Tcw, 48);
        for (int l = 0; l < 16; l++) cam[12 + l] = l < c.nlevels ? c.scale[l] : 0.0f;
        w.put(s_last, c.kps_last, nq * kb); w.put(s_cam, cam, sizeof cam);
    }
    const uint8_t* d_valid = c.valid ? w.dev<const uint8_t>(s_valid) : nullptr;
    for (int attempt = 0;; attempt++) {
        const int32_t zero[2] = {0, 0};
        w.put(s_taken, c.taken, n); w.put(s_cnt, zero, 8);
        if ((rc = w.upload())) return rc;
        if (c.P)
            hipLaunchKernelGGL(k_project_map_points, dim3((c.nq + 255) / 256), dim3(256), 0, s, w.dev<const float>(s_x3), d_valid,
                               w.dev<const float>(s_min), w.dev<const float>(s_max), c.normal ? w.dev<const float>(s_nrm) : nullptr, c.nq, *c.P,
                               w.dev<SbpQuery>(s_q));
        else if (c.kps_last)
            hipLaunchKernelGGL(k_project_last_frame, dim3((c.nq + 255) / 256), dim3(256), 0, s, w.dev<const float>(s_x3), d_valid,
                               w.dev<const orbfe_keypoint>(s_last), c.nq, w.dev<const float>(s_cam), make_float4(c.K4[0], c.K4[1], c.K4[2], c.K4[3]),
                               c.bnd, w.dev<const float>(s_cam) + 12, c.nlevels, c.th, w.dev<SbpQuery>(s_q), w.dev<float>(s_angle));
        ORBFE_HIP(hipGetLastError());
        if ((rc = sbp_launch(m, B, 1, c.bnd, c.mode, c.th_high, c.nnratio, c.factor, c.check_ori, s)) || (rc = w.download()) || (rc = w.sync()))
            return rc;
        const int32_t ovf = w.host<const int32_t>(s_cnt)[1];
        if (!ovf) break;
        if (attempt) return fail(ORBFE_ERR_CAPACITY, "candidate row overflow (%d)", ovf);
        m.sbp_stride = sbp_stride_after(m.sbp_stride, ovf);
    }
    int32_t* const out[6] = {c.best_idx, c.best_dist, c.best_level, c.second_dist, c.second_level, c.match};
    for (int k = 0; k < 6; k++) w.get(out[k], s_out + k * nq * 4, nq * 4);
    w.get(c.match_cur, s_cur, n * 4); w.get(c.nmatches, s_cnt, 4); w.get(c.taken_out, s_taken, n);
    return ORBFE_OK;
}

} // namespace orbfe

using namespace orbfe;

extern "C" {

int orbfe_debug_control(const char* key, int value)
{
    if (key && !strcmp(key, "knn2_path") && value >= 0 && value <= 2) { g_match_switches.knn2_path = value; return ORBFE_OK; }
#ifdef ORBFE_ABLATION // diagnosis build only; the shipped library cannot skip work
    if (key && !strcmp(key, "orb_skip")) { orbfe::g_orb_skip = value; return ORBFE_OK; }
    if (key && !strcmp(key, "aruco_skip")) { orbfe::g_aruco_skip = value; return ORBFE_OK; }
#endif
    return fail(ORBFE_ERR_INVALID, "orbfe_debug_control: unknown key or value");
}

int orbfe_hamming(const uint8_t* a, const uint8_t* b)
{
    // host-side scalar helper: the 256-bit Hamming distance of ORBmatcher::DescriptorDistance (ORBmatcher.cc:1651-1667)
    uint64_t x[4], y[4];
    memcpy(x, a, 32);
    memcpy(y, b, 32);
    int dist = 0;
    for (int i = 0; i < 4; i++) dist += __builtin_popcountll(x[i] ^ y[i]);
    return dist;
}

void orbfe_three_maxima(const int32_t* counts, int L, int32_t* ind3)
{
    // host-side scalar helper: ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1605-1646) on the bin populations; the device
    // searches carry their own copy (rot_hist_maxima).  A running top three with strict '>' (the earliest bin wins ties), then the
    // 10 % rule on the runner-ups.
    int top[3] = {0, 0, 0};
    ind3[0] = ind3[1] = ind3[2] = -1;
    for (int i = 0; i < L; i++) {
        const int c = counts[i];
        int k = 0;
        while (k < 3 && c <= top[k]) k++;
        if (k == 3) continue;
        for (int j = 2; j > k; j--) { top[j] = top[j - 1]; ind3[j] = ind3[j - 1]; }
        top[k] = c;
        ind3[k] = i;
    }
    const float floor_ = 0.1f * (float)top[0];
    if ((float)top[1] < floor_) ind3[1] = ind3[2] = -1;
    else if ((float)top[2] < floor_) ind3[2] = -1;
}

int orbfe_epipolar_distance_ok(float x1, float y1, float x2, float y2, const float* F12, float level_sigma2)
{
    // host-side scalar helper: ORBmatcher::CheckDistEpipolarLine (ORBmatcher.cc:139-157); l = x1' F12, row-major 3 x 3
    float l[3];
    for (int j = 0; j < 3; j++) l[j] = x1 * F12[j] + y1 * F12[3 + j] + F12[6 + j];
    const float num = l[0] * x2 + l[1] * y2 + l[2];
    const float den = l[0] * l[0] + l[1] * l[1];
    if (den == 0) return 0;
    return num * num / den < 3.84 * level_sigma2; // the comparison is in double, as in the reference
}

int orbfe_knn2_batch_device(const uint8_t* d_Q, const int32_t* d_nq, size_t q_stride, int max_nq, const uint8_t* d_T,
                            const int32_t* d_nt, size_t t_stride, int max_nt, int npairs, int init,
                            int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_second_dist, void* stream)
{
    if (!d_Q || !d_T || !d_nt || !d_best_idx || !d_best_dist || !d_second_dist || max_nq <= 0 || max_nt < 0 ||
        npairs <= 0)
        return fail(ORBFE_ERR_INVALID, "orbfe_knn2_batch_device: invalid argument");
    return knn2_launch(d_Q, d_nq, q_stride, max_nq, d_T, d_nt, t_stride, max_nt, npairs, init, d_best_idx,
                       d_best_dist, d_second_dist, (hipStream_t)stream);
}

int orbfe_knn2(const uint8_t* Q, int nq, const uint8_t* T, int nt, int init, int32_t* best_idx, int32_t* best_dist,
               int32_t* second_dist, int device)
{
    if (nq < 0 || nt < 0 || (nq && (!Q || !best_idx || !best_dist || !second_dist)) || (nt && !T))
        return fail(ORBFE_ERR_INVALID, "orbfe_knn2: invalid argument");
    int rc = use_device(device);
    if (rc) return rc;
    if (nq == 0) return ORBFE_OK;
    HostStage& w = match_host_stage();
    const size_t Q4 = (size_t)nq * 4;
    IoLayout l;
    const size_t i_q = l.take((size_t)nq * 32), i_t = l.take((size_t)nt * 32), i_nt = l.take(4);
    l.outputs();
    const size_t o_idx = l.take(Q4), o_best = l.take(Q4), o_second = l.take(Q4);
    if ((rc = w.begin(l))) return rc;
    w.put(i_q, Q, (size_t)nq * 32); w.put(i_t, T, (size_t)nt * 32); w.put(i_nt, &nt, 4);
    if ((rc = w.upload()) ||
        (rc = knn2_launch(w.dev<const uint8_t>(i_q), nullptr, 0, nq, w.dev<const uint8_t>(i_t), w.dev<const int32_t>(i_nt), 0, nt, 1, init,
                          w.dev<int32_t>(o_idx), w.dev<int32_t>(o_best), w.dev<int32_t>(o_second), w.stream)) ||
        (rc = w.download()) || (rc = w.sync()))
        return rc;
    w.get(best_idx, o_idx, Q4); w.get(best_dist, o_best, Q4); w.get(second_dist, o_second, Q4);
    return ORBFE_OK;
}

int orbfe_search_for_initialization_batch_device(const orbfe_keypoint* d_kps, const uint8_t* d_desc,
                                                 const int32_t* d_n, int capacity, int npairs, int cols, int rows,
                                                 const float* bounds, int window_size, float nnratio, int check_orientation,
                                                 int32_t* d_matches12, int32_t* d_nmatches, void* stream)
{
    if (!d_kps || !d_desc || !d_n || !d_matches12 || !d_nmatches || capacity <= 0 || npairs <= 0 || cols <= 0 ||
        rows <= 0)
        return fail(ORBFE_ERR_INVALID, "orbfe_search_for_initialization_batch_device: invalid argument");
    return sfi_launch(d_kps, d_desc, d_n, capacity, npairs, frame_bounds(cols, rows, bounds), window_size, nnratio, check_orientation,
                      nullptr, nullptr, d_matches12, d_nmatches, (hipStream_t)stream, ws((hipStream_t)stream));
}

int orbfe_search_for_initialization_batch_status(void* stream, int32_t* overflow)
{
    if (!overflow) return fail(ORBFE_ERR_INVALID, "orbfe_search_for_initialization_batch_status: null argument");
    *overflow = 0;
    hipStream_t s = (hipStream_t)stream;
    MatchWorkspace& w = ws(s);
    if (!w.sfi_overflow.p) return ORBFE_OK; // no batch on this (thread, device, stream) yet
    ORBFE_HIP(hipStreamSynchronize(s));
    int32_t f[2] = {0, 0};
    ORBFE_HIP(hipMemcpy(f, w.sfi_overflow.p, 8, hipMemcpyDeviceToHost));
    return sfi_take_flags(w, f, s, overflow);
}

int orbfe_search_for_initialization(const orbfe_keypoint* kps1, const uint8_t* desc1, int n1,
                                    const orbfe_keypoint* kps2, const uint8_t* desc2, int n2, int cols, int rows,
                                    const float* bounds, float* prev_matched, int32_t* matches12, int window_size, float nnratio,
                                    int check_orientation, int32_t* nmatches, int device)
{
    if (n1 < 0 || n2 < 0 || !nmatches || (n1 && (!kps1 || !desc1 || !matches12 || !prev_matched)) ||
        (n2 && (!kps2 || !desc2)) || cols <= 0 || rows <= 0)
        return fail(ORBFE_ERR_INVALID, "orbfe_search_for_initialization: invalid argument");
    int rc = use_device(device);
    if (rc) return rc;
    *nmatches = 0;
    if (n1 == 0) return ORBFE_OK;
    const size_t cap = (size_t)std::max(std::max(n1, n2), 1), kb = cap * sizeof(orbfe_keypoint), db = cap * 32;
    HostStage& w = match_host_stage();
    // prev_matched travels both ways; the two flag words live in the kernels' workspace and come down to o_flags of the page-locked half
    IoLayout l;
    const size_t i_kps = l.take(2 * kb), i_desc = l.take(2 * db), i_nk = l.take(8);
    l.inout();
    const size_t io_prev = l.take(cap * 8);
    l.outputs();
    const size_t o_m12 = l.take(cap * 4), o_nm = l.take(4), o_flags = l.take(8);
    if ((rc = w.begin(l))) return rc;
    const hipStream_t s = w.stream;
    MatchWorkspace& m = ws(s);
    const int32_t nn[2] = {n1, n2};
    w.put(i_kps, kps1, (size_t)n1 * sizeof(orbfe_keypoint)); w.put(i_kps + kb, kps2, (size_t)n2 * sizeof(orbfe_keypoint));
    w.put(i_desc, desc1, (size_t)n1 * 32); w.put(i_desc + db, desc2, (size_t)n2 * 32);
    w.put(i_nk, nn, 8);
    for (int attempt = 0;; attempt++) {
        // a run overwrites the device copy of prev_matched: every attempt starts from the caller's
        w.put(io_prev, prev_matched, (size_t)n1 * 8);
        if ((rc = w.upload()) ||
            (rc = sfi_launch(w.dev<const orbfe_keypoint>(i_kps), w.dev<const uint8_t>(i_desc), w.dev<const int32_t>(i_nk), (int)cap, 1,
                             frame_bounds(cols, rows, bounds), window_size, nnratio, check_orientation, w.dev<const float>(io_prev),
                             w.dev<float>(io_prev), w.dev<int32_t>(o_m12), w.dev<int32_t>(o_nm), s, m)))
            return rc;
        // the download: the results and the flag words in ONE launch that writes the page-locked half (OutPack, orbfe_common.hpp:
        // the flags are not part of the io block, and every small copy would be a blit kernel of its own)
        OutPack op;
        op.add(w.host<void>(o_m12), w.dev<void>(o_m12), (size_t)n1 * 4);
        op.add(w.host<void>(io_prev), w.dev<void>(io_prev), (size_t)n1 * 8);
        op.add(w.host<void>(o_nm), w.dev<void>(o_nm), 4);
        op.add(w.host<void>(o_flags), m.sfi_overflow.p, 8);
        if ((rc = op.flush<3>(s)) || (rc = w.sync())) return rc;
        const int32_t* fl = w.host<const int32_t>(o_flags);
        if (!fl[0] && !fl[1]) break;
        int32_t ovf = 0;
        if ((rc = sfi_take_flags(m, fl, s, &ovf))) return rc; // clears the flags, grows the pool
        if (attempt) return fail(ORBFE_ERR_CAPACITY, "candidate pool overflow (%d)", ovf);
    }
    w.get(matches12, o_m12, (size_t)n1 * 4); w.get(prev_matched, io_prev, (size_t)n1 * 8); w.get(nmatches, o_nm, 4);
    return ORBFE_OK;
}

int orbfe_search_by_projection(const orbfe_keypoint* kps, const uint8_t* desc, int n, int cols, int rows, const float* bounds,
                               const orbfe_window_query* queries, const uint8_t* qdesc, int nq, uint8_t* taken, const uint8_t* q_observed,
                               int mode, int th_high, float nnratio, int32_t* best_idx, int32_t* best_dist, int32_t* best_level,
                               int32_t* second_dist, int32_t* second_level, int32_t* match, int32_t* nmatches, int device)
{
    if (n < 0 || nq < 0 || cols <= 0 || rows <= 0 || (mode != 0 && mode != 1) || (n && (!kps || !desc)) ||
        (nq && (!queries || !qdesc)) || (mode == 1 && nq && (!match || !nmatches)) ||
        (best_idx && (!best_dist || !best_level || !second_dist || !second_level)))
        return fail(ORBFE_ERR_INVALID, "orbfe_search_by_projection: invalid argument");
    int rc = use_device(device);
    if (rc) return rc;
    if (nmatches) *nmatches = 0;
    if (nq == 0) return ORBFE_OK;
    SbpHostCall c{kps, desc, n, frame_bounds(cols, rows, bounds), taken, nq, qdesc, q_observed};
    c.window = queries;
    c.mode = mode; c.th_high = th_high; c.nnratio = nnratio;
    c.best_idx = best_idx; c.best_dist = best_dist; c.best_level = best_level; c.second_dist = second_dist; c.second_level = second_level;
    if (mode == 1) { c.match = match; c.nmatches = nmatches; c.taken_out = taken; }
    return sbp_host_run(c);
}

int orbfe_search_by_projection_best(const orbfe_keypoint* kps, const uint8_t* desc, int n, int cols, int rows, const float* bounds,
                                    const orbfe_window_query* queries, const float* q_angle, const uint8_t* qdesc, const uint8_t* q_blocks,
                                    int nq, const uint8_t* taken, int th_high, int check_orientation, float factor, int32_t* match_cur,
                                    int32_t* nmatches, int device)
{
    if (n < 0 || nq < 0 || cols <= 0 || rows <= 0 || !nmatches || (n && (!kps || !desc || !match_cur)) ||
        (nq && (!queries || !qdesc || (check_orientation && !q_angle))))
        return fail(ORBFE_ERR_INVALID, "orbfe_search_by_projection_best: invalid argument");
    int rc = use_device(device);
    if (rc) return rc;
    *nmatches = 0;
    for (int i = 0; i < n; i++) match_cur[i] = -1;
    if (nq == 0 || n == 0) return ORBFE_OK;
    SbpHostCall c{kps, desc, n, frame_bounds(cols, rows, bounds), taken, nq, qdesc, q_blocks, q_angle};
    c.window = queries;
    c.mode = 2; c.th_high = th_high; c.factor = factor; c.check_ori = check_orientation;
    c.match_cur = match_cur; c.nmatches = nmatches;
    return sbp_host_run(c);
}

int orbfe_search_by_projection_last_frame(const orbfe_keypoint* kps_cur, const uint8_t* desc_cur, int n_cur, const uint8_t* taken_cur,
                                          int cols, int rows, const float* bounds, const orbfe_keypoint* kps_last, int n_last,
                                          const uint8_t* valid_last, const float* x3Dw, const uint8_t* mp_desc, const uint8_t* mp_observed,
                                          const float* Tcw, const float* K4, const float* scale_factors, int nlevels, float th, int th_high,
                                          int check_orientation, int32_t* match_cur, int32_t* nmatches, int device)
{
    if (n_cur < 0 || n_last < 0 || cols <= 0 || rows <= 0 || !nmatches || (n_cur && (!kps_cur || !desc_cur || !match_cur)) ||
        (n_last && (!kps_last || !x3Dw || !mp_desc)) || !Tcw || !K4 || !scale_factors || nlevels < 1 || nlevels > 16)
        return fail(ORBFE_ERR_INVALID, "orbfe_search_by_projection_last_frame: invalid argument");
    int rc = use_device(device);
    if (rc) return rc;
    *nmatches = 0;
    for (int i = 0; i < n_cur; i++) match_cur[i] = -1;
    if (n_last == 0 || n_cur == 0) return ORBFE_OK;
    SbpHostCall c{kps_cur, desc_cur, n_cur, frame_bounds(cols, rows, bounds), taken_cur, n_last, mp_desc, mp_observed};
    c.x3Dw = x3Dw; c.valid = valid_last; c.kps_last = kps_last; c.Tcw = Tcw; c.K4 = K4; c.scale = scale_factors; c.nlevels = nlevels; c.th = th;
    c.mode = 2; c.th_high = th_high; c.factor = 1.0f / 30 /* :1341 */; c.check_ori = check_orientation;
    c.match_cur = match_cur; c.nmatches = nmatches;
    return sbp_host_run(c);
}

static int project_params(ProjectParams& P, const float* Tcw, const float* Ow, const float* K4, int cols, int rows, const float* bounds,
                          int strict_max, const float* scale, int nlevels, float log_scale, float th, int below, int above, const char* who)
{
    if (!Tcw || !Ow || !K4 || !scale || nlevels < 1 || nlevels > 16 || cols <= 0 || rows <= 0 || !(log_scale > 0.0f))
        return fail(ORBFE_ERR_INVALID, "%s: invalid camera / pyramid argument", who);
    memcpy(P.T, Tcw, 48); memcpy(P.Ow, Ow, 12); memcpy(P.K, K4, 16);
    const float4 b = frame_bounds(cols, rows, bounds);
    P.bnd[0] = b.x; P.bnd[1] = b.y; P.bnd[2] = b.z; P.bnd[3] = b.w;
    for (int l = 0; l < 16; l++) P.scale[l] = scale[std::min(l, nlevels - 1)];
    P.nlevels = nlevels; P.strict_max = strict_max; P.level_below = below; P.level_above = above; P.log_scale = log_scale; P.th = th;
    P.use_T2 = 0;
    for (int i = 0; i < 12; i++) P.T2[i] = 0.0f;
    P.frame_variant = 0;
    return ORBFE_OK;
}

int orbfe_project_map_points(const float* p3Dw, const uint8_t* valid, const float* min_dist, const float* max_dist, const float* normal, int n,
                             const float* Tcw, const float* Ow, const float* K4, int cols, int rows, const float* bounds, int keyframe_variant,
                             const float* scale_factors, int nlevels, float log_scale_factor, float th, int level_below, int level_above,
                             orbfe_window_query* queries, int device)
{
    if (n < 0 || (n && (!p3Dw || !min_dist || !max_dist || !queries)))
        return fail(ORBFE_ERR_INVALID, "orbfe_project_map_points: invalid argument");
    ProjectParams P;
    int rc = project_params(P, Tcw, Ow, K4, cols, rows, bounds, keyframe_variant, scale_factors, nlevels, log_scale_factor, th, level_below,
                            level_above, "orbfe_project_map_points");
    P.frame_variant = !keyframe_variant;
    if (rc || (rc = use_device(device)) || n == 0) return rc;
    HostStage& w = match_host_stage();
    const size_t N = (size_t)n;
    IoLayout l;
    const size_t i_p = l.take(N * 12), i_min = l.take(N * 4), i_max = l.take(N * 4), i_nrm = l.take(N * 12), i_valid = l.take(N);
    l.outputs();
    const size_t o_q = l.take(N * sizeof(orbfe_window_query));
    if ((rc = w.begin(l))) return rc;
    w.put(i_p, p3Dw, N * 12); w.put(i_min, min_dist, N * 4); w.put(i_max, max_dist, N * 4);
    w.put(i_nrm, normal, N * 12); w.put(i_valid, valid, N);
    if ((rc = w.upload())) return rc;
    hipLaunchKernelGGL(k_project_map_points, dim3((n + 255) / 256), dim3(256), 0, w.stream, w.dev<const float>(i_p),
                       valid ? w.dev<const uint8_t>(i_valid) : nullptr, w.dev<const float>(i_min), w.dev<const float>(i_max),
                       normal ? w.dev<const float>(i_nrm) : nullptr, n, P, w.dev<SbpQuery>(o_q));
    ORBFE_HIP(hipGetLastError());
    if ((rc = w.download()) || (rc = w.sync())) return rc;
    w.get(queries, o_q, N * sizeof(orbfe_window_query));
    return ORBFE_OK;
}

int orbfe_fuse_search(const orbfe_keypoint* kps, const uint8_t* desc, int n, int cols, int rows, const float* bounds, const float* p3Dw,
                      const uint8_t* valid, const float* min_dist, const float* max_dist, const float* normal, const uint8_t* mp_desc, int nmp,
                      const float* Tcw, const float* Ow, const float* K4, const float* scale_factors, const float* inv_level_sigma2, int nlevels,
                      float log_scale_factor, float th, double chi2, int32_t* best_idx, int32_t* best_dist, int device)
{
    if (n < 0 || nmp < 0 || (n && (!kps || !desc)) || (nmp && (!p3Dw || !min_dist || !max_dist || !normal || !mp_desc || !best_idx || !best_dist)) ||
        (chi2 > 0.0 && !inv_level_sigma2))
        return fail(ORBFE_ERR_INVALID, "orbfe_fuse_search: invalid argument");
    ProjectParams P;
    int rc = project_params(P, Tcw, Ow, K4, cols, rows, bounds, 1, scale_factors, nlevels, log_scale_factor, th, 1, 0, "orbfe_fuse_search");
    if (rc || (rc = use_device(device))) return rc;
    for (int i = 0; i < nmp; i++) { best_idx[i] = -1; best_dist[i] = 256; }
    if (nmp == 0 || n == 0) return ORBFE_OK;
    SbpHostCall c{kps, desc, n, frame_bounds(cols, rows, bounds), nullptr, nmp, mp_desc};
    c.x3Dw = p3Dw; c.valid = valid; c.P = &P; c.min_dist = min_dist; c.max_dist = max_dist; c.normal = normal;
    c.chi2 = chi2; c.inv_sigma2 = inv_level_sigma2; c.nlevels = nlevels; c.best_idx = best_idx; c.best_dist = best_dist;
    return sbp_host_run(c);
}

int orbfe_search_by_sim3(const orbfe_keypoint* kps1, const uint8_t* desc1, int n1, const orbfe_keypoint* kps2, const uint8_t* desc2, int n2,
                         int cols, int rows, const float* bounds, const float* p3Dw1, const uint8_t* valid1, const float* min_dist1,
                         const float* max_dist1, const uint8_t* mp_desc1, const float* p3Dw2, const uint8_t* valid2, const float* min_dist2,
                         const float* max_dist2, const uint8_t* mp_desc2, const float* T1w, const float* T2w, const float* sT12,
                         const float* sT21, const float* K4, const float* scale_factors, int nlevels, float log_scale_factor, float th,
                         int th_high, int32_t* match12, int32_t* nfound, int device)
{
    if (n1 < 0 || n2 < 0 || !nfound || (n1 && (!kps1 || !desc1 || !p3Dw1 || !min_dist1 || !max_dist1 || !mp_desc1 || !match12)) ||
        (n2 && (!kps2 || !desc2 || !p3Dw2 || !min_dist2 || !max_dist2 || !mp_desc2)) || !T1w || !T2w || !sT12 || !sT21)
        return fail(ORBFE_ERR_INVALID, "orbfe_search_by_sim3: invalid argument");
    const float zero3[3] = {0.0f, 0.0f, 0.0f};
    ProjectParams P12, P21;
    // KF1's points: camera 1, then sR21 | t21 into camera 2, searched in KF2 (:1148-1219); KF2's points the other way (:1228-1299)
    int rc = project_params(P12, T1w, zero3, K4, cols, rows, bounds, 1, scale_factors, nlevels, log_scale_factor, th, 1, 0, "orbfe_search_by_sim3");
    if (rc || (rc = project_params(P21, T2w, zero3, K4, cols, rows, bounds, 1, scale_factors, nlevels, log_scale_factor, th, 1, 0,
                                   "orbfe_search_by_sim3")) || (rc = use_device(device)))
        return rc;
    P12.use_T2 = 1; memcpy(P12.T2, sT21, 48);
    P21.use_T2 = 1; memcpy(P21.T2, sT12, 48);
    *nfound = 0;
    for (int i = 0; i < n1; i++) match12[i] = -1;
    if (n1 == 0 || n2 == 0) return ORBFE_OK;
    std::vector<int32_t> m1(n1), d1(n1), m2(n2), d2(n2);
    // the best keypoint (mode 0) of every map point of one keyframe in the other
    const float4 bnd = frame_bounds(cols, rows, bounds);
    SbpHostCall c12{kps2, desc2, n2, bnd, nullptr, n1, mp_desc1}, c21{kps1, desc1, n1, bnd, nullptr, n2, mp_desc2};
    c12.x3Dw = p3Dw1; c12.valid = valid1; c12.P = &P12; c12.min_dist = min_dist1; c12.max_dist = max_dist1; c12.best_idx = m1.data(); c12.best_dist = d1.data();
    c21.x3Dw = p3Dw2; c21.valid = valid2; c21.P = &P21; c21.min_dist = min_dist2; c21.max_dist = max_dist2; c21.best_idx = m2.data(); c21.best_dist = d2.data();
    if ((rc = sbp_host_run(c12)) || (rc = sbp_host_run(c21))) return rc;
    int found = 0;
    for (int i1 = 0; i1 < n1; i1++) { // check agreement (:1302-1318)
        const int idx2 = d1[i1] <= th_high ? m1[i1] : -1;
        if (idx2 >= 0) {
            const int idx1 = d2[idx2] <= th_high ? m2[idx2] : -1;
            if (idx1 == i1) { match12[i1] = idx2; found++; }
        }
    }
    *nfound = found;
    return ORBFE_OK;
}

int orbfe_search_by_projection_sim3(const orbfe_keypoint* kps, const uint8_t* desc, int n, int cols, int rows, const float* bounds,
                                    const uint8_t* matched, const float* p3Dw, const uint8_t* valid, const float* min_dist,
                                    const float* max_dist, const float* normal, const uint8_t* mp_desc, int nmp, const float* Tcw,
                                    const float* Ow, const float* K4, const float* scale_factors, int nlevels, float log_scale_factor, int th,
                                    int32_t* match_kf, int32_t* nmatches, int device)
{
    if (nmp < 0 || (nmp && (!p3Dw || !min_dist || !max_dist || !normal || !mp_desc)) || !nmatches)
        return fail(ORBFE_ERR_INVALID, "orbfe_search_by_projection_sim3: invalid argument");
    std::vector<orbfe_window_query> q(std::max(nmp, 1));
    // :321-358 projection and gates, then the loop of :360-401: best only, <= TH_LOW, a matched keypoint is taken, no rotation check
    int rc = orbfe_project_map_points(p3Dw, valid, min_dist, max_dist, normal, nmp, Tcw, Ow, K4, cols, rows, bounds, 1, scale_factors, nlevels,
                                      log_scale_factor, (float)th, 1, 0, q.data(), device);
    if (rc) return rc;
    return orbfe_search_by_projection_best(kps, desc, n, cols, rows, bounds, q.data(), nullptr, mp_desc, nullptr, nmp, matched, 50, 0, 0.0f,
                                           match_kf, nmatches, device);
}

int orbfe_search_by_projection_keyframe(const orbfe_keypoint* kps_cur, const uint8_t* desc_cur, int n_cur, const uint8_t* taken_cur, int cols,
                                        int rows, const float* bounds, int n_kf, const float* kf_angle, const uint8_t* valid, const float* p3Dw,
                                        const float* min_dist, const float* max_dist, const uint8_t* mp_desc, const float* Tcw, const float* Ow,
                                        const float* K4, const float* scale_factors, int nlevels, float log_scale_factor, float th, int orb_dist,
                                        int check_orientation, int32_t* match_cur, int32_t* nmatches, int device)
{
    if (n_cur < 0 || n_kf < 0 || !nmatches || (n_cur && (!kps_cur || !desc_cur || !match_cur)) ||
        (n_kf && (!p3Dw || !min_dist || !max_dist || !mp_desc || (check_orientation && !kf_angle))))
        return fail(ORBFE_ERR_INVALID, "orbfe_search_by_projection_keyframe: invalid argument");
    ProjectParams P;
    // :1497-1530: Frame arithmetic and bounds, no viewing-angle gate, levels predicted - 1 .. predicted + 1 (:1532)
    int rc = project_params(P, Tcw, Ow, K4, cols, rows, bounds, 0, scale_factors, nlevels, log_scale_factor, th, 1, 1,
                            "orbfe_search_by_projection_keyframe");
    P.frame_variant = 1;
    if (rc || (rc = use_device(device))) return rc;
    *nmatches = 0;
    for (int i = 0; i < n_cur; i++) match_cur[i] = -1;
    if (n_kf == 0 || n_cur == 0) return ORBFE_OK;
    SbpHostCall c{kps_cur, desc_cur, n_cur, frame_bounds(cols, rows, bounds), taken_cur, n_kf, mp_desc, nullptr, kf_angle};
    c.x3Dw = p3Dw; c.valid = valid; c.P = &P; c.min_dist = min_dist; c.max_dist = max_dist;
    c.mode = 2; c.th_high = orb_dist; c.factor = 1.0f / 30 /* :1488 */; c.check_ori = check_orientation;
    c.match_cur = match_cur; c.nmatches = nmatches;
    return sbp_host_run(c);
}

int orbfe_search_by_projection_batch_device(const orbfe_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int capacity, int nframes,
                                            int cols, int rows, const float* bounds, const orbfe_window_query* d_queries,
                                            const uint8_t* d_qdesc, const int32_t* d_nq, int qcapacity, uint8_t* d_taken,
                                            const uint8_t* d_q_observed, const float* d_q_angle, int mode, int th_high, float nnratio,
                                            float factor, int check_orientation, int32_t* d_best_idx, int32_t* d_best_dist,
                                            int32_t* d_best_level, int32_t* d_second_dist, int32_t* d_second_level, int32_t* d_match,
                                            int32_t* d_match_cur, int32_t* d_nmatches, void* stream)
{
    if (!d_kps || !d_desc || !d_n || !d_queries || !d_qdesc || !d_nq || !d_match || !d_nmatches || capacity <= 0 || qcapacity <= 0 ||
        nframes <= 0 || cols <= 0 || rows <= 0 || mode < 0 || mode > 2 || (mode == 2 && (!d_match_cur || (check_orientation && !d_q_angle))) ||
        (d_best_idx && (!d_best_dist || !d_best_level || !d_second_dist || !d_second_level)))
        return fail(ORBFE_ERR_INVALID, "orbfe_search_by_projection_batch_device: invalid argument");
    hipStream_t s = (hipStream_t)stream;
    MatchWorkspace& w = ws(s);
    int rc;
    if ((rc = w.scratch.ensure((size_t)nframes * qcapacity * 4 + 256)) || (rc = ensure_sticky_flag(w.sbp_batch_overflow))) return rc;
    SbpBatch B{};
    B.kps = d_kps; B.desc = d_desc; B.n = d_n; B.capacity = capacity;
    B.queries = reinterpret_cast<const SbpQuery*>(d_queries); B.qdesc = d_qdesc; B.nq = d_nq; B.qcapacity = qcapacity;
    B.taken = d_taken; B.q_observed = d_q_observed; B.q_angle = d_q_angle;
    B.best_idx = d_best_idx; B.best_dist = d_best_dist; B.best_level = d_best_level; B.second_dist = d_second_dist; B.second_level = d_second_level;
    B.match = d_match; B.nmatches = d_nmatches; B.overflow = w.sbp_batch_overflow.as<int32_t>();
    B.match_cur = d_match_cur; B.qbin = w.scratch.as<int32_t>();
    return sbp_launch(w, B, nframes, frame_bounds(cols, rows, bounds), mode, th_high, nnratio, factor, check_orientation, s);
}

int orbfe_fuse_search_batch_device(const orbfe_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int capacity, int nkf, int cols, int rows,
                                   const float* bounds, const float* d_p3Dw, const uint8_t* d_valid, const float* d_min_dist,
                                   const float* d_max_dist, const float* d_normal, const uint8_t* d_mp_desc, int nmp, const float* Tcw,
                                   const float* Ow, const float* K4, const float* scale_factors, const float* inv_level_sigma2, int nlevels,
                                   float log_scale_factor, float th, double chi2, int32_t* d_best_idx, int32_t* d_best_dist, void* stream)
{
    if (!d_kps || !d_desc || !d_n || capacity <= 0 || nkf <= 0 || nmp <= 0 || !d_p3Dw || !d_min_dist || !d_max_dist || !d_normal || !d_mp_desc ||
        !Tcw || !Ow || !d_best_idx || !d_best_dist || (chi2 > 0.0 && !inv_level_sigma2))
        return fail(ORBFE_ERR_INVALID, "orbfe_fuse_search_batch_device: invalid argument");
    hipStream_t s = (hipStream_t)stream;
    MatchWorkspace& w = ws(s);
    const FuseBatchLayout fl = plan_fuse_batch(nkf, nmp);
    int rc;
    if ((rc = w.q.ensure(fl.q_bytes)) || (rc = w.obest.ensure(fl.obest_bytes)) || (rc = ensure_sticky_flag(w.sbp_batch_overflow))) return rc;
    for (int k = 0; k < nkf; k++) { // the projection and the gates of :848-915, one small launch per keyframe pose
        ProjectParams P;
        if ((rc = project_params(P, Tcw + 12 * k, Ow + 3 * k, K4, cols, rows, bounds, 1, scale_factors, nlevels, log_scale_factor, th, 1, 0,
                                 "orbfe_fuse_search_batch_device")))
            return rc;
        hipLaunchKernelGGL(k_project_map_points, dim3((nmp + 255) / 256), dim3(256), 0, s, d_p3Dw, d_valid ? d_valid + (size_t)k * nmp : nullptr,
                           d_min_dist, d_max_dist, d_normal, nmp, P, w.q.as<SbpQuery>() + (size_t)k * nmp);
    }
    int32_t* o = w.obest.as<int32_t>();
    int32_t* d_nq = o + fl.nq;
    ORBFE_HIP(hipMemsetD32Async((hipDeviceptr_t)d_nq, nmp, nkf, s));
    SbpBatch B{};
    B.kps = d_kps; B.desc = d_desc; B.n = d_n; B.capacity = capacity;
    B.queries = w.q.as<SbpQuery>(); B.qdesc = d_mp_desc; B.qdesc_shared = 1; B.nq = d_nq; B.qcapacity = nmp;
    B.best_idx = d_best_idx; B.best_dist = d_best_dist; B.best_level = o + fl.best_level; B.second_dist = o + fl.second_dist;
    B.second_level = o + fl.second_level; B.match = o + fl.match; B.nmatches = o + fl.nmatches; B.overflow = w.sbp_batch_overflow.as<int32_t>();
    if (chi2 > 0.0) { B.chi2 = chi2; for (int l = 0; l < 16; l++) B.inv_sigma2[l] = inv_level_sigma2[std::min(l, nlevels - 1)]; }
    return sbp_launch(w, B, nkf, frame_bounds(cols, rows, bounds), 0, 256, 0.0f, 0.0f, 0, s);
}

int orbfe_search_by_projection_batch_status(void* stream, int32_t* overflow)
{
    if (!overflow) return fail(ORBFE_ERR_INVALID, "orbfe_search_by_projection_batch_status: null argument");
    *overflow = 0;
    hipStream_t s = (hipStream_t)stream;
    MatchWorkspace& w = ws(s);
    if (!w.sbp_batch_overflow.p) return ORBFE_OK; // no batch on this (thread, device, stream) yet
    ORBFE_HIP(hipStreamSynchronize(s));
    ORBFE_HIP(hipMemcpy(overflow, w.sbp_batch_overflow.p, 4, hipMemcpyDeviceToHost));
    if (*overflow) ORBFE_HIP(hipMemset(w.sbp_batch_overflow.p, 0, 4)); // covers every batch since it was last read
    w.sbp_stride = sbp_stride_after(w.sbp_stride, *overflow); // the next batch on this stream has the room
    return ORBFE_OK;
}

int orbfe_release_stream_scratch(void* stream)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(ORBFE_ERR_NO_DEVICE, "orbfe_release_stream_scratch: no HIP device (this library has no CPU fallback)");
    hipStream_t s = (hipStream_t)stream;
    ORBFE_HIP(hipStreamSynchronize(s));
    tl_ws.release(s);
    return ORBFE_OK;
}

int orbfe_knn2_csr(const uint8_t* Q, int nq, const uint8_t* T, int nt, const int32_t* offsets, const int32_t* idx, int init,
                   int32_t* best_idx, int32_t* best_dist, int32_t* second_dist, int device)
{
    if (nq < 0 || nt < 0 || (nq && (!Q || !offsets || !best_idx || !best_dist || !second_dist)))
        return fail(ORBFE_ERR_INVALID, "orbfe_knn2_csr: invalid argument");
    int rc = use_device(device);
    if (rc) return rc;
    if (nq == 0) return ORBFE_OK;
    const int total = offsets[nq];
    if (offsets[0] != 0 || total < 0 || (total && (!idx || !T))) return fail(ORBFE_ERR_INVALID, "orbfe_knn2_csr: bad candidate lists");
    for (int q = 0; q < nq; q++)
        if (offsets[q + 1] < offsets[q]) return fail(ORBFE_ERR_INVALID, "orbfe_knn2_csr: offsets must be non-decreasing");
    for (int k = 0; k < total; k++)
        if (idx[k] < 0 || idx[k] >= nt) return fail(ORBFE_ERR_INVALID, "orbfe_knn2_csr: candidate %d out of range", idx[k]);
    HostStage& w = match_host_stage();
    const size_t Q4 = (size_t)nq * 4;
    IoLayout l;
    const size_t i_q = l.take((size_t)nq * 32), i_t = l.take((size_t)nt * 32), i_off = l.take(Q4 + 4), i_idx = l.take((size_t)total * 4);
    l.outputs();
    const size_t o_idx = l.take(Q4), o_best = l.take(Q4), o_second = l.take(Q4);
    if ((rc = w.begin(l))) return rc;
    w.put(i_q, Q, (size_t)nq * 32); w.put(i_t, T, (size_t)nt * 32);
    w.put(i_off, offsets, Q4 + 4); w.put(i_idx, idx, (size_t)total * 4);
    if ((rc = w.upload())) return rc;
    hipLaunchKernelGGL(k_knn2_csr, dim3((nq + 3) / 4), dim3(256), 0, w.stream, w.dev<const uint8_t>(i_q), nq, w.dev<const uint8_t>(i_t),
                       w.dev<const int32_t>(i_off), w.dev<const int32_t>(i_idx), init, w.dev<int32_t>(o_idx), w.dev<int32_t>(o_best),
                       w.dev<int32_t>(o_second));
    ORBFE_HIP(hipGetLastError());
    if ((rc = w.download()) || (rc = w.sync())) return rc;
    w.get(best_idx, o_idx, Q4); w.get(best_dist, o_best, Q4); w.get(second_dist, o_second, Q4);
    return ORBFE_OK;
}

int orbfe_distinctive_descriptors_device(const uint8_t* d_desc, const int32_t* d_offsets, int npoints, int32_t* d_best_idx, uint8_t* d_best_desc,
                                         void* stream)
{
    if (npoints < 0 || (npoints && (!d_desc || !d_offsets || !d_best_idx)))
        return fail(ORBFE_ERR_INVALID, "orbfe_distinctive_descriptors_device: invalid argument");
    if (npoints == 0) return ORBFE_OK;
    hipLaunchKernelGGL(k_distinctive, dim3((npoints + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_desc, d_offsets, npoints, d_best_idx, d_best_desc);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

int orbfe_distinctive_descriptors(const uint8_t* desc, const int32_t* offsets, int npoints, int32_t* best_idx, uint8_t* best_desc, int device)
{
    if (npoints < 0 || (npoints && (!offsets || !best_idx))) return fail(ORBFE_ERR_INVALID, "orbfe_distinctive_descriptors: invalid argument");
    if (npoints == 0) return ORBFE_OK;
    if (offsets[0] != 0) return fail(ORBFE_ERR_INVALID, "orbfe_distinctive_descriptors: offsets must start at 0");
    for (int p = 0; p < npoints; p++) {
        if (offsets[p + 1] < offsets[p]) return fail(ORBFE_ERR_INVALID, "orbfe_distinctive_descriptors: offsets must be non-decreasing");
        if (offsets[p + 1] - offsets[p] > DD_MAXN)
            return fail(ORBFE_ERR_CAPACITY, "map point %d has %d observations, at most %d are supported", p, offsets[p + 1] - offsets[p], DD_MAXN);
    }
    const int total = offsets[npoints];
    if (total && !desc) return fail(ORBFE_ERR_INVALID, "orbfe_distinctive_descriptors: null descriptors");
    int rc = use_device(device);
    if (rc) return rc;
    HostStage& w = match_host_stage();
    const size_t NP = (size_t)npoints;
    IoLayout l;
    const size_t i_desc = l.take((size_t)total * 32), i_off = l.take((NP + 1) * 4);
    l.outputs();
    const size_t o_idx = l.take(NP * 4), o_desc = l.take(best_desc ? NP * 32 : 0);
    if ((rc = w.begin(l))) return rc;
    w.put(i_desc, desc, (size_t)total * 32); w.put(i_off, offsets, (NP + 1) * 4);
    if ((rc = w.upload()) ||
        (rc = orbfe_distinctive_descriptors_device(w.dev<const uint8_t>(i_desc), w.dev<const int32_t>(i_off), npoints, w.dev<int32_t>(o_idx),
                                                   best_desc ? w.dev<uint8_t>(o_desc) : nullptr, w.stream)) ||
        (rc = w.download()) || (rc = w.sync()))
        return rc;
    w.get(best_idx, o_idx, NP * 4); w.get(best_desc, o_desc, NP * 32);
    return ORBFE_OK;
}

int orbfe_undistort_points(const float* src, int n, const float* K4, const float* dist, int ndist, float* dst, int device)
{
    if (n < 0 || (n && (!src || !dst))) return fail(ORBFE_ERR_INVALID, "orbfe_undistort_points: invalid argument");
    UndistortParams P;
    int rc = undistort_params(K4, dist, ndist, P, "orbfe_undistort_points");
    if (rc || (rc = use_device(device))) return rc;
    if (n == 0) return ORBFE_OK;
    HostStage& w = match_host_stage();
    IoLayout l;
    const size_t i_src = l.take((size_t)n * 8);
    l.outputs();
    const size_t o_dst = l.take((size_t)n * 8);
    if ((rc = w.begin(l))) return rc;
    w.put(i_src, src, (size_t)n * 8);
    if ((rc = w.upload())) return rc;
    hipLaunchKernelGGL(k_undistort_points, dim3((n + 255) / 256), dim3(256), 0, w.stream, w.dev<const float2>(i_src), n, P, w.dev<float2>(o_dst));
    ORBFE_HIP(hipGetLastError());
    if ((rc = w.download()) || (rc = w.sync())) return rc;
    w.get(dst, o_dst, (size_t)n * 8);
    return ORBFE_OK;
}

int orbfe_undistort_keypoints_batch_device(const orbfe_keypoint* d_kps, const int32_t* d_n, int capacity, int nframes,
                                           const float* K4, const float* dist, int ndist, orbfe_keypoint* d_kps_un, void* stream)
{
    if (nframes < 0 || capacity < 0 || (nframes && capacity && (!d_kps || !d_n || !d_kps_un)))
        return fail(ORBFE_ERR_INVALID, "orbfe_undistort_keypoints_batch_device: invalid argument");
    UndistortParams P;
    int rc = undistort_params(K4, dist, ndist, P, "orbfe_undistort_keypoints_batch_device");
    if (rc) return rc;
    if (nframes == 0 || capacity == 0) return ORBFE_OK;
    hipStream_t s = (hipStream_t)stream;
    if (ndist == 0 || dist[0] == 0.0f) { // Frame.cc:359-363: mvKeysUn = mvKeys
        if (d_kps_un != d_kps)
            ORBFE_HIP(hipMemcpyAsync(d_kps_un, d_kps, (size_t)nframes * capacity * sizeof(orbfe_keypoint), hipMemcpyDeviceToDevice, s));
        return ORBFE_OK;
    }
    hipLaunchKernelGGL(k_undistort_keypoints, dim3((capacity + 255) / 256, nframes), dim3(256), 0, s, d_kps, d_n, capacity, P, d_kps_un);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

int orbfe_compute_image_bounds(int cols, int rows, const float* K4, const float* dist, int ndist, float* bounds, int device)
{
    if (cols <= 0 || rows <= 0 || !bounds) return fail(ORBFE_ERR_INVALID, "orbfe_compute_image_bounds: invalid argument");
    if (ndist == 0 || (dist && dist[0] == 0.0f)) { // Frame.cc:444-450
        bounds[0] = 0.0f; bounds[1] = 0.0f; bounds[2] = (float)cols; bounds[3] = (float)rows;
        return ORBFE_OK;
    }
    const float c[8] = {0.0f, 0.0f, (float)cols, 0.0f, 0.0f, (float)rows, (float)cols, (float)rows};
    float u[8];
    int rc = orbfe_undistort_points(c, 4, K4, dist, ndist, u, device);
    if (rc) return rc;
    bounds[0] = std::min(u[0], u[4]); // mnMinX = min(top-left.x, bottom-left.x)   (Frame.cc:437)
    bounds[2] = std::max(u[2], u[6]); // mnMaxX = max(top-right.x, bottom-right.x) (:438)
    bounds[1] = std::min(u[1], u[3]); // mnMinY = min(top-left.y, top-right.y)     (:439)
    bounds[3] = std::max(u[5], u[7]); // mnMaxY = max(bottom-left.y, bottom-right.y) (:440)
    return ORBFE_OK;
}

} // extern "C"
