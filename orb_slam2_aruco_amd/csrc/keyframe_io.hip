// On-disk keyframe feature records of the reference's map files (src/Map.cc:297-321 SaveKeyFrame, :478-511 LoadKeyFrame):
// per feature  pt.x pt.y size angle response (5 x f32) | octave (i32) | mDescriptors.cols (i32, always 32) | 32 descriptor
// bytes | map point index (u64, ULONG_MAX = none)  = 68 bytes = 17 dwords, packed back to back after the keyframe header.
// Every offset in the file is a multiple of 4, so the records are moved as dwords.  Pure byte shuffling, HBM-bound:
// a workgroup stages 256 records (17 KB) through LDS so that both the file side and the array side are read and written
// as contiguous dwords; the stride of 17 dwords is odd, i.e. free of LDS bank conflicts.
#include "host_stage.hpp"
#include "orbfe_common.hpp"

using namespace orbfe;

#define KF_REC_DWORDS 17
#define KF_THREADS 256

namespace {

// file image -> arrays.  Segment s (one keyframe): records at byte offset seg_off[s] (multiple of 4), nrec = seg_first[s+1] -
// seg_first[s], first output index seg_first[s].  seg_off == NULL: one segment at offset 0 with n records.
__global__ __launch_bounds__(KF_THREADS) void k_kf_unpack(const uint32_t* __restrict__ file, const unsigned long long* __restrict__ seg_off,
                                                         const int32_t* __restrict__ seg_first, int n_single,
                                                         uint32_t* __restrict__ kps, uint32_t* __restrict__ desc,
                                                         uint32_t* __restrict__ mp, int32_t* __restrict__ bad)
{
    __shared__ uint32_t s_rec[KF_THREADS * KF_REC_DWORDS];
    const int s = blockIdx.y;
    const size_t src0 = seg_off ? (size_t)(seg_off[s] >> 2) : 0;
    const int first = seg_first ? seg_first[s] : 0;
    const int nrec = seg_first ? seg_first[s + 1] - first : n_single;
    const int r0 = blockIdx.x * KF_THREADS;
    if (r0 >= nrec) return;
    const int cnt = min(KF_THREADS, nrec - r0);
    const uint32_t* src = file + src0 + (size_t)r0 * KF_REC_DWORDS;
    {
        uint32_t v[KF_REC_DWORDS]; // all loads of the tile in flight before the first LDS store
#pragma unroll
        for (int k = 0; k < KF_REC_DWORDS; k++) {
            const int j = threadIdx.x + k * KF_THREADS;
            v[k] = j < cnt * KF_REC_DWORDS ? src[j] : 0u;
        }
#pragma unroll
        for (int k = 0; k < KF_REC_DWORDS; k++) {
            const int j = threadIdx.x + k * KF_THREADS;
            if (j < cnt * KF_REC_DWORDS) s_rec[j] = v[k];
        }
    }
    __syncthreads();
    const size_t o = (size_t)first + r0;
    for (int j = threadIdx.x; j < cnt * 7; j += KF_THREADS) { // cv::KeyPoint: 6 stored fields + class_id (not stored: -1)
        const int r = j / 7, c = j - r * 7;
        kps[o * 7 + j] = c < 6 ? s_rec[r * KF_REC_DWORDS + c] : 0xffffffffu;
    }
    for (int j = threadIdx.x; j < cnt * 8; j += KF_THREADS) desc[o * 8 + j] = s_rec[(j >> 3) * KF_REC_DWORDS + 7 + (j & 7)];
    if (mp)
        for (int j = threadIdx.x; j < cnt * 2; j += KF_THREADS) mp[o * 2 + j] = s_rec[(j >> 1) * KF_REC_DWORDS + 15 + (j & 1)];
    if (threadIdx.x < cnt && s_rec[threadIdx.x * KF_REC_DWORDS + 6] != 32u) atomicAdd(bad, 1); // Descriptors.cols (Map.cc:492)
}

__global__ __launch_bounds__(KF_THREADS) void k_kf_pack(const uint32_t* __restrict__ kps, const uint32_t* __restrict__ desc,
                                                       const uint32_t* __restrict__ mp, const unsigned long long* __restrict__ seg_off,
                                                       const int32_t* __restrict__ seg_first, int n_single, uint32_t* __restrict__ file)
{
    __shared__ uint32_t s_rec[KF_THREADS * KF_REC_DWORDS];
    const int s = blockIdx.y;
    const size_t dst0 = seg_off ? (size_t)(seg_off[s] >> 2) : 0;
    const int first = seg_first ? seg_first[s] : 0;
    const int nrec = seg_first ? seg_first[s + 1] - first : n_single;
    const int r0 = blockIdx.x * KF_THREADS;
    if (r0 >= nrec) return;
    const int cnt = min(KF_THREADS, nrec - r0);
    const size_t o = (size_t)first + r0;
    {
        uint32_t a[7], b[8], c2[2]; // the tile's 17 loads per thread in flight together
#pragma unroll
        for (int k = 0; k < 7; k++) { const int j = threadIdx.x + k * KF_THREADS; a[k] = j < cnt * 7 ? kps[o * 7 + j] : 0u; }
#pragma unroll
        for (int k = 0; k < 8; k++) { const int j = threadIdx.x + k * KF_THREADS; b[k] = j < cnt * 8 ? desc[o * 8 + j] : 0u; }
#pragma unroll
        for (int k = 0; k < 2; k++) { const int j = threadIdx.x + k * KF_THREADS; c2[k] = (mp && j < cnt * 2) ? mp[o * 2 + j] : 0xffffffffu; } // ULONG_MAX = no map point (Map.cc:316-317)
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const int j = threadIdx.x + k * KF_THREADS;
            const int r = j / 7, c = j - r * 7;
            if (j < cnt * 7 && c < 6) s_rec[r * KF_REC_DWORDS + c] = a[k];
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int j = threadIdx.x + k * KF_THREADS;
            if (j < cnt * 8) s_rec[(j >> 3) * KF_REC_DWORDS + 7 + (j & 7)] = b[k];
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int j = threadIdx.x + k * KF_THREADS;
            if (j < cnt * 2) s_rec[(j >> 1) * KF_REC_DWORDS + 15 + (j & 1)] = c2[k];
        }
    }
    if (threadIdx.x < cnt) s_rec[threadIdx.x * KF_REC_DWORDS + 6] = 32u; // mDescriptors.cols
    __syncthreads();
    uint32_t* dst = file + dst0 + (size_t)r0 * KF_REC_DWORDS;
    for (int j = threadIdx.x; j < cnt * KF_REC_DWORDS; j += KF_THREADS) dst[j] = s_rec[j];
}

} // namespace

extern "C" {

int orbfe_keyframe_features_unpack_device(const uint8_t* d_file, const uint64_t* d_seg_offset, const int32_t* d_seg_first, int nsegments,
                                          int max_records_per_segment, orbfe_keypoint* d_kps, uint8_t* d_desc, uint64_t* d_mp_index,
                                          int32_t* d_bad, void* stream)
{
    if (nsegments < 0 || max_records_per_segment < 0 || (nsegments && max_records_per_segment && (!d_file || !d_kps || !d_desc || !d_bad)) ||
        ((d_seg_offset == nullptr) != (d_seg_first == nullptr)) || (!d_seg_offset && nsegments > 1) || ((uintptr_t)d_file & 3))
        return fail(ORBFE_ERR_INVALID, "orbfe_keyframe_features_unpack_device: invalid argument");
    if (nsegments == 0 || max_records_per_segment == 0) return ORBFE_OK;
    hipLaunchKernelGGL(k_kf_unpack, dim3((max_records_per_segment + KF_THREADS - 1) / KF_THREADS, nsegments), dim3(KF_THREADS), 0,
                       (hipStream_t)stream, (const uint32_t*)d_file, (const unsigned long long*)d_seg_offset, d_seg_first,
                       max_records_per_segment, (uint32_t*)d_kps, (uint32_t*)d_desc, (uint32_t*)d_mp_index, d_bad);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

int orbfe_keyframe_features_pack_device(const orbfe_keypoint* d_kps, const uint8_t* d_desc, const uint64_t* d_mp_index,
                                        const uint64_t* d_seg_offset, const int32_t* d_seg_first, int nsegments,
                                        int max_records_per_segment, uint8_t* d_file, void* stream)
{
    if (nsegments < 0 || max_records_per_segment < 0 || (nsegments && max_records_per_segment && (!d_file || !d_kps || !d_desc)) ||
        ((d_seg_offset == nullptr) != (d_seg_first == nullptr)) || (!d_seg_offset && nsegments > 1) || ((uintptr_t)d_file & 3))
        return fail(ORBFE_ERR_INVALID, "orbfe_keyframe_features_pack_device: invalid argument");
    if (nsegments == 0 || max_records_per_segment == 0) return ORBFE_OK;
    hipLaunchKernelGGL(k_kf_pack, dim3((max_records_per_segment + KF_THREADS - 1) / KF_THREADS, nsegments), dim3(KF_THREADS), 0,
                       (hipStream_t)stream, (const uint32_t*)d_kps, (const uint32_t*)d_desc, (const uint32_t*)d_mp_index,
                       (const unsigned long long*)d_seg_offset, d_seg_first, max_records_per_segment, (uint32_t*)d_file);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

int orbfe_keyframe_features_pack(const orbfe_keypoint* kps, const uint8_t* desc, const uint64_t* mp_index, int n, uint8_t* out, int device)
{
    if (n < 0 || (n && (!kps || !desc || !out))) return fail(ORBFE_ERR_INVALID, "orbfe_keyframe_features_pack: invalid argument");
    int rc = use_device(device);
    if (rc || n == 0) return rc;
    HostStage& w = match_host_stage();
    const size_t N = (size_t)n;
    IoLayout l;
    const size_t i_kps = l.take(N * sizeof(orbfe_keypoint)), i_desc = l.take(N * 32), i_mp = l.take(mp_index ? N * 8 : 0);
    l.outputs();
    const size_t o_file = l.take(N * ORBFE_KF_FEATURE_BYTES);
    if ((rc = w.begin(l))) return rc;
    w.put(i_kps, kps, N * sizeof(orbfe_keypoint)); w.put(i_desc, desc, N * 32); w.put(i_mp, mp_index, N * 8);
    if ((rc = w.upload()) ||
        (rc = orbfe_keyframe_features_pack_device(w.dev<orbfe_keypoint>(i_kps), w.dev<uint8_t>(i_desc), mp_index ? w.dev<uint64_t>(i_mp) : nullptr,
                                                  nullptr, nullptr, 1, n, w.dev<uint8_t>(o_file), w.stream)) ||
        (rc = w.download()) || (rc = w.sync()))
        return rc;
    w.get(out, o_file, N * ORBFE_KF_FEATURE_BYTES);
    return ORBFE_OK;
}

int orbfe_keyframe_features_unpack(const uint8_t* in, int n, orbfe_keypoint* kps, uint8_t* desc, uint64_t* mp_index, int device)
{
    if (n < 0 || (n && (!in || !kps || !desc))) return fail(ORBFE_ERR_INVALID, "orbfe_keyframe_features_unpack: invalid argument");
    int rc = use_device(device);
    if (rc || n == 0) return rc;
    HostStage& w = match_host_stage();
    const size_t N = (size_t)n;
    IoLayout l;
    const size_t i_file = l.take(N * ORBFE_KF_FEATURE_BYTES);
    l.inout();
    const size_t io_bad = l.take(4); // the kernel counts in it: goes up as zero, comes back with the results
    l.outputs();
    const size_t o_kps = l.take(N * sizeof(orbfe_keypoint)), o_desc = l.take(N * 32), o_mp = l.take(mp_index ? N * 8 : 0);
    if ((rc = w.begin(l))) return rc;
    const int32_t zero = 0;
    w.put(i_file, in, N * ORBFE_KF_FEATURE_BYTES); w.put(io_bad, &zero, 4);
    if ((rc = w.upload()) ||
        (rc = orbfe_keyframe_features_unpack_device(w.dev<uint8_t>(i_file), nullptr, nullptr, 1, n, w.dev<orbfe_keypoint>(o_kps), w.dev<uint8_t>(o_desc),
                                                    mp_index ? w.dev<uint64_t>(o_mp) : nullptr, w.dev<int32_t>(io_bad), w.stream)) ||
        (rc = w.download()) || (rc = w.sync()))
        return rc;
    const int32_t bad = *w.host<const int32_t>(io_bad);
    if (bad) return fail(ORBFE_ERR_INVALID, "orbfe_keyframe_features_unpack: %d records with a descriptor length other than 32", bad);
    w.get(kps, o_kps, N * sizeof(orbfe_keypoint)); w.get(desc, o_desc, N * 32); w.get(mp_index, o_mp, N * 8);
    return ORBFE_OK;
}

} // extern "C"
