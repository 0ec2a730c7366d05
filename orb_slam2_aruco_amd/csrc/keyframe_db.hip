// keyframe_db.hip -- the candidate queries of KeyFrameDatabase (src/KeyFrameDatabase.cc:76-309) and DBoW2's L1 score
// (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) on gfx950.
//
// A query is two launches, whatever the number of queries:
//   - k_kfdb_score, grid (K / 8, nq): the workgroup stages the query's BowVector in LDS (4096 x 12 B); each wave takes keyframes,
//     its lanes stride over the keyframe's words and look each up in the staged query words (binary search).  The terms of the
//     common words of a 64-word step are added in lane order -- ascending word order -- into ONE double that every lane carries,
//     so the sum is the reference's sum bit for bit.  The same pass counts the common words and keeps the first one as its index
//     in the query, which orders like the word id.  Every active keyframe is scored; what the scores mean is decided next.
//     Per (query, keyframe): d_common = first << 13 | count, d_scratch = the float score.
//   - k_kfdb_select, one workgroup per query: the connected keyframes are struck out, the sharing keyframes are collected and
//     sorted by (first common word, position) -- the order in which the reference's walk over the inverted file meets them -- as
//     32-bit keys in LDS (bitonic); the word-count gate and min_score pick the kept ones, whose scores are committed to the
//     caller's state; one thread per kept entry walks its ten neighbours serially in float; bestAccScore is reduced with the
//     earliest entry winning ties (the reference's strict >); the retained entries' pBestKF are de-duplicated with an atomicMin
//     of the entry index per keyframe, and written in entry order.
// k_bow_score_pairs and k_bow_min_score use the same wave function on BowVectors in global memory.
#include "host_stage.hpp"
#include "orbfe_common.hpp"
#include "ransac_sets.hpp"   // clampn
#include <cmath>

namespace orbfe {
namespace {

constexpr int KD_THREADS = 256, KD_WAVES = KD_THREADS / 64;
constexpr int KD_KF_PER_WG = 8;    // two keyframes a wave: a single query of a few thousand keyframes still fills the device
constexpr int KD_CNT_BITS = 13;                       // a count is at most ORBFE_KFDB_MAX_WORDS = 2^12
constexpr uint32_t KD_CNT_MASK = (1u << KD_CNT_BITS) - 1u;
constexpr int KD_POS_BITS = 13;                       // a position is below ORBFE_KFDB_MAX_KEYFRAMES = 2^13
constexpr uint32_t KD_POS_MASK = (1u << KD_POS_BITS) - 1u;
static_assert(ORBFE_KFDB_MAX_WORDS <= (1 << (KD_CNT_BITS - 1)) && ORBFE_KFDB_MAX_KEYFRAMES <= (1 << KD_POS_BITS), "packing");

// where the BowVector of frame f is: blocks of `capacity` (the vocabulary transform's layout), or CSR (the host calls)
struct BowSet {
    const uint32_t* word;
    const double* value;
    const int32_t* nbow;      // blocks: entries of frame f, clamped to the block
    const int32_t* offsets;   // CSR: frame f owns offsets[f] .. offsets[f + 1]; NULL = blocks
    int capacity;
};

__device__ __forceinline__ int bow_of(const BowSet& B, int f, const uint32_t*& w, const double*& v)
{
    w = B.word; v = B.value;
    if (f < 0) return 0;
    if (B.offsets) {
        const int o = B.offsets[f], n = B.offsets[f + 1] - o;
        w += o; v += o;
        return n < 0 ? 0 : n;
    }
    w += (size_t)f * B.capacity; v += (size_t)f * B.capacity;
    return clampn(B.nbow[f], B.capacity);
}

struct L1Common {
    double sum;    // Sum(|vi - wi| - |vi| - |wi|) over the common words, ascending
    int count;     // common words
    int first;     // index in the query of the first common word
};

// One wave: query (qw ascending, qv; LDS or global) against keyframe (kw ascending, kv).  The result is the same in every lane.
__device__ __forceinline__ L1Common l1_common(const uint32_t* qw, const double* qv, int nq, const uint32_t* kw, const double* kv, int nk,
                                              int lane)
{
    L1Common r{0.0, 0, 0};
    for (int base = 0; base < nk; base += 64) {
        const int i = base + lane;
        int hit = -1;
        if (i < nk) {
            const uint32_t w = kw[i];
            int lo = 0, hi = nq;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (qw[mid] < w) lo = mid + 1; else hi = mid;
            }
            if (lo < nq && qw[lo] == w) hit = lo;
        }
        unsigned long long m = __ballot(hit >= 0);
        if (!m) continue;
        double term = 0.0;
        if (hit >= 0) {
            const double vi = qv[hit], wi = kv[i];
            term = fabs(vi - wi) - fabs(vi) - fabs(wi);
        }
        if (r.count == 0) r.first = __shfl(hit, __ffsll(m) - 1, 64);
        r.count += (int)__popcll(m);
        while (m) {   // lane order = ascending word order; a word that is not common adds nothing
            const int b = __ffsll(m) - 1;
            m &= m - 1;
            r.sum += __shfl(term, b, 64);
        }
    }
    return r;
}

__device__ __forceinline__ float l1_score(double sum) { return (float)(-sum / 2.0); }

// the query's BowVector into LDS; returns its length.  Ends in a barrier.
__device__ __forceinline__ int stage_query(const BowSet& B, int f, uint32_t* s_w, double* s_v)
{
    const uint32_t* w; const double* v;
    const int n = min(bow_of(B, f, w, v), ORBFE_KFDB_MAX_WORDS);
    for (int i = threadIdx.x; i < n; i += KD_THREADS) { s_w[i] = w[i]; s_v[i] = v[i]; }
    __syncthreads();
    return n;
}

struct KfdbArgs {
    BowSet B;
    const int32_t* db;
    const uint8_t* active;
    int K;
    const int32_t* query;
    const int32_t* neigh;
    const int32_t* conn_offsets;
    const int32_t* conn;
    const float* min_score;
    float* scores;
    int32_t* candidates;
    int32_t* common;
    uint32_t* scratch;
    orbfe_kfdb_result* res;
    int mode;
};

__global__ __launch_bounds__(KD_THREADS) void k_kfdb_score(KfdbArgs a)
{
    __shared__ uint32_t s_w[ORBFE_KFDB_MAX_WORDS];
    __shared__ double s_v[ORBFE_KFDB_MAX_WORDS];
    const int q = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nqw = stage_query(a.B, a.query[q], s_w, s_v);
    for (int kk = wv; kk < KD_KF_PER_WG; kk += KD_WAVES) {
        const int k = blockIdx.x * KD_KF_PER_WG + kk;
        if (k >= a.K) break;
        uint32_t packed = 0;
        float sc = 0.f;
        if (!a.active || a.active[k]) {
            const uint32_t* kw; const double* kv;
            const int nk = bow_of(a.B, a.db ? a.db[k] : k, kw, kv);
            const L1Common r = l1_common(s_w, s_v, nqw, kw, kv, nk, lane);
            if (r.count) {
                packed = ((uint32_t)r.first << KD_CNT_BITS) | (uint32_t)r.count;
                sc = l1_score(r.sum);
            }
        }
        if (lane == 0) {
            a.common[(size_t)q * a.K + k] = (int32_t)packed;
            a.scratch[(size_t)q * a.K + k] = __float_as_uint(sc);
        }
    }
}

// The rank of this thread's flag among the workgroup's flags in thread order, counted from `base`; `base` moves on by their number.
// Every thread of the workgroup calls it.
__device__ __forceinline__ int wg_rank(bool flag, int* s_cnt, int& base)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    __syncthreads();   // the readers of the previous round are done
    if (lane == 0) s_cnt[wv] = (int)__popcll(b);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < KD_WAVES; w++) {
        const int c = s_cnt[w];
        total += c;
        if (w < wv) before += c;
    }
    const int r = base + before + (int)__popcll(b & ((1ull << lane) - 1ull));
    base += total;
    return r;
}

// (value, index): the greater value, the earlier index among equal ones -- a serial scan with a strict > in index order
struct Best { float v; int i; };
__device__ __forceinline__ void take_greater(Best& a, const Best& b) { if (b.v > a.v || (b.v == a.v && b.i < a.i)) a = b; }
__device__ __forceinline__ void take_less(Best& a, const Best& b) { if (b.v < a.v || (b.v == a.v && b.i < a.i)) a = b; }

__device__ __forceinline__ void write_record(const KfdbArgs& a, int q, int n_sharing, int maxc, int minc, int n_scored, int n_kept, int n_cand,
                                             float best_acc, float retain, int status)
{
    orbfe_kfdb_result r;
    r.n_sharing = n_sharing; r.max_common_words = maxc; r.min_common_words = minc; r.n_scored = n_scored; r.n_kept = n_kept;
    r.n_candidates = n_cand; r.best_acc_score = best_acc; r.min_score_to_retain = retain; r.status = status;
    a.res[q] = r;
}

// P = the power of two the keys are sorted in: >= K.  Dynamic LDS: keys, accScore, pBestKF, P entries each.
__global__ __launch_bounds__(KD_THREADS) void k_kfdb_select(KfdbArgs a, int P)
{
    extern __shared__ __align__(16) unsigned char kd_smem[];
    uint32_t* keys = (uint32_t*)kd_smem;
    float* acc = (float*)(keys + P);
    int32_t* best = (int32_t*)(acc + P);
    __shared__ int s_cnt[KD_WAVES], s_n, s_max, s_scored, s_bad, s_bi[KD_WAVES];
    __shared__ float s_bv[KD_WAVES];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, K = a.K;
    const bool loop = a.mode == ORBFE_KFDB_LOOP;
    int32_t* common = a.common + (size_t)q * K;
    uint32_t* scratch = a.scratch + (size_t)q * K;
    float* scores = a.scores + (size_t)q * K;
    int32_t* cand = a.candidates + (size_t)q * K;
    if (tid == 0) { s_n = 0; s_max = 0; s_scored = 0; s_bad = 0; }
    __syncthreads();

    // GetConnectedKeyFrames(): never in the sharing list
    float min_score = 0.f;
    if (loop) {
        min_score = a.min_score[q];
        const int c0 = a.conn_offsets[q], c1 = a.conn_offsets[q + 1];
        if (c0 < 0 || c1 < c0) { if (tid == 0) s_bad = 1; }
        else
            for (int i = c0 + tid; i < c1; i += KD_THREADS) {
                const int p = a.conn[i];
                if (p < 0 || p >= K) s_bad = 1;
            }
        __syncthreads();
        if (s_bad) {   // a skipped query
            for (int k = tid; k < K; k += KD_THREADS) common[k] = 0;
            if (tid == 0) write_record(a, q, 0, 0, 0, 0, 0, 0, 0.f, 0.f, ORBFE_ERR_INVALID);
            return;
        }
        for (int i = c0 + tid; i < c1; i += KD_THREADS) common[a.conn[i]] = 0;
        __syncthreads();
    }

    // lKFsSharingWords, in any order; maxCommonWords
    for (int k = tid; k < K; k += KD_THREADS) {
        const uint32_t pk = (uint32_t)common[k];
        const int cnt = (int)(pk & KD_CNT_MASK);
        if (cnt) {
            atomicMax(&s_max, cnt);
            keys[atomicAdd(&s_n, 1)] = ((pk >> KD_CNT_BITS) << KD_POS_BITS) | (uint32_t)k;
        }
    }
    __syncthreads();
    const int n = s_n, maxc = s_max;
    if (n == 0) {   // every count is zero already
        if (tid == 0) write_record(a, q, 0, 0, 0, 0, 0, 0, 0.f, 0.f, ORBFE_OK);
        return;
    }
    const int minc = (int)(maxc * 0.8f);

    // the list's order: ascending (first common word, position)
    int P2 = 2;
    while (P2 < n) P2 <<= 1;
    for (int i = n + tid; i < P2; i += KD_THREADS) keys[i] = 0xffffffffu;
    for (int size = 2; size <= P2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < (P2 >> 1); t += KD_THREADS) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const uint32_t x = keys[lo], y = keys[hi];
                if ((x > y) == ((lo & size) == 0)) { keys[lo] = y; keys[hi] = x; }
            }
        }
    __syncthreads();

    // the word-count gate: score committed; the min_score gate: kept, in list order (best[] holds the kept positions for now)
    int n_kept = 0;
    for (int i0 = 0; i0 < n; i0 += KD_THREADS) {
        const int i = i0 + tid;
        bool kept = false;
        int k = 0;
        if (i < n) {
            k = (int)(keys[i] & KD_POS_MASK);
            if ((int)((uint32_t)common[k] & KD_CNT_MASK) > minc) {
                const float si = __uint_as_float(scratch[k]);
                scores[k] = si;
                atomicAdd(&s_scored, 1);
                kept = !loop || si >= min_score;
            }
        }
        const int pos = wg_rank(kept, s_cnt, n_kept);
        if (kept) best[pos] = k;
    }
    __syncthreads();
    // d_common as the caller reads it: the counts
    for (int k = tid; k < K; k += KD_THREADS) common[k] = (int32_t)((uint32_t)common[k] & KD_CNT_MASK);
    __syncthreads();   // the committed scores and the counts are visible to the workgroup from here
    const int n_scored = s_scored;
    if (n_kept == 0) {
        if (tid == 0) write_record(a, q, n, maxc, minc, n_scored, 0, 0, 0.f, 0.f, ORBFE_OK);
        return;
    }

    // accumulate over the covisible keyframes
    Best top{loop ? min_score : 0.f, -1};
    for (int j = tid; j < n_kept; j += KD_THREADS) {
        const int k = best[j];
        const float si = scores[k];
        float best_score = si, acc_score = si;
        int pbest = k;
        for (int t = 0; t < ORBFE_KFDB_NEIGHBOURS; t++) {
            const int nb = a.neigh[(size_t)k * ORBFE_KFDB_NEIGHBOURS + t];
            if (nb < 0 || nb >= K) continue;
            const int c = common[nb];   // 0: not in the sharing list (not met, erased, connected)
            if (loop ? c <= minc : c <= 0) continue;
            const float s2 = scores[nb];
            acc_score += s2;
            if (s2 > best_score) { pbest = nb; best_score = s2; }
        }
        acc[j] = acc_score;
        best[j] = pbest;
        take_greater(top, Best{acc_score, j});
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const Best o{__shfl_xor(top.v, off, 64), __shfl_xor(top.i, off, 64)};
        take_greater(top, o);
    }
    if (lane == 0) { s_bv[wv] = top.v; s_bi[wv] = top.i; }
    __syncthreads();
    top = Best{s_bv[0], s_bi[0]};
    for (int w = 1; w < KD_WAVES; w++) take_greater(top, Best{s_bv[w], s_bi[w]});
    const float best_acc = top.v, retain = 0.75f * best_acc;

    // the retained entries' pBestKF, first occurrences, in entry order.  The scores in d_scratch have been used: it now holds,
    // for each pBestKF of a retained entry, the first entry that names it
    for (int j = tid; j < n_kept; j += KD_THREADS)
        if (acc[j] > retain) scratch[best[j]] = 0xffffffffu;
    __syncthreads();
    for (int j = tid; j < n_kept; j += KD_THREADS)
        if (acc[j] > retain) atomicMin(&scratch[best[j]], (uint32_t)j);
    __syncthreads();
    int n_cand = 0;
    for (int j0 = 0; j0 < n_kept; j0 += KD_THREADS) {
        const int j = j0 + tid;
        const bool first = j < n_kept && acc[j] > retain && scratch[best[j]] == (uint32_t)j;
        const int pos = wg_rank(first, s_cnt, n_cand);
        if (first) cand[pos] = best[j];
    }
    if (tid == 0) write_record(a, q, n, maxc, minc, n_scored, n_kept, n_cand, best_acc, retain, ORBFE_OK);
}

// DetectLoop's minScore: one workgroup per query, one wave per connected keyframe
__global__ __launch_bounds__(KD_THREADS) void k_bow_min_score(BowSet B, const int32_t* db, const uint8_t* active, int K, const int32_t* query,
                                                             const int32_t* conn_offsets, const int32_t* conn, float* out)
{
    __shared__ uint32_t s_w[ORBFE_KFDB_MAX_WORDS];
    __shared__ double s_v[ORBFE_KFDB_MAX_WORDS];
    __shared__ float s_bv[KD_WAVES];
    __shared__ int s_bi[KD_WAVES];
    const int q = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nqw = stage_query(B, query[q], s_w, s_v);
    const int c0 = conn_offsets[q], c1 = conn_offsets[q + 1];
    Best low{1.0f, -1};
    for (int i = max(c0, 0) + wv; i < c1; i += KD_WAVES) {
        const int p = conn[i];
        if (p < 0 || p >= K || (active && !active[p])) continue;
        const uint32_t* kw; const double* kv;
        const int nk = bow_of(B, db ? db[p] : p, kw, kv);
        const L1Common r = l1_common(s_w, s_v, nqw, kw, kv, nk, lane);
        take_less(low, Best{l1_score(r.sum), i});
    }
    if (lane == 0) { s_bv[wv] = low.v; s_bi[wv] = low.i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        low = Best{s_bv[0], s_bi[0]};
        for (int w = 1; w < KD_WAVES; w++) take_less(low, Best{s_bv[w], s_bi[w]});
        out[q] = low.v;
    }
}

// the raw scores: one wave per pair
__global__ __launch_bounds__(KD_THREADS) void k_bow_score_pairs(BowSet B, const int32_t* pair1, const int32_t* pair2, int npairs, float* out)
{
    const int p = blockIdx.x * KD_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= npairs) return;
    const uint32_t *w1, *w2; const double *v1, *v2;
    const int n1 = bow_of(B, pair1[p], w1, v1), n2 = bow_of(B, pair2[p], w2, v2);
    const L1Common r = l1_common(w1, v1, n1, w2, v2, n2, lane);
    if (lane == 0) out[p] = l1_score(r.sum);
}

// ------------------------------------------------------------------------------------------- host --
int check_scoring(int scoring, const char* name)
{
    if (scoring != 0) return fail(ORBFE_ERR_INVALID, "%s: scoring %d is not L1_NORM (0), the only one built", name, scoring);
    return ORBFE_OK;
}

int launch_query(const KfdbArgs& a, int nq, hipStream_t s)
{
    int P = KD_THREADS;
    while (P < a.K) P <<= 1;
    const size_t lds = (size_t)P * 12;
    int rc = ensure_dyn_lds((const void*)k_kfdb_select, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k_kfdb_score, dim3((a.K + KD_KF_PER_WG - 1) / KD_KF_PER_WG, nq), dim3(KD_THREADS), 0, s, a);
    ORBFE_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_kfdb_select, dim3(nq), dim3(KD_THREADS), lds, s, a, P);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

// a CSR set of BowVectors as the host calls take it
int check_bow_csr(const int32_t* offsets, const uint32_t* word, const double* value, int nframes, const char* name)
{
    if (offsets[0] != 0) return fail(ORBFE_ERR_INVALID, "%s: offsets[0] = %d, not 0", name, offsets[0]);
    for (int f = 0; f < nframes; f++) {
        if (offsets[f + 1] < offsets[f]) return fail(ORBFE_ERR_INVALID, "%s: offsets decrease at %d", name, f);
        if (offsets[f + 1] > offsets[f] && (!word || !value)) return fail(ORBFE_ERR_INVALID, "%s: NULL word or value", name);
        for (int i = offsets[f]; i < offsets[f + 1]; i++) {
            if (i > offsets[f] && word[i] <= word[i - 1]) return fail(ORBFE_ERR_INVALID, "%s: the words of BowVector %d are not strictly ascending", name, f);
            if (!std::isfinite(value[i])) return fail(ORBFE_ERR_INVALID, "%s: BowVector %d has a value that is not finite", name, f);
        }
    }
    return ORBFE_OK;
}

} // namespace
} // namespace orbfe

using namespace orbfe;

extern "C" int orbfe_detect_candidates_batch_device(int mode, int scoring, const uint32_t* d_bow_word, const double* d_bow_value,
                                                    const int32_t* d_nbow, int capacity, const int32_t* d_db, const uint8_t* d_active, int K,
                                                    const int32_t* d_query, int nq, const int32_t* d_neigh, const int32_t* d_conn_offsets,
                                                    const int32_t* d_conn, const float* d_min_score, float* d_scores, int32_t* d_candidates,
                                                    int32_t* d_common, uint32_t* d_scratch, orbfe_kfdb_result* d_res, void* stream)
{
    static const char* name = "orbfe_detect_candidates_batch_device";
    if (mode != ORBFE_KFDB_LOOP && mode != ORBFE_KFDB_RELOC) return fail(ORBFE_ERR_INVALID, "%s: unknown mode %d", name, mode);
    int rc = check_scoring(scoring, name);
    if (rc) return rc;
    if (!d_bow_word || !d_bow_value || !d_nbow || !d_query || !d_neigh || !d_scores || !d_candidates || !d_common || !d_scratch || !d_res ||
        capacity <= 0 || K <= 0 || nq < 0 || (mode == ORBFE_KFDB_LOOP && (!d_conn_offsets || !d_conn || !d_min_score)))
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument (NULL pointer or non-positive size)", name);
    if (K > ORBFE_KFDB_MAX_KEYFRAMES || capacity > ORBFE_KFDB_MAX_WORDS)
        return fail(ORBFE_ERR_CAPACITY, "%s: K = %d, capacity = %d: at most %d keyframes of %d words", name, K, capacity, ORBFE_KFDB_MAX_KEYFRAMES,
                    ORBFE_KFDB_MAX_WORDS);
    if (nq == 0) return ORBFE_OK;
    if (nq > 65535) return fail(ORBFE_ERR_CAPACITY, "%s: nq = %d: at most 65535 queries a call", name, nq);
    KfdbArgs a{};
    a.B = BowSet{d_bow_word, d_bow_value, d_nbow, nullptr, capacity};
    a.db = d_db; a.active = d_active; a.K = K; a.query = d_query; a.neigh = d_neigh; a.conn_offsets = d_conn_offsets; a.conn = d_conn;
    a.min_score = d_min_score; a.scores = d_scores; a.candidates = d_candidates; a.common = d_common; a.scratch = d_scratch; a.res = d_res;
    a.mode = mode;
    return launch_query(a, nq, (hipStream_t)stream);
}

extern "C" int orbfe_detect_candidates(int mode, int scoring, const uint32_t* q_word, const double* q_value, int nbow, const int32_t* offsets,
                                       const uint32_t* word, const double* value, const uint8_t* active, int K, const int32_t* neigh,
                                       const int32_t* connected, int nconn, float min_score, float* scores, int32_t* candidates,
                                       int32_t* common, orbfe_kfdb_result* res, int device)
{
    static const char* name = "orbfe_detect_candidates";
    if (mode != ORBFE_KFDB_LOOP && mode != ORBFE_KFDB_RELOC) return fail(ORBFE_ERR_INVALID, "%s: unknown mode %d", name, mode);
    const bool loop = mode == ORBFE_KFDB_LOOP;
    int rc = check_scoring(scoring, name);
    if (rc) return rc;
    if (!res || nbow < 0 || K < 0 || (nbow && (!q_word || !q_value)) || !offsets || (K && (!neigh || !scores || !candidates)) ||
        (loop && (nconn < 0 || (nconn && !connected))))
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument (NULL pointer or negative size)", name);
    if ((rc = check_bow_csr(offsets, word, value, K, name))) return rc;
    const size_t T = (size_t)offsets[K];
    for (int i = 0; i < nbow; i++) {
        if (i && q_word[i] <= q_word[i - 1]) return fail(ORBFE_ERR_INVALID, "%s: the query's words are not strictly ascending", name);
        if (!std::isfinite(q_value[i])) return fail(ORBFE_ERR_INVALID, "%s: the query has a value that is not finite", name);
    }
    for (size_t i = 0; i < (size_t)K * ORBFE_KFDB_NEIGHBOURS; i++)
        if (neigh[i] >= K) return fail(ORBFE_ERR_INVALID, "%s: neigh[%zu] = %d is not below K = %d", name, i, neigh[i], K);
    if (loop) {
        if (!std::isfinite(min_score)) return fail(ORBFE_ERR_INVALID, "%s: min_score is not finite", name);
        for (int i = 0; i < nconn; i++)
            if (connected[i] < 0 || connected[i] >= K) return fail(ORBFE_ERR_INVALID, "%s: connected[%d] = %d is not in [0, K)", name, i, connected[i]);
    }
    if (K > ORBFE_KFDB_MAX_KEYFRAMES || nbow > ORBFE_KFDB_MAX_WORDS)
        return fail(ORBFE_ERR_CAPACITY, "%s: K = %d, nbow = %d: at most %d keyframes, %d query words", name, K, nbow, ORBFE_KFDB_MAX_KEYFRAMES,
                    ORBFE_KFDB_MAX_WORDS);
    if (T + (size_t)nbow > 0x7fffffffull) return fail(ORBFE_ERR_CAPACITY, "%s: more than 2^31 words", name);
    if ((rc = use_device(device))) return rc;
    if (K == 0) {
        *res = orbfe_kfdb_result{};
        return ORBFE_OK;
    }
    HostStage& w = match_host_stage();
    const size_t Kz = (size_t)K, W = T + (size_t)nbow, nc = loop ? (size_t)nconn : 0;
    // device io: [offsets K + 2 (the query is frame K) | word | value | active | neigh | conn offsets 2 | conn | min_score | query index]
    //            [scores, in/out] [candidates | common | record]
    IoLayout l;
    const size_t i_off = l.take((Kz + 2) * 4), i_w = l.take(W * 4), i_v = l.take(W * 8), i_act = l.take(active ? Kz : 0),
                 i_ng = l.take(Kz * ORBFE_KFDB_NEIGHBOURS * 4), i_co = l.take(8), i_c = l.take(nc * 4), i_ms = l.take(4), i_q = l.take(4);
    l.inout();
    const size_t io_sc = l.take(Kz * 4);
    l.outputs();
    const size_t o_cand = l.take(Kz * 4), o_com = l.take(Kz * 4), o_res = l.take(sizeof(orbfe_kfdb_result));
    if ((rc = w.begin(l)) || (rc = w.host_scratch.ensure(Kz * 4))) return rc;
    w.put(i_off, offsets, (Kz + 1) * 4);
    w.host<int32_t>(i_off)[K + 1] = (int32_t)W;
    w.put(i_w, word, T * 4); w.put(i_w + T * 4, q_word, (size_t)nbow * 4);
    w.put(i_v, value, T * 8); w.put(i_v + T * 8, q_value, (size_t)nbow * 8);
    w.put(i_act, active, Kz);
    w.put(i_ng, neigh, Kz * ORBFE_KFDB_NEIGHBOURS * 4);
    const int32_t co[2] = {0, (int32_t)nc}, qi = K;
    w.put(i_co, co, 8); w.put(i_c, connected, nc * 4); w.put(i_ms, &min_score, 4); w.put(i_q, &qi, 4);
    w.put(io_sc, scores, Kz * 4);
    if ((rc = w.upload())) return rc;
    KfdbArgs a{};
    a.B = BowSet{w.dev<const uint32_t>(i_w), w.dev<const double>(i_v), nullptr, w.dev<const int32_t>(i_off), ORBFE_KFDB_MAX_WORDS};
    a.active = active ? w.dev<const uint8_t>(i_act) : nullptr;
    a.K = K; a.query = w.dev<const int32_t>(i_q); a.neigh = w.dev<const int32_t>(i_ng);
    a.conn_offsets = w.dev<const int32_t>(i_co); a.conn = w.dev<const int32_t>(i_c); a.min_score = w.dev<const float>(i_ms);
    a.scores = w.dev<float>(io_sc); a.candidates = w.dev<int32_t>(o_cand); a.common = w.dev<int32_t>(o_com);
    a.scratch = w.host_scratch.as<uint32_t>(); a.res = w.dev<orbfe_kfdb_result>(o_res);
    a.mode = mode;
    if ((rc = launch_query(a, 1, w.stream)) || (rc = w.download()) || (rc = w.sync())) return rc;
    *res = *w.host<const orbfe_kfdb_result>(o_res);
    w.get(scores, io_sc, Kz * 4);
    w.get(candidates, o_cand, (size_t)res->n_candidates * 4);
    w.get(common, o_com, Kz * 4);
    return ORBFE_OK;
}

extern "C" int orbfe_bow_min_score_batch_device(int scoring, const uint32_t* d_bow_word, const double* d_bow_value, const int32_t* d_nbow,
                                                int capacity, const int32_t* d_db, const uint8_t* d_active, int K, const int32_t* d_query, int nq,
                                                const int32_t* d_conn_offsets, const int32_t* d_conn, float* d_min_score, void* stream)
{
    static const char* name = "orbfe_bow_min_score_batch_device";
    int rc = check_scoring(scoring, name);
    if (rc) return rc;
    if (!d_bow_word || !d_bow_value || !d_nbow || !d_query || !d_conn_offsets || !d_conn || !d_min_score || capacity <= 0 || K <= 0 || nq < 0)
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument (NULL pointer or non-positive size)", name);
    if (capacity > ORBFE_KFDB_MAX_WORDS) return fail(ORBFE_ERR_CAPACITY, "%s: capacity = %d: at most %d words", name, capacity, ORBFE_KFDB_MAX_WORDS);
    if (nq == 0) return ORBFE_OK;
    hipLaunchKernelGGL(k_bow_min_score, dim3(nq), dim3(KD_THREADS), 0, (hipStream_t)stream, BowSet{d_bow_word, d_bow_value, d_nbow, nullptr, capacity},
                       d_db, d_active, K, d_query, d_conn_offsets, d_conn, d_min_score);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" int orbfe_bow_score_batch_device(int scoring, const uint32_t* d_bow_word, const double* d_bow_value, const int32_t* d_nbow, int capacity,
                                            const int32_t* d_pair1, const int32_t* d_pair2, int npairs, float* d_scores, void* stream)
{
    static const char* name = "orbfe_bow_score_batch_device";
    int rc = check_scoring(scoring, name);
    if (rc) return rc;
    if (!d_bow_word || !d_bow_value || !d_nbow || !d_pair1 || !d_pair2 || !d_scores || capacity <= 0 || npairs < 0)
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument (NULL pointer or non-positive size)", name);
    if (npairs == 0) return ORBFE_OK;
    hipLaunchKernelGGL(k_bow_score_pairs, dim3((npairs + KD_WAVES - 1) / KD_WAVES), dim3(KD_THREADS), 0, (hipStream_t)stream,
                       BowSet{d_bow_word, d_bow_value, d_nbow, nullptr, capacity}, d_pair1, d_pair2, npairs, d_scores);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" int orbfe_bow_score(int scoring, const int32_t* offsets, const uint32_t* word, const double* value, int nframes, const int32_t* pair1,
                               const int32_t* pair2, int npairs, float* scores, int device)
{
    static const char* name = "orbfe_bow_score";
    int rc = check_scoring(scoring, name);
    if (rc) return rc;
    if (!offsets || nframes < 0 || npairs < 0 || (npairs && (!pair1 || !pair2 || !scores)))
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument (NULL pointer or negative size)", name);
    if ((rc = check_bow_csr(offsets, word, value, nframes, name))) return rc;
    for (int p = 0; p < npairs; p++)
        if (pair1[p] < 0 || pair1[p] >= nframes || pair2[p] < 0 || pair2[p] >= nframes)
            return fail(ORBFE_ERR_INVALID, "%s: pair %d = (%d, %d) is not inside [0, %d)", name, p, pair1[p], pair2[p], nframes);
    if ((rc = use_device(device))) return rc;
    if (npairs == 0) return ORBFE_OK;
    HostStage& w = match_host_stage();
    const size_t F = (size_t)nframes, T = (size_t)offsets[nframes], NP = (size_t)npairs;
    IoLayout l;
    const size_t i_off = l.take((F + 1) * 4), i_w = l.take(T * 4), i_v = l.take(T * 8), i_p1 = l.take(NP * 4), i_p2 = l.take(NP * 4);
    l.outputs();
    const size_t o_s = l.take(NP * 4);
    if ((rc = w.begin(l))) return rc;
    w.put(i_off, offsets, (F + 1) * 4); w.put(i_w, word, T * 4); w.put(i_v, value, T * 8);
    w.put(i_p1, pair1, NP * 4); w.put(i_p2, pair2, NP * 4);
    if ((rc = w.upload())) return rc;
    hipLaunchKernelGGL(k_bow_score_pairs, dim3((npairs + KD_WAVES - 1) / KD_WAVES), dim3(KD_THREADS), 0, w.stream,
                       BowSet{w.dev<const uint32_t>(i_w), w.dev<const double>(i_v), nullptr, w.dev<const int32_t>(i_off), 0},
                       w.dev<const int32_t>(i_p1), w.dev<const int32_t>(i_p2), npairs, w.dev<float>(o_s));
    ORBFE_HIP(hipGetLastError());
    if ((rc = w.download()) || (rc = w.sync())) return rc;
    w.get(scores, o_s, NP * 4);
    return ORBFE_OK;
}
