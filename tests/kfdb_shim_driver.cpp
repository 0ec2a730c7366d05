// kfdb_shim_driver.cpp -- drives a KeyFrameDatabase through the class interface of include/KeyFrameDatabase.h (test infrastructure).
// Linked with include/shims/KeyFrameDatabase_orbfe.cc it runs the library; tests/gen_kfdb_golden.py links the same source with the
// reference's own KeyFrameDatabase.cc (-DKFDB_REFERENCE: the vocabulary then scores with DBoW2's L1Scoring) to record what the
// tests expect.
//   kfdb_shim_driver script        a mock map of 40 keyframes: add, both queries, erase, a repeated relocalization query, clear
//   kfdb_shim_driver cull          9000 add() calls with all but the last 30 keyframes erased again, three queries on the way
//   kfdb_shim_driver case FILE     one query on a case of tests/kfdb_cases.py (FILE: kfdb_cases.dump); the keyframes' score fields
//                                  start from the case's state, so this mode means something with the reference only
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "KeyFrameDatabase.h"
#ifdef KFDB_REFERENCE
#include "Thirdparty/DBoW2/DBoW2/ScoringObject.h"
#endif

using namespace ORB_SLAM2;

static double score_l1(const DBoW2::BowVector& a, const DBoW2::BowVector& b)
{
#ifdef KFDB_REFERENCE
    static DBoW2::L1Scoring scoring;
    return scoring.score(a, b);
#else
    double s = 0;
    for (DBoW2::BowVector::const_iterator it = a.begin(); it != a.end(); ++it) {
        DBoW2::BowVector::const_iterator f = b.find(it->first);
        if (f != b.end()) s += fabs(it->second - f->second) - fabs(it->second) - fabs(f->second);
    }
    return -s / 2.0;
#endif
}

static uint32_t g_x = 12345u;
static uint32_t rnd() { g_x = g_x * 1664525u + 1013904223u; return g_x >> 8; }

// nw distinct words out of [lo, lo + span), positive values with sum 1
static DBoW2::BowVector sliding_bow(unsigned lo, unsigned span, int nw)
{
    DBoW2::BowVector bv;
    while ((int)bv.size() < nw) bv[lo + rnd() % span] = 0.05 + (rnd() % 1000) / 1000.0;
    double sum = 0;
    for (DBoW2::BowVector::iterator it = bv.begin(); it != bv.end(); ++it) sum += it->second;
    for (DBoW2::BowVector::iterator it = bv.begin(); it != bv.end(); ++it) it->second /= sum;
    return bv;
}

static void print_ids(const char* what, const std::vector<KeyFrame*>& v)
{
    printf("%s:", what);
    for (size_t i = 0; i < v.size(); i++) printf(" %lu", v[i]->mnId);
    printf("\n");
}

static float detect_loop_min_score(KeyFrame* cur)
{
    const std::vector<KeyFrame*> vpConnected = cur->GetVectorCovisibleKeyFrames();
    float minScore = 1;
    for (size_t i = 0; i < vpConnected.size(); i++) {
        if (vpConnected[i]->isBad()) continue;
        float score = score_l1(cur->mBowVec, vpConnected[i]->mBowVec);
        if (score < minScore) minScore = score;
    }
    return minScore;
}

static int run_script()
{
    const int N = 50, SPAN = 160, SLIDE = 12, NW = 70;
    ORBVocabulary voc(1u << 16, score_l1);
    KeyFrameDatabase db(voc);
    std::vector<KeyFrame> kfs(N);
    for (int k = 0; k < N; k++) {
        const int at = k < 40 ? k : k - 40;   // 40 .. 49: a second map over the start of the first one's trajectory
        kfs[k].mnId = 100 + k;
        kfs[k].mBowVec = sliding_bow(1000 + at * SLIDE, SPAN, NW);
    }
    // covisibility: the keyframes at distance 1, 2, 3, ... inside the same map, nearest first, a few left out
    for (int k = 0; k < N; k++)
        for (int d = 1; d <= 7; d++)
            for (int s = -1; s <= 1; s += 2) {
                const int o = k + s * d;
                if (o < 0 || o >= N || (o < 40) != (k < 40) || rnd() % 5 == 0) continue;
                kfs[k].mvpOrderedConnectedKeyFrames.push_back(&kfs[o]);
            }
    Frame f1, f2, f3;
    f1.mBowVec = sliding_bow(1000 + 12 * SLIDE, SPAN, NW);
    f2.mBowVec = sliding_bow(1000 + 20 * SLIDE, SPAN, NW);
    f3.mBowVec = sliding_bow(1000 + 4 * SLIDE, SPAN, NW);

    for (int k = 0; k < 30; k++) db.add(&kfs[k]);
    f1.mnId = 1001;
    print_ids("reloc f1", db.DetectRelocalizationCandidates(&f1));
    // a loop query whose own neighbourhood is far away: keyframe 30 looks at the map's start through a BowVector from there
    kfs[30].mBowVec = sliding_bow(1000 + 6 * SLIDE, SPAN, NW);
    const float min30 = detect_loop_min_score(&kfs[30]);
    print_ids("loop kf30", db.DetectLoopCandidates(&kfs[30], min30 < 0.05f ? min30 : 0.05f));
    db.add(&kfs[30]);
    db.erase(&kfs[12]);
    kfs[12].mbBad = true;
    db.erase(&kfs[13]);
    kfs[13].mbBad = true;
    f1.mnId = 1002;
    print_ids("reloc f1 again", db.DetectRelocalizationCandidates(&f1));
    f2.mnId = 1003;
    print_ids("reloc f2", db.DetectRelocalizationCandidates(&f2));
    db.add(&kfs[12]);   // back at the end of every word's list, with the score the queries before left it
    kfs[12].mbBad = false;
    f1.mnId = 1007;
    print_ids("reloc f1 after re-add", db.DetectRelocalizationCandidates(&f1));
    for (int k = 31; k < 39; k++) db.add(&kfs[k]);
    kfs[39].mBowVec = sliding_bow(1000 + 20 * SLIDE, SPAN, NW);
    print_ids("loop kf39", db.DetectLoopCandidates(&kfs[39], 0.02f));
    print_ids("loop kf39 high", db.DetectLoopCandidates(&kfs[39], 0.9f));
    db.clear();
    f3.mnId = 1004;
    print_ids("reloc f3 empty", db.DetectRelocalizationCandidates(&f3));
    for (int k = 40; k < 50; k++) db.add(&kfs[k]);
    f3.mnId = 1005;
    print_ids("reloc f3", db.DetectRelocalizationCandidates(&f3));
    f3.mnId = 1006;
    print_ids("reloc f3 again", db.DetectRelocalizationCandidates(&f3));
    return 0;
}

// more add() calls than a single call of the library takes keyframes, nearly all of them erased again (keyframe culling)
static int run_cull()
{
    const int N = 9000, ALIVE = 30;
    ORBVocabulary voc(1u << 16, score_l1);
    KeyFrameDatabase db(voc);
    std::vector<KeyFrame> kfs(N);
    for (int k = 0; k < N; k++) {
        kfs[k].mnId = k;
        kfs[k].mBowVec = sliding_bow(1000 + (k % 50) * 12, 160, 20);
        for (int d = 1; d <= 4; d++)
            if (k - d >= 0) kfs[k].mvpOrderedConnectedKeyFrames.push_back(&kfs[k - d]);
    }
    Frame f;
    f.mBowVec = sliding_bow(1000 + ((N - 10) % 50) * 12, 160, 40);
    for (int k = 0; k < N; k++) {
        db.add(&kfs[k]);
        if (k >= ALIVE) db.erase(&kfs[k - ALIVE]);
        if (k % 3000 == 2999) {
            f.mnId = 1 + k;
            print_ids("reloc", db.DetectRelocalizationCandidates(&f));
        }
    }
    return 0;
}

template <class T> static bool rd(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int run_cases(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    int32_t ncases = 0;
    if (fread(&ncases, 4, 1, f) != 1) return 2;
    for (int ci = 0; ci < ncases; ci++) {
        int32_t h[6];   // mode, K, nbow, total words, nconn, has_active
        if (fread(h, 4, 6, f) != 6) return 2;
        const int mode = h[0], K = h[1], nbow = h[2], T = h[3], nconn = h[4];
        std::vector<uint32_t> qw, word;
        std::vector<double> qv, value;
        std::vector<int32_t> offsets, neigh, connected;
        std::vector<uint8_t> active;
        std::vector<float> ms, scores;
        if (!rd(f, qw, nbow) || !rd(f, qv, nbow) || !rd(f, offsets, K + 1) || !rd(f, word, T) || !rd(f, value, T) || !rd(f, active, h[5] ? K : 0) ||
            !rd(f, neigh, (size_t)K * 10) || !rd(f, connected, nconn) || !rd(f, ms, 1) || !rd(f, scores, K))
            return 2;
        ORBVocabulary voc(1u << 20, score_l1);
        KeyFrameDatabase db(voc);
        std::vector<KeyFrame> kfs(K);
        KeyFrame outsider;   // stands for every neighbour that is not in the database
        outsider.mnId = 999999;
        const unsigned long id = 7;
        for (int k = 0; k < K; k++) {
            kfs[k].mnId = 1000 + k;
            for (int i = offsets[k]; i < offsets[k + 1]; i++) kfs[k].mBowVec[word[i]] = value[i];
            kfs[k].mLoopScore = kfs[k].mRelocScore = scores[k];
            for (int t = 0; t < 10; t++) {
                const int nb = neigh[k * 10 + t];
                kfs[k].mvpOrderedConnectedKeyFrames.push_back(nb >= 0 ? &kfs[nb] : &outsider);
            }
        }
        for (int k = 0; k < K; k++) db.add(&kfs[k]);
        if (h[5])
            for (int k = 0; k < K; k++)
                if (!active[k]) db.erase(&kfs[k]);
        std::vector<KeyFrame*> got;
        if (mode == 0) {
            KeyFrame q;
            q.mnId = id;
            for (int i = 0; i < nbow; i++) q.mBowVec[qw[i]] = qv[i];
            for (int i = 0; i < nconn; i++) q.mvpOrderedConnectedKeyFrames.push_back(&kfs[connected[i]]);
            got = db.DetectLoopCandidates(&q, ms[0]);
        } else {
            Frame q;
            q.mnId = id;
            for (int i = 0; i < nbow; i++) q.mBowVec[qw[i]] = qv[i];
            got = db.DetectRelocalizationCandidates(&q);
        }
        printf("case %d %d", ci, (int)got.size());
        for (size_t i = 0; i < got.size(); i++) printf(" %lu", got[i]->mnId - 1000);
        printf("\nscores");
        for (int k = 0; k < K; k++) {
            const float s = mode == 0 ? kfs[k].mLoopScore : kfs[k].mRelocScore;
            uint32_t u;
            memcpy(&u, &s, 4);
            printf(" %08x", u);
        }
        printf("\nwords");
        for (int k = 0; k < K; k++)
            printf(" %d", mode == 0 ? (kfs[k].mnLoopQuery == id ? kfs[k].mnLoopWords : 0) : (kfs[k].mnRelocQuery == id ? kfs[k].mnRelocWords : 0));
        printf("\n");
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "script")) return run_script();
    if (argc == 2 && !strcmp(argv[1], "cull")) return run_cull();
    if (argc == 3 && !strcmp(argv[1], "case")) return run_cases(argv[2]);
    fprintf(stderr, "usage: %s script | cull | case FILE\n", argv[0]);
    return 2;
}
