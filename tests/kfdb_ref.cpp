// kfdb_ref.cpp -- a single-threaded CPU restatement of KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates
// (src/KeyFrameDatabase.cc:76-309), of DetectLoop's minScore (src/LoopClosing.cc:232-246) and of DBoW2's L1Scoring::score
// (ScoringObject.cpp:23-68), driven over the flat arrays of include/orbfe.h.  Test infrastructure: it keeps the reference's
// containers (std::map BowVectors, a std::list per word of the inverted file, lists of pairs) and its statement order, so that
// the order of everything returned comes from the same walk.  tests/golden/kfdb_cases.npz pins it to the reference's own code.
#include <cmath>
#include <cstdint>
#include <list>
#include <map>
#include <set>
#include <vector>

namespace {

typedef std::map<unsigned int, double> BowVector;

struct KF {
    int pos;
    BowVector bow;
    long query;      // mnLoopQuery / mnRelocQuery
    int words;       // mnLoopWords / mnRelocWords
    std::vector<KF*> neigh;   // GetBestCovisibilityKeyFrames(10)
};

// what the reference holds between queries: the keyframes (their query fields included) and the inverted file
struct Database {
    std::vector<KF> kfs;
    std::map<unsigned int, std::list<KF*> > inverted;   // mvInvertedFile, only the words that occur
    long queries;
};

struct Result {
    int32_t n_sharing, max_common_words, min_common_words, n_scored, n_kept, n_candidates;
    float best_acc_score, min_score_to_retain;
    int32_t status;
};

double l1_score(const BowVector& v1, const BowVector& v2)
{
    BowVector::const_iterator v1_it = v1.begin(), v2_it = v2.begin();
    const BowVector::const_iterator v1_end = v1.end(), v2_end = v2.end();
    double score = 0;
    while (v1_it != v1_end && v2_it != v2_end) {
        const double& vi = v1_it->second;
        const double& wi = v2_it->second;
        if (v1_it->first == v2_it->first) {
            score += fabs(vi - wi) - fabs(vi) - fabs(wi);
            ++v1_it;
            ++v2_it;
        } else if (v1_it->first < v2_it->first)
            v1_it = v1.lower_bound(v2_it->first);
        else
            v2_it = v2.lower_bound(v1_it->first);
    }
    score = -score / 2.0;
    return score;
}

BowVector make_bow(const uint32_t* w, const double* v, int n)
{
    BowVector b;
    for (int i = 0; i < n; i++) b.insert(b.end(), std::make_pair(w[i], v[i]));
    return b;
}

} // namespace

extern "C" double kfdb_score(const uint32_t* w1, const double* v1, int n1, const uint32_t* w2, const double* v2, int n2)
{
    return l1_score(make_bow(w1, v1, n1), make_bow(w2, v2, n2));
}

// minScore of DetectLoop over the connected positions, in their order; an inactive keyframe is skipped (isBad())
extern "C" float kfdb_min_score(const uint32_t* qw, const double* qv, int nbow, const int32_t* offsets, const uint32_t* word,
                                const double* value, const uint8_t* active, int K, const int32_t* connected, int nconn)
{
    const BowVector cur = make_bow(qw, qv, nbow);
    float minScore = 1;
    for (int i = 0; i < nconn; i++) {
        const int p = connected[i];
        if (p < 0 || p >= K || (active && !active[p])) continue;
        const BowVector bv = make_bow(word + offsets[p], value + offsets[p], offsets[p + 1] - offsets[p]);
        float score = l1_score(cur, bv);
        if (score < minScore) minScore = score;
    }
    return minScore;
}

// The database from the flat arrays: add() of every keyframe in order, erase() of the inactive ones.
extern "C" Database* kfdb_open(const int32_t* offsets, const uint32_t* word, const double* value, const uint8_t* active, int K,
                               const int32_t* neigh)
{
    Database* db = new Database();
    db->queries = 0;
    db->kfs.resize(K);
    for (int k = 0; k < K; k++) {
        KF& kf = db->kfs[k];
        kf.pos = k;
        kf.bow = make_bow(word + offsets[k], value + offsets[k], offsets[k + 1] - offsets[k]);
        kf.query = 0;
        kf.words = 0;
        for (int t = 0; t < 10; t++) {
            const int nb = neigh[k * 10 + t];
            if (nb >= 0 && nb < K) kf.neigh.push_back(&db->kfs[nb]);
        }
        if (!active || active[k])   // an erased keyframe is in no list
            for (BowVector::const_iterator vit = kf.bow.begin(); vit != kf.bow.end(); vit++) db->inverted[vit->first].push_back(&kf);
    }
    return db;
}

extern "C" void kfdb_close(Database* db) { delete db; }

// One query.  scores[k] = mLoopScore / mRelocScore of keyframe k, the caller's state.  order[0 .. n_sharing) = lKFsSharingWords as
// positions.  extra[0] = retained entries (before the duplicates go), [1] = entries whose pBestKF is not their own keyframe,
// [2] = neighbour contributions of a score this call did not write (relocalization), [3] = kept scores equal to min_score (loop)
extern "C" int kfdb_query(Database* db, int mode, const uint32_t* qw, const double* qv, int nbow, const int32_t* connected, int nconn,
                          float minScore, float* scores, int32_t* candidates, int32_t* common, Result* res, int32_t* extra, int32_t* order)
{
    const bool loop = mode == 0;
    const long id = ++db->queries;
    std::vector<KF>& kfs = db->kfs;
    std::map<unsigned int, std::list<KF*> >& inverted = db->inverted;
    const int K = (int)kfs.size();
    const BowVector query = make_bow(qw, qv, nbow);
    std::set<KF*> spConnected;
    if (loop)
        for (int i = 0; i < nconn; i++) spConnected.insert(&kfs[connected[i]]);
    *res = Result();
    for (int i = 0; i < 4; i++) extra[i] = 0;
    for (int k = 0; k < K; k++) common[k] = 0;

    std::list<KF*> lKFsSharingWords;
    for (BowVector::const_iterator vit = query.begin(), vend = query.end(); vit != vend; vit++) {
        std::map<unsigned int, std::list<KF*> >::iterator f = inverted.find(vit->first);
        if (f == inverted.end()) continue;
        std::list<KF*>& lKFs = f->second;
        for (std::list<KF*>::iterator lit = lKFs.begin(), lend = lKFs.end(); lit != lend; lit++) {
            KF* pKFi = *lit;
            if (pKFi->query != id) {
                pKFi->words = 0;
                if (!loop || !spConnected.count(pKFi)) {
                    pKFi->query = id;
                    lKFsSharingWords.push_back(pKFi);
                }
            }
            pKFi->words++;
        }
    }
    res->n_sharing = (int32_t)lKFsSharingWords.size();
    if (lKFsSharingWords.empty()) return 0;

    int maxCommonWords = 0, nlist = 0;
    for (std::list<KF*>::iterator lit = lKFsSharingWords.begin(); lit != lKFsSharingWords.end(); lit++) {
        order[nlist++] = (*lit)->pos;
        common[(*lit)->pos] = (*lit)->words;
        if ((*lit)->words > maxCommonWords) maxCommonWords = (*lit)->words;
    }
    int minCommonWords = maxCommonWords * 0.8f;
    res->max_common_words = maxCommonWords;
    res->min_common_words = minCommonWords;

    std::list<std::pair<float, KF*> > lScoreAndMatch;
    std::set<KF*> scoredNow;
    int nscores = 0;
    for (std::list<KF*>::iterator lit = lKFsSharingWords.begin(); lit != lKFsSharingWords.end(); lit++) {
        KF* pKFi = *lit;
        if (pKFi->words > minCommonWords) {
            nscores++;
            float si = l1_score(query, pKFi->bow);
            scores[pKFi->pos] = si;
            scoredNow.insert(pKFi);
            if (!loop || si >= minScore) {
                lScoreAndMatch.push_back(std::make_pair(si, pKFi));
                if (loop && si == minScore) extra[3]++;
            }
        }
    }
    res->n_scored = nscores;
    res->n_kept = (int32_t)lScoreAndMatch.size();
    if (lScoreAndMatch.empty()) return 0;

    std::list<std::pair<float, KF*> > lAccScoreAndMatch;
    float bestAccScore = loop ? minScore : 0;
    for (std::list<std::pair<float, KF*> >::iterator it = lScoreAndMatch.begin(); it != lScoreAndMatch.end(); it++) {
        KF* pKFi = it->second;
        float bestScore = it->first;
        float accScore = it->first;
        KF* pBestKF = pKFi;
        for (std::vector<KF*>::iterator vit = pKFi->neigh.begin(); vit != pKFi->neigh.end(); vit++) {
            KF* pKF2 = *vit;
            if (loop) {
                if (!(pKF2->query == id && pKF2->words > minCommonWords)) continue;
            } else {
                if (pKF2->query != id) continue;
                if (!scoredNow.count(pKF2)) extra[2]++;
            }
            accScore += scores[pKF2->pos];
            if (scores[pKF2->pos] > bestScore) {
                pBestKF = pKF2;
                bestScore = scores[pKF2->pos];
            }
        }
        if (pBestKF != pKFi) extra[1]++;
        lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
        if (accScore > bestAccScore) bestAccScore = accScore;
    }

    float minScoreToRetain = 0.75f * bestAccScore;
    res->best_acc_score = bestAccScore;
    res->min_score_to_retain = minScoreToRetain;
    std::set<KF*> spAlreadyAddedKF;
    int n = 0;
    for (std::list<std::pair<float, KF*> >::iterator it = lAccScoreAndMatch.begin(); it != lAccScoreAndMatch.end(); it++) {
        if (it->first > minScoreToRetain) {
            extra[0]++;
            KF* pKFi = it->second;
            if (!spAlreadyAddedKF.count(pKFi)) {
                candidates[n++] = pKFi->pos;
                spAlreadyAddedKF.insert(pKFi);
            }
        }
    }
    res->n_candidates = n;
    return 0;
}

// open, one query, close
extern "C" int kfdb_detect(int mode, const uint32_t* qw, const double* qv, int nbow, const int32_t* offsets, const uint32_t* word,
                           const double* value, const uint8_t* active, int K, const int32_t* neigh, const int32_t* connected, int nconn,
                           float minScore, float* scores, int32_t* candidates, int32_t* common, Result* res, int32_t* extra,
                           int32_t* order)
{
    Database* db = kfdb_open(offsets, word, value, active, K, neigh);
    const int rc = kfdb_query(db, mode, qw, qv, nbow, connected, nconn, minScore, scores, candidates, common, res, extra, order);
    kfdb_close(db);
    return rc;
}
