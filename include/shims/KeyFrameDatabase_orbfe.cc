/*
 * KeyFrameDatabase_orbfe.cc (shim) -- KeyFrameDatabase (src/KeyFrameDatabase.cc) implemented on liborbfe.so.  Compile it INSTEAD of
 * src/KeyFrameDatabase.cc.  include/KeyFrameDatabase.h, KeyFrame, Frame and ORBVocabulary stay the reference's own;
 * the vocabulary must score with L1_NORM, as ORBvoc.txt declares.
 *
 * The class keeps no inverted file.  add() appends the keyframe and its BowVector to flat arrays (a "position" is the place in the
 * order of add() calls among the keyframes still in the database: it orders the keyframes inside every word's list of the
 * reference's inverted file), erase() clears the position's active flag, clear() empties everything.  The next query squeezes the
 * erased positions out before it uploads, so K is the number of keyframes alive, whatever was culled before; ORBFE_KFDB_MAX_KEYFRAMES
 * bounds that number.  A query walks the covisibility graph on the host -- GetConnectedKeyFrames() of the query keyframe and
 * GetBestCovisibilityKeyFrames(10) of every keyframe in the database, as positions -- makes ONE
 * orbfe_detect_candidates call, which uploads the whole database, and maps the positions back to KeyFrame*.  The reference's
 * per-keyframe query fields are not written: mLoopScore / mRelocScore live here as two float arrays (the state a relocalization
 * query reads from the queries before it, see include/orbfe.h), and nothing else in the reference reads mnLoopQuery, mnLoopWords
 * or their Reloc twins.  A keyframe that is added again after an erase keeps its two scores (eight bytes stay behind for every
 * erased keyframe until clear()).
 *
 * The arrays hang off the object's address in a table of this file, because the class declaration is the reference's.  The
 * constructor and clear() drop the address's entry; the class has no destructor to do it, so the entry of a database that is
 * destroyed without clear() stays until an object is constructed at that address again (one database per System).  Library errors
 * are thrown as std::runtime_error.
 */
#include "KeyFrameDatabase.h"

#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
#include "orbfe.h"

using namespace std;

namespace ORB_SLAM2
{

namespace
{

struct FlatDatabase {
    vector<KeyFrame*> kf;          // by position
    vector<int32_t> offsets;       // CSR of the BowVectors, positions + 1 entries
    vector<uint32_t> word;
    vector<double> value;
    vector<uint8_t> active;
    vector<float> loopScore, relocScore;
    map<KeyFrame*, int> where;     // the position of every keyframe in the arrays
    map<KeyFrame*, pair<float, float> > retired;   // the two scores of the keyframes squeezed out, for an add() after an erase()
    int erased;
    FlatDatabase() : offsets(1, 0), erased(0) {}
};

mutex gTableMutex;
map<const KeyFrameDatabase*, FlatDatabase> gTable;

FlatDatabase& flat(const KeyFrameDatabase* db)
{
    unique_lock<mutex> lock(gTableMutex);
    return gTable[db];
}

void bow_arrays(const DBoW2::BowVector& bv, vector<uint32_t>& w, vector<double>& v)
{
    for (DBoW2::BowVector::const_iterator vit = bv.begin(), vend = bv.end(); vit != vend; vit++) {
        w.push_back(vit->first);
        v.push_back(vit->second);
    }
}

// the erased positions out of every array, the order of the others kept
void squeeze(FlatDatabase& d)
{
    if (!d.erased) return;
    FlatDatabase n;
    for (size_t k = 0; k < d.kf.size(); k++) {
        if (!d.active[k]) {
            if (d.where[d.kf[k]] == (int)k) d.retired[d.kf[k]] = make_pair(d.loopScore[k], d.relocScore[k]);
            continue;
        }
        n.where[d.kf[k]] = (int)n.kf.size();
        n.kf.push_back(d.kf[k]);
        n.word.insert(n.word.end(), d.word.begin() + d.offsets[k], d.word.begin() + d.offsets[k + 1]);
        n.value.insert(n.value.end(), d.value.begin() + d.offsets[k], d.value.begin() + d.offsets[k + 1]);
        n.offsets.push_back((int32_t)n.word.size());
        n.active.push_back(1);
        n.loopScore.push_back(d.loopScore[k]);
        n.relocScore.push_back(d.relocScore[k]);
    }
    d.kf.swap(n.kf); d.offsets.swap(n.offsets); d.word.swap(n.word); d.value.swap(n.value); d.active.swap(n.active);
    d.loopScore.swap(n.loopScore); d.relocScore.swap(n.relocScore); d.where.swap(n.where);
    d.erased = 0;
}

vector<KeyFrame*> query(FlatDatabase& d, int mode, const DBoW2::BowVector& bv, const set<KeyFrame*>* spConnected, float minScore)
{
    squeeze(d);
    const int K = (int)d.kf.size();
    if (K == 0) return vector<KeyFrame*>();
    vector<uint32_t> qw;
    vector<double> qv;
    bow_arrays(bv, qw, qv);
    vector<int32_t> connected;
    if (spConnected)
        for (set<KeyFrame*>::const_iterator sit = spConnected->begin(); sit != spConnected->end(); sit++) {
            map<KeyFrame*, int>::const_iterator f = d.where.find(*sit);
            if (f != d.where.end()) connected.push_back(f->second);
        }
    vector<int32_t> neigh((size_t)K * ORBFE_KFDB_NEIGHBOURS, -1);
    for (int k = 0; k < K; k++) {
        const vector<KeyFrame*> vpNeighs = d.kf[k]->GetBestCovisibilityKeyFrames(ORBFE_KFDB_NEIGHBOURS);
        for (size_t i = 0; i < vpNeighs.size() && i < ORBFE_KFDB_NEIGHBOURS; i++) {
            map<KeyFrame*, int>::const_iterator f = d.where.find(vpNeighs[i]);
            if (f != d.where.end()) neigh[(size_t)k * ORBFE_KFDB_NEIGHBOURS + i] = f->second;
        }
    }
    vector<int32_t> candidates(K);
    orbfe_kfdb_result res;
    vector<float>& scores = mode == ORBFE_KFDB_LOOP ? d.loopScore : d.relocScore;
    const int rc = orbfe_detect_candidates(mode, 0 /* L1_NORM */, qw.data(), qv.data(), (int)qw.size(), d.offsets.data(), d.word.data(),
                                           d.value.data(), d.active.data(), K, neigh.data(), connected.data(), (int)connected.size(),
                                           minScore, scores.data(), candidates.data(), NULL, &res, 0);
    if (rc != ORBFE_OK) throw runtime_error(string("orbfe_detect_candidates: ") + orbfe_last_error());
    vector<KeyFrame*> vpCandidates;
    vpCandidates.reserve(res.n_candidates);
    for (int i = 0; i < res.n_candidates; i++) vpCandidates.push_back(d.kf[candidates[i]]);
    return vpCandidates;
}

} // namespace

KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary& voc) : mpVoc(&voc)
{
    unique_lock<mutex> lock(gTableMutex);
    gTable.erase(this);   // what a database destroyed at this address without clear() left behind
}

void KeyFrameDatabase::add(KeyFrame* pKF)
{
    unique_lock<mutex> lock(mMutex);
    FlatDatabase& d = flat(this);
    float loopScore = 0, relocScore = 0;
    map<KeyFrame*, int>::const_iterator f = d.where.find(pKF);
    if (f != d.where.end()) {   // added again: the earlier position goes
        loopScore = d.loopScore[f->second];
        relocScore = d.relocScore[f->second];
        if (d.active[f->second]) d.erased++;
        d.active[f->second] = 0;
    } else {
        map<KeyFrame*, pair<float, float> >::iterator r = d.retired.find(pKF);
        if (r != d.retired.end()) {
            loopScore = r->second.first;
            relocScore = r->second.second;
            d.retired.erase(r);
        }
    }
    d.where[pKF] = (int)d.kf.size();
    d.kf.push_back(pKF);
    bow_arrays(pKF->mBowVec, d.word, d.value);
    d.offsets.push_back((int32_t)d.word.size());
    d.active.push_back(1);
    d.loopScore.push_back(loopScore);
    d.relocScore.push_back(relocScore);
}

void KeyFrameDatabase::erase(KeyFrame* pKF)
{
    unique_lock<mutex> lock(mMutex);
    FlatDatabase& d = flat(this);
    map<KeyFrame*, int>::const_iterator f = d.where.find(pKF);
    if (f != d.where.end() && d.active[f->second]) {
        d.active[f->second] = 0;
        d.erased++;
    }
}

void KeyFrameDatabase::clear()
{
    unique_lock<mutex> lock(gTableMutex);
    gTable.erase(this);
}

vector<KeyFrame*> KeyFrameDatabase::DetectLoopCandidates(KeyFrame* pKF, float minScore)
{
    const set<KeyFrame*> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
    unique_lock<mutex> lock(mMutex);
    return query(flat(this), ORBFE_KFDB_LOOP, pKF->mBowVec, &spConnectedKeyFrames, minScore);
}

vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame* F)
{
    unique_lock<mutex> lock(mMutex);
    return query(flat(this), ORBFE_KFDB_RELOC, F->mBowVec, NULL, 0.f);
}

} // namespace ORB_SLAM2
