// The state-dependent tail of cORBmatcher::Fuse for one target keyframe, on the host, over a flat
// stand-in of the map (C-ABI of include/mcs_matcher.h, mcs_fuse_select).  Plain C++: no device.
//
// Reference: the query loop heads and tails of the three overloads, src/cORBmatcher.cpp
// :1279-1287 + :1379-1415 (rule 0), :1433-1440 + :1536-1563 (rule 1), :1596-1602 + :1692-1715
// (rule 2); cMapPoint::Replace src/cMapPoint.cpp:208-250, AddObservation :90-96, IsInKeyFrame
// :447-451; cMultiKeyFrame::AddMapPoint / EraseMapPointMatch / ReplaceMapPointMatch / GetMapPoint
// / GetMapPoints src/cMultiKeyFrame.cpp:273-304, :328-332.
#include "../../include/mcs_matcher.h"
#include <algorithm>
#include <vector>

namespace mcs {
void set_error(const char* msg);
}

extern "C" int mcs_fuse_select(int32_t rule, int32_t nq, int32_t n_cams, const int32_t* q_mp,
                               const int32_t* best_kp, const uint8_t* epi_ok, int32_t n_mp,
                               uint8_t* mp_bad, uint8_t* mp_in_kf, int32_t n_kp, int32_t* kp_mp,
                               int32_t* actions, int32_t action_cap, int32_t* n_actions,
                               int32_t* n_fused, int32_t* requery_ids, int32_t* n_requery) {
  if (rule < 0 || rule > 2 || nq < 0 || n_cams < 1 || n_mp < 0 || n_kp < 0 || action_cap < 0 ||
      !n_actions || !n_fused || (nq > 0 && (!q_mp || !best_kp || (rule == 0 && !epi_ok))) ||
      (n_mp > 0 && (!mp_bad || !mp_in_kf)) || (n_kp > 0 && !kp_mp) || (action_cap > 0 && !actions)) {
    mcs::set_error("fuse select: bad argument");
    return MCS_ERR_ARG;
  }
  for (int i = 0; i < nq; i++) {
    if (q_mp[i] < -1 || q_mp[i] >= n_mp) { mcs::set_error("fuse select: map-point id out of range"); return MCS_ERR_ARG; }
    for (int c = 0; c < n_cams; c++)
      if (best_kp[(size_t)i * n_cams + c] < -1 || best_kp[(size_t)i * n_cams + c] >= n_kp) {
        mcs::set_error("fuse select: keypoint index out of range");
        return MCS_ERR_ARG;
      }
  }
  for (int k = 0; k < n_kp; k++)
    if (kp_mp[k] < -1 || kp_mp[k] >= n_mp) { mcs::set_error("fuse select: slot holds an id out of range"); return MCS_ERR_ARG; }

  // mObservations[target] of every map point: the slots that hold it, when it is in the keyframe
  std::vector<std::vector<int32_t>> obs(n_mp);
  for (int k = 0; k < n_kp; k++)
    if (kp_mp[k] >= 0 && mp_in_kf[kp_mp[k]]) obs[kp_mp[k]].push_back(k);
  std::vector<uint8_t> found, is_query(n_mp, 0), listed(n_mp, 0);
  if (rule == 2) {   // spAlreadyFound = pKF->GetMapPoints(): the non-bad points in slots (:1588)
    found.assign(n_mp, 0);
    for (int k = 0; k < n_kp; k++)
      if (kp_mp[k] >= 0 && !mp_bad[kp_mp[k]]) found[kp_mp[k]] = 1;
  }
  for (int i = 0; i < nq; i++)
    if (q_mp[i] >= 0) is_query[q_mp[i]] = 1;

  int na = 0, nf = 0, nr = 0;
  bool overflow = false;
  auto emit = [&](int kind, int q, int k, int other) {
    if (na < action_cap) {
      int32_t* a = actions + 4 * (size_t)na;
      a[0] = kind; a[1] = q; a[2] = k; a[3] = other;
    } else {
      overflow = true;
    }
    na++;
  };
  for (int i = 0; i < nq; i++) {
    const int mp = q_mp[i];
    if (mp < 0) continue;                                    // if (!pMP) continue;
    if (mp_bad[mp] || (rule == 2 ? found[mp] : mp_in_kf[mp])) continue;
    for (int c = 0; c < n_cams; c++) {                       // bestIdxs in camera order
      const int k = best_kp[(size_t)i * n_cams + c];
      if (k < 0) continue;
      const int in_kf = kp_mp[k];                            // pMPinKF = pKF->GetMapPoint(bestIdx)
      if (in_kf >= 0) {
        if (mp_bad[in_kf] || (rule == 0 && !epi_ok[(size_t)i * n_cams + c])) continue;
        emit(MCS_FUSE_REPLACE, i, k, in_kf);
        nf++;                                                // ++nFused, also after the early return
        if (in_kf == mp) continue;                           // Replace: same mnId -> return
        std::vector<int32_t> mine;
        mine.swap(obs[mp]);                                  // obs = mObservations; clear; mbBad
        mp_bad[mp] = 1;
        mp_in_kf[mp] = 0;
        for (int32_t s : mine) {
          if (!mp_in_kf[in_kf]) {                            // ReplaceMapPointMatch + AddObservation
            kp_mp[s] = in_kf;
            obs[in_kf].push_back(s);
            mp_in_kf[in_kf] = 1;
          } else {
            kp_mp[s] = -1;                                   // EraseMapPointMatch
          }
        }
        if (is_query[in_kf] && !listed[in_kf]) {             // its descriptor is recomputed (:244)
          listed[in_kf] = 1;
          if (requery_ids) requery_ids[nr] = in_kf;
          nr++;
        }
      } else {
        emit(MCS_FUSE_ADD, i, k, mp);
        obs[mp].push_back(k);                                // pMP->AddObservation(pKF, bestIdx)
        mp_in_kf[mp] = 1;
        kp_mp[k] = mp;                                       // pKF->AddMapPoint(pMP, bestIdx)
      }
    }
  }
  *n_actions = na;
  *n_fused = nf;
  if (n_requery) *n_requery = nr;
  if (overflow) {
    mcs::set_error("fuse select: action list too small (required size in *n_actions)");
    return MCS_ERR_CAPACITY;
  }
  return MCS_OK;
}
