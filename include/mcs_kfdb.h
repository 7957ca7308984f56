/*
 * mcs_kfdb.h -- C-ABI drop-in boundary for the keyframe database (place recognition queries).
 *
 * Replaces (billamiable/MultiCol-SLAM-Annotation):
 *   cMultiKeyFrameDatabase::add / erase / clear            src/cMultiKeyFrameDatabase.cpp:43-79
 *   cMultiKeyFrameDatabase::DetectLoopCandidates           :82-221
 *   cMultiKeyFrameDatabase::DetectRelocalisationCandidates :223-340
 *   L1Scoring::score                       ThirdParty/DBoW2/DBoW2/ScoringObject.cpp:23-68
 *   the minScore loop of cLoopClosing::DetectLoop          src/cLoopClosing.cpp:141-157
 * Callers: cTracking::Relocalisation (src/cTracking.cpp:1148) and cLoopClosing::DetectLoop
 * (src/cLoopClosing.cpp:164).  The candidates feed mcs_search_by_bow[_kf]_device.
 *
 * The reference keeps an inverted file (word -> list of keyframes) and six members per keyframe
 * (include/cMultiKeyFrame.h:201-206).  Here the database holds the BowVectors of the added
 * keyframes packed in add order and the six members per slot, all on the device; one query is one
 * streaming pass over the packed vectors.  A keyframe is named by its slot: the add sequence
 * number, handed out by the host and never reused (mcs_kfdb_clear starts again at 0).
 *
 * Only L1 scoring (scoring type 0, what the Lafida vocabulary uses) is built; a vocabulary with
 * another scoring gets MCS_ERR_UNSUPPORTED from create.
 *
 * Device entries are stream-ordered, allocate nothing and never synchronise with the host.  Every
 * slot, count and neighbour id that is device data is clamped in the kernels.  One database serves
 * one stream at a time: the word table and the scratch are shared between calls.
 */
#ifndef MCS_KFDB_H
#define MCS_KFDB_H

#include <stdint.h>
#include "mcs_common.h"
#include "mcs_vocab.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcs_kfdb mcs_kfdb;

/* neighbours per keyframe: GetBestCovisibilityKeyFrames(10) (:173, :294) */
#define MCS_KFDB_NEIGH 10

/* A BowVector on the device: n = *d_n entries (clamped to [0, cap]), word ascending and unique. */
typedef struct mcs_kfdb_query {
  const uint32_t* d_word;
  const double* d_value;
  const int32_t* d_n;
  int32_t cap;
} mcs_kfdb_query;

/* Outputs of one detect call.  d_candidates [cap] slots in the reference's output order,
 * d_n_candidates the number found (may exceed cap; the first cap are written).  Nullable
 * diagnostics per slot [n_slots]: d_common = words shared with the query in this call (0 for an
 * erased keyframe), d_score = L1 score of the query against the slot (-0.0 when nothing is shared). */
typedef struct mcs_kfdb_result {
  int32_t* d_candidates;
  int32_t cap;
  int32_t* d_n_candidates;
  int32_t* d_common;
  double* d_score;
} mcs_kfdb_result;

/* A database for a vocabulary of n_words words on `device`: at most max_keyframes adds and
 * max_entries BowVector entries in total.  mcs_kfdb_create reads n_words and the scoring from the
 * vocabulary.  Argument errors and MCS_ERR_UNSUPPORTED (scoring != L1) come before any device use. */
int mcs_kfdb_create_n(int32_t device, int32_t n_words, int32_t scoring, int32_t max_keyframes,
                      int32_t max_entries, mcs_kfdb** out);
int mcs_kfdb_create(int32_t device, const mcs_vocab* voc, int32_t max_keyframes, int32_t max_entries,
                    mcs_kfdb** out);
void mcs_kfdb_destroy(mcs_kfdb* db);
/* number of slots handed out so far (host value) */
int32_t mcs_kfdb_size(const mcs_kfdb* db);

/* add(pKF): append a keyframe's BowVector (device data of *d_bow_n <= n_upper entries; n_upper is
 * the caller's bound, e.g. the descriptor count).  *slot = its sequence number.  The host accounts
 * capacity with n_upper: MCS_ERR_CAPACITY, with nothing written, when max_keyframes or max_entries
 * would be passed.  loop_query and reloc_query start at 0 (src/cMultiKeyFrame.cpp:44-45).  The
 * reference never initialises mRelocScore yet DetectRelocalisationCandidates can read it before
 * writing it (:306), so its first value is the caller's choice: reloc_score_init (loop_score
 * starts at the same value; it is never read before it is written). */
int mcs_kfdb_add_device(mcs_kfdb* db, const uint32_t* d_bow_word, const double* d_bow_value,
                        const int32_t* d_bow_n, int32_t n_upper, double reloc_score_init,
                        int32_t* slot, void* stream);
/* erase(pKF): the keyframe leaves every query; the order of the others is kept.  Its members stay
 * readable as a neighbour's, as the reference's object stays alive. */
int mcs_kfdb_erase(mcs_kfdb* db, int32_t slot, void* stream);
/* clear(): empty database, slots start again at 0 */
int mcs_kfdb_clear(mcs_kfdb* db, void* stream);

/* The minScore loop of DetectLoop: *d_min_score = min(1.0, score(query, slot) for the n listed
 * slots), strict '<' from 1.0.  Slots outside [0, size) are skipped. */
int mcs_kfdb_min_score_device(mcs_kfdb* db, const mcs_kfdb_query* query, const int32_t* d_slots,
                              int32_t n, double* d_min_score, void* stream);

/* DetectLoopCandidates(pKF, minScore).  query_id = pKF->mnId; d_connected [size] uint8 flags of
 * GetConnectedKeyFrames; d_min_score a device double; d_neigh [size][MCS_KFDB_NEIGH] int32 slots of
 * GetBestCovisibilityKeyFrames(10) per keyframe in the reference's order, -1 = padding or a
 * keyframe that is not in the database. */
int mcs_kfdb_detect_loop_device(mcs_kfdb* db, const mcs_kfdb_query* query, int64_t query_id,
                                const uint8_t* d_connected, const double* d_min_score,
                                const int32_t* d_neigh, const mcs_kfdb_result* out, void* stream);
/* DetectRelocalisationCandidates(F).  query_id = F->mnId. */
int mcs_kfdb_detect_reloc_device(mcs_kfdb* db, const mcs_kfdb_query* query, int64_t query_id,
                                 const int32_t* d_neigh, const mcs_kfdb_result* out, void* stream);

/* The six members per slot (include/cMultiKeyFrame.h:201-206), copied out on `stream` into device
 * buffers of size entries each; any pointer may be null. */
int mcs_kfdb_members_device(const mcs_kfdb* db, int64_t* d_loop_query, int32_t* d_loop_words,
                            double* d_loop_score, int64_t* d_reloc_query, int32_t* d_reloc_words,
                            double* d_reloc_score, void* stream);

/* Host-buffer forms (synchronous, default stream): the query is q_word / q_value [q_n]; connected
 * [size], neigh [size][MCS_KFDB_NEIGH], candidates [cap], common / score [size] nullable.
 * MCS_ERR_ARG before any device use, MCS_ERR_NO_DEVICE without a GPU; the detect forms return
 * MCS_ERR_CAPACITY (with the first cap candidates) when *n_candidates > cap. */
int mcs_kfdb_add(mcs_kfdb* db, const uint32_t* bow_word, const double* bow_value, int32_t n,
                 double reloc_score_init, int32_t* slot);
int mcs_kfdb_min_score(mcs_kfdb* db, const uint32_t* q_word, const double* q_value, int32_t q_n,
                       const int32_t* slots, int32_t n, double* min_score);
int mcs_kfdb_detect_loop(mcs_kfdb* db, const uint32_t* q_word, const double* q_value, int32_t q_n,
                         int64_t query_id, const uint8_t* connected, double min_score,
                         const int32_t* neigh, int32_t* candidates, int32_t cap,
                         int32_t* n_candidates, int32_t* common, double* score);
int mcs_kfdb_detect_reloc(mcs_kfdb* db, const uint32_t* q_word, const double* q_value, int32_t q_n,
                          int64_t query_id, const int32_t* neigh, int32_t* candidates, int32_t cap,
                          int32_t* n_candidates, int32_t* common, double* score);

#ifdef __cplusplus
}
#endif
#endif /* MCS_KFDB_H */
