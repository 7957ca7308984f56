/*
 * mcs_essgraph.h -- cOptimizer::OptimizeEssentialGraph on the device: the Sim3 pose graph that
 * applies a loop correction to the map (reference src/cOptimizerLoopStuff.cpp:273-519, called at
 * src/cLoopClosing.cpp:648).  FP64, deterministic (no floating-point atomics), stream-ordered.
 *
 * Keyframes are given in ascending id order (the text's std::map / std::set iterate in pointer
 * order; the order changes the summation order only) and no keyframe is bad (the text gives a bad
 * keyframe no vertex and dereferences it afterwards).  A Sim3 travels as 8 doubles:
 * s, qw qx qy qz, tx ty tz.
 */
#ifndef MCS_ESSGRAPH_H
#define MCS_ESSGRAPH_H

#include "mcs_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCS_ESSGRAPH_MAX_ITERATIONS 64
#define MCS_ESSGRAPH_MAX_TRIALS 64

/* The flat covisibility / spanning-tree / loop description the edge list is built from
 * (replaces the four loops of :355-382 and :385-470).  Neighbours are keyframe indices. */
typedef struct mcs_essgraph_map {
  int32_t n_kf;
  const int64_t* kf_id;          /* [n_kf] ascending */
  const int32_t* parent;         /* [n_kf] GetParent() as an index, -1 = none (:397) */
  const uint8_t* has_corrected;  /* [n_kf] the keyframe is a key of NonCorrectedSim3 / CorrectedSim3 */
  const int32_t* loop_ptr;       /* [n_kf + 1] GetLoopEdges() (:421) */
  const int32_t* loop_idx;
  const int32_t* cov_ptr;        /* [n_kf + 1] covisible neighbours with their weights, in the order */
  const int32_t* cov_idx;        /*            GetCovisiblesByWeight would list them (:447) */
  const int32_t* cov_weight;
  const int32_t* lc_ptr;         /* [n_kf + 1] LoopConnections (:355): an empty row = not a key */
  const int32_t* lc_idx;
  const int32_t* lc_weight;      /* MKF->GetWeight(connection) (:370) */
  int32_t current_index, loop_index;
  int32_t min_weight;            /* minNumFeat = 100 (:309) */
} mcs_essgraph_map;

/* Edge list of :355-470 in the order of the text: loop connections, then per keyframe its parent,
 * its earlier loop edges, its covisibility edges.  edges [cap][3] = v0, v1, kind; kind 0 = the
 * measurement comes from vScw, 1 = from the non-corrected table.  insertedEdges is never consulted
 * in the text, so a pair can carry several edges.  n_edges is the full count also when it exceeds
 * cap (MCS_ERR_CAPACITY).  counts [4]: edges per source. */
int mcs_essgraph_select_edges(const mcs_essgraph_map* m, int32_t* edges, int32_t cap, int32_t* n_edges,
                              int32_t* counts);

/* Solver setup of :283-295 and :474. */
typedef struct mcs_essgraph_options {
  int32_t iterations;           /* optimize(20) */
  int32_t terminate_max_iter;   /* terminateAction->setMaxIterations(15) */
  double gain_threshold;        /* setGainThreshold(1e-6) */
  double lambda0;               /* setUserLambdaInit(1e-6) */
  int32_t max_trials;           /* g2o's maxTrialsAfterFailure, 10 */
  /* Tile band of the system: the largest |tile(7 u0) - tile(7 u1 + 6)| + 1 over the edges, with u
   * the index among the free keyframes and 64-wide tiles; 0 = dense.  The edge list lives on the
   * device, so the caller states it (mcs_essgraph_tile_band); an edge outside it is MCS_ERR_ARG. */
  int32_t tile_band;
} mcs_essgraph_options;
void mcs_essgraph_default_options(mcs_essgraph_options* o);
/* The band of a host edge list [E][3] for n_kf keyframes with the fixed one at loop_index. */
int32_t mcs_essgraph_tile_band(int32_t n_kf, int32_t loop_index, const int32_t* edges, int32_t n_edges);
/* MCS_OK when the solver takes n_kf keyframes at this band, else MCS_ERR_UNSUPPORTED (pure size
 * arithmetic, no device use). */
int mcs_essgraph_supported(int32_t n_kf, int32_t tile_band);

typedef struct mcs_essgraph_workspace mcs_essgraph_workspace;
int mcs_essgraph_workspace_create(int32_t device, int32_t max_kf, int32_t max_edges, int32_t max_points,
                                  mcs_essgraph_workspace** out);
void mcs_essgraph_workspace_destroy(mcs_essgraph_workspace* ws);

/* Device outputs; every pointer but status may be null. */
typedef struct mcs_essgraph_out {
  double* sim3;        /* [N][8] optimised Siw (vertex estimates after :474) */
  double* rot;         /* [N][9] its rotation matrix */
  double* pose;        /* [N][16] invMat(toCvSE3(R, t / s)), the SetPose argument (:490) */
  int32_t* iterations; /* [1] */
  int32_t* trials;     /* [MCS_ESSGRAPH_MAX_ITERATIONS] LM trials of every iteration */
  double* chi2;        /* [MCS_ESSGRAPH_MAX_ITERATIONS] chi2 after every iteration */
  double* lambda;      /* [1] final lambda */
  double* edge_chi2;   /* [E] at the final estimate */
  int32_t* status;     /* [1] required: 0, MCS_ERR_ARG (an index of the device data out of range or
                          outside tile_band: nothing else was written) or MCS_ERR_HIP (the solver's
                          hand-off wait gave up) */
} mcs_essgraph_out;

/* :501-507 on the device: point_ref[j] = index of the keyframe whose id is corrected_ref[j] when
 * corrected_by[j] == current_id, else of ref_kf[j]; -1 when no keyframe has that id.  kf_id [N]
 * ascending. */
int mcs_essgraph_resolve_point_refs_device(int32_t N, const int64_t* d_kf_id, int32_t P, const int64_t* d_corrected_by,
                                           const int64_t* d_corrected_ref, const int64_t* d_ref_kf, int64_t current_id,
                                           int32_t* d_point_ref, void* stream);

/* :281-518 after the edge list.  d_Scw [N][8]: CorrectedSim3 where present, else Sim3(R, t, 1) of
 * GetPoseInverse() (:311-348); d_Snc [N][8]: NonCorrectedSim3 where present, else d_Scw.
 * d_edges [E][3] in the order of mcs_essgraph_select_edges.  d_point_pos [P][3] is corrected in
 * place (:496-518) for the points with d_point_bad == 0; d_point_ref [P] keyframe indices.
 * Stream-ordered: no host synchronisation, no allocation.  Argument errors that the host can see
 * return before any device use; those of the device data arrive in out->status and leave poses and
 * points untouched. */
int mcs_optimize_essential_graph_device(mcs_essgraph_workspace* ws, int32_t N, const double* d_Scw,
                                        const double* d_Snc, int32_t loop_index, int32_t E, const int32_t* d_edges,
                                        int32_t P, double* d_point_pos, const int32_t* d_point_ref,
                                        const uint8_t* d_point_bad, const mcs_essgraph_options* opts,
                                        const mcs_essgraph_out* out, void* stream);

/* The same on host buffers (out holds host pointers): creates a workspace, copies, runs, waits. */
int mcs_optimize_essential_graph(int32_t device, int32_t N, const double* Scw, const double* Snc, int32_t loop_index,
                                 int32_t E, const int32_t* edges, int32_t P, double* point_pos,
                                 const int32_t* point_ref, const uint8_t* point_bad,
                                 const mcs_essgraph_options* opts, const mcs_essgraph_out* out);

/* ---- The block-sparse path: maps beyond the 878 keyframes of the entries above ----------------
 *
 * A plan is made on the host from the edge list, once per loop closure (the one host-synchronous
 * step, beside mcs_essgraph_select_edges): the graph of the free keyframes (the fixed loop
 * keyframe left out, a pair that carries several edges counted once), a nested-dissection ordering
 * by breadth-first level sets, the pattern of L in 7 x 7 blocks, its supernodes (the separators
 * and leaves) and their levels.  The plan is canonical: a permuted edge list gives the same plan
 * (equal digest).  It owns its device copies and all numeric storage (the assembled system and L
 * in the pattern of L, the right-hand sides, and the per-call buffers sized by max_edges and
 * max_points): a call on a plan allocates nothing.
 *
 * Limits, from arithmetic on counts and not from 878: every index is an int32; max_edges < 2^31 /
 * 112; one copy of the pattern of L (the supernodes' dense panels, 392 bytes per block) holds at
 * most 1 GiB, and the plan keeps three.  Above that plan_create returns MCS_ERR_UNSUPPORTED.
 * device < 0 makes a host-only plan: info and arrays, no device storage, not accepted by
 * mcs_optimize_essential_graph_planned_device. */
typedef struct mcs_essgraph_plan_options {
  int32_t leaf_size;   /* the dissection stops at this many keyframes; 0 = the default, 4 */
} mcs_essgraph_plan_options;
void mcs_essgraph_plan_default_options(mcs_essgraph_plan_options* o);

typedef struct mcs_essgraph_plan mcs_essgraph_plan;
/* edges [n_edges][3] on the host, as mcs_essgraph_select_edges leaves them.  max_edges (raised to
 * n_edges) and max_points size the per-call buffers; options may be null. */
int mcs_essgraph_plan_create(int32_t device, int32_t n_kf, int32_t loop_index, const int32_t* edges, int32_t n_edges,
                             int32_t max_edges, int32_t max_points, const mcs_essgraph_plan_options* options,
                             mcs_essgraph_plan** out);
void mcs_essgraph_plan_destroy(mcs_essgraph_plan* plan);

typedef struct mcs_essgraph_plan_info {
  int32_t n_kf, loop_index;
  int32_t free_blocks;                /* n_kf - 1 block rows */
  int32_t leaf_size, supernodes, levels;
  int32_t max_supernode_columns;      /* block columns of the widest supernode */
  int32_t solver_launches_per_trial;  /* factor (with the forward solve) + backward solve */
  int32_t launches_per_trial;         /* all launches of one LM trial */
  int64_t a_blocks;                   /* lower blocks of A: the diagonals and the planned pairs */
  int64_t l_blocks;                   /* lower blocks of L; l_blocks / a_blocks is the fill ratio */
  int64_t panel_blocks;               /* blocks stored (the panels' upper triangles included) */
  int64_t flops_per_factor;
  int64_t device_bytes;               /* 0 for a host-only plan */
  uint64_t digest;                    /* FNV-1a over every array of the plan */
} mcs_essgraph_plan_info;
int mcs_essgraph_plan_get_info(const mcs_essgraph_plan* plan, mcs_essgraph_plan_info* info);

/* The plan's host arrays, valid until the plan is destroyed.  S = supernodes.  Supernode s owns
 * the columns col0[s] .. col0[s + 1] - 1 of the permuted matrix; rows[row_ptr[s] .. row_ptr[s + 1])
 * are its block rows (its own columns, then the rows below, ascending): the pattern of L. */
typedef struct mcs_essgraph_plan_arrays {
  const int32_t* perm;      /* [free_blocks] free keyframe -> column of the permuted matrix */
  const int32_t* col0;      /* [S + 1] */
  const int32_t* row_ptr;   /* [S + 1] */
  const int32_t* rows;      /* [n_rows] */
  int32_t n_rows;
  const int32_t* parent;    /* [S] supernodal tree, -1 = a root */
  const int32_t* level;     /* [S] height in the tree = the launch it runs in */
  const int32_t* block_off; /* [S + 1] first stored block of a supernode: row position p, own column c
                               is block block_off[s] + p * columns(s) + c */
  const uint8_t* a_block;   /* [panel_blocks] 1 = a block of A */
} mcs_essgraph_plan_arrays;
int mcs_essgraph_plan_get_arrays(const mcs_essgraph_plan* plan, mcs_essgraph_plan_arrays* arrays);

/* mcs_optimize_essential_graph_device with the plan's solver.  opts->tile_band is ignored.
 * Stream-ordered, no host synchronisation, no allocation.  out->status: MCS_ERR_ARG also when N
 * or loop_index are not the plan's or an edge joins two free keyframes whose pair the plan does
 * not hold (nothing else is written); never MCS_ERR_HIP, the path has no hand-off wait.  E above
 * max_edges or P above max_points return MCS_ERR_ARG before any device use. */
int mcs_optimize_essential_graph_planned_device(mcs_essgraph_plan* plan, int32_t N, const double* d_Scw,
                                                const double* d_Snc, int32_t loop_index, int32_t E,
                                                const int32_t* d_edges, int32_t P, double* d_point_pos,
                                                const int32_t* d_point_ref, const uint8_t* d_point_bad,
                                                const mcs_essgraph_options* opts, const mcs_essgraph_out* out,
                                                void* stream);

/* The same on host buffers (out holds host pointers): plans, copies, runs, waits. */
int mcs_optimize_essential_graph_sparse(int32_t device, int32_t N, const double* Scw, const double* Snc,
                                        int32_t loop_index, int32_t E, const int32_t* edges, int32_t P,
                                        double* point_pos, const int32_t* point_ref, const uint8_t* point_bad,
                                        const mcs_essgraph_options* opts, const mcs_essgraph_out* out);

#ifdef __cplusplus
}
#endif
#endif /* MCS_ESSGRAPH_H */
