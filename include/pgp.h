/* include/pgp.h -- C ABI of the MI355X-native pose-hypothesis scoring path (libpgp.so).
 *
 * This is the drop-in boundary for the hot path of cmitash/PhysimGlobalPose: everything the
 * reference computes between "a list of candidate transforms exists" and "every candidate has an
 * LCP score and the best one is known" (S4/algorithms/match4pcsBase.cc:1885-1901, with
 * S4 = src/3rdparty/super4pcs/src/super4pcs), plus the steps either side of it as they are
 * added (rigid fit from congruent pairs, ICP refinement).  Plain pointers and sizes only.
 *
 * Frames and layouts are the reference's own, so its containers can be passed without copies:
 *   - a cloud is n x 3 row-major float (pos() of each Point3D, S4/shared4pcs.h:61-111);
 *   - a transform is the memory image of Eigen::Matrix<float,4,4>: 16 floats, COLUMN-major
 *     (element (r,c) at [4*c + r]); `allTransforms.data()` (base.cc:1468) is such an array;
 *   - scoring happens in the CENTRED frames of Match4PCSBase::init (base.cc:242-268): the scene
 *     cloud minus centroid_P, the validation model minus centroid_Q.  pgp_center() does that.
 *
 * Every function returns 0 on success or a negative PGP_E* code; pgp_last_error() then holds a
 * message for the calling thread.  A context is bound to one HIP device; calls on one context
 * must not overlap (the reference is single-threaded: main.cpp:212), distinct contexts are
 * independent.  The *_device entry points queue their kernels on the caller's stream and return; a
 * context serves ONE such stream at a time (its workspaces are shared), and any later call on the
 * host-pointer call on the context -- pgp_set_model, pgp_set_scene, pgp_score_lcp ... -- first waits for
 * the queued work (a device synchronisation), so the arrays a queued kernel reads are never rewritten under it.
 * There is NO CPU fallback: without a usable HIP device pgp_create() fails.
 */
#ifndef PGP_H
#define PGP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgp_ctx pgp_ctx;

enum {
  PGP_OK = 0,
  PGP_EINVAL = -1,   /* bad argument (null pointer, negative size, NaN delta ...) */
  PGP_ENODEV = -2,   /* no usable HIP device / runtime error at create */
  PGP_EHIP = -3,     /* a HIP call failed */
  PGP_ESTATE = -4,   /* scene / model / index not set for this call */
  PGP_ENOMEM = -5
};

/* Scoring mode: which reference verifier is reproduced. */
enum {
  PGP_MODE_PLAIN = 0,    /* Match4PCSBase::Verify, base.cc:1699-1731, WITHOUT the early-out
                            (every hypothesis gets its true inlier count) */
  PGP_MODE_WEIGHTED = 1  /* Match4PCSBase::WeightedVerify, base.cc:1733-1766 (live operMode=1) */
};

int pgp_version(void);
const char* pgp_last_error(void);

/* Replaces the construction of the per-call MatchSuper4PCS object (S4/super4pcs_test.cc:102).
 * device_id < 0 selects the current HIP device. */
int pgp_create(pgp_ctx** out, int device_id);
int pgp_destroy(pgp_ctx* ctx);

/* Replaces Match4PCSBase::init's centring loop (base.cc:242-268): in place, float arithmetic in
 * the reference's order.  P is centred on centroid(P); Qs (search model) and Qv (validation
 * model) on centroid(Qs).  Pure host helper (O(n)); any of the clouds may be empty. */
int pgp_center(float* P_xyz, int nP, float* Qs_xyz, int nQs, float* Qv_xyz, int nQv,
               float centroid_P[3], float centroid_Q[3]);

/* Replaces the "priority based sampling" loop of Match4PCSBase::init (base.cc:317-340): the
 * per-scene-point weight orig_probabilities_[i] = probImg(row, col) with probImg = u16 / 10000
 * and (col,row) = int(K * (p_i + centroid_P)) / z, float arithmetic in the reference's order.
 * P_xyz is the CENTRED cloud; K is the 3x3 intrinsic matrix, row-major; img is the decoded
 * 16-bit probability image (rows x cols, row-major).  Pixels outside the image give weight 0
 * (the reference reads out of bounds there).  Pure host helper. */
int pgp_weights_from_image(const float* P_xyz, int n, const float centroid_P[3], const float K[9],
                           const unsigned short* img, int rows, int cols, float* weights);

/* The image rows pgp_weights_from_image reads for these points (the same arithmetic, so the answer is exact):
 * *row_min / *row_max over the points that fall inside a rows x cols image, -1 / -1 when none does.  A caller
 * that decodes the probability image while the clouds are being set up (the drop-in's file hand-off, base.cc:317)
 * can stop decoding after row_max.  Pure host helper. */
int pgp_image_rows_needed(const float* P_xyz, int n, const float centroid_P[3], const float K[9], int rows,
                          int cols, int* row_min, int* row_max);

/* Replaces `sampled_P_3D_ = P` + initKdTree() + orig_probabilities_ (base.cc:235,270,1046-1056,
 * 327-340): uploads the (centred) scene cloud and builds the device spatial index for inlier
 * radius `delta` (options_.delta, S4/super4pcs_test.cc:20).  nrm and weight may be NULL
 * (weights default to 1; PGP_MODE_WEIGHTED then needs normals and fails without them).
 * The index is a uniform grid of cell 0.85 delta with dilated candidate lists; its block table is a dense array
 * for scenes within 1024 cells per axis and 2^26 cells, a hashed table of the occupied blocks beyond (up to
 * 16 384 cells per axis at that cell size; pgp_index_info.sparse says which).  Answers are identical.
 * Host pointers, synchronous. */
int pgp_set_scene(pgp_ctx* ctx, const float* xyz, const float* nrm, const float* weight, int n,
                  float delta);

/* Replaces the weights of the resident scene (n must be the scene's point count) without touching
 * its points or index: the per-point probabilities come from an image (base.cc:317-340) that a caller
 * can still be decoding while pgp_set_scene builds the index from the coordinates.  Host pointer,
 * synchronous.  pgp_multi_set_scene_weights: the same on every device of a group. */
int pgp_set_scene_weights(pgp_ctx* ctx, const float* weight, int n);

/* Replaces `validation_Q_3D = Q_validation` (base.cc:237).  Host pointers, synchronous. */
int pgp_set_model(pgp_ctx* ctx, const float* xyz, const float* nrm, int n);

/* Replaces the verification loop of Perform_N_steps (base.cc:1885-1901) for n_h transforms.
 *   scores[n_h]     : lcp per hypothesis (inliers / nQ, or weighted sum / nQ), as allPose[i].second
 *   counts[n_h]     : (nullable) integer inlier count per hypothesis (for weighted mode: the
 *                     number of registered points)
 *   best_index      : (nullable) what best_lcp_index ends as: the lowest index attaining the
 *                     maximum score if that maximum is > 0, else -1 (base.cc:1891,309)
 *   best_score      : (nullable) best_LCP_
 * gate_deg is the normal-agreement gate of base.cc:1758 (30 in the reference; ignored in plain
 * mode).  Host pointers, synchronous. */
int pgp_score_lcp(pgp_ctx* ctx, const float* T, int n_h, int mode, float gate_deg,
                  float* scores, int* counts, int* best_index, float* best_score);

/* Same computation with DEVICE pointers, enqueued on `stream` (a hipStream_t; NULL = default
 * stream) and not synchronised: for callers that keep the hypothesis batch resident (bench.py,
 * multi-GPU sharding).  d_best (nullable) receives 2 ints: {best_index, float bits of best
 * score}.  No allocation happens inside when n_h <= the capacity reserved by
 * pgp_reserve(); otherwise PGP_ESTATE.
 * A context serves ONE stream at a time: its workspaces (partials, arg-max key, ticket) are
 * shared by every queued call, so the *_device calls of one context must all go to the same
 * stream (or be ordered by the caller's events); different contexts are independent.
 * pgp_set_scene / pgp_set_model / pgp_set_search_model / a growing pgp_reserve wait for
 * everything queued on the device (hipDeviceSynchronize) before they replace arrays a queued
 * launch may still be reading.
 * Weighted mode: hypotheses within 4.1 * 2^-24 * sqrt(nQ) * best_score of the maximum (ten standard
 * deviations of the reference's own summation error; 6.2e-6 at 5000 model points) are re-summed on
 * the device in the reference's order (sequential float adds in model order, base.cc:1759) and
 * their score entries overwritten with that value, so best_index is the reference's also under
 * near-ties; all other weighted scores carry the library's fixed summation tree (within 2e-6 of
 * the reference at those sizes). */
int pgp_reserve(pgp_ctx* ctx, int max_hypotheses);
int pgp_score_lcp_device(pgp_ctx* ctx, const float* d_T, int n_h, int mode, float gate_deg,
                         float* d_scores, int* d_counts, int* d_best, void* stream);

/* Arg-max over a COMPLETE score vector assembled from several partial calls (the slices of
 * several devices after the score all-reduce, or several batches of one object): publishes
 * d_best = {best_index, float bits of best score} with the rule of base.cc:1891 (lowest index of
 * the maximum, -1 when the maximum is not > 0) and, in weighted mode, the exact near-tie
 * settlement described above -- d_T must hold ALL n_h transforms and the context the clouds the
 * scores were computed on; settled entries of d_scores are overwritten with the reference-order
 * value.  Device pointers, enqueued on `stream`. */
int pgp_settle_best_device(pgp_ctx* ctx, const float* d_T, int n_h, int mode, float gate_deg,
                           float* d_scores, int* d_best, void* stream);

/* Replaces `registered_indices = temp_registered_indices` (base.cc:1897): the scene-point ids
 * matched under ONE transform, in model-point order.  ids has capacity nQ; *n receives the
 * count.  In plain mode every inlier's nearest scene point is reported. */
int pgp_registered(pgp_ctx* ctx, const float* T16, int mode, float gate_deg, int* ids, int* n);

/* Replaces Match4PCSBase::getRegisteredModel (base.cc:347-375; defined but not called by
 * ComputeTransformation): the scene ids registered by the points of ANOTHER cloud with normals
 * (sampled_Q_3D_, the search model) under one transform, with the gate on the DIRECTED normal angle
 * (acos(dot) * 180 / pi < gate_deg; the fold of WeightedVerify is commented out there, :368).
 * q_xyz / q_nrm: n x 3; ids (capacity n) in cloud order; *n_ids their number.  Host pointers. */
int pgp_registered_model(pgp_ctx* ctx, const float* T16, const float* q_xyz, const float* q_nrm, int n,
                         float gate_deg, int* ids, int* n_ids);

/* Opt-in: plain-mode scores and counts as the reference's Verify returns them, WITH its early termination
 * (base.cc:1708,1725-1727: a hypothesis that can no longer beat the running best stops, and its
 * allPose[i].second is the fraction counted so far -- an order-dependent lower bound).  Off (default):
 * every hypothesis is counted completely.  Best index and best score are the same either way.  Costs up to
 * one more pass over the batch.  Applies to pgp_score_lcp / pgp_score_lcp_device in PGP_MODE_PLAIN;
 * pgp_verify_early_out_device applies it to a complete vector assembled elsewhere (d_scores / d_counts hold
 * the TRUE values of all n_h hypotheses, e.g. after the all-reduce of a device group). */
int pgp_set_verify_early_out(pgp_ctx* ctx, int on);
int pgp_verify_early_out_device(pgp_ctx* ctx, const float* d_T, int n_h, float* d_scores, int* d_counts, void* stream);

/* Weighted mode, the running-best LIST (base.cc:1891-1908, what the drop-in returns as hypothesisSet): with
 * pgp_set_exact_records(ctx, 1) every later weighted scoring call on the context also re-scores, exactly as
 * the reference sums (sequential float adds in model order), every hypothesis whose score comes within the
 * summation tolerance of the running maximum before it -- the records and whatever could displace or tie one;
 * pgp_running_best over the returned scores is then the reference's list, entry for entry.  Costs three
 * small launches per call (~60 us at 4096 hypotheses x 5000 model points); off by default (the best pose is
 * exact either way).  Call it after pgp_set_model (it reserves a workspace of 128 rows of model size).
 * pgp_settle_records_device does the same for a score vector assembled elsewhere (the slices of several
 * devices), like pgp_settle_best_device. */
int pgp_set_exact_records(pgp_ctx* ctx, int on);

/* Exact distance ties.  KdTree::doQueryRestrictedClosestIndex accepts a candidate when `sqdist <= cl_dist`
 * (kdtree.h:424): of several scene points at exactly the same float distance from a query it returns the one its
 * descent visits last (the query's side of every split plane first, points of a leaf in the order the build left
 * them).  This library's index breaks such a tie by the lowest scene index instead -- the registered point, hence
 * the normal gate and the weight of that model point, can then differ from the reference's (about one query in
 * 10^7 with two neighbours on real clouds; every query near a DUPLICATED scene point).  With on != 0, every later
 * pgp_set_scene / pgp_set_scene_device also builds the reference's tree on the host (its own splits, partition
 * and leaf sizes, kdtree.h:522-641; ~5 ms per 50 000 points) and the scoring paths ask it whenever two different
 * candidates share the minimal distance: scores, registered points and records then follow the reference on ties
 * as well.  Default off.  Takes effect at the next scene set-up. */
int pgp_set_exact_ties(pgp_ctx* ctx, int on);
int pgp_settle_records_device(pgp_ctx* ctx, const float* d_T, int n_h, int mode, float gate_deg, float* d_scores,
                              void* stream);

/* Running-best subsequence of base.cc:1891-1908 over a score vector (host helper): writes the
 * indices i with scores[i] > max(scores[0..i-1], 0) to selected (capacity n_h). */
int pgp_running_best(const float* scores, int n_h, int* selected, int* n_selected);

/* Introspection for DESIGN.md / bench.py: sizes of the device index of the current scene. */
typedef struct {
  int n_scene, n_model;
  int grid_nx, grid_ny, grid_nz;
  float cell_size, delta;
  long long n_cells, n_candidates;      /* entries in the dilated per-cell candidate lists */
  long long n_occupied;                 /* cells with a non-empty candidate list */
  long long bytes_index;                /* query-time index: words + occupied offsets + lists */
  float build_ms;                       /* device time of the last index build */
  int sparse;                           /* 1: hashed table of the occupied 4x4x2 blocks, 0: dense block array */
  long long n_blocks;                   /* blocks in the table (sparse) or in the dense array */
} pgp_index_info;
int pgp_get_index_info(pgp_ctx* ctx, pgp_index_info* info);

/* Nearest-only candidate lists.  The scoring paths ask a cell's list for the NEAREST scene point within delta (weighted)
 * or for ANY (plain); many entries of a list can be neither for any position inside the cell, because another entry of the
 * list is closer everywhere in it.  The index therefore keeps a pruned twin of its lists for those paths (what it keeps
 * of a scene is reported by pgp_get_nn_lists_info; DESIGN.md section 5 has the measured figures); the full lists stay for
 * pgp_radius_outlier_filter, which counts every neighbour.  Scores, counts, registered points and records are the same
 * bits with either: the rule's margin covers the float rounding of the distance test (csrc/nn_prune.h).
 *   mode 0  off.
 *   mode 1  (default) behind the calls: the twin is built on a side stream when the SECOND scoring launch against a
 *           scene is issued, and later launches take it once it is complete.  No call waits for it; a scene that is
 *           scored once pays nothing.  Launches captured into a graph neither start nor take it (a graph keeps the
 *           lists it was captured with; both stay valid until the next pgp_set_scene).
 *   mode 2  with the index: built, waited for and taken before the first scoring launch of a scene (callers who
 *           know they will score many batches; tests).
 * Takes effect at once (0 returns to the full lists; 1 and 2 apply from the next scoring launch or scene set-up).  A twin
 * that the current scene already has is kept across mode changes and taken up again, never rebuilt: its buffers are written
 * once per scene, so a graph captured with them may replay at any time.  The launch that starts the pass allocates its
 * memory (once per context; a larger scene than any before grows it, which synchronises the device).
 * The environment variable PGP_NN_PRUNE=0|1|2 sets the mode a new context starts with. */
int pgp_set_nn_pruning(pgp_ctx* ctx, int mode);
enum {
  PGP_NN_LISTS_FULL = 0,     /* the scoring paths read the full lists (no twin yet, or mode 0) */
  PGP_NN_LISTS_QUEUED = 1,   /* the twin is being built; the full lists are still in use */
  PGP_NN_LISTS_ADOPTED = 2   /* the scoring paths read the twin */
};
/* state: PGP_NN_LISTS_*; entries_full / entries_kept: entries of all lists, and of the twin (0 until adopted);
 * lists_emptied: occupied cells whose twin list came out empty (0 by the rule); pass_ms: device time of the pruning
 * pass (0 until adopted).  Any pointer may be NULL.  Never waits. */
int pgp_get_nn_lists_info(pgp_ctx* ctx, int* state, long long* entries_full, long long* entries_kept, long long* lists_emptied,
                          float* pass_ms);

/* Replaces `sampled_Q_3D_ = Q` (base.cc:236): the sparse search model whose points the
 * congruent quads index.  Host pointer, synchronous. */
int pgp_set_search_model(pgp_ctx* ctx, const float* xyz, int n);

/* ---- Step 1 of Perform_N_steps: stochastic base selection (base.cc:600-792) on the device -------
 * pgp_set_ppf_map replaces the node's hand-over of the model's pair-feature table
 * (std::map<std::vector<int>, std::vector<std::pair<int,int>>> PPFMap, PPE/data_layer/Objects.cpp:31-49;
 * parameter of getProbableTransformsSuper4PCS): keys[n_keys][4] = the discretised features
 * (computePPF + approximate_bin, base.cc:582-598,150-160), counts[n_keys] (nullable) and
 * pairs[sum(counts)][2] (nullable) the pair list of every key in key order (ids into the search
 * model).  The first occurrence of a key counts, as std::map::insert.  The keys become a device
 * hash set; the ratio thresholds that stand in for atan2f are measured on the host's libm here. */
int pgp_set_ppf_map(pgp_ctx* ctx, const int* keys, const int* counts, const int* pairs, int n_keys);

/* The same table BUILT on the device from the n-point search model (xyz / nrm: n x 3, host pointers; synchronous), for
 * an object that has no PPFMap.txt yet, and installed exactly as pgp_set_ppf_map(keys, counts, pairs) installs it: the
 * hash set, the pair lists and their offsets, the model angles of pgp_set_ppf_model redone, a resident congruent batch
 * discarded.  The pair lists never visit the host; *n_keys / *n_pairs (nullable) receive the table's size.
 * The table: every ordered pair (i, j), i != j, of the model is filed under the key computePPF(i, j)
 * (base.cc:582-598: u = p_i - p_j, the distance in mm binned to 5, the angles (n_i, u), (n_j, u), (n_i, n_j) binned to
 * 10 degrees, approximate_bin base.cc:150-160), evaluated by the code that evaluates the scene's pairs, with the
 * host-measured atan2f thresholds; the normals are used as given, like pgp_set_scene's, so pgp_ppf_features of the
 * same cloud set as a scene returns the same four integers.  A pair whose feature is no key (a non-finite input) is
 * left out.  Keys come in std::map<std::vector<int>, ...> order (lexicographic), the pairs of a key in ascending
 * (i, j) -- the order a double loop over the model inserts them; the result is bitwise the same from run to run.
 * PGP_EINVAL: n outside 2 .. PGP_PPF_BUILD_MAX_POINTS, a null xyz / nrm, or a model whose finite points span more
 * than PGP_PPF_BUILD_MAX_MM millimetres (the distance field of the 64-bit sort keys).  The previous table survives
 * these; a failure later in the build (PGP_ENOMEM, PGP_EHIP) leaves the context without a table.
 * Memory: 16 n^2 bytes of sort keys (two buffers of 8 n^2; 2 x 0.5 GB at the cap) plus rocPRIM's scratch (a few MB)
 * while the call runs, all released before it returns; what stays is what pgp_set_ppf_map holds: 8 bytes per pair,
 * 4 per key of offsets and <= 48 per key of hash set. */
#define PGP_PPF_BUILD_MAX_POINTS 8192
#define PGP_PPF_BUILD_MAX_MM 10000000
int pgp_set_ppf_map_from_model(pgp_ctx* ctx, const float* xyz, const float* nrm, int n, int* n_keys, long long* n_pairs);

/* Reads the installed table back in pgp_set_ppf_map's layout (to write PPFMap.txt, or to fill the std::map of an
 * unmodified node): keys[cap_keys][4], counts[cap_keys], pairs[cap_pairs][2], each nullable.  *n_keys / *n_pairs
 * (nullable) receive the FULL counts, which may exceed the caps; the arrays are filled up to their caps.  A row whose
 * key no lookup can reach (pgp_set_ppf_map was handed a repeated or an out-of-range key) reads {-1, -1, -1, -1}.
 * PGP_ESTATE without a table, or when `pairs` is asked for and the table was set without pair lists. */
int pgp_get_ppf_map(pgp_ctx* ctx, int* keys, int* counts, int* pairs, int cap_keys, long long cap_pairs, int* n_keys,
                    long long* n_pairs);

/* Replaces n_attempts calls of Match4PCSBase::SelectQuadrilateralStoCS (base.cc:600-792; the
 * reference seeds a fresh engine per call, so attempts are independent) + TryQuadrilateral
 * (:415-464) in ONE launch, on the scene set by pgp_set_scene (positions, normals, weights =
 * orig_probabilities_) and the table set by pgp_set_ppf_map.  u[n_attempts][4]: the uniform variates
 * in [0,1) of the four std::discrete_distribution draws, taken by the CALLER from its own engine
 * (std::generate_canonical<double, 53>, what discrete_distribution::operator() consumes).
 * ids[n_attempts][4]: scene ids of the base in TryQuadrilateral's order; invariants[n_attempts][2];
 * status[n_attempts]: 1 = base found, 0 = the reference would have returned false (no candidate
 * left for the 2nd / 3rd / 4th point).  Host pointers, synchronous. */
int pgp_select_bases(pgp_ctx* ctx, const double* u, int n_attempts, int* ids, float* invariants, int* status);
/* The same, and rows[n_attempts][2]: the rows of the pair-feature table under which ExtractCongruentSet finds pairs1 and
 * pairs6 of the base -- PPFMap->find(computePPF(ids[0], ids[1])) and (ids[2], ids[3]), base.cc:1970-1981; -1: not a key --
 * computed where the base is selected, for pgp_find_congruent_batch_rows below (one launch and one round trip less per
 * object than asking for them again). */
int pgp_select_bases_rows(pgp_ctx* ctx, const double* u, int n_attempts, int* ids, float* invariants, int* status, int* rows);
/* pgp_select_bases_rows in two halves, for a caller with host work of its own to do meanwhile (the drop-in hashes the
 * validation model while the selection's ~0.1 ms kernel runs): _begin copies the variates, queues the launch and returns;
 * _end waits and returns what pgp_select_bases_rows returns (rows nullable).  Between the two, only calls that leave the
 * scene, its weights and the pair-feature table alone (pgp_set_model); any other selection call drops the begun one. */
int pgp_select_bases_rows_begin(pgp_ctx* ctx, const double* u, int n_attempts);
int pgp_select_bases_rows_end(pgp_ctx* ctx, int* ids, float* invariants, int* status, int* rows);

/* The pieces of the above, for parity tests and for callers that keep their own sampling loop:
 * pgp_ppf_features: computePPF for m (i, j) pairs of scene ids -> features[m][4] (-1: not a key,
 *   NaN inputs) and rows[m] (nullable): index of the key in the table or -1 (PPFMap->find);
 * pgp_stocs_stage_weights: ONE weighting loop of SelectQuadrilateralStoCS (stage 2: base.cc:625-652,
 *   3: :662-699, 4: :713-769) for given base points; cur[nP] in = curr_probabilities_ entering the
 *   loop (stage 2: orig_probabilities_), out = the values the reference leaves (divided by the
 *   sequential float sum when a candidate is present); *sum, *present as in the reference;
 * pgp_base_invariants: TryQuadrilateral for m bases given as scene ids[m][4] (reordered in place),
 *   invariants[m][2], ok[m] (1, or -1 for a bad id). */
int pgp_ppf_features(pgp_ctx* ctx, const int* pairs, int m, int* features, int* rows);
int pgp_stocs_stage_weights(pgp_ctx* ctx, int stage, int base1, int base2, int base3, float* cur, float* sum,
                            int* present);
int pgp_base_invariants(pgp_ctx* ctx, int* ids, int m, float* invariants, int* ok);

/* Replaces ComputeRigidTransformFromCongruentPair + ComputeRigidTransformation
 * (base.cc:1411-1488, 1504-1614) for n congruent pairs.  base_ids[n][4] index the scene cloud
 * (base_3D_ ids), quad_ids[n][4] the search model; only the first three of each are used, as in
 * the reference.  Outputs (host, caller-owned, any of pose/rms nullable):
 *   T[n][16]     centred transform, column-major float = what allTransforms receives (:1468)
 *   pose[n][16]  de-centred transform as double, column-major = allPose[i].first (:1484)
 *   status[n]    1 pushed | 0 rejected (non-orthogonal / rms) | 2 degenerate input | -1 bad index
 *   rms[n]
 * Entries with status != 1 hold NaN transforms (they score 0); the reference simply does not
 * push them -- compact by status to reproduce its lists. */
int pgp_rigid_from_congruent(pgp_ctx* ctx, const int* base_ids, const int* quad_ids, int n,
                             const float centroid_P[3], const float centroid_Q[3], float* T,
                             double* pose, int* status, float* rms);
/* Same with device pointers on `stream` (ids as int4 arrays; d_pose / d_rms nullable). */
int pgp_rigid_from_congruent_device(pgp_ctx* ctx, const int* d_base_ids, const int* d_quad_ids, int n,
                                    const float centroid_P[3], const float centroid_Q[3], float* d_T,
                                    double* d_pose, int* d_status, float* d_rms, void* stream);

/* Replaces MatchSuper4PCS::ExtractPairs (S4/algorithms/super4pcs.cc:193-236; operMode 0) over the
 * search model set by pgp_set_search_model: every ordered pair (a,b), a != b, with
 * | |q_a - q_b| - pair_distance | <= eps (no normal / colour / angle gates, as the fork sets
 * them), written as (j,i),(i,j) for i > j in (i,j) order.  pairs: cap x 2 ints; *n_pairs = the
 * full count (may exceed cap).  Same SET as the reference's octree functor. */
int pgp_extract_pairs(pgp_ctx* ctx, float pair_distance, float eps, int* pairs, int cap, int* n_pairs);

/* Replaces MatchSuper4PCS::FindCongruentQuadrilaterals (super4pcs.cc:78-187) for one base:
 * base[4][3] = positions of base_3D_ (row-major), invariants of the base, threshold =
 * distance_factor * delta (base.cc:1989-1990), P_pairs / Q_pairs = the two pair lists (flat
 * (first,second) ids into the search model: pairs1 / pairs6 of base.cc:1970-1981).  quads:
 * cap x 4 ints in the reference's order (its std::set of (P-pair id, Q-pair id));
 * *n_quads = the full count.  A list of 2^24 pairs or more: PGP_EINVAL (the join's keys hold a
 * pair index in 24 bits).  The call runs on the batch's workspaces: it always discards the
 * context's resident quad batch and its fits (below), whatever it finds; an empty list on either
 * side gives 0 quads and touches nothing. */
int pgp_find_congruent(pgp_ctx* ctx, const float* base, float invariant1, float invariant2, float threshold,
                       const int* P_pairs, int nP, const int* Q_pairs, int nQ, int* quads, int cap,
                       int* n_quads);

/* Replaces Match4PCS::FindCongruentQuadrilaterals (S4/algorithms/4pcs.cc:61-103; the classic 4PCS
 * matcher, not instantiated by the node): for every Q-pair i, every P-pair id whose invariant point
 * e1 = p1 + invariant1 (p2 - p1) lies at SQUARED distance < threshold (strict; kdtree.h:491) of
 * e2 = q1 + invariant2 (q2 - q1) emits (P_pairs[id / 2], Q_pairs[i]) -- `id / 2` as the reference
 * writes it.  Quads come out in (i, id) order (the reference's kd-tree leaves the order inside one i
 * unspecified).  Pair lists as in pgp_find_congruent; *n_quads = full count. */
int pgp_find_congruent_4pcs(pgp_ctx* ctx, float invariant1, float invariant2, float threshold, const int* P_pairs,
                            int nP, const int* Q_pairs, int nQ, int* quads, int cap, int* n_quads);

/* Replaces the loop `for (auto base_it: baseSet) ExtractCongruentSet(base_it)` of Perform_N_steps
 * (base.cc:1855-1874 -> :1929-1993, operMode 1) for ALL bases of an object in one pass: for base b,
 * pairs1 = PPFMap[computePPF(id0, id1)], pairs6 = PPFMap[computePPF(id2, id3)] are looked up in the
 * device table of pgp_set_ppf_map (which must have been given the pair lists), then
 * FindCongruentQuadrilaterals(invariant1, invariant2, threshold, ...) as in pgp_find_congruent.
 * base_ids[n_bases][4]: scene ids in TryQuadrilateral's order; base_xyz[n_bases][4][3]: their
 * (centred) positions; invariants[n_bases][2].  n_quads[n_bases] receives every base's full quad
 * count; the sorted quad lists stay ON THE DEVICE until the next call:
 *   pgp_congruent_batch_quads copies the picked quads (picks[m][2] = (base, j): the j-th quad of
 *     that base in the reference's order) to the host, quads[m][4];
 *   pgp_congruent_batch_fit runs ComputeRigidTransformFromCongruentPair (as
 *     pgp_rigid_from_congruent) on the picked (base, quad) pairs without the quads leaving the
 *     device: the reference's sampling of <= 100 quads per base (base.cc:1858-1872) decides the picks. */
int pgp_find_congruent_batch(pgp_ctx* ctx, const int* base_ids, const float* base_xyz, const float* invariants,
                             int n_bases, float threshold, int* n_quads);
/* pgp_find_congruent_batch for a caller that already holds rows[n_bases][2] (pgp_select_bases_rows, or pgp_ppf_features of
 * the edges (ids 0-1), (ids 2-3)): same quads, same order.  A row outside [-1, rows of the table) is PGP_EINVAL. */
int pgp_find_congruent_batch_rows(pgp_ctx* ctx, const int* base_ids, const float* base_xyz, const float* invariants,
                                  const int* rows, int n_bases, float threshold, int* n_quads);
int pgp_congruent_batch_quads(pgp_ctx* ctx, const int* picks, int m, int* quads);
int pgp_congruent_batch_fit(pgp_ctx* ctx, const int* picks, const int* base_ids, int m, const float centroid_P[3],
                            const float centroid_Q[3], float* T, double* pose, int* status, float* rms);

/* pgp_congruent_batch_fit and the verification of its fits WITHOUT a round trip of the transforms: the fits stay in
 * HBM, every pick is scored there ([Weighted]Verify, base.cc:1885-1901; a fit the reference does not push -- status
 * != 1, base.cc:1467-1485 -- scores 0 and can therefore never enter the strict-`>` walk), and only scores[m],
 * status[m] and the best {index, score} come back.  With pgp_set_exact_records the scores at the walk's decisions are
 * the reference's own sums.  pgp_congruent_batch_fetch then returns the float transform and the double pose of the few
 * picks the caller keeps (the running-best list, the best pose): index[k] -> T[k][16], pose[k][16], either nullable. */
int pgp_congruent_batch_fit_score(pgp_ctx* ctx, const int* picks, const int* base_ids, int m, const float centroid_P[3],
                                  const float centroid_Q[3], int mode, float gate_deg, float* scores, int* status,
                                  int* best_index, float* best_score);
int pgp_congruent_batch_fetch(pgp_ctx* ctx, const int* index, int k, float* T, double* pose);
/* pgp_congruent_batch_fit_score and everything the caller of Perform_N_steps reads afterwards, in ONE call with ONE copy
 * back and ONE synchronisation: the running-best walk of the verification loop (base.cc:1891-1908, what pgp_running_best
 * computes on the host -- run with pgp_set_exact_records for the reference's own decisions) on the device, the poses it
 * keeps, the best pose (base.cc:1787-1790) and the scene points the best pose registers (pgp_registered).
 *   n_list: the number of records; list_index / list_score / list_T [.][16] / list_pose [.][16] hold the first
 *     min(n_list, list_cap) of them in walk order (list_cap <= 4096; n_list > list_cap: call pgp_congruent_batch_fetch
 *     for the rest -- the scores stay on the device, the fits too);
 *   n_pushed (nullable): the number of fits the reference pushes (status == 1, base.cc:1467-1485);
 *   best_index = -1: no hypothesis scored above 0 -- best_T / best_pose / registered are then left alone, n_registered = 0;
 *   registered: room for every model point (pgp_set_model's n).  Nullable outputs: n_pushed, best_*, registered. */
int pgp_congruent_batch_fit_score_list(pgp_ctx* ctx, const int* picks, const int* base_ids, int m, const float centroid_P[3],
                                       const float centroid_Q[3], int mode, float gate_deg, int list_cap, int* n_list,
                                       int* list_index, float* list_score, float* list_T, double* list_pose, int* n_pushed,
                                       int* best_index, float* best_score, float* best_T, double* best_pose, int* registered,
                                       int* n_registered);

/* The same call with the sampling of the quads (base.cc:1858-1866: at most 100 random quads per base) done ON THE DEVICE, where
 * the quad counts are: no picks to draw on the host between the congruent sets and the fits, none to upload.  The draw is a
 * function of (seed, base, the base's quad count) alone -- a counter-based splitmix64 generator per base feeding Floyd's subset
 * algorithm (max_per_base steps whatever the count, every subset equally likely), handed out in ascending order; a base with
 * fewer quads hands out all of them --, so the bases are drawn side by side, and pgp_sample_quads is the same function on the
 * host (the reference draws from rand() seeded from the clock: any uniform sample of max_per_base distinct quads is its
 * behaviour).  Works on the batch pgp_find_congruent_batch[_rows]
 * left resident; base_ids[n_bases][4] as there.  picks_out (nullable, room for n_bases x max_per_base x 2) / n_picks
 * (nullable) return what was drawn: the picks a pgp_congruent_batch_fit_score_list call would need for the same result.
 * 1 <= max_per_base <= 128. */
int pgp_congruent_batch_sample_fit_score_list(pgp_ctx* ctx, unsigned long long seed, int max_per_base, const int* base_ids,
                                              const float centroid_P[3], const float centroid_Q[3], int mode, float gate_deg,
                                              int list_cap, int* n_list, int* list_index, float* list_score, float* list_T,
                                              double* list_pose, int* n_pushed, int* best_index, float* best_score, float* best_T,
                                              double* best_pose, int* registered, int* n_registered, int* picks_out, int* n_picks);
/* Host helper: the picks that call draws, from the quad counts alone.  picks (nullable: count only) [sum][2] = (base, quad). */
int pgp_sample_quads(unsigned long long seed, const int* n_quads, int n_bases, int max_per_base, int* picks, int* n_picks);

/* ---- The matcher's tetrahedron-base mode (operMode 2, "V4PCS"): pose hypotheses from POSITIONS ALONE ----------------------
 * Needs the scene (pgp_set_scene, positions), the search model (pgp_set_search_model) and, for the scores of
 * pgp_v4pcs_hypotheses, the validation model (pgp_set_model); no normals, no pair-feature table, no probability image.
 * Its workspaces are its own: a resident pgp_find_congruent_batch batch survives these calls and the other way round.
 *
 * LIMIT: the widest-triangle rule places bases on the EXTREME points of the scene cloud, so the mode wants a clean segment.
 * In a CPU prototype of the rule (300-point search model, 155-point clean segment) all 100 bases lay on the object; with 40
 * clutter points in a box padded by 5 cm around the segment, none of 100 did.
 *
 * pgp_select_tetrahedron_bases replaces n_attempts calls of Match4PCSBase::SelectTetrahedronBase (base.cc:466-503, over
 * SelectRandomTriangle :377-410) on the scene: a random first point; over triangle_trials (reference: 1000) random
 * (second, third) draws the triangle with the largest |u x w| (strict `>` from 0: the first maximum in trial order) whose
 * two edges from the first point are both shorter than max_base_diameter; over fourth_trials (reference: 100) random fourth
 * points the one with the largest |(v1 x v2) . v3| / 6 (strict `>` from 0: a zero volume never wins).  One attempt is one
 * (triangle, fourth point) trial: a caller who wants 100 bases asks for more attempts and keeps the first 100 with status 1.
 * max_base_diameter (> 0): the reference takes the largest of 1000 random pair distances of the search model
 * (base.cc:274-287); the model's diameter or any such estimate serves.
 * The reference draws from rand() seeded from the clock; here attempt a draws from the counter-based generator of
 * pgp_sample_quads: with st = state(seed, a) and r(i) = variate(st, i) % n: first = r(0); trial i: second = r(1 + 2 i),
 * third = r(2 + 2 i); fourth draw k: r(1 + 2 triangle_trials + k).  Floats: every operation rounded on its own, cross products
 * as (a.y b.z - a.z b.y, ...), dot products and squared norms as (x x + y y) + z z, correctly rounded sqrt and divide.
 * ids[n_attempts][4] (scene ids; -1 where status is 0), dist[n_attempts][6] = |b0 b1|, |b0 b2|, |b0 b3|, |b1 b2|, |b1 b3|,
 * |b2 b3| (d1 .. d6 of FindCongruentQuadrilateralsV4PCS; 0 where status is 0), status[n_attempts]: 1 = base, 0 = none (no
 * triangle within the diameter, or every fourth point coplanar).  The same bits from call to call.  Host pointers, synchronous. */
int pgp_select_tetrahedron_bases(pgp_ctx* ctx, unsigned long long seed, int n_attempts, int triangle_trials, int fourth_trials,
                                 float max_base_diameter, int* ids, float* dist, int* status);

/* Replaces FindCongruentQuadrilateralsV4PCS (base.cc:978-1044) and the six ExtractPairs calls that feed it (:1963-1969,
 * :1998-2020) for one base, over the search model (4 .. PGP_V4PCS_MAX_POINTS points, else PGP_EINVAL; none: PGP_ESTATE):
 * (v1, v2, v3, v4) is a quad iff (v1,v2)~d1, (v1,v3)~d2, (v1,v4)~d3, (v2,v3)~d4, (v2,v4)~d5 and (v3,v4)~d6, where (a,b)~d
 * is pgp_extract_pairs' predicate: a != b and not (| |q_a - q_b| - d | > eps), float distance, comparison in double,
 * inclusive; symmetric in (a, b).  dist[6] = d1 .. d6 as pgp_select_tetrahedron_bases returns them, eps = distance_factor *
 * delta, un-normalised.  If any of the six pair sets is empty there is no quad (:2022-2024).
 * Quads come out in ASCENDING (v1, v2, v3, v4) order (the reference's goes through an unordered_set and is unspecified).
 * quads: cap x 4 ints, the first min(*n_quads, cap) quads in that order; *n_quads = the full count.
 * COST: the count visits every (v1, v2, v3) that passes its three predicates, so the time grows with the number of QUADS, not
 * with cap / per_base_cap (which bound only what is written): 100 bases on a 4096-point surface with eps = 5 mm hold 164 M
 * quads and take 186 ms; an eps as large as the model makes the count cubic in the model's size, seconds per base. */
#define PGP_V4PCS_MAX_POINTS 4096
int pgp_find_congruent_v4pcs(pgp_ctx* ctx, const float dist[6], float eps, int* quads, int cap, long long* n_quads);
/* The same for n_bases bases at once (dist[n_bases][6]; at most 65535).  n_quads[n_bases] (nullable): every base's full
 * count; n_stored[n_bases] (nullable): min(n_quads, per_base_cap) -- a base KEEPS its first per_base_cap quads in ascending
 * order, on the device, until the next batch call or pgp_set_search_model; whoever samples quads afterwards draws from that
 * kept prefix.  pgp_v4pcs_batch_quads copies picked quads to the host: picks[m][2] = (base, j), the j-th kept quad of that
 * base, quads[m][4]; a pick at or past n_stored is PGP_EINVAL, no resident batch PGP_ESTATE. */
int pgp_find_congruent_v4pcs_batch(pgp_ctx* ctx, const float* dist, int n_bases, float eps, int per_base_cap, long long* n_quads,
                                   int* n_stored);
int pgp_v4pcs_batch_quads(pgp_ctx* ctx, const int* picks, int m, int* quads);

/* The mode as one call (Perform_N_steps in operMode 2, base.cc:1837-1842, :1855-1874, :1494-1499):
 *   1. max_attempts attempts of pgp_select_tetrahedron_bases(seed, ...); the first n_bases with status 1 are the bases
 *      (fewer when the attempts run out);
 *   2. pgp_find_congruent_v4pcs_batch(their dist, eps, per_base_cap);
 *   3. the picks pgp_sample_quads(seed, n_stored, max_per_base) draws (at most max_per_base <= 128 kept quads per base);
 *   4. the fit of pgp_rigid_from_congruent: the base's four scene ids against the quad's four model ids;
 *   5. the plain score of pgp_score_lcp (PGP_MODE_PLAIN; plain Verify, base.cc:1498-1499).  A fit with status != 1 scores 0.
 * Outputs, with room for n_bases x max_per_base hypotheses: T[.][16], pose[.][16] (nullable), status[.], scores[.],
 * picks[.][2] (nullable); *n_hyp = how many there are; *n_bases / base_ids[n_bases][4] (nullable): the bases found.
 * best_index (nullable) = the lowest index of the greatest score, -1 when no hypothesis scores above 0 (best_T / best_pose
 * are then left alone); best_score, best_T[16], best_pose[16] nullable.  The join's quads stay resident as after step 2.
 * Host pointers, synchronous. */
typedef struct pgp_v4pcs_options {
  unsigned long long seed;
  int n_bases;             /* 100 */
  int max_attempts;        /* 200 */
  int triangle_trials;     /* 1000 */
  int fourth_trials;       /* 100 */
  float max_base_diameter; /* no default: the model's diameter or an estimate of it, > 0 */
  float eps;               /* 0.005 */
  int max_per_base;        /* 100 */
  int per_base_cap;        /* 4096 */
} pgp_v4pcs_options;
int pgp_v4pcs_default_options(pgp_v4pcs_options* opt);
int pgp_v4pcs_hypotheses(pgp_ctx* ctx, const pgp_v4pcs_options* opt, const float centroid_P[3], const float centroid_Q[3],
                         int* n_bases, int* base_ids, int* n_hyp, float* T, double* pose, int* status, float* scores, int* picks,
                         int* best_index, float* best_score, float* best_T, double* best_pose);

/* ---- The matcher's classic mode (operMode 0, "Super4PCS"): wide planar bases, two pair lists per base -----------------------
 * Needs the scene (pgp_set_scene, positions), the search model (pgp_set_search_model) and, for the scores of
 * pgp_super4pcs_hypotheses, the validation model (pgp_set_model); no normals, no pair-feature table, no probability image.
 *
 * pgp_select_wide_bases replaces n_attempts calls of Match4PCSBase::SelectQuadrilateral (base.cc:505-580, over
 * SelectRandomTriangle :377-410 and TryQuadrilateral :415-464) on the scene.  One attempt is one triangle and one search for
 * the fourth point; the reference's retry loop becomes "ask for more attempts and keep the first n with status 1".
 * Triangle: the rule, the draw and the rounding of pgp_select_tetrahedron_bases (first = r(0); trial i: second = r(1 + 2 i),
 * third = r(2 + 2 i); the widest |u x w|, strict `>` from 0, both edges from the first point shorter than max_base_diameter).
 * Fourth point (:527-565): with the nine coordinates of the triangle as doubles, denom = -x3 y2 z1 + x2 y3 z1 + x3 y1 z2 -
 * x1 y3 z2 - x2 y1 z3 + x1 y2 z3 (left to right, products as (a b) c), narrowed to float; denom == 0: status 0.  A, B, C =
 * (their double numerators, :542-547) / (double)denom, narrowed to float.  too_small = (float)pow((double)(max_base_diameter *
 * 0.1f), 2).  Scene point i qualifies when its squared distances to the three, (x x + y y) + z z in float, are all >= too_small;
 * its distance = (float)fabs((double)((A x + B y) + C z) - 1.0) with float products and sums.  The smallest distance wins,
 * strict `<` from FLT_MAX walking i upward: the lowest index among equals, never a NaN or an infinite one; no winner: status 0.
 * TryQuadrilateral then reorders the four ids and gives the invariants, as pgp_base_invariants does.
 * ids[n_attempts][4] (scene ids in their final order; -1 where status is 0), invariants[n_attempts][2], dist[n_attempts][2] =
 * |b0 b1|, |b2 b3| of the reordered base (distance1 / distance6 of :1952-1953; norms as x x + (y y + z z), correctly rounded
 * sqrt; 0 where status is 0), status[n_attempts]: 1 = base, 0 = none.  max_base_diameter <= 0 or a negative count: PGP_EINVAL;
 * no scene: PGP_ESTATE.  The same bits from call to call.  Host pointers, synchronous. */
int pgp_select_wide_bases(pgp_ctx* ctx, unsigned long long seed, int n_attempts, int triangle_trials, float max_base_diameter,
                          int* ids, float* invariants, float* dist, int* status);

/* pgp_extract_pairs for n_lists distances at once (the two ExtractPairs calls per base of :1963-1969): list k is exactly what
 * pgp_extract_pairs(dist[k], eps) returns -- the same predicate, the same order ((j, i) then (i, j) for i > j, in (i, j)
 * order) -- and all lists STAY ON THE DEVICE, in a buffer of the context's own, until the next pgp_extract_pairs_batch or
 * pgp_set_search_model.  n_pairs[n_lists] (nullable): pairs per list.  A list of 2^24 pairs or more, or 2^31 in all:
 * PGP_EINVAL (the join's keys hold a pair index in 24 bits); at most 131070 lists over at most 65536 points; no search model:
 * PGP_ESTATE.  pgp_extract_pairs_batch_fetch copies list `list` to the host: *n_pairs = its full count, pairs[cap][2] receives
 * the first min(count, cap); a list out of range: PGP_EINVAL, no resident lists: PGP_ESTATE. */
int pgp_extract_pairs_batch(pgp_ctx* ctx, const float* dist, int n_lists, float eps, int* n_pairs);
int pgp_extract_pairs_batch_fetch(pgp_ctx* ctx, int list, int* pairs, int cap, int* n_pairs);

/* pgp_find_congruent_batch with every base's pair lists taken from the lists of pgp_extract_pairs_batch instead of the
 * pair-feature table: lists[n_bases][2] = (pairs1, pairs6) list numbers, base_xyz[n_bases][4][3], invariants[n_bases][2],
 * n_quads[n_bases].  Per base the quads and their order are those of pgp_find_congruent on the two fetched lists; a base with
 * an empty list has none (:1984).  The result is THE resident quad batch of the context (there is one): pgp_congruent_batch_quads,
 * _fit, _fit_score, _fit_score_list, _sample_fit_score_list and _fetch work on it unchanged; it replaces a batch of
 * pgp_find_congruent_batch and is replaced by one; a new pgp_extract_pairs_batch or pgp_set_search_model discards it, and so,
 * always, does a pgp_find_congruent with two non-empty lists
 * (PGP_ESTATE from the calls above).  A list number out of range: PGP_EINVAL; no resident lists: PGP_ESTATE. */
int pgp_find_congruent_batch_lists(pgp_ctx* ctx, const float* base_xyz, const float* invariants, const int* lists, int n_bases,
                                   float threshold, int* n_quads);

/* The mode as one call (Perform_N_steps in operMode 0, base.cc:1837-1842, :1855-1874, :1494-1499):
 *   1. max_attempts attempts of pgp_select_wide_bases(seed, ...); the first n_bases with status 1 are the bases (fewer when
 *      the attempts run out);
 *   2. pgp_extract_pairs_batch over their 2 n distances (base b: lists 2 b and 2 b + 1), with eps;
 *   3. pgp_find_congruent_batch_lists, threshold = eps (distance_factor is 1);
 *   4. the picks pgp_sample_quads(seed, n_quads, max_per_base) draws (max_per_base <= 128);
 *   5. the fit of pgp_rigid_from_congruent: the base's four scene ids against the quad's four model ids;
 *   6. the plain score of pgp_score_lcp (PGP_MODE_PLAIN; plain Verify, :1494-1499).  A fit with status != 1 scores 0.
 * Outputs as pgp_v4pcs_hypotheses, with room for n_bases x max_per_base hypotheses, plus base_invariants[n_bases][2]
 * (nullable).  best_index = the lowest index of the greatest score, -1 when no hypothesis scores above 0.  No base found: zero
 * hypotheses, best_index -1, PGP_OK.  The pair lists and the quad batch stay resident as after steps 2 and 3.
 * Host pointers, synchronous. */
typedef struct pgp_super4pcs_options {
  unsigned long long seed;
  int n_bases;             /* 100 */
  int max_attempts;        /* 200 */
  int triangle_trials;     /* 1000 */
  float max_base_diameter; /* no default: the model's diameter or an estimate of it, > 0 */
  float eps;               /* 0.005 */
  int max_per_base;        /* 100 */
} pgp_super4pcs_options;
int pgp_super4pcs_default_options(pgp_super4pcs_options* opt);
int pgp_super4pcs_hypotheses(pgp_ctx* ctx, const pgp_super4pcs_options* opt, const float centroid_P[3], const float centroid_Q[3],
                             int* n_bases, int* base_ids, float* base_invariants, int* n_hyp, float* T, double* pose, int* status,
                             float* scores, int* picks, int* best_index, float* best_score, float* best_T, double* best_pose);

/* ---- The classic mode's pair gates: Match4PCSOptions::max_normal_difference, max_color_distance, max_translation_distance and
 * max_angle (S4/shared4pcs.h:157-163) as PairCreationFunctor::process applies them (S4/pairCreationFunctor.h:167-253) ----------
 * The fork ships all four switched off (S4/super4pcs_test.cc:91-99) and the calls above behave so.  The calls below apply them
 * while the pair lists are made; the join, the sampling, the fits and the scores take the gated lists as they take any.
 *
 * Point attributes.  The scene's normals are the ones pgp_set_scene[_device] took.  pgp_set_scene_colors: rgb[n][3], n = the
 * resident scene's count.  pgp_set_search_model_attributes: nrm[n][3] and rgb[n][3], either may be NULL, n = the resident
 * search model's count; what is NULL becomes absent (a call replaces both).  A point with rgb[0] < 0 has no colour (Point3D's
 * default, (-1, -1, -1)); absent normals count as zero normals, absent colours as (-1, -1, -1).  pgp_set_scene[_device]
 * discards the scene's colours, pgp_set_search_model the search model's attributes.  A NaN or an infinite value, or a wrong n:
 * PGP_EINVAL; no scene / no search model: PGP_ESTATE.  Host pointers, synchronous. */
int pgp_set_scene_colors(pgp_ctx* ctx, const float* rgb, int n);
int pgp_set_search_model_attributes(pgp_ctx* ctx, const float* nrm, const float* rgb, int n);

/* The gates.  pgp_pair_gates_default switches everything off (host only, no context).  A NaN or an infinite field, or a
 * max_angle above 180: PGP_EINVAL from the calls that take the struct.
 *
 * List k has a base edge, the scene ids (b1, b2) = base_ids[k]; its record is made on the device: pna = |n_b1 - n_b2|
 * (base.cc:1956-1957), seg1 = (pos_b2 - pos_b1).normalized() (:157; Eigen's: v / sqrt(z) when z = |v|^2 > 0, else v), the two
 * positions and the two colours.  For every i > j of the search model that passes pgp_extract_pairs' distance predicate
 * (unchanged), p = Q[j], q = Q[i].  Every float operation is rounded on its own, three-vector reductions are x x + (y y + z z),
 * square roots and divisions are correctly rounded, |v| is a float unless widened:
 *   normals (:182-196), when max_normal_difference > 0 and |n_q|^2 > 0 and |n_p|^2 > 0:
 *     thr = (float)(0.5 * (double)max_normal_difference * M_PI / 180.0); f = (double)|n_q - n_p|, s = (double)|n_q + n_p|;
 *     d = (float)min(fabs(f - (double)pna), fabs(s - (double)pna)) (std::min: the second when it is smaller, else the first);
 *     the pair is dropped when d > thr.
 *   colour (:198-208), when max_color_distance > 0 and p, q, b1, b2 all have rgb[0] >= 0: dropped unless
 *     (double)|rgb_p - rgb_b1| < (double)max and (double)|rgb_q - rgb_b2| < (double)max -- both strict.
 *   translation (:210-216), when max_translation_distance > 0: dropped unless (double)|pos_p - pos_b1| < (double)max and
 *     (double)|pos_q - pos_b2| < (double)max -- both strict.  Positions are the resident ones: centre both clouds as the
 *     reference does (pgp_center).
 *   angle (:238-251), when max_angle > 0: seg2 = (pos_q - pos_p).normalized(), c = (float)cos((double)max_angle * M_PI / 180.0)
 *     (on the host); (j, i) is emitted iff dot(seg1, seg2) >= c, (i, j) iff dot(seg1, -seg2) >= c: either, both or neither; a NaN
 *     dot emits nothing.  The reference writes acos(dot) <= max_angle * M_PI / 180.0: the cosine form decides differently only
 *     for dots within rounding of the threshold, and keeps acos off the device.  With the gate off both pairs are emitted.
 *   directed = 0 is the reference's rule: colour and translation are tested once per unordered pair, the lower index against
 *     b1, and then both orders may come out -- so (i, j) can be emitted although q does not match b1.  directed = 1 tests each
 *     ordered pair (a, b) in its own direction, a against b1 and b against b2, and emits it iff its own colour, translation and
 *     angle tests pass.  The normal gate is symmetric either way.
 * Order inside a list: rows i ascending, j ascending within a row, (j, i) before (i, j).
 *
 * pgp_extract_pairs_batch_gated leaves THE resident pair lists of the context, exactly as pgp_extract_pairs_batch does: the
 * same buffer, the same limits (2^24 pairs per list, 2^31 in all, 131070 lists, 65536 points), the same discard rules;
 * pgp_extract_pairs_batch_fetch, pgp_find_congruent_batch_lists and everything behind them work on them unchanged.
 * base_ids[n_lists][2]: scene ids.  gates NULL or every gate off: the lists are bit-equal to pgp_extract_pairs_batch's and
 * base_ids may be NULL.  A base id outside the scene: PGP_EINVAL; gates switched on with no scene: PGP_ESTATE.
 *
 * pgp_super4pcs_hypotheses_gated is pgp_super4pcs_hypotheses with step 2 gated: list 2 b has the base edge (ids 0, 1) of base
 * b, list 2 b + 1 the edge (ids 2, 3) (base.cc:1964-1968).  gates NULL or all off: every output is bit-equal.
 *
 * Not here: the Euler-angle test that max_angle >= 0 also switches on in ComputeRigidTransformation (base.cc:1567-1582) -- the
 * fit stays as shipped; gates on the tetrahedron mode's six pair sets (its bit matrices are symmetric) and in
 * pgp_find_congruent_4pcs; the single-list pgp_extract_pairs; pgp_multi_*. */
typedef struct pgp_pair_gates {
  float max_normal_difference;    /* degrees; <= 0: off */
  float max_color_distance;       /* <= 0: off */
  float max_translation_distance; /* <= 0: off */
  float max_angle;                /* degrees, (0, 180]; <= 0: off */
  int directed;                   /* 0: the reference's rule; 1: every ordered pair in its own direction */
} pgp_pair_gates;
int pgp_pair_gates_default(pgp_pair_gates* gates);
int pgp_extract_pairs_batch_gated(pgp_ctx* ctx, const float* dist, const int* base_ids, int n_lists, float eps,
                                  const pgp_pair_gates* gates, int* n_pairs);
int pgp_super4pcs_hypotheses_gated(pgp_ctx* ctx, const pgp_super4pcs_options* opt, const pgp_pair_gates* gates,
                                   const float centroid_P[3], const float centroid_Q[3], int* n_bases, int* base_ids,
                                   float* base_invariants, int* n_hyp, float* T, double* pose, int* status, float* scores, int* picks,
                                   int* best_index, float* best_score, float* best_T, double* best_pose);

/* ICP refinement. Replaces the inner loop behind pcl::recognition::TrimmedICP::align
 * (PPE/hypothesis_verification/mcts/UCTState.cpp:137-139,194; PPE/misc/utilities.cpp:666-676) and
 * pcl::IterativeClosestPoint::align (utilities.cpp:697-703; PPE/data_layer/SceneCfg.cpp:101,135-141)
 * for a batch of n initial guesses at once.  PCL is not vendored in the reference, so the
 * arithmetic is this library's own statement of the algorithm: exact nearest neighbour
 * (an index over the static target, identical to an exhaustive search: smallest d2, then lowest
 * index), keep the |trim*n_src| closest pairs (or those within max_corr_dist), Horn's
 * closed-form rigid update, repeat while mean-squared-distance / previous < energy_ratio. */
typedef struct {
  int max_iterations;    /* <= 0: 100 (utilities.cpp:698); TrimmedICP itself is unbounded */
  float trim_fraction;   /* (0,1]: k = (int)|trim * n_src| (UCTState.cpp:176,194); 1 = use all */
  float max_corr_dist;   /* > 0: drop pairs farther than this instead of trimming (State.cpp:139) */
  float energy_ratio;    /* setNewToOldEnergyRatio: 1.0 at the call sites (UCTState.cpp:139) */
} pgp_icp_params;

/* src: points that are moved (the scene segment in the reference), tgt: the cloud searched for
 * neighbours (the model).  T[n][16]: column-major float, source frame -> target frame; initial
 * guesses in, refined transforms out (UCTState.cpp:184-203 inverts the pose before and after).
 * energy[n] (nullable): final mean squared distance of the selected pairs; iters[n] (nullable).
 * Host pointers, synchronous. */
int pgp_icp_refine(pgp_ctx* ctx, const float* src_xyz, int n_src, const float* tgt_xyz, int n_tgt,
                   float* T, int n, const pgp_icp_params* params, float* energy, int* iters);
/* Device pointers: d_src / d_tgt are float4 arrays {x,y,z,-}; enqueued on `stream`.  Default
 * (target index fits LDS, n_src <= 4096): the index is built (the call synchronises once, for the
 * target's bounding box) and ONE launch runs every iteration of every pose.  Otherwise the
 * iterations are driven from the host (many workgroups per pose) and the call synchronises the
 * stream every four iterations to test for convergence.  While few poses are in flight (n x 4 or
 * n x 2 <= the device's compute units) that ONE launch has 4 or 2 workgroups per pose sharing the search, one per
 * compute unit (a plain launch of a grid that fits the device -- PGP_COOPERATIVE_LAUNCH=1: hipLaunchCooperativeKernel,
 * whose queue makes the hardware scheduler time-slice the GPU between processes; not on a stream that is being
 * captured; PGP_ICP_WGS=1 switches the sharing off).  Should the
 * workgroups of a pose ever fail to meet (another process holding the GPU's compute units for seconds), the pose's
 * first workgroup searches every query again and finishes the pose alone, inside the same launch -- the caller always
 * receives refined transforms, the same bits.  Clustered launches of one process never overlap on a device.
 * The scene-sized capped form in one launch (n_src > 4096, a correspondence cap, no trimming, n <= 64) reports a pose
 * whose work did not arrive within the same clock bound with d_iters = -1 and leaves its transform where it was; the
 * host-pointer calls then redo the job with the host-driven iterations themselves.
 * Checker paths, same results:
 * PGP_ICP_NN=scan (exhaustive search), PGP_ICP_PERSIST=0 (index, host-driven iterations),
 * PGP_ICP_SPLIT=0/1 (the exhaustive persistent / host-driven kernels). */
int pgp_icp_refine_device(pgp_ctx* ctx, const float* d_src4, int n_src, const float* d_tgt4, int n_tgt,
                          float* d_T, int n, const pgp_icp_params* params, float* d_energy,
                          int* d_iters, void* stream);

/* SEVERAL (segment, target) pairs refined by ONE launch: the children of an MCTS expansion belong to different objects
 * (PPE/hypothesis_verification/mcts/UCTSearch.cpp:200-266 -> UCTState.cpp:121-204) and the node's object loop
 * (PPE/data_layer/SceneCfg.cpp:379-402) refines the candidates of every object of a frame -- through
 * pgp_icp_refine_device that is one launch per object, each wanting the whole chip.  Every job names the context
 * that keeps its target's index (pgp_icp_target_token applies per context), its clouds and its own transform /
 * energy / iteration arrays; all contexts on one device.  Results are bit-identical to one pgp_icp_refine_device
 * call per job -- which is also what happens when the single launch cannot serve the jobs (more than 8 of them, a
 * target whose index does not fit a compute unit's LDS, a segment beyond 4096 points, or two jobs that name the SAME
 * context: a context keeps one target index, so give every job of a launch its own context when the single launch
 * matters).  Enqueued on `stream`. */
typedef struct {
  pgp_ctx* ctx;
  const float* d_src4;   /* float4 {x,y,z,-} [n_src] */
  int n_src;
  const float* d_tgt4;   /* float4 {x,y,z,-} [n_tgt] */
  int n_tgt;
  float* d_T;            /* [n][16] in/out */
  int n;
  float* d_energy;       /* [n], nullable */
  int* d_iters;          /* [n], nullable */
} pgp_icp_job;
int pgp_icp_refine_multi_device(const pgp_icp_job* jobs, int n_jobs, const pgp_icp_params* params, void* stream);

/* The k best-scoring hypotheses of a scored batch, in HBM: d_T_out[k][16] = their transforms in descending score
 * order (equal scores: lower index first -- a stable argsort of -score), inverted as rigid transforms {R^T, -R^T t}
 * when invert != 0 (UCTState.cpp:184-185 hands `pose.inverse()` to ICP); d_index_out[k] (nullable) = their indices,
 * *d_n_out = how many of the k have a score > 0 (the rest: index -1, identity).  The hand-off
 * HypothesisSelection.cpp:248-257 -> UCTState::performTrICP without a trip to the host.  Enqueued on `stream`. */
int pgp_select_top_device(pgp_ctx* ctx, const float* d_T, const float* d_scores, int n, int k, int invert,
                          float* d_T_out, int* d_index_out, int* d_n_out, void* stream);

/* The index over the target is built per call unless the caller vouches that the target has not
 * changed: after pgp_icp_target_token(ctx, token != 0), *_device calls with the same (d_tgt pointer,
 * n_tgt, token) reuse the resident index (the reference builds TrimmedICP's search structure once per
 * model, UCTState.cpp:137-139).  token 0 (default) = rebuild on every call.  The host-pointer calls do
 * this by themselves with a hash of the target's coordinates. */
int pgp_icp_target_token(pgp_ctx* ctx, unsigned long long token);

/* The other ICP forms of the call sites, on the same kernels (csrc/icp.hip).  Fields <= 0 / < 0 switch
 * a rule off as noted; pgp_icp_default_options() fills the TrimmedICP form of pgp_icp_params.
 *   greedy_bfs/State.cpp:139-142   pcl::IterativeClosestPoint, setMaxCorrespondenceDistance(max_corr),
 *                                  50 iterations, setTransformationEpsilon(1e-8):
 *                                  {50, 1, max_corr, 0, 0, 1e-8f, 0, 1e-12f, 0, 0, 0, 0}
 *   misc/utilities.cpp:697-703     pcl::IterativeClosestPoint, 100 iterations, PCL defaults:
 *                                  {100, 1, 0, 0, 0, 0.f, 0, 1e-12f, 0, 0, 0, 0}
 *   misc/utilities.cpp:709-739     pcl::IterativeClosestPointWithNormals: the same with error_metric 1
 *   misc/utilities.cpp:744-838     libpointmatcher chain: {100, 0.75f, 0, 0, 0, -1, 0, -1, 0.001f, 0.005f, 4, 0}
 *   data_layer/SceneCfg.cpp:135-141  table ICP on scene-sized clouds: max_corr 0.01, 50 iterations,
 *                                  transformation epsilon 1e-9 (nn_search 0 picks the grid search there) */
typedef struct {
  int max_iterations;            /* <= 0: 100 */
  float trim_fraction;           /* (0,1]: keep the |trim * n_src| closest pairs; 1 (or <= 0) = all */
  float max_corr_dist;           /* > 0: pairs farther than this are dropped (instead of trimming) */
  float energy_ratio;            /* > 0: go on only while E / E_old < ratio (TrimmedICP); <= 0: off */
  int error_metric;              /* 0 point-to-point (Horn closed form), 1 point-to-plane (linearised
                                    least squares; needs target normals) */
  float transformation_epsilon;  /* >= 0: stop when an iteration's update has cos(angle) >= 1 - eps and
                                    |t|^2 <= eps (pcl DefaultConvergenceCriteria); < 0: off */
  float relative_mse;            /* > 0: stop when |E - E_old| / E_old < this; <= 0: off */
  float absolute_mse;            /* >= 0: stop when |E - E_old| < this (PCL: 1e-12); < 0: off */
  float min_diff_rot;            /* > 0 with min_diff_trans > 0: libpointmatcher's                  */
  float min_diff_trans;          /*   DifferentialTransformationChecker on the last smooth_length    */
  int smooth_length;             /*   iterations (1..8)                                              */
  int nn_search;                 /* 0 auto, 1 exhaustive scan, 2 uniform grid (needs max_corr_dist > 0),
                                    3 exact index of the static target (its image in LDS up to ~6000 points,
                                    read from L2 beyond; fails above 65 535 points); auto = 3 when it applies,
                                    else 2 for capped scene-sized searches, else 1.  All return identical results. */
} pgp_icp_options;
int pgp_icp_default_options(pgp_icp_options* opt);
/* tgt_nrm: n_tgt x 3 unit normals of the target (nullable unless error_metric is 1).  Otherwise as
 * pgp_icp_refine / pgp_icp_refine_device (d_tgt_n4: float4 {nx,ny,nz,-}). */
int pgp_icp_refine_ex(pgp_ctx* ctx, const float* src_xyz, int n_src, const float* tgt_xyz, const float* tgt_nrm,
                      int n_tgt, float* T, int n, const pgp_icp_options* opt, float* energy, int* iters);
int pgp_icp_refine_ex_device(pgp_ctx* ctx, const float* d_src4, int n_src, const float* d_tgt4,
                             const float* d_tgt_n4, int n_tgt, float* d_T, int n, const pgp_icp_options* opt,
                             float* d_energy, int* d_iters, void* stream);

/* Segment pre-processing in front of the path (PPE/hypothesis_generation/ObjectPoseCandidateSet.cpp:
 * 28-51): pcl::RadiusOutlierRemoval(radius 0.03, min neighbours 10) followed by
 * flipNormalTowardsViewpoint((0,0,0)) + re-normalisation.  PCL is not vendored, so the
 * filter follows PCL 1.7 / FLANN as published: k = number of points with squared distance
 * STRICTLY below radius^2 (the point itself included), keep iff k > min_neighbors.
 * xyz / nrm: n x 3 (nrm nullable); keep[n] receives 0/1; nrm_out (nullable, n x 3) the flipped,
 * re-normalised normals of ALL points (callers compact by keep).  *n_kept = number kept (the
 * node bails out when <= 30 remain, :34-37).  Builds a temporary index in the context: call it
 * before pgp_set_scene.  Host pointers, synchronous. */
int pgp_radius_outlier_filter(pgp_ctx* ctx, const float* xyz, const float* nrm, int n, float radius,
                              int min_neighbors, unsigned char* keep, float* nrm_out, int* n_kept);

/* The part of a segment that the objects already placed do NOT explain, in front of the ICP refinement of
 * the next object (UCTState::performTrICP, PPE/hypothesis_verification/mcts/UCTState.cpp:142-174): a segment
 * point is dropped when any point of any placed object's model, moved to that object's pose, lies within
 * `radius` of it (pointRemovalThreshold = 0.008, UCTState.cpp:9; strictly below, as FLANN's radius search).
 *   seg_xyz: n x 3; model_xyz: the placed objects' model points one object after the other;
 *   model_offsets[n_objects + 1]: object k owns points model_offsets[k] .. model_offsets[k + 1] - 1;
 *   T: n_objects x 16 column-major float, model -> the segment's frame (the objects' poses);
 *   keep[n]: 1 = unexplained (stays in the cloud handed to pgp_icp_refine), *n_kept (nullable) their number.
 * n_objects == 0 keeps everything (the reference skips the step for the first object).  Host pointers,
 * synchronous.  PCL / FLANN are not vendored: unpinned against their bits. */
int pgp_unexplained_segment(pgp_ctx* ctx, const float* seg_xyz, int n, const float* model_xyz, const int* model_offsets,
                            const float* T, int n_objects, float radius, unsigned char* keep, int* n_kept);

/* pgp_set_scene with DEVICE pointers (d_xyz: n x 3 floats; d_nrm: n x 3 or NULL; d_weight: n or NULL):
 * the segment a previous device call produced (pgp_backproject_depth_device, pgp_voxel_grid_device)
 * becomes the scene without a host round trip.  Enqueued on `stream`, which is synchronised (the
 * index build needs the bounding box and two counts on the host). */
int pgp_set_scene_device(pgp_ctx* ctx, const float* d_xyz, const float* d_nrm, const float* d_weight, int n,
                         float delta, void* stream);

/* Replaces pcl::VoxelGrid<PointXYZRGB> with setLeafSize(leaf, leaf, leaf) in front of the segment
 * (PPE/segmentation/Segmentation.cpp:234-237; positions only).  PCL is not vendored: PCL 1.7's
 * published algorithm -- bounds over the finite points, voxel index (ijk relative to
 * floor(min * 1/leaf)) = i + j * div_x + k * div_x * div_y, one centroid (float sum / count) per
 * occupied voxel, leaves in ascending voxel index.  PCL leaves the order in which a voxel's points
 * are added unspecified (std::sort); here it is the point index, so results are reproducible.
 * out_xyz receives min(*n_out, cap) leaves; *n_out their full number.  Host pointers, synchronous;
 * the _device form takes n x 3 / cap x 3 device arrays and synchronises `stream` for the count. */
int pgp_voxel_grid(pgp_ctx* ctx, const float* xyz, int n, float leaf, float* out_xyz, int cap, int* n_out);
int pgp_voxel_grid_device(pgp_ctx* ctx, const float* d_xyz, int n, float leaf, float* d_out_xyz, int cap,
                          int* n_out, void* stream);

/* Replaces pcl::MovingLeastSquares<PointXYZRGB, PointXYZRGBNormal> as PPE/segmentation/Segmentation.cpp:
 * 239-246 configures it: setComputeNormals(true), setPolynomialFit(true) (order 2), setSearchRadius(radius =
 * 0.02), kd-tree radius search, no upsampling -- the step that gives the (voxel-gridded) segment its normals.
 * PCL is not vendored: PCL 1.7's published computeMLSPointNormal, in double where PCL uses double
 * (csrc/mls.hip lists the steps).  A point with fewer than 3 neighbours inside the radius (itself included)
 * is dropped, as performProcessing does; with fewer than 6 it keeps the plane's projection and normal.
 * Outputs, in input order, min(*n_out, cap) rows: out_xyz the smoothed positions, out_nrm (nullable) the
 * normals -- NOT re-normalised and not oriented, as PCL 1.7 leaves them (the node normalises and flips them
 * towards the camera afterwards, ObjectPoseCandidateSet.cpp:39-51 = pgp_radius_outlier_filter) --,
 * out_curvature (nullable) = |lambda_min / trace|, out_index (nullable) the input index of each row.
 * Host pointers, synchronous; the _device form takes device arrays and synchronises `stream` for the count. */
int pgp_mls_normals(pgp_ctx* ctx, const float* xyz, int n, float radius, float* out_xyz, float* out_nrm,
                    float* out_curvature, int* out_index, int cap, int* n_out);
int pgp_mls_normals_device(pgp_ctx* ctx, const float* d_xyz, int n, float radius, float* d_out_xyz, float* d_out_nrm,
                           float* d_out_curvature, int* d_out_index, int cap, int* n_out, void* stream);

/* Replaces Match4PCSBase::c_dist_pose and c_dist_pose_mean (S4/algorithms/match4pcsBase.cc:1616-1655)
 * for m pairs of poses: hull_xyz[n_hull][3] = hull_Q_3D (<= 4096 points), T[n_poses][16] =
 * allTransforms (column-major), pairs[m][2] = (index_1, index_2).  dist_max[m] = the directed
 * Hausdorff distance max_i min_j |T1 h_i - T2 h_j|; dist_sum[m] (nullable) = sum_i min_j (what the
 * reference calls the mean distance), added in hull order.  Host pointers, synchronous. */
int pgp_pose_hausdorff(pgp_ctx* ctx, const float* hull_xyz, int n_hull, const float* T, int n_poses,
                       const int* pairs, int m, float* dist_max, float* dist_sum);

/* pgp_backproject_depth with DEVICE pointers: d_image (rows x cols, u16 or f32), d_mask (nullable),
 * d_xyz_out (cap x 3).  *n_out (host) = full count; `stream` is synchronised for it. */
int pgp_backproject_depth_device(pgp_ctx* ctx, const void* d_image, int raw16, const unsigned char* d_mask,
                                 int rows, int cols, const float K[9], double z_min, double z_max,
                                 float* d_xyz_out, int cap, int* n_out, void* stream);

/* Depth image -> camera-frame cloud in front of the segment (PPE/misc/utilities.cpp:47-61 decode,
 * PPE/segmentation/Segmentation.cpp:219 mask, utilities.cpp:190-206 / 210-231 back-projection).
 * image: rows x cols, either the raw 16-bit PNG samples (raw16 != 0: rotated right by 3 and divided
 * by 10000 as the reference does) or depth in metres as float (raw16 == 0); mask (nullable, rows x
 * cols bytes): a pixel with mask == 0 is dropped; K: 3x3 row-major intrinsics.  Pixels with
 * z_min < depth < z_max (0.1, 2.0 in the reference) are emitted IN ROW-MAJOR ORDER as
 * x = (v - cx) * depth / fx, y = (u - cy) * depth / fy, z = depth, float operations in that order:
 * the reference's list, bit for bit.  xyz_out receives min(*n_out, cap) points; *n_out the full
 * count.  Host pointers, synchronous. */
int pgp_backproject_depth(pgp_ctx* ctx, const void* image, int raw16, const unsigned char* mask, int rows,
                          int cols, const float K[9], double z_min, double z_max, float* xyz_out, int cap,
                          int* n_out);

/* ---- The segment front end on device arrays: radius filter, centring, weights, and the chain as one call ----
 * pgp_radius_outlier_filter with DEVICE pointers, and with what the host form leaves to its caller done on the
 * device too: the same rule (k = points with squared distance STRICTLY below radius^2, the point itself included;
 * kept iff k > min_neighbors), then ONE ordered compaction.  min(*n_kept, cap) rows are written IN INPUT ORDER:
 * d_out_xyz the position, d_out_index (nullable) the input index, d_out_nrm (nullable; written when d_nrm is given
 * too) the normal flipped towards (0,0,0) when (0 - p).n < 0 and divided by its magnitude, float operations in the
 * host form's order -- a zero normal gives NaN, as there.  *n_kept (host) = the full count; `stream` is synchronised
 * for it.  As the host form, it builds the index of d_xyz with delta = radius in the context: the RESIDENT SCENE IS
 * REPLACED by it, so call it before pgp_set_scene / pgp_set_scene_device.  Outputs that overlap the inputs or each
 * other, and radius <= 0, are PGP_EINVAL; n == 0 is PGP_OK with *n_kept = 0. */
int pgp_radius_outlier_filter_device(pgp_ctx* ctx, const float* d_xyz, const float* d_nrm, int n, float radius,
                                     int min_neighbors, float* d_out_xyz, float* d_out_nrm, int* d_out_index, int cap,
                                     int* n_kept, void* stream);

/* pgp_center for ONE cloud of n x 3 device floats, in place: centroid += pos in index order in float, / (float)n,
 * every point minus the centroid (base.cc:242-264) -- the same bits as pgp_center.  The sum is sequential (one lane
 * adds; a tree sum gives other bits), so the call costs time proportional to n.  centroid[3] (host) receives the
 * centroid; `stream` is synchronised for it.  n == 0 is PGP_EINVAL (the host helper divides by zero there).
 * pgp_shift_device subtracts a vector the caller has (the models are centred on centroid_Q) the same way; it is
 * enqueued and not synchronised. */
int pgp_center_device(pgp_ctx* ctx, float* d_xyz, int n, float centroid[3], void* stream);
int pgp_shift_device(pgp_ctx* ctx, float* d_xyz, int n, const float shift[3], void* stream);

/* pgp_weights_from_image with DEVICE pointers (d_xyz_centred: n x 3, d_img: rows x cols u16, d_weights: n): the same
 * arithmetic per point, the same bits; a point outside the image gets weight 0.  Enqueued on `stream`, not
 * synchronised. */
int pgp_weights_from_image_device(pgp_ctx* ctx, const float* d_xyz_centred, int n, const float centroid_P[3],
                                  const float K[9], const unsigned short* d_img, int rows, int cols, float* d_weights,
                                  void* stream);

/* Depth image -> scene in one call, every intermediate in a workspace of the context (it grows on demand):
 * pgp_backproject_depth_device -> pgp_voxel_grid_device -> pgp_mls_normals_device -> pgp_radius_outlier_filter_device
 * -> pgp_center_device -> pgp_weights_from_image_device -> pgp_set_scene_device with normals and weights; the result
 * is what those calls give one after the other.  d_prob (nullable): the probability image, rows x cols u16; without
 * it every weight is 1.  counts[4] = points back-projected, voxel leaves, MLS rows, rows the filter kept.  When the
 * filter keeps at most min_points rows the node bails out (ObjectPoseCandidateSet.cpp:34-37): *installed = 0, PGP_OK,
 * and the context has NO scene (scoring returns PGP_ESTATE).  Otherwise *installed = 1, centroid_P the centroid the
 * scene was centred on, and the scene is the centred, oriented, weighted segment: pgp_score_lcp in
 * PGP_MODE_WEIGHTED works on it at once.  `stream` is synchronised once per stage count. */
typedef struct pgp_segment_options {
  double z_min, z_max;     /* 0.1, 2.0 */
  float voxel_leaf;        /* 0.01 */
  float mls_radius;        /* 0.02 */
  float filter_radius;     /* 0.03 */
  int   min_neighbors;     /* 10 */
  int   min_points;        /* 30: at most this many kept -> no scene, as the node bails */
  float delta;             /* 0.005 */
} pgp_segment_options;
int pgp_segment_default_options(pgp_segment_options* opt);
int pgp_segment_from_depth_device(pgp_ctx* ctx, const pgp_segment_options* opt, const void* d_image, int raw16,
                                  const unsigned char* d_mask, int rows, int cols, const float K[9],
                                  const unsigned short* d_prob /*nullable: weights 1*/,
                                  int counts[4] /* back-projected, voxels, MLS rows, kept */, int* installed,
                                  float centroid_P[3], void* stream);

/* ---- Table-plane removal (SceneCfg::removeTable / getTableParams, PPE/data_layer/SceneCfg.cpp:38-157) ----
 * Replaces pcl::SACSegmentation with SACMODEL_PLANE, SAC_MSAC, setDistanceThreshold(0.005),
 * setMaxIterations(1000), setOptimizeCoefficients(true), and the loop that zeroes the depth pixels near the
 * plane.  PCL is not vendored and its sampler is seeded from the clock, so PCL's bits are NOT pinned; what is
 * implemented, step by step (csrc/plane.hip):
 *   candidates  the n_samples triples given (their order is the candidate order), or max_iterations + 1 drawn
 *               slots (PCL's loop counts an iteration before it tests iterations > max_iterations, so it
 *               evaluates up to max_iterations + 1 models).  Slot i draws three point indices as
 *               variate % n from the counter-based splitmix64 stream keyed by (seed, i) -- attempt a uses
 *               variates 3a, 3a + 1, 3a + 2 --; a draw with a repeated index or an exactly zero cross product
 *               is redrawn, up to 64 attempts, after which the slot is invalid.  A given triple with a zero
 *               cross product is an invalid slot.  Invalid slots are skipped and never counted.
 *   coefficients  in float, in this order: n = (p1 - p0) x (p2 - p0); |n| = sqrt((nx^2 + ny^2) + nz^2)
 *               (correctly rounded); (a, b, c) = n / |n|; d = -((a x0 + b y0) + c z0).
 *   scoring     dist = |((a x + b y) + c z) + d| in float; MSAC penalty = sum of min(dist, threshold) in
 *               DOUBLE (PCL's published rule: the truncated distance, not its square); inliers = dist <= threshold.
 *   stop        PGP_PLANE_STOP_ADAPTIVE: PCL's sequential rule over the valid candidates in order -- a candidate
 *               whose penalty is strictly below the best so far is a record; at a record
 *               k = log(1 - probability) / log(clamp(1 - w^3, eps, 1 - eps)), w = inliers / n (double); the loop
 *               ends after the e-th evaluated candidate when e >= k or e > max_iterations; the last record wins.
 *               PGP_PLANE_STOP_ALL: the minimum penalty over every valid candidate, the lowest index on ties.
 *   refit       (optimize != 0, setOptimizeCoefficients(true)): the points with dist < threshold (strict, as
 *               PCL's selectWithinDistance) of the chosen sample; their centroid and the covariance about it,
 *               double, fixed-order sums; normal = eigenvector of the smallest eigenvalue (pcl::eigen33, sign as it
 *               comes), d = -n . centroid, rounded to float.  Fewer than 3 such points keep the sampled plane.
 *   inliers     the final plane's points with dist < threshold (strict, selectWithinDistance): inliers[n] = 1/0.
 * Every sum has a fixed order (no float atomics): the same call gives the same bits on every run.
 * When every slot is invalid (collinear input, say) the call succeeds with all-zero coefficients and 0 inliers,
 * as PCL returns an empty model.  n < 3, a non-finite coordinate, threshold <= 0, probability outside (0, 1),
 * max_iterations < 1 (or above 65535 candidates), an unknown stop rule or a sample index outside [0, n) are
 * PGP_EINVAL. */
enum { PGP_PLANE_STOP_ADAPTIVE = 0, PGP_PLANE_STOP_ALL = 1 };

typedef struct {
  float threshold;            /* 0.005 (SceneCfg.cpp:61, :116) */
  int max_iterations;         /* 1000 */
  double probability;         /* 0.99, PCL's default */
  int stop;                   /* PGP_PLANE_STOP_ADAPTIVE (default) | PGP_PLANE_STOP_ALL */
  int optimize;               /* 1 = refit on the inliers + re-selection */
  unsigned long long seed;    /* keys the drawn candidates (unused with explicit samples) */
} pgp_plane_options;
int pgp_plane_default_options(pgp_plane_options* opt);

typedef struct {
  int status;                 /* PGP_OK, or PGP_EINVAL when the device form met a non-finite point or a bad sample index
                                 (the result is then empty: zero coefficients, 0 inliers) */
  int chosen;                 /* candidate index of the winning sample; -1 when no slot is valid */
  int n_evaluated;            /* valid candidates the stop rule evaluated */
  int n_valid;                /* valid candidates in the list */
  int n_candidates;           /* slots in the list: n_samples, or max_iterations + 1 */
  int sampled_inliers;        /* the chosen sample's dist <= threshold count (the w of the stop rule) */
  double penalty;             /* the chosen sample's MSAC penalty */
  float sampled[4];           /* the chosen sample's coefficients, before the refit */
} pgp_plane_info;

/* The plane fit.  xyz: n x 3; samples (nullable): n_samples x 3 point indices replacing the draw; coeff[4] =
 * (a, b, c, d) of a x + b y + c z + d = 0; inliers (nullable): n bytes; *n_inliers their number; info
 * (nullable).  Host pointers, synchronous. */
int pgp_fit_plane(pgp_ctx* ctx, const float* xyz, int n, const pgp_plane_options* opt, const int* samples, int n_samples,
                  float coeff[4], unsigned char* inliers, int* n_inliers, pgp_plane_info* info);
/* The same with DEVICE arrays, results written to device memory (d_coeff: 4 floats, d_inliers: n bytes or NULL,
 * d_n_inliers: 1 int, d_info: one pgp_plane_info or NULL).  Enqueued on `stream` with no host synchronisation, so it
 * chains behind pgp_voxel_grid_device; the workspace is sized once and kept in the context.  Finiteness and the sample
 * indices are checked on the device (d_info->status). */
int pgp_fit_plane_device(pgp_ctx* ctx, const float* d_xyz, int n, const pgp_plane_options* opt, const int* d_samples,
                         int n_samples, float* d_coeff, unsigned char* d_inliers, int* d_n_inliers,
                         pgp_plane_info* d_info, void* stream);

/* The depth mask of SceneCfg::removeTable (SceneCfg.cpp:69-80), bit for bit: per pixel (u, v),
 * x = (float)((v - cx) * depth / fx), y = (float)((u - cy) * depth / fy), z = depth (float operations);
 * dist = |((a x + b y) + c z) + d| in DOUBLE from the float coefficients (pcl::pointToPlaneDistance);
 * the pixel becomes 0 when dist < threshold (strict; 0.005 there).  image (in-out): rows x cols, float metres
 * (raw16 == 0) or the raw 16-bit encoding pgp_backproject_depth reads (raw16 != 0; a masked pixel becomes raw
 * 0); K: 3x3 row-major; *n_masked (nullable) = pixels zeroed.  Host pointers, synchronous; the _device form
 * takes a device image, writes the count to d_n_masked (nullable) and does not synchronise `stream`. */
int pgp_mask_plane_depth(pgp_ctx* ctx, void* image, int raw16, int rows, int cols, const float K[9],
                         const float coeff[4], double threshold, int* n_masked);
int pgp_mask_plane_depth_device(pgp_ctx* ctx, void* d_image, int raw16, int rows, int cols, const float K[9],
                                const float coeff[4], double threshold, int* d_n_masked, void* stream);

/* SceneCfg::removeTable in one call: back-projection (0.1 < z < 2.0, as convert3dOrganizedRGB), the voxel grid
 * (leaf; 0.005 there), pgp_fit_plane_device and the depth mask, all on the device: the image goes up once and
 * comes back once, no cloud leaves the device.  The mask threshold is opt->threshold read as the double of its
 * shortest decimal form (0.005f -> 0.005, the reference's literal).  coeff[4] (nullable) receives the plane,
 * *n_masked (nullable) the pixels zeroed.  One deviation: the reference's organised cloud keeps out-of-range
 * pixels as (0, 0, 0) points, which puts one voxel at the camera origin into the fit; they are dropped here. */
int pgp_remove_table(pgp_ctx* ctx, void* image, int raw16, int rows, int cols, const float K[9], float leaf,
                     const pgp_plane_options* opt, float coeff[4], int* n_masked);

/* ---- Object proposals: connected components of a depth image (csrc/components.hip) ----
 * What stands on the table once pgp_remove_table has zeroed it: Euclidean clustering on the organised image, i.e.
 * connected-component labelling with a 3-D distance test between neighbouring pixels (PCL's
 * OrganizedConnectedComponentSegmentation + EuclideanClusterComparator).  The reference has no such step -- its masks
 * come from a CNN or a ground-truth file (Segmentation.cpp) -- so nothing of its bits is pinned; the rules, all of them:
 *   validity   pixel (u, v) is valid iff (mask == NULL or mask[u, v] != 0) and z_min < depth < z_max (both strict, NaN
 *              invalid): pgp_backproject_depth's rule, decode (raw16) and point: x = (v - cx) * depth / fx,
 *              y = (u - cy) * depth / fy, z = depth, float operations in that order.
 *   edges      connectivity 4: the right and the down neighbour; 8: both diagonals as well.  Two neighbouring valid
 *              pixels are connected iff ((dx dx + dy dy) + dz dz) <= tolerance * tolerance, every product and sum
 *              rounded to float on its own, the comparison inclusive.
 *   labels     roots[u cols + v] = the smallest row-major pixel index of the pixel's component, -1 for an invalid
 *              pixel: independent of scheduling.
 *   table      per component: pixel count, inclusive bounding box (rows u, columns v), depth range, and per coordinate
 *              the sum over its pixels of llrint((double)coord * 1e6) -- integers, so the same bits on every run;
 *              centroid = sum_um / pixels / 1e6.  (-0 counts as below +0 in the depth range.)
 *   selection  kept iff pixels >= min_pixels and (max_pixels <= 0 or pixels <= max_pixels); the kept ones ranked by
 *              descending pixels, ties by ascending root; the first min(kept, cap) get ids 1, 2, ... and info rows
 *              0, 1, ... in that order (further rows of info are not written).  ids[u cols + v] = the id of the
 *              pixel's component, 0 for invalid pixels, unkept components and kept ones beyond cap.
 *   counts     [0] kept components (the full number, it may exceed cap), [1] components of any size, [2] valid pixels.
 * Touching objects are one component: that is the method's limit, not an error (pgp_depth_objects below cuts them
 * along the concave crease between them).
 * tolerance <= 0 or not finite, a connectivity other than 4 or 8, min_pixels < 1, cap < 0, cap > 0 without info,
 * rows * cols > 2^30 and outputs that overlap the inputs or each other are PGP_EINVAL; rows == 0 or cols == 0 is PGP_OK
 * with zero counts. */
typedef struct pgp_components_options {
  double z_min, z_max;   /* 0.1, 2.0 */
  float  tolerance;      /* 0.01 m */
  int    connectivity;   /* 4 (default) or 8 */
  int    min_pixels;     /* 500: ours, the reference has no such step */
  int    max_pixels;     /* 0 = no upper bound */
} pgp_components_options;
int pgp_components_default_options(pgp_components_options* opt);

typedef struct pgp_component_info {
  int root;            /* canonical label: smallest row-major pixel index */
  int pixels;
  int u_min, u_max, v_min, v_max;      /* bounding box, rows u, columns v, inclusive */
  float z_min, z_max;                  /* depth range */
  long long sum_um[3];                 /* sum over the pixels of llrint((double)coord * 1e6), coord = x, y, z:
                                          centroid = sum_um / pixels / 1e6, the same bits on every run */
} pgp_component_info;

/* image: rows x cols, float metres (raw16 == 0) or the raw 16-bit encoding (raw16 != 0); mask (nullable): rows x cols
 * bytes; K: 3x3 row-major; roots, ids (nullable): rows x cols ints; info (nullable when cap == 0): cap rows; counts[3].
 * Host pointers, synchronous. */
int pgp_depth_components(pgp_ctx* ctx, const pgp_components_options* opt, const void* image, int raw16,
                         const unsigned char* mask, int rows, int cols, const float K[9], int* roots, int* ids,
                         pgp_component_info* info, int cap, int counts[3]);
/* The same on DEVICE arrays, results in device memory (d_counts: 3 ints).  Enqueued on `stream` with no host
 * synchronisation and sized by bounds (rows * cols), not by counts read home, so it chains behind
 * pgp_mask_plane_depth_device; the workspace lives in the context and grows on demand. */
int pgp_depth_components_device(pgp_ctx* ctx, const pgp_components_options* opt, const void* d_image, int raw16,
                                const unsigned char* d_mask, int rows, int cols, const float K[9], int* d_roots,
                                int* d_ids, pgp_component_info* d_info, int cap, int* d_counts, void* stream);

/* mask[u, v] = (ids[u, v] == id) as 1 / 0: the byte mask pgp_segment_from_depth_device and
 * pgp_backproject_depth_device read.  Host pointers, synchronous; the _device form is enqueued and not synchronised. */
int pgp_component_mask(pgp_ctx* ctx, const int* ids, int rows, int cols, int id, unsigned char* mask);
int pgp_component_mask_device(pgp_ctx* ctx, const int* d_ids, int rows, int cols, int id, unsigned char* d_mask,
                              void* stream);

/* Which component does each object's 2-D mask fall into, and which objects can share a search tree
 * (MCTSSelection::selectBestPoses builds `independentTrees` and then puts every object into one,
 * HypothesisSelection.cpp:242-247): objects whose pixels lie in different components cannot touch.
 * classes: the reference's class image (GTSegmentation, Segmentation.cpp:187-206; FCNSegmentation, :118-129), rows x cols
 * of class_bytes = 1 (uchar) or 2 (ushort) bytes; object o is the pixels with classes == class_values[o]; ids: what
 * pgp_depth_components wrote, values in [0, min(rows * cols, 65535)] (an id names a component of at least one pixel;
 * anything else is PGP_EINVAL).  Per object:
 *   pixels_total[o]  pixels of its class with ids != 0
 *   component[o]     the id that holds most of them, the lower id on ties; 0 when pixels_total[o] == 0
 *   pixels_in[o]     that count
 *   group[o]         objects with the same non-zero component share a group, an object with component 0 is a group of
 *                    its own; groups are numbered from 0 in the order of their first object.
 * The votes are an n_objects x (ids' bound + 1) integer histogram filled with integer atomics.  n_objects outside 1..64
 * and class_bytes other than 1 or 2 are PGP_EINVAL; an empty image gives all-zero counts and one group per object.  Host
 * pointers, synchronous; the _device form takes device images, writes HOST result arrays and synchronises `stream` once. */
int pgp_assign_masks_to_components(pgp_ctx* ctx, const int* ids, const void* classes, int class_bytes, int rows, int cols,
                                   const int* class_values, int n_objects, int* component, int* pixels_in,
                                   int* pixels_total, int* group);
int pgp_assign_masks_to_components_device(pgp_ctx* ctx, const int* d_ids, const void* d_classes, int class_bytes, int rows,
                                          int cols, const int* class_values, int n_objects, int* component,
                                          int* pixels_in, int* pixels_total, int* group, void* stream);

/* ---- Touching objects: the concave-crease cut (csrc/depth_crease.hip) ----
 * Where two objects touch, the depth image has no jump, but the surface has a concave crease; one rigid, roughly convex
 * object shows convex edges.  This is the local-convexity criterion of LCCP (Stein et al. 2014) on the pixel grid, as the
 * edge maps of Tateno et al. 2015: surface normals of the organised image, a concavity test between pixels a few steps
 * apart, pgp_depth_components on what is left (the cores), and a few passes that hand the crease pixels back.  The
 * reference has no such step, so nothing of its bits is pinned; the rules, all of them:
 *   points     pixels, validity (the caller's mask included), z_min / z_max and tolerance are pgp_depth_components',
 *              taken from a pgp_components_options.
 *   floats     every float operation is rounded on its own; a three-term sum is (a + b) + c; divide and square root
 *              are IEEE.  dist2(p, q) = ((dx dx + dy dy) + dz dz).
 *   reach      the pixel q at offset (du, dv) is reachable from p iff both are valid, k = max(|du|, |dv|) >= 1 and
 *              dist2(p, q) <= t * t with t = tolerance * (float)k (float products).
 *   raw normal (s = normal_step) the horizontal tangent h is p(u, v + s) - p(u, v - s) when both are reachable,
 *              p(u, v + s) - p when only the first is, p - p(u, v - s) when only the second is; with neither the pixel
 *              has no normal.  The vertical tangent g likewise from p(u +- s, v).  m = g x h (it points towards the
 *              camera), z = (mx mx + my my) + mz mz; the normal is m / sqrt(z) when z > 0, else there is none.
 *   smoothed   (w = smooth_radius) only for a pixel with a raw normal: acc = (+0, +0, +0); for du = -w .. w (outer) and
 *              dv = -w .. w (inner) the raw normal of (u + du, v + dv) is added component-wise when (du, dv) == (0, 0)
 *              or that pixel is reachable and has a raw normal; normalised as above, a zero sum is no normal.
 *   crease     (c = crease_step) for a pixel i with a smoothed normal n_i and each of the eight pixels j at (+-c, 0),
 *              (0, +-c), (+-c, +-c) that is reachable and has a smoothed normal: the pair is concave iff
 *              (n_j - n_i) . (p_j - p_i) < 0, and a concave pair's penalty is 1 - n_i . n_j (dots as three-term sums),
 *              any other pair's 0.  i is a crease pixel iff its largest penalty > concavity (strict).
 *   cores      pgp_depth_components with mask = (caller's mask) AND (not crease): roots is that labelling (-1 on crease
 *              and invalid pixels); selection, ranking and the ids 1 .. min(kept, cap) are decided on the cores.
 *   growing    grow_passes Jacobi passes, each reading the ids of the one before: a valid pixel with id 0 (a crease
 *              pixel, or one of an unkept core or of one beyond cap) takes the smallest non-zero id among its four
 *              neighbours that are reachable (k = 1), or stays 0.
 *   table      the info rows keep the cores' order and root; pixels, bounding box, depth range and sum_um describe the
 *              grown ids, folded in integers as in pgp_depth_components.
 *   counts     [0] kept cores, [1] cores of any size, [2] valid pixels, [3] crease pixels, [4] pixels labelled by growing.
 * Limits: a convex contact -- two boxes flush side by side with coplanar tops -- has no concave crease and is not cut;
 * a strongly concave single object (the inside of a mug, a bowl) is cut.
 * Refused (PGP_EINVAL): whatever pgp_depth_components refuses, normal_step or crease_step outside 1..8, smooth_radius
 * outside 0..4, grow_passes outside 0..64, concavity negative or not finite.  rows == 0 or cols == 0 is PGP_OK with zero
 * counts. */
typedef struct pgp_crease_options {
  int   normal_step;     /* 3: pixels between a pixel and the two its tangent is taken from */
  int   smooth_radius;   /* 2: the normals are summed over (2 w + 1)^2 pixels */
  int   crease_step;     /* 4: pixels between the two ends of a tested pair */
  float concavity;       /* 0.06: a concave pair with 1 - n_i . n_j above this is a crease (about 20 degrees) */
  int   grow_passes;     /* 12 */
} pgp_crease_options;
int pgp_crease_default_options(pgp_crease_options* opt);

/* The smoothed normals: normals[(u cols + v) 4 ..] = (nx, ny, nz, 1) for a pixel that has one, (0, 0, 0, 0) for any
 * other.  image, mask, K as in pgp_depth_components.  Host pointers, synchronous; the _device forms of all three calls
 * take DEVICE arrays, are enqueued on `stream` with no host synchronisation and are sized by rows * cols, so they chain
 * behind pgp_mask_plane_depth_device; the workspace lives in the context and grows on demand. */
int pgp_depth_normals(pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* crease, const void* image,
                      int raw16, const unsigned char* mask, int rows, int cols, const float K[9], float* normals);
int pgp_depth_normals_device(pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* crease,
                             const void* d_image, int raw16, const unsigned char* d_mask, int rows, int cols,
                             const float K[9], float* d_normals, void* stream);

/* keep[u cols + v] = 1 for a pixel that is valid (the caller's mask included) and not a crease pixel, else 0: the byte
 * mask pgp_depth_components and pgp_segment_from_depth_device read.  *n_crease = the crease pixels. */
int pgp_depth_crease_mask(pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* crease,
                          const void* image, int raw16, const unsigned char* mask, int rows, int cols, const float K[9],
                          unsigned char* keep, int* n_crease);
int pgp_depth_crease_mask_device(pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* crease,
                                 const void* d_image, int raw16, const unsigned char* d_mask, int rows, int cols,
                                 const float K[9], unsigned char* d_keep, int* d_n_crease, void* stream);

/* The whole chain.  roots, ids (nullable), info (nullable when cap == 0) as in pgp_depth_components; counts[5].  The
 * device form always runs all grow_passes passes: nothing is read home in between. */
int pgp_depth_objects(pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* crease, const void* image,
                      int raw16, const unsigned char* mask, int rows, int cols, const float K[9], int* roots, int* ids,
                      pgp_component_info* info, int cap, int counts[5]);
int pgp_depth_objects_device(pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* crease,
                             const void* d_image, int raw16, const unsigned char* d_mask, int rows, int cols,
                             const float K[9], int* d_roots, int* d_ids, pgp_component_info* d_info, int cap,
                             int* d_counts, void* stream);

/* Replaces UCTState::computeCost (PPE/hypothesis_verification/mcts/UCTState.cpp:93-116) for n
 * rendered depth images against one observed image (all rows x cols float, row-major, metres):
 * render_score[i] = obScore + renScore - intScore with the pixel tests of the reference and
 * threshold = explanationThreshold (0.01 there, UCTState.cpp:8).  counts (nullable) receives the
 * three integer tallies per image.  Host pointers, synchronous.  At most 65535 images per call (this
 * form and the device form): more is PGP_EINVAL, nothing is launched. */
int pgp_depth_cost(pgp_ctx* ctx, const float* observed, const float* rendered, int n, int rows, int cols,
                   float threshold, float* render_score, int* counts);

/* Device-pointer form of pgp_depth_cost: d_observed (rows x cols) and d_rendered (n x rows x cols) are
 * float images in HBM, d_counts (n x 3 ints, {obScore, renScore, intScore}) and d_scores (nullable, n
 * floats = renderScore) are written there too; enqueued on `stream`, no synchronisation, no allocation. */
int pgp_depth_cost_device(pgp_ctx* ctx, const float* d_observed, const float* d_rendered, int n, int rows, int cols,
                          float threshold, int* d_counts, float* d_scores, void* stream);

/* Depth images of a posed object for a batch of MCTS leaf states, rendered in HBM.  Replaces the OpenGL
 * pass behind UCTState::render (PPE/hypothesis_verification/mcts/UCTState.cpp:44-72 ->
 * src/3rdparty/depth_sim/src/renderScene.cpp:45-72): the object is drawn under each of the n poses with
 * the camera's intrinsics, fragments beyond z_max are dropped (renderScene.cpp:69: 1 m), and every
 * image starts from the parent state's image, the nearer surface winning (UCTState.cpp:62-68).
 *   vertices: n_vert x vertex_stride floats (stride 3 or 4), object frame
 *   triangles: n_tri x 3 vertex indices, or NULL = every vertex is splatted into its nearest pixel
 *   T: n x 16 column-major float, object -> camera frame (convertToWorld/convertToCamera done by the caller)
 *   parent (nullable): parent_stride == 0: ONE rows x cols image under all n; else image i at parent + i * parent_stride
 *   depth: n x rows x cols floats, metres, 0 = no surface
 *   n: at most 65535 images per call, vertex_stride 3 or 4, rows * cols at most 2^28: else PGP_EINVAL
 * The rasterisation rules (pixel centres, inclusive edges, perspective-correct depth, near-plane clipping,
 * atomic-min z-buffer) are stated in csrc/render.hip; OpenGL's are implementation-defined, so parity with
 * the reference's renderer is unpinned.  oracle/render_oracle.py restates the rules in numpy float32, bit
 * for bit, and tests/_render_raycast.py checks that restatement against a float64 ray caster. */
typedef struct {
  int rows, cols;
  float fx, fy, cx, cy;
  float z_near;   /* points at z <= z_near are dropped (<= 0: 0); a triangle with one or two vertices there is
                     CLIPPED against z = z_near (1e-4 when z_near is 0), with all three it is dropped */
  float z_max;    /* fragments with z > z_max are dropped (<= 0: no limit); the reference uses 1.0 */
} pgp_camera;
int pgp_render_depth_device(pgp_ctx* ctx, const float* d_vertices, int vertex_stride, int n_vert, const int* d_triangles,
                            int n_tri, const float* d_T, int n, const pgp_camera* cam, const float* d_parent,
                            size_t parent_stride, float* d_depth, void* stream);
/* Host pointers, synchronous (tests, small callers): parent is ONE image or NULL. */
int pgp_render_depth(pgp_ctx* ctx, const float* vertices, int n_vert, const int* triangles, int n_tri, const float* T,
                     int n, const pgp_camera* cam, const float* parent, float* depth);

/* Replaces HypothesisSelection::greedyClustering (PPE/hypothesis_verification/HypothesisSelection.cpp:
 * 66-115) and its pose distance utilities::getPoseError (PPE/misc/utilities.cpp:514-548) for one
 * object's scored hypothesis list.  T: n_h x 16 col-major float (the Matrix4f images convertToMatrix
 * yields, utilities.cpp:276-280), scores: n_h (allPose[i].second), best_score = bestHypothesis.second,
 * sym_deg = the object's symInfo (per axis 0 / 90 / 180 / 360, PPE/data_layer/Objects.hpp:22).
 * params NULL = the reference's constants {0.5, 10, 0.02} (:70,:99).  Hypotheses with
 * score > accept_fraction * best_score are visited in descending score order (equal scores in
 * index order; the reference's std::sort leaves ties unspecified) and kept unless an earlier kept
 * one is within both thresholds.  rep_index (cap entries) receives the kept hypothesis ids in
 * that order = clusteredHypothesisSet; *n_rep their number (may exceed cap: the list is then
 * truncated); assignment (nullable, n_h) the id of the representative that absorbed each
 * hypothesis (itself for a representative, -1 when pruned).  The `+=` at :102 acts on a copy in
 * the reference, so cluster scores are the representatives' own scores[rep_index[k]].
 * Host pointers, synchronous. */
typedef struct pgp_cluster_params {
  float accept_fraction; /* 0.5  */
  float rot_thresh_deg;  /* 10   */
  float trans_thresh;    /* 0.02 */
} pgp_cluster_params;
int pgp_cluster_poses(pgp_ctx* ctx, const float* T, const float* scores, int n_h, float best_score,
                      const float sym_deg[3], const pgp_cluster_params* params, int* rep_index, int cap,
                      int* n_rep, int* assignment);
/* pgp_cluster_poses with DEVICE pointers (d_T n_h x 16, d_scores n_h, d_rep_index n_h ints,
 * d_assignment n_h ints): *n_rep (host) = number of representatives; `stream` is synchronised. */
int pgp_cluster_poses_device(pgp_ctx* ctx, const float* d_T, const float* d_scores, int n_h, float best_score,
                             const float sym_deg[3], const pgp_cluster_params* params, int* d_rep_index,
                             int* d_assignment, int* n_rep, void* stream);
/* The pose distance alone, for n pairs (test[i], gt[i]) of 4x4 col-major transforms. */
int pgp_pose_error(pgp_ctx* ctx, const float* test, const float* gt, int n, const float sym_deg[3],
                   float* rot_err_deg, float* trans_err);

/* ---- PPF Hough voting: the hypotheses of the node's PPF_HOUGH mode ---------------------------------------------
 * SceneCfg::generateHypothesis with hypoGenMode "PPF_HOUGH" (PPE/data_layer/SceneCfg.cpp:376-402) builds a
 * pose_candidates::PPFVoting whose generate (PPE/hypothesis_generation/ObjectPoseCandidateSet.cpp:76-117) filters and
 * orients the segment and then leaves the estimator commented out.  The reference has no estimator to match: the
 * algorithm below is this library's statement of point-pair-feature voting (Drost et al., CVPR 2010), its rules
 * stated exactly (csrc/ppf_vote.hip) and restated in numpy by tests/_ppf_restate.py.
 *   table      the one of pgp_set_ppf_map, WITH its pair lists: a pair (a, b) of key k has computePPF(a, b) = k, ids
 *              into the PPF model; the scene pair (s_r, s_j) is keyed by the same device function (u = s_r - s_j,
 *              the host-libm angle thresholds, 5 mm distance bins), so m_r = a corresponds to s_r
 *   T_g(p, n)  the rigid map x -> R_g (x - p) with n^ = n / |n| and, when 1 + n^x > 1e-6,
 *                R_g = [[n^x, n^y, n^z], [-n^y, 1 - k n^y^2, -k n^y n^z], [-n^z, -k n^y n^z, 1 - k n^z^2]],
 *                k = 1 / (1 + n^x)  (the rotation about n^ x e_x that sends n^ to +x); else diag(-1, -1, 1)
 *   alpha      of a pair (r, i): q = R_g(r) (p_i - p_r), alpha = atan2(-q_z, q_y) in [-pi, pi]
 *   votes      for reference point s_r and every other scene point s_j whose key is in the table, every pair
 *              (m_r, m_i) of the key's list votes +1 into cell m_r * n_bins + bin, bin = floor(d n_bins / 2 pi)
 *              (clamped to n_bins - 1) of d = alpha_m - alpha_s wrapped into [0, 2 pi); 32-bit integer counters,
 *              integer atomics only: the counts do not depend on the order of arrival
 *   peaks      the maximal cell of each reference point (ties: lowest cell), then up to peaks_per_ref - 1 further
 *              cells in descending (votes, then ascending cell) order; a cell is kept while votes >= min_votes,
 *              votes > 0 and (float)votes >= min_vote_fraction * (float)max
 *   pose       T = T_s(s_r)^-1 R_x(alpha) T_m(m_r) with alpha = (bin + 0.5) 2 pi / n_bins, R_x(a) = rotation by a
 *              about +x: model frame -> scene frame, 16 floats column-major
 * Clouds are the centred ones of pgp_center: the scene of pgp_set_scene (with normals) and the PPF model of
 * pgp_set_ppf_model (the node's pclModelSampled minus centroid_Q, what pgp_set_search_model holds), so the poses are
 * in the frame pgp_score_lcp expects.  Hypotheses come out in (reference point, peak rank) order.  Unpinned: float
 * rounding of alpha (its error grows as k = 1 / (1 + n^x) for normals near -x) may move a vote whose angle lies near a
 * bin edge to the neighbouring bin.
 * PGP_ESTATE: no scene with normals, no table, a table without pair lists, or no PPF model; PGP_EINVAL: bad options
 * or a model that does not cover the pair ids of the table.  PGP_PPF_ACC=hbm forces the HBM accumulator path
 * (checker switch: identical results). */
typedef struct {
  int ref_step;             /* reference points are scene points 0, ref_step, 2 ref_step, ...: 5 (>= 1) */
  int n_bins;               /* alpha bins over [0, 2 pi): 30 (1 .. 360) */
  int peaks_per_ref;        /* 1 (1 .. 4) */
  float min_vote_fraction;  /* 0.9 ([0, 1]): of the reference point's maximum, for peaks after the first */
  int min_votes;            /* 3 (>= 1): no hypothesis below this count */
} pgp_ppf_options;
int pgp_ppf_default_options(pgp_ppf_options* opt);

/* The positions and normals the pair ids of the table index (n x 3 each, host pointers; n >= 0).  Computes the model
 * angle alpha_m of every pair of the table once, kept as long as the table and the model stay. */
int pgp_set_ppf_model(pgp_ctx* ctx, const float* xyz, const float* nrm, int n);

/* The hypotheses in HBM: d_T [cap][16], d_votes [cap], d_ref [cap] (scene id of s_r, nullable), d_cell [cap]
 * (m_r * n_bins + bin, nullable), d_n_out: 1 int = the full count (may exceed cap: the list is truncated).  Enqueued on
 * `stream`, no synchronisation; the workspace (peak slots, HBM accumulators) is kept in the context and grows only
 * when a call needs more than an earlier one. */
int pgp_ppf_vote_device(pgp_ctx* ctx, const pgp_ppf_options* opt, float* d_T, int* d_votes, int* d_ref, int* d_cell,
                        int cap, int* d_n_out, void* stream);
/* Host pointers, synchronous (ref / cell nullable); *n_out may exceed cap, as in pgp_cluster_poses. */
int pgp_ppf_vote(pgp_ctx* ctx, const pgp_ppf_options* opt, float* T, int* votes, int* ref, int* cell, int cap,
                 int* n_out);
/* What PPFVoting::generate should return, in one call with one synchronisation: the votes, then every hypothesis
 * scored on the device as pgp_score_lcp(mode, gate_deg) scores it (needs pgp_set_model; the scores equal
 * pgp_score_lcp's on the returned transforms bit for bit).  T [cap][16], scores [cap], votes [cap] (nullable) =
 * hypothesisSet in (reference, peak) order, *n_out the full count; best_index (into the list, -1 when no score is
 * > 0; the rule of pgp_score_lcp), best_score and best_T [16] = bestHypothesis (nullable; best_T is left alone at -1). */
int pgp_ppf_hypotheses(pgp_ctx* ctx, const pgp_ppf_options* opt, int mode, float gate_deg, float* T, float* scores,
                       int* votes, int cap, int* n_out, int* best_index, float* best_score, float* best_T);
/* Debug export for parity tests: the full accumulator of k given reference points (scene ids), acc [k][n_model][n_bins]
 * int32 (n_model = pgp_set_ppf_model's n).  Host pointers, synchronous. */
int pgp_ppf_accumulator(pgp_ctx* ctx, const pgp_ppf_options* opt, const int* ref_ids, int k, int* acc);
/* Debug export: alpha_m of every pair of the table in pair-list order (alpha[n], n = the table's pair count). */
int pgp_ppf_model_angles(pgp_ctx* ctx, float* alpha, long long n);

/* ---- physics settling of MCTS child states: UCTState::correctPhysics --------------------------------------------
 * Replaces UCTState::correctPhysics (PPE/hypothesis_verification/mcts/UCTState.cpp:208-270, called on every expanded
 * child and at every rollout level, UCTSearch.cpp:99,158,226) and the Bullet world of physim::PhySim
 * (PPE/hypothesis_verification/physics_reasoning/PhySim.cpp): every earlier object static (mass 0), the newest one
 * dynamic, the table a static box of half extents (0.40, 0.40, 0.20) at tableParams (SceneCfg.cpp:145-156), gravity
 * (0, 0, -2), simulate(60) = 60 x stepSimulation(1/60), the settled pose back in the camera frame.  Bullet is not
 * matched bit for bit: the device runs the stepping rules stated exactly in csrc/physics.hip (vertex-face contacts,
 * at most 4 per body pair, sequential impulses, first-order quaternion update), restated in numpy float32 by
 * tests/_physics_restate.py.  Only one body moves, so its mass cancels: impulses are per unit mass.
 * Vertex-face contacts alone miss two hulls that meet without a vertex of either inside the other (crossed bars, a
 * yawed box on a box): the dynamic body falls through.  pgp_physics_set_edge_contacts adds edge-edge contacts, off by
 * default (the rule: csrc/physics.hip step 3e, restated by tests/_physics_edges_restate.py).  Its limits: a body
 * thinner than `reach` can pick up an edge pair of its far side; an overlap deeper than `reach` falls back to
 * vertex-face contacts; it is still not GJK/EPA (no face-face clipping, no closest features of separated hulls).
 * pgp_physics_set_polyhedral_contacts replaces both rules by a separating-axis test with face clipping that has no
 * `reach` (step 3p), also off by default.  Its limits: one contact point for an edge-edge contact; no persistent
 * manifold and no warm start; no closest features of separated hulls (hulls farther apart than their margins make no
 * contact); and a cost that grows with the product of the two hulls' edge counts.
 * Shapes live in a per-context arena until pgp_destroy.  Shape 0 is the built-in table box (8 vertices, 6 planes,
 * margin 0); pgp_physics_add_shape hands out 1, 2, ... */
#define PGP_PHYSICS_TABLE_SHAPE 0
#define PGP_PHYSICS_MAX_VERTICES 256   /* hull vertex cap of one shape */
#define PGP_PHYSICS_MAX_STATICS 16     /* static bodies of one state besides the table */
#define PGP_PHYSICS_MAX_CONTACTS 68    /* 4 per body pair: (1 + 16) x 4 */
typedef struct {
  float dt;               /* 1/60 (> 0): stepSimulation(1.f/60.f), PhySim.cpp:112 */
  int steps;              /* 60 (0 .. 100000): simulate(60), UCTState.cpp:247 */
  float gravity[3];       /* (0, 0, -2), world frame: PhySim.cpp:3,16,110 */
  float linear_damping;   /* 0.99 ([0, 1)): setDamping(0.99f, 0.99f), PhySim.cpp:43,73 */
  float angular_damping;  /* 0.99 ([0, 1)) */
  float friction;         /* 1 (>= 0): the product of the two bodies' frictions (1 x 1) */
  int iterations;         /* 10 (1 .. 1000): sequential-impulse sweeps per step (Bullet's default) */
  float erp;              /* 0.2 ([0, 1]): Baumgarte factor beta of the normal rows (Bullet's default) */
} pgp_physics_options;
typedef struct {
  int n_contacts;    /* contacts of the last step (-1: the state was rejected on the device, T_out is NaN) */
  float min_depth;   /* the smallest contact depth of the last step (<= 0 while touching; 0 without contacts) */
  float lin_speed;   /* |v| after the last step */
  float ang_speed;   /* |omega| after the last step */
} pgp_physics_info;
int pgp_physics_default_options(pgp_physics_options* opt);

/* The convex hull of n points (n x 3 floats), pure host helper (no context, like pgp_center).  An incremental hull
 * in double precision with the tolerance eps = 1e-7 x (largest |coordinate|), about float rounding: a point within eps
 * of a face plane is not outside it.  Coplanar triangles (every vertex within eps of the first triangle's plane) merge into one plane.
 * When the hull has more than max_vertices (4 .. 256) vertices, max_vertices of them are kept by farthest-point
 * selection (start: the largest x, ties the lowest input index; then the vertex farthest from the kept set, ties
 * the lowest index) and the hull of the kept points is rebuilt.  hull_xyz (max_vertices x 3) receives the hull
 * vertices in ascending input order, planes (2 max_vertices x 4) the outward unit normal and offset (n . x <= d
 * inside) of each face.  PGP_EINVAL: a NaN / inf, fewer than 4 points, or no 4 points spanning a volume. */
int pgp_convex_hull(const float* xyz, int n, int max_vertices, float* hull_xyz, int* n_vert, float* planes,
                    int* n_planes);
/* Appends the hull of a mesh's vertices (n x 3, body frame: the model frame, its origin the centre of mass) to the
 * context's shape arena: btConvexHullShape + setMargin (PhySim.cpp:53-79).  The unit-mass inertia is Bullet's
 * btPolyhedralConvexShape::calculateLocalInertia: the box inertia I = (ly^2 + lz^2, lx^2 + lz^2, lx^2 + ly^2) / 12
 * of l = hull extent + 6 margin per axis (the cached local AABB carries one margin per side, btTransformAabb adds
 * one, calculateLocalInertia one more).  margin in [0, 0.1]; *shape_id receives the id. */
int pgp_physics_add_shape(pgp_ctx* ctx, const float* xyz, int n, float margin, int max_vertices, int* shape_id);
/* What the device holds for a shape: hull_xyz (256 x 3), planes (512 x 4), inertia[3], margin (each nullable). */
int pgp_physics_shape_info(pgp_ctx* ctx, int shape_id, float* hull_xyz, int* n_vert, float* planes, int* n_planes,
                           float inertia[3], float* margin);
/* The hull edges the device holds for a shape: rows (v0, v1, f0, f1), v0 < v1 two hull vertices, f0 < f1 the two
 * planes that meet there (indices into pgp_physics_shape_info's vertices and planes), ascending by (v0, v1).  An edge
 * between coplanar triangles that merged into one plane is none.  edges ((3 x 256 - 6) x 4 ints) and n_edges are
 * nullable; a hull of V vertices has at most 3 V - 6 edges, the table box 12. */
#define PGP_PHYSICS_MAX_EDGES (3 * PGP_PHYSICS_MAX_VERTICES - 6)
int pgp_physics_shape_edges(pgp_ctx* ctx, int shape_id, int* edges, int* n_edges);
/* Edge-edge contacts in every later settle of this context (pgp_physics_settle, _settle_device, _trace,
 * pgp_mcts_search); a context setting like pgp_set_exact_ties, off by default: while off, the settle kernel is the
 * vertex-face one, bit for bit.  reach (metres, > 0, finite): the largest distance between the closest
 * points of two edges that still makes a contact.  PGP_EINVAL: NULL context or a bad reach (nothing changes). */
#define PGP_PHYSICS_EDGE_REACH_DEFAULT 0.01f
int pgp_physics_set_edge_contacts(pgp_ctx* ctx, int on, float reach);
/* The face loops the device holds for a shape: the loop of plane f is face_vertices[face_offsets[f]] ..
 * face_vertices[face_offsets[f + 1] - 1], indices into pgp_physics_shape_info's vertices, counter-clockwise seen from
 * outside, starting at the loop's lowest vertex index.  *n_faces = the plane count; face_offsets (n_faces + 1 ints, at
 * most 2 x 256 + 1) and face_vertices (twice the edge count, at most 2 x PGP_PHYSICS_MAX_EDGES ints) are nullable. */
int pgp_physics_shape_faces(pgp_ctx* ctx, int shape_id, int* face_offsets, int* face_vertices, int* n_faces);
/* Polyhedral contacts in every later settle of this context (pgp_physics_settle, _settle_device, _trace,
 * pgp_mcts_search): a separating-axis test over the face normals of both hulls and the edge pairs that form a face of
 * their Minkowski difference, then the incident face clipped against the reference face (csrc/physics.hip step 3p,
 * restated by tests/_physics_sat_restate.py).  A context setting, off by default.  While on it replaces the
 * vertex-face and the edge-edge rule, whatever pgp_physics_set_edge_contacts says; turned off, the context is back at
 * what that switch selects.  face_bias (metres, >= 0, finite): an edge axis is taken only when its separation exceeds
 * the best face separation by more than this, so that nearly equal penetrations do not flicker between a one-point
 * and a four-point manifold; the default is the reference's collision margin (PhySim.cpp:64).
 * PGP_EINVAL: NULL context or a bad face_bias (nothing changes). */
#define PGP_PHYSICS_FACE_BIAS_DEFAULT 0.001f
int pgp_physics_set_polyhedral_contacts(pgp_ctx* ctx, int on, float face_bias);
/* correctPhysics for n_states independent states, one dynamic body each: state i drops dyn_shape[i] at T[i] among the
 * table and its statics static_shape[j] at static_T[j], j in [static_offsets[i], static_offsets[i + 1]) (at most 16).
 * Poses are 16 floats column-major, object -> camera frame like every T of this header; world = cam_pose . T
 * (convertToWorld, utilities.cpp:294-296) and T_out = cam_pose^-1 . world (convertToCamera, :324-329) with the rigid
 * inverse formed on the host.  cam_pose NULL: the poses are world-frame.  table_params: the 12 floats of tableParams,
 * rows of [R | t] in the world frame.  steps == 0 copies T to T_out bit for bit.  info (nullable, n_states).
 * Host pointers, synchronous. */
int pgp_physics_settle(pgp_ctx* ctx, const pgp_physics_options* opt, int n_states, const int* dyn_shape,
                       const float* T, const int* static_offsets, const int* static_shape, const float* static_T,
                       const float table_params[12], const float cam_pose[16], float* T_out, pgp_physics_info* info);
/* The same with DEVICE arrays (d_dyn_shape, d_T, d_static_offsets, d_static_shape, d_static_T, d_T_out, d_info
 * nullable); table_params and cam_pose stay host arrays (passed by value).  Enqueued on `stream`: no synchronisation,
 * no allocation.  The shape ids and static ranges are checked on the device: a state that names an unknown shape or
 * more than 16 statics gets a NaN T_out and n_contacts = -1.  d_T_out may be d_T, and may be the d_T that
 * pgp_render_depth_device reads next on the same stream. */
int pgp_physics_settle_device(pgp_ctx* ctx, const pgp_physics_options* opt, int n_states, const int* d_dyn_shape,
                              const float* d_T, const int* d_static_offsets, const int* d_static_shape,
                              const float* d_static_T, const float table_params[12], const float cam_pose[16],
                              float* d_T_out, pgp_physics_info* d_info, void* stream);
/* Debug export for parity tests: one state (n_static statics), host pointers, synchronous.  Per step k (opt->steps):
 * state[k][13] = world x[3], q[4] (x, y, z, w), v[3], omega[3] after the step; contacts[k][68][8] = point[3],
 * normal[3], depth, final lambda_n of each reduced contact in solver order; n_contacts[k] their count. */
int pgp_physics_trace(pgp_ctx* ctx, const pgp_physics_options* opt, int dyn_shape, const float T[16], int n_static,
                      const int* static_shape, const float* static_T, const float table_params[12],
                      const float cam_pose[16], float* state, float* contacts, int* n_contacts);

/* ---- MCTS hypothesis selection: UCTSearch::performSearch ----------------------------------------------------------
 * Replaces the node's MCTS verification mode (SceneCfg.cpp:410-421 -> HypothesisSelection.cpp:241-265 ->
 * mcts/UCTSearch.cpp, mcts/UCTState.cpp).  The tree and the stop rules live on the host; every state is settled
 * (pgp_physics_settle's kernel), rendered (pgp_render_depth's) and costed (pgp_depth_cost's) on the device, one
 * launch per level and stage for all the descents of a step.  The search rules are stated exactly in csrc/mcts.hip
 * and restated in Python by tests/_mcts_restate.py.  leaves_per_step = 1 follows the reference's order exactly;
 * B > 1 makes B descents per step with in-flight (virtual) visits. */
#define PGP_MCTS_ROLLOUT_RANDOM 0   /* UCTSearch::defaultPolicy: a counter-based draw per (descent, level) */
#define PGP_MCTS_ROLLOUT_LCP 1      /* UCTSearch::LCPPolicy: the first hypothesis of the highest score */
#define PGP_MCTS_MAX_OBJECTS 17     /* the newest object settles among at most 16 statics */
#define PGP_MCTS_MAX_LEAVES_PER_STEP 256
#define PGP_MCTS_STOP_EXPANSIONS 1  /* expansions >= max_expansions (the reference's test) */
#define PGP_MCTS_STOP_ITERATIONS 2  /* descents == max_iterations */
#define PGP_MCTS_STOP_EXHAUSTED 3   /* every node of the tree expanded: the best state can no longer change */
#define PGP_MCTS_STOP_TIME 4        /* elapsed > max_seconds after a step */
typedef struct {
  long long max_expansions;      /* <= 0: the reference's sum_{i=0..n_obj} 25^i (UCTSearch.cpp:290-293), clamped to 2^31-1 */
  int max_iterations;            /* cap on descents (the reference has none); > 0 */
  float max_seconds;             /* maxSearchTime (60, UCTSearch.cpp:10); 0 = none; checked between steps only */
  float alpha;                   /* 5000 (UCTState.cpp:10): the exploration weight of getBestChild */
  float explanation_threshold;   /* 0.01 (UCTState.cpp:8): computeCost's pixel threshold */
  int rollout;                   /* PGP_MCTS_ROLLOUT_RANDOM (the live defaultPolicy) | PGP_MCTS_ROLLOUT_LCP */
  unsigned long long seed;       /* the random rollout's draws */
  int leaves_per_step;           /* B in [1, 256]; 1 = the reference's order exactly */
  float virtual_cost;            /* V, the reward of an in-flight visit when B > 1; <= 0: rows * cols */
  pgp_physics_options physics;   /* correctPhysics */
} pgp_mcts_options;
/* One object of objOrder: its physics shape, its render mesh and its hypothesisSet. */
typedef struct {
  int shape_id;              /* from pgp_physics_add_shape */
  const float* vertices;     /* n_vert x vertex_stride floats (stride 3 or 4), object frame; host */
  int vertex_stride;
  int n_vert;
  const int* triangles;      /* n_tri x 3 vertex indices, or NULL: vertices are splatted (pgp_render_depth) */
  int n_tri;
  int n_hyp;                 /* >= 1 */
  const float* T;            /* n_hyp x 16 column-major, object -> camera frame */
  const float* scores;       /* n_hyp LCP scores (finite, >= 0): the children's hval */
} pgp_mcts_object;
typedef struct {
  long long descents;            /* tree-policy descents (the reference's loop iterations) */
  long long steps;               /* device steps: one synchronisation each */
  long long expansions;          /* numExpansionsSearch: nodes added to the tree */
  long long settle_evaluations;  /* states settled (expanded children plus rollout levels) */
  int stop_reason;               /* PGP_MCTS_STOP_* */
  float elapsed_ms;              /* wall time of the search, uploads and downloads included */
} pgp_mcts_info;
typedef struct {
  int step;            /* the step that made this descent */
  int t;               /* the descent's global 0-based index */
  int depth;           /* depth of the selected node: the expanded child, or a leaf selected again */
  int hyp[PGP_MCTS_MAX_OBJECTS];   /* the full leaf state's hypothesis per object (-1 past n_obj) */
  int evaluated;       /* 1: this descent settled, rendered and costed a new leaf state */
  float render_score;  /* the leaf state's renderScore */
  float reward;        /* what backupReward added along the path */
} pgp_mcts_record;
int pgp_mcts_default_options(pgp_mcts_options* opt);
/* Runs the search over n_obj objects (1 .. 17) on the frame `observed` (cam->rows x cam->cols float metres, host).
 * table_params: tableParams (12 floats, rows of [R | t], world frame); cam_pose: camPose (column-major, NULL: poses
 * are world-frame), as in pgp_physics_settle.  opt NULL: the defaults.  best_hyp[n_obj] and best_T[n_obj x 16]
 * receive the best leaf state (bestState): its hypothesis ids and its settled poses (camera frame); *best_score its
 * renderScore (bestRenderScore).  info (nullable).  trace (nullable, trace_cap records): one record per descent in
 * order; *n_trace (nullable) the number of descents, which may exceed trace_cap (the list is then truncated).
 * PGP_EINVAL: n_obj outside 1..17, n_hyp < 1, a NaN, infinite or negative score, a non-finite pose, an unknown shape
 * id, a bad mesh, leaves_per_step outside 1..256, alpha not finite, max_iterations <= 0, bad physics options, NULL
 * observed.
 * Synchronous; the context stays usable after an error. */
int pgp_mcts_search(pgp_ctx* ctx, const pgp_mcts_options* opt, const pgp_mcts_object* objs, int n_obj,
                    const float table_params[12], const float cam_pose[16], const pgp_camera* cam, const float* observed,
                    int* best_hyp, float* best_T, float* best_score, pgp_mcts_info* info, pgp_mcts_record* trace,
                    int trace_cap, int* n_trace);

/* ---- trimmed-ICP refinement of MCTS child states: UCTState::performTrICP --------------------------------------------
 * Replaces UCTState::performTrICP (UCTState.cpp:137-139, 142-174, 194; called at UCTSearch.cpp:98, 157, 225 between
 * updateNewObject and correctPhysics).  One launch refines n states, ONE workgroup per state from the unexplained
 * filter to the final pose (csrc/tricp_states.hip, restated by tests/_tricp_restate.py).  Per state:
 *   1. unexplained filter: a point of the object's segment is dropped when any point of any static's model, placed at
 *      that static's pose, lies strictly within removal_radius (pgp_unexplained_segment's arithmetic; every static
 *      with its OWN model); skipped without statics or with removal_radius <= 0.  The kept points keep their order.
 *   2. guess G = rigid inverse of T (camera -> object), float64, rounded once;
 *   3. TrimmedICP of the kept points onto the object's model (pgp_icp_refine's definition, trimmed form):
 *      k = (int)|trim_fraction * (float)n_kept| clamped to [1, n_kept], exhaustive nearest neighbours, the k smallest
 *      distances (ties: lowest source index), Horn's closed form, while E / E_old < energy_ratio;
 *   4. T <- rigid inverse of G.
 * The library's own rules: k < 3 (n_kept == 0 included) leaves the state exactly as it came (T bit for bit, iters 0,
 * energy 0); a non-finite pose, an unknown object index or more than 16 statics gives a NaN T and iters = -1 in the
 * device call (the host call refuses them); a model of one or two points leaves the rotation about it undetermined: the
 * result is then some proper rigid pose that puts the selected points' centroid on their targets' (n_kept, iters and
 * energy are what they are for any such pose).  Exhaustive search: no index of the target yet.
 * With trim_fraction 0.5 on a segment that overlaps its model completely TrimmedICP can stall some degrees from the
 * optimum (the half it keeps is already at rest); 0.9 recovers 5 mm / 5 degree offsets. */
#define PGP_TRICP_MAX_SEGMENT 4096   /* points of one object's segment */
#define PGP_TRICP_MAX_STATICS 16     /* placed objects of one state */
#define PGP_TRICP_MAX_MODEL 65535    /* points of one object's model */
typedef struct {
  float trim_fraction;    /* 0.5 = trimICPthreshold (UCTSearch.cpp:9); (0, 1] */
  float removal_radius;   /* 0.008 = pointRemovalThreshold (UCTState.cpp:9); <= 0: no filter */
  float energy_ratio;     /* 1.0 (UCTState.cpp:139) */
  int max_iterations;     /* <= 0: 100; at most 1000 */
} pgp_tricp_options;
typedef struct {
  const float* model_xyz;     /* n_model x 3 floats, object frame; host */
  int n_model;                /* 1 .. PGP_TRICP_MAX_MODEL */
  const float* segment_xyz;   /* n_segment x 3 floats, camera frame; host */
  int n_segment;              /* 0 .. PGP_TRICP_MAX_SEGMENT */
} pgp_tricp_object;
int pgp_tricp_default_options(pgp_tricp_options* opt);
/* Copies the clouds of n_obj objects to the device; replaces an earlier set; n_obj == 0 frees them.  The call drains the
 * device first (launches of pgp_tricp_states_device still queued on a caller's stream read the set that is replaced);
 * it must not be made while a stream is capturing.  Coordinates are not checked for being finite: a segment point with a
 * NaN, an infinite or a huge coordinate (its squared distances are NaN or overflow) is never explained by a static, finds
 * no neighbour (d2 = FLT_MAX), is ranked last by the trim and never enters a sum; a model point of that kind explains
 * nothing and is nobody's nearest neighbour.  PGP_EINVAL: an empty or oversized model, a segment over the limit,
 * a NULL cloud (the earlier set stays). */
int pgp_tricp_set_objects(pgp_ctx* ctx, const pgp_tricp_object* objs, int n_obj);
/* Refines n_states states: state i is object obj[i] at T[i] (16 floats column-major, object -> camera, in/out) among
 * the statics (static_obj[j], static_T[j]), j in [static_offsets[i], static_offsets[i + 1]).  energy (the last
 * iteration's mean squared distance of the selected pairs), iters and n_kept are nullable.  opt NULL: the defaults.
 * Host pointers, synchronous.  PGP_ESTATE: no object set.  PGP_EINVAL with a message: an object index out of range,
 * more than 16 statics, a non-finite pose, non-finite or out-of-range options. */
int pgp_tricp_states(pgp_ctx* ctx, const pgp_tricp_options* opt, int n_states, const int* obj, float* T,
                     const int* static_offsets, const int* static_obj, const float* static_T, float* energy, int* iters,
                     int* n_kept);
/* The same with DEVICE arrays, enqueued on `stream`: no synchronisation, no allocation.  The states are checked on the
 * device: a bad one gets a NaN T, iters = -1, energy = 0 and n_kept = 0.  d_static_obj and d_static_T may be NULL only
 * together and only when NO state of the batch has statics (the ranges are on the device, the host cannot look): then a
 * state whose range is not empty is a bad state. */
int pgp_tricp_states_device(pgp_ctx* ctx, const pgp_tricp_options* opt, int n_states, const int* d_obj, float* d_T,
                            const int* d_static_offsets, const int* d_static_obj, const float* d_static_T,
                            float* d_energy, int* d_iters, int* d_n_kept, void* stream);
/* The switch, in the style of pgp_physics_set_edge_contacts: every later pgp_mcts_search of the context runs
 * pgp_tricp_states' kernel on each state that adds an object, before it is settled (object l of the search is object
 * l of the set, its statics the objects 0 .. l-1 at their settled poses).  opt NULL: the defaults; on == 0: off (the
 * default): the search's launches are exactly those without this call.  While on, pgp_mcts_search returns PGP_EINVAL
 * when the context holds no object set or one whose count differs from n_obj. */
int pgp_mcts_set_tricp(pgp_ctx* ctx, int on, const pgp_tricp_options* opt);

/* ---- several GPUs of one node (north_star; SceneCfg.cpp:376-406 and
 * HypothesisSelection.cpp:248-257 are the consumers) -----------------------------------------------
 * A pgp_multi is a group of devices in ONE process: one pgp_ctx, one host thread and one stream per
 * device, the clouds and the index replicated on each.  pgp_multi_score_lcp block-partitions the
 * n_h hypotheses (pgp_multi_slice: contiguous slices, sizes differing by at most one), every device
 * scores its slice into a zero-initialised full-length vector, ONE RCCL all-reduce(sum) over xGMI
 * (scores as float, counts as int32, grouped) leaves every device with all of them, and device 0
 * takes the arg-max (pgp_settle_best_device) and copies the arrays back.  Outputs are those of
 * pgp_score_lcp on one device, bit for bit (plain) / with the same summation tree (weighted).
 * device_ids NULL = devices 0 .. n_dev-1; n_dev <= 0 = every visible device.  RCCL (librccl.so.1)
 * is bound at run time and only when the group has more than one device (or
 * PGP_MULTI_FORCE_COLLECTIVE=1).  Every member's worker thread queues its slice, its own ncclAllReduce (one
 * communicator per device) and, on member 0, the arg-max and the copy back: one rendezvous of the calling thread per
 * call.
 * Member 0 holds all transforms (it settles near-ties across slices), the others copy their slice only.
 * Calls on one pgp_multi must not overlap. */
typedef struct pgp_multi pgp_multi;
int pgp_multi_create(pgp_multi** out, const int* device_ids, int n_dev);
int pgp_multi_destroy(pgp_multi* m);
int pgp_multi_size(const pgp_multi* m);
pgp_ctx* pgp_multi_context(pgp_multi* m, int k);       /* device k's context, for the other entry points */
int pgp_multi_slice(int n_total, int k, int n_dev, int* lo, int* hi);   /* host helper: device k's [lo, hi) */
int pgp_multi_set_scene(pgp_multi* m, const float* xyz, const float* nrm, const float* weight, int n,
                        float delta);
int pgp_multi_set_scene_weights(pgp_multi* m, const float* weight, int n);
int pgp_multi_set_model(pgp_multi* m, const float* xyz, const float* nrm, int n);
int pgp_multi_score_lcp(pgp_multi* m, const float* T, int n_h, int mode, float gate_deg, float* scores,
                        int* counts, int* best_index, float* best_score);
/* The two halves of pgp_multi_score_lcp, for callers that score one resident batch repeatedly
 * (bench.py): copy the transforms to every device once, then score what is there. */
int pgp_multi_upload(pgp_multi* m, const float* T, int n_h);
int pgp_multi_score_uploaded(pgp_multi* m, int mode, float gate_deg, float* scores, int* counts,
                             int* best_index, float* best_score);
/* ---- a group that holds SEVERAL objects (BASELINE configs[3]: 6 objects, 64 k hypotheses over 8 GPUs) -----
 * The node loops over the objects of a frame (PPE/data_layer/SceneCfg.cpp:376-406), each with its own segment (scene
 * side), validation model and hypothesis list.  An OBJECT of a group is one such (scene, model) pair, replicated on
 * every member; object 0 exists from pgp_multi_create on -- the single-object entry points above act on it --
 * and pgp_multi_add_object appends one (returns its id >= 1, or a negative PGP_E* code).
 * pgp_multi_score_objects flattens (object, hypothesis) into ONE index space (object after object), gives member k the
 * contiguous share pgp_multi_slice(sum n_h, k, ...) of it -- pgp_multi_flat_slices lists that share as (object, lo, hi)
 * pieces --, every member scores its pieces on the objects' contexts into a zeroed full-length vector, ONE all-reduce
 * for the concatenated {scores | counts} of all objects, and member 0 takes every object's arg-max with the near-tie
 * settlement of pgp_settle_best_device (pgp_set_exact_records / pgp_set_verify_early_out on
 * pgp_multi_object_context(m, obj, 0) apply as for one object).
 *   T[n_obj], n_h[n_obj]: every object's transform list (objects 0 .. n_obj-1 of the group; a count may be 0)
 *   scores / counts (nullable): flat, sum(n_h) entries, object after object -- per object what pgp_score_lcp returns
 *   best_index[n_obj] (nullable): per object, relative to the object's list; best_score[n_obj] (nullable). */
int pgp_multi_add_object(pgp_multi* m);
int pgp_multi_objects(const pgp_multi* m);
pgp_ctx* pgp_multi_object_context(pgp_multi* m, int obj, int k);
int pgp_multi_set_object_scene(pgp_multi* m, int obj, const float* xyz, const float* nrm, const float* weight, int n,
                               float delta);
int pgp_multi_set_object_scene_weights(pgp_multi* m, int obj, const float* weight, int n);
int pgp_multi_set_object_model(pgp_multi* m, int obj, const float* xyz, const float* nrm, int n);
int pgp_multi_set_object_search_model(pgp_multi* m, int obj, const float* xyz, int n);
int pgp_multi_set_object_ppf_map(pgp_multi* m, int obj, const int* keys, const int* counts, const int* pairs, int n_keys);
/* pgp_set_ppf_map_from_model on every member's context of the object: each member builds its own copy (nothing but
 * the n points and normals crosses to it); the counts are member 0's, and every member's are the same. */
int pgp_multi_set_object_ppf_map_from_model(pgp_multi* m, int obj, const float* xyz, const float* nrm, int n, int* n_keys,
                                            long long* n_pairs);
int pgp_multi_flat_slices(const int* n_h, int n_obj, int k, int n_dev, int* obj, int* lo, int* hi, int* n_pieces);
int pgp_multi_score_objects(pgp_multi* m, const float* const* T, const int* n_h, int n_obj, int mode, float gate_deg,
                            float* scores, int* counts, int* best_index, float* best_score);
int pgp_multi_upload_objects(pgp_multi* m, const float* const* T, const int* n_h, int n_obj);
int pgp_multi_score_objects_uploaded(pgp_multi* m, int mode, float gate_deg, float* scores, int* counts, int* best_index,
                                     float* best_score);

/* ICP over the group: the poses to refine are sharded like the hypotheses ("shard poses-to-refine the same way;
 * no collective except the final gather").  The jobs are the (segment, target) pairs of pgp_icp_refine -- the children of
 * an MCTS expansion (PPE/hypothesis_verification/mcts/UCTSearch.cpp:200-266 -> UCTState.cpp:121-204), the objects of a
 * frame -- with HOST pointers; the flat (job, pose) space is block-partitioned over the members
 * (pgp_multi_flat_slices), every member refines its pieces in ONE launch (pgp_icp_refine_multi_device; the target of job
 * j keeps its index on the member's j-th ICP context from call to call) and writes its poses' results straight into the
 * caller's arrays.  Results are those of one pgp_icp_refine per job on one context, bit for bit. */
typedef struct {
  const float* src_xyz;  /* n_src x 3: the points that are moved (the segment) */
  int n_src;
  const float* tgt_xyz;  /* n_tgt x 3: the cloud searched for neighbours (the model) */
  int n_tgt;
  float* T;              /* [n][16] in/out */
  int n;
  float* energy;         /* [n], nullable */
  int* iters;            /* [n], nullable */
} pgp_multi_icp_job;
int pgp_multi_icp_refine(pgp_multi* m, const pgp_multi_icp_job* jobs, int n_jobs, const pgp_icp_params* params);

/* Congruent sets over the group: the bases of an object are sharded ("shard by base (100 bases/object);
 * gather variable-length transform lists on host"; the loop base.cc:1855-1874).  Member k runs pgp_find_congruent_batch
 * for the bases pgp_multi_slice(n_bases, k, ...) on its context of object `obj` (which needs the object's scene, search
 * model and pair-feature table: pgp_multi_set_object_*), n_quads[n_bases] is gathered, and the sorted quad lists stay on
 * the member that owns the base.  pgp_multi_congruent_batch_quads / _fit route every pick (base, j) to that member and
 * return the results in the caller's pick order -- what pgp_congruent_batch_quads / _fit return on one context
 * (base_ids[n_bases][4] as there). */
int pgp_multi_find_congruent_batch(pgp_multi* m, int obj, const int* base_ids, const float* base_xyz,
                                   const float* invariants, int n_bases, float threshold, int* n_quads);
int pgp_multi_congruent_batch_quads(pgp_multi* m, int obj, const int* picks, int cnt, int* quads);
int pgp_multi_congruent_batch_fit(pgp_multi* m, int obj, const int* picks, const int* base_ids, int cnt,
                                  const float centroid_P[3], const float centroid_Q[3], float* T, double* pose,
                                  int* status, float* rms);

/* ---- a group that spans several PROCESSES (one process per GPU under a launcher: python -m torch.distributed.run, mpirun) ----
 * The same group, its members spread over processes: this process holds n_local members (devices device_ids[0 ..
 * n_local-1]) which are ranks rank0 .. rank0 + n_local - 1 of `world`.  One process calls pgp_multi_unique_id
 * (ncclGetUniqueId; 128 bytes) and hands the id to the others by whatever channel the launcher offers (a torch.distributed
 * store, MPI_Bcast, a file); every process then calls pgp_multi_create_ranked with it (ncclCommInitRank: the calls meet).
 * Every process uploads the SAME clouds and the SAME complete hypothesis list; rank r scores the slice
 * pgp_multi_slice(n_h, r, world), the all-reduce leaves every process with all scores, and member 0 of EVERY process takes
 * the arg-max -- each process returns what pgp_score_lcp returns on one device.  The scoring entry points
 * (pgp_multi_score_lcp, _upload, _score_uploaded, _score_objects*, the streaming form below) work on such a group; the
 * calls that gather into the caller's arrays without a collective (pgp_multi_icp_refine, pgp_multi_find_congruent_batch,
 * ...) need a single-process group and return PGP_ESTATE otherwise.  The consumer is the same per-object loop
 * (SceneCfg.cpp:376-406) in a node that was started once per GPU. */
int pgp_multi_unique_id(void* id128);
int pgp_multi_create_ranked(pgp_multi** out, const int* device_ids, int n_local, int rank0, int world, const void* id128);

/* What the group is made of.  rccl_ranks = ncclCommCount of the communicator the exchange runs on (0: the group has no
 * communicator -- one member without PGP_MULTI_FORCE_COLLECTIVE, or an emulated group); exchanges = all-reduces (or, in
 * an emulated group, sum kernels) issued so far. */
typedef struct {
  int n_local, world, rank0;
  int rccl_ranks;
  int emulated;
  int devices[16];        /* the first 16 local members' devices */
  long long exchanges;
} pgp_multi_info;
int pgp_multi_get_info(pgp_multi* m, pgp_multi_info* info);

/* ---- streaming form: the verification loop batch after batch without a host wait per batch (base.cc:1885-1901 run over
 * the lists of successive objects / expansions; bench.py's N > 1 headline) --------------------------------------------
 * pgp_multi_upload_slot leaves a hypothesis list resident in one of 16 slots (object 0's clouds; synchronous).
 * pgp_multi_enqueue_slot queues one scoring step over a slot and returns: every member scores its slice into one of two
 * {scores | counts} vectors on its stream, the all-reduce runs on a SECOND stream of the member -- under the scoring of
 * the next step --, and member 0's arg-max (near-tie settlement, exact records, Verify's early termination as set on
 * member 0's context) follows it on that second stream, with a settlement workspace of its own.  pgp_multi_collect completes everything queued and
 * returns the LAST step's arrays, bit for bit those of pgp_multi_score_lcp on the same list.  pgp_multi_upload_slot
 * between an enqueue and its collect returns PGP_ESTATE. */
int pgp_multi_upload_slot(pgp_multi* m, int slot, const float* T, int n_h);
int pgp_multi_enqueue_slot(pgp_multi* m, int slot, int mode, float gate_deg);
int pgp_multi_collect(pgp_multi* m, float* scores, int* counts, int* best_index, float* best_score);

/* Host wall clock of the last scoring call in ms: upload (pinned copy + H2D enqueue), enqueue
 * (kernels + collective issued on every device), total (until the results are back). */
int pgp_multi_last_timing(pgp_multi* m, float* upload_ms, float* enqueue_ms, float* total_ms);

/* Per-kernel timing for bench.py's roofline line.  enable = N >= 1: every Nth pgp_score_lcp[_device]
 * call (the 1st, N+1st, ...) attaches a start and a stop HIP event to its dominant kernel's dispatch
 * (score_hypotheses), on the SAME stream it is launched on; 0 switches it off.  Timing a launch costs
 * the stream about 8 us (the runtime serialises around a timed dispatch), which is why a throughput
 * measurement samples (N = 8 in bench.py) instead of timing every step.  pgp_get_kernel_timing
 * synchronises those events and returns the number of timed launches and the sum of their
 * durations since the last reset. */
int pgp_set_kernel_timing(pgp_ctx* ctx, int enable);
int pgp_get_kernel_timing(pgp_ctx* ctx, int* launches, float* total_ms, int reset);

/* ---- model clouds from an object's mesh: surface sampling + farthest-point order -----------------------------------
 * The node reads model_validation.ply and model_search.ply, prepared offline (PPE/data_layer/Objects.cpp:22-28).  These
 * calls make both from the mesh that pgp_mcts_object / pgp_physics_add_shape already take: a dense oriented sample of
 * the surface, put into farthest-point order.  Both rules are exact: tests/_model_prep_restate.py reproduces every
 * output bit for bit in numpy.
 *
 * pgp_sample_mesh: n_samples points of the surface, uniform by area.  vertices: n_vert x vertex_stride floats (stride 3
 * or 4, as in pgp_mcts_object), triangles: n_tri x 3 ints, 1 <= n_tri <= PGP_SAMPLE_MESH_MAX_TRIANGLES.  Out:
 * xyz[n_samples][3], nrm[n_samples][3] (nullable), tri[n_samples] (nullable: the triangle a sample lies on).
 *   Area.  e1 = v1 - v0 and e2 = v2 - v0 in double from the float vertices, c = e1 x e2, A_t = 0.5 sqrt((cx cx + cy cy)
 *     + cz cz), every operation rounded on its own, the square root correctly rounded.
 *   Integer weights.  A_max = the exact maximum; w_t = (uint64) floor((A_t / A_max) 2^32) with an IEEE double divide;
 *     C_t = the inclusive prefix sums in uint64 and W = C_{n_tri - 1} < 2^55, so no order of summation shows.  A
 *     triangle whose w_t is 0 -- no area, or less than 2^-32 of the largest -- is NEVER drawn.
 *   Draws.  Sample s uses v_i = variate i (31 bits, i = 0 .. 3) of the counter-based stream (seed, s) that
 *     pgp_sample_quads and pgp_fit_plane draw from.  r = v0 << 31 | v1 (62 bits); target = (r W) >> 62 from the 128-bit
 *     product; the triangle is the first t with C_t > target.
 *   Position.  a = float(v2) 2^-31, b = float(v3) 2^-31 (the integer converted round-to-nearest, then scaled); if a + b
 *     > 1 then a = 1 - a, b = 1 - b; p = (v0 + a (v1 - v0)) + b (v2 - v0) per component in float, in that order, each
 *     operation rounded on its own.
 *   Normal.  (v1 - v0) x (v2 - v0) in float, normalised as Eigen's normalized() does (left as it is when its squared
 *     norm is 0): the winding gives the side.
 * PGP_EINVAL: a NaN or infinite vertex, an index outside [0, n_vert), W == 0 (no triangle has an area), bad counts or a
 * bad stride.  The host form checks vertices and indices before anything is launched.  The _device form takes device
 * arrays, is enqueued on `stream` and SYNCHRONISES that stream once, for the error flag; a flagged mesh is never read
 * out of bounds, and the outputs are then left unwritten. */
#define PGP_SAMPLE_MESH_MAX_TRIANGLES 4194304
int pgp_sample_mesh(pgp_ctx* ctx, const float* vertices, int n_vert, int vertex_stride, const int* triangles, int n_tri,
                    int n_samples, unsigned long long seed, float* xyz, float* nrm, int* tri);
int pgp_sample_mesh_device(pgp_ctx* ctx, const float* d_vertices, int n_vert, int vertex_stride, const int* d_triangles,
                           int n_tri, int n_samples, unsigned long long seed, float* d_xyz, float* d_nrm, int* d_tri,
                           void* stream);

/* The farthest-point order of a cloud: xyz n x 3 floats, 1 <= k <= n (else PGP_EINVAL); order[k], radius2[k] (nullable).
 * order[0] = start; start == -1: the point of largest x, ties to the lowest index (pgp_convex_hull's rule).  Every
 * point keeps d_i, the smallest squared distance to a point picked so far, computed in float as (dx dx + dy dy) + dz dz
 * of the rounded differences p_i - p_pick, each operation rounded on its own; a picked point's d becomes -1, so a
 * duplicate is never picked twice.  The next pick is the largest d under strict >, ties to the lowest index.
 * radius2[0] = FLT_MAX, radius2[j] = d of pick j at the moment it was picked: non-increasing from j = 1 on, and the
 * squared covering radius of the first j picks.  Every prefix of the order is the order of a smaller k.
 * Two forms with identical results: n <= 16384 runs in ONE workgroup that keeps the cloud in registers for all k
 * picks; a larger n takes one launch per pick over up to 256 workgroups (no workgroup waits for another), queued back to
 * back.  PGP_FPS_FORM=multi in the environment forces the second form at any n (a checker path).
 * The host form rejects non-finite points and start outside -1 .. n - 1.  The _device form takes float4 points
 * {x, y, z, -} like the ICP calls, is enqueued on `stream` and does not synchronise; the multi-launch form may grow
 * its workspace (an allocation) on first use. */
int pgp_farthest_points(pgp_ctx* ctx, const float* xyz, int n, int k, int start, int* order, float* radius2);
int pgp_farthest_points_device(pgp_ctx* ctx, const float* d_xyz4, int n, int k, int start, int* d_order, float* d_radius2,
                               void* stream);

/* Both in one call, the dense sample never leaving the device: pgp_sample_mesh(n_dense samples, seed), then
 * pgp_farthest_points(k = n_model <= n_dense, start = -1) over them; xyz[n_model][3], nrm[n_model][3] (nullable),
 * tri[n_model] (nullable) are the rows order[0 .. n_model) of the sample, radius2[n_model] (nullable) as above -- bit
 * for bit the two calls composed.  Rows 0 .. m - 1 are the farthest-point subset of size m for EVERY m <= n_model: a
 * model_validation cloud made this way holds its model_search cloud as its first rows.  Host pointers, synchronous. */
int pgp_model_from_mesh(pgp_ctx* ctx, const float* vertices, int n_vert, int vertex_stride, const int* triangles, int n_tri,
                        int n_dense, int n_model, unsigned long long seed, float* xyz, float* nrm, int* tri, float* radius2);

#ifdef __cplusplus
}
#endif
#endif /* PGP_H */
