/*
 * rgbd360_overlap.h -- sensed-space overlap of the frames of a resident frame store: which pairs are worth an alignment.
 * Part of the C ABI of rgbd360_hip.h, which includes this header at its end; include either.  Device side: csrc/store_overlap.h,
 * host side: csrc/rgbd360_host.cpp.
 */
#ifndef RGBD360_OVERLAP_H
#define RGBD360_OVERLAP_H

#include "rgbd360_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- sensed-space overlap of stored frames (csrc/store_overlap.h) -----------------------------------------------------------
 * Which pairs of stored frames are worth an alignment.  The reference scores a pair by its SSO, visible pixels / image size, which it
 * only has after a finished alignment (RegisterPhotoICP.h:3226; keyframe selection KFsphere_SLAM.cpp:402-478, connection scores
 * LoopClosure360.h:321, 360, the adjacency matrices of TopologicalMap360.h:65, 107-131).  With the frames resident, the overlap of
 * any list of pairs, or of all ordered pairs of a set of frames, is one launch at a coarse pyramid level: no Jacobians, no solve.
 * On a 360-degree image nearly every point lands somewhere, so the measure also compares ranges.  Per pair: target entry t, source
 * entry s, pose T (source in target, 16 floats column-major, as the guesses of rgbd360_store_align), level L.  Every source pixel,
 * on its own (no z-buffer, no winner rule; all counts are exact integers and do not depend on any order):
 *   1 point    the source point of entry s at level L as the per-pixel pass loads it; valid as the pass tests it        -> n_valid
 *   2 warp     the warp of rgbd360_warp_indices / rgbd360_warp_images in the context's index arithmetic: visibility, target pixel,
 *              range = |R p + t|.  Valid and visible -> n_visible: the rows != (-1,-1) rgbd360_warp_indices reports for a context
 *              holding the two frames, the reference's numVisiblePixels
 *   3 target   D = the target entry's depth at that pixel; visible and D finite (RegisterPhotoICP.h:3064)               -> n_target
 *   4 classes  float32, every operation rounded on its own (no fused multiply-add):
 *                diff = range - D;   tol = tol_abs + tol_rel * D
 *                |diff| <= tol  n_consistent;   diff > tol  n_behind (hidden behind the surface the target sees);
 *                -diff > tol    n_in_front (the target sees past it).     n_consistent + n_behind + n_in_front == n_target.
 * Both calls follow the store's rules (one thread at a time, destroyed before the context), synchronise once, and leave the
 * alignment engines untouched: rgbd360_store_align gives the same bits before and after.
 * Out of scope: normalised-cut partitioning of the matrix (TopologicalMap360::Partitioner, MRPT's spectral partition), PbMap guesses,
 * occlusion-aware (z-buffered) overlap, distinct-target-pixel coverage, the pinhole and rig paths, several GPUs. */
typedef struct {
    int   level;              /* pyramid level, 0 .. n_pyr-1 (-3 otherwise) */
    float tol_abs, tol_rel;   /* metres, and a fraction of the target depth; both finite and >= 0 (-1 otherwise) */
} rgbd360_overlap_params;
typedef struct {
    int32_t evaluated;        /* 1: the pair was evaluated; 0: skipped by rgbd360_store_overlap_all (every count is 0 then) */
    int32_t n_valid, n_visible, n_target, n_consistent, n_behind, n_in_front, reserved;
} rgbd360_overlap;
/* level = the coarsest (n_pyr - 1), tol_abs = 0.05, tol_rel = 0.02 (the project's max_depth_change_factor): conventions. */
void rgbd360_store_overlap_default_params(const rgbd360_store* st, rgbd360_overlap_params* p);
/* n_pairs records in list order; poses: n_pairs x 16 floats, NULL = identity for all.  trg[k] == src[k] and repeated pairs are
 * allowed; n_pairs == 0 returns 0.  -1 and no launch at all if any index is out of range or names an empty entry (the message names
 * the first such pair), -3 bad level, -1 bad tolerance; other negatives: HIP errors. */
int  rgbd360_store_overlap(rgbd360_store* st, int n_pairs, const int* trg, const int* src, const float* poses,
                           const rgbd360_overlap_params* params, rgbd360_overlap* out);
/* The matrix of n distinct, occupied entries at their world poses (n x 16 floats, column-major, world <- frame):
 * out[a * n + b] = target entries[a], source entries[b] at the relative pose T_ab = W_a^-1 W_b, computed on the host in float64 from
 * the float32 inputs and rounded to float32 once.  With R(r,c) = W[4 c + r], t(r) = W[12 + r], r, c = 0..2, all in float64:
 *   it(r)     = -((Ra(0,r) ta(0) + Ra(1,r) ta(1)) + Ra(2,r) ta(2))                      the translation of (Ra^T, -Ra^T ta)
 *   R_ab(r,c) =  (Ra(0,r) Rb(0,c) + Ra(1,r) Rb(1,c)) + Ra(2,r) Rb(2,c)
 *   t_ab(r)   = ((Ra(0,r) tb(0) + Ra(1,r) tb(1)) + Ra(2,r) tb(2)) + it(r)
 * every product and sum rounded on its own; the last row is 0 0 0 1.  A pair is evaluated iff a != b and
 * sqrt((t_ab(0)^2 + t_ab(1)^2) + t_ab(2)^2) (float64, before the rounding to float32) <= max_translation; max_translation <= 0 or
 * not finite: every a != b.  Skipped pairs are all zero.  An evaluated record is identical to what rgbd360_store_overlap returns for
 * (entries[a], entries[b], T_ab).  rel_poses_out (may be NULL): 16 n n floats, T_ab of every pair, skipped ones and the diagonal
 * included.  -1 if an entry is out of range, empty or named twice. */
int  rgbd360_store_overlap_all(rgbd360_store* st, int n, const int* entries, const float* world_poses, float max_translation,
                               const rgbd360_overlap_params* params, rgbd360_overlap* out, float* rel_poses_out);
/* Host side, no device: which pairs of an overlap matrix m (n x n records as rgbd360_store_overlap_all writes them; level_px = the
 * pixels of the level it was made at) to align.  score(a,b) = min(m[a,b].n_consistent, m[b,a].n_consistent) / level_px, symmetric,
 * and 0 unless both directions were evaluated.  For b ascending, the candidates are the a < b with b - a >= min_gap,
 * score >= min_score and {a,b} not among the n_known known edges (known_a[k], known_b[k], either orientation); by score descending,
 * ties to the smaller a, at most max_per_frame of them (<= 0: no limit).  Returns the number found and writes the first max_out
 * (out_a, out_b, out_score; any may be NULL); -1 bad arguments. */
int  rgbd360_overlap_candidates(int n, const rgbd360_overlap* m, int level_px, float min_score, int min_gap, int max_per_frame, int n_known,
                                const int* known_a, const int* known_b, int max_out, int* out_a, int* out_b, float* out_score);
/* The most representative frame of a subset (TopologicalMap360.h:216-234): the member (an index into the matrix) with the largest sum
 * of score(member, other) over the other members, ties to the first in `subset`.  -1 bad arguments. */
int  rgbd360_overlap_representative(int n, const rgbd360_overlap* m, int level_px, const int* subset, int n_subset);

#ifdef __cplusplus
}
#endif
#endif /* RGBD360_OVERLAP_H */
