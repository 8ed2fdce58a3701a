/* rgbd360_hip_diag.h -- measurement and self-test entry points of librgbd360_hip.so (RGBD360_DIAG).
 *
 * Not part of the drop-in boundary (include/rgbd360_hip.h): nothing the reference's RegisterPhotoICP / Frame360 callers would
 * bind.  bench.py uses the forced schedule and the kernel timers, the GPU test-suite the arithmetic self-test; a deployment
 * may strip them.
 */
#ifndef RGBD360_HIP_DIAG_H
#define RGBD360_HIP_DIAG_H

#include "rgbd360_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Forced schedule for throughput measurement: n_iters Gauss-Newton iterations on `level`
 * starting at pose0, every step applied regardless of the accept rule, no host round trip.  One iteration =
 * one launch of k_eval_fs (the solve of the previous pass + the fused pass; the last solve in a one-block launch of its own), or one
 * fused pass + one solve launch under rgbd360_debug_set_schedule(ctx, 0, 1).  Enqueued on the context's stream; *elapsed_ms (may be NULL) is the HIP
 * event time around the n_iters iterations (NULL: no events are recorded and the call waits for its result the way
 * rgbd360_align360 does, csrc/host_wait.h). */
int rgbd360_forced_iters(rgbd360_ctx* ctx, int level, const float pose0[16], int method, int n_iters,
                         float pose_out[16], double* last_rms, float* elapsed_ms);
/* The same forced schedule in the lock-step sequence engine's regime (csrc/sequence_engine.h): n_pairs (<= 32) copies of ONE pair
 * (host images as in rgbd360_set_target / _set_source, both frames with the same strides) iterate side by side, every {pass, solve}
 * launch serving all of them.  *elapsed_ms = HIP event time around the n_iters iterations of all pairs; poses_out (may be NULL):
 * n_pairs x 16 floats, the pose every pair reached (identical for all of them, and identical to rgbd360_forced_iters').
 * pass_avg_us (may be NULL): average duration of ten back-to-back launches of the batch pass alone (all n_pairs slots) afterwards. */
int rgbd360_forced_iters_batch(rgbd360_ctx* ctx, int n_pairs, const uint8_t* rgb_trg, const void* depth_trg, const uint8_t* rgb_src,
                               const void* depth_src, size_t rgb_step, size_t depth_step, int depth_type, int rows, int cols,
                               int level, const float pose0[16], int method, int n_iters, float* poses_out, float* elapsed_ms,
                               float* pass_avg_us);
/* One solve on a hand-made partial table (row 0 = `row`: 21 upper-triangle terms of H, 6 of g, the two error sums, the three
 * counts; every other row zero) at the identity pose on `level`, through the two-launch form (fused = 0: k_solve) or the fused form
 * (fused = 1: the prologue of k_eval_fs; the state is read as that launch leaves it; fused = 2: the same with the row at table row 40
 * and a launch that was told to expect one pending row -- the device checks the host's bound and fetches the rest, same result; needs
 * a level of more than 40 block rows).  Drives the state-machine paths real images hardly ever reach (ILL-POSED).
 * out_i: {status, done, level_active, it, n_evals, pend_nb}; cand_out / update_out (may be NULL): the state's candidate pose / update. */
int rgbd360_debug_solve_partials(rgbd360_ctx* ctx, int level, const double row[32], int method, int fused, int out_i[6],
                                 float cand_out[16], float update_out[6]);
/* One pending solve on a hand-made partial TABLE at the identity pose on `level`: table rows 0 ... n_rows - 1 = `rows` (n_rows x 32
 * doubles, 1 <= n_rows <= 256), every other row zero, the state's pend_nb = n_rows.  route 0: k_solve on n_rows rows; 1: the prologue
 * of the fused launch k_eval_fs; 2: k_solve_pending; routes 1 and 2 are launched with rows_hint (1 ... 256) as the host's bound on the
 * pending rows -- a bound below n_rows is the late-row path: the device notices and fetches the rest.  tot_out: the state's 32 column
 * totals (a wrong row group or summation order shows in their bits; one row cannot show it).  out_i, cand_out (may be NULL): as
 * rgbd360_debug_solve_partials.  Both frames must be set. */
int rgbd360_debug_solve_table(rgbd360_ctx* ctx, int level, const double* rows, int n_rows, int rows_hint, int method, int route,
                              double tot_out[32], int out_i[6], float cand_out[16]);
/* One solve from a chosen Gauss-Newton state: the state of `level` is initialised at in->pose (pose and cand), then update, lambda,
 * error, first and it are overwritten with the given values; the solve runs with the given termination settings (max_iters,
 * tol_residual, tol_update, forced) and error form (occlusion 0: sqrt(sum / n); 1 / 2: photo RMS + depth RMS) on the partial row
 * `row` (as rgbd360_debug_solve_partials).  route 0: k_solve; 1: the prologue of the fused launch k_eval_fs; 2: the same with the
 * row at table row 40 behind a launch told to expect one pending row (needs a level of more than 40 block rows).  The state is read
 * as the launch leaves it. */
typedef struct {
    float pose[16];      /* column-major */
    float update[6];
    double lambda, error;
    int first, it;
    int max_iters, forced;
    double tol_residual, tol_update;
} rgbd360_solve_state_in;
typedef struct {
    int status, done, level_active, it, n_evals, pend_nb;
    int iters_level;     /* iters[level] */
    float cand[16], pose[16], update[6];
    double lambda, error, new_error, diff_error;
} rgbd360_solve_state_out;
int rgbd360_debug_solve_state(rgbd360_ctx* ctx, int level, const double row[32], const rgbd360_solve_state_in* in, int method,
                              int occlusion, int route, rgbd360_solve_state_out* out);
/* Average duration in microseconds of `reps` back-to-back launches of the fused per-pixel kernel alone
 * (HIP events on the stream the kernel is launched on). want_hg = 0 times the error-only variant, want_hg = 2 the launch of the
 * single-pair product schedule: k_eval_fs in the forced schedule, i.e. {solve of the previous pass, pass} = one whole Gauss-Newton
 * iteration per launch. */
int rgbd360_time_eval_kernel(rgbd360_ctx* ctx, int level, const float pose[16], int method, int want_hg, int reps,
                             float* avg_us);

/* rgbd360_warp_images (rgbd360_hip.h) under HIP events, averages over `reps` back-to-back launches on `level` in microseconds:
 * avg_us[0] the winner pass, [1] the resolve pass (all four float planes), [2] the whole rgbd360_warp_images_dev sequence (clear of
 * the winner plane + both passes), [3] ONE k_warp_indices launch (the kernel of rgbd360_warp_indices) at the same size: the cost of
 * the warp alone, the yardstick for what scatter and resolve add.  Outputs go to the context's staging. */
int rgbd360_time_warp_images(rgbd360_ctx* ctx, int level, const float pose[16], int method, int reps, float avg_us[4]);

/* rgbd360_store_overlap / rgbd360_store_overlap_all (rgbd360_overlap.h) with the kernel launches of the call repeated `reps` times, each
 * repetition (counters cleared first) between two HIP events on the store's stream: kernel_us[r] = microseconds of repetition r.
 * out as in the product calls (the counts of the last repetition).  kernel (all-pairs entry): 0 the list kernel over the evaluated
 * pairs, 1 the source-stationary kernel (the product call chooses by the level's size). */
int rgbd360_store_time_overlap(rgbd360_store* st, int n_pairs, const int* trg, const int* src, const float* poses,
                               const rgbd360_overlap_params* params, int reps, float* kernel_us, rgbd360_overlap* out);
int rgbd360_store_time_overlap_all(rgbd360_store* st, int n, const int* entries, const float* world_poses, float max_translation,
                                   const rgbd360_overlap_params* params, int kernel, int reps, float* kernel_us, rgbd360_overlap* out);

/* The voxel map's kernels (rgbd360_map_*, rgbd360_hip.h) under HIP events on a sphere frame in device memory, averages over `reps`
 * rounds in microseconds: avg_us[0] k_vmap_insert into the EMPTY map, [1] k_vmap_insert into the map that already holds the frame's
 * voxels (the steady state of odometry), [2] k_vmap_extract (centroids only), [3] ONE k_sphere_cloud_s4 launch of the same size,
 * [4] a device-to-device copy of the frame's input bytes (the copy rate of the input-bytes floor).  *global_updates (may be NULL):
 * slot updates the insert into the empty map issued after on-chip combining.  The map is cleared first and holds the frame twice
 * afterwards. */
int rgbd360_map_time_kernels(rgbd360_map* map, const uint8_t* rgb_dev, size_t rgb_step, const void* depth_dev, size_t depth_step,
                             int depth_type, int rows, int cols, int convention, const float pose[16], int reps, float avg_us[5],
                             long long* global_updates);

/* The map's editing kernels (rgbd360_map_remove_* / _move_* / _rehash / _census, rgbd360_hip.h) under HIP events on a sphere frame in
 * device memory, averages over `reps` rounds in microseconds.  Every round clears the map and inserts the frame twice, so that the
 * removal empties no voxel: avg_us[0] one k_vmap_insert launch into that map (new voxels counted by their claims, the form of a map
 * that never had a voxel emptied), [1] the removal kernel over the same map, [2] one k_vmap_insert launch counting revivals (the form
 * of a map that may hold tombstones: a returning count add per entry), [3] the clear of a second table of the same size and
 * k_vmap_rehash into it (the tables are not swapped), [4] the census scan, [5] one k_vmap_extract scan (centroids only) over the same
 * table, [6] a whole move of the frame from `pose` to `pose` out of device memory (both launches and the one wait).  The map holds the
 * frame twice afterwards. */
int rgbd360_map_time_edit(rgbd360_map* map, const uint8_t* rgb_dev, size_t rgb_step, const void* depth_dev, size_t depth_step,
                          int depth_type, int rows, int cols, int convention, const float pose[16], int reps, float avg_us[7]);

/* One evaluation of the map alignment (rgbd360_map_align_*, rgbd360_hip.h: steps 1-5 of its definition) at `pose`, and the trace of
 * the map's last alignment.  depth != NULL: the sphere frame; otherwise the n points xyz.  sums[17]: n, sum w (3), sum w_j w_k (xx, xy,
 * xz, yy, yz, zz), sum e (3), sum w x e (3), sum e.e; counters[3]: n_valid, n_box_rejected, n_out_of_range.  key3_dev / d2_dev (DEVICE
 * arrays of 3 / 1 values per input point, may be NULL): the key (i_x, i_y, i_z) of the kept match, or three times INT32_MIN where the
 * point has none, and d2 of the nearest candidate whether kept or not (+Inf where the point has no candidate or did not reach the
 * search).  pose == NULL: no evaluation, the trace only.  trace (may be NULL): the first min(max_trace, steps) records of the last
 * rgbd360_map_align_* call of this map, one per applied step: the kept matches and sum e.e of the evaluation the step came from, and
 * the step; *n_trace (may be NULL): the number of steps. */
typedef struct { long long n; double sum_sq; float update[6]; } rgbd360_map_align_trace;
typedef struct { long long n; double cost; float max_vv, max_ww; } rgbd360_rig_calib_step;       /* rgbd360_rig_calib_trace below */
int rgbd360_map_align_eval(rgbd360_map* map, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                           const float* xyz, long long n, const float pose[16], int on_device, const rgbd360_map_align_params* params,
                           double sums[17], long long counters[3], int32_t* key3_dev, float* d2_dev, int max_trace, int* n_trace,
                           rgbd360_map_align_trace* trace);
/* The trace of job `job` of the map's last batch (rgbd360_map_align_batch_* / rgbd360_map_align_plane_batch_*, rgbd360_hip.h): trace
 * (may be NULL) gets the first min(max_trace, steps) records, *n_trace (may be NULL) the number of steps; the records are those of the
 * single call of that job.  A job on an empty input has none.  0; -1 for a job outside the last batch (none yet: every job).  After a
 * batch the single-call trace above is empty; after a single call the batch's traces stay what they were. */
int rgbd360_map_align_batch_trace(rgbd360_map* map, int job, int max_trace, int* n_trace, rgbd360_map_align_trace* trace);
/* The rig calibration's solve (csrc/rig_calib.h; the definition is in rgbd360_hip.h) on given rows: rows[30 (k S + s)] the 30 sums of
 * input (k, s) -- n, the 21 upper-triangle terms, sum J r (6), sum r r, sum e.e -- poses[16 K], extrinsics[16 S] and params (not NULL; only
 * refine_poses, fixed_sensor, lambda, min_input_matches and plane.min_matches matter) -> one step: updates[6 (K + S)] the float32 delta_k
 * then epsilon_s as applied (zeros where there is none), the new poses and extrinsics, the status (RGBD360_OK, RGBD360_ILL_POSED,
 * RGBD360_NO_VALID_PIXELS; the inputs are returned unchanged unless OK).  _host is the host build of the one solve text, _dev runs the
 * kernels of a call on the map's stream (k_rig_init, k_rig_input with each row as its input's only partial row, k_rig_frames,
 * k_rig_solve): the same bytes.  Any output may be NULL.  0; -1 bad arguments. */
int rgbd360_rig_calib_solve_host(const double* rows, int n_frames, int n_sensors, const float* poses, const float* extrinsics,
                                 const rgbd360_rig_calib_params* params, float* updates, float* poses_new, float* extrinsics_new, int* status);
int rgbd360_rig_calib_solve_dev(rgbd360_map* map, const double* rows, int n_frames, int n_sensors, const float* poses, const float* extrinsics,
                                const rgbd360_rig_calib_params* params, float* updates, float* poses_new, float* extrinsics_new, int* status);
/* The solve launches of one rig-calibration step under HIP events on the given rows with their gradients zeroed (the updates are then
 * exactly zero, the poses stay and every repetition solves the same system), averages over `reps` launch chains in microseconds:
 * avg_us[0] k_rig_init alone, [1] init + k_rig_input, [2] + k_rig_frames, [3] + k_rig_solve; a kernel's time is the difference of two
 * chains.  0; -1 bad arguments. */
int rgbd360_rig_calib_time_solve(rgbd360_map* map, const double* rows, int n_frames, int n_sensors, const float* poses, const float* extrinsics,
                                 const rgbd360_rig_calib_params* params, int reps, float avg_us[4]);
/* The trace of the map's last rig calibration, one record per applied step: the contributing points and sum r r of the evaluation the
 * step was solved from, the largest v.v and omega.omega over the blocks' float32 updates.  As rgbd360_map_align_batch_trace. */
int rgbd360_rig_calib_trace(rgbd360_map* map, int max_trace, int* n_trace, rgbd360_rig_calib_step* trace);
/* The alignment's kernels under HIP events on a sphere frame in device memory, averages over `reps` launches in microseconds:
 * avg_us[0] k_vmap_icp_eval, [1] k_vmap_icp_solve, [2] one k_vmap_insert launch of the frame into the map as it is (the map holds the
 * frame once more afterwards), [3] a device-to-device copy of the frame's depth bytes, [4] a whole alignment of params->max_iters
 * iterations from `pose` (enqueue to synchronisation, wall clock).  *probes (may be NULL): table slots read per point that reached the
 * search, in one evaluation at `pose`. */
int rgbd360_map_time_align(rgbd360_map* map, const void* depth_dev, size_t depth_step, int depth_type, int rows, int cols, int convention,
                           const float pose[16], const rgbd360_map_align_params* params, int reps, float avg_us[5], double* probes);

/* One evaluation of the point-to-plane alignment (rgbd360_map_align_plane_*, rgbd360_hip.h: steps 1-5 of its definition) at `pose`,
 * inputs as in rgbd360_map_align_eval.  row[30]: n, the 21 upper-triangle terms of sum J J^T row by row, sum J r (6), sum r r,
 * sum e_match . e_match; counters[5]: n_valid, n_box_rejected, n_out_of_range, n_unsupported, n_nonplanar.  DEVICE arrays per input
 * point, any may be NULL: key3_dev / d2_dev as in rgbd360_map_align_eval (the kept match whatever became of the point afterwards),
 * normal_r_dev four doubles (the normal and r as the sums take them, unrounded; zeros unless the class is 1), class_dev one byte:
 * 0 no kept match, 1 contributing, 2 unsupported, 3 nonplanar.  The trace of the last alignment, of either kind, is
 * rgbd360_map_align_eval's. */
int rgbd360_map_align_plane_eval(rgbd360_map* map, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                 const float* xyz, long long n, const float pose[16], int on_device,
                                 const rgbd360_map_align_plane_params* params, double row[30], long long counters[5], int32_t* key3_dev,
                                 float* d2_dev, double* normal_r_dev, uint8_t* class_dev);
/* Step 3 of that definition on the host (the function the kernel calls, compiled for the CPU): cov = C00, C01, C02, C11, C12, C22.
 * normal[3]; eigen[2] (may be NULL) = l0, l1.  1 planar, 0 not, -1 a NULL argument.  Needs no device. */
int rgbd360_map_plane_fit(const double cov[6], double max_flatness, double normal[3], double eigen[2]);
/* The point-to-plane kernels under HIP events on a sphere frame in device memory, averages over `reps` launches in microseconds:
 * avg_us[0] k_vmap_plane_eval, [1] k_vmap_icp_eval on the same frame, map and five shared parameters in the same run, [2]
 * k_vmap_plane_solve, [3] a whole point-to-plane alignment of params->max_iters iterations from `pose` (enqueue to synchronisation, wall
 * clock).  *probes as in rgbd360_map_time_align.  The map is not changed. */
int rgbd360_map_time_align_plane(rgbd360_map* map, const void* depth_dev, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                 const float pose[16], const rgbd360_map_align_plane_params* params, int reps, float avg_us[4], double* probes);

/* One evaluation of generalized ICP against the map (rgbd360_map_align_gicp_*, rgbd360_hip.h: steps 1-6 of its definition) at `pose`,
 * inputs as in rgbd360_map_align_plane_eval; normal: the cloud's 3 n normals where xyz is, or NULL (ignored with a depth image).
 * row[30]: n, the 21 upper-triangle terms of sum J^T M J row by row, sum J^T M e (6), sum e^T M e, sum e.e; counters[6]: n_valid,
 * n_box_rejected, n_out_of_range, n_target_planes, n_source_planes, n_plane_pairs.  DEVICE arrays per input point, any may be NULL:
 * key3_dev / d2_dev as in rgbd360_map_align_eval, weight_cost_dev seven doubles (M00 M01 M02 M11 M12 M22 and e^T M e as the sums take
 * them; zeros without a kept match), class_dev one byte: bit 0 a kept match, bit 1 a target normal was used, bit 2 a source normal. */
int rgbd360_map_align_gicp_eval(rgbd360_map* map, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                const float* xyz, const float* normal, long long n, const float pose[16], int on_device,
                                const rgbd360_map_align_gicp_params* params, double row[30], long long counters[6], int32_t* key3_dev,
                                float* d2_dev, double* weight_cost_dev, uint8_t* class_dev);
/* Steps 2-4 of that definition on the host (the function the kernel calls, compiled for the CPU): nb the target normal (has_b: the
 * voxel has one), na the source normal as passed (has_a: an array was passed), pose column-major, M = M00 M01 M02 M11 M12 M22.
 * Returns 2 x (a target normal was used) + 4 x (a source normal was used), -1 on a NULL argument.  Needs no device. */
int rgbd360_map_gicp_weight(const double nb[3], int has_b, const float na[3], int has_a, const float pose[16], float epsilon, double M[6]);
/* The kernels of the three methods under HIP events on a sphere frame in device memory, averages over `reps` launches in microseconds:
 * avg_us[0] k_vmap_gicp_eval (the normal layer built beforehand), [1] k_vmap_icp_eval and [2] k_vmap_plane_eval on the same frame, map
 * and shared parameters in the same run, [3] the solve kernel on this method's row, [4] a whole alignment of params->max_iters
 * iterations from `pose` (enqueue to synchronisation, wall clock).  *probes as in rgbd360_map_time_align.  The map is not changed. */
int rgbd360_map_time_align_gicp(rgbd360_map* map, const void* depth_dev, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                const float pose[16], const rgbd360_map_align_gicp_params* params, int reps, float avg_us[5], double* probes);

/* Steps 3-4 of the colour layer's definition (colour of the map, rgbd360_hip.h) on the host -- the function k_vmap_colour_layer runs,
 * compiled for the CPU: the voxel's float32 normal and intensity, its m neighbours in their order as r (3 m floats, the float32 centroid
 * differences) and intensity_nb (m floats).  gradient: d.  Returns RGBD360_COLOUR_OK or RGBD360_COLOUR_NO_GRADIENT, -1 on a NULL argument.
 * Needs no device. */
int rgbd360_map_colour_gradient(const float normal[3], float intensity, int m, const float* r, const float* intensity_nb, int min_gradient_support,
                                float min_spread, float gradient[3]);
/* Step 1 of that definition on the host: I64 of the colour sums of `count` points (0 when count < 1).  Needs no device. */
double rgbd360_map_colour_intensity(long long sr, long long sg, long long sb, long long count);
/* The build of the colour layer under HIP events: build_us[r], r < reps, one k_vmap_colour_layer launch over the table with the clear of
 * its counters (the normal layer standing), normals_us[r] (may be NULL) one k_vmap_normals launch likewise and scan_us[r] (may be NULL) ONE
 * k_vmap_extract launch (centroids only) over the same table, all in the same run, in microseconds (the caller takes medians); one
 * untimed build of both layers runs first.  stats (may be NULL): those of the last build; *layer_bytes (may be NULL): device memory of
 * the layer.  -1 on an empty map.  Both layers stay valid for the parameters given; the map is not changed. */
int rgbd360_map_time_colours(rgbd360_map* map, const rgbd360_map_colour_params* params, int reps, float* build_us, float* normals_us, float* scan_us,
                             rgbd360_map_colour_stats* stats, long long* layer_bytes);
/* One evaluation of coloured ICP against the map (rgbd360_map_align_colour_*, rgbd360_hip.h: steps 1-6 of its definition) at `pose`: the
 * sphere frame (rgb, depth) where depth is not NULL, otherwise the cloud (xyz, rgb3, n); host memory, or device memory with on_device.
 * row[31]: n, the 21 upper-triangle terms of H row by row, g (6), cost, sum r_G^2, sum r_C^2; counters[5]: n_valid, n_box_rejected,
 * n_out_of_range, n_no_normal, n_no_gradient.  DEVICE arrays per input point, any may be NULL: key3_dev / d2_dev as in
 * rgbd360_map_align_eval (the key of the kept match whatever the point's class), residuals_dev two doubles (r_G, r_C; zeros unless the
 * point contributes), class_dev one byte: bit 0 a kept match, bit 1 dropped for want of a normal, bit 2 it contributes with d = 0.
 * -1 without colours: a cloud's row and counters are then zeroed, an image's outputs untouched. */
int rgbd360_map_align_colour_eval(rgbd360_map* map, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step, int depth_type, int rows,
                                  int cols, int convention, const float* xyz, const uint8_t* rgb3, long long n, const float pose[16], int on_device,
                                  const rgbd360_map_align_colour_params* params, double row[31], long long counters[5], int32_t* key3_dev,
                                  float* d2_dev, double* residuals_dev, uint8_t* class_dev);
/* The coloured evaluation beside generalized ICP's under HIP events on a sphere frame in device memory, averages over `reps` launches in
 * microseconds: avg_us[0] k_vmap_colour_eval (both layers built beforehand), [1] k_vmap_gicp_eval (epsilon 1e-3, target normals) on the
 * same frame, map and shared parameters in the same run, [2] the solve kernel on this method's row, [3] a whole alignment of
 * params->max_iters iterations from `pose` (enqueue to synchronisation, wall clock).  *probes as in rgbd360_map_time_align.  The map is
 * not changed. */
int rgbd360_map_time_align_colour(rgbd360_map* map, const uint8_t* rgb_dev, size_t rgb_step, const void* depth_dev, size_t depth_step, int depth_type,
                                  int rows, int cols, int convention, const float pose[16], const rgbd360_map_align_colour_params* params, int reps,
                                  float avg_us[4], double* probes);
/* One evaluation of `method` (RGBD360_MAP_METHOD_*) in its robust form (rgbd360_hip.h, "robust kernels of the alignments against the map")
 * at `pose`, under the map's setting for the method, which must not be RGBD360_MAP_ROBUST_NONE.  The input forms are those of the four
 * evaluation entries above together: the sphere frame (depth; rgb for the colour method) where depth is not NULL, otherwise the cloud
 * (xyz, n; normal for generalized ICP, may be NULL; rgb3 for the colour method); host memory, or device memory with on_device.  params:
 * the method's own parameter struct (rgbd360_map_align_params / _plane_params / _gicp_params / _colour_params), NULL: its defaults.
 * row[40]: the whole robust row -- the method's row, counters and probe words included, as doubles, then the number of contributing points
 * and the number of them with w < 1; the words behind the method's width + 2 are zero.  w_dev (a DEVICE array, may be NULL): w per input
 * point, 0.0 for a point that does not contribute.  -1 with the outputs untouched: what the method's entry refuses, an unknown method, a
 * method whose setting is NONE. */
int rgbd360_map_align_robust_eval(rgbd360_map* map, int method, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step, int depth_type,
                                  int rows, int cols, int convention, const float* xyz, const float* normal, const uint8_t* rgb3, long long n,
                                  const float pose[16], int on_device, const void* params, double row[40], double* w_dev);
/* The robust form of `method` next to its quadratic form under HIP events on a sphere frame in device memory (rgb_dev: the colour method
 * alone), the same frame, map, buffers and parameters, the launches of the two forms alternating, averages over `reps` pairs in
 * microseconds: avg_us[0] the robust evaluation kernel, [1] the quadratic one, [2] the solve kernel on the robust row, [3] on the
 * quadratic row, [4] a whole robust alignment of params->max_iters iterations from `pose` (enqueue to synchronisation, wall clock), [5] a
 * whole quadratic one.  The map's setting for the method must not be NONE.  The map is not changed. */
int rgbd360_map_time_align_robust(rgbd360_map* map, int method, const uint8_t* rgb_dev, size_t rgb_step, const void* depth_dev, size_t depth_step,
                                  int depth_type, int rows, int cols, int convention, const float pose[16], const void* params, int reps, float avg_us[6]);

/* The pose graph's linearisation at its current poses (rgbd360_graph_*, rgbd360_hip.h): per edge r (6 doubles) and A = dr/dx_i (36
 * doubles, column-major), either may be NULL.  The graph is not changed. */
int rgbd360_graph_linearize(rgbd360_graph* g, double* r, double* A);
/* y = (H + lambda diag H) x of that linearisation through the optimiser's own kernels (edge product and per-vertex gather): x and y hold
 * 6 doubles per vertex of the graph; the entries of fixed and isolated vertices are read as 0 and written as 0. */
int rgbd360_graph_apply(rgbd360_graph* g, double lambda, const double* x, double* y);
/* The optimiser's kernels under HIP events at the current poses, averages over `reps` launches in microseconds: avg_us[0] the
 * linearisation, [1] the per-vertex assembly, [2] - [5] the four launches of a conjugate-gradient iteration (edge product, gather,
 * update, direction), [6] the trial poses, [7] chi2 at the trial poses, [8] the decision, [9] one of those launches returning at once on
 * the state word.  The poses are not changed. */
int rgbd360_graph_time_kernels(rgbd360_graph* g, int reps, float avg_us[10]);
/* The kernels of one covariance batch (rgbd360_graph_marginals of the n <= 16 vertices `vertices`, 6 n columns in lock step) under HIP
 * events at the current poses, averages over `reps` launches in microseconds: avg_us[0] the start of the columns, [1] the edge product
 * with one thread per (edge, column), [2] the same product with one thread per (edge, query) holding W for six columns, [3] - [5]
 * gather, update, direction, [6] the B^T X / adjoint / symmetrisation kernel, [7] a launch returning at once on the columns' stop words.
 * The poses are not changed. */
int rgbd360_graph_time_cov_kernels(rgbd360_graph* g, int n, const int* vertices, int reps, float avg_us[8]);

/* The render's kernels (rgbd360_map_render_*, rgbd360_hip.h) under HIP events, averages over `reps` back-to-back launches in
 * microseconds: avg_us[0] k_vmap_render_depth, [1] k_vmap_render_key, [2] k_vmap_render_resolve (all four planes), [3] the whole
 * rgbd360_map_render_sphere_dev sequence (the clears and the three passes), [4] ONE k_vmap_extract launch (centroids only) over the
 * same table: the cost of merely scanning it.  form: 0 every lane walks its own voxel's footprint, 1 a wave walks the footprints of
 * its voxels together (csrc/map_render.h).  stats (may be NULL): those of one render; *atomics (may be NULL): atomicMin operations the
 * depth pass of one render issued (the key pass issues at most as many).  Outputs go to the map's staging; the map is not changed. */
int rgbd360_map_time_render(rgbd360_map* map, int rows, int cols, const float pose[16], const rgbd360_map_render_params* params, int form,
                            int reps, float avg_us[5], rgbd360_map_render_stats* stats, long long* atomics);

/* The ray cast's traversal switch (rgbd360_map_raycast*, rgbd360_hip.h): plain != 0 selects the one-level traversal, one voxel-table
 * lookup per cell, for every later ray cast of this map; 0 (the default) the coarse layer.  The outputs are the same bits. */
int rgbd360_map_raycast_set_plain(rgbd360_map* map, int plain);
/* The ray cast under HIP events, one figure per repetition in microseconds (the caller takes medians): build_us[r] the layer build (both
 * scans, their clears and the read-back between them), cast_us[r] one traversal launch with the clear of its counters, scan_us[r] (may
 * be NULL) ONE k_vmap_extract launch (centroids only) over the same table, the cost of merely scanning it.  origins_dev NULL: the
 * panorama of rows x cols at pose; else the n rays of the two device arrays.  plain: as above, for this call only.  stats (may be
 * NULL): those of the last launch; *layer_bytes (may be NULL): device memory of the layer.  The map is not changed. */
int rgbd360_map_time_raycast(rgbd360_map* map, long long n, const float* origins_dev, const float* dirs_dev, int rows, int cols, const float pose[16],
                             const rgbd360_map_raycast_params* params, int plain, int reps, float* build_us, float* cast_us, float* scan_us,
                             rgbd360_map_raycast_stats* stats, long long* layer_bytes);
/* How k_depth_train adds a lane's three terms (rgbd360_depth_trainer_accumulate_*, rgbd360_hip.h; csrc/depth_train.h), for every later
 * call of this trainer: 0 plain per-lane 64-bit atomics, 1 the lanes of equal bin merged over the wave and one atomic per bin and word,
 * 2 (the default: the fastest, profiles/depth_train_perf.txt) a per-block LDS table flushed once per touched word.  The sums are the
 * same bits. */
int rgbd360_depth_trainer_set_form(rgbd360_depth_trainer* trainer, int form);
/* The map route's kernel under HIP events, one figure per repetition in microseconds (the caller takes medians): train_us[form * reps + r]
 * one k_depth_train launch in form 0, 1, 2 with the clear of its counters over the device image meas_dev of the trainer's size, cast_us[r]
 * one launch of the surface cast (k_vmap_raycast<.., SURFACE>; depth, normal and status planes) over the n = rows cols rays of the two
 * device arrays, which the caller forms by the map route's definition.  stats (may be NULL): those of the last k_depth_train launch.  The
 * trainer's sums are put back as they were; the map is not changed. */
int rgbd360_depth_trainer_time_map(rgbd360_depth_trainer* trainer, rgbd360_map* map, const void* meas_dev, size_t meas_step, int depth_type, float fx,
                                   float fy, float cx, float cy, const float sensor_pose[16], const rgbd360_depth_train_params* params,
                                   const float* origins_dev, const float* dirs_dev, int reps, float* train_us, float* cast_us,
                                   rgbd360_depth_train_stats* stats);
/* The packed, pointer-free form of a rig's depth models that rgbd360_depth_models_create keeps on the device (rgbd360_hip.h, "applying
 * the depth models on the device"; csrc/depth_apply.h) and the per-pixel text over it run on the CPU.  Host only, no context, no device.
 *   pack:    models[n_sensors], a NULL entry: identity.  blob NULL: *bytes = the size needed; else *bytes is the room of blob and, on
 *            return, the size written.  -1: what rgbd360_depth_models_create refuses, or too little room.
 *   repack:  old_blob with `sensor` replaced by model (NULL: identity), as rgbd360_depth_models_set does; the other sections are copied.
 *   undistort_packed_host: rgbd360_depth_model_undistort over the blob -- the SAME __host__ __device__ function the kernels call, so the
 *            packing and the arithmetic are checked without a GPU.  In place; a sensor with a model needs an image of the set's size. */
int rgbd360_depth_models_pack(const rgbd360_depth_model* const* models, int n_sensors, void* blob, size_t* bytes);
int rgbd360_depth_models_repack(const void* old_blob, int sensor, const rgbd360_depth_model* model, void* blob, size_t* bytes);
int rgbd360_depth_models_undistort_packed_host(const void* blob, int sensor, float* depth_m, size_t depth_step, int rows, int cols);
/* The kernel of a rgbd360_depth_undistort, rgbd360_rig_depth_clouds or rgbd360_depth_evaluate_map call (the last with the clear of its
 * counters) under HIP events: timing(ctx, 1) makes every such call of the context record an event in front of and behind its launch,
 * last_us gives the microseconds of the last one (-1 without a timed call).  time_copy: a device-to-device copy of `bytes` on the
 * context's stream between the same events, the yardstick of the stand-alone undistort (tools/depth_apply_perf.py). */
int rgbd360_depth_apply_timing(rgbd360_ctx* ctx, int on);
int rgbd360_depth_apply_last_us(rgbd360_ctx* ctx, float* us);
int rgbd360_depth_apply_time_copy(rgbd360_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes, float* us);
/* An observation (rgbd360_map_observe_sphere, rgbd360_hip.h) under HIP events, one figure per repetition in microseconds (the caller takes
 * medians): observe_us[r] one k_vmap_observe launch over the device image with the clear of its counters, on zeroed votes (the coarse
 * layer is built before the first); carve_us[r] (may be NULL) ONE k_vmap_carve launch over the table with thresholds that no voxel meets:
 * the carve's scan, the table unchanged.  plain: the one-level traversal, for this call only.  stats (may be NULL): those of the last
 * launch.  The votes of the last repetition stay with the map. */
int rgbd360_map_time_observe(rgbd360_map* map, const void* depth_dev, size_t depth_step, int depth_type, int rows, int cols, int convention,
                             const float pose[16], const rgbd360_map_observe_params* params, int plain, int reps, float* observe_us, float* carve_us,
                             rgbd360_map_observe_stats* stats);
/* The build of the normal layer (rgbd360_map_normals, rgbd360_hip.h) under HIP events: build_us[r], r < reps, one k_vmap_normals launch over
 * the table with the clear of its counters, in microseconds (the caller takes medians); one untimed build runs first.  scan_us[r] (may
 * be NULL): ONE k_vmap_extract launch (centroids only) over the same table, the cost of merely scanning it.  stats (may be NULL): those
 * of the last build; *layer_bytes (may be NULL): device memory of the layer.  -1 on an empty map.  The layer stays valid
 * for the parameters given; the map is not changed. */
int rgbd360_map_time_normals(rgbd360_map* map, const rgbd360_map_normal_params* params, int reps, float* build_us, float* scan_us,
                             rgbd360_map_normal_stats* stats, long long* layer_bytes);

/* A plane record from a region's sums on the host (planar regions of the map, rgbd360_hip.h; the function rgbd360_map_planes calls): N
 * member voxels, P points, the root's centroid, sums[9] = the three sums of q_k then those of q_x q_x, q_x q_y, q_x q_z, q_y q_y, q_y q_z,
 * q_z q_z.  plane: centroid, normal (facing viewpoint; NULL: the origin), d, curvature, count = P, root = 0, elongation, ppal_dir,
 * area_moment, area = area_moment, center_hull = centroid, no hull and no colour.  0, or -1 on a NULL argument or N < 1.  Needs no device. */
int rgbd360_map_plane_from_sums(long long n_voxels, long long n_points, const float root_centroid[3], const long long sums[9],
                                const float viewpoint[3], rgbd360_plane* plane);
/* The same with the hull: member_xyz (3 floats) and member_key3 (3 ints) of the region's n_voxels members, in any order.  The extremes
 * are taken on the host, operation for operation as the device takes them, so the record is byte for byte the one rgbd360_map_planes
 * returns for that region (but for `root`, 0 here).  Needs no device. */
int rgbd360_map_plane_from_members(long long n_voxels, long long n_points, const float root_centroid[3], const long long sums[9],
                                   const float* member_xyz, const int32_t* member_key3, const float viewpoint[3], rgbd360_plane* plane);
/* The range rule of a region's sums: 1 iff n_voxels ((extent_cells + 2) (double)leaf 2^16)^2 < 2^62 in float64, else 0.  Needs no device. */
int rgbd360_map_plane_sums_in_range(long long n_voxels, long long extent_cells, float leaf);
/* The build of the planar segmentation (rgbd360_map_planes) under HIP events: stage_us[8 r + k], r < reps, the stages of rebuild r in
 * microseconds -- 0 the clear of the layer (k_vmap_pl_init), 1 k_vmap_pl_link, 2 k_vmap_pl_compress, 3 k_vmap_pl_count, 4
 * k_vmap_pl_roots, 5 k_vmap_pl_sums, 6 k_vmap_pl_scatter, 7 k_vmap_pl_extremes; the host work between them is not in any of them.  One
 * untimed build runs first; the normal layer is built before and is not part of the stages.  merge_waves: 1 the sums pass as shipped (a
 * wave whose members share one region adds once), 0 every lane adds on its own.  stats (may be NULL): those of the last build.  -1 on
 * an empty map.  The map is not changed. */
int rgbd360_map_time_planes(rgbd360_map* map, const rgbd360_map_plane_seg_params* params, int reps, int merge_waves, float* stage_us,
                            rgbd360_map_plane_seg_stats* stats);

/* The build of the map pyramid (rgbd360_map_level, rgbd360_hip.h) under HIP events, averages over `reps` in microseconds: avg_us[s - 1],
 * 1 <= s <= top_shift, the build of level s out of level s - 1 (the clear of its table and of the counters, one k_vmap_coarsen launch);
 * avg_us[6] the builds of levels 1 .. top_shift back to back; avg_us[7] ONE k_vmap_extract launch (centroids only) over the parent's
 * table, the cost of merely scanning it.  Entries of levels above top_shift are 0.  counters (may be NULL): per level s four words at
 * 4 (s - 1): live slots read, voxels created, points carried, voxels dropped.  Levels 1 .. top_shift are refreshed first (untimed) and
 * are valid afterwards; the map is not changed. */
int rgbd360_map_time_coarsen(rgbd360_map* map, int top_shift, int reps, float avg_us[8], long long* counters);

/* The merge kernel (rgbd360_map_merge / _unmerge, rgbd360_hip.h) under HIP events, averages over `reps` in microseconds per launch, each
 * with the clear of its counters: avg_us[0] src merged into an EMPTY scratch table of dst's size, leaf and fill state (every destination
 * voxel is claimed), avg_us[1] merged into it a second time (every destination voxel is found), avg_us[2] one of the two taken off
 * again (the un-merge kernel), avg_us[3] ONE k_vmap_extract launch (centroids only) over src's table, the cost of merely scanning it.
 * pose as for rgbd360_map_merge (NULL: sum mode).  The scratch table goes when the call returns; neither map is changed.  Refusals as
 * for rgbd360_map_merge. */
int rgbd360_map_time_merge(rgbd360_map* dst, rgbd360_map* src, const float pose[16], int reps, float* avg_us);

/* The same timer with the launches rotating over n_ctx contexts of one device (each with its own copy of a frame pair) on
 * ctxs[0]'s stream: once n_ctx x the level's working set exceeds the 256 MiB Infinity Cache every launch is fed from HBM. */
int rgbd360_time_eval_kernel_rotating(rgbd360_ctx* const* ctxs, int n_ctx, int level, const float pose[16], int method,
                                      int want_hg, int reps, float* avg_us);

/* Same for the solve launch (mode 0: reduction + Gauss-Newton step, forced; mode 1: reduction only), re-using the
 * partials of the last pass. */
int rgbd360_time_solve_kernel(rgbd360_ctx* ctx, int level, int mode, int reps, float* avg_us);

/* Device self-test of the correctly rounded sqrt / reciprocal sequences the warp front end uses: compares them
 * with the compiler's IEEE sqrtf and 1.f/x for the `count` float bit patterns starting at `first_bits`;
 * mismatches[0] = sqrt, mismatches[1] = reciprocal, mismatches[2] = the round-half-up float->int conversion
 * against floor((double)x + 0.5) for |x| < 1e9 (both signs). */
/* Test hooks: the alternative schedules the parity tests hold against the default ones (poses, iteration counts and status must be
 * bit-identical).  fused_solve 0: every Gauss-Newton iteration as a {k_eval, k_solve} launch pair instead of one k_eval_fs launch;
 * fused_occ 0: the occlusion-aware iterations as {k_occ_build, k_eval_occ, k_solve} triples.  Not while an alignment is in flight. */
int rgbd360_debug_set_schedule(rgbd360_ctx* ctx, int fused_solve, int fused_occ);
/* route 1: rgbd360_align360_batch runs every sequence over the per-context route (one context per sub-chunk of pairs; what the
 * occlusion-aware sequences always use) with at most max_contexts contexts (0: the default cap); route 0: the lock-step engines. */
int rgbd360_debug_set_sequence_route(rgbd360_ctx* ctx, int route, int max_contexts);
/* 1 when the library was built with -DRGBD360_DEBUG_KNOBS (csrc/knobs.h: it then reads the A/B environment variables of the measurement tools) */
int rgbd360_debug_knobs_enabled(void);

/* Stage times of rgbd360_frame_planes[_dev], measured with HIP events ON THE CONTEXT'S STREAM at the stage
 * boundaries: us[0] the kernel that forms the organised cloud (and the depth-change mask) = a13, us[1] distance map + normal map = a14,
 * us[2] plane stage (link flags ... hull records, colour when an image is registered) = a15.  _stage_timing(ctx, 1) arms the context's
 * later calls (four event records per call), _stage_times reads the last call's.  With the refinement on, a15 ends at the last kernel in
 * front of the refinement (the refinement synchronises with the host).  bench.py's `roofline_frame360` block. */
int rgbd360_frame_planes_stage_timing(rgbd360_ctx* ctx, int on);
int rgbd360_frame_planes_stage_times(rgbd360_ctx* ctx, float us[3]);

/* The per-region records the host turned into the plane records of the context's last plane call (rgbd360_plane_fit,
 * _frame_planes[_dev], _cloud_planes, _sensor_planes), after the refinement's commit when the refinement is on: region slot s (the
 * order the device assigned, not PCL's) has root pixel root[s], count[s] points and the nine exact sums mom[9 s + 0 .. 8] =
 * sum x, y, z, xx, xy, xz, yy, yz, zz in units of 2^-28 m (m^2), each term rounded to the unit (half to even), two's complement.
 * Every region that exceeded min_inliers is listed, also those the curvature filter dropped.  *n = number of regions (at most 4096; 0
 * before the first plane call), of which the first `max` are copied; root / count / mom may be NULL.  Copies host memory only. */
int rgbd360_debug_plane_sums(rgbd360_ctx* ctx, int max, int* n, int32_t* root, int32_t* count, int64_t* mom);

/* The target pixel of every source pixel of every sensor of an 8-sensor rig at rig pose `pose` on `level`, in the rig's current
 * arithmetic (rgbd360_rig_set_index_arithmetic) -- the warp k_eval_rig runs.  chain 0: the error pass's (calcPhotoICPError_robot),
 * 1: the H / g pass's (calcHessianGradient_robot); in the device definition (mode 0) both are the same.  out: [S][rows * cols][2]
 * int32 (row, col), the convention of rgbd360_warp_indices_pinhole: (-1, -1) for a source pixel without a valid point (depth outside
 * (min_depth, max_depth)) and for a projection outside the image or not finite.  The saliency list is not applied.  Needs the
 * source frame only. */
int rgbd360_rig_warp_indices(rgbd360_rig* rig, int level, const float pose[16], int chain, int32_t* out);

int rgbd360_selftest_math(rgbd360_ctx* ctx, uint32_t first_bits, uint32_t count, unsigned long long mismatches[3]);
/* csrc/libm_f32.h (asinf / atanf / roundf / atan2f restated operation for operation, what rgbd360_set_index_arithmetic(ctx, 1) computes
 * with) as the DEVICE evaluates it, against the C library of this process: the floats first_bits .. first_bits + count - 1 through the
 * one-argument functions (asinf where |x| <= 1.5), `count` drawn pairs through atan2f.  mismatches[4] = {asinf, atanf, roundf, atan2f}. */
int rgbd360_selftest_libm(rgbd360_ctx* ctx, uint32_t first_bits, uint32_t count, unsigned long long mismatches[4]);

#ifdef __cplusplus
}
#endif
#endif /* RGBD360_HIP_DIAG_H */
