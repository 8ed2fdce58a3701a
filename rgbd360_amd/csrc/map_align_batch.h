// map_align_batch.h -- many alignments against the resident voxel map in lock step: n_inputs clouds, or sphere frames of one geometry,
// and n_jobs jobs (input, guess), every job the single call rgbd360_map_align_* / rgbd360_map_align_plane_* of its input from its guess,
// byte for byte (pose, result struct, trace), whatever else is in the batch.  Relocalisation from a lattice of guesses, the keyframes of a
// window after a pose-graph correction, the eight clouds of a rig: small inputs that, one call each, leave a few workgroups on the GPU and
// pay a synchronisation apiece.  Part of the Frame360 translation unit, behind map_align.h and map_align_plane.h.
//
// Definition (include/rgbd360_hip.h, "many alignments against the map in lock step").  The driver is written over the
// method description M as icp_enqueue<M> is (map_align.h), the batched evaluation launch (batch_launch_eval<M>) included.  Point-to-point
// and point-to-plane are instantiated.
//
//   BatchJob                     a job in device memory: its Source, its guess, its own grid extent (tiles per image row, workgroups), its
//                                LoopState and trace, its slice of the partial rows.  Next to the jobs the exclusive prefix of their
//                                workgroup counts.
//   k_vmap_icp_init_batch        one 64-lane workgroup per job: icp_init_state, as k_vmap_icp_init, on the job's state from the job's guess.
//   k_vmap_eval_batch<M, SRC>    ONE flat launch over the workgroups of all jobs.  A workgroup finds its job by bisection of the prefix
//                                table (at most 10 steps for 1024 jobs, the same in every lane), returns before any other load when the job
//                                has ended, and evaluates tile (local % gx, local / gx) of the job's source at the job's pose with
//                                eval_tile<M, SRC, false>, the function k_vmap_eval calls, into row `local` of the job's slice: the row
//                                vmap::block_row gives under the job's own grid.  Clouds of one batch may differ in size 100-fold: a
//                                grid.z per job over the largest grid would launch mostly empty workgroups.
//   k_vmap_icp_solve_batch<Row>  one 64-lane workgroup per job: icp_solve_rows<Row>, the function k_vmap_icp_solve calls, on the job's
//                                state, rows (ascending) and trace.  The same rows added in the same order: the sums of the single call.
//   host                         one init, max_iters x (eval, solve), the final pass, one copy of all states and traces, ONE
//                                synchronisation: 2 max_iters + 3 launches whatever n_jobs is.  Host inputs go up packed into the map's
//                                upload buffer at 256-byte aligned offsets, each once however many jobs use it.
// No floating-point atomics, no inline assembly; contraction is off as in the single kernels.
#pragma once

namespace vmap {

struct BatchJob {
    Source src;
    float guess[16];
    void* state;                         // LoopState<WORDS> of the method
    rgbd360_map_align_trace* trace;
    double* part;                        // the job's slice of the partial rows: n_rows rows
    unsigned gx, n_rows;                 // the job's own grid: tiles per image row (a cloud: its tiles), workgroups
};

// the job of workgroup wg: the last j with prefix[j] <= wg (prefix[0] = 0, prefix[n_jobs] = the launch's workgroups > wg)
__device__ __forceinline__ int batch_job_of(const unsigned* __restrict__ prefix, int n_jobs, unsigned wg) {
    int lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= wg) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <int WORDS>
__global__ __launch_bounds__(64) void k_vmap_icp_init_batch(const BatchJob* __restrict__ jobs) {
    const BatchJob& job = jobs[blockIdx.x];
    icp_init_state(static_cast<LoopState<WORDS>*>(job.state), job.guess);
}

// (no per-point outputs in a batch: the pointers of c and a are null and not looked at)
template <class M, int SRC>
__global__ __launch_bounds__(kThreads) void k_vmap_eval_batch(Params P, const BatchJob* __restrict__ jobs, const unsigned* __restrict__ prefix, int n_jobs,
                                                              EvalCommon c, typename M::Args a, int final_pass) {
#pragma clang fp contract(off)
    const int j = batch_job_of(prefix, n_jobs, blockIdx.x);
    const BatchJob& job = jobs[j];
    const LoopState<M::kWords>* st = static_cast<const LoopState<M::kWords>*>(job.state);
    if (!final_pass && st->done) return;
    __shared__ double s_red[kThreads / 64][M::kWords];
#pragma unroll
    for (int k = 0; k < 16; ++k) P.pose[k] = st->pose[k];
    const Source src = job.src;
    const unsigned local = blockIdx.x - prefix[j], gx = job.gx;
    const unsigned bx = SRC == 0 ? local % gx : local, by = SRC == 0 ? local / gx : 0u;
    eval_tile<M, SRC, false>(P, src, bx, by, c, a, s_red, job.part + (size_t)local * M::kWords);
}

template <class M>
__global__ __launch_bounds__(64) void k_vmap_icp_solve_batch(const BatchJob* __restrict__ jobs, int final_pass, long long min_matches, float eps) {
    const BatchJob& job = jobs[blockIdx.x];
    LoopState<M::kWords>* const st = static_cast<LoopState<M::kWords>*>(job.state);
    if (!final_pass && st->done) return;
    __shared__ double s_row[M::kWords];
    icp_solve_rows<M>(st, job.trace, job.part, (int)job.n_rows, final_pass, min_matches, eps, s_row);
}

}  // namespace vmap

namespace {

// the bounds of a batch (RGBD360_MAP_BATCH_MAX, _MAX_ROWS, _MAX_UPLOAD of the public header)
constexpr long long kBatchMaxRows = RGBD360_MAP_BATCH_MAX_ROWS;
constexpr unsigned long long kBatchMaxUpload = RGBD360_MAP_BATCH_MAX_UPLOAD;

// what a launch of the batched kernels takes besides the method's parameters
struct BatchLaunch {
    const vmap::BatchJob* jobs;
    const unsigned* prefix;
    int n_jobs;                  // the jobs on the device: those of non-empty inputs
    unsigned n_rows;             // the workgroups of all of them
    bool cloud;
};

// the batched evaluation launch of method M: icp_launch_eval's preparation, no per-point outputs
template <class M>
int batch_launch_eval(rgbd360_map* m, const IcpJob& job, const BatchLaunch& b, const vmap::Params& P, int final_pass) {
    typename M::Args a{};
    if (const int rc = M::eval_args(m, job, typename M::Out{}, a)) return rc;
    const vmap::EvalCommon c = icp_common(m, job, nullptr, nullptr);
    with_choice<0, 1>(b.cloud, [&](auto S) {
        hipLaunchKernelGGL((vmap::k_vmap_eval_batch<typename M::Row, decltype(S)::value>), dim3(b.n_rows), dim3(vmap::kThreads), 0, m->s->stream, P, b.jobs, b.prefix,
                           b.n_jobs, c, a, final_pass);
    });
    HIPC(m, hipGetLastError());
    return 0;
}

size_t batch_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// A batch of method M: everything is checked before anything is launched, uploaded or allocated; then the schedule of the header comment.
template <class M>
int icp_align_batch(rgbd360_map* m, const std::vector<MapInput>& inputs, const rgbd360_map_batch_job* jobs, int n_jobs, const typename M::Params* params,
                    float* poses_out, typename M::Result* results) {
    using State = IcpState<M>;
    IcpJob base;
    if (const int rc = M::check(m, params, base)) return rc;
    if (!jobs || !poses_out) return vmap_fail(m, -1, "jobs and poses_out must not be null");
    if (n_jobs < 1 || n_jobs > RGBD360_MAP_BATCH_MAX) return vmap_fail(m, -1, "n_jobs must lie in 1 .. RGBD360_MAP_BATCH_MAX");
    const int n_inputs = (int)inputs.size();
    const bool cloud = inputs[0].cloud;
    std::vector<unsigned long long> rows_of(n_inputs, 0), bytes_of(n_inputs, 0);      // workgroups per job of the input; packed bytes (0: empty)
    std::vector<unsigned> gx_of(n_inputs, 0);
    for (int i = 0; i < n_inputs; ++i) {
        const MapInput& in = inputs[i];
        const int chk = vmap_check(m, in, true);
        if (chk < 0) return chk;
        if (chk == 1) continue;
        if (cloud) {
            rows_of[i] = (unsigned long long)((in.n + vmap::kTile - 1) / vmap::kTile);
            bytes_of[i] = (unsigned long long)in.n * 3 * sizeof(float);
        } else {
            gx_of[i] = (unsigned)((in.cols + vmap::kTile - 1) / vmap::kTile);
            rows_of[i] = (unsigned long long)gx_of[i] * (unsigned long long)in.rows;
            bytes_of[i] = (unsigned long long)in.cols * (in.depth_type == 0 ? 2 : 4) * (unsigned long long)in.rows;
        }
        if (rows_of[i] > (unsigned long long)kBatchMaxRows) return vmap_fail(m, -1, "an input of the batch needs more than RGBD360_MAP_BATCH_MAX_ROWS workgroups");
        if (cloud) gx_of[i] = (unsigned)rows_of[i];
    }
    std::vector<char> used(n_inputs, 0);
    std::vector<int> live;               // the jobs that run: those of non-empty inputs, in the batch's order
    unsigned long long total_rows = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int i = jobs[j].input;
        if (i < 0 || i >= n_inputs) return vmap_fail(m, -1, "a job's input index is out of range");
        if (rows_of[i] == 0) continue;
        used[i] = 1;
        live.push_back(j);
        total_rows += rows_of[i];
    }
    if (total_rows > (unsigned long long)kBatchMaxRows) return vmap_fail(m, -1, "the jobs of the batch need more than RGBD360_MAP_BATCH_MAX_ROWS workgroups");
    std::vector<size_t> offset_of(n_inputs, 0);
    unsigned long long upload = 0;
    for (int i = 0; i < n_inputs && !inputs[0].on_device; ++i) {
        if (!used[i]) continue;
        offset_of[i] = (size_t)upload;
        upload = batch_align256((size_t)(upload + bytes_of[i]));
        if (upload > kBatchMaxUpload) return vmap_fail(m, -1, "the host inputs of the batch exceed RGBD360_MAP_BATCH_MAX_UPLOAD bytes");
    }

    // the batch runs from here on
    m->a_trace.clear();
    m->b_trace.assign((size_t)n_jobs, {});
    const double no_row[M::kWords] = {};     // (a job of an empty input: nothing contributed)
    m->b_robust.assign((size_t)n_jobs, icp_robust_info<M>(base, no_row));
    for (int j = 0; j < n_jobs; ++j) {       // a job of an empty input: the single call's answer; the others are overwritten below
        if (rows_of[jobs[j].input] != 0) continue;
        memcpy(poses_out + 16 * (size_t)j, jobs[j].guess, 16 * sizeof(float));
        if (results) {
            memset(&results[j], 0, sizeof(results[j]));
            results[j].status = RGBD360_NO_VALID_PIXELS;
        }
    }
    const int n_live = (int)live.size();
    if (n_live == 0) return 0;

    hipSetDevice(m->s->p.device);
    hipStream_t stream = m->s->stream;
    const int iters = base.p.max_iters;
    const size_t state_stride = sizeof(State) + (size_t)std::max(iters, 1) * sizeof(rgbd360_map_align_trace);
    static_assert(sizeof(State) % 8 == 0 && sizeof(rgbd360_map_align_trace) % 8 == 0 && sizeof(vmap::BatchJob) % 8 == 0, "states, traces and jobs stay 8-byte aligned");
    const size_t desc_bytes = (size_t)n_live * sizeof(vmap::BatchJob) + ((size_t)n_live + 1) * sizeof(unsigned);
    HIPC(m, m->a_part.ensure((size_t)total_rows * vmap::kIcpMaxWords));
    HIPC(m, m->a_state.ensure((size_t)n_live * state_stride));
    HIPC(m, m->a_host.ensure((size_t)n_live * state_stride));
    HIPC(m, m->b_desc.ensure(desc_bytes));
    HIPC(m, m->b_desc_host.ensure(desc_bytes));
    if (upload) HIPC(m, m->up_depth.ensure((size_t)upload));
    const float* tab = nullptr;
    if (!cloud) {
        if (const int rc = sphere_tables_dev(m->s, inputs[0].rows, inputs[0].cols, inputs[0].convention)) {
            m->err = m->s->err;
            return rc;
        }
        tab = m->s->f_tab;
    }
    // the inputs as the kernels take them, a host input uploaded once
    std::vector<vmap::Source> source(n_inputs);
    for (int i = 0; i < n_inputs; ++i) {
        if (!used[i]) continue;
        const MapInput& in = inputs[i];
        const void* points = cloud ? (const void*)in.xyz : in.depth;
        size_t pstep = in.depth_step;
        if (!in.on_device) {
            uint8_t* dst = m->up_depth.get() + offset_of[i];
            if (cloud) {
                HIPC(m, hipMemcpyAsync(dst, points, (size_t)bytes_of[i], hipMemcpyHostToDevice, stream));
            } else {
                const size_t prow = (size_t)in.cols * (in.depth_type == 0 ? 2 : 4);
                HIPC(m, hipMemcpy2DAsync(dst, prow, points, pstep, prow, (size_t)in.rows, hipMemcpyHostToDevice, stream));
                pstep = prow;
            }
            points = dst;
        }
        if (cloud) source[i] = {nullptr, 0, nullptr, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, static_cast<const float*>(points), in.n};
        else
            source[i] = {points, pstep, nullptr, 0, in.depth_type, in.rows, in.cols, in.convention, tab, tab + in.cols, tab + 2 * in.cols, tab + 2 * in.cols + in.rows,
                         nullptr, 0};
    }
    // the jobs and the prefix of their workgroup counts
    vmap::BatchJob* hj = reinterpret_cast<vmap::BatchJob*>(m->b_desc_host.get());
    unsigned* hp = reinterpret_cast<unsigned*>(m->b_desc_host.get() + (size_t)n_live * sizeof(vmap::BatchJob));
    unsigned at = 0;
    for (int k = 0; k < n_live; ++k) {
        const rgbd360_map_batch_job& job = jobs[live[k]];
        vmap::BatchJob& d = hj[k];
        d.src = source[job.input];
        memcpy(d.guess, job.guess, sizeof(d.guess));
        unsigned char* st = m->a_state.get() + (size_t)k * state_stride;
        d.state = st;
        d.trace = reinterpret_cast<rgbd360_map_align_trace*>(st + sizeof(State));
        d.part = m->a_part.get() + (size_t)at * M::kWords;
        d.gx = gx_of[job.input];
        d.n_rows = (unsigned)rows_of[job.input];
        hp[k] = at;
        at += d.n_rows;
    }
    hp[n_live] = at;
    HIPC(m, hipMemcpyAsync(m->b_desc, m->b_desc_host, desc_bytes, hipMemcpyHostToDevice, stream));
    const BatchLaunch b = {reinterpret_cast<const vmap::BatchJob*>(m->b_desc.get()),
                           reinterpret_cast<const unsigned*>(m->b_desc.get() + (size_t)n_live * sizeof(vmap::BatchJob)), n_live, at, cloud};
    const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const vmap::Params P = vmap_params(m, eye);      // (the pose of a job comes from its state)

    hipLaunchKernelGGL((vmap::k_vmap_icp_init_batch<M::kWords>), dim3(n_live), dim3(64), 0, stream, b.jobs);
    HIPC(m, hipGetLastError());
    for (int it = 0; it <= iters; ++it) {
        const int final_pass = it == iters ? 1 : 0;
        if (const int rc = batch_launch_eval<M>(m, base, b, P, final_pass)) return rc;
        hipLaunchKernelGGL((vmap::k_vmap_icp_solve_batch<typename M::Row>), dim3(n_live), dim3(64), 0, stream, b.jobs, final_pass, base.p.min_matches, base.p.eps);
        HIPC(m, hipGetLastError());
    }
    HIPC(m, hipMemcpyAsync(m->a_host, m->a_state, (size_t)n_live * state_stride, hipMemcpyDeviceToHost, stream));
    HIPC(m, hipStreamSynchronize(stream));

    for (int k = 0; k < n_live; ++k) {
        const int j = live[k];
        const unsigned char* base_k = m->a_host.get() + (size_t)k * state_stride;
        const State& st = *reinterpret_cast<const State*>(base_k);
        const rgbd360_map_align_trace* tr = reinterpret_cast<const rgbd360_map_align_trace*>(base_k + sizeof(State));
        m->b_trace[j].assign(tr, tr + st.iterations);
        memcpy(poses_out + 16 * (size_t)j, st.pose, 16 * sizeof(float));
        if (results) icp_fill_result<M>(st, &results[j]);
        m->b_robust[j] = icp_robust_info<M>(base, st.row);
    }
    return 0;
}

// the inputs of the batch entries as MapInputs; -1 with a message for a bad count or a null array
int batch_count(rgbd360_map* m, const void* inputs, int n_inputs) {
    if (n_inputs < 1 || n_inputs > RGBD360_MAP_BATCH_MAX) return vmap_fail(m, -1, "n_inputs must lie in 1 .. RGBD360_MAP_BATCH_MAX");
    return inputs ? 0 : vmap_fail(m, -1, "inputs must not be null");
}
template <class M>
int batch_clouds(rgbd360_map* m, const rgbd360_map_batch_cloud* inputs, int n_inputs, int on_device, const rgbd360_map_batch_job* jobs, int n_jobs,
                 const typename M::Params* params, float* poses_out, typename M::Result* results) {
    if (!m) return -1;
    m->err.clear();
    if (const int rc = batch_count(m, inputs, n_inputs)) return rc;
    std::vector<MapInput> in((size_t)n_inputs);
    for (int i = 0; i < n_inputs; ++i) in[i] = cloud_input(inputs[i].xyz, nullptr, inputs[i].n, on_device);
    return icp_align_batch<M>(m, in, jobs, n_jobs, params, poses_out, results);
}
template <class M>
int batch_frames(rgbd360_map* m, const rgbd360_map_batch_frame* inputs, int n_inputs, int depth_type, int rows, int cols, int convention, int on_device,
                 const rgbd360_map_batch_job* jobs, int n_jobs, const typename M::Params* params, float* poses_out, typename M::Result* results) {
    if (!m) return -1;
    m->err.clear();
    if (const int rc = batch_count(m, inputs, n_inputs)) return rc;
    std::vector<MapInput> in((size_t)n_inputs);
    for (int i = 0; i < n_inputs; ++i) in[i] = sphere_input(nullptr, 0, inputs[i].depth, inputs[i].depth_step, depth_type, rows, cols, convention, on_device);
    return icp_align_batch<M>(m, in, jobs, n_jobs, params, poses_out, results);
}

// the winner among the jobs of one input: an inlier count, not part of the alignment
template <class R>
int batch_best(const R* results, int n, long long min_matched) {
    int best = -1;
    for (int i = 0; results && i < n; ++i) {
        const R& r = results[i];
        if (r.status != RGBD360_OK || r.n_matched < min_matched) continue;
        if (best < 0 || r.n_matched > results[best].n_matched || (r.n_matched == results[best].n_matched && r.fitness < results[best].fitness)) best = i;
    }
    return best;
}
}  // namespace

extern "C" int rgbd360_map_align_batch_cloud(rgbd360_map* m, const rgbd360_map_batch_cloud* inputs, int n_inputs, int on_device,
                                             const rgbd360_map_batch_job* jobs, int n_jobs, const rgbd360_map_align_params* params, float* poses_out,
                                             rgbd360_map_align_result* results) {
    return icp_by_setting<PointIcp>(m, [&](auto M) {
        return batch_clouds<typename decltype(M)::type>(m, inputs, n_inputs, on_device, jobs, n_jobs, params, poses_out, results);
    });
}
extern "C" int rgbd360_map_align_batch_sphere(rgbd360_map* m, const rgbd360_map_batch_frame* inputs, int n_inputs, int depth_type, int rows, int cols,
                                              int convention, int on_device, const rgbd360_map_batch_job* jobs, int n_jobs,
                                              const rgbd360_map_align_params* params, float* poses_out, rgbd360_map_align_result* results) {
    return icp_by_setting<PointIcp>(m, [&](auto M) {
        return batch_frames<typename decltype(M)::type>(m, inputs, n_inputs, depth_type, rows, cols, convention, on_device, jobs, n_jobs, params, poses_out, results);
    });
}
extern "C" int rgbd360_map_align_plane_batch_cloud(rgbd360_map* m, const rgbd360_map_batch_cloud* inputs, int n_inputs, int on_device,
                                                   const rgbd360_map_batch_job* jobs, int n_jobs, const rgbd360_map_align_plane_params* params,
                                                   float* poses_out, rgbd360_map_align_plane_result* results) {
    return icp_by_setting<PlaneIcp>(m, [&](auto M) {
        return batch_clouds<typename decltype(M)::type>(m, inputs, n_inputs, on_device, jobs, n_jobs, params, poses_out, results);
    });
}
extern "C" int rgbd360_map_align_plane_batch_sphere(rgbd360_map* m, const rgbd360_map_batch_frame* inputs, int n_inputs, int depth_type, int rows, int cols,
                                                    int convention, int on_device, const rgbd360_map_batch_job* jobs, int n_jobs,
                                                    const rgbd360_map_align_plane_params* params, float* poses_out,
                                                    rgbd360_map_align_plane_result* results) {
    return icp_by_setting<PlaneIcp>(m, [&](auto M) {
        return batch_frames<typename decltype(M)::type>(m, inputs, n_inputs, depth_type, rows, cols, convention, on_device, jobs, n_jobs, params, poses_out, results);
    });
}
extern "C" int rgbd360_map_align_best(const rgbd360_map_align_result* results, int n, long long min_matched) { return batch_best(results, n, min_matched); }
extern "C" int rgbd360_map_align_plane_best(const rgbd360_map_align_plane_result* results, int n, long long min_matched) {
    return batch_best(results, n, min_matched);
}

// measurement and tests (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_align_batch_trace(rgbd360_map* m, int job, int max_trace, int* n_trace, rgbd360_map_align_trace* trace) {
    if (!m) return -1;
    m->err.clear();
    if (job < 0 || job >= (int)m->b_trace.size()) return vmap_fail(m, -1, "no such job in the map's last batch");
    const std::vector<rgbd360_map_align_trace>& tr = m->b_trace[(size_t)job];
    if (n_trace) *n_trace = (int)tr.size();
    for (int k = 0; trace && k < max_trace && k < (int)tr.size(); ++k) trace[k] = tr[k];
    return 0;
}
