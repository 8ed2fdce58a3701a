// depth_train.h -- training the sensors' intrinsic depth models (depth_model.h applies them) against the resident voxel map: the training
// half of CLAMS' DiscreteDepthDistortionModel (Teichman et al.; vendored by the reference under OpenNI2_Grabber/third_party/CLAMS:
// DiscreteFrustum::addExample, discrete_depth_distortion_model.cpp:21-36, and DiscreteDepthDistortionModel::accumulate :193-217) with the
// per-frustum sums kept on the device as integers.  A ground-truth depth image of a sensor at a pose is one surface cast of the sensor's
// pinhole rays through the map (map_raycast.h, map_normals.h); the kernel below casts, pairs each depth with the sensor's raw
// measurement and adds the example to its (frustum, slice).  Part of the Frame360 translation unit (rgbd360_frame360.hip includes it
// behind map_raycast.h, map_normals.h and map_planes.h, whose per-wave merge by key it calls).
//
// Definition (include/rgbd360_hip.h, "training the depth model"; tests/depth_train_reference.py restates it).  An example
// is a ground-truth z `gt` and a measured z `meas`, float32 metres widened to double; float64 + - x / floor without contraction.
//   1 measurement   meas finite and > 0 (uint16: non-zero, 0.001f * (float)v as every entry scales it); else n_no_measurement
//   2 range         meas > max_range or gt > max_range: n_out_of_range
//   3 multiplier    mult = gt / meas; mult > max_mult || mult < min_mult: n_mult_rejected (addExample's test, against the doubles of the
//                   float32 parameters)
//   4 slice         idx = min(num_bins - 1, (int)floor(meas / bin_depth))
//   5 frustum       (min(v / bin_height, num_bins_y - 1), min(u / bin_width, num_bins_x - 1))
//   6 sums          count += 1, num += llrint(gt gt 2^20), den += llrint(gt meas 2^20): integer atomics only
// The image route takes gt from an image (0, negative or not finite: n_no_hit, looked at before step 1).  The map route casts the ray of
// pixel (v, u): o = the sensor pose's translation, f = ((u - cx) / fx, (v - cy) / fy, 1) in float32, d_k = (R_k0 f_x + R_k1 f_y) + R_k2 f_z
// (the rounding of the panorama's rays), so that t is the sensor-frame z; gt = the surface cast's float32 t of that ray.  Gates in this
// order: no measurement (no ray is cast), a miss of any status (n_no_hit), require_plane and the plane depth not taken (n_off_plane),
// min_cos_incidence > 0 and no normal or |q| < min_cos_incidence sqrt((d_x^2 + d_y^2) + d_z^2), q = n . d in double (n_grazing), then 2-6.
//
// The state: three 64-bit words (count, num, den) per (frustum, slice), interleaved, bins in [num_bins_y][num_bins_x][num_bins] order.  With
// max_range <= 16 a term is below 2^28, and a call is refused once the examples so far plus its pixels reach 2^34: no word can wrap.
// Integer sums: the bits do not depend on the order of the frames, on the launch shape or on the run.
//
//   k_depth_train<MAP, LAYER>   one lane per pixel, 256 threads = a tile of 16 x 16 pixels, a wave = 8 x 8 of them: neighbouring rays
//                               walk the same bricks and a wave touches few frustums.  vmap::cast_ray<LAYER>(.., FirstHit) and
//                               vmap::surface_step as they are.  The three adds of a lane go to words many lanes share (a bin is tens
//                               of pixels of nearly one depth); three forms, one result: 0 plain per-lane atomics, 1 the lanes of equal
//                               bin summed over the wave and one atomic per bin and word (vmap::wave_add_by_key, map_planes.h), 2 a
//                               per-block LDS table (integer LDS atomics; one slot per distinct bin of the block, claimed by an LDS
//                               compare-and-swap) flushed once per touched word.  Counters through ballots, one add per wave.
//                               The gates and the counters are train_gates and train_counters, the functions depth_apply.h's
//                               k_depth_eval calls too: the evaluation judges a model on exactly the trainer's examples.
#pragma once

struct rgbd360_depth_trainer {
    rgbd360_ctx* ctx = nullptr;
    F360State* s = nullptr;              // the context's Frame360 state: device and stream (not owned)
    int width = 0, height = 0, bin_width = 0, bin_height = 0, nbx = 0, nby = 0, nb = 0, smoothing = 0;
    double bin_depth = 0;
    long long n_examples = 0;            // examples in the sums (the bound of a call's refusal)
    int form = 2;                        // how the kernel adds (rgbd360_depth_trainer_set_form): the per-block LDS table, the fastest of the
                                         // three on the device (profiles/depth_train_perf.txt)
    std::string err;
    DevBuf<unsigned long long> sums, d_stats;      // 3 words per bin; the counters
    PinnedBuf<unsigned long long> h_stats;
    DevBuf<uint8_t> up_gt, up_meas;      // host images on their way to the kernel
    DevBuf<float> gt_stage;              // gt_out of a host call
    size_t bins() const { return (size_t)nby * nbx * nb; }
};

namespace vmap {

constexpr int kTrainThreads = 256;
constexpr int kTrainTile = 16;           // a workgroup's pixels: 16 x 16, four waves of 8 x 8
enum { kTrPixels, kTrNoMeas, kTrNoHit, kTrOffPlane, kTrGrazing, kTrRange, kTrMult, kTrExamples, kTrWords };      // rgbd360_depth_train_stats in its order

struct TrainJob {
    DevGrid G;                           // the map route: the cast's tables, limits and the normal layer
    RayParams P;
    const uint4* normals;
    double shift2_max;
    float fx, fy, cx, cy;
    float pose[16];
    int require_plane;
    double min_cos;
    const void* gt;                      // the image route: the ground-truth image
    size_t gt_step;
    const void* meas;
    size_t meas_step;
    int depth_type, rows, cols;
    double min_mult, max_mult, max_range, bin_depth;
    int bin_width, bin_height, nbx, nby, nb;
    int form;
    float* gt_out;                       // may be null
    unsigned long long *sums, *stats;
};

__device__ __forceinline__ float train_depth_at(const void* img, size_t step, int depth_type, int v, int u) {
    const unsigned char* row = (const unsigned char*)img + (size_t)v * step;
    return depth_type == 0 ? 0.001f * (float)((const uint16_t*)row)[u] : ((const float*)row)[u];
}

// what the gates leave of a pixel: the measurement and the ground truth, cat (the one counter of the pixel), reached (step 2 onwards),
// example, and an example's bin and three terms
struct TrainPixel {
    float meas32, gt32;
    int cat;
    bool reached, example;
    int bin;
    long long term[3];
};
// steps "measurement ... multiplier" of pixel (v, u) of the map or image route; in: whether it lies in the image
template <bool MAP, bool LAYER>
__device__ __forceinline__ TrainPixel train_gates(const TrainJob& J, int v, int u, bool in) {
#pragma clang fp contract(off)
    TrainPixel px;
    const float meas32 = in ? train_depth_at(J.meas, J.meas_step, J.depth_type, v, u) : 0.f;
    const bool measured = in && __builtin_isfinite(meas32) && meas32 > 0.f;
    int cat = kTrNoMeas;                 // the one counter of this pixel
    float gt32 = 0.f;
    if (MAP) {
        if (measured) {
            const float fx = ((float)u - J.cx) / J.fx, fy = ((float)v - J.cy) / J.fy, fz = 1.f;
            float o[3], d[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                d[k] = (J.pose[k] * fx + J.pose[k + 4] * fy) + J.pose[k + 8] * fz;
                o[k] = J.pose[12 + k];
            }
            RayResult H;
            cast_ray<LAYER>(J.G, J.P, o, d, H);
            cat = kTrNoHit;
            if (H.status == kRayHit) {
                const uint4 rec = J.normals[(H.rec - J.G.table) / kFields];
                float c[3], nrm[3];
                centroid(H.rec, H.rec[1], c);
                double t = H.t;
                const bool on_plane = surface_step(rec, c, o, d, J.P.t_min, (double)J.P.inv_leaf, J.shift2_max, nrm, t);
                cat = kTrExamples;
                if (J.require_plane && !on_plane) {
                    cat = kTrOffPlane;
                } else if (J.min_cos > 0.0) {
                    const NormalRec R = normal_unpack(rec);
                    const double q = ((double)R.n[0] * (double)d[0] + (double)R.n[1] * (double)d[1]) + (double)R.n[2] * (double)d[2];
                    const double dd = ((double)d[0] * (double)d[0] + (double)d[1] * (double)d[1]) + (double)d[2] * (double)d[2];
                    if (R.status != kClassKept || fabs(q) < J.min_cos * sqrt(dd)) cat = kTrGrazing;
                }
                if (cat == kTrExamples) gt32 = (float)t;
            }
        }
    } else if (in) {
        const float g = train_depth_at(J.gt, J.gt_step, J.depth_type, v, u);
        if (!(__builtin_isfinite(g) && g > 0.f)) cat = kTrNoHit;
        else if (measured) cat = kTrExamples, gt32 = g;
    }
    const bool reached = in && cat == kTrExamples;      // step 2 onwards
    long long term[3] = {0ll, 0ll, 0ll};
    int bin = 0;
    if (reached) {
        const double gt = (double)gt32, meas = (double)meas32;
        const double mult = gt / meas;
        if (meas > J.max_range || gt > J.max_range) {
            cat = kTrRange;
        } else if (mult > J.max_mult || mult < J.min_mult) {
            cat = kTrMult;
        } else {
            const double sl = __builtin_floor(meas / J.bin_depth);
            const int idx = sl < (double)(J.nb - 1) ? (int)sl : J.nb - 1;
            const int by = min(v / J.bin_height, J.nby - 1), bx = min(u / J.bin_width, J.nbx - 1);
            bin = (by * J.nbx + bx) * J.nb + idx;
            term[0] = 1ll;
            term[1] = __double2ll_rn(gt * gt * 1048576.0);
            term[2] = __double2ll_rn(gt * meas * 1048576.0);
        }
    }
    px.meas32 = meas32, px.gt32 = gt32, px.cat = cat, px.reached = reached, px.example = reached && cat == kTrExamples, px.bin = bin;
#pragma unroll
    for (int q = 0; q < 3; ++q) px.term[q] = term[q];
    return px;
}
// the counters of a pixel's wave (rgbd360_depth_train_stats) through ballots
__device__ __forceinline__ void train_counters(unsigned long long* stats, int lane, bool in, int cat) {
    unsigned long long b[kTrWords];
#pragma unroll
    for (int q = 1; q < kTrWords; ++q) b[q] = __ballot(in && cat == q);
    b[kTrPixels] = __ballot(in);
    if (lane == 0 && b[kTrPixels]) {      // one add per wave and counter
#pragma unroll
        for (int q = 0; q < kTrWords; ++q)
            if (b[q]) atomicAdd(stats + q, (unsigned long long)__popcll(b[q]));
    }
}

template <bool MAP, bool LAYER>
__global__ __launch_bounds__(kTrainThreads) void k_depth_train(TrainJob J) {
#pragma clang fp contract(off)
    __shared__ int l_key[kTrainThreads];
    __shared__ unsigned long long l_val[3 * kTrainThreads];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.x * kTrainTile + (wave & 1) * 8 + (lane & 7), v = blockIdx.y * kTrainTile + (wave >> 1) * 8 + (lane >> 3);
    const bool in = u < J.cols && v < J.rows;
    if (J.form == 2) {      // (uniform over the launch)
        l_key[threadIdx.x] = -1;
#pragma unroll
        for (int q = 0; q < 3; ++q) l_val[3 * threadIdx.x + q] = 0ull;
        __syncthreads();
    }
    const TrainPixel px = train_gates<MAP, LAYER>(J, v, u, in);
    if (J.form == 2) {
        if (px.example) {
            const int bin = px.bin;
            unsigned slot = ((unsigned)bin * 2654435761u) >> 24;      // (at most 256 distinct bins in a block: every one finds a slot)
            for (;;) {
                const int k0 = atomicCAS(&l_key[slot], -1, bin);
                if (k0 == -1 || k0 == bin) break;
                slot = (slot + 1) & (kTrainThreads - 1);
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) atomicAdd(&l_val[3 * slot + q], (unsigned long long)px.term[q]);
        }
        __syncthreads();
        const int k0 = l_key[threadIdx.x];
        if (k0 >= 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) atomicAdd(J.sums + (size_t)k0 * 3 + q, l_val[3 * threadIdx.x + q]);
        }
    } else {
        wave_add_by_key<3>(px.example, px.bin, px.term, J.sums, J.form == 1);
    }
    train_counters(J.stats, lane, in, px.cat);
    if (in && J.gt_out) J.gt_out[(size_t)v * J.cols + u] = px.reached ? px.gt32 : 0.f;
}

}  // namespace vmap

namespace {

static_assert(sizeof(rgbd360_depth_train_stats) == vmap::kTrWords * sizeof(unsigned long long), "the statistics are the counters in their order");

int train_fail(rgbd360_depth_trainer* t, int code, const char* msg) {
    t->err = msg;
    return code;
}
void train_fill_stats(const unsigned long long* w, rgbd360_depth_train_stats* st) {
    if (!st) return;
    long long* out = &st->n_pixels;
    for (int k = 0; k < vmap::kTrWords; ++k) out[k] = w ? (long long)w[k] : 0;
}
// what both routes check of the example's parameters, of the image and of the room left in the words; 1: no pixels
int train_check(rgbd360_depth_trainer* t, const rgbd360_depth_train_params& p, const void* meas, size_t meas_step, int depth_type, int rows, int cols) {
    if (!(p.max_range > 0.f) || !(p.max_range <= 16.f)) return train_fail(t, -1, "max_range must lie in (0, 16]");
    if (!(p.min_mult >= 0.f) || !(p.max_mult >= p.min_mult)) return train_fail(t, -1, "0 <= min_mult <= max_mult is required");
    if (depth_type != 0 && depth_type != 1) return train_fail(t, -1, "bad depth type");
    if (rows < 0 || cols < 0) return train_fail(t, -1, "bad image size");
    if (rows == 0 || cols == 0) return 1;
    if (rows != t->height || cols != t->width) return train_fail(t, -1, "the image is not of the trainer's size");
    if (!meas) return train_fail(t, -1, "the measured image must not be null");
    if (meas_step < (size_t)cols * (depth_type == 0 ? 2 : 4)) return train_fail(t, -1, "row step shorter than a row");
    if (t->n_examples + (long long)rows * cols >= (1ll << 34)) return train_fail(t, -1, "the trainer is full: 2^34 examples (read the sums out and clear)");
    return 0;
}
// a host image packed on the device, or the device image as it is
int train_image(rgbd360_depth_trainer* t, DevBuf<uint8_t>& buf, const void*& img, size_t& step, int depth_type, int rows, int cols, int on_device) {
    if (on_device) return 0;
    const size_t row = (size_t)cols * (depth_type == 0 ? 2 : 4);
    HIPC(t, buf.ensure(row * (size_t)rows));
    HIPC(t, hipMemcpy2DAsync(buf, row, img, step, row, (size_t)rows, hipMemcpyHostToDevice, t->s->stream));
    img = buf.get(), step = row;
    return 0;
}
// the job of a checked call but for the map's part
vmap::TrainJob train_job(rgbd360_depth_trainer* t, const rgbd360_depth_train_params& p, const void* meas, size_t meas_step, int depth_type) {
    vmap::TrainJob J = {};
    J.meas = meas, J.meas_step = meas_step, J.depth_type = depth_type, J.rows = t->height, J.cols = t->width;
    J.min_mult = (double)p.min_mult, J.max_mult = (double)p.max_mult, J.max_range = (double)p.max_range, J.bin_depth = t->bin_depth;
    J.bin_width = t->bin_width, J.bin_height = t->bin_height, J.nbx = t->nbx, J.nby = t->nby, J.nb = t->nb;
    J.form = t->form;
    J.sums = t->sums, J.stats = t->d_stats;
    return J;
}
// the kernel over the job, enqueued behind the clear of its counters; layered: the map route's traversal
int train_launch(rgbd360_depth_trainer* t, const vmap::TrainJob& J, bool map_route, bool layered) {
    HIPC(t, hipMemsetAsync(t->d_stats, 0, vmap::kTrWords * sizeof(unsigned long long), t->s->stream));
    const dim3 grid((unsigned)((J.cols + vmap::kTrainTile - 1) / vmap::kTrainTile), (unsigned)((J.rows + vmap::kTrainTile - 1) / vmap::kTrainTile));
    if (!map_route) hipLaunchKernelGGL((vmap::k_depth_train<false, false>), grid, dim3(vmap::kTrainThreads), 0, t->s->stream, J);
    else if (layered) hipLaunchKernelGGL((vmap::k_depth_train<true, true>), grid, dim3(vmap::kTrainThreads), 0, t->s->stream, J);
    else hipLaunchKernelGGL((vmap::k_depth_train<true, false>), grid, dim3(vmap::kTrainThreads), 0, t->s->stream, J);
    HIPC(t, hipGetLastError());
    return 0;
}
// the counters read back; the call waits
int train_finish(rgbd360_depth_trainer* t, rgbd360_depth_train_stats* stats) {
    HIPC(t, hipMemcpyAsync(t->h_stats, t->d_stats, vmap::kTrWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, t->s->stream));
    HIPC(t, hipStreamSynchronize(t->s->stream));
    t->n_examples += (long long)t->h_stats[vmap::kTrExamples];
    train_fill_stats(t->h_stats, stats);
    return 0;
}
// The map's part of a job: both parameter structs checked, the coarse layer and the normal layer built or reused as the surface cast does
// (ray_prepare), the pinhole and the gates.  The map's error text goes to the trainer.
int train_map_job(rgbd360_depth_trainer* t, rgbd360_map* m, const rgbd360_depth_train_params& p, float fx, float fy, float cx, float cy, const float* pose,
                  vmap::TrainJob& J, bool prepare) {
    rgbd360_map_raycast_params rp;
    rgbd360_map_normal_params np;
    int rc = ray_check_params(m, &p.ray, rp);
    if (rc == 0) rc = normal_check_params(m, &p.normal, np);
    if (rc == 0 && prepare) rc = ray_prepare(m, &np);
    if (rc) {
        t->err = m->err;
        return rc;
    }
    const vmap::RayJob R = ray_job(m, rp);
    J.G = R.G, J.P = R.P;
    J.normals = m->nm_layer;
    J.shift2_max = (double)np.max_shift * (double)np.max_shift;
    J.fx = fx, J.fy = fy, J.cx = cx, J.cy = cy;
    memcpy(J.pose, pose, sizeof(J.pose));
    J.require_plane = p.require_plane != 0;
    J.min_cos = (double)p.min_cos_incidence;
    return 0;
}
int train_check_map(rgbd360_depth_trainer* t, const rgbd360_map* m, const rgbd360_depth_train_params& p, float fx, float fy, float cx, float cy,
                    const float* pose) {
    if (!m) return train_fail(t, -1, "map must not be null");
    if (m->s != t->s) return train_fail(t, -1, "the map belongs to another context");
    if (!pose) return train_fail(t, -1, "sensor_pose must not be null");
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(pose[k])) return train_fail(t, -1, "sensor_pose must be finite");
    if (!std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy) || fx == 0.f || fy == 0.f)
        return train_fail(t, -1, "fx, fy, cx, cy must be finite and the focal lengths not zero");
    if (!(p.min_cos_incidence >= 0.f) || !(p.min_cos_incidence <= 1.f)) return train_fail(t, -1, "min_cos_incidence must lie in [0, 1]");
    return 0;
}
int train_read_sums(rgbd360_depth_trainer* t, std::vector<unsigned long long>& w) {
    hipSetDevice(t->s->p.device);
    w.resize(3 * t->bins());
    HIPC(t, hipMemcpyAsync(w.data(), t->sums, w.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, t->s->stream));
    HIPC(t, hipStreamSynchronize(t->s->stream));
    return 0;
}

}  // namespace

extern "C" int rgbd360_depth_trainer_create(rgbd360_ctx* ctx_, int width, int height, int bin_width, int bin_height, double bin_depth, int smoothing,
                                            rgbd360_depth_trainer** out) {
    if (out) *out = nullptr;
    if (!ctx_ || !out) return -1;
    F360_ENTER(ctx_);
    if (width < 1 || height < 1 || width > 16384 || height > 16384 || bin_width < 1 || bin_height < 1 || width % bin_width != 0 ||
        height % bin_height != 0)
        return fail(ctx, -1, "rgbd360_depth_trainer_create: the image sides must lie in 1 .. 16384 and be multiples of the bin sides");
    if (!(bin_depth > 0) || !(10.0 / bin_depth <= 4096.0) || smoothing < 0)
        return fail(ctx, -1, "rgbd360_depth_trainer_create: bin_depth must be positive (at most 4096 slices) and smoothing not negative");
    std::unique_ptr<rgbd360_depth_trainer> t(new rgbd360_depth_trainer());
    t->ctx = ctx_, t->s = ctx;
    t->width = width, t->height = height, t->bin_width = bin_width, t->bin_height = bin_height;
    t->nbx = width / bin_width, t->nby = height / bin_height, t->nb = (int)std::ceil(10.0 / bin_depth);      // DiscreteFrustum: max_dist 10
    t->bin_depth = bin_depth, t->smoothing = smoothing;
    if ((long long)t->nbx * t->nby * t->nb > (1ll << 26)) return fail(ctx, -1, "rgbd360_depth_trainer_create: more than 2^26 (frustum, slice) bins");
    hipSetDevice(ctx->p.device);
    if (t->sums.ensure(3 * t->bins()) != hipSuccess || t->d_stats.ensure(vmap::kTrWords) != hipSuccess || t->h_stats.ensure(vmap::kTrWords) != hipSuccess ||
        hipMemsetAsync(t->sums, 0, 3 * t->bins() * sizeof(unsigned long long), ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, -103, "rgbd360_depth_trainer_create: out of memory");
    }
    *out = t.release();
    return 0;
}
extern "C" void rgbd360_depth_trainer_destroy(rgbd360_depth_trainer* t) {
    if (!t) return;
    hipSetDevice(t->s->p.device);
    hipStreamSynchronize(t->s->stream);
    delete t;
}
extern "C" const char* rgbd360_depth_trainer_last_error(rgbd360_depth_trainer* t) { return t ? t->err.c_str() : "null trainer"; }
extern "C" int rgbd360_depth_trainer_clear(rgbd360_depth_trainer* t) {
    if (!t) return -1;
    t->err.clear();
    hipSetDevice(t->s->p.device);
    HIPC(t, hipMemsetAsync(t->sums, 0, 3 * t->bins() * sizeof(unsigned long long), t->s->stream));
    HIPC(t, hipStreamSynchronize(t->s->stream));
    t->n_examples = 0;
    return 0;
}

extern "C" void rgbd360_depth_default_train_params(const rgbd360_map* map, rgbd360_depth_train_params* p) {
    if (!p) return;
    rgbd360_map_default_raycast_params(map, &p->ray);
    rgbd360_map_default_normal_params(map, &p->normal);
    p->require_plane = 1;
    p->min_cos_incidence = 0.f;
    p->min_mult = 0.7f;          // stream_sequence/typedefs.h:6-7
    p->max_mult = 1.3f;
    p->max_range = 10.f;
}

extern "C" int rgbd360_depth_trainer_accumulate_images(rgbd360_depth_trainer* t, const void* gt, size_t gt_step, const void* meas, size_t meas_step,
                                                       int depth_type, int rows, int cols, int on_device, const rgbd360_depth_train_params* params,
                                                       rgbd360_depth_train_stats* stats) {
    if (!t) return -1;
    t->err.clear();
    rgbd360_depth_train_params p;
    if (params) p = *params;
    else rgbd360_depth_default_train_params(nullptr, &p);
    const int chk = train_check(t, p, meas, meas_step, depth_type, rows, cols);
    if (chk < 0) return chk;
    train_fill_stats(nullptr, stats);
    if (chk == 1) return 0;
    if (!gt) return train_fail(t, -1, "the ground-truth image must not be null");
    if (gt_step < (size_t)cols * (depth_type == 0 ? 2 : 4)) return train_fail(t, -1, "row step shorter than a row");
    hipSetDevice(t->s->p.device);
    if (const int rc = train_image(t, t->up_gt, gt, gt_step, depth_type, rows, cols, on_device)) return rc;
    if (const int rc = train_image(t, t->up_meas, meas, meas_step, depth_type, rows, cols, on_device)) return rc;
    vmap::TrainJob J = train_job(t, p, meas, meas_step, depth_type);
    J.gt = gt, J.gt_step = gt_step;
    if (const int rc = train_launch(t, J, false, false)) return rc;
    return train_finish(t, stats);
}

extern "C" int rgbd360_depth_trainer_accumulate_map(rgbd360_depth_trainer* t, rgbd360_map* m, const void* meas, size_t meas_step, int depth_type, int rows,
                                                    int cols, float fx, float fy, float cx, float cy, const float sensor_pose[16], int on_device,
                                                    const rgbd360_depth_train_params* params, float* gt_out, rgbd360_depth_train_stats* stats) {
    if (!t) return -1;
    t->err.clear();
    if (!m) return train_fail(t, -1, "map must not be null");
    m->err.clear();
    rgbd360_depth_train_params p;
    if (params) p = *params;
    else rgbd360_depth_default_train_params(m, &p);
    const int chk = train_check(t, p, meas, meas_step, depth_type, rows, cols);
    if (chk < 0) return chk;
    if (const int rc = train_check_map(t, m, p, fx, fy, cx, cy, sensor_pose)) return rc;
    vmap::TrainJob J = {};
    if (chk == 0) J = train_job(t, p, meas, meas_step, depth_type);
    if (const int rc = train_map_job(t, m, p, fx, fy, cx, cy, sensor_pose, J, false)) return rc;      // (the parameters alone)
    train_fill_stats(nullptr, stats);
    if (chk == 1) return 0;
    hipSetDevice(t->s->p.device);
    hipStream_t stream = t->s->stream;
    const size_t n = (size_t)rows * cols;
    if (m->n_voxels == 0) {      // nothing to hit: no kernel
        if (gt_out && on_device) {
            HIPC(t, hipMemsetAsync(gt_out, 0, n * sizeof(float), stream));
            HIPC(t, hipStreamSynchronize(stream));
        } else if (gt_out) {
            memset(gt_out, 0, n * sizeof(float));
        }
        return 0;
    }
    if (const int rc = train_map_job(t, m, p, fx, fy, cx, cy, sensor_pose, J, true)) return rc;
    if (const int rc = train_image(t, t->up_meas, meas, meas_step, depth_type, rows, cols, on_device)) return rc;
    J.meas = meas, J.meas_step = meas_step;
    if (gt_out && !on_device) {
        HIPC(t, t->gt_stage.ensure(n));
        J.gt_out = t->gt_stage;
    } else {
        J.gt_out = gt_out;
    }
    if (const int rc = train_launch(t, J, true, !m->rc_plain)) return rc;
    if (gt_out && !on_device) HIPC(t, hipMemcpyAsync(gt_out, J.gt_out, n * sizeof(float), hipMemcpyDeviceToHost, stream));
    return train_finish(t, stats);
}

extern "C" int rgbd360_depth_trainer_sums(rgbd360_depth_trainer* t, int64_t* count, int64_t* num, int64_t* den) {
    if (!t) return -1;
    t->err.clear();
    if (!count || !num || !den) return train_fail(t, -1, "count, num and den must not be null");
    try {
        std::vector<unsigned long long> w;
        if (const int rc = train_read_sums(t, w)) return rc;
        for (size_t k = 0; k < t->bins(); ++k) count[k] = (int64_t)w[3 * k], num[k] = (int64_t)w[3 * k + 1], den[k] = (int64_t)w[3 * k + 2];
        return 0;
    } catch (const std::exception&) {
        return train_fail(t, -103, "out of memory");
    }
}
extern "C" int rgbd360_depth_trainer_add_sums(rgbd360_depth_trainer* t, const int64_t* count, const int64_t* num, const int64_t* den) {
    if (!t) return -1;
    t->err.clear();
    if (!count || !num || !den) return train_fail(t, -1, "count, num and den must not be null");
    try {
        // what another trainer of this shape can hold: terms below 2^28 each, and room for them here
        long long added = 0;
        for (size_t k = 0; k < t->bins(); ++k) {
            if (count[k] < 0 || count[k] >= (1ll << 34) || num[k] < 0 || den[k] < 0 || num[k] > (count[k] << 28) || den[k] > (count[k] << 28))
                return train_fail(t, -1, "these are not the sums of a trainer");
            added += count[k];
            if (t->n_examples + added >= (1ll << 34)) return train_fail(t, -1, "the trainer is full: 2^34 examples (read the sums out and clear)");
        }
        std::vector<unsigned long long> w;
        if (const int rc = train_read_sums(t, w)) return rc;
        for (size_t k = 0; k < t->bins(); ++k) {
            w[3 * k] += (unsigned long long)count[k];
            w[3 * k + 1] += (unsigned long long)num[k];
            w[3 * k + 2] += (unsigned long long)den[k];
        }
        HIPC(t, hipMemcpyAsync(t->sums, w.data(), w.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, t->s->stream));
        HIPC(t, hipStreamSynchronize(t->s->stream));      // `w` (pageable) must outlive the copy
        t->n_examples += added;
        return 0;
    } catch (const std::exception&) {
        return train_fail(t, -103, "out of memory");
    }
}
extern "C" int rgbd360_depth_trainer_model(rgbd360_depth_trainer* t, rgbd360_depth_model** out) {
    if (out) *out = nullptr;
    if (!t) return -1;
    t->err.clear();
    if (!out) return train_fail(t, -1, "out must not be null");
    try {
        const size_t n = t->bins();
        std::vector<int64_t> s(3 * n);
        if (const int rc = rgbd360_depth_trainer_sums(t, s.data(), s.data() + n, s.data() + 2 * n)) return rc;
        if (rgbd360_depth_model_from_sums(t->width, t->height, t->bin_width, t->bin_height, t->bin_depth, t->smoothing, s.data(), s.data() + n, s.data() + 2 * n,
                                          out) != 0)
            return train_fail(t, -1, "rgbd360_depth_model_from_sums refused the sums");
        return 0;
    } catch (const std::exception&) {
        return train_fail(t, -103, "out of memory");
    }
}

// measurement and the form switch (rgbd360_hip_diag.h)
extern "C" int rgbd360_depth_trainer_set_form(rgbd360_depth_trainer* t, int form) {
    if (!t) return -1;
    t->err.clear();
    if (form < 0 || form > 2) return train_fail(t, -1, "form must be 0, 1 or 2");
    t->form = form;
    return 0;
}
extern "C" int rgbd360_depth_trainer_time_map(rgbd360_depth_trainer* t, rgbd360_map* m, const void* meas_dev, size_t meas_step, int depth_type, float fx,
                                              float fy, float cx, float cy, const float sensor_pose[16], const rgbd360_depth_train_params* params,
                                              const float* origins_dev, const float* dirs_dev, int reps, float* train_us, float* cast_us,
                                              rgbd360_depth_train_stats* stats) {
    if (!t) return -1;
    t->err.clear();
    if (!m || !params || !origins_dev || !dirs_dev || reps < 1 || !train_us || !cast_us) return train_fail(t, -1, "bad arguments");
    m->err.clear();
    const rgbd360_depth_train_params p = *params;
    if (train_check(t, p, meas_dev, meas_step, depth_type, t->height, t->width) != 0) return -1;
    if (const int rc = train_check_map(t, m, p, fx, fy, cx, cy, sensor_pose)) return rc;
    if (m->n_voxels == 0) return train_fail(t, -1, "the map is empty");
    hipSetDevice(t->s->p.device);
    vmap::TrainJob J = train_job(t, p, meas_dev, meas_step, depth_type);
    if (const int rc = train_map_job(t, m, p, fx, fy, cx, cy, sensor_pose, J, true)) return rc;
    const size_t n = (size_t)t->height * t->width;
    HIPC(t, m->rc_stage.ensure(39 * n));
    // the yardstick: the surface cast of the same rays with its depth, normal and status planes
    rgbd360_map_raycast_params rp = p.ray;
    rgbd360_map_normal_params np = p.normal;
    vmap::RayJob R = ray_job(m, rp);
    ray_surface_job(m, R, np);
    R.n = (long long)n;
    R.origins = origins_dev, R.dirs = dirs_dev;
    uint8_t* sg = m->rc_stage;
    R.t = reinterpret_cast<float*>(sg);
    R.status = reinterpret_cast<int32_t*>(sg + 8 * n);
    R.normal = reinterpret_cast<float*>(sg + 24 * n);
    // the sums are put back after the timed launches: a measurement leaves the trainer as it was
    std::vector<unsigned long long> keep;
    if (const int rc = train_read_sums(t, keep)) return rc;
    VmapTimer timer(m, t->s->stream);
    for (int r = 0; r < reps && timer.rc == 0; ++r) {
        for (int form = 0; form < 3; ++form) {
            J.form = form;
            timer.timed(train_us[form * reps + r], 1, [&] { return train_launch(t, J, true, !m->rc_plain); });
        }
        timer.timed(cast_us[r], 1, [&] { return ray_launch(m, R, false, m->rc_plain, true); });
    }
    if (timer.rc) {
        (void)hipGetLastError();
        if (t->err.empty()) t->err = m->err;
        return timer.rc;
    }
    HIPC(t, hipMemcpyAsync(t->h_stats, t->d_stats, vmap::kTrWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, t->s->stream));
    HIPC(t, hipMemcpyAsync(t->sums, keep.data(), keep.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, t->s->stream));
    HIPC(t, hipStreamSynchronize(t->s->stream));
    train_fill_stats(t->h_stats, stats);
    return 0;
}
