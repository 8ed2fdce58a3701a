// depth_apply.h -- applying the sensors' intrinsic depth models (depth_model.h) on the device: the models of a rig resident in device
// memory as one packed, pointer-free blob, ONE per-pixel text over that blob for host and device, a stand-alone undistort, the same
// correction inside the rig calibration's cloud formation (rig_calib.h) and the evaluation of a model against the map on the trainer's
// own examples (depth_train.h).  The step "undistort" of CLAMS' loop "map, train, save, undistort, re-map, calibrate, repeat".
// Two units include it: rgbd360_host.cpp (with DEPTH_APPLY_PACKER: the packer, which sees depthmodel::Model, and the host run of the
// per-pixel text) and rgbd360_frame360.hip behind rig_calib.h and depth_train.h (the kernels and the entries: the map, the trainer's
// gates and k_rig_pinhole_cloud live in that unit).
//
// The blob (include/rgbd360_hip.h, "applying the depth models on the device"; tests/depth_apply_reference.py restates
// the arithmetic).  Head, then one section per sensor that has a model:
//   Head        magic, n_sensors, width, height (0 x 0: no sensor has a model), bytes, and per sensor {has, bin_width, bin_height,
//               num_bins_x, num_bins_y, offset and bytes of its section}
//   section     num_bins_y x num_bins_x Frustum records {bin_depth (float64), num_bins, first slice} -- the file gives every frustum
//               its own num_bins and bin_depth and they are kept -- then the Slice records {multiplier, count} (float32, as loaded: the
//               comparison count < 50 is literally the host's) of all frustums, a frustum's slices side by side.  The first slice is an
//               index in Slice units from the section's start, so a section can be moved (rgbd360_depth_models_set).
// Every model rgbd360_depth_model_load or _from_sums can hold is represented exactly; a set whose blob would exceed kMaxBytes (1 GiB) is
// refused.  Nothing is approximated.
//
//   apply_px              depthmodel::slice_of + undistort_px (depth_model.h:130-149), operation for operation, under fp contract(off):
//                         the float64 floor(z / bin_depth), the !(q < num_bins - 1) clamp, start = (float)(bin_depth idx), the half-slice
//                         test in double, the float32 fall-back z multipliers[max(idx, 0)], the float64 interpolation.  A z that is 0,
//                         negative or NaN is returned as it is; +Inf takes the fall-back branch.
//   k_depth_undistort     ONE launch over all images of a call, one lane per pixel, 256 threads = 16 x 16 pixels, a wave = 8 x 8 (as
//                         k_depth_train): a wave touches a handful of frustums.  uint16 millimetres are converted (float)(0.001 (double)v),
//                         Frame360::undistort's and OpenCV's convertTo(.., 0.001) -- NOT the 0.001f (float)v of the map entries.
//   k_rig_cloud_models    k_rig_pinhole_cloud with z corrected by the image's sensor before the ray product; the pixel's text is
//                         rigc::pinhole_pixel, shared with that kernel.
//   k_depth_eval          vmap::train_gates, the function k_depth_train calls: the trainer's gates (on the RAW measurement), then per example
//                         e_raw = meas - gt, e_cor = z' - gt in float64 and five integer terms, summed over the wave, one 64-bit integer
//                         atomic per wave and word.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define DA_HD __host__ __device__
#else
#define DA_HD
#endif

namespace depthapply {

constexpr int kMaxSensors = 16;                              // RGBD360_RIG_CALIB_MAX_SENSORS
constexpr unsigned kMagic = 0x31304d44u;                     // "DM01"
constexpr unsigned long long kMaxBytes = 1ull << 30;         // the documented bound of a blob

struct Sensor {
    int has, bin_width, bin_height, nbx, nby, pad;
    unsigned long long offset, bytes;                        // the section, from the blob's start
};
struct Head {
    unsigned magic;
    int n_sensors, width, height;
    unsigned long long bytes;
    Sensor sensor[kMaxSensors];
};
struct Frustum {
    double bin_depth;
    int num_bins;
    unsigned first;                                          // its first Slice, in Slice units from the section's start
};
struct Slice {
    float multiplier, count;
};
static_assert(sizeof(Sensor) == 40 && sizeof(Head) == 24 + 40 * kMaxSensors && sizeof(Frustum) == 16 && sizeof(Slice) == 8, "the blob's layout");

// the two millimetre conversions of the library: Frame360::undistort's (the stand-alone undistort) and the map entries'
// (rgbd360_set_target, the trainer, k_rig_pinhole_cloud; the cloud formation and the evaluation here)
DA_HD inline float metres_convert_to(unsigned short raw) { return (float)(0.001 * (double)raw); }
DA_HD inline float metres_map_entries(unsigned short raw) { return 0.001f * (float)raw; }

// the corrected z of pixel (v, u) of `sensor`; the pixel lies inside the set's image
DA_HD inline float apply_px(const unsigned char* blob, int sensor, int v, int u, float z) {
#pragma clang fp contract(off)
    if (z == 0.f || !(z > 0.f)) return z;                    // (no measurement; a negative or NaN depth has no slice either)
    const Sensor& S = reinterpret_cast<const Head*>(blob)->sensor[sensor];
    if (!S.has) return z;
    const unsigned char* sec = blob + S.offset;
    const int yb = v / S.bin_height < S.nby - 1 ? v / S.bin_height : S.nby - 1;
    const int xb = u / S.bin_width < S.nbx - 1 ? u / S.bin_width : S.nbx - 1;
    const Frustum F = reinterpret_cast<const Frustum*>(sec)[(size_t)yb * (size_t)S.nbx + (size_t)xb];
    const Slice* sl = reinterpret_cast<const Slice*>(sec) + F.first;
    const double q = floor((double)z / F.bin_depth);
    int idx;
    if (!(q < (double)(F.num_bins - 1))) idx = F.num_bins - 1;      // beyond the last slice, +Inf: no float -> int conversion out of range
    else idx = q < 0 ? -1 : (int)q;
    const float start = (float)(F.bin_depth * idx);
    const int idx1 = ((double)(z - start) < F.bin_depth / 2) ? idx : idx + 1;
    const int idx0 = idx1 - 1;
    if (idx0 < 0 || idx1 >= F.num_bins || sl[idx0].count < 50 || sl[idx1].count < 50) return z * sl[idx < 0 ? 0 : idx].multiplier;
    const double z0 = (idx0 + 1) * F.bin_depth - F.bin_depth * 0.5;
    const double coeff1 = ((double)z - z0) / F.bin_depth;
    const double coeff0 = 1.0 - coeff1;
    const double mult = coeff0 * (double)sl[idx0].multiplier + coeff1 * (double)sl[idx1].multiplier;
    return (float)((double)z * mult);
}

// what every reader checks of a blob it is handed (the host entries; the device object packs its own)
inline bool blob_ok(const void* blob) {
    const Head* H = static_cast<const Head*>(blob);
    return H && H->magic == kMagic && H->n_sensors >= 1 && H->n_sensors <= kMaxSensors && H->bytes >= sizeof(Head) && H->bytes <= kMaxBytes;
}

#if defined(DEPTH_APPLY_PACKER)
// ---- the packer (rgbd360_host.cpp; depth_model.h is included before this header)
inline bool model_ok(const depthmodel::Model& M) {
    if (M.width < 1 || M.height < 1 || M.bin_width < 1 || M.bin_height < 1 || M.num_bins_x < 1 || M.num_bins_y < 1 ||
        M.frustums.size() != (size_t)M.num_bins_x * (size_t)M.num_bins_y)
        return false;
    for (const depthmodel::Frustum& F : M.frustums)
        if (F.num_bins < 1 || F.counts.size() < (size_t)F.num_bins || F.multipliers.size() < (size_t)F.num_bins || !(F.bin_depth > 0)) return false;
    return true;
}
inline unsigned long long section_bytes(const depthmodel::Model& M) {
    unsigned long long slices = 0;
    for (const depthmodel::Frustum& F : M.frustums) slices += (unsigned long long)F.num_bins;
    return (unsigned long long)M.frustums.size() * sizeof(Frustum) + slices * sizeof(Slice);
}
inline void write_section(const depthmodel::Model& M, unsigned char* dst) {
    Frustum* fr = reinterpret_cast<Frustum*>(dst);
    Slice* sl = reinterpret_cast<Slice*>(dst);
    size_t at = M.frustums.size() * sizeof(Frustum) / sizeof(Slice);
    for (size_t k = 0; k < M.frustums.size(); ++k) {
        const depthmodel::Frustum& F = M.frustums[k];
        fr[k].bin_depth = F.bin_depth, fr[k].num_bins = F.num_bins, fr[k].first = (unsigned)at;
        for (int i = 0; i < F.num_bins; ++i, ++at) sl[at].multiplier = F.multipliers[(size_t)i], sl[at].count = F.counts[(size_t)i];
    }
}
// The blob of `models` (a null entry: identity), or, with `old_blob`, that blob with `sensor` replaced by models[0].  blob null: *bytes is
// the size needed; else *bytes is the room, and on return the size written.  0; -1 what the header names.
inline int pack(const depthmodel::Model* const* models, int n_sensors, const void* old_blob, int sensor, void* blob, size_t* bytes) {
    if (!models || !bytes) return -1;
    const Head* O = static_cast<const Head*>(old_blob);
    if (O) {
        if (!blob_ok(O) || sensor < 0 || sensor >= O->n_sensors) return -1;
        n_sensors = O->n_sensors;
    }
    if (n_sensors < 1 || n_sensors > kMaxSensors) return -1;
    Head H;
    memset(&H, 0, sizeof(H));
    H.magic = kMagic, H.n_sensors = n_sensors;
    const depthmodel::Model* of[kMaxSensors] = {};
    unsigned long long at = sizeof(Head);
    for (int s = 0; s < n_sensors; ++s) {
        Sensor& S = H.sensor[s];
        if (O && s != sensor) {
            S = O->sensor[s];
            if (S.has) {
                if (H.width && (H.width != O->width || H.height != O->height)) return -1;
                H.width = O->width, H.height = O->height;
            }
        } else if (const depthmodel::Model* M = O ? models[0] : models[s]) {
            if (!model_ok(*M)) return -1;
            if (H.width && (H.width != M->width || H.height != M->height)) return -1;      // one width x height over the set
            H.width = M->width, H.height = M->height;
            of[s] = M;
            S.has = 1, S.bin_width = M->bin_width, S.bin_height = M->bin_height, S.nbx = M->num_bins_x, S.nby = M->num_bins_y;
            S.bytes = section_bytes(*M);
        }
        S.offset = S.has ? at : 0;
        at += S.has ? S.bytes : 0;
        if (at > kMaxBytes) return -1;
    }
    H.bytes = at;
    if (!blob) {
        *bytes = (size_t)at;
        return 0;
    }
    if (*bytes < at) return -1;
    unsigned char* out = static_cast<unsigned char*>(blob);
    memcpy(out, &H, sizeof(H));
    for (int s = 0; s < n_sensors; ++s) {
        if (!H.sensor[s].has) continue;
        if (of[s]) write_section(*of[s], out + H.sensor[s].offset);
        else memcpy(out + H.sensor[s].offset, static_cast<const unsigned char*>(old_blob) + O->sensor[s].offset, (size_t)H.sensor[s].bytes);
    }
    *bytes = (size_t)at;
    return 0;
}
// depthmodel::undistort over the blob: the per-pixel text on the host
inline int undistort_packed(const void* blob, int sensor, float* depth, size_t step_bytes, int rows, int cols) {
    const Head* H = static_cast<const Head*>(blob);
    if (!blob_ok(H) || sensor < 0 || sensor >= H->n_sensors || !depth || rows < 0 || cols < 0 || step_bytes < (size_t)cols * 4) return -1;
    if (H->sensor[sensor].has && (rows != H->height || cols != H->width)) return -1;
    for (int v = 0; v < rows; ++v) {
        float* row = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(depth) + (size_t)v * step_bytes);
        for (int u = 0; u < cols; ++u) {
            uint32_t in, out;
            const float z = apply_px(static_cast<const unsigned char*>(blob), sensor, v, u, row[u]);
            memcpy(&in, &row[u], 4), memcpy(&out, &z, 4);
            if (in != out) row[u] = z;
        }
    }
    return 0;
}
#endif  // DEPTH_APPLY_PACKER

}  // namespace depthapply

#if defined(__HIPCC__)
// ---- the device half (rgbd360_frame360.hip, behind rig_calib.h and depth_train.h)
struct rgbd360_depth_models {
    rgbd360_ctx* ctx = nullptr;
    F360State* s = nullptr;              // the context's Frame360 state: device and stream (not owned)
    std::vector<unsigned char> host;     // the blob as uploaded
    DevBuf<unsigned char> dev;
    const depthapply::Head& head() const { return *reinterpret_cast<const depthapply::Head*>(host.data()); }
};

namespace depthapply {

struct Image {                           // one image of an undistort call
    const void* in;
    size_t in_step;
    float* out;
    size_t out_step;
    int sensor, pad;
};

__global__ __launch_bounds__(vmap::kTrainThreads) void k_depth_undistort(const Image* __restrict__ images, const unsigned char* __restrict__ blob, int depth_type,
                                                                          int rows, int cols) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.x * vmap::kTrainTile + (wave & 1) * 8 + (lane & 7), v = blockIdx.y * vmap::kTrainTile + (wave >> 1) * 8 + (lane >> 3);
    if (u >= cols || v >= rows) return;
    const Image im = images[blockIdx.z];
    const unsigned char* line = static_cast<const unsigned char*>(im.in) + (size_t)v * im.in_step;
    float z = depth_type == 0 ? metres_convert_to(reinterpret_cast<const unsigned short*>(line)[u]) : reinterpret_cast<const float*>(line)[u];
    if (blob) z = apply_px(blob, im.sensor, v, u, z);
    reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(im.out) + (size_t)v * im.out_step)[u] = z;
}

// the correction of image k S + s by sensor s's model (rigc::pinhole_pixel); a corrected z that is not finite and positive is none
struct RigCorrection {
    static constexpr bool kOn = true;
    const unsigned char* blob;
    int n_sensors;
    __device__ bool operator()(int image, int v, int u, float& z) const {
        z = apply_px(blob, image % n_sensors, v, u, z);
        return z > 0.f && z < __builtin_inff();
    }
};
__global__ __launch_bounds__(256) void k_rig_cloud_models(const rigc::Image* __restrict__ images, const unsigned char* __restrict__ blob, int n_sensors,
                                                           int depth_type, int rows, int cols, float fx, float fy, float cx, float cy, float* __restrict__ out) {
    rigc::pinhole_pixel(images, depth_type, rows, cols, fx, fy, cx, cy, out, RigCorrection{blob, n_sensors});
}

enum { kEvN, kEvRawE, kEvRawEE, kEvCorE, kEvCorEE, kEvWords };      // rgbd360_depth_eval_sums in its order
constexpr double kEvalFix = 1073741824.0;                           // 2^30

}  // namespace depthapply

namespace vmap {

struct EvalJob {
    const unsigned char* blob;           // null: no set, the corrected depth is the raw one
    int sensor;
    unsigned long long* sums;            // [depthapply::kEvWords]
};

// k_depth_train<true, LAYER>'s pixel (its tile, its gates, its counters: the functions that kernel calls), with the example judged
// instead of added to a trainer's sums.  J.stats are the counters; J.sums, J.form and J.gt_out are not read.
template <bool LAYER>
__global__ __launch_bounds__(kTrainThreads) void k_depth_eval(TrainJob J, EvalJob E) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.x * kTrainTile + (wave & 1) * 8 + (lane & 7), v = blockIdx.y * kTrainTile + (wave >> 1) * 8 + (lane >> 3);
    const bool in = u < J.cols && v < J.rows;
    const TrainPixel px = train_gates<true, LAYER>(J, v, u, in);       // (an example is not added to a trainer's sums here: no bin, no terms)
    long long ev[depthapply::kEvWords] = {0ll, 0ll, 0ll, 0ll, 0ll};
    if (px.example) {
        const double gt = (double)px.gt32, meas = (double)px.meas32;
        const float zc = E.blob ? depthapply::apply_px(E.blob, E.sensor, v, u, px.meas32) : px.meas32;
        const double e_raw = meas - gt, e_cor = (double)zc - gt;
        ev[depthapply::kEvN] = 1ll;
        ev[depthapply::kEvRawE] = __double2ll_rn(e_raw * depthapply::kEvalFix);
        ev[depthapply::kEvRawEE] = __double2ll_rn(e_raw * e_raw * depthapply::kEvalFix);
        ev[depthapply::kEvCorE] = __double2ll_rn(e_cor * depthapply::kEvalFix);
        ev[depthapply::kEvCorEE] = __double2ll_rn(e_cor * e_cor * depthapply::kEvalFix);
    }
    if (__ballot(px.example)) {          // (the wave's lanes alike)
#pragma unroll
        for (int q = 0; q < depthapply::kEvWords; ++q) {
            long long s = ev[q];
#pragma unroll
            for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
            if (lane == 0 && s) atomicAdd(E.sums + q, (unsigned long long)s);      // one add per wave and word
        }
    }
    train_counters(J.stats, lane, in, px.cat);
}

}  // namespace vmap

namespace {

static_assert(depthapply::kMaxSensors == RGBD360_RIG_CALIB_MAX_SENSORS, "a set holds a rig's sensors");
static_assert(sizeof(rgbd360_depth_eval_sums) == depthapply::kEvWords * sizeof(long long), "the sums are the words in their order");

template <class Owner>
int rig_depth_launch(Owner* o, hipStream_t stream, const rgbd360_depth_models* set, const rigc::Image* images, int n_inputs, int n_sensors, int depth_type, int rows,
                     int cols, float fx, float fy, float cx, float cy, float* out) {
    const long long n = (long long)rows * cols;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)n_inputs);
    if (set)
        hipLaunchKernelGGL(depthapply::k_rig_cloud_models, grid, dim3(256), 0, stream, images, set->dev.get(), n_sensors, depth_type, rows, cols, fx, fy, cx, cy, out);
    else
        hipLaunchKernelGGL(rigc::k_rig_pinhole_cloud, grid, dim3(256), 0, stream, images, depth_type, rows, cols, fx, fy, cx, cy, out);
    HIPC(o, hipGetLastError());
    return 0;
}

// what every entry refuses of a set next to its images: the reason, or null
const char* da_set_refusal(const rgbd360_depth_models* set, const F360State* s, int rows, int cols) {
    if (!set) return nullptr;
    if (set->s != s) return "the set of depth models belongs to another context";
    const depthapply::Head& H = set->head();
    if (H.width && (long long)rows * cols > 0 && (rows != H.height || cols != H.width)) return "the images are not of the set's size";
    return nullptr;
}
// measurement: the events around the kernel of an entry (rgbd360_depth_apply_timing)
void da_mark(F360State* ctx, int which) {
    if (!ctx->da_timing) return;
    hipEventRecord(ctx->da_ev[which], ctx->stream);
    ctx->da_timed = which == 1;
}
int da_upload(rgbd360_depth_models* set, F360State* ctx) {
    hipSetDevice(ctx->p.device);
    HIPC(ctx, set->dev.ensure(set->host.size()));
    HIPC(ctx, hipMemcpyAsync(set->dev, set->host.data(), set->host.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));      // (`host` is pageable)
    return 0;
}

}  // namespace

extern "C" int rgbd360_depth_models_create(rgbd360_ctx* ctx_, const rgbd360_depth_model* const* models, int n_sensors, rgbd360_depth_models** out) {
    if (out) *out = nullptr;
    if (!ctx_ || !out) return -1;
    F360_ENTER(ctx_);
    if (!models) return fail(ctx, -1, "rgbd360_depth_models_create: models must not be null");
    try {
        std::unique_ptr<rgbd360_depth_models> set(new rgbd360_depth_models());
        set->ctx = ctx_, set->s = ctx;
        size_t bytes = 0;
        if (rgbd360_depth_models_pack(models, n_sensors, nullptr, &bytes) != 0)
            return fail(ctx, -1, "rgbd360_depth_models_create: 1 .. RGBD360_RIG_CALIB_MAX_SENSORS sensors, models of one width x height, at most 1 GiB packed");
        set->host.resize(bytes);
        if (rgbd360_depth_models_pack(models, n_sensors, set->host.data(), &bytes) != 0) return fail(ctx, -1, "rgbd360_depth_models_create: packing failed");
        if (const int rc = da_upload(set.get(), ctx)) return rc;
        *out = set.release();
        return 0;
    } catch (const std::exception&) {
        return fail(ctx, -103, "rgbd360_depth_models_create: out of memory");
    }
}
extern "C" void rgbd360_depth_models_destroy(rgbd360_depth_models* set) {
    if (!set) return;
    hipSetDevice(set->s->p.device);
    hipStreamSynchronize(set->s->stream);
    delete set;
}
extern "C" size_t rgbd360_depth_models_bytes(const rgbd360_depth_models* set) { return set ? set->host.size() : 0; }
extern "C" int rgbd360_depth_models_set(rgbd360_depth_models* set, int sensor, const rgbd360_depth_model* model) {
    if (!set) return -1;
    F360_ENTER(set->ctx);
    try {
        size_t bytes = 0;
        if (rgbd360_depth_models_repack(set->host.data(), sensor, model, nullptr, &bytes) != 0)
            return fail(ctx, -1, "rgbd360_depth_models_set: sensor outside the set, a model of another width x height, or more than 1 GiB packed");
        std::vector<unsigned char> blob(bytes);
        if (rgbd360_depth_models_repack(set->host.data(), sensor, model, blob.data(), &bytes) != 0) return fail(ctx, -1, "rgbd360_depth_models_set: packing failed");
        hipSetDevice(ctx->p.device);
        HIPC(ctx, hipStreamSynchronize(ctx->stream));      // (no launch reads the old blob any more)
        set->host.swap(blob);
        return da_upload(set, ctx);
    } catch (const std::exception&) {
        return fail(ctx, -103, "rgbd360_depth_models_set: out of memory");
    }
}

extern "C" int rgbd360_depth_undistort(rgbd360_ctx* ctx_, const rgbd360_depth_models* set, const rgbd360_map_batch_frame* images, const int* sensor_of_image,
                                       int n_images, int depth_type, int rows, int cols, int on_device, float* const* out_m, size_t out_step) {
    if (!ctx_) return -1;
    F360_ENTER(ctx_);
    if (n_images < 0 || n_images > 65535) return fail(ctx, -1, "rgbd360_depth_undistort: n_images must lie in 0 .. 65535");
    if (depth_type != 0 && depth_type != 1) return fail(ctx, -1, "rgbd360_depth_undistort: bad depth type");
    if (rows < 0 || cols < 0 || (long long)rows * cols >= (1ll << 30)) return fail(ctx, -1, "rgbd360_depth_undistort: bad image size");
    if (const char* why = da_set_refusal(set, ctx, rows, cols)) return fail(ctx, -1, why);
    const size_t n = (size_t)rows * (size_t)cols;
    if (n_images == 0 || n == 0) return 0;
    if (!images || !out_m || (set && !sensor_of_image)) return fail(ctx, -1, "rgbd360_depth_undistort: images, out_m and (with a set) sensor_of_image must not be null");
    const size_t prow = (size_t)cols * (depth_type == 0 ? 2 : 4), orow = (size_t)cols * 4;
    if (out_step < orow) return fail(ctx, -1, "rgbd360_depth_undistort: row step shorter than a row");
    size_t upload = 0;
    for (int i = 0; i < n_images; ++i) {
        if (!images[i].depth || !out_m[i]) return fail(ctx, -1, "rgbd360_depth_undistort: an image must not be null");
        if (images[i].depth_step < prow) return fail(ctx, -1, "rgbd360_depth_undistort: row step shorter than a row");
        if (set && (sensor_of_image[i] < 0 || sensor_of_image[i] >= set->head().n_sensors)) return fail(ctx, -1, "rgbd360_depth_undistort: sensor_of_image outside the set");
        if (!on_device) upload = batch_align256(upload + prow * (size_t)rows);
    }
    if (upload > kBatchMaxUpload || (!on_device && n * (size_t)n_images * 4 > kBatchMaxUpload))
        return fail(ctx, -1, "rgbd360_depth_undistort: the host images of the call exceed RGBD360_MAP_BATCH_MAX_UPLOAD bytes");
    hipSetDevice(ctx->p.device);
    hipStream_t stream = ctx->stream;
    const size_t desc = sizeof(depthapply::Image) * (size_t)n_images;
    HIPC(ctx, ctx->da_img.ensure(desc));
    HIPC(ctx, ctx->da_img_host.ensure(desc));
    if (!on_device) {
        HIPC(ctx, ctx->da_up.ensure(upload));
        HIPC(ctx, ctx->da_out.ensure(n * (size_t)n_images));
    }
    depthapply::Image* hi = reinterpret_cast<depthapply::Image*>(ctx->da_img_host.get());
    size_t at = 0;
    for (int i = 0; i < n_images; ++i) {
        hi[i] = {images[i].depth, images[i].depth_step, out_m[i], out_step, set ? sensor_of_image[i] : 0, 0};
        if (!on_device) {
            uint8_t* dst = ctx->da_up.get() + at;
            HIPC(ctx, hipMemcpy2DAsync(dst, prow, images[i].depth, images[i].depth_step, prow, (size_t)rows, hipMemcpyHostToDevice, stream));
            hi[i].in = dst, hi[i].in_step = prow;
            hi[i].out = ctx->da_out.get() + (size_t)i * n, hi[i].out_step = orow;
            at = batch_align256(at + prow * (size_t)rows);
        }
    }
    HIPC(ctx, hipMemcpyAsync(ctx->da_img, ctx->da_img_host, desc, hipMemcpyHostToDevice, stream));
    const dim3 grid((unsigned)((cols + vmap::kTrainTile - 1) / vmap::kTrainTile), (unsigned)((rows + vmap::kTrainTile - 1) / vmap::kTrainTile), (unsigned)n_images);
    da_mark(ctx, 0);
    hipLaunchKernelGGL(depthapply::k_depth_undistort, grid, dim3(vmap::kTrainThreads), 0, stream, reinterpret_cast<const depthapply::Image*>(ctx->da_img.get()),
                       set ? set->dev.get() : (const unsigned char*)nullptr, depth_type, rows, cols);
    da_mark(ctx, 1);
    HIPC(ctx, hipGetLastError());
    for (int i = 0; i < n_images && !on_device; ++i)
        HIPC(ctx, hipMemcpy2DAsync(out_m[i], out_step, ctx->da_out.get() + (size_t)i * n, orow, orow, (size_t)rows, hipMemcpyDeviceToHost, stream));
    HIPC(ctx, hipStreamSynchronize(stream));
    return 0;
}

extern "C" int rgbd360_rig_depth_clouds(rgbd360_ctx* ctx_, const rgbd360_depth_models* set, const rgbd360_map_batch_frame* images, int n_frames, int n_sensors,
                                        int depth_type, int rows, int cols, float fx, float fy, float cx, float cy, int on_device, float* xyz_out_dev) {
    if (!ctx_) return -1;
    F360_ENTER(ctx_);
    if (n_frames < 1 || n_sensors < 1 || n_sensors > RGBD360_RIG_CALIB_MAX_SENSORS || (long long)n_frames * n_sensors > RGBD360_MAP_BATCH_MAX)
        return fail(ctx, -1, "rgbd360_rig_depth_clouds: n_frames >= 1, n_sensors in 1 .. RGBD360_RIG_CALIB_MAX_SENSORS, their product at most RGBD360_MAP_BATCH_MAX");
    if (!images) return fail(ctx, -1, "rgbd360_rig_depth_clouds: images must not be null");
    if (set && set->s == ctx && set->head().n_sensors != n_sensors) return fail(ctx, -1, "rgbd360_rig_depth_clouds: n_sensors is not the set's");
    const int n_inputs = n_frames * n_sensors;
    unsigned long long upload = 0;
    if (const char* why = rig_depth_refusal(images, n_inputs, depth_type, rows, cols, fx, fy, cx, cy, on_device, upload)) return fail(ctx, -1, why);
    if (const char* why = da_set_refusal(set, ctx, rows, cols)) return fail(ctx, -1, why);
    if ((long long)rows * cols == 0) return 0;
    if (!xyz_out_dev) return fail(ctx, -1, "rgbd360_rig_depth_clouds: xyz_out_dev must not be null");
    hipSetDevice(ctx->p.device);
    if (const int rc = rig_depth_stage(ctx, ctx->stream, images, n_inputs, depth_type, rows, cols, on_device, upload, ctx->da_up, ctx->da_img, ctx->da_img_host)) return rc;
    da_mark(ctx, 0);
    if (const int rc = rig_depth_launch(ctx, ctx->stream, set, reinterpret_cast<const rigc::Image*>(ctx->da_img.get()), n_inputs, n_sensors, depth_type, rows, cols, fx,
                                        fy, cx, cy, xyz_out_dev))
        return rc;
    da_mark(ctx, 1);
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int rgbd360_map_calibrate_rig_depth_models(rgbd360_map* m, const rgbd360_depth_models* set, const rgbd360_map_batch_frame* depth, int depth_type,
                                                      int rows, int cols, float fx, float fy, float cx, float cy, int n_frames, int n_sensors, int on_device,
                                                      float* poses, float* extrinsics, const rgbd360_rig_calib_params* params, rgbd360_rig_calib_result* result,
                                                      rgbd360_rig_calib_sensor* sensors) {
    if (!m) return -1;
    m->err.clear();
    if (const char* why = da_set_refusal(set, m->s, rows, cols)) return vmap_fail(m, -1, why);
    if (set && set->head().n_sensors != n_sensors) return vmap_fail(m, -1, "n_sensors is not the set's");
    return rig_calibrate_depth(m, set, depth, depth_type, rows, cols, fx, fy, cx, cy, n_frames, n_sensors, on_device, poses, extrinsics, params, result, sensors);
}

extern "C" int rgbd360_depth_evaluate_map(rgbd360_ctx* ctx_, rgbd360_map* m, const rgbd360_depth_models* set, int sensor, const void* meas, size_t meas_step,
                                          int depth_type, int rows, int cols, float fx, float fy, float cx, float cy, const float sensor_pose[16], int on_device,
                                          const rgbd360_depth_train_params* params, rgbd360_depth_train_stats* stats, rgbd360_depth_eval_sums* sums) {
    if (!ctx_) return -1;
    F360_ENTER(ctx_);
    if (!m) return fail(ctx, -1, "rgbd360_depth_evaluate_map: map must not be null");
    m->err.clear();
    // the trainer's own checks and job, on a trainer of the image's size that holds nothing: what accumulate_map refuses is refused here
    rgbd360_depth_trainer t;
    t.ctx = ctx_, t.s = ctx, t.width = cols, t.height = rows;
    const auto refuse = [&](int rc) {
        ctx->err = "rgbd360_depth_evaluate_map: " + t.err;
        return rc;
    };
    rgbd360_depth_train_params p;
    if (params) p = *params;
    else rgbd360_depth_default_train_params(m, &p);
    const int chk = train_check(&t, p, meas, meas_step, depth_type, rows, cols);
    if (chk < 0) return refuse(chk);
    if (const int rc = train_check_map(&t, m, p, fx, fy, cx, cy, sensor_pose)) return refuse(rc);
    if ((long long)rows * cols > (1ll << 24)) return fail(ctx, -1, "rgbd360_depth_evaluate_map: more than 2^24 pixels in one call");
    if (const char* why = da_set_refusal(set, ctx, rows, cols)) return fail(ctx, -1, why);
    if (set && (sensor < 0 || sensor >= set->head().n_sensors)) return fail(ctx, -1, "rgbd360_depth_evaluate_map: sensor outside the set");
    vmap::TrainJob J = {};
    if (chk == 0) J = train_job(&t, p, meas, meas_step, depth_type);
    if (const int rc = train_map_job(&t, m, p, fx, fy, cx, cy, sensor_pose, J, false)) return refuse(rc);      // (the parameters alone)
    train_fill_stats(nullptr, stats);
    if (sums) memset(sums, 0, sizeof(*sums));
    if (chk == 1 || m->n_voxels == 0) return 0;      // no pixels, or nothing to hit: no kernel
    hipSetDevice(ctx->p.device);
    hipStream_t stream = ctx->stream;
    if (const int rc = train_map_job(&t, m, p, fx, fy, cx, cy, sensor_pose, J, true)) return refuse(rc);
    if (const int rc = train_image(&t, ctx->da_up, meas, meas_step, depth_type, rows, cols, on_device)) return refuse(rc);
    J.meas = meas, J.meas_step = meas_step;
    constexpr int kWords = vmap::kTrWords + depthapply::kEvWords;
    HIPC(ctx, ctx->da_words.ensure(kWords));
    HIPC(ctx, ctx->da_words_host.ensure(kWords));
    da_mark(ctx, 0);      // (the clear of the counters counts, as in rgbd360_depth_trainer_time_map)
    HIPC(ctx, hipMemsetAsync(ctx->da_words, 0, kWords * sizeof(unsigned long long), stream));
    J.stats = ctx->da_words;
    const vmap::EvalJob E = {set ? set->dev.get() : (const unsigned char*)nullptr, sensor, ctx->da_words.get() + vmap::kTrWords};
    const dim3 grid((unsigned)((cols + vmap::kTrainTile - 1) / vmap::kTrainTile), (unsigned)((rows + vmap::kTrainTile - 1) / vmap::kTrainTile));
    if (!m->rc_plain) hipLaunchKernelGGL(vmap::k_depth_eval<true>, grid, dim3(vmap::kTrainThreads), 0, stream, J, E);
    else hipLaunchKernelGGL(vmap::k_depth_eval<false>, grid, dim3(vmap::kTrainThreads), 0, stream, J, E);
    da_mark(ctx, 1);
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, hipMemcpyAsync(ctx->da_words_host, ctx->da_words, kWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIPC(ctx, hipStreamSynchronize(stream));
    train_fill_stats(ctx->da_words_host, stats);
    if (sums) memcpy(sums, ctx->da_words_host.get() + vmap::kTrWords, sizeof(*sums));
    return 0;
}

// measurement (rgbd360_hip_diag.h)
extern "C" int rgbd360_depth_apply_timing(rgbd360_ctx* ctx_, int on) {
    if (!ctx_) return -1;
    F360_ENTER(ctx_);
    hipSetDevice(ctx->p.device);
    if (on)
        for (hipEvent_t& e : ctx->da_ev)
            if (!e) HIPC(ctx, hipEventCreate(&e));
    ctx->da_timing = on != 0;
    ctx->da_timed = false;
    return 0;
}
extern "C" int rgbd360_depth_apply_last_us(rgbd360_ctx* ctx_, float* us) {
    if (!ctx_ || !us) return -1;
    F360_ENTER(ctx_);
    if (!ctx->da_timing || !ctx->da_timed) return fail(ctx, -1, "no timed call (rgbd360_depth_apply_timing(ctx, 1) first)");
    hipSetDevice(ctx->p.device);
    HIPC(ctx, hipEventSynchronize(ctx->da_ev[1]));
    float ms = 0.f;
    HIPC(ctx, hipEventElapsedTime(&ms, ctx->da_ev[0], ctx->da_ev[1]));
    *us = ms * 1000.f;
    return 0;
}
extern "C" int rgbd360_depth_apply_time_copy(rgbd360_ctx* ctx_, void* dst_dev, const void* src_dev, size_t bytes, float* us) {
    if (!ctx_ || !us) return -1;
    F360_ENTER(ctx_);
    if (!dst_dev || !src_dev || !ctx->da_timing) return fail(ctx, -1, "rgbd360_depth_apply_time_copy: null pointers, or timing is off");
    hipSetDevice(ctx->p.device);
    da_mark(ctx, 0);
    HIPC(ctx, hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    da_mark(ctx, 1);
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return rgbd360_depth_apply_last_us(ctx_, us);
}
#endif
