// depth_model.h -- the intrinsic depth-distortion model Frame360::undistort applies to every sensor image before the clouds are built
// (include/Frame360.h:293-311, 1084-1097 -> calib->intrinsic_model_[sensor].undistort, Calib360.h:104-119): CLAMS'
// DiscreteDepthDistortionModel (Teichman et al.; vendored by the reference under OpenNI2_Grabber/third_party/CLAMS, files
// Calibration/Intrinsics/distortion_model1..8).  The image is cut into bins of bin_width x bin_height pixels; every bin holds a
// "frustum" of num_bins depth slices of bin_depth metres with a multiplier each; a measured z becomes z * m, m interpolated linearly
// between the two slices whose centres enclose z when both have seen at least 50 training examples, else the slice's own multiplier.
// File layout (restated from the reference's serialisation code): the line "DiscreteDepthDistortionModel v01", then raw little-endian
// scalars width, height, bin_width, bin_height (int32), bin_depth (float64), num_bins_x, num_bins_y (int32), then per frustum (row of
// bins after row of bins) max_dist (float64), num_bins (int32), bin_depth (float64) and four float32 vectors {counts, total numerators,
// total denominators, multipliers}, each written as {4, rows, cols} (int32) + data.  Host code; depth_apply.h packs these models for the
// device and restates slice_of / undistort_px below, operation for operation, as one __host__ __device__ function.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace depthmodel {

struct Frustum {
    double max_dist = 0, bin_depth = 0;
    int num_bins = 0;
    std::vector<float> counts, numerators, denominators, multipliers;      // the file's four vectors, all kept: load then save is the same file
};
struct Model {
    int width = 0, height = 0, bin_width = 0, bin_height = 0, num_bins_x = 0, num_bins_y = 0;
    double bin_depth = 0;
    std::vector<Frustum> frustums;      // [num_bins_y][num_bins_x]
};

inline bool read_exact(std::FILE* f, void* dst, size_t n) { return std::fread(dst, 1, n, f) == n; }
inline bool read_vec(std::FILE* f, std::vector<float>& v) {
    int32_t hdr[3];
    if (!read_exact(f, hdr, sizeof(hdr)) || hdr[0] != 4 || hdr[1] < 0 || hdr[2] < 0 || (long long)hdr[1] * hdr[2] > (1 << 20)) return false;
    v.resize((size_t)hdr[1] * hdr[2]);
    return v.empty() || read_exact(f, v.data(), v.size() * 4);
}
// 0 ok, 1 cannot open, 2 not a model file / truncated
inline int load(const char* path, Model& M) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return 1;
    int rc = 2;
    char line[64];
    static const char kMagic[] = "DiscreteDepthDistortionModel v01\n";
    do {
        if (!std::fgets(line, sizeof(line), f) || std::strcmp(line, kMagic) != 0) break;
        int32_t a[4], b[2];
        if (!read_exact(f, a, sizeof(a)) || !read_exact(f, &M.bin_depth, 8) || !read_exact(f, b, sizeof(b))) break;
        M.width = a[0]; M.height = a[1]; M.bin_width = a[2]; M.bin_height = a[3]; M.num_bins_x = b[0]; M.num_bins_y = b[1];
        if (M.width < 1 || M.height < 1 || M.bin_width < 1 || M.bin_height < 1 || M.num_bins_x < 1 || M.num_bins_y < 1 ||
            (long long)M.num_bins_x * M.num_bins_y > (1 << 22) || !(M.bin_depth > 0))
            break;
        M.frustums.assign((size_t)M.num_bins_x * M.num_bins_y, Frustum());
        bool ok = true;
        for (Frustum& F : M.frustums) {
            int32_t nb;
            ok = read_exact(f, &F.max_dist, 8) && read_exact(f, &nb, 4) && read_exact(f, &F.bin_depth, 8) && read_vec(f, F.counts) &&
                 read_vec(f, F.numerators) && read_vec(f, F.denominators) && read_vec(f, F.multipliers);
            if (!ok) break;
            F.num_bins = nb;
            ok = nb >= 1 && (int)F.counts.size() == nb && (int)F.multipliers.size() == nb && F.bin_depth > 0;      // (what undistort indexes)
            if (!ok) break;
        }
        if (ok) rc = 0;
    } while (false);
    std::fclose(f);
    return rc;
}
// DiscreteDepthDistortionModel::serialize / DiscreteFrustum::serialize: the layout above, every vector as {4, size, 1}.  0 ok, 1 cannot
// open or write
inline bool write_vec(std::FILE* f, const std::vector<float>& v) {
    const int32_t hdr[3] = {4, (int32_t)v.size(), 1};
    return std::fwrite(hdr, 1, sizeof(hdr), f) == sizeof(hdr) && (v.empty() || std::fwrite(v.data(), 4, v.size(), f) == v.size());
}
inline int save(const char* path, const Model& M) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return 1;
    const int32_t a[4] = {M.width, M.height, M.bin_width, M.bin_height}, b[2] = {M.num_bins_x, M.num_bins_y};
    bool ok = std::fputs("DiscreteDepthDistortionModel v01\n", f) >= 0 && std::fwrite(a, 1, sizeof(a), f) == sizeof(a) &&
              std::fwrite(&M.bin_depth, 1, 8, f) == 8 && std::fwrite(b, 1, sizeof(b), f) == sizeof(b);
    for (size_t k = 0; ok && k < M.frustums.size(); ++k) {
        const Frustum& F = M.frustums[k];
        const int32_t nb = F.num_bins;
        ok = std::fwrite(&F.max_dist, 1, 8, f) == 8 && std::fwrite(&nb, 1, 4, f) == 4 && std::fwrite(&F.bin_depth, 1, 8, f) == 8 && write_vec(f, F.counts) &&
             write_vec(f, F.numerators) && write_vec(f, F.denominators) && write_vec(f, F.multipliers);
    }
    ok = (std::fclose(f) == 0) && ok;
    return ok ? 0 : 1;
}
// The model of a training run's integer sums (csrc/depth_train.h; include/rgbd360_hip.h, "training the depth model"): the shape of
// DiscreteDepthDistortionModel's constructor (discrete_depth_distortion_model.cpp:116-139, DiscreteFrustum :10-19: max_dist 10, num_bins =
// ceil(10 / bin_depth)), count / num / den [num_bins_y][num_bins_x][num_bins] with num and den in units of 2^-20 m^2.  In float64:
// N = smoothing + num 2^-20, D = smoothing + den 2^-20, multiplier (float)(N / D) or 1 when D == 0, counts (float)(smoothing + count).
inline int train_num_bins(double bin_depth) { return (int)std::ceil(10.0 / bin_depth); }
inline bool from_sums(int width, int height, int bin_width, int bin_height, double bin_depth, int smoothing, const int64_t* count, const int64_t* num,
                      const int64_t* den, Model& M) {
    if (width < 1 || height < 1 || width > 16384 || height > 16384 || bin_width < 1 || bin_height < 1 || width % bin_width != 0 ||
        height % bin_height != 0 || !(bin_depth > 0) || !(10.0 / bin_depth <= 4096.0) || smoothing < 0)
        return false;
    M.width = width; M.height = height; M.bin_width = bin_width; M.bin_height = bin_height; M.bin_depth = bin_depth;
    M.num_bins_x = width / bin_width; M.num_bins_y = height / bin_height;
    const int nb = train_num_bins(bin_depth);
    M.frustums.assign((size_t)M.num_bins_x * M.num_bins_y, Frustum());
    for (size_t k = 0; k < M.frustums.size(); ++k) {
        Frustum& F = M.frustums[k];
        F.max_dist = 10.0; F.bin_depth = bin_depth; F.num_bins = nb;
        F.counts.resize((size_t)nb); F.numerators.resize((size_t)nb); F.denominators.resize((size_t)nb); F.multipliers.resize((size_t)nb);
        for (int i = 0; i < nb; ++i) {
            const size_t w = k * (size_t)nb + (size_t)i;
            if (count[w] < 0 || num[w] < 0 || den[w] < 0) return false;
            const double N = (double)smoothing + (double)num[w] * (1.0 / 1048576.0), D = (double)smoothing + (double)den[w] * (1.0 / 1048576.0);
            F.counts[(size_t)i] = (float)((double)smoothing + (double)count[w]);
            F.numerators[(size_t)i] = (float)N;
            F.denominators[(size_t)i] = (float)D;
            F.multipliers[(size_t)i] = D == 0.0 ? 1.f : (float)(N / D);
        }
    }
    return true;
}
// DiscreteDepthDistortionModel::downsampleParams: the model of the full-resolution sensor used on images `step` times smaller
inline bool downsample(Model& M, int step) {
    if (step < 1 || M.bin_width % step != 0 || M.bin_height % step != 0) return false;
    M.width /= step; M.height /= step; M.bin_width /= step; M.bin_height /= step;
    return true;
}
// DiscreteFrustum::index / undistort / interpolatedUndistort, operation for operation (float z, double interpolation weights)
inline int slice_of(const Frustum& F, float z) {
    const double q = std::floor((double)z / F.bin_depth);
    if (!(q < (double)(F.num_bins - 1))) return F.num_bins - 1;      // beyond the last slice, +Inf (and NaN, which undistort() never passes): no float -> int conversion out of range
    return q < 0 ? -1 : (int)q;
}
inline void undistort_px(const Frustum& F, float* z) {
    const int idx = slice_of(F, *z);
    const float start = (float)(F.bin_depth * idx);
    const int idx1 = ((double)(*z - start) < F.bin_depth / 2) ? idx : idx + 1;
    const int idx0 = idx1 - 1;
    if (idx0 < 0 || idx1 >= F.num_bins || F.counts[(size_t)idx0] < 50 || F.counts[(size_t)idx1] < 50) {
        *z *= F.multipliers[(size_t)(idx < 0 ? 0 : idx)];
        return;
    }
    const double z0 = (idx0 + 1) * F.bin_depth - F.bin_depth * 0.5;
    const double coeff1 = ((double)*z - z0) / F.bin_depth;
    const double coeff0 = 1.0 - coeff1;
    const double mult = coeff0 * (double)F.multipliers[(size_t)idx0] + coeff1 * (double)F.multipliers[(size_t)idx1];
    *z = (float)((double)*z * mult);
}
// DiscreteDepthDistortionModel::undistort on a rows x cols float32 image in metres (0 = no measurement), in place.  The reference
// loops over 240 x 320 whatever the model says; here the image has to be the model's size.
inline bool undistort(const Model& M, float* depth, size_t step_bytes, int rows, int cols) {
    if (rows != M.height || cols != M.width) return false;
    for (int v = 0; v < rows; ++v) {
        float* row = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(depth) + (size_t)v * step_bytes);
        const int yb = std::min(v / M.bin_height, M.num_bins_y - 1);
        for (int u = 0; u < cols; ++u) {
            if (row[u] == 0.f || !(row[u] > 0.f)) continue;      // (no measurement; a negative or NaN depth has no slice either)
            undistort_px(M.frustums[(size_t)yb * M.num_bins_x + (size_t)std::min(u / M.bin_width, M.num_bins_x - 1)], &row[u]);
        }
    }
    return true;
}

}  // namespace depthmodel
