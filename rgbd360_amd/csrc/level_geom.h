// level_geom.h -- the host-side definition of a pyramid level that every caller of the per-pixel pass shares: size checks, the
// spherical geometry constants, the angle tables and the work split of the pass.  The one-pair context (rgbd360_api.hip) and the
// lock-step engine (sequence_engine.h, and through it the rig and the frame store) build their levels from THESE functions, which
// is what makes their results agree bit for bit.  Host code; included by rgbd360_api.hip behind photo_icp_kernels.h.
#pragma once

#include <vector>

namespace {

// nullptr, or why an image of this size cannot be aligned with p.n_pyr levels
const char* check_image_size(const rgbd360_params& p, int rows, int cols) {
    if (rows < 2 || cols < 8) return "image too small";
    if ((rows >> (p.n_pyr - 1)) < 2 || (cols >> (p.n_pyr - 1)) < 8)
        return "too many pyramid levels for this image size (coarsest level must be >= 2 x 8)";
    if ((long long)rows * cols >= (1ll << 24) || rows >= (1 << 15) || cols >= (1 << 15))
        return "image too large (the fused pass uses 24-bit index arithmetic: < 16 Mpx)";
    return nullptr;
}

struct LevelGeom {
    int rows = 0, cols = 0, n = 0;
    float half_nRows = 0.f, angle_res_inv = 0.f;
    int chunk = 0, nblocks = 0;      // work split of the per-pixel pass: nblocks contiguous spans of chunk pixels
};

float level_angle_res(int cols) { return 2 * kPI / cols; }      // RPI.h:2554

LevelGeom level_geom(int rows, int cols, int max_eval_blocks) {
    LevelGeom g;
    g.rows = rows; g.cols = cols; g.n = rows * cols;
    const float angle_res = level_angle_res(cols);
    g.angle_res_inv = 1 / angle_res;            // RPI.h:2555
    g.half_nRows = 0.5 * rows - 0.5;            // RPI.h:2557
    // work split of the fused pass: <= max_eval_blocks blocks, contiguous spans that are multiples of kEvalThreads pixels
    int chunk = (g.n + max_eval_blocks - 1) / max_eval_blocks;
    chunk = ((chunk + kEvalThreads - 1) / kEvalThreads) * kEvalThreads;
    g.chunk = chunk;
    g.nblocks = (g.n + chunk - 1) / chunk;
    return g;
}

// grid of a stage kernel that runs one lane per pixel of the level, in blocks of `threads` lanes (warp_images.h)
dim3 level_pixel_grid(const LevelGeom& g, int threads) { return dim3((g.n + threads - 1) / threads); }

struct AngleTables {
    std::vector<float> st, ct, sp, cp;      // sin / cos of theta per column, of phi per row
    std::vector<float2> tt, tp;             // the same values interleaved {sin, cos}: one 8-byte load per pixel in the recompute forms of the pass
};

// RPI.h:4556-4571: per-column / per-row sin, cos of float arguments (host libm, once per size)
AngleTables angle_tables(const LevelGeom& g) {
    const int r = g.rows, c = g.cols;
    const float angle_res = level_angle_res(c);
    AngleTables t;
    t.st.resize(c); t.ct.resize(c); t.sp.resize(r); t.cp.resize(r); t.tt.resize(c); t.tp.resize(r);
    for (int j = 0; j < c; ++j) {
        float theta = j * angle_res;
        t.st[j] = sinf(theta);
        t.ct[j] = cosf(theta);
    }
    for (int i = 0; i < r; ++i) {
        float phi = (g.half_nRows - i) * angle_res;
        t.sp[i] = sinf(phi);
        t.cp[i] = cosf(phi);
    }
    for (int j = 0; j < c; ++j) t.tt[j] = make_float2(t.st[j], t.ct[j]);
    for (int i = 0; i < r; ++i) t.tp[i] = make_float2(t.sp[i], t.cp[i]);
    return t;
}

// the six arrays into device buffers of the caller (cols / rows elements each)
hipError_t upload_angle_tables(const AngleTables& t, float* sinT, float* cosT, float* sinP, float* cosP, float2* tabT, float2* tabP) {
    const struct { void* dst; const void* src; size_t bytes; } copies[6] = {
        {sinT, t.st.data(), t.st.size() * sizeof(float)},  {cosT, t.ct.data(), t.ct.size() * sizeof(float)},
        {sinP, t.sp.data(), t.sp.size() * sizeof(float)},  {cosP, t.cp.data(), t.cp.size() * sizeof(float)},
        {tabT, t.tt.data(), t.tt.size() * sizeof(float2)}, {tabP, t.tp.data(), t.tp.size() * sizeof(float2)}};
    for (const auto& c : copies) {
        const hipError_t e = hipMemcpy(c.dst, c.src, c.bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the geometry part of a level's kernel argument; the callers add their pointers
void fill_level_dev(LevelDev& d, const LevelGeom& g) {
    d.rows = g.rows; d.cols = g.cols; d.n = g.n;
    d.half_nRows = g.half_nRows; d.angle_res_inv = g.angle_res_inv;
    d.pi_k = (float)(kPI * (double)g.angle_res_inv);
}

}  // namespace
