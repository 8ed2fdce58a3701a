// rgbd360/FrameStore.hpp -- RAII wrapper of the resident frame store (rgbd360_store_*, ../rgbd360_hip.h): frames prepared once in
// HBM, arbitrary (target entry, source entry, guess) triples aligned in lock step.  Header-only, depends on the C ABI and on the
// PODs of RegisterPhotoICP.hpp.  The call patterns it serves: one keyframe against every following frame
// (OdometryKeyFrame360.cpp:244-253), the nearest keyframe against the current frame (KFsphere_SLAM.cpp:146-150, 370-375), a new
// keyframe against several old ones in both roles with one PbMap guess per candidate (LoopClosure360.h:309-312, 348-351).
// And which pairs to align at all: the sensed-space overlap of stored frames (overlap / overlapMatrix) with the host-side candidate
// selection (overlapScore / overlapCandidates / overlapRepresentative; LoopClosure360.h:321, 360, TopologicalMap360.h:107-131, 216-234).
#pragma once

#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "RegisterPhotoICP.hpp"

namespace rgbd360 {

// An overlap matrix as rgbd360_store_overlap_all returns it: records[a * n + b] = target entries[a], source entries[b].
struct OverlapMatrix {
    int n = 0;
    std::vector<rgbd360_overlap> records;
    std::vector<Mat4f> rel_poses;      // W_a^-1 W_b of every pair, as the library formed them
    const rgbd360_overlap& at(int a, int b) const { return records[(size_t)a * n + b]; }
    const Mat4f& relPose(int a, int b) const { return rel_poses[(size_t)a * n + b]; }
};
struct OverlapCandidate {
    int a, b;
    float score;
};

// Host side (no device).  m: n x n records; level_px: the pixels of the level the matrix was made at.
inline float overlapScore(const std::vector<rgbd360_overlap>& m, int n, int level_px, int a, int b) {
    float s = 0.f;
    const rgbd360_overlap &ab = m.at((size_t)a * n + b), &ba = m.at((size_t)b * n + a);
    if (ab.evaluated && ba.evaluated) s = (float)(ab.n_consistent < ba.n_consistent ? ab.n_consistent : ba.n_consistent) / (float)level_px;
    return s;
}
// known: edges (either orientation) to leave out; max_per_frame <= 0: no limit.  In the order of rgbd360_overlap_candidates.
inline std::vector<OverlapCandidate> overlapCandidates(const std::vector<rgbd360_overlap>& m, int n, int level_px, float min_score, int min_gap,
                                                       int max_per_frame, const std::vector<std::pair<int, int>>& known) {
    if (n < 0 || m.size() != (size_t)n * n) throw std::runtime_error("overlapCandidates: the matrix must hold n x n records");
    std::vector<int> ka, kb;
    for (const auto& e : known) {
        ka.push_back(e.first);
        kb.push_back(e.second);
    }
    const int cap = n * (n - 1) / 2;
    std::vector<int> a(cap + 1), b(cap + 1);
    std::vector<float> s(cap + 1);
    const int found = rgbd360_overlap_candidates(n, m.data(), level_px, min_score, min_gap, max_per_frame, (int)known.size(), ka.data(), kb.data(), cap,
                                                 a.data(), b.data(), s.data());
    if (found < 0) throw std::runtime_error("rgbd360_overlap_candidates: bad arguments");
    std::vector<OverlapCandidate> out;
    for (int k = 0; k < found && k < cap; ++k) out.push_back(OverlapCandidate{a[k], b[k], s[k]});
    return out;
}
inline int overlapRepresentative(const std::vector<rgbd360_overlap>& m, int n, int level_px, const std::vector<int>& subset) {
    if (n < 1 || m.size() != (size_t)n * n) throw std::runtime_error("overlapRepresentative: the matrix must hold n x n records");
    const int r = rgbd360_overlap_representative(n, m.data(), level_px, subset.data(), (int)subset.size());
    if (r < 0) throw std::runtime_error("rgbd360_overlap_representative: bad arguments");
    return r;
}

class FrameStore {
   public:
    struct Pair {
        int target, source;
    };
    // The store takes align's parameters (pyramid levels, depth range, ...) as they are NOW: configure `align` first, and keep it
    // alive (and its setters untouched) for the lifetime of the store.
    FrameStore(RegisterPhotoICP& align, int capacity, int rows, int cols) : capacity_(capacity) {
        rgbd360_ctx* ctx = align.context();
        const int rc = rgbd360_store_create(ctx, capacity, rows, cols, &st_);
        if (rc != 0) throw std::runtime_error("rgbd360_store_create (" + std::to_string(rc) + "): " + rgbd360_last_error(ctx));
    }
    ~FrameStore() { rgbd360_store_destroy(st_); }
    FrameStore(const FrameStore&) = delete;
    FrameStore& operator=(const FrameStore&) = delete;

    int capacity() const { return capacity_; }
    size_t entryBytes() const { return rgbd360_store_entry_bytes(st_); }
    bool occupied(int entry) const { return rgbd360_store_occupied(st_, entry) == 1; }

    // Host images (all of one depth type and with the same row steps), prepared together; they are free when the call returns.
    void put(const std::vector<int>& entries, const std::vector<ImageView>& rgb, const std::vector<ImageView>& depth) {
        if (entries.size() != rgb.size() || rgb.size() != depth.size()) throw std::runtime_error("FrameStore::put: one entry, colour and depth image per frame");
        if (entries.empty()) return;
        std::vector<const uint8_t*> pr;
        std::vector<const void*> pd;
        for (size_t k = 0; k < rgb.size(); ++k) {
            if (rgb[k].type != ImageView::U8C3 || depth[k].type == ImageView::U8C3 || depth[k].type != depth[0].type ||
                rgb[k].step != rgb[0].step || depth[k].step != depth[0].step)
                throw std::runtime_error("FrameStore::put: frames of one call share types and row steps");
            pr.push_back((const uint8_t*)rgb[k].data);
            pd.push_back(depth[k].data);
        }
        check(rgbd360_store_put(st_, (int)entries.size(), entries.data(), pr.data(), rgb[0].step, pd.data(), depth[0].step,
                                depth[0].type == ImageView::U16C1 ? 0 : 1, 0),
              "rgbd360_store_put");
    }
    void put(int entry, const ImageView& rgb, const ImageView& depth) { put(std::vector<int>{entry}, {rgb}, {depth}); }

    // guesses: empty (identity for all) or one per pair.  Returns the poses in list order; results (optional) the full records.
    std::vector<Mat4f> align(const std::vector<Pair>& pairs, const std::vector<Mat4f>& guesses, int method = RGBD360_PHOTO_DEPTH,
                             int n_inflight = 32, std::vector<rgbd360_result>* results = nullptr) {
        if (!guesses.empty() && guesses.size() != pairs.size()) throw std::runtime_error("FrameStore::align: one guess per pair, or none");
        std::vector<int> t, s;
        for (const Pair& p : pairs) {
            t.push_back(p.target);
            s.push_back(p.source);
        }
        std::vector<Mat4f> poses(pairs.size());
        std::vector<rgbd360_result> res(pairs.size());
        if (pairs.empty()) {
            if (results) results->clear();
            return poses;
        }
        check(rgbd360_store_align(st_, (int)pairs.size(), t.data(), s.data(), guesses.empty() ? nullptr : guesses[0].m, method, 0, n_inflight,
                                  poses[0].m, res.data()),
              "rgbd360_store_align");
        if (results) *results = res;
        return poses;
    }

    // ---- sensed-space overlap (rgbd360_store_overlap*): level = the coarsest, tolerances 0.05 m + 0.02 D
    rgbd360_overlap_params overlapDefaultParams() const {
        rgbd360_overlap_params p;
        rgbd360_store_overlap_default_params(st_, &p);
        return p;
    }
    // poses (source in target): empty (identity for all) or one per pair.  One record per pair, in list order.
    std::vector<rgbd360_overlap> overlap(const std::vector<Pair>& pairs, const std::vector<Mat4f>& poses, const rgbd360_overlap_params& params) {
        if (!poses.empty() && poses.size() != pairs.size()) throw std::runtime_error("FrameStore::overlap: one pose per pair, or none");
        std::vector<int> t, s;
        for (const Pair& p : pairs) {
            t.push_back(p.target);
            s.push_back(p.source);
        }
        std::vector<rgbd360_overlap> out(pairs.size());
        check(rgbd360_store_overlap(st_, (int)pairs.size(), t.data(), s.data(), poses.empty() ? nullptr : poses[0].m, &params, out.data()),
              "rgbd360_store_overlap");
        return out;
    }
    // entries: distinct and occupied; world_poses (world <- frame): one per entry; max_translation <= 0: every pair a != b.
    OverlapMatrix overlapMatrix(const std::vector<int>& entries, const std::vector<Mat4f>& world_poses, float max_translation,
                                const rgbd360_overlap_params& params) {
        if (world_poses.size() != entries.size()) throw std::runtime_error("FrameStore::overlapMatrix: one world pose per entry");
        OverlapMatrix M;
        M.n = (int)entries.size();
        M.records.resize(entries.size() * entries.size());
        M.rel_poses.resize(M.records.size());
        if (entries.empty()) return M;
        check(rgbd360_store_overlap_all(st_, M.n, entries.data(), world_poses[0].m, max_translation, &params, M.records.data(), M.rel_poses[0].m),
              "rgbd360_store_overlap_all");
        return M;
    }

    rgbd360_store* handle() { return st_; }

   private:
    void check(int rc, const char* what) {
        if (rc != 0) throw std::runtime_error(std::string(what) + " (" + std::to_string(rc) + "): " + rgbd360_store_last_error(st_));
    }
    rgbd360_store* st_ = nullptr;
    int capacity_ = 0;
};

}  // namespace rgbd360
