// rgbd360/FrameStore.hpp -- RAII wrapper of the resident frame store (rgbd360_store_*, ../rgbd360_hip.h): frames prepared once in
// HBM, arbitrary (target entry, source entry, guess) triples aligned in lock step.  Header-only, depends on the C ABI and on the
// PODs of RegisterPhotoICP.hpp.  The call patterns it serves: one keyframe against every following frame
// (OdometryKeyFrame360.cpp:244-253), the nearest keyframe against the current frame (KFsphere_SLAM.cpp:146-150, 370-375), a new
// keyframe against several old ones in both roles with one PbMap guess per candidate (LoopClosure360.h:309-312, 348-351).
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include "RegisterPhotoICP.hpp"

namespace rgbd360 {

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

    rgbd360_store* handle() { return st_; }

   private:
    void check(int rc, const char* what) {
        if (rc != 0) throw std::runtime_error(std::string(what) + " (" + std::to_string(rc) + "): " + rgbd360_store_last_error(st_));
    }
    rgbd360_store* st_ = nullptr;
    int capacity_ = 0;
};

}  // namespace rgbd360
