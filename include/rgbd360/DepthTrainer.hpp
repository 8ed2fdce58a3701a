// DepthTrainer.hpp -- training the sensors' intrinsic depth models against the resident voxel map (rgbd360_depth_trainer_*, rgbd360_hip.h,
// "training the depth model"): the training half of clams::DiscreteDepthDistortionModel, which the reference vendors next to the half it
// uses (OpenNI2_Grabber/third_party/CLAMS/discrete_depth_distortion_model.cpp: addExample :21-36, accumulate :193-217) and whose files
// Calib360::loadIntrinsicCalibration reads (Calib360.h:104-119).
//
//   DepthTrainer      one sensor: the constructor of DiscreteDepthDistortionModel, accumulate(ground_truth, measurement), and
//                     accumulate(GlobalMap&, ...) with the ground truth cast out of the map
//   DepthTrainerRig   the eight sensors of a rig: accumulate(frame, pose, map) feeds every sensor's raw depth image with calib->K() and
//                     pose x calib->Rt_[s]; saveIntrinsicCalibration(dir) writes distortion_model1..8
//
// The sums are exact integers on the device: the order of the frames does not matter, and trainers of one shape are joined by addSums.
#pragma once

#include <array>
#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "Frame360.hpp"
#include "GlobalMap.hpp"

namespace rgbd360 {

class DepthTrainer {
   public:
    // DiscreteDepthDistortionModel(int width, int height, int bin_width = 8, int bin_height = 6, double bin_depth = 2.0, int smoothing = 1);
    // `align`: the context (device, stream) the trainer lives on -- that of the GlobalMap it is trained against
    DepthTrainer(RegisterPhotoICP& align, int width, int height, int bin_width = 8, int bin_height = 6, double bin_depth = 2.0, int smoothing = 1)
        : width_(width), height_(height), bin_width_(bin_width), bin_height_(bin_height), smoothing_(smoothing), bin_depth_(bin_depth) {
        rgbd360_ctx* ctx = align.context();
        const int rc = rgbd360_depth_trainer_create(ctx, width, height, bin_width, bin_height, bin_depth, smoothing, &t_);
        if (rc != 0) throw std::runtime_error("rgbd360_depth_trainer_create (" + std::to_string(rc) + "): " + rgbd360_last_error(ctx));
        num_bins_ = (size_t)(height / bin_height) * (size_t)(width / bin_width) * (size_t)std::ceil(10.0 / bin_depth);
    }
    ~DepthTrainer() { rgbd360_depth_trainer_destroy(t_); }
    DepthTrainer(const DepthTrainer&) = delete;
    DepthTrainer& operator=(const DepthTrainer&) = delete;

    int width() const { return width_; }
    int height() const { return height_; }
    size_t numBins() const { return num_bins_; }      // (frustum, slice) bins: the length of each of the three sum arrays

    // the defaults of `map` (or of no map: the image route needs none)
    rgbd360_depth_train_params params(GlobalMap* map = nullptr) const {
        rgbd360_depth_train_params p;
        rgbd360_depth_default_train_params(map ? map->handle() : nullptr, &p);
        return p;
    }

    // DiscreteDepthDistortionModel::accumulate(ground_truth, measurement): two images of the trainer's size and one type (16UC1 mm or 32FC1
    // m); returns the number of training examples, as the source does
    size_t accumulate(const ImageView& ground_truth, const ImageView& measurement, const rgbd360_depth_train_params* params = nullptr) {
        if (ground_truth.type != measurement.type || ground_truth.rows != measurement.rows || ground_truth.cols != measurement.cols)
            throw std::invalid_argument("DepthTrainer::accumulate: the two images must have one size and type");
        check(rgbd360_depth_trainer_accumulate_images(t_, ground_truth.data, ground_truth.step, measurement.data, measurement.step, depthType(measurement),
                                                      measurement.rows, measurement.cols, 0, params, &stats_),
              "rgbd360_depth_trainer_accumulate_images");
        return (size_t)stats_.n_examples;
    }
    // The ground truth cast out of `map`: K = {fx, fy, cx, cy}, sensorPose world <- sensor.  ground_truth (may be null): the cast depth of
    // the pixels that became candidates, rows x cols metres
    size_t accumulate(GlobalMap& map, const ImageView& measurement, const std::array<float, 4>& K, const Mat4f& sensorPose,
                      const rgbd360_depth_train_params* params = nullptr, std::vector<float>* ground_truth = nullptr) {
        if (ground_truth) ground_truth->assign((size_t)measurement.rows * measurement.cols, 0.f);
        check(rgbd360_depth_trainer_accumulate_map(t_, map.handle(), measurement.data, measurement.step, depthType(measurement), measurement.rows,
                                                   measurement.cols, K[0], K[1], K[2], K[3], sensorPose.m, 0, params,
                                                   ground_truth ? ground_truth->data() : nullptr, &stats_),
              "rgbd360_depth_trainer_accumulate_map");
        return (size_t)stats_.n_examples;
    }
    const rgbd360_depth_train_stats& stats() const { return stats_; }      // of the last accumulate

    void clear() { check(rgbd360_depth_trainer_clear(t_), "rgbd360_depth_trainer_clear"); }
    void sums(std::vector<int64_t>& count, std::vector<int64_t>& num, std::vector<int64_t>& den) const {
        count.resize(num_bins_), num.resize(num_bins_), den.resize(num_bins_);
        check(rgbd360_depth_trainer_sums(t_, count.data(), num.data(), den.data()), "rgbd360_depth_trainer_sums");
    }
    void addSums(const std::vector<int64_t>& count, const std::vector<int64_t>& num, const std::vector<int64_t>& den) {
        if (count.size() != num_bins_ || num.size() != num_bins_ || den.size() != num_bins_)
            throw std::invalid_argument("DepthTrainer::addSums: the sums of a trainer of another shape");
        check(rgbd360_depth_trainer_add_sums(t_, count.data(), num.data(), den.data()), "rgbd360_depth_trainer_add_sums");
    }
    // the model of the sums as they stand, as Calib360::intrinsic_model_ holds one
    std::shared_ptr<rgbd360_depth_model> model() const {
        rgbd360_depth_model* m = nullptr;
        check(rgbd360_depth_trainer_model(t_, &m), "rgbd360_depth_trainer_model");
        return std::shared_ptr<rgbd360_depth_model>(m, rgbd360_depth_model_free);
    }
    // DiscreteDepthDistortionModel::save.  upsamplingStep: the inverse of downsampleParams -- the file states the image and bin sizes of a
    // sensor `upsamplingStep` times larger (the same frustums), which is what a loader that calls downsampleParams(upsamplingStep) expects
    void save(const std::string& path, int upsamplingStep = 1) const {
        std::shared_ptr<rgbd360_depth_model> m = model();
        if (upsamplingStep != 1) {
            std::vector<int64_t> count, num, den;
            sums(count, num, den);
            rgbd360_depth_model* up = nullptr;
            if (upsamplingStep < 1 || rgbd360_depth_model_from_sums(width_ * upsamplingStep, height_ * upsamplingStep, bin_width_ * upsamplingStep,
                                                                    bin_height_ * upsamplingStep, bin_depth_, smoothing_, count.data(), num.data(), den.data(),
                                                                    &up) != 0)
                throw std::invalid_argument("DepthTrainer::save: bad upsamplingStep");
            m = std::shared_ptr<rgbd360_depth_model>(up, rgbd360_depth_model_free);
        }
        if (rgbd360_depth_model_save(m.get(), path.c_str()) != 0) throw std::runtime_error("DepthTrainer::save: cannot write " + path);
    }
    rgbd360_depth_trainer* handle() { return t_; }

   private:
    static int depthType(const ImageView& depth) { return depth.type == ImageView::U16C1 ? 0 : 1; }
    void check(int rc, const char* what) const {
        if (rc != 0) throw std::runtime_error(std::string(what) + " (" + std::to_string(rc) + "): " + rgbd360_depth_trainer_last_error(t_));
    }
    rgbd360_depth_trainer* t_ = nullptr;
    int width_, height_, bin_width_, bin_height_, smoothing_;
    double bin_depth_;
    size_t num_bins_ = 0;
    rgbd360_depth_train_stats stats_{};
};

// The eight sensors of a rig, trained against one map from posed frames.
class DepthTrainerRig {
   public:
    DepthTrainerRig(RegisterPhotoICP& align, int width, int height, int bin_width = 8, int bin_height = 6, double bin_depth = 2.0, int smoothing = 1) {
        for (auto& t : trainers_) t.reset(new DepthTrainer(align, width, height, bin_width, bin_height, bin_depth, smoothing));
    }
    DepthTrainer& sensor(int s) { return *trainers_.at((size_t)s); }

    // Every sensor's raw depth image (Frame360::sensorDepth: what the device delivered, before any undistort) against the map at
    // pose x calib->Rt_[s]; returns the examples of the eight sensors together.  total (may be null): their statistics added up
    size_t accumulate(const Frame360& frame, const Mat4f& pose, GlobalMap& map, const rgbd360_depth_train_params* params = nullptr,
                      rgbd360_depth_train_stats* total = nullptr) {
        const std::array<float, 4> K = frame.calib->K();
        size_t n = 0;
        for (int s = 0; s < 8; ++s) {
            n += trainers_[(size_t)s]->accumulate(map, frame.sensorDepth(s), K, multiply(pose, frame.calib->Rt_[(size_t)s]), params);
            if (total) {
                const rgbd360_depth_train_stats& st = trainers_[(size_t)s]->stats();
                total->n_pixels += st.n_pixels, total->n_no_measurement += st.n_no_measurement, total->n_no_hit += st.n_no_hit;
                total->n_off_plane += st.n_off_plane, total->n_grazing += st.n_grazing, total->n_out_of_range += st.n_out_of_range;
                total->n_mult_rejected += st.n_mult_rejected, total->n_examples += st.n_examples;
            }
        }
        return n;
    }
    // distortion_model1..8 in `pathToIntrinsicModel`, where Calib360::loadIntrinsicCalibration reads them.  That loader calls
    // downsampleParams(2) (Calib360.h:116: the files describe the full-resolution sensor, the rig delivers half-size images), so the files
    // state twice the size the trainers were fed with; downsamplingStep 1 writes the trainers' own size
    void saveIntrinsicCalibration(const std::string& pathToIntrinsicModel, int downsamplingStep = 2) const {
        for (int s = 0; s < 8; ++s) trainers_[(size_t)s]->save(pathToIntrinsicModel + "/distortion_model" + std::to_string(s + 1), downsamplingStep);
    }
    // the models as they stand into a calibration, for Frame360::undistort
    void install(Calib360& calib) const {
        for (int s = 0; s < 8; ++s) calib.intrinsic_model_[(size_t)s] = trainers_[(size_t)s]->model();
    }

    static Mat4f multiply(const Mat4f& A, const Mat4f& B) {
        Mat4f C{};
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) C(r, c) = ((A(r, 0) * B(0, c) + A(r, 1) * B(1, c)) + A(r, 2) * B(2, c)) + A(r, 3) * B(3, c);
        return C;
    }

    // the models as they stand, for DepthModels below
    std::vector<std::shared_ptr<rgbd360_depth_model>> models() const {
        std::vector<std::shared_ptr<rgbd360_depth_model>> out;
        for (const auto& t : trainers_) out.push_back(t->model());
        return out;
    }

   private:
    std::array<std::unique_ptr<DepthTrainer>, 8> trainers_;
};

// The depth models of a rig's sensors resident on the device (rgbd360_depth_models_*, rgbd360_hip.h, "applying the depth models on the
// device"): the step "undistort" of CLAMS' loop without leaving the device.  A null model means identity.  The set lives on `align`'s
// context: destroy it before the context.
class DepthModels {
   public:
    DepthModels(RegisterPhotoICP& align, const std::vector<std::shared_ptr<rgbd360_depth_model>>& models) : ctx_(align.context()), n_((int)models.size()) {
        std::vector<const rgbd360_depth_model*> raw;
        for (const auto& m : models) raw.push_back(m.get());
        const int rc = rgbd360_depth_models_create(ctx_, raw.data(), n_, &set_);
        if (rc != 0) throw std::runtime_error("rgbd360_depth_models_create (" + std::to_string(rc) + "): " + rgbd360_last_error(ctx_));
    }
    // the models a calibration holds (Calib360::loadIntrinsicCalibration, DepthTrainerRig::install)
    DepthModels(RegisterPhotoICP& align, const Calib360& calib)
        : DepthModels(align, std::vector<std::shared_ptr<rgbd360_depth_model>>(calib.intrinsic_model_.begin(), calib.intrinsic_model_.end())) {}
    ~DepthModels() { rgbd360_depth_models_destroy(set_); }
    DepthModels(const DepthModels&) = delete;
    DepthModels& operator=(const DepthModels&) = delete;

    int sensors() const { return n_; }
    size_t bytes() const { return rgbd360_depth_models_bytes(set_); }
    const rgbd360_depth_models* handle() const { return set_; }
    // one sensor's model replaced (null: identity), e.g. after a training round
    void set(int sensor, const rgbd360_depth_model* model) { check(rgbd360_depth_models_set(set_, sensor, model), "rgbd360_depth_models_set"); }

    // images[i] (host memory; 16UC1 mm, converted as Frame360::undistort converts, or 32FC1 m; one size and type) corrected by the model of
    // sensorOfImage[i] into out[i * rows * cols ..], float32 metres: one launch, one synchronisation
    void undistort(const std::vector<ImageView>& images, const std::vector<int>& sensorOfImage, std::vector<float>& out) const {
        if (images.empty() || images.size() != sensorOfImage.size()) throw std::invalid_argument("DepthModels::undistort: one sensor per image");
        std::vector<rgbd360_map_batch_frame> in = frames(images, "DepthModels::undistort");
        const size_t n = (size_t)images[0].rows * (size_t)images[0].cols;
        out.resize(n * images.size());
        std::vector<float*> dst(images.size());
        for (size_t i = 0; i < images.size(); ++i) dst[i] = out.data() + i * n;
        check(rgbd360_depth_undistort(ctx_, set_, in.data(), sensorOfImage.data(), (int)images.size(), depthType(images[0]), images[0].rows, images[0].cols, 0,
                                      dst.data(), (size_t)images[0].cols * 4),
              "rgbd360_depth_undistort");
    }
    // depths[k S + s] (host memory) into the corrected clouds of the sensors' frames in device memory (3 rows cols floats per image; NaN
    // triples without a measurement), ready for GlobalMap's device-memory inputs
    void rigClouds(const std::vector<ImageView>& depths, const std::array<float, 4>& K4, int n_frames, float* xyz_out_dev) const {
        if (depths.empty() || depths.size() != (size_t)n_frames * (size_t)n_) throw std::invalid_argument("DepthModels::rigClouds: one image per frame and sensor");
        std::vector<rgbd360_map_batch_frame> in = frames(depths, "DepthModels::rigClouds");
        check(rgbd360_rig_depth_clouds(ctx_, set_, in.data(), n_frames, n_, depthType(depths[0]), depths[0].rows, depths[0].cols, K4[0], K4[1], K4[2], K4[3], 0,
                                       xyz_out_dev),
              "rgbd360_rig_depth_clouds");
    }
    // `sensor`'s model judged on one image against the map: the sums of the raw and the corrected error over the trainer's examples
    // (add the sums of several images; rms() and bias() read them).  stats (may be null): the trainer's counters
    rgbd360_depth_eval_sums evaluate(GlobalMap& map, int sensor, const ImageView& measurement, const std::array<float, 4>& K, const Mat4f& sensorPose,
                                     const rgbd360_depth_train_params* params = nullptr, rgbd360_depth_train_stats* stats = nullptr) const {
        rgbd360_depth_eval_sums sums{};
        check(rgbd360_depth_evaluate_map(ctx_, map.handle(), set_, sensor, measurement.data, measurement.step, depthType(measurement), measurement.rows,
                                         measurement.cols, K[0], K[1], K[2], K[3], sensorPose.m, 0, params, stats, &sums),
              "rgbd360_depth_evaluate_map");
        return sums;
    }
    static void add(rgbd360_depth_eval_sums& total, const rgbd360_depth_eval_sums& s) {
        total.n += s.n, total.raw_e += s.raw_e, total.raw_ee += s.raw_ee, total.cor_e += s.cor_e, total.cor_ee += s.cor_ee;
    }
    // metres, of sums in units of 2^-30 m^2 and 2^-30 m
    static double rms(long long ee, long long n) { return n > 0 ? std::sqrt((double)ee / 1073741824.0 / (double)n) : 0.0; }
    static double bias(long long e, long long n) { return n > 0 ? (double)e / 1073741824.0 / (double)n : 0.0; }

   private:
    static int depthType(const ImageView& depth) { return depth.type == ImageView::U16C1 ? 0 : 1; }
    static std::vector<rgbd360_map_batch_frame> frames(const std::vector<ImageView>& images, const char* what) {
        std::vector<rgbd360_map_batch_frame> in(images.size());
        for (size_t k = 0; k < images.size(); ++k) {
            if (images[k].rows != images[0].rows || images[k].cols != images[0].cols || images[k].type != images[0].type)
                throw std::invalid_argument(std::string(what) + ": the images of a call share one size and depth type");
            in[k].depth = images[k].data;
            in[k].depth_step = images[k].step;
        }
        return in;
    }
    void check(int rc, const char* what) const {
        if (rc != 0) throw std::runtime_error(std::string(what) + " (" + std::to_string(rc) + "): " + rgbd360_last_error(ctx_));
    }
    rgbd360_ctx* ctx_;
    int n_;
    rgbd360_depth_models* set_ = nullptr;
};

}  // namespace rgbd360
