// PCR/HipRegister.hpp -- header-only C++ mirror of the reference's registration plugin over the
// C ABI of libpcr_hip.so (include/pcr_hip.h).  No PCL, no Eigen: the cloud and pose types below have
// the memory layout of the reference's (pcl::PointXYZI = 32 bytes, Eigen::Isometry3d = 16 doubles
// column-major), so an adapter for a tree that has PCL+Eigen only forwards pointers.
//
// Mirrors (reference): PCR/include/PCR/PointCloudRegister.hpp:12-38, LoamRegister.hpp, NdtRegister.hpp,
// VgicpRegister.hpp; the factory of frontend/src/LidarOdometry.cpp:44-54.
#pragma once
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <cstdio>

#include "../../../include/pcr_hip.h"
#include "../config/params.hpp"

namespace context { class ScanContext; }

namespace PCR {

using scalar_t = double;                       // common/types/basic.hpp:16

struct alignas(16) PointXYZI {                 // pcl::PointXYZI: x y z 1 | intensity pad pad pad
    float x = 0, y = 0, z = 0, w = 1.f;
    float intensity = 0, pad[3] = {0, 0, 0};
};
static_assert(sizeof(PointXYZI) == 32, "must match pcl::PointXYZI");

struct PointCloud {
    std::vector<PointXYZI> points;
    size_t size() const { return points.size(); }
};
using PC_Ptr = std::shared_ptr<PointCloud>;
using PC_cPtr = std::shared_ptr<const PointCloud>;

struct pose_t {                                // Eigen::Isometry3d: 4x4 column-major
    double m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    double* data() { return m; }
    const double* data() const { return m; }
    double& operator()(int r, int c) { return m[c * 4 + r]; }
    double operator()(int r, int c) const { return m[c * 4 + r]; }
};

class PointCloudRegister {
protected:
    bool isConverge = false;
    int cores = 1;                             // cfg["cores"]: OpenMP team of the CPU reference; the GPU path has no use for it
    std::string lastError_;
    // the reference logs through its spdlog singleton (`this->lg->error(...)`, LoamRegister.cpp:174); here: stderr
    void logError(const std::string& msg) { lastError_ = msg; std::fprintf(stderr, "[error] %s\n", msg.c_str()); }
public:
    using Ptr = std::shared_ptr<PointCloudRegister>;
    // PointCloudRegister.hpp:28-32: `cores = cfg["cores"].get<int>()` -- when a configuration has been loaded (config::Params::load)
    PointCloudRegister() { if (config::Params::loaded()) cores = config::Params::getInstance()["cores"].get<int>(); }
    int getCores() const { return cores; }
    const std::string& lastError() const { return lastError_; }
    virtual scalar_t getFitnessScore() { return 0; }
    virtual bool scan2Map(const PC_cPtr& src, const PC_cPtr& dst, pose_t& res) = 0;
    virtual ~PointCloudRegister() {}
};

// Common implementation: one pcr_handle per registrar (own HIP stream and buffers, so the odometry and the
// loop-closure registrars of the reference can run on their own threads concurrently).
class HipRegister : public PointCloudRegister {
protected:
    pcr_handle* h_ = nullptr;
    explicit HipRegister(const char* method, const pcr_params* p = nullptr) {
        h_ = pcr_create(method, p);
        if (!h_) throw std::runtime_error(pcr_last_error(nullptr));
    }
    // one int32 field of the live handle's parameters through pcr_get_params / pcr_set_params (a refused value throws)
    void setField(int32_t pcr_params::*field, int value) {
        pcr_params p;
        if (pcr_get_params(h_, &p)) throw std::runtime_error(pcr_last_error(h_));
        p.*field = value;
        if (pcr_set_params(h_, &p)) throw std::runtime_error(pcr_last_error(h_));
    }
public:
    HipRegister(const HipRegister&) = delete;
    HipRegister& operator=(const HipRegister&) = delete;
    ~HipRegister() override { pcr_destroy(h_); }

    // Error behaviour of the reference: scan2Map never throws -- it logs and returns false (LoamRegister.cpp:173-176,222; `res` keeps
    // what the iterations had reached, here the caller's guess).  lastError() holds the library's message.
    bool scan2Map(const PC_cPtr& src, const PC_cPtr& dst, pose_t& res) override {
        int conv = 0;
        if (pcr_scan2map(h_, src->points.data(), src->size(), dst->points.data(), dst->size(), sizeof(PointXYZI), res.data(), &conv)) {
            logError(pcr_last_error(h_));
            return isConverge = false;
        }
        lastError_.clear();
        isConverge = conv != 0;
        return isConverge;
    }
    // static-map localisation (test/loc.cpp): index the map once.  (No counterpart in the reference's interface: failures throw.)
    void setTarget(const PC_cPtr& dst) {
        if (pcr_set_target(h_, dst->points.data(), dst->size(), sizeof(PointXYZI), 0)) throw std::runtime_error(pcr_last_error(h_));
    }
    bool align(const PC_cPtr& src, pose_t& res) {
        int conv = 0;
        if (pcr_align(h_, src->points.data(), src->size(), sizeof(PointXYZI), 0, res.data(), &conv)) {
            logError(pcr_last_error(h_));
            return isConverge = false;
        }
        lastError_.clear();
        isConverge = conv != 0;
        return isConverge;
    }
    // Relocalisation from a coarse pose (pcr_relocalize) against the target set by setTarget: the reloc branch of
    // LidarOdometry::generateOdom (frontend/src/LidarOdometry.cpp:121-126), where the operator's click (RelocDataProxy.cpp:34-48) is `res`.
    // `res` becomes the chosen candidate's refined pose; p = nullptr: pcr_reloc_default_params.  Fails like align: logs, returns false and
    // leaves `res` alone.  cands / chosen (optional): every refined candidate and the index of the one taken.
    bool relocalize(const PC_cPtr& src, pose_t& res, const pcr_reloc_params* p = nullptr, std::vector<pcr_reloc_candidate>* cands = nullptr,
                    size_t* chosen = nullptr) {
        pcr_reloc_params dp;
        pcr_reloc_default_params(&dp);
        if (!p) p = &dp;
        std::vector<pcr_reloc_candidate> c((size_t)(p->refine_top > 0 ? p->refine_top : 0) + 1);
        size_t nc = 0, ch = 0;
        int conv = 0;
        pose_t out = res;
        if (pcr_relocalize(h_, src->points.data(), src->size(), sizeof(PointXYZI), 0, p, out.data(), &conv, c.data(), c.size(), &nc, &ch)) {
            logError(pcr_last_error(h_));
            return isConverge = false;
        }
        lastError_.clear();
        res = out;
        c.resize(nc);
        if (cands) *cands = c;
        if (chosen) *chosen = ch;
        isConverge = conv != 0;
        return isConverge;
    }
    // Global relocalisation (pcr_relocalize_global) against the target set by setTarget -- the whole map: no pose at all, at start-up or
    // when tracking is lost.  sc holds one ScanContext per key frame, kf_poses their poses.  `res` becomes the chosen candidate's refined
    // pose; p = nullptr: pcr_global_reloc_default_params.  Fails like align: logs, returns false and leaves `res` alone.
    inline bool relocalizeGlobal(const PC_cPtr& src, const context::ScanContext& sc, const std::vector<pose_t>& kf_poses, pose_t& res,
                                 const pcr_global_reloc_params* p = nullptr, std::vector<pcr_global_reloc_candidate>* cands = nullptr,
                                 size_t* chosen = nullptr);
    pcr_handle* handle() { return h_; }
    // getFitnessScore of the reference's test/align.cpp:29-61: mean squared 1-NN distance (<= max_sq) of the source under `pose`
    // against the target of the last registration; -1 when no point is that close
    scalar_t gatedFitness(const PC_cPtr& src, const pose_t& pose, double max_sq = 1.0, int64_t* n_in = nullptr) {
        double score = -1.0;
        if (pcr_fitness_gated(h_, src->points.data(), src->size(), sizeof(PointXYZI), 0, pose.data(), max_sq, &score, n_in))
            throw std::runtime_error(pcr_last_error(h_));
        return score;
    }

    // scan2Map with `dst` = the sub-map a SubMap keeps in HBM (the scan is uploaded, the map never leaves the device)
    bool scan2Map(const PC_cPtr& src, const class SubMap& dst, pose_t& res);
    // ... with a source that is in HBM already, in the map's point layout: a stored key frame (SubMap::keyFramePointer), lcHandler's lc_scan_
    bool scan2Map(const void* d_src, size_t n_src, const class SubMap& dst, pose_t& res);
};

// MapManager's key-frame store and sub-map (frontend/src/MapManager.cpp:151-201), kept in HBM
class SubMap {
    pcr_map* m_ = nullptr;
    explicit SubMap(pcr_map* view) : m_(view) {}
public:
    SubMap() : m_(pcr_map_create(-1)) { if (!m_) throw std::runtime_error(pcr_map_last_error(nullptr)); }
    SubMap(const SubMap&) = delete;
    SubMap& operator=(const SubMap&) = delete;
    ~SubMap() { pcr_map_destroy(m_); }
    void addKeyFrame(const PC_cPtr& pc, const pose_t& pose) {                 // KeyFrame{pc, pose}, common/types/basic.hpp:33-40
        if (pcr_map_add_keyframe(m_, pc->points.data(), pc->size(), sizeof(PointXYZI), 0, pose.data())) throw std::runtime_error(pcr_map_last_error(m_));
    }
    // ... from a cloud that is in HBM already (PointXYZI layout): a scan filtered with out_on_device = 1, another map's sub-map
    void addKeyFrame(const void* d_pts, size_t n, const pose_t& pose) {
        if (pcr_map_add_keyframe(m_, d_pts, n, sizeof(PointXYZI), 1, pose.data())) throw std::runtime_error(pcr_map_last_error(m_));
    }
    // MapManager::updateMap around `position`; returns the number of sub-map points
    size_t updateMap(const double position[3], double radius = 8.0 /* mSurroundingKeyframeSearchRadius */, double grid_size = 0.4) {
        size_t n = 0;
        if (pcr_map_update(m_, position, radius, grid_size, &n)) throw std::runtime_error(pcr_map_last_error(m_));
        return n;
    }
    // ... in two halves (MapManager's own thread as a stream, MapManager.cpp:109-119): queue the assembly; wait() -- or the next registration against this map -- collects it
    void updateMapBegin(const double position[3], double radius = 8.0, double grid_size = 0.4) {
        if (pcr_map_update_begin(m_, position, radius, grid_size)) throw std::runtime_error(pcr_map_last_error(m_));
    }
    size_t wait() {
        size_t n = 0;
        if (pcr_map_wait(m_, &n)) throw std::runtime_error(pcr_map_last_error(m_));
        return n;
    }
    std::vector<int64_t> submapIdx() const {                                    // mSubmapIdx
        size_t n = 0;
        pcr_map_submap_indices(m_, nullptr, 0, &n);
        std::vector<int64_t> idx(n);
        if (n) pcr_map_submap_indices(m_, idx.data(), n, &n);
        return idx;
    }
    const void* devicePointer(size_t* n, size_t* stride_bytes) const { return pcr_map_submap(m_, n, stride_bytes); }
    // pcr_map_rank_near: for every query key frame of [first, first + count) the k nearest of [0, q - num_exclude_recent) within `radius`, on the
    // device; idx and d2 get count * k entries, row q - first, tails -1 / DBL_MAX
    void rankNear(size_t first, size_t count, double radius, int k, int num_exclude_recent, std::vector<int64_t>& idx, std::vector<double>& d2) const {
        std::vector<int64_t> i(count * (size_t)(k > 0 ? k : 0));
        std::vector<double> d(i.size());
        if (pcr_map_rank_near(m_, first, count, num_exclude_recent, radius, k, i.data(), d.data())) throw std::runtime_error(pcr_map_last_error(m_));
        idx.swap(i); d2.swap(d);
    }
    size_t keyframes() const {
        size_t n = 0;
        if (pcr_map_keyframes(m_, &n)) throw std::runtime_error(pcr_map_last_error(m_));
        return n;
    }
    // LoopClosureManager::loopFindNearKeyframes (LoopClosureManager.cpp:40-60): key frames key +- search_num as this object's sub-map.  On a
    // view() it is lc_map_: the odometry sub-map of the parent stays what it is.
    size_t loopFindNearKeyframes(long long key, int search_num, double grid_size = 0.4) {
        size_t n = 0;
        if (pcr_map_update_window(m_, key, search_num, grid_size, &n)) throw std::runtime_error(pcr_map_last_error(m_));
        return n;
    }
    // the whole map (test/vis_globalmap.cpp:33-66): every key frame under its pose, concatenated, voxel-filtered
    size_t updateAll(double grid_size = 0.4) {
        size_t n = 0;
        if (pcr_map_update_all(m_, grid_size, &n)) throw std::runtime_error(pcr_map_last_error(m_));
        return n;
    }
    // ... with pcp::VoxelDownSampleV3 in place of pcl::VoxelGrid (pcr_map_update_all_sparse): filtered whatever the map's extent
    size_t updateAllSparse(double grid_size = 0.4) {
        size_t n = 0;
        if (pcr_map_update_all_sparse(m_, grid_size, &n)) throw std::runtime_error(pcr_map_last_error(m_));
        return n;
    }
    // Backend::optimHandler (Backend.cpp:315-318): the optimised poses of key frames first .. first + poses.size() - 1
    void setPoses(size_t first, const std::vector<pose_t>& poses) {
        static_assert(sizeof(pose_t) == 16 * sizeof(double), "poses are handed over as one array");
        if (pcr_map_set_poses(m_, first, poses.size(), poses.empty() ? nullptr : poses[0].data())) throw std::runtime_error(pcr_map_last_error(m_));
    }
    // key frame i as stored, in HBM: valid until the store next changes
    const void* keyFramePointer(size_t i, size_t* n, size_t* stride_bytes = nullptr, pose_t* pose = nullptr) const {
        if (i >= keyframes()) throw std::runtime_error("key-frame index out of range");
        return pcr_map_keyframe(m_, i, n, stride_bytes, pose ? pose->data() : nullptr);
    }
    // ... and on the host: KeyFrame{pc, pose}
    PC_Ptr keyFrame(size_t i, pose_t* pose = nullptr) const {
        size_t n = 0;
        keyFramePointer(i, &n);
        auto pc = std::make_shared<PointCloud>();
        pc->points.resize(n);
        if (pcr_map_read_keyframe(m_, i, pc->points.data(), n, &n, pose ? pose->data() : nullptr)) throw std::runtime_error(pcr_map_last_error(m_));
        return pc;
    }
    // MapManager::saveKfs (MapManager.cpp:211) / MapManager() (:46): key frames first .. end voxel-filtered in place; returns the points in the store
    size_t downSampleKeyFrames(size_t first, double grid_size) {
        size_t n = 0;
        if (pcr_map_downsample_keyframes(m_, first, grid_size, &n)) throw std::runtime_error(pcr_map_last_error(m_));
        return n;
    }
    // A session on disk (pcr_map_save / pcr_map_load; the reference's saveMapDir).  save: {dir}/{i}.pcd for key frames first .. end as the
    // store holds them now and tum.txt for all of them (stamps: one per key frame, empty: the index); the default tum.txt rounds to the
    // millimetre and to 1e-6, precise writes 17 digits.  load (MapManager::MapManager(), MapManager.cpp:33-49) into a store without key frames:
    // tum.txt's poses -- quaternions as read, NOT normalised -- and {i}.pcd, then with grid_size > 0 the in-place filter; returns the stamps
    // (none when there is no tum.txt).  The loaded key frames are PointXYZI records, like every cloud of this class.
    void save(const std::string& dir, size_t first = 0, const std::vector<double>& stamps = {}, bool precise = false) const {
        if (!stamps.empty() && stamps.size() != keyframes()) throw std::runtime_error("SubMap::save: one stamp per key frame");
        if (pcr_map_save(m_, dir.c_str(), first, stamps.empty() ? nullptr : stamps.data(), precise ? 1 : 0)) throw std::runtime_error(pcr_map_last_error(m_));
    }
    std::vector<double> load(const std::string& dir, double grid_size = 0.0) {
        usePointXYZI();
        size_t n = 0;
        if (pcr_map_load(m_, dir.c_str(), grid_size, nullptr, 0, &n)) throw std::runtime_error(pcr_map_last_error(m_));
        return stampsOf(dir, n);
    }
    // a store that never held a key frame takes its point layout from the first one: an empty PointXYZI key frame, added and cleared
    // again, fixes it (pcr_map_clear keeps the layout) so that a load fills the store with the records addKeyFrame appends later
    void usePointXYZI() {
        size_t stride = 0;
        (void)pcr_map_keyframe(m_, 0, nullptr, &stride, nullptr);
        if (stride != 0 || m_ == nullptr || keyframes() != 0) return;
        const pose_t eye;
        if (pcr_map_add_keyframe(m_, nullptr, 0, sizeof(PointXYZI), 0, eye.data()) || pcr_map_clear(m_)) throw std::runtime_error(pcr_map_last_error(m_));
    }
    // the stamps of the first n non-blank lines of {dir}/tum.txt (pcr_tum_parse)
    static std::vector<double> stampsOf(const std::string& dir, size_t n) {
        std::vector<double> stamps;
        FILE* f = n ? std::fopen((dir + "/tum.txt").c_str(), "r") : nullptr;
        if (!f) return stamps;
        std::string line;
        for (int c = 0; stamps.size() < n && c != EOF;) {
            line.clear();
            while ((c = std::fgetc(f)) != EOF && c != '\n') line.push_back((char)c);
            double stamp = 0, pose[16];
            if (pcr_tum_parse(line.c_str(), &stamp, pose) == PCR_TUM_OK) stamps.push_back(stamp);
        }
        std::fclose(f);
        return stamps;
    }
    // another sub-map over the same key frames (pcr_map_view); this object must outlive it, or the view fails every call from then on
    std::unique_ptr<SubMap> view() {
        pcr_map* v = pcr_map_view(m_);
        if (!v) throw std::runtime_error(pcr_map_last_error(m_));
        return std::unique_ptr<SubMap>(new SubMap(v));
    }
    const pcr_map* handle() const { return m_; }
    pcr_map* handle() { return m_; }
    uint64_t generation() const { uint64_t id = 0, g = 0; pcr_map_generation(m_, &id, &g); return g; }
};

inline bool HipRegister::scan2Map(const PC_cPtr& src, const SubMap& dst, pose_t& res) {
    // The handle keeps the target structures it builds from the sub-map for as long as the map stays at the same generation
    // (pcr_scan2map_submap): LidarOdometry registers several scans between two MapManager::updateMap calls.
    int conv = 0;
    if (pcr_scan2map_submap(h_, src->points.data(), src->size(), 0, dst.handle(), res.data(), &conv)) {
        logError(pcr_last_error(h_));
        return isConverge = false;
    }
    lastError_.clear();
    isConverge = conv != 0;
    return isConverge;
}

inline bool HipRegister::scan2Map(const void* d_src, size_t n_src, const SubMap& dst, pose_t& res) {
    int conv = 0;
    if (pcr_scan2map_submap(h_, d_src, n_src, 1, dst.handle(), res.data(), &conv)) {
        logError(pcr_last_error(h_));
        return isConverge = false;
    }
    lastError_.clear();
    isConverge = conv != 0;
    return isConverge;
}

// trans::SixDof2Mobile (common/geometry/trans.hpp:68-86; applied to every refined pose at LidarOdometry.cpp:211): x, y and the rotation about Z
// when the pose's rotation axis is within ~18 degrees of it; otherwise the heading is dropped, as in the reference (pcr_pose_to_mobile)
inline pose_t SixDof2Mobile(const pose_t& p) {
    pose_t res;
    if (pcr_pose_to_mobile(p.data(), res.data())) throw std::runtime_error("pcr_pose_to_mobile failed");
    return res;
}

// The per-scan loop of LidarOdometry::handler around scan2Map (LidarOdometry.cpp:160-214, MapManager.cpp:109-201) over a registrar and a SubMap,
// both borrowed: pcr_frontend_*.  step(): voxel filter -> scan2Map against the sub-map -> SixDof2Mobile (params.mobile) -> setCurPose -> putKeyFrame
// -> updateMap (queued; the next step, or finish(), collects it).  Failures throw with the library's message.
class Frontend {
    pcr_frontend* fe_ = nullptr;
    static pcr_frontend_params params_or_default(const pcr_frontend_params* p) {
        pcr_frontend_params d;
        pcr_frontend_default_params(&d);
        return p ? *p : d;
    }
public:
    Frontend(HipRegister& reg, SubMap& map, const pcr_frontend_params* p = nullptr) {
        const pcr_frontend_params prm = params_or_default(p);
        fe_ = pcr_frontend_create(reg.handle(), map.handle(), &prm);
        if (!fe_) throw std::runtime_error(pcr_frontend_last_error(nullptr));
    }
    Frontend(const Frontend&) = delete;
    Frontend& operator=(const Frontend&) = delete;
    ~Frontend() { pcr_frontend_destroy(fe_); }
    // one scan from `init` (generateOdom's guess: previous pose o odometry) -> the pose; info: what the step did and how long its parts took
    pose_t step(const PC_cPtr& scan, const pose_t& init, pcr_frontend_info* info = nullptr) {
        return step(scan->points.data(), scan->size(), false, init, info);
    }
    // ... a scan that is in HBM already (PointXYZI layout)
    pose_t step(const void* pts, size_t n, bool on_device, const pose_t& init, pcr_frontend_info* info = nullptr) {
        pose_t res;
        if (pcr_frontend_step(fe_, pts, n, sizeof(PointXYZI), on_device ? 1 : 0, init.data(), res.data(), info)) throw std::runtime_error(pcr_frontend_last_error(fe_));
        return res;
    }
    // one scan of a moving sensor: pcr_deskew into a device buffer of the front end's, then step() on that buffer (the key frame is the deskewed
    // scan).  times: one float per point, seconds after m.t0, living where the scan lives; nullptr: the float at byte `time_offset` of every record
    pose_t stepTimed(const void* pts, size_t n, bool on_device, const float* times, const pcr_deskew_motion& m, const pose_t& init,
                     pcr_frontend_info* info = nullptr, pcr_deskew_info* dinfo = nullptr, long long time_offset = 0) {
        pose_t res;
        if (pcr_frontend_step_timed(fe_, pts, n, sizeof(PointXYZI), on_device ? 1 : 0, times, PCR_TIME_F32_SECONDS, time_offset, &m, init.data(), res.data(), info, dinfo))
            throw std::runtime_error(pcr_frontend_last_error(fe_));
        return res;
    }
    pose_t stepTimed(const PC_cPtr& scan, const std::vector<float>& times, const pcr_deskew_motion& m, const pose_t& init, pcr_frontend_info* info = nullptr,
                     pcr_deskew_info* dinfo = nullptr) {
        if (times.size() != scan->size()) throw std::runtime_error("stepTimed: one time per point");
        return stepTimed(scan->points.data(), scan->size(), false, times.data(), m, init, info, dinfo);
    }
    // the NEXT scan's voxel filter, queued beside this scan's registration
    void prefetch(const PC_cPtr& next) { prefetch(next->points.data(), next->size(), false); }
    void prefetch(const void* pts, size_t n, bool on_device) {
        if (pcr_frontend_prefetch(fe_, pts, n, sizeof(PointXYZI), on_device ? 1 : 0)) throw std::runtime_error(pcr_frontend_last_error(fe_));
    }
    size_t finish() {
        size_t n = 0;
        if (pcr_frontend_finish(fe_, &n)) throw std::runtime_error(pcr_frontend_last_error(fe_));
        return n;
    }
    void reset() { if (pcr_frontend_reset(fe_)) throw std::runtime_error(pcr_frontend_last_error(fe_)); }
    // mClosestKfIdx (MapManager.cpp:146): per key frame this front end added, the key frame nearest to it then; -1 for the first
    std::vector<int64_t> closest() const {
        size_t n = 0;
        if (pcr_frontend_closest(fe_, nullptr, 0, &n)) throw std::runtime_error(pcr_frontend_last_error(fe_));
        std::vector<int64_t> idx(n);
        if (n && pcr_frontend_closest(fe_, idx.data(), n, &n)) throw std::runtime_error(pcr_frontend_last_error(fe_));
        return idx;
    }
    pcr_frontend* handle() { return fe_; }
};

class LoamRegister : public HipRegister {
public:
    LoamRegister() : HipRegister("loam") {}
    explicit LoamRegister(const pcr_params& p) : HipRegister("loam", &p) {}
};

class NdtRegister : public HipRegister {
public:
    NdtRegister() : HipRegister("ndt") {}
    explicit NdtRegister(const pcr_params& p) : HipRegister("ndt", &p) {}
    // pclomp::NormalDistributionsTransform::setNeighborhoodSearchMethod (ndt_omp.h:189-191): PCR_NDT_DIRECT26 / _DIRECT7 / _DIRECT1, in pclomp's
    // enum order.  The prepared target is kept (the voxel Gaussians do not depend on it); PCR_NDT_KDTREE or a value out of range throws.
    void setNeighborhoodSearchMethod(int method) { setField(&pcr_params::ndt_search, method); }
};

class VgicpRegister : public HipRegister {
    static pcr_params lc_params() {            // VgicpRegister::initForLC (VgicpRegister.cpp:21-28)
        pcr_params p;
        pcr_default_params(&p);
        p.vgicp_max_iters = 100;
        p.vgicp_trans_eps = 1e-6;
        return p;
    }
public:
    VgicpRegister() : HipRegister("vgicp") {}
    explicit VgicpRegister(const pcr_params& p) : HipRegister("vgicp", &p) {}
    static std::shared_ptr<VgicpRegister> makeForLC() { return std::make_shared<VgicpRegister>(lc_params()); }
    // VgicpRegister::initForLC (VgicpRegister.cpp:21-28) on the live object, as LoopClosureManager's constructor calls it
    // (backend/src/LoopClosureManager.cpp:21-22): 100 iterations, transformation epsilon 1e-6
    void initForLC() {
        pcr_params p;
        if (pcr_get_params(h_, &p)) throw std::runtime_error(pcr_last_error(h_));
        p.vgicp_max_iters = 100;
        p.vgicp_trans_eps = 1e-6;
        if (pcr_set_params(h_, &p)) throw std::runtime_error(pcr_last_error(h_));
    }
    // fast_gicp::FastGICP::setRegularizationMethod / FastVGICP::setVoxelAccumulationMode (gicp_settings.hpp:6,10): PCR_REG_* / PCR_VOXEL_*.
    // The prepared target is dropped when the value changes; a value out of range throws.
    void setRegularizationMethod(int method) { setField(&pcr_params::vgicp_regularization, method); }
    void setVoxelAccumulationMode(int mode) { setField(&pcr_params::vgicp_voxel_mode, mode); }
    // fast_gicp::FastVGICP::setNeighborSearchMethod (gicp_settings.hpp:8): PCR_VGICP_DIRECT27 / _DIRECT7 / _DIRECT1, in fast_gicp's enum order.  The
    // prepared target is kept (the voxels do not depend on it); PCR_VGICP_DIRECT_RADIUS or a value out of range throws.
    void setNeighborSearchMethod(int method) { setField(&pcr_params::vgicp_search, method); }
    scalar_t getFitnessScore() override { return pcr_fitness(h_); }
};

// VgicpRegister with fast_gicp::FastGICP as its registrar (fast_gicp_impl.hpp:103-237): correspondences by exact nearest neighbour
class GicpRegister : public HipRegister {
public:
    GicpRegister() : HipRegister("gicp") {}
    explicit GicpRegister(const pcr_params& p) : HipRegister("gicp", &p) {}
    // VgicpRegister::initForLC (VgicpRegister.cpp:21-28): here its setMaxCorrespondenceDistance(150) acts too (fast_gicp_impl.hpp:136)
    void initForLC() {
        pcr_params p;
        if (pcr_get_params(h_, &p)) throw std::runtime_error(pcr_last_error(h_));
        p.vgicp_max_iters = 100;
        p.vgicp_trans_eps = 1e-6;
        p.gicp_max_corr_dist = 150.0;
        if (pcr_set_params(h_, &p)) throw std::runtime_error(pcr_last_error(h_));
    }
    // fast_gicp::FastGICP::setRegularizationMethod (PCR_REG_*); the prepared target is dropped when the value changes
    void setRegularizationMethod(int method) { setField(&pcr_params::vgicp_regularization, method); }
    scalar_t getFitnessScore() override { return pcr_fitness(h_); }
};

// LioScan2map of the reference's test/comp/liorf_scan2map.cpp (LIO-SAM's surface scan-to-map) under the plugin interface: scan2Map takes the
// six numbers out of `res`, iterates on the device and returns pcl::getTransformation of the final six
class LiorfRegister : public HipRegister {
public:
    LiorfRegister() : HipRegister("liorf") {}
    explicit LiorfRegister(const pcr_params& p) : HipRegister("liorf", &p) {}
    // isDegenerate of the last scan2Map (iteration 0: the smallest eigenvalue of AtA below liorf_degenerate_eig)
    bool isDegenerate() {
        int deg = 0;
        if (pcr_liorf_result(h_, nullptr, &deg, nullptr)) throw std::runtime_error(pcr_last_error(h_));
        return deg != 0;
    }
    // the file's own getFitnessScore (:22-54): mean squared 1-NN distance over d2 <= 1, -1 when there is none
    scalar_t getFitnessScore() override { return pcr_fitness(h_); }
};

// The static-map adapter: test/loc.cpp loads the global map ONCE (MapManager::MapManager(pcd_file), frontend/src/MapManager.cpp:52-78) and
// registers every scan against it -- through the unchanged scan2Map(src, dst, res) interface.  Wrapped around any registrar above it
// indexes `dst` at its first call (pcr_set_target: the map crosses PCIe once) and aligns every later scan against what the device holds
// (pcr_align: only the scan is uploaded).  The CALLER says when the map's content has changed -- invalidate() -- the adapter never keys
// anything on the pointer it was handed (a cloud edited in place keeps its address).  Same poses as scan2Map, bit for bit.
class StaticMapRegister : public PointCloudRegister {
    std::shared_ptr<HipRegister> reg_;
    bool have_target_ = false;
public:
    explicit StaticMapRegister(std::shared_ptr<HipRegister> reg) : reg_(std::move(reg)) {}
    void invalidate() { have_target_ = false; }
    bool scan2Map(const PC_cPtr& src, const PC_cPtr& dst, pose_t& res) override {
        if (!have_target_) {
            try { reg_->setTarget(dst); } catch (const std::exception& e) { logError(e.what()); return isConverge = false; }
            have_target_ = true;
        }
        isConverge = reg_->align(src, res);
        lastError_ = reg_->lastError();
        return isConverge;
    }
    // the reloc branch of generateOdom against the static map: `dst` indexed at the first call, as scan2Map does
    bool relocalize(const PC_cPtr& src, const PC_cPtr& dst, pose_t& res, const pcr_reloc_params* p = nullptr,
                    std::vector<pcr_reloc_candidate>* cands = nullptr, size_t* chosen = nullptr) {
        if (!have_target_) {
            try { reg_->setTarget(dst); } catch (const std::exception& e) { logError(e.what()); return isConverge = false; }
            have_target_ = true;
        }
        isConverge = reg_->relocalize(src, res, p, cands, chosen);
        lastError_ = reg_->lastError();
        return isConverge;
    }
    // global relocalisation against the static map: `dst` indexed at the first call, as scan2Map does
    bool relocalizeGlobal(const PC_cPtr& src, const PC_cPtr& dst, const context::ScanContext& sc, const std::vector<pose_t>& kf_poses, pose_t& res,
                          const pcr_global_reloc_params* p = nullptr, std::vector<pcr_global_reloc_candidate>* cands = nullptr,
                          size_t* chosen = nullptr) {
        if (!have_target_) {
            try { reg_->setTarget(dst); } catch (const std::exception& e) { logError(e.what()); return isConverge = false; }
            have_target_ = true;
        }
        isConverge = reg_->relocalizeGlobal(src, sc, kf_poses, res, p, cands, chosen);
        lastError_ = reg_->lastError();
        return isConverge;
    }
    scalar_t getFitnessScore() override { return reg_->getFitnessScore(); }
    HipRegister& inner() { return *reg_; }
};

// The reference's spatial index, nanoflann::PointCloudKdtree<PointType, double> (third_parties/nanoflann/include/nanoflann/pcl_adaptor.hpp:11-78),
// over the index a registrar keeps in HBM: the same two member names and argument orders -- one query of three doubles, std::vector outputs --
// so that a call site such as test/align.cpp:47 changes its type and nothing else.  The cloud is the registrar's kept target: setInputCloud
// hands it to the adapter's own handle (pcr_set_target); an adapter made over a registrar's handle queries the target that registrar holds.
// Answers: pcr_knn / pcr_radius_search -- nanoflann's squared distances in double, ascending by (distance, index).  Failures throw.
// Batched overloads take n records of stride_bytes (x, y, z floats first) and answer every query in one call.
class PointCloudKdtree {
    pcr_handle* h_ = nullptr;
    bool own_ = false;
public:
    PointCloudKdtree() : h_(pcr_create("loam", nullptr)), own_(true) { if (!h_) throw std::runtime_error(pcr_last_error(nullptr)); }
    explicit PointCloudKdtree(pcr_handle* h) : h_(h) {}
    explicit PointCloudKdtree(HipRegister& reg) : h_(reg.handle()) {}
    PointCloudKdtree(const PointCloudKdtree&) = delete;
    PointCloudKdtree& operator=(const PointCloudKdtree&) = delete;
    ~PointCloudKdtree() { if (own_) pcr_destroy(h_); }

    void setInputCloud(const PC_cPtr& cloud) {
        if (pcr_set_target(h_, cloud->points.data(), cloud->size(), sizeof(PointXYZI), 0)) throw std::runtime_error(pcr_last_error(h_));
    }
    // pcr_params.query_index: PCR_QUERY_INDEX_AUTO (the dense cell table wherever it holds every point, the sparse index for a target whose box
    // cannot be tabulated) or PCR_QUERY_INDEX_SPARSE (always the sparse index); the same answers.  A value out of range throws.
    void setQueryIndex(int query_index) {
        pcr_params p;
        if (pcr_get_params(h_, &p)) throw std::runtime_error(pcr_last_error(h_));
        p.query_index = query_index;
        if (pcr_set_params(h_, &p)) throw std::runtime_error(pcr_last_error(h_));
    }
    // the index that answered the last search or fitness score (a score a cut dense index cannot give is taken on the sparse one): its kind (PCR_QUERY_INDEX_DENSE / _SPARSE; -1: none yet), its points, its bytes of device memory
    struct QueryIndexInfo { int kind; size_t n_points, bytes; };
    QueryIndexInfo queryIndexInfo() const {
        QueryIndexInfo i{-1, 0, 0};
        if (pcr_query_index_info(h_, &i.kind, &i.n_points, &i.bytes)) throw std::runtime_error(pcr_last_error(h_));
        return i;
    }
    size_t nearestKSearch(double* point, int k, std::vector<size_t>& k_indices, std::vector<double>& k_sqr_distances) const {
        const float q[4] = {(float)point[0], (float)point[1], (float)point[2], 0.f};
        std::vector<int64_t> idx((size_t)(k > 0 ? k : 0));
        k_sqr_distances.assign(idx.size(), 0.0);
        if (pcr_knn(h_, q, 1, sizeof q, 0, k, idx.data(), k_sqr_distances.data())) throw std::runtime_error(pcr_last_error(h_));
        size_t n = 0;
        while (n < idx.size() && idx[n] >= 0) ++n;
        k_indices.assign(idx.size(), 0);
        for (size_t i = 0; i < n; ++i) k_indices[i] = (size_t)idx[i];
        return n;      // KNNResultSet::size(): the entries found
    }
    size_t radiusSearch(double* point, double radius, std::vector<size_t>& k_indices, std::vector<double>& k_sqr_distances, bool sorted = false) const {
        const float q[4] = {(float)point[0], (float)point[1], (float)point[2], 0.f};
        std::vector<uint64_t> offsets;
        std::vector<int64_t> idx;
        radiusSearch(q, 1, sizeof q, radius, offsets, idx, k_sqr_distances, sorted);
        k_indices.assign(idx.begin(), idx.end());
        return idx.size();
    }
    // n queries at once: idx / d2 hold n x k entries, row by row (idx -1, d2 +inf where the target has fewer than k points)
    void nearestKSearch(const void* queries, size_t n, size_t stride_bytes, int k, std::vector<int64_t>& idx, std::vector<double>& d2,
                        bool on_device = false) const {
        idx.assign(n * (size_t)(k > 0 ? k : 0), -1);
        d2.assign(idx.size(), 0.0);
        if (pcr_knn(h_, queries, n, stride_bytes, on_device ? 1 : 0, k, idx.data(), d2.data())) throw std::runtime_error(pcr_last_error(h_));
    }
    // ... query q's neighbours are idx / d2 [offsets[q], offsets[q + 1]): counted first, then fetched into arrays of that size
    void radiusSearch(const void* queries, size_t n, size_t stride_bytes, double radius, std::vector<uint64_t>& offsets, std::vector<int64_t>& idx,
                      std::vector<double>& d2, bool sorted = false, bool on_device = false) const {
        offsets.assign(n + 1, 0);
        size_t total = 0;
        // (sized for what the vectors already hold: a repeated search is answered by one call)
        idx.resize(std::min(idx.size(), d2.size())); d2.resize(idx.size());
        int rc = pcr_radius_search(h_, queries, n, stride_bytes, on_device ? 1 : 0, radius, sorted ? 1 : 0, idx.size(), offsets.data(), idx.data(), d2.data(), &total);
        if (rc && total > idx.size()) {
            idx.resize(total); d2.resize(total);
            rc = pcr_radius_search(h_, queries, n, stride_bytes, on_device ? 1 : 0, radius, sorted ? 1 : 0, total, offsets.data(), idx.data(), d2.data(), &total);
        }
        if (rc) throw std::runtime_error(pcr_last_error(h_));
        idx.resize(total); d2.resize(total);
    }
};

// frontend/src/LidarOdometry.cpp:44-54
inline PointCloudRegister::Ptr makeRegister(const std::string& pcr_type) {
    if (pcr_type == "loam") return std::make_shared<LoamRegister>();
    if (pcr_type == "ndt") return std::make_shared<NdtRegister>();
    if (pcr_type == "vgicp") return std::make_shared<VgicpRegister>();
    if (pcr_type == "gicp") return std::make_shared<GicpRegister>();
    if (pcr_type == "liorf") return std::make_shared<LiorfRegister>();
    throw std::runtime_error("such pcr type(" + pcr_type + ") is not exist, please implemented your self!");
}
// ... the same registrar behind the static-map adapter (localisation against a map that is loaded once)
inline std::shared_ptr<StaticMapRegister> makeStaticMapRegister(const std::string& pcr_type) {
    return std::make_shared<StaticMapRegister>(std::dynamic_pointer_cast<HipRegister>(makeRegister(pcr_type)));
}

}  // namespace PCR

// backend/include/backend/ScanContext.hpp: the loop-closure descriptor database (addContext, query)
namespace context {
class ScanContext {
    pcr_sc* s_ = nullptr;
    pcr_sc_params prm_;
public:
    using QueryResult = std::pair<int, float>;                                  // {matched key frame or -1, yaw in rad}
    explicit ScanContext(const pcr_sc_params* p = nullptr) : s_(pcr_sc_create(-1, p)) {
        if (!s_) throw std::runtime_error(pcr_sc_last_error(nullptr));
        if (p) prm_ = *p; else pcr_sc_default_params(&prm_);
    }
    ScanContext(const ScanContext&) = delete;
    ScanContext& operator=(const ScanContext&) = delete;
    ~ScanContext() { pcr_sc_destroy(s_); }
    void addContext(const PCR::PointCloud& scan_down) {
        if (pcr_sc_add(s_, scan_down.points.data(), scan_down.size(), sizeof(PCR::PointXYZI), 0)) throw std::runtime_error(pcr_sc_last_error(s_));
    }
    // LoopClosureManager::addContext (LoopClosureManager.cpp:28-37) over stored key frames [first, first + count) of a SubMap (or a view of one) in
    // one batched pass (pcr_sc_add_keyframes): each key frame's own cloud, voxel-filtered at grid_size when that is positive -> contexts added
    size_t addKeyFrames(const PCR::SubMap& map, size_t first, size_t count, double grid_size = 0) {
        size_t n = 0;
        if (pcr_sc_add_keyframes(s_, map.handle(), first, count, grid_size, &n)) throw std::runtime_error(pcr_sc_last_error(s_));
        return n;
    }
    QueryResult query(int id) {
        long long match = -1;
        float yaw = 0;
        if (pcr_sc_query(s_, id, &match, &yaw, nullptr)) throw std::out_of_range(pcr_sc_last_error(s_));     // ringcontexts_.at(id)
        return {(int)match, yaw};
    }
    size_t size() const { size_t n = 0; pcr_sc_size(s_, &n); return n; }
    // distanceBtnScanContext of an outside scan (not added) against every stored context, on the device: what distance(q, i) would be
    // had the scan been added as context q
    void distances(const PCR::PointCloud& scan_down, std::vector<double>& dist, std::vector<int32_t>& shift) const {
        dist.assign(size(), 0.0);
        shift.assign(dist.size(), 0);
        if (pcr_sc_distances(s_, scan_down.points.data(), scan_down.size(), sizeof(PCR::PointXYZI), 0, dist.data(), shift.data()))
            throw std::runtime_error(pcr_sc_last_error(s_));
    }
    // Stored against stored, on the device (pcr_sc_rank_stored): for every query q of [first, first + count) the k best candidates i of
    // [0, q - num_exclude_recent) by (distance(q, i), i); row q - first of each array, tail idx -1 / DBL_MAX / 0
    struct Ranking { size_t first = 0, count = 0; int k = 0; std::vector<int64_t> idx; std::vector<double> dist; std::vector<int32_t> shift; };
    Ranking rankStored(size_t first, size_t count, int k = 1) const {
        Ranking r;
        r.first = first; r.count = count; r.k = k;
        const size_t n = count * (size_t)(k > 0 ? k : 0);
        r.idx.assign(n, -1); r.dist.assign(n, std::numeric_limits<double>::max()); r.shift.assign(n, 0);
        // (a vector of no elements may hand out a null pointer, which the call refuses when count > 0: k out of range is reported first)
        if (pcr_sc_rank_stored(s_, first, count, k, r.idx.data(), r.dist.data(), r.shift.data())) throw std::runtime_error(pcr_sc_last_error(s_));
        return r;
    }
    // LoopClosureManager::lcHandler's walk over key frames [first, first + count) in one call: the k = 1 ranking, then query's threshold
    // (strict, ScanContext.cpp:273) and yaw.  match = -1 (yaw 0) when there is no candidate or min_dist > dist_thres.
    struct Loop { int id; int match; float yaw; double min_dist; };
    std::vector<Loop> findLoops(size_t first, size_t count) const {
        const Ranking r = rankStored(first, count, 1);
        std::vector<Loop> out(count);
        for (size_t j = 0; j < count; ++j) {
            const bool hit = r.idx[j] >= 0 && !(r.dist[j] > (double)(float)prm_.dist_thres);
            out[j] = {(int)(first + j), hit ? (int)r.idx[j] : -1, hit ? pcr_sc_shift_yaw(r.shift[j]) : 0.f, r.dist[j]};
        }
        return out;
    }
    pcr_sc* handle() const { return s_; }
};
}  // namespace context

// backend/src/Backend.cpp: Backend::Gtsam (addPrior, addEstimate, addBetween, addLC) and what Backend::optimHandler does with it, on the
// device (pcr_graph).  Ids are positions: addEstimate(id, pose) must be called with id = the number of poses so far.
namespace backend {
class PoseGraph {
    pcr_graph* g_ = nullptr;
    static const double* noise(int kind, const double* info21, double* buf) {
        if (info21) return info21;
        pcr_graph_noise(kind, buf);
        return buf;
    }
    void check(int rc) const { if (rc) throw std::runtime_error(pcr_graph_last_error(g_)); }
public:
    using Result = pcr_graph_result;
    explicit PoseGraph(int device = -1) : g_(pcr_graph_create(device)) { if (!g_) throw std::runtime_error(pcr_graph_last_error(nullptr)); }
    PoseGraph(const PoseGraph&) = delete;
    PoseGraph& operator=(const PoseGraph&) = delete;
    ~PoseGraph() { pcr_graph_destroy(g_); }
    // info21 = the 21 upper-triangular entries of the information matrix in [omega; v] order; nullptr = the reference's preset (Backend.cpp:90-97)
    void addPrior(const PCR::pose_t& pose, size_t id = 0, const double* info21 = nullptr) {
        double buf[21];
        check(pcr_graph_add_prior(g_, id, pose.data(), noise(PCR_GRAPH_PRIOR, info21, buf)));
    }
    void addEstimate(size_t id, const PCR::pose_t& pose) {
        if (id != poses()) throw std::invalid_argument("PoseGraph::addEstimate: ids are consecutive from 0");
        check(pcr_graph_add_poses(g_, pose.data(), 1));
    }
    void addBetween(size_t from, size_t to, const PCR::pose_t& between, const double* info21 = nullptr) {
        double buf[21];
        check(pcr_graph_add_between(g_, from, to, between.data(), noise(PCR_GRAPH_ODOM, info21, buf)));
    }
    void addLC(size_t from, size_t to, const PCR::pose_t& between, const double* info21 = nullptr) {
        double buf[21];
        check(pcr_graph_add_loop(g_, from, to, between.data(), noise(PCR_GRAPH_LOOP, info21, buf)));      // the robust mark: nothing under NONE
    }
    // The kernel of the marked between factors (PCR_GRAPH_ROBUST_*; delta in units of a residual's Mahalanobis length); marks and switches by
    // index among the between factors in the order added.  A factor that is off adds nothing and links nothing.
    void setRobustKernel(int kind, double delta = 0.0) { check(pcr_graph_set_robust_kernel(g_, kind, delta)); }
    void setBetweenRobust(size_t first, size_t count = 1, bool on = true) { check(pcr_graph_set_between_robust(g_, first, count, on ? 1 : 0)); }
    void setBetweenEnabled(size_t first, size_t count = 1, bool on = true) { check(pcr_graph_set_between_enabled(g_, first, count, on ? 1 : 0)); }
    // A fixed pose is a constant of the problem: optimize() moves the free poses only and hands the fixed ones back bit for bit (g2o's setFixed)
    void setFixed(size_t first, size_t count = 1, bool on = true) { check(pcr_graph_set_fixed(g_, first, count, on ? 1 : 0)); }
    std::vector<uint8_t> fixed() const {
        std::vector<uint8_t> out(poses());
        check(pcr_graph_fixed(g_, 0, out.size(), out.data()));
        return out;
    }
    // the verdict at the current estimates, per between factor: s = r^T Omega r, the kernel's weight at s (1 when unmarked), the mark, the switch
    struct Weights { std::vector<double> s, w; std::vector<uint8_t> robust, enabled; };
    Weights betweenWeights(size_t first = 0, size_t count = (size_t)-1) {
        size_t b = 0;
        pcr_graph_size(g_, nullptr, nullptr, &b);
        if (count == (size_t)-1) count = b - std::min(first, b);
        Weights o;
        o.s.resize(count); o.w.resize(count); o.robust.resize(count); o.enabled.resize(count);
        check(pcr_graph_between_weights(g_, first, count, o.s.data(), o.w.data(), o.robust.data(), o.enabled.data()));
        return o;
    }
    // Backend::addOdomFactor (Backend.cpp:241-247): the between factor of the two current estimates
    void addOdomFactor(size_t from, size_t to, const double* info21 = nullptr) {
        double buf[21];
        check(pcr_graph_add_between_poses(g_, from, to, noise(PCR_GRAPH_ODOM, info21, buf)));
    }
    Result optimize(const pcr_graph_params* p = nullptr) {
        Result r;
        check(pcr_graph_optimize(g_, p, &r));
        return r;
    }
    // the defaults with another preconditioner: PCR_GRAPH_PRECOND_TREE for a loaded map (an odometry tree plus few loops, thousands of poses)
    Result optimize(int pcg_preconditioner) {
        pcr_graph_params p;
        pcr_graph_default_params(&p);
        p.pcg_preconditioner = pcg_preconditioner;
        return optimize(&p);
    }
    // the spanning forest the tree preconditioner uses: parent[p], -1 at the roots; the between factors in it, the others (host code)
    std::vector<int64_t> tree(size_t* n_tree_edges = nullptr, size_t* n_other_edges = nullptr) const {
        std::vector<int64_t> parent(poses());
        check(pcr_graph_tree(g_, parent.data(), parent.size(), n_tree_edges, n_other_edges));
        return parent;
    }
    // z = M^-1 r at the current estimates, 6 doubles per pose, by the solve's own factorisation and sweeps
    std::vector<double> precondition(double lambda, const std::vector<double>& r, int kind = PCR_GRAPH_PRECOND_TREE) {
        if (r.size() != 6 * poses()) throw std::invalid_argument("PoseGraph::precondition: r holds 6 entries per pose");
        std::vector<double> z(r.size());
        check(pcr_graph_precondition(g_, lambda, kind, r.data(), z.data()));
        return z;
    }
    size_t poses() const { size_t n = 0; pcr_graph_size(g_, &n, nullptr, nullptr); return n; }
    size_t factors() const { size_t p = 0, b = 0; pcr_graph_size(g_, nullptr, &p, &b); return p + b; }
    std::vector<PCR::pose_t> poses(size_t first, size_t count) const {
        static_assert(sizeof(PCR::pose_t) == 16 * sizeof(double), "poses are handed over as 16 doubles each");
        std::vector<PCR::pose_t> out(count);
        check(pcr_graph_poses(g_, first, count, count ? out.front().data() : nullptr));
        return out;
    }
    // Backend.cpp:315-318: the optimised poses become the key frames' poses, device to store (pcr_map_set_poses_from_graph)
    void applyTo(PCR::SubMap& map, size_t first = 0, size_t count = (size_t)-1) const {
        if (count == (size_t)-1) count = poses() - std::min(first, poses());
        if (pcr_map_set_poses_from_graph(map.handle(), g_, first, count)) throw std::runtime_error(pcr_map_last_error(map.handle()));
    }
    double chi2() { double c = 0; check(pcr_graph_linearize(g_, nullptr, nullptr, nullptr, &c)); return c; }
    void loadG2o(const std::string& path) { check(pcr_graph_load_g2o(g_, path.c_str())); }
    void saveG2o(const std::string& path) const { check(pcr_graph_save_g2o(g_, path.c_str())); }
    void clear() { check(pcr_graph_clear(g_)); }
    pcr_graph* handle() const { return g_; }
};

// Backend::optimHandler's NewKFCome and LC events and LoopClosureManager::lcHandler in the library (pcr_backend) over a SubMap it
// borrows (a parent).  graph(), sc() and reg() are the owned handles, for the C interfaces that exist (pcr_graph_set_robust_kernel,
// pcr_graph_save_g2o, pcr_sc_descriptor, pcr_get_stats, ...); sc() is a new handle after reset().
class Backend {
    pcr_backend* be_ = nullptr;
    PCR::SubMap& map_;
    void check(int rc) const { if (rc) throw std::runtime_error(pcr_backend_last_error(be_)); }
public:
    using Info = pcr_backend_info;
    using Loop = pcr_backend_loop;
    static pcr_backend_params defaults() { pcr_backend_params p; pcr_backend_default_params(&p); return p; }
    explicit Backend(PCR::SubMap& map, const pcr_backend_params* p = nullptr) : be_(pcr_backend_create(map.handle(), p)), map_(map) {
        if (!be_) throw std::runtime_error(pcr_backend_last_error(nullptr));
    }
    Backend(const Backend&) = delete;
    Backend& operator=(const Backend&) = delete;
    ~Backend() { pcr_backend_destroy(be_); }
    // closest: Frontend::closest()'s entries for the key frames the store has gained since the last event (nullptr: every edge from i - 1)
    Info addKeyFrames(const int64_t* closest = nullptr, size_t n_closest = 0) { Info i; check(pcr_backend_add_keyframes(be_, closest, n_closest, &i)); return i; }
    Info closeLoops() { Info i; check(pcr_backend_close_loops(be_, &i)); return i; }
    void step(const int64_t* closest, size_t n_closest, Info* add = nullptr, Info* lc = nullptr) { check(pcr_backend_step(be_, closest, n_closest, add, lc)); }
    std::vector<Loop> loops() const {
        size_t n = 0;
        check(pcr_backend_loops(be_, nullptr, 0, &n));
        std::vector<Loop> out(n);
        if (n) check(pcr_backend_loops(be_, out.data(), n, &n));
        return out;
    }
    void reset() { check(pcr_backend_reset(be_)); }
    // saveMapDir (pcr_backend_set_save_dir; "" = off): addKeyFrames then writes {dir}/{i}.pcd of every new key frame raw, before saveKfs' filter
    void setSaveDir(const std::string& dir) { check(pcr_backend_set_save_dir(be_, dir.c_str())); }
    // ~Backend's tum.txt and fg.g2o into the save directory (stamps: one per key frame, empty: the index)
    void save(const std::vector<double>& stamps = {}, bool precise = false) { check(pcr_backend_save(be_, stamps.empty() ? nullptr : stamps.data(), precise ? 1 : 0)); }
    // pcr_backend_load into a fresh or reset back end over an empty store: raw key frames, their contexts, the filter, the graph; the next
    // events take what comes after.  Returns the stamps.
    std::vector<double> load(const std::string& dir, Info* info = nullptr) {
        map_.usePointXYZI();
        Info i;
        check(pcr_backend_load(be_, dir.c_str(), nullptr, 0, &i));
        if (info) *info = i;
        return PCR::SubMap::stampsOf(dir, (size_t)i.keyframes);
    }
    pcr_graph* graph() { return pcr_backend_graph(be_); }
    pcr_sc* sc() { return pcr_backend_sc(be_); }
    pcr_handle* reg() { return pcr_backend_register(be_); }
    pcr_backend* handle() { return be_; }
};
}  // namespace backend

namespace PCR {
inline bool HipRegister::relocalizeGlobal(const PC_cPtr& src, const context::ScanContext& sc, const std::vector<pose_t>& kf_poses, pose_t& res,
                                          const pcr_global_reloc_params* p, std::vector<pcr_global_reloc_candidate>* cands, size_t* chosen) {
    static_assert(sizeof(pose_t) == 16 * sizeof(double), "key-frame poses are handed over as 16 doubles each");
    pcr_global_reloc_params dp;
    pcr_global_reloc_default_params(&dp);
    if (!p) p = &dp;
    std::vector<pcr_global_reloc_candidate> c((size_t)(p->places > 0 ? p->places : 0) * (size_t)(p->local.refine_top > 0 ? p->local.refine_top : 0) + 1);
    size_t nc = 0, ch = 0;
    int conv = 0;
    pose_t out = res;
    if (pcr_relocalize_global(h_, sc.handle(), kf_poses.empty() ? nullptr : kf_poses.front().data(), kf_poses.size(), src->points.data(), src->size(),
                              sizeof(PointXYZI), 0, p, out.data(), &conv, c.data(), c.size(), &nc, &ch)) {
        logError(pcr_last_error(h_));
        return isConverge = false;
    }
    lastError_.clear();
    res = out;
    c.resize(nc);
    if (cands) *cands = c;
    if (chosen) *chosen = ch;
    isConverge = conv != 0;
    return isConverge;
}
}  // namespace PCR

// common/pcp/pcp.hpp:14-28 (pcl::VoxelGrid with leaf = grid_size on all axes), on the device
namespace pcp {
inline void voxelDownSample(const PCR::PC_cPtr& cloudIn, PCR::PointCloud& cloudOut, float grid_size) {
    pcr_handle* h = pcr_create("loam", nullptr);       // any method: the filter only needs a device context
    if (!h) throw std::runtime_error(pcr_last_error(nullptr));
    const size_t n = cloudIn->size();
    std::vector<PCR::PointXYZI> tmp(n ? n : 1);
    size_t n_out = 0;
    const int rc = pcr_voxel_filter(h, cloudIn->points.data(), n, sizeof(PCR::PointXYZI), 0, grid_size, tmp.data(), n, 0, &n_out);
    const std::string msg = rc ? pcr_last_error(h) : "";
    pcr_destroy(h);
    if (rc) throw std::runtime_error(msg);
    tmp.resize(n_out);
    cloudOut.points.swap(tmp);
}
inline void voxelDownSample(PCR::PC_Ptr& cloud, float grid_size) {      // in place, like pcp.hpp:14-20
    PCR::PointCloud out;
    voxelDownSample(PCR::PC_cPtr(cloud), out, grid_size);
    cloud->points.swap(out.points);
}

// A scan's motion distortion undone (pcr_deskew; the reference has no counterpart: its points carry no time).  The sensor's motion as control poses
// at stamps; times: one float per point, seconds after t0.  deskew() runs on the registrar's handle and stream, deskewHost() on the CPU (the
// definition: the two agree bit for bit).  cloudOut may be the input's own cloud.  -> the counts; a refused call throws with the library's message.
struct DeskewMotion {
    std::vector<PCR::pose_t> poses;
    std::vector<double> stamps;
    double t0 = 0.0, t_ref = 0.0;
    pcr_deskew_motion c() const {
        static_assert(sizeof(PCR::pose_t) == 16 * sizeof(double), "poses are handed over as one array of doubles");
        if (poses.size() != stamps.size()) throw std::runtime_error("DeskewMotion: one stamp per control pose");
        return pcr_deskew_motion{poses.empty() ? nullptr : poses.front().data(), stamps.data(), stamps.size(), t0, t_ref};
    }
};
inline pcr_deskew_info deskew(PCR::HipRegister& reg, const PCR::PointCloud& cloudIn, const std::vector<float>& times, const DeskewMotion& motion, PCR::PointCloud& cloudOut) {
    if (times.size() != cloudIn.size()) throw std::runtime_error("deskew: one time per point");
    const pcr_deskew_motion m = motion.c();
    if (&cloudOut != &cloudIn) cloudOut.points.resize(cloudIn.size());
    pcr_deskew_info info;
    if (pcr_deskew(reg.handle(), cloudIn.points.data(), cloudIn.size(), sizeof(PCR::PointXYZI), 0, times.data(), PCR_TIME_F32_SECONDS, 0, &m, cloudOut.points.data(), 0, &info))
        throw std::runtime_error(pcr_last_error(reg.handle()));
    return info;
}
inline pcr_deskew_info deskewHost(const PCR::PointCloud& cloudIn, const std::vector<float>& times, const DeskewMotion& motion, PCR::PointCloud& cloudOut) {
    if (times.size() != cloudIn.size()) throw std::runtime_error("deskewHost: one time per point");
    const pcr_deskew_motion m = motion.c();
    if (&cloudOut != &cloudIn) cloudOut.points.resize(cloudIn.size());
    pcr_deskew_info info;
    if (pcr_deskew_host(cloudIn.points.data(), cloudIn.size(), sizeof(PCR::PointXYZI), times.data(), PCR_TIME_F32_SECONDS, 0, &m, cloudOut.points.data(), &info))
        throw std::runtime_error(pcr_last_error(nullptr));
    return info;
}

// common/pcp/pcp.hpp:78-263: the reference's own sparse voxel filters, on the device (pcr_voxel_filter_sparse).  Objects of both classes are
// long-lived members in the reference (LidarOdometry.hpp:58-59): each keeps one handle, and with it the device buffers, between calls.
// Output in ascending (z, y, x) voxel order; rows with a non-finite coordinate are dropped; a refused cloud throws with the library's message.
class VoxelSparseBase {
protected:
    pcr_handle* h_ = nullptr;
    pcr_voxel_sparse_params prm_;
    float _grid_size = 0.f;
    VoxelSparseBase() { pcr_voxel_sparse_default_params(&prm_); }
    ~VoxelSparseBase() { if (h_) pcr_destroy(h_); }
    VoxelSparseBase(const VoxelSparseBase& o) : prm_(o.prm_), _grid_size(o._grid_size) {}      // (a copy gets a handle of its own when it first filters)
    VoxelSparseBase& operator=(const VoxelSparseBase& o) { prm_ = o.prm_; _grid_size = o._grid_size; return *this; }
    void run(const PCR::PointCloud& in, std::vector<PCR::PointXYZI>& out) {
        if (!h_ && !(h_ = pcr_create("loam", nullptr))) throw std::runtime_error(pcr_last_error(nullptr));      // any method: the filter only needs a device context
        const size_t n = in.size();
        out.assign(n ? n : 1, PCR::PointXYZI());
        size_t n_out = 0;
        if (pcr_voxel_filter_sparse(h_, in.points.data(), n, sizeof(PCR::PointXYZI), 0, _grid_size, &prm_, out.data(), n, 0, &n_out))
            throw std::runtime_error(pcr_last_error(h_));
        out.resize(n_out);
    }
};

class VoxelDownSampleV2 : public VoxelSparseBase {
public:
    VoxelDownSampleV2() = default;
    VoxelDownSampleV2(float gs, int max_vp = 20, int min_vp = 0) {
        _grid_size = gs; prm_.kind = PCR_VOXEL_SPARSE_V2; prm_.max_voxel_pts = max_vp; prm_.min_voxel_pts = min_vp;
    }
    template <typename PointType = PCR::PointXYZI>
    PCR::PC_Ptr filter(const PCR::PC_cPtr& cloud) {
        PCR::PC_Ptr out = std::make_shared<PCR::PointCloud>();
        run(*cloud, out->points);
        return out;
    }
};

class VoxelDownSampleV3 : public VoxelSparseBase {
public:
    VoxelDownSampleV3() = default;
    VoxelDownSampleV3(float gs) { _grid_size = gs; prm_.kind = PCR_VOXEL_SPARSE_V3; }
    template <typename PointType = PCR::PointXYZI>
    void filter(const PCR::PC_cPtr& cloud, PCR::PC_Ptr& out) {
        if (cloud->points.empty()) return;                       // pcp.hpp:175
        std::vector<PCR::PointXYZI> tmp;
        run(*cloud, tmp);
        out->points.swap(tmp);                                   // (cloud.get() == out.get(), pcp.hpp:222,253: the input was read in full before this)
    }
};
}  // namespace pcp
