// submap.hip -- MapManager's key-frame store and sub-map assembly on the device (gfx950).
//
// The producer of `dst` for every scan2Map call:
//   MapManager::updateMap            frontend/src/MapManager.cpp:151-201
//     key frames within mSurroundingKeyframeSearchRadius (8 m, MapManager.hpp:68) of the current position:
//     KeyFramesKdtree::radiusSearch  third_parties/nanoflann/include/nanoflann/kfs_adaptor.hpp:57-75  (squared L2 in
//     double, strict '<' as nanoflann's RadiusResultSet accepts)
//     per key frame pcp::transformPointCloud(pose cast to float)   common/pcp/pcp.hpp:38-62   -> concatenate
//     pcp::voxelDownSample(mSubmap, mGridSize)                     common/pcp/pcp.hpp:14-20   (pcl::VoxelGrid)
// Key frames stay in HBM; an update is one transform+concatenate launch plus pcr_voxel_filter, and the sub-map it
// leaves in HBM is what pcr_scan2map_device takes as `dst` -- no host copy of the map on the registration path.
// The result does not depend on the order in which the key frames are concatenated (centroids are summed in f64).
// The back end shares the store: Backend::optimHandler's pose updates (pcr_map_set_poses), LoopClosureManager's lc_map_ as a
// view with a sub-map of its own (pcr_map_view), the stored key frames read back (pcr_map_keyframe, pcr_map_read_keyframe), saveKfs's in-place
// filter (pcr_map_downsample_keyframes) and the whole map (pcr_map_update_all) -- the same transform pass and voxel filter throughout.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pcr_hip.h"

// (library-internal, defined in capi.hip) the stream a handle queues its work on; the voxel filter in two halves (queue; synchronise and collect)
hipStream_t pcr_internal_stream(const pcr_handle* h);
int pcr_internal_vf_begin(pcr_handle* h, const void* d_pts, size_t n, size_t stride_bytes, double leaf, void* d_out, size_t out_capacity);
int pcr_internal_vf_end(pcr_handle* h, size_t* n_out);
void pcr_internal_vf_reserve(pcr_handle* h, size_t points);
// (defined in voxel_sparse_host.hip) pcp::VoxelDownSampleV3 of device memory into device memory, synchronous
int pcr_internal_vs_v3(pcr_handle* h, const void* d_pts, size_t n, size_t stride_bytes, double leaf, void* d_out, size_t out_capacity, size_t* n_out);
// (pcr_internal.h, defined in graph_host.hip) the device a pose graph lives on, PCR_GRAPH_HOST for a graph without one
namespace pcr { int graph_device(const pcr_graph* g); }

namespace {

struct KfDesc {              // one selected key frame in the concatenation
    unsigned long long src_off;   // first float of its points in the store
    unsigned int first_out;       // first output point
    unsigned int n;
    float R[9], t[3];             // pose_t cast to float (pcp.hpp:41-46), row-major rotation
};

// One thread per output point.  pto = tr * pfrom in float: ((r0 x + r1 y) + r2 z) + t per row -- Eigen's coefficient-based
// 3x3 * 3x1 product followed by the translation; compiled without FMA contraction so that the voxel a point falls
// into is the one the CPU computes.
__device__ inline void submap_transform_point(const float* __restrict__ store, const KfDesc* __restrict__ kf, int n_kf, unsigned int i, unsigned int stride,
                                              float* __restrict__ out) {
    int lo = 0, hi = n_kf - 1;                    // last key frame whose first_out <= i
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (kf[mid].first_out <= i) lo = mid; else hi = mid - 1; }
    const KfDesc d = kf[lo];
    const float* p = store + d.src_off + (size_t)(i - d.first_out) * stride;
    float* o = out + (size_t)i * stride;
    const float x = p[0], y = p[1], z = p[2];
    o[0] = ((d.R[0] * x + d.R[1] * y) + d.R[2] * z) + d.t[0];
    o[1] = ((d.R[3] * x + d.R[4] * y) + d.R[5] * z) + d.t[1];
    o[2] = ((d.R[6] * x + d.R[7] * y) + d.R[8] * z) + d.t[2];
    for (unsigned int c = 3; c < stride; ++c) o[c] = p[c];          // data[3] = 1 and the intensity travel unchanged
}

__global__ __launch_bounds__(256) void submap_transform_kernel(const float* __restrict__ store, const KfDesc* __restrict__ kf, int n_kf,
                                                               unsigned int n_total, unsigned int stride, float* __restrict__ out) {
    const unsigned int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_total) submap_transform_point(store, kf, n_kf, i, stride, out);
}

// ... the same with the descriptors in the kernel's ARGUMENTS (up to 48 key frames: 3 KB of the 4 KB a launch carries): no copy in front of the launch,
// no buffer to keep alive behind it
static constexpr int kPackMax = 48;
struct KfPack { KfDesc d[kPackMax]; };
__global__ __launch_bounds__(256) void submap_transform_pack_kernel(const float* __restrict__ store, const KfPack pack, int n_kf,
                                                                    unsigned int n_total, unsigned int stride, float* __restrict__ out) {
    const unsigned int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_total) submap_transform_point(store, pack.d, n_kf, i, stride, out);
}

struct Buf {
    void* p = nullptr; size_t cap = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }
    // keep: the contents move along (the key-frame store); the other buffers are written anew by every assembly
    hipError_t reserve(size_t bytes, bool keep = true) {
        if (bytes <= cap) return hipSuccess;
        void* q = nullptr;
        const size_t want = 2 * bytes + 4096;      // (doubling: every growth is a device-wide stop -- allocation, copy, free -- and a session's first minutes are made of them)
        hipError_t e = hipMalloc(&q, want);
        if (e != hipSuccess) return e;
        if (p && !keep) (void)hipFree(p);
        else if (p) { e = hipMemcpy(q, p, cap, hipMemcpyDeviceToDevice); (void)hipFree(p); if (e != hipSuccess) { (void)hipFree(q); p = nullptr; cap = 0; return e; } }
        p = q; cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

}  // namespace

static constexpr int kWindow = 16;      // key frames a sub-map is expected to hold (8 m radius, a key frame per metre: MapManager.hpp:67-68)

struct pcr_map {
    int device = 0;
    pcr_handle* filter = nullptr;     // device context of the voxel filter
    size_t stride = 0;                // bytes per point, fixed by the first key frame
    Buf store, concat, submap, desc;
    KfDesc* desc_host = nullptr;      // page-locked staging of the descriptors
    size_t desc_host_cap = 0;
    size_t store_floats = 0;
    struct Kf { size_t off_floats, n; double pose[16]; };
    std::vector<Kf> kfs;
    std::vector<long long> selected;  // mSubmapIdx
    size_t n_submap = 0;
    size_t max_kf_points = 0;         // the largest key frame so far: buffers are sized for a window of kWindow such key frames from the start
    bool pending = false;             // an assembly is queued on the filter's stream and has not been collected (pcr_map_update_begin): n_submap is not known yet
    uint64_t id = 0, generation = 0;  // identity of this store and of the sub-map it currently holds (every update is a new generation)
    std::string err;
    // A view (pcr_map_view: LoopClosureManager's lc_map_ beside MapManager's mSubmap) has everything above for ITS sub-map -- filter handle and stream,
    // concat / submap / desc buffers, selection, pending flag, id and generation -- and reads stride, store, store_floats, kfs and max_kf_points of
    // its parent (store_of); its own copies of those stay empty.
    pcr_map* parent = nullptr;
    bool detached = false;            // a view whose parent has been destroyed: every call fails, pcr_map_destroy frees it
    std::vector<pcr_map*> views;      // (parent) the views that read this store
    std::mutex views_mu;              // guards `views`: a view may be created and destroyed from different threads
    Buf scratch;                      // (parent) pcr_map_downsample_keyframes filters a key frame into it and copies back
    Buf rank;                         // pcr_map_rank_near (kf_rank.hip): the positions it uploads and the rows it reads back; a view has its own
};

static thread_local std::string g_map_err;
static int mfail(pcr_map* m, const std::string& s) { if (m) m->err = s; else g_map_err = s; return 1; }
static int mfail(const pcr_map* m, const std::string& s) { return mfail(const_cast<pcr_map*>(m), s); }
static const pcr_map* store_of(const pcr_map* m) { return m->parent ? m->parent : m; }
namespace pcr { int map_device(const pcr_map* m) { return m->device; } }      // (pcr_internal.h: the device a store, or a view of one, lives on)
// (pcr_internal.h, for kf_rank.hip) pcr_map_last_error's message set from another unit, and this object's own buffer for the ranking
namespace pcr {
int map_set_error(const pcr_map* m, const std::string& s) { return mfail(m, s); }
void* map_scratch(const pcr_map* m, size_t bytes) {
    pcr_map* w = const_cast<pcr_map*>(m);
    return w->rank.reserve(bytes, false) == hipSuccess ? w->rank.p : nullptr;
}
}  // namespace pcr
// every entry point but pcr_map_destroy: a view that outlived its parent has no store to read
#define M_ALIVE(m) do { if ((m)->detached) return mfail(m, "parent destroyed: this view can only be destroyed"); } while (0)
#define M_OWNER(m, what) do { if ((m)->parent) return mfail(m, std::string(what) + ": this pcr_map is a view (pcr_map_view) and cannot change the store; call it on the parent"); } while (0)
#define M_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return mfail(m, std::string(#x) + ": " + hipGetErrorString(_e)); } while (0)

// collect the queued assembly, if any: the one synchronisation of an update (and the filter's second try when the index's hints did not hold)
static int finish_pending(pcr_map* m) {
    if (!m->pending) return 0;
    m->pending = false;
    m->n_submap = 0;
    M_TRY(hipSetDevice(m->device));
    size_t n_out = 0;
    if (pcr_internal_vf_end(m->filter, &n_out)) return mfail(m, std::string("voxel filter: ") + pcr_last_error(m->filter));
    m->n_submap = n_out;
    return 0;
}

// Every view's queued assembly has run: its transform pass is the one thing of a view that reads the parent's store (the filter behind it reads the
// view's own concatenation).  The view keeps its pending flag and collects the result itself.
static int views_quiesce(pcr_map* m) {
    std::lock_guard<std::mutex> g(m->views_mu);
    for (pcr_map* v : m->views) M_TRY(hipStreamSynchronize(pcr_internal_stream(v->filter)));
    return 0;
}

extern "C" {

pcr_map* pcr_map_create(int device) {
    pcr_params p;
    pcr_default_params(&p);
    p.device = device;
    pcr_handle* h = pcr_create("loam", &p);
    if (!h) { g_map_err = pcr_last_error(nullptr); return nullptr; }
    static std::atomic<uint64_t> next_id{1};
    pcr_map* m = new pcr_map;
    m->id = next_id.fetch_add(1);
    m->filter = h;
    if (device >= 0) m->device = device; else (void)hipGetDevice(&m->device);
    return m;
}

pcr_map* pcr_map_view(pcr_map* parent) {
    if (!parent) { g_map_err = "map is NULL"; return nullptr; }
    parent->err.clear();
    if (parent->detached) { mfail(parent, "parent destroyed: this view can only be destroyed"); return nullptr; }
    if (parent->parent) { mfail(parent, "pcr_map_view: this pcr_map is a view (pcr_map_view) and cannot change the store; call it on the parent"); return nullptr; }
    pcr_map* v = pcr_map_create(parent->device);
    if (!v) { mfail(parent, g_map_err); return nullptr; }
    v->parent = parent;
    std::lock_guard<std::mutex> g(parent->views_mu);
    parent->views.push_back(v);
    return v;
}

void pcr_map_destroy(pcr_map* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->parent) {      // a view of a living store: the parent forgets it
        std::lock_guard<std::mutex> g(m->parent->views_mu);
        std::vector<pcr_map*>& vs = m->parent->views;
        vs.erase(std::remove(vs.begin(), vs.end(), m), vs.end());
    }
    for (pcr_map* v : m->views) {      // a store with views: what they have queued reads it -- waited for; then they are on their own
        (void)hipStreamSynchronize(pcr_internal_stream(v->filter));
        v->parent = nullptr; v->detached = true;
    }
    m->views.clear();
    pcr_destroy(m->filter);           // (first: it waits for whatever is still queued on its stream -- an assembly nobody collected reads the buffers m holds)
    if (m->desc_host) (void)hipHostFree(m->desc_host);
    delete m;
}

const char* pcr_map_last_error(const pcr_map* m) { return m ? m->err.c_str() : g_map_err.c_str(); }

int pcr_map_add_keyframe(pcr_map* m, const void* pts, size_t n, size_t stride_bytes, int on_device, const double pose[16]) {
    if (!m) return 1;
    m->err.clear();
    M_ALIVE(m);
    M_OWNER(m, "pcr_map_add_keyframe");
    if (n && !pts) return mfail(m, "NULL cloud with nonzero size");
    if (!pose) return mfail(m, "NULL pose");
    if (stride_bytes < 12 || stride_bytes % 4) return mfail(m, "stride_bytes must be a multiple of 4 and >= 12");
    if (m->stride == 0) m->stride = stride_bytes;
    else if (m->stride != stride_bytes) return mfail(m, "all key frames of a map must share one point layout");
    M_TRY(hipSetDevice(m->device));
    if (finish_pending(m)) return 1;      // (a queued assembly reads the store, which may move below)
    if (views_quiesce(m)) return 1;       // (... and so does a view's)
    const size_t nf = n * (stride_bytes / 4);
    m->max_kf_points = std::max(m->max_kf_points, n);
    // (room for a window of key frames from the first one on: a store that grows is copied, and every growth is a device-wide stop)
    M_TRY(m->store.reserve((std::max(m->store_floats + nf, (size_t)kWindow * nf) + 4) * sizeof(float)));
    if (nf && on_device) {      // on the filter's stream, waited for: the caller may reuse its buffer when this returns (the blocking copy on the null stream took 60 us for 1 MB, round 5)
        hipStream_t fs = pcr_internal_stream(m->filter);
        M_TRY(hipMemcpyAsync(static_cast<float*>(m->store.p) + m->store_floats, pts, nf * sizeof(float), hipMemcpyDeviceToDevice, fs));
        M_TRY(hipStreamSynchronize(fs));
    } else if (nf) M_TRY(hipMemcpy(static_cast<float*>(m->store.p) + m->store_floats, pts, nf * sizeof(float), hipMemcpyHostToDevice));
    pcr_map::Kf k;
    k.off_floats = m->store_floats; k.n = n;
    for (int i = 0; i < 16; ++i) k.pose[i] = pose[i];
    m->kfs.push_back(k);
    m->store_floats += nf;
    return 0;
}

int pcr_map_clear(pcr_map* m) {
    if (!m) return 1;
    m->err.clear();
    M_ALIVE(m);
    M_OWNER(m, "pcr_map_clear");
    M_TRY(hipSetDevice(m->device));
    (void)finish_pending(m); m->err.clear();
    m->kfs.clear(); m->selected.clear();
    m->store_floats = 0; m->n_submap = 0;
    m->generation += 1;           // whatever was built from the previous sub-map is stale
    std::lock_guard<std::mutex> g(m->views_mu);
    for (pcr_map* v : m->views) {      // ... and so is every view's: waited for, dropped, a new generation
        (void)finish_pending(v); v->err.clear();
        v->selected.clear();
        v->n_submap = 0;
        v->generation += 1;
    }
    return 0;
}

int pcr_map_keyframes(const pcr_map* m, size_t* n_keyframes) {
    if (!m || !n_keyframes) return 1;
    M_ALIVE(m);
    *n_keyframes = store_of(m)->kfs.size();
    return 0;
}

int pcr_map_set_poses(pcr_map* m, size_t first, size_t count, const double* poses) {
    if (!m) return 1;
    m->err.clear();
    M_ALIVE(m);
    M_OWNER(m, "pcr_map_set_poses");
    if (first > m->kfs.size() || count > m->kfs.size() - first) return mfail(m, "pcr_map_set_poses: first + count exceeds the number of key frames");
    if (count == 0) return 0;
    if (!poses) return mfail(m, "NULL poses");
    // An assembly that is queued was selected, and its descriptors were written, under the poses as they are: it finishes as such before they change.
    M_TRY(hipSetDevice(m->device));
    M_TRY(hipStreamSynchronize(pcr_internal_stream(m->filter)));
    if (views_quiesce(m)) return 1;
    for (size_t i = 0; i < count; ++i) memcpy(m->kfs[first + i].pose, poses + 16 * i, 16 * sizeof(double));
    return 0;      // (no sub-map, selection or generation is touched: the reference's mSubmap stays what it is until the next updateMap)
}

// The optimiser's poses straight from the graph's device memory (graph_host.hip) into the store's pose table, which lives on the host next to
// the key frames' offsets: one copy, no buffer of the caller's in between.  Everything else is pcr_map_set_poses.
int pcr_map_set_poses_from_graph(pcr_map* m, const pcr_graph* g, size_t first, size_t count) {
    if (!m) return 1;
    m->err.clear();
    M_ALIVE(m);
    M_OWNER(m, "pcr_map_set_poses_from_graph");
    if (!g) return mfail(m, "pcr_map_set_poses_from_graph: graph is NULL");
    if (pcr::graph_device(g) != m->device)
        return mfail(m, "pcr_map_set_poses_from_graph: the graph (device " + std::to_string(pcr::graph_device(g)) + ") and the map (device " +
                            std::to_string(m->device) + ") are on different devices");
    if (first > m->kfs.size() || count > m->kfs.size() - first) return mfail(m, "pcr_map_set_poses_from_graph: first + count exceeds the number of key frames");
    size_t n_graph = 0;
    if (pcr_graph_size(g, &n_graph, nullptr, nullptr)) return mfail(m, "pcr_map_set_poses_from_graph: the graph is not usable");
    if (first > n_graph || count > n_graph - first) return mfail(m, "pcr_map_set_poses_from_graph: first + count exceeds the number of poses in the graph");
    if (count == 0) return 0;
    M_TRY(hipSetDevice(m->device));
    size_t n_dev = 0;
    const double* d = pcr_graph_device_poses(g, &n_dev);
    if (!d || n_dev < first + count) return mfail(m, std::string("pcr_map_set_poses_from_graph: ") + pcr_graph_last_error(g));
    std::vector<double> tmp(16 * count);
    M_TRY(hipMemcpy(tmp.data(), d + 16 * first, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
    return pcr_map_set_poses(m, first, count, tmp.data());
}

const void* pcr_map_keyframe(const pcr_map* m, size_t i, size_t* n, size_t* stride_bytes, double pose[16]) {
    if (n) *n = 0;
    if (stride_bytes) *stride_bytes = 0;
    if (!m) return nullptr;
    if (m->detached) { mfail(m, "parent destroyed: this view can only be destroyed"); return nullptr; }
    const pcr_map* s = store_of(m);
    if (stride_bytes) *stride_bytes = s->stride;
    if (i >= s->kfs.size()) { mfail(m, "key-frame index out of range"); return nullptr; }
    const pcr_map::Kf& k = s->kfs[i];
    if (n) *n = k.n;
    if (pose) memcpy(pose, k.pose, 16 * sizeof(double));
    return k.n ? static_cast<const float*>(s->store.p) + k.off_floats : nullptr;
}

int pcr_map_read_keyframe(const pcr_map* m, size_t i, void* out, size_t capacity_points, size_t* n, double pose[16]) {
    if (!m) return 1;
    M_ALIVE(m);
    const pcr_map* s = store_of(m);
    if (i >= s->kfs.size()) return mfail(m, "key-frame index out of range");
    const pcr_map::Kf& k = s->kfs[i];
    if (n) *n = k.n;
    if (capacity_points < k.n) return mfail(m, "output capacity too small: the key frame holds " + std::to_string(k.n) + " points");
    if (k.n && !out) return mfail(m, "NULL output");
    if (pose) memcpy(pose, k.pose, 16 * sizeof(double));
    if (k.n == 0) return 0;
    M_TRY(hipSetDevice(m->device));
    // (the null stream's blocking copy: whatever wrote these bytes -- pcr_map_add_keyframe, pcr_map_downsample_keyframes -- synchronised before it returned)
    M_TRY(hipMemcpy(out, static_cast<const float*>(s->store.p) + k.off_floats, k.n * s->stride, hipMemcpyDeviceToHost));
    return 0;
}

int pcr_map_downsample_keyframes(pcr_map* m, size_t first, double grid_size, size_t* store_points_after) {
    if (!m) return 1;
    m->err.clear();
    M_ALIVE(m);
    M_OWNER(m, "pcr_map_downsample_keyframes");
    if (first > m->kfs.size()) return mfail(m, "pcr_map_downsample_keyframes: first exceeds the number of key frames");
    if (!(grid_size > 0)) return mfail(m, "grid_size must be positive");
    const size_t sf = m->stride / 4;
    if (store_points_after) *store_points_after = sf ? m->store_floats / sf : 0;
    if (first == m->kfs.size()) return 0;
    M_TRY(hipSetDevice(m->device));
    if (finish_pending(m)) return 1;      // (queued assemblies read the store; this one's filter handle is about to be used)
    if (views_quiesce(m)) return 1;
    size_t largest = 0;
    for (size_t i = first; i < m->kfs.size(); ++i) largest = std::max(largest, m->kfs[i].n);
    if (largest > 0xfffffff0ull) return mfail(m, "key frame too large");
    M_TRY(m->scratch.reserve((largest ? largest : 1) * m->stride, false));
    hipStream_t fs = pcr_internal_stream(m->filter);
    float* base = static_cast<float*>(m->store.p);
    size_t w = m->kfs[first].off_floats;      // where the next key frame goes: never beyond where it is now
    for (size_t i = first; i < m->kfs.size(); ++i) {
        pcr_map::Kf& k = m->kfs[i];
        size_t n_out = 0;
        if (k.n) {
            // into scratch and back: written in place, a key frame's result would land on points of it that the filter has yet to read
            if (pcr_internal_vf_begin(m->filter, base + k.off_floats, k.n, m->stride, grid_size, m->scratch.p, k.n) || pcr_internal_vf_end(m->filter, &n_out))
                return mfail(m, std::string("voxel filter: ") + pcr_last_error(m->filter));
            M_TRY(hipMemcpyAsync(base + w, m->scratch.p, n_out * m->stride, hipMemcpyDeviceToDevice, fs));
            M_TRY(hipStreamSynchronize(fs));      // (the key frame is in its place before its entry says so)
        }
        k.off_floats = w; k.n = n_out;
        w += n_out * sf;
    }
    m->store_floats = w;
    if (store_points_after) *store_points_after = w / sf;
    return 0;
}

// transform + concatenate the selected key frames (m->selected, ascending) into m->concat, queued on the filter's stream; room for the result in m->submap
static int concat_selected(pcr_map* m, size_t* n_total) {
    const pcr_map* s = store_of(m);
    *n_total = 0;
    std::vector<KfDesc> desc;
    size_t total = 0;
    for (long long i : m->selected) {
        const pcr_map::Kf& k = s->kfs[(size_t)i];
        if (k.n == 0) continue;
        if (total + k.n > 0xfffffff0ull) return mfail(m, "sub-map too large");
        KfDesc e;
        e.src_off = k.off_floats; e.first_out = (unsigned int)total; e.n = (unsigned int)k.n;
        for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) e.R[r * 3 + c] = (float)k.pose[c * 4 + r]; e.t[r] = (float)k.pose[12 + r]; }
        desc.push_back(e);
        total += k.n;
    }
    if (total == 0) return 0;
    const size_t stride = s->stride, sf = stride / 4;
    const size_t room = std::max(total, (size_t)kWindow * s->max_kf_points);      // (the concatenation of a window of key frames: the buffers, the filter's and its index's, start at that size)
    M_TRY(m->concat.reserve(room * stride, false));
    M_TRY(m->submap.reserve(room * stride, false));
    pcr_internal_vf_reserve(m->filter, room);
    M_TRY(m->desc.reserve(desc.size() * sizeof(KfDesc), false));
    // the descriptors and the transform pass go onto the FILTER's stream, in front of the filter's own launches: one synchronisation -- the filter's,
    // for its voxel count -- serves the whole assembly (round 4: a blocking copy, the pass on the null stream, a device-wide synchronisation, then the
    // filter with two more: 0.49 ms for a 500 k-point concatenation of which a third was waiting; round 5, scripts/seq_breakdown.py)
    hipStream_t fs = pcr_internal_stream(m->filter);
    if (desc.size() <= (size_t)kPackMax) {
        KfPack pack;
        memcpy(pack.d, desc.data(), desc.size() * sizeof(KfDesc));
        hipLaunchKernelGGL(submap_transform_pack_kernel, dim3((unsigned int)((total + 255) / 256)), dim3(256), 0, fs, static_cast<const float*>(s->store.p),
                           pack, (int)desc.size(), (unsigned int)total, (unsigned int)sf, static_cast<float*>(m->concat.p));
    } else {
    if (m->desc_host_cap < desc.size()) {
        if (m->desc_host) (void)hipHostFree(m->desc_host);
        m->desc_host = nullptr; m->desc_host_cap = 0;
        M_TRY(hipHostMalloc((void**)&m->desc_host, (desc.size() + 64) * sizeof(KfDesc), hipHostMallocDefault));
        m->desc_host_cap = desc.size() + 64;
    }
    memcpy(m->desc_host, desc.data(), desc.size() * sizeof(KfDesc));      // (page-locked staging: the copy below does not block; the previous assembly's has completed -- its filter synchronised)
    M_TRY(hipMemcpyAsync(m->desc.p, m->desc_host, desc.size() * sizeof(KfDesc), hipMemcpyHostToDevice, fs));
    hipLaunchKernelGGL(submap_transform_kernel, dim3((unsigned int)((total + 255) / 256)), dim3(256), 0, fs, static_cast<const float*>(s->store.p),
                       static_cast<const KfDesc*>(m->desc.p), (int)desc.size(), (unsigned int)total, (unsigned int)sf, static_cast<float*>(m->concat.p));
    }
    M_TRY(hipGetLastError());
    *n_total = total;
    return 0;
}

// transform + concatenate the selected key frames (m->selected, ascending) and voxel-filter the result into m->submap
static int assemble_selected(pcr_map* m, double grid_size, size_t* n_submap, bool wait = true) {
    size_t total = 0;
    if (concat_selected(m, &total)) return 1;
    if (total == 0) return 0;
    const size_t stride = store_of(m)->stride;
    if (pcr_internal_vf_begin(m->filter, m->concat.p, total, stride, grid_size, m->submap.p, total))
        return mfail(m, std::string("voxel filter: ") + pcr_last_error(m->filter));
    m->pending = true;
    if (!wait) return 0;
    if (finish_pending(m)) return 1;
    if (n_submap) *n_submap = m->n_submap;
    return 0;
}

static int update_by_radius(pcr_map* m, const double position[3], double radius, double grid_size, size_t* n_submap, bool wait) {
    if (!m) return 1;
    m->err.clear();
    M_ALIVE(m);
    if (!position) return mfail(m, "NULL position");
    if (!(grid_size > 0)) return mfail(m, "grid_size must be positive");
    M_TRY(hipSetDevice(m->device));
    (void)finish_pending(m); m->err.clear();      // (an assembly nobody collected: waited for -- its buffers are about to be written again -- and superseded, whatever became of it)
    m->selected.clear();
    m->n_submap = 0;
    m->generation += 1;           // whatever happens below, the previous sub-map is gone
    if (n_submap) *n_submap = 0;
    const std::vector<pcr_map::Kf>& kfs = store_of(m)->kfs;
    if (kfs.empty()) return 0;                             // "no any keyframes to update!!" (MapManager.cpp:166-169)
    // radius search over the key-frame positions: squared distance in double, accumulated x, y, z; strict '<'
    const double r2 = radius * radius;
    for (size_t i = 0; i < kfs.size(); ++i) {
        double d = 0;
        for (int c = 0; c < 3; ++c) { const double e = position[c] - kfs[i].pose[12 + c]; d += e * e; }
        if (d < r2) m->selected.push_back((long long)i);
    }
    return assemble_selected(m, grid_size, n_submap, wait);
}

int pcr_map_update(pcr_map* m, const double position[3], double radius, double grid_size, size_t* n_submap) {
    return update_by_radius(m, position, radius, grid_size, n_submap, true);
}

int pcr_map_update_begin(pcr_map* m, const double position[3], double radius, double grid_size) {
    return update_by_radius(m, position, radius, grid_size, nullptr, false);
}

int pcr_map_wait(pcr_map* m, size_t* n_submap) {
    if (!m) return 1;
    if (n_submap) *n_submap = 0;
    M_ALIVE(m);
    if (m->pending) m->err.clear();
    if (finish_pending(m)) return 1;
    if (n_submap) *n_submap = m->n_submap;
    return 0;
}

int pcr_map_update_window(pcr_map* m, long long key, int search_num, double grid_size, size_t* n_submap) {
    if (!m) return 1;
    m->err.clear();
    M_ALIVE(m);
    if (!(grid_size > 0)) return mfail(m, "grid_size must be positive");
    if (search_num < 0) return mfail(m, "search_num must not be negative");
    M_TRY(hipSetDevice(m->device));
    (void)finish_pending(m); m->err.clear();
    m->selected.clear();
    m->n_submap = 0;
    m->generation += 1;           // whatever happens below, the previous sub-map is gone
    if (n_submap) *n_submap = 0;
    const long long count = (long long)store_of(m)->kfs.size();
    for (long long i = -(long long)search_num; i <= (long long)search_num; ++i) {      // LoopClosureManager.cpp:46-57
        const long long near = key + i;
        if (near >= 0 && near < count) m->selected.push_back(near);
    }
    return assemble_selected(m, grid_size, n_submap);
}

int pcr_map_update_all(pcr_map* m, double grid_size, size_t* n_submap) {
    if (!m) return 1;
    m->err.clear();
    M_ALIVE(m);
    if (!(grid_size > 0)) return mfail(m, "grid_size must be positive");
    M_TRY(hipSetDevice(m->device));
    (void)finish_pending(m); m->err.clear();
    m->selected.clear();
    m->n_submap = 0;
    m->generation += 1;           // whatever happens below, the previous sub-map is gone
    if (n_submap) *n_submap = 0;
    const size_t count = store_of(m)->kfs.size();
    for (size_t i = 0; i < count; ++i) m->selected.push_back((long long)i);      // test/vis_globalmap.cpp:40-47
    return assemble_selected(m, grid_size, n_submap);
}

int pcr_map_update_all_sparse(pcr_map* m, double grid_size, size_t* n_submap) {
    if (!m) return 1;
    m->err.clear();
    M_ALIVE(m);
    if (!(grid_size > 0)) return mfail(m, "grid_size must be positive");
    M_TRY(hipSetDevice(m->device));
    (void)finish_pending(m); m->err.clear();
    m->selected.clear();
    m->n_submap = 0;
    m->generation += 1;           // whatever happens below, the previous sub-map is gone
    if (n_submap) *n_submap = 0;
    const size_t count = store_of(m)->kfs.size();
    for (size_t i = 0; i < count; ++i) m->selected.push_back((long long)i);
    size_t total = 0, n_out = 0;
    if (concat_selected(m, &total)) return 1;
    if (total == 0) return 0;
    // pcp::VoxelDownSampleV3 where pcr_map_update_all runs pcl::VoxelGrid: behind the transform pass on the same stream, collected at once
    if (pcr_internal_vs_v3(m->filter, m->concat.p, total, store_of(m)->stride, grid_size, m->submap.p, total, &n_out))
        return mfail(m, std::string("sparse voxel filter: ") + pcr_last_error(m->filter));
    m->n_submap = n_out;
    if (n_submap) *n_submap = n_out;
    return 0;
}

const void* pcr_map_submap(const pcr_map* m, size_t* n, size_t* stride_bytes) {
    if (!m) return nullptr;
    const size_t stride = m->detached ? 0 : store_of(m)->stride;
    if (m->detached) mfail(m, "parent destroyed: this view can only be destroyed");
    if (m->detached || (m->pending && finish_pending(const_cast<pcr_map*>(m)))) { if (n) *n = 0; if (stride_bytes) *stride_bytes = stride; return nullptr; }      // (the queued assembly is collected by whoever asks for the sub-map first; its error is pcr_map_last_error's)
    if (n) *n = m->n_submap;
    if (stride_bytes) *stride_bytes = stride;
    return m->n_submap ? m->submap.p : nullptr;
}

int pcr_map_generation(const pcr_map* m, uint64_t* id, uint64_t* generation) {
    if (!m) return 1;
    M_ALIVE(m);
    if (id) *id = m->id;
    if (generation) *generation = m->generation;
    return 0;
}

int pcr_map_submap_indices(const pcr_map* m, int64_t* idx, size_t capacity, size_t* n) {
    if (!m || !n) return 1;
    *n = 0;
    M_ALIVE(m);
    *n = m->selected.size();
    if (!idx) return 0;
    if (capacity < m->selected.size()) return 1;
    for (size_t i = 0; i < m->selected.size(); ++i) idx[i] = m->selected[i];
    return 0;
}

}  // extern "C"
