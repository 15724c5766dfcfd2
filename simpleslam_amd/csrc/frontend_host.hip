// frontend_host.hip -- the caller's per-scan loop (pcr_frontend_*) and trans::SixDof2Mobile (pcr_pose_to_mobile).  Host code only: the loop
// strings together entry points that exist -- pcr_voxel_filter(_begin / _end), pcr_scan2map_submap, pcr_map_add_keyframe, pcr_map_update_begin,
// pcr_map_wait -- in the order of simpleslam_amd/sequence.py's drive() over GpuFront, and owns nothing but the filtered scans' buffers, the second
// filter handle and the key-frame positions.  DESIGN 4.16.

#include <chrono>

#include "handle.h"

using namespace pcr;
using namespace pcr::host;

namespace {

thread_local std::string g_frontend_error;      // what pcr_frontend_last_error(NULL) returns

// a filter that pcr_frontend_prefetch queued (on fe->filt, into fe->out[slot]) or has collected since
struct Ahead {
    bool on = false;
    const void* scan = nullptr;
    size_t n = 0, stride = 0;
    int slot = 0;
    size_t count = 0;       // collected: the voxels
    bool is(const void* s, size_t n_, size_t st) const { return on && scan == s && n == n_ && stride == st; }
};

double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

}  // namespace

struct pcr_frontend {
    pcr_handle* reg = nullptr;      // borrowed
    pcr_map* map = nullptr;         // borrowed
    pcr_frontend_params prm{};
    int device = 0;
    pcr_handle* filt = nullptr;     // pcr_frontend_prefetch: the filter's own handle (a stream of its own), created on first use
    DeviceBuf out[2], direct;       // filtered scans: the two a prefetch alternates between, and the one of a step that filters for itself
    DeviceBuf up_ahead[2];          // pcr_frontend_prefetch: host scans on their way in
    DeviceBuf deskewed;             // pcr_frontend_step_timed: the scan with its motion taken out, which the step then runs on
    Ahead queued, ready;            // the filter in flight on `filt`; the one collected and not yet taken by a step
    std::vector<double> kf_pos;     // key-frame positions, xyz each
    std::vector<int64_t> closest;   // per key frame this front end added: the key frame step 6 found nearest, -1 for the first (mClosestKfIdx, MapManager.cpp:146)
    bool have_update = false;       // an assembly has happened (setCurPose)
    double last_update[3] = {0, 0, 0};
    bool assembly_queued = false;   // pcr_map_update_begin has queued one that nobody collected
    size_t n_submap = 0;            // ... else: the sub-map's points
    long long updates = 0;
    bool failed = false;            // an inner call of a step failed: the loop's state is partial until pcr_frontend_reset
    std::string failure;            // ... and what it said
    std::string err;
};

namespace {

int ffail(pcr_frontend* fe, const std::string& msg) { fe->err = msg; return 1; }
// an inner call failed: its message under the step's name; the front end refuses further steps until it is reset
int inner_fail(pcr_frontend* fe, const char* step, const char* msg) {
    fe->failed = true;
    fe->failure = std::string(step) + ": " + (msg && *msg ? msg : "failed");
    return ffail(fe, fe->failure);
}
#define FE_HIP(step, x) do { hipError_t _e = (x); if (_e != hipSuccess) return inner_fail(fe, step, (std::string(#x) + ": " + hipGetErrorString(_e)).c_str()); } while (0)

// the filter in flight is collected: it becomes `ready` (an earlier one that no step took is dropped)
int collect_queued(pcr_frontend* fe) {
    if (!fe->queued.on) return 0;
    fe->ready = fe->queued;
    fe->queued.on = false;
    if (pcr_voxel_filter_end(fe->filt, &fe->ready.count)) { fe->ready.on = false; return inner_fail(fe, "voxel", pcr_last_error(fe->filt)); }
    return 0;
}

int collect_assembly(pcr_frontend* fe, const char* step) {
    if (!fe->assembly_queued) return 0;
    fe->assembly_queued = false;
    fe->n_submap = 0;
    if (pcr_map_wait(fe->map, &fe->n_submap)) return inner_fail(fe, step, pcr_map_last_error(fe->map));
    return 0;
}

int check_scan(pcr_frontend* fe, const void* scan, size_t n, const double* pose_a, const void* pose_b) {
    if (n == 0) return ffail(fe, "a scan of 0 points cannot be registered or kept");
    if (!scan) return ffail(fe, "scan is NULL");
    if (n > kMaxPoints) return ffail(fe, "scan too large");
    if (!pose_a || !pose_b) return ffail(fe, "pose is NULL");
    return 0;
}

}  // namespace

extern "C" {

int pcr_pose_to_mobile(const double T[16], double out[16]) {
    if (!T || !out) return 1;
    // column-major: m(r, c) = T[c * 4 + r]
    const double m[3][3] = {{T[0], T[4], T[8]}, {T[1], T[5], T[9]}, {T[2], T[6], T[10]}};
    const double tx = T[12], ty = T[13];
    // Eigen::Quaternion(Matrix3) (Eigen/src/Geometry/Quaternion.h: quaternionbase_assign_impl<Other, 3, 3>)
    double q[3], w;
    double t = (m[0][0] + m[1][1]) + m[2][2];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        w = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[2][1] - m[1][2]) * t;
        q[1] = (m[0][2] - m[2][0]) * t;
        q[2] = (m[1][0] - m[0][1]) * t;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        w = (m[k][j] - m[j][k]) * t;
        q[j] = (m[j][i] + m[i][j]) * t;
        q[k] = (m[k][i] + m[i][k]) * t;
    }
    // Eigen::AngleAxis(Quaternion) (Eigen/src/Geometry/AngleAxis.h: operator=(QuaternionBase))
    double n = sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    double angle = 0.0, axis_z = 0.0;      // (n == 0: axis (1, 0, 0))
    if (n != 0.0) {
        angle = 2.0 * atan2(n, fabs(w));
        if (w < 0.0) n = -n;
        axis_z = q[2] / n;
    }
    for (int i = 0; i < 16; ++i) out[i] = (i % 5 == 0) ? 1.0 : 0.0;
    out[12] = tx; out[13] = ty;
    if (fabs(axis_z) > 0.95) {      // AngleAxis(angle, copysign(1, axis.z) * UnitZ).toRotationMatrix()
        const double a = copysign(1.0, axis_z), c = cos(angle), s = sin(angle);
        out[0] = c; out[5] = c;
        out[4] = -(a * s);      // R01
        out[1] = a * s;         // R10
        out[10] = (1.0 - c) + c;
    }
    return 0;
}

void pcr_frontend_default_params(pcr_frontend_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->grid_size = 0.5;
    p->radius = 8.0;
    p->kf_gap = 1.0;
    p->mobile = 0;
}

pcr_frontend* pcr_frontend_create(pcr_handle* reg, pcr_map* map, const pcr_frontend_params* p) {
    if (!reg) { g_frontend_error = "pcr_frontend_create: the register is NULL"; return nullptr; }
    if (!map) { g_frontend_error = "pcr_frontend_create: the map is NULL"; return nullptr; }
    pcr_frontend_params prm;
    pcr_frontend_default_params(&prm);
    if (p) prm = *p;
    if (!(prm.grid_size > 0)) { g_frontend_error = "pcr_frontend_create: grid_size must be positive"; return nullptr; }
    if (!(prm.radius > 0)) { g_frontend_error = "pcr_frontend_create: radius must be positive"; return nullptr; }
    if (!(prm.kf_gap >= 0)) { g_frontend_error = "pcr_frontend_create: kf_gap must not be negative"; return nullptr; }
    size_t n_kf = 0;
    if (pcr_map_keyframes(map, &n_kf)) { g_frontend_error = std::string("pcr_frontend_create: ") + pcr_map_last_error(map); return nullptr; }
    pcr_frontend* fe = new pcr_frontend;
    fe->reg = reg; fe->map = map; fe->prm = prm;
    fe->device = reg->device;
    // a store that holds key frames already is taken over as it is: their positions, and the sub-map it holds
    for (size_t i = 0; i < n_kf; ++i) {
        size_t n = 0, stride = 0;
        double pose[16];
        (void)pcr_map_keyframe(map, i, &n, &stride, pose);
        fe->kf_pos.insert(fe->kf_pos.end(), {pose[12], pose[13], pose[14]});
    }
    fe->assembly_queued = true;      // (pcr_map_wait returns what the map holds, queued or not)
    return fe;
}

void pcr_frontend_destroy(pcr_frontend* fe) {
    if (!fe) return;
    (void)hipSetDevice(fe->device);
    if (fe->queued.on) { size_t n = 0; (void)pcr_voxel_filter_end(fe->filt, &n); }      // (it writes a buffer that goes with fe)
    if (fe->filt) pcr_destroy(fe->filt);
    (void)hipStreamSynchronize(fe->reg->stream);      // (the last registration read a filtered scan of fe's)
    delete fe;
}

const char* pcr_frontend_last_error(const pcr_frontend* fe) { return fe ? fe->err.c_str() : g_frontend_error.c_str(); }

int pcr_frontend_prefetch(pcr_frontend* fe, const void* next_scan, size_t n, size_t stride_bytes, int on_device) {
    if (!fe) return 1;
    fe->err.clear();
    if (fe->failed) return ffail(fe, "an earlier step of this front end failed (" + fe->failure + "): pcr_frontend_reset starts over");
    if (n == 0) return ffail(fe, "a scan of 0 points cannot be registered or kept");
    if (!next_scan) return ffail(fe, "scan is NULL");
    if (n > kMaxPoints) return ffail(fe, "scan too large");
    FE_HIP("voxel", hipSetDevice(fe->device));
    if (!fe->filt) {
        pcr_params p;
        pcr_default_params(&p);
        p.device = fe->device;
        fe->filt = pcr_create("loam", &p);      // (any method: the filter is the handle's, not the registrar's)
        if (!fe->filt) return inner_fail(fe, "voxel", pcr_last_error(nullptr));
    }
    if (collect_queued(fe)) return 1;
    Ahead a;
    a.on = true; a.scan = next_scan; a.n = n; a.stride = stride_bytes;
    a.slot = (fe->ready.on && fe->ready.slot == 0) ? 1 : 0;
    const void* d_scan = next_scan;
    if (!on_device) {
        FE_HIP("voxel", fe->up_ahead[a.slot].reserve(n * stride_bytes));
        FE_HIP("voxel", hipMemcpy(fe->up_ahead[a.slot].p, next_scan, n * stride_bytes, hipMemcpyHostToDevice));
        d_scan = fe->up_ahead[a.slot].p;
    }
    FE_HIP("voxel", fe->out[a.slot].reserve(n * stride_bytes));
    if (pcr_voxel_filter_begin(fe->filt, d_scan, n, stride_bytes, fe->prm.grid_size, fe->out[a.slot].p, n)) return inner_fail(fe, "voxel", pcr_last_error(fe->filt));
    fe->queued = a;
    return 0;
}

int pcr_frontend_step(pcr_frontend* fe, const void* scan, size_t n, size_t stride_bytes, int on_device, const double init_pose[16],
                      double pose_out[16], pcr_frontend_info* info) {
    if (!fe) return 1;
    fe->err.clear();
    if (fe->failed) return ffail(fe, "an earlier step of this front end failed (" + fe->failure + "): pcr_frontend_reset starts over");
    if (check_scan(fe, scan, n, init_pose, pose_out)) return 1;
    pcr_frontend_info inf;
    memset(&inf, 0, sizeof inf);
    FE_HIP("voxel", hipSetDevice(fe->device));

    // 1. the voxel filter (LidarOdometry.cpp:170-171), or the one queued ahead for this very scan
    auto t0 = std::chrono::steady_clock::now();
    const void* d_filtered = nullptr;
    size_t n_filtered = 0;
    if (fe->queued.is(scan, n, stride_bytes) && collect_queued(fe)) return 1;
    if (fe->ready.is(scan, n, stride_bytes)) {
        fe->ready.on = false;
        d_filtered = fe->out[fe->ready.slot].p;
        n_filtered = fe->ready.count;
    } else {
        FE_HIP("voxel", fe->direct.reserve(n * stride_bytes));
        if (pcr_voxel_filter(fe->reg, scan, n, stride_bytes, on_device, fe->prm.grid_size, fe->direct.p, n, 1, &n_filtered))
            return inner_fail(fe, "voxel", pcr_last_error(fe->reg));
        d_filtered = fe->direct.p;
    }
    inf.n_filtered = (int64_t)n_filtered;
    inf.seconds[0] = seconds_since(t0);

    // 2. the sub-map this scan meets: an assembly the previous step queued is collected here
    t0 = std::chrono::steady_clock::now();
    if (collect_assembly(fe, "wait")) return 1;
    inf.n_submap = (int64_t)fe->n_submap;
    inf.seconds[1] = seconds_since(t0);
    if (fe->n_submap > 0) {      // (the map's point layout is its first key frame's)
        size_t n_dst = 0, map_stride = 0;
        (void)pcr_map_submap(fe->map, &n_dst, &map_stride);
        if (map_stride != stride_bytes) return ffail(fe, "the scan and the map's key frames must share one point layout (stride_bytes)");
    }

    // 3. scan2Map from the caller's initial pose (LidarOdometry.cpp:179-184)
    double pose[16];
    for (int i = 0; i < 16; ++i) pose[i] = init_pose[i];
    inf.converged = 1;
    if (fe->n_submap > 0) {
        t0 = std::chrono::steady_clock::now();
        int conv = 0;
        if (pcr_scan2map_submap(fe->reg, d_filtered, n_filtered, 1, fe->map, pose, &conv)) return inner_fail(fe, "scan2map", pcr_last_error(fe->reg));
        pcr_stats st;
        (void)pcr_get_stats(fe->reg, &st);
        inf.registered = 1; inf.converged = conv ? 1 : 0; inf.iterations = st.iterations;
        inf.seconds[2] = seconds_since(t0);
    }

    // 4. SixDof2Mobile (LidarOdometry.cpp:211): before setCurPose, before the key frame, before the pose is handed back
    if (fe->prm.mobile) (void)pcr_pose_to_mobile(pose, pose);

    // 5. setCurPose (MapManager.cpp:109-119)
    const double t[3] = {pose[12], pose[13], pose[14]};
    bool due = !fe->have_update;
    if (!due) {
        const double dx = fe->last_update[0] - t[0], dy = fe->last_update[1] - t[1], dz = fe->last_update[2] - t[2];
        due = sqrt((dx * dx + dy * dy) + dz * dz) > fe->prm.kf_gap;
    }

    // 6. putKeyFrame (MapManager.cpp:121-149): nearestKSearch's SQUARED distance against minKFGap itself (:141-143)
    bool add = fe->kf_pos.empty();
    int64_t nearest = -1;      // (recorded for pcr_frontend_closest; the rule reads `best` alone)
    if (!add) {
        double best = DBL_MAX;
        for (size_t i = 0; i + 2 < fe->kf_pos.size(); i += 3) {
            const double dx = fe->kf_pos[i] - t[0], dy = fe->kf_pos[i + 1] - t[1], dz = fe->kf_pos[i + 2] - t[2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < best) { best = d2; nearest = (int64_t)(i / 3); }
        }
        add = best > fe->prm.kf_gap;
    }
    if (add) {
        t0 = std::chrono::steady_clock::now();
        if (pcr_map_add_keyframe(fe->map, scan, n, stride_bytes, on_device, pose)) return inner_fail(fe, "add_keyframe", pcr_map_last_error(fe->map));
        fe->kf_pos.insert(fe->kf_pos.end(), {t[0], t[1], t[2]});
        fe->closest.push_back(nearest);
        inf.keyframe_added = 1;
        inf.seconds[3] = seconds_since(t0);
    }

    // 7. updateMap (MapManager.cpp:151-201), queued: the next step's wait -- or pcr_frontend_finish -- collects it
    if (due) {
        t0 = std::chrono::steady_clock::now();
        if (pcr_map_update_begin(fe->map, t, fe->prm.radius, fe->prm.grid_size)) return inner_fail(fe, "update_map", pcr_map_last_error(fe->map));
        fe->assembly_queued = true;
        fe->have_update = true;
        for (int i = 0; i < 3; ++i) fe->last_update[i] = t[i];
        fe->updates += 1;
        inf.update_queued = 1;
        inf.seconds[4] = seconds_since(t0);
    }
    inf.keyframes = (int64_t)(fe->kf_pos.size() / 3);
    inf.updates = fe->updates;
    for (int i = 0; i < 16; ++i) pose_out[i] = pose[i];
    if (info) *info = inf;
    return 0;
}

int pcr_frontend_step_timed(pcr_frontend* fe, const void* scan, size_t n, size_t stride_bytes, int on_device, const void* times, int time_kind,
                            long long time_offset_bytes, const pcr_deskew_motion* m, const double init_pose[16], double pose_out[16],
                            pcr_frontend_info* info, pcr_deskew_info* dinfo) {
    if (!fe) return 1;
    fe->err.clear();
    if (fe->failed) return ffail(fe, "an earlier step of this front end failed (" + fe->failure + "): pcr_frontend_reset starts over");
    if (check_scan(fe, scan, n, init_pose, pose_out)) return 1;
    if (stride_bytes < 16 || stride_bytes % 4 != 0) return ffail(fe, "deskew: stride_bytes must be a multiple of 4 and >= 16");
    if (n > SIZE_MAX / stride_bytes) return ffail(fe, "scan too large");
    FE_HIP("deskew", hipSetDevice(fe->device));
    // a filter queued ahead is of another scan (timed scans are not prefetched): collected and dropped
    if (collect_queued(fe)) return 1;
    fe->ready.on = false;
    FE_HIP("deskew", fe->deskewed.reserve(n * stride_bytes));
    // (a refusal writes nothing and the loop's state is as it was: no reset is needed after it)
    if (pcr_deskew(fe->reg, scan, n, stride_bytes, on_device, times, time_kind, time_offset_bytes, m, fe->deskewed.p, 1, dinfo))
        return ffail(fe, std::string("deskew: ") + pcr_last_error(fe->reg));
    return pcr_frontend_step(fe, fe->deskewed.p, n, stride_bytes, 1, init_pose, pose_out, info);
}

int pcr_frontend_finish(pcr_frontend* fe, size_t* n_submap) {
    if (!fe) return 1;
    fe->err.clear();
    if (n_submap) *n_submap = 0;
    if (collect_assembly(fe, "wait")) return 1;
    if (n_submap) *n_submap = fe->n_submap;
    return 0;
}

int pcr_frontend_closest(const pcr_frontend* fe, int64_t* idx, size_t capacity, size_t* n) {
    if (!fe) return 1;
    pcr_frontend* w = const_cast<pcr_frontend*>(fe);
    w->err.clear();
    if (n) *n = fe->closest.size();
    if (!idx) return 0;      // (the count alone, as pcr_map_submap_indices)
    if (capacity < fe->closest.size()) return ffail(w, "output capacity too small: " + std::to_string(fe->closest.size()) + " key frames were added");
    std::copy(fe->closest.begin(), fe->closest.end(), idx);
    return 0;
}

int pcr_frontend_reset(pcr_frontend* fe) {
    if (!fe) return 1;
    fe->err.clear();
    fe->failed = false;
    (void)hipSetDevice(fe->device);
    if (fe->queued.on) {      // a filter nobody took: collected and dropped
        size_t n = 0;
        fe->queued.on = false;
        (void)pcr_voxel_filter_end(fe->filt, &n);
    }
    fe->ready.on = false;
    fe->kf_pos.clear();
    fe->closest.clear();
    fe->have_update = false;
    fe->assembly_queued = false;
    fe->n_submap = 0;
    fe->updates = 0;
    if (pcr_map_clear(fe->map)) return ffail(fe, std::string("reset: ") + pcr_map_last_error(fe->map));
    return 0;
}

}  // extern "C"
