// session_host.hip -- a session to and from disk (pcr_tum_*, pcr_pcd_*, pcr_map_save / _load, pcr_backend_set_save_dir / _save / _load).  Host
// code only, and no kernel behind it that was not there: the reference's saveMapDir -- {i}.pcd (MapManager::saveKfs, frontend/src/MapManager.cpp:
// 203-213), tum.txt (utils::file::writeAsTum / loadFromTum, common/utils/File.hpp:49-95) and fg.g2o (Backend.cpp:198-222) -- written and read
// over entry points that exist: pcr_map_read_keyframe, pcr_map_add_keyframe, pcr_sc_add_keyframes, pcr_map_downsample_keyframes,
// pcr_graph_save_g2o / _load_g2o.  The PCD reader and writer are pcd_format.h's, shared with the C++ mirror.  DESIGN 4.19.

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "handle.h"
#include "backend_state.h"
#include "pcd_format.h"

using namespace pcr;

namespace {

thread_local std::string g_session_error;      // pcr_session_last_error
int sfail(const std::string& s) { g_session_error = s; return 1; }

double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// Eigen::Quaternion(R) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl): small_math.h's t2se3 without its normalisation; q = x y z w
void quat_of(const double* T, double q[4]) {
#define M_(i, j) T[(j) * 4 + (i)]
    double t = M_(0, 0) + M_(1, 1) + M_(2, 2);
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t; t = 0.5 / t;
        q[0] = (M_(2, 1) - M_(1, 2)) * t; q[1] = (M_(0, 2) - M_(2, 0)) * t; q[2] = (M_(1, 0) - M_(0, 1)) * t;
    } else {
        int i = 0;
        if (M_(1, 1) > M_(0, 0)) i = 1;
        if (M_(2, 2) > M_(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(M_(i, i) - M_(j, j) - M_(k, k) + 1.0);
        q[i] = 0.5 * t; t = 0.5 / t;
        q[3] = (M_(k, j) - M_(j, k)) * t;
        q[j] = (M_(j, i) + M_(i, j)) * t;
        q[k] = (M_(k, i) + M_(i, k)) * t;
    }
#undef M_
}

// one line of writeAsTum; nonzero with *err when the stamp or the pose is not finite
int tum_line(double stamp, const double* T, int precise, std::string* line, std::string* err) {
    bool finite = std::isfinite(stamp);
    for (int c = 0; c < 4; ++c) for (int r = 0; r < 3; ++r) finite = finite && std::isfinite(T[c * 4 + r]);
    if (!finite) { *err = "the stamp or the pose is not finite"; return 1; }
    double q[4];
    quat_of(T, q);
    char buf[512];
    const char* fmt = precise ? "%.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n" : "%.3f %.3f %.3f %.3f %.6f %.6f %.6f %.6f\n";
    const int len = snprintf(buf, sizeof buf, fmt, stamp, T[12], T[13], T[14], q[0], q[1], q[2], q[3]);
    if (len < 0 || (size_t)len >= sizeof buf) {      // (%.3f of 1e300 is 300 digits: a stamp or a translation that long is not a session's)
        *err = "the line would exceed " + std::to_string(sizeof buf - 1) + " characters";
        return 1;
    }
    line->assign(buf, (size_t)len);
    return 0;
}

bool blank(const char* s) {
    for (; *s; ++s) if (!isspace((unsigned char)*s)) return false;
    return true;
}

// the eight numbers of a line -> how many could be read
int tum_numbers(const char* line, double v[8]) {
    const char* p = line;
    int k = 0;
    for (; k < 8; ++k) {
        char* end = nullptr;
        v[k] = strtod(p, &end);
        if (end == p) break;
        p = end;
    }
    return k;
}

// identity . translate(t) . rotate(q): Eigen's toRotationMatrix (Quaternion.h) of q as read
void tum_pose(const double v[8], double* T) {
    const double x = v[4], y = v[5], z = v[6], w = v[7];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
#define M_(i, j) T[(j) * 4 + (i)]
    M_(0, 0) = 1 - (tyy + tzz); M_(0, 1) = txy - twz; M_(0, 2) = txz + twy;
    M_(1, 0) = txy + twz; M_(1, 1) = 1 - (txx + tzz); M_(1, 2) = tyz - twx;
    M_(2, 0) = txz - twy; M_(2, 1) = tyz + twx; M_(2, 2) = 1 - (txx + tyy);
    M_(3, 0) = 0; M_(3, 1) = 0; M_(3, 2) = 0; M_(3, 3) = 1;
    M_(0, 3) = v[1]; M_(1, 3) = v[2]; M_(2, 3) = v[3];
#undef M_
}

std::string quoted(const char* line) {
    std::string s(line);
    while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
    if (s.size() > 120) s = s.substr(0, 120) + "...";
    return "\"" + s + "\"";
}

int parse_line(const char* line, double* stamp, double* pose16, std::string* err) {
    if (blank(line)) return PCR_TUM_SKIP;
    double v[8];
    const int k = tum_numbers(line, v);
    if (k < 8) {
        *err = "a line holds 8 numbers (stamp, t.x t.y t.z, q.x q.y q.z q.w); this one holds " + std::to_string(k) + ": " + quoted(line);
        return PCR_TUM_ERROR;
    }
    if (stamp) *stamp = v[0];
    tum_pose(v, pose16);
    return PCR_TUM_OK;
}

// where the intensity of a point of `stride` bytes lies (float index; 0: it has none): pcr_hip.h's rule for the voxel filter
size_t intensity_at(size_t stride) { return stride >= 20 ? 4 : stride == 16 ? 3 : 0; }
bool stride_ok(size_t stride) { return stride >= 12 && stride % 4 == 0; }

int write_pcd(const std::string& path, const void* pts, size_t n, size_t stride) {
    const size_t ii = intensity_at(stride);
    const char* base = static_cast<const char*>(pts);
    return pcd::write(path, n, [&](size_t p, float r[4]) {
        const char* row = base + p * stride;
        memcpy(r, row, 12);
        if (ii) memcpy(r + 3, row + 4 * ii, 4); else r[3] = 0.f;
    });
}

struct XyziSink {      // pcd::read into packed x y z intensity rows
    std::vector<float>& v;
    void resize(size_t n) { v.assign(4 * n, 0.f); }
    void set(size_t p, int k, float x) { v[4 * p + (size_t)k] = x; }
};

// 0, or 1 with *err (which names the path)
int read_pcd(const std::string& path, std::vector<float>& xyzi, std::string* err) {
    try {
        XyziSink sink{xyzi};
        if (pcd::read(path, sink) == -1) { *err = "cannot open " + path; return 1; }
    } catch (const std::exception& e) {
        const std::string what = e.what();
        *err = what.find(path) == std::string::npos ? path + ": " + what : what;
        return 1;
    }
    return 0;
}

// packed x y z intensity rows into points of `stride` bytes
void expand_rows(const float* xyzi, size_t n, size_t stride, void* out) {
    const size_t ii = intensity_at(stride);
    char* base = static_cast<char*>(out);
    for (size_t p = 0; p < n; ++p) {
        char* row = base + p * stride;
        memset(row, 0, stride);
        memcpy(row, xyzi + 4 * p, 12);
        if (ii == 4) { const float one = 1.f; memcpy(row + 12, &one, 4); }
        if (ii) memcpy(row + 4 * ii, xyzi + 4 * p + 3, 4);
    }
}

int write_tum(const pcr_map* m, const std::string& dir, size_t n, const double* stamps, int precise, std::string* err) {
    const std::string path = dir + "/tum.txt";
    std::string text, line;
    for (size_t i = 0; i < n; ++i) {
        double pose[16];
        size_t np = 0;
        (void)pcr_map_keyframe(m, i, &np, nullptr, pose);
        std::string why;
        if (tum_line(stamps ? stamps[i] : (double)i, pose, precise, &line, &why)) { *err = path + ": key frame " + std::to_string(i) + ": " + why; return 1; }
        text += line;
    }
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { *err = "cannot write " + path; return 1; }
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if (fclose(f) != 0 || !ok) { *err = "cannot write " + path; return 1; }
    return 0;
}

struct Session {
    std::vector<double> stamps, poses;           // per key frame: stamp, 16 doubles column-major
    std::vector<std::vector<float>> clouds;      // x y z intensity
};

// tum.txt and every {i}.pcd into host memory; *have_tum = false (and 0) when there is no tum.txt
int read_session(const std::string& dir, Session* s, bool* have_tum, std::string* err) {
    const std::string tum = dir + "/tum.txt";
    std::ifstream f(tum);
    *have_tum = (bool)f;
    if (!f) return 0;
    std::string line;
    for (size_t no = 1; std::getline(f, line); ++no) {
        double stamp = 0, pose[16];
        std::string why;
        const int rc = parse_line(line.c_str(), &stamp, pose, &why);
        if (rc == PCR_TUM_SKIP) continue;
        if (rc != PCR_TUM_OK) { *err = tum + " line " + std::to_string(no) + ": " + why; return 1; }
        s->stamps.push_back(stamp);
        s->poses.insert(s->poses.end(), pose, pose + 16);
    }
    s->clouds.resize(s->stamps.size());
    for (size_t i = 0; i < s->clouds.size(); ++i)
        if (read_pcd(dir + "/" + std::to_string(i) + ".pcd", s->clouds[i], err)) return 1;
    return 0;
}

// the key frames into an empty store, in its point layout; on a failure the store is emptied again
int upload_session(pcr_map* m, const Session& s, std::string* err) {
    size_t stride = 0;
    (void)pcr_map_keyframe(m, 0, nullptr, &stride, nullptr);      // (the layout of a store that held key frames before; 0: it never did)
    if (stride == 0) stride = 16;
    std::vector<char> rows;
    for (size_t i = 0; i < s.clouds.size(); ++i) {
        const size_t n = s.clouds[i].size() / 4;
        rows.resize(n * stride);
        expand_rows(s.clouds[i].data(), n, stride, rows.data());
        if (pcr_map_add_keyframe(m, n ? rows.data() : nullptr, n, stride, 0, &s.poses[16 * i])) {
            *err = std::string("key frame ") + std::to_string(i) + ": " + pcr_map_last_error(m);
            (void)pcr_map_clear(m);
            return 1;
        }
    }
    return 0;
}

void stamps_out(const Session& s, double* stamps, size_t capacity, size_t* n_loaded) {
    if (stamps) for (size_t i = 0; i < std::min(capacity, s.stamps.size()); ++i) stamps[i] = s.stamps[i];
    if (n_loaded) *n_loaded = s.stamps.size();
}

int befail(pcr_backend* be, const std::string& msg) { be->err = msg; return 1; }
int be_inner_fail(pcr_backend* be, const char* step, const std::string& msg) {
    be->failed = true;
    be->failure = std::string(step) + ": " + (msg.empty() ? "failed" : msg);
    return befail(be, be->failure);
}

}  // namespace

namespace pcr {

int session_write_keyframes(const pcr_map* m, const std::string& dir, size_t first, std::string* err) {
    size_t n_kf = 0;
    if (pcr_map_keyframes(m, &n_kf)) { *err = pcr_map_last_error(m); return 1; }
    if (first > n_kf) { *err = "first exceeds the number of key frames"; return 1; }
    std::vector<char> host;
    for (size_t i = first; i < n_kf; ++i) {
        size_t n = 0, stride = 0;
        (void)pcr_map_keyframe(m, i, &n, &stride, nullptr);
        host.resize(n * stride);
        if (pcr_map_read_keyframe(m, i, host.data(), n, &n, nullptr)) { *err = std::string("key frame ") + std::to_string(i) + ": " + pcr_map_last_error(m); return 1; }
        const std::string path = dir + "/" + std::to_string(i) + ".pcd";
        if (write_pcd(path, host.data(), n, stride ? stride : 16)) { *err = "cannot write " + path; return 1; }
    }
    return 0;
}

}  // namespace pcr

extern "C" {

const char* pcr_session_last_error(void) { return g_session_error.c_str(); }

int pcr_tum_format(double stamp, const double pose16[16], int precise, char* buf, size_t capacity) {
    g_session_error.clear();
    if (!pose16 || !buf) return sfail("pcr_tum_format: NULL argument");
    std::string line, why;
    if (tum_line(stamp, pose16, precise, &line, &why)) return sfail("pcr_tum_format: " + why);
    if (capacity < line.size() + 1) return sfail("pcr_tum_format: the line takes " + std::to_string(line.size() + 1) + " bytes with its NUL, capacity is " + std::to_string(capacity));
    memcpy(buf, line.c_str(), line.size() + 1);
    return 0;
}

int pcr_tum_parse(const char* line, double* stamp, double pose16[16]) {
    g_session_error.clear();
    if (!line || !pose16) { sfail("pcr_tum_parse: NULL argument"); return PCR_TUM_ERROR; }
    std::string why;
    const int rc = parse_line(line, stamp, pose16, &why);
    if (rc == PCR_TUM_ERROR) sfail("pcr_tum_parse: " + why);
    return rc;
}

int pcr_pcd_write(const char* path, const void* pts, size_t n, size_t stride_bytes) {
    g_session_error.clear();
    if (!path) return sfail("pcr_pcd_write: NULL path");
    if (n && !pts) return sfail("pcr_pcd_write: NULL cloud with nonzero size");
    if (!stride_ok(stride_bytes)) return sfail("pcr_pcd_write: stride_bytes must be a multiple of 4 and >= 12");
    if (write_pcd(path, pts, n, stride_bytes)) return sfail(std::string("pcr_pcd_write: cannot write ") + path);
    return 0;
}

int pcr_pcd_read(const char* path, void* out, size_t capacity_points, size_t stride_bytes, size_t* n) {
    g_session_error.clear();
    if (n) *n = 0;
    if (!path) return sfail("pcr_pcd_read: NULL path");
    if (!stride_ok(stride_bytes)) return sfail("pcr_pcd_read: stride_bytes must be a multiple of 4 and >= 12");
    std::vector<float> xyzi;
    std::string why;
    if (read_pcd(path, xyzi, &why)) return sfail("pcr_pcd_read: " + why);
    const size_t count = xyzi.size() / 4;
    if (n) *n = count;
    if (!out && capacity_points == 0) return 0;
    if (capacity_points < count) return sfail("pcr_pcd_read: output capacity too small: " + std::string(path) + " holds " + std::to_string(count) + " points");
    if (count && !out) return sfail("pcr_pcd_read: NULL output");
    expand_rows(xyzi.data(), count, stride_bytes, out);
    return 0;
}

int pcr_map_save(const pcr_map* m, const char* dir, size_t first, const double* stamps, int precise) {
    if (!m) return 1;
    if (!dir || !*dir) return map_set_error(m, "pcr_map_save: no directory");
    if (pcr_map_wait(const_cast<pcr_map*>(m), nullptr)) return 1;      // a queued assembly is collected first (its own message stands)
    size_t n_kf = 0;
    if (pcr_map_keyframes(m, &n_kf)) return 1;
    if (first > n_kf) return map_set_error(m, "pcr_map_save: first exceeds the number of key frames");
    std::string why;
    if (session_write_keyframes(m, dir, first, &why)) return map_set_error(m, "pcr_map_save: " + why);
    if (write_tum(m, dir, n_kf, stamps, precise, &why)) return map_set_error(m, "pcr_map_save: " + why);
    map_set_error(m, "");
    return 0;
}

int pcr_map_load(pcr_map* m, const char* dir, double grid_size, double* stamps, size_t capacity, size_t* n_loaded) {
    if (!m) return 1;
    if (n_loaded) *n_loaded = 0;
    if (!dir || !*dir) return map_set_error(m, "pcr_map_load: no directory");
    size_t n_kf = 0;
    if (pcr_map_keyframes(m, &n_kf)) return 1;
    if (n_kf) return map_set_error(m, "pcr_map_load: the store holds " + std::to_string(n_kf) + " key frames; a session loads into a store without key frames (pcr_map_clear)");
    Session s;
    bool have_tum = false;
    std::string why;
    if (read_session(dir, &s, &have_tum, &why)) return map_set_error(m, "pcr_map_load: " + why);
    if (!have_tum) { map_set_error(m, ""); return 0; }      // (the reference warns and starts fresh, MapManager.cpp:35-38)
    if (upload_session(m, s, &why)) return map_set_error(m, "pcr_map_load: " + why);
    if (grid_size > 0 && pcr_map_downsample_keyframes(m, 0, grid_size, nullptr)) {
        why = pcr_map_last_error(m);
        (void)pcr_map_clear(m);
        return map_set_error(m, "pcr_map_load: " + why);
    }
    stamps_out(s, stamps, capacity, n_loaded);
    map_set_error(m, "");
    return 0;
}

int pcr_backend_set_save_dir(pcr_backend* be, const char* dir) {
    if (!be) return 1;
    be->err.clear();
    be->save_dir = dir ? dir : "";
    return 0;
}

int pcr_backend_save(pcr_backend* be, const double* stamps, int precise) {
    if (!be) return 1;
    be->err.clear();
    if (be->save_dir.empty()) return befail(be, "pcr_backend_save: no save directory is set (pcr_backend_set_save_dir)");
    size_t n_kf = 0;
    if (pcr_map_keyframes(be->map, &n_kf)) return befail(be, std::string("pcr_backend_save: ") + pcr_map_last_error(be->map));
    std::string why;
    if (write_tum(be->map, be->save_dir, n_kf, stamps, precise, &why)) return befail(be, "pcr_backend_save: " + why);
    const std::string g2o = be->save_dir + "/fg.g2o";
    if (pcr_graph_save_g2o(be->graph, g2o.c_str())) return befail(be, std::string("pcr_backend_save: ") + pcr_graph_last_error(be->graph));
    return 0;
}

int pcr_backend_load(pcr_backend* be, const char* dir, double* stamps, size_t capacity, pcr_backend_info* info) {
    if (!be) return 1;
    be->err.clear();
    if (be->failed) return befail(be, "an earlier event of this back end failed (" + be->failure + "): pcr_backend_reset starts over");
    if (!dir || !*dir) return befail(be, "pcr_backend_load: no directory");
    // everything that can be refused is refused here, before the store, the contexts or the graph change
    size_t n_kf = 0, n_ctx = 0, g_poses = 0, g_priors = 0, g_between = 0;
    if (pcr_map_keyframes(be->map, &n_kf)) return befail(be, std::string("pcr_backend_load: ") + pcr_map_last_error(be->map));
    (void)pcr_sc_size(be->sc, &n_ctx);
    (void)pcr_graph_size(be->graph, &g_poses, &g_priors, &g_between);
    if (n_kf || n_ctx || g_poses || g_priors || g_between || be->done || be->lc_done)
        return befail(be, "pcr_backend_load: a session loads into a freshly created or reset back end over an empty store (this one holds " + std::to_string(n_kf) +
                              " key frames, " + std::to_string(n_ctx) + " contexts, " + std::to_string(g_poses) + " graph poses)");
    const std::string g2o = std::string(dir) + "/fg.g2o";
    if (FILE* f = fopen(g2o.c_str(), "rb")) fclose(f);
    else return befail(be, "pcr_backend_load: cannot open " + g2o + ": without the graph the first component has no prior; pcr_map_load loads a map alone");
    auto t0 = std::chrono::steady_clock::now();
    Session s;
    bool have_tum = false;
    std::string why;
    if (read_session(dir, &s, &have_tum, &why)) return befail(be, "pcr_backend_load: " + why);
    if (!have_tum) return befail(be, std::string("pcr_backend_load: cannot open ") + dir + "/tum.txt");
    const size_t n = s.stamps.size();
    {   // the graph file, read once into a host graph: does it load, and does it hold one vertex per key frame?
        pcr_graph* probe = pcr_graph_create(PCR_GRAPH_HOST);
        if (!probe) return befail(be, std::string("pcr_backend_load: ") + pcr_graph_last_error(nullptr));
        size_t vertices = 0;
        const int rc = pcr_graph_load_g2o(probe, g2o.c_str());
        if (rc) why = pcr_graph_last_error(probe);
        else (void)pcr_graph_size(probe, &vertices, nullptr, nullptr);
        pcr_graph_destroy(probe);
        if (rc) return befail(be, "pcr_backend_load: " + why);
        if (vertices != n)
            return befail(be, "pcr_backend_load: " + g2o + " holds " + std::to_string(vertices) + " vertices, " + dir + "/tum.txt " + std::to_string(n) + " key frames");
    }
    double sec[5] = {seconds_since(t0), 0, 0, 0, 0};
    // 1. the raw key frames
    t0 = std::chrono::steady_clock::now();
    if (upload_session(be->map, s, &why)) return be_inner_fail(be, "load", why);
    sec[1] = seconds_since(t0);
    auto give_up = [&](const char* step, const char* msg) {
        const std::string keep = msg ? msg : "";
        (void)pcr_map_clear(be->map);
        return be_inner_fail(be, step, keep);
    };
    // 2. their contexts, from the raw clouds
    t0 = std::chrono::steady_clock::now();
    if (pcr_sc_add_keyframes(be->sc, be->map, 0, n, be->prm.context_grid_size, nullptr)) return give_up("contexts", pcr_sc_last_error(be->sc));
    sec[2] = seconds_since(t0);
    // 3. saveKfs' filter, as the loading constructor applies it (MapManager.cpp:46)
    t0 = std::chrono::steady_clock::now();
    if (be->prm.grid_size > 0 && pcr_map_downsample_keyframes(be->map, 0, be->prm.grid_size, nullptr)) return give_up("downsample", pcr_map_last_error(be->map));
    sec[3] = seconds_since(t0);
    // 4. the graph
    t0 = std::chrono::steady_clock::now();
    if (pcr_graph_load_g2o(be->graph, g2o.c_str())) return give_up("factors", pcr_graph_last_error(be->graph));
    sec[4] = seconds_since(t0);
    be->done = n;
    be->lc_done = n;
    be->loops.clear();
    for (int i = 0; i < 5; ++i) be->load_seconds[i] = sec[i];
    stamps_out(s, stamps, capacity, nullptr);
    if (info) {
        memset(info, 0, sizeof *info);
        for (int i = 0; i < 16; ++i) info->delta[i] = info->graph.delta[i] = (i % 5 == 0) ? 1.0 : 0.0;
        info->keyframes = info->contexts = (int64_t)n;
        info->keyframes_added = (int32_t)n;
        info->seconds[0] = sec[2]; info->seconds[1] = sec[3]; info->seconds[2] = sec[4];
    }
    return 0;
}

int pcr_backend_load_seconds(const pcr_backend* be, double seconds[5]) {
    if (!be || !seconds) return 1;
    for (int i = 0; i < 5; ++i) seconds[i] = be->load_seconds[i];
    return 0;
}

}  // extern "C"
