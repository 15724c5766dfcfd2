// graph_store.h -- the host side of a pose graph that touches no device: the poses and factor lists with their one revision
// counter, the checks every use of the graph starts with, the arrays the device reads (pack) and the g2o reader and writer.  Plain C++17, no
// HIP header: graph_host.hip serves the C ABI from it, host/graph_host_check.cpp runs it alone (and under a host sanitiser).
// Every function that can refuse returns its message; an empty string means fine.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <fstream>
#include <numeric>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pcr_hip.h"

namespace pcr {
namespace graph {

struct Factor {
    long long from;      // -1: a prior
    long long to;
    double z[16];
    double info[36];     // full symmetric, row-major
    unsigned char flags = 0;      // kMarkRobust, kMarkOff (between factors only): nothing a g2o file carries
};
constexpr unsigned char kMarkRobust = 1, kMarkOff = 2;      // the bits of graph_dev.h's Factors::flags (graph_host.hip asserts it)
// ... and the two pack() adds for the device, from the poses' fixed flags: the factor's "from" end, its "to" end is a fixed pose
constexpr unsigned char kPackFromFixed = 4, kPackToFixed = 8;

// Poses and factors each: the device indexes entry k of factor e at [k * F + e] with k < 36 (and [p * 51 + k] per pose) in 32-bit ints, and the
// host rounds buffer sizes up by 256 bytes.
constexpr size_t kMaxCount = 0x7fffff00u / 36;

struct Store {
    std::vector<double> poses;               // 16 per pose, column-major
    std::vector<Factor> priors, betweens;
    std::vector<unsigned char> fixed;        // per pose: 1 when the pose is a constant of the problem (set_fixed); as long as the poses are many
    int robust_kind = PCR_GRAPH_ROBUST_NONE; // the kernel of the marked between factors; it outlives clear()
    double robust_delta = 0.0;
    // THE staleness rule: every mutator ends in touch().  `revision` counts every change, `structure` is the revision of the last one that
    // added or cleared poses or factors or set a mark, a switch or a pose's fixed flag.  Whoever keeps something derived (the device's factor tables and CSR, the
    // forest, its schedule on the device, a converged optimisation) remembers the number it was made at and compares.
    uint64_t revision = 1, structure = 1;
    void touch(bool structural) { ++revision; if (structural) structure = revision; }

    size_t n_poses() const { return poses.size() / 16; }
    size_t n_factors() const { return priors.size() + betweens.size(); }
    bool is_fixed(size_t p) const { return p < fixed.size() && fixed[p] != 0; }
    size_t n_fixed() const { size_t n = 0; for (unsigned char f : fixed) n += f ? 1 : 0; return n; }
    const Factor& factor(size_t e) const { return e < priors.size() ? priors[e] : betweens[e - priors.size()]; }      // priors first
};

inline void expand_info(const double info21[21], double full[36]) {
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { full[i * 6 + j] = info21[k]; full[j * 6 + i] = info21[k]; ++k; }
}

// Backend.cpp:90-97: diagonal VARIANCES, [rotation; translation]; false for an unknown kind
inline bool noise_preset(int kind, double info21[21]) {
    static const double kVar[3][6] = {{1e-2, 1e-2, M_PI / 72, 1e-1, 1e-1, 1e-1}, {1e-4, 1e-4, 1e-4, 1e-1, 1e-1, 1e-1}, {1e-1, 1e-1, 1e-1, 1e-1, 1e-1, 1e-1}};
    static_assert(PCR_GRAPH_PRIOR == 0 && PCR_GRAPH_ODOM == 1 && PCR_GRAPH_LOOP == 2, "kVar is indexed by the kind");
    if (kind < PCR_GRAPH_PRIOR || kind > PCR_GRAPH_LOOP) return false;
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) info21[k++] = (i == j) ? 1.0 / kVar[kind][i] : 0.0;
    return true;
}

inline bool all_finite(const double* v, int n) {
    for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

// ---- the mutators ------------------------------------------------------------------------------------------------------------------------

inline std::string add_poses(Store& s, const char* what, const double* poses16, size_t count) {
    if (count == 0) return "";
    if (!poses16) return std::string(what) + ": NULL poses";
    if (s.n_poses() + count > kMaxCount) return std::string(what) + ": more poses than the device's 32-bit indices address";
    s.poses.insert(s.poses.end(), poses16, poses16 + 16 * count);
    s.fixed.resize(s.n_poses(), 0);      // a new pose is free
    s.touch(true);      // (the CSR has a row per pose)
    return "";
}

inline std::string add_factor(Store& s, const char* what, long long from, size_t to, const double z[16], const double info21[21], unsigned char flags = 0) {
    if (!z || !info21) return std::string(what) + ": NULL pose or information matrix";
    if (s.n_factors() + 1 > kMaxCount) return std::string(what) + ": more factors than the device's 32-bit indices address";
    Factor f;
    f.from = from; f.to = (long long)to; f.flags = flags;
    memcpy(f.z, z, sizeof f.z);
    expand_info(info21, f.info);
    (from < 0 ? s.priors : s.betweens).push_back(f);
    s.touch(true);
    return "";
}

inline std::string set_between_flag(Store& s, const char* what, size_t first, size_t count, unsigned char bit, bool set) {
    const size_t B = s.betweens.size();
    if (first > B || count > B - first) return std::string(what) + ": first + count exceeds the number of between factors (" + std::to_string(B) + ")";
    if (count == 0) return "";
    for (size_t e = first; e < first + count; ++e) s.betweens[e].flags = set ? (s.betweens[e].flags | bit) : (s.betweens[e].flags & (unsigned char)~bit);
    s.touch(true);      // as after an add
    return "";
}

// The fixed flag of poses first .. first + count - 1: a fixed pose is a constant of the problem ("Fixed poses").  The checks in
// their order: the range, then nothing to do.
inline std::string set_fixed(Store& s, const char* what, size_t first, size_t count, bool on) {
    const size_t N = s.n_poses();
    if (first > N || count > N - first) return std::string(what) + ": first + count exceeds the number of poses (" + std::to_string(N) + ")";
    if (count == 0) return "";
    s.fixed.resize(N, 0);
    for (size_t p = first; p < first + count; ++p) s.fixed[p] = on ? 1 : 0;
    s.touch(true);      // the factor tables carry the flags of their ends, the forest's roots follow them
    return "";
}

inline std::string set_robust_kernel(Store& s, const char* what, int kind, double delta) {
    if (kind < PCR_GRAPH_ROBUST_NONE || kind > PCR_GRAPH_ROBUST_TUKEY)
        return std::string(what) + ": unknown kind " + std::to_string(kind) +
               " (PCR_GRAPH_ROBUST_NONE = 0, PCR_GRAPH_ROBUST_HUBER = 1, PCR_GRAPH_ROBUST_GEMAN_MCCLURE = 2, PCR_GRAPH_ROBUST_TUKEY = 3)";
    if (kind != PCR_GRAPH_ROBUST_NONE && !(std::isfinite(delta) && delta > 0.0)) return std::string(what) + ": delta must be finite and greater than 0";
    s.robust_kind = kind;
    s.robust_delta = kind == PCR_GRAPH_ROBUST_NONE ? 0.0 : delta;
    s.touch(false);      // (the kernel and delta travel with every launch: no table is older for it)
    return "";
}

inline void clear(Store& s) {
    s.poses.clear(); s.priors.clear(); s.betweens.clear(); s.fixed.clear();
    s.touch(true);
}

// ---- the checks --------------------------------------------------------------------------------------------------------------------------

// Every refusal of pcr_graph_optimize (and of linearize / apply / tree / ..., which need the same graph), in this order: ids, from == to,
// numbers.  Poses below `first_pose` are not looked at: they are the device's, which came out of an optimisation of finite numbers, and a step
// that is not finite is never accepted (graph_opt.h: lm_step, and the NaN and inf cases of graph_host_check).
inline std::string check(const Store& s, const char* what, size_t first_pose = 0) {
    const size_t N = s.n_poses();
    const std::string w = std::string(what) + ": ";
    for (size_t i = 0; i < s.priors.size(); ++i)
        if (s.priors[i].to < 0 || (size_t)s.priors[i].to >= N)
            return w + "prior " + std::to_string(i) + ": id " + std::to_string(s.priors[i].to) + " out of range (the graph holds " + std::to_string(N) + " poses)";
    for (size_t i = 0; i < s.betweens.size(); ++i) {
        const Factor& f = s.betweens[i];
        for (long long id : {f.from, f.to})
            if (id < 0 || (size_t)id >= N)
                return w + "between factor " + std::to_string(i) + ": id " + std::to_string(id) + " out of range (the graph holds " + std::to_string(N) + " poses)";
        if (f.from == f.to) return w + "between factor " + std::to_string(i) + ": from == to (" + std::to_string(f.to) + ")";
    }
    for (size_t p = first_pose; p < N; ++p)
        if (!all_finite(&s.poses[16 * p], 16)) return w + "pose " + std::to_string(p) + " is not finite";
    for (size_t i = 0; i < s.priors.size(); ++i) {
        if (!all_finite(s.priors[i].z, 16)) return w + "prior " + std::to_string(i) + ": the pose is not finite";
        if (!all_finite(s.priors[i].info, 36)) return w + "prior " + std::to_string(i) + ": the information matrix is not finite";
    }
    for (size_t i = 0; i < s.betweens.size(); ++i) {
        if (!all_finite(s.betweens[i].z, 16)) return w + "between factor " + std::to_string(i) + ": the pose is not finite";
        if (!all_finite(s.betweens[i].info, 36)) return w + "between factor " + std::to_string(i) + ": the information matrix is not finite";
    }
    return "";
}

// union-find over the between factors that are switched on: the first pose whose connected component holds no anchor -- neither a prior nor
// a fixed pose -- or -1.  ONLY after check().
inline long long first_pose_without_prior(const Store& s) {
    const size_t N = s.n_poses();
    std::vector<size_t> parent(N);
    std::iota(parent.begin(), parent.end(), (size_t)0);
    auto find = [&](size_t a) { while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; } return a; };
    for (const Factor& f : s.betweens) {
        if (f.flags & kMarkOff) continue;
        const size_t a = find((size_t)f.from), b = find((size_t)f.to);
        if (a != b) parent[a > b ? a : b] = a > b ? b : a;
    }
    std::vector<char> has(N, 0);
    for (const Factor& f : s.priors) has[find((size_t)f.to)] = 1;
    for (size_t p = 0; p < N; ++p) if (s.is_fixed(p)) has[find(p)] = 1;
    for (size_t p = 0; p < N; ++p) if (!has[find(p)]) return (long long)p;
    return -1;
}

// ... as the refusal of whoever solves with the graph (optimize, tree, precondition).  ONLY after check().
inline std::string check_priors(const Store& s, const char* what) {
    const long long lone = first_pose_without_prior(s);
    if (lone < 0) return "";
    return std::string(what) + ": pose " + std::to_string(lone) + " lies in a connected component without a prior: the system would be singular";
}

// Is there anything to optimise: a factor that is switched on with a free pose at one of its ends.  (After check_priors() every free pose has
// one, so this is false exactly when every pose is fixed -- or the graph holds none.)  ONLY after check().
inline bool has_free_pose_with_factor(const Store& s) {
    for (const Factor& f : s.priors) if (!s.is_fixed((size_t)f.to)) return true;
    for (const Factor& f : s.betweens) {
        if (f.flags & kMarkOff) continue;
        if (!s.is_fixed((size_t)f.from) || !s.is_fixed((size_t)f.to)) return true;
    }
    return false;
}

// ---- what the device reads ---------------------------------------------------------------------------------------------------------------

// Factors in the order priors, betweens, structure-of-arrays (entry k of factor e at [k * F + e]), and the CSR of every pose's incident factors:
// ent[row_ptr[p] .. row_ptr[p + 1]), ascending by factor, entry = factor * 2 + (1: p is the "to" end).  flags holds F + 1 entries and ent at least
// one, so that no upload is of nothing.  A factor's flags carry kPackFromFixed / kPackToFixed when that end is a fixed pose (a prior has no
// "from" end); pose_fixed holds N + 1 entries, any_fixed says whether one of them is set.  ONLY after check(): the CSR is indexed by the factors' ids, and a wrong row here is a fault on the device.
struct Packed {
    std::vector<int> from, to, row_ptr, ent;
    std::vector<unsigned char> flags, pose_fixed;
    bool any_fixed = false;
    std::vector<double> z, omega;
};
inline Packed pack(const Store& s) {
    const size_t N = s.n_poses(), F = s.n_factors();
    Packed k;
    k.from.resize(F); k.to.resize(F);
    k.z.resize(16 * F); k.omega.resize(36 * F);
    k.flags.assign(F + 1, 0);
    k.row_ptr.assign(N + 1, 0);
    k.pose_fixed.assign(N + 1, 0);
    for (size_t p = 0; p < N; ++p) if (s.is_fixed(p)) { k.pose_fixed[p] = 1; k.any_fixed = true; }
    for (size_t e = 0; e < F; ++e) {
        const Factor& f = s.factor(e);
        k.from[e] = (int)f.from; k.to[e] = (int)f.to;
        k.flags[e] = (unsigned char)(f.flags | (f.from >= 0 && k.pose_fixed[f.from] ? kPackFromFixed : 0) | (k.pose_fixed[f.to] ? kPackToFixed : 0));
        for (int i = 0; i < 16; ++i) k.z[i * F + e] = f.z[i];
        for (int i = 0; i < 36; ++i) k.omega[i * F + e] = f.info[i];
        if (f.from >= 0) k.row_ptr[f.from + 1]++;
        k.row_ptr[f.to + 1]++;
    }
    for (size_t p = 0; p < N; ++p) k.row_ptr[p + 1] += k.row_ptr[p];
    k.ent.assign(k.row_ptr[N] > 0 ? k.row_ptr[N] : 1, 0);
    std::vector<int> fill(k.row_ptr.begin(), k.row_ptr.end() - 1);
    for (size_t e = 0; e < F; ++e) {      // ascending factor id within every row
        if (k.from[e] >= 0) k.ent[fill[k.from[e]]++] = (int)(e * 2);
        k.ent[fill[k.to[e]]++] = (int)(e * 2 + 1);
    }
    return k;
}

// ---- g2o ---------------------------------------------------------------------------------------------------------------------------------

// quaternion (x, y, z, w) of a rotation, Eigen's Quaternion(Matrix3) (the trace branch, or the branch of the largest diagonal element)
inline void rot_to_quat(const double* T, double q[4]) {
    auto M = [T](int i, int j) { return T[j * 4 + i]; };
    double t = M(0, 0) + M(1, 1) + M(2, 2);
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t; t = 0.5 / t;
        q[0] = (M(2, 1) - M(1, 2)) * t; q[1] = (M(0, 2) - M(2, 0)) * t; q[2] = (M(1, 0) - M(0, 1)) * t;
    } else {
        int i = 0;
        if (M(1, 1) > M(0, 0)) i = 1;
        if (M(2, 2) > M(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(M(i, i) - M(j, j) - M(k, k) + 1.0);
        q[i] = 0.5 * t; t = 0.5 / t;
        q[3] = (M(k, j) - M(j, k)) * t;
        q[j] = (M(j, i) + M(i, j)) * t;
        q[k] = (M(k, i) + M(i, k)) * t;
    }
}

// Rot3::quaternion(w, x, y, z) + Point3: Eigen's Quaternion::toRotationMatrix, the quaternion taken as it stands (not normalised)
inline void quat_to_pose(const double q[4], const double t[3], double* T) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[j * 4 + i] = R[i * 3 + j];
        T[12 + i] = t[i];
        T[i * 4 + 3] = 0.0;
    }
    T[15] = 1.0;
}

// Appends the file's vertices and edges.  Everything is read into temporaries first: a file that is refused leaves the store as it was.
inline std::string load_g2o(Store& s, const char* what, const char* path) {
    if (!path) return std::string(what) + ": NULL path";
    std::ifstream in(path);
    if (!in.is_open()) return std::string(what) + ": cannot open " + path;
    std::vector<double> poses;
    std::vector<Factor> priors, betweens;
    std::vector<std::pair<long long, std::string>> fix;      // FIX records: the id and where it stood
    const size_t N0 = s.n_poses();
    std::string line;
    size_t lineno = 0;
    while (std::getline(in, line)) {
        ++lineno;
        std::istringstream ss(line);
        std::string tag;
        ss >> tag;
        const std::string at = std::string(what) + ": " + path + ":" + std::to_string(lineno) + ": ";
        if (tag == "VERTEX3" || tag == "EDGE3")
            return at + tag + " records (Euler angles) are not read: write the graph with VERTEX_SE3:QUAT and EDGE_SE3:QUAT";
        if (tag == "VERTEX_SE3:QUAT") {
            long long id; double t[3], q[4];
            if (!(ss >> id >> t[0] >> t[1] >> t[2] >> q[0] >> q[1] >> q[2] >> q[3])) return at + "malformed VERTEX_SE3:QUAT";
            if (id != (long long)(N0 + poses.size() / 16))
                return at + "vertex id " + std::to_string(id) + " where " + std::to_string(N0 + poses.size() / 16) + " is next: ids are consecutive from 0";
            double T[16];
            quat_to_pose(q, t, T);
            if (id == 0) {      // Backend.cpp:154-155: the reader's own prior on vertex 0
                Factor f; f.from = -1; f.to = 0;
                memcpy(f.z, T, sizeof T);
                double i21[21];
                noise_preset(PCR_GRAPH_PRIOR, i21);
                expand_info(i21, f.info);
                priors.push_back(f);
            }
            poses.insert(poses.end(), T, T + 16);
        } else if (tag == "EDGE_SE3:QUAT") {
            long long id1, id2; double t[3], q[4], m[6][6];
            if (!(ss >> id1 >> id2 >> t[0] >> t[1] >> t[2] >> q[0] >> q[1] >> q[2] >> q[3])) return at + "malformed EDGE_SE3:QUAT";
            for (int i = 0; i < 6; ++i)
                for (int j = i; j < 6; ++j) {
                    double v;
                    if (!(ss >> v)) return at + "malformed EDGE_SE3:QUAT: 21 information entries expected";
                    m[i][j] = v; m[j][i] = v;
                }
            if (id1 < 0 || id2 < 0) return at + "negative id";
            Factor f; f.from = id1; f.to = id2;
            quat_to_pose(q, t, f.z);
            // Backend.cpp:186-190: g2o orders [translation; rotation]; the diagonal blocks swap, the off-diagonal blocks are taken as they stand
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    f.info[i * 6 + j] = m[3 + i][3 + j];
                    f.info[(3 + i) * 6 + 3 + j] = m[i][j];
                    f.info[i * 6 + 3 + j] = m[i][3 + j];
                    f.info[(3 + i) * 6 + j] = m[3 + i][j];
                }
            betweens.push_back(f);
        } else if (tag == "FIX") {      // g2o's convention for a vertex that is held constant: one or more ids
            long long id;
            if (!(ss >> id)) return at + "malformed FIX";
            do fix.emplace_back(id, at); while (ss >> id);
        }
    }
    // (a FIX record may stand before its vertex: looked at once the whole file is read)
    for (const auto& f : fix)
        if (f.first < (long long)N0 || f.first >= (long long)(N0 + poses.size() / 16))
            return f.second + "FIX " + std::to_string(f.first) + ": the file defines no vertex of that id";
    if (N0 + poses.size() / 16 > kMaxCount || s.n_factors() + priors.size() + betweens.size() > kMaxCount)
        return std::string(what) + ": more poses or factors than the device's 32-bit indices address";
    s.poses.insert(s.poses.end(), poses.begin(), poses.end());
    s.priors.insert(s.priors.end(), priors.begin(), priors.end());
    s.betweens.insert(s.betweens.end(), betweens.begin(), betweens.end());
    s.fixed.resize(s.n_poses(), 0);
    for (const auto& f : fix) s.fixed[(size_t)f.first] = 1;
    s.touch(true);
    return "";
}

// The poses, a FIX record per fixed pose and the between factors (g2o files carry neither priors nor marks nor switches), 17 digits each.
inline std::string save_g2o(const Store& s, const char* what, const char* path) {
    if (!path) return std::string(what) + ": NULL path";
    FILE* fp = fopen(path, "w");
    if (!fp) return std::string(what) + ": cannot open " + path;
    const size_t N = s.n_poses();
    for (size_t p = 0; p < N; ++p) {
        const double* T = &s.poses[16 * p];
        double q[4];
        rot_to_quat(T, q);
        fprintf(fp, "VERTEX_SE3:QUAT %zu %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", p, T[12], T[13], T[14], q[0], q[1], q[2], q[3]);
    }
    for (size_t p = 0; p < N; ++p) if (s.is_fixed(p)) fprintf(fp, "FIX %zu\n", p);
    for (const Factor& f : s.betweens) {
        double q[4], m[6][6];
        rot_to_quat(f.z, q);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {      // the inverse of the reader's block handling
                m[3 + i][3 + j] = f.info[i * 6 + j];
                m[i][j] = f.info[(3 + i) * 6 + 3 + j];
                m[i][3 + j] = f.info[i * 6 + 3 + j];
                m[3 + i][j] = f.info[(3 + i) * 6 + j];
            }
        fprintf(fp, "EDGE_SE3:QUAT %lld %lld %.17g %.17g %.17g %.17g %.17g %.17g %.17g", f.from, f.to, f.z[12], f.z[13], f.z[14], q[0], q[1], q[2], q[3]);
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j) fprintf(fp, " %.17g", m[i][j]);
        fprintf(fp, "\n");
    }
    if (fclose(fp) != 0) return std::string(what) + ": write failed: " + path;
    return "";
}

}  // namespace graph
}  // namespace pcr
