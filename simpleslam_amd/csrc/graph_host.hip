// graph_host.hip -- pcr_graph: the pose-graph back end of the C ABI (include/pcr_hip.h).
//
// Backend::optimHandler (backend/src/Backend.cpp:224-347 of the reference): one prior on key frame 0, one between factor per key frame from its
// closest earlier key frame, one per accepted loop; optimised here by Levenberg-Marquardt whose linear solve is a preconditioned conjugate
// gradient on the device (graph.hip).  The host keeps the factor lists, checks the graph (ranges, finiteness, a prior in every connected
// component), builds the CSR of incident factors and drives the trial steps; per trial step it reads 24 bytes back.
// A graph created with PCR_GRAPH_HOST touches no device: it serves everything but optimize / apply, and linearises through graph_math.h on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/pcr_hip.h"
#include "graph_dev.h"
#include "graph_forest.h"
#include "graph_math.h"
#include "small_math.h"

using namespace pcr::graph;
namespace gm = pcr::gm;

namespace {

struct DBuf {
    void* p = nullptr; size_t cap = 0;
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() { if (p) (void)hipFree(p); }
    hipError_t reserve(size_t bytes, bool keep) {
        if (bytes <= cap) return hipSuccess;
        void* q = nullptr;
        const size_t want = 2 * bytes + 256;
        hipError_t e = hipMalloc(&q, want);
        if (e != hipSuccess) return e;
        if (p && keep) e = hipMemcpy(q, p, cap, hipMemcpyDeviceToDevice);
        if (p) (void)hipFree(p);
        p = q; cap = want;
        return e;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

struct Factor {
    long long from;      // -1: a prior
    long long to;
    double z[16];
    double info[36];     // full symmetric, row-major
    unsigned char flags = 0;      // kFactorRobust, kFactorOff (between factors only): nothing a g2o file carries
};

}  // namespace

struct pcr_graph {
    int device = 0;
    bool host_only = false;
    std::vector<double> poses;               // 16 per pose, column-major; entries below n_uploaded are older than the device's while host_stale
    std::vector<Factor> priors, betweens;
    int robust_kind = PCR_GRAPH_ROBUST_NONE; // the kernel of the marked between factors; it outlives pcr_graph_clear
    double robust_delta = 0.0;
    bool dirty = false;                      // something was added, marked, switched or set since the last optimize
    bool dirty_factors = true;               // the device's factor arrays and CSR are older than the lists
    bool dirty_forest = true;                // ... and so is `forest` (poses or factors were added since it was planned)
    bool dirty_tree_dev = true;              // ... and so are the device's copies of its schedule
    ForestPlan forest;                       // the tree preconditioner's spanning forest and schedule (graph_forest.h)
    size_t n_uploaded = 0;
    bool host_stale = false;
    double last_chi2 = 0.0;
    double last_rel_tol = 0.0, last_abs_tol = 0.0;      // the tolerances the last optimisation converged under
    std::string err;
    // device side
    hipStream_t stream = nullptr;
    DBuf d_poses[2], d_lin[2], d_from, d_to, d_z, d_omega, d_rowptr, d_ent, d_vec, d_u, d_partial, d_status, d_tree_i, d_tree_d, d_in_m, d_flags;
    size_t tree_lch = 0, tree_paths = 0;     // entries of the device's light-children list and paths
    int cur = 0;
    size_t F_dev = 0;
    double* h_status = nullptr;              // page-locked, 3 doubles
};

static thread_local std::string g_graph_err;
static int gfail(pcr_graph* g, const std::string& s) { if (g) g->err = s; else g_graph_err = s; return 1; }
static int gfail(const pcr_graph* g, const std::string& s) { return gfail(const_cast<pcr_graph*>(g), s); }
#define G_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return gfail(g, std::string(#x) + ": " + hipGetErrorString(_e)); } while (0)

namespace pcr { int graph_device(const pcr_graph* g) { return g->host_only ? PCR_GRAPH_HOST : g->device; } }      // (submap.hip: pcr_map_set_poses_from_graph)

static void expand_info(const double info21[21], double full[36]) {
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { full[i * 6 + j] = info21[k]; full[j * 6 + i] = info21[k]; ++k; }
}

static bool all_finite(const double* v, int n) {
    for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

static size_t n_poses(const pcr_graph* g) { return g->poses.size() / 16; }

// Every refusal of pcr_graph_optimize (and of linearize / apply, which need the same graph), in this order: ids, from == to, numbers, priors.
static int validate(pcr_graph* g, const char* what) {
    const size_t N = n_poses(g);
    const std::string w = std::string(what) + ": ";
    for (size_t i = 0; i < g->priors.size(); ++i)
        if (g->priors[i].to < 0 || (size_t)g->priors[i].to >= N)
            return gfail(g, w + "prior " + std::to_string(i) + ": id " + std::to_string(g->priors[i].to) + " out of range (the graph holds " + std::to_string(N) + " poses)");
    for (size_t i = 0; i < g->betweens.size(); ++i) {
        const Factor& f = g->betweens[i];
        for (long long id : {f.from, f.to})
            if (id < 0 || (size_t)id >= N)
                return gfail(g, w + "between factor " + std::to_string(i) + ": id " + std::to_string(id) + " out of range (the graph holds " + std::to_string(N) + " poses)");
        if (f.from == f.to) return gfail(g, w + "between factor " + std::to_string(i) + ": from == to (" + std::to_string(f.to) + ")");
    }
    for (size_t p = 0; p < N; ++p) {
        if (g->host_stale && p < g->n_uploaded) continue;      // (the device's poses came out of an optimisation of finite numbers; a step that is not finite is never accepted)
        if (!all_finite(&g->poses[16 * p], 16)) return gfail(g, w + "pose " + std::to_string(p) + " is not finite");
    }
    for (size_t i = 0; i < g->priors.size(); ++i) {
        if (!all_finite(g->priors[i].z, 16)) return gfail(g, w + "prior " + std::to_string(i) + ": the pose is not finite");
        if (!all_finite(g->priors[i].info, 36)) return gfail(g, w + "prior " + std::to_string(i) + ": the information matrix is not finite");
    }
    for (size_t i = 0; i < g->betweens.size(); ++i) {
        if (!all_finite(g->betweens[i].z, 16)) return gfail(g, w + "between factor " + std::to_string(i) + ": the pose is not finite");
        if (!all_finite(g->betweens[i].info, 36)) return gfail(g, w + "between factor " + std::to_string(i) + ": the information matrix is not finite");
    }
    return 0;
}

// union-find over the between factors that are switched on: the first pose whose connected component holds no prior, or -1
static long long first_pose_without_prior(const pcr_graph* g) {
    const size_t N = n_poses(g);
    std::vector<size_t> parent(N);
    std::iota(parent.begin(), parent.end(), (size_t)0);
    auto find = [&](size_t a) { while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; } return a; };
    for (const Factor& f : g->betweens) {
        if (f.flags & kFactorOff) continue;
        const size_t a = find((size_t)f.from), b = find((size_t)f.to);
        if (a != b) parent[a > b ? a : b] = a > b ? b : a;
    }
    std::vector<char> has(N, 0);
    for (const Factor& f : g->priors) has[find((size_t)f.to)] = 1;
    for (size_t p = 0; p < N; ++p) if (!has[find(p)]) return (long long)p;
    return -1;
}

// pose `id` as it currently is (the device's when an optimisation moved it)
static int current_pose(pcr_graph* g, size_t id, double out[16]) {
    if (g->host_stale && id < g->n_uploaded) {
        G_TRY(hipSetDevice(g->device));
        G_TRY(hipMemcpy(out, g->d_poses[g->cur].as<double>() + 16 * id, 16 * sizeof(double), hipMemcpyDeviceToHost));
    } else memcpy(out, &g->poses[16 * id], 16 * sizeof(double));
    return 0;
}

static int sync_host(pcr_graph* g) {
    if (!g->host_stale) return 0;
    G_TRY(hipSetDevice(g->device));
    if (g->n_uploaded) G_TRY(hipMemcpy(g->poses.data(), g->d_poses[g->cur].p, g->n_uploaded * 16 * sizeof(double), hipMemcpyDeviceToHost));
    g->host_stale = false;
    return 0;
}

// the chi2 of the device's fold, on the host: blocks of 256 factors, each wave's tree, the four waves in order, then one wave over the blocks
static double wave_tree(double v[64]) {
    for (int off = 32; off > 0; off >>= 1) for (int l = 0; l + off < 64; ++l) if (l < off) v[l] += v[l + off];
    return v[0];
}
static double fold_chi2(const std::vector<double>& c) {
    const int F = (int)c.size(), nb = lin_blocks(F);
    std::vector<double> partial(nb);
    for (int b = 0; b < nb; ++b) {
        double ws[4];
        for (int w = 0; w < 4; ++w) {
            double v[64];
            for (int l = 0; l < 64; ++l) { const int e = b * kLinBlock + w * 64 + l; v[l] = e < F ? c[e] : 0.0; }
            ws[w] = wave_tree(v);
        }
        partial[b] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
    }
    double v[64];
    for (int l = 0; l < 64; ++l) { double s = 0.0; for (int b = l; b < nb; b += 64) s += partial[b]; v[l] = s; }
    return wave_tree(v);
}

// poses added since the last upload: nothing here reads a factor, so it serves a graph that has not been checked (pcr_graph_device_poses)
static int upload_poses(pcr_graph* g) {
    const size_t N = n_poses(g);
    G_TRY(hipSetDevice(g->device));
    if (N > g->n_uploaded) {
        G_TRY(g->d_poses[g->cur].reserve(N * 16 * sizeof(double), true));
        G_TRY(hipMemcpy(g->d_poses[g->cur].as<double>() + 16 * g->n_uploaded, &g->poses[16 * g->n_uploaded], (N - g->n_uploaded) * 16 * sizeof(double),
                        hipMemcpyHostToDevice));
        g->n_uploaded = N;
    }
    return 0;
}

// ... and -- when factors were added -- the factor arrays and the CSR.  ONLY after validate(): the CSR is indexed by the factors' ids.
static int upload(pcr_graph* g) {
    const size_t N = n_poses(g);
    if (upload_poses(g)) return 1;
    G_TRY(g->d_poses[g->cur ^ 1].reserve(N * 16 * sizeof(double), false));
    G_TRY(g->d_vec.reserve((N * (5 * 6 + 21) + 8) * sizeof(double) + 0, false));
    if (!g->dirty_factors) return 0;
    const size_t P = g->priors.size(), F = P + g->betweens.size();
    std::vector<int> from(F), to(F);
    std::vector<double> z(16 * F), om(36 * F);
    std::vector<unsigned char> flags(F + 1, 0);
    std::vector<int> rowptr(N + 1, 0);
    for (size_t e = 0; e < F; ++e) {
        const Factor& f = e < P ? g->priors[e] : g->betweens[e - P];
        from[e] = (int)f.from; to[e] = (int)f.to;
        flags[e] = f.flags;
        for (int k = 0; k < 16; ++k) z[k * F + e] = f.z[k];
        for (int k = 0; k < 36; ++k) om[k * F + e] = f.info[k];
        if (f.from >= 0) rowptr[f.from + 1]++;
        rowptr[f.to + 1]++;
    }
    for (size_t p = 0; p < N; ++p) rowptr[p + 1] += rowptr[p];
    std::vector<int> ent(rowptr[N] > 0 ? rowptr[N] : 1), fill(rowptr.begin(), rowptr.end() - 1);
    for (size_t e = 0; e < F; ++e) {      // ascending factor id within every row
        if (from[e] >= 0) ent[fill[from[e]]++] = (int)(e * 2);
        ent[fill[to[e]]++] = (int)(e * 2 + 1);
    }
    G_TRY(g->d_from.reserve((F + 1) * sizeof(int), false));
    G_TRY(g->d_to.reserve((F + 1) * sizeof(int), false));
    G_TRY(g->d_flags.reserve(flags.size(), false));
    G_TRY(g->d_z.reserve((16 * F + 1) * sizeof(double), false));
    G_TRY(g->d_omega.reserve((36 * F + 1) * sizeof(double), false));
    G_TRY(g->d_rowptr.reserve((N + 1) * sizeof(int), false));
    G_TRY(g->d_ent.reserve(ent.size() * sizeof(int), false));
    for (int i = 0; i < 2; ++i) G_TRY(g->d_lin[i].reserve((Lin::kDoublesPerFactor * F + 1) * sizeof(double), false));
    G_TRY(g->d_partial.reserve((lin_blocks((int)F) + 1) * sizeof(double), false));
    G_TRY(g->d_u.reserve((6 * F + 1) * sizeof(double), false));
    if (F) {
        G_TRY(hipMemcpy(g->d_from.p, from.data(), F * sizeof(int), hipMemcpyHostToDevice));
        G_TRY(hipMemcpy(g->d_to.p, to.data(), F * sizeof(int), hipMemcpyHostToDevice));
        G_TRY(hipMemcpy(g->d_flags.p, flags.data(), F, hipMemcpyHostToDevice));
        G_TRY(hipMemcpy(g->d_z.p, z.data(), 16 * F * sizeof(double), hipMemcpyHostToDevice));
        G_TRY(hipMemcpy(g->d_omega.p, om.data(), 36 * F * sizeof(double), hipMemcpyHostToDevice));
    }
    G_TRY(hipMemcpy(g->d_rowptr.p, rowptr.data(), (N + 1) * sizeof(int), hipMemcpyHostToDevice));
    G_TRY(hipMemcpy(g->d_ent.p, ent.data(), ent.size() * sizeof(int), hipMemcpyHostToDevice));
    g->F_dev = F;
    g->dirty_factors = false;
    return 0;
}

static Factors dev_factors(const pcr_graph* g) {
    Factors f;
    f.F = (int)g->F_dev; f.from = g->d_from.as<int>(); f.to = g->d_to.as<int>(); f.z = g->d_z.as<double>(); f.omega = g->d_omega.as<double>();
    f.flags = g->d_flags.as<unsigned char>();
    return f;
}
static Robust robust_of(const pcr_graph* g) {
    Robust rb;
    rb.kind = g->robust_kind; rb.delta = g->robust_delta; rb.d = g->robust_delta * g->robust_delta;
    return rb;
}
static Csr dev_csr(const pcr_graph* g) { return Csr{g->d_rowptr.as<int>(), g->d_ent.as<int>()}; }
static SolveBufs dev_bufs(const pcr_graph* g, size_t N) {
    double* v = g->d_vec.as<double>();
    SolveBufs b;
    b.x = v; b.res = v + 6 * N; b.z = v + 12 * N; b.dir = v + 18 * N; b.ap = v + 24 * N; b.L = v + 30 * N; b.u = nullptr;
    return b;
}

// The tree preconditioner's forest, planned anew only when poses or factors were added, or a factor switched, since it was made.  ONLY after validate().
static const ForestPlan& forest_of(pcr_graph* g) {
    if (g->dirty_forest) {
        // over the between factors that are switched on; the plan's factor indices are then put back into the full list's
        std::vector<long long> from, to, prior(g->priors.size());
        std::vector<int> full;
        for (size_t e = 0; e < g->betweens.size(); ++e) {
            if (g->betweens[e].flags & kFactorOff) continue;
            from.push_back(g->betweens[e].from); to.push_back(g->betweens[e].to); full.push_back((int)e);
        }
        for (size_t i = 0; i < g->priors.size(); ++i) prior[i] = g->priors[i].to;
        g->forest = plan_forest(n_poses(g), from.data(), to.data(), from.size(), prior.data(), prior.size());
        std::vector<uint8_t> in_tree(g->betweens.size(), 0);
        for (size_t k = 0; k < full.size(); ++k) in_tree[full[k]] = g->forest.in_tree[k];
        g->forest.in_tree.swap(in_tree);
        for (int& e : g->forest.tree_factor) if (e >= 0) e = full[e];
        g->dirty_forest = false;
        g->dirty_tree_dev = true;
    }
    return g->forest;
}

// ... and its schedule on the device, by position (graph_dev.h: Tree).  After upload().
static int upload_tree(pcr_graph* g) {
    const ForestPlan& fp = forest_of(g);
    const size_t N = n_poses(g), P = g->priors.size(), F = P + g->betweens.size();
    G_TRY(g->d_tree_d.reserve((N * (36 + 21 + 6) + 8) * sizeof(double), false));
    if (!g->dirty_tree_dev) return 0;
    std::vector<int> up(N), tf(N), lptr(N + 1, 0), lch;
    for (size_t q = 0; q < N; ++q) {
        const int p = fp.node[q];
        up[q] = fp.parent[p] >= 0 ? fp.pos_of[fp.parent[p]] : -1;
        tf[q] = fp.tree_factor[p] >= 0 ? (int)((P + (size_t)fp.tree_factor[p]) * 2 + fp.is_to[p]) : -1;
        for (int k = fp.child_ptr[p]; k < fp.child_ptr[p + 1]; ++k)
            if (fp.child[k] != fp.heavy[p]) lch.push_back(fp.pos_of[fp.child[k]]);
        lptr[q + 1] = (int)lch.size();
    }
    std::vector<unsigned char> in_m(F + 1, 1);
    for (size_t e = 0; e < g->betweens.size(); ++e) in_m[P + e] = fp.in_tree[e];
    // one int buffer: node, pos_of, up, tf (N each), lptr (N + 1), lch, pbeg (paths + 1), rptr (R + 1)
    std::vector<int> all;
    all.reserve(5 * N + lch.size() + fp.path_ptr.size() + fp.round_ptr.size() + 8);
    all.insert(all.end(), fp.node.begin(), fp.node.end());
    all.insert(all.end(), fp.pos_of.begin(), fp.pos_of.end());
    all.insert(all.end(), up.begin(), up.end());
    all.insert(all.end(), tf.begin(), tf.end());
    all.insert(all.end(), lptr.begin(), lptr.end());
    all.insert(all.end(), lch.begin(), lch.end());
    all.insert(all.end(), fp.path_ptr.begin(), fp.path_ptr.end());
    all.insert(all.end(), fp.round_ptr.begin(), fp.round_ptr.end());
    g->tree_lch = lch.size();
    g->tree_paths = fp.path_ptr.size() - 1;
    G_TRY(g->d_tree_i.reserve(all.size() * sizeof(int), false));
    G_TRY(g->d_in_m.reserve(in_m.size(), false));
    G_TRY(hipMemcpy(g->d_tree_i.p, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice));
    G_TRY(hipMemcpy(g->d_in_m.p, in_m.data(), in_m.size(), hipMemcpyHostToDevice));
    g->dirty_tree_dev = false;
    return 0;
}

static Tree dev_tree(const pcr_graph* g, size_t N) {
    Tree t;
    const int* i = g->d_tree_i.as<int>();
    t.R = g->forest.rounds();
    t.node = i; t.pos_of = i + N; t.up = i + 2 * N; t.tf = i + 3 * N; t.lptr = i + 4 * N; t.lch = i + 5 * N + 1;
    t.pbeg = t.lch + g->tree_lch; t.rptr = t.pbeg + g->tree_paths + 1;
    t.in_m = g->d_in_m.as<unsigned char>();
    double* d = g->d_tree_d.as<double>();
    t.G = d; t.S = d + 36 * N; t.y = d + 57 * N;
    return t;
}

// quaternion (x, y, z, w) of a rotation, Eigen's Quaternion(Matrix3) (the trace branch, or the branch of the largest diagonal element)
static void rot_to_quat(const double* T, double q[4]) {
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

// Rot3::quaternion(w, x, y, z) + Point3: Eigen's Quaternion::toRotationMatrix, the quaternion taken as it stands (not normalised)
static void quat_to_pose(const double q[4], const double t[3], double* T) {
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

extern "C" {

pcr_graph* pcr_graph_create(int device) {
    pcr_graph* g = new pcr_graph;
    if (device == PCR_GRAPH_HOST) { g->host_only = true; g->device = PCR_GRAPH_HOST; return g; }
    hipError_t e = hipSuccess;
    if (device >= 0) { g->device = device; e = hipSetDevice(device); }
    else e = hipGetDevice(&g->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&g->h_status), 4 * sizeof(double), hipHostMallocDefault);
    if (e == hipSuccess) e = g->d_status.reserve(4 * sizeof(double), false);
    if (e != hipSuccess) {
        g_graph_err = std::string("pcr_graph_create: ") + hipGetErrorString(e);
        if (g->stream) (void)hipStreamDestroy(g->stream);
        if (g->h_status) (void)hipHostFree(g->h_status);
        delete g;
        return nullptr;
    }
    return g;
}

void pcr_graph_destroy(pcr_graph* g) {
    if (!g) return;
    if (!g->host_only) {
        (void)hipSetDevice(g->device);
        if (g->stream) { (void)hipStreamSynchronize(g->stream); (void)hipStreamDestroy(g->stream); }
        if (g->h_status) (void)hipHostFree(g->h_status);
    }
    delete g;
}

const char* pcr_graph_last_error(const pcr_graph* g) { return g ? g->err.c_str() : g_graph_err.c_str(); }

int pcr_graph_noise(int kind, double info21[21]) {
    if (!info21) return 1;
    double var[6];
    switch (kind) {      // Backend.cpp:90-97: diagonal VARIANCES, [rotation; translation]
        case PCR_GRAPH_PRIOR: { const double v[6] = {1e-2, 1e-2, M_PI / 72, 1e-1, 1e-1, 1e-1}; memcpy(var, v, sizeof v); break; }
        case PCR_GRAPH_ODOM: { const double v[6] = {1e-4, 1e-4, 1e-4, 1e-1, 1e-1, 1e-1}; memcpy(var, v, sizeof v); break; }
        case PCR_GRAPH_LOOP: { const double v[6] = {1e-1, 1e-1, 1e-1, 1e-1, 1e-1, 1e-1}; memcpy(var, v, sizeof v); break; }
        default: return 1;
    }
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) info21[k++] = (i == j) ? 1.0 / var[i] : 0.0;
    return 0;
}

int pcr_graph_add_poses(pcr_graph* g, const double* poses16, size_t count) {
    if (!g) return 1;
    g->err.clear();
    if (count == 0) return 0;
    if (!poses16) return gfail(g, "pcr_graph_add_poses: NULL poses");
    if (n_poses(g) + count > 0x7fffff00u / 36) return gfail(g, "pcr_graph_add_poses: more poses than the device's 32-bit indices address");
    g->poses.insert(g->poses.end(), poses16, poses16 + 16 * count);
    g->dirty = true;
    g->dirty_factors = true; g->dirty_forest = true; g->dirty_tree_dev = true;      // (the CSR has a row per pose)
    return 0;
}

static int add_factor(pcr_graph* g, const char* what, long long from, size_t to, const double z[16], const double info21[21]) {
    if (!g) return 1;
    g->err.clear();
    if (!z || !info21) return gfail(g, std::string(what) + ": NULL pose or information matrix");
    if ((g->priors.size() + g->betweens.size() + 1) > 0x7fffff00u / 36) return gfail(g, std::string(what) + ": more factors than the device's 32-bit indices address");
    Factor f;
    f.from = from; f.to = (long long)to;
    memcpy(f.z, z, sizeof f.z);
    expand_info(info21, f.info);
    (from < 0 ? g->priors : g->betweens).push_back(f);
    g->dirty = true;
    g->dirty_factors = true; g->dirty_forest = true; g->dirty_tree_dev = true;
    return 0;
}

int pcr_graph_add_prior(pcr_graph* g, size_t id, const double pose[16], const double info21[21]) {
    return add_factor(g, "pcr_graph_add_prior", -1, id, pose, info21);
}

int pcr_graph_add_between(pcr_graph* g, size_t from, size_t to, const double z[16], const double info21[21]) {
    if (g && (long long)from < 0) return gfail(g, "pcr_graph_add_between: id out of range");
    return add_factor(g, "pcr_graph_add_between", (long long)from, to, z, info21);
}

int pcr_graph_add_between_poses(pcr_graph* g, size_t from, size_t to, const double info21[21]) {
    if (!g) return 1;
    g->err.clear();
    const size_t N = n_poses(g);
    if (from >= N || to >= N)
        return gfail(g, "pcr_graph_add_between_poses: id " + std::to_string(from >= N ? from : to) + " out of range (the graph holds " + std::to_string(N) + " poses)");
    double Xi[16], Xj[16], Xii[16], Z[16];
    if (current_pose(g, from, Xi) || current_pose(g, to, Xj)) return 1;
    gm::pose_inv(Xi, Xii);
    gm::pose_mul(Xii, Xj, Z);
    return add_factor(g, "pcr_graph_add_between_poses", (long long)from, to, Z, info21);
}

int pcr_graph_add_loop(pcr_graph* g, size_t from, size_t to, const double z[16], const double info21[21]) {
    if (g && (long long)from < 0) return gfail(g, "pcr_graph_add_loop: id out of range");
    if (add_factor(g, "pcr_graph_add_loop", (long long)from, to, z, info21)) return 1;
    g->betweens.back().flags |= kFactorRobust;
    return 0;
}

int pcr_graph_robust_rho_w(int kind, double delta, double s, double* rho, double* w) {
    if (kind < PCR_GRAPH_ROBUST_NONE || kind > PCR_GRAPH_ROBUST_TUKEY) return 1;
    if (kind != PCR_GRAPH_ROBUST_NONE && !(std::isfinite(delta) && delta > 0.0)) return 1;
    if (!(s >= 0.0)) return 1;
    double ro, wo;
    gm::robust_rho_w(kind, s, delta, delta * delta, &ro, &wo);
    if (rho) *rho = ro;
    if (w) *w = wo;
    return 0;
}

int pcr_graph_set_robust_kernel(pcr_graph* g, int kind, double delta) {
    if (!g) return 1;
    g->err.clear();
    if (kind < PCR_GRAPH_ROBUST_NONE || kind > PCR_GRAPH_ROBUST_TUKEY)
        return gfail(g, "pcr_graph_set_robust_kernel: unknown kind " + std::to_string(kind) +
                            " (PCR_GRAPH_ROBUST_NONE = 0, PCR_GRAPH_ROBUST_HUBER = 1, PCR_GRAPH_ROBUST_GEMAN_MCCLURE = 2, PCR_GRAPH_ROBUST_TUKEY = 3)");
    if (kind != PCR_GRAPH_ROBUST_NONE && !(std::isfinite(delta) && delta > 0.0))
        return gfail(g, "pcr_graph_set_robust_kernel: delta must be finite and greater than 0");
    g->robust_kind = kind;
    g->robust_delta = kind == PCR_GRAPH_ROBUST_NONE ? 0.0 : delta;
    g->dirty = true;      // (the kernel and delta travel with every launch: no table is older for it)
    return 0;
}

int pcr_graph_get_robust_kernel(const pcr_graph* g, int* kind, double* delta) {
    if (!g) return 1;
    if (kind) *kind = g->robust_kind;
    if (delta) *delta = g->robust_delta;
    return 0;
}

static int set_between_flag(pcr_graph* g, const char* what, size_t first, size_t count, unsigned char bit, bool set) {
    if (!g) return 1;
    g->err.clear();
    const size_t B = g->betweens.size();
    if (first > B || count > B - first)
        return gfail(g, std::string(what) + ": first + count exceeds the number of between factors (" + std::to_string(B) + ")");
    if (count == 0) return 0;
    for (size_t e = first; e < first + count; ++e) g->betweens[e].flags = set ? (g->betweens[e].flags | bit) : (g->betweens[e].flags & (unsigned char)~bit);
    g->dirty = true;
    g->dirty_factors = true; g->dirty_forest = true; g->dirty_tree_dev = true;      // as after an add
    return 0;
}

int pcr_graph_set_between_robust(pcr_graph* g, size_t first, size_t count, int on) {
    return set_between_flag(g, "pcr_graph_set_between_robust", first, count, kFactorRobust, on != 0);
}

int pcr_graph_set_between_enabled(pcr_graph* g, size_t first, size_t count, int on) {
    return set_between_flag(g, "pcr_graph_set_between_enabled", first, count, kFactorOff, on == 0);
}

int pcr_graph_size(const pcr_graph* g, size_t* np, size_t* n_priors, size_t* n_between) {
    if (!g) return 1;
    if (np) *np = n_poses(g);
    if (n_priors) *n_priors = g->priors.size();
    if (n_between) *n_between = g->betweens.size();
    return 0;
}

int pcr_graph_clear(pcr_graph* g) {
    if (!g) return 1;
    g->err.clear();
    g->poses.clear(); g->priors.clear(); g->betweens.clear();
    g->dirty = false; g->dirty_factors = true; g->dirty_forest = true; g->dirty_tree_dev = true; g->n_uploaded = 0; g->host_stale = false; g->F_dev = 0; g->last_chi2 = 0.0; g->last_rel_tol = g->last_abs_tol = 0.0;
    return 0;
}

void pcr_graph_default_params(pcr_graph_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->struct_size = (uint32_t)sizeof *p;
    p->max_iterations = 100;
    p->rel_tol = 1e-5; p->abs_tol = 1e-5;
    p->lambda_init = 1e-5; p->lambda_factor = 10.0; p->lambda_max = 1e5;
    p->pcg_max_iterations = 0;      // max(100, 10 * poses)
    p->pcg_rel_tol = 1e-10;
    p->pcg_preconditioner = PCR_GRAPH_PRECOND_BLOCK_JACOBI;
}

int pcr_graph_poses(const pcr_graph* gc, size_t first, size_t count, double* poses16) {
    pcr_graph* g = const_cast<pcr_graph*>(gc);
    if (!g) return 1;
    g->err.clear();
    const size_t N = n_poses(g);
    if (first > N || count > N - first) return gfail(g, "pcr_graph_poses: first + count exceeds the number of poses");
    if (count == 0) return 0;
    if (!poses16) return gfail(g, "pcr_graph_poses: NULL output");
    if (sync_host(g)) return 1;
    memcpy(poses16, &g->poses[16 * first], count * 16 * sizeof(double));
    return 0;
}

const double* pcr_graph_device_poses(const pcr_graph* gc, size_t* n) {
    pcr_graph* g = const_cast<pcr_graph*>(gc);
    if (n) *n = 0;
    if (!g) return nullptr;
    g->err.clear();
    if (g->host_only) { gfail(g, "pcr_graph_device_poses: a PCR_GRAPH_HOST graph has no device"); return nullptr; }
    if (n_poses(g) == 0) return nullptr;
    if (upload_poses(g)) return nullptr;      // (the poses alone: the factors may name poses that do not exist yet)
    if (n) *n = g->n_uploaded;
    return g->d_poses[g->cur].as<double>();
}

// s = r^T Omega r in the linearise kernel's order, and the kernel's rho(s) and w(s) for this factor (s and 1 unless it is marked)
static double factor_rho(const pcr_graph* g, const Factor& f, const double* rr, double* s_out, double* w_out) {
    double s = 0.0;
    for (int k = 0; k < 6; ++k) {
        double w = 0.0;
        for (int m = 0; m < 6; ++m) w += f.info[k * 6 + m] * rr[m];
        s += rr[k] * w;
    }
    double rho, wk;
    gm::robust_rho_w((f.flags & kFactorRobust) ? g->robust_kind : 0, s, g->robust_delta, g->robust_delta * g->robust_delta, &rho, &wk);
    if (s_out) *s_out = s;
    if (w_out) *w_out = wk;
    return rho;
}

int pcr_graph_linearize(pcr_graph* g, double* r, double* j_from, double* j_to, double* chi2) {
    if (!g) return 1;
    g->err.clear();
    if (validate(g, "pcr_graph_linearize")) return 1;
    const size_t P = g->priors.size(), F = P + g->betweens.size();
    if (g->host_only) {
        std::vector<double> c(F);
        for (size_t e = 0; e < F; ++e) {
            const Factor& f = e < P ? g->priors[e] : g->betweens[e - P];
            double rr[6], Jf[36], Jt[36];
            const double* Xj = &g->poses[16 * f.to];
            gm::factor_linearize(f.from >= 0, f.from >= 0 ? &g->poses[16 * f.from] : Xj, Xj, f.z, rr, Jf, Jt);
            c[e] = (f.flags & kFactorOff) ? 0.0 : factor_rho(g, f, rr, nullptr, nullptr);
            if (r) memcpy(r + 6 * e, rr, sizeof rr);
            if (j_from) memcpy(j_from + 36 * e, Jf, sizeof Jf);
            if (j_to) memcpy(j_to + 36 * e, Jt, sizeof Jt);
        }
        if (chi2) *chi2 = fold_chi2(c);
        return 0;
    }
    if (upload(g)) return 1;
    if (F == 0) { if (chi2) *chi2 = 0.0; return 0; }
    const Lin lin = lin_view(g->d_lin[g->cur].as<double>(), F);
    G_TRY(launch_linearize(g->d_poses[g->cur].as<double>(), dev_factors(g), robust_of(g), lin, g->d_partial.as<double>(), g->d_status.as<double>(), g->stream));
    G_TRY(hipMemcpyAsync(g->h_status, g->d_status.p, 3 * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    std::vector<double> buf((6 + 72) * F);
    G_TRY(hipMemcpyAsync(buf.data(), lin.r, 6 * F * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    G_TRY(hipMemcpyAsync(buf.data() + 6 * F, lin.jf, 72 * F * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    G_TRY(hipStreamSynchronize(g->stream));
    for (size_t e = 0; e < F; ++e) {
        if (r) for (int k = 0; k < 6; ++k) r[6 * e + k] = buf[k * F + e];
        if (j_from) for (int k = 0; k < 36; ++k) j_from[36 * e + k] = buf[6 * F + k * F + e];
        if (j_to) for (int k = 0; k < 36; ++k) j_to[36 * e + k] = buf[42 * F + k * F + e];
    }
    if (chi2) *chi2 = g->h_status[0];
    return 0;
}

int pcr_graph_between_weights(pcr_graph* g, size_t first, size_t count, double* s, double* w, uint8_t* robust, uint8_t* enabled) {
    if (!g) return 1;
    g->err.clear();
    const size_t P = g->priors.size(), B = g->betweens.size(), F = P + B;
    if (first > B || count > B - first)
        return gfail(g, "pcr_graph_between_weights: first + count exceeds the number of between factors (" + std::to_string(B) + ")");
    if (validate(g, "pcr_graph_between_weights")) return 1;
    for (size_t i = 0; i < count; ++i) {
        const unsigned char fl = g->betweens[first + i].flags;
        if (robust) robust[i] = (fl & kFactorRobust) ? 1 : 0;
        if (enabled) enabled[i] = (fl & kFactorOff) ? 0 : 1;
    }
    if (count == 0 || (!s && !w)) return 0;
    if (g->host_only) {
        for (size_t i = 0; i < count; ++i) {
            const Factor& f = g->betweens[first + i];
            double rr[6], Jf[36], Jt[36];
            gm::factor_linearize(true, &g->poses[16 * f.from], &g->poses[16 * f.to], f.z, rr, Jf, Jt);
            (void)factor_rho(g, f, rr, s ? s + i : nullptr, w ? w + i : nullptr);
        }
        return 0;
    }
    if (upload(g)) return 1;
    const Lin lin = lin_view(g->d_lin[g->cur].as<double>(), F);
    G_TRY(launch_linearize(g->d_poses[g->cur].as<double>(), dev_factors(g), robust_of(g), lin, g->d_partial.as<double>(), g->d_status.as<double>(), g->stream));
    if (s) G_TRY(hipMemcpyAsync(s, lin.s + P + first, count * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    if (w) G_TRY(hipMemcpyAsync(w, lin.w + P + first, count * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    G_TRY(hipStreamSynchronize(g->stream));
    return 0;
}

int pcr_graph_apply(pcr_graph* g, double lambda, const double* x, double* y) {
    if (!g) return 1;
    g->err.clear();
    if (validate(g, "pcr_graph_apply")) return 1;
    if (g->host_only) return gfail(g, "pcr_graph_apply: a PCR_GRAPH_HOST graph has no device: the product is the solve kernel's");
    const size_t N = n_poses(g);
    if (N == 0) return 0;
    if (!x || !y) return gfail(g, "pcr_graph_apply: NULL vector");
    if (!std::isfinite(lambda)) return gfail(g, "pcr_graph_apply: lambda is not finite");
    if (upload(g)) return 1;
    const size_t F = g->F_dev;
    const Lin lin = lin_view(g->d_lin[g->cur].as<double>(), F);
    const SolveBufs b = dev_bufs(g, N);
    G_TRY(launch_linearize(g->d_poses[g->cur].as<double>(), dev_factors(g), robust_of(g), lin, g->d_partial.as<double>(), g->d_status.as<double>(), g->stream));
    G_TRY(hipMemcpyAsync(b.res, x, 6 * N * sizeof(double), hipMemcpyHostToDevice, g->stream));
    G_TRY(launch_apply((int)N, dev_factors(g), lin, dev_csr(g), lambda, b.res, b.ap, g->d_u.as<double>(), g->stream));
    G_TRY(hipMemcpyAsync(y, b.ap, 6 * N * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    G_TRY(hipStreamSynchronize(g->stream));
    return 0;
}

int pcr_graph_tree(const pcr_graph* gc, int64_t* parent, size_t n, size_t* n_tree_edges, size_t* n_other_edges) {
    pcr_graph* g = const_cast<pcr_graph*>(gc);
    if (!g) return 1;
    g->err.clear();
    const size_t N = n_poses(g);
    if (validate(g, "pcr_graph_tree")) return 1;
    const long long lone = first_pose_without_prior(g);
    if (lone >= 0)
        return gfail(g, "pcr_graph_tree: pose " + std::to_string(lone) + " lies in a connected component without a prior: the system would be singular");
    if (parent && n < N) return gfail(g, "pcr_graph_tree: parent has room for " + std::to_string(n) + " entries, the graph holds " + std::to_string(N) + " poses");
    const ForestPlan& fp = forest_of(g);
    if (parent) for (size_t p = 0; p < N; ++p) parent[p] = fp.parent[p];
    if (n_tree_edges) *n_tree_edges = fp.n_tree;
    if (n_other_edges) *n_other_edges = fp.n_other;
    return 0;
}

int pcr_graph_precondition(pcr_graph* g, double lambda, int kind, const double* r, double* z) {
    if (!g) return 1;
    g->err.clear();
    if (kind != PCR_GRAPH_PRECOND_BLOCK_JACOBI && kind != PCR_GRAPH_PRECOND_TREE)
        return gfail(g, "pcr_graph_precondition: unknown preconditioner " + std::to_string(kind) + " (PCR_GRAPH_PRECOND_BLOCK_JACOBI = 0, PCR_GRAPH_PRECOND_TREE = 1)");
    if (validate(g, "pcr_graph_precondition")) return 1;
    const long long lone = first_pose_without_prior(g);
    if (lone >= 0)
        return gfail(g, "pcr_graph_precondition: pose " + std::to_string(lone) + " lies in a connected component without a prior: the system would be singular");
    if (g->host_only) return gfail(g, "pcr_graph_precondition: a PCR_GRAPH_HOST graph has no device: the sweeps are the solve kernel's");
    const size_t N = n_poses(g);
    if (N == 0) return 0;
    if (!r || !z) return gfail(g, "pcr_graph_precondition: NULL vector");
    if (!(lambda >= 0.0) || !std::isfinite(lambda)) return gfail(g, "pcr_graph_precondition: lambda must be finite and not negative");
    if (upload(g)) return 1;
    const bool tree = kind == PCR_GRAPH_PRECOND_TREE;
    if (tree && upload_tree(g)) return 1;
    const Tree tr = tree ? dev_tree(g, N) : Tree{};
    const size_t F = g->F_dev;
    const Lin lin = lin_view(g->d_lin[g->cur].as<double>(), F);
    const SolveBufs b = dev_bufs(g, N);
    int* d_flag = reinterpret_cast<int*>(g->d_status.as<double>() + 3);
    G_TRY(launch_linearize(g->d_poses[g->cur].as<double>(), dev_factors(g), robust_of(g), lin, g->d_partial.as<double>(), g->d_status.as<double>(), g->stream));
    G_TRY(hipMemcpyAsync(b.res, r, 6 * N * sizeof(double), hipMemcpyHostToDevice, g->stream));
    G_TRY(launch_precondition((int)N, dev_factors(g), lin, dev_csr(g), tree ? &tr : nullptr, lambda, b, d_flag, g->stream));
    G_TRY(hipMemcpyAsync(z, b.z, 6 * N * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    G_TRY(hipMemcpyAsync(g->h_status + 3, d_flag, sizeof(int), hipMemcpyDeviceToHost, g->stream));
    G_TRY(hipStreamSynchronize(g->stream));
    int flag = 0;
    memcpy(&flag, g->h_status + 3, sizeof flag);
    if (flag) return gfail(g, "pcr_graph_precondition: a block of the preconditioner is not positive definite");
    return 0;
}

int pcr_graph_optimize(pcr_graph* g, const pcr_graph_params* params, pcr_graph_result* out) {
    if (!g) return 1;
    g->err.clear();
    pcr_graph_result res;
    memset(&res, 0, sizeof res);
    for (int i = 0; i < 16; ++i) res.delta[i] = (i % 5 == 0) ? 1.0 : 0.0;
    pcr_graph_params prm;
    pcr_graph_default_params(&prm);
    if (params) {
        if (params->struct_size != sizeof prm) return gfail(g, "pcr_graph_optimize: pcr_graph_params.struct_size does not match (use pcr_graph_default_params)");
        prm = *params;
    }
    if (!(prm.lambda_factor > 1.0) || !(prm.lambda_init > 0.0) || !std::isfinite(prm.lambda_max) || prm.max_iterations < 0 || prm.pcg_max_iterations < 0 ||
        !(prm.pcg_rel_tol >= 0.0) || !(prm.rel_tol >= 0.0) || !(prm.abs_tol >= 0.0))
        return gfail(g, "pcr_graph_optimize: parameters out of range (lambda_factor > 1, lambda_init > 0, tolerances and caps >= 0)");
    if (prm.pcg_preconditioner != PCR_GRAPH_PRECOND_BLOCK_JACOBI && prm.pcg_preconditioner != PCR_GRAPH_PRECOND_TREE)
        return gfail(g, "pcr_graph_optimize: unknown pcg_preconditioner " + std::to_string(prm.pcg_preconditioner) +
                            " (PCR_GRAPH_PRECOND_BLOCK_JACOBI = 0, PCR_GRAPH_PRECOND_TREE = 1)");
    const size_t N = n_poses(g);
    if (N == 0 && g->priors.empty() && g->betweens.empty()) { if (out) *out = res; return 0; }      // an empty graph: nothing to do
    if (validate(g, "pcr_graph_optimize")) return 1;
    const long long lone = first_pose_without_prior(g);
    if (lone >= 0)
        return gfail(g, "pcr_graph_optimize: pose " + std::to_string(lone) + " lies in a connected component without a prior: the system would be singular");
    if (g->host_only) return gfail(g, "pcr_graph_optimize: a PCR_GRAPH_HOST graph has no device (create the graph with a device ordinal, or -1)");
    // Nothing new since an optimisation that CONVERGED under tolerances no looser than these: it stands.  One that ran out of iterations or of
    // lambda, or converged under looser tolerances, goes on from the current estimates.
    if (!g->dirty && prm.rel_tol >= g->last_rel_tol && prm.abs_tol >= g->last_abs_tol) {
        res.converged = 1;
        res.chi2_initial = res.chi2_final = g->last_chi2;
        res.lambda = prm.lambda_init;
        if (out) *out = res;
        return 0;
    }
    double last_old[16];
    if (current_pose(g, N - 1, last_old)) return 1;
    if (upload(g)) return 1;
    const bool tree = prm.pcg_preconditioner == PCR_GRAPH_PRECOND_TREE;
    if (tree && upload_tree(g)) return 1;
    const Tree tr = tree ? dev_tree(g, N) : Tree{};
    const size_t F = g->F_dev;
    const Factors fac = dev_factors(g);
    const Robust rb = robust_of(g);
    const Csr csr = dev_csr(g);
    SolveBufs b = dev_bufs(g, N);
    b.u = g->d_u.as<double>();
    double* d_status = g->d_status.as<double>();
    double* d_partial = g->d_partial.as<double>();
    const long long cap64 = prm.pcg_max_iterations > 0 ? prm.pcg_max_iterations : std::max<long long>(100, 10 * (long long)N);
    const int cap = (int)std::min<long long>(cap64, 0x7fffffff);

    Lin lin = lin_view(g->d_lin[g->cur].as<double>(), F);
    G_TRY(launch_linearize(g->d_poses[g->cur].as<double>(), fac, rb, lin, d_partial, d_status, g->stream));
    G_TRY(hipMemcpyAsync(g->h_status, d_status, 3 * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    G_TRY(hipStreamSynchronize(g->stream));
    double chi2 = g->h_status[0];
    if (!std::isfinite(chi2)) return gfail(g, "pcr_graph_optimize: chi2 of the initial estimates is not finite");
    res.chi2_initial = chi2;
    double lambda = prm.lambda_init;
    while (res.iterations < prm.max_iterations) {
        const int trial = g->cur ^ 1;
        const Lin lin_trial = lin_view(g->d_lin[trial].as<double>(), F);
        if (tree) G_TRY(launch_solve_tree((int)N, fac, lin, csr, tr, lambda, cap, prm.pcg_rel_tol, b, d_status, g->stream));
        else G_TRY(launch_solve((int)N, fac, lin, csr, lambda, cap, prm.pcg_rel_tol, b, d_status, g->stream));
        G_TRY(launch_retract((int)N, g->d_poses[g->cur].as<double>(), b.x, g->d_poses[trial].as<double>(), g->stream));
        G_TRY(launch_linearize(g->d_poses[trial].as<double>(), fac, rb, lin_trial, d_partial, d_status, g->stream));
        G_TRY(hipMemcpyAsync(g->h_status, d_status, 3 * sizeof(double), hipMemcpyDeviceToHost, g->stream));
        G_TRY(hipStreamSynchronize(g->stream));
        int words[2];
        memcpy(words, &g->h_status[2], sizeof words);
        const double chi2_new = g->h_status[0];
        res.iterations += 1;
        res.pcg_iterations += words[0];
        if (words[1] == 1) res.pcg_capped += 1;
        if (chi2_new < chi2) {      // accepted: the trial poses and their linearisation become the current ones
            const double dec = chi2 - chi2_new;
            g->cur = trial;
            g->host_stale = true;
            lin = lin_trial;
            res.accepted += 1;
            lambda /= prm.lambda_factor;
            const double before = chi2;
            chi2 = chi2_new;
            if (dec < prm.abs_tol || dec < prm.rel_tol * before) { res.converged = 1; break; }
        } else {
            // rejected.  A step that could not lower chi2 and raised it by less than abs_tol: the estimate is at its minimum to that tolerance
            if (chi2_new - chi2 < prm.abs_tol) { res.converged = 1; break; }
            lambda *= prm.lambda_factor;
            if (lambda > prm.lambda_max) break;
        }
    }
    res.chi2_final = chi2;
    res.lambda = lambda;
    g->last_chi2 = chi2;
    g->dirty = !res.converged;
    g->last_rel_tol = prm.rel_tol; g->last_abs_tol = prm.abs_tol;
    double last_new[16], inv_old[16];
    if (current_pose(g, N - 1, last_new)) return 1;
    gm::pose_inv(last_old, inv_old);
    gm::pose_mul(last_new, inv_old, res.delta);      // Backend.cpp:321: keyframes.back().pose * latest_pose.inverse()
    pcr::t2se3(res.delta);                           // :331
    if (out) *out = res;
    return 0;
}

int pcr_graph_load_g2o(pcr_graph* g, const char* path) {
    if (!g) return 1;
    g->err.clear();
    if (!path) return gfail(g, "pcr_graph_load_g2o: NULL path");
    std::ifstream in(path);
    if (!in.is_open()) return gfail(g, std::string("pcr_graph_load_g2o: cannot open ") + path);
    // read everything first: a file that is refused leaves the graph as it was
    std::vector<double> poses;
    std::vector<Factor> priors, betweens;
    const size_t N0 = n_poses(g);
    std::string line;
    size_t lineno = 0;
    while (std::getline(in, line)) {
        ++lineno;
        std::istringstream ss(line);
        std::string tag;
        ss >> tag;
        const std::string at = std::string("pcr_graph_load_g2o: ") + path + ":" + std::to_string(lineno) + ": ";
        if (tag == "VERTEX3" || tag == "EDGE3")
            return gfail(g, at + tag + " records (Euler angles) are not read: write the graph with VERTEX_SE3:QUAT and EDGE_SE3:QUAT");
        if (tag == "VERTEX_SE3:QUAT") {
            long long id; double t[3], q[4];
            if (!(ss >> id >> t[0] >> t[1] >> t[2] >> q[0] >> q[1] >> q[2] >> q[3])) return gfail(g, at + "malformed VERTEX_SE3:QUAT");
            if (id != (long long)(N0 + poses.size() / 16))
                return gfail(g, at + "vertex id " + std::to_string(id) + " where " + std::to_string(N0 + poses.size() / 16) + " is next: ids are consecutive from 0");
            double T[16];
            quat_to_pose(q, t, T);
            if (id == 0) {      // Backend.cpp:154-155: the reader's own prior on vertex 0
                Factor f; f.from = -1; f.to = 0;
                memcpy(f.z, T, sizeof T);
                double i21[21];
                pcr_graph_noise(PCR_GRAPH_PRIOR, i21);
                expand_info(i21, f.info);
                priors.push_back(f);
            }
            poses.insert(poses.end(), T, T + 16);
        } else if (tag == "EDGE_SE3:QUAT") {
            long long id1, id2; double t[3], q[4], m[6][6];
            if (!(ss >> id1 >> id2 >> t[0] >> t[1] >> t[2] >> q[0] >> q[1] >> q[2] >> q[3])) return gfail(g, at + "malformed EDGE_SE3:QUAT");
            for (int i = 0; i < 6; ++i)
                for (int j = i; j < 6; ++j) {
                    double v;
                    if (!(ss >> v)) return gfail(g, at + "malformed EDGE_SE3:QUAT: 21 information entries expected");
                    m[i][j] = v; m[j][i] = v;
                }
            if (id1 < 0 || id2 < 0) return gfail(g, at + "negative id");
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
        }
    }
    if ((N0 + poses.size() / 16) > 0x7fffff00u / 36 || g->priors.size() + g->betweens.size() + priors.size() + betweens.size() > 0x7fffff00u / 36)
        return gfail(g, "pcr_graph_load_g2o: more poses or factors than the device's 32-bit indices address");
    g->poses.insert(g->poses.end(), poses.begin(), poses.end());
    g->priors.insert(g->priors.end(), priors.begin(), priors.end());
    g->betweens.insert(g->betweens.end(), betweens.begin(), betweens.end());
    g->dirty = true; g->dirty_factors = true; g->dirty_forest = true; g->dirty_tree_dev = true;
    return 0;
}

int pcr_graph_save_g2o(const pcr_graph* gc, const char* path) {
    pcr_graph* g = const_cast<pcr_graph*>(gc);
    if (!g) return 1;
    g->err.clear();
    if (!path) return gfail(g, "pcr_graph_save_g2o: NULL path");
    if (sync_host(g)) return 1;
    FILE* fp = fopen(path, "w");
    if (!fp) return gfail(g, std::string("pcr_graph_save_g2o: cannot open ") + path);
    const size_t N = n_poses(g);
    for (size_t p = 0; p < N; ++p) {
        const double* T = &g->poses[16 * p];
        double q[4];
        rot_to_quat(T, q);
        fprintf(fp, "VERTEX_SE3:QUAT %zu %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", p, T[12], T[13], T[14], q[0], q[1], q[2], q[3]);
    }
    for (const Factor& f : g->betweens) {
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
    if (fclose(fp) != 0) return gfail(g, std::string("pcr_graph_save_g2o: write failed: ") + path);
    return 0;
}

}  // extern "C"
