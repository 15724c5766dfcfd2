// graph_host.hip -- pcr_graph: the pose-graph back end of the C ABI (include/pcr_hip.h): the entry points and the device side.
//
// Backend::optimHandler (backend/src/Backend.cpp:224-347 of the reference): one prior on key frame 0, one between factor per key frame from its
// closest earlier key frame, one per accepted loop; optimised here by Levenberg-Marquardt whose linear solve is a preconditioned conjugate
// gradient on the device (graph.hip).  The lists, their checks, the arrays the device reads and the g2o files are graph_store.h's; the
// decisions between two launches are graph_opt.h's.  This file keeps the device's mirror of the store current (prepare), launches, and per trial
// step reads 24 bytes back.
// A graph created with PCR_GRAPH_HOST touches no device: it serves everything but optimize / apply, and linearises through graph_math.h on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pcr_hip.h"
#include "graph_dev.h"
#include "graph_forest.h"
#include "graph_math.h"
#include "graph_opt.h"
#include "graph_store.h"
#include "small_math.h"

using namespace pcr::graph;
using namespace pcr::graph_opt;
namespace gm = pcr::gm;

static_assert(kMarkRobust == kFactorRobust && kMarkOff == kFactorOff && kPackFromFixed == kFactorFromFixed && kPackToFixed == kFactorToFixed,
              "the store's flags are the bits the kernels read");

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

// The status words as the host reads them (graph_dev.h: status): the first kStatusRead bytes are one trial step's read; the fourth double of
// the device's buffer is the int launch_precondition writes its flag into.
struct Status {
    double chi2, pcg_residual;
    int pcg_iterations, pcg_flag;
    int precond_flag, unused;
};
constexpr size_t kStatusRead = offsetof(Status, precond_flag);
static_assert(sizeof(Status) == 4 * sizeof(double) && kStatusRead == 3 * sizeof(double), "four doubles on the device, three per read");

// `vec`: per pose the solve's five work vectors and the preconditioner's 21-entry factor, one array after another (SolveBufs)
enum : size_t { kVecX = 0, kVecRes = 6, kVecZ = 12, kVecDir = 18, kVecAp = 24, kVecL = 30, kVecPerPose = kVecL + 21 };
// `tree_d`: per position G (36), S (21), y (6) (Tree)
enum : size_t { kTreeG = 0, kTreeS = 36, kTreeY = 57, kTreePerPose = kTreeY + 6 };

// The device's mirror of the store and the solve's work space.
struct Device {
    int ordinal = 0;
    hipStream_t stream = nullptr;
    Status* h_status = nullptr;      // page-locked
    DBuf poses[2], lin[2], from, to, z, omega, flags, pose_fixed, rowptr, ent, vec, u, partial, status, tree_i, tree_d, in_m;
    bool any_fixed = false;          // a pose of the packed tables is fixed: the launches take the instantiations that read the flags
    int cur = 0;                     // which of poses[] / lin[] holds the current estimates
    size_t n_poses = 0;              // poses the device holds
    bool ahead = false;              // ... and an optimisation moved them: the store's first n_poses are older
    size_t F = 0;
    uint64_t factors_rev = 0;        // the store's `structure` the factor tables and the CSR were packed at
    size_t tree_lch = 0, tree_paths = 0;      // entries of the light-children list and paths of the schedule in tree_i
    uint64_t tree_rev = 0;           // ... and the `structure` it was uploaded at
};

}  // namespace

struct pcr_graph {
    bool host_only = false;
    Store store;
    ForestPlan forest;               // the tree preconditioner's spanning forest and schedule (graph_forest.h)
    uint64_t forest_rev = 0;         // the store's `structure` it was planned at
    LmSettled settled;
    std::string err;
    Device dev;
};

static thread_local std::string g_graph_err;
static int gfail(pcr_graph* g, const std::string& s) { if (g) g->err = s; else g_graph_err = s; return 1; }
static int gfail(const pcr_graph* g, const std::string& s) { return gfail(const_cast<pcr_graph*>(g), s); }
static int refuse(pcr_graph* g, const std::string& message) { return message.empty() ? 0 : gfail(g, message); }
#define G_ENTER(g) do { if (!(g)) return 1; (g)->err.clear(); } while (0)
#define G_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return gfail(g, std::string(#x) + ": " + hipGetErrorString(_e)); } while (0)

namespace pcr { int graph_device(const pcr_graph* g) { return g->host_only ? PCR_GRAPH_HOST : g->dev.ordinal; } }      // (submap.hip: pcr_map_set_poses_from_graph)

// graph_store.h's check; the poses an optimisation left on the device are not looked at
static int validate(pcr_graph* g, const char* what) { return refuse(g, check(g->store, what, g->dev.ahead ? g->dev.n_poses : 0)); }

// pose `id` as it currently is (the device's when an optimisation moved it)
static int current_pose(pcr_graph* g, size_t id, double out[16]) {
    const Device& d = g->dev;
    if (d.ahead && id < d.n_poses) {
        G_TRY(hipSetDevice(d.ordinal));
        G_TRY(hipMemcpy(out, d.poses[d.cur].as<double>() + 16 * id, 16 * sizeof(double), hipMemcpyDeviceToHost));
    } else memcpy(out, &g->store.poses[16 * id], 16 * sizeof(double));
    return 0;
}

static int sync_host(pcr_graph* g) {
    Device& d = g->dev;
    if (!d.ahead) return 0;
    G_TRY(hipSetDevice(d.ordinal));
    if (d.n_poses) G_TRY(hipMemcpy(g->store.poses.data(), d.poses[d.cur].p, d.n_poses * 16 * sizeof(double), hipMemcpyDeviceToHost));
    d.ahead = false;
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

// ---- the device's mirror: what is older than the store is uploaded ------------------------------------------------------------------------

// poses added since the last upload: nothing here reads a factor, so it serves a graph that has not been checked (pcr_graph_device_poses)
static int upload_poses(pcr_graph* g) {
    Device& d = g->dev;
    const size_t N = g->store.n_poses();
    G_TRY(hipSetDevice(d.ordinal));
    if (N > d.n_poses) {
        G_TRY(d.poses[d.cur].reserve(N * 16 * sizeof(double), true));
        G_TRY(hipMemcpy(d.poses[d.cur].as<double>() + 16 * d.n_poses, &g->store.poses[16 * d.n_poses], (N - d.n_poses) * 16 * sizeof(double), hipMemcpyHostToDevice));
        d.n_poses = N;
    }
    return 0;
}

// ... and -- when the structure changed -- the factor arrays and the CSR.  ONLY after validate() (graph_store.h: pack).
static int upload(pcr_graph* g) {
    Device& d = g->dev;
    const size_t N = g->store.n_poses();
    if (upload_poses(g)) return 1;
    G_TRY(d.poses[d.cur ^ 1].reserve(N * 16 * sizeof(double), false));
    G_TRY(d.vec.reserve((N * kVecPerPose + 8) * sizeof(double), false));
    if (d.factors_rev == g->store.structure) return 0;
    const Packed k = pack(g->store);
    const size_t F = k.from.size();
    // what pack() made: buffer, source, room (never of nothing), bytes
    const struct { DBuf& buf; const void* src; size_t room, bytes; } tables[] = {
        {d.from, k.from.data(), (F + 1) * sizeof(int), F * sizeof(int)},
        {d.to, k.to.data(), (F + 1) * sizeof(int), F * sizeof(int)},
        {d.flags, k.flags.data(), k.flags.size(), F},
        {d.pose_fixed, k.pose_fixed.data(), k.pose_fixed.size(), N},
        {d.z, k.z.data(), (16 * F + 1) * sizeof(double), 16 * F * sizeof(double)},
        {d.omega, k.omega.data(), (36 * F + 1) * sizeof(double), 36 * F * sizeof(double)},
        {d.rowptr, k.row_ptr.data(), (N + 1) * sizeof(int), (N + 1) * sizeof(int)},
        {d.ent, k.ent.data(), k.ent.size() * sizeof(int), k.ent.size() * sizeof(int)},
    };
    for (const auto& t : tables) G_TRY(t.buf.reserve(t.room, false));
    for (int i = 0; i < 2; ++i) G_TRY(d.lin[i].reserve((Lin::kDoublesPerFactor * F + 1) * sizeof(double), false));
    G_TRY(d.partial.reserve((lin_blocks((int)F) + 1) * sizeof(double), false));
    G_TRY(d.u.reserve((6 * F + 1) * sizeof(double), false));
    for (const auto& t : tables) if (t.bytes) G_TRY(hipMemcpy(t.buf.p, t.src, t.bytes, hipMemcpyHostToDevice));
    d.F = F;
    d.any_fixed = k.any_fixed;
    d.factors_rev = g->store.structure;
    return 0;
}

// The tree preconditioner's forest, planned anew only when the structure changed since it was made.  ONLY after validate().
static const ForestPlan& forest_of(pcr_graph* g) {
    const Store& s = g->store;
    if (g->forest_rev != s.structure) {
        // over the between factors that are switched on; the plan's factor indices are then put back into the full list's.  The anchors a
        // root is chosen among: the poses that hold a prior and the fixed poses.
        std::vector<long long> from, to, prior(s.priors.size());
        std::vector<int> full;
        for (size_t e = 0; e < s.betweens.size(); ++e) {
            if (s.betweens[e].flags & kMarkOff) continue;
            from.push_back(s.betweens[e].from); to.push_back(s.betweens[e].to); full.push_back((int)e);
        }
        for (size_t i = 0; i < s.priors.size(); ++i) prior[i] = s.priors[i].to;
        for (size_t p = 0; p < s.n_poses(); ++p) if (s.is_fixed(p)) prior.push_back((long long)p);
        g->forest = plan_forest(s.n_poses(), from.data(), to.data(), from.size(), prior.data(), prior.size());
        std::vector<uint8_t> in_tree(s.betweens.size(), 0);
        for (size_t k = 0; k < full.size(); ++k) in_tree[full[k]] = g->forest.in_tree[k];
        g->forest.in_tree.swap(in_tree);
        for (int& e : g->forest.tree_factor) if (e >= 0) e = full[e];
        g->forest_rev = s.structure;
    }
    return g->forest;
}

// ... and its schedule on the device, by position (graph_dev.h: Tree).  After upload().
static int upload_tree(pcr_graph* g) {
    Device& d = g->dev;
    const ForestPlan& fp = forest_of(g);
    const size_t N = g->store.n_poses(), P = g->store.priors.size(), B = g->store.betweens.size(), F = P + B;
    G_TRY(d.tree_d.reserve((N * kTreePerPose + 8) * sizeof(double), false));
    if (d.tree_rev == g->store.structure) return 0;
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
    for (size_t e = 0; e < B; ++e) in_m[P + e] = fp.in_tree[e];
    // one int buffer: node, pos_of, up, tf (N each), lptr (N + 1), lch, pbeg (paths + 1), rptr (R + 1)
    std::vector<int> all;
    for (const std::vector<int>* part : std::initializer_list<const std::vector<int>*>{&fp.node, &fp.pos_of, &up, &tf, &lptr, &lch, &fp.path_ptr, &fp.round_ptr}) all.insert(all.end(), part->begin(), part->end());
    d.tree_lch = lch.size();
    d.tree_paths = fp.path_ptr.size() - 1;
    G_TRY(d.tree_i.reserve(all.size() * sizeof(int), false));
    G_TRY(d.in_m.reserve(in_m.size(), false));
    G_TRY(hipMemcpy(d.tree_i.p, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice));
    G_TRY(hipMemcpy(d.in_m.p, in_m.data(), in_m.size(), hipMemcpyHostToDevice));
    d.tree_rev = g->store.structure;
    return 0;
}

// Every view a launch takes, made by prepare() and valid until the store changes.  poses[] and lin[] are indexed like Device's: by buffer.
struct Ctx {
    size_t N = 0, P = 0, F = 0;
    Factors fac;
    Robust rb;
    bool fixed = false;         // the graph holds a fixed pose ...
    const unsigned char* pose_fixed = nullptr;      // ... and then the flag per pose
    Csr csr;
    double* poses[2];
    Lin lin[2];
    SolveBufs b;
    Tree tree;                  // filled when prepare() was asked for it
    double *partial, *status;
    int* precond_flag;          // the fourth double of status
    hipStream_t stream;
};

// Uploads what is older than the store (the tree's schedule too when `tree`) and fills the views.  ONLY after validate().
static int prepare(pcr_graph* g, bool tree, Ctx* c) {
    if (upload(g)) return 1;
    if (tree && upload_tree(g)) return 1;
    const Device& d = g->dev;
    const size_t N = g->store.n_poses(), F = d.F;
    c->N = N; c->P = g->store.priors.size(); c->F = F;
    c->fac.F = (int)F; c->fac.from = d.from.as<int>(); c->fac.to = d.to.as<int>(); c->fac.z = d.z.as<double>(); c->fac.omega = d.omega.as<double>();
    c->fac.flags = d.flags.as<unsigned char>();
    c->rb.kind = g->store.robust_kind; c->rb.delta = g->store.robust_delta; c->rb.d = g->store.robust_delta * g->store.robust_delta;
    c->fixed = d.any_fixed; c->pose_fixed = d.any_fixed ? d.pose_fixed.as<unsigned char>() : nullptr;
    c->csr = Csr{d.rowptr.as<int>(), d.ent.as<int>()};
    for (int i = 0; i < 2; ++i) { c->poses[i] = d.poses[i].as<double>(); c->lin[i] = lin_view(d.lin[i].as<double>(), F); }
    double* v = d.vec.as<double>();
    c->b.x = v + kVecX * N; c->b.res = v + kVecRes * N; c->b.z = v + kVecZ * N; c->b.dir = v + kVecDir * N; c->b.ap = v + kVecAp * N; c->b.L = v + kVecL * N;
    c->b.u = d.u.as<double>();
    c->tree = Tree{};
    if (tree) {
        Tree& t = c->tree;
        const int* i = d.tree_i.as<int>();
        t.R = g->forest.rounds();
        t.node = i; t.pos_of = i + N; t.up = i + 2 * N; t.tf = i + 3 * N; t.lptr = i + 4 * N; t.lch = i + 5 * N + 1;
        t.pbeg = t.lch + d.tree_lch; t.rptr = t.pbeg + d.tree_paths + 1;
        t.in_m = d.in_m.as<unsigned char>();
        double* td = d.tree_d.as<double>();
        t.G = td + kTreeG * N; t.S = td + kTreeS * N; t.y = td + kTreeY * N;
    }
    c->partial = d.partial.as<double>();
    c->status = d.status.as<double>();
    c->precond_flag = reinterpret_cast<int*>(c->status + kStatusRead / sizeof(double));
    c->stream = d.stream;
    return 0;
}

// linearise every factor at poses[which] into lin[which]; chi2 into status[0]
static hipError_t linearize_at(const Ctx& c, int which) {
    return launch_linearize(c.poses[which], c.fac, c.rb, c.fixed, c.lin[which], c.partial, c.status, c.stream);
}

// one trial step's read: chi2 and the solve's words into g->dev.h_status
static hipError_t read_status(const pcr_graph* g, const Ctx& c) {
    hipError_t e = hipMemcpyAsync(g->dev.h_status, c.status, kStatusRead, hipMemcpyDeviceToHost, c.stream);
    return e != hipSuccess ? e : hipStreamSynchronize(c.stream);
}

extern "C" {

pcr_graph* pcr_graph_create(int device) {
    pcr_graph* g = new pcr_graph;
    Device& d = g->dev;
    if (device == PCR_GRAPH_HOST) { g->host_only = true; d.ordinal = PCR_GRAPH_HOST; return g; }
    hipError_t e = hipSuccess;
    if (device >= 0) { d.ordinal = device; e = hipSetDevice(device); }
    else e = hipGetDevice(&d.ordinal);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&d.h_status), sizeof(Status), hipHostMallocDefault);
    if (e == hipSuccess) e = d.status.reserve(sizeof(Status), false);
    if (e != hipSuccess) {
        g_graph_err = std::string("pcr_graph_create: ") + hipGetErrorString(e);
        if (d.stream) (void)hipStreamDestroy(d.stream);
        if (d.h_status) (void)hipHostFree(d.h_status);
        delete g;
        return nullptr;
    }
    return g;
}

void pcr_graph_destroy(pcr_graph* g) {
    if (!g) return;
    if (!g->host_only) {
        (void)hipSetDevice(g->dev.ordinal);
        if (g->dev.stream) { (void)hipStreamSynchronize(g->dev.stream); (void)hipStreamDestroy(g->dev.stream); }
        if (g->dev.h_status) (void)hipHostFree(g->dev.h_status);
    }
    delete g;
}

const char* pcr_graph_last_error(const pcr_graph* g) { return g ? g->err.c_str() : g_graph_err.c_str(); }

int pcr_graph_noise(int kind, double info21[21]) { return info21 && noise_preset(kind, info21) ? 0 : 1; }

int pcr_graph_add_poses(pcr_graph* g, const double* poses16, size_t count) {
    G_ENTER(g);
    return refuse(g, add_poses(g->store, "pcr_graph_add_poses", poses16, count));
}

int pcr_graph_add_prior(pcr_graph* g, size_t id, const double pose[16], const double info21[21]) {
    G_ENTER(g);
    return refuse(g, add_factor(g->store, "pcr_graph_add_prior", -1, id, pose, info21));
}

int pcr_graph_add_between(pcr_graph* g, size_t from, size_t to, const double z[16], const double info21[21]) {
    if (!g) return 1;
    if ((long long)from < 0) return gfail(g, "pcr_graph_add_between: id out of range");
    g->err.clear();
    return refuse(g, add_factor(g->store, "pcr_graph_add_between", (long long)from, to, z, info21));
}

int pcr_graph_add_between_poses(pcr_graph* g, size_t from, size_t to, const double info21[21]) {
    G_ENTER(g);
    const size_t N = g->store.n_poses();
    if (from >= N || to >= N)
        return gfail(g, "pcr_graph_add_between_poses: id " + std::to_string(from >= N ? from : to) + " out of range (the graph holds " + std::to_string(N) + " poses)");
    double Xi[16], Xj[16], Xii[16], Z[16];
    if (current_pose(g, from, Xi) || current_pose(g, to, Xj)) return 1;
    gm::pose_inv(Xi, Xii);
    gm::pose_mul(Xii, Xj, Z);
    return refuse(g, add_factor(g->store, "pcr_graph_add_between_poses", (long long)from, to, Z, info21));
}

int pcr_graph_add_loop(pcr_graph* g, size_t from, size_t to, const double z[16], const double info21[21]) {
    if (!g) return 1;
    if ((long long)from < 0) return gfail(g, "pcr_graph_add_loop: id out of range");
    g->err.clear();
    return refuse(g, add_factor(g->store, "pcr_graph_add_loop", (long long)from, to, z, info21, kMarkRobust));
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
    G_ENTER(g);
    return refuse(g, set_robust_kernel(g->store, "pcr_graph_set_robust_kernel", kind, delta));
}

int pcr_graph_get_robust_kernel(const pcr_graph* g, int* kind, double* delta) {
    if (!g) return 1;
    if (kind) *kind = g->store.robust_kind;
    if (delta) *delta = g->store.robust_delta;
    return 0;
}

int pcr_graph_set_between_robust(pcr_graph* g, size_t first, size_t count, int on) {
    G_ENTER(g);
    return refuse(g, set_between_flag(g->store, "pcr_graph_set_between_robust", first, count, kMarkRobust, on != 0));
}

int pcr_graph_set_between_enabled(pcr_graph* g, size_t first, size_t count, int on) {
    G_ENTER(g);
    return refuse(g, set_between_flag(g->store, "pcr_graph_set_between_enabled", first, count, kMarkOff, on == 0));
}

int pcr_graph_set_fixed(pcr_graph* g, size_t first, size_t count, int on) {
    G_ENTER(g);
    return refuse(g, set_fixed(g->store, "pcr_graph_set_fixed", first, count, on != 0));
}

int pcr_graph_fixed(const pcr_graph* gc, size_t first, size_t count, uint8_t* fixed) {
    pcr_graph* g = const_cast<pcr_graph*>(gc);
    G_ENTER(g);
    const size_t N = g->store.n_poses();
    if (first > N || count > N - first) return gfail(g, "pcr_graph_fixed: first + count exceeds the number of poses (" + std::to_string(N) + ")");
    if (count == 0) return 0;
    if (!fixed) return gfail(g, "pcr_graph_fixed: NULL output");
    for (size_t i = 0; i < count; ++i) fixed[i] = g->store.is_fixed(first + i) ? 1 : 0;
    return 0;
}

int pcr_graph_size(const pcr_graph* g, size_t* np, size_t* n_priors, size_t* n_between) {
    if (!g) return 1;
    if (np) *np = g->store.n_poses();
    if (n_priors) *n_priors = g->store.priors.size();
    if (n_between) *n_between = g->store.betweens.size();
    return 0;
}

int pcr_graph_clear(pcr_graph* g) {
    G_ENTER(g);
    clear(g->store);
    g->dev.n_poses = 0; g->dev.ahead = false;      // the device's poses go with the store's; its tables are older by the store's own rule
    g->settled = LmSettled{};
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
    G_ENTER(g);
    const size_t N = g->store.n_poses();
    if (first > N || count > N - first) return gfail(g, "pcr_graph_poses: first + count exceeds the number of poses");
    if (count == 0) return 0;
    if (!poses16) return gfail(g, "pcr_graph_poses: NULL output");
    if (sync_host(g)) return 1;
    memcpy(poses16, &g->store.poses[16 * first], count * 16 * sizeof(double));
    return 0;
}

const double* pcr_graph_device_poses(const pcr_graph* gc, size_t* n) {
    pcr_graph* g = const_cast<pcr_graph*>(gc);
    if (n) *n = 0;
    if (!g) return nullptr;
    g->err.clear();
    if (g->host_only) { gfail(g, "pcr_graph_device_poses: a PCR_GRAPH_HOST graph has no device"); return nullptr; }
    if (g->store.n_poses() == 0) return nullptr;
    if (upload_poses(g)) return nullptr;      // (the poses alone: the factors may name poses that do not exist yet)
    if (n) *n = g->dev.n_poses;
    return g->dev.poses[g->dev.cur].as<double>();
}

// s = r^T Omega r in the linearise kernel's order, and the kernel's rho(s) and w(s) for this factor (s and 1 unless it is marked)
static double factor_rho(const Store& st, const Factor& f, const double* rr, double* s_out, double* w_out) {
    double s = 0.0;
    for (int k = 0; k < 6; ++k) {
        double w = 0.0;
        for (int m = 0; m < 6; ++m) w += f.info[k * 6 + m] * rr[m];
        s += rr[k] * w;
    }
    double rho, wk;
    gm::robust_rho_w((f.flags & kMarkRobust) ? st.robust_kind : 0, s, st.robust_delta, st.robust_delta * st.robust_delta, &rho, &wk);
    if (s_out) *s_out = s;
    if (w_out) *w_out = wk;
    return rho;
}

int pcr_graph_linearize(pcr_graph* g, double* r, double* j_from, double* j_to, double* chi2) {
    G_ENTER(g);
    if (validate(g, "pcr_graph_linearize")) return 1;
    const Store& st = g->store;
    const size_t F = st.n_factors();
    if (g->host_only) {
        std::vector<double> c(F);
        for (size_t e = 0; e < F; ++e) {
            const Factor& f = st.factor(e);
            double rr[6], Jf[36], Jt[36];
            const double* Xj = &st.poses[16 * f.to];
            gm::factor_linearize(f.from >= 0, f.from >= 0 ? &st.poses[16 * f.from] : Xj, Xj, f.z, rr, Jf, Jt);
            c[e] = (f.flags & kMarkOff) ? 0.0 : factor_rho(st, f, rr, nullptr, nullptr);
            if (r) memcpy(r + 6 * e, rr, sizeof rr);
            if (j_from) memcpy(j_from + 36 * e, Jf, sizeof Jf);
            if (j_to) memcpy(j_to + 36 * e, Jt, sizeof Jt);
        }
        if (chi2) *chi2 = fold_chi2(c);
        return 0;
    }
    Ctx c;
    if (prepare(g, false, &c)) return 1;
    if (F == 0) { if (chi2) *chi2 = 0.0; return 0; }
    const Lin& lin = c.lin[g->dev.cur];
    G_TRY(linearize_at(c, g->dev.cur));
    G_TRY(hipMemcpyAsync(g->dev.h_status, c.status, kStatusRead, hipMemcpyDeviceToHost, c.stream));
    std::vector<double> buf((6 + 72) * F);
    G_TRY(hipMemcpyAsync(buf.data(), lin.r, 6 * F * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    G_TRY(hipMemcpyAsync(buf.data() + 6 * F, lin.jf, 72 * F * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    G_TRY(hipStreamSynchronize(c.stream));
    for (size_t e = 0; e < F; ++e) {
        if (r) for (int k = 0; k < 6; ++k) r[6 * e + k] = buf[k * F + e];
        if (j_from) for (int k = 0; k < 36; ++k) j_from[36 * e + k] = buf[6 * F + k * F + e];
        if (j_to) for (int k = 0; k < 36; ++k) j_to[36 * e + k] = buf[42 * F + k * F + e];
    }
    if (chi2) *chi2 = g->dev.h_status->chi2;
    return 0;
}

int pcr_graph_between_weights(pcr_graph* g, size_t first, size_t count, double* s, double* w, uint8_t* robust, uint8_t* enabled) {
    G_ENTER(g);
    const Store& st = g->store;
    const size_t B = st.betweens.size();
    if (first > B || count > B - first)
        return gfail(g, "pcr_graph_between_weights: first + count exceeds the number of between factors (" + std::to_string(B) + ")");
    if (validate(g, "pcr_graph_between_weights")) return 1;
    for (size_t i = 0; i < count; ++i) {
        const unsigned char fl = st.betweens[first + i].flags;
        if (robust) robust[i] = (fl & kMarkRobust) ? 1 : 0;
        if (enabled) enabled[i] = (fl & kMarkOff) ? 0 : 1;
    }
    if (count == 0 || (!s && !w)) return 0;
    if (g->host_only) {
        for (size_t i = 0; i < count; ++i) {
            const Factor& f = st.betweens[first + i];
            double rr[6], Jf[36], Jt[36];
            gm::factor_linearize(true, &st.poses[16 * f.from], &st.poses[16 * f.to], f.z, rr, Jf, Jt);
            (void)factor_rho(st, f, rr, s ? s + i : nullptr, w ? w + i : nullptr);
        }
        return 0;
    }
    Ctx c;
    if (prepare(g, false, &c)) return 1;
    const Lin& lin = c.lin[g->dev.cur];
    G_TRY(linearize_at(c, g->dev.cur));
    if (s) G_TRY(hipMemcpyAsync(s, lin.s + c.P + first, count * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    if (w) G_TRY(hipMemcpyAsync(w, lin.w + c.P + first, count * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    G_TRY(hipStreamSynchronize(c.stream));
    return 0;
}

int pcr_graph_apply(pcr_graph* g, double lambda, const double* x, double* y) {
    G_ENTER(g);
    if (validate(g, "pcr_graph_apply")) return 1;
    if (g->host_only) return gfail(g, "pcr_graph_apply: a PCR_GRAPH_HOST graph has no device: the product is the solve kernel's");
    const size_t N = g->store.n_poses();
    if (N == 0) return 0;
    if (!x || !y) return gfail(g, "pcr_graph_apply: NULL vector");
    if (!std::isfinite(lambda)) return gfail(g, "pcr_graph_apply: lambda is not finite");
    Ctx c;
    if (prepare(g, false, &c)) return 1;
    G_TRY(linearize_at(c, g->dev.cur));
    G_TRY(hipMemcpyAsync(c.b.res, x, 6 * N * sizeof(double), hipMemcpyHostToDevice, c.stream));
    G_TRY(launch_apply((int)N, c.fac, c.fixed, c.lin[g->dev.cur], c.csr, lambda, c.b.res, c.b.ap, c.b.u, c.stream));
    G_TRY(hipMemcpyAsync(y, c.b.ap, 6 * N * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    G_TRY(hipStreamSynchronize(c.stream));
    return 0;
}

int pcr_graph_tree(const pcr_graph* gc, int64_t* parent, size_t n, size_t* n_tree_edges, size_t* n_other_edges) {
    pcr_graph* g = const_cast<pcr_graph*>(gc);
    G_ENTER(g);
    const size_t N = g->store.n_poses();
    if (validate(g, "pcr_graph_tree")) return 1;
    if (refuse(g, check_priors(g->store, "pcr_graph_tree"))) return 1;
    if (parent && n < N) return gfail(g, "pcr_graph_tree: parent has room for " + std::to_string(n) + " entries, the graph holds " + std::to_string(N) + " poses");
    const ForestPlan& fp = forest_of(g);
    if (parent) for (size_t p = 0; p < N; ++p) parent[p] = fp.parent[p];
    if (n_tree_edges) *n_tree_edges = fp.n_tree;
    if (n_other_edges) *n_other_edges = fp.n_other;
    return 0;
}

int pcr_graph_precondition(pcr_graph* g, double lambda, int kind, const double* r, double* z) {
    G_ENTER(g);
    if (kind != PCR_GRAPH_PRECOND_BLOCK_JACOBI && kind != PCR_GRAPH_PRECOND_TREE)
        return gfail(g, "pcr_graph_precondition: unknown preconditioner " + std::to_string(kind) + " (PCR_GRAPH_PRECOND_BLOCK_JACOBI = 0, PCR_GRAPH_PRECOND_TREE = 1)");
    if (validate(g, "pcr_graph_precondition")) return 1;
    if (refuse(g, check_priors(g->store, "pcr_graph_precondition"))) return 1;
    if (g->host_only) return gfail(g, "pcr_graph_precondition: a PCR_GRAPH_HOST graph has no device: the sweeps are the solve kernel's");
    const size_t N = g->store.n_poses();
    if (N == 0) return 0;
    if (!r || !z) return gfail(g, "pcr_graph_precondition: NULL vector");
    if (!(lambda >= 0.0) || !std::isfinite(lambda)) return gfail(g, "pcr_graph_precondition: lambda must be finite and not negative");
    const bool tree = kind == PCR_GRAPH_PRECOND_TREE;
    Ctx c;
    if (prepare(g, tree, &c)) return 1;
    Status* h = g->dev.h_status;
    G_TRY(linearize_at(c, g->dev.cur));
    G_TRY(hipMemcpyAsync(c.b.res, r, 6 * N * sizeof(double), hipMemcpyHostToDevice, c.stream));
    G_TRY(launch_precondition((int)N, c.fac, c.fixed, c.lin[g->dev.cur], c.csr, tree ? &c.tree : nullptr, lambda, c.b, c.precond_flag, c.stream));
    G_TRY(hipMemcpyAsync(z, c.b.z, 6 * N * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    G_TRY(hipMemcpyAsync(&h->precond_flag, c.precond_flag, sizeof(int), hipMemcpyDeviceToHost, c.stream));
    G_TRY(hipStreamSynchronize(c.stream));
    if (h->precond_flag) return gfail(g, "pcr_graph_precondition: a block of the preconditioner is not positive definite");
    return 0;
}

int pcr_graph_optimize(pcr_graph* g, const pcr_graph_params* params, pcr_graph_result* out) {
    G_ENTER(g);
    pcr_graph_params prm;
    pcr_graph_default_params(&prm);
    if (params) {
        if (params->struct_size != sizeof prm) return gfail(g, "pcr_graph_optimize: pcr_graph_params.struct_size does not match (use pcr_graph_default_params)");
        prm = *params;
    }
    if (refuse(g, check_params("pcr_graph_optimize", prm))) return 1;
    const Store& st = g->store;
    const size_t N = st.n_poses();
    if (N == 0 && st.n_factors() == 0) { if (out) *out = empty_result(); return 0; }      // an empty graph: nothing to do
    if (validate(g, "pcr_graph_optimize")) return 1;
    if (refuse(g, check_priors(st, "pcr_graph_optimize"))) return 1;
    if (g->host_only) return gfail(g, "pcr_graph_optimize: a PCR_GRAPH_HOST graph has no device (create the graph with a device ordinal, or -1)");
    if (lm_stands(g->settled, st.revision, prm)) { if (out) *out = lm_standing_result(g->settled, prm); return 0; }
    if (!has_free_pose_with_factor(st)) {      // every pose is fixed: nothing to move, chi2 is a constant and is evaluated
        Ctx c;
        if (prepare(g, false, &c)) return 1;
        pcr_graph_result res = empty_result();
        if (c.F > 0) {
            G_TRY(linearize_at(c, g->dev.cur));
            G_TRY(read_status(g, c));
            res.chi2_initial = res.chi2_final = g->dev.h_status->chi2;
        }
        res.converged = 1;
        res.lambda = prm.lambda_init;
        if (out) *out = res;
        return 0;
    }
    double last_old[16];
    if (current_pose(g, N - 1, last_old)) return 1;
    const bool tree = prm.pcg_preconditioner == PCR_GRAPH_PRECOND_TREE;
    Ctx c;
    if (prepare(g, tree, &c)) return 1;
    const long long cap64 = prm.pcg_max_iterations > 0 ? prm.pcg_max_iterations : std::max<long long>(100, 10 * (long long)N);
    const int cap = (int)std::min<long long>(cap64, 0x7fffffff);
    Device& d = g->dev;
    const Status* h = d.h_status;

    G_TRY(linearize_at(c, d.cur));
    G_TRY(read_status(g, c));
    if (!std::isfinite(h->chi2)) return gfail(g, "pcr_graph_optimize: chi2 of the initial estimates is not finite");
    LmState lm;
    lm_init(&lm, prm, h->chi2);
    while (lm_wants_trial(lm)) {
        const int cur = d.cur, trial = cur ^ 1;
        if (tree) G_TRY(launch_solve_tree((int)N, c.fac, c.fixed, c.lin[cur], c.csr, c.tree, lm.lambda, cap, prm.pcg_rel_tol, c.b, c.status, c.stream));
        else G_TRY(launch_solve((int)N, c.fac, c.fixed, c.lin[cur], c.csr, lm.lambda, cap, prm.pcg_rel_tol, c.b, c.status, c.stream));
        G_TRY(launch_retract((int)N, c.poses[cur], c.b.x, c.pose_fixed, c.poses[trial], c.stream));
        G_TRY(linearize_at(c, trial));
        G_TRY(read_status(g, c));
        if (lm_step(&lm, h->chi2, h->pcg_iterations, h->pcg_flag) & kLmAccept) { d.cur = trial; d.ahead = true; }      // the trial's buffers become the current ones
    }
    pcr_graph_result res = lm_result(lm);
    g->settled = lm_settle(lm, st.revision);
    if (!st.is_fixed(N - 1)) {      // (a fixed last pose did not move: delta stays the identity lm_result starts from)
        double last_new[16], inv_old[16];
        if (current_pose(g, N - 1, last_new)) return 1;
        gm::pose_inv(last_old, inv_old);
        gm::pose_mul(last_new, inv_old, res.delta);      // Backend.cpp:321: keyframes.back().pose * latest_pose.inverse()
        pcr::t2se3(res.delta);                           // :331
    }
    if (out) *out = res;
    return 0;
}

int pcr_graph_load_g2o(pcr_graph* g, const char* path) {
    G_ENTER(g);
    return refuse(g, load_g2o(g->store, "pcr_graph_load_g2o", path));
}

int pcr_graph_save_g2o(const pcr_graph* gc, const char* path) {
    pcr_graph* g = const_cast<pcr_graph*>(gc);
    G_ENTER(g);
    if (!path) return gfail(g, "pcr_graph_save_g2o: NULL path");
    if (sync_host(g)) return 1;
    return refuse(g, save_g2o(g->store, "pcr_graph_save_g2o", path));
}

}  // extern "C"
