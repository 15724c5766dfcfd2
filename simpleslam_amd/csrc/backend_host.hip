// backend_host.hip -- the back end's key-frame and loop-closure loop (pcr_backend_*).  Host code only: Backend::optimHandler's NewKFCome and LC
// events (backend/src/Backend.cpp:270-347) and LoopClosureManager::lcHandler (backend/src/LoopClosureManager.cpp:62-119) strung together over
// entry points that exist -- pcr_sc_add_keyframes, pcr_map_downsample_keyframes, pcr_graph_*, pcr_sc_query / _rank_stored, pcr_map_rank_near,
// pcr_map_update_window, pcr_scan2map_submap, pcr_fitness, pcr_map_set_poses_from_graph -- in the reference's order.  It owns a view of the
// store, a ScanContext database, the loop-closure register and the pose graph, and borrows the store.  DESIGN 4.18.

#include <chrono>
#include <cmath>

#include "handle.h"
#include "graph_math.h"
#include "backend_state.h"

using namespace pcr;

namespace {

thread_local std::string g_backend_error;      // what pcr_backend_last_error(NULL) returns

double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
enum { kContexts = 0, kDownsample, kFactors, kDetect, kWindow, kScan2map, kFitness, kOptimize, kSetPoses };      // pcr_backend_info.seconds

void identity16(double* T) { for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0; }

}  // namespace

// (struct pcr_backend: backend_state.h, shared with session_host.hip)

namespace {

int bfail(pcr_backend* be, const std::string& msg) { be->err = msg; return 1; }
int inner_fail(pcr_backend* be, const char* step, const char* msg) {
    be->failed = true;
    be->failure = std::string(step) + ": " + (msg && *msg ? msg : "failed");
    return bfail(be, be->failure);
}

pcr_sc* make_sc(pcr_backend* be) { return pcr_sc_create(be->device, &be->prm.sc); }

void start_info(pcr_backend_info* inf) {
    memset(inf, 0, sizeof *inf);
    identity16(inf->delta);
    identity16(inf->graph.delta);
}

int enter(pcr_backend* be) {
    be->err.clear();
    if (be->failed) return bfail(be, "an earlier event of this back end failed (" + be->failure + "): pcr_backend_reset starts over");
    return 0;
}

// steps 6 to 8 of an event: optimise, the poses back into the store, delta
int optimize_and_store(pcr_backend* be, pcr_backend_info* inf) {
    auto t0 = std::chrono::steady_clock::now();
    if (pcr_graph_optimize(be->graph, &be->prm.graph, &inf->graph)) return inner_fail(be, "optimize", pcr_graph_last_error(be->graph));
    inf->seconds[kOptimize] = seconds_since(t0);
    t0 = std::chrono::steady_clock::now();
    if (pcr_map_set_poses_from_graph(be->map, be->graph, 0, be->done)) return inner_fail(be, "set_poses", pcr_map_last_error(be->map));
    inf->seconds[kSetPoses] = seconds_since(t0);
    inf->optimized = 1;
    for (int i = 0; i < 16; ++i) inf->delta[i] = inf->graph.delta[i];
    return 0;
}

void finish_info(const pcr_backend* be, pcr_backend_info* inf) {
    size_t n_ctx = 0;
    (void)pcr_sc_size(be->sc, &n_ctx);
    inf->keyframes = (int64_t)be->done;
    inf->contexts = (int64_t)n_ctx;
}

// a candidate pair joins the list, or its detector bit joins the pair that is there
void propose(std::vector<pcr_backend_loop>& loops, size_t from, long long cur, long long old, int bit) {
    for (size_t i = from; i < loops.size(); ++i)
        if (loops[i].cur == cur && loops[i].old == old) { loops[i].detector |= bit; return; }
    pcr_backend_loop l;
    memset(&l, 0, sizeof l);
    l.cur = cur; l.old = old; l.detector = bit;
    l.fitness = DBL_MAX;
    loops.push_back(l);
}

}  // namespace

extern "C" {

void pcr_backend_default_params(pcr_backend_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->grid_size = 0.5;
    p->context_grid_size = 0.5;
    p->history_range = 1;
    p->fitness_threshold = 0.3;
    p->detectors = PCR_BACKEND_SC_QUERY;
    p->dist_radius = 5.0;
    p->dist_exclude_recent = -1;
    p->lc_method = PCR_VGICP;
    p->lc_between_refined = 1;
    pcr_sc_default_params(&p->sc);
    pcr_graph_default_params(&p->graph);
}

pcr_backend* pcr_backend_create(pcr_map* map, const pcr_backend_params* p) {
    auto refuse = [](const std::string& s) { g_backend_error = "pcr_backend_create: " + s; return (pcr_backend*)nullptr; };
    if (!map) return refuse("the map is NULL");
    pcr_backend_params prm;
    pcr_backend_default_params(&prm);
    if (p) prm = *p;
    if (!(prm.context_grid_size > 0)) return refuse("context_grid_size must be positive");
    if (prm.history_range < 0) return refuse("history_range must not be negative");
    if (prm.detectors & ~(PCR_BACKEND_SC_QUERY | PCR_BACKEND_SC_RANK | PCR_BACKEND_DISTANCE)) return refuse("detectors holds an unknown bit");
    if (prm.lc_method != PCR_VGICP && prm.lc_method != PCR_GICP) return refuse("lc_method must be PCR_VGICP or PCR_GICP");
    if (!(prm.dist_radius >= 0) || !std::isfinite(prm.dist_radius)) return refuse("dist_radius must be finite and not negative");
    if (prm.dist_exclude_recent < 0) prm.dist_exclude_recent = prm.sc.num_exclude_recent;
    if (prm.dist_exclude_recent < 0) return refuse("dist_exclude_recent must not be negative");
    size_t n_kf = 0;
    if (pcr_map_keyframes(map, &n_kf)) return refuse(pcr_map_last_error(map));
    pcr_backend* be = new pcr_backend;
    be->map = map; be->prm = prm; be->device = map_device(map);
    auto give_up = [&](const std::string& s) { pcr_backend_destroy(be); return refuse(s); };
    be->view = pcr_map_view(map);      // (refuses a view: the store must be a parent)
    if (!be->view) return give_up(pcr_map_last_error(map));
    be->sc = make_sc(be);
    if (!be->sc) return give_up(pcr_sc_last_error(nullptr));
    pcr_params rp;      // VgicpRegister::initForLC (VgicpRegister.cpp:21-28)
    pcr_default_params(&rp);
    rp.device = be->device;
    rp.vgicp_max_iters = 100;
    rp.vgicp_trans_eps = 1e-6;
    if (prm.lc_method == PCR_GICP) rp.gicp_max_corr_dist = 150.0;      // (acts in the non-voxel registrar only, fast_gicp_impl.hpp:136)
    be->reg = pcr_create(prm.lc_method == PCR_GICP ? "gicp" : "vgicp", &rp);
    if (!be->reg) return give_up(pcr_last_error(nullptr));
    be->graph = pcr_graph_create(be->device);
    if (!be->graph) return give_up(pcr_graph_last_error(nullptr));
    return be;
}

void pcr_backend_destroy(pcr_backend* be) {
    if (!be) return;
    if (be->reg) pcr_destroy(be->reg);      // (first: its last registration read the view's sub-map)
    if (be->view) pcr_map_destroy(be->view);
    if (be->sc) pcr_sc_destroy(be->sc);
    if (be->graph) pcr_graph_destroy(be->graph);
    delete be;
}

const char* pcr_backend_last_error(const pcr_backend* be) { return be ? be->err.c_str() : g_backend_error.c_str(); }
pcr_graph* pcr_backend_graph(pcr_backend* be) { return be ? be->graph : nullptr; }
pcr_sc* pcr_backend_sc(pcr_backend* be) { return be ? be->sc : nullptr; }
pcr_handle* pcr_backend_register(pcr_backend* be) { return be ? be->reg : nullptr; }

int pcr_backend_add_keyframes(pcr_backend* be, const int64_t* closest, size_t n_closest, pcr_backend_info* info) {
    if (!be) return 1;
    if (enter(be)) return 1;
    pcr_backend_info inf;
    start_info(&inf);
    size_t n_kf = 0;
    if (pcr_map_keyframes(be->map, &n_kf)) return bfail(be, std::string("add_keyframes: ") + pcr_map_last_error(be->map));
    if (n_kf < be->done) return bfail(be, "add_keyframes: the store holds fewer key frames than the graph (cleared behind the back end?): pcr_backend_reset starts over");
    const size_t first = be->done, count = n_kf - first;
    if (closest) {      // checked as a whole before anything changes
        if (n_closest < count) return bfail(be, "add_keyframes: closest holds " + std::to_string(n_closest) + " entries for " + std::to_string(count) + " new key frames");
        for (size_t j = 0; j < count; ++j) {
            const size_t i = first + j;
            const int64_t c = closest[j];
            if (i == 0 ? c != -1 : (c < 0 || (size_t)c >= i))
                return bfail(be, "add_keyframes: closest[" + std::to_string(j) + "] = " + std::to_string((long long)c) + " is no earlier key frame of key frame " + std::to_string(i));
        }
    }
    if (count == 0) { finish_info(be, &inf); if (info) *info = inf; return 0; }

    // 1. contexts from the RAW key frames, before saveKfs filters them (Backend.cpp:285-286)
    auto t0 = std::chrono::steady_clock::now();
    if (pcr_sc_add_keyframes(be->sc, be->map, first, count, be->prm.context_grid_size, nullptr)) return inner_fail(be, "contexts", pcr_sc_last_error(be->sc));
    inf.seconds[kContexts] = seconds_since(t0);
    // 2. saveKfs (:288): with a save directory the raw clouds go to disk first -- the filter below destroys them (MapManager.cpp:209-211)
    if (!be->save_dir.empty()) {
        std::string msg;
        if (session_write_keyframes(be->map, be->save_dir, first, &msg)) return inner_fail(be, "save", msg.c_str());
    }
    if (be->prm.grid_size > 0) {
        t0 = std::chrono::steady_clock::now();
        if (pcr_map_downsample_keyframes(be->map, first, be->prm.grid_size, nullptr)) return inner_fail(be, "downsample", pcr_map_last_error(be->map));
        inf.seconds[kDownsample] = seconds_since(t0);
    }
    // 3. - 5. addOdomFactor (:224-253)
    t0 = std::chrono::steady_clock::now();
    double info21[21];
    std::vector<double> poses(16 * count);
    for (size_t j = 0; j < count; ++j) {
        size_t n = 0;
        (void)pcr_map_keyframe(be->map, first + j, &n, nullptr, poses.data() + 16 * j);
    }
    size_t g_poses = 0, g_priors = 0, g_between = 0;
    (void)pcr_graph_size(be->graph, &g_poses, &g_priors, &g_between);
    if (g_poses == 0 && g_priors == 0 && g_between == 0) {
        (void)pcr_graph_noise(PCR_GRAPH_PRIOR, info21);
        if (pcr_graph_add_prior(be->graph, 0, poses.data(), info21)) return inner_fail(be, "factors", pcr_graph_last_error(be->graph));
    }
    if (pcr_graph_add_poses(be->graph, poses.data(), count)) return inner_fail(be, "factors", pcr_graph_last_error(be->graph));
    be->done = n_kf;
    (void)pcr_graph_noise(PCR_GRAPH_ODOM, info21);
    for (size_t j = 0; j < count; ++j) {
        const size_t i = first + j;
        if (i == 0) continue;
        const size_t from = closest ? (size_t)closest[j] : i - 1;
        if (pcr_graph_add_between_poses(be->graph, from, i, info21)) return inner_fail(be, "factors", pcr_graph_last_error(be->graph));
        inf.factors_added += 1;
    }
    inf.keyframes_added = (int32_t)count;
    inf.seconds[kFactors] = seconds_since(t0);
    // 6. - 8.
    if (optimize_and_store(be, &inf)) return 1;
    finish_info(be, &inf);
    if (info) *info = inf;
    return 0;
}

int pcr_backend_close_loops(pcr_backend* be, pcr_backend_info* info) {
    if (!be) return 1;
    if (enter(be)) return 1;
    pcr_backend_info inf;
    start_info(&inf);
    be->loops.clear();
    size_t n_ctx = 0;
    if (pcr_sc_size(be->sc, &n_ctx)) return bfail(be, "close_loops: the context database is not usable");
    const size_t first = be->lc_done, count = n_ctx > first ? n_ctx - first : 0;
    const int det = be->prm.detectors;

    // the candidates, detector by detector, then in (cur, detector bit) order
    auto t0 = std::chrono::steady_clock::now();
    std::vector<long long> by_query(count, -1), by_rank(count, -1), by_dist(count, -1);
    if (count && (det & PCR_BACKEND_SC_QUERY)) {
        for (size_t r = 0; r < count; ++r) {
            long long match = -1;
            if (pcr_sc_query(be->sc, (long long)(first + r), &match, nullptr, nullptr)) return inner_fail(be, "detect", pcr_sc_last_error(be->sc));
            by_query[r] = match;
        }
    }
    if (count && (det & PCR_BACKEND_SC_RANK)) {
        std::vector<int64_t> idx(count);
        std::vector<double> dist(count);
        std::vector<int32_t> shift(count);
        if (pcr_sc_rank_stored(be->sc, first, count, 1, idx.data(), dist.data(), shift.data())) return inner_fail(be, "detect", pcr_sc_last_error(be->sc));
        const double thres = (double)(float)be->prm.sc.dist_thres;      // (the reference keeps scDistThres as a float)
        for (size_t r = 0; r < count; ++r) by_rank[r] = (idx[r] >= 0 && !(dist[r] > thres)) ? idx[r] : -1;
    }
    if (count && (det & PCR_BACKEND_DISTANCE)) {
        std::vector<int64_t> idx(count);
        std::vector<double> d2(count);
        if (pcr_map_rank_near(be->view, first, count, be->prm.dist_exclude_recent, be->prm.dist_radius, 1, idx.data(), d2.data()))
            return inner_fail(be, "detect", pcr_map_last_error(be->view));
        for (size_t r = 0; r < count; ++r) by_dist[r] = idx[r];
    }
    for (size_t r = 0; r < count; ++r) {
        const size_t from = be->loops.size();
        if (by_query[r] >= 0) propose(be->loops, from, (long long)(first + r), by_query[r], PCR_BACKEND_SC_QUERY);
        if (by_rank[r] >= 0) propose(be->loops, from, (long long)(first + r), by_rank[r], PCR_BACKEND_SC_RANK);
        if (by_dist[r] >= 0) propose(be->loops, from, (long long)(first + r), by_dist[r], PCR_BACKEND_DISTANCE);
    }
    be->lc_done = n_ctx;      // (lc_size_ = ctb_->size(), :114)
    inf.seconds[kDetect] = seconds_since(t0);

    // lcHandler's body per candidate (:77-109)
    double loop21[21];
    (void)pcr_graph_noise(PCR_GRAPH_LOOP, loop21);
    for (pcr_backend_loop& l : be->loops) {
        inf.candidates += 1;
        double old_pose[16], cur_pose[16];
        size_t n_old = 0, n_cur = 0, n_sub = 0;
        (void)pcr_map_keyframe(be->map, (size_t)l.old, &n_old, nullptr, old_pose);
        t0 = std::chrono::steady_clock::now();
        if (pcr_map_update_window(be->view, l.old, be->prm.history_range, be->prm.context_grid_size, &n_sub)) return inner_fail(be, "window", pcr_map_last_error(be->view));
        inf.seconds[kWindow] += seconds_since(t0);
        const void* src = pcr_map_keyframe(be->map, (size_t)l.cur, &n_cur, nullptr, cur_pose);
        for (int i = 0; i < 16; ++i) l.pose[i] = cur_pose[i];
        if (!src || n_cur == 0 || n_sub == 0) continue;      // nothing to register: the record stands as not converged
        t0 = std::chrono::steady_clock::now();
        int conv = 0;
        if (pcr_scan2map_submap(be->reg, src, n_cur, 1, be->view, l.pose, &conv)) return inner_fail(be, "scan2map", pcr_last_error(be->reg));
        pcr_stats st;
        (void)pcr_get_stats(be->reg, &st);
        l.converged = conv ? 1 : 0;
        l.iterations = st.iterations;
        inf.seconds[kScan2map] += seconds_since(t0);
        t0 = std::chrono::steady_clock::now();
        l.fitness = pcr_fitness(be->reg);
        inf.seconds[kFitness] += seconds_since(t0);
        if (!(l.converged && l.fitness < be->prm.fitness_threshold)) continue;
        t0 = std::chrono::steady_clock::now();
        if (be->prm.lc_between_refined) {
            double inv_old[16], z[16];
            gm::pose_inv(old_pose, inv_old);
            gm::pose_mul(inv_old, l.pose, z);
            if (pcr_graph_add_loop(be->graph, (size_t)l.old, (size_t)l.cur, z, loop21)) return inner_fail(be, "factors", pcr_graph_last_error(be->graph));
        } else {      // the reference as written: old_pose.inverse() * cur_pose (:107), the pair of current estimates
            size_t n_between = 0;
            (void)pcr_graph_size(be->graph, nullptr, nullptr, &n_between);
            if (pcr_graph_add_between_poses(be->graph, (size_t)l.old, (size_t)l.cur, loop21) || pcr_graph_set_between_robust(be->graph, n_between, 1, 1))
                return inner_fail(be, "factors", pcr_graph_last_error(be->graph));
        }
        l.accepted = 1;
        inf.accepted += 1;
        inf.factors_added += 1;
        inf.seconds[kFactors] += seconds_since(t0);
    }
    // the LC event (Backend.cpp:293-296 and on)
    if (inf.factors_added > 0 && optimize_and_store(be, &inf)) return 1;
    finish_info(be, &inf);
    if (info) *info = inf;
    return 0;
}

int pcr_backend_loops(const pcr_backend* be, pcr_backend_loop* out, size_t capacity, size_t* n) {
    if (!be) return 1;
    pcr_backend* w = const_cast<pcr_backend*>(be);
    w->err.clear();
    if (n) *n = be->loops.size();
    if (!out) return 0;
    if (capacity < be->loops.size()) return bfail(w, "output capacity too small: the last pcr_backend_close_loops verified " + std::to_string(be->loops.size()) + " pairs");
    std::copy(be->loops.begin(), be->loops.end(), out);
    return 0;
}

int pcr_backend_step(pcr_backend* be, const int64_t* closest, size_t n_closest, pcr_backend_info* add_info, pcr_backend_info* loop_info) {
    if (pcr_backend_add_keyframes(be, closest, n_closest, add_info)) return 1;
    return pcr_backend_close_loops(be, loop_info);
}

int pcr_backend_reset(pcr_backend* be) {
    if (!be) return 1;
    be->err.clear();
    be->failed = false;
    be->loops.clear();
    be->done = 0;
    be->lc_done = 0;
    if (pcr_graph_clear(be->graph)) return bfail(be, std::string("reset: ") + pcr_graph_last_error(be->graph));
    // a context database cannot be emptied: a new one takes its place (pcr_backend_sc returns the new handle from here on)
    pcr_sc* fresh = make_sc(be);
    if (!fresh) return bfail(be, std::string("reset: ") + pcr_sc_last_error(nullptr));
    pcr_sc_destroy(be->sc);
    be->sc = fresh;
    return 0;
}

}  // extern "C"
