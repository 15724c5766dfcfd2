// graph_opt.h -- the pose graph's Levenberg-Marquardt controller as a pure state machine, like ndt_opt.h, vgicp_opt.h and
// liorf_opt.h for theirs: every decision pcr_graph_optimize takes between two launches, and nothing else.  Plain C++17, no HIP header.
// pcr_graph_optimize (graph_host.hip) feeds it the 24 bytes it reads per trial step; host/graph_host_check.cpp feeds it scripted sequences, and
// tests/graph_ref.py (lm_decisions) restates it.
#pragma once
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <string>

#include "../../include/pcr_hip.h"

namespace pcr {
namespace graph_opt {

inline std::string check_params(const char* what, const pcr_graph_params& p) {
    if (!(p.lambda_factor > 1.0) || !(p.lambda_init > 0.0) || !std::isfinite(p.lambda_max) || p.max_iterations < 0 || p.pcg_max_iterations < 0 ||
        !(p.pcg_rel_tol >= 0.0) || !(p.rel_tol >= 0.0) || !(p.abs_tol >= 0.0))
        return std::string(what) + ": parameters out of range (lambda_factor > 1, lambda_init > 0, tolerances and caps >= 0)";
    if (p.pcg_preconditioner != PCR_GRAPH_PRECOND_BLOCK_JACOBI && p.pcg_preconditioner != PCR_GRAPH_PRECOND_TREE)
        return std::string(what) + ": unknown pcg_preconditioner " + std::to_string(p.pcg_preconditioner) +
               " (PCR_GRAPH_PRECOND_BLOCK_JACOBI = 0, PCR_GRAPH_PRECOND_TREE = 1)";
    return "";
}

// what a caller gets who has nothing to optimise, and what every run starts from: zeros and delta = I
inline pcr_graph_result empty_result() {
    pcr_graph_result r;
    memset(&r, 0, sizeof r);
    for (int i = 0; i < 16; ++i) r.delta[i] = (i % 5 == 0) ? 1.0 : 0.0;
    return r;
}

struct LmState {
    pcr_graph_params p;
    double chi2, lambda;      // of the current estimates; of the next solve
    pcr_graph_result res;     // in progress: iterations, accepted, pcg_iterations, pcg_capped, converged, chi2_initial
    bool stopped;
};

// what to do with the trial step that was just evaluated; kLmStop comes on top of either
enum : int { kLmReject = 0, kLmAccept = 1, kLmStop = 2 };

inline void lm_init(LmState* s, const pcr_graph_params& p, double chi2_initial) {
    s->p = p;
    s->chi2 = chi2_initial;
    s->lambda = p.lambda_init;
    s->res = empty_result();
    s->res.chi2_initial = chi2_initial;
    s->stopped = false;
}

inline bool lm_wants_trial(const LmState& s) { return !s.stopped && s.res.iterations < s.p.max_iterations; }

// One trial step was solved at s->lambda and evaluated: its chi2, the PCG's iteration count and flag (1: the cap ended it).  A chi2 that is NaN
// or +inf fails `chi2_new < chi2` and `chi2_new - chi2 < abs_tol` alike: never accepted, lambda grows, and the run ends past lambda_max.
inline int lm_step(LmState* s, double chi2_new, int pcg_iterations, int pcg_flag) {
    s->res.iterations += 1;
    s->res.pcg_iterations += pcg_iterations;
    if (pcg_flag == 1) s->res.pcg_capped += 1;
    if (chi2_new < s->chi2) {      // accepted: the trial poses and their linearisation become the current ones
        const double dec = s->chi2 - chi2_new, before = s->chi2;
        s->res.accepted += 1;
        s->lambda /= s->p.lambda_factor;
        s->chi2 = chi2_new;
        if (dec < s->p.abs_tol || dec < s->p.rel_tol * before) { s->res.converged = 1; s->stopped = true; }
        return kLmAccept | (s->stopped ? kLmStop : 0);
    }
    // rejected.  A step that could not lower chi2 and raised it by less than abs_tol: the estimate is at its minimum to that tolerance
    if (chi2_new - s->chi2 < s->p.abs_tol) { s->res.converged = 1; s->stopped = true; return kLmReject | kLmStop; }
    s->lambda *= s->p.lambda_factor;
    if (s->lambda > s->p.lambda_max) { s->stopped = true; return kLmReject | kLmStop; }
    return kLmReject;
}

// the result as it stands (delta is the caller's to fill)
inline pcr_graph_result lm_result(const LmState& s) {
    pcr_graph_result r = s.res;
    r.chi2_final = s.chi2;
    r.lambda = s.lambda;
    return r;
}

// Nothing new since an optimisation that CONVERGED under tolerances no looser than these: it stands.  One that ran out of iterations or of
// lambda, or converged under looser tolerances, goes on from the current estimates.  `revision` is the store's (graph_store.h).
struct LmSettled {
    uint64_t revision = 0;      // the store's revision the last optimisation converged at; 0: none did
    double chi2 = 0.0, rel_tol = 0.0, abs_tol = 0.0;
};
inline bool lm_stands(const LmSettled& last, uint64_t revision, const pcr_graph_params& p) {
    return last.revision == revision && p.rel_tol >= last.rel_tol && p.abs_tol >= last.abs_tol;
}
inline pcr_graph_result lm_standing_result(const LmSettled& last, const pcr_graph_params& p) {
    pcr_graph_result r = empty_result();
    r.converged = 1;
    r.chi2_initial = r.chi2_final = last.chi2;
    r.lambda = p.lambda_init;
    return r;
}
inline LmSettled lm_settle(const LmState& s, uint64_t revision) {
    LmSettled last;
    last.revision = s.res.converged ? revision : 0;
    last.chi2 = s.chi2; last.rel_tol = s.p.rel_tol; last.abs_tol = s.p.abs_tol;
    return last;
}

}  // namespace graph_opt
}  // namespace pcr
