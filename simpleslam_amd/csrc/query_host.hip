// query_host.hip -- questions to the target a handle keeps: fitness scores at given poses (pcr_fitness_gated, pcr_fitness_batch),
// relocalisation from a coarse pose and over every key frame, exact k-NN and radius queries.

#include <stdio.h>

#include <algorithm>
#include <vector>

#include "handle.h"

using namespace pcr;
using namespace pcr::host;

namespace pcr {
namespace host {

// An index cut to a region (a target too spread out for the dense tables: its bulk, or the room around a scan) cannot tell the nearest target
// point of a source point that lies beyond a cut face, or nearer to one than to every point it holds.  Such a score is refused, never guessed.
void drop_query_index(pcr_handle* h) {
    pcr_handle::Query::Sparse& sp = h->q.sparse;
    if (sp.keys.p || sp.pts.p) (void)hipSetDevice(h->device);
    sp.keys.release(); sp.pts.release();
    sp.valid = false; sp.view = sw::View{};
    h->q.last_kind = -1; h->q.last_points = 0; h->q.last_bytes = 0;
}

std::string cut_fitness_message(double n) {
    return std::to_string((long long)n) + " source points may have their nearest target point in the part of the target the index was cut off "
           "(a target too spread out for the dense index, a stray point far from the map?): no fitness score against a cut index";
}

}  // namespace host
}  // namespace pcr

namespace {

// The index a nearest-neighbour score of the handle's current target runs on (pcr_fitness_gated, pcr_fitness_batch); it may index the
// target again.
int fit_grid_for(pcr_handle* h, const GridIndex** out) {
    *out = &h->grid;
    if (h->grid.filtered) {
        // The last pcr_scan2map (NDT, VGICP) indexed only the target points of its scan's region; a nearest-neighbour search needs them all.
        // VGICP searched its covariances on a grid of its own that holds every point (pcr_fitness answers from it too).  Otherwise a target
        // that came in as a HOST buffer still lies in this handle's staging copy and is indexed again, in full; a device buffer is the
        // caller's and may be gone.
        const bool staged = h->tgt_ptr == h->tgt_stage.as<float>() && h->tgt_n;
        if (h->method == kVgicp && h->cov_l1.valid && !h->cov_l1.filtered) {
            *out = &h->cov_l1;
        } else if (h->method == kVgicp && staged) {
            // (cov_l1 is the search grid of the next preparation's covariances: it is built again there, whatever it holds)
            const double scale = h->cov_scale_hint >= 1.3 ? h->cov_scale_hint : 1.0;
            if (settle_grid(h, h->cov_l1, h->tgt_ptr, h->tgt_n, h->tgt_stride, h->prm.vgicp_resolution * scale, 0, nullptr)) return 1;
            *out = &h->cov_l1;
        } else if (h->method == kNdt && staged) {
            h->target_ready = false;
            if (settle_grid(h, h->grid, h->tgt_ptr, h->tgt_n, h->tgt_stride, (double)(float)h->prm.ndt_resolution, 1)) return 1;
        } else if (h->method == kVgicp) {
            return fail(h, "the voxel lattice of the last pcr_scan2map holds the scan's region only (pcr_stats.region_index), its search grid does not hold "
                           "every point either, and the target was a device buffer: call pcr_set_target, or set pcr_params.full_target, before asking for "
                           "a fitness score against it");
        } else {
            return fail(h, "the target index of the last pcr_scan2map holds the scan's region only (pcr_stats.region_index) and the target was a device buffer: "
                           "call pcr_set_target, or set pcr_params.full_target, before asking for a fitness score against it");
        }
    }
    return 0;
}

int sparse_index_for(pcr_handle* h, const char* who);      // (below, with the queries)

// pcr_query_index_info after a score or a query: the index that answered
void note_dense_index(pcr_handle* h, const GridIndex& g) {
    h->q.last_kind = PCR_QUERY_INDEX_DENSE; h->q.last_points = g.n_points;
    h->q.last_bytes = g.sorted.cap + g.cell_start.cap + g.header.cap;
}
void note_sparse_index(pcr_handle* h) {
    h->q.last_kind = PCR_QUERY_INDEX_SPARSE; h->q.last_points = h->q.sparse.view.n;
    h->q.last_bytes = h->q.sparse.keys.cap + h->q.sparse.pts.cap;
}

// The sparse index for a score.  n_viol > 0: the fall-back of a score the cut dense index refused for that many points; an index that cannot be had
// (the target was a caller's device buffer, a key of more than 63 bits) then leaves the refusal standing, with its own reason behind it.
int sparse_index_for_score(pcr_handle* h, const char* who, double n_viol) {
    if (!sparse_index_for(h, who)) return 0;
    if (n_viol > 0) h->err = cut_fitness_message(n_viol) + "; and the sparse index, which holds every point, cannot be had: " + h->err;
    return 1;
}

}  // namespace

namespace pcr {
namespace host {

int sparse_fitness_run(pcr_handle* h, const char* who, double n_viol, const float* d_src, size_t n_src, size_t stride_floats, const double pose[16],
                       double max_sq) {
    if (sparse_index_for_score(h, who, n_viol) || ensure_out32(h)) return 1;
    h->seq += 1.0;
    H_TRY(sparse_fitness_launch(h->q.sparse.view, d_src, n_src, stride_floats, pose, max_sq, h->vg_partials.as<double>(), h->out32.dev, h->stream, h->seq));
    if (wait_result(h, &h->out32.host[31], h->seq)) return 1;
    note_sparse_index(h);
    return 0;
}

}  // namespace host
}  // namespace pcr

extern "C" {

int pcr_fitness_gated(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device, const double pose[16], double max_sq,
                      double* score, int64_t* n_in) {
    if (!h) return 1;
    h->err.clear();
    if (!pose || !score) return fail(h, "pose or score is NULL");
    if (n_src && !src) return fail(h, "NULL cloud with nonzero size");
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    if (!h->have_target || !h->grid.valid) return fail(h, "no target: register a scan or call pcr_set_target first");
    if (n_src > kMaxPoints) return fail(h, "source cloud too large");
    const float* d_src = (const float*)src;
    // the score as read from h->out32.host, whichever index left it there
    auto answer = [&]() {
        const double cnt = h->out32.host[1];
        *score = cnt > 0 ? h->out32.host[0] / cnt : -1.0;      // align.cpp:56-59
        if (n_in) *n_in = (int64_t)cnt;
    };
    if (scores_on_sparse(h)) {
        if (!on_device && stage_host(h, &h->src_stage, src, n_src, stride_bytes, &d_src)) return 1;
        if (sparse_fitness_run(h, "pcr_fitness_gated", 0.0, d_src, n_src, stride_bytes / 4, pose, max_sq)) return 1;
        answer();
        return 0;
    }
    const GridIndex* fit_grid = nullptr;
    if (fit_grid_for(h, &fit_grid)) return 1;
    if (!on_device && stage_host(h, &h->src_stage, src, n_src, stride_bytes, &d_src)) return 1;
    if (ensure_out32(h)) return 1;
    FitTile ft;
    memset(&ft, 0, sizeof ft);
    if (h->use_tile) {
        ft.use = 1;
        for (int d = 0; d < 3; ++d) { ft.lo[d] = h->tile_lo[d]; ft.hi[d] = h->tile_hi[d]; ft.ext_lo[d] = -1e300; ft.ext_hi[d] = 1e300; }
        if (h->have_halo) shard_extent(h, ft.ext_lo, ft.ext_hi);
    }
    h->seq += 1.0;
    H_TRY(fitness_launch(*fit_grid, d_src, n_src, stride_bytes / 4, pose, max_sq, h->vg_partials.as<double>(), h->out32.dev, h->stream, h->seq,
                         h->use_tile ? &ft : nullptr));
    if (wait_result(h, &h->out32.host[31], h->seq)) return 1;
    if (sharded(h) && ranks_allreduce(h, h->out32.host, 3)) return 1;
    answer();
    if (h->use_tile && h->out32.host[2] > 0) return fail(h, "sharded fitness: a source point's nearest map point may lie beyond this rank's halo");
    if (h->out32.host[2] > 0) {
        // the index was cut and a nearest neighbour may lie in what it left out: the sparse index holds every point (a sharded handle has none)
        *score = -1.0; if (n_in) *n_in = 0;
        if (sharded(h)) return fail(h, cut_fitness_message(h->out32.host[2]));
        if (sparse_fitness_run(h, "pcr_fitness_gated", h->out32.host[2], d_src, n_src, stride_bytes / 4, pose, max_sq)) return 1;
        answer();
        return 0;
    }
    note_dense_index(h, *fit_grid);
    return 0;
}

}  // extern "C"

// ---- relocalisation from a coarse pose (pcr_fitness_batch, pcr_reloc_hypotheses, pcr_relocalize) ----------------------------------------

namespace {

// The lattice's half-widths in steps and its size, or a message.
int reloc_dims(const pcr_reloc_params* p, long long* nx, long long* nk, size_t* K, std::string* err) {
    if (!p) { *err = "pcr_reloc_params is NULL"; return 1; }
    if (p->struct_size != sizeof(pcr_reloc_params)) { *err = "pcr_reloc_params.struct_size mismatch (start from pcr_reloc_default_params)"; return 1; }
    if (!(p->xy_range >= 0.0) || !(p->yaw_range >= 0.0) || !std::isfinite(p->xy_range) || !std::isfinite(p->yaw_range)) {
        *err = "xy_range and yaw_range must be finite and >= 0"; return 1;
    }
    if (p->xy_range > 0.0 && !(p->xy_step > 0.0)) { *err = "xy_step must be > 0 when xy_range is not 0"; return 1; }
    if (p->yaw_range > 0.0 && !(p->yaw_step > 0.0)) { *err = "yaw_step must be > 0 when yaw_range is not 0"; return 1; }
    if (p->refine_top < 1) { *err = "refine_top must be >= 1"; return 1; }
    if (std::isnan(p->max_sq)) { *err = "max_sq is NaN"; return 1; }
    const double fx = p->xy_range > 0.0 ? floor(p->xy_range / p->xy_step + 1e-9) : 0.0;
    const double fk = p->yaw_range > 0.0 ? floor(p->yaw_range / p->yaw_step + 1e-9) : 0.0;
    const double k = (2.0 * fx + 1.0) * (2.0 * fx + 1.0) * (2.0 * fk + 1.0);
    if (!(k <= (double)PCR_RELOC_MAX_POSES)) {
        *err = "the lattice has " + std::to_string(k) + " hypotheses, more than PCR_RELOC_MAX_POSES (" + std::to_string(PCR_RELOC_MAX_POSES) + ")";
        return 1;
    }
    *nx = (long long)fx; *nk = (long long)fk; *K = (size_t)k;
    return 0;
}

// Pose of hypothesis number hyp: translation t_c + (i step, j step, 0), rotation Rz(k yaw_step) R_c, row by row.
void reloc_pose(const double C[16], const pcr_reloc_params* p, long long nx, long long nk, size_t hyp, double out[16]) {
    const long long w = 2 * nx + 1;
    const long long i = (long long)(hyp % (size_t)w) - nx, j = (long long)((hyp / (size_t)w) % (size_t)w) - nx, k = (long long)(hyp / (size_t)(w * w)) - nk;
    const double a = (double)k * p->yaw_step, c = cos(a), s = sin(a);
    for (int col = 0; col < 4; ++col) {      // column-major: entry (row, col) at col * 4 + row
        const double r0 = C[col * 4], r1 = C[col * 4 + 1];
        out[col * 4] = c * r0 - s * r1;
        out[col * 4 + 1] = s * r0 + c * r1;
        out[col * 4 + 2] = C[col * 4 + 2];
        out[col * 4 + 3] = C[col * 4 + 3];
    }
    out[12] = C[12] + (double)i * p->xy_step;
    out[13] = C[13] + (double)j * p->xy_step;
    out[14] = C[14];
}

// The points scored per pose are capped at PCR_BATCH_MAX_POINTS (2^26 = 2^18 chunks of 256): with at least 8 poses per launch the
// [pose][chunk] partials then stay within kPartMax = 2^21 entries (32 MB).
int batch_points_check(pcr_handle* h, size_t n_src, size_t score_points) {
    const size_t m = score_points == 0 || score_points >= n_src ? n_src : score_points;
    if (m > PCR_BATCH_MAX_POINTS)
        return fail(h, "pcr_fitness_batch scores at most PCR_BATCH_MAX_POINTS (" + std::to_string(PCR_BATCH_MAX_POINTS) + ") points per pose, " +
                       std::to_string(m) + " were asked for: set score_points");
    return 0;
}

// One pass of pcr_fitness_batch over the poses which[0 .. count) (nullptr: poses 0 .. count - 1), in groups whose partials stay within kPartMax
// entries: on the dense index `grid`, or on the handle's sparse index (grid = nullptr).  A pose the dense kernel cannot answer (a cut index) gets
// (-1, -1) and is listed in *refused.
int fitness_batch_pass(pcr_handle* h, const GridIndex* grid, const float* d_src, size_t n_src, size_t stride_floats, size_t m, const double* poses,
                       const size_t* which, size_t count, double max_sq, double* scores, int64_t* n_in, std::vector<size_t>* refused) {
    static constexpr size_t kPartMax = size_t(1) << 21, kGroupMax = 16384;
    const size_t chunks = std::max<size_t>((m + 255) / 256, 1);      // <= 2^18
    const size_t group = std::min(kGroupMax, kPartMax / chunks / 8 * 8);      // >= 8: group x chunks <= kPartMax
    std::vector<float> pf;
    std::vector<RelocSum> sums;
    for (size_t k0 = 0; k0 < count; k0 += group) {
        const size_t g = std::min(group, count - k0);
        pf.assign(g * 16, 0.f);
        for (size_t q = 0; q < g; ++q) {
            const double* P = poses + (which ? which[k0 + q] : k0 + q) * 16;
            for (int e = 0; e < 16; ++e) pf[q * 16 + e] = (float)P[e];
        }
        sums.resize(g);
        H_TRY(h->q.rl_poses.reserve(g * 16 * sizeof(float)));
        H_TRY(h->q.rl_part.reserve(g * chunks * sizeof(RelocPart)));
        H_TRY(h->q.rl_out.reserve(g * sizeof(RelocSum)));
        H_TRY(hipMemcpyAsync(h->q.rl_poses.p, pf.data(), g * 16 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        if (grid) H_TRY(fitness_batch_launch(*grid, d_src, n_src, stride_floats, m, h->q.rl_poses.as<float>(), g, max_sq, h->q.rl_part.as<RelocPart>(),
                                             h->q.rl_out.as<RelocSum>(), h->stream));
        else H_TRY(sparse_fitness_batch_launch(h->q.sparse.view, d_src, n_src, stride_floats, m, h->q.rl_poses.as<float>(), g, max_sq,
                                               h->q.rl_part.as<RelocPart>(), h->q.rl_out.as<RelocSum>(), h->stream));
        H_TRY(hipMemcpyAsync(sums.data(), h->q.rl_out.p, g * sizeof(RelocSum), hipMemcpyDeviceToHost, h->stream));
        H_TRY(hipStreamSynchronize(h->stream));
        for (size_t q = 0; q < g; ++q) {
            const RelocSum& r = sums[q];
            const size_t at = which ? which[k0 + q] : k0 + q;
            if (r.viol > 0) { scores[at] = -1.0; n_in[at] = -1; refused->push_back(at); continue; }
            const double cnt = (double)r.cnt;
            scores[at] = cnt > 0 ? r.sum / cnt : -1.0;
            n_in[at] = (int64_t)r.cnt;
        }
    }
    return 0;
}

// pcr_fitness_batch on a device source (arguments checked).  grid: the dense index (score_grid_for), every pose scored on it as ever, and exactly
// the poses it refuses -- a cut index, a nearest neighbour that may lie in what was cut off -- scored again on the sparse index, which holds every
// point; where that index cannot be had they keep (-1, -1), as pcr_fitness_gated keeps its refusal.  grid = nullptr (pcr_params.query_index =
// SPARSE): every pose on the sparse index.
int fitness_batch_run(pcr_handle* h, const GridIndex* grid, const float* d_src, size_t n_src, size_t stride_floats, const double* poses, size_t K,
                      double max_sq, size_t score_points, double* scores, int64_t* n_in) {
    const size_t m = score_points == 0 || score_points >= n_src ? n_src : score_points;
    if (batch_points_check(h, n_src, score_points)) return 1;
    std::vector<size_t> refused, none;
    if (grid) {
        if (fitness_batch_pass(h, grid, d_src, n_src, stride_floats, m, poses, nullptr, K, max_sq, scores, n_in, &refused)) return 1;
        note_dense_index(h, *grid);
        if (refused.empty()) return 0;
        if (sparse_index_for(h, "pcr_fitness_batch")) { h->err.clear(); return 0; }
    } else if (sparse_index_for(h, "pcr_fitness_batch")) {
        return 1;
    }
    if (fitness_batch_pass(h, nullptr, d_src, n_src, stride_floats, m, poses, grid ? refused.data() : nullptr, grid ? refused.size() : K, max_sq, scores,
                           n_in, &none)) return 1;
    note_sparse_index(h);
    return 0;
}

// The index the scores of pcr_fitness_batch and of relocalisation run on: the dense one (fit_grid_for), or none (*out = nullptr) where
// pcr_params.query_index sends every score to the sparse index
int score_grid_for(pcr_handle* h, const GridIndex** out) {
    *out = nullptr;
    return scores_on_sparse(h) ? 0 : fit_grid_for(h, out);
}

int batch_preconditions(pcr_handle* h, size_t n_src, size_t stride_bytes) {
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    if (sharded(h)) return fail(h, "pcr_fitness_batch / pcr_relocalize do not serve sharded handles");
    if (h->use_tile) return fail(h, "pcr_fitness_batch / pcr_relocalize do not serve a handle with a query tile (pcr_set_query_tile)");
    if (!h->have_target || !h->grid.valid) return fail(h, "no target: register a scan or call pcr_set_target first");
    if (n_src > kMaxPoints) return fail(h, "source cloud too large");
    return 0;
}

// pcr_relocalize step 2: hypotheses 0 .. K-1 of one lattice with a point in the gate, ranked by (-n_in, score, h); refused ones (n_in = -1)
// and those with nothing in the gate are not ranked
std::vector<size_t> reloc_rank(const double* score, const int64_t* nin, size_t K) {
    std::vector<size_t> rank;
    for (size_t q = 0; q < K; ++q) if (nin[q] > 0) rank.push_back(q);
    std::sort(rank.begin(), rank.end(), [&](size_t a, size_t b) {
        if (nin[a] != nin[b]) return nin[a] > nin[b];
        if (score[a] != score[b]) return score[a] < score[b];
        return a < b;
    });
    return rank;
}

// (i, j, k) lattice coordinates of hypothesis q, each counted from 0
void reloc_ijk(size_t q, long long nx, long long* o) {
    const long long w = 2 * nx + 1;
    o[0] = (long long)(q % (size_t)w); o[1] = (long long)((q / (size_t)w) % (size_t)w); o[2] = (long long)(q / (size_t)(w * w));
}

// pcr_relocalize step 3: down the ranking, a hypothesis is taken unless one taken already lies within one step of it in each of i, j and k
std::vector<size_t> reloc_distinct(const std::vector<size_t>& rank, long long nx, int32_t refine_top) {
    std::vector<size_t> taken;
    for (size_t q : rank) {
        if (taken.size() >= (size_t)refine_top) break;
        long long a[3], b[3];
        reloc_ijk(q, nx, a);
        bool near = false;
        for (size_t t : taken) { reloc_ijk(t, nx, b); near = near || (llabs(a[0] - b[0]) <= 1 && llabs(a[1] - b[1]) <= 1 && llabs(a[2] - b[2]) <= 1); }
        if (!near) taken.push_back(q);
    }
    return taken;
}

// pcr_relocalize step 5: the candidate of hypothesis `hyp` (its pose, coarse score) refined by pcr_align from that pose.  On failure: the message.
int reloc_refine(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_bytes, size_t hyp, const double pose[16], double coarse_score,
                 int64_t coarse_n_in, pcr_reloc_candidate& o, std::string* why) {
    memset(&o, 0, sizeof o);
    o.hypothesis = (int64_t)hyp;
    o.coarse_n_in = coarse_n_in;
    o.coarse_score = coarse_score;
    memcpy(o.pose, pose, sizeof o.pose);
    int conv = 0;
    if (pcr_align(h, d_src, n_src, stride_bytes, 1, o.pose, &conv)) { *why = h->err; return 1; }
    o.converged = conv;
    return 0;
}

// pcr_relocalize step 6: the refined poses scored on the whole source in one pass; *best = the first by (-n_in, score, candidate order),
// *any = false when none has a point in the gate (*best is then left alone)
int reloc_choose(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_bytes, double max_sq, pcr_reloc_candidate* const* cands, size_t nc,
                 size_t* best, bool* any) {
    std::vector<double> refined(nc * 16), fs(nc);
    std::vector<int64_t> fn(nc);
    for (size_t c = 0; c < nc; ++c) memcpy(&refined[c * 16], cands[c]->pose, 16 * sizeof(double));
    const GridIndex* fit_grid = nullptr;
    if (score_grid_for(h, &fit_grid)) return 1;
    if (fitness_batch_run(h, fit_grid, d_src, n_src, stride_bytes / 4, refined.data(), nc, max_sq, 0, fs.data(), fn.data())) return 1;
    *any = false;
    for (size_t c = 0; c < nc; ++c) {
        cands[c]->n_in = fn[c];
        cands[c]->score = fs[c];
        if (fn[c] <= 0) continue;
        if (!*any || fn[c] > fn[*best] || (fn[c] == fn[*best] && fs[c] < fs[*best])) { *best = c; *any = true; }
    }
    return 0;
}

// pcr_relocalize step 7, the handle's side: pcr_fitness() evaluates the pose of the handle's last alignment (VGICP: fit_pose, kept by
// run_vgicp); that was the last candidate's, so it is pointed at the chosen one -- the same scan, the same target: what a fresh pcr_align
// from the chosen hypothesis leaves
void reloc_point_fitness_at(pcr_handle* h, const double pose[16]) {
    if (h->fit_pending) { memcpy(h->fit_pose, pose, sizeof h->fit_pose); h->fitness = DBL_MAX; }
}

// exactly `bytes` of device memory (DeviceBuf::reserve doubles, for buffers that grow; the sparse index is built once per target)
hipError_t reserve_exact(DeviceBuf& b, size_t bytes) {
    if (b.p && b.cap == bytes) return hipSuccess;
    b.release();
    const hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) { b.p = nullptr; return e; }
    b.cap = bytes;
    return hipSuccess;
}

// The sparse index of the kept target, built when the handle has none: from the handle's own copy of the target's points (pcr_set_target's, or the
// staged host target of pcr_scan2map) -- a caller's device buffer may be gone by now.  One synchronisation; the sort's scratch is freed on return.
int sparse_index_for(pcr_handle* h, const char* who) {
    pcr_handle::Query::Sparse& sp = h->q.sparse;
    if (sp.valid) return 0;
    if (h->tgt_n && h->tgt_ptr != h->tgt_stage.as<float>())      // (a target of no points is nobody's buffer: its index is empty)
        return fail(h, std::string(who) + ": the sparse index is built from the handle's own copy of the target, and this target was a device buffer of the caller's "
                       "(pcr_scan2map_device, pcr_scan2map_submap) that may be gone: call pcr_set_target");
    const size_t n = h->tgt_n;
    if (n > kMaxPoints) return fail(h, std::string(who) + ": target too large");
    DeviceBuf hdr, key[2], row[2], hist;
    H_TRY(hdr.reserve(256));
    for (int i = 0; i < 2; ++i) { H_TRY(key[i].reserve((n + 1) * sizeof(unsigned long long))); H_TRY(row[i].reserve((n + 1) * sizeof(uint32_t))); }
    H_TRY(hist.reserve(key_sort_hist_bytes(n)));
    H_TRY(reserve_exact(sp.keys, (n ? n : 1) * sizeof(unsigned long long)));
    H_TRY(reserve_exact(sp.pts, (n ? n : 1) * sizeof(sw::Point)));
    H_TRY(sp.ret.ensure());
    SiBuffers b;
    b.hdr = hdr.p; b.hist = hist.as<uint32_t>();
    for (int i = 0; i < 2; ++i) { b.key[i] = key[i].as<unsigned long long>(); b.row[i] = row[i].as<uint32_t>(); }
    H_TRY(sparse_index_build_launch(b, h->tgt_ptr, h->tgt_stride, n, sp.keys.as<unsigned long long>(), sp.pts.as<sw::Point>(), sp.ret.dev, h->stream));
    H_TRY(hipStreamSynchronize(h->stream));
    const SiResult r = *sp.ret.host;
    if (r.lay.refused) {
        char ext[160];
        snprintf(ext, sizeof ext, "%.6g x %.6g x %.6g", r.lay.extd[0], r.lay.extd[1], r.lay.extd[2]);
        sp.keys.release(); sp.pts.release();
        return fail(h, std::string(who) + (r.lay.refused == sw::kRefusedBits
                           ? ": the sparse index's cell key needs " + std::to_string(r.lay.b[0] + r.lay.b[1] + r.lay.b[2]) + " bits, more than 63"
                           : std::string(": a cell number of the sparse index leaves the 62-bit range")) +
                       ": extents " + ext + " cells of " + std::to_string(kSparseCell) + " m (x, y, z): refused (a stray point far from the map?)");
    }
    sw::View v;
    v.keys = sp.keys.as<unsigned long long>(); v.pts = sp.pts.as<sw::Point>();
    v.n = r.kept; v.b0 = r.lay.b[0]; v.b1 = r.lay.b[1]; v.b2 = r.lay.b[2];
    for (int a = 0; a < 3; ++a) { v.lo[a] = r.lay.lo[a]; v.ext[a] = r.lay.ext[a]; }
    v.cell = kSparseCell;
    sp.view = v; sp.valid = true;
    return 0;
}

// pcr_knn / pcr_radius_search: the index that answers (pcr_params.query_index).  The dense one: the full index of the kept target (prepared in full
// first, as pcr_relocalize does), its header checked on the host; *grid = nullptr: the sparse one (h->q.sparse.view), for a target whose dense
// index was cut to the bulk of the cloud, or when the caller asks for it.
int query_index_for(pcr_handle* h, const char* who, size_t n_q, size_t stride_bytes, const GridIndex** grid) {
    *grid = nullptr;
    if (!h->have_target || !h->grid.valid) return fail(h, std::string(who) + ": no kept target: call pcr_set_target first");
    if (batch_preconditions(h, n_q, stride_bytes)) { h->err = std::string(who) + ": " + h->err; return 1; }
    if (h->prm.query_index != PCR_QUERY_INDEX_SPARSE) {
        if (ensure_full_target(h)) return 1;
        if (fit_grid_for(h, grid)) return 1;
        GridHeader hdr;
        H_TRY(hipMemcpyAsync(&hdr, (*grid)->header.p, sizeof hdr, hipMemcpyDeviceToHost, h->stream));
        H_TRY(hipStreamSynchronize(h->stream));
        if (hdr.overflow || hdr.stale || (*grid)->filtered) return fail(h, std::string(who) + ": the target index is not complete (internal)");
        if (!hdr.clamped) { note_dense_index(h, **grid); return 0; }
        *grid = nullptr;      // the box cannot be tabulated and the index was cut to the bulk of the cloud: an exact query needs every point
    }
    if (sparse_index_for(h, who)) return 1;
    note_sparse_index(h);
    return 0;
}

}  // namespace

extern "C" {

int pcr_fitness_batch(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device, const double* poses, size_t K,
                      double max_sq, size_t score_points, double* scores, int64_t* n_in) {
    if (!h) return 1;
    h->err.clear();
    if (K > PCR_RELOC_MAX_POSES) return fail(h, "K = " + std::to_string(K) + " is more than PCR_RELOC_MAX_POSES (" + std::to_string(PCR_RELOC_MAX_POSES) + ")");
    if (K && (!poses || !scores || !n_in)) return fail(h, "poses, scores or n_in is NULL");
    if (n_src && !src) return fail(h, "NULL cloud with nonzero size");
    if (batch_preconditions(h, n_src, stride_bytes)) return 1;
    const GridIndex* fit_grid = nullptr;
    if (score_grid_for(h, &fit_grid)) return 1;
    if (K == 0) return 0;
    if (batch_points_check(h, n_src, score_points)) return 1;
    const float* d_src = (const float*)src;
    if (!on_device && stage_host(h, &h->src_stage, src, n_src, stride_bytes, &d_src)) return 1;
    return fitness_batch_run(h, fit_grid, d_src, n_src, stride_bytes / 4, poses, K, max_sq, score_points, scores, n_in);
}

int pcr_knn(pcr_handle* h, const void* queries, size_t n_q, size_t stride_bytes, int on_device, int k, int64_t* idx, double* d2) {
    if (!h) return 1;
    h->err.clear();
    if (k < 1 || k > PCR_KNN_MAX_K) return fail(h, "pcr_knn: k = " + std::to_string(k) + " is outside 1 .. PCR_KNN_MAX_K (" + std::to_string(PCR_KNN_MAX_K) + ")");
    if (n_q && (!queries || !idx || !d2)) return fail(h, "pcr_knn: queries, idx or d2 is NULL");
    const GridIndex* grid = nullptr;
    if (query_index_for(h, "pcr_knn", n_q, stride_bytes, &grid)) return 1;
    if (n_q == 0) return 0;
    const float* d_q = (const float*)queries;
    if (!on_device && stage_host(h, &h->src_stage, queries, n_q, stride_bytes, &d_q)) return 1;
    // in chunks: the results of 2^20 queries at k = 32 are 512 MB
    const size_t chunk = size_t(1) << 20;
    H_TRY(h->q.idx.reserve(std::min(n_q, chunk) * (size_t)k * sizeof(int64_t)));
    H_TRY(h->q.d2.reserve(std::min(n_q, chunk) * (size_t)k * sizeof(double)));
    for (size_t q0 = 0; q0 < n_q; q0 += chunk) {
        const size_t m = std::min(chunk, n_q - q0);
        if (grid) H_TRY(knn_query_launch(*grid, d_q + q0 * (stride_bytes / 4), m, stride_bytes / 4, k, h->q.idx.as<int64_t>(), h->q.d2.as<double>(), h->stream));
        else H_TRY(knn_sparse_launch(h->q.sparse.view, d_q + q0 * (stride_bytes / 4), m, stride_bytes / 4, k, h->q.idx.as<int64_t>(), h->q.d2.as<double>(), h->stream));
        H_TRY(hipMemcpyAsync(idx + q0 * (size_t)k, h->q.idx.p, m * (size_t)k * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        H_TRY(hipMemcpyAsync(d2 + q0 * (size_t)k, h->q.d2.p, m * (size_t)k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        H_TRY(hipStreamSynchronize(h->stream));
    }
    return 0;
}

int pcr_radius_search(pcr_handle* h, const void* queries, size_t n_q, size_t stride_bytes, int on_device, double radius, int sorted,
                      size_t capacity, uint64_t* offsets, int64_t* idx, double* d2, size_t* n_total) {
    if (!h) return 1;
    h->err.clear();
    if (!(radius > 0.0) || !std::isfinite(radius)) return fail(h, "pcr_radius_search: radius must be finite and > 0");
    if (!offsets || !n_total) return fail(h, "pcr_radius_search: offsets or n_total is NULL");
    if (n_q && !queries) return fail(h, "pcr_radius_search: queries is NULL");
    if (capacity && (!idx || !d2)) return fail(h, "pcr_radius_search: idx or d2 is NULL with a nonzero capacity");
    if (n_q > 0x7fffffffull) return fail(h, "pcr_radius_search: more than 2^31 - 1 queries in one call");
    const GridIndex* grid = nullptr;
    if (query_index_for(h, "pcr_radius_search", n_q, stride_bytes, &grid)) return 1;
    const float* d_q = (const float*)queries;
    if (!on_device && n_q && stage_host(h, &h->src_stage, queries, n_q, stride_bytes, &d_q)) return 1;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "offsets are 64-bit");
    H_TRY(h->q.counts.reserve((n_q + 1) * sizeof(uint32_t)));
    H_TRY(h->q.offsets.reserve((n_q + 1) * sizeof(uint64_t)));
    if (grid) H_TRY(radius_count_launch(*grid, d_q, n_q, stride_bytes / 4, radius, h->q.counts.as<uint32_t>(), h->q.offsets.as<unsigned long long>(), h->stream));
    else H_TRY(radius_sparse_count_launch(h->q.sparse.view, d_q, n_q, stride_bytes / 4, radius, h->q.counts.as<uint32_t>(), h->q.offsets.as<unsigned long long>(), h->stream));
    H_TRY(hipMemcpyAsync(offsets, h->q.offsets.p, (n_q + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    H_TRY(hipStreamSynchronize(h->stream));
    const uint64_t total = offsets[n_q];
    *n_total = (size_t)total;
    if (total > (uint64_t)capacity)
        return fail(h, "pcr_radius_search: the arrays hold " + std::to_string(capacity) + " entries, the search has " + std::to_string(total) +
                       " results: size idx and d2 for *n_total and call again");
    if (total == 0) return 0;
    const size_t t = (size_t)total;
    H_TRY(h->q.idx.reserve(t * sizeof(int64_t)));
    H_TRY(h->q.d2.reserve(t * sizeof(double)));
    if (grid) H_TRY(radius_fill_launch(*grid, d_q, n_q, stride_bytes / 4, radius, h->q.offsets.as<unsigned long long>(), h->q.idx.as<int64_t>(), h->q.d2.as<double>(), h->stream));
    else H_TRY(radius_sparse_fill_launch(h->q.sparse.view, d_q, n_q, stride_bytes / 4, radius, h->q.offsets.as<unsigned long long>(), h->q.idx.as<int64_t>(), h->q.d2.as<double>(), h->stream));
    const void *r_idx = h->q.idx.p, *r_d2 = h->q.d2.p;
    if (sorted) {
        H_TRY(h->q.idx2.reserve(t * sizeof(int64_t)));
        H_TRY(h->q.d22.reserve(t * sizeof(double)));
        H_TRY(radius_sort_launch(n_q, h->q.offsets.as<unsigned long long>(), h->q.idx.as<int64_t>(), h->q.d2.as<double>(), h->q.idx2.as<int64_t>(),
                                 h->q.d22.as<double>(), h->stream));
        r_idx = h->q.idx2.p; r_d2 = h->q.d22.p;
    }
    H_TRY(hipMemcpyAsync(idx, r_idx, t * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    H_TRY(hipMemcpyAsync(d2, r_d2, t * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    H_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int pcr_query_index_info(pcr_handle* h, int* kind, size_t* n_points, size_t* bytes) {
    if (!h) return 1;
    if (kind) *kind = h->q.last_kind;
    if (n_points) *n_points = h->q.last_points;
    if (bytes) *bytes = h->q.last_bytes;
    return 0;
}

void pcr_reloc_default_params(pcr_reloc_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->struct_size = sizeof(pcr_reloc_params);
    p->xy_range = 2.0; p->xy_step = 0.5;
    p->yaw_range = 30.0 * M_PI / 180.0; p->yaw_step = 5.0 * M_PI / 180.0;
    p->max_sq = 1.0;
    p->refine_top = 4;
    p->score_points = 4096;
}

int pcr_reloc_hypotheses(const double coarse[16], const pcr_reloc_params* p, double* poses, size_t capacity, size_t* K) {
    g_create_error.clear();
    long long nx = 0, nk = 0;
    size_t k = 0;
    if (!coarse || !K) { g_create_error = "pcr_reloc_hypotheses: coarse or K is NULL"; return 1; }
    if (reloc_dims(p, &nx, &nk, &k, &g_create_error)) { g_create_error = "pcr_reloc_hypotheses: " + g_create_error; return 1; }
    *K = k;
    if (!poses || capacity < k) {
        g_create_error = "pcr_reloc_hypotheses: the output holds " + std::to_string(poses ? capacity : 0) + " poses, the lattice has " + std::to_string(k);
        return 1;
    }
    for (size_t q = 0; q < k; ++q) reloc_pose(coarse, p, nx, nk, q, poses + q * 16);
    return 0;
}

int pcr_relocalize(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device, const pcr_reloc_params* p,
                   double pose_inout[16], int* converged, pcr_reloc_candidate* cands, size_t capacity, size_t* n_cands, size_t* chosen) {
    if (!h) return 1;
    h->err.clear();
    if (!pose_inout || !cands || !n_cands || !chosen) return fail(h, "pose_inout, cands, n_cands or chosen is NULL");
    if (n_src && !src) return fail(h, "NULL cloud with nonzero size");
    long long nx = 0, nk = 0;
    size_t K = 0;
    std::string e;
    if (reloc_dims(p, &nx, &nk, &K, &e)) return fail(h, e);
    if (capacity < (size_t)p->refine_top + 1) return fail(h, "cands holds " + std::to_string(capacity) + " candidates, refine_top + 1 = " + std::to_string(p->refine_top + 1) + " are needed");
    if (batch_preconditions(h, n_src, stride_bytes)) return 1;
    if (ensure_full_target(h)) return 1;      // (pcr_align's precondition; the coarse score then runs on the full index too)
    const float* d_src = (const float*)src;
    if (!on_device && stage_host(h, &h->q.rl_src, src, n_src, stride_bytes, &d_src)) return 1;      // once, for every step below

    // 1. the coarse score of every hypothesis on the subset
    double click[16];
    memcpy(click, pose_inout, sizeof click);
    std::vector<double> poses(K * 16), score(K);
    std::vector<int64_t> nin(K);
    for (size_t q = 0; q < K; ++q) reloc_pose(click, p, nx, nk, q, &poses[q * 16]);
    const GridIndex* fit_grid = nullptr;
    if (score_grid_for(h, &fit_grid)) return 1;
    if (fitness_batch_run(h, fit_grid, d_src, n_src, stride_bytes / 4, poses.data(), K, p->max_sq, (size_t)p->score_points, score.data(), nin.data())) return 1;
    // 2. ranked by (-n_in, score, h); refused hypotheses and those with nothing in the gate are not ranked
    const std::vector<size_t> rank = reloc_rank(score.data(), nin.data(), K);
    if (rank.empty())
        return fail(h, "relocalisation: no hypothesis has a source point within the gate (max_sq = " + std::to_string(p->max_sq) +
                       ") of the target: is the coarse pose on the map?");
    // 3. distinct winners: none within one step of another in each of i, j and k; 4. the click itself
    std::vector<size_t> taken = reloc_distinct(rank, nx, p->refine_top);
    const long long w = 2 * nx + 1;
    const size_t centre = (size_t)((nk * w + nx) * w + nx);
    if (std::find(taken.begin(), taken.end(), centre) == taken.end()) taken.push_back(centre);
    // 5. each candidate refined by pcr_align from its hypothesis pose
    const size_t nc = taken.size();
    std::vector<pcr_reloc_candidate*> cp(nc);
    for (size_t c = 0; c < nc; ++c) {
        cp[c] = &cands[c];
        std::string why;
        if (reloc_refine(h, d_src, n_src, stride_bytes, taken[c], &poses[taken[c] * 16], score[taken[c]], nin[taken[c]], cands[c], &why)) {
            *n_cands = c;
            return fail(h, "relocalisation: refining hypothesis " + std::to_string(taken[c]) + ": " + why);
        }
    }
    *n_cands = nc;
    // 6. the refined poses scored on the whole source; the first by (-n_in, score, candidate order); the click when none has a point in the gate
    size_t best = nc - 1;
    bool any = false;
    if (reloc_choose(h, d_src, n_src, stride_bytes, p->max_sq, cp.data(), nc, &best, &any)) return 1;
    if (!any) best = (size_t)(std::find(taken.begin(), taken.end(), centre) - taken.begin());
    // 7. the chosen pose
    memcpy(pose_inout, cands[best].pose, 16 * sizeof(double));
    reloc_point_fitness_at(h, cands[best].pose);
    if (converged) *converged = cands[best].converged;
    *chosen = best;
    return 0;
}

}  // extern "C"

// ---- global relocalisation (pcr_global_reloc_hypotheses, pcr_relocalize_global) ----------------------------------------------------------

namespace {

// The coarse pose of a place: kf_pose * Rz(-yaw), yaw = deg2rad<float>(6 deg * shift) exactly as pcr_sc_query forms it.  Column by column
// (c = cos(yaw), s = sin(yaw), double): col0 = c C0 - s C1, col1 = s C0 + c C1, col2 and col3 as they are.
void place_pose(const double T[16], int32_t shift, double out[16]) {
    const float yaw = (float)((double)((360.0f / 60.0f) * (float)shift) * 3.14159265358979323846 / 180.0);      // deg2rad<float>
    const double c = cos((double)yaw), s = sin((double)yaw);
    memcpy(out, T, 16 * sizeof(double));
    for (int r = 0; r < 4; ++r) {
        out[r] = c * T[r] - s * T[4 + r];
        out[4 + r] = s * T[r] + c * T[4 + r];
    }
}

int global_params_check(const pcr_global_reloc_params* p, long long* nx, long long* nk, size_t* K, std::string* err) {
    if (!p) { *err = "pcr_global_reloc_params is NULL"; return 1; }
    if (p->struct_size != sizeof(pcr_global_reloc_params)) {
        *err = "pcr_global_reloc_params.struct_size mismatch (start from pcr_global_reloc_default_params)"; return 1;
    }
    if (p->places < 1) { *err = "places must be >= 1"; return 1; }
    if (std::isnan(p->max_dist)) { *err = "max_dist is NaN"; return 1; }
    if (reloc_dims(&p->local, nx, nk, K, err)) { *err = "local lattice: " + *err; return 1; }
    return 0;
}

}  // namespace

extern "C" {

void pcr_global_reloc_default_params(pcr_global_reloc_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->struct_size = sizeof(pcr_global_reloc_params);
    p->places = 5;
    p->max_dist = DBL_MAX;
    pcr_reloc_default_params(&p->local);
    p->local.yaw_range = 9.0 * M_PI / 180.0; p->local.yaw_step = 3.0 * M_PI / 180.0;      // the yaw of a place is known to one 6-degree sector
    p->local.refine_top = 2;
}

int pcr_global_reloc_hypotheses(const double kf_pose[16], int32_t shift, const pcr_reloc_params* local, double* poses, size_t capacity, size_t* K) {
    g_create_error.clear();
    if (!kf_pose || !K) { g_create_error = "pcr_global_reloc_hypotheses: kf_pose or K is NULL"; return 1; }
    long long nx = 0, nk = 0;
    size_t k = 0;
    if (reloc_dims(local, &nx, &nk, &k, &g_create_error)) { g_create_error = "pcr_global_reloc_hypotheses: " + g_create_error; return 1; }
    *K = k;
    if (!poses || capacity < k) {
        g_create_error = "pcr_global_reloc_hypotheses: the output holds " + std::to_string(poses ? capacity : 0) + " poses, the lattice has " + std::to_string(k);
        return 1;
    }
    double coarse[16];
    place_pose(kf_pose, shift, coarse);
    for (size_t q = 0; q < k; ++q) reloc_pose(coarse, local, nx, nk, q, poses + q * 16);
    return 0;
}

int pcr_relocalize_global(pcr_handle* h, pcr_sc* sc, const double* kf_poses, size_t n_kf, const void* src, size_t n_src, size_t stride_bytes,
                          int on_device, const pcr_global_reloc_params* p, double pose_out[16], int* converged,
                          pcr_global_reloc_candidate* cands, size_t capacity, size_t* n_cands, size_t* chosen) {
    // argument errors go to the handle, or to pcr_last_error(NULL) when there is none
    auto refuse = [&](const std::string& m) { if (h) return fail(h, m); g_create_error = "pcr_relocalize_global: " + m; return 1; };
    g_create_error.clear();
    if (h) h->err.clear();
    long long nx = 0, nk = 0;
    size_t K = 0;
    std::string e;
    if (global_params_check(p, &nx, &nk, &K, &e)) return refuse(e);
    const size_t need = (size_t)p->places * (size_t)p->local.refine_top;
    if (!pose_out || !cands || !n_cands || !chosen) return refuse("pose_out, cands, n_cands or chosen is NULL");
    if (capacity < need) return refuse("cands holds " + std::to_string(capacity) + " candidates, places x refine_top = " + std::to_string(need) + " are needed");
    if (!h) return refuse("the handle is NULL");
    if (!sc) return fail(h, "sc is NULL");
    if (n_src && !src) return fail(h, "NULL cloud with nonzero size");
    size_t M = 0;
    pcr_sc_size(sc, &M);
    if (n_kf != M) return fail(h, "n_kf = " + std::to_string(n_kf) + " key-frame poses for " + std::to_string(M) + " ScanContexts: one pose per context");
    if (M && !kf_poses) return fail(h, "kf_poses is NULL");
    if (sc_device(sc) != h->device) return fail(h, "the ScanContext database lives on device " + std::to_string(sc_device(sc)) + ", the handle on " + std::to_string(h->device));
    if (batch_preconditions(h, n_src, stride_bytes)) return 1;
    if (batch_points_check(h, n_src, 0)) return 1;      // (the final score covers every point)

    // 1. the places: the scan's ScanContext distance to every key frame's, best by (dist, id); none at DBL_MAX or beyond max_dist
    std::vector<double> dist(M);
    std::vector<int32_t> shift(M);
    if (pcr_sc_distances(sc, src, n_src, stride_bytes, on_device, dist.data(), shift.data()))
        return fail(h, std::string("global relocalisation: ScanContext distances: ") + pcr_sc_last_error(sc));
    if (set_device(h)) return 1;
    std::vector<size_t> place;
    for (size_t i = 0; i < M; ++i) if (dist[i] != DBL_MAX && dist[i] <= p->max_dist) place.push_back(i);
    const size_t np = std::min(place.size(), (size_t)p->places);
    std::partial_sort(place.begin(), place.begin() + np, place.end(), [&](size_t a, size_t b) { return dist[a] != dist[b] ? dist[a] < dist[b] : a < b; });
    place.resize(np);
    if (place.empty())
        return fail(h, "global relocalisation: no place qualifies (" + std::to_string(M) + " contexts, max_dist = " + std::to_string(p->max_dist) +
                       "): is the scan from the mapped area, and were its key frames added to the ScanContext database?");
    if (np * K > (size_t)PCR_RELOC_MAX_POSES)
        return fail(h, "global relocalisation: " + std::to_string(np) + " places x " + std::to_string(K) + " hypotheses is more than PCR_RELOC_MAX_POSES (" +
                       std::to_string(PCR_RELOC_MAX_POSES) + ")");
    if (ensure_full_target(h)) return 1;      // (pcr_align's precondition; the coarse score then runs on the full index too)
    const float* d_src = (const float*)src;
    if (!on_device && stage_host(h, &h->q.rl_src, src, n_src, stride_bytes, &d_src)) return 1;      // once, for every step below

    // 2. every place's lattice around its coarse pose, all in one batched score on the subset
    std::vector<double> poses(np * K * 16), score(np * K);
    std::vector<int64_t> nin(np * K);
    for (size_t pl = 0; pl < np; ++pl) {
        double coarse[16];
        place_pose(kf_poses + place[pl] * 16, shift[place[pl]], coarse);
        for (size_t q = 0; q < K; ++q) reloc_pose(coarse, &p->local, nx, nk, q, &poses[(pl * K + q) * 16]);
    }
    const GridIndex* fit_grid = nullptr;
    if (score_grid_for(h, &fit_grid)) return 1;
    if (fitness_batch_run(h, fit_grid, d_src, n_src, stride_bytes / 4, poses.data(), np * K, p->local.max_sq, (size_t)p->local.score_points,
                          score.data(), nin.data())) return 1;
    // 3. per place: ranked by (-n_in, score, h), distinct winners (pcr_relocalize steps 2-3, no click)
    std::vector<std::pair<size_t, size_t>> taken;      // (place rank, hypothesis)
    for (size_t pl = 0; pl < np; ++pl)
        for (size_t q : reloc_distinct(reloc_rank(&score[pl * K], &nin[pl * K], K), nx, p->local.refine_top)) taken.emplace_back(pl, q);
    if (taken.empty())
        return fail(h, "global relocalisation: no hypothesis of the " + std::to_string(np) + " places has a source point within the gate (max_sq = " +
                       std::to_string(p->local.max_sq) + ") of the target: is the target the whole map?");
    // 4. each candidate refined by pcr_align; the refined poses scored on the whole source, the first by (-n_in, score, candidate order)
    const size_t nc = taken.size();
    std::vector<pcr_reloc_candidate*> cp(nc);
    for (size_t c = 0; c < nc; ++c) {
        const size_t pl = taken[c].first, q = taken[c].second, at = pl * K + q;
        pcr_global_reloc_candidate& o = cands[c];
        memset(&o, 0, sizeof o);
        o.place = (int64_t)place[pl];
        o.sc_dist = dist[place[pl]];
        o.sc_shift = shift[place[pl]];
        cp[c] = &o.c;
        std::string why;
        if (reloc_refine(h, d_src, n_src, stride_bytes, q, &poses[at * 16], score[at], nin[at], o.c, &why)) {
            *n_cands = c;
            return fail(h, "global relocalisation: refining hypothesis " + std::to_string(q) + " of place " + std::to_string(place[pl]) + ": " + why);
        }
    }
    *n_cands = nc;
    size_t best = 0;
    bool any = false;
    if (reloc_choose(h, d_src, n_src, stride_bytes, p->local.max_sq, cp.data(), nc, &best, &any)) return 1;
    // 5. the chosen pose; the handle as after pcr_relocalize
    memcpy(pose_out, cands[best].c.pose, 16 * sizeof(double));
    reloc_point_fitness_at(h, cands[best].c.pose);
    if (converged) *converged = cands[best].c.converged;
    *chosen = best;
    return 0;
}

}  // extern "C"
