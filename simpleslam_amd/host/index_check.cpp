// index_check -- builds grid indices on the device through pcr::GridIndex, one kernel variant after another, and compares the WHOLE result of
// every build -- header, cell_start[0 .. n_cells], sorted[0 .. cell_start[n_cells]) -- with the counting sort of host/index_ref.hpp.  Exactly:
// the one-level path's float sum of count^2 too is required exactly while it is below 2^24, which it is in every case (sum_sq_agrees below).
//
//   index_check            every case on the device, in order, in one process.  A HIP error ends the run at once (exit code 2, no further case);
//                          a mismatch is recorded (up to 20 are printed with cell, slot, got and want) and the run ends with exit code 1.
//   index_check --self     the reference alone against cell tables worked out by hand (below): no HIP call
//   index_check --plan     no HIP call either: every case with plan_build() / commit_build() (csrc/grid_plan.h) standing in for the device and the
//                          reference's header for the device's -- it holds the plans the cases expect to what the planner would say, on a machine
//                          without a GPU.  The device run never computes a plan: it reads GridIndex::last_plan, what build() enqueued.
//   index_check --list     the case names
//
// Every step of a case asserts the plan it expects FIRST (path, bin variant, place pass, keep pass, tile variants, header / layout reuse, filter,
// tail): a case that quietly took another path fails.  At the end the variants reached by steps that PASSED their comparison are printed, and the
// run fails unless all kBinVariants bin variants, all kTileVariants tile variants, both place kernels, both keep kernels and the one-level path are
// among them: a new instantiation needs a new case.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <functional>
#include <string>
#include <vector>

#include "../csrc/pcr_internal.h"
#include "index_ref.hpp"

namespace {

using pcr::BuildPlan;
using pcr::GridHeader;
using pcr::GridIndex;

bool g_dry = false;          // --plan
int g_mismatches = 0;        // printed so far (the cap of 20 ends the printing, never the comparing)
bool g_case_ok = true;       // the running case
std::string g_case;

#define HIPX(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP ERROR %s: %s (case %s)\nindex_check ABORTED\n", #x, hipGetErrorString(e_), g_case.c_str()); fflush(stdout); exit(2); } } while (0)

void mismatch(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void mismatch(const char* fmt, ...) {
    g_case_ok = false;
    if (g_mismatches >= 20) return;
    ++g_mismatches;
    va_list ap;
    va_start(ap, fmt);
    printf("  MISMATCH [%s] ", g_case.c_str());
    vprintf(fmt, ap);
    printf("\n");
    va_end(ap);
}

// ---- clouds ----------------------------------------------------------------------------------------------------------
struct Rng {      // a fixed generator: the clouds are the same wherever the program runs
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    float uni(float lo, float hi) { return lo + (hi - lo) * ((float)(next() >> 7) * (1.0f / 16777216.0f)); }
};
struct P3 { float x, y, z; };
typedef std::vector<P3> Pts;

void add_box(Pts& p, Rng& r, size_t n, float x0, float y0, float z0, float x1, float y1, float z1) {
    for (size_t i = 0; i < n; ++i) { P3 q; q.x = r.uni(x0, x1); q.y = r.uni(y0, y1); q.z = r.uni(z0, z1); p.push_back(q); }
}
void shuffle(Pts& p, Rng& r) { for (size_t i = p.size(); i > 1; --i) std::swap(p[i - 1], p[r.next() % i]); }

struct Cloud {      // a cloud as a build is given it: stride in floats, the first point `off` floats into the buffer
    std::vector<float> host;
    size_t n = 0, stride = 4, off = 0;
    float* d = nullptr;
    const float* hp() const { return host.data() + off; }
    const float* dp() const { return d + off; }
    bool vec() const { return stride % 4 == 0 && off % 4 == 0; }
    Cloud() = default;
    Cloud(const Cloud&) = delete;
    Cloud& operator=(const Cloud&) = delete;
    ~Cloud() { if (d && !g_dry) (void)hipFree(d); }
    void set(const Pts& p, size_t stride_ = 4, size_t off_ = 0) {
        if (d && !g_dry) (void)hipFree(d);
        d = nullptr;
        n = p.size(); stride = stride_; off = off_;
        host.assign(n * stride + off + 8, 7.25f);      // (what lies between the points is never a coordinate)
        for (size_t i = 0; i < n; ++i) { float* q = host.data() + off + i * stride; q[0] = p[i].x; q[1] = p[i].y; q[2] = p[i].z; }
        if (g_dry) { d = reinterpret_cast<float*>((uintptr_t)0x10000000); return; }      // (tested for alignment, never read)
        HIPX(hipMalloc(&d, host.size() * sizeof(float)));
        HIPX(hipMemcpy(d, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    }
};

// ---- one index and what the host knows of it ---------------------------------------------------------------------------
struct Ix {
    GridIndex g;
    index_ref::Header last{};      // the lattice of the last build whose header the host has seen to be good
    bool have_last = false;
};

enum MaskKind { kNoMask = 0, kMaskZero, kMaskOne, kMaskChecker };
struct Opt {
    double cell = 1.0, shift = 0.0;
    int pcl = 0;
    const index_ref::Clamp* clamp = nullptr;
    bool allow_hint = false;
    MaskKind mask = kNoMask;
    bool want_tail = false;
    int min_points = 3;
    bool room_over = false;      // a bin gets more points than the layout left it room for: the build must say stale = 2
    bool room_either = false;    // a bin MAY get more than its room (the rooms follow from cuts this program does not restate): stale = 2, or a complete index
    int want_cut_mask = -1;      // clamp cases: the bits worked out by hand
};
struct Expect {      // the plan a step must run (bin: the 16-byte variant; a cloud that is not 16-byte aligned takes its twin)
    int tiled = 1, bin = 6, tile0 = 9, tile1 = -1, reuse = 0, layout = 0, sub = 0, keep = 0, filtered = 0, tail = 0, preset = 0, tshift = -1;
};
Expect one_level() { Expect e; e.tiled = 0; e.bin = e.tile0 = -1; return e; }
Expect fresh(int tile0 = 9, int tshift = 10) { Expect e; e.tile0 = tile0; e.tshift = tshift; return e; }
Expect boxed(int tile0, int tile1 = -1, int tshift = -1) { Expect e; e.tile0 = tile0; e.tile1 = tile1; e.tshift = tshift; return e; }
Expect reused(int bin, int tile0, int tile1 = -1) { Expect e; e.bin = bin; e.tile0 = tile0; e.tile1 = tile1; e.reuse = e.layout = 1; e.sub = bin <= 3 && (bin == 0 || bin >= 2) ? 1 : 0; return e; }
Expect filt(Expect e, int keep = 0, int tail = 0) { e.filtered = 1; e.keep = keep; e.tail = tail; return e; }

struct Coverage { bool bin[pcr::kBinVariants] = {}, tile[pcr::kTileVariants] = {}, place[2] = {}, keep[2] = {}, one_level = false; } g_cov;

bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0 || a == b; }
void compare_lattice(const GridHeader& h, const index_ref::Header& r, bool with_counts) {
    for (int d = 0; d < 3; ++d) {
        if (!same_bits(h.origin[d], r.origin[d])) mismatch("header origin[%d] got %.17g want %.17g", d, h.origin[d], r.origin[d]);
        if (!same_bits(h.org[d], r.org[d])) mismatch("header org[%d] got %.17g want %.17g", d, h.org[d], r.org[d]);
        if (h.dims[d] != r.dims[d]) mismatch("header dims[%d] got %d want %d", d, h.dims[d], r.dims[d]);
        if (h.min_b[d] != r.min_b[d]) mismatch("header min_b[%d] got %d want %d", d, h.min_b[d], r.min_b[d]);
    }
    if (!same_bits(h.cell, r.cell) || !same_bits(h.inv_cell, r.inv_cell) || !same_bits(h.shift, r.shift)) mismatch("header cell / inv_cell / shift got %.17g %.17g %.17g want %.17g %.17g %.17g", h.cell, h.inv_cell, h.shift, r.cell, r.inv_cell, r.shift);
    if (h.pcl_mode != r.pcl_mode || h.inv_leaf_f != r.inv_leaf_f || h.too_fine != r.too_fine) mismatch("header pcl_mode / inv_leaf_f / too_fine got %d %.9g %d want %d %.9g %d", h.pcl_mode, h.inv_leaf_f, h.too_fine, r.pcl_mode, r.inv_leaf_f, r.too_fine);
    if (h.clamped != r.clamped || h.cut_mask != r.cut_mask) mismatch("header clamped / cut_mask got %d 0x%x want %d 0x%x", h.clamped, h.cut_mask, r.clamped, r.cut_mask);
    if (with_counts) {
        if (h.n_cells != r.n_cells) mismatch("header n_cells got %llu want %llu", (unsigned long long)h.n_cells, (unsigned long long)r.n_cells);
        if (h.n_points != r.n_points) mismatch("header n_points got %u want %u", h.n_points, r.n_points);
        if (h.overflow != r.overflow || h.empty != r.empty) mismatch("header overflow / empty got %d %d want %d %d", h.overflow, h.empty, r.overflow, r.empty);
    }
}

// The one-level path adds the cells' count^2 up in float (grid_scan_local_kernel, grid_scan_add_kernel).  Every term is the square of an integer, and while
// the exact sum stays below 2^24 every term and every partial sum -- in whatever order -- is an integer that float holds exactly: the float sum then IS
// the integer, and the step requires sum_sq == (float)exact, bit for bit.  Every case of this program is in that range.  Only for a sum of 2^24 or more
// (no case today) a bound takes over: every term is >= 0, so for ANY order of t additions of terms rounded once each
// |float sum - exact| <= exact * gamma(t + 1), gamma(k) = k u / (1 - k u), u = 2^-24 (Higham, Accuracy and Stability, lemma 3.1 and section 4.2);
// t < n_cells + 1 terms.
bool sum_sq_agrees(float got, unsigned long long exact, uint64_t n_cells) {
    if (exact < (1ull << 24)) return got == (float)exact;
    const double k = (double)n_cells + 2.0, u = 1.0 / 16777216.0;
    return fabs((double)got - (double)exact) <= (double)exact * (k * u / (1.0 - k * u));
}

// the plan of a step, as one line; false: not the plan the case is about
bool check_plan(const BuildPlan& p, const Expect& ex0, const Cloud& cl, const char* label) {
    Expect ex = ex0;
    if (ex.tiled && !cl.vec() && ex.bin >= 2) ex.bin += 1;
    const int bin = p.tiled_path ? pcr::variant_index(p.bin) : -1;
    const int t0 = p.tiled_path && p.n_tile > 0 ? pcr::variant_index(p.tile[0]) : -1, t1 = p.tiled_path && p.n_tile > 1 ? pcr::variant_index(p.tile[1]) : -1;
    printf("  step %-22s plan path=%s bin=%d place=%d keep=%d tile=%d,%d reuse_header=%d preset=%d use_layout=%d use_sub=%d cuts_now=%d filtered=%d with_tail=%d tshift=%d vec=%d\n", label,
           p.tiled_path ? "tiled" : "one_level", bin, p.tiled_path && p.place ? 1 : 0, p.keep_pass ? 1 : 0, t0, t1, p.reuse_header ? 1 : 0, p.preset ? 1 : 0, p.use_layout ? 1 : 0, p.use_sub ? 1 : 0,
           p.cuts_now ? 1 : 0, p.filtered ? 1 : 0, p.with_tail ? 1 : 0, p.tshift, p.vec ? 1 : 0);
    bool ok = (int)p.tiled_path == ex.tiled && (int)p.preset == ex.preset;
    if (ex.tiled) ok = ok && bin == ex.bin && t0 == ex.tile0 && t1 == ex.tile1 && (int)p.reuse_header == ex.reuse && (int)p.use_layout == ex.layout && (int)p.use_sub == ex.sub &&
                       (int)p.keep_pass == ex.keep && (int)p.filtered == ex.filtered && (int)p.with_tail == ex.tail && p.place == !p.use_layout && (ex.tshift < 0 || p.tshift == ex.tshift);
    if (!ok) mismatch("step %s: expected plan path=%s bin=%d tile=%d,%d reuse_header=%d preset=%d use_layout=%d use_sub=%d keep=%d filtered=%d with_tail=%d tshift=%d", label, ex.tiled ? "tiled" : "one_level", ex.bin,
                      ex.tile0, ex.tile1, ex.reuse, ex.preset, ex.layout, ex.sub, ex.keep, ex.filtered, ex.tail, ex.tshift);
    return ok;
}

std::vector<uint8_t> make_mask(const index_ref::Header& lat, MaskKind kind, int mshift) {
    std::vector<uint8_t> m(index_ref::macro_count(lat, mshift) + 16, kind == kMaskOne ? 1 : 0);
    if (kind == kMaskChecker) {      // every other macro cell: each tile of the lattice is split many times over
        const uint32_t m0 = index_ref::macro_dim(lat, mshift, 0), m1 = index_ref::macro_dim(lat, mshift, 1), m2 = index_ref::macro_dim(lat, mshift, 2);
        for (uint32_t z = 0; z < m2; ++z) for (uint32_t y = 0; y < m1; ++y) for (uint32_t x = 0; x < m0; ++x) m[((size_t)z * m1 + y) * m0 + x] = ((x + y + z) & 1u) ? 0 : 255;
    }
    return m;
}

// One build and its whole comparison.  Returns the header the device left (in --plan mode: the one the reference expects).
// preset_from: the header the twin's build must have written for this one (a preset build)
bool step(Ix& ix, const Cloud& cl, const Opt& o, const Expect& ex, const char* label, const index_ref::Header* preset_from = nullptr) {
    GridIndex& g = ix.g;
    const int mshift = 1;
    // what the build will be given
    const uint64_t cap_before = g.cell_capacity ? (uint64_t)g.effective_capacity() : (uint64_t)(g.cells_hint ? std::min<size_t>((size_t)1 << 20, std::max<size_t>(2 * (size_t)g.cells_hint + 64, 1024)) : (size_t)1 << 20);
    const int mg_xy = (o.allow_hint && !o.clamp) ? g.hint_margin : 0, mg_z = (o.allow_hint && !o.clamp) ? g.hint_margin_z_pcl : 0;
    std::vector<uint8_t> mask_host;
    uint8_t* d_mask = nullptr;
    pcr::BuildFilter filter;
    uint32_t *d_slot = nullptr, *d_list = nullptr, *d_count = nullptr;
    const uint64_t tail_cells = ix.have_last ? ix.last.n_cells : 0;
    if (o.mask != kNoMask && ix.have_last) {
        mask_host = make_mask(ix.last, o.mask, mshift);
        if (!g_dry) { HIPX(hipMalloc(&d_mask, mask_host.size())); HIPX(hipMemcpy(d_mask, mask_host.data(), mask_host.size(), hipMemcpyHostToDevice)); }
        else d_mask = reinterpret_cast<uint8_t*>((uintptr_t)0x20000000);
        filter.enqueue_mask = [&]() { filter.mask = d_mask; filter.mshift = mshift; return hipSuccess; };
        if (o.want_tail) {
            filter.want_tail = true;
            if (!g_dry) {
                HIPX(hipMalloc(&d_slot, (tail_cells + 8) * 4)); HIPX(hipMalloc(&d_list, (tail_cells + 8) * 4)); HIPX(hipMalloc(&d_count, 64));
                HIPX(hipMemset(d_slot, 0x5a, (tail_cells + 8) * 4));
                const uint32_t init[2] = {0u, 77u};
                HIPX(hipMemcpy(d_count, init, sizeof init, hipMemcpyHostToDevice));
            }
            filter.tail.vox_slot = d_slot; filter.tail.list = d_list; filter.tail.count = d_count; filter.tail.count_next = d_count ? d_count + 1 : nullptr;
            filter.tail.min_points = o.min_points; filter.tail.capacity = (uint32_t)tail_cells;
        }
    }
    pcr::ClampBox cb;
    memset(&cb, 0, sizeof cb);
    index_ref::Clamp no_clamp;
    if (o.clamp) { cb.use = 1; for (int d = 0; d < 3; ++d) { cb.lo[d] = o.clamp->lo[d]; cb.hi[d] = o.clamp->hi[d]; } }
    BuildPlan p;
    if (!g_dry) {
        std::string err;
        const hipError_t e = g.build(cl.dp(), cl.n, cl.stride, o.cell, nullptr, &err, o.shift, o.pcl, o.clamp ? &cb : nullptr, o.allow_hint, filter.enqueue_mask ? &filter : nullptr);
        if (e != hipSuccess) { printf("HIP ERROR in build(): %s (case %s, step %s)\nindex_check ABORTED\n", err.c_str(), g_case.c_str(), label); fflush(stdout); exit(2); }
        HIPX(g.enqueue_density(nullptr));
        HIPX(hipStreamSynchronize(nullptr));
        HIPX(hipDeviceSynchronize());
        p = g.last_plan;
    } else {      // the planner stands in for the device: what build() does around enqueue_build, without it
        if (!g.cell_capacity) g.cell_capacity = (size_t)1 << 20;
        g.valid = false; g.filtered = false;
        g.has_mirror = false; g.has_twin = g.twin && g.twin != &g;
        pcr::BuildRequest rq;
        rq.pts = cl.dp(); rq.n = cl.n; rq.stride_floats = cl.stride; rq.cell = o.cell; rq.shift = o.shift; rq.pcl_mode = o.pcl; rq.clamp = o.clamp != nullptr; rq.allow_hint = o.allow_hint;
        rq.mask_callback = (bool)filter.enqueue_mask; rq.want_tail = filter.want_tail;
        p = pcr::plan_build(g, rq);
        if (p.asks_mask) { rq.mask_set = true; p = pcr::plan_build(g, rq); }
        if (p.feeds_twin) { g.twin->header_preset = true; g.twin->preset_pts = cl.dp(); g.twin->preset_n = cl.n; g.twin->preset_cell = g.twin_cell; }
        pcr::commit_build(g, rq, p);
        g.valid = true;
    }
    bool ok_before = g_case_ok;
    g_case_ok = true;
    const bool plan_ok = check_plan(p, ex, cl, label);
    // ---- the lattice in use, and what it must hold ----
    index_ref::Header lat;
    if (ex.reuse) lat = ix.last;
    else if (ex.preset && preset_from) lat = *preset_from;
    else lat = index_ref::fresh_header(cl.hp(), cl.n, cl.stride, o.cell, o.shift, o.pcl, o.clamp ? *o.clamp : no_clamp, mg_xy, mg_z, cap_before);
    GridHeader h;
    memset(&h, 0, sizeof h);
    std::vector<uint32_t> cs;
    std::vector<float4> sorted;
    index_ref::Mask rm;
    rm.bytes = mask_host.data(); rm.mshift = mshift;
    const bool indexed = !lat.overflow && !lat.empty;
    index_ref::Table ref;
    if (indexed) ref = index_ref::build_table(lat, cl.hp(), cl.n, cl.stride, ex.filtered ? &rm : nullptr);
    int want_stale = o.room_over ? 2 : (ex.reuse && ref.outside ? 1 : 0);
    if (plan_ok && !g_dry) {
        HIPX(hipMemcpy(&h, g.header.p, sizeof h, hipMemcpyDeviceToHost));
        if (o.room_either && !want_stale && h.stale == 2) want_stale = 2;
        compare_lattice(h, lat, !ex.reuse);
        if (ex.reuse && (h.n_cells != lat.n_cells || h.n_points != lat.n_points || h.overflow || h.empty)) mismatch("step %s: the reused header changed", label);
        if (o.want_cut_mask >= 0 && h.cut_mask != o.want_cut_mask) mismatch("step %s: cut_mask got 0x%x, worked out by hand 0x%x", label, h.cut_mask, o.want_cut_mask);
        if (h.stale != want_stale) mismatch("step %s: header stale got %d want %d (%zu points outside the box)", label, h.stale, want_stale, ref.outside);
        if (g_case_ok && indexed && !want_stale) {
            const size_t nc = (size_t)lat.n_cells;
            cs.resize(nc + 1);
            HIPX(hipMemcpy(cs.data(), g.cell_start.p, (nc + 1) * 4, hipMemcpyDeviceToHost));
            bool shape = cs[0] == 0;
            if (!shape) mismatch("step %s: cell_start[0] = %u", label, cs[0]);
            for (size_t c = 0; c < nc && shape; ++c) if (cs[c + 1] < cs[c]) { mismatch("step %s: cell_start decreases at cell %zu: %u -> %u", label, c, cs[c], cs[c + 1]); shape = false; }
            if (cs[nc] != ref.order.size()) { mismatch("step %s: cell_start[n_cells] got %u want %zu indexed points (%zu non-finite, %zu outside, %zu masked of %zu)", label, cs[nc], ref.order.size(), ref.non_finite, ref.outside, ref.masked, cl.n); shape = false; }
            for (size_t c = 0; c <= nc; ++c) if (cs[c] != ref.cell_start[c]) { mismatch("step %s: cell_start[%zu] got %u want %u", label, c, cs[c], ref.cell_start[c]); shape = false; }
            if (shape) {
                sorted.resize(cs[nc] + 1);
                if (cs[nc]) HIPX(hipMemcpy(sorted.data(), g.sorted.p, (size_t)cs[nc] * sizeof(float4), hipMemcpyDeviceToHost));
                std::vector<uint32_t> w;
                for (size_t c = 0; c < nc; ++c) {
                    const uint32_t a = cs[c], b = cs[c + 1];
                    if (a == b) continue;
                    w.resize(b - a);
                    for (uint32_t s = a; s < b; ++s) memcpy(&w[s - a], &sorted[s].w, 4);
                    if (b - a > 1) std::sort(w.begin(), w.end());      // (the order inside a cell is immaterial)
                    for (uint32_t s = a; s < b; ++s) if (w[s - a] != ref.order[s]) { mismatch("step %s: cell %zu, %u-th smallest original index got %u want %u", label, c, s - a, w[s - a], ref.order[s]); break; }
                    for (uint32_t s = a; s < b; ++s) {
                        uint32_t i; memcpy(&i, &sorted[s].w, 4);
                        if (i >= cl.n) { mismatch("step %s: cell %zu slot %u holds original index %u of %zu points", label, c, s, i, cl.n); break; }
                        if (memcmp(&sorted[s], cl.hp() + (size_t)i * cl.stride, 12) != 0) { const float* q = cl.hp() + (size_t)i * cl.stride; mismatch("step %s: cell %zu slot %u (point %u) got (%.9g %.9g %.9g) want (%.9g %.9g %.9g)", label, c, s, i, sorted[s].x, sorted[s].y, sorted[s].z, q[0], q[1], q[2]); break; }
                    }
                }
            }
            if (p.tiled_path) { if (h.sum_sq_u != ref.sum_sq) mismatch("step %s: sum_sq_u got %llu want %llu", label, h.sum_sq_u, ref.sum_sq); }
            else if (!sum_sq_agrees(h.sum_sq, ref.sum_sq, lat.n_cells)) mismatch("step %s: sum_sq got %.9g want %llu%s", label, h.sum_sq, ref.sum_sq, ref.sum_sq < (1ull << 24) ? " exactly" : " within the summation bound");
            if (ex.tail) {      // NDT's tail: the cells inside the mask with min_points points or more, as a set; every cell's slot; the other counter cleared
                uint32_t cnt[2];
                HIPX(hipMemcpy(cnt, d_count, sizeof cnt, hipMemcpyDeviceToHost));
                std::vector<uint32_t> want, got(std::min<uint64_t>(cnt[0], tail_cells)), slot(nc);
                for (size_t c = 0; c < nc; ++c) if (index_ref::mask_holds_cell(lat, rm, c) && (int)(ref.cell_start[c + 1] - ref.cell_start[c]) >= o.min_points) want.push_back((uint32_t)c);
                if (!got.empty()) HIPX(hipMemcpy(got.data(), d_list, got.size() * 4, hipMemcpyDeviceToHost));
                std::sort(got.begin(), got.end());
                if (cnt[0] != want.size() || got != want) mismatch("step %s: tail list holds %u cells, want %zu (or the cells differ)", label, cnt[0], want.size());
                if (cnt[1] != 0u) mismatch("step %s: tail count_next got %u want 0", label, cnt[1]);
                HIPX(hipMemcpy(slot.data(), d_slot, nc * 4, hipMemcpyDeviceToHost));
                for (size_t c = 0; c < nc; ++c) { const uint32_t ws = index_ref::mask_holds_cell(lat, rm, c) ? 0u : pcr::kNdtUnprepared; if (slot[c] != ws) { mismatch("step %s: tail vox_slot[%zu] got 0x%x want 0x%x", label, c, slot[c], ws); break; } }
            }
        }
        // the counters every build promises to leave zeroed
        std::vector<uint32_t> z;
        if (g.ticket.p) { z.resize(64); HIPX(hipMemcpy(z.data(), g.ticket.p, 256, hipMemcpyDeviceToHost)); for (size_t i = 0; i < z.size(); ++i) if (z[i]) { mismatch("step %s: ticket word %zu = %u after the build", label, i, z[i]); break; } }
        if (p.tiled_path && g.bin_count.p) {
            z.resize(((size_t)pcr::kMaxBins + 64) * 16);
            HIPX(hipMemcpy(z.data(), g.bin_count.p, z.size() * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < z.size(); ++i) if (z[i]) { mismatch("step %s: bin_count word %zu (bin %zu) = %u after the build", label, i, i / 16, z[i]); break; }
        }
        if (!p.tiled_path && g.cell_count.p && !lat.overflow) {
            z.resize((size_t)lat.n_cells + 1);
            HIPX(hipMemcpy(z.data(), g.cell_count.p, z.size() * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < z.size(); ++i) if (z[i]) { mismatch("step %s: cell_count[%zu] = %u after the build", label, i, z[i]); break; }
        }
    }
    const bool passed = g_case_ok;
    if (passed && (!g_dry)) {      // reached, by a step that passed its comparison
        if (!p.tiled_path) g_cov.one_level = true;
        else {
            g_cov.bin[pcr::variant_index(p.bin)] = true;
            for (int i = 0; i < p.n_tile; ++i) g_cov.tile[pcr::variant_index(p.tile[i])] = true;
            if (p.place) g_cov.place[p.vec ? 1 : 0] = true;
            if (p.keep_pass) g_cov.keep[p.vec ? 1 : 0] = true;
        }
    }
    printf("  step %-22s %s  cells=%llu indexed=%zu non_finite=%zu outside=%zu masked=%zu overflow=%d empty=%d stale=%d\n", label, passed ? "ok" : "FAILED", (unsigned long long)lat.n_cells, ref.order.size(),
           ref.non_finite, ref.outside, ref.masked, lat.overflow, lat.empty, want_stale);
    // what a caller does with a header it has read (loam_host.hip, ndt_host.hip): a good one bounds the next build's cells and may be reused
    if (!lat.overflow && !want_stale) {
        g.note_cells(lat.n_cells);
        if (!lat.empty && !o.clamp) g.confirm();
        if (!ex.reuse) { ix.last = lat; ix.have_last = true; }
    }
    if (!g_dry) { if (d_mask) HIPX(hipFree(d_mask)); if (d_slot) HIPX(hipFree(d_slot)); if (d_list) HIPX(hipFree(d_list)); if (d_count) HIPX(hipFree(d_count)); }
    g_case_ok = ok_before && passed;
    return passed;
}

// ---- the clouds the cases share ------------------------------------------------------------------------------------------
// 1 m cells.  The walk's cloud: a 20 x 20 x 8 m box (24 x 24 x 12 = 6 912 cells with the pads: from the second build on tiles of 2^7 cells, eight points
// per thread, tiles cut at hs = 2 048), a 3 m cube that holds several times hs (its tiles are cut into slabs) and a 0.2 m cube of more than 4 096 points
// (one cell, which no cut divides: the chunked path of the tile pass).
Pts walk_points(Rng& r, size_t bulk = 10000, size_t cube = 8000, size_t tight = 5000) {
    Pts p;
    p.push_back(P3{-10.f, -10.f, -2.f}); p.push_back(P3{9.5f, 9.5f, 5.5f});      // the box, whatever the draw
    add_box(p, r, bulk, -10.f, -10.f, -2.f, 9.5f, 9.5f, 5.5f);
    add_box(p, r, cube, 3.3f, -7.6f, 0.4f, 6.3f, -4.6f, 3.4f);
    add_box(p, r, tight, 4.6f, -6.5f, 1.3f, 4.8f, -6.3f, 1.5f);
    shuffle(p, r);
    return p;
}
// a small dense cloud in the same box
Pts small_points(Rng& r, size_t n) {
    Pts p;
    p.push_back(P3{-10.f, -10.f, -2.f}); p.push_back(P3{9.5f, 9.5f, 5.5f});
    add_box(p, r, n - 2, -10.f, -10.f, -2.f, 9.5f, 9.5f, 5.5f);
    return p;
}
// n points in an 8 x 8 x 4 m box, no fixed corners (the n edges of the two paths)
Pts edge_points(Rng& r, size_t n) { Pts p; add_box(p, r, n, 0.f, 0.f, 0.f, 8.f, 8.f, 4.f); return p; }

// a sparse grid: points over an 80 x 80 x 30 m box (84 x 84 x 34 = 239 904 cells > 4 n + 65 536), ring by ring: eight consecutive points per cell
Pts sparse_points(Rng& r, size_t cells, bool clusters) {
    Pts p;
    p.push_back(P3{-40.f, -40.f, -10.f}); p.push_back(P3{39.5f, 39.5f, 19.5f});
    for (size_t c = 0; c < cells; ++c) {
        const float x = floorf(r.uni(-40.f, 39.f)), y = floorf(r.uni(-40.f, 39.f)), z = floorf(r.uni(-10.f, 19.f));
        add_box(p, r, 8, x, y, z, x + 0.99f, y + 0.99f, z + 0.99f);
    }
    if (clusters) {      // more than 3 072 points in one tile; about 12 000 in one cell -- one bin whatever is cut: three chunks of the 1 024-thread variant
        add_box(p, r, 5000, 10.f, 10.f, 5.f, 13.99f, 10.99f, 5.99f);
        add_box(p, r, 12000, -20.2f, -20.7f, 3.1f, -20.1f, -20.5f, 3.4f);
    }
    return p;
}

typedef void (*CaseFn)();
struct Case { const char* name; CaseFn fn; };

// ---- one-level path --------------------------------------------------------------------------------------------------------
void one_level_case(const Pts& p) { Ix ix; ix.g.prefer_one_level = true; Cloud c; c.set(p); Opt o; step(ix, c, o, one_level(), "fresh"); }
template <int N> void c_one_level_n() { Rng r(100 + N); one_level_case(edge_points(r, N)); }
void c_one_level_one_cell() { Rng r(7); Pts p; add_box(p, r, 300, 0.1f, 0.1f, 0.1f, 0.9f, 0.9f, 0.9f); one_level_case(p); }
void c_one_level_scan_tiles() {
    // a 166-cell row: dims (170, 5, 5) = 4 250 cells, three scan blocks; the first inner cell has key (2 * 5 + 2) * 170 + 2 = 2 042, so the cells
    // x = 4, 5 (keys 2 046, 2 047) and x = 6, 7 (2 048, 2 049) lie either side of the first 2 048-cell boundary, and 4 096 falls into the pads
    Pts p;
    for (int i = 0; i < 166; ++i) for (int k = 0; k < 3; ++k) p.push_back(P3{(float)i + 0.25f * (float)(k + 1), 0.5f, 0.5f});
    one_level_case(p);
}
const float kBad[3] = {NAN, INFINITY, -INFINITY};
void c_one_level_non_finite() {
    Rng r(9); Pts p = edge_points(r, 200);
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) { P3 q = p[10 + 3 * a + b]; (a == 0 ? q.x : a == 1 ? q.y : q.z) = kBad[b]; p[20 * (3 * a + b) + 5] = q; }
    one_level_case(p);
}
void c_one_level_all_non_finite() { Pts p; for (int i = 0; i < 10; ++i) p.push_back(P3{kBad[i % 3], 1.f, kBad[(i + 1) % 3]}); one_level_case(p); }

// ---- fresh tiled build: by tile, place pass, sixteen points per thread -------------------------------------------------------
void fresh_case(const Pts& p, size_t stride = 4, size_t off = 0) { Ix ix; Cloud c; c.set(p, stride, off); Opt o; step(ix, c, o, fresh(), "fresh"); }
template <int N> void c_fresh_n() { Rng r(200 + N); fresh_case(edge_points(r, N)); }
void c_fresh_non_finite() {
    Rng r(19); Pts p = edge_points(r, 3000);
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) { P3 q = p[10 + 3 * a + b]; (a == 0 ? q.x : a == 1 ? q.y : q.z) = kBad[b]; p[300 * (3 * a + b) + 5] = q; }
    fresh_case(p);
}
void c_fresh_all_non_finite() { Pts p; for (int i = 0; i < 300; ++i) p.push_back(P3{kBad[i % 3], 1.f, kBad[(i + 1) % 3]}); fresh_case(p); }
template <int S, int O> void c_fresh_stride() { Rng r(300 + 10 * S + O); fresh_case(edge_points(r, 5000), S, O); }

// ---- the walk: fresh -> tile size by the cells seen -> header and layout reused, the cloud growing inside its box ------------------------------
void walk(size_t stride, bool coherent) {
    Rng r(42);
    Pts p = walk_points(r);
    Ix ix; ix.g.coherent_input = coherent;
    Cloud c; c.set(p, stride);
    Opt o; o.allow_hint = true;
    step(ix, c, o, fresh(coherent ? 3 : 9), "fresh");
    ix.g.reserve_points = 3 * p.size();
    step(ix, c, o, boxed(coherent ? 2 : 8, -1, 7), "tiles_by_cells");
    add_box(p, r, 20, -9.f, -9.f, -1.f, 9.f, 9.f, 5.f); add_box(p, r, 10, 4.6f, -6.5f, 1.3f, 4.8f, -6.3f, 1.5f);      // (at most 32 points: every bin has that room)
    c.set(p, stride);
    step(ix, c, o, reused(2, coherent ? 2 : 8), "reuse_layout");
    add_box(p, r, 30, 3.3f, -7.6f, 0.4f, 6.3f, -4.6f, 3.4f);
    c.set(p, stride);
    step(ix, c, o, reused(2, coherent ? 2 : 8), "reuse_cut_layout");
    // the 3 m cube's points go (every eighth stays): the slabs its tiles were cut into are merged back, one step per build
    Pts q; size_t k = 0;
    for (const P3& a : p) { const bool in = a.x >= 3.3f && a.x <= 6.3f && a.y >= -7.6f && a.y <= -4.6f && a.z >= 0.4f && a.z <= 3.4f; if (!in || (k++ % 8) == 0) q.push_back(a); }
    c.set(q, stride);
    step(ix, c, o, reused(2, coherent ? 2 : 8), "shrunk");
    step(ix, c, o, reused(2, coherent ? 2 : 8), "merged_back");
    c.set(p, stride);      // ... and come back: more than the merged slabs have room for is possible, so the build may say so -- or must be complete
    Opt oe = o; oe.room_either = true;
    if (!step(ix, c, oe, reused(2, coherent ? 2 : 8), "merged_again") || ix.g.hint_ok) return;
    step(ix, c, o, boxed(coherent ? 2 : 8, -1, 7), "fresh_box_after_stale");
}
void c_walk_vec() { walk(4, false); }
void c_walk_not_vec() { walk(3, false); }
void c_walk_coherent() { walk(4, true); }

// ---- a layout without cuts (bin = tile): a bin that fills its room exactly, and one point more -------------------------------------------------------
// 50 000 points in a 2 x 2 x 1 m box: 6 x 6 x 5 = 180 cells, tiles of 4 cells holding > 1 024 points on average: sixteen per thread, nothing is cut.
// A bin's room is what it held + that >> lay_room_shift + lay_room_add (csrc/grid_plan.h); the bin pass promises that a bin which outgrows it raises
// header.stale (= 2) and stores nothing out of bounds: so exactly room points must give a complete index, room + 1 the flag.
void room_case(int extra_over) {
    Rng r(77);
    Pts p; p.push_back(P3{0.f, 0.f, 0.f}); p.push_back(P3{1.99f, 1.99f, 0.99f});
    add_box(p, r, 49998, 0.f, 0.f, 0.f, 1.99f, 1.99f, 0.99f);
    Ix ix; Cloud c; c.set(p);
    Opt o; o.allow_hint = true;
    step(ix, c, o, fresh(), "fresh");
    step(ix, c, o, boxed(9, -1, 2), "tiles_by_cells");
    // the tile of the cells (2, 2, 2) and (3, 2, 2): keys 86 and 87, tile 21 = cells 84 .. 87
    const index_ref::Table t = index_ref::build_table(ix.last, c.hp(), c.n, c.stride);
    const uint32_t held = t.cell_start[88] - t.cell_start[84];
    const uint32_t room = held + (held >> ix.g.lay_room_shift) + ix.g.lay_room_add;
    add_box(p, r, room - held + (uint32_t)extra_over, 0.f, 0.f, 0.f, 1.99f, 0.99f, 0.99f);
    c.set(p);
    Opt o2 = o; o2.room_over = extra_over > 0;
    step(ix, c, o2, reused(4, 9), extra_over ? "room_plus_one" : "room_exactly");
    if (extra_over) {      // what a caller does then (loam_host.hip): a fresh box, from then on padded
        ix.g.hint_margin = 8; ix.g.cells_hint = 0;
        step(ix, c, o, fresh(), "rebuilt");
    }
}
void c_room_exact() { room_case(0); }
void c_room_plus_one() { room_case(1); }

// ---- stale: a point outside the reused box ------------------------------------------------------------------------------------------
// the box of small_points spans the cells [-10, 10) x [-10, 10) x [-2, 6): the last float inside and the first outside, on each of the six faces
void c_stale_faces() {
    Rng r(5);
    const Pts base = small_points(r, 5000);
    Ix ix; Cloud c; c.set(base);
    Opt o; o.allow_hint = true;
    step(ix, c, o, fresh(), "fresh");
    step(ix, c, o, boxed(8, -1, 7), "tiles_by_cells");
    const float face_lo[3] = {-10.f, -10.f, -2.f}, face_hi[3] = {10.f, 10.f, 6.f};
    char label[64];
    for (int f = 0; f < 6; ++f) {
        const int d = f % 3; const bool up = f >= 3;
        const float on = up ? nextafterf(face_hi[d], 0.f) : face_lo[d];                         // the last cell inside
        const float ulp = up ? face_hi[d] : nextafterf(face_lo[d], -INFINITY);                 // one float further: the first pad cell
        const float cellout = up ? face_hi[d] + 1.5f : face_lo[d] - 1.5f;                      // ... and a cell and a half further: the second
        const float v[3] = {on, ulp, cellout};
        for (int k = 0; k < 3; ++k) {
            Pts p = base; P3& q = p[1234 + f]; (d == 0 ? q.x : d == 1 ? q.y : q.z) = v[k];
            c.set(p);
            snprintf(label, sizeof label, "%c%s_%s", "xyz"[d], up ? "hi" : "lo", k == 0 ? "inside" : k == 1 ? "ulp_out" : "cell_out");
            step(ix, c, o, reused(2, 8), label);      // (k > 0: the reference finds the point outside, and the step requires stale = 1)
            if (k > 0) { c.set(base); step(ix, c, o, boxed(8, -1, 7), "fresh_box_again"); }      // a stale build leaves no hint: a box pass, then the header serves again
        }
    }
    // after a failed hint the callers pad the next fresh box (hint_margin) and forget the cell count
    Pts p = base; p[99].x = 13.25f; c.set(p);
    step(ix, c, o, reused(2, 8), "failed_hint");
    ix.g.hint_margin = 8; ix.g.cells_hint = 0;
    step(ix, c, o, fresh(), "rebuilt_with_margin");
    step(ix, c, o, boxed(8), "margin_tiles_by_cells");
    p[100].x = 16.5f; c.set(p);      // inside the margin now
    step(ix, c, o, reused(2, 8), "margin_serves");
}

// ---- overflow: a box of exactly effective_capacity() cells needs one table entry too many ----------------------------------------------------------------
void c_overflow() {
    Rng r(3);
    Ix ix; Cloud c; c.set(edge_points(r, 3000));      // 12 x 12 x 8 = 1 152 cells: the next build may use 2 * 1 152 + 64 = 2 368
    Opt o; o.allow_hint = true;
    step(ix, c, o, fresh(), "fresh");
    Pts p; add_box(p, r, 3000, 0.f, 0.f, 0.f, 4.f, 4.f, 33.f);
    p[0] = P3{0.5f, 0.5f, 0.5f}; p[1] = P3{3.5f, 3.5f, 32.5f};      // 8 x 8 x 37 = 2 368 cells: + 1 start > 2 368
    c.set(p);
    step(ix, c, o, boxed(8), "one_cell_too_many");      // (the step requires overflow = 1 and n_cells = 2 368, and reads no table)
    std::string err;
    if (ix.g.grow_cells(2368, &err) != hipSuccess) mismatch("grow_cells: %s", err.c_str());
    step(ix, c, o, boxed(8), "after_grow_cells");
    Pts q; add_box(q, r, 3000, 0.f, 0.f, 0.f, 4.f, 4.f, 32.f);
    q[0] = P3{0.5f, 0.5f, 0.5f}; q[1] = P3{3.5f, 3.5f, 31.5f}; c.set(q);      // 8 x 8 x 36 = 2 304 cells: a cell row fewer fits
    Ix iy; Cloud c2; Rng r2(3); c2.set(edge_points(r2, 3000));
    step(iy, c2, o, fresh(), "fresh_b");
    step(iy, c, o, boxed(8), "fits");
}

// ---- clamp: a region of interest that cuts each face in turn ------------------------------------------------------------------------------------------
void c_clamp_faces() {
    Rng r(11);
    Cloud c; c.set(small_points(r, 6000));
    char label[32];
    for (int f = 0; f < 6; ++f) {
        Ix ix;
        index_ref::Clamp cl; cl.use = true;
        for (int d = 0; d < 3; ++d) { cl.lo[d] = -1000.0; cl.hi[d] = 1000.0; }
        if (f < 3) cl.lo[f] = f == 2 ? 0.25 : -3.25; else cl.hi[f - 3] = f == 5 ? 2.75 : 4.5;
        Opt o; o.clamp = &cl; o.want_cut_mask = f < 3 ? 1 << f : 8 << (f - 3);
        snprintf(label, sizeof label, "cut_%c%s", "xyz"[f % 3], f < 3 ? "lo" : "hi");
        step(ix, c, o, fresh(), label);
    }
    index_ref::Clamp cl; cl.use = true;
    for (int d = 0; d < 3; ++d) { cl.lo[d] = d == 2 ? -1.5 : -2.5; cl.hi[d] = 3.0; }      // (the cloud's z starts at -2)
    Opt o; o.clamp = &cl; o.want_cut_mask = 63;
    Ix ix, iy;
    step(ix, c, o, fresh(), "cut_all_six");
    for (int d = 0; d < 3; ++d) { cl.lo[d] = 500.0; cl.hi[d] = 600.0; }      // nothing inside: empty
    o.want_cut_mask = -1;
    step(iy, c, o, fresh(), "nothing_inside");
}

// ---- sparse grids -----------------------------------------------------------------------------------------------------------------------
void sparse(bool coherent, bool cut, bool shuffled, bool split = true) {
    Rng r(21);
    Pts p = sparse_points(r, 250, cut);
    if (shuffled) shuffle(p, r);
    Ix ix; ix.g.coherent_input = coherent; ix.g.cut_sparse = cut; ix.g.split_sparse_tiles = split;
    Cloud c; c.set(p);
    Opt o; o.allow_hint = true;
    step(ix, c, o, fresh(coherent ? 3 : 9), "fresh");
    printf("  cells_hint=%llu\n", (unsigned long long)ix.g.cells_hint);
    const int ts = cut ? 12 : 11;
    if (!split) {      // the owner's switch: one dense instantiation for every tile
        step(ix, c, o, boxed(8, -1, ts), "tiles_by_cells");
        step(ix, c, o, reused(2, 8), "reuse_layout");
        return;
    }
    step(ix, c, o, boxed(coherent ? 0 : 4, coherent ? 1 : 5, ts), "tiles_by_cells");
    add_box(p, r, 16, -30.f, -30.f, 0.f, 30.f, 30.f, 10.f); c.set(p);
    step(ix, c, o, reused(cut ? 2 : 4, coherent ? 0 : 4, coherent ? 1 : 5), "reuse_layout");
    if (cut) { add_box(p, r, 16, 10.f, 10.f, 5.f, 13.99f, 10.99f, 5.99f); c.set(p); step(ix, c, o, reused(2, coherent ? 0 : 4, coherent ? 1 : 5), "reuse_cut_layout"); }
}
void c_sparse_rings() { sparse(false, false, false); }
void c_sparse_shuffled() { sparse(false, false, true); }
void c_sparse_coherent_rings() { sparse(true, false, false); }
void c_sparse_coherent_shuffled() { sparse(true, false, true); }
void c_sparse_cut_clusters() { sparse(false, true, false); }
void c_sparse_cut_coherent_clusters() { sparse(true, true, false); }
void c_sparse_not_split() { sparse(false, false, false, false); }

// ---- pcl::VoxelGrid's lattice (the voxel filter's index) ------------------------------------------------------------------------------------------
void pcl_case(double leaf) {
    Rng r(31);
    Pts p; add_box(p, r, 3000, -3.f, -3.f, -1.f, 3.f, 3.f, 1.f);
    // a float either side of voxel faces, negative coordinates included
    for (int k = -20; k <= 20; ++k) {
        const float f = (float)k * (float)leaf;
        p.push_back(P3{f, 0.3f, 0.2f}); p.push_back(P3{nextafterf(f, -INFINITY), f, 0.2f}); p.push_back(P3{nextafterf(f, INFINITY), 0.1f, f * 0.25f}); p.push_back(P3{-0.7f, nextafterf(f, -INFINITY), nextafterf(f * 0.25f, INFINITY)});
    }
    Ix ix; ix.g.cut_sparse = true; ix.g.coherent_input = true; ix.g.hint_margin = 16; ix.g.hint_margin_z_pcl = 4; ix.g.lay_room_shift = 1; ix.g.lay_room_add = 256;      // (voxel_host.hip)
    Cloud c; c.set(p);
    Opt o; o.cell = leaf; o.pcl = 1; o.allow_hint = true;
    step(ix, c, o, fresh(3), "fresh");
    Expect e2; e2.tile0 = 0; e2.tile1 = 1;      // with the margins of 16, 16 and 4 voxels a sparse grid at either leaf (0.5: 104 044 voxels for 3 164 points)
    step(ix, c, o, e2, "tiles_by_cells");
    add_box(p, r, 40, -4.f, -4.f, -1.2f, 4.f, 4.f, 1.2f); c.set(p);      // inside the margins
    step(ix, c, o, reused(2, e2.tile0, e2.tile1), "reuse_layout");
    p[5].z = 9.f; c.set(p);      // beyond the four voxels of margin in z (leaf 0.5: 1 + 2 m): the hint fails, the next box is fresh
    step(ix, c, o, reused(2, e2.tile0, e2.tile1), "failed_hint");
    ix.g.cells_hint = 0;
    step(ix, c, o, fresh(3), "rebuilt_with_margins");
    Opt plain; plain.cell = leaf; plain.pcl = 1;      // without hints: no margins
    Ix iy; step(iy, c, plain, fresh(), "no_margins");
}
void c_pcl_leaf_01() { pcl_case(0.1); }
void c_pcl_leaf_05() { pcl_case(0.5); }

// ---- shifted lattice (VGICP's voxels: shift = 0.5), points exactly on the half-cell planes; and an edge that is no power of two --------------------
void shifted_case(double cell) {
    Rng r(41);
    Pts p; add_box(p, r, 3000, -6.f, -6.f, -2.f, 6.f, 6.f, 2.f);
    for (int k = -10; k <= 10; ++k) {
        const float f = (float)(((double)k + 0.5) * cell);
        p.push_back(P3{f, f, 0.f}); p.push_back(P3{nextafterf(f, -INFINITY), 0.f, f * 0.25f}); p.push_back(P3{0.f, nextafterf(f, INFINITY), 0.f});
    }
    Ix ix; Cloud c; c.set(p);
    Opt o; o.cell = cell; o.shift = 0.5; o.allow_hint = true;
    step(ix, c, o, fresh(), "fresh");
    // (cell 0.3: 38 475 cells keep the first build's tiles of 2^10 cells, so its header and its layout -- planned without cuts -- serve at once)
    step(ix, c, o, cell < 0.5 ? reused(4, 8) : boxed(8), "tiles_by_cells");
    step(ix, c, o, reused(2, 8), "reuse_layout");
    Ix iy; iy.g.prefer_one_level = true;
    step(iy, c, o, one_level(), "one_level");
}
void c_shifted_cell_1() { shifted_case(1.0); }
void c_shifted_cell_03() { shifted_case(0.3); }

// ---- filtered builds: only the points inside a region's mask (macro cells of 2 x 2 x 2 cells) --------------------------------------------
void filtered_dense(bool tail) {      // eight per thread, tiles that are cut: bin 2, tile 8 / 6
    Rng r(51);
    Pts p = walk_points(r);
    Ix ix; Cloud c; c.set(p);
    Opt o; o.allow_hint = true;
    step(ix, c, o, fresh(), "fresh");
    step(ix, c, o, boxed(8, -1, 7), "tiles_by_cells");
    step(ix, c, o, reused(2, 8), "full_with_layout");
    const MaskKind kinds[3] = {kMaskChecker, kMaskZero, kMaskOne};
    const char* names[3] = {"mask_splits_tiles", "mask_all_zero", "mask_all_one"};
    for (int k = 0; k < 3; ++k) {
        Opt f = o; f.mask = kinds[k]; f.want_tail = tail;
        step(ix, c, f, filt(reused(2, tail ? 6 : 8), 0, tail ? 1 : 0), names[k]);
    }
    add_box(p, r, 20, -9.f, -9.f, -1.f, 9.f, 9.f, 5.f); c.set(p);
    step(ix, c, o, reused(2, 8), "full_after_filtered");      // the layout was handed on as it came: a full build is complete
}
void c_filtered_bin_pass() { filtered_dense(false); }
void c_filtered_tail_per8() { filtered_dense(true); }
void c_filtered_tail_per16() {      // sixteen per thread, nothing cut: bin 4, tile 7
    Rng r(52);
    Pts p; p.push_back(P3{0.f, 0.f, 0.f}); p.push_back(P3{3.99f, 3.99f, 0.99f});
    add_box(p, r, 99998, 0.f, 0.f, 0.f, 3.99f, 3.99f, 0.99f);      // 8 x 8 x 5 = 320 cells, tiles of 4 cells
    Ix ix; Cloud c; c.set(p);
    Opt o; o.allow_hint = true;
    step(ix, c, o, fresh(), "fresh");
    step(ix, c, o, boxed(9, -1, 2), "tiles_by_cells");
    Opt f = o; f.mask = kMaskChecker; f.want_tail = true; f.min_points = 6;
    step(ix, c, f, filt(reused(4, 7), 0, 1), "mask_splits_tiles");
    f.mask = kMaskOne;
    step(ix, c, f, filt(reused(4, 7), 0, 1), "mask_all_one");
    step(ix, c, o, reused(4, 9), "full_after_filtered");
}
// the threshold of the keep pass: 2 000 000 points and one fewer, over 96 x 96 x 96 m (100^3 cells: eight per thread, tiles that are cut) ...
void c_filtered_keep_2m() {
    Rng r(61);
    Pts p; p.reserve(2000000); p.push_back(P3{0.f, 0.f, 0.f}); p.push_back(P3{95.5f, 95.5f, 95.5f});
    add_box(p, r, 1999998, 0.f, 0.f, 0.f, 95.5f, 95.5f, 95.5f);
    Cloud c; c.set(p);
    Opt o; o.allow_hint = true;
    Opt f = o; f.mask = kMaskChecker;
    {
        Ix ix;
        step(ix, c, o, fresh(), "fresh");
        step(ix, c, o, boxed(8, -1, 8), "tiles_by_cells");
        step(ix, c, f, filt(reused(0, 8), 1), "keep_pass_packed_sub");
        step(ix, c, o, reused(2, 8), "full_after_filtered");
    }
    c.n = 1999999;      // (the same buffer: its last point is left out; the box is the first two points')
    Ix iy;
    step(iy, c, o, fresh(), "fresh_below");
    step(iy, c, o, boxed(8, -1, 8), "tiles_by_cells_below");
    step(iy, c, f, filt(reused(2, 8), 0), "mask_in_bin_pass");
}
// ... and over 20 x 20 x 8 m (sixteen per thread, nothing cut), 12-byte points: the packed variant without the tiles' words, the keep pass's other instantiation
void c_filtered_keep_2m_dense() {
    Rng r(62);
    Pts p; p.reserve(2000000); p.push_back(P3{-10.f, -10.f, -2.f}); p.push_back(P3{9.5f, 9.5f, 5.5f});
    add_box(p, r, 1999998, -10.f, -10.f, -2.f, 9.5f, 9.5f, 5.5f);
    Ix ix; Cloud c; c.set(p, 3);
    Opt o; o.allow_hint = true;
    step(ix, c, o, fresh(), "fresh");
    step(ix, c, o, boxed(9, -1, 2), "tiles_by_cells");
    Opt f = o; f.mask = kMaskChecker; f.want_tail = true; f.min_points = 300;
    step(ix, c, f, filt(reused(1, 7), 1, 1), "keep_pass_packed");
    step(ix, c, o, reused(4, 9), "full_after_filtered");
}

// ---- twin: one box pass writes the headers of two indices over the same cloud --------------------------------------------------------------
void c_twin_preset() {
    Rng r(71);
    Ix a, b; Cloud c; c.set(small_points(r, 5000));
    a.g.twin = &b.g; a.g.twin_cell = 2.0;
    Opt o1, o2, o4; o2.cell = 2.0; o4.cell = 4.0;
    index_ref::Clamp none;
    const index_ref::Header hb = index_ref::fresh_header(c.hp(), c.n, c.stride, 2.0, 0.0, 0, none, 0, 0, (uint64_t)1 << 20);
    step(a, c, o1, fresh(), "feeds_twin");
    Expect pre = fresh(); pre.preset = 1;
    step(b, c, o2, pre, "preset", &hb);
    step(a, c, o1, boxed(8), "feeds_twin_again");
    step(b, c, o4, boxed(8), "refused_other_cell");      // a header written for cell 2 does not serve cell 4: a box pass of its own
    step(a, c, o1, boxed(8), "feeds_twin_third");
    c.n -= 1;
    step(b, c, o2, boxed(8), "refused_other_cloud");
}

// ---- one index through unrelated clouds ------------------------------------------------------------------------------------------------------
void unrelated(bool no_hints) {
    Rng r(81);
    Ix ix; ix.g.no_hints = no_hints;
    Cloud big, tiny; big.set(walk_points(r));
    Pts t; add_box(t, r, 50, 500.f, 500.f, 50.f, 503.f, 502.f, 51.f); tiny.set(t);
    Opt o; o.allow_hint = true;
    step(ix, big, o, fresh(), "big_fresh");
    step(ix, big, o, boxed(8, -1, 7), "big_tiles_by_cells");
    step(ix, big, o, no_hints ? boxed(8, -1, 7) : reused(2, 8), "big_again");
    if (no_hints) { step(ix, tiny, o, boxed(8, -1, 7), "tiny_elsewhere"); step(ix, tiny, o, boxed(8), "tiny_again"); }
    else {
        step(ix, tiny, o, reused(2, 8), "tiny_outside_old_box");      // every point outside: stale
        ix.g.hint_margin = 8; ix.g.cells_hint = 0;
        step(ix, tiny, o, fresh(), "tiny_rebuilt");
        step(ix, tiny, o, boxed(8), "tiny_tiles_by_cells");
        step(ix, tiny, o, reused(2, 8), "tiny_reuse");
    }
    // with hints: outside the tiny box, stale again.  Without: the cells the tiny cloud left as a bound (2 * 210 + 64 -> 1 024) do not hold the big one:
    // overflow, the bound is lifted (grow_cells), and the rebuild is exact
    step(ix, big, o, no_hints ? boxed(8) : reused(2, 8), "big_back");
    if (no_hints) {
        std::string err;
        if (ix.g.grow_cells(6912, &err) != hipSuccess) mismatch("grow_cells: %s", err.c_str());
        step(ix, big, o, boxed(8, -1, 7), "big_after_grow_cells");
    }
}
void c_unrelated_hints() { unrelated(false); }
void c_unrelated_no_hints() { unrelated(true); }

const Case kCases[] = {
    {"one_level/n0", c_one_level_n<0>}, {"one_level/n1", c_one_level_n<1>}, {"one_level/n255", c_one_level_n<255>}, {"one_level/n256", c_one_level_n<256>}, {"one_level/n257", c_one_level_n<257>},
    {"one_level/one_cell", c_one_level_one_cell}, {"one_level/scan_tile_boundary", c_one_level_scan_tiles}, {"one_level/non_finite", c_one_level_non_finite}, {"one_level/all_non_finite", c_one_level_all_non_finite},
    {"fresh/n0", c_fresh_n<0>}, {"fresh/n1", c_fresh_n<1>}, {"fresh/n255", c_fresh_n<255>}, {"fresh/n256", c_fresh_n<256>}, {"fresh/n257", c_fresh_n<257>}, {"fresh/n2047", c_fresh_n<2047>}, {"fresh/n2048", c_fresh_n<2048>},
    {"fresh/n2049", c_fresh_n<2049>}, {"fresh/n5000_partial_chunk", c_fresh_n<5000>}, {"fresh/non_finite", c_fresh_non_finite}, {"fresh/all_non_finite", c_fresh_all_non_finite},
    {"fresh/stride4_vec", c_fresh_stride<4, 0>}, {"fresh/stride8_vec", c_fresh_stride<8, 0>}, {"fresh/stride3", c_fresh_stride<3, 0>}, {"fresh/stride5", c_fresh_stride<5, 0>}, {"fresh/stride4_one_float_in", c_fresh_stride<4, 1>},
    {"walk/vec", c_walk_vec}, {"walk/not_vec", c_walk_not_vec}, {"dense_coherent/walk", c_walk_coherent},
    {"room/exactly_full", c_room_exact}, {"room/one_too_many", c_room_plus_one},
    {"stale/six_faces", c_stale_faces}, {"overflow/one_cell_too_many", c_overflow}, {"clamp/six_faces", c_clamp_faces},
    {"sparse/rings", c_sparse_rings}, {"sparse/shuffled", c_sparse_shuffled}, {"sparse/coherent_rings", c_sparse_coherent_rings}, {"sparse/coherent_shuffled", c_sparse_coherent_shuffled},
    {"sparse/cut_clusters", c_sparse_cut_clusters}, {"sparse/cut_coherent_clusters", c_sparse_cut_coherent_clusters}, {"sparse/not_split", c_sparse_not_split},
    {"pcl/leaf_0.1", c_pcl_leaf_01}, {"pcl/leaf_0.5", c_pcl_leaf_05}, {"shifted/cell_1", c_shifted_cell_1}, {"shifted/cell_0.3", c_shifted_cell_03},
    {"filtered/bin_pass", c_filtered_bin_pass}, {"filtered/tail_per8", c_filtered_tail_per8}, {"filtered/tail_per16", c_filtered_tail_per16},
    {"filtered/keep_2m", c_filtered_keep_2m}, {"filtered/keep_2m_dense", c_filtered_keep_2m_dense},
    {"twin/preset", c_twin_preset}, {"unrelated/hints", c_unrelated_hints}, {"unrelated/no_hints", c_unrelated_no_hints},
};

// ---- --self: the reference against tables worked out by hand ------------------------------------------------------------------------------------
int g_self_bad = 0;
void want(bool ok, const char* what) { if (!ok) { printf("self: FAILED %s\n", what); ++g_self_bad; } }
bool starts_are(const index_ref::Table& t, std::vector<std::pair<size_t, uint32_t>> steps) {      // cell_start[c] = the value of the last step at or below c
    for (size_t c = 0; c < t.cell_start.size(); ++c) { uint32_t v = 0; for (auto& s : steps) if (c >= s.first) v = s.second; if (t.cell_start[c] != v) return false; }
    return true;
}
int self_check() {
    using namespace index_ref;
    Clamp none;
    {   // A. 1 m cells.  x in {0.25, 0.5, 2.5} -> cells 0 .. 2, y and z one cell: org = (-2, -2, -2), dims = (7, 5, 5), 175 cells.
        // (0.5, 0.5, 0.5) and (0.25, 0.75, 0.9): cell (2, 2, 2), key (2 * 5 + 2) * 7 + 2 = 86.  (2.5, 0.5, 0.5): (4, 2, 2), key 88.  The NaN point: nowhere.
        const float p[] = {0.5f, 0.5f, 0.5f, 9, 2.5f, 0.5f, 0.5f, 9, 0.25f, 0.75f, 0.9f, 9, NAN, 0.f, 0.f, 9};
        const Header h = fresh_header(p, 4, 4, 1.0, 0.0, 0, none, 0, 0, 1 << 20);
        want(h.org[0] == -2 && h.org[1] == -2 && h.org[2] == -2 && h.dims[0] == 7 && h.dims[1] == 5 && h.dims[2] == 5 && h.n_cells == 175 && !h.empty && !h.overflow && h.n_points == 4, "A header");
        want(h.origin[0] == -2.0 && h.origin[2] == -2.0, "A origin");
        const Table t = build_table(h, p, 4, 4);
        want(t.order == std::vector<uint32_t>({0, 2, 1}) && t.sum_sq == 5 && t.non_finite == 1 && t.outside == 0, "A order");
        want(starts_are(t, {{0, 0}, {87, 2}, {89, 3}}), "A cell_start");
        // the same lattice reused: x = 2.9999 is the last cell inside (4), x = 3.5 the first pad cell, x = 5.5 the second, x = 7.5 beyond the table
        want(cell_of(h, 2.9999f, 0.5f, 0.5f) == 88 && cell_of(h, 3.5f, 0.5f, 0.5f) == kOutside && cell_of(h, 5.5f, 0.5f, 0.5f) == kOutside && cell_of(h, 7.5f, 0.5f, 0.5f) == kOutside, "A upper face");
        want(cell_of(h, 0.f, 0.f, 0.f) == 86 && cell_of(h, -0.0001f, 0.5f, 0.5f) == kOutside && cell_of(h, 0.5f, 0.5f, INFINITY) == kNonFinite, "A lower face");
        // a table that holds 175 cells + 1 start needs capacity 176
        want(fresh_header(p, 4, 4, 1.0, 0.0, 0, none, 0, 0, 175).overflow == 1 && fresh_header(p, 4, 4, 1.0, 0.0, 0, none, 0, 0, 175).n_cells == 175 && fresh_header(p, 4, 4, 1.0, 0.0, 0, none, 0, 0, 176).overflow == 0, "A overflow");
        // margin 3: three cells more in x and y, two in z: dims (13, 11, 9), org (-5, -5, -4)
        const Header m = fresh_header(p, 4, 4, 1.0, 0.0, 0, none, 3, 0, 1 << 20);
        want(m.dims[0] == 13 && m.dims[1] == 11 && m.dims[2] == 9 && m.org[0] == -5 && m.org[2] == -4, "A margin");
        // clamp to [0, 1]^3: the upper x face is cut (bit 3); hi = 1 -> cells 0 .. 1, dims (6, 5, 5); (2.5, ..) is outside; key of (2, 2, 2) = (2 * 5 + 2) * 6 + 2 = 74
        Clamp cl; cl.use = true; for (int d = 0; d < 3; ++d) { cl.lo[d] = 0.0; cl.hi[d] = 1.0; }
        const Header hc = fresh_header(p, 4, 4, 1.0, 0.0, 0, cl, 0, 0, 1 << 20);
        want(hc.clamped == 1 && hc.cut_mask == 8 && hc.dims[0] == 6 && hc.n_cells == 150, "A clamp header");
        const Table tc = build_table(hc, p, 4, 4);
        want(tc.order == std::vector<uint32_t>({0, 2}) && tc.outside == 1 && starts_are(tc, {{0, 0}, {75, 2}}), "A clamp table");
        // region mask, macro cells of 2 x 2 x 2: macro dims (4, 3, 3); cell (2, 2, 2) -> macro (1, 1, 1) = (1 * 3 + 1) * 4 + 1 = 17, cell (4, 2, 2) -> macro (2, 1, 1) = 18
        std::vector<uint8_t> mb(macro_count(h, 1), 0); mb[18] = 1;
        Mask mk; mk.bytes = mb.data(); mk.mshift = 1;
        want(macro_count(h, 1) == 36 && macro_of(h, 1, 2, 2, 2) == 17 && macro_of(h, 1, 4, 2, 2) == 18 && mask_holds_cell(h, mk, 88) && !mask_holds_cell(h, mk, 86), "A macro cells");
        const Table tm = build_table(h, p, 4, 4, &mk);
        want(tm.order == std::vector<uint32_t>({1}) && tm.masked == 2 && starts_are(tm, {{0, 0}, {89, 1}}), "A masked table");
    }
    {   // B. 0.5 m cells, negative coordinates, a point ON a face.  (-0.25, -0.75, 0): x / cell = -0.5 -> -1, -1.5 -> -2, 0.  (-0.5, -0.5, 0.49): -1 (on the face: the
        // cell that starts there), -1, 0.  first = (-1, -2, 0), last = (-1, -1, 0): org = (-3, -4, -2), dims (5, 6, 5) = 150, origin = org / 2.
        // keys: (2, 2, 2) -> (2 * 6 + 2) * 5 + 2 = 72; (2, 3, 2) -> (2 * 6 + 3) * 5 + 2 = 77
        const float p[] = {-0.25f, -0.75f, 0.f, -0.5f, -0.5f, 0.49f};
        const Header h = fresh_header(p, 2, 3, 0.5, 0.0, 0, none, 0, 0, 1 << 20);
        want(h.org[0] == -3 && h.org[1] == -4 && h.org[2] == -2 && h.dims[0] == 5 && h.dims[1] == 6 && h.dims[2] == 5 && h.origin[0] == -1.5 && h.origin[1] == -2.0 && h.origin[2] == -1.0, "B header");
        const Table t = build_table(h, p, 2, 3);
        want(t.order == std::vector<uint32_t>({0, 1}) && starts_are(t, {{0, 0}, {73, 1}, {78, 2}}) && t.sum_sq == 2, "B table");
    }
    {   // C. shift 0.5 (VGICP's voxels), 1 m: x = 0.5 lies ON the half-cell plane: floor(0.5 - 0.5) = 0; 0.49 -> -1.  y = z = 0 -> -1.
        // first (-1, -1, -1), last (0, -1, -1): org (-3, -3, -3), dims (6, 5, 5), origin = (org + 0.5): keys (3, 2, 2) -> (2 * 5 + 2) * 6 + 3 = 75, (2, 2, 2) -> 74
        const float p[] = {0.5f, 0.f, 0.f, 0.49f, 0.f, 0.f};
        const Header h = fresh_header(p, 2, 3, 1.0, 0.5, 0, none, 0, 0, 1 << 20);
        want(h.org[0] == -3 && h.dims[0] == 6 && h.dims[1] == 5 && h.origin[0] == -2.5 && h.n_cells == 150, "C header");
        const Table t = build_table(h, p, 2, 3);
        want(t.order == std::vector<uint32_t>({1, 0}) && starts_are(t, {{0, 0}, {75, 1}, {76, 2}}), "C table");
    }
    {   // D. pcl::VoxelGrid's lattice, leaf 0.5: floor(x * 2) = 0, 1, -1 -> min_b = (-1, 0, 0), dims (3, 1, 1): no pad cells.  One margin voxel in x and y, two in z: dims (5, 3, 5)
        const float p[] = {0.1f, 0.1f, 0.1f, 0.6f, 0.1f, 0.1f, -0.1f, 0.1f, 0.1f};
        const Header h = fresh_header(p, 3, 3, 0.5, 0.0, 1, none, 0, 0, 1 << 20);
        want(h.pcl_mode == 1 && h.min_b[0] == -1 && h.min_b[1] == 0 && h.dims[0] == 3 && h.dims[1] == 1 && h.dims[2] == 1 && h.n_cells == 3 && h.inv_leaf_f == 2.0f, "D header");
        const Table t = build_table(h, p, 3, 3);
        want(t.order == std::vector<uint32_t>({2, 0, 1}) && t.cell_start == std::vector<uint32_t>({0, 1, 2, 3}) && t.sum_sq == 3, "D table");
        want(cell_of(h, 1.0f, 0.1f, 0.1f) == kOutside && cell_of(h, 0.999f, 0.1f, 0.1f) == 2 && cell_of(h, -0.5f, 0.1f, 0.1f) == 0 && cell_of(h, -0.5001f, 0.1f, 0.1f) == kOutside, "D faces");
        const Header m = fresh_header(p, 3, 3, 0.5, 0.0, 1, none, 1, 2, 1 << 20);
        want(m.dims[0] == 5 && m.dims[1] == 3 && m.dims[2] == 5 && m.min_b[0] == -2 && m.min_b[2] == -2, "D margins");
    }
    {   // E. nothing finite: empty, the box of the origin: dims (5, 5, 5)
        const float p[] = {NAN, 0.f, 0.f, 0.f, INFINITY, 0.f};
        const Header h = fresh_header(p, 2, 3, 1.0, 0.0, 0, none, 8, 0, 1 << 20);
        want(h.empty == 1 && h.n_cells == 125 && h.dims[0] == 5, "E empty");
    }
    if (g_self_bad) { printf("index_check --self FAILED\n"); return 1; }
    printf("index_check --self ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const char* only = nullptr;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--self")) return self_check();
        if (!strcmp(argv[i], "--list")) { for (const Case& c : kCases) printf("%s\n", c.name); return 0; }
        if (!strcmp(argv[i], "--plan")) g_dry = true;
        else if (!strcmp(argv[i], "--case") && i + 1 < argc) only = argv[++i];      // cases whose name begins so (the coverage check is then skipped)
        else { fprintf(stderr, "usage: index_check [--self | --list | --plan] [--case PREFIX]\n"); return 2; }
    }
    if (!g_dry) { HIPX(hipSetDevice(0)); HIPX(hipFree(nullptr)); }
    int failed = 0, ran = 0;
    for (const Case& c : kCases) {
        if (only && strncmp(c.name, only, strlen(only)) != 0) continue;
        g_case = c.name; g_case_ok = true;
        printf("case %s\n", c.name);
        c.fn();
        if (!g_dry) HIPX(hipDeviceSynchronize());
        printf("case %s %s\n", c.name, g_case_ok ? "PASS" : "FAIL");
        fflush(stdout);
        failed += g_case_ok ? 0 : 1; ++ran;
    }
    if (g_dry) { printf("index_check --plan %s: %d cases, %d with a plan other than the expected one\n", failed ? "FAILED" : "ok", ran, failed); return failed ? 1 : 0; }
    int nbin = 0, ntile = 0;
    printf("coverage bin=");
    for (int i = 0; i < pcr::kBinVariants; ++i) if (g_cov.bin[i]) { printf("%s%d", nbin ? "," : "", i); ++nbin; }
    printf(" tile=");
    for (int i = 0; i < pcr::kTileVariants; ++i) if (g_cov.tile[i]) { printf("%s%d", ntile ? "," : "", i); ++ntile; }
    printf(" bins=%d/%d tiles=%d/%d place_vec=%d place_not_vec=%d keep=%d keep_vec=%d keep_not_vec=%d one_level=%d\n", nbin, pcr::kBinVariants, ntile, pcr::kTileVariants, g_cov.place[1] ? 1 : 0, g_cov.place[0] ? 1 : 0,
           (g_cov.keep[0] || g_cov.keep[1]) ? 1 : 0, g_cov.keep[1] ? 1 : 0, g_cov.keep[0] ? 1 : 0, g_cov.one_level ? 1 : 0);
    const bool covered = nbin == pcr::kBinVariants && ntile == pcr::kTileVariants && g_cov.place[0] && g_cov.place[1] && g_cov.keep[0] && g_cov.keep[1] && g_cov.one_level;
    if (!only && !covered) { printf("index_check FAILED: a kernel variant was reached by no case that passed\n"); return 1; }
    if (failed) { printf("index_check FAILED: %d of %d cases\n", failed, ran); return 1; }
    printf("index_check ok: %d cases\n", ran);
    return 0;
}
