// index_ref.hpp -- what a build of the grid index must produce, restated as a plain counting sort on the host (no HIP header, no code shared
// with the kernels of csrc/grid_index.hip: the rules below are written from the documentation of GridHeader in csrc/pcr_internal.h and from
// the rule grid_bbox_header_kernel states for a fresh box).  host/index_check.cpp compares every build on the device with it, exactly.
//
//   cell of a point      floor(x / cell - shift) - org per axis, in double; x fastest: key = (cz * dims[1] + cy) * dims[0] + cx.
//                        kPad = 2 pad cells on every side hold no point: a point whose cell is not in [2, dims - 2) is OUTSIDE the lattice.
//   pcl_mode lattice     (int)(floorf(x * inv_leaf) - (float)min_b), all in float, no pad cells: pcl::VoxelGrid's own arithmetic.
//   fresh box            lo / hi = the float minimum / maximum of the finite points per axis (none: empty, lo = hi = 0), cut to the clamp box
//                        when one is given (cut_mask: bit d = points below the lower face of axis d, bit 3 + d = above the upper one);
//                        first cell floor(lo / cell - shift), last cell floor(hi / cell - shift), `margin` cells more on both sides
//                        (x and y; z at most 2) unless empty; org = first - 2, dims = last - first + 1 + 4.  More cells than the table
//                        holds (cells + 1 > capacity): overflow, n_cells = the cells needed.
//   region mask          one byte per macro cell of 2^mshift cells per axis, macro dims = ceil(dims / 2^mshift), x fastest.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace index_ref {

static constexpr int kPadCells = 2;

struct Header {
    double origin[3], org[3], cell, inv_cell, shift;
    int32_t dims[3];
    uint32_t n_points;
    uint64_t n_cells;
    int32_t overflow, empty, pcl_mode;
    float inv_leaf_f;
    int32_t min_b[3], too_fine, clamped, cut_mask;
};
struct Clamp { bool use = false; double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}; };
struct Mask { const uint8_t* bytes = nullptr; int mshift = 0; };

inline bool finite3(float x, float y, float z) { return std::isfinite(x) && std::isfinite(y) && std::isfinite(z); }

inline Header fresh_header(const float* pts, size_t n, size_t stride, double cell, double shift, int pcl_mode, const Clamp& clamp, int margin_xy,
                           int margin_z_pcl, uint64_t capacity) {
    Header h;
    h.cell = cell; h.inv_cell = 1.0 / cell; h.shift = shift; h.n_points = (uint32_t)n;      // (n_points: the points the build was given)
    h.empty = 0; h.overflow = 0; h.pcl_mode = pcl_mode; h.inv_leaf_f = 1.0f / (float)cell; h.too_fine = 0;
    h.min_b[0] = h.min_b[1] = h.min_b[2] = 0;
    h.clamped = (clamp.use && !pcl_mode) ? 1 : 0; h.cut_mask = 0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = 0; i < n; ++i) {
        const float* p = pts + i * stride;
        if (!finite3(p[0], p[1], p[2])) continue;
        for (int d = 0; d < 3; ++d) { lo[d] = std::min(lo[d], p[d]); hi[d] = std::max(hi[d], p[d]); }
    }
    double nc = 1.0, nc_tight = 1.0;
    int mg_xy = margin_xy, mg_z = margin_z_pcl;
    if (pcl_mode) {      // the margins are dropped when the padded box would not fit a dense table
        double padded = 1.0;
        for (int d = 0; d < 3; ++d) {
            if (!(lo[d] <= hi[d])) continue;
            nc_tight *= (double)truncf((hi[d] - lo[d]) * h.inv_leaf_f) + 1.0;
            padded *= (double)floorf(hi[d] * h.inv_leaf_f) - (double)floorf(lo[d] * h.inv_leaf_f) + 1.0 + 2.0 * (d < 2 ? mg_xy : mg_z);
        }
        if (padded > 4.0e9) mg_xy = mg_z = 0;
    }
    for (int d = 0; d < 3; ++d) {
        float l = lo[d], u = hi[d];
        if (!(l <= u)) { h.empty = 1; l = u = 0.f; }
        if (h.clamped) {
            if (l < (float)clamp.lo[d]) h.cut_mask |= 1 << d;
            if (u > (float)clamp.hi[d]) h.cut_mask |= 8 << d;
            l = std::max(l, (float)clamp.lo[d]); u = std::min(u, (float)clamp.hi[d]);
            if (!(l <= u)) { h.empty = 1; l = u = 0.f; }
        }
        if (pcl_mode) {
            float fl = floorf(l * h.inv_leaf_f), fu = floorf(u * h.inv_leaf_f);
            const int mg = d < 2 ? mg_xy : mg_z;
            if (!h.empty && mg) { fl -= (float)mg; fu += (float)mg; }
            const double dim = (double)fu - (double)fl + 1.0;
            h.min_b[d] = fabsf(fl) < 2.0e9f ? (int32_t)fl : 0;
            h.org[d] = (double)fl; h.origin[d] = (double)fl * cell;
            h.dims[d] = dim < 2.0e9 ? (int32_t)dim : 0x7fffffff;
            nc *= dim;
            continue;
        }
        double first = floor((double)l / cell - shift), last = floor((double)u / cell - shift);
        if (!h.empty) { const int mg = d < 2 ? margin_xy : std::min(margin_xy, 2); first -= mg; last += mg; }
        h.org[d] = first - kPadCells;
        h.origin[d] = (first - kPadCells + shift) * cell;
        const double dim = last - first + 1.0 + 2.0 * kPadCells;
        h.dims[d] = dim < 2.0e9 ? (int32_t)dim : 0x7fffffff;
        nc *= dim;
    }
    if (pcl_mode && nc_tight > 2147483647.0) h.too_fine = 1;
    if (h.too_fine) { h.overflow = 0; h.empty = 1; h.n_cells = 1; }
    else if (nc + 1.0 > (double)capacity || nc > 4.0e9) { h.overflow = 1; h.n_cells = nc < 1.8e19 ? (uint64_t)nc : ~0ull; }
    else h.n_cells = (uint64_t)h.dims[0] * (uint64_t)h.dims[1] * (uint64_t)h.dims[2];
    return h;
}

static constexpr int64_t kNonFinite = -1, kOutside = -2;
// the linear cell of a point in the lattice `h`, kNonFinite, or kOutside (cxyz: the cell's coordinates too)
inline int64_t cell_of(const Header& h, float x, float y, float z, int32_t* cxyz = nullptr) {
    if (!finite3(x, y, z)) return kNonFinite;
    const float p[3] = {x, y, z};
    int64_t c[3];
    for (int d = 0; d < 3; ++d) {
        if (h.pcl_mode) {
            const float v = floorf(p[d] * h.inv_leaf_f) - (float)h.min_b[d];
            if (!(v >= 0.f && v < (float)h.dims[d])) return kOutside;
            c[d] = (int64_t)(int)v;
            if (c[d] >= h.dims[d]) return kOutside;
        } else {
            const double v = floor((double)p[d] / h.cell - h.shift) - h.org[d];
            if (!(v >= (double)kPadCells && v < (double)(h.dims[d] - kPadCells))) return kOutside;
            c[d] = (int64_t)v;
        }
    }
    if (cxyz) { cxyz[0] = (int32_t)c[0]; cxyz[1] = (int32_t)c[1]; cxyz[2] = (int32_t)c[2]; }
    return (c[2] * h.dims[1] + c[1]) * h.dims[0] + c[0];
}

inline uint32_t macro_dim(const Header& h, int mshift, int d) { return ((uint32_t)h.dims[d] + (1u << mshift) - 1u) >> mshift; }
inline size_t macro_count(const Header& h, int mshift) { return (size_t)macro_dim(h, mshift, 0) * macro_dim(h, mshift, 1) * macro_dim(h, mshift, 2); }
inline size_t macro_of(const Header& h, int mshift, int32_t cx, int32_t cy, int32_t cz) {
    return ((size_t)(cz >> mshift) * macro_dim(h, mshift, 1) + (size_t)(cy >> mshift)) * macro_dim(h, mshift, 0) + (size_t)(cx >> mshift);
}
inline bool mask_holds_cell(const Header& h, const Mask& m, uint64_t key) {
    const uint64_t d0 = (uint64_t)h.dims[0], d1 = (uint64_t)h.dims[1];
    const int32_t cx = (int32_t)(key % d0), cy = (int32_t)((key / d0) % d1), cz = (int32_t)(key / (d0 * d1));
    return m.bytes[macro_of(h, m.mshift, cx, cy, cz)] != 0;
}

struct Table {
    std::vector<uint32_t> cell_start;      // n_cells + 1
    std::vector<uint32_t> order;           // original indices, by cell and ascending inside a cell
    unsigned long long sum_sq = 0;         // sum over the cells of count^2
    size_t outside = 0, masked = 0, non_finite = 0;
};
// (mask: only the points whose cell's macro cell is marked are indexed)
inline Table build_table(const Header& h, const float* pts, size_t n, size_t stride, const Mask* mask = nullptr) {
    Table t;
    t.cell_start.assign((size_t)h.n_cells + 1, 0u);
    std::vector<int64_t> key(n);
    for (size_t i = 0; i < n; ++i) {
        const float* p = pts + i * stride;
        int32_t c[3];
        int64_t k = cell_of(h, p[0], p[1], p[2], c);
        if (k == kNonFinite) ++t.non_finite;
        else if (k == kOutside) ++t.outside;
        else if (mask && mask->bytes[macro_of(h, mask->mshift, c[0], c[1], c[2])] == 0) { k = -3; ++t.masked; }
        key[i] = k;
        if (k >= 0) ++t.cell_start[(size_t)k + 1];
    }
    for (size_t c = 0; c < (size_t)h.n_cells; ++c) {
        const unsigned long long cnt = t.cell_start[c + 1];
        t.sum_sq += cnt * cnt;
        t.cell_start[c + 1] += t.cell_start[c];
    }
    t.order.resize(t.cell_start[(size_t)h.n_cells]);
    std::vector<uint32_t> fill(t.cell_start.begin(), t.cell_start.end() - 1);
    for (size_t i = 0; i < n; ++i) if (key[i] >= 0) t.order[fill[(size_t)key[i]]++] = (uint32_t)i;
    return t;
}

}  // namespace index_ref
