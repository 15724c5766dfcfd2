// sparse_walk.h -- the walk of the sparse target index (sparse_index.hip), written once for the device and the host (host/sparse_index_check.cpp
// runs it on the CPU against brute force and counts its look-ups; in the manner of graph_math.h and small_math.h).
//
// The index is two arrays in key order and nothing else: keys[j] = ((z << b1) | y) << b0 | x, the cell of stored point j relative to the
// cloud's box (cell edge `cell`, a power of two, so that x / cell is exact; b0, b1, b2 = the bits the three extents need), and pts[j] = its
// coordinates with the original row number.  There is no cell table: the points of the cells [a, b) of one row are
// [lower_bound(key(a)), lower_bound(key(b))), and because the key is linear a band of rows of one z layer is contiguous too.
//
// Exactness is knn_query.hip's: every bound is a distance to a face of the block of cells actually scanned less the slop (slab_gap /
// slop_of below, shared with that file), a row is passed over only when its bound EXCEEDS the distance it competes with, and the visitor
// alone computes distances and decides by (d2, original index).  The walk never assumes that the query lies in the centre cell.
//
// Cost: a look-up is one binary search.  The k-NN walk makes at most kRingLookups of them in its two rings and one for the seed; the box
// scan (of the k-NN walk's third step, and the whole of a radius query) makes at most 1 + kRowLookups R + kLayerLookups L, R = the
// occupied rows of the (z, y) range of the block it scans, L = the occupied z layers of its z range -- whatever the block's volume.
// Where the numbers come from is said at box_scan.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define SW_FN __host__ __device__ __forceinline__
#else
#define SW_FN inline
#endif

namespace pcr {
namespace sw {

static constexpr int kRingLookups = 102, kRowLookups = 5, kLayerLookups = 2;

SW_FN double slop_of(double face, double q, double cell) { return (fabs(face) + fabs(q) + cell) * 0x1p-20; }

// distance from q to the slab of cells i of one axis (0 inside it), never more than the true gap to any point the build put there
SW_FN double slab_gap(double o, long long i, double cell, double q) {
    const double lo = (o + (double)i) * cell, hi = (o + (double)i + 1.0) * cell;
    const double g = fmax(fmax(lo - q, q - hi), 0.0);
    return fmax(g - slop_of(fmax(fabs(lo), fabs(hi)), q, cell), 0.0);
}

struct alignas(16) Point { float x, y, z; uint32_t row; };      // (the dense index's float4 with the row number in w)

struct View {
    const unsigned long long* keys;
    const Point* pts;
    uint32_t n;                   // stored points (the finite rows of the cloud)
    int32_t b0, b1, b2;           // key bits of x, y, z: b0 + b1 + b2 <= 63
    long long lo[3];              // lattice value floor(x / cell) of cell 0 of every axis (|.| < 2^62)
    unsigned long long ext[3];    // cells per axis, ext[a] <= 2^b_a
    double cell;
};

// The key layout a cloud asks for, from the least and the greatest lattice value floor(x / cell) of every axis over its finite rows (both
// integer-valued doubles).  Refused, never wrapped: a lattice value of 2^62 or beyond (kRefusedRange: the cell numbers are 64-bit integers),
// more than 63 key bits in all (kRefusedBits).  extd: the three extents as doubles, for the message.
static constexpr int kRefusedRange = 1, kRefusedBits = 2;
struct Layout {
    long long lo[3];
    unsigned long long ext[3];
    int32_t b[3], refused;
    double extd[3];
};
SW_FN int bits_of(unsigned long long v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }
SW_FN Layout layout_of(const double vmin[3], const double vmax[3]) {
    Layout l;
    l.refused = 0;
    for (int a = 0; a < 3; ++a) { l.lo[a] = 0; l.ext[a] = 1; l.b[a] = 0; l.extd[a] = vmax[a] - vmin[a] + 1.0; }
    for (int a = 0; a < 3; ++a) if (!(fabs(vmin[a]) < 0x1p62) || !(fabs(vmax[a]) < 0x1p62)) l.refused = kRefusedRange;
    if (l.refused) return l;
    for (int a = 0; a < 3; ++a) {
        l.lo[a] = (long long)vmin[a];
        l.ext[a] = (unsigned long long)((long long)vmax[a] - l.lo[a]) + 1ull;      // (< 2^63 + 1)
        l.b[a] = bits_of(l.ext[a] - 1ull);
    }
    if (l.b[0] + l.b[1] + l.b[2] > 63) l.refused = kRefusedBits;
    return l;
}

struct Box { long long x0, x1, y0, y1, z0, z1; };

// the walk's own cost, for the host (the device passes NoStats, which is nothing)
struct NoStats {
    SW_FN void lookup() {}
    SW_FN void scanned(uint32_t) {}
    SW_FN void boxed(const Box&) {}
};
struct Stats {
    unsigned long long lookups = 0, points = 0;
    int boxes = 0;                // box scans made (0 or 1)
    Box box = {0, 0, 0, 0, 0, 0};
    void lookup() { ++lookups; }
    void scanned(uint32_t m) { points += m; }
    void boxed(const Box& b) { ++boxes; box = b; }
};

SW_FN unsigned long long key_of(const View& v, long long z, long long y, long long x) {
    return ((((unsigned long long)z << v.b1) | (unsigned long long)y) << v.b0) | (unsigned long long)x;
}

// first position in [lo, hi) whose key is not below k
template <class S>
SW_FN uint32_t lower_bound(const View& v, uint32_t lo, uint32_t hi, unsigned long long k, S& st) {
    st.lookup();
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (v.keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the cell of q on axis a, clamped into the box
SW_FN long long cell_clamped(const View& v, int a, double q) {
    const double f = floor(q / v.cell) - (double)v.lo[a];
    if (!(f > 0.0)) return 0;
    if (f >= (double)(v.ext[a] - 1)) return (long long)(v.ext[a] - 1);
    return (long long)f;
}

// The cells of one axis that can hold a point within `radius` of q (radius may be +inf): false when there is none
SW_FN bool axis_range(const View& v, int a, double q, double radius, long long* lo, long long* hi) {
    const double A = q - radius, B = q + radius, o = (double)v.lo[a], top = (double)(v.ext[a] - 1);
    const double fl = floor((A - slop_of(A, q, v.cell)) / v.cell) - o, fh = floor((B + slop_of(B, q, v.cell)) / v.cell) - o;
    if (!(fh >= 0.0) || !(fl <= top)) return false;
    *lo = fl > 0.0 ? (fl >= top ? (long long)(v.ext[a] - 1) : (long long)fl) : 0;
    *hi = fh >= top ? (long long)(v.ext[a] - 1) : (long long)fh;
    return true;
}

// Every stored point of the block b, less those of the block *ex (the cells the rings have visited; nullptr: none), to vis.run(s, e) once, in
// key order.  vis.skip(g2): nothing at a squared distance of g2 or more can matter any longer.
// The scan reads the key where it stands, decodes its row, and moves on by one binary search -- to the first column of the block in that row,
// behind its last, to the row's end, to the next row or layer -- so it only ever stands on stored points.  Per occupied row of the block's
// (z, y) range: at most one look-up to reach the block's first column, one for the end of its columns, two around *ex, and one to leave the
// row: kRowLookups = 5.  Per occupied layer of its z range: at most one landing on a row below the block's rows and one on a row above them, a
// look-up each: kLayerLookups = 2 (a layer that vis.skip rules out costs one).  And the one that starts the scan.
template <class V, class S>
SW_FN void box_scan(const View& v, const Box& b, const Box* ex, double qy, double qz, V& vis, S& st) {
    st.boxed(b);
    const int sz = v.b0 + v.b1;
    const unsigned long long mx = (1ull << v.b0) - 1ull, my = (1ull << v.b1) - 1ull;
    uint32_t pos = lower_bound(v, 0u, v.n, key_of(v, b.z0, b.y0, b.x0), st);
    while (pos < v.n) {
        const unsigned long long k = v.keys[pos];
        const long long z = (long long)(k >> sz), y = (long long)((k >> v.b0) & my), x = (long long)(k & mx);
        if (z > b.z1) break;
        const double gz = slab_gap((double)v.lo[2], z, v.cell, qz);
        if (vis.skip(gz * gz) || y > b.y1) {      // on to the next layer
            if (z == b.z1) break;
            pos = lower_bound(v, pos, v.n, key_of(v, z + 1, b.y0, b.x0), st);
            continue;
        }
        if (y < b.y0) { pos = lower_bound(v, pos, v.n, key_of(v, z, b.y0, b.x0), st); continue; }
        const double gy = slab_gap((double)v.lo[1], y, v.cell, qy);
        if (x < b.x0 && !vis.skip(gy * gy + gz * gz)) { pos = lower_bound(v, pos, v.n, key_of(v, z, y, b.x0), st); continue; }
        if (x > b.x1 || vis.skip(gy * gy + gz * gz)) {      // on to the next row
            if (y == b.y1 && z == b.z1) break;
            pos = lower_bound(v, pos, v.n, y == b.y1 ? key_of(v, z + 1, b.y0, b.x0) : key_of(v, z, y + 1, b.x0), st);
            continue;
        }
        const uint32_t e = lower_bound(v, pos, v.n, key_of(v, z, y, b.x1) + 1ull, st);
        if (ex && z >= ex->z0 && z <= ex->z1 && y >= ex->y0 && y <= ex->y1 && ex->x0 <= b.x1 && ex->x1 >= b.x0) {
            const uint32_t a = lower_bound(v, pos, e, key_of(v, z, y, ex->x0), st), c = lower_bound(v, a, e, key_of(v, z, y, ex->x1) + 1ull, st);
            st.scanned(a - pos + e - c);
            vis.run(pos, a);
            vis.run(c, e);
        } else {
            st.scanned(e - pos);
            vis.run(pos, e);
        }
        pos = e;
    }
}

// pcr_radius_search: every stored point that can lie within `radius` of the query, once
template <class V, class S>
SW_FN void radius_walk(const View& v, double qx, double qy, double qz, double radius, V& vis, S& st) {
    Box b;
    if (v.n == 0 || !axis_range(v, 0, qx, radius, &b.x0, &b.x1) || !axis_range(v, 1, qy, radius, &b.y0, &b.y1) || !axis_range(v, 2, qz, radius, &b.z0, &b.z1)) return;
    box_scan(v, b, (const Box*)nullptr, qy, qz, vis, st);
}

// pcr_knn.  The visitor keeps the list of the K best by (d2, index): run(s, e) offers it the stored points [s, e), kth() is its K-th d2 (+inf
// while it holds fewer), max_d2(s, e) the largest d2 of [s, e) WITHOUT touching the list, cap(r2) tells it that the K-th distance cannot
// exceed r2, and skip(g2) = g2 > min(kth(), the cap).
//   1. rings 1 and 2 around the (clamped) centre cell, as knn_query.hip's: ring r adds the shell of the block [c - r, c + r]; a layer's band of
//      rows is found by two look-ups and every row inside it by searches of that band alone.  Ends as soon as the K-th distance is proven
//      final, or the block covers the box.  At most 3 (2 + 3 x 2) + 2 (2 + 5 x 2) + 3 (2 + 2 x 2 + 3 x 4) = 102 look-ups: kRingLookups.
//   2. the seed: any K stored points bound the K-th distance by their farthest; the K around the centre cell's place in key order are near
//      the query whenever anything is.  With the list's own K-th distance, the smaller is R^2.  (Fewer than K points stored: R = +inf.)
//   3. the box scan of [q - R, q + R] less the rings' block.  Everything within R is then in the list, and the K-th is among it.
// A query 15 km from the nearest point costs the rows of the cluster its box reaches, not the rings in between.
template <class V, class S>
SW_FN void knn_walk(const View& v, double qx, double qy, double qz, uint32_t K, V& vis, S& st) {
    if (v.n == 0) return;
    const long long cx = cell_clamped(v, 0, qx), cy = cell_clamped(v, 1, qy), cz = cell_clamped(v, 2, qz);
    const long long tx = (long long)(v.ext[0] - 1), ty = (long long)(v.ext[1] - 1), tz = (long long)(v.ext[2] - 1);
    const double ox = (double)v.lo[0], oy = (double)v.lo[1], oz = (double)v.lo[2];
    for (long long r = 1; r <= 2; ++r) {
        const long long z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < tz ? cz + r : tz, y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < ty ? cy + r : ty;
        const long long x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < tx ? cx + r : tx;
        for (long long z = z0; z <= z1; ++z) {
            const double gz = slab_gap(oz, z, v.cell, qz);
            if (vis.skip(gz * gz)) continue;
            const uint32_t bs = lower_bound(v, 0u, v.n, key_of(v, z, y0, 0), st);
            const uint32_t be = lower_bound(v, bs, v.n, key_of(v, z, y1, tx) + 1ull, st);
            if (bs == be) continue;
            for (long long y = y0; y <= y1; ++y) {
                const double gy = slab_gap(oy, y, v.cell, qy);
                if (vis.skip(gy * gy + gz * gz)) continue;      // the whole row is farther than the K-th distance as it stands
                const bool shell_row = r == 1 || z == cz - r || z == cz + r || y == cy - r || y == cy + r;
                if (shell_row) {
                    const uint32_t s = lower_bound(v, bs, be, key_of(v, z, y, x0), st), e = lower_bound(v, s, be, key_of(v, z, y, x1) + 1ull, st);
                    st.scanned(e - s);
                    vis.run(s, e);
                } else {
                    uint32_t s = bs;
                    if (cx - r >= 0) {
                        s = lower_bound(v, s, be, key_of(v, z, y, cx - r), st);
                        const uint32_t e = lower_bound(v, s, be, key_of(v, z, y, cx - r) + 1ull, st);
                        st.scanned(e - s);
                        vis.run(s, e);
                        s = e;
                    }
                    if (cx + r <= tx) {
                        s = lower_bound(v, s, be, key_of(v, z, y, cx + r), st);
                        const uint32_t e = lower_bound(v, s, be, key_of(v, z, y, cx + r) + 1ull, st);
                        st.scanned(e - s);
                        vis.run(s, e);
                    }
                }
            }
        }
        // Every point not yet visited lies beyond a face of the block [c - r, c + r] that is not on the box's boundary, and the query is on
        // the near side of each such face (or in its plane's slop): its distance is at least the least of the face distances below.
        double bound = INFINITY;
        if (cx - r > 0) { const double f = (ox + (double)(cx - r)) * v.cell; bound = fmin(bound, qx - f - slop_of(f, qx, v.cell)); }
        if (cx + r < tx) { const double f = (ox + (double)(cx + r + 1)) * v.cell; bound = fmin(bound, f - qx - slop_of(f, qx, v.cell)); }
        if (cy - r > 0) { const double f = (oy + (double)(cy - r)) * v.cell; bound = fmin(bound, qy - f - slop_of(f, qy, v.cell)); }
        if (cy + r < ty) { const double f = (oy + (double)(cy + r + 1)) * v.cell; bound = fmin(bound, f - qy - slop_of(f, qy, v.cell)); }
        if (cz - r > 0) { const double f = (oz + (double)(cz - r)) * v.cell; bound = fmin(bound, qz - f - slop_of(f, qz, v.cell)); }
        if (cz + r < tz) { const double f = (oz + (double)(cz + r + 1)) * v.cell; bound = fmin(bound, f - qz - slop_of(f, qz, v.cell)); }
        if (bound == INFINITY) return;      // the block covers the whole box
        // strictly nearer than anything unvisited: a tie with an unvisited point of lower index cannot occur
        if (bound > 0.0 && vis.kth() < bound * bound * (1.0 - 0x1p-40)) return;
    }
    double r2 = vis.kth();
    if (v.n >= K) {
        const uint32_t at = lower_bound(v, 0u, v.n, key_of(v, cz, cy, cx), st);
        uint32_t s = at > K / 2 ? at - K / 2 : 0u;
        if (s + K > v.n) s = v.n - K;
        r2 = fmin(r2, vis.max_d2(s, s + K));
    }
    vis.cap(r2);
    const double R = sqrt(r2);      // (+inf: the whole box)
    Box b;
    if (!axis_range(v, 0, qx, R, &b.x0, &b.x1) || !axis_range(v, 1, qy, R, &b.y0, &b.y1) || !axis_range(v, 2, qz, R, &b.z0, &b.z1)) return;
    Box ex;
    ex.x0 = cx - 2 > 0 ? cx - 2 : 0; ex.x1 = cx + 2 < tx ? cx + 2 : tx;
    ex.y0 = cy - 2 > 0 ? cy - 2 : 0; ex.y1 = cy + 2 < ty ? cy + 2 : ty;
    ex.z0 = cz - 2 > 0 ? cz - 2 : 0; ex.z1 = cz + 2 < tz ? cz + 2 : tz;
    box_scan(v, b, &ex, qy, qz, vis, st);
}

// The fitness scores' visitor (sparse_fitness.hip; host/sparse_index_check.cpp runs it on the CPU): knn_walk with K = 1 in the SCORE's metric.
// The score wants the least FLOAT squared distance d = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), dx = fl(q - p) (ring_search.h: ring_scan_run;
// FLANN's L2_Simple<float>, no FMA), and only when it is within the gate; which point has it does not matter, so ties need no order and a point
// offered twice changes nothing.  The walk's bounds are exact (f64) distances, so the visitor widens every comparison by how far d can fall below the
// exact squared distance D of the same two float points:
//   dx = (q - p)(1 + e), |e| <= u = 2^-24 (a float difference is never subnormal-rounded); the square and the two sums round once each, and all terms
//   are >= 0, so every one of them only scales by (1 - u) at worst: d >= D (1 - u)^5 - 3 x 2^-150 > D (1 - 5 x 2^-24) - 2^-148 (the last term: products
//   that underflow).  kWiden = 2^-20 > 5 x 2^-24 with eleven parts in sixteen to spare; the underflow term never decides, because every bound the walk
//   hands over (slab_gap, the face distances of knn_walk, the box of axis_range) already lies slop_of >= cell x 2^-20 inside the true one.
// Hence: a row, a face or a box whose exact bound g2 has g2 (1 - kWiden) > lim holds no point with d <= lim, where lim = min(least d so far, the gate).
// skip() says exactly that; kth() hands the walk lim (1 + kWiden), so that its own tests "kth() < bound^2" and "the box of radius sqrt(kth())" leave
// out only points with D > lim (1 + kWiden), i.e. d > lim.  The gate is a bound from the start: a point farther than it from everything costs the rings'
// look-ups and nothing more.  The visitor alone computes d.
static constexpr double kWiden = 0x1p-20;
struct NearestF32 {
    const Point* pts;
    float qx, qy, qz;
    float best;      // the least d so far; kNone: no point yet (fitness_kernel's 3.0e38f)
    double lim;
    static constexpr float kNone = 3.0e38f;
    SW_FN void start(const Point* p, float x, float y, float z, float gate) { pts = p; qx = x; qy = y; qz = z; best = kNone; lim = (double)gate; }
    SW_FN bool skip(double g2) const { return g2 * (1.0 - kWiden) > lim; }
    SW_FN double kth() const { return lim * (1.0 + kWiden); }
    SW_FN void cap(double) {}      // (kth() has said it already)
    SW_FN void run(uint32_t s, uint32_t e) {
        for (uint32_t j = s; j < e; ++j) {
            const Point p = pts[j];
            const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
            float d = dx * dx;
            d += dy * dy;
            d += dz * dz;
            if (d < best) { best = d; lim = fmin(lim, (double)d); }
        }
    }
    // the seed: its points may as well be taken (a second offer changes nothing), and the bound is the list's own again
    SW_FN double max_d2(uint32_t s, uint32_t e) { run(s, e); return kth(); }
};

}  // namespace sw
}  // namespace pcr
