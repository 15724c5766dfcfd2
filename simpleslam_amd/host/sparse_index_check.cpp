// sparse_index_check.cpp -- the walk of the sparse target index (csrc/sparse_walk.h) on the CPU, with no GPU call, no HIP header and no library:
//   sparse_index_check <points.f32> <queries.f32> <k> <radius> <out.bin>
// points / queries: records of four floats (x, y, z, one more).  The index is built here with a plain stable sort -- the layout of
// sparse_walk.h, the cell floor(x / cell) in f64, rows that are not finite dropped -- and every query is answered by the shared walk under
// host visitors that order by (d2, original row) exactly as the device's do.  out.bin: the k-NN rows (int64 idx[nq][k], double d2[nq][k]),
// then the radius search (uint64 offsets[nq + 1], int64 idx[total], double d2[total], every segment ascending by (d2, idx)).
// stdout, one line per query: the look-ups and points scanned of its k-NN walk, whether it came to the box scan and, if so, the occupied
// rows R and layers L of the block scanned (counted here from the sorted keys, not by the walk) -- the walk's bound is
// kRingLookups + 2 + kRowLookups R + kLayerLookups L -- and the same for its radius walk (bound: 1 + kRowLookups R + kLayerLookups L).
// A cloud the index refuses: "refused <reason> <extents>" and exit status 3.
//   sparse_index_check fitness <points.f32> <queries.f32> <gate>
// The fitness scores' search (csrc/sparse_fitness.hip) on the CPU: the same walk with K = 1 under the same visitor, sw::NearestF32 -- the least
// FLOAT squared distance within the gate (a float; 3.4028235e38 for none) -- against a brute force over every stored point in the same float
// arithmetic.  stdout, one line per query: the bits of the walk's answer and of the brute force's (a distance beyond the gate is nobody's
// answer: both print the bits of 3.0e38f), the walk's look-ups and points, whether it came to the box scan and that block's occupied rows and
// layers; then "mismatches <count>".  The walk's bound is the k-NN walk's: kRingLookups + 1 + box (1 + kRowLookups R + kLayerLookups L).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <numeric>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../csrc/sparse_walk.h"

using namespace pcr;

static std::vector<float> load(const char* path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    const size_t bytes = (size_t)f.tellg();
    std::vector<float> v(bytes / 4);
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * 4));
    return v;
}

static double dist2(const sw::Point& p, double qx, double qy, double qz) {
    const double dx = qx - (double)p.x, dy = qy - (double)p.y, dz = qz - (double)p.z;
    double d = dx * dx;
    d += dy * dy;
    d += dz * dz;
    return d;
}

// the k-NN list: (d2, row) pairs ascending, at most K
struct KnnVisitor {
    const sw::Point* pts;
    double qx, qy, qz, capv = INFINITY;
    size_t K;
    std::vector<std::pair<double, uint32_t>> L;
    std::set<uint32_t> seen;      // a point offered twice is a bug of the walk
    bool twice = false;
    double kth() const { return L.size() < K ? INFINITY : L.back().first; }
    bool skip(double g2) const { return g2 > std::fmin(kth(), capv); }
    void cap(double r2) { capv = r2; }
    void run(uint32_t s, uint32_t e) {
        for (uint32_t j = s; j < e; ++j) {
            if (!seen.insert(j).second) twice = true;
            const std::pair<double, uint32_t> c(dist2(pts[j], qx, qy, qz), pts[j].row);
            if (L.size() == K && !(c < L.back())) continue;
            L.insert(std::upper_bound(L.begin(), L.end(), c), c);
            if (L.size() > K) L.pop_back();
        }
    }
    double max_d2(uint32_t s, uint32_t e) const {
        double m = 0.0;
        for (uint32_t j = s; j < e; ++j) m = std::fmax(m, dist2(pts[j], qx, qy, qz));
        return m;
    }
};

struct RadiusVisitor {
    const sw::Point* pts;
    double qx, qy, qz, r2;
    std::vector<std::pair<double, uint32_t>> out;
    std::set<uint32_t> seen;
    bool twice = false;
    bool skip(double g2) const { return g2 >= r2 * (1.0 + 0x1p-40); }
    void run(uint32_t s, uint32_t e) {
        for (uint32_t j = s; j < e; ++j) {
            if (!seen.insert(j).second) twice = true;
            const double d = dist2(pts[j], qx, qy, qz);
            if (d < r2) out.emplace_back(d, pts[j].row);
        }
    }
};

// occupied rows of the (z, y) range of a block and occupied layers of its z range, from the sorted keys
static void rows_layers(const sw::View& v, const sw::Box& b, unsigned long long* rows, unsigned long long* layers) {
    std::set<unsigned long long> r, l;
    for (uint32_t j = 0; j < v.n; ++j) {
        const unsigned long long zy = v.keys[j] >> v.b0, z = zy >> v.b1, y = zy & ((1ull << v.b1) - 1ull);
        if ((long long)z < b.z0 || (long long)z > b.z1) continue;
        l.insert(z);
        if ((long long)y >= b.y0 && (long long)y <= b.y1) r.insert(zy);
    }
    *rows = r.size(); *layers = l.size();
}

// the build: box of the lattice values over the finite rows, layout, keys, a stable sort
struct Index {
    sw::View v;
    sw::Layout lay;
    std::vector<unsigned long long> keys;
    std::vector<sw::Point> pts;
};
static bool build_index(const std::vector<float>& P, double cell, Index& ix) {
    const size_t n = P.size() / 4;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    std::vector<uint32_t> kept;
    for (size_t i = 0; i < n; ++i) {
        const float* p = &P[i * 4];
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;
        kept.push_back((uint32_t)i);
        for (int a = 0; a < 3; ++a) { const double f = std::floor((double)p[a] / cell); lo[a] = std::fmin(lo[a], f); hi[a] = std::fmax(hi[a], f); }
    }
    if (kept.empty()) for (int a = 0; a < 3; ++a) lo[a] = hi[a] = 0.0;
    const sw::Layout lay = sw::layout_of(lo, hi);
    ix.lay = lay;
    if (lay.refused) {
        std::printf("refused %s %.6g x %.6g x %.6g\n", lay.refused == sw::kRefusedBits ? "bits" : "range", lay.extd[0], lay.extd[1], lay.extd[2]);
        return false;
    }
    sw::View& v = ix.v;
    v.n = (uint32_t)kept.size(); v.b0 = lay.b[0]; v.b1 = lay.b[1]; v.b2 = lay.b[2]; v.cell = cell;
    for (int a = 0; a < 3; ++a) { v.lo[a] = lay.lo[a]; v.ext[a] = lay.ext[a]; }
    std::vector<unsigned long long> key_of_row(kept.size());
    for (size_t j = 0; j < kept.size(); ++j) {
        const float* p = &P[(size_t)kept[j] * 4];
        long long c[3];
        for (int a = 0; a < 3; ++a) c[a] = (long long)std::floor((double)p[a] / cell) - lay.lo[a];
        key_of_row[j] = sw::key_of(v, c[2], c[1], c[0]);
    }
    std::vector<uint32_t> order(kept.size());
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key_of_row[a] < key_of_row[b]; });
    ix.keys.assign(kept.size() + 1, 0ull);      // (+ 1: never an empty array behind the pointers)
    ix.pts.assign(kept.size() + 1, sw::Point{0.f, 0.f, 0.f, 0u});
    for (size_t j = 0; j < kept.size(); ++j) {
        const uint32_t row = kept[order[j]];
        ix.keys[j] = key_of_row[order[j]];
        ix.pts[j] = sw::Point{P[(size_t)row * 4], P[(size_t)row * 4 + 1], P[(size_t)row * 4 + 2], row};
    }
    v.keys = ix.keys.data(); v.pts = ix.pts.data();
    std::printf("index %u points, bits %d %d %d, extents %llu %llu %llu\n", v.n, v.b0, v.b1, v.b2, v.ext[0], v.ext[1], v.ext[2]);
    return true;
}

static uint32_t bits_of_float(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// the `fitness` mode
static int fitness_mode(const char* points, const char* queries, const char* gate_text) {
    const std::vector<float> P = load(points), Q = load(queries);
    const float gate = std::strtof(gate_text, nullptr);
    Index ix;
    if (!build_index(P, 1.0, ix)) return 3;
    const sw::View& v = ix.v;
    unsigned long long mismatches = 0;
    for (size_t i = 0; i < Q.size() / 4; ++i) {
        const float* q = &Q[i * 4];
        sw::Stats st;
        unsigned long long rows = 0, layers = 0;
        float got = sw::NearestF32::kNone, want = sw::NearestF32::kNone;
        if (std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2])) {
            sw::NearestF32 vis;
            vis.start(v.pts, q[0], q[1], q[2], gate);
            sw::knn_walk(v, (double)q[0], (double)q[1], (double)q[2], 1u, vis, st);
            if (vis.best <= gate) got = vis.best;
            if (st.boxes) rows_layers(v, st.box, &rows, &layers);
            sw::NearestF32 all;      // brute force: the visitor's own arithmetic over every stored point, no walk and no bound
            all.start(v.pts, q[0], q[1], q[2], gate);
            all.run(0u, v.n);
            if (all.best <= gate) want = all.best;
        }
        mismatches += bits_of_float(got) != bits_of_float(want);
        std::printf("q %zu got %u want %u lookups %llu points %llu box %d rows %llu layers %llu\n", i, bits_of_float(got), bits_of_float(want), st.lookups,
                    st.points, st.boxes, rows, layers);
    }
    std::printf("bounds ring %d row %d layer %d\n", sw::kRingLookups, sw::kRowLookups, sw::kLayerLookups);
    std::printf("mismatches %llu\n", mismatches);
    return mismatches ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && std::string(argv[1]) == "fitness") {
        try { return fitness_mode(argv[2], argv[3], argv[4]); }
        catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 1; }
    }
    if (argc != 6) { std::fprintf(stderr, "usage: %s <points.f32> <queries.f32> <k> <radius> <out.bin>\n", argv[0]); return 2; }
    try {
        const std::vector<float> P = load(argv[1]), Q = load(argv[2]);
        const size_t nq = Q.size() / 4;
        const size_t K = (size_t)std::atoi(argv[3]);
        const double radius = std::atof(argv[4]), cell = 1.0;
        if (K < 1 || K > 32 || !(radius > 0.0)) throw std::runtime_error("k must be 1 .. 32 and the radius positive");
        Index ix;
        if (!build_index(P, cell, ix)) return 3;
        const sw::View& v = ix.v;
        const std::vector<sw::Point>& pts = ix.pts;

        std::vector<int64_t> kidx(nq * K, -1);
        std::vector<double> kd2(nq * K, INFINITY);
        std::vector<uint64_t> offsets(nq + 1, 0);
        std::vector<int64_t> ridx;
        std::vector<double> rd2;
        bool twice = false;
        for (size_t i = 0; i < nq; ++i) {
            const float* q = &Q[i * 4];
            const bool finite = std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2]);
            sw::Stats ks, rs;
            unsigned long long krows = 0, klayers = 0, rrows = 0, rlayers = 0;
            if (finite) {
                KnnVisitor kv;
                kv.pts = pts.data(); kv.qx = q[0]; kv.qy = q[1]; kv.qz = q[2]; kv.K = K;
                sw::knn_walk(v, kv.qx, kv.qy, kv.qz, (uint32_t)K, kv, ks);
                for (size_t j = 0; j < kv.L.size(); ++j) { kidx[i * K + j] = kv.L[j].second; kd2[i * K + j] = kv.L[j].first; }
                if (ks.boxes) rows_layers(v, ks.box, &krows, &klayers);
                RadiusVisitor rv;
                rv.pts = pts.data(); rv.qx = q[0]; rv.qy = q[1]; rv.qz = q[2]; rv.r2 = radius * radius;
                sw::radius_walk(v, rv.qx, rv.qy, rv.qz, radius, rv, rs);
                if (rs.boxes) rows_layers(v, rs.box, &rrows, &rlayers);
                std::sort(rv.out.begin(), rv.out.end());
                for (const auto& e : rv.out) { ridx.push_back(e.second); rd2.push_back(e.first); }
                twice = twice || kv.twice || rv.twice;
            }
            offsets[i + 1] = ridx.size();
            std::printf("q %zu knn_lookups %llu knn_points %llu knn_box %d knn_rows %llu knn_layers %llu rad_lookups %llu rad_points %llu rad_box %d rad_rows %llu rad_layers %llu\n",
                        i, ks.lookups, ks.points, ks.boxes, krows, klayers, rs.lookups, rs.points, rs.boxes, rrows, rlayers);
        }
        std::printf("bounds ring %d row %d layer %d\n", sw::kRingLookups, sw::kRowLookups, sw::kLayerLookups);
        if (twice) { std::printf("a stored point was visited twice\n"); return 1; }
        std::ofstream out(argv[5], std::ios::binary);
        if (!out) throw std::runtime_error(std::string("cannot write ") + argv[5]);
        out.write(reinterpret_cast<const char*>(kidx.data()), (std::streamsize)(kidx.size() * 8));
        out.write(reinterpret_cast<const char*>(kd2.data()), (std::streamsize)(kd2.size() * 8));
        out.write(reinterpret_cast<const char*>(offsets.data()), (std::streamsize)(offsets.size() * 8));
        out.write(reinterpret_cast<const char*>(ridx.data()), (std::streamsize)(ridx.size() * 8));
        out.write(reinterpret_cast<const char*>(rd2.data()), (std::streamsize)(rd2.size() * 8));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
