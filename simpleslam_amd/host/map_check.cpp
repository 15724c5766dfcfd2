// map_check.cpp -- the key-frame store's life beyond the front end through the C++ mirror (PCR::SubMap), on the GPU:
//   key frames added -> updateMap on the store -> setPoses (Backend::optimHandler) -> a view's loopFindNearKeyframes
//   (LoopClosureManager's lc_map_) -> read-back of key frames and of both sub-maps.
// Every point sits alone in its voxel of a 0.5 m lattice, at coordinates and under poses that are exact in float, so the
// program knows every sub-map it must get: the transformed points in ascending voxel index (z, then y, then x).
// Exit code 0 and "map_check ok"; 1 with a message on the first mismatch.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "PCR/HipRegister.hpp"

namespace {

struct P4 { float x, y, z, i; };
bool by_voxel(const P4& a, const P4& b) { return std::tie(a.z, a.y, a.x) < std::tie(b.z, b.y, b.x); }

[[noreturn]] void die(const std::string& what) {
    std::fprintf(stderr, "map_check: %s\n", what.c_str());
    std::exit(1);
}

// a sub-map (or any cloud in HBM) on the host: taken in as the one key frame of a scratch store and read back
std::vector<PCR::PointXYZI> fetch(const PCR::SubMap& sm) {
    size_t n = 0, stride = 0;
    const void* d = sm.devicePointer(&n, &stride);
    if (n == 0) return {};
    if (!d || stride != sizeof(PCR::PointXYZI)) die("a sub-map of " + std::to_string(n) + " points has no pointer or another stride");
    PCR::SubMap tmp;
    tmp.addKeyFrame(d, n, PCR::pose_t());
    return tmp.keyFrame(0)->points;
}

void expect_cloud(const char* name, const std::vector<PCR::PointXYZI>& got, std::vector<P4> want) {
    std::sort(want.begin(), want.end(), by_voxel);
    if (got.size() != want.size()) die(std::string(name) + ": " + std::to_string(got.size()) + " points, expected " + std::to_string(want.size()));
    for (size_t k = 0; k < got.size(); ++k)
        if (got[k].x != want[k].x || got[k].y != want[k].y || got[k].z != want[k].z || got[k].intensity != want[k].i) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: point %zu is (%.9g %.9g %.9g | %.9g), expected (%.9g %.9g %.9g | %.9g)", name, k, got[k].x, got[k].y, got[k].z,
                          got[k].intensity, want[k].x, want[k].y, want[k].z, want[k].i);
            die(buf);
        }
}

void expect_idx(const char* name, const std::vector<int64_t>& got, const std::vector<int64_t>& want) {
    if (got != want) die(std::string(name) + ": other key frames selected than expected");
}

}  // namespace

int main() {
    try {
        const int kKf = 5, kPts = 6;
        const double grid = 0.5;
        PCR::SubMap map;
        std::vector<PCR::PC_Ptr> clouds;
        for (int j = 0; j < kKf; ++j) {      // key frame j: a row of points along x, in its own frame; the vehicle moves along y, 2 m a key frame
            auto pc = std::make_shared<PCR::PointCloud>();
            for (int i = 0; i < kPts; ++i) { PCR::PointXYZI p; p.x = i + 0.25f; p.y = 0.25f; p.z = 0.25f; p.intensity = 10.f * j + i; pc->points.push_back(p); }
            PCR::pose_t T;
            T(1, 3) = 2.0 * j;
            map.addKeyFrame(pc, T);
            clouds.push_back(pc);
        }
        auto row = [&](int j, double ty) { std::vector<P4> r; for (int i = 0; i < kPts; ++i) r.push_back({i + 0.25f, (float)ty + 0.25f, 0.25f, 10.f * j + i}); return r; };
        auto cat = [](std::vector<P4> a, const std::vector<P4>& b) { a.insert(a.end(), b.begin(), b.end()); return a; };

        // the odometry sub-map: key frames within 3 m of (0, 4, 0)
        const double at[3] = {0, 4, 0};
        if (map.updateMap(at, 3.0, grid) != 3u * kPts) die("updateMap: wrong number of points");
        expect_idx("updateMap", map.submapIdx(), {1, 2, 3});
        const std::vector<PCR::PointXYZI> odom = fetch(map);
        expect_cloud("updateMap", odom, cat(cat(row(1, 2), row(2, 4)), row(3, 6)));
        const uint64_t gen = map.generation();

        // the optimiser moves key frame 1 away and turns key frame 2 by a quarter about z: nothing assembled changes
        std::vector<PCR::pose_t> opt(2);
        opt[0](1, 3) = 20.0;
        opt[1](0, 0) = 0; opt[1](0, 1) = -1; opt[1](1, 0) = 1; opt[1](1, 1) = 0; opt[1](1, 3) = 4.0;
        map.setPoses(1, opt);
        if (map.generation() != gen) die("setPoses started a new generation");
        expect_idx("after setPoses", map.submapIdx(), {1, 2, 3});
        expect_cloud("after setPoses", fetch(map), cat(cat(row(1, 2), row(2, 4)), row(3, 6)));

        // the loop-closure sub-map on a view: key frames 2 +- 1 under the NEW poses, beside the odometry sub-map
        auto lc = map.view();
        if (lc->loopFindNearKeyframes(2, 1, grid) != 3u * kPts) die("view window: wrong number of points");
        expect_idx("view window", lc->submapIdx(), {1, 2, 3});
        std::vector<P4> turned;
        for (int i = 0; i < kPts; ++i) turned.push_back({-0.25f, i + 0.25f + 4.f, 0.25f, 20.f + i});
        expect_cloud("view window", fetch(*lc), cat(cat(row(1, 20), turned), row(3, 6)));
        if (map.generation() != gen) die("the view's window started a new generation on the parent");
        const std::vector<PCR::PointXYZI> odom_after = fetch(map);
        if (odom_after.size() != odom.size() || std::memcmp(odom_after.data(), odom.data(), odom.size() * sizeof(PCR::PointXYZI)))
            die("the view's window changed the parent's sub-map");
        // ... and the parent's next update sees the new poses as well: key frame 1 is out of reach now
        if (map.updateMap(at, 3.0, grid) != 2u * kPts) die("updateMap after setPoses: wrong number of points");
        expect_idx("updateMap after setPoses", map.submapIdx(), {2, 3});

        // read-back: the stored bytes and the pose in force, from the store and through the view
        for (int j = 0; j < kKf; ++j) {
            PCR::pose_t T;
            const PCR::PC_Ptr back = (j % 2 ? lc->keyFrame(j, &T) : map.keyFrame(j, &T));
            if (back->size() != clouds[j]->size() || std::memcmp(back->points.data(), clouds[j]->points.data(), back->size() * sizeof(PCR::PointXYZI)))
                die("key frame " + std::to_string(j) + " does not read back as stored");
            PCR::pose_t want;
            if (j == 1) want = opt[0]; else if (j == 2) want = opt[1]; else want(1, 3) = 2.0 * j;
            if (std::memcmp(T.data(), want.data(), sizeof want.m)) die("pose of key frame " + std::to_string(j) + " is not the one in force");
        }
        // a view cannot change the store, and says why
        bool refused = false;
        try { lc->setPoses(0, opt); } catch (const std::exception& e) { refused = std::string(e.what()).find("view") != std::string::npos; }
        if (!refused) die("setPoses on a view was not refused as such");
        std::printf("map_check ok\n");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "map_check: error: %s\n", e.what());
        return 1;
    }
}
