// session_check.cpp -- a session to and from disk through the C++ mirror (PCR::SubMap::save / load, backend::Backend::setSaveDir / save / load,
// pcp::savePCDFile), checked against values this program computes itself.
//   session_check pcd <in.f32> <out.pcd>   raw float records x y z intensity -> pcp::savePCDFile (binary).  No GPU call: the CPU suite compares
//                                          the file with what pcr_pcd_write writes for the same cloud.
//   session_check map <dir>                on the GPU: a store of four small key frames (0, 1, 70 and 300 points) -> save (precise) -> load into a
//                                          new store: the same bytes, the poses of pcr_tum_parse over the written lines, the stamps; then a back end
//                                          with a save directory takes the key frames, saves, and a new back end over a new store loads the session:
//                                          key-frame, context and graph totals, the raw clouds on disk, the filtered ones in both stores.
//                                          Prints "session_check ok"; exit status 1 with the first difference otherwise.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "PCR/HipRegister.hpp"
#include "pcp/pcd_io.hpp"

#define REQUIRE(cond, what) do { if (!(cond)) { std::fprintf(stderr, "session_check: %s (%s:%d)\n", what, __FILE__, __LINE__); return 1; } } while (0)

static PCR::PC_Ptr cloud_of(size_t n, unsigned seed) {
    auto pc = std::make_shared<PCR::PointCloud>();
    unsigned s = seed * 2654435761u + 12345u;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / (float)(1u << 24); };
    for (size_t i = 0; i < n; ++i) {
        PCR::PointXYZI p;
        p.x = 20.f * next() - 10.f; p.y = 20.f * next() - 10.f; p.z = 3.f * next(); p.intensity = 255.f * next();
        pc->points.push_back(p);
    }
    return pc;
}

static PCR::pose_t pose_of(double yaw, double x, double y, double z) {
    PCR::pose_t T;
    T(0, 0) = std::cos(yaw); T(0, 1) = -std::sin(yaw); T(1, 0) = std::sin(yaw); T(1, 1) = std::cos(yaw);
    T(0, 3) = x; T(1, 3) = y; T(2, 3) = z;
    return T;
}

static bool same_cloud(const PCR::PointCloud& a, const PCR::PointCloud& b) {
    return a.size() == b.size() && (a.size() == 0 || std::memcmp(a.points.data(), b.points.data(), a.size() * sizeof(PCR::PointXYZI)) == 0);
}

static int pcd_mode(const char* in, const char* out) {
    std::ifstream f(in, std::ios::binary);
    REQUIRE((bool)f, "cannot open the input");
    PCR::PointCloud pc;
    float r[4];
    while (f.read(reinterpret_cast<char*>(r), sizeof r)) {
        PCR::PointXYZI p;
        p.x = r[0]; p.y = r[1]; p.z = r[2]; p.intensity = r[3];
        pc.points.push_back(p);
    }
    REQUIRE(pcp::savePCDFile(out, pc) == 0, "savePCDFile failed");
    return 0;
}

static int map_mode(const std::string& dir) {
    const size_t sizes[4] = {0, 1, 70, 300};
    std::vector<PCR::PC_Ptr> clouds;
    std::vector<PCR::pose_t> poses;
    const std::vector<double> stamps = {0.0, 0.5, 1.25, 1000.125};
    for (size_t k = 0; k < 4; ++k) {
        clouds.push_back(cloud_of(sizes[k], (unsigned)k + 1));
        poses.push_back(pose_of(0.3 * (double)k - 0.2, 1.5 * (double)k, -0.25 * (double)k, 0.125));
    }
    {   // the store alone
        PCR::SubMap a;
        for (size_t k = 0; k < 4; ++k) a.addKeyFrame(clouds[k], poses[k]);
        a.save(dir, 0, stamps, true);
        PCR::SubMap b;
        const std::vector<double> got = b.load(dir);
        REQUIRE(got == stamps, "the loaded stamps differ");
        REQUIRE(b.keyframes() == 4, "the loaded store does not hold 4 key frames");
        std::ifstream tum(dir + "/tum.txt");
        for (size_t k = 0; k < 4; ++k) {
            PCR::pose_t p, want;
            REQUIRE(same_cloud(*b.keyFrame(k, &p), *clouds[k]), "a loaded key frame differs from the one saved");
            std::string line;
            REQUIRE((bool)std::getline(tum, line), "tum.txt is short");
            double stamp = 0;
            REQUIRE(pcr_tum_parse(line.c_str(), &stamp, want.data()) == PCR_TUM_OK && stamp == stamps[k], "a line of tum.txt does not parse");
            REQUIRE(std::memcmp(p.m, want.m, sizeof p.m) == 0, "a loaded pose is not pcr_tum_parse of its line");
            for (int i = 0; i < 3; ++i) REQUIRE(p(i, 3) == poses[k](i, 3), "precise: a translation did not come back bit for bit");
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) REQUIRE(std::fabs(p(i, j) - poses[k](i, j)) < 1e-14, "precise: a rotation moved");
        }
        bool refused = false;
        try { b.load(dir); } catch (const std::exception&) { refused = true; }
        REQUIRE(refused && b.keyframes() == 4, "a load into a store with key frames was not refused");
        b.addKeyFrame(clouds[3], poses[3]);      // (the loaded store has the layout of the clouds added afterwards)
    }
    {   // the back end: raw clouds to disk from inside the event, then the session into new handles
        pcr_backend_params prm = backend::Backend::defaults();
        prm.detectors = 0;
        PCR::SubMap a;
        backend::Backend be(a, &prm);
        be.setSaveDir(dir);
        for (size_t k = 0; k < 4; ++k) a.addKeyFrame(clouds[k], poses[k]);
        be.addKeyFrames();
        be.save(stamps, false);
        PCR::PointCloud raw;
        REQUIRE(pcp::loadPCDFile(dir + "/3.pcd", raw) == 0 && same_cloud(raw, *clouds[3]), "3.pcd is not the raw key frame");
        REQUIRE(a.keyFrame(3)->size() < 300, "the in-place filter did not run");
        PCR::SubMap b;
        backend::Backend be2(b, &prm);
        backend::Backend::Info info;
        const std::vector<double> got = be2.load(dir, &info);
        REQUIRE(got == stamps, "the back end's loaded stamps differ");
        REQUIRE(info.keyframes == 4 && info.contexts == 4 && b.keyframes() == 4, "the loaded totals differ");
        size_t n_poses = 0, n_priors = 0, n_between = 0, want_between = 0;
        pcr_graph_size(be2.graph(), &n_poses, &n_priors, &n_between);
        pcr_graph_size(be.graph(), nullptr, nullptr, &want_between);
        REQUIRE(n_poses == 4 && n_priors == 1 && n_between == want_between && n_between == 3, "the loaded graph differs in size");
        for (size_t k = 0; k < 4; ++k) REQUIRE(same_cloud(*a.keyFrame(k), *b.keyFrame(k)), "a loaded, filtered key frame differs from the first session's");
        b.addKeyFrame(clouds[2], poses[3]);
        const backend::Backend::Info add = be2.addKeyFrames();
        REQUIRE(add.keyframes_added == 1 && add.keyframes == 5 && add.contexts == 5, "the event after the load did not take exactly the new key frame");
    }
    std::printf("session_check ok\n");
    return 0;
}

int main(int argc, char** argv) {
    try {
        if (argc == 4 && std::string(argv[1]) == "pcd") return pcd_mode(argv[2], argv[3]);
        if (argc == 3 && std::string(argv[1]) == "map") return map_mode(argv[2]);
        std::fprintf(stderr, "usage: %s pcd <in.f32> <out.pcd> | map <dir>\n", argv[0]);
        return 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
