// seq_harness.cpp -- the front end's per-scan loop driven from C++: LidarOdometry::handler around scan2Map (frontend/src/LidarOdometry.cpp:160-214,
// frontend/src/MapManager.cpp:109-201) over a recording, through PCR::Frontend (pcr_frontend_*: the loop itself lives in the library).
//   seq_harness <method> <list.txt> <cmds.txt> <start.txt> [--grid g] [--mobile] [--prefetch] [--reps r] [--backend] [--save DIR] [--load DIR]
// method     loam | ndt | vgicp | gicp | liorf (the factory of LidarOdometry.cpp:44-54: unknown throws)
// list.txt   one scan file per line: .pcd (pcp/pcd_io.hpp) or raw float records x y z intensity (.f32, as the other harnesses read them)
// cmds.txt   one 4x4 per line, 16 numbers row by row: cmds[k] = the motion from scan k-1 to scan k as the odometer reports it (cmds[0]: identity)
// start.txt  the pose before scan 0, 16 numbers row by row
// --grid g   downSampleVoxelGridSize (default 0.5);  --mobile  SixDof2Mobile on every refined pose (LidarOdometry.cpp:211)
// --prefetch the next scan's voxel filter is queued before this scan is registered;  --reps r  the drive r times on the same handles
// --backend  backend::Backend (pcr_backend_*) behind the front end, as sequence.drive_slam has it: after every scan that added a key frame,
//            pcr_backend_step with Frontend::closest()'s new entries, and the next guess starts from lc.delta * (add.delta * pose) (the same
//            fixed-order product).  Prints one "backend k ..." line per event of the first drive: key frames, candidates, accepted, LM iterations
// --save DIR the session goes to DIR (which must exist) as the reference's saveMapDir: every new key frame raw as {i}.pcd from inside the add event,
//            tum.txt and fg.g2o at the end of the drive; prints "saved keyframes n".  --load DIR starts from such a session: backend::Backend::load
//            before the first scan, the sub-map about the start pose, then the drive goes on behind the loaded key frames; prints "loaded keyframes
//            n".  Both imply --backend and take one drive (--reps 1).
// The scans are uploaded before the timed loop (into a key-frame store of their own: no HIP call in this file).  generateOdom's guess is chained
// here, init = pose * cmds[k], by one fixed-order product -- rows times columns, every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3, no contraction --
// so that any caller can repeat it to the bit.
// Prints one line per scan of the FIRST drive: "scan k" + the pose as 16 C hex floats (%a), row by row, + converged iterations keyframe_added
// update_queued n_submap; then one summary line (scans/s and the host time of the five steps) for the first drive and, with --reps > 1, for the
// last one, which follows pcr_frontend_reset on the same handles.  Every later drive must give the first one's poses bit for bit: exit status 4 if not.
#include <chrono>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "PCR/HipRegister.hpp"
#include "pcp/pcd_io.hpp"

static const char* kUsage = "usage: %s <loam|ndt|vgicp|gicp|liorf> <list.txt> <cmds.txt> <start.txt> [--grid g] [--mobile] [--prefetch] [--reps r] [--backend] [--save DIR] [--load DIR]\n";

static bool ends_with(const std::string& s, const char* suffix) {
    const size_t n = std::char_traits<char>::length(suffix);
    return s.size() >= n && s.compare(s.size() - n, n, suffix) == 0;
}

static PCR::PC_Ptr load_scan(const std::string& path) {
    auto pc = std::make_shared<PCR::PointCloud>();
    if (ends_with(path, ".pcd")) {
        if (pcp::loadPCDFile(path, *pc) == -1) throw std::runtime_error("can't load scan from: " + path);
        return pc;
    }
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    float r[4];
    while (f.read(reinterpret_cast<char*>(r), sizeof r)) {
        PCR::PointXYZI p;
        p.x = r[0]; p.y = r[1]; p.z = r[2]; p.intensity = r[3];
        pc->points.push_back(p);
    }
    return pc;
}

// 4x4 matrices, 16 numbers per line, row by row (decimal or C hex floats: strtod reads both exactly)
static std::vector<PCR::pose_t> read_poses(const char* path) {
    std::ifstream f(path);
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    std::vector<PCR::pose_t> out;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ls(line);
        std::string tok;
        std::vector<double> v;
        while (ls >> tok) {
            char* end = nullptr;
            const double x = std::strtod(tok.c_str(), &end);
            if (end == tok.c_str() || *end) throw std::runtime_error(std::string(path) + ": not a number: " + tok);
            v.push_back(x);
        }
        if (v.empty()) continue;
        if (v.size() != 16) throw std::runtime_error(std::string(path) + ": a line must hold the 16 numbers of a 4x4 matrix");
        PCR::pose_t T;
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T(r, c) = v[(size_t)r * 4 + c];
        out.push_back(T);
    }
    return out;
}

static PCR::pose_t product(const PCR::pose_t& a, const PCR::pose_t& b) {
    PCR::pose_t o;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) o(r, c) = ((a(r, 0) * b(0, c) + a(r, 1) * b(1, c)) + a(r, 2) * b(2, c)) + a(r, 3) * b(3, c);
    return o;
}

struct Drive {
    std::vector<PCR::pose_t> poses;
    std::vector<pcr_frontend_info> infos;
    double seconds = 0, step[5] = {0, 0, 0, 0, 0};
};

static void summary(const char* which, const Drive& d) {
    const pcr_frontend_info& last = d.infos.back();
    std::printf("summary %s scans %zu seconds %.6f scans_per_s %.2f voxel %.6f wait %.6f scan2map %.6f add_keyframe %.6f update_map %.6f keyframes %lld updates %lld\n",
                which, d.poses.size(), d.seconds, (double)d.poses.size() / d.seconds, d.step[0], d.step[1], d.step[2], d.step[3], d.step[4],
                (long long)last.keyframes, (long long)last.updates);
}

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, kUsage, argv[0]); return 2; }
    double grid = 0.5;
    bool mobile = false, prefetch = false, with_backend = false;
    long reps = 1;
    std::string save_dir, load_dir;
    for (int i = 5; i < argc; ++i) {
        const std::string a = argv[i];
        char* end = nullptr;
        if (a == "--mobile") mobile = true;
        else if (a == "--prefetch") prefetch = true;
        else if (a == "--backend") with_backend = true;
        else if (a == "--save" && i + 1 < argc) { save_dir = argv[++i]; with_backend = true; }
        else if (a == "--load" && i + 1 < argc) { load_dir = argv[++i]; with_backend = true; }
        else if (a == "--grid" && i + 1 < argc) { grid = std::strtod(argv[++i], &end); if (end == argv[i] || *end || !(grid > 0)) { std::fprintf(stderr, "error: --grid takes a positive number\n"); return 2; } }
        else if (a == "--reps" && i + 1 < argc) { reps = std::strtol(argv[++i], &end, 10); if (end == argv[i] || *end || reps < 1) { std::fprintf(stderr, "error: --reps takes a count >= 1\n"); return 2; } }
        else { std::fprintf(stderr, "error: unknown or incomplete argument %s\n", a.c_str()); std::fprintf(stderr, kUsage, argv[0]); return 2; }
    }
    if ((!save_dir.empty() || !load_dir.empty()) && reps != 1) { std::fprintf(stderr, "error: --save and --load take one drive (--reps 1)\n"); return 2; }
    try {
        auto reg = std::dynamic_pointer_cast<PCR::HipRegister>(PCR::makeRegister(argv[1]));      // throws on an unknown type, LidarOdometry.cpp:50-54
        pcr_set_profile(reg->handle(), 0);      // no timing events inside the calls: the drive is timed from outside, as bench.py times its own
        std::vector<PCR::PC_Ptr> scans;
        {
            std::ifstream lf(argv[2]);
            if (!lf) throw std::runtime_error(std::string("cannot open ") + argv[2]);
            std::string file;
            while (lf >> file) {
                scans.push_back(load_scan(file));
                if (scans.back()->size() == 0) throw std::runtime_error("no points in " + file);
            }
        }
        if (scans.empty()) throw std::runtime_error(std::string("no scan is listed in ") + argv[2]);
        const std::vector<PCR::pose_t> cmds = read_poses(argv[3]);
        const std::vector<PCR::pose_t> start = read_poses(argv[4]);
        if (cmds.size() < scans.size()) throw std::runtime_error(std::string(argv[3]) + " holds fewer motions than there are scans");
        if (start.size() != 1) throw std::runtime_error(std::string(argv[4]) + " must hold one pose");

        // the recording goes into HBM before anything is timed: a store of its own, whose key frames are the scans as they are
        PCR::SubMap recording;
        for (const auto& s : scans) recording.addKeyFrame(s, PCR::pose_t());
        std::vector<std::pair<const void*, size_t>> d_scans(scans.size());
        for (size_t k = 0; k < scans.size(); ++k) d_scans[k].first = recording.keyFramePointer(k, &d_scans[k].second);

        PCR::SubMap map;
        pcr_frontend_params prm;
        pcr_frontend_default_params(&prm);
        prm.grid_size = grid;
        prm.mobile = mobile ? 1 : 0;
        std::unique_ptr<backend::Backend> be;
        if (with_backend) be.reset(new backend::Backend(map));
        if (!load_dir.empty()) {      // before the front end exists: it takes over the store as it finds it, key frames and sub-map
            const std::vector<double> stamps = be->load(load_dir);
            std::printf("loaded keyframes %zu\n", stamps.size());
            const double at[3] = {start[0](0, 3), start[0](1, 3), start[0](2, 3)};
            if (!stamps.empty()) map.updateMap(at, prm.radius, prm.grid_size);
        }
        if (!save_dir.empty()) be->setSaveDir(save_dir);
        PCR::Frontend fe(*reg, map, &prm);
        std::vector<std::string> events;

        Drive first, last;
        int differing = 0;
        for (long rep = 0; rep < reps; ++rep) {
            Drive d;
            if (rep) { fe.reset(); if (be) be->reset(); }
            size_t taken = 0;
            PCR::pose_t pose = start[0];
            const auto t0 = std::chrono::steady_clock::now();
            for (size_t k = 0; k < scans.size(); ++k) {
                double ahead = 0;
                if (prefetch && k + 1 < scans.size()) {
                    const auto t1 = std::chrono::steady_clock::now();
                    fe.prefetch(d_scans[k + 1].first, d_scans[k + 1].second, true);
                    ahead = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
                }
                pcr_frontend_info info;
                pose = fe.step(d_scans[k].first, d_scans[k].second, true, product(pose, cmds[k]), &info);      // generateOdom: the guess, then scan2Map
                d.poses.push_back(pose);
                d.infos.push_back(info);
                for (int i = 0; i < 5; ++i) d.step[i] += info.seconds[i];
                d.step[0] += ahead;
                if (be && info.keyframe_added) {      // optimHandler's NewKFCome, then lcHandler and the LC event; delta onto the odometry (Backend.cpp:321-346)
                    const std::vector<int64_t> closest = fe.closest();
                    backend::Backend::Info add, lc;
                    be->step(closest.data() + taken, closest.size() - taken, &add, &lc);
                    taken = closest.size();
                    PCR::pose_t da, dl;
                    std::memcpy(da.data(), add.delta, sizeof add.delta);
                    std::memcpy(dl.data(), lc.delta, sizeof lc.delta);
                    pose = product(dl, product(da, pose));
                    if (rep == 0) {
                        char line[160];
                        std::snprintf(line, sizeof line, "backend %zu keyframes %lld candidates %d accepted %d lm_iterations %d %d", k, (long long)add.keyframes,
                                      (int)lc.candidates, (int)lc.accepted, (int)add.graph.iterations, (int)lc.graph.iterations);
                        events.push_back(line);
                    }
                }
            }
            const auto t1 = std::chrono::steady_clock::now();
            fe.finish();
            d.step[1] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
            d.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (rep == 0) first = d;
            else for (size_t k = 0; k < d.poses.size(); ++k) differing += std::memcmp(d.poses[k].m, first.poses[k].m, sizeof first.poses[k].m) != 0;
            last = d;
        }
        for (size_t k = 0; k < first.poses.size(); ++k) {
            std::printf("scan %zu", k);
            for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) std::printf(" %a", first.poses[k](r, c));
            const pcr_frontend_info& i = first.infos[k];
            std::printf(" %d %d %d %d %lld\n", (int)i.converged, (int)i.iterations, (int)i.keyframe_added, (int)i.update_queued, (long long)i.n_submap);
        }
        for (const std::string& e : events) std::printf("%s\n", e.c_str());
        if (!save_dir.empty()) {
            be->save();
            std::printf("saved keyframes %zu\n", map.keyframes());
        }
        summary("first", first);
        if (reps > 1) {
            summary("last", last);
            std::printf("drives %ld differing poses %d\n", reps, differing);
        }
        return differing ? 4 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
