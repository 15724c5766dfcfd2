// sc_loops_check.cpp -- loop discovery over a range of stored key frames through the C++ mirror (context::ScanContext), on the GPU:
//   50 contexts added (the last 15 revisit the first 15 with a yaw of 4 sectors) -> findLoops(0, 50) and rankStored(0, 50, 3)
// against what a host loop of pcr_sc_distance over the same (query, candidate) pairs gives: the (dist, index) minimum, the strict
// threshold, the yaw of pcr_sc_query's helper, every figure to the bit.
// Exit code 0 and "sc_loops_check ok"; 1 with a message on the first mismatch.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "PCR/HipRegister.hpp"

namespace {

[[noreturn]] void die(const std::string& what) {
    std::fprintf(stderr, "sc_loops_check: %s\n", what.c_str());
    std::exit(1);
}

// a few hundred points of a scene that differs from place to place, seen after a yaw of `sectors` sectors
PCR::PointCloud scan(unsigned place, int sectors) {
    PCR::PointCloud pc;
    unsigned long long s = 0x9E3779B97F4A7C15ull * (place + 1);
    auto next = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; };
    const double th = sectors * 6.0 * 3.14159265358979323846 / 180.0;
    for (int i = 0; i < 400; ++i) {
        const double r = 0.5 + 74.5 * next(), a = -3.14159265358979323846 + 6.28318530717958647692 * next(), h = -2.0 + 8.0 * next();
        PCR::PointXYZI p;
        p.x = (float)(r * std::cos(a + th)); p.y = (float)(r * std::sin(a + th)); p.z = (float)(h * (1 + std::sin(3 * a + place)));
        pc.points.push_back(p);
    }
    return pc;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

}  // namespace

int main() {
    try {
        const int kN = 50, kExcl = 10, kK = 3;
        pcr_sc_params prm;
        pcr_sc_default_params(&prm);
        prm.num_exclude_recent = kExcl;
        prm.dist_thres = 0.5;
        context::ScanContext sc(&prm);
        for (int i = 0; i < kN; ++i) sc.addContext(i < 35 ? scan(i, 0) : scan(i - 35, 4));
        if (sc.size() != (size_t)kN) die("the database does not hold what was added");

        const auto loops = sc.findLoops(0, kN);
        const auto rank = sc.rankStored(0, kN, kK);
        if (loops.size() != (size_t)kN || rank.idx.size() != (size_t)kN * kK) die("a result of another size than asked for");
        int found = 0;
        for (int q = 0; q < kN; ++q) {
            std::vector<std::tuple<double, int, int>> all;      // (dist, candidate, shift) of the host function, sorted by (dist, candidate)
            for (int i = 0; i < q - kExcl; ++i) {
                double d; int sh;
                if (pcr_sc_distance(sc.handle(), q, i, &d, &sh)) die("pcr_sc_distance failed");
                all.emplace_back(d, i, sh);
            }
            std::sort(all.begin(), all.end());
            for (int r = 0; r < kK; ++r) {
                const size_t at = (size_t)q * kK + r;
                const bool have = r < (int)all.size();
                const double d = have ? std::get<0>(all[r]) : DBL_MAX;
                const int64_t i = have ? std::get<1>(all[r]) : -1;
                const int32_t sh = have ? std::get<2>(all[r]) : 0;
                if (rank.idx[at] != i || !same_bits(rank.dist[at], d) || rank.shift[at] != sh)
                    die("rankStored: query " + std::to_string(q) + " place " + std::to_string(r) + " is (" + std::to_string(rank.idx[at]) + ", " +
                        std::to_string(rank.dist[at]) + ", " + std::to_string(rank.shift[at]) + "), the host loop gives (" + std::to_string(i) + ", " +
                        std::to_string(d) + ", " + std::to_string(sh) + ")");
            }
            const auto& l = loops[q];
            const bool hit = !all.empty() && !(std::get<0>(all[0]) > (double)(float)prm.dist_thres);
            const int match = hit ? std::get<1>(all[0]) : -1;
            const float yaw = hit ? pcr_sc_shift_yaw(std::get<2>(all[0])) : 0.f;
            const double md = all.empty() ? DBL_MAX : std::get<0>(all[0]);
            if (l.id != q || l.match != match || std::memcmp(&l.yaw, &yaw, sizeof yaw) || !same_bits(l.min_dist, md))
                die("findLoops: query " + std::to_string(q) + " gives match " + std::to_string(l.match) + ", the host loop " + std::to_string(match));
            if (q >= 35 && l.match == q - 35) {
                ++found;
                if (std::fabs(l.yaw - 4 * 6.0 * 3.14159265358979323846 / 180.0) > 1e-6) die("a revisit was found at another yaw than it was made with");
            }
        }
        if (found < 12) die("only " + std::to_string(found) + " of the 15 revisits were found");
        std::printf("sc_loops_check ok\n");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "sc_loops_check: error: %s\n", e.what());
        return 1;
    }
}
