// voxel_sparse_check -- pcp::VoxelDownSampleV3 and pcp::VoxelDownSampleV2 of the C++ mirror (PCR/HipRegister.hpp) on a PCD file, on the GPU:
//   voxel_sparse_check <cloud.pcd> <grid_size> [max_voxel_pts min_voxel_pts]
// prints, per class, the number of points it returned and a checksum over their bytes (FNV-1a, 64 bit, over x y z w intensity of every point in
// output order), V3 also through its in-place form (cloud == out).  tests/test_voxel_sparse_gpu.py compares the lines with Python's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "PCR/HipRegister.hpp"
#include "pcp/pcd_io.hpp"

static uint64_t checksum(const PCR::PointCloud& c) {
    uint64_t h = 1469598103934665603ull;
    for (const PCR::PointXYZI& p : c.points) {
        const float v[5] = {p.x, p.y, p.z, p.w, p.intensity};
        unsigned char b[sizeof(v)];
        memcpy(b, v, sizeof(v));
        for (unsigned char x : b) { h ^= x; h *= 1099511628211ull; }
    }
    return h;
}

int main(int argc, char** argv) {
    if (argc != 3 && argc != 5) { std::fprintf(stderr, "usage: voxel_sparse_check <cloud.pcd> <grid_size> [max_voxel_pts min_voxel_pts]\n"); return 2; }
    PCR::PC_Ptr cloud = std::make_shared<PCR::PointCloud>();
    if (pcp::loadPCDFile(argv[1], *cloud) != 0) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 4; }
    const float gs = (float)std::atof(argv[2]);
    const int max_vp = argc == 5 ? std::atoi(argv[3]) : 20, min_vp = argc == 5 ? std::atoi(argv[4]) : 0;
    try {
        std::printf("input %zu\n", cloud->size());
        pcp::VoxelDownSampleV3 v3(gs);
        PCR::PC_Ptr out3 = std::make_shared<PCR::PointCloud>();
        v3.filter<PCR::PointXYZI>(cloud, out3);
        std::printf("v3 %zu %016llx\n", out3->size(), (unsigned long long)checksum(*out3));
        pcp::VoxelDownSampleV2 v2(gs, max_vp, min_vp);
        PCR::PC_Ptr out2 = v2.filter<PCR::PointXYZI>(cloud);
        std::printf("v2 %zu %016llx\n", out2->size(), (unsigned long long)checksum(*out2));
        PCR::PC_Ptr same = std::make_shared<PCR::PointCloud>(*cloud);      // cloud.get() == out.get(), pcp.hpp:222
        v3.filter<PCR::PointXYZI>(same, same);
        std::printf("v3_in_place %zu %016llx\n", same->size(), (unsigned long long)checksum(*same));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
