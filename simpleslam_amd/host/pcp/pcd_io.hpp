// pcp/pcd_io.hpp -- PCD files in and out, without PCL: what test/loc.cpp and test/align.cpp feed the registration path with.
//
// Mirrors (reference): pcl::io::loadPCDFile<pcl::PointXYZI> as called at frontend/src/MapManager.cpp:68 (the map named by
// cfg["pcd_file"]), test/align.cpp:97-107 (target and source clouds) and common/pcp/pcp.hpp (savePCDFile).  The PCD format
// itself is PCL's (absent from the reference tree; restated from its published v0.7 layout): a text header
//   VERSION / FIELDS / SIZE / TYPE / COUNT / WIDTH / HEIGHT / VIEWPOINT / POINTS / DATA ascii|binary|binary_compressed
// followed by one record per point (the reader and writer themselves: csrc/pcd_format.h, which the library's pcr_pcd_read / pcr_pcd_write share).  Read: the fields named x, y, z (required) and intensity (optional, 0 when absent -- PCL
// warns and leaves the default) of any scalar TYPE/SIZE, in any order, other fields skipped ("_" padding of PCL's own binary
// files included); binary_compressed is PCL's LZF stream holding the fields one after the other.  Written: x y z intensity as
// F 4, ascii or binary.  Errors throw std::runtime_error; loadPCDFile returns -1 where PCL's returns -1 (file cannot be opened).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../PCR/HipRegister.hpp"
#include "../../csrc/pcd_format.h"

namespace pcp {

namespace detail {

using pcd::PcdField;
using pcd::pcd_scalar;
using pcd::lzf_decompress;

struct CloudSink {      // pcd::read into pcl::PointXYZI records
    PCR::PointCloud& cloud;
    void resize(size_t n) { cloud.points.clear(); cloud.points.resize(n); }
    void set(size_t p, int k, float v) {
        PCR::PointXYZI& q = cloud.points[p];
        if (k == 0) q.x = v; else if (k == 1) q.y = v; else if (k == 2) q.z = v; else q.intensity = v;
    }
};

}  // namespace detail

// pcl::io::loadPCDFile<pcl::PointXYZI>(file, cloud): 0 on success, -1 when the file cannot be opened; a malformed file throws.
inline int loadPCDFile(const std::string& path, PCR::PointCloud& cloud) {
    detail::CloudSink sink{cloud};
    return pcd::read(path, sink);
}

// pcl::io::savePCDFileBinary / savePCDFileASCII for PointXYZI clouds
inline int savePCDFile(const std::string& path, const PCR::PointCloud& cloud, bool binary = true) {
    return pcd::write(path, cloud.size(), [&](size_t p, float r[4]) {
        const PCR::PointXYZI& q = cloud.points[p];
        r[0] = q.x; r[1] = q.y; r[2] = q.z; r[3] = q.intensity;
    }, binary);
}

}  // namespace pcp
