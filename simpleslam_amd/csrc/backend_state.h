// backend_state.h -- struct pcr_backend, shared by the two host units that work on it: backend_host.hip (the events) and session_host.hip
// (a session to and from disk).  Host code only.
#pragma once
#include <string>
#include <vector>

#include "../../include/pcr_hip.h"

struct pcr_backend {
    pcr_map* map = nullptr;         // borrowed: the store (a parent)
    pcr_map* view = nullptr;        // lc_map_
    pcr_sc* sc = nullptr;
    pcr_handle* reg = nullptr;      // pcr_ with initForLC's settings
    pcr_graph* graph = nullptr;
    pcr_backend_params prm{};
    int device = 0;
    size_t done = 0;                // key frames the graph holds
    size_t lc_done = 0;             // contexts lcHandler has walked (lc_size_)
    std::vector<pcr_backend_loop> loops;
    bool failed = false;            // an inner call of an event failed: the state is partial until pcr_backend_reset
    std::string failure;
    std::string err;
    std::string save_dir;           // saveMapDir (pcr_backend_set_save_dir); empty: nothing is written
    double load_seconds[5] = {0, 0, 0, 0, 0};      // pcr_backend_load_seconds
};

namespace pcr {
// (session_host.hip) {dir}/{i}.pcd for key frames [first, n) of the store as it holds them now; nonzero with the message in *err
int session_write_keyframes(const pcr_map* m, const std::string& dir, size_t first, std::string* err);
}  // namespace pcr
