// comm_host.hip -- the ranks of a sharded handle: the RCCL loader, the peer exchange's sessions, the all-reduce of host values,
// the tile a rank holds (pcr_set_shard, pcr_set_query_tile) and every pcr_comm_* entry point.

#include <dlfcn.h>

#include <algorithm>
#include <mutex>

#include "handle.h"

using namespace pcr;
using namespace pcr::host;

namespace {

// --- RCCL, loaded lazily (multi-GPU sharded mode only) ---------------------------
struct NcclId { char internal[128]; };
typedef int (*nccl_get_id_fn)(NcclId*);
typedef int (*nccl_init_rank_fn)(void**, int, NcclId, int);
typedef int (*nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_destroy_fn)(void*);
typedef int (*nccl_comm_int_fn)(void*, int*);
struct Rccl {
    void* lib = nullptr;
    nccl_get_id_fn get_id = nullptr;
    nccl_init_rank_fn init_rank = nullptr;
    nccl_allreduce_fn allreduce = nullptr;
    nccl_destroy_fn destroy = nullptr;
    nccl_comm_int_fn comm_count = nullptr, comm_user_rank = nullptr;
    bool load(std::string* err) {
        if (lib) return true;
        const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names) { lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (lib) break; }
        if (!lib) { if (err) *err = std::string("dlopen(librccl) failed: ") + dlerror(); return false; }
        get_id = (nccl_get_id_fn)dlsym(lib, "ncclGetUniqueId");
        init_rank = (nccl_init_rank_fn)dlsym(lib, "ncclCommInitRank");
        allreduce = (nccl_allreduce_fn)dlsym(lib, "ncclAllReduce");
        destroy = (nccl_destroy_fn)dlsym(lib, "ncclCommDestroy");
        comm_count = (nccl_comm_int_fn)dlsym(lib, "ncclCommCount");
        comm_user_rank = (nccl_comm_int_fn)dlsym(lib, "ncclCommUserRank");
        if (!get_id || !init_rank || !allreduce || !destroy) { if (err) *err = "librccl lacks ncclGetUniqueId/CommInitRank/AllReduce"; return false; }
        return true;
    }
};
Rccl g_rccl;
std::mutex g_rccl_mu;

}  // namespace

namespace pcr {
namespace host {

// the peer session, if one is open: the peers' buffers unmapped, the transport off (pcr_comm_init / pcr_comm_init_host / a new pcr_comm_init_peer / pcr_destroy)
void peer_close(pcr_handle* h) {
    if (h->comm.peer_on) for (int p = 0; p < h->comm.peer.nranks; ++p) if (p != h->comm.peer.rank && h->comm.peer.buf[p]) (void)hipIpcCloseMemHandle(h->comm.peer.buf[p]);
    memset(&h->comm.peer, 0, sizeof h->comm.peer);
    h->comm.peer_on = false; h->comm.peer_broken = false; h->comm.peer_seq = 0.0;
}
// before an exchange is queued / after its results have arrived: a session in which an exchange timed out is over
int peer_check(pcr_handle* h) {
    if (!h->comm.peer_on) return 0;
    if (h->comm.peer_status.host && __atomic_load_n(h->comm.peer_status.host, __ATOMIC_ACQUIRE) != 0) h->comm.peer_broken = true;
    if (h->comm.peer_broken)
        return fail(h, "peer exchange: a rank did not arrive within 2 s; the session is over (the ranks' sequence numbers no longer agree): "
                       "pcr_comm_peer_export + pcr_comm_init_peer on every rank start a new one");
    return 0;
}
// pcr_destroy: the RCCL communicator, the peer session and this rank's receive buffer
void comm_release(pcr_handle* h) {
    if (h->comm.rccl && g_rccl.destroy) g_rccl.destroy(h->comm.rccl);
    peer_close(h);
    if (h->comm.peer_own) (void)hipFree(h->comm.peer_own);
}

// n doubles in device memory summed over the ranks of the RCCL communicator, in place, on the handle's stream
int rccl_sum(pcr_handle* h, void* d_buf, size_t n) {
    const int rc = g_rccl.allreduce(d_buf, d_buf, n, /*ncclFloat64*/ 8, /*ncclSum*/ 0, h->comm.rccl, h->stream);
    if (rc != 0) return fail(h, "ncclAllReduce failed with code " + std::to_string(rc));
    return 0;
}

// Combine n (<= 64) doubles held in host memory over the ranks of a sharded handle, in place: the caller's collective, or RCCL
// through a device staging buffer.  The stream is idle when this is called (the values were just waited for).
int ranks_allreduce(pcr_handle* h, double* v, int n, int op) {
    if (h->comm.host_ar) {
        const int rc = h->comm.host_ar(v, (size_t)n, op, h->comm.host_ar_user);
        if (rc != 0) return fail(h, "the caller's all-reduce failed with code " + std::to_string(rc));
        return 0;
    }
    if (h->comm.peer_on) {
        if (peer_check(h)) return 1;
        H_TRY(h->comm.ar_stage.reserve(64 * sizeof(double)));
        H_TRY(hipMemcpyAsync(h->comm.ar_stage.p, v, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
        h->comm.peer_seq += 1.0;
        H_TRY(peer_launch_allreduce(h->comm.ar_stage.as<double>(), n, op, h->comm.peer, h->comm.peer_seq, h->stream));
        H_TRY(hipMemcpyAsync(v, h->comm.ar_stage.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        H_TRY(hipStreamSynchronize(h->stream));
        return peer_check(h);      // (the status word, not the values: a sum may be NaN in its own right)
    }
    if (h->comm.rccl) {
        H_TRY(h->comm.ar_stage.reserve(64 * sizeof(double)));
        H_TRY(hipMemcpyAsync(h->comm.ar_stage.p, v, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
        const int rc = g_rccl.allreduce(h->comm.ar_stage.p, h->comm.ar_stage.p, (size_t)n, /*ncclFloat64*/ 8, op == 1 ? /*ncclMax*/ 2 : /*ncclSum*/ 0, h->comm.rccl, h->stream);
        if (rc != 0) return fail(h, "ncclAllReduce failed with code " + std::to_string(rc));
        H_TRY(hipMemcpyAsync(v, h->comm.ar_stage.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        H_TRY(hipStreamSynchronize(h->stream));
    }
    return 0;
}

}  // namespace host
}  // namespace pcr

namespace {

// pcr_set_shard: faces farther out than this are open (the outer tiles reach to +-1e30, shard.py)
inline bool open_face(double v) { return !(fabs(v) < 1e29); }

// the entry points that give a handle a tile or a communicator: a method whose row of the method table says it is not shardable refuses, by name
int refuse_if_unshardable(pcr_handle* h, const char* entry_point) {
    if (ops(h).shardable) return 0;
    return fail(h, std::string(ops(h).name) + ": sharded targets are not supported in this version (" + entry_point + ")");
}

}  // namespace

namespace pcr {
namespace host {

static const char* ndt_search_name(int search) {
    return search == PCR_NDT_DIRECT26 ? "DIRECT26" : search == PCR_NDT_DIRECT1 ? "DIRECT1" : search == PCR_NDT_KDTREE ? "KDTREE" : "DIRECT7";
}
// What an ndt tile's halo must hold.  A scan point is evaluated by the rank whose tile [lo, hi) holds its transformed position; lo and hi are
// multiples of the resolution.  Every voxel the point's neighbourhood reaches must be COMPLETE on that rank (all of its points present):
//   the neighbourhood   DIRECT7 reaches one cell along an axis, DIRECT26 one cell along every axis at once -- the tile's extension
//                       [lo - halo, hi + halo) is a box (shard_extent), so the one voxel per axis that holds the face cells holds the edge and
//                       corner cells too; DIRECT1 reaches the point's own cell only: nothing
//   the rounding        the point's cell is floorf(p / leaf) and a target point's voxel floorf(p * (1 / leaf)), both in float
//                       (voxel_grid_covariance_omp_impl.hpp:380-382, :218-220): exact when the resolution is a power of two -- the cell then
//                       lies inside the tile and its points inside the cell -- and otherwise off by up to one cell at a face: one voxel more
double ndt_halo_need(int search, double res) {
    int e;
    const bool pow2 = frexp(res, &e) == 0.5;
    return ((search == PCR_NDT_DIRECT1 ? 0.0 : 1.0) + (pow2 ? 0.0 : 1.0)) * res;
}
std::string ndt_halo_message(int search, double need) {
    const std::string name = ndt_search_name(search);
    return "ndt: the halo must hold what the " + name + " neighbourhood (pcr_params.ndt_search) reads" +
           (search == PCR_NDT_DIRECT1 ? " (the point's own voxel where the float lattice rounds across a face)" : search == PCR_NDT_DIRECT26 ? " (the face, edge and corner voxels)" : " (the DIRECT7 face voxels)") +
           ": >= " + std::to_string(need) + " m at this resolution";
}

void shard_extent(const pcr_handle* h, double ext_lo[3], double ext_hi[3]) {
    for (int d = 0; d < 3; ++d) {
        ext_lo[d] = open_face(h->tile_lo[d]) ? -1e300 : h->tile_lo[d] - h->halo;
        ext_hi[d] = open_face(h->tile_hi[d]) ? 1e300 : h->tile_hi[d] + h->halo;
    }
}

// Sharded calls: before any rank enters an exchange loop every rank must know that ALL ranks have a usable target (a rank
// returning early would leave the others' collectives without a peer).  One MAX over the ranks of a status word.
int agree_prepared(pcr_handle* h, int rc_local) {
    if (!sharded(h)) return rc_local;
    const std::string err = h->err;
    double flag = rc_local ? 1.0 : 0.0;
    if (ranks_allreduce(h, &flag, 1, 1)) return 1;
    if (rc_local) { h->err = err; return 1; }
    if (flag != 0.0) return fail(h, "sharded call: another rank could not prepare its map tile");
    return 0;
}

}  // namespace host
}  // namespace pcr

extern "C" {

int pcr_set_query_tile(pcr_handle* h, const double lo[3], const double hi[3]) {
    if (!h) return 1;
    h->err.clear();
    if (!lo || !hi || lo[0] > hi[0]) { h->use_tile = 0; h->have_halo = false; return 0; }
    if (refuse_if_unshardable(h, "pcr_set_query_tile")) return 1;
    // NDT and VGICP tiles must sit on the voxel lattice and come with a halo that is checked: pcr_set_shard
    if (h->method != kLoam) return fail(h, "pcr_set_query_tile serves loam handles; ndt and vgicp tiles are set with pcr_set_shard (voxel-aligned bounds + halo)");
    h->use_tile = 1; h->have_halo = false;
    for (int d = 0; d < 3; ++d) { h->tile_lo[d] = lo[d]; h->tile_hi[d] = hi[d]; }
    return 0;
}

int pcr_set_shard(pcr_handle* h, const double lo[3], const double hi[3], double halo) {
    if (!h) return 1;
    h->err.clear();
    if (!lo || !hi || lo[0] > hi[0]) { h->use_tile = 0; h->have_halo = false; return 0; }
    if (refuse_if_unshardable(h, "pcr_set_shard")) return 1;
    if (!(halo >= 0.0)) return fail(h, "halo must be >= 0");
    for (int d = 0; d < 3; ++d) if (!(lo[d] < hi[d])) return fail(h, "tile bounds must satisfy lo < hi on every axis");
    auto on_lattice = [](double v, double res, double shift) {      // v = (k + shift) * res for an integer k, or an open face
        if (open_face(v)) return true;
        const double k = v / res - shift;
        return fabs(k - nearbyint(k)) <= 1e-9 * std::max(1.0, fabs(k));
    };
    if (h->method == kLoam) {
        const double gate = sqrt(std::max(0.0, h->prm.loam_knn_max_sq));
        if (halo < gate) return fail(h, "loam: the halo must cover the k-NN gate radius (" + std::to_string(gate) + " m, LoamRegister.cpp:59)");
    } else if (h->method == kNdt) {
        const double res = (double)(float)h->prm.ndt_resolution;
        for (int d = 0; d < 3; ++d)
            if (!on_lattice(lo[d], res, 0.0) || !on_lattice(hi[d], res, 0.0)) return fail(h, "ndt: tile bounds must be multiples of ndt_resolution (whole voxels per rank)");
        const double need = ndt_halo_need(h->prm.ndt_search, res);
        if (halo < need * (1.0 - 1e-12)) return fail(h, ndt_halo_message(h->prm.ndt_search, need));
    } else {
        if (const char* no = vgicp_search_shard_refusal(h, h->prm.vgicp_search, true)) return fail(h, no);
        const double res = h->prm.vgicp_resolution;
        for (int d = 0; d < 3; ++d)
            if (!on_lattice(lo[d], res, 0.5) || !on_lattice(hi[d], res, 0.5))
                return fail(h, "vgicp: tile bounds must lie on the voxel lattice, (k + 0.5) * vgicp_resolution (fast_vgicp_voxel.hpp:158-160)");
        if (halo < res) return fail(h, "vgicp: the halo must be at least one voxel (and hold every tile point's 20 nearest neighbours: checked per call)");
        h->target_ready = false;      // a target prepared for another tile was checked against another halo (vgicp_prepare_target: the halo check)
    }
    h->use_tile = 1; h->have_halo = true; h->halo = halo;
    for (int d = 0; d < 3; ++d) { h->tile_lo[d] = lo[d]; h->tile_hi[d] = hi[d]; }
    return 0;
}

int pcr_comm_init_host(pcr_handle* h, pcr_allreduce_fn fn, void* user, int rank, int nranks) {
    if (!h) return 1;
    h->err.clear();
    if (!fn) { h->comm.host_ar = nullptr; h->comm.host_ar_user = nullptr; if (!h->comm.rccl) { h->comm.nranks = 1; h->comm.rank = 0; } return 0; }
    if (refuse_if_unshardable(h, "pcr_comm_init_host")) return 1;
    if (const char* no = vgicp_search_shard_refusal(h, h->prm.vgicp_search, true)) return fail(h, no);
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(h, "bad communicator arguments");
    if (h->comm.rccl) return fail(h, "an RCCL communicator is already set on this handle");
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    peer_close(h);      // (one transport at a time)
    h->comm.host_ar = fn; h->comm.host_ar_user = user; h->comm.rank = rank; h->comm.nranks = nranks;
    return 0;
}

int pcr_comm_unique_id(void* out128) {
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (!out128 || !g_rccl.load(&g_create_error)) return 1;
    NcclId id;
    int rc = g_rccl.get_id(&id);
    if (rc != 0) { g_create_error = "ncclGetUniqueId failed with code " + std::to_string(rc); return 1; }
    memcpy(out128, &id, sizeof(id));
    return 0;
}

int pcr_comm_info(const pcr_handle* h, int* rank, int* nranks, int* transport) {
    if (!h) return 1;
    int r = h->comm.rank, n = h->comm.nranks, t = 0;
    if (h->comm.rccl) {
        // what the communicator itself reports, not what the caller passed to pcr_comm_init
        std::lock_guard<std::mutex> lk(g_rccl_mu);
        t = 1;
        if (g_rccl.comm_count && g_rccl.comm_count(h->comm.rccl, &n) != 0) return 1;
        if (g_rccl.comm_user_rank && g_rccl.comm_user_rank(h->comm.rccl, &r) != 0) return 1;
    } else if (h->comm.host_ar) t = 2;
    else if (h->comm.peer_on) t = 3;
    if (rank) *rank = r;
    if (nranks) *nranks = n;
    if (transport) *transport = t;
    return 0;
}

int pcr_comm_peer_export(pcr_handle* h, void* ipc_handle64) {
    if (!h) return 1;
    h->err.clear();
    if (!ipc_handle64) return fail(h, "ipc_handle64 is NULL");
    if (set_device(h)) return 1;
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "the C ABI says 64 bytes");
    const size_t bytes = (size_t)2 * kMaxPeers * kPeerSlot * sizeof(double);
    if (h->stream) H_TRY(hipStreamSynchronize(h->stream));      // (nothing of an earlier session is in flight)
    if (!h->comm.peer_own) {
        // fine-grained: the peers' stores and this rank's polls meet in memory, not in a cache that nobody invalidates inside a kernel.  No
        // fallback to ordinary (coarse-grained) memory: remote stores might never be seen there, and every exchange would run into its timeout.
        const hipError_t e = hipExtMallocWithFlags((void**)&h->comm.peer_own, bytes, hipDeviceMallocFinegrained);
        if (e != hipSuccess) { (void)hipGetLastError(); h->comm.peer_own = nullptr; return fail(h, std::string("peer exchange: no fine-grained device memory for the receive buffer (") + hipGetErrorString(e) + ")"); }
    }
    H_TRY(h->comm.peer_status.ensure(16));      // (64 bytes)
    // EVERY export starts a session from nothing: sequence words of an earlier session could otherwise match the new one's.  The ranks share their
    // handles only after every rank has exported (that exchange is the barrier): no peer writes into this buffer before it has been cleared.
    H_TRY(hipMemset(h->comm.peer_own, 0, bytes));
    H_TRY(hipDeviceSynchronize());
    *h->comm.peer_status.host = 0;
    h->comm.peer_exported = true;
    hipIpcMemHandle_t mh;
    H_TRY(hipIpcGetMemHandle(&mh, h->comm.peer_own));
    memcpy(ipc_handle64, &mh, 64);
    return 0;
}

int pcr_comm_init_peer(pcr_handle* h, const void* ipc_handles, int rank, int nranks) {
    if (!h) return 1;
    h->err.clear();
    if (refuse_if_unshardable(h, "pcr_comm_init_peer")) return 1;
    if (const char* no = vgicp_search_shard_refusal(h, h->prm.vgicp_search, true)) return fail(h, no);
    if (!ipc_handles || nranks < 1 || nranks > kMaxPeers || rank < 0 || rank >= nranks) return fail(h, "bad peer-exchange arguments (at most 8 ranks)");
    if (!h->comm.peer_own || !h->comm.peer_exported) return fail(h, "call pcr_comm_peer_export first (every rank, for every session), then share the handles");
    if (h->comm.rccl) return fail(h, "an RCCL communicator is already set on this handle");
    if (set_device(h)) return 1;
    if (h->stream) H_TRY(hipStreamSynchronize(h->stream));
    peer_close(h);      // (the mappings of an earlier session)
    h->comm.peer_exported = false;
    for (int p = 0; p < nranks; ++p) {
        if (p == rank) { h->comm.peer.buf[p] = h->comm.peer_own; continue; }
        hipIpcMemHandle_t mh;
        memcpy(&mh, (const char*)ipc_handles + (size_t)p * 64, 64);
        void* mapped = nullptr;
        const hipError_t e = hipIpcOpenMemHandle(&mapped, mh, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            for (int q = 0; q < p; ++q) if (q != rank && h->comm.peer.buf[q]) (void)hipIpcCloseMemHandle(h->comm.peer.buf[q]);
            memset(&h->comm.peer, 0, sizeof h->comm.peer);
            return fail(h, std::string("hipIpcOpenMemHandle of rank ") + std::to_string(p) + "'s receive buffer: " + hipGetErrorString(e));
        }
        h->comm.peer.buf[p] = (double*)mapped;
    }
    h->comm.peer.rank = rank; h->comm.peer.nranks = nranks; h->comm.peer.status = h->comm.peer_status.dev;
    h->comm.rank = rank; h->comm.nranks = nranks;
    h->comm.peer_seq = 0.0;
    h->comm.peer_on = true; h->comm.peer_broken = false;
    h->comm.host_ar = nullptr; h->comm.host_ar_user = nullptr;
    return 0;
}

int pcr_comm_init(pcr_handle* h, const void* unique_id128, int rank, int nranks) {
    if (!h) return 1;
    h->err.clear();
    if (refuse_if_unshardable(h, "pcr_comm_init")) return 1;
    if (const char* no = vgicp_search_shard_refusal(h, h->prm.vgicp_search, true)) return fail(h, no);
    if (!unique_id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(h, "bad communicator arguments");
    if (set_device(h)) return 1;
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (!g_rccl.load(&h->err)) return 1;
    NcclId id;
    memcpy(&id, unique_id128, sizeof(id));
    if (h->comm.rccl) return fail(h, "an RCCL communicator is already set on this handle");
    int rc = g_rccl.init_rank(&h->comm.rccl, nranks, id, rank);
    if (rc != 0) { h->comm.rccl = nullptr; return fail(h, "ncclCommInitRank failed with code " + std::to_string(rc)); }
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    peer_close(h);      // (one transport at a time)
    h->comm.nranks = nranks; h->comm.rank = rank;
    h->comm.host_ar = nullptr; h->comm.host_ar_user = nullptr;
    return 0;
}

}  // extern "C"
