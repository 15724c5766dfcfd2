// staging_host.hip -- host clouds on their way into HBM, the handle's result blocks, and the host ranges the caller page-locked.

#include <mutex>
#include <vector>

#include "handle.h"

using namespace pcr;
using namespace pcr::host;

// ---- host ranges page-locked by pcr_host_pin, and who copies out of them ----
// pcr_host_unpin must not unregister a range while a copy out of it is in flight.  Every upload that reads a pinned range notes (device, stream)
// with the range; unpinning waits for exactly those streams -- not for every device of the node (which created a context on each of them, waited
// for unrelated work, and switched the calling thread's device: ADVICE r4).  A handle that goes away, or is given another stream, takes its
// entries with it (after waiting for its own stream).

namespace {

struct PinUse { int device; hipStream_t stream; };
struct PinnedRange { const void* p; size_t bytes; std::vector<PinUse> uses; };
std::mutex g_pin_mu;
std::vector<PinnedRange> g_pinned;
void pin_note_copy(const void* src, size_t bytes, int device, hipStream_t stream) {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    if (g_pinned.empty()) return;
    const char* a = (const char*)src;
    for (PinnedRange& r : g_pinned) {
        const char* b = (const char*)r.p;
        if (a < b + r.bytes && b < a + bytes) {      // the copy reads from the range
            bool known = false;
            for (const PinUse& u : r.uses) known = known || (u.device == device && u.stream == stream);
            if (!known) r.uses.push_back(PinUse{device, stream});
        }
    }
}

}  // namespace

namespace pcr {
namespace host {

void pin_forget_stream(hipStream_t stream) {      // (the caller has waited for the stream)
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (PinnedRange& r : g_pinned)
        for (size_t i = r.uses.size(); i-- > 0;) if (r.uses[i].stream == stream) r.uses.erase(r.uses.begin() + (long)i);
}

// Host clouds are uploaded verbatim.  pcr_params.host_copy_xyz = 1: of records wider than 16 bytes (pcl::PointXYZI is 32: basic.hpp:16 -- what
// the plugin adapter hands over) only the first 16 bytes cross PCIe, by a pitched copy into a staging area of the SAME stride
// (nothing downstream changes; whole_records: every field is needed -- pcr_voxel_filter).  Measured and NOT the default: the pitched copy of a
// 1 M-point map takes 3.5 ms, pageable or page-locked, where the verbatim copy of twice the bytes takes 0.6 ms.
int stage_host(pcr_handle* h, DeviceBuf* buf, const void* src, size_t n, size_t stride_bytes, const float** out, bool whole_records) {
    const size_t bytes = n * stride_bytes;
    H_TRY(buf->reserve(bytes ? bytes : 16));
    if (bytes) {
        if (stride_bytes > 16 && !whole_records && h->prm.host_copy_xyz == 1)
            H_TRY(hipMemcpy2DAsync(buf->p, stride_bytes, src, stride_bytes, 16, n, hipMemcpyHostToDevice, h->stream));
        else
            H_TRY(hipMemcpyAsync(buf->p, src, bytes, hipMemcpyHostToDevice, h->stream));
        pin_note_copy(src, bytes, h->device, h->stream);
    }
    *out = buf->as<float>();
    return 0;
}

int check_stride(pcr_handle* h, size_t stride_bytes) {
    if (stride_bytes < 12 || stride_bytes % 4 != 0) return fail(h, "stride_bytes must be a multiple of 4 and >= 12");
    return 0;
}

int set_device(pcr_handle* h) {
    H_TRY(hipSetDevice(h->device));
    return 0;
}

int ensure_out32(pcr_handle* h) {
    H_TRY(h->out32.ensure(32));
    H_TRY(h->vg_partials.reserve((size_t)512 * 32 * sizeof(double)));
    return 0;
}

// Wait until the kernel that was given `seq` has written it into the last word of a host-mapped result block (it does so
// after everything else, with a system-scope release).  A short spin returns ~15 us before a sleeping thread would be
// woken by the stream's completion signal, and the LM / line-search drivers wait like this a dozen times per call.
int wait_result(pcr_handle* h, const double* flag_word, double seq) {
    const volatile double* f = flag_word;
    if (h->profile == 0) {
        for (int spin = 0; spin < 200000 && *f != seq; ++spin) __builtin_ia32_pause();
        std::atomic_thread_fence(std::memory_order_acquire);
        if (*f == seq) return 0;
    }
    H_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

}  // namespace host
}  // namespace pcr

extern "C" {

// ---- host buffers handed to pcr_scan2map / pcr_set_target / pcr_align: page-locking them is the caller's call ----
// hipMemcpyAsync from pageable memory goes through the runtime's own staging buffers; from a registered range the copy engine reads the
// caller's pages directly.  The registration is keyed on what the caller SAYS -- (pointer, size), pinned until pcr_host_unpin -- never on
// what the library guesses from a pointer it has seen before: a buffer that was freed and allocated again at the same address would be
// read through stale page mappings (the hazard of SURVEY F10, one level down).
int pcr_host_pin(const void* ptr, size_t bytes) {
    g_create_error.clear();
    if (!ptr || !bytes) { g_create_error = "pcr_host_pin: NULL or empty range"; return 1; }
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (const PinnedRange& r : g_pinned)
        if (r.p == ptr) {
            if (r.bytes == bytes) return 0;      // the same range again: nothing to do
            g_create_error = "pcr_host_pin: this address is already pinned with another size (pcr_host_unpin it first)";
            return 1;
        }
    const hipError_t e = hipHostRegister(const_cast<void*>(ptr), bytes, hipHostRegisterDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); g_create_error = std::string("hipHostRegister: ") + hipGetErrorString(e); return 1; }
    g_pinned.push_back(PinnedRange{ptr, bytes, {}});
    return 0;
}

int pcr_host_unpin(const void* ptr) {
    g_create_error.clear();
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (size_t i = 0; i < g_pinned.size(); ++i)
        if (g_pinned[i].p == ptr) {
            {   // no copy out of the range may still be in flight: the streams that have copied from it (stage_host notes them), and only those
                int cur = -1;
                const bool have_cur = hipGetDevice(&cur) == hipSuccess;
                for (const PinUse& u : g_pinned[i].uses) {
                    if (hipSetDevice(u.device) != hipSuccess) { (void)hipGetLastError(); continue; }
                    if (hipStreamSynchronize(u.stream) != hipSuccess) (void)hipGetLastError();
                }
                if (have_cur && !g_pinned[i].uses.empty()) (void)hipSetDevice(cur);
            }
            const hipError_t e = hipHostUnregister(const_cast<void*>(ptr));
            g_pinned.erase(g_pinned.begin() + (long)i);
            if (e != hipSuccess) { (void)hipGetLastError(); g_create_error = std::string("hipHostUnregister: ") + hipGetErrorString(e); return 1; }
            return 0;
        }
    g_create_error = "pcr_host_unpin: this address was not pinned with pcr_host_pin";
    return 1;
}

}  // extern "C"
