// deskew_host.hip -- pcr_deskew_host (the definition: deskew_math.h's loop on host memory) and pcr_deskew (the same through deskew.hip's kernel, on
// the handle's stream).  Both make the checks of dsk::prepare before anything is written.  DESIGN 4.20.

#include <vector>

#include "handle.h"
#include "deskew_math.h"

using namespace pcr;
using namespace pcr::host;

extern "C" {

int pcr_deskew_host(const void* pts, size_t n, size_t stride_bytes, const void* times, int time_kind, long long time_offset_bytes,
                    const pcr_deskew_motion* m, void* out, pcr_deskew_info* info) {
    g_create_error.clear();
    const dsk::Call c{pts, n, stride_bytes, times, time_kind, time_offset_bytes, m, out, true};
    if (const char* why = dsk::deskew_host(c, info)) { g_create_error = std::string("pcr_deskew_host: ") + why; return 1; }
    return 0;
}

int pcr_deskew(pcr_handle* h, const void* pts, size_t n, size_t stride_bytes, int on_device, const void* times, int time_kind,
               long long time_offset_bytes, const pcr_deskew_motion* m, void* out, int out_on_device, pcr_deskew_info* info) {
    if (!h) return 1;
    h->err.clear();
    const dsk::Call c{pts, n, stride_bytes, times, time_kind, time_offset_bytes, m, out, (on_device != 0) == (out_on_device != 0)};
    // the control block as it goes up in one copy: the three counts (and a word of padding), zero, then the table
    constexpr size_t kHead = 4;
    std::vector<double> ctl(kHead + dsk::kRec * dsk::kMaxK, 0.0);
    dsk::Ref ref;
    if (const char* why = dsk::prepare(c, ctl.data() + kHead, &ref)) return fail(h, std::string("pcr_deskew: ") + why);
    if (n > kDeskewMaxPoints) return fail(h, "pcr_deskew: n is too large");
    pcr_deskew_info inf;
    memset(&inf, 0, sizeof inf);
    inf.ref_clamped = ref.clamped;
    if (n == 0) { if (info) *info = inf; return 0; }
    if (set_device(h)) return 1;

    const size_t bytes = n * stride_bytes, K = m->K;
    const float* d_pts = static_cast<const float*>(pts);
    const void* d_times = times;
    if (!on_device) {
        if (stage_host(h, &h->dsk.in, pts, n, stride_bytes, &d_pts, true)) return 1;
        if (times) {
            const size_t tb = n * (size_t)dsk::time_bytes(time_kind);
            H_TRY_DRAIN(h->dsk.times.reserve(tb));
            H_TRY_DRAIN(hipMemcpyAsync(h->dsk.times.p, times, tb, hipMemcpyHostToDevice, h->stream));
            d_times = h->dsk.times.p;
        }
    }
    // a result that goes back to the host is formed in place in the staged input, or in a buffer of the handle's when the input is the caller's
    void* d_out = out;
    if (!out_on_device) {
        if (on_device) { H_TRY_DRAIN(h->dsk.out.reserve(bytes)); d_out = h->dsk.out.p; }
        else d_out = h->dsk.in.p;
    }
    H_TRY_DRAIN(h->dsk.ctl.reserve(ctl.size() * sizeof(double)));
    H_TRY_DRAIN(h->dsk.ret.ensure(kHead));
    H_TRY_DRAIN(hipMemcpyAsync(h->dsk.ctl.p, ctl.data(), (kHead + dsk::kRec * K) * sizeof(double), hipMemcpyHostToDevice, h->stream));

    DeskewArgs a;
    a.pts = reinterpret_cast<const char*>(d_pts); a.times = static_cast<const char*>(d_times); a.out = static_cast<char*>(d_out);
    a.tab = h->dsk.ctl.as<double>() + kHead; a.counts = h->dsk.ctl.as<unsigned long long>();
    a.n = n; a.stride = (uint32_t)stride_bytes; a.time_off = times ? 0u : (uint32_t)time_offset_bytes;
    a.kind = time_kind; a.K = (int32_t)K; a.t0 = m->t0;
    for (int i = 0; i < 9; ++i) a.Rr[i] = ref.R[i];
    for (int i = 0; i < 3; ++i) a.pr[i] = ref.p[i];
    H_TRY_DRAIN(deskew_launch(a, h->stream));
    H_TRY_DRAIN(hipMemcpyAsync(h->dsk.ret.host, h->dsk.ctl.p, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    if (!out_on_device) H_TRY_DRAIN(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, h->stream));
    H_TRY(hipStreamSynchronize(h->stream));
    inf.before = (int64_t)h->dsk.ret.host[0]; inf.after = (int64_t)h->dsk.ret.host[1]; inf.nonfinite = (int64_t)h->dsk.ret.host[2];
    if (info) *info = inf;
    return 0;
}

}  // extern "C"
