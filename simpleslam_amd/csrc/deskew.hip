// deskew.hip -- pcr_deskew's kernel: every point of a sweep moved from the sensor frame at its own time into the sensor frame at one reference
// time.  The arithmetic is deskew_math.h's, which pcr_deskew_host runs on the host: the two agree bit for bit.  DESIGN 4.20.

#include "pcr_internal.h"
#include "deskew_math.h"

using namespace pcr;

namespace {

constexpr int kThreads = 256;
static_assert(kDeskewMaxPoints == 0x7fffffffull * kThreads, "the largest grid covers kDeskewMaxPoints");

// Lane i of the grid owns record i (a 64-bit index; byte offsets are formed in 64 bits) and touches nothing else of pts / out: it reads its
// record's coordinates and time words first and writes afterwards, so out == pts is safe.  Every access lies inside record i < n -- words
// [0, stride / 4) of it, the time field inside the stride by the host's check -- or inside element i of the packed times; the table is read at
// records [0, K) (dsk::eval).  Records are 4-byte aligned at least, so everything moves as 32-bit words (a double time as two).
// The control table is read with plain loads and not staged in LDS: a point needs two records and log2 K stamps of it, the points of a sweep
// come in time order so a wave's lanes ask for the same few cache lines, and the whole table (at most 64 KB) stays in L2; staging it would
// load up to 64 KB per block to serve the 9 KB of a block's points.
// The counts: one ballot per wave and counter, one integer atomic per wave that has something to add -- sums of integers, no order to depend on.
__global__ __launch_bounds__(kThreads) void deskew_kernel(const DeskewArgs a) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
    bool before = false, after = false, bad = false;
    if (i < a.n) {
        const uint32_t* rec = reinterpret_cast<const uint32_t*>(a.pts + i * a.stride);
        uint32_t* dst = reinterpret_cast<uint32_t*>(a.out + i * a.stride);
        const uint32_t* tw = a.times ? reinterpret_cast<const uint32_t*>(a.times + i * (unsigned long long)dsk::time_bytes(a.kind))
                                     : rec + a.time_off / 4;
        const uint32_t w0 = tw[0], w1 = a.kind == PCR_TIME_F64_SECONDS ? tw[1] : 0u;
        const uint32_t cx = rec[0], cy = rec[1], cz = rec[2];
        const uint32_t words = a.stride / 4;
        if (dst != rec) for (uint32_t w = 3; w < words; ++w) dst[w] = rec[w];
        const float fx = __uint_as_float(cx), fy = __uint_as_float(cy), fz = __uint_as_float(cz);
        const double tau = dsk::time_of(a.kind, w0, w1, a.t0);
        float o[3] = {fx, fy, fz};
        if (dsk::record_finite(fx, fy, fz, tau)) {
            double R[9], p[3];
            const int cl = dsk::eval(a.tab, a.K, tau, R, p);
            before = cl < 0; after = cl > 0;
            dsk::move_point(R, p, a.Rr, a.pr, fx, fy, fz, o);
            dst[0] = __float_as_uint(o[0]); dst[1] = __float_as_uint(o[1]); dst[2] = __float_as_uint(o[2]);
        } else {
            bad = true;
            if (dst != rec) { dst[0] = cx; dst[1] = cy; dst[2] = cz; }
        }
    }
    const unsigned long long nb = __popcll(__ballot(before)), na = __popcll(__ballot(after)), nn = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0) {
        if (nb) atomicAdd(a.counts + 0, nb);
        if (na) atomicAdd(a.counts + 1, na);
        if (nn) atomicAdd(a.counts + 2, nn);
    }
}

}  // namespace

namespace pcr {

hipError_t deskew_launch(const DeskewArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    if (a.n > kDeskewMaxPoints) return hipErrorInvalidValue;
    const unsigned int blocks = (unsigned int)((a.n + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(deskew_kernel, dim3(blocks), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace pcr
