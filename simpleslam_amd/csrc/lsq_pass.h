// lsq_pass.h -- one pass of fast_gicp::LsqRegistration's Gauss-Newton / Levenberg-Marquardt loop on the device, for the methods that
// run it (vgicp.hip, gicp.hip): the fixed-order block reduction of a pass's 28 or 29 sums into [block][32] rows, the fold of the
// previous launch's rows, and a launch of the device-resident loop -- its prologue and its pass (vgicp_opt.h: VgCtl, ctl_step).  A unit brings
// its per-point functions in a small method type:
//     void   lin(const Pose16& T, uint32_t i, double v[28], bool to_next)   update_correspondences + linearize of source point i; the pair goes
//                                                                           to the current correspondence buffers, or to the other pair
//     double err(const Pose16& T, uint32_t i)                               compute_error of point i on the current buffers
// No atomics anywhere: the same numbers are added in the same order whatever the launch -- device loop equals host loop, sharded equals
// unsharded, bit for bit.  Kernel code only (hipcc); the host units see the launchers in pcr_internal.h.
#pragma once
#include "pcr_internal.h"
#include "vgicp_opt.h"

namespace pcr {

static constexpr int kLinStride = 258;      // row stride of the block reduction's [29][256] doubles in LDS
static constexpr int kVgCtlWords = (int)((sizeof(VgCtl) + 3) / 4);
static_assert(sizeof(VgCtl) % 4 == 0, "VgCtl is copied word by word");

// kWithError = false: linearize(T) -- correspondences to the current buffers, partial sums [0..27].
// kWithError = true: one pass for an LM trial pose T: [28] = compute_error(T) on the correspondences of the last linearisation (the current
// buffers, read only) AND, speculatively, the linearisation AT T (correspondences to the other buffers, sums [0..27]).  When the trial is
// accepted -- the usual case -- T is the next linearisation point and the buffers change places instead of another launch and round trip;
// when it is rejected the sums are dropped.  One source point per thread; both kinds of sums leave through the same fixed-order LDS
// reduction into [block][32] rows: bit-identical values.
template <bool kWithError, class Method>
__device__ __forceinline__ void lsq_lin_body(const Method& m, const Pose16& T, uint32_t n_src, double* __restrict__ partials,
                                             double* sh /* [29][kLinStride] */, double* sh_sum /* [8][32] */) {
    constexpr int kRows = kWithError ? 29 : 28;
    const int tid = threadIdx.x, e = tid & 31, ch = tid >> 5;
    double acc = 0.0;
    for (uint32_t base = blockIdx.x * 256; base < n_src; base += gridDim.x * 256) {
        const uint32_t i = base + tid;
        double v[28];
#pragma unroll
        for (int k = 0; k < 28; ++k) v[k] = 0.0;
        double err = 0.0;
        if (i < n_src) {
            if (kWithError) err = m.err(T, i);
            m.lin(T, i, v, kWithError);
        }
#pragma unroll
        for (int k = 0; k < 28; ++k) sh[k * kLinStride + tid] = v[k];
        if (kWithError) sh[28 * kLinStride + tid] = err;
        __syncthreads();
        if (e < kRows) {
            const double* row = sh + e * kLinStride + ch * 32;
#pragma unroll 8
            for (int k = 0; k < 32; ++k) acc += row[k];
        }
        __syncthreads();
    }
    sh_sum[ch * 32 + e] = e < kRows ? acc : 0.0;
    __syncthreads();
    if (tid < 32) {
        double s = sh_sum[tid];
#pragma unroll
        for (int c = 1; c < 8; ++c) s += sh_sum[c * 32 + tid];
        partials[(size_t)blockIdx.x * 32 + tid] = s;
    }
}

// A thread's share of the fold of a launch's rows ([n_rows][32], n_rows <= 512): component t & 31 of the rows r0 + (t >> 5) + 8 u, u
// ascending, r0 = 0, 256 -- 32 loads in flight per round.  The eight slices of a component are added by the caller, in slice order.
// first: there are no rows yet (zeros).  kWithCtl (the prologue of a pass): the state's words are requested behind the first round's
// rows and in front of its additions, so that both arrive in one round trip.
template <bool kWithCtl>
__device__ __forceinline__ double lsq_fold_rows(const double* __restrict__ rows, uint32_t n_rows, int first, const VgCtl* ctl, uint32_t* sh_ctl) {
    const int t = threadIdx.x, comp = t & 31, slice = t >> 5;
    double acc = 0.0;
    double v[32];
#pragma unroll
    for (int u = 0; u < 32; ++u) {
        const uint32_t row = (uint32_t)(slice + 8 * u);
        v[u] = (!first && row < n_rows) ? rows[(size_t)row * 32 + comp] : 0.0;
    }
    if (kWithCtl) for (int w = t; w < kVgCtlWords; w += 256) sh_ctl[w] = reinterpret_cast<const uint32_t*>(ctl)[w];
#pragma unroll
    for (int u = 0; u < 32; ++u) acc += v[u];
    if (!first)
        for (uint32_t r0 = 256; r0 < n_rows; r0 += 256) {      // (more than 65 536 source points: 512 rows)
#pragma unroll
            for (int u = 0; u < 32; ++u) {
                const uint32_t row = r0 + (uint32_t)(slice + 8 * u);
                v[u] = row < n_rows ? rows[(size_t)row * 32 + comp] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 32; ++u) acc += v[u];
        }
    return acc;
}

// ------------------------------------------------------------------------------
// Device-resident Levenberg-Marquardt loop: one launch per pass.  The prologue of a launch folds the 29 sums of the previous one and
// takes the optimiser's step (vgicp_opt.h: ctl_step) -- in every block, the same instructions on the same numbers, as
// ndt_pass_pro_kernel and loam_iterate_kernel do; block 0 writes the new state and the progress word.  State and rows are
// double-buffered by launch parity; the two correspondence buffers are chosen by the state's own parity (an accepted trial makes
// the buffer it wrote the current one).  The loop ends in the prologue of the launch after its last pass.
// ------------------------------------------------------------------------------
struct LsqProArgs {
    const double* rows_prev;     // [rows_prev_n][32]
    const VgCtl* ctl_prev;
    VgCtl* ctl_next;
    VgOut* out;
    double seq;
    uint32_t rows_prev_n;
    int32_t first;
    const double* reduced;       // sharded over the peer exchange: the previous launch's 32 sums, already folded over the rows AND the ranks (vgicp_peer_exchange_kernel); else NULL
};

// launch `index` of the loop over nb blocks: d_ctl2 = two VgCtl, d_rows2 = two buffers of 512 * 32 doubles, this launch's at lsq_rows()
inline double* lsq_rows(double* d_rows2, int index) { return d_rows2 + (size_t)(index & 1) * 512 * 32; }
inline LsqProArgs lsq_pro_args(VgCtl* d_ctl2, double* d_rows2, VgOut* d_out, double seq, int index, uint32_t nb) {
    LsqProArgs pa;
    pa.rows_prev = lsq_rows(d_rows2, index + 1);
    pa.ctl_prev = index == 0 ? d_ctl2 : d_ctl2 + ((index + 1) & 1);
    pa.ctl_next = d_ctl2 + (index & 1);
    pa.out = d_out; pa.seq = seq; pa.rows_prev_n = nb; pa.first = index == 0 ? 1 : 0;
    pa.reduced = nullptr;
    return pa;
}

// A launch of the loop: everything in front of its pass -- the fold, the step, the state handed on, the result or the progress word -- and,
// unless the loop has finished, the pass of Method over `a_in` with the correspondence buffers as the state's parity says, at the state's pose.
// kPeer: pa.reduced may carry the sums (the peer exchange).  roi_escapes: the counter reported with the result (a target prepared for one
// scan), or NULL.  (One function, whose early returns end the kernel: behind a prologue that returned "there is a pass" to its caller the
// compiler scheduled the candidate loop of GICP's search with one wait for its four loads; this way it is the schedule of the kernel that had
// the prologue written out, profiles/gicp_notes.md.)
template <bool kPeer, class Method, class Args>
__device__ __forceinline__ void lsq_pass(const Args& a_in, const LsqProArgs& pa, const uint32_t* __restrict__ roi_escapes, double* sh /* [29][kLinStride] */,
                                         double* sh_sum /* [8][32] */, uint32_t* sh_ctl /* [kVgCtlWords] */, double* sh_sums /* [32] */) {
    const int t = threadIdx.x;
    VgCtl* const c = reinterpret_cast<VgCtl*>(sh_ctl);
    // one round trip: the state and the rows of the previous launch ([8 slices][32 components], 32 rows a thread for <= 256 rows)
    const int comp = t & 31, slice = t >> 5;
    double acc = 0.0;
    if (kPeer && pa.reduced) {      // (block-uniform) the sums arrive folded: slice 0 carries them, the others zeros
        if (!pa.first && slice == 0) acc = pa.reduced[comp];
        for (int w = t; w < kVgCtlWords; w += 256) sh_ctl[w] = reinterpret_cast<const uint32_t*>(pa.ctl_prev)[w];
    } else {
        acc = lsq_fold_rows<true>(pa.rows_prev, pa.rows_prev_n, pa.first, pa.ctl_prev, sh_ctl);
    }
    sh_sum[slice * 32 + comp] = acc;
    __syncthreads();
    if (c->done) {      // finished in an earlier launch: hand the state on to whatever is queued behind
        if (blockIdx.x == 0) for (int w = t; w < kVgCtlWords; w += 256) reinterpret_cast<uint32_t*>(pa.ctl_next)[w] = sh_ctl[w];
        return;
    }
    if (!pa.first) {
        if (t < 32) {
            double s = sh_sum[t];
#pragma unroll
            for (int k = 1; k < 8; ++k) s += sh_sum[k * 32 + t];
            sh_sums[t] = s;
        }
        __syncthreads();
        if (t == 0) vg_opt::ctl_step(c, sh_sums);
        __syncthreads();
        if (blockIdx.x == 0) {
            for (int w = t; w < kVgCtlWords; w += 256) reinterpret_cast<uint32_t*>(pa.ctl_next)[w] = sh_ctl[w];
            if (t == 0) {
                VgOut* const out = pa.out;
                if (c->done) {
                    out->x0 = c->x0;
                    out->conv = c->conv; out->outer = c->outer; out->n_lin = c->n_lin; out->n_err = c->n_err; out->passes = c->passes;
                    // (every pass ran in an earlier launch of this stream: the count is final)
                    out->roi_escapes = roi_escapes ? (int32_t)min(*roi_escapes, 0x7fffffffu) : 0;
                    __threadfence_system();
                    __hip_atomic_store(&out->seq, pa.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                } else {
                    __hip_atomic_store(&out->progress, pa.seq * kProgressWindow + (double)c->passes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        }
        if (c->done) return;
    }
    // the pose of this pass and the correspondence buffers, as scalars
    Pose16 T;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const double v = c->xi.m[i];
        T.m[i] = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
    }
    const int kind = __builtin_amdgcn_readfirstlane(c->kind), parity = __builtin_amdgcn_readfirstlane(c->parity);
    const Args a = swapped(a_in, parity);
    const Method m{a};
    __syncthreads();      // (sh_sum is reused by the body)
    if (kind == kVgPassLinearize) lsq_lin_body<false>(m, T, a.n_src, a.partials, sh, sh_sum);
    else lsq_lin_body<true>(m, T, a.n_src, a.partials, sh, sh_sum);
}

}  // namespace pcr
