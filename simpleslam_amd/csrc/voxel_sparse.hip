// voxel_sparse.hip -- pcp::VoxelDownSampleV3 and pcp::VoxelDownSampleV2 on the device (gfx950).
//
// The reference's own voxel filters (common/pcp/pcp.hpp:157-263 and :78-154), written because pcl::VoxelGrid gives up once the voxel box
// exceeds INT_MAX cells: V3 is "simplified pcl" over a hash map keyed by a size_t index, V2 is KISS-ICP's voxel hash.  Both hold the occupied
// voxels only.  Here a voxel is its integer triple, packed relative to the box of the kept rows into one 64-bit key (z most significant, then
// y, then x; an axis of extent e takes bits(e - 1) bits), and the (key, row) pairs go through a stable LSD radix sort:
//   box      min / max of the lattice integers over the finite rows (integer atomics: the result does not depend on their order)
//   key      the key layout from the box, then key and row per input row; a non-finite row is marked and leaves in the first digit pass
//   sort     per 8-bit digit the key's used bits reach: histogram per tile of 2048 rows, scan over [bin][tile], stable scatter
//   runs     voxel starts; V3: segmented double sums by the mark-and-centroid scheme of voxel_filter.hip (per wave of 64 sorted rows the sum
//            in front of its first start, a backward segmented scan inside the wave, the start adds the leads of the waves its run reaches
//            into); V2: one lane per start sums at most max_voxel_pts rows one after the other in float
// Stability is what makes V2's "first max_voxel_pts rows by index" and V3's order of additions functions of the input alone.  Nothing is
// sized by the voxel box.  The box, the key layout, the number of digit passes and the number of kept rows are only known on the device: all
// eight digit passes are queued and the ones the key does not reach leave at once, so that the whole call needs one synchronisation; the last
// launch writes the counts and the verdict into page-locked memory.
#include <limits.h>

#include "pcr_internal.h"

namespace pcr {

static constexpr int kVsTile = 2048;          // rows per block of the box, key and digit passes: 8 rounds of 256
static constexpr int kVsBins = 257;           // 256 digit values + one bin behind them for the dropped rows (first pass only)
static constexpr int kVsScan = 1024;          // threads of the one-block scans
static constexpr int kVsMaxPasses = 8;

struct VsHdr {
    int32_t lo[3], hi[3];          // box of the lattice integers over the kept rows
    uint32_t range_bad;            // a finite row's lattice value left the int range
    uint32_t total;                // voxels emitted
    KeySortCtl sort;               // the sort's digit passes; its kept rows -- the finite ones -- are known after the first
    int32_t refused, bits;
    int32_t shift[3];
    int32_t pad_;
    unsigned long long ext[3];
};
struct VsLead { double x, y, z, w; };

// floor(p * inv) (V3) / trunc(p / gs) (V2) as a float; the caller tests the int range before it casts
__device__ inline float vs_lattice(int kind, float c, float gs, float inv) { return kind == kVsV3 ? floorf(c * inv) : truncf(c / gs); }
__device__ inline bool vs_in_int(float f) { return f >= -2147483648.0f && f < 2147483648.0f; }      // (false for NaN)
__device__ inline bool vs_finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }
__device__ inline int vs_bits(unsigned long long v) { return v ? 64 - __builtin_clzll(v) : 0; }

__global__ __launch_bounds__(64) void vs_init_kernel(VsHdr* __restrict__ hdr) {
    if (threadIdx.x != 0) return;
    VsHdr h;
    for (int a = 0; a < 3; ++a) { h.lo[a] = INT_MAX; h.hi[a] = INT_MIN; h.shift[a] = 0; h.ext[a] = 0; }
    h.range_bad = 0; h.sort.kept = 0; h.total = 0; h.sort.passes = 0; h.refused = 0; h.bits = 0; h.pad_ = 0;
    *hdr = h;
}

__global__ __launch_bounds__(256) void vs_box_kernel(const float* __restrict__ pts, uint32_t sf, uint32_t n, float gs, float inv, int kind,
                                                     VsHdr* __restrict__ hdr) {
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
    bool bad = false;
    const uint32_t base = blockIdx.x * kVsTile;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint32_t j = base + r * 256 + threadIdx.x;
        if (j >= n) continue;
        const float* p = pts + (size_t)j * sf;
        const float c[3] = {p[0], p[1], p[2]};
        if (!vs_finite3(c[0], c[1], c[2])) continue;
        float f[3];
        bool ok = true;
        for (int a = 0; a < 3; ++a) { f[a] = vs_lattice(kind, c[a], gs, inv); ok = ok && vs_in_int(f[a]); }
        if (!ok) { bad = true; continue; }
        for (int a = 0; a < 3; ++a) { const int l = (int)f[a]; lo[a] = min(lo[a], l); hi[a] = max(hi[a], l); }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], __shfl_xor(lo[a], m, 64)); hi[a] = max(hi[a], __shfl_xor(hi[a], m, 64)); }
    const bool any_bad = __any(bad);
    if ((threadIdx.x & 63) == 0) {
        if (lo[0] <= hi[0]) for (int a = 0; a < 3; ++a) { atomicMin(&hdr->lo[a], lo[a]); atomicMax(&hdr->hi[a], hi[a]); }
        if (any_bad) atomicOr(&hdr->range_bad, 1u);
    }
}

// The key layout the box asks for.  V3: extent = (floor(max * inv) - (float)min_b) + 1 with the subtraction in float, as a row's own ijk is
// formed; V2: the exact integer difference.
__device__ inline void vs_layout(VsHdr& h, int kind) {
    h.sort.passes = 0; h.refused = 0; h.bits = 0;
    for (int a = 0; a < 3; ++a) { h.shift[a] = 0; h.ext[a] = 0; }
    if (h.range_bad) { h.refused = kVsRefusedRange; return; }
    if (h.lo[0] > h.hi[0]) { h.sort.passes = 1; return; }      // no finite row: the first pass still runs and counts none kept
    int at = 0;
    for (int a = 0; a < 3; ++a) {
        const unsigned long long span = kind == kVsV3 ? (unsigned long long)((float)h.hi[a] - (float)h.lo[a])
                                                      : (unsigned long long)((long long)h.hi[a] - (long long)h.lo[a]);
        h.ext[a] = span + 1ull;
        h.shift[a] = at;
        at += vs_bits(span);
    }
    h.bits = at;
    if (at > 64) { h.refused = kVsRefusedBits; return; }
    h.sort.passes = at ? (at + 7) / 8 : 1;
}

__global__ __launch_bounds__(256) void vs_key_kernel(const float* __restrict__ pts, uint32_t sf, uint32_t n, float gs, float inv, int kind,
                                                     VsHdr* __restrict__ hdr, unsigned long long* __restrict__ key, uint32_t* __restrict__ row) {
    __shared__ VsHdr sh;
    if (threadIdx.x == 0) {
        VsHdr h = *hdr;
        vs_layout(h, kind);
        sh = h;
        if (blockIdx.x == 0) {      // (every block computes the same from the same box; the later launches read it from here)
            hdr->sort.passes = h.sort.passes; hdr->refused = h.refused; hdr->bits = h.bits;
            for (int a = 0; a < 3; ++a) { hdr->shift[a] = h.shift[a]; hdr->ext[a] = h.ext[a]; }
        }
    }
    __syncthreads();
    if (sh.sort.passes == 0) return;
    const uint32_t base = blockIdx.x * kVsTile;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint32_t j = base + r * 256 + threadIdx.x;
        if (j >= n) continue;
        const float* p = pts + (size_t)j * sf;
        const float c[3] = {p[0], p[1], p[2]};
        unsigned long long k = 0;
        const bool keep = vs_finite3(c[0], c[1], c[2]);
        if (keep) {
            for (int a = 0; a < 3; ++a) {
                const float f = vs_lattice(kind, c[a], gs, inv);
                const unsigned long long rel = kind == kVsV3 ? (unsigned long long)(f - (float)sh.lo[a])
                                                             : (unsigned long long)((long long)(int)f - (long long)sh.lo[a]);
                if (sh.shift[a] < 64) k |= rel << sh.shift[a];      // (a shift of 64: the axes below took every bit and this one has extent 1)
            }
        }
        key[j] = k;
        row[j] = keep ? j : kVsDropped;
    }
}

__device__ inline uint32_t vs_digit(unsigned long long k, uint32_t r, int d) { return (d == 0 && r == kVsDropped) ? 256u : (uint32_t)((k >> (8 * d)) & 255ull); }

// Digit pass d, first launch: per tile of 2048 rows the count of every digit value, to hist[bin][tile].
__global__ __launch_bounds__(256) void vs_hist_kernel(const KeySortCtl* __restrict__ ctl, int d, uint32_t n, const unsigned long long* __restrict__ key,
                                                      const uint32_t* __restrict__ row, uint32_t* __restrict__ hist) {
    __shared__ uint32_t sh[kVsBins];
    if (d >= ctl->passes) return;
    const uint32_t n_cur = d == 0 ? n : ctl->kept;
    const uint32_t tiles = (uint32_t)(((size_t)n_cur + kVsTile - 1) / kVsTile);
    if (blockIdx.x >= tiles) return;
    for (int b = threadIdx.x; b < kVsBins; b += 256) sh[b] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kVsTile;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint32_t j = base + r * 256 + threadIdx.x;
        if (j < n_cur) atomicAdd(&sh[vs_digit(key[j], row[j], d)], 1u);      // (integer counts: the order of the atomics does not show)
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kVsBins; b += 256) hist[(size_t)b * tiles + blockIdx.x] = sh[b];
}

// exclusive scan of a[0 .. m) in place by one block of 1024 threads: a contiguous chunk per thread; returns the total to every thread
__device__ inline uint32_t vs_scan_block(uint32_t* __restrict__ a, size_t m) {
    __shared__ uint32_t sh_wave[kVsScan / 64];
    const size_t chunk = (m + kVsScan - 1) / kVsScan;
    const size_t lo = min((size_t)threadIdx.x * chunk, m), hi = min(lo + chunk, m);
    uint32_t s = 0;
    for (size_t i = lo; i < hi; ++i) s += a[i];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = s;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) { const uint32_t t = __shfl_up(inc, k, 64); if (lane >= k) inc += t; }
    if (lane == 63) sh_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int w = 0; w < kVsScan / 64; ++w) { const uint32_t v = sh_wave[w]; total += v; if (w < wave) before += v; }
    uint32_t run = before + inc - s;
    for (size_t i = lo; i < hi; ++i) { const uint32_t v = a[i]; a[i] = run; run += v; }
    return total;
}

// Digit pass d, second launch: hist[bin][tile] -> where the rows of (bin, tile) go.  The first pass also learns the number of kept rows:
// everything in front of the bin of the dropped ones.
__global__ __launch_bounds__(kVsScan) void vs_scan_hist_kernel(KeySortCtl* __restrict__ ctl, int d, uint32_t n, uint32_t* __restrict__ hist) {
    if (d >= ctl->passes) return;
    const uint32_t n_cur = d == 0 ? n : ctl->kept;
    const uint32_t tiles = (uint32_t)(((size_t)n_cur + kVsTile - 1) / kVsTile);
    (void)vs_scan_block(hist, (size_t)kVsBins * tiles);
    __syncthreads();
    if (d == 0 && threadIdx.x == 0) ctl->kept = tiles ? hist[(size_t)256 * tiles] : 0u;
}

// Digit pass d, third launch: the stable scatter.  A tile's rows go round by round (256 rows each), wave by wave, lane by lane: a row's place is
// the start of its (bin, tile), plus the rows of its digit in earlier rounds, in lower waves of its round and in lower lanes of its wave.
__global__ __launch_bounds__(256) void vs_scatter_kernel(const KeySortCtl* __restrict__ ctl, int d, uint32_t n, const unsigned long long* __restrict__ key,
                                                         const uint32_t* __restrict__ row, const uint32_t* __restrict__ hist,
                                                         unsigned long long* __restrict__ key_out, uint32_t* __restrict__ row_out) {
    __shared__ uint32_t sh_base[kVsBins];
    __shared__ uint32_t sh_cnt[4][kVsBins];
    if (d >= ctl->passes) return;
    const uint32_t n_cur = d == 0 ? n : ctl->kept;
    const uint32_t tiles = (uint32_t)(((size_t)n_cur + kVsTile - 1) / kVsTile);
    if (blockIdx.x >= tiles) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = threadIdx.x; b < kVsBins; b += 256) {
        sh_base[b] = hist[(size_t)b * tiles + blockIdx.x];
        for (int w = 0; w < 4; ++w) sh_cnt[w][b] = 0;
    }
    __syncthreads();
    const uint32_t base = blockIdx.x * kVsTile;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int r = 0; r < 8; ++r) {
        const uint32_t j = base + r * 256 + threadIdx.x;
        const bool valid = j < n_cur;
        unsigned long long k = 0;
        uint32_t rw = 0, dg = 0;
        if (valid) { k = key[j]; rw = row[j]; dg = vs_digit(k, rw, d); }
        unsigned long long same = __ballot(valid);      // the lanes of this wave that hold the same digit
#pragma unroll
        for (int b = 0; b < 9; ++b) { const unsigned long long v = __ballot((dg >> b) & 1u); same &= ((dg >> b) & 1u) ? v : ~v; }
        const uint32_t rank = (uint32_t)__popcll(same & below);
        if (valid && rank == 0) sh_cnt[wave][dg] = (uint32_t)__popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t pos = sh_base[dg] + rank;
            for (int w = 0; w < wave; ++w) pos += sh_cnt[w][dg];
            if (pos < n_cur) { key_out[pos] = k; row_out[pos] = rw; }      // (always, when the histogram is this tile's: the test keeps a wrong one inside the buffer)
        }
        __syncthreads();
        for (int b = threadIdx.x; b < kVsBins; b += 256) {
            uint32_t s = 0;
            for (int w = 0; w < 4; ++w) { s += sh_cnt[w][b]; sh_cnt[w][b] = 0; }
            sh_base[b] += s;
        }
        __syncthreads();
    }
}

// sorted row j starts a voxel: its key differs from its predecessor's
__device__ inline bool vs_is_head(const unsigned long long* __restrict__ key, uint32_t j, bool valid, unsigned long long k) {
    const int lane = threadIdx.x & 63;
    unsigned long long prev = __shfl_up(k, 1, 64);
    if (lane == 0 && valid && j > 0) prev = key[j - 1];
    return valid && (j == 0 || prev != k);
}

__device__ inline void vs_gather(const float* __restrict__ pts, uint32_t sf, int intensity_at, uint32_t r, double& x, double& y, double& z, double& w) {
    const float* p = pts + (size_t)r * sf;
    x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
    w = intensity_at >= 0 ? (double)p[intensity_at] : 0.0;
}

// Run pass, first launch: per wave of 64 sorted rows its first voxel start (64: none -- the rows behind the cloud's end count as one) and, for V3,
// the double sums of the rows in front of it (they belong to a voxel that started in an earlier wave).
__global__ __launch_bounds__(256) void vs_mark_kernel(const VsHdr* __restrict__ hdr, const unsigned long long* __restrict__ key0,
                                                      const unsigned long long* __restrict__ key1, const uint32_t* __restrict__ row0,
                                                      const uint32_t* __restrict__ row1, const float* __restrict__ pts, uint32_t sf, int intensity_at,
                                                      int kind, uint32_t* __restrict__ first, VsLead* __restrict__ lead) {
    const uint32_t kept = hdr->sort.kept;
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if ((j & ~63u) >= kept) return;      // (wave-uniform)
    const unsigned long long* key = (hdr->sort.passes & 1) ? key1 : key0;
    const uint32_t* row = (hdr->sort.passes & 1) ? row1 : row0;
    const int lane = threadIdx.x & 63;
    const bool valid = j < kept;
    const unsigned long long k = valid ? key[j] : 0ull;
    const bool head = vs_is_head(key, j, valid, k);
    const unsigned long long bound = __ballot(head || !valid);
    const int f = bound ? __builtin_ctzll(bound) : 64;
    if (lane == 0) first[j >> 6] = (uint32_t)f;
    if (kind != kVsV3) return;
    double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
    if (lane < f) vs_gather(pts, sf, intensity_at, row[j], sx, sy, sz, sw);      // (in front of the first start: valid by construction)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { sx += __shfl_xor(sx, m, 64); sy += __shfl_xor(sy, m, 64); sz += __shfl_xor(sz, m, 64); sw += __shfl_xor(sw, m, 64); }
    if (lane == 0) { VsLead a; a.x = sx; a.y = sy; a.z = sz; a.w = sw; lead[j >> 6] = a; }
}

// Run pass, second launch: per voxel start the rows of its voxel -- to the next start in its wave, or through the waves behind it -- and whether the
// voxel is emitted (V3: always; V2: min(rows, max_voxel_pts) > min_voxel_pts); per block of 256 sorted rows the voxels emitted.
__global__ __launch_bounds__(256) void vs_count_kernel(const VsHdr* __restrict__ hdr, const unsigned long long* __restrict__ key0,
                                                       const unsigned long long* __restrict__ key1, const uint32_t* __restrict__ first, int kind,
                                                       uint32_t max_pts, uint32_t min_pts, uint32_t* __restrict__ cnt, uint32_t* __restrict__ tile) {
    __shared__ uint32_t sh[4];
    const uint32_t kept = hdr->sort.kept;
    if ((size_t)blockIdx.x * 256 >= kept) return;      // (block-uniform)
    const unsigned long long* key = (hdr->sort.passes & 1) ? key1 : key0;
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = j < kept;
    const unsigned long long k = valid ? key[j] : 0ull;
    const bool head = vs_is_head(key, j, valid, k);
    const unsigned long long bound = __ballot(head || !valid);
    const unsigned long long above = lane == 63 ? 0ull : (bound & ~((2ull << lane) - 1ull));
    const int nxt = above ? __builtin_ctzll(above) : 64;
    uint32_t c = (uint32_t)(nxt - lane);
    if (head && nxt == 64)
        for (size_t w = (size_t)(j >> 6) + 1; w * 64 < kept; ++w) { const uint32_t f = first[w]; c += f; if (f < 64u) break; }
    const bool emit = head && (kind == kVsV3 || min(c, max_pts) > min_pts);
    if (valid) cnt[j] = emit ? c : 0u;
    const unsigned long long em = __ballot(emit);
    if (lane == 0) sh[threadIdx.x >> 6] = (uint32_t)__popcll(em);
    __syncthreads();
    if (threadIdx.x == 0) tile[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(kVsScan) void vs_scan_tile_kernel(VsHdr* __restrict__ hdr, uint32_t* __restrict__ tile) {
    const uint32_t total = vs_scan_block(tile, ((size_t)hdr->sort.kept + 255) / 256);
    if (threadIdx.x == 0) hdr->total = total;
}

// where an emitted voxel goes: the voxels emitted in the blocks before this one, in lower waves of the block and in lower lanes of the wave.
// Block 0 reports the call's counts and verdict.
__device__ inline uint32_t vs_out_pos(const VsHdr* __restrict__ hdr, const uint32_t* __restrict__ tile, bool emit, VsResult* __restrict__ result) {
    __shared__ uint32_t sh[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        VsResult r;
        r.count = hdr->total; r.kept = hdr->sort.kept; r.passes = hdr->sort.passes; r.refused = hdr->refused; r.bits = hdr->bits; r.pad_ = 0;
        for (int a = 0; a < 3; ++a) r.ext[a] = hdr->ext[a];
        *result = r;
    }
    const unsigned long long em = __ballot(emit);
    if (lane == 0) sh[wave] = (uint32_t)__popcll(em);
    __syncthreads();
    uint32_t pos = (uint32_t)__popcll(em & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += sh[w];
    return pos + ((size_t)blockIdx.x * 256 < hdr->sort.kept ? tile[blockIdx.x] : 0u);
}

// Run pass of V3, last launch, a thread per sorted row: the start of a voxel gets the sum of its run -- its wave's part by a backward segmented scan,
// the rest from the leads of the waves the run reaches into -- and writes the centroid of all fields.  The order of the additions is a function of
// the sorted array alone.
__global__ __launch_bounds__(256) void vs_emit_v3_kernel(const VsHdr* __restrict__ hdr, const uint32_t* __restrict__ row0, const uint32_t* __restrict__ row1,
                                                         const float* __restrict__ pts, uint32_t sf, int intensity_at, const uint32_t* __restrict__ cnt,
                                                         const uint32_t* __restrict__ first, const VsLead* __restrict__ lead,
                                                         const uint32_t* __restrict__ tile, float* __restrict__ out, uint32_t out_capacity,
                                                         VsResult* __restrict__ result) {
    const uint32_t kept = hdr->sort.kept;
    const uint32_t* row = (hdr->sort.passes & 1) ? row1 : row0;
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = j < kept;
    const uint32_t c = valid ? cnt[j] : 0u;      // (V3 emits every voxel: the rows with a count are the voxel starts)
    const bool head = c > 0u;
    const uint32_t pos = vs_out_pos(hdr, tile, head, result);
    if ((j & ~63u) >= kept) return;      // (wave-uniform)
    double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
    if (valid) vs_gather(pts, sf, intensity_at, row[j], sx, sy, sz, sw);
    const unsigned long long bound = __ballot(head || !valid);
    const unsigned long long above = lane == 63 ? 0ull : (bound & ~((2ull << lane) - 1ull));
    const int nxt = above ? __builtin_ctzll(above) : 64;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {      // lane l <- sum over [l, min(l + 2 d, nxt))
        const double tx = __shfl_down(sx, d, 64), ty = __shfl_down(sy, d, 64), tz = __shfl_down(sz, d, 64), tw = __shfl_down(sw, d, 64);
        if (lane + d < nxt) { sx += tx; sy += ty; sz += tz; sw += tw; }
    }
    if (!head) return;
    if (nxt == 64)
        for (size_t w = (size_t)(j >> 6) + 1; w * 64 < kept; ++w) {
            const uint32_t f = first[w];
            if (f == 0u) break;
            const VsLead a = lead[w]; sx += a.x; sy += a.y; sz += a.z; sw += a.w;
            if (f < 64u) break;
        }
    if (pos >= out_capacity) return;
    const double inv = 1.0 / (double)c;
    float* o = out + (size_t)pos * sf;
    for (uint32_t q = 0; q < sf; ++q) o[q] = 0.f;
    o[0] = (float)(sx * inv); o[1] = (float)(sy * inv); o[2] = (float)(sz * inv);
    if (sf >= 8) o[3] = 1.0f;      // pcl::PointXYZI keeps data[3] = 1
    if (intensity_at >= 0) o[intensity_at] = (float)(sw * inv);
}

// Run pass of V2, last launch: one lane per emitted voxel.  Its first min(rows, max_voxel_pts) sorted rows are the rows of lowest index (the sort is
// stable); p.setZero(), p += each in turn, p /= (float)count (pcp.hpp:139-143), into a copy of the first row's bytes.
__global__ __launch_bounds__(256) void vs_emit_v2_kernel(const VsHdr* __restrict__ hdr, const uint32_t* __restrict__ row0, const uint32_t* __restrict__ row1,
                                                         const float* __restrict__ pts, uint32_t sf, uint32_t max_pts, const uint32_t* __restrict__ cnt,
                                                         const uint32_t* __restrict__ tile, float* __restrict__ out, uint32_t out_capacity,
                                                         VsResult* __restrict__ result) {
    const uint32_t kept = hdr->sort.kept;
    const uint32_t* row = (hdr->sort.passes & 1) ? row1 : row0;
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    const uint32_t c = j < kept ? cnt[j] : 0u;
    const uint32_t pos = vs_out_pos(hdr, tile, c > 0u, result);
    if (c == 0u || pos >= out_capacity) return;
    const uint32_t m = min(c, max_pts);
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (uint32_t i = 0; i < m; ++i) { const float* p = pts + (size_t)row[j + i] * sf; sx += p[0]; sy += p[1]; sz += p[2]; }
    const float fm = (float)m;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(pts + (size_t)row[j] * sf);
    uint32_t* o = reinterpret_cast<uint32_t*>(out + (size_t)pos * sf);
    for (uint32_t q = 3; q < sf; ++q) o[q] = src[q];
    o[0] = __float_as_uint(sx / fm); o[1] = __float_as_uint(sy / fm); o[2] = __float_as_uint(sz / fm);
}

// The stable sort of n (key, row) pairs on its own, for every user of it (the voxel filters here, the sparse target index of sparse_index.hip).
// In: the pairs in key[0] / row[0], rows marked kVsDropped leave in the first pass; ctl->passes = the digit passes the keys' used bits reach, set on
// the device by the launch in front (0: nothing runs).  All eight passes are queued and those beyond ctl->passes leave at once.  Out: the
// sorted pairs in key[ctl->passes & 1] / row[ctl->passes & 1], ctl->kept = their number.
size_t key_sort_hist_bytes(size_t n) { return (size_t)kVsBins * (n / kVsTile + 1) * sizeof(uint32_t); }
void key_sort_launch(KeySortCtl* d_ctl, size_t n, unsigned long long* const key[2], uint32_t* const row[2], uint32_t* hist, hipStream_t s) {
    const uint32_t n32 = (uint32_t)n;
    const int tiles = (int)((n + kVsTile - 1) / kVsTile ? (n + kVsTile - 1) / kVsTile : 1);
    for (int d = 0; d < kVsMaxPasses; ++d) {
        const int from = d & 1, to = from ^ 1;
        hipLaunchKernelGGL(vs_hist_kernel, dim3(tiles), dim3(256), 0, s, d_ctl, d, n32, key[from], row[from], hist);
        hipLaunchKernelGGL(vs_scan_hist_kernel, dim3(1), dim3(kVsScan), 0, s, d_ctl, d, n32, hist);
        hipLaunchKernelGGL(vs_scatter_kernel, dim3(tiles), dim3(256), 0, s, d_ctl, d, n32, key[from], row[from], hist, key[to], row[to]);
    }
}

VsSizes voxel_sparse_bytes(size_t n) {
    VsSizes s;
    s.hdr = 256;
    s.key = (n + 1) * sizeof(unsigned long long);
    s.row = (n + 1) * sizeof(uint32_t);
    s.hist = key_sort_hist_bytes(n);
    s.cnt = (n + 1) * sizeof(uint32_t);
    s.first = (n / 64 + 1) * sizeof(uint32_t);
    s.lead = (n / 64 + 1) * sizeof(VsLead);
    s.tile = (n / 256 + 1) * sizeof(uint32_t);
    return s;
}

hipError_t voxel_sparse_launch(const VsBuffers& b, const float* d_pts, size_t stride_floats, size_t n, float leaf, int kind, int max_voxel_pts,
                               int min_voxel_pts, float* d_out, size_t out_capacity, VsResult* result_mapped, hipStream_t s) {
    static_assert(sizeof(VsHdr) <= 256, "the header's buffer");
    const uint32_t n32 = (uint32_t)n, sf = (uint32_t)stride_floats;
    const float inv = 1.0f / leaf;
    const int tiles = (int)((n + kVsTile - 1) / kVsTile ? (n + kVsTile - 1) / kVsTile : 1);
    const int blocks = (int)((n + 255) / 256 ? (n + 255) / 256 : 1);
    const int intensity_at = stride_floats >= 8 ? 4 : (stride_floats >= 4 ? 3 : -1);
    const uint32_t cap = (uint32_t)std::min<size_t>(out_capacity, 0xffffffffu);
    VsHdr* hdr = static_cast<VsHdr*>(b.hdr);
    hipLaunchKernelGGL(vs_init_kernel, dim3(1), dim3(64), 0, s, hdr);
    hipLaunchKernelGGL(vs_box_kernel, dim3(tiles), dim3(256), 0, s, d_pts, sf, n32, leaf, inv, kind, hdr);
    hipLaunchKernelGGL(vs_key_kernel, dim3(tiles), dim3(256), 0, s, d_pts, sf, n32, leaf, inv, kind, hdr, b.key[0], b.row[0]);
    key_sort_launch(&hdr->sort, n, b.key, b.row, b.hist, s);
    hipLaunchKernelGGL(vs_mark_kernel, dim3(blocks), dim3(256), 0, s, hdr, b.key[0], b.key[1], b.row[0], b.row[1], d_pts, sf, intensity_at, kind, b.first,
                       static_cast<VsLead*>(b.lead));
    hipLaunchKernelGGL(vs_count_kernel, dim3(blocks), dim3(256), 0, s, hdr, b.key[0], b.key[1], b.first, kind, (uint32_t)max_voxel_pts,
                       (uint32_t)min_voxel_pts, b.cnt, b.tile);
    hipLaunchKernelGGL(vs_scan_tile_kernel, dim3(1), dim3(kVsScan), 0, s, hdr, b.tile);
    if (kind == kVsV3)
        hipLaunchKernelGGL(vs_emit_v3_kernel, dim3(blocks), dim3(256), 0, s, hdr, b.row[0], b.row[1], d_pts, sf, intensity_at, b.cnt, b.first,
                           static_cast<const VsLead*>(b.lead), b.tile, d_out, cap, result_mapped);
    else
        hipLaunchKernelGGL(vs_emit_v2_kernel, dim3(blocks), dim3(256), 0, s, hdr, b.row[0], b.row[1], d_pts, sf, (uint32_t)max_voxel_pts, b.cnt, b.tile,
                           d_out, cap, result_mapped);
    return hipGetLastError();
}

}  // namespace pcr
