// grid_plan.h -- what a build of the grid index (grid_index.hip: GridIndex::build) will do, decided on the host before anything is queued.
// Host-only and free of HIP types: plan_build() is a pure function of the index's hints and of the call, so the rules below -- measured facts,
// each with its record in a comment -- run, print and are tested without a GPU (host/index_plan_check.cpp, tests/test_index_plan_host.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

namespace pcr {

static constexpr int kBBoxBlocks = 256;  // partial bounding boxes
static constexpr int kMaxBins = 8192;    // tiles of the tiled build path (grid_index.hip): one 32 KB LDS histogram
static constexpr int kMaxTileShift = 13; // a tile's cells are histogrammed in LDS too
static constexpr int kScanPerThread = 8;
static constexpr int kScanBlock = 256;
static constexpr int kScanTile = kScanPerThread * kScanBlock;  // 2048 cells per block
static constexpr int kBinPerThread = 8;               // points per thread and chunk of the bin kernel
static constexpr uint32_t kNoCut = 0xffffffffu;       // BuildPlan::hs of a build whose layout cuts no tile

// What a build leaves for the next one of the same index, and what the owner of the index sets once: everything the decisions read.
// GridIndex derives from it (pcr_internal.h), so `grid.cut_sparse`, `grid.hint_margin` and the like are these fields.
struct BuildHints {
    int tiled_shift = -1;                       // log2(cells per tile) of the last build when it took the tiled path
    // Bounding-box hint: a build whose header the host has seen to be good (confirm()) lets the NEXT build of the same kind skip
    // the bounding-box pass and reuse that header -- a sub-map changes by a key frame at a time.  The bin kernel checks every
    // point against the box; one outside sets header.stale and the caller rebuilds with a fresh (and from then on padded) box.
    bool hint_ok = false;
    double hint_cell = 0.0, hint_shift = 0.0;
    int hint_pcl = 0;                           // lattice kind of the build the hint comes from (a hint serves only a build of the same kind)
    int hint_margin = 0;                        // cells added around a fresh box in x and y (0 until a hint has failed once)
    int hint_margin_z_pcl = 0;                  // ... and in z, for a pcl::VoxelGrid lattice (the voxel filter; the other lattices: see grid_bbox_header_kernel)
    bool used_hint = false;                     // the last build() reused the header
    bool no_hints = false;                      // pcr_params.index_no_hints: never reuse a header or a tile layout
    bool coherent_input = false;                // the clouds are stored in a spatially coherent order (scans, ring by ring): the tile pass counts by runs of equal cells (grid_tile_kernel: kRuns)
    bool cut_sparse = false;                    // sparse grids too have their heavy tiles cut into slabs by the layout hint (grid_index.hip: BINS); the voxel filter's index
    bool split_sparse_tiles = true;             // sparse grids: light and heavy tiles by an instantiation of the tile kernel each (grid_index.hip)
    bool prefer_one_level = false;              // build by the one-level path (histogram with ranks -> scan -> scatter): a small cloud on a COARSE grid puts
                                                // a third of its points into one tile, which one block of the tiled path then sorts alone
    // Layout hint: where each BIN's points may go in `tiled` (an eighth more room than the bin held + 32) and which bins the tiles are cut into
    // (grid_index.hip: BINS), planned by one block of every tiled build's tile pass for the next one; two buffers, alternating.  Used only
    // together with a reused header.
    int lay_idx = 0, lay_shift = -1;
    uint32_t lay_nb_max = 0;                    // bins the layout in hand was planned for (the next build must have room for as many)
    bool lay_cuts = false;                      // ... and it may hold tiles that are cut (the bin pass then reads the tiles' words)
    size_t lay_n = 0;
    uint32_t lay_room_add = 32;                 // ... + lay_room_add
    int lay_room_shift = 3;                     // a bin's room in the layout: what it held + that >> lay_room_shift + 32 (the voxel filter's clouds change more from call to call: 1)
    bool lay_ok = false, used_layout = false;
    bool filtered = false;                      // the last build() indexed the points of a region only (BuildFilter)
    // A build WITHOUT hints computes the bounding box itself; then (grid_bbox_header_kernel) the header is also written to the index's host-mapped
    // mirror, if it has one (`mirrored` says so), and the index's twin, if it has one, gets its header from the same pass: header_preset, and for
    // which cloud and cell.  build() notes before it plans whether the two exist (GridIndex::header_mirror, GridIndex::twin).
    bool has_mirror = false, has_twin = false;
    bool mirrored = false;
    bool header_preset = false;
    const float* preset_pts = nullptr; size_t preset_n = 0; double preset_cell = 0.0;
    size_t cell_capacity = 0;   // entries available in cell_count / cell_start
    uint64_t cells_hint = 0;    // cells of the last header of this index the host has seen (0: none): bounds the next build's cell count and sets its tile size
    void note_cells(uint64_t n_cells) { if (n_cells) cells_hint = n_cells; }
    // The cell count a build may use: the table's capacity, or -- once a header of this index has been seen (note_cells) -- twice that
    // header's count.  The tile size follows from it, and a grid of a few hundred cells (the coarse levels of the covariance search)
    // must not be cut into 256-cell tiles: two blocks then sorted a whole scan between them (158 us).  A cloud that needs more cells
    // than the bound raises header.overflow like a table that is too small, and grow_cells() lifts the bound.
    size_t effective_capacity() const {
        size_t cap_eff = cell_capacity;
        if (cells_hint) cap_eff = std::min<size_t>(cell_capacity, std::max<size_t>(2 * (size_t)cells_hint + 64, 1024));
        return cap_eff;
    }
};

// What build() is called with, as far as the decisions need it.
struct BuildRequest {
    const float* pts = nullptr;         // compared (a preset header is for one cloud) and tested for 16-byte alignment, never read
    size_t n = 0, stride_floats = 0;
    double cell = 0.0, shift = 0.0;
    int pcl_mode = 0;
    bool clamp = false;                 // a ClampBox is in use
    bool allow_hint = false;
    bool mask_callback = false;         // a BuildFilter with enqueue_mask was passed
    bool want_tail = false;             // ... and it wants the tile pass to list NDT's voxel cells (BuildFilter::want_tail)
    bool mask_set = false;              // the callback has been called and left a mask: known only after a first plan said BuildPlan::asks_mask
};

// The instantiations of the two templated passes that a build may launch: the launchers of grid_index.hip instantiate these and no others.
struct TileVariant { int per, mode, threads; bool tail, plan, runs; };      // grid_tile_kernel<kTilePer, kMode, kThreads, kTail, kPlan, kRuns>
struct BinVariant { bool vec, place, sub, packed; };                        // grid_bin_kernel<kVec, kBinPerThread, kPlace, kSub, kPacked>
constexpr bool operator==(const TileVariant& a, const TileVariant& b) { return a.per == b.per && a.mode == b.mode && a.threads == b.threads && a.tail == b.tail && a.plan == b.plan && a.runs == b.runs; }
constexpr bool operator==(const BinVariant& a, const BinVariant& b) { return a.vec == b.vec && a.place == b.place && a.sub == b.sub && a.packed == b.packed; }
static constexpr int kTileVariants = 10, kBinVariants = 8;
static constexpr TileVariant kTileVariant[kTileVariants] = {
    {1, 1, 256, false, false, true},  {4, 2, 1024, false, true, true},      // sparse grids of coherent clouds: light tiles, heavy tiles
    {8, 0, 256, false, true, true},   {16, 0, 256, false, true, true},      // dense grids of coherent clouds
    {1, 1, 256, false, false, false}, {16, 2, 256, false, true, false},     // sparse grids: light tiles, heavy tiles
    {8, 0, 256, true, true, false},   {16, 0, 256, true, true, false},      // dense grids, with NDT's tail
    {8, 0, 256, false, true, false},  {16, 0, 256, false, true, false},     // dense grids
};
static constexpr BinVariant kBinVariant[kBinVariants] = {
    {true, true, true, true},    {true, true, false, true},         // from the list the keep pass left, placed by a layout with / without tiles that are cut
    {true, true, true, false},   {false, true, true, false},        // placed by a layout that may hold tiles that are cut
    {true, true, false, false},  {false, true, false, false},       // placed by the layout in hand
    {true, false, false, false}, {false, false, false, false},      // by tile; the place pass follows
};
constexpr int variant_index(const TileVariant& v) { for (int i = 0; i < kTileVariants; ++i) if (kTileVariant[i] == v) return i; return -1; }
constexpr int variant_index(const BinVariant& v) { for (int i = 0; i < kBinVariants; ++i) if (kBinVariant[i] == v) return i; return -1; }

struct BuildPlan {
    size_t cap_eff = 0;                 // cells the header may describe (BuildHints::effective_capacity)
    bool tiled_path = false;            // else the one-level path: count -> scan (two launches) -> scatter
    bool reuse_header = false, preset = false;      // the header is the previous build's / was written by the twin's build
    bool box = false;                   // the box kernel runs ...
    bool feeds_twin = false;            // ... and writes the twin's header too
    bool mirrored = false;              // the header this build uses is also in the host-mapped mirror
    int box_margin = 0, box_margin_z_pcl = 0;
    int tshift = 0;
    int pt_blocks = 1, scan_blocks = 1; // one-level path (pt_blocks: count and scatter)
    // tiled path
    uint32_t max_bins = 0, nb_bin = 0, nb_max = 0, hs = kNoCut;
    bool vec = false, sparse = false, per8 = false;
    bool use_layout = false, use_sub = false, cuts_now = false;
    bool asks_mask = false;             // the filter's mask callback is to be called (then plan again with BuildRequest::mask_set)
    bool filtered = false, keep_pass = false, with_tail = false;
    int bin_blocks = 1, place_blocks = 1, keep_blocks = 1, packed_blocks = 1, tile_blocks = 1;
    size_t bin_lds = 0, place_lds = 0;
    size_t tiled_need = 0;              // float4s `tiled` must hold for the layout's rooms (0: the cloud's own size serves)
    BinVariant bin = {};
    bool place = false;                 // the place pass follows the bin pass
    int n_tile = 0;                     // launches of the tile pass
    TileVariant tile[2] = {};
    size_t tile_lds[2] = {0, 0};
};

inline BuildPlan plan_build(const BuildHints& h, const BuildRequest& r) {
    BuildPlan p;
    const size_t n = r.n;
    p.pt_blocks = (int)std::min<size_t>(2048, (n + 255) / 256 ? (n + 255) / 256 : 1);
    const size_t cap_eff = p.cap_eff = h.effective_capacity();
    // tile size: ~512 points per tile on average, at most 4096 tiles, at least 4 cells per tile (16-byte accesses of the tile kernel)
    // (the bound was 2048: the 5 M-point map of the NDT configuration -- 2.45 M cells of 1 m -- then got 1 195 tiles of 2 048 cells; with 2 390 tiles
    //  of 1 024 a call takes 0.321 instead of 0.337 ms, with 4 780 of 512 0.361, A/B on one box; clouds of up to 1 M points are not affected)
    const size_t tiles_target = std::min<size_t>(4096, std::max<size_t>(64, n / 512));
    // (never more than 2^11 cells per tile unless the counter array forces it: a tile's block zeroes, scans and writes every cell of it,
    //  and a sparse fine grid -- 3.6 M cells for a 65 k-point scan -- is better served by many small tiles than by 440 blocks of 8 192 cells)
    int tshift;
    // (the voxel filter's grids -- 65 536 points over 2.3 M cells of 0.5 m -- take tiles of 4 096 cells: half the bins for the bin pass's last block to read back,
    //  7 % off a scan's filter; 8 192 cells: slower again.  Round 5, scripts/seq_breakdown.py, two rounds on one box.)
    const int tshift_cap = h.cut_sparse ? 12 : 11;
    if (h.cells_hint) { tshift = 2; while ((h.cells_hint >> tshift) > tiles_target && tshift < tshift_cap) ++tshift; }
    else { tshift = 8; while (((uint64_t)cap_eff >> tshift) + 2 > 2048 && tshift < 11) ++tshift; }
    while (((uint64_t)cap_eff >> tshift) + 2 > (uint64_t)kMaxBins) ++tshift;
    p.tshift = tshift;
    const bool tiled_path = p.tiled_path = tshift <= kMaxTileShift && !h.prefer_one_level;
    const bool reuse_header = p.reuse_header = r.allow_hint && !h.no_hints && h.hint_ok && tiled_path && h.hint_pcl == r.pcl_mode && h.hint_shift == r.shift && !r.clamp && h.hint_cell == r.cell && h.tiled_shift == tshift;
    // (a header written by the twin's build -- see BuildHints -- serves if it was made for this very cloud and cell)
    p.preset = h.header_preset && h.preset_pts == r.pts && h.preset_n == n && h.preset_cell == r.cell && !reuse_header && !r.clamp && r.pcl_mode == 0 && r.shift == 0.0;
    p.box = !reuse_header && !p.preset;
    p.feeds_twin = p.box && h.has_twin && !r.clamp && r.pcl_mode == 0 && r.shift == 0.0 && !r.allow_hint;
    p.mirrored = !reuse_header && h.has_mirror;
    p.box_margin = (r.allow_hint && !r.clamp) ? h.hint_margin : 0;
    p.box_margin_z_pcl = (r.allow_hint && !r.clamp) ? h.hint_margin_z_pcl : 0;
    if (!tiled_path) {
        p.scan_blocks = (int)((h.cell_capacity + kScanTile - 1) / kScanTile);
        return p;
    }
    // Tile size from the CAPACITY of the cell table (the device-side cell count never exceeds it: a larger box is an overflow):
    // ~2048 tiles when the table allows it -- 8 KB of LDS counters per block in the bin kernel, tiles of a few hundred to a few
    // thousand points -- never more than kMaxBins.
    const uint32_t max_bins = p.max_bins = (uint32_t)(((uint64_t)cap_eff >> tshift) + 2);      // tiles the (bounded) cell table can make
    const bool vec = p.vec = (r.stride_floats % 4 == 0) && ((uintptr_t)r.pts % 16 == 0);
    const size_t bin_chunk = (size_t)256 * kBinPerThread;
    p.bin_blocks = (int)std::min<size_t>(4096, (n + bin_chunk - 1) / bin_chunk ? (n + bin_chunk - 1) / bin_chunk : 1);
    p.place_blocks = (int)std::min<size_t>(2048, (n + 1023) / 1024 ? (n + 1023) / 1024 : 1);
    // (a grid with many more cells than points: light tiles and heavy tiles by an instantiation each, see grid_tile_kernel)
    const bool sparse = p.sparse = h.split_sparse_tiles && h.cells_hint > 4 * (uint64_t)n + 65536;
    const uint64_t tiles_est = h.cells_hint ? (h.cells_hint >> tshift) + 1 : 0;
    // dense grids: eight points per thread (135 VGPRs, three waves per SIMD) while a tile holds ~1 000 points or fewer on average, sixteen
    // beyond (A/B: 1 M points in 1 464 tiles 48.4 -> 46.8 us with eight; 5 M and 10 M points are faster with sixteen)
    const bool per8 = p.per8 = !sparse && tiles_est && n / tiles_est <= 1024;
    // BINS (see the top of the tiled path): a tile whose fullest slab holds more than `hs` points is cut one step further in the layout this build
    // leaves -- three quarters of what a block of the tile pass holds in registers -- while the bins stay within nb_max.  pcr_params.index_no_hints:
    // no layout is ever used, so nothing is cut.
    // Measured (round 5, A/B on one box, profiles/r05_notes.md): at 1 M points hs = 2 048 or 3 072 takes the tile pass from 26.0 to 18.6 us and costs the bin pass
    // 1.5 us (more bins: more claims); 1 024 costs it 4 us.  At 10 M points (tiles of 8 192 cells, sixteen points per thread) cutting does NOT pay: the bin
    // pass's stores scatter over twice the bins (151 -> 186-235 us) and the tile pass, whose length there is blocks x latency / occupancy and not its heaviest
    // block, stays at 153-169 us: clouds whose tiles hold more than ~1 000 points on average are never cut.
    // (cut_sparse -- the voxel filter's index: a concatenation of raw key frames on the 0.5 m lattice is a sparse grid whose few tiles next to the vehicle's
    //  path hold tens of thousands of points each; one block sorted such a tile alone, 95 us of a 150 us build.  Its bins hold up to 4 096 points in registers.)
    const uint32_t hs = p.hs = per8 ? 2048u : (sparse && h.cut_sparse ? 3072u : kNoCut);
    // bins a layout may hold: the tiles + two bins per `hs` points (a slab that was cut holds between hs / 2 and hs), never fewer than the tiles the table
    // can make, and never fewer than the layout in hand was planned for (the bin pass sizes its LDS by it)
    uint32_t nb_max = (uint32_t)std::min<uint64_t>((uint64_t)kMaxBins, std::max<uint64_t>((uint64_t)max_bins, (tiles_est ? tiles_est + 2 : (uint64_t)max_bins) + (hs != kNoCut ? 2 * (uint64_t)n / hs : 0)));
    if (hs == kNoCut && !(h.lay_ok && h.lay_cuts)) nb_max = max_bins;
    if (h.lay_ok && h.lay_shift == tshift) nb_max = std::max(nb_max, h.lay_nb_max);
    p.nb_max = nb_max;
    // Layout hint (see grid_bin_kernel<.., kPlace>): the previous build of this index left, next to its header, where each bin's
    // points may go; a build that reuses the header places by it and skips the placing pass.
    const bool use_layout = p.use_layout = reuse_header && h.lay_ok && h.lay_shift == tshift && h.lay_nb_max <= nb_max;
    if (use_layout) {      // room for every bin's slack, the children of a tile that is cut one step further get their parent's room each:
                           // at most twice the cloud's (the device also checks every store against the capacity it is told)
        const size_t need = 2 * (h.lay_n + (h.lay_n >> h.lay_room_shift)) + (size_t)h.lay_room_add * (nb_max + 1) + 16;
        if (need > n + 16) p.tiled_need = need;
    }
    // the lattice is the reused header's, the rooms are the full cloud's: this build may leave points out
    p.asks_mask = r.mask_callback && use_layout;
    const bool filtered = p.filtered = p.asks_mask && r.mask_set;
    const bool cuts_now = p.cuts_now = hs != kNoCut;               // the layout this build plans may cut tiles
    const bool use_sub = p.use_sub = use_layout && h.lay_cuts;     // the layout in hand may hold tiles that are cut
    const bool plan_lds = cuts_now || use_sub;                     // block 0 of the tile pass plans with cuts (or merges some back): it keeps the bins' positions + the tiles' words in LDS
    // (sizing the bin pass's LDS by the tiles the reused header HAS instead of the tiles the table could make -- four blocks per CU instead of three at
    //  10 M points -- changed nothing: 300 / 306 us against 298 / 310, round 5.  At 10 M points the two passes move ~750 MB in 300 us: 2.5 TB/s of real traffic)
    const uint32_t nb_bin = p.nb_bin = use_layout ? nb_max : max_bins;      // bins the bin pass counts in LDS
    p.bin_lds = (size_t)nb_bin * 4 + (use_layout ? ((size_t)nb_bin + 4) * 4 : 0) + (use_sub ? ((size_t)max_bins + 8) * 2 : 0);
    p.place_lds = ((size_t)max_bins + 4) * 4;
    const size_t cells_lds = (size_t)(1u << tshift) * 4;           // a tile's cell counters
    const size_t tile_lds = std::max<size_t>(cells_lds, plan_lds ? ((size_t)nb_max + 4) * 4 + ((size_t)max_bins + 8) * 2 : 0);
    // region-only builds of large clouds: the region's points are listed first, the bin pass reads the list (grid_keep_kernel; smaller clouds: the bin
    // pass tests the mask itself)
    const bool keep_pass = p.keep_pass = filtered && n >= 2000000;      // (a 1 M-point lattice build -- VGICP's -- is 1.5 % SLOWER with the extra launch)
    if (keep_pass) {
        p.keep_blocks = (int)std::min<size_t>(1024, (n + 2047) / 2048);
        p.packed_blocks = std::min(p.bin_blocks, 512);      // (a block takes chunk after chunk: the list's length is the device's to know)
    }
    p.bin = keep_pass ? BinVariant{true, true, use_sub, true} : BinVariant{vec, use_layout, use_sub, false};
    p.place = !use_layout;
    // the tile pass: a block per bin, + block 0 (persistent blocks -- 6 / 4 / 2 per CU by their registers -- measured no better at 1 M points and
    // 6 % worse at 10 M, round 5)
    // (a block per bin the host EXPECTS -- the tiles of the header it has seen + a bin per hs points when tiles are cut -- not per bin the table could
    //  make: a block that finds no bin still waits for the header, ~2 us of a slot each, and there were 3 000 of them at 10 M points; a block takes
    //  bin after bin, so more bins than blocks are served all the same)
    const uint32_t bins_bound = use_layout ? nb_max : max_bins;
    const uint32_t bins_expected = tiles_est ? (uint32_t)std::min<uint64_t>(bins_bound, tiles_est + 16 + (use_layout && hs != kNoCut ? (uint64_t)n / hs : 0)) : bins_bound;
    p.tile_blocks = (int)bins_expected + 1;
    // (measured and not kept: blocks of 1 024 threads for the 5 M and 10 M-point maps cut the slowest tile of the 10 M-point map from 165 to 69 us
    //  and left the kernel at 165 us: one block per CU then, 19 rounds of ~8 us; profiles/r04_notes.md)
    // (the tile pass lists NDT's voxel cells beside its own work: dense grids, tiles of at most 2^13 cells -- 32 per thread)
    const bool with_tail = p.with_tail = filtered && r.want_tail && !sparse && tshift <= 13;
    // (sparse grids: the launch of the light tiles carries no planning block -- its 58 registers are what lets eight of its blocks share a CU)
    // (the heavy bins of the voxel filter's clouds by blocks of 1 024 threads: what a block holds in registers is the same 4 096 points, a bin of 12 000 --
    //  three chunks, two sweeps each -- is through four times sooner)
    const int per = per8 ? 8 : 16;
    if (h.coherent_input && sparse) { p.n_tile = 2; p.tile[0] = {1, 1, 256, false, false, true}; p.tile[1] = {4, 2, 1024, false, true, true}; }
    else if (h.coherent_input && !with_tail) { p.n_tile = 1; p.tile[0] = {per, 0, 256, false, true, true}; }
    else if (sparse) { p.n_tile = 2; p.tile[0] = {1, 1, 256, false, false, false}; p.tile[1] = {16, 2, 256, false, true, false}; }
    else { p.n_tile = 1; p.tile[0] = {per, 0, 256, with_tail, true, false}; }
    // (only a launch with the planning block needs more LDS than the tile's cell counters)
    for (int i = 0; i < p.n_tile; ++i) p.tile_lds[i] = p.tile[i].plan ? tile_lds : cells_lds;
    return p;
}

// The hints as they stand after the build that `p` describes has been queued.
inline void commit_build(BuildHints& h, const BuildRequest& r, const BuildPlan& p) {
    h.hint_ok = false;      // until the host has seen this build's header (confirm())
    h.used_hint = p.reuse_header;
    h.hint_cell = r.cell; h.hint_shift = r.shift; h.hint_pcl = r.pcl_mode;
    h.header_preset = false;
    h.mirrored = p.mirrored;
    h.filtered = p.filtered;
    if (!p.tiled_path) { h.tiled_shift = -1; return; }
    h.tiled_shift = p.tshift;
    h.used_layout = p.use_layout;
    h.lay_nb_max = p.nb_max; h.lay_cuts = p.cuts_now || p.use_sub;
    h.lay_idx ^= 1; h.lay_ok = true; h.lay_shift = p.tshift;      // (what this build's last block wrote serves the next one)
    if (!p.filtered) h.lay_n = r.n;
}

}  // namespace pcr
