// index_plan_check -- the rules by which GridIndex::build() decides what to launch (csrc/grid_plan.h: plan_build, commit_build), checked on the CPU:
// cases worked out by hand from the rules as their comments state them, and invariants over a sweep of sizes, capacities and hints.
// No GPU call and no HIP header.  Prints "index_plan_check ok" and returns 0, or says what failed and returns 1.
#include <stdio.h>
#include <stdint.h>
#include <initializer_list>
#include "../csrc/grid_plan.h"

using namespace pcr;

static int g_failed = 0;
static long g_checked = 0;
#define CHECK(cond, ...) do { ++g_checked; if (!(cond)) { if (++g_failed <= 20) { printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static const size_t kLdsPerWorkGroup = 160 * 1024;      // gfx950: 160 KB of LDS per CU, and a work-group may have all of it

// a device pointer as hipMalloc returns them (256-byte aligned); + 4 bytes: a view that starts at the second float
static const float* const kAligned = reinterpret_cast<const float*>((uintptr_t)0x7f0000001000ull);
static const float* const kUnaligned = reinterpret_cast<const float*>((uintptr_t)0x7f0000001004ull);

static BuildRequest request(size_t n, size_t stride = 4, double cell = 1.0) {
    BuildRequest r;
    r.pts = kAligned; r.n = n; r.stride_floats = stride; r.cell = cell;
    return r;
}
// the index after the host has seen a header of `cells` cells: GridIndex::confirm() + note_cells()
static void seen(BuildHints& h, uint64_t cells) { h.hint_ok = h.tiled_shift >= 0; h.note_cells(cells); }

// ---- documented cases ----------------------------------------------------------------------------------------------
static void documented_cases() {
    const TileVariant dense16 = {16, 0, 256, false, true, false}, dense8 = {8, 0, 256, false, true, false};
    // A fresh index: ensure_tables() has made a table of 2^20 cells, no header has been seen (cells_hint = 0), so cap_eff = 2^20.
    // tshift starts at 8 and rises while (2^20 >> tshift) + 2 > 2048: 4098 at 8, 2050 at 9, 1026 at 10 -> tshift = 10, max_bins = 1026.
    // No hint: the box kernel runs, no layout, so bin (by tile) -> place -> tile.  tiles_est = 0: sixteen per thread, nothing is cut (hs = kNoCut),
    // nb_max = max_bins, a block per bin the table can make + block 0 = 1027 blocks, LDS = the 2^10 cell counters of a tile = 4096 bytes.
    for (size_t n : {(size_t)0, (size_t)1, (size_t)30000, (size_t)1000000, (size_t)10000000}) {
        BuildHints h;
        h.cell_capacity = (size_t)1 << 20;
        BuildRequest r = request(n);
        r.allow_hint = true;
        const BuildPlan p = plan_build(h, r);
        CHECK(p.tiled_path && p.tshift == 10 && p.max_bins == 1026, "fresh index, n = %zu: tshift %d max_bins %u", n, p.tshift, p.max_bins);
        CHECK(p.box && !p.reuse_header && !p.preset && !p.use_layout, "fresh index: box %d reuse %d preset %d layout %d", p.box, p.reuse_header, p.preset, p.use_layout);
        CHECK(p.place && !p.keep_pass && p.bin == (BinVariant{true, false, false, false}), "fresh index: place %d", p.place);
        CHECK(p.n_tile == 1 && p.tile[0] == dense16 && p.tile_blocks == 1027 && p.tile_lds[0] == 4096, "fresh index: %d launches, %d blocks, %zu bytes", p.n_tile, p.tile_blocks, p.tile_lds[0]);
        CHECK(p.hs == kNoCut && p.nb_max == 1026 && p.nb_bin == 1026 && p.bin_lds == 1026 * 4, "fresh index: hs %u nb_max %u bin_lds %zu", p.hs, p.nb_max, p.bin_lds);
    }
    // The NDT map: 5 M points, 2.45 M cells of 1 m seen.  tiles_target = min(4096, max(64, 5 M / 512 = 9765)) = 4096; tshift rises from 2 while
    // (2.45 M >> tshift) > 4096: 4785 at 9, 2392 at 10 -> tshift = 10, the comment's "2 390 tiles of 1 024".  2 393 tiles of ~2 090 points: sixteen per thread, no cuts.
    {
        BuildHints h;
        h.cell_capacity = (size_t)1 << 23;
        h.cells_hint = 2450000;
        const BuildPlan p = plan_build(h, request(5000000));
        CHECK(p.tiled_path && p.tshift == 10, "NDT map: tshift %d", p.tshift);
        CHECK(!p.sparse && !p.per8 && p.hs == kNoCut && p.tile[0] == dense16, "NDT map: sparse %d per8 %d", p.sparse, p.per8);
        // cap_eff = min(2^23, 2 x 2.45 M + 64) = 4 900 064 -> max_bins = (4 900 064 >> 10) + 2 = 4 787; blocks: tiles_est + 16 = 2 393 + 16, + block 0
        CHECK(p.max_bins == 4787 && p.tile_blocks == 2393 + 16 + 1, "NDT map: max_bins %u tile_blocks %d", p.max_bins, p.tile_blocks);
    }
    // The voxel filter's cloud: 65 536 points, 2.3 M cells of 0.5 m seen.  tiles_target = max(64, 65 536 / 512) = 128, so tshift rises to its cap:
    // 12 (tiles of 4 096 cells) with cut_sparse, 11 without.  2.3 M > 4 x 65 536 + 65 536: a sparse grid -- light and heavy tiles by a launch each, the
    // first without the planning block; with cut_sparse the heavy tiles are cut at hs = 3 072, and a coherent cloud goes by runs, its heavy bins by 1 024 threads.
    for (int cut = 0; cut < 2; ++cut) {
        BuildHints h;
        h.cell_capacity = (size_t)1 << 23;
        h.cells_hint = 2300000;
        h.cut_sparse = h.coherent_input = cut != 0;
        const BuildPlan p = plan_build(h, request(65536));
        CHECK(p.tiled_path && p.tshift == (cut ? 12 : 11), "voxel filter, cut_sparse %d: tshift %d", cut, p.tshift);
        CHECK(p.sparse && !p.per8 && p.hs == (cut ? 3072u : kNoCut) && p.n_tile == 2, "voxel filter, cut_sparse %d: sparse %d hs %u", cut, p.sparse, p.hs);
        CHECK(p.tile[0] == (TileVariant{1, 1, 256, false, false, cut != 0}) && p.tile[1] == (cut ? TileVariant{4, 2, 1024, false, true, true} : TileVariant{16, 2, 256, false, true, false}), "voxel filter: variants");
        CHECK(p.tile_lds[0] == ((size_t)4 << p.tshift), "voxel filter: the light tiles' launch holds a tile's cell counters only, %zu", p.tile_lds[0]);
    }
    // LOAM's 1 M-point map ("1 464 tiles of ~700 points", shift 11 best at 1 M): 1 464 x 2 048 cells seen.  tiles_target = 1 M / 512 = 1 953;
    // 2 928 tiles at shift 10, 1 464 at 11 -> tshift = 11.  1 M / 1 465 = 682 points per tile <= 1 024: eight per thread, tiles cut at hs = 2 048.
    {
        BuildHints h;
        h.cell_capacity = (size_t)1 << 23;
        h.cells_hint = (uint64_t)1464 << 11;
        const BuildPlan p = plan_build(h, request(1000000));
        CHECK(p.tshift == 11 && p.per8 && p.hs == 2048 && p.cuts_now && p.tile[0] == dense8, "LOAM map: tshift %d per8 %d hs %u", p.tshift, p.per8, p.hs);
        // block 0 plans with cuts: its LDS holds the bins' positions + the tiles' words, (nb_max + 4) x 4 + (max_bins + 8) x 2 > the 8 KB of a tile's cells
        CHECK(p.tile_lds[0] == ((size_t)p.nb_max + 4) * 4 + ((size_t)p.max_bins + 8) * 2, "LOAM map: tile_lds %zu", p.tile_lds[0]);
    }
    // A 10 M-point map on a table that forces tiles of 8 192 cells (20 M cells seen: cap_eff = 40 M, (40 M >> 12) + 2 > kMaxBins, (40 M >> 13) + 2 = 4 884):
    // 2 442 tiles of ~4 095 points, more than ~1 000 on average: sixteen per thread and never cut.
    {
        BuildHints h;
        h.cell_capacity = (size_t)1 << 26;
        h.cells_hint = 20000000;
        const BuildPlan p = plan_build(h, request(10000000));
        CHECK(p.tiled_path && p.tshift == 13 && !p.per8 && p.hs == kNoCut && !p.cuts_now && p.tile[0] == dense16, "10 M map: tshift %d per8 %d hs %u", p.tshift, p.per8, p.hs);
    }
    // The keep pass: a filtered build lists the region's points first from 2 000 000 points on, not below (VGICP's 1 M-point lattice is slower with it).
    for (size_t n : {(size_t)1999999, (size_t)2000000}) {
        BuildHints h;
        h.cell_capacity = (size_t)1 << 23;
        BuildRequest r = request(n);
        r.allow_hint = true;
        commit_build(h, r, plan_build(h, r));
        seen(h, 2450000);
        commit_build(h, r, plan_build(h, r));      // (the cell count seen has changed the tile size: this build makes the layout the next one uses)
        seen(h, 2450000);
        r.mask_callback = r.want_tail = true;
        const BuildPlan first = plan_build(h, r);
        CHECK(first.reuse_header && first.use_layout && first.asks_mask && !first.filtered, "n = %zu: reuse %d layout %d asks %d", n, first.reuse_header, first.use_layout, first.asks_mask);
        r.mask_set = true;
        const BuildPlan p = plan_build(h, r);
        CHECK(p.filtered && p.with_tail && p.keep_pass == (n >= 2000000) && p.bin.packed == p.keep_pass, "n = %zu: filtered %d keep_pass %d", n, p.filtered, p.keep_pass);
        // (2 393 tiles of ~835 points: eight per thread)
        CHECK(p.tile[0] == (TileVariant{8, 0, 256, true, true, false}), "n = %zu: the tile pass lists NDT's cells", n);
    }
    // A twin: a build without hints feeds its twin's header, and the twin's build over the same cloud then launches no box kernel.
    {
        BuildHints a, b;
        a.cell_capacity = b.cell_capacity = (size_t)1 << 20;
        a.has_twin = a.has_mirror = true;
        const BuildPlan pa = plan_build(a, request(65536));
        CHECK(pa.box && pa.feeds_twin && pa.mirrored, "twin: box %d feeds %d mirrored %d", pa.box, pa.feeds_twin, pa.mirrored);
        b.header_preset = true; b.preset_pts = kAligned; b.preset_n = 65536; b.preset_cell = 3.0;
        const BuildPlan pb = plan_build(b, request(65536, 4, 3.0));
        CHECK(pb.preset && !pb.box, "twin's build: preset %d box %d", pb.preset, pb.box);
        const BuildPlan other = plan_build(b, request(65535, 4, 3.0));
        CHECK(!other.preset && other.box, "another cloud: preset %d box %d", other.preset, other.box);
    }
}

// ---- invariants ------------------------------------------------------------------------------------------------------
static void check_plan(const BuildHints& h, const BuildRequest& r, const BuildPlan& p) {
#define WHERE "n %zu cap %zu cells %llu tshift %d", r.n, h.cell_capacity, (unsigned long long)h.cells_hint, p.tshift
    CHECK(p.pt_blocks >= 1, WHERE);
    CHECK(!(h.no_hints && (p.reuse_header || p.use_layout)), WHERE);
    CHECK(p.box == (!p.reuse_header && !p.preset) && !(p.feeds_twin && !p.box), WHERE);
    if (!p.tiled_path) {
        CHECK(p.scan_blocks >= 1 && !p.reuse_header && !p.use_layout && !p.filtered, WHERE);
        return;
    }
    CHECK(p.tshift >= 2 && p.tshift <= kMaxTileShift, WHERE);
    CHECK(p.max_bins >= 1 && p.max_bins <= (uint32_t)kMaxBins && p.nb_max <= (uint32_t)kMaxBins && p.nb_bin <= (uint32_t)kMaxBins && p.nb_max >= p.max_bins, WHERE);
    CHECK(((uint64_t)p.cap_eff >> p.tshift) + 2 == p.max_bins, WHERE);      // every tile the table can make has a bin
    CHECK(p.bin_blocks >= 1 && p.place_blocks >= 1 && p.keep_blocks >= 1 && p.packed_blocks >= 1 && p.tile_blocks >= 1 && p.tile_blocks <= kMaxBins + 1, WHERE);
    CHECK(p.bin_lds <= kLdsPerWorkGroup && p.place_lds <= kLdsPerWorkGroup, WHERE);
    CHECK(p.bin_lds >= (size_t)p.nb_bin * 4 && p.place_lds >= (size_t)p.max_bins * 4, WHERE);
    CHECK(!p.use_layout || p.reuse_header, WHERE);
    CHECK(!p.use_layout || h.lay_nb_max <= p.nb_max, WHERE);      // the layout in hand fits the bin pass's LDS
    CHECK(!p.use_sub || p.use_layout, WHERE);
    CHECK(!p.filtered || (p.use_layout && p.asks_mask && r.mask_set), WHERE);
    CHECK(!p.keep_pass || (p.filtered && r.n >= 2000000), WHERE);
    CHECK(!p.with_tail || (p.filtered && r.want_tail), WHERE);
    CHECK(p.place == !p.use_layout, WHERE);
    CHECK(p.tiled_need == 0 || (p.use_layout && p.tiled_need > r.n + 16), WHERE);
    CHECK(variant_index(p.bin) >= 0, WHERE);
    CHECK(p.bin.place == p.use_layout && p.bin.sub == p.use_sub && p.bin.packed == p.keep_pass && (p.bin.packed || p.bin.vec == p.vec), WHERE);
    CHECK(p.n_tile == 1 || p.n_tile == 2, WHERE);
    int planning = 0;
    for (int i = 0; i < p.n_tile; ++i) {
        CHECK(variant_index(p.tile[i]) >= 0, WHERE);
        CHECK(p.tile_lds[i] <= kLdsPerWorkGroup && p.tile_lds[i] >= ((size_t)4 << p.tshift), WHERE);
        CHECK(p.tile[i].tail == p.with_tail && p.tile[i].runs == (h.coherent_input && !p.with_tail), WHERE);
        planning += p.tile[i].plan;
    }
    CHECK(planning == 1, WHERE);      // one block of every tiled build plans the next layout
#undef WHERE
}

static void sweep() {
    const size_t ns[] = {0, 1, 255, 256, 65536, 1000000, 2000000 - 1, 2000000, 10000000, 0xffffffffull - 16};
    for (size_t n : ns)
    for (int cap_log = 20; cap_log <= 28; ++cap_log) {
        const size_t cap = (size_t)1 << cap_log;
        const uint64_t cells[] = {0, 1, 300, 70000, cap / 64, cap / 8, cap / 2 - 64, cap / 2, cap - 1, cap};
        for (uint64_t c : cells)
        for (int hb = 0; hb < 32; ++hb)
        for (int masked = 0; masked < 2; ++masked) {
            BuildHints h;
            h.cell_capacity = cap;
            h.no_hints = hb & 1; h.coherent_input = hb & 2; h.cut_sparse = hb & 4; h.split_sparse_tiles = !(hb & 8); h.prefer_one_level = hb & 16;
            // three builds in a row, the host seeing `c` cells after each: fresh -> tile size by the cells seen -> header and layout reused
            for (int stage = 0; stage < 3; ++stage) {
                for (int rb = 0; rb < 128; ++rb) {
                    BuildRequest r = request(n, rb & 1 ? 4 : 3);
                    if (rb & 2) r.pts = kUnaligned;
                    r.allow_hint = rb & 4; r.clamp = rb & 8; r.mask_callback = rb & 16; r.want_tail = rb & 32;
                    BuildHints hh = h;
                    hh.has_mirror = hh.has_twin = rb & 64;
                    const BuildPlan first = plan_build(hh, r);
                    check_plan(hh, r, first);
                    r.mask_set = true;
                    const BuildPlan p = plan_build(hh, r);
                    check_plan(hh, r, p);
                    // the filter's answer changes nothing that is on the stream, or reserved, before its callback runs
                    CHECK(p.box == first.box && p.reuse_header == first.reuse_header && p.use_layout == first.use_layout && p.asks_mask == first.asks_mask &&
                          p.tiled_need == first.tiled_need && p.tshift == first.tshift && p.feeds_twin == first.feeds_twin, "n %zu cap %zu cells %llu", n, cap, (unsigned long long)c);
                    CHECK(p.filtered == first.asks_mask, "n %zu cap %zu cells %llu", n, cap, (unsigned long long)c);
                }
                BuildRequest r = request(n);
                r.allow_hint = true; r.mask_callback = r.want_tail = masked; r.mask_set = masked && plan_build(h, r).asks_mask;
                const BuildPlan p = plan_build(h, r);
                commit_build(h, r, p);
                CHECK(!h.hint_ok && !h.header_preset && h.used_hint == p.reuse_header && h.filtered == p.filtered && h.tiled_shift == (p.tiled_path ? p.tshift : -1), "commit");
                CHECK(!p.tiled_path || (h.lay_ok && h.lay_shift == p.tshift && h.lay_nb_max == p.nb_max && h.used_layout == p.use_layout), "commit");
                seen(h, c);
            }
        }
    }
}

int main() {
    documented_cases();
    sweep();
    if (g_failed) { printf("index_plan_check: %d of %ld checks failed\n", g_failed, g_checked); return 1; }
    printf("index_plan_check ok\n");
    return 0;
}
