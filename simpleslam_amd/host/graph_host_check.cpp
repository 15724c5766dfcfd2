// graph_host_check -- the pose graph's host side that touches no device, on the CPU: csrc/graph_store.h (checks, pack, union-find, g2o) and
// csrc/graph_opt.h (the Levenberg-Marquardt controller).  No GPU call, no HIP header, no library.  Built with -fsanitize=address,undefined it is
// the checked run of the parser and of pack's index arithmetic.
//
// usage: graph_host_check                 the built-in worked cases; exit status 1 on a mismatch
//        graph_host_check steps.txt ...   scripted controller runs, one printed line per step.  A file holds cases, each
//            "case NAME max_iterations rel_tol abs_tol lambda_init lambda_factor lambda_max chi2_initial", then lines "step chi2_new pcg_it pcg_flag";
//            numbers as strtod reads them (hex floats, nan, inf).  Steps after the controller stopped are counted, not taken.
#include <stdlib.h>
#include <unistd.h>

#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../csrc/graph_opt.h"
#include "../csrc/graph_store.h"

using namespace pcr::graph;
using namespace pcr::graph_opt;

static int g_bad = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { fprintf(stderr, "graph_host_check: FAILED: %s\n", what); ++g_bad; }
}
static void expect_msg(const std::string& got, const std::string& want) {
    if (got != want) { fprintf(stderr, "graph_host_check: FAILED: message\n  got:  %s\n  want: %s\n", got.c_str(), want.c_str()); ++g_bad; }
}

static const double kEye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// factor number `tag`: z[k] = 100 tag + k, the information's upper triangle 1000 tag + 0 .. 20
static void add_tagged(Store& s, long long from, size_t to, int tag) {
    double z[16], i21[21];
    for (int k = 0; k < 16; ++k) z[k] = 100.0 * tag + k;
    for (int k = 0; k < 21; ++k) i21[k] = 1000.0 * tag + k;
    expect(add_factor(s, "t", from, to, z, i21).empty(), "add_factor");
}

static void add_eye_poses(Store& s, size_t n) {
    for (size_t i = 0; i < n; ++i) expect(add_poses(s, "t", kEye, 1).empty(), "add_poses");
}

static void check_pack() {
    {   // 3 poses, a prior on pose 1 (factor 0), betweens (0,1), (2,1), (0,2) (factors 1, 2, 3), the last switched off: it keeps its CSR entries
        Store s;
        add_eye_poses(s, 3);
        add_tagged(s, 0, 1, 1); add_tagged(s, 2, 1, 2); add_tagged(s, 0, 2, 3);
        add_tagged(s, -1, 1, 0);      // added last, packed first
        expect(set_between_flag(s, "t", 2, 1, kMarkOff, true).empty(), "switch off");
        const Packed k = pack(s);
        const size_t F = 4;
        expect(k.from == std::vector<int>({-1, 0, 2, 0}) && k.to == std::vector<int>({1, 1, 1, 2}), "pack 1: from, to (priors first)");
        expect(k.flags == std::vector<unsigned char>({0, 0, 0, kMarkOff, 0}), "pack 1: flags, F + 1 of them");
        // pose 0: from-end of 1 and 3; pose 1: to-end of 0, 1, 2; pose 2: from-end of 2, to-end of 3
        expect(k.row_ptr == std::vector<int>({0, 2, 5, 7}), "pack 1: row_ptr");
        expect(k.ent == std::vector<int>({1 * 2, 3 * 2, 0 * 2 + 1, 1 * 2 + 1, 2 * 2 + 1, 2 * 2, 3 * 2 + 1}), "pack 1: ent = factor * 2 + end, ascending by factor");
        bool ok = k.z.size() == 16 * F && k.omega.size() == 36 * F;
        for (size_t e = 0; ok && e < F; ++e) {
            double i21[21], full[36];
            for (int i = 0; i < 21; ++i) i21[i] = 1000.0 * e + i;
            expand_info(i21, full);
            for (int i = 0; i < 16; ++i) ok = ok && k.z[i * F + e] == 100.0 * e + i;
            for (int i = 0; i < 36; ++i) ok = ok && k.omega[i * F + e] == full[i];
        }
        expect(ok, "pack 1: z and omega at [k * F + e]");
        double i21[21], full[36];
        for (int i = 0; i < 21; ++i) i21[i] = i;
        expand_info(i21, full);
        expect(full[0 * 6 + 5] == 5 && full[5 * 6 + 0] == 5 && full[1 * 6 + 1] == 6 && full[4 * 6 + 5] == 19 && full[5 * 6 + 4] == 19 && full[35] == 20, "expand_info");
    }
    {   // 1 pose, 1 prior
        Store s;
        add_eye_poses(s, 1);
        add_tagged(s, -1, 0, 0);
        const Packed k = pack(s);
        expect(k.from == std::vector<int>({-1}) && k.to == std::vector<int>({0}) && k.flags.size() == 2, "pack 2: the factor");
        expect(k.row_ptr == std::vector<int>({0, 1}) && k.ent == std::vector<int>({1}), "pack 2: the CSR");
    }
    {   // 2 poses, no factor: nothing to index, and still no empty upload
        Store s;
        add_eye_poses(s, 2);
        const Packed k = pack(s);
        expect(k.from.empty() && k.to.empty() && k.z.empty() && k.omega.empty() && k.flags.size() == 1, "pack 3: no factor");
        expect(k.row_ptr == std::vector<int>({0, 0, 0}) && k.ent.size() == 1, "pack 3: row_ptr all zero, ent not empty");
        expect(k.pose_fixed == std::vector<unsigned char>({0, 0, 0}) && !k.any_fixed, "pack 3: pose_fixed, N + 1 of them, none set");
    }
    {   // pack 1's graph with poses 0 and 2 fixed: every factor carries the bits of its ends, beside the mark it has; nothing else moves
        Store s;
        add_eye_poses(s, 3);
        add_tagged(s, 0, 1, 1); add_tagged(s, 2, 1, 2); add_tagged(s, 0, 2, 3);
        add_tagged(s, -1, 1, 0);
        expect(set_between_flag(s, "t", 2, 1, kMarkOff, true).empty(), "switch off");
        const Packed free_k = pack(s);
        expect(!free_k.any_fixed && free_k.flags == std::vector<unsigned char>({0, 0, 0, kMarkOff, 0}), "pack 4: no flag, no bit");
        expect(set_fixed(s, "t", 0, 1, true).empty() && set_fixed(s, "t", 2, 1, true).empty(), "fix 0 and 2");
        const Packed k = pack(s);
        expect(k.any_fixed && k.pose_fixed == std::vector<unsigned char>({1, 0, 1, 0}), "pack 4: pose_fixed");
        // factor 0: the prior on 1 (free); 1: 0 -> 1; 2: 2 -> 1; 3: 0 -> 2, off, both ends fixed
        expect(k.flags == std::vector<unsigned char>({0, kPackFromFixed, kPackFromFixed, (unsigned char)(kMarkOff | kPackFromFixed | kPackToFixed), 0}), "pack 4: the ends' bits");
        expect(k.from == free_k.from && k.to == free_k.to && k.row_ptr == free_k.row_ptr && k.ent == free_k.ent && k.z == free_k.z && k.omega == free_k.omega,
               "pack 4: the flags change nothing else");
        Store p;      // a prior on a fixed pose: the "to" bit, never the "from" bit
        add_eye_poses(p, 1);
        add_tagged(p, -1, 0, 0);
        expect(set_fixed(p, "t", 0, 1, true).empty() && pack(p).flags[0] == kPackToFixed, "pack 4: a prior on a fixed pose");
    }
}

static void check_checks() {
    // a graph with every fault at once; each refusal in its order, then that fault is mended
    Store s;
    add_eye_poses(s, 3);
    const double nan = std::nan(""), inf = HUGE_VAL;
    add_tagged(s, -1, 0, 0); add_tagged(s, -1, 9, 1);
    add_tagged(s, 0, 1, 2); add_tagged(s, 7, 1, 3); add_tagged(s, 2, 2, 4);
    s.poses[16 * 1 + 13] = nan;
    s.priors[0].z[3] = nan; s.priors[0].info[7] = inf;
    s.betweens[0].z[12] = inf; s.betweens[0].info[35] = nan;
    expect_msg(check(s, "t"), "t: prior 1: id 9 out of range (the graph holds 3 poses)");
    s.priors[1].to = 2;
    expect_msg(check(s, "t"), "t: between factor 1: id 7 out of range (the graph holds 3 poses)");
    s.betweens[1].from = 2; s.betweens[1].to = -1;
    expect_msg(check(s, "t"), "t: between factor 1: id -1 out of range (the graph holds 3 poses)");
    s.betweens[1].to = 1;
    expect_msg(check(s, "t"), "t: between factor 2: from == to (2)");
    s.betweens[2].to = 0;
    expect_msg(check(s, "t"), "t: pose 1 is not finite");
    expect_msg(check(s, "t", 2), "t: prior 0: the pose is not finite");      // poses below first_pose are the device's: not looked at
    s.poses[16 * 1 + 13] = 0.0;
    expect_msg(check(s, "t"), "t: prior 0: the pose is not finite");
    s.priors[0].z[3] = 0.0;
    expect_msg(check(s, "t"), "t: prior 0: the information matrix is not finite");
    s.priors[0].info[7] = 1.0;
    expect_msg(check(s, "t"), "t: between factor 0: the pose is not finite");
    s.betweens[0].z[12] = 0.0;
    expect_msg(check(s, "t"), "t: between factor 0: the information matrix is not finite");
    s.betweens[0].info[35] = 1.0;
    expect_msg(check(s, "other"), "");
    { Store one; add_eye_poses(one, 1); add_tagged(one, -1, 1, 0); expect_msg(check(one, "t"), "t: prior 0: id 1 out of range (the graph holds 1 poses)"); }
    { Store e; expect_msg(check(e, "t"), ""); expect(first_pose_without_prior(e) == -1, "an empty graph has no lone pose"); }

    // the mutators' own refusals, and the one revision counter
    Store m;
    const uint64_t r0 = m.revision;
    expect_msg(add_poses(m, "t", nullptr, 1), "t: NULL poses");
    expect_msg(add_poses(m, "t", kEye, kMaxCount + 1), "t: more poses than the device's 32-bit indices address");
    expect_msg(add_factor(m, "t", -1, 0, nullptr, nullptr), "t: NULL pose or information matrix");
    expect_msg(set_between_flag(m, "t", 0, 1, kMarkOff, true), "t: first + count exceeds the number of between factors (0)");
    expect_msg(set_robust_kernel(m, "t", 4, 1.0), "t: unknown kind 4 (PCR_GRAPH_ROBUST_NONE = 0, PCR_GRAPH_ROBUST_HUBER = 1, PCR_GRAPH_ROBUST_GEMAN_MCCLURE = 2, PCR_GRAPH_ROBUST_TUKEY = 3)");
    expect_msg(set_robust_kernel(m, "t", PCR_GRAPH_ROBUST_HUBER, 0.0), "t: delta must be finite and greater than 0");
    expect_msg(set_fixed(m, "t", 0, 1, true), "t: first + count exceeds the number of poses (0)");
    expect(m.revision == r0 && m.structure == r0, "a refused change is none");
    expect(add_poses(m, "t", kEye, 0).empty() && set_between_flag(m, "t", 0, 0, kMarkOff, true).empty() && m.revision == r0, "nothing added, nothing changed");
    add_eye_poses(m, 2);
    add_tagged(m, 0, 1, 0);
    const uint64_t r1 = m.revision;
    expect(r1 == r0 + 3 && m.structure == r1, "every add is a structural change");
    expect(set_robust_kernel(m, "t", PCR_GRAPH_ROBUST_TUKEY, 2.0).empty() && m.revision == r1 + 1 && m.structure == r1, "the kernel is a change, not a structural one");
    expect(set_between_flag(m, "t", 0, 1, kMarkRobust, true).empty() && m.structure == m.revision && m.betweens[0].flags == kMarkRobust, "a mark is structural");
    {   // the fixed flag: the range first (the store untouched), then nothing to do, then a structural change either way
        const uint64_t rf = m.revision;
        expect(m.fixed == std::vector<unsigned char>({0, 0}) && m.n_fixed() == 0, "a new pose is free");
        expect_msg(set_fixed(m, "t", 1, 2, true), "t: first + count exceeds the number of poses (2)");
        expect_msg(set_fixed(m, "t", 3, 0, true), "t: first + count exceeds the number of poses (2)");
        expect_msg(set_fixed(m, "t", 2, (size_t)-1, true), "t: first + count exceeds the number of poses (2)");
        expect(m.revision == rf && m.n_fixed() == 0, "a refused range fixes nothing");
        expect(set_fixed(m, "t", 2, 0, true).empty() && m.revision == rf, "an empty range at the end: nothing changed");
        expect(set_fixed(m, "t", 1, 1, true).empty() && m.revision == rf + 1 && m.structure == m.revision && m.is_fixed(1) && !m.is_fixed(0) && m.n_fixed() == 1,
               "a flag is structural");
        expect(set_fixed(m, "t", 0, 2, false).empty() && m.revision == rf + 2 && m.structure == m.revision && m.n_fixed() == 0, "clearing one is too");
        expect(set_fixed(m, "t", 0, 2, true).empty() && !has_free_pose_with_factor(m), "every pose fixed: nothing to optimise");
        expect(set_fixed(m, "t", 1, 1, false).empty() && has_free_pose_with_factor(m), "one free end of a factor: something to optimise");
        expect(set_between_flag(m, "t", 0, 1, kMarkOff, true).empty() && !has_free_pose_with_factor(m), "... unless the factor is off");
        expect(set_between_flag(m, "t", 0, 1, kMarkOff, false).empty() && set_fixed(m, "t", 0, 1, true).empty(), "as before");
        add_eye_poses(m, 1);
        expect(m.fixed == std::vector<unsigned char>({1, 0, 0}), "the flags stay with their poses when one is added");
    }
    clear(m);
    expect(m.n_poses() == 0 && m.n_factors() == 0 && m.structure == m.revision && m.robust_kind == PCR_GRAPH_ROBUST_TUKEY, "clear keeps the kernel");
    add_eye_poses(m, 1);
    expect(m.fixed == std::vector<unsigned char>({0}), "clear drops the fixed flags");
    double i21[21];
    expect(noise_preset(PCR_GRAPH_ODOM, i21) && i21[0] == 1.0 / 1e-4 && i21[1] == 0.0 && i21[20] == 1.0 / 1e-1 && !noise_preset(3, i21), "noise presets");
}

static void check_union_find() {
    Store s;
    add_eye_poses(s, 9);
    add_tagged(s, -1, 1, 0);
    const int e[][2] = {{0, 1}, {1, 2}, {2, 0}, {5, 4}, {4, 7}, {3, 8}, {8, 2}};      // components {0 1 2 3 8}, {4 5 7}, {6}
    for (auto& x : e) add_tagged(s, x[0], x[1], 1);
    expect(first_pose_without_prior(s) == 4, "union-find: pose 4");
    expect_msg(check_priors(s, "entry"), "entry: pose 4 lies in a connected component without a prior: the system would be singular");
    add_tagged(s, -1, 7, 0);
    expect(first_pose_without_prior(s) == 6, "union-find: pose 6");
    expect(set_between_flag(s, "t", 5, 1, kMarkOff, true).empty(), "switch (3, 8) off");
    expect(first_pose_without_prior(s) == 3, "union-find: pose 3 once its only edge is off");
    expect(set_between_flag(s, "t", 5, 1, kMarkOff, false).empty(), "switch (3, 8) on");
    add_tagged(s, -1, 6, 0);
    expect(first_pose_without_prior(s) == -1, "union-find: every component holds a prior");
    expect_msg(check_priors(s, "entry"), "");
    Store one;
    add_eye_poses(one, 1);
    expect(first_pose_without_prior(one) == 0, "union-find: a lone pose");
    expect(set_fixed(one, "t", 0, 1, true).empty() && first_pose_without_prior(one) == -1, "union-find: a lone fixed pose anchors itself");

    // the anchor rule: a component is anchored by a prior or by a fixed pose
    Store a;
    add_eye_poses(a, 9);
    for (auto& x : e) add_tagged(a, x[0], x[1], 1);      // the same components, no prior anywhere
    expect(first_pose_without_prior(a) == 0, "anchor: no prior, no fixed pose");
    expect(set_fixed(a, "t", 8, 1, true).empty() && first_pose_without_prior(a) == 4, "anchor: pose 8 fixed holds {0 1 2 3 8}");
    expect_msg(check_priors(a, "entry"), "entry: pose 4 lies in a connected component without a prior: the system would be singular");
    expect(set_fixed(a, "t", 4, 4, true).empty() && first_pose_without_prior(a) == -1, "anchor: 4 .. 7 fixed hold {4 5 7} and {6}");
    expect(set_between_flag(a, "t", 5, 1, kMarkOff, true).empty(), "switch (3, 8) off");
    expect(first_pose_without_prior(a) == 3, "anchor: pose 3 once its only edge to the fixed pose is off");
    expect(set_between_flag(a, "t", 5, 1, kMarkOff, false).empty(), "switch (3, 8) on");
    expect(set_between_flag(a, "t", 6, 1, kMarkOff, true).empty(), "switch (8, 2) off");
    expect(first_pose_without_prior(a) == 0, "anchor: the edge that joins {0 1 2} to its fixed pose is off: its first pose is named");
    expect_msg(check_priors(a, "entry"), "entry: pose 0 lies in a connected component without a prior: the system would be singular");
    add_tagged(a, -1, 1, 0);
    expect(first_pose_without_prior(a) == -1, "anchor: a prior holds what the fixed pose no longer does");
    expect(set_fixed(a, "t", 0, 9, false).empty() && first_pose_without_prior(a) == 3, "anchor: the flags cleared, the prior-only rule is back");
}

static bool same(const Factor& a, const Factor& b) {
    return a.from == b.from && a.to == b.to && a.flags == b.flags && memcmp(a.z, b.z, sizeof a.z) == 0 && memcmp(a.info, b.info, sizeof a.info) == 0;
}
static bool same(const Store& a, const Store& b) {
    bool ok = a.poses.size() == b.poses.size() && a.priors.size() == b.priors.size() && a.betweens.size() == b.betweens.size() && a.fixed == b.fixed &&
              (a.poses.empty() || memcmp(a.poses.data(), b.poses.data(), a.poses.size() * sizeof(double)) == 0);
    for (size_t i = 0; ok && i < a.priors.size(); ++i) ok = same(a.priors[i], b.priors[i]);
    for (size_t i = 0; ok && i < a.betweens.size(); ++i) ok = same(a.betweens[i], b.betweens[i]);
    return ok;
}

static void write_text(const std::string& path, const std::string& text) {
    FILE* fp = fopen(path.c_str(), "w");
    if (!fp || fputs(text.c_str(), fp) < 0 || fclose(fp) != 0) { fprintf(stderr, "graph_host_check: cannot write %s\n", path.c_str()); exit(2); }
}

static void check_g2o() {
    const char* base = getenv("TMPDIR");
    std::string dir = std::string(base && *base ? base : "/tmp") + "/graph_host_check.XXXXXX";
    if (!mkdtemp(&dir[0])) { fprintf(stderr, "graph_host_check: cannot make %s\n", dir.c_str()); exit(2); }
    const std::string good = dir + "/good.g2o", bad = dir + "/bad.g2o";

    // write, read back: poses and measurements pass through a quaternion (rounding), the information matrices through 17 digits (the same bits)
    Store a;
    const double quats[3][4] = {{0, 0, 0, 1}, {0.5, -0.5, 0.5, 0.5}, {0.8, 0, -0.6, 0}};      // the trace branch twice, then w = 0: the diagonal branch
    for (int p = 0; p < 3; ++p) {
        const double t[3] = {1.5 * p, -2.25 * p, 0.125 + p};
        double T[16];
        quat_to_pose(quats[p], t, T);
        expect(add_poses(a, "t", T, 1).empty(), "add_poses");
    }
    for (int e = 0; e < 3; ++e) {
        const double t[3] = {0.1 * e, 0.2, -0.3};
        double Z[16], i21[21];
        quat_to_pose(quats[(e + 1) % 3], t, Z);
        for (int k = 0; k < 21; ++k) i21[k] = 1.0 / 3.0 + 7.0 * e + 0.1 * k;
        expect(add_factor(a, "t", e == 2 ? 2 : e, e == 2 ? 0 : e + 1, Z, i21, e == 1 ? kMarkRobust : 0).empty(), "add_factor");
    }
    expect_msg(save_g2o(a, "save", good.c_str()), "");
    Store b;
    expect_msg(load_g2o(b, "load", good.c_str()), "");
    bool ok = b.n_poses() == 3 && b.priors.size() == 1 && b.betweens.size() == 3;
    expect(ok, "g2o: 3 poses, the reader's own prior on vertex 0, 3 edges");
    if (ok) {
        double worst = 0.0, i21[21], full[36];
        for (size_t i = 0; i < a.poses.size(); ++i) worst = std::fmax(worst, std::fabs(a.poses[i] - b.poses[i]));
        for (int e = 0; e < 3; ++e) {
            const Factor &fa = a.betweens[e], &fb = b.betweens[e];
            expect(fa.from == fb.from && fa.to == fb.to && fb.flags == 0, "g2o: an edge's ids; marks are not carried");
            for (int k = 0; k < 16; ++k) worst = std::fmax(worst, std::fabs(fa.z[k] - fb.z[k]));
            for (int k = 0; k < 36; ++k) expect(fa.info[k] == fb.info[k], "g2o: an information entry comes back to the bit");
        }
        expect(worst < 4e-15 * 5, "g2o: poses and measurements come back to rounding");
        noise_preset(PCR_GRAPH_PRIOR, i21);
        expand_info(i21, full);
        expect(b.priors[0].from == -1 && b.priors[0].to == 0 && memcmp(b.priors[0].z, &b.poses[0], sizeof kEye) == 0 && memcmp(b.priors[0].info, full, sizeof full) == 0,
               "g2o: the prior is the preset at vertex 0's pose");
    }

    // refusals: path:line: and the reason; whatever was parsed before the bad line is dropped with it
    Store s;
    add_eye_poses(s, 4);
    add_tagged(s, -1, 0, 0);
    for (int i = 0; i < 3; ++i) add_tagged(s, i, i + 1, i + 1);
    const Store before = s;
    const std::string vertex4 = "VERTEX_SE3:QUAT 4 1 2 3 0 0 0 1\n";
    const struct { std::string text, message; } refused[] = {
        {"VERTEX3 0 0 0 0 0 0 0\n", ":1: VERTEX3 records (Euler angles) are not read: write the graph with VERTEX_SE3:QUAT and EDGE_SE3:QUAT"},
        {"EDGE3 0 1 0 0 0 0 0 0\n", ":1: EDGE3 records (Euler angles) are not read: write the graph with VERTEX_SE3:QUAT and EDGE_SE3:QUAT"},
        {"VERTEX_SE3:QUAT 7 0 0 0 0 0 0 1\n", ":1: vertex id 7 where 4 is next: ids are consecutive from 0"},
        {"EDGE_SE3:QUAT 0 1 0 0 0 0 0 0 1 1 2 3\n", ":1: malformed EDGE_SE3:QUAT: 21 information entries expected"},
        {vertex4 + "EDGE_SE3:QUAT 3 4 0 0 0 0 0 0 1 1 2 3 4 5", ":2: malformed EDGE_SE3:QUAT: 21 information entries expected"},      // the last line breaks off
        {vertex4 + "# a comment\nVERTEX_SE3:QUAT 5 1 2", ":3: malformed VERTEX_SE3:QUAT"},
        {vertex4 + "EDGE_SE3:QUAT 3", ":2: malformed EDGE_SE3:QUAT"},
        {"EDGE_SE3:QUAT -1 2 0 0 0 0 0 0 1 1 0 0 0 0 0 1 0 0 0 0 1 0 0 0 1 0 0 1 0 1\n", ":1: negative id"},
        {vertex4 + "FIX 5\n", ":2: FIX 5: the file defines no vertex of that id"},
        {vertex4 + "FIX 3\n", ":2: FIX 3: the file defines no vertex of that id"},      // the store's own pose: not the file's
        {"FIX 4 9\n" + vertex4, ":1: FIX 9: the file defines no vertex of that id"},     // the first id is fine (defined further down), the second is not
        {vertex4 + "FIX -1\n", ":2: FIX -1: the file defines no vertex of that id"},
        {vertex4 + "FIX\n", ":2: malformed FIX"},
    };
    for (const auto& r : refused) {
        write_text(bad, r.text);
        expect_msg(load_g2o(s, "load", bad.c_str()), "load: " + bad + r.message);
        expect(same(s, before) && s.revision == before.revision, "g2o: a refused file leaves the store as it was");
    }
    write_text(bad, "");      // an empty file is read, and holds nothing
    expect_msg(load_g2o(s, "load", bad.c_str()), "");
    expect(same(s, before), "g2o: an empty file adds nothing");
    expect_msg(load_g2o(s, "load", (dir + "/missing.g2o").c_str()), "load: cannot open " + dir + "/missing.g2o");
    expect_msg(load_g2o(s, "load", nullptr), "load: NULL path");
    expect_msg(save_g2o(s, "save", (dir + "/none/x.g2o").c_str()), "save: cannot open " + dir + "/none/x.g2o");
    write_text(bad, vertex4 + "FIX 4\n\nEDGE_SE3:QUAT 4 0 0 0 1 0 0 0 1 1 0 0 0 0 0 1 0 0 0 0 1 0 0 0 1 0 0 1 0 1\n");      // and a good one is appended
    expect_msg(load_g2o(s, "load", bad.c_str()), "");
    expect(s.n_poses() == 5 && s.priors.size() == 1 && s.betweens.size() == 4 && s.betweens[3].from == 4 && s.betweens[3].to == 0 && s.poses[16 * 4 + 13] == 2.0,
           "g2o: a good file is appended, no second prior (vertex 0 is not in it)");
    expect(s.fixed == std::vector<unsigned char>({0, 0, 0, 0, 1}), "g2o: FIX 4 fixes the file's vertex 4 and no other pose");

    // FIX records: written after the vertices, read back, and the second save is the first one's bytes; without a flag no record is written
    {
        const std::string one = dir + "/one.g2o", two = dir + "/two.g2o", plain = dir + "/plain.g2o";
        auto slurp = [](const std::string& path) { std::ifstream in(path); std::stringstream ss; ss << in.rdbuf(); return ss.str(); };
        expect_msg(save_g2o(a, "save", plain.c_str()), "");
        const std::string plain_text = slurp(plain);
        expect(plain_text.find("FIX") == std::string::npos && plain_text == slurp(good), "g2o: no flag, no FIX record");
        Store f = a;
        expect(set_fixed(f, "t", 0, 1, true).empty() && set_fixed(f, "t", 2, 1, true).empty(), "fix 0 and 2");
        expect_msg(save_g2o(f, "save", one.c_str()), "");
        const std::string text = slurp(one);
        const size_t last_vertex = text.rfind("VERTEX_SE3:QUAT"), fix0 = text.find("FIX 0\nFIX 2\n"), first_edge = text.find("EDGE_SE3:QUAT");
        expect(fix0 != std::string::npos && last_vertex < fix0 && fix0 < first_edge, "g2o: one FIX record per fixed pose, after the vertices");
        Store back;
        expect_msg(load_g2o(back, "load", one.c_str()), "");
        expect(back.fixed == std::vector<unsigned char>({1, 0, 1}), "g2o: the flags come back");
        // (poses pass through a quaternion: the text of a second save is compared after a second load, whose quaternions are the first save's)
        expect_msg(save_g2o(back, "save", two.c_str()), "");
        Store again;
        expect_msg(load_g2o(again, "load", two.c_str()), "");
        expect(again.fixed == back.fixed, "g2o: ... and again");
        expect(set_fixed(f, "t", 0, 3, false).empty(), "free them");
        expect_msg(save_g2o(f, "save", one.c_str()), "");
        expect(slurp(one) == plain_text, "g2o: flags set and cleared: the bytes of a store that never had one");
        unlink(one.c_str()); unlink(two.c_str()); unlink(plain.c_str());
    }
    unlink(good.c_str()); unlink(bad.c_str()); rmdir(dir.c_str());
}

// ---- scripted controller runs ------------------------------------------------------------------------------------------------------------

static bool number(std::istringstream& ss, double* v) {
    std::string w;
    if (!(ss >> w)) return false;
    char* end = nullptr;
    *v = strtod(w.c_str(), &end);
    return end && *end == 0 && end != w.c_str();
}

static int run_script(const char* path) {
    std::ifstream in(path);
    if (!in.is_open()) { fprintf(stderr, "graph_host_check: cannot open %s\n", path); return 2; }
    std::string line, name;
    LmState lm = LmState();
    bool open = false;
    int step = 0, ignored = 0;
    auto end_case = [&]() {
        if (!open) return;
        const pcr_graph_result r = lm_result(lm);
        printf("%s end: chi2 %a lambda %a converged %d iterations %d accepted %d pcg_iterations %lld pcg_capped %d ignored %d\n", name.c_str(), r.chi2_final,
               r.lambda, r.converged, r.iterations, r.accepted, (long long)r.pcg_iterations, r.pcg_capped, ignored);
    };
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string tag;
        ss >> tag;
        if (tag == "case") {
            end_case();
            pcr_graph_params p;
            memset(&p, 0, sizeof p);
            p.struct_size = (uint32_t)sizeof p;
            p.pcg_rel_tol = 1e-10;
            double it = 0, chi2 = 0;
            if (!(ss >> name) || !number(ss, &it) || !number(ss, &p.rel_tol) || !number(ss, &p.abs_tol) || !number(ss, &p.lambda_init) ||
                !number(ss, &p.lambda_factor) || !number(ss, &p.lambda_max) || !number(ss, &chi2)) {
                fprintf(stderr, "graph_host_check: %s: malformed case line \"%s\"\n", path, line.c_str());
                return 2;
            }
            p.max_iterations = (int32_t)it;
            const std::string refusal = check_params("case", p);
            if (!refusal.empty()) { fprintf(stderr, "graph_host_check: %s: %s: %s\n", path, name.c_str(), refusal.c_str()); return 2; }
            lm_init(&lm, p, chi2);
            open = true; step = 0; ignored = 0;
        } else if (tag == "step") {
            double chi2_new = 0, it = 0, flag = 0;
            if (!open || !number(ss, &chi2_new) || !number(ss, &it) || !number(ss, &flag)) {
                fprintf(stderr, "graph_host_check: %s: malformed step line \"%s\"\n", path, line.c_str());
                return 2;
            }
            if (!lm_wants_trial(lm)) { ++ignored; continue; }
            const int d = lm_step(&lm, chi2_new, (int)it, (int)flag);
            printf("%s step %d: %s%s chi2 %a lambda %a converged %d iterations %d accepted %d pcg_iterations %lld pcg_capped %d\n", name.c_str(), step++,
                   (d & kLmAccept) ? "accept" : "reject", (d & kLmStop) ? "+stop" : "", lm.chi2, lm.lambda, lm.res.converged, lm.res.iterations, lm.res.accepted,
                   (long long)lm.res.pcg_iterations, lm.res.pcg_capped);
        }
    }
    end_case();
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2) {
        for (int i = 1; i < argc; ++i) { const int rc = run_script(argv[i]); if (rc) return rc; }
        return 0;
    }
    check_pack();
    check_checks();
    check_union_find();
    check_g2o();
    printf("graph_host_check: pack, checks, union-find, g2o: %d failed\n", g_bad);
    return g_bad ? 1 : 0;
}
