// graph_forest_check -- plan_forest() (csrc/graph_forest.h), the spanning forest and path schedule of the pose graph's tree preconditioner, on
// the CPU: no GPU call, no HIP header.  Plans every edge list it is given (or a built-in set), checks the plan's invariants and prints one
// line per graph.  Built with -fsanitize=address,undefined it is the checked run of the forest function.
//
// usage: graph_forest_check [edges.txt ...]      a file holds graphs, each: "graph NAME N", then lines "prior ID", "fixed ID" and "edge FROM TO"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../csrc/graph_forest.h"

using pcr::graph::ForestPlan;
using pcr::graph::plan_forest;

struct Case {
    std::string name;
    size_t N = 0;
    std::vector<long long> from, to, prior, fixed;      // fixed: the poses that carry the fixed flag, anchors like the priors'
    std::vector<int> roots;                             // when not empty: the roots worked by hand, ascending
};

static int fail(const Case& c, const char* what, long long at) {
    fprintf(stderr, "graph_forest_check: %s: %s (at %lld)\n", c.name.c_str(), what, at);
    return 1;
}

static int check(const Case& c) {
    // the anchors as pcr_graph hands them over: the priors' poses, then the fixed poses
    std::vector<long long> anchors(c.prior);
    anchors.insert(anchors.end(), c.fixed.begin(), c.fixed.end());
    const ForestPlan f = plan_forest(c.N, c.from.data(), c.to.data(), c.from.size(), anchors.data(), anchors.size());
    const int N = (int)c.N;
    if (f.n_tree + f.n_other != c.from.size()) return fail(c, "tree + other edges != between factors", (long long)f.n_tree);
    if ((int)f.node.size() != N || (int)f.pos_of.size() != N) return fail(c, "positions do not cover the poses", (long long)f.node.size());
    int roots = 0;
    for (int p = 0; p < N; ++p) {
        if (f.pos_of[p] < 0 || f.pos_of[p] >= N || f.node[f.pos_of[p]] != p) return fail(c, "pos_of and node are not inverse", p);
        const int par = f.parent[p];
        if (par < 0) { ++roots; if (f.tree_factor[p] != -1) return fail(c, "a root with a tree factor", p); continue; }
        if (f.pos_of[par] <= f.pos_of[p]) return fail(c, "a parent is not after its child in elimination order", p);
        const int e = f.tree_factor[p];
        if (e < 0 || (size_t)e >= c.from.size() || !f.in_tree[e]) return fail(c, "tree factor out of range or not in the forest", p);
        const long long me = f.is_to[p] ? c.to[e] : c.from[e], other = f.is_to[p] ? c.from[e] : c.to[e];
        if (me != p || other != par) return fail(c, "the tree factor does not join the pose to its parent", p);
    }
    if ((size_t)(N - roots) != f.n_tree) return fail(c, "poses - roots != tree edges", roots);
    // the root rule: a component's root is its lowest-numbered anchor (a prior's pose or a fixed pose), its lowest-numbered pose when it has none
    {
        std::vector<uint8_t> anchor(N, 0);
        for (long long a : anchors) anchor[a] = 1;
        std::vector<int> root_of(N, -1), want(N, -1);      // by walking up; per root the pose the rule names
        for (int p = 0; p < N; ++p) { int r = p; while (f.parent[r] >= 0) r = f.parent[r]; root_of[p] = r; }
        for (int p = 0; p < N; ++p) if (anchor[p] && want[root_of[p]] < 0) want[root_of[p]] = p;
        for (int p = 0; p < N; ++p) if (want[root_of[p]] < 0) want[root_of[p]] = p;
        std::vector<int> got;
        for (int p = 0; p < N; ++p) {
            if (f.parent[p] >= 0) continue;
            got.push_back(p);
            if (want[p] != p) return fail(c, "a root is not the lowest-numbered anchor of its component", p);
        }
        if (!c.roots.empty() && got != c.roots) return fail(c, "the roots are not the ones worked by hand", got.empty() ? -1 : got[0]);
    }
    // children CSR: ascending, complete; the heavy child
    std::vector<int> size(N, 1);
    for (int q = 0; q < N; ++q) { const int p = f.node[q]; if (f.parent[p] >= 0) size[f.parent[p]] += size[p]; }
    for (int p = 0; p < N; ++p) {
        int best = -1;
        for (int k = f.child_ptr[p]; k < f.child_ptr[p + 1]; ++k) {
            const int ch = f.child[k];
            if (f.parent[ch] != p) return fail(c, "a listed child has another parent", p);
            if (k > f.child_ptr[p] && f.child[k - 1] >= ch) return fail(c, "children do not ascend", p);
            if (best < 0 || size[ch] > size[best]) best = ch;
        }
        if (f.heavy[p] != best) return fail(c, "the heavy child is not the largest subtree (lowest id on a tie)", p);
    }
    if (f.child_ptr[N] != N - roots) return fail(c, "the children list does not hold every non-root", f.child_ptr[N]);
    // paths: contiguous positions, bottom to head along heavy children; rounds ascend and respect the light children
    const int paths = (int)f.path_ptr.size() - 1;
    if ((int)f.path_round.size() != paths || f.path_ptr[paths] != N) return fail(c, "paths do not cover the positions", paths);
    std::vector<int> path_of(N, -1);
    for (int k = 0; k < paths; ++k) {
        if (f.path_ptr[k + 1] <= f.path_ptr[k]) return fail(c, "an empty path", k);
        if (k > 0 && f.path_round[k] < f.path_round[k - 1]) return fail(c, "rounds do not ascend", k);
        for (int q = f.path_ptr[k]; q < f.path_ptr[k + 1]; ++q) {
            path_of[f.node[q]] = k;
            const int below = q > f.path_ptr[k] ? f.node[q - 1] : -1;
            if (f.heavy[f.node[q]] != below) return fail(c, "a path does not follow the heavy children", q);
        }
    }
    for (int r = 0; r < f.rounds(); ++r)
        for (int k = f.round_ptr[r]; k < f.round_ptr[r + 1]; ++k)
            if (f.path_round[k] != r) return fail(c, "round_ptr disagrees with path_round", k);
    if (f.round_ptr[f.rounds()] != paths) return fail(c, "round_ptr does not cover the paths", paths);
    for (int k = 0; k < paths; ++k) {
        int want = 0;
        for (int q = f.path_ptr[k]; q < f.path_ptr[k + 1]; ++q) {
            const int p = f.node[q];
            for (int i = f.child_ptr[p]; i < f.child_ptr[p + 1]; ++i)
                if (f.child[i] != f.heavy[p] && f.path_round[path_of[f.child[i]]] + 1 > want) want = f.path_round[path_of[f.child[i]]] + 1;
        }
        if (f.path_round[k] != want) return fail(c, "a path's round is not 1 + the largest round hanging off it", k);
    }
    int log2n = 0;
    while ((1 << log2n) < N) ++log2n;
    if (f.rounds() > log2n + 1) return fail(c, "more rounds than log2(N) + 1", f.rounds());
    printf("%s: poses %d priors %zu between %zu | tree %zu other %zu roots %d paths %d rounds %d", c.name.c_str(), N, c.prior.size(), c.from.size(),
           f.n_tree, f.n_other, roots, paths, f.rounds());
    if (!c.fixed.empty()) printf(" | fixed %zu", c.fixed.size());
    printf("\n");
    return 0;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static std::vector<Case> built_in() {
    std::vector<Case> out;
    { Case c; c.name = "empty"; out.push_back(c); }
    { Case c; c.name = "one"; c.N = 1; c.prior = {0}; out.push_back(c); }
    { Case c; c.name = "two"; c.N = 2; c.prior = {0}; c.from = {0}; c.to = {1}; out.push_back(c); }
    for (int n : {300, 1025, 20000}) {
        Case c; c.name = "chain" + std::to_string(n); c.N = n; c.prior = {0};
        for (int i = 0; i + 1 < n; ++i) { c.from.push_back(i); c.to.push_back(i + 1); }
        c.from.push_back(0); c.to.push_back(n - 1);
        out.push_back(c);
    }
    { Case c; c.name = "chain against its ids"; c.N = 40; c.prior = {39};
      for (int i = 0; i + 1 < 40; ++i) { c.from.push_back(i + 1); c.to.push_back(i); }
      out.push_back(c); }
    { Case c; c.name = "star"; c.N = 65; c.prior = {0};
      for (int i = 1; i < 65; ++i) { c.from.push_back(0); c.to.push_back(i); }
      for (int i = 0; i < 3; ++i) { c.from.push_back(5 + i); c.to.push_back(40 + i); }
      out.push_back(c); }
    for (int n : {200, 5000}) {
        Case c; c.name = "closest key frame " + std::to_string(n); c.N = n; c.prior = {0};
        for (int i = 1; i < n; ++i) { c.from.push_back((long long)(rnd() % i)); c.to.push_back(i); }
        c.from.push_back(n - 1); c.to.push_back(3);                       // from > to
        c.from.push_back(c.from[10]); c.to.push_back(c.to[10]);           // a duplicate of a tree edge
        c.from.push_back(7); c.to.push_back(n / 2);
        out.push_back(c);
    }
    { Case c; c.name = "two components, no prior on the second"; c.N = 9; c.prior = {1, 1};
      const int e[][2] = {{0, 1}, {1, 2}, {2, 0}, {5, 4}, {4, 7}, {3, 8}, {8, 2}};
      for (auto& x : e) { c.from.push_back(x[0]); c.to.push_back(x[1]); }
      out.push_back(c); }
    // fixed poses as roots, worked by hand.  A chain 0 - 1 - ... - 11:
    { Case c; c.name = "fixed root, no prior"; c.N = 12; c.fixed = {5}; c.roots = {5};
      for (int i = 0; i + 1 < 12; ++i) { c.from.push_back(i); c.to.push_back(i + 1); }
      out.push_back(c); }
    { Case c; c.name = "fixed block below the prior"; c.N = 12; c.prior = {8}; c.fixed = {4, 5, 6, 7}; c.roots = {4};      // 4 < 8: the fixed pose wins
      for (int i = 0; i + 1 < 12; ++i) { c.from.push_back(i); c.to.push_back(i + 1); }
      c.from.push_back(11); c.to.push_back(0);
      out.push_back(c); }
    { Case c; c.name = "prior below the fixed block"; c.N = 12; c.prior = {0}; c.fixed = {7, 6, 5, 4}; c.roots = {0};       // in any order
      for (int i = 0; i + 1 < 12; ++i) { c.from.push_back(i); c.to.push_back(i + 1); }
      out.push_back(c); }
    { Case c; c.name = "two components, a fixed pose holds the second"; c.N = 9; c.prior = {1}; c.fixed = {7, 6}; c.roots = {1, 4 /* no anchor */, 6, 7};
      const int e[][2] = {{0, 1}, {1, 2}, {2, 0}, {5, 4}, {3, 8}, {8, 2}};      // {0 1 2 3 8}, {4 5}, {6}, {7}
      for (auto& x : e) { c.from.push_back(x[0]); c.to.push_back(x[1]); }
      out.push_back(c); }
    { Case c; c.name = "the same pose holds a prior and is fixed"; c.N = 3; c.prior = {2}; c.fixed = {2}; c.roots = {2};
      c.from = {0, 1}; c.to = {1, 2};
      out.push_back(c); }
    { Case c; c.name = "binary tree"; c.N = 1023; c.prior = {0};
      for (int i = 1; i < 1023; ++i) { c.from.push_back((i - 1) / 2); c.to.push_back(i); }
      out.push_back(c); }
    return out;
}

static int read_file(const char* path, std::vector<Case>& out) {
    std::ifstream in(path);
    if (!in.is_open()) { fprintf(stderr, "graph_forest_check: cannot open %s\n", path); return 1; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string tag;
        ss >> tag;
        if (tag == "graph") {
            Case c;
            long long n = -1;
            if (!(ss >> c.name >> n) || n < 0) { fprintf(stderr, "graph_forest_check: %s: malformed graph line\n", path); return 1; }
            c.N = (size_t)n;
            out.push_back(c);
        } else if (tag == "prior" || tag == "fixed" || tag == "edge") {
            if (out.empty()) { fprintf(stderr, "graph_forest_check: %s: a record before the first graph line\n", path); return 1; }
            Case& c = out.back();
            long long a = -1, b = -1;
            const bool ok = tag != "edge" ? !!(ss >> a) : !!(ss >> a >> b);
            // what pcr_graph's own check refuses before anything is planned
            if (!ok || a < 0 || (size_t)a >= c.N || (tag == "edge" && (b < 0 || (size_t)b >= c.N || a == b))) {
                fprintf(stderr, "graph_forest_check: %s: %s: id out of range or from == to in \"%s\"\n", path, c.name.c_str(), line.c_str());
                return 1;
            }
            if (tag == "prior") c.prior.push_back(a);
            else if (tag == "fixed") c.fixed.push_back(a);
            else { c.from.push_back(a); c.to.push_back(b); }
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    std::vector<Case> cases;
    if (argc < 2) cases = built_in();
    for (int i = 1; i < argc; ++i) if (read_file(argv[i], cases)) return 2;
    int bad = 0;
    for (const Case& c : cases) bad += check(c);
    printf("%zu graphs, %d failed\n", cases.size(), bad);
    return bad ? 1 : 0;
}
