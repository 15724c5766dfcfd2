// graph_forest.h -- the spanning forest of the pose graph's tree preconditioner and the schedule its sweeps run by, decided on the host.
// Host-only and free of HIP types: plan_forest() is a pure function of the factor lists, so the rule below runs, prints and is tested
// without a GPU (pcr_graph_tree, host/graph_forest_check.cpp, tests/test_graph_tree_host.py).  DESIGN.md 4.17.
//
// The rule.  The between factors are taken in the order they were added; one joins the forest when its two ends lie in different components
// (union-find).  Every other between factor -- a loop closure, a duplicate of a tree edge, whatever its noise and whichever way it points --
// is left to the conjugate gradient.  The root of a component is its lowest-numbered ANCHOR: a pose that holds a prior or is fixed (a component
// without one, which pcr_graph_optimize refuses, is rooted at its lowest-numbered pose).  The caller lists the fixed poses among prior_id[]:
// to this function the two kinds of anchor are one, and without a fixed pose the plan is what it was before poses could be fixed.  No ordering of the ids is assumed.
//
// The schedule.  Every tree is cut into paths: a node continues into its child with the largest subtree (the lowest id on a tie), every
// other ("light") child heads a path of its own.  A path's round is 0 when no light child hangs off its nodes, otherwise 1 + the largest
// round among the paths that do.  A light child's subtree holds at most half of its parent's, so there are at most log2(N) + 1 rounds.
// Positions number the nodes path by path -- paths by round, then by head id; inside a path from its bottom node to its head -- which is an
// elimination order: every child has a lower position than its parent.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <numeric>
#include <vector>

namespace pcr {
namespace graph {

struct ForestPlan {
    size_t n_tree = 0, n_other = 0;          // between factors in the forest; the others
    std::vector<int> parent;                 // per pose: the parent pose, -1 for a root
    std::vector<int> tree_factor;            // per pose: its tree factor's index among the between factors, -1 for a root
    std::vector<uint8_t> is_to;              // per pose: 1 when the pose is the "to" end of its tree factor
    std::vector<uint8_t> in_tree;            // per between factor
    std::vector<int> child_ptr, child;       // children of pose p: child[child_ptr[p] .. child_ptr[p + 1]), ascending id
    std::vector<int> heavy;                  // per pose: the child its path continues into, -1 at a path's bottom
    std::vector<int> path_ptr, node;         // path k holds positions [path_ptr[k], path_ptr[k + 1]); node[position] = the pose, bottom first
    std::vector<int> path_round;             // per path, ascending
    std::vector<int> round_ptr;              // round r holds paths [round_ptr[r], round_ptr[r + 1])
    std::vector<int> pos_of;                 // per pose: its position
    int rounds() const { return (int)round_ptr.size() - 1; }
};

// N poses; B between factors (from[e], to[e], every id in [0, N), from != to); P anchors: the poses prior_id[] hold a prior or are fixed
// (in any order, repeats allowed).
inline ForestPlan plan_forest(size_t N, const long long* from, const long long* to, size_t B, const long long* prior_id, size_t P) {
    ForestPlan f;
    const int n = (int)N;
    f.parent.assign(N, -1);
    f.tree_factor.assign(N, -1);
    f.is_to.assign(N, 0);
    f.in_tree.assign(B, 0);
    f.heavy.assign(N, -1);
    f.pos_of.assign(N, -1);
    f.child_ptr.assign(N + 1, 0);
    f.path_ptr.assign(1, 0);
    f.round_ptr.assign(1, 0);

    // the forest's edges, and each pose's neighbours in it (CSR over both ends)
    std::vector<int> uf(N);
    std::iota(uf.begin(), uf.end(), 0);
    auto find = [&](int a) { while (uf[a] != a) { uf[a] = uf[uf[a]]; a = uf[a]; } return a; };
    std::vector<int> deg(N + 1, 0);
    for (size_t e = 0; e < B; ++e) {
        const int a = find((int)from[e]), b = find((int)to[e]);
        if (a == b) { ++f.n_other; continue; }
        uf[a > b ? a : b] = a > b ? b : a;
        f.in_tree[e] = 1;
        ++f.n_tree;
        ++deg[from[e] + 1];
        ++deg[to[e] + 1];
    }
    for (size_t p = 0; p < N; ++p) deg[p + 1] += deg[p];
    std::vector<int> adj(deg[N] > 0 ? deg[N] : 1), fill(deg.begin(), deg.end() - 1);
    for (size_t e = 0; e < B; ++e) {
        if (!f.in_tree[e]) continue;
        adj[fill[from[e]]++] = (int)(e * 2);           // the neighbour is the factor's "to" end
        adj[fill[to[e]]++] = (int)(e * 2 + 1);         // ... its "from" end
    }

    // roots: per component the lowest-numbered anchor, else the lowest-numbered pose
    std::vector<int> root(N, -1);
    std::vector<uint8_t> has_prior(N, 0);
    for (size_t i = 0; i < P; ++i) has_prior[prior_id[i]] = 1;
    for (int p = 0; p < n; ++p) if (has_prior[p] && root[find(p)] < 0) root[find(p)] = p;
    for (int p = 0; p < n; ++p) if (root[find(p)] < 0) root[find(p)] = p;

    // breadth first from every root: parents, and an order in which a parent comes before its children
    std::vector<int> order;
    order.reserve(N);
    std::vector<uint8_t> seen(N, 0);
    for (int p = 0; p < n; ++p) {
        if (root[find(p)] != p) continue;
        seen[p] = 1;
        order.push_back(p);
    }
    for (size_t head = 0; head < order.size(); ++head) {
        const int p = order[head];
        for (int i = deg[p]; i < deg[p + 1]; ++i) {
            const int e = adj[i] >> 1;
            const int q = (adj[i] & 1) ? (int)from[e] : (int)to[e];
            if (seen[q]) continue;
            seen[q] = 1;
            f.parent[q] = p;
            f.tree_factor[q] = e;
            f.is_to[q] = (adj[i] & 1) ? 0 : 1;
            order.push_back(q);
        }
    }

    // children in ascending id, subtree sizes, the heavy child
    for (int p = 0; p < n; ++p) if (f.parent[p] >= 0) ++f.child_ptr[f.parent[p] + 1];
    for (size_t p = 0; p < N; ++p) f.child_ptr[p + 1] += f.child_ptr[p];
    f.child.assign(f.child_ptr[N] > 0 ? f.child_ptr[N] : 0, 0);
    {
        std::vector<int> at(f.child_ptr.begin(), f.child_ptr.end() - 1);
        for (int p = 0; p < n; ++p) if (f.parent[p] >= 0) f.child[at[f.parent[p]]++] = p;
    }
    std::vector<int> size(N, 1), level(N, 0);      // level: the round of the part of p's path at and below p
    for (size_t i = order.size(); i-- > 0;) {
        const int p = order[i];
        int best = -1;
        for (int k = f.child_ptr[p]; k < f.child_ptr[p + 1]; ++k) {
            const int c = f.child[k];
            size[p] += size[c];
            if (best < 0 || size[c] > size[best]) best = c;
        }
        f.heavy[p] = best;
        int lv = 0;
        for (int k = f.child_ptr[p]; k < f.child_ptr[p + 1]; ++k) {
            const int c = f.child[k];
            const int v = (c == best) ? level[c] : level[c] + 1;
            if (v > lv) lv = v;
        }
        level[p] = lv;
    }

    // paths: heads are the roots and the light children; by round, then by head id
    int n_rounds = 0;
    std::vector<int> heads;
    for (int p = 0; p < n; ++p) {
        const bool head = f.parent[p] < 0 || f.heavy[f.parent[p]] != p;
        if (!head) continue;
        heads.push_back(p);
        if (level[p] + 1 > n_rounds) n_rounds = level[p] + 1;
    }
    std::vector<int> count(n_rounds + 1, 0);
    for (int h : heads) ++count[level[h] + 1];
    for (int r = 0; r < n_rounds; ++r) count[r + 1] += count[r];
    f.round_ptr.assign(count.begin(), count.end());
    if (f.round_ptr.empty()) f.round_ptr.assign(1, 0);
    std::vector<int> sorted(heads.size());
    {
        std::vector<int> at(count.begin(), count.end());
        for (int h : heads) sorted[at[level[h]]++] = h;      // heads ascend, so every round's do
    }
    f.node.reserve(N);
    std::vector<int> walk;
    for (int h : sorted) {
        walk.clear();
        for (int p = h; p >= 0; p = f.heavy[p]) walk.push_back(p);
        for (size_t i = walk.size(); i-- > 0;) {
            f.pos_of[walk[i]] = (int)f.node.size();
            f.node.push_back(walk[i]);
        }
        f.path_ptr.push_back((int)f.node.size());
        f.path_round.push_back(level[h]);
    }
    return f;
}

}  // namespace graph
}  // namespace pcr
