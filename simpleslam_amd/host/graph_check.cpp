// graph_check -- backend::PoseGraph (PCR/HipRegister.hpp) over a graph read from a g2o file, on the GPU: chi2 before, chi2 after and the
// iteration counts.  usage: graph_check graph.g2o [out.g2o] [--preconditioner block_jacobi|tree] [--robust none|huber|geman_mcclure|tukey
// --delta D] [--loops-robust] [--fix-before N]   (block_jacobi and none when absent).  --loops-robust marks every between factor that
// pcr_graph_tree leaves outside the forest (g2o files carry no marks); with a robust kernel the s and w of the ten lowest-weight factors are
// printed after the solve.  --fix-before N fixes poses [0, N) before optimising (on top of the file's FIX records) and prints how many poses
// were free; the fixed ones are checked to come back bit for bit.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "PCR/HipRegister.hpp"

// The between factors outside the forest, by the rule of the tree preconditioner (pcr_hip.h): in file order an edge joins the forest when its
// ends lie in different components.  The library tells the counts, not the edges, so the ids are read from the file's EDGE_SE3:QUAT records.
static std::vector<size_t> edges_outside_the_forest(const char* path, size_t n_poses) {
    std::vector<size_t> uf(n_poses), out;
    std::iota(uf.begin(), uf.end(), (size_t)0);
    auto find = [&](size_t a) { while (uf[a] != a) { uf[a] = uf[uf[a]]; a = uf[a]; } return a; };
    std::ifstream in(path);
    std::string line, tag;
    size_t e = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        long long i = -1, j = -1;
        if (!(ss >> tag) || tag != "EDGE_SE3:QUAT" || !(ss >> i >> j)) continue;
        if (i >= 0 && j >= 0 && (size_t)i < n_poses && (size_t)j < n_poses) {
            const size_t a = find((size_t)i), b = find((size_t)j);
            if (a == b) out.push_back(e);
            else uf[std::max(a, b)] = std::min(a, b);
        }
        ++e;
    }
    return out;
}

int main(int argc, char** argv) {
    int precond = PCR_GRAPH_PRECOND_BLOCK_JACOBI, robust = PCR_GRAPH_ROBUST_NONE;
    double delta = 1.0;
    bool loops_robust = false;
    long long fix_before = 0;
    const char* files[2] = {nullptr, nullptr};
    int n_files = 0;
    bool bad = false;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--preconditioner") && i + 1 < argc) {
            ++i;
            if (!strcmp(argv[i], "tree")) precond = PCR_GRAPH_PRECOND_TREE;
            else if (!strcmp(argv[i], "block_jacobi")) precond = PCR_GRAPH_PRECOND_BLOCK_JACOBI;
            else bad = true;
        } else if (!strcmp(argv[i], "--robust") && i + 1 < argc) {
            ++i;
            if (!strcmp(argv[i], "none")) robust = PCR_GRAPH_ROBUST_NONE;
            else if (!strcmp(argv[i], "huber")) robust = PCR_GRAPH_ROBUST_HUBER;
            else if (!strcmp(argv[i], "geman_mcclure")) robust = PCR_GRAPH_ROBUST_GEMAN_MCCLURE;
            else if (!strcmp(argv[i], "tukey")) robust = PCR_GRAPH_ROBUST_TUKEY;
            else bad = true;
        } else if (!strcmp(argv[i], "--delta") && i + 1 < argc) delta = atof(argv[++i]);
        else if (!strcmp(argv[i], "--loops-robust")) loops_robust = true;
        else if (!strcmp(argv[i], "--fix-before") && i + 1 < argc) { fix_before = atoll(argv[++i]); if (fix_before < 0) bad = true; }
        else if (n_files < 2 && argv[i][0] != '-') files[n_files++] = argv[i];
        else bad = true;
    }
    if (bad || n_files < 1) {
        fprintf(stderr, "usage: %s graph.g2o [out.g2o] [--preconditioner block_jacobi|tree] [--robust none|huber|geman_mcclure|tukey --delta D] [--loops-robust] [--fix-before N]\n",
                argv[0]);
        return 2;
    }
    try {
        backend::PoseGraph graph;
        graph.loadG2o(files[0]);
        if (loops_robust) {
            size_t n_tree = 0, n_other = 0;
            graph.tree(&n_tree, &n_other);
            const std::vector<size_t> loops = edges_outside_the_forest(files[0], graph.poses());
            if (loops.size() != n_other) {
                fprintf(stderr, "graph_check: %zu edges outside the forest by the file, %zu by pcr_graph_tree\n", loops.size(), n_other);
                return 1;
            }
            for (size_t e : loops) graph.setBetweenRobust(e);
            printf("loops_marked %zu\n", loops.size());
        }
        if (robust != PCR_GRAPH_ROBUST_NONE) graph.setRobustKernel(robust, delta);
        if (fix_before > 0) graph.setFixed(0, (size_t)fix_before);      // (a range beyond the poses is the library's to refuse)
        const std::vector<uint8_t> fixed = graph.fixed();
        const size_t n_fixed = (size_t)std::count(fixed.begin(), fixed.end(), (uint8_t)1);
        if (n_fixed) printf("poses_fixed %zu poses_free %zu\n", n_fixed, fixed.size() - n_fixed);
        const std::vector<PCR::pose_t> held = n_fixed ? graph.poses(0, fixed.size()) : std::vector<PCR::pose_t>();
        const double before = graph.chi2();
        const backend::PoseGraph::Result r = graph.optimize(precond);
        if (n_fixed) {
            const std::vector<PCR::pose_t> now = graph.poses(0, fixed.size());
            for (size_t p = 0; p < fixed.size(); ++p)
                if (fixed[p] && memcmp(held[p].data(), now[p].data(), 16 * sizeof(double)) != 0) {
                    fprintf(stderr, "graph_check: fixed pose %zu moved\n", p);
                    return 1;
                }
        }
        printf("poses %zu factors %zu\n", graph.poses(), graph.factors());
        printf("chi2_before %.17g\nchi2_after %.17g\n", before, r.chi2_final);
        printf("lm_iterations %d accepted %d pcg_iterations %lld pcg_capped %d converged %d lambda %g\n", r.iterations, r.accepted,
               (long long)r.pcg_iterations, r.pcg_capped, r.converged, r.lambda);
        if (robust != PCR_GRAPH_ROBUST_NONE) {
            const backend::PoseGraph::Weights v = graph.betweenWeights();
            std::vector<size_t> order(v.w.size());
            std::iota(order.begin(), order.end(), (size_t)0);
            std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return v.w[a] < v.w[b]; });
            for (size_t k = 0; k < order.size() && k < 10; ++k)
                printf("between %zu s %.17g w %.17g robust %d\n", order[k], v.s[order[k]], v.w[order[k]], (int)v.robust[order[k]]);
        }
        if (files[1]) graph.saveG2o(files[1]);
        return (r.chi2_final <= before) ? 0 : 1;
    } catch (const std::exception& e) {
        fprintf(stderr, "graph_check: %s\n", e.what());
        return 1;
    }
}
