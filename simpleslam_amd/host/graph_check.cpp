// graph_check -- backend::PoseGraph (PCR/HipRegister.hpp) over a graph read from a g2o file, on the GPU: chi2 before, chi2 after and the
// iteration counts.  usage: graph_check graph.g2o [out.g2o] [--preconditioner block_jacobi|tree]   (block_jacobi when absent)
#include <cstdio>
#include <cstring>
#include <exception>

#include "PCR/HipRegister.hpp"

int main(int argc, char** argv) {
    int precond = PCR_GRAPH_PRECOND_BLOCK_JACOBI;
    const char* files[2] = {nullptr, nullptr};
    int n_files = 0;
    bool bad = false;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--preconditioner") && i + 1 < argc) {
            ++i;
            if (!strcmp(argv[i], "tree")) precond = PCR_GRAPH_PRECOND_TREE;
            else if (!strcmp(argv[i], "block_jacobi")) precond = PCR_GRAPH_PRECOND_BLOCK_JACOBI;
            else bad = true;
        } else if (n_files < 2 && argv[i][0] != '-') files[n_files++] = argv[i];
        else bad = true;
    }
    if (bad || n_files < 1) {
        fprintf(stderr, "usage: %s graph.g2o [out.g2o] [--preconditioner block_jacobi|tree]\n", argv[0]);
        return 2;
    }
    try {
        backend::PoseGraph graph;
        graph.loadG2o(files[0]);
        const double before = graph.chi2();
        const backend::PoseGraph::Result r = graph.optimize(precond);
        printf("poses %zu factors %zu\n", graph.poses(), graph.factors());
        printf("chi2_before %.17g\nchi2_after %.17g\n", before, r.chi2_final);
        printf("lm_iterations %d accepted %d pcg_iterations %lld pcg_capped %d converged %d lambda %g\n", r.iterations, r.accepted,
               (long long)r.pcg_iterations, r.pcg_capped, r.converged, r.lambda);
        if (files[1]) graph.saveG2o(files[1]);
        return (r.chi2_final <= before) ? 0 : 1;
    } catch (const std::exception& e) {
        fprintf(stderr, "graph_check: %s\n", e.what());
        return 1;
    }
}
