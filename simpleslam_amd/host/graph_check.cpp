// graph_check -- backend::PoseGraph (PCR/HipRegister.hpp) over a graph read from a g2o file, on the GPU: chi2 before, chi2 after and the
// iteration counts.  usage: graph_check graph.g2o [out.g2o]
#include <cstdio>
#include <exception>

#include "PCR/HipRegister.hpp"

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s graph.g2o [out.g2o]\n", argv[0]);
        return 2;
    }
    try {
        backend::PoseGraph graph;
        graph.loadG2o(argv[1]);
        const double before = graph.chi2();
        const backend::PoseGraph::Result r = graph.optimize();
        printf("poses %zu factors %zu\n", graph.poses(), graph.factors());
        printf("chi2_before %.17g\nchi2_after %.17g\n", before, r.chi2_final);
        printf("lm_iterations %d accepted %d pcg_iterations %lld pcg_capped %d converged %d lambda %g\n", r.iterations, r.accepted,
               (long long)r.pcg_iterations, r.pcg_capped, r.converged, r.lambda);
        if (argc > 2) graph.saveG2o(argv[2]);
        return (r.chi2_final <= before) ? 0 : 1;
    } catch (const std::exception& e) {
        fprintf(stderr, "graph_check: %s\n", e.what());
        return 1;
    }
}
