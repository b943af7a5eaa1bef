// graph_to_csr.cpp — the reference's edge list (mm/inc/graph.h) to a CSR on the device, through include/g4s/csr.hpp.
//   graph_to_csr EDGES      EDGES: "m n" on the first line, then m lines "start end w" (a directed edge start → end with an integer weight)
// Prints two matrices, each as four lines (rows cols nnz / rowptr / colids / values with 17 digits):
//   1. FromGraph(g, keep, G4S_DUP_KEEP) — every edge an entry, each source's edges in ascending target, repeats in input order;
//   2. SortAndMerge(keep, c)           — repeats summed: what the reference's CSR(graph&) builds (mm/inc/CSR.h:255-329), and FromGraph(g, c) itself.
// Exit status 1 when FromGraph(g, c) and SortAndMerge disagree.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "g4s/csr.hpp"

static void print(const g4s::CSR<int32_t, double> &a)
{
    std::printf("%d %d %d\n", a.rows, a.cols, a.nnz);
    for (int32_t r = 0; r <= a.rows; ++r) std::printf("%d ", a.rowptr[r]);
    std::printf("\n");
    for (int32_t k = 0; k < a.nnz; ++k) std::printf("%d ", a.colids[k]);
    std::printf("\n");
    for (int32_t k = 0; k < a.nnz; ++k) std::printf("%.17g ", a.values[k]);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s EDGES\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    long m = 0, n = 0;
    if (std::fscanf(f, "%ld %ld", &m, &n) != 2 || m < 0 || n < 0) { std::fprintf(stderr, "bad header\n"); return 2; }
    std::vector<long> start(m), end(m);
    std::vector<double> w(m);
    for (long e = 0; e < m; ++e)
        if (std::fscanf(f, "%ld %ld %lf", &start[e], &end[e], &w[e]) != 3) { std::fprintf(stderr, "bad edge %ld\n", e); return 2; }
    std::fclose(f);
    try {
        const g4s::graph g = {m, n, start.data(), end.data(), w.data()};
        g4s::CSR<int32_t, double> keep, merged, direct;
        g4s_coo_info info = {};
        g4s::FromGraph(g, keep, G4S_DUP_KEEP, &info);
        g4s::SortAndMerge(keep, merged);
        g4s::FromGraph(g, direct);
        print(keep);
        print(merged);
        std::printf("longest_run %lld\n", (long long)info.longest_run);
        bool same = merged.nnz == direct.nnz && merged.rows == direct.rows;
        for (int32_t r = 0; same && r <= merged.rows; ++r) same = merged.rowptr[r] == direct.rowptr[r];
        for (int32_t k = 0; same && k < merged.nnz; ++k) same = merged.colids[k] == direct.colids[k] && merged.values[k] == direct.values[k];
        if (!same) { std::fprintf(stderr, "FromGraph and SortAndMerge disagree\n"); return 1; }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
