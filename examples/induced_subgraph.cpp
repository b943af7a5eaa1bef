// induced_subgraph.cpp — a part of a graph and a relabelling of it on the device, through include/g4s/csr.hpp.
//   induced_subgraph EDGES IDS     EDGES: "m n" on the first line, then m lines "start end w" (the reference's edge list, mm/inc/graph.h)
//                                  IDS:   "k" on the first line, then k vertex ids in any order, repeats allowed
// Prints two matrices, each as four lines (rows cols nnz / rowptr / colids / values with 17 digits):
//   1. Extract(a, ids, ids)        — the subgraph induced by ids: vertex ids[p] of the graph is vertex p of the result;
//   2. Permute(a, n − 1 … 0)       — the whole graph with its vertices numbered backwards.
// a is FromGraph(g, a): repeats summed, rows ascending. Exit status 1 when the values of 1. are not a.values[src] for the src Extract hands back.
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
    if (argc < 3) { std::fprintf(stderr, "usage: %s EDGES IDS\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    long m = 0, n = 0;
    if (std::fscanf(f, "%ld %ld", &m, &n) != 2 || m < 0 || n < 0) { std::fprintf(stderr, "bad header\n"); return 2; }
    std::vector<long> start(m), end(m);
    std::vector<double> w(m);
    for (long e = 0; e < m; ++e)
        if (std::fscanf(f, "%ld %ld %lf", &start[e], &end[e], &w[e]) != 3) { std::fprintf(stderr, "bad edge %ld\n", e); return 2; }
    std::fclose(f);
    f = std::fopen(argv[2], "r");
    if (!f) { std::perror(argv[2]); return 2; }
    long k = 0;
    if (std::fscanf(f, "%ld", &k) != 1 || k < 0) { std::fprintf(stderr, "bad id count\n"); return 2; }
    std::vector<int32_t> ids(k);
    for (long i = 0; i < k; ++i)
        if (std::fscanf(f, "%d", &ids[i]) != 1) { std::fprintf(stderr, "bad id %ld\n", i); return 2; }
    std::fclose(f);
    try {
        const g4s::graph g = {m, n, start.data(), end.data(), w.data()};
        g4s::CSR<int32_t, double> a;
        g4s::FromGraph(g, a);
        std::vector<int32_t> src, backwards((size_t)n);
        for (long v = 0; v < n; ++v) backwards[(size_t)v] = (int32_t)(n - 1 - v);
        const g4s::CSR<int32_t, double> sub = g4s::Extract(a, ids, ids, &src);
        const g4s::CSR<int32_t, double> rev = g4s::Permute(a, backwards);
        print(sub);
        print(rev);
        bool same = src.size() == (size_t)sub.nnz;
        for (int32_t x = 0; same && x < sub.nnz; ++x) same = sub.values[x] == a.values[src[(size_t)x]] && a.colids[src[(size_t)x]] == ids[(size_t)sub.colids[x]];
        if (!same) { std::fprintf(stderr, "src does not lead back to the entries of the graph\n"); return 1; }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
