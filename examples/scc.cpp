// scc.cpp — which vertices of a directed graph can reach each other: strongly connected components on the device, through include/g4s/csr.hpp.
//   scc EDGES     EDGES: "m n" on the first line, then m lines "start end" (a directed edge list in any order, repeats and self-loops allowed)
// FromCOO (repeats merged, rows ascending) → StronglyConnectedComponents. Prints
//   C components, largest V vertices (label L), T trimmed, pivot P (S vertices), R colouring rounds
// and then one line "v label" per vertex when n <= 64.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "g4s/csr.hpp"

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s EDGES\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    long m = 0, n = 0;
    if (std::fscanf(f, "%ld %ld", &m, &n) != 2 || m < 0 || n < 0 || n > INT32_MAX) { std::fprintf(stderr, "bad header\n"); return 2; }
    std::vector<int32_t> row((size_t)m), col((size_t)m);
    for (long e = 0; e < m; ++e)
        if (std::fscanf(f, "%d %d", &row[(size_t)e], &col[(size_t)e]) != 2) { std::fprintf(stderr, "bad edge %ld\n", e); return 2; }
    std::fclose(f);
    try {
        g4s::CSR<int32_t, double> a;
        g4s::FromCOO<int32_t, double>((int32_t)n, (int32_t)n, (int64_t)m, row.data(), col.data(), nullptr, a, G4S_COMBINE_MAX);
        std::vector<int32_t> labels((size_t)n);
        g4s_scc_info info = {};
        g4s::StronglyConnectedComponents(a, labels.data(), &info);
        std::printf("%lld components, largest %lld vertices (label %d), %d trimmed, pivot %d (%d vertices), %d colouring rounds\n", (long long)info.components,
                    (long long)info.largest, info.largest_label, info.trimmed, info.pivot, info.pivot_size, info.color_rounds);
        if (n <= 64)
            for (long v = 0; v < n; ++v) std::printf("%ld %d\n", v, labels[(size_t)v]);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
