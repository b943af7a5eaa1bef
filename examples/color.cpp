// color.cpp — how few colours a graph needs at most: the smallest-last greedy colouring on the device, through include/g4s/csr.hpp.
//   color EDGES     EDGES: "m n" on the first line, then m lines "start end" (an undirected edge list in any order, repeats and self-loops allowed)
// FromCOO (repeats merged, rows ascending) → Symmetrise (the pattern of the undirected graph) → KCore (the peel round is the key of the smallest-last
// order) → GreedyColor. Prints
//   C colours (degeneracy + 1 = D), independent set of S vertices, R rounds
// and then one line "v colour round" per vertex when n <= 64.
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
        g4s::CSR<int32_t, double> a, s;
        g4s::FromCOO<int32_t, double>((int32_t)n, (int32_t)n, (int64_t)m, row.data(), col.data(), nullptr, a, G4S_COMBINE_MAX);
        g4s::Symmetrise(a, s);
        std::vector<int32_t> core((size_t)n), peel((size_t)n), color((size_t)n), round((size_t)n);
        g4s_kcore_info kinfo = {};
        g4s::KCore(s, core.data(), peel.data(), INT32_MAX, &kinfo);
        g4s_color_info info = {};
        g4s::GreedyColor(s, color.data(), peel.data(), 0, round.data(), false, &info);
        std::printf("%d colours (degeneracy + 1 = %d), independent set of %lld vertices, %d rounds\n", info.colors, kinfo.degeneracy + 1, (long long)info.class0,
                    info.rounds);
        if (n <= 64)
            for (long v = 0; v < n; ++v) std::printf("%ld %d %d\n", v, color[(size_t)v], round[(size_t)v]);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
