// ktruss.cpp — how tightly the edges of a graph are knit: truss numbers on the device, through include/g4s/csr.hpp.
//   ktruss EDGES     EDGES: "m n" on the first line, then m lines "start end" (an undirected edge list in any order, repeats and self-loops allowed)
// FromCOO (repeats merged, rows ascending) → Symmetrise (the pattern of the undirected graph) → KTruss. Prints
//   T triangles, max truss K on E edges, L levels, R rounds
// and then one line "u v truss round support" per undirected edge when n <= 64.
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
        std::vector<int32_t> truss((size_t)s.nnz), round((size_t)s.nnz), support((size_t)s.nnz);
        g4s_ktruss_info info = {};
        g4s::KTruss(s, truss.data(), round.data(), support.data(), INT32_MAX, &info);
        std::printf("%lld triangles, max truss %d on %lld edges, %d levels, %d rounds\n", (long long)info.triangles, info.max_truss,
                    (long long)info.top_truss_edges, info.levels, info.rounds);
        if (n <= 64)
            for (int32_t u = 0; u < s.rows; ++u)
                for (int32_t p = s.rowptr[u]; p < s.rowptr[u + 1]; ++p)
                    if (s.colids[p] > u) std::printf("%d %d %d %d %d\n", u, s.colids[p], truss[(size_t)p], round[(size_t)p], support[(size_t)p]);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
