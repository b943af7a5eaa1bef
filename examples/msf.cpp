// msf.cpp — the minimum spanning forest of a weighted undirected graph on the device, through include/g4s/csr.hpp.
//   msf FILE.mtx [max]     FILE.mtx: a MatrixMarket coordinate file (g4s/mtx.hpp); every off-diagonal entry is an undirected edge, its value the
//                          weight; a "symmetric" file stores both directions, which changes nothing. "max": the maximum spanning forest.
// read_matrix_market → MinimumSpanningForest / MaximumSpanningForest. Prints
//   E edges, C components, weight W, R rounds
// and then one line "position row col value" per forest entry when the matrix has at most 64 rows.
#include <cstdio>
#include <cstring>
#include <vector>
#include "g4s/mtx.hpp"

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s FILE.mtx [max]\n", argv[0]); return 2; }
    const bool maximum = argc > 2 && std::strcmp(argv[2], "max") == 0;
    try {
        const auto a = g4s::read_matrix_market(argv[1]);
        std::vector<int32_t> edges((size_t)(a.rows > 1 ? a.rows - 1 : 1)), labels((size_t)(a.rows > 0 ? a.rows : 1));
        g4s_msf_info info = {};
        const int64_t m = maximum ? g4s::MaximumSpanningForest(a, edges.data(), labels.data(), &info) : g4s::MinimumSpanningForest(a, edges.data(), labels.data(), &info);
        std::printf("%lld edges, %lld components, weight %.17g, %d rounds\n", (long long)m, (long long)info.components, info.weight, info.rounds);
        if (a.rows <= 64) {
            int32_t row = 0;
            for (int64_t e = 0; e < m; ++e) {                       // the positions ascend, so the row only moves forward
                const int32_t k = edges[(size_t)e];
                while (a.rowptr[row + 1] <= k) ++row;
                std::printf("%d %d %d %.17g\n", k, row, a.colids[k], a.values[k]);
            }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
