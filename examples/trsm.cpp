// trsm.cpp — a sparse triangular solve with a block of k right-hand sides on the device, through include/g4s/csr.hpp.
//   trsm FILE.mtx [lower|upper] [k]   FILE.mtx: a MatrixMarket coordinate file (g4s/mtx.hpp) of a square matrix; only its lower (upper) triangle is
//                                     read, as in trsv.cpp. k: the number of right-hand sides (default 4).
// read_matrix_market → TriangularSolve → ONE solve of the n × k block B whose column j is (j + 1)·(T·1), T·1 summed left to right in file order, so
// that column j of X should be all j + 1. The k columns ride on the launches of one solve. Prints
//   n N, nnz_triangle Z, L levels, widest W, K launches per solve, C chains
// and then one line "i j x" per element of X, x as a hexadecimal float: every bit of it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "g4s/mtx.hpp"

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s FILE.mtx [lower|upper] [k]\n", argv[0]); return 2; }
    const bool lower = !(argc > 2 && std::strcmp(argv[2], "upper") == 0);
    const int k = argc > 3 ? std::atoi(argv[3]) : 4;
    if (k < 0 || k > G4S_TRSV_MAX_RHS) { std::fprintf(stderr, "k must be in [0, %d]\n", G4S_TRSV_MAX_RHS); return 2; }
    try {
        const auto a = g4s::read_matrix_market(argv[1]);
        const size_t n = (size_t)a.rows, kk = (size_t)k;
        std::vector<double> t1(n ? n : 1, 0.0), B(n * kk ? n * kk : 1, 0.0);
        for (int32_t i = 0; i < a.rows; ++i)
            for (int32_t e = a.rowptr[i]; e < a.rowptr[i + 1]; ++e)
                if (lower ? a.colids[e] <= i : a.colids[e] >= i) t1[(size_t)i] += a.values[e];
        for (size_t i = 0; i < n; ++i)
            for (size_t j = 0; j < kk; ++j) B[i * kk + j] = (double)(j + 1) * t1[i];
        g4s::TriangularSolve plan(a, lower);
        plan.solve(B.data(), B.data(), k);
        const g4s_trsv_info &info = plan.info();
        std::printf("n %d, nnz_triangle %lld, %d levels, widest %d, %d launches per solve, %d chains\n", info.n, (long long)info.nnz_triangle, info.levels,
                    info.widest_level, info.launches_per_solve, info.chains);
        for (size_t i = 0; i < n; ++i)
            for (size_t j = 0; j < kk; ++j) std::printf("%zu %zu %a\n", i, j, B[i * kk + j]);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
