// trsv.cpp — a sparse triangular solve on the device, through include/g4s/csr.hpp.
//   trsv FILE.mtx [upper]   FILE.mtx: a MatrixMarket coordinate file (g4s/mtx.hpp) of a square matrix; only its lower (upper) triangle is read, so the
//                           file may hold a whole matrix A: the solve is then the (D + L) x = b of a Gauss–Seidel sweep on A.
// read_matrix_market → TriangularSolve → solve with b = T·1, so that x should be all ones. Prints
//   n N, nnz_triangle Z, L levels, widest W, K launches per solve, C chains
//   residual R        max_i |b − T x|_i / (|T||x|)_i, computed on the host
// and then one line "i level x" per row when the matrix has at most 64 rows.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "g4s/mtx.hpp"

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s FILE.mtx [upper]\n", argv[0]); return 2; }
    const bool lower = !(argc > 2 && std::strcmp(argv[2], "upper") == 0);
    try {
        const auto a = g4s::read_matrix_market(argv[1]);
        const size_t n = (size_t)a.rows;
        auto in_triangle = [&](int32_t i, int32_t c) { return lower ? c <= i : c >= i; };
        std::vector<double> b(n ? n : 1, 0.0), x(n ? n : 1, 0.0);
        std::vector<int32_t> level(n ? n : 1, 0);
        for (int32_t i = 0; i < a.rows; ++i)
            for (int32_t k = a.rowptr[i]; k < a.rowptr[i + 1]; ++k)
                if (in_triangle(i, a.colids[k])) b[(size_t)i] += a.values[k];
        g4s::TriangularSolve plan(a, lower, false, level.data());
        plan.solve(b.data(), x.data());
        const g4s_trsv_info &info = plan.info();
        std::printf("n %d, nnz_triangle %lld, %d levels, widest %d, %d launches per solve, %d chains\n", info.n, (long long)info.nnz_triangle, info.levels,
                    info.widest_level, info.launches_per_solve, info.chains);
        double worst = 0.0;
        for (int32_t i = 0; i < a.rows; ++i) {
            double r = b[(size_t)i], scale = 0.0;
            for (int32_t k = a.rowptr[i]; k < a.rowptr[i + 1]; ++k)
                if (in_triangle(i, a.colids[k])) {
                    r -= a.values[k] * x[(size_t)a.colids[k]];
                    scale += std::fabs(a.values[k] * x[(size_t)a.colids[k]]);
                }
            if (scale > 0.0) worst = std::fmax(worst, std::fabs(r) / scale);
        }
        std::printf("residual %.3g\n", worst);
        if (a.rows <= 64)
            for (int32_t i = 0; i < a.rows; ++i) std::printf("%d %d %.17g\n", i, level[(size_t)i], x[(size_t)i]);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
