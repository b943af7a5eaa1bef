// ilu.cpp — an ILU(0) preconditioner on the device, through include/g4s/csr.hpp.
//   ilu [NX]        NX (default 8): the five-point Laplacian of an NX × NX grid, 4 on the diagonal and −1 beside it
// CSR → ILU0 → apply with r = A·1, refactorise with the values doubled. Prints
//   n N, nnz Z, L levels, widest W, K launches per factor, C chains, P launches per apply, bad pivot B
//   defect D          max over the stored positions of |(L U)_ij − a_ij| / |a_ij|, computed on the host: an ILU(0) reproduces A on its pattern
//   refactor B        the pivot word of the factorisation of 2·A
// and then, when the grid has at most 64 points, one line "f k value" per factor value, one line "z i value" per entry of z and one line "g k value"
// per factor value of 2·A.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "g4s/csr.hpp"

int main(int argc, char **argv)
{
    const int nx = argc > 1 ? std::atoi(argv[1]) : 8;
    if (nx < 1 || nx > 4096) { std::fprintf(stderr, "usage: %s [NX], 1 <= NX <= 4096\n", argv[0]); return 2; }
    const int32_t n = nx * nx;
    std::vector<int32_t> rp(1, 0), ci;
    std::vector<double> va;
    for (int y = 0; y < nx; ++y)
        for (int x = 0; x < nx; ++x) {
            const int32_t i = y * nx + x;
            if (y > 0) { ci.push_back(i - nx); va.push_back(-1.0); }
            if (x > 0) { ci.push_back(i - 1); va.push_back(-1.0); }
            ci.push_back(i); va.push_back(4.0);
            if (x < nx - 1) { ci.push_back(i + 1); va.push_back(-1.0); }
            if (y < nx - 1) { ci.push_back(i + nx); va.push_back(-1.0); }
            rp.push_back((int32_t)ci.size());
        }
    try {
        const g4s::CSR<int32_t, double> a(rp.data(), ci.data(), va.data(), n, n, (int32_t)ci.size());
        g4s::ILU0<int32_t, double> ilu(a);
        const g4s_ilu0_info &info = ilu.info();
        std::printf("n %d, nnz %lld, %d levels, widest %d, %d launches per factor, %d chains, %d launches per apply, bad pivot %d\n", info.n, (long long)info.nnz,
                    info.levels, info.widest_level, info.launches_per_factor, info.chains, info.launches_per_apply, info.bad_pivot);
        std::vector<double> f(va.size()), r((size_t)n, 0.0), z((size_t)n, 0.0);
        ilu.factors(f.data());
        auto at = [&](int32_t i, int32_t j) {               // the position of (i, j), −1 when it is not stored
            for (int32_t k = rp[(size_t)i]; k < rp[(size_t)i + 1]; ++k)
                if (ci[(size_t)k] == j) return k;
            return (int32_t)-1;
        };
        double worst = 0.0;
        for (int32_t i = 0; i < n; ++i)
            for (int32_t q = rp[(size_t)i]; q < rp[(size_t)i + 1]; ++q) {
                const int32_t j = ci[(size_t)q];
                double s = j >= i ? f[(size_t)q] : 0.0;     // l_ii = 1
                for (int32_t p = rp[(size_t)i]; p < rp[(size_t)i + 1] && ci[(size_t)p] < i && ci[(size_t)p] <= j; ++p) {
                    const int32_t t = at(ci[(size_t)p], j);
                    if (t >= 0) s += f[(size_t)p] * f[(size_t)t];
                }
                worst = std::fmax(worst, std::fabs(s - va[(size_t)q]) / std::fabs(va[(size_t)q]));
            }
        std::printf("defect %.3g\n", worst);
        for (int32_t i = 0; i < n; ++i)
            for (int32_t k = rp[(size_t)i]; k < rp[(size_t)i + 1]; ++k) r[(size_t)i] += va[(size_t)k];
        ilu.apply(r.data(), z.data());
        std::vector<double> twice(va);
        for (double &v : twice) v *= 2.0;
        std::printf("refactor %d\n", ilu.factor(twice.data()));
        if (n <= 64) {
            for (size_t k = 0; k < f.size(); ++k) std::printf("f %zu %.17g\n", k, f[k]);
            for (int32_t i = 0; i < n; ++i) std::printf("z %d %.17g\n", i, z[(size_t)i]);
            ilu.factors(f.data());
            for (size_t k = 0; k < f.size(); ++k) std::printf("g %zu %.17g\n", k, f[k]);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
