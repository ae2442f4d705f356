// Stand-alone host program around the Gauss-Newton step of csrc/reg_solve.hpp (it is __host__ __device__ for this purpose).  Per
// case it reads from standard input: similarity (0 / 1), reject, tol, the MP_REG_SLOT summed slot values and the MP_REG_STATE state
// values; it prints one line: the flag reg_step returned, delta [7] and the new state.  Built and run by
// tests/test_registration_cpu.py, with the host sanitizers on.
#include "../multiply_amd/csrc/reg_solve.hpp"
#include <cstdio>

int main() {
    int similarity;
    double reject, tol;
    while (scanf("%d %lf %lf", &similarity, &reject, &tol) == 3) {
        double sums[MP_REG_SLOT], st[MP_REG_STATE], delta[7];
        for (int i = 0; i < MP_REG_SLOT; ++i)
            if (scanf("%lf", sums + i) != 1) return 2;
        for (int i = 0; i < MP_REG_STATE; ++i)
            if (scanf("%lf", st + i) != 1) return 2;
        const int flag = reg_step(sums, similarity, reject, tol, st, delta);
        printf("%d", flag);
        for (int i = 0; i < 7; ++i) printf(" %.17g", delta[i]);
        for (int i = 0; i < MP_REG_STATE; ++i) printf(" %.17g", st[i]);
        printf("\n");
    }
    return 0;
}
