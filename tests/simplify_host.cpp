// Stand-alone host program around the cell representative of csrc/quadric_solve.hpp (it is __host__ __device__ for this purpose).
// Per case it reads from standard input: A (6, packed upper triangle), b (3), mean (3), lam, half; it prints one line: whether it
// solved (1) or took the mean (0), x [3] after the clamp, x [3] before it.  Built and run by tests/test_mesh_simplify_cpu.py, with
// the host sanitizers on.
#include "../multiply_amd/csrc/quadric_solve.hpp"
#include <cstdio>

int main() {
    double in[14];
    while (scanf("%lf", in) == 1) {
        for (int i = 1; i < 14; ++i)
            if (scanf("%lf", in + i) != 1) return 2;
        double x[3], x_free[3];
        const int solved = quadric_point(in, in + 6, in + 9, in[12], in[13], x, x_free);
        printf("%d %.17g %.17g %.17g %.17g %.17g %.17g\n", solved, x[0], x[1], x[2], x_free[0], x_free[1], x_free[2]);
    }
    return 0;
}
