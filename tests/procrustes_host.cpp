// Stand-alone host program around the Procrustes routine of csrc/pose_metrics.hip (it is __host__ __device__ for this purpose):
// reads 3 x 3 matrices H (row-major, nine numbers per line) from standard input and prints tr(S D) and R (row-major) per line.
// Built and run by tests/test_pose_procrustes_cpu.py, with the host sanitizers on.
#include "../multiply_amd/csrc/pose_metrics.hip"
#include <cstdio>

int main() {
    double H[9];
    while (scanf("%lf %lf %lf %lf %lf %lf %lf %lf %lf", H, H + 1, H + 2, H + 3, H + 4, H + 5, H + 6, H + 7, H + 8) == 9) {
        double R[9], tr;
        procrustes(H, R, tr);
        printf("%.17g", tr);
        for (int i = 0; i < 9; ++i) printf(" %.17g", R[i]);
        printf("\n");
    }
    return 0;
}
