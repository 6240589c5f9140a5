// TEST INFRASTRUCTURE: the scalar fp64 routines of buffer_amd/csrc/pose_math.h compiled for the host and run on a file of cases
// (tests/test_pose_math_cpu.py writes the cases and holds the float64 references).  Built with a plain host compiler:
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -D__host__= -D__device__= pose_math_host.cpp -o pose_math_host
// and once more with -fsanitize=address,undefined.
//   pose_math_host <cases> <results>
// cases:   float64 rows of 28: [0] the routine (0 kabsch_rotation, 1 solve6, 2 rot_zyx), [1..27] its input
//          (kabsch: H 9 row-major; solve6: upper triangle 21, g 6; rot_zyx: x 6)
// results: float64 rows of 10: [0] the routine's return value (1 / 0; rot_zyx: 1), [1..9] its output (kabsch: R, preset to 7 so
//          that an untouched R shows; solve6: x 6; rot_zyx: R)
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../buffer_amd/csrc/pose_math.h"

#define IN_W 28
#define OUT_W 10

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <cases> <results>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % (long)(IN_W * sizeof(double)) != 0) { fprintf(stderr, "%s: not rows of %d doubles\n", argv[1], IN_W); return 2; }
    const size_t n = (size_t)bytes / (IN_W * sizeof(double));
    std::vector<double> in(n * IN_W), out(n * OUT_W, 0.0);
    if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) { fprintf(stderr, "%s: short read\n", argv[1]); return 2; }
    fclose(f);
    for (size_t i = 0; i < n; i++) {
        const double* c = in.data() + i * IN_W;
        double* r = out.data() + i * OUT_W;
        const int kind = (int)c[0];
        if (kind == 0) {
            for (int k = 0; k < 9; k++) r[1 + k] = 7.0;
            r[0] = kabsch_rotation(c + 1, r + 1) ? 1.0 : 0.0;
        } else if (kind == 1) {
            double x[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
            r[0] = solve6(c + 1, c + 22, x) ? 1.0 : 0.0;
            for (int k = 0; k < 6; k++) r[1 + k] = x[k];
        } else if (kind == 2) {
            rot_zyx(c + 1, r + 1);
            r[0] = 1.0;
        } else {
            fprintf(stderr, "case %zu: unknown routine %d\n", i, kind);
            return 2;
        }
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { fprintf(stderr, "%s: short write\n", argv[2]); return 2; }
    fclose(f);
    return 0;
}
