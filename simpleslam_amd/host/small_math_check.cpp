// small_math_check -- pcr::t2se3 and pcr::se3_exp (csrc/small_math.h, the __host__ __device__ routines the LOAM kernel's tail and the pose graph call)
// on the CPU: the header's own code, compiled for the host, no GPU call.  Reads records from stdin, runs the routine, prints the result with
// %.17g.  Built with -Xarch_host -fsanitize=address,undefined it is the checked run of the two routines.
//
// stdin, one record per line:
//   "t2se3" and 16 numbers: a 4x4 pose, row by row   ->  "t2se3" and the 16 numbers of the pose after pcr::t2se3, row by row
//   "exp" and 6 numbers: a twist [rho; omega]        ->  "exp" and the 16 numbers of pcr::se3_exp of it, row by row
#include <cstdio>
#include <cstring>

#include "../csrc/small_math.h"

static void print_rows(const char* tag, const double* col_major) {
    printf("%s", tag);
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) printf(" %.17g", col_major[c * 4 + r]);
    printf("\n");
}

int main() {
    char tag[16];
    int line = 0;
    while (scanf("%15s", tag) == 1) {
        ++line;
        if (!strcmp(tag, "t2se3")) {
            double rows[16], T[16];
            for (int i = 0; i < 16; ++i)
                if (scanf("%lf", &rows[i]) != 1) { fprintf(stderr, "small_math_check: record %d: a pose needs 16 numbers\n", line); return 2; }
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < 4; ++c) T[c * 4 + r] = rows[r * 4 + c];
            pcr::t2se3(T);
            print_rows("t2se3", T);
        } else if (!strcmp(tag, "exp")) {
            double k[6], T[16];
            for (int i = 0; i < 6; ++i)
                if (scanf("%lf", &k[i]) != 1) { fprintf(stderr, "small_math_check: record %d: a twist needs 6 numbers\n", line); return 2; }
            pcr::se3_exp(k, T);
            print_rows("exp", T);
        } else {
            fprintf(stderr, "small_math_check: record %d: unknown routine '%s'\n", line, tag);
            return 2;
        }
    }
    return 0;
}
