// Host evaluation of sig_sampler::quotient, position, locate, column and lerp (signals_amd/csrc/sig_sampler.h), the text sampler.hip
// compiles for the device, for tests/test_sampler_host.py.  -O2 -ffp-contract=off, as the device code is built; the header needs
// nothing of HIP.
//
// Input, one case per line, doubles as C hexadecimal floats (or nan / inf), integers in decimal:
//   P n rate gate_on ratio offset T loop_start loop_end  -> "on u kind i j f": u = ((n / rate - gate_on) * rate) * ratio + offset, on = the
//                                                           trigger has passed, then locate(u): kind 0 silence | 1 NaN | 2 read, the two
//                                                           indices and the fraction (0 0 0 where nothing is read)
//   U u T loop_start loop_end                            -> "kind i j f": locate alone
//   C select W                                           -> "w": the column
//   L a b f                                              -> "y": a + f * (b - a)
//   S T W loop_start loop_end                            -> "ok": the table and loop rule of the C entry
// Output: one line per case, doubles as %a.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sig_sampler.h"

static void where(double u, long T, long ls, long le) {
    const sig_sampler::Shape sh = sig_sampler::shape((int)T, (int)ls, (int)le);
    int i = -1, j = -1;
    double f = -1.0;
    const int kind = le != 0 ? (int)sig_sampler::locate<true>(u, sh, i, j, f) : (int)sig_sampler::locate<false>(u, sh, i, j, f);
    printf("%d %d %d %a\n", kind, i, j, f);
}

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        char* p = line + 1;
        if (line[0] == 'P') {
            const long long n = strtoll(p, &p, 10);
            const double rate = strtod(p, &p), gate = strtod(p, &p), ratio = strtod(p, &p), offset = strtod(p, &p);
            const long T = strtol(p, &p, 10), ls = strtol(p, &p, 10), le = strtol(p, &p, 10);
            bool on = false;
            const double u = sig_sampler::position(sig_sampler::quotient((int64_t)n, rate), rate, gate, ratio, offset, on);
            printf("%d %a ", on ? 1 : 0, u);
            where(u, T, ls, le);
        } else if (line[0] == 'U') {
            const double u = strtod(p, &p);
            const long T = strtol(p, &p, 10), ls = strtol(p, &p, 10), le = strtol(p, &p, 10);
            where(u, T, ls, le);
        } else if (line[0] == 'C') {
            const double select = strtod(p, &p);
            printf("%d\n", sig_sampler::column(select, (int)strtol(p, &p, 10)));
        } else if (line[0] == 'L') {
            const double a = strtod(p, &p), b = strtod(p, &p), f = strtod(p, &p);
            printf("%a\n", sig_sampler::lerp(a, b, f));
        } else if (line[0] == 'S') {
            const long long T = strtoll(p, &p, 10), W = strtoll(p, &p, 10), ls = strtoll(p, &p, 10), le = strtoll(p, &p, 10);
            printf("%d\n", sig_sampler::shape_ok(T, W, ls, le) ? 1 : 0);
        } else if (line[0] != '\n') {
            fprintf(stderr, "bad case: %s", line);
            return 2;
        }
    }
    return 0;
}
