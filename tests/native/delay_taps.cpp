// Host evaluation of sig_delay::tap, sig_delay::read and sig_delay::add (signals_amd/csrc/sig_delay.h), the text delay.hip compiles for
// the device, for tests/test_delay_host.py.  -O2 -ffp-contract=off, as the device code is built; the header needs nothing of HIP.
//
// Input, one case per line, numbers as C hexadecimal floats (or nan / inf):
//   T t rate m              -> "ok i f":  d = clip((t * rate) * m, 0, 99) = i + f; ok = 0 for a NaN d (i = 0, f = 0 then)
//   S u acc g x0 x1 f       -> "y":       tap u's term added to acc, y = (u == 0 ? g * s : acc + g * s), s = x0 + f * (x1 - x0)
// Output: one line per case, doubles as %a.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sig_delay.h"

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        char* p = line + 1;
        if (line[0] == 'T') {
            const double t = strtod(p, &p), rate = strtod(p, &p), m = strtod(p, &p);
            int i = -1;
            double f = -1.0;
            const bool ok = sig_delay::tap(t, rate, m, i, f);
            printf("%d %d %a\n", ok ? 1 : 0, i, f);
        } else if (line[0] == 'S') {
            const int u = (int)strtol(p, &p, 10);
            const double acc = strtod(p, &p), g = strtod(p, &p), x0 = strtod(p, &p), x1 = strtod(p, &p), f = strtod(p, &p);
            printf("%a\n", sig_delay::add(u, acc, g, sig_delay::read(x0, x1, f)));
        } else if (line[0] != '\n') {
            fprintf(stderr, "bad case: %s", line);
            return 2;
        }
    }
    return 0;
}
