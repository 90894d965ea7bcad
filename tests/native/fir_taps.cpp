// Host evaluation of sig_fir::column, sig_fir::first / next and sig_fir::mac (signals_amd/csrc/sig_fir.h), the text fir.hip compiles
// for the device, for tests/test_fir_host.py.  -O2 -ffp-contract=off, as the device code is built; the header needs nothing of HIP.
//
// Input, one case per line, numbers as C hexadecimal floats (or nan / inf):
//   C select W                     -> "w":   the column clip(floor(select), 0, W - 1), NaN -> 0
//   F L h_0 .. h_{L-1} x_0 .. x_{L-1}  -> "y":   acc = h_0 * x_0, then acc = acc + h_k * x_k in ascending k (x_k stands for x[n - k])
//   K                              -> "context max_taps max_points": the header's constants
// Output: one line per case, doubles as %a.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "sig_fir.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        char* p = &line[0] + 1;
        if (line[0] == 'C') {
            const double select = strtod(p, &p);
            const int W = (int)strtol(p, &p, 10);
            printf("%d\n", sig_fir::column(select, W));
        } else if (line[0] == 'F') {
            const int L = (int)strtol(p, &p, 10);
            if (L < 1 || L > sig_fir::kMaxTaps) { fprintf(stderr, "bad length: %d\n", L); return 2; }
            std::vector<double> h(L), x(L);
            for (int k = 0; k < L; ++k) h[k] = strtod(p, &p);
            for (int k = 0; k < L; ++k) x[k] = strtod(p, &p);
            double acc = 0.0;
            for (int k = 0; k < L; ++k) acc = sig_fir::mac(k, acc, h[k], x[k]);
            printf("%a\n", acc);
        } else if (line[0] == 'K') {
            printf("%d %d %d\n", sig_fir::kContext, sig_fir::kMaxTaps, sig_fir::kMaxPoints);
        } else {
            fprintf(stderr, "bad case: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
