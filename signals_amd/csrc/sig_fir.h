// The arithmetic of the dense FIR filter (chain/ext.py FIR, fir.hip), one text for the device and for the host program of
// tests/native/fir_taps.cpp: it includes nothing of HIP.  f64, every operation rounded (built with -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SIG_FIR_FN __host__ __device__ __forceinline__
#else
#define SIG_FIR_FN inline
#endif

namespace sig_fir {

constexpr int kContext = 100;        // rows of context in front of a block: the filters' window
constexpr int kMaxTaps = 101;        // x[n - 100] .. x[n]: every row of that window and the sample itself
constexpr int kMaxPoints = 4096;     // taps x columns of one table

// the column a `select` value picks: clip(floor(select), 0, W - 1); NaN -> 0, -0 -> 0, +inf -> W - 1, -inf -> 0
SIG_FIR_FN int column(double select, int W) {
    const double s = floor(select);
    return (s >= 1.0) ? ((s >= (double)(W - 1)) ? W - 1 : (int)s) : 0;
}

// acc = h[0] * x[n]: the first product is the sum's first value, not added to a zero (0 + -0 is +0)
SIG_FIR_FN double first(double h, double x) { return h * x; }

// acc = acc + h[k] * x[n - k], k >= 1 ascending: the product rounded, then the sum rounded
SIG_FIR_FN double next(double acc, double h, double x) {
    const double p = h * x;
    return acc + p;
}

// the multiply-accumulate step of tap k
SIG_FIR_FN double mac(int k, double acc, double h, double x) { return k == 0 ? first(h, x) : next(acc, h, x); }

}  // namespace sig_fir
