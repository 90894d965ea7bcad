// The tap arithmetic of the short delay line (chain/ext.py Delay, delay.hip), one text for the device and for the host program of
// tests/native/delay_taps.cpp: it includes nothing of HIP.  f64, every operation rounded (built with -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SIG_DELAY_FN __host__ __device__ __forceinline__
#else
#define SIG_DELAY_FN inline
#endif

namespace sig_delay {

constexpr int kContext = 100;        // rows of context in front of a block: the filters' window
constexpr int kMaxFrames = 99;       // the longest delay: the context minus the one further row the interpolation reads
constexpr int kMaxTaps = 16;

// One tap of one voice in one block: d = clip((t * rate) * m, 0, 99), i = floor(d), f = d - i.  False: d is NaN, and then i = 0 and
// f = 0 -- no index is formed from a NaN; the caller answers NaN for the voice's rows.
SIG_DELAY_FN bool tap(double t, double rate, double m, int& i, double& f) {
    const double d = (t * rate) * m;
    const double c = (d < 0.0) ? 0.0 : ((d > (double)kMaxFrames) ? (double)kMaxFrames : d);   // np.clip: NaN stays NaN
    const bool ok = (c == c);
    const double whole = ok ? floor(c) : 0.0;
    i = (int)whole;                  // 0 .. 99
    f = ok ? c - whole : 0.0;        // in [0, 1)
    return ok;
}

// the interpolated read between x0 = x[n - i] and x1 = x[n - i - 1]
SIG_DELAY_FN double read(double x0, double x1, double f) { return x0 + f * (x1 - x0); }

// out = g_0 * s_0, then + g_u * s_u in ascending u
SIG_DELAY_FN double add(int u, double acc, double g, double s) {
    const double p = g * s;
    return u == 0 ? p : acc + p;
}

}  // namespace sig_delay
