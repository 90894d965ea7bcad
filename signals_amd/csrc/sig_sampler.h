// The read-position arithmetic and the neighbour rule of the sample-playback node (chain/ext.py Sampler, sampler.hip), one text for
// the device and for the host program of tests/native/sampler_index.cpp: it includes nothing of HIP.  f64, every operation rounded
// (built with -ffp-contract=off).  For absolute frame n and one voice:
//   q = n / rate;  e = q - gate_on;  s = e * rate;  u = s * ratio + offset
//   not (e >= 0) -> silence;  u NaN or +-inf -> NaN (no index is formed from it)
//   no loop:  u < 0 or u > T - 1 -> silence;  i = floor(u); f = u - i; j = min(i + 1, T - 1)
//   loop:     u < 0 -> silence;  L = loop_end - loop_start;  u >= loop_end: d = u - loop_start; c = floor(d / L);
//             u = (d - c * L) + loop_start, and loop_start where that rounds to >= loop_end (or, from 2^53 frames on, where the
//             rounded quotient exceeds the true one and the remainder falls below loop_start);
//             i = floor(u); f = u - i; j = (i + 1 >= loop_end) ? loop_start : i + 1
//   out = tbl[i] + f * (tbl[j] - tbl[i])
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SIG_SAMPLER_FN __host__ __device__ __forceinline__
#else
#define SIG_SAMPLER_FN inline
#endif

namespace sig_sampler {

constexpr int64_t kMaxPoints = (int64_t)1 << 26;     // frames x recordings of one table

enum Kind { kSilence = 0, kNaN = 1, kRead = 2 };

// what a launch knows of the table and the loop: loop_end == 0 means no loop, else 0 <= loop_start < loop_end <= T
struct Shape {
    int T, loop_start, loop_end;
    double last, lo, hi, len;                        // T - 1, loop_start, loop_end, loop_end - loop_start as doubles
};

SIG_SAMPLER_FN Shape shape(int T, int loop_start, int loop_end) {
    return Shape{T, loop_start, loop_end, (double)(T - 1), (double)loop_start, (double)loop_end, (double)(loop_end - loop_start)};
}

SIG_SAMPLER_FN bool shape_ok(int64_t T, int64_t W, int64_t loop_start, int64_t loop_end) {
    if (T < 2 || W < 1 || T > kMaxPoints || W > kMaxPoints || T * W > kMaxPoints) return false;
    return loop_end == 0 ? loop_start >= 0 : (0 <= loop_start && loop_start < loop_end && loop_end <= T);
}

// osc.py's order: frame_range / rate, one IEEE divide
SIG_SAMPLER_FN double quotient(int64_t n, double rate) { return (double)n / rate; }

// the column a `select` value picks: clip(floor(select), 0, W - 1), NaN -> 0 (Wavetable's rule)
SIG_SAMPLER_FN int column(double select, int W) {
    const double s = floor(select);
    return (s >= 1.0) ? ((s >= (double)(W - 1)) ? W - 1 : (int)s) : 0;
}

// the read position u of one sample; `on` false: before the trigger (a NaN gate included), u is not to be used
SIG_SAMPLER_FN double position(double q, double rate, double gate_on, double ratio, double offset, bool& on) {
    const double e = q - gate_on;
    const double s = e * rate;
    on = (e >= 0.0);
    return s * ratio + offset;                       // two roundings
}

// where u reads: kRead with 0 <= i, j < T and f in [0, 1); otherwise i = j = 0, f = 0 and nothing is to be read
template <bool LOOP>
SIG_SAMPLER_FN Kind locate(double u, const Shape& sh, int& i, int& j, double& f) {
    i = 0; j = 0; f = 0.0;
    if (!(fabs(u) < (double)INFINITY)) return kNaN;  // NaN, +inf, -inf
    if (u < 0.0) return kSilence;
    if (LOOP) {
        if (u >= sh.hi) {
            const double d = u - sh.lo;
            const double c = floor(d / sh.len);
            u = (d - c * sh.len) + sh.lo;
            if (!(u >= sh.lo && u < sh.hi)) u = sh.lo;
        }
    } else if (u > sh.last) {
        return kSilence;
    }
    const double whole = floor(u);
    int at = (int)whole;
    const int top = LOOP ? sh.loop_end - 1 : sh.T - 1;
    at = at < 0 ? 0 : (at > top ? top : at);               // (holds already by the lines above; keeps every index inside the table)
    f = u - whole;
    i = at;
    j = LOOP ? ((at + 1 >= sh.loop_end) ? sh.loop_start : at + 1) : ((at + 1 < sh.T) ? at + 1 : sh.T - 1);
    return kRead;
}

// the interpolated read between a = tbl[i] and b = tbl[j]
SIG_SAMPLER_FN double lerp(double a, double b, double f) { return a + f * (b - a); }

}  // namespace sig_sampler
