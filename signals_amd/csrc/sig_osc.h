// Oscillator waveforms shared by osc_bank.hip and the fused kernels (sig_fused_*.h): `t` (cycles, f64) -> sample.
// Reference: src/signals/chain/osc.py:40-62.  See osc_bank.hip for the precision notes.
#pragma once
#include "sig_common.h"

namespace sig_osc {

constexpr double kPi = 3.141592653589793115997963468544185161590576171875;   // np.pi
constexpr double kPiTail = 1.2246467991473532e-16;                            // pi - fl(pi)
constexpr double kTwoPiHi = 6.28318530717958623199592693708837032318115234375;
constexpr double kTwoPiLo = 2.4492935982947064e-16;

// sin(x) for |x| <= pi/2 + eps, odd Taylor polynomial through x^21 (remainder < 2e-18).
__device__ __forceinline__ double sin_poly(double x) {
    const double s = x * x;
    double p = -1.9572941063391263e-20;                 // -1/21!
    p = fma(p, s, 8.2206352466243295e-18);              //  1/19!
    p = fma(p, s, -2.8114572543455206e-15);             // -1/17!
    p = fma(p, s, 7.6471637318198164e-13);              //  1/15!
    p = fma(p, s, -1.6059043836821613e-10);             // -1/13!
    p = fma(p, s, 2.5052108385441720e-08);              //  1/11!
    p = fma(p, s, -2.7557319223985893e-06);             // -1/9!
    p = fma(p, s, 1.9841269841269841e-04);              //  1/7!
    p = fma(p, s, -8.3333333333333332e-03);             // -1/5!
    p = fma(p, s, 1.6666666666666666e-01);              //  1/3!   (sign folded below)
    // sin x = x - x^3/6 + ... ; the chain above carries alternating signs starting at +1/3!
    return fma(-(x * s), p, x);
}

// np.sin(t * 2 * np.pi) reproduced including the reference's own argument rounding:
//   a = fl(fl(2t) * fl(pi)) = fl(t * 2fl(pi)) is what numpy hands to libm;  a = 2*pi*t - s  with
//   s = (t*2fl(pi) - a) + t*2(pi - fl(pi)); the first term is exact via fma.
// So sin(a) = sin(2*pi*(t - K/2) + pi*K - s) with K = rint(2t): rq = t - K/2 is exact in f64, |rq| <= 1/4,
// and an odd K flips the sign.  K and its parity come from one magic-number add (RNE to an integer in the
// low mantissa bits), valid for |t| < 2^50 cycles -- beyond that f64 has no fraction bits left anyway.
constexpr double kRoundMagic = 6755399441055744.0;      // 1.5 * 2^52
constexpr double kTwoPi = 2.0 * kPi;                     // exact doubling of fl(pi)
constexpr double kTwoPiTail = 2.0 * kPiTail;

struct SinePhase { double rq; double s; unsigned flip; };   // quarter-range revolutions, -(delta), sign bit

__device__ __forceinline__ SinePhase sine_phase(double t) {
    SinePhase p;
    const double a = t * kTwoPi;
    const double e = fma(t, kTwoPi, -a);                // a + e == t * 2fl(pi) exactly
    p.s = fma(t, kTwoPiTail, e);
    const double u = fma(t, 2.0, kRoundMagic);          // = fl(2t + M): low mantissa bits = rint(2t)
    const double k = u - kRoundMagic;                   // exact
    p.rq = fma(k, -0.5, t);                             // exact, |rq| <= 0.25
    p.flip = ((unsigned)__double2loint(u) & 1u) << 31;  // parity of K
    return p;
}

// f64 store path (block-rate control values): polynomial on [-pi/2, pi/2], ~1 ulp(f64)
__device__ __forceinline__ double osc_sine(double t) {
    const SinePhase p = sine_phase(t);
    const double x = fma(p.rq, kTwoPiHi, fma(p.rq, kTwoPiLo, -p.s));
    const double y = sin_poly(x);
    return __hiloint2double(__double2hiint(y) ^ (int)p.flip, __double2loint(y));
}

__device__ __forceinline__ double osc_square(double t) {       // osc.py:48-49
    return sig_sign(0.5 - sig_npmod_pow2<1>(t));
}

__device__ __forceinline__ double osc_sawtooth(double t) {     // osc.py:54-55
    return fma(sig_npmod_pow2<1>(t - 0.5), 2.0, -1.0);     // 2m is exact: the same single rounding as 2*m - 1
}

__device__ __forceinline__ double osc_triangle(double t) {     // osc.py:60-62
    const double u = t - 0.25;
    return (4.0 * sig_npmod_pow2<2>(u) - 1.0) * sig_sign(sig_npmod_pow2<1>(u) - 0.5);
}

// f32 store path of Sine: same exact phase reduction, then the hardware sine (v_sin_f32 takes
// REVOLUTIONS; measured max |err| 1.07e-7 on [-0.25, 0.25]).  Total error vs the reference
// <= 1.3e-7 (bar 1e-6), at ~13 f64-rate ops per sample instead of 27, which is what makes the oscillator
// kernel HBM-write-bound instead of f64-VALU-bound.
constexpr double kInvTwoPi = 0.15915494309189535;
__device__ __forceinline__ float osc_sine_f32(double t) {
    const SinePhase p = sine_phase(t);
    const float rev = (float)fma(p.s, -kInvTwoPi, p.rq);
    return __uint_as_float(__float_as_uint(__builtin_amdgcn_sinf(rev)) ^ p.flip);
}

// Fast Sine phase for f64-issue-bound kernels that walk consecutive rows: within a chunk of rows the phase
// advances by d = hertz/rate revolutions per row, so  t_j ~ t_0 + j*d  and only frac(t_0) (exact) and d are
// needed.  Relative to the exact path this drops (a) the tracking of numpy's own argument rounding,
// |fl(t*2pi) - 2pi*t| <= 9.4e-16*|t| rad, and (b) the roundings inside fl(fl(n/rate)*hertz)+phase, <= ulp(t)
// cycles: together <= 3 |t| 2^-53 cycles = 2.1e-15 |t| rad per row of reference rounding noise that the incremental
// phase does not reproduce, plus the same bound once more for the seed (which carries the reference's rounding at the
// span's first row): < 2.9e-7 while |t| < 2^26 cycles, a third of the 1e-6 bar, which the caller checks per wave
// (kSineFastMaxT); beyond that the exact path is used.  f_j = fma(j, d, f0) is a single rounding from exact operands.
constexpr double kSineFastMaxT = 67108864.0;            // 2^26 cycles (10.6 h at 1760 Hz, 56 min at 20 kHz)

__device__ __forceinline__ float osc_sine_f32_fast(double f0, double d, double j) {
    const double f = fma(j, d, f0);                     // |f| <= 0.5 + 64*0.5
    const double u = fma(f, 2.0, kRoundMagic);
    const double k = u - kRoundMagic;
    const float rev = (float)fma(k, -0.5, f);           // |rev| <= 0.25
    const unsigned flip = ((unsigned)__double2loint(u) & 1u) << 31;
    return __uint_as_float(__float_as_uint(__builtin_amdgcn_sinf(rev)) ^ flip);
}

// Sawtooth for the fused kernels, whose oscillator sample feeds an f64 filter: m = t' - floor(t') as ONE instruction
// (v_fract_f64).  It differs from sig_npmod_pow2 only where the rounded subtraction would reach 1.0 (t' in (-2^-54, 0)):
// v_fract_f64 answers the largest double below 1 instead, 2.2e-16 away in the sample; the per-node oscillator kernel, whose
// float32 output is compared bit for bit, keeps the two-instruction form.
__device__ __forceinline__ double osc_sawtooth_fract(double t) {
    return fma(__builtin_amdgcn_fract(t - 0.5), 2.0, -1.0);
}

// Square for the fused kernels: sign(d), d = 0.5 - m, as copysign(1, d) (one v_and_or_b32 on the high word) kept where
// |d| > 0 and d itself (a zero, or a NaN from NaN parameters) elsewhere -- one compare and two 32-bit selects instead of
// np.sign's two compares and four.  Same values as osc_square except in v_fract_f64's corner (see above), where both
// answer -1.
__device__ __forceinline__ double osc_square_fract(double t) {
    const double d = 0.5 - __builtin_amdgcn_fract(t);
    const double one = __hiloint2double((int)(((unsigned)__double2hiint(d) & 0x80000000u) | 0x3ff00000u), 0);
    return (fabs(d) > 0.0) ? one : d;
}

// Triangle for the fused kernels.  The reference's (4 mod(u, 1/2) - 1) * sign(mod(u, 1) - 1/2), u = t - 1/4, is
// 4 |m - 1/2| - 1 with m = mod(u, 1), in one rounding of the same real number on either branch (m - 1/2 and mod(u, 1/2)
// are exact), except AT m = 1/2, where sign(0) makes it a zero: kept.  5 instructions + the zero fix instead of 15.
__device__ __forceinline__ double osc_triangle_fract(double t) {
    const double d = __builtin_amdgcn_fract(t - 0.25) - 0.5;
    const double r = fma(fabs(d), 4.0, -1.0);
    return (d == 0.0) ? 0.0 : r;
}

template <int KIND> __device__ __forceinline__ double osc_wave_fused(double t) {
    if (KIND == SIG_OSC_SQUARE) return osc_square_fract(t);
    if (KIND == SIG_OSC_SAWTOOTH) return osc_sawtooth_fract(t);
    if (KIND == SIG_OSC_TRIANGLE) return osc_triangle_fract(t);
    return osc_sine(t);
}

// ---- band-limited Square / Sawtooth / Triangle (chain/ext.py BlepOsc): the naive waveform plus a two-sample polynomial residual
// (PolyBLEP) around each edge.  d = min(|hertz| / rate, 0.5) is the phase increment per sample, inv_d = 1 / d (the caller divides
// once per copy, voice and block; the rows multiply).  With x = m / d below d and y = (m - 1) / d above 1 - d the definition's
//   step(m)   = 2x - x*x - 1 = -(x - 1)^2   |   y*y + 2y + 1 = (y + 1)^2   |   0
//   corner(m) = (1 - x)^3    = -(x - 1)^3   |   (y + 1)^3                  |   0
// are both one power of z = x - 1 | y + 1, negated below d: one multiply and one add per side, one select, the power, the sign.
// Against the definition evaluated in numpy's order: inv_d is within 1 ulp of 1 / d and x, y lie in [-1, 1], so z is within 3.4e-16
// of the definition's; the powers have slope <= 3 and round twice more: < 2e-15 per term, inside the 1e-14 the entry promises.
// Every choice is a select: with d == 0 (inv_d == inf) z is an infinity or a NaN that no window takes, and the result is 0.
// The two windows exclude each other for d <= 0.5.  A NaN m takes none.
// SIG_BLEP_SKIP=1 is a tuning build of osc_bank.hip ALONE (FILE=osc_bank.hip tools/build_variant.sh): the residual behind a
// wave-uniform branch, skipped where no lane of the wave is in a window.  The ballot needs every lane of the wave active, which
// holds in osc_bank_blep_kernel (its only exits are wave-uniform) and was not examined for the program handlers: sig_vp_machine.h
// refuses the macro.  Measured against the selects and not taken: DESIGN.md section 7.
#ifndef SIG_BLEP_SKIP
#define SIG_BLEP_SKIP 0
#endif
template <int POW> __device__ __forceinline__ double blep_residual(double m, double d, double inv_d) {
    const bool below = m < d, above = m > 1.0 - d;
#if SIG_BLEP_SKIP
    if (__builtin_amdgcn_ballot_w64(below || above) == 0) return 0.0;          // (every lane is active in osc_bank_blep_kernel)
#endif
    const double z = below ? m * inv_d - 1.0 : (m - 1.0) * inv_d + 1.0;
    const double p = (POW == 2) ? z * z : z * z * z;
    return below ? -p : (above ? p : 0.0);
}

// m = mod(t, 1): numpy's (the per-node kernel, whose f64 store is compared within 1e-14 and whose rows outside every window are
// the plain oscillator's bits) or v_fract_f64 (the fused handlers: see osc_sawtooth_fract; the corrected waveform is continuous, so
// the corner costs 2.2e-16 * (2 + 2 / d) in the sample at most)
template <bool FRACT> __device__ __forceinline__ double blep_mod1(double t) {
    if (FRACT) return __builtin_amdgcn_fract(t);
    return sig_npmod_pow2<1>(t);
}

// Above rate / 4 (d > 0.25) the Square's two windows overlap and above rate / 2 d is clamped: still the definition, no longer a
// band limit.  The naive parts of Square and Triangle have no zero at the edge (np.sign's there would leave a spike of height 1
// at exactly m = 1/2 in the corrected wave); a NaN m stays a NaN.
template <int KIND, bool FRACT = false> __device__ __forceinline__ double osc_blep(double t, double d, double inv_d) {
    static_assert(KIND == SIG_OSC_SQUARE || KIND == SIG_OSC_SAWTOOTH || KIND == SIG_OSC_TRIANGLE, "no band-limited Sine: it has no edge");
    if (KIND == SIG_OSC_SAWTOOTH) {
        const double m = blep_mod1<FRACT>(t - 0.5);
        return fma(m, 2.0, -1.0) - blep_residual<2>(m, d, inv_d);              // (2m is exact: the single rounding of 2 * m - 1)
    }
    if (KIND == SIG_OSC_SQUARE) {
        const double m = blep_mod1<FRACT>(t);
        const double naive = (m < 0.5) ? 1.0 : ((m >= 0.5) ? -1.0 : m);
        return (naive + blep_residual<2>(m, d, inv_d)) - blep_residual<2>(blep_mod1<FRACT>(t + 0.5), d, inv_d);
    }
    // Triangle: the reference's own closed form (4 mod(u, 1/2) - 1) * sign(mod(u, 1) - 1/2), u = t - 1/4, with the sign's zero dropped
    // -- 4 |m - 1/2| - 1 in real numbers, but in this order the value outside the windows is osc_triangle's bit for bit (m - 1/2
    // rounds for m < 1/4).  mod(u, 1/2) is m or m - 1/2 (exact above 1/2) behind v_fract_f64
    const double u = t - 0.25;
    const double m = blep_mod1<FRACT>(u);
    const double half = FRACT ? ((m < 0.5) ? m : m - 0.5) : sig_npmod_pow2<2>(u);
    const double r = fma(half, 4.0, -1.0);                                     // (the product by 4 is exact: numpy's 4 * mod(u, 0.5) - 1)
    const double naive = (m < 0.5) ? -r : r;                                   // (a NaN m: r is a NaN already)
    return naive + (4.0 / 3.0 * d) * (blep_residual<3>(blep_mod1<FRACT>(t + 0.25), d, inv_d) - blep_residual<3>(m, d, inv_d));
}

// d and 1 / d of a copy at h hertz: one IEEE divide each, per copy, voice and block
__device__ __forceinline__ void blep_increment(double h, double rate, double& d, double& inv_d) {
    d = fmin(fabs(h) / rate, 0.5);                                             // (a NaN h: fmin answers 0.5, and t is NaN anyway)
    inv_d = 1.0 / d;
}

// ---- hard-sync Sawtooth / Square (chain/ext.py SyncOsc): a slave oscillator at R = max(ratio, 1) times the master's pitch, reset at
// every cycle of the master; on top of the band-limited forms above.  With m = mod(t, 1) the master's phase, the slave's is
// s = m R, k = floor(s) its cycle since the reset and f = s - k (exact) its phase.  The slave's own edges, those strictly inside the
// master's cycle, take the residual at the slave's increment ds = min(d R, 0.5) (sync_residual: blep_residual<2> whose two sides are
// each switched by a condition on k); the reset at m = 0, of height 2 g for the Sawtooth (g = R - (ceil(R) - 1), the length of the
// last, cut slave cycle) and 0 | 2 for the Square (g <= 0.5 | g > 0.5), takes blep_residual<2> at the master's d, weighted.
// Block-invariant, hoisted by the caller: per voice R, g and the reset's weight (sync_ratio), per copy ds and 1 / ds
// (sync_increment).  A ratio that is not finite makes R a NaN (a select: fmax would drop it), and with it s, f and the sample; the
// Square's naive part passes a NaN f on like osc_blep's.  d == 0: ds == 0, no window, as above.  Where the last interior edge lies
// closer to the reset than one window (g < ds; the Square: 0 < g mod 0.5 < ds) its trailing window is cut at the reset: the
// definition's own discontinuity (ext.py), the same selects here.
struct SyncRatio { double R, g, reset; };
template <int KIND> __device__ __forceinline__ SyncRatio sync_ratio(double ratio) {
    static_assert(KIND == SIG_OSC_SQUARE || KIND == SIG_OSC_SAWTOOTH, "hard sync: Sawtooth and Square (a reset of Sine or Triangle changes the slope too)");
    SyncRatio p;
    p.R = (fabs(ratio) < __builtin_inf()) ? fmax(ratio, 1.0) : __builtin_nan("");
    p.g = p.R - (ceil(p.R) - 1.0);
    p.reset = (KIND == SIG_OSC_SAWTOOTH) ? p.g : ((p.g <= 0.5) ? 0.0 : 1.0);
    return p;
}

__device__ __forceinline__ void sync_increment(double d, double R, double& ds, double& inv_ds) {
    ds = fmin(d * R, 0.5);                                                     // (a NaN R: the sample is NaN anyway)
    inv_ds = 1.0 / ds;
}

__device__ __forceinline__ double sync_residual(double p, double ds, double inv_ds, bool lo_ok, bool hi_ok) {
    const bool low = p < ds;
    const bool below = low & lo_ok, above = (p > 1.0 - ds) & hi_ok;            // (they exclude each other for ds <= 0.5)
    const double z = low ? p * inv_ds - 1.0 : (p - 1.0) * inv_ds + 1.0;
    const double q = z * z;
    return below ? -q : (above ? q : 0.0);
}

// FUSED: m by v_fract_f64 (the program handlers), else numpy's mod (the per-node kernel: s, k and f are then the restatement's bits)
template <int KIND, bool FUSED = false>
__device__ __forceinline__ double osc_sync(double t, double d, double inv_d, const SyncRatio& r, double ds, double inv_ds) {
    static_assert(KIND == SIG_OSC_SQUARE || KIND == SIG_OSC_SAWTOOTH, "hard sync: Sawtooth and Square");
    const double m = blep_mod1<FUSED>(t);
    const double s = m * r.R;
    const double k = floor(s);
    const double f = s - k;
    const double edge = sync_residual(f, ds, inv_ds, k >= 1.0, k + 1.0 < r.R);
    const double reset = r.reset * blep_residual<2>(m, d, inv_d);
    if (KIND == SIG_OSC_SAWTOOTH) return (fma(f, 2.0, -1.0) - edge) - reset;   // (2f is exact: the single rounding of 2 * f - 1)
    const double sb = s + 0.5;
    const double kb = floor(sb);
    const double naive = (f < 0.5) ? 1.0 : ((f >= 0.5) ? -1.0 : f);
    return ((naive + edge) - sync_residual(sb - kb, ds, inv_ds, kb >= 1.0, kb + 0.5 < r.R)) + reset;
}

// ---- additive oscillator (chain/ext.py Additive): sin and cos of 2 pi m for a phase m = mod(t, 1) in [0, 1], the seed of the
// harmonic recurrence of osc_bank_additive_kernel.  cos(x) for |x| <= pi/2 + eps, even Taylor polynomial through x^22 (remainder
// < 1e-19), beside sin_poly.
__device__ __forceinline__ double cos_poly(double x) {
    const double s = x * x;
    double p = -8.8967913924505741e-22;                 // -1/22!
    p = fma(p, s, 4.1103176233121648e-19);              //  1/20!
    p = fma(p, s, -1.5619206968586225e-16);             // -1/18!
    p = fma(p, s, 4.7794773323873853e-14);              //  1/16!
    p = fma(p, s, -1.1470745597729725e-11);             // -1/14!
    p = fma(p, s, 2.0876756987868100e-09);              //  1/12!
    p = fma(p, s, -2.7557319223985888e-07);             // -1/10!
    p = fma(p, s, 2.4801587301587302e-05);              //  1/8!
    p = fma(p, s, -1.3888888888888889e-03);             // -1/6!
    p = fma(p, s, 4.1666666666666664e-02);              //  1/4!
    p = fma(p, s, -0.5);
    return fma(p, s, 1.0);
}

// K = rint(2m) by sine_phase's magic-number add, r = m - K/2 exact with |r| <= 1/4, x = 2 pi r to an ulp (2 fl(pi) and its tail),
// both polynomials on [-pi/2, pi/2], an odd K flips both signs.  Absolute error of either < 3e-16.  A NaN m gives NaNs.
__device__ __forceinline__ void cycle_sincos(double m, double& sn, double& cs) {
    const double u = fma(m, 2.0, kRoundMagic);
    const double k = u - kRoundMagic;
    const double r = fma(k, -0.5, m);
    const double x = fma(r, kTwoPiHi, r * kTwoPiLo);
    const int flip = (int)(((unsigned)__double2loint(u) & 1u) << 31);
    const double s = sin_poly(x), c = cos_poly(x);
    sn = __hiloint2double(__double2hiint(s) ^ flip, __double2loint(s));
    cs = __hiloint2double(__double2hiint(c) ^ flip, __double2loint(c));
}

template <int KIND, typename OUT> __device__ __forceinline__ OUT osc_wave(double t) {
    if (KIND == SIG_OSC_SINE) {
        if (sizeof(OUT) == 4) return (OUT)osc_sine_f32(t);
        return (OUT)osc_sine(t);
    }
    if (KIND == SIG_OSC_SQUARE) return (OUT)osc_square(t);
    if (KIND == SIG_OSC_SAWTOOTH) return (OUT)osc_sawtooth(t);
    return (OUT)osc_triangle(t);
}

}  // namespace sig_osc
