// The latency-mode kernel of the fused voice chain (fused_scan_kernel); entry points: fused_voice.hip.
#pragma once
#include "sig_osc.h"
#include "sig_steady.h"

namespace {

using namespace sig_fused;

// ---------------------------------------------------------------------------------------------------
// Latency mode: wavefront prefix-scan over TIME.  With one block per launch there are only `voices`
// independent chains (16 waves for 1024 voices) and each lane walks c+N rows serially: ~50 us for N=256 on
// an otherwise idle chip.  Here one WAVE owns one (voice, block) and its 64 lanes own consecutive chunks of
// L = ceil((c+N)/64) rows.  The recurrence is affine in the state s = (z0, z1):
//     s_n = A s_{n-1} + B x_n,   y_n = b0 x_n + z0_{n-1},   A = [[-a1, 1], [-a2, 0]]
// so (1) every lane runs its chunk from ZERO state (local outputs + local end state e_l), (2) a 6-step
// Hillis-Steele scan over the lanes with the matrices A^(L 2^k) turns the e_l into true chunk end states,
// (3) every lane adds the homogeneous response of its true start state to its local outputs.
// ~14 serial row steps + 6 scan steps instead of 356.  The scan reassociates the sums, so results match
// the serial kernels to ~1e-13 (f64), not bit for bit.
constexpr int kScanMaxL = 8;                                                  // rows per lane: c + N <= 512

template <int KIND, bool GAIN>
__global__ __launch_bounds__(256) void fused_scan_kernel(FusedArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);        // one wave = one (voice, block)
    const int v = (int)(item % a.voices);
    const int64_t b = item / a.voices;
    if (b >= a.K) return;
    const int64_t p_b = (a.pos_dev ? *a.pos_dev : a.position) + b * a.N;
    const int c = (int)((p_b < (int64_t)a.ctx) ? p_b : (int64_t)a.ctx);
    const int64_t n0 = p_b - c;
    const int total = c + a.N;
    const int L = (total + SIG_WAVE - 1) / SIG_WAVE;                           // <= kScanMaxL (host-checked)

    Biquad q;
    const bool ok = design_butter2(a.type, a.cutoff[(int64_t)v * a.cs], a.rate, q);
    if (!ok && a.status && lane == 0) atomicOr(a.status, SIG_STATUS_BAD_CUTOFF);
    const double hz = a.hertz[(int64_t)v * a.hs];
    const double ph = a.phase ? a.phase[(int64_t)v * a.ps] : 0.0;
    const double g = GAIN ? a.gain[(int64_t)v * a.gs] : 1.0;

    // (1) local pass from zero state
    double yl[kScanMaxL];
    double z0 = 0.0, z1 = 0.0;
#pragma unroll
    for (int k = 0; k < kScanMaxL; ++k) {
        const int r = lane * L + k;
        const bool valid = (k < L) && (r < total);
        const double t = (double)(n0 + r) / a.rate * hz + ph;                  // osc.py:32, same operator order
        double x = (KIND == SIG_OSC_SINE) ? (double)sig_osc::osc_sine_f32(t) : sig_osc::osc_wave_fused<KIND>(t);
        x = valid ? x : 0.0;
        const double y = fma(q.b0, x, z0);
        const double nz0 = fma(q.b1, x, fma(-q.a1, y, z1));
        const double nz1 = fma(q.b2, x, -q.a2 * y);
        yl[k] = y;
        if (k < L) { z0 = nz0; z1 = nz1; }                                     // rows past the chunk do not exist
    }

    // (2) scan of chunk end states: S_l = M S_{l-1} + e_l,  M = A^L
    const M2 A = {-q.a1, 1.0, -q.a2, 0.0};
    M2 M = A;
    for (int k = 1; k < L; ++k) M = m2_mul(A, M);
    double s0 = z0, s1 = z1;
#pragma unroll
    for (int d = 1; d < SIG_WAVE; d <<= 1) {
        const double p0 = __hiloint2double(__shfl_up(__double2hiint(s0), d, SIG_WAVE), __shfl_up(__double2loint(s0), d, SIG_WAVE));
        const double p1 = __hiloint2double(__shfl_up(__double2hiint(s1), d, SIG_WAVE), __shfl_up(__double2loint(s1), d, SIG_WAVE));
        if (lane >= d) {
            s0 += fma(M.a, p0, M.b * p1);
            s1 += fma(M.c, p0, M.d * p1);
        }
        M = m2_mul(M, M);
    }
    // true start state of this lane's chunk = end state of the previous lane's chunk
    double t0 = __hiloint2double(__shfl_up(__double2hiint(s0), 1, SIG_WAVE), __shfl_up(__double2loint(s0), 1, SIG_WAVE));
    double t1 = __hiloint2double(__shfl_up(__double2hiint(s1), 1, SIG_WAVE), __shfl_up(__double2loint(s1), 1, SIG_WAVE));
    if (lane == 0) { t0 = 0.0; t1 = 0.0; }

    // (3) homogeneous response of the start state, added to the local outputs
    float* dst = a.out + (b * a.N - c) * a.out_ld + v;
#pragma unroll
    for (int k = 0; k < kScanMaxL; ++k) {
        const int r = lane * L + k;
        const double yh = t0;                                                  // y = b0*0 + z0
        const double y = yl[k] + yh;
        const double u0 = fma(-q.a1, yh, t1);
        t1 = -q.a2 * yh;
        t0 = u0;
        if (k < L && r >= c && r < total) dst[(int64_t)r * a.out_ld] = (float)(GAIN ? y * g : y);
    }
}

// chains below which the serial walk leaves most of the chip idle (one wave per SIMD = 65536 lanes)
constexpr int64_t kScanMaxChains = 16384;

}  // namespace
