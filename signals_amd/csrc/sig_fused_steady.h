// The Sine closed form of the fused voice chain (fused_steady_bus_kernel and its per-voice constants, steady_prep_kernel);
// arguments and the constants' derivation: sig_steady.h, entry points: fused_voice.hip.
#pragma once
#include <type_traits>

#include "sig_biquad.h"
#include "sig_bus_tile.h"
#include "sig_osc.h"
#include "sig_steady.h"

namespace {      // (private to the translation unit that instantiates them: fused_voice.hip)

using namespace sig_fused;
using sig_bus::kPairs;
using sig_bus::kTileStride;

// ---------------------------------------------------------------------------------------------------
// Sine through a cold-started LTI filter in closed form ("steady" kernel).  For x_n = sin(phi_n), phi_n = phi_0 +
// n theta, the filter's response from zero state at row r0 is the steady-state sinusoid plus a decaying
// homogeneous solution:
//     y_n = yss_n + yh_n,     yss_n = Im(H(e^{j theta}) e^{j phi_n}),     (z0h, z1h)_n = A (z0h, z1h)_{n-1},  yh_n = z0h_{n-1}
// with the homogeneous state at r0 - 1 equal to minus the steady-state DF2T state there (so the total state is
// zero, fx.py:104's sosfilt start).  Every ingredient is linear in (yss_n, yss_{n+1} - yss_n), so the homogeneous
// state at a block's first row p = r0 + c is one per-voice 2x2 matrix applied to the steady-state oscillator's
// state at p:   (z0h, z1h)_{p-1} = T_c (yss_p, dss_p),   T_c = -A^c Mss(c)   -- no warm-up rows at all.
// Per stored sample: 1 (yss: the two-term recurrence y_{n+1} = 2 cos(theta) y_n - y_{n-1}, one fma, re-seeded from the
// reference's own t at every span start; its error grows like rows * 2e-16 / sin(theta), < 1e-9 for the voices this
// kernel accepts) + C (bus) + C/VPT (flush), and -- only while the homogeneous part of a voice is still above 1e-11
// of that voice's full scale -- 2 (homogeneous recurrence) + 1 (sum).  The homogeneous part decays like the pole
// radius^n and has already decayed over the c warm-up rows when the block starts: steady_prep_kernel bounds it
// rigorously per voice (rows from the cold start until it is below the tolerance, SC_ND), the kernel takes the wave
// maximum per voice SLOT (the i-th voice of every lane) and runs row groups in variants with only the first M slots
// "live".  A caller that orders its voices so that a slot holds neighbours in cutoff (the engine sorts by cutoff,
// slot-major) gets most row groups at M = 0; any order is correct.  Mathematically identical to the walker; rounding
// differs at 1e-10.  A wave takes this path when every voice of it passes steady_voice_ok(); the rare other waves run
// steady_fallback_span inside the same launch.
// Per-voice constants, computed once per launch by steady_prep_kernel into the tail of the workspace (SoA, kSteadyConsts
// rows of `voices` doubles): the filter, the oscillator step, H(e^{j theta}), T_c for c = ctx and for the launch's first
// block (c = min(ctx, position)), and the decay bound.
enum { SC_NA1, SC_NA2, SC_SCALE, SC_K2C, SC_ST, SC_CT, SC_HRE, SC_HIM, SC_ND, SC_T, SC_T0 = SC_T + 4, kSteadyConsts = SC_T0 + 4 };

// does the steady kernel take the wave of voices [v0, v0 + vpt) x 64 lanes for the span starting at frame p0?
__device__ __forceinline__ bool steady_wave(const FusedArgs& a, int v0, int vpt, int64_t p0, int nb) {
    const double q_first = (double)p0 / a.rate, q_last = (double)(p0 + (int64_t)nb * a.N - 1) / a.rate;
    bool ok = true;
    for (int i = 0; i < vpt; ++i) {
        const int v = (v0 + i < a.voices) ? v0 + i : ((v0 < a.voices) ? v0 : 0);
        ok &= steady_voice_ok(a.hertz[(int64_t)v * a.hs], a.phase ? a.phase[(int64_t)v * a.ps] : 0.0, a.rate,
                              a.steady_consts[(int64_t)SC_ST * a.voices + v], q_first, q_last);
    }
    return __all(ok);
}

// the closed form's per-voice constants (see the enum above), derived from the voice's parameters
template <bool GAIN>
__global__ __launch_bounds__(256) void steady_prep_kernel(FusedArgs a, double* __restrict__ consts)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.voices) return;
    const SteadyVoice c = steady_constants<GAIN>(a, v);
    if (!c.ok && a.status) atomicOr(a.status, SIG_STATUS_BAD_CUTOFF);
    auto put = [&](int k, double x) { consts[(int64_t)k * a.voices + v] = x; };
    put(SC_NA1, c.na1); put(SC_NA2, c.na2); put(SC_SCALE, c.scale);
    put(SC_K2C, c.k2c); put(SC_ST, c.st); put(SC_CT, c.ct);
    put(SC_HRE, c.hre); put(SC_HIM, c.him); put(SC_ND, c.nd);
    put(SC_T + 0, c.T.a); put(SC_T + 1, c.T.b); put(SC_T + 2, c.T.c); put(SC_T + 3, c.T.d);
    put(SC_T0 + 0, c.T0.a); put(SC_T0 + 1, c.T0.b); put(SC_T0 + 2, c.T0.c); put(SC_T0 + 3, c.T0.d);
}

// The rare waves the closed form does not take (a voice below ~8 Hz, above rate/4 or past 2^26 cycles), done inside the
// same launch by the plainest possible code: every block on its own, exact per-row phase (one IEEE divide per row),
// the b0-normalised recurrence from zero state over [c context rows | block], rows staged one at a time.  Rolled
// loops and no row groups, so that this path does not set the kernel's register budget; ~4x slower per voice-sample
// than the closed form, and it saves launching the span walker over every wave just to find nothing to do.
template <int VPT, int C>
__device__ __forceinline__ void steady_fallback_span(const FusedArgs& a, const BusArgs& bus, double* tile, int lane, int vt,
                                                  int64_t b_first, int nb, int v0)
{
    const int vc = (v0 < a.voices) ? v0 : 0;
    const double* sc = a.steady_consts;
    const double s2 = (a.type == SIG_FILT_LOWPASS) ? 2.0 : -2.0;
    sig_bus::PipelinedTile<C> stage(tile, lane, bus.partials + (int64_t)vt * bus.rows * C, b_first * a.N);
    for (int i = 0; i < VPT; ++i)                                              // a rejected design is NaN in the constants
        if (v0 + i < a.voices && a.status && sc[(int64_t)SC_NA1 * a.voices + v0 + i] != sc[(int64_t)SC_NA1 * a.voices + v0 + i])
            atomicOr(a.status, SIG_STATUS_BAD_CUTOFF);
#pragma unroll 1
    for (int bi = 0; bi < nb; ++bi) {
        const int64_t p_b = a.position + (b_first + bi) * a.N;
        const int c = (int)((p_b < (int64_t)a.ctx) ? p_b : (int64_t)a.ctx);
        double z0[VPT], z1[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) z0[i] = z1[i] = 0.0;
#pragma unroll 1
        for (int r = -c; r < a.N; ++r) {
            const double q = (double)(p_b + r) / a.rate;                       // osc.py:32
            double acc[C];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) acc[ch] = 0.0;
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const bool live = v0 + i < a.voices;
                const int v = live ? v0 + i : vc;
                const double t = q * a.hertz[(int64_t)v * a.hs] + (a.phase ? a.phase[(int64_t)v * a.ps] : 0.0);
                const double x = (double)sig_osc::osc_sine_f32(t);
                double na1 = sc[(int64_t)SC_NA1 * a.voices + v], na2 = sc[(int64_t)SC_NA2 * a.voices + v];
                double scale = live ? sc[(int64_t)SC_SCALE * a.voices + v] : 0.0;
                if (a.cutoff_rows > 1) {                                       // per-block cutoff rows: the block's own design (wave-uniform branch)
                    Biquad qd;
                    design_butter2(a.type, a.cutoff[(b_first + bi) * (int64_t)(a.cs ? a.voices : 1) + (int64_t)v * a.cs], a.rate, qd);
                    na1 = -qd.a1; na2 = -qd.a2;
                    scale = live ? qd.b0 : 0.0;
                    if (a.gain && a.gain_rows == 1) scale *= a.gain[(int64_t)v * a.gs];
                }
                const double y = x + z0[i];
                z0[i] = fma(na1, y, fma(s2, x, z1[i]));
                z1[i] = fma(na2, y, x);
                if (a.gain_rows > 1) scale *= a.gain[(b_first + bi) * (int64_t)(a.gs ? a.voices : 1) + (int64_t)v * a.gs];   // per-block gain rows (the constants then hold b0 only)
#pragma unroll
                for (int ch = 0; ch < C; ++ch) acc[ch] = fma(bus.pan ? bus.pan[ch * bus.pan_ld + v] * scale : scale, y, acc[ch]);
            }
            if (r >= 0) {                                                      // wave-uniform
#pragma unroll
                for (int ch = 0; ch < C; ++ch) stage.slot[ch * kTileStride] = acc[ch];
                stage.advance();
            }
        }
    }
    if (stage.staged) stage.now();
}

// the row-group variants of fused_steady_bus_kernel: "the first M of the lane's VPT voice slots still carry their
// homogeneous part", largest first
template <int VPT> struct SteadyVariants {
    static constexpr int count = (VPT >= 8) ? 7 : (VPT == 4) ? 4 : (VPT == 2) ? 3 : 2;
    static constexpr int at(int k) {                   // (16 voices per lane: registers for 8 live slots, like 8 per lane)
        constexpr int v8[7] = {8, 6, 4, 3, 2, 1, 0}, v4[4] = {4, 2, 1, 0}, v2[3] = {2, 1, 0}, v1[2] = {1, 0};
        return (VPT >= 8) ? v8[k] : (VPT == 4) ? v4[k] : (VPT == 2) ? v2[k] : v1[k];
    }
};

// Register budget of the closed-form kernel, as waves per SIMD the compiler must leave room for: its row groups are
// straight-line code with many independent chains, which the scheduler otherwise spreads over every register it can
// get (8 voices per lane: 417 registers and scratch, for 210 live values).
#ifndef SIG_STEADY_OCC8
#define SIG_STEADY_OCC8 1
#endif
#ifndef SIG_STEADY_AUTO16
#define SIG_STEADY_AUTO16 0              // 16 voices per lane (live slots capped at 8): 512 registers, AGPR copies and scratch -- 266 us vs 205 with 8: tuning hook only
#endif
#ifndef SIG_STEADY_OCC16
#define SIG_STEADY_OCC16 1
#endif
template <int VPT> struct SteadyOcc { static constexpr int waves = (VPT == 16) ? SIG_STEADY_OCC16 : (VPT == 8) ? SIG_STEADY_OCC8 : 2; };

// GROWS: the gain is read per block (a tremolo: sig_fused_voice_bus_rows with rows for the gain only); the constants then hold
// b0 alone and the bus weights are rebuilt at every block's first row
// CROWS: the cutoff (and possibly the gain) is read per block: the filter, its response H, T_c and the decay bound are derived
// at every block's first row from that block's rows, the steady-state recurrence is re-seeded at every block's first row with that block's H
// (the oscillator itself runs on: the phase of the row is recomputed from the reference's own t, two sines per voice and block)
template <int VPT, int C, bool GROWS, bool CROWS = false>
__device__ __forceinline__ void steady_bus_wave(const FusedArgs& a, const BusArgs& bus, double* tile, int lane, int wave, double* osc_store = nullptr)
{
    constexpr bool OSC_LDS = CROWS && VPT >= 8;                                // the per-span oscillator parts in LDS instead of registers (osc_store)
    constexpr int R = kPairs / C;          // rows per flush
    constexpr int LC = SteadyVariants<VPT>::at(0);     // voice slots that can carry a homogeneous part (all of them up to 8 per lane)
    static_assert(R % 2 == 0, "the two-term recurrence rotates two registers per voice: row groups are even");
    const int64_t item = (int64_t)blockIdx.x * 4 + wave;
    const int vt = (int)(item % a.voice_tiles);
    const int64_t b_first = (item / a.voice_tiles) * a.span;
    if (b_first >= a.K) return;                                               // wave-uniform
    const int nb = (int)((a.K - b_first < (int64_t)a.span) ? a.K - b_first : (int64_t)a.span);
    const int v0 = (vt * SIG_WAVE + lane) * VPT;
    const int vc = (v0 < a.voices) ? v0 : 0;
    const int64_t p0 = a.position + b_first * a.N;
    if (!steady_wave(a, v0, VPT, p0, nb)) {                                   // wave-uniform, rare
        steady_fallback_span<VPT, C>(a, bus, tile, lane, vt, b_first, nb, v0);
        return;
    }
    const double* sc = a.steady_consts;

    // per voice: the filter (na1, na2), the oscillator step k = 2 cos(theta), the steady-state output at rows p0 - 1
    // and p0 (ya, yb), the bus weights; per voice SLOT (wave-uniform): rows from a cold start after which the
    // homogeneous part is dropped
    double na1[LC], na2[LC], k2c[VPT], ya[VPT], yb[VPT], wt[C][VPT];
    int nd_total[VPT];
    const double q_first = (double)p0 / a.rate;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const bool live = v0 + i < a.voices;
        const int v = live ? v0 + i : vc;                                      // dead voices shadow a live one ...
        auto cst = [&](int k) { return sc[(int64_t)k * a.voices + v]; };
        const double na1_i = cst(SC_NA1);
        if (i < LC) { na1[i < LC ? i : 0] = na1_i; na2[i < LC ? i : 0] = cst(SC_NA2); }
        k2c[i] = cst(SC_K2C);
        // the design is checked where the constants are made (steady_prep_kernel); a caller that keeps them across
        // calls skips that launch, so every launch that USES a rejected design (NaN coefficients) reports it again
        if (live && na1_i != na1_i && a.status) atomicOr(a.status, SIG_STATUS_BAD_CUTOFF);
        const double scale = cst(SC_SCALE);
#pragma unroll
        for (int ch = 0; ch < C; ++ch)                                         // ... with weight exactly 0 on the bus
            wt[ch][i] = live ? (bus.pan ? bus.pan[ch * bus.pan_ld + v] * scale : scale) : 0.0;
        // steady-state oscillator at the span's first row: w = H e^{j phi}, yss_p0 = Im w, yss_{p0-1} = Im(w e^{-j theta})
        const double hz = a.hertz[(int64_t)v * a.hs], ph = a.phase ? a.phase[(int64_t)v * a.ps] : 0.0;
        const double t_first = q_first * hz + ph;                              // osc.py:32
        const double f0 = t_first - rint(t_first);                             // exact, |f0| <= 0.5
        const double ur = sin2pi(f0 + 0.25), ui = sin2pi(f0);
        const double hre = cst(SC_HRE), him = cst(SC_HIM);
        const double wr = fma(hre, ur, -(him * ui)), wi = fma(hre, ui, him * ur);
        yb[i] = wi;
        ya[i] = fma(wi, cst(SC_CT), -(wr * cst(SC_ST)));
        const double nd = cst(SC_ND);
        nd_total[i] = (live && nd < (double)kNeverDrops) ? (int)nd : (live ? kNeverDrops : 0);   // NaN: never
    }
    // ... per voice SLOT: the wave maximum, the VPT butterflies side by side (one after the other their cross-lane round trips
    // were a tenth of a one-block span)
#pragma unroll
    for (int d = 1; d < SIG_WAVE; d <<= 1) {
        int other[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) other[i] = __shfl_xor(nd_total[i], d, SIG_WAVE);
#pragma unroll
        for (int i = 0; i < VPT; ++i) nd_total[i] = (other[i] > nd_total[i]) ? other[i] : nd_total[i];
    }
#pragma unroll
    for (int i = 0; i < VPT; ++i) nd_total[i] = __builtin_amdgcn_readfirstlane(nd_total[i]);

    double* dstp = bus.partials + (int64_t)vt * bus.rows * C;                  // [tile][row][c]
    sig_bus::PipelinedTile<C> stage(tile, lane, dstp, b_first * a.N);

    // 16 voices per lane: only the first 8 slots have registers for a homogeneous part; the caller vouched (consts_ready
    // bit 1) that the others have none at any block start of this launch -- checked here, a wave it does not hold for takes
    // the plain fallback (correct, slow)
    if constexpr (LC < VPT) {
        const int c_min = (b_first == 0 && a.position < (int64_t)a.ctx) ? (int)a.position : a.ctx;
        bool capped = true;
#pragma unroll
        for (int i = LC; i < VPT; ++i) capped &= nd_total[i] <= c_min;
        if (!capped) {                                                         // wave-uniform
            steady_fallback_span<VPT, C>(a, bus, tile, lane, vt, b_first, nb, v0);
            return;
        }
    }
    [[maybe_unused]] OscPart osc[(CROWS && !OSC_LDS) ? VPT : 1];               // CROWS: what the per-block constants need of the oscillator (once per span)
    auto osc_slot = [&](int field, int i) -> double& { return osc_store[((size_t)field * VPT + i) * SIG_WAVE + lane]; };
    if constexpr (CROWS) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int v = (v0 + i < a.voices) ? v0 + i : vc;
            const OscPart made = steady_osc_part(a.type, a.hertz[(int64_t)v * a.hs], a.rate, a.ctx);
            if constexpr (OSC_LDS) {
                osc_slot(0, i) = made.ct; osc_slot(1, i) = made.st; osc_slot(2, i) = made.beta; osc_slot(3, i) = made.enr; osc_slot(4, i) = made.eni;
            } else {
                osc[i] = made;
            }
        }
    }
    double z0h[LC], z1h[LC];
    // One row of every voice; the first M slots carry their homogeneous part, the others have dropped it.  The row's C
    // sums over the lane's voices go to `sums` (registers of the group being built, or the LDS slot of the single-row
    // form).  The two-term recurrence runs IN PLACE on two registers per voice: on an even row yb is the sample and ya
    // becomes the one after next, on an odd row the roles are swapped -- no register rotation for the compiler to undo.
    auto row = [&](double* sums, int sums_stride, auto m_tag, auto odd_tag) {
        constexpr int M = decltype(m_tag)::value;
        constexpr bool ODD = decltype(odd_tag)::value;
        double y[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const double ys = ODD ? ya[i] : yb[i];
            if (ODD) yb[i] = fma(k2c[i], ya[i], -yb[i]);
            else ya[i] = fma(k2c[i], yb[i], -ya[i]);
            if (i < M) {
                const int j = i < LC ? i : 0;                                  // (M <= LC: always i itself)
                y[i] = ys + z0h[j];
                const double yh = z0h[j];
                z0h[j] = fma(na1[j], yh, z1h[j]);
                z1h[j] = na2[j] * yh;
            } else {
                y[i] = ys;
            }
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < VPT; ++i) acc = fma(wt[ch][i], y[i], acc);
            sums[ch * sums_stride] = acc;
        }
    };
    // One group of R rows: their kPairs sums stay in registers, are folded across lanes (sig_bus::FoldedGroup) and the
    // LDS reads of the last step are issued at once; they are consumed half-way through the NEXT group, when they (and
    // the stores in front of them: a wave's LDS operations complete in order) have long retired.
    sig_bus::FoldedGroup<C> folded(tile, lane, dstp);
    double pend[4];
    int64_t pend_row = 0;
    bool have = false;
    // Two consecutive rows at once (an even one and an odd one, see `row`), so that their 2 C bus sums are FOUR
    // independent accumulation chains: a lone wave issues an f64 instruction every 4 cycles but a dependent one only
    // every ~10, and two interleaved chains (one row's two channels) ran at 60 % of the issue rate.
    auto rows2 = [&](double* sums, auto m_tag) {
        constexpr int M = decltype(m_tag)::value;
        double y0[VPT], y1[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            y0[i] = yb[i];
            ya[i] = fma(k2c[i], yb[i], -ya[i]);
            y1[i] = ya[i];
            yb[i] = fma(k2c[i], ya[i], -yb[i]);
            if (i < M) {
                const int j = i < LC ? i : 0;                                  // (M <= LC: always i itself)
                const double h0 = z0h[j];
                y0[i] += h0;
                const double h1 = fma(na1[j], h0, z1h[j]);
                y1[i] += h1;
                z0h[j] = fma(na1[j], h1, na2[j] * h0);
                z1h[j] = na2[j] * h1;
            }
        }
        double acc0[C], acc1[C];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) { acc0[ch] = 0.0; acc1[ch] = 0.0; }
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                acc0[ch] = fma(wt[ch][i], y0[i], acc0[ch]);
                acc1[ch] = fma(wt[ch][i], y1[i], acc1[ch]);
            }
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) { sums[ch] = acc0[ch]; sums[C + ch] = acc1[ch]; }
    };
    auto group = [&](auto m_tag) {
        double acc[kPairs];
#pragma unroll
        for (int k = 0; k < R; k += 2) {
            rows2(acc + k * C, m_tag);
#pragma unroll
            for (int q = 0; q < kPairs / 4; ++q)                               // every four sums are folded as soon as they exist
                if (4 * q + 3 < (k + 2) * C && 4 * q + 3 >= k * C)
                    folded.fold4(q, acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
            if (k + 2 == R / 2 && have) folded.finish(pend, pend_row, R);
        }
        folded.issue(pend);
        pend_row = stage.first; stage.first += R; have = true;
    };
    // Row groups come in variants "the first M slots live", M from kVariants; within a block the number of live slots only
    // falls, so a block is a sequence of PHASES, one plain loop per variant (a switch per group cost 20-30 %: the
    // variants' registers had to be shuffled into one layout at every merge).  Phase of variant M runs until every slot
    // >= the next smaller variant has dropped.
    using Variants = SteadyVariants<VPT>;

    for (int bi = 0; bi < nb; ++bi) {
        if constexpr (GROWS && !CROWS) {
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const bool live = v0 + i < a.voices;
                const int v = live ? v0 + i : vc;
                const double scale = sc[(int64_t)SC_SCALE * a.voices + v] * a.gain[(b_first + bi) * (int64_t)(a.gs ? a.voices : 1) + (int64_t)v * a.gs];
#pragma unroll
                for (int ch = 0; ch < C; ++ch) wt[ch][i] = live ? (bus.pan ? bus.pan[ch * bus.pan_ld + v] * scale : scale) : 0.0;
            }
        }
        // homogeneous state at the block's first row; only the launch's very first block can have a short context
        const bool first = (b_first + bi == 0);
        const int tk = first ? SC_T0 : SC_T;
        const int c = first ? (int)((a.position < (int64_t)a.ctx) ? a.position : (int64_t)a.ctx) : a.ctx;
        if constexpr (CROWS) {
            // this block's filter, derived here from cutoff row b (and gain row b): coefficients, bus weights, the steady-state
            // seeds from its H at the voice's frequency, T_c for the block's context and the decay bound per slot.  ~300 f64
            // operations per voice and block (steady_block_constants) against ~1100 for the block's 256 rows -- and no round trip of 80 bytes per
            // (block, voice) through HBM, which a prep launch would cost (measured: 31 us + 29 us per 1024-block batch)
            const int64_t blk = b_first + bi;
            const double q_b = (double)(p0 + (int64_t)bi * a.N) / a.rate;
            // every load of the block first, all voices side by side: the rows of block b come from HBM, and one voice after
            // the other (each voice's constants end in a loop) their latencies added up to 20 us per block
            double cut_i[VPT], gain_i[VPT];                                    // (the block-invariant rows -- pan, hertz, phase -- sit in the caches)
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int v = (v0 + i < a.voices) ? v0 + i : vc;
                cut_i[i] = a.cutoff[(a.cutoff_rows > 1 ? blk * (int64_t)(a.cs ? a.voices : 1) : 0) + (int64_t)v * a.cs];
                gain_i[i] = a.gain ? a.gain[(a.gain_rows > 1 ? blk * (int64_t)(a.gs ? a.voices : 1) : 0) + (int64_t)v * a.gs] : 1.0;
            }
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const bool live = v0 + i < a.voices;
                const int v = live ? v0 + i : vc;
                const double cutoff = cut_i[i], gain = gain_i[i];
                const double hz_v = a.hertz[(int64_t)v * a.hs], ph_v = a.phase ? a.phase[(int64_t)v * a.ps] : 0.0;
                // the oscillator's part is kept per voice for c = ctx; the launch's first block may have a shorter context
                OscPart op;
                if constexpr (OSC_LDS) op = OscPart{osc_slot(0, i), osc_slot(1, i), osc_slot(2, i), osc_slot(3, i), osc_slot(4, i)};
                else op = osc[i];
                if (__builtin_expect(c != a.ctx, 0)) op = steady_osc_part(a.type, hz_v, a.rate, c);      // (wave-uniform, the first block of a stream only)
                const double ct_i = op.ct, st_i = op.st;
                const BlockVoice cv = steady_block_constants(a.type, a.rate, cutoff, gain, op, c);
                if (i < LC) { na1[i < LC ? i : 0] = cv.na1; na2[i < LC ? i : 0] = cv.na2; }
                if (live && !cv.ok && a.status) atomicOr(a.status, SIG_STATUS_BAD_CUTOFF);
#pragma unroll
                for (int ch = 0; ch < C; ++ch) wt[ch][i] = live ? (bus.pan ? bus.pan[ch * bus.pan_ld + v] * cv.scale : cv.scale) : 0.0;
                const double t_first = q_b * hz_v + ph_v;                      // osc.py:32
                const double f0 = t_first - rint(t_first);
                const double ur = sin2pi(f0 + 0.25), ui = sin2pi(f0);
                const double wr = fma(cv.hre, ur, -(cv.him * ui)), wi = fma(cv.hre, ui, cv.him * ur);
                yb[i] = wi;
                ya[i] = fma(wi, ct_i, -(wr * st_i));
                if (i < LC) {                                                  // the homogeneous state at the block's first row (zeroed below where the slot has none)
                    const double dss = fma(k2c[i], yb[i], -ya[i]) - yb[i];      // yss_{p+1} - yss_p
                    z0h[i < LC ? i : 0] = fma(cv.T.a, yb[i], cv.T.b * dss);
                    z1h[i < LC ? i : 0] = fma(cv.T.c, yb[i], cv.T.d * dss);
                }
                nd_total[i] = (live && cv.nd < (double)kNeverDrops) ? (int)cv.nd : (live ? kNeverDrops : 0);
            }
#pragma unroll
            for (int d = 1; d < SIG_WAVE; d <<= 1) {
                int other[VPT];
#pragma unroll
                for (int i = 0; i < VPT; ++i) other[i] = __shfl_xor(nd_total[i], d, SIG_WAVE);
#pragma unroll
                for (int i = 0; i < VPT; ++i) nd_total[i] = (other[i] > nd_total[i]) ? other[i] : nd_total[i];
            }
#pragma unroll
            for (int i = 0; i < VPT; ++i) nd_total[i] = __builtin_amdgcn_readfirstlane(nd_total[i]);
        }
        int drop_at[LC];                                                       // row of the block from which slot i is dropped
#pragma unroll
        for (int i = 0; i < LC; ++i) {
            drop_at[i] = (nd_total[i] > c) ? nd_total[i] - c : 0;              // wave-uniform
            if (drop_at[i] > 0) {
                const int v = (v0 + i < a.voices) ? v0 + i : vc;
                const double dss = fma(k2c[i], yb[i], -ya[i]) - yb[i];          // yss_{p+1} - yss_p
                if constexpr (!CROWS) {                                       // (CROWS: made with the block's constants above)
                    const double* t = sc + (int64_t)tk * a.voices + v;
                    z0h[i] = fma(t[0], yb[i], t[a.voices] * dss);
                    z1h[i] = fma(t[2 * (int64_t)a.voices], yb[i], t[3 * (int64_t)a.voices] * dss);
                }
            } else {
                z0h[i] = 0.0; z1h[i] = 0.0;
            }
        }
        int done = 0;
        auto single = [&]() {                                                  // (dropped slots carry zeros: the full row is exact)
            row(stage.slot, kTileStride, std::integral_constant<int, LC>{}, std::false_type{});
#pragma unroll
            for (int i = 0; i < VPT; ++i) { const double t = ya[i]; ya[i] = yb[i]; yb[i] = t; }   // back to (previous, current)
            ++done;
            stage.advance();
        };
        while (stage.staged != 0 && done < a.N) single();
        // phases; after single rows `done` is not a multiple of R, the groups simply start there
        const int last_group_row = done + ((a.N - done) / R) * R;
        auto phase = [&](auto k_tag) {
            constexpr int K = decltype(k_tag)::value;
            constexpr int M = Variants::at(K);
            constexpr int lower = (K + 1 < Variants::count) ? Variants::at(K + 1) : 0;
            int until = 0;                                                     // first row at which every slot >= lower has dropped
#pragma unroll
            for (int i = lower; i < LC; ++i) until = (i < M && drop_at[i] > until) ? drop_at[i] : until;
            if (M == 0) until = a.N;
            until = (until < last_group_row) ? until : last_group_row;
            while (done < until) {                                             // (a group that starts before `until` runs whole)
                group(std::integral_constant<int, M>{});
                done += R;
            }
        };
#define SIG_PHASE(K) if constexpr (K < Variants::count) phase(std::integral_constant<int, K>{});
        SIG_PHASE(0) SIG_PHASE(1) SIG_PHASE(2) SIG_PHASE(3) SIG_PHASE(4) SIG_PHASE(5) SIG_PHASE(6) SIG_PHASE(7) SIG_PHASE(8)
#undef SIG_PHASE
        if (done < a.N) {                                                      // rows left over: one at a time, after the pending flush
            if (have) { folded.finish(pend, pend_row, R); have = false; }
#pragma unroll
            for (int i = 0; i < LC; ++i)
                if (drop_at[i] <= done) { z0h[i] = 0.0; z1h[i] = 0.0; }        // dropped slots were not advanced: exact zeros
            while (done < a.N) single();
        }
    }
    if (have) folded.finish(pend, pend_row, R);
    if (stage.staged) stage.now();
}

template <int VPT, int C, bool GROWS = false, bool CROWS = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CROWS ? 1 : SteadyOcc<VPT>::waves, 8)))
void fused_steady_bus_kernel(FusedArgs a, BusArgs bus)
{
    __shared__ double lds[4][kPairs * kTileStride];
    // per-block constants at 8 voices per lane: the per-span oscillator parts (5 doubles per voice) do not fit the register file
    // beside the row state -- they live here, [wave][field][voice][lane], 80 KiB per workgroup (one workgroup per CU: the kernel
    // runs one wave per SIMD anyway)
    constexpr bool kOscInLds = CROWS && VPT >= 8;
    __shared__ double osc_lds[kOscInLds ? 4 * 5 * VPT * SIG_WAVE : 1];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);        // wave-uniform BY CONSTRUCTION: tell the compiler, so that
    steady_bus_wave<VPT, C, GROWS, CROWS>(a, bus, lds[wave], lane, wave,       // everything derived from it lives in SGPRs and branches are scalar
                                          kOscInLds ? osc_lds + (size_t)wave * 5 * VPT * SIG_WAVE : nullptr);
    if (bus.out) sig_bus::sum_tiles_in_workgroup<C>(bus.partials, a.voice_tiles, bus.rows, a.span, a.K, a.N, bus.out, bus.out_ld, lane, wave);
}

// workspace of sig_fused_voice_bus: [tile partials, worst case one tile per 64 voices][steady constants]
int64_t steady_consts_offset(int voices, int64_t rows, int bus_channels) {
    return (int64_t)sig_voice_tiles(voices, 1) * rows * bus_channels;       // in doubles
}

// the closed form: per-voice constants, then one launch (closed form per wave, or its built-in plain fallback
// steady_fallback_span); sets bus.out when the kernel adds the voice tiles itself
template <bool GAIN, int C, bool GROWS, bool CROWS = false>
int launch_steady(FusedArgs& a, BusArgs& bus, int vpt, float* out, int64_t out_ld, hipStream_t stream)
{
    double* consts = a.consts_ext ? a.consts_ext : bus.partials + steady_consts_offset(a.voices, bus.rows, C);
    a.steady_consts = consts;
    if (!(a.consts_ext && a.consts_ready))
        steady_prep_kernel<GAIN><<<(a.voices + 255) / 256, 256, 0, stream>>>(a, consts);

    a.voice_tiles = sig_voice_tiles(a.voices, vpt);
    unsigned nwg;
    if (!sig_workgroups(sig_span_waves(a.voice_tiles, a.K, a.span), nwg)) return (int)hipErrorInvalidValue;
    if (sig_bus::tiles_sum_in_workgroup(a.voice_tiles) && tuning().tile_sum_kernel == 0) { bus.out = out; bus.out_ld = out_ld; }
    switch (vpt) {
        case 1: fused_steady_bus_kernel<1, C, GROWS, CROWS><<<nwg, 256, 0, stream>>>(a, bus); break;
        case 2: fused_steady_bus_kernel<2, C, GROWS, CROWS><<<nwg, 256, 0, stream>>>(a, bus); break;
        case 8: fused_steady_bus_kernel<8, C, GROWS, CROWS><<<nwg, 256, 0, stream>>>(a, bus); break;
        case 16: if constexpr (!CROWS) { fused_steady_bus_kernel<16, C, GROWS><<<nwg, 256, 0, stream>>>(a, bus); break; }
        default: fused_steady_bus_kernel<4, C, GROWS, CROWS><<<nwg, 256, 0, stream>>>(a, bus); break;
    }
    return sig_launch_status();
}

}  // namespace
