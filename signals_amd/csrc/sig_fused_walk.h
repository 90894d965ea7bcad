// The span walker of the fused voice chain for gfx950 (fused_walk_kernel; entry points: fused_voice.hip): Osc -> cold-start Butterworth biquad -> [x per-voice gain] -> f32 store or
// -> [pan x gain] -> bus partial sums, K blocks per launch.  Chosen by the batched engine when a LowPass/HighPass
// reads an oscillator nobody else consumes (and, optionally, feeds a Gain and a SumBus nobody else consumes): the
// oscillator samples never touch HBM, so the stage costs 4 B/voice-sample (the store) or ~0.13 B (the bus
// partials) instead of 4 + 8 (+ 8 + 4).
//
// Same design and phase arithmetic as the node kernels (sig_osc.h, sig_biquad.h; reference osc.py:26-62,
// fx.py:85-121, fx.py:51-52): f64 phase, f64 recurrence from zero state over [c context rows | block].  What
// differs from the per-node path, all of it below 1e-9 of the f64 reference and far inside the 1e-6 bar:
//   * the filter input is the oscillator's f64 sample, not its f32-rounded store;
//   * the recurrence runs on the b0-normalised filter  y' = y / b0  (b = [1, +-2, 1] for a Butterworth
//     low/high-pass), 4 fused multiply-adds per row instead of sosfilt's 8 separately rounded operations; b0 is
//     folded into the per-voice output weight (gain, pan), which is applied in f64 before the one f32 rounding;
//   * SPAN WALKER: a lane owns `span` consecutive blocks of its voices.  Block b+1 cold-starts from zero state
//     at its row -c, i.e. inside block b: its warm-up runs as a second recurrence on the oscillator sample the
//     lane has just computed for block b, and becomes the output recurrence at the block boundary.  Every
//     oscillator sample is computed once (not (N+c)/N times); the arithmetic of each chain is unchanged;
//   * Sine, while every |t| of the span is < 2^26 cycles and the voice advances by at most a quarter turn per
//     row (|hertz| <= rate/4 after aliasing): the oscillator is the two-term recurrence in difference (Reinsch)
//     form   x <- x + d;  d <- d - m x,   m = 4 sin^2(theta/2),  d_0 = 2 sin(theta/2) cos(phi_0 + theta/2),
//     seeded once per span from the reference's own t at the span's first row (sin by the f64 polynomial).
//     2 f64 ops per sample, no divide, no conversion, no v_sin_f32; rounding grows like rows x 1e-16 (the
//     difference form has no 1/theta amplification), i.e. ~1e-13 from sin(2 pi t) instead of v_sin_f32's 1e-7.
//     Otherwise (wave-uniform test) the exact per-row phase of sig_osc.h is used, as for the other waveforms.
//
// Mapping: one wave = 64*VPT consecutive voices x `span` consecutive blocks, lanes walk rows serially.  On the
// exact-phase path the per-row quotient n/rate (IEEE f64 divide) is computed 64 rows at a time, one row per
// lane, and broadcast with v_readlane.  f64-VALU-bound: Sine ~ 2 (osc) + 4 (N+c')/N (filter) + C (bus) f64
// ops per voice-sample.
#pragma once
#include <type_traits>

#include "sig_biquad.h"
#include "sig_bus_tile.h"
#include "sig_mix_tile.h"
#include "sig_osc.h"
#include "sig_steady.h"

namespace {      // (kernels and launchers are private to each translation unit that instantiates them: fused_voice.hip, fused_voice_b.hip)

using namespace sig_fused;
using sig_vec::OutVec;
using sig_vec::put;
// Bus sums: sig_bus_tile.h (wave-private LDS tile, transposed reduction, per-tile f64 partials + fixed-order tile sum)
using sig_bus::kPairs;
using sig_bus::kTileStride;

// Register budget per voices-per-lane variant, as waves per SIMD the compiler must leave room for (0 = its own
// choice): the row groups below are straight-line code with many independent chains, which the scheduler would
// otherwise spread over every register it can get.  Values from tools/sweep_fused.sh.
#ifndef SIG_FUSED_OCC1
#define SIG_FUSED_OCC1 0
#endif
#ifndef SIG_FUSED_OCC2
#define SIG_FUSED_OCC2 0
#endif
#ifndef SIG_FUSED_OCC4
#define SIG_FUSED_OCC4 0
#endif
template <int VPT> struct Occ;
template <> struct Occ<1> { static constexpr int lo = SIG_FUSED_OCC1 ? SIG_FUSED_OCC1 : 1, hi = SIG_FUSED_OCC1 ? SIG_FUSED_OCC1 : 8; };
template <> struct Occ<2> { static constexpr int lo = SIG_FUSED_OCC2 ? SIG_FUSED_OCC2 : 1, hi = SIG_FUSED_OCC2 ? SIG_FUSED_OCC2 : 8; };
template <> struct Occ<4> { static constexpr int lo = SIG_FUSED_OCC4 ? SIG_FUSED_OCC4 : 1, hi = SIG_FUSED_OCC4 ? SIG_FUSED_OCC4 : 8; };

// C == 0: store (float)(weight * y) to a.out; C > 0: C bus channels into bus.partials; C == -1 (one voice per lane,
// voices a multiple of 64): the MixMatrix sink -- the wave's 64 voices are one matrix group, every 32 rows of
// float32 samples are staged in a wave-private LDS tile and multiplied by the 64 x 64 matrix on the matrix cores
// (sig_mix_tile.h: each float32 as three bfloat16, six bf16 MFMAs per k-block), then stored.  The per-voice rows
// never touch HBM.
// ROWS: cutoff and gain are read per block (the reference reads a control port once per block, at the block's position:
// chain/__init__.py:305-306 -- an LFO on a cutoff, a tremolo); the filter is then designed per block, the next block's
// warm-up chain with the next block's design.  GAIN is ignored (a null gain pointer means 1).
template <int KIND, int VPT, bool GAIN, int C, bool ROWS>
__device__ __forceinline__ void walk_wave(const FusedArgs& a, const BusArgs& bus, double* tile, int lane, int wave)
{
    constexpr bool BUS = C > 0, MIX = C < 0;
    constexpr int CC = BUS ? C : 1;
    constexpr int R = kPairs / CC;         // rows per flush
    static_assert(!MIX || VPT == 1, "the MixMatrix sink maps one matrix group to one wave");
    using Vec = typename OutVec<VPT>::type;
    const int64_t item = (int64_t)blockIdx.x * 4 + wave;
    const int vt = (int)(item % a.voice_tiles);
    const int64_t b_first = (item / a.voice_tiles) * a.span;
    if (b_first >= a.K) return;                                               // wave-uniform
    const int nb = (int)((a.K - b_first < (int64_t)a.span) ? a.K - b_first : (int64_t)a.span);
    const int v0 = (vt * SIG_WAVE + lane) * VPT;
    const bool live0 = v0 < a.voices;
    const int vc = live0 ? v0 : 0;

    const int64_t p0 = (a.pos_dev ? *a.pos_dev : a.position) + b_first * a.N;  // first frame of the span's first block
    const int c0 = (int)((p0 < (int64_t)a.ctx) ? p0 : (int64_t)a.ctx);
    const double s2 = (a.type == SIG_FILT_LOWPASS) ? 2.0 : -2.0;                // b1 / b0

    double na1[VPT], na2[VPT], z0[VPT], z1[VPT], wt[CC][VPT];
    double wna1[ROWS ? VPT : 1], wna2[ROWS ? VPT : 1], wwt[ROWS ? CC : 1][ROWS ? VPT : 1];   // ROWS: the next block's design and weights
    // the filter and the output weights of block b (ROWS: from parameter row b)
    auto design_block = [&](int64_t b, double* n1, double* n2, auto weights) {
        bool ok = true, any_live = false;
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const bool live = v0 + i < a.voices;
            const int v = live ? v0 + i : vc;                                  // dead voices shadow a live one ...
            any_live |= live;
            const int64_t crow = (ROWS && a.cutoff_rows > 1) ? b * (int64_t)(a.cs ? a.voices : 1) : 0;
            const int64_t grow = (ROWS && a.gain_rows > 1) ? b * (int64_t)(a.gs ? a.voices : 1) : 0;
            Biquad q;
            ok &= design_butter2(a.type, a.cutoff[crow + (int64_t)v * a.cs], a.rate, q) || !live;
            n1[i] = -q.a1; n2[i] = -q.a2;
            const double scale = (ROWS ? a.gain != nullptr : GAIN) ? q.b0 * a.gain[grow + (int64_t)v * a.gs] : q.b0;
#pragma unroll
            for (int ch = 0; ch < CC; ++ch)                                    // ... with weight exactly 0 on the bus
                weights(ch, i, BUS ? (live ? (bus.pan ? bus.pan[ch * bus.pan_ld + v] * scale : scale) : 0.0) : scale);
        }
        if (!ok && any_live && a.status) atomicOr(a.status, SIG_STATUS_BAD_CUTOFF);
    };
    design_block(b_first, na1, na2, [&](int ch, int i, double w) { wt[ch][i] = w; });
#pragma unroll
    for (int i = 0; i < VPT; ++i) z0[i] = z1[i] = 0.0;

    // hertz / phase of the lane's voices (re-read where needed rather than kept live across the row loops)
    // ROWS with hertz_rows / phase_rows > 1: row `blk` of the launch (-1: the row in front of it, *_hist)
    const bool fm = ROWS && (a.hertz_hist || a.phase_hist);                    // (a one-block launch has one row, and still a row in front)
    auto load_hz_ph = [&](double (&hz)[VPT], double (&ph)[VPT], int64_t blk = 0) {
        const double* hp = a.hertz; const double* pp = a.phase;
        if (ROWS && a.hertz_hist) hp = (blk < 0) ? a.hertz_hist : a.hertz + (a.hertz_rows > 1 ? blk * (int64_t)(a.hs ? a.voices : 1) : 0);
        if (ROWS && a.phase_hist) pp = (blk < 0) ? a.phase_hist : a.phase + (a.phase_rows > 1 ? blk * (int64_t)(a.ps ? a.voices : 1) : 0);
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int v = (v0 + i < a.voices) ? v0 + i : vc;
            hz[i] = hp[(int64_t)v * a.hs];
            ph[i] = pp ? pp[(int64_t)v * a.ps] : 0.0;
        }
    };

    // Sine as a two-term recurrence (see the header): seeded at the span's first row; under block-rate FM at every block's
    // first row (and for the span's warm-up rows) with that block's hertz / phase -- the recurrence then never runs longer
    // than a block
    bool fast = false;
    double sx[VPT], sdl[VPT], snm[VPT];                                        // x, d, -m
    int64_t seeded_blk = b_first - 1;                                          // FM: the block whose rows the recurrence was last seeded for
    // seeds for rows from frame n on, made with parameter row `blk`; returns whether every voice qualifies up to frame n_last
    auto seed_sine = [&](int64_t blk, int64_t n, int64_t n_last) {
        double hz[VPT], ph[VPT];
        load_hz_ph(hz, ph, blk);
        const double q_first = (double)n / a.rate;                             // osc.py:32
        const double q_last = (double)n_last / a.rate;
        bool small = true;
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const double t_first = q_first * hz[i] + ph[i];
            const double t_last = q_last * hz[i] + ph[i];                      // t is monotonic in the row
            const double d = hz[i] / a.rate;                                   // revolutions per row
            const double dr = d - rint(d);
            small &= fabs(t_first) < sig_osc::kSineFastMaxT && fabs(t_last) < sig_osc::kSineFastMaxT && fabs(dr) <= 0.25;
            const double f0 = t_first - rint(t_first);                         // exact, |f0| <= 0.5
            const double sh = sin2pi(0.5 * dr);                                // sin(theta / 2)
            sx[i] = sin2pi(f0);
            sdl[i] = 2.0 * sh * sin2pi(f0 + 0.5 * dr + 0.25);                  // x_1 - x_0
            snm[i] = -4.0 * sh * sh;
        }
        return small;
    };
    if (KIND == SIG_OSC_SINE) {
        bool small = true;
        if (fm) {                                                              // every block of the span must qualify with its own row
            for (int bi = nb - 1; bi >= 0; --bi)
                small &= seed_sine(b_first + bi, p0 + (int64_t)bi * a.N, p0 + (int64_t)(bi + 1) * a.N - 1);
            small &= seed_sine(b_first - 1, p0 - c0, p0 - 1 >= p0 - c0 ? p0 - 1 : p0 - c0);     // (last: the warm-up rows come first)
        } else {
            small = seed_sine(0, p0 - c0, p0 + (int64_t)nb * a.N - 1);
        }
        fast = __all(small);
    }

    float* dst = (BUS || MIX) ? nullptr : a.out + vc;                          // row index = frame - position
    double* dstp = BUS ? bus.partials + (int64_t)vt * bus.rows * C : nullptr;  // [tile][row][c]
    sig_bus::PipelinedTile<CC> stage(tile, lane, dstp, b_first * a.N);
    int64_t n_cur = p0 - c0;                                                   // absolute frame of the next row

    // MixMatrix sink: rows staged as float32, 32 at a time through the matrix cores (sig_mix_tile.h)
    std::conditional_t<MIX, sig_mix::Sink, int> sink{};
    if constexpr (MIX) sink.init(a.mix, reinterpret_cast<float*>(tile), a.out + (int64_t)vt * 64, a.out_ld, b_first * a.N, lane);

    // one row of the lane's recurrences: y = output of the current block's chain; WARM rows also advance the
    // next block's warm-up chain on the same input
    auto chains = [&](const double (&x)[VPT], double (&y)[VPT], double (&w0)[VPT], double (&w1)[VPT], auto warm_tag) {
        constexpr bool WARM = decltype(warm_tag)::value;
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            y[i] = x[i] + z0[i];                                               // DF2T of [1, s2, 1] / [1, a1, a2]
            z0[i] = fma(na1[i], y[i], fma(s2, x[i], z1[i]));
            z1[i] = fma(na2[i], y[i], x[i]);
            if (WARM) {
                const double yw = x[i] + w0[i];
                w0[i] = fma(ROWS ? wna1[i] : na1[i], yw, fma(s2, x[i], w1[i]));
                w1[i] = fma(ROWS ? wna2[i] : na2[i], yw, x[i]);
            }
        }
    };
    auto to_tile = [&](const double (&y)[VPT], double* where, int stride = kTileStride) {
#pragma unroll
        for (int ch = 0; ch < CC; ++ch) {
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < VPT; ++i) acc = fma(wt[ch][i], y[i], acc);
            where[ch * stride] = acc;
        }
    };
    sig_bus::FoldedGroup<CC> folded(tile, lane, dstp);                         // whole groups of R rows: sums folded in registers
    auto to_out = [&](const double (&y)[VPT], int64_t out_row) {
        if constexpr (MIX) {                                                   // rows arrive in order: stage, multiply every 32
            sink.stage((float)(y[0] * wt[0][0]));
            return;
        }
        float y32[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) y32[i] = (float)(y[i] * wt[0][i]);
        if (live0) {
            Vec o; put(o, y32);
            *reinterpret_cast<Vec*>(dst + out_row * a.out_ld) = o;
        }
    };

    // `count` consecutive rows from n_cur on; OUT rows go to output rows out_row, out_row + 1, ...
    auto walk = [&](int count, int64_t out_row, double (&w0)[VPT], double (&w1)[VPT], auto out_tag, auto warm_tag, auto fast_tag, auto pair_tag, int64_t blk) {
        constexpr bool OUT = decltype(out_tag)::value, FAST = decltype(fast_tag)::value;
        double hz[VPT], ph[VPT], q_lane = 0.0;
        int64_t qbase = 0;
        bool q_valid = false;
        if (!FAST) load_hz_ph(hz, ph, blk);
        if constexpr (FAST && ROWS) {
            if (fm && blk != seeded_blk) {                                     // wave-uniform: a new block's hertz / phase
                seed_sine(blk, n_cur, n_cur);
                seeded_blk = blk;
            }
        }
        // second oscillator of a Mix / RingMod source (ROWS kernels only; its waveform is a wave-uniform run-time switch)
        constexpr bool paired = ROWS && decltype(pair_tag)::value;               // (a compile-time copy of the row code: a run-time test per row cut the groups into pieces)
        double hz2[ROWS ? VPT : 1], ph2[ROWS ? VPT : 1], mx[ROWS ? VPT : 1];
        if constexpr (ROWS) {
            if (paired) {
#pragma unroll
                for (int i = 0; i < VPT; ++i) {
                    const int v = (v0 + i < a.voices) ? v0 + i : vc;
                    hz2[i] = a.hertz2[(int64_t)v * a.hs2];
                    ph2[i] = a.phase2 ? a.phase2[(int64_t)v * a.ps2] : 0.0;
                    mx[i] = a.mixrow ? a.mixrow[(int64_t)v * a.ms] : 0.0;
                }
            }
        }
        // exact phase: n/rate (IEEE divide) for 64 rows at a time, one row per lane (osc.py:32)
        auto ensure = [&](int rows) {
            if ((!FAST || paired) && (!q_valid || n_cur + rows > qbase + SIG_WAVE)) {     // wave-uniform
                qbase = n_cur;
                q_lane = (double)(qbase + lane) / a.rate;
                q_valid = true;
            }
        };
        auto gen = [&](double (&x)[VPT], int k) {                              // sample of row n_cur + k
            if (FAST) {
#pragma unroll
                for (int i = 0; i < VPT; ++i) {
                    x[i] = sx[i];
                    sx[i] = x[i] + sdl[i];
                    sdl[i] = fma(snm[i], sx[i], sdl[i]);
                }
            } else {
                const double t_s = sig_readlane_f64(q_lane, (int)(n_cur - qbase) + k);
#pragma unroll
                for (int i = 0; i < VPT; ++i) {
                    const double t = t_s * hz[i] + ph[i];
                    x[i] = (KIND == SIG_OSC_SINE) ? (double)sig_osc::osc_sine_f32(t) : sig_osc::osc_wave_fused<KIND>(t);
                }
            }
            if constexpr (ROWS) {
                if (paired) {                                                  // x = mix * A + (1 - mix) * B (fx.py:38-40) or A * B (fx.py:45-46)
                    const double t_s = sig_readlane_f64(q_lane, (int)(n_cur - qbase) + k);
#pragma unroll
                    for (int i = 0; i < VPT; ++i) {
                        const double t = t_s * hz2[i] + ph2[i];
                        double b;
                        switch (a.kind2) {                                     // wave-uniform
                            case SIG_OSC_SINE: b = (double)sig_osc::osc_sine_f32(t); break;
                            case SIG_OSC_SQUARE: b = sig_osc::osc_square_fract(t); break;
                            case SIG_OSC_SAWTOOTH: b = sig_osc::osc_sawtooth_fract(t); break;
                            default: b = sig_osc::osc_triangle_fract(t); break;
                        }
                        x[i] = (a.pair_op == 1) ? mx[i] * x[i] + (1.0 - mx[i]) * b : x[i] * b;
                    }
                }
            }
        };
        int done = 0;
        // the exact-phase Sine path is the rare one (positions beyond 2^26 cycles): rolled loops, so that its
        // register needs do not set the kernel's budget
        constexpr bool GROUPED = FAST || KIND != SIG_OSC_SINE || ROWS;           // (ROWS: under block-rate FM the exact phase IS the Sine path)
        if (!OUT || !BUS) {
            constexpr int U = GROUPED ? 4 : 1;                                 // rows per unrolled step
            for (; done + U <= count; done += U) {
                ensure(U);
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    double x[VPT], y[VPT];
                    gen(x, k);
                    chains(x, y, w0, w1, warm_tag);
                    if (OUT) to_out(y, out_row + done + k);
                }
                n_cur += U;
            }
            for (; done < count; ++done) {
                double x[VPT], y[VPT];
                ensure(1);
                gen(x, 0);
                chains(x, y, w0, w1, warm_tag);
                if (OUT) to_out(y, out_row + done);
                ++n_cur;
            }
            return;
        }
        auto single = [&]() {
            double x[VPT], y[VPT];
            ensure(1);
            gen(x, 0);
            chains(x, y, w0, w1, warm_tag);
            to_tile(y, stage.slot);
            ++n_cur; ++done;
            stage.advance();
        };
        while (stage.staged != 0 && done < count) single();                    // until the tile is empty
        double pend[4];
        int64_t pend_row = 0;
        bool have = false;
        for (; GROUPED && done + R <= count; done += R) {                      // whole groups: sums in registers, folded across lanes
            ensure(R);                                                         // (sig_bus::FoldedGroup), the flush one group behind
            double acc[kPairs];
#pragma unroll
            for (int k = 0; k < R; ++k) {
                double x[VPT], y[VPT];
                gen(x, k);
                chains(x, y, w0, w1, warm_tag);
                to_tile(y, acc + k * CC, 1);
#pragma unroll
                for (int g = 0; g < kPairs / 4; ++g)
                    if (4 * g + 3 < (k + 1) * CC && 4 * g + 3 >= k * CC)
                        folded.fold4(g, acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
                if (k + 1 == R / 2 && have) folded.finish(pend, pend_row, R);
            }
            n_cur += R;
            folded.issue(pend);
            pend_row = stage.first; stage.first += R; have = true;
        }
        if (have) folded.finish(pend, pend_row, R);
        while (done < count) single();
    };
    // `blk`: the block whose hertz / phase rows these rows were made with (only read under block-rate FM)
    auto walk_any = [&](int count, int64_t out_row, double (&w0)[VPT], double (&w1)[VPT], auto out_tag, auto warm_tag, int64_t blk) {
        if constexpr (ROWS) {
            if (a.pair_op != 0) {                                              // wave-uniform
                if (KIND == SIG_OSC_SINE && fast) walk(count, out_row, w0, w1, out_tag, warm_tag, std::true_type{}, std::true_type{}, blk);
                else walk(count, out_row, w0, w1, out_tag, warm_tag, std::false_type{}, std::true_type{}, blk);
                return;
            }
        }
        if (KIND == SIG_OSC_SINE && fast) walk(count, out_row, w0, w1, out_tag, warm_tag, std::true_type{}, std::false_type{}, blk);
        else walk(count, out_row, w0, w1, out_tag, warm_tag, std::false_type{}, std::false_type{}, blk);
    };

    walk_any(c0, 0, z0, z1, std::false_type{}, std::false_type{}, b_first - 1);   // warm-up of the span's first block: the previous block's samples
    for (int bi = 0; bi < nb; ++bi) {
        const int64_t orow = (b_first + bi) * a.N;
        const int tail = (bi + 1 < nb) ? a.ctx : 0;                            // rows that also warm the next block up (N >= ctx)
        walk_any(a.N - tail, orow, z0, z1, std::true_type{}, std::false_type{}, b_first + bi);
        if (tail) {
            double w0[VPT], w1[VPT];                                           // the next block's chain, from zero state
#pragma unroll
            for (int i = 0; i < VPT; ++i) { w0[i] = 0.0; w1[i] = 0.0; }
            if constexpr (ROWS) {
                if (a.cutoff_rows > 1 || a.gain_rows > 1) {                    // (block-rate FM alone: one design for the launch)
                    design_block(b_first + bi + 1, wna1, wna2, [&](int ch, int i, double w) { wwt[ch][i] = w; });
                } else {
#pragma unroll
                    for (int i = 0; i < VPT; ++i) {
                        wna1[i] = na1[i]; wna2[i] = na2[i];
#pragma unroll
                        for (int ch = 0; ch < CC; ++ch) wwt[ch][i] = wt[ch][i];
                    }
                }
            }
            walk_any(tail, orow + a.N - tail, w0, w1, std::true_type{}, std::true_type{}, b_first + bi);
#pragma unroll
            for (int i = 0; i < VPT; ++i) { z0[i] = w0[i]; z1[i] = w1[i]; }
            if constexpr (ROWS) {
#pragma unroll
                for (int i = 0; i < VPT; ++i) {
                    na1[i] = wna1[i]; na2[i] = wna2[i];
#pragma unroll
                    for (int ch = 0; ch < CC; ++ch) wt[ch][i] = wwt[ch][i];
                }
            }
        }
    }
    if (BUS && stage.staged) stage.now();
    if constexpr (MIX) sink.finish();
}

template <int KIND, int VPT, bool GAIN, int C, bool ROWS = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Occ<VPT>::lo, Occ<VPT>::hi)))
void fused_walk_kernel(FusedArgs a, BusArgs bus)
{
    constexpr bool BUS = C > 0, MIX = C < 0;
    __shared__ __attribute__((aligned(16))) double lds[(BUS || MIX) ? 4 : 1][BUS ? kPairs * kTileStride : (MIX ? sig_mix::kTileRows * sig_mix::kLdsStride / 2 : 1)];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);        // wave-uniform by construction: block / tile indices in SGPRs
    walk_wave<KIND, VPT, GAIN, C, ROWS>(a, bus, lds[(BUS || MIX) ? wave : 0], lane, wave);
    if constexpr (BUS) {
        if (bus.out) sig_bus::sum_tiles_in_workgroup<C>(bus.partials, a.voice_tiles, bus.rows, a.span, a.K, a.N, bus.out, bus.out_ld, lane, wave);
    }
}

template <int KIND, bool GAIN, int C, bool ROWS = false>
int launch_walk(FusedArgs a, BusArgs bus, int vpt, hipStream_t stream)
{
    a.voice_tiles = sig_voice_tiles(a.voices, vpt);
    unsigned nwg;
    if (!sig_workgroups(sig_span_waves(a.voice_tiles, a.K, a.span), nwg)) return (int)hipErrorInvalidValue;
    if constexpr (C < 0) {
        fused_walk_kernel<KIND, 1, GAIN, C, ROWS><<<nwg, 256, 0, stream>>>(a, bus);
    } else {
        switch (vpt) {
            case 1: fused_walk_kernel<KIND, 1, GAIN, C, ROWS><<<nwg, 256, 0, stream>>>(a, bus); break;
            case 2: fused_walk_kernel<KIND, 2, GAIN, C, ROWS><<<nwg, 256, 0, stream>>>(a, bus); break;
            case 4: fused_walk_kernel<KIND, 4, GAIN, C, ROWS><<<nwg, 256, 0, stream>>>(a, bus); break;
            default: return (int)hipErrorInvalidValue;
        }
    }
    return sig_launch_status();
}

}  // namespace
