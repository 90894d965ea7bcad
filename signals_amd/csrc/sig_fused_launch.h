// Launch planning of the fused voice chain: which kernel (span walker, Sine closed form, latency scan) takes a problem, and
// with which geometry.  Included by the translation units that instantiate the kernels (fused_voice.hip, fused_voice_b.hip).
#pragma once
#include <type_traits>

#include "sig_fused_scan.h"
#include "sig_fused_steady.h"
#include "sig_fused_walk.h"

namespace {

// Launch geometry (tools/sweep_fused.sh).  Voices per lane: 4 amortises the per-row work shared by a lane's voices
// (bus staging, loop control) best and leaves room for two waves per SIMD.  Blocks per lane (span): the first
// block of a span pays a c-row warm-up that computes the oscillator only for the filter, so longer spans waste
// less -- but a lane walks its rows serially and one wave per SIMD cannot keep the f64 pipe busy, so the span
// only grows while the launch still has two waves per SIMD; and in the latency regime (one block, few voices)
// the voices are spread over more, shorter waves instead.
constexpr int64_t kWavesWanted = 2048;     // two waves per SIMD

// waves of a launch with `v` voices per lane and `s` blocks per lane
int64_t waves_of(const FusedArgs& a, int v, int s) { return sig_span_waves(sig_voice_tiles(a.voices, v), a.K, s); }

void pick_geometry(const FusedArgs& a, int max_vpt, int& vpt, int& span) {
    const int env_vpt = tuning().vpt, env_span = tuning().span;               // tuning / test hooks
    const int max_span = (a.N >= a.ctx) ? 8 : 1;
    vpt = max_vpt; span = max_span;
    while (span > 1 && waves_of(a, vpt, span) < kWavesWanted) span >>= 1;
    while (vpt > 1 && waves_of(a, vpt, 1) < kWavesWanted / 2) vpt >>= 1;
    if (env_vpt == 1 || env_vpt == 2 || env_vpt == 4) vpt = (env_vpt <= max_vpt) ? env_vpt : max_vpt;
    if (env_span >= 1) span = (env_span <= max_span) ? env_span : max_span;
}

struct BusPlan { int vpt, span, steady; };

// What sig_fused_voice_bus launches for this problem: voices per lane, blocks per lane, and whether the Sine closed
// form (fused_steady_bus_kernel) takes the launch.  One decision function for the launcher and for
// sig_fused_voice_bus_plan (tests and bench.py name the kernel they time with it).
BusPlan plan_voice_bus(const FusedArgs& a, int kind) {
    BusPlan p{4, 1, 0};
    pick_geometry(a, 4, p.vpt, p.span);
    if (kind == SIG_OSC_SINE && !a.force_walk && (a.N >= a.ctx || a.position >= a.ctx)) {   // at most the first block has a short context
        p.steady = tuning().steady < 0 ? 1 : tuning().steady;                  // tuning / test hook
        if (p.steady) {
            // the closed form needs few registers per voice: 8 voices per lane (one wave per SIMD, 302 registers) beat
            // 4 (two waves) by 5 % when the launch still has a wave for every SIMD -- half the flushes per sample
            // Better still 16 (the cross-lane flush -- 16 LDS stores and 16 loads per lane per 8 rows, the kernel's real
            // bottleneck: 13 + 8 cycles of the CU's LDS path per pair, shared by four SIMDs -- is paid per LANE and row,
            // so its cost per voice-sample halves), with shorter spans if that is what keeps a wave on every SIMD.
            const int env_vpt = tuning().vpt;                                  // tuning / test hook
            if (env_vpt == 8 || (env_vpt == 0 && p.vpt == 4 && waves_of(a, 8, p.span) >= kWavesWanted / 2)) p.vpt = 8;
            if (env_vpt == 16 || (SIG_STEADY_AUTO16 && env_vpt == 0 && p.vpt == 8 && a.voices >= SIG_WAVE * 16)) {
                int span = p.span;
                while (span > 1 && waves_of(a, 16, span) < kWavesWanted / 2) span >>= 1;
                if (env_vpt == 16 || waves_of(a, 16, span) >= kWavesWanted / 2) {
                    p.vpt = 16;
                    if (tuning().span == 0) p.span = span;
                }
            }
        }
    }
    return p;
}

// the per-block-parameter entry points (sig_fused_osc_biquad_rows, sig_fused_voice_bus_rows, *_fm, *_pair): the walker --
// except a Sine voice whose ONLY per-block parameter is its gain (a tremolo), which keeps the closed form with the bus
// weights rebuilt at every block's first row (fused_steady_bus_kernel<.., GROWS = true>)
template <int KIND, int C>
int launch_rows(FusedArgs a, BusArgs bus, float* out, int64_t out_ld, hipStream_t stream)
{
    if constexpr (KIND == SIG_OSC_SINE && C > 0) {
        const bool gain_only = a.gain && a.gain_rows > 1 && a.cutoff_rows == 1;
        if ((gain_only || a.cutoff_rows > 1) && !a.hertz_hist && !a.phase_hist && a.pair_op == 0) {
            BusPlan plan = plan_voice_bus(a, KIND);
            if (plan.steady) {
                if (plan.vpt > 8) plan.vpt = 8;
                // per-block constants: 8 voices per lane where the launch is big enough for them (one wave per SIMD; the per-span
                // oscillator parts then live in LDS -- in registers the kernel passed 512 and spilled 132, 20 us of scratch round
                // trips per block), else 2 (195 registers: two waves per SIMD under the constants' long dependent chains; 4 need
                // 335 and run one wave, 7 % slower than 2).  Tuning hook: as forced
                if (!gain_only && tuning().vpt == 0) plan.vpt = (plan.vpt >= 8) ? 8 : (plan.vpt > 2 ? 2 : plan.vpt);
                a.span = plan.span;
                a.steady = 1;
                // a swept cutoff (with or without a tremolo): per-(block, voice) filter constants; a tremolo alone: the bus
                // weights rebuilt per block
                const int err = gain_only ? launch_steady<false, C, true>(a, bus, plan.vpt, out, out_ld, stream)
                                          : launch_steady<false, C, true, true>(a, bus, plan.vpt, out, out_ld, stream);
                if (err || bus.out) return err;
                const int tiles_s = sig_voice_tiles(a.voices, plan.vpt);
                return sig_bus::launch_partials<C>(bus.partials, tiles_s, bus.rows, out, out_ld, stream);
            }
        }
    }
    auto ok = [&](int vpt) {
        return C > 0 || ((a.voices % vpt == 0) && (a.out_ld % vpt == 0) && (reinterpret_cast<uintptr_t>(a.out) % (vpt * 4) == 0));
    };
    int max_vpt = 4;
    while (max_vpt > 1 && !ok(max_vpt)) max_vpt >>= 1;
    int vpt;
    pick_geometry(a, max_vpt, vpt, a.span);
    const int tiles = sig_voice_tiles(a.voices, vpt);
    if (C > 0 && sig_bus::tiles_sum_in_workgroup(tiles) && tuning().tile_sum_kernel == 0) { bus.out = out; bus.out_ld = out_ld; }
    const int err = launch_walk<KIND, false, C, true>(a, bus, vpt, stream);
    if (err || C == 0 || bus.out) return err;
    return sig_bus::launch_partials<(C > 0 ? C : 1)>(bus.partials, tiles, bus.rows, out, out_ld, stream);
}

template <int KIND, bool GAIN, int C>
int launch_voice_bus(FusedArgs a, BusArgs bus, float* out, int64_t out_ld, hipStream_t stream)
{
    const BusPlan plan = plan_voice_bus(a, KIND);
    const int vpt = plan.vpt;
    a.span = plan.span;
    a.steady = plan.steady;
    bool done = false;
    if constexpr (KIND == SIG_OSC_SINE) {                                      // (the closed form exists for a sinusoid only: not instantiated for the others)
        if (a.steady) {
            const int e2 = launch_steady<GAIN, C, false>(a, bus, vpt, out, out_ld, stream);
            if (e2 || bus.out) return e2;                                      // (the kernel added the voice tiles itself)
            done = true;
        }
    }
    if (!done) {                                                               // (Sine with the closed form: that launch did every wave)
        const int tiles_w = sig_voice_tiles(a.voices, vpt);
        if (sig_bus::tiles_sum_in_workgroup(tiles_w) && tuning().tile_sum_kernel == 0) { bus.out = out; bus.out_ld = out_ld; }
        const int err = launch_walk<KIND, GAIN, C>(a, bus, vpt, stream);
        if (err || bus.out) return err;                                        // (the kernel added the voice tiles itself)
    }
    const int tiles = sig_voice_tiles(a.voices, vpt);
    return sig_bus::launch_partials<C>(bus.partials, tiles, bus.rows, out, out_ld, stream);
}

template <int KIND, bool GAIN>
int dispatch_bus_channels(int C, const FusedArgs& a, const BusArgs& bus, float* out, int64_t out_ld, hipStream_t s)
{
    switch (C) {
#ifndef SIG_TUNE_SINE_ONLY
        case 1: return launch_voice_bus<KIND, GAIN, 1>(a, bus, out, out_ld, s);
        case 4: return launch_voice_bus<KIND, GAIN, 4>(a, bus, out, out_ld, s);
#endif
        case 2: return launch_voice_bus<KIND, GAIN, 2>(a, bus, out, out_ld, s);
    }
    return (int)hipErrorInvalidValue;
}

template <int KIND, bool GAIN>
int launch_fused(FusedArgs a, hipStream_t stream)
{
    {
        const int scan_env = tuning().scan;                                    // tuning / test hook
        const int64_t chains = (int64_t)a.voices * a.K;
        const bool fits = a.ctx + a.N <= kScanMaxL * SIG_WAVE;
        const bool want = scan_env >= 0 ? scan_env != 0 : chains <= kScanMaxChains;
        if (fits && want) {
            unsigned nwg;
            if (!sig_workgroups(chains, nwg)) return (int)hipErrorInvalidValue;
            fused_scan_kernel<KIND, GAIN><<<nwg, 256, 0, stream>>>(a);
            return sig_launch_status();
        }
    }
    auto ok = [&](int vpt) {
        return (a.voices % vpt == 0) && (a.out_ld % vpt == 0) && (reinterpret_cast<uintptr_t>(a.out) % (vpt * 4) == 0);
    };
    int max_vpt = 4;
    while (max_vpt > 1 && !ok(max_vpt)) max_vpt >>= 1;
    int vpt;
    pick_geometry(a, max_vpt, vpt, a.span);
    return launch_walk<KIND, GAIN, 0>(a, BusArgs{nullptr, 0, nullptr, 0}, vpt, stream);
}

template <int KIND, bool GAIN>
int launch_mix(FusedArgs a, hipStream_t stream)
{
    int vpt;
    pick_geometry(a, 1, vpt, a.span);                                          // one voice per lane: a wave = one matrix group
    if (KIND == SIG_OSC_SINE && (tuning().steady < 0 ? 1 : tuning().steady)) { // closed form per wave (or its built-in plain fallback)
        // (fused_mix.hip; blocks per wave: see launch_steady_mix)
        if (tuning().span == 0) a.span = 0;
        a.voice_tiles = a.voices / SIG_WAVE;
        a.steady = tuning().mix_f32 ? 3 : 1;
        return launch_steady_mix(a, GAIN, stream);
    }
    return launch_walk<KIND, GAIN, -1>(a, BusArgs{nullptr, 0, nullptr, 0}, 1, stream);
}


// Which oscillator kinds a translation unit instantiates -- the one place that says so.  fused_voice.hip: Sine here, the others
// behind the plain functions part_b_* (sig_steady.h); fused_voice_b.hip (SIG_FUSED_PART_B): the others; a tuning build
// (tools/build_variant.sh -DSIG_TUNE_SINE_ONLY): Sine alone, one unit.  `here` gets the kind as a std::integral_constant.
template <class Here, class PartB>
int dispatch_osc_kind(int kind, Here here, PartB part_b)
{
    switch (kind) {
#if defined(SIG_FUSED_PART_B)
        case SIG_OSC_SQUARE: return here(std::integral_constant<int, SIG_OSC_SQUARE>{});
        case SIG_OSC_SAWTOOTH: return here(std::integral_constant<int, SIG_OSC_SAWTOOTH>{});
        case SIG_OSC_TRIANGLE: return here(std::integral_constant<int, SIG_OSC_TRIANGLE>{});
#else
        case SIG_OSC_SINE: return here(std::integral_constant<int, SIG_OSC_SINE>{});
#if !defined(SIG_TUNE_SINE_ONLY)
        case SIG_OSC_SQUARE: case SIG_OSC_SAWTOOTH: case SIG_OSC_TRIANGLE: return part_b();
#endif
#endif
    }
    return (int)hipErrorInvalidValue;
}

// the four launch families by run-time kind (and gain / sink); fused_voice_b.hip exports its side of them as part_b_*
int dispatch_chain(bool gain, int kind, const FusedArgs& a, hipStream_t s)
{
    return dispatch_osc_kind(kind,
        [&](auto k) { constexpr int KIND = decltype(k)::value; return gain ? launch_fused<KIND, true>(a, s) : launch_fused<KIND, false>(a, s); },
        [&] { return part_b_chain(gain, kind, a, s); });
}

int dispatch_mix(bool gain, int kind, const FusedArgs& a, hipStream_t s)
{
    return dispatch_osc_kind(kind,
        [&](auto k) { constexpr int KIND = decltype(k)::value; return gain ? launch_mix<KIND, true>(a, s) : launch_mix<KIND, false>(a, s); },
        [&] { return part_b_mix(gain, kind, a, s); });
}

int dispatch_bus(bool gain, int kind, int C, const FusedArgs& a, const BusArgs& bus, float* out, int64_t out_ld, hipStream_t s)
{
    return dispatch_osc_kind(kind,
        [&](auto k) {
            constexpr int KIND = decltype(k)::value;
            return gain ? dispatch_bus_channels<KIND, true>(C, a, bus, out, out_ld, s) : dispatch_bus_channels<KIND, false>(C, a, bus, out, out_ld, s);
        },
        [&] { return part_b_bus(gain, kind, C, a, bus, out, out_ld, s); });
}

// C: 0 (per-voice rows), or the 1 or 2 channels of a bus (4-channel buses with per-block parameters: the per-node schedule)
int dispatch_rows(int C, int kind, const FusedArgs& a, const BusArgs& bus, float* out, int64_t out_ld, hipStream_t s)
{
    return dispatch_osc_kind(kind,
        [&](auto k) {
            constexpr int KIND = decltype(k)::value;
            switch (C) {
                case 0: return launch_rows<KIND, 0>(a, bus, out, out_ld, s);
                case 1: return launch_rows<KIND, 1>(a, bus, out, out_ld, s);
                case 2: return launch_rows<KIND, 2>(a, bus, out, out_ld, s);
            }
            return (int)hipErrorInvalidValue;
        },
        [&] { return part_b_rows(C, kind, a, bus, out, out_ld, s); });
}

}  // namespace
