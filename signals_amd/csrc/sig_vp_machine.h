// A whole frame-rate voice graph in ONE launch, gfx950: the general form of the fused voice kernels.
//
// The fused kernels of sig_fused_*.h / fused_cascade.hip each cover one graph shape (Filter(Osc), Filter(Filter(Osc)) ...).
// Everything else -- an Amp or a Mix behind a filter, RingMod of two filtered voices, three filters in series, block-rate
// FM together with a second oscillator, blocks shorter than the filter context -- ran one kernel per node (24+ B per
// voice-sample through HBM) or, for short blocks, the eager pull path (~150 us per block).  Here the per-voice graph is
// compiled on the host into a short straight-line program for an ACCUMULATOR MACHINE and interpreted per row by every
// lane for its own voices (lanes = voices, like the walkers): the accumulator and a few temporaries live in VGPRs, the
// program word of instruction pc sits in lane pc of one VGPR and is fetched with v_readlane (a wave-uniform scalar), the
// dispatch is a scalar compare chain.  State arrays (filter slots, oscillator slots, parameter registers, temporaries)
// are indexed by a wave-uniform slot number through a compile-time switch, so they stay in registers.
//
// What makes one machine enough for every shape is the reference's block structure, reproduced as a sequence of blocks:
//   * a filter answers a block from ZERO state over [<=100 context rows | block] (CritFilter._filter, fx.py:85-106);
//   * with blocks longer than the context, the context rows in front of block j are the input's rows of block j - 1: the
//     input keeps its previous block cached and the context request is a slice of it (BlockCachingEmitter,
//     chain/__init__.py:431-442) -- for a filter input that block was itself cold-started 100 rows before block j - 1;
//   * every node reads its control ports once per block, at the block's position (forward_at_block_rate,
//     chain/__init__.py:305-306).
// So every filter slot carries TWO recurrences: the CURRENT block's chain, and -- over the last min(100, .) rows of a
// block -- the NEXT block's chain, cold-started there on the same input (the current block's values, which is exactly
// what the cache serves as context) with the next block's design.  At a block boundary next becomes current.  A lane
// that starts its span at block b first re-walks the D - 1 blocks in front of it (D = filters in series) plus 100 rows:
// a filter at level l of the cascade is exact from block b - D + l on (induction over levels), so level D is exact from
// block b.  In front of the launch those are the previous render's blocks, or on a fresh graph the virtual 100-row
// blocks the reference's context requests create ([p - 100, p) answered as a block of its own, controls read at p - 100).
// Blocks SHORTER than the context (PortAudio callbacks of 32 or 64 frames): a context request then lies in no single
// cached block, and the reference answers it as a block of its own for EVERY block -- each output block is walked on its
// own behind its virtual block (controls read at max(p - 100, 0)); two filters in series at most in that mode.
//
// Arithmetic: f64 throughout, exact per-row phase t = n / rate * hertz + phase (osc.py:32, one IEEE divide per row shared
// by the wave), Butterworth design per block in-kernel (sig_biquad.h), b0-normalised DF2T recurrence (4 FMAs + 1).  No
// float32 rounding between nodes: closer to the f64 reference than the per-node schedule; 1e-6 parity by test.
//
// This header is the DEVICE half: the argument blocks, the family descriptors, the machine (vp_wave) and the kernels.  The host
// half (validation, geometry, launch, the C entries) is voice_program.hip; the interpreter's kernels are instantiated one family
// per file (vp_<family>.hip, through sig_vp_launch.h); voice_program.hip built with -DSIG_VP_STATIC_CODE is the specialised kernel.
#pragma once
#include <cstdint>
#include <type_traits>

#include "sig_adsr.h"
#include "sig_biquad.h"
#include "sig_bus_tile.h"
#include "sig_noise.h"
#if defined(SIG_BLEP_SKIP) && SIG_BLEP_SKIP
#error "SIG_BLEP_SKIP is a tuning build of osc_bank.hip alone: the OscBlep handler's lanes were not examined for its ballot"
#endif
#include "sig_osc.h"
#include "sig_table.h"

// The argument blocks and the family descriptors cross translation units (voice_program.hip fills them, vp_<family>.hip launches
// with them), so they have a namespace with a name; the device code below is each unit's own.
namespace sig_vp {

constexpr int kMaxIns = SIG_VP_MAX_INS;
#ifndef SIG_VP_ROWS
#define SIG_VP_ROWS 8
#endif
constexpr int kRowGroup = SIG_VP_ROWS;     // the interpreter runs every instruction for this many consecutive rows at a time: its dispatch
                                           // (fetch, decode, two scalar switches) is paid once per group, and a handler has rows x voices
                                           // independent evaluations to overlap

struct Rows { const double* ptr; int cs; int rows; };      // (rows, V | 1) float64: rows == 1 holds for every block

struct VpArgs {
    double rate; int64_t position; int N, K, ctx, voices;
    int n_ins; uint32_t code[kMaxIns];                       // op | kind << 5 | a << 8 | b << 12 | c << 16
    int n_oscs; Rows hertz[SIG_VP_MAX_OSCS], phase[SIG_VP_MAX_OSCS];
    int n_params; Rows params[SIG_VP_MAX_PARAMS];
    int n_filters; Rows cutoff[SIG_VP_MAX_FILTERS]; int ftype[SIG_VP_MAX_FILTERS]; int flevel[SIG_VP_MAX_FILTERS];
    sig_env::AdsrRows adsr; int has_adsr;
    uint64_t seeds[2];
    int depth, hist, small, blocks_before; int64_t hist_pos[SIG_VP_MAX_HIST];
    int span, voice_tiles;
    float* out; int64_t out_ld;                              // store sink
    const double* pan; int64_t pan_ld; double* partials; int64_t rows; float* bus_out; int64_t bus_out_ld;   // bus sink
    int* status;
};

// The wavetables of the OscTable instruction: (T, W) float32, staged in LDS.  A kernel parameter of its own that only the TAB
// variant has, so that the argument block -- and with it the code -- of every other instantiation is what it was without the op.
struct VpTables { const float* ptr[SIG_VP_MAX_TABLES]; int T[SIG_VP_MAX_TABLES], W[SIG_VP_MAX_TABLES]; };
struct VpNoTables {};
// The copies of the OscUni instruction (unison oscillators, ext.py UnisonOsc): relative detune and phase offset per copy, by value.
// Travels the way VpTables does -- a second kernel parameter that only the UNI variant has -- and for the same reason.  Wave-uniform:
// the handler's loop count and both values are scalars.
struct VpUnison { int copies; double detune[SIG_UNISON_MAX_COPIES], offset[SIG_UNISON_MAX_COPIES]; };
// Both at once, for the MIXED variant (programs that combine two or more of Band, OscPM, OscTable / Shape, FilterQ and OscUni): the
// fields of VpTables followed by those of VpUnison.  The names are disjoint, so the handlers read tb.ptr / T / W and tb.copies /
// detune / offset from it as they do from the one they were written for.
struct VpMixed {
    const float* ptr[SIG_VP_MAX_TABLES]; int T[SIG_VP_MAX_TABLES], W[SIG_VP_MAX_TABLES];
    int copies; double detune[SIG_UNISON_MAX_COPIES], offset[SIG_UNISON_MAX_COPIES];
};

}  // namespace sig_vp

namespace {

using namespace sig_vp;
using sig_biquad::Biquad;
using sig_bus::kTileStride;

// f(integral_constant<int, i>) for a wave-uniform i < N: a scalar switch, so arrays indexed inside stay in registers
template <int N, typename F>
__device__ __forceinline__ void with_index(int i, F&& f) {
    switch (i) {
        case 0: if constexpr (N > 0) f(std::integral_constant<int, 0>{}); break;
        case 1: if constexpr (N > 1) f(std::integral_constant<int, 1>{}); break;
        case 2: if constexpr (N > 2) f(std::integral_constant<int, 2>{}); break;
        case 3: if constexpr (N > 3) f(std::integral_constant<int, 3>{}); break;
        case 4: if constexpr (N > 4) f(std::integral_constant<int, 4>{}); break;
        case 5: if constexpr (N > 5) f(std::integral_constant<int, 5>{}); break;
        case 6: if constexpr (N > 6) f(std::integral_constant<int, 6>{}); break;
        case 7: if constexpr (N > 7) f(std::integral_constant<int, 7>{}); break;
        default: break;
    }
}

// An opaque copy of a wave-uniform double.  A handler's arithmetic on the row's n / rate and the slot's block-invariant
// registers does not depend on the instruction counter, so the optimiser hoists it out of the instruction loop and evaluates
// EVERY case of every slot once per row, unconditionally (measured: all four waveforms of all oscillator slots per row, ~10x
// the work of the program itself and twice the registers).  Passing an input through an empty volatile asm pins the work to
// the case that needs it.
__device__ __forceinline__ double vp_pin(double x) {
    asm volatile("" : "+s"(x));
    return x;
}

// sig_biquad.h's design_butter2 with a light tangent: libm's tan() carries a Payne-Hanek reduction for huge arguments whose
// temporaries set the register budget of the whole kernel (+110 VGPRs, measured), and the argument here is pi Wn / 2 with
// Wn in (0, 1): tan = sin / cos from the odd polynomial of sig_osc.h on [0, pi/2], cos(x) = sin(pi/2 - x) with pi/2 as hi + lo.
// Coefficients within 1e-15 (relative) of the libm form.
struct VpTan {                                              // tan(x), x in [0, pi/2]
    __device__ __forceinline__ double operator()(double x) const {
        const double xc = (1.5707963267948966 - x) + 6.123233995736766e-17;
        return sig_osc::sin_poly(x) / sig_osc::sin_poly(xc);
    }
};
__device__ __forceinline__ bool vp_design(int type, double cutoff, double rate, Biquad& q) {
    double wn = cutoff / (rate * 0.5);                      // scaled_crit /= rate / 2  (fx.py:99-101)
    wn = (wn < 0.0) ? 0.0 : ((wn > 1.0) ? 1.0 : wn);
    const bool bad = !(wn > 0.0 && wn < 1.0);               // scipy raises (NaN too)
    const double x = sig_biquad::kPi * wn / 2.0;
    const double k = VpTan{}(x);
    const double k2 = k * k;
    const double nrm = 1.0 / (1.0 + sig_biquad::kSqrt2 * k + k2);
    q.b0 = (type == SIG_FILT_LOWPASS) ? k2 * nrm : nrm;
    q.a1 = 2.0 * (k2 - 1.0) * nrm;
    q.a2 = (1.0 - sig_biquad::kSqrt2 * k + k2) * nrm;
    if (bad) { q.b0 = q.a1 = q.a2 = __builtin_nan(""); }
    q.b1 = q.b2 = 0.0;                                      // (the recurrence is b0-normalised: b = b0 [1, +-2, 1])
    return !bad;
}

// vp_design with the damping as an argument: the resonant low-pass / high-pass of chain/ext.py (sig_biquad.h design_resonant2 with the
// light tangent), d = 1 / q -- one divide more per voice and block -- or sqrt2 for a Butterworth slot of the same program, which
// then gets vp_design's bits.  `lowpass`: the slot's response; `q_ok`: the resonance was finite and > 0 (or unplugged).  Returns 0 or
// the status bits of what was refused.
__device__ __forceinline__ int vp_design_res(bool lowpass, double cutoff, double d, bool q_ok, double rate, Biquad& q) {
    double wn = cutoff / (rate * 0.5);
    wn = (wn < 0.0) ? 0.0 : ((wn > 1.0) ? 1.0 : wn);
    const int bad = (!(wn > 0.0 && wn < 1.0) ? SIG_STATUS_BAD_CUTOFF : 0) | (q_ok ? 0 : SIG_STATUS_BAD_RESONANCE);
    const double x = sig_biquad::kPi * wn / 2.0;
    const double k = VpTan{}(x);
    const double k2 = k * k;
    const double nrm = 1.0 / (1.0 + d * k + k2);
    q.b0 = lowpass ? k2 * nrm : nrm;
    q.a1 = 2.0 * (k2 - 1.0) * nrm;
    q.a2 = (1.0 - d * k + k2) * nrm;
    if (bad) { q.b0 = q.a1 = q.a2 = __builtin_nan(""); }
    q.b1 = q.b2 = 0.0;
    return bad;
}

// The equaliser designs of a FilterEq slot (sig_biquad.h design_eq2 with the light tangent): all five coefficients, the numerator's
// three taps free.  `has_q` / `has_gain`: the control is plugged (else d = sqrt2 / 0 dB).  Returns 0 or the status bits.
__device__ __forceinline__ int vp_design_eq(int type, double cutoff, bool has_q, double qv, bool has_gain, double db, double rate, Biquad& q) {
    return sig_biquad::design_eq2(type, cutoff, has_q ? &qv : nullptr, has_gain ? &db : nullptr, rate, q, VpTan{});
}

__device__ __noinline__ double vp_amp(double x, double e) { return copysign(pow(x, e), x); }   // fx.py:60 (kept out of line: pow is long)

// Register-file sizes per variant (the host picks the smallest variant a program fits).  SMALL: two filter slots, three
// oscillator slots, four parameter registers, one temporary (a temporary is a whole row group: 8 rows x 2 voices = 32 VGPRs), no Amp / ADSR / White -- the common synthesiser voice; its
// state fits two waves per SIMD at two voices per lane, which the interpreter's scalar dispatch needs to hide its branches.
// The full register file (four filters, four oscillators, eight parameters, four temporaries, every instruction) runs at one.
template <bool SMALL> struct VpLimits {
#ifndef SIG_VP_S_NF
#define SIG_VP_S_NF 2
#define SIG_VP_S_NO 3
#define SIG_VP_S_NP 4
#define SIG_VP_S_NT 1
#endif
    static constexpr int NF = SMALL ? SIG_VP_S_NF : 4, NO = SMALL ? SIG_VP_S_NO : 4, NP = SMALL ? SIG_VP_S_NP : 8, NT = SMALL ? SIG_VP_S_NT : 4;
#ifdef SIG_VP_S_EXT
    static constexpr bool EXT = !SMALL || (SIG_VP_S_EXT != 0);
#else
    static constexpr bool EXT = !SMALL;
#endif
};

// C == 0: store (float) acc to a.out; C > 0: C bus channels into a.partials.  EXT: Amp, ADSR and White instructions.
// BAND: the Band instruction (band filters' per-voice middle taps and their design; a variant of its own, so that programs
// without one keep the registers they had -- the band state and its inlined design cost the SMALL file ~200 B of scratch per lane)
// PM: the OscPM instruction (phase-modulation carriers), a variant of its own for the same reason
// TAB: the OscTable and Shape instructions (wavetable oscillators and waveshapers, ext.py Wavetable / Shaper), likewise; `tab`: the launch's tables in LDS, each
// column-major with T + 1 floats per column (the guard entry [T] = [0], sig_table.h), table 1 behind table 0
// SHP: the Shape instruction on top of TAB, a variant of its own once more: with the handler in the one TAB variant the SMALL
// table kernels went from 260-312 to 412-472 B of scratch per lane, which wavetable-only programs would have paid
// RES: the FilterQ instruction (resonant low-pass / high-pass, ext.py ResonantFilter): slots of type SIG_FILT_RES_* whose design reads
// a second block-rate control, q, from the parameter rows the word names; a variant of its own (never with BAND, PM or TAB), so that
// programs without the word keep their registers and scratch.  Filter words run in it too
// UNI: the OscUni instruction (unison oscillators, ext.py UnisonOsc): the mean of the copies of one waveform; a variant of its own once
// more (never with BAND, PM, TAB or RES).  `tb` is then the variant's VpUnison: Extra is whatever second kernel parameter the
// variant has (VpTables, VpUnison) or VpNoTables
// BLP: the OscBlep instruction (band-limited oscillators, ext.py BlepOsc) on top of UNI, whose copies and operands it shares: a flag
// of its own, so that programs with OscUni alone keep the UNI variant's code (vp_family::blep has both handlers)
// EQ: the FilterEq instruction (the RBJ equaliser biquads, ext.py EqFilter) on top of RES, whose q scan and exclusions it shares:
// slots of type SIG_FILT_EQ_* with three free numerator taps (fb0 and eb1 / eb2; xb0 / xb1 / xb2 for the next block's chain) and a third
// block-rate control, the gain, from the parameter rows the word's b names.  A flag of its own -- a second set of kernels, RES+EQ
// (vp_family::resonant_eq) and MIXED+EQ (vp_family::mixed_eq), which the launch picks exactly when the program has the word -- so
// that programs without it keep the code of the RES and MIXED variants (the taps cost 5 x NF x VPT doubles of state)
// SYN: the OscSync instruction (hard-sync oscillators, ext.py SyncOsc) on top of BLP, whose copies, operands and residual it shares,
// with a fourth block-rate control, the ratio, from the parameter rows the word's b names.  A flag of its own and a second set of
// kernels once more -- BLP+SYN (vp_family::sync) and MIXED+SYN (vp_family::mixed_sync), picked by the launch exactly when the
// program has the word -- so that programs without it keep the code of the BLEP and MIXED variants.  Never with EQ
// The "never with" above is the single-family variants'.  The MIXED variant (vp_family::mixed, reached only through
// sig_voice_program_mixed) has all seven flags on and a VpMixed as `tb`.  What the flags share then, and why it holds:
//   * RES on: every LowPass / HighPass slot is designed by vp_design_res at d = sqrt2 (`single` is off), which are vp_design's bits;
//     band slots are neither `resonant` nor `plain` there and keep design_band2;
//   * a run of band slots pairs from its start whatever stands next to it: bfirst[f] looks only at bfirst[f - 1], and a resonant or
//     plain slot at f - 1 is never a band's first.  Two pairs cannot share f / 2 (that would take slots f, f + 1 and f + 1, f + 2);
//   * the qreg scan reads the FilterQ words alone, the handlers in front of the switch (FilterQ, OscUni, OscBlep, Shape, OscTable) each test
//     their own opcode and `continue`, so their order does not matter;
//   * with no table in the launch tb.ptr[0] is null and nothing is staged (no dynamic LDS is asked for either).
}  // namespace

namespace sig_vp {

// One interpreter variant: the flags above, and `Extra`, the second kernel parameter that follows from them (two or more of the
// five families: both the tables and the copies).
template <bool BAND_, bool PM_, bool TAB_, bool SHP_, bool RES_, bool UNI_, bool BLP_, bool EQ_, bool SYN_>
struct VpFamily {
    static constexpr bool BAND = BAND_, PM = PM_, TAB = TAB_, SHP = SHP_, RES = RES_, UNI = UNI_, BLP = BLP_, EQ = EQ_, SYN = SYN_;
    static_assert(BLP || !SYN, "OscSync sits on top of BLP");
    static_assert(TAB || !SHP, "Shape sits on top of TAB");
    static_assert(UNI || !BLP, "OscBlep sits on top of UNI");
    static_assert(RES || !EQ, "FilterEq sits on top of RES");
    static constexpr int families = (int)BAND + (int)PM + (int)TAB + (int)RES + (int)UNI;
    using Extra = std::conditional_t<(families >= 2), VpMixed,
                  std::conditional_t<TAB, VpTables, std::conditional_t<UNI, VpUnison, VpNoTables>>>;
};

// the nine variants the interpreter is built in, in the order of SIG_VP_FAMILY_* (include/signals_amd.h)
namespace vp_family {
//                       BAND   PM     TAB    SHP    RES    UNI    BLP    EQ     SYN
using plain    = VpFamily<false, false, false, false, false, false, false, false, false>;
using band     = VpFamily<true,  false, false, false, false, false, false, false, false>;
using pm       = VpFamily<false, true,  false, false, false, false, false, false, false>;
using table    = VpFamily<false, false, true,  false, false, false, false, false, false>;
using shape    = VpFamily<false, false, true,  true,  false, false, false, false, false>;
using resonant = VpFamily<false, false, false, false, true,  false, false, false, false>;
using unison   = VpFamily<false, false, false, false, false, true,  false, false, false>;
using blep     = VpFamily<false, false, false, false, false, true,  true,  false, false>;
using mixed    = VpFamily<true,  true,  true,  true,  true,  true,  true,  false, false>;
// the second set of RESONANT and MIXED, for programs with a FilterEq word (no SIG_VP_FAMILY_* of their own: the launch picks them)
using resonant_eq = VpFamily<false, false, false, false, true, false, false, true, false>;
using mixed_eq    = VpFamily<true,  true,  true,  true,  true, true,  true,  true, false>;
// the second set of BLEP and MIXED, for programs with an OscSync word (likewise picked by the launch; never together with FilterEq)
using sync       = VpFamily<false, false, false, false, false, true, true, false, true>;
using mixed_sync = VpFamily<true,  true,  true,  true,  true,  true, true, false, true>;
}  // namespace vp_family

}  // namespace sig_vp

namespace {

template <int VPT, bool SMALL, int C, typename FAM>
__device__ __forceinline__ void vp_wave(const VpArgs& a, double* tile, int lane, int wave, [[maybe_unused]] const typename FAM::Extra& tb,
                                        [[maybe_unused]] const float* tab)
{
    // (the body reads the family's flags by their bare names)
    [[maybe_unused]] constexpr bool BAND = FAM::BAND, PM = FAM::PM, TAB = FAM::TAB, SHP = FAM::SHP, RES = FAM::RES, UNI = FAM::UNI, BLP = FAM::BLP, EQ = FAM::EQ, SYN = FAM::SYN;
    constexpr int RG = SMALL ? kRowGroup : kRowGroup / 2;                      // rows per instruction dispatch (the full register file: four temporaries of a row group each)
    constexpr bool BUS = C > 0;
    constexpr int CC = BUS ? C : 1;
    using L = VpLimits<SMALL>;
    constexpr int NF = L::NF, NO = L::NO, NP = L::NP, NT = L::NT;
    constexpr bool EXT = L::EXT;
    using Vec = typename sig_vec::OutVec<VPT>::type;
    const int64_t item = (int64_t)blockIdx.x * 4 + wave;
    const int vt = (int)(item % a.voice_tiles);
    const int64_t b_first = (item / a.voice_tiles) * a.span;
    if (b_first >= a.K) return;                                               // wave-uniform
    const int nb = (int)((a.K - b_first < (int64_t)a.span) ? a.K - b_first : (int64_t)a.span);
    const int v0 = (vt * SIG_WAVE + lane) * VPT;
    const bool live0 = v0 < a.voices;
    const int vc = live0 ? v0 : 0;
    auto voice = [&](int i) { return (v0 + i < a.voices) ? v0 + i : vc; };     // dead voices shadow a live one (weight 0 / not stored)

    // the program: word pc in lane pc
    uint32_t codev = 0;
#pragma unroll
    for (int k = 0; k < kMaxIns; ++k) codev = (lane == k) ? a.code[k] : codev;

    double acc[RG][VPT], T[NT > 0 ? NT : 1][RG][VPT], pr[NP][VPT], ohz[NO][VPT], oph[NO][VPT];
    double z0[NF][VPT], z1[NF][VPT], w0[NF][VPT], w1[NF][VPT], na1[NF][VPT], na2[NF][VPT], fb0[NF][VPT], xa1[NF][VPT], xa2[NF][VPT];
    double s2[NF];
    // EQ: the numerator of a FilterEq slot is b0 = fb0, b1 = eb1, b2 = eb2 (not b0 [1, +-2, 1]); xb0 / xb1 / xb2: the next block's chain
    constexpr int NE = EQ ? NF : 1;
    [[maybe_unused]] double eb1[NE][VPT], eb2[NE][VPT], xb0[NE][VPT], xb1[NE][VPT], xb2[NE][VPT];
    if constexpr (EQ) {
#pragma unroll
        for (int f = 0; f < NE; ++f)
#pragma unroll
            for (int i = 0; i < VPT; ++i) eb1[f][i] = eb2[f][i] = xb0[f][i] = xb1[f][i] = xb2[f][i] = 0.0;
    }
    // band filters (Band): two consecutive slots f, f + 1 -- the sections of butter(2, [low, high]) -- whose middle taps vary per
    // voice and block: beta of the first section (current and next chains) in bq / xbq[f / 2]; the second's is -beta (bp) or beta
    // (bs); the band's gain is the second slot's fb0.  A run of band slots pairs up from its start (the host emits them that way,
    // sig_voice_program checks it)
    constexpr int NB = NF / 2 > 0 ? NF / 2 : 1;
    double bq[NB][VPT], xbq[NB][VPT];
    bool bfirst[NF];
    double wt[CC][VPT];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < VPT; ++i) bq[b][i] = xbq[b][i] = 0.0;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const bool band = f < a.n_filters && (a.ftype[f] == SIG_FILT_BANDPASS || a.ftype[f] == SIG_FILT_BANDSTOP);
        bfirst[f] = BAND && band && f + 1 < NF && !(f > 0 && bfirst[f > 0 ? f - 1 : 0]);
        s2[f] = (f < a.n_filters && (a.ftype[f] == SIG_FILT_HIGHPASS || (RES && a.ftype[f] == SIG_FILT_RES_HIGHPASS))) ? -2.0 : 2.0;
#pragma unroll
        for (int i = 0; i < VPT; ++i) { z0[f][i] = z1[f][i] = w0[f][i] = w1[f][i] = 0.0; na1[f][i] = na2[f][i] = fb0[f][i] = xa1[f][i] = xa2[f][i] = 0.0; }
    }
#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int r = 0; r < RG; ++r)
#pragma unroll
            for (int i = 0; i < VPT; ++i) T[k][r][i] = 0.0;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
#pragma unroll
        for (int r = 0; r < RG; ++r) acc[r][i] = 0.0;
#pragma unroll
        for (int ch = 0; ch < CC; ++ch) wt[ch][i] = BUS ? ((v0 + i < a.voices) ? (a.pan ? a.pan[ch * a.pan_ld + voice(i)] : 1.0) : 0.0) : 1.0;
    }

    // RES: the parameter slot that holds filter slot f's q rows (-1: a Butterworth slot, or q unplugged), from the FilterQ words
    [[maybe_unused]] int qreg[NF];
    [[maybe_unused]] int greg[NE];                                             // EQ: likewise the slot's gain rows, from the FilterEq words' b
    if constexpr (RES) {
#pragma unroll
        for (int f = 0; f < NF; ++f) qreg[f] = -1;
        if constexpr (EQ) {
#pragma unroll
            for (int f = 0; f < NE; ++f) greg[f] = -1;
        }
        for (int k = 0; k < a.n_ins; ++k) {
            const uint32_t w = a.code[k];                                      // (wave-uniform: the argument block)
            if ((w & 31u) != (uint32_t)SIG_VP_FILTERQ && !(EQ && (w & 31u) == (uint32_t)SIG_VP_FILTEREQ)) continue;
            const int slot = (int)((w >> 8) & 15u), reg = (int)((w >> 16) & 15u);
#pragma unroll
            for (int f = 0; f < NF; ++f)
                if (f == slot) qreg[f] = (reg < a.n_params) ? reg : -1;        // (15: unplugged)
            if constexpr (EQ) {
                const int gr = (int)((w >> 12) & 15u);                         // (FilterQ's b is 0: its slot is no equaliser slot, greg is not read)
#pragma unroll
                for (int f = 0; f < NE; ++f)
                    if (f == slot) greg[f] = ((w & 31u) == (uint32_t)SIG_VP_FILTEREQ && gr < a.n_params) ? gr : -1;
            }
        }
    }

    // ---- per-block state: parameter registers, oscillator rows, filter designs
    auto row_at = [&](const Rows& r, int64_t cri, int v) {
        return r.ptr[(r.rows > 1 ? cri * (int64_t)(r.cs ? a.voices : 1) : 0) + (int64_t)v * r.cs];
    };
    bool params_loaded = false;
    auto load_params = [&](int64_t cri) {
#pragma unroll
        for (int k = 0; k < NP; ++k)
            if (k < a.n_params && (!params_loaded || a.params[k].rows > 1)) {
#pragma unroll
                for (int i = 0; i < VPT; ++i) pr[k][i] = row_at(a.params[k], cri, voice(i));
            }
#pragma unroll
        for (int k = 0; k < NO; ++k)
            if (k < a.n_oscs) {
                if (!params_loaded || a.hertz[k].rows > 1) {
#pragma unroll
                    for (int i = 0; i < VPT; ++i) ohz[k][i] = row_at(a.hertz[k], cri, voice(i));
                }
                if (!params_loaded || a.phase[k].rows > 1) {
#pragma unroll
                    for (int i = 0; i < VPT; ++i) oph[k][i] = a.phase[k].ptr ? row_at(a.phase[k], cri, voice(i)) : 0.0;
                }
            }
        params_loaded = true;
    };
    bool designed = false;                                                     // block-invariant designs are made once
    auto design = [&](int64_t cri, int min_level, auto next_tag) {
        constexpr bool NEXT = decltype(next_tag)::value;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const int g = (f + 1 < NF) ? f + 1 : f;                            // the second slot of a band filter at f
            if (BAND && f < a.n_filters && a.flevel[f] >= min_level && bfirst[f] && (!designed || a.cutoff[f].rows > 1 || a.cutoff[g].rows > 1)) {
                bool ok = true;
#pragma unroll
                for (int i = 0; i < VPT; ++i) {
                    __builtin_amdgcn_sched_barrier(0);
                    Biquad q1, q2;
                    double beta = 0.0;
                    ok &= sig_biquad::design_band2<false>(a.ftype[f], row_at(a.cutoff[f], cri, voice(i)), row_at(a.cutoff[g], cri, voice(i)),
                                                          a.rate, q1, q2, &beta, nullptr, VpTan{}) || !(v0 + i < a.voices);
                    if (NEXT) { xa1[f][i] = -q1.a1; xa2[f][i] = -q1.a2; xa1[g][i] = -q2.a1; xa2[g][i] = -q2.a2; xbq[f / 2][i] = beta; }
                    else { na1[f][i] = -q1.a1; na2[f][i] = -q1.a2; fb0[f][i] = 1.0; na1[g][i] = -q2.a1; na2[g][i] = -q2.a2; fb0[g][i] = q1.b0; bq[f / 2][i] = beta; }
                    if (!NEXT && !designed) { xa1[f][i] = -q1.a1; xa2[f][i] = -q1.a2; xa1[g][i] = -q2.a1; xa2[g][i] = -q2.a2; xbq[f / 2][i] = beta; }
                }
                if (!ok && a.status) atomicOr(a.status, SIG_STATUS_BAD_CUTOFF);
            }
            if constexpr (RES) {                                               // every slot of this variant: vp_design_res, a Butterworth slot at d = sqrt2
                const bool resonant = f < a.n_filters && (a.ftype[f] == SIG_FILT_RES_LOWPASS || a.ftype[f] == SIG_FILT_RES_HIGHPASS);
                const bool plain = f < a.n_filters && (a.ftype[f] == SIG_FILT_LOWPASS || a.ftype[f] == SIG_FILT_HIGHPASS);
                const bool swept_q = resonant && qreg[f] >= 0 && a.params[qreg[f] >= 0 ? qreg[f] : 0].rows > 1;
                if ((resonant || plain) && a.flevel[f] >= min_level && (!designed || a.cutoff[f].rows > 1 || swept_q)) {
                    const bool lowpass = a.ftype[f] == SIG_FILT_LOWPASS || a.ftype[f] == SIG_FILT_RES_LOWPASS;
                    int bad = 0;
#pragma unroll
                    for (int i = 0; i < VPT; ++i) {
                        __builtin_amdgcn_sched_barrier(0);
                        double d = sig_biquad::kSqrt2;
                        bool q_ok = true;
                        if (resonant && qreg[f] >= 0) {
                            const double r = row_at(a.params[qreg[f]], cri, voice(i));
                            q_ok = r > 0.0 && r < __builtin_inf();             // 0, negative, NaN, +-inf: refused
                            d = 1.0 / r;
                        }
                        Biquad q;
                        const int got = vp_design_res(lowpass, row_at(a.cutoff[f], cri, voice(i)), d, q_ok, a.rate, q);
                        bad |= (v0 + i < a.voices) ? got : 0;                  // a dead (padding) lane never reports
                        if (NEXT) { xa1[f][i] = -q.a1; xa2[f][i] = -q.a2; }
                        else { na1[f][i] = -q.a1; na2[f][i] = -q.a2; fb0[f][i] = q.b0; }
                        if (!NEXT && !designed) { xa1[f][i] = -q.a1; xa2[f][i] = -q.a2; }
                    }
                    if (bad && a.status) atomicOr(a.status, bad);
                }
                if constexpr (EQ) {                                            // an equaliser slot: all five coefficients, q and gain from the word's rows
                    const bool eq = f < a.n_filters && a.ftype[f] >= SIG_FILT_EQ_BANDPASS && a.ftype[f] <= SIG_FILT_EQ_HIGHSHELF;
                    const bool has_q = eq && qreg[f] >= 0, has_gain = eq && greg[f] >= 0;
                    const bool swept_eq = (has_q && a.params[has_q ? qreg[f] : 0].rows > 1) || (has_gain && a.params[has_gain ? greg[f] : 0].rows > 1);
                    if (eq && a.flevel[f] >= min_level && (!designed || a.cutoff[f].rows > 1 || swept_eq)) {
                        int bad = 0;
#pragma unroll
                        for (int i = 0; i < VPT; ++i) {
                            __builtin_amdgcn_sched_barrier(0);
                            const double qv = has_q ? row_at(a.params[qreg[f]], cri, voice(i)) : 0.0;
                            const double db = has_gain ? row_at(a.params[greg[f]], cri, voice(i)) : 0.0;
                            Biquad q;
                            const int got = vp_design_eq(a.ftype[f], row_at(a.cutoff[f], cri, voice(i)), has_q, qv, has_gain, db, a.rate, q);
                            bad |= (v0 + i < a.voices) ? got : 0;              // a dead (padding) lane never reports
                            if (NEXT) { xa1[f][i] = -q.a1; xa2[f][i] = -q.a2; xb0[f][i] = q.b0; xb1[f][i] = q.b1; xb2[f][i] = q.b2; }
                            else { na1[f][i] = -q.a1; na2[f][i] = -q.a2; fb0[f][i] = q.b0; eb1[f][i] = q.b1; eb2[f][i] = q.b2; }
                            if (!NEXT && !designed) { xa1[f][i] = -q.a1; xa2[f][i] = -q.a2; xb0[f][i] = q.b0; xb1[f][i] = q.b1; xb2[f][i] = q.b2; }
                        }
                        if (bad && a.status) atomicOr(a.status, bad);
                    }
                }
            }
            const bool single = !RES && f < a.n_filters && (a.ftype[f] == SIG_FILT_LOWPASS || a.ftype[f] == SIG_FILT_HIGHPASS);
            if (single && a.flevel[f] >= min_level && (!designed || a.cutoff[f].rows > 1)) {
                bool ok = true;
#pragma unroll
                for (int i = 0; i < VPT; ++i) {
                    __builtin_amdgcn_sched_barrier(0);                         // one design at a time: four interleaved tan() set the kernel's register budget
                    Biquad q;
                    ok &= vp_design(a.ftype[f], row_at(a.cutoff[f], cri, voice(i)), a.rate, q) || !(v0 + i < a.voices);
                    if (NEXT) { xa1[f][i] = -q.a1; xa2[f][i] = -q.a2; }
                    else { na1[f][i] = -q.a1; na2[f][i] = -q.a2; fb0[f][i] = q.b0; }
                    if (!NEXT && !designed) { xa1[f][i] = -q.a1; xa2[f][i] = -q.a2; }
                }
                if (!ok && a.status) atomicOr(a.status, SIG_STATUS_BAD_CUTOFF);
            }
        }
    };
    auto start_next = [&](int64_t cri, int min_level) {                        // the next block's chains (of filters at that level of a cascade or deeper): zero state, its design
        design(cri, min_level, std::true_type{});
#pragma unroll
        for (int f = 0; f < NF; ++f)
            if (f < a.n_filters && a.flevel[f] >= min_level) {
#pragma unroll
                for (int i = 0; i < VPT; ++i) { w0[f][i] = 0.0; w1[f][i] = 0.0; }
            }
    };
    auto enter_block = [&](int64_t cri) {                                      // next becomes current
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int i = 0; i < VPT; ++i) { z0[f][i] = w0[f][i]; z1[f][i] = w1[f][i]; }
        design(cri, 0, std::false_type{});
        designed = true;
    };

    // ---- envelope (EXT): the voice's current linear stage, re-derived where a run of rows starts and where a stage ends
    [[maybe_unused]] sig_env::Segment seg[EXT ? VPT : 1];
    auto seed_envelope = [&](double t) {
        if constexpr (EXT) {
            if (a.has_adsr) {
#pragma unroll
                for (int i = 0; i < VPT; ++i) seg[i] = sig_env::segment_at(sig_env::load_voice(a.adsr, voice(i)), t);
            }
        }
    };

    float* dst = BUS ? nullptr : a.out + vc;
    double* dstp = BUS ? a.partials + (int64_t)vt * a.rows * CC : nullptr;     // [tile][row][c]
    sig_bus::PipelinedTile<CC> stage(tile, lane, dstp, b_first * a.N);

    // ---- the block sequence of this span (see the header) as a list of STEPS: [load parameters] [next -> current] [start the
    // next block's chains] then rows [from, to).  One loop, so that the row interpreter exists once in the code.
    const int D = a.depth, H = a.hist;
    const int ctx = (D > 0) ? a.ctx : 0;                                       // no filter: no context rows at all
    // `warm_from`: the row from which the NEXT block's chains run too (their zero state and design are set up when the walk gets
    // there); == to: none in this step
    struct Step { bool load, enter, out, next0; int next_level; int64_t cri_load, cri_enter, cri_next, from, to, warm_from; };   // next0: the next chains start with the step, even an empty one
    auto bpos = [&](int64_t j) -> int64_t { return j >= 0 ? a.position + j * (int64_t)a.N : a.hist_pos[H + j]; };   // j >= -H
    auto cri = [&](int64_t j) -> int64_t { return j + H + 1; };                // control rows: [one in front | H blocks in front | K blocks]
    int64_t j0 = b_first - (D > 1 ? D - 1 : 0);
    if (j0 < -(int64_t)H) j0 = -(int64_t)H;
    const int64_t j_end = b_first + nb;
    int n_steps;
    if (!a.small) n_steps = 1 + (int)(j_end - j0);
    else n_steps = (D >= 2) ? 4 : 2;
    auto make_step = [&](int t) {
        Step st{false, false, false, false, 0, 0, 0, 0, 0, 0, 0};
        if (!a.small) {
            if (t == 0) {                                                      // the rows in front of the first block belong to the block before it
                const int64_t s0 = bpos(j0);
                const int64_t c0 = (s0 < (int64_t)ctx) ? s0 : (int64_t)ctx;
                st.load = true; st.cri_load = cri(j0) - 1;
                st.cri_next = cri(j0); st.next0 = true;
                st.from = s0 - c0; st.to = s0; st.warm_from = st.from;
                return st;
            }
            const int64_t j = j0 + (t - 1);
            const int64_t s0 = bpos(j), e = bpos(j + 1);
            int64_t cn = (j + 1 < j_end) ? ((e < (int64_t)ctx) ? e : (int64_t)ctx) : 0;     // the next block's context, inside this one
            if (cn > e - s0) cn = e - s0;
            st.out = j >= b_first;
            st.enter = true; st.cri_enter = cri(j);
            st.load = true; st.cri_load = cri(j);
            st.cri_next = cri(j + 1);
            st.from = s0; st.to = e; st.warm_from = e - cn;
            return st;
        }
        // Blocks shorter than the context: every block behind its own virtual block [vp, p), vp = max(p - ctx, 0), whose
        // controls are row b of the per-block arrays; the block's own are row K + b.  What feeds the LAST filter over the
        // block's own rows is the oldest cached block of that input containing them: the input's reply to the `after`
        // request made m = min((ctx - N) / N, blocks rendered before) blocks earlier, at q = p - m N (chain/__init__.py:
        // 435-442: the first containing block in insertion order) -- a filter in it was cold-started min(ctx, q) rows before q,
        // and everything in it read its controls at q (the caller evaluates those rows of the K + b group there).
        const int64_t p = a.position + b_first * (int64_t)a.N;
        const int64_t vp = (p > (int64_t)ctx) ? p - ctx : 0;
        if (D < 2) {
            if (t == 0) {                                                      // the virtual block: the whole of it is the block's context
                st.load = true; st.cri_load = b_first;
                st.cri_next = a.K + b_first; st.next0 = true;
                st.from = vp; st.to = p; st.warm_from = vp;
            } else {
                st.enter = true; st.cri_enter = a.K + b_first;
                st.load = true; st.cri_load = a.K + b_first;
                st.from = p; st.to = p + a.N; st.warm_from = st.to; st.out = true;
            }
            return st;
        }
        const int64_t bg = (int64_t)a.blocks_before + b_first;                // blocks of this size rendered since the graph was fresh
        int64_t m = (a.N > 0) ? (ctx - a.N) / a.N : 0;
        if (m > bg - 1) m = bg - 1;
        if (m < 0) m = 0;
        const int64_t q = p - m * a.N;
        const int64_t qc = q - ((q < (int64_t)ctx) ? q : (int64_t)ctx);        // where the inner filter of the block's own rows cold-starts
        const int64_t c0 = (vp < (int64_t)ctx) ? vp : (int64_t)ctx;
        const int64_t r0 = vp - c0;                                            // ... and where the virtual block's inner filter does
        const int64_t r1 = (qc < r0) ? r0 : ((qc > vp) ? vp : qc);
        if (t == 0) {                                                          // the virtual block's inner filter alone (current chains from zero)
            st.enter = true; st.cri_enter = b_first;
            st.load = true; st.cri_load = b_first;
            st.from = r0; st.to = r1; st.warm_from = r1;
        } else if (t == 1) {                                                   // + the inner filter of the block's own rows warms up
            st.next_level = 1; st.cri_next = a.K + b_first; st.next0 = true;
            st.from = r1; st.to = vp; st.warm_from = r1;
        } else if (t == 2) {                                                   // the virtual block: the outer filter cold-starts on it
            st.next_level = 2; st.cri_next = a.K + b_first; st.next0 = true;
            st.from = vp; st.to = p; st.warm_from = vp;
        } else {
            st.enter = true; st.cri_enter = a.K + b_first;
            st.load = true; st.cri_load = a.K + b_first;
            st.from = p; st.to = p + a.N; st.warm_from = st.to; st.out = true;
        }
        return st;
    };

    // rows [from, to): every instruction of the program for a group of R consecutive rows at a time (R = RG, then single rows
    // for what is left of the segment); WARM rows also advance the next block's chains
    double q_lane = 0.0;
    int64_t qbase = 0;
    bool q_valid = false;
    sig_bus::FoldedGroup<CC> folded(tile, lane, dstp);                         // whole groups of the bus sink: sums folded across lanes in registers
    // one biquad section of filter slot F over the group's R rows, in place on the accumulator: DF2T of [1, beta, 1] / [1, a1, a2]
    // (b0-normalised; `scale`: times the slot's b0 after).  beta(i) / xbeta(i): the current and next chains' middle taps
    auto section = [&](auto I, int warm_r, auto rows_tag, auto beta, auto xbeta, bool scale) {
        constexpr int F = decltype(I)::value;
        constexpr int R = decltype(rows_tag)::value;
        if (warm_r < R) {                                                      // wave-uniform: the next block's chain, on the same input rows
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r >= warm_r) {                                             // (wave-uniform too: a group may straddle the first warm row)
#pragma unroll
                    for (int i = 0; i < VPT; ++i) {
                        const double x = acc[r][i];
                        const double yw = x + w0[F][i];
                        w0[F][i] = fma(xa1[F][i], yw, fma(xbeta(i), x, w1[F][i]));
                        w1[F][i] = fma(xa2[F][i], yw, x);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double x = acc[r][i];
                const double y = x + z0[F][i];
                z0[F][i] = fma(na1[F][i], y, fma(beta(i), x, z1[F][i]));
                z1[F][i] = fma(na2[F][i], y, x);
                acc[r][i] = scale ? fb0[F][i] * y : y;
            }
        }
    };
    // EQ: the section of an equaliser slot F, the general transposed direct form II y = b0 x + z0; z0 = b1 x - a1 y + z1; z1 = b2 x - a2 y
    // (the state is not b0-normalised: b0 may be 0, an all-pass at d k = 1 + k k)
    [[maybe_unused]] auto section_eq = [&](auto I, int warm_r, auto rows_tag) {
        constexpr int F = decltype(I)::value;
        constexpr int R = decltype(rows_tag)::value;
        if constexpr (EQ) {
            if (warm_r < R) {                                                  // wave-uniform: the next block's chain, on the same input rows
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (r >= warm_r) {
#pragma unroll
                        for (int i = 0; i < VPT; ++i) {
                            const double x = acc[r][i];
                            const double yw = fma(xb0[F][i], x, w0[F][i]);
                            w0[F][i] = fma(xa1[F][i], yw, fma(xb1[F][i], x, w1[F][i]));
                            w1[F][i] = fma(xa2[F][i], yw, xb2[F][i] * x);
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double x = acc[r][i];
                    const double y = fma(fb0[F][i], x, z0[F][i]);
                    z0[F][i] = fma(na1[F][i], y, fma(eb1[F][i], x, z1[F][i]));
                    z1[F][i] = fma(na2[F][i], y, eb2[F][i] * x);
                    acc[r][i] = y;
                }
            }
        }
    };
    auto group = [&](int64_t n, int warm_r, bool out, auto rows_tag) {        // warm_r: the first row of the group that also advances the next chains (R: none)
        constexpr int R = decltype(rows_tag)::value;
        if (!q_valid || n < qbase || n + R > qbase + SIG_WAVE) {                // n / rate (IEEE divide) for 64 rows at a time, one per lane
            qbase = n;
            q_lane = (double)(qbase + lane) / a.rate;
            q_valid = true;
        }
        double q[R];
#pragma unroll
        for (int r = 0; r < R; ++r) q[r] = sig_readlane_f64(q_lane, (int)(n - qbase) + r);     // osc.py:32
#ifdef SIG_VP_STATIC_CODE
        // a specialised build: the program is a compile-time constant, the loop is unrolled and every switch below folds away
        constexpr uint32_t kStatic[] = SIG_VP_STATIC_CODE;
        constexpr bool kStaticExt = [] {
            constexpr uint32_t c[] = SIG_VP_STATIC_CODE;
            bool ext = false;
            for (unsigned k = 0; k < sizeof(c) / sizeof(c[0]); ++k) {
                const uint32_t op = c[k] & 31u;
                ext |= op == (uint32_t)SIG_VP_AMP || op == (uint32_t)SIG_VP_ADSR || op == (uint32_t)SIG_VP_NOISE;
            }
            return ext;
        }();
        static_assert(EXT || !kStaticExt, "the program uses Amp / ADSR / White: build with -DSIG_VP_S_EXT=1");
#pragma unroll
        for (int pc = 0; pc < (int)(sizeof(kStatic) / sizeof(kStatic[0])); ++pc) {
            const uint32_t w = kStatic[pc];
#else
        for (int pc = 0; pc < a.n_ins; ++pc) {
            const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)codev, pc);
#endif
            const int op = (int)(w & 31u), kind = (int)((w >> 5) & 7u), ia = (int)((w >> 8) & 15u), ib = (int)((w >> 12) & 15u),
                      ic = (int)((w >> 16) & 15u);
            // OscTable is dispatched in front of the switch, and only in the TAB variant: a case of its own, even an empty one, changes
            // the code of every other instantiation (the compare chain of the dispatch), and those are to stay what they were
            if constexpr (RES) {                                               // FilterQ: the Filter handler on a resonant slot, in front of the switch like OscTable
                if (op == SIG_VP_FILTERQ) {
                    with_index<NF>(ia, [&](auto I) {
                        constexpr int F = decltype(I)::value;
                        section(I, warm_r, rows_tag, [&](int) { return s2[F]; }, [&](int) { return s2[F]; }, true);
                    });
                    continue;
                }
            }
            if constexpr (EQ) {                                                // FilterEq: an equaliser slot's section, in front of the switch likewise
                if (op == SIG_VP_FILTEREQ) {
                    with_index<NF>(ia, [&](auto I) { section_eq(I, warm_r, rows_tag); });
                    continue;
                }
            }
            if constexpr (UNI) {                                               // OscUni: in front of the switch like OscTable
                if (op == SIG_VP_OSCUNI) {
                    // sig_osc_bank_unison's expression with the fused waveforms: r = 1 + spread d, h = hertz r, q = phase + p per copy
                    // (block-invariant, but 2 x copies x VPT registers: recomputed per group), t = n / rate * h + q, the sum in u
                    // ascending, divided by the count.  The copy loop's trip count is wave-uniform (the argument block)
                    double sp[VPT];
#pragma unroll
                    for (int i = 0; i < VPT; ++i) sp[i] = 0.0;                 // (15: spread unplugged)
                    if (ic < NP) {
                        with_index<NP>(ic, [&](auto I) {
#pragma unroll
                            for (int i = 0; i < VPT; ++i) sp[i] = pr[decltype(I)::value][i];
                        });
                    }
                    const int copies = tb.copies;
                    with_index<NO>(ia, [&](auto I) {
                        constexpr int S = decltype(I)::value;
                        for (int u = 0; u < copies; ++u) {
                            const double d = tb.detune[u], p = tb.offset[u];
                            double h[VPT], qu[VPT];
#pragma unroll
                            for (int i = 0; i < VPT; ++i) {
                                h[i] = ohz[S][i] * (1.0 + sp[i] * d);
                                qu[i] = oph[S][i] + p;
                            }
                            auto add = [&](auto wave) {
#pragma unroll
                                for (int r = 0; r < R; ++r) {
                                    const double qr = vp_pin(q[r]);
#pragma unroll
                                    for (int i = 0; i < VPT; ++i) {
                                        const double w = wave(qr * h[i] + qu[i]);
                                        acc[r][i] = (u == 0) ? w : acc[r][i] + w;
                                    }
                                }
                            };
                            switch (kind) {
                                case SIG_OSC_SINE: add([](double t) { return sig_osc::osc_wave_fused<SIG_OSC_SINE>(t); }); break;
                                case SIG_OSC_SAWTOOTH: add([](double t) { return sig_osc::osc_wave_fused<SIG_OSC_SAWTOOTH>(t); }); break;
                                case SIG_OSC_SQUARE: add([](double t) { return sig_osc::osc_wave_fused<SIG_OSC_SQUARE>(t); }); break;
                                default: add([](double t) { return sig_osc::osc_wave_fused<SIG_OSC_TRIANGLE>(t); }); break;
                            }
                        }
                        const double count = (double)copies;
#pragma unroll
                        for (int r = 0; r < R; ++r)
#pragma unroll
                            for (int i = 0; i < VPT; ++i) acc[r][i] = acc[r][i] / count;
                    });
                    continue;
                }
            }
            if constexpr (BLP) {                                               // OscBlep: OscUni's operands and copies, sig_osc_bank_blep's waveforms
                if (op == SIG_VP_OSCBLEP) {
                    // the OscUni handler with sig_osc::osc_blep (m by v_fract_f64, like the fused waveforms) per copy.  d = min(|h| / rate,
                    // 0.5) and 1 / d are block-invariant too, and 4 x copies x VPT registers with h and q: recomputed per group, two
                    // divides per copy and voice for the group's R rows; the rows multiply
                    double sp[VPT];
#pragma unroll
                    for (int i = 0; i < VPT; ++i) sp[i] = 0.0;                 // (15: spread unplugged)
                    if (ic < NP) {
                        with_index<NP>(ic, [&](auto I) {
#pragma unroll
                            for (int i = 0; i < VPT; ++i) sp[i] = pr[decltype(I)::value][i];
                        });
                    }
                    const int copies = tb.copies;
                    with_index<NO>(ia, [&](auto I) {
                        constexpr int S = decltype(I)::value;
                        for (int u = 0; u < copies; ++u) {
                            const double du = tb.detune[u], pu = tb.offset[u];
                            double h[VPT], qu[VPT], d[VPT], inv_d[VPT];
#pragma unroll
                            for (int i = 0; i < VPT; ++i) {
                                h[i] = ohz[S][i] * (1.0 + sp[i] * du);
                                qu[i] = oph[S][i] + pu;
                                sig_osc::blep_increment(h[i], a.rate, d[i], inv_d[i]);
                            }
                            auto add = [&](auto wave) {
#pragma unroll
                                for (int r = 0; r < R; ++r) {
                                    const double qr = vp_pin(q[r]);
#pragma unroll
                                    for (int i = 0; i < VPT; ++i) {
                                        const double w = wave(qr * h[i] + qu[i], d[i], inv_d[i]);
                                        acc[r][i] = (u == 0) ? w : acc[r][i] + w;
                                    }
                                }
                            };
                            switch (kind) {                                    // (Sine is refused by the entry)
                                case SIG_OSC_SAWTOOTH: add([](double t, double d, double v) { return sig_osc::osc_blep<SIG_OSC_SAWTOOTH, true>(t, d, v); }); break;
                                case SIG_OSC_SQUARE: add([](double t, double d, double v) { return sig_osc::osc_blep<SIG_OSC_SQUARE, true>(t, d, v); }); break;
                                default: add([](double t, double d, double v) { return sig_osc::osc_blep<SIG_OSC_TRIANGLE, true>(t, d, v); }); break;
                            }
                        }
                        const double count = (double)copies;
#pragma unroll
                        for (int r = 0; r < R; ++r)
#pragma unroll
                            for (int i = 0; i < VPT; ++i) acc[r][i] = acc[r][i] / count;
                    });
                    continue;
                }
            }
            if constexpr (SYN) {                                               // OscSync: OscBlep's operands and copies, the ratio in params[b], sig_osc_bank_sync's waveforms
                if (op == SIG_VP_OSCSYNC) {
                    // the OscBlep handler with sig_osc::osc_sync (m by v_fract_f64).  R, g and the reset's weight per voice, ds and
                    // 1 / ds per copy and voice are block-invariant like d and 1 / d: recomputed per group, three divides per copy and
                    // voice for the group's R rows; the rows multiply
                    double sp[VPT], ratio[VPT];
#pragma unroll
                    for (int i = 0; i < VPT; ++i) { sp[i] = 0.0; ratio[i] = 0.0; }     // (15: spread / ratio unplugged)
                    if (ic < NP) {
                        with_index<NP>(ic, [&](auto I) {
#pragma unroll
                            for (int i = 0; i < VPT; ++i) sp[i] = pr[decltype(I)::value][i];
                        });
                    }
                    if (ib < NP) {
                        with_index<NP>(ib, [&](auto I) {
#pragma unroll
                            for (int i = 0; i < VPT; ++i) ratio[i] = pr[decltype(I)::value][i];
                        });
                    }
                    const int copies = tb.copies;
                    auto run = [&](auto kind_tag) {
                        constexpr int KIND = decltype(kind_tag)::value;
                        sig_osc::SyncRatio ra[VPT];
#pragma unroll
                        for (int i = 0; i < VPT; ++i) ra[i] = sig_osc::sync_ratio<KIND>(ratio[i]);
                        with_index<NO>(ia, [&](auto I) {
                            constexpr int S = decltype(I)::value;
                            for (int u = 0; u < copies; ++u) {
                                const double du = tb.detune[u], pu = tb.offset[u];
                                double h[VPT], qu[VPT], d[VPT], inv_d[VPT], ds[VPT], inv_ds[VPT];
#pragma unroll
                                for (int i = 0; i < VPT; ++i) {
                                    h[i] = ohz[S][i] * (1.0 + sp[i] * du);
                                    qu[i] = oph[S][i] + pu;
                                    sig_osc::blep_increment(h[i], a.rate, d[i], inv_d[i]);
                                    sig_osc::sync_increment(d[i], ra[i].R, ds[i], inv_ds[i]);
                                }
#pragma unroll
                                for (int r = 0; r < R; ++r) {
                                    const double qr = vp_pin(q[r]);
#pragma unroll
                                    for (int i = 0; i < VPT; ++i) {
                                        const double w = sig_osc::osc_sync<KIND, true>(qr * h[i] + qu[i], d[i], inv_d[i], ra[i], ds[i], inv_ds[i]);
                                        acc[r][i] = (u == 0) ? w : acc[r][i] + w;
                                    }
                                }
                            }
                            const double count = (double)copies;
#pragma unroll
                            for (int r = 0; r < R; ++r)
#pragma unroll
                                for (int i = 0; i < VPT; ++i) acc[r][i] = acc[r][i] / count;
                        });
                    };
                    if (kind == SIG_OSC_SAWTOOTH) run(std::integral_constant<int, SIG_OSC_SAWTOOTH>{});    // (Sine and Triangle are refused by the entry)
                    else run(std::integral_constant<int, SIG_OSC_SQUARE>{});
                    continue;
                }
            }
            if constexpr (TAB) {
                // the column of table slot ib that parameter slot ic selects, per voice: its first float in `tab`
                auto columns = [&](int (&col)[VPT], int& TT) {
                    const int slot = ib & (SIG_VP_MAX_TABLES - 1);
                    TT = tb.T[slot];
                    const int W = tb.W[slot], S = TT + 1;
                    const int first = slot ? (tb.T[0] + 1) * tb.W[0] : 0;
#pragma unroll
                    for (int i = 0; i < VPT; ++i) col[i] = first;
                    if (ic < NP) {                                             // (15: select unplugged, column 0)
                        with_index<NP>(ic, [&](auto I) {
#pragma unroll
                            for (int i = 0; i < VPT; ++i) col[i] = first + sig_table::column(pr[decltype(I)::value][i], W) * S;
                        });
                    }
                };
                if constexpr (SHP) {
                    if (op == SIG_VP_SHAPE) {                                  // the accumulator through a transfer curve (ext.py Shaper, shaper.hip)
                        int col[VPT], TT;
                        columns(col, TT);
                        const double half = (double)(TT - 1) * 0.5;
                        const int last = TT - 2;
#pragma unroll
                        for (int r = 0; r < R; ++r) {
#pragma unroll
                            for (int i = 0; i < VPT; ++i) {
                                const double x = acc[r][i];
                                const double c = (x < -1.0) ? -1.0 : ((x > 1.0) ? 1.0 : x);     // np.clip: NaN stays NaN
                                const double u = (c + 1.0) * half;
                                const int k = (u >= 0.0) ? min((int)floor(u), last) : 0;         // (NaN: entry 0, u - k carries it)
                                const int at = col[i] + k;                     // at + 1 <= the column's entry T - 1
                                const double lo = (double)tab[at], hi = (double)tab[at + 1];
                                acc[r][i] = lo + (u - (double)k) * (hi - lo);
                            }
                        }
                        continue;
                    }
                }
                if (op == SIG_VP_OSCTABLE) {                                   // the Osc handler's phase, looked up in table slot ib (ext.py Wavetable)
                    // m = t - floor(t) as v_fract_f64: not the definition's 1.0 for t in (-2^-54, 0) but the largest double below
                    // it, i.e. the last segment at f = 1 - T 2^-53 instead of entry 0 at f = 0 -- one rounding of a table step apart
                    int col[VPT], TT;
                    columns(col, TT);
                    const double scale = (double)TT;
                    const int mask = TT - 1;
                    with_index<NO>(ia, [&](auto I) {
                        constexpr int S_ = decltype(I)::value;
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const double qr = vp_pin(q[r]);
#pragma unroll
                            for (int i = 0; i < VPT; ++i) {
                                const double u = __builtin_amdgcn_fract(qr * ohz[S_][i] + oph[S_][i]) * scale;
                                const double fl = floor(u);
                                const int at = col[i] + ((int)fl & mask);
                                const double lo = (double)tab[at], hi = (double)tab[at + 1];
                                acc[r][i] = lo + (u - fl) * (hi - lo);
                            }
                        }
                    });
                    continue;
                }
            }
            switch (op) {
                case SIG_VP_OSC:
                    with_index<NO>(ia, [&](auto I) {
                        constexpr int S = decltype(I)::value;
                        double t[R][VPT];
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const double qr = vp_pin(q[r]);
#pragma unroll
                            for (int i = 0; i < VPT; ++i) t[r][i] = qr * ohz[S][i] + oph[S][i];
                        }
                        switch (kind) {
                            case SIG_OSC_SINE:
#pragma unroll
                                for (int r = 0; r < R; ++r)
#pragma unroll
                                    for (int i = 0; i < VPT; ++i) acc[r][i] = (double)sig_osc::osc_sine_f32(t[r][i]);
                                break;
                            case SIG_OSC_SAWTOOTH:
#pragma unroll
                                for (int r = 0; r < R; ++r)
#pragma unroll
                                    for (int i = 0; i < VPT; ++i) acc[r][i] = sig_osc::osc_sawtooth_fract(t[r][i]);
                                break;
                            case SIG_OSC_SQUARE:
#pragma unroll
                                for (int r = 0; r < R; ++r)
#pragma unroll
                                    for (int i = 0; i < VPT; ++i) acc[r][i] = sig_osc::osc_square_fract(t[r][i]);
                                break;
                            default:
#pragma unroll
                                for (int r = 0; r < R; ++r)
#pragma unroll
                                    for (int i = 0; i < VPT; ++i) acc[r][i] = sig_osc::osc_triangle_fract(t[r][i]);
                                break;
                        }
                    });
                    break;
                case SIG_VP_OSCPM: if constexpr (PM) {                         // the Osc handler, its phase offset by index * accumulator (ext.py PMOsc)
                    double ix[VPT];
                    with_index<NP>(ib, [&](auto I) {
#pragma unroll
                        for (int i = 0; i < VPT; ++i) ix[i] = pr[decltype(I)::value][i];
                    });
                    with_index<NO>(ia, [&](auto I) {
                        constexpr int S = decltype(I)::value;
                        double t[R][VPT];
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const double qr = vp_pin(q[r]);
#pragma unroll
                            for (int i = 0; i < VPT; ++i) t[r][i] = (qr * ohz[S][i] + oph[S][i]) + ix[i] * acc[r][i];
                        }
                        switch (kind) {
                            case SIG_OSC_SINE:
#pragma unroll
                                for (int r = 0; r < R; ++r)
#pragma unroll
                                    for (int i = 0; i < VPT; ++i) acc[r][i] = (double)sig_osc::osc_sine_f32(t[r][i]);
                                break;
                            case SIG_OSC_SAWTOOTH:
#pragma unroll
                                for (int r = 0; r < R; ++r)
#pragma unroll
                                    for (int i = 0; i < VPT; ++i) acc[r][i] = sig_osc::osc_sawtooth_fract(t[r][i]);
                                break;
                            case SIG_OSC_SQUARE:
#pragma unroll
                                for (int r = 0; r < R; ++r)
#pragma unroll
                                    for (int i = 0; i < VPT; ++i) acc[r][i] = sig_osc::osc_square_fract(t[r][i]);
                                break;
                            default:
#pragma unroll
                                for (int r = 0; r < R; ++r)
#pragma unroll
                                    for (int i = 0; i < VPT; ++i) acc[r][i] = sig_osc::osc_triangle_fract(t[r][i]);
                                break;
                        }
                    });
                }
                    break;
                case SIG_VP_FILTER:
                    with_index<NF>(ia, [&](auto I) {
                        constexpr int F = decltype(I)::value;
                        section(I, warm_r, rows_tag, [&](int) { return s2[F]; }, [&](int) { return s2[F]; }, true);
                    });
                    break;
                case SIG_VP_BAND:                                              // two sections in series, the band's gain on the second's output
                    with_index<NF>(ia, [&](auto I) {
                        constexpr int F = decltype(I)::value;
                        if constexpr (BAND && F + 1 < NF) {
                            constexpr int G = F + 1;
                            const double sg = (a.ftype[F] == SIG_FILT_BANDPASS) ? -1.0 : 1.0;     // the second section's beta
                            if (warm_r < R) {                                  // the next block's band: BOTH next chains in series on the input
#pragma unroll
                                for (int r = 0; r < R; ++r) {
                                    if (r >= warm_r) {
#pragma unroll
                                        for (int i = 0; i < VPT; ++i) {
                                            const double x = acc[r][i];
                                            const double y1 = x + w0[F][i];
                                            w0[F][i] = fma(xa1[F][i], y1, fma(xbq[F / 2][i], x, w1[F][i]));
                                            w1[F][i] = fma(xa2[F][i], y1, x);
                                            const double y2 = y1 + w0[G][i];
                                            w0[G][i] = fma(xa1[G][i], y2, fma(sg * xbq[F / 2][i], y1, w1[G][i]));
                                            w1[G][i] = fma(xa2[G][i], y2, y1);
                                        }
                                    }
                                }
                            }
                            section(I, R, rows_tag, [&](int i) { return bq[F / 2][i]; }, [&](int i) { return bq[F / 2][i]; }, false);
                            section(std::integral_constant<int, G>{}, R, rows_tag, [&](int i) { return sg * bq[F / 2][i]; },
                                    [&](int i) { return sg * bq[F / 2][i]; }, true);
                        }
                    });
                    break;
                case SIG_VP_GAIN:
                    with_index<NP>(ia, [&](auto I) {
#pragma unroll
                        for (int r = 0; r < R; ++r)
#pragma unroll
                            for (int i = 0; i < VPT; ++i) acc[r][i] = acc[r][i] * pr[decltype(I)::value][i];      // fx.py:52
                    });
                    break;
                case SIG_VP_MUL:
                    with_index<NT>(ia, [&](auto I) {
#pragma unroll
                        for (int r = 0; r < R; ++r)
#pragma unroll
                            for (int i = 0; i < VPT; ++i) acc[r][i] = T[decltype(I)::value][r][i] * acc[r][i];     // fx.py:46
                    });
                    break;
                case SIG_VP_SAVE:
                    with_index<NT>(ia, [&](auto I) {
#pragma unroll
                        for (int r = 0; r < R; ++r)
#pragma unroll
                            for (int i = 0; i < VPT; ++i) T[decltype(I)::value][r][i] = acc[r][i];
                    });
                    break;
                case SIG_VP_LOAD:
                    with_index<NT>(ia, [&](auto I) {
#pragma unroll
                        for (int r = 0; r < R; ++r)
#pragma unroll
                            for (int i = 0; i < VPT; ++i) acc[r][i] = T[decltype(I)::value][r][i];
                    });
                    break;
                case SIG_VP_MIX: {                                             // m * L + (1 - m) * R (fx.py:40); ic: the accumulator is L
                    double m[VPT];
                    with_index<NP>(ib, [&](auto I) {
#pragma unroll
                        for (int i = 0; i < VPT; ++i) m[i] = pr[decltype(I)::value][i];
                    });
                    with_index<NT>(ia, [&](auto I) {
#pragma unroll
                        for (int r = 0; r < R; ++r)
#pragma unroll
                            for (int i = 0; i < VPT; ++i) {
                                const double l = ic ? acc[r][i] : T[decltype(I)::value][r][i], rr = ic ? T[decltype(I)::value][r][i] : acc[r][i];
                                acc[r][i] = m[i] * l + (1.0 - m[i]) * rr;
                            }
                    });
                    break;
                }
                case SIG_VP_CONST:
                    with_index<NP>(ia, [&](auto I) {
#pragma unroll
                        for (int r = 0; r < R; ++r)
#pragma unroll
                            for (int i = 0; i < VPT; ++i) acc[r][i] = pr[decltype(I)::value][i];
                    });
                    break;
                default:
                    if constexpr (EXT) {
                        if (op == SIG_VP_AMP) {
                            with_index<NP>(ia, [&](auto I) {
#pragma unroll
                                for (int r = 0; r < R; ++r)
#pragma unroll
                                    for (int i = 0; i < VPT; ++i) acc[r][i] = vp_amp(acc[r][i], pr[decltype(I)::value][i]);
                            });
                        } else if (op == SIG_VP_ADSR) {
#pragma unroll
                            for (int r = 0; r < R; ++r) {
                                const double qr = vp_pin(q[r]);
                                bool stale = false;
#pragma unroll
                                for (int i = 0; i < VPT; ++i) stale |= !(qr < seg[i].end);
                                if (__any(stale)) seed_envelope(qr);           // a stage ended: a handful of times per voice and stream
#pragma unroll
                                for (int i = 0; i < VPT; ++i) acc[r][i] = fma(seg[i].slope, qr - seg[i].t0, seg[i].l0);
                            }
                        } else if (op == SIG_VP_NOISE) {
#pragma unroll
                            for (int r = 0; r < R; ++r)
#pragma unroll
                                for (int i = 0; i < VPT; ++i) acc[r][i] = (double)sig_noise::noise_value(a.seeds[ia & 1], n + r, v0 + i);
                        }
                    }
                    break;
            }
        }
        if (out) {
            if constexpr (BUS && (R * CC == 16 || R * CC == 8)) {
                // a whole group of the bus: its R x C sums stay in registers, are folded across lanes four at a time (two
                // register-to-register halving steps, sig_bus::FoldedGroup) and only a quarter goes through the LDS
                if (stage.staged) stage.now();                                 // single rows staged before: out first, in order
                double sums[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) sums[k] = 0.0;
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int ch = 0; ch < CC; ++ch) {
                        double sum = 0.0;
#pragma unroll
                        for (int i = 0; i < VPT; ++i) sum = fma(wt[ch][i], acc[r][i], sum);
                        sums[r * CC + ch] = sum;
                    }
#pragma unroll
                for (int g4 = 0; g4 < (R * CC) / 4; ++g4) folded.fold4(g4, sums[4 * g4], sums[4 * g4 + 1], sums[4 * g4 + 2], sums[4 * g4 + 3]);
                double pend[4];
                folded.issue(pend);
                folded.finish(pend, stage.first, R);
                stage.first += R;
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if constexpr (BUS) {
#pragma unroll
                        for (int ch = 0; ch < CC; ++ch) {
                            double sum = 0.0;
#pragma unroll
                            for (int i = 0; i < VPT; ++i) sum = fma(wt[ch][i], acc[r][i], sum);
                            stage.slot[ch * kTileStride] = sum;
                        }
                        stage.advance();
                    } else {
                        float y32[VPT];
#pragma unroll
                        for (int i = 0; i < VPT; ++i) y32[i] = (float)acc[r][i];
                        if (live0) {
                            Vec o; sig_vec::put(o, y32);
                            *reinterpret_cast<Vec*>(dst + (n + r - a.position) * a.out_ld) = o;
                        }
                    }
                }
            }
        }
    };
    for (int t = 0; t < n_steps; ++t) {
        const Step st = make_step(t);
        if (st.load) load_params(st.cri_load);
        if (st.enter) enter_block(st.cri_enter);
        bool started = false;                                                  // the next chains of this step
        if (st.next0) { start_next(st.cri_next, st.next_level); started = true; }
        if (st.from >= st.to) continue;
        seed_envelope((double)st.from / a.rate);
        int64_t n = st.from;
        auto warm_rows = [&](int64_t at, int rows) {                           // first warm row of the group at `at` (rows: none), chains started on arrival
            if (st.warm_from >= at + rows) return rows;
            if (!started) { start_next(st.cri_next, st.next_level); started = true; }
            return (st.warm_from <= at) ? 0 : (int)(st.warm_from - at);
        };
        if constexpr (RG > 1) {
            for (; n + RG <= st.to; n += RG) group(n, warm_rows(n, RG), st.out, std::integral_constant<int, RG>{});
        }
        for (; n < st.to; ++n) group(n, warm_rows(n, 1), st.out, std::integral_constant<int, 1>{});
    }
    if (BUS && stage.staged) stage.now();
}

#ifndef SIG_VP_WAVES
#define SIG_VP_WAVES 2
#endif
#ifndef SIG_VP_WAVES1
#define SIG_VP_WAVES1 3
#endif
template <int VPT, bool SMALL, int C, typename FAM>
__device__ __forceinline__ void vp_kernel_body(const VpArgs& a, const typename FAM::Extra& tb)
{
    constexpr bool BUS = C > 0;
    __shared__ double lds[BUS ? 4 : 1][BUS ? sig_bus::kPairs * kTileStride : 1];
    const float* tab = nullptr;
    if constexpr (FAM::TAB) {                                                    // the tables into (dynamic) LDS, once per workgroup
        extern __shared__ float vp_tab[];
        int first = 0;
#pragma unroll
        for (int k = 0; k < SIG_VP_MAX_TABLES; ++k) {
            if (!tb.ptr[k]) break;                                             // (slots are filled from 0)
            sig_table::stage<256>(vp_tab + first, tb.ptr[k], tb.T[k], tb.W[k]);
            first += (tb.T[k] + 1) * tb.W[k];
        }
        __syncthreads();
        tab = vp_tab;
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    vp_wave<VPT, SMALL, C, FAM>(a, lds[BUS ? wave : 0], lane, wave, tb, tab);
    if constexpr (BUS) {
        if (a.bus_out) sig_bus::sum_tiles_in_workgroup<C>(a.partials, a.voice_tiles, a.rows, a.span, a.K, a.N, a.bus_out, a.bus_out_ld, lane, wave);
    }
}

// The interpreter's kernel: VPT voices per lane (1, 2), the SMALL or the full register file, sink C, family FAM.  A pair, because a
// family without a second parameter keeps the argument block it always had (an empty struct by value would still be an argument).
#define SIG_VP_KERNEL __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SMALL ? (VPT == 1 ? SIG_VP_WAVES1 : SIG_VP_WAVES) : 1, 8)))
template <int VPT, bool SMALL, int C, typename FAM>
SIG_VP_KERNEL void voice_program_kernel(VpArgs a)
{
    vp_kernel_body<VPT, SMALL, C, FAM>(a, VpNoTables{});
}
template <int VPT, bool SMALL, int C, typename FAM>
SIG_VP_KERNEL void voice_program_kernel(VpArgs a, typename FAM::Extra extra)
{
    vp_kernel_body<VPT, SMALL, C, FAM>(a, extra);
}
#undef SIG_VP_KERNEL

}  // namespace
