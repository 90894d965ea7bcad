// The block-rate control machine of control_program.hip, stated once for its two builds (the interpreter and the build
// specialised for one program's structure): where a workgroup's block lies, what an instruction is worth there, a ROW's
// load, a filter's design, an output's store, the ADSRARGS / ADSR pair rule.  What the builds do NOT share stays in
// control_program.hip: where the registers live (`get`), the loops over the instructions, the threads per workgroup.
// Arithmetic as in the per-node kernels (osc_bank.hip's f64 store path, elementwise.hip's ew_apply): the same expressions
// under -ffp-contract=off, so the same bits.
#pragma once
#include "sig_adsr.h"
#include "sig_biquad.h"
#include "sig_noise.h"
#include "sig_osc.h"

#define SIG_CTL_CONTEXT 100                 // a filter's `before` window: min(100, p) rows (fx.py:105, CritFilter.context_frames)

namespace sig_ctl {

constexpr int kThreads = 128;               // the interpreter's workgroup
constexpr int kSpecThreads = 256;           // the specialised kernel's: its launch bounds and the host's hipModuleLaunchKernel
static_assert(kThreads > SIG_CTL_CONTEXT && kSpecThreads > SIG_CTL_CONTEXT, "a one-column filter spreads its h + 1 <= 101 window rows over the threads");

// The ADSRARGS / ADSR pairs of n instructions (the header's words): an ADSR's other three registers ride in the ADSRARGS word
// right in front of it, both of one width and rate.  `op(k)` / `wide(k)`: instruction k's op and its `wide` bits.
template <typename Op, typename Wide>
constexpr bool pairs_formed(int n, Op op, Wide wide) {
    for (int k = 0; k < n; ++k) {
        if (op(k) == SIG_CTL_ADSR && (k == 0 || op(k - 1) != SIG_CTL_ADSRARGS || wide(k - 1) != wide(k))) return false;
        if (op(k) == SIG_CTL_ADSRARGS && (k + 1 >= n || op(k + 1) != SIG_CTL_ADSR)) return false;
    }
    return true;
}

// One workgroup per block.  The last workgroup of a launch with a front position evaluates the program ONCE more, at that
// position, into the outputs' `front` rows (the controls of the block in front of the batch: sig_fused_*_fm's *_hist).
struct Block {
    bool front;
    int64_t b, position, step, min_position;
    __device__ __forceinline__ Block(int64_t position_, int64_t step_, int nblocks, int64_t front_position, int64_t min_position_) {
        front = front_position >= 0 && blockIdx.x == (unsigned)nblocks;
        b = front ? 0 : blockIdx.x;
        position = position_, step = step_, min_position = min_position_;
        if (front) { position = front_position; step = 0; }
    }
    __device__ __forceinline__ int64_t frame() const {
        int64_t frame = position + b * step;
        if (!front && frame < min_position) frame = min_position;              // (the first blocks of a run that starts before min_position are evaluated there)
        return frame;
    }
};
// a filter's history rows at that frame -- BlockLoc.before: min(100, p)
__device__ __forceinline__ int window_rows(int64_t frame) { return (int)(frame < SIG_CTL_CONTEXT ? frame : SIG_CTL_CONTEXT); }

__device__ __forceinline__ double row_value(const sig_ctl_ins& ins, int64_t b, int v) {
    return ins.row[(ins.rows > 1 ? b * (int64_t)(ins.stride ? ins.cols : 1) : 0) + (int64_t)(v < ins.cols ? v : 0) * ins.stride];
}

struct Carrier { int a, b, c; };            // an ADSRARGS word's registers: release, gate_on, gate_off

// The value `x` of instruction `I` (anything with op, kind, a, b, c) at `frame`, column v; false: it has none (an ADSRARGS, read
// by the ADSR behind it).  `mem`: the instruction with its pointer (ROW: the rows, NOISE: the seed); `get(r)`: register r, 0.0
// for r < 0; `carrier()`: the Carrier of an ADSR.  `narrow`: a history row of a filter's window -- every node's reply is
// float32 audio there.  EXT: also NOISE and `narrow`; ENV: also the ADSR pair (handlers a variant cannot reach are not compiled;
// without EXT only OSC reads a frame, the block's own).
template <bool EXT, bool ENV, typename Word, typename Get, typename CarrierOf>
__device__ __forceinline__ double value(const Word& I, const sig_ctl_ins& mem, const Block& blk, int v, int64_t frame, double rate, bool narrow,
                                      Get get, CarrierOf carrier)
{
    double x;
    switch (I.op) {
        case SIG_CTL_ROW: x = row_value(mem, blk.b, v); break;
        case SIG_CTL_OSC: {
            if (!EXT) frame = blk.frame();
            const double t = (double)frame / rate * get(I.a) + get(I.b);          // osc.py:32
            if (EXT && narrow) {                                                   // osc_bank.hip's f32 store path
                switch (I.kind) {
                    case SIG_OSC_SINE: x = sig_osc::osc_wave<SIG_OSC_SINE, float>(t); break;
                    case SIG_OSC_SQUARE: x = sig_osc::osc_wave<SIG_OSC_SQUARE, float>(t); break;
                    case SIG_OSC_SAWTOOTH: x = sig_osc::osc_wave<SIG_OSC_SAWTOOTH, float>(t); break;
                    default: x = sig_osc::osc_wave<SIG_OSC_TRIANGLE, float>(t); break;
                }
                break;
            }
            switch (I.kind) {
                case SIG_OSC_SINE: x = sig_osc::osc_sine(t); break;
                case SIG_OSC_SQUARE: x = sig_osc::osc_square(t); break;
                case SIG_OSC_SAWTOOTH: x = sig_osc::osc_sawtooth(t); break;
                default: x = sig_osc::osc_triangle(t); break;
            }
            break;
        }
        case SIG_CTL_MIX: { const double c = get(I.c); x = c * get(I.a) + (1.0 - c) * get(I.b); break; }   // fx.py:40
        case SIG_CTL_AMP: { const double a = get(I.a); x = copysign(pow(a, get(I.b)), a); break; }           // fx.py:60
        case SIG_CTL_NOISE:
            if (EXT) { x = sig_noise::noise_value((uint64_t)(uintptr_t)mem.row, frame, v); break; }         // noise.hip
            [[fallthrough]];
        case SIG_CTL_ADSRARGS:
            if (ENV) { x = 0.0; break; }
            [[fallthrough]];
        case SIG_CTL_ADSR:
            if (ENV) {                                                                                     // adsr.hip: the level at this one frame
                const Carrier g = carrier();
                const sig_env::Voice p = sig_env::make_voice(get(I.a), get(I.b), get(I.c), get(g.a), get(g.b), get(g.c));
                x = sig_env::level(p, (double)frame / rate);
                break;
            }
            [[fallthrough]];
        default: x = get(I.a) * get(I.b); break;                                                           // Gain, RingMod: fx.py:46, :52
    }
    if (EXT && narrow) x = (double)(float)x;
    return x;
}

// FILTER `f` (`kind`: SIG_FILT_LOWPASS / _HIGHPASS): the biquad designed from the cutoff, cold-started by its caller over the rows
// p - h .. p (biquad.hip: design_butter2, then sig_biquad::step); a refused cutoff is reported into the filter's status word
__device__ __forceinline__ void design(int kind, double cutoff, double rate, bool report, const sig_ctl_ins& f, sig_biquad::Biquad& q) {
    const bool ok = sig_biquad::design_butter2(kind, cutoff, rate, q);
    if (!ok && report && f.row) atomicOr(reinterpret_cast<int*>(const_cast<double*>(f.row)), SIG_STATUS_BAD_CUTOFF);
}

// the register value `x()` into output `o[k]`: the block's row, or the front row where the output has one.  WIDE: column v of its
// cols.  (Every operand is read where it is used, the value last: read ahead of the branches, the interpreter's loads move.)
template <bool WIDE, typename X>
__device__ __forceinline__ void store(const sig_ctl_out* o, int k, const Block& blk, int v, X x) {
    if (WIDE && v >= o[k].cols) return;
    if (!blk.front) o[k].out[WIDE ? blk.b * o[k].cols + v : blk.b] = x();
    else if (o[k].front) o[k].front[WIDE ? v : 0] = x();
}

}  // namespace sig_ctl
