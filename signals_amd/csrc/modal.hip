// Modal resonator bank for gfx950 (chain/ext.py Modal; build-defined, the reference has no counterpart): per voice up to 64 exponentially
// decaying sinusoids struck at gate_on, each with its own frequency ratio, amplitude and decay rate from a float64 (W, M, 3) table,
//   q = n / rate;  e = q - gate_on;  not (e >= 0) -> 0
//   F_i = hertz * r_i;  g_i = clip(((rate / 2) - |F_i|) / |hertz|, 0, 1)
//   out = sum_i (a_i g_i) exp(-(lambda_i + damp) e) sin(2 pi mod(e F_i, 1))
// a pure function of the absolute frame.  The definition (include/signals_amd.h) is in float64, every operation rounded; this kernel is
// held to 1e-6 * max(1, sum |a|) against it, not to bits, because it does not evaluate exp and sin per sample:
//
// Runs.  The rows of a launch lie on the lattice L = position / step + row; a RUN is the 64 lattice rows [64 k, 64 k + 64).  One wave
// renders one run of 64 voices (lanes own voices: a row's float32 store is one coalesced 256 bytes).  Per voice and mode the run starts
// from the closed form -- one exp and one sine / cosine pair at the voice's first sounding row of the run -- and advances by the
// complex multiplier  w = exp(-(lambda + damp) dt) (cos, sin)(2 pi F dt),  dt = step / rate:  z' = z w, 4 multiplies and 2 additions,
// and the sample's sum takes Im z, one more addition: 7 float64 operations per mode and sample, none fused (built with
// -ffp-contract=off; the definition has no fused operation and neither has the recurrence).  The amplitude a g is folded into the seed,
// so a run's first sounding row has the definition's own product ((a g) exp(-k)) sin.
// A run always starts from its first LATTICE row, also where the launch begins or ends inside it or where a parameter row changes
// inside it (the part is then rendered once per parameter row, each from the run's start): a sample's bits depend on its frame, its
// voice's parameters and the lattice, not on how a stretch of frames is cut into launches or blocks.  That is what makes a block
// rendered alone and the same block inside a batch equal bit for bit.
// The strike.  e is monotone in the row, so a voice's silent rows are a prefix of the run: js rows, counted per lane only in a run some
// lane of which is struck (else 0 for all).  The lane seeds at ITS row js, where e >= 0 is the definition's e -- no exp of a positive
// argument is ever formed for the strike, a far-future gate included -- and its step t renders row js + t: accumulator t of a lane is
// its t-th sounding row, the indices stay static, and only a struck run stores rows that differ between lanes.  A part whose last
// row is silent for every lane stores zeros and evaluates nothing.
// Modes are the outer loop over a tile of 64 row accumulators held in registers (128 VGPRs); the mode's state is 4 doubles and its
// multiplier 4.  Per mode and run the set-up is a divide, two exp and two sine / cosine pairs (about 140 operations) against 448 in the
// recurrence.  The table sits in LDS, staged once per workgroup (sig_modal.h); a lane reads its set's row as three doubles, lanes of one
// set read one address.
// Error: the seed is exact to the exp's and the polynomial's 1e-16; 63 multiplications by w add < 63 * 3e-16 relative.  What the
// recurrence does NOT follow is the rounding of n / rate row by row: it advances the time by the exact dt, the definition by rounded
// quotients, half an ulp of q apart -- 3.6e-12 s at frame 2^31, times 2 pi F in the sample.  Measured: DESIGN.md.
// Roofline: 4 B written per voice-sample against 7 M float64 operations: float64-VALU-bound from the first mode on.
#include <type_traits>

#include "sig_modal.h"
#include "sig_osc.h"
#include "sig_param_rows.h"
#include "sig_table.h"

namespace {

using sig_rows::row_value;
using Rows = sig_rows::Row;                                       // one control row: (1 | P, V | 1) f64, NULL = unplugged = 0

constexpr int kRun = sig_modal::kRun;
constexpr int kWavesPerWg = 4;
constexpr int kGuard = 8;                                         // rows of the recurrence between two looks at the part's end

static_assert(kRun == SIG_WAVE, "lane l holds the quotient of a run's row l");
static_assert(sig_modal::kMaxModes == SIG_MODAL_MAX_MODES && sig_modal::kMaxPoints == SIG_MODAL_MAX_POINTS,
              "sig_modal.h and signals_amd.h disagree");

struct ModalArgs {
    int64_t position, step; double rate; int64_t rows; int voices; int64_t rpp;   // rpp == 0: one control row for the launch
    Rows hertz, gate, damp, select;
    const double* modes; int W, M;                                 // (W, M, 3) row-major
    int64_t base, first_run, runs;                                 // position / step; the first run's index; runs the launch touches
    int per_wave;                                                  // runs a wave renders
};

template <typename OUT>
__global__ __launch_bounds__(64 * kWavesPerWg) void modal_bank_kernel(ModalArgs a, OUT* __restrict__ out, int64_t ld, int voice_tiles)
{
    extern __shared__ double tab[];                                // [W][M][3]
    sig_modal::stage_rows<64 * kWavesPerWg>(tab, a.modes, a.W * a.M * 3);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int vt = blockIdx.x % voice_tiles;
    const int64_t rt = blockIdx.x / voice_tiles;
    const int v = vt * SIG_WAVE + lane;
    const bool live = v < a.voices;
    const double nyquist = 0.5 * a.rate;
    const double dt = (double)a.step / a.rate;                     // the time between two rows

    for (int g = 0; g < a.per_wave; ++g) {
        const int64_t run = (rt * a.per_wave + g) * kWavesPerWg + wave;
        if (run >= a.runs) break;                                  // wave-uniform
        const int64_t r0 = (a.first_run + run) * kRun - a.base;    // the launch row of the run's first lattice row (may lie outside)
        const int64_t lo = r0 > 0 ? r0 : 0;
        const int64_t hi = (r0 + kRun < a.rows) ? r0 + kRun : a.rows;
        // q = n / rate (one IEEE divide) of the run's 64 lattice rows, one per lane; the frame of every lattice row is >= 0
        const double q_lane = (double)(a.position + (r0 + lane) * a.step) / a.rate;
        const double q_first = sig_readlane_f64(q_lane, 0);

        int64_t prow = a.rpp ? lo / a.rpp : 0;
        for (int64_t part_lo = lo; part_lo < hi; ++prow) {         // the run's rows of one parameter row (wave-uniform bounds)
            int64_t part_hi = hi;
            if (a.rpp && (prow + 1) * a.rpp < hi) part_hi = (prow + 1) * a.rpp;
            const int first = (int)(part_lo - r0), count = (int)(part_hi - r0);       // rows [first, count) of the run are stored
            part_lo = part_hi;

            const double hz = row_value(a.hertz, prow, v, live);
            const double gate = row_value(a.gate, prow, v, live);
            const double damp = row_value(a.damp, prow, v, live);
            const int set = sig_table::column(row_value(a.select, prow, v, live), a.W) * a.M * 3;
            const int64_t at = r0 * ld + v;                        // row j of the run at out[at + j * ld]; only rows first .. count - 1 are touched

            const double q_end = sig_readlane_f64(q_lane, count - 1);
            if (__ballot(live && (q_end - gate >= 0.0)) == 0) {    // every voice still before its strike: zeros, nothing evaluated
                for (int j = first; j < count; ++j)
                    if (live) out[at + (int64_t)j * ld] = (OUT)0.0;
                continue;
            }
            // this voice's silent rows among the part's run rows 0 .. count - 1, and the definition's e at its first sounding row.  The
            // rows are taken from the broadcast quotients (v_readlane with a uniform index), never from a lane-indexed read of another
            // lane's register: that would return 0 from a lane the compiler has masked off
            int js = 0;
            double e0 = q_first - gate;
            const bool struck = __ballot(!(e0 >= 0.0)) != 0;       // (a dead lane has gate 0: never)
            if (struck) {
                e0 = 0.0;                                          // (a voice that stays silent seeds at 0 and stores nothing)
                for (int j = 0; j < count; ++j) {
                    const double ej = sig_readlane_f64(q_lane, j) - gate;
                    const bool on = ej >= 0.0;
                    if (on && js == j) e0 = ej;                    // e is monotone: the first sounding row follows js == j silent ones
                    js += on ? 0 : 1;
                }
            }
            const bool bad = !(fabs(hz) < (double)INFINITY && fabs(damp) < (double)INFINITY);   // NaN rows where it sounds

            double acc[kRun];
#pragma unroll
            for (int t = 0; t < kRun; ++t) acc[t] = 0.0;
            const double ahz = fabs(hz);
            for (int i = 0; i < a.M; ++i) {
                const double r = tab[set + 3 * i], amp = tab[set + 3 * i + 1], lambda = tab[set + 3 * i + 2];
                const double F = hz * r;
                const double fade = fmin(fmax((nyquist - fabs(F)) / ahz, 0.0), 1.0);  // IEEE: 0 Hz gives +inf -> 1
                const double decay = lambda + damp;
                const double m = sig_npmod_pow2<1>(e0 * F);
                const double level = (amp * fade) * exp(-(decay * e0));
                double sn, cs;
                sig_osc::cycle_sincos(m, sn, cs);
                double y = level * sn, x = level * cs;             // z = x + i y at the first sounding row
                double ws, wc;
                sig_osc::cycle_sincos(sig_npmod_pow2<1>(F * dt), ws, wc);
                const double shrink = exp(-(decay * dt));
                double wr = shrink * wc, wi = shrink * ws;         // the step: z' = z w
                if (!(fade > 0.0)) { x = 0.0; y = 0.0; wr = 0.0; wi = 0.0; }          // a dropped mode adds exactly 0 (and no NaN of a huge F)
#pragma unroll
                for (int t0 = 0; t0 < kRun; t0 += kGuard) {
                    if (t0 < count) {                              // wave-uniform: no row of the part lies further
#pragma unroll
                        for (int t = t0; t < t0 + kGuard; ++t) {
                            acc[t] = acc[t] + y;
                            const double xn = x * wr - y * wi;
                            y = x * wi + y * wr;
                            x = xn;
                        }
                    }
                }
            }
            // accumulator t is row js + t of the run
#pragma unroll
            for (int t = 0; t < kRun; ++t) {
                const int j = js + t;
                if (live && j >= first && j < count) out[at + (int64_t)j * ld] = (OUT)(bad ? __builtin_nan("") : acc[t]);
            }
            if (struck)
                for (int j = first; j < count; ++j)
                    if (live && j < js) out[at + (int64_t)j * ld] = (OUT)0.0;
        }
    }
}

template <typename OUT>
int launch_modal(ModalArgs& a, OUT* out, int64_t ld, hipStream_t s)
{
    const int voice_tiles = (a.voices + SIG_WAVE - 1) / SIG_WAVE;
    // as many runs per wave as still leave four workgroups for every CU of an MI355X (the table is staged once per workgroup)
    a.per_wave = 8;
    auto groups = [&] { return (a.runs + (int64_t)kWavesPerWg * a.per_wave - 1) / ((int64_t)kWavesPerWg * a.per_wave); };
    while (a.per_wave > 1 && groups() * voice_tiles < 1024) a.per_wave >>= 1;
    const int64_t nwg = groups() * voice_tiles;
    if (nwg > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    modal_bank_kernel<OUT><<<(unsigned)nwg, 64 * kWavesPerWg, sig_modal::lds_bytes(a.W, a.M), s>>>(a, out, ld, voice_tiles);
    return sig_launch_status();
}

}  // namespace

extern "C" int sig_modal_bank(int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                              int32_t voices, int32_t rows_per_param,
                              const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                              const double* gate_on, int32_t gate_on_stride, int64_t gate_on_row_stride,
                              const double* damp, int32_t damp_stride, int64_t damp_row_stride,
                              const double* select, int32_t select_stride, int64_t select_row_stride,
                              const double* modes, int32_t sets, int32_t count,
                              void* out, int32_t out_dtype, int64_t out_ld, void* stream)
{
    SIG_CHECK_ARG(sig_rows::head_ok(position, position_step, rate, rows, voices, rows_per_param));
    SIG_CHECK_ARG(modes != nullptr && hertz != nullptr && out != nullptr && out_ld >= voices);
    SIG_CHECK_ARG(sig_modal::shape_ok(sets, count));
    SIG_CHECK_ARG(sig_rows::strides_ok(hertz_stride, hertz_row_stride) && sig_rows::strides_ok(gate_on_stride, gate_on_row_stride) &&
                  sig_rows::strides_ok(damp_stride, damp_row_stride) && sig_rows::strides_ok(select_stride, select_row_stride));
    SIG_CHECK_ARG(out_dtype == SIG_F32 || out_dtype == SIG_F64);
    if (rows == 0 || voices == 0) return 0;
    ModalArgs a{};
    a.position = position; a.step = position_step; a.rate = (double)rate; a.rows = rows; a.voices = voices; a.rpp = rows_per_param;
    a.hertz = Rows{hertz, hertz_stride, hertz_row_stride};
    a.gate = Rows{gate_on, gate_on_stride, gate_on_row_stride};
    a.damp = Rows{damp, damp_stride, damp_row_stride};
    a.select = Rows{select, select_stride, select_row_stride};
    a.modes = modes; a.W = sets; a.M = count;
    a.base = position / position_step;
    a.first_run = a.base / kRun;
    a.runs = (a.base + rows - 1) / kRun - a.first_run + 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return sig_rows::dispatch_out(out, out_dtype, [&](auto* o) { return launch_modal(a, o, out_ld, s); });
}
