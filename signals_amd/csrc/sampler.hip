// Sample playback for gfx950 (chain/ext.py Sampler; build-defined, the reference has no counterpart): W recordings of T frames read
// with linear interpolation at a position that is a pure function of the absolute frame n, per voice
//   q = n / rate;  e = q - gate_on;  s = e * rate;  u = s * ratio + offset;  out = tbl[i, w] + f * (tbl[j, w] - tbl[i, w])
// in float64, every operation rounded once in that order (built with -ffp-contract=off; the arithmetic, the loop wrap, the neighbour
// rule and the silence / NaN / outside cases are sig_sampler.h's, the text the host test compiles too).
//
// Layout (rows, voices), voices contiguous, lanes own voices: a wave's row is one coalesced 256-byte float32 store.  The table sits in
// HBM column-major, each recording contiguous (the node uploads the transpose), so a lane that walks forward reads consecutive
// addresses of its own recording: a 128-byte line serves 32 / ratio of its rows, and the lane's next rows find it in the CU's L1 or in
// L2.  Every lane of a wave reads another line, so a row costs the wave up to 64 lines whatever the ratio; nothing is staged in LDS (the
// table has up to 2^26 points and every voice its own place in it).  A wave owns 32 consecutive rows of 64 voices: lanes 0 .. 31 each
// divide once for one row's q = n / rate and the row loop broadcasts it (v_readlane), so the per-sample cost is three f64 operations,
// the locate (a floor; a divide only behind a loop's end), two 4-byte loads and the lerp.  The row loop is unrolled four times and the two
// loads are unconditional -- a silent, NaN or dead lane reads entry 0 of a column that exists -- so eight loads per lane are in flight
// before the first is needed.  gate_on, ratio, offset and the column's base are read where the block changes, not per row.
// Roofline: 4 B written + 4 * max(ratio, 1/32) B of table lines read per voice-sample (f32 out).
#include <type_traits>

#include "sig_param_rows.h"
#include "sig_sampler.h"

namespace {

using sig_rows::row_value;
using Rows = sig_rows::Row;                                       // one control row: (1 | P, V | 1) f64, NULL = unplugged = 0

constexpr int kRowsPerWave = 32;
constexpr int kWavesPerWg = 4;
constexpr int kRowsInFlight = 4;

static_assert(kRowsPerWave % kRowsInFlight == 0 && kRowsPerWave <= 64, "the row loop's groups and the quotient lanes");

static_assert(sig_sampler::kMaxPoints == SIG_SAMPLER_MAX_POINTS, "sig_sampler.h and signals_amd.h disagree");

struct SamplerArgs {
    int64_t position, step; double rate; int64_t rows; int voices; int64_t rpp;   // rpp == 0: one control row for the launch
    Rows ratio, offset, gate, select;
    const float* table; int W;                                     // (W, T) row-major: recording w at table + w * T
    sig_sampler::Shape sh;
};

template <bool LOOP, typename OUT>
__global__ __launch_bounds__(64 * kWavesPerWg) void sampler_play_kernel(SamplerArgs a, OUT* __restrict__ out, int64_t ld, int voice_tiles)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int vt = blockIdx.x % voice_tiles;
    const int64_t rt = blockIdx.x / voice_tiles;
    const int v = vt * SIG_WAVE + lane;
    const bool live = v < a.voices;
    const int64_t r0 = (rt * kWavesPerWg + wave) * kRowsPerWave;
    if (r0 >= a.rows) return;                                      // wave-uniform
    const int count = (int)((a.rows - r0 < kRowsPerWave) ? a.rows - r0 : kRowsPerWave);

    // q = n / rate once per row for the wave: lane l holds the quotient of row r0 + (l & 31)
    const double q_lane = sig_sampler::quotient(a.position + (r0 + (lane & (kRowsPerWave - 1))) * a.step, a.rate);

    int64_t prow = a.rpp ? r0 / a.rpp : 0;                         // wave-uniform: the control row of row r0
    int64_t left = a.rpp ? a.rpp - (r0 - prow * a.rpp) : INT64_MAX;   // rows until the next one
    double gate = 0.0, ratio = 0.0, offset = 0.0;
    const float* __restrict__ col = a.table;
    bool fresh = true;
    for (int j0 = 0; j0 < count; j0 += kRowsInFlight) {
        float lo[kRowsInFlight], hi[kRowsInFlight];
        double f[kRowsInFlight];
        int kind[kRowsInFlight];
        // the positions and the loads of four rows first, so that eight loads are out before the first value is needed
#pragma unroll
        for (int k = 0; k < kRowsInFlight; ++k) {
            const int j = j0 + k;                                  // < kRowsPerWave; rows past `count` are computed from what is loaded, not stored
            if (fresh && j < count) {                              // where the block changes: the four controls of this voice
                fresh = false;
                gate = row_value(a.gate, prow, v, live);
                ratio = row_value(a.ratio, prow, v, live);
                offset = row_value(a.offset, prow, v, live);
                col = a.table + (int64_t)sig_sampler::column(row_value(a.select, prow, v, live), a.W) * a.sh.T;
            }
            const double q = sig_readlane_f64(q_lane, j);
            bool on;
            const double u = sig_sampler::position(q, a.rate, gate, ratio, offset, on);
            int i, jn;
            const sig_sampler::Kind where = sig_sampler::locate<LOOP>(u, a.sh, i, jn, f[k]);
            lo[k] = col[i]; hi[k] = col[jn];                       // 0 <= i, jn < T always; entry 0 where nothing is read
            kind[k] = on ? (int)where : (int)sig_sampler::kSilence;
            if (--left == 0) { ++prow; left = a.rpp; fresh = true; }
        }
#pragma unroll
        for (int k = 0; k < kRowsInFlight; ++k) {
            double y = sig_sampler::lerp((double)lo[k], (double)hi[k], f[k]);
            y = (kind[k] == sig_sampler::kRead) ? y : ((kind[k] == sig_sampler::kNaN) ? __builtin_nan("") : 0.0);
            if (live && j0 + k < count) out[(r0 + j0 + k) * ld + v] = (OUT)y;
        }
    }
}

template <typename OUT>
int launch_sampler(const SamplerArgs& a, OUT* out, int64_t ld, hipStream_t s)
{
    const int voice_tiles = (a.voices + SIG_WAVE - 1) / SIG_WAVE;
    const int64_t rows_per_wg = (int64_t)kRowsPerWave * kWavesPerWg;
    const int64_t nwg = ((a.rows + rows_per_wg - 1) / rows_per_wg) * voice_tiles;
    if (nwg > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    if (a.sh.loop_end != 0)
        sampler_play_kernel<true, OUT><<<(unsigned)nwg, 64 * kWavesPerWg, 0, s>>>(a, out, ld, voice_tiles);
    else
        sampler_play_kernel<false, OUT><<<(unsigned)nwg, 64 * kWavesPerWg, 0, s>>>(a, out, ld, voice_tiles);
    return sig_launch_status();
}

}  // namespace

extern "C" int sig_sampler_play(int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                                int32_t voices, int32_t rows_per_param,
                                const double* ratio, int32_t ratio_stride, int64_t ratio_row_stride,
                                const double* offset, int32_t offset_stride, int64_t offset_row_stride,
                                const double* gate_on, int32_t gate_on_stride, int64_t gate_on_row_stride,
                                const double* select, int32_t select_stride, int64_t select_row_stride,
                                const float* table, int32_t table_frames, int32_t table_waves,
                                int32_t loop_start, int32_t loop_end,
                                void* out, int32_t out_dtype, int64_t out_ld, void* stream)
{
    SIG_CHECK_ARG(sig_rows::head_ok(position, position_step, rate, rows, voices, rows_per_param));
    SIG_CHECK_ARG(table != nullptr && out != nullptr && out_ld >= voices);
    SIG_CHECK_ARG(sig_sampler::shape_ok(table_frames, table_waves, loop_start, loop_end));
    SIG_CHECK_ARG(sig_rows::strides_ok(ratio_stride, ratio_row_stride) && sig_rows::strides_ok(offset_stride, offset_row_stride) &&
                  sig_rows::strides_ok(gate_on_stride, gate_on_row_stride) && sig_rows::strides_ok(select_stride, select_row_stride));
    SIG_CHECK_ARG(out_dtype == SIG_F32 || out_dtype == SIG_F64);
    if (rows == 0 || voices == 0) return 0;
    SamplerArgs a{};
    a.position = position; a.step = position_step; a.rate = (double)rate; a.rows = rows; a.voices = voices; a.rpp = rows_per_param;
    a.ratio = Rows{ratio, ratio_stride, ratio_row_stride};
    a.offset = Rows{offset, offset_stride, offset_row_stride};
    a.gate = Rows{gate_on, gate_on_stride, gate_on_row_stride};
    a.select = Rows{select, select_stride, select_row_stride};
    a.table = table; a.W = table_waves;
    a.sh = sig_sampler::shape(table_frames, loop_start, loop_end);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return sig_rows::dispatch_out(out, out_dtype, [&](auto* o) { return launch_sampler(a, o, out_ld, s); });
}
