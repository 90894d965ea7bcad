// Table-lookup waveshaper for gfx950 (chain/ext.py Shaper; build-defined, the reference has no counterpart): a memoryless
// transfer curve read at the SIGNAL's value.  `table` is (T, W) float32 -- W curves of T points spanning input -1 .. +1:
//   c = clip(x, -1, 1);  u = (c + 1) * ((T - 1) / 2);  i = min(floor(u), T - 2);  f = u - i
//   out = tbl[i, w] + f * (tbl[i + 1, w] - tbl[i, w]),   w = clip(floor(select), 0, W - 1) per voice
// in float64, every operation rounded once in that order (built with -ffp-contract=off), so the value in front of the store has
// numpy's bits; NaN in, NaN out (the index of a NaN is 0, f carries it).
//
// A 512-thread workgroup stages the table in LDS once (sig_table.h: the layout and staging loop of the wavetable oscillator; the
// guard entry is never read here, i + 1 <= T - 1) and then walks `groups` 16-row groups per wave of its 64 * VEC voices: lanes,
// rows and 16-byte accesses as in osc_bank_kernel.  A wave loads four rows before it computes and stores them, so four 1 KiB
// loads are in flight per wave.  The gather is one paired LDS read per sample at a data-dependent address: neighbouring voices
// with nearby sample values in one column fall on nearby banks, equal values on one address (a broadcast, no conflict).
// Roofline: 4 B read + 4 B written per voice-sample (f32 in and out).
#include "sig_param_rows.h"
#include "sig_table.h"

namespace {

constexpr int kRowsPerWave = 16;
constexpr int kShaperWaves = 8;
constexpr int kRowsInFlight = 4;

struct ShaperArgs {
    int64_t rows; int voices;
    const void* in; int64_t ild; int ics;                          // (rows|1, V|1): ild == 0 one row, ics == 0 one column
    const double* select; int ss; int64_t srs; int rps;            // (1|P, V|1) f64; rps rows share a select row (0: one row); NULL: column 0
    const float* table; int T, W;                                  // (T, W) row-major, device memory
    int groups;                                                    // 16-row groups per wave
};

// VEC voices per lane; IVEC: the lane's VEC input samples are one 16-byte (f32) / 32-byte (f64) access, like its store
template <int VEC, typename IN, typename OUT, bool IVEC>
__global__ __launch_bounds__(64 * kShaperWaves) void shaper_table_kernel(ShaperArgs a, OUT* __restrict__ out, int64_t ld, int voice_tiles)
{
    extern __shared__ float tab[];                                 // [W][T + 1], sig_table.h
    const int T = a.T, W = a.W, S = T + 1;
    sig_table::stage<64 * kShaperWaves>(tab, a.table, T, W);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int vt = blockIdx.x % voice_tiles;
    const int64_t rt = blockIdx.x / voice_tiles;
    const int v0 = (vt * SIG_WAVE + lane) * VEC;
    const double half = (double)(T - 1) * 0.5;                     // exact
    const int last = T - 2;
    const IN* in = static_cast<const IN*>(a.in);

    int col[VEC];                                                  // the voice's column: its first float in `tab`
#pragma unroll
    for (int i = 0; i < VEC; ++i) col[i] = 0;
    int64_t loaded = -1;                                           // select row currently in registers
    for (int g = 0; g < a.groups; ++g) {
        const int64_t r0 = ((rt * a.groups + g) * kShaperWaves + wave) * kRowsPerWave;
        if (r0 >= a.rows) break;                                   // wave-uniform
        for (int j0 = 0; j0 < kRowsPerWave; j0 += kRowsInFlight) {
            if (r0 + j0 >= a.rows) break;                          // wave-uniform
            double x[kRowsInFlight][VEC];
#pragma unroll
            for (int j = 0; j < kRowsInFlight; ++j) {
                const int64_t row = (r0 + j0 + j < a.rows) ? r0 + j0 + j : a.rows - 1;       // (a clamped row is loaded, not stored)
                const IN* src = in + row * a.ild;
                if constexpr (IVEC) {
                    typename sig_vec4<IN>::type q{};
                    if (v0 < a.voices) q = *reinterpret_cast<const typename sig_vec4<IN>::type*>(src + v0);   // voices % 4 == 0 on this path
                    x[j][0] = (double)q.x; x[j][1] = (double)q.y; x[j][2] = (double)q.z; x[j][3] = (double)q.w;
                } else {
#pragma unroll
                    for (int i = 0; i < VEC; ++i)
                        x[j][i] = (v0 + i < a.voices) ? (double)src[(int64_t)(v0 + i) * a.ics] : 0.0;
                }
            }
#pragma unroll
            for (int j = 0; j < kRowsInFlight; ++j) {
                const int64_t row = r0 + j0 + j;
                if (row >= a.rows) break;                          // wave-uniform
                const int64_t srow = a.rps ? row / a.rps : 0;      // wave-uniform
                if (a.select && srow != loaded) {
                    loaded = srow;
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        const int v = v0 + i;
                        col[i] = (v < a.voices) ? sig_table::column(a.select[srow * a.srs + (int64_t)v * a.ss], W) * S : 0;
                    }
                }
                OUT y[VEC];
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const double xi = x[j][i];
                    const double c = (xi < -1.0) ? -1.0 : ((xi > 1.0) ? 1.0 : xi);            // np.clip: NaN stays NaN
                    const double u = (c + 1.0) * half;             // in [0, T - 1], or NaN
                    const int k = (u >= 0.0) ? min((int)floor(u), last) : 0;                  // (NaN: entry 0; f below carries the NaN)
                    const double f = u - (double)k;                // in [0, 1]: x = +1 reads the last segment at f = 1
                    const int at = col[i] + k;                     // <= col + T - 2, so at + 1 stays inside the column
                    const double lo = (double)tab[at], hi = (double)tab[at + 1];
                    y[i] = (OUT)(lo + f * (hi - lo));
                }
                OUT* dst = out + row * ld + v0;
                if constexpr (VEC == 4) {
                    if (v0 < a.voices) {                           // voices % 4 == 0 on this path
                        typename sig_vec4<OUT>::type o;
                        o.x = y[0]; o.y = y[1]; o.z = y[2]; o.w = y[3];
                        *reinterpret_cast<typename sig_vec4<OUT>::type*>(dst) = o;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < VEC; ++i)
                        if (v0 + i < a.voices) dst[i] = y[i];
                }
            }
        }
    }
}

template <typename IN, typename OUT>
int launch_shaper(ShaperArgs a, OUT* out, int64_t ld, hipStream_t stream)
{
    const bool vec4 = (a.voices % 4 == 0) && (ld % 4 == 0) &&
                      ((reinterpret_cast<uintptr_t>(out) % (4 * sizeof(OUT))) == 0);
    const bool ivec = vec4 && a.ics == 1 && (a.ild % 4 == 0) &&
                      ((reinterpret_cast<uintptr_t>(a.in) % (4 * sizeof(IN))) == 0);
    const int span = SIG_WAVE * (vec4 ? 4 : 1);
    const int voice_tiles = (a.voices + span - 1) / span;
    const int64_t rows_per_pass = (int64_t)kRowsPerWave * kShaperWaves;
    const int64_t passes = (a.rows + rows_per_pass - 1) / rows_per_pass;
    // as many row groups per wave as still leave two workgroups for every CU of an MI355X (the staging is paid per workgroup)
    a.groups = 8;
    while (a.groups > 1 && ((passes + a.groups - 1) / a.groups) * voice_tiles < 512) a.groups >>= 1;
    const int64_t nwg = ((passes + a.groups - 1) / a.groups) * voice_tiles;
    if (nwg > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    const size_t lds = sig_table::lds_bytes(a.T, a.W);
    if (ivec)
        shaper_table_kernel<4, IN, OUT, true><<<(unsigned)nwg, 64 * kShaperWaves, lds, stream>>>(a, out, ld, voice_tiles);
    else if (vec4)
        shaper_table_kernel<4, IN, OUT, false><<<(unsigned)nwg, 64 * kShaperWaves, lds, stream>>>(a, out, ld, voice_tiles);
    else
        shaper_table_kernel<1, IN, OUT, false><<<(unsigned)nwg, 64 * kShaperWaves, lds, stream>>>(a, out, ld, voice_tiles);
    return sig_launch_status();
}

template <typename IN>
int run_shaper(const ShaperArgs& a, void* out, int32_t out_dtype, int64_t out_ld, hipStream_t s)
{
    return sig_rows::dispatch_out(out, out_dtype, [&](auto* o) { return launch_shaper<IN>(a, o, out_ld, s); });
}

}  // namespace

extern "C" int sig_shaper_table(int64_t rows, int32_t voices,
                                const void* in, int32_t in_dtype, int64_t in_ld, int32_t in_stride,
                                const double* select, int32_t select_stride, int64_t select_row_stride, int32_t rows_per_select,
                                const float* table, int32_t table_points, int32_t table_waves,
                                void* out, int32_t out_dtype, int64_t out_ld, void* stream)
{
    SIG_CHECK_ARG(rows >= 0 && voices >= 0 && rows_per_select >= 0);
    SIG_CHECK_ARG(in != nullptr && out != nullptr && out_ld >= voices);
    SIG_CHECK_ARG((in_dtype == SIG_F32 || in_dtype == SIG_F64) && (out_dtype == SIG_F32 || out_dtype == SIG_F64));
    SIG_CHECK_ARG((in_stride == 0 || in_stride == 1) && (in_ld == 0 || in_ld >= (in_stride ? voices : 1)));
    SIG_CHECK_ARG(sig_rows::strides_ok(select_stride, select_row_stride));
    SIG_CHECK_ARG(table != nullptr && table_points >= 2 && table_waves >= 1 &&
                  (int64_t)table_points * table_waves <= SIG_TABLE_MAX_POINTS);
    if (rows == 0 || voices == 0) return 0;
    const ShaperArgs a{rows, voices, in, in_ld, in_stride, select, select_stride, select_row_stride, rows_per_select,
                       table, table_points, table_waves, 1};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (in_dtype == SIG_F32) return run_shaper<float>(a, out, out_dtype, out_ld, s);
    return run_shaper<double>(a, out, out_dtype, out_ld, s);
}
