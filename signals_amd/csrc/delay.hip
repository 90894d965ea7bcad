// Short multi-tap delay line for gfx950 (chain/ext.py Delay; build-defined, the reference has no counterpart): per voice and block
//   d_u = clip((time * rate) * m_u, 0, 99);  i_u = floor(d_u);  f_u = d_u - i_u
//   out[n] = sum over u ascending of g_u * (x[n - i_u] + f_u * (x[n - i_u - 1] - x[n - i_u]))
// in float64, every operation rounded once in that order (built with -ffp-contract=off; the arithmetic is sig_delay.h's, the text the
// host test compiles too), x[m] = 0 for an absolute frame m < 0, NaN rows for a voice whose d_u is NaN.
//
// Layout (rows, voices), voices contiguous, lanes own voices.  Read straight from memory every lane of a wave would touch another
// row -- another cache line -- twice per tap.  So a 512-thread workgroup stages a tile of (kTileRows + 100) rows x 64 voices of float32
// input in LDS with coalesced 256-byte row loads (rows in front of absolute frame 0 are zero-filled, not read; no load passes the
// window's first or last row) and every lane then reads its own column: lane l's address is (row * 64 + l) * 4, bank l mod 32
// whatever the row, so the per-voice offsets cost no bank conflict (ds_read_b32 is served in two groups of 32 lanes).  The tile is
// 320 x 64 x 4 B = 80 KiB: two workgroups per CU inside the 160 KiB.  Tiles run over the launch's rows whatever the block size; a wave
// owns 28 consecutive rows of its tile and re-derives i_u and f_u only where the block changes.  The taps are unrolled 16 times
// behind a uniform `u < U`, so i_u and f_u stay in registers.  float64 input (a one-frame request's window) takes a plain gather.
// Roofline: 4 B read (x 320 / 220 for the halo) + 4 B written per voice-sample, f32 in and out.
#include <type_traits>

#include "sig_common.h"
#include "sig_delay.h"

namespace {

constexpr int kTileRows = SIG_DELAY_TILE_ROWS;
constexpr int kHalo = sig_delay::kContext;
constexpr int kDelayWaves = 8;
constexpr int kWaveRows = (kTileRows + kDelayWaves - 1) / kDelayWaves;
constexpr int kMaxTaps = sig_delay::kMaxTaps;

static_assert(sig_delay::kContext == SIG_DELAY_CONTEXT && sig_delay::kMaxFrames == SIG_DELAY_MAX_FRAMES &&
              sig_delay::kMaxTaps == SIG_DELAY_MAX_TAPS, "sig_delay.h and signals_amd.h disagree");
static_assert((kTileRows + kHalo) * SIG_WAVE * sizeof(float) * 2 <= 160 * 1024, "two workgroups per CU");

struct DelayArgs {
    int N; int64_t rows; int c0; int voices;                       // rows = N * K output rows behind c0 context rows
    double rate;
    const void* in; int64_t ild; int ics;                          // the window, (c0 + rows, V | 1); ics == 0: one column
    const double* time; int ts; int64_t trs;                       // (1 | K, V | 1) f64; trs == 0: one row; NULL: 0
    int U; double m[kMaxTaps], g[kMaxTaps];                        // by value
    int64_t old;
};

// TILE: float32 input staged in LDS; otherwise every read goes to memory
template <typename IN, typename OUT, bool TILE>
__global__ __launch_bounds__(64 * kDelayWaves) void delay_taps_kernel(DelayArgs a, OUT* __restrict__ out, int voice_tiles)
{
    __shared__ float tile[TILE ? (kTileRows + kHalo) * SIG_WAVE : 1];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int vt = blockIdx.x % voice_tiles;
    const int64_t t0 = (int64_t)(blockIdx.x / voice_tiles) * kTileRows;       // the tile's first output row
    const int count = (int)((a.rows - t0 < kTileRows) ? a.rows - t0 : kTileRows);
    const int v = vt * SIG_WAVE + lane;
    const bool live = v < a.voices;
    const IN* in = static_cast<const IN*>(a.in) + (live ? (int64_t)v * a.ics : 0);
    // output row t0 + j is window row c0 + t0 + j; tile row j holds window row w0 + j, so output row j reads tile rows j + 100 - i - {0, 1}
    const int64_t w0 = (int64_t)a.c0 + t0 - kHalo;

    if constexpr (TILE) {
        const int total = count + kHalo;                                       // <= c0 + rows - w0: the window's last row at most
#pragma unroll 8
        for (int j = wave; j < total; j += kDelayWaves) {
            const int64_t w = w0 + j;
            float x = 0.0f;                                                    // w < 0: in front of absolute frame 0 (c0 < 100 then)
            if (w >= 0 && live) x = in[w * a.ild];
            tile[j * SIG_WAVE + lane] = x;
        }
        __syncthreads();
    }

    const int j0 = wave * kWaveRows;
    const int j1 = (j0 + kWaveRows < count) ? j0 + kWaveRows : count;
    if (j0 >= j1) return;                                                      // wave-uniform, behind the barrier
    int64_t b = (t0 + j0) / a.N;                                               // wave-uniform: the block of row j
    int n = (int)((t0 + j0) - b * a.N);
    int ti[kMaxTaps];
    double tf[kMaxTaps];
    bool bad = false, fresh = true;
    for (int j = j0; j < j1; ++j) {
        if (fresh) {                                                           // once per block: i_u and f_u
            fresh = false;
            const double t = (a.time && live) ? a.time[b * a.trs + (int64_t)v * a.ts] : 0.0;
            bad = false;
#pragma unroll
            for (int u = 0; u < kMaxTaps; ++u)
                if (u < a.U) bad |= !sig_delay::tap(t, a.rate, a.m[u], ti[u], tf[u]);
        }
        double y = 0.0;
#pragma unroll
        for (int u = 0; u < kMaxTaps; ++u) {
            if (u < a.U) {                                                     // uniform
                double x0, x1;
                if constexpr (TILE) {
                    const int at = (j + kHalo - ti[u]) * SIG_WAVE + lane;      // tile row >= j + 1, so the row below it is there too
                    x0 = (double)tile[at];
                    x1 = (double)tile[at - SIG_WAVE];
                } else {
                    const int64_t w = (int64_t)a.c0 + t0 + j - ti[u];
                    x0 = (w >= 0 && live) ? (double)in[w * a.ild] : 0.0;
                    x1 = (w >= 1 && live) ? (double)in[(w - 1) * a.ild] : 0.0;
                }
                y = sig_delay::add(u, y, a.g[u], sig_delay::read(x0, x1, tf[u]));
            }
        }
        if (bad) y = __builtin_nan("");
        if (live) out[(t0 + j) * a.old + v] = (OUT)y;
        if (++n == a.N) { n = 0; ++b; fresh = true; }
    }
}

template <typename IN, typename OUT>
int launch_delay(const DelayArgs& a, OUT* out, hipStream_t stream)
{
    const int voice_tiles = (a.voices + SIG_WAVE - 1) / SIG_WAVE;
    const int64_t nwg = ((a.rows + kTileRows - 1) / kTileRows) * voice_tiles;
    if (nwg > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    constexpr bool tile = std::is_same<IN, float>::value;
    delay_taps_kernel<IN, OUT, tile><<<(unsigned)nwg, 64 * kDelayWaves, 0, stream>>>(a, out, voice_tiles);
    return sig_launch_status();
}

template <typename IN>
int dispatch_out(const DelayArgs& a, void* out, int32_t out_dtype, hipStream_t s)
{
    if (out_dtype == SIG_F32) return launch_delay<IN, float>(a, static_cast<float*>(out), s);
    return launch_delay<IN, double>(a, static_cast<double*>(out), s);
}

}  // namespace

extern "C" int sig_delay_taps(int32_t rate, int64_t position, int32_t block_frames, int32_t nblocks, int32_t context_rows, int32_t voices,
                              const void* in, int32_t in_dtype, int64_t in_ld, int32_t in_stride,
                              const double* time, int32_t time_stride, int64_t time_row_stride, int32_t time_blocks,
                              int32_t taps, const double* multiplier, const double* gain,
                              void* out, int32_t out_dtype, int64_t out_ld, void* stream)
{
    SIG_CHECK_ARG(rate > 0 && position >= 0 && block_frames >= 1 && nblocks >= 0 && voices >= 0);
    SIG_CHECK_ARG(taps >= 1 && taps <= SIG_DELAY_MAX_TAPS && multiplier != nullptr && gain != nullptr);
    SIG_CHECK_ARG(context_rows >= 0 && context_rows <= SIG_DELAY_CONTEXT &&
                  context_rows == (position < SIG_DELAY_CONTEXT ? position : (int64_t)SIG_DELAY_CONTEXT));
    SIG_CHECK_ARG(in != nullptr && out != nullptr && out_ld >= voices);
    SIG_CHECK_ARG((in_dtype == SIG_F32 || in_dtype == SIG_F64) && (out_dtype == SIG_F32 || out_dtype == SIG_F64));
    SIG_CHECK_ARG((in_stride == 0 || in_stride == 1) && in_ld >= (in_stride ? voices : 1));
    SIG_CHECK_ARG((time_stride == 0 || time_stride == 1) && time_row_stride >= 0 && (time_blocks == 1 || time_blocks == nblocks));
    if (nblocks == 0 || voices == 0) return 0;
    DelayArgs a{};
    a.N = block_frames; a.rows = (int64_t)block_frames * nblocks; a.c0 = context_rows; a.voices = voices;
    a.rate = (double)rate;
    a.in = in; a.ild = in_ld; a.ics = in_stride;
    a.time = time; a.ts = time_stride; a.trs = (time_blocks > 1) ? time_row_stride : 0;
    a.U = taps;
    for (int u = 0; u < taps; ++u) { a.m[u] = multiplier[u]; a.g[u] = gain[u]; }
    a.old = out_ld;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (in_dtype == SIG_F32) return dispatch_out<float>(a, out, out_dtype, s);
    return dispatch_out<double>(a, out, out_dtype, s);
}
