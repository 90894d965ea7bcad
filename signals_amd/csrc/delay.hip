// Short multi-tap delay line for gfx950 (chain/ext.py Delay; build-defined, the reference has no counterpart): per voice and block
//   d_u = clip((time * rate) * m_u, 0, 99);  i_u = floor(d_u);  f_u = d_u - i_u
//   out[n] = sum over u ascending of g_u * (x[n - i_u] + f_u * (x[n - i_u - 1] - x[n - i_u]))
// in float64, every operation rounded once in that order (built with -ffp-contract=off; the arithmetic is sig_delay.h's, the text the
// host test compiles too), x[m] = 0 for an absolute frame m < 0, NaN rows for a voice whose d_u is NaN.
//
// The window's layout and its float32 tile in LDS are described in sig_window_tile.h, which also holds what this file shares with
// fir.hip: the argument struct's common members, the tile coordinates, the entry's common checks, the grid and the dtype dispatch (and
// says why the staging loop and the block walk's start are written out here all the same).
// Here: a 512-thread workgroup, tiles of 220 rows -- (220 + 100) x 64 x 4 B = 80 KiB, two workgroups per CU inside the
// 160 KiB -- of which a wave owns 28 consecutive rows, re-deriving i_u and f_u only where the block changes; output row j reads tile
// rows j + 100 - i_u - {0, 1}.  The taps are unrolled 16 times behind a uniform `u < U`, so i_u and f_u stay in registers.
// Roofline: 4 B read (x 320 / 220 for the halo) + 4 B written per voice-sample, f32 in and out.
#include <type_traits>

#include "sig_window_tile.h"
#include "sig_delay.h"

namespace {

constexpr int kTileRows = SIG_DELAY_TILE_ROWS;
constexpr int kHalo = sig_window::kHalo;
constexpr int kDelayWaves = 8;
constexpr int kWaveRows = (kTileRows + kDelayWaves - 1) / kDelayWaves;
constexpr int kMaxTaps = sig_delay::kMaxTaps;

static_assert(sig_delay::kContext == kHalo && sig_delay::kContext == SIG_DELAY_CONTEXT && sig_delay::kMaxFrames == SIG_DELAY_MAX_FRAMES &&
              sig_delay::kMaxTaps == SIG_DELAY_MAX_TAPS, "sig_delay.h and signals_amd.h disagree");
static_assert((kTileRows + kHalo) * SIG_WAVE * sizeof(float) * 2 <= 160 * 1024, "two workgroups per CU");

struct DelayArgs {
    sig_window::Frame f;
    double rate;
    sig_window::Input x;
    sig_window::Rows time;                                         // seconds; NULL: 0
    int U; double m[kMaxTaps], g[kMaxTaps];                        // by value
    int64_t old;
};

// TILE: float32 input staged in LDS; otherwise every read goes to memory
template <typename IN, typename OUT, bool TILE>
__global__ __launch_bounds__(64 * kDelayWaves) void delay_taps_kernel(DelayArgs a, OUT* __restrict__ out, int voice_tiles)
{
    __shared__ float tile[TILE ? (kTileRows + kHalo) * SIG_WAVE : 1];
    const sig_window::Tile c = sig_window::tile_at<kTileRows>(voice_tiles, a.f.rows, a.f.voices);
    const IN* in = sig_window::column<IN>(c, a.x.in, a.x.ics);

    if constexpr (TILE) {                                                      // written out: sig_window_tile.h says why
        const int64_t w0 = (int64_t)a.f.c0 + c.t0 - kHalo;
        const int total = c.count + kHalo;                                     // <= c0 + rows - w0: the window's last row at most
#pragma unroll 8
        for (int j = c.wave; j < total; j += kDelayWaves) {
            const int64_t w = w0 + j;
            float x = 0.0f;                                                    // w < 0: in front of absolute frame 0 (c0 < 100 then)
            if (w >= 0 && c.live) x = in[w * a.x.ild];
            tile[j * SIG_WAVE + c.lane] = x;
        }
        __syncthreads();
    }

    const int j0 = c.wave * kWaveRows;
    const int j1 = (j0 + kWaveRows < c.count) ? j0 + kWaveRows : c.count;
    if (j0 >= j1) return;                                                      // wave-uniform, behind the barrier
    int64_t b = (c.t0 + j0) / a.f.N;                                           // wave-uniform: the block of row j
    int n = (int)((c.t0 + j0) - b * a.f.N);
    int ti[kMaxTaps];
    double tf[kMaxTaps];
    bool bad = false, fresh = true;
    for (int j = j0; j < j1; ++j) {
        if (fresh) {                                                           // once per block: i_u and f_u
            fresh = false;
            const double t = (a.time.ptr && c.live) ? a.time.ptr[b * a.time.rs + (int64_t)c.v * a.time.cs] : 0.0;
            bad = false;
#pragma unroll
            for (int u = 0; u < kMaxTaps; ++u)
                if (u < a.U) bad |= !sig_delay::tap(t, a.rate, a.m[u], ti[u], tf[u]);
        }
        double y = 0.0;
#pragma unroll
        for (int u = 0; u < kMaxTaps; ++u) {
            if (u < a.U) {                                                     // uniform
                double x0, x1;                                                 // tile rows j + 100 - i_u and the one below it
                if constexpr (TILE) {
                    const int at = (j + kHalo - ti[u]) * SIG_WAVE + c.lane;    // tile row >= j + 1, so the row below it is there too
                    x0 = (double)tile[at];
                    x1 = (double)tile[at - SIG_WAVE];
                } else {
                    const int64_t w = (int64_t)a.f.c0 + c.t0 + j - ti[u];
                    x0 = (w >= 0 && c.live) ? (double)in[w * a.x.ild] : 0.0;
                    x1 = (w >= 1 && c.live) ? (double)in[(w - 1) * a.x.ild] : 0.0;
                }
                y = sig_delay::add(u, y, a.g[u], sig_delay::read(x0, x1, tf[u]));
            }
        }
        if (bad) y = __builtin_nan("");
        if (c.live) out[(c.t0 + j) * a.old + c.v] = (OUT)y;
        if (++n == a.f.N) { n = 0; ++b; fresh = true; }
    }
}

template <typename IN, typename OUT>
int launch_delay(const DelayArgs& a, OUT* out, hipStream_t stream)
{
    int voice_tiles;
    unsigned nwg;
    if (!sig_window::workgroups(a.f, kTileRows, voice_tiles, nwg)) return (int)hipErrorInvalidValue;
    delay_taps_kernel<IN, OUT, std::is_same<IN, float>::value><<<nwg, 64 * kDelayWaves, 0, stream>>>(a, out, voice_tiles);
    return sig_launch_status();
}

}  // namespace

extern "C" int sig_delay_taps(int32_t rate, int64_t position, int32_t block_frames, int32_t nblocks, int32_t context_rows, int32_t voices,
                              const void* in, int32_t in_dtype, int64_t in_ld, int32_t in_stride,
                              const double* time, int32_t time_stride, int64_t time_row_stride, int32_t time_blocks,
                              int32_t taps, const double* multiplier, const double* gain,
                              void* out, int32_t out_dtype, int64_t out_ld, void* stream)
{
    SIG_CHECK_ARG(sig_window::args_ok(rate, position, block_frames, nblocks, context_rows, voices, in, in_dtype, in_ld, in_stride,
                                      time_stride, time_row_stride, time_blocks, out, out_dtype, out_ld));
    SIG_CHECK_ARG(taps >= 1 && taps <= SIG_DELAY_MAX_TAPS && multiplier != nullptr && gain != nullptr);
    if (nblocks == 0 || voices == 0) return 0;
    DelayArgs a{};
    a.f = sig_window::frame(block_frames, nblocks, context_rows, voices);
    a.rate = (double)rate;
    a.x = {in, in_ld, in_stride};
    a.time = sig_window::rows(time, time_stride, time_row_stride, time_blocks);
    a.U = taps;
    for (int u = 0; u < taps; ++u) { a.m[u] = multiplier[u]; a.g[u] = gain[u]; }
    a.old = out_ld;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return sig_window::dispatch(in_dtype, out_dtype, out, [&](auto x, auto* o) { return launch_delay<decltype(x)>(a, o, s); });
}
