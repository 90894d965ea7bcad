// Dense FIR filter for gfx950 (chain/ext.py FIR; build-defined, the reference has no counterpart): per voice and block
//   w = clip(floor(select), 0, W - 1);  acc = h[0, w] * x[n];  acc = acc + h[k, w] * x[n - k]  for k = 1 .. L - 1 ascending;  out[n] = acc
// in float64, every operation rounded once in that order (built with -ffp-contract=off; the arithmetic is sig_fir.h's, the text the
// host test compiles too), x[m] = +0 for an absolute frame m < 0, no tap skipped -- zero taps and the zero-filled rows are multiplied
// and added like the rest, so NaN and inf propagate as the numpy restatement's do.
//
// The window's layout and its float32 tile in LDS are described in sig_window_tile.h, which also holds what this file shares with
// delay.hip: the argument struct's common members, the tile coordinates, the entry's common checks, the grid and the dtype dispatch (and
// says why the staging loop and the block walk's start are written out here all the same).
// Here: a 1024-thread workgroup, tiles of 256 rows, and the launch's (L, W) float64 table in LDS beside the input
// tile, row-major as it is given: at one k the lanes of a wave read h[k, w_lane], equal columns one address (a broadcast), different
// columns consecutive doubles -- different banks up to 32 columns apart.  The naive loop reads one x and one tap per multiply.  Here a
// lane computes a RUN of kRun = 8 consecutive output rows at once: tap k is read once per run and serves 8 products, and the input
// slides through a ring of 8 registers -- going from k to k + 1 the run needs x[j - k - 1] as its one new value and drops x[j + 7 - k].
// The k loop is unrolled 8 times so that the ring's slots are fixed registers.  Per k and lane: 1 ds_read_b32 + 1 ds_read_b64 and one
// widening for 8 multiplies and 8 additions.  L is wave-uniform (one per launch).  A run ends at its block's last row: the column is
// re-derived there and nothing but the taps is read anew.  A wave owns 16 consecutive rows of its tile, two full runs where no block
// ends inside them.  float64 input (a one-frame request's window) takes a plain gather through the same loop.
// LDS: 356 x 64 x 4 B = 91136 B of input + 4096 x 8 B = 32768 B of table = 123904 B: one workgroup of 16 waves per CU, 4 per SIMD.
// Roofline: 4 B read (x 356 / 256 for the halo) + 4 B written and 2 L - 1 f64 operations per voice-sample, f32 in and out.
#include <type_traits>

#include "sig_window_tile.h"
#include "sig_fir.h"

namespace {

constexpr int kTileRows = SIG_FIR_TILE_ROWS;
constexpr int kHalo = sig_window::kHalo;
constexpr int kFirWaves = 16;
constexpr int kRun = 8;                                            // consecutive output rows a lane computes at once
constexpr int kWaveRows = kTileRows / kFirWaves;

static_assert(sig_fir::kContext == kHalo && sig_fir::kContext == SIG_FIR_CONTEXT && sig_fir::kMaxTaps == SIG_FIR_MAX_TAPS && sig_fir::kMaxPoints == SIG_FIR_MAX_POINTS,
              "sig_fir.h and signals_amd.h disagree");
static_assert(kTileRows % (kFirWaves * kRun) == 0, "a wave's rows are whole runs");
static_assert(sig_fir::kMaxTaps - 1 <= kHalo, "the last tap reads the halo's first row");
static_assert((kTileRows + kHalo) * SIG_WAVE * sizeof(float) + sig_fir::kMaxPoints * sizeof(double) <= 160 * 1024, "one workgroup per CU");

struct FirArgs {
    sig_window::Frame f;
    sig_window::Input x;
    sig_window::Rows select;                                       // NULL: column 0
    const double* taps; int L, W;                                  // (L, W) f64 on the device, row-major
    int64_t old;
};

// TILE: float32 input staged in LDS; otherwise every read goes to memory
template <typename IN, typename OUT, bool TILE>
__global__ __launch_bounds__(64 * kFirWaves) void fir_taps_kernel(FirArgs a, OUT* __restrict__ out, int voice_tiles)
{
    __shared__ float tile[TILE ? (kTileRows + kHalo) * SIG_WAVE : 1];
    __shared__ double tab[sig_fir::kMaxPoints];
    const sig_window::Tile c = sig_window::tile_at<kTileRows>(voice_tiles, a.f.rows, a.f.voices);
    const IN* in = sig_window::column<IN>(c, a.x.in, a.x.ics);
    const int lane = c.lane, v = c.v;
    const bool live = c.live;
    const int64_t t0 = c.t0, w0 = (int64_t)a.f.c0 + t0 - kHalo;
    const int L = a.L, W = a.W;

    for (int i = threadIdx.x; i < L * W; i += 64 * kFirWaves) tab[i] = a.taps[i];       // L * W <= kMaxPoints (the entry checks)
    if constexpr (TILE) {                                                      // written out: sig_window_tile.h says why
        const int total = c.count + kHalo;                                     // <= c0 + rows - w0: the window's last row at most
#pragma unroll 8
        for (int t = c.wave; t < total; t += kFirWaves) {
            const int64_t w = w0 + t;
            float x = 0.0f;                                                    // w < 0: in front of absolute frame 0 (c0 < 100 then)
            if (w >= 0 && live) x = in[w * a.x.ild];
            tile[t * SIG_WAVE + lane] = x;
        }
    }
    __syncthreads();

    // tile row t of this lane's voice, widened exactly; t <= count + 99 wherever it is called
    auto x_at = [&](int t) -> double {
        if constexpr (TILE) {
            return (double)tile[t * SIG_WAVE + lane];
        } else {
            const int64_t w = w0 + t;
            return (w >= 0 && live) ? (double)in[w * a.x.ild] : 0.0;
        }
    };

    const int j0 = c.wave * kWaveRows;
    const int j1 = (j0 + kWaveRows < c.count) ? j0 + kWaveRows : c.count;
    if (j0 >= j1) return;                                                      // wave-uniform, behind the barrier
    int64_t b = (t0 + j0) / a.f.N;                                             // wave-uniform: the block of row j
    int n = (int)((t0 + j0) - b * a.f.N);
    int col = 0;
    bool fresh = true;
    for (int j = j0; j < j1;) {
        if (fresh) {                                                           // once per block: the column
            fresh = false;
            col = (a.select.ptr && live) ? sig_fir::column(a.select.ptr[b * a.select.rs + (int64_t)v * a.select.cs], W) : 0;
        }
        int r = (j1 - j < kRun) ? j1 - j : kRun;                               // wave-uniform: the run's rows, inside the block
        if (a.f.N - n < r) r = a.f.N - n;
        double xr[kRun], acc[kRun];                                            // xr[i] = x[j + i - k] at the head of a chunk of taps
#pragma unroll
        for (int i = 0; i < kRun; ++i) xr[i] = (i < r) ? x_at(j + kHalo + i) : 0.0;       // (rows past the run are computed, not stored)
        const double* h = tab + col;                                           // h[k * W]: tap k of this lane's column
        {
            const double h0 = h[0];
#pragma unroll
            for (int i = 0; i < kRun; ++i) acc[i] = sig_fir::first(h0, xr[i]);
        }
        for (int k0 = 0; k0 + 1 < L; k0 += kRun) {
#pragma unroll
            for (int u = 1; u <= kRun; ++u) {
                const int k = k0 + u;
                if (k < L) {                                                   // uniform
                    const double hk = h[k * W];
                    xr[(kRun - u) % kRun] = x_at(j + kHalo - k);               // the slot of x[j + 8 - u - k0], which no row reads any more
#pragma unroll
                    for (int i = 0; i < kRun; ++i) acc[i] = sig_fir::next(acc[i], hk, xr[(i - u + kRun) % kRun]);
                }
            }
        }
        if (live) {
#pragma unroll
            for (int i = 0; i < kRun; ++i)
                if (i < r) out[(t0 + j + i) * a.old + v] = (OUT)acc[i];
        }
        j += r;
        n += r;
        if (n == a.f.N) { n = 0; ++b; fresh = true; }
    }
}

template <typename IN, typename OUT>
int launch_fir(const FirArgs& a, OUT* out, hipStream_t stream)
{
    int voice_tiles;
    unsigned nwg;
    if (!sig_window::workgroups(a.f, kTileRows, voice_tiles, nwg)) return (int)hipErrorInvalidValue;
    fir_taps_kernel<IN, OUT, std::is_same<IN, float>::value><<<nwg, 64 * kFirWaves, 0, stream>>>(a, out, voice_tiles);
    return sig_launch_status();
}

}  // namespace

extern "C" int sig_fir_taps(int32_t rate, int64_t position, int32_t block_frames, int32_t nblocks, int32_t context_rows, int32_t voices,
                            const void* in, int32_t in_dtype, int64_t in_ld, int32_t in_stride,
                            const double* select, int32_t select_stride, int64_t select_row_stride, int32_t select_blocks,
                            const double* taps, int32_t table_taps, int32_t table_waves,
                            void* out, int32_t out_dtype, int64_t out_ld, void* stream)
{
    SIG_CHECK_ARG(sig_window::args_ok(rate, position, block_frames, nblocks, context_rows, voices, in, in_dtype, in_ld, in_stride,
                                      select_stride, select_row_stride, select_blocks, out, out_dtype, out_ld));
    SIG_CHECK_ARG(taps != nullptr && table_taps >= 1 && table_taps <= SIG_FIR_MAX_TAPS && table_waves >= 1 &&
                  (int64_t)table_taps * table_waves <= SIG_FIR_MAX_POINTS);
    if (nblocks == 0 || voices == 0) return 0;
    FirArgs a{};
    a.f = sig_window::frame(block_frames, nblocks, context_rows, voices);
    a.x = {in, in_ld, in_stride};
    a.select = sig_window::rows(select, select_stride, select_row_stride, select_blocks);
    a.taps = taps; a.L = table_taps; a.W = table_waves;
    a.old = out_ld;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return sig_window::dispatch(in_dtype, out_dtype, out, [&](auto x, auto* o) { return launch_fir<decltype(x)>(a, o, s); });
}
