// Dense FIR filter for gfx950 (chain/ext.py FIR; build-defined, the reference has no counterpart): per voice and block
//   w = clip(floor(select), 0, W - 1);  acc = h[0, w] * x[n];  acc = acc + h[k, w] * x[n - k]  for k = 1 .. L - 1 ascending;  out[n] = acc
// in float64, every operation rounded once in that order (built with -ffp-contract=off; the arithmetic is sig_fir.h's, the text the
// host test compiles too), x[m] = +0 for an absolute frame m < 0, no tap skipped -- zero taps and the zero-filled rows are multiplied
// and added like the rest, so NaN and inf propagate as the numpy restatement's do.
//
// Layout (rows, voices), voices contiguous, lanes own voices.  A 1024-thread workgroup stages a tile of (kTileRows + 100) rows x 64
// voices of float32 input in LDS with coalesced 256-byte row loads, as delay.hip does (rows in front of absolute frame 0 are
// zero-filled, not read; no load passes the window's first or last row), and the launch's (L, W) float64 table beside it, row-major as
// it is given: at one k the lanes of a wave read h[k, w_lane], equal columns one address (a broadcast), different columns consecutive
// doubles -- different banks up to 32 columns apart.  The naive loop reads one x and one tap per multiply.  Here a lane computes a RUN
// of kRun = 8 consecutive output rows at once: tap k is read once per run and serves 8 products, and the input slides through a ring of
// 8 registers -- going from k to k + 1 the run needs x[j - k - 1] as its one new value and drops x[j + 7 - k].  The k loop is
// unrolled 8 times so that the ring's slots are fixed registers.  Per k and lane: 1 ds_read_b32 + 1 ds_read_b64 and one widening for
// 8 multiplies and 8 additions.  L is wave-uniform (one per launch).  A run ends at its block's last row: the column is re-derived there
// and nothing but the taps is read anew.  A wave owns 16 consecutive rows of its tile, two full runs where no block ends inside them.
// float64 input (a one-frame request's window) takes a plain gather through the same loop.
// LDS: 356 x 64 x 4 B = 91136 B of input + 4096 x 8 B = 32768 B of table = 123904 B: one workgroup of 16 waves per CU, 4 per SIMD.
// Roofline: 4 B read (x 356 / 256 for the halo) + 4 B written and 2 L - 1 f64 operations per voice-sample, f32 in and out.
#include <type_traits>

#include "sig_common.h"
#include "sig_fir.h"

namespace {

constexpr int kTileRows = SIG_FIR_TILE_ROWS;
constexpr int kHalo = sig_fir::kContext;
constexpr int kFirWaves = 16;
constexpr int kRun = 8;                                            // consecutive output rows a lane computes at once
constexpr int kWaveRows = kTileRows / kFirWaves;

static_assert(sig_fir::kContext == SIG_FIR_CONTEXT && sig_fir::kMaxTaps == SIG_FIR_MAX_TAPS && sig_fir::kMaxPoints == SIG_FIR_MAX_POINTS,
              "sig_fir.h and signals_amd.h disagree");
static_assert(kTileRows % (kFirWaves * kRun) == 0, "a wave's rows are whole runs");
static_assert(sig_fir::kMaxTaps - 1 <= kHalo, "the last tap reads the halo's first row");
static_assert((kTileRows + kHalo) * SIG_WAVE * sizeof(float) + sig_fir::kMaxPoints * sizeof(double) <= 160 * 1024, "one workgroup per CU");

struct FirArgs {
    int N; int64_t rows; int c0; int voices;                       // rows = N * K output rows behind c0 context rows
    const void* in; int64_t ild; int ics;                          // the window, (c0 + rows, V | 1); ics == 0: one column
    const double* select; int ss; int64_t srs;                     // (1 | K, V | 1) f64; srs == 0: one row; NULL: column 0
    const double* taps; int L, W;                                  // (L, W) f64 on the device, row-major
    int64_t old;
};

// TILE: float32 input staged in LDS; otherwise every read goes to memory
template <typename IN, typename OUT, bool TILE>
__global__ __launch_bounds__(64 * kFirWaves) void fir_taps_kernel(FirArgs a, OUT* __restrict__ out, int voice_tiles)
{
    __shared__ float tile[TILE ? (kTileRows + kHalo) * SIG_WAVE : 1];
    __shared__ double tab[sig_fir::kMaxPoints];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int vt = blockIdx.x % voice_tiles;
    const int64_t t0 = (int64_t)(blockIdx.x / voice_tiles) * kTileRows;       // the tile's first output row
    const int count = (int)((a.rows - t0 < kTileRows) ? a.rows - t0 : kTileRows);
    const int v = vt * SIG_WAVE + lane;
    const bool live = v < a.voices;
    const IN* in = static_cast<const IN*>(a.in) + (live ? (int64_t)v * a.ics : 0);
    // output row t0 + j is window row c0 + t0 + j; tile row t holds window row w0 + t, so output row j reads tile rows j + 100 - k
    const int64_t w0 = (int64_t)a.c0 + t0 - kHalo;
    const int L = a.L, W = a.W;

    for (int i = threadIdx.x; i < L * W; i += 64 * kFirWaves) tab[i] = a.taps[i];       // L * W <= kMaxPoints (the entry checks)
    if constexpr (TILE) {
        const int total = count + kHalo;                                       // <= c0 + rows - w0: the window's last row at most
#pragma unroll 8
        for (int t = wave; t < total; t += kFirWaves) {
            const int64_t w = w0 + t;
            float x = 0.0f;                                                    // w < 0: in front of absolute frame 0 (c0 < 100 then)
            if (w >= 0 && live) x = in[w * a.ild];
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
            return (w >= 0 && live) ? (double)in[w * a.ild] : 0.0;
        }
    };

    const int j0 = wave * kWaveRows;
    const int j1 = (j0 + kWaveRows < count) ? j0 + kWaveRows : count;
    if (j0 >= j1) return;                                                      // wave-uniform, behind the barrier
    int64_t b = (t0 + j0) / a.N;                                               // wave-uniform: the block of row j
    int n = (int)((t0 + j0) - b * a.N);
    int col = 0;
    bool fresh = true;
    for (int j = j0; j < j1;) {
        if (fresh) {                                                           // once per block: the column
            fresh = false;
            col = (a.select && live) ? sig_fir::column(a.select[b * a.srs + (int64_t)v * a.ss], W) : 0;
        }
        int r = (j1 - j < kRun) ? j1 - j : kRun;                               // wave-uniform: the run's rows, inside the block
        if (a.N - n < r) r = a.N - n;
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
        if (n == a.N) { n = 0; ++b; fresh = true; }
    }
}

template <typename IN, typename OUT>
int launch_fir(const FirArgs& a, OUT* out, hipStream_t stream)
{
    const int voice_tiles = (a.voices + SIG_WAVE - 1) / SIG_WAVE;
    const int64_t nwg = ((a.rows + kTileRows - 1) / kTileRows) * voice_tiles;
    if (nwg > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    constexpr bool tile = std::is_same<IN, float>::value;
    fir_taps_kernel<IN, OUT, tile><<<(unsigned)nwg, 64 * kFirWaves, 0, stream>>>(a, out, voice_tiles);
    return sig_launch_status();
}

template <typename IN>
int dispatch_out(const FirArgs& a, void* out, int32_t out_dtype, hipStream_t s)
{
    if (out_dtype == SIG_F32) return launch_fir<IN, float>(a, static_cast<float*>(out), s);
    return launch_fir<IN, double>(a, static_cast<double*>(out), s);
}

}  // namespace

extern "C" int sig_fir_taps(int32_t rate, int64_t position, int32_t block_frames, int32_t nblocks, int32_t context_rows, int32_t voices,
                            const void* in, int32_t in_dtype, int64_t in_ld, int32_t in_stride,
                            const double* select, int32_t select_stride, int64_t select_row_stride, int32_t select_blocks,
                            const double* taps, int32_t table_taps, int32_t table_waves,
                            void* out, int32_t out_dtype, int64_t out_ld, void* stream)
{
    SIG_CHECK_ARG(rate > 0 && position >= 0 && block_frames >= 1 && nblocks >= 0 && voices >= 0);
    SIG_CHECK_ARG(taps != nullptr && table_taps >= 1 && table_taps <= SIG_FIR_MAX_TAPS && table_waves >= 1 &&
                  (int64_t)table_taps * table_waves <= SIG_FIR_MAX_POINTS);
    SIG_CHECK_ARG(context_rows >= 0 && context_rows <= SIG_FIR_CONTEXT &&
                  context_rows == (position < SIG_FIR_CONTEXT ? position : (int64_t)SIG_FIR_CONTEXT));
    SIG_CHECK_ARG(in != nullptr && out != nullptr && out_ld >= voices);
    SIG_CHECK_ARG((in_dtype == SIG_F32 || in_dtype == SIG_F64) && (out_dtype == SIG_F32 || out_dtype == SIG_F64));
    SIG_CHECK_ARG((in_stride == 0 || in_stride == 1) && in_ld >= (in_stride ? voices : 1));
    SIG_CHECK_ARG((select_stride == 0 || select_stride == 1) && select_row_stride >= 0 && (select_blocks == 1 || select_blocks == nblocks));
    if (nblocks == 0 || voices == 0) return 0;
    FirArgs a{};
    a.N = block_frames; a.rows = (int64_t)block_frames * nblocks; a.c0 = context_rows; a.voices = voices;
    a.in = in; a.ild = in_ld; a.ics = in_stride;
    a.select = select; a.ss = select_stride; a.srs = (select_blocks > 1) ? select_row_stride : 0;
    a.taps = taps; a.L = table_taps; a.W = table_waves;
    a.old = out_ld;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (in_dtype == SIG_F32) return dispatch_out<float>(a, out, out_dtype, s);
    return dispatch_out<double>(a, out, out_dtype, s);
}
