// What the window-node files (delay.hip, fir.hip) share.  Both take a filter's window -- at most 100 context rows, then the launch's
// N * K rows -- in the layout (rows, voices), voices contiguous, lanes own voices.  Read straight from memory every lane of a wave
// would touch another row -- another cache line -- once per tap.  So a workgroup of WAVES waves stages a tile of (ROWS + 100) rows x 64
// voices of float32 input in LDS with coalesced 256-byte row loads (rows in front of absolute frame 0 are zero-filled, not read; no
// load passes the window's first or last row) and every lane then reads its own column: lane l's address is (row * 64 + l) * 4, bank
// l mod 32 whatever the row, so per-voice row offsets cost no bank conflict (ds_read_b32 is served in two groups of 32 lanes).  Tiles
// run over the launch's rows whatever the block size; a wave owns consecutive rows of its tile and re-reads the per-block control row
// only where the block changes.  float64 input (a one-frame request's window) takes a plain gather through the same code.
// Here: the shared members of the kernels' argument structs, the tile coordinates and a lane's column;
// on the host the entries' common argument checks, the grid and the in x out dtype dispatch.
#pragma once
#include "sig_common.h"

namespace sig_window {

constexpr int kHalo = 100;                                         // the context rows of a filter's window
static_assert(SIG_DELAY_CONTEXT == kHalo && SIG_FIR_CONTEXT == kHalo, "signals_amd.h: one context for every window node");

// ---- the shared members of a kernel's argument struct.  A file composes them in this order -- Frame, Input, Rows -- with its own
// members between and behind them and the output's leading dimension last: the kernels' scalar loads keep their offsets.
struct Frame { int N; int64_t rows; int c0; int voices; };        // rows = N * K output rows behind c0 context rows
struct Input { const void* in; int64_t ild; int ics; };           // the window, (c0 + rows, V | 1); ics == 0: one column
struct Rows { const double* ptr; int cs; int64_t rs; };           // per-block control, (1 | K, V | 1) f64; rs == 0: one row; NULL: unplugged

// ---- where a thread stands: voice tile vt, the tile's first output row t0 and its `count` rows, voice v (`live`: inside the launch).
// The helpers below take the kernel's arguments as values, each where the kernels first read it: handed the argument struct (by
// reference or by value) they moved the kernels' scalar loads and changed their code (tools/compare_kernels.py --by-content).
struct Tile { int lane, wave, vt; int64_t t0; int count; int v; bool live; };

template <int ROWS>
__device__ __forceinline__ Tile tile_at(int voice_tiles, int64_t rows, int voices)
{
    Tile c;
    c.lane = threadIdx.x & 63;
    c.wave = threadIdx.x >> 6;
    c.vt = blockIdx.x % voice_tiles;
    c.t0 = (int64_t)(blockIdx.x / voice_tiles) * ROWS;
    c.count = (int)((rows - c.t0 < ROWS) ? rows - c.t0 : ROWS);
    c.v = c.vt * SIG_WAVE + c.lane;
    c.live = c.v < voices;
    return c;
}

// this lane's column of the window (a dead lane: column 0, never read)
template <typename IN>
__device__ __forceinline__ const IN* column(const Tile& c, const void* in, int ics)
{
    return static_cast<const IN*>(in) + (c.live ? (int64_t)c.v * ics : 0);
}

// The staging loop, the read of a tile row and the start of the block walk are NOT here.  As a function handed `ild` and `w0` as
// values the staging loop had its row multiply's operands swapped throughout; handed them by reference it lost 68 instructions of
// delay.hip's kernels; a walk start handed N reordered fir.hip's loop tail.  So both files keep these written out, like the row
// lookup sig_coldstart.h tells of.  Their text (tile row t holds window row w0 + t, w0 = c0 + t0 - 100, so output row j reads tile
// rows j + 100 - k; rows in front of absolute frame 0 are zero-filled, not read; wave w owns rows [w * WAVE_ROWS, ...) of the tile):
//     for (int t = wave; t < count + 100; t += WAVES) tile[t * 64 + lane] = (w0 + t >= 0 && live) ? in[(w0 + t) * ild] : 0.0f;
//     b = (t0 + j0) / N;  n = (t0 + j0) - b * N;  ...  if (fresh) { fresh = false; <read Rows at b> }  ...  if (n == N) { n = 0; ++b; fresh = true; }

// ---- host: what both entries check the same way (the control row's strides and block count with them), and what they fill
inline bool args_ok(int32_t rate, int64_t position, int32_t block_frames, int32_t nblocks, int32_t context_rows, int32_t voices,
                    const void* in, int32_t in_dtype, int64_t in_ld, int32_t in_stride,
                    int32_t ctl_stride, int64_t ctl_row_stride, int32_t ctl_blocks, const void* out, int32_t out_dtype, int64_t out_ld)
{
    return rate > 0 && position >= 0 && block_frames >= 1 && nblocks >= 0 && voices >= 0 &&
           context_rows >= 0 && context_rows <= kHalo && context_rows == (position < kHalo ? position : (int64_t)kHalo) &&
           in != nullptr && out != nullptr && out_ld >= voices &&
           (in_dtype == SIG_F32 || in_dtype == SIG_F64) && (out_dtype == SIG_F32 || out_dtype == SIG_F64) &&
           (in_stride == 0 || in_stride == 1) && in_ld >= (in_stride ? voices : 1) &&
           (ctl_stride == 0 || ctl_stride == 1) && ctl_row_stride >= 0 && (ctl_blocks == 1 || ctl_blocks == nblocks);
}
inline Frame frame(int32_t block_frames, int32_t nblocks, int32_t context_rows, int32_t voices) {
    return Frame{block_frames, (int64_t)block_frames * nblocks, context_rows, voices};
}
inline Rows rows(const double* ptr, int32_t stride, int64_t row_stride, int32_t blocks) {
    return Rows{ptr, stride, (blocks > 1) ? row_stride : 0};
}

// one workgroup per tile of `tile_rows` rows x 64 voices (false: more than a grid dimension holds)
inline bool workgroups(const Frame& f, int tile_rows, int& voice_tiles, unsigned& nwg)
{
    voice_tiles = (f.voices + SIG_WAVE - 1) / SIG_WAVE;
    const int64_t n = ((f.rows + tile_rows - 1) / tile_rows) * voice_tiles;
    if (n > 0x7fffffffLL) return false;
    nwg = (unsigned)n;
    return true;
}

// launch(IN(), OUT* out) with the buffers' types float | double (the dtypes are checked: args_ok)
template <typename F>
int dispatch(int32_t in_dtype, int32_t out_dtype, void* out, F&& launch)
{
    if (in_dtype == SIG_F32)
        return (out_dtype == SIG_F32) ? launch(float(), static_cast<float*>(out)) : launch(float(), static_cast<double*>(out));
    return (out_dtype == SIG_F32) ? launch(double(), static_cast<float*>(out)) : launch(double(), static_cast<double*>(out));
}

}  // namespace sig_window
