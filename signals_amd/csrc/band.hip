// Cold-start 4th-order Butterworth band filters for gfx950: BandPass / BandStop as two DF2T biquad
// sections in series.  The reference's DoubleCritFilter (src/signals/chain/fx.py:132-163)
// raises TypeError at fx.py:99 on every block; its intent is
//   sos = butter(N=2, Wn=[low, high]/(rate/2), btype='bp'|'bs', output='sos');  y = sosfilt(sos, window)
// with the same [<=100 context | block] cold start as LowPass/HighPass.  Same mapping as biquad.hip's plain
// kernel (wave = 64*VPT voices of one block, serial over rows, register ring of row loads); 4 f64 state
// registers and 10 coefficients per voice.  HBM-bound: 8 B per voice-sample, 18 f64 ops.
// `param_blocks` > 1: row b of `low` / `high` holds block b's band (a swept band: an LFO on either edge, read at
// the block's position like biquad.hip's cutoff rows); the design stays once per wave, a wave being one block.
#include "sig_coldstart.h"

namespace {

using namespace sig_cold;
using sig_biquad::Biquad;
using sig_biquad::design_band2;

constexpr int kRing = 8;

template <typename T, int VPT>
__global__ __launch_bounds__(256) void band_coldstart_kernel(
    int type, double rate, int64_t position, int N, int K, int ctx, int voices,
    const double* __restrict__ low, int ls, const double* __restrict__ high, int hs, int param_blocks,
    const T* __restrict__ in, int64_t in_ld, T* __restrict__ out, int64_t out_ld,
    int voice_tiles, int* __restrict__ status)
{
    using Vec = typename RowVec<T, VPT>::type;
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int vt = (int)(item % voice_tiles);
    const int64_t b = item / voice_tiles;
    if (b >= K) return;
    const int v0 = (vt * SIG_WAVE + lane) * VPT;
    const bool live = v0 < voices;
    const int vc = live ? v0 : 0;
    const int64_t p_b = position + b * N;
    const int c = (int)((p_b < (int64_t)ctx) ? p_b : (int64_t)ctx);

    Biquad q1[VPT], q2[VPT];
    double s10[VPT], s11[VPT], s20[VPT], s21[VPT];
    bool ok = true;
    const int64_t lrow = (param_blocks > 1) ? b * (int64_t)(ls ? voices : 1) : 0;   // block b's row of each edge
    const int64_t hrow = (param_blocks > 1) ? b * (int64_t)(hs ? voices : 1) : 0;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int v = (vc + i < voices) ? vc + i : vc;
        ok &= design_band2(type, low[lrow + (int64_t)v * ls], high[hrow + (int64_t)v * hs], rate, q1[i], q2[i]);
        s10[i] = s11[i] = s20[i] = s21[i] = 0.0;
    }
    if (!ok && live && status) atomicOr(status, SIG_STATUS_BAD_CUTOFF);

    const int total = c + N;
    const T* src = in + (b * N - c) * in_ld + vc;
    T* dst = out + (b * N - c) * out_ld + vc;
    Vec ring[kRing];
#pragma unroll
    for (int u = 0; u < kRing; ++u) {
        const int r = (u < total) ? u : total - 1;
        ring[u] = *reinterpret_cast<const Vec*>(src + (int64_t)r * in_ld);
    }
    for (int r0 = 0; r0 < total; r0 += kRing) {
#pragma unroll
        for (int u = 0; u < kRing; ++u) {
            const int r = r0 + u;
            if (r >= total) break;
            double x[VPT], y[VPT];
            unpack(ring[u], x);
            const int rn = (r + kRing < total) ? r + kRing : total - 1;
            ring[u] = *reinterpret_cast<const Vec*>(src + (int64_t)rn * in_ld);
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                // scipy _sosfilt: section by section for each sample, one rounding per op
                const double y1 = q1[i].b0 * x[i] + s10[i];
                s10[i] = q1[i].b1 * x[i] - q1[i].a1 * y1 + s11[i];
                s11[i] = q1[i].b2 * x[i] - q1[i].a2 * y1;
                y[i] = q2[i].b0 * y1 + s20[i];
                s20[i] = q2[i].b1 * y1 - q2[i].a1 * y[i] + s21[i];
                s21[i] = q2[i].b2 * y1 - q2[i].a2 * y[i];
            }
            if (r >= c && live) {
                Vec o; pack(o, y);
                *reinterpret_cast<Vec*>(dst + (int64_t)r * out_ld) = o;
            }
        }
    }
}

template <typename T>
int launch_band(int type, int32_t rate, int64_t position, int32_t N, int32_t K, int32_t ctx, int32_t voices,
                const double* low, int ls, const double* high, int hs, int param_blocks,
                const T* in, int64_t in_ld, T* out, int64_t out_ld, int32_t* status, hipStream_t stream)
{
    const bool vec4 = vec_ok(4, sizeof(T), voices, {in_ld, out_ld}, {in, out});
    const int voice_tiles = sig_voice_tiles(voices, vec4 ? 4 : 1);
    unsigned nwg;
    if (!sig_workgroups(sig_span_waves(voice_tiles, K, 1), nwg)) return (int)hipErrorInvalidValue;
    if (vec4)
        band_coldstart_kernel<T, 4><<<nwg, 256, 0, stream>>>(type, (double)rate, position, N, K, ctx, voices,
                                                                         low, ls, high, hs, param_blocks, in, in_ld, out, out_ld, voice_tiles, status);
    else
        band_coldstart_kernel<T, 1><<<nwg, 256, 0, stream>>>(type, (double)rate, position, N, K, ctx, voices,
                                                                         low, ls, high, hs, param_blocks, in, in_ld, out, out_ld, voice_tiles, status);
    return sig_launch_status();
}

int run_band(int type, int32_t rate, int64_t position, int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
             const double* low, int32_t low_stride, const double* high, int32_t high_stride, int32_t param_blocks,
             const void* in, int64_t in_ld, int64_t in_history, void* out, int64_t out_ld, int32_t dtype,
             int32_t* status, void* stream)
{
    SIG_CHECK_ARG(type == SIG_FILT_BANDPASS || type == SIG_FILT_BANDSTOP);
    bool empty;
    SIG_CHECK_ARG(window_ok(rate, position, block_frames, nblocks, context, voices, in, in_ld, in_history, out, empty) && out_ld >= voices);
    SIG_CHECK_ARG(rows_ok({low, low_stride, param_blocks}, nblocks, true) && rows_ok({high, high_stride, param_blocks}, nblocks, true));
    if (empty) return 0;
    return dispatch_dtype(dtype, in, out, [&](auto* x, auto* y) {
        return launch_band(type, rate, position, block_frames, nblocks, context, voices, low, low_stride, high, high_stride,
                           param_blocks, x, in_ld, y, out_ld, status, static_cast<hipStream_t>(stream));
    });
}

}  // namespace

extern "C" int sig_band_coldstart(int type, int32_t rate, int64_t position,
                                  int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                  const double* low, int32_t low_stride, const double* high, int32_t high_stride,
                                  const void* in, int64_t in_ld, int64_t in_history,
                                  void* out, int64_t out_ld, int32_t dtype,
                                  int32_t* status, void* stream)
{
    return run_band(type, rate, position, block_frames, nblocks, context, voices, low, low_stride, high, high_stride, 1,
                    in, in_ld, in_history, out, out_ld, dtype, status, stream);
}

extern "C" int sig_band_coldstart_blocks(int type, int32_t rate, int64_t position,
                                         int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                         const double* low, int32_t low_stride, const double* high, int32_t high_stride,
                                         int32_t param_blocks, const void* in, int64_t in_ld, int64_t in_history,
                                         void* out, int64_t out_ld, int32_t dtype,
                                         int32_t* status, void* stream)
{
    return run_band(type, rate, position, block_frames, nblocks, context, voices, low, low_stride, high, high_stride, param_blocks,
                    in, in_ld, in_history, out, out_ld, dtype, status, stream);
}
