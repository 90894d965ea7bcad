// Cold-start 4-pole ladder filter bank for gfx950 (chain/ext.py Ladder; build-defined, the reference has no counterpart): four
// trapezoidal ("TPT") one-pole low-passes in series, the resonance k fed back around all four with the zero-delay loop solved in
// closed form, and a tanh saturator of drive d at the loop's summing point.  Per voice and block, in float64, from ZERO state over
// [<= 100 context rows | block] like every filter here (biquad.hip), every operation rounded once in this order (contraction off):
//   wn = clip(cutoff / (rate / 2), 0, 1);  g = tan(pi wn / 2);  G = g / (1 + g);  H = 1 - G
//   k  = clip(resonance, 0, 4);  d = max(drive, 0);  c = 1 / (1 + k ((G G) (G G)))
//   per row:  S = H (((s1 G + s2) G + s3) G + s4);  u = (x - k S) c;  if d > 0: u = tanh(d u) / d
//             four times:  v = (u - s_j) G;  y_j = v + s_j;  s_j = y_j + v;  u = y_j
//             out = y_poles
// (tests/ladder_reference.py restates it in numpy; the kernel multiplies by a rounded 1 / d where that divides.)
//
// Mapping: biquad.hip's.  One wave = 64 * VPT consecutive voices of ONE block, lanes walk the rows serially with a ring of row
// loads in flight; (block, voice) pairs are independent chains, so blocks go on the grid.  What differs is the row loop: 26 f64
// operations per voice (7 for S, 3 for the solve, 4 per stage), 22 of them ONE dependent chain, where the biquad has 9 and a recurrence
// of 4, and with drive a tanh in the middle of the chain.  ILP comes from the VPT independent chains of a lane and from the waves of
// a SIMD.  tan and the two divides of the design run once per (block, voice), outside the row loop.
// DRIVE false (the host saw a null drive row): no tanh anywhere in the kernel's code.  DRIVE true: `d > 0` per lane and voice.
#include <type_traits>

#include "sig_coldstart.h"

namespace {

using namespace sig_cold;
using sig_biquad::kPi;

template <typename T, int VPT, int kRing, bool DRIVE>          // kRing = rows of loads in flight per lane
__global__ __launch_bounds__(256) void ladder_coldstart_kernel(
    double rate, int64_t position, int N, int K, int ctx, int voices,
    BlockRows cutoff, BlockRows resonance, BlockRows drive, int poles,
    const T* __restrict__ in, int64_t in_ld, T* __restrict__ out, int64_t out_ld,
    int voice_tiles, int* __restrict__ status)
{
    using Vec = typename RowVec<T, VPT>::type;
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);       // one wave = one item
    const int vt = (int)(item % voice_tiles);
    const int64_t b = item / voice_tiles;
    if (b >= K) return;                                                        // wave-uniform
    const int v0 = (vt * SIG_WAVE + lane) * VPT;
    const bool live = v0 < voices;                                             // VPT > 1: voices % VPT == 0
    const int vc = live ? v0 : 0;                                              // clamp: dead lanes shadow voice 0

    const int64_t p_b = position + b * N;
    const int c = (int)((p_b < (int64_t)ctx) ? p_b : (int64_t)ctx);            // BlockLoc.before: min(ctx, position)

    // ---- the design, once per (block, voice)
    auto at = [&](const BlockRows& rows, int v) {
        return rows.ptr[(rows.blocks > 1 ? b * (int64_t)(rows.stride ? voices : 1) : 0) + (int64_t)v * rows.stride];
    };
    double G[VPT], H[VPT], kk[VPT], cc[VPT];
    [[maybe_unused]] double dd[VPT], inv_d[VPT];
    double s1[VPT], s2[VPT], s3[VPT], s4[VPT];
    int bad = 0;                                                               // SIG_STATUS_BAD_CUTOFF | SIG_STATUS_BAD_RESONANCE
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int v = (vc + i < voices) ? vc + i : vc;
        double wn = at(cutoff, v) / (rate * 0.5);
        wn = (wn < 0.0) ? 0.0 : ((wn > 1.0) ? 1.0 : wn);                       // clip(0, 1); NaN stays NaN
        int refused = !(wn > 0.0 && wn < 1.0) ? SIG_STATUS_BAD_CUTOFF : 0;
        double k = 0.0;                                                        // null: unplugged, no feedback
        if (resonance.ptr) {
            k = at(resonance, v);
            if (!(fabs(k) < __builtin_inf())) refused |= SIG_STATUS_BAD_RESONANCE;      // NaN, +-inf
            k = (k < 0.0) ? 0.0 : ((k > 4.0) ? 4.0 : k);
        }
        bool silent = false;                                                   // a drive that is NaN or +inf: NaN rows, no status bit
        if constexpr (DRIVE) {
            double d = at(drive, v);
            silent = !(d < __builtin_inf());
            d = (d > 0.0) ? d : 0.0;                                           // max(drive, 0): -inf and negatives are 0
            dd[i] = d;
            inv_d[i] = 1.0 / d;                                                // (inf at d = 0: never used there)
        }
        const double g = tan(kPi * wn / 2.0);
        G[i] = g / (1.0 + g);
        H[i] = 1.0 - G[i];
        const double G2 = G[i] * G[i];
        cc[i] = 1.0 / (1.0 + k * (G2 * G2));
        kk[i] = k;
        if (refused || silent) G[i] = __builtin_nan("");                       // every row of the voice follows
        bad |= refused;
        s1[i] = s2[i] = s3[i] = s4[i] = 0.0;
    }
    if (bad && live && status) atomicOr(status, bad);                          // (a dead lane shadows voice 0, which a live lane reports)

    const int total = c + N;
    const T* src = in + (b * N - c) * in_ld + vc;        // first context row of this block
    T* dst = out + (b * N - c) * out_ld + vc;            // aligned with src; rows < c are never stored

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
            const bool valid = r < total;                                      // wave-uniform; tail rows are no-ops
            double x[VPT], y[VPT];
            unpack(ring[u], x);
            const int rn = (r + kRing < total) ? r + kRing : total - 1;        // refill this slot
            ring[u] = *reinterpret_cast<const Vec*>(src + (int64_t)rn * in_ld);
            if (valid) {
#pragma unroll
                for (int i = 0; i < VPT; ++i) {
                    const double S = H[i] * (((s1[i] * G[i] + s2[i]) * G[i] + s3[i]) * G[i] + s4[i]);
                    double w = (x[i] - kk[i] * S) * cc[i];
                    if constexpr (DRIVE) {
                        if (dd[i] > 0.0) w = tanh(dd[i] * w) * inv_d[i];
                    }
                    double v = (w - s1[i]) * G[i];
                    const double y1 = v + s1[i];
                    s1[i] = y1 + v;
                    v = (y1 - s2[i]) * G[i];
                    const double y2 = v + s2[i];
                    s2[i] = y2 + v;
                    v = (y2 - s3[i]) * G[i];
                    const double y3 = v + s3[i];
                    s3[i] = y3 + v;
                    v = (y3 - s4[i]) * G[i];
                    const double y4 = v + s4[i];
                    s4[i] = y4 + v;
                    y[i] = (poles == 4) ? y4 : ((poles == 3) ? y3 : ((poles == 2) ? y2 : y1));      // uniform
                }
            }
            if (valid && r >= c && live) {
                Vec o; pack(o, y);
                *reinterpret_cast<Vec*>(dst + (int64_t)r * out_ld) = o;
            }
        }
    }
}

// ---- host

template <typename T>
struct Launch {
    int32_t rate; int64_t position; int32_t N, K, ctx, voices;
    BlockRows cutoff, resonance, drive; int32_t poles;
    const T* in; int64_t in_ld; T* out; int64_t out_ld;
    int32_t* status; hipStream_t stream;
};

template <typename T, int VPT, int kRing>
int launch_shape(const Launch<T>& a)
{
    const int voice_tiles = sig_voice_tiles(a.voices, VPT);
    unsigned nwg;
    if (!sig_workgroups(sig_span_waves(voice_tiles, a.K, 1), nwg)) return (int)hipErrorInvalidValue;
    if (a.drive.ptr)
        ladder_coldstart_kernel<T, VPT, kRing, true><<<nwg, 256, 0, a.stream>>>(
            (double)a.rate, a.position, a.N, a.K, a.ctx, a.voices, a.cutoff, a.resonance, a.drive, a.poles, a.in, a.in_ld, a.out, a.out_ld,
            voice_tiles, a.status);
    else                                                                       // unplugged: the kernel without tanh
        ladder_coldstart_kernel<T, VPT, kRing, false><<<nwg, 256, 0, a.stream>>>(
            (double)a.rate, a.position, a.N, a.K, a.ctx, a.voices, a.cutoff, a.resonance, a.drive, a.poles, a.in, a.in_ld, a.out, a.out_ld,
            voice_tiles, a.status);
    return sig_launch_status();
}

// the widest row access every buffer allows: 4 voices per lane and 8 rows in flight, else 2 or 1 with 16
template <typename T>
int launch_ladder(const Launch<T>& a)
{
    auto ok = [&](int vpt) { return vec_ok(vpt, sizeof(T), a.voices, {a.in_ld, a.out_ld}, {a.in, a.out}); };
    if (ok(4)) return launch_shape<T, 4, 8>(a);
    if (ok(2)) return launch_shape<T, 2, 16>(a);
    return launch_shape<T, 1, 16>(a);
}

}  // namespace

extern "C" int sig_ladder_coldstart(int32_t rate, int64_t position,
                                    int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                    const double* cutoff, int32_t cutoff_stride, int32_t cutoff_blocks,
                                    const double* resonance, int32_t resonance_stride, int32_t resonance_blocks,
                                    const double* drive, int32_t drive_stride, int32_t drive_blocks,
                                    int32_t poles,
                                    const void* in, int64_t in_ld, int64_t in_history,
                                    void* out, int64_t out_ld, int32_t dtype,
                                    int32_t* status, void* stream)
{
    const BlockRows cut{cutoff, cutoff_stride, cutoff_blocks}, res{resonance, resonance_stride, resonance_blocks},
                    drv{drive, drive_stride, drive_blocks};                    // (a null row: unplugged, its stride and count still checked)
    bool empty;
    SIG_CHECK_ARG(poles >= 1 && poles <= 4);
    SIG_CHECK_ARG(window_ok(rate, position, block_frames, nblocks, context, voices, in, in_ld, in_history, out, empty));
    SIG_CHECK_ARG(rows_ok(cut, nblocks, true) && rows_ok(res, nblocks, false) && rows_ok(drv, nblocks, false) && out_ld >= voices);
    SIG_CHECK_ARG(dtype == SIG_F32 || dtype == SIG_F64);
    if (empty) return 0;
    return dispatch_dtype(dtype, in, out, [&](auto* x, auto* y) {
        using T = std::remove_pointer_t<decltype(y)>;
        const Launch<T> a{rate, position, block_frames, nblocks, context, voices, cut, res, drv, poles,
                          x, in_ld, y, out_ld, status, static_cast<hipStream_t>(stream)};
        return launch_ladder<T>(a);
    });
}
