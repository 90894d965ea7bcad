// Cold-start Butterworth biquad bank for gfx950.
// Replaces CritFilter._filter / _get_sos (reference src/signals/chain/fx.py:85-121) for LowPass and
// HighPass: per voice, per block, design butter(N=2) and run scipy's sosfilt recurrence from ZERO
// state over [<=100 context frames | block], keeping the block.  The reference re-warms every block
// (SURVEY.md §0-2), so (voice, block) pairs are independent chains: lanes = voices, and blocks go on
// the grid.  Coefficients and both state registers stay in f64 VGPRs (f32 recurrence misses the 1e-6
// bar); HBM storage is f32.
//
// Mapping: one wave = 64*VPT consecutive voices of ONE block; each lane walks the rows serially with a
// U-deep register ring of row loads in flight (each row of a wave is 64 x 4*VPT B contiguous).
// Algorithmic traffic: 4 B read + 4 B written per voice-sample; the (N+c)/N context re-read is the
// previous block's tail and is served by L2/Infinity Cache when the neighbouring wave ran recently.
#include <cstdlib>
#include <type_traits>

#include "sig_adsr.h"
#include "sig_coldstart.h"

namespace {

using namespace sig_cold;
using sig_biquad::Biquad;
using sig_biquad::design_butter2;

// ENV: multiply the stored rows by a per-voice ADSR envelope evaluated at the row's time (the
// RingMod(Filter, ADSR) pair of BASELINE config 3 without a separate pass; sig_adsr.h).  n/rate is computed for
// 64 rows at a time, one row per lane, and broadcast with v_readlane, like in the oscillator kernels.
// RES: the resonance rows of sig_biquad_coldstart_q (ResRows), or NoRes: the Butterworth design, and nothing of the other in the code
struct NoRes {};
using ResRows = BlockRows;                                // q; ptr null: unplugged = 1/sqrt2
struct EqRows { BlockRows q, gain; };                     // sig_biquad_coldstart_eq: q as above, gain (dB) likewise; null: 0 dB

template <typename T, int VPT, int kRing, bool ENV, typename RES>   // kRing = rows of loads in flight per lane
__device__ __forceinline__ void biquad_coldstart_body(
    int type, double rate, int64_t position, int N, int K, int ctx, int voices,
    const double* __restrict__ cutoff, int cs, int cutoff_blocks,
    const T* __restrict__ in, int64_t in_ld, T* __restrict__ out, int64_t out_ld,
    int voice_tiles, int* __restrict__ status, const sig_env::AdsrRows& env, [[maybe_unused]] const RES& res)
{
    using Vec = typename RowVec<T, VPT>::type;
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);       // one wave = one item
    const int vt = (int)(item % voice_tiles);
    const int64_t b = item / voice_tiles;
    if (b >= K) return;                                                        // wave-uniform
    const int v0 = (vt * SIG_WAVE + lane) * VPT;
    const bool live = v0 < voices;                                             // VPT==4 path: voices % 4 == 0
    const int vc = live ? v0 : 0;                                              // clamp: dead lanes shadow voice 0

    const int64_t p_b = position + b * N;
    const int c = (int)((p_b < (int64_t)ctx) ? p_b : (int64_t)ctx);            // BlockLoc.before: min(ctx, position)

    Biquad q[VPT];
    double z0[VPT], z1[VPT];
    if constexpr (std::is_same<RES, NoRes>::value) {
        bool ok = true;
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int v = (vc + i < voices) ? vc + i : vc;
            const double hz = cutoff[(cutoff_blocks > 1 ? b * (int64_t)(cs ? voices : 1) : 0) + (int64_t)v * cs];
            ok &= design_butter2(type, hz, rate, q[i]);
            z0[i] = 0.0; z1[i] = 0.0;
        }
        if (!ok && live && status) atomicOr(status, SIG_STATUS_BAD_CUTOFF);
    } else if constexpr (std::is_same<RES, EqRows>::value) {
        int bad = 0;                                                           // SIG_STATUS_BAD_CUTOFF | _BAD_RESONANCE | _BAD_GAIN
        auto at = [&](const BlockRows& rows, int v) {
            return rows.ptr ? rows.ptr + (rows.blocks > 1 ? b * (int64_t)(rows.stride ? voices : 1) : 0) + (int64_t)v * rows.stride : nullptr;
        };
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int v = (vc + i < voices) ? vc + i : vc;
            const double hz = cutoff[(cutoff_blocks > 1 ? b * (int64_t)(cs ? voices : 1) : 0) + (int64_t)v * cs];
            bad |= sig_biquad::design_eq2(type, hz, at(res.q, v), at(res.gain, v), rate, q[i]);
            z0[i] = 0.0; z1[i] = 0.0;
        }
        if (bad && live && status) atomicOr(status, bad);
    } else {
        int bad = 0;                                                           // SIG_STATUS_BAD_CUTOFF | SIG_STATUS_BAD_RESONANCE
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int v = (vc + i < voices) ? vc + i : vc;
            const double hz = cutoff[(cutoff_blocks > 1 ? b * (int64_t)(cs ? voices : 1) : 0) + (int64_t)v * cs];
            const double* r = res.ptr ? res.ptr + (res.blocks > 1 ? b * (int64_t)(res.stride ? voices : 1) : 0) + (int64_t)v * res.stride : nullptr;
            bad |= sig_biquad::design_resonant2(type, hz, r, rate, q[i]);
            z0[i] = 0.0; z1[i] = 0.0;
        }
        if (bad && live && status) atomicOr(status, bad);                      // (a dead lane shadows voice 0, which a live lane reports)
    }
    sig_env::Voice ev[ENV ? VPT : 1];
    double q_lane = 0.0;
    if (ENV) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) ev[i] = sig_env::load_voice(env, (vc + i < voices) ? vc + i : vc);
    }

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
                    // scipy _sosfilt, transposed direct form II, one rounding per op (contract off)
                    y[i] = q[i].b0 * x[i] + z0[i];
                    z0[i] = q[i].b1 * x[i] - q[i].a1 * y[i] + z1[i];
                    z1[i] = q[i].b2 * x[i] - q[i].a2 * y[i];
                }
            }
            if (ENV && valid) {
                if ((r & 63) == 0) q_lane = (double)(p_b - c + r + lane) / rate;                       // wave-uniform
                if (r >= c) {
                    const double t = sig_readlane_f64(q_lane, r & 63);
#pragma unroll
                    for (int i = 0; i < VPT; ++i) y[i] *= sig_env::level(ev[i], t);
                }
            }
            if (valid && r >= c && live) {
                Vec o; pack(o, y);
                *reinterpret_cast<Vec*>(dst + (int64_t)r * out_ld) = o;
            }
        }
    }
}

template <typename T, int VPT, int kRing, bool ENV>
__global__ __launch_bounds__(256) void biquad_coldstart_kernel(
    int type, double rate, int64_t position, int N, int K, int ctx, int voices,
    const double* __restrict__ cutoff, int cs, int cutoff_blocks,
    const T* __restrict__ in, int64_t in_ld, T* __restrict__ out, int64_t out_ld,
    int voice_tiles, int* __restrict__ status, sig_env::AdsrRows env)
{
    biquad_coldstart_body<T, VPT, kRing, ENV>(type, rate, position, N, K, ctx, voices, cutoff, cs, cutoff_blocks, in, in_ld, out, out_ld,
                                              voice_tiles, status, env, NoRes{});
}

// the same body with the resonant design (sig_biquad_coldstart_q): a kernel of its own, so that the one above keeps its arguments
// and its code
template <typename T, int VPT, int kRing>
__global__ __launch_bounds__(256) void biquad_coldstart_q_kernel(
    int type, double rate, int64_t position, int N, int K, int ctx, int voices,
    const double* __restrict__ cutoff, int cs, int cutoff_blocks, ResRows res,
    const T* __restrict__ in, int64_t in_ld, T* __restrict__ out, int64_t out_ld,
    int voice_tiles, int* __restrict__ status)
{
    biquad_coldstart_body<T, VPT, kRing, false>(type, rate, position, N, K, ctx, voices, cutoff, cs, cutoff_blocks, in, in_ld, out, out_ld,
                                                voice_tiles, status, sig_env::AdsrRows{}, res);
}

// ... and with the equaliser designs (sig_biquad_coldstart_eq): the recurrence of the body is the general one already
template <typename T, int VPT, int kRing>
__global__ __launch_bounds__(256) void biquad_coldstart_eq_kernel(
    int type, double rate, int64_t position, int N, int K, int ctx, int voices,
    const double* __restrict__ cutoff, int cs, int cutoff_blocks, EqRows eq,
    const T* __restrict__ in, int64_t in_ld, T* __restrict__ out, int64_t out_ld,
    int voice_tiles, int* __restrict__ status)
{
    biquad_coldstart_body<T, VPT, kRing, false>(type, rate, position, N, K, ctx, voices, cutoff, cs, cutoff_blocks, in, in_ld, out, out_ld,
                                                voice_tiles, status, sig_env::AdsrRows{}, eq);
}

// ---------------------------------------------------------------------------------------------------
// Span walker: one lane owns VPT voices x `span` CONSECUTIVE blocks and reads every input row ONCE.
// The plain kernel re-reads each block's 100 context rows (they are the previous block's tail): measured
// with rocprofv3 FETCH_SIZE the read side is 1.39x the algorithmic bytes at N=256 and none of it is
// absorbed by L2 / Infinity Cache.  Here block m's warm-up (rows [(m+1)N-ctx, (m+1)N) of block m's main
// region) runs as a SECOND chain on the same loaded row while block m's own chain is still producing
// output; at the block boundary the warm chain becomes the output chain.  Arithmetic per chain is
// unchanged (same zero start, same rows, same order), so results are bit-identical to the plain kernel.
// Needs N > ctx (at most two live chains) and one cutoff row for all blocks.
template <typename T, int VPT, int kRing, bool ENV>
__global__ __launch_bounds__(256) void biquad_walk_kernel(
    int type, double rate, int64_t position, int N, int K, int ctx, int voices, int span,
    const double* __restrict__ cutoff, int cs,
    const T* __restrict__ in, int64_t in_ld, T* __restrict__ out, int64_t out_ld,
    int voice_tiles, int* __restrict__ status, sig_env::AdsrRows env)
{
    using Vec = typename RowVec<T, VPT>::type;
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int vt = (int)(item % voice_tiles);
    const int64_t b0 = (item / voice_tiles) * span;                           // first block of this lane's span
    if (b0 >= K) return;                                                       // wave-uniform
    const int nb = (K - b0 < span) ? (int)(K - b0) : span;                     // blocks in this span
    const int v0 = (vt * SIG_WAVE + lane) * VPT;
    const bool live = v0 < voices;
    const int vc = live ? v0 : 0;

    const int64_t p0 = position + b0 * N;
    const int c0 = (int)((p0 < (int64_t)ctx) ? p0 : (int64_t)ctx);             // only the span's first block can be short

    Biquad q[VPT];
    double a0[VPT], a1[VPT], w0[VPT], w1[VPT];                                  // output chain / warm-up chain states
    bool ok = true;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int v = (vc + i < voices) ? vc + i : vc;
        ok &= design_butter2(type, cutoff[(int64_t)v * cs], rate, q[i]);
        a0[i] = a1[i] = w0[i] = w1[i] = 0.0;
    }
    if (!ok && live && status) atomicOr(status, SIG_STATUS_BAD_CUTOFF);
    sig_env::Voice ev[ENV ? VPT : 1];
    double q_lane = 0.0;
    if (ENV) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) ev[i] = sig_env::load_voice(env, (vc + i < voices) ? vc + i : vc);
    }

    const int total = c0 + nb * N;
    const T* src = in + (b0 * N - c0) * in_ld + vc;
    T* dst = out + (b0 * N - c0) * out_ld + vc;

    Vec ring[kRing];
#pragma unroll
    for (int u = 0; u < kRing; ++u) {
        const int r = (u < total) ? u : total - 1;
        ring[u] = *reinterpret_cast<const Vec*>(src + (int64_t)r * in_ld);
    }

    int in_block = -c0;                 // row index inside the current block; negative = the first block's own warm-up
    int blocks_left = nb;
    for (int r0 = 0; r0 < total; r0 += kRing) {
#pragma unroll
        for (int u = 0; u < kRing; ++u) {
            const int r = r0 + u;
            const bool valid = r < total;                                      // wave-uniform; tail rows are no-ops
            double x[VPT], y[VPT];
            unpack(ring[u], x);
            const int rn = (r + kRing < total) ? r + kRing : total - 1;
            ring[u] = *reinterpret_cast<const Vec*>(src + (int64_t)rn * in_ld);
            const bool warm = valid && (blocks_left > 1) && (in_block >= N - ctx);   // next block's context rows
            if (valid) {
#pragma unroll
                for (int i = 0; i < VPT; ++i) {
                    y[i] = q[i].b0 * x[i] + a0[i];
                    a0[i] = q[i].b1 * x[i] - q[i].a1 * y[i] + a1[i];
                    a1[i] = q[i].b2 * x[i] - q[i].a2 * y[i];
                }
            }
            if (warm) {
#pragma unroll
                for (int i = 0; i < VPT; ++i) {
                    const double yw = q[i].b0 * x[i] + w0[i];
                    w0[i] = q[i].b1 * x[i] - q[i].a1 * yw + w1[i];
                    w1[i] = q[i].b2 * x[i] - q[i].a2 * yw;
                }
            }
            if (ENV && valid) {
                if ((r & 63) == 0) q_lane = (double)(p0 - c0 + r + lane) / rate;                       // wave-uniform
                if (in_block >= 0) {
                    const double t = sig_readlane_f64(q_lane, r & 63);
#pragma unroll
                    for (int i = 0; i < VPT; ++i) y[i] *= sig_env::level(ev[i], t);
                }
            }
            if (valid && in_block >= 0 && live) {
                Vec o; pack(o, y);
                *reinterpret_cast<Vec*>(dst + (int64_t)r * out_ld) = o;
            }
            in_block += valid ? 1 : 0;
            if (in_block == N) {                                                // block boundary: warm chain takes over
                in_block = 0;
                --blocks_left;
#pragma unroll
                for (int i = 0; i < VPT; ++i) { a0[i] = w0[i]; a1[i] = w1[i]; w0[i] = 0.0; w1[i] = 0.0; }
            }
        }
    }
}

// ---- host

// one launch in the entries' terms; env, res, eq: at most one, null otherwise
template <typename T>
struct Launch {
    int type; int32_t rate; int64_t position; int32_t N, K, ctx, voices;
    BlockRows cutoff;
    const T* in; int64_t in_ld; T* out; int64_t out_ld;
    int32_t* status; hipStream_t stream;
    const sig_env::AdsrRows* env; const ResRows* res; const EqRows* eq;
};

template <int VPT, int RING> struct Shape { static constexpr int vpt = VPT, ring = RING; };

// f(Shape<vpt, ring>) for a pair among PAIRS (each written vpt * 100 + ring, like the tuning hooks), hipErrorInvalidValue
// without a call for any other
template <int... PAIRS, typename F>
int dispatch_shape(int vpt, int ring, F&& f)
{
    int err = (int)hipErrorInvalidValue;
    auto one = [&](auto shape) { if (vpt == shape.vpt && ring == shape.ring) err = f(shape); };
    (one(Shape<PAIRS / 100, PAIRS % 100>{}), ...);
    return err;
}

static int env_int(const char* name, int otherwise) { const char* e = getenv(name); return e ? atoi(e) : otherwise; }

template <typename T, bool ENV>
int launch_biquad(const Launch<T>& a)
{
    const int K = a.K, voices = a.voices;
    const sig_env::AdsrRows env = ENV ? *a.env : sig_env::AdsrRows{};
    auto ok = [&](int vpt) { return vec_ok(vpt, sizeof(T), voices, {a.in_ld, a.out_ld}, {a.in, a.out}); };
    // tuning hook: SIG_BIQUAD_VARIANT=<vpt><ring> e.g. "416" = 4 voices/lane, 16-row ring
    static const int variant = env_int("SIG_BIQUAD_VARIANT", 0);
    // span walker: every row read once (see biquad_walk_kernel).  Keep >= ~1024 waves on the chip.
    {
        static const int walk_env = env_int("SIG_BIQUAD_WALK", -1);
        static const int walk_variant = env_int("SIG_WALK_VARIANT", 0);
        int wvpt = walk_variant ? walk_variant / 100 : 4;                     // tuning: <vpt><ring>, e.g. 216
        const int wring = walk_variant ? walk_variant % 100 : 16;
        while (wvpt > 1 && !ok(wvpt)) wvpt >>= 1;
        const int tiles = sig_voice_tiles(voices, wvpt);
        // measured on C2 at K=1024 (vpt x ring x span sweep): 4 voices/lane, 16 rows in flight, span 4 is the best
        // point (5.0 TB/s algorithmic); longer spans starve the chip of waves, shorter ones re-read more context
        int span = (int)(((int64_t)tiles * K) / 1024);
        if (span > 4) span = 4;
        if (walk_env >= 0) span = walk_env;                                    // tuning: 0/1 disables
        if (span >= 2 && a.N > a.ctx && a.cutoff.blocks == 1 && variant == 0 && !a.res && !a.eq) {   // (the resonant and the equaliser entries: the plain kernel only)
            unsigned nwg;
            if (!sig_workgroups(sig_span_waves(tiles, K, span), nwg)) return (int)hipErrorInvalidValue;
            return dispatch_shape<116, 132, 216, 232, 408, 416, 432>(wvpt, wring, [&](auto s) {
                biquad_walk_kernel<T, s.vpt, s.ring, ENV><<<nwg, 256, 0, a.stream>>>(
                    a.type, (double)a.rate, a.position, a.N, K, a.ctx, voices, span, a.cutoff.ptr, a.cutoff.stride,
                    a.in, a.in_ld, a.out, a.out_ld, tiles, a.status, env);
                return sig_launch_status();
            });
        }
    }
    int vpt = variant ? variant / 100 : 4;
    int ring = variant ? variant % 100 : 8;
    if (!variant) {
        // lanes walk rows serially: with few (voice tile, block) items prefer more, narrower waves and a deeper
        // ring (big blocks x few blocks, e.g. N=1024 K=64, would otherwise leave 3/4 of the SIMDs idle)
        while (vpt > 1 && sig_span_waves(sig_voice_tiles(voices, vpt), K, 1) < 2048) vpt >>= 1;
        ring = (vpt == 4) ? 8 : 16;
    }
    while (vpt > 1 && !ok(vpt)) vpt >>= 1;
    if (vpt == 1 && !variant) ring = 16;
    const int voice_tiles = sig_voice_tiles(voices, vpt);
    unsigned nwg;
    if (!sig_workgroups(sig_span_waves(voice_tiles, K, 1), nwg)) return (int)hipErrorInvalidValue;
    return dispatch_shape<108, 116, 132, 208, 216, 232, 408, 416, 432>(vpt, ring, [&](auto s) {
        constexpr int V = decltype(s)::vpt, R = decltype(s)::ring;
        const double rate = a.rate;
        const BlockRows& c = a.cutoff;
        if (!ENV && a.eq) {
            if constexpr (!ENV)
                biquad_coldstart_eq_kernel<T, V, R><<<nwg, 256, 0, a.stream>>>(
                    a.type, rate, a.position, a.N, K, a.ctx, voices, c.ptr, c.stride, c.blocks, *a.eq, a.in, a.in_ld, a.out, a.out_ld, voice_tiles, a.status);
        } else if (!ENV && a.res) {
            if constexpr (!ENV)
                biquad_coldstart_q_kernel<T, V, R><<<nwg, 256, 0, a.stream>>>(
                    a.type, rate, a.position, a.N, K, a.ctx, voices, c.ptr, c.stride, c.blocks, *a.res, a.in, a.in_ld, a.out, a.out_ld, voice_tiles, a.status);
        } else {
            biquad_coldstart_kernel<T, V, R, ENV><<<nwg, 256, 0, a.stream>>>(
                a.type, rate, a.position, a.N, K, a.ctx, voices, c.ptr, c.stride, c.blocks, a.in, a.in_ld, a.out, a.out_ld, voice_tiles, a.status, env);
        }
        return sig_launch_status();
    });
}

int run_biquad(int type, int32_t rate, int64_t position, int32_t block_frames, int32_t nblocks, int32_t context,
               int32_t voices, const double* cutoff, int32_t cutoff_stride, int32_t cutoff_blocks,
               const void* in, int64_t in_ld, int64_t in_history, void* out, int64_t out_ld, int32_t dtype,
               int32_t* status, void* stream, const sig_env::AdsrRows* env, const ResRows* res = nullptr, const EqRows* eq = nullptr)
{
    bool empty;
    SIG_CHECK_ARG(eq ? (type >= SIG_FILT_EQ_BANDPASS && type <= SIG_FILT_EQ_HIGHSHELF) : (type == SIG_FILT_LOWPASS || type == SIG_FILT_HIGHPASS));
    SIG_CHECK_ARG(!res || (!env && rows_ok(*res, nblocks, false)));
    SIG_CHECK_ARG(!eq || (!env && !res && rows_ok(eq->q, nblocks, false) && rows_ok(eq->gain, nblocks, false)));
    SIG_CHECK_ARG(window_ok(rate, position, block_frames, nblocks, context, voices, in, in_ld, in_history, out, empty));
    SIG_CHECK_ARG(rows_ok({cutoff, cutoff_stride, cutoff_blocks}, nblocks, true) && out_ld >= voices);
    if (empty) return 0;
    return dispatch_dtype(dtype, in, out, [&](auto* x, auto* y) {
        using T = std::remove_pointer_t<decltype(y)>;
        const Launch<T> a{type, rate, position, block_frames, nblocks, context, voices, {cutoff, cutoff_stride, cutoff_blocks},
                          x, in_ld, y, out_ld, status, static_cast<hipStream_t>(stream), env, res, eq};
        if (!env) return launch_biquad<T, false>(a);
        if constexpr (std::is_same<T, float>::value) return launch_biquad<float, true>(a);      // the envelope epilogue: float32 only
        return (int)hipErrorInvalidValue;
    });
}

}  // namespace

extern "C" int sig_biquad_coldstart(int type, int32_t rate, int64_t position,
                                    int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                    const double* cutoff, int32_t cutoff_stride, int32_t cutoff_blocks,
                                    const void* in, int64_t in_ld, int64_t in_history,
                                    void* out, int64_t out_ld, int32_t dtype,
                                    int32_t* status, void* stream)
{
    return run_biquad(type, rate, position, block_frames, nblocks, context, voices, cutoff, cutoff_stride, cutoff_blocks,
                      in, in_ld, in_history, out, out_ld, dtype, status, stream, nullptr);
}

extern "C" int sig_biquad_coldstart_env(int type, int32_t rate, int64_t position,
                                        int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                        const double* cutoff, int32_t cutoff_stride, int32_t cutoff_blocks,
                                        const double* const* adsr_params, const int32_t* adsr_strides,
                                        const float* in, int64_t in_ld, int64_t in_history,
                                        float* out, int64_t out_ld, int32_t* status, void* stream)
{
    sig_env::AdsrRows env;
    SIG_CHECK_ARG(sig_env::load_rows(adsr_params, adsr_strides, env));
    return run_biquad(type, rate, position, block_frames, nblocks, context, voices, cutoff, cutoff_stride, cutoff_blocks,
                      in, in_ld, in_history, out, out_ld, SIG_F32, status, stream, &env);
}

extern "C" int sig_biquad_coldstart_q(int type, int32_t rate, int64_t position,
                                      int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                      const double* cutoff, int32_t cutoff_stride, int32_t cutoff_blocks,
                                      const double* resonance, int32_t resonance_stride, int32_t resonance_blocks,
                                      const void* in, int64_t in_ld, int64_t in_history,
                                      void* out, int64_t out_ld, int32_t dtype,
                                      int32_t* status, void* stream)
{
    const ResRows res{resonance, resonance_stride, resonance_blocks};          // (a null row: unplugged, its stride and count still checked)
    return run_biquad(type, rate, position, block_frames, nblocks, context, voices, cutoff, cutoff_stride, cutoff_blocks,
                      in, in_ld, in_history, out, out_ld, dtype, status, stream, nullptr, &res);
}

extern "C" int sig_biquad_coldstart_eq(int type, int32_t rate, int64_t position,
                                       int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                       const double* cutoff, int32_t cutoff_stride, int32_t cutoff_blocks,
                                       const double* resonance, int32_t resonance_stride, int32_t resonance_blocks,
                                       const double* gain, int32_t gain_stride, int32_t gain_blocks,
                                       const void* in, int64_t in_ld, int64_t in_history,
                                       void* out, int64_t out_ld, int32_t dtype,
                                       int32_t* status, void* stream)
{
    const EqRows eq{{resonance, resonance_stride, resonance_blocks}, {gain, gain_stride, gain_blocks}};     // (null rows: unplugged, still checked)
    return run_biquad(type, rate, position, block_frames, nblocks, context, voices, cutoff, cutoff_stride, cutoff_blocks,
                      in, in_ld, in_history, out, out_ld, dtype, status, stream, nullptr, nullptr, &eq);
}
