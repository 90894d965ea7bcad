// Oscillator bank for gfx950: closed-form in absolute position, f64 phase, f32 (or f64) store.
// Replaces Osc._eval + Sine/Square/Sawtooth/Triangle._osc (reference src/signals/chain/osc.py:26-62).
//
// Mapping: one wave = 64*VEC consecutive voices x 16 consecutive rows; a 256-thread workgroup
// stacks 4 waves in time (64 rows).  Lane l owns voices [VEC*l, VEC*l+VEC) of the wave's span, so a
// row is stored as 64 x 16-B lanes = 1 KiB, fully coalesced.  The per-row quotient n/rate (an IEEE
// f64 divide, the expensive op) is computed ONCE per row by lanes 0..15 and broadcast with
// v_readlane, so the per-sample cost is mul + add + waveform.
//
// Roofline: 4 B written per voice-sample (f32), no reads beyond 2 x 8 B per voice per wave.
#include <type_traits>

#include "sig_osc.h"
#include "sig_param_rows.h"
#include "sig_table.h"

namespace {

using sig_osc::osc_wave;
using sig_rows::dispatch_out;

constexpr int kRowsPerWave = 16;
constexpr int kWavesPerWg = 4;

// Parameter rows: hertz/phase are (1|P, V|1) f64.  `rpp` (rows per parameter row) = 0: one row for the whole
// launch; otherwise output row r reads parameter row r / rpp -- rpp = block_frames for an audio-rate launch whose
// control inputs change per block (forward_at_block_rate, osc.py:28-30), rpp = 1 with `step` = block_frames for
// a block-RATE launch (one output row per block: what a control port sees for K consecutive blocks).
struct OscArgs {
    int64_t position, step; double rate; int64_t rows; int voices;
    const double* hertz; int hs; int64_t hrs; const double* phase; int ps; int64_t prs; int rpp;
};

// A thread's place in the mapping above: lane, first voice, first row.  1-D grid: consecutive workgroups cover adjacent voice
// tiles of the same rows; a workgroup owns `waves` consecutive 16-row tiles, its wave w the w-th.  (The wavetable kernel, whose
// waves walk several row groups, keeps its own form of these lines: through this helper it compiled to other registers.)
struct Tile { int lane, v0; int64_t r0; };

template <int VEC>
__device__ __forceinline__ Tile tile_of(int voice_tiles, int waves)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int vt = blockIdx.x % voice_tiles;
    const int64_t rt = blockIdx.x / voice_tiles;
    return {lane, (vt * SIG_WAVE + lane) * VEC, (rt * waves + wave) * kRowsPerWave};
}

// osc.py:32  frame_range / rate : int64 -> f64, IEEE divide, one per row: lane l holds the quotient of row r0 + (l & 15)
__device__ __forceinline__ double row_quotients(const OscArgs& a, int64_t r0, int lane)
{
    return (double)(a.position + (r0 + (lane & (kRowsPerWave - 1))) * a.step) / a.rate;
}

template <int KIND, int VEC, typename OUT>
__global__ __launch_bounds__(256) void osc_bank_kernel(OscArgs a, OUT* __restrict__ out, int64_t ld, int voice_tiles)
{
    const auto [lane, v0, r0] = tile_of<VEC>(voice_tiles, kWavesPerWg);
    if (r0 >= a.rows) return;                                      // wave-uniform

    const double q_lane = row_quotients(a, r0, lane);

    double hz[VEC], ph[VEC];
    int64_t loaded = -1;                                           // parameter row currently in registers
#pragma unroll 2                                                    // keep the loop body inside the I-cache
    for (int j = 0; j < kRowsPerWave; ++j) {
        const int64_t row = r0 + j;
        if (row >= a.rows) break;                                  // wave-uniform
        const int64_t prow = a.rpp ? row / a.rpp : 0;              // wave-uniform
        if (prow != loaded) {
            loaded = prow;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const int v = v0 + i;
                hz[i] = (v < a.voices) ? a.hertz[prow * a.hrs + (int64_t)v * a.hs] : 0.0;
                ph[i] = (v < a.voices && a.phase) ? a.phase[prow * a.prs + (int64_t)v * a.ps] : 0.0;
            }
        }
        const double q = sig_readlane_f64(q_lane, j);
        OUT y[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const double t = q * hz[i] + ph[i];                    // two roundings, like numpy
            y[i] = osc_wave<KIND, OUT>(t);
        }
        OUT* dst = out + row * ld + v0;
        if (VEC == 4) {
            if (v0 < a.voices) {                                   // voices % 4 == 0 on this path
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

// ---- phase modulation: t = (n / rate * hertz + phase) + index * mod[n, v], the modulator a frame-rate buffer.
// Same mapping as osc_bank_kernel (tile_of), plus one read per
// voice-sample: with VEC == 4 and MVEC a lane loads its four float32 modulator samples as one 16-byte access, like its store.
// Roofline: 4 B read + 4 B written per voice-sample (f32 modulator and store).
struct PmArgs {
    const double* index; int is; int64_t irs;                      // (1|P, V|1) f64 like hertz / phase; NULL: unplugged = 0
    const void* mod; int64_t mld; int mcs;                         // (rows|1, V|1): mld == 0 one row, mcs == 0 one column; NULL: 0
};

template <int KIND, int VEC, typename OUT, typename MOD, bool MVEC>
__global__ __launch_bounds__(256) void osc_bank_pm_kernel(OscArgs a, PmArgs m, OUT* __restrict__ out, int64_t ld, int voice_tiles)
{
    const auto [lane, v0, r0] = tile_of<VEC>(voice_tiles, kWavesPerWg);
    if (r0 >= a.rows) return;                                      // wave-uniform

    const double q_lane = row_quotients(a, r0, lane);
    const MOD* __restrict__ mod = static_cast<const MOD*>(m.mod);

    double hz[VEC], ph[VEC], ix[VEC];
    int64_t loaded = -1;
#pragma unroll 2
    for (int j = 0; j < kRowsPerWave; ++j) {
        const int64_t row = r0 + j;
        if (row >= a.rows) break;                                  // wave-uniform
        const int64_t prow = a.rpp ? row / a.rpp : 0;              // wave-uniform
        if (prow != loaded) {
            loaded = prow;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const int v = v0 + i;
                hz[i] = (v < a.voices) ? a.hertz[prow * a.hrs + (int64_t)v * a.hs] : 0.0;
                ph[i] = (v < a.voices && a.phase) ? a.phase[prow * a.prs + (int64_t)v * a.ps] : 0.0;
                ix[i] = (v < a.voices && m.index) ? m.index[prow * m.irs + (int64_t)v * m.is] : 0.0;
            }
        }
        double x[VEC];
        if (MVEC) {                                                // float32 (rows, V) modulator, 16-byte aligned rows, voices % 4 == 0
            float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
            if (v0 < a.voices) w = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(m.mod) + row * m.mld + v0);
            const float f[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int i = 0; i < VEC; ++i) x[i] = (double)f[i & 3];
        } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                x[i] = (mod && v0 + i < a.voices) ? (double)mod[row * m.mld + (int64_t)(v0 + i) * m.mcs] : 0.0;
        }
        const double q = sig_readlane_f64(q_lane, j);
        OUT y[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const double t = (q * hz[i] + ph[i]) + ix[i] * x[i];   // every operation rounded, in numpy's order
            y[i] = osc_wave<KIND, OUT>(t);
        }
        OUT* dst = out + row * ld + v0;
        if (VEC == 4) {
            if (v0 < a.voices) {                                   // voices % 4 == 0 on this path
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

// ---- wavetable: out = lerp of a (T, W) float32 table (W single-cycle waveforms of T points, T a power of two) at
// m = np.mod(n / rate * hertz + phase, 1), column w = clip(floor(select), 0, W - 1) per voice (chain/ext.py Wavetable).
// A 512-thread workgroup stages the whole table in LDS once -- column-major, T + 1 floats per column, the guard entry
// tab[w][T] = tab[w][0] (sig_table.h, shared with the waveshaper) -- and then walks `groups` 16-row groups per wave of its 64 * VEC voices, so the staging (<= 64 KiB
// read from L2) is amortised over up to 1 MiB of stores.  The guard makes the two lerp operands ONE paired read at a single
// address (i & (T - 1), + 1: the last segment wraps without a second mask, and m == 1.0 lands on entry 0 with f == 0), and the
// odd column stride T + 1 keeps equal indices of different columns on different banks.  Lanes, rows and stores as in
// osc_bank_kernel.  64 KiB of table: two workgroups per CU = 16 waves, four per SIMD.
// Arithmetic: the definition's, every operation rounded once in its order (t - floor(t) is np.mod(t, 1), sig_npmod_pow2;
// m * T, floor, u - i are exact), so the float64 value in front of the store has numpy's bits.
// Roofline: 4 B written per voice-sample (f32).
constexpr int kTableWaves = 8;

struct TableArgs {
    const float* table; int T, W;                                  // (T, W) row-major, device memory
    const double* select; int ss; int64_t srs;                     // (1|P, V|1) f64 like hertz / phase; NULL: unplugged = column 0
    int groups;                                                    // 16-row groups per wave
};

template <int VEC, typename OUT>
__global__ __launch_bounds__(64 * kTableWaves) void osc_bank_table_kernel(OscArgs a, TableArgs tb, OUT* __restrict__ out, int64_t ld, int voice_tiles)
{
    extern __shared__ float tab[];                                 // [W][T + 1], sig_table.h
    const int T = tb.T, W = tb.W, S = T + 1;
    sig_table::stage<64 * kTableWaves>(tab, tb.table, T, W);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int vt = blockIdx.x % voice_tiles;
    const int64_t rt = blockIdx.x / voice_tiles;
    const int v0 = (vt * SIG_WAVE + lane) * VEC;
    const double scale = (double)T;
    const int mask = T - 1;

    double hz[VEC], ph[VEC];
    int col[VEC];                                                  // the voice's column: its first float in `tab`
    int64_t loaded = -1;                                           // parameter row currently in registers
    for (int g = 0; g < tb.groups; ++g) {
        const int64_t r0 = ((rt * tb.groups + g) * kTableWaves + wave) * kRowsPerWave;
        if (r0 >= a.rows) break;                                   // wave-uniform
        const double q_lane = row_quotients(a, r0, lane);
        for (int j = 0; j < kRowsPerWave; ++j) {
            const int64_t row = r0 + j;
            if (row >= a.rows) break;                              // wave-uniform
            const int64_t prow = a.rpp ? row / a.rpp : 0;          // wave-uniform
            if (prow != loaded) {
                loaded = prow;
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const int v = v0 + i;
                    hz[i] = (v < a.voices) ? a.hertz[prow * a.hrs + (int64_t)v * a.hs] : 0.0;
                    ph[i] = (v < a.voices && a.phase) ? a.phase[prow * a.prs + (int64_t)v * a.ps] : 0.0;
                    const double s = (v < a.voices && tb.select) ? floor(tb.select[prow * tb.srs + (int64_t)v * tb.ss]) : 0.0;
                    const int w = (s >= 1.0) ? ((s >= (double)(W - 1)) ? W - 1 : (int)s) : 0;     // clip; NaN -> 0
                    col[i] = w * S;
                }
            }
            const double q = sig_readlane_f64(q_lane, j);
            OUT y[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const double t = q * hz[i] + ph[i];                // two roundings, like numpy
                const double u = sig_npmod_pow2<1>(t) * scale;     // in [0, T]
                const double fl = floor(u);
                const double f = u - fl;
                const int at = col[i] + ((int)fl & mask);          // <= col + T - 1, so at + 1 reaches the guard at most
                const double lo = (double)tab[at], hi = (double)tab[at + 1];
                y[i] = (OUT)(lo + f * (hi - lo));
            }
            OUT* dst = out + row * ld + v0;
            if (VEC == 4) {
                if (v0 < a.voices) {                               // voices % 4 == 0 on this path
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

// ---- additive: out = sum over h = 1 .. k of c_h sin(2 pi h m), m = np.mod(n / rate * hertz + phase, 1), the amplitudes a (H, W) float32
// table -- row h - 1 the harmonic h, column w = clip(floor(select), 0, W - 1) per voice -- and k, g the band limit per voice and
// parameter row (chain/ext.py Additive): nf = (rate / 2) / |hertz|, k = clip(ceil(nf) - 1, 0, H), g = min(1, nf - k) on partial k alone.
// The wavetable kernel's workgroup, rows and stores: 512 threads stage the table in LDS once (column-major, sig_table.h's
// stage_columns; the column stride H | 1 where that fits 64 KiB, so that equal harmonics of different columns fall on different
// banks, else H) and each wave walks `groups` 16-row groups of its 64 * VEC voices.
// Hoisted, once per voice and parameter row: the IEEE divide for nf, k, the column's first float, and the wave's largest k, which
// bounds the partial loop (a butterfly over the lanes; the loop counter is then scalar).  The weight of partial h is
//   clamp(nf - h, 0, 1)  ==  1 for h < k,  g for h == k,  0 for h > k
// in the definition's own bits (nf - h >= 1 below k and <= 0 above it, since k >= nf - 1; at h == k the subtraction IS the
// definition's; a k clipped to H leaves h <= H only): lanes with a smaller k than the wave's are predicated off by a zero weight,
// and no lane compares h with its k.  k == 0 is answered 0.0 and a NaN hertz NaN by a select behind the loop (0 * NaN is no zero).
// Per sample: t and m as every oscillator here (two roundings, np.mod), ONE sine / cosine pair of 2 pi m (sig_osc::cycle_sincos,
// < 3e-16 each), then the plane rotation
//   s_{h+1} = s_h C + c_h S,   c_{h+1} = c_h C - s_h S,   acc += c_h_weighted * s_h          (S, C = sin, cos of 2 pi m; 2 mul + 3 fma)
// Why this holds 1e-6 * max(1, sum |a|) everywhere, the 0.01 Hz voice included: a rotation by a matrix whose entries are off by
// < 3e-16 keeps |(s, c)| within 1 + 5e-16 per step and turns the angle by theta (1 + O(1e-16)) + O(3e-16), so after h steps s_h is
// within ~ h * 1e-15 of sin(h theta) -- linear in h, < 7e-14 at h = 64 -- whatever theta is; nothing divides by theta or by
// 2 - 2 cos(theta), which is where the three-term recurrence s_{h+1} = 2 cos(theta) s_h - s_{h-1} loses eps h^2 / theta.  The sum
// adds < 64 roundings of terms bounded by |a_h|.  The float32 store's own rounding (6e-8 relative) is what is left.
// R consecutive rows of a voice go through the partial loop together: one LDS read, one conversion and one weight feed R chains of
// 5 dependent float64 operations each, VEC * R independent chains per lane.  Passes are cut where the parameter row changes.
// Roofline: 4 B written per voice-sample against 5 k float64 operations: float64-VALU-bound from a few partials on.
struct AddArgs {
    const float* table; int H, W, S;                               // (H, W) row-major, device memory; S: the column stride in LDS
    const double* select; int ss; int64_t srs;                     // (1|P, V|1) f64 like hertz / phase; NULL: unplugged = column 0
    int groups;                                                    // 16-row groups per wave
};

template <int VEC, int R, typename OUT>
__global__ __launch_bounds__(64 * kTableWaves) void osc_bank_additive_kernel(OscArgs a, AddArgs ad, OUT* __restrict__ out, int64_t ld, int voice_tiles)
{
    extern __shared__ float tab[];                                 // [W][S]
    const int H = ad.H, W = ad.W, S = ad.S;
    sig_table::stage_columns<64 * kTableWaves>(tab, ad.table, H, W, S);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int vt = blockIdx.x % voice_tiles;
    const int64_t rt = blockIdx.x / voice_tiles;
    const int v0 = (vt * SIG_WAVE + lane) * VEC;
    const double nyquist = 0.5 * a.rate;

    double hz[VEC], ph[VEC], nf[VEC];
    int col[VEC], kk[VEC];                                         // the voice's column: its first float in `tab`; its k
    int kmax = 0;                                                  // the wave's largest k (wave-uniform)
    int64_t loaded = -1;                                           // parameter row currently in registers
    for (int g = 0; g < ad.groups; ++g) {
        const int64_t r0 = ((rt * ad.groups + g) * kTableWaves + wave) * kRowsPerWave;
        if (r0 >= a.rows) break;                                   // wave-uniform
        const int nrows = (int)((a.rows - r0 < (int64_t)kRowsPerWave) ? a.rows - r0 : (int64_t)kRowsPerWave);
        const double q_lane = row_quotients(a, r0, lane);
        for (int j = 0; j < nrows;) {                              // passes of up to R rows of one parameter row (wave-uniform bounds)
            const int64_t row = r0 + j;
            const int64_t prow = a.rpp ? row / a.rpp : 0;
            int n = (nrows - j < R) ? nrows - j : R;
            if (a.rpp) {
                const int64_t left = (prow + 1) * a.rpp - row;
                if (left < (int64_t)n) n = (int)left;
            }
            if (prow != loaded) {
                loaded = prow;
                int top = 0;
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const int v = v0 + i;
                    const bool live = v < a.voices;
                    hz[i] = live ? a.hertz[prow * a.hrs + (int64_t)v * a.hs] : 0.0;
                    ph[i] = (live && a.phase) ? a.phase[prow * a.prs + (int64_t)v * a.ps] : 0.0;
                    col[i] = sig_table::column((live && ad.select) ? ad.select[prow * ad.srs + (int64_t)v * ad.ss] : 0.0, W) * S;
                    nf[i] = nyquist / fabs(hz[i]);                 // IEEE divide; 0 Hz: inf, every partial at weight 1
                    const double kd = ceil(nf[i]) - 1.0;
                    kk[i] = (live && kd >= 1.0) ? ((kd >= (double)H) ? H : (int)kd) : 0;      // clip; NaN -> 0 (answered NaN below)
                    top = (kk[i] > top) ? kk[i] : top;
                }
#pragma unroll
                for (int mask = 1; mask < SIG_WAVE; mask <<= 1) {
                    const int other = __shfl_xor(top, mask, SIG_WAVE);
                    top = (other > top) ? other : top;
                }
                kmax = __builtin_amdgcn_readfirstlane(top);
            }
            double s[R][VEC], c[R][VEC], S1[R][VEC], C1[R][VEC], acc[R][VEC];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double q = sig_readlane_f64(q_lane, (j + r) & (kRowsPerWave - 1));      // (rows past n: computed, not stored)
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const double t = q * hz[i] + ph[i];            // two roundings, like numpy
                    sig_osc::cycle_sincos(sig_npmod_pow2<1>(t), S1[r][i], C1[r][i]);
                    s[r][i] = S1[r][i]; c[r][i] = C1[r][i]; acc[r][i] = 0.0;
                }
            }
            for (int h = 1; h <= kmax; ++h) {                      // scalar bounds; h <= kmax <= H, so col + h - 1 stays inside the column
                const double hd = (double)h;
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const double weight = fmin(fmax(nf[i] - hd, 0.0), 1.0);
                    const double amp = (double)tab[col[i] + h - 1] * weight;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        acc[r][i] = fma(amp, s[r][i], acc[r][i]);
                        const double sn = fma(s[r][i], C1[r][i], c[r][i] * S1[r][i]);
                        c[r][i] = fma(c[r][i], C1[r][i], -(s[r][i] * S1[r][i]));
                        s[r][i] = sn;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r < n) {                                       // wave-uniform
                    OUT y[VEC];
#pragma unroll
                    for (int i = 0; i < VEC; ++i)
                        y[i] = (OUT)((hz[i] != hz[i]) ? hz[i] : ((kk[i] == 0) ? 0.0 : acc[r][i]));
                    OUT* dst = out + (row + r) * ld + v0;
                    if (VEC == 4) {
                        if (v0 < a.voices) {                       // voices % 4 == 0 on this path
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
            j += n;
        }
    }
}

// ---- unison: the mean of `copies` detuned copies of one waveform per voice (chain/ext.py UnisonOsc),
//   r_u = 1 + spread * d[u];  h_u = hertz * r_u;  q_u = phase + p[u];  t_u = n / rate * h_u + q_u;  out = (sum_u w(t_u)) / copies
// every operation rounded in that order, the sum in u ascending.  Same mapping as osc_bank_kernel (a wave = 64 * VEC voices x 16
// rows, n / rate once per row).  d[] and p[] sit in the argument block: the copy loop's trip count and both values are
// wave-uniform, so they are scalar loads and SGPRs, and the per-sample work is copies x (6 f64 operations + the waveform) on
// VEC voices' registers.  No table, no LDS, no carried state.
// Roofline: 4 B written per voice-sample (f32) against ~12 copies f64 operations: f64-VALU-bound from a few copies on.
struct UniArgs {
    const double* spread; int ss; int64_t srs;                     // (1|P, V|1) f64 like hertz / phase; NULL: unplugged = 0
    int copies; double detune[SIG_UNISON_MAX_COPIES], offset[SIG_UNISON_MAX_COPIES];
};

// one copy's sample as the f64 summand: the f32 store of Sine sums sig_osc_bank's hardware sine (so that one copy keeps its bits)
template <int KIND, typename OUT> __device__ __forceinline__ double unison_wave(double t) {
    if (KIND == SIG_OSC_SINE && sizeof(OUT) == 4) return (double)sig_osc::osc_sine_f32(t);
    return osc_wave<KIND, double>(t);
}

template <int KIND, int VEC, typename OUT>
__global__ __launch_bounds__(256) void osc_bank_unison_kernel(OscArgs a, UniArgs un, OUT* __restrict__ out, int64_t ld, int voice_tiles)
{
    const auto [lane, v0, r0] = tile_of<VEC>(voice_tiles, kWavesPerWg);
    if (r0 >= a.rows) return;                                      // wave-uniform

    const double q_lane = row_quotients(a, r0, lane);
    const int copies = un.copies;                                  // 1 .. SIG_UNISON_MAX_COPIES (checked by the entry)
    const double count = (double)copies;

    double hz[VEC], ph[VEC], sp[VEC];
    int64_t loaded = -1;
    for (int j = 0; j < kRowsPerWave; ++j) {
        const int64_t row = r0 + j;
        if (row >= a.rows) break;                                  // wave-uniform
        const int64_t prow = a.rpp ? row / a.rpp : 0;              // wave-uniform
        if (prow != loaded) {
            loaded = prow;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const int v = v0 + i;
                hz[i] = (v < a.voices) ? a.hertz[prow * a.hrs + (int64_t)v * a.hs] : 0.0;
                ph[i] = (v < a.voices && a.phase) ? a.phase[prow * a.prs + (int64_t)v * a.ps] : 0.0;
                sp[i] = (v < a.voices && un.spread) ? un.spread[prow * un.srs + (int64_t)v * un.ss] : 0.0;
            }
        }
        const double q = sig_readlane_f64(q_lane, j);
        double s[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) s[i] = 0.0;
        for (int u = 0; u < copies; ++u) {                         // wave-uniform trip count
            const double d = un.detune[u], p = un.offset[u];       // (scalar loads from the argument block)
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const double r = 1.0 + sp[i] * d;
                const double h = hz[i] * r;
                const double qu = ph[i] + p;
                const double w = unison_wave<KIND, OUT>(q * h + qu);
                s[i] = (u == 0) ? w : s[i] + w;
            }
        }
        OUT y[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) y[i] = (OUT)(s[i] / count);
        OUT* dst = out + row * ld + v0;
        if (VEC == 4) {
            if (v0 < a.voices) {                                   // voices % 4 == 0 on this path
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

// ---- band-limited unison (chain/ext.py BlepOsc): osc_bank_unison_kernel's expression and tiling with sig_osc::osc_blep as the
// waveform, which wants d = min(|h_u| / rate, 0.5) and 1 / d per copy and voice: two IEEE divides that must not be paid per sample.
// So the loops are turned round: the tile's rows are cut where the parameter row changes (once, for the whole tile, unless a block
// boundary crosses it), and for each piece the copy loop runs outside the row loop -- h, q, d and 1 / d once per copy, voice and
// piece, the 16 x VEC running sums in registers (the row loop is unrolled under a wave-uniform predicate, so they are never
// indexed at run time).  Per sample and copy: the 3 operations of t, ~12 (Sawtooth), ~24 (Square, Triangle) of the waveform, the add.
// Every lane evaluates the residual and selects; the wave-uniform skip (-DSIG_BLEP_SKIP=1) was measured against it: DESIGN.md.
// No table, no LDS, no carried state; f64-VALU-bound at every copy count.
template <int KIND, int VEC, typename OUT>
__global__ __launch_bounds__(256) void osc_bank_blep_kernel(OscArgs a, UniArgs un, OUT* __restrict__ out, int64_t ld, int voice_tiles)
{
    const auto [lane, v0, r0] = tile_of<VEC>(voice_tiles, kWavesPerWg);
    if (r0 >= a.rows) return;                                      // wave-uniform
    const int nrows = (int)((a.rows - r0 < (int64_t)kRowsPerWave) ? a.rows - r0 : (int64_t)kRowsPerWave);

    const double q_lane = row_quotients(a, r0, lane);
    const int copies = un.copies;                                  // 1 .. SIG_UNISON_MAX_COPIES (checked by the entry)

    double s[kRowsPerWave][VEC];
#pragma unroll
    for (int j = 0; j < kRowsPerWave; ++j)
#pragma unroll
        for (int i = 0; i < VEC; ++i) s[j][i] = 0.0;
    for (int j0 = 0; j0 < nrows;) {                                // pieces of one parameter row each (wave-uniform bounds)
        const int64_t prow = a.rpp ? (r0 + j0) / a.rpp : 0;
        const int64_t left = a.rpp ? (prow + 1) * a.rpp - r0 : (int64_t)nrows;
        const int j1 = (left < (int64_t)nrows) ? (int)left : nrows;
        double hz[VEC], ph[VEC], sp[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const int v = v0 + i;
            hz[i] = (v < a.voices) ? a.hertz[prow * a.hrs + (int64_t)v * a.hs] : 0.0;
            ph[i] = (v < a.voices && a.phase) ? a.phase[prow * a.prs + (int64_t)v * a.ps] : 0.0;
            sp[i] = (v < a.voices && un.spread) ? un.spread[prow * un.srs + (int64_t)v * un.ss] : 0.0;
        }
        for (int u = 0; u < copies; ++u) {                         // wave-uniform trip count
            const double du = un.detune[u], pu = un.offset[u];     // (scalar loads from the argument block)
            double h[VEC], qu[VEC], d[VEC], inv_d[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const double r = 1.0 + sp[i] * du;
                h[i] = hz[i] * r;
                qu[i] = ph[i] + pu;
                sig_osc::blep_increment(h[i], a.rate, d[i], inv_d[i]);
            }
#pragma unroll
            for (int j = 0; j < kRowsPerWave; ++j) {
                if (j >= j0 && j < j1) {                           // wave-uniform
                    const double q = sig_readlane_f64(q_lane, j);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        const double w = sig_osc::osc_blep<KIND>(q * h[i] + qu[i], d[i], inv_d[i]);
                        s[j][i] = (u == 0) ? w : s[j][i] + w;
                    }
                }
            }
        }
        j0 = j1;
    }
    const double count = (double)copies;
#pragma unroll
    for (int j = 0; j < kRowsPerWave; ++j) {
        if (j < nrows) {                                           // wave-uniform: row r0 + j < a.rows
            OUT y[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) y[i] = (OUT)(s[j][i] / count);
            OUT* dst = out + (r0 + j) * ld + v0;
            if (VEC == 4) {
                if (v0 < a.voices) {                               // voices % 4 == 0 on this path
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

// ---- hard sync (chain/ext.py SyncOsc): osc_bank_blep_kernel's tiling, pieces and loops with sig_osc::osc_sync as the waveform and
// one more parameter row, the ratio.  Block-invariant and hoisted like d and 1 / d: per voice and piece R, g and the reset's weight
// (sig_osc::sync_ratio), per copy, voice and piece ds and 1 / ds -- a third IEEE divide there, none per sample.  Every lane evaluates every
// residual and selects.  No table, no LDS, no carried state.
struct SyncArgs { const double* ratio; int rs; int64_t rrs; };      // (1|P, V|1) f64 like hertz / phase; NULL: unplugged = 0 (R = 1)

template <int KIND, int VEC, typename OUT>
__global__ __launch_bounds__(256) void osc_bank_sync_kernel(OscArgs a, UniArgs un, SyncArgs sy, OUT* __restrict__ out, int64_t ld, int voice_tiles)
{
    const auto [lane, v0, r0] = tile_of<VEC>(voice_tiles, kWavesPerWg);
    if (r0 >= a.rows) return;                                      // wave-uniform
    const int nrows = (int)((a.rows - r0 < (int64_t)kRowsPerWave) ? a.rows - r0 : (int64_t)kRowsPerWave);

    const double q_lane = row_quotients(a, r0, lane);
    const int copies = un.copies;                                  // 1 .. SIG_UNISON_MAX_COPIES (checked by the entry)

    double s[kRowsPerWave][VEC];
#pragma unroll
    for (int j = 0; j < kRowsPerWave; ++j)
#pragma unroll
        for (int i = 0; i < VEC; ++i) s[j][i] = 0.0;
    for (int j0 = 0; j0 < nrows;) {                                // pieces of one parameter row each (wave-uniform bounds)
        const int64_t prow = a.rpp ? (r0 + j0) / a.rpp : 0;
        const int64_t left = a.rpp ? (prow + 1) * a.rpp - r0 : (int64_t)nrows;
        const int j1 = (left < (int64_t)nrows) ? (int)left : nrows;
        double hz[VEC], ph[VEC], sp[VEC];
        sig_osc::SyncRatio ra[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const int v = v0 + i;
            hz[i] = (v < a.voices) ? a.hertz[prow * a.hrs + (int64_t)v * a.hs] : 0.0;
            ph[i] = (v < a.voices && a.phase) ? a.phase[prow * a.prs + (int64_t)v * a.ps] : 0.0;
            sp[i] = (v < a.voices && un.spread) ? un.spread[prow * un.srs + (int64_t)v * un.ss] : 0.0;
            ra[i] = sig_osc::sync_ratio<KIND>((v < a.voices && sy.ratio) ? sy.ratio[prow * sy.rrs + (int64_t)v * sy.rs] : 0.0);
        }
        for (int u = 0; u < copies; ++u) {                         // wave-uniform trip count
            const double du = un.detune[u], pu = un.offset[u];     // (scalar loads from the argument block)
            double h[VEC], qu[VEC], d[VEC], inv_d[VEC], ds[VEC], inv_ds[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const double r = 1.0 + sp[i] * du;
                h[i] = hz[i] * r;
                qu[i] = ph[i] + pu;
                sig_osc::blep_increment(h[i], a.rate, d[i], inv_d[i]);
                sig_osc::sync_increment(d[i], ra[i].R, ds[i], inv_ds[i]);
            }
#pragma unroll
            for (int j = 0; j < kRowsPerWave; ++j) {
                if (j >= j0 && j < j1) {                           // wave-uniform
                    const double q = sig_readlane_f64(q_lane, j);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        const double w = sig_osc::osc_sync<KIND>(q * h[i] + qu[i], d[i], inv_d[i], ra[i], ds[i], inv_ds[i]);
                        s[j][i] = (u == 0) ? w : s[j][i] + w;
                    }
                }
            }
        }
        j0 = j1;
    }
    const double count = (double)copies;
#pragma unroll
    for (int j = 0; j < kRowsPerWave; ++j) {
        if (j < nrows) {                                           // wave-uniform: row r0 + j < a.rows
            OUT y[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) y[i] = (OUT)(s[j][i] / count);
            OUT* dst = out + (r0 + j) * ld + v0;
            if (VEC == 4) {
                if (v0 < a.voices) {                               // voices % 4 == 0 on this path
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

// ---- host: the launch geometry, the kind and store-type dispatch, the entries' common arguments

template <int N> using Const = std::integral_constant<int, N>;

// Voices per lane and voice tiles of a launch: four voices and one 16-byte store per lane where every row of `out` allows it
struct VoiceTiling { bool vec4; int voice_tiles; };

template <typename OUT>
VoiceTiling voice_tiling(const OscArgs& a, const OUT* out, int64_t ld)
{
    const bool vec4 = (a.voices % 4 == 0) && (ld % 4 == 0) &&
                      ((reinterpret_cast<uintptr_t>(out) % (4 * sizeof(OUT))) == 0);
    return {vec4, sig_voice_tiles(a.voices, vec4 ? 4 : 1)};
}

// launch(Const<VEC>, workgroups, voice_tiles) over `row_tiles` workgroup rows; refuses more workgroups than a grid dimension holds
template <typename LAUNCH>
int launch_tiles(const VoiceTiling& vt, int64_t row_tiles, LAUNCH&& launch)
{
    const int64_t nwg = row_tiles * vt.voice_tiles;
    if (nwg > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    if (vt.vec4)
        launch(Const<4>{}, (unsigned)nwg, vt.voice_tiles);
    else
        launch(Const<1>{}, (unsigned)nwg, vt.voice_tiles);
    return sig_launch_status();
}

// the same for the kernels whose workgroup is kWavesPerWg waves of kRowsPerWave rows
template <typename OUT, typename LAUNCH>
int launch_bank(const OscArgs& a, OUT* out, int64_t ld, LAUNCH&& launch)
{
    const int64_t rows_per_wg = (int64_t)kRowsPerWave * kWavesPerWg;
    return launch_tiles(voice_tiling(a, out, ld), (a.rows + rows_per_wg - 1) / rows_per_wg, launch);
}

// f(Const<KIND>) for a `kind` among KINDS..., hipErrorInvalidValue without a call for any other
template <int... KINDS, typename F>
int dispatch_kind(int kind, F&& f)
{
    constexpr unsigned allowed = ((1u << KINDS) | ...);
    switch (kind) {
#define SIG_KIND_CASE(K) case K: if constexpr ((allowed >> K) & 1u) return f(Const<K>{}); break;
        SIG_KIND_CASE(SIG_OSC_SINE)
        SIG_KIND_CASE(SIG_OSC_SQUARE)
        SIG_KIND_CASE(SIG_OSC_SAWTOOTH)
        SIG_KIND_CASE(SIG_OSC_TRIANGLE)
#undef SIG_KIND_CASE
    }
    return (int)hipErrorInvalidValue;
}

int run_osc(int kind, const OscArgs& a, void* out, int32_t out_dtype, int64_t ld, void* stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dispatch_out(out, out_dtype, [&](auto* o) {
        using OUT = std::remove_pointer_t<decltype(o)>;
        return dispatch_kind<SIG_OSC_SINE, SIG_OSC_SQUARE, SIG_OSC_SAWTOOTH, SIG_OSC_TRIANGLE>(kind, [&](auto k) {
            return launch_bank(a, o, ld, [&](auto vec, unsigned nwg, int voice_tiles) {
                osc_bank_kernel<decltype(k)::value, decltype(vec)::value, OUT><<<nwg, 256, 0, s>>>(a, o, ld, voice_tiles);
            });
        });
    });
}

template <typename MOD>
int run_pm(int kind, const OscArgs& a, const PmArgs& m, void* out, int32_t out_dtype, int64_t ld, hipStream_t s)
{
    return dispatch_out(out, out_dtype, [&](auto* o) {
        using OUT = std::remove_pointer_t<decltype(o)>;
        return dispatch_kind<SIG_OSC_SINE, SIG_OSC_SQUARE, SIG_OSC_SAWTOOTH, SIG_OSC_TRIANGLE>(kind, [&](auto k) {
            return launch_bank(a, o, ld, [&](auto vec, unsigned nwg, int voice_tiles) {
                constexpr int KIND = decltype(k)::value, VEC = decltype(vec)::value;
                if constexpr (VEC == 4 && sizeof(MOD) == 4) {      // (the 16-byte modulator load exists for float32 only)
                    if (m.mod && m.mcs == 1 && m.mld > 0 && m.mld % 4 == 0 && (reinterpret_cast<uintptr_t>(m.mod) % 16) == 0) {
                        osc_bank_pm_kernel<KIND, 4, OUT, MOD, true><<<nwg, 256, 0, s>>>(a, m, o, ld, voice_tiles);
                        return;
                    }
                }
                osc_bank_pm_kernel<KIND, VEC, OUT, MOD, false><<<nwg, 256, 0, s>>>(a, m, o, ld, voice_tiles);
            });
        });
    });
}

int run_table(const OscArgs& a, TableArgs tb, void* out, int32_t out_dtype, int64_t ld, hipStream_t s)
{
    return dispatch_out(out, out_dtype, [&](auto* o) {
        using OUT = std::remove_pointer_t<decltype(o)>;
        const VoiceTiling vt = voice_tiling(a, o, ld);
        const int64_t rows_per_pass = (int64_t)kRowsPerWave * kTableWaves;
        const int64_t passes = (a.rows + rows_per_pass - 1) / rows_per_pass;
        // as many row groups per wave as still leave two workgroups for every CU of an MI355X (the staging is paid per workgroup)
        tb.groups = 8;
        while (tb.groups > 1 && ((passes + tb.groups - 1) / tb.groups) * vt.voice_tiles < 512) tb.groups >>= 1;
        const size_t lds = sig_table::lds_bytes(tb.T, tb.W);
        return launch_tiles(vt, (passes + tb.groups - 1) / tb.groups, [&](auto vec, unsigned nwg, int voice_tiles) {
            osc_bank_table_kernel<decltype(vec)::value, OUT><<<nwg, 64 * kTableWaves, lds, s>>>(a, tb, o, ld, voice_tiles);
        });
    });
}

// rows of a voice that go through the partial loop together (R of osc_bank_additive_kernel): 8 chains per lane with four voices,
// 4 with one -- 16 chains spill (256 VGPRs and scratch), these compile to 195 and 96 VGPRs without any
template <int VEC> constexpr int kAdditiveRows = (VEC == 4) ? 2 : 4;

int run_additive(const OscArgs& a, AddArgs ad, void* out, int32_t out_dtype, int64_t ld, hipStream_t s)
{
    return dispatch_out(out, out_dtype, [&](auto* o) {
        using OUT = std::remove_pointer_t<decltype(o)>;
        const VoiceTiling vt = voice_tiling(a, o, ld);
        const int64_t rows_per_pass = (int64_t)kRowsPerWave * kTableWaves;
        const int64_t passes = (a.rows + rows_per_pass - 1) / rows_per_pass;
        // run_table's rule: as many row groups per wave as still leave two workgroups for every CU of an MI355X
        ad.groups = 8;
        while (ad.groups > 1 && ((passes + ad.groups - 1) / ad.groups) * vt.voice_tiles < 512) ad.groups >>= 1;
        const size_t lds = (size_t)ad.S * ad.W * sizeof(float);
        return launch_tiles(vt, (passes + ad.groups - 1) / ad.groups, [&](auto vec, unsigned nwg, int voice_tiles) {
            osc_bank_additive_kernel<decltype(vec)::value, kAdditiveRows<decltype(vec)::value>, OUT><<<nwg, 64 * kTableWaves, lds, s>>>(a, ad, o, ld, voice_tiles);
        });
    });
}

// the three launches of (OscArgs, UniArgs[, SyncArgs]) kernels: LAUNCH(Const<KIND>, Const<VEC>, out, workgroups, voice_tiles)
template <int... KINDS, typename LAUNCH>
int run_copies(int kind, const OscArgs& a, void* out, int32_t out_dtype, int64_t ld, LAUNCH&& launch)
{
    return dispatch_out(out, out_dtype, [&](auto* o) {
        return dispatch_kind<KINDS...>(kind, [&](auto k) {
            return launch_bank(a, o, ld, [&](auto vec, unsigned nwg, int voice_tiles) { launch(k, vec, o, nwg, voice_tiles); });
        });
    });
}

// The arguments common to the entries, checked, as OscArgs
int osc_args(OscArgs& a, int64_t position, int64_t position_step, int32_t rate, int64_t rows, int32_t voices, int32_t rows_per_param,
             const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
             const double* phase, int32_t phase_stride, int64_t phase_row_stride, const void* out, int64_t out_ld)
{
    SIG_CHECK_ARG(sig_rows::head_ok(position, position_step, rate, rows, voices, rows_per_param));
    SIG_CHECK_ARG(hertz != nullptr && out != nullptr && out_ld >= voices);
    SIG_CHECK_ARG(sig_rows::strides_ok(hertz_stride, hertz_row_stride) && sig_rows::strides_ok(phase_stride, phase_row_stride));
    a = OscArgs{position, position_step, (double)rate, rows, voices, hertz, hertz_stride, hertz_row_stride,
                phase, phase_stride, phase_row_stride, rows_per_param};
    return 0;
}

// The spread row and the copies of the unison entries, checked, as UniArgs
int uni_args(UniArgs& un, const double* spread, int32_t spread_stride, int64_t spread_row_stride,
             int32_t copies, const double* detune, const double* offsets)
{
    SIG_CHECK_ARG(sig_rows::strides_ok(spread_stride, spread_row_stride));
    SIG_CHECK_ARG(copies >= 1 && copies <= SIG_UNISON_MAX_COPIES && detune != nullptr && offsets != nullptr);
    un = UniArgs{spread, spread_stride, spread_row_stride, copies, {0.0}, {0.0}};
    for (int u = 0; u < copies; ++u) { un.detune[u] = detune[u]; un.offset[u] = offsets[u]; }
    return 0;
}

#define SIG_TRY(call) do { const int status_ = (call); if (status_ != 0) return status_; } while (0)

}  // namespace

extern "C" int sig_osc_bank_sync(int kind, int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                                 int32_t voices, int32_t rows_per_param,
                                 const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                                 const double* phase, int32_t phase_stride, int64_t phase_row_stride,
                                 const double* spread, int32_t spread_stride, int64_t spread_row_stride,
                                 const double* ratio, int32_t ratio_stride, int64_t ratio_row_stride,
                                 int32_t copies, const double* detune, const double* offsets,
                                 void* out, int32_t out_dtype, int64_t out_ld, void* stream)
{
    OscArgs a;
    UniArgs un;
    SIG_CHECK_ARG(kind == SIG_OSC_SQUARE || kind == SIG_OSC_SAWTOOTH);
    SIG_TRY(osc_args(a, position, position_step, rate, rows, voices, rows_per_param, hertz, hertz_stride, hertz_row_stride,
                     phase, phase_stride, phase_row_stride, out, out_ld));
    SIG_TRY(uni_args(un, spread, spread_stride, spread_row_stride, copies, detune, offsets));
    SIG_CHECK_ARG(sig_rows::strides_ok(ratio_stride, ratio_row_stride));
    SIG_CHECK_ARG(out_dtype == SIG_F32 || out_dtype == SIG_F64);
    if (rows == 0 || voices == 0) return 0;
    const SyncArgs sy{ratio, ratio_stride, ratio_row_stride};
    hipStream_t s = static_cast<hipStream_t>(stream);
    return run_copies<SIG_OSC_SQUARE, SIG_OSC_SAWTOOTH>(                       // (Sine, Triangle: their reset changes the slope too)
        kind, a, out, out_dtype, out_ld, [&](auto k, auto vec, auto* o, unsigned nwg, int voice_tiles) {
            osc_bank_sync_kernel<decltype(k)::value, decltype(vec)::value><<<nwg, 256, 0, s>>>(a, un, sy, o, out_ld, voice_tiles);
        });
}

extern "C" int sig_osc_bank_blep(int kind, int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                                 int32_t voices, int32_t rows_per_param,
                                 const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                                 const double* phase, int32_t phase_stride, int64_t phase_row_stride,
                                 const double* spread, int32_t spread_stride, int64_t spread_row_stride,
                                 int32_t copies, const double* detune, const double* offsets,
                                 void* out, int32_t out_dtype, int64_t out_ld, void* stream)
{
    OscArgs a;
    UniArgs un;
    SIG_CHECK_ARG(kind == SIG_OSC_SQUARE || kind == SIG_OSC_SAWTOOTH || kind == SIG_OSC_TRIANGLE);
    SIG_TRY(osc_args(a, position, position_step, rate, rows, voices, rows_per_param, hertz, hertz_stride, hertz_row_stride,
                     phase, phase_stride, phase_row_stride, out, out_ld));
    SIG_TRY(uni_args(un, spread, spread_stride, spread_row_stride, copies, detune, offsets));
    SIG_CHECK_ARG(out_dtype == SIG_F32 || out_dtype == SIG_F64);
    if (rows == 0 || voices == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return run_copies<SIG_OSC_SQUARE, SIG_OSC_SAWTOOTH, SIG_OSC_TRIANGLE>(     // (Sine: it has no edge to correct)
        kind, a, out, out_dtype, out_ld, [&](auto k, auto vec, auto* o, unsigned nwg, int voice_tiles) {
            osc_bank_blep_kernel<decltype(k)::value, decltype(vec)::value><<<nwg, 256, 0, s>>>(a, un, o, out_ld, voice_tiles);
        });
}

extern "C" int sig_osc_bank_unison(int kind, int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                                   int32_t voices, int32_t rows_per_param,
                                   const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                                   const double* phase, int32_t phase_stride, int64_t phase_row_stride,
                                   const double* spread, int32_t spread_stride, int64_t spread_row_stride,
                                   int32_t copies, const double* detune, const double* offsets,
                                   void* out, int32_t out_dtype, int64_t out_ld, void* stream)
{
    OscArgs a;
    UniArgs un;
    SIG_CHECK_ARG(kind >= SIG_OSC_SINE && kind <= SIG_OSC_TRIANGLE);
    SIG_TRY(osc_args(a, position, position_step, rate, rows, voices, rows_per_param, hertz, hertz_stride, hertz_row_stride,
                     phase, phase_stride, phase_row_stride, out, out_ld));
    SIG_TRY(uni_args(un, spread, spread_stride, spread_row_stride, copies, detune, offsets));
    SIG_CHECK_ARG(out_dtype == SIG_F32 || out_dtype == SIG_F64);
    if (rows == 0 || voices == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return run_copies<SIG_OSC_SINE, SIG_OSC_SQUARE, SIG_OSC_SAWTOOTH, SIG_OSC_TRIANGLE>(
        kind, a, out, out_dtype, out_ld, [&](auto k, auto vec, auto* o, unsigned nwg, int voice_tiles) {
            osc_bank_unison_kernel<decltype(k)::value, decltype(vec)::value><<<nwg, 256, 0, s>>>(a, un, o, out_ld, voice_tiles);
        });
}

extern "C" int sig_osc_bank_table(int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                                  int32_t voices, int32_t rows_per_param,
                                  const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                                  const double* phase, int32_t phase_stride, int64_t phase_row_stride,
                                  const double* select, int32_t select_stride, int64_t select_row_stride,
                                  const float* table, int32_t table_points, int32_t table_waves,
                                  void* out, int32_t out_dtype, int64_t out_ld, void* stream)
{
    OscArgs a;
    SIG_TRY(osc_args(a, position, position_step, rate, rows, voices, rows_per_param, hertz, hertz_stride, hertz_row_stride,
                     phase, phase_stride, phase_row_stride, out, out_ld));
    SIG_CHECK_ARG(sig_rows::strides_ok(select_stride, select_row_stride));
    SIG_CHECK_ARG(table != nullptr && table_points >= 2 && (table_points & (table_points - 1)) == 0 && table_waves >= 1 &&
                  (int64_t)table_points * table_waves <= SIG_TABLE_MAX_POINTS);
    SIG_CHECK_ARG(out_dtype == SIG_F32 || out_dtype == SIG_F64);
    if (rows == 0 || voices == 0) return 0;
    const TableArgs tb{table, table_points, table_waves, select, select_stride, select_row_stride, 1};
    return run_table(a, tb, out, out_dtype, out_ld, static_cast<hipStream_t>(stream));
}

extern "C" int sig_osc_bank_additive(int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                                     int32_t voices, int32_t rows_per_param,
                                     const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                                     const double* phase, int32_t phase_stride, int64_t phase_row_stride,
                                     const double* select, int32_t select_stride, int64_t select_row_stride,
                                     const float* table, int32_t table_partials, int32_t table_waves,
                                     void* out, int32_t out_dtype, int64_t out_ld, void* stream)
{
    OscArgs a;
    SIG_TRY(osc_args(a, position, position_step, rate, rows, voices, rows_per_param, hertz, hertz_stride, hertz_row_stride,
                     phase, phase_stride, phase_row_stride, out, out_ld));
    SIG_CHECK_ARG(sig_rows::strides_ok(select_stride, select_row_stride));
    SIG_CHECK_ARG(table != nullptr && table_partials >= 1 && table_partials <= SIG_ADDITIVE_MAX_PARTIALS && table_waves >= 1 &&
                  (int64_t)table_partials * table_waves <= SIG_TABLE_MAX_POINTS);
    SIG_CHECK_ARG(out_dtype == SIG_F32 || out_dtype == SIG_F64);
    if (rows == 0 || voices == 0) return 0;
    const int odd = table_partials | 1;                            // (the odd stride where the table still fits 64 KiB of LDS)
    const int stride = ((int64_t)odd * table_waves <= SIG_TABLE_MAX_POINTS) ? odd : table_partials;
    const AddArgs ad{table, table_partials, table_waves, stride, select, select_stride, select_row_stride, 1};
    return run_additive(a, ad, out, out_dtype, out_ld, static_cast<hipStream_t>(stream));
}

extern "C" int sig_osc_bank_pm(int kind, int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                               int32_t voices, int32_t rows_per_param,
                               const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                               const double* phase, int32_t phase_stride, int64_t phase_row_stride,
                               const double* index, int32_t index_stride, int64_t index_row_stride,
                               const void* mod, int32_t mod_dtype, int64_t mod_ld, int32_t mod_stride,
                               void* out, int32_t out_dtype, int64_t out_ld, void* stream)
{
    OscArgs a;
    SIG_TRY(osc_args(a, position, position_step, rate, rows, voices, rows_per_param, hertz, hertz_stride, hertz_row_stride,
                     phase, phase_stride, phase_row_stride, out, out_ld));
    SIG_CHECK_ARG(sig_rows::strides_ok(index_stride, index_row_stride));
    SIG_CHECK_ARG(mod == nullptr || ((mod_dtype == SIG_F32 || mod_dtype == SIG_F64) && (mod_stride == 0 || mod_stride == 1) &&
                                     (mod_ld == 0 || mod_ld >= (mod_stride ? voices : 1))));
    if (rows == 0 || voices == 0) return 0;
    const PmArgs m{index, index_stride, index_row_stride, mod, mod_ld, mod_stride};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (mod != nullptr && mod_dtype == SIG_F64) return run_pm<double>(kind, a, m, out, out_dtype, out_ld, s);
    return run_pm<float>(kind, a, m, out, out_dtype, out_ld, s);
}

extern "C" int sig_osc_bank(int kind, int64_t position, int32_t rate, int64_t rows, int32_t voices,
                            const double* hertz, int32_t hertz_stride,
                            const double* phase, int32_t phase_stride,
                            void* out, int32_t out_dtype, int64_t out_ld, void* stream)
{
    OscArgs a;                                                     // one parameter row, consecutive frames
    SIG_TRY(osc_args(a, position, 1, rate, rows, voices, 0, hertz, hertz_stride, 0, phase, phase_stride, 0, out, out_ld));
    if (rows == 0 || voices == 0) return 0;
    return run_osc(kind, a, out, out_dtype, out_ld, stream);
}

extern "C" int sig_osc_bank_mod(int kind, int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                                int32_t voices, int32_t rows_per_param,
                                const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                                const double* phase, int32_t phase_stride, int64_t phase_row_stride,
                                void* out, int32_t out_dtype, int64_t out_ld, void* stream)
{
    OscArgs a;
    SIG_TRY(osc_args(a, position, position_step, rate, rows, voices, rows_per_param, hertz, hertz_stride, hertz_row_stride,
                     phase, phase_stride, phase_row_stride, out, out_ld));
    if (rows == 0 || voices == 0) return 0;
    return run_osc(kind, a, out, out_dtype, out_ld, stream);
}

extern "C" int sig_abi_version(void) { return SIG_ABI_VERSION; }
