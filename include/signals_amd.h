/* signals_amd.h -- C ABI of the MI355X (gfx950) block-render kernels.
 *
 * The reference (noah-aviel-dove/signals) is 100 % Python: its render path has no FFI.
 * The functions a native back end has to replace are the numpy/scipy bodies of the
 * nodes' `_eval` methods; each entry point below names the one it stands in for
 * (paths relative to /root/reference/src/signals/).  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *  - audio buffers: row-major (frames, channels), channel (= voice) index contiguous,
 *    `ld` = elements between consecutive rows.  dtype f32 (SIG_F32) by default; every
 *    entry also accepts f64 (SIG_F64) buffers, which block-rate (frames == 1) control
 *    requests use.
 *  - control rows (hertz, phase, cutoff, gain ...): f64, `stride` 1 = one value per voice,
 *    0 = one scalar broadcast to every voice (a (1,1) reply, chain/__init__.py:59-63).
 *  - every pointer is a DEVICE pointer; the caller owns all memory; nothing is allocated,
 *    freed or synchronised inside (safe to capture into a hipGraph).
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *  - return value: 0 on success, otherwise a hipError_t (1 = hipErrorInvalidValue for
 *    argument errors).  No exceptions cross the boundary.
 */
#ifndef SIGNALS_AMD_H
#define SIGNALS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIG_ABI_VERSION 7

enum { SIG_F32 = 0, SIG_F64 = 1 };

/* oscillator kinds: osc.py:40-62 */
enum { SIG_OSC_SINE = 0, SIG_OSC_SQUARE = 1, SIG_OSC_SAWTOOTH = 2, SIG_OSC_TRIANGLE = 3 };

/* critical-frequency filter types: fx.py:68-72 (only lp/hp are live in the reference, fx.py:142-151) */
enum { SIG_FILT_LOWPASS = 0, SIG_FILT_HIGHPASS = 1, SIG_FILT_BANDPASS = 2, SIG_FILT_BANDSTOP = 3,
       /* filter slots of a voice program that a FILTERQ word runs: the resonant low-pass / high-pass of chain/ext.py */
       SIG_FILT_RES_LOWPASS = 4, SIG_FILT_RES_HIGHPASS = 5,
       /* the RBJ equaliser biquads of chain/ext.py EqFilter: sig_biquad_coldstart_eq's types, and the filter slots of a voice program
        * that a FILTEREQ word runs */
       SIG_FILT_EQ_BANDPASS = 6, SIG_FILT_EQ_NOTCH = 7, SIG_FILT_EQ_ALLPASS = 8, SIG_FILT_EQ_PEAKING = 9, SIG_FILT_EQ_LOWSHELF = 10,
       SIG_FILT_EQ_HIGHSHELF = 11,
       /* the 4-pole ladder of chain/ext.py Ladder: the node's own type, run by sig_ladder_coldstart alone */
       SIG_FILT_LADDER = 12 };

/* element-wise effects: fx.py:35-60 */
enum { SIG_EW_GAIN = 0, SIG_EW_MIX = 1, SIG_EW_RINGMOD = 2, SIG_EW_AMP = 3 };

/* bits OR-ed into the optional device status word by kernels (never cleared by them) */
enum { SIG_STATUS_BAD_CUTOFF = 1,     /* Wn <= 0 or >= 1: scipy raises ValueError (fx.py:99-102) */
       SIG_STATUS_BAD_RESONANCE = 2,    /* a resonant filter's q that is not finite and > 0 (build-defined, chain/ext.py ResonantFilter) */
       SIG_STATUS_BAD_GAIN = 4 };       /* an equaliser filter's gain (dB) that is not finite (build-defined, chain/ext.py EqFilter) */

int sig_abi_version(void);

/* Replaces Osc._eval + Sine/Square/Sawtooth/Triangle._osc (osc.py:26-62):
 *   t[n,v] = (position + n) / rate * hertz[v] + phase[v]      (f64, that operator order)
 *   out[n,v] = wave_kind(t[n,v])
 * Position-pure: `rows` may span any number of consecutive blocks.
 * Square/Sawtooth/Triangle are bit-exact in f64 before the store.  Sine: f64 store within 1 ulp(f64)
 * (f64 polynomial); f32 store within 1.3e-7 (exact f64 phase reduction, then v_sin_f32). */
int sig_osc_bank(int kind, int64_t position, int32_t rate, int64_t rows, int32_t voices,
                 const double* hertz, int32_t hertz_stride,
                 const double* phase, int32_t phase_stride,   /* phase may be NULL = unplugged = 0 */
                 void* out, int32_t out_dtype, int64_t out_ld, void* stream);

/* sig_osc_bank for launches whose control inputs change per block (Osc._eval reads hertz and phase through
 * forward_at_block_rate, osc.py:28-30, so in a K-block batch they are K rows) and for block-RATE launches:
 *   output row r is frame position + r * position_step and uses parameter row r / rows_per_param
 *   (rows_per_param == 0: a single parameter row, the *_row_stride arguments are ignored).
 * audio rate, per-block parameters: position_step = 1, rows_per_param = block_frames;
 * block rate (what a control port sees for K blocks): position_step = block_frames, rows_per_param = 1. */
int sig_osc_bank_mod(int kind, int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                     int32_t voices, int32_t rows_per_param,
                     const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                     const double* phase, int32_t phase_stride, int64_t phase_row_stride,
                     void* out, int32_t out_dtype, int64_t out_ld, void* stream);

/* Phase-modulation (FM) oscillators, chain/ext.py PMSine / PMSquare / PMSawtooth / PMTriangle: sig_osc_bank_mod with the phase
 * offset by a frame-rate modulator,
 *   t[n,v]   = ((position + n * position_step) / rate * hertz[v] + phase[v]) + index[v] * (double) mod[n,v]   (f64, that order)
 *   out[n,v] = wave_kind(t[n,v])
 * `index` rows: like hertz / phase (per block with rows_per_param); NULL = unplugged = 0.  `mod`: SIG_F32 | SIG_F64,
 * row n at mod + n * mod_ld, mod_stride 1 = (rows, voices), 0 = (rows, 1); mod_ld 0 = one row for every n; NULL = unplugged = 0.
 * Position-pure given `mod`.  Same contract as sig_osc_bank: Square / Sawtooth / Triangle bit-exact in f64 before the store,
 * Sine f64 store within 1 ulp(f64) of the f64 polynomial, f32 store within 1.3e-7. */
int sig_osc_bank_pm(int kind, int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                    int32_t voices, int32_t rows_per_param,
                    const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                    const double* phase, int32_t phase_stride, int64_t phase_row_stride,
                    const double* index, int32_t index_stride, int64_t index_row_stride,
                    const void* mod, int32_t mod_dtype, int64_t mod_ld, int32_t mod_stride,
                    void* out, int32_t out_dtype, int64_t out_ld, void* stream);

/* Wavetable oscillator, chain/ext.py Wavetable: sig_osc_bank_mod's phase looked up in a table of W single-cycle waveforms of T
 * points each, `table` float32 (T, W) row-major in device memory, T a power of two >= 2, W >= 1, T * W <= SIG_TABLE_MAX_POINTS:
 *   t = (position + n * position_step) / rate * hertz[v] + phase[v]        (f64, that order)
 *   m = np.mod(t, 1.0);  u = m * T;  i = floor(u);  f = u - i              (m == 1.0 for t in (-2^-54, 0): entry 0, f == 0)
 *   w = clip(floor(select[v]), 0, W - 1)                                   (NaN -> 0; select NULL = unplugged = column 0)
 *   out[n,v] = tbl[i & (T-1), w] + f * (tbl[(i+1) & (T-1), w] - tbl[i & (T-1), w])      tbl = (double) table, every operation rounded
 * `select` rows like hertz / phase (per block with rows_per_param).  Position-pure.  The float64 value in front of the store is
 * bit-exact against numpy.  A null table, T not a power of two, T * W over the cap or out_ld < voices: hipErrorInvalidValue,
 * nothing launched; rows == 0: no launch. */
enum { SIG_TABLE_MAX_POINTS = 16384 };
int sig_osc_bank_table(int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                       int32_t voices, int32_t rows_per_param,
                       const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                       const double* phase, int32_t phase_stride, int64_t phase_row_stride,
                       const double* select, int32_t select_stride, int64_t select_row_stride,
                       const float* table, int32_t table_points, int32_t table_waves,
                       void* out, int32_t out_dtype, int64_t out_ld, void* stream);

/* Additive oscillator, chain/ext.py Additive: up to SIG_ADDITIVE_MAX_PARTIALS harmonics per voice with amplitudes from a table, the
 * partials above half the rate dropped per voice and parameter row.  `table` float32 (H, W) row-major in device memory, row h - 1
 * the amplitude of harmonic h for each of W spectra, 1 <= H <= SIG_ADDITIVE_MAX_PARTIALS, W >= 1, H * W <= SIG_TABLE_MAX_POINTS:
 *   t  = (position + n * position_step) / rate * hertz[v] + phase[v];  m = np.mod(t, 1.0)         (f64, that order)
 *   w  = clip(floor(select[v]), 0, W - 1)                                   (NaN -> 0; select NULL = unplugged = column 0)
 *   nf = (0.5 * rate) / |hertz[v]|;  k = clip(ceil(nf) - 1, 0, H);  g = min(1.0, nf - k)
 *   out[n,v] = sum over h = 1 .. k of a[h-1, w] * (h == k ? g : 1) * sin(2 pi h m)                  a = (double) table
 * k == 0 (|hertz| >= rate / 2, +-inf too): exactly 0.0; a NaN hertz: NaN; a non-finite phase with k >= 1: NaN.  hertz / phase /
 * select rows like sig_osc_bank_table (per block with rows_per_param).  Position-pure.  Held to a bound, not to bits: both stores
 * within 1e-6 * max(1, A) of the definition with the sum in extended precision, A the largest column sum of |a| (measured:
 * DESIGN.md).  A null table / hertz / out, H or H * W out of range, out_ld < voices, a negative position or a stride other than
 * 0 / 1: hipErrorInvalidValue, nothing launched; rows == 0: no launch. */
enum { SIG_ADDITIVE_MAX_PARTIALS = 64 };
int sig_osc_bank_additive(int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                          int32_t voices, int32_t rows_per_param,
                          const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                          const double* phase, int32_t phase_stride, int64_t phase_row_stride,
                          const double* select, int32_t select_stride, int64_t select_row_stride,
                          const float* table, int32_t table_partials, int32_t table_waves,
                          void* out, int32_t out_dtype, int64_t out_ld, void* stream);

/* Unison oscillator, chain/ext.py UnisonSine / UnisonSquare / UnisonSawtooth / UnisonTriangle: `copies` detuned copies of one waveform
 * per voice, summed and divided by their number (the supersaw, detuned square leads, thickened sines).  For row n and voice v, in
 * f64, every operation rounded, u = 0 .. copies - 1 ascending:
 *   r_u = 1.0 + spread[v] * detune[u];   h_u = hertz[v] * r_u;   q_u = phase[v] + offsets[u]
 *   t_u = (position + n * position_step) / rate * h_u + q_u
 *   out[n,v] = (((w(t_0) + w(t_1)) + w(t_2)) + ...) / copies               w = wave_kind, sig_osc_bank's two-instruction forms
 * hertz / phase / spread rows like sig_osc_bank_mod (per block with rows_per_param); phase or spread NULL = unplugged = 0.
 * `detune` and `offsets` are HOST arrays of `copies` doubles, 1 <= copies <= SIG_UNISON_MAX_COPIES, copied into the kernel's
 * argument block (wave-uniform values).  Position-pure.  Square / Sawtooth / Triangle: the float64 value in front of the store is
 * bit-exact against numpy; Sine: the f64 store sums the f64 polynomial, the f32 store sums the hardware sine of sig_osc_bank's f32
 * store per copy in f64 (within 1.3e-7 per copy, so is the mean).  copies == 1 with detune[0] == offsets[0] == 0: sig_osc_bank's
 * bits in both stores.  A null hertz / out / detune / offsets, copies out of range, out_ld < voices or a stride other than 0 / 1:
 * hipErrorInvalidValue, nothing launched; rows == 0: no launch. */
enum { SIG_UNISON_MAX_COPIES = 16 };
int sig_osc_bank_unison(int kind, int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                        int32_t voices, int32_t rows_per_param,
                        const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                        const double* phase, int32_t phase_stride, int64_t phase_row_stride,
                        const double* spread, int32_t spread_stride, int64_t spread_row_stride,
                        int32_t copies, const double* detune, const double* offsets,
                        void* out, int32_t out_dtype, int64_t out_ld, void* stream);

/* Band-limited oscillator, chain/ext.py BlepSquare / BlepSawtooth / BlepTriangle: sig_osc_bank_unison's arguments, checks and
 * expression with each copy's waveform corrected by a two-sample polynomial band-limited step (PolyBLEP) around its edges.  kind is
 * SIG_OSC_SQUARE, SIG_OSC_SAWTOOTH or SIG_OSC_TRIANGLE; SIG_OSC_SINE has no edge and is hipErrorInvalidValue.  With r_u, h_u, q_u and
 * t_u as there (bit for bit), per copy, voice and parameter row  d = min(|h_u| / rate, 0.5)  and, per sample,
 *   step(m)   = 2x - x*x - 1, x = m / d  if m < d  |  y*y + 2y + 1, y = (m - 1) / d  if m > 1 - d  |  0
 *   corner(m) = (1 - m/d)^3              if m < d  |  ((m - 1)/d + 1)^3              if m > 1 - d  |  0
 *   Sawtooth: m = mod(t - 0.5, 1);   w = (2m - 1) - step(m)
 *   Square:   m = mod(t, 1);         w = (m < 0.5 ? 1 : -1) + step(m) - step(mod(t + 0.5, 1))
 *   Triangle: m = mod(t - 0.25, 1);  w = (4 mod(t - 0.25, 0.5) - 1) * (m < 0.5 ? -1 : 1) + (4/3) d (corner(mod(t + 0.25, 1)) - corner(m))
 *             (the first term is 4|m - 0.5| - 1 in sig_osc_bank's order of operations)
 *   out[n,v] = (((w_0 + w_1) + w_2) + ...) / copies
 * The kernel multiplies by a rounded 1 / d (one divide per copy, voice and parameter row, none per sample): the float64 value in
 * front of the store is within 1e-14 of the expression evaluated in numpy's order; outside every window it is the naive waveform's
 * bits, so copies == 1 with detune[0] == offsets[0] == 0 gives sig_osc_bank's samples there.  d == 0 (0 Hz) selects no window;
 * hertz < 0 uses |h_u|; above rate / 4 the Square's windows overlap and above rate / 2 d is clamped: defined, no longer a band
 * limit.  A non-finite t gives NaN.  Position-pure. */
int sig_osc_bank_blep(int kind, int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                      int32_t voices, int32_t rows_per_param,
                      const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                      const double* phase, int32_t phase_stride, int64_t phase_row_stride,
                      const double* spread, int32_t spread_stride, int64_t spread_row_stride,
                      int32_t copies, const double* detune, const double* offsets,
                      void* out, int32_t out_dtype, int64_t out_ld, void* stream);

/* Hard-sync oscillator, chain/ext.py SyncSawtooth / SyncSquare: sig_osc_bank_blep's arguments, checks and phase with one more
 * parameter row, `ratio` ((1|P, V|1) f64 like spread; NULL: unplugged = 0): a slave oscillator at R = max(ratio, 1) times the pitch,
 * reset at every cycle of the master.  kind is SIG_OSC_SAWTOOTH or SIG_OSC_SQUARE; SIG_OSC_SINE and SIG_OSC_TRIANGLE (whose reset
 * changes the slope too) are hipErrorInvalidValue.  With r_u, h_u, q_u, t_u, d and step(m) (at d) as there, per copy, voice and
 * parameter row  ds = min(d R, 0.5)  and  g = R - (ceil(R) - 1),  and per sample  m = mod(t, 1), s = m R, k = floor(s), f = s - k,
 *   estep(p, lo_ok, hi_ok) = 2x - x*x - 1, x = p / ds  if p < ds and lo_ok  |  y*y + 2y + 1, y = (p - 1) / ds  if p > 1 - ds and hi_ok  |  0
 *   Sawtooth: w = (2f - 1) - estep(f, k >= 1, k + 1 < R) - g step(m)
 *   Square:   sb = s + 0.5, kb = floor(sb), fb = sb - kb
 *             w = (f < 0.5 ? 1 : -1) + estep(f, k >= 1, k + 1 < R) - estep(fb, kb >= 1, kb + 0.5 < R) + (g <= 0.5 ? 0 : 1) step(m)
 *   out[n,v] = (((w_0 + w_1) + w_2) + ...) / copies
 * The kernel multiplies by a rounded 1 / d and 1 / ds (divides per copy, voice and parameter row, none per sample): the float64 value
 * in front of the store is within 1e-14 of the expression evaluated in numpy's order.  A ratio that is not finite gives NaN rows for
 * that voice; ratio <= 1 is the band-limited oscillator (the Sawtooth's at phase + 0.5).  d == 0 selects no window; a non-finite t
 * gives NaN.  Where the last interior edge lies closer to the reset than one window (g < ds; Square: 0 < g mod 0.5 < ds) its trailing
 * window is cut at the reset: the expression is the definition there too.  Above ds = 0.5 it no longer band-limits.  Position-pure.
 * Argument errors: hipErrorInvalidValue before any HIP call. */
int sig_osc_bank_sync(int kind, int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                      int32_t voices, int32_t rows_per_param,
                      const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                      const double* phase, int32_t phase_stride, int64_t phase_row_stride,
                      const double* spread, int32_t spread_stride, int64_t spread_row_stride,
                      const double* ratio, int32_t ratio_stride, int64_t ratio_row_stride,
                      int32_t copies, const double* detune, const double* offsets,
                      void* out, int32_t out_dtype, int64_t out_ld, void* stream);

/* Table-lookup waveshaper, chain/ext.py Shaper (build-defined: the reference has no memoryless non-linearity but Amp).  `table`
 * float32 (T, W) row-major in device memory: W transfer curves of T points each, spanning input -1 .. +1; T >= 2 (any integer: 2^k + 1
 * points put a knot at x = 0), W >= 1, T * W <= SIG_TABLE_MAX_POINTS.  For every row n and voice v, in f64, every operation rounded:
 *   c = clip(in[n,v], -1, 1)                                               (+-inf clip; NaN stays NaN)
 *   u = (c + 1.0) * ((T - 1) * 0.5);  i = min(floor(u), T - 2);  f = u - i (f in [0, 1]: in = +1 reads the last segment at f = 1)
 *   w = clip(floor(select[v]), 0, W - 1)                                   (NaN -> 0; select NULL = unplugged = column 0)
 *   out[n,v] = tbl[i, w] + f * (tbl[i+1, w] - tbl[i, w])                   tbl = (double) table; NaN where in is NaN
 * `in`: float32 or float64 (rows | 1, voices | 1): in_ld == 0 one row for all, in_stride == 0 one column broadcast over the voices.
 * `select`: f64 (1 | P, voices | 1), output row n reads select row n / rows_per_select (0: one row for the whole launch).
 * The float64 value in front of the store is bit-exact against numpy.  A null pointer, T < 2, T * W over the cap, out_ld < voices or
 * a stride other than 0 / 1: hipErrorInvalidValue, nothing launched; rows == 0: no launch. */
int sig_shaper_table(int64_t rows, int32_t voices,
                     const void* in, int32_t in_dtype, int64_t in_ld, int32_t in_stride,
                     const double* select, int32_t select_stride, int64_t select_row_stride, int32_t rows_per_select,
                     const float* table, int32_t table_points, int32_t table_waves,
                     void* out, int32_t out_dtype, int64_t out_ld, void* stream);

/* Short multi-tap delay line, chain/ext.py Delay (build-defined: the reference has no node that delays a signal).  The rows are
 * `nblocks` consecutive blocks of `block_frames` frames behind `context_rows` rows of context: `in` points at the FIRST row of that
 * window, (context_rows + nblocks * block_frames, voices | 1) float32 or float64 (in_stride == 0: one column broadcast over the
 * voices), whose row r is absolute frame position - context_rows + r; context_rows == min(SIG_DELAY_CONTEXT, position), like a
 * cold-start filter's history.  x[m] = 0 for an absolute frame m < 0: such rows are not read.  `taps` rows (multiplier[u], gain[u]),
 * 1 <= taps <= SIG_DELAY_MAX_TAPS, are HOST arrays copied into the kernel's arguments.  For block b, its row n and voice v, in f64,
 * every operation rounded, the input widened exactly:
 *   t   = time[b or 0, v]                                                  (seconds; NULL = unplugged = 0)
 *   d_u = clip((t * rate) * multiplier[u], 0, SIG_DELAY_MAX_FRAMES)        (NaN stays NaN, +inf -> 99, -inf -> 0)
 *   i_u = floor(d_u);  f_u = d_u - i_u                                     (once per block)
 *   s_u = x[n - i_u] + f_u * (x[n - i_u - 1] - x[n - i_u])
 *   out[n,v] = gain[0] * s_0  (+ gain[1] * s_1 + ... in ascending u)
 * A NaN d_u makes every row of that voice in that block NaN; no index is formed from it.  `time`: f64 (1 | nblocks, voices | 1),
 * time_blocks rows time_row_stride apart.  The float64 value in front of the store is bit-exact against numpy
 * (tests/delay_reference.py).  float32 input is staged in LDS tiles of (SIG_DELAY_TILE_ROWS + SIG_DELAY_CONTEXT) x 64 voices with
 * coalesced row loads; float64 input is gathered.  taps outside 1 .. 16, context_rows > SIG_DELAY_CONTEXT or != min(SIG_DELAY_CONTEXT,
 * position), a null in / out / multiplier / gain, block_frames < 1, out_ld < voices or a stride other than 0 / 1:
 * hipErrorInvalidValue, nothing launched; nblocks == 0 or voices == 0: no launch. */
enum { SIG_DELAY_CONTEXT = 100, SIG_DELAY_MAX_FRAMES = 99, SIG_DELAY_MAX_TAPS = 16, SIG_DELAY_TILE_ROWS = 220 };
int sig_delay_taps(int32_t rate, int64_t position, int32_t block_frames, int32_t nblocks, int32_t context_rows, int32_t voices,
                   const void* in, int32_t in_dtype, int64_t in_ld, int32_t in_stride,
                   const double* time, int32_t time_stride, int64_t time_row_stride, int32_t time_blocks,
                   int32_t taps, const double* multiplier, const double* gain,
                   void* out, int32_t out_dtype, int64_t out_ld, void* stream);

/* Dense FIR filter, chain/ext.py FIR (build-defined: every filter of the reference is recursive).  The window, the blocks and the
 * buffers of sig_delay_taps: `nblocks` consecutive blocks of `block_frames` frames behind `context_rows` == min(SIG_FIR_CONTEXT,
 * position) rows of context, `in` pointing at the window's FIRST row, float32 or float64 (in_stride == 0: one column broadcast over
 * the voices); x[m] = +0 for an absolute frame m < 0: such rows are not read.  `taps` is a DEVICE array, float64 (table_taps,
 * table_waves) row-major: table_waves impulse responses of table_taps = L taps each, 1 <= L <= SIG_FIR_MAX_TAPS, table_waves = W >= 1,
 * L * W <= SIG_FIR_MAX_POINTS.  For block b, its row n and voice v, in f64, every operation rounded, the input widened exactly:
 *   w   = clip(floor(select[b or 0, v]), 0, W - 1)                         (NULL = unplugged, NaN: column 0; once per block)
 *   acc = taps[0, w] * x[n]
 *   acc = acc + taps[k, w] * x[n - k]                                      (k = 1 .. L - 1, ascending)
 *   out[n, v] = acc
 * No tap is skipped: zero taps and the zero-filled rows are multiplied and added like the rest, so NaN and +-inf in the input
 * propagate as they do in numpy; no status word.  `select`: f64 (1 | nblocks, voices | 1), select_blocks rows select_row_stride
 * apart.  The float64 value in front of the store is bit-exact against numpy (tests/fir_reference.py).  float32 input is staged in LDS
 * tiles of (SIG_FIR_TILE_ROWS + SIG_FIR_CONTEXT) x 64 voices beside the table; float64 input is gathered.  L outside 1 .. 101, W < 1,
 * L * W > SIG_FIR_MAX_POINTS, context_rows > SIG_FIR_CONTEXT or != min(SIG_FIR_CONTEXT, position), a null in / out / taps,
 * block_frames < 1, out_ld < voices or a stride other than 0 / 1: hipErrorInvalidValue, nothing launched; nblocks == 0 or
 * voices == 0: no launch. */
enum { SIG_FIR_CONTEXT = 100, SIG_FIR_MAX_TAPS = 101, SIG_FIR_MAX_POINTS = 4096, SIG_FIR_TILE_ROWS = 256 };
int sig_fir_taps(int32_t rate, int64_t position, int32_t block_frames, int32_t nblocks, int32_t context_rows, int32_t voices,
                 const void* in, int32_t in_dtype, int64_t in_ld, int32_t in_stride,
                 const double* select, int32_t select_stride, int64_t select_row_stride, int32_t select_blocks,
                 const double* taps, int32_t table_taps, int32_t table_waves,
                 void* out, int32_t out_dtype, int64_t out_ld, void* stream);

/* Sample playback, chain/ext.py Sampler (build-defined: the reference streams a file linearly and has no pitch, trigger or per-voice
 * start).  `table` float32 in device memory, COLUMN-major: table_waves recordings of table_frames frames, recording w contiguous at
 * table + w * table_frames (the transpose of the node's (T, W) state); T >= 2, W >= 1, T * W <= SIG_SAMPLER_MAX_POINTS.  loop_end == 0:
 * no loop, else 0 <= loop_start < loop_end <= T.  Rows, strides, `position_step` and `rows_per_param` as sig_osc_bank_table takes them:
 * output row r is absolute frame n = position + r * position_step and reads control row r / rows_per_param (0: one row for the whole
 * launch); ratio, offset, gate_on, select: f64 (1 | P, voices | 1), NULL = unplugged = 0.  A pure function of n, no carried read
 * pointer; per voice v, in f64, every operation rounded, tbl = (double) table:
 *   q = n / rate;  e = q - gate_on[v];  s = e * rate;  u = s * ratio[v] + offset[v]
 *   not (e >= 0)          -> out = 0                                       (before the trigger; a NaN gate is silence)
 *   u is NaN or +-inf     -> out = NaN                                     (no index is formed from it)
 *   no loop:  u < 0 or u > T - 1 -> out = 0;  i = floor(u); f = u - i; j = min(i + 1, T - 1)
 *   loop:     u < 0 -> out = 0;  L = loop_end - loop_start
 *             u >= loop_end:  c = floor((u - loop_start) / L);  u = (u - loop_start) - c * L + loop_start
 *                             if that rounds to u >= loop_end:  u = loop_start
 *                             (likewise if it falls below loop_start: from 2^53 frames on the rounded quotient can exceed the true one)
 *             i = floor(u); f = u - i; j = (i + 1 >= loop_end) ? loop_start : i + 1
 *   w = clip(floor(select[v]), 0, W - 1)                                   (NaN -> 0)
 *   out[n,v] = tbl[i, w] + f * (tbl[j, w] - tbl[i, w])
 * The float64 value in front of the store is bit-exact against numpy (tests/sampler_reference.py); no status word.  Lanes own voices
 * and gather from the table in HBM (no LDS).  A null table or out, T < 2, W < 1, T * W over the cap, loop bounds outside the rule,
 * out_ld < voices or a stride other than 0 / 1: hipErrorInvalidValue, nothing launched; rows == 0 or voices == 0: no launch. */
enum { SIG_SAMPLER_MAX_POINTS = 1 << 26 };
int sig_sampler_play(int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                     int32_t voices, int32_t rows_per_param,
                     const double* ratio, int32_t ratio_stride, int64_t ratio_row_stride,
                     const double* offset, int32_t offset_stride, int64_t offset_row_stride,
                     const double* gate_on, int32_t gate_on_stride, int64_t gate_on_row_stride,
                     const double* select, int32_t select_stride, int64_t select_row_stride,
                     const float* table, int32_t table_frames, int32_t table_waves,
                     int32_t loop_start, int32_t loop_end,
                     void* out, int32_t out_dtype, int64_t out_ld, void* stream);

/* Modal resonator bank, chain/ext.py Modal (build-defined: the reference has no struck or plucked source): per voice up to
 * SIG_MODAL_MAX_MODES exponentially decaying sinusoids struck at gate_on, each with its own frequency ratio, amplitude and decay.
 * `modes` float64 in device memory, (sets, count, 3) row-major: row i of set w is (ratio r >= 0, amplitude a, decay rate lambda in
 * 1 / s; the node computes lambda = ln(1000) / t60 on the host, t60 = inf -> 0), 1 <= count <= SIG_MODAL_MAX_MODES, sets >= 1,
 * sets * count <= SIG_MODAL_MAX_POINTS.  Rows, strides, `position_step` and `rows_per_param` as sig_sampler_play takes them: output row
 * r is absolute frame n = position + r * position_step and reads control row r / rows_per_param (0: one row for the whole launch);
 * hertz, gate_on, damp, select: f64 (1 | P, voices | 1), NULL = unplugged = 0 (hertz must be given).  A pure function of n, no state;
 * per voice v, in f64, every operation rounded, no fused multiply-add, i = 0 .. count - 1 added in ascending order:
 *   q = n / rate;  e = q - gate_on[v]
 *   not (e >= 0)          -> out = 0.0                                     (before the strike; a NaN gate is silence; exact zero)
 *   w = clip(floor(select[v]), 0, sets - 1)                                (NaN -> 0)
 *   F_i = hertz[v] * r_i
 *   g_i = clip(((0.5 * rate) - |F_i|) / |hertz[v]|, 0, 1)                  (IEEE: hertz = 0 gives +inf -> 1)
 *   c_i = e * F_i;  m_i = np.mod(c_i, 1.0);  k_i = (lambda_i + damp[v]) * e
 *   out[n,v] = sum_i (a_i * g_i) * exp(-k_i) * sin(2 pi m_i)               (a mode with g_i == 0 adds exactly 0)
 * A hertz or damp that is not finite gives NaN on sounding rows (e >= 0) and 0.0 before the strike; every mode dropped: exactly 0.0.
 * Held to a bound, not to bits: both stores within 1e-6 * max(1, A) of the definition, A the largest set's sum of |a| (the kernel
 * starts each run of 64 rows from the closed form and advances it by a complex multiplication per row; measured: DESIGN.md).  A
 * sample's bits do not depend on how a stretch of frames is cut into launches or parameter rows.  No status word.  A null modes /
 * hertz / out, count or sets * count out of range, out_ld < voices, a negative position or a stride other than 0 / 1:
 * hipErrorInvalidValue, nothing launched; rows == 0 or voices == 0: no launch. */
enum { SIG_MODAL_MAX_MODES = 64, SIG_MODAL_MAX_POINTS = 2048 };
int sig_modal_bank(int64_t position, int64_t position_step, int32_t rate, int64_t rows,
                   int32_t voices, int32_t rows_per_param,
                   const double* hertz, int32_t hertz_stride, int64_t hertz_row_stride,
                   const double* gate_on, int32_t gate_on_stride, int64_t gate_on_row_stride,
                   const double* damp, int32_t damp_stride, int64_t damp_row_stride,
                   const double* select, int32_t select_stride, int64_t select_row_stride,
                   const double* modes, int32_t sets, int32_t count,
                   void* out, int32_t out_dtype, int64_t out_ld, void* stream);

/* Replaces CritFilter._filter + _get_sos (fx.py:85-121) for LowPass/HighPass (order 2 = one
 * biquad section), batched over `nblocks` consecutive blocks of `block_frames` frames.
 * For block b (p_b = position + b*block_frames, c_b = min(context, p_b)):
 *   design butter(2, clip(cutoff[b or 0, v] / (rate/2), 0, 1)) in closed form,
 *   run the DF2T recurrence in f64 from ZERO state over in rows [b*N - c_b, (b+1)*N),
 *   store rows [b*N, (b+1)*N).
 * `in` points at the row aligned with out row 0; `in_history` rows (>= min(context, position))
 * must precede it in the same allocation (same ld).  The reference's `after` window never
 * reaches the kept samples (sosfilt is causal) and is not read.
 * cutoff: (cutoff_blocks, voices) f64 with cutoff_blocks in {1, nblocks}; stride 0/1 as above.
 * status: optional device int32; SIG_STATUS_BAD_CUTOFF is OR-ed in and the voice's output is NaN. */
int sig_biquad_coldstart(int type, int32_t rate, int64_t position,
                         int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                         const double* cutoff, int32_t cutoff_stride, int32_t cutoff_blocks,
                         const void* in, int64_t in_ld, int64_t in_history,
                         void* out, int64_t out_ld, int32_t dtype,
                         int32_t* status, void* stream);

/* sig_biquad_coldstart with a resonance control: the resonant 2-pole low-pass / high-pass of chain/ext.py ResonantLowPass /
 * ResonantHighPass (build-defined: every filter of the reference is a Butterworth at q = 1/sqrt2).  Per voice and block, in f64:
 *   wn = clip(cutoff / (rate / 2), 0, 1);  k = tan(pi wn / 2);  d = 1 / q;  nrm = 1 / (1 + d k + k k)
 *   lp: b = (k k, 2 k k, k k) nrm      hp: b = (1, -2, 1) nrm      a = (1, 2 (k k - 1) nrm, (1 - d k + k k) nrm)
 * -- the bilinear transform with prewarping, the RBJ cookbook's low-pass / high-pass with alpha = sin(w0) / (2 q) -- then the same
 * cold-start recurrence, buffers and block semantics as sig_biquad_coldstart (the same kernel source).
 * resonance: f64 (resonance_blocks, voices | 1) contiguous rows of q, resonance_blocks in {1, nblocks} like cutoff_blocks (either
 * control may be per block on its own: a swept cutoff, a swept q), resonance_stride 0 / 1; NULL: unplugged = 1/sqrt2, the damping is
 * sqrt2 itself and the call computes what sig_biquad_coldstart computes.  A q that is 0, negative, NaN or +-inf gives NaN rows for
 * that voice (in that block) and sets SIG_STATUS_BAD_RESONANCE, next to SIG_STATUS_BAD_CUTOFF for the cutoff; voices past `voices`
 * (padding lanes) never set either.  type: SIG_FILT_LOWPASS | SIG_FILT_HIGHPASS.  Argument errors: hipErrorInvalidValue, nothing launched. */
int sig_biquad_coldstart_q(int type, int32_t rate, int64_t position,
                           int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                           const double* cutoff, int32_t cutoff_stride, int32_t cutoff_blocks,
                           const double* resonance, int32_t resonance_stride, int32_t resonance_blocks,
                           const void* in, int64_t in_ld, int64_t in_history,
                           void* out, int64_t out_ld, int32_t dtype,
                           int32_t* status, void* stream);

/* sig_biquad_coldstart_q for the RBJ equaliser biquads of chain/ext.py (ResonantBandPass, Notch, AllPass, Peaking, LowShelf,
 * HighShelf; build-defined): three free numerator taps and, for the last three, a gain control.  Per voice and block, in f64:
 *   wn, k and d = 1 / q as sig_biquad_coldstart_q;  A = exp(gain ln(10) / 40);  g = sqrt(A) d;  sos = [b nrm, 1, a1 nrm, a2 nrm]
 *   EQ_BANDPASS  b = (d k, 0, -d k)                                   a1 = 2 (k k - 1), a2 = 1 - d k + k k, 1 / nrm = 1 + d k + k k
 *   EQ_NOTCH     b = (1 + k k, 2 (k k - 1), 1 + k k)                  a and nrm as EQ_BANDPASS
 *   EQ_ALLPASS   b = (1 - d k + k k, 2 (k k - 1), 1 + d k + k k)      a and nrm as EQ_BANDPASS
 *   EQ_PEAKING   b = (1 + d A k + k k, 2 (k k - 1), 1 - d A k + k k)  a1 = 2 (k k - 1), a2 = 1 - (d / A) k + k k, 1 / nrm = 1 + (d / A) k + k k
 *   EQ_LOWSHELF  b = A (1 + g k + A k k, 2 (A k k - 1), 1 - g k + A k k)   a1 = 2 (k k - A), a2 = A - g k + k k, 1 / nrm = A + g k + k k
 *   EQ_HIGHSHELF b = A (A + g k + k k, 2 (k k - A), A - g k + k k)         a1 = 2 (A k k - 1), a2 = 1 - g k + A k k, 1 / nrm = 1 + g k + A k k
 * (the cookbook's BPF with a constant 0 dB peak, notch, APF, peakingEQ, lowShelf, highShelf), then the general transposed direct
 * form II  y = b0 x + z0;  z0 = b1 x - a1 y + z1;  z1 = b2 x - a2 y  from zero state over [<= context rows | block], buffers and block
 * semantics as sig_biquad_coldstart.  resonance and gain: f64 (blocks, voices | 1) rows like sig_biquad_coldstart_q's resonance, each
 * per block on its own; resonance NULL: unplugged = 1/sqrt2; gain (dB) NULL: unplugged = 0 dB; gain is not read for the first three
 * types (its stride and row count are still checked).  A q that is not finite and > 0 sets SIG_STATUS_BAD_RESONANCE, a gain that is
 * not finite SIG_STATUS_BAD_GAIN, a cutoff outside (0, rate / 2) SIG_STATUS_BAD_CUTOFF; that voice's rows (of that block) are NaN;
 * voices past `voices` never set a bit.  type: SIG_FILT_EQ_BANDPASS .. SIG_FILT_EQ_HIGHSHELF.  Argument errors:
 * hipErrorInvalidValue, nothing launched. */
int sig_biquad_coldstart_eq(int type, int32_t rate, int64_t position,
                            int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                            const double* cutoff, int32_t cutoff_stride, int32_t cutoff_blocks,
                            const double* resonance, int32_t resonance_stride, int32_t resonance_blocks,
                            const double* gain, int32_t gain_stride, int32_t gain_blocks,
                            const void* in, int64_t in_ld, int64_t in_history,
                            void* out, int64_t out_ld, int32_t dtype,
                            int32_t* status, void* stream);

/* The 4-pole ladder low-pass of chain/ext.py Ladder (build-defined: every other filter here is a linear biquad): four trapezoidal
 * one-pole low-passes in series, the resonance k fed back around all four with the zero-delay loop solved in closed form, a tanh
 * saturator of drive d at the loop's summing point.  Per voice and block, in f64, states s1..s4 = 0 at the window's first row:
 *   wn = clip(cutoff / (rate / 2), 0, 1);  g = tan(pi wn / 2);  G = g / (1 + g);  H = 1 - G
 *   k = clip(resonance, 0, 4);  d = max(drive, 0);  c = 1 / (1 + k ((G G) (G G)))
 *   per row:  S = H (((s1 G + s2) G + s3) G + s4);  u = (x - k S) c;  if d > 0: u = tanh(d u) / d
 *             for j = 1..4:  v = (u - s_j) G;  y_j = v + s_j;  s_j = y_j + v;  u = y_j
 *             out = y_poles
 * (tests/ladder_reference.py restates it), with the buffers, the window [<= context rows | block] and the block semantics of
 * sig_biquad_coldstart.  cutoff, resonance, drive: f64 (blocks, voices | 1) contiguous rows, blocks in {1, nblocks} each on its
 * own, stride 0 / 1; resonance or drive NULL: unplugged = 0 (no feedback; a linear loop -- a NULL drive launches a kernel without
 * tanh; their strides and row counts are still checked).  A cutoff outside (0, rate / 2) or NaN sets SIG_STATUS_BAD_CUTOFF, a k that
 * is NaN or +-inf SIG_STATUS_BAD_RESONANCE, and that voice's rows (of that block) are NaN; a drive that is NaN or +inf gives NaN rows
 * and no status bit; voices past `voices` never set a bit.  poles in 1 .. 4: the output tap, 6 / 12 / 18 / 24 dB per octave, one for
 * the launch.  No filter type argument: the node's type is SIG_FILT_LADDER, which no other entry accepts.  Argument errors:
 * hipErrorInvalidValue, nothing launched; a launch with nothing to render is a success. */
int sig_ladder_coldstart(int32_t rate, int64_t position,
                         int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                         const double* cutoff, int32_t cutoff_stride, int32_t cutoff_blocks,
                         const double* resonance, int32_t resonance_stride, int32_t resonance_blocks,
                         const double* drive, int32_t drive_stride, int32_t drive_blocks,
                         int32_t poles,
                         const void* in, int64_t in_ld, int64_t in_history,
                         void* out, int64_t out_ld, int32_t dtype,
                         int32_t* status, void* stream);

/* sig_biquad_coldstart whose stored rows are multiplied by a per-voice ADSR envelope evaluated at the row's
 * time (f32 buffers): RingMod(Filter(x), ADSR) -- fx.py:43-46 over fx.py:85-121 and the envelope of sig_adsr --
 * without the envelope store and the extra read/write pass.  adsr_params / adsr_strides as in sig_adsr. */
int sig_biquad_coldstart_env(int type, int32_t rate, int64_t position,
                             int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                             const double* cutoff, int32_t cutoff_stride, int32_t cutoff_blocks,
                             const double* const* adsr_params, const int32_t* adsr_strides,
                             const float* in, int64_t in_ld, int64_t in_history,
                             float* out, int64_t out_ld, int32_t* status, void* stream);

/* Filter [x envelope] summed straight into the bus: out[n,c] = sum_v bus_gains[c,v] * env[n,v] * Filter(in)[n,v]
 * -- SumBus(Filter(x)) or SumBus(RingMod(Filter(x), ADSR)) (fx.py:85-121, fx.py:43-46, the build-defined bus) in
 * one pass over `in`; nothing per-voice is written.  adsr_params == NULL: no envelope.  bus_gains == NULL:
 * bus_channels == 1, plain sum.  `workspace`: device, at least sig_fused_voice_bus_workspace(voices, rows,
 * bus_channels) bytes (per-voice-tile f64 partials, added in a fixed order by a second launch).  Buffers as in
 * sig_biquad_coldstart (float32 only). */
int sig_biquad_coldstart_bus(int type, int32_t rate, int64_t position,
                             int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                             const double* cutoff, int32_t cutoff_stride, int32_t cutoff_blocks,
                             const double* const* adsr_params, const int32_t* adsr_strides,
                             const float* in, int64_t in_ld, int64_t in_history,
                             const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                             double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream);

/* BandPass / BandStop done right (the reference's DoubleCritFilter raises TypeError at
 * fx.py:99, its intent being butter(N=2, Wn=[low, high], btype='bp'|'bs', output='sos') + sosfilt):
 * two biquad sections in series, designed in closed form per voice, same cold-start block semantics and
 * buffer conventions as sig_biquad_coldstart.  low/high: f64 rows (1,V)|(1,1).
 * Pinned against scipy.signal.butter + sosfilt (the reference itself has no working output to compare). */
int sig_band_coldstart(int type, int32_t rate, int64_t position,
                       int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                       const double* low, int32_t low_stride, const double* high, int32_t high_stride,
                       const void* in, int64_t in_ld, int64_t in_history,
                       void* out, int64_t out_ld, int32_t dtype,
                       int32_t* status, void* stream);
/* sig_band_coldstart with per-block bands (a swept BandPass / BandStop): param_blocks is 1 (the rows hold for
 * every block) or nblocks (row b of low / high, each (nblocks, V)|(nblocks, 1) contiguous, is block b's band).
 * A bad band in block b (low >= high, or outside (0, rate/2)) is NaN for that voice in that block only and sets
 * SIG_STATUS_BAD_CUTOFF. */
int sig_band_coldstart_blocks(int type, int32_t rate, int64_t position,
                              int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                              const double* low, int32_t low_stride, const double* high, int32_t high_stride,
                              int32_t param_blocks, const void* in, int64_t in_ld, int64_t in_history,
                              void* out, int64_t out_ld, int32_t dtype,
                              int32_t* status, void* stream);

/* One operand of an element-wise effect.  row_stride / col_stride are in elements; 0 broadcasts
 * that axis (numpy broadcasting of (1,V), (N,1), (1,1) replies). */
typedef struct sig_operand {
    const void* ptr;
    int64_t row_stride;
    int32_t col_stride;
    int32_t dtype;      /* SIG_F32 or SIG_F64 */
    int32_t row_div;    /* > 1: output row r reads operand row r / row_div (a block-rate operand that changes per
                           block in a batched launch: row_div = block_frames); 0 or 1: operand row = r */
    int32_t reserved;
} sig_operand;

/* Replaces Gain/Mix/RingMod/Amp._eval (fx.py:35-60), arithmetic in f64:
 *   GAIN    out = a * b                       (b = right at block rate)
 *   MIX     out = c * a + (1 - c) * b         (c = mix at block rate)
 *   RINGMOD out = a * b
 *   AMP     out = copysign(a ** b, a)         (NaN for a < 0 with fractional b, like numpy) */
int sig_elementwise(int op, int64_t rows, int32_t cols,
                    const sig_operand* a, const sig_operand* b, const sig_operand* c,
                    void* out, int64_t out_ld, int32_t out_dtype, void* stream);

/* Build-defined sum bus (the reference's Flatten/FlattenUnit crash, shape.py:32-41):
 *   gains == NULL : out[n,0] = sum_v x[n,v]                          (bus_channels must be 1)
 *   gains (C,V)   : out[n,c] = sum_v gains[c*gains_ld + v] * x[n,v]
 * f64 accumulation, fixed summation order (lane-strided, then a butterfly), deterministic. */
int sig_sum_bus(int64_t rows, int32_t voices, const void* x, int64_t x_ld, int32_t x_dtype,
                const double* gains, int64_t gains_ld, int32_t bus_channels,
                void* out, int64_t out_ld, int32_t out_dtype, void* stream);

/* Replaces White._eval (noise.py:22-23: np.random.rand(frames, channels), uniform [0,1), global
 * unseeded RNG -- not reproducible, so parity is statistical only).  Here the value of sample
 * (position + n, channel) is a counter-based hash of (seed, frame, channel): position-pure and
 * reproducible; 24 random mantissa bits, u = k * 2^-24, k in [0, 2^24). */
int sig_white_noise(uint64_t seed, int64_t position, int64_t rows, int32_t channels,
                    void* out, int32_t out_dtype, int64_t out_ld, void* stream);

/* Build-defined ADSR envelope bank (the reference has only a dead sketch, sig.py:89-100):
 * position-pure piecewise-linear envelope per voice at frame rate; definition in
 * oracle/chain_ref.py:adsr.  params[6] = device pointers to the f64 rows
 * {attack, decay, sustain, release, gate_on, gate_off} (seconds; sustain is a level), strides[6]
 * their 0/1 strides.  `params` and `strides` themselves are HOST arrays. */
int sig_adsr(int64_t position, int32_t rate, int64_t rows, int32_t voices,
             const double* const* params, const int32_t* strides,
             void* out, int32_t out_dtype, int64_t out_ld, void* stream);

/* out = ADSR envelope * x in one pass: the RingMod(x, ADSR) pair (fx.py:43-46 over the envelope of sig_adsr) without
 * storing the envelope -- 8 B per voice-sample instead of 16.  f32 in / f32 out, product formed in f64. */
int sig_adsr_apply(int64_t position, int32_t rate, int64_t rows, int32_t voices,
                   const double* const* params, const int32_t* strides,
                   const float* x, int64_t x_ld, float* out, int64_t out_ld, void* stream);

/* Build-defined dense mix matrix (BASELINE config 5), f32 in/out, exact-f32 MFMA
 * (v_mfma_f32_32x32x2_f32):  out[n, 64g:64g+64] = x[n, 64g:64g+64] @ matrix,  matrix (64,64)
 * row-major contiguous, voices % 64 == 0, x 16-byte aligned with x_ld % 4 == 0. */
int sig_mix_matrix(int64_t rows, int32_t voices, const float* x, int64_t x_ld,
                   const float* matrix, float* out, int64_t out_ld, void* stream);

/* Fused voice chain, chosen by the batched engine when the intermediate node outputs have no other
 * consumer:  out = [gain *] Filter(Osc)  for `nblocks` cold-started blocks, i.e. sig_osc_bank ->
 * sig_biquad_coldstart -> sig_elementwise(GAIN) without the oscillator / filter stores
 * (osc.py:26-62 + fx.py:85-121 + fx.py:51-52).  Context rows are recomputed from the position-pure
 * oscillator.  f32 store; gain == NULL skips the gain stage; cutoff is one (1,V)|(1,1) row. */
int sig_fused_osc_biquad(int osc_kind, int filt_type, int32_t rate, int64_t position,
                         int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                         const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                         const double* cutoff, int32_t cutoff_stride,
                         const double* gain, int32_t gain_stride,
                         float* out, int64_t out_ld, int32_t* status, void* stream);

/* The fused chain / chain + bus with cutoff and gain read PER BLOCK: the reference reads a control port once per block,
 * at the block's position (forward_at_block_rate, chain/__init__.py:305-306), so an LFO on a cutoff or a tremolo gives
 * every block its own filter design and gain.  cutoff_rows / gain_rows: 1 (one row for the launch) or nblocks (row b
 * for block b, rows contiguous: row b of a per-voice parameter starts at + b * voices, of a broadcast one at + b).
 * The row-by-row span walker (the next block's warm-up chain runs with the next block's design) -- except a Sine voice
 * under a bus (sig_fused_voice_bus_rows), which keeps the closed form of sig_fused_voice_bus: the filter, its response at the
 * voice's frequency, T_c and the decay bound derived per (block, voice) inside the launch, the steady-state recurrence re-seeded
 * at every block's first row.  gain may be NULL; bus_channels 1 or 2.  hertz and phase stay one row here (sig_fused_*_fm below takes rows for them too). */
int sig_fused_osc_biquad_rows(int osc_kind, int filt_type, int32_t rate, int64_t position,
                              int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                              const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                              const double* cutoff, int32_t cutoff_stride, int32_t cutoff_rows,
                              const double* gain, int32_t gain_stride, int32_t gain_rows,
                              float* out, int64_t out_ld, int32_t* status, void* stream);
int sig_fused_voice_bus_rows(int osc_kind, int filt_type, int32_t rate, int64_t position,
                             int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                             const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                             const double* cutoff, int32_t cutoff_stride, int32_t cutoff_rows,
                             const double* gain, int32_t gain_stride, int32_t gain_rows,
                             const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                             double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream);

/* ... and with hertz and phase read per block as well: block-rate frequency / phase modulation (Osc._eval reads both
 * ports with forward_at_block_rate, osc.py:28-30).  hertz_rows / phase_rows: 1 or nblocks, rows laid out like cutoff's.
 * The reference's oscillators keep their previous block (BlockCachingEmitter, chain/__init__.py:424-442), so the context
 * rows a filter sees in front of block b are block b - 1's samples (block_frames >= context: with shorter blocks the
 * reference answers the context request as a block of its own -- not this entry point's semantics, callers keep such graphs
 * on the per-node path), made with parameter row b - 1: the walker's
 * warm-up chain already runs on the samples at hand.  For the launch's first block that row is *_hist (one (1,V)|(1,1)
 * row, same stride; non-NULL marks the parameter as modulated -- also in a one-block launch, whose single row still has a
 * different row in front; required when the matching *_rows > 1): the previous batch's last row on a continuing stream, the
 * controls evaluated at position - min(context, position) on a fresh graph.  Sine's incremental phase is re-seeded at every
 * block's first row with that block's hertz / phase. */
int sig_fused_osc_biquad_fm(int osc_kind, int filt_type, int32_t rate, int64_t position,
                            int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                            const double* hertz, int32_t hertz_stride, int32_t hertz_rows, const double* hertz_hist,
                            const double* phase, int32_t phase_stride, int32_t phase_rows, const double* phase_hist,
                            const double* cutoff, int32_t cutoff_stride, int32_t cutoff_rows,
                            const double* gain, int32_t gain_stride, int32_t gain_rows,
                            float* out, int64_t out_ld, int32_t* status, void* stream);
int sig_fused_voice_bus_fm(int osc_kind, int filt_type, int32_t rate, int64_t position,
                           int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                           const double* hertz, int32_t hertz_stride, int32_t hertz_rows, const double* hertz_hist,
                           const double* phase, int32_t phase_stride, int32_t phase_rows, const double* phase_hist,
                           const double* cutoff, int32_t cutoff_stride, int32_t cutoff_rows,
                           const double* gain, int32_t gain_stride, int32_t gain_rows,
                           const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                           double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream);

/* The same two entry points for a filter that reads TWO oscillators through an element-wise node: pair_op 1 =
 * Mix(A, B, mix): mix * A + (1 - mix) * B with mix one (1,V)|(1,1) row (Mix._eval, fx.py:35-40); pair_op 2 =
 * RingMod(A, B): A * B (fx.py:43-46; mix ignored, may be NULL).  A = (osc_kind, hertz, phase), B = (osc2_kind, hertz2,
 * phase2); both evaluated per row in the walker (B always with the exact per-row phase), nothing per-voice stored. */
int sig_fused_osc_pair_biquad(int osc_kind, int osc2_kind, int pair_op, int filt_type, int32_t rate, int64_t position,
                              int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                              const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                              const double* hertz2, int32_t hertz2_stride, const double* phase2, int32_t phase2_stride,
                              const double* mix, int32_t mix_stride,
                              const double* cutoff, int32_t cutoff_stride, int32_t cutoff_rows,
                              const double* gain, int32_t gain_stride, int32_t gain_rows,
                              float* out, int64_t out_ld, int32_t* status, void* stream);
int sig_fused_voice_pair_bus(int osc_kind, int osc2_kind, int pair_op, int filt_type, int32_t rate, int64_t position,
                             int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                             const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                             const double* hertz2, int32_t hertz2_stride, const double* phase2, int32_t phase2_stride,
                             const double* mix, int32_t mix_stride,
                             const double* cutoff, int32_t cutoff_stride, int32_t cutoff_rows,
                             const double* gain, int32_t gain_stride, int32_t gain_rows,
                             const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                             double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream);

/* hipGraph support for the launch-bound latency loop (one block per pull): the same chain with the frame
 * position read from DEVICE memory, plus a one-thread kernel that advances it, so a captured graph
 * [chain(position_dev) -> bus -> position_dev += block_frames*nblocks] replays unchanged block after block. */
int sig_fused_osc_biquad_devpos(int osc_kind, int filt_type, int32_t rate, const int64_t* position_dev,
                                int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                                const double* cutoff, int32_t cutoff_stride,
                                const double* gain, int32_t gain_stride,
                                float* out, int64_t out_ld, int32_t* status, void* stream);
int sig_advance_position(int64_t* position_dev, int64_t delta, void* stream);

/* A block-rate control subgraph as one launch.  The reference reads a control port once per block, at the block's position
 * (BoundPort.forward_at_block_rate, chain/__init__.py:305-306); an LFO sweep or a tremolo is an oscillator evaluated at one
 * frame per block (Osc._eval, osc.py:26-62) combined by element-wise nodes (fx.py:35-60).  `program` (device memory, n_ins <=
 * SIG_CTL_MAX_INS = SIG_CTL_MAX_REGS: one register per instruction, the register file is sized by n_ins; a longer program is refused with
 * hipErrorInvalidValue) is that subgraph in evaluation order over registers dst < n_ins; thread (b, v) runs it for
 * block b (frame position + b * step) at column v < cols and writes register outs[k].reg to outs[k].out[b * outs[k].cols + v]
 * for v < outs[k].cols.  `position` may lie before `min_position` (even be negative): blocks whose frame position + b * step is below
 * min_position are evaluated AT min_position (the virtual blocks in front of short blocks read their controls at max(p - context, 0);
 * what feeds the last filter of a short block read them at an earlier block's position, never before the stream's second block).  A register index of -1 reads 0.  Same expressions as sig_osc_bank (f64 store) and sig_elementwise,
 * so the same bits as the node-by-node evaluation.
 *
 * Two more ops run only through sig_control_program_windowed (the same arguments; sig_control_program keeps its kernel, and a
 * program holding one of them must not be given to it):
 *  - SIG_CTL_NOISE: White at block rate, `row` = the seed (a uint64 in the pointer field), column v = channel v: the same hash
 *    and scaling as sig_white_noise.
 *  - SIG_CTL_FILTER: a LowPass / HighPass read at one frame (fx.py:85-106 with forward_with_context): kind = SIG_FILT_LOWPASS |
 *    SIG_FILT_HIGHPASS, a = its input register, b = its cutoff register (block rate), `row` = an int32 status word (or NULL)
 *    that collects SIG_STATUS_BAD_CUTOFF.  The instructions that feed `a` are WINDOW-RATE (`reserved` = 1; they form the
 *    contiguous run right in front of the filter and feed nothing else): for the block evaluated at frame p they run for the
 *    h = min(100, p) history rows p - h + j, every result rounded to float32 when h > 1 (a reply of more than one row is
 *    float32 audio), and once more at p in float64; a cold-started Butterworth biquad (sig_biquad.h, transposed direct form
 *    II) steps over the h + 1 rows and its last output is the filter's register.  Window-rate operands other than window-rate
 *    registers must be block-invariant (ROW).  A one-column filter spreads its rows over the workgroup's threads (thread j
 *    evaluates row j); a wider one walks them per column.
 *
 * Two more run only through sig_control_program_envelope (the same arguments again, a kernel variant of its own that also
 * runs everything above, so the other two entries keep their kernels):
 *  - SIG_CTL_ADSR: the ADSR envelope (sig_adsr) read at one frame: for the block evaluated at frame p (after the min_position
 *    clamp; the front position likewise) its value is the envelope's level at t = (double)p / rate in float64 -- the operations of
 *    sig_adsr with rows = 1 and a float64 output at that position, so the same bits.  Its six parameters are registers (block
 *    rate: a ROW or any computed register, column v or column 0 of a one-column one): a, b, c = attack, decay, sustain here and
 *  - SIG_CTL_ADSRARGS: a, b, c = release, gate_on, gate_off in a carrier instruction IMMEDIATELY IN FRONT of the SIG_CTL_ADSR
 *    (an instruction has three operand registers).  The carrier computes nothing and nothing else reads its register; it has
 *    the ADSR's `cols` and `reserved`.  `cols` = the broadcast of the six widths.  With `reserved` = 1 the pair is part of a
 *    filter's window run (a smoothed envelope): evaluated per window row and rounded to float32 there like every window-rate
 *    result; its parameters are then block-invariant rows.  A pair that is not formed like this (an ADSR without its carrier
 *    in front, a carrier without its ADSR behind) is refused with hipErrorInvalidValue where the library can read the structure
 *    -- sig_control_program_attach's description, which sig_control_program_attached then runs; a `program` in device memory
 *    it cannot read, and there an ADSR without its carrier reads release = gate_on = gate_off = 0. */
enum { SIG_CTL_ROW = 0, SIG_CTL_OSC = 1, SIG_CTL_GAIN = 2, SIG_CTL_MIX = 3, SIG_CTL_RINGMOD = 4, SIG_CTL_AMP = 5,
       SIG_CTL_NOISE = 6, SIG_CTL_FILTER = 7, SIG_CTL_ADSRARGS = 8, SIG_CTL_ADSR = 9 };
enum { SIG_CTL_MAX_REGS = 48, SIG_CTL_MAX_INS = 48 };
typedef struct {
    int32_t op;              /* SIG_CTL_* */
    int32_t kind;            /* OSC: SIG_OSC_* */
    int32_t a, b, c;         /* operand registers.  OSC: a = hertz, b = phase; GAIN / RINGMOD / AMP: a, b; MIX: a, b, c = mix;
                                ADSR: attack, decay, sustain; ADSRARGS: release, gate_on, gate_off */
    int32_t dst;             /* result register */
    int32_t stride, rows;    /* ROW: a (rows, cols) float64 array, rows 1 | nblocks, rows contiguous, element v * stride (cols 1: stride 0) */
    int32_t cols;            /* EVERY instruction: columns of its result (1: evaluated once per block; the broadcast of its operands' widths otherwise) */
    int32_t reserved;        /* 1: a window-rate instruction (in front of a SIG_CTL_FILTER); 0 otherwise */
    const double* row;       /* ROW: the rows; NOISE: the seed; FILTER: the status word */
} sig_ctl_ins;
typedef struct { int32_t reg; int32_t cols; double* out; double* front; } sig_ctl_out;   /* out: (nblocks, cols) float64, contiguous; front: (1, cols) or NULL */
/* front_position >= 0: the program is evaluated once more, at that frame position, into the outputs' `front` rows (the
 * controls of the block in front of the batch -- sig_fused_*_fm's *_hist -- without a launch of their own); -1: not.  The front
 * evaluation is not clamped at min_position, it runs with nblocks == 0 too (the front rows alone), an output whose `front` is
 * NULL is skipped, and a ROW with rows == nblocks is read at its row 0 there (there is no block in front of the first: a program
 * whose front row matters keeps such rows out of it).  A ROW with rows == nblocks is (nblocks, cols) contiguous: block b reads
 * element b * cols + v * stride (cols 1, stride 0: element b). */
int sig_control_program(int32_t rate, int64_t position, int32_t step, int32_t nblocks, int32_t cols, int64_t front_position,
                        int64_t min_position,
                        const sig_ctl_ins* program, int32_t n_ins, const sig_ctl_out* outs, int32_t n_outs, void* stream);
/* sig_control_program for programs with SIG_CTL_NOISE / SIG_CTL_FILTER instructions (a kernel variant of its own, so the
 * programs without them keep their registers) */
int sig_control_program_windowed(int32_t rate, int64_t position, int32_t step, int32_t nblocks, int32_t cols, int64_t front_position,
                                 int64_t min_position,
                                 const sig_ctl_ins* program, int32_t n_ins, const sig_ctl_out* outs, int32_t n_outs, void* stream);
/* sig_control_program_windowed for programs that also hold SIG_CTL_ADSRARGS / SIG_CTL_ADSR pairs (a third kernel variant, so the
 * other two keep their code and registers) */
int sig_control_program_envelope(int32_t rate, int64_t position, int32_t step, int32_t nblocks, int32_t cols, int64_t front_position,
                                 int64_t min_position,
                                 const sig_ctl_ins* program, int32_t n_ins, const sig_ctl_out* outs, int32_t n_outs, void* stream);

/* SPECIALISED control programs: signals_amd/csrc/control_program.hip built as a gfx950 code object for one program STRUCTURE
 * (macros SIG_CTL_STATIC_INS = {{op, kind, a, b, c, dst, wide}, ...} in evaluation order -- wide: bit 0 = more than one
 * column, bit 1 = window-rate and SIG_CTL_STATIC_OUTS = {{reg, wide},
 * ...}; `hipcc --genco`, signals_amd/specialise.py): the registers are VGPRs instead of an LDS file behind an interpretive loop.
 * `description` = [n_ins, n_outs, the seven words per instruction, the two per output]; the image must describe itself the same
 * way (its sig_ctl_specialised_info kernel) or hipErrorInvalidImage.  A set-up call (allocates, launches, synchronises); the
 * handle (>= 1) is valid for the life of the process.  sig_control_program_attached = sig_control_program through that kernel:
 * the CALLER vouches that `program` / `outs` have the structure the handle was built for (they are device memory, the library
 * cannot look); row pointers, strides and output pointers are read from them as usual.  The same values, bit for bit. */
int sig_control_program_attach(const int32_t* description, int32_t n_words, const void* image, int32_t* handle);
int sig_control_program_attached(int32_t handle, int32_t rate, int64_t position, int32_t step, int32_t nblocks, int32_t cols,
                                 int64_t front_position, int64_t min_position,
                                 const sig_ctl_ins* program, int32_t n_ins, const sig_ctl_out* outs, int32_t n_outs, void* stream);

/* Fused voice chain + dense mix matrix:  out[n, 64g : 64g+64] = ([gain *] Filter(Osc))[n, 64g : 64g+64] @ matrix
 * -- Osc._eval (chain/osc.py:26-62), CritFilter._filter (chain/fx.py:85-121), Gain._eval (chain/fx.py:49-52) and the
 * build-defined MixMatrix, i.e. the chain of sig_fused_osc_biquad feeding sig_mix_matrix (BASELINE config 5) without the per-voice rows going
 * through HBM: every 32 rows of a 64-voice group are staged as float32 in LDS and multiplied on the matrix cores.  The default
 * sink contracts each float32 operand as the exact sum of three bfloat16 (six v_mfma_f32_32x32x16_bf16 products per k-block,
 * float32 accumulators, the three cross terms below 2^-26 of a product dropped; sig_mix_tile.h): WITHIN A FEW float32 ULP of
 * sig_mix_matrix over sig_fused_osc_biquad's output (measured 4-7 ulp of the rows' scale between the two, each 2-5 ulp from
 * the f64 product), not bit for bit.  sig_fused_set_tuning(closed_form = 3) selects v_mfma_f32_32x32x2_f32 (the instruction
 * of sig_mix_matrix) instead.  Non-finite rows: the split forms x - bf16(x), so an Inf sample becomes NaN in the mixed row where
 * the float32 instruction keeps Inf (either way the row is unusable and a rejected design also sets the status bit); residual
 * words below bfloat16's range (|x| < ~1e-33 after two splits) flush to zero, an absolute error below 1e-35.
 * voices % 64 == 0; matrix (64, 64) float32 row-major on the device. */
int sig_fused_osc_biquad_mix(int osc_kind, int filt_type, int32_t rate, int64_t position,
                             int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                             const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                             const double* cutoff, int32_t cutoff_stride,
                             const double* gain, int32_t gain_stride,
                             const float* matrix, float* out, int64_t out_ld, int32_t* status, void* stream);

/* Fused voice chain + sum bus:  out[n,c] = sum_v bus_gains[c,v] * ([gain[v] *] Filter(Osc)[n,v])
 * (bus_gains == NULL: bus_channels == 1, plain sum).  Nothing per-voice touches HBM.  Launches inside: the chain
 * kernel writes per-voice-tile f64 partials into `workspace` (device, at least
 * sig_fused_voice_bus_workspace(voices, rows, bus_channels) bytes, rows = block_frames*nblocks), a second kernel adds
 * the tiles in a fixed order and rounds to f32; for a Sine oscillator a one-thread-per-voice kernel first derives the
 * constants of the closed form (steady-state sinusoid + homogeneous transient per cold-started block; voices it does
 * not cover are walked row by row in the same launch) into the tail of the workspace.  Deterministic; no atomics. */
int64_t sig_fused_voice_bus_workspace(int32_t voices, int64_t rows, int32_t bus_channels);
/* sig_fused_voice_bus restricted to the row-by-row span walker (never the Sine closed form).  The closed form, like
 * the walker's incremental Sine phase, holds while |t| = |frame / rate * hertz + phase| < 2^26 cycles (past that the
 * reference's own rounding of t, which neither reproduces, approaches the 1e-6 bar): a wave with a voice beyond it is
 * done inside the closed-form launch by a plain per-row fallback that is correct but ~40x slower, fine for a few
 * waves.  A caller that knows a whole launch lies beyond the limit (max |hertz| and the position are host-side
 * knowledge) calls this entry instead: the walker's exact-phase path runs at about a third of the closed form's rate. */
int sig_fused_voice_bus_walk(int osc_kind, int filt_type, int32_t rate, int64_t position,
                             int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                             const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                             const double* cutoff, int32_t cutoff_stride,
                             const double* gain, int32_t gain_stride,
                             const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                             double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream);
/* sig_fused_voice_bus with the per-voice constants of its Sine closed form (filter design, H(e^{j theta}), the
 * block-start matrices: ~5 us of kernel time per call) kept by the caller across calls: `consts` is a device buffer of
 * sig_fused_voice_consts_size(voices) bytes; consts_ready == 0 fills it (and uses it), consts_ready != 0 skips that.
 * The buffer stays valid while hertz, cutoff, gain (their values), filt_type, rate, context, voices and
 * min(context, position) are unchanged; the caller vouches for that.  Other waveforms ignore it. */
int64_t sig_fused_voice_consts_size(int32_t voices);
int sig_fused_voice_bus_prepared(int osc_kind, int filt_type, int32_t rate, int64_t position,
                                 int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                 const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                                 const double* cutoff, int32_t cutoff_stride,
                                 const double* gain, int32_t gain_stride,
                                 const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                                 double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream,
                                 double* consts, int32_t consts_ready);

/* sig_fused_voice_bus_prepared (walk == 0) / sig_fused_voice_bus_walk (walk != 0) with every argument that does not change from
 * batch to batch in a caller-held block: what a host binding with a per-argument cost (ctypes: ~5 us for 26 arguments, a
 * quarter of a 256-block batch) calls per batch.  `consts` may be NULL when only the walker is ever asked for. */
typedef struct {
    int32_t osc_kind, filt_type, rate, block_frames, nblocks, context, voices;
    int32_t hertz_stride, phase_stride, cutoff_stride, gain_stride, bus_channels;
    const double* hertz; const double* phase; const double* cutoff; const double* gain; const double* bus_gains;
    int64_t bus_gains_ld, out_ld;
    double* workspace; int32_t* status; double* consts;
} sig_fused_voice_bus_call;
int sig_fused_voice_bus_bound(const sig_fused_voice_bus_call* call, int64_t position, float* out, int32_t consts_ready,
                              int32_t walk, void* stream);

/* Fused filter cascade + envelope + sum bus (BASELINE config 3's whole graph in one launch):
 *   out[n,c] = sum_v bus_gains[c,v] * [gain[v] *] [ADSR_v(n) *] Filter2(Filter1(Osc))[n,v]
 * i.e. Osc._eval (chain/osc.py:26-62), two CritFilter._filter (chain/fx.py:85-121) in series with the reference's
 * block-cache semantics between them (chain/__init__.py:431-442, SURVEY.md 8a A9: the outer filter's 100 context rows
 * are the LAST 100 ROWS OF THE INNER FILTER'S PREVIOUS BLOCK, which was cold-started 100 rows before that block),
 * RingMod with the build-defined ADSR (adsr_params == NULL: none; layout as sig_adsr) and the build-defined SumBus.
 * `first_history_start`: the frame at which the block in front of `position` started when the stream was rendered
 * sequentially -- position - previous_block_frames on a continuing stream, position - min(context, position) on a
 * fresh graph (the reference then renders [position - 100, position) as a block of its own), == position exactly when
 * position == 0.  Requires block_frames > context and block_frames % (16 / bus_channels) == 0; cutoffs are one
 * (1,V)|(1,1) row each.  `workspace`: sig_fused_voice_bus_workspace(voices, rows, bus_channels) bytes.
 * Deterministic (fixed summation order, no atomics). */
int sig_fused_cascade_bus(int osc_kind, int filt1_type, int filt2_type, int32_t rate, int64_t position,
                          int64_t first_history_start, int32_t block_frames, int32_t nblocks, int32_t context,
                          int32_t voices,
                          const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                          const double* cutoff1, int32_t cutoff1_stride, const double* cutoff2, int32_t cutoff2_stride,
                          const double* gain, int32_t gain_stride,
                          const double* const* adsr_params, const int32_t* adsr_strides,
                          const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                          double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream);
/* Introspection: voices per lane and consecutive blocks per lane sig_fused_cascade_bus uses (every span of blocks walks
 * one extra block of oscillator + inner filter, the history; bench.py's operation count depends on it). */
int sig_fused_cascade_geometry(int32_t voices, int32_t nblocks, int32_t* voices_per_lane, int32_t* blocks_per_lane);
/* Tuning / test hook (process-wide): force voices per lane (1, 2, 4; 0 = heuristic) and blocks per lane (>= 1; 0 = heuristic;
 * given as its negative: that many, and the voice tiles are added by a second launch instead of inside the kernel). */
int sig_fused_cascade_set_tuning(int32_t voices_per_lane, int32_t blocks_per_lane);

/* Latency mode of the same graph for a Sine oscillator: ONE block per launch, rows x voices parallelism (closed form
 * seeded per 16-row chunk), the voice tiles added and the float32 bus written by the last workgroup to finish -- a
 * single launch per block.  `workspace`: device, sig_latency_voice_bus_workspace(voices, block_frames, bus_channels)
 * bytes, whose last 8 bytes (the arrival counter) must be zero before the FIRST launch; the kernel re-arms it, so
 * launches that share a workspace must be ordered (one stream, or events between streams).
 * position_dev != NULL: the block's position is read from device memory and advanced by block_frames by the same
 * launch (hipGraph replay with no other node); otherwise `position` is used. */
int64_t sig_latency_voice_bus_workspace(int32_t voices, int32_t block_frames, int32_t bus_channels);
int sig_latency_voice_bus(int filt_type, int32_t rate, int64_t position, int64_t* position_dev,
                          int32_t block_frames, int32_t context, int32_t voices,
                          const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                          const double* cutoff, int32_t cutoff_stride,
                          const double* gain, int32_t gain_stride,
                          const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                          double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream);

/* Introspection: the launch geometry the two fused entry points use for this problem size -- voices per lane
 * (1, 2 or 4) and consecutive blocks per lane (the span walker, sig_fused_walk.h).  For measurement tools (the
 * f64 operation count per voice-sample depends on the span) and tests; no device work. */
int sig_fused_geometry(int32_t voices, int32_t block_frames, int32_t nblocks, int32_t context,
                       int32_t* voices_per_lane, int32_t* blocks_per_lane);
/* Introspection, no device work: what sig_fused_voice_bus launches for this problem -- voices per lane (1, 2, 4 or 8),
 * consecutive blocks per lane, and closed_form = 1 when the Sine closed-form kernel (fused_steady_bus_kernel) takes
 * the launch, 0 for the row-by-row span walker (fused_walk_kernel).  bench.py and the tests name the kernel they
 * time / check with it. */
int sig_fused_voice_bus_plan(int osc_kind, int64_t position, int32_t voices, int32_t block_frames, int32_t nblocks,
                             int32_t context, int32_t* voices_per_lane, int32_t* blocks_per_lane, int32_t* closed_form);
/* Tuning / test hook of the fused entry points: force the voices per lane (0 = heuristic), the blocks per lane
 * (0 = heuristic), the Sine closed form (-1 = heuristic, 0 = off, 1 = on, 2 = on with the voice tiles added by a second
 * launch instead of inside the kernel, 3 = on with the MixMatrix sink on the float32 MFMA instead of three-way bfloat16
 * splits) and the latency-mode prefix-scan kernel
 * (-1 = heuristic, 0 = off, 1 = on).  Process-wide, not thread-safe against concurrent launches; the initial values
 * come from SIG_FUSED_VPT / _SPAN / _STEADY / _SCAN, read once. */
int sig_fused_set_tuning(int32_t voices_per_lane, int32_t blocks_per_lane, int32_t closed_form, int32_t scan);
int sig_fused_voice_bus(int osc_kind, int filt_type, int32_t rate, int64_t position,
                        int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                        const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                        const double* cutoff, int32_t cutoff_stride,
                        const double* gain, int32_t gain_stride,
                        const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                        double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream);

/* A whole frame-rate voice graph in ONE launch (voice_program.hip): the general form of the fused entry points above, for
 * the graph shapes none of them covers.  Replaces, for every voice of a graph at once, the bodies of
 *   Osc._eval + _osc (osc.py:26-62), CritFilter._filter / _get_sos for LowPass / HighPass (fx.py:85-121), Gain / Mix / RingMod /
 *   Amp._eval (fx.py:35-60), Fixed._eval as an audio operand (fixed.py:38-39), White._eval (noise.py:22-23), the build-defined
 *   ADSR, and the sink: the rows themselves or the build-defined SumBus
 * together with the block structure between them: every node reads its control ports once per block at the block's position
 * (BoundPort.forward_at_block_rate, chain/__init__.py:305-306); a filter answers a block from zero state over
 * [<= context rows | block] (fx.py:93-105, forward_with_context chain/__init__.py:308-315); the context rows in front of block j
 * are the input's rows of block j - 1 as its block cache holds them (BlockCachingEmitter, chain/__init__.py:431-442), or -- on a
 * fresh graph, and for EVERY block when blocks are shorter than the context -- the input rendered as a block of its own
 * [p - context, p) with its controls read at max(p - context, 0).
 *
 * `program` (HOST memory, copied into the launch): the per-voice graph as straight-line code for an accumulator machine.
 *   OSC    acc = wave_kind(n / rate * hertz[a] + phase[a])         oscillator slot a (hertz / phase rows below)
 *   FILTER acc = filter slot a applied to acc                      (cutoff rows / type below; one slot per filter node)
 *   GAIN   acc = acc * params[a]          AMP  acc = copysign(acc ** params[a], acc)          CONST  acc = params[a]
 *   MUL    acc = temp[a] * acc            MIX  acc = m L + (1 - m) R, m = params[b], (L, R) = c ? (acc, temp[a]) : (temp[a], acc)
 *   SAVE   temp[a] = acc                  LOAD acc = temp[a]
 *   ADSR   acc = envelope level at n / rate (the six rows `adsr`)     NOISE acc = White sample (noise_seed[a], frame n, channel)
 *   BAND   acc = band filter over slots a, a + 1 applied to acc    (BandPass / BandStop: cutoff[a] = low rows, cutoff[a + 1] = high
 *          rows, filter_type both SIG_FILT_BANDPASS or both SIG_FILT_BANDSTOP, one filter_level; a run of band slots pairs up from
 *          its first slot; designed per block like butter(2, [low, high]) and run as its two sections)
 *   OSCPM  acc = wave_kind(n / rate * hertz[a] + phase[a] + params[b] * acc)     oscillator slot a, index = parameter slot b (a
 *          phase-modulation carrier: the modulator's code runs first and leaves its sample in the accumulator; a program with both
 *          BAND and OSCPM is refused, hipErrorInvalidValue: the interpreter is built with either, not both)
 *   OSCTABLE acc = wavetable lookup (sig_osc_bank_table's expression) at n / rate * hertz[a] + phase[a] in table slot b of the
 *          `tables` argument of sig_voice_program_ex, column = params[c] (select rows), c == -1: unplugged = column 0.  The tables
 *          sit in LDS for the whole launch.  m = t - floor(t) is one v_fract_f64 here, like the other fused oscillators: it differs
 *          from the definition only for t in (-2^-54, 0), where it reads the table's last segment at f = 1 - 2^-53 instead of entry 0
 *          (the two agree to one ulp of a table step).  A program that combines OSCTABLE with BAND or OSCPM is refused,
 *          hipErrorInvalidValue; so is one launched without its tables
 *   SHAPE  acc = waveshaper lookup (sig_shaper_table's expression) of the accumulator in table slot b of the `tables` argument,
 *          column = params[c] (select rows), c == -1: unplugged = column 0.  Refused with BAND or OSCPM and without its tables, like
 *          OSCTABLE.  A slot that only SHAPE words read may have any T >= 2; a slot an OSCTABLE word reads is a power of two
 *   FILTERQ acc = resonant filter slot a applied to acc (sig_biquad_coldstart_q's design, the FILTER word's recurrence): the slot's
 *          filter_type is SIG_FILT_RES_LOWPASS | SIG_FILT_RES_HIGHPASS, its cutoff rows as for FILTER, q = params[c] read per block
 *          with the cutoff (the rows of the block the design is for), c == -1: unplugged = 1/sqrt2.  One FILTERQ word per slot;
 *          FILTER words run in the same program (ResonantHighPass -> LowPass is one program).  Refused together with BAND, OSCPM,
 *          OSCTABLE or SHAPE, hipErrorInvalidValue: the interpreter variant with the resonant design has none of them
 *   OSCUNI acc = unison oscillator (sig_osc_bank_unison's expression with the fused waveforms: m = t - floor(t) as one v_fract_f64,
 *          the f64 sine) of kind `kind` on oscillator slot a, over the copies of unison slot b of the `unison` argument of
 *          sig_voice_program_unison (only slot 0 exists, SIG_VP_MAX_UNISON = 1), spread = params[c], c == -1: unplugged = 0.  The
 *          copies travel by value in the launch.  Refused together with BAND, OSCPM, OSCTABLE, SHAPE or FILTERQ,
 *          hipErrorInvalidValue: the interpreter variant with the unison handler has none of them; so is one launched without `unison`
 *   OSCBLEP acc = band-limited oscillator (sig_osc_bank_blep's expression, m = t - floor(t) as one v_fract_f64) of kind `kind` (not
 *          SIG_OSC_SINE) with OSCUNI's operands: oscillator slot a, the copies of unison slot b = 0, spread = params[c], c == -1:
 *          unplugged = 0.  A word of the unison family: it reads the `unison` argument, and is refused wherever OSCUNI is
 *   FILTEREQ acc = equaliser filter slot a applied to acc (sig_biquad_coldstart_eq's design and recurrence): the slot's filter_type
 *          is SIG_FILT_EQ_BANDPASS .. SIG_FILT_EQ_HIGHSHELF, its cutoff rows as for FILTER, q = params[c] and gain (dB) = params[b]
 *          read per block with the cutoff, c == -1: unplugged = 1/sqrt2, b == -1: unplugged = 0 dB (the only word whose b may be -1;
 *          gain is not read for the three types without one).  One FILTEREQ word per slot; FILTER and FILTERQ words run in the same
 *          program.  A word of the resonant family: refused wherever FILTERQ is, and launched by kernels of its own (the resonant and
 *          the mixed variant once more with the general numerator), so that programs without the word run the code they ran before;
 *          sig_voice_program_variant still answers RESONANT or MIXED
 *   OSCSYNC acc = hard-sync oscillator (sig_osc_bank_sync's expression, m = t - floor(t) as one v_fract_f64) of kind `kind`
 *          (SIG_OSC_SAWTOOTH or SIG_OSC_SQUARE) with OSCBLEP's operands -- oscillator slot a, the copies of the `unison` argument,
 *          spread = params[c], c == -1: unplugged = 0 -- and ratio = params[b] read per block, b == -1: unplugged (R = 1).  A word of
 *          the unison family: refused wherever OSCUNI is, and launched by kernels of its own (the band-limited and the mixed variant
 *          once more with this handler), so that programs without the word run the code they ran before; sig_voice_program_variant
 *          still answers BLEP or MIXED.  Refused together with FILTEREQ by every entry (no kernel set has both)
 * The accumulator after the last instruction is the voice's sample of that row.  Rows (sig_vp_rows) are float64 (rows, voices | 1)
 * arrays, col_stride 1 | 0: rows == 1 holds for every block; otherwise rows == control_rows, one row per block:
 *   block_frames >= context:  [the block in front of the first history block | hist_blocks history blocks | nblocks blocks],
 *                             control_rows = hist_blocks + 1 + nblocks
 *   block_frames <  context:  [nblocks virtual blocks (controls read at max(p_b - context, 0)) | nblocks blocks], control_rows = 2 nblocks.
 *                             There the rows a block's LAST filter reads over the block itself are the oldest cached reply of its input that
 *                             contains them (chain/__init__.py:435-442): the reply to the `after` request made m_b = min((context -
 *                             block_frames) / block_frames, blocks_before + b - 1) blocks earlier, at q_b = p_b - m_b block_frames (block 0 of
 *                             a fresh graph: q = p) -- every node in front of the last filter read its controls THERE, so the caller
 *                             evaluates their rows of the second group at q_b, those of the last filter and behind it at p_b.
 *                             `blocks_before`: blocks of this size rendered contiguously in front of the launch since the graph was fresh.
 *                             16 <= block_frames (below that the reference's 16-entry block cache evicts what a block reads), depth <= 2.
 * `depth` = filters in series on the longest path to the sink.  `hist_positions[hist_blocks]` (ascending, < position): where the
 * depth - 1 blocks in front of the launch start -- the previous render's blocks on a continuing stream, the virtual blocks
 * p - context, p - 2 context ... (clipped at 0) on a fresh graph; ignored when block_frames < context (at most two filters in
 * series there).  bus_channels 0: out (nblocks * block_frames, voices) float32; 1 | 2: out (.., bus_channels) = sum over voices of
 * bus_gains[c, v] * sample (bus_gains NULL: mono sum), float64 accumulation in a fixed order; workspace of
 * sig_fused_voice_bus_workspace(voices, rows, bus_channels) bytes.  f64 arithmetic, no float32 rounding between the nodes.
 * A rejected filter design (fx.py:99-102) gives NaN rows and sets SIG_STATUS_BAD_CUTOFF; a FILTERQ slot's q that is not finite and
 * > 0 likewise and sets SIG_STATUS_BAD_RESONANCE, a FILTEREQ slot's gain that is not finite SIG_STATUS_BAD_GAIN (never for a voice past
 * `voices`). */
enum { SIG_VP_OSC = 0, SIG_VP_FILTER = 1, SIG_VP_GAIN = 2, SIG_VP_MUL = 3, SIG_VP_MIX = 4, SIG_VP_SAVE = 5, SIG_VP_LOAD = 6,
       SIG_VP_CONST = 7, SIG_VP_AMP = 8, SIG_VP_ADSR = 9, SIG_VP_NOISE = 10, SIG_VP_BAND = 11, SIG_VP_OSCPM = 12,
       SIG_VP_OSCTABLE = 13, SIG_VP_SHAPE = 14, SIG_VP_FILTERQ = 15, SIG_VP_OSCUNI = 16, SIG_VP_OSCBLEP = 17,
       SIG_VP_FILTEREQ = 18, SIG_VP_OSCSYNC = 19 };
enum { SIG_VP_MAX_TABLES = 2, SIG_VP_MAX_UNISON = 1 };
enum { SIG_VP_MAX_INS = 32, SIG_VP_MAX_OSCS = 4, SIG_VP_MAX_PARAMS = 8, SIG_VP_MAX_FILTERS = 4, SIG_VP_MAX_TEMPS = 4, SIG_VP_MAX_HIST = 3 };
typedef struct { int32_t op, kind, a, b, c; } sig_vp_ins;                          /* a, b, c in 0..15; OSCTABLE, SHAPE, FILTERQ, OSCUNI, OSCBLEP: c may be -1; FILTEREQ, OSCSYNC: c and b may */
typedef struct { const double* ptr; int32_t col_stride; int32_t rows; } sig_vp_rows;
typedef struct {
    int32_t n_ins; sig_vp_ins ins[SIG_VP_MAX_INS];
    int32_t n_oscs; sig_vp_rows hertz[SIG_VP_MAX_OSCS], phase[SIG_VP_MAX_OSCS];     /* phase.ptr NULL: unplugged = 0 */
    int32_t n_params; sig_vp_rows params[SIG_VP_MAX_PARAMS];
    int32_t n_filters; sig_vp_rows cutoff[SIG_VP_MAX_FILTERS]; int32_t filter_type[SIG_VP_MAX_FILTERS];
    int32_t filter_level[SIG_VP_MAX_FILTERS];                                       /* 1 + the filters in series in front of this one */
    int32_t n_temps, depth;
    const double* adsr[6]; int32_t adsr_stride[6];                                  /* attack decay sustain release gate_on gate_off */
    uint64_t noise_seed[2];
} sig_voice_program_t;
int sig_voice_program(const sig_voice_program_t* program, int32_t rate, int64_t position, int32_t block_frames,
                      int32_t nblocks, int32_t context, int32_t voices, int32_t control_rows,
                      int32_t hist_blocks, const int64_t* hist_positions, int32_t blocks_before,
                      const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                      double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream);
/* sig_voice_program with the tables of its OSCTABLE and SHAPE instructions: up to SIG_VP_MAX_TABLES tables, each float32 (points, waves)
 * row-major in device memory under sig_osc_bank_table's rules (points a power of two) where an OSCTABLE word reads it, under
 * sig_shaper_table's (points >= 2) where only SHAPE words do, together at most SIG_TABLE_MAX_POINTS entries (they share the LDS of
 * a workgroup).  `tables` (HOST memory) may be NULL for a program without the instruction: sig_voice_program is this call with NULL. */
typedef struct { int32_t n_tables; struct { const float* ptr; int32_t points, waves; } table[SIG_VP_MAX_TABLES]; } sig_vp_tables_t;
int sig_voice_program_ex(const sig_voice_program_t* program, int32_t rate, int64_t position, int32_t block_frames,
                         int32_t nblocks, int32_t context, int32_t voices, int32_t control_rows,
                         int32_t hist_blocks, const int64_t* hist_positions, int32_t blocks_before,
                         const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                         double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream,
                         const sig_vp_tables_t* tables);
/* sig_voice_program_ex with the copies of its OSCUNI instructions: `unison` (HOST memory, copied into the launch as a kernel
 * parameter of its own): 1 <= copies <= SIG_UNISON_MAX_COPIES rows (detune[u], offset[u]).  NULL for a program without the
 * instruction: sig_voice_program_ex is this call with NULL.  Refused before any device work, hipErrorInvalidValue: copies out of
 * range, NULL with an OSCUNI word in the program, an OSCUNI word with b != 0, a >= n_oscs, c >= n_params or a kind above
 * SIG_OSC_TRIANGLE, and OSCUNI together with BAND, OSCPM, OSCTABLE, SHAPE or FILTERQ.  An OSCBLEP word reads the same copies and
 * is refused in the same cases, and with kind SIG_OSC_SINE; an OSCSYNC word likewise, and with kind SIG_OSC_TRIANGLE, b >= n_params
 * (its b is a parameter slot or -1, not a unison slot) or a FILTEREQ word in the program. */
typedef struct { int32_t copies; double detune[SIG_UNISON_MAX_COPIES], offset[SIG_UNISON_MAX_COPIES]; } sig_vp_unison_t;
int sig_voice_program_unison(const sig_voice_program_t* program, int32_t rate, int64_t position, int32_t block_frames,
                             int32_t nblocks, int32_t context, int32_t voices, int32_t control_rows,
                             int32_t hist_blocks, const int64_t* hist_positions, int32_t blocks_before,
                             const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                             double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream,
                             const sig_vp_tables_t* tables, const sig_vp_unison_t* unison);
/* sig_voice_program_unison for programs that COMBINE the extension words: two or more of the families BAND, OSCPM, OSCTABLE / SHAPE,
 * FILTERQ and OSCUNI in one program (a unison oscillator behind a resonant filter, a wavetable through a swept band filter ...), which
 * the three entries above refuse as described per word.  Such a program runs the interpreter's MIXED variant -- one more kernel with
 * every handler, its second parameter the tables and the copies together -- or the image attached for it (built with
 * -DSIG_VP_S_MIXED=1, which has exactly the program's families).  Only the exclusivity rules are lifted: a FILTERQ word and its
 * resonant slot still go together, band slots still pair from the start of their run, an OSCTABLE table is a power of two, the
 * tables stay inside SIG_TABLE_MAX_POINTS, an OSCUNI word needs `unison`.  In this variant LowPass / HighPass slots are designed by
 * the resonant design at damping sqrt2, which gives the Butterworth design's bits.  A program with one family or none is launched
 * exactly as by sig_voice_program_unison. */
int sig_voice_program_mixed(const sig_voice_program_t* program, int32_t rate, int64_t position, int32_t block_frames,
                            int32_t nblocks, int32_t context, int32_t voices, int32_t control_rows,
                            int32_t hist_blocks, const int64_t* hist_positions, int32_t blocks_before,
                            const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                            double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream,
                            const sig_vp_tables_t* tables, const sig_vp_unison_t* unison);
/* Tuning / test hook: force the voices per lane (1, 2; 0 = heuristic; ignored where the program does not fit the variant) and
 * the blocks per lane (0 = heuristic) of sig_voice_program.  Process-wide. */
int sig_voice_program_set_tuning(int32_t voices_per_lane, int32_t blocks_per_lane);
/* Introspection, no device work: the voices per lane and blocks per lane sig_voice_program picks for a problem.
 * store_aligned (bus_channels == 0): 4 = `out` 16-byte aligned with voices and out_ld multiples of 4, 2 = 8-byte aligned with
 * even voices and out_ld, else 1.  specialised != 0: as if a kernel specialised for four voices per lane were attached (the
 * interpreter runs one or two; sig_voice_program takes four where such an image is attached, the store is aligned for it or
 * there is a bus, and the launch still has a wave for every SIMD) -- what to build the image for. */
int sig_voice_program_geometry(int32_t voices, int32_t block_frames, int32_t nblocks, int32_t context, int32_t depth,
                               int32_t bus_channels, int32_t store_aligned, int32_t specialised,
                               int32_t* voices_per_lane, int32_t* blocks_per_lane);
/* Introspection, no device work: the interpreter variant sig_voice_program (and _ex, _unison, _mixed) launches for a program --
 * `family`: the one variant that has every extension word of the program, or MIXED for a program with words of two or more of
 * band, pm, table / shape, resonant and unison / blep -- and whether the program fits the small register file (1) or takes the full
 * one (0).  Reads the words and the slot counts of `program` (n_ins, ins, n_oscs, n_params, n_filters, n_temps), not its rows. */
enum { SIG_VP_FAMILY_PLAIN = 0, SIG_VP_FAMILY_BAND = 1, SIG_VP_FAMILY_PM = 2, SIG_VP_FAMILY_TABLE = 3, SIG_VP_FAMILY_SHAPE = 4,
       SIG_VP_FAMILY_RESONANT = 5, SIG_VP_FAMILY_UNISON = 6, SIG_VP_FAMILY_BLEP = 7, SIG_VP_FAMILY_MIXED = 8 };
int sig_voice_program_variant(const sig_voice_program_t* program, int32_t* family, int32_t* small_file);
/* SPECIALISED kernels.  The interpreter's source (signals_amd/csrc/voice_program.hip) built once more as a gfx950 code object
 * with ONE program as a compile-time constant -- macros SIG_VP_STATIC_CODE={words}, SIG_VP_S_NF / _NO / _NP / _NT / _EXT (the
 * register file: filter, oscillator, parameter, temporary slots; Amp / ADSR / White enabled), SIG_VP_STATIC_VPT, SIG_VP_STATIC_C,
 * SIG_VP_STATIC_WAVES; `hipcc --genco`, see signals_amd/specialise.py -- runs the same arithmetic as straight-line code (the
 * dispatch loop unrolls, every switch folds: 1.5-1.7x the interpreter).  sig_voice_program_attach hands such an image to the
 * library: it is loaded (hipModuleLoadData), asked what it was built for (its sig_vp_specialised_info kernel: the size of
 * the argument block, voices per lane, sink, program words -- anything else than THIS library's and the program given is
 * hipErrorInvalidImage) and from then on launched by sig_voice_program whenever it is called with the same words, slot counts
 * (n_oscs, n_params, n_filters, n_temps of `program`; its row pointers are not read), voices per lane and bus_channels.
 * A set-up call: allocates, launches and synchronises; not for a capturing stream.  sig_voice_program_use_attached(0) makes
 * every launch use the interpreter again (test hook), sig_voice_program_detach_all unloads the images (no launch may be in
 * flight).  sig_voice_program_args_size: sizeof of the kernels' argument block in this build. */
int sig_voice_program_attach(const sig_voice_program_t* program, int32_t voices_per_lane, int32_t bus_channels, const void* image);
int sig_voice_program_detach_all(void);
int sig_voice_program_use_attached(int32_t on);
int64_t sig_voice_program_args_size(void);

#ifdef __cplusplus
}
#endif
#endif /* SIGNALS_AMD_H */
