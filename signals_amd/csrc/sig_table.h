// A (T, W) float32 table held in LDS: what the wavetable oscillator (osc_bank.hip), the waveshaper (shaper.hip) and the table
// variant of the voice program (sig_vp_machine.h) share.
// Layout: column-major, S = T + 1 floats per column -- entry (i, w) at tab[w * S + i] -- and the guard entry tab[w * S + T] =
// tab[w * S + 0].  A linear interpolation reads its two operands (i, i + 1) of one column as ONE paired access at one address; the
// guard lets an oscillator's last segment wrap without a second mask (the shaper never reaches it: its last segment ends at T - 1);
// the odd column stride keeps equal indices of different columns on different banks.
#pragma once
#include "sig_common.h"

namespace sig_table {

inline size_t lds_bytes(int T, int W) { return (size_t)(T + 1) * W * sizeof(float); }

// Stage the row-major device table into `tab`, all THREADS threads of the workgroup taking part; the caller synchronises.
// Coalesced read: element k = i * W + w goes to column w, row i; (i, w) advance by a workgroup's worth of elements per step, so the
// division is paid once per thread, not per element.
template <int THREADS>
__device__ __forceinline__ void stage(float* tab, const float* table, int T, int W)
{
    const int S = T + 1;
    const int di = THREADS / W, dw = THREADS - di * W;
    int si = (int)threadIdx.x / W, sw = (int)threadIdx.x - si * W;
    for (int k = threadIdx.x; k < T * W; k += THREADS) {
        tab[sw * S + si] = table[k];
        si += di; sw += dw;
        if (sw >= W) { sw -= W; ++si; }
    }
    for (int w = threadIdx.x; w < W; w += THREADS) tab[w * S + T] = table[w];
}

// The same staging for a table that is read one entry at a time (the additive oscillator's (H, W) amplitudes, osc_bank.hip): column
// stride S >= T given by the caller, no guard entry -- entry (i, w) at tab[w * S + i], S * W floats in all.
template <int THREADS>
__device__ __forceinline__ void stage_columns(float* tab, const float* table, int T, int W, int S)
{
    const int di = THREADS / W, dw = THREADS - di * W;
    int si = (int)threadIdx.x / W, sw = (int)threadIdx.x - si * W;
    for (int k = threadIdx.x; k < T * W; k += THREADS) {
        tab[sw * S + si] = table[k];
        si += di; sw += dw;
        if (sw >= W) { sw -= W; ++si; }
    }
}

// the column a `select` value picks: clip(floor(select), 0, W - 1), NaN -> 0
__device__ __forceinline__ int column(double select, int W)
{
    const double s = floor(select);
    return (s >= 1.0) ? ((s >= (double)(W - 1)) ? W - 1 : (int)s) : 0;
}

}  // namespace sig_table
