// The modal resonator bank (chain/ext.py Modal, modal.hip): the table's limits, its staging into LDS and the geometry of a run.
// The table is float64 (W, M, 3) row-major in device memory -- W mode sets of M rows (ratio r, amplitude a, decay rate lambda in 1/s).
#pragma once
#include <stdint.h>

#include "sig_common.h"

namespace sig_modal {

constexpr int kMaxModes = 64;          // M: rows of one mode set
constexpr int kMaxPoints = 2048;       // W * M: rows of the table, 48 KiB of LDS as doubles
constexpr int kRun = SIG_WAVE;         // rows of a run: lane l holds the quotient n / rate of the run's row l

inline bool shape_ok(int64_t sets, int64_t count)
{
    return count >= 1 && count <= kMaxModes && sets >= 1 && sets * count <= kMaxPoints;
}

inline size_t lds_bytes(int sets, int count) { return (size_t)sets * count * 3 * sizeof(double); }

#if defined(__HIPCC__)
// Stage `n` doubles of the device table into `tab` as they lie, all THREADS threads of the workgroup taking part (coalesced 8-byte
// reads); the caller synchronises.  The float64 sibling of sig_table.h's stage_columns: a mode's three values stay adjacent, since one
// lane reads all three.
template <int THREADS>
__device__ __forceinline__ void stage_rows(double* tab, const double* table, int n)
{
    for (int k = threadIdx.x; k < n; k += THREADS) tab[k] = table[k];
}
#endif

}  // namespace sig_modal
