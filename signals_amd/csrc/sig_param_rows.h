// What the entries that take block-rate parameter rows state alike (sampler.hip, modal.hip, shaper.hip, osc_bank.hip): the row as the C
// ABI passes it, the kernel's read of it, and the checks and the store-type dispatch in front of a launch.  Host code but for
// row_value(); kernels keep their own parameter loads where they have them (OscArgs and the oscillator kernels do).
#pragma once
#include "sig_common.h"

namespace sig_rows {

// One parameter row: (1 | P, V | 1) f64 -- `stride` between voices (0: one column), `row_stride` between rows; NULL = unplugged = 0
struct Row { const double* p; int stride; int64_t row_stride; };

// voice v's value in parameter row `prow`; 0 for an unplugged row and for a lane past the voices
__device__ __forceinline__ double row_value(const Row& r, int64_t prow, int v, bool live)
{
    return (r.p && live) ? r.p[prow * r.row_stride + (int64_t)v * r.stride] : 0.0;
}

// One parameter's strides as every entry takes them
inline bool strides_ok(int32_t stride, int64_t row_stride) { return (stride == 0 || stride == 1) && row_stride >= 0; }

// The head of a launch over `rows` frames from `position` on, `position_step` apart, one parameter row per `rows_per_param` of them
inline bool head_ok(int64_t position, int64_t position_step, int32_t rate, int64_t rows, int32_t voices, int32_t rows_per_param)
{
    return rows >= 0 && voices >= 0 && rate > 0 && position >= 0 && position_step >= 1 && rows_per_param >= 0;
}

// f(out as float* | double*), hipErrorInvalidValue without a call for any other `out_dtype`
template <typename F>
int dispatch_out(void* out, int32_t out_dtype, F&& f)
{
    if (out_dtype == SIG_F32) return f(static_cast<float*>(out));
    if (out_dtype == SIG_F64) return f(static_cast<double*>(out));
    return (int)hipErrorInvalidValue;
}

}  // namespace sig_rows
