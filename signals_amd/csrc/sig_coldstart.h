// What the cold-start filter files (biquad.hip, band.hip, biquad_bus.hip) share: the row vectors a lane loads and stores, the
// per-block control rows, and on the host the entries' common argument checks, the 16-byte-access predicate and the buffer-type
// dispatch.  Launch geometry: sig_common.h.
#pragma once
#include <initializer_list>

#include "sig_biquad.h"

namespace sig_cold {

// ---- a lane's VPT consecutive samples of one row, as one load / store
template <typename T, int VPT> struct RowVec;
template <> struct RowVec<float, 1> { using type = float; };
template <> struct RowVec<double, 1> { using type = double; };
template <> struct RowVec<float, 2> { using type = float2; };
template <> struct RowVec<double, 2> { using type = double2; };
template <> struct RowVec<float, 4> { using type = float4; };
template <> struct RowVec<double, 4> { using type = double4; };

template <typename T> __device__ __forceinline__ void unpack(const T& v, double (&x)[1]) { x[0] = (double)v; }
__device__ __forceinline__ void unpack(const float2& v, double (&x)[2]) { x[0] = v.x; x[1] = v.y; }
__device__ __forceinline__ void unpack(const double2& v, double (&x)[2]) { x[0] = v.x; x[1] = v.y; }
__device__ __forceinline__ void unpack(const float4& v, double (&x)[4]) { x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
__device__ __forceinline__ void unpack(const double4& v, double (&x)[4]) { x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
__device__ __forceinline__ void pack(float& v, const double (&y)[1]) { v = (float)y[0]; }
__device__ __forceinline__ void pack(double& v, const double (&y)[1]) { v = y[0]; }
__device__ __forceinline__ void pack(float2& v, const double (&y)[2]) { v = make_float2((float)y[0], (float)y[1]); }
__device__ __forceinline__ void pack(double2& v, const double (&y)[2]) { v = make_double2(y[0], y[1]); }
__device__ __forceinline__ void pack(float4& v, const double (&y)[4]) { v = make_float4((float)y[0], (float)y[1], (float)y[2], (float)y[3]); }
__device__ __forceinline__ void pack(double4& v, const double (&y)[4]) { v = make_double4(y[0], y[1], y[2], y[3]); }

// ---- (blocks, voices | 1) f64 control rows, blocks = 1: one row for every block; ptr null: unplugged
// Block b, voice v is at  ptr + (blocks > 1 ? b * (stride ? voices : 1) : 0) + v * stride.  The kernels write that expression out
// by hand on purpose, as they do their wave coordinates, register ring, DF2T step and status report: an accessor here, tried as a
// member and as an inline function, changed the register allocation and the branch structure of every kernel that used it, and
// this family is held to its generated code, instruction for instruction (tools/compare_kernels.py --by-content).
struct BlockRows {
    const double* ptr;
    int stride, blocks;
};

// ---- host: what every cold-start entry checks the same way.  `in` points behind `history` context rows; block 0 reads
// min(context, position) of them, later blocks reach back into earlier blocks' rows and, when block_frames < context, also into
// the history.  `empty`: nothing to launch, which is a success once every check has passed.
inline bool window_ok(int32_t rate, int64_t position, int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                      const void* in, int64_t in_ld, int64_t in_history, const void* out, bool& empty)
{
    empty = block_frames == 0 || nblocks == 0 || voices == 0;
    return rate > 0 && position >= 0 && block_frames >= 0 && nblocks >= 0 && context >= 0 && voices >= 0 &&
           in != nullptr && out != nullptr && in_ld >= voices && in_history >= (position < context ? position : context);
}
// control rows: one column or one per voice, one row or one per block; `plugged`: must be there
inline bool rows_ok(const BlockRows& r, int32_t nblocks, bool plugged) {
    return (r.ptr || !plugged) && (r.stride == 0 || r.stride == 1) && (r.blocks == 1 || r.blocks == nblocks);
}

// every row of every buffer allows one access of `vpt` elements of `elem` bytes per lane
inline bool vec_ok(int vpt, size_t elem, int voices, std::initializer_list<int64_t> lds, std::initializer_list<const void*> ptrs)
{
    bool ok = voices % vpt == 0;
    for (int64_t ld : lds) ok = ok && ld % vpt == 0;
    for (const void* p : ptrs) ok = ok && reinterpret_cast<uintptr_t>(p) % (vpt * elem) == 0;
    return ok;
}

// f(in, out) with the buffers as float* | double*, hipErrorInvalidValue without a call for any other dtype
template <typename F>
int dispatch_dtype(int32_t dtype, const void* in, void* out, F&& f)
{
    if (dtype == SIG_F32) return f(static_cast<const float*>(in), static_cast<float*>(out));
    if (dtype == SIG_F64) return f(static_cast<const double*>(in), static_cast<double*>(out));
    return (int)hipErrorInvalidValue;
}

}  // namespace sig_cold
