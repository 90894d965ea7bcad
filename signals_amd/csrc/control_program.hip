// A whole block-rate control subgraph in ONE launch, gfx950.
//
// The reference reads a control port once per block, at the block's position (BoundPort.forward_at_block_rate,
// chain/__init__.py:305-306): an LFO on a cutoff is an oscillator evaluated at one frame per block, scaled and offset by
// element-wise nodes (osc.py:26-62, fx.py:35-60).  Node by node that is a handful of launches of a few microseconds of
// work each -- a vibrato + cutoff sweep + tremolo voice spent half of its batch time (and all of its host time) in eleven
// of them.  Here the subgraph is a short straight-line program over registers, the same for every (block, column): thread
// (b, v) evaluates it for block b at column v and writes the requested registers to their (nblocks, cols) outputs.
// The machine itself -- an instruction's value, a block's frame, the filter, the stores -- is sig_ctl_machine.h, one statement
// for both builds of this file; here is what they do not share.  In the interpreter registers live in LDS, [register][thread]:
// every thread executes the same instruction, so a register index is uniform and the accesses are conflict-free (a private
// array indexed by a run-time value would go to scratch).  Instruction k writes register dst < n_ins (the host assigns them in
// instruction order).
#include <cstring>
#include <mutex>
#include <vector>

#include "sig_ctl_machine.h"

using sig_ctl::kSpecThreads;
using sig_ctl::kThreads;

#ifdef SIG_CTL_STATIC_INS
// A SPECIALISED build of this file (signals_amd/specialise.py: hipcc --genco with the program's structure as macros): the
// registers are VGPRs, the interpretive loop and its chain of dependent LDS accesses are gone.  SIG_CTL_STATIC_INS = {{op, kind,
// a, b, c, dst, wide}, ...} in evaluation order, SIG_CTL_STATIC_OUTS = {{reg, wide}, ...}; row pointers, strides and output
// pointers are still read from the run-time `program` / `outs` arrays (uniform loads).  One workgroup per block: the one-column
// instructions once per thread, the wide ones per chunk of 256 columns.
namespace {
struct SIns { int op, kind, a, b, c, dst, wide; };
struct SOut { int reg, wide; };
constexpr SIns kIns[] = SIG_CTL_STATIC_INS;
constexpr SOut kOuts[] = SIG_CTL_STATIC_OUTS;
constexpr int kN = (int)(sizeof(kIns) / sizeof(kIns[0])), kNO = (int)(sizeof(kOuts) / sizeof(kOuts[0]));
// wide: bit 0 = more than one column, bit 1 = window-rate (the run right in front of a FILTER)
constexpr int window_start(int k) { int w = k; while (w > 0 && (kIns[w - 1].wide & 2)) --w; return w; }
constexpr bool has_filter() { for (int k = 0; k < kN; ++k) if (kIns[k].op == SIG_CTL_FILTER) return true; return false; }
constexpr bool kHasFilter = has_filter();
constexpr int op_of(int k) { return kIns[k].op; }
constexpr int wide_of(int k) { return kIns[k].wide; }
static_assert(sig_ctl::pairs_formed(kN, op_of, wide_of), "every SIG_CTL_ADSR has its SIG_CTL_ADSRARGS right in front of it");
}  // namespace

extern "C" __global__ __launch_bounds__(kSpecThreads) void sig_ctl_specialised(double rate, int64_t position, int64_t step, int nblocks, int cols,
                                                                               int64_t front_position, int64_t min_position,
                                                                               const sig_ctl_ins* __restrict__ program, int n_ins,
                                                                               const sig_ctl_out* __restrict__ outs, int n_outs)
{
    const sig_ctl::Block blk(position, step, nblocks, front_position, min_position);
    const int64_t frame_b = blk.frame();
    const int h = sig_ctl::window_rows(frame_b);
    double reg[kN];
#pragma unroll
    for (int k = 0; k < kN; ++k) reg[k] = 0.0;
    auto get = [&](int r) { return r < 0 ? 0.0 : reg[r]; };
    auto exec = [&](int k, int v, int64_t frame, bool narrow) {
        return sig_ctl::value<true, true>(kIns[k], program[k], blk, v, frame, rate, narrow, get,
                                          [&] { const SIns G = kIns[k > 0 ? k - 1 : 0]; return sig_ctl::Carrier{G.a, G.b, G.c}; });
    };
    // window-rate instructions [window_start(k), k) of the FILTER k for the row at `frame`
    auto window = [&](int k, int v, int64_t frame, bool narrow) {
#pragma unroll
        for (int w = 0; w < kN; ++w)
            if (w >= window_start(k) && w < k) reg[kIns[w].dst] = exec(w, v, frame, narrow);
    };
    __shared__ double xs[kHasFilter ? kSpecThreads : 1];                       // a one-column filter's window rows
    auto run = [&](int v, bool wide_pass) {
#pragma unroll
        for (int k = 0; k < kN; ++k) {
            const SIns I = kIns[k];
            if (I.wide & 2) continue;                                          // window-rate: run by its filter
            if (((I.wide & 1) != 0) != wide_pass) continue;
            if (I.op != SIG_CTL_FILTER) { reg[I.dst] = exec(k, v, frame_b, false); continue; }
            sig_biquad::Biquad q;
            double z0 = 0.0, z1 = 0.0, y = 0.0;
            if (!wide_pass) {                                                  // thread j evaluates row j; every thread steps the filter
                const int j = threadIdx.x;
                if (j <= h) { window(k, 0, frame_b - h + j, j < h && h > 1); xs[j] = get(I.a); }
                __syncthreads();
                sig_ctl::design(I.kind, get(I.b), rate, threadIdx.x == 0, program[k], q);
                for (int i = 0; i <= h; ++i) y = sig_biquad::step(q, xs[i], z0, z1);
                __syncthreads();
            } else {                                                           // thread v walks the rows of its column
                sig_ctl::design(I.kind, get(I.b), rate, v < program[k].cols, program[k], q);
                for (int j = 0; j <= h; ++j) {
                    window(k, v, frame_b - h + j, j < h && h > 1);
                    y = sig_biquad::step(q, get(I.a), z0, z1);
                }
            }
            reg[I.dst] = y;
        }
    };
    run(0, false);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kNO; ++k)
            if (!kOuts[k].wide) sig_ctl::store<false>(outs, k, blk, 0, [&] { return reg[kOuts[k].reg]; });
    }
    for (int v0 = 0; v0 < cols; v0 += kSpecThreads) {
        const int v = v0 + threadIdx.x;
        run(v, true);
#pragma unroll
        for (int k = 0; k < kNO; ++k)
            if (kOuts[k].wide) { const sig_ctl_out o = outs[k]; sig_ctl::store<true>(&o, 0, blk, v, [&] { return reg[kOuts[k].reg]; }); }
    }
}
// what the attaching library checks: the structure the image was built for
extern "C" __global__ void sig_ctl_specialised_info(int32_t* out)
{
    out[0] = kN; out[1] = kNO;
    for (int k = 0; k < kN; ++k) {
        int32_t* w = out + 2 + 7 * k;
        w[0] = kIns[k].op; w[1] = kIns[k].kind; w[2] = kIns[k].a; w[3] = kIns[k].b; w[4] = kIns[k].c; w[5] = kIns[k].dst; w[6] = kIns[k].wide;
    }
    for (int k = 0; k < kNO; ++k) { out[2 + 7 * kN + 2 * k] = kOuts[k].reg; out[2 + 7 * kN + 2 * k + 1] = kOuts[k].wide; }
}
#else

namespace {

// One workgroup per block.  The program is copied into LDS once (fetching every instruction from global memory cost a
// dependent scalar load of ~0.5 us per instruction per wave); the register file behind it is sized by the program (n_regs x
// 128 threads x 8 B, dynamic LDS).  Instructions whose result is one column wide (an LFO: oscillator, scale, offset) run
// ONCE per block, before the loop over the columns; only the wide ones (the final products with per-voice rows) run per
// column chunk -- a vibrato + sweep + tremolo program over 1024 blocks x 1024 voices took 65 us with every (block, column)
// thread running all 26 instructions, three f64 sines among them.
// EXT (sig_control_program_windowed): also NOISE and FILTER with its window-rate instructions (the header's description).
// ENV (sig_control_program_envelope): EXT and the ADSRARGS / ADSR pair.
template <bool EXT, bool ENV = false>
__global__ __launch_bounds__(kThreads) void control_program_kernel(double rate, int64_t position, int64_t step, int nblocks, int cols,
                                                                   int64_t front_position, int64_t min_position,
                                                                   const sig_ctl_ins* __restrict__ program, int n_ins,
                                                                   const sig_ctl_out* __restrict__ outs, int n_outs)
{
    __shared__ sig_ctl_ins prog[SIG_CTL_MAX_INS];
    extern __shared__ double regs[];                                           // [register][thread]
    static_assert(EXT || !ENV, "the envelope variant is the windowed one and the ADSR pair");
    {
        const int words = n_ins * (int)(sizeof(sig_ctl_ins) / 4);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(program);
        uint32_t* dst = reinterpret_cast<uint32_t*>(prog);
        for (int w = threadIdx.x; w < words; w += kThreads) dst[w] = src[w];
    }
    __syncthreads();
    const sig_ctl::Block blk(position, step, nblocks, front_position, min_position);
    double* r = regs + threadIdx.x;
    auto get = [&](int reg) { return reg < 0 ? 0.0 : r[reg * kThreads]; };
    const int64_t frame_b = EXT ? blk.frame() : 0;                             // (EXT: the filters' window position)
    auto execute = [&](const sig_ctl_ins& ins, int v, int64_t frame, bool narrow) {
        if (ENV && ins.op == SIG_CTL_ADSRARGS) return;                         // (read by the ADSR behind it)
        r[ins.dst * kThreads] = sig_ctl::value<EXT, ENV>(ins, ins, blk, v, frame, rate, narrow, get, [&] {
            const sig_ctl_ins* g = &ins - 1;                                   // a lone ADSR reads zeros for the carrier's three
            const bool paired = &ins != prog && g->op == SIG_CTL_ADSRARGS;
            return sig_ctl::Carrier{paired ? g->a : -1, paired ? g->b : -1, paired ? g->c : -1};
        });
    };
    // FILTER `f` over the window-rate instructions [w0, k), cold-started over the rows p - h .. p
    const int h = sig_ctl::window_rows(frame_b);
    // one column: thread j evaluates window row j, then every thread steps the filter over the rows in the register file
    auto filter_narrow = [&](const sig_ctl_ins& f, int w0, int k) {
        const int j = threadIdx.x;
        if (j <= h)
            for (int w = w0; w < k; ++w) execute(prog[w], 0, frame_b - h + j, j < h && h > 1);
        __syncthreads();
        sig_biquad::Biquad q;
        sig_ctl::design(f.kind, get(f.b), rate, threadIdx.x == 0, f, q);
        double z0 = 0.0, z1 = 0.0, y = 0.0;
        const double* xs = regs + f.a * kThreads;
        for (int i = 0; i <= h; ++i) y = sig_biquad::step(q, xs[i], z0, z1);
        __syncthreads();                                                       // (every thread has read the rows)
        r[f.dst * kThreads] = y;
    };
    // wider: thread v walks the rows of its own column
    auto filter_wide = [&](const sig_ctl_ins& f, int w0, int k, int v) {
        sig_biquad::Biquad q;
        sig_ctl::design(f.kind, get(f.b), rate, v < f.cols, f, q);
        double z0 = 0.0, z1 = 0.0, y = 0.0;
        for (int j = 0; j <= h; ++j) {
            for (int w = w0; w < k; ++w) execute(prog[w], v, frame_b - h + j, j < h && h > 1);
            y = sig_biquad::step(q, get(f.a), z0, z1);
        }
        r[f.dst * kThreads] = y;
    };
    // ---- one column wide: once per block (every thread computes the same value into its own copy of the register).
    // Leading ROW instructions of that kind keep their global loads four in flight.
    int k0 = 0;
    while (k0 < n_ins && prog[k0].op == SIG_CTL_ROW && prog[k0].cols == 1) ++k0;
    for (int k = 0; k < k0; k += 4) {
        double x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = (k + u < k0) ? sig_ctl::row_value(prog[k + u], blk.b, 0) : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) if (k + u < k0) r[prog[k + u].dst * kThreads] = x[u];
    }
    if (!EXT) {
        for (int k = k0; k < n_ins; ++k)
            if (prog[k].cols == 1) execute(prog[k], 0, frame_b, false);
    } else {
        int w0 = -1;                                                           // first instruction of the current window run
        for (int k = k0; k < n_ins; ++k) {
            const sig_ctl_ins& ins = prog[k];
            if (ins.reserved) { if (w0 < 0) w0 = k; continue; }
            if (ins.op == SIG_CTL_FILTER) {
                if (ins.cols == 1) filter_narrow(ins, w0 < 0 ? k : w0, k);
                w0 = -1;
            } else if (ins.cols == 1) {
                execute(ins, 0, frame_b, false);
            }
        }
    }
    if (threadIdx.x == 0)
        for (int k = 0; k < n_outs; ++k)
            if (outs[k].cols == 1) sig_ctl::store<false>(outs, k, blk, 0, [&] { return r[outs[k].reg * kThreads]; });
    // ---- wider: per chunk of 128 columns
    for (int v0 = 0; v0 < cols; v0 += kThreads) {
        const int v = v0 + threadIdx.x;
        if (!EXT) {
            for (int k = k0; k < n_ins; ++k)
                if (prog[k].cols > 1) execute(prog[k], v, frame_b, false);
        } else {
            int w0 = -1;
            for (int k = k0; k < n_ins; ++k) {
                const sig_ctl_ins& ins = prog[k];
                if (ins.reserved) { if (w0 < 0) w0 = k; continue; }
                if (ins.op == SIG_CTL_FILTER) {
                    if (ins.cols > 1) filter_wide(ins, w0 < 0 ? k : w0, k, v);
                    w0 = -1;
                } else if (ins.cols > 1) {
                    execute(ins, v, frame_b, false);
                }
            }
        }
        for (int k = 0; k < n_outs; ++k) {
            const sig_ctl_out o = outs[k];
            if (o.cols > 1) sig_ctl::store<true>(&o, 0, blk, v, [&] { return r[o.reg * kThreads]; });
        }
    }
}

// What every launching entry checks, and the workgroups of the launch: one per block and one for a front position; 0 where
// there is nothing to do
int ctl_workgroups(int32_t rate, int32_t step, int32_t nblocks, int32_t cols, int64_t front_position, int64_t min_position,
                   const sig_ctl_ins* program, int32_t n_ins, const sig_ctl_out* outs, int32_t n_outs, unsigned& workgroups)
{
    SIG_CHECK_ARG(rate > 0 && step >= 0 && nblocks >= 0 && cols >= 1 && n_ins >= 0 && n_outs >= 0 && front_position >= -1 && min_position >= 0);
    SIG_CHECK_ARG((program || n_ins == 0) && (outs || n_outs == 0) && n_ins <= SIG_CTL_MAX_INS);
    workgroups = ((nblocks == 0 && front_position < 0) || n_outs == 0) ? 0u : (unsigned)(nblocks + (front_position >= 0 ? 1 : 0));
    return 0;
}

template <bool EXT, bool ENV = false>
int launch_control_program(int32_t rate, int64_t position, int32_t step, int32_t nblocks, int32_t cols,
                           int64_t front_position, int64_t min_position,
                           const sig_ctl_ins* program, int32_t n_ins, const sig_ctl_out* outs, int32_t n_outs, void* stream)
{
    unsigned workgroups = 0;
    if (const int bad = ctl_workgroups(rate, step, nblocks, cols, front_position, min_position, program, n_ins, outs, n_outs, workgroups)) return bad;
    if (workgroups == 0) return 0;
    // one register per instruction (dst < n_ins): the program lives in device memory, so register indices cannot be checked
    // here -- the LDS register file is sized by n_ins, and n_ins <= SIG_CTL_MAX_INS == SIG_CTL_MAX_REGS was checked above
    static_assert(SIG_CTL_MAX_INS <= SIG_CTL_MAX_REGS, "the register file is sized by the instruction count");
    const int n_regs = n_ins > 0 ? n_ins : 1;
    control_program_kernel<EXT, ENV><<<workgroups, kThreads, (size_t)n_regs * kThreads * sizeof(double), static_cast<hipStream_t>(stream)>>>(
        (double)rate, position, step, nblocks, cols, front_position, min_position, program, n_ins, outs, n_outs);
    return sig_launch_status();
}

}  // namespace

extern "C" int sig_control_program(int32_t rate, int64_t position, int32_t step, int32_t nblocks, int32_t cols,
                                   int64_t front_position, int64_t min_position,
                                   const sig_ctl_ins* program, int32_t n_ins, const sig_ctl_out* outs, int32_t n_outs, void* stream)
{
    return launch_control_program<false>(rate, position, step, nblocks, cols, front_position, min_position, program, n_ins, outs, n_outs, stream);
}

extern "C" int sig_control_program_windowed(int32_t rate, int64_t position, int32_t step, int32_t nblocks, int32_t cols,
                                            int64_t front_position, int64_t min_position,
                                            const sig_ctl_ins* program, int32_t n_ins, const sig_ctl_out* outs, int32_t n_outs, void* stream)
{
    return launch_control_program<true>(rate, position, step, nblocks, cols, front_position, min_position, program, n_ins, outs, n_outs, stream);
}

extern "C" int sig_control_program_envelope(int32_t rate, int64_t position, int32_t step, int32_t nblocks, int32_t cols,
                                            int64_t front_position, int64_t min_position,
                                            const sig_ctl_ins* program, int32_t n_ins, const sig_ctl_out* outs, int32_t n_outs, void* stream)
{
    return launch_control_program<true, true>(rate, position, step, nblocks, cols, front_position, min_position, program, n_ins, outs, n_outs, stream);
}

// ---- specialised builds of this file (see the top): attached at run time, launched through a handle.  The program itself is in
// device memory, so the library cannot match it against the image: the caller keeps the handle with the program it built the
// image from (signals_amd/engine/control.py: _ControlProgram).
namespace {
struct CtlSpecial { hipModule_t mod; hipFunction_t fn; };
std::vector<CtlSpecial>& ctl_specials() { static std::vector<CtlSpecial> v; return v; }
std::mutex& ctl_specials_lock() { static std::mutex m; return m; }
}  // namespace

extern "C" int sig_control_program_attach(const int32_t* description, int32_t n_words, const void* image, int32_t* handle)
{
    SIG_CHECK_ARG(description && image && handle && n_words >= 2 && n_words <= 2 + 7 * SIG_CTL_MAX_INS + 2 * 64);
    const int n = description[0];
    SIG_CHECK_ARG(n >= 0 && n <= SIG_CTL_MAX_INS && 2 + 7 * n <= n_words);
    SIG_CHECK_ARG(sig_ctl::pairs_formed(n, [&](int k) { return description[2 + 7 * k]; }, [&](int k) { return description[2 + 7 * k + 6]; }));
    CtlSpecial e{};
    hipError_t err = hipModuleLoadData(&e.mod, image);
    if (err != hipSuccess) { (void)hipGetLastError(); return (int)err; }
    hipFunction_t info = nullptr;
    err = hipModuleGetFunction(&e.fn, e.mod, "sig_ctl_specialised");
    if (err == hipSuccess) err = hipModuleGetFunction(&info, e.mod, "sig_ctl_specialised_info");
    std::vector<int32_t> got((size_t)2 + 7 * SIG_CTL_MAX_INS + 2 * 64, 0);
    int32_t* dev = nullptr;
    if (err == hipSuccess) err = hipMalloc(&dev, got.size() * sizeof(int32_t));
    if (err == hipSuccess) {
        void* params[] = {&dev};
        err = hipModuleLaunchKernel(info, 1, 1, 1, 1, 1, 1, 0, nullptr, params, nullptr);
        if (err == hipSuccess) err = hipMemcpy(got.data(), dev, got.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
        (void)hipFree(dev);
    }
    if (err == hipSuccess && memcmp(got.data(), description, sizeof(int32_t) * (size_t)n_words) != 0) err = hipErrorInvalidImage;
    if (err == hipSuccess && 2 + 7 * got[0] + 2 * got[1] != n_words) err = hipErrorInvalidImage;
    if (err != hipSuccess) { (void)hipModuleUnload(e.mod); (void)hipGetLastError(); return (int)err; }
    std::lock_guard<std::mutex> g(ctl_specials_lock());
    ctl_specials().push_back(e);
    *handle = (int32_t)ctl_specials().size();
    return 0;
}

extern "C" int sig_control_program_attached(int32_t handle, int32_t rate, int64_t position, int32_t step, int32_t nblocks, int32_t cols,
                                            int64_t front_position, int64_t min_position,
                                            const sig_ctl_ins* program, int32_t n_ins, const sig_ctl_out* outs, int32_t n_outs, void* stream)
{
    unsigned workgroups = 0;
    if (const int bad = ctl_workgroups(rate, step, nblocks, cols, front_position, min_position, program, n_ins, outs, n_outs, workgroups)) return bad;
    hipFunction_t fn = nullptr;
    {
        std::lock_guard<std::mutex> g(ctl_specials_lock());
        SIG_CHECK_ARG(handle >= 1 && (size_t)handle <= ctl_specials().size());
        fn = ctl_specials()[(size_t)handle - 1].fn;
    }
    if (workgroups == 0) return 0;
    double rate_d = (double)rate;
    int64_t step64 = step;
    void* params[] = {&rate_d, &position, &step64, &nblocks, &cols, &front_position, &min_position, &program, &n_ins, &outs, &n_outs};
    return (int)hipModuleLaunchKernel(fn, workgroups, 1, 1, kSpecThreads, 1, 1, 0, static_cast<hipStream_t>(stream), params, nullptr);
}
#endif  // SIG_CTL_STATIC_INS
