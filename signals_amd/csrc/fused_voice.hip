// Fused voice chain for gfx950: Osc -> cold-start Butterworth biquad -> [x per-voice gain] -> f32 store or
// -> [pan x gain] -> bus partial sums, K blocks per launch (design and arithmetic: sig_fused_walk.h).  This translation unit
// instantiates the Sine kernels -- the span walker (sig_fused_walk.h), the closed form (sig_fused_steady.h), the latency scan
// (sig_fused_scan.h), planned by sig_fused_launch.h -- and holds the C ABI of the family; fused_voice_b.hip instantiates the
// walkers of Square, Sawtooth and Triangle.  Tuning builds (tools/build_variant.sh -DSIG_TUNE_SINE_ONLY) keep this unit alone,
// with the Sine kernels and a stereo bus only.
#include <cstdlib>

#include "sig_fused_launch.h"

// Tuning / test hooks.  Product launches read four plain ints; they start from the environment (SIG_FUSED_VPT, _SPAN,
// _STEADY, _SCAN: read ONCE, when the first launch asks) and tests set them through sig_fused_set_tuning.
// (struct Tuning and tuning() are declared in sig_steady.h: ONE instance for both translation units)
sig_fused::Tuning& sig_fused::tuning() {
    static Tuning t = [] {
        auto env = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
        Tuning u;
        u.vpt = env("SIG_FUSED_VPT", 0); u.span = env("SIG_FUSED_SPAN", 0);
        u.steady = env("SIG_FUSED_STEADY", -1); u.scan = env("SIG_FUSED_SCAN", -1);
        if (u.steady == 2) { u.steady = 1; u.tile_sum_kernel = 1; }
        if (u.steady == 3) { u.steady = 1; u.mix_f32 = 1; }
        return u;
    }();
    return t;
}

namespace {

// One description of a fused call.  Every extern "C" entry below fills it (the leading members in the order all of them share,
// then the parts it has); run_call() checks it, builds the kernels' arguments from it and launches.
enum Sink { SINK_VOICES, SINK_MIX, SINK_BUS };      // (block_frames * nblocks, voices) rows | those rows x a 64 x 64 matrix | bus channels
struct FusedCall {
    int osc_kind, filt_type; int32_t rate; int64_t position;
    int32_t block_frames, nblocks, context, voices;
    const double* hertz; int32_t hertz_stride; const double* phase; int32_t phase_stride;
    const double* cutoff; int32_t cutoff_stride; const double* gain; int32_t gain_stride;
    float* out; int64_t out_ld; int32_t* status; void* stream;
    Sink sink = SINK_VOICES;
    bool rows = false;                                   // the per-block-parameter entries (*_rows, *_fm, *_pair): launch_rows
    int32_t cutoff_rows = 1, gain_rows = 1;
    // *_pair: Mix (op 1) or RingMod (op 2) of two oscillators
    int pair_op = 0, kind2 = 0;
    const double* hertz2 = nullptr; int32_t hertz2_stride = 0; const double* phase2 = nullptr; int32_t phase2_stride = 0;
    const double* mix = nullptr; int32_t mix_stride = 0;
    // *_fm: hertz / phase rows per block + the row in front of the launch
    int32_t hertz_rows = 1, phase_rows = 1; const double* hertz_hist = nullptr; const double* phase_hist = nullptr;
    bool devpos = false; const int64_t* position_dev = nullptr;       // *_devpos: the position is read from device memory
    const float* matrix = nullptr;                       // SINK_MIX
    // SINK_BUS
    const double* bus_gains = nullptr; int64_t bus_gains_ld = 0; int32_t bus_channels = 0; double* workspace = nullptr;
    double* consts = nullptr; int32_t consts_ready = 0; int force_walk = 0;
};

bool stride_ok(int32_t s) { return (s | 1) == 1; }

bool call_ok(const FusedCall& c)
{
    const bool bus = c.sink == SINK_BUS;
    if (c.filt_type != SIG_FILT_LOWPASS && c.filt_type != SIG_FILT_HIGHPASS) return false;
    if (!(c.rate > 0 && (c.devpos ? c.position_dev != nullptr : c.position >= 0))) return false;
    if (!(c.block_frames >= 0 && c.nblocks >= 0 && c.context >= 0 && c.voices >= 0)) return false;
    if (!(c.hertz && c.cutoff && c.out && c.out_ld >= (bus ? c.bus_channels : c.voices))) return false;
    if (!(stride_ok(c.hertz_stride) && stride_ok(c.phase_stride) && stride_ok(c.cutoff_stride) && stride_ok(c.gain_stride))) return false;
    if (!((c.cutoff_rows == 1 || c.cutoff_rows == c.nblocks) && (c.gain_rows == 1 || c.gain_rows == c.nblocks))) return false;
    if (c.pair_op != 0 && !((c.pair_op == 1 || c.pair_op == 2) && c.kind2 >= SIG_OSC_SINE && c.kind2 <= SIG_OSC_TRIANGLE && c.hertz2 &&
                            stride_ok(c.hertz2_stride) && stride_ok(c.phase2_stride) && stride_ok(c.mix_stride) && (c.pair_op == 2 || c.mix)))
        return false;
    if ((c.hertz_hist || c.phase_hist) && c.block_frames < c.context) return false;   // (the context of a shorter block is not the previous block's samples)
    if (!((c.hertz_rows == 1 || (c.hertz_rows == c.nblocks && c.hertz_hist)) &&
          (c.phase_rows == 1 || (c.phase_rows == c.nblocks && c.phase_hist)) && (!c.phase_hist || c.phase))) return false;
    if (c.sink == SINK_MIX && !(c.matrix && c.voices % 64 == 0)) return false;
    if (bus && !(c.workspace && (c.bus_gains ? c.bus_gains_ld >= c.voices : c.bus_channels == 1))) return false;
    return true;
}

int run_call(const FusedCall& c)
{
    SIG_CHECK_ARG(call_ok(c));
    if (c.block_frames == 0 || c.nblocks == 0 || c.voices == 0) return 0;
    const bool bus = c.sink == SINK_BUS;
    FusedArgs a{c.filt_type, (double)c.rate, c.devpos ? 0 : c.position, c.block_frames, c.nblocks, c.context, c.voices,
                c.hertz, c.hertz_stride, c.phase, c.phase_stride, c.cutoff, c.cutoff_stride, c.gain, c.gain_stride,
                bus ? nullptr : c.out, bus ? 0 : c.out_ld, 0, c.status, c.devpos ? c.position_dev : nullptr};
    a.mix = c.matrix;
    a.consts_ext = c.consts; a.consts_ready = c.consts_ready; a.force_walk = c.force_walk;
    a.cutoff_rows = c.cutoff_rows; a.gain_rows = c.gain_rows;
    a.hertz_rows = c.hertz_rows; a.phase_rows = c.phase_rows; a.hertz_hist = c.hertz_hist; a.phase_hist = c.phase_hist;
    a.pair_op = c.pair_op; a.kind2 = c.kind2; a.hertz2 = c.hertz2; a.hs2 = c.hertz2_stride; a.phase2 = c.phase2; a.ps2 = c.phase2_stride;
    a.mixrow = c.mix; a.ms = c.mix_stride;
    const BusArgs busargs = bus ? BusArgs{c.bus_gains, c.bus_gains_ld, c.workspace, (int64_t)c.block_frames * c.nblocks}
                                : BusArgs{nullptr, 0, nullptr, 0};
    hipStream_t s = static_cast<hipStream_t>(c.stream);
    if (c.rows) {
        SIG_CHECK_ARG(!bus || c.bus_channels == 1 || c.bus_channels == 2);    // (4-channel buses: the per-node schedule)
        return dispatch_rows(bus ? c.bus_channels : 0, c.osc_kind, a, busargs, c.out, c.out_ld, s);
    }
    switch (c.sink) {
        case SINK_BUS: return dispatch_bus(c.gain != nullptr, c.osc_kind, c.bus_channels, a, busargs, c.out, c.out_ld, s);
        case SINK_MIX: return dispatch_mix(c.gain != nullptr, c.osc_kind, a, s);
        default: return dispatch_chain(c.gain != nullptr, c.osc_kind, a, s);
    }
}

void set_rows(FusedCall& c, int32_t cutoff_rows, int32_t gain_rows) { c.rows = true; c.cutoff_rows = cutoff_rows; c.gain_rows = gain_rows; }

void set_bus(FusedCall& c, const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels, double* workspace)
{
    c.sink = SINK_BUS; c.bus_gains = bus_gains; c.bus_gains_ld = bus_gains_ld; c.bus_channels = bus_channels; c.workspace = workspace;
}

void set_pair(FusedCall& c, int pair_op, int osc2_kind, const double* hertz2, int32_t hertz2_stride, const double* phase2,
              int32_t phase2_stride, const double* mix, int32_t mix_stride)
{
    c.pair_op = pair_op; c.kind2 = osc2_kind; c.hertz2 = hertz2; c.hertz2_stride = hertz2_stride;
    c.phase2 = phase2; c.phase2_stride = phase2_stride; c.mix = mix; c.mix_stride = mix_stride;
}

void set_fm(FusedCall& c, int32_t hertz_rows, const double* hertz_hist, int32_t phase_rows, const double* phase_hist)
{
    c.hertz_rows = hertz_rows; c.hertz_hist = hertz_hist; c.phase_rows = phase_rows; c.phase_hist = phase_hist;
}

}  // namespace

extern "C" int sig_fused_osc_biquad(int osc_kind, int filt_type, int32_t rate, int64_t position,
                                    int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                    const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                                    const double* cutoff, int32_t cutoff_stride,
                                    const double* gain, int32_t gain_stride,
                                    float* out, int64_t out_ld, int32_t* status, void* stream)
{
    FusedCall c{osc_kind, filt_type, rate, position, block_frames, nblocks, context, voices, hertz, hertz_stride, phase, phase_stride,
                cutoff, cutoff_stride, gain, gain_stride, out, out_ld, status, stream};
    return run_call(c);
}

extern "C" int sig_fused_osc_pair_biquad(int osc_kind, int osc2_kind, int pair_op, int filt_type, int32_t rate, int64_t position,
                                         int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                         const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                                         const double* hertz2, int32_t hertz2_stride, const double* phase2, int32_t phase2_stride,
                                         const double* mix, int32_t mix_stride,
                                         const double* cutoff, int32_t cutoff_stride, int32_t cutoff_rows,
                                         const double* gain, int32_t gain_stride, int32_t gain_rows,
                                         float* out, int64_t out_ld, int32_t* status, void* stream)
{
    SIG_CHECK_ARG(pair_op == 1 || pair_op == 2);
    FusedCall c{osc_kind, filt_type, rate, position, block_frames, nblocks, context, voices, hertz, hertz_stride, phase, phase_stride,
                cutoff, cutoff_stride, gain, gain_stride, out, out_ld, status, stream};
    set_rows(c, cutoff_rows, gain_rows);
    set_pair(c, pair_op, osc2_kind, hertz2, hertz2_stride, phase2, phase2_stride, mix, mix_stride);
    return run_call(c);
}

extern "C" int sig_fused_voice_pair_bus(int osc_kind, int osc2_kind, int pair_op, int filt_type, int32_t rate, int64_t position,
                                        int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                        const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                                        const double* hertz2, int32_t hertz2_stride, const double* phase2, int32_t phase2_stride,
                                        const double* mix, int32_t mix_stride,
                                        const double* cutoff, int32_t cutoff_stride, int32_t cutoff_rows,
                                        const double* gain, int32_t gain_stride, int32_t gain_rows,
                                        const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                                        double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream)
{
    SIG_CHECK_ARG(pair_op == 1 || pair_op == 2);
    FusedCall c{osc_kind, filt_type, rate, position, block_frames, nblocks, context, voices, hertz, hertz_stride, phase, phase_stride,
                cutoff, cutoff_stride, gain, gain_stride, out, out_ld, status, stream};
    set_rows(c, cutoff_rows, gain_rows);
    set_pair(c, pair_op, osc2_kind, hertz2, hertz2_stride, phase2, phase2_stride, mix, mix_stride);
    set_bus(c, bus_gains, bus_gains_ld, bus_channels, workspace);
    return run_call(c);
}

extern "C" int sig_fused_osc_biquad_rows(int osc_kind, int filt_type, int32_t rate, int64_t position,
                                         int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                         const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                                         const double* cutoff, int32_t cutoff_stride, int32_t cutoff_rows,
                                         const double* gain, int32_t gain_stride, int32_t gain_rows,
                                         float* out, int64_t out_ld, int32_t* status, void* stream)
{
    FusedCall c{osc_kind, filt_type, rate, position, block_frames, nblocks, context, voices, hertz, hertz_stride, phase, phase_stride,
                cutoff, cutoff_stride, gain, gain_stride, out, out_ld, status, stream};
    set_rows(c, cutoff_rows, gain_rows);
    return run_call(c);
}

extern "C" int sig_fused_voice_bus_rows(int osc_kind, int filt_type, int32_t rate, int64_t position,
                                        int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                        const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                                        const double* cutoff, int32_t cutoff_stride, int32_t cutoff_rows,
                                        const double* gain, int32_t gain_stride, int32_t gain_rows,
                                        const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                                        double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream)
{
    FusedCall c{osc_kind, filt_type, rate, position, block_frames, nblocks, context, voices, hertz, hertz_stride, phase, phase_stride,
                cutoff, cutoff_stride, gain, gain_stride, out, out_ld, status, stream};
    set_rows(c, cutoff_rows, gain_rows);
    set_bus(c, bus_gains, bus_gains_ld, bus_channels, workspace);
    return run_call(c);
}

extern "C" int sig_fused_osc_biquad_fm(int osc_kind, int filt_type, int32_t rate, int64_t position,
                                       int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                       const double* hertz, int32_t hertz_stride, int32_t hertz_rows, const double* hertz_hist,
                                       const double* phase, int32_t phase_stride, int32_t phase_rows, const double* phase_hist,
                                       const double* cutoff, int32_t cutoff_stride, int32_t cutoff_rows,
                                       const double* gain, int32_t gain_stride, int32_t gain_rows,
                                       float* out, int64_t out_ld, int32_t* status, void* stream)
{
    FusedCall c{osc_kind, filt_type, rate, position, block_frames, nblocks, context, voices, hertz, hertz_stride, phase, phase_stride,
                cutoff, cutoff_stride, gain, gain_stride, out, out_ld, status, stream};
    set_rows(c, cutoff_rows, gain_rows);
    set_fm(c, hertz_rows, hertz_hist, phase_rows, phase_hist);
    return run_call(c);
}

extern "C" int sig_fused_voice_bus_fm(int osc_kind, int filt_type, int32_t rate, int64_t position,
                                      int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                      const double* hertz, int32_t hertz_stride, int32_t hertz_rows, const double* hertz_hist,
                                      const double* phase, int32_t phase_stride, int32_t phase_rows, const double* phase_hist,
                                      const double* cutoff, int32_t cutoff_stride, int32_t cutoff_rows,
                                      const double* gain, int32_t gain_stride, int32_t gain_rows,
                                      const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                                      double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream)
{
    FusedCall c{osc_kind, filt_type, rate, position, block_frames, nblocks, context, voices, hertz, hertz_stride, phase, phase_stride,
                cutoff, cutoff_stride, gain, gain_stride, out, out_ld, status, stream};
    set_rows(c, cutoff_rows, gain_rows);
    set_fm(c, hertz_rows, hertz_hist, phase_rows, phase_hist);
    set_bus(c, bus_gains, bus_gains_ld, bus_channels, workspace);
    return run_call(c);
}

extern "C" int sig_fused_osc_biquad_devpos(int osc_kind, int filt_type, int32_t rate, const int64_t* position_dev,
                                           int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                           const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                                           const double* cutoff, int32_t cutoff_stride,
                                           const double* gain, int32_t gain_stride,
                                           float* out, int64_t out_ld, int32_t* status, void* stream)
{
    FusedCall c{osc_kind, filt_type, rate, 0, block_frames, nblocks, context, voices, hertz, hertz_stride, phase, phase_stride,
                cutoff, cutoff_stride, gain, gain_stride, out, out_ld, status, stream};
    c.devpos = true; c.position_dev = position_dev;
    return run_call(c);
}

namespace {
__global__ void advance_kernel(int64_t* p, int64_t delta) { *p += delta; }
}  // namespace

extern "C" int sig_advance_position(int64_t* position_dev, int64_t delta, void* stream)
{
    SIG_CHECK_ARG(position_dev != nullptr);
    advance_kernel<<<1, 1, 0, static_cast<hipStream_t>(stream)>>>(position_dev, delta);
    return sig_launch_status();
}

extern "C" int sig_fused_osc_biquad_mix(int osc_kind, int filt_type, int32_t rate, int64_t position,
                                        int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                        const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                                        const double* cutoff, int32_t cutoff_stride,
                                        const double* gain, int32_t gain_stride,
                                        const float* matrix, float* out, int64_t out_ld, int32_t* status, void* stream)
{
    FusedCall c{osc_kind, filt_type, rate, position, block_frames, nblocks, context, voices, hertz, hertz_stride, phase, phase_stride,
                cutoff, cutoff_stride, gain, gain_stride, out, out_ld, status, stream};
    c.sink = SINK_MIX; c.matrix = matrix;
    return run_call(c);
}

extern "C" int sig_fused_geometry(int32_t voices, int32_t block_frames, int32_t nblocks, int32_t context,
                                  int32_t* voices_per_lane, int32_t* blocks_per_lane)
{
    SIG_CHECK_ARG(voices >= 0 && block_frames >= 0 && nblocks >= 0 && context >= 0 && voices_per_lane && blocks_per_lane);
    FusedArgs a{};
    a.N = block_frames; a.K = nblocks; a.ctx = context; a.voices = voices;
    int vpt = 1, span = 1;
    pick_geometry(a, 4, vpt, span);
    *voices_per_lane = vpt;
    *blocks_per_lane = span;
    return 0;
}

extern "C" int sig_fused_voice_bus_plan(int osc_kind, int64_t position, int32_t voices, int32_t block_frames, int32_t nblocks,
                                       int32_t context, int32_t* voices_per_lane, int32_t* blocks_per_lane,
                                       int32_t* closed_form)
{
    SIG_CHECK_ARG(voices >= 0 && block_frames >= 0 && nblocks >= 0 && context >= 0 && position >= 0);
    SIG_CHECK_ARG(voices_per_lane && blocks_per_lane && closed_form);
    FusedArgs a{};
    a.position = position; a.N = block_frames; a.K = nblocks; a.ctx = context; a.voices = voices;
    const BusPlan p = plan_voice_bus(a, osc_kind);
    *voices_per_lane = p.vpt;
    *blocks_per_lane = p.span;
    *closed_form = p.steady;
    return 0;
}

extern "C" int sig_fused_set_tuning(int32_t voices_per_lane, int32_t blocks_per_lane, int32_t closed_form, int32_t scan)
{
    SIG_CHECK_ARG(voices_per_lane >= 0 && blocks_per_lane >= 0 && closed_form >= -1 && closed_form <= 3 && scan >= -1);
    Tuning& t = tuning();
    t.vpt = voices_per_lane; t.span = blocks_per_lane; t.scan = scan;
    t.steady = (closed_form == 2 || closed_form == 3) ? 1 : closed_form;       // 2: closed form on, voice tiles added by partials_kernel
    t.tile_sum_kernel = (closed_form == 2) ? 1 : 0;
    t.mix_f32 = (closed_form == 3) ? 1 : 0;                                    // 3: closed form on, the MixMatrix sink on v_mfma_f32_32x32x2_f32
    return 0;
}

extern "C" int64_t sig_fused_voice_bus_workspace(int32_t voices, int64_t rows, int32_t bus_channels)
{
    return (steady_consts_offset(voices, rows, bus_channels) + (int64_t)kSteadyConsts * voices) * (int64_t)sizeof(double);
}

extern "C" int sig_fused_voice_bus(int osc_kind, int filt_type, int32_t rate, int64_t position,
                                   int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                   const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                                   const double* cutoff, int32_t cutoff_stride,
                                   const double* gain, int32_t gain_stride,
                                   const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                                   double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream)
{
    FusedCall c{osc_kind, filt_type, rate, position, block_frames, nblocks, context, voices, hertz, hertz_stride, phase, phase_stride,
                cutoff, cutoff_stride, gain, gain_stride, out, out_ld, status, stream};
    set_bus(c, bus_gains, bus_gains_ld, bus_channels, workspace);
    return run_call(c);
}

extern "C" int sig_fused_voice_bus_walk(int osc_kind, int filt_type, int32_t rate, int64_t position,
                                        int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                        const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                                        const double* cutoff, int32_t cutoff_stride,
                                        const double* gain, int32_t gain_stride,
                                        const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                                        double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream)
{
    FusedCall c{osc_kind, filt_type, rate, position, block_frames, nblocks, context, voices, hertz, hertz_stride, phase, phase_stride,
                cutoff, cutoff_stride, gain, gain_stride, out, out_ld, status, stream};
    set_bus(c, bus_gains, bus_gains_ld, bus_channels, workspace);
    c.force_walk = 1;
    return run_call(c);
}

extern "C" int64_t sig_fused_voice_consts_size(int32_t voices)
{
    return (int64_t)kSteadyConsts * voices * (int64_t)sizeof(double);
}

extern "C" int sig_fused_voice_bus_prepared(int osc_kind, int filt_type, int32_t rate, int64_t position,
                                            int32_t block_frames, int32_t nblocks, int32_t context, int32_t voices,
                                            const double* hertz, int32_t hertz_stride, const double* phase, int32_t phase_stride,
                                            const double* cutoff, int32_t cutoff_stride,
                                            const double* gain, int32_t gain_stride,
                                            const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                                            double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream,
                                            double* consts, int32_t consts_ready)
{
    SIG_CHECK_ARG(consts != nullptr);
    FusedCall c{osc_kind, filt_type, rate, position, block_frames, nblocks, context, voices, hertz, hertz_stride, phase, phase_stride,
                cutoff, cutoff_stride, gain, gain_stride, out, out_ld, status, stream};
    set_bus(c, bus_gains, bus_gains_ld, bus_channels, workspace);
    c.consts = consts; c.consts_ready = consts_ready;
    return run_call(c);
}

// sig_fused_voice_bus_prepared / _walk with everything but the position, the output and the stream in a caller-held block: a
// host binding that marshals every argument per call (ctypes: ~5 us for the 26 of them) pays that once
extern "C" int sig_fused_voice_bus_bound(const sig_fused_voice_bus_call* b, int64_t position, float* out, int32_t consts_ready,
                                         int32_t walk, void* stream)
{
    SIG_CHECK_ARG(b != nullptr && (walk || b->consts != nullptr));
    FusedCall c{b->osc_kind, b->filt_type, b->rate, position, b->block_frames, b->nblocks, b->context, b->voices, b->hertz, b->hertz_stride,
                b->phase, b->phase_stride, b->cutoff, b->cutoff_stride, b->gain, b->gain_stride, out, b->out_ld, b->status, stream};
    set_bus(c, b->bus_gains, b->bus_gains_ld, b->bus_channels, b->workspace);
    if (walk) c.force_walk = 1;
    else { c.consts = b->consts; c.consts_ready = consts_ready; }
    return run_call(c);
}
