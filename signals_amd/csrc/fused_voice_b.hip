// The fused voice chain's second translation unit: the span walkers of Square, Sawtooth and Triangle (sig_fused_walk.h) behind
// four plain functions, which fused_voice.hip's dispatchers call (sig_fused_launch.h: dispatch_osc_kind).  Two units because one
// took 4 min 50 s to compile (240 walker instantiations + the closed form); they build in parallel.
#define SIG_FUSED_PART_B 1
#include "sig_fused_launch.h"

namespace sig_fused {
int part_b_rows(int C, int kind, const FusedArgs& a, const BusArgs& bus, float* out, int64_t out_ld, hipStream_t s) {
    return dispatch_rows(C, kind, a, bus, out, out_ld, s);
}
int part_b_bus(int gain, int kind, int C, const FusedArgs& a, const BusArgs& bus, float* out, int64_t out_ld, hipStream_t s) {
    return dispatch_bus(gain != 0, kind, C, a, bus, out, out_ld, s);
}
int part_b_mix(int gain, int kind, const FusedArgs& a, hipStream_t s) { return dispatch_mix(gain != 0, kind, a, s); }
int part_b_chain(int gain, int kind, const FusedArgs& a, hipStream_t s) { return dispatch_chain(gain != 0, kind, a, s); }
}  // namespace sig_fused
