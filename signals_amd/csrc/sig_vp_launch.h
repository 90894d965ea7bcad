// Launching the voice-program interpreter (sig_vp_machine.h): internal to the library, not part of the C ABI.
//
// VpLaunch<F>::run starts the kernel of family F for a register file, voices per lane and sink chosen at run time.  Its 12 kernels
// (2 voices per lane x 2 register files x 3 sinks) are instantiated in the ONE file that has F's SIG_VP_INSTANTIATE line, so that
// no translation unit carries more than a family or two and the files build side by side; every other unit -- voice_program.hip,
// the caller -- sees the declarations at the end of this header.  A new family: a name in vp_family, a line there and below, a file.
#pragma once
#include <hip/hip_runtime.h>

#include "sig_vp_machine.h"

namespace {

using namespace sig_vp;

template <int VPT, bool SMALL, int C, typename F>
void vp_start(const VpArgs& a, const typename F::Extra& extra, unsigned nwg, size_t lds, hipStream_t s) {
    if constexpr (std::is_same_v<typename F::Extra, VpNoTables>) voice_program_kernel<VPT, SMALL, C, F><<<nwg, 256, lds, s>>>(a);
    else voice_program_kernel<VPT, SMALL, C, F><<<nwg, 256, lds, s>>>(a, extra);
}

template <int VPT, bool SMALL, typename F>
int vp_launch(const VpArgs& a, const typename F::Extra& extra, int C, unsigned nwg, size_t lds, hipStream_t s) {
    switch (C) {
        case 0: vp_start<VPT, SMALL, 0, F>(a, extra, nwg, lds, s); break;
        case 1: vp_start<VPT, SMALL, 1, F>(a, extra, nwg, lds, s); break;
        case 2: vp_start<VPT, SMALL, 2, F>(a, extra, nwg, lds, s); break;
        default: return (int)hipErrorInvalidValue;
    }
    return sig_launch_status();
}

}  // namespace

namespace sig_vp {

template <typename F>
struct __attribute__((visibility("hidden"))) VpLaunch {
    // C: bus channels (0: store).  Returns 0 or a hipError_t.
    static int run(const VpArgs& a, const typename F::Extra& extra, int voices_per_lane, bool small_file, int C, unsigned nwg, size_t lds,
                   hipStream_t s);
};

template <typename F>
int VpLaunch<F>::run(const VpArgs& a, const typename F::Extra& extra, int voices_per_lane, bool small_file, int C, unsigned nwg, size_t lds,
                     hipStream_t s) {
    switch ((voices_per_lane == 2 ? 2 : 0) + (small_file ? 1 : 0)) {
        case 0: return vp_launch<1, false, F>(a, extra, C, nwg, lds, s);
        case 1: return vp_launch<1, true, F>(a, extra, C, nwg, lds, s);
        case 2: return vp_launch<2, false, F>(a, extra, C, nwg, lds, s);
        default: return vp_launch<2, true, F>(a, extra, C, nwg, lds, s);
    }
}

// in vp_<family>.hip: the definition of that family's launch, and with it its kernels
#define SIG_VP_INSTANTIATE(name) template struct sig_vp::VpLaunch<sig_vp::vp_family::name>;

extern template struct VpLaunch<vp_family::plain>;
extern template struct VpLaunch<vp_family::band>;
extern template struct VpLaunch<vp_family::pm>;
extern template struct VpLaunch<vp_family::table>;
extern template struct VpLaunch<vp_family::shape>;
extern template struct VpLaunch<vp_family::resonant>;
extern template struct VpLaunch<vp_family::unison>;
extern template struct VpLaunch<vp_family::blep>;
extern template struct VpLaunch<vp_family::mixed>;
extern template struct VpLaunch<vp_family::resonant_eq>;
extern template struct VpLaunch<vp_family::mixed_eq>;
extern template struct VpLaunch<vp_family::sync>;
extern template struct VpLaunch<vp_family::mixed_sync>;

}  // namespace sig_vp
