// The voice-program interpreter (sig_vp_machine.h), family `mixed_sync` (MIXED + the OscSync word): its 12 kernels and their launch.
#include "sig_vp_launch.h"

SIG_VP_INSTANTIATE(mixed_sync)
