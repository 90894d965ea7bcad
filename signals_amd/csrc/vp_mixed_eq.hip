// The voice-program interpreter (sig_vp_machine.h), family `mixed_eq` (MIXED + the FilterEq word): its 12 kernels and their launch.
#include "sig_vp_launch.h"

SIG_VP_INSTANTIATE(mixed_eq)
