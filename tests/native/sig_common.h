// Host stand-in for signals_amd/csrc/sig_common.h, for compiling sig_adsr.h and sig_noise.h with the host compiler
// (tests/native/adsr_tracker.cpp, tests/native/noise_hash.cpp): the device qualifiers go away, the math is the C library's.
#pragma once
#include <math.h>
#include <stdint.h>

#define __device__
#define __forceinline__ inline
