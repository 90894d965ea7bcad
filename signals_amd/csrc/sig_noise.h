// White noise hash shared by noise.hip and control_program.hip: a sample is a function of (seed, frame, channel) only, so a
// block is the same whatever launch geometry or position batching produced it.  One 64-bit mix per PAIR of adjacent channels
// (high and low words).
#pragma once
#include "sig_common.h"

namespace sig_noise {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint32_t noise_bits(uint64_t seed, int64_t frame, int channel) {
    const uint64_t h = mix64(seed + (uint64_t)frame * 0x9E3779B97F4A7C15ULL + (uint64_t)(channel >> 1) * 0xD1B54A32D192ED03ULL);
    return (channel & 1) ? (uint32_t)(h >> 32) : (uint32_t)h;
}

// uniform [0, 1): the top 24 bits times 2^-24, exact in float32 (and so the same value stored as float32 or float64)
__device__ __forceinline__ float noise_value(uint64_t seed, int64_t frame, int channel) {
    return (float)(noise_bits(seed, frame, channel) >> 8) * 5.9604644775390625e-8f;
}

}  // namespace sig_noise
