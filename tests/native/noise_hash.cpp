// Host evaluation of sig_noise::noise_bits / noise_value (signals_amd/csrc/sig_noise.h) for tests/test_oracle_white.py.
// Compiled against a copy of the header next to the stub sig_common.h that defines the device qualifiers away.
//
// Input (native endianness): int64 groups, then per group  uint64 seed;  int64 position, frames, channels.
// Output per group:  uint32 bits[frames][channels];  float value[frames][channels].
#include <cstdio>
#include <cstdint>
#include <vector>

#include "sig_noise.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 2; }
    int64_t groups = 0;
    if (fread(&groups, sizeof groups, 1, in) != 1) return 3;
    for (int64_t g = 0; g < groups; ++g) {
        uint64_t seed;
        int64_t hdr[3];
        if (fread(&seed, sizeof seed, 1, in) != 1 || fread(hdr, sizeof(int64_t), 3, in) != 3) return 3;
        const int64_t position = hdr[0], frames = hdr[1], channels = hdr[2];
        std::vector<uint32_t> bits(frames * channels);
        std::vector<float> value(frames * channels);
        for (int64_t r = 0; r < frames; ++r)
            for (int64_t c = 0; c < channels; ++c) {
                bits[r * channels + c] = sig_noise::noise_bits(seed, position + r, (int)c);
                value[r * channels + c] = sig_noise::noise_value(seed, position + r, (int)c);
            }
        fwrite(bits.data(), sizeof(uint32_t), bits.size(), out);
        fwrite(value.data(), sizeof(float), value.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
