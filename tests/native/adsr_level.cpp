// Host evaluation of sig_env::make_voice + sig_env::level (signals_amd/csrc/sig_adsr.h) at single frames, the way the control
// program's SIG_CTL_ADSR word uses them, for tests/test_control_adsr_host.py.  Compiled against a copy of the header next to the
// stub sig_common.h that defines the device qualifiers away; -O2 -ffp-contract=off, as the device code is built.
//
// Input (native endianness):  int64 voices, positions;  double rate;  double params[6][voices] (attack, decay, sustain, release,
// gate_on, gate_off);  int64 position[positions].  Output:  double level[positions][voices] with t = (double)position / rate.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "sig_adsr.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 2; }
    int64_t hdr[2];
    double rate;
    if (fread(hdr, sizeof(int64_t), 2, in) != 2 || fread(&rate, sizeof(double), 1, in) != 1) return 3;
    const int64_t V = hdr[0], P = hdr[1];
    if (V < 1 || P < 0) return 3;
    std::vector<double> params(6 * V), level(P * V);
    std::vector<int64_t> positions(P);
    if (fread(params.data(), sizeof(double), params.size(), in) != params.size()) return 3;
    if (fread(positions.data(), sizeof(int64_t), positions.size(), in) != positions.size()) return 3;
    for (int64_t v = 0; v < V; ++v) {
        const sig_env::Voice p = sig_env::make_voice(params[0 * V + v], params[1 * V + v], params[2 * V + v], params[3 * V + v],
                                                     params[4 * V + v], params[5 * V + v]);
        for (int64_t k = 0; k < P; ++k) level[k * V + v] = sig_env::level(p, (double)positions[k] / rate);
    }
    fwrite(level.data(), sizeof(double), level.size(), out);
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
