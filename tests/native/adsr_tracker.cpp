// Host walk of sig_env::segment_at (signals_amd/csrc/sig_adsr.h) the way the forward-walking kernels use it, for
// tests/test_adsr_tracker_host.py.  Compiled against a copy of the header next to a stub sig_common.h that defines the
// device qualifiers away; -O2 -ffp-contract=off, as the device code is built.
//
// Per voice and row n of [start, start + frames):  t = n / rate;  re-derive the stage when !(t < end);  the level is
// fma(slope, t - t0, l0) (voice_program.hip's form).  Input (native endianness): int64 groups, then per group
//     int64 start, frames, voices, probes;  double rate;  double params[6][voices];  int64 probe_frames[probes]
// (params in sig_env::AdsrRows order: attack, decay, sustain, release, gate_on, gate_off).  Output per group:
//     double tracked[probes][voices];  double level[probes][voices];  double max_abs_diff[voices]
// -- the tracked level and the header's level() at the probe rows, and max |tracked - level()| over every row walked.
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <vector>

#include "sig_adsr.h"

template <typename T> static bool get(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <typename T> static void put(FILE* f, const T* p, size_t n) { fwrite(p, sizeof(T), n, f); }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 2; }
    int64_t groups = 0;
    if (!get(in, &groups, 1)) return 3;
    for (int64_t g = 0; g < groups; ++g) {
        int64_t hdr[4];
        double rate;
        if (!get(in, hdr, 4) || !get(in, &rate, 1)) return 3;
        const int64_t start = hdr[0], frames = hdr[1], V = hdr[2], P = hdr[3];
        std::vector<double> params(6 * V);
        std::vector<int64_t> probes(P);
        if (!get(in, params.data(), params.size()) || !get(in, probes.data(), probes.size())) return 3;
        std::vector<double> tracked(P * V), level(P * V), maxdiff(V, 0.0);
        for (int64_t v = 0; v < V; ++v) {
            sig_env::AdsrRows rows;
            for (int i = 0; i < 6; ++i) { rows.p[i] = &params[i * V + v]; rows.s[i] = 0; }
            const sig_env::Voice p = sig_env::load_voice(rows, 0);
            sig_env::Segment s{0.0, 0.0, 0.0, -1.0};             // derived at the first row
            int64_t k = 0;
            for (int64_t n = start; n < start + frames; ++n) {
                const double t = (double)n / rate;
                if (!(t < s.end)) s = sig_env::segment_at(p, t);
                const double x = fma(s.slope, t - s.t0, s.l0);
                const double ref = sig_env::level(p, t);
                const double d = std::fabs(x - ref);
                if (!(d <= maxdiff[v])) maxdiff[v] = d;            // (NaN sticks)
                while (k < P && probes[k] < n) ++k;
                for (int64_t j = k; j < P && probes[j] == n; ++j) { tracked[j * V + v] = x; level[j * V + v] = ref; }
            }
        }
        put(out, tracked.data(), tracked.size());
        put(out, level.data(), level.size());
        put(out, maxdiff.data(), maxdiff.size());
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
