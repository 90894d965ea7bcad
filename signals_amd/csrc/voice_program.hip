// The voice program's HOST half: tuning, attached images, geometry, validation, launch and the C entries of the accumulator
// machine in sig_vp_machine.h (read that first).  The interpreter's kernels live one family per file (vp_<family>.hip) and are
// reached through sig_vp_launch.h; this file instantiates none of them.
//
// Built with -DSIG_VP_STATIC_CODE={words} (signals_amd/specialise.py) this file is instead ONE kernel: the machine specialised
// for one program, below.
#include <cstring>
#include <mutex>
#include <tuple>
#include <vector>

#include "sig_vp_machine.h"

#ifdef SIG_VP_STATIC_CODE
// A SPECIALISED build of this file (signals_amd/specialise.py: hipcc --genco with the program, the exact register file, the
// voices per lane and the sink as macros): one kernel, the same source as the interpreter with the program a compile-time
// constant -- the dispatch loop unrolls and every switch folds.  Attached to the library with sig_voice_program_attach.
namespace {
// does the program this file is specialised for have an instruction with this opcode?
constexpr bool vp_static_has(int op) {
    constexpr uint32_t c[] = SIG_VP_STATIC_CODE;
    for (unsigned k = 0; k < sizeof(c) / sizeof(c[0]); ++k)
        if ((c[k] & 31u) == (uint32_t)op) return true;
    return false;
}
}  // namespace
#ifndef SIG_VP_S_TAB
#define SIG_VP_S_TAB 0                     // 1: the program has an OscTable or a Shape word, the kernel takes the tables as a second parameter
#endif
#ifndef SIG_VP_S_UNI
#define SIG_VP_S_UNI 0                     // 1: the program has an OscUni word, the kernel takes the copies as a second parameter
#endif
#ifndef SIG_VP_S_BLEP
#define SIG_VP_S_BLEP 0                    // 1: the program has an OscBlep word (with -DSIG_VP_S_UNI=1: the same copies parameter)
#endif
#ifndef SIG_VP_S_SYNC
#define SIG_VP_S_SYNC 0                    // 1: the program has an OscSync word (with -DSIG_VP_S_UNI=1: the same copies parameter; the band-limited residual comes with it)
#endif
#ifndef SIG_VP_S_MIXED
#define SIG_VP_S_MIXED 0                   // 1: the program combines two or more of Band, OscPM, OscTable / Shape, FilterQ, OscUni; the kernel takes a VpMixed
#endif
#ifndef SIG_VP_S_RES
#define SIG_VP_S_RES 0                     // 1: the program has a FilterQ or a FilterEq word (the resonant design)
#endif
#ifndef SIG_VP_S_EQ
#define SIG_VP_S_EQ 0                      // 1: the program has a FilterEq word (with -DSIG_VP_S_RES=1: the general numerator on top of it)
#endif
extern "C" __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SIG_VP_STATIC_WAVES, 8)))
#if SIG_VP_S_MIXED
void sig_vp_specialised(VpArgs a, VpMixed extra)
#elif SIG_VP_S_TAB
void sig_vp_specialised(VpArgs a, VpTables extra)
#elif SIG_VP_S_UNI
void sig_vp_specialised(VpArgs a, VpUnison extra)
#else
void sig_vp_specialised(VpArgs a)
#endif
{
    constexpr bool kBand = vp_static_has(SIG_VP_BAND), kPm = vp_static_has(SIG_VP_OSCPM), kShape = vp_static_has(SIG_VP_SHAPE);
    constexpr bool kTab = vp_static_has(SIG_VP_OSCTABLE) || kShape;
    constexpr bool kEq = vp_static_has(SIG_VP_FILTEREQ);
    constexpr bool kRes = vp_static_has(SIG_VP_FILTERQ) || kEq;                // (one family: FilterEq reads FilterQ's q rows)
    static_assert(kRes == (SIG_VP_S_RES != 0), "a program with a FilterQ or a FilterEq word is built with -DSIG_VP_S_RES=1, any other without");
    static_assert(kEq == (SIG_VP_S_EQ != 0), "a program with a FilterEq word is built with -DSIG_VP_S_EQ=1, any other without");
    static_assert(kTab == (SIG_VP_S_TAB != 0), "a program with an OscTable or a Shape word is built with -DSIG_VP_S_TAB=1, any other without");
    constexpr bool kBlep = vp_static_has(SIG_VP_OSCBLEP);
    constexpr bool kSync = vp_static_has(SIG_VP_OSCSYNC);
    constexpr bool kUni = vp_static_has(SIG_VP_OSCUNI) || kBlep || kSync;      // (one family: OscBlep and OscSync read OscUni's copies)
    static_assert(kUni == (SIG_VP_S_UNI != 0), "a program with an OscUni, an OscBlep or an OscSync word is built with -DSIG_VP_S_UNI=1, any other without");
    static_assert(kBlep == (SIG_VP_S_BLEP != 0), "a program with an OscBlep word is built with -DSIG_VP_S_BLEP=1, any other without");
    static_assert(kSync == (SIG_VP_S_SYNC != 0), "a program with an OscSync word is built with -DSIG_VP_S_SYNC=1, any other without");
    static_assert(!(kSync && kEq), "OscSync with FilterEq: no kernel set has both");
    constexpr int kFamilies = (int)kBand + (int)kPm + (int)kTab + (int)kRes + (int)kUni;
    static_assert((kFamilies >= 2) == (SIG_VP_S_MIXED != 0), "a program with two or more of Band, OscPM, OscTable / Shape, FilterQ and OscUni is built with -DSIG_VP_S_MIXED=1, any other without");
#if !SIG_VP_S_MIXED
    static_assert(!(kRes && (kTab || kBand || kPm)), "FilterQ with Band, OscPM, OscTable or Shape: no variant has both");
    static_assert(!(kUni && (kTab || kBand || kPm || kRes)), "OscUni with Band, OscPM, OscTable, Shape or FilterQ: no variant has both");
    static_assert(!(kBand && kPm) && !(kTab && (kBand || kPm)), "Band, OscPM and OscTable / Shape: no variant has two of them");
#endif
    using F = VpFamily<kBand, kPm, kTab, kShape, kRes, kUni, kBlep || kSync, kEq, kSync>;   // exactly the families the program has (SYN sits on top of BLP)
#if SIG_VP_S_MIXED || SIG_VP_S_TAB || SIG_VP_S_UNI
    static_assert(std::is_same_v<F::Extra, decltype(extra)>, "the second kernel parameter is the one the program's families take");
    vp_kernel_body<SIG_VP_STATIC_VPT, true, SIG_VP_STATIC_C, F>(a, extra);
#else
    vp_kernel_body<SIG_VP_STATIC_VPT, true, SIG_VP_STATIC_C, F>(a, VpNoTables{});
#endif
}
// what the attaching library checks before it trusts the image: the argument block's size and the program it was built for
extern "C" __global__ void sig_vp_specialised_info(uint32_t* out)
{
    constexpr uint32_t code[] = SIG_VP_STATIC_CODE;
    out[0] = (uint32_t)sizeof(VpArgs); out[1] = SIG_VP_STATIC_VPT; out[2] = SIG_VP_STATIC_C; out[3] = (uint32_t)(sizeof(code) / sizeof(code[0]));
    for (unsigned k = 0; k < sizeof(code) / sizeof(code[0]); ++k) out[4 + k] = code[k];
}
#else
#include "sig_vp_launch.h"

namespace {

struct VpTuning { int vpt = 0, span = 0, attached = 1; };
VpTuning& vp_tuning() { static VpTuning t; return t; }

// Specialised kernels attached at run time (sig_voice_program_attach): this file built once more for ONE program, found again
// by the program's words, the slot counts, the voices per lane and the sink.  Entries are never removed while launches may be
// in flight (detach is for tests and process exit); the list is short, a linear search costs less than the launch.
struct VpSpecial { uint32_t code[kMaxIns]; int n_ins, n_oscs, n_params, n_filters, n_temps, vpt, C; hipModule_t mod; hipFunction_t fn; };
std::vector<VpSpecial>& vp_specials() { static std::vector<VpSpecial> v; return v; }
std::mutex& vp_specials_lock() { static std::mutex m; return m; }

// ---- the two rules about words, each written once
// may this word's c be -1?  (no select / no q / no spread; encoded as 15, a slot number no register file has)
constexpr bool vp_c_optional(int op) {
    return op == SIG_VP_OSCTABLE || op == SIG_VP_SHAPE || op == SIG_VP_FILTERQ || op == SIG_VP_OSCUNI || op == SIG_VP_OSCBLEP ||
           op == SIG_VP_FILTEREQ || op == SIG_VP_OSCSYNC;
}
// ... and its b?  (FilterEq: no gain; OscSync: no ratio)
constexpr bool vp_b_optional(int op) { return op == SIG_VP_FILTEREQ || op == SIG_VP_OSCSYNC; }
// the variant that has this word's handler and no other extension word's (SIG_VP_FAMILY_*; PLAIN: every variant has it)
constexpr int vp_word_family(int op) {
    switch (op) {
        case SIG_VP_BAND: return SIG_VP_FAMILY_BAND;
        case SIG_VP_OSCPM: return SIG_VP_FAMILY_PM;
        case SIG_VP_OSCTABLE: return SIG_VP_FAMILY_TABLE;
        case SIG_VP_SHAPE: return SIG_VP_FAMILY_SHAPE;
        case SIG_VP_FILTERQ: return SIG_VP_FAMILY_RESONANT;
        case SIG_VP_FILTEREQ: return SIG_VP_FAMILY_RESONANT;                   // (the same family and exclusions; its kernels: VpNeeds::eq)
        case SIG_VP_OSCUNI: return SIG_VP_FAMILY_UNISON;
        case SIG_VP_OSCBLEP: return SIG_VP_FAMILY_BLEP;
        case SIG_VP_OSCSYNC: return SIG_VP_FAMILY_BLEP;                        // (the same family and exclusions; its kernels: VpNeeds::sync)
        default: return SIG_VP_FAMILY_PLAIN;
    }
}

bool vp_word_ok(const sig_vp_ins& x) {
    return x.op >= SIG_VP_OSC && x.op <= SIG_VP_OSCSYNC && x.kind >= 0 && x.kind <= 7 && x.a >= 0 && x.a <= 15 &&
           x.b >= (vp_b_optional(x.op) ? -1 : 0) && x.b <= 15 &&
           x.c >= (vp_c_optional(x.op) ? -1 : 0) && x.c <= 15;
}

bool vp_encode(const sig_voice_program_t& P, uint32_t* code) {
    for (int k = 0; k < P.n_ins; ++k) {
        const sig_vp_ins& x = P.ins[k];
        if (!vp_word_ok(x)) return false;
        code[k] = (uint32_t)x.op | ((uint32_t)x.kind << 5) | ((uint32_t)x.a << 8) | ((uint32_t)(x.b & 15) << 12) | ((uint32_t)(x.c & 15) << 16);
    }
    return true;
}

hipFunction_t vp_find_special(const VpArgs& a, const sig_voice_program_t& P, int vpt, int C) {
    if (!vp_tuning().attached) return nullptr;
    std::lock_guard<std::mutex> g(vp_specials_lock());
    for (const VpSpecial& e : vp_specials())
        if (e.n_ins == a.n_ins && e.vpt == vpt && e.C == C && e.n_oscs == P.n_oscs && e.n_params == P.n_params &&
            e.n_filters == P.n_filters && e.n_temps == P.n_temps && memcmp(e.code, a.code, sizeof(uint32_t) * a.n_ins) == 0)
            return e.fn;
    return nullptr;
}

// What a program asks of the machine: slots, the extended handlers (Amp, ADSR, White), and `words`: bit f is set when the program
// has a word of family f (vp_word_family).
struct VpNeeds {
    int oscs, params, temps, filters; bool ext, adsr; unsigned words;
    bool eq;                                                                   // a FilterEq word: the RES+EQ / MIXED+EQ kernels (vp_family::resonant_eq, mixed_eq)
    bool sync;                                                                 // an OscSync word: the BLP+SYN / MIXED+SYN kernels (vp_family::sync, mixed_sync)
    bool has(int family) const { return (words >> family) & 1u; }
    bool table() const { return has(SIG_VP_FAMILY_TABLE) || has(SIG_VP_FAMILY_SHAPE); }      // (Shape sits on top of the table family)
    bool uni() const { return has(SIG_VP_FAMILY_UNISON) || has(SIG_VP_FAMILY_BLEP); }        // (OscBlep: the unison family, the same copies, the same exclusions)
    // the families of which every single-family variant has one
    int families() const { return (int)has(SIG_VP_FAMILY_BAND) + (int)has(SIG_VP_FAMILY_PM) + (int)table() + (int)has(SIG_VP_FAMILY_RESONANT) + (int)uni(); }
};

VpNeeds vp_needs(const sig_voice_program_t& P) {              // (n_ins was checked; any op may stand in a word)
    VpNeeds n{P.n_oscs, P.n_params, P.n_temps, P.n_filters, false, false, 0u, false, false};
    for (int k = 0; k < P.n_ins; ++k) {
        const int op = P.ins[k].op;
        if (op == SIG_VP_AMP || op == SIG_VP_ADSR || op == SIG_VP_NOISE) n.ext = true;
        if (op == SIG_VP_ADSR) n.adsr = true;
        if (op == SIG_VP_FILTEREQ) n.eq = true;
        if (op == SIG_VP_OSCSYNC) n.sync = true;
        n.words |= 1u << vp_word_family(op);
    }
    return n;
}

bool fits_small(const VpNeeds& n) {
    using L = VpLimits<true>;
    return n.oscs <= L::NO && n.params <= L::NP && n.temps <= L::NT && n.filters <= L::NF && !n.ext;
}

// The variant a program runs in (SIG_VP_FAMILY_*): two or more families: MIXED (a table never with a band or a PM carrier, a PM
// carrier never with a band, a resonant filter or a unison oscillator with none of them nor with each other: refused by every
// entry but sig_voice_program_mixed); else the one variant that has every word of the program.
int vp_variant(const VpNeeds& n) {
    if (n.families() >= 2) return SIG_VP_FAMILY_MIXED;
    for (int f : {SIG_VP_FAMILY_BLEP, SIG_VP_FAMILY_UNISON, SIG_VP_FAMILY_RESONANT, SIG_VP_FAMILY_SHAPE, SIG_VP_FAMILY_TABLE,
                  SIG_VP_FAMILY_PM, SIG_VP_FAMILY_BAND})
        if (n.has(f)) return f;
    return SIG_VP_FAMILY_PLAIN;
}

// f(descriptor) for a SIG_VP_FAMILY_* value
template <typename Fn>
int vp_with_family(int variant, Fn&& f) {
    switch (variant) {
        case SIG_VP_FAMILY_PLAIN: return f(vp_family::plain{});
        case SIG_VP_FAMILY_BAND: return f(vp_family::band{});
        case SIG_VP_FAMILY_PM: return f(vp_family::pm{});
        case SIG_VP_FAMILY_TABLE: return f(vp_family::table{});
        case SIG_VP_FAMILY_SHAPE: return f(vp_family::shape{});
        case SIG_VP_FAMILY_RESONANT: return f(vp_family::resonant{});
        case SIG_VP_FAMILY_UNISON: return f(vp_family::unison{});
        case SIG_VP_FAMILY_BLEP: return f(vp_family::blep{});
        case SIG_VP_FAMILY_MIXED: return f(vp_family::mixed{});
        default: return (int)hipErrorInvalidValue;
    }
}

// voices per lane and blocks per lane.  4 voices per lane amortise the interpreter's scalar work best; a lane's span
// re-walks (depth - 1) blocks + the context once, so longer spans waste less -- while the launch still has a wave or two
// for every SIMD
// `four`: a kernel SPECIALISED for four voices per lane is at hand (the interpreter exists for 1 and 2): straight-line code
// keeps a lone wave per SIMD busy, and the bus flush and the row's n / rate are paid per lane -- taken when the store is
// 16-byte aligned (or there is a bus) and the launch still has a wave for every SIMD
void vp_geometry(const VpArgs& a, int store_aligned, bool four, int& vpt, int& span) {
    auto waves = [&](int v, int s) { return sig_span_waves(sig_voice_tiles(a.voices, v), a.K, s); };
    const bool bus = a.partials != nullptr;
    vpt = ((bus || store_aligned >= 2) && waves(2, 1) >= 1024) ? 2 : 1;
    const bool can4 = four && (bus || store_aligned >= 4);
    if (can4 && waves(4, 1) >= 1024) vpt = 4;
    const int t = vp_tuning().vpt;
    if (t == 1 || (t == 2 && (bus || store_aligned >= 2)) || (t == 4 && can4)) vpt = t;
    span = 1;
    if (!a.small) {
        span = 16;
        while (span > 1 && waves(vpt, span) < (vpt == 4 ? 1024 : 2048)) span >>= 1;
        if (vp_tuning().span >= 1) span = vp_tuning().span;
    }
}

// what sig_voice_program and its three extensions are called with
struct VpRequest {
    const sig_voice_program_t* program; int32_t rate; int64_t position; int32_t block_frames, nblocks, context, voices, control_rows;
    int32_t hist_blocks; const int64_t* hist_positions; int32_t blocks_before;
    const double* bus_gains; int64_t bus_gains_ld; int32_t bus_channels;
    double* workspace; float* out; int64_t out_ld; int32_t* status; void* stream;
    const sig_vp_tables_t* tables; const sig_vp_unison_t* unison;
    bool allow_mixed;                                                          // sig_voice_program_mixed: the three exclusivity checks are off
};

// a checked call: the kernels' arguments, but for the geometry
struct VpCall {
    bool empty;                                                                // nothing to render (and nothing below is filled)
    VpArgs a; VpNeeds need; size_t table_lds;
    std::tuple<VpNoTables, VpTables, VpUnison, VpMixed> extra;                 // the second kernel parameter, by family (VpFamily::Extra)
};

// Checks the call and the program and fills `c`.  Host only: no HIP call.
int vp_check(const VpRequest& r, VpCall& c)
{
    const sig_vp_tables_t* tables = r.tables;
    const sig_vp_unison_t* unison = r.unison;
    SIG_CHECK_ARG(!unison || (unison->copies >= 1 && unison->copies <= SIG_UNISON_MAX_COPIES));
    SIG_CHECK_ARG(r.program && r.rate > 0 && r.position >= 0 && r.block_frames >= 0 && r.nblocks >= 0 && r.context >= 0 && r.voices >= 0);
    SIG_CHECK_ARG(r.out && (r.bus_channels == 0 || r.bus_channels == 1 || r.bus_channels == 2));
    SIG_CHECK_ARG(r.bus_channels == 0 ? r.out_ld >= r.voices : (r.out_ld >= r.bus_channels && r.workspace != nullptr));
    SIG_CHECK_ARG(r.bus_gains ? (r.bus_channels > 0 && r.bus_gains_ld >= r.voices) : r.bus_channels <= 1);
    const sig_voice_program_t& P = *r.program;
    SIG_CHECK_ARG(P.n_ins >= 1 && P.n_ins <= SIG_VP_MAX_INS && P.n_oscs >= 0 && P.n_oscs <= SIG_VP_MAX_OSCS);
    SIG_CHECK_ARG(P.n_params >= 0 && P.n_params <= SIG_VP_MAX_PARAMS && P.n_filters >= 0 && P.n_filters <= SIG_VP_MAX_FILTERS);
    SIG_CHECK_ARG(P.n_temps >= 0 && P.n_temps <= SIG_VP_MAX_TEMPS && P.depth >= 0 && P.depth <= P.n_filters);
    SIG_CHECK_ARG(r.hist_blocks >= 0 && r.hist_blocks <= SIG_VP_MAX_HIST && (r.hist_blocks == 0 || r.hist_positions) && r.blocks_before >= 0);
    const bool small = P.depth > 0 && r.block_frames < r.context;
    SIG_CHECK_ARG(!small || (P.depth <= 2 && r.block_frames >= 16));          // (deeper cascades, or blocks so short that the reference's 16-entry block cache evicts what they read: the eager path)
    SIG_CHECK_ARG(small || r.position == 0 || r.hist_blocks >= (P.depth > 1 ? 1 : 0));
    SIG_CHECK_ARG(r.control_rows == (small ? 2 * r.nblocks : r.hist_blocks + 1 + r.nblocks));
    c.empty = r.block_frames == 0 || r.nblocks == 0 || r.voices == 0;
    if (c.empty) return 0;
    VpArgs& a = c.a;
    a = VpArgs{};
    a.rate = (double)r.rate; a.position = r.position; a.N = r.block_frames; a.K = r.nblocks; a.ctx = r.context; a.voices = r.voices;
    auto rows_ok = [&](const sig_vp_rows& rows, bool optional) {
        if (!rows.ptr) return optional;
        return (rows.col_stride | 1) == 1 && (rows.rows == 1 || rows.rows == r.control_rows);
    };
    // the tables: together inside the cap (one workgroup's LDS holds them all); a power of two where an OscTable word reads one (below)
    const int n_tables = tables ? tables->n_tables : 0;
    SIG_CHECK_ARG(n_tables >= 0 && n_tables <= SIG_VP_MAX_TABLES);
    c.table_lds = 0;
    for (int k = 0, points = 0; k < n_tables; ++k) {
        const auto& t = tables->table[k];
        SIG_CHECK_ARG(t.ptr != nullptr && t.points >= 2 && t.waves >= 1 &&
                      (int64_t)t.points * t.waves <= SIG_TABLE_MAX_POINTS - points);
        points += t.points * t.waves;
        c.table_lds += (size_t)(t.points + 1) * t.waves * sizeof(float);
    }
    a.n_ins = P.n_ins;
    for (int k = 0; k < P.n_ins; ++k) {
        const sig_vp_ins& x = P.ins[k];
        SIG_CHECK_ARG(vp_word_ok(x));
        switch (x.op) {
            case SIG_VP_OSCTABLE:
                SIG_CHECK_ARG(x.a < P.n_oscs && x.b < n_tables && x.c < P.n_params);
                SIG_CHECK_ARG((tables->table[x.b].points & (tables->table[x.b].points - 1)) == 0);     // the oscillator wraps with a mask
                break;
            case SIG_VP_SHAPE: SIG_CHECK_ARG(x.b < n_tables && x.c < P.n_params); break;
            case SIG_VP_OSC: SIG_CHECK_ARG(x.a < P.n_oscs && x.kind <= SIG_OSC_TRIANGLE); break;
            case SIG_VP_OSCPM: SIG_CHECK_ARG(x.a < P.n_oscs && x.b < P.n_params && x.kind <= SIG_OSC_TRIANGLE); break;
            case SIG_VP_FILTER: SIG_CHECK_ARG(x.a < P.n_filters); break;
            case SIG_VP_FILTERQ: SIG_CHECK_ARG(x.a < P.n_filters && x.c < P.n_params); break;
            case SIG_VP_FILTEREQ: SIG_CHECK_ARG(x.a < P.n_filters && x.b < P.n_params && x.c < P.n_params); break;
            case SIG_VP_OSCUNI:
                SIG_CHECK_ARG(unison != nullptr && x.a < P.n_oscs && x.b < SIG_VP_MAX_UNISON && x.c < P.n_params && x.kind <= SIG_OSC_TRIANGLE);
                break;
            case SIG_VP_OSCBLEP:                                               // OscUni's operands; no Sine
                SIG_CHECK_ARG(unison != nullptr && x.a < P.n_oscs && x.b < SIG_VP_MAX_UNISON && x.c < P.n_params &&
                              x.kind >= SIG_OSC_SQUARE && x.kind <= SIG_OSC_TRIANGLE);
                break;
            case SIG_VP_OSCSYNC:                                               // OscBlep's operands, b: the ratio's parameter slot | -1; Sawtooth and Square
                SIG_CHECK_ARG(unison != nullptr && x.a < P.n_oscs && x.b < P.n_params && x.c < P.n_params &&
                              (x.kind == SIG_OSC_SAWTOOTH || x.kind == SIG_OSC_SQUARE));
                break;
            case SIG_VP_BAND: SIG_CHECK_ARG(x.a + 1 < P.n_filters); break;
            case SIG_VP_GAIN: case SIG_VP_CONST: case SIG_VP_AMP: SIG_CHECK_ARG(x.a < P.n_params); break;
            case SIG_VP_MUL: case SIG_VP_SAVE: case SIG_VP_LOAD: SIG_CHECK_ARG(x.a < P.n_temps); break;
            case SIG_VP_MIX: SIG_CHECK_ARG(x.a < P.n_temps && x.b < P.n_params); break;
            case SIG_VP_NOISE: SIG_CHECK_ARG(x.a < 2); break;
            default: break;
        }
    }
    const VpNeeds need = c.need = vp_needs(P);
    SIG_CHECK_ARG(!(need.sync && need.eq));                                    // (no kernel set has both handlers: the engine keeps such a graph per node)
    if (!r.allow_mixed) {
        const bool band = need.has(SIG_VP_FAMILY_BAND), pm = need.has(SIG_VP_FAMILY_PM), res = need.has(SIG_VP_FAMILY_RESONANT);
        SIG_CHECK_ARG(!(need.uni() && (band || pm || need.table() || res)));
        SIG_CHECK_ARG(!(res && (band || pm || need.table())));
        SIG_CHECK_ARG(!(band && pm) && !(need.table() && (band || pm)));      // (no single-family variant with two of them; the engine keeps such a graph per node unless asked for mixed programs)
    }
    VpTables& tb = std::get<VpTables>(c.extra);
    tb = VpTables{};
    for (int k = 0; k < n_tables; ++k) { tb.ptr[k] = tables->table[k].ptr; tb.T[k] = tables->table[k].points; tb.W[k] = tables->table[k].waves; }
    if (!need.table()) c.table_lds = 0;
    VpUnison& un = std::get<VpUnison>(c.extra);
    un = VpUnison{};
    if (need.uni()) {
        un.copies = unison->copies;
        for (int u = 0; u < un.copies; ++u) { un.detune[u] = unison->detune[u]; un.offset[u] = unison->offset[u]; }
    }
    VpMixed& mx = std::get<VpMixed>(c.extra);
    mx = VpMixed{};
    if (need.families() >= 2) {
        for (int k = 0; k < SIG_VP_MAX_TABLES; ++k) { mx.ptr[k] = need.table() ? tb.ptr[k] : nullptr; mx.T[k] = tb.T[k]; mx.W[k] = tb.W[k]; }     // (no table word: nothing is staged)
        mx.copies = un.copies;
        for (int u = 0; u < un.copies; ++u) { mx.detune[u] = un.detune[u]; mx.offset[u] = un.offset[u]; }
    }
    SIG_CHECK_ARG(vp_encode(P, a.code));
    a.n_oscs = P.n_oscs; a.n_params = P.n_params; a.n_filters = P.n_filters;
    for (int k = 0; k < P.n_oscs; ++k) {
        SIG_CHECK_ARG(rows_ok(P.hertz[k], false) && rows_ok(P.phase[k], true));
        a.hertz[k] = Rows{P.hertz[k].ptr, P.hertz[k].col_stride, P.hertz[k].rows};
        a.phase[k] = Rows{P.phase[k].ptr, P.phase[k].col_stride, P.phase[k].ptr ? P.phase[k].rows : 1};
    }
    for (int k = 0; k < P.n_params; ++k) {
        SIG_CHECK_ARG(rows_ok(P.params[k], false));
        a.params[k] = Rows{P.params[k].ptr, P.params[k].col_stride, P.params[k].rows};
    }
    // filter slots: a Filter instruction runs a LowPass / HighPass slot; a Band instruction at slot f runs the pair f, f + 1 (its
    // low and high rows), of one band type and one level, which the kernel finds by pairing every run of band slots from its start
    int role[SIG_VP_MAX_FILTERS] = {0};                                        // 1: single, 2: first of a band, 3: second, 4: resonant (one FilterQ word), 5: equaliser (one FilterEq word)
    for (int k = 0; k < P.n_ins; ++k) {
        const sig_vp_ins& x = P.ins[k];
        if (x.op == SIG_VP_FILTER) {
            SIG_CHECK_ARG(role[x.a] == 0 || role[x.a] == 1);
            role[x.a] = 1;
        } else if (x.op == SIG_VP_FILTERQ) {
            SIG_CHECK_ARG(role[x.a] == 0);
            role[x.a] = 4;
        } else if (x.op == SIG_VP_FILTEREQ) {
            SIG_CHECK_ARG(role[x.a] == 0);
            role[x.a] = 5;
        } else if (x.op == SIG_VP_BAND) {
            SIG_CHECK_ARG((role[x.a] == 0 || role[x.a] == 2) && (role[x.a + 1] == 0 || role[x.a + 1] == 3));
            role[x.a] = 2; role[x.a + 1] = 3;
        }
    }
    for (int k = 0, run = 0; k < P.n_filters; ++k) {
        const bool band = P.filter_type[k] == SIG_FILT_BANDPASS || P.filter_type[k] == SIG_FILT_BANDSTOP;
        run = band ? run + 1 : 0;
        if (role[k] == 1) SIG_CHECK_ARG(P.filter_type[k] == SIG_FILT_LOWPASS || P.filter_type[k] == SIG_FILT_HIGHPASS);
        else if (role[k] == 2) SIG_CHECK_ARG(band && run % 2 == 1 && P.filter_type[k + 1] == P.filter_type[k] &&
                                             P.filter_level[k + 1] == P.filter_level[k]);
        else if (role[k] == 3) SIG_CHECK_ARG(band && run % 2 == 0);
        const bool resonant = P.filter_type[k] == SIG_FILT_RES_LOWPASS || P.filter_type[k] == SIG_FILT_RES_HIGHPASS;
        SIG_CHECK_ARG(resonant == (role[k] == 4));                             // a resonant slot and its FilterQ word go together
        const bool eq = P.filter_type[k] >= SIG_FILT_EQ_BANDPASS && P.filter_type[k] <= SIG_FILT_EQ_HIGHSHELF;
        SIG_CHECK_ARG(eq == (role[k] == 5));                                   // ... an equaliser slot and its FilterEq word
    }
    for (int k = 0; k < P.n_filters; ++k) {
        SIG_CHECK_ARG(rows_ok(P.cutoff[k], false) && P.filter_type[k] >= SIG_FILT_LOWPASS && P.filter_type[k] <= SIG_FILT_EQ_HIGHSHELF);
        a.cutoff[k] = Rows{P.cutoff[k].ptr, P.cutoff[k].col_stride, P.cutoff[k].rows};
        a.ftype[k] = P.filter_type[k];
        SIG_CHECK_ARG(P.filter_level[k] >= 1 && P.filter_level[k] <= P.depth);
        a.flevel[k] = P.filter_level[k];
    }
    if (need.adsr) {
        SIG_CHECK_ARG(sig_env::load_rows(P.adsr, P.adsr_stride, a.adsr));
        a.has_adsr = 1;
    }
    a.seeds[0] = P.noise_seed[0]; a.seeds[1] = P.noise_seed[1];
    a.depth = P.depth; a.small = small ? 1 : 0; a.blocks_before = r.blocks_before;
    a.hist = small ? 0 : r.hist_blocks;
    for (int k = 0; k < a.hist; ++k) {
        SIG_CHECK_ARG(r.hist_positions[k] >= 0 && r.hist_positions[k] < (k + 1 < a.hist ? r.hist_positions[k + 1] : r.position));
        a.hist_pos[k] = r.hist_positions[k];
    }
    a.status = r.status;
    if (r.bus_channels > 0) {
        a.pan = r.bus_gains; a.pan_ld = r.bus_gains_ld; a.partials = r.workspace; a.rows = (int64_t)r.block_frames * r.nblocks;
    } else {
        a.out = r.out; a.out_ld = r.out_ld;
    }
    return 0;
}

// Picks the geometry of a checked call and launches it: the image attached for this very program, or the interpreter variant
// vp_variant names.
int vp_launch_call(const VpRequest& r, VpCall& c)
{
    VpArgs& a = c.a;
    const sig_voice_program_t& P = *r.program;
    const int C = r.bus_channels;
    const int64_t rows = (int64_t)r.block_frames * r.nblocks;
    const int aligned = (r.voices % 4 == 0 && r.out_ld % 4 == 0 && reinterpret_cast<uintptr_t>(r.out) % 16 == 0) ? 4
                      : (r.voices % 2 == 0 && r.out_ld % 2 == 0 && reinterpret_cast<uintptr_t>(r.out) % 8 == 0) ? 2 : 1;
    int vpt = 1;
    vp_geometry(a, aligned, vp_find_special(a, P, 4, C) != nullptr, vpt, a.span);
    a.voice_tiles = sig_voice_tiles(r.voices, vpt);
    unsigned nwg;
    if (!sig_workgroups(sig_span_waves(a.voice_tiles, a.K, a.span), nwg)) return (int)hipErrorInvalidValue;
    if (C > 0 && sig_bus::tiles_sum_in_workgroup(a.voice_tiles)) { a.bus_out = r.out; a.bus_out_ld = r.out_ld; }
    hipStream_t s = static_cast<hipStream_t>(r.stream);
    int err;
    if (hipFunction_t fn = vp_find_special(a, P, vpt, C)) {                    // this very program, built as straight-line code
        void* second = c.need.families() >= 2 ? (void*)&std::get<VpMixed>(c.extra)
                     : c.need.uni() ? (void*)&std::get<VpUnison>(c.extra) : (void*)&std::get<VpTables>(c.extra);
        void* params[] = {&a, second};                                         // (an image built for a mixed, a table or a unison program takes both, any other the first)
        err = (int)hipModuleLaunchKernel(fn, nwg, 1, 1, 256, 1, 1, (unsigned)c.table_lds, s, params, nullptr);
    } else if (vpt == 4) {
        return (int)hipErrorInvalidValue;                                      // (forced by the tuning hook after the image was switched off)
    } else if (c.need.eq) {
        // a FilterEq word: the second set of the resonant or the mixed variant (vp_variant answers one of the two: the word is of the
        // resonant family), chosen here and only here, so that every program without the word gets the kernels it always got
        err = vp_variant(c.need) == SIG_VP_FAMILY_MIXED
            ? VpLaunch<vp_family::mixed_eq>::run(a, std::get<VpMixed>(c.extra), vpt, fits_small(c.need), C, nwg, c.table_lds, s)
            : VpLaunch<vp_family::resonant_eq>::run(a, std::get<VpNoTables>(c.extra), vpt, fits_small(c.need), C, nwg, c.table_lds, s);
    } else if (c.need.sync) {
        // an OscSync word: the second set of the band-limited or the mixed variant, chosen here and only here likewise
        err = vp_variant(c.need) == SIG_VP_FAMILY_MIXED
            ? VpLaunch<vp_family::mixed_sync>::run(a, std::get<VpMixed>(c.extra), vpt, fits_small(c.need), C, nwg, c.table_lds, s)
            : VpLaunch<vp_family::sync>::run(a, std::get<VpUnison>(c.extra), vpt, fits_small(c.need), C, nwg, c.table_lds, s);
    } else {
        err = vp_with_family(vp_variant(c.need), [&](auto family) {
            using F = decltype(family);
            return VpLaunch<F>::run(a, std::get<typename F::Extra>(c.extra), vpt, fits_small(c.need), C, nwg, c.table_lds, s);
        });
    }
    if (err || C == 0 || a.bus_out) return err;
    switch (C) {
        case 1: return sig_bus::launch_partials<1>(a.partials, a.voice_tiles, rows, r.out, r.out_ld, s);
        default: return sig_bus::launch_partials<2>(a.partials, a.voice_tiles, rows, r.out, r.out_ld, s);
    }
}

// The one body of sig_voice_program, _ex, _unison (allow_mixed false) and _mixed (true): everything but the three exclusivity
// checks is the same for a program that combines the extension words.
int vp_run(const VpRequest& r)
{
    VpCall c;
    if (const int err = vp_check(r, c)) return err;
    return c.empty ? 0 : vp_launch_call(r, c);
}

}  // namespace

extern "C" int sig_voice_program_set_tuning(int32_t voices_per_lane, int32_t blocks_per_lane)
{
    SIG_CHECK_ARG(voices_per_lane >= 0 && blocks_per_lane >= 0);
    vp_tuning().vpt = voices_per_lane;
    vp_tuning().span = blocks_per_lane;
    return 0;
}

extern "C" int sig_voice_program_geometry(int32_t voices, int32_t block_frames, int32_t nblocks, int32_t context, int32_t depth,
                                          int32_t bus_channels, int32_t store_aligned, int32_t specialised,
                                          int32_t* voices_per_lane, int32_t* blocks_per_lane)
{
    SIG_CHECK_ARG(voices >= 0 && block_frames >= 0 && nblocks >= 0 && context >= 0 && depth >= 0 && voices_per_lane && blocks_per_lane);
    VpArgs a{};
    a.voices = voices; a.N = block_frames; a.K = nblocks; a.ctx = context;
    a.small = (depth > 0 && block_frames < context) ? 1 : 0;
    double dummy = 0.0;
    a.partials = bus_channels > 0 ? &dummy : nullptr;                          // (only asked whether there is a bus)
    int vpt = 1, span = 1;
    vp_geometry(a, store_aligned, specialised != 0, vpt, span);
    *voices_per_lane = vpt; *blocks_per_lane = span;
    return 0;
}

extern "C" int sig_voice_program_variant(const sig_voice_program_t* program, int32_t* family, int32_t* small_file)
{
    SIG_CHECK_ARG(program && family && small_file && program->n_ins >= 1 && program->n_ins <= SIG_VP_MAX_INS);
    const VpNeeds need = vp_needs(*program);
    *family = vp_variant(need);                                                // (what vp_launch_call asks)
    *small_file = fits_small(need) ? 1 : 0;
    return 0;
}

extern "C" int64_t sig_voice_program_args_size(void) { return (int64_t)sizeof(VpArgs); }

extern "C" int sig_voice_program_use_attached(int32_t on) { vp_tuning().attached = on ? 1 : 0; return 0; }

extern "C" int sig_voice_program_attach(const sig_voice_program_t* program, int32_t voices_per_lane, int32_t bus_channels,
                                        const void* image)
{
    SIG_CHECK_ARG(program && image && (voices_per_lane == 1 || voices_per_lane == 2 || voices_per_lane == 4) && bus_channels >= 0 && bus_channels <= 2);
    const sig_voice_program_t& P = *program;
    SIG_CHECK_ARG(P.n_ins >= 1 && P.n_ins <= SIG_VP_MAX_INS);
    VpSpecial e{};
    SIG_CHECK_ARG(vp_encode(P, e.code));
    e.n_ins = P.n_ins; e.n_oscs = P.n_oscs; e.n_params = P.n_params; e.n_filters = P.n_filters; e.n_temps = P.n_temps;
    e.vpt = voices_per_lane; e.C = bus_channels;
    hipError_t err = hipModuleLoadData(&e.mod, image);
    if (err != hipSuccess) { (void)hipGetLastError(); return (int)err; }       // (not sticky: the caller's next HIP call must not inherit it)
    hipFunction_t info = nullptr;
    err = hipModuleGetFunction(&e.fn, e.mod, "sig_vp_specialised");
    if (err == hipSuccess) err = hipModuleGetFunction(&info, e.mod, "sig_vp_specialised_info");
    // the image says what it was built for: the argument block's size, voices per lane, sink and program must be THIS library's
    uint32_t* dev = nullptr;
    uint32_t got[4 + kMaxIns] = {0};
    if (err == hipSuccess) err = hipMalloc(&dev, sizeof(got));
    if (err == hipSuccess) {
        void* params[] = {&dev};
        err = hipModuleLaunchKernel(info, 1, 1, 1, 1, 1, 1, 0, nullptr, params, nullptr);
        if (err == hipSuccess) err = hipMemcpy(got, dev, sizeof(got), hipMemcpyDeviceToHost);
        (void)hipFree(dev);
    }
    if (err == hipSuccess &&
        (got[0] != (uint32_t)sizeof(VpArgs) || got[1] != (uint32_t)e.vpt || got[2] != (uint32_t)e.C || got[3] != (uint32_t)e.n_ins ||
         memcmp(got + 4, e.code, sizeof(uint32_t) * e.n_ins) != 0))
        err = hipErrorInvalidImage;
    if (err != hipSuccess) { (void)hipModuleUnload(e.mod); (void)hipGetLastError(); return (int)err; }
    std::lock_guard<std::mutex> g(vp_specials_lock());
    vp_specials().push_back(e);
    return 0;
}

extern "C" int sig_voice_program_detach_all(void)
{
    std::lock_guard<std::mutex> g(vp_specials_lock());
    for (VpSpecial& e : vp_specials()) (void)hipModuleUnload(e.mod);
    vp_specials().clear();
    return 0;
}

extern "C" int sig_voice_program(const sig_voice_program_t* program, int32_t rate, int64_t position, int32_t block_frames,
                                 int32_t nblocks, int32_t context, int32_t voices, int32_t control_rows,
                                 int32_t hist_blocks, const int64_t* hist_positions, int32_t blocks_before,
                                 const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                                 double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream)
{
    return vp_run({program, rate, position, block_frames, nblocks, context, voices, control_rows, hist_blocks, hist_positions,
                   blocks_before, bus_gains, bus_gains_ld, bus_channels, workspace, out, out_ld, status, stream, nullptr, nullptr, false});
}

extern "C" int sig_voice_program_ex(const sig_voice_program_t* program, int32_t rate, int64_t position, int32_t block_frames,
                                    int32_t nblocks, int32_t context, int32_t voices, int32_t control_rows,
                                    int32_t hist_blocks, const int64_t* hist_positions, int32_t blocks_before,
                                    const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                                    double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream,
                                    const sig_vp_tables_t* tables)
{
    return vp_run({program, rate, position, block_frames, nblocks, context, voices, control_rows, hist_blocks, hist_positions,
                   blocks_before, bus_gains, bus_gains_ld, bus_channels, workspace, out, out_ld, status, stream, tables, nullptr, false});
}

extern "C" int sig_voice_program_unison(const sig_voice_program_t* program, int32_t rate, int64_t position, int32_t block_frames,
                                        int32_t nblocks, int32_t context, int32_t voices, int32_t control_rows,
                                        int32_t hist_blocks, const int64_t* hist_positions, int32_t blocks_before,
                                        const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                                        double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream,
                                        const sig_vp_tables_t* tables, const sig_vp_unison_t* unison)
{
    return vp_run({program, rate, position, block_frames, nblocks, context, voices, control_rows, hist_blocks, hist_positions,
                   blocks_before, bus_gains, bus_gains_ld, bus_channels, workspace, out, out_ld, status, stream, tables, unison, false});
}

// sig_voice_program_unison for programs that combine two or more of Band, OscPM, OscTable / Shape, FilterQ and OscUni: the MIXED
// variant of the interpreter (or the image attached for the program).  Every other check of the body holds
extern "C" int sig_voice_program_mixed(const sig_voice_program_t* program, int32_t rate, int64_t position, int32_t block_frames,
                                        int32_t nblocks, int32_t context, int32_t voices, int32_t control_rows,
                                        int32_t hist_blocks, const int64_t* hist_positions, int32_t blocks_before,
                                        const double* bus_gains, int64_t bus_gains_ld, int32_t bus_channels,
                                        double* workspace, float* out, int64_t out_ld, int32_t* status, void* stream,
                                        const sig_vp_tables_t* tables, const sig_vp_unison_t* unison)
{
    return vp_run({program, rate, position, block_frames, nblocks, context, voices, control_rows, hist_blocks, hist_positions,
                   blocks_before, bus_gains, bus_gains_ld, bus_channels, workspace, out, out_ld, status, stream, tables, unison, true});
}
#endif  // SIG_VP_STATIC_CODE
