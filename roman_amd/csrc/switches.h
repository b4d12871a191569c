// switches.h — every ROMAN_* environment switch of libroman_hip.so: its field, its values, when it is read and who uses it.
// Plain C++17, no HIP: tests/switches_main.cpp builds it with the host compiler alone (tests/test_switches_cpu.py holds the
// expected value of every field for every kind of string).  The switches select kernels, force A/B paths and serve as test hooks;
// the decisions they enter stay where they are taken (roman_hip.hip) — here is only what a string means.
//
// PER CALL: read_switches() reads the variable every time — once per entry into the launch sequence (enqueue_score, enqueue_solve,
// roman_set_matrix_data, roman_debug_cosine) and once per roman_ctx_create; a test may set it with monkeypatch between two calls.
// READ ONCE: switches_once() reads the variable the first time anything asks for a switch and never again in the process; set it
// before the process starts (tools/ scripts, A/B runs) — a test that sets it with monkeypatch tests nothing.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace roman {

// A forced choice: CHOICE_LIB = the library decides by its own rule, 0 = forced off ("never"), 1 = forced on ("always" / wherever the results allow it).
constexpr int CHOICE_LIB = -1;

struct Switches {
    // ---- read once ------------------------------------------------------------------------------------------------------------
    bool debug = false;             // ROMAN_DEBUG: set (any value, "" too) -> synchronise after every launch and name it on stderr, print a batch's totals (tools/gpu_step_debug.py)
    int wide = CHOICE_LIB;          // ROMAN_WIDE: unset -> library; "1…" -> k_solve_wide whenever a fallback problem can exist; anything else -> never ("" too: an accident of the missing empty check) (A/B, profiles/r06/wide)
    bool small_fused = true;        // ROMAN_SMALL_FUSED: "0…" -> never k_small (A/B, tools/gpu_demo_scale.py)
    bool small_only = true;         // ROMAN_SMALL_ONLY: "0…" -> never leave the general kernels out beside k_small (A/B, tools/gpu_demo_scale.py)
    bool small = true;              // ROMAN_SMALL: "0…" -> never the one-wave-per-problem k_solve_up (A/B)

    // ---- per call: unset or "" -> library, "1…" -> on, anything else -> off -------------------------------------------------------
    int cos_sel = CHOICE_LIB;       // ROMAN_COS_SEL: the cosine screen k_cos_sel / k_cos_live ("approx" and "gated" are therefore "off" here) (test_gpu_cos_sel, test_gpu_cos_live, test_gpu_cos_screen_adversarial)
    int cos_sel_matrix = 0;         // ROMAN_COS_SEL once more, for roman_debug_cosine alone: COS_SEL_GATED at "gated", COS_SEL_APPROX at "approx" (whole string), else 0 (same tests)
    int cos_deal = CHOICE_LIB;      // ROMAN_COS_DEAL: the dealt-block cosine kernel k_cos_deal (A/B, test_gpu_parity)
    int cos_block = CHOICE_LIB;     // ROMAN_COS_BLOCK, maps of at most 48 objects: k_cos_block instead of k_cos_wave (A/B, test_gpu_parity)
    bool cos_block_large = true;    // ROMAN_COS_BLOCK once more, larger maps, by ANOTHER rule: only "0…" keeps k_cos_block away ("2" is off above and on here) (test_gpu_parity)

    // ---- per call: unset -> library, "0…" -> off, anything else -> on ("" too: forced ON, an accident of the missing empty check) ------
    int count_pre = CHOICE_LIB;     // ROMAN_COUNT_PRE: k_count's prefiltered sweep; merely SET (whatever the value) it also lifts the live-set limit 4096 -> 16000 (A/B, test_gpu_parity, test_gpu_count_heights)
    int count_whole = CHOICE_LIB;   // ROMAN_COUNT_WHOLE: whole problems / blocks of rows as the prefiltered sweep's work items (A/B, test_gpu_parity, test_gpu_lists_queue, test_gpu_count_heights)
    int lists = CHOICE_LIB;         // ROMAN_LISTS: k_lists / the four kernels of the symmetric matrix (A/B, test_gpu_parity, test_gpu_lists_queue, test_gpu_count_heights)
    int wide_upper = CHOICE_LIB;    // ROMAN_WIDE_UPPER: k_solve_wide's half-copy instantiation — but "" -> library here (test_gpu_full_configs, test_gpu_wide_sums)

    // ---- per call: off only at "0…" ---------------------------------------------------------------------------------------------------
    bool wide_idx16 = true;         // ROMAN_WIDE_IDX16: "0…" -> 32-bit column labels for k_solve_wide always (test_gpu_full_configs)
    bool count_zlds = true;         // ROMAN_COUNT_ZLDS: "0…" -> the prefiltered sweep's exact gate reads the heights from memory (test_gpu_count_heights)

    // ---- per call: numbers ------------------------------------------------------------------------------------------------------------
    int sort_eq_max = 512;          // ROMAN_SORT_EQMAX (atoi, at least 0; unset or "" -> 512): rows of one degree at most for the sort-free placement of the stream layout's
                                    // positions (place_keys(), kernels.hip.h); beyond, the bitonic sort.  0: always the sort (A/B, test_gpu_parity)
    int lists_lds = -1;             // ROMAN_LISTS_LDS (atoi, at least 0; "" -> 0; unset -> -1 = all the LDS k_lists leaves): bytes of k_lists' window, 0: none (A/B, test_gpu_lists_queue)
    bool wide_teams_set = false;    // ROMAN_WIDE_TEAMS (atoi; "" -> 0): set -> wide_teams replaces the library's count AND roman_ctx_set_wide_teams: 0 never, 1..4 teams per XCD
    int wide_teams = 0;             //   whenever the live sets fit, anything else like 0 (tools/gpu_mid_live.py, test_gpu_full_configs, test_gpu_wide_sums)
    bool wide_compact_set = false;  // ROMAN_WIDE_COMPACT (strtol base 0; unset or "" -> not set = the library's 0x048006): 0 no column compaction, 0xWWTTCC passes per window /
    int wide_compact = 0;           //   threshold x 256 / compactions allowed per problem (test_gpu_batch, test_gpu_full_configs, test_gpu_wide_sums)
    bool test_capnnz_set = false;   // ROMAN_TEST_CAPNNZ (atoll; "" -> 0): the matrix pool's capacity for a batch WITHOUT history: its first attempt overflows, which exercises
    long long test_capnnz = 0;      //   the skip / retry path (test_gpu_batch, test_gpu_submap_align_grid)
    bool test_caplist_set = false;  // ROMAN_TEST_CAPLIST (atoll; "" -> 0): likewise the list pool's (k_lists' overflow: kind 2) (test_gpu_lists_queue)
    long long test_caplist = 0;

    // ---- per call, used by roman_ctx_create -------------------------------------------------------------------------------------------
    int num_xcc = 0;                // ROMAN_NUM_XCC (atoi, 1..64; else 0 = the device's own count): the XCD count the HOST sizes k_solve_wide's teams from (test_gpu_batch)
    double wide_spin_ms = -1.0;     // ROMAN_WIDE_SPIN_MS (atof, >= 0 — "" and "x" are 0 —; else -1 = the library's 4000): budget of a barrier wait of k_solve_wide; 0: the first
                                    // unsuccessful poll of a wait is a timeout (test_gpu_batch)
};
constexpr int COS_SEL_GATED = 1, COS_SEL_APPROX = 2;

// ---- the rules for the strings --------------------------------------------------------------------------------------------------------
inline const char* nonempty(const char* e) { return (e && e[0]) ? e : nullptr; }                  // "" counts as unset
inline int on_at_1(const char* e) { return e ? (e[0] == '1' ? 1 : 0) : CHOICE_LIB; }              // unset -> library, "1…" -> on, else off
inline int off_at_0(const char* e) { return e ? (e[0] != '0' ? 1 : 0) : CHOICE_LIB; }             // unset -> library, "0…" -> off, else on
inline bool not_0(const char* e) { return !(e && e[0] == '0'); }                                   // off only at "0…"

// the read-once fields (the others at their defaults): filled the first time it is called
inline const Switches& switches_once()
{
    static const Switches once = [] {
        Switches s;
        s.debug = getenv("ROMAN_DEBUG") != nullptr;
        s.wide = on_at_1(getenv("ROMAN_WIDE"));
        s.small_fused = not_0(getenv("ROMAN_SMALL_FUSED"));
        s.small_only = not_0(getenv("ROMAN_SMALL_ONLY"));
        s.small = not_0(getenv("ROMAN_SMALL"));
        return s;
    }();
    return once;
}

// every switch as of now: the read-once fields as first read, the per-call fields from the environment of this moment
inline Switches read_switches()
{
    Switches s = switches_once();
    const char* e = getenv("ROMAN_COS_SEL");
    s.cos_sel = on_at_1(nonempty(e));
    s.cos_sel_matrix = !e ? 0 : !strcmp(e, "gated") ? COS_SEL_GATED : !strcmp(e, "approx") ? COS_SEL_APPROX : 0;
    s.cos_deal = on_at_1(nonempty(getenv("ROMAN_COS_DEAL")));
    e = getenv("ROMAN_COS_BLOCK");
    s.cos_block = on_at_1(nonempty(e));
    s.cos_block_large = not_0(e);
    s.count_pre = off_at_0(getenv("ROMAN_COUNT_PRE"));
    s.count_whole = off_at_0(getenv("ROMAN_COUNT_WHOLE"));
    s.lists = off_at_0(getenv("ROMAN_LISTS"));
    s.wide_upper = off_at_0(nonempty(getenv("ROMAN_WIDE_UPPER")));
    s.wide_idx16 = not_0(getenv("ROMAN_WIDE_IDX16"));
    s.count_zlds = not_0(getenv("ROMAN_COUNT_ZLDS"));
    if ((e = nonempty(getenv("ROMAN_SORT_EQMAX")))) s.sort_eq_max = std::max(0, atoi(e));
    if ((e = getenv("ROMAN_LISTS_LDS"))) s.lists_lds = std::max(0, atoi(e));
    if ((e = getenv("ROMAN_WIDE_TEAMS"))) { s.wide_teams_set = true; s.wide_teams = atoi(e); }
    if ((e = nonempty(getenv("ROMAN_WIDE_COMPACT")))) { s.wide_compact_set = true; s.wide_compact = (int)strtol(e, nullptr, 0); }
    if ((e = getenv("ROMAN_TEST_CAPNNZ"))) { s.test_capnnz_set = true; s.test_capnnz = atoll(e); }
    if ((e = getenv("ROMAN_TEST_CAPLIST"))) { s.test_caplist_set = true; s.test_caplist = atoll(e); }
    if ((e = getenv("ROMAN_NUM_XCC"))) { const int v = atoi(e); if (v >= 1 && v <= 64) s.num_xcc = v; }
    if ((e = getenv("ROMAN_WIDE_SPIN_MS"))) { const double v = atof(e); if (v >= 0.0) s.wide_spin_ms = v; }
    return s;
}

}  // namespace roman
