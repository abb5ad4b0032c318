// Tuning / test knobs: THE list, the FW_KNOBS=1 gate and the typed readers.
//
// Every knob is an environment variable FW_*, read ONLY when FW_KNOBS=1 is set.  The compiled-in defaults are the product; a stray
// FW_* variable in a user's environment must not change what the library does.  tests/conftest.py, bench.py (for its one-chain /
// host-seam passes) and the scripts under profiles/tools set FW_KNOBS=1.  All knobs leave results unchanged unless their line says
// otherwise.  DESIGN.md section 5 carries a copy of this table; tests/test_knobs_cpu.py checks that the two agree on the names, that
// nothing under csrc/ reads the environment besides this file, and that every knob a test or tool sets exists here.
//
// The readers do not cache: a site that must see a knob flipped inside a live process calls them every time, a site that may
// latch the value keeps it in a `static const`.  Clamping and kind-dependent defaults stay where the value is applied, beside
// the measurement notes that chose them.
#pragma once
#include <cstdlib>

// X(environment name, "what it does; default")
#define FW_KNOB_LIST(X)                                                                                                                                                   \
    /* ---- which path runs (tests and bench.py switch these inside a live process: read per call) ---- */                                                                \
    X(FW_HOST_HITON, "1: HITON-PC through the host job pool instead of the device rounds; default 0")                                                                     \
    X(FW_HOST_BH, "1: Benjamini-Hochberg and neighbour lists on the host instead of fw_bh.hip; default 0")                                                                \
    X(FW_DEV_MIN_TARGETS, "fewest targets of a round that take the device path; default 64 (fz, fz_nz) / 256 (discrete)")                                                 \
    X(FW_NZ_DEV, "0: fz_nz rounds through the host pool; default on")                                                                                                     \
    X(FW_MI_SCHED, "0: discrete kinds as one launch per round with the host in between instead of the device schedule; default on")                                       \
    X(FW_FZ_SCHED, "0: fz feed-forward rounds one by one with the host in between instead of the device schedule; default on")                                            \
    X(FW_MI_ROUNDS, "non-zero: discrete kinds as level-synchronous rounds over the segment kernels instead of the persistent kernel; default 0")                          \
    X(FW_DH_CHAINS, "concurrent chains of device rounds (fz), clamped to 1..4; default 2")                                                                                \
    X(FW_DH_CHAINS_DISC, "the same for the discrete kinds under FW_MI_ROUNDS, clamped to 1..4; default 2")                                                                \
    X(FW_DH_CHAIN_MIN, "targets per chain below which a round stays on one chain (positive); default 48")                                                                 \
    X(FW_DH_HEAVY_PCT, "percent of the heaviest targets that get chain 0 to themselves in small rounds; default 0 (off)")                                                 \
    X(FW_DH_HEAVY_BELOW, "... only in rounds of at most this many targets; default 512")                                                                                  \
    X(FW_FZS_GRAM, "0: streamed-column tests without the Gram-matrix kernel; default on")                                                                                 \
    X(FW_NO_HK, "set: generic size-4/5 kernel for every job instead of the level-2 table kernel; default unset")                                                          \
    X(FW_NO_TAB, "set: in-lane caching kernel for every job instead of the table kernel; default unset")                                                                  \
    X(FW_ZC_OUT, "0: segment results staged through device memory instead of written to pinned host memory; default on")                                                  \
    X(FW_L0_MFMA, "discrete level 0 on the matrix cores: 0 never, 2 wherever defined; default 1 (mi_nz from 1 024 variables on)")                                         \
    X(FW_MI_ROWK, "row-count form of the discrete test core, 99: popcount form only; default 2")                                                                          \
    X(FW_MI_ROW4, "0: one subset per wavefront step, 2: four per step up to MI4_N samples; default 1 (four up to 2 048 samples)")                                         \
    /* ---- host job pool (fw_pool.cpp, fw_hiton.cpp) ---- */                                                                                                             \
    X(FW_WINDOW_GROWTH, "2..64: fixed growth factor of a job's evaluation window; default 0 (by launch size, see fw_pool_growth)")                                        \
    X(FW_SMALL_LAUNCH, "ranks below which a launch counts as small and windows grow x256; default 4194304")                                                               \
    X(FW_W0_BIG, "first window of a job with 64 accepted variables or more; default 16384 (device rounds, fz max_k <= 3: 32768, see dh_make_params)")                     \
    X(FW_W0_SMALL, "first window of a smaller job in the device rounds (positive, fz only); default per kind / max_k, see dh_make_params")                                \
    X(FW_SEG_TARGET, "workgroups per launch the segment length aims for (positive); default per kind / max_k, see dh_policy / fw_pool_seglen")                            \
    X(FW_SPEC_DEPTH, "candidates the host pool tests ahead per target; default 8")                                                                                        \
    X(FW_SPEC_TARGETS, "... in rounds of at most this many targets; default 512")                                                                                         \
    /* ---- device rounds: windows and look-ahead (dh_make_params, dh_policy in fw_devhiton.hip) ---- */                                                                  \
    X(FW_ELIM_FULL, "0: elimination jobs start with a first window like interleaving jobs instead of the full enumeration; default 1")                                    \
    X(FW_DH_GROWTH, "window growth factor of a job (positive); default 4")                                                                                                \
    X(FW_DH_GROWTH_SMALL, "... after a launch of fewer than FW_SMALL_LAUNCH ranks (positive); default 256")                                                               \
    X(FW_DH_GROWTH_BUSY, "... with more than FW_DH_BUSY_JOBS live jobs (positive); default 4")                                                                            \
    X(FW_DH_BUSY_JOBS, "live jobs from which a round counts as busy (positive); default 2048")                                                                            \
    X(FW_DH_SPEC, "elimination look-ahead: members tested ahead per target, clamped to 0..DH_MAX_SPEC; default 4 (exact elimination: DH_SPEC_EXACT)")                     \
    X(FW_DH_SPEC_BELOW, "... only after a launch of fewer ranks than this (positive); default 30000000 (max_k <= 3, 256 targets or more) / 12000000")                     \
    X(FW_DH_SPEC0, "interleaving look-ahead: candidates tested ahead per target, clamped to 0..DH_MAX_SPEC; default 2")                                                   \
    X(FW_DH_SPEC0_BELOW, "... only after a launch of fewer ranks than this (positive); default 12000000")                                                                 \
    X(FW_DH_SPEC0_JOBS, "... and of fewer jobs than this (positive); default 4096")                                                                                       \
    X(FW_DH_SPEC0_LIGHT, "deeper interleaving look-ahead after light launches, at least FW_DH_SPEC0; default FW_DH_SPEC0")                                                \
    X(FW_DH_SPEC0_LIGHT_BELOW, "ranks below which a launch counts as light (positive); default 400000")                                                                   \
    X(FW_DH_SPEC1, "look-ahead behind a candidate about to be accepted (fz), clamped to 0..DH_MAX_SPEC; default 2")                                                       \
    X(FW_SEG_A, "launches of fewer ranks than this use a third of FW_SEG_TARGET (fz); default 8000000")                                                                   \
    X(FW_SEG_B, "... fewer than this, two thirds; default 12000000")                                                                                                      \
    X(FW_SEG_GRID, "cap on the striding workgroups of the segment kernel (positive); default 2048 (fz, max_k <= 3) / FW_SEG_TARGET + 512")                                \
    X(FW_DH_LIGHT_DEG, "largest level-0 degree of a target that one workgroup runs from start to end (fz, max_k <= 3), clamped to FW_TAB_A / 2, 0: off; default 32")      \
    X(FW_FZ_TMAT, "smallest degree of a target that gets a local correlation matrix, 0: none; default 16 (max_k > 3: 1)")                                                 \
    X(FW_DH_BATCH, "rounds per batch (positive, at most 16); default 4 up to 1 024 targets, else 16")                                                                     \
    X(FW_DH_TIME_EVERY, "one segment launch in this many is timed with events (positive); default 4")                                                                     \
    X(FW_DH_HP, "1: step / compact / plan / fill kernels on a high-priority stream; default off")                                                                         \
    X(FW_DH_PLAN_SMALL, "0: the 1 024-thread plan kernel instead of the 256-thread one; default 1")                                                                       \
    /* ---- persistent discrete kernel (dh_make_params, dh_mi_launch) ---- */                                                                                             \
    X(FW_MI_SEQ, "tests a job runs before it opens a board (positive); default 48")                                                                                       \
    X(FW_MI_SEQ_HEAVY, "... for a job of a heavy target (FW_MI_HEAVY); default FW_MI_SEQ")                                                                                \
    X(FW_MI_SEQ_TAIL, "... once the target list is exhausted (tail of a launch); default 4")                                                                              \
    X(FW_MI_HEAVY, "candidates from which a target never works on other targets' boards, 0: off; default 48")                                                             \
    X(FW_MI_WIN0, "first window of a board (positive); default 128")                                                                                                      \
    X(FW_MI_WIN0_TAIL, "... in the tail of a launch (at least 1); default 1024")                                                                                          \
    X(FW_MI_CHUNK_DIV, "ranks per record of a board: its window over this (positive); default 256")                                                                       \
    X(FW_MI_CHUNK_MIN, "... at least this (positive); default 8")                                                                                                         \
    X(FW_MI_CHUNK_MAX, "... at most this (positive); default 64")                                                                                                         \
    X(FW_MI_CHUNK_TAIL, "... at least this in the tail of a launch (at least 1); default FW_MI_CHUNK_MIN")                                                                \
    X(FW_MI_HELP_JOBS, "0: idle wavefronts do not help on other targets' boards; default 1")                                                                              \
    X(FW_MI_ELIM_MIN, "elimination jobs of more ranks than this open a board for the whole enumeration at once, 0: off; default 64")                                      \
    X(FW_MI_AHEAD, "0: no first tests of up to four interleaving candidates in one step (mi_first4); default 1")                                                          \
    X(FW_MI_TEAM_MIN, "candidates from which a target is run by a whole workgroup, 0: none; default 96")                                                                  \
    X(FW_MI_TEAM_MAX, "most such targets per launch; default 192")                                                                                                        \
    X(FW_MI_TEAM_STEPS, "lock-step rounds of a team job before its enumeration goes to a board; default 2")                                                               \
    X(FW_MI_TEAM_TAIL, "non-zero: team targets publish tail-mode boards from the start; default 0")                                                                       \
    X(FW_MI_WG_PER_CU, "workgroups of the persistent kernel per compute unit (positive); default 1")                                                                      \
    /* ---- tracing and profiling (FW_*_DBG: ablations, INVALID results) ---- */                                                                                          \
    X(FW_TRACE_HOST, "set: host-side phase times, per-chain test counts and list lengths on stderr; default unset")                                                       \
    X(FW_TRACE_ROUNDS, "file: one line per round of the host pool; default unset")                                                                                        \
    X(FW_TRACE_JOBS, "file: one line per finished job of the host pool; default unset")                                                                                   \
    X(FW_DH_LOG, "file: one line per planned launch of the device rounds (profiles/README.md); default unset")                                                            \
    X(FW_NZ_TRACE, "set: shape of every fz_nz sub-matrix launch on stderr; default unset")                                                                                \
    X(FW_L0_VERBOSE, "set: pair / candidate counts and phase cycles of the discrete level 0 on stderr; default unset")                                                    \
    X(FW_MI_PROF, "set: shader cycles per phase of the discrete batch tests; default unset")                                                                              \
    X(FW_L0_DBG, "discrete level-0 ablations, bits 1 no epilogue, 2 no loads, 4 no popcounts, 8 no exact pass; default 0")                                                \
    X(FW_FZ_DBG, "Fisher-z kernel ablation flags (fz_dbg_flags); default 0")

namespace knob {
enum Id {
#define X(name, doc) name,
    FW_KNOB_LIST(X)
#undef X
        COUNT
};
}  // namespace knob

// raw value; nullptr when the knob is unset or FW_KNOBS=1 is not given
inline const char *fw_knob_str(knob::Id k)
{
    static const char *const names[knob::COUNT] = {
#define X(name, doc) #name,
        FW_KNOB_LIST(X)
#undef X
    };
    const char *on = getenv("FW_KNOBS");
    return (on && on[0] == '1') ? getenv(names[k]) : nullptr;
}
// "set at all"
inline bool fw_knob_set(knob::Id k) { return fw_knob_str(k) != nullptr; }
// integer with default
inline int fw_knob_int(knob::Id k, int dflt)
{
    const char *e = fw_knob_str(k);
    return e ? atoi(e) : dflt;
}
// "on unless set to 0"
inline bool fw_knob_on(knob::Id k) { return fw_knob_int(k, 1) != 0; }
// 64-bit with default (negative input wraps, as a cast of atoll always did)
inline unsigned long long fw_knob_u64(knob::Id k, unsigned long long dflt)
{
    const char *e = fw_knob_str(k);
    return e ? (unsigned long long)atoll(e) : dflt;
}
// "positive value or default"
inline unsigned long long fw_knob_pos(knob::Id k, unsigned long long dflt)
{
    const char *e = fw_knob_str(k);
    return e && atoll(e) > 0 ? (unsigned long long)atoll(e) : dflt;
}

// knobs that several sites read by the same rule
inline bool fw_trace_host() { return fw_knob_set(knob::FW_TRACE_HOST); }
inline bool fw_host_hiton() { return fw_knob_int(knob::FW_HOST_HITON, 0) == 1; }
inline bool fw_mi_rounds() { return fw_knob_int(knob::FW_MI_ROUNDS, 0) != 0; }
inline bool fw_no_hk() { return fw_knob_set(knob::FW_NO_HK); }
inline bool fw_l0_verbose() { return fw_knob_set(knob::FW_L0_VERBOSE); }
inline unsigned long long fw_small_launch() { return fw_knob_u64(knob::FW_SMALL_LAUNCH, 1ull << 22); }
inline unsigned long long fw_seg_target() { return fw_knob_pos(knob::FW_SEG_TARGET, 0ull); }  // 0: the site's default
