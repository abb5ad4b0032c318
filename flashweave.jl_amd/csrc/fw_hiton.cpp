// Host driver: the caller side of the hot path, restated for hosts without Julia.
//   LGL                      learning.jl:203-279 (target order :97-98)
//   si_HITON_PC              hiton.jl:283-400 (interleaving/elimination via hiton_backend :109-149,
//                            check_candidate! :80-107, update_sig_result! :53-78, update_PC_dict! :249-256)
//   feed-forward whitelist   interleaved.jl:112-183 (as level-synchronous rounds)
//   make_weights / make_symmetric_graph   misc.jl:137-159, 201-272
// Every target is a small state machine; one step of the loop collects the pending (T, candidate, accepted)
// job of every active target and runs them as ONE fw_test_subsets batch on the device.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <thread>

#include "fw_internal.h"
#include "fw_unrank.h"

namespace {

struct ODict {  // OrderedDict{Int,Tuple{Float64,Float64}}: insertion order, re-assignment keeps the slot
    std::vector<int32_t> key;
    std::vector<double> stat, pval;
    int find(int32_t k) const
    {
        for (size_t i = 0; i < key.size(); ++i)
            if (key[i] == k) return (int)i;
        return -1;
    }
    // Every key is assigned exactly once per phase (the candidate lists hold distinct variables: a neighbour list in
    // the interleaving phase, keys(TPC) in the elimination phase), so assignment is an append -- no lookup.
    void set(int32_t k, double s, double p)
    {
        key.push_back(k);
        stat.push_back(s);
        pval.push_back(p);
    }
};

struct Target {
    int32_t T = 0;
    int phase = 0;  // 0 = interleaving, 1 = elimination, 2 = finished
    size_t pos = 0;
    std::vector<int32_t> cands;   // current phase's candidate list
    int32_t nc_dev = -1;          // device rounds: number of candidates in the device-built list (no host copy)
    std::vector<int32_t> acc;     // accepted (conditioning pool)
    ODict TPC, PC;
    const int32_t *wl = nullptr;  // sorted whitelist (snapshot of the running graph)
    int wl_n = 0;
    // speculative posting (interleaving phase): candidates [pos, posted_end) have a job in the pool or a buffered result
    size_t posted_end = 0;
    std::vector<std::pair<int32_t, FwJobOut>> ready;  // finished but not yet committed (candidate index, result)
    // exact elimination (fw_learn_opts.elim_mode 1 / 2, fast_elim = false): every member re-enters the pool whatever its verdict
    // (hiton.jl:67-70), so the pool of member j + 1 is (pool of j without c_{j+1}) + [c_j] -- known before any result.  post_acc:
    // the pool as it will stand before candidate posted_end (elimination phase only)
    int elim_mode = 0;
    std::vector<int32_t> post_acc;
    bool in_wl(int32_t v) const { return wl_n > 0 && std::binary_search(wl, wl + wl_n, v); }
};

// the level-0 lists of the context as the host algorithms of fw_graph.h read them (idx / stat / pval: after fwi_nb_host_ensure)
FwLevel0 level0_view(const fw_ctx *c) { return FwLevel0{c->P.p, c->nb_off.data(), c->nb_idx.data(), c->nb_stat.data(), c->nb_p.data()}; }

// Advance a target until it needs a device test (returns true, job = (T, cands[pos], acc)) or finishes.
bool advance(const FwLevel0 &l0, Target &t)
{
    for (;;) {
        if (t.phase == 2) return false;
        ODict &dict = t.phase == 0 ? t.TPC : t.PC;
        while (t.pos < t.cands.size()) {
            const int32_t cand = t.cands[t.pos];
            if (t.in_wl(cand)) {  // hiton.jl:20-30
                t.acc.push_back(cand);
                dict.set(cand, NAN, NAN);
                ++t.pos;
                continue;
            }
            if (t.phase == 1)  // hiton.jl:134-136
                t.acc.erase(std::remove(t.acc.begin(), t.acc.end(), cand), t.acc.end());
            if (t.acc.empty()) {  // tests.jl:285 sentinel + hiton.jl:57-59
                double s, p;
                if (t.phase == 0) {
                    const int64_t q = l0.find(t.T, cand);
                    s = l0.stat[q];
                    p = l0.pval[q];
                } else {
                    const int i = t.TPC.find(cand);
                    s = t.TPC.stat[i];
                    p = t.TPC.pval[i];
                }
                t.acc.push_back(cand);
                dict.set(cand, s, p);
                ++t.pos;
                continue;
            }
            return true;
        }
        if (t.phase == 0) {  // hiton.jl:242: elimination over keys(TPC) in insertion order
            t.phase = 1;
            t.cands = t.TPC.key;
            t.acc = t.cands;
            t.pos = 0;
            t.posted_end = 0;  // every interleaving candidate has been committed at this point
            t.ready.clear();
            if (t.elim_mode != 0) t.post_acc = t.acc;
        } else {  // hiton.jl:249-256 update_PC_dict!, skipped when fast_elim = no_red_tests = false (:388-390)
            for (size_t i = 0; t.elim_mode != 2 && i < t.PC.key.size(); ++i) {
                const int ti = t.TPC.find(t.PC.key[i]);
                if (ti >= 0 && (t.TPC.pval[ti] > t.PC.pval[i] || std::isnan(t.PC.pval[i]))) {
                    t.PC.stat[i] = t.TPC.stat[ti];
                    t.PC.pval[i] = t.TPC.pval[ti];
                }
            }
            t.phase = 2;
        }
    }
}

// ---- rejection log (fw_set_track_rejections): one slot per directed level-0 entry, on the host for the job pool and in device memory
// for the paths whose state machine lives there; merged and compacted behind the conditional stage ----
struct RejGuard {
    fw_ctx *c;
    ~RejGuard()
    {
        c->d_rej_run = nullptr;
        std::vector<fw_rejection>().swap(c->rej_slots);
    }
};

// empties the slots on both sides; *rej_n: number of slots (0: nothing is logged)
int rej_begin(fw_ctx *c, size_t *rej_n)
{
    c->rej.clear();
    c->rej_slot.clear();
    c->rej_host.clear();
    c->rej_gathered = false;
    *rej_n = c->track_rej != 0 && c->P.max_k > 0 ? (size_t)c->nb_off[c->P.p] : 0;
    c->rej_n_last = *rej_n;
    if (!*rej_n) return FW_OK;
    fw_rejection none;
    memset(&none, 0xff, sizeof(none));  // n_zs = -1: no record
    c->rej_slots.assign(*rej_n, none);
    if (int rc = fw_dev_reserve(c, c->d_rej, sizeof(fw_rejection) * *rej_n)) return rc;
    FW_HIP(c, hipMemset(c->d_rej.ptr, 0xff, sizeof(fw_rejection) * *rej_n));
    FW_HIP(c, hipDeviceSynchronize());  // (the device paths run on non-blocking streams of their own)
    c->d_rej_run = (fw_rejection *)c->d_rej.ptr;
    return FW_OK;
}

// update_sig_result! (hiton.jl:71-76) with track_rejections: the job of (T, cand) against t.acc ended with a test that is not
// significant -> its record goes to the candidate's slot of T's level-0 list (fw_internal.h: rej_slots)
void rej_store(fw_ctx *c, const FwLevel0 &l0, const Target &t, int32_t cand, const FwJobOut &o)
{
    fw_rejection &r = c->rej_slots[(size_t)l0.find(t.T, cand)];
    r = fw_rejection{};
    r.target = t.T;
    r.candidate = cand;
    r.n_zs = o.n_zs;
    for (int q = 0; q < o.n_zs; ++q) r.zs[q] = o.zs[q];
    r.df = o.df;
    r.suff_power = o.suff_power;
    r.phase = t.phase;
    r.n_acc = (int32_t)t.acc.size();
    r.num_tests = o.num_tests;
    r.stat = o.stat;
    r.pval = o.pval;
}

// The slot -> list pass.  Device records win their slot (a target ran on one path only: at most one of the two copies is filled);
// host_slots may be null (fw_rejections_allgather_*: every record is in device memory by then).  Beside every entry the context keeps
// its slot and which side wrote it: what fw_rejections_allgather_* needs of the job pool's slots once they are gone.
int rej_compact(fw_ctx *c, size_t rej_n, const fw_rejection *host_slots)
{
    c->rej.clear();
    c->rej_slot.clear();
    c->rej_host.clear();
    if (rej_n) {
        std::vector<fw_rejection> dev(rej_n);
        FW_HIP(c, hipMemcpy(dev.data(), c->d_rej.ptr, sizeof(fw_rejection) * rej_n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < rej_n; ++i) {
            const bool from_host = dev[i].n_zs < 0;
            if (from_host && !host_slots) continue;
            fw_rejection r = from_host ? host_slots[i] : dev[i];
            if (r.n_zs < 0) continue;
            double total = 0.0;  // tests.jl:313,327-332: every subset of sizes max_k .. 1, not capped by max_tests (integer binomials)
            for (int s = c->P.max_k; s >= 1; --s) total += (double)fw_binom_any(r.n_acc, s);
            r.frac = r.num_tests > 0 && total > 0.0 ? (double)r.num_tests / total : 0.0;
            for (int q = r.n_zs; q < FW_MAX_K; ++q) r.zs[q] = 0;
            c->rej.push_back(r);
            c->rej_slot.push_back((int64_t)i);
            c->rej_host.push_back(from_host ? 1 : 0);
        }
    }
    return FW_OK;
}

int rej_finish(fw_ctx *c, size_t rej_n)
{
    if (int rc = rej_compact(c, rej_n, c->rej_slots.data())) return rc;
    if (c->track_rej != 0) c->have_rej = true;
    return FW_OK;
}

// ---- which path a round takes (DESIGN.md section 4.5 has the table) ----
enum Path { PATH_DEV_SCHEDULE, PATH_DEV_ROUNDS, PATH_HOST_POOL };
const char *const path_name[] = {"device schedule", "device rounds", "host pool"};
struct PathChoice {
    Path path;
    bool dev_cands;   // device rounds: the candidate order already built on the device (fw_bh.hip) is used
    const char *why;  // host pool: the first condition that keeps the round off the device
};

// round == nullptr asks for the whole run: PATH_DEV_SCHEDULE (fwi_devhiton_mi_schedule: discrete kinds on bit planes, one rank, no
// exchange callback, level-0 lists and candidate order on the device, rounds the persistent kernel is worth launching for;
// fwi_devhiton_fz_schedule: fz under the same conditions, when EVERY round of the schedule would take the device rounds), else the
// rounds are asked one by one (`why` then says what kept the schedule off): order[r0 .. r1), n_my of them this rank's.
// Knobs are read per call: the tests and bench.py switch them inside a live process.
// subset: fw_learn_neighbors -- order holds the listed targets alone.  Every count below (nt, the rounds, n_my) is then a count of listed
// targets, and the degrees are read through order[], so the tests hold as they stand; one condition is the subset's own.
PathChoice choose_path(fw_ctx *c, const fw_learn_opts &opt, bool has_exchange, const int32_t *order, int nt, const int *round, size_t n_my, bool subset)
{
    auto host = [](const char *why) { return PathChoice{PATH_HOST_POOL, false, why}; };
    const int kind = c->P.kind;
    const bool discrete = kind == FW_MI || kind == FW_MI_NZ;
    if (fw_host_hiton()) return host("FW_HOST_HITON=1");
    // (the persistent kernel runs four tests per wavefront, the job pool one: another summation order of the same terms, DESIGN.md
    // section 2.  Which of the two a run takes depends on the number of targets -- a target's row would change in its last bits with
    // the length of the list it was named in)
    if (subset && discrete) return host("fw_learn_neighbors, discrete kind: a neighbourhood must not depend on how many targets are listed");
    if (c->f64) return host("Float64 matrix (fw_fz64.hip): the general-form segment kernel serves the host pool");
    if (!discrete && !c->P.recursive_pcor) return host("streamed columns (recursive_pcor = 0): fw_fzs.hip serves the host pool");
    if (!discrete && c->P.n < c->n_obs_min_eff) return host("no power: fewer observations than n_obs_min, no device work at all");
    if (c->mi_generic) return host("generic discrete form (a variable with more than three levels, fw_mi_core.h)");
    if (c->P.max_k > FW_MAX_K_FAST) return host("max_k above FW_MAX_K_FAST: conditioning sets of 6 and 7 variables take the general-form kernels");
    // (test knob)  cfg2 (1000 targets): 19 ms on the device, 28 ms through the host pool; the reference's single_il schedule posts one
    // target per round and would pay the device set-up each time.  Discrete kinds run as one persistent launch (dh_mi_target_kernel):
    // worth it from a few hundred targets on.  (a negative value: every round of the schedule, no round of the per-round paths)
    const long long min_targets = (long long)fw_knob_u64(knob::FW_DEV_MIN_TARGETS, discrete ? 256 : 64);
    if (!round) {
        if (!discrete && kind != FW_FZ) return host("device schedule: not for fz_nz");
        if (has_exchange || opt.world_size > 1) return host("device schedule: exchange callback present");
        if (!c->d_cand || !c->d_nb_idx || !c->d_nb_off) return host("device schedule: level-0 lists not on the device (FW_HOST_BH)");
        if (!discrete) {  // fwi_devhiton_fz_schedule
            if (!fw_knob_on(knob::FW_FZ_SCHED)) return host("device schedule: FW_FZ_SCHED=0");  // (A/B runs, tests/test_gpu_fz_sched.py compares the two)
            if (c->track_rej != 0) return host("device schedule: track_rejections runs on the round loop");
            if (fw_knob_str(knob::FW_DH_LOG)) return host("device schedule: FW_DH_LOG is written by the round loop");
            // (accepted-list buffers of every target at its level-0 offset: 8 * (look-ahead + 1) bytes per level-0 entry)
            if ((unsigned long long)c->nb_off[c->P.p] > (1ull << 27)) return host("device schedule: level-0 lists too long for buffers at level-0 offsets");
            // every round must be one the round loop would give to the device: a round for the host pool keeps the whole run on the loop
            for (int r0 = 0, r1 = 0; r0 < nt; r0 = r1) {
                r1 = fw_round_end(r0, opt.round_size, nt);
                if (r1 - r0 < min_targets) return host("device schedule: a round of fewer targets than FW_DEV_MIN_TARGETS");
            }
            const int R = (opt.round_size <= 0 || opt.round_size > nt) ? nt : opt.round_size;
            if (R < 2) return host("device schedule: single_il");
            // (dh_fz_round_begin_kernel sorts a device-built whitelist, at most the degree long, in 16 KB of LDS by a quadratic rank sort)
            if (opt.feed_forward)
                for (int i = 0; i < nt; ++i)
                    if (c->nb_off[order[i] + 1] - c->nb_off[order[i]] > 4096) return host("device schedule: a level-0 list beyond 4096 entries (whitelist sort)");
            return PathChoice{PATH_DEV_SCHEDULE, true, ""};
        }
        if (fw_mi_rounds()) return host("device schedule: FW_MI_ROUNDS=1");
        if (!fw_knob_on(knob::FW_MI_SCHED)) return host("device schedule: FW_MI_SCHED=0");  // (A/B runs, tests/test_gpu_mi.py compares the two)
        const int R = (opt.round_size <= 0 || opt.round_size > nt) ? nt : opt.round_size;
        // (R = 1 is the reference's single_il master, whose first round holds TWO targets -- fw_round_end knows that rule, the device
        // schedule cuts rounds of exactly R; r05 fuzz, 3 of 4 500 networks with the threshold forced to 1)
        if (R < min_targets || R < 2) return host("device schedule: rounds of fewer targets than FW_DEV_MIN_TARGETS (or single_il)");
        return PathChoice{PATH_DEV_SCHEDULE, true, ""};
    }
    // fz_nz (r05): device rounds when the longest possible list fits the sub-matrix kernel's LDS; FW_NZ_DEV=0 keeps the host pool (A/B, tests)
    if (kind == FW_FZ_NZ) {
        if (!fw_knob_on(knob::FW_NZ_DEV)) return host("FW_NZ_DEV=0");
        int64_t dmax = 0;
        for (int i = round[0]; i < round[1]; ++i) dmax = std::max<int64_t>(dmax, c->nb_off[order[i] + 1] - c->nb_off[order[i]]);
        // (feed-forward: a whitelisted member of the elimination pool is pushed a second time, hiton.jl:24-26 -- a list can reach twice
        // the candidates)
        if (fwi_fznz_dev_limits(c, (int)(opt.feed_forward ? 2 * dmax : dmax) + 2) != FW_OK) return host("fz_nz list too long for the sub-matrix kernel's LDS");
    }
    if ((unsigned long long)n_my < (unsigned long long)min_targets) return host("fewer targets than FW_DEV_MIN_TARGETS");
    return PathChoice{PATH_DEV_ROUNDS, c->d_cand != nullptr, c->d_cand ? "candidate order from the device" : "candidate order built on the host"};
}

// What the stages of one fw_learn_network / fw_learn_neighbors call share.
struct Learn {
    fw_ctx *c;
    fw_learn_opts opt;
    fw_allgather_fn allgather;
    void *user;
    bool discrete;
    size_t rej_n = 0;
    double t0 = 0.0;             // start of the conditional stage
    std::vector<int32_t> order;  // learning.jl:97-98
    int nt = 0;                  // targets of the schedule (fw_learn_opts.max_targets; fw_learn_neighbors: the listed ones)
    bool subset = false;         // fw_learn_neighbors: order holds the listed targets alone, nt of them
    FwDirected all;              // directed results of every target; all ranks hold all of them after each round's exchange
};

// This rank's targets of the round order[r0 .. r1) with their candidate lists (on the host, or nc_dev: the device's) and whitelists.
int build_targets(Learn &L, const FwRunningGraph &graph, const std::vector<int32_t> &owner, int r0, int r1, bool dev_cands, std::vector<Target> &tg)
{
    fw_ctx *c = L.c;
    if (!dev_cands)
        if (int rc = fwi_nb_host_ensure(c)) return rc;
    const FwLevel0 l0 = level0_view(c);
    for (int i = r0; i < r1; ++i) {
        if (owner[i - r0] != L.opt.rank) continue;
        Target t;
        t.T = L.order[i];
        t.elim_mode = L.opt.elim_mode;
        if (L.discrete && c->levels[t.T] < 2) {  // hiton.jl:182-184
            t.phase = 2;
            tg.push_back(std::move(t));
            continue;
        }
        // hiton.jl:211-217: candidates with adj p < alpha, stable sort by p
        const int64_t o = l0.off[t.T];
        const int deg = (int)l0.deg(t.T);
        if (dev_cands) {
            t.nc_dev = deg;  // every stored neighbour has adj p < alpha; the sorted list lives in c->d_cand
            if (deg == 0) t.phase = 2;
        } else {
            std::vector<int32_t> idx;
            for (int q = 0; q < deg; ++q)
                if (l0.pval[o + q] < c->P.alpha) idx.push_back(q);
            std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) { return l0.pval[o + a] < l0.pval[o + b]; });
            for (int32_t q : idx) t.cands.push_back(l0.idx[o + q]);
            if (t.cands.empty()) t.phase = 2;  // hiton.jl:336-338
        }
        if (L.opt.feed_forward) t.wl = graph.whitelist(t.T, &t.wl_n);  // the running graph is only modified between rounds
        tg.push_back(std::move(t));
    }
    return FW_OK;
}

// ---- device leg (fw_devhiton.hip): no host round trip per window ----
// FW_DH_CHAINS = K (default 2, FlashWeave-S): the round's targets are dealt to K independent chains of device rounds that run
// concurrently (own host thread, stream and arena each): while one chain is between two launches (step / plan / fill, the thinning tail
// of its segment kernel) the other keeps the CUs busy.  cfg3, ms per pass with 1 / 2 / 3 / 4 chains: 261.8 / 229.4 / 224.2 / 274.3 on
// one GPU, 70.5 / 62.4 / 63.7 for one rank of eight; the per-launch duration of the segment kernel grows with the overlap (224 -> 167 us
// for launches half the size), which is what HIP events and rocprofv3 see
int chain_count(const fw_ctx *c, size_t n_targets)
{
    // read per round: bench.py times a one-chain pass for the per-kernel figures.  r02: cfg3 227 / 218 / 268 ms with 2 / 3 / 4 in a bare
    // process, but 226 / 298 under torch.distributed.run and 325 with GPU_MAX_HW_QUEUES=8: the third stream's hardware queue is not ours
    // to choose -> 2
    const int dh_chains = std::min(std::max(fw_knob_int(knob::FW_DH_CHAINS, 2), 1), FW_DH_MAX_CHAINS);
    static const size_t dh_chain_min = (size_t)fw_knob_pos(knob::FW_DH_CHAIN_MIN, 48);  // r03: 256 -> 48 (one rank of eight holds 98 targets in cfg3's last round: 75 -> 69 ms with two chains)
    static const int dh_chains_disc = std::min(std::max(fw_knob_int(knob::FW_DH_CHAINS_DISC, 2), 1), FW_DH_MAX_CHAINS);  // cfg4: 248.7 / 232.9 / 227.2 / 253.1 ms with 1 / 2 / 3 / 4
    // discrete kinds run as ONE persistent launch that fills the GPU by itself (dh_mi_target_kernel); concurrent chains only apply to
    // their level-synchronous form (FW_MI_ROUNDS=1)
    static const bool mi_rounds = fw_mi_rounds();
    const int want = c->P.kind == FW_FZ ? dh_chains : (mi_rounds ? dh_chains_disc : 1);
    return n_targets >= (size_t)want * dh_chain_min ? want : 1;
}

// Which chain target i goes to (and its index there).  Default: dealt in schedule order.  Few targets (the latency-bound regime: a rank
// of a multi-GPU job, the last feed-forward round): the heaviest FW_DH_HEAVY_PCT of them get chain 0 to themselves -- its launches stay
// small, so the rounds of the longest chains are short
void deal_chains(size_t n, int K, std::vector<int> &chain_of, std::vector<size_t> &chain_idx)
{
    static const int heavy_pct = fw_knob_int(knob::FW_DH_HEAVY_PCT, 0);
    static const size_t heavy_below = (size_t)fw_knob_u64(knob::FW_DH_HEAVY_BELOW, 512);
    chain_of.assign(n, 0);
    chain_idx.assign(n, 0);
    std::vector<size_t> cnt((size_t)K, 0);
    const bool split = K >= 2 && heavy_pct > 0 && n <= heavy_below;
    const size_t n_heavy = split ? std::max<size_t>(1, n * (size_t)heavy_pct / 100) : 0;
    for (size_t i = 0; i < n; ++i) {
        int q;
        if (split)  // schedule order = ascending degree: the last n_heavy targets are the heaviest
            q = i >= n - n_heavy ? 0 : 1 + (int)(i % (size_t)(K - 1));
        else
            q = (int)(i % (size_t)K);
        chain_of[i] = q;
        chain_idx[i] = cnt[(size_t)q]++;
    }
}

// chain q runs the targets dealt to it, chains 1.. on threads of their own (the round loop; fwi_devhiton_fz_schedule keeps its own)
int run_chains(fw_ctx *c, std::vector<FwDhTarget> &din, const std::vector<int> &chain_of, std::vector<std::vector<FwDhResult>> &pres,
               std::vector<FwDhFlat> &pflat)
{
    const int K = (int)pres.size();
    if (K == 1) return fwi_devhiton_run(c, din, pres[0], pflat[0]);
    std::vector<std::vector<FwDhTarget>> part((size_t)K);
    for (size_t i = 0; i < din.size(); ++i) part[(size_t)chain_of[i]].push_back(std::move(din[i]));
    std::vector<int> rcs((size_t)K, FW_OK);
    std::vector<std::thread> th;
    for (int q = 1; q < K; ++q)
        th.emplace_back([&, q] {
            (void)hipSetDevice(c->P.device);
            rcs[q] = fwi_devhiton_run(c, part[q], pres[q], pflat[q], q);
        });
    rcs[0] = fwi_devhiton_run(c, part[0], pres[0], pflat[0], 0);
    for (std::thread &t : th) t.join();
    int rc = FW_OK;
    for (int q = 0; q < K; ++q)
        if (rcs[q]) rc = rcs[q];
    return rc;
}

// the round on the device: its directed results go to `out` straight from the chains' flat arrays, every target ends finished
int run_device_round(Learn &L, std::vector<Target> &tg, bool dev_cands, FwDirected &out)
{
    fw_ctx *c = L.c;
    std::vector<FwDhTarget> din(tg.size());
    for (size_t i = 0; i < tg.size(); ++i) {
        din[i].T = tg[i].T;
        if (tg[i].phase != 2) {
            din[i].cands = tg[i].cands;
            din[i].nc_dev = tg[i].nc_dev;
        } else if (dev_cands) {
            din[i].nc_dev = 0;
        }
        din[i].wl = tg[i].wl;
        din[i].wl_n = tg[i].wl_n;
    }
    const double tdev0 = fwi_now_s();
    if (fw_trace_host()) fprintf(stderr, "[fw] round set-up on the host: %.2f ms\n", 1e3 * (tdev0 - L.t0));
    const int K = chain_count(c, din.size());
    std::vector<int> chain_of;
    std::vector<size_t> chain_idx;
    deal_chains(din.size(), K, chain_of, chain_idx);
    std::vector<std::vector<FwDhResult>> pres((size_t)K);
    std::vector<FwDhFlat> pflat((size_t)K);
    if (int rc = run_chains(c, din, chain_of, pres, pflat)) return rc;
    if (fw_trace_host()) fprintf(stderr, "[fw] device rounds (all chains): %.2f ms\n", 1e3 * (fwi_now_s() - tdev0));
    size_t nres = 0;
    for (size_t i = 0; i < tg.size(); ++i) nres += (size_t)pres[(size_t)chain_of[i]][chain_idx[i]].n;
    out.reserve(nres);
    for (size_t i = 0; i < tg.size(); ++i) {
        const FwDhResult &r = pres[(size_t)chain_of[i]][chain_idx[i]];
        const FwDhFlat &f = pflat[(size_t)chain_of[i]];
        for (int32_t j = 0; j < r.n; ++j) out.push(tg[i].T, f.key[(size_t)r.off + j], f.stat[(size_t)r.off + j], f.pval[(size_t)r.off + j]);
        tg[i].phase = 2;
    }
    return FW_OK;
}

// ---- host leg: asynchronous job pool with speculative candidates ----
// A rejected candidate leaves the accepted set unchanged (hiton.jl:67-70), so during the interleaving phase the next FW_SPEC_DEPTH
// candidates of a target are posted together against the current accepted set; results are committed strictly in candidate order, and
// the first acceptance bumps the target's epoch, which cancels / voids everything posted after it.  The sequence of committed
// (T, candidate, accepted) jobs is therefore exactly the reference's; only the number of latency-bound rounds shrinks.  Every pool
// round = one window of every in-flight job = ONE kernel launch.
struct HostPool {
    std::vector<Target> &tg;
    FwLevel0 l0;
    bool log_rej;  // the rejection log keeps the conditioning set of the stopping test
    FwPool pool;
    std::vector<int32_t> epoch;  // per target: bumped when its accepted set changes
    std::vector<int> touched;    // targets with new results (at first: all)
    std::vector<uint8_t> is_touched;
    long n_unfinished;
};

// commit the finished results of target ti in candidate order; false: the target has finished
bool pool_commit(fw_ctx *c, HostPool &S, int ti)
{
    Target &t = S.tg[ti];
    while (advance(S.l0, t)) {
        int ri = -1;
        for (size_t q = 0; q < t.ready.size(); ++q)
            if ((size_t)t.ready[q].first == t.pos) {
                ri = (int)q;
                break;
            }
        if (ri < 0) break;
        const FwJobOut o = t.ready[ri].second;
        t.ready.erase(t.ready.begin() + ri);
        c->cnt.cond_tests_ref += o.num_tests;
        c->cnt.subsets_calls += 1;
        const int32_t cand = t.cands[t.pos];
        ++t.pos;
        const bool exact = t.elim_mode != 0 && t.phase == 1;  // the pool grows either way: nothing posted is void
        if (o.pval < c->P.alpha && o.suff_power) {  // issig, tests.jl:1-3; hiton.jl:61-63
            t.acc.push_back(cand);
            (t.phase == 0 ? t.TPC : t.PC).set(cand, o.stat, o.pval);
            if (!exact) {
                ++S.epoch[ti];  // accepted set changed: later speculative jobs / results are void
                t.ready.clear();
                t.posted_end = t.pos;
            }
        } else {
            if (S.log_rej) rej_store(c, S.l0, t, cand, o);  // hiton.jl:71-76
            if (exact) t.acc.push_back(cand);               // hiton.jl:67-70
        }
    }
    return t.phase != 2;
}

void pool_post_job(fw_ctx *c, HostPool &S, int ti, size_t ci, const std::vector<int32_t> &acc)
{
    fwi_pool_add(c, S.pool, S.tg[ti].T, S.tg[ti].cands[ci], acc.data(), (int)acc.size(), ti);
    S.pool.live.back().aux = (int32_t)ci;
    S.pool.live.back().epoch = S.epoch[ti];
}

// post the next jobs of target ti: the current candidate, plus speculative ones while interleaving.  Speculation is only used once few
// targets are left (the latency-bound tail); with thousands of active targets the launches are full anyway and the extra host
// bookkeeping would cost more than the saved rounds.
void pool_post(fw_ctx *c, HostPool &S, int ti)
{
    static const int FW_SPEC_DEPTH = fw_knob_int(knob::FW_SPEC_DEPTH, 8);
    static const long FW_SPEC_TARGETS = (long)fw_knob_u64(knob::FW_SPEC_TARGETS, 512);
    Target &t = S.tg[ti];
    if (t.elim_mode != 0 && t.phase == 1) {
        // exact elimination: every member's job at once, each against its own pool (they are independent)
        if (t.posted_end < t.pos) {  // (members advance() settled without a test: t.acc is the pool before t.pos)
            t.posted_end = t.pos;
            t.post_acc = t.acc;
        }
        for (; t.posted_end < t.cands.size(); ++t.posted_end) {
            const int32_t cand = t.cands[t.posted_end];
            if (t.in_wl(cand)) {  // hiton.jl:20-30: pushed once more, no test (advance() records it)
                t.post_acc.push_back(cand);
                continue;
            }
            t.post_acc.erase(std::remove(t.post_acc.begin(), t.post_acc.end(), cand), t.post_acc.end());
            if (!t.post_acc.empty()) pool_post_job(c, S, ti, t.posted_end, t.post_acc);  // (an empty pool is the sentinel of advance(): no test)
            t.post_acc.push_back(cand);
        }
        return;
    }
    if (t.posted_end < t.pos) t.posted_end = t.pos;
    const size_t depth = S.n_unfinished <= FW_SPEC_TARGETS ? (size_t)FW_SPEC_DEPTH : 1;
    const size_t limit = t.phase == 0 ? std::min(t.cands.size(), t.pos + depth) : t.pos + 1;
    for (; t.posted_end < limit; ++t.posted_end) {
        if (t.posted_end > t.pos && t.in_wl(t.cands[t.posted_end])) break;  // a whitelisted candidate will change the accepted set
        pool_post_job(c, S, ti, t.posted_end, t.acc);
    }
}

// the round through the job pool: every target ends finished, its results in its PC
int run_host_pool(Learn &L, std::vector<Target> &tg)
{
    fw_ctx *c = L.c;
    HostPool S{tg, level0_view(c), L.rej_n != 0, {}, std::vector<int32_t>(tg.size(), 0), std::vector<int>(tg.size()), std::vector<uint8_t>(tg.size(), 0),
               (long)tg.size()};
    S.pool.want_zs = S.log_rej;
    S.pool.owner_epoch = &S.epoch;
    std::iota(S.touched.begin(), S.touched.end(), 0);
    std::vector<FwPoolJob> fin;
    for (;;) {
        const double ta0 = fwi_now_s();
        for (int ti : S.touched) {
            S.is_touched[ti] = 0;
            if (pool_commit(c, S, ti))
                pool_post(c, S, ti);
            else
                --S.n_unfinished;
        }
        S.touched.clear();
        // a speculative job (not the head candidate of its target) only ever runs its first window: most rejections happen within the
        // first few tests, and a voided long job would be pure waste (exact elimination: no job is speculative)
        for (FwPoolJob &j : S.pool.live) {
            const Target &t = tg[(size_t)j.tag];
            j.hold = (size_t)j.aux != t.pos && j.next > 0 && !(t.elim_mode != 0 && t.phase == 1);
        }
        c->cnt.t_host_advance_s += fwi_now_s() - ta0;
        if (S.pool.live.empty()) break;
        fin.clear();
        if (int rc = fwi_pool_round(c, S.pool, fin)) return rc;
        const double ta1 = fwi_now_s();
        for (FwPoolJob &j : fin) {
            const int ti = (int)j.tag;
            c->cnt.cond_tests_evaluated += j.out.evaluated;
            c->cnt.alg_bytes_subsets += fwi_alg_bytes(c, (int)j.acc.size(), j.out.evaluated);
            if (j.epoch != S.epoch[ti]) continue;  // posted before an acceptance: void
            tg[ti].ready.emplace_back(j.aux, j.out);
            if (!S.is_touched[ti]) {
                S.is_touched[ti] = 1;
                S.touched.push_back(ti);
            }
        }
        c->cnt.t_host_advance_s += fwi_now_s() - ta1;
    }
    c->cnt.cond_tests_evaluated += S.pool.dropped_evaluated;
    c->cnt.alg_bytes_subsets += S.pool.dropped_alg_bytes;
    return FW_OK;
}

// exchange this round's directed results (mine: the device leg's, plus the PCs of the host leg's targets) and keep the running graph
int exchange_round(Learn &L, const std::vector<Target> &tg, FwDirected &mine, FwRunningGraph &graph, bool need_graph)
{
    for (const Target &t : tg)
        for (size_t i = 0; i < t.PC.key.size(); ++i) mine.push(t.T, t.PC.key[i], t.PC.stat[i], t.PC.pval[i]);
    int64_t ntot = (int64_t)mine.size();
    const int32_t *at = mine.t.data(), *an = mine.u.data();
    const double *as = mine.s.data(), *ap = mine.p.data();
    if (L.allgather) {  // also with world_size = 1 (the callback then returns what it was given): one code path
        int rc = L.allgather(L.user, (int64_t)mine.size(), mine.t.data(), mine.u.data(), mine.s.data(), mine.p.data(), &ntot, &at, &an, &as, &ap);
        if (rc) return fw_fail(L.c, FW_ERR_ARG, "fw_learn_network: allgather callback failed (%d)", rc);
    }
    L.all.append(at, an, as, ap, (size_t)ntot);
    if (need_graph) graph.add(at, an, ntot);
    return FW_OK;
}

// the feed-forward rounds (interleaved.jl:112-183 as level-synchronous rounds): deal, path, targets, one leg, exchange
int run_rounds(Learn &L)
{
    fw_ctx *c = L.c;
    const FwLevel0 l0 = level0_view(c);  // (offsets only: the lists may still live on the device)
    FwRunningGraph graph(c->P.p);
    for (int r0 = 0, r1 = 0; r0 < L.nt; r0 = r1) {
        r1 = fw_round_end(r0, L.opt.round_size, L.nt);
        const std::vector<int32_t> owner = fw_deal_round(l0, L.order.data(), r0, r1, L.opt.world_size, c->P.max_k);
        const size_t n_my = (size_t)std::count(owner.begin(), owner.end(), L.opt.rank);
        const int round[2] = {r0, r1};
        const PathChoice path = choose_path(c, L.opt, L.allgather != nullptr, L.order.data(), L.nt, round, n_my, L.subset);
        if (fw_trace_host()) fprintf(stderr, "[fw] round of targets %d..%d (%zu here): %s (%s)\n", r0, r1, n_my, path_name[path.path], path.why);
        std::vector<Target> tg;
        tg.reserve(n_my);
        if (int rc = build_targets(L, graph, owner, r0, r1, path.dev_cands, tg)) return rc;
        FwDirected mine;
        if (int rc = path.path == PATH_DEV_ROUNDS ? run_device_round(L, tg, path.dev_cands, mine) : run_host_pool(L, tg)) return rc;
        // (only the whitelists of later rounds read the running graph: nothing to maintain after the last round or without
        // feed-forward -- cfg4, one round: 380 000 appends and 50 000 sorts for nothing)
        if (int rc = exchange_round(L, tg, mine, graph, L.opt.feed_forward && r1 < L.nt)) return rc;
    }
    return FW_OK;
}

// learning.jl:171-172 (max_k = 0): the level-0 lists are the network.  targets == nullptr: every variable, ascending; else the rows of
// targets[0 .. nt) alone (fw_learn_neighbors; the CSR over targets of fw_graph.h does not depend on the order of the rows)
int level0_as_directed(fw_ctx *c, const int32_t *targets, int nt, FwDirected &all)
{
    if (int rc = fwi_nb_host_ensure(c)) return rc;
    const FwLevel0 l0 = level0_view(c);
    for (int i = 0; i < (targets ? nt : l0.p); ++i) {
        const int v = targets ? targets[i] : i;
        for (int64_t q = l0.off[v]; q < l0.off[v + 1]; ++q) all.push(v, l0.idx[q], l0.stat[q], l0.pval[q]);
    }
    return FW_OK;
}

// max_k = 0 / device schedule of the whole run / round loop -> L.all
int conditional_stage(Learn &L)
{
    fw_ctx *c = L.c;
    if (c->P.max_k == 0) return level0_as_directed(c, L.subset ? L.order.data() : nullptr, L.nt, L.all);
    const PathChoice whole = choose_path(c, L.opt, L.allgather != nullptr, L.order.data(), L.nt, nullptr, 0, L.subset);
    if (whole.path != PATH_DEV_SCHEDULE) {
        if (fw_trace_host()) fprintf(stderr, "[fw] no %s\n", whole.why);
        return run_rounds(L);
    }
    // the whole schedule stays on the device (whitelists built between the launches, one download at the end) -- same kernel, order
    // and team sizes per round as the round loop
    const int R = L.opt.round_size <= 0 ? L.nt : L.opt.round_size;
    return L.discrete ? fwi_devhiton_mi_schedule(c, L.order.data(), L.nt, R, L.opt.feed_forward != 0, L.all)
                      : fwi_devhiton_fz_schedule(c, L.order.data(), L.nt, R, L.opt.feed_forward != 0, L.all);
}

// make_weights / make_symmetric_graph (fw_graph.h) on the host threads of the context
int graph_stage(fw_ctx *c, const FwDirected &all, bool discrete)
{
    const double tp0 = fwi_now_s();
    if (discrete)
        if (int rc = fwi_nb_host_ensure(c)) return rc;
    const double tp1 = fwi_now_s();
    if (fw_trace_host()) fprintf(stderr, "[fw] neighbour lists to the host: %.2f ms\n", 1e3 * (tp1 - tp0));
    const size_t ne = all.size();
    const int n_thr = ne < 20000 ? 1 : (int)std::min<size_t>(8, std::max(1u, std::thread::hardware_concurrency()));
    if (n_thr > 1 && (!c->host_workers || c->host_workers->blocks() != n_thr)) {
        fwi_host_workers_free(c);
        c->host_workers = new FwHostWorkers(n_thr);
    }
    FwGraphTimes tm;
    if (!fw_graph_passes(level0_view(c), all, discrete, n_thr, c->host_workers, c->net, tm))
        return fw_fail(c, FW_ERR_NOMEM, "weights / symmetric graph: a host block ran out of memory");
    c->have_network = true;
    if (fw_trace_host()) {
        fprintf(stderr, "[fw] weights + symmetric graph on the host: %.2f ms (directed CSR %.2f, signs %.2f, transpose %.2f, edges %.2f; %d threads)\n",
                1e3 * (fwi_now_s() - tp1), 1e3 * tm.csr, 1e3 * tm.signs, 1e3 * tm.transpose, 1e3 * tm.edges, n_thr);
        fprintf(stderr, "[fw]   edges pass: latest start %.3f ms after the call, longest block %.3f ms, return %.3f ms, concatenation %.3f ms (ne %zu)\n",
                1e3 * tm.latest_start, 1e3 * tm.longest_block, 1e3 * tm.edges_return, 1e3 * tm.concatenation, ne);
    }
    return FW_OK;
}

// The per-round exchange of fw_learn_network through a fw_dev_exchange (fw_learn_network_dev): the round's directed entries are
// packed into 24-byte records here (no numpy on the way), copied into the caller's device send buffer, all-gathered by the caller's
// collective (RCCL on torch tensors in bench.py) and unpacked from the gathered buffer.  Implements fw_allgather_fn.
struct DevXRec {
    int32_t t, u;
    double s, p;
};
static_assert(sizeof(DevXRec) == 24, "round exchange record");
struct DevXAdapter {
    fw_ctx *c;
    const fw_dev_exchange *x;
    int world;
    std::vector<DevXRec> stage;
    FwDirected got;
};
int devx_allgather(void *user, int64_t n, const int32_t *tgt, const int32_t *nbr, const double *stat, const double *pval, int64_t *n_total,
                   const int32_t **tgt_all, const int32_t **nbr_all, const double **stat_all, const double **pval_all)
{
    DevXAdapter *A = (DevXAdapter *)user;
    std::vector<int64_t> counts((size_t)A->world, 0), aux((size_t)A->world, 0);
    void *d_send = nullptr, *d_recv = nullptr;
    int64_t cap = 0;
    if (A->x->prepare(A->x->user, n, 0, (int32_t)sizeof(DevXRec), &d_send, &d_recv, counts.data(), aux.data(), &cap)) return 1;
    if (n > cap || !d_recv || (n > 0 && !d_send)) return 2;
    A->stage.resize((size_t)std::max<int64_t>(n, 1));
    for (int64_t i = 0; i < n; ++i) A->stage[(size_t)i] = DevXRec{tgt[i], nbr[i], stat[i], pval[i]};
    if (n > 0 && hipMemcpy(d_send, A->stage.data(), (size_t)n * sizeof(DevXRec), hipMemcpyHostToDevice) != hipSuccess) return 3;
    if (A->x->exchange(A->x->user)) return 4;
    int64_t total = 0;
    for (int r = 0; r < A->world; ++r) {
        if (counts[(size_t)r] < 0 || counts[(size_t)r] > cap) return 5;
        total += counts[(size_t)r];
    }
    A->stage.resize((size_t)std::max<int64_t>(total, 1));
    int64_t off = 0;
    for (int r = 0; r < A->world; ++r) {
        const int64_t k = counts[(size_t)r];
        if (k > 0 && hipMemcpy(A->stage.data() + off, (const char *)d_recv + (size_t)r * (size_t)cap * sizeof(DevXRec), (size_t)k * sizeof(DevXRec),
                               hipMemcpyDeviceToHost) != hipSuccess)
            return 6;
        off += k;
    }
    FwDirected &g = A->got;
    g.resize((size_t)std::max<int64_t>(total, 1));
    for (int64_t i = 0; i < total; ++i) {
        const DevXRec &q = A->stage[(size_t)i];
        g.t[(size_t)i] = q.t, g.u[(size_t)i] = q.u, g.s[(size_t)i] = q.s, g.p[(size_t)i] = q.p;
    }
    *n_total = total;
    *tgt_all = g.t.data();
    *nbr_all = g.u.data();
    *stat_all = g.s.data();
    *pval_all = g.p.data();
    return 0;
}

// dense rules + mi_nz: HITON-PC hands test_subsets a row view of the data (prepare_nzdata, hiton.jl:41-50,85,193); the kernels apply
// it as one more AND plane.  Restored on every exit path by the guard.
struct ViewGuard {
    fw_ctx *c;
    int old;
    ~ViewGuard() { c->mi_view = old; }
};
struct ElimGuard {  // the device rounds read the mode from the context (fw_devhiton.hip)
    fw_ctx *c;
    ~ElimGuard() { c->elim_mode = 0; }
};

}  // namespace

int fwi_chain_count(const fw_ctx *c, size_t n_targets) { return chain_count(c, n_targets); }
int fwi_rej_compact(fw_ctx *c, size_t rej_n, const fw_rejection *host_slots) { return rej_compact(c, rej_n, host_slots); }
void fwi_deal_chains(size_t n, int K, std::vector<int> &chain_of, std::vector<size_t> &chain_idx) { deal_chains(n, K, chain_of, chain_idx); }

void fwi_host_workers_free(fw_ctx *c)
{
    delete c->host_workers;
    c->host_workers = nullptr;
}

namespace {

// The body fw_learn_network and fw_learn_neighbors share, behind their argument checks: level 0 (if not yet run), the schedule, the
// conditional stage, the rejection log, the graph.  targets == nullptr: every variable in schedule order, the first
// fw_learn_opts.max_targets of them; else the listed variables alone, in the order the schedule gives them -- every consumer of
// order / nt below reads that list only, and what is sized per variable (round_of, the whitelist counts, the level-0 offsets the
// targets' lists sit at, the rejection slots) stays sized for all p.
int learn_body(Learn &L, const int32_t *targets, int32_t n_targets, int64_t *n_edges_out)
{
    fw_ctx *c = L.c;
    const fw_learn_opts &opt = L.opt;
    if (!c->have_level0)
        if (int rc = fw_level0(c, nullptr)) return rc;
    ViewGuard view_guard{c, c->mi_view};
    c->mi_view = 1;
    ElimGuard elim_guard{c};
    c->elim_mode = opt.elim_mode;
    RejGuard rej_guard{c};
    if (int rc = rej_begin(c, &L.rej_n)) return rc;
    c->rej_rank = opt.rank;
    c->rej_world = opt.world_size;
    L.t0 = fwi_now_s();
    L.order = fw_target_order(level0_view(c));
    L.nt = opt.max_targets > 0 && opt.max_targets < c->P.p ? opt.max_targets : c->P.p;
    if (targets) {
        std::vector<uint8_t> listed((size_t)c->P.p, 0);
        for (int32_t i = 0; i < n_targets; ++i) listed[(size_t)targets[i]] = 1;
        L.order.erase(std::remove_if(L.order.begin(), L.order.end(), [&](int32_t v) { return !listed[(size_t)v]; }), L.order.end());
        L.nt = (int)L.order.size();
        L.subset = true;
    }

    if (int rc = conditional_stage(L)) return rc;
    if (int rc = rej_finish(c, L.rej_n)) return rc;
    c->cnt.t_cond_s += fwi_now_s() - L.t0;
    if (fw_trace_host()) fprintf(stderr, "[fw] conditional stage: %.2f ms\n", 1e3 * (fwi_now_s() - L.t0));

    if (int rc = graph_stage(c, L.all, L.discrete)) return rc;
#ifdef FW_FZ_FASTDBG
    fwi_fz_fastdbg_print();
#endif
    if (n_edges_out) *n_edges_out = (int64_t)c->net.e_src.size();
    return FW_OK;
}

}  // namespace

extern "C" int fw_learn_network(fw_ctx *c, const fw_learn_opts *opts_in, fw_allgather_fn allgather, void *user, int64_t *n_edges_out)
{
    if (!c) return fw_fail(nullptr, FW_ERR_ARG, "NULL context");
    (void)hipSetDevice(c->P.device);
    Learn L{c, fw_learn_opts{}, allgather, user, c->P.kind == FW_MI || c->P.kind == FW_MI_NZ};
    fw_learn_opts &opt = L.opt;
    opt.feed_forward = 1;
    opt.round_size = 1;
    opt.world_size = 1;
    if (opts_in) opt = *opts_in;
    if (opt.world_size < 1) opt.world_size = 1;
    if (opt.rank < 0 || opt.rank >= opt.world_size) return fw_fail(c, FW_ERR_ARG, "fw_learn_network: rank %d outside world of %d", opt.rank, opt.world_size);
    if (opt.world_size > 1 && !allgather) return fw_fail(c, FW_ERR_ARG, "fw_learn_network: world_size > 1 needs an allgather callback");
    if (opt.elim_mode < 0 || opt.elim_mode > 2) return fw_fail(c, FW_ERR_ARG, "fw_learn_network: elim_mode %d is not 0, 1 or 2", opt.elim_mode);
    return learn_body(L, nullptr, 0, n_edges_out);
}

// si_HITON_PC(T, data; ...) (hiton.jl:402-409) for a list of targets: every refusal before anything runs, then the shared body
extern "C" int fw_learn_neighbors(fw_ctx *c, const fw_learn_opts *opts_in, const int32_t *targets, int32_t n_targets, int64_t *n_edges_out)
{
    if (!c) return fw_fail(nullptr, FW_ERR_ARG, "NULL context");
    if (!targets) return fw_fail(c, FW_ERR_ARG, "fw_learn_neighbors: targets is NULL");
    if (n_targets < 1) return fw_fail(c, FW_ERR_ARG, "fw_learn_neighbors: n_targets %d: at least one target", n_targets);
    Learn L{c, fw_learn_opts{}, nullptr, nullptr, c->P.kind == FW_MI || c->P.kind == FW_MI_NZ};
    fw_learn_opts &opt = L.opt;  // (all zero: no feed-forward, one round, fast_elim)
    if (opts_in) opt = *opts_in;
    if (opt.feed_forward != 0)
        return fw_fail(c, FW_ERR_ARG, "fw_learn_neighbors: feed_forward %d: every neighbourhood is learned on its own, pass 0", opt.feed_forward);
    if (opt.world_size > 1) return fw_fail(c, FW_ERR_ARG, "fw_learn_neighbors: world_size %d: sharded runs are not served", opt.world_size);
    if (opt.rank != 0) return fw_fail(c, FW_ERR_ARG, "fw_learn_neighbors: rank %d: sharded runs are not served", opt.rank);
    if (opt.max_targets != 0) return fw_fail(c, FW_ERR_ARG, "fw_learn_neighbors: max_targets %d: the list names the targets, pass 0", opt.max_targets);
    if (opt.elim_mode < 0 || opt.elim_mode > 2) return fw_fail(c, FW_ERR_ARG, "fw_learn_neighbors: elim_mode %d is not 0, 1 or 2", opt.elim_mode);
    opt.world_size = 1;
    {
        std::vector<uint8_t> seen((size_t)c->P.p, 0);
        for (int32_t i = 0; i < n_targets; ++i) {
            const int32_t v = targets[i];
            if (v < 0 || v >= c->P.p) return fw_fail(c, FW_ERR_ARG, "fw_learn_neighbors: targets[%d] = %d is outside 0 .. %d", i, v, c->P.p - 1);
            if (seen[(size_t)v]) return fw_fail(c, FW_ERR_ARG, "fw_learn_neighbors: targets[%d] = %d is a duplicate", i, v);
            seen[(size_t)v] = 1;
        }
    }
    (void)hipSetDevice(c->P.device);
    return learn_body(L, targets, n_targets, n_edges_out);
}

extern "C" int fw_learn_network_dev(fw_ctx *c, const fw_learn_opts *opts_in, const fw_dev_exchange *x, int64_t *n_edges_out)
{
    if (!c) return fw_fail(nullptr, FW_ERR_ARG, "NULL context");
    const int world = opts_in ? std::max(opts_in->world_size, 1) : 1;
    if (world > 1 && (!x || !x->prepare || !x->exchange)) return fw_fail(c, FW_ERR_ARG, "fw_learn_network_dev: world_size > 1 needs both exchange callbacks");
    if (c->f64) return fw_fail(c, FW_ERR_LIMIT, "fw_learn_network_dev is not served in Float64 mode");
    if (!x) return fw_learn_network(c, opts_in, nullptr, nullptr, n_edges_out);
    (void)hipSetDevice(c->P.device);
    DevXAdapter A{c, x, world, {}, {}};
    return fw_learn_network(c, opts_in, devx_allgather, &A, n_edges_out);
}

extern "C" int fw_network_get(const fw_ctx *c, int32_t *src, int32_t *dst, double *weight)
{
    if (!c) return fw_fail(nullptr, FW_ERR_ARG, "NULL context");
    if (!c->have_network) return fw_fail(c, FW_ERR_STATE, "fw_network_get: fw_learn_network has not run");
    const FwNetwork &g = c->net;
    const size_t k = g.e_src.size();
    if (k) {
        if (src) memcpy(src, g.e_src.data(), sizeof(int32_t) * k);
        if (dst) memcpy(dst, g.e_dst.data(), sizeof(int32_t) * k);
        if (weight) memcpy(weight, g.e_w.data(), sizeof(double) * k);
    }
    return FW_OK;
}

extern "C" int fw_network_get_directed(const fw_ctx *c, int64_t *off, int32_t *idx, double *weight, double *pval)
{
    if (!c) return fw_fail(nullptr, FW_ERR_ARG, "NULL context");
    if (!c->have_network) return fw_fail(c, FW_ERR_STATE, "fw_network_get_directed: fw_learn_network has not run");
    const FwNetwork &g = c->net;
    if (off) memcpy(off, g.pc_off.data(), sizeof(int64_t) * g.pc_off.size());
    const size_t k = g.pc_idx.size();
    if (k) {
        if (idx) memcpy(idx, g.pc_idx.data(), sizeof(int32_t) * k);
        if (weight) memcpy(weight, g.pc_w.data(), sizeof(double) * k);
        if (pval) memcpy(pval, g.pc_p.data(), sizeof(double) * k);
    }
    return FW_OK;
}
