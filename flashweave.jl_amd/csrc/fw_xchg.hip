// Device-resident exchange of level-0 results between the ranks of a target-sharded run (fw_level0_sharded_dev): the significant
// pairs a rank's share of the pair tiles produced are packed into 24-byte records straight inside a send buffer the CALLER owns
// (torch tensors in bench.py: RCCL all-gathers them over xGMI without a host copy), and the gathered, rank-padded buffer is
// compacted back into the structure-of-arrays form the BH / neighbour-list epilogue (fw_bh.hip) reads.  r02 sent the same data
// through pinned host memory, numpy and a C callback: 8.8 s per cfg4 pass over gloo, which made level-0 sharding unusable.
//
// The rejection log of a target-sharded run (fw_rejections_allgather_dev / _comm) travels the same way: every rank packs the filled
// slots of its slot array (fw_internal.h: one 88-byte fw_rejection per directed level-0 entry, n_zs < 0 = empty) into the send buffer,
// the blocks are gathered, and every rank scatters the other ranks' records into its own slot array.  A record carries its SLOT INDEX
// beside the 88 bytes (96-byte wire record): level 0 is replicated, so a slot means the same (target, candidate) on every rank, and the
// receiver places a record without looking anything up -- the kernels never read the level-0 lists, which is why the same path serves
// a context whose lists are not resident on the device (FW_HOST_BH).  The slot -> list pass of the conditional stage
// (fwi_rej_compact) then rebuilds ctx->rej from the slots: order and frac are those of a one-rank log by construction.
#include <algorithm>

#include "fw_internal.h"

namespace {

struct FwL0Rec {  // wire format: 24 bytes
    int32_t i, j;
    double stat, pval;
};
static_assert(sizeof(FwL0Rec) == 24, "level-0 exchange record");

__global__ __launch_bounds__(256) void l0_pack_kernel(const int32_t *__restrict__ i, const int32_t *__restrict__ j,
                                                      const double *__restrict__ s, const double *__restrict__ p, long long k,
                                                      FwL0Rec *__restrict__ out)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= k) return;
    FwL0Rec r;
    r.i = i[t];
    r.j = j[t];
    r.stat = s[t];
    r.pval = p[t];
    out[t] = r;
}

// recv: world blocks of cap records, block r holds counts[r] of them; off[r] = exclusive prefix sum of counts
__global__ __launch_bounds__(256) void l0_unpack_kernel(const FwL0Rec *__restrict__ recv, long long cap, int world,
                                                        const long long *__restrict__ off, long long total, int32_t *__restrict__ i,
                                                        int32_t *__restrict__ j, double *__restrict__ s, double *__restrict__ p)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    int r = 0;
    while (r + 1 < world && off[r + 1] <= t) ++r;  // world <= a few dozen
    const FwL0Rec v = recv[(long long)r * cap + (t - off[r])];
    i[t] = v.i;
    j[t] = v.j;
    s[t] = v.stat;
    p[t] = v.pval;
}

struct FwRejRec {  // wire format: 96 bytes
    fw_rejection r;
    long long slot;
};
static_assert(sizeof(fw_rejection) == 88 && sizeof(FwRejRec) == 96, "rejection log exchange record");

// counters of one gather, in device memory (zeroed before the first kernel)
enum { RJ_CURSOR = 0, RJ_PLACED, RJ_COLLISIONS, RJ_BAD_SLOTS, RJ_COUNTERS };

// Filled slots -> the send buffer, compactly.  Offsets: the filled lanes of a wavefront are counted by ballot, lane 0 reserves their
// run with one atomic, each takes its place in it; the order between wavefronts is whatever the atomics give (the receiver places by
// slot).  Nothing is written past `cap` records: the cursor then says how many there would have been and the host refuses.
__global__ __launch_bounds__(256) void rej_pack_kernel(const fw_rejection *__restrict__ slots, long long n_slots, FwRejRec *__restrict__ out,
                                                       long long cap, unsigned long long *__restrict__ ctr)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool filled = t < n_slots && slots[t].n_zs >= 0;
    const unsigned long long m = __ballot(filled);
    if (m == 0ull) return;
    const int lane = threadIdx.x & 63;
    unsigned long long base = 0ull;
    if (lane == __ffsll((long long)m) - 1) base = atomicAdd(&ctr[RJ_CURSOR], (unsigned long long)__popcll(m));
    base = __shfl(base, __ffsll((long long)m) - 1, 64);
    if (!filled) return;
    const long long at = (long long)base + __popcll(m & ((1ull << lane) - 1ull));
    if (at >= cap) return;
    FwRejRec v;
    v.r = slots[t];
    v.slot = t;
    out[at] = v;
}

// Records -> their slots.  recs: `blocks` blocks of `stride` records, block b holds counts[b] of them; block `skip` (this rank's own
// in the gathered buffer, -1: none) is left out.  A slot is claimed by a compare-and-swap on its n_zs (-1 = empty), so that two
// records for one slot are SEEN whatever their timing.  strict = 0 (the host job pool's records on their way into the device slots):
// a taken slot keeps what it has -- the device record wins.  strict = 1 (the gathered blocks): targets are disjoint across ranks, a
// taken slot is a collision and is counted, as is a slot outside the array; the host then refuses the whole gather.
__global__ __launch_bounds__(256) void rej_place_kernel(const FwRejRec *__restrict__ recs, long long stride, int blocks, const long long *__restrict__ counts,
                                                        int skip, fw_rejection *__restrict__ slots, long long n_slots, int strict,
                                                        unsigned long long *__restrict__ ctr)
{
    const int b = blockIdx.y;
    if (b >= blocks || b == skip) return;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= counts[b] || t >= stride) return;
    const FwRejRec v = recs[(long long)b * stride + t];
    if (v.slot < 0 || v.slot >= n_slots || v.r.n_zs < 0) {
        atomicAdd(&ctr[RJ_BAD_SLOTS], 1ull);
        return;
    }
    fw_rejection *dst = slots + v.slot;
    if (atomicCAS(&dst->n_zs, -1, v.r.n_zs) != -1) {
        if (strict) atomicAdd(&ctr[RJ_COLLISIONS], 1ull);
        return;
    }
    *dst = v.r;
    atomicAdd(&ctr[RJ_PLACED], 1ull);
}

}  // namespace

// fw_rejections_allgather_dev / _comm.  Collective; see include/flashweave_amd.h.
int fwi_rej_allgather(fw_ctx *c, const fw_dev_exchange *x, const char *who)
{
    if (!c->have_rej) return fw_fail(c, FW_ERR_STATE, "%s: no fw_learn_network has run with fw_set_track_rejections(1)", who);
    if (c->rej_gathered) return FW_OK;
    const int world = c->rej_world, rank = c->rej_rank;
    const size_t n_slots = c->rej_n_last;
    if (n_slots && (!c->have_level0 || (size_t)c->nb_off[c->P.p] != n_slots || c->d_rej.cap < n_slots * sizeof(fw_rejection)))
        return fw_fail(c, FW_ERR_STATE, "%s: level 0 ran again since the tracked fw_learn_network (its slots are gone)", who);
    (void)hipSetDevice(c->P.device);
    const int64_t n_local = (int64_t)c->rej.size();
    int64_t n_host = 0;
    for (uint8_t h : c->rej_host) n_host += h;
    if (n_local && !n_slots) return fw_fail(c, FW_ERR_STATE, "%s: %lld entries without slots", who, (long long)n_local);

    // counters [RJ_COUNTERS] | the ranks' counts [world] | the host-written records [n_host]
    const size_t hdr = sizeof(unsigned long long) * RJ_COUNTERS + sizeof(long long) * (size_t)world;
    if (int rc = fw_dev_reserve(c, c->d_rej_x, hdr + sizeof(FwRejRec) * (size_t)std::max<int64_t>(n_host, 1))) return rc;
    unsigned long long *d_ctr = (unsigned long long *)c->d_rej_x.ptr;
    long long *d_counts = (long long *)(d_ctr + RJ_COUNTERS);
    FwRejRec *d_stage = (FwRejRec *)((char *)c->d_rej_x.ptr + hdr);
    static_assert((sizeof(unsigned long long) * RJ_COUNTERS) % 8 == 0, "staging alignment");
    fw_rejection *d_slots = (fw_rejection *)c->d_rej.ptr;
    unsigned long long h_ctr[RJ_COUNTERS] = {0ull, 0ull, 0ull, 0ull};
    FW_HIP(c, hipMemsetAsync(d_ctr, 0, sizeof(h_ctr), c->stream));

    // 1. the job pool's records join the device slots (filled ones only; a device record keeps its slot)
    std::vector<FwRejRec> stage;
    if (n_host) {
        stage.reserve((size_t)n_host);
        for (size_t i = 0; i < c->rej.size(); ++i)
            if (c->rej_host[i]) stage.push_back(FwRejRec{c->rej[i], (long long)c->rej_slot[i]});
        const long long one = n_host;
        FW_HIP(c, hipMemcpyAsync(d_stage, stage.data(), sizeof(FwRejRec) * stage.size(), hipMemcpyHostToDevice, c->stream));
        FW_HIP(c, hipMemcpyAsync(d_counts, &one, sizeof(one), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(rej_place_kernel, dim3((unsigned)((n_host + 255) / 256), 1), dim3(256), 0, c->stream, (const FwRejRec *)d_stage, (long long)n_host, 1,
                           (const long long *)d_counts, -1, d_slots, (long long)n_slots, 0, d_ctr);
        FW_HIP(c, hipGetLastError());
        FW_HIP(c, hipMemcpyAsync(h_ctr, d_ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, c->stream));
        FW_HIP(c, hipStreamSynchronize(c->stream));  // (the staging vector and `one` may go)
        if (h_ctr[RJ_BAD_SLOTS] || (int64_t)h_ctr[RJ_PLACED] != n_host)
            return fw_fail(c, FW_ERR_DEVICE, "%s: %llu of %lld host-written records found their slot (%llu outside the %zu slots)", who, h_ctr[RJ_PLACED],
                           (long long)n_host, h_ctr[RJ_BAD_SLOTS], n_slots);
        std::fill(c->rej_host.begin(), c->rej_host.end(), (uint8_t)0);  // they are device records now (a failed exchange may be repeated)
    }
    c->rej_packed_host = n_host;
    c->rej_packed_dev = n_local - n_host;

    // 2. header: every rank's count; room for the largest
    std::vector<int64_t> counts((size_t)world, 0), aux((size_t)world, 0);
    void *d_send = nullptr, *d_recv = nullptr;
    int64_t cap = 0;
    int rc = x->prepare(x->user, n_local, (int64_t)n_slots, (int32_t)sizeof(FwRejRec), &d_send, &d_recv, counts.data(), aux.data(), &cap);
    if (rc) return fw_fail(c, FW_ERR_ARG, "%s: exchange.prepare failed (%d)", who, rc);
    if (n_local > cap || (!d_send && n_local) || !d_recv) return fw_fail(c, FW_ERR_ARG, "%s: exchange.prepare returned no room (cap %lld for %lld records)", who, (long long)cap, (long long)n_local);

    // 3. pack
    if (n_local) {
        hipLaunchKernelGGL(rej_pack_kernel, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, c->stream, (const fw_rejection *)d_slots, (long long)n_slots,
                           (FwRejRec *)d_send, (long long)n_local, d_ctr);
        FW_HIP(c, hipGetLastError());
        FW_HIP(c, hipMemcpyAsync(h_ctr, d_ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, c->stream));
    }
    FW_HIP(c, hipStreamSynchronize(c->stream));  // the caller's collective runs on its own stream
    const bool pack_ok = !n_local || (int64_t)h_ctr[RJ_CURSOR] == n_local;

    // 4. gather (also when this rank has a complaint: the other ranks are in the collective)
    rc = x->exchange(x->user);
    if (rc) return fw_fail(c, FW_ERR_ARG, "%s: exchange.exchange failed (%d)", who, rc);
    if (!pack_ok) return fw_fail(c, FW_ERR_DEVICE, "%s: %llu filled slots on the device, the log has %lld entries", who, h_ctr[RJ_CURSOR], (long long)n_local);
    int64_t total = 0;
    for (int r = 0; r < world; ++r) {
        if (counts[(size_t)r] < 0 || counts[(size_t)r] > cap) return fw_fail(c, FW_ERR_ARG, "%s: rank %d reports %lld records (cap %lld)", who, r, (long long)counts[(size_t)r], (long long)cap);
        if (counts[(size_t)r] && aux[(size_t)r] != (int64_t)n_slots)
            return fw_fail(c, FW_ERR_ARG, "%s: rank %d logged over %lld level-0 entries, this rank over %zu: the ranks did not run the same problem", who, r, (long long)aux[(size_t)r], n_slots);
        total += counts[(size_t)r];
    }
    if (rank < 0 || rank >= world || counts[(size_t)rank] != n_local) return fw_fail(c, FW_ERR_ARG, "%s: block %d of the gathered buffer is not this rank's (%lld records, %lld sent)", who, rank, rank >= 0 && rank < world ? (long long)counts[(size_t)rank] : -1ll, (long long)n_local);
    const int64_t foreign = total - n_local;

    // 5. the other ranks' records into this rank's slots, then the slot -> list pass
    if (foreign) {
        int64_t mx = 0;
        for (int r = 0; r < world; ++r)
            if (r != rank) mx = std::max(mx, counts[(size_t)r]);
        std::vector<long long> cl(counts.begin(), counts.end());
        FW_HIP(c, hipMemcpyAsync(d_counts, cl.data(), sizeof(long long) * (size_t)world, hipMemcpyHostToDevice, c->stream));
        FW_HIP(c, hipMemsetAsync(d_ctr, 0, sizeof(h_ctr), c->stream));
        hipLaunchKernelGGL(rej_place_kernel, dim3((unsigned)((mx + 255) / 256), (unsigned)world), dim3(256), 0, c->stream, (const FwRejRec *)d_recv, (long long)cap, world,
                           (const long long *)d_counts, rank, d_slots, (long long)n_slots, 1, d_ctr);
        FW_HIP(c, hipGetLastError());
        FW_HIP(c, hipMemcpyAsync(h_ctr, d_ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, c->stream));
        FW_HIP(c, hipStreamSynchronize(c->stream));
        if (h_ctr[RJ_COLLISIONS] || h_ctr[RJ_BAD_SLOTS] || (int64_t)h_ctr[RJ_PLACED] != foreign)
            return fw_fail(c, FW_ERR_DEVICE, "%s: %llu of %lld gathered records placed: %llu met a slot another rank or this one had filled (targets are dealt to one rank each), %llu name a slot outside 0 .. %zu",
                           who, h_ctr[RJ_PLACED], (long long)foreign, h_ctr[RJ_COLLISIONS], h_ctr[RJ_BAD_SLOTS], n_slots);
        if (int rc2 = fwi_rej_compact(c, n_slots, nullptr)) return rc2;
        if ((int64_t)c->rej.size() != total) return fw_fail(c, FW_ERR_DEVICE, "%s: %zu entries after the gather, the ranks announced %lld", who, c->rej.size(), (long long)total);
        for (size_t i = 0; i < c->rej.size(); ++i) {  // a record sits in its target's stretch of the slot array
            const fw_rejection &r = c->rej[i];
            if (r.target < 0 || r.target >= c->P.p || c->rej_slot[i] < c->nb_off[(size_t)r.target] || c->rej_slot[i] >= c->nb_off[(size_t)r.target + 1])
                return fw_fail(c, FW_ERR_DEVICE, "%s: the record of (%d, %d) arrived in slot %lld, outside its target's level-0 list", who, r.target, r.candidate, (long long)c->rej_slot[i]);
        }
    }
    c->rej_received = foreign;
    c->rej_gathered = true;
    return FW_OK;
}

extern "C" int fw_rejections_allgather_dev(fw_ctx *c, const fw_dev_exchange *x)
{
    if (!c) return fw_fail(nullptr, FW_ERR_ARG, "NULL context");
    if (!x || !x->prepare || !x->exchange) return fw_fail(c, FW_ERR_ARG, "fw_rejections_allgather_dev: NULL exchange (both callbacks are needed)");
    return fwi_rej_allgather(c, x, "fw_rejections_allgather_dev");
}

extern "C" int fw_rejections_allgather_stats(const fw_ctx *c, int64_t *packed_host, int64_t *packed_dev, int64_t *received)
{
    if (!c) return fw_fail(nullptr, FW_ERR_ARG, "NULL context");
    if (!c->rej_gathered) return fw_fail(c, FW_ERR_STATE, "fw_rejections_allgather_stats: no fw_rejections_allgather_* since the last fw_learn_network");
    if (packed_host) *packed_host = c->rej_packed_host;
    if (packed_dev) *packed_dev = c->rej_packed_dev;
    if (received) *received = c->rej_received;
    return FW_OK;
}

int fwi_l0_exchange_dev(fw_ctx *c, const fw_dev_exchange *x, int world, const FwL0Dev &local, int64_t m_local, FwL0Dev *merged,
                        int64_t *m_sum)
{
    std::vector<int64_t> counts((size_t)world, 0), aux((size_t)world, 0);
    void *d_send = nullptr, *d_recv = nullptr;
    int64_t cap = 0;
    int rc = x->prepare(x->user, (int64_t)local.k, m_local, (int32_t)sizeof(FwL0Rec), &d_send, &d_recv, counts.data(), aux.data(), &cap);
    if (rc) return fw_fail(c, FW_ERR_ARG, "fw_level0_sharded_dev: exchange.prepare failed (%d)", rc);
    if ((int64_t)local.k > cap || (!d_send && local.k) || !d_recv) return fw_fail(c, FW_ERR_ARG, "fw_level0_sharded_dev: exchange.prepare returned no room (cap %lld for %zu records)", (long long)cap, local.k);
    if (local.k) {
        hipLaunchKernelGGL(l0_pack_kernel, dim3((unsigned)((local.k + 255) / 256)), dim3(256), 0, c->stream, local.i, local.j, local.stat64,
                           local.pval, (long long)local.k, (FwL0Rec *)d_send);
        FW_HIP(c, hipGetLastError());
    }
    FW_HIP(c, hipStreamSynchronize(c->stream));  // the caller's collective runs on its own stream
    rc = x->exchange(x->user);
    if (rc) return fw_fail(c, FW_ERR_ARG, "fw_level0_sharded_dev: exchange.exchange failed (%d)", rc);
    std::vector<long long> off((size_t)world + 1, 0);
    int64_t msum = 0;
    for (int r = 0; r < world; ++r) {
        if (counts[r] < 0 || counts[r] > cap) return fw_fail(c, FW_ERR_ARG, "fw_level0_sharded_dev: rank %d reports %lld records (cap %lld)", r, (long long)counts[r], (long long)cap);
        off[r + 1] = off[r] + counts[r];
        msum += aux[r];
    }
    const size_t total = (size_t)off[world];
    if ((rc = fw_dev_reserve(c, c->d_l0m_i, (total + 1) * 2 * sizeof(int32_t)))) return rc;
    if ((rc = fw_dev_reserve(c, c->d_l0m_d, (total + 1) * 2 * sizeof(double) + ((size_t)world + 1) * sizeof(long long)))) return rc;
    int32_t *oi = (int32_t *)c->d_l0m_i.ptr, *oj = oi + total;
    double *os = (double *)c->d_l0m_d.ptr, *op = os + total;
    long long *d_off = (long long *)(op + total + 1);
    FW_HIP(c, hipMemcpyAsync(d_off, off.data(), sizeof(long long) * ((size_t)world + 1), hipMemcpyHostToDevice, c->stream));
    if (total) {
        hipLaunchKernelGGL(l0_unpack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, (const FwL0Rec *)d_recv, (long long)cap,
                           world, (const long long *)d_off, (long long)total, oi, oj, os, op);
        FW_HIP(c, hipGetLastError());
    }
    FW_HIP(c, hipStreamSynchronize(c->stream));
    *merged = FwL0Dev{};
    merged->i = oi;
    merged->j = oj;
    merged->stat64 = os;
    merged->pval = op;
    merged->k = total;
    *m_sum = msum;
    return FW_OK;
}
