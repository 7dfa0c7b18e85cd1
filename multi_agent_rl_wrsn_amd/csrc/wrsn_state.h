// wrsn_state.h -- gfx950 kernels that save, load and clone whole environments (wrsn_save_envs / wrsn_load_envs / wrsn_clone_envs).
//
// The state of environment e is plain per-environment slices of the handle's arrays (wrsn_types.h): WrsnEnvConst, the topology
// arrays, the `live` and `snap` WrsnNodeArrays with their WrsnEnvDyn and, for handles that keep generators, WrsnStochDev.  The host
// lists those slices once per handle in a segment table (base address, per-environment stride, bytes, offset in the record); the
// kernels below are one copy loop over that table.  A record is a 256-byte header followed by the segments at 16-byte aligned offsets,
// padded to a multiple of 256 bytes.
//
// Copy loop: a record is cut into 16-byte chunks and chunk g of the launch goes to thread g (grid-stride): consecutive lanes take
// consecutive chunks, so both the record and the environment slices are read and written in full 1 KB wave rows (dwordx4, guide
// Guideline 13).  Slices that are not 16-byte aligned per environment (nb_off / tc_off are NP + 1 / TP + 1 words, WrsnEnvDyn,
// prob_gp) are copied by the word.  Writes are ordinary vector stores.
#pragma once
#include <cstddef>
#include "wrsn_sim.h"

#define WRSN_REC_MAGIC 0x52534E57u       // "WNSR"
#define WRSN_REC_VERSION 1
#define WRSN_REC_HDR 256                 // header bytes at the start of every record
#define WRSN_REC_MAXSEG 64               // segments of a record (48 with the generator block)

// The header of a record.  The geometry fields decide whether a record fits a handle (wrsn_load_envs); the request fields hold the
// row's pending request at wrsn_save_envs.
struct WrsnRecHeader {
    uint32_t magic, version;
    int32_t ec_bytes, dyn_bytes;         // sizeof(WrsnEnvConst), sizeof(WrsnEnvDyn)
    int32_t NP, TP, ECAP, CCAP, M;
    int32_t n_node, n_target, conn_bound;
    int32_t has_gen, nseg;               // a generator block follows (mt_live/snap, es_live/snap, pgp); segments of the record
    int64_t rec_bytes;                   // bytes of the record (a multiple of 256)
    double prob_gp;                      // WrsnStochDev.pgp of the environment (1 without a generator block)
    int32_t agent_id, status;            // the pending request of the row (wrsn_step_out)
    double reward, now;
    int32_t terminal, pad0;
    uint8_t reserved[WRSN_REC_HDR - 104];
};
static_assert(sizeof(WrsnRecHeader) == WRSN_REC_HDR, "record header is 256 bytes");

// copy kinds of a segment
#define WRSN_SEG_V16 0                   // base, stride and bytes are multiples of 16: dwordx4 copies
#define WRSN_SEG_WORD 1                  // word copies
#define WRSN_SEG_DYN 2                   // the live WrsnEnvDyn: word copies, normalised on the destination (wrsn_rec_dyn_word)

struct WrsnSeg {
    uint64_t base;                       // device address of environment 0's slice
    int64_t stride;                      // bytes from one environment's slice to the next
    int32_t bytes;                       // bytes of one slice (a multiple of 4)
    int32_t c0;                          // first 16-byte chunk of the segment in the record
    int32_t kind, pad;
};
static_assert(sizeof(WrsnSeg) == 32, "segment table entry");

// copy directions of wrsn_rec_copy_kernel
#define WRSN_REC_PACK 0                  // environment slices -> records
#define WRSN_REC_UNPACK 1                // records -> environment slices
#define WRSN_REC_CLONE 2                 // environment slices -> environment slices

// What becomes of word `o` (byte offset) of a live WrsnEnvDyn written by a load or a clone: 0 copied, 1 the destination keeps its own
// (counters that run since create: n_steps, tot_ticks, tot_zero_steps, roll[]), 2 zeroed (map1_valid / map1_ptr: the observation row a
// map 1 was rendered into belongs to the source's row, a device address)
WDEV int wrsn_rec_dyn_word(int o) {
    const int ns = (int)offsetof(WrsnEnvDyn, n_steps), tt = (int)offsetof(WrsnEnvDyn, tot_ticks), tz = (int)offsetof(WrsnEnvDyn, tot_zero_steps);
    const int rl = (int)offsetof(WrsnEnvDyn, roll), mv = (int)offsetof(WrsnEnvDyn, map1_valid), mp = (int)offsetof(WrsnEnvDyn, map1_ptr);
    if ((o >= ns && o < ns + 8) || (o >= tt && o < tz + 8) || (o >= rl && o < rl + (int)sizeof(double) * (WRSN_MAX_MC + 3))) return 1;
    if ((o >= mv && o < mv + 4) || (o >= mp && o < mp + 8)) return 2;
    return 0;
}

#ifndef WRSN_LD_U4_DEFINED
WDEV void wrsn_st_u4(WrsnU4 WRSN_GLOBAL_AS* p, const WrsnU4& v) {
    typedef uint32_t v4_ __attribute__((ext_vector_type(4)));
    v4_ t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
    *(v4_ WRSN_GLOBAL_AS*)p = t;
}
#else
inline void wrsn_st_u4(WrsnU4* p, const WrsnU4& v) { *p = v; }
#endif

// One chunk of the copy loop, shared by wrsn_rec_copy_kernel and wrsn_pool_copy_kernel: 16-byte chunk c of the record layout for pair r
// (source environment src_env[r] for pack and clone, destination environment dst_env[r] for unpack and clone); rp is the address of
// the chunk in the pair's record (pack, unpack; NULL for a clone).  `tab` is the segment table in LDS.
WDEV void wrsn_rec_copy_chunk(const WrsnSeg* tab, int nseg, int mode, const int32_t* __restrict__ src_env, const int32_t* __restrict__ dst_env,
                              int r, int c, uint8_t* rp) {
    int lo = 0, hi = nseg - 1;                                  // the last segment that starts at or before chunk c
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tab[mid].c0 <= c) lo = mid; else hi = mid - 1; }
    const WrsnSeg sg = tab[lo];
    const int o = (c - sg.c0) * 16;                             // byte offset in the slice
    if (o >= sg.bytes) {                                        // alignment padding of the record
        if (mode == WRSN_REC_PACK) { WrsnU4 z; z.x = z.y = z.z = z.w = 0u; wrsn_st_u4(wrsn_global((WrsnU4*)rp), z); }
        return;
    }
    const uint8_t* sp = mode == WRSN_REC_UNPACK ? rp : (const uint8_t*)(uintptr_t)(sg.base + (uint64_t)src_env[r] * (uint64_t)sg.stride + (uint64_t)o);
    uint8_t* dp = mode == WRSN_REC_PACK ? rp : (uint8_t*)(uintptr_t)(sg.base + (uint64_t)dst_env[r] * (uint64_t)sg.stride + (uint64_t)o);
    if (sg.kind == WRSN_SEG_V16 || mode == WRSN_REC_UNPACK) {
        const WrsnU4 v = wrsn_ld_u4(wrsn_global((const WrsnU4*)sp));   // (the record side is always 16-byte aligned)
        if (sg.kind == WRSN_SEG_V16) { wrsn_st_u4(wrsn_global((WrsnU4*)dp), v); return; }
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
        uint32_t WRSN_GLOBAL_AS* d32 = wrsn_global((uint32_t*)dp);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ok = o + 4 * k;
            if (ok >= sg.bytes) break;
            const int rule = sg.kind == WRSN_SEG_DYN ? wrsn_rec_dyn_word(ok) : 0;
            if (rule != 1) d32[k] = rule == 2 ? 0u : w4[k];
        }
        return;
    }
    // a word-copied slice read from an environment (pack, clone)
    const uint32_t WRSN_GLOBAL_AS* s32 = wrsn_global((const uint32_t*)sp);
    uint32_t w4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w4[k] = (o + 4 * k < sg.bytes) ? s32[k] : 0u;
    if (mode == WRSN_REC_PACK) {
        WrsnU4 v; v.x = w4[0]; v.y = w4[1]; v.z = w4[2]; v.w = w4[3];
        wrsn_st_u4(wrsn_global((WrsnU4*)dp), v);
        return;
    }
    uint32_t WRSN_GLOBAL_AS* d32 = wrsn_global((uint32_t*)dp);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ok = o + 4 * k;
        if (ok >= sg.bytes) break;
        const int rule = sg.kind == WRSN_SEG_DYN ? wrsn_rec_dyn_word(ok) : 0;
        if (rule != 1) d32[k] = rule == 2 ? 0u : w4[k];
    }
}

// the segment table of the handle into LDS (every thread of the 256-thread block calls this)
WDEV void wrsn_rec_load_table(WrsnSeg* tab, const WrsnSeg* __restrict__ segs, int nseg) {
    const uint64_t* g = (const uint64_t*)segs; uint64_t* l = (uint64_t*)tab;
    for (int w = threadIdx.x; w < nseg * 4; w += 256) l[w] = g[w];
    __syncthreads();
}

// One copy loop for the three directions.  Pair i (record i0 + i of the call) copies chunks [WRSN_REC_HDR / 16, chunks) of the record
// layout: source environment src_env[i0 + i] (pack, clone), destination environment dst_env[i0 + i] (unpack, clone), record
// rec + (i0 + i) * rec_stride (pack, unpack).  Launch: 256 threads, LDS nseg * 32 bytes (the segment table).
__global__ void __launch_bounds__(256) wrsn_rec_copy_kernel(const WrsnSeg* __restrict__ segs, int nseg, int mode, const int32_t* __restrict__ src_env,
                                                            const int32_t* __restrict__ dst_env, uint8_t* __restrict__ rec, long long rec_stride,
                                                            int i0, int n, int chunks) {
    extern __shared__ double smem[];
    WrsnSeg* tab = (WrsnSeg*)smem;
    wrsn_rec_load_table(tab, segs, nseg);
    const int hc = WRSN_REC_HDR / 16, per = chunks - hc;      // chunks of one pair
    const int total = n * per, step = (int)gridDim.x * 256;
    for (int g = (int)blockIdx.x * 256 + (int)threadIdx.x; g < total; g += step) {
        const int i = g / per, c = g - i * per + hc, r = i0 + i;
        uint8_t* rp = rec ? rec + (size_t)r * (size_t)rec_stride + (size_t)c * 16 : nullptr;
        wrsn_rec_copy_chunk(tab, nseg, mode, src_env, dst_env, r, c, rp);
    }
}

// wrsn_save_envs: the header of record i -- the handle's template (geometry) plus what belongs to environment env[i]: its sizes and
// conn_bound, prob_gp and the row's pending request.  One thread per record.
__global__ void __launch_bounds__(256) wrsn_rec_header_kernel(WrsnDev d, const double* __restrict__ pgp, WrsnRecHeader tmpl, const int32_t* __restrict__ env,
                                                              int n, uint8_t* __restrict__ rec, long long rec_stride, WrsnStepOutDev req) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const int e = env[i];
    WrsnRecHeader* hd = (WrsnRecHeader*)(rec + (size_t)i * (size_t)rec_stride);
    *hd = tmpl;
    const WrsnEnvConst* ec = d.ec + e;
    hd->n_node = ec->n_node; hd->n_target = ec->n_target; hd->conn_bound = ec->conn_bound;
    hd->prob_gp = pgp ? pgp[e] : 1.0;
    hd->agent_id = req.agent_id[e]; hd->status = req.status[e]; hd->reward = req.reward[e]; hd->now = req.now[e]; hd->terminal = req.terminal[e];
}

// wrsn_load_envs: the headers of n records (stride rec_stride) side by side in hdr[n], for the host to validate.  One thread per record.
__global__ void __launch_bounds__(256) wrsn_rec_gather_kernel(const uint8_t* __restrict__ rec, long long rec_stride, int n, uint8_t* __restrict__ hdr) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const WrsnU4* s = (const WrsnU4*)(rec + (size_t)i * (size_t)rec_stride);
    WrsnU4* o = (WrsnU4*)(hdr + (size_t)i * WRSN_REC_HDR);
    for (int k = 0; k < WRSN_REC_HDR / 16; ++k) wrsn_st_u4(wrsn_global(o + k), wrsn_ld_u4(wrsn_global(s + k)));
}

// The request rows of the environments a load, a clone or a pool reset replaced: from header i of `hdr` (load: the gathered headers,
// hdr_stride = WRSN_REC_HDR, rec_idx NULL; pool reset: the pool itself, header rec_idx[i] at hdr_stride = record bytes) or from row
// src_env[i] of `out` (clone) into row dst_env[i]; NULL fields of `out` are skipped.  n_dev, when set, holds the number of rows in
// device memory (n is then the launch's upper bound).  status_as < 0: the saved status, else that value.  row_state = row_st
// (0: a following wrsn_rollout_collect appends nothing for the row; 2: it discards what was pending, as after a reset); rend[dst] = the
// request's charger for the observation pass (rows not named keep -1).  pool_cur, when set (load, clone): the pool record the
// destination runs, -1 after a load, the source's after a clone.  One thread per row.
__global__ void __launch_bounds__(256) wrsn_rec_rows_kernel(WrsnDev d, const uint8_t* __restrict__ hdr, long long hdr_stride, const int32_t* __restrict__ rec_idx,
                                                            const int32_t* __restrict__ src_env, const int32_t* __restrict__ dst_env, int n,
                                                            const int32_t* __restrict__ n_dev, WrsnStepOutDev out, int32_t* __restrict__ rend,
                                                            int status_as, int row_st, int32_t* __restrict__ pool_cur) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n || (n_dev && i >= *n_dev)) return;
    const int e = dst_env[i];
    int aid = -1, st = 0, term = 0; double rw = 0.0, nw = 0.0;
    if (hdr) {
        const WrsnRecHeader* hd = (const WrsnRecHeader*)(hdr + (size_t)(rec_idx ? rec_idx[i] : i) * (size_t)hdr_stride);
        aid = hd->agent_id; st = hd->status; term = hd->terminal; rw = hd->reward; nw = hd->now;
        if (pool_cur) pool_cur[e] = -1;
    } else {
        const int s = src_env[i];
        if (out.agent_id) aid = out.agent_id[s];
        if (out.status) st = out.status[s];
        if (out.terminal) term = out.terminal[s];
        if (out.reward) rw = out.reward[s];
        if (out.now) nw = out.now[s];
        if (pool_cur) pool_cur[e] = pool_cur[s];
    }
    if (status_as >= 0) st = status_as;
    if (out.agent_id) out.agent_id[e] = aid;
    if (out.status) out.status[e] = st;
    if (out.terminal) out.terminal[e] = (uint8_t)term;
    if (out.reward) out.reward[e] = rw;
    if (out.now) out.now[e] = nw;
    d.row_state[e] = row_st;
    if (rend) rend[e] = aid;
}

// ------------------------------------------------------------------ scenario pools (wrsn_pool_set / wrsn_pool_reset)
// A pool is P records back to back in caller-owned device memory.  wrsn_pool_reset replaces the environments the DEVICE selects by pool
// records the DEVICE selects, with no host round trip: wrsn_pool_select_kernel compacts the (environment, record) pairs,
// wrsn_pool_copy_kernel is the unpack direction of the copy loop above over that list, wrsn_rec_rows_kernel writes the request rows.

#define WRSN_POOL_BAD_INDEX (-5)         // per-row status of a selected row whose pool_index is outside [0, P) (WRSN_STATUS_POOL_INDEX)
#define WRSN_POOL_STRIPS 8               // 64-row strips whose loads one pass of the select kernel keeps in flight

// The record environment e takes at its k-th swap since wrsn_pool_set(seed): splitmix64 of the (environment, swap) counter, the high 32
// bits scaled to [0, P).  multi_agent_rl_wrsn_amd.pool_draw is the same function on the host.
WDEV int wrsn_pool_draw(uint64_t seed, int e, uint32_t k, int P) {
    uint64_t z = (seed ^ (((uint64_t)(uint32_t)e << 32) | (uint64_t)k)) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (int)(((z >> 32) * (uint64_t)(uint32_t)P) >> 32);
}

// Select and compact: ONE wave.  Row e is selected by mask[e] != 0, or with mask == NULL by live.dyn[e].terminal_pending (the rows an
// auto-reset would take); its record is pool_index[e], or with pool_index == NULL the draw.  The selected rows with a record in [0, P)
// become the pair list (pair_env[i], pair_rec[i]), i < *count, in ascending environment order: the wave walks the rows in 64-row
// strips, a ballot of the strip and the popcount of the lanes below give every lane its place, so the order is a pure function of the
// inputs.  The loads of WRSN_POOL_STRIPS strips are issued before the first ballot.  For every pair: agent_id[e] = -2 (when given: the
// caller's next wrsn_step leaves the row alone), cur[e] = record, swaps[e] += 1.  A selected row with a bad index gets status
// WRSN_POOL_BAD_INDEX and nothing else.  rend (when given) is preset to -1 for every row.  Launch: 1 block of 64 threads.
__global__ void __launch_bounds__(64) wrsn_pool_select_kernel(WrsnDev d, const uint8_t* __restrict__ mask, const int32_t* __restrict__ pool_index, int P,
                                                              uint64_t seed, int32_t* __restrict__ agent_id, int32_t* __restrict__ cur,
                                                              int32_t* __restrict__ swaps, int32_t* __restrict__ pair_env, int32_t* __restrict__ pair_rec,
                                                              int32_t* __restrict__ count, int32_t* __restrict__ status, int32_t* __restrict__ rend) {
    const int lane = (int)threadIdx.x, B = d.B;
    const unsigned long long below = (1ull << lane) - 1ull;
    int base = 0;
    for (int e0 = 0; e0 < B; e0 += 64 * WRSN_POOL_STRIPS) {
        int sel[WRSN_POOL_STRIPS];
#pragma unroll
        for (int s = 0; s < WRSN_POOL_STRIPS; ++s) {
            const int e = e0 + 64 * s + lane;
            sel[s] = e < B ? (mask ? (int)mask[e] : d.live.dyn[e].terminal_pending) : 0;
        }
#pragma unroll
        for (int s = 0; s < WRSN_POOL_STRIPS; ++s) {
            const int e = e0 + 64 * s + lane;
            if (e0 + 64 * s >= B) break;                       // (wave-uniform)
            int rec = -1, k = 0, ok = 0;
            if (sel[s] != 0) {
                k = swaps[e];
                rec = pool_index ? pool_index[e] : wrsn_pool_draw(seed, e, (uint32_t)k, P);
                ok = rec >= 0 && rec < P;
                if (!ok && status) status[e] = WRSN_POOL_BAD_INDEX;
            }
            if (rend && e < B) rend[e] = -1;
            const unsigned long long m = __ballot(ok);
            if (ok) {
                const int pos = base + __popcll(m & below);
                pair_env[pos] = e; pair_rec[pos] = rec;
                cur[e] = rec; swaps[e] = k + 1;
                if (agent_id) agent_id[e] = -2;
            }
            base += __popcll(m);
        }
    }
    if (lane == 0) *count = base;
}

// The unpack direction of the copy loop over a pair list whose length is in device memory: pair i replaces environment dst_env[i] by
// record rec_idx[i] of the pool (pool + rec_idx[i] * rec_stride).  The grid is fixed by the host (it does not know the length) and
// grid-stride; with no pair every block leaves at once.  Launch: 256 threads, LDS nseg * 32 bytes.
__global__ void __launch_bounds__(256) wrsn_pool_copy_kernel(const WrsnSeg* __restrict__ segs, int nseg, const int32_t* __restrict__ dst_env,
                                                             const int32_t* __restrict__ rec_idx, const int32_t* __restrict__ n_dev,
                                                             const uint8_t* __restrict__ pool, long long rec_stride, int chunks) {
    extern __shared__ double smem[];
    const int n = *n_dev;
    if (n <= 0) return;                                         // (uniform over the grid)
    WrsnSeg* tab = (WrsnSeg*)smem;
    wrsn_rec_load_table(tab, segs, nseg);
    const int hc = WRSN_REC_HDR / 16, per = chunks - hc;      // chunks of one pair
    const long long total = (long long)n * per;
    if (total < (1ll << 31)) {                                  // 32-bit chunk indices, as in wrsn_rec_copy_kernel
        const unsigned tot = (unsigned)total, step = gridDim.x * 256u;
        for (unsigned g = blockIdx.x * 256u + threadIdx.x; g < tot; g += step) {
            const int i = (int)(g / (unsigned)per), c = (int)(g - (unsigned)i * (unsigned)per) + hc;
            uint8_t* rp = (uint8_t*)pool + (size_t)rec_idx[i] * (size_t)rec_stride + (size_t)c * 16;
            wrsn_rec_copy_chunk(tab, nseg, WRSN_REC_UNPACK, nullptr, dst_env, i, c, rp);
        }
    } else {
        const long long step = (long long)gridDim.x * 256;
        for (long long g = (long long)blockIdx.x * 256 + (long long)threadIdx.x; g < total; g += step) {
            const int i = (int)(g / per), c = (int)(g - (long long)i * per) + hc;
            uint8_t* rp = (uint8_t*)pool + (size_t)rec_idx[i] * (size_t)rec_stride + (size_t)c * 16;
            wrsn_rec_copy_chunk(tab, nseg, WRSN_REC_UNPACK, nullptr, dst_env, i, c, rp);
        }
    }
}
