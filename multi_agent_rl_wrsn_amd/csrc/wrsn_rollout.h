// wrsn_rollout.h -- device-side roll-out bookkeeping of the asynchronous-agent batch (gfx950).
//
// Restates, for B environments at once, what the reference's trainer does per environment with Python lists
// (controller/ippo/IPPO.py:119-156, the same in controller/ppo/PPO.py:115-152):
//   * when charger a of an environment is given an action, the trainer remembers the observation it acted on, the raw
//     policy output (`input_action`: a 3-vector, or the G x G density map) and its log-probability (IPPO.py:141-142;
//     WRSN.step keeps prev_state / input_action per agent, WRSN.py:292,303);
//   * when a later WRSN.step returns that charger (not terminal), one transition (prev_state, input_action, log-prob,
//     reward, state) is appended to the charger's lists (IPPO.py:150-155); a charger returned before it ever acted in
//     the episode is skipped (IPPO.py:146-147: the first transition of every agent is dropped);
//   * a terminal return ends the episode: what the chargers had pending is discarded (IPPO.py:144-145).
// Stored terminals are therefore all False and cal_rt_adv's bootstrap term vanishes (IPPO.py:80-81): returns == rewards.
//
// Two kernels, both pure data movement (HBM-bound; 16-byte accesses).  Observation rows (pend_state, state, next_state, obs) are
// copied in the element size of the handle's observation format (`obs_es`: 4 = float32, 2 = bf16 bit patterns):
//   wrsn_tr_record_kernel   pending[env][agent] <- (observation row, action row, log-prob)       one block per environment
//   wrsn_tr_collect_kernel  transition[agent][slot] <- (pending state/action/log-prob, reward, observation row)
//
// Below them, wrsn_entity_kernel: the ENTITY observation (wrsn_set_entity_out / wrsn_entities), the per-node, per-charger and
// per-environment terms get_state(agent) is made of (WRSN.py:130-186) as float32 rows instead of the 4 x G x G image.
//
// At the end, wrsn_tr_record_entities_kernel / wrsn_tr_collect_entities_kernel: the two bookkeeping kernels again for stored states
// that are packed entity rows (6.6 KB instead of 160 KB): a wave per row, four rows per block.
#pragma once
#include <stdint.h>
#include "wrsn_state.h"

struct WrsnTrBuffers {                    // mirrors wrsn_transition_buffers of include/wrsn_hip.h (device pointers)
    int32_t capacity, action_elems;
    float* pend_state; float* pend_action; float* pend_logp; uint8_t* pend_valid;
    float* state; float* action; float* next_state; float* reward; float* logp; double* now; int32_t* env; int32_t* count;
};

template <typename T>
__device__ __forceinline__ void wrsn_tr_copy(T* __restrict__ dst, const T* __restrict__ src, int n, int tid, int nthreads) {
    // rows are 16-byte aligned whenever n is a multiple of 4 floats (G*G and 4*G*G with even G; 3-vectors take the tail loop) or of
    // 8 bf16 (4*G*G with even G)
    constexpr int per = 16 / (int)sizeof(T);                  // elements of a 16-byte access
    const int n4 = ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0) ? (n / per) : 0;
    const float4* s4 = (const float4*)src; float4* d4 = (float4*)dst;
    for (int i = tid; i < n4; i += nthreads) d4[i] = s4[i];
    for (int i = per * n4 + tid; i < n; i += nthreads) dst[i] = src[i];
}
// row `row` (S elements of obs_es bytes) of src -> row `drow` of dst
__device__ __forceinline__ void wrsn_tr_copy_obs(float* dst, size_t drow, const float* src, size_t srow, int S, int obs_es, int tid) {
    if (obs_es == 2) wrsn_tr_copy((uint16_t*)dst + drow * S, (const uint16_t*)src + srow * S, S, tid, 256);
    else wrsn_tr_copy(dst + drow * S, src + srow * S, S, tid, 256);
}

__global__ void __launch_bounds__(256) wrsn_tr_record_kernel(int B, int M, int G, WrsnTrBuffers t, const int32_t* __restrict__ agent_id,
                                                             const float* __restrict__ action, const float* __restrict__ logp,
                                                             const float* __restrict__ obs, int obs_es) {
    const int e = blockIdx.x;
    if (e >= B) return;
    const int a = agent_id[e];
    if (a < 0 || a >= M) return;
    const int S = 4 * G * G, A = t.action_elems;
    const size_t slot = (size_t)e * M + a;
    wrsn_tr_copy_obs(t.pend_state, slot, obs, (size_t)e, S, obs_es, threadIdx.x);
    wrsn_tr_copy(t.pend_action + slot * A, action + (size_t)e * A, A, threadIdx.x, 256);
    if (threadIdx.x == 0) { t.pend_logp[slot] = logp[e]; t.pend_valid[slot] = 1; }
}

__global__ void __launch_bounds__(256) wrsn_tr_collect_kernel(int B, int M, int G, WrsnTrBuffers t, const int32_t* __restrict__ agent_id,
                                                              const double* __restrict__ reward, const double* __restrict__ now,
                                                              int32_t* __restrict__ row_state, const float* __restrict__ obs, int obs_es) {
    extern __shared__ double smem[];                          // one int: the slot the block's transition goes to
    int* s_slot = (int*)smem;
    const int e = blockIdx.x;
    if (e >= B) return;
    // what the last environment launch did with this row (WrsnDev.row_state): only a row whose WRSN.step completed in that launch
    // carries a fresh request; rows left untouched (agent -2 / masked out) or still in flight (step budget) are skipped
    const int st = row_state[e];
    if (st == 0 || st == 3) return;
    __syncthreads();
    if (threadIdx.x == 0) row_state[e] = 0;                   // consumed: a second call after the same launch finds nothing
    if (st == 2 || st == 4) {                                 // episode over (terminal return) or restarted ((auto-)reset): pending actions are discarded
        if ((int)threadIdx.x < M) t.pend_valid[(size_t)e * M + threadIdx.x] = 0;
        return;
    }
    const int a = agent_id[e];
    if (a < 0 || a >= M) return;
    const size_t pslot = (size_t)e * M + a;
    if (!t.pend_valid[pslot]) return;                         // this charger has not acted yet in this episode (IPPO.py:146-147)
    if (threadIdx.x == 0) *s_slot = atomicAdd(&t.count[a], 1);
    __syncthreads();
    const int slot = *s_slot;
    if (slot >= t.capacity) return;                           // buffer full: counted, not stored
    const int S = 4 * G * G, A = t.action_elems;
    const size_t q = (size_t)a * t.capacity + slot;
    wrsn_tr_copy_obs(t.state, q, t.pend_state, pslot, S, obs_es, threadIdx.x);
    wrsn_tr_copy_obs(t.next_state, q, obs, (size_t)e, S, obs_es, threadIdx.x);
    wrsn_tr_copy(t.action + q * A, t.pend_action + pslot * A, A, threadIdx.x, 256);
    if (threadIdx.x == 0) { t.reward[q] = (float)reward[e]; t.logp[q] = t.pend_logp[pslot]; t.now[q] = now[e]; t.env[q] = e; }
}

// ------------------------------------------------------------------ entity observation (wrsn_set_entity_out / wrsn_entities)
// get_state(agent) rasterises a small set of numbers: one weighted Gaussian per live node (map 1) and at most M rank-1 terms built from the
// chargers (maps 2..4).  This kernel writes those numbers themselves, float32, for the rows the render pass of a call draws:
//   node [B][N][8]   u, v (position in the frame), w_n (the map-1 weight, WRSN.py:146), (E - thr) / (cap - thr), CS / (alpha/beta^2),
//                    RR / (alpha/beta^2), level, 1; a dead node keeps u, v and has 0 elsewhere; rows beyond the environment's own
//                    n_node are all zero (N = the handle's node count: the row stride);
//   mc   [B][M][12]  loc (frame), energy / capacity, is the asking charger, status != 0, charging, cur_phy_action x, y (frame),
//                    cur_phy_action[2] / charging_time_max, the map-4 amplitude with the reference's mixed index (WRSN.py:184;
//                    0 for the asking charger), 0, 0;
//   env  [B][8]      hX, hY (bandwidths of maps 1, 3, 4), the two bandwidths of map 2, asking charger, n_node, 0, 0.
// Every value is a float64 expression of the fields wrsn_obs_body reads, rounded once at the store.  A gather with no reduction and no
// LDS: one 256-thread block per row (block b takes row_map[map0 + b], or b), nodes in id order, K nodes per thread (K * 256 >= N), the
// loads of all K issued -- with clamped indices, not predicates -- before the first use; a node row leaves as two 16-byte stores, a
// charger row as three from one thread, the environment row as two.  It reads no map1_ptr / map1_valid and writes nothing but its rows.
struct WrsnEntityOut { float* node; float* mc; float* env; };   // mirrors wrsn_entity_out of include/wrsn_hip.h (device pointers)
#define WRSN_ENT_NODE_F 8
#define WRSN_ENT_MC_F 12
#define WRSN_ENT_ENV_F 8

WDEV void wrsn_ent_store4(float* p, float a, float b, float c, float e) {
    WrsnU4 v;
    v.x = (uint32_t)__float_as_int(a); v.y = (uint32_t)__float_as_int(b); v.z = (uint32_t)__float_as_int(c); v.w = (uint32_t)__float_as_int(e);
    wrsn_st_u4(wrsn_global((WrsnU4*)p), v);
}

template <int K>
__global__ void __launch_bounds__(256) wrsn_entity_kernel(WrsnDev d, const int32_t* __restrict__ agent_id, WrsnEntityOut out,
                                                          const int32_t* __restrict__ row_map, int map0) {
    const int tid = (int)threadIdx.x;
    const int env = __builtin_amdgcn_readfirstlane(row_map ? row_map[map0 + (int)blockIdx.x] : (int)blockIdx.x);
    if (env < 0 || env >= d.B) return;
    const int aid = __builtin_amdgcn_readfirstlane(agent_id[env]);
    if (aid < 0 || aid >= d.M) return;
    const int NP = d.NP, NR = d.N, M = d.M;                    // NR: node rows of an output row (the handle's node count <= NP)
    const size_t nb = (size_t)env * NP;
    // ---- every load of the K nodes of this thread, then the constants: one memory round trip
    const auto gls = wrsn_global(d.live.ls + nb);
    const auto gx = wrsn_global(d.node_x + nb), gy = wrsn_global(d.node_y + nb);
    const auto gE = wrsn_global(d.live.E + nb), gCS = wrsn_global(d.live.CS + nb), gRR = wrsn_global(d.live.RR + nb);
    int lsw[K]; double px[K], py[K], en[K], cs[K], rr[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int n = tid + 256 * k, src = n < NR ? n : NR - 1;   // clamped: rows beyond NR are not stored
        lsw[k] = gls[src]; px[k] = gx[src]; py[k] = gy[src]; en[k] = gE[src]; cs[k] = gCS[src]; rr[k] = gRR[src];
    }
    const WrsnEnvConst WRSN_GLOBAL_AS* ec = wrsn_global((const WrsnEnvConst*)(d.ec + env));
    const int N = ec->n_node;
    const double fx0 = ec->frame[0], fy0 = ec->frame[2];
    const double W = ec->frame[1] - fx0, H = ec->frame[3] - fy0;
    const double invW = 1.0 / W, invH = 1.0 / H;
    const double a_b2 = ec->alpha / (ec->beta * ec->beta), thr = ec->threshold, span = ec->capacity - ec->threshold;
    const double inv_ab2 = 1.0 / a_b2, inv_span = 1.0 / span;
    float* orow = out.node + (size_t)env * NR * WRSN_ENT_NODE_F;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int n = tid + 256 * k;
        if (n >= NR) break;
        // selects, not branches: nothing the loads above could be sunk into (a dead node's quotient is computed and dropped)
        const bool in = n < N, live = in && (lsw[k] & 1);
        const double de = en[k] - thr;
        float f[8];
        f[0] = in ? (float)((px[k] - fx0) * invW) : 0.f; f[1] = in ? (float)((py[k] - fy0) * invH) : 0.f;
        f[2] = live ? (float)((cs[k] * span) / (a_b2 * de)) : 0.f;   // the weight as wrsn_obs_body forms it: one division
        f[3] = live ? (float)(de * inv_span) : 0.f;
        f[4] = live ? (float)(cs[k] * inv_ab2) : 0.f; f[5] = live ? (float)(rr[k] * inv_ab2) : 0.f;
        f[6] = live ? (float)((lsw[k] >> 1) - 1) : 0.f; f[7] = live ? 1.f : 0.f;
        wrsn_ent_store4(orow + (size_t)n * WRSN_ENT_NODE_F, f[0], f[1], f[2], f[3]);
        wrsn_ent_store4(orow + (size_t)n * WRSN_ENT_NODE_F + 4, f[4], f[5], f[6], f[7]);
    }
    // ---- the chargers: thread o writes charger o; thread M the environment row
    if (tid < M) {
        const WrsnAgent WRSN_GLOBAL_AS* ag = wrsn_global((const WrsnAgent*)d.live.dyn[env].ag);
        const int o = tid;
        const double lx = ag[o].loc[0], ly = ag[o].loc[1], eo = ag[o].energy, c0 = ag[o].cur[0], c1 = ag[o].cur[1], c2 = ag[o].cur[2];
        const double ay = ag[aid].cur[1];
        const int st = ag[o].status, ch = ag[o].type_charging;
        const double amp = o == aid ? 0.0 : (dist2(lx, ly, c0, ay) / ec->velocity) / ec->moving_time_max;   // mixed index as in WRSN.py:184
        float* q = out.mc + ((size_t)env * M + o) * WRSN_ENT_MC_F;
        wrsn_ent_store4(q, (float)((lx - fx0) * invW), (float)((ly - fy0) * invH), (float)(eo / ec->mc_capacity), o == aid ? 1.f : 0.f);
        wrsn_ent_store4(q + 4, st != 0 ? 1.f : 0.f, ch != 0 ? 1.f : 0.f, (float)((c0 - fx0) * invW), (float)((c1 - fy0) * invH));
        wrsn_ent_store4(q + 8, (float)(c2 / ec->charging_time_max), (float)amp, 0.f, 0.f);
    } else if (tid == M) {
        const double tmp = H < W ? H : W;
        float* q = out.env + (size_t)env * WRSN_ENT_ENV_F;
        wrsn_ent_store4(q, (float)(ec->charging_range * invW), (float)(ec->charging_range * invH), (float)(0.5 * tmp * invW), (float)(0.5 * tmp * invH));
        wrsn_ent_store4(q + 4, (float)aid, (float)N, 0.f, 0.f);
    }
}

// ------------------------------------------------------------------ entity transition rows (wrsn_rollout_record_entities / wrsn_rollout_collect_entities)
// The bookkeeping of wrsn_tr_record_kernel / wrsn_tr_collect_kernel above, statement for statement, for a stored state that is the entity
// observation instead of the image: one packed float32 row of R = 8 N + 12 M + 8 elements -- node [N][8], then mc [M][12], then env [8], as
// wrsn_entity_out lays them out -- in pend_state [B, M, R], state and next_state [M, capacity, R] of the same WrsnTrBuffers.  Every part is
// a multiple of 16 bytes, so a row is C = 2 N + 3 M + 2 chunks of 16 bytes and every part boundary is a chunk boundary.
// A row is 6.6 KB at 200 x 3 (32 KB at 1 000 x 8), not 160 KB: ONE 64-LANE WAVE PER ROW, WRSN_ENT_ROWS rows per 256-thread block, no LDS
// and no __syncthreads.  Consecutive lanes take consecutive chunks through the wrsn_global casts; a pass is up to eight chunks per lane
// (8 KB per wave) whose loads are all issued -- with clamped indices, not predicates -- before its first store.  The slot claim is one
// atomicAdd of lane 0, broadcast with wrsn_wave_first (v_readfirstlane); a wave whose row has nothing to do leaves at its first test.
#define WRSN_ENT_ROWS 4                                       // rows (waves) per block
#define WRSN_ENT_PASS 8                                       // 16-byte chunks per lane and pass

// where chunk c of a packed row comes from: [0, cn) at `a`, [cn, cm) at `b`, the rest at `c` (cn == cm == the row's chunks: one plain row at `a`)
struct WrsnEntRowSrc { const WrsnU4* a; const WrsnU4* b; const WrsnU4* c; int cn, cm; };

WDEV WrsnEntRowSrc wrsn_ent_row_gather(const WrsnEntityOut& ent, int e, int N, int M) {
    WrsnEntRowSrc s;
    s.a = (const WrsnU4*)(ent.node + (size_t)e * N * WRSN_ENT_NODE_F);
    s.b = (const WrsnU4*)(ent.mc + (size_t)e * M * WRSN_ENT_MC_F);
    s.c = (const WrsnU4*)(ent.env + (size_t)e * WRSN_ENT_ENV_F);
    s.cn = 2 * N; s.cm = 2 * N + 3 * M;
    return s;
}
WDEV WrsnEntRowSrc wrsn_ent_row_plain(const float* row, int C) {
    WrsnEntRowSrc s; s.a = s.b = s.c = (const WrsnU4*)row; s.cn = s.cm = C; return s;
}

// the C chunks of one row, by the 64 lanes of a wave.  The three parts are addressed from one base: chunk c lies at a + 16 c, plus the
// wave-uniform distance of its part from where the row would go on behind `a` -- two selects per chunk, no branch between the loads.
WDEV void wrsn_ent_row_copy(float* dst, const WrsnEntRowSrc& s, int C, int lane) {
    const auto d = wrsn_global((WrsnU4*)dst);
    const uintptr_t a = (uintptr_t)s.a;
    const int64_t db = (int64_t)((uintptr_t)s.b - a) - 16ll * s.cn, dc = (int64_t)((uintptr_t)s.c - a) - 16ll * s.cm;
    for (int c0 = 0; c0 < C; c0 += 64 * WRSN_ENT_PASS) {
        WrsnU4 v[WRSN_ENT_PASS];
#pragma unroll
        for (int k = 0; k < WRSN_ENT_PASS; ++k) {
            const int i = c0 + 64 * k + lane, c = i < C ? i : C - 1;   // clamped: chunks beyond C are not stored
            const int64_t off = 16ll * c + (c < s.cn ? 0ll : c < s.cm ? db : dc);
            v[k] = wrsn_ld_u4(wrsn_global((const WrsnU4*)(a + (uintptr_t)off)));
        }
#pragma unroll
        for (int k = 0; k < WRSN_ENT_PASS; ++k) {
            const int i = c0 + 64 * k + lane;
            if (i < C) wrsn_st_u4(d + i, v[k]);
        }
    }
}

__global__ void __launch_bounds__(64 * WRSN_ENT_ROWS) wrsn_tr_record_entities_kernel(int B, int M, int N, WrsnTrBuffers t, const int32_t* __restrict__ agent_id,
                                                                                      const float* __restrict__ action, const float* __restrict__ logp,
                                                                                      WrsnEntityOut ent) {
    const int lane = (int)threadIdx.x & 63;
    const int e = (int)blockIdx.x * WRSN_ENT_ROWS + ((int)threadIdx.x >> 6);
    if (e >= B) return;
    const int a = wrsn_wave_first(agent_id[e]);
    if (a < 0 || a >= M) return;
    const int C = 2 * N + 3 * M + 2, A = t.action_elems;
    const size_t slot = (size_t)e * M + a;
    wrsn_ent_row_copy(t.pend_state + slot * C * 4, wrsn_ent_row_gather(ent, e, N, M), C, lane);
#pragma clang loop vectorize(disable) interleave(disable)
    for (int i = lane; i < A; i += 64) t.pend_action[slot * A + i] = action[(size_t)e * A + i];
    if (lane == 0) { t.pend_logp[slot] = logp[e]; t.pend_valid[slot] = 1; }
}

__global__ void __launch_bounds__(64 * WRSN_ENT_ROWS) wrsn_tr_collect_entities_kernel(int B, int M, int N, WrsnTrBuffers t, const int32_t* __restrict__ agent_id,
                                                                                       const double* __restrict__ reward, const double* __restrict__ now,
                                                                                       int32_t* row_state, WrsnEntityOut ent, int consume) {
    const int lane = (int)threadIdx.x & 63;
    const int e = (int)blockIdx.x * WRSN_ENT_ROWS + ((int)threadIdx.x >> 6);
    if (e >= B) return;
    const int st = wrsn_wave_first(row_state[e]);             // the row_state rules of wrsn_tr_collect_kernel; every lane has read before lane 0 writes
    if (st == 0 || st == 3) return;
    if (consume && lane == 0) row_state[e] = 0;               // consume == 0: left for the image collect that follows
    if (st == 2 || st == 4) {                                 // episode over or restarted: pending actions are discarded
        if (lane < M) t.pend_valid[(size_t)e * M + lane] = 0;
        return;
    }
    const int a = wrsn_wave_first(agent_id[e]);
    if (a < 0 || a >= M) return;
    const size_t pslot = (size_t)e * M + a;
    if (!wrsn_wave_first((int)t.pend_valid[pslot])) return;   // this charger has not acted yet in this episode (IPPO.py:146-147)
    int slot = 0;
    if (lane == 0) slot = atomicAdd(&t.count[a], 1);
    slot = wrsn_wave_first(slot);
    if (slot >= t.capacity) return;                           // buffer full: counted, not stored
    const int C = 2 * N + 3 * M + 2, A = t.action_elems;
    const size_t q = (size_t)a * t.capacity + slot;
    wrsn_ent_row_copy(t.state + q * C * 4, wrsn_ent_row_plain(t.pend_state + pslot * C * 4, C), C, lane);
    wrsn_ent_row_copy(t.next_state + q * C * 4, wrsn_ent_row_gather(ent, e, N, M), C, lane);
#pragma clang loop vectorize(disable) interleave(disable)
    for (int i = lane; i < A; i += 64) t.action[q * A + i] = t.pend_action[pslot * A + i];
    if (lane == 0) { t.reward[q] = (float)reward[e]; t.logp[q] = t.pend_logp[pslot]; t.now[q] = now[e]; t.env[q] = e; }
}

// ------------------------------------------------------------------ entity policy: acting from entity rows (wrsn_entity_act)
// The actor of build_entity_networks (ippo.py) evaluated on the device, one packed float32 block per charger (layout: include/wrsn_hip.h;
// every Linear stored [in, out], its bias behind it).  Three launches on the handle's stream:
//   wrsn_entpol_group_kernel   row lists per charger: one ballot per charger and wave, one atomicAdd per wave into M counters
//   wrsn_entpol_trunk_kernel   one 256-thread block per row: node MLP on the matrix cores, the pools, the charger MLP -> feat[e][200]
//   wrsn_entpol_head_kernel    one block per (charger, tile of <= 32 of its rows): head1, head2 on the matrix cores, the six 128-long
//                              dot products, the clamp, the sample and the log-probability
// All matrix products are v_mfma_f32_32x32x2_f32 in the TRANSPOSED orientation: D[unit i][column j] = sum_k W[k][i] X[k][j], units in D's
// rows, nodes (trunk) or batch rows (head) in D's columns.  The A operand of k-pair kk is W[2 kk + (l >> 5)][32 t + (l & 31)]: two runs of
// 32 consecutive floats of the [in, out] block.  An accumulator register r of a finished layer holds, for column l & 31, unit
// u(r) = (r & 3) + 8 (r >> 2) in lanes 0..31 and unit u(r) + 4 in lanes 32..63: that IS a B operand for the k-pair (u, u + 4), so the node
// MLP's second layer takes the first layer's 32 registers as they are, in a fixed permutation of k, with no trip through LDS.
// What a row's outputs depend on: its own entity rows, its charger's block, its eps.  Every sum has a fixed order that nothing outside
// the row enters: a column's MFMA chain is k-ordered whatever the column; a wave folds the 32 columns of a tile by a fixed butterfly and
// adds its tiles in tile order; the four waves are added in wave order; the six final dot products are four chains over k mod 4 each.
// The order of the row lists may differ from run to run; the column a row lands in changes no bit of it.
// Registers: the pools are folded tile by tile, so a lane carries two sums and two maxima, not 64 values: 91 VGPRs + 32 AGPRs, no scratch,
// four waves per SIMD (profiles/entity_act_kernel_resource_usage.csv).
#define WRSN_ENTPOL_FEAT 200
// The packed block (include/wrsn_hip.h): per layer the weights [in][out], then the bias [out], layer after layer
#define WRSN_EP_NODE1 0                                                            // node1    8 ->  64
#define WRSN_EP_NODE1_B (WRSN_EP_NODE1 + WRSN_ENT_NODE_F * 64)
#define WRSN_EP_NODE2 (WRSN_EP_NODE1_B + 64)                                       // node2   64 ->  64
#define WRSN_EP_NODE2_B (WRSN_EP_NODE2 + 64 * 64)
#define WRSN_EP_MC1 (WRSN_EP_NODE2_B + 64)                                         // mc1     12 ->  32
#define WRSN_EP_MC1_B (WRSN_EP_MC1 + WRSN_ENT_MC_F * 32)
#define WRSN_EP_MC2 (WRSN_EP_MC1_B + 32)                                           // mc2     32 ->  32
#define WRSN_EP_MC2_B (WRSN_EP_MC2 + 32 * 32)
#define WRSN_EP_HEAD1 (WRSN_EP_MC2_B + 32)                                         // head1  200 -> 128
#define WRSN_EP_HEAD1_B (WRSN_EP_HEAD1 + WRSN_ENTPOL_FEAT * 128)
#define WRSN_EP_HEAD2 (WRSN_EP_HEAD1_B + 128)                                      // head2  128 -> 128
#define WRSN_EP_HEAD2_B (WRSN_EP_HEAD2 + 128 * 128)
#define WRSN_EP_MEAN (WRSN_EP_HEAD2_B + 128)                                       // mean   128 ->   3
#define WRSN_EP_MEAN_B (WRSN_EP_MEAN + 128 * 3)
#define WRSN_EP_LSTD (WRSN_EP_MEAN_B + 3)                                          // log_std 128 -> 3
#define WRSN_EP_LSTD_B (WRSN_EP_LSTD + 128 * 3)
#define WRSN_EP_FLOATS ((WRSN_EP_LSTD_B + 3 + 3) / 4 * 4)                          // rounded up to a multiple of 4
static_assert(WRSN_ENTPOL_FEAT == 64 + 64 + 32 + 32 + WRSN_ENT_ENV_F, "head1 reads both node pools, both charger pools and the env row");
static_assert(WRSN_EP_HEAD1 == 6208 && WRSN_EP_MEAN == 48448 && WRSN_EP_FLOATS == 49224, "the layout documented in include/wrsn_hip.h");
static_assert(WRSN_EP_MC1 % 4 == 0, "the trunk stages the first WRSN_EP_MC1 floats in LDS by 16-byte loads");
// LDS of the trunk block, in floats: node1 / node2 with their biases (the first WRSN_EP_MC1 floats of the block), the pools of the four
// waves, their live-node counts, the two charger layers
#define WRSN_EP_T_SUM WRSN_EP_MC1
#define WRSN_EP_T_MAX (WRSN_EP_T_SUM + 256)
#define WRSN_EP_T_CNT (WRSN_EP_T_MAX + 256)
#define WRSN_EP_T_G1 (WRSN_EP_T_CNT + 4)
#define WRSN_EP_T_G2 (WRSN_EP_T_G1 + 256)
#define WRSN_EP_T_LDS ((WRSN_EP_T_G2 + 256) * 4)              // bytes
// LDS of the head block, in floats: the feature tile [32][201] (later the second layer's output [128][32]), the first layer's output
// [128][32] (later the six dot products [6][32])
#define WRSN_EP_H_LD 201
#define WRSN_EP_H_Z (32 * WRSN_EP_H_LD)
#define WRSN_EP_H_LDS ((WRSN_EP_H_Z + 128 * 32) * 4)          // bytes
#define WRSN_EP_HEAD_ROWS 32                                  // rows (columns of the product) per head block

struct WrsnEntActOut { float* action; double* action_f64; float* logp; float* mean; float* log_std; };   // mirrors wrsn_entity_act_out

WDEV int wrsn_ep_unit(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }   // row of D that register r holds in lane half h

// v[r] of the 32 lanes of a half wave folded into the lanes with (l & 15) == r (of each half): sum or max over the 32 columns in a fixed
// butterfly -- four halving steps (8 + 4 + 2 + 1 exchanges) and one plain exchange, not 80
template <bool MAX>
WDEV float wrsn_ep_fold16(float (&v)[16], int lane) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int m = 8 >> s;                                 // lane distance and half the number of values left
        const bool up = (lane & m) != 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (r < m) {
                const float a = v[r], b = v[r + m];
                const float got = __shfl_xor(up ? a : b, m);
                const float keep = up ? b : a;
                v[r] = MAX ? fmaxf(keep, got) : keep + got;
            }
        }
    }
    const float o = __shfl_xor(v[0], 16);
    return MAX ? fmaxf(v[0], o) : v[0] + o;
}

__global__ void __launch_bounds__(64) wrsn_entpol_group_kernel(int B, int M, const int32_t* __restrict__ agent_id, int32_t* __restrict__ list,
                                                               int32_t* cnt) {
    const int lane = (int)threadIdx.x, e = (int)blockIdx.x * 64 + lane;
    const int a = e < B ? agent_id[e] : -1;
    for (int c = 0; c < M; ++c) {
        const unsigned long long m = __ballot(a == c);
        if (m == 0ull) continue;                              // wave-uniform
        int base = 0;
        if (lane == 0) base = atomicAdd(&cnt[c], __popcll(m));
        base = wrsn_wave_first(base);
        if (a == c) list[(size_t)c * B + base + __popcll(m & ((1ull << lane) - 1ull))] = e;
    }
}

__global__ void __launch_bounds__(256) wrsn_entpol_trunk_kernel(int B, int M, int N, const float* __restrict__ actors,
                                                                const int32_t* __restrict__ agent_id, WrsnEntityOut ent, float* __restrict__ feat,
                                                                int stride) {   // floats from one charger's block to the next: the trunk leads every actor block
    extern __shared__ double smem[];
    float* sW = (float*)smem;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    const int e = (int)blockIdx.x;
    if (e >= B) return;
    const int aid = wrsn_wave_first(agent_id[e]);
    if (aid < 0 || aid >= M) return;
    const float* blk = actors + (size_t)aid * stride;
    {   // node1, node2 and their biases: 1 184 chunks of 16 bytes
        const auto src = wrsn_global((const WrsnU4*)blk);
        WrsnU4* dst = (WrsnU4*)sW;
        for (int i = tid; i < WRSN_EP_MC1 / 4; i += 256) dst[i] = wrsn_ld_u4(src + i);
    }
    __syncthreads();
    float psum[2] = {0.f, 0.f}, pmax[2] = {0.f, 0.f}, cnt = 0.f;   // lane (r, h) of a wave: units 32 t2 + u(r) + 4 h, r = lane & 15
    const float* nrow = ent.node + (size_t)e * N * WRSN_ENT_NODE_F;
    const int ntile = (N + 31) >> 5;
    for (int tile = wave; tile < ((ntile + 3) & ~3); tile += 4) {   // every wave the same number of rounds: the folds below are exchanges
        const bool on = tile < ntile;                          // wave-uniform; a round without a tile folds zeros
        const int n = tile * 32 + col, srcn = n < N ? n : N - 1;   // clamped: a column beyond N is computed on zeros and pooled nowhere
        const auto p = wrsn_global((const WrsnU4*)(nrow + (size_t)srcn * WRSN_ENT_NODE_F));
        const WrsnU4 c0 = wrsn_ld_u4(p), c1 = wrsn_ld_u4(p + 1);
        const bool alive = n < N && __int_as_float((int)c1.w) == 1.f;
        float x[4];                                           // features 2 kk + h of the column, zeros unless the node is alive (a select)
        x[0] = __int_as_float((int)(h ? c0.y : c0.x)); x[1] = __int_as_float((int)(h ? c0.w : c0.z));
        x[2] = __int_as_float((int)(h ? c1.y : c1.x)); x[3] = __int_as_float((int)(h ? c1.w : c1.z));
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) x[kk] = alive ? x[kk] : 0.f;
        wrsn_v16f h1[2];
        if (on) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                wrsn_v16f acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = sW[WRSN_EP_NODE1_B + 32 * t + wrsn_ep_unit(r, h)];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sW[WRSN_EP_NODE1 + (2 * kk + h) * 64 + 32 * t + col], x[kk], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) h1[t][r] = fmaxf(acc[r], 0.f);
            }
        }
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
            float v[16], w[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = 0.f;
            if (on) {
                wrsn_v16f acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = sW[WRSN_EP_NODE2_B + 32 * t2 + wrsn_ep_unit(r, h)];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)              // register r of h1[t]: the k-pair (u, u + 4), u = 32 t + (r & 3) + 8 (r >> 2)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sW[WRSN_EP_NODE2 + (32 * t + wrsn_ep_unit(r, h)) * 64 + 32 * t2 + col], h1[t][r], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] = alive ? fmaxf(acc[r], 0.f) : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) w[r] = v[r];
            psum[t2] += wrsn_ep_fold16<false>(v, lane);        // the tile's 32 columns, then the wave's tiles in tile order
            pmax[t2] = fmaxf(pmax[t2], wrsn_ep_fold16<true>(w, lane));
        }
        cnt += (on && alive) ? 1.f : 0.f;
    }
    // ---- the four waves: through LDS, added in wave order below
    cnt += __shfl_xor(cnt, 1); cnt += __shfl_xor(cnt, 2); cnt += __shfl_xor(cnt, 4); cnt += __shfl_xor(cnt, 8); cnt += __shfl_xor(cnt, 16);
    if ((lane & 16) == 0) {
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
            const int unit = 32 * t2 + wrsn_ep_unit(lane & 15, h);
            sW[WRSN_EP_T_SUM + 64 * wave + unit] = psum[t2]; sW[WRSN_EP_T_MAX + 64 * wave + unit] = pmax[t2];
        }
        if (lane == 0) sW[WRSN_EP_T_CNT + wave] = cnt;
    }
    // ---- the charger MLP on the VALU: thread (c, o) = unit o of charger c
    const float* mrow = ent.mc + (size_t)e * M * WRSN_ENT_MC_F;
    const int c = tid >> 5, o = tid & 31;
    if (c < M) {
        float s = blk[WRSN_EP_MC1_B + o];
#pragma unroll
        for (int k = 0; k < WRSN_ENT_MC_F; ++k) s = fmaf(mrow[c * WRSN_ENT_MC_F + k], blk[WRSN_EP_MC1 + k * 32 + o], s);
        sW[WRSN_EP_T_G1 + tid] = fmaxf(s, 0.f);
    }
    __syncthreads();
    if (c < M) {
        float s = blk[WRSN_EP_MC2_B + o];
#pragma unroll 8
        for (int k = 0; k < 32; ++k) s = fmaf(sW[WRSN_EP_T_G1 + 32 * c + k], blk[WRSN_EP_MC2 + k * 32 + o], s);
        sW[WRSN_EP_T_G2 + tid] = fmaxf(s, 0.f);
    }
    __syncthreads();
    float* frow = feat + (size_t)e * WRSN_ENTPOL_FEAT;
    if (tid < 64) {
        const float n_alive = ((sW[WRSN_EP_T_CNT] + sW[WRSN_EP_T_CNT + 1]) + sW[WRSN_EP_T_CNT + 2]) + sW[WRSN_EP_T_CNT + 3];
        const float sum = ((sW[WRSN_EP_T_SUM + tid] + sW[WRSN_EP_T_SUM + 64 + tid]) + sW[WRSN_EP_T_SUM + 128 + tid]) + sW[WRSN_EP_T_SUM + 192 + tid];
        const float mx = fmaxf(fmaxf(sW[WRSN_EP_T_MAX + tid], sW[WRSN_EP_T_MAX + 64 + tid]), fmaxf(sW[WRSN_EP_T_MAX + 128 + tid], sW[WRSN_EP_T_MAX + 192 + tid]));
        frow[tid] = sum / fmaxf(n_alive, 1.f);
        frow[64 + tid] = mx;                                  // ReLU outputs pooled from 0: zeros when no node is alive
    } else if (tid < 96) {
        const int u = tid - 64;
        float sa = 0.f, so = 0.f, na = 0.f;
        for (int k = 0; k < M; ++k) {
            const float g = sW[WRSN_EP_T_G2 + 32 * k + u];
            const bool al = mrow[k * WRSN_ENT_MC_F + 4] == 1.f, self = mrow[k * WRSN_ENT_MC_F + 3] == 1.f;   // ENT_MC["alive"], ENT_MC["is_self"]
            sa += al ? g : 0.f; na += al ? 1.f : 0.f; so += self ? g : 0.f;
        }
        frow[128 + u] = sa / fmaxf(na, 1.f);
        frow[160 + u] = so;
    } else if (tid < 104) {
        const int k = tid - 96;
        const float v = ent.env[(size_t)e * WRSN_ENT_ENV_F + k];
        frow[192 + k] = k == 4 ? v * (1.f / (float)M) : k == 5 ? v * (1.f / (float)(N > 1 ? N : 1)) : v;   // ENT_ENV["agent"] / M, ENT_ENV["n_node"] / N
    }
}

// The front of a head block, shared by wrsn_entpol_head_kernel and wrsn_entptr_head_kernel: which (charger, tile of <= 32 of its rows) the
// block is -- the tiles of charger 0, then of charger 1, ... --, then head1 and head2 of the block at `actors + a * stride` on that tile.
// false (block-uniform): more blocks than tiles.  On return sF holds ReLU(head2(ReLU(head1(features)))) as [128 units][32 columns];
// a column beyond `rows` repeats the last row.  Ends in a __syncthreads.
WDEV bool wrsn_ep_head_front(int B, int M, int stride, const float* __restrict__ actors, const float* __restrict__ feat,
                             const int32_t* __restrict__ list, const int32_t* __restrict__ cnt, float* sF, float* sZ, int& rows,
                             const int32_t*& mine, const float*& blk) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    int b = (int)blockIdx.x, a = -1, first = 0;
    rows = 0;
    for (int c = 0; c < M; ++c) {
        int k = cnt[c]; k = k < 0 ? 0 : (k > B ? B : k);
        const int nt = (k + WRSN_EP_HEAD_ROWS - 1) / WRSN_EP_HEAD_ROWS;
        if (a < 0) {
            if (b < nt) { a = c; first = WRSN_EP_HEAD_ROWS * b; rows = k - first < WRSN_EP_HEAD_ROWS ? k - first : WRSN_EP_HEAD_ROWS; }
            else b -= nt;
        }
    }
    if (a < 0) return false;
    mine = list + (size_t)a * B + first;
    blk = actors + (size_t)a * stride;
    for (int i = tid; i < WRSN_EP_HEAD_ROWS * WRSN_ENTPOL_FEAT; i += 256) {   // a column beyond `rows` repeats the last row: computed, not stored
        const int j = i / WRSN_ENTPOL_FEAT, k = i - j * WRSN_ENTPOL_FEAT;
        const int row = mine[j < rows ? j : rows - 1];
        sF[j * WRSN_EP_H_LD + k] = feat[(size_t)row * WRSN_ENTPOL_FEAT + k];
    }
    __syncthreads();
    {   // head1: wave w holds units 32 w .. 32 w + 31 of all 32 columns
        wrsn_v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = blk[WRSN_EP_HEAD1_B + 32 * wave + wrsn_ep_unit(r, h)];
        const float* wa = blk + WRSN_EP_HEAD1 + h * 128 + 32 * wave + col;
        const float* xb = sF + col * WRSN_EP_H_LD + h;
#pragma unroll 10
        for (int kk = 0; kk < WRSN_ENTPOL_FEAT / 2; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kk * 256], xb[2 * kk], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) sZ[(32 * wave + wrsn_ep_unit(r, h)) * 32 + col] = fmaxf(acc[r], 0.f);
    }
    __syncthreads();
    {   // head2
        wrsn_v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = blk[WRSN_EP_HEAD2_B + 32 * wave + wrsn_ep_unit(r, h)];
        const float* wa = blk + WRSN_EP_HEAD2 + h * 128 + 32 * wave + col;
        const float* xb = sZ + h * 32 + col;
#pragma unroll 8
        for (int kk = 0; kk < 64; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kk * 256], xb[kk * 64], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) sF[(32 * wave + wrsn_ep_unit(r, h)) * 32 + col] = fmaxf(acc[r], 0.f);   // the feature tile is dead
    }
    __syncthreads();
    return true;
}

__global__ void __launch_bounds__(256) wrsn_entpol_head_kernel(int B, int M, const float* __restrict__ actors, const float* __restrict__ feat,
                                                               const int32_t* __restrict__ list, const int32_t* __restrict__ cnt,
                                                               const float* __restrict__ eps, WrsnEntActOut out) {
    extern __shared__ double smem[];
    float* sF = (float*)smem;
    float* sZ = sF + WRSN_EP_H_Z;
    const int tid = (int)threadIdx.x;
    int rows; const int32_t* mine; const float* blk;
    if (!wrsn_ep_head_front(B, M, WRSN_EP_FLOATS, actors, feat, list, cnt, sF, sZ, rows, mine, blk)) return;   // block-uniform
    if (tid < 192) {                                          // six dot products per column: thread (d, j); four k-ordered chains over k mod 4, the
        const int j = tid & 31, d = tid >> 5;                 // bias in the first, added as (0 + 1) + (2 + 3): a quarter of the chain length
        const float* w = blk + (d < 3 ? WRSN_EP_MEAN + d : WRSN_EP_LSTD + d - 3);
        float s0 = d < 3 ? blk[WRSN_EP_MEAN_B + d] : blk[WRSN_EP_LSTD_B + d - 3], s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 4
        for (int k = 0; k < 128; k += 4) {
            s0 = fmaf(sF[k * 32 + j], w[3 * k], s0); s1 = fmaf(sF[(k + 1) * 32 + j], w[3 * k + 3], s1);
            s2 = fmaf(sF[(k + 2) * 32 + j], w[3 * k + 6], s2); s3 = fmaf(sF[(k + 3) * 32 + j], w[3 * k + 9], s3);
        }
        sZ[d * 32 + j] = (s0 + s1) + (s2 + s3);               // head1's output is dead
    }
    __syncthreads();
    if (tid < rows) {
        const int e = mine[tid];
        float lp = 0.f;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float mu = sZ[d * 32 + tid];
            const float ls = fminf(fmaxf(sZ[(3 + d) * 32 + tid], -4.f), 1.f);
            const float ep = eps ? eps[(size_t)e * 3 + d] : 0.f;
            const float x = fmaf(expf(ls), ep, mu);
            lp += -0.5f * ep * ep - ls;
            out.action[(size_t)e * 3 + d] = x;
            if (out.action_f64) out.action_f64[(size_t)e * 3 + d] = (double)x;
            if (out.mean) out.mean[(size_t)e * 3 + d] = mu;
            if (out.log_std) out.log_std[(size_t)e * 3 + d] = ls;
        }
        out.logp[e] = lp - 2.7568156f;                        // 1.5 log(2 pi)
    }
}

// ------------------------------------------------------------------ heuristic baseline on the entity rows (wrsn_entity_heuristic_act)
// "The most critical node nobody else is serving" (include/wrsn_hip.h has the rule, statement for statement): a wave per row,
// WRSN_ENT_ROWS rows per block like the entity bookkeeping kernels, no LDS and no __syncthreads.  The chargers (at most eight) are read
// by every lane with wave-uniform addresses; lane l takes nodes l, l + 64, ... as two 16-byte loads each, with clamped indices, and
// keeps two candidates -- the best alive node, the best alive node that is not claimed -- as (score, index) pairs under `>`, so the
// lowest index of a lane wins a tie.  Both candidates are then reduced by every wave, whether or not the fallback is needed (no
// wave-divergent reduction): the maximum of the score, then the minimum of the index among the lanes that hold the maximum.  Maximum
// and minimum are exact, so the order of the reduction does not enter the result; it is a __shfl_xor butterfly, not the DPP chain of
// wrsn_sim.h, because the emulator of tests/emu models DPP rows for one-wave blocks only and this block holds four waves.
// float32 throughout, contraction off where a product feeds a sum.
#define WRSN_EH_NONE 0x7fffffff                               // index of "no candidate"

WDEV bool wrsn_eh_claims(float u, float v, float cx, float cy, float hx, float hy) {
#pragma clang fp contract(off)
    const float dx = (u - cx) / hx, dy = (v - cy) / hy;
    const float a = dx * dx, b = dy * dy;
    return a + b <= 1.f;                                      // a NaN compares false
}
WDEV float wrsn_eh_charge(float charge_scale, float level) {
#pragma clang fp contract(off)
    const float r = 1.f - level;
    const float t = charge_scale * r;
    return t > 0.f ? (t < 1.f ? t : 1.f) : 0.f;               // selects: a NaN gives 0
}
// (score, index) of the wave's best candidate in every lane: lanes without a candidate hold (-inf, WRSN_EH_NONE)
WDEV int wrsn_eh_wave_best(float s, int i) {
    float m = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const float o = __shfl_xor(m, d); m = o > m ? o : m; }
    int k = (s == m) ? i : WRSN_EH_NONE;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_xor(k, d); k = o < k ? o : k; }
    return k;
}

__global__ void __launch_bounds__(64 * WRSN_ENT_ROWS) wrsn_entity_heuristic_kernel(int B, int M, int N, const int32_t* __restrict__ agent_id, WrsnEntityOut ent,
                                                                                    float charge_scale, float* __restrict__ action,
                                                                                    double* __restrict__ action_f64) {
    const int lane = (int)threadIdx.x & 63;
    const int e = (int)blockIdx.x * WRSN_ENT_ROWS + ((int)threadIdx.x >> 6);
    if (e >= B) return;
    const int a = wrsn_wave_first(agent_id[e]);
    if (a < 0 || a >= M) return;
    const float* mc = ent.mc + (size_t)e * M * WRSN_ENT_MC_F;
    const float hx = ent.env[(size_t)e * WRSN_ENT_ENV_F], hy = ent.env[(size_t)e * WRSN_ENT_ENV_F + 1];
    int self = a;
    for (int o = M - 1; o >= 0; --o) if (mc[o * WRSN_ENT_MC_F + 3] == 1.f) self = o;
    float cx[WRSN_MAX_MC], cy[WRSN_MAX_MC]; bool on[WRSN_MAX_MC];
#pragma unroll
    for (int o = 0; o < WRSN_MAX_MC; ++o) {
        const int c = o < M ? o : M - 1;                      // clamped: chargers beyond M are switched off
        on[o] = o < M && o != self && mc[c * WRSN_ENT_MC_F + 4] == 1.f;
        cx[o] = mc[c * WRSN_ENT_MC_F + 6]; cy[o] = mc[c * WRSN_ENT_MC_F + 7];
    }
    const auto node = wrsn_global((const WrsnU4*)(ent.node + (size_t)e * N * WRSN_ENT_NODE_F));
    const float ninf = -__builtin_inff();
    float sA = ninf, sU = ninf; int iA = WRSN_EH_NONE, iU = WRSN_EH_NONE;
    for (int n0 = 0; n0 < N; n0 += 64) {
        const int n = n0 + lane, c = n < N ? n : N - 1;       // clamped: nodes beyond N are no candidates
        const WrsnU4 p = wrsn_ld_u4(node + 2 * c), q = wrsn_ld_u4(node + 2 * c + 1);
        const float u = __int_as_float((int)p.x), v = __int_as_float((int)p.y), w = __int_as_float((int)p.z);
        const bool alive = n < N && __int_as_float((int)q.w) == 1.f;
        bool claimed = false;
#pragma unroll
        for (int o = 0; o < WRSN_MAX_MC; ++o) claimed = claimed || (on[o] && wrsn_eh_claims(u, v, cx[o], cy[o], hx, hy));
        const float s = w > ninf ? w : ninf;                  // a NaN never beats a number
        if (alive && (iA == WRSN_EH_NONE || s > sA)) { sA = s; iA = n; }
        if (alive && !claimed && (iU == WRSN_EH_NONE || s > sU)) { sU = s; iU = n; }
    }
    const int bU = wrsn_eh_wave_best(sU, iU), bA = wrsn_eh_wave_best(sA, iA);
    const int n = bU != WRSN_EH_NONE ? bU : bA;
    if (lane != 0) return;
    float x, y, t;
    if (n != WRSN_EH_NONE) {
        const float* r = ent.node + ((size_t)e * N + n) * WRSN_ENT_NODE_F;
        x = r[0]; y = r[1]; t = wrsn_eh_charge(charge_scale, r[3]);
    } else { x = mc[self * WRSN_ENT_MC_F]; y = mc[self * WRSN_ENT_MC_F + 1]; t = 0.f; }
    float* o = action + (size_t)e * 3;
    o[0] = x; o[1] = y; o[2] = t;
    if (action_f64) { double* d = action_f64 + (size_t)e * 3; d[0] = (double)x; d[1] = (double)y; d[2] = (double)t; }
}

// ------------------------------------------------------------------ the heuristic's decision as a pointer label (wrsn_entity_heuristic_label)
// The pick of wrsn_entity_heuristic_kernel -- the same loop over the same helpers, so the node is that kernel's node -- kept as the
// node-pointer policy stores a decision: ((float) node, x), x being the pre-sigmoid charge for which the pointer's
// min_charge + (1 - min_charge) sigmoid(x) is the heuristic's charging time c, up to the clamp to [-x_clip, x_clip].  A wave per row,
// no LDS, no __syncthreads; the action, when asked for, is the heuristic's own (u_n, v_n, c).
WDEV float wrsn_eh_label_x(float c, float min_charge, float x_clip) {
#pragma clang fp contract(off)
    const float cm = c > min_charge ? c : min_charge;
    const float num = cm - min_charge, den = 1.f - min_charge;
    float u = num / den;
    const float ex = expf(x_clip);
    const float u_lo = 1.f / (1.f + ex), u_hi = 1.f - u_lo;
    u = u < u_lo ? u_lo : (u > u_hi ? u_hi : u);
    const float om = 1.f - u;
    return logf(u / om);
}

__global__ void __launch_bounds__(64 * WRSN_ENT_ROWS) wrsn_entity_heuristic_label_kernel(int B, int M, int N, const int32_t* __restrict__ agent_id, WrsnEntityOut ent,
                                                                                          float charge_scale, float min_charge, float x_clip,
                                                                                          float* __restrict__ stored, float* __restrict__ action,
                                                                                          double* __restrict__ action_f64) {
    const int lane = (int)threadIdx.x & 63;
    const int e = (int)blockIdx.x * WRSN_ENT_ROWS + ((int)threadIdx.x >> 6);
    if (e >= B) return;
    const int a = wrsn_wave_first(agent_id[e]);
    if (a < 0 || a >= M) return;
    const float* mc = ent.mc + (size_t)e * M * WRSN_ENT_MC_F;
    const float hx = ent.env[(size_t)e * WRSN_ENT_ENV_F], hy = ent.env[(size_t)e * WRSN_ENT_ENV_F + 1];
    int self = a;
    for (int o = M - 1; o >= 0; --o) if (mc[o * WRSN_ENT_MC_F + 3] == 1.f) self = o;
    float cx[WRSN_MAX_MC], cy[WRSN_MAX_MC]; bool on[WRSN_MAX_MC];
#pragma unroll
    for (int o = 0; o < WRSN_MAX_MC; ++o) {
        const int c = o < M ? o : M - 1;                      // clamped: chargers beyond M are switched off
        on[o] = o < M && o != self && mc[c * WRSN_ENT_MC_F + 4] == 1.f;
        cx[o] = mc[c * WRSN_ENT_MC_F + 6]; cy[o] = mc[c * WRSN_ENT_MC_F + 7];
    }
    const auto node = wrsn_global((const WrsnU4*)(ent.node + (size_t)e * N * WRSN_ENT_NODE_F));
    const float ninf = -__builtin_inff();
    float sA = ninf, sU = ninf; int iA = WRSN_EH_NONE, iU = WRSN_EH_NONE;
    for (int n0 = 0; n0 < N; n0 += 64) {
        const int n = n0 + lane, c = n < N ? n : N - 1;       // clamped: nodes beyond N are no candidates
        const WrsnU4 p = wrsn_ld_u4(node + 2 * c), q = wrsn_ld_u4(node + 2 * c + 1);
        const float u = __int_as_float((int)p.x), v = __int_as_float((int)p.y), w = __int_as_float((int)p.z);
        const bool alive = n < N && __int_as_float((int)q.w) == 1.f;
        bool claimed = false;
#pragma unroll
        for (int o = 0; o < WRSN_MAX_MC; ++o) claimed = claimed || (on[o] && wrsn_eh_claims(u, v, cx[o], cy[o], hx, hy));
        const float s = w > ninf ? w : ninf;                  // a NaN never beats a number
        if (alive && (iA == WRSN_EH_NONE || s > sA)) { sA = s; iA = n; }
        if (alive && !claimed && (iU == WRSN_EH_NONE || s > sU)) { sU = s; iU = n; }
    }
    const int bU = wrsn_eh_wave_best(sU, iU), bA = wrsn_eh_wave_best(sA, iA);
    const int n = bU != WRSN_EH_NONE ? bU : bA;
    if (lane != 0) return;
    float x, y, t, kf, xs;
    if (n != WRSN_EH_NONE) {
        const float* r = ent.node + ((size_t)e * N + n) * WRSN_ENT_NODE_F;
        x = r[0]; y = r[1]; t = wrsn_eh_charge(charge_scale, r[3]);
        kf = (float)n; xs = wrsn_eh_label_x(t, min_charge, x_clip);
    } else { x = mc[self * WRSN_ENT_MC_F]; y = mc[self * WRSN_ENT_MC_F + 1]; t = 0.f; kf = -1.f; xs = -x_clip; }
    stored[(size_t)e * 2] = kf; stored[(size_t)e * 2 + 1] = xs;
    if (action) { float* o = action + (size_t)e * 3; o[0] = x; o[1] = y; o[2] = t; }
    if (action_f64) { double* d = action_f64 + (size_t)e * 3; d[0] = (double)x; d[1] = (double)y; d[2] = (double)t; }
}

// ------------------------------------------------------------------ the heuristic's K best picks (wrsn_lookahead_candidates)
// The ranking wrsn_entity_heuristic_label_kernel takes the head of: the alive unclaimed nodes by (score descending, index ascending), then
// the alive claimed ones in the same order.  The shape of that kernel -- a wave per row, WRSN_ENT_ROWS rows per block, no LDS, no
// __syncthreads, __shfl_xor butterflies -- with its loop over the nodes run K times: pass k leaves out the k nodes taken so far (wave-uniform
// registers; the loops over them are unrolled, so nothing is indexed at run time) and keeps two candidates per lane, the best unclaimed and
// the best claimed node, both reduced by every wave.  Pass 0 is the heuristic's own pick: with no unclaimed node every alive node is
// claimed, so "best claimed" is its fallback over all alive nodes.  The row is fetched from HBM once; passes 1 .. K - 1 read it from the
// cache.  Lane 0 writes slot r = k * B + e of the k-major outputs and of the lookahead state after every pass.
#define WRSN_LOOKAHEAD_MAX_K 8

struct WrsnLookahead {                                        // mirrors wrsn_lookahead_state of include/wrsn_hip.h (device pointers)
    int32_t K, B;
    double *t0, *t_end, *last_now, *ret, *survived;
    uint8_t *done, *died;
};

__global__ void __launch_bounds__(64 * WRSN_ENT_ROWS) wrsn_lookahead_candidates_kernel(int B, int M, int N, int K, const int32_t* __restrict__ agent_id,
                                                                                        WrsnEntityOut ent, const double* __restrict__ now, WrsnLookahead L,
                                                                                        double horizon, float charge_scale, double min_charge, float x_clip,
                                                                                        int32_t* __restrict__ cand_node, int32_t* __restrict__ sim_agent_id,
                                                                                        double* __restrict__ sim_action, float* __restrict__ stored) {
    const int lane = (int)threadIdx.x & 63;
    const int e = (int)blockIdx.x * WRSN_ENT_ROWS + ((int)threadIdx.x >> 6);
    if (e >= B) return;
    const int a = wrsn_wave_first(agent_id[e]);
    if (a < 0 || a >= M) return;
    const float* mc = ent.mc + (size_t)e * M * WRSN_ENT_MC_F;
    const float hx = ent.env[(size_t)e * WRSN_ENT_ENV_F], hy = ent.env[(size_t)e * WRSN_ENT_ENV_F + 1];
    int self = a;
    for (int o = M - 1; o >= 0; --o) if (mc[o * WRSN_ENT_MC_F + 3] == 1.f) self = o;
    float cx[WRSN_MAX_MC], cy[WRSN_MAX_MC]; bool on[WRSN_MAX_MC];
#pragma unroll
    for (int o = 0; o < WRSN_MAX_MC; ++o) {
        const int c = o < M ? o : M - 1;                      // clamped: chargers beyond M are switched off
        on[o] = o < M && o != self && mc[c * WRSN_ENT_MC_F + 4] == 1.f;
        cx[o] = mc[c * WRSN_ENT_MC_F + 6]; cy[o] = mc[c * WRSN_ENT_MC_F + 7];
    }
    const auto node = wrsn_global((const WrsnU4*)(ent.node + (size_t)e * N * WRSN_ENT_NODE_F));
    const float ninf = -__builtin_inff();
    const float mcf = (float)min_charge;                      // the label's min_charge, as wrsn_entity_heuristic_label takes it
    const double t_now = now[e];
    int taken[WRSN_LOOKAHEAD_MAX_K];
#pragma unroll
    for (int j = 0; j < WRSN_LOOKAHEAD_MAX_K; ++j) taken[j] = WRSN_EH_NONE;
#pragma unroll
    for (int k = 0; k < WRSN_LOOKAHEAD_MAX_K; ++k) {
        if (k >= K) break;                                    // (uniform over the grid)
        float sC = ninf, sU = ninf; int iC = WRSN_EH_NONE, iU = WRSN_EH_NONE;
        for (int n0 = 0; n0 < N; n0 += 64) {
            const int n = n0 + lane, c = n < N ? n : N - 1;   // clamped: nodes beyond N are no candidates
            const WrsnU4 p = wrsn_ld_u4(node + 2 * c), q = wrsn_ld_u4(node + 2 * c + 1);
            const float u = __int_as_float((int)p.x), v = __int_as_float((int)p.y), w = __int_as_float((int)p.z);
            bool free = n < N && __int_as_float((int)q.w) == 1.f;   // alive and not taken by an earlier pass
#pragma unroll
            for (int j = 0; j < WRSN_LOOKAHEAD_MAX_K; ++j) free = free && !(j < k && taken[j] == n);
            bool claimed = false;
#pragma unroll
            for (int o = 0; o < WRSN_MAX_MC; ++o) claimed = claimed || (on[o] && wrsn_eh_claims(u, v, cx[o], cy[o], hx, hy));
            const float s = w > ninf ? w : ninf;              // a NaN never beats a number
            if (free && claimed && (iC == WRSN_EH_NONE || s > sC)) { sC = s; iC = n; }
            if (free && !claimed && (iU == WRSN_EH_NONE || s > sU)) { sU = s; iU = n; }
        }
        const int bU = wrsn_eh_wave_best(sU, iU), bC = wrsn_eh_wave_best(sC, iC);
        const int n = bU != WRSN_EH_NONE ? bU : bC;
        taken[k] = n;
        if (lane != 0) continue;
        const bool valid = n != WRSN_EH_NONE || k == 0;       // no alive node: slot 0 stands still, as the heuristic does
        const size_t r = (size_t)k * B + e;
        if (valid) {
            float x, y, t, kf, xs;
            if (n != WRSN_EH_NONE) {
                const float* row = ent.node + ((size_t)e * N + n) * WRSN_ENT_NODE_F;
                x = row[0]; y = row[1]; t = wrsn_eh_charge(charge_scale, row[3]);
                kf = (float)n; xs = wrsn_eh_label_x(t, mcf, x_clip);
            } else { x = mc[self * WRSN_ENT_MC_F]; y = mc[self * WRSN_ENT_MC_F + 1]; t = 0.f; kf = -1.f; xs = -x_clip; }
            const double td = (double)t;
            cand_node[r] = n != WRSN_EH_NONE ? n : -1; sim_agent_id[r] = a;
            double* d = sim_action + r * 3; d[0] = (double)x; d[1] = (double)y; d[2] = td > min_charge ? td : min_charge;
            stored[r * 2] = kf; stored[r * 2 + 1] = xs;
        } else { cand_node[r] = -1; sim_agent_id[r] = -2; }
        L.t0[r] = t_now; L.t_end[r] = t_now + horizon; L.last_now[r] = t_now; L.ret[r] = 0.0;
        L.died[r] = 0; L.done[r] = valid ? 0 : 1;
    }
}

// ------------------------------------------------------------------ node-pointer entity policy: acting (wrsn_entity_pointer_act)
// The actor of build_entity_pointer_networks (ippo.py): the trunk of the set policy, a categorical choice of ONE alive node by a score per
// node, and a charge head on the chosen node's features.  The query needs z, z needs the pools over all nodes: the nodes are visited
// twice.  Four launches on the handle's stream:
//   wrsn_entpol_group_kernel   as for wrsn_entity_act
//   wrsn_entpol_trunk_kernel   as for wrsn_entity_act, with the pointer block's stride -> feat[e][200]
//   wrsn_entptr_head_kernel    head1, head2 (wrsn_ep_head_front), then query 128 -> 64 on the matrix cores by waves 0 and 1 -> z[e][128], q[e][64]
//   wrsn_entptr_score_kernel   one 256-thread block per row: h_i recomputed tile by tile exactly as the trunk kernel does and never stored;
//                              l_i = 0.125 <h_i, q> into LDS; then maximum, arg-max of l_i + g_i, log-sum-exp, the charge head, the outputs
// The bits of l_i do not depend on the tile, wave or column of node i: a column's MFMA chains are k-ordered whatever the column, the dot
// product with q is ONE fmaf chain over the lane's 32 units in (t2, r) order, and the two half-lanes of a column are added as
// (units of half 0) + (units of half 1) in both.  Every reduction over the nodes is either exact (maximum; minimum index among the holders
// of the maximum, as wrsn_entity_heuristic_kernel) or a sum in a fixed order: thread t adds nodes t, t + 256, ... in order, a __shfl_xor
// butterfly adds the lanes (both partners add the same two numbers), the four waves are added in wave order.  No DPP row operation: the
// emulator of tests/emu models those for one-wave blocks only.
#define WRSN_PP_QUERY WRSN_EP_MEAN                                                 // query  128 ->  64: where the Gaussian heads of the set actor sit
#define WRSN_PP_QUERY_B (WRSN_PP_QUERY + 128 * 64)
#define WRSN_PP_CHARGE_IN (128 + WRSN_ENT_NODE_F)
#define WRSN_PP_CHARGE (WRSN_PP_QUERY_B + 64)                                      // charge 136 ->   2: rows z [128], then the chosen node's features [8]
#define WRSN_PP_CHARGE_B (WRSN_PP_CHARGE + WRSN_PP_CHARGE_IN * 2)
#define WRSN_PP_FLOATS ((WRSN_PP_CHARGE_B + 2 + 3) / 4 * 4)                        // rounded up to a multiple of 4
static_assert(WRSN_PP_QUERY == 48448 && WRSN_PP_QUERY_B == 56640 && WRSN_PP_CHARGE == 56704 && WRSN_PP_CHARGE_B == 56976 && WRSN_PP_FLOATS == 56980,
              "the layout documented in include/wrsn_hip.h");
static_assert(WRSN_PP_CHARGE_IN % 4 == 0, "the charge head runs four chains over k mod 4");
// LDS of the score block, in floats: node1 / node2 with their biases, q [64], z [128], the reduction slots [16], l [N rounded up to whole tiles]
#define WRSN_PP_S_Q WRSN_EP_MC1
#define WRSN_PP_S_Z (WRSN_PP_S_Q + 64)
#define WRSN_PP_S_RED (WRSN_PP_S_Z + 128)
#define WRSN_PP_S_L (WRSN_PP_S_RED + 16)
#define WRSN_PP_SCORE_LDS(N) ((size_t)(WRSN_PP_S_L + (((N) + 31) & ~31)) * 4)     // bytes

// The candidate mask (wrsn_set_entity_pointer_mask, WRSN_POINTER_MASK_CLAIMED; include/wrsn_hip.h has the rule, statement for statement):
// one pass of the 256-thread score block over sL, between the barrier behind the tile loop that fills it and the first reduction.  The
// chargers (at most eight) and the disc's half-axes are read with block-uniform addresses, as wrsn_entity_heuristic_kernel reads them; a
// claimer is an alive charger row that is not is_self, so acting rows and stored packed rows give the same mask.  Thread t takes nodes
// t, t + 256, ... -- the nodes it takes in every reduction behind, so what it writes here it alone reads until the next barrier.  The
// block ORs "some alive node is unclaimed" (exact: a __shfl_xor butterfly, then four LDS slots in wave order; no DPP row operation) and,
// where that holds, every claimed node's sL becomes -inf; where it does not -- every alive node claimed, or none alive -- sL stays: the
// heuristic's fallback.  Behind the pass -inf IS "no candidate": nothing reads a flag again.  One __syncthreads; `claimed` is formed
// twice (before and behind it) and not kept, a row holds any number of nodes per thread.  sAny: four int slots nobody else holds now.
WDEV void wrsn_pp_mask_claimed(float* sL, int* sAny, const float* __restrict__ nrow, const float* __restrict__ mc, const float* __restrict__ env,
                               int N, int M) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float ninf = -__builtin_inff();
    const float hx = env[0], hy = env[1];
    float cx[WRSN_MAX_MC], cy[WRSN_MAX_MC]; bool on[WRSN_MAX_MC];
#pragma unroll
    for (int o = 0; o < WRSN_MAX_MC; ++o) {
        const int c = o < M ? o : M - 1;                      // clamped: chargers beyond M are switched off
        on[o] = o < M && mc[c * WRSN_ENT_MC_F + 4] == 1.f && !(mc[c * WRSN_ENT_MC_F + 3] == 1.f);   // alive and not is_self
        cx[o] = mc[c * WRSN_ENT_MC_F + 6]; cy[o] = mc[c * WRSN_ENT_MC_F + 7];
    }
    int any = 0;
    for (int n = tid; n < N; n += 256) {
        const float u = nrow[(size_t)n * WRSN_ENT_NODE_F], v = nrow[(size_t)n * WRSN_ENT_NODE_F + 1];
        bool claimed = false;
#pragma unroll
        for (int o = 0; o < WRSN_MAX_MC; ++o) claimed = claimed || (on[o] && wrsn_eh_claims(u, v, cx[o], cy[o], hx, hy));
        any |= (sL[n] > ninf && !claimed) ? 1 : 0;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) any |= __shfl_xor(any, d);
    if (lane == 0) sAny[wave] = any;
    __syncthreads();
    if (!(sAny[0] | sAny[1] | sAny[2] | sAny[3])) return;     // block-uniform: no alive node is unclaimed, the alive nodes stay
    for (int n = tid; n < N; n += 256) {
        const float u = nrow[(size_t)n * WRSN_ENT_NODE_F], v = nrow[(size_t)n * WRSN_ENT_NODE_F + 1];
        bool claimed = false;
#pragma unroll
        for (int o = 0; o < WRSN_MAX_MC; ++o) claimed = claimed || (on[o] && wrsn_eh_claims(u, v, cx[o], cy[o], hx, hy));
        if (claimed) sL[n] = ninf;
    }
}

struct WrsnEntPtrOut { int32_t* node; float* stored; float* action; double* action_f64; float* logp; float* node_logp; float* charge_mean; float* charge_log_std; };   // mirrors wrsn_entity_pointer_out

__global__ void __launch_bounds__(256) wrsn_entptr_head_kernel(int B, int M, const float* __restrict__ actors, const float* __restrict__ feat,
                                                               const int32_t* __restrict__ list, const int32_t* __restrict__ cnt,
                                                               float* __restrict__ zbuf, float* __restrict__ qbuf) {
    extern __shared__ double smem[];
    float* sF = (float*)smem;
    float* sZ = sF + WRSN_EP_H_Z;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    int rows; const int32_t* mine; const float* blk;
    if (!wrsn_ep_head_front(B, M, WRSN_PP_FLOATS, actors, feat, list, cnt, sF, sZ, rows, mine, blk)) return;   // block-uniform
    for (int i = tid; i < rows * 128; i += 256) {             // z = sF [128 units][32 columns], row by row
        const int j = i >> 7, u = i & 127;
        zbuf[(size_t)mine[j] * 128 + u] = sF[u * 32 + j];
    }
    if (wave < 2) {                                           // query: wave w holds units 32 w .. 32 w + 31 of all 32 columns (wave-uniform)
        wrsn_v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = blk[WRSN_PP_QUERY_B + 32 * wave + wrsn_ep_unit(r, h)];
        const float* wa = blk + WRSN_PP_QUERY + h * 64 + 32 * wave + col;
        const float* xb = sF + h * 32 + col;
#pragma unroll 8
        for (int kk = 0; kk < 64; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kk * 128], xb[kk * 64], acc, 0, 0, 0);
        if (col < rows) {
            float* q = qbuf + (size_t)mine[col] * 64 + 32 * wave;
#pragma unroll
            for (int r = 0; r < 16; ++r) q[wrsn_ep_unit(r, h)] = acc[r];
        }
    }
}

__global__ void __launch_bounds__(256) wrsn_entptr_score_kernel(int B, int M, int N, const float* __restrict__ actors,
                                                                const int32_t* __restrict__ agent_id, WrsnEntityOut ent,
                                                                const float* __restrict__ zbuf, const float* __restrict__ qbuf,
                                                                const float* __restrict__ gumbel, const float* __restrict__ eps,
                                                                float min_charge, WrsnEntPtrOut out, int mask) {
    extern __shared__ double smem[];
    float* sW = (float*)smem;
    float* sQ = sW + WRSN_PP_S_Q;
    float* sZ = sW + WRSN_PP_S_Z;
    float* sR = sW + WRSN_PP_S_RED;
    int* sK = (int*)sR;                                       // the index slots of the reductions
    float* sL = sW + WRSN_PP_S_L;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    const int e = (int)blockIdx.x;
    if (e >= B) return;
    const int aid = wrsn_wave_first(agent_id[e]);
    if (aid < 0 || aid >= M) return;
    const float* blk = actors + (size_t)aid * WRSN_PP_FLOATS;
    {   // node1, node2 and their biases, as the trunk kernel stages them
        const auto src = wrsn_global((const WrsnU4*)blk);
        WrsnU4* dst = (WrsnU4*)sW;
        for (int i = tid; i < WRSN_EP_MC1 / 4; i += 256) dst[i] = wrsn_ld_u4(src + i);
    }
    if (tid < 64) sQ[tid] = qbuf[(size_t)e * 64 + tid];
    else if (tid < 192) sZ[tid - 64] = zbuf[(size_t)e * 128 + tid - 64];
    __syncthreads();
    const float ninf = -__builtin_inff();
    const float* nrow = ent.node + (size_t)e * N * WRSN_ENT_NODE_F;
    const int ntile = (N + 31) >> 5;
    for (int tile = wave; tile < ((ntile + 3) & ~3); tile += 4) {   // every wave the same number of rounds: the exchange below is one
        const bool on = tile < ntile;                          // wave-uniform
        const int n = tile * 32 + col, srcn = n < N ? n : N - 1;   // clamped: a column beyond N is computed on zeros and stored nowhere
        const auto p = wrsn_global((const WrsnU4*)(nrow + (size_t)srcn * WRSN_ENT_NODE_F));
        const WrsnU4 c0 = wrsn_ld_u4(p), c1 = wrsn_ld_u4(p + 1);
        const bool alive = n < N && __int_as_float((int)c1.w) == 1.f;
        float x[4];                                           // features 2 kk + h of the column, zeros unless the node is alive (a select)
        x[0] = __int_as_float((int)(h ? c0.y : c0.x)); x[1] = __int_as_float((int)(h ? c0.w : c0.z));
        x[2] = __int_as_float((int)(h ? c1.y : c1.x)); x[3] = __int_as_float((int)(h ? c1.w : c1.z));
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) x[kk] = alive ? x[kk] : 0.f;
        float part = 0.f;                                     // <h_i, q> over this lane's 32 units: 32 t2 + u(r) + 4 h
        if (on) {
            wrsn_v16f h1[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                wrsn_v16f acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = sW[WRSN_EP_NODE1_B + 32 * t + wrsn_ep_unit(r, h)];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sW[WRSN_EP_NODE1 + (2 * kk + h) * 64 + 32 * t + col], x[kk], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) h1[t][r] = fmaxf(acc[r], 0.f);
            }
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) {
                wrsn_v16f acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = sW[WRSN_EP_NODE2_B + 32 * t2 + wrsn_ep_unit(r, h)];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)              // register r of h1[t]: the k-pair (u, u + 4), u = 32 t + (r & 3) + 8 (r >> 2)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sW[WRSN_EP_NODE2 + (32 * t + wrsn_ep_unit(r, h)) * 64 + 32 * t2 + col], h1[t][r], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) part = fmaf(fmaxf(acc[r], 0.f), sQ[32 * t2 + wrsn_ep_unit(r, h)], part);
            }
        }
        const float other = __shfl_xor(part, 32);             // the column's other half: both halves form (half 0) + (half 1)
        const float l = 0.125f * ((h ? other : part) + (h ? part : other));
        if (on && h == 0 && n < N) sL[n] = (alive && l > ninf) ? l : ninf;   // a select: whatever a dead or padded node row holds never enters; -inf IS "not alive" below
    }
    __syncthreads();
    if (mask)                                                 // block-uniform: the candidates among the alive nodes; behind it -inf IS "no candidate"
        wrsn_pp_mask_claimed(sL, sK + 12, nrow, ent.mc + (size_t)e * M * WRSN_ENT_MC_F, ent.env + (size_t)e * WRSN_ENT_ENV_F, N, M);
    // ---- over the alive nodes: the maximum of l and the maximum of l + g -- thread t takes nodes t, t + 256, ...
    const float* grow = gumbel ? gumbel + (size_t)e * N : nullptr;
    float mx = ninf, bs = ninf;
    for (int n = tid; n < N; n += 256) {
        const float l = sL[n];
        if (!(l > ninf)) continue;                            // -inf marks a node that is not alive: the flag is not read again
        mx = l > mx ? l : mx;
        const float sc = grow ? l + grow[n] : l;
        const float s = sc > ninf ? sc : ninf;                // a NaN never beats a number
        bs = s > bs ? s : bs;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_xor(mx, d); mx = o > mx ? o : mx;
        const float b = __shfl_xor(bs, d); bs = b > bs ? b : bs;
    }
    if (lane == 0) { sR[wave] = mx; sR[4 + wave] = bs; }
    __syncthreads();
    const float m_all = fmaxf(fmaxf(sR[0], sR[1]), fmaxf(sR[2], sR[3]));
    const float b_all = fmaxf(fmaxf(sR[4], sR[5]), fmaxf(sR[6], sR[7]));
    // ---- the lowest index among the holders of the best score; the sum of exp(l - max) in a fixed order
    float sum = 0.f; int k = WRSN_EH_NONE;
    for (int n = tid; n < N; n += 256) {
        const float l = sL[n];
        if (!(l > ninf)) continue;
        sum += expf(l - m_all);
        const float sc = grow ? l + grow[n] : l;
        const float s = sc > ninf ? sc : ninf;
        if (k == WRSN_EH_NONE && s == b_all) k = n;           // increasing n: the lane's lowest
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        sum += __shfl_xor(sum, d);
        const int o = __shfl_xor(k, d); k = o < k ? o : k;
    }
    if (lane == 0) { sR[8 + wave] = sum; sK[12 + wave] = k; }
    __syncthreads();
    const float s_all = ((sR[8] + sR[9]) + sR[10]) + sR[11];
    int node = sK[12];
#pragma unroll
    for (int w = 1; w < 4; ++w) node = sK[12 + w] < node ? sK[12 + w] : node;
    const bool any = node != WRSN_EH_NONE;                    // block-uniform: some node is alive
    const float lse = m_all + logf(s_all);                    // used only when `any`
    if (out.node_logp) {
        float* o = out.node_logp + (size_t)e * N;
        for (int n = tid; n < N; n += 256) o[n] = sL[n] > ninf ? sL[n] - lse : ninf;
    }
    // ---- the charge head on [z, x_k]: thread d = 0 (mean), 1 (log_std); four k-ordered chains over k mod 4, added as (0 + 1) + (2 + 3)
    if (tid < 2) {
        const float* w = blk + WRSN_PP_CHARGE + tid;
        const float* z = sZ;
        const float* xk = nrow + (size_t)(any ? node : 0) * WRSN_ENT_NODE_F;
        float s0 = blk[WRSN_PP_CHARGE_B + tid], s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 4
        for (int i = 0; i < 128; i += 4) {
            s0 = fmaf(z[i], w[2 * i], s0); s1 = fmaf(z[i + 1], w[2 * i + 2], s1);
            s2 = fmaf(z[i + 2], w[2 * i + 4], s2); s3 = fmaf(z[i + 3], w[2 * i + 6], s3);
        }
#pragma unroll
        for (int i = 0; i < WRSN_ENT_NODE_F; i += 4) {        // the chosen node's own features; zeros when no node is alive (a select)
            const float* wn = w + 2 * (128 + i);
            s0 = fmaf(any ? xk[i] : 0.f, wn[0], s0); s1 = fmaf(any ? xk[i + 1] : 0.f, wn[2], s1);
            s2 = fmaf(any ? xk[i + 2] : 0.f, wn[4], s2); s3 = fmaf(any ? xk[i + 3] : 0.f, wn[6], s3);
        }
        sR[tid] = (s0 + s1) + (s2 + s3);                      // the maxima of sR[0..7] were read before the last barrier
    }
    __syncthreads();
    if (tid != 0) return;
    const float mu = sR[0], ls = fminf(fmaxf(sR[1], -4.f), 1.f);
    const float ep = eps ? eps[e] : 0.f;
    const float x = fmaf(expf(ls), ep, mu);
    const float c = min_charge + (1.f - min_charge) * (1.f / (1.f + expf(-x)));
    float u, v;
    if (any) { u = nrow[(size_t)node * WRSN_ENT_NODE_F]; v = nrow[(size_t)node * WRSN_ENT_NODE_F + 1]; }
    else {                                                    // the asking charger's own position: the heuristic's rule
        const float* mc = ent.mc + (size_t)e * M * WRSN_ENT_MC_F;
        int self = aid;
        for (int o = M - 1; o >= 0; --o) if (mc[o * WRSN_ENT_MC_F + 3] == 1.f) self = o;
        u = mc[self * WRSN_ENT_MC_F]; v = mc[self * WRSN_ENT_MC_F + 1];
    }
    const int kout = any ? node : -1;
    const float lp = (any ? sL[node] - lse : 0.f) + (-0.5f * ep * ep - ls - 0.9189385f);   // 0.5 log(2 pi)
    out.node[e] = kout;
    out.stored[(size_t)e * 2] = (float)kout; out.stored[(size_t)e * 2 + 1] = x;
    float* a = out.action + (size_t)e * 3;
    a[0] = u; a[1] = v; a[2] = c;
    if (out.action_f64) { double* d = out.action_f64 + (size_t)e * 3; d[0] = (double)u; d[1] = (double)v; d[2] = (double)c; }
    out.logp[e] = lp;
    if (out.charge_mean) out.charge_mean[e] = mu;
    if (out.charge_log_std) out.charge_log_std[e] = ls;
}

// ------------------------------------------------------------------ episode ledger (wrsn_episodes_collect)
// One entry per finished episode and environment, and the restart mask of the evaluation loop.  One thread per environment, 256 per
// block: a row's state lives in its own slots of the caller's arrays, so there is no atomic, no reduction and no order to fix.  The
// rules (include/wrsn_hip.h) are keyed on WrsnDev.row_state exactly as wrsn_tr_collect_entities_kernel's are.
struct WrsnEpisodeLog {                                       // mirrors wrsn_episode_log of include/wrsn_hip.h (device pointers)
    int32_t episodes, quota;
    double* run_return; int32_t* run_decisions; int32_t* finished; int32_t* dropped;
    double* lifetime; double* ep_return; int32_t* decisions; int32_t* ended; int32_t* record;
};

__global__ void __launch_bounds__(256) wrsn_episodes_kernel(int B, int M, WrsnEpisodeLog L, const int32_t* __restrict__ agent_id,
                                                            const double* __restrict__ reward, const double* __restrict__ now,
                                                            const int32_t* __restrict__ status, int32_t* __restrict__ row_state,
                                                            const int32_t* __restrict__ pool_cur, double time_limit,
                                                            int32_t* __restrict__ next_agent_id, uint8_t* __restrict__ restart, int consume) {
    const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (e >= B) return;
    const int st = row_state[e];
    const int k = L.finished[e];
    double* run = L.run_return + (size_t)e * M; int32_t* dec = L.run_decisions + (size_t)e * M;
    int next = 0, close = 0; bool has_next = false; uint8_t again = 0;
    if (L.quota > 0 && k >= L.quota) { next = -2; has_next = true; }          // parked: whatever the launch did with the row
    else if (st == 3) { next = -1; has_next = true; }                         // step in flight
    else if (st == 2) {                                                       // reset / auto-reset / pool swap: an episode starts
        for (int m = 0; m < M; ++m) { run[m] = 0.0; dec[m] = 0; }
        next = agent_id[e]; has_next = true;
    } else if (st == 1) {                                                     // fresh request
        const int a = agent_id[e];
        if (a >= 0 && a < M) { run[a] += reward[e]; dec[a] += 1; }
        if (status[e] == 1) close = 3;
        else if (time_limit > 0.0 && now[e] >= time_limit) close = 2;
        else { next = a; has_next = true; }
    } else if (st == 4) close = 1;                                            // terminal return
    if (close) {
        if (k < L.episodes) {
            const size_t q = (size_t)k * B + e;
            L.lifetime[q] = now[e]; L.ended[q] = close;
            for (int m = 0; m < M; ++m) { L.ep_return[q * M + m] = run[m]; L.decisions[q * M + m] = dec[m]; }
            if (L.record) L.record[q] = pool_cur[e];
        } else L.dropped[e] += 1;
        L.finished[e] = k + 1;
        for (int m = 0; m < M; ++m) { run[m] = 0.0; dec[m] = 0; }
        next = -2; has_next = true;
        again = (L.quota > 0 && k + 1 >= L.quota) ? 0 : 1;                    // parked from now on: not restarted
    }
    if (next_agent_id && has_next) next_agent_id[e] = next;
    if (restart) restart[e] = again;
    if (consume && (st == 1 || st == 2 || st == 4)) row_state[e] = 0;
}

// ------------------------------------------------------------------ lookahead bookkeeping and choice (wrsn_lookahead_collect, wrsn_lookahead_pick)
// The roll-forward of the K * B cloned environments of a simulation handle, booked per slot as the episode ledger books an environment:
// one thread per slot, 256 per block, keyed on WrsnDev.row_state exactly as wrsn_episodes_kernel; a slot's state lives in its own elements
// of the caller's arrays, so there is no atomic, no reduction and no order to fix.  The rules are in include/wrsn_hip.h.  The row state is
// always consumed.
__global__ void __launch_bounds__(256) wrsn_lookahead_collect_kernel(int R, WrsnLookahead L, const int32_t* __restrict__ agent_id,
                                                                     const double* __restrict__ reward, const double* __restrict__ now,
                                                                     const int32_t* __restrict__ status, int32_t* __restrict__ row_state,
                                                                     int32_t* __restrict__ next_agent_id, int close_all) {
    const int r = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (r >= R) return;
    const int st = row_state[r];
    if (st == 1 || st == 2 || st == 4) row_state[r] = 0;
    if (L.done[r]) { next_agent_id[r] = -2; return; }
    double last = L.last_now[r];
    bool close = false;
    if (st == 3) next_agent_id[r] = -1;                                       // step in flight
    else if (st == 1) {                                                       // fresh request
        L.ret[r] += reward[r];
        last = now[r]; L.last_now[r] = last;
        if (status[r] == 1 || last >= L.t_end[r]) close = true;
        else next_agent_id[r] = agent_id[r];
    } else if (st == 4) {                                                     // terminal return: no reward, as in the ledger
        L.died[r] = 1;
        last = now[r]; L.last_now[r] = last;
        close = true;
    }
    if (close || close_all) {
        const double te = L.t_end[r];
        L.survived[r] = (last < te ? last : te) - L.t0[r];
        L.done[r] = 1;
        next_agent_id[r] = -2;
    }
}

// One thread per row of the REAL batch: the lexicographic best over the row's valid, finished slots -- survived descending, then ret
// descending, then k ascending; anything that is not > -inf (a NaN) counts as -inf, so a NaN never beats a number.  No weight between
// the two keys.  Nothing qualifies: k = 0.
__global__ void __launch_bounds__(256) wrsn_lookahead_pick_kernel(int B, int M, const int32_t* __restrict__ agent_id, WrsnLookahead L,
                                                                  const int32_t* __restrict__ sim_agent_id, const double* __restrict__ sim_action,
                                                                  const float* __restrict__ cand_stored, int32_t* __restrict__ choice,
                                                                  double* __restrict__ action_f64, float* __restrict__ action,
                                                                  float* __restrict__ stored) {
    const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (e >= B) return;
    const int a = agent_id[e];
    if (a < 0 || a >= M) return;
    const double ninf = -__builtin_inf();
    int best = -1; double bs = ninf, br = ninf;
    for (int k = 0; k < L.K; ++k) {
        const size_t r = (size_t)k * B + e;
        if (sim_agent_id[r] < 0 || !L.done[r]) continue;
        const double sv = L.survived[r], rt = L.ret[r];
        const double s = sv > ninf ? sv : ninf, q = rt > ninf ? rt : ninf;
        if (best < 0 || s > bs || (s == bs && q > br)) { best = k; bs = s; br = q; }
    }
    if (best < 0) best = 0;
    const size_t r = (size_t)best * B + e;
    choice[e] = best;
    const double x = sim_action[r * 3], y = sim_action[r * 3 + 1], t = sim_action[r * 3 + 2];
    if (action_f64) { double* d = action_f64 + (size_t)e * 3; d[0] = x; d[1] = y; d[2] = t; }
    if (action) { float* o = action + (size_t)e * 3; o[0] = (float)x; o[1] = (float)y; o[2] = (float)t; }
    if (stored) { stored[(size_t)e * 2] = cand_stored[r * 2]; stored[(size_t)e * 2 + 1] = cand_stored[r * 2 + 1]; }
}
