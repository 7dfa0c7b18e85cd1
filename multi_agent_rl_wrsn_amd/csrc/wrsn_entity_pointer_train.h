// wrsn_entity_pointer_train.h -- the PPO gradient of the node-pointer policy on the device (gfx950): wrsn_entity_pointer_eval,
// wrsn_entity_pointer_ppo_grad and the multi-group forms wrsn_entity_pointer_ppo_grad_multi, wrsn_entity_pointer_adam_multi and
// wrsn_entity_pointer_ppo_update of include/wrsn_hip.h.  Every kernel serves G groups (WrsnEtGroups) in one launch, the group folded into
// blockIdx.x; the single-group calls are G = 1.  Group g's slice of the pointer scratch lies g * WrsnEtpScratch::chunk floats behind group 0's.
//
// EntityPointerActor.forward, EntityCritic.forward and PPOLearner.minibatch_loss (ippo.py) on packed entity rows, a pointer block
// (wrsn_entity_pointer_act's layout: the set actor's trunk, then query and charge) and a critic block.  The trunk and the two head layers
// are the set policy's, at the same offsets, so the kernels of wrsn_entity_train.h serve both nets as they are; what the pointer adds:
//   wrsn_et_trunk_fwd_kernel, wrsn_et_head_fwd_kernel   unchanged: z = head2's output [n][128] of the actor, the critic's value.  (The six
//                              Gaussian dot products the head kernel forms for an actor read inside the query weights and land in raw[0..5],
//                              which nothing of this file reads.)
//   wrsn_etp_query_kernel      tiles of <= 32 rows: q = query(z) on the matrix cores, wrsn_entptr_head_kernel's chain -> q [n][64]
//   wrsn_etp_score_fwd_kernel  one 256-thread block per row: wrsn_entptr_score_kernel on a packed row with the STORED node in place of the
//                              arg-max -- l_i through wrsn_et_tile_fwd, maximum, exp-sum and the charge head in that kernel's orders, so
//                              node_logp, the charge mean and log_std are its bits --, then the categorical entropy, logp and H; with
//                              the candidate mask (wrsn_set_entity_pointer_mask) that kernel's pass wrsn_pp_mask_claimed on the packed
//                              row, behind which -inf IS "no candidate": kv, the stored log p and dl carry the mask to the two
//                              backward kernels, which read no alive flag for the scores and stay as they are
//   wrsn_etp_loss_kernel       wrsn_et_loss_body<true>: the loss on scalar (logp, H) -> a = d loss / d logp, e = d loss / d H, d / d value
//   wrsn_etp_score_bwd_kernel  one block per row: dl in place of node_logp, dq = 0.125 sum_i dl_i h_i with h_i recomputed tile by tile
//                              (tile order, then wave order), (dmu, ds_raw), and dz = W_charge[0:128] (dmu, ds_raw) + W_query dq
//   wrsn_etp_head_bwd_kernel   wrsn_et_head_bwd_body<true>: the actor starts from that dz, the critic from its value as ever
//   wrsn_et_trunk_bwd_kernel   unchanged, both nets: the pools' part of delta2
//   wrsn_etp_trunk_bwd_kernel  the actor's rows: the scores' part of delta2, 0.125 dl_i q_u, through the same tiles on its own (see there)
//   wrsn_etp_reduce_kernel     wrsn_et_reduce_body<true>: the pointer block's layout; node1 / node2 add the two partials
// The rules of wrsn_entity_train.h hold: every sum in a fixed order, no float atomics, no DPP row operation, at most 64 KB of LDS.
#pragma once
#include "wrsn_entity_train.h"

// LDS of the score kernels, in floats: wrsn_entptr_score_kernel's (node1 / node2, q [64], z [128], 16 reduction slots, l [N in whole tiles]);
// the backward keeps the four waves' dq partials where the forward keeps q and z
#define WRSN_ETP_S_PART (WRSN_PP_S_Q)
#define WRSN_ETP_B_DL (WRSN_ETP_S_PART + 256 + 64)
#define WRSN_ETP_BWD_LDS(N) ((size_t)(WRSN_ETP_B_DL + (((N) + 31) & ~31)) * 4)   // bytes

struct WrsnEtpEvalOut { float* logp; float* entropy; float* node_logp; float* charge_mean; float* charge_log_std; };   // any may be null

static inline size_t wrsn_etp_scratch_floats(size_t n, int N, bool grad) {   // host
    const size_t ld = (size_t)((N + 31) & ~31);
    return n * (64 + ld + 8) + (grad ? n * (64 + 4 + WRSN_EP_MC1) : 0);
}

// group g's slice of the pointer scratch
WDEV WrsnEtpScratch wrsn_etp_slice(WrsnEtpScratch ps, int g) {
    const size_t o = (size_t)g * ps.chunk;
    ps.q += o; ps.lp += o; ps.prow += o; ps.dq += o; ps.dch += o; ps.part2 += o;
    return ps;
}

// which (group, row) a block of the per-row pointer kernels is: these serve the actor alone, so their grid is G * n -- block index =
// group * n + row -- and not wrsn_et_who's 2 * G * n with a critic half that returns at once.  The group's entry of the table is read
// by that wave-uniform index (scalar loads).  src: the row's place in the group's rows and batch arrays.
struct WrsnEtpWho { int grp, i; size_t src; const float* blk; const float* row; const float* stored; };
WDEV WrsnEtpWho wrsn_etp_who(const WrsnEtGroups& gs, const WrsnEtDims& dm) {
    WrsnEtpWho w;
    w.grp = (int)blockIdx.x / dm.n; w.i = (int)blockIdx.x - w.grp * dm.n;
    const WrsnEtGroup& G = gs.g[w.grp];
    w.blk = G.actor; w.stored = G.b.action;
    const int32_t* index = G.index;
    w.src = (size_t)(index ? wrsn_wave_first(index[w.i]) : w.i);
    w.row = G.rows + w.src * (size_t)(WRSN_ENT_NODE_F * dm.N + WRSN_ENT_MC_F * dm.M + WRSN_ENT_ENV_F);
    return w;
}

__global__ void __launch_bounds__(256) wrsn_etp_query_kernel(WrsnEtGroups gs, int n, WrsnEtScratch s0, WrsnEtpScratch ps0) {
    extern __shared__ double smem[];
    float* sF = (float*)smem;                                 // z [128 units][32 columns]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    const int nt = (n + WRSN_EP_HEAD_ROWS - 1) / WRSN_EP_HEAD_ROWS;
    const int grp = (int)blockIdx.x / nt;                     // block index = group * (tiles per group) + tile
    const float* blk = gs.g[grp].actor;
    const WrsnEtScratch s = wrsn_et_slice(s0, grp);
    const WrsnEtpScratch ps = wrsn_etp_slice(ps0, grp);
    const int first = ((int)blockIdx.x - grp * nt) * WRSN_EP_HEAD_ROWS;
    const int rows = n - first < WRSN_EP_HEAD_ROWS ? n - first : WRSN_EP_HEAD_ROWS;
    for (int i = tid; i < WRSN_EP_HEAD_ROWS * 128; i += 256) {   // a column beyond `rows` repeats the last row: computed, not stored
        const int j = i >> 7, u = i & 127;
        sF[u * 32 + j] = s.z2[(size_t)(first + (j < rows ? j : rows - 1)) * 128 + u];
    }
    __syncthreads();
    if (wave < 2) {                                           // wave w holds units 32 w .. 32 w + 31 of all 32 columns (wave-uniform)
        wrsn_v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = blk[WRSN_PP_QUERY_B + 32 * wave + wrsn_ep_unit(r, h)];
        const float* wa = blk + WRSN_PP_QUERY + h * 64 + 32 * wave + col;
        const float* xb = sF + h * 32 + col;
#pragma unroll 8
        for (int kk = 0; kk < 64; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kk * 128], xb[kk * 64], acc, 0, 0, 0);
        if (col < rows) {
            float* q = ps.q + (size_t)(first + col) * 64 + 32 * wave;
#pragma unroll
            for (int r = 0; r < 16; ++r) q[wrsn_ep_unit(r, h)] = acc[r];
        }
    }
}

// the stored node of a row: (int) kf when kf is finite and that index names a node, else -1.  A select on the float: nothing is indexed by it before
WDEV int wrsn_etp_node(float kf, int N) {
    const bool fin = kf > -2147483648.f && kf < 2147483648.f;     // a NaN fails both
    const int k = fin ? (int)kf : -1;
    return (k >= 0 && k < N) ? k : -1;
}

// stored0: the decisions of wrsn_entity_pointer_eval (one group); null in the gradient path, where they are the group's b.action
__global__ void __launch_bounds__(256) wrsn_etp_score_fwd_kernel(WrsnEtGroups gs, WrsnEtDims dm, WrsnEtScratch s0, WrsnEtpScratch ps0,
                                                                 const float* __restrict__ stored0, WrsnEtpEvalOut out, int mask) {
    extern __shared__ double smem[];
    float* sW = (float*)smem;
    float* sQ = sW + WRSN_PP_S_Q;
    float* sZ = sW + WRSN_PP_S_Z;
    float* sR = sW + WRSN_PP_S_RED;
    float* sL = sW + WRSN_PP_S_L;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    const WrsnEtpWho who = wrsn_etp_who(gs, dm);
    const float* blk = who.blk;
    const WrsnEtScratch s = wrsn_et_slice(s0, who.grp);
    const WrsnEtpScratch ps = wrsn_etp_slice(ps0, who.grp);
    const int N = dm.N, i = who.i;
    const size_t src = who.src;
    const float* stored = stored0 ? stored0 : who.stored;
    {   // node1, node2 and their biases, as the trunk kernel stages them
        const auto g = wrsn_global((const WrsnU4*)blk);
        WrsnU4* dst = (WrsnU4*)sW;
        for (int j = tid; j < WRSN_EP_MC1 / 4; j += 256) dst[j] = wrsn_ld_u4(g + j);
    }
    if (tid < 64) sQ[tid] = ps.q[(size_t)i * 64 + tid];
    else if (tid < 192) sZ[tid - 64] = s.z2[(size_t)i * 128 + tid - 64];
    __syncthreads();
    const float ninf = -__builtin_inff();
    const float* nrow = who.row;
    const int ntile = (N + 31) >> 5;
    for (int tile = wave; tile < ((ntile + 3) & ~3); tile += 4) {   // every wave the same number of rounds: the exchange below is one
        const bool on = tile < ntile;                          // wave-uniform
        const int n = tile * 32 + col;
        float part = 0.f;                                     // <h_i, q> over this lane's 32 units: 32 t2 + u(r) + 4 h
        bool alive = false;
        if (on) {
            float x[4]; wrsn_v16f h1[2], h2[2];
            alive = wrsn_et_tile_fwd(sW, nrow, N, tile, col, h, x, h1, h2);
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
                for (int r = 0; r < 16; ++r) part = fmaf(h2[t2][r], sQ[32 * t2 + wrsn_ep_unit(r, h)], part);
        }
        const float other = __shfl_xor(part, 32);             // the column's other half: both halves form (half 0) + (half 1)
        const float l = 0.125f * ((h ? other : part) + (h ? part : other));
        if (on && h == 0 && n < N) sL[n] = (alive && l > ninf) ? l : ninf;   // -inf IS "not alive" below
    }
    __syncthreads();
    if (mask)                                                 // block-uniform: wrsn_entptr_score_kernel's pass on the packed row [node | mc | env]
        wrsn_pp_mask_claimed(sL, (int*)sR + 12, nrow, nrow + (size_t)N * WRSN_ENT_NODE_F,
                             nrow + (size_t)N * WRSN_ENT_NODE_F + (size_t)dm.M * WRSN_ENT_MC_F, N, dm.M);
    // ---- over the alive nodes: the maximum, then the sum of exp(l - max) -- thread t takes nodes t, t + 256, ...; lanes by a butterfly, waves in order
    float mx = ninf;
    for (int n = tid; n < N; n += 256) {
        const float l = sL[n];
        if (!(l > ninf)) continue;
        mx = l > mx ? l : mx;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const float o = __shfl_xor(mx, d); mx = o > mx ? o : mx; }
    if (lane == 0) sR[wave] = mx;
    __syncthreads();
    const float m_all = fmaxf(fmaxf(sR[0], sR[1]), fmaxf(sR[2], sR[3]));
    float sum = 0.f;
    for (int n = tid; n < N; n += 256) {
        const float l = sL[n];
        if (!(l > ninf)) continue;
        sum += expf(l - m_all);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) sum += __shfl_xor(sum, d);
    if (lane == 0) sR[8 + wave] = sum;
    __syncthreads();
    const float s_all = ((sR[8] + sR[9]) + sR[10]) + sR[11];
    const bool any = m_all > ninf;                            // block-uniform: some node is alive
    const float lse = m_all + logf(s_all);                    // used only when `any`
    // ---- log-probabilities of the nodes and the categorical entropy -sum p log p, in the same order
    float hs = 0.f;
    float* lrow = ps.lp + (size_t)i * ps.ld;
    for (int n = tid; n < ps.ld; n += 256) {
        const float lp = (n < N && sL[n] > ninf) ? sL[n] - lse : ninf;
        lrow[n] = lp;
        if (out.node_logp && n < N) out.node_logp[(size_t)i * N + n] = lp;
        if (lp > ninf) hs += expf(lp) * lp;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) hs += __shfl_xor(hs, d);
    if (lane == 0) sR[4 + wave] = hs;
    const int k = wrsn_etp_node(stored[src * 2], N), kk = k < 0 ? 0 : k;
    // ---- the charge head on [z, x_k]: thread d = 0 (mean), 1 (log_std); four k-ordered chains over k mod 4, added as (0 + 1) + (2 + 3)
    if (tid < 2) {
        const float* w = blk + WRSN_PP_CHARGE + tid;
        const float* z = sZ;
        const float* xk = nrow + (size_t)kk * WRSN_ENT_NODE_F;   // the node row as it stands, alive or not; zeros for node -1 (a select)
        float s0 = blk[WRSN_PP_CHARGE_B + tid], s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 4
        for (int j = 0; j < 128; j += 4) {
            s0 = fmaf(z[j], w[2 * j], s0); s1 = fmaf(z[j + 1], w[2 * j + 2], s1);
            s2 = fmaf(z[j + 2], w[2 * j + 4], s2); s3 = fmaf(z[j + 3], w[2 * j + 6], s3);
        }
#pragma unroll
        for (int j = 0; j < WRSN_ENT_NODE_F; j += 4) {
            const float* wn = w + 2 * (128 + j);
            s0 = fmaf(k >= 0 ? xk[j] : 0.f, wn[0], s0); s1 = fmaf(k >= 0 ? xk[j + 1] : 0.f, wn[2], s1);
            s2 = fmaf(k >= 0 ? xk[j + 2] : 0.f, wn[4], s2); s3 = fmaf(k >= 0 ? xk[j + 3] : 0.f, wn[6], s3);
        }
        sR[tid] = (s0 + s1) + (s2 + s3);                      // the maxima of sR[0..3] were read before the last barrier
    }
    __syncthreads();
    if (tid != 0) return;
    const float hcat = any ? -(((sR[4] + sR[5]) + sR[6]) + sR[7]) : 0.f;
    const float mu = sR[0], sraw = sR[1], ls = fminf(fmaxf(sraw, -4.f), 1.f);
    const bool kv = k >= 0 && sL[kk] > ninf;                  // the stored node is alive -- under the mask: a candidate, sL says both
    const float t = (stored[src * 2 + 1] - mu) / expf(ls);
    const float lp = (kv ? sL[kk] - lse : 0.f) + (-0.5f * t * t - ls - 0.9189385f);   // 0.5 log(2 pi)
    const float H = ((hcat + ls) + 0.5f) + 0.9189385f;
    float* pr = ps.prow + (size_t)i * 8;
    pr[0] = lp; pr[1] = H; pr[2] = hcat; pr[3] = mu; pr[4] = sraw; pr[5] = (float)k; pr[6] = kv ? 1.f : 0.f; pr[7] = t;
    if (out.logp) out.logp[i] = lp;
    if (out.entropy) out.entropy[i] = H;
    if (out.charge_mean) out.charge_mean[i] = mu;
    if (out.charge_log_std) out.charge_log_std[i] = ls;
}

__global__ void __launch_bounds__(256) wrsn_etp_loss_kernel(WrsnEtGroups gs, int n, WrsnEtHyper hp, WrsnEtScratch s0, WrsnEtpScratch ps) {
    wrsn_et_loss_body<true>(gs, n, hp, s0, ps.prow + (size_t)blockIdx.x * ps.chunk);   // one block per group
}

__global__ void __launch_bounds__(256) wrsn_etp_score_bwd_kernel(WrsnEtGroups gs, WrsnEtDims dm, WrsnEtScratch s0, WrsnEtpScratch ps0) {
    extern __shared__ double smem[];
    float* sW = (float*)smem;
    float* sP = sW + WRSN_ETP_S_PART;                          // [4 waves][64 units], then dq [64]
    float* sDq = sP + 256;
    float* sDL = sW + WRSN_ETP_B_DL;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    const WrsnEtpWho who = wrsn_etp_who(gs, dm);
    const float* blk = who.blk;
    const WrsnEtScratch s = wrsn_et_slice(s0, who.grp);
    const WrsnEtpScratch ps = wrsn_etp_slice(ps0, who.grp);
    const int N = dm.N, i = who.i;
    {
        const auto g = wrsn_global((const WrsnU4*)blk);
        WrsnU4* dst = (WrsnU4*)sW;
        for (int j = tid; j < WRSN_EP_MC1 / 4; j += 256) dst[j] = wrsn_ld_u4(g + j);
    }
    const float ninf = -__builtin_inff();
    const float* pr = ps.prow + (size_t)i * 8;
    const float a = s.dout[(size_t)i * 8], e = s.dout[(size_t)i * 8 + 1];   // d loss / d logp, d loss / d H
    const float hcat = pr[2], sraw = pr[4], t = pr[7];
    const int k = (int)pr[5];
    const bool kv = pr[6] == 1.f;
    // ---- dl_i = a ([kv, i = k] - [kv] p_i) - e p_i (log p_i + H_cat) over the alive nodes, zero elsewhere: in place of log p
    float* lrow = ps.lp + (size_t)i * ps.ld;
    for (int n = tid; n < ps.ld; n += 256) {
        const float lp = lrow[n];
        float dl = 0.f;
        if (lp > ninf) {
            const float p = expf(lp);
            dl = a * (((kv && n == k) ? 1.f : 0.f) - (kv ? p : 0.f)) - e * p * (lp + hcat);
        }
        sDL[n] = dl; lrow[n] = dl;
    }
    __syncthreads();
    // ---- dq_u = 0.125 sum_i dl_i h_{i,u}: the tile's 32 columns folded, the wave's tiles in tile order, the four waves in wave order
    float acc[2] = {0.f, 0.f};
    const float* nrow = who.row;
    const int ntile = (N + 31) >> 5;
    for (int tile = wave; tile < ((ntile + 3) & ~3); tile += 4) {   // every wave the same number of rounds: the folds are exchanges
        const bool on = tile < ntile;
        float x[4]; wrsn_v16f h1[2], h2[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) h2[t2][r] = 0.f;
        if (on) (void)wrsn_et_tile_fwd(sW, nrow, N, tile, col, h, x, h1, h2);
        const float dl = on ? sDL[tile * 32 + col] : 0.f;     // zero beyond N and for nodes that are not alive
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = dl * h2[t2][r];
            acc[t2] += wrsn_ep_fold16<false>(v, lane);
        }
    }
    if ((lane & 16) == 0) {
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) sP[64 * wave + 32 * t2 + wrsn_ep_unit(lane & 15, h)] = acc[t2];
    }
    __syncthreads();
    if (tid < 64) {
        const float dq = 0.125f * (((sP[tid] + sP[64 + tid]) + sP[128 + tid]) + sP[192 + tid]);
        sDq[tid] = dq; ps.dq[(size_t)i * 64 + tid] = dq;
    }
    // ---- the charge head: dmu = a t / exp(s), ds_raw = [-4 <= s_raw <= 1] (a (t^2 - 1) + e)
    const float ls = fminf(fmaxf(sraw, -4.f), 1.f);
    const float dmu = a * t / expf(ls);
    const float ds = (sraw >= -4.f && sraw <= 1.f) ? a * (t * t - 1.f) + e : 0.f;
    if (tid == 0) { ps.dch[(size_t)i * 2] = dmu; ps.dch[(size_t)i * 2 + 1] = ds; }
    __syncthreads();
    // ---- dz = W_charge[0:128] (dmu, ds_raw) + W_query dq: thread u reads row u of the [in, out] weights; head2's ReLU gates it in the head backward
    if (tid < 128) {
        const float* wq = blk + WRSN_PP_QUERY + 64 * tid;
        float a0 = blk[WRSN_PP_CHARGE + 2 * tid] * dmu, a1 = blk[WRSN_PP_CHARGE + 2 * tid + 1] * ds, a2 = 0.f, a3 = 0.f;
#pragma unroll 4
        for (int j = 0; j < 64; j += 4) {
            a0 = fmaf(wq[j], sDq[j], a0); a1 = fmaf(wq[j + 1], sDq[j + 1], a1); a2 = fmaf(wq[j + 2], sDq[j + 2], a2); a3 = fmaf(wq[j + 3], sDq[j + 3], a3);
        }
        s.dz2[(size_t)i * 128 + tid] = (a0 + a1) + (a2 + a3);
    }
}

__global__ void __launch_bounds__(256) wrsn_etp_head_bwd_kernel(WrsnEtGroups gs, int n, WrsnEtScratch s0) {
    wrsn_et_head_bwd_body<true>(gs, n, s0);
}

// The second pass of the trunk backward, for the actor's rows (block index = group * n + row).  The trunk's gradient is linear in delta2, so the term the
// scores add, delta2 = relu' 0.125 dl_i q_u, goes through wrsn_et_trunk_bwd_kernel's tiles on its own: that kernel holds 256 VGPRs and 250
// AGPRs and one more addend in it spills.  node1 / node2 and their biases only -- the scores do not see the chargers -- into ps.part2; the
// reduce adds the two partials.  The tile loop and the wave sum are that kernel's, statement for statement.
__global__ void __launch_bounds__(256) wrsn_etp_trunk_bwd_kernel(WrsnEtGroups gs, WrsnEtDims dm, WrsnEtScratch s0, WrsnEtpScratch ps0) {
    extern __shared__ double smem[];
    float* sT = (float*)smem;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    const WrsnEtpWho who = wrsn_etp_who(gs, dm);
    const float* blk = who.blk;
    const WrsnEtpScratch ps = wrsn_etp_slice(ps0, who.grp);
    const int N = dm.N;
    float* sA = sT + wave * 4096;                             // h1 of the wave's tile [node][unit], later delta1
    float* sB = sA + 2048;                                    // delta2 [node][unit], later x [node][8]
    const float* q = ps.q + (size_t)who.i * 64;
    wrsn_v16f dW2[2][2], dW1[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { dW2[0][0][r] = 0.f; dW2[0][1][r] = 0.f; dW2[1][0][r] = 0.f; dW2[1][1][r] = 0.f; dW1[0][r] = 0.f; dW1[1][r] = 0.f; }
    float db1 = 0.f, db2 = 0.f;                               // lane = unit
    const float* nrow = who.row;
    const int ntile = (N + 31) >> 5;
    for (int tile = wave; tile < ((ntile + 3) & ~3); tile += 4) {   // every wave the same number of rounds: the block meets at every exchange
        const bool on = tile < ntile;
        float x[4] = {0.f, 0.f, 0.f, 0.f}; wrsn_v16f h1[2], h2[2], d2[2], d1[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) { h1[t][r] = 0.f; h2[t][r] = 0.f; d1[t][r] = 0.f; }
        if (on) (void)wrsn_et_tile_fwd(blk, nrow, N, tile, col, h, x, h1, h2);
        const int nd0 = tile * 32 + col;
        const float dlq = (on && nd0 < N) ? 0.125f * ps.lp[(size_t)who.i * ps.ld + nd0] : 0.f;   // 0.125 d loss / d l of the lane's node
        // delta2 = relu' 0.125 dl_i q_u; h2 > 0 only where the node is alive
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int u = 32 * t2 + wrsn_ep_unit(r, h);
                const float g = dlq * q[u];
                d2[t2][r] = h2[t2][r] > 0.f ? g : 0.f;
            }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int u = 32 * t + wrsn_ep_unit(r, h);
                sA[WRSN_ET_TILE(col, u)] = h1[t][r]; sB[WRSN_ET_TILE(col, u)] = d2[t][r];
            }
        if (on) {                                             // delta1 = relu' (W2 delta2): register r of delta2[t2] is the k-pair (u, u + 4)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                wrsn_v16f acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(blk[WRSN_EP_NODE2 + (32 * t + col) * 64 + 32 * t2 + wrsn_ep_unit(r, h)], d2[t2][r], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) d1[t][r] = h1[t][r] > 0.f ? acc[r] : 0.f;
            }
        }
        __syncthreads();
        if (on) {                                             // dW2[i][j] += sum over the tile's nodes of h1[node][i] delta2[node][j]
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll 4
                    for (int kk = 0; kk < 16; ++kk) {
                        const int nd = 2 * kk + h;
                        dW2[t][t2] = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[WRSN_ET_TILE(nd, 32 * t + col)], sB[WRSN_ET_TILE(nd, 32 * t2 + col)], dW2[t][t2], 0, 0, 0);
                    }
            for (int nd = 0; nd < 32; ++nd) db2 += sB[WRSN_ET_TILE(nd, lane)];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) sA[WRSN_ET_TILE(col, 32 * t + wrsn_ep_unit(r, h))] = d1[t][r];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) sB[col * WRSN_ENT_NODE_F + 2 * kk + h] = x[kk];
        __syncthreads();
        if (on) {                                             // dW1[f][j] += sum over the tile's nodes of x[node][f] delta1[node][j]: rows f < 8 of D
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll 4
                for (int kk = 0; kk < 16; ++kk) {
                    const int nd = 2 * kk + h;
                    dW1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(col < WRSN_ENT_NODE_F ? sB[nd * WRSN_ENT_NODE_F + col] : 0.f, sA[WRSN_ET_TILE(nd, 32 * t + col)], dW1[t], 0, 0, 0);
                }
            for (int nd = 0; nd < 32; ++nd) db1 += sA[WRSN_ET_TILE(nd, lane)];
        }
        __syncthreads();
    }
    // ---- the four waves, added in wave order: dW2, then dW1 and the two biases
    float* part = ps.part2 + (size_t)who.i * WRSN_EP_MC1;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) sT[wave * 4096 + (32 * t + wrsn_ep_unit(r, h)) * 64 + 32 * t2 + col] = dW2[t][t2][r];
    __syncthreads();
    for (int i = tid; i < 4096; i += 256) part[WRSN_EP_NODE2 + i] = ((sT[i] + sT[4096 + i]) + sT[8192 + i]) + sT[12288 + i];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) sT[wave * 768 + wrsn_ep_unit(r, h) * 64 + 32 * t + col] = dW1[t][r];
    sT[wave * 768 + 512 + lane] = db1; sT[wave * 768 + 576 + lane] = db2;
    __syncthreads();
    for (int i = tid; i < 640; i += 256) {
        const float v = ((sT[i] + sT[768 + i]) + sT[1536 + i]) + sT[2304 + i];
        part[i < 512 ? WRSN_EP_NODE1 + i : i < 576 ? WRSN_EP_NODE1_B + i - 512 : WRSN_EP_NODE2_B + i - 576] = v;
    }
}

__global__ void __launch_bounds__(256) wrsn_etp_reduce_kernel(WrsnEtGroups gs, WrsnEtDims dm, WrsnEtScratch s0, WrsnEtpScratch ps) {
    const int grp = ((int)blockIdx.x / ((WRSN_PP_FLOATS + 255) / 256)) >> 1;   // the body's own split: (group * 2 + net) * (blocks per net) + ...
    wrsn_et_reduce_body<true>(gs, dm.n, s0, wrsn_etp_slice(ps, grp), dm.N, dm.M);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Behaviour cloning (wrsn_entity_pointer_bc_grad, _bc_grad_multi, _bc_update): loss = -mean(logp) - ent_coef mean(H) of the stored pairs,
// the actor alone.  Every kernel above is launched as it stands on a group table WITHOUT critics: the forward kernels skip a net that is
// not given, the per-row pointer kernels serve the actor anyway (G * n blocks), and the three that index (group, net) by the block --
// head backward, trunk backward, reduce -- are launched once per group on that group's entry and slice, with the actor half of the grid
// only (block index / n == 0: group 0, net 0).  New is this loss kernel, one block per group in the place of wrsn_etp_loss_kernel:
//   dout[0] = -inv_n, dout[1] = -ent_coef inv_n, the other six slots zero (the value slot among them) -- the floats wrsn_et_loss_body
//   writes for ratio 1, advantage 1 and equal terms under the max, so the backward kernels produce the PPO call's bytes from them;
//   stats[0..7] = loss, -mean(logp), -mean over the rows with kv of the node term, -mean of the Gaussian term, mean(H), top-1 (the share
//   of the rows with kv whose stored node attains the row's largest node_logp, ties are hits), the share of rows with kv, 0.  The two
//   means over "rows with kv" divide by THEIR count (0 when there is none).  node_logp is read from the lp rows the score forward left
//   in the scratch, before the score backward overwrites them; the row maximum is taken by a wave per row (exact, so no order enters).
// Sums in double through wrsn_et_block_sum: thread t takes rows t, t + 256, ...; no float atomics.
__global__ void __launch_bounds__(256) wrsn_etp_bc_loss_kernel(WrsnEtGroups gs, int n, int N, float ent_coef, WrsnEtScratch s0, WrsnEtpScratch ps0) {
    extern __shared__ double smem[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = (int)blockIdx.x;   // one block per group
    float* stats = gs.g[grp].stats;
    const WrsnEtScratch s = wrsn_et_slice(s0, grp);
    const WrsnEtpScratch ps = wrsn_etp_slice(ps0, grp);
    const float ninf = -__builtin_inff();
    const float inv_n = 1.f / (float)n;
    double a_lp = 0.0, a_node = 0.0, a_g = 0.0, a_h = 0.0, a_kv = 0.0, a_hit = 0.0;
    for (int i = tid; i < n; i += 256) {
        const float* pr = ps.prow + (size_t)i * 8;
        float* dout = s.dout + (size_t)i * 8;
        const float sraw = pr[4], t = pr[7], ls = fminf(fmaxf(sraw, -4.f), 1.f);
        const int k = (int)pr[5];
        const bool kv = pr[6] == 1.f;
        a_lp += (double)pr[0]; a_h += (double)pr[1];
        a_g += (double)(-0.5f * t * t - ls - 0.9189385f);     // the Gaussian term as the score kernel forms it
        if (kv) { a_node += (double)ps.lp[(size_t)i * ps.ld + k]; a_kv += 1.0; }
        dout[0] = -inv_n; dout[1] = -ent_coef * inv_n; dout[2] = 0.f; dout[3] = 0.f; dout[4] = 0.f; dout[5] = 0.f; dout[6] = 0.f; dout[7] = 0.f;
    }
    for (int i = wave; i < n; i += 4) {                       // wave-uniform: the row's largest node_logp, lanes by a butterfly
        const float* lrow = ps.lp + (size_t)i * ps.ld;
        float mx = ninf;
        for (int j = lane; j < N; j += 64) { const float l = lrow[j]; mx = l > mx ? l : mx; }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const float o = __shfl_xor(mx, d); mx = o > mx ? o : mx; }
        const float* pr = ps.prow + (size_t)i * 8;
        const int k = (int)pr[5];
        if (lane == 0 && pr[6] == 1.f && lrow[k] >= mx) a_hit += 1.0;
    }
    const double lp = wrsn_et_block_sum(a_lp, smem, tid) / n, en = wrsn_et_block_sum(a_h, smem, tid) / n, ga = wrsn_et_block_sum(a_g, smem, tid) / n;
    const double nd = wrsn_et_block_sum(a_node, smem, tid), kc = wrsn_et_block_sum(a_kv, smem, tid), hit = wrsn_et_block_sum(a_hit, smem, tid);
    if (tid == 0) {
        stats[0] = (float)(-lp - (double)ent_coef * en);
        stats[1] = (float)(-lp); stats[2] = kc > 0.0 ? (float)(-nd / kc) : 0.f; stats[3] = (float)(-ga); stats[4] = (float)en;
        stats[5] = kc > 0.0 ? (float)(hit / kc) : 0.f; stats[6] = (float)(kc / n); stats[7] = 0.f;
    }
}
