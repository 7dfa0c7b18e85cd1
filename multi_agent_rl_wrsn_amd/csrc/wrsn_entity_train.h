// wrsn_entity_train.h -- the PPO update of the entity policy on the device (gfx950): wrsn_entity_eval, wrsn_entity_ppo_grad,
// wrsn_entity_adam and their multi-group forms wrsn_entity_ppo_grad_multi, wrsn_entity_adam_multi, wrsn_entity_ppo_update of
// include/wrsn_hip.h.  Every kernel serves G groups (WrsnEtGroups below) in one launch; the single-group calls are G = 1.  At the end of
// the file: wrsn_entity_prepare, the batch preparation (values, GAE, gathers) on the same forward kernels.
//
// One minibatch step of PPOLearner.update for the set networks of build_entity_networks (ippo.py) on packed entity rows
// (R = 8 N + 12 M + 8 floats, as the transition buffers store them), an actor block (wrsn_entity_act's layout) and a critic block (the same
// trunk offsets, `value` 128 -> 1 behind head2's bias).  Every group's two nets go through every kernel together: block index = (group * 2 + net) * (blocks per net) + ...
//   wrsn_et_trunk_fwd_kernel   one 256-thread block per (row, net): the trunk of wrsn_entpol_trunk_kernel restated on a packed row --
//                              the same MFMA chains, folds, tile and wave order, so the 200 features are its features bit for bit --
//                              plus the live count and, per pooled unit, the lowest-index node that attains the maximum
//   wrsn_et_head_fwd_kernel    tiles of <= 32 rows: head1, head2 on the matrix cores as wrsn_entpol_head_kernel, the six (actor) or one
//                              (critic) last dot products in four chains; keeps head1's and head2's outputs and the raw outputs
//   wrsn_et_loss_kernel        one block per group: the loss of PPOLearner.minibatch_loss, its statistics, d loss / d (mean, log_std, value) per row
//   wrsn_et_head_bwd_kernel    one block per (row, net): back through the last layers, head2 and head1 on the VALU (a row is a
//                              128-vector: 42 k multiply-adds) -> d / d features
//   wrsn_et_trunk_bwd_kernel   one block per (row, net): per 32-node tile h1, h2 recomputed exactly as the forward does, delta2 from the two
//                              pools, delta1 = relu' (W2 delta2), dW2 = sum_nodes h1 delta2^T and dW1 = sum_nodes x delta1^T on the matrix
//                              cores, the charger MLP on the VALU; per-row partial gradients of the trunk to scratch
//   wrsn_et_reduce_kernel      one thread per float of a gradient block: trunk partials summed over the rows in index order; the weight
//                              gradients of head1, head2 and the last layers as sums over the rows of (input x delta) in index order
//   wrsn_et_norm_kernel / wrsn_et_adam_kernel   clip_grad_norm_ and torch.optim.Adam on up to 16 blocks (WrsnEtAdamBlocks), each clipped by its own norm
// Orientation of the matrix products: that of wrsn_rollout.h, D[i][j] = sum_k A[k][i] B[k][j] with v_mfma_f32_32x32x2_f32, units in D's rows and
// nodes in D's columns.  delta2 in accumulator layout is a B operand as it stands (k-pair (u, u + 4)), so delta1 needs no exchange; its A
// operand is W2 read along its rows.  dW2 and dW1 contract over the NODES, which the accumulators hold in lanes: h1, delta2 (then delta1, x) of a
// wave's tile go through LDS as [node][unit] -- A = h1[node 2 kk + h][unit], B = delta2[node 2 kk + h][unit] -- with the unit index XOR-ed
// by the node so that neither the column-wise stores nor the row-wise loads meet in a bank.  16 KB per wave, 64 KB per block: the
// weights are read from global memory (19 KB per net: L1-resident) in the backward, from LDS in the forward.
// Every sum has a fixed order: MFMA chains are k-ordered, a wave adds its tiles in tile order, the four waves are added in wave order,
// rows in index order; block sums are trees over a fixed thread-to-row map.  No float atomics.  Two calls on equal inputs give equal bytes.
#pragma once
#include <stdint.h>
#include "wrsn_rollout.h"

// The critic block: the trunk at the actor's offsets, then value [128][1] and its bias, zeros up to a multiple of 4
#define WRSN_EC_VALUE WRSN_EP_MEAN
#define WRSN_EC_VALUE_B (WRSN_EC_VALUE + 128)
#define WRSN_EC_FLOATS ((WRSN_EC_VALUE_B + 1 + 3) / 4 * 4)
static_assert(WRSN_EC_VALUE == 48448 && WRSN_EC_VALUE_B == 48576 && WRSN_EC_FLOATS == 48580, "the layout documented in include/wrsn_hip.h");
#define WRSN_ET_TRUNK_FLOATS WRSN_EP_HEAD1                    // node1, node2, mc1, mc2 with their biases: what a row's partial gradient holds
// LDS of the forward trunk: that of wrsn_entpol_trunk_kernel, then the 64 maxima and the arg-max candidates of the four waves
#define WRSN_ET_T_MX (WRSN_EP_T_G2 + 256)
#define WRSN_ET_T_ARG (WRSN_ET_T_MX + 64)
#define WRSN_ET_T_LDS ((WRSN_ET_T_ARG + 256) * 4)             // bytes
#define WRSN_ET_B_LDS (4 * 4096 * 4)                          // bytes: two [32 nodes][64 units] tiles per wave
#define WRSN_ET_TILE(n_, u_) ((n_) * 64 + ((u_) ^ (n_)))      // [node < 32][unit < 64], bank-swizzled

struct WrsnEtDims { int n, N, M; };                           // rows of the minibatch, nodes and chargers of a row: common to the groups of a call
struct WrsnEtBatch { const float* action; const float* logp_old; const float* advantage; const float* ret; const float* value_old; };
struct WrsnEtHyper { float clip, ent_coef, vf_coef; int norm_adv, clip_vloss; };
// A GROUP: one (actor, critic) pair with its rows, batch and outputs (wrsn_entity_group of include/wrsn_hip.h; the single-group calls are
// one group).  The groups of a call reach every kernel as ONE by-value argument: the block index carries the group,
// (group * 2 + net) * (blocks per net) + ..., and a block picks its entry by that wave-uniform index -- scalar loads from the kernel-argument
// segment, no vector register, no scratch (profiles/entity_update_joint_kernel_resource_usage.csv).  Group g's slice of the scratch area
// lies g * `chunk` floats behind group 0's.
struct WrsnEtGroup {
    const float* actor; const float* critic; float* grad_actor; float* grad_critic;
    const float* rows; const int32_t* index; WrsnEtBatch b; float* stats;
};
// 2 * WRSN_MAX_MC entries: the update calls fill at most WRSN_MAX_MC; wrsn_entity_prepare fills two per group (below)
#define WRSN_ET_MAX_GROUPS (2 * WRSN_MAX_MC)
struct WrsnEtGroups { WrsnEtGroup g[WRSN_ET_MAX_GROUPS]; };
// the blocks of an Adam call: at most an actor and a critic per group
struct WrsnEtAdamBlock { float* p; const float* g; float* m; float* v; float* norm_out; int nf; float step_size, inv_sqrt_bc2; };
struct WrsnEtAdamBlocks { WrsnEtAdamBlock b[2 * WRSN_MAX_MC]; };
// scratch of one group, [2 nets][n rows] each unless stated
struct WrsnEtScratch {
    float* feat;    // [.][200] head inputs
    float* arg;     // [.][64]  node index (as a float) the max pool of the unit took, -1: none (maximum 0)
    float* cnt;     // [.]      live nodes
    float* z1;      // [.][128] head1 output (after ReLU)
    float* z2;      // [.][128] head2 output (after ReLU)
    float* dz1;     // [.][128] d loss / d head1 pre-activation
    float* dz2;     // [.][128] d loss / d head2 pre-activation
    float* dfeat;   // [.][200]
    float* part;    // [.][WRSN_ET_TRUNK_FLOATS] a row's gradient of the trunk's first four layers
    float* raw;     // [n][8] mean 3, log_std before the clamp 3, value, 0
    float* dout;    // [n][8] d loss / d of those
    size_t chunk;   // floats from a group's slice to the next group's
};
// group g's slice
WDEV WrsnEtScratch wrsn_et_slice(WrsnEtScratch s, int g) {
    const size_t o = (size_t)g * s.chunk;
    s.feat += o; s.arg += o; s.cnt += o; s.z1 += o; s.z2 += o; s.dz1 += o; s.dz2 += o; s.dfeat += o; s.part += o; s.raw += o; s.dout += o;
    return s;
}

// what the node-pointer update (wrsn_entity_pointer_train.h) keeps per row next to the above; null in every call of the set policy
struct WrsnEtpScratch {
    float* q;       // [n][64]  query(z)
    float* lp;      // [n][ld]  log-probability of every node (-inf: not alive), then d loss / d l in place
    float* prow;    // [n][8]   logp, H, H_cat, mu, s_raw, the validated node (-1: none) as a float, [it is alive], t = (x - mu) / exp(s)
    float* dq;      // [n][64]  d loss / d q
    float* dch;     // [n][2]   d loss / d (mu, s_raw)
    float* part2;   // [n][WRSN_EP_MC1] the row's gradient of node1 / node2 through the scores
    int ld;         // floats per row of lp: N rounded up to whole tiles
    size_t chunk;   // floats from a group's slice to the next group's (as WrsnEtScratch::chunk)
};

static inline size_t wrsn_et_scratch_floats(size_t n, bool grad) {   // host
    return 2 * n * (WRSN_ENTPOL_FEAT + 64 + 4 + 128 + 128) + 8 * n + (grad ? 2 * n * (128 + 128 + WRSN_ENTPOL_FEAT + WRSN_ET_TRUNK_FLOATS) + 8 * n : 0);
}

// h1 (after ReLU) and h2 (after ReLU, zero unless the node is alive) of the 32 nodes of `tile` in accumulator layout, and the node's masked
// inputs x: wrsn_entpol_trunk_kernel's arithmetic, operation for operation.  W: the block's first WRSN_EP_MC1 floats (LDS or global).
WDEV bool wrsn_et_tile_fwd(const float* W, const float* nrow, int N, int tile, int col, int h, float (&x)[4], wrsn_v16f (&h1)[2], wrsn_v16f (&h2)[2]) {
    const int n = tile * 32 + col, srcn = n < N ? n : N - 1;
    const auto p = wrsn_global((const WrsnU4*)(nrow + (size_t)srcn * WRSN_ENT_NODE_F));
    const WrsnU4 c0 = wrsn_ld_u4(p), c1 = wrsn_ld_u4(p + 1);
    const bool alive = n < N && __int_as_float((int)c1.w) == 1.f;
    x[0] = __int_as_float((int)(h ? c0.y : c0.x)); x[1] = __int_as_float((int)(h ? c0.w : c0.z));
    x[2] = __int_as_float((int)(h ? c1.y : c1.x)); x[3] = __int_as_float((int)(h ? c1.w : c1.z));
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) x[kk] = alive ? x[kk] : 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        wrsn_v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = W[WRSN_EP_NODE1_B + 32 * t + wrsn_ep_unit(r, h)];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(W[WRSN_EP_NODE1 + (2 * kk + h) * 64 + 32 * t + col], x[kk], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) h1[t][r] = fmaxf(acc[r], 0.f);
    }
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
        wrsn_v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = W[WRSN_EP_NODE2_B + 32 * t2 + wrsn_ep_unit(r, h)];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(W[WRSN_EP_NODE2 + (32 * t + wrsn_ep_unit(r, h)) * 64 + 32 * t2 + col], h1[t][r], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) h2[t2][r] = alive ? fmaxf(acc[r], 0.f) : 0.f;
    }
    return alive;
}

// which (group, net, row) a block of the per-row kernels is, and where its packed row lies
struct WrsnEtWho { int grp, net, i; const float* blk; const float* row; };
WDEV WrsnEtWho wrsn_et_who(const WrsnEtGroups& gs, const WrsnEtDims& dm) {
    WrsnEtWho w;
    const int q = (int)blockIdx.x / dm.n;                     // group * 2 + net
    w.i = (int)blockIdx.x - q * dm.n; w.grp = q >> 1; w.net = q & 1;
    const WrsnEtGroup& G = gs.g[w.grp];
    w.blk = w.net ? G.critic : G.actor;
    const int32_t* index = G.index;
    const int src = index ? wrsn_wave_first(index[w.i]) : w.i;
    w.row = G.rows + (size_t)src * (size_t)(WRSN_ENT_NODE_F * dm.N + WRSN_ENT_MC_F * dm.M + WRSN_ENT_ENV_F);
    return w;
}

__global__ void __launch_bounds__(256) wrsn_et_trunk_fwd_kernel(WrsnEtGroups gs, WrsnEtDims dm, WrsnEtScratch s0) {
    extern __shared__ double smem[];
    float* sW = (float*)smem;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    const WrsnEtWho who = wrsn_et_who(gs, dm);
    const float* blk = who.blk;
    if (!blk) return;                                         // block-uniform: this net is not asked for
    const WrsnEtScratch s = wrsn_et_slice(s0, who.grp);
    const int N = dm.N, M = dm.M;
    const size_t base = (size_t)who.net * dm.n + who.i;
    {
        const auto src = wrsn_global((const WrsnU4*)blk);
        WrsnU4* dst = (WrsnU4*)sW;
        for (int i = tid; i < WRSN_EP_MC1 / 4; i += 256) dst[i] = wrsn_ld_u4(src + i);
    }
    __syncthreads();
    float psum[2] = {0.f, 0.f}, pmax[2] = {0.f, 0.f}, cnt = 0.f;
    float bmv[2][16], bmi[2][16];                             // per register: the largest value this lane's nodes gave, and the first node that gave it
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int r = 0; r < 16; ++r) { bmv[t2][r] = 0.f; bmi[t2][r] = -1.f; }
    const float* nrow = who.row;
    const int ntile = (N + 31) >> 5;
    for (int tile = wave; tile < ((ntile + 3) & ~3); tile += 4) {   // every wave the same number of rounds: the folds are exchanges
        const bool on = tile < ntile;
        float x[4]; wrsn_v16f h1[2], h2[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) h2[t2][r] = 0.f;
        bool alive = false;
        if (on) alive = wrsn_et_tile_fwd(sW, nrow, N, tile, col, h, x, h1, h2);
        const float nf = (float)(tile * 32 + col);
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
            float v[16], w[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                v[r] = h2[t2][r]; w[r] = v[r];
                if (v[r] > bmv[t2][r]) { bmv[t2][r] = v[r]; bmi[t2][r] = nf; }
            }
            psum[t2] += wrsn_ep_fold16<false>(v, lane);
            pmax[t2] = fmaxf(pmax[t2], wrsn_ep_fold16<true>(w, lane));
        }
        cnt += (on && alive) ? 1.f : 0.f;
    }
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
    const float* mrow = who.row + (size_t)N * WRSN_ENT_NODE_F;
    const float* erow = mrow + (size_t)M * WRSN_ENT_MC_F;
    const int c = tid >> 5, o = tid & 31;
    if (c < M) {
        float a = blk[WRSN_EP_MC1_B + o];
#pragma unroll
        for (int k = 0; k < WRSN_ENT_MC_F; ++k) a = fmaf(mrow[c * WRSN_ENT_MC_F + k], blk[WRSN_EP_MC1 + k * 32 + o], a);
        sW[WRSN_EP_T_G1 + tid] = fmaxf(a, 0.f);
    }
    __syncthreads();
    if (c < M) {
        float a = blk[WRSN_EP_MC2_B + o];
#pragma unroll 8
        for (int k = 0; k < 32; ++k) a = fmaf(sW[WRSN_EP_T_G1 + 32 * c + k], blk[WRSN_EP_MC2 + k * 32 + o], a);
        sW[WRSN_EP_T_G2 + tid] = fmaxf(a, 0.f);
    }
    __syncthreads();
    float* frow = s.feat + base * WRSN_ENTPOL_FEAT;
    if (tid < 64) {
        const float n_alive = ((sW[WRSN_EP_T_CNT] + sW[WRSN_EP_T_CNT + 1]) + sW[WRSN_EP_T_CNT + 2]) + sW[WRSN_EP_T_CNT + 3];
        const float sum = ((sW[WRSN_EP_T_SUM + tid] + sW[WRSN_EP_T_SUM + 64 + tid]) + sW[WRSN_EP_T_SUM + 128 + tid]) + sW[WRSN_EP_T_SUM + 192 + tid];
        const float mx = fmaxf(fmaxf(sW[WRSN_EP_T_MAX + tid], sW[WRSN_EP_T_MAX + 64 + tid]), fmaxf(sW[WRSN_EP_T_MAX + 128 + tid], sW[WRSN_EP_T_MAX + 192 + tid]));
        frow[tid] = sum / fmaxf(n_alive, 1.f);
        frow[64 + tid] = mx;
        sW[WRSN_ET_T_MX + tid] = mx;
        if (tid == 0) s.cnt[base] = n_alive;
    } else if (tid < 96) {
        const int u = tid - 64;
        float sa = 0.f, so = 0.f, na = 0.f;
        for (int k = 0; k < M; ++k) {
            const float g = sW[WRSN_EP_T_G2 + 32 * k + u];
            const bool al = mrow[k * WRSN_ENT_MC_F + 4] == 1.f, self = mrow[k * WRSN_ENT_MC_F + 3] == 1.f;
            sa += al ? g : 0.f; na += al ? 1.f : 0.f; so += self ? g : 0.f;
        }
        frow[128 + u] = sa / fmaxf(na, 1.f);
        frow[160 + u] = so;
    } else if (tid < 104) {
        const int k = tid - 96;
        const float v = erow[k];
        frow[192 + k] = k == 4 ? v * (1.f / (float)M) : k == 5 ? v * (1.f / (float)(N > 1 ? N : 1)) : v;
    }
    __syncthreads();
    // ---- the arg-max of every pooled unit: the lowest node index among the lanes whose best value IS the maximum (none when it is 0)
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
        float cand[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float mx = sW[WRSN_ET_T_MX + 32 * t2 + wrsn_ep_unit(r, h)];
            cand[r] = (bmv[t2][r] > 0.f && bmv[t2][r] == mx) ? -bmi[t2][r] : -3.0e38f;
        }
        const float m = wrsn_ep_fold16<true>(cand, lane);
        if ((lane & 16) == 0) sW[WRSN_ET_T_ARG + 64 * wave + 32 * t2 + wrsn_ep_unit(lane & 15, h)] = m;
    }
    __syncthreads();
    if (tid < 64) {
        const float m = fmaxf(fmaxf(sW[WRSN_ET_T_ARG + tid], sW[WRSN_ET_T_ARG + 64 + tid]), fmaxf(sW[WRSN_ET_T_ARG + 128 + tid], sW[WRSN_ET_T_ARG + 192 + tid]));
        s.arg[base * 64 + tid] = m < -1.0e38f ? -1.f : -m;
    }
}

struct WrsnEtEvalOut { float* mean; float* log_std; float* value; };   // any may be null

__global__ void __launch_bounds__(256) wrsn_et_head_fwd_kernel(WrsnEtGroups gs, int n, WrsnEtScratch s0, WrsnEtEvalOut out) {
    extern __shared__ double smem[];
    float* sF = (float*)smem;
    float* sZ = sF + WRSN_EP_H_Z;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    const int nt = (n + WRSN_EP_HEAD_ROWS - 1) / WRSN_EP_HEAD_ROWS;
    const int q = (int)blockIdx.x / nt, grp = q >> 1, net = q & 1, first = ((int)blockIdx.x - q * nt) * WRSN_EP_HEAD_ROWS;
    const float* blk = net ? gs.g[grp].critic : gs.g[grp].actor;
    if (!blk) return;
    const WrsnEtScratch s = wrsn_et_slice(s0, grp);
    const int rows = n - first < WRSN_EP_HEAD_ROWS ? n - first : WRSN_EP_HEAD_ROWS;
    const size_t base = (size_t)net * n + first;
    for (int i = tid; i < WRSN_EP_HEAD_ROWS * WRSN_ENTPOL_FEAT; i += 256) {   // a column beyond `rows` repeats the last row: computed, not stored
        const int j = i / WRSN_ENTPOL_FEAT, k = i - j * WRSN_ENTPOL_FEAT;
        sF[j * WRSN_EP_H_LD + k] = s.feat[(base + (j < rows ? j : rows - 1)) * WRSN_ENTPOL_FEAT + k];
    }
    __syncthreads();
    {
        wrsn_v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = blk[WRSN_EP_HEAD1_B + 32 * wave + wrsn_ep_unit(r, h)];
        const float* wa = blk + WRSN_EP_HEAD1 + h * 128 + 32 * wave + col;
        const float* xb = sF + col * WRSN_EP_H_LD + h;
#pragma unroll 10
        for (int kk = 0; kk < WRSN_ENTPOL_FEAT / 2; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kk * 256], xb[2 * kk], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int u = 32 * wave + wrsn_ep_unit(r, h);
            const float z = fmaxf(acc[r], 0.f);
            sZ[u * 32 + col] = z;
            if (col < rows) s.z1[(base + col) * 128 + u] = z;
        }
    }
    __syncthreads();
    {
        wrsn_v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = blk[WRSN_EP_HEAD2_B + 32 * wave + wrsn_ep_unit(r, h)];
        const float* wa = blk + WRSN_EP_HEAD2 + h * 128 + 32 * wave + col;
        const float* xb = sZ + h * 32 + col;
#pragma unroll 8
        for (int kk = 0; kk < 64; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kk * 256], xb[kk * 64], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int u = 32 * wave + wrsn_ep_unit(r, h);
            const float z = fmaxf(acc[r], 0.f);
            sF[u * 32 + col] = z;                             // the feature tile is dead
            if (col < rows) s.z2[(base + col) * 128 + u] = z;
        }
    }
    __syncthreads();
    const int nd = net ? 1 : 6;                               // last dot products per column: four k-ordered chains over k mod 4 each
    if (tid < 32 * nd) {
        const int j = tid & 31, d = tid >> 5, st = net ? 1 : 3;
        const float* w = net ? blk + WRSN_EC_VALUE : blk + (d < 3 ? WRSN_EP_MEAN + d : WRSN_EP_LSTD + d - 3);
        float s0 = net ? blk[WRSN_EC_VALUE_B] : d < 3 ? blk[WRSN_EP_MEAN_B + d] : blk[WRSN_EP_LSTD_B + d - 3], s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 4
        for (int k = 0; k < 128; k += 4) {
            s0 = fmaf(sF[k * 32 + j], w[st * k], s0); s1 = fmaf(sF[(k + 1) * 32 + j], w[st * (k + 1)], s1);
            s2 = fmaf(sF[(k + 2) * 32 + j], w[st * (k + 2)], s2); s3 = fmaf(sF[(k + 3) * 32 + j], w[st * (k + 3)], s3);
        }
        sZ[d * 32 + j] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
    if (tid < rows) {
        const size_t e = (size_t)first + tid;
        float* raw = s.raw + e * 8;
        if (net) {
            const float v = sZ[tid];
            raw[6] = v; raw[7] = 0.f;
            if (out.value) out.value[e] = v;
        } else {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float mu = sZ[d * 32 + tid], lr = sZ[(3 + d) * 32 + tid];
                raw[d] = mu; raw[3 + d] = lr;
                if (out.mean) out.mean[e * 3 + d] = mu;
                if (out.log_std) out.log_std[e * 3 + d] = fminf(fmaxf(lr, -4.f), 1.f);
            }
        }
    }
}

// sum of v over the 256 threads of the block: a tree with a fixed shape
WDEV double wrsn_et_block_sum(double v, double* s, int tid) {
    s[tid] = v;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) s[tid] += s[tid + st];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

// PPOLearner.minibatch_loss, statement for statement, and its derivative with respect to the raw outputs.  Thread t takes rows t, t + 256, ...
// PTR: the node-pointer actor -- log-probability and entropy of a row are the two floats the score kernel left in prow, and what goes back is
// d loss / d logp and d loss / d H (dout[0], dout[1]).
template <bool PTR>
WDEV void wrsn_et_loss_body(const WrsnEtGroups& gs, int n, const WrsnEtHyper& hp, const WrsnEtScratch& s0, const float* prow) {
    extern __shared__ double smem[];
    const int tid = (int)threadIdx.x, grp = (int)blockIdx.x;  // one block per group
    const int32_t* index = gs.g[grp].index;
    const WrsnEtBatch b = gs.g[grp].b;
    float* stats = gs.g[grp].stats;
    const WrsnEtScratch s = wrsn_et_slice(s0, grp);
    double mean = 0.0, sd = 1.0;
    if (hp.norm_adv) {
        double a = 0.0;
        for (int i = tid; i < n; i += 256) a += (double)b.advantage[index ? index[i] : i];
        mean = wrsn_et_block_sum(a, smem, tid) / (double)n;
        a = 0.0;
        for (int i = tid; i < n; i += 256) { const double d = (double)b.advantage[index ? index[i] : i] - mean; a += d * d; }
        sd = sqrt(wrsn_et_block_sum(a, smem, tid) / (double)(n - 1));
    }
    const float inv_n = 1.f / (float)n, lo = 1.f - hp.clip, hi = 1.f + hp.clip;
    double a_pg = 0.0, a_v = 0.0, a_h = 0.0, a_kl = 0.0, a_cf = 0.0;
    for (int i = tid; i < n; i += 256) {
        const size_t q = (size_t)(index ? index[i] : i);
        const float* raw = s.raw + (size_t)i * 8;
        float* dout = s.dout + (size_t)i * 8;
        float z[3], sg[3], newlogp = 0.f, H = 0.f;
        bool pass[3];
        if constexpr (PTR) { newlogp = prow[(size_t)i * 8]; H = prow[(size_t)i * 8 + 1]; }
        else {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float lr = raw[3 + d], ls = fminf(fmaxf(lr, -4.f), 1.f);
            pass[d] = lr >= -4.f && lr <= 1.f;
            sg[d] = expf(ls);
            z[d] = (b.action[q * 3 + d] - raw[d]) / sg[d];
            newlogp += -0.5f * z[d] * z[d] - ls;
            H += ls + 1.4189385f;                             // 1/2 + 1/2 log(2 pi)
        }
        newlogp -= 2.7568156f;                                // 1.5 log(2 pi)
        }
        const float lratio = newlogp - b.logp_old[q], ratio = expf(lratio);
        a_kl += (double)expm1f(lratio) - (double)lratio;     // (r - 1) - l without the cancellation in r - 1
        a_cf += fabsf(ratio - 1.f) > hp.clip ? 1.0 : 0.0;
        const float A = hp.norm_adv ? (float)(((double)b.advantage[q] - mean) / (sd + 1e-8)) : b.advantage[q];
        const bool inside = ratio >= lo && ratio <= hi;
        const float t1 = -A * ratio, t2 = -A * fminf(fmaxf(ratio, lo), hi);
        a_pg += (double)fmaxf(t1, t2);
        const float d1 = -A, d2 = inside ? -A : 0.f;         // of two terms under a max the larger counts; equal terms share
        const float dr = t1 > t2 ? d1 : t2 > t1 ? d2 : 0.5f * d1 + 0.5f * d2;
        const float glp = dr * ratio * inv_n;
        if constexpr (PTR) { dout[0] = glp; dout[1] = -hp.ent_coef * inv_n; dout[2] = 0.f; dout[3] = 0.f; dout[4] = 0.f; dout[5] = 0.f; }
        else {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            dout[d] = glp * z[d] / sg[d];
            dout[3 + d] = pass[d] ? glp * (z[d] * z[d] - 1.f) - hp.ent_coef * inv_n : 0.f;
        }
        }
        a_h += (double)H;
        const float v = raw[6], R = b.ret[q], u = v - R;
        float vl = u * u, dv = 2.f * u;
        if (hp.clip_vloss) {
            const float V = b.value_old[q], dvv = v - V;
            const float w = V + fminf(fmaxf(dvv, -hp.clip), hp.clip) - R, wl = w * w;
            const float dw = (dvv >= -hp.clip && dvv <= hp.clip) ? 2.f * w : 0.f;
            dv = vl > wl ? dv : wl > vl ? dw : 0.5f * dv + 0.5f * dw;
            vl = fmaxf(vl, wl);
        }
        a_v += (double)vl;
        dout[6] = hp.vf_coef * 0.5f * dv * inv_n;
        dout[7] = 0.f;
    }
    const double pg = wrsn_et_block_sum(a_pg, smem, tid) / n, vl = 0.5 * wrsn_et_block_sum(a_v, smem, tid) / n;
    const double en = wrsn_et_block_sum(a_h, smem, tid) / n, kl = wrsn_et_block_sum(a_kl, smem, tid) / n, cf = wrsn_et_block_sum(a_cf, smem, tid) / n;
    if (tid == 0) {
        stats[0] = (float)(pg - (double)hp.ent_coef * en + (double)hp.vf_coef * vl);
        stats[1] = (float)pg; stats[2] = (float)vl; stats[3] = (float)en; stats[4] = (float)kl; stats[5] = (float)cf; stats[6] = 0.f; stats[7] = 0.f;
    }
}
__global__ void __launch_bounds__(256) wrsn_et_loss_kernel(WrsnEtGroups gs, int n, WrsnEtHyper hp, WrsnEtScratch s0) {
    wrsn_et_loss_body<false>(gs, n, hp, s0, nullptr);
}

// one block per (row, net): d / d (head2 pre-activation), d / d (head1 pre-activation), d / d features.  Thread k owns unit k and reads
// row k of the [in, out] weights.
// PTR: the actor's d / d (head2 pre-activation) is given (the score backward wrote it to dz2); the critic's rows are as ever.
template <bool PTR>
WDEV void wrsn_et_head_bwd_body(const WrsnEtGroups& gs, int n, const WrsnEtScratch& s0) {
    extern __shared__ double smem[];
    float* sD = (float*)smem;
    const int tid = (int)threadIdx.x;
    const int q = (int)blockIdx.x / n, grp = q >> 1, net = q & 1, i = (int)blockIdx.x - q * n;
    const float* blk = net ? gs.g[grp].critic : gs.g[grp].actor;
    const WrsnEtScratch s = wrsn_et_slice(s0, grp);
    const size_t base = (size_t)net * n + i;
    const float* dout = s.dout + (size_t)i * 8;
    if (tid < 128) {
        float g;
        if (net) g = dout[6] * blk[WRSN_EC_VALUE + tid];
        else if constexpr (PTR) g = s.dz2[base * 128 + tid];
        else {
            g = 0.f;
#pragma unroll
            for (int d = 0; d < 3; ++d) g = fmaf(dout[d], blk[WRSN_EP_MEAN + 3 * tid + d], g);
#pragma unroll
            for (int d = 0; d < 3; ++d) g = fmaf(dout[3 + d], blk[WRSN_EP_LSTD + 3 * tid + d], g);
        }
        g = s.z2[base * 128 + tid] > 0.f ? g : 0.f;
        sD[tid] = g; s.dz2[base * 128 + tid] = g;
    }
    __syncthreads();
    if (tid < 128) {
        const float* w = blk + WRSN_EP_HEAD2 + 128 * tid;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 4
        for (int j = 0; j < 128; j += 4) {
            a0 = fmaf(w[j], sD[j], a0); a1 = fmaf(w[j + 1], sD[j + 1], a1); a2 = fmaf(w[j + 2], sD[j + 2], a2); a3 = fmaf(w[j + 3], sD[j + 3], a3);
        }
        const float g = s.z1[base * 128 + tid] > 0.f ? (a0 + a1) + (a2 + a3) : 0.f;
        sD[128 + tid] = g; s.dz1[base * 128 + tid] = g;
    }
    __syncthreads();
    if (tid < WRSN_ENTPOL_FEAT) {
        const float* w = blk + WRSN_EP_HEAD1 + 128 * tid;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 4
        for (int j = 0; j < 128; j += 4) {
            a0 = fmaf(w[j], sD[128 + j], a0); a1 = fmaf(w[j + 1], sD[129 + j], a1); a2 = fmaf(w[j + 2], sD[130 + j], a2); a3 = fmaf(w[j + 3], sD[131 + j], a3);
        }
        s.dfeat[base * WRSN_ENTPOL_FEAT + tid] = (a0 + a1) + (a2 + a3);
    }
}
__global__ void __launch_bounds__(256) wrsn_et_head_bwd_kernel(WrsnEtGroups gs, int n, WrsnEtScratch s0) {
    wrsn_et_head_bwd_body<false>(gs, n, s0);
}

__global__ void __launch_bounds__(256) wrsn_et_trunk_bwd_kernel(WrsnEtGroups gs, WrsnEtDims dm, WrsnEtScratch s0) {
    extern __shared__ double smem[];
    float* sT = (float*)smem;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    const WrsnEtWho who = wrsn_et_who(gs, dm);
    const float* blk = who.blk;
    const WrsnEtScratch s = wrsn_et_slice(s0, who.grp);
    const int N = dm.N, M = dm.M;
    const size_t base = (size_t)who.net * dm.n + who.i;
    float* sA = sT + wave * 4096;                             // h1 of the wave's tile [node][unit], later delta1
    float* sB = sA + 2048;                                    // delta2 [node][unit], later x [node][8]
    const float* df = s.dfeat + base * WRSN_ENTPOL_FEAT;
    const float* ag = s.arg + base * 64;
    const float live = fmaxf(s.cnt[base], 1.f);
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
        const float nf = (float)(tile * 32 + col);
        // delta2 = relu' alive (d mean / live + d max [node is the arg-max]); h2 > 0 only where the node is alive
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int u = 32 * t2 + wrsn_ep_unit(r, h);
                const float g = df[u] / live + (ag[u] == nf ? df[64 + u] : 0.f);
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
    float* part = s.part + base * WRSN_ET_TRUNK_FLOATS;
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
    __syncthreads();
    // ---- the charger MLP on the VALU: forward as wrsn_et_trunk_fwd_kernel, then back.  Thread (c, o) = unit o of charger c
    float* sG1 = sT; float* sG2 = sT + 256; float* sD1 = sT + 512;
    const float* mrow = who.row + (size_t)N * WRSN_ENT_NODE_F;
    const int c = tid >> 5, o = tid & 31;
    if (c < M) {
        float a = blk[WRSN_EP_MC1_B + o];
#pragma unroll
        for (int k = 0; k < WRSN_ENT_MC_F; ++k) a = fmaf(mrow[c * WRSN_ENT_MC_F + k], blk[WRSN_EP_MC1 + k * 32 + o], a);
        sG1[tid] = fmaxf(a, 0.f);
    }
    __syncthreads();
    {
        float g = 0.f;
        if (c < M) {
            float a = blk[WRSN_EP_MC2_B + o];
#pragma unroll 8
            for (int k = 0; k < 32; ++k) a = fmaf(sG1[32 * c + k], blk[WRSN_EP_MC2 + k * 32 + o], a);
            float na = 0.f;
            for (int k = 0; k < M; ++k) na += mrow[k * WRSN_ENT_MC_F + 4] == 1.f ? 1.f : 0.f;
            const bool al = mrow[c * WRSN_ENT_MC_F + 4] == 1.f, self = mrow[c * WRSN_ENT_MC_F + 3] == 1.f;
            g = (al ? df[128 + o] / fmaxf(na, 1.f) : 0.f) + (self ? df[160 + o] : 0.f);
            g = a > 0.f ? g : 0.f;
        }
        sG2[tid] = g;                                         // d / d (mc2 pre-activation)
    }
    __syncthreads();
    {
        float g = 0.f;
        if (c < M) {
            float a = 0.f;
#pragma unroll 8
            for (int u = 0; u < 32; ++u) a = fmaf(blk[WRSN_EP_MC2 + o * 32 + u], sG2[32 * c + u], a);
            g = sG1[tid] > 0.f ? a : 0.f;
        }
        sD1[tid] = g;                                         // d / d (mc1 pre-activation)
    }
    __syncthreads();
    for (int i = tid; i < 1024; i += 256) {
        const int k = i >> 5, u = i & 31;
        float a = 0.f;
        for (int q = 0; q < M; ++q) a = fmaf(sG1[32 * q + k], sG2[32 * q + u], a);
        part[WRSN_EP_MC2 + i] = a;
    }
    for (int i = tid; i < WRSN_ENT_MC_F * 32; i += 256) {
        const int f = i >> 5, k = i & 31;
        float a = 0.f;
        for (int q = 0; q < M; ++q) a = fmaf(mrow[q * WRSN_ENT_MC_F + f], sD1[32 * q + k], a);
        part[WRSN_EP_MC1 + i] = a;
    }
    if (tid < 32) {
        float a = 0.f, b = 0.f;
        for (int q = 0; q < M; ++q) { a += sD1[32 * q + tid]; b += sG2[32 * q + tid]; }
        part[WRSN_EP_MC1_B + tid] = a; part[WRSN_EP_MC2_B + tid] = b;
    }
}

// one thread per float of a gradient block; rows in index order
// PTR: the actor's block is the node-pointer actor's -- WRSN_PP_FLOATS floats, query and charge behind head2 -- and node1 / node2 add the second partial.
template <bool PTR>
WDEV void wrsn_et_reduce_body(const WrsnEtGroups& gs, int n, const WrsnEtScratch& s0, const WrsnEtpScratch& ps, int dmN, int dmM) {
    const int nb = ((PTR ? WRSN_PP_FLOATS : WRSN_EP_FLOATS) + 255) / 256;
    const int q = (int)blockIdx.x / nb, grp = q >> 1, net = q & 1, p = ((int)blockIdx.x - q * nb) * 256 + (int)threadIdx.x;
    if (p >= (net ? WRSN_EC_FLOATS : PTR ? WRSN_PP_FLOATS : WRSN_EP_FLOATS)) return;
    const WrsnEtScratch s = wrsn_et_slice(s0, grp);
    const size_t b0 = (size_t)net * n;
    float a = 0.f;
    if (p < WRSN_EP_HEAD1) {
        for (int i = 0; i < n; ++i) a += s.part[(b0 + i) * WRSN_ET_TRUNK_FLOATS + p];
        if constexpr (PTR) {
            if (!net && p < WRSN_EP_MC1) {
                float b = 0.f;
                for (int i = 0; i < n; ++i) b += ps.part2[(size_t)i * WRSN_EP_MC1 + p];
                a += b;
            }
        }
    } else if (p < WRSN_EP_HEAD1_B) {
        const int k = (p - WRSN_EP_HEAD1) >> 7, j = (p - WRSN_EP_HEAD1) & 127;
        for (int i = 0; i < n; ++i) a = fmaf(s.feat[(b0 + i) * WRSN_ENTPOL_FEAT + k], s.dz1[(b0 + i) * 128 + j], a);
    } else if (p < WRSN_EP_HEAD2) {
        for (int i = 0; i < n; ++i) a += s.dz1[(b0 + i) * 128 + p - WRSN_EP_HEAD1_B];
    } else if (p < WRSN_EP_HEAD2_B) {
        const int k = (p - WRSN_EP_HEAD2) >> 7, j = (p - WRSN_EP_HEAD2) & 127;
        for (int i = 0; i < n; ++i) a = fmaf(s.z1[(b0 + i) * 128 + k], s.dz2[(b0 + i) * 128 + j], a);
    } else if (p < WRSN_EP_MEAN) {
        for (int i = 0; i < n; ++i) a += s.dz2[(b0 + i) * 128 + p - WRSN_EP_HEAD2_B];
    } else if (net) {
        if (p < WRSN_EC_VALUE_B) { for (int i = 0; i < n; ++i) a = fmaf(s.z2[(b0 + i) * 128 + p - WRSN_EC_VALUE], s.dout[(size_t)i * 8 + 6], a); }
        else if (p == WRSN_EC_VALUE_B) { for (int i = 0; i < n; ++i) a += s.dout[(size_t)i * 8 + 6]; }
    } else if constexpr (PTR) {
        if (p < WRSN_PP_QUERY_B) {                            // query: z x dq
            const int k = (p - WRSN_PP_QUERY) >> 6, j = (p - WRSN_PP_QUERY) & 63;
            for (int i = 0; i < n; ++i) a = fmaf(s.z2[(b0 + i) * 128 + k], ps.dq[(size_t)i * 64 + j], a);
        } else if (p < WRSN_PP_CHARGE) {
            for (int i = 0; i < n; ++i) a += ps.dq[(size_t)i * 64 + p - WRSN_PP_QUERY_B];
        } else if (p < WRSN_PP_CHARGE + 256) {                // charge, rows z: z x (dmu, ds_raw)
            const int k = (p - WRSN_PP_CHARGE) >> 1, d = (p - WRSN_PP_CHARGE) & 1;
            for (int i = 0; i < n; ++i) a = fmaf(s.z2[(b0 + i) * 128 + k], ps.dch[(size_t)i * 2 + d], a);
        } else if (p < WRSN_PP_CHARGE_B) {                    // charge, rows x_k: the stored node's features as they stand, zeros for node -1
            const int f = (p - WRSN_PP_CHARGE - 256) >> 1, d = (p - WRSN_PP_CHARGE) & 1;
            const int32_t* index = gs.g[grp].index;
            const size_t R = (size_t)(WRSN_ENT_NODE_F * dmN + WRSN_ENT_MC_F * dmM + WRSN_ENT_ENV_F);
            for (int i = 0; i < n; ++i) {
                const int k = (int)ps.prow[(size_t)i * 8 + 5];
                const int kk = k < 0 ? 0 : k;
                const float x = gs.g[grp].rows[(size_t)(index ? index[i] : i) * R + (size_t)kk * WRSN_ENT_NODE_F + f];
                a = fmaf(k < 0 ? 0.f : x, ps.dch[(size_t)i * 2 + d], a);
            }
        } else if (p < WRSN_PP_CHARGE_B + 2) {
            for (int i = 0; i < n; ++i) a += ps.dch[(size_t)i * 2 + p - WRSN_PP_CHARGE_B];
        }
    } else {
        if (p < WRSN_EP_MEAN_B) {
            const int k = (p - WRSN_EP_MEAN) / 3, d = (p - WRSN_EP_MEAN) - 3 * k;
            for (int i = 0; i < n; ++i) a = fmaf(s.z2[(b0 + i) * 128 + k], s.dout[(size_t)i * 8 + d], a);
        } else if (p < WRSN_EP_LSTD) {
            for (int i = 0; i < n; ++i) a += s.dout[(size_t)i * 8 + p - WRSN_EP_MEAN_B];
        } else if (p < WRSN_EP_LSTD_B) {
            const int k = (p - WRSN_EP_LSTD) / 3, d = (p - WRSN_EP_LSTD) - 3 * k;
            for (int i = 0; i < n; ++i) a = fmaf(s.z2[(b0 + i) * 128 + k], s.dout[(size_t)i * 8 + 3 + d], a);
        } else if (p < WRSN_EP_LSTD_B + 3) {
            for (int i = 0; i < n; ++i) a += s.dout[(size_t)i * 8 + 3 + p - WRSN_EP_LSTD_B];
        }
    }
    (net ? gs.g[grp].grad_critic : gs.g[grp].grad_actor)[p] = a;   // the padding: zero
}
__global__ void __launch_bounds__(256) wrsn_et_reduce_kernel(WrsnEtGroups gs, int n, WrsnEtScratch s0) {
    wrsn_et_reduce_body<false>(gs, n, s0, WrsnEtpScratch{}, 0, 0);
}

// ||g|| of a block, summed by one workgroup in a fixed order: workgroup k takes block k of the table
__global__ void __launch_bounds__(256) wrsn_et_norm_kernel(WrsnEtAdamBlocks bs, float* __restrict__ norm) {
    extern __shared__ double smem[];
    const int tid = (int)threadIdx.x, k = (int)blockIdx.x;
    const float* g = bs.b[k].g;
    const int nf = bs.b[k].nf;
    float* norm_out = bs.b[k].norm_out;
    double a = 0.0;
    for (int i = tid; i < nf; i += 256) a += (double)g[i] * (double)g[i];
    const double t = wrsn_et_block_sum(a, smem, tid);
    if (tid == 0) { const float r = (float)sqrt(t); norm[k] = r; if (norm_out) *norm_out = r; }
}

// clip_grad_norm_ then torch.optim.Adam (no weight decay, no amsgrad) on every block of the table, in place: `per` workgroups per block
__global__ void __launch_bounds__(256) wrsn_et_adam_kernel(WrsnEtAdamBlocks bs, int per, const float* __restrict__ norm, float beta1, float beta2,
                                                           float omb1, float omb2, float eps, float max_norm) {   // omb: 1 - beta, rounded once
    const int k = (int)blockIdx.x / per, i = ((int)blockIdx.x - k * per) * 256 + (int)threadIdx.x;
    if (i >= bs.b[k].nf) return;
    float* p = bs.b[k].p; const float* g = bs.b[k].g; float* m = bs.b[k].m; float* v = bs.b[k].v;
    const float step_size = bs.b[k].step_size, inv_sqrt_bc2 = bs.b[k].inv_sqrt_bc2;
    const float scale = fminf(1.f, max_norm / (norm[k] + 1e-6f));
    const float gi = g[i] * scale;
    const float mi = beta1 * m[i] + omb1 * gi;
    const float vi = beta2 * v[i] + omb2 * gi * gi;
    m[i] = mi; v[i] = vi;
    p[i] = p[i] - step_size * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
}

// ------------------------------------------------------------------------------------------------------------------------------------
// wrsn_entity_prepare: the PPO batch of G groups -- values, PPOLearner.cal_rt_adv (gae=True), gathers -- in three launches.
//   the two forward kernels above, unchanged, on 2 G ROW SETS: entry 2 g of the group table is (no actor, group g's critic, its `state`
//       rows), entry 2 g + 1 the same critic on its `next_state` rows, both under group g's index.  An entry without an actor costs a
//       block that returns at once; the value of row i of an entry is raw[8 i + 6] of the entry's scratch slice -- the float
//       wrsn_entity_eval writes for that row and block, from the same instructions
//   wrsn_et_prepare_kernel   1 + n blocks per group, the group in blockIdx.x alone.  Block 0 of a group: delta_t and c tm_t of a chunk of
//       WRSN_ET_PREP_CHUNK positions formed by the 256 threads into LDS (the small gathers ride along), then ONE lane runs the
//       dependent chain over the chunk from its end, eight positions' operands loaded ahead of their use; chunks go from the last to the
//       first and the lane carries `last` across them, so n is unbounded and the order is the reference's.  Block 1 + i of a group:
//       out_state[i] and out_next_state[i] as 16-byte copies.
// The recurrence is the reference's float32 statement sequence: every product and sum below is rounded on its own (contraction off).
#define WRSN_ET_PREP_CHUNK 256
#define WRSN_ET_PREP_LDS (3 * WRSN_ET_PREP_CHUNK * 4)         // bytes: delta / advantage, c tm, value
struct WrsnEtPrepGroup {
    const float* state; const float* next_state; const float* reward; const float* terminal; const float* action; const float* logp;
    float* value; float* advantage; float* ret; float* out_state; float* out_next_state; float* out_action; float* out_logp; float* out_reward;
};
struct WrsnEtPrepGroups { WrsnEtPrepGroup g[WRSN_MAX_MC]; };

// delta = (r + (g nv) tm) - v, and last' = delta + (ctm last): four, then two roundings
WDEV float wrsn_et_gae_delta(float r, float g, float nv, float tm, float v) {
#pragma clang fp contract(off)
    const float a = g * nv;
    const float b = a * tm;
    const float c = r + b;
    return c - v;
}
WDEV float wrsn_et_gae_step(float delta, float ctm, float last) {
#pragma clang fp contract(off)
    const float a = ctm * last;
    return delta + a;
}
WDEV float wrsn_et_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
WDEV float wrsn_et_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

__global__ void __launch_bounds__(256) wrsn_et_prepare_kernel(WrsnEtPrepGroups ps, int n, int row_u4, const int32_t* __restrict__ index, float g, float c,
                                                              WrsnEtScratch s0) {
    extern __shared__ double smem[];
    const int tid = (int)threadIdx.x;
    const int grp = (int)blockIdx.x / (n + 1), j = (int)blockIdx.x - grp * (n + 1);
    const WrsnEtPrepGroup& P = ps.g[grp];
    const int32_t* idx = index ? index + (size_t)grp * n : nullptr;
    if (j > 0) {                                              // ---- the rows of position i, 16 bytes per thread and pass
        const int i = j - 1;
        const size_t src = (size_t)(idx ? idx[i] : i) * row_u4, dst = (size_t)i * row_u4;
        const WrsnU4* a = (const WrsnU4*)P.state; const WrsnU4* b = (const WrsnU4*)P.next_state;
        WrsnU4* oa = (WrsnU4*)P.out_state; WrsnU4* ob = (WrsnU4*)P.out_next_state;
        for (int k = tid; k < row_u4; k += 256) {
            if (oa) wrsn_st_u4(wrsn_global(oa + dst + k), wrsn_ld_u4(wrsn_global(a + src + k)));
            if (ob) wrsn_st_u4(wrsn_global(ob + dst + k), wrsn_ld_u4(wrsn_global(b + src + k)));
        }
        return;
    }
    float* sD = (float*)smem; float* sC = sD + WRSN_ET_PREP_CHUNK; float* sV = sC + WRSN_ET_PREP_CHUNK;
    const float* raw_v = wrsn_et_slice(s0, 2 * grp).raw;      // [n][8]: slot 6 is the critic's value of the row
    const float* raw_nv = wrsn_et_slice(s0, 2 * grp + 1).raw;
    float last = 0.f;                                         // thread 0's, carried from chunk to chunk
    for (int hi = n; hi > 0; hi -= WRSN_ET_PREP_CHUNK) {      // block-uniform
        const int lo = hi > WRSN_ET_PREP_CHUNK ? hi - WRSN_ET_PREP_CHUNK : 0, m = hi - lo;
        for (int k = tid; k < m; k += 256) {
            const size_t t = (size_t)(lo + k), s = (size_t)(idx ? idx[t] : (int)t);
            const float r = P.reward[s], tm = P.terminal ? P.terminal[s] : 0.f;
            const float v = raw_v[t * 8 + 6], nv = raw_nv[t * 8 + 6];
            sD[k] = wrsn_et_gae_delta(r, g, nv, tm, v); sC[k] = wrsn_et_mul(c, tm); sV[k] = v;
            P.value[t] = v;
            if (P.out_reward) P.out_reward[t] = r;
            if (P.out_logp) P.out_logp[t] = P.logp[s];
            if (P.out_action) { P.out_action[t * 3] = P.action[s * 3]; P.out_action[t * 3 + 1] = P.action[s * 3 + 1]; P.out_action[t * 3 + 2] = P.action[s * 3 + 2]; }
        }
        __syncthreads();
        if (tid == 0) {                                       // the dependent chain: t = hi - 1 .. lo
            int k = m;
            for (; k >= 8; k -= 8) {
                float d[8], cf[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { d[u] = sD[k - 1 - u]; cf[u] = sC[k - 1 - u]; }
#pragma unroll
                for (int u = 0; u < 8; ++u) { last = wrsn_et_gae_step(d[u], cf[u], last); sD[k - 1 - u] = last; }
            }
            for (; k > 0; --k) { last = wrsn_et_gae_step(sD[k - 1], sC[k - 1], last); sD[k - 1] = last; }
        }
        __syncthreads();
        for (int k = tid; k < m; k += 256) {
            const size_t t = (size_t)(lo + k);
            const float a = sD[k];
            P.advantage[t] = a; P.ret[t] = wrsn_et_add(a, sV[k]);
        }
        __syncthreads();                                      // the next chunk overwrites the LDS arrays
    }
}
