// wrsn_api.hip -- host side of libwrsn_hip.so: the C-ABI declared in include/wrsn_hip.h.
// Owns device memory of a handle and launches the gfx950 kernels of wrsn_sim.h.  There is no CPU
// execution path: without a HIP device wrsn_create fails with WRSN_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <cstdlib>
#include <vector>

#include "../../include/wrsn_hip.h"
#include "wrsn_sim.h"
#include "wrsn_rollout.h"
#include "wrsn_state.h"
#include "wrsn_entity_train.h"
#include "wrsn_entity_pointer_train.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(WRSN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// Every entry point runs on the handle's device and leaves the calling thread's current device as it found it (handles of
// different GPUs may share a process and a thread with torch).
struct DeviceGuard {
    int prev; bool ok;
    explicit DeviceGuard(int dev) : prev(-1), ok(false) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (prev == dev) || hipSetDevice(dev) == hipSuccess;
        if (prev == dev) prev = -1;                            // nothing to restore
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define WRSN_ON_DEVICE(h_)                                                                             \
    DeviceGuard guard_((h_)->cfg.device);                                                              \
    if (!guard_.ok) return fail(WRSN_ERR_HIP, "hipSetDevice failed for the handle's device")

int npl_for(int n_node) {
    int need = (n_node + 63) / 64;
    const int choices[] = {1, 2, 4, 8, 16};
    for (int c : choices) if (c >= need) return c;
    return -1;
}

}  // namespace

// nodes-per-lane dispatch (select_kernels): `M_(NPL)` for the handle's register-slot count.  Diagnostic builds (tools/ab_build.sh) compile one slot count only
// (-DWRSN_ONLY_NPL=4: a quarter of the build time); the product build has all five.
#ifdef WRSN_ONLY_NPL
#define WRSN_NPL_SWITCH(npl_, M_, bad_) switch (npl_) { case WRSN_ONLY_NPL: M_(WRSN_ONLY_NPL); break; default: bad_; }
#else
#define WRSN_NPL_SWITCH(npl_, M_, bad_) switch (npl_) { case 1: M_(1); break; case 2: M_(2); break; case 4: M_(4); break; case 8: M_(8); break; case 16: M_(16); break; default: bad_; }
#endif

// every step kernel has one signature, and so has every warm-up kernel: a handle picks its pair once (select_kernels)
typedef void (*wrsn_step_fn)(const WrsnDev*, int, const int32_t*, const double*, int, int, long long, int, const uint8_t*, WrsnStepOutDev, int, int, int);
typedef void (*wrsn_warmup_fn)(const WrsnDev*, int);

struct wrsn_handle {
    wrsn_cfg cfg{};
    WrsnDev dev{};
    hipStream_t stream = nullptr;
    int npl = 0;
    int scenario_set = 0;
    int lds_env = 0, lds_obs = 0;   // LDS bytes of an environment wave, of an observation block
    int cc_bound = 0;               // largest WrsnEnvConst.conn_bound of the scenarios set so far (-> WrsnDev.CC)
    hipStream_t stream2 = nullptr;  // the short stage of a pipelined step call runs here, beside the long one on `stream`
    hipEvent_t ev_fork = nullptr, ev_join = nullptr; int ev2_ok = 0;
    int cus = 256;                  // compute units of the device
    int slots = 0;                  // wave slots of the device for the step kernel (CUs x resident waves per CU): launch-order dependent budgets
    long long epoch = 1;            // counter of wrsn_step calls: an argument of the step kernels that they do not read
    int step_budget = 0;            // work units one wrsn_step launch may spend per environment, 0 = run every step to its end
    int deadline_ticks = 0;         // wrsn_set_step_deadline in 100 MHz wall-clock ticks, 0 = none
    int pipe = 1;                   // step calls that render run as a two-stage pipeline over the launch order (WRSN_PIPE=0 disables)
    int obs_reuse = 0;              // wrsn_set_obs_reuse: the caller keeps the observation rows the library wrote
    int obs_fmt = WRSN_OBS_F32;     // wrsn_set_obs_format: WRSN_OBS_F32 / WRSN_OBS_BF16, the element type behind every observation pointer
    int timing = 0;                 // record HIP events around the kernels of every wrsn_step (wrsn_set_timing)
    hipEvent_t ev[4] = {};          // before the order kernels, after them, after the step kernel, after the observation
    int ev_ok = 0;                  // events created
    int ev_mask = 0;                // bit i: the last timed wrsn_step recorded ev[i] (time_mark)
    int bp2 = 0;                    // B rounded up to a power of two when the launch order is sorted on the device (B <= 8192), else 0
    std::vector<void*> allocs;
    WrsnDev* d_dev = nullptr;       // device copy of `dev`: the environment kernels read it through the constant cache; `sd` follows it
    WrsnStochDev sd{};              // prob_gp < 1: MT19937 state, send costs, prob_gp per environment (allocated by the first seeded call)
    int stoch = 0;                  // an environment was loaded with prob_gp != 1 through wrsn_set_scenario_seeded: the stochastic kernels run
    wrsn_step_fn step_kernel = nullptr;   // the kernels of this handle's `npl` and `stoch` (select_kernels)
    wrsn_warmup_fn warmup_kernel = nullptr;
    std::vector<uint8_t> filled;    // per environment: holds a scenario (wrsn_set_scenario*, wrsn_load_envs, wrsn_clone_envs)
    // environment records (wrsn_state.h): the segment table of this handle's layout (generator block iff sd.mt_live), on the host and in
    // device memory; staging for the host index arrays, the gathered headers of a load and the charger list of the observation pass
    WrsnSeg segs[WRSN_REC_MAXSEG] = {}; int nseg = 0; int64_t rec_bytes = 0;
    WrsnSeg* d_segs = nullptr;
    int32_t* d_idx = nullptr; size_t idx_cap = 0;
    uint8_t* d_hdr = nullptr;       // [B] headers (destinations of a load are distinct)
    int32_t* d_rend = nullptr;
    // scenario pool (wrsn_pool_set / wrsn_pool_reset): the caller's records, and what belongs to the HANDLE rather than to an environment's
    // record: per environment the pool record it runs (-1: none) and its swaps since wrsn_pool_set; the pair list of a pool reset
    // ([0, B) environments, [B, 2B) records) and its length
    const uint8_t* pool = nullptr; int pool_n = 0; uint64_t pool_seed = 0; int64_t pool_rec_bytes = 0;
    int32_t* d_pool_cur = nullptr; int32_t* d_pool_swaps = nullptr;
    int32_t* d_pairs = nullptr; int32_t* d_pair_n = nullptr;
    int ptr_mask = WRSN_POINTER_MASK_NONE;   // wrsn_set_entity_pointer_mask: the candidate mask of the node-pointer calls, read when they enqueue
    WrsnEntityOut ent{};            // wrsn_set_entity_out: the caller's entity-observation buffers (node == nullptr: off, the default)
    // wrsn_entity_act (allocated by its first call): the head's inputs [B, WRSN_ENTPOL_FEAT], the row lists [M, B] and counters [8] per charger
    float* ep_feat = nullptr; int32_t* ep_list = nullptr; int32_t* ep_cnt = nullptr;
    // wrsn_entity_pointer_act (allocated by its first call): z [B, 128] and q [B, 64] between its head and score kernels; it shares the above
    float* pp_z = nullptr; float* pp_q = nullptr;
    // wrsn_entity_eval / wrsn_entity_ppo_grad / wrsn_entity_adam: the scratch area (grown on demand, the old one kept until wrsn_destroy: launches
    // in flight may still use it) and the gradient norm of the Adam call
    float* et_scratch = nullptr; size_t et_cap = 0; float* et_norm = nullptr;
    // wrsn_clone_envs_from, on the DESTINATION handle: the records of the distinct sources of a call (grown on demand, the old area kept
    // until wrsn_destroy: launches in flight may still read it)
    uint8_t* xfer = nullptr; size_t xfer_cap = 0;
};

namespace {

template <typename T>
int dalloc(wrsn_handle* h, T** p, size_t count) {
    void* q = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = sizeof(T);
    HIPCHK(hipMalloc(&q, bytes));
    HIPCHK(hipMemset(q, 0, bytes));
    h->allocs.push_back(q);
    *p = (T*)q;
    return 0;
}

// THE table of per-environment arrays: every array of a handle that holds one slice per environment, in record order.  The order is
// fixed by record format version 1 (WRSN_REC_VERSION, wrsn_state.h): an array added here changes the format.  Calls
// f(pointer, bytes of one environment's slice, copy kind) for the arrays of `parts` until one call returns non-zero, and returns that.
// Allocation (wrsn_create, alloc_stoch) and the segment table of a record (rec_segments) both come from here and from nowhere else, so an
// array cannot be part of a handle without being part of its records.  Copy kind: WRSN_SEG_DYN for the live WrsnEnvDyn, else
// WRSN_SEG_V16 = 16-byte copies where base and size allow.  43 arrays in ENV_ARRAYS_DEV, 5 in ENV_ARRAYS_GEN.
enum { ENV_ARRAYS_DEV = 1,     // WrsnDev: constants, topology, the `live` and `snap` node arrays
       ENV_ARRAYS_GEN = 2 };   // WrsnStochDev: the generator block of handles that keep generators
template <typename H, typename F>
int for_each_env_array(H* h, int parts, F f) {
    auto& d = h->dev;
    const int64_t NP = d.NP, TP = d.TP, ECAP = d.ECAP, CCAP = d.CCAP;
    int rc = 0;
    auto a = [&](auto& p, int64_t bytes, int kind = WRSN_SEG_V16) { if (!rc) rc = f(p, bytes, kind); };
    if (parts & ENV_ARRAYS_DEV) {
        a(d.ec, sizeof(WrsnEnvConst));
        a(d.node_x, NP * 8); a(d.node_y, NP * 8); a(d.dist_bs, NP * 8);
        a(d.target_x, TP * 8); a(d.target_y, TP * 8);
        a(d.nb_off, (NP + 1) * 4); a(d.nb_idx, ECAP * 4); a(d.nb_dist, ECAP * 8);
        a(d.tc_off, (TP + 1) * 4); a(d.tc_idx, CCAP * 4);
        a(d.ncov, NP * 4); a(d.nflags, NP * 4); a(d.nbp, NP * 16);
        a(d.nbp_es, NP * 64); a(d.es_bs, NP * 8); a(d.adjm, NP * 32);
        a(d.xorder, NP * 4); a(d.tcp, TP * 16);
        for (int k = 0; k < 2; ++k) {
            auto& n = k == 0 ? d.live : d.snap;
            a(n.E, NP * 8); a(n.CS, NP * 8); a(n.RR, NP * 8);
            a(n.d1, NP * 8); a(n.d2, NP * 8); a(n.ring, WRSN_RING * NP * 8);
            a(n.logbuf, NP * 8); a(n.ls, NP * 4); a(n.rcv, NP * 4);
            a(n.conn, WRSN_MAX_MC * WRSN_CONN_CAP * 2); a(n.conn_xy, WRSN_MAX_MC * WRSN_CONN_CAP * 2 * 8);
            a(n.dyn, sizeof(WrsnEnvDyn), k == 0 ? WRSN_SEG_DYN : WRSN_SEG_V16);
        }
    }
    if (parts & ENV_ARRAYS_GEN) {
        auto& s = h->sd;
        a(s.mt_live, WRSN_MT_STRIDE * 4); a(s.mt_snap, WRSN_MT_STRIDE * 4);
        a(s.es_live, NP * 8); a(s.es_snap, NP * 8); a(s.pgp, 8);
    }
    return rc;
}

// device memory, zero-filled, for the arrays of `parts`: B slices each
int alloc_env_arrays(wrsn_handle* h, int parts) {
    const size_t B = h->dev.B;
    return for_each_env_array(h, parts, [&](auto*& p, int64_t bytes, int) { return dalloc(h, &p, B * (size_t)bytes / sizeof(*p)); });
}

// the step and warm-up kernels of the handle's nodes-per-lane count, stochastic (prob_gp < 1) or plain
int select_kernels(wrsn_handle* h) {
#define WRSN_PICK(NPL_) h->step_kernel = h->stoch ? wrsn_step_stoch_kernel<NPL_> : wrsn_step_kernel<NPL_>; \
                        h->warmup_kernel = h->stoch ? wrsn_warmup_stoch_kernel<NPL_> : wrsn_warmup_kernel<NPL_>
    WRSN_NPL_SWITCH(h->npl, WRSN_PICK, return fail(WRSN_ERR_ARG, "unsupported nodes-per-lane"))
#undef WRSN_PICK
    return 0;
}

// kernels, LDS sizes, wave slots and the device copy of the descriptor; again whenever WrsnDev.CC changes or `stoch` is switched on
int configure_launch(wrsn_handle* h) {
    WrsnDev& d = h->dev;
    if (int rc = select_kernels(h)) return rc;
    h->lds_env = wrsn_lds_bytes(d.NP, d.M, d.CC) + (h->stoch ? wrsn_stoch_lds_bytes(d.NP) : 0);
    {   // wave slots of the step kernel on this device (registers and LDS decide): the budget taper of a launch starts behind the blocks
        // that are resident from the first moment
        int per_cu = 0;
        const hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, h->step_kernel, 64, (size_t)h->lds_env);
        h->slots = h->cus * 8;
        if (oe == hipSuccess && per_cu >= 1 && per_cu <= 16) h->slots = h->cus * per_cu;
    }
    HIPCHK(hipMemcpy(h->d_dev, &h->dev, sizeof(WrsnDev), hipMemcpyHostToDevice));
    if (h->stoch) HIPCHK(hipMemcpy(h->d_dev + 1, &h->sd, sizeof(WrsnStochDev), hipMemcpyHostToDevice));
    return 0;
}

// The scenarios or records that just came in need connected-node lists of `conn_bound` entries, and the stochastic kernels if
// `want_stoch`: WrsnDev.CC is the largest bound so far rounded up to a multiple of 4 (4..WRSN_CONN_CAP); a change of either is a new
// launch configuration (LDS and wave slots of the step kernel).
int fit_launch(wrsn_handle* h, int conn_bound, bool want_stoch) {
    if (conn_bound > h->cc_bound) h->cc_bound = conn_bound;
    int cc = ((h->cc_bound + 3) / 4) * 4; cc = cc < 4 ? 4 : (cc > WRSN_CONN_CAP ? WRSN_CONN_CAP : cc);
    const bool stoch_on = want_stoch && !h->stoch;
    if (cc == h->dev.CC && !stoch_on) return 0;
    h->dev.CC = cc; if (stoch_on) h->stoch = 1;
    return configure_launch(h);
}

WrsnStepOutDev step_out_dev(const wrsn_step_out* out, bool with_obs = true) {
    WrsnStepOutDev o;
    o.agent_id = out->agent_id; o.reward = out->reward; o.terminal = out->terminal; o.now = out->now; o.status = out->status;
    o.obs = with_obs ? out->obs : nullptr;
    return o;
}

// ------------------------------------------------------------------ launches
// The one observation launch: blocks [block0, block0 + nblocks) of `order` (nullptr: of the environments themselves) on `stream`, float32
// or bf16 rows as the handle says (`obs` holds bf16 bit patterns then: the C-ABI keeps one pointer type).
void launch_obs(wrsn_handle* h, hipStream_t stream, const int32_t* agent_id, float* obs, const int32_t* order, int block0, int nblocks) {
    if (h->obs_fmt == WRSN_OBS_BF16)
        hipLaunchKernelGGL(wrsn_obs_bf16_kernel, dim3(nblocks), dim3(256), h->lds_obs, stream, h->dev, agent_id, (uint16_t*)obs, h->obs_reuse, order, block0);
    else
        hipLaunchKernelGGL(wrsn_obs_kernel, dim3(nblocks), dim3(256), h->lds_obs, stream, h->dev, agent_id, obs, h->obs_reuse, order, block0);
}

// The one entity-observation launch, next to launch_obs on the same stream with the same rows: nothing unless buffers are registered
// (wrsn_set_entity_out) or `to` names some (wrsn_entities).  K nodes per thread: the smallest of 1, 2, 4 with K * 256 >= N.
void launch_entities(wrsn_handle* h, hipStream_t stream, const int32_t* agent_id, const int32_t* order, int block0, int nblocks, const WrsnEntityOut* to = nullptr) {
    const WrsnEntityOut& e = to ? *to : h->ent;
    if (!e.node) return;
    const int k = (h->dev.N + 255) / 256;
    if (k <= 1) hipLaunchKernelGGL(wrsn_entity_kernel<1>, dim3(nblocks), dim3(256), 0, stream, h->dev, agent_id, e, order, block0);
    else if (k == 2) hipLaunchKernelGGL(wrsn_entity_kernel<2>, dim3(nblocks), dim3(256), 0, stream, h->dev, agent_id, e, order, block0);
    else hipLaunchKernelGGL(wrsn_entity_kernel<4>, dim3(nblocks), dim3(256), 0, stream, h->dev, agent_id, e, order, block0);
}

// the rows of `agent_id` over the whole batch on the caller's stream: the image when `obs` is given, then the entity rows when registered
int launch_render_all(wrsn_handle* h, const int32_t* agent_id, float* obs) {
    if (obs) launch_obs(h, h->stream, agent_id, obs, nullptr, 0, h->dev.B);
    launch_entities(h, h->stream, agent_id, nullptr, 0, h->dev.B);
    HIPCHK(hipGetLastError());
    return 0;
}

// wrsn_set_timing: event i of this wrsn_step on the caller's stream; nothing unless the call is timed
void time_mark(wrsn_handle* h, int i) {
    if (!h->timing) return;
    (void)hipEventRecord(h->ev[i], h->stream);
    h->ev_mask |= 1 << i;
}

// what the step-kernel launches of one call have in common
struct StepCall {
    int reset_call;
    const int32_t* agent_id; const double* action; int auto_reset;
    long long epoch;
    int slots;                 // wave slots (low 16 bits) | budget taper over the launch order; 0: neither (time-sliced launch)
    const uint8_t* mask;
    WrsnStepOutDev out;
    int handoff, deadline;     // 3 / wall-clock ticks for a time-sliced launch, else 0
};

// budget taper over the launch order in units of slots / 8 blocks, start << 16 | length << 24: start 8 = after the first `slots` blocks,
// length 16 = down to zero over two times `slots` blocks (the floor of a quarter applies first)
const int STEP_TAPER = (8 << 16) | (16 << 24);
int tapered_slots(const wrsn_handle* h) { return (h->slots & 0xFFFF) | STEP_TAPER; }

// the one step-kernel launch: blocks [block0, block0 + nblocks) of the launch order on `stream` with work budget `budget`
void launch_step_blocks(wrsn_handle* h, const StepCall& c, hipStream_t stream, int block0, int nblocks, int budget) {
    hipLaunchKernelGGL(h->step_kernel, dim3(nblocks), dim3(64), h->lds_env, stream, (const WrsnDev*)h->d_dev, c.reset_call, c.agent_id, c.action,
                       c.auto_reset, budget, c.epoch, c.slots, c.mask, c.out, c.handoff, c.deadline, block0);
}

int launch_warmup(wrsn_handle* h, int env0, int nenv) {
    hipLaunchKernelGGL(h->warmup_kernel, dim3(nenv), dim3(64), h->lds_env, h->stream, (const WrsnDev*)h->d_dev, env0);
    HIPCHK(hipGetLastError());
    return 0;
}

// the step kernel as a reset of the environments of `mask`, then their observations when out.obs is set
int launch_reset(wrsn_handle* h, const uint8_t* mask, const WrsnStepOutDev& out) {
    const StepCall c = {1, nullptr, nullptr, 0, 0, tapered_slots(h), mask, out, 0, 0};
    launch_step_blocks(h, c, h->stream, 0, h->dev.B, 0);
    HIPCHK(hipGetLastError());
    return (out.obs || h->ent.node) ? launch_render_all(h, h->dev.render_agent, out.obs) : 0;
}

// launch order of a step call, longest job first (wrsn_estimate_kernel / wrsn_sort_kernel, wrsn_sim.h): two tiny launches
void launch_order(wrsn_handle* h, const StepCall& c) {
    hipLaunchKernelGGL(wrsn_estimate_kernel, dim3((h->bp2 + WRSN_EST_THREADS - 1) / WRSN_EST_THREADS), dim3(WRSN_EST_THREADS), 0, h->stream, h->dev, c.agent_id, c.action, c.auto_reset, h->bp2);
    const int kpt = h->bp2 / WRSN_SORT_THREADS;                // keys per thread of the sort workgroup (0, 1: plain network in LDS)
    const size_t lb = (size_t)wrsn_sort_lds_bytes();
#define WRSN_SORT(K_) hipLaunchKernelGGL((wrsn_sort_kernel<K_>), dim3(1), dim3(WRSN_SORT_THREADS), lb, h->stream, h->dev, h->bp2)
    switch (kpt) {
    case 2: WRSN_SORT(2); break;
    case 4: WRSN_SORT(4); break;
    case 8: WRSN_SORT(8); break;                               // the most there is: wrsn_create sorts on the device up to 8 keys per thread
    default: WRSN_SORT(1); break;
    }
#undef WRSN_SORT
}

// behind the step launch(es) of a call that is not pipelined: one observation launch over the whole batch when the call renders, one
// entity launch when entity buffers are registered
int finish_step(wrsn_handle* h, const StepCall& c) {
    time_mark(h, 2);
    HIPCHK(hipGetLastError());
    if (!c.out.obs && !h->ent.node) return 0;
    if (int rc = launch_render_all(h, h->dev.render_agent, c.out.obs)) return rc;
    time_mark(h, 3);
    return 0;
}

// Time-sliced step call (wrsn_set_step_deadline): latch + preset kernel, then one block per environment in this launch's cyclic order:
// the blocks that only start when the time slice is over leave their environments alone
int launch_step_sliced(wrsn_handle* h, StepCall c) {
    const int B = h->dev.B;
    hipLaunchKernelGGL(wrsn_latch_kernel, dim3((B + 255) / 256), dim3(256), 0, h->stream, h->dev, c.agent_id, c.action, c.out);
    time_mark(h, 1);
    c.slots = 0; c.handoff = 3; c.deadline = h->deadline_ticks;
    launch_step_blocks(h, c, h->stream, 0, B, h->step_budget > 0 ? h->step_budget : (1 << 28));   // the deadline is looked at wherever a work budget is
    return finish_step(h, c);
}

int launch_step_single(wrsn_handle* h, const StepCall& c) {
    launch_step_blocks(h, c, h->stream, 0, h->dev.B, h->step_budget);
    return finish_step(h, c);
}

// A step call that renders, as a PIPELINE over the two halves of the launch order (longest job first): the short half is stepped on the
// second stream and rendered there as soon as it is done -- nearly all of its steps complete, it carries ~60 % of the observations of
// the call -- while the long half (work-capped or slow steps, the tail of the launch) is still being stepped on the caller's stream;
// only the observations of the long half are left for afterwards.  The step kernel is bound by instruction issue and latency and leaves
// the HBM idle, the observation kernel is a 160 KB store stream per row: they overlap well.  Same blocks, same budgets, same results.
// (only when the batch is at most two rounds of the wave slots: with more, the short half is the longer one and nothing overlaps --
//  4 096 environments of 1 000 nodes on 768 slots: 0.87 M env-steps/s with the pipeline, 0.96 M without)
bool step_pipelines(const wrsn_handle* h, const StepCall& c) {
    const int B = h->dev.B;
    return c.out.obs && h->pipe && h->ev2_ok && h->bp2 > 0 && B >= 512 && B <= 2 * h->slots;
}

const int PIPE_LONG_PCT = 50;      // share of the launch order that is the long stage
const int PIPE_SHORT_PCT = 40;     // work cap of the short stage in per cent of the step budget (its stragglers go on in the next call)

// Stages over the launch order: [0, n2) the long half (caller's stream), [n2, B) the short half with its own work cap (second stream, high
// priority: its blocks get wave slots first); n2 <= wave slots: the long half's jobs all start at once.  The short half is launched first.
int launch_step_pipeline(wrsn_handle* h, const StepCall& c) {
    const int B = h->dev.B, budget = h->step_budget;
    const int32_t* agent = h->dev.render_agent; const int32_t* order = h->dev.order;
    int n2 = (B * PIPE_LONG_PCT / 100 + 63) & ~63; if (n2 > h->slots) n2 = h->slots & ~63; if (n2 < 64) n2 = 64;
    const int b_short = budget > 0 ? (budget * PIPE_SHORT_PCT / 100 > 64 ? budget * PIPE_SHORT_PCT / 100 : 64) : 0;
    (void)hipEventRecord(h->ev_fork, h->stream); (void)hipStreamWaitEvent(h->stream2, h->ev_fork, 0);
    launch_step_blocks(h, c, h->stream2, n2, B - n2, b_short);
    launch_obs(h, h->stream2, agent, c.out.obs, order, n2, B - n2);
    launch_entities(h, h->stream2, agent, order, n2, B - n2);
    (void)hipEventRecord(h->ev_join, h->stream2);
    launch_step_blocks(h, c, h->stream, 0, n2, budget);
    time_mark(h, 2);
    launch_obs(h, h->stream, agent, c.out.obs, order, 0, n2);
    launch_entities(h, h->stream, agent, order, 0, n2);
    (void)hipStreamWaitEvent(h->stream, h->ev_join, 0);
    time_mark(h, 3);
    HIPCHK(hipGetLastError());
    return 0;
}

// one wrsn_step: the step of every environment and, when out.obs is set, the observations of the new requests
int launch_step(wrsn_handle* h, const int32_t* agent_id, const double* action, int auto_reset, const WrsnStepOutDev& out) {
    const StepCall c = {0, agent_id, action, auto_reset, ++h->epoch, tapered_slots(h), nullptr, out, 0, 0};
    h->ev_mask = 0;
    time_mark(h, 0);
    if (h->deadline_ticks > 0) return launch_step_sliced(h, c);
    if (h->bp2 > 0) launch_order(h, c);
    time_mark(h, 1);
    return step_pipelines(h, c) ? launch_step_pipeline(h, c) : launch_step_single(h, c);
}

// xoshiro256** seeded by splitmix64: the synthetic generator's own counter-free RNG
struct Rng {
    uint64_t s[4];
    static uint64_t splitmix(uint64_t& x) {
        uint64_t z = (x += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    explicit Rng(uint64_t seed) { uint64_t x = seed; for (int i = 0; i < 4; ++i) s[i] = splitmix(x); }
    static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
    uint64_t next() {
        uint64_t r = rotl(s[1] * 5, 7) * 9, t = s[1] << 17;
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t; s[3] = rotl(s[3], 45);
        return r;
    }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    double uni(double a, double b) { return a + (b - a) * uni(); }
    int below(int n) { return (int)(uni() * n) % (n > 0 ? n : 1); }
    double normal() { double u1 = uni(), u2 = uni(); if (u1 < 1e-300) u1 = 1e-300; return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2); }
};

// random.seed(s) of CPython for an integer s (init_by_array over the little-endian 32-bit words of abs(s)), then index 624 and no
// draws yet: one environment's block of WrsnStochDev.mt_* (WRSN_MT_STRIDE words)
void mt_seed(int64_t seed, uint32_t* st) {
    uint64_t n = seed < 0 ? (uint64_t)0 - (uint64_t)seed : (uint64_t)seed;
    uint32_t key[2]; int klen = 0;
    do { key[klen++] = (uint32_t)n; n >>= 32; } while (n != 0);
    uint32_t* mt = st;
    mt[0] = 19650218u;
    for (int i = 1; i < WRSN_MT_N; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    int i = 1, j = 0;
    for (int k = WRSN_MT_N > klen ? WRSN_MT_N : klen; k; --k) {
        mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
        ++i; ++j;
        if (i >= WRSN_MT_N) { mt[0] = mt[WRSN_MT_N - 1]; i = 1; }
        if (j >= klen) j = 0;
    }
    for (int k = WRSN_MT_N - 1; k; --k) {
        mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
        ++i;
        if (i >= WRSN_MT_N) { mt[0] = mt[WRSN_MT_N - 1]; i = 1; }
    }
    mt[0] = 0x80000000u;
    st[WRSN_MT_N] = WRSN_MT_N; st[WRSN_MT_N + 1] = 0; st[WRSN_MT_N + 2] = 0; st[WRSN_MT_N + 3] = 0;
}

// ------------------------------------------------------------------ environment records (wrsn_state.h)
// The segments of a record: the per-environment slices of for_each_env_array, in its order, each at the next 16-byte aligned offset behind
// the header.  with_gen: the generator block too (its base addresses are the handle's, 0 while it has none: then the table only serves to
// size a record).  Returns the record bytes.
int64_t rec_segments(const wrsn_handle* h, int with_gen, WrsnSeg* segs, int* nseg) {
    int ns = 0; int64_t off = WRSN_REC_HDR;
    for_each_env_array(h, ENV_ARRAYS_DEV | (with_gen ? ENV_ARRAYS_GEN : 0), [&](const void* base, int64_t bytes, int kind) {
        WrsnSeg& g = segs[ns++];
        g.base = (uint64_t)(uintptr_t)base; g.stride = bytes; g.bytes = (int32_t)bytes; g.c0 = (int32_t)(off / 16); g.pad = 0;
        g.kind = kind != WRSN_SEG_V16 ? kind : ((g.base % 16 == 0 && bytes % 16 == 0) ? WRSN_SEG_V16 : WRSN_SEG_WORD);
        off += (bytes + 15) & ~(int64_t)15;
        return 0;
    });
    *nseg = ns;
    return (off + 255) & ~(int64_t)255;
}

// the handle's own layout (generator block iff it keeps generators), uploaded for the copy kernel
int rec_layout(wrsn_handle* h) {
    h->rec_bytes = rec_segments(h, h->sd.mt_live ? 1 : 0, h->segs, &h->nseg);
    HIPCHK(hipMemcpy(h->d_segs, h->segs, (size_t)h->nseg * sizeof(WrsnSeg), hipMemcpyHostToDevice));
    return 0;
}

// the stochastic block of a handle: MT state (live / snapshot), send costs (live / snapshot), prob_gp = 1 everywhere until set
int alloc_stoch(wrsn_handle* h) {
    if (h->sd.mt_live) return 0;
    const size_t B = h->dev.B;
    if (int rc = alloc_env_arrays(h, ENV_ARRAYS_GEN)) return rc;
    std::vector<double> one(B, 1.0);
    HIPCHK(hipMemcpy(h->sd.pgp, one.data(), B * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_dev + 1, &h->sd, sizeof(WrsnStochDev), hipMemcpyHostToDevice));
    return rec_layout(h);                                      // records of this handle carry the generator block from now on
}

// what every record of this handle says about its geometry (wrsn_rec_header_kernel adds the environment's own fields)
WrsnRecHeader rec_template(const wrsn_handle* h) {
    WrsnRecHeader t; std::memset(&t, 0, sizeof(t));
    t.magic = WRSN_REC_MAGIC; t.version = WRSN_REC_VERSION; t.ec_bytes = (int32_t)sizeof(WrsnEnvConst); t.dyn_bytes = (int32_t)sizeof(WrsnEnvDyn);
    t.NP = h->dev.NP; t.TP = h->dev.TP; t.ECAP = h->dev.ECAP; t.CCAP = h->dev.CCAP; t.M = h->dev.M;
    t.has_gen = h->sd.mt_live ? 1 : 0; t.nseg = h->nseg; t.rec_bytes = h->rec_bytes; t.prob_gp = 1.0;
    return t;
}

// Is record i a record this handle can load?  (Geometry, sizes, format; not yet whether its generator block fits the handle.)
int rec_check(const wrsn_handle* h, const WrsnRecHeader& r, int i) {
    const WrsnDev& d = h->dev;
    auto bad = [&](const char* field, long long got, long long want) {
        return fail(WRSN_ERR_ARG, "record " + std::to_string(i) + ": " + field + " is " + std::to_string(got) + ", this handle needs " + std::to_string(want));
    };
    if (r.magic != WRSN_REC_MAGIC) return bad("magic", (long long)r.magic, (long long)WRSN_REC_MAGIC);
    if (r.version != WRSN_REC_VERSION) return bad("version", (long long)r.version, WRSN_REC_VERSION);
    if (r.ec_bytes != (int32_t)sizeof(WrsnEnvConst)) return bad("ec_bytes (sizeof(WrsnEnvConst))", r.ec_bytes, (long long)sizeof(WrsnEnvConst));
    if (r.dyn_bytes != (int32_t)sizeof(WrsnEnvDyn)) return bad("dyn_bytes (sizeof(WrsnEnvDyn))", r.dyn_bytes, (long long)sizeof(WrsnEnvDyn));
    if (r.NP != d.NP) return bad("NP", r.NP, d.NP);
    if (r.TP != d.TP) return bad("TP", r.TP, d.TP);
    if (r.ECAP != d.ECAP) return bad("ECAP", r.ECAP, d.ECAP);
    if (r.CCAP != d.CCAP) return bad("CCAP", r.CCAP, d.CCAP);
    if (r.M != d.M) return bad("M", r.M, d.M);
    if (r.n_node < 1 || r.n_node > d.N) return bad("n_node", r.n_node, d.N);
    if (r.n_target < 1 || r.n_target > d.T) return bad("n_target", r.n_target, d.T);
    if (r.conn_bound < 0 || r.conn_bound > WRSN_CONN_CAP) return bad("conn_bound", r.conn_bound, WRSN_CONN_CAP);
    if (r.has_gen != 0 && r.has_gen != 1) return bad("has_gen", r.has_gen, 1);
    WrsnSeg tmp[WRSN_REC_MAXSEG]; int ns = 0;
    const int64_t want = rec_segments(h, r.has_gen, tmp, &ns);
    if (r.nseg != ns) return bad("nseg", r.nseg, ns);
    if (r.rec_bytes != want) return bad("rec_bytes", r.rec_bytes, want);
    if (!(r.prob_gp >= 0.0 && r.prob_gp <= 1.0) || (!r.has_gen && r.prob_gp != 1.0)) return fail(WRSN_ERR_ARG, "record " + std::to_string(i) + ": prob_gp out of range");
    return 0;
}

// host index arrays: every index in [0, B); `distinct`: no index twice; `filled`: every environment holds a scenario
int check_envs(const wrsn_handle* h, const int32_t* env, int32_t n, bool distinct, bool filled, const char* what) {
    std::vector<uint8_t> seen(distinct ? h->dev.B : 0, 0);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t e = env[i];
        if (e < 0 || e >= h->dev.B) return fail(WRSN_ERR_ARG, std::string(what) + "[" + std::to_string(i) + "] = " + std::to_string(e) + " is out of range");
        if (filled && !h->filled[e]) return fail(WRSN_ERR_ARG, std::string(what) + "[" + std::to_string(i) + "]: environment " + std::to_string(e) + " holds no scenario");
        if (distinct) { if (seen[e]) return fail(WRSN_ERR_ARG, std::string(what) + ": environment " + std::to_string(e) + " appears twice"); seen[e] = 1; }
    }
    return 0;
}

// room for `n` staged indices
int ensure_idx(wrsn_handle* h, size_t n) {
    if (n <= h->idx_cap) return 0;
    if (h->d_idx) HIPCHK(hipFree(h->d_idx));
    h->d_idx = nullptr; h->idx_cap = 0;
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, n * sizeof(int32_t)));
    h->d_idx = (int32_t*)q; h->idx_cap = n;
    return 0;
}

// the copy loop over n pairs, in launches of at most 2^30 chunks (32-bit chunk indices); grid capped at eight blocks per CU, grid-stride
int launch_rec_copy(wrsn_handle* h, int mode, const int32_t* src_env, const int32_t* dst_env, uint8_t* rec, int n) {
    const int chunks = (int)(h->rec_bytes / 16), per = chunks - WRSN_REC_HDR / 16;
    const int max_pairs = (1 << 30) / per > 0 ? (1 << 30) / per : 1;
    for (int i0 = 0; i0 < n; i0 += max_pairs) {
        const int m = n - i0 < max_pairs ? n - i0 : max_pairs;
        const long long need = ((long long)m * per + 255) / 256;
        const int blocks = (int)(need < (long long)h->cus * 8 ? need : (long long)h->cus * 8);
        hipLaunchKernelGGL(wrsn_rec_copy_kernel, dim3(blocks), dim3(256), (size_t)h->nseg * sizeof(WrsnSeg), h->stream, (const WrsnSeg*)h->d_segs, h->nseg,
                           mode, src_env, dst_env, rec, (long long)h->rec_bytes, i0, m, chunks);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// request rows of replaced environments (+ their observations when out->obs is set, their entity rows when registered)
int launch_rec_rows(wrsn_handle* h, const uint8_t* hdr, const int32_t* src_env, const int32_t* dst_env, int n, const wrsn_step_out* out) {
    const bool renders = out->obs || h->ent.node;
    if (renders) HIPCHK(hipMemsetAsync(h->d_rend, 0xFF, (size_t)h->dev.B * sizeof(int32_t), h->stream));
    hipLaunchKernelGGL(wrsn_rec_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->dev, hdr, (long long)WRSN_REC_HDR, (const int32_t*)nullptr, src_env, dst_env, n,
                       (const int32_t*)nullptr, step_out_dev(out), renders ? h->d_rend : (int32_t*)nullptr, -1, 0, h->d_pool_cur);
    HIPCHK(hipGetLastError());
    if (renders) return launch_render_all(h, h->d_rend, out->obs);
    return 0;
}

int set_scenario_impl(wrsn_t* h, int32_t env0, int32_t nenv, const double* node_xy, const double* target_xy,
                      const double* bs_xy, const int32_t* n_node_env, const int32_t* n_target_env,
                      const wrsn_node_spec* node_spec, int32_t node_spec_stride, const wrsn_mc_spec* mc_spec,
                      int32_t mc_spec_stride, const int64_t* seed);

}  // namespace

extern "C" {

const char* wrsn_last_error(void) { return g_err.c_str(); }
const char* wrsn_version(void) { return "wrsn_hip 0.1 (gfx950)"; }

int wrsn_create(const wrsn_cfg* cfg, wrsn_t** out) {
    if (!cfg || !out) return fail(WRSN_ERR_ARG, "null argument");
    *out = nullptr;
    if (cfg->n_env < 1 || cfg->n_node < 1 || cfg->n_target < 1 || cfg->n_mc < 1 || cfg->n_mc > WRSN_MAX_MC || cfg->map_size < 4 ||
        cfg->map_size > 128 || cfg->n_node > 1024 || !(cfg->warm_up_time > 0.0))
        return fail(WRSN_ERR_ARG, "wrsn_cfg out of range (n_mc 1..8, n_node 1..1024, map_size 4..128, warm_up_time > 0)");
    int ndev = 0;
    {
        const hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev <= 0)
            return fail(WRSN_ERR_NO_DEVICE, std::string("no HIP device: libwrsn_hip has no CPU fallback (hipGetDeviceCount: ") + hipGetErrorString(e) + ")");
    }
    if (cfg->device < 0 || cfg->device >= ndev) return fail(WRSN_ERR_ARG, "device ordinal out of range");
    DeviceGuard guard_(cfg->device);
    if (!guard_.ok) return fail(WRSN_ERR_HIP, "hipSetDevice failed");
    wrsn_handle* h = new wrsn_handle();
    h->cfg = *cfg;
    { const char* e = std::getenv("WRSN_PIPE"); h->pipe = (e && *e == '0') ? 0 : 1; }
    // the second stream: high priority where the device offers a priority range -- its launch is the SHORT half of a pipelined step call, whose
    // blocks should get wave slots first so that its observations can be rendered while the long half is still being stepped
    hipError_t se = hipErrorUnknown;
    int lo_p = 0, hi_p = 0;
    if (hipDeviceGetStreamPriorityRange(&lo_p, &hi_p) == hipSuccess && hi_p != lo_p) se = hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, hi_p);
    if (se != hipSuccess) se = hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking);
    if (se == hipSuccess && hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) == hipSuccess) {
        if (hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) == hipSuccess) h->ev2_ok = 1; else (void)hipEventDestroy(h->ev_fork);
    }
    { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, cfg->device) == hipSuccess && pr.multiProcessorCount > 0) h->cus = pr.multiProcessorCount; }
    h->npl = npl_for(cfg->n_node);
    if (h->npl < 0) { wrsn_destroy(h); return fail(WRSN_ERR_ARG, "n_node too large"); }
    WrsnDev& d = h->dev;
    d.B = cfg->n_env; d.N = cfg->n_node; d.T = cfg->n_target; d.M = cfg->n_mc; d.G = cfg->map_size;
    d.NP = h->npl * 64; d.TP = ((cfg->n_target + 63) / 64) * 64;
    d.ECAP = (cfg->max_degree > 0 ? cfg->max_degree : 24) * d.NP;
    d.CCAP = (cfg->max_cover > 0 ? cfg->max_cover : 8) * d.NP;
    // observation tile geometry must fit the register tile of wrsn_obs_kernel
    {
        int CG = (d.G + 3) / 4; int RG = 256 / CG; if (RG < 1) { wrsn_destroy(h); return fail(WRSN_ERR_ARG, "map_size too large"); }
        int RPG = (d.G + RG - 1) / RG; if (RPG > WRSN_OBS_MAXROWS) { wrsn_destroy(h); return fail(WRSN_ERR_ARG, "map_size too large for the observation tile"); }
    }
    d.CC = 4;                                                  // raised by wrsn_set_scenario to what the scenarios need
    h->lds_obs = wrsn_obs_lds_bytes(d.G, d.NP);
    const size_t B = d.B;
    int rc = 0;
    do {
        if ((rc = alloc_env_arrays(h, ENV_ARRAYS_DEV))) break;
        if ((rc = dalloc(h, &d.counters, B * 25))) break;
        { int p2 = 1; while (p2 < d.B) p2 <<= 1; h->bp2 = (d.B <= 8192 && p2 <= 8 * WRSN_SORT_THREADS) ? p2 : 0; }   // 8 keys per sort thread at most (launch_order)
        if ((rc = dalloc(h, &d.order_key, (size_t)(h->bp2 > 0 ? h->bp2 : 1)))) break;
        if ((rc = dalloc(h, &d.order, (size_t)(h->bp2 > d.B ? h->bp2 : d.B)))) break;
        if ((rc = dalloc(h, &d.launch_t0, 1))) break;
        if ((rc = dalloc(h, &d.render_agent, B))) break;
        if ((rc = dalloc(h, &d.row_state, B))) break;
        if ((rc = dalloc(h, &d.queue, 8 + 64))) break;
        if ((rc = dalloc(h, &d.qskip, B))) break;
        if ((rc = dalloc(h, &h->d_segs, WRSN_REC_MAXSEG))) break;
        if ((rc = dalloc(h, &h->d_hdr, B * WRSN_REC_HDR))) break;
        if ((rc = dalloc(h, &h->d_rend, B))) break;
        if ((rc = dalloc(h, &h->d_pool_cur, B))) break;
        if ((rc = dalloc(h, &h->d_pool_swaps, B))) break;
        if ((rc = dalloc(h, &h->d_pairs, 2 * B))) break;
        if ((rc = dalloc(h, &h->d_pair_n, 1))) break;
        {   // the descriptor the kernels read, and the stochastic block behind it (wrsn_sim.h: Sim::SD)
            uint8_t* p = nullptr;
            if ((rc = dalloc(h, &p, sizeof(WrsnDev) + sizeof(WrsnStochDev)))) break;
            h->d_dev = (WrsnDev*)p;
        }
    } while (0);
    if (rc) { wrsn_destroy(h); return rc; }
    {   // identity launch order: what a handle too large for the device-side sort keeps
        std::vector<int32_t> ident(B); for (size_t e = 0; e < B; ++e) ident[e] = (int32_t)e;
        if (hipMemcpy(d.order, ident.data(), B * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) { wrsn_destroy(h); return fail(WRSN_ERR_HIP, "hipMemcpy"); }
    }
    if ((rc = configure_launch(h))) { wrsn_destroy(h); return rc; }
    if (hipMemset(h->d_pool_cur, 0xFF, B * sizeof(int32_t)) != hipSuccess) { wrsn_destroy(h); return fail(WRSN_ERR_HIP, "hipMemset"); }
    h->filled.assign(B, 0);
    if (rec_layout(h) != 0 || ensure_idx(h, 2 * B) != 0) { wrsn_destroy(h); return fail(WRSN_ERR_HIP, "hipMemcpy"); }
    *out = h;
    return WRSN_OK;
}

void wrsn_destroy(wrsn_t* h) {
    if (!h) return;
    DeviceGuard guard_(h->cfg.device);
    if (h->ev_ok) for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    if (h->ev2_ok) { (void)hipEventDestroy(h->ev_fork); (void)hipEventDestroy(h->ev_join); }
    if (h->stream2) { (void)hipStreamSynchronize(h->stream2); (void)hipStreamDestroy(h->stream2); }
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->d_idx) (void)hipFree(h->d_idx);
    delete h;
}

int wrsn_set_stream(wrsn_t* h, void* hip_stream) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    h->stream = (hipStream_t)hip_stream;
    return WRSN_OK;
}

int wrsn_set_scenario(wrsn_t* h, int32_t env0, int32_t nenv, const double* node_xy, const double* target_xy,
                      const double* bs_xy, const int32_t* n_node_env, const int32_t* n_target_env,
                      const wrsn_node_spec* node_spec, int32_t node_spec_stride, const wrsn_mc_spec* mc_spec,
                      int32_t mc_spec_stride) {
    return set_scenario_impl(h, env0, nenv, node_xy, target_xy, bs_xy, n_node_env, n_target_env, node_spec, node_spec_stride, mc_spec,
                             mc_spec_stride, nullptr);
}

int wrsn_set_scenario_seeded(wrsn_t* h, int32_t env0, int32_t nenv, const double* node_xy, const double* target_xy,
                             const double* bs_xy, const int32_t* n_node_env, const int32_t* n_target_env,
                             const wrsn_node_spec* node_spec, int32_t node_spec_stride, const wrsn_mc_spec* mc_spec,
                             int32_t mc_spec_stride, const int64_t* seed) {
    if (!seed) return fail(WRSN_ERR_ARG, "null seed array");
    return set_scenario_impl(h, env0, nenv, node_xy, target_xy, bs_xy, n_node_env, n_target_env, node_spec, node_spec_stride, mc_spec,
                             mc_spec_stride, seed);
}

}  // extern "C"

namespace {

int set_scenario_impl(wrsn_t* h, int32_t env0, int32_t nenv, const double* node_xy, const double* target_xy,
                      const double* bs_xy, const int32_t* n_node_env, const int32_t* n_target_env,
                      const wrsn_node_spec* node_spec, int32_t node_spec_stride, const wrsn_mc_spec* mc_spec,
                      int32_t mc_spec_stride, const int64_t* seed) {
    if (!h || !node_xy || !target_xy || !bs_xy || !node_spec || !mc_spec) return fail(WRSN_ERR_ARG, "null argument");
    const WrsnDev& d = h->dev;
    if (env0 < 0 || nenv < 1 || env0 + nenv > d.B) return fail(WRSN_ERR_ARG, "environment range out of bounds");
    WRSN_ON_DEVICE(h);
    const size_t NP = d.NP, TP = d.TP;
    std::vector<double> hx(nenv * NP, 0.0), hy(nenv * NP, 0.0), tx(nenv * TP, 0.0), ty(nenv * TP, 0.0);
    std::vector<WrsnEnvConst> ec(nenv);
    for (int e = 0; e < nenv; ++e) {
        const int n = n_node_env ? n_node_env[e] : d.N, t = n_target_env ? n_target_env[e] : d.T;
        if (n < 1 || n > d.N || t < 1 || t > d.T) return fail(WRSN_ERR_ARG, "per-environment node/target count out of range");
        const wrsn_node_spec& ns = node_spec[(size_t)e * (node_spec_stride ? 1 : 0)];
        const wrsn_mc_spec& ms = mc_spec[(size_t)e * (mc_spec_stride ? 1 : 0)];
        if (ns.prob_gp != 1.0 && !seed)
            return fail(WRSN_ERR_ARG, "prob_gp != 1 needs wrsn_set_scenario_seeded (Node.py:61 draws Python's MT19937, seeded by NetworkIO.py:23)");
        if (!(ns.prob_gp >= 0.0 && ns.prob_gp <= 1.0)) return fail(WRSN_ERR_ARG, "prob_gp outside [0, 1]");
        for (int i = 0; i < n; ++i) { hx[e * NP + i] = node_xy[((size_t)e * d.N + i) * 2]; hy[e * NP + i] = node_xy[((size_t)e * d.N + i) * 2 + 1]; }
        for (int i = 0; i < t; ++i) { tx[e * TP + i] = target_xy[((size_t)e * d.T + i) * 2]; ty[e * TP + i] = target_xy[((size_t)e * d.T + i) * 2 + 1]; }
        WrsnEnvConst& c = ec[e];
        std::memset(&c, 0, sizeof(c));
        c.capacity = ns.capacity; c.threshold = ns.threshold; c.com_range = ns.com_range; c.sen_range = ns.sen_range;
        c.package_size = ns.package_size; c.er = ns.er; c.et = ns.et; c.efs = ns.efs; c.emp = ns.emp; c.max_time = ns.max_time;
        c.mc_capacity = ms.capacity; c.mc_threshold = ms.threshold; c.velocity = ms.velocity; c.pm = ms.pm;
        c.charging_range = ms.charging_range; c.alpha = ms.alpha; c.beta = ms.beta; c.epsilon = ms.epsilon;
        c.bs[0] = bs_xy[e * 2]; c.bs[1] = bs_xy[e * 2 + 1];
        c.warm_up_time = h->cfg.warm_up_time;
        c.n_node = n; c.n_target = t;
    }
    HIPCHK(hipMemcpy(d.node_x + (size_t)env0 * NP, hx.data(), hx.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.node_y + (size_t)env0 * NP, hy.data(), hy.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.target_x + (size_t)env0 * TP, tx.data(), tx.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.target_y + (size_t)env0 * TP, ty.data(), ty.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.ec + env0, ec.data(), ec.size() * sizeof(WrsnEnvConst), hipMemcpyHostToDevice));
    bool want_stoch = false;                                   // an environment of this call draws: the stochastic kernels from now on
    if (seed || h->sd.mt_live) {
        // prob_gp and the seeded generator of every environment of the range (random.seed(seed), NetworkIO.py:23); environments loaded
        // through wrsn_set_scenario keep prob_gp 1 and an all-zero state (their draws are counted, never used)
        int rc0 = alloc_stoch(h); if (rc0) return rc0;
        std::vector<double> pg(nenv); std::vector<uint32_t> mt((size_t)nenv * WRSN_MT_STRIDE, 0u);
        for (int e = 0; e < nenv; ++e) {
            const wrsn_node_spec& ns = node_spec[(size_t)e * (node_spec_stride ? 1 : 0)];
            pg[e] = seed ? ns.prob_gp : 1.0;
            if (seed) mt_seed(seed[e], mt.data() + (size_t)e * WRSN_MT_STRIDE);
            if (pg[e] != 1.0) want_stoch = true;
        }
        HIPCHK(hipMemcpy(h->sd.pgp + env0, pg.data(), (size_t)nenv * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->sd.mt_live + (size_t)env0 * WRSN_MT_STRIDE, mt.data(), mt.size() * 4, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(wrsn_topology_kernel, dim3(nenv), dim3(64), 0, h->stream, h->dev, env0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(ec.data(), d.ec + env0, ec.size() * sizeof(WrsnEnvConst), hipMemcpyDeviceToHost));
    for (int e = 0; e < nenv; ++e) {
        if (ec[e].error == -1) return fail(WRSN_ERR_CAPACITY, "neighbour list capacity exceeded (raise wrsn_cfg.max_degree); env " + std::to_string(env0 + e) + " has " + std::to_string(ec[e].n_edges) + " directed edges");
        if (ec[e].error == -2) return fail(WRSN_ERR_CAPACITY, "coverage list capacity exceeded (raise wrsn_cfg.max_cover); env " + std::to_string(env0 + e));
    }
    int conn_bound = 0;                                        // (WrsnEnvConst.conn_bound, wrsn_topology_kernel)
    for (int e = 0; e < nenv; ++e) if (ec[e].conn_bound > conn_bound) conn_bound = ec[e].conn_bound;
    int rc = fit_launch(h, conn_bound, want_stoch);
    if (rc) return rc;
    if ((rc = launch_warmup(h, env0, nenv))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemset(h->d_pool_cur + env0, 0xFF, (size_t)nenv * sizeof(int32_t)));   // these environments run no pool record
    h->scenario_set = 1;
    for (int e = 0; e < nenv; ++e) h->filled[env0 + e] = 1;
    return WRSN_OK;
}

}  // namespace

extern "C" {

int wrsn_reset(wrsn_t* h, const uint8_t* env_mask, const wrsn_step_out* out) {
    if (!h || !out) return fail(WRSN_ERR_ARG, "null argument");
    if (!h->scenario_set) return fail(WRSN_ERR_STATE, "wrsn_set_scenario has not been called");
    WRSN_ON_DEVICE(h);
    // rows of environments the mask leaves out keep every output, agent_id included; what the render pass draws comes
    // from the list the environment kernel writes (WrsnDev.render_agent), not from the caller's agent_id array
    return launch_reset(h, env_mask, step_out_dev(out));
}

int wrsn_step(wrsn_t* h, const int32_t* agent_id, const double* action, int32_t auto_reset, const wrsn_step_out* out) {
    if (!h || !out || !agent_id || !action) return fail(WRSN_ERR_ARG, "null argument");
    if (!h->scenario_set) return fail(WRSN_ERR_STATE, "wrsn_set_scenario has not been called");
    WRSN_ON_DEVICE(h);
    // rows with agent_id -2 keep every output (their pending request included)
    return launch_step(h, agent_id, action, auto_reset, step_out_dev(out));
}

int wrsn_set_obs_reuse(wrsn_t* h, int32_t on) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    h->obs_reuse = on ? 1 : 0;
    return WRSN_OK;
}

int wrsn_set_obs_format(wrsn_t* h, int32_t format) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    if (format != WRSN_OBS_F32 && format != WRSN_OBS_BF16) return fail(WRSN_ERR_ARG, "unknown observation format");
    h->obs_fmt = format;                                       // read at launch time: the launches enqueued so far keep theirs
    return WRSN_OK;
}

int wrsn_set_timing(wrsn_t* h, int32_t on) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    WRSN_ON_DEVICE(h);
    if (on && !h->ev_ok) {
        for (hipEvent_t& e : h->ev) HIPCHK(hipEventCreate(&e));
        h->ev_ok = 1;
    }
    if (!on || !h->timing) h->ev_mask = 0;
    h->timing = on ? 1 : 0;
    return WRSN_OK;
}

int wrsn_kernel_times(wrsn_t* h, float* ms) {
    if (!h || !ms) return fail(WRSN_ERR_ARG, "null argument");
    if (!h->ev_ok || !h->timing) return fail(WRSN_ERR_STATE, "wrsn_set_timing(h, 1) first");
    if (!h->ev_mask) return fail(WRSN_ERR_STATE, "no wrsn_step has run since wrsn_set_timing(h, 1)");
    WRSN_ON_DEVICE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    ms[0] = ms[1] = ms[2] = ms[3] = 0.f;
    HIPCHK(hipEventElapsedTime(&ms[0], h->ev[0], h->ev[1]));
    HIPCHK(hipEventElapsedTime(&ms[1], h->ev[1], h->ev[2]));
    if (h->ev_mask & (1 << 3)) HIPCHK(hipEventElapsedTime(&ms[3], h->ev[2], h->ev[3]));   // the call rendered; ms[2] stays 0
    return WRSN_OK;
}

int wrsn_set_step_budget(wrsn_t* h, int32_t work_units) {
    if (!h || work_units < 0) return fail(WRSN_ERR_ARG, "bad step budget");
    WRSN_ON_DEVICE(h);
    h->step_budget = work_units;
    return WRSN_OK;
}

int wrsn_set_step_deadline(wrsn_t* h, int32_t microseconds) {
    if (!h || microseconds < 0 || microseconds > 10000000) return fail(WRSN_ERR_ARG, "bad step deadline");
    h->deadline_ticks = microseconds * 100;                    // wall_clock64 counts at 100 MHz
    return WRSN_OK;
}

int wrsn_density_action(wrsn_t* h, const int32_t* agent_id, const double* dmap, double* action) {
    if (!h || !agent_id || !dmap || !action) return fail(WRSN_ERR_ARG, "null argument");
    if (!h->scenario_set) return fail(WRSN_ERR_STATE, "wrsn_set_scenario has not been called");
    WRSN_ON_DEVICE(h);
    // np.percentile(map, 99.9), method "linear": virtual index (n - 1) q, the two order statistics around it and the weight
    const int n = h->dev.G * h->dev.G;
    const double q = 99.9 / 100.0, vi = (double)(n - 1) * q, lo = std::floor(vi);
    const int n_top = n - (int)lo;                              // elements from the lower order statistic to the maximum
    if (n_top < 1 || n_top > WRSN_DM_KMAX) return fail(WRSN_ERR_ARG, "map size out of range for the percentile selection");
    hipLaunchKernelGGL(wrsn_density_kernel, dim3(h->dev.B), dim3(64), wrsn_density_lds_bytes(), h->stream, h->dev, agent_id, dmap, action,
                       n_top, vi - lo);
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int wrsn_rollout_table(wrsn_t* h, double* dst, int32_t zero_after) {
    if (!h || !dst) return fail(WRSN_ERR_ARG, "null argument");
    if (!h->scenario_set) return fail(WRSN_ERR_STATE, "wrsn_set_scenario has not been called");
    WRSN_ON_DEVICE(h);
    hipLaunchKernelGGL(wrsn_rollout_kernel, dim3((h->dev.B + 255) / 256), dim3(256), 0, h->stream, h->dev, dst, (int)zero_after);
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

static int tr_buffers(const wrsn_transition_buffers* b, WrsnTrBuffers* t) {
    if (!b || b->capacity < 1 || b->action_elems < 1 || !b->pend_state || !b->pend_action || !b->pend_logp || !b->pend_valid || !b->state ||
        !b->action || !b->next_state || !b->reward || !b->logp || !b->now || !b->env || !b->count)
        return fail(WRSN_ERR_ARG, "wrsn_transition_buffers: null pointer or empty geometry");
    t->capacity = b->capacity; t->action_elems = b->action_elems;
    t->pend_state = b->pend_state; t->pend_action = b->pend_action; t->pend_logp = b->pend_logp; t->pend_valid = b->pend_valid;
    t->state = b->state; t->action = b->action; t->next_state = b->next_state; t->reward = b->reward; t->logp = b->logp;
    t->now = b->now; t->env = b->env; t->count = b->count;
    return 0;
}

static int obs_elem_bytes(const wrsn_t* h) { return h->obs_fmt == WRSN_OBS_BF16 ? 2 : 4; }   // of the rows the image copy kernels move

int wrsn_rollout_record(wrsn_t* h, const wrsn_transition_buffers* buf, const int32_t* agent_id, const float* action, const float* logp,
                        const float* obs) {
    if (!h || !agent_id || !action || !logp || !obs) return fail(WRSN_ERR_ARG, "null argument");
    WrsnTrBuffers t; int rc = tr_buffers(buf, &t); if (rc) return rc;
    WRSN_ON_DEVICE(h);
    hipLaunchKernelGGL(wrsn_tr_record_kernel, dim3(h->dev.B), dim3(256), 0, h->stream, h->dev.B, h->dev.M, h->dev.G, t, agent_id, action, logp, obs, obs_elem_bytes(h));
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int wrsn_rollout_collect(wrsn_t* h, const wrsn_transition_buffers* buf, const wrsn_step_out* out) {
    if (!h || !out || !out->agent_id || !out->reward || !out->terminal || !out->now || !out->status || !out->obs)
        return fail(WRSN_ERR_ARG, "wrsn_rollout_collect needs every wrsn_step_out field");
    WrsnTrBuffers t; int rc = tr_buffers(buf, &t); if (rc) return rc;
    WRSN_ON_DEVICE(h);
    hipLaunchKernelGGL(wrsn_tr_collect_kernel, dim3(h->dev.B), dim3(256), 16, h->stream, h->dev.B, h->dev.M, h->dev.G, t, out->agent_id,
                       out->reward, out->now, h->dev.row_state, out->obs, obs_elem_bytes(h));
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int wrsn_render(wrsn_t* h, const int32_t* agent_id, float* obs) {
    if (!h || !agent_id || !obs) return fail(WRSN_ERR_ARG, "null argument");
    if (!h->scenario_set) return fail(WRSN_ERR_STATE, "wrsn_set_scenario has not been called");
    WRSN_ON_DEVICE(h);
    launch_obs(h, h->stream, agent_id, obs, nullptr, 0, h->dev.B);   // the image alone: entity rows of arbitrary agents are wrsn_entities
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

static int entity_out(const wrsn_entity_out* ent, WrsnEntityOut* e) {
    if (!ent->node || !ent->mc || !ent->env) return fail(WRSN_ERR_ARG, "wrsn_entity_out: node, mc and env must all be given");
    if (((uintptr_t)ent->node | (uintptr_t)ent->mc | (uintptr_t)ent->env) % 16) return fail(WRSN_ERR_ARG, "wrsn_entity_out: node, mc and env must be 16-byte aligned");
    e->node = ent->node; e->mc = ent->mc; e->env = ent->env;
    return 0;
}

int wrsn_set_entity_out(wrsn_t* h, const wrsn_entity_out* ent) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    WrsnEntityOut e{};
    if (ent) { const int rc = entity_out(ent, &e); if (rc) return rc; }
    h->ent = e;                                                // read at launch time: the launches enqueued so far keep theirs
    return WRSN_OK;
}

int wrsn_entities(wrsn_t* h, const int32_t* agent_id, const wrsn_entity_out* ent) {
    if (!h || !agent_id || !ent) return fail(WRSN_ERR_ARG, "null argument");
    if (!h->scenario_set) return fail(WRSN_ERR_STATE, "wrsn_set_scenario has not been called");
    WrsnEntityOut e{}; const int rc = entity_out(ent, &e); if (rc) return rc;
    WRSN_ON_DEVICE(h);
    launch_entities(h, h->stream, agent_id, nullptr, 0, h->dev.B, &e);
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

// The entity buffers a call reads: those of `ent`, checked, or with ent == NULL the registered ones.
static int entity_in(const wrsn_t* h, const wrsn_entity_out* ent, WrsnEntityOut* e) {
    if (ent) return entity_out(ent, e);
    if (!h->ent.node) return fail(WRSN_ERR_ARG, "no entity buffers: pass wrsn_entity_out or register them with wrsn_set_entity_out");
    *e = h->ent;
    return 0;
}

// Entity transition rows: the buffers of `ent` (NULL: the registered ones) and the three row pointers of the transition buffers, all
// checked before anything is enqueued or changed.
static int tr_entity_args(wrsn_t* h, const wrsn_transition_buffers* buf, const wrsn_entity_out* ent, WrsnTrBuffers* t, WrsnEntityOut* e) {
    int rc = entity_in(h, ent, e); if (rc) return rc;
    rc = tr_buffers(buf, t); if (rc) return rc;
    if (((uintptr_t)t->pend_state | (uintptr_t)t->state | (uintptr_t)t->next_state) % 16)
        return fail(WRSN_ERR_ARG, "wrsn_transition_buffers: pend_state, state and next_state of entity rows must be 16-byte aligned");
    return 0;
}

static dim3 entity_row_grid(int B) { return dim3((B + WRSN_ENT_ROWS - 1) / WRSN_ENT_ROWS); }   // of blocks of 64 * WRSN_ENT_ROWS: a wave per row

int wrsn_rollout_record_entities(wrsn_t* h, const wrsn_transition_buffers* buf, const int32_t* agent_id, const float* action, const float* logp,
                                 const wrsn_entity_out* ent) {
    if (!h || !agent_id || !action || !logp) return fail(WRSN_ERR_ARG, "null argument");
    WrsnTrBuffers t; WrsnEntityOut e{};
    const int rc = tr_entity_args(h, buf, ent, &t, &e); if (rc) return rc;
    WRSN_ON_DEVICE(h);
    const int B = h->dev.B;
    hipLaunchKernelGGL(wrsn_tr_record_entities_kernel, entity_row_grid(B), dim3(64 * WRSN_ENT_ROWS), 0, h->stream, B, h->dev.M,
                       h->dev.N, t, agent_id, action, logp, e);
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int wrsn_rollout_collect_entities(wrsn_t* h, const wrsn_transition_buffers* buf, const wrsn_step_out* out, const wrsn_entity_out* ent, int32_t consume) {
    if (!h || !out || !out->agent_id || !out->reward || !out->terminal || !out->now || !out->status)   // out->obs may be NULL: entity-only batches
        return fail(WRSN_ERR_ARG, "wrsn_rollout_collect_entities needs agent_id, reward, terminal, now and status of wrsn_step_out");
    WrsnTrBuffers t; WrsnEntityOut e{};
    const int rc = tr_entity_args(h, buf, ent, &t, &e); if (rc) return rc;
    WRSN_ON_DEVICE(h);
    const int B = h->dev.B;
    hipLaunchKernelGGL(wrsn_tr_collect_entities_kernel, entity_row_grid(B), dim3(64 * WRSN_ENT_ROWS), 0, h->stream, B, h->dev.M,
                       h->dev.N, t, out->agent_id, out->reward, out->now, h->dev.row_state, e, (int)(consume != 0));
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int32_t wrsn_entity_actor_floats(void) { return WRSN_EP_FLOATS; }

int wrsn_entity_act(wrsn_t* h, const float* actors, const int32_t* agent_id, const float* eps, const wrsn_entity_out* ent,
                    const wrsn_entity_act_out* out) {
    if (!h || !actors || !agent_id || !out || !out->action || !out->logp)
        return fail(WRSN_ERR_ARG, "wrsn_entity_act needs actors, agent_id, out->action and out->logp");
    WrsnEntityOut e{};
    { const int rc = entity_in(h, ent, &e); if (rc) return rc; }
    if ((uintptr_t)actors % 16) return fail(WRSN_ERR_ARG, "wrsn_entity_act: actors must be 16-byte aligned");
    WRSN_ON_DEVICE(h);
    const int B = h->dev.B, M = h->dev.M;
    if (!h->ep_cnt) {
        int rc = dalloc(h, &h->ep_feat, (size_t)B * WRSN_ENTPOL_FEAT);
        if (!rc) rc = dalloc(h, &h->ep_list, (size_t)B * M);
        if (!rc) rc = dalloc(h, &h->ep_cnt, (size_t)WRSN_MAX_MC);
        if (rc) return rc;
    }
    WrsnEntActOut o; o.action = out->action; o.action_f64 = out->action_f64; o.logp = out->logp; o.mean = out->mean; o.log_std = out->log_std;
    HIPCHK(hipMemsetAsync(h->ep_cnt, 0, WRSN_MAX_MC * sizeof(int32_t), h->stream));
    hipLaunchKernelGGL(wrsn_entpol_group_kernel, dim3((B + 63) / 64), dim3(64), 0, h->stream, B, M, agent_id, h->ep_list, h->ep_cnt);
    hipLaunchKernelGGL(wrsn_entpol_trunk_kernel, dim3(B), dim3(256), WRSN_EP_T_LDS, h->stream, B, M, h->dev.N, actors, agent_id, e, h->ep_feat,
                       (int)WRSN_EP_FLOATS);
    hipLaunchKernelGGL(wrsn_entpol_head_kernel, dim3((B + WRSN_EP_HEAD_ROWS - 1) / WRSN_EP_HEAD_ROWS + M), dim3(256), WRSN_EP_H_LDS, h->stream, B, M,
                       actors, (const float*)h->ep_feat, (const int32_t*)h->ep_list, (const int32_t*)h->ep_cnt, eps, o);
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int32_t wrsn_entity_pointer_floats(void) { return WRSN_PP_FLOATS; }

int wrsn_entity_pointer_act(wrsn_t* h, const float* actors, const int32_t* agent_id, const float* gumbel, const float* eps, float min_charge,
                            const wrsn_entity_out* ent, const wrsn_entity_pointer_out* out) {
    if (!h || !actors || !agent_id || !out || !out->node || !out->stored || !out->action || !out->logp)
        return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_act needs actors, agent_id, out->node, out->stored, out->action and out->logp");
    if (!(min_charge >= 0.f && min_charge < 1.f)) return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_act: min_charge must lie in [0, 1)");   // a NaN fails both
    WrsnEntityOut e{};
    { const int rc = entity_in(h, ent, &e); if (rc) return rc; }
    if ((uintptr_t)actors % 16) return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_act: actors must be 16-byte aligned");
    WRSN_ON_DEVICE(h);
    const int B = h->dev.B, M = h->dev.M, N = h->dev.N;
    if (!h->ep_cnt) {                                         // the scratch of wrsn_entity_act: the two calls share it, in stream order
        int rc = dalloc(h, &h->ep_feat, (size_t)B * WRSN_ENTPOL_FEAT);
        if (!rc) rc = dalloc(h, &h->ep_list, (size_t)B * M);
        if (!rc) rc = dalloc(h, &h->ep_cnt, (size_t)WRSN_MAX_MC);
        if (rc) return rc;
    }
    if (!h->pp_z) {
        int rc = dalloc(h, &h->pp_z, (size_t)B * 128);
        if (!rc) rc = dalloc(h, &h->pp_q, (size_t)B * 64);
        if (rc) return rc;
    }
    WrsnEntPtrOut o; o.node = out->node; o.stored = out->stored; o.action = out->action; o.action_f64 = out->action_f64; o.logp = out->logp;
    o.node_logp = out->node_logp; o.charge_mean = out->charge_mean; o.charge_log_std = out->charge_log_std;
    HIPCHK(hipMemsetAsync(h->ep_cnt, 0, WRSN_MAX_MC * sizeof(int32_t), h->stream));
    hipLaunchKernelGGL(wrsn_entpol_group_kernel, dim3((B + 63) / 64), dim3(64), 0, h->stream, B, M, agent_id, h->ep_list, h->ep_cnt);
    hipLaunchKernelGGL(wrsn_entpol_trunk_kernel, dim3(B), dim3(256), WRSN_EP_T_LDS, h->stream, B, M, N, actors, agent_id, e, h->ep_feat,
                       (int)WRSN_PP_FLOATS);
    hipLaunchKernelGGL(wrsn_entptr_head_kernel, dim3((B + WRSN_EP_HEAD_ROWS - 1) / WRSN_EP_HEAD_ROWS + M), dim3(256), WRSN_EP_H_LDS, h->stream, B, M,
                       actors, (const float*)h->ep_feat, (const int32_t*)h->ep_list, (const int32_t*)h->ep_cnt, h->pp_z, h->pp_q);
    hipLaunchKernelGGL(wrsn_entptr_score_kernel, dim3(B), dim3(256), WRSN_PP_SCORE_LDS(N), h->stream, B, M, N, actors, agent_id, e,
                       (const float*)h->pp_z, (const float*)h->pp_q, gumbel, eps, min_charge, o, h->ptr_mask);
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int wrsn_set_entity_pointer_mask(wrsn_t* h, int32_t mode) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    if (mode != WRSN_POINTER_MASK_NONE && mode != WRSN_POINTER_MASK_CLAIMED) return fail(WRSN_ERR_ARG, "unknown node-pointer mask");
    h->ptr_mask = mode;                                        // read at launch time: the launches enqueued so far keep theirs
    return WRSN_OK;
}

int wrsn_entity_heuristic_act(wrsn_t* h, const int32_t* agent_id, const wrsn_entity_out* ent, float charge_scale, float* action, double* action_f64) {
    if (!h || !agent_id || !action) return fail(WRSN_ERR_ARG, "wrsn_entity_heuristic_act needs agent_id and action");
    WrsnEntityOut e{};
    { const int rc = entity_in(h, ent, &e); if (rc) return rc; }
    WRSN_ON_DEVICE(h);
    const int B = h->dev.B;
    hipLaunchKernelGGL(wrsn_entity_heuristic_kernel, entity_row_grid(B), dim3(64 * WRSN_ENT_ROWS), 0, h->stream, B, h->dev.M, h->dev.N, agent_id, e,
                       charge_scale, action, action_f64);
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int wrsn_entity_heuristic_label(wrsn_t* h, const int32_t* agent_id, const wrsn_entity_out* ent, float charge_scale, float min_charge, float x_clip,
                                float* stored, float* action, double* action_f64) {
    if (!h || !agent_id || !stored) return fail(WRSN_ERR_ARG, "wrsn_entity_heuristic_label needs agent_id and stored");
    if (!std::isfinite(min_charge) || min_charge < 0.f || min_charge >= 1.f)
        return fail(WRSN_ERR_ARG, "wrsn_entity_heuristic_label: min_charge must be finite and in [0, 1)");
    if (!std::isfinite(x_clip) || x_clip <= 0.f) return fail(WRSN_ERR_ARG, "wrsn_entity_heuristic_label: x_clip must be finite and > 0");
    WrsnEntityOut e{};
    { const int rc = entity_in(h, ent, &e); if (rc) return rc; }
    WRSN_ON_DEVICE(h);
    const int B = h->dev.B;
    hipLaunchKernelGGL(wrsn_entity_heuristic_label_kernel, entity_row_grid(B), dim3(64 * WRSN_ENT_ROWS), 0, h->stream, B, h->dev.M, h->dev.N, agent_id, e,
                       charge_scale, min_charge, x_clip, stored, action, action_f64);
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int wrsn_episodes_collect(wrsn_t* h, const wrsn_episode_log* log, const wrsn_step_out* out, double time_limit, int32_t* next_agent_id,
                          uint8_t* restart, int32_t consume) {
    if (!h || !log || !out) return fail(WRSN_ERR_ARG, "null argument");
    if (!log->run_return || !log->run_decisions || !log->finished || !log->dropped || !log->lifetime || !log->ep_return || !log->decisions || !log->ended)
        return fail(WRSN_ERR_ARG, "wrsn_episode_log: every array but record is required");
    if (!out->agent_id || !out->reward || !out->now || !out->status)
        return fail(WRSN_ERR_ARG, "wrsn_episodes_collect needs agent_id, reward, now and status of wrsn_step_out");
    if (log->episodes < 1) return fail(WRSN_ERR_ARG, "wrsn_episode_log: episodes must be at least 1");
    if (log->quota < 0 || log->quota > log->episodes) return fail(WRSN_ERR_ARG, "wrsn_episode_log: quota must lie in [0, episodes]");
    if (next_agent_id == out->agent_id) return fail(WRSN_ERR_ARG, "wrsn_episodes_collect: next_agent_id must not be out->agent_id");
    WrsnEpisodeLog L;
    L.episodes = log->episodes; L.quota = log->quota; L.run_return = log->run_return; L.run_decisions = log->run_decisions;
    L.finished = log->finished; L.dropped = log->dropped; L.lifetime = log->lifetime; L.ep_return = log->ep_return;
    L.decisions = log->decisions; L.ended = log->ended; L.record = log->record;
    WRSN_ON_DEVICE(h);
    const int B = h->dev.B;
    hipLaunchKernelGGL(wrsn_episodes_kernel, dim3((B + 255) / 256), dim3(256), 0, h->stream, B, h->dev.M, L, (const int32_t*)out->agent_id,
                       (const double*)out->reward, (const double*)out->now, (const int32_t*)out->status, h->dev.row_state,
                       (const int32_t*)h->d_pool_cur, time_limit, next_agent_id, restart, (int)(consume != 0));
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

// ------------------------------------------------------------------ the PPO update of the entity policy (wrsn_entity_train.h)
int32_t wrsn_entity_critic_floats(void) { return WRSN_EC_FLOATS; }

namespace {
const char* entity_rows_bad(const wrsn_entity_rows* r) {
    if (!r || !r->rows) return "rows and rows->rows are required";
    if ((uintptr_t)r->rows % 16) return "rows->rows must be 16-byte aligned";
    if (r->n < 1) return "n must be >= 1";
    if (r->n_mc < 1 || r->n_mc > WRSN_MAX_MC) return "n_mc must be in [1, 8]";
    if (r->n_node < 1) return "n_node must be >= 1";
    return nullptr;
}
// group 0's slice of the scratch area for G groups of n rows; group g's lies g * s->chunk floats behind it
int entity_scratch(wrsn_handle* h, int n, bool grad, int G, WrsnEtScratch* s) {
    s->chunk = wrsn_et_scratch_floats((size_t)n, grad);
    const size_t need = (size_t)G * s->chunk;
    if (need > h->et_cap) {
        const int rc = dalloc(h, &h->et_scratch, need);
        if (rc) return rc;
        h->et_cap = need;
    }
    float* p = h->et_scratch;
    const size_t q = 2 * (size_t)n;
    s->feat = p; p += q * WRSN_ENTPOL_FEAT; s->arg = p; p += q * 64; s->cnt = p; p += q * 4; s->z1 = p; p += q * 128; s->z2 = p; p += q * 128;
    s->raw = p; p += 8 * (size_t)n;
    s->dz1 = s->dz2 = s->dfeat = s->part = s->dout = nullptr;
    if (grad) {
        s->dz1 = p; p += q * 128; s->dz2 = p; p += q * 128; s->dfeat = p; p += q * WRSN_ENTPOL_FEAT; s->part = p; p += q * WRSN_ET_TRUNK_FLOATS;
        s->dout = p; p += 8 * (size_t)n;
    }
    return 0;
}
void entity_forward(wrsn_handle* h, const WrsnEtGroups& gs, int G, const WrsnEtDims& dm, const WrsnEtScratch& s, const WrsnEtEvalOut& o) {
    hipLaunchKernelGGL(wrsn_et_trunk_fwd_kernel, dim3(2 * G * dm.n), dim3(256), WRSN_ET_T_LDS, h->stream, gs, dm, s);
    hipLaunchKernelGGL(wrsn_et_head_fwd_kernel, dim3(2 * G * ((dm.n + WRSN_EP_HEAD_ROWS - 1) / WRSN_EP_HEAD_ROWS)), dim3(256), WRSN_EP_H_LDS, h->stream,
                       gs, dm.n, s, o);
}
// one gradient step of G groups: six launches however large G is.  Arguments are checked by the callers.
int entity_grad_launch(wrsn_handle* h, const WrsnEtGroups& gs, int G, const WrsnEtDims& dm, const WrsnEtHyper& hp) {
    WrsnEtScratch s;
    { const int rc = entity_scratch(h, dm.n, true, G, &s); if (rc) return rc; }
    WrsnEtEvalOut o; o.mean = nullptr; o.log_std = nullptr; o.value = nullptr;
    const int n = dm.n;
    entity_forward(h, gs, G, dm, s, o);
    hipLaunchKernelGGL(wrsn_et_loss_kernel, dim3(G), dim3(256), 256 * sizeof(double), h->stream, gs, n, hp, s);
    hipLaunchKernelGGL(wrsn_et_head_bwd_kernel, dim3(2 * G * n), dim3(256), 256 * sizeof(float), h->stream, gs, n, s);
    hipLaunchKernelGGL(wrsn_et_trunk_bwd_kernel, dim3(2 * G * n), dim3(256), WRSN_ET_B_LDS, h->stream, gs, dm, s);
    hipLaunchKernelGGL(wrsn_et_reduce_kernel, dim3(2 * G * ((WRSN_EP_FLOATS + 255) / 256)), dim3(256), 0, h->stream, gs, n, s);
    return 0;
}
// entry k of an Adam table: the block, and the bias corrections of `step` formed in double and rounded once
void entity_adam_block(WrsnEtAdamBlocks* bs, int k, float* p, const float* g, float* m, float* v, float* norm_out, int nf, int step, float lr, float beta1,
                       float beta2) {
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step), bc2 = 1.0 - std::pow((double)beta2, (double)step);
    WrsnEtAdamBlock& b = bs->b[k];
    b.p = p; b.g = g; b.m = m; b.v = v; b.norm_out = norm_out; b.nf = nf;
    b.step_size = (float)((double)lr / bc1); b.inv_sqrt_bc2 = (float)(1.0 / std::sqrt(bc2));
}
// one Adam step on the nb blocks of the table: two launches.  max_nf: the floats of the largest block
int entity_adam_launch(wrsn_handle* h, const WrsnEtAdamBlocks& bs, int nb, int max_nf, float beta1, float beta2, float eps, float max_norm) {
    if (!h->et_norm) { const int rc = dalloc(h, &h->et_norm, (size_t)(2 * WRSN_MAX_MC)); if (rc) return rc; }
    const int per = (max_nf + 255) / 256;
    hipLaunchKernelGGL(wrsn_et_norm_kernel, dim3(nb), dim3(256), 256 * sizeof(double), h->stream, bs, h->et_norm);
    hipLaunchKernelGGL(wrsn_et_adam_kernel, dim3(nb * per), dim3(256), 0, h->stream, bs, per, (const float*)h->et_norm, beta1, beta2,
                       (float)(1.0 - (double)beta1), (float)(1.0 - (double)beta2), eps, max_norm);
    return 0;
}
WrsnEtHyper entity_hyper(const wrsn_ppo_hyper* hyper) {
    WrsnEtHyper hp; hp.clip = hyper->clip; hp.ent_coef = hyper->ent_coef; hp.vf_coef = hyper->vf_coef; hp.norm_adv = hyper->norm_adv != 0;
    hp.clip_vloss = hyper->clip_vloss != 0;
    return hp;
}
// what is wrong with the G groups of a multi call, or nullptr.  batch: the gradient's inputs are needed; moments: Adam's; critic: the
// call has a critic side (a call without one looks at the actor's side of a group alone, and of its batch at the stored pairs)
const char* groups_bad(const wrsn_entity_group* groups, int G, bool batch, bool moments, bool critic) {
    if (G < 1 || G > WRSN_MAX_MC) return "n_groups must be in [1, 8]";
    if (!groups) return "groups is required";
    const void* named[WRSN_MAX_MC][8];
    const int sides = critic ? 2 : 1, per = moments ? 4 : 2, nn = sides * per;
    for (int g = 0; g < G; ++g) {
        const wrsn_entity_group& q = groups[g];
        if (!q.actor || !q.grad_actor || (critic && (!q.critic || !q.grad_critic)))
            return critic ? "every group needs actor, critic, grad_actor and grad_critic" : "every group needs actor and grad_actor";
        if ((uintptr_t)q.actor % 16 || (uintptr_t)q.grad_actor % 16 || (critic && ((uintptr_t)q.critic % 16 || (uintptr_t)q.grad_critic % 16)))
            return "blocks and gradient buffers must be 16-byte aligned";
        if (batch) {
            if (!q.rows || !q.batch.action || (critic && (!q.batch.logp_old || !q.batch.advantage || !q.batch.ret || !q.batch.value_old)))
                return critic ? "every group needs rows and every batch array" : "every group needs rows and the stored pairs (batch.action)";
            if ((uintptr_t)q.rows % 16) return "rows must be 16-byte aligned";
        }
        if (moments) {
            if (!q.m_actor || !q.v_actor || (critic && (!q.m_critic || !q.v_critic)))
                return critic ? "every group needs m_actor, v_actor, m_critic and v_critic" : "every group needs m_actor and v_actor";
            if ((uintptr_t)q.m_actor % 16 || (uintptr_t)q.v_actor % 16 || (critic && ((uintptr_t)q.m_critic % 16 || (uintptr_t)q.v_critic % 16)))
                return "moments must be 16-byte aligned";
            if (q.adam_step < 0) return "adam_step must be >= 0";
        }
        const void* mine[2][4] = {{q.actor, q.grad_actor, q.m_actor, q.v_actor}, {q.critic, q.grad_critic, q.m_critic, q.v_critic}};
        for (int k = 0; k < nn; ++k) {                        // the 2, 4 or 8 buffers the call names: none of them in an earlier group
            const void* mk = mine[k / per][k % per];
            for (int g2 = 0; g2 < g; ++g2)
                for (int k2 = 0; k2 < nn; ++k2)
                    if (named[g2][k2] == mk) return "two groups name the same block, moment or gradient buffer";
            named[g][k] = mk;
        }
    }
    return nullptr;
}
const char* entity_dims_bad(int n, int n_node, int n_mc) {
    if (n < 1) return "n must be >= 1";
    if (n_mc < 1 || n_mc > WRSN_MAX_MC) return "n_mc must be in [1, 8]";
    if (n_node < 1) return "n_node must be >= 1";
    return nullptr;
}
WrsnEtDims dims_of(int n, int n_node, int n_mc) { WrsnEtDims dm; dm.n = n; dm.N = n_node; dm.M = n_mc; return dm; }
// the table of a single-group call
WrsnEtGroups one_group(const float* actor, const float* critic, const wrsn_entity_rows* rows, WrsnEtBatch b = WrsnEtBatch{}, float* grad_actor = nullptr,
                       float* grad_critic = nullptr, float* stats = nullptr) {
    WrsnEtGroups gs{};
    WrsnEtGroup& G = gs.g[0];
    G.actor = actor; G.critic = critic; G.grad_actor = grad_actor; G.grad_critic = grad_critic; G.rows = rows->rows; G.index = rows->index; G.b = b;
    G.stats = stats;
    return gs;
}
}  // namespace

int wrsn_entity_eval(wrsn_t* h, const float* actor, const float* critic, const wrsn_entity_rows* rows, float* mean, float* log_std, float* value) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    if (const char* bad = entity_rows_bad(rows)) return fail(WRSN_ERR_ARG, std::string("wrsn_entity_eval: ") + bad);
    if (!actor && !critic) return fail(WRSN_ERR_ARG, "wrsn_entity_eval needs an actor or a critic");
    if ((actor && !mean && !log_std) || (critic && !value)) return fail(WRSN_ERR_ARG, "wrsn_entity_eval: a net that is given needs an output");
    if ((!actor && (mean || log_std)) || (!critic && value)) return fail(WRSN_ERR_ARG, "wrsn_entity_eval: outputs of a net that is not given must be NULL");
    if ((uintptr_t)actor % 16 || (uintptr_t)critic % 16) return fail(WRSN_ERR_ARG, "wrsn_entity_eval: blocks must be 16-byte aligned");
    WRSN_ON_DEVICE(h);
    WrsnEtScratch s;
    { const int rc = entity_scratch(h, rows->n, false, 1, &s); if (rc) return rc; }
    WrsnEtEvalOut o; o.mean = mean; o.log_std = log_std; o.value = value;
    entity_forward(h, one_group(actor, critic, rows), 1, dims_of(rows->n, rows->n_node, rows->n_mc), s, o);
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int wrsn_entity_ppo_grad(wrsn_t* h, const float* actor, const float* critic, const wrsn_entity_rows* rows, const wrsn_ppo_batch* batch,
                         const wrsn_ppo_hyper* hyper, float* grad_actor, float* grad_critic, float* stats) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    if (const char* bad = entity_rows_bad(rows)) return fail(WRSN_ERR_ARG, std::string("wrsn_entity_ppo_grad: ") + bad);
    if (!actor || !critic || !batch || !hyper || !grad_actor || !grad_critic || !stats || !batch->action || !batch->logp_old || !batch->advantage ||
        !batch->ret || !batch->value_old)
        return fail(WRSN_ERR_ARG, "wrsn_entity_ppo_grad needs actor, critic, every batch array, hyper, grad_actor, grad_critic and stats");
    if ((uintptr_t)actor % 16 || (uintptr_t)critic % 16 || (uintptr_t)grad_actor % 16 || (uintptr_t)grad_critic % 16)
        return fail(WRSN_ERR_ARG, "wrsn_entity_ppo_grad: blocks and gradient buffers must be 16-byte aligned");
    if (hyper->norm_adv && rows->n < 2) return fail(WRSN_ERR_ARG, "wrsn_entity_ppo_grad: norm_adv needs n >= 2");
    WRSN_ON_DEVICE(h);
    const WrsnEtBatch b{batch->action, batch->logp_old, batch->advantage, batch->ret, batch->value_old};
    const WrsnEtGroups gs = one_group(actor, critic, rows, b, grad_actor, grad_critic, stats);
    if (const int rc = entity_grad_launch(h, gs, 1, dims_of(rows->n, rows->n_node, rows->n_mc), entity_hyper(hyper))) return rc;
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int wrsn_entity_adam(wrsn_t* h, float* param, const float* grad, float* m, float* v, int32_t n_floats, int32_t step, float lr, float beta1,
                     float beta2, float eps, float max_norm, float* norm_out) {
    if (!h || !param || !grad || !m || !v) return fail(WRSN_ERR_ARG, "wrsn_entity_adam needs param, grad, m and v");
    if ((uintptr_t)param % 16 || (uintptr_t)grad % 16 || (uintptr_t)m % 16 || (uintptr_t)v % 16)
        return fail(WRSN_ERR_ARG, "wrsn_entity_adam: param, grad, m and v must be 16-byte aligned");
    if (n_floats < 1) return fail(WRSN_ERR_ARG, "wrsn_entity_adam: n_floats must be >= 1");
    if (step < 1) return fail(WRSN_ERR_ARG, "wrsn_entity_adam: step must be >= 1");
    WRSN_ON_DEVICE(h);
    WrsnEtAdamBlocks bs{};
    entity_adam_block(&bs, 0, param, grad, m, v, norm_out, (int)n_floats, (int)step, lr, beta1, beta2);
    if (const int rc = entity_adam_launch(h, bs, 1, (int)n_floats, beta1, beta2, eps, max_norm)) return rc;
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

// ------------------------------------------------------------------ the PPO gradient of the node-pointer policy (wrsn_entity_pointer_train.h)
namespace {
// the set policy's scratch for G groups of n rows, and behind it what the pointer kernels keep: G slices, group 0's first (with G = 1 it
// sits right behind the one set-policy slice), group g's ps->chunk floats behind it
int pointer_scratch(wrsn_handle* h, int n, int N, bool grad, int G, WrsnEtScratch* s, WrsnEtpScratch* ps) {
    const size_t et = (size_t)G * wrsn_et_scratch_floats((size_t)n, grad);
    ps->chunk = wrsn_etp_scratch_floats((size_t)n, N, grad);
    const size_t need = et + (size_t)G * ps->chunk;
    if (need > h->et_cap) {
        const int rc = dalloc(h, &h->et_scratch, need);
        if (rc) return rc;
        h->et_cap = need;
    }
    { const int rc = entity_scratch(h, n, grad, G, s); if (rc) return rc; }
    float* p = h->et_scratch + et;
    ps->ld = (N + 31) & ~31;
    ps->q = p; p += (size_t)n * 64; ps->lp = p; p += (size_t)n * ps->ld; ps->prow = p; p += (size_t)n * 8;
    ps->dq = ps->dch = ps->part2 = nullptr;
    if (grad) { ps->dq = p; p += (size_t)n * 64; ps->dch = p; p += (size_t)n * 4; ps->part2 = p; p += (size_t)n * WRSN_EP_MC1; }
    return 0;
}
// trunk and heads of both nets, then -- with an actor -- the query and the scores of the stored decisions
// stored: wrsn_entity_pointer_eval's decisions (G = 1); NULL: every group's b.action.  A call without an actor is the eval of a critic alone.
void pointer_forward(wrsn_handle* h, const WrsnEtGroups& gs, int G, const WrsnEtDims& dm, const WrsnEtScratch& s, const WrsnEtpScratch& ps,
                     const float* stored, float* value, const WrsnEtpEvalOut& o, int mask) {
    WrsnEtEvalOut eo; eo.mean = nullptr; eo.log_std = nullptr; eo.value = value;
    entity_forward(h, gs, G, dm, s, eo);
    if (!gs.g[0].actor) return;
    hipLaunchKernelGGL(wrsn_etp_query_kernel, dim3(G * ((dm.n + WRSN_EP_HEAD_ROWS - 1) / WRSN_EP_HEAD_ROWS)), dim3(256), 128 * 32 * sizeof(float), h->stream,
                       gs, dm.n, s, ps);
    hipLaunchKernelGGL(wrsn_etp_score_fwd_kernel, dim3(G * dm.n), dim3(256), WRSN_PP_SCORE_LDS(dm.N), h->stream, gs, dm, s, ps, stored, o, mask);
}
// one gradient step of G groups: ten launches however large G is.  The pointer-only per-row kernels run G * n blocks (the actor's rows),
// the shared ones 2 * G * n.  Arguments are checked by the callers.
int pointer_grad_launch(wrsn_handle* h, const WrsnEtGroups& gs, int G, const WrsnEtDims& dm, const WrsnEtHyper& hp, int mask) {
    WrsnEtScratch s; WrsnEtpScratch ps;
    { const int rc = pointer_scratch(h, dm.n, dm.N, true, G, &s, &ps); if (rc) return rc; }
    const int n = dm.n;
    pointer_forward(h, gs, G, dm, s, ps, nullptr, nullptr, WrsnEtpEvalOut{}, mask);
    hipLaunchKernelGGL(wrsn_etp_loss_kernel, dim3(G), dim3(256), 256 * sizeof(double), h->stream, gs, n, hp, s, ps);
    hipLaunchKernelGGL(wrsn_etp_score_bwd_kernel, dim3(G * n), dim3(256), WRSN_ETP_BWD_LDS(dm.N), h->stream, gs, dm, s, ps);
    hipLaunchKernelGGL(wrsn_etp_head_bwd_kernel, dim3(2 * G * n), dim3(256), 256 * sizeof(float), h->stream, gs, n, s);
    hipLaunchKernelGGL(wrsn_et_trunk_bwd_kernel, dim3(2 * G * n), dim3(256), WRSN_ET_B_LDS, h->stream, gs, dm, s);
    hipLaunchKernelGGL(wrsn_etp_trunk_bwd_kernel, dim3(G * n), dim3(256), WRSN_ET_B_LDS, h->stream, gs, dm, s, ps);
    hipLaunchKernelGGL(wrsn_etp_reduce_kernel, dim3(2 * G * ((WRSN_PP_FLOATS + 255) / 256)), dim3(256), 0, h->stream, gs, dm, s, ps);
    return 0;
}
// group g's slices of the two scratch areas, formed on the host (wrsn_et_slice / wrsn_etp_slice)
WrsnEtScratch host_slice(WrsnEtScratch s, int g) {
    const size_t o = (size_t)g * s.chunk;
    s.feat += o; s.arg += o; s.cnt += o; s.z1 += o; s.z2 += o; s.dz1 += o; s.dz2 += o; s.dfeat += o; s.part += o; s.raw += o; s.dout += o;
    return s;
}
WrsnEtpScratch host_slice_ptr(WrsnEtpScratch ps, int g) {
    const size_t o = (size_t)g * ps.chunk;
    ps.q += o; ps.lp += o; ps.prow += o; ps.dq += o; ps.dch += o; ps.part2 += o;
    return ps;
}
// one behaviour-cloning gradient step of G groups: pointer_grad_launch with wrsn_etp_bc_loss_kernel for the loss and, for the three
// kernels whose grid carries (group, net), one launch per group on the actor half alone.  7 + 3 G launches.  Arguments are checked by the callers.
int pointer_bc_launch(wrsn_handle* h, const WrsnEtGroups& gs, int G, const WrsnEtDims& dm, float ent_coef, int mask) {
    WrsnEtScratch s; WrsnEtpScratch ps;
    { const int rc = pointer_scratch(h, dm.n, dm.N, true, G, &s, &ps); if (rc) return rc; }
    const int n = dm.n;
    pointer_forward(h, gs, G, dm, s, ps, nullptr, nullptr, WrsnEtpEvalOut{}, mask);
    hipLaunchKernelGGL(wrsn_etp_bc_loss_kernel, dim3(G), dim3(256), 256 * sizeof(double), h->stream, gs, n, dm.N, ent_coef, s, ps);
    hipLaunchKernelGGL(wrsn_etp_score_bwd_kernel, dim3(G * n), dim3(256), WRSN_ETP_BWD_LDS(dm.N), h->stream, gs, dm, s, ps);
    for (int g = 0; g < G; ++g) {
        WrsnEtGroups one{};
        one.g[0] = gs.g[g];
        const WrsnEtScratch sg = host_slice(s, g);
        hipLaunchKernelGGL(wrsn_etp_head_bwd_kernel, dim3(n), dim3(256), 256 * sizeof(float), h->stream, one, n, sg);
        hipLaunchKernelGGL(wrsn_et_trunk_bwd_kernel, dim3(n), dim3(256), WRSN_ET_B_LDS, h->stream, one, dm, sg);
    }
    hipLaunchKernelGGL(wrsn_etp_trunk_bwd_kernel, dim3(G * n), dim3(256), WRSN_ET_B_LDS, h->stream, gs, dm, s, ps);
    for (int g = 0; g < G; ++g) {
        WrsnEtGroups one{};
        one.g[0] = gs.g[g];
        hipLaunchKernelGGL(wrsn_etp_reduce_kernel, dim3((WRSN_PP_FLOATS + 255) / 256), dim3(256), 0, h->stream, one, dm, host_slice(s, g), host_slice_ptr(ps, g));
    }
    return 0;
}
}  // namespace

int wrsn_entity_pointer_eval(wrsn_t* h, const float* actor, const float* critic, const wrsn_entity_rows* rows, const float* stored, float* logp,
                             float* entropy, float* node_logp, float* charge_mean, float* charge_log_std, float* value) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    if (const char* bad = entity_rows_bad(rows)) return fail(WRSN_ERR_ARG, std::string("wrsn_entity_pointer_eval: ") + bad);
    if (!actor && !critic) return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_eval needs an actor or a critic");
    if (actor && !stored) return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_eval: an actor needs stored");
    if ((actor && !logp && !entropy && !node_logp && !charge_mean && !charge_log_std) || (critic && !value))
        return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_eval: a net that is given needs an output");
    if ((!actor && (logp || entropy || node_logp || charge_mean || charge_log_std)) || (!critic && value))
        return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_eval: outputs of a net that is not given must be NULL");
    if ((uintptr_t)actor % 16 || (uintptr_t)critic % 16) return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_eval: blocks must be 16-byte aligned");
    if (WRSN_PP_SCORE_LDS(rows->n_node) > 65536) return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_eval: too many nodes for the score block's LDS");
    WRSN_ON_DEVICE(h);
    WrsnEtScratch s; WrsnEtpScratch ps;
    { const int rc = pointer_scratch(h, rows->n, rows->n_node, false, 1, &s, &ps); if (rc) return rc; }
    WrsnEtpEvalOut o; o.logp = logp; o.entropy = entropy; o.node_logp = node_logp; o.charge_mean = charge_mean; o.charge_log_std = charge_log_std;
    pointer_forward(h, one_group(actor, critic, rows), 1, dims_of(rows->n, rows->n_node, rows->n_mc), s, ps, stored, value, o, h->ptr_mask);
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int wrsn_entity_pointer_ppo_grad(wrsn_t* h, const float* actor, const float* critic, const wrsn_entity_rows* rows, const wrsn_pointer_batch* batch,
                                 const wrsn_ppo_hyper* hyper, float* grad_actor, float* grad_critic, float* stats) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    if (const char* bad = entity_rows_bad(rows)) return fail(WRSN_ERR_ARG, std::string("wrsn_entity_pointer_ppo_grad: ") + bad);
    if (!actor || !critic || !batch || !hyper || !grad_actor || !grad_critic || !stats || !batch->stored || !batch->logp_old || !batch->advantage ||
        !batch->ret || !batch->value_old)
        return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_ppo_grad needs actor, critic, every batch array, hyper, grad_actor, grad_critic and stats");
    if ((uintptr_t)actor % 16 || (uintptr_t)critic % 16 || (uintptr_t)grad_actor % 16 || (uintptr_t)grad_critic % 16)
        return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_ppo_grad: blocks and gradient buffers must be 16-byte aligned");
    if (hyper->norm_adv && rows->n < 2) return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_ppo_grad: norm_adv needs n >= 2");
    if (WRSN_ETP_BWD_LDS(rows->n_node) > 65536) return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_ppo_grad: too many nodes for the score block's LDS");
    WRSN_ON_DEVICE(h);
    const WrsnEtBatch b{batch->stored, batch->logp_old, batch->advantage, batch->ret, batch->value_old};
    const WrsnEtGroups gs = one_group(actor, critic, rows, b, grad_actor, grad_critic, stats);
    if (const int rc = pointer_grad_launch(h, gs, 1, dims_of(rows->n, rows->n_node, rows->n_mc), entity_hyper(hyper), h->ptr_mask)) return rc;
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

// ------------------------------------------------------------------ behaviour cloning of the node-pointer actor (wrsn_entity_pointer_train.h,
// at its end): the PPO calls' kernels on a group table without critics, one new loss kernel, Adam on the actor blocks alone
int wrsn_entity_pointer_bc_grad(wrsn_t* h, const float* actor, const wrsn_entity_rows* rows, const float* stored, float ent_coef, float* grad_actor,
                                float* stats) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    if (const char* bad = entity_rows_bad(rows)) return fail(WRSN_ERR_ARG, std::string("wrsn_entity_pointer_bc_grad: ") + bad);
    if (!actor || !stored || !grad_actor || !stats) return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_bc_grad needs actor, stored, grad_actor and stats");
    if ((uintptr_t)actor % 16 || (uintptr_t)grad_actor % 16)
        return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_bc_grad: the block and the gradient buffer must be 16-byte aligned");
    if (!std::isfinite(ent_coef)) return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_bc_grad: ent_coef must be finite");
    if (WRSN_ETP_BWD_LDS(rows->n_node) > 65536) return fail(WRSN_ERR_ARG, "wrsn_entity_pointer_bc_grad: too many nodes for the score block's LDS");
    WRSN_ON_DEVICE(h);
    WrsnEtBatch b{}; b.action = stored;
    const WrsnEtGroups gs = one_group(actor, nullptr, rows, b, grad_actor, nullptr, stats);
    if (const int rc = pointer_bc_launch(h, gs, 1, dims_of(rows->n, rows->n_node, rows->n_mc), ent_coef, h->ptr_mask)) return rc;
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

// ------------------------------------------------------------------ the multi-group calls of the three training kinds: one host path
namespace {
// What tells the set policy's PPO, the node-pointer policy's PPO and the node-pointer actor's cloning apart on the host.  A new training
// kind is a new entry here and a new case in grad_step.
enum GradLaunch { GRAD_SET_PPO, GRAD_POINTER_PPO, GRAD_POINTER_BC };
struct TrainKind {
    int actor_floats;      // WRSN_EP_FLOATS (set block) or WRSN_PP_FLOATS (pointer block)
    bool critic;           // the groups have a critic side and the call takes a wrsn_ppo_hyper; without: the actor alone and an ent_coef
    GradLaunch grad;       // entity_grad_launch, pointer_grad_launch or pointer_bc_launch
    bool lds_limit;        // n_node is bounded by the score block's LDS
};
const TrainKind SET_PPO{WRSN_EP_FLOATS, true, GRAD_SET_PPO, false}, POINTER_PPO{WRSN_PP_FLOATS, true, GRAD_POINTER_PPO, true},
    POINTER_BC{WRSN_PP_FLOATS, false, GRAD_POINTER_BC, true};

// one gradient step of G groups; hp: entity_hyper of the call's hyper, of a cloning call only its ent_coef
int grad_step(wrsn_handle* h, const TrainKind& K, const WrsnEtGroups& gs, int G, const WrsnEtDims& dm, const WrsnEtHyper& hp, int mask) {
    switch (K.grad) {
    case GRAD_SET_PPO: return entity_grad_launch(h, gs, G, dm, hp);
    case GRAD_POINTER_PPO: return pointer_grad_launch(h, gs, G, dm, hp, mask);
    default: return pointer_bc_launch(h, gs, G, dm, hp.ent_coef, mask);
    }
}
WrsnEtHyper kind_hyper(const TrainKind& K, const wrsn_ppo_hyper* hyper, float ent_coef) {
    if (K.critic) return entity_hyper(hyper);
    WrsnEtHyper hp{}; hp.ent_coef = ent_coef;
    return hp;
}
// the device table of the groups for one step: minibatch rows index + g * index_stride (NULL: rows 0 .. n - 1), statistics stats + g *
// stats_stride.  Without a critic no kernel sees a critic, its gradient buffer or the PPO batch arrays, whatever the caller's group names.
void group_table(const TrainKind& K, const wrsn_entity_group* groups, int G, const int32_t* index, size_t index_stride, float* stats, size_t stats_stride,
                 WrsnEtGroups* gs) {
    for (int g = 0; g < G; ++g) {
        const wrsn_entity_group& q = groups[g];
        WrsnEtGroup& d = gs->g[g];
        d.actor = q.actor; d.grad_actor = q.grad_actor; d.rows = q.rows; d.b.action = q.batch.action;
        if (K.critic) {
            d.critic = q.critic; d.grad_critic = q.grad_critic;
            d.b.logp_old = q.batch.logp_old; d.b.advantage = q.batch.advantage; d.b.ret = q.batch.ret; d.b.value_old = q.batch.value_old;
        }
        d.index = index ? index + (size_t)g * index_stride : nullptr;
        d.stats = stats + (size_t)g * stats_stride;
    }
}
// the Adam table of the groups, group g at adam_step + 1 + step_offset, and its number of entries: with a critic 2 G, the actor at 2 g and
// the critic at 2 g + 1; without, the G actor blocks
int adam_table(const TrainKind& K, const wrsn_entity_group* groups, int G, int step_offset, const wrsn_adam_hyper* a, WrsnEtAdamBlocks* bs) {
    const int per = K.critic ? 2 : 1;
    for (int g = 0; g < G; ++g) {
        const wrsn_entity_group& q = groups[g];
        const int step = q.adam_step + 1 + step_offset;
        entity_adam_block(bs, per * g, q.actor, q.grad_actor, q.m_actor, q.v_actor, nullptr, K.actor_floats, step, a->lr, a->beta1, a->beta2);
        if (K.critic) entity_adam_block(bs, 2 * g + 1, q.critic, q.grad_critic, q.m_critic, q.v_critic, nullptr, WRSN_EC_FLOATS, step, a->lr, a->beta1, a->beta2);
    }
    return per * G;
}
int adam_step(wrsn_handle* h, const TrainKind& K, const wrsn_entity_group* groups, int G, int step_offset, const wrsn_adam_hyper* a) {
    WrsnEtAdamBlocks bs{};
    const int nb = adam_table(K, groups, G, step_offset, a, &bs);
    return entity_adam_launch(h, bs, nb, K.actor_floats, a->beta1, a->beta2, a->eps, a->max_norm);
}
// the arguments a kind's calls share, beyond the groups: fn names the exported function in the messages
int kind_args_bad(const TrainKind& K, const char* fn, int n, int n_node, int n_mc, float ent_coef) {
    const std::string at = std::string(fn) + ": ";
    if (const char* bad = entity_dims_bad(n, n_node, n_mc)) return fail(WRSN_ERR_ARG, at + bad);
    if (!K.critic && !std::isfinite(ent_coef)) return fail(WRSN_ERR_ARG, at + "ent_coef must be finite");
    if (K.lds_limit && WRSN_ETP_BWD_LDS(n_node) > 65536) return fail(WRSN_ERR_ARG, at + "too many nodes for the score block's LDS");
    return 0;
}

int grad_multi(wrsn_t* h, const TrainKind& K, const char* fn, const wrsn_entity_group* groups, int n_groups, int n, int n_node, int n_mc,
               const int32_t* index, const wrsn_ppo_hyper* hyper, float ent_coef, float* stats) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    const std::string at = std::string(fn) + ": ";
    if (const char* bad = groups_bad(groups, n_groups, true, false, K.critic)) return fail(WRSN_ERR_ARG, at + bad);
    if ((K.critic && !hyper) || !stats) return fail(WRSN_ERR_ARG, std::string(fn) + (K.critic ? " needs hyper and stats" : " needs stats"));
    if (const int rc = kind_args_bad(K, fn, n, n_node, n_mc, ent_coef)) return rc;
    if (K.critic && hyper->norm_adv && n < 2) return fail(WRSN_ERR_ARG, at + "norm_adv needs n >= 2");
    WRSN_ON_DEVICE(h);
    WrsnEtGroups gs{};
    group_table(K, groups, n_groups, index, (size_t)n, stats, 8, &gs);
    if (const int rc = grad_step(h, K, gs, n_groups, dims_of(n, n_node, n_mc), kind_hyper(K, hyper, ent_coef), h->ptr_mask)) return rc;
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int adam_multi(wrsn_t* h, const TrainKind& K, const char* fn, const wrsn_entity_group* groups, int n_groups, const wrsn_adam_hyper* adam) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    if (const char* bad = groups_bad(groups, n_groups, false, true, K.critic)) return fail(WRSN_ERR_ARG, std::string(fn) + ": " + bad);
    if (!adam) return fail(WRSN_ERR_ARG, std::string(fn) + " needs the Adam hyper-parameters");
    WRSN_ON_DEVICE(h);
    if (const int rc = adam_step(h, K, groups, n_groups, 0, adam)) return rc;
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

// epochs x ceil(batch_size / minibatch) steps of gradient and Adam for every group: the whole of a kind's update call
int update_loop(wrsn_t* h, const TrainKind& K, const char* fn, const wrsn_entity_group* groups, int n_groups, int n_node, int n_mc, const int32_t* index,
                int batch_size, int minibatch, int epochs, const wrsn_ppo_hyper* hyper, float ent_coef, const wrsn_adam_hyper* adam, float* stats) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    const std::string at = std::string(fn) + ": ";
    if (const char* bad = groups_bad(groups, n_groups, true, true, K.critic)) return fail(WRSN_ERR_ARG, at + bad);
    if (batch_size < 1 || minibatch < 1 || epochs < 1) return fail(WRSN_ERR_ARG, at + "batch_size, minibatch and epochs must be >= 1");
    if (!index || (K.critic && !hyper) || !adam || !stats)
        return fail(WRSN_ERR_ARG, std::string(fn) + (K.critic ? " needs index, hyper, adam and stats" : " needs index, adam and stats"));
    if (const int rc = kind_args_bad(K, fn, batch_size, n_node, n_mc, ent_coef)) return rc;
    const int per_epoch = (int)(((int64_t)batch_size + minibatch - 1) / minibatch);
    const int64_t steps64 = (int64_t)per_epoch * epochs;
    if (steps64 > INT32_MAX) return fail(WRSN_ERR_ARG, at + "too many steps");
    const int steps = (int)steps64, n_full = minibatch < batch_size ? minibatch : batch_size, n_last = batch_size - (per_epoch - 1) * minibatch;
    if (K.critic && hyper->norm_adv && (n_full < 2 || n_last < 2)) return fail(WRSN_ERR_ARG, at + "norm_adv needs every minibatch to hold >= 2 rows");
    WRSN_ON_DEVICE(h);
    {   // the scratch area of the largest step and Adam's norms, so that no step of the loop allocates
        WrsnEtScratch s; WrsnEtpScratch ps;
        int rc = K.grad == GRAD_SET_PPO ? entity_scratch(h, n_full, true, n_groups, &s) : pointer_scratch(h, n_full, n_node, true, n_groups, &s, &ps);
        if (!rc && !h->et_norm) rc = dalloc(h, &h->et_norm, (size_t)(2 * WRSN_MAX_MC));
        if (rc) return rc;
    }
    const WrsnEtHyper hp = kind_hyper(K, hyper, ent_coef);
    const int mask = h->ptr_mask;                             // read once: every step of the loop under the same mask
    int k = 0;
    for (int e = 0; e < epochs; ++e)
        for (int start = 0; start < batch_size; start += minibatch, ++k) {   // only enqueues: nothing is read back, nothing synchronises
            WrsnEtGroups gs{};
            group_table(K, groups, n_groups, index + (size_t)e * batch_size + start, (size_t)epochs * batch_size, stats + (size_t)k * 8, (size_t)steps * 8, &gs);
            const int n = batch_size - start < minibatch ? batch_size - start : minibatch;
            if (const int rc = grad_step(h, K, gs, n_groups, dims_of(n, n_node, n_mc), hp, mask)) return rc;
            if (const int rc = adam_step(h, K, groups, n_groups, k, adam)) return rc;
        }
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}
}  // namespace

int wrsn_entity_ppo_grad_multi(wrsn_t* h, const wrsn_entity_group* groups, int32_t n_groups, int32_t n, int32_t n_node, int32_t n_mc,
                               const int32_t* index, const wrsn_ppo_hyper* hyper, float* stats) {
    return grad_multi(h, SET_PPO, "wrsn_entity_ppo_grad_multi", groups, n_groups, n, n_node, n_mc, index, hyper, 0.f, stats);
}
int wrsn_entity_adam_multi(wrsn_t* h, const wrsn_entity_group* groups, int32_t n_groups, const wrsn_adam_hyper* adam) {
    return adam_multi(h, SET_PPO, "wrsn_entity_adam_multi", groups, n_groups, adam);
}
int wrsn_entity_ppo_update(wrsn_t* h, const wrsn_entity_group* groups, int32_t n_groups, int32_t n_node, int32_t n_mc, const int32_t* index,
                           int32_t batch_size, int32_t minibatch, int32_t epochs, const wrsn_ppo_hyper* hyper, const wrsn_adam_hyper* adam,
                           float* stats) {
    return update_loop(h, SET_PPO, "wrsn_entity_ppo_update", groups, n_groups, n_node, n_mc, index, batch_size, minibatch, epochs, hyper, 0.f, adam, stats);
}

int wrsn_entity_pointer_ppo_grad_multi(wrsn_t* h, const wrsn_entity_group* groups, int32_t n_groups, int32_t n, int32_t n_node, int32_t n_mc,
                                       const int32_t* index, const wrsn_ppo_hyper* hyper, float* stats) {
    return grad_multi(h, POINTER_PPO, "wrsn_entity_pointer_ppo_grad_multi", groups, n_groups, n, n_node, n_mc, index, hyper, 0.f, stats);
}
int wrsn_entity_pointer_adam_multi(wrsn_t* h, const wrsn_entity_group* groups, int32_t n_groups, const wrsn_adam_hyper* adam) {
    return adam_multi(h, POINTER_PPO, "wrsn_entity_pointer_adam_multi", groups, n_groups, adam);
}
int wrsn_entity_pointer_ppo_update(wrsn_t* h, const wrsn_entity_group* groups, int32_t n_groups, int32_t n_node, int32_t n_mc, const int32_t* index,
                                   int32_t batch_size, int32_t minibatch, int32_t epochs, const wrsn_ppo_hyper* hyper, const wrsn_adam_hyper* adam,
                                   float* stats) {
    return update_loop(h, POINTER_PPO, "wrsn_entity_pointer_ppo_update", groups, n_groups, n_node, n_mc, index, batch_size, minibatch, epochs, hyper, 0.f,
                       adam, stats);
}

int wrsn_entity_pointer_bc_grad_multi(wrsn_t* h, const wrsn_entity_group* groups, int32_t n_groups, int32_t n, int32_t n_node, int32_t n_mc,
                                      const int32_t* index, float ent_coef, float* stats) {
    return grad_multi(h, POINTER_BC, "wrsn_entity_pointer_bc_grad_multi", groups, n_groups, n, n_node, n_mc, index, nullptr, ent_coef, stats);
}
int wrsn_entity_pointer_bc_update(wrsn_t* h, const wrsn_entity_group* groups, int32_t n_groups, int32_t n_node, int32_t n_mc, const int32_t* index,
                                  int32_t batch_size, int32_t minibatch, int32_t epochs, float ent_coef, const wrsn_adam_hyper* adam, float* stats) {
    return update_loop(h, POINTER_BC, "wrsn_entity_pointer_bc_update", groups, n_groups, n_node, n_mc, index, batch_size, minibatch, epochs, nullptr, ent_coef,
                       adam, stats);
}

namespace {
// what is wrong with the G groups of wrsn_entity_prepare, or nullptr
const char* prepare_groups_bad(const wrsn_prepare_group* groups, int G) {
    if (G < 1 || G > WRSN_MAX_MC) return "n_groups must be in [1, 8]";
    if (!groups) return "groups is required";
    const void* named[WRSN_MAX_MC * 8];
    int nn = 0;
    for (int g = 0; g < G; ++g) {
        const wrsn_prepare_group& q = groups[g];
        if (!q.critic || !q.state || !q.next_state || !q.reward || !q.value || !q.advantage || !q.ret)
            return "every group needs critic, state, next_state, reward, value, advantage and ret";
        if ((q.out_action && !q.action) || (q.out_logp && !q.logp)) return "an output is given whose source is NULL";
        if ((uintptr_t)q.critic % 16 || (uintptr_t)q.state % 16 || (uintptr_t)q.next_state % 16 || (uintptr_t)q.out_state % 16 ||
            (uintptr_t)q.out_next_state % 16)
            return "the critic block, state, next_state, out_state and out_next_state must be 16-byte aligned";
        const void* mine[8] = {q.value, q.advantage, q.ret, q.out_state, q.out_next_state, q.out_action, q.out_logp, q.out_reward};
        for (int k = 0; k < 8; ++k) {
            if (!mine[k]) continue;
            for (int k2 = 0; k2 < nn; ++k2)
                if (named[k2] == mine[k]) return "two groups name the same output buffer";
            named[nn++] = mine[k];
        }
    }
    return nullptr;
}
}  // namespace

int wrsn_entity_prepare(wrsn_t* h, const wrsn_prepare_group* groups, int32_t n_groups, int32_t n, int32_t n_node, int32_t n_mc, const int32_t* index,
                        float gamma, float gae_lambda) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    if (const char* bad = prepare_groups_bad(groups, n_groups)) return fail(WRSN_ERR_ARG, std::string("wrsn_entity_prepare: ") + bad);
    if (const char* bad = entity_dims_bad(n, n_node, n_mc)) return fail(WRSN_ERR_ARG, std::string("wrsn_entity_prepare: ") + bad);
    if (!std::isfinite(gamma) || !std::isfinite(gae_lambda)) return fail(WRSN_ERR_ARG, "wrsn_entity_prepare: gamma and gae_lambda must be finite");
    WRSN_ON_DEVICE(h);
    const int G = n_groups;
    WrsnEtScratch s;
    { const int rc = entity_scratch(h, n, false, 2 * G, &s); if (rc) return rc; }
    WrsnEtGroups gs{};                                        // two row sets per group: its critic on `state` and on `next_state`
    WrsnEtPrepGroups ps{};
    for (int g = 0; g < G; ++g) {
        const wrsn_prepare_group& q = groups[g];
        for (int k = 0; k < 2; ++k) {
            WrsnEtGroup& d = gs.g[2 * g + k];
            d.critic = q.critic; d.rows = k ? q.next_state : q.state; d.index = index ? index + (size_t)g * n : nullptr;
        }
        WrsnEtPrepGroup& p = ps.g[g];
        p.state = q.state; p.next_state = q.next_state; p.reward = q.reward; p.terminal = q.terminal; p.action = q.action; p.logp = q.logp;
        p.value = q.value; p.advantage = q.advantage; p.ret = q.ret; p.out_state = q.out_state; p.out_next_state = q.out_next_state;
        p.out_action = q.out_action; p.out_logp = q.out_logp; p.out_reward = q.out_reward;
    }
    WrsnEtEvalOut o; o.mean = nullptr; o.log_std = nullptr; o.value = nullptr;
    entity_forward(h, gs, 2 * G, dims_of(n, n_node, n_mc), s, o);
    const int row_u4 = (WRSN_ENT_NODE_F * n_node + WRSN_ENT_MC_F * n_mc + WRSN_ENT_ENV_F) / 4;   // R is a multiple of 4 floats
    hipLaunchKernelGGL(wrsn_et_prepare_kernel, dim3((unsigned)G * ((unsigned)n + 1u)), dim3(256), WRSN_ET_PREP_LDS, h->stream, ps, (int)n, row_u4, index,
                       gamma, (float)((double)gamma * (double)gae_lambda), s);
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int wrsn_sync(wrsn_t* h) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    WRSN_ON_DEVICE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    return WRSN_OK;
}

int wrsn_peek(wrsn_t* h, int32_t what, void* dst) {
    if (!h || !dst) return fail(WRSN_ERR_ARG, "null argument");
    const WrsnDev& d = h->dev;
    const size_t B = d.B, NP = d.NP, N = d.N;
    WRSN_ON_DEVICE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    auto node_f64 = [&](const double* src) -> int {
        std::vector<double> tmp(B * NP);
        HIPCHK(hipMemcpy(tmp.data(), src, tmp.size() * 8, hipMemcpyDeviceToHost));
        double* o = (double*)dst;
        for (size_t e = 0; e < B; ++e) for (size_t i = 0; i < N; ++i) o[e * N + i] = tmp[e * NP + i];
        return 0;
    };
    auto node_i32 = [&](const int32_t* src, int mode) -> int {
        std::vector<int32_t> tmp(B * NP);
        HIPCHK(hipMemcpy(tmp.data(), src, tmp.size() * 4, hipMemcpyDeviceToHost));
        int32_t* o = (int32_t*)dst;
        for (size_t e = 0; e < B; ++e)
            for (size_t i = 0; i < N; ++i) {
                int32_t v = tmp[e * NP + i];
                o[e * N + i] = mode == 0 ? v : (mode == 1 ? (v & 1) : ((v >> 1) - 1));
            }
        return 0;
    };
    switch (what) {
    case WRSN_PEEK_NODE_ENERGY: return node_f64(d.live.E);
    case WRSN_PEEK_NODE_CS: return node_f64(d.live.CS);
    case WRSN_PEEK_NODE_RR: return node_f64(d.live.RR);
    case WRSN_PEEK_NODE_STATUS: return node_i32(d.live.ls, 1);
    case WRSN_PEEK_NODE_LEVEL: return node_i32(d.live.ls, 2);
    case WRSN_PEEK_NODE_NCOVER: return node_i32(d.ncov, 0);
    case WRSN_PEEK_NODE_DIRECT: return node_i32(d.nflags, 1);
    case WRSN_PEEK_NODE_DEGREE: {
        std::vector<int32_t> tmp(B * (NP + 1));
        HIPCHK(hipMemcpy(tmp.data(), d.nb_off, tmp.size() * 4, hipMemcpyDeviceToHost));
        int32_t* o = (int32_t*)dst;
        for (size_t e = 0; e < B; ++e) for (size_t i = 0; i < N; ++i) o[e * N + i] = tmp[e * (NP + 1) + i + 1] - tmp[e * (NP + 1) + i];
        return 0; }
    case WRSN_PEEK_MC: {
        std::vector<WrsnEnvDyn> dy(B);
        HIPCHK(hipMemcpy(dy.data(), d.live.dyn, B * sizeof(WrsnEnvDyn), hipMemcpyDeviceToHost));
        double* o = (double*)dst;
        for (size_t e = 0; e < B; ++e)
            for (int m = 0; m < d.M; ++m) {
                const WrsnAgent& a = dy[e].ag[m]; double* q = o + (e * d.M + m) * 16;
                q[0] = a.loc[0]; q[1] = a.loc[1]; q[2] = a.energy; q[3] = a.status; q[4] = a.type_charging;
                q[5] = a.cur[0]; q[6] = a.cur[1]; q[7] = a.cur[2]; q[8] = a.n_conn; q[9] = a.excl; q[10] = a.prev_minfit;
                q[11] = a.action[0]; q[12] = a.action[1]; q[13] = a.action[2]; q[14] = dy[e].error; q[15] = dy[e].frozen ? -1.0 : (double)dy[e].safe_ticks;
            }
        return 0; }
    case WRSN_PEEK_ENV: {
        std::vector<WrsnEnvDyn> dy(B); std::vector<WrsnEnvConst> ec(B);
        HIPCHK(hipMemcpy(dy.data(), d.live.dyn, B * sizeof(WrsnEnvDyn), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ec.data(), d.ec, B * sizeof(WrsnEnvConst), hipMemcpyDeviceToHost));
        double* o = (double*)dst;
        for (size_t e = 0; e < B; ++e) {
            double* q = o + e * 16;
            q[0] = ec[e].frame[0]; q[1] = ec[e].frame[1]; q[2] = ec[e].frame[2]; q[3] = ec[e].frame[3];
            q[4] = ec[e].density; q[5] = ec[e].moving_time_max; q[6] = ec[e].charging_time_max; q[7] = ec[e].avg_nodes_agent;
            q[8] = dy[e].now; q[9] = dy[e].alive; q[10] = (double)dy[e].n_ticks; q[11] = (double)dy[e].n_exact;
            q[12] = (double)dy[e].n_events; q[13] = dy[e].last_minfit; q[14] = ec[e].n_edges; q[15] = ec[e].n_cover;
        }
        return 0; }
    case WRSN_PEEK_TARGETS_ACTIVE: {
        // Network.setLevels marks the targets of every node it reaches (Network.py:45-55); the level words keep what the
        // last setLevels found (a node that died since keeps its level until the next one, exactly like node.level)
        const size_t TP = d.TP, T = d.T;
        std::vector<int32_t> ls(B * NP), off(B * (TP + 1)), idx(B * (size_t)d.CCAP);
        std::vector<WrsnEnvConst> ec(B);
        HIPCHK(hipMemcpy(ls.data(), d.live.ls, ls.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(off.data(), d.tc_off, off.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(idx.data(), d.tc_idx, idx.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ec.data(), d.ec, B * sizeof(WrsnEnvConst), hipMemcpyDeviceToHost));
        int32_t* o = (int32_t*)dst;
        for (size_t e = 0; e < B; ++e)
            for (size_t t = 0; t < T; ++t) {
                int32_t act = 0;
                if ((int)t < ec[e].n_target)
                    for (int32_t p = off[e * (TP + 1) + t]; p < off[e * (TP + 1) + t + 1]; ++p)
                        if ((ls[e * NP + idx[e * (size_t)d.CCAP + p]] >> 1) >= 2) act = 1;     // level >= 1
                o[e * T + t] = act;
            }
        return 0; }
    case 10: {   // diagnostic builds (-DWRSN_PROFILE): int64 [B,25] per-phase cycle totals (+ whole kernel); zeros otherwise
        HIPCHK(hipMemcpy(dst, d.counters, B * 25 * sizeof(int64_t), hipMemcpyDeviceToHost));
        return 0; }
    case WRSN_PEEK_RNG_STATE: {
        if (!h->stoch) return fail(WRSN_ERR_STATE, "the generator is tracked by handles that run the stochastic kernels only (an environment with prob_gp != 1 loaded through wrsn_set_scenario_seeded)");
        std::vector<uint32_t> tmp(B * WRSN_MT_STRIDE);
        HIPCHK(hipMemcpy(tmp.data(), h->sd.mt_live, tmp.size() * 4, hipMemcpyDeviceToHost));
        uint32_t* o = (uint32_t*)dst;
        for (size_t e = 0; e < B; ++e) std::memcpy(o + e * 627, tmp.data() + e * WRSN_MT_STRIDE, 627 * 4);
        return 0; }
    case WRSN_PEEK_POOL: {
        std::vector<int32_t> cur(B), sw(B);
        HIPCHK(hipMemcpy(cur.data(), h->d_pool_cur, B * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(sw.data(), h->d_pool_swaps, B * 4, hipMemcpyDeviceToHost));
        int32_t* o = (int32_t*)dst;
        for (size_t e = 0; e < B; ++e) { o[2 * e] = cur[e]; o[2 * e + 1] = sw[e]; }
        return 0; }
    case WRSN_PEEK_ORDER: {
        if (h->bp2 <= 0) return fail(WRSN_ERR_STATE, "the launch order of this handle is not sorted (more environments than the sort workgroup takes)");
        uint32_t* o = (uint32_t*)dst;
        HIPCHK(hipMemcpy(o, d.order_key, B * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(o + B, d.order, B * 4, hipMemcpyDeviceToHost));
        return 0; }
    default: return fail(WRSN_ERR_ARG, "unknown peek selector");
    }
}

int wrsn_counters(wrsn_t* h, int64_t* dst) {
    if (!h || !dst) return fail(WRSN_ERR_ARG, "null argument");
    const size_t B = h->dev.B;
    WRSN_ON_DEVICE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<WrsnEnvDyn> dy(B);
    HIPCHK(hipMemcpy(dy.data(), h->dev.live.dyn, B * sizeof(WrsnEnvDyn), hipMemcpyDeviceToHost));
    // n_ticks / n_exact / n_events restart at every reset (they live in the snapshot); n_steps is cumulative
    for (int k = 0; k < 8; ++k) dst[k] = 0;
    for (size_t e = 0; e < B; ++e) {
        dst[0] += dy[e].n_ticks; dst[1] += dy[e].n_exact; dst[2] += dy[e].n_events; dst[3] += dy[e].n_steps;
        dst[4] += dy[e].tot_ticks; dst[5] += dy[e].tot_zero_steps;
    }
    return WRSN_OK;
}

int wrsn_env_record_bytes(wrsn_t* h, int64_t* bytes) {
    if (!h || !bytes) return fail(WRSN_ERR_ARG, "null argument");
    *bytes = h->rec_bytes;
    return WRSN_OK;
}

int wrsn_save_envs(wrsn_t* h, const int32_t* env, int32_t n, const wrsn_step_out* req, void* dst) {
    if (!h || !env || !req || !dst || n < 1) return fail(WRSN_ERR_ARG, "null argument or n < 1");
    if (!req->agent_id || !req->reward || !req->terminal || !req->now || !req->status)
        return fail(WRSN_ERR_ARG, "wrsn_save_envs needs the request rows: agent_id, reward, terminal, now and status");
    if ((uintptr_t)dst % 16) return fail(WRSN_ERR_ARG, "dst must be 16-byte aligned");
    int rc = check_envs(h, env, n, false, true, "env"); if (rc) return rc;
    WRSN_ON_DEVICE(h);
    if ((rc = ensure_idx(h, (size_t)n))) return rc;
    HIPCHK(hipMemcpyAsync(h->d_idx, env, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(wrsn_rec_header_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->dev, (const double*)h->sd.pgp, rec_template(h),
                       (const int32_t*)h->d_idx, (int)n, (uint8_t*)dst, (long long)h->rec_bytes, step_out_dev(req, false));
    HIPCHK(hipGetLastError());
    return launch_rec_copy(h, WRSN_REC_PACK, h->d_idx, nullptr, (uint8_t*)dst, n);
}

int wrsn_load_envs(wrsn_t* h, const int32_t* env, int32_t n, const void* src, const wrsn_step_out* out) {
    if (!h || !env || !src || !out || n < 1) return fail(WRSN_ERR_ARG, "null argument or n < 1");
    if ((uintptr_t)src % 16) return fail(WRSN_ERR_ARG, "src must be 16-byte aligned");
    int rc = check_envs(h, env, n, true, false, "env"); if (rc) return rc;
    WRSN_ON_DEVICE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    // record 0 decides the stride of the records (validated against this handle's geometry first), then every header is gathered and
    // validated before anything changes
    WrsnRecHeader r0;
    HIPCHK(hipMemcpy(&r0, src, sizeof(r0), hipMemcpyDeviceToHost));
    if ((rc = rec_check(h, r0, 0))) return rc;
    hipLaunchKernelGGL(wrsn_rec_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, (const uint8_t*)src, (long long)r0.rec_bytes, (int)n, h->d_hdr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<WrsnRecHeader> hd(n);
    HIPCHK(hipMemcpy(hd.data(), h->d_hdr, (size_t)n * sizeof(WrsnRecHeader), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        if ((rc = rec_check(h, hd[i], i))) return rc;
        if (hd[i].has_gen != r0.has_gen) return fail(WRSN_ERR_ARG, "record " + std::to_string(i) + ": has_gen differs from record 0's");
    }
    // generator blocks: the stochastic kernels read them for every environment of a stochastic handle, so they go only where the handle
    // keeps generators (or holds no scenario yet, and then gets them); a record without one goes only where the handle keeps none
    bool any_filled = false;
    for (uint8_t f : h->filled) any_filled = any_filled || f;
    if (r0.has_gen && !h->sd.mt_live && any_filled)
        return fail(WRSN_ERR_ARG, "has_gen: the records hold a generator block, this handle keeps no generators and already holds a scenario");
    if (!r0.has_gen && h->sd.mt_live)
        return fail(WRSN_ERR_ARG, "has_gen: the records hold no generator block, this handle keeps generators");
    // ---- every record fits: replace the environments
    if (r0.has_gen && !h->sd.mt_live && (rc = alloc_stoch(h))) return rc;
    bool want_stoch = false; int conn_bound = 0;               // as wrsn_set_scenario
    for (int i = 0; i < n; ++i) {
        if (hd[i].prob_gp != 1.0) want_stoch = true;
        if (hd[i].conn_bound > conn_bound) conn_bound = hd[i].conn_bound;
    }
    if ((rc = fit_launch(h, conn_bound, want_stoch))) return rc;
    HIPCHK(hipMemcpyAsync(h->d_idx, env, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if ((rc = launch_rec_copy(h, WRSN_REC_UNPACK, nullptr, h->d_idx, (uint8_t*)src, n))) return rc;
    if ((rc = launch_rec_rows(h, h->d_hdr, nullptr, h->d_idx, n, out))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; ++i) h->filled[env[i]] = 1;
    h->scenario_set = 1;
    return WRSN_OK;
}

int wrsn_clone_envs(wrsn_t* h, const int32_t* src, const int32_t* dst, int32_t n, const wrsn_step_out* out) {
    if (!h || !src || !dst || !out || n < 1) return fail(WRSN_ERR_ARG, "null argument or n < 1");
    if ((out->obs || h->ent.node) && !out->agent_id) return fail(WRSN_ERR_ARG, "rendering the cloned rows needs out->agent_id");
    int rc = check_envs(h, src, n, false, true, "src"); if (rc) return rc;
    if ((rc = check_envs(h, dst, n, true, false, "dst"))) return rc;
    {
        std::vector<uint8_t> is_src(h->dev.B, 0);
        for (int i = 0; i < n; ++i) is_src[src[i]] = 1;
        for (int i = 0; i < n; ++i)
            if (is_src[dst[i]]) return fail(WRSN_ERR_ARG, "dst[" + std::to_string(i) + "] = " + std::to_string(dst[i]) + " is also a source");
    }
    WRSN_ON_DEVICE(h);
    if ((rc = ensure_idx(h, 2 * (size_t)n))) return rc;
    HIPCHK(hipMemcpyAsync(h->d_idx, src, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_idx + n, dst, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if ((rc = launch_rec_copy(h, WRSN_REC_CLONE, h->d_idx, h->d_idx + n, nullptr, n))) return rc;
    if ((rc = launch_rec_rows(h, nullptr, h->d_idx, h->d_idx + n, n, out))) return rc;
    for (int i = 0; i < n; ++i) h->filled[dst[i]] = 1;
    return WRSN_OK;
}

// Across two handles: the distinct sources are packed into records in an area the destination owns (wrsn_rec_header_kernel and the pack
// direction of the copy loop, on the SOURCE's segment table), then unpacked into the destinations by wrsn_pool_copy_kernel on the
// destination's table, whose record index is the fan-out; wrsn_rec_rows_kernel takes the request rows from the records' headers.  No new
// copy kernel, no host read; every check comes before the first launch.
int wrsn_clone_envs_from(wrsn_t* dst_h, wrsn_t* src_h, const int32_t* src, const int32_t* dst, int32_t n, const wrsn_step_out* src_req,
                         const wrsn_step_out* dst_out) {
    if (!dst_h || !src_h || !src || !dst || !src_req || !dst_out || n < 1) return fail(WRSN_ERR_ARG, "wrsn_clone_envs_from: null argument or n < 1");
    if (dst_h == src_h) return fail(WRSN_ERR_ARG, "wrsn_clone_envs_from: source and destination are the same handle (wrsn_clone_envs clones inside one)");
    if (!src_req->agent_id || !src_req->reward || !src_req->terminal || !src_req->now || !src_req->status)
        return fail(WRSN_ERR_ARG, "wrsn_clone_envs_from needs the source's request rows: agent_id, reward, terminal, now and status");
    if ((dst_out->obs || dst_h->ent.node) && !dst_out->agent_id) return fail(WRSN_ERR_ARG, "rendering the cloned rows needs dst_out->agent_id");
    if (src_h->cfg.device != dst_h->cfg.device) return fail(WRSN_ERR_ARG, "wrsn_clone_envs_from: the handles are on different devices");
    if (src_h->stream != dst_h->stream) return fail(WRSN_ERR_ARG, "wrsn_clone_envs_from: the handles run on different streams (wrsn_set_stream)");
    {
        const WrsnDev &s = src_h->dev, &d = dst_h->dev;
        auto bad = [&](const char* field, long long got, long long want) {
            return fail(WRSN_ERR_ARG, std::string("wrsn_clone_envs_from: ") + field + " of the source is " + std::to_string(got) + ", the destination needs " + std::to_string(want));
        };
        if (s.NP != d.NP) return bad("NP", s.NP, d.NP);
        if (s.TP != d.TP) return bad("TP", s.TP, d.TP);
        if (s.ECAP != d.ECAP) return bad("ECAP", s.ECAP, d.ECAP);
        if (s.CCAP != d.CCAP) return bad("CCAP", s.CCAP, d.CCAP);
        if (s.M != d.M) return bad("M", s.M, d.M);
        if (s.N > d.N) return bad("n_node", s.N, d.N);
        if (s.T > d.T) return bad("n_target", s.T, d.T);
    }
    if ((src_h->sd.mt_live != nullptr) != (dst_h->sd.mt_live != nullptr))
        return fail(WRSN_ERR_ARG, "wrsn_clone_envs_from: one handle keeps generators and the other does not");
    if (src_h->rec_bytes != dst_h->rec_bytes || src_h->nseg != dst_h->nseg) return fail(WRSN_ERR_ARG, "wrsn_clone_envs_from: the record layouts of the handles differ");
    int rc = check_envs(src_h, src, n, false, true, "src"); if (rc) return rc;
    if ((rc = check_envs(dst_h, dst, n, true, false, "dst"))) return rc;
    // ---- everything fits.  Host index arrays, staged in the destination's area: dst [n], record of pair i [n], distinct sources [u], n
    std::vector<int32_t> rec_of((size_t)src_h->dev.B, -1), idx((size_t)2 * n);
    std::vector<int32_t> uniq;
    for (int i = 0; i < n; ++i) {
        if (rec_of[src[i]] < 0) { rec_of[src[i]] = (int32_t)uniq.size(); uniq.push_back(src[i]); }
        idx[i] = dst[i]; idx[(size_t)n + i] = rec_of[src[i]];
    }
    const int u = (int)uniq.size();
    idx.insert(idx.end(), uniq.begin(), uniq.end());
    idx.push_back(n);
    WRSN_ON_DEVICE(dst_h);
    wrsn_handle* h = dst_h;
    if (src_h->cc_bound > h->cc_bound || (src_h->stoch && !h->stoch)) {   // a new launch configuration, as a load's: once at most
        HIPCHK(hipStreamSynchronize(h->stream));
        if ((rc = fit_launch(h, src_h->cc_bound, src_h->stoch != 0))) return rc;
    }
    const size_t need = (size_t)u * (size_t)h->rec_bytes;
    if (need > h->xfer_cap) {
        void* q = nullptr;
        HIPCHK(hipMalloc(&q, need));
        h->allocs.push_back(q);                               // the old area stays allocated: it is in h->allocs already
        h->xfer = (uint8_t*)q; h->xfer_cap = need;
    }
    if ((rc = ensure_idx(h, idx.size()))) return rc;
    HIPCHK(hipMemcpyAsync(h->d_idx, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    const int32_t *d_dst = h->d_idx, *d_rec = h->d_idx + n, *d_uniq = h->d_idx + 2 * (size_t)n, *d_n = h->d_idx + 2 * (size_t)n + u;
    hipLaunchKernelGGL(wrsn_rec_header_kernel, dim3((u + 255) / 256), dim3(256), 0, h->stream, src_h->dev, (const double*)src_h->sd.pgp, rec_template(src_h),
                       d_uniq, u, h->xfer, (long long)h->rec_bytes, step_out_dev(src_req, false));
    HIPCHK(hipGetLastError());
    if ((rc = launch_rec_copy(src_h, WRSN_REC_PACK, d_uniq, nullptr, h->xfer, u))) return rc;
    {
        const int chunks = (int)(h->rec_bytes / 16), per = chunks - WRSN_REC_HDR / 16;
        const long long want = ((long long)n * per + 255) / 256;
        const int blocks = (int)(want < (long long)h->cus * 8 ? want : (long long)h->cus * 8);
        hipLaunchKernelGGL(wrsn_pool_copy_kernel, dim3(blocks), dim3(256), (size_t)h->nseg * sizeof(WrsnSeg), h->stream, (const WrsnSeg*)h->d_segs, h->nseg,
                           d_dst, d_rec, d_n, (const uint8_t*)h->xfer, (long long)h->rec_bytes, chunks);
        HIPCHK(hipGetLastError());
    }
    const bool renders = dst_out->obs || h->ent.node;
    if (renders) HIPCHK(hipMemsetAsync(h->d_rend, 0xFF, (size_t)h->dev.B * sizeof(int32_t), h->stream));
    hipLaunchKernelGGL(wrsn_rec_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->dev, (const uint8_t*)h->xfer, (long long)h->rec_bytes, d_rec,
                       (const int32_t*)nullptr, d_dst, (int)n, (const int32_t*)nullptr, step_out_dev(dst_out), renders ? h->d_rend : (int32_t*)nullptr, -1, 0,
                       h->d_pool_cur);
    HIPCHK(hipGetLastError());
    if (renders && (rc = launch_render_all(h, h->d_rend, dst_out->obs))) return rc;
    for (int i = 0; i < n; ++i) h->filled[dst[i]] = 1;
    h->scenario_set = 1;
    return WRSN_OK;
}

// ------------------------------------------------------------------ one-step lookahead over the heuristic's K best picks (wrsn_rollout.h)
namespace {
const char* lookahead_bad(const wrsn_lookahead_state* st) {
    if (!st) return "wrsn_lookahead_state is NULL";
    if (st->K < 1 || st->K > WRSN_LOOKAHEAD_MAX_K) return "wrsn_lookahead_state: K must lie in [1, WRSN_LOOKAHEAD_MAX_K]";
    if (st->B < 1) return "wrsn_lookahead_state: B must be at least 1";
    if (!st->t0 || !st->t_end || !st->last_now || !st->ret || !st->survived || !st->done || !st->died) return "wrsn_lookahead_state: every array is required";
    const void* f8[] = {st->t0, st->t_end, st->last_now, st->ret, st->survived};
    for (const void* p : f8) if ((uintptr_t)p % 8) return "wrsn_lookahead_state: a float64 array is not 8-byte aligned";
    return nullptr;
}
WrsnLookahead lookahead_dev(const wrsn_lookahead_state* st) {
    WrsnLookahead L;
    L.K = st->K; L.B = st->B; L.t0 = st->t0; L.t_end = st->t_end; L.last_now = st->last_now; L.ret = st->ret; L.survived = st->survived;
    L.done = st->done; L.died = st->died;
    return L;
}
}  // namespace

int wrsn_lookahead_candidates(wrsn_t* h, const int32_t* agent_id, const wrsn_entity_out* ent, const double* now, const wrsn_lookahead_state* st,
                              double horizon, float charge_scale, double min_charge, float x_clip, int32_t* node, int32_t* sim_agent_id,
                              double* sim_action, float* stored) {
    if (!h || !agent_id || !now || !node || !sim_agent_id || !sim_action || !stored)
        return fail(WRSN_ERR_ARG, "wrsn_lookahead_candidates needs agent_id, now, node, sim_agent_id, sim_action and stored");
    if (const char* m = lookahead_bad(st)) return fail(WRSN_ERR_ARG, m);
    if (st->B != h->dev.B) return fail(WRSN_ERR_ARG, "wrsn_lookahead_candidates: wrsn_lookahead_state.B is not the handle's batch");
    if ((uintptr_t)agent_id % 4 || (uintptr_t)node % 4 || (uintptr_t)sim_agent_id % 4 || (uintptr_t)stored % 4 || (uintptr_t)now % 8 || (uintptr_t)sim_action % 8)
        return fail(WRSN_ERR_ARG, "wrsn_lookahead_candidates: an array is not aligned to its element size");
    if (!std::isfinite(horizon) || horizon <= 0.0) return fail(WRSN_ERR_ARG, "wrsn_lookahead_candidates: horizon must be finite and > 0");
    if (!std::isfinite(min_charge) || min_charge < 0.0 || min_charge >= 1.0)
        return fail(WRSN_ERR_ARG, "wrsn_lookahead_candidates: min_charge must be finite and in [0, 1)");
    if (!std::isfinite(x_clip) || x_clip <= 0.f) return fail(WRSN_ERR_ARG, "wrsn_lookahead_candidates: x_clip must be finite and > 0");
    WrsnEntityOut e{};
    { const int rc = entity_in(h, ent, &e); if (rc) return rc; }
    WRSN_ON_DEVICE(h);
    const int B = h->dev.B;
    hipLaunchKernelGGL(wrsn_lookahead_candidates_kernel, entity_row_grid(B), dim3(64 * WRSN_ENT_ROWS), 0, h->stream, B, h->dev.M, h->dev.N, (int)st->K, agent_id, e,
                       now, lookahead_dev(st), horizon, charge_scale, min_charge, x_clip, node, sim_agent_id, sim_action, stored);
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int wrsn_lookahead_collect(wrsn_t* sim_h, const wrsn_lookahead_state* st, const wrsn_step_out* out, int32_t* next_agent_id, int32_t close_all) {
    if (!sim_h || !out || !next_agent_id) return fail(WRSN_ERR_ARG, "wrsn_lookahead_collect needs the handle, out and next_agent_id");
    if (const char* m = lookahead_bad(st)) return fail(WRSN_ERR_ARG, m);
    if ((long long)st->K * st->B != (long long)sim_h->dev.B)
        return fail(WRSN_ERR_ARG, "wrsn_lookahead_collect: the handle's batch is not K * B of wrsn_lookahead_state");
    if (!out->agent_id || !out->reward || !out->now || !out->status)
        return fail(WRSN_ERR_ARG, "wrsn_lookahead_collect needs agent_id, reward, now and status of wrsn_step_out");
    if (next_agent_id == out->agent_id) return fail(WRSN_ERR_ARG, "wrsn_lookahead_collect: next_agent_id must not be out->agent_id");
    WRSN_ON_DEVICE(sim_h);
    const int R = sim_h->dev.B;
    hipLaunchKernelGGL(wrsn_lookahead_collect_kernel, dim3((R + 255) / 256), dim3(256), 0, sim_h->stream, R, lookahead_dev(st), (const int32_t*)out->agent_id,
                       (const double*)out->reward, (const double*)out->now, (const int32_t*)out->status, sim_h->dev.row_state, next_agent_id,
                       (int)(close_all != 0));
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int wrsn_lookahead_pick(wrsn_t* h, const int32_t* agent_id, const wrsn_lookahead_state* st, const int32_t* sim_agent_id, const double* sim_action,
                        const float* cand_stored, int32_t* choice, double* action_f64, float* action, float* stored) {
    if (!h || !agent_id || !sim_agent_id || !sim_action || !choice) return fail(WRSN_ERR_ARG, "wrsn_lookahead_pick needs agent_id, sim_agent_id, sim_action and choice");
    if (stored && !cand_stored) return fail(WRSN_ERR_ARG, "wrsn_lookahead_pick: stored needs the candidates' stored pairs");
    if (const char* m = lookahead_bad(st)) return fail(WRSN_ERR_ARG, m);
    if (st->B != h->dev.B) return fail(WRSN_ERR_ARG, "wrsn_lookahead_pick: wrsn_lookahead_state.B is not the handle's batch");
    WRSN_ON_DEVICE(h);
    const int B = h->dev.B;
    hipLaunchKernelGGL(wrsn_lookahead_pick_kernel, dim3((B + 255) / 256), dim3(256), 0, h->stream, B, h->dev.M, agent_id, lookahead_dev(st), sim_agent_id, sim_action,
                       cand_stored, choice, action_f64, action, stored);
    HIPCHK(hipGetLastError());
    return WRSN_OK;
}

int wrsn_pool_set(wrsn_t* h, const void* records, int32_t n_records, uint64_t seed) {
    if (!h) return fail(WRSN_ERR_ARG, "null handle");
    if (!records && n_records == 0) {                          // clear
        h->pool = nullptr; h->pool_n = 0; h->pool_seed = 0; h->pool_rec_bytes = 0;
        return WRSN_OK;
    }
    if (!records || n_records < 1) return fail(WRSN_ERR_ARG, "null records or n_records < 1");
    if ((uintptr_t)records % 16) return fail(WRSN_ERR_ARG, "records must be 16-byte aligned");
    WRSN_ON_DEVICE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    // as wrsn_load_envs: record 0 decides the stride, then every header is gathered (B at a time: the staging holds B) and validated
    // before anything changes
    WrsnRecHeader r0;
    HIPCHK(hipMemcpy(&r0, records, sizeof(r0), hipMemcpyDeviceToHost));
    int rc = rec_check(h, r0, 0); if (rc) return rc;
    const int B = h->dev.B;
    std::vector<WrsnRecHeader> hd((size_t)n_records);
    for (int i0 = 0; i0 < n_records; i0 += B) {
        const int m = n_records - i0 < B ? n_records - i0 : B;
        hipLaunchKernelGGL(wrsn_rec_gather_kernel, dim3((m + 255) / 256), dim3(256), 0, h->stream, (const uint8_t*)records + (size_t)i0 * (size_t)r0.rec_bytes,
                           (long long)r0.rec_bytes, m, h->d_hdr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(hd.data() + i0, h->d_hdr, (size_t)m * sizeof(WrsnRecHeader), hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < n_records; ++i) {
        if ((rc = rec_check(h, hd[i], i))) return rc;
        if (hd[i].has_gen != r0.has_gen) return fail(WRSN_ERR_ARG, "record " + std::to_string(i) + ": has_gen differs from record 0's");
    }
    bool any_filled = false;
    for (uint8_t f : h->filled) any_filled = any_filled || f;
    if (r0.has_gen && !h->sd.mt_live && any_filled)
        return fail(WRSN_ERR_ARG, "has_gen: the records hold a generator block, this handle keeps no generators and already holds a scenario");
    if (!r0.has_gen && h->sd.mt_live)
        return fail(WRSN_ERR_ARG, "has_gen: the records hold no generator block, this handle keeps generators");
    // ---- every record fits: one launch configuration for whatever a later swap brings in
    if (r0.has_gen && !h->sd.mt_live && (rc = alloc_stoch(h))) return rc;
    bool want_stoch = false; int conn_bound = 0;
    for (int i = 0; i < n_records; ++i) {
        if (hd[i].prob_gp != 1.0) want_stoch = true;
        if (hd[i].conn_bound > conn_bound) conn_bound = hd[i].conn_bound;
    }
    if ((rc = fit_launch(h, conn_bound, want_stoch))) return rc;
    HIPCHK(hipMemset(h->d_pool_swaps, 0, (size_t)B * sizeof(int32_t)));
    h->pool = (const uint8_t*)records; h->pool_n = n_records; h->pool_seed = seed; h->pool_rec_bytes = h->rec_bytes;
    return WRSN_OK;
}

int wrsn_pool_reset(wrsn_t* h, const uint8_t* env_mask, const int32_t* pool_index, int32_t* agent_id, const wrsn_step_out* out) {
    if (!h || !out) return fail(WRSN_ERR_ARG, "null argument");
    if (!h->pool) return fail(WRSN_ERR_STATE, "no scenario pool is set (wrsn_pool_set)");
    if (h->pool_rec_bytes != h->rec_bytes) return fail(WRSN_ERR_STATE, "the record layout of the handle changed since wrsn_pool_set: set the pool again");
    for (size_t e = 0; e < h->filled.size(); ++e)
        if (!h->filled[e]) return fail(WRSN_ERR_STATE, "environment " + std::to_string(e) + " holds no scenario yet: wrsn_pool_reset needs every environment filled");
    if (agent_id && agent_id == out->agent_id) return fail(WRSN_ERR_ARG, "agent_id must not be out->agent_id (selected rows get -2 there and the record's charger here)");
    if (out->obs && !out->agent_id) return fail(WRSN_ERR_ARG, "rendering the replaced rows needs out->agent_id");
    WRSN_ON_DEVICE(h);
    const int B = h->dev.B;
    const bool renders = out->obs || h->ent.node;              // (the entity rows take the charger from the record's header)
    int32_t* rend = renders ? h->d_rend : (int32_t*)nullptr;
    hipLaunchKernelGGL(wrsn_pool_select_kernel, dim3(1), dim3(64), 0, h->stream, h->dev, env_mask, pool_index, h->pool_n, h->pool_seed, agent_id, h->d_pool_cur,
                       h->d_pool_swaps, h->d_pairs, h->d_pairs + B, h->d_pair_n, out->status, rend);
    {   // fixed grid: at most eight blocks per CU, no more than the whole batch needs
        const int chunks = (int)(h->rec_bytes / 16), per = chunks - WRSN_REC_HDR / 16;
        const long long need = ((long long)B * per + 255) / 256;
        const int blocks = (int)(need < (long long)h->cus * 8 ? need : (long long)h->cus * 8);
        hipLaunchKernelGGL(wrsn_pool_copy_kernel, dim3(blocks), dim3(256), (size_t)h->nseg * sizeof(WrsnSeg), h->stream, (const WrsnSeg*)h->d_segs, h->nseg,
                           (const int32_t*)h->d_pairs, (const int32_t*)(h->d_pairs + B), (const int32_t*)h->d_pair_n, h->pool, (long long)h->rec_bytes, chunks);
    }
    hipLaunchKernelGGL(wrsn_rec_rows_kernel, dim3((B + 255) / 256), dim3(256), 0, h->stream, h->dev, h->pool, (long long)h->rec_bytes, (const int32_t*)(h->d_pairs + B),
                       (const int32_t*)nullptr, (const int32_t*)h->d_pairs, B, (const int32_t*)h->d_pair_n, step_out_dev(out), rend, env_mask ? 0 : 3, 2, (int32_t*)nullptr);
    HIPCHK(hipGetLastError());
    if (renders) return launch_render_all(h, h->d_rend, out->obs);
    return WRSN_OK;
}

int wrsn_synth_network(uint64_t seed, int32_t n_node, int32_t n_target, double side, double com_range,
                       double sen_range, double* node_xy, double* target_xy, double* bs_xy) {
    if (n_node < 2 || n_target < 1 || !node_xy || !target_xy || !bs_xy || !(com_range > 0) || !(sen_range > 0))
        return fail(WRSN_ERR_ARG, "bad generator argument");
    if (side <= 0) side = 1000.0 * std::fmax(1.0, std::sqrt(n_node / 200.0));
    Rng rng(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull);
    const double com = com_range, sen = sen_range;
    const double bx = side / 2, by = side / 2;
    const double hop_lo = 0.62 * com, hop_hi = 0.995 * com, min_sep = 0.56 * com;
    std::vector<int> tips;
    // Nodes next to the base station: 2..4 up to 512 nodes (the shipped scenarios have 2..3; networks of that size are unchanged), one more per
    // 125 nodes above 256 (at most six) for the larger ones -- every packet of the network passes one of them, and with three of them a 1 000-node /
    // 1 000-target network loses its first relay 40 s after the warm-up, which makes a benchmark of resets, not of the dynamics
    int n = 0, n_direct = 2 + rng.below(3);
    if (n_node > 512) { n_direct += (n_node - 256) / 125; if (n_direct > 6) n_direct = 6; }   // (six fit the ring around the base station at the minimum separation)
    long tries = 0;
    while (n < n_node) {
        if (++tries > 4000000L) return fail(WRSN_ERR_ARG, "synthetic generator could not place the nodes (field too small?)");
        double px, py; int par = -1;
        if (n < n_direct) {
            double ang = rng.uni(0, 6.283185307179586), r = rng.uni(0.35 * com, 0.95 * com);
            px = bx + r * std::cos(ang); py = by + r * std::sin(ang);
        } else {
            if (!tips.empty() && rng.uni() < 0.93) par = tips[rng.below((int)tips.size())];
            else par = rng.below(n);
            double ox = node_xy[2 * par] - bx, oy = node_xy[2 * par + 1] - by;
            double ang = std::atan2(oy, ox) + 0.75 * rng.normal(), r = rng.uni(hop_lo, hop_hi);
            px = node_xy[2 * par] + r * std::cos(ang); py = node_xy[2 * par + 1] + r * std::sin(ang);
        }
        if (px < 0 || px > side || py < 0 || py > side) continue;
        bool ok = true;
        for (int k = 0; k < n && ok; ++k) { double dx = node_xy[2 * k] - px, dy = node_xy[2 * k + 1] - py; if (dx * dx + dy * dy < min_sep * min_sep) ok = false; }
        if (!ok) continue;
        node_xy[2 * n] = px; node_xy[2 * n + 1] = py;
        for (size_t k = 0; k < tips.size(); ++k) if (tips[k] == par) { tips.erase(tips.begin() + k); break; }
        tips.push_back(n);
        if (tips.size() > 24) tips.erase(tips.begin());
        ++n;
    }
    // targets: inside 0.93 * sensing range of an owner node, biased towards the outer nodes
    std::vector<double> cum(n_node);
    double dmax = 0; for (int i = 0; i < n_node; ++i) dmax = std::fmax(dmax, std::hypot(node_xy[2 * i] - bx, node_xy[2 * i + 1] - by));
    double acc = 0; for (int i = 0; i < n_node; ++i) { acc += 0.25 + std::hypot(node_xy[2 * i] - bx, node_xy[2 * i + 1] - by) / dmax; cum[i] = acc; }
    for (int t = 0; t < n_target; ++t) {
        double u = rng.uni() * acc; int lo = 0, hi = n_node - 1;
        while (lo < hi) { int mid = (lo + hi) / 2; if (cum[mid] < u) lo = mid + 1; else hi = mid; }
        double ang = rng.uni(0, 6.283185307179586), r = 0.93 * sen * std::sqrt(rng.uni());
        target_xy[2 * t] = node_xy[2 * lo] + r * std::cos(ang); target_xy[2 * t + 1] = node_xy[2 * lo + 1] + r * std::sin(ang);
    }
    bs_xy[0] = bx; bs_xy[1] = by;
    return WRSN_OK;
}

}  // extern "C"
