// sqrl_kernels.hip -- SQRL constraint-sampling acting (SAC._sqrl_action, recovery_rl/sac.py:139-161) as ONE MFMA kernel
// for gfx950: per env, k candidate actions from the task policy's head, the twin Q_risk on every candidate, and the pick.
//
// The module path expands every observation to k rows and runs both networks on n k rows.  The policy sees the same state
// k times, so its head is taken from the n-row acting forward that exists already; what is left is the twin Q_risk
// (4 -> 256 relu -> 256 relu -> 1, two heads) on n k rows.  One workgroup owns one env: its candidates go through the
// network in passes of up to 64 rows with the activations in LDS (the planner's tile, plan_kernels.hip), W2 arrives from
// L2 in MFMA fragment order (rrl_w2_pack: the copy the optimiser launch keeps current), and only action[n, 2] leaves the
// chip.  Arithmetic is v_mfma_f32_16x16x4_f32 (exact f32 fma chains).
//
// The tile and the twin-head phase (q_phase) come from mfma_tile.hpp, shared with qsample_kernels.hip.
#include "mfma_tile.hpp"
#include "rrl_device.hpp"
#include "rrl_host.hpp"
#include "pack.hpp"

using namespace rrl_host;
using namespace rrl_tile;

namespace {

using rrl::psum;

constexpr uint32_t kStreamSqrl = RRL_STREAM_SQRL, kStreamSqrlPick = RRL_STREAM_SQRL_PICK;
constexpr int kMaxK = 128;                // candidates per env
constexpr float kLogSigMax = 2.f, kLogSigMin = -20.f, kEps = 1e-6f;   // model.py:14-16
constexpr float kHalfLog2Pi = 0.918938533204672742f;

// LDS carve-up (floats), behind the tile's act / xs / qpart
constexpr int kOffCand = kOffOwn;                            // [128][2] candidate actions
constexpr int kOffLogp = kOffCand + kMaxK * 2;               // [128]
constexpr int kOffQ = kOffLogp + kMaxK;                      // [128] max(sigmoid z0, sigmoid z1)
constexpr int kOffW = kOffQ + kMaxK;                         // [128] doubles: the pick's weights
constexpr int kOffPick = kOffW + 2 * kMaxK;                  // 4 ints: {n_safe, argmin, -, -}, then 2 x u64 safe masks
constexpr int kLdsFloats = kOffPick + 8;
constexpr int kLdsBytes = kLdsFloats * 4;                    // 75.8 KB: two workgroups per CU
static_assert(kOffW % 2 == 0 && kOffPick % 2 == 0, "doubles and 64-bit masks need 8-byte alignment");

struct SqrlArgs {
    int k, n_part;
    int n;                                    // the envs of THIS learner (a packed grid holds several learners' workgroups)
    long long part_stride;
    const float *obs, *head, *scale, *bias;
    const float *W1, *b1, *W2p, *b2, *W3, *b3;
    float eps_safe;
    uint64_t seed, counter;
    uint64_t* counter_dev;
    uint64_t counter_inc;
    const float* eps_in;
    const double* u_in;
    float* action;
    float *q, *logp, *cand, *z;
    int32_t *pick, *cstar, *n_safe;
};

// One pass: rows [base, base + 16 MR) of the env's candidates through the twin heads; q (and z) of the live ones.
template <int MR>
__device__ __forceinline__ void score_pass(float* lds, const SqrlArgs& a, long long env, int base, float ox, float oy,
                                           int tid, int wave, int lane) {
    const int k = a.k;
    if (tid < kRows) {
        const int c = base + tid;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};           // rows past k: finite inputs, results never read
        if (c < k) x = f32x4{ox, oy, lds[kOffCand + 2 * c], lds[kOffCand + 2 * c + 1]};
        *reinterpret_cast<f32x4*>(lds + kOffXs + tid * 4) = x;
    }
    __syncthreads();
    q_phase<MR>(lds, a, wave, lane);
    if (tid < kRows && base + tid < k) {
        const int c = base + tid;
        const TwinQ t = twin_q(lds, a, tid);
        lds[kOffQ + c] = t.q;
        if (a.q) a.q[env * k + c] = t.q;
        if (a.z) {
            a.z[env * k + c] = t.z[0];
            a.z[((long long)a.n + env) * k + c] = t.z[1];
        }
    }
    // xs and qpart are rewritten only behind the next pass's barriers
}

// One env of one learner: candidates, scores, pick.  Stated once; the stand-alone and the packed kernel differ only in where
// `a` and `env` come from (and in how many workgroups share the learner's tick).
// NT = row tiles of 16 candidates (ceil(k / 16), 1..8): pass 0 takes min(NT, 4) of them, pass 1 the rest
template <int NT>
__device__ __forceinline__ void sqrl_env(const SqrlArgs& a, const long long env, float* lds) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = a.k;
    const uint64_t ctr = rrl::effective_counter(a.counter, a.counter_dev);

    // ---- candidates: a[e, c], logp[e, c] (gauss_head_fwd_row of update_kernels.hip, same expression order) ----
    if (tid < k) {
        const int c = tid;
        float e2[2];
        if (a.eps_in) {
            e2[0] = a.eps_in[(env * k + c) * 2];
            e2[1] = a.eps_in[(env * k + c) * 2 + 1];
        } else {
            double d0, d1;
            rrl::normal_at(a.seed, uint32_t(env * k + c), kStreamSqrl, ctr, d0, d1);
            e2[0] = float(d0);
            e2[1] = float(d1);
        }
        float lp = 0.f, act2[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float mean = psum(a.head, 4 * env + j, a.n_part, a.part_stride);
            const float ls = fminf(fmaxf(psum(a.head, 4 * env + 2 + j, a.n_part, a.part_stride), kLogSigMin), kLogSigMax);
            const float e = e2[j];
            const float y = tanhf(mean + expf(ls) * e);
            act2[j] = y * a.scale[j] + a.bias[j];
            lp += -0.5f * e * e - ls - kHalfLog2Pi - logf(a.scale[j] * (1.f - y * y) + kEps);
        }
        lds[kOffCand + 2 * c] = act2[0];
        lds[kOffCand + 2 * c + 1] = act2[1];
        lds[kOffLogp + c] = lp;
        if (a.cand) {
            a.cand[(env * k + c) * 2] = act2[0];
            a.cand[(env * k + c) * 2 + 1] = act2[1];
        }
        if (a.logp) a.logp[env * k + c] = lp;
    }
    const float ox = a.obs[2 * env], oy = a.obs[2 * env + 1];
    __syncthreads();

    // ---- scores ----
    constexpr int MR0 = NT < 4 ? NT : 4, MR1 = NT - MR0;
    score_pass<MR0>(lds, a, env, 0, ox, oy, tid, wave, lane);
    if constexpr (MR1 > 0) score_pass<MR1>(lds, a, env, kRows, ox, oy, tid, wave, lane);

    // ---- pick (sac.py:153-158; the position in the SAFE list is applied to the FULL list, as the reference does) ----
    double* wts = reinterpret_cast<double*>(lds + kOffW);
    int* pk = reinterpret_cast<int*>(lds + kOffPick);
    unsigned long long* masks = reinterpret_cast<unsigned long long*>(lds + kOffPick + 4);
    __syncthreads();                              // q of every candidate is in LDS
    if (wave == 0) {
        float qv[2], lpv[2];
        bool safe[2];
        unsigned long long m[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int c = lane + 64 * hf;
            const bool live = c < k;
            qv[hf] = live ? lds[kOffQ + c] : 0.f;
            lpv[hf] = live ? lds[kOffLogp + c] : 0.f;
            safe[hf] = live && qv[hf] <= a.eps_safe;
            m[hf] = __ballot(safe[hf]);
        }
        // argmin of q, lowest index on ties; NaN counts as the smallest (torch.argmin)
        float best = __builtin_inff();
        int bidx = kMaxK;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int c = lane + 64 * hf;
            const float key = qv[hf] != qv[hf] ? -__builtin_inff() : qv[hf];
            if (c < k && key < best) {           // ascending c: strict < keeps the lower index
                best = key;
                bidx = c;
            }
        }
        // the largest safe logp
        float L = -__builtin_inff();
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
            if (safe[hf]) L = fmaxf(L, lpv[hf]);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float ob = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bidx, off, 64);
            if (ob < best || (ob == best && oi < bidx)) {
                best = ob;
                bidx = oi;
            }
            L = fmaxf(L, __shfl_xor(L, off, 64));
        }
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int c = lane + 64 * hf;
            if (c < k) wts[c] = safe[hf] ? exp(double(lpv[hf]) - double(L)) : 0.0;
        }
        if (lane == 0) {
            pk[0] = __popcll(m[0]) + __popcll(m[1]);
            pk[1] = bidx;
            masks[0] = m[0];
            masks[1] = m[1];
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int n_safe = pk[0];
        int pick = pk[1], cs = -1;
        if (n_safe > 0) {
            const unsigned long long m0 = masks[0], m1 = masks[1];
            const double u = a.u_in ? a.u_in[env] : rrl::unit_open(rrl::philox_at(a.seed, uint32_t(env), kStreamSqrlPick, ctr).lo);
            double T = 0.0;
            for (int c = 0; c < k; ++c) T += wts[c];
            const double thr = u * T;
            double run = 0.0;
            int last = -1;
            for (int c = 0; c < k; ++c) {
                const bool s = ((c < 64 ? m0 >> c : m1 >> (c - 64)) & 1ULL) != 0;
                if (!s) continue;
                last = c;
                run += wts[c];
                if (cs < 0 && run > thr) cs = c;
            }
            if (cs < 0) cs = last;
            // safe candidates with index <= c*, minus one
            const unsigned long long lo = cs < 64 ? (m0 & (~0ULL >> (63 - cs))) : m0;
            const unsigned long long hi = cs < 64 ? 0ULL : (m1 & (~0ULL >> (127 - cs)));
            pick = __popcll(lo) + __popcll(hi) - 1;
        }
        a.action[2 * env] = lds[kOffCand + 2 * pick];
        a.action[2 * env + 1] = lds[kOffCand + 2 * pick + 1];
        if (a.pick) a.pick[env] = pick;
        if (a.cstar) a.cstar[env] = cs;
        if (a.n_safe) a.n_safe[env] = n_safe;
    }
}

template <int NT>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void sqrl_act_kernel(const SqrlArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    sqrl_env<NT>(a, blockIdx.x, lds);
    rrl::advance_counter(a.counter_dev, a.counter_inc);
}

// S learners side by side (pack.hpp): workgroup b serves env `local` of seed s, on seed s's own argument block.  All seeds share
// NT (one k per call).  A seed's tick is advanced by the last of ITS n workgroups -- the grid's size says nothing about it --
// and a padding workgroup of a pinned mapping leaves before it touches anything, the ticket included.
template <int NT>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void sqrl_act_pack_kernel(const SqrlArgs* __restrict__ blocks, rrl_pack::Idx ix) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int s, local;
    if (!rrl_pack::locate(ix, blockIdx.x, s, local)) return;
    SqrlArgs a = blocks[s];
    rrl_pack::to_global_all(a.obs, a.head, a.scale, a.bias, a.W1, a.b1, a.W2p, a.b2, a.W3, a.b3, a.counter_dev, a.eps_in, a.u_in,
                            a.action, a.q, a.logp, a.cand, a.z, a.pick, a.cstar, a.n_safe);
    sqrl_env<NT>(a, local, lds);
    rrl::advance_counter_blocks(a.counter_dev, a.counter_inc, unsigned(a.n));
}

template <int NT>
int launch(const SqrlArgs& a, int n, hipStream_t st) {
    static bool lds_set = false;
    const int rc = grant_lds(sqrl_act_kernel<NT>, kLdsBytes, lds_set);
    if (rc != RRL_OK) return rc;
    hipLaunchKernelGGL(sqrl_act_kernel<NT>, dim3((unsigned)n), dim3(kThreads), kLdsBytes, st, a);
    return check_launch();
}

template <int NT>
int launch_pack(const rrl_pack::Plan& plan, hipStream_t st) {
    static bool lds_set = false;
    const int rc = grant_lds(sqrl_act_pack_kernel<NT>, kLdsBytes, lds_set);
    if (rc != RRL_OK) return rc;
    hipLaunchKernelGGL(sqrl_act_pack_kernel<NT>, dim3((unsigned)plan.grid), dim3(kThreads), kLdsBytes, st,
                       (const SqrlArgs*)plan.dev, plan.ix);
    return check_launch();
}

// the checks of one descriptor, before any launch (rrl_hip.h)
int check_desc(const rrl_sqrl_act_t* p) {
    if (!p || !p->obs || !p->head || !p->scale || !p->bias || !p->W1 || !p->b1 || !p->W2p || !p->b2 || !p->W3 || !p->b3 ||
        !p->action || p->n <= 0 || p->H != kH || p->d_obs != 2 || p->d_act != 2 || p->n_part < 1 || p->n_part > 4 ||
        (reinterpret_cast<uintptr_t>(p->W2p) & 15))
        return RRL_EINVAL;
    if (p->k < 1 || p->k > kMaxK || (long long)p->n * p->k >= (1LL << 32)) return RRL_ERANGE;
    return RRL_OK;
}

SqrlArgs block_of(const rrl_sqrl_act_t* p) {
    return SqrlArgs{p->k, p->n_part, p->n, p->part_stride, p->obs, p->head, p->scale, p->bias, p->W1, p->b1, p->W2p, p->b2,
                    p->W3, p->b3, p->eps_safe, p->seed, p->counter, p->counter_dev, p->counter_inc, p->eps_in, p->u_in,
                    p->action, p->q, p->logp, p->cand, p->z, p->pick, p->cstar, p->n_safe};
}

}  // namespace

extern "C" {

long long rrl_sqrl_scratch_floats(long long n, int k) {
    if (n <= 0) return RRL_EINVAL;
    if (k < 1 || k > kMaxK || n * k >= (1LL << 32)) return RRL_ERANGE;
    return 0;            // the one-kernel form keeps q, logp and the candidates in LDS
}

int rrl_sqrl_act(const rrl_sqrl_act_t* p, void* stream) {
    const int rc = check_desc(p);
    if (rc != RRL_OK) return rc;
    const SqrlArgs a = block_of(p);
    hipStream_t st = (hipStream_t)stream;
    switch ((p->k + 15) / 16) {
        case 1: return launch<1>(a, p->n, st);
        case 2: return launch<2>(a, p->n, st);
        case 3: return launch<3>(a, p->n, st);
        case 4: return launch<4>(a, p->n, st);
        case 5: return launch<5>(a, p->n, st);
        case 6: return launch<6>(a, p->n, st);
        case 7: return launch<7>(a, p->n, st);
        default: return launch<8>(a, p->n, st);
    }
}

int rrl_sqrl_act_packed(int S, const rrl_sqrl_act_t* args, void* stream) {
    if (S <= 0 || S > rrl_pack::kMaxSeeds || !args) return RRL_EINVAL;
    for (int s = 0; s < S; ++s) {               // every seed's descriptor is checked before anything is stored or launched
        const int rc = check_desc(args + s);
        if (rc != RRL_OK) return rc;
    }
    for (int s = 1; s < S; ++s)                 // NT is a template parameter of the kernel: one k per call
        if (args[s].k != args[0].k) return RRL_EINVAL;
    // one seed: the packed launch IS the solo launch (argument block in the kernel arguments, no plan)
    if (S == 1) return rrl_sqrl_act(args, stream);
    rrl_pack::Key key(rrl_pack::Site::SqrlAct, S);
    key.add(args, sizeof(rrl_sqrl_act_t) * S);
    hipStream_t st = (hipStream_t)stream;
    const rrl_pack::Plan* plan = rrl_pack::lookup(key);
    if (!plan) {
        std::vector<SqrlArgs> blocks(S);
        int count[rrl_pack::kMaxSeeds];
        for (int s = 0; s < S; ++s) {           // one workgroup per env, as in the solo kernel
            if (args[s].n > INT32_MAX / rrl_pack::kMaxSeeds) return RRL_ERANGE;     // the grid of any mapping fits an int
            blocks[s] = block_of(args + s);
            count[s] = args[s].n;
        }
        rrl_pack::Launch l = rrl_pack::place(S, count);
        l.i0 = (args[0].k + 15) / 16;
        plan = rrl_pack::publish(key, blocks, l, st);
        if (!plan) return rrl_pack::store_error();
    }
    switch (plan->i0) {
        case 1: return launch_pack<1>(*plan, st);
        case 2: return launch_pack<2>(*plan, st);
        case 3: return launch_pack<3>(*plan, st);
        case 4: return launch_pack<4>(*plan, st);
        case 5: return launch_pack<5>(*plan, st);
        case 6: return launch_pack<6>(*plan, st);
        case 7: return launch_pack<7>(*plan, st);
        default: return launch_pack<8>(*plan, st);
    }
}

}  // extern "C"
