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
// The matrix helpers are restated from plan_kernels.hip, not shared: a shared header would move that file's kernels.
#include "rrl_device.hpp"
#include "rrl_host.hpp"
#include "pack.hpp"

using namespace rrl_host;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kStreamSqrl = RRL_STREAM_SQRL, kStreamSqrlPick = RRL_STREAM_SQRL_PICK;
constexpr int kH = 256, kTiles = kH / 16;
constexpr int kMaxK = 128;                // candidates per env
constexpr int kRows = 64;                 // rows per pass: 4 row tiles, every wave owns 2 column tiles of all of them
constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;
constexpr int kActStride = kH + 4;        // +4 floats: row r starts at bank 4r, ds_read_b128 conflict-free
constexpr float kLogSigMax = 2.f, kLogSigMin = -20.f, kEps = 1e-6f;   // model.py:14-16
constexpr float kHalfLog2Pi = 0.918938533204672742f;

// LDS carve-up (floats)
constexpr int kOffAct = 0;                                   // [64][260] activations of the current pass
constexpr int kOffXs = kOffAct + kRows * kActStride;         // [64][4] (obs, candidate)
constexpr int kOffQpart = kOffXs + kRows * 4;                // [2 heads][8 waves][64 rows] partial last-layer sums
constexpr int kOffCand = kOffQpart + 2 * kWaves * kRows;     // [128][2] candidate actions
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

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// Identity the optimiser cannot see through: address arithmetic derived from opaque(lane) is redone per phase instead of
// being hoisted and kept live across the matrix loops.
__device__ __forceinline__ int opaque(int x) {
    asm volatile("" : "+v"(x));
    return x;
}
__device__ __forceinline__ float reluf(float x) { return x < 0.f ? 0.f : x; }   // NaN stays NaN (F.relu)
__device__ __forceinline__ float sigmoidf(float z) { return 1.f / (1.f + expf(-z)); }

// psum of update_kernels.hip: element idx of a stack output that arrives as np <= 4 partial sums, ((p0 + p1) + p2) + p3
__device__ __forceinline__ float psum(const float* p, long long idx, int np, long long ps) {
    const float v0 = p[idx];
    const float v1 = p[(np > 1 ? ps : 0) + idx];
    const float v2 = p[(np > 2 ? 2 * ps : 0) + idx];
    const float v3 = p[(np > 3 ? 3 * ps : 0) + idx];
    float v = v0;
    v = np > 1 ? v + v1 : v;
    v = np > 2 ? v + v2 : v;
    v = np > 3 ? v + v3 : v;
    return v;
}

// B fragments of K chunk j for this wave's two column tiles: W2p is [ct][j][lane] float4 (rrl_w2_pack), one coalesced
// 1 KB load per fragment
__device__ __forceinline__ void load_b(f32x4 (&b)[2], const float* __restrict__ w2p, const int (&ct)[2], int j, int lane) {
#pragma unroll
    for (int c = 0; c < 2; ++c)
        b[c] = *reinterpret_cast<const f32x4*>(w2p + ((size_t)(ct[c] * kTiles + j) * 64 + lane) * 4);
}

// acc[r][c] += act[row tile r, 16 j .. 16 j + 15] * W2[column tile ct[c]]; chunk step t uses k = 16 j + 4 (lane / 16) + t
template <int MR>
__device__ __forceinline__ void mma_chunk(f32x4 (&acc)[MR][2], const float* act, const f32x4 (&b)[2], int j, int lane) {
    f32x4 a[MR];
#pragma unroll
    for (int r = 0; r < MR; ++r)
        a[r] = *reinterpret_cast<const f32x4*>(act + (r * 16 + (lane & 15)) * kActStride + 16 * j + (lane >> 4) * 4);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < MR; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[r][c] = mfma(a[r][t], b[c][t], acc[r][c]);
}

// layer 2: the weight fragments of chunk j + 1 are requested before the MFMAs of chunk j (register double buffer)
template <int MR>
__device__ __forceinline__ void layer_mma(f32x4 (&acc)[MR][2], const float* act, const float* __restrict__ w2p,
                                          const int (&ct)[2], int lane) {
    f32x4 b0[2], b1[2];
    load_b(b0, w2p, ct, 0, lane);
    int j = 0;
#pragma unroll 1
    for (; j + 2 < kTiles; j += 2) {
        load_b(b1, w2p, ct, j + 1, lane);
        __builtin_amdgcn_sched_barrier(0);      // keep the prefetch ahead of the MFMAs it hides behind
        mma_chunk<MR>(acc, act, b0, j, lane);
        load_b(b0, w2p, ct, j + 2, lane);
        __builtin_amdgcn_sched_barrier(0);
        mma_chunk<MR>(acc, act, b1, j + 1, lane);
    }
    load_b(b1, w2p, ct, kTiles - 1, lane);
    mma_chunk<MR>(acc, act, b0, kTiles - 2, lane);
    mma_chunk<MR>(acc, act, b1, kTiles - 1, lane);
}

__device__ __forceinline__ float reduce16(float v) {   // sum over the 16 lanes that share lane / 16
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    return v;
}

// The twin heads on the first MR row tiles of xs; leaves qpart[h][wave][row] (the output's pre-activation is b3 + the sum
// over the 8 waves, added by the caller in wave order).  Ends with a barrier.
template <int MR>
__device__ __forceinline__ void q_phase(float* lds, const SqrlArgs& a, int wave, int lane) {
    const int ln = opaque(lane);
    const int ct[2] = {2 * wave, 2 * wave + 1};
    float* act = lds + kOffAct;
    const float* xs = lds + kOffXs;
    float* qpart = lds + kOffQpart;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        // epilogue constants first: their latency hides behind the matrix work
        float b1v[2], b2v[2], w3v[2], w1v[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int col = ct[c] * 16 + (ln & 15);
            b1v[c] = a.b1[h * kH + col];
            b2v[c] = a.b2[h * kH + col];
            w3v[c] = a.W3[h * kH + col];
            w1v[c] = a.W1[(h * kH + col) * 4 + (ln >> 4)];        // B operand of layer 1: W1[col][k = lane / 16]
        }
        f32x4 acc[MR][2];
#pragma unroll
        for (int r = 0; r < MR; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
        // layer 1: K = 4 inputs = ONE mfma per tile
#pragma unroll
        for (int r = 0; r < MR; ++r) {
            const float x = xs[(r * 16 + (ln & 15)) * 4 + (ln >> 4)];
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[r][c] = mfma(x, w1v[c], acc[r][c]);
        }
        // act[row][col] = relu(acc + b1[col]); C layout: row = 16 r + 4 (lane / 16) + i, col = 16 ct + lane % 16
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int col = ct[c] * 16 + (opaque(lane) & 15);
#pragma unroll
            for (int r = 0; r < MR; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    act[(r * 16 + 4 * (opaque(lane) >> 4) + i) * kActStride + col] = reluf(acc[r][c][i] + b1v[c]);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < MR; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
        layer_mma<MR>(acc, act, a.W2p + (size_t)h * kH * kH, ct, opaque(lane));
        // last layer folded in: z[row] = sum_col relu(h2 + b2) w3[col]
#pragma unroll
        for (int r = 0; r < MR; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < 2; ++c) s += reluf(acc[r][c][i] + b2v[c]) * w3v[c];
                const float v = reduce16(s);
                if ((ln & 15) == 0) qpart[(h * kWaves + wave) * kRows + r * 16 + 4 * (ln >> 4) + i] = v;
            }
        __syncthreads();       // act is free again; qpart[h] complete
    }
}

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
        float zv[2], q[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float v = a.b3[h];
#pragma unroll
            for (int w = 0; w < kWaves; ++w) v += lds[kOffQpart + (h * kWaves + w) * kRows + tid];
            zv[h] = v;
            q[h] = sigmoidf(v);
        }
        const float qm = (q[0] > q[1] || q[0] != q[0]) ? q[0] : q[1];      // torch.max: NaN propagates
        lds[kOffQ + c] = qm;
        if (a.q) a.q[env * k + c] = qm;
        if (a.z) {
            a.z[env * k + c] = zv[0];
            a.z[((long long)a.n + env) * k + c] = zv[1];
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

template <class K>
int grant_lds(K kernel, bool& done) {       // > 64 KB of LDS has to be granted explicitly, once per kernel
    if (done) return RRL_OK;
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes) != hipSuccess) {
        last_hip_error = int(hipGetLastError());
        return RRL_ELAUNCH;
    }
    done = true;
    return RRL_OK;
}

template <int NT>
int launch(const SqrlArgs& a, int n, hipStream_t st) {
    static bool lds_set = false;
    const int rc = grant_lds(sqrl_act_kernel<NT>, lds_set);
    if (rc != RRL_OK) return rc;
    hipLaunchKernelGGL(sqrl_act_kernel<NT>, dim3((unsigned)n), dim3(kThreads), kLdsBytes, st, a);
    return check_launch();
}

template <int NT>
int launch_pack(const rrl_pack::Plan& plan, hipStream_t st) {
    static bool lds_set = false;
    const int rc = grant_lds(sqrl_act_pack_kernel<NT>, lds_set);
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
    rrl_pack::Key key;
    key.pod(11);
    key.pod(S);
    key.add(args, sizeof(rrl_sqrl_act_t) * S);
    hipStream_t st = (hipStream_t)stream;
    rrl_pack::Plan* plan = rrl_pack::lookup(key);
    if (!plan) {
        std::vector<SqrlArgs> blocks(S);
        rrl_pack::Idx ix;
        ix.S = S;
        ix.first[0] = 0;
        for (int s = 0; s < S; ++s) {           // one workgroup per env, as in the solo kernel
            if (args[s].n > INT32_MAX / rrl_pack::kMaxSeeds) return RRL_ERANGE;     // the grid of any mapping fits an int
            blocks[s] = block_of(args + s);
            ix.first[s + 1] = ix.first[s] + args[s].n;
        }
        for (int s = S; s < rrl_pack::kMaxSeeds; ++s) ix.first[s + 1] = ix.first[S];
        plan = rrl_pack::store(key, blocks.data(), sizeof(SqrlArgs) * S, st);
        if (!plan) return rrl_pack::store_error();
        plan->grid = rrl_pack::finish(ix);
        plan->ix = ix;
        plan->i0 = (args[0].k + 15) / 16;
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
