// eval_kernels.hip -- policy evaluation (Experiment.get_test_rollout, recovery_rl/experiment.py:493-538) for gfx950: one
// deterministic-policy episode of n Navigation 1 / 2 or Maze envs -- reset, then T x (task policy -> Q_risk gate -> recovery
// policy -> transition), per-env return and flags -- as ONE launch with no launch boundary inside.
//
// The module path runs horizon + 1 times three nn.Linear stacks, an eager env step and a handful of small torch ops: a few
// thousand dependent launches.  Here a workgroup owns a tile of 16 envs for the whole rollout: the env state (double position,
// return, flags) lives in the registers of the workgroup's first 16 threads, the networks run on one row tile of the tile of
// qsample_kernels.hip -- activations in LDS at stride 260, W2 from L2 in MFMA fragment order (rrl_w2_pack), one coalesced
// 1 KB load per fragment, v_mfma_f32_16x16x4_f32 with k ascending, 8 waves with 2 column tiles each -- and no weight changes
// during the rollout, so nothing has to leave the workgroup between two steps.
//
// Rows per workgroup: 16, one MFMA row tile (the issue allows 16 .. 64).  The rollout is a chain of T dependent steps, each a
// few L2 round trips long, so width over the chip comes before rows per workgroup: 4096 envs are 256 workgroups, one per CU.
// Larger tiles would read W2 less often per env; no other tile size was built or timed, so that trade is NOT measured
// (DESIGN section 7 has the times as shipped).
//
// The stand-alone and the packed kernel (rrl_eval_rollout_packed: S seeds side by side, pack.hpp) have ONE body
// (rollout_tile); they differ only in where the argument block and the tile index come from.
//
// The tile's primitives and layer-2 helpers come from mfma_tile.hpp (one row tile: MR = 1); run_stack is this file's own,
// for its 16 rows, DIN < 4 inputs and NOUT outputs.  The body is generic over the env (a trait with reset and step, as
// step_push.hpp's): NavRoll restates nav_kernels.hip's NavEnv, MazeRoll is maze_device.hpp's transition behind kernels of
// its own (rrl_eval_rollout_maze[_packed]), so the Navigation kernels carry no Maze branch.
#include "maze_device.hpp"
#include "mfma_tile.hpp"
#include "pack.hpp"
#include "rrl_device.hpp"
#include "rrl_host.hpp"

using namespace rrl_host;

namespace {

using rrl_tile::f32x4;
using rrl_tile::kActStride;
using rrl_tile::kH;
using rrl_tile::kThreads;
using rrl_tile::kWaves;
using rrl_tile::layer_mma;
using rrl_tile::mfma;
using rrl_tile::opaque;
using rrl_tile::reduce16;
using rrl_tile::reluf;

constexpr uint32_t kStreamEval = RRL_STREAM_EVAL;
constexpr int kRows = 16;                 // rows per workgroup: one row tile, every wave owns 2 column tiles of it
constexpr int kMaxT = 4096, kMaxN = 1 << 22;

// LDS carve-up (floats)
constexpr int kOffAct = 0;                                   // [16][260] activations of the current stack
constexpr int kOffXs = kOffAct + kRows * kActStride;         // [16][4] (obs, task action)
constexpr int kOffPart = kOffXs + kRows * 4;                 // [2 outputs][8 waves][16 rows] partial last-layer sums
constexpr int kLdsFloats = kOffPart + 2 * kWaves * kRows;
constexpr int kLdsBytes = kLdsFloats * 4;                    // 17.5 KB

struct Net {
    const float *W1, *b1, *W2p, *b2, *W3, *b3;
};

struct EvArgs {
    int n, T, kind, reset;                    // reset: 0 or 1
    int blocks;                               // workgroups of this rollout
    const double* pos;
    Net p;
    const float *scale, *bias;
    Net q;
    float eps_safe;
    Net r;
    const float *rscale, *rbias, *rlog_std;
    float min_log_std;
    uint64_t seed, counter;
    uint64_t* counter_dev;
    float* ret;
    uint8_t *success, *violation;
    int32_t* steps;
    double* tr_pos;
    float *tr_task, *tr_real, *tr_z, *tr_eps, *tr_reward;
    uint8_t* tr_flags;
};

// One 2-hidden-layer stack (head `head` of w) on the row tile in xs: inputs = the first DIN columns of xs, outputs = the
// first NOUT rows of W3.  Leaves part[o][wave][row] (output o's pre-activation is b3[o] + the sum over the 8 waves, added by
// the caller in wave order).  Ends with a barrier.
template <int DIN, int NOUT>
__device__ __forceinline__ void run_stack(float* lds, const Net& w, int head, float* part, int wave, int lane) {
    const float* __restrict__ W1 = w.W1 + (size_t)head * kH * DIN;
    const float* __restrict__ b1 = w.b1 + head * kH;
    const float* __restrict__ W2p = w.W2p + (size_t)head * kH * kH;
    const float* __restrict__ b2 = w.b2 + head * kH;
    const float* __restrict__ W3 = w.W3 + head * kH * NOUT;
    const int ln = opaque(lane);
    const int ct[2] = {2 * wave, 2 * wave + 1};
    float* act = lds + kOffAct;
    const float* xs = lds + kOffXs;
    const int k1 = ln >> 4;                                  // layer 1's K index of this lane; inputs past DIN count as 0
    // epilogue constants first: their latency hides behind the matrix work
    float b1v[2], b2v[2], w3v[NOUT][2], w1v[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int col = ct[c] * 16 + (ln & 15);
        b1v[c] = b1[col];
        b2v[c] = b2[col];
#pragma unroll
        for (int o = 0; o < NOUT; ++o) w3v[o][c] = W3[o * kH + col];
        const float wv = W1[col * DIN + (k1 < DIN ? k1 : 0)];  // B operand of layer 1: W1[col][k]
        w1v[c] = k1 < DIN ? wv : 0.f;
    }
    f32x4 acc[1][2];
    // layer 1: K = 4 inputs = ONE mfma per column tile
    const float xv = xs[(ln & 15) * 4 + k1];
    const float x = k1 < DIN ? xv : 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[0][c] = mfma(x, w1v[c], f32x4{0.f, 0.f, 0.f, 0.f});
    // act[row][col] = relu(acc + b1[col]); C layout: row = 4 (lane / 16) + i, col = 16 ct + lane % 16
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int col = ct[c] * 16 + (opaque(lane) & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i) act[(4 * (opaque(lane) >> 4) + i) * kActStride + col] = reluf(acc[0][c][i] + b1v[c]);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[0][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    layer_mma<1>(acc, act, W2p, ct, opaque(lane));
    // last layer folded in: out_o[row] = sum_col relu(h2 + b2) W3[o][col]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 2; ++c) s += reluf(acc[0][c][i] + b2v[c]) * w3v[o][c];
            const float v = reduce16(s);
            if ((ln & 15) == 0) part[(o * kWaves + wave) * kRows + 4 * (ln >> 4) + i] = v;
        }
    __syncthreads();       // act is free again; part complete
}

// b3 + the eight waves' partial sums of output o, in wave order
__device__ __forceinline__ float fold_part(const float* part, int o, int row, float b3) {
    float v = b3;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) v += part[(o * kWaves + w) * kRows + row];
    return v;
}

// NavEnv::step of nav_kernels.hip: (next state, cost, constraint) of one transition
__device__ __forceinline__ bool nav_step(int kind, double x, double y, float ax, float ay, double ex, double ey, double& nx,
                                         double& ny, double& cost) {
    if (kind == RRL_ENV_NAV1) {
        rrl::nav_transition<0>(x, y, double(ax), double(ay), ex, ey, nx, ny, cost);
        return rrl::in_obstacle<0>(nx, ny);
    }
    rrl::nav_transition<1>(x, y, double(ax), double(ay), ex, ey, nx, ny, cost);
    return rrl::in_obstacle<1>(nx, ny);
}

// What one transition leaves: the next state, the reward and the three flags of the eager env's step()
struct Outcome {
    double nx, ny;
    float rew;
    bool cons, succ, done;
};

// Navigation 1 / 2: start at START + N(0, I); the cost is judged at the OLD state, done = success | constraint
struct NavRoll {
    __device__ __forceinline__ void reset(const EvArgs& a, long long row, uint64_t tick, double& x, double& y) const {
        double z0, z1;                                       // NavEnv::reset: START_STATE + randn(2)
        rrl::normal_at(a.seed, uint32_t(row), rrl::kStreamReset, tick, z0, z1);
        x = -50.0 + z0;
        y = 0.0 + z1;
    }
    __device__ __forceinline__ Outcome step(const EvArgs& a, long long row, uint64_t ctr, int, double x, double y, float ax,
                                            float ay) const {
        double ex, ey, nx, ny, cost;
        rrl::normal_at(a.seed, uint32_t(row), rrl::kStreamStep, ctr, ex, ey);
        const bool cons = nav_step(a.kind, x, y, ax, ay, ex, ey, nx, ny, cost);
        const bool sc = cost > -4.0;
        const bool dn = sc | cons;
        return Outcome{nx, ny, float(cost), cons, sc, dn};
    }
};

// Maze (MazeVecEnv(auto_reset=False), maze_kernels.hip's maze_step_kernel / MazeEnv): reset of mode 0 with the rejection
// loop; the step draws nothing, the reward is judged at the NEW state, and the env's own horizon ends a row with neither flag
struct MazeRoll {
    int horizon;
    __device__ __forceinline__ void reset(const EvArgs& a, long long row, uint64_t tick, double& x, double& y) const {
        rrl_maze::reset_one(a.seed, uint32_t(row), tick, 0, true, x, y);
    }
    __device__ __forceinline__ Outcome step(const EvArgs&, long long, uint64_t, int j, double x, double y, float ax,
                                            float ay) const {
        Outcome o;
        o.nx = x;
        o.ny = y;
        rrl_maze::move(o.nx, o.ny, double(ax), double(ay));  // clamps to +-0.1 itself
        const double d = rrl_maze::goal_distance(o.nx, o.ny);
        o.rew = float(-d);
        o.cons = rrl_maze::in_contact(o.nx, o.ny);
        o.succ = -d > -0.03;
        o.done = (j + 1 >= horizon) | o.cons | (d < rrl_maze::kGoalThresh);
        return o;
    }
};

// Workgroup b of the argument block's own grid: envs [16 b, 16 (b + 1)) through the whole rollout.  Thread tid < 16
// owns env 16 b + tid: state and results in its registers, written once at the end.
template <class Env>
__device__ __forceinline__ void rollout_tile(const EvArgs& a, const Env& env, unsigned b, float* lds) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int R = kRows;
    const long long row = (long long)b * R + tid;
    const bool mine = tid < R && row < a.n;                  // rows >= n: finite inputs, nothing read back, nothing written
    const uint64_t tick = rrl::effective_counter(a.counter, a.counter_dev);
    const bool has_q = a.q.W1 != nullptr, has_r = a.r.W1 != nullptr;
    float* xs = lds + kOffXs;
    float* part = lds + kOffPart;

    double x = 0.0, y = 0.0;
    if (mine) {
        if (a.reset) {
            env.reset(a, row, tick, x, y);
        } else {
            x = a.pos[2 * row];
            y = a.pos[2 * row + 1];
        }
    }
    bool alive = mine, succ = false, viol = false;
    float ret = 0.f;
    int steps = 0;

#pragma unroll 1
    for (int j = 0; j < a.T; ++j) {
        if (tid < kRows) *reinterpret_cast<f32x4*>(xs + tid * 4) = f32x4{float(x), float(y), 0.f, 0.f};
        if (!__syncthreads_or(int(alive))) break;            // every row of the tile has finished its episode
        const uint64_t ctr = tick + uint64_t(a.reset) + uint64_t(j);

        // ---- task action: the Gaussian policy's mean rows ----
        run_stack<2, 2>(lds, a.p, 0, part, wave, lane);
        float t0 = 0.f, t1 = 0.f;
        if (tid < R) {
            t0 = tanhf(fold_part(part, 0, tid, a.p.b3[0])) * a.scale[0] + a.bias[0];
            t1 = tanhf(fold_part(part, 1, tid, a.p.b3[1])) * a.scale[1] + a.bias[1];
            xs[tid * 4 + 2] = t0;
            xs[tid * 4 + 3] = t1;
        }
        float r0 = t0, r1 = t1, z0 = 0.f, z1 = 0.f, e0 = 0.f, e1 = 0.f;
        bool rec = false;
        if (has_q) {
            // ---- the gate: twin Q_risk on [obs | task action] ----
            __syncthreads();                                  // xs complete
#pragma unroll 1
            for (int h = 0; h < 2; ++h) run_stack<4, 1>(lds, a.q, h, part + h * kWaves * kRows, wave, lane);
            if (tid < R) {
                z0 = fold_part(part, 0, tid, a.q.b3[0]);
                z1 = fold_part(part, 1, tid, a.q.b3[1]);
                rec = alive && rrl::recovery_gate(z0, z1, a.eps_safe);
            }
            // ---- recovery action, when a row of the tile asks for one (the fold above is behind this barrier) ----
            const bool any = has_r && __syncthreads_or(int(rec));
            if (any) run_stack<2, 2>(lds, a.r, 0, part, wave, lane);
            if (has_r && alive && (rec || a.tr_eps)) {
                double d0, d1;
                rrl::normal_at(a.seed, uint32_t(row), kStreamEval, ctr, d0, d1);
                e0 = float(d0);
                e1 = float(d1);
            }
            if (any && rec) {
                r0 = tanhf(fold_part(part, 0, tid, a.r.b3[0])) * a.rscale[0] + a.rbias[0] +
                     expf(fmaxf(a.rlog_std[0], a.min_log_std)) * e0;
                r1 = tanhf(fold_part(part, 1, tid, a.r.b3[1])) * a.rscale[1] + a.rbias[1] +
                     expf(fmaxf(a.rlog_std[1], a.min_log_std)) * e1;
            }
        }

        // ---- transition ----
        if (alive) {
            const long long o = (long long)j * a.n + row;
            const Outcome t = env.step(a, row, ctr, j, x, y, r0, r1);
            const bool cons = t.cons, sc = t.succ, dn = t.done;
            const float rew = t.rew;
            if (a.tr_pos) {
                a.tr_pos[2 * o] = x;
                a.tr_pos[2 * o + 1] = y;
            }
            if (a.tr_task) {
                a.tr_task[2 * o] = t0;
                a.tr_task[2 * o + 1] = t1;
            }
            if (a.tr_real) {
                a.tr_real[2 * o] = r0;
                a.tr_real[2 * o + 1] = r1;
            }
            if (a.tr_z && has_q) {
                a.tr_z[(long long)(2 * j) * a.n + row] = z0;
                a.tr_z[(long long)(2 * j + 1) * a.n + row] = z1;
            }
            if (a.tr_eps && has_r) {
                a.tr_eps[2 * o] = e0;
                a.tr_eps[2 * o + 1] = e1;
            }
            if (a.tr_reward) a.tr_reward[o] = rew;
            if (a.tr_flags) a.tr_flags[o] = uint8_t(1 | (int(dn) << 1) | (int(cons) << 2) | (int(sc) << 3) | (int(rec) << 4));
            ret += rew;
            succ |= sc;
            viol |= cons;
            ++steps;
            x = t.nx;
            y = t.ny;
            alive = !dn;
        }
    }
    if (mine) {
        a.ret[row] = ret;
        a.success[row] = uint8_t(succ);
        a.violation[row] = uint8_t(viol);
        a.steps[row] = steps;
    }
    rrl::advance_counter_blocks(a.counter_dev, uint64_t(a.T) + uint64_t(a.reset), unsigned(a.blocks));
}

__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void eval_rollout_kernel(const EvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    rollout_tile(a, NavRoll{}, blockIdx.x, lds);
}

// The copied argument block's pointers as global ones (pack.hpp: to_global)
__device__ __forceinline__ void globalize(Net& w) { rrl_pack::to_global_all(w.W1, w.b1, w.W2p, w.b2, w.W3, w.b3); }
__device__ __forceinline__ void globalize(EvArgs& a) {
    globalize(a.p);
    globalize(a.q);
    globalize(a.r);
    rrl_pack::to_global_all(a.pos, a.scale, a.bias, a.rscale, a.rbias, a.rlog_std, a.counter_dev, a.ret, a.success, a.violation,
                            a.steps, a.tr_pos, a.tr_task, a.tr_real, a.tr_z, a.tr_eps, a.tr_reward, a.tr_flags);
}

// S evaluations side by side (pack.hpp): workgroup b serves tile `local` of seed s's own grid, on seed s's argument block.
// A padding workgroup of a pinned mapping leaves before it touches anything.
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void eval_rollout_pack_kernel(const EvArgs* __restrict__ blocks, rrl_pack::Idx ix) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int s, local;
    if (!rrl_pack::locate(ix, blockIdx.x, s, local)) return;
    EvArgs a = blocks[s];
    globalize(a);
    rollout_tile(a, NavRoll{}, unsigned(local), lds);
}

// The Maze kernels: the same body on MazeRoll.  The argument block is EvArgs unchanged; the horizon rides beside it (the
// solo kernel's second argument, MazeBlock's tail in a packed plan), so the Navigation kernels' argument offsets stay put.
struct MazeBlock {
    EvArgs a;
    int horizon;
};

__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void eval_rollout_maze_kernel(const EvArgs a, int horizon) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    rollout_tile(a, MazeRoll{horizon}, blockIdx.x, lds);
}

__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void eval_rollout_maze_pack_kernel(const MazeBlock* __restrict__ blocks, rrl_pack::Idx ix) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int s, local;
    if (!rrl_pack::locate(ix, blockIdx.x, s, local)) return;
    EvArgs a = blocks[s].a;
    const int horizon = blocks[s].horizon;
    globalize(a);
    rollout_tile(a, MazeRoll{horizon}, unsigned(local), lds);
}

template <size_t N>
int given(const void* const (&p)[N]) {
    int k = 0;
    for (const void* q : p) k += q != nullptr;
    return k;
}

constexpr int kMaxHorizon = 1 << 30;

// the checks of a descriptor, before any launch (rrl_hip.h); maze: the entry's env is Maze, else Navigation 1 / 2
int check_desc(const rrl_eval_rollout_t* p, bool maze = false) {
    if (!p) return RRL_EINVAL;
    const void* const need[] = {p->pW1, p->pb1, p->pW2p, p->pb2, p->pW3, p->pb3, p->scale, p->bias,
                                p->ret, p->success, p->violation, p->steps};
    const void* const qg[] = {p->qW1, p->qb1, p->qW2p, p->qb2, p->qW3, p->qb3};
    const void* const rg[] = {p->rW1, p->rb1, p->rW2p, p->rb2, p->rW3, p->rb3, p->rscale, p->rbias, p->rlog_std};
    const int nq = given(qg), nr = given(rg);
    const auto aligned = [](const void* w) { return (reinterpret_cast<uintptr_t>(w) & 15) == 0; };
    if (given(need) != 12 || (nq != 0 && nq != 6) || (nr != 0 && nr != 9) || (nr && !nq) || p->H != kH || p->d_obs != 2 ||
        p->d_act != 2 || p->n <= 0 || !(maze ? p->env_kind == RRL_ENV_MAZE : (p->env_kind == RRL_ENV_NAV1 || p->env_kind == RRL_ENV_NAV2)) ||
        !aligned(p->pW2p) ||
        !aligned(p->qW2p) || !aligned(p->rW2p) || (!p->reset && !p->pos))
        return RRL_EINVAL;
    if (p->T < 1 || p->T > kMaxT || p->n > kMaxN) return RRL_ERANGE;
    return RRL_OK;
}

EvArgs block_of(const rrl_eval_rollout_t* p) {
    EvArgs a{};
    a.n = p->n;
    a.T = p->T;
    a.kind = p->env_kind;
    a.reset = p->reset ? 1 : 0;
    a.blocks = (p->n + kRows - 1) / kRows;
    a.pos = p->pos;
    a.p = Net{p->pW1, p->pb1, p->pW2p, p->pb2, p->pW3, p->pb3};
    a.scale = p->scale;
    a.bias = p->bias;
    a.q = Net{p->qW1, p->qb1, p->qW2p, p->qb2, p->qW3, p->qb3};
    a.eps_safe = p->eps_safe;
    a.r = Net{p->rW1, p->rb1, p->rW2p, p->rb2, p->rW3, p->rb3};
    a.rscale = p->rscale;
    a.rbias = p->rbias;
    a.rlog_std = p->rlog_std;
    a.min_log_std = p->min_log_std;
    a.seed = p->seed;
    a.counter = p->counter;
    a.counter_dev = p->counter_dev;
    a.ret = p->ret;
    a.success = p->success;
    a.violation = p->violation;
    a.steps = p->steps;
    a.tr_pos = p->tr_pos;
    a.tr_task = p->tr_task;
    a.tr_real = p->tr_real;
    a.tr_z = p->tr_z;
    a.tr_eps = p->tr_eps;
    a.tr_reward = p->tr_reward;
    a.tr_flags = p->tr_flags;
    return a;
}

int launch_solo(const rrl_eval_rollout_t* p, void* stream) {
    const int rc = check_desc(p);
    if (rc != RRL_OK) return rc;
    const EvArgs a = block_of(p);
    hipLaunchKernelGGL(eval_rollout_kernel, dim3((unsigned)a.blocks), dim3(kThreads), kLdsBytes, (hipStream_t)stream, a);
    return check_launch();
}

int check_maze(const rrl_eval_rollout_t* p, int horizon) {
    const int rc = check_desc(p, true);
    if (rc != RRL_OK) return rc;
    return horizon < 1 || horizon > kMaxHorizon ? RRL_ERANGE : RRL_OK;
}

int launch_maze_solo(const rrl_eval_rollout_t* p, int horizon, void* stream) {
    const int rc = check_maze(p, horizon);
    if (rc != RRL_OK) return rc;
    const EvArgs a = block_of(p);
    hipLaunchKernelGGL(eval_rollout_maze_kernel, dim3((unsigned)a.blocks), dim3(kThreads), kLdsBytes, (hipStream_t)stream, a,
                       horizon);
    return check_launch();
}

}  // namespace

extern "C" {

int rrl_eval_rollout(const rrl_eval_rollout_t* p, void* stream) { return launch_solo(p, stream); }

int rrl_eval_rollout_packed(int S, const rrl_eval_rollout_t* args, void* stream) {
    if (!args) return RRL_EINVAL;
    if (S <= 0 || S > rrl_pack::kMaxSeeds) return RRL_ERANGE;
    int worst = RRL_OK;
    for (int s = 0; s < S; ++s) {               // every seed is checked before anything is stored or launched
        const int rc = check_desc(args + s);
        if (rc == RRL_EINVAL) return rc;        // an invalid field wins over a size out of range, whichever seed has it
        if (rc != RRL_OK) worst = rc;
    }
    if (worst != RRL_OK) return worst;
    // one seed: the packed launch IS the solo launch (argument block in the kernel arguments, no plan)
    if (S == 1) return launch_solo(args, stream);
    rrl_pack::Key key;
    key.pod(13);
    key.pod(S);
    key.add(args, sizeof(rrl_eval_rollout_t) * S);
    hipStream_t st = (hipStream_t)stream;
    rrl_pack::Plan* plan = rrl_pack::lookup(key);
    if (!plan) {
        std::vector<EvArgs> blocks(S);
        int count[rrl_pack::kMaxSeeds];
        for (int s = 0; s < S; ++s) {
            blocks[s] = block_of(args + s);
            count[s] = blocks[s].blocks;            // <= 2^18 workgroups per seed: any mapping's grid fits an int
        }
        rrl_pack::Idx ix;
        rrl_pack::ranges(ix, S, count);
        const int grid = rrl_pack::finish(ix);
        plan = rrl_pack::store(key, blocks.data(), sizeof(EvArgs) * S, st);
        if (!plan) return rrl_pack::store_error();
        plan->grid = grid;
        plan->ix = ix;
    }
    hipLaunchKernelGGL(eval_rollout_pack_kernel, dim3((unsigned)plan->grid), dim3(kThreads), kLdsBytes, st,
                       (const EvArgs*)plan->dev, plan->ix);
    return check_launch();
}

int rrl_eval_rollout_maze(const rrl_eval_rollout_t* p, int horizon, void* stream) {
    return launch_maze_solo(p, horizon, stream);
}

int rrl_eval_rollout_maze_packed(int S, const rrl_eval_rollout_t* args, const int* horizon, void* stream) {
    if (!args || !horizon) return RRL_EINVAL;
    if (S <= 0 || S > rrl_pack::kMaxSeeds) return RRL_ERANGE;
    int worst = RRL_OK;
    for (int s = 0; s < S; ++s) {               // every seed is checked before anything is stored or launched
        const int rc = check_maze(args + s, horizon[s]);
        if (rc == RRL_EINVAL) return rc;        // an invalid field wins over a size out of range, whichever seed has it
        if (rc != RRL_OK) worst = rc;
    }
    if (worst != RRL_OK) return worst;
    if (S == 1) return launch_maze_solo(args, horizon[0], stream);
    rrl_pack::Key key;
    key.pod(14);
    key.pod(S);
    key.add(args, sizeof(rrl_eval_rollout_t) * S);
    key.add(horizon, sizeof(int) * S);
    hipStream_t st = (hipStream_t)stream;
    rrl_pack::Plan* plan = rrl_pack::lookup(key);
    if (!plan) {
        std::vector<MazeBlock> blocks(S);
        int count[rrl_pack::kMaxSeeds];
        for (int s = 0; s < S; ++s) {
            blocks[s] = MazeBlock{block_of(args + s), horizon[s]};
            count[s] = blocks[s].a.blocks;
        }
        rrl_pack::Idx ix;
        rrl_pack::ranges(ix, S, count);
        const int grid = rrl_pack::finish(ix);
        plan = rrl_pack::store(key, blocks.data(), sizeof(MazeBlock) * S, st);
        if (!plan) return rrl_pack::store_error();
        plan->grid = grid;
        plan->ix = ix;
    }
    hipLaunchKernelGGL(eval_rollout_maze_pack_kernel, dim3((unsigned)plan->grid), dim3(kThreads), kLdsBytes, st,
                       (const MazeBlock*)plan->dev, plan->ix);
    return check_launch();
}

}  // extern "C"
