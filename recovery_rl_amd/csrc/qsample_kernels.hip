// qsample_kernels.hip -- Q-sampling recovery (QRiskWrapper.select_action, recovery_rl/qrisk.py:214-225) for gfx950: per GATED
// env, k uniform candidate actions from the action box, the twin Q_risk on every candidate, and the argmin.
//
// The module path expands every observation to k = 1000 rows and runs Q_risk on n k rows, gated or not.  Here work follows
// the gate: the grid is n x ceil(k / 128) workgroups, a workgroup of an env whose gate did not fire leaves before it reads a
// weight, and a gated env's candidates are spread over its P = ceil(k / 128) workgroups (a handful of gated envs then puts
// one chunk, not k rows, on the critical path).  A workgroup scores its chunk in passes of up to 64 rows -- the tile of
// sqrl_kernels.hip: activations in LDS, W2 from L2 in MFMA fragment order (rrl_w2_pack), v_mfma_f32_16x16x4_f32 -- and leaves
// (smallest q, its index, that candidate) in scratch; a second small kernel folds an env's P partials in ascending chunk
// order, writes action[e] and advances the tick.
//
// The recovery gate is either a mask (rrl_qsample_act) or evaluated here from Q_risk's partial last-layer sums
// (rrl_qsample_act_gated: what rrl_recovery_select would have left, without its launch and without the summing one).  Both
// kernels have ONE body (score_chunk, fold_envs); the stand-alone and the packed kernels (rrl_qsample_act_packed: S seeds side
// by side, pack.hpp) differ only in where the argument block and (env, chunk) come from.
//
// The tile and the twin-head phase (q_phase) come from mfma_tile.hpp, shared with sqrl_kernels.hip.
#include "mfma_tile.hpp"
#include "pack.hpp"
#include "rrl_device.hpp"
#include "rrl_host.hpp"

using namespace rrl_host;
using namespace rrl_tile;

namespace {

constexpr uint32_t kStreamQsample = RRL_STREAM_QSAMPLE;
constexpr int kMaxK = 1024;               // candidates per env
constexpr int kChunk = 128;               // candidates per workgroup
constexpr int kPartial = 4;               // floats of a workgroup's partial: key, index (int bits), candidate x, y

// LDS carve-up (floats), behind the tile's act / xs / qpart
constexpr int kOffCand = kOffOwn;                            // [128][2] candidate actions of the chunk
constexpr int kOffQ = kOffCand + kChunk * 2;                 // [128] max(sigmoid z0, sigmoid z1)
constexpr int kLdsFloats = kOffQ + kChunk;
constexpr int kLdsBytes = kLdsFloats * 4;                    // 73.2 KB: two workgroups per CU

struct QsArgs {
    int k, n, P;                              // P = chunks per env
    const float* obs;
    const uint8_t* mask;
    const float *lo, *hi;
    const float *W1, *b1, *W2p, *b2, *W3, *b3;
    uint64_t seed, counter;
    uint64_t* counter_dev;
    uint64_t counter_inc;
    const float* cand_in;
    float* scratch;
    float* action;
    float *q, *z, *cand;
    int32_t* pick;
    // the gate evaluated in the launch (gz != nullptr; mask is NULL then): rrl_qsample_gate_t
    const float* gz;
    int g_np;
    long long g_ps;
    float g_eps;
    const float* g_task;
    int g_ld;
    float* g_task_out;
    uint8_t* g_rec_out;
};

// Did env e's gate fire?  From the mask, or from the 2 x n_part partial sums of z = Q_risk(s, a_task), added in the fixed order
// every consumer of a stack output uses.  Eight loads are requested together whatever n_part is -- partial 0 is read again in
// the place of an absent one, as the env-step kernel does: no branch between the requests.
__device__ __forceinline__ bool gate_fired(const QsArgs& a, long long e) {
    if (!a.gz) return !a.mask || a.mask[e];
    const int np = a.g_np;
    float zu[4], zw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long off = np > k ? k * a.g_ps : 0;
        zu[k] = a.gz[off + e];
        zw[k] = a.gz[off + a.n + e];
    }
    float z0 = zu[0], z1 = zw[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        z0 = np > k ? z0 + zu[k] : z0;
        z1 = np > k ? z1 + zw[k] : z1;
    }
    return rrl::recovery_gate(z0, z1, a.g_eps);
}

// One pass: rows [base, base + 16 MR) of the chunk's `rows` candidates (candidate c0 + row of env) through the twin heads;
// q (and z) of the live ones.
template <int MR>
__device__ __forceinline__ void score_pass(float* lds, const QsArgs& a, long long env, int c0, int rows, int base, float ox,
                                           float oy, int tid, int wave, int lane) {
    if (tid < kRows) {
        const int r = base + tid;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};           // rows past the chunk: finite inputs, results never read
        if (r < rows) x = f32x4{ox, oy, lds[kOffCand + 2 * r], lds[kOffCand + 2 * r + 1]};
        *reinterpret_cast<f32x4*>(lds + kOffXs + tid * 4) = x;
    }
    __syncthreads();
    q_phase<MR>(lds, a, wave, lane);
    if (tid < kRows && base + tid < rows) {
        const int r = base + tid;
        const TwinQ t = twin_q(lds, a, tid);
        lds[kOffQ + r] = t.q;
        const long long row = env * a.k + c0 + r;
        if (a.q) a.q[row] = t.q;
        if (a.z) {
            a.z[row] = t.z[0];
            a.z[(long long)a.n * a.k + row] = t.z[1];
        }
    }
    // xs and qpart are rewritten only behind the next pass's barriers
}

// Workgroup b = env b / P, chunk b % P of the argument block's own grid: candidates [128 chunk, 128 chunk + rows) of a gated
// env -> scratch[b] = its partial.  Reads the tick, never writes it (the fold kernel advances it).
__device__ __forceinline__ void score_chunk(const QsArgs& a, unsigned b, float* lds) {
    const long long env = b / (unsigned)a.P;
    if (!gate_fired(a, env)) return;              // the gate did not fire: nothing else read, nothing written
    const int chunk = b % (unsigned)a.P;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = a.k, c0 = chunk * kChunk;
    const int rows = k - c0 < kChunk ? k - c0 : kChunk;
    const uint64_t ctr = rrl::effective_counter(a.counter, a.counter_dev);

    // ---- candidates: a_j = float(lo_j + (hi_j - lo_j) u_j) in double, u = the open-unit pair of the row's 128 bits ----
    if (tid < rows) {
        const long long row = env * k + c0 + tid;
        float c2[2];
        if (a.cand_in) {
            c2[0] = a.cand_in[2 * row];
            c2[1] = a.cand_in[2 * row + 1];
        } else {
            const rrl::Bits128 bits = rrl::philox_at(a.seed, uint32_t(row), kStreamQsample, ctr);
            const double u[2] = {rrl::unit_open(bits.lo), rrl::unit_open(bits.hi)};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const double l = double(a.lo[j]), h = double(a.hi[j]);
                c2[j] = float(l + (h - l) * u[j]);
            }
        }
        lds[kOffCand + 2 * tid] = c2[0];
        lds[kOffCand + 2 * tid + 1] = c2[1];
        if (a.cand) {
            a.cand[2 * row] = c2[0];
            a.cand[2 * row + 1] = c2[1];
        }
    }
    const float ox = a.obs[2 * env], oy = a.obs[2 * env + 1];
    __syncthreads();

    // ---- scores: row tiles of 16, at most four per pass ----
    const int nt = (rows + 15) >> 4;
#pragma unroll 1
    for (int base = 0; base < rows; base += kRows) {
        const int mr = nt - (base >> 4);
        switch (mr) {
            case 1: score_pass<1>(lds, a, env, c0, rows, base, ox, oy, tid, wave, lane); break;
            case 2: score_pass<2>(lds, a, env, c0, rows, base, ox, oy, tid, wave, lane); break;
            case 3: score_pass<3>(lds, a, env, c0, rows, base, ox, oy, tid, wave, lane); break;
            default: score_pass<4>(lds, a, env, c0, rows, base, ox, oy, tid, wave, lane); break;
        }
    }
    __syncthreads();                              // q of every candidate of the chunk is in LDS

    // ---- the chunk's argmin, lowest index on ties; NaN counts as the smallest (torch.argmin) ----
    if (wave == 0) {
        float best = __builtin_inff();
        int bidx = kChunk;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int r = lane + 64 * hf;
            if (r < rows) {
                const float qv = lds[kOffQ + r];
                const float key = qv != qv ? -__builtin_inff() : qv;
                if (key < best) {                 // ascending r: strict < keeps the lower index
                    best = key;
                    bidx = r;
                }
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float ob = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bidx, off, 64);
            if (ob < best || (ob == best && oi < bidx)) {
                best = ob;
                bidx = oi;
            }
        }
        if (lane == 0) {
            float* part = a.scratch + (size_t)b * kPartial;
            part[0] = best;
            part[1] = __int_as_float(c0 + bidx);
            part[2] = lds[kOffCand + 2 * bidx];
            part[3] = lds[kOffCand + 2 * bidx + 1];
        }
    }
}

__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void qsample_score_kernel(const QsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    score_chunk(a, blockIdx.x, lds);
}

// The copied argument block's pointers as global ones (pack.hpp: to_global)
__device__ __forceinline__ void globalize(QsArgs& a) {
    rrl_pack::to_global_all(a.obs, a.mask, a.lo, a.hi, a.W1, a.b1, a.W2p, a.b2, a.W3, a.b3, a.counter_dev, a.cand_in, a.scratch,
                            a.action, a.q, a.z, a.cand, a.pick, a.gz, a.g_task, a.g_task_out, a.g_rec_out);
}

// S learners side by side (pack.hpp): workgroup b serves workgroup `local` of seed s's own n x P grid, on seed s's argument
// block.  A padding workgroup of a pinned mapping leaves before it touches anything.
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void qsample_score_pack_kernel(const QsArgs* __restrict__ blocks, rrl_pack::Idx ix) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int s, local;
    if (!rrl_pack::locate(ix, blockIdx.x, s, local)) return;
    QsArgs a = blocks[s];
    globalize(a);
    score_chunk(a, unsigned(local), lds);
}

// One thread per env (envs e0, e0 + stride, ...): with a gate in the launch, recovery_out[e], task_out[e] and the task action
// into action[e] of an env whose gate did not fire -- what rrl_recovery_select leaves; then the P partials of a gated env in
// ascending chunk order (strict <: the lowest index wins) -> action[e] (and pick[e]).  The thread of env 0 advances the tick:
// every reader of it ran in the score kernel before this one.
__device__ __forceinline__ void fold_envs(const QsArgs& a, long long e0, long long stride) {
    for (long long e = e0; e < a.n; e += stride) {
        const bool rec = gate_fired(a, e);
        if (a.gz) {
            const float t0 = a.g_task[e * a.g_ld], t1 = a.g_task[e * a.g_ld + 1];
            a.g_rec_out[e] = uint8_t(rec);
            if (a.g_task_out) {
                a.g_task_out[2 * e] = t0;
                a.g_task_out[2 * e + 1] = t1;
            }
            if (!rec) {
                a.action[2 * e] = t0;
                a.action[2 * e + 1] = t1;
            }
        }
        if (!rec) continue;
        const float* part = a.scratch + (size_t)e * a.P * kPartial;
        float best = part[0];
        int p = 0;
        for (int c = 1; c < a.P; ++c)
            if (part[c * kPartial] < best) {
                best = part[c * kPartial];
                p = c;
            }
        a.action[2 * e] = part[p * kPartial + 2];
        a.action[2 * e + 1] = part[p * kPartial + 3];
        if (a.pick) a.pick[e] = __float_as_int(part[p * kPartial + 1]);
    }
    if (e0 == 0 && a.counter_dev && a.counter_inc) a.counter_dev[0] += a.counter_inc;
}

__global__ __launch_bounds__(kBlock) void qsample_fold_kernel(const QsArgs a) {
    fold_envs(a, (long long)blockIdx.x * kBlock + threadIdx.x, (long long)gridDim.x * kBlock);
}

// ... of S seeds: seed s's envs on its own ix.first[s + 1] - ix.first[s] = grid_for(n[s]) workgroups; its tick is advanced by the
// thread of ITS env 0, whatever the grid holds
__global__ __launch_bounds__(kBlock) void qsample_fold_pack_kernel(const QsArgs* __restrict__ blocks, rrl_pack::Idx ix) {
    int s, local;
    if (!rrl_pack::locate(ix, blockIdx.x, s, local)) return;
    QsArgs a = blocks[s];
    globalize(a);
    fold_envs(a, (long long)local * kBlock + threadIdx.x, (long long)(ix.first[s + 1] - ix.first[s]) * kBlock);
}

int chunks_of(int k) { return (k + kChunk - 1) / kChunk; }

// the checks of a descriptor, before any launch (rrl_hip.h)
int check_desc(const rrl_qsample_act_t* p) {
    if (!p || !p->obs || !p->lo || !p->hi || !p->W1 || !p->b1 || !p->W2p || !p->b2 || !p->W3 || !p->b3 || !p->scratch ||
        !p->action || p->n <= 0 || p->H != kH || p->d_obs != 2 || p->d_act != 2 || (reinterpret_cast<uintptr_t>(p->W2p) & 15))
        return RRL_EINVAL;
    if (p->k < 1 || p->k > kMaxK || (long long)p->n * p->k >= (1LL << 32)) return RRL_ERANGE;
    return RRL_OK;
}

// ... and of a gate given with it
int check_both(const rrl_qsample_act_t* p, const rrl_qsample_gate_t* g) {
    const int rc = check_desc(p);
    if (!g || rc == RRL_EINVAL) return rc;
    if (p->mask || !g->z || !g->task_action || !g->recovery_out || g->n_part < 1 || g->n_part > 4 || g->ld_task < 2 ||
        (g->ld_task & 1))
        return RRL_EINVAL;                  // an invalid field wins over a size out of range
    return rc;
}

QsArgs block_of(const rrl_qsample_act_t* p, const rrl_qsample_gate_t* g) {
    QsArgs a{p->k, p->n, chunks_of(p->k), p->obs, p->mask, p->lo, p->hi, p->W1, p->b1, p->W2p, p->b2, p->W3, p->b3,
             p->seed, p->counter, p->counter_dev, p->counter_inc, p->cand_in, p->scratch, p->action, p->q, p->z,
             p->cand, p->pick, nullptr, 1, 0, 0.f, nullptr, 2, nullptr, nullptr};
    if (g) {
        a.gz = g->z;
        a.g_np = g->n_part;
        a.g_ps = g->part_stride;
        a.g_eps = g->eps_safe;
        a.g_task = g->task_action;
        a.g_ld = g->ld_task;
        a.g_task_out = g->task_out;
        a.g_rec_out = g->recovery_out;
    }
    return a;
}

// rrl_qsample_act (g == nullptr) and rrl_qsample_act_gated: the two kernels on one argument block
int launch_solo(const rrl_qsample_act_t* p, const rrl_qsample_gate_t* g, void* stream) {
    const int rc = check_both(p, g);
    if (rc != RRL_OK) return rc;
    const QsArgs a = block_of(p, g);
    hipStream_t st = (hipStream_t)stream;
    static bool lds_set = false;
    const int rl = grant_lds(qsample_score_kernel, kLdsBytes, lds_set);
    if (rl != RRL_OK) return rl;
    hipLaunchKernelGGL(qsample_score_kernel, dim3((unsigned)((long long)a.n * a.P)), dim3(kThreads), kLdsBytes, st, a);
    const int rs = check_launch();
    if (rs != RRL_OK) return rs;
    hipLaunchKernelGGL(qsample_fold_kernel, dim3((unsigned)grid_for(a.n)), dim3(kBlock), 0, st, a);
    return check_launch();
}

}  // namespace

extern "C" {

long long rrl_qsample_scratch_floats(long long n, int k) {
    if (n <= 0) return RRL_EINVAL;
    if (k < 1 || k > kMaxK || n * k >= (1LL << 32)) return RRL_ERANGE;
    return n * chunks_of(k) * kPartial;      // one partial per workgroup of the score kernel
}

int rrl_qsample_act(const rrl_qsample_act_t* p, void* stream) { return launch_solo(p, nullptr, stream); }

int rrl_qsample_act_gated(const rrl_qsample_act_t* p, const rrl_qsample_gate_t* g, void* stream) {
    if (!g) return RRL_EINVAL;
    return launch_solo(p, g, stream);
}

int rrl_qsample_act_packed(int S, const rrl_qsample_act_t* args, const rrl_qsample_gate_t* gates, void* stream) {
    if (S <= 0 || S > rrl_pack::kMaxSeeds || !args) return RRL_EINVAL;
    for (int s = 0; s < S; ++s) {               // every seed is checked before anything is stored or launched
        const int rc = check_both(args + s, gates ? gates + s : nullptr);
        if (rc != RRL_OK) return rc;
    }
    // one seed: the packed launch IS the solo launch (argument block in the kernel arguments, no plan)
    if (S == 1) return launch_solo(args, gates, stream);
    for (int s = 0; s < S; ++s)                 // the grid of any mapping fits an int
        if ((long long)args[s].n * chunks_of(args[s].k) > INT32_MAX / rrl_pack::kMaxSeeds) return RRL_ERANGE;
    rrl_pack::Key key(rrl_pack::Site::QsampleAct, S);
    key.pod(int(gates != nullptr));
    key.add(args, sizeof(rrl_qsample_act_t) * S);
    if (gates) key.add(gates, sizeof(rrl_qsample_gate_t) * S);
    hipStream_t st = (hipStream_t)stream;
    const rrl_pack::Plan* plan = rrl_pack::lookup(key);
    if (!plan) {
        std::vector<QsArgs> blocks(S);
        int score[rrl_pack::kMaxSeeds], fold[rrl_pack::kMaxSeeds];
        for (int s = 0; s < S; ++s) {
            const QsArgs& a = blocks[s] = block_of(args + s, gates ? gates + s : nullptr);
            score[s] = a.n * a.P;                              // n x ceil(k / 128) workgroups, as in the solo kernel
            fold[s] = grid_for(a.n);                           // one thread per env
        }
        rrl_pack::Launch l = rrl_pack::place(S, score);     // the score kernel's placement, and in ix2 / i0 the fold kernel's
        const rrl_pack::Launch f = rrl_pack::place(S, fold);
        l.ix2 = f.ix;
        l.i0 = f.grid;
        plan = rrl_pack::publish(key, blocks, l, st);
        if (!plan) return rrl_pack::store_error();
    }
    static bool lds_set = false;
    const int rc = grant_lds(qsample_score_pack_kernel, kLdsBytes, lds_set);
    if (rc != RRL_OK) return rc;
    hipLaunchKernelGGL(qsample_score_pack_kernel, dim3((unsigned)plan->grid), dim3(kThreads), kLdsBytes, st,
                       (const QsArgs*)plan->dev, plan->ix);
    const int rs = check_launch();
    if (rs != RRL_OK) return rs;
    hipLaunchKernelGGL(qsample_fold_pack_kernel, dim3((unsigned)plan->i0), dim3(kBlock), 0, st, (const QsArgs*)plan->dev,
                       plan->ix2);
    return check_launch();
}

}  // extern "C"
