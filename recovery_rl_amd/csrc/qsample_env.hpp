// qsample_env.hpp -- the body of the Q-sampling recovery acting call (rrl_qsample_act_t, rrl_qsample_gate_t): the gate, a
// workgroup's chunk of candidates (draws, score passes, the chunk's argmin), the fold over an env's partials, the descriptor
// checks and the host protocol of the solo and the packed entries.  Stated once for the kernels that differ only in the
// arithmetic of the score passes: qsample_kernels.hip (exact f32, the tile of mfma_tile.hpp) and qsample_f16x3_kernels.hip
// (layer 2 as three f16 products, mfma_tile_f16x3.hpp).  A kernel names its tile as a class:
//     kOffXs, kOffOwn                     where the pass's inputs [64][4] go, where the regions below may start (floats)
//     q_phase<MR>(lds, a, wave, lane)     the twin heads on the first MR row tiles of xs; ends with a barrier
//     twin_q(lds, a, row)                 z[2] and q of one row behind q_phase
//
// Everything on the device side is forced inline and the offsets are compile-time constants: qsample_kernels.hip compiles to
// the instructions it had with this text in the source itself (profiles/qsample_f16x3_fingerprint.txt).
#pragma once

#include <vector>

#include "mfma_tile.hpp"
#include "pack.hpp"
#include "rrl_device.hpp"
#include "rrl_host.hpp"

namespace rrl_qsample {

using namespace rrl_tile;

constexpr uint32_t kStreamQsample = RRL_STREAM_QSAMPLE;
constexpr int kMaxK = 1024;               // candidates per env
constexpr int kChunk = 128;               // candidates per workgroup
constexpr int kPartial = 4;               // floats of a workgroup's partial: key, index (int bits), candidate x, y

// LDS carve-up (floats), behind the tile's act / xs / qpart
template <class Tile>
struct Lds {
    static constexpr int kOffCand = Tile::kOffOwn;                      // [128][2] candidate actions of the chunk
    static constexpr int kOffQ = kOffCand + kChunk * 2;                 // [128] max(sigmoid z0, sigmoid z1)
    static constexpr int kLdsFloats = kOffQ + kChunk;
    static constexpr int kLdsBytes = kLdsFloats * 4;
    static_assert(kLdsBytes <= 80 * 1024, "two workgroups share a CU's LDS");
};

// The argument block of one learner: the kernel argument of the stand-alone kernels, one element of a packed plan
struct ArgBlock {
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
__device__ __forceinline__ bool gate_fired(const ArgBlock& a, long long e) {
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
template <int MR, class Tile>
__device__ __forceinline__ void score_pass(float* lds, const ArgBlock& a, long long env, int c0, int rows, int base, float ox,
                                           float oy, int tid, int wave, int lane) {
    using L = Lds<Tile>;
    if (tid < kRows) {
        const int r = base + tid;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};           // rows past the chunk: finite inputs, results never read
        if (r < rows) x = f32x4{ox, oy, lds[L::kOffCand + 2 * r], lds[L::kOffCand + 2 * r + 1]};
        *reinterpret_cast<f32x4*>(lds + Tile::kOffXs + tid * 4) = x;
    }
    __syncthreads();
    Tile::template q_phase<MR>(lds, a, wave, lane);
    if (tid < kRows && base + tid < rows) {
        const int r = base + tid;
        const TwinQ t = Tile::twin_q(lds, a, tid);
        lds[L::kOffQ + r] = t.q;
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
template <class Tile>
__device__ __forceinline__ void score_chunk(const ArgBlock& a, unsigned b, float* lds) {
    using L = Lds<Tile>;
    constexpr int kOffCand = L::kOffCand, kOffQ = L::kOffQ;
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
            case 1: score_pass<1, Tile>(lds, a, env, c0, rows, base, ox, oy, tid, wave, lane); break;
            case 2: score_pass<2, Tile>(lds, a, env, c0, rows, base, ox, oy, tid, wave, lane); break;
            case 3: score_pass<3, Tile>(lds, a, env, c0, rows, base, ox, oy, tid, wave, lane); break;
            default: score_pass<4, Tile>(lds, a, env, c0, rows, base, ox, oy, tid, wave, lane); break;
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

// The copied argument block's pointers as global ones (pack.hpp: to_global)
__device__ __forceinline__ void globalize(ArgBlock& a) {
    rrl_pack::to_global_all(a.obs, a.mask, a.lo, a.hi, a.W1, a.b1, a.W2p, a.b2, a.W3, a.b3, a.counter_dev, a.cand_in, a.scratch,
                            a.action, a.q, a.z, a.cand, a.pick, a.gz, a.g_task, a.g_task_out, a.g_rec_out);
}

// One thread per env (envs e0, e0 + stride, ...): with a gate in the launch, recovery_out[e], task_out[e] and the task action
// into action[e] of an env whose gate did not fire -- what rrl_recovery_select leaves; then the P partials of a gated env in
// ascending chunk order (strict <: the lowest index wins) -> action[e] (and pick[e]).  The thread of env 0 advances the tick:
// every reader of it ran in the score kernel before this one.
__device__ __forceinline__ void fold_envs(const ArgBlock& a, long long e0, long long stride) {
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

inline int chunks_of(int k) { return (k + kChunk - 1) / kChunk; }

// the checks of a descriptor, before any launch (rrl_hip.h)
inline int check_desc(const rrl_qsample_act_t* p) {
    if (!p || !p->obs || !p->lo || !p->hi || !p->W1 || !p->b1 || !p->W2p || !p->b2 || !p->W3 || !p->b3 || !p->scratch ||
        !p->action || p->n <= 0 || p->H != kH || p->d_obs != 2 || p->d_act != 2 || (reinterpret_cast<uintptr_t>(p->W2p) & 15))
        return RRL_EINVAL;
    if (p->k < 1 || p->k > kMaxK || (long long)p->n * p->k >= (1LL << 32)) return RRL_ERANGE;
    return RRL_OK;
}

// ... and of a gate given with it
inline int check_both(const rrl_qsample_act_t* p, const rrl_qsample_gate_t* g) {
    const int rc = check_desc(p);
    if (!g || rc == RRL_EINVAL) return rc;
    if (p->mask || !g->z || !g->task_action || !g->recovery_out || g->n_part < 1 || g->n_part > 4 || g->ld_task < 2 ||
        (g->ld_task & 1))
        return RRL_EINVAL;                  // an invalid field wins over a size out of range
    return rc;
}

inline ArgBlock block_of(const rrl_qsample_act_t* p, const rrl_qsample_gate_t* g) {
    ArgBlock a{p->k, p->n, chunks_of(p->k), p->obs, p->mask, p->lo, p->hi, p->W1, p->b1, p->W2p, p->b2, p->W3, p->b3,
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

// The fold kernels are arithmetic-free and exist once, in qsample_kernels.hip: their launchers for both kernel families.
// launch_fold: one argument block on grid_for(n) workgroups; launch_fold_pack: a packed plan's blocks on plan.i0 workgroups
// placed by plan.ix2.
int launch_fold(const ArgBlock& a, hipStream_t st);
int launch_fold_pack(const rrl_pack::Plan& plan, hipStream_t st);

// The stand-alone entry (g == nullptr: the mask form): score(block, workgroups, stream) is the kernel family's score launcher;
// the fold kernel follows it on the same argument block
template <class Score>
int solo_entry(const rrl_qsample_act_t* p, const rrl_qsample_gate_t* g, void* stream, Score&& score) {
    const int rc = check_both(p, g);
    if (rc != RRL_OK) return rc;
    const ArgBlock a = block_of(p, g);
    hipStream_t st = (hipStream_t)stream;
    const int rs = score(a, (unsigned)((long long)a.n * a.P), st);
    if (rs != RRL_OK) return rs;
    return launch_fold(a, st);
}

// The packed entry (pack.hpp's host protocol) at `site`: score is the family's solo score launcher (S == 1),
// score_pack(plan, stream) its packed one
template <class Score, class ScorePack>
int packed_entry(rrl_pack::Site site, int S, const rrl_qsample_act_t* args, const rrl_qsample_gate_t* gates, void* stream,
                 Score&& score, ScorePack&& score_pack) {
    if (S <= 0 || S > rrl_pack::kMaxSeeds || !args) return RRL_EINVAL;
    for (int s = 0; s < S; ++s) {               // every seed is checked before anything is stored or launched
        const int rc = check_both(args + s, gates ? gates + s : nullptr);
        if (rc != RRL_OK) return rc;
    }
    // one seed: the packed launch IS the solo launch (argument block in the kernel arguments, no plan)
    if (S == 1) return solo_entry(args, gates, stream, score);
    for (int s = 0; s < S; ++s)                 // the grid of any mapping fits an int
        if ((long long)args[s].n * chunks_of(args[s].k) > INT32_MAX / rrl_pack::kMaxSeeds) return RRL_ERANGE;
    rrl_pack::Key key(site, S);
    key.pod(int(gates != nullptr));
    key.add(args, sizeof(rrl_qsample_act_t) * S);
    if (gates) key.add(gates, sizeof(rrl_qsample_gate_t) * S);
    hipStream_t st = (hipStream_t)stream;
    const rrl_pack::Plan* plan = rrl_pack::lookup(key);
    if (!plan) {
        std::vector<ArgBlock> blocks(S);
        int scores[rrl_pack::kMaxSeeds], fold[rrl_pack::kMaxSeeds];
        for (int s = 0; s < S; ++s) {
            const ArgBlock& a = blocks[s] = block_of(args + s, gates ? gates + s : nullptr);
            scores[s] = a.n * a.P;                             // n x ceil(k / 128) workgroups, as in the solo kernel
            fold[s] = rrl_host::grid_for(a.n);                 // one thread per env
        }
        rrl_pack::Launch l = rrl_pack::place(S, scores);    // the score kernel's placement, and in ix2 / i0 the fold kernel's
        const rrl_pack::Launch f = rrl_pack::place(S, fold);
        l.ix2 = f.ix;
        l.i0 = f.grid;
        plan = rrl_pack::publish(key, blocks, l, st);
        if (!plan) return rrl_pack::store_error();
    }
    const int rs = score_pack(*plan, st);
    if (rs != RRL_OK) return rs;
    return launch_fold_pack(*plan, st);
}

}  // namespace rrl_qsample
