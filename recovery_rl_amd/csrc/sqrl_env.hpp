// sqrl_env.hpp -- one env of SQRL's constraint-sampling acting pass (rrl_sqrl_act_t): candidates, scores, pick.  Stated once
// for the kernels that differ only in the arithmetic of the score passes: sqrl_kernels.hip (exact f32, the tile of
// mfma_tile.hpp) and sqrl_f16x3_kernels.hip (layer 2 as three f16 products).  A kernel names its tile as a class:
//     kOffXs, kOffOwn                     where the pass's inputs [64][4] go, where the regions below may start (floats)
//     q_phase<MR>(lds, a, wave, lane)     the twin heads on the first MR row tiles of xs; ends with a barrier
//     twin_q(lds, a, row)                 z[2] and q of one row behind q_phase
//
// Everything here is forced inline and the offsets are compile-time constants: sqrl_kernels.hip compiles to the instructions
// it had with this text in the source itself (profiles/sqrl_f16x3_fingerprint.txt).
#pragma once

#include <type_traits>
#include <vector>

#include "mfma_tile.hpp"
#include "rrl_device.hpp"
#include "rrl_host.hpp"
#include "pack.hpp"

namespace rrl_sqrl {

using namespace rrl_tile;
using rrl::psum;

constexpr uint32_t kStreamSqrl = RRL_STREAM_SQRL, kStreamSqrlPick = RRL_STREAM_SQRL_PICK;
constexpr int kMaxK = 128;                // candidates per env
constexpr float kLogSigMax = 2.f, kLogSigMin = -20.f, kEps = 1e-6f;   // model.py:14-16
constexpr float kHalfLog2Pi = 0.918938533204672742f;

// LDS carve-up (floats), behind the tile's act / xs / qpart
template <class Tile>
struct Lds {
    static constexpr int kOffCand = Tile::kOffOwn;                      // [128][2] candidate actions
    static constexpr int kOffLogp = kOffCand + kMaxK * 2;               // [128]
    static constexpr int kOffQ = kOffLogp + kMaxK;                      // [128] max(sigmoid z0, sigmoid z1)
    static constexpr int kOffW = kOffQ + kMaxK;                         // [128] doubles: the pick's weights
    static constexpr int kOffPick = kOffW + 2 * kMaxK;                  // 4 ints: {n_safe, argmin, -, -}, then 2 x u64 safe masks
    static constexpr int kLdsFloats = kOffPick + 8;
    static constexpr int kLdsBytes = kLdsFloats * 4;
    static_assert(kOffW % 2 == 0 && kOffPick % 2 == 0, "doubles and 64-bit masks need 8-byte alignment");
    static_assert(2 * kLdsBytes <= 160 * 1024, "two workgroups share a CU's LDS");
};

// The argument block of one learner: the kernel argument of the stand-alone kernels, one element of a packed plan
struct ArgBlock {
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
template <int MR, class Tile>
__device__ __forceinline__ void score_pass(float* lds, const ArgBlock& a, long long env, int base, float ox, float oy,
                                           int tid, int wave, int lane) {
    using L = Lds<Tile>;
    const int k = a.k;
    if (tid < kRows) {
        const int c = base + tid;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};           // rows past k: finite inputs, results never read
        if (c < k) x = f32x4{ox, oy, lds[L::kOffCand + 2 * c], lds[L::kOffCand + 2 * c + 1]};
        *reinterpret_cast<f32x4*>(lds + Tile::kOffXs + tid * 4) = x;
    }
    __syncthreads();
    Tile::template q_phase<MR>(lds, a, wave, lane);
    if (tid < kRows && base + tid < k) {
        const int c = base + tid;
        const TwinQ t = Tile::twin_q(lds, a, tid);
        lds[L::kOffQ + c] = t.q;
        if (a.q) a.q[env * k + c] = t.q;
        if (a.z) {
            a.z[env * k + c] = t.z[0];
            a.z[((long long)a.n + env) * k + c] = t.z[1];
        }
    }
    // xs and qpart are rewritten only behind the next pass's barriers
}

// One env of one learner: candidates, scores, pick.  The stand-alone and the packed kernel differ only in where `a` and `env`
// come from (and in how many workgroups share the learner's tick).
// NT = row tiles of 16 candidates (ceil(k / 16), 1..8): pass 0 takes min(NT, 4) of them, pass 1 the rest
template <int NT, class Tile>
__device__ __forceinline__ void sqrl_env(const ArgBlock& a, const long long env, float* lds) {
    using L = Lds<Tile>;
    constexpr int kOffCand = L::kOffCand, kOffLogp = L::kOffLogp, kOffQ = L::kOffQ, kOffW = L::kOffW, kOffPick = L::kOffPick;
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
    score_pass<MR0, Tile>(lds, a, env, 0, ox, oy, tid, wave, lane);
    if constexpr (MR1 > 0) score_pass<MR1, Tile>(lds, a, env, kRows, ox, oy, tid, wave, lane);

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

// the checks of one descriptor, before any launch (rrl_hip.h)
inline int check_desc(const rrl_sqrl_act_t* p) {
    if (!p || !p->obs || !p->head || !p->scale || !p->bias || !p->W1 || !p->b1 || !p->W2p || !p->b2 || !p->W3 || !p->b3 ||
        !p->action || p->n <= 0 || p->H != kH || p->d_obs != 2 || p->d_act != 2 || p->n_part < 1 || p->n_part > 4 ||
        (reinterpret_cast<uintptr_t>(p->W2p) & 15))
        return RRL_EINVAL;
    if (p->k < 1 || p->k > kMaxK || (long long)p->n * p->k >= (1LL << 32)) return RRL_ERANGE;
    return RRL_OK;
}

inline ArgBlock block_of(const rrl_sqrl_act_t* p) {
    return ArgBlock{p->k, p->n_part, p->n, p->part_stride, p->obs, p->head, p->scale, p->bias, p->W1, p->b1, p->W2p, p->b2,
                    p->W3, p->b3, p->eps_safe, p->seed, p->counter, p->counter_dev, p->counter_inc, p->eps_in, p->u_in,
                    p->action, p->q, p->logp, p->cand, p->z, p->pick, p->cstar, p->n_safe};
}

// f(std::integral_constant<int, NT>, args...) for NT = nt row tiles (1..8): NT is a template parameter of the kernels
template <class F, class... A>
int by_row_tiles(int nt, F&& f, A&&... args) {
    switch (nt) {
        case 1: return f(std::integral_constant<int, 1>{}, args...);
        case 2: return f(std::integral_constant<int, 2>{}, args...);
        case 3: return f(std::integral_constant<int, 3>{}, args...);
        case 4: return f(std::integral_constant<int, 4>{}, args...);
        case 5: return f(std::integral_constant<int, 5>{}, args...);
        case 6: return f(std::integral_constant<int, 6>{}, args...);
        case 7: return f(std::integral_constant<int, 7>{}, args...);
        default: return f(std::integral_constant<int, 8>{}, args...);
    }
}

// The stand-alone entry: launch(NT, block, n, stream) is the kernel family's launcher
template <class Launch>
int solo_entry(const rrl_sqrl_act_t* p, void* stream, Launch&& launch) {
    const int rc = check_desc(p);
    if (rc != RRL_OK) return rc;
    return by_row_tiles((p->k + 15) / 16, launch, block_of(p), p->n, (hipStream_t)stream);
}

// The packed entry (pack.hpp's host protocol) at `site`: solo(args, stream) is the family's stand-alone entry,
// launch_pack(NT, plan, stream) its packed launcher
template <class Solo, class LaunchPack>
int packed_entry(rrl_pack::Site site, int S, const rrl_sqrl_act_t* args, void* stream, Solo&& solo, LaunchPack&& launch_pack) {
    if (S <= 0 || S > rrl_pack::kMaxSeeds || !args) return RRL_EINVAL;
    for (int s = 0; s < S; ++s) {               // every seed's descriptor is checked before anything is stored or launched
        const int rc = check_desc(args + s);
        if (rc != RRL_OK) return rc;
    }
    for (int s = 1; s < S; ++s)                 // NT is a template parameter of the kernel: one k per call
        if (args[s].k != args[0].k) return RRL_EINVAL;
    // one seed: the packed launch IS the solo launch (argument block in the kernel arguments, no plan)
    if (S == 1) return solo(args, stream);
    rrl_pack::Key key(site, S);
    key.add(args, sizeof(rrl_sqrl_act_t) * S);
    hipStream_t st = (hipStream_t)stream;
    const rrl_pack::Plan* plan = rrl_pack::lookup(key);
    if (!plan) {
        std::vector<ArgBlock> blocks(S);
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
    return by_row_tiles(plan->i0, launch_pack, *plan, st);
}

}  // namespace rrl_sqrl
