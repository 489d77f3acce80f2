// nav_kernels.hip -- batched Navigation1 / Navigation2 env kernels for gfx950 (MI355X).
//
// Structure-of-arrays state in HBM, every access unit-stride across the 64-lane wavefront; one, two or four
// consecutive envs per lane depending on the launch size (latency regime / one resident round / streaming).
// General layout (rrl_nav_step: the reference's arrays): 28 B read + 44 B written per env-step; compact layout
// (rrl_nav_step_compact: u16 status words, one observation array): 26 B + 30 B.  All arithmetic in registers
// (Philox + Box-Muller in f64); LDS only for the per-wave list of finished rows whose start states are drawn
// once per wave and pass.  Grid: <= 2048 workgroups of 256 threads, grid-stride.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "replay_device.hpp"
#include "rrl_device.hpp"
#include "rrl_host.hpp"
#include "step_push.hpp"

#pragma clang fp contract(off)

namespace {

using rrl_host::check_launch;
using rrl_host::grid_for;
using rrl_host::kBlock;

using rrl_env::NavEnv;
using rrl_env::Outcome;

// Resets of the bandwidth-regime kernels.  With a ~1.2 % termination rate per step, one to three of the 256 envs a wave
// steps per pass finish, and an inline reset sends the whole wave through the Philox + Box-Muller chain again for each k
// that has a finished lane (2.2 extra trips per pass).  Measured at 2^24 envs, all variants interleaved in one process
// (profiles/nav_step_probe.py; compact layout without reset_obs / general layout; no resets at all: 233 / 261 us):
//   inline per lane                                            268 / 276 us
//   once per wave and pass, handed back through LDS (below)     243 / 262 us   <- kept
//   deferred to the end of the wave, pos patched by scattered stores       267 / 353 us
//   once per workgroup and pass (two barriers)                  ~340 / 357 us
//   once per wave and TWO passes, the first parked in LDS (nav_hold_kernel, two envs per thread)   222 / 249 us
// Scattered small stores are what the deferred variant pays for: ~200 k of them per launch cost 35-50 us next to the
// streaming traffic (profiles/sparse_write_probe.hip: anything below a whole 64-byte granule is a read-modify-write).
// The reset draws of the rows a wave finished in this pass, evaluated once per wave and pass.  The finished
// rows of the wave's V x 64 envs are listed in LDS (slots from ballots), the first `total` lanes evaluate normal_at() for
// them in ONE trip (instead of one trip per k with any finished lane: 2.2 trips per pass at a 1.2 % termination rate), and
// the owners read the pair back and store it with their dense stores -- no scattered store anywhere.
template <int V>
__device__ __forceinline__ void wave_reset_draws(uint64_t seed, uint64_t ctr, const uint32_t (&row)[V],
                                                 const bool (&fin)[V], double (&z0)[V], double (&z1)[V], uint32_t* rows,
                                                 double2* draws) {
    const int lane = threadIdx.x & 63;
    const uint64_t below = (1ULL << lane) - 1ULL;
    int slot[V], total = 0;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const uint64_t bal = __ballot(fin[k]);
        slot[k] = total + __popcll(bal & below);
        total += __popcll(bal);
    }
    if (total == 0) return;
    if (total > 64) {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (fin[k]) rrl::normal_at(seed, row[k], rrl::kStreamReset, ctr, z0[k], z1[k]);
        return;
    }
#pragma unroll
    for (int k = 0; k < V; ++k)
        if (fin[k]) rows[slot[k]] = row[k];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < total) {
        double x, y;
        rrl::normal_at(seed, rows[lane], rrl::kStreamReset, ctr, x, y);
        draws[lane] = make_double2(x, y);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < V; ++k)
        if (fin[k]) {
            const double2 d = draws[slot[k]];
            z0[k] = d.x;
            z1[k] = d.y;
        }
    __builtin_amdgcn_wave_barrier();   // the lists are reused by the wave's next pass
}

// ---- the wide step kernels: two templates (V envs per thread; two envs per thread with HOLD parked passes) over a layout ----
// A thread steps a GROUP of V consecutive envs.  All loads of the group are issued before the first dependent f64 operation
// (V x the bytes in flight per thread), the accesses are vectors of up to 16 bytes where the layout allows, and a wave touches
// V KB of contiguous positions.  The per-env arithmetic is the scalar kernel's, call for call (NavEnv), so the results are
// bit-identical.  A layout owns its argument struct, the load and the two stores of a group (what a reset does not touch;
// position and per-env state), how the step count is read and the state word formed, and what a parked pass keeps of the state.

// N values of T as one aligned vector access (N sizeof(T) <= 16)
template <class T, int N>
struct alignas(sizeof(T) * N) Vec {
    T v[N];
};
template <class T, int N>
__device__ __forceinline__ Vec<T, N>& vec_at(T* base, int64_t idx) { return reinterpret_cast<Vec<T, N>*>(base)[idx]; }
template <class T, int N>
__device__ __forceinline__ const Vec<T, N>& vec_at(const T* base, int64_t idx) { return reinterpret_cast<const Vec<T, N>*>(base)[idx]; }

// per-thread inputs of a group; t = the step count (arrays layout) or the status word (status layout)
template <int V>
struct GroupIn {
    double2 p[V], e[V];
    float ax[V], ay[V];
    uint32_t t[V];
};

// what a group's step leaves besides the positions.  state = the step count or the status word after the step; the four mask
// words (arrays layout) hold one byte per env, so that the V masks of an array go out as one store
template <int V>
struct GroupOut {
    float2 nobs[V];
    float rew[V];
    uint32_t state[V];
    uint32_t dn = 0, cons = 0, succ = 0, epd = 0;
};

// pos, action pairs and noise of whole group q, in that order around `state` (the layout's own load)
template <int V, bool EXT_NOISE, class ARGS, class STATE>
__device__ __forceinline__ void load_whole(const ARGS& a, int64_t q, GroupIn<V>& in, STATE&& state) {
    static_assert(V % 2 == 0, "whole groups are pairs of envs");
#pragma unroll
    for (int k = 0; k < V; ++k) in.p[k] = a.pos[q * V + k];
    Vec<float2, 2> act[V / 2];
#pragma unroll
    for (int j = 0; j < V / 2; ++j) act[j] = vec_at<float2, 2>(a.action, q * (V / 2) + j);
    state();
    if constexpr (EXT_NOISE) {
#pragma unroll
        for (int k = 0; k < V; ++k) in.e[k] = a.noise[q * V + k];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
        in.ax[k] = act[k / 2].v[k % 2].x;
        in.ay[k] = act[k / 2].v[k % 2].y;
    }
}

template <int V>
__device__ __forceinline__ void store_obs_pairs(float2* arr, int64_t q, const float2 (&o)[V]) {
#pragma unroll
    for (int j = 0; j < V / 2; ++j) vec_at<float2, 2>(arr, q * (V / 2) + j) = Vec<float2, 2>{{o[2 * j], o[2 * j + 1]}};
}

// Arrays layout (rrl_nav_step: the reference's arrays): four u8 masks, an i32 step count of which all 32 bits are kept, two
// observation arrays.  Whole groups only: the host sends n % V == 0 and the alignment of V-wide accesses.
struct ArraysLayout {
    using Args = StepArgs;
    static constexpr bool kRagged = false;
    template <int V, bool EXT_NOISE>
    static __device__ __forceinline__ void load(const Args& a, int64_t q, int, GroupIn<V>& in) {
        load_whole<V, EXT_NOISE>(a, q, in, [&] {
            const Vec<int32_t, V> tv = vec_at<int32_t, V>(a.t, q);
#pragma unroll
            for (int k = 0; k < V; ++k) in.t[k] = uint32_t(tv.v[k]);
        });
    }
    static __device__ __forceinline__ uint32_t steps(uint32_t t) { return t; }
    template <int V>
    static __device__ __forceinline__ void note(GroupOut<V>& out, int k, const Outcome& o, uint32_t ti, bool epd, bool fin) {
        out.dn |= uint32_t(o.done) << (8 * k);
        out.cons |= uint32_t(o.constraint) << (8 * k);
        out.succ |= uint32_t(o.success) << (8 * k);
        out.epd |= uint32_t(epd) << (8 * k);
        out.state[k] = fin ? 0u : ti;
    }
    template <int V>
    static __device__ __forceinline__ void store_step(const Args& a, int64_t q, int, const GroupOut<V>& out) {
        using Mask = std::conditional_t<V == 4, uint32_t, uint16_t>;
        store_obs_pairs<V>(a.next_obs, q, out.nobs);
        Vec<float, V> rew;
#pragma unroll
        for (int k = 0; k < V; ++k) rew.v[k] = out.rew[k];
        vec_at<float, V>(a.reward, q) = rew;
        reinterpret_cast<Mask*>(a.done)[q] = Mask(out.dn);
        reinterpret_cast<Mask*>(a.constraint)[q] = Mask(out.cons);
        reinterpret_cast<Mask*>(a.success)[q] = Mask(out.succ);
        if (a.ep_done) reinterpret_cast<Mask*>(a.ep_done)[q] = Mask(out.epd);
    }
    static __device__ __forceinline__ void store_reset(const Args&, int64_t, double2) {}      // obs goes out densely, below
    template <int V>
    static __device__ __forceinline__ void store_state(const Args& a, int64_t q, int, const double2 (&p)[V],
                                                       const uint32_t (&state)[V]) {
        float2 obs[V];
        Vec<int32_t, V> tv;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            a.pos[q * V + k] = p[k];
            obs[k] = make_float2(float(p[k].x), float(p[k].y));
            tv.v[k] = int32_t(state[k]);
        }
        if (a.obs) store_obs_pairs<V>(a.obs, q, obs);
        vec_at<int32_t, V>(a.t, q) = tv;
    }
    struct Parked {                  // of a pass of two envs per thread: both step counts
        int32_t t[2][kBlock];
        __device__ __forceinline__ void park(int tid, const uint32_t (&state)[2]) {
            t[0][tid] = int32_t(state[0]);
            t[1][tid] = int32_t(state[1]);
        }
        __device__ __forceinline__ void unpark(int tid, uint32_t (&state)[2]) const {
            state[0] = uint32_t(t[0][tid]);
            state[1] = uint32_t(t[1][tid]);
        }
    };
};

// ---- compact form (rrl_nav_step_compact): 56 B moved per env-step instead of 72 ----
// The general entry keeps the reference's separate arrays (four u8 masks, an i32 step count, two f32 observations).
// Here the step count and the four flags share one u16 status word per env (read for the count, rewritten), and the
// post-reset observation -- equal to next_obs wherever the episode goes on -- is written only for the rows whose
// episode ended.  Every access of a whole group is a vector (16 bytes; 8 or 4 for the status words); a last partial
// group goes through scalar accesses.  Per-env arithmetic = the general kernel's, call for call.
struct CompactArgs {
    int64_t n;
    double2* pos;
    const float2* action;
    const double2* noise;
    uint64_t seed, counter;
    uint64_t* counter_dev;
    uint64_t counter_inc;
    float2* next_obs;
    float2* reset_obs;
    float* reward;
    uint16_t* status;
    int32_t horizon, auto_reset;
};

// Status layout: `have` of the group's V envs exist (the last group may be ragged; V = 1 is always "ragged": scalar accesses)
struct StatusLayout {
    using Args = CompactArgs;
    static constexpr bool kRagged = true;
    template <int V, bool EXT_NOISE>
    static __device__ __forceinline__ void load(const Args& a, int64_t q, int have, GroupIn<V>& in) {
        if constexpr (V > 1) {
            if (have == V) {
                load_whole<V, EXT_NOISE>(a, q, in, [&] {
                    const Vec<uint32_t, V / 2> sv = vec_at<uint32_t, V / 2>(reinterpret_cast<const uint32_t*>(a.status), q);
#pragma unroll
                    for (int k = 0; k < V; ++k) in.t[k] = k % 2 ? sv.v[k / 2] >> 16 : sv.v[k / 2] & 0xffffu;
                });
                return;
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int64_t i = q * V + (k < have ? k : 0);
            in.p[k] = a.pos[i];
            const float2 ak = a.action[i];
            in.ax[k] = ak.x;
            in.ay[k] = ak.y;
            in.t[k] = a.status[i];
            if constexpr (EXT_NOISE) in.e[k] = a.noise[i];
        }
    }
    static __device__ __forceinline__ uint32_t steps(uint32_t st) { return st & RRL_STATUS_STEPS; }
    template <int V>
    static __device__ __forceinline__ void note(GroupOut<V>& out, int k, const Outcome& o, uint32_t ti, bool epd, bool fin) {
        if (ti > RRL_STATUS_STEPS) ti = RRL_STATUS_STEPS;
        out.state[k] = (fin ? 0u : ti) | (o.done ? RRL_STATUS_DONE : 0u) | (o.constraint ? RRL_STATUS_CONSTRAINT : 0u) |
                       (o.success ? RRL_STATUS_SUCCESS : 0u) | (epd ? RRL_STATUS_EP_DONE : 0u);
    }
    template <int V>
    static __device__ __forceinline__ void store_step(const Args& a, int64_t q, int have, const GroupOut<V>& out) {
        if constexpr (V > 1) {
            if (have == V) {
                store_obs_pairs<V>(a.next_obs, q, out.nobs);
                Vec<float, V> rew;
#pragma unroll
                for (int k = 0; k < V; ++k) rew.v[k] = out.rew[k];
                vec_at<float, V>(a.reward, q) = rew;
                return;
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (k < have) {
                a.next_obs[q * V + k] = out.nobs[k];
                a.reward[q * V + k] = out.rew[k];
            }
    }
    static __device__ __forceinline__ void store_reset(const Args& a, int64_t i, double2 p) {
        if (a.reset_obs) a.reset_obs[i] = make_float2(float(p.x), float(p.y));
    }
    template <int V>
    static __device__ __forceinline__ void store_state(const Args& a, int64_t q, int have, const double2 (&p)[V],
                                                       const uint32_t (&state)[V]) {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (k < have) a.pos[q * V + k] = p[k];
        if constexpr (V > 1) {
            if (have == V) {
                Vec<uint32_t, V / 2> sv;
#pragma unroll
                for (int j = 0; j < V / 2; ++j) sv.v[j] = state[2 * j] | (state[2 * j + 1] << 16);
                vec_at<uint32_t, V / 2>(reinterpret_cast<uint32_t*>(a.status), q) = sv;
                return;
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (k < have) a.status[q * V + k] = uint16_t(state[k]);
    }
    struct Parked {                  // of a pass of two envs per thread: both status words
        uint32_t st[kBlock];
        __device__ __forceinline__ void park(int tid, const uint32_t (&state)[2]) { st[tid] = state[0] | (state[1] << 16); }
        __device__ __forceinline__ void unpark(int tid, uint32_t (&state)[2]) const {
            state[0] = st[tid] & 0xffffu;
            state[1] = st[tid] >> 16;
        }
    };
};

// The groups of a launch: nq groups of V envs, dealt to the grid pass by pass.  Uniform trip count (the reset lists need
// whole waves): idle lanes shadow the last group and store nothing.
template <int V, bool RAGGED>
struct Groups {
    int64_t n, nq, stride, n_pass, q_first;
    __device__ __forceinline__ explicit Groups(int64_t n_)
        : n(n_), nq((n_ + V - 1) / V), stride(int64_t(gridDim.x) * kBlock), n_pass((nq + stride - 1) / stride),
          q_first(int64_t(blockIdx.x) * kBlock + threadIdx.x) {}
    __device__ __forceinline__ bool live(int64_t pass) const { return pass * stride + q_first < nq; }
    __device__ __forceinline__ int64_t group(int64_t pass) const {
        const int64_t q = pass * stride + q_first;
        return q < nq ? q : nq - 1;
    }
    __device__ __forceinline__ int have(int64_t q) const { return RAGGED ? int(n - q * V < V ? n - q * V : V) : V; }
};

// One step of group q's envs: what is stored in `out`, the next positions in p; returns the finished rows that take a reset (bit k)
template <int KIND, bool EXT_NOISE, class L, int V>
__device__ __forceinline__ uint32_t step_group(const typename L::Args& a, uint64_t ctr, int64_t q, int have, bool live,
                                               GroupOut<V>& out, double2 (&p)[V]) {
    GroupIn<V> in;
    L::template load<V, EXT_NOISE>(a, q, have, in);
    uint32_t finbits = 0;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const uint32_t row = uint32_t(q * V + k);
        Outcome o;
        if constexpr (EXT_NOISE) o = NavEnv<KIND>::step(in.p[k], double(in.ax[k]), double(in.ay[k]), in.e[k].x, in.e[k].y);
        else o = NavEnv<KIND>::step(a.seed, row, ctr, in.p[k], make_float2(in.ax[k], in.ay[k]));
        const uint32_t ti = L::steps(in.t[k]) + 1u;
        const bool epd = o.done | (int32_t(ti) == a.horizon);
        const bool fin = live & (k < have) & epd & (a.auto_reset != 0);
        out.nobs[k] = make_float2(float(o.x), float(o.y));
        out.rew[k] = o.reward;
        L::template note<V>(out, k, o, ti, epd, fin);
        finbits |= uint32_t(fin) << k;
        p[k] = make_double2(o.x, o.y);
    }
    return finbits;
}

// V envs per thread, the reset draws once per wave and pass.  Arrays layout: V = 4 at 2^19 <= n < 2^22 (measured: 34.9 ->
// 27.1 us at 2^20, slower below 2^18; a single round of 4 waves per SIMD covers 2^20 envs, beyond that the two-env kernel
// below wins).  Status layout: 4 in the same range, 1 when the launch is latency-bound (a short dependent chain per thread
// matters more than wide accesses; resets inline).  (Requesting the next pass's inputs before the f64 chain of the current
// one -- software pipelining -- measured 257.5 vs 258.0 us at 2^24 envs: not kept.)
// This build (profiles/kernel_resources.py): V = 4 takes 112 - 133 VGPRs in the arrays layout and 121 - 133 in the status
// layout, three or four waves per SIMD (four with caller-given noise, three with the draw), 5 KB of LDS; V = 1 takes 49 - 50.
template <int KIND, bool EXT_NOISE, class L, int V>
__global__ __launch_bounds__(kBlock) void nav_wide_kernel(typename L::Args a) {
    __shared__ uint32_t wave_rows[V > 1 ? kBlock / 64 : 1][64];
    __shared__ double2 wave_draws[V > 1 ? kBlock / 64 : 1][64];
    const uint64_t ctr = rrl::effective_counter(a.counter, a.counter_dev);
    const Groups<V, L::kRagged> g(a.n);
    for (int64_t pass = 0; pass < g.n_pass; ++pass) {
        const bool live = g.live(pass);
        const int64_t q = g.group(pass);
        const int have = g.have(q);
        GroupOut<V> out;
        double2 p[V];
        const uint32_t finbits = step_group<KIND, EXT_NOISE, L, V>(a, ctr, q, have, live, out, p);
        bool fin[V];
        uint32_t row[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            fin[k] = (finbits >> k) & 1u;
            row[k] = uint32_t(q * V + k);
        }
        double w0[V], w1[V];
        if constexpr (V > 1) {
            wave_reset_draws<V>(a.seed, ctr, row, fin, w0, w1, wave_rows[threadIdx.x >> 6], wave_draws[threadIdx.x >> 6]);
        }
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (fin[k]) {
                if constexpr (V == 1) p[k] = NavEnv<KIND>::reset(a.seed, row[k], ctr);
                else p[k] = NavEnv<KIND>::reset(w0[k], w1[k]);
                L::store_reset(a, q * V + k, p[k]);
            }
        if (!live) continue;
        L::template store_step<V>(a, q, have, out);
        L::template store_state<V>(a, q, have, p, out.state);
    }
    rrl::advance_counter(a.counter_dev, a.counter_inc);
}

// Streaming variant (n >= 2^22): two envs per thread, and HOLD passes share ONE reset draw.  A pass stores what a reset does
// not touch (next_obs, reward; the arrays layout's four masks) at once and parks its positions, its state (step counts or
// status words) and finished flags in LDS (40 - 44 B per thread and pass); after HOLD passes the wave draws the start states of
// all the rows it finished in them in one trip through normal_at(), applies them to the parked positions and stores positions
// and state densely.  At a 1.2 % termination rate that is ~1 trip per 64 x 2 x HOLD envs instead of 0.79 per 128.  The passes
// of a group run in a loop that is NOT unrolled: the register footprint stays that of one pass (holding them in registers
// let the compiler interleave them: 118 VGPRs, no gain).  Two rather than four envs per thread at this size: fewer registers,
// more waves per SIMD, and no SGPR-spill traffic.
// This build: HOLD = 2 takes 79 - 83 VGPRs in the arrays layout and 89 - 91 in the status layout, five waves per SIMD either
// way (four envs per thread: three or four), and 27 / 25 KB of LDS per workgroup.
template <class L>
struct HeldPass {
    double2 p[2][kBlock];
    typename L::Parked s;
    uint32_t fin[kBlock];      // bit k: row k finished and takes a reset
};

template <int KIND, bool EXT_NOISE, class L, int HOLD>
__global__ __launch_bounds__(kBlock) void nav_hold_kernel(typename L::Args a) {
    constexpr int V = 2;
    __shared__ HeldPass<L> held[HOLD];
    __shared__ uint32_t wave_rows[kBlock / 64][64];
    __shared__ double2 wave_draws[kBlock / 64][64];
    const int tid = threadIdx.x;
    const uint64_t ctr = rrl::effective_counter(a.counter, a.counter_dev);
    const Groups<V, L::kRagged> g(a.n);
    for (int64_t pass0 = 0; pass0 < g.n_pass; pass0 += HOLD) {
        const int n_here = int(g.n_pass - pass0 < HOLD ? g.n_pass - pass0 : HOLD);      // wave-uniform
#pragma unroll 1
        for (int h = 0; h < n_here; ++h) {
            const bool live = g.live(pass0 + h);
            const int64_t q = g.group(pass0 + h);
            const int have = g.have(q);
            GroupOut<V> out;
            double2 p[V];
            held[h].fin[tid] = step_group<KIND, EXT_NOISE, L, V>(a, ctr, q, have, live, out, p);
#pragma unroll
            for (int k = 0; k < V; ++k) held[h].p[k][tid] = p[k];
            held[h].s.park(tid, out.state);
            if (live) L::template store_step<V>(a, q, have, out);
        }
        // one reset draw for the rows this wave finished in the group's passes (own LDS slots: no barrier needed)
        bool fin[HOLD * V];
        uint32_t row[HOLD * V];
#pragma unroll
        for (int h = 0; h < HOLD; ++h) {
            const uint32_t fb = h < n_here ? held[h].fin[tid] : 0u;
            const int64_t q = g.group(h < n_here ? pass0 + h : pass0);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                fin[h * V + k] = (fb >> k) & 1u;
                row[h * V + k] = uint32_t(q * V + k);
            }
        }
        double w0[HOLD * V], w1[HOLD * V];
        wave_reset_draws<HOLD * V>(a.seed, ctr, row, fin, w0, w1, wave_rows[tid >> 6], wave_draws[tid >> 6]);
#pragma unroll
        for (int h = 0; h < HOLD; ++h) {
            if (h >= n_here || !g.live(pass0 + h)) continue;
            const int64_t q = g.group(pass0 + h);
            double2 p[V];
            uint32_t state[V];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                p[k] = held[h].p[k][tid];
                if (fin[h * V + k]) {
                    p[k] = NavEnv<KIND>::reset(w0[h * V + k], w1[h * V + k]);
                    L::store_reset(a, q * V + k, p[k]);
                }
            }
            held[h].s.unpark(tid, state);
            L::template store_state<V>(a, q, g.have(q), p, state);
        }
    }
    rrl::advance_counter(a.counter_dev, a.counter_inc);
}

__global__ __launch_bounds__(kBlock) void nav_reset_kernel(int64_t n, double2* pos, float2* obs,
                                                           int32_t* t, const uint8_t* mask,
                                                           const double2* noise, uint64_t seed,
                                                           uint64_t counter,
                                                           const uint64_t* counter_dev) {
    const uint64_t ctr = rrl::effective_counter(counter, counter_dev);
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
        if (mask && !mask[i]) continue;
        double z0, z1;
        if (noise) {
            z0 = noise[i].x;
            z1 = noise[i].y;
        } else {
            rrl::normal_at(seed, uint32_t(i), rrl::kStreamReset, ctr, z0, z1);
        }
        const double2 p = NavEnv<0>::reset(z0, z1);       // one start state for both kinds
        pos[i] = p;
        if (t) t[i] = 0;
        if (obs) obs[i] = make_float2(float(p.x), float(p.y));
    }
}

// T open-loop steps per env with the state in registers; per step only the action (8 B) is
// read and the requested outputs are written.
template <int KIND>
__global__ __launch_bounds__(kBlock) void nav_rollout_kernel(int64_t n, int32_t T, double2* pos,
                                                             const float2* actions, uint64_t seed,
                                                             uint64_t counter,
                                                             const uint64_t* counter_dev,
                                                             float2* obs_seq, float* reward_seq,
                                                             uint8_t* constraint_seq,
                                                             uint8_t* done_seq) {
    const uint64_t ctr = rrl::effective_counter(counter, counter_dev);
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
        double2 p = pos[i];
        for (int32_t k = 0; k < T; ++k) {
            const int64_t o = int64_t(k) * n + i;
            const float2 act = actions[o];
            const Outcome out = NavEnv<KIND>::step(seed, uint32_t(i), ctr + uint64_t(k), p, act);
            if (obs_seq) obs_seq[o] = make_float2(float(out.x), float(out.y));
            if (reward_seq) reward_seq[o] = out.reward;
            if (constraint_seq) constraint_seq[o] = uint8_t(out.constraint);
            if (done_seq) done_seq[o] = uint8_t(out.done);
            p = make_double2(out.x, out.y);
        }
        pos[i] = p;
    }
}


// ---- offline constraint data (env/navigation1.py:133-164, env/navigation2.py:133-243) ----
struct OfflinePlan {
    int64_t n_roll, n0, n1;
};

inline OfflinePlan offline_plan(int env_kind, int64_t num) {
    OfflinePlan p{0, 0, 0};
    if (env_kind == RRL_ENV_NAV1) {
        p.n_roll = num / 10;
    } else {
        p.n0 = num / 10 / 3;
        p.n1 = num / 10 / 4;
        p.n_roll = p.n0 + 4 * p.n1;
    }
    return p;
}

__device__ __forceinline__ void offline_uniform2(uint64_t seed, uint32_t row, uint64_t k,
                                                 uint32_t hi, double& u0, double& u1) {
    const rrl::Bits128 b = rrl::philox_at(seed, row, rrl::kStreamOffline, k | (uint64_t(hi) << 32));
    u0 = rrl::unit_open(b.lo);
    u1 = rrl::unit_open(b.hi);
}

// Simulates rollout `i`; when WRITE, stores its rows starting at row `base`. Returns its length.
template <int KIND, bool WRITE>
__device__ __forceinline__ int offline_rollout(int64_t i, int64_t n0, int64_t n1, uint64_t seed,
                                               int64_t base, float2* s, float2* a, float* c,
                                               float2* s2, float* m) {
    const uint32_t row = uint32_t(i);
    double u0, u1, v0, v1, x, y;
    offline_uniform2(seed, row, 0, 0, u0, u1);
    offline_uniform2(seed, row, 1, 0, v0, v1);
    int phase = 0;
    if constexpr (KIND == 0) {
        x = -80.0 + 130.0 * u1;
        y = (u0 < 0.5) ? (-5.0 + 3.0 * v0) : (2.0 + 3.0 * v0);
    } else {
        phase = (i < n0) ? 0 : 1 + int((i - n0) / (n1 > 0 ? n1 : 1));
        if (phase == 0) {
            x = -40.0 + 50.0 * u0;
            y = -25.0 + 50.0 * u1;
            for (uint32_t r = 0; NavEnv<KIND>::in_constraint(x, y); ++r) {
                double q0, q1;
                offline_uniform2(seed, row, 0, 1 + r, q0, q1);
                x = -40.0 + 50.0 * q0;
                y = -25.0 + 50.0 * q1;
            }
        } else if (phase == 1) {
            x = -35.0 + 5.0 * u0;
            y = -12.0 + 24.0 * u1;
        } else if (phase == 2) {
            x = -20.0 + 5.0 * u0;
            y = -12.0 + 24.0 * u1;
        } else if (phase == 3) {
            x = -30.0 + 10.0 * u0;
            y = 10.0 + 5.0 * u1;
        } else {
            x = -30.0 + 10.0 * u0;
            y = -15.0 + 5.0 * u1;
        }
    }
    int len = 0;
    for (int j = 0; j < 10; ++j) {
        double z0, z1, q0, q1, e0, e1;
        rrl::normal_at(seed, row, rrl::kStreamOffline, uint64_t(2 + 3 * j), z0, z1);
        offline_uniform2(seed, row, uint64_t(3 + 3 * j), 0, q0, q1);
        rrl::normal_at(seed, row, rrl::kStreamOffline, uint64_t(4 + 3 * j), e0, e1);
        double ax = rrl::clamp_unit(z0), ay = rrl::clamp_unit(z1);
        if (phase == 1) ax = 0.5 + 0.5 * q0;
        else if (phase == 2) ax = -1.0 + 0.5 * q0;
        else if (phase == 3) ay = -1.0 + 0.5 * q0;
        else if (phase == 4) ay = 0.5 + 0.5 * q0;
        const float axf = float(ax), ayf = float(ay);
        // the transition takes the float64 action, as the reference (navigation1.py:149-150)
        const Outcome out = NavEnv<KIND>::step(make_double2(x, y), ax, ay, e0, e1);
        const double nx = out.x, ny = out.y;
        const bool cons = out.constraint;
        if constexpr (WRITE) {
            const int64_t w = base + len;
            s[w] = make_float2(float(x), float(y));
            a[w] = make_float2(axf, ayf);
            c[w] = cons ? 1.0f : 0.0f;
            s2[w] = make_float2(float(nx), float(ny));
            m[w] = cons ? 0.0f : 1.0f;
        }
        ++len;
        x = nx;
        y = ny;
        if (cons) break;
    }
    return len;
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void offline_count_kernel(int64_t n_roll, int64_t n0,
                                                               int64_t n1, uint64_t seed,
                                                               int32_t* lens) {
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i < n_roll)
        lens[i] = offline_rollout<KIND, false>(i, n0, n1, seed, 0, nullptr, nullptr, nullptr,
                                               nullptr, nullptr);
}

// single workgroup: in-place exclusive scan of lens[0..n), total -> lens[n] and *count_dev
__global__ __launch_bounds__(1024) void exclusive_scan_kernel(int32_t* lens, int64_t n,
                                                              int64_t* count_dev) {
    __shared__ int32_t part[1024];
    __shared__ int32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const int32_t v = (i < n) ? lens[i] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int32_t add = (int(threadIdx.x) >= off) ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        const int32_t incl = part[threadIdx.x];
        const int32_t c0 = carry;
        if (i < n) lens[i] = c0 + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c0 + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        lens[n] = carry;
        if (count_dev) *count_dev = carry;
    }
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void offline_write_kernel(int64_t n_roll, int64_t n0,
                                                               int64_t n1, uint64_t seed,
                                                               const int32_t* offs, int64_t capacity,
                                                               float2* s, float2* a, float* c,
                                                               float2* s2, float* m) {
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n_roll) return;
    const int64_t base = offs[i];
    if (int64_t(offs[i + 1]) > capacity) return;  // caller sized the arrays too small: drop
    offline_rollout<KIND, true>(i, n0, n1, seed, base, s, a, c, s2, m);
}

__global__ void counter_add_kernel(uint64_t* ctr, uint64_t inc) { *ctr += inc; }

// (env_kind, noise given) -> compile-time constants: f(integral_constant<int, KIND>, bool_constant<EXT_NOISE>), for every
// launch site of a navigation kernel (the sites without a noise argument pass false)
template <class F>
auto with_nav_kind(int env_kind, bool ext_noise, F&& f) {
    using Nav1 = std::integral_constant<int, 0>;
    using Nav2 = std::integral_constant<int, 1>;
    if (env_kind == RRL_ENV_NAV1) return ext_noise ? f(Nav1{}, std::true_type{}) : f(Nav1{}, std::false_type{});
    return ext_noise ? f(Nav2{}, std::true_type{}) : f(Nav2{}, std::false_type{});
}

bool aligned(const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & (m - 1)) == 0; }

// Envs per thread of rrl_nav_step.  Bandwidth regime (n >= 2^22, n even): two, with two passes sharing one reset draw (the
// plain two-env kernel: 236 vs 225 us at 2^24).  Mid range (n >= 2^19, n % 4 == 0): four.  Both need the alignment of their
// vector accesses, which torch gives whole tensors; anything else: one.
int arrays_width(const StepArgs& a) {
    const auto masks = [&](uintptr_t m) {
        return aligned(a.done, m) && aligned(a.constraint, m) && aligned(a.success, m) && aligned(a.ep_done, m);
    };
    const bool obs16 = aligned(a.action, 16) && aligned(a.next_obs, 16) && aligned(a.obs, 16);
    if (a.n >= (1 << 22) && (a.n & 1) == 0 && obs16 && aligned(a.reward, 8) && aligned(a.t, 8) && masks(2)) return 2;
    if (a.n >= (1 << 19) && (a.n & 3) == 0 && obs16 && aligned(a.reward, 16) && aligned(a.t, 16) && masks(4)) return 4;
    return 1;
}

// Envs per thread of rrl_nav_step_compact, measured at 2^24 envs in one process (profiles/nav_step_probe.py): without resets
// 1 and 2 run at 192 us, 4 at 220 us (236 SGPR-spill reads per pass); with resets 241 / 231 / 236 us -- the once-per-wave
// reset draw batches 64 V envs, and at V = 1 every finished lane costs its wave a second chain.  Below 2^22 envs four per
// thread: 2^20 envs are then ONE round of 4 waves per SIMD (24.5 us; two per thread 34 us).  Below 2^18 one: the latency
// regime, a short dependent chain per thread, resets inline.
int status_width(int64_t n) { return n < (1 << 18) ? 1 : (n < (1 << 22) ? 4 : 2); }

}  // namespace

thread_local int rrl_host::last_hip_error = 0;

extern "C" {

int rrl_pack_clear(void) { return rrl_pack::clear(); }

// 2: pos_cnt carries a second count level (RRL_POS_CNT_LEN); 3: rrl_replay_t.pinned; 4: RRL_DRAW_DEMO_SHARE;
// 5: the positional forms of the fused env step (plain and with the recovery gate) are gone: rrl_step_push_t is its one form;
// 6: likewise the stack backward and the optimiser step (rrl_*_bwd_t, rrl_adam_seg_t); 7: the replay draws and the policy-head
// forwards (rrl_draw_t through rrl_sample_multi, rrl_policy_head_t through rrl_policy_heads_fwd_multi)
int rrl_abi_version(void) { return 8; }

int rrl_last_hip_error(void) { return rrl_host::last_hip_error; }

int rrl_counter_add(uint64_t* ctr, uint64_t inc, void* stream) {
    if (!ctr) return RRL_EINVAL;
    hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, ctr, inc);
    return check_launch();
}

int rrl_nav_step(int env_kind, int64_t n, double* pos, const float* action, const double* noise,
                 uint64_t seed, uint64_t counter, uint64_t* counter_dev, uint64_t counter_inc,
                 float* next_obs,
                 float* obs, float* reward, uint8_t* done, uint8_t* constraint, uint8_t* success,
                 uint8_t* ep_done, int32_t* t, int32_t horizon, int auto_reset, void* stream) {
    if (env_kind != RRL_ENV_NAV1 && env_kind != RRL_ENV_NAV2) return RRL_EINVAL;
    if (n < 0 || n > 0xffffffffLL) return RRL_ERANGE;
    if (!pos || !action || !next_obs || !reward || !done || !constraint || !success || !t)
        return RRL_EINVAL;
    if (n == 0) return RRL_OK;
    StepArgs a{n, (double2*)pos, (const float2*)action, (const double2*)noise, seed, counter,
               counter_dev, counter_inc, (float2*)next_obs, (float2*)obs, reward, done, constraint, success,
               ep_done, t, horizon, auto_reset};
    const int v = arrays_width(a);
    // (four per thread: 2048 workgroups, 8 per CU, although fewer are resident: measured 262 vs 272 us for one full round)
    const dim3 grid(grid_for(n / v)), block(kBlock);
    hipStream_t st = (hipStream_t)stream;
    with_nav_kind(env_kind, noise != nullptr, [&](auto kind, auto ext) {
        constexpr int K = decltype(kind)::value;
        constexpr bool E = decltype(ext)::value;
        if (v == 2) hipLaunchKernelGGL((nav_hold_kernel<K, E, ArraysLayout, 2>), grid, block, 0, st, a);
        else if (v == 4) hipLaunchKernelGGL((nav_wide_kernel<K, E, ArraysLayout, 4>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((env_step_kernel<NavEnv<K>, E>), grid, block, 0, st, a);
    });
    return check_launch();
}

int rrl_nav_step_compact(int env_kind, int64_t n, double* pos, const float* action, const double* noise,
                         uint64_t seed, uint64_t counter, uint64_t* counter_dev, uint64_t counter_inc,
                         float* next_obs, float* reset_obs, float* reward, uint16_t* status, int32_t horizon,
                         int auto_reset, void* stream) {
    if (env_kind != RRL_ENV_NAV1 && env_kind != RRL_ENV_NAV2) return RRL_EINVAL;
    if (n < 0 || n > 0xffffffffLL || horizon < 1 || horizon > int32_t(RRL_STATUS_STEPS)) return RRL_ERANGE;
    if (!pos || !action || !next_obs || !reward || !status) return RRL_EINVAL;
    if (!aligned(pos, 16) || !aligned(action, 16) || !aligned(noise, 16) || !aligned(next_obs, 16) ||
        !aligned(reset_obs, 8) || !aligned(reward, 16) || !aligned(status, 8))
        return RRL_EINVAL;
    if (n == 0) return RRL_OK;
    CompactArgs a{n, (double2*)pos, (const float2*)action, (const double2*)noise, seed, counter, counter_dev,
                  counter_inc, (float2*)next_obs, (float2*)reset_obs, reward, status, horizon, auto_reset};
    const int v = status_width(n);
    const dim3 grid(grid_for((n + v - 1) / v)), block(kBlock);
    hipStream_t st = (hipStream_t)stream;
    with_nav_kind(env_kind, noise != nullptr, [&](auto kind, auto ext) {
        constexpr int K = decltype(kind)::value;
        constexpr bool E = decltype(ext)::value;
        // passes that share one reset draw (parked in LDS): 1 -> 236 us, 2 -> 225 us, 3 -> 228 us, 4 -> 240 us at 2^24
        // envs (the larger groups cost registers in the apply phase)
        if (v == 2) hipLaunchKernelGGL((nav_hold_kernel<K, E, StatusLayout, 2>), grid, block, 0, st, a);
        else if (v == 4) hipLaunchKernelGGL((nav_wide_kernel<K, E, StatusLayout, 4>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((nav_wide_kernel<K, E, StatusLayout, 1>), grid, block, 0, st, a);
    });
    return check_launch();
}

int rrl_nav_reset(int env_kind, int64_t n, double* pos, float* obs, int32_t* t,
                  const uint8_t* mask, const double* noise, uint64_t seed, uint64_t counter,
                  const uint64_t* counter_dev, void* stream) {
    if (env_kind != RRL_ENV_NAV1 && env_kind != RRL_ENV_NAV2) return RRL_EINVAL;
    if (n < 0 || n > 0xffffffffLL) return RRL_ERANGE;
    if (!pos) return RRL_EINVAL;
    if (n == 0) return RRL_OK;
    hipLaunchKernelGGL(nav_reset_kernel, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream,
                       n, (double2*)pos, (float2*)obs, t, mask, (const double2*)noise, seed,
                       counter, counter_dev);
    return check_launch();
}

int rrl_nav_rollout(int env_kind, int64_t n, int32_t T, double* pos, const float* actions,
                    uint64_t seed, uint64_t counter, const uint64_t* counter_dev, float* obs_seq,
                    float* reward_seq, uint8_t* constraint_seq, uint8_t* done_seq, void* stream) {
    if (env_kind != RRL_ENV_NAV1 && env_kind != RRL_ENV_NAV2) return RRL_EINVAL;
    if (n < 0 || n > 0xffffffffLL || T < 0) return RRL_ERANGE;
    if (!pos || !actions) return RRL_EINVAL;
    if (n == 0 || T == 0) return RRL_OK;
    with_nav_kind(env_kind, false, [&](auto kind, auto) {
        hipLaunchKernelGGL((nav_rollout_kernel<decltype(kind)::value>), dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream,
                           n, T, (double2*)pos, (const float2*)actions, seed, counter, counter_dev, (float2*)obs_seq,
                           reward_seq, constraint_seq, done_seq);
    });
    return check_launch();
}

int64_t rrl_nav_offline_rollouts(int env_kind, int64_t num_transitions) {
    if (env_kind != RRL_ENV_NAV1 && env_kind != RRL_ENV_NAV2) return RRL_EINVAL;
    if (num_transitions < 0) return RRL_EINVAL;
    return offline_plan(env_kind, num_transitions).n_roll;
}

int rrl_nav_offline(int env_kind, int64_t num_transitions, uint64_t seed, float* s, float* a,
                    float* c, float* s2, float* m, int64_t capacity, int64_t* count_dev,
                    int32_t* scratch, void* stream) {
    if (env_kind != RRL_ENV_NAV1 && env_kind != RRL_ENV_NAV2) return RRL_EINVAL;
    if (num_transitions < 0 || !s || !a || !c || !s2 || !m || !scratch) return RRL_EINVAL;
    const OfflinePlan p = offline_plan(env_kind, num_transitions);
    if (p.n_roll > 0x7fffffffLL / 10) return RRL_ERANGE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((p.n_roll + kBlock - 1) / kBlock > 0 ? (p.n_roll + kBlock - 1) / kBlock : 1)),
        block(kBlock);
    with_nav_kind(env_kind, false, [&](auto kind, auto) {
        constexpr int K = decltype(kind)::value;
        hipLaunchKernelGGL((offline_count_kernel<K>), grid, block, 0, st, p.n_roll, p.n0, p.n1, seed, scratch);
        hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, st, scratch, p.n_roll, count_dev);
        hipLaunchKernelGGL((offline_write_kernel<K>), grid, block, 0, st, p.n_roll, p.n0, p.n1, seed,
                           scratch, capacity, (float2*)s, (float2*)a, c, (float2*)s2, m);
    });
    return check_launch();
}

static int nav_step_push_launch(int env_kind, const rrl_step::StepPushArgs& p, int64_t n, void* stream) {
    with_nav_kind(env_kind, false, [&](auto kind, auto) {
        rrl_step::launch<NavEnv<decltype(kind)::value>>(p, n, (hipStream_t)stream);
    });
    return check_launch();
}

int rrl_nav_step_push_x(int env_kind, const rrl_step_push_t* a, void* stream) {
    if (env_kind != RRL_ENV_NAV1 && env_kind != RRL_ENV_NAV2) return RRL_EINVAL;
    rrl_step::StepPushArgs p;
    const int rc = rrl_step::fill_args(p, a);
    if (rc != RRL_OK || a->n == 0) return rc;
    return nav_step_push_launch(env_kind, p, a->n, stream);
}

int rrl_nav_step_push_packed(int S, int env_kind, const rrl_step_push_t* a, void* stream) {
    if ((env_kind != RRL_ENV_NAV1 && env_kind != RRL_ENV_NAV2) || S <= 0 || S > rrl_pack::kMaxSeeds || !a) return RRL_EINVAL;
    // one seed: the packed launch IS the solo launch (argument block in the kernel arguments, no plan)
    if (S == 1) return rrl_nav_step_push_x(env_kind, &a[0], stream);
    rrl_pack::Key key(rrl_pack::Site::NavStep, S);
    key.pod(env_kind);
    return with_nav_kind(env_kind, false, [&](auto kind, auto) {
        return rrl_step::launch_packed<NavEnv<decltype(kind)::value>>(key, S, a, (hipStream_t)stream);
    });
}

}  // extern "C"
