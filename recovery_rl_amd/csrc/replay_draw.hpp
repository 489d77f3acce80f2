// replay_draw.hpp -- the replay draws' device code (index selection, gather, the per-mode bodies and the noise fill) and
// their launch parameters, shared by the draw launches (replay_kernels.hip) and by the forward
// launch that takes the draws along as rider workgroups (mlp_fwd_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "replay_device.hpp"
#include "rrl_device.hpp"
#include "rrl_host.hpp"

namespace {

using rrl_replay::kChunk;

// ---- sampling -------------------------------------------------------------------------------
struct BatchOut {
    float2* s;
    float2* a;
    float* r;
    float2* s2;
    float* m;
    int64_t* idx;
    float4* xu;    // optional [B,4] rows (s, a): the critics' input, written by the gather itself
    float4* x2u;   // optional [B,4] rows (s', *, *): columns 2..3 are left for the policy head kernel
    float4* xpu;   // optional [B,4] rows (s,  *, *)
};

// B distinct draws per group from [0, population): each slot draws independently; a slot loses
// a round when an accepted slot, or a lower-numbered pending slot of its group, holds the same
// value, and redraws with the round number bumped (uniform over ordered subsets by symmetry).
// cand / acc live in LDS.  Returns false if the round cap is hit.
// Implementation: per round an LDS hash table maps value -> lowest claiming tag (accepted lanes claim
// with tag 0, pending lane i with tag i + 1) through 64-bit atomicMin on (value << 32 | tag); the table
// content that matters (minimum tag per value) does not depend on insertion order, so the outcome is the
// same as the sequential all-pairs rule of the CPU checker.  O(B) work per round instead of O(B^2).
// `group` (0/1) keeps the two populations of the stratified sampler apart.  key[i] = value | accepted << 31.
__device__ __forceinline__ uint32_t hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// `whole`: this lane's class is taken whole (as many rows requested as it has -- what the clamped stratified draw does to
// a starved class): its lanes get the ranks 0, 1, ... in lane order instead of drawing.  (Drawing n distinct values out
// of n by rejection needs O(n) rounds: 50 us for 69 positives in the Maze loop.)
__device__ __forceinline__ bool draw_distinct(int i, int B, int group, uint64_t population, uint64_t seed,
                                              uint32_t stream, uint64_t ctr, int row, uint32_t* key,
                                              unsigned long long* table, int table_mask, bool whole = false) {
    const unsigned long long kEmpty = ~0ULL;
    const bool active = i < B;
    bool mine = !active;  // inactive lanes count as settled
    uint32_t v = 0;
    if (active && whole) {
        mine = true;
        v = uint32_t(row);
        key[i] = v | 0x80000000u;
    }
    for (uint32_t round = 0; round <= 4096; ++round) {
        for (int e = threadIdx.x; e <= table_mask; e += blockDim.x) table[e] = kEmpty;
        if (active && !mine) {
            const rrl::Bits128 b = rrl::philox_at(seed, uint32_t(row), stream, (ctr << 12) | round);
            v = uint32_t(__umul64hi(b.lo, population));
        }
        __syncthreads();
        const uint32_t hv = v | (uint32_t(group) << 31);            // value tagged with its population
        if (active) {                                                // claim: accepted lanes with tag 0
            const unsigned long long pack = ((unsigned long long)hv << 32) | (mine ? 0u : uint32_t(i + 1));
            uint32_t h = hash32(hv) & table_mask;
            for (;;) {
                unsigned long long cur = table[h];
                if (cur == kEmpty) {
                    cur = atomicCAS(&table[h], kEmpty, pack);
                    if (cur == kEmpty) break;
                }
                if (uint32_t(cur >> 32) == hv) {
                    atomicMin(&table[h], pack);
                    break;
                }
                h = (h + 1) & table_mask;
            }
        }
        __syncthreads();
        if (active && !mine) {
            uint32_t h = hash32(hv) & table_mask;
            while (uint32_t(table[h] >> 32) != hv) h = (h + 1) & table_mask;
            if (uint32_t(table[h]) == uint32_t(i + 1)) {             // lowest claimant of this value: accepted
                mine = true;
                key[i] = v | 0x80000000u;
            }
        }
        if (__syncthreads_count(!mine) == 0) return true;
    }
    return false;
}

__device__ __forceinline__ void gather_row(const rrl_replay_t& rb, int64_t slot, int i,
                                           const BatchOut& out) {
    const float2 s = ((const float2*)rb.s)[slot], a = ((const float2*)rb.a)[slot];
    const float2 s2 = ((const float2*)rb.s2)[slot];
    out.s[i] = s;
    out.a[i] = a;
    out.r[i] = rb.r[slot];
    out.s2[i] = s2;
    out.m[i] = rb.m[slot];
    if (out.idx) out.idx[i] = slot;
    if (out.xu) out.xu[i] = make_float4(s.x, s.y, a.x, a.y);
    if (out.x2u) ((float2*)out.x2u)[2 * i] = s2;
    if (out.xpu) ((float2*)out.xpu)[2 * i] = s;
}

// The uniform draw in two halves.  SELECT: B distinct keys for a ring of `size` rows at tick `ctr`, left in LDS (`key`);
// 0, or the error code the whole draw flags in rb.state[3] (1: B > size, 2: round cap).  GATHER: the rows of the keys.
// The whole draw (mode 1) runs both in one workgroup; the draw-ahead form (rrl_draw_ahead_t) runs the select half one env step
// early -- `size` is then the size AFTER that step's rows, min(cap, size now + rows_ahead) -- and the gather half after it.
__device__ __forceinline__ int select_keys(int B, int64_t size, uint64_t seed, uint64_t ctr, uint32_t* key,
                                           unsigned long long* table, int table_mask) {
    const int i = threadIdx.x;
    return draw_distinct(i, B, 0, uint64_t(size), seed, rrl::kStreamSample, ctr, i, key, table, table_mask) ? 0 : 2;
}

__device__ __forceinline__ void sample_gather_body(const rrl_replay_t& rb, int B, uint64_t seed, uint64_t counter,
                                                   uint64_t* counter_dev, uint64_t counter_inc, int table_mask,
                                                   const BatchOut& out, char* smem) {
    unsigned long long* table = (unsigned long long*)smem;      // [table_mask + 1]
    uint32_t* key = (uint32_t*)(table + table_mask + 1);
    const int64_t size = rb.state[1];
    const uint64_t ctr = rrl::effective_counter(counter, counter_dev);      // requested with the size, not behind its test
    if (int64_t(B) > size) {  // random.sample would raise ValueError
        if (threadIdx.x == 0) rb.state[3] = 1;
        return;
    }
    rrl::advance_counter_single(counter_dev, counter_inc, counter, ctr);        // one workgroup per draw
    const int i = threadIdx.x;
    if (select_keys(B, size, seed, ctr, key, table, table_mask)) {
        if (threadIdx.x == 0) rb.state[3] = 2;
        return;
    }
    if (i < B) gather_row(rb, int64_t(key[i] & 0x7fffffffu), i, out);
}

// Keys selected ahead live in a device buffer of B + RRL_AHEAD_META words: the keys, then the tick and the ring size they were
// drawn for (two words each) and the select half's error code.  The select half changes nothing else: the tick advances and
// the error flag is raised where the whole draw would do it, by the gather half one step later -- between the two
// every observable word (tick, rb.state) reads as in a run without draw-ahead.
constexpr int kAheadMeta = RRL_AHEAD_META;

__device__ __forceinline__ void select_ahead_body(const rrl_replay_t& rb, int B, uint64_t seed, uint64_t counter,
                                                  const uint64_t* counter_dev, int table_mask, int64_t rows_ahead,
                                                  uint32_t* keys_out, char* smem) {
    unsigned long long* table = (unsigned long long*)smem;      // [table_mask + 1]
    uint32_t* key = (uint32_t*)(table + table_mask + 1);
    const int64_t size = min(rb.cap, rb.state[1] + rows_ahead);
    const uint64_t ctr = rrl::effective_counter(counter, counter_dev);
    const int i = threadIdx.x;
    const int err = int64_t(B) > size ? 1 : select_keys(B, size, seed, ctr, key, table, table_mask);
    if (!err && i < B) keys_out[i] = key[i] & 0x7fffffffu;
    if (i == 0) {
        uint32_t* meta = keys_out + B;
        meta[0] = uint32_t(ctr); meta[1] = uint32_t(ctr >> 32);
        meta[2] = uint32_t(size); meta[3] = uint32_t(uint64_t(size) >> 32);
        meta[4] = uint32_t(err);
    }
}

// ... and the gather half for keys selected ahead: what sample_gather_body does around its selection, in its order.  Keys
// drawn for another tick or ring size (the host's validity rule was broken) are not used: error flag 4.
__device__ __forceinline__ void gather_ahead_body(const rrl_replay_t& rb, int B, uint64_t counter, uint64_t* counter_dev,
                                                  uint64_t counter_inc, const uint32_t* keys, const BatchOut& out) {
    const int64_t size = rb.state[1];
    const uint64_t ctr = rrl::effective_counter(counter, counter_dev);
    const int i = threadIdx.x;
    const uint32_t* meta = keys + B;
    const uint64_t for_ctr = uint64_t(meta[0]) | (uint64_t(meta[1]) << 32);
    const int64_t for_size = int64_t(uint64_t(meta[2]) | (uint64_t(meta[3]) << 32));
    const int err = int(meta[4]);
    const uint32_t k = keys[min(i, B - 1)];
    if (for_ctr != ctr || for_size != size) {
        if (i == 0) rb.state[3] = 4;
        return;
    }
    if (err == 1) {
        if (i == 0) rb.state[3] = 1;
        return;
    }
    rrl::advance_counter_single(counter_dev, counter_inc, counter, ctr);
    if (err) {
        if (i == 0) rb.state[3] = err;
        return;
    }
    if (i < B) gather_row(rb, int64_t(k), i, out);
}

// Stratified: lanes [0,n_pos) draw ranks among positives, lanes [n_pos,B) among negatives.
__device__ __forceinline__ void creplay_sample_gather_body(const rrl_replay_t& rb, int n_pos, int n_neg, int n_chunks,
                                                           uint64_t seed, uint64_t counter, uint64_t* counter_dev,
                                                           uint64_t counter_inc, int table_mask, const BatchOut& out,
                                                           char* smem) {
    const int B = n_pos + n_neg;
    unsigned long long* table = (unsigned long long*)smem;      // [table_mask + 1]
    uint32_t* key = (uint32_t*)(table + table_mask + 1);
    int32_t* sup = (int32_t*)(key + ((B + 3) & ~3));      // [n_super + 1] exclusive positive counts per super-chunk
    const int64_t size = rb.state[1];
    const int tid = threadIdx.x;
    // Second count level (one entry per 1024 slots, <= 2048 of them) -> exclusive scan in LDS.  (The first version
    // copied and scanned the whole first level -- 15 625 entries at 1e6 slots, 62 KB -- in this one workgroup: 27 us.)
    const int n_super = int(rrl_replay::count_supers(rb.cap));
    const int32_t* sup_cnt = rb.pos_cnt + rrl_replay::super_base(rb.cap);
    // wave 0: lane l owns entries 32 l .. 32 l + 31 (cap <= 2^21: at most 2048 entries), wave prefix by shuffles
    if (tid < 64) {
        constexpr int kOwn = 32;
        int32_t v[kOwn], run = 0;
        const bool vec = (reinterpret_cast<uintptr_t>(sup_cnt) & 15) == 0;
#pragma unroll
        for (int q = 0; q < kOwn / 4; ++q) {             // eight independent 16-byte loads per lane, in flight together
            const int c = kOwn * tid + 4 * q;
            if (vec && c + 3 < n_super) {
                const int4 t4 = *reinterpret_cast<const int4*>(sup_cnt + c);
                v[4 * q] = t4.x; v[4 * q + 1] = t4.y; v[4 * q + 2] = t4.z; v[4 * q + 3] = t4.w;
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) v[4 * q + u] = c + u < n_super ? sup_cnt[c + u] : 0;
            }
        }
#pragma unroll
        for (int u = 0; u < kOwn; ++u) run += v[u];
        int32_t incl = run;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t up = __shfl_up(incl, off, 64);
            if (tid >= off) incl += up;
        }
        int32_t acc = incl - run;                      // exclusive prefix of this lane's first entry
#pragma unroll
        for (int u = 0; u < kOwn; ++u) {
            const int c = kOwn * tid + u;
            if (c <= n_super) sup[c] = acc;
            acc += v[u];
        }
        if (kOwn * tid + kOwn == n_super) sup[n_super] = acc;     // total, when n_super is a multiple of kOwn
    }
    __syncthreads();
    const int64_t total_pos = sup[n_super];
    const int64_t total_neg = size - total_pos;
    if (int64_t(n_pos) > total_pos || int64_t(n_neg) > total_neg) {
        const bool feasible = int64_t(B) <= size && (rb.flags & RRL_REPLAY_CLAMP_STRATIFIED);
        if (!feasible) {
            if (tid == 0) rb.state[3] = 1;
            return;
        }
        // every row of the short class, the rest of the batch from the other one (uniform for all threads)
        if (int64_t(n_pos) > total_pos) n_pos = int(total_pos);
        else n_pos = B - int(total_neg);
        n_neg = B - n_pos;
    }
    const uint64_t ctr = rrl::effective_counter(counter, counter_dev);
    rrl::advance_counter_single(counter_dev, counter_inc, counter, ctr);
    const bool is_pos = tid < n_pos;
    const uint64_t population = uint64_t(is_pos ? total_pos : total_neg);
    const uint32_t stream = is_pos ? rrl::kStreamSample : rrl::kStreamSampleNeg;
    // lanes of the negative group are numbered from 0 within their group, like a separate call
    const int gi = is_pos ? tid : tid - n_pos;
    const bool class_whole = population == uint64_t(is_pos ? n_pos : n_neg);
    if (!draw_distinct(tid, B, is_pos ? 0 : 1, population, seed, stream, ctr, gi, key, table, table_mask, class_whole)) {
        if (tid == 0) rb.state[3] = 2;
        return;
    }
    if (tid >= B) return;
    // rank -> slot: binary search the super-chunk in LDS, walk its 64 first-level counts (16 independent 16-byte loads),
    // then scan the chunk's 64 rewards
    const int64_t k = int64_t(key[tid] & 0x7fffffffu);
    auto before_super = [&](int sc) -> int64_t {  // rows of my class in super-chunks [0, sc)
        const int64_t filled = min(size, int64_t(sc) * rrl_replay::kSuper);
        return is_pos ? int64_t(sup[sc]) : filled - int64_t(sup[sc]);
    };
    int sa = 0, sb = n_super;  // invariant: before_super(sa) <= k < before_super(sb)
    while (sb - sa > 1) {
        const int mid = (sa + sb) >> 1;
        if (before_super(mid) <= k) sa = mid; else sb = mid;
    }
    constexpr int kPer = rrl_replay::kSuper / kChunk;     // 16 chunks per super-chunk
    const int c_first = sa * kPer;
    int4 cv[kPer / 4];
    {
        const int4* src = reinterpret_cast<const int4*>(rb.pos_cnt + c_first);   // c_first % 4 == 0, table 16-byte aligned
        const bool all = c_first + kPer <= n_chunks && (reinterpret_cast<uintptr_t>(rb.pos_cnt) & 15) == 0;
#pragma unroll
        for (int q = 0; q < kPer / 4; ++q) {
            if (all) {
                cv[q] = src[q];
            } else {
                int t4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) t4[u] = c_first + 4 * q + u < n_chunks ? rb.pos_cnt[c_first + 4 * q + u] : 0;
                cv[q] = make_int4(t4[0], t4[1], t4[2], t4[3]);
            }
        }
    }
    // From here on everything is relative to the super-chunk / chunk and fits 32 bits (the 64-bit version of these two
    // 64-step walks was 20 of the kernel's 26 us: ~1300 emulated-int64 instructions per lane on a single CU).
    int32_t rem = int32_t(k - before_super(sa));                          // rank inside the super-chunk, < 1024
    const int64_t sup_lo = int64_t(c_first) * kChunk;
    const int32_t filled_sup = int32_t(min(int64_t(rrl_replay::kSuper), max(int64_t(0), size - sup_lo)));
    int32_t a_rel = -1;
#pragma unroll
    for (int q = 0; q < kPer / 4; ++q) {
        const int e4[4] = {cv[q].x, cv[q].y, cv[q].z, cv[q].w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int cu = 4 * q + u;
            const int32_t filled = min(max(filled_sup - cu * kChunk, 0), kChunk);      // filled slots of this chunk
            const int32_t mine = is_pos ? e4[u] : filled - e4[u];
            const bool take = (a_rel < 0) & (rem < mine);
            a_rel = take ? cu : a_rel;
            rem = a_rel < 0 ? rem - mine : rem;
        }
    }
    if (a_rel < 0) {          // the two count levels disagree
        rb.state[3] = 3;
        return;
    }
    const int a = c_first + a_rel;
    const int64_t c0 = int64_t(a) * kChunk;
    // the chunk's bit mask instead of its 64 rewards (256 B and a 64-step compare chain per row: 6 of the kernel's 19 us):
    // the rem-th set bit of the class's candidates, by popcounts of halves
    const int32_t filled_c = int32_t(min(int64_t(kChunk), max(int64_t(0), size - c0)));
    const unsigned long long pos_bits = rrl_replay::chunk_masks(rb)[a];
    const unsigned long long filled_bits = filled_c >= kChunk ? ~0ULL : ((1ULL << filled_c) - 1ULL);
    unsigned long long cand = is_pos ? (pos_bits & filled_bits) : (filled_bits & ~pos_bits);
    int32_t slot_rel = -1;
    if (rem < __popcll(cand)) {
        int32_t at = 0;
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) {
            const unsigned long long low = cand & ((1ULL << w) - 1ULL);
            const int32_t c = __popcll(low);
            const bool upper = rem >= c;
            rem -= upper ? c : 0;
            cand = upper ? (cand >> w) : low;
            at += upper ? w : 0;
        }
        slot_rel = at;
    }
    const int64_t slot = slot_rel < 0 ? int64_t(-1) : c0 + slot_rel;
    if (slot < 0) {  // count table out of sync with the rows: flag, never read out of bounds
        rb.state[3] = 3;
        return;
    }
    gather_row(rb, slot, tid, out);
}

// Demonstration-share draw (the lock-step loop's rule for the safety critic's batch, DESIGN "replay"): lanes [0, n_demo)
// draw distinct rows of the pinned range [0, pinned) -- the offline constraint demonstrations, experiment.py:278-286 --
// lanes [n_demo, B) distinct rows of the online range [pinned, size).  A range with too few rows gives all it has and
// the other one fills the batch.  Ranks ARE slots here (demo rank k = slot k, online rank k = slot pinned + k).
__device__ __forceinline__ void split_sample_gather_body(const rrl_replay_t& rb, int n_demo, int n_online, uint64_t seed,
                                                         uint64_t counter, uint64_t* counter_dev, uint64_t counter_inc,
                                                         int table_mask, const BatchOut& out, char* smem) {
    const int B = n_demo + n_online;
    unsigned long long* table = (unsigned long long*)smem;      // [table_mask + 1]
    uint32_t* key = (uint32_t*)(table + table_mask + 1);
    const int64_t size = rb.state[1];
    const int tid = threadIdx.x;
    if (int64_t(B) > size) {  // random.sample would raise ValueError
        if (tid == 0) rb.state[3] = 1;
        return;
    }
    const int64_t demo_total = min(rb.pinned, size), online_total = size - demo_total;
    if (int64_t(n_online) > online_total) { n_online = int(online_total); n_demo = B - n_online; }
    else if (int64_t(n_demo) > demo_total) { n_demo = int(demo_total); n_online = B - n_demo; }
    const uint64_t ctr = rrl::effective_counter(counter, counter_dev);
    rrl::advance_counter_single(counter_dev, counter_inc, counter, ctr);
    const bool is_demo = tid < n_demo;
    const uint64_t population = uint64_t(is_demo ? demo_total : online_total);
    const uint32_t stream = is_demo ? rrl::kStreamSample : rrl::kStreamSampleNeg;
    const int gi = is_demo ? tid : tid - n_demo;              // numbered from 0 within the group, like a separate call
    const bool whole = population == uint64_t(is_demo ? n_demo : n_online);
    if (!draw_distinct(tid, B, is_demo ? 0 : 1, population, seed, stream, ctr, gi, key, table, table_mask, whole)) {
        if (tid == 0) rb.state[3] = 2;
        return;
    }
    if (tid >= B) return;
    const int64_t k = int64_t(key[tid] & 0x7fffffffu);
    gather_row(rb, is_demo ? k : demo_total + k, tid, out);
}

// The two draws of one lock-step iteration (task buffer for the SAC update, safety buffer for the Q_risk update:
// experiment.py:397-416) and the iteration's policy noise do not depend on each other: one launch, workgroup 0 and 1
// are the samplers (one draw_body each; an absent member has mode 0), the remaining workgroups fill the noise buffer.
struct DrawArgs {
    rrl_replay_t rb;
    int mode;            // 0: none, 1: RRL_DRAW_UNIFORM, 2: RRL_DRAW_STRATIFIED, 3: RRL_DRAW_DEMO_SHARE (n_pos demo, n_neg online rows)
    int B, n_pos, n_neg, n_chunks, table_mask;
    uint64_t seed, counter;
    uint64_t* counter_dev;
    uint64_t counter_inc;
    BatchOut out;
};
struct NoiseArgs {
    long long n_pairs;
    uint64_t seed, counter;
    uint64_t* counter_dev;
    uint64_t counter_inc;
    float* out;
    int blocks;
};

__device__ __forceinline__ void draw_body(const DrawArgs& d, char* smem) {
    if (d.mode == 1)
        sample_gather_body(d.rb, d.B, d.seed, d.counter, d.counter_dev, d.counter_inc, d.table_mask, d.out, smem);
    else if (d.mode == 2)
        creplay_sample_gather_body(d.rb, d.n_pos, d.n_neg, d.n_chunks, d.seed, d.counter, d.counter_dev, d.counter_inc,
                                   d.table_mask, d.out, smem);
    else if (d.mode == 3)
        split_sample_gather_body(d.rb, d.n_pos, d.n_neg, d.seed, d.counter, d.counter_dev, d.counter_inc, d.table_mask,
                                 d.out, smem);
}

// N(0,1) pairs of Philox stream RRL_STREAM_NOISE (rrl_normal_fill), workgroup `block` of nz.blocks
__device__ __forceinline__ void noise_body(const NoiseArgs& nz, int block) {
    const uint64_t ctr = rrl::effective_counter(nz.counter, nz.counter_dev);
    const long long stride = (long long)nz.blocks * blockDim.x;
    for (long long i = (long long)block * blockDim.x + threadIdx.x; i < nz.n_pairs; i += stride) {
        double z0, z1;
        rrl::normal_at(nz.seed, uint32_t(i), rrl::kStreamNoise, ctr, z0, z1);
        reinterpret_cast<float2*>(nz.out)[i] = make_float2(float(z0), float(z1));
    }
    rrl::advance_counter_blocks(nz.counter_dev, nz.counter_inc, unsigned(nz.blocks));
}

__device__ __forceinline__ void sample_group_body(const DrawArgs& a, const DrawArgs& b, const NoiseArgs& nz, int block,
                                                  char* smem) {
    if (block == 0) { draw_body(a, smem); return; }
    if (block == 1) { draw_body(b, smem); return; }
    noise_body(nz, block - 2);
}

// ---- host side: launch parameters -------------------------------------------------------------------------------
inline bool valid_rb(const rrl_replay_t* rb) {
    return rb && rb->s && rb->a && rb->r && rb->s2 && rb->m && rb->state && rb->cap > 0;
}

// one draw's checks and launch parameters (threads, dynamic LDS): rrl_draw_t's contract (include/rrl_hip.h) in code
inline int draw_setup(const rrl_draw_t& d, DrawArgs& a, int& threads, size_t& lds) {
    const rrl_replay_t* rb = d.rb;
    if (!valid_rb(rb) || !d.s || !d.a || !d.r || !d.s2 || !d.m) return RRL_EINVAL;
    a.rb = *rb;
    a.seed = d.seed; a.counter = d.counter; a.counter_dev = d.counter_dev; a.counter_inc = d.counter_inc;
    a.out = BatchOut{(float2*)d.s, (float2*)d.a, d.r, (float2*)d.s2, d.m, d.idx_out, (float4*)d.xu, (float4*)d.x2u,
                     (float4*)d.xpu};
    const int B = d.n_pos + d.n_neg;
    if (d.n_pos < 0 || d.n_neg < 0 || B <= 0 || B > 1024) return RRL_ERANGE;
    a.B = B; a.n_pos = d.n_pos; a.n_neg = d.n_neg;
    int table_size = 64;
    while (table_size < 4 * B) table_size <<= 1;
    a.table_mask = table_size - 1;
    threads = ((B + 63) / 64) * 64;
    if (d.stratified == RRL_DRAW_UNIFORM || d.stratified == RRL_DRAW_DEMO_SHARE) {
        if (rb->cap >= (int64_t(1) << 31)) return RRL_ERANGE;
        if (d.stratified == RRL_DRAW_DEMO_SHARE && (rb->pinned < 0 || rb->pinned >= rb->cap)) return RRL_ERANGE;
        a.mode = d.stratified == RRL_DRAW_UNIFORM ? 1 : 3;
        a.n_chunks = 0;
        lds = size_t(table_size) * 8 + size_t(B) * 4 + 16;
        return RRL_OK;
    }
    if (d.stratified != RRL_DRAW_STRATIFIED) return RRL_EINVAL;
    if (!rb->pos_cnt) return RRL_EINVAL;
    if (rb->cap > (int64_t(1) << 21)) return RRL_ERANGE;
    a.mode = 2;
    a.n_chunks = int((rb->cap + kChunk - 1) / kChunk);
    if (threads < 64) threads = 64;
    lds = size_t(table_size) * 8 + size_t((B + 3) & ~3) * 4 + size_t(rrl_replay::count_supers(rb->cap) + 2) * 4 + 16;
    return RRL_OK;
}

inline void noise_blocks(NoiseArgs& nz, int threads) {
    if (nz.n_pairs > 0) {
        long long nb = (nz.n_pairs + threads - 1) / threads;
        nz.blocks = int(nb < 1 ? 1 : (nb > 1024 ? 1024 : nb));
    }
}

}  // namespace
