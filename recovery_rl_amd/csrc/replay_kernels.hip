// replay_kernels.hip -- device-resident replay buffers for gfx950 (MI355X).
//
// Replaces recovery_rl/replay_memory.py (python list of tuples + random.sample + np.stack +
// five host->device copies per batch) with a structure-of-arrays ring in HBM:
//   push           : n rows x 32 B, coalesced (lane i -> slot pos+i), one launch
//   sample+gather  : ONE workgroup draws B distinct slots (Philox + LDS all-pairs dedupe) and
//                    gathers the rows into five contiguous batch tensors -- 16 KB moved for
//                    B=256; latency-bound by design (DESIGN.md "replay")
//   stratified     : per-64-slot positive counts maintained by push; the sampler scans the
//                    count table in LDS and touches 64 rewards per drawn row instead of the
//                    reference's O(capacity) argwhere per call (replay_memory.py:58-66)
#include <hip/hip_runtime.h>

#include "replay_draw.hpp"
#include "pack.hpp"
#include "rrl_host.hpp"

namespace {

using rrl_host::check_launch;
using rrl_host::grid_for;
using rrl_host::kBlock;

constexpr int kTile = 1024;   // rows per workgroup in the masked push
using rrl_replay::advance_ring;

struct Rows {
    const float2* s;
    const float2* a;
    const float* r;
    const float2* s2;
    const float* m;
};

__device__ __forceinline__ void store_row(const rrl_replay_t& rb, int64_t slot, int64_t size,
                                          const Rows& in, int64_t i) {
    rrl_replay::store_values(rb, slot, rrl_replay::was_positive(rb, slot, size), in.s[i], in.a[i], in.r[i], in.s2[i], in.m[i]);
}

__global__ __launch_bounds__(kBlock) void push_kernel(rrl_replay_t rb, int64_t n, Rows in) {
    const int64_t pos = rb.state[0], size = rb.state[1];
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride)
        store_row(rb, rrl_replay::ring_slot(rb, pos, i), size, in, i);
    advance_ring(rb, pos, size, n);
}

// masked push, pass 1: valid rows per 1024-row tile
__global__ __launch_bounds__(kBlock) void mask_count_kernel(const uint8_t* valid, int64_t n,
                                                            int32_t* tile_cnt) {
    __shared__ int32_t wave_cnt[kBlock / 64];
    const int64_t base = int64_t(blockIdx.x) * kTile;
    int32_t c = 0;
    for (int k = 0; k < kTile / kBlock; ++k) {
        const int64_t i = base + k * kBlock + threadIdx.x;
        c += (i < n && valid[i]) ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t tot = 0;
        for (int w = 0; w < kBlock / 64; ++w) tot += wave_cnt[w];
        tile_cnt[blockIdx.x] = tot;
    }
}

// masked push, pass 2: rows keep their order; tile offsets come from the pass-1 counts
__global__ __launch_bounds__(kBlock) void push_masked_kernel(rrl_replay_t rb, int64_t n, Rows in,
                                                             const uint8_t* valid,
                                                             const int32_t* tile_cnt) {
    __shared__ int64_t red[kBlock];
    __shared__ int32_t wave_off[kBlock / 64];
    const int64_t pos = rb.state[0], size = rb.state[1];
    // exclusive offset of this tile and the grand total
    int64_t before = 0, total = 0;
    for (int j = threadIdx.x; j < int(gridDim.x); j += kBlock) {
        const int32_t c = tile_cnt[j];
        total += c;
        if (j < int(blockIdx.x)) before += c;
    }
    red[threadIdx.x] = before;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if (int(threadIdx.x) < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    before = red[0];
    __syncthreads();
    red[threadIdx.x] = total;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if (int(threadIdx.x) < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    total = red[0];
    __syncthreads();
    int64_t run = before;
    const int64_t base = int64_t(blockIdx.x) * kTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < kTile / kBlock; ++k) {
        const int64_t i = base + k * kBlock + threadIdx.x;
        const bool v = (i < n) && valid[i];
        const unsigned long long bal = __ballot(v);
        const int rank_in_wave = __popcll(bal & ((1ULL << lane) - 1ULL));
        if (lane == 0) wave_off[wave] = __popcll(bal);
        __syncthreads();
        int32_t woff = 0, tile_tot = 0;
        for (int w = 0; w < kBlock / 64; ++w) {
            const int32_t c = wave_off[w];
            if (w < wave) woff += c;
            tile_tot += c;
        }
        if (v) store_row(rb, rrl_replay::ring_slot(rb, pos, run + woff + rank_in_wave), size, in, i);
        run += tile_tot;
        __syncthreads();
    }
    advance_ring(rb, pos, size, total);
}

// the select half on its own (rrl_draw_select): the keys a draw would use `rows_ahead` pushed rows from now
__global__ __launch_bounds__(1024) void select_ahead_kernel(rrl_replay_t rb, int B, uint64_t seed, uint64_t counter,
                                                            const uint64_t* counter_dev, int table_mask, int64_t rows_ahead,
                                                            uint32_t* keys) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    select_ahead_body(rb, B, seed, counter, counter_dev, table_mask, rows_ahead, keys, smem);
}

__global__ __launch_bounds__(1024) void sample_group_kernel(DrawArgs a, DrawArgs b, NoiseArgs nz) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    sample_group_body(a, b, nz, blockIdx.x, smem);
}

// the same launch for S seeds (pack.hpp)
struct SamplePack {
    DrawArgs a, b;
    NoiseArgs nz;
};
__global__ __launch_bounds__(1024) void sample_pack_kernel(const SamplePack* __restrict__ packs, rrl_pack::Idx ix) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int s, block;
    if (!rrl_pack::locate(ix, blockIdx.x, s, block)) return;
    // a sampler workgroup copies its own draw, a noise workgroup the noise block, out of device memory
    // (pointers that come out of device memory are passed through the global address space: rrl_pack::to_global)
    auto glob = [](DrawArgs& d) __attribute__((always_inline)) {
        rrl_pack::globalize(d.rb);
        rrl_pack::to_global_all(d.counter_dev, d.out.s, d.out.a, d.out.r, d.out.s2, d.out.m, d.out.idx, d.out.xu, d.out.x2u, d.out.xpu);
    };
    if (block == 0) { DrawArgs d = packs[s].a; glob(d); draw_body(d, smem); return; }
    if (block == 1) { DrawArgs d = packs[s].b; glob(d); draw_body(d, smem); return; }
    NoiseArgs nz = packs[s].nz;
    rrl_pack::to_global_all(nz.counter_dev, nz.out);
    sample_group_body(packs[s].a, packs[s].b, nz, block, smem);
}

}  // namespace

// gfx950 has 160 KiB of LDS per CU; opt in (once per size) above the 64 KiB default
template <class K>
static bool grant_sample_lds(K kernel, size_t lds, size_t& granted) {
    if (lds > granted) {
        if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        granted = lds;
    }
    return true;
}

extern "C" {

int rrl_replay_push(const rrl_replay_t* rb, int64_t n, const float* s, const float* a,
                    const float* r, const float* s2, const float* m, const uint8_t* valid,
                    int32_t* scratch, void* stream) {
    if (!valid_rb(rb) || !s || !a || !r || !s2 || !m || n < 0) return RRL_EINVAL;
    if (rb->pinned < 0 || rb->pinned >= rb->cap || n > rb->cap - rb->pinned) return RRL_ERANGE;
    if (n == 0) return RRL_OK;
    const Rows in{(const float2*)s, (const float2*)a, r, (const float2*)s2, m};
    hipStream_t st = (hipStream_t)stream;
    if (!valid) {
        hipLaunchKernelGGL(push_kernel, dim3(grid_for(n)), dim3(kBlock), 0, st, *rb, n, in);
        return check_launch();
    }
    if (!scratch) return RRL_EINVAL;
    const int64_t tiles = (n + kTile - 1) / kTile;
    if (tiles > 65535 * 16) return RRL_ERANGE;
    hipLaunchKernelGGL(mask_count_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, st, valid, n, scratch);
    hipLaunchKernelGGL(push_masked_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, st, *rb, n, in,
                       valid, (const int32_t*)scratch);
    return check_launch();
}

static int build_sample(const rrl_draw_t* first, const rrl_draw_t* second, long long noise_pairs, uint64_t noise_seed,
                        uint64_t noise_counter, uint64_t* noise_counter_dev, uint64_t noise_counter_inc, float* noise_out,
                        DrawArgs& a, DrawArgs& b, NoiseArgs& nz, int& threads, size_t& lds) {
    if (!first) return RRL_EINVAL;
    if (noise_pairs < 0 || noise_pairs >= (1LL << 32) || (noise_pairs > 0 && !noise_out)) return RRL_EINVAL;
    a = DrawArgs{};
    b = DrawArgs{};
    int ta = 0, tb = 0;
    size_t la = 0, lb = 0;
    int rc = draw_setup(*first, a, ta, la);
    if (rc != RRL_OK) return rc;
    if (second) {
        rc = draw_setup(*second, b, tb, lb);
        if (rc != RRL_OK) return rc;
    }
    // every member's results are independent of the workgroup size (integer prefix sums, per-index Philox draws), so
    // the launch takes the largest thread count a member would use on its own
    threads = ta > tb ? ta : tb;
    if (noise_pairs > 0 && threads < 256) threads = 256;
    lds = la > lb ? la : lb;
    nz = NoiseArgs{noise_pairs, noise_seed, noise_counter, noise_counter_dev, noise_counter_inc, noise_out, 0};
    return RRL_OK;
}

int rrl_sample_multi(const rrl_draw_t* first, const rrl_draw_t* second, long long noise_pairs, uint64_t noise_seed,
                     uint64_t noise_counter, uint64_t* noise_counter_dev, uint64_t noise_counter_inc, float* noise_out,
                     void* stream) {
    DrawArgs a, b;
    NoiseArgs nz;
    int threads;
    size_t lds;
    const int rc = build_sample(first, second, noise_pairs, noise_seed, noise_counter, noise_counter_dev, noise_counter_inc,
                                noise_out, a, b, nz, threads, lds);
    if (rc != RRL_OK) return rc;
    static size_t granted = 64 * 1024;
    if (!grant_sample_lds(sample_group_kernel, lds, granted)) return RRL_ERANGE;
    noise_blocks(nz, threads);
    hipLaunchKernelGGL(sample_group_kernel, dim3(2 + nz.blocks), dim3(threads), lds, (hipStream_t)stream, a, b, nz);
    return check_launch();
}

int rrl_draw_select(const rrl_draw_ahead_t* sel, void* stream) {
    if (!sel || !sel->draw || !sel->keys || sel->rows_ahead < 0 || sel->draw->stratified != RRL_DRAW_UNIFORM) return RRL_EINVAL;
    DrawArgs a{};
    int threads;
    size_t lds;
    const int rc = draw_setup(*sel->draw, a, threads, lds);
    if (rc != RRL_OK) return rc;
    hipLaunchKernelGGL(select_ahead_kernel, dim3(1), dim3(threads), lds, (hipStream_t)stream, a.rb, a.B, a.seed, a.counter,
                       a.counter_dev, a.table_mask, sel->rows_ahead, sel->keys);
    return check_launch();
}

static void key_draw(rrl_pack::Key& key, const rrl_draw_t* d) {
    key.pod(d != nullptr);
    if (d) {
        key.pod(*d);
        if (d->rb) key.pod(*d->rb);          // capacity / pinned rows / flags belong to the launch
    }
}

int rrl_sample_multi_packed(int S, const rrl_sample_args_t* args, void* stream) {
    if (S <= 0 || S > rrl_pack::kMaxSeeds || !args) return RRL_EINVAL;
    // one seed: the packed launch IS the solo launch (argument block in the kernel arguments, no plan)
    if (S == 1)
        return rrl_sample_multi(args[0].first, args[0].second, args[0].noise_pairs, args[0].noise_seed, args[0].noise_counter,
                                args[0].noise_counter_dev, args[0].noise_counter_inc, args[0].noise_out, stream);
    rrl_pack::Key key(rrl_pack::Site::ReplayDraw, S);
    for (int s = 0; s < S; ++s) {
        key_draw(key, args[s].first);
        key_draw(key, args[s].second);
        key.pod(args[s].noise_pairs); key.pod(args[s].noise_seed); key.pod(args[s].noise_counter);
        key.pod(args[s].noise_counter_dev); key.pod(args[s].noise_counter_inc); key.pod(args[s].noise_out);
    }
    hipStream_t st = (hipStream_t)stream;
    const rrl_pack::Plan* plan = rrl_pack::lookup(key);
    if (!plan) {
        std::vector<SamplePack> packs(S);
        int threads = 0;
        size_t lds = 0;
        for (int s = 0; s < S; ++s) {
            const rrl_sample_args_t& g = args[s];
            int t;
            size_t l;
            const int rc = build_sample(g.first, g.second, g.noise_pairs, g.noise_seed, g.noise_counter, g.noise_counter_dev,
                                        g.noise_counter_inc, g.noise_out, packs[s].a, packs[s].b, packs[s].nz, t, l);
            if (rc != RRL_OK) return rc;
            threads = t > threads ? t : threads;
            lds = l > lds ? l : lds;
        }
        int count[rrl_pack::kMaxSeeds];
        for (int s = 0; s < S; ++s) {
            noise_blocks(packs[s].nz, threads);
            count[s] = 2 + packs[s].nz.blocks;
        }
        static size_t granted = 64 * 1024;
        if (!grant_sample_lds(sample_pack_kernel, lds, granted)) return RRL_ERANGE;
        rrl_pack::Launch l = rrl_pack::place(S, count);
        l.i0 = threads;
        l.z0 = lds;
        plan = rrl_pack::publish(key, packs, l, st);
        if (!plan) return rrl_pack::store_error();
    }
    hipLaunchKernelGGL(sample_pack_kernel, dim3(plan->grid), dim3(plan->i0), plan->z0, st,
                       (const SamplePack*)plan->dev, plan->ix);
    return check_launch();
}

}  // extern "C"
