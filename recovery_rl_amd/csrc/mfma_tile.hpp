// mfma_tile.hpp -- the exact-f32 MFMA tile of a 4 -> 256 relu -> 256 relu -> out stack, shared by the acting and evaluation
// kernels (sqrl_kernels.hip, qsample_kernels.hip, eval_kernels.hip): activations in LDS at stride 260, W2 streamed from L2 in
// MFMA fragment order (rrl_w2_pack), v_mfma_f32_16x16x4_f32 with k ascending, 8 waves with 2 column tiles each.  The
// primitives at the top (f32x4, mfma, opaque, reluf, reduce16) also serve plan_kernels.hip and the ensemble trainers.
//
// Everything here is forced inline: a kernel that takes a helper from this header compiles to the instructions it had with a
// copy of its own (profiles/shared_tile_fingerprint.txt).
#pragma once

#include <hip/hip_runtime.h>

namespace rrl_tile {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kH = 256, kTiles = kH / 16;
constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;
constexpr int kActStride = kH + 4;        // +4 floats: row r starts at bank 4r, ds_read_b128 conflict-free

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// Identity the optimiser cannot see through: address arithmetic derived from opaque(lane) is redone per phase instead of
// being hoisted out of the loop around the phases and kept live across the matrix loops (hoisted, the per-element addresses
// of the epilogues cost > 200 VGPRs in ens_train_big_kernels.hip's tile loop, > 100 in plan_kernels.hip's rollout loop)
__device__ __forceinline__ int opaque(int x) {
    asm volatile("" : "+v"(x));
    return x;
}
__device__ __forceinline__ float reluf(float x) { return x < 0.f ? 0.f : x; }   // NaN stays NaN (F.relu)
// exact IEEE division (plan_kernels.hip keeps a v_rcp_f32 one of its own)
__device__ __forceinline__ float sigmoidf(float z) { return 1.f / (1.f + expf(-z)); }

__device__ __forceinline__ float reduce16(float v) {   // sum over the 16 lanes that share lane / 16
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
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

// ---- the 64-row twin-head tile (4 -> 256 -> 256 -> 1, two heads) ----
constexpr int kRows = 64;                 // rows per pass: 4 row tiles, every wave owns 2 column tiles of all of them

// LDS carve-up (floats): the prefix every user of q_phase shares; a kernel's own regions start at kOffOwn
constexpr int kOffAct = 0;                                   // [64][260] activations of the current pass
constexpr int kOffXs = kOffAct + kRows * kActStride;         // [64][4] (obs, candidate)
constexpr int kOffQpart = kOffXs + kRows * 4;                // [2 heads][8 waves][64 rows] partial last-layer sums
constexpr int kOffOwn = kOffQpart + 2 * kWaves * kRows;

// The twin heads on the first MR row tiles of xs; leaves qpart[h][wave][row] (the output's pre-activation is b3 + the sum
// over the 8 waves, added by twin_q in wave order).  Ends with a barrier.  Args: W1, b1, W2p, b2, W3 (and b3) of both heads.
template <int MR, class Args>
__device__ __forceinline__ void q_phase(float* lds, const Args& a, int wave, int lane) {
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

// Row `row` of the pass behind q_phase: z[h] = b3[h] + the eight waves' partial sums in wave order, and q = max(sigmoid z0,
// sigmoid z1) as torch.max does (NaN propagates).  Returned by value, with the callers' own expressions: the form in which
// their kernels keep their instructions.  OffQpart: where qpart is, for a tile with a carve-up of its own (mfma_tile_f16x3.hpp).
struct TwinQ {
    float z[2], q;
};
template <class Args, int OffQpart = kOffQpart>
__device__ __forceinline__ TwinQ twin_q(const float* lds, const Args& a, int row) {
    TwinQ t;
    float q[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        float v = a.b3[h];
#pragma unroll
        for (int w = 0; w < kWaves; ++w) v += lds[OffQpart + (h * kWaves + w) * kRows + row];
        t.z[h] = v;
        q[h] = sigmoidf(v);
    }
    t.q = (q[0] > q[1] || q[0] != q[0]) ? q[0] : q[1];
    return t;
}

}  // namespace rrl_tile
