// mfma_tile_f16x3.hpp -- the 64-row twin-head tile of mfma_tile.hpp with layer 2 as three v_mfma_f32_16x16x32_f16 products of
// hi / lo f16 splits instead of v_mfma_f32_16x16x4_f32: the planner's F16X3 arithmetic (plan_kernels.hip: split16,
// layer_mma_k32, pack_layer_f16x3_k32_kernel), restated on the tile conventions of mfma_tile.hpp (2 column tiles per wave, MR
// row tiles, k ascending).  Shared by the acting kernels that score on it: sqrl_f16x3_kernels.hip and qsample_f16x3_kernels.hip.
//
// Precision (rrl_hip.h): layer 1 (K = 4) is one exact f32 MFMA per tile.  Its relu output v is kept as hi = f16(v),
// lo = f16(v - hi) in two f16 planes; W2 arrives split the same way (rrl_w2_pack_f16x3).  Layer 2 accumulates, per 32-wide
// k block in ascending order, hi*lo, hi*hi, lo*hi in f32; lo*lo (2^-22 of the product) is dropped.
//
// Everything here is forced inline: a kernel that takes the tile from this header compiles to the instructions it had with the
// text in its own source (profiles/qsample_f16x3_fingerprint.txt).
#pragma once

#include "mfma_tile.hpp"

namespace rrl_tile {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// The activations as two f16 planes (hi, lo) of [64][kHalfStride]: 132 words per row, so row r starts at bank 4r and the
// 16-byte fragment reads of a quarter-wave hit different banks (the planner's layout)
constexpr int kHalfStride = kH + 8;
constexpr int kPlaneHalves = kRows * kHalfStride;
constexpr int kActFloats = kPlaneHalves;          // 2 planes x 64 x 264 x 2 B = 67 584 B (the f32 tile: 66 560 B)

// v = hi + lo with hi = f16(v), lo = f16(v - hi), lo UNSCALED (f16 subnormals are not flushed by the CDNA4 f16 MFMA): the
// planner's split.  relu outputs are bounded below; above the f16 range they saturate; NaN compares false and stays NaN.
__device__ __forceinline__ void split16(float v, _Float16& hi, _Float16& lo) {
    v = v > 65504.f ? 65504.f : v;
    hi = (_Float16)v;
    lo = (_Float16)(v - (float)hi);
}

// Slot j (a float4 = 8 halves per lane) of this wave's two column tiles: W2h is [ct][2 jp + {0: hi, 1: lo}][lane]
__device__ __forceinline__ void load_h(f32x4 (&b)[2], const float* __restrict__ w2h, const int (&ct)[2], int j, int lane) {
#pragma unroll
    for (int c = 0; c < 2; ++c)
        b[c] = *reinterpret_cast<const f32x4*>(w2h + ((size_t)(ct[c] * kTiles + j) * 64 + lane) * 4);
}

__device__ __forceinline__ f32x4 mfma16(f16x8 a, f32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// One 32-wide k block: acc[r][c] += ahi * blo, then ahi * bhi, then alo * bhi (lane l holds k = 32 jp + 8 (l / 16) + 0..7 on
// both operands).  The lo set has one buffer: the next block's is requested as soon as the hi*lo products are issued.
template <int MR>
__device__ __forceinline__ void mma_block(f32x4 (&acc)[MR][2], const _Float16* ah, const _Float16* al, const f32x4 (&bh)[2],
                                          f32x4 (&bl)[2], const float* __restrict__ w2h, const int (&ct)[2], int jp, bool more,
                                          int lane) {
    f16x8 ahi[MR], alo[MR];
#pragma unroll
    for (int r = 0; r < MR; ++r) {
        const int off = (r * 16 + (lane & 15)) * kHalfStride + 32 * jp + (lane >> 4) * 8;
        ahi[r] = *reinterpret_cast<const f16x8*>(ah + off);
        alo[r] = *reinterpret_cast<const f16x8*>(al + off);
    }
#pragma unroll
    for (int r = 0; r < MR; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[r][c] = mfma16(ahi[r], bl[c], acc[r][c]);
    if (more) load_h(bl, w2h, ct, 2 * jp + 3, lane);
#pragma unroll
    for (int prod = 0; prod < 2; ++prod)
#pragma unroll
        for (int r = 0; r < MR; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[r][c] = mfma16(prod ? alo[r] : ahi[r], bh[c], acc[r][c]);
}

// layer 2 over the kH / 32 blocks: the next block's hi set is requested before this block's MFMAs (register double buffer)
template <int MR>
__device__ __forceinline__ void layer_mma_f16x3(f32x4 (&acc)[MR][2], const float* act, const float* __restrict__ w2h,
                                                const int (&ct)[2], int lane) {
    constexpr int NB = kH / 32;
    static_assert(NB % 2 == 0, "the loop below takes the blocks in pairs");
    const _Float16* ah = reinterpret_cast<const _Float16*>(act);
    const _Float16* al = ah + kPlaneHalves;
    f32x4 h0[2], h1[2], l[2];
    load_h(h0, w2h, ct, 0, lane);
    load_h(l, w2h, ct, 1, lane);
    int jp = 0;
#pragma unroll 1
    for (; jp + 2 < NB; jp += 2) {
        load_h(h1, w2h, ct, 2 * jp + 2, lane);
        __builtin_amdgcn_sched_barrier(0);      // keep the prefetch ahead of the MFMAs it hides behind
        mma_block<MR>(acc, ah, al, h0, l, w2h, ct, jp, true, lane);
        load_h(h0, w2h, ct, 2 * jp + 4, lane);
        __builtin_amdgcn_sched_barrier(0);
        mma_block<MR>(acc, ah, al, h1, l, w2h, ct, jp + 1, true, lane);
    }
    load_h(h1, w2h, ct, 2 * NB - 2, lane);
    mma_block<MR>(acc, ah, al, h0, l, w2h, ct, NB - 2, true, lane);
    mma_block<MR>(acc, ah, al, h1, l, w2h, ct, NB - 1, false, lane);
}

// The 64-row twin-head tile with f16 activation planes: the carve-up of mfma_tile.hpp moved behind the larger tile
struct TileF16x3 {
    static constexpr int kOffAct = 0;                                   // 2 planes [64][264] halves
    static constexpr int kOffXs = kOffAct + kActFloats;                 // [64][4] (obs, candidate)
    static constexpr int kOffQpart = kOffXs + kRows * 4;                // [2 heads][8 waves][64 rows]
    static constexpr int kOffOwn = kOffQpart + 2 * kWaves * kRows;

    // q_phase of mfma_tile.hpp with layer 1's output split into the planes and layer 2 on layer_mma_f16x3
    template <int MR, class Args>
    static __device__ __forceinline__ void q_phase(float* lds, const Args& a, int wave, int lane) {
        const int ln = opaque(lane);
        const int ct[2] = {2 * wave, 2 * wave + 1};
        float* act = lds + kOffAct;
        _Float16* ah = reinterpret_cast<_Float16*>(act);
        _Float16* al = ah + kPlaneHalves;
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
            // layer 1: K = 4 inputs = ONE exact f32 mfma per tile
#pragma unroll
            for (int r = 0; r < MR; ++r) {
                const float x = xs[(r * 16 + (ln & 15)) * 4 + (ln >> 4)];
#pragma unroll
                for (int c = 0; c < 2; ++c) acc[r][c] = mfma(x, w1v[c], acc[r][c]);
            }
            // hi / lo of relu(acc + b1[col]); C layout: row = 16 r + 4 (lane / 16) + i, col = 16 ct + lane % 16
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int col = ct[c] * 16 + (opaque(lane) & 15);
#pragma unroll
                for (int r = 0; r < MR; ++r)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        _Float16 hi, lo;
                        split16(reluf(acc[r][c][i] + b1v[c]), hi, lo);
                        const int at = (r * 16 + 4 * (opaque(lane) >> 4) + i) * kHalfStride + col;
                        ah[at] = hi;
                        al[at] = lo;
                    }
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < MR; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
            layer_mma_f16x3<MR>(acc, act, a.W2p + (size_t)h * kH * kH, ct, opaque(lane));
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
            __syncthreads();       // the planes are free again; qpart[h] complete
        }
    }

    template <class Args>
    static __device__ __forceinline__ TwinQ twin_q(const float* lds, const Args& a, int row) {
        return rrl_tile::twin_q<Args, kOffQpart>(lds, a, row);
    }
};

}  // namespace rrl_tile
