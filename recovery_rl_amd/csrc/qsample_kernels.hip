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
// The matrix helpers are restated from sqrl_kernels.hip, not shared: a shared header would move that file's kernels.
#include "rrl_device.hpp"
#include "rrl_host.hpp"

using namespace rrl_host;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kStreamQsample = RRL_STREAM_QSAMPLE;
constexpr int kH = 256, kTiles = kH / 16;
constexpr int kMaxK = 1024;               // candidates per env
constexpr int kChunk = 128;               // candidates per workgroup
constexpr int kRows = 64;                 // rows per pass: 4 row tiles, every wave owns 2 column tiles of all of them
constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;
constexpr int kActStride = kH + 4;        // +4 floats: row r starts at bank 4r, ds_read_b128 conflict-free
constexpr int kPartial = 4;               // floats of a workgroup's partial: key, index (int bits), candidate x, y

// LDS carve-up (floats)
constexpr int kOffAct = 0;                                   // [64][260] activations of the current pass
constexpr int kOffXs = kOffAct + kRows * kActStride;         // [64][4] (obs, candidate)
constexpr int kOffQpart = kOffXs + kRows * 4;                // [2 heads][8 waves][64 rows] partial last-layer sums
constexpr int kOffCand = kOffQpart + 2 * kWaves * kRows;     // [128][2] candidate actions of the chunk
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
__device__ __forceinline__ void q_phase(float* lds, const QsArgs& a, int wave, int lane) {
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
        lds[kOffQ + r] = qm;
        const long long row = env * a.k + c0 + r;
        if (a.q) a.q[row] = qm;
        if (a.z) {
            a.z[row] = zv[0];
            a.z[(long long)a.n * a.k + row] = zv[1];
        }
    }
    // xs and qpart are rewritten only behind the next pass's barriers
}

// Workgroup b = env b / P, chunk b % P: candidates [128 chunk, 128 chunk + rows) of a gated env -> scratch[b] = its partial.
// Reads the tick, never writes it (the fold kernel advances it).
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void qsample_score_kernel(const QsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const long long env = blockIdx.x / (unsigned)a.P;
    if (a.mask && !a.mask[env]) return;           // the gate did not fire: nothing read, nothing written
    const int chunk = blockIdx.x % (unsigned)a.P;
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
            float* part = a.scratch + (size_t)blockIdx.x * kPartial;
            part[0] = best;
            part[1] = __int_as_float(c0 + bidx);
            part[2] = lds[kOffCand + 2 * bidx];
            part[3] = lds[kOffCand + 2 * bidx + 1];
        }
    }
}

// One thread per env: the P partials of a gated env in ascending chunk order (strict <: the lowest index wins), then
// action[e] (and pick[e]).  Thread 0 advances the tick: every reader of it ran in the score kernel before this one.
__global__ __launch_bounds__(kBlock) void qsample_fold_kernel(const QsArgs a) {
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < a.n; e += (long long)gridDim.x * kBlock) {
        if (a.mask && !a.mask[e]) continue;
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
    if (a.counter_dev && a.counter_inc && blockIdx.x == 0 && threadIdx.x == 0) a.counter_dev[0] += a.counter_inc;
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

}  // namespace

extern "C" {

long long rrl_qsample_scratch_floats(long long n, int k) {
    if (n <= 0) return RRL_EINVAL;
    if (k < 1 || k > kMaxK || n * k >= (1LL << 32)) return RRL_ERANGE;
    return n * chunks_of(k) * kPartial;      // one partial per workgroup of the score kernel
}

int rrl_qsample_act(const rrl_qsample_act_t* p, void* stream) {
    const int rc = check_desc(p);
    if (rc != RRL_OK) return rc;
    const QsArgs a{p->k, p->n, chunks_of(p->k), p->obs, p->mask, p->lo, p->hi, p->W1, p->b1, p->W2p, p->b2, p->W3, p->b3,
                   p->seed, p->counter, p->counter_dev, p->counter_inc, p->cand_in, p->scratch, p->action, p->q, p->z,
                   p->cand, p->pick};
    hipStream_t st = (hipStream_t)stream;
    static bool lds_set = false;            // > 64 KB of LDS has to be granted explicitly, once
    if (!lds_set) {
        if (hipFuncSetAttribute((const void*)qsample_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes) !=
            hipSuccess) {
            last_hip_error = int(hipGetLastError());
            return RRL_ELAUNCH;
        }
        lds_set = true;
    }
    hipLaunchKernelGGL(qsample_score_kernel, dim3((unsigned)((long long)a.n * a.P)), dim3(kThreads), kLdsBytes, st, a);
    const int rs = check_launch();
    if (rs != RRL_OK) return rs;
    hipLaunchKernelGGL(qsample_fold_kernel, dim3((unsigned)grid_for(a.n)), dim3(kBlock), 0, st, a);
    return check_launch();
}

}  // extern "C"
