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
// The tile and the twin-head phase (q_phase) come from mfma_tile.hpp, shared with sqrl_kernels.hip; the body itself (gate, chunk,
// fold), the descriptor checks and the host protocol of the entries from qsample_env.hpp, shared with qsample_f16x3_kernels.hip.
// The fold kernels live here only: both families launch them through rrl_qsample::launch_fold / launch_fold_pack.
#include "qsample_env.hpp"

using namespace rrl_host;
using namespace rrl_tile;
using namespace rrl_qsample;

namespace {

// the argument block under the name these kernels' symbols carry
struct QsArgs : ArgBlock {};

// the exact-f32 tile of mfma_tile.hpp, as qsample_env names a tile
struct TileF32 {
    static constexpr int kOffXs = rrl_tile::kOffXs, kOffOwn = rrl_tile::kOffOwn;
    template <int MR>
    static __device__ __forceinline__ void q_phase(float* lds, const ArgBlock& a, int wave, int lane) {
        rrl_tile::q_phase<MR>(lds, a, wave, lane);
    }
    static __device__ __forceinline__ TwinQ twin_q(const float* lds, const ArgBlock& a, int row) {
        return rrl_tile::twin_q(lds, a, row);
    }
};

constexpr int kLdsBytes = Lds<TileF32>::kLdsBytes;           // 73.2 KB: two workgroups per CU

__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void qsample_score_kernel(const QsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    score_chunk<TileF32>(a, blockIdx.x, lds);
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
    score_chunk<TileF32>(a, unsigned(local), lds);
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

int launch_score(const ArgBlock& a, unsigned grid, hipStream_t st) {
    static bool lds_set = false;
    const int rc = grant_lds(qsample_score_kernel, kLdsBytes, lds_set);
    if (rc != RRL_OK) return rc;
    hipLaunchKernelGGL(qsample_score_kernel, dim3(grid), dim3(kThreads), kLdsBytes, st, QsArgs{a});
    return check_launch();
}

int launch_score_pack(const rrl_pack::Plan& plan, hipStream_t st) {
    static bool lds_set = false;
    const int rc = grant_lds(qsample_score_pack_kernel, kLdsBytes, lds_set);
    if (rc != RRL_OK) return rc;
    hipLaunchKernelGGL(qsample_score_pack_kernel, dim3((unsigned)plan.grid), dim3(kThreads), kLdsBytes, st,
                       (const QsArgs*)plan.dev, plan.ix);
    return check_launch();
}

}  // namespace

namespace rrl_qsample {

int launch_fold(const ArgBlock& a, hipStream_t st) {
    hipLaunchKernelGGL(qsample_fold_kernel, dim3((unsigned)grid_for(a.n)), dim3(kBlock), 0, st, QsArgs{a});
    return check_launch();
}

int launch_fold_pack(const rrl_pack::Plan& plan, hipStream_t st) {
    hipLaunchKernelGGL(qsample_fold_pack_kernel, dim3((unsigned)plan.i0), dim3(kBlock), 0, st, (const QsArgs*)plan.dev,
                       plan.ix2);
    return check_launch();
}

}  // namespace rrl_qsample

extern "C" {

long long rrl_qsample_scratch_floats(long long n, int k) {
    if (n <= 0) return RRL_EINVAL;
    if (k < 1 || k > kMaxK || n * k >= (1LL << 32)) return RRL_ERANGE;
    return n * chunks_of(k) * kPartial;      // one partial per workgroup of the score kernel
}

int rrl_qsample_act(const rrl_qsample_act_t* p, void* stream) { return solo_entry(p, nullptr, stream, launch_score); }

int rrl_qsample_act_gated(const rrl_qsample_act_t* p, const rrl_qsample_gate_t* g, void* stream) {
    if (!g) return RRL_EINVAL;
    return solo_entry(p, g, stream, launch_score);
}

int rrl_qsample_act_packed(int S, const rrl_qsample_act_t* args, const rrl_qsample_gate_t* gates, void* stream) {
    return packed_entry(rrl_pack::Site::QsampleAct, S, args, gates, stream, launch_score, launch_score_pack);
}

}  // extern "C"
