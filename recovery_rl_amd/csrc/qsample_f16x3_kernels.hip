// qsample_f16x3_kernels.hip -- the score kernels of the Q-sampling recovery acting call (qsample_kernels.hip, qsample_env.hpp)
// with layer 2 of the twin Q_risk as three v_mfma_f32_16x16x32_f16 products of hi / lo f16 splits instead of
// v_mfma_f32_16x16x4_f32: the planner's F16X3 arithmetic on the tile of mfma_tile_f16x3.hpp (TileF16x3, shared with
// sqrl_f16x3_kernels.hip).  The gate, the candidate draws, the folded last layer, twin_q, the chunk's argmin, the partials and
// the tick protocol are the f32 kernels' text (qsample_env.hpp); the fold kernels are the f32 family's own
// (rrl_qsample::launch_fold).  W2p names the hi / lo stream rrl_w2_pack_f16x3 writes.
//
// Precision (rrl_hip.h): layer 1 (K = 4) is one exact f32 MFMA per tile.  Its relu output v is kept as hi = f16(v),
// lo = f16(v - hi) in two f16 planes; layer 2 accumulates, per 32-wide k block in ascending order, hi*lo, hi*hi, lo*hi in f32;
// lo*lo (2^-22 of the product) is dropped.
#include "mfma_tile_f16x3.hpp"
#include "qsample_env.hpp"

using namespace rrl_host;
using namespace rrl_tile;
using namespace rrl_qsample;

namespace {

// the tile's kOffOwn (18 176 floats) + [128][2] candidates + [128] q
constexpr int kLdsBytes = Lds<TileF16x3>::kLdsBytes;         // 74 240 B: two workgroups per CU
static_assert(kLdsBytes == 74240 && kLdsBytes <= 80 * 1024, "two workgroups share a CU");

__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void qsample_score_f16x3_kernel(const ArgBlock a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    score_chunk<TileF16x3>(a, blockIdx.x, lds);
}

// S learners side by side, as qsample_score_pack_kernel (qsample_kernels.hip)
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void qsample_score_f16x3_pack_kernel(const ArgBlock* __restrict__ blocks, rrl_pack::Idx ix) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int s, local;
    if (!rrl_pack::locate(ix, blockIdx.x, s, local)) return;
    ArgBlock a = blocks[s];
    globalize(a);
    score_chunk<TileF16x3>(a, unsigned(local), lds);
}

int launch_score(const ArgBlock& a, unsigned grid, hipStream_t st) {
    static bool lds_set = false;
    const int rc = grant_lds(qsample_score_f16x3_kernel, kLdsBytes, lds_set);
    if (rc != RRL_OK) return rc;
    hipLaunchKernelGGL(qsample_score_f16x3_kernel, dim3(grid), dim3(kThreads), kLdsBytes, st, a);
    return check_launch();
}

int launch_score_pack(const rrl_pack::Plan& plan, hipStream_t st) {
    static bool lds_set = false;
    const int rc = grant_lds(qsample_score_f16x3_pack_kernel, kLdsBytes, lds_set);
    if (rc != RRL_OK) return rc;
    hipLaunchKernelGGL(qsample_score_f16x3_pack_kernel, dim3((unsigned)plan.grid), dim3(kThreads), kLdsBytes, st,
                       (const ArgBlock*)plan.dev, plan.ix);
    return check_launch();
}

}  // namespace

extern "C" {

int rrl_qsample_act_f16x3(const rrl_qsample_act_t* p, void* stream) { return solo_entry(p, nullptr, stream, launch_score); }

int rrl_qsample_act_gated_f16x3(const rrl_qsample_act_t* p, const rrl_qsample_gate_t* g, void* stream) {
    if (!g) return RRL_EINVAL;
    return solo_entry(p, g, stream, launch_score);
}

int rrl_qsample_act_f16x3_packed(int S, const rrl_qsample_act_t* args, const rrl_qsample_gate_t* gates, void* stream) {
    return packed_entry(rrl_pack::Site::QsampleActF16x3, S, args, gates, stream, launch_score, launch_score_pack);
}

}  // extern "C"
