// sqrl_f16x3_kernels.hip -- SQRL's constraint-sampling acting pass (sqrl_kernels.hip, sqrl_env.hpp) with layer 2 of the twin
// Q_risk as three v_mfma_f32_16x16x32_f16 products of hi / lo f16 splits instead of v_mfma_f32_16x16x4_f32: the planner's
// F16X3 arithmetic on the tile of mfma_tile_f16x3.hpp (TileF16x3, shared with qsample_f16x3_kernels.hip).  Candidates,
// log-probabilities, the folded last layer, twin_q, the pick and the tick protocol are the f32 kernel's text (sqrl_env.hpp).
//
// Precision (rrl_hip.h): layer 1 (K = 4) is one exact f32 MFMA per tile.  Its relu output v is kept as hi = f16(v),
// lo = f16(v - hi) in two f16 planes; W2 arrives split the same way (rrl_w2_pack_f16x3).  Layer 2 accumulates, per 32-wide
// k block in ascending order, hi*lo, hi*hi, lo*hi in f32; lo*lo (2^-22 of the product) is dropped.
#include "mfma_tile_f16x3.hpp"
#include "sqrl_env.hpp"
#include "pack.hpp"

using namespace rrl_host;
using namespace rrl_tile;
using namespace rrl_sqrl;

namespace {

constexpr int kLdsBytes = Lds<TileF16x3>::kLdsBytes;         // 75 808 B: two workgroups per CU
static_assert(kLdsBytes <= 80 * 1024, "two workgroups share a CU");

template <int NT>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void sqrl_act_f16x3_kernel(const ArgBlock a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    sqrl_env<NT, TileF16x3>(a, blockIdx.x, lds);
    rrl::advance_counter(a.counter_dev, a.counter_inc);
}

// S learners side by side, as sqrl_act_pack_kernel (sqrl_kernels.hip)
template <int NT>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void sqrl_act_f16x3_pack_kernel(const ArgBlock* __restrict__ blocks, rrl_pack::Idx ix) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int s, local;
    if (!rrl_pack::locate(ix, blockIdx.x, s, local)) return;
    ArgBlock a = blocks[s];
    rrl_pack::to_global_all(a.obs, a.head, a.scale, a.bias, a.W1, a.b1, a.W2p, a.b2, a.W3, a.b3, a.counter_dev, a.eps_in, a.u_in,
                            a.action, a.q, a.logp, a.cand, a.z, a.pick, a.cstar, a.n_safe);
    sqrl_env<NT, TileF16x3>(a, local, lds);
    rrl::advance_counter_blocks(a.counter_dev, a.counter_inc, unsigned(a.n));
}

// The hi / lo fragment stream of G [H, H] matrices (rrl_hip.h): one thread per (matrix, column tile, 32-wide block, lane) writes
// its two float4 slots.  The planner's pack (pack_layer_f16x3_k32_kernel), weights beyond the f16 range clamped as there.
__global__ __launch_bounds__(kBlock) void w2_pack_f16x3_kernel(int G, int H, const float* __restrict__ W2,
                                                               float* __restrict__ W2h) {
    const int J = H / 16, NB = H / 32;
    const long long total = (long long)G * J * NB * 64;
    for (long long f = blockIdx.x * (long long)kBlock + threadIdx.x; f < total; f += (long long)gridDim.x * kBlock) {
        const int lane = int(f & 63);
        const long long blk = f >> 6;
        const int jp = int(blk % NB), ct = int((blk / NB) % J), g = int(blk / ((long long)NB * J));
        const int n = 16 * ct + (lane & 15);
        const float* src = W2 + ((long long)g * H + n) * H + 32 * jp + 8 * (lane >> 4);
        float* dst = W2h + (long long)g * H * H;
        _Float16* hi = reinterpret_cast<_Float16*>(dst + (((long long)ct * J + 2 * jp) * 64 + lane) * 4);
        _Float16* lo = reinterpret_cast<_Float16*>(dst + (((long long)ct * J + 2 * jp + 1) * 64 + lane) * 4);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            float w = src[t];
            w = w > 65504.f ? 65504.f : (w < -65504.f ? -65504.f : w);
            const _Float16 h = (_Float16)w;
            hi[t] = h;
            lo[t] = (_Float16)(w - (float)h);
        }
    }
}

template <int NT>
int launch(const ArgBlock& a, int n, hipStream_t st) {
    static bool lds_set = false;
    const int rc = grant_lds(sqrl_act_f16x3_kernel<NT>, kLdsBytes, lds_set);
    if (rc != RRL_OK) return rc;
    hipLaunchKernelGGL(sqrl_act_f16x3_kernel<NT>, dim3((unsigned)n), dim3(kThreads), kLdsBytes, st, a);
    return check_launch();
}

template <int NT>
int launch_pack(const rrl_pack::Plan& plan, hipStream_t st) {
    static bool lds_set = false;
    const int rc = grant_lds(sqrl_act_f16x3_pack_kernel<NT>, kLdsBytes, lds_set);
    if (rc != RRL_OK) return rc;
    hipLaunchKernelGGL(sqrl_act_f16x3_pack_kernel<NT>, dim3((unsigned)plan.grid), dim3(kThreads), kLdsBytes, st,
                       (const ArgBlock*)plan.dev, plan.ix);
    return check_launch();
}

}  // namespace

extern "C" {

int rrl_w2_pack_f16x3(int G, int H, const float* W2, float* W2h, void* stream) {
    if (!W2 || !W2h || (reinterpret_cast<uintptr_t>(W2h) & 15) || G <= 0 || H <= 0 || (H & 31)) return RRL_EINVAL;
    const long long total = (long long)G * (H / 16) * (H / 32) * 64;
    hipLaunchKernelGGL(w2_pack_f16x3_kernel, dim3(grid_for(total)), dim3(kBlock), 0, (hipStream_t)stream, G, H, W2, W2h);
    return check_launch();
}

int rrl_sqrl_act_f16x3(const rrl_sqrl_act_t* p, void* stream) {
    return solo_entry(p, stream, [](auto nt, const ArgBlock& a, int n, hipStream_t st) {
        return launch<decltype(nt)::value>(a, n, st);
    });
}

int rrl_sqrl_act_f16x3_packed(int S, const rrl_sqrl_act_t* args, void* stream) {
    return packed_entry(rrl_pack::Site::SqrlActF16x3, S, args, stream, rrl_sqrl_act_f16x3,
                        [](auto nt, const rrl_pack::Plan& plan, hipStream_t st) {
                            return launch_pack<decltype(nt)::value>(plan, st);
                        });
}

}  // extern "C"
