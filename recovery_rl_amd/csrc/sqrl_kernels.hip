// sqrl_kernels.hip -- SQRL constraint-sampling acting (SAC._sqrl_action, recovery_rl/sac.py:139-161) as ONE MFMA kernel
// for gfx950: per env, k candidate actions from the task policy's head, the twin Q_risk on every candidate, and the pick.
//
// The module path expands every observation to k rows and runs both networks on n k rows.  The policy sees the same state
// k times, so its head is taken from the n-row acting forward that exists already; what is left is the twin Q_risk
// (4 -> 256 relu -> 256 relu -> 1, two heads) on n k rows.  One workgroup owns one env: its candidates go through the
// network in passes of up to 64 rows with the activations in LDS (the planner's tile, plan_kernels.hip), W2 arrives from
// L2 in MFMA fragment order (rrl_w2_pack: the copy the optimiser launch keeps current), and only action[n, 2] leaves the
// chip.  Arithmetic is v_mfma_f32_16x16x4_f32 (exact f32 fma chains).
//
// The tile and the twin-head phase (q_phase) come from mfma_tile.hpp, shared with qsample_kernels.hip; the env itself (candidates,
// score passes, pick), the descriptor checks and the host protocol of the entries from sqrl_env.hpp, shared with
// sqrl_f16x3_kernels.hip.
#include "sqrl_env.hpp"
#include "pack.hpp"

using namespace rrl_host;
using namespace rrl_tile;
using namespace rrl_sqrl;

namespace {

// the argument block under the name these kernels' symbols carry
struct SqrlArgs : ArgBlock {};

// the exact-f32 tile of mfma_tile.hpp, as sqrl_env names a tile
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

constexpr int kLdsBytes = Lds<TileF32>::kLdsBytes;           // 74.8 KB: two workgroups per CU

template <int NT>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void sqrl_act_kernel(const SqrlArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    sqrl_env<NT, TileF32>(a, blockIdx.x, lds);
    rrl::advance_counter(a.counter_dev, a.counter_inc);
}

// S learners side by side (pack.hpp): workgroup b serves env `local` of seed s, on seed s's own argument block.  All seeds share
// NT (one k per call).  A seed's tick is advanced by the last of ITS n workgroups -- the grid's size says nothing about it --
// and a padding workgroup of a pinned mapping leaves before it touches anything, the ticket included.
template <int NT>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void sqrl_act_pack_kernel(const SqrlArgs* __restrict__ blocks, rrl_pack::Idx ix) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int s, local;
    if (!rrl_pack::locate(ix, blockIdx.x, s, local)) return;
    SqrlArgs a = blocks[s];
    rrl_pack::to_global_all(a.obs, a.head, a.scale, a.bias, a.W1, a.b1, a.W2p, a.b2, a.W3, a.b3, a.counter_dev, a.eps_in, a.u_in,
                            a.action, a.q, a.logp, a.cand, a.z, a.pick, a.cstar, a.n_safe);
    sqrl_env<NT, TileF32>(a, local, lds);
    rrl::advance_counter_blocks(a.counter_dev, a.counter_inc, unsigned(a.n));
}

template <int NT>
int launch(const SqrlArgs& a, int n, hipStream_t st) {
    static bool lds_set = false;
    const int rc = grant_lds(sqrl_act_kernel<NT>, kLdsBytes, lds_set);
    if (rc != RRL_OK) return rc;
    hipLaunchKernelGGL(sqrl_act_kernel<NT>, dim3((unsigned)n), dim3(kThreads), kLdsBytes, st, a);
    return check_launch();
}

template <int NT>
int launch_pack(const rrl_pack::Plan& plan, hipStream_t st) {
    static bool lds_set = false;
    const int rc = grant_lds(sqrl_act_pack_kernel<NT>, kLdsBytes, lds_set);
    if (rc != RRL_OK) return rc;
    hipLaunchKernelGGL(sqrl_act_pack_kernel<NT>, dim3((unsigned)plan.grid), dim3(kThreads), kLdsBytes, st,
                       (const SqrlArgs*)plan.dev, plan.ix);
    return check_launch();
}

}  // namespace

extern "C" {

long long rrl_sqrl_scratch_floats(long long n, int k) {
    if (n <= 0) return RRL_EINVAL;
    if (k < 1 || k > kMaxK || n * k >= (1LL << 32)) return RRL_ERANGE;
    return 0;            // the one-kernel form keeps q, logp and the candidates in LDS
}

int rrl_sqrl_act(const rrl_sqrl_act_t* p, void* stream) {
    return solo_entry(p, stream, [](auto nt, const ArgBlock& a, int n, hipStream_t st) {
        return launch<decltype(nt)::value>(SqrlArgs{a}, n, st);
    });
}

int rrl_sqrl_act_packed(int S, const rrl_sqrl_act_t* args, void* stream) {
    return packed_entry(rrl_pack::Site::SqrlAct, S, args, stream, rrl_sqrl_act,
                        [](auto nt, const rrl_pack::Plan& plan, hipStream_t st) {
                            return launch_pack<decltype(nt)::value>(plan, st);
                        });
}

}  // extern "C"
