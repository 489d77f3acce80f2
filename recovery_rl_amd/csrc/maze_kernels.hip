// maze_kernels.hip -- batched Maze env for gfx950 (MI355X).
//
// Counterpart of env/maze.py:139-232.  The reference advances MuJoCo 1.50 (500 sim steps per
// env step); that third-party engine is not available, so the kernels run the documented
// kinematic surrogate: straight-line displacement GAIN * a, stopped at the
// first of 64 sub-steps where the disc touches a wall rectangle or an arena plane.  Same I/O
// layout and launch shape as the navigation kernels: one lane per env, SoA, HBM-bound.
#include <hip/hip_runtime.h>

#include "env_models.hpp"
#include "maze_device.hpp"
#include "replay_device.hpp"
#include "rrl_device.hpp"
#include "rrl_host.hpp"
#include "step_push.hpp"

#pragma clang fp contract(off)

namespace {

using rrl_host::check_launch;
using rrl_host::grid_for;
using rrl_host::kBlock;

using namespace rrl_maze;
using rrl_env::MazeEnv;

__global__ __launch_bounds__(kBlock) void maze_reset_kernel(int64_t n, double2* pos, float2* obs,
                                                            int32_t* t, const uint8_t* mask, int mode,
                                                            int check, uint64_t seed, uint64_t counter,
                                                            const uint64_t* counter_dev) {
    const uint64_t ctr = rrl::effective_counter(counter, counter_dev);
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
        if (mask && !mask[i]) continue;
        double x, y;
        reset_one(seed, uint32_t(i), ctr, mode, check != 0, x, y);
        pos[i] = make_double2(x, y);
        if (t) t[i] = 0;
        if (obs) obs[i] = make_float2(float(x), float(y));
    }
}

// one lane per 20-step segment (env/maze.py:41-52: reset every 20 transitions)
__global__ __launch_bounds__(kBlock) void maze_offline_kernel(int64_t half, int64_t n_seg, uint64_t seed,
                                                              float2* s, float2* a, float* c, float2* s2,
                                                              float* m) {
    const int64_t g_all = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (g_all >= 2 * n_seg) return;
    const int part = g_all >= n_seg;
    const int64_t g = g_all - part * n_seg;
    const uint32_t row = uint32_t(g_all);
    const rrl::Bits128 b = rrl::philox_at(seed, row, rrl::kStreamOffline, 0);
    const double sample = rrl::unit_open(b.lo);
    const int mode = sample < 0.3 ? 1 : (sample < 0.6 ? 2 : 0);
    double x, y;
    reset_one(seed, row, 1ULL << 40, mode, false, x, y);
    const int64_t len = (g == n_seg - 1) ? half - 20 * g : 20;
    int64_t w = part * half + 20 * g;
    int steps = 0;
    for (int64_t j = 0; j < len; ++j, ++w) {
        double ax, ay;
        if (part == 0) {
            const rrl::Bits128 u = rrl::philox_at(seed, row, rrl::kStreamOffline, uint64_t(1 + j));
            ax = double(float(-0.1 + 0.2 * rrl::unit_open(u.lo)));   // action_space.sample() is float32 (:58)
            ay = double(float(-0.1 + 0.2 * rrl::unit_open(u.hi)));
        } else {
            expert_action(x, y, ax, ay);                             // float64 into step() (:88-89)
        }
        const float axf = float(ax), ayf = float(ay);
        const rrl_env::Outcome o = MazeEnv::step(make_double2(x, y), ax, ay);
        steps += 1;
        const bool dn = MazeEnv::timed_out(steps, 100) | o.done;
        s[w] = make_float2(float(x), float(y));
        a[w] = make_float2(axf, ayf);
        c[w] = o.constraint ? 1.0f : 0.0f;
        s2[w] = make_float2(float(o.x), float(o.y));
        m[w] = dn ? 0.0f : 1.0f;
        x = o.x;
        y = o.y;
    }
}

}  // namespace

extern "C" {

int rrl_maze_step(int64_t n, double* pos, const float* action, uint64_t seed, uint64_t counter,
                  uint64_t* counter_dev, uint64_t counter_inc, float* next_obs, float* obs,
                  float* reward, uint8_t* done, uint8_t* constraint, uint8_t* success,
                  uint8_t* ep_done, int32_t* t, int32_t horizon, int auto_reset, void* stream) {
    if (n < 0 || n > 0xffffffffLL) return RRL_ERANGE;
    if (!pos || !action || !next_obs || !reward || !done || !constraint || !success || !t)
        return RRL_EINVAL;
    if (n == 0) return RRL_OK;
    StepArgs a{n, (double2*)pos, (const float2*)action, nullptr, seed, counter, counter_dev, counter_inc,
               (float2*)next_obs, (float2*)obs, reward, done, constraint, success, ep_done, t, horizon,
               auto_reset};
    hipLaunchKernelGGL((env_step_kernel<MazeEnv, false>), dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch();
}

int rrl_maze_reset(int64_t n, double* pos, float* obs, int32_t* t, const uint8_t* mask, int mode,
                   int check_constraint, uint64_t seed, uint64_t counter,
                   const uint64_t* counter_dev, void* stream) {
    if (n < 0 || n > 0xffffffffLL) return RRL_ERANGE;
    if (!pos || mode < 0 || mode > 3) return RRL_EINVAL;
    if (n == 0) return RRL_OK;
    hipLaunchKernelGGL(maze_reset_kernel, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, n,
                       (double2*)pos, (float2*)obs, t, mask, mode, check_constraint, seed, counter,
                       counter_dev);
    return check_launch();
}

int rrl_maze_offline(int64_t num_transitions, uint64_t seed, float* s, float* a, float* c, float* s2,
                     float* m, int64_t capacity, void* stream) {
    if (num_transitions < 0 || !s || !a || !c || !s2 || !m) return RRL_EINVAL;
    const int64_t half = num_transitions / 2;
    if (2 * half > capacity) return RRL_ERANGE;
    if (half == 0) return RRL_OK;
    const int64_t n_seg = (half + 19) / 20;
    hipLaunchKernelGGL(maze_offline_kernel, dim3((unsigned)((2 * n_seg + kBlock - 1) / kBlock)),
                       dim3(kBlock), 0, (hipStream_t)stream, half, n_seg, seed, (float2*)s, (float2*)a, c,
                       (float2*)s2, m);
    return check_launch();
}

// (the solo entry stays in front of the packed one: the compiler emits the kernels in the order their launches are
// instantiated, and advance_cursors_kernel comes out an instruction longer in the other order)
int rrl_maze_step_push_x(const rrl_step_push_t* a, void* stream) {
    rrl_step::StepPushArgs p;
    const int rc = rrl_step::fill_args(p, a);
    if (rc != RRL_OK || a->n == 0) return rc;
    // latency regime: the reset draw (one Philox call + the contact test of the candidate; the start region is clear of
    // the walls, so the rejection loop runs once) beside the move instead of after it, and the early cursor ticket
    rrl_step::launch<MazeEnv>(p, a->n, (hipStream_t)stream);
    return check_launch();
}

int rrl_maze_step_push_packed(int S, const rrl_step_push_t* a, void* stream) {
    if (S <= 0 || S > rrl_pack::kMaxSeeds || !a) return RRL_EINVAL;
    // one seed: the packed launch IS the solo launch (argument block in the kernel arguments, no plan)
    if (S == 1) return rrl_maze_step_push_x(&a[0], stream);
    return rrl_step::launch_packed<MazeEnv>(rrl_pack::Key(rrl_pack::Site::MazeStep, S), S, a, (hipStream_t)stream);
}

}  // extern "C"
