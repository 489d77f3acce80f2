// env_models.hpp -- each env stated once: the transition with its flags, and the start state.  Every kernel that steps an
// env (the stand-alone step kernels, the open-loop and offline rollouts, the fused step + push of step_push.hpp, the
// evaluation rollout) calls these; the arithmetic itself is rrl_device.hpp's (navigation) and maze_device.hpp's (maze).
// The trait the step kernels are templates on:
//   static Outcome ENV::step(seed, row, ctr, pos, action)      one transition, its noise (if any) drawn
//   static bool    ENV::timed_out(t_after, horizon)            whether the env itself ends an episode at its horizon
//   static double2 ENV::reset(seed, row, ctr)                  the start state of a new episode
//   ENV::kLongStep                                             ask for whatever the step does not read BEHIND it
// Next to the trait stands each env's transition proper, which takes the action in f64 and the noise as a value (offline
// data, caller-given noise).
// The horizon rule is apart from the step because the step does not need the count: a caller ORs it into `done` behind the
// step, where it holds the count (asked for in front of the maze's 64 sub-steps, the count stays in a register across them;
// and the evaluation rollout's kernels keep their instruction sequence only with the comparison behind the move).
// Force-inlined and returned by value: the six results stay in registers, and the callers keep the instruction sequences of
// the spelled-out text.  The trait form widens the f32 action BEHIND its draw: widened at the call site, the fused step + push
// kernels come out with another schedule (up to 90 instructions fewer or 11 more).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "maze_device.hpp"
#include "rrl_device.hpp"

namespace rrl_env {

// What one transition leaves: the next state, the reward and the three flags of the eager env's step()
struct Outcome {
    double x, y;        // next position (before an auto-reset)
    float reward;
    bool constraint, success, done;   // done = the env's own termination but for ENV::timed_out(), which the caller ORs in
};

// the step noise of row `row` at counter `ctr` (the same for both kinds: a caller that picks the kind at run time draws once)
__device__ __forceinline__ double2 nav_step_noise(uint64_t seed, uint32_t row, uint64_t ctr) {
    double ex, ey;
    rrl::normal_at(seed, row, rrl::kStreamStep, ctr, ex, ey);
    return make_double2(ex, ey);
}

// what the navigation envs make of a move: the kind enters only the move and its obstacle test (NavEnv::move), not the flags
__device__ __forceinline__ Outcome nav_outcome(double nx, double ny, double cost, bool constraint) {
    Outcome o;
    o.x = nx;
    o.y = ny;
    o.reward = float(cost);
    o.constraint = constraint;
    o.success = cost > -4.0;
    o.done = o.success | o.constraint;
    return o;
}

// Navigation 1 / 2 (env/navigation1.py:71-110): start at START_STATE + N(0, I); the cost is judged at the OLD state,
// done = success | constraint.  The step noise and the start-state noise are either given or drawn from the row's streams.
template <int KIND>
struct NavEnv {
    static constexpr bool kLongStep = false;
    static __device__ __forceinline__ bool in_constraint(double x, double y) { return rrl::in_obstacle<KIND>(x, y); }
    // next state and cost; returns the constraint flag (for the caller that picks the kind at run time, around this alone)
    static __device__ __forceinline__ bool move(double2 p, double ax, double ay, double ex, double ey, double& nx, double& ny,
                                                double& cost) {
        rrl::nav_transition<KIND>(p.x, p.y, ax, ay, ex, ey, nx, ny, cost);
        return rrl::in_obstacle<KIND>(nx, ny);
    }
    static __device__ __forceinline__ Outcome step(double2 p, double ax, double ay, double ex, double ey) {
        double nx, ny, cost;
        const bool constraint = move(p, ax, ay, ex, ey, nx, ny, cost);
        return nav_outcome(nx, ny, cost, constraint);
    }
    static __device__ __forceinline__ Outcome step(uint64_t seed, uint32_t row, uint64_t ctr, double2 p, float2 act) {
        const double2 e = nav_step_noise(seed, row, ctr);
        return step(p, double(act.x), double(act.y), e.x, e.y);
    }
    static __device__ __forceinline__ bool timed_out(int32_t, int32_t) { return false; }     // the horizon is the caller's
    static __device__ __forceinline__ double2 reset(double z0, double z1) {
        return make_double2(-50.0 + z0, 0.0 + z1);     // START_STATE + randn(2), navigation1.py:92
    }
    static __device__ __forceinline__ double2 reset(uint64_t seed, uint32_t row, uint64_t ctr) {
        double z0, z1;
        rrl::normal_at(seed, row, rrl::kStreamReset, ctr, z0, z1);
        return reset(z0, z1);
    }
};

// Maze (env/maze.py:139-232 on the kinematic surrogate of maze_device.hpp): reset of mode 0 with the rejection loop; the
// step draws nothing, the reward is judged at the NEW state, and the env's own horizon ends an episode with neither flag
struct MazeEnv {
    static constexpr bool kLongStep = true;        // 64 collision sub-steps: what can be asked for behind the step should be
    static __device__ __forceinline__ bool timed_out(int32_t t_after, int32_t horizon) { return t_after >= horizon; }
    static __device__ __forceinline__ Outcome step(double2 p, double ax, double ay) {
        Outcome o;
        o.x = p.x;
        o.y = p.y;
        rrl_maze::move(o.x, o.y, ax, ay);          // clamps to +-0.1 itself
        const double d = rrl_maze::goal_distance(o.x, o.y);
        o.reward = float(-d);
        o.constraint = rrl_maze::in_contact(o.x, o.y);
        o.success = -d > -0.03;
        o.done = o.constraint | (d < rrl_maze::kGoalThresh);      // env/maze.py:207-213, with timed_out()
        return o;
    }
    static __device__ __forceinline__ Outcome step(uint64_t, uint32_t, uint64_t, double2 p, float2 act) {
        return step(p, double(act.x), double(act.y));
    }
    static __device__ __forceinline__ double2 reset(uint64_t seed, uint32_t row, uint64_t ctr) {
        double x, y;
        rrl_maze::reset_one(seed, row, ctr, 0, true, x, y);
        return make_double2(x, y);
    }
};

}  // namespace rrl_env
