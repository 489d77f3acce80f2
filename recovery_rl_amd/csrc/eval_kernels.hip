// eval_kernels.hip -- policy evaluation (Experiment.get_test_rollout, recovery_rl/experiment.py:493-538) for gfx950: one
// deterministic-policy episode of n Navigation 1 / 2 or Maze envs -- reset, then T x (task policy -> Q_risk gate -> recovery
// policy -> transition), per-env return and flags -- as ONE launch with no launch boundary inside.
//
// The module path runs horizon + 1 times three nn.Linear stacks, an eager env step and a handful of small torch ops: a few
// thousand dependent launches.  Here a workgroup owns a tile of 16 envs for the whole rollout: the env state (double position,
// return, flags) lives in the registers of the workgroup's first 16 threads, the networks run on one row tile of the tile of
// qsample_kernels.hip -- activations in LDS at stride 260, W2 from L2 in MFMA fragment order (rrl_w2_pack), one coalesced
// 1 KB load per fragment, v_mfma_f32_16x16x4_f32 with k ascending, 8 waves with 2 column tiles each -- and no weight changes
// during the rollout, so nothing has to leave the workgroup between two steps.
//
// Rows per workgroup: 16, one MFMA row tile (the issue allows 16 .. 64).  The rollout is a chain of T dependent steps, each a
// few L2 round trips long, so width over the chip comes before rows per workgroup: 4096 envs are 256 workgroups, one per CU.
// Larger tiles would read W2 less often per env; no other tile size was built or timed, so that trade is NOT measured
// (DESIGN section 7 has the times as shipped).
//
// ONE body (rollout_tile<Env, Form>) and two kernel templates over it: eval_rollout_kernel (the argument block in the kernel
// arguments, the tile index from the grid) and eval_rollout_pack_kernel (S seeds side by side, pack.hpp: block and tile index
// from a packed plan).  Their instantiations are the grid Env x Form, twenty kernels:
//   Env   NavRoll / MazeRoll adapt env_models.hpp's NavEnv / MazeEnv (a trait with reset and step, as step_push.hpp's), so the
//         Navigation kernels carry no Maze branch.
//   Form  NoQs (rrl_eval_rollout, rrl_eval_rollout_maze); QsOn / QsOnH (rrl_eval_rollout_qs[_f16x3]); SqOn / SqOnH
//         (rrl_eval_rollout_sqrl[_f16x3]); every entry has a _packed form.  The form names its descriptor, the group its
//         argument block carries, its LDS bytes and its occupancy; the host path (launch_solo / launch_packed) is one for all.
//
// The tile's primitives and layer-2 helpers come from mfma_tile.hpp (one row tile: MR = 1); run_stack is this file's own,
// for its 16 rows, DIN < 4 inputs and NOUT outputs.
//
// Q-sampling recovery (QsOn): a row whose gate fired while alive draws k uniform candidates (stream RRL_STREAM_EVAL_QSAMPLE,
// keyed by (env row, step) alone), scores them on the 64-row twin-head tile of mfma_tile.hpp (q_phase / twin_q: the bits of
// rrl_qsample_act) in passes of up to four row tiles, and executes the argmin.  The gated rows of a tile are served one
// after another in ascending row order (a workgroup-uniform loop over the gate's ballot), so k up to 1024 stays within one
// workgroup's LDS: the 64-row tile prefix (70.0 KB; the 16-row rollout regions lie inside its activation region, every
// hand-over behind a barrier) + candidates and their q (12 KB) + obs / results / mask (0.4 KB) = 82.4 KB, one workgroup per
// CU of the 160 KB -- the launch's shape anyway (4096 envs = 256 workgroups).  A tile with no gated live row skips the
// phase; rows that are not gated, dead or >= n draw and score nothing.
//
// SQRL (SqOn) has a different cost shape: there is no gate, EVERY live row needs k <= 128 candidates of the task policy's
// tanh-Gaussian head on every step.  The policy stack runs with four outputs (run_stack<2, 4>: mean and log_std rows; rows
// 0 .. 1 keep the bits of the two-output form, every output is a chain of its own), the candidates of the tile's live rows
// are drawn by all 512 threads (stream RRL_STREAM_EVAL_SQRL, keyed by (env row, step) alone) and FLATTENED, live rows in
// ascending order, into passes of up to four row tiles on the same 64-row twin-head tile -- every xs row carries its own
// obs, so candidates of different env rows share a pass: 25 passes per step at k = 100 with 16 live rows, against 32 when
// each row is served alone with a ragged second pass.  The candidates, logp and q of the whole tile stay in LDS, and the
// picks of different rows run on different waves (wave w: rows w and w + 8; the pick's double weights stay in registers and
// are read across the wave in ascending candidate order, so the sums are those of rrl_sqrl_act).  LDS: the 64-row tile
// prefix (70.0 KB) + candidates / logp / q (16 x 128 x 4 floats = 32 KB) + head / obs / results / row table / mask (0.9 KB)
// = 103.0 KB, one workgroup per CU.  The candidate-head arithmetic and the pick of sqrl_kernels.hip are RESTATED here
// (sq_candidates, sq_pick), not shared through a header: rrl_sqrl_act keeps its pick's weights in LDS and serves one env per
// workgroup, and its kernels keep their code untouched this way; tests/test_eval_sqrl_gpu.py holds the two to the same bits.
//
// f16x3 scoring (QsOnH / SqOnH): the candidate phases are templates on the scoring tile -- TileF32 (mfma_tile.hpp) or TileF16x3
// (mfma_tile_f16x3.hpp: layer 2 as three v_mfma_f32_16x16x32_f16 products of hi / lo splits, the bits of rrl_qsample_act_f16x3
// / rrl_sqrl_act_f16x3) -- and the per-form LDS regions start at the tile's kOffOwn (QsLds / SqLds: 83.4 KB and 104.0 KB on
// TileF16x3, whose planes are 1 KB larger).  These forms' groups carry the rrl_w2_pack_f16x3 stream as their last pointer;
// start, policy stack, gate (exact f32 on the 16-row stack, from the rrl_w2_pack copy), draws, head, picks, transition,
// results, traces and tick are the f32 forms' text.
//
// The twenty kernels are, instruction for instruction, the twenty hand-written ones they replace
// (profiles/eval_one_body_fingerprint.txt).
#include <type_traits>

#include "env_models.hpp"
#include "maze_device.hpp"
#include "mfma_tile.hpp"
#include "mfma_tile_f16x3.hpp"
#include "pack.hpp"
#include "rrl_device.hpp"
#include "rrl_host.hpp"

using namespace rrl_host;

namespace {

using rrl_env::Outcome;
using rrl_tile::f32x4;
using rrl_tile::kActStride;
using rrl_tile::kH;
using rrl_tile::kThreads;
using rrl_tile::kWaves;
using rrl_tile::layer_mma;
using rrl_tile::mfma;
using rrl_tile::opaque;
using rrl_tile::reduce16;
using rrl_tile::reluf;

constexpr uint32_t kStreamEval = RRL_STREAM_EVAL;
constexpr int kRows = 16;                 // rows per workgroup: one row tile, every wave owns 2 column tiles of it
constexpr int kMaxT = 4096, kMaxN = 1 << 22;

// LDS carve-up (floats)
constexpr int kOffAct = 0;                                   // [16][260] activations of the current stack
constexpr int kOffXs = kOffAct + kRows * kActStride;         // [16][4] (obs, task action)
constexpr int kOffPart = kOffXs + kRows * 4;                 // [2 outputs][8 waves][16 rows] partial last-layer sums
constexpr int kLdsFloats = kOffPart + 2 * kWaves * kRows;
constexpr int kLdsBytes = kLdsFloats * 4;                    // 17.5 KB

// Q-sampling form: the 64-row tile's prefix (act / xs / qpart of the scoring tile: TileF32 = mfma_tile.hpp, TileF16x3 =
// mfma_tile_f16x3.hpp) overlays the regions above -- they are dead between the gate's fold and the next step's xs, which is
// where the candidate phase runs -- and its own regions follow at the tile's kOffOwn
constexpr uint32_t kStreamEvalQs = RRL_STREAM_EVAL_QSAMPLE;
constexpr int kMaxK = 1024;                                  // candidates per gated row
template <class Tile>
struct QsLds {
    static constexpr int kOffCand = Tile::kOffOwn;           // [1024][2] candidates of the row being served
    static constexpr int kOffQ = kOffCand + kMaxK * 2;       // [1024] max(sigmoid z0, sigmoid z1)
    static constexpr int kOffObs = kOffQ + kMaxK;            // [16][2] float(pos) of the tile's rows
    static constexpr int kOffRes = kOffObs + kRows * 2;      // [16][4] pick (int bits), its q, that candidate
    static constexpr int kOffMask = kOffRes + kRows * 4;     // [1] the gate of the tile's rows, one bit each (int bits)
    static constexpr int kFloats = kOffMask + 4;
    static constexpr int kBytes = kFloats * 4;               // TileF32: 82.4 KB, TileF16x3: 83.4 KB -- one workgroup per CU
    static_assert(kLdsFloats <= Tile::kOffXs, "the rollout's regions lie inside the 64-row tile's activation region");
    static_assert(kBytes <= 160 * 1024, "one workgroup's LDS");
};

// SQRL form: the same overlay; the policy stack's four-output partial sums ([4][8][16] at kOffPart) stay inside the 64-row
// tile's activation region as well
constexpr uint32_t kStreamEvalSqrl = RRL_STREAM_EVAL_SQRL, kStreamEvalSqrlPick = RRL_STREAM_EVAL_SQRL_PICK;
constexpr int kSqMaxK = 128;                                 // candidates per live row
constexpr float kLogSigMax = 2.f, kLogSigMin = -20.f, kEps = 1e-6f;   // model.py:14-16 (sqrl_kernels.hip's)
constexpr float kHalfLog2Pi = 0.918938533204672742f;
template <class Tile>
struct SqLds {
    static constexpr int kOffCand = Tile::kOffOwn;                  // [16][128][2] candidates of the tile's rows
    static constexpr int kOffLogp = kOffCand + kRows * kSqMaxK * 2; // [16][128]
    static constexpr int kOffQ = kOffLogp + kRows * kSqMaxK;        // [16][128] max(sigmoid z0, sigmoid z1)
    static constexpr int kOffHead = kOffQ + kRows * kSqMaxK;        // [16][4] the policy's last-layer output
    static constexpr int kOffObs = kOffHead + kRows * 4;            // [16][2] float(pos)
    static constexpr int kOffRes = kOffObs + kRows * 2;             // [16][8] pick, cstar, n_safe (int bits), q, that candidate
    static constexpr int kOffRow = kOffRes + kRows * 8;             // [16] tile row of the s-th live row (int bits)
    static constexpr int kOffMask = kOffRow + kRows;                // [1] the live rows of the tile, one bit each (int bits)
    static constexpr int kFloats = kOffMask + 4;
    static constexpr int kBytes = kFloats * 4;               // TileF32: 103.0 KB, TileF16x3: 104.0 KB -- one workgroup per CU
    static_assert(kOffPart + 4 * kWaves * kRows <= Tile::kOffXs, "four outputs' partial sums lie inside the activation region");
    static_assert(kBytes <= 160 * 1024, "one workgroup's LDS");
};

struct Net {
    const float *W1, *b1, *W2p, *b2, *W3, *b3;
};

struct EvArgs {
    int n, T, kind, reset;                    // reset: 0 or 1
    int blocks;                               // workgroups of this rollout
    const double* pos;
    Net p;
    const float *scale, *bias;
    Net q;
    float eps_safe;
    Net r;
    const float *rscale, *rbias, *rlog_std;
    float min_log_std;
    uint64_t seed, counter;
    uint64_t* counter_dev;
    float* ret;
    uint8_t *success, *violation;
    int32_t* steps;
    double* tr_pos;
    float *tr_task, *tr_real, *tr_z, *tr_eps, *tr_reward;
    uint8_t* tr_flags;
};

// A form of the rollout is a trait: what rollout_tile does between the task action and the transition (on / sqrl), the tile
// its candidates are scored on and the Q_risk group they are scored with, and what a launch of it needs -- the descriptor,
// the group its argument block carries behind EvArgs (Args; globalize: its pointers in a packed plan's copy), the LDS
// bytes and the waves per SIMD its kernels are compiled for.

// The Q-sampling group (rrl_eval_rollout_qs_t's own fields)
struct QsArgs {
    int k;
    const float *lo, *hi;
    int32_t* tr_pick;
    float* tr_q;
};
// The base form: no candidate phase and no group (Args only types the pointer rollout_tile never follows), the stack's own
// 17.5 KB of LDS
struct NoQs {
    static constexpr bool on = false, sqrl = false;
    static constexpr int kWavesPerEu = 4, kLds = kLdsBytes;
    using Desc = rrl_eval_rollout_t;
    using Args = QsArgs;
};
// the exact-f32 tile of mfma_tile.hpp, as the candidate phases name a tile (TileF16x3 is the other one)
struct TileF32 {
    static constexpr int kOffXs = rrl_tile::kOffXs, kOffOwn = rrl_tile::kOffOwn;
    template <int MR>
    static __device__ __forceinline__ void q_phase(float* lds, const Net& q, int wave, int lane) {
        rrl_tile::q_phase<MR>(lds, q, wave, lane);
    }
    static __device__ __forceinline__ rrl_tile::TwinQ twin_q(const float* lds, const Net& q, int row) {
        return rrl_tile::twin_q(lds, q, row);
    }
};
using rrl_tile::TileF16x3;
// The candidate forms: 82.4 .. 104.0 KB of LDS put one workgroup = two waves per SIMD on a CU, so their kernels ask for that
// occupancy and its registers (at four waves' budget the rollout state beside the four-row-tile accumulators spilled)
struct QsOn {
    static constexpr bool on = true, sqrl = false;
    using Desc = rrl_eval_rollout_qs_t;
    using Args = QsArgs;
    using Tile = TileF32;
    static constexpr int kWavesPerEu = 2, kLds = QsLds<Tile>::kBytes;
    // the Q_risk group the candidates are scored with
    static __device__ __forceinline__ const Net& score_net(const EvArgs& a, const QsArgs&) { return a.q; }
    static __device__ __forceinline__ void globalize(QsArgs& g) { rrl_pack::to_global_all(g.lo, g.hi, g.tr_pick, g.tr_q); }
};
// f16x3 scoring (rrl_eval_rollout_qs_f16x3): the gate keeps a.q with its rrl_w2_pack copy, the candidates' layer 2 reads
// the rrl_w2_pack_f16x3 stream that rides beside the descriptor, the group's last pointer
struct QsArgsH : QsArgs {
    const float* w2h;
};
struct QsOnH {
    static constexpr bool on = true, sqrl = false;
    using Desc = rrl_eval_rollout_qs_t;
    using Args = QsArgsH;
    using Tile = TileF16x3;
    static constexpr int kWavesPerEu = 2, kLds = QsLds<Tile>::kBytes;
    static __device__ __forceinline__ Net score_net(const EvArgs& a, const QsArgsH& s) {
        return Net{a.q.W1, a.q.b1, s.w2h, a.q.b2, a.q.W3, a.q.b3};
    }
    static __device__ __forceinline__ void globalize(QsArgsH& g) {
        rrl_pack::to_global_all(g.lo, g.hi, g.tr_pick, g.tr_q, g.w2h);
    }
};
// ... and the SQRL group (rrl_eval_rollout_sqrl_t's own fields)
struct SqArgs {
    int k;
    float* tr_head;
    int32_t *tr_pick, *tr_cstar, *tr_nsafe;
    float* tr_q;
};
struct SqOn {
    static constexpr bool on = false, sqrl = true;
    using Desc = rrl_eval_rollout_sqrl_t;
    using Args = SqArgs;
    using Tile = TileF32;
    static constexpr int kWavesPerEu = 2, kLds = SqLds<Tile>::kBytes;
    static __device__ __forceinline__ const Net& score_net(const EvArgs& a, const SqArgs&) { return a.q; }
    static __device__ __forceinline__ void globalize(SqArgs& g) {
        rrl_pack::to_global_all(g.tr_head, g.tr_pick, g.tr_cstar, g.tr_nsafe, g.tr_q);
    }
};
// f16x3 scoring (rrl_eval_rollout_sqrl_f16x3): a.q.W2p is not read, layer 2 reads the rrl_w2_pack_f16x3 stream
struct SqArgsH : SqArgs {
    const float* w2h;
};
struct SqOnH {
    static constexpr bool on = false, sqrl = true;
    using Desc = rrl_eval_rollout_sqrl_t;
    using Args = SqArgsH;
    using Tile = TileF16x3;
    static constexpr int kWavesPerEu = 2, kLds = SqLds<Tile>::kBytes;
    static __device__ __forceinline__ Net score_net(const EvArgs& a, const SqArgsH& s) {
        return Net{a.q.W1, a.q.b1, s.w2h, a.q.b2, a.q.W3, a.q.b3};
    }
    static __device__ __forceinline__ void globalize(SqArgsH& g) {
        rrl_pack::to_global_all(g.tr_head, g.tr_pick, g.tr_cstar, g.tr_nsafe, g.tr_q, g.w2h);
    }
};
static_assert(QsOnH::kLds == QsOn::kLds + 1024 && SqOnH::kLds == SqOn::kLds + 1024, "the f16 planes cost 1 KB over the f32 activations");
template <class Form>
constexpr bool kHasGroup = Form::on || Form::sqrl;

// One 2-hidden-layer stack (head `head` of w) on the row tile in xs: inputs = the first DIN columns of xs, outputs = the
// first NOUT rows of W3.  Leaves part[o][wave][row] (output o's pre-activation is b3[o] + the sum over the 8 waves, added by
// the caller in wave order).  Ends with a barrier.
template <int DIN, int NOUT>
__device__ __forceinline__ void run_stack(float* lds, const Net& w, int head, float* part, int wave, int lane) {
    const float* __restrict__ W1 = w.W1 + (size_t)head * kH * DIN;
    const float* __restrict__ b1 = w.b1 + head * kH;
    const float* __restrict__ W2p = w.W2p + (size_t)head * kH * kH;
    const float* __restrict__ b2 = w.b2 + head * kH;
    const float* __restrict__ W3 = w.W3 + head * kH * NOUT;
    const int ln = opaque(lane);
    const int ct[2] = {2 * wave, 2 * wave + 1};
    float* act = lds + kOffAct;
    const float* xs = lds + kOffXs;
    const int k1 = ln >> 4;                                  // layer 1's K index of this lane; inputs past DIN count as 0
    // epilogue constants first: their latency hides behind the matrix work
    float b1v[2], b2v[2], w3v[NOUT][2], w1v[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int col = ct[c] * 16 + (ln & 15);
        b1v[c] = b1[col];
        b2v[c] = b2[col];
#pragma unroll
        for (int o = 0; o < NOUT; ++o) w3v[o][c] = W3[o * kH + col];
        const float wv = W1[col * DIN + (k1 < DIN ? k1 : 0)];  // B operand of layer 1: W1[col][k]
        w1v[c] = k1 < DIN ? wv : 0.f;
    }
    f32x4 acc[1][2];
    // layer 1: K = 4 inputs = ONE mfma per column tile
    const float xv = xs[(ln & 15) * 4 + k1];
    const float x = k1 < DIN ? xv : 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[0][c] = mfma(x, w1v[c], f32x4{0.f, 0.f, 0.f, 0.f});
    // act[row][col] = relu(acc + b1[col]); C layout: row = 4 (lane / 16) + i, col = 16 ct + lane % 16
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int col = ct[c] * 16 + (opaque(lane) & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i) act[(4 * (opaque(lane) >> 4) + i) * kActStride + col] = reluf(acc[0][c][i] + b1v[c]);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[0][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    layer_mma<1>(acc, act, W2p, ct, opaque(lane));
    // last layer folded in: out_o[row] = sum_col relu(h2 + b2) W3[o][col]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 2; ++c) s += reluf(acc[0][c][i] + b2v[c]) * w3v[o][c];
            const float v = reduce16(s);
            if ((ln & 15) == 0) part[(o * kWaves + wave) * kRows + 4 * (ln >> 4) + i] = v;
        }
    __syncthreads();       // act is free again; part complete
}

// b3 + the eight waves' partial sums of output o, in wave order
__device__ __forceinline__ float fold_part(const float* part, int o, int row, float b3) {
    float v = b3;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) v += part[(o * kWaves + w) * kRows + row];
    return v;
}

// The rollout's env traits over env_models.hpp: step(a, row, ctr, j, x, y, ax, ay) and reset(a, row, tick, x, y).
// Navigation 1 / 2: the kind is an argument of the launch, so the step draws its noise once and picks the kind's transition
struct NavRoll {
    __device__ __forceinline__ void reset(const EvArgs& a, long long row, uint64_t tick, double& x, double& y) const {
        const double2 p = rrl_env::NavEnv<0>::reset(a.seed, uint32_t(row), tick);     // one start state for both kinds
        x = p.x;
        y = p.y;
    }
    __device__ __forceinline__ Outcome step(const EvArgs& a, long long row, uint64_t ctr, int, double x, double y, float ax,
                                            float ay) const {
        const double2 e = rrl_env::nav_step_noise(a.seed, uint32_t(row), ctr), p = make_double2(x, y);
        double nx, ny, cost;
        const bool cons = a.kind == RRL_ENV_NAV1 ? rrl_env::NavEnv<0>::move(p, double(ax), double(ay), e.x, e.y, nx, ny, cost)
                                                 : rrl_env::NavEnv<1>::move(p, double(ax), double(ay), e.x, e.y, nx, ny, cost);
        return rrl_env::nav_outcome(nx, ny, cost, cons);
    }
};

// Maze (MazeVecEnv(auto_reset=False)): the env's own horizon is the block's
struct MazeRoll {
    int horizon;
    __device__ __forceinline__ void reset(const EvArgs& a, long long row, uint64_t tick, double& x, double& y) const {
        const double2 p = rrl_env::MazeEnv::reset(a.seed, uint32_t(row), tick);
        x = p.x;
        y = p.y;
    }
    __device__ __forceinline__ Outcome step(const EvArgs&, long long, uint64_t, int j, double x, double y, float ax,
                                            float ay) const {
        Outcome o = rrl_env::MazeEnv::step(make_double2(x, y), double(ax), double(ay));
        o.done = rrl_env::MazeEnv::timed_out(j + 1, horizon) | o.done;
        return o;
    }
};

// One pass of the candidate phase: candidates [base, base + 16 MR) of the k in LDS through the twin heads on [obs | candidate];
// q of the live ones into LDS (score_pass of qsample_kernels.hip on this file's carve-up)
template <int MR, class Tile>
__device__ __forceinline__ void qs_pass(float* lds, const Net& q, int k, int base, float ox, float oy, int tid, int wave,
                                        int lane) {
    constexpr int kOffQsCand = QsLds<Tile>::kOffCand, kOffQsQ = QsLds<Tile>::kOffQ;
    if (tid < rrl_tile::kRows) {
        const int r = base + tid;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};           // rows past k: finite inputs, results never read
        if (r < k) x = f32x4{ox, oy, lds[kOffQsCand + 2 * r], lds[kOffQsCand + 2 * r + 1]};
        *reinterpret_cast<f32x4*>(lds + Tile::kOffXs + tid * 4) = x;
    }
    __syncthreads();
    Tile::template q_phase<MR>(lds, q, wave, lane);
    if (tid < rrl_tile::kRows && base + tid < k) lds[kOffQsQ + base + tid] = Tile::twin_q(lds, q, tid).q;
    // xs and qpart are rewritten only behind the next pass's barriers
}

// The candidate phase of tile row g (env `grow`) at step counter ctr: k draws, their scores on Tile with the Q_risk group q,
// the argmin -> res[g] in LDS.  Every thread of the workgroup takes part; starts behind a barrier and ends with one.
template <class Tile>
__device__ __forceinline__ void qs_row(float* lds, const EvArgs& a, const Net& q, const QsArgs& s, int g, long long grow,
                                       uint64_t ctr, int tid, int wave, int lane) {
    constexpr int kOffQsCand = QsLds<Tile>::kOffCand, kOffQsQ = QsLds<Tile>::kOffQ, kOffQsObs = QsLds<Tile>::kOffObs,
                  kOffQsRes = QsLds<Tile>::kOffRes;
    const int k = s.k;
    // ---- candidates: a_j = float(lo_j + (hi_j - lo_j) u_j) in double, u = the open-unit pair of the row's 128 bits ----
#pragma unroll 1
    for (int c = tid; c < k; c += kThreads) {
        const rrl::Bits128 bits = rrl::philox_at(a.seed, uint32_t(grow * k + c), kStreamEvalQs, ctr);
        const double u[2] = {rrl::unit_open(bits.lo), rrl::unit_open(bits.hi)};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double l = double(s.lo[j]), h = double(s.hi[j]);
            lds[kOffQsCand + 2 * c + j] = float(l + (h - l) * u[j]);
        }
    }
    const float ox = lds[kOffQsObs + 2 * g], oy = lds[kOffQsObs + 2 * g + 1];
    __syncthreads();

    // ---- scores: row tiles of 16, at most four per pass ----
    const int nt = (k + 15) >> 4;
#pragma unroll 1
    for (int base = 0; base < k; base += rrl_tile::kRows) {
        const int mr = nt - (base >> 4);
        switch (mr) {
            case 1: qs_pass<1, Tile>(lds, q, k, base, ox, oy, tid, wave, lane); break;
            case 2: qs_pass<2, Tile>(lds, q, k, base, ox, oy, tid, wave, lane); break;
            case 3: qs_pass<3, Tile>(lds, q, k, base, ox, oy, tid, wave, lane); break;
            default: qs_pass<4, Tile>(lds, q, k, base, ox, oy, tid, wave, lane); break;
        }
    }
    __syncthreads();                              // q of every candidate is in LDS

    // ---- argmin, lowest index on ties; NaN counts as the smallest (torch.argmin) ----
    if (wave == 0) {
        float best = __builtin_inff();
        int bidx = kMaxK;
#pragma unroll 1
        for (int r = lane; r < k; r += 64) {      // ascending r: strict < keeps the lower index
            const float qv = lds[kOffQsQ + r];
            const float key = qv != qv ? -__builtin_inff() : qv;
            if (key < best) {
                best = key;
                bidx = r;
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
            bidx = bidx < k ? bidx : 0;           // every q = +inf cannot happen (q <= 1); keeps the reads below in range
            float* res = lds + kOffQsRes + 4 * g;
            res[0] = __int_as_float(bidx);
            res[1] = lds[kOffQsQ + bidx];
            res[2] = lds[kOffQsCand + 2 * bidx];
            res[3] = lds[kOffQsCand + 2 * bidx + 1];
        }
    }
    __syncthreads();                              // res[g] is out; candidates and q are free for the next gated row
}

// ---- SQRL: candidates, scores and picks of the tile's live rows (sqrl_kernels.hip's arithmetic, restated) ----

// Candidates of the `nl` live rows, flattened: f = slot k + c, slot-th live row g = rowof[slot].  a_c and logp_c are
// rrl_sqrl_act's tanh-Gaussian head (gauss_head_fwd_row of update_kernels.hip), in the same expression order.
template <class Tile>
__device__ __forceinline__ void sq_candidates(float* lds, const EvArgs& a, int k, int nl, unsigned b, uint64_t ctr, int tid) {
    constexpr int kOffSqCand = SqLds<Tile>::kOffCand, kOffSqLogp = SqLds<Tile>::kOffLogp, kOffSqHead = SqLds<Tile>::kOffHead,
                  kOffSqRow = SqLds<Tile>::kOffRow;
    const int total = nl * k;
#pragma unroll 1
    for (int f = tid; f < total; f += kThreads) {
        const int slot = f / k, c = f - slot * k;
        const int g = __float_as_int(lds[kOffSqRow + slot]);
        const long long grow = (long long)b * kRows + g;
        double d0, d1;
        rrl::normal_at(a.seed, uint32_t(grow * k + c), kStreamEvalSqrl, ctr, d0, d1);
        const float e2[2] = {float(d0), float(d1)};
        float lp = 0.f, act2[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float mean = lds[kOffSqHead + 4 * g + j];
            const float ls = fminf(fmaxf(lds[kOffSqHead + 4 * g + 2 + j], kLogSigMin), kLogSigMax);
            const float e = e2[j];
            const float y = tanhf(mean + expf(ls) * e);
            act2[j] = y * a.scale[j] + a.bias[j];
            lp += -0.5f * e * e - ls - kHalfLog2Pi - logf(a.scale[j] * (1.f - y * y) + kEps);
        }
        const int qi = g * kSqMaxK + c;
        lds[kOffSqCand + 2 * qi] = act2[0];
        lds[kOffSqCand + 2 * qi + 1] = act2[1];
        lds[kOffSqLogp + qi] = lp;
    }
}

// One pass: flattened candidates [f0, f0 + 16 MR) through the twin heads, every row with its own obs; q of the live ones
template <int MR, class Tile>
__device__ __forceinline__ void sq_pass(float* lds, const Net& q, int k, int total, int f0, int tid, int wave, int lane) {
    constexpr int kOffSqCand = SqLds<Tile>::kOffCand, kOffSqQ = SqLds<Tile>::kOffQ, kOffSqObs = SqLds<Tile>::kOffObs,
                  kOffSqRow = SqLds<Tile>::kOffRow;
    int qi = -1;
    if (tid < rrl_tile::kRows) {
        const int f = f0 + tid;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};           // rows past the last candidate: finite inputs, results never read
        if (f < total) {
            const int slot = f / k, c = f - slot * k;
            const int g = __float_as_int(lds[kOffSqRow + slot]);
            qi = g * kSqMaxK + c;
            x = f32x4{lds[kOffSqObs + 2 * g], lds[kOffSqObs + 2 * g + 1], lds[kOffSqCand + 2 * qi], lds[kOffSqCand + 2 * qi + 1]};
        }
        *reinterpret_cast<f32x4*>(lds + Tile::kOffXs + tid * 4) = x;
    }
    __syncthreads();
    Tile::template q_phase<MR>(lds, q, wave, lane);
    if (qi >= 0) lds[kOffSqQ + qi] = Tile::twin_q(lds, q, tid).q;
    // xs and qpart are rewritten only behind the next pass's barriers
}

// lane l's double, l wave-uniform
__device__ __forceinline__ double lane_double(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// The pick of tile row g (env `grow`) by ONE wave (sac.py:153-158; the position in the SAFE list is applied to the FULL list,
// as the reference does): rrl_sqrl_act's, with the double weights in registers (lane l holds candidates l and l + 64) read in
// ascending candidate order -- the same sums.  Leaves res[g].
template <class Tile>
__device__ __forceinline__ void sq_pick(float* lds, const EvArgs& a, int k, int g, long long grow, uint64_t ctr, int lane) {
    constexpr int kOffSqCand = SqLds<Tile>::kOffCand, kOffSqLogp = SqLds<Tile>::kOffLogp, kOffSqQ = SqLds<Tile>::kOffQ,
                  kOffSqRes = SqLds<Tile>::kOffRes;
    const float* qrow = lds + kOffSqQ + g * kSqMaxK;
    const float* lprow = lds + kOffSqLogp + g * kSqMaxK;
    float qv[2], lpv[2];
    bool safe[2];
    unsigned long long m[2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        const int c = lane + 64 * hf;
        const bool live = c < k;
        qv[hf] = live ? qrow[c] : 0.f;
        lpv[hf] = live ? lprow[c] : 0.f;
        safe[hf] = live && qv[hf] <= a.eps_safe;
        m[hf] = __ballot(safe[hf]);
    }
    // argmin of q, lowest index on ties; NaN counts as the smallest (torch.argmin)
    float best = __builtin_inff();
    int bidx = kSqMaxK;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        const int c = lane + 64 * hf;
        const float key = qv[hf] != qv[hf] ? -__builtin_inff() : qv[hf];
        if (c < k && key < best) {               // ascending c: strict < keeps the lower index
            best = key;
            bidx = c;
        }
    }
    float L = -__builtin_inff();                  // the largest safe logp
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
        if (safe[hf]) L = fmaxf(L, lpv[hf]);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bidx, off, 64);
        if (ob < best || (ob == best && oi < bidx)) {
            best = ob;
            bidx = oi;
        }
        L = fmaxf(L, __shfl_xor(L, off, 64));
    }
    double w[2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) w[hf] = safe[hf] ? exp(double(lpv[hf]) - double(L)) : 0.0;
    const int n_safe = __popcll(m[0]) + __popcll(m[1]);
    int pick = bidx < k ? bidx : 0, cs = -1;      // every q = +inf cannot happen (q <= 1); keeps the reads below in range
    if (n_safe > 0) {                             // wave-uniform; every lane runs the same scalar chain
        const unsigned long long m0 = m[0], m1 = m[1];
        const double u = rrl::unit_open(rrl::philox_at(a.seed, uint32_t(grow), kStreamEvalSqrlPick, ctr).lo);
        const int k0 = k < 64 ? k : 64;
        double T = 0.0;
#pragma unroll 1
        for (int c = 0; c < k0; ++c) T += lane_double(w[0], c);
#pragma unroll 1
        for (int c = 64; c < k; ++c) T += lane_double(w[1], c - 64);
        const double thr = u * T;
        double run = 0.0;
        int last = -1;
#pragma unroll 1
        for (int c = 0; c < k0; ++c) {
            const double wc = lane_double(w[0], c);
            if (!((m0 >> c) & 1ULL)) continue;
            last = c;
            run += wc;
            if (cs < 0 && run > thr) cs = c;
        }
#pragma unroll 1
        for (int c = 64; c < k; ++c) {
            const double wc = lane_double(w[1], c - 64);
            if (!((m1 >> (c - 64)) & 1ULL)) continue;
            last = c;
            run += wc;
            if (cs < 0 && run > thr) cs = c;
        }
        if (cs < 0) cs = last;
        // safe candidates with index <= c*, minus one
        const unsigned long long lo = cs < 64 ? (m0 & (~0ULL >> (63 - cs))) : m0;
        const unsigned long long hi = cs < 64 ? 0ULL : (m1 & (~0ULL >> (127 - cs)));
        pick = __popcll(lo) + __popcll(hi) - 1;
    }
    if (lane == 0) {
        float* res = lds + kOffSqRes + 8 * g;
        res[0] = __int_as_float(pick);
        res[1] = __int_as_float(cs);
        res[2] = __int_as_float(n_safe);
        res[3] = qrow[pick];
        res[4] = lds[kOffSqCand + 2 * (g * kSqMaxK + pick)];
        res[5] = lds[kOffSqCand + 2 * (g * kSqMaxK + pick) + 1];
    }
}

// The SQRL phase of one step: starts behind the fold of the policy's four outputs (head / obs of the tile's rows are in LDS
// behind the barrier in here), ends with res[g] of every live row g behind a barrier.  Every thread takes part.  The scores
// come from Tile with the Q_risk group q.
template <class Tile>
__device__ __forceinline__ void sq_phase(float* lds, const EvArgs& a, const Net& q, int k, unsigned b, uint64_t ctr, bool alive,
                                         int tid, int wave, int lane) {
    constexpr int kOffSqRow = SqLds<Tile>::kOffRow, kOffSqMask = SqLds<Tile>::kOffMask;
    const unsigned long long live = __ballot(alive);         // wave 0: bit t = row t; alive is false elsewhere
    if (alive) lds[kOffSqRow + __popcll(live & ((1ULL << tid) - 1ULL))] = __int_as_float(tid);
    if (tid == 0) lds[kOffSqMask] = __int_as_float(int(live));
    __syncthreads();                              // the policy's fold is behind this barrier: act / xs / part are free
    const unsigned m = __builtin_amdgcn_readfirstlane(__float_as_int(lds[kOffSqMask]));
    const int nl = __popc(m), total = nl * k;
    sq_candidates<Tile>(lds, a, k, nl, b, ctr, tid);
    __syncthreads();
    // ---- scores: the flattened candidates in row tiles of 16, at most four per pass ----
    const int nt = (total + 15) >> 4;
#pragma unroll 1
    for (int f0 = 0; f0 < total; f0 += rrl_tile::kRows) {
        const int mr = nt - (f0 >> 4);
        switch (mr) {
            case 1: sq_pass<1, Tile>(lds, q, k, total, f0, tid, wave, lane); break;
            case 2: sq_pass<2, Tile>(lds, q, k, total, f0, tid, wave, lane); break;
            case 3: sq_pass<3, Tile>(lds, q, k, total, f0, tid, wave, lane); break;
            default: sq_pass<4, Tile>(lds, q, k, total, f0, tid, wave, lane); break;
        }
    }
    __syncthreads();                              // q of every candidate is in LDS
    // ---- picks: wave w serves rows w and w + 8 ----
#pragma unroll 1
    for (int g = wave; g < kRows; g += kWaves)
        if ((m >> g) & 1u) sq_pick<Tile>(lds, a, k, g, (long long)b * kRows + g, ctr, lane);
    __syncthreads();                              // res is out
}

// Workgroup b of the argument block's own grid: envs [16 b, 16 (b + 1)) through the whole rollout.  Thread tid < 16
// owns env 16 b + tid: state and results in its registers, written once at the end.  Qs = QsOn: a gated live row executes
// the argmin of its k candidates (qs_row) in the place of a recovery policy's action.  The body declares no local for that
// form (the pick is read back from LDS where it is traced): with two more locals the NoQs instantiations kept their
// instruction counts but not their register numbering.  Qs = SqOn: no gate; every live row executes the pick of sq_phase.
template <class Env, class Qs = NoQs>
__device__ __forceinline__ void rollout_tile(const EvArgs& a, const Env& env, unsigned b, float* lds,
                                             const typename Qs::Args* qsp = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int R = kRows;
    const long long row = (long long)b * R + tid;
    const bool mine = tid < R && row < a.n;                  // rows >= n: finite inputs, nothing read back, nothing written
    const uint64_t tick = rrl::effective_counter(a.counter, a.counter_dev);
    const bool has_q = a.q.W1 != nullptr, has_r = a.r.W1 != nullptr;
    float* xs = lds + kOffXs;
    float* part = lds + kOffPart;

    double x = 0.0, y = 0.0;
    if (mine) {
        if (a.reset) {
            env.reset(a, row, tick, x, y);
        } else {
            x = a.pos[2 * row];
            y = a.pos[2 * row + 1];
        }
    }
    bool alive = mine, succ = false, viol = false;
    float ret = 0.f;
    int steps = 0;

#pragma unroll 1
    for (int j = 0; j < a.T; ++j) {
        if (tid < kRows) *reinterpret_cast<f32x4*>(xs + tid * 4) = f32x4{float(x), float(y), 0.f, 0.f};
        if (!__syncthreads_or(int(alive))) break;            // every row of the tile has finished its episode
        const uint64_t ctr = tick + uint64_t(a.reset) + uint64_t(j);

        // ---- task action: the Gaussian policy's mean rows ----
        if constexpr (Qs::sqrl)
            run_stack<2, 4>(lds, a.p, 0, part, wave, lane);   // mean rows, then log_std rows
        else
            run_stack<2, 2>(lds, a.p, 0, part, wave, lane);
        float t0 = 0.f, t1 = 0.f;
        if (tid < R) {
            t0 = tanhf(fold_part(part, 0, tid, a.p.b3[0])) * a.scale[0] + a.bias[0];
            t1 = tanhf(fold_part(part, 1, tid, a.p.b3[1])) * a.scale[1] + a.bias[1];
            xs[tid * 4 + 2] = t0;
            xs[tid * 4 + 3] = t1;
        }
        float r0 = t0, r1 = t1, z0 = 0.f, z1 = 0.f, e0 = 0.f, e1 = 0.f;
        bool rec = false;
        if constexpr (Qs::sqrl) {
            // ---- SQRL: the head of every row, then candidates, scores and picks of the live ones ----
            using L = SqLds<typename Qs::Tile>;
            if (tid < R) {
#pragma unroll
                for (int o = 0; o < 4; ++o) lds[L::kOffHead + 4 * tid + o] = fold_part(part, o, tid, a.p.b3[o]);
                lds[L::kOffObs + 2 * tid] = float(x);
                lds[L::kOffObs + 2 * tid + 1] = float(y);
            }
            sq_phase<typename Qs::Tile>(lds, a, Qs::score_net(a, *qsp), qsp->k, b, ctr, alive, tid, wave, lane);
            if (alive) {
                r0 = lds[L::kOffRes + 8 * tid + 4];
                r1 = lds[L::kOffRes + 8 * tid + 5];
            }
        } else if (has_q) {
            // ---- the gate: twin Q_risk on [obs | task action] ----
            __syncthreads();                                  // xs complete
#pragma unroll 1
            for (int h = 0; h < 2; ++h) run_stack<4, 1>(lds, a.q, h, part + h * kWaves * kRows, wave, lane);
            if (tid < R) {
                z0 = fold_part(part, 0, tid, a.q.b3[0]);
                z1 = fold_part(part, 1, tid, a.q.b3[1]);
                rec = alive && rrl::recovery_gate(z0, z1, a.eps_safe);
            }
            // ---- recovery action, when a row of the tile asks for one (the fold above is behind this barrier) ----
            const bool any = has_r && __syncthreads_or(int(rec));
            if (any) run_stack<2, 2>(lds, a.r, 0, part, wave, lane);
            if (has_r && alive && (rec || a.tr_eps)) {
                double d0, d1;
                rrl::normal_at(a.seed, uint32_t(row), kStreamEval, ctr, d0, d1);
                e0 = float(d0);
                e1 = float(d1);
            }
            if (any && rec) {
                r0 = tanhf(fold_part(part, 0, tid, a.r.b3[0])) * a.rscale[0] + a.rbias[0] +
                     expf(fmaxf(a.rlog_std[0], a.min_log_std)) * e0;
                r1 = tanhf(fold_part(part, 1, tid, a.r.b3[1])) * a.rscale[1] + a.rbias[1] +
                     expf(fmaxf(a.rlog_std[1], a.min_log_std)) * e1;
            }
            if constexpr (Qs::on) {
                // ---- Q-sampling: the gated live rows of the tile, one after another in ascending row order ----
                using L = QsLds<typename Qs::Tile>;
                if (tid < R) {
                    lds[L::kOffObs + 2 * tid] = float(x);
                    lds[L::kOffObs + 2 * tid + 1] = float(y);
                }
                const unsigned long long fired = __ballot(rec);      // wave 0: bit t = row t; rec is false elsewhere
                if (tid == 0) lds[L::kOffMask] = __int_as_float(int(fired));
                __syncthreads();                              // the gate's fold is behind this barrier: act / xs / part are free
                unsigned m = __builtin_amdgcn_readfirstlane(__float_as_int(lds[L::kOffMask]));
#pragma unroll 1
                while (m) {                                   // workgroup-uniform; no gated row: the phase is skipped
                    const int g = __builtin_ctz(m);
                    m &= m - 1;
                    qs_row<typename Qs::Tile>(lds, a, Qs::score_net(a, *qsp), *qsp, g, (long long)b * R + g, ctr, tid, wave, lane);
                }
                if (rec) {
                    r0 = lds[L::kOffRes + 4 * tid + 2];
                    r1 = lds[L::kOffRes + 4 * tid + 3];
                }
            }
        }

        // ---- transition ----
        if (alive) {
            const long long o = (long long)j * a.n + row;
            const Outcome t = env.step(a, row, ctr, j, x, y, r0, r1);
            const bool cons = t.constraint, sc = t.success, dn = t.done;
            const float rew = t.reward;
            if (a.tr_pos) {
                a.tr_pos[2 * o] = x;
                a.tr_pos[2 * o + 1] = y;
            }
            if (a.tr_task) {
                a.tr_task[2 * o] = t0;
                a.tr_task[2 * o + 1] = t1;
            }
            if (a.tr_real) {
                a.tr_real[2 * o] = r0;
                a.tr_real[2 * o + 1] = r1;
            }
            if constexpr (!Qs::sqrl)
                if (a.tr_z && has_q) {
                    a.tr_z[(long long)(2 * j) * a.n + row] = z0;
                    a.tr_z[(long long)(2 * j + 1) * a.n + row] = z1;
                }
            if (a.tr_eps && has_r) {
                a.tr_eps[2 * o] = e0;
                a.tr_eps[2 * o + 1] = e1;
            }
            if constexpr (Qs::on) {
                // res[tid] of this step stands until the next step's candidate phase, behind that step's barriers
                using L = QsLds<typename Qs::Tile>;
                if (rec && qsp->tr_pick) qsp->tr_pick[o] = __float_as_int(lds[L::kOffRes + 4 * tid]);
                if (rec && qsp->tr_q) qsp->tr_q[o] = lds[L::kOffRes + 4 * tid + 1];
            }
            if constexpr (Qs::sqrl) {
                // head / res[tid] of this step stand until the next step's phase, behind that step's barriers
                using L = SqLds<typename Qs::Tile>;
                if (qsp->tr_head)
#pragma unroll
                    for (int c = 0; c < 4; ++c) qsp->tr_head[4 * o + c] = lds[L::kOffHead + 4 * tid + c];
                if (qsp->tr_pick) qsp->tr_pick[o] = __float_as_int(lds[L::kOffRes + 8 * tid]);
                if (qsp->tr_cstar) qsp->tr_cstar[o] = __float_as_int(lds[L::kOffRes + 8 * tid + 1]);
                if (qsp->tr_nsafe) qsp->tr_nsafe[o] = __float_as_int(lds[L::kOffRes + 8 * tid + 2]);
                if (qsp->tr_q) qsp->tr_q[o] = lds[L::kOffRes + 8 * tid + 3];
            }
            if (a.tr_reward) a.tr_reward[o] = rew;
            if (a.tr_flags) a.tr_flags[o] = uint8_t(1 | (int(dn) << 1) | (int(cons) << 2) | (int(sc) << 3) | (int(rec) << 4));
            ret += rew;
            succ |= sc;
            viol |= cons;
            ++steps;
            x = t.x;
            y = t.y;
            alive = !dn;
        }
    }
    if (mine) {
        a.ret[row] = ret;
        a.success[row] = uint8_t(succ);
        a.violation[row] = uint8_t(viol);
        a.steps[row] = steps;
    }
    rrl::advance_counter_blocks(a.counter_dev, uint64_t(a.T) + uint64_t(a.reset), unsigned(a.blocks));
}

// ---- the kernels: one solo and one packed template over (Env, Form) ----

// The argument block of a launch: EvArgs, the form's group, the Maze horizon (the tail, unused by Navigation: one layout for
// both env kinds of a candidate form).  The solo kernel takes one as its argument, a packed plan holds S of them.  The base
// form has no group, and its Navigation block is EvArgs alone.
template <class Env, class Form>
struct Block {
    EvArgs a;
    typename Form::Args g;
    int horizon;
};
template <>
struct Block<NavRoll, NoQs> {
    EvArgs a;
};
template <>
struct Block<MazeRoll, NoQs> {
    EvArgs a;
    int horizon;
};

template <class Env, class Form>
__device__ __forceinline__ Env env_of(const Block<Env, Form>& k) {
    if constexpr (std::is_same<Env, MazeRoll>::value)
        return MazeRoll{k.horizon};
    else
        return NavRoll{};
}
template <class Env, class Form>
__device__ __forceinline__ const typename Form::Args* group_of(const Block<Env, Form>& k) {
    if constexpr (kHasGroup<Form>)
        return &k.g;
    else
        return nullptr;
}

// The copied argument block's pointers as global ones (pack.hpp: to_global)
__device__ __forceinline__ void globalize(Net& w) { rrl_pack::to_global_all(w.W1, w.b1, w.W2p, w.b2, w.W3, w.b3); }
__device__ __forceinline__ void globalize(EvArgs& a) {
    globalize(a.p);
    globalize(a.q);
    globalize(a.r);
    rrl_pack::to_global_all(a.pos, a.scale, a.bias, a.rscale, a.rbias, a.rlog_std, a.counter_dev, a.ret, a.success, a.violation,
                            a.steps, a.tr_pos, a.tr_task, a.tr_real, a.tr_z, a.tr_eps, a.tr_reward, a.tr_flags);
}

// Workgroup blockIdx.x of the block's own grid.  The kernel's arguments are the block's parts: the block as one argument,
// but EvArgs and the horizon as two for the base Maze form (launch_block) -- read out of one by-value struct, that
// kernel's horizon load is scheduled elsewhere.
template <class Env, class Form, class... Part>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(Form::kWavesPerEu, Form::kWavesPerEu)))
void eval_rollout_kernel(const Part... part) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Block<Env, Form> k{part...};
    rollout_tile<Env, Form>(k.a, env_of(k), blockIdx.x, lds, group_of(k));
}

// S evaluations side by side (pack.hpp): workgroup b serves tile `local` of seed s's own grid, on seed s's argument block.
// A padding workgroup of a pinned mapping leaves before it touches anything.
template <class Env, class Form>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(Form::kWavesPerEu, Form::kWavesPerEu)))
void eval_rollout_pack_kernel(const Block<Env, Form>* __restrict__ blocks, rrl_pack::Idx ix) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int s, local;
    if (!rrl_pack::locate(ix, blockIdx.x, s, local)) return;
    Block<Env, Form> k = blocks[s];
    globalize(k.a);
    if constexpr (kHasGroup<Form>) Form::globalize(k.g);
    rollout_tile<Env, Form>(k.a, env_of(k), unsigned(local), lds, group_of(k));
}

// ---- the host path: one for the twelve entries ----
// An entry is a form and what rides beside the descriptor, per seed (Side): nothing, the Maze horizon of the base form
// (rrl_eval_rollout_maze) or the rrl_w2_pack_f16x3 stream of an f16x3 form.

struct None {};
constexpr None kNoSides[rrl_pack::kMaxSeeds] = {};           // the packed entries' side array, where nothing rides

template <size_t N>
int given(const void* const (&p)[N]) {
    int k = 0;
    for (const void* q : p) k += q != nullptr;
    return k;
}

constexpr int kMaxHorizon = 1 << 30;
int check_horizon(int horizon) { return horizon < 1 || horizon > kMaxHorizon ? RRL_ERANGE : RRL_OK; }

// The env family of a launch.  A candidate descriptor names it (and carries the Maze horizon); a base entry fixes it -- the
// Maze one is the one with a horizon beside the descriptor -- and check_desc holds the descriptor to it.
template <class Desc, class Side>
bool is_maze(const Desc* p, Side) {
    if constexpr (std::is_same<Desc, rrl_eval_rollout_t>::value)
        return std::is_same<Side, int>::value;
    else
        return p->base.env_kind == RRL_ENV_MAZE;
}
template <class Desc, class Side>
int horizon_of(const Desc* p, Side side) {
    if constexpr (std::is_same<Side, int>::value)
        return side;
    else if constexpr (std::is_same<Desc, rrl_eval_rollout_t>::value)
        return 0;                                            // a base Navigation entry: never asked
    else
        return p->horizon;
}
const rrl_eval_rollout_t* base_of(const rrl_eval_rollout_t* p) { return p; }
template <class Desc>
const rrl_eval_rollout_t* base_of(const Desc* p) { return &p->base; }

// the checks of a descriptor, before any launch (rrl_hip.h); maze: the entry's env is Maze, else Navigation 1 / 2
int check_desc(const rrl_eval_rollout_t* p, bool maze = false) {
    if (!p) return RRL_EINVAL;
    const void* const need[] = {p->pW1, p->pb1, p->pW2p, p->pb2, p->pW3, p->pb3, p->scale, p->bias,
                                p->ret, p->success, p->violation, p->steps};
    const void* const qg[] = {p->qW1, p->qb1, p->qW2p, p->qb2, p->qW3, p->qb3};
    const void* const rg[] = {p->rW1, p->rb1, p->rW2p, p->rb2, p->rW3, p->rb3, p->rscale, p->rbias, p->rlog_std};
    const int nq = given(qg), nr = given(rg);
    const auto aligned = [](const void* w) { return (reinterpret_cast<uintptr_t>(w) & 15) == 0; };
    if (given(need) != 12 || (nq != 0 && nq != 6) || (nr != 0 && nr != 9) || (nr && !nq) || p->H != kH || p->d_obs != 2 ||
        p->d_act != 2 || p->n <= 0 || !(maze ? p->env_kind == RRL_ENV_MAZE : (p->env_kind == RRL_ENV_NAV1 || p->env_kind == RRL_ENV_NAV2)) ||
        !aligned(p->pW2p) ||
        !aligned(p->qW2p) || !aligned(p->rW2p) || (!p->reset && !p->pos))
        return RRL_EINVAL;
    if (p->T < 1 || p->T > kMaxT || p->n > kMaxN) return RRL_ERANGE;
    return RRL_OK;
}

// the checks of a candidate form's descriptor: the base's for its env kind, then its own fields (Q-sampling: the box; the
// k limit is the form's); an invalid field wins over a size out of range
template <class Form>
int check_group(const typename Form::Desc* p) {
    if (!p) return RRL_EINVAL;
    const rrl_eval_rollout_t* e = &p->base;
    const bool maze = is_maze(p, None{});
    const int rc = check_desc(e, maze);
    if (rc == RRL_EINVAL) return rc;
    const void* const rg[] = {e->rW1, e->rb1, e->rW2p, e->rb2, e->rW3, e->rb3, e->rscale, e->rbias, e->rlog_std};
    if (!e->qW1 || given(rg) != 0) return RRL_EINVAL;        // (a Q_risk group given in part: check_desc)
    if constexpr (Form::on)
        if (!p->lo || !p->hi) return RRL_EINVAL;
    if (rc != RRL_OK) return rc;
    constexpr int kmax = Form::sqrl ? kSqMaxK : kMaxK;
    if (p->k < 1 || p->k > kmax || (long long)e->n * p->k >= (1LL << 32)) return RRL_ERANGE;
    return maze ? check_horizon(p->horizon) : RRL_OK;
}

// rc of the descriptor's checks; a NULL or misaligned stream is an invalid field, so it wins over a size out of range
int check_w2h(int rc, const float* w2h) {
    if (rc == RRL_EINVAL) return rc;
    if (!w2h || (reinterpret_cast<uintptr_t>(w2h) & 15) != 0) return RRL_EINVAL;
    return rc;
}

// every check of one seed: the descriptor's, then what rides beside it
template <class Form, class Side>
int check(const typename Form::Desc* p, Side side) {
    int rc;
    if constexpr (kHasGroup<Form>)
        rc = check_group<Form>(p);
    else
        rc = check_desc(p, is_maze(p, side));
    if constexpr (std::is_same<Side, int>::value)
        return rc != RRL_OK ? rc : check_horizon(side);
    else if constexpr (std::is_same<Side, const float*>::value)
        return check_w2h(rc, side);
    else
        return rc;
}

EvArgs block_of(const rrl_eval_rollout_t* p) {
    EvArgs a{};
    a.n = p->n;
    a.T = p->T;
    a.kind = p->env_kind;
    a.reset = p->reset ? 1 : 0;
    a.blocks = (p->n + kRows - 1) / kRows;
    a.pos = p->pos;
    a.p = Net{p->pW1, p->pb1, p->pW2p, p->pb2, p->pW3, p->pb3};
    a.scale = p->scale;
    a.bias = p->bias;
    a.q = Net{p->qW1, p->qb1, p->qW2p, p->qb2, p->qW3, p->qb3};
    a.eps_safe = p->eps_safe;
    a.r = Net{p->rW1, p->rb1, p->rW2p, p->rb2, p->rW3, p->rb3};
    a.rscale = p->rscale;
    a.rbias = p->rbias;
    a.rlog_std = p->rlog_std;
    a.min_log_std = p->min_log_std;
    a.seed = p->seed;
    a.counter = p->counter;
    a.counter_dev = p->counter_dev;
    a.ret = p->ret;
    a.success = p->success;
    a.violation = p->violation;
    a.steps = p->steps;
    a.tr_pos = p->tr_pos;
    a.tr_task = p->tr_task;
    a.tr_real = p->tr_real;
    a.tr_z = p->tr_z;
    a.tr_eps = p->tr_eps;
    a.tr_reward = p->tr_reward;
    a.tr_flags = p->tr_flags;
    return a;
}

void fill(QsArgs& g, const rrl_eval_rollout_qs_t* p) {
    g.k = p->k;
    g.lo = p->lo;
    g.hi = p->hi;
    g.tr_pick = p->tr_pick;
    g.tr_q = p->tr_q;
}
void fill(SqArgs& g, const rrl_eval_rollout_sqrl_t* p) {
    g.k = p->k;
    g.tr_head = p->tr_head;
    g.tr_pick = p->tr_pick;
    g.tr_cstar = p->tr_cstar;
    g.tr_nsafe = p->tr_nsafe;
    g.tr_q = p->tr_q;
}

template <class Env, class Form, class Side>
Block<Env, Form> block_of(const typename Form::Desc* p, Side side) {
    Block<Env, Form> b{};
    b.a = block_of(base_of(p));
    if constexpr (kHasGroup<Form>) fill(b.g, p);
    if constexpr (std::is_same<Side, const float*>::value) b.g.w2h = side;
    if constexpr (std::is_same<Env, MazeRoll>::value) b.horizon = horizon_of(p, side);
    return b;
}

// One launch of a form's kernel.  > 64 KB of dynamic LDS is granted once per kernel: `granted` is the flag of the caller's
// own (Env, Form) instantiation.
template <class Form, class Kernel, class... Arg>
int launch(Kernel kernel, bool& granted, int grid, void* stream, const Arg&... arg) {
    if (Form::kLds > 64 * 1024) {
        const int rl = grant_lds(kernel, Form::kLds, granted);
        if (rl != RRL_OK) return rl;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kThreads), Form::kLds, (hipStream_t)stream, arg...);
    return check_launch();
}

template <class Env, class Form>
int launch_block(const Block<Env, Form>& b, void* stream) {
    static bool granted = false;
    if constexpr (std::is_same<Block<Env, Form>, Block<MazeRoll, NoQs>>::value)
        return launch<Form>(eval_rollout_kernel<Env, Form, EvArgs, int>, granted, b.a.blocks, stream, b.a, b.horizon);
    else
        return launch<Form>(eval_rollout_kernel<Env, Form, Block<Env, Form>>, granted, b.a.blocks, stream, b);
}

template <class Form, class Side>
int launch_solo(const typename Form::Desc* p, Side side, void* stream) {
    const int rc = check<Form>(p, side);
    if (rc != RRL_OK) return rc;
    return is_maze(p, side) ? launch_block(block_of<MazeRoll, Form>(p, side), stream)
                            : launch_block(block_of<NavRoll, Form>(p, side), stream);
}

// The packed entries check every seed before anything is stored or launched, and an invalid field (RRL_EINVAL) wins over
// a size out of range (RRL_ERANGE), whichever seed has it: RRL_EINVAL at once, else the last seed's failure, else RRL_OK
template <class Check>
int check_seeds(int S, Check check) {
    int worst = RRL_OK;
    for (int s = 0; s < S; ++s) {
        const int rc = check(s);
        if (rc == RRL_EINVAL) return rc;
        if (rc != RRL_OK) worst = rc;
    }
    return worst;
}

// ... and launch alike (pack.hpp): `key` holds the entry's input; on a miss every seed's argument block is built and placed
// by its tiles (<= 2^18 workgroups per seed: any mapping's grid fits an int)
template <class Env, class Form, class Side>
int launch_plan(const rrl_pack::Key& key, int S, const typename Form::Desc* args, const Side* sides, void* stream) {
    static bool granted = false;
    const rrl_pack::Plan* plan = rrl_pack::lookup(key);
    if (!plan) {
        std::vector<Block<Env, Form>> blocks(S);
        int count[rrl_pack::kMaxSeeds];
        for (int s = 0; s < S; ++s) count[s] = (blocks[s] = block_of<Env, Form>(args + s, sides[s])).a.blocks;
        plan = rrl_pack::publish(key, blocks, rrl_pack::place(S, count), (hipStream_t)stream);
        if (!plan) return rrl_pack::store_error();
    }
    return launch<Form>(eval_rollout_pack_kernel<Env, Form>, granted, plan->grid, stream, (const Block<Env, Form>*)plan->dev,
                        plan->ix);
}

template <class Form, class Side>
int launch_packed(rrl_pack::Site site, int S, const typename Form::Desc* args, const Side* sides, void* stream) {
    if (!args || !sides) return RRL_EINVAL;
    if (S <= 0 || S > rrl_pack::kMaxSeeds) return RRL_ERANGE;
    const int worst = check_seeds(S, [&](int s) { return check<Form>(args + s, sides[s]); });
    if (worst == RRL_EINVAL) return worst;
    const bool maze = is_maze(args, sides[0]);
    if constexpr (kHasGroup<Form>)                           // (a base entry's env is the entry's own)
        for (int s = 1; s < S; ++s)
            if (is_maze(args + s, sides[s]) != maze) return RRL_EINVAL;   // one env family per launch: the kernels differ
    if (worst != RRL_OK) return worst;
    // one seed: the packed launch IS the solo launch (argument block in the kernel arguments, no plan)
    if (S == 1) return launch_solo<Form>(args, sides[0], stream);
    rrl_pack::Key key(site, S);
    key.add(args, sizeof(*args) * S);
    if constexpr (!std::is_same<Side, None>::value) key.add(sides, sizeof(Side) * S);
    return maze ? launch_plan<MazeRoll, Form>(key, S, args, sides, stream) : launch_plan<NavRoll, Form>(key, S, args, sides, stream);
}

using rrl_pack::Site;

}  // namespace

extern "C" {

int rrl_eval_rollout(const rrl_eval_rollout_t* p, void* stream) { return launch_solo<NoQs>(p, None{}, stream); }
int rrl_eval_rollout_packed(int S, const rrl_eval_rollout_t* args, void* stream) {
    return launch_packed<NoQs>(Site::EvalRollout, S, args, kNoSides, stream);
}
int rrl_eval_rollout_maze(const rrl_eval_rollout_t* p, int horizon, void* stream) { return launch_solo<NoQs>(p, horizon, stream); }
int rrl_eval_rollout_maze_packed(int S, const rrl_eval_rollout_t* args, const int* horizon, void* stream) {
    return launch_packed<NoQs>(Site::EvalRolloutMaze, S, args, horizon, stream);
}

int rrl_eval_rollout_qs(const rrl_eval_rollout_qs_t* p, void* stream) { return launch_solo<QsOn>(p, None{}, stream); }
int rrl_eval_rollout_qs_packed(int S, const rrl_eval_rollout_qs_t* args, void* stream) {
    return launch_packed<QsOn>(Site::EvalRolloutQs, S, args, kNoSides, stream);
}
int rrl_eval_rollout_sqrl(const rrl_eval_rollout_sqrl_t* p, void* stream) { return launch_solo<SqOn>(p, None{}, stream); }
int rrl_eval_rollout_sqrl_packed(int S, const rrl_eval_rollout_sqrl_t* args, void* stream) {
    return launch_packed<SqOn>(Site::EvalRolloutSqrl, S, args, kNoSides, stream);
}

int rrl_eval_rollout_qs_f16x3(const rrl_eval_rollout_qs_t* p, const float* qW2h, void* stream) {
    return launch_solo<QsOnH>(p, qW2h, stream);
}
int rrl_eval_rollout_qs_f16x3_packed(int S, const rrl_eval_rollout_qs_t* args, const float* const* qW2h, void* stream) {
    return launch_packed<QsOnH>(Site::EvalRolloutQsF16x3, S, args, qW2h, stream);
}
int rrl_eval_rollout_sqrl_f16x3(const rrl_eval_rollout_sqrl_t* p, const float* qW2h, void* stream) {
    return launch_solo<SqOnH>(p, qW2h, stream);
}
int rrl_eval_rollout_sqrl_f16x3_packed(int S, const rrl_eval_rollout_sqrl_t* args, const float* const* qW2h, void* stream) {
    return launch_packed<SqOnH>(Site::EvalRolloutSqrlF16x3, S, args, qW2h, stream);
}

}  // extern "C"

