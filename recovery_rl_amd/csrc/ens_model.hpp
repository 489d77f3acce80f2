// ens_model.hpp -- what the two training entries of the PETS dynamics ensemble share (ens_train_kernels.hip: batch <= 32, one
// launch; ens_train_big_kernels.hip: the large-batch re-fit): the reference's shape, swish, a member's parameters, the
// bootstrap gather (config/navigation1.py:72), the Gaussian NLL with its softplus log-variance bounds (MPC.py:276-287), and
// the entries' host checks and epoch loop.  Tiling, LDS layouts, reductions and launch geometry stay with the kernels.
// plan_kernels.hip's ensemble forward is not this one (v_rcp_f32 / __expf on purpose).  Device code is forced inline.
#pragma once

#include "rrl_host.hpp"

namespace rrl_ens {

// 4 inputs (obs 2 + action 2) -> 3 x 200 swish -> 4 outputs (mean 2, logvar 2); 4 bound sums + 60 losses = 64 reduction threads
constexpr int kH = 200, kDin = 4, kDout = 4, kMaxNets = 60;
constexpr float kLogvarReg = 0.01f;      // 0.01 (sum max_logvar - sum min_logvar) in the loss, MPC.py:271

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }   // F.softplus
__device__ __forceinline__ float softplus_grad(float x) { return x > 20.f ? 1.f : sigm(x); }

// h = swish(pre) and dh = d swish / d pre from one sigmoid
__device__ __forceinline__ void swish(float pre, float& h, float& dh) {
    const float sg = sigm(pre);
    h = pre * sg;
    dh = sg * (1.f + pre * (1.f - sg));
}

// member e's parameters; weight layout [net][in][out] (torch.baddbmm(b, x, w))
struct Member { const float *w0, *b0, *w1, *b1, *w2, *b2, *w3, *b3; };
__device__ __forceinline__ Member member_of(const rrl_ens_t& m, int e) {
    return {m.w0 + (size_t)e * kDin * kH, m.b0 + (size_t)e * kH, m.w1 + (size_t)e * kH * kH,    m.b1 + (size_t)e * kH,
            m.w2 + (size_t)e * kH * kH,   m.b2 + (size_t)e * kH, m.w3 + (size_t)e * kH * kDout, m.b3 + (size_t)e * kDout};
}

// One thread's share of the bootstrap gather: input column k of the dataset row *idx_row names, standardised, and for k < 2
// its target.  A dead row (past the member's batch) reads no index and contributes zeros.
__device__ __forceinline__ void gather(const rrl_ens_t& m, const float* train_in, const float* train_targ,
                                       const int64_t* idx_row, bool live, int k, float* xin_slot, float* yt_slot) {
    const int64_t row = live ? *idx_row : 0;
    *xin_slot = live ? (train_in[row * kDin + k] - m.mu[k]) / m.sigma[k] : 0.f;
    if (k < 2) *yt_slot = live ? train_targ[row * 2 + k] : 0.f;
}

// The loss of one (row, output dim), tl = (mean - targ)^2 exp(-lv) + lv with lv0 held below max_logvar and above min_logvar
// by softplus, and its gradient w.r.t. the two outputs and the two bounds under the mean over n2 = 2 x (real rows) terms.
// live = 1.f for a real row, 0.f for padding.
struct NllTerm { float tl, d_mean, d_lv, d_max, d_min; };
template <class Int>
__device__ __forceinline__ NllTerm nll(float mx, float mn, float mean, float lv0, float targ, float live, Int n2) {
    const float a1 = mx - lv0, lv1 = mx - softplus(a1);
    const float a2 = lv1 - mn, lv2 = mn + softplus(a2);
    const float inv = expf(-lv2), diff = mean - targ;
    const float scale = live / float(n2);                    // mean over the real rows and the two dims
    const float d_lv2 = (1.f - diff * diff * inv) * scale;
    const float s2 = softplus_grad(a2), d_lv1 = d_lv2 * s2;
    const float s1 = softplus_grad(a1);
    return {(diff * diff * inv + lv2) * live, 2.f * diff * inv * scale, d_lv1 * s1, d_lv1 * (1.f - s1), d_lv2 * (1.f - s2)};
}

// ---- host: every pointer an entry hands to its kernels (second_halves: the small entry's g2_* and partials) ----
inline bool desc_complete(const rrl_ens_t* m, bool second_halves) {
    return m && m->n_nets >= 1 && m->n_nets <= kMaxNets && m->w0 && m->b0 && m->w1 && m->b1 && m->w2 && m->b2 && m->w3 &&
           m->b3 && m->max_logvar && m->min_logvar && m->mu && m->sigma && m->g_w0 && m->g_b0 && m->g_w1 && m->g_b1 &&
           m->g_w2 && m->g_b2 && m->g_w3 && m->g_b3 && m->g_max_logvar && m->g_min_logvar &&
           (!second_halves || (m->g2_w0 && m->g2_b0 && m->g2_w1 && m->g2_b1 && m->g2_w2 && m->g2_b2 && m->g2_w3 &&
                               m->g2_b3 && m->g_logvar_part && m->loss_part));
}

// One epoch of MPC.train's batch loop (MPC.py:266-292) issued from C: ceil(n_rows / batch) x {grad(rows of this step, its
// index columns), Adam}.  ~4 us of host time per launch instead of ~20 us through Python: the 35-us small step stays GPU-bound.
template <class Int, class Grad>
int train_epoch(int n_seg, const rrl_adam_seg_t* segs, float lr, float beta1, float beta2, float eps, const int64_t* idx,
                long long n_rows, Int batch, void* stream, Grad grad) {
    if (!idx || n_rows <= 0 || batch <= 0 || !segs) return RRL_EINVAL;
    for (long long lo = 0; lo < n_rows; lo += batch) {
        int rc = grad(Int(n_rows - lo < batch ? n_rows - lo : batch), idx + lo);
        if (rc == RRL_OK) rc = rrl_adam_step_multi(n_seg, segs, lr, beta1, beta2, eps, stream);
        if (rc != RRL_OK) return rc;
    }
    return RRL_OK;
}

}  // namespace rrl_ens
