// Independent multi-output Gaussian likelihood (reference: GaussianLikelihood, var_gp/likelihoods.py:66-110) in closed form:
//   v = var + exp(obs_log_var[c]),  r = y - mu,  n = S C
//   nll = sum_b mean_{s,c} [ 1/2 log(2 pi v) + 1/2 r^2 / v ]
// and its gradients.  A latency-bound pair of launches (Config 2: S C B = 15k elements); no workspace, no float atomics:
// every sum goes through a fixed-order per-thread stride loop and the block tree (block_sum), so the results are
// bitwise reproducible.
//   class workgroups (blockIdx.x < C, backward only): gmu, gvar of class c and g_obs_log_var[c] = exp(olv[c]) sum_{s,b} gvar
//   nll workgroup   (blockIdx.x == C in the backward, the only one in the forward): the scalar, over all classes
// The nll workgroup sums class by class (per thread at most ceil(S B / 1024) terms, then one add per class), so no thread
// carries a long serial sum.  Measured at Config 2 (S3 C10 B512, backward with the value): 11.0 us per launch, bound by
// the single nll workgroup's ~15k log evaluations on one CU.
#include "common.h"

namespace vargp {

constexpr int kGaussThreads = 1024;
constexpr float kHalfLog2Pi = 0.91893853320467274178f;

__global__ __launch_bounds__(kGaussThreads) void gauss_nll_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                                   const float* __restrict__ y, int64_t ldy,
                                                                   const float* __restrict__ obs_log_var,
                                                                   const float* __restrict__ seed, float* __restrict__ gmu,
                                                                   float* __restrict__ gvar, float* __restrict__ g_olv,
                                                                   float* __restrict__ nll, int S, int C, int B,
                                                                   int nclass_blocks) {
  __shared__ float red[kGaussThreads / kWave];
  const int SB = S * B;
  const int64_t CB = (int64_t)C * B;
  const float inv_n = 1.f / ((float)S * (float)C);
  if ((int)blockIdx.x < nclass_blocks) {
    // one class: element e = s * B + b of the class's (S, B) slab
    const int c = blockIdx.x;
    const float obs = expf(obs_log_var[c]);
    const float g = seed[0] * inv_n;
    const float* yc = y + (int64_t)c * ldy;
    float acc = 0.f;
    for (int e = threadIdx.x; e < SB; e += kGaussThreads) {
      const int s = e / B, b = e - s * B;
      const int64_t i = (int64_t)s * CB + (int64_t)c * B + b;
      const float v = var[i] + obs, iv = 1.f / v, r = yc[b] - mu[i], riv = r * iv;
      const float gv = 0.5f * g * (iv - riv * riv);
      gmu[i] = -g * riv;
      gvar[i] = gv;
      acc += gv;
    }
    acc = block_sum<kGaussThreads>(acc, red);
    if (threadIdx.x == 0) g_olv[c] = obs * acc;
    return;
  }
  float acc = 0.f;
  for (int c = 0; c < C; ++c) {
    const float obs = expf(obs_log_var[c]);
    const float* yc = y + (int64_t)c * ldy;
    float part = 0.f;
    for (int e = threadIdx.x; e < SB; e += kGaussThreads) {
      const int s = e / B, b = e - s * B;
      const int64_t i = (int64_t)s * CB + (int64_t)c * B + b;
      const float v = var[i] + obs, r = yc[b] - mu[i];
      part += kHalfLog2Pi + 0.5f * (logf(v) + r * r / v);
    }
    acc += part;
  }
  acc = block_sum<kGaussThreads>(acc, red);
  if (threadIdx.x == 0) nll[0] = acc * inv_n;
}

}  // namespace vargp

using namespace vargp;

extern "C" int vargp_gauss_nll_fwd(const float* mu, const float* var, const float* y, int64_t ldy, const float* obs_log_var,
                                   float* nll, int S, int C, int B, vargp_stream_t stream) {
  VARGP_REQUIRE(mu && var && y && obs_log_var && nll && S > 0 && C > 0 && B > 0 && (ldy == 0 || ldy >= B),
                "gauss_nll_fwd: bad arguments");
  VARGP_REQUIRE((int64_t)S * B <= INT32_MAX, "gauss_nll_fwd: S * B too large");
  hipLaunchKernelGGL(gauss_nll_kernel, dim3(1), dim3(kGaussThreads), 0, as_stream(stream), mu, var, y, ldy, obs_log_var,
                     nullptr, nullptr, nullptr, nullptr, nll, S, C, B, 0);
  return check_launch("gauss_nll_fwd");
}

extern "C" int vargp_gauss_nll_bwd(const float* mu, const float* var, const float* y, int64_t ldy, const float* obs_log_var,
                                   const float* seed, float* gmu, float* gvar, float* g_obs_log_var, float* nll, int S, int C,
                                   int B, vargp_stream_t stream) {
  VARGP_REQUIRE(mu && var && y && obs_log_var && seed && gmu && gvar && g_obs_log_var && S > 0 && C > 0 && B > 0 &&
                    (ldy == 0 || ldy >= B),
                "gauss_nll_bwd: bad arguments");
  VARGP_REQUIRE((int64_t)S * B <= INT32_MAX, "gauss_nll_bwd: S * B too large");
  const int nblk = C + (nll ? 1 : 0);
  hipLaunchKernelGGL(gauss_nll_kernel, dim3(nblk), dim3(kGaussThreads), 0, as_stream(stream), mu, var, y, ldy, obs_log_var,
                     seed, gmu, gvar, g_obs_log_var, nll, S, C, B, C);
  return check_launch("gauss_nll_bwd");
}
