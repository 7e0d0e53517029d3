// Independent-output Bernoulli likelihood (binary / multi-label / one-vs-rest classification).  Not in the reference.
//   p(t | f) = Lambda(s f), s = 2 t - 1, Lambda = Phi (probit, link 0) or the logistic function (logit, link 1)
// The expected log-likelihood under f ~ N(mu, var) is DEFINED by the 20-node Gauss-Hermite rule:
//   ell[s,c,b] = sum_k w^_k log Lambda(s_cb (mu + sqrt(2 var) x_k)),   nll = - sum_b sum_c mean_s ell
// and the gradients are the exact derivatives of that sum.  The nodes are symmetric, so they are visited in +-x_k pairs:
//   d ell / d mu  = s sum_{k>0} w^_k (g_k + g_-k),   d ell / d var = s sum_{k>0} w^_k x_k (g_k - g_-k) / sqrt(2 var)
// with g = (log Lambda)' -- the pair difference carries the whole variance gradient, which at small var would otherwise be
// the small remainder of twenty terms of either sign.
// Launch layout: a latency-bound launch (Config 2: S C B = 15k elements, 20 transcendental evaluations each), so the value is
// NOT summed by one workgroup as in gauss_lik.hip: workgroup (c, j) handles the elements e = j * 256 + tid (+ nsplit * 256 ...)
// of class c's (S, B) slab, writes gmu / gvar and leaves its partial value in partials[c * nsplit + j]; a second launch of one
// wavefront adds the partials in index order.  No float atomics anywhere: every sum has a fixed order, two runs are bitwise
// equal, and the backward's value equals the forward's bit for bit (contraction is switched off in the shared arithmetic so
// that the two instantiations round alike).
#include "common.h"

namespace vargp {

constexpr int kBernThreads = 256;
constexpr int kBernMaxSplit = 32;
constexpr int kGhPairs = 10;
// x, w = numpy.polynomial.hermite.hermgauss(20); the positive half x[10:] and w[10:] / sqrt(pi) (17 digits; fp32 keeps 9)
__device__ constexpr float kGhX[kGhPairs] = {0.24534070830090124f, 0.73747372854539439f, 1.2340762153953231f,
                                             1.7385377121165861f,  2.2549740020892757f,  2.7888060584281305f,
                                             3.3478545673832163f,  3.9447640401156252f,  4.6036824495507442f,
                                             5.3874808900112328f};
__device__ constexpr float kGhW[kGhPairs] = {0.26079306344955488f,    0.16173933398399998f,    0.061506372063976897f,
                                             0.013997837447101022f,   0.00183010313108049f,    0.00012882627996192928f,
                                             4.402121090230851e-06f,  6.127490259982928e-08f,  2.4820623623151755e-10f,
                                             1.2578006724379234e-13f};
constexpr float kInvSqrt2 = 0.70710678118654752440f;
constexpr float kInvSqrt2Pi = 0.39894228040143267794f;

// A link: eval(z, lp, dlp) = log Lambda(z) and its derivative; prob(z) = Lambda(z).
struct LinkProbit {
  // With a = |z| / sqrt2 and the scaled complementary error function erfcx(a) = exp(a^2) erfc(a) (finite and accurate for every
  // a >= 0):  z < 0:  Phi(z) = erfcx(a) exp(-a^2) / 2  ->  log Phi = log(erfcx(a) / 2) - a^2,  phi / Phi = sqrt(2 / pi) / erfcx(a)
  //           z >= 0: Phi(z) = 1 - q, q = erfcx(a) exp(-a^2) / 2  ->  log Phi = log1p(-q),     phi / Phi = exp(-a^2) / (sqrt(2 pi) (1 - q))
  template <bool GRAD>
  static __device__ __forceinline__ void eval(float z, float& lp, float& dlp) {
#pragma clang fp contract(off)
    const float a = fabsf(z) * kInvSqrt2, a2 = a * a, ex = erfcxf(a);
    if (z < 0.f) {
      lp = logf(0.5f * ex) - a2;
      if (GRAD) dlp = (2.f * kInvSqrt2Pi) / ex;
    } else {
      const float e = expf(-a2), q = 0.5f * ex * e;
      lp = log1pf(-q);
      if (GRAD) dlp = kInvSqrt2Pi * e / (1.f - q);
    }
  }
  static __device__ __forceinline__ float prob(float z) { return 0.5f * erfcf(-z * kInvSqrt2); }
};
struct LinkLogit {
  // log sigma(z) = -softplus(-z) = min(z, 0) - log1p(exp(-|z|));  (log sigma)' = sigma(-z)
  template <bool GRAD>
  static __device__ __forceinline__ void eval(float z, float& lp, float& dlp) {
#pragma clang fp contract(off)
    const float t = expf(-fabsf(z)), r = 1.f / (1.f + t);
    lp = fminf(z, 0.f) - log1pf(t);
    if (GRAD) dlp = z < 0.f ? r : t * r;
  }
  static __device__ __forceinline__ float prob(float z) {
    const float t = expf(-fabsf(z)), r = 1.f / (1.f + t);
    return z < 0.f ? t * r : r;
  }
};

// ell of one element and (GRAD) its derivatives with respect to mu and var; sgn = 2 t - 1
template <class LINK, bool GRAD>
__device__ __forceinline__ float bern_element(float mu, float var, float sgn, float& dmu, float& dvar) {
#pragma clang fp contract(off)
  const float sd = sqrtf(2.f * var);
  float ell = 0.f, am = 0.f, av = 0.f;
#pragma unroll
  for (int k = 0; k < kGhPairs; ++k) {
    const float d = sd * kGhX[k];
    float lp, gp = 0.f, lm, gm = 0.f;
    LINK::template eval<GRAD>(sgn * (mu + d), lp, gp);
    LINK::template eval<GRAD>(sgn * (mu - d), lm, gm);
    ell += kGhW[k] * (lp + lm);
    if (GRAD) {
      am += kGhW[k] * (gp + gm);
      av += (kGhW[k] * kGhX[k]) * (gp - gm);
    }
  }
  if (GRAD) {
    dmu = sgn * am;
    dvar = sgn * av / fmaxf(sd, 1e-30f);      // (var = 0: the pair differences are exactly 0, and so is the result)
  }
  return ell;
}

__device__ __forceinline__ float bern_sign(const float* __restrict__ t, int64_t ldt, const int64_t* __restrict__ labels, int c,
                                           int b) {
  // one-vs-rest labels: a label outside [0, C) matches no output (every output of that point is a negative)
  if (labels) return labels[b] == (int64_t)c ? 1.f : -1.f;
  return 2.f * t[(int64_t)c * ldt + b] - 1.f;
}

// grid (C, nsplit).  GRAD: gmu, gvar = seed[0] * d nll / d (mu, var).  partials (may be NULL): [C * nsplit] values of sum ell
template <class LINK, bool GRAD>
__global__ __launch_bounds__(kBernThreads) void bern_nll_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                                const float* __restrict__ t, int64_t ldt,
                                                                const int64_t* __restrict__ labels,
                                                                const float* __restrict__ seed, float* __restrict__ gmu,
                                                                float* __restrict__ gvar, float* __restrict__ partials, int S,
                                                                int C, int B) {
  __shared__ float red[kBernThreads / kWave];
  const int c = blockIdx.x, nsplit = gridDim.y;
  const int SB = S * B;
  const int64_t CB = (int64_t)C * B;
  const float g = GRAD ? -seed[0] / (float)S : 0.f;
  float acc = 0.f;
  for (int64_t e = (int64_t)blockIdx.y * kBernThreads + threadIdx.x; e < SB; e += (int64_t)nsplit * kBernThreads) {
    const int s = (int)(e / B), b = (int)(e - (int64_t)s * B);
    const int64_t i = (int64_t)s * CB + (int64_t)c * B + b;
    float dmu = 0.f, dvar = 0.f;
    acc += bern_element<LINK, GRAD>(mu[i], var[i], bern_sign(t, ldt, labels, c, b), dmu, dvar);
    if (GRAD) {
      gmu[i] = g * dmu;
      gvar[i] = g * dvar;
    }
  }
  if (partials) {
    acc = block_sum<kBernThreads>(acc, red);
    if (threadIdx.x == 0) partials[(int64_t)c * nsplit + blockIdx.y] = acc;
  }
}

// one wavefront: nll = -(1 / S) sum_i partials[i], lanes stride the array in index order, then the wave tree
__global__ __launch_bounds__(kWave) void bern_finish_kernel(const float* __restrict__ partials, int n, float inv_s,
                                                            float* __restrict__ nll) {
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += kWave) acc += partials[i];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) nll[0] = -inv_s * acc;
}

// grid over (c, b), b fastest: probs[b, c] = mean_s P(t = 1).  Probit: closed form Phi(mu / sqrt(1 + var)); logit: the rule
template <class LINK>
__global__ __launch_bounds__(kBernThreads) void bern_predict_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                                    float* __restrict__ probs, int S, int C, int B) {
  const int64_t CB = (int64_t)C * B;
  const int64_t j = (int64_t)blockIdx.x * kBernThreads + threadIdx.x;
  if (j >= CB) return;
  const int c = (int)(j / B), b = (int)(j - (int64_t)c * B);
  float acc = 0.f;
  for (int s = 0; s < S; ++s) {
    const float m = mu[(int64_t)s * CB + j], v = var[(int64_t)s * CB + j];
    if (std::is_same<LINK, LinkProbit>::value) {
      acc += LinkProbit::prob(m * rsqrtf(1.f + v));
    } else {
      const float sd = sqrtf(2.f * v);
      float p = 0.f;
#pragma unroll
      for (int k = 0; k < kGhPairs; ++k) p += kGhW[k] * (LINK::prob(m + sd * kGhX[k]) + LINK::prob(m - sd * kGhX[k]));
      acc += p;
    }
  }
  probs[(int64_t)b * C + c] = acc / (float)S;
}

static int bern_nsplit(int S, int B) {
  const int n = cdiv((int64_t)S * B, kBernThreads);
  return n < kBernMaxSplit ? n : kBernMaxSplit;
}

template <bool GRAD>
static int bern_launch(const char* what, const float* mu, const float* var, const float* t, int64_t ldt, const int64_t* labels,
                       int link, const float* seed, float* gmu, float* gvar, float* nll, int S, int C, int B, float* ws,
                       size_t ws_bytes, hipStream_t st) {
  const int nsplit = bern_nsplit(S, B);
  float* partials = nll ? ws : nullptr;
  const dim3 grid(C, nsplit), block(kBernThreads);
  if (link == 0)
    hipLaunchKernelGGL((bern_nll_kernel<LinkProbit, GRAD>), grid, block, 0, st, mu, var, t, ldt, labels, seed, gmu, gvar,
                       partials, S, C, B);
  else
    hipLaunchKernelGGL((bern_nll_kernel<LinkLogit, GRAD>), grid, block, 0, st, mu, var, t, ldt, labels, seed, gmu, gvar,
                       partials, S, C, B);
  if (nll) hipLaunchKernelGGL(bern_finish_kernel, dim3(1), dim3(kWave), 0, st, partials, C * nsplit, 1.f / (float)S, nll);
  return check_launch(what);
}

}  // namespace vargp

using namespace vargp;

#define BERN_CHECK_COMMON(what)                                                                                          \
  VARGP_REQUIRE(mu && var && S > 0 && C > 0 && B > 0, what ": bad arguments");                                          \
  VARGP_REQUIRE(link == 0 || link == 1, what ": link must be 0 (probit) or 1 (logit)");                                \
  VARGP_REQUIRE((int64_t)S * B <= INT32_MAX, what ": S * B too large")
#define BERN_CHECK_TARGET(what)                                                                                          \
  VARGP_REQUIRE((t != nullptr) != (labels != nullptr), what ": exactly one of t and labels");                           \
  VARGP_REQUIRE(labels || ldt == 0 || ldt >= B, what ": ldt must be 0 or >= B");                                        \
  VARGP_REQUIRE((int64_t)C * kBernMaxSplit <= INT32_MAX, what ": C too large")

extern "C" size_t vargp_bernoulli_workspace_bytes(int S, int C, int B) {
  if (S <= 0 || C <= 0 || B <= 0) return 0;
  return (size_t)C * bern_nsplit(S, B) * sizeof(float);
}

extern "C" int vargp_bernoulli_nll_fwd(const float* mu, const float* var, const float* t, int64_t ldt, const int64_t* labels,
                                       int link, float* nll, int S, int C, int B, float* ws, size_t ws_bytes,
                                       vargp_stream_t stream) {
  BERN_CHECK_COMMON("bernoulli_nll_fwd");
  BERN_CHECK_TARGET("bernoulli_nll_fwd");
  VARGP_REQUIRE(nll && ws && ws_bytes >= vargp_bernoulli_workspace_bytes(S, C, B), "bernoulli_nll_fwd: nll / workspace");
  return bern_launch<false>("bernoulli_nll_fwd", mu, var, t, ldt, labels, link, nullptr, nullptr, nullptr, nll, S, C, B, ws,
                            ws_bytes, as_stream(stream));
}

extern "C" int vargp_bernoulli_nll_bwd(const float* mu, const float* var, const float* t, int64_t ldt, const int64_t* labels,
                                       int link, const float* seed, float* gmu, float* gvar, float* nll, int S, int C, int B,
                                       float* ws, size_t ws_bytes, vargp_stream_t stream) {
  BERN_CHECK_COMMON("bernoulli_nll_bwd");
  BERN_CHECK_TARGET("bernoulli_nll_bwd");
  VARGP_REQUIRE(seed && gmu && gvar, "bernoulli_nll_bwd: bad arguments");
  VARGP_REQUIRE(!nll || (ws && ws_bytes >= vargp_bernoulli_workspace_bytes(S, C, B)), "bernoulli_nll_bwd: workspace too small");
  return bern_launch<true>("bernoulli_nll_bwd", mu, var, t, ldt, labels, link, seed, gmu, gvar, nll, S, C, B, ws, ws_bytes,
                           as_stream(stream));
}

extern "C" int vargp_bernoulli_predict(const float* mu, const float* var, int link, float* probs, int S, int C, int B,
                                       vargp_stream_t stream) {
  BERN_CHECK_COMMON("bernoulli_predict");
  VARGP_REQUIRE(probs && (int64_t)C * B <= (int64_t)INT32_MAX * kBernThreads, "bernoulli_predict: bad arguments");
  const dim3 grid(cdiv((int64_t)C * B, kBernThreads)), block(kBernThreads);
  if (link == 0)
    hipLaunchKernelGGL(bern_predict_kernel<LinkProbit>, grid, block, 0, as_stream(stream), mu, var, probs, S, C, B);
  else
    hipLaunchKernelGGL(bern_predict_kernel<LinkLogit>, grid, block, 0, as_stream(stream), mu, var, probs, S, C, B);
  return check_launch("bernoulli_predict");
}
