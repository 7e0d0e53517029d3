// The ELBO term of the likelihoods with independent outputs -- Bernoulli (probit / logit), Poisson, Student-t (lik.h; none is
// in the reference) -- on one launch frame:  nll = - sum_b sum_c mean_s ell[s,c,b]  and its seeded gradients.
// mu, var [S, C, B]; the values SUM over the outputs and take the mean over the hyper-samples: the ELBO of C independent outputs.
// That is C times the convention of gauss_lik.hip, which keeps the reference's mean over outputs.
// Launch layout: a latency-bound launch (Config 2: S C B = 15k elements, up to 20 transcendental evaluations each), so the value
// is NOT summed by one workgroup as in gauss_lik.hip: workgroup (c, j) of a (C, nsplit <= 32) grid handles the elements
// e = j * 256 + tid (+ nsplit * 256 ...) of output c's (S, B) slab, writes gmu / gvar and leaves its partial sums in the caller's
// scratch -- values in ws[c * nsplit + j], the sums of d ell / d parameter (Student-t's log_scale) behind them; a second launch
// of one wavefront adds them in index order.  No float atomics anywhere: every sum has a fixed order, two runs are bitwise
// equal, and the backward's value equals the forward's bit for bit.
// Precision: inputs and outputs are fp32; an element's arithmetic, the partial sums (ws is read as LIK::real) and the adder run
// in LIK::real.  Where that is double the launch is still bound by latency, not by the fp64 rate.
#include "lik.h"

namespace vargp {

constexpr int kLikThreads = 256;
constexpr int kLikMaxSplit = 32;

// grid (C, nsplit).  GRAD: gmu, gvar = seed[0] * d nll / d (mu, var).  vpart (may be NULL): [C * nsplit] sums of ell;
// ppart (GRAD, kHasParam): [C * nsplit] sums of d ell / d parameter
template <class LIK, bool GRAD>
__global__ __launch_bounds__(kLikThreads) void nll_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                          typename LIK::Args args, const float* __restrict__ seed,
                                                          float* __restrict__ gmu, float* __restrict__ gvar,
                                                          typename LIK::real* __restrict__ vpart,
                                                          typename LIK::real* __restrict__ ppart, int S, int C, int B) {
  using real = typename LIK::real;
  __shared__ real red[kLikThreads / kWave];
  const int c = blockIdx.x, nsplit = gridDim.y;
  const int SB = S * B;
  const int64_t CB = (int64_t)C * B;
  const real g = GRAD ? -(real)seed[0] / (real)S : (real)0;
  const typename LIK::Cls cls = LIK::cls(args, c);
  real acc = 0, pacc = 0;
  for (int64_t e = (int64_t)blockIdx.y * kLikThreads + threadIdx.x; e < SB; e += (int64_t)nsplit * kLikThreads) {
    const int s = (int)(e / B), b = (int)(e - (int64_t)s * B);
    const int64_t i = (int64_t)s * CB + (int64_t)c * B + b;
    real dmu = 0, dvar = 0, dpar = 0;
    acc += LIK::template element<GRAD>(cls, (real)mu[i], (real)var[i], LIK::template target<real>(args, c, b), dmu, dvar, dpar);
    if (GRAD) {
      gmu[i] = (float)(g * dmu);
      gvar[i] = (float)(g * dvar);
      pacc += dpar;
    }
  }
  if (vpart) {
    acc = block_sum<kLikThreads>(acc, red);
    if (threadIdx.x == 0) vpart[(int64_t)c * nsplit + blockIdx.y] = acc;
  }
  if (GRAD && LIK::kHasParam) {
    pacc = block_sum<kLikThreads>(pacc, red);
    if (threadIdx.x == 0) ppart[(int64_t)c * nsplit + blockIdx.y] = pacc;
  }
}

// one wavefront.  nll (may be NULL) = -(1 / S) sum_i vpart[i]: lanes stride the array in index order, then the wave tree;
// gpar (may be NULL): gpar[c] = -(seed / S) sum_j ppart[c * nsplit + j], one lane per output, j in order
template <class real>
__global__ __launch_bounds__(kWave) void finish_kernel(const real* __restrict__ vpart, const real* __restrict__ ppart, int C,
                                                       int nsplit, real inv_s, const float* __restrict__ seed,
                                                       float* __restrict__ nll, float* __restrict__ gpar) {
  if (nll) {
    real acc = 0;
    for (int i = threadIdx.x; i < C * nsplit; i += kWave) acc += vpart[i];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) nll[0] = (float)(-inv_s * acc);
  }
  if (gpar) {
    const real g = -(real)seed[0] * inv_s;
    for (int c = threadIdx.x; c < C; c += kWave) {
      real acc = 0;
      for (int j = 0; j < nsplit; ++j) acc += ppart[(int64_t)c * nsplit + j];
      gpar[c] = (float)(g * acc);
    }
  }
}

// grid over (c, b), b fastest: probs[b, c] = mean_s P(t = 1).  Probit: closed form Phi(mu / sqrt(1 + var)); logit: the rule
template <class LINK>
__global__ __launch_bounds__(kLikThreads) void bern_predict_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                                   float* __restrict__ probs, int S, int C, int B) {
  const int64_t CB = (int64_t)C * B;
  const int64_t j = (int64_t)blockIdx.x * kLikThreads + threadIdx.x;
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
      for (int k = 0; k < kGhPairs; ++k)
        p += (float)kGhW[k] * (LINK::prob(m + sd * (float)kGhX[k]) + LINK::prob(m - sd * (float)kGhX[k]));
      acc += p;
    }
  }
  probs[(int64_t)b * C + c] = acc / (float)S;
}

// rate[s, c, b] = E exp(f) = exp(mu + var / 2)
__global__ __launch_bounds__(kLikThreads) void poisson_predict_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                                      float* __restrict__ rate, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kLikThreads + threadIdx.x;
  if (i < n) rate[i] = (float)exp((double)mu[i] + 0.5 * (double)var[i]);
}

static int nsplit_of(int S, int B) {
  const int n = cdiv((int64_t)S * B, kLikThreads);
  return n < kLikMaxSplit ? n : kLikMaxSplit;
}

template <class LIK>
static size_t workspace_bytes(int S, int C, int B) {
  if (S <= 0 || C <= 0 || B <= 0) return 0;
  return (size_t)C * nsplit_of(S, B) * sizeof(typename LIK::real) * (LIK::kHasParam ? 2 : 1);
}

template <class LIK, bool GRAD>
static int launch(const char* what, const float* mu, const float* var, typename LIK::Args args, const float* seed, float* gmu,
                  float* gvar, float* gpar, float* nll, int S, int C, int B, float* ws, hipStream_t st) {
  using real = typename LIK::real;
  const int nsplit = nsplit_of(S, B);
  real* part = reinterpret_cast<real*>(ws);                       // (aligned: LIK_CHECK_NLL)
  real* vpart = nll ? part : nullptr;
  real* ppart = GRAD && LIK::kHasParam ? part + (size_t)C * nsplit : nullptr;
  hipLaunchKernelGGL((nll_kernel<LIK, GRAD>), dim3(C, nsplit), dim3(kLikThreads), 0, st, mu, var, args, seed, gmu, gvar, vpart,
                     ppart, S, C, B);
  if (nll || ppart)
    hipLaunchKernelGGL(finish_kernel<real>, dim3(1), dim3(kWave), 0, st, vpart, ppart, C, nsplit, (real)1 / (real)S, seed, nll,
                       ppart ? gpar : nullptr);
  return check_launch(what);
}

using Probit = Bernoulli<LinkProbit>;
using Logit = Bernoulli<LinkLogit>;

}  // namespace vargp

using namespace vargp;

// `big`: the message for a size past the frame's limits (each entry keeps the wording it has always had)
#define LIK_CHECK_COMMON(what, big)                                                                                      \
  VARGP_REQUIRE(mu && var && S > 0 && C > 0 && B > 0, what ": bad arguments");                                          \
  VARGP_REQUIRE((int64_t)S * B <= INT32_MAX, what big)
// the frame's own limits: the grid, and partial sums that are read as LIK::real
#define LIK_CHECK_NLL(what, LIK, big)                                                                                    \
  VARGP_REQUIRE((int64_t)C * kLikMaxSplit <= INT32_MAX, what big);                                                      \
  VARGP_REQUIRE(reinterpret_cast<uintptr_t>(ws) % sizeof(LIK::real) == 0 || sizeof(LIK::real) == sizeof(float),         \
                what ": ws must be 8-byte aligned")
#define BERN_BIG_SB ": S * B too large"
#define BERN_BIG_C ": C too large"
#define REG_BIG ": S * B or C too large"
#define BERN_CHECK_LINK(what) VARGP_REQUIRE(link == 0 || link == 1, what ": link must be 0 (probit) or 1 (logit)")
#define BERN_CHECK_TARGET(what)                                                                                          \
  VARGP_REQUIRE((t != nullptr) != (labels != nullptr), what ": exactly one of t and labels");                           \
  VARGP_REQUIRE(labels || ldt == 0 || ldt >= B, what ": ldt must be 0 or >= B")
#define REG_CHECK_TARGET(what) VARGP_REQUIRE(y && (ldy == 0 || ldy >= B), what ": y must be given, ldy 0 or >= B")

extern "C" size_t vargp_bernoulli_workspace_bytes(int S, int C, int B) { return workspace_bytes<Probit>(S, C, B); }

extern "C" int vargp_bernoulli_nll_fwd(const float* mu, const float* var, const float* t, int64_t ldt, const int64_t* labels,
                                       int link, float* nll, int S, int C, int B, float* ws, size_t ws_bytes,
                                       vargp_stream_t stream) {
  LIK_CHECK_COMMON("bernoulli_nll_fwd", BERN_BIG_SB);
  BERN_CHECK_LINK("bernoulli_nll_fwd");
  BERN_CHECK_TARGET("bernoulli_nll_fwd");
  LIK_CHECK_NLL("bernoulli_nll_fwd", Probit, BERN_BIG_C);
  VARGP_REQUIRE(nll && ws && ws_bytes >= vargp_bernoulli_workspace_bytes(S, C, B), "bernoulli_nll_fwd: nll / workspace");
  return (link == 0 ? launch<Probit, false> : launch<Logit, false>)("bernoulli_nll_fwd", mu, var, {t, ldt, labels}, nullptr,
                                                                    nullptr, nullptr, nullptr, nll, S, C, B, ws,
                                                                    as_stream(stream));
}

extern "C" int vargp_bernoulli_nll_bwd(const float* mu, const float* var, const float* t, int64_t ldt, const int64_t* labels,
                                       int link, const float* seed, float* gmu, float* gvar, float* nll, int S, int C, int B,
                                       float* ws, size_t ws_bytes, vargp_stream_t stream) {
  LIK_CHECK_COMMON("bernoulli_nll_bwd", BERN_BIG_SB);
  BERN_CHECK_LINK("bernoulli_nll_bwd");
  BERN_CHECK_TARGET("bernoulli_nll_bwd");
  LIK_CHECK_NLL("bernoulli_nll_bwd", Probit, BERN_BIG_C);
  VARGP_REQUIRE(seed && gmu && gvar, "bernoulli_nll_bwd: bad arguments");
  VARGP_REQUIRE(!nll || (ws && ws_bytes >= vargp_bernoulli_workspace_bytes(S, C, B)), "bernoulli_nll_bwd: workspace too small");
  return (link == 0 ? launch<Probit, true> : launch<Logit, true>)("bernoulli_nll_bwd", mu, var, {t, ldt, labels}, seed, gmu, gvar,
                                                                  nullptr, nll, S, C, B, ws, as_stream(stream));
}

extern "C" int vargp_bernoulli_predict(const float* mu, const float* var, int link, float* probs, int S, int C, int B,
                                       vargp_stream_t stream) {
  LIK_CHECK_COMMON("bernoulli_predict", BERN_BIG_SB);
  BERN_CHECK_LINK("bernoulli_predict");
  VARGP_REQUIRE(probs && (int64_t)C * B <= (int64_t)INT32_MAX * kLikThreads, "bernoulli_predict: bad arguments");
  const dim3 grid(cdiv((int64_t)C * B, kLikThreads)), block(kLikThreads);
  if (link == 0)
    hipLaunchKernelGGL(bern_predict_kernel<LinkProbit>, grid, block, 0, as_stream(stream), mu, var, probs, S, C, B);
  else
    hipLaunchKernelGGL(bern_predict_kernel<LinkLogit>, grid, block, 0, as_stream(stream), mu, var, probs, S, C, B);
  return check_launch("bernoulli_predict");
}

extern "C" size_t vargp_poisson_workspace_bytes(int S, int C, int B) { return workspace_bytes<Poisson>(S, C, B); }

extern "C" int vargp_poisson_nll_fwd(const float* mu, const float* var, const float* y, int64_t ldy, float* nll, int S, int C,
                                     int B, float* ws, size_t ws_bytes, vargp_stream_t stream) {
  LIK_CHECK_COMMON("poisson_nll_fwd", REG_BIG);
  REG_CHECK_TARGET("poisson_nll_fwd");
  LIK_CHECK_NLL("poisson_nll_fwd", Poisson, REG_BIG);
  VARGP_REQUIRE(nll && ws && ws_bytes >= vargp_poisson_workspace_bytes(S, C, B), "poisson_nll_fwd: nll / workspace");
  return launch<Poisson, false>("poisson_nll_fwd", mu, var, {{y, ldy}}, nullptr, nullptr, nullptr, nullptr, nll, S, C, B, ws,
                                as_stream(stream));
}

extern "C" int vargp_poisson_nll_bwd(const float* mu, const float* var, const float* y, int64_t ldy, const float* seed,
                                     float* gmu, float* gvar, float* nll, int S, int C, int B, float* ws, size_t ws_bytes,
                                     vargp_stream_t stream) {
  LIK_CHECK_COMMON("poisson_nll_bwd", REG_BIG);
  REG_CHECK_TARGET("poisson_nll_bwd");
  LIK_CHECK_NLL("poisson_nll_bwd", Poisson, REG_BIG);
  VARGP_REQUIRE(seed && gmu && gvar, "poisson_nll_bwd: bad arguments");
  VARGP_REQUIRE(!nll || (ws && ws_bytes >= vargp_poisson_workspace_bytes(S, C, B)), "poisson_nll_bwd: workspace too small");
  return launch<Poisson, true>("poisson_nll_bwd", mu, var, {{y, ldy}}, seed, gmu, gvar, nullptr, nll, S, C, B, ws,
                               as_stream(stream));
}

extern "C" int vargp_poisson_predict(const float* mu, const float* var, float* rate, int S, int C, int B,
                                     vargp_stream_t stream) {
  LIK_CHECK_COMMON("poisson_predict", REG_BIG);
  const int64_t n = (int64_t)S * C * B;
  VARGP_REQUIRE((int64_t)C * kLikMaxSplit <= INT32_MAX, "poisson_predict" REG_BIG);
  VARGP_REQUIRE(rate && n <= (int64_t)INT32_MAX * kLikThreads, "poisson_predict: bad arguments");
  hipLaunchKernelGGL(poisson_predict_kernel, dim3(cdiv(n, kLikThreads)), dim3(kLikThreads), 0, as_stream(stream), mu, var, rate,
                     n);
  return check_launch("poisson_predict");
}

extern "C" size_t vargp_studentt_workspace_bytes(int S, int C, int B) { return workspace_bytes<StudentT>(S, C, B); }

extern "C" int vargp_studentt_nll_fwd(const float* mu, const float* var, const float* y, int64_t ldy, const float* log_scale,
                                      float df, float lognorm, float* nll, int S, int C, int B, float* ws, size_t ws_bytes,
                                      vargp_stream_t stream) {
  LIK_CHECK_COMMON("studentt_nll_fwd", REG_BIG);
  REG_CHECK_TARGET("studentt_nll_fwd");
  LIK_CHECK_NLL("studentt_nll_fwd", StudentT, REG_BIG);
  VARGP_REQUIRE(log_scale && df > 0.f, "studentt_nll_fwd: log_scale must be given, df > 0");
  VARGP_REQUIRE(nll && ws && ws_bytes >= vargp_studentt_workspace_bytes(S, C, B), "studentt_nll_fwd: nll / workspace");
  return launch<StudentT, false>("studentt_nll_fwd", mu, var, {{y, ldy}, log_scale, df, lognorm}, nullptr, nullptr, nullptr,
                                 nullptr, nll, S, C, B, ws, as_stream(stream));
}

extern "C" int vargp_studentt_nll_bwd(const float* mu, const float* var, const float* y, int64_t ldy, const float* log_scale,
                                      float df, float lognorm, const float* seed, float* gmu, float* gvar, float* g_log_scale,
                                      float* nll, int S, int C, int B, float* ws, size_t ws_bytes, vargp_stream_t stream) {
  LIK_CHECK_COMMON("studentt_nll_bwd", REG_BIG);
  REG_CHECK_TARGET("studentt_nll_bwd");
  LIK_CHECK_NLL("studentt_nll_bwd", StudentT, REG_BIG);
  VARGP_REQUIRE(log_scale && df > 0.f, "studentt_nll_bwd: log_scale must be given, df > 0");
  VARGP_REQUIRE(seed && gmu && gvar && g_log_scale, "studentt_nll_bwd: bad arguments");
  VARGP_REQUIRE(ws && ws_bytes >= vargp_studentt_workspace_bytes(S, C, B), "studentt_nll_bwd: workspace too small");
  return launch<StudentT, true>("studentt_nll_bwd", mu, var, {{y, ldy}, log_scale, df, lognorm}, seed, gmu, gvar, g_log_scale,
                                nll, S, C, B, ws, as_stream(stream));
}
