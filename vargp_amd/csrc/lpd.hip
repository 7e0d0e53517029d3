// Held-out log predictive density (LPD) of every likelihood: the last stage (mu, var, y) -> log E_q[p(y | f)].  Not in the
// reference.  (The nll entries give E_q[log p], the ELBO term; the LPD needs the variance and the MIXTURE over hyper-samples.)
// mu, var [S, C, B] are the predictive moments of f under hyper-sample s.  Per (s, c, b) the log marginal likelihood of the target:
//   Gaussian          lp = log N(y; mu, var + exp(obs_log_var[c]))                                        (closed form)
//   Bernoulli probit  lp = log Phi(s_cb mu / sqrt(1 + var)) = log(erfc(-z / sqrt2) / 2), s = 2 t - 1      (closed form)
//   Bernoulli logit   lp = logsumexp_k( log w^_k + log sigma(s_cb f_k) )
//   Poisson           lp = logsumexp_k( log w^_k + y f_k - exp(f_k) ) - lgamma(y + 1)
//   Student-t         lp = logsumexp_k( log w^_k - (nu + 1) / 2 log1p((y - f_k)^2 / (nu sigma_c^2)) ) + K_c
// with f_k = mu + sqrt(2 var) x_k and (x_k, w^_k) the 20-node Gauss-Hermite rule of lik.h (which also has each likelihood's lp and tail); as in indep_lik.hip, the
// quadrature sums are the DEFINITION.  The hyper-sample is shared by all outputs of a point, so the density of a point's whole
// target vector is the mixture of products, and the per-output marginals mix each output alone:
//   lpd[b]       = logsumexp_s( sum_c lp[s,c,b] ) - log S
//   lpd_out[c,b] = logsumexp_s( lp[s,c,b] )       - log S
// Softmax, eps [S, F, C, B], y int64 [B]:  lpd[b] = logsumexp_{s,f}( log_softmax_c(mu + sqrt(var) eps)[y_b] ) - log(S F).
// Probit below z ~ -37.5: erfc underflows in fp64 and lp = -inf, which is what log(0) is; a term of -inf drops out of the
// logsumexp (no NaN), and a point whose every term is -inf gets lpd = -inf.
//
// Launch layout.  Lanes run along b (mu / var / y / eps are contiguous in b: coalesced loads).  Joint kernel: workgroup j owns the
// 64 points [64 j, 64 j + 64) for all (s, c); its nw = min(S, 8) waves split the hyper-samples (wave w: s = w, w + nw, ...), each
// keeps a running (max, sum) pair per lane, and wave 0 combines the nw pairs through LDS in wave order.  Parts of lp that do not
// depend on s (lgamma(y + 1), K_c: `tail`) are added once, after the mixture.  Per-output kernel (a second loop order, c outer and
// s inner, recomputing lp; optional and cheap): workgroup (j, q), wave w owns output c = 4 q + w of the same 64 points and walks
// s in order; no LDS.  No workspace, no float atomics: every sum has a fixed order and two runs are bitwise equal.
// Precision: inputs and outputs are fp32; element arithmetic and every sum run in fp64 (as the Poisson and Student-t ELBO terms), so each output is the
// definition's value rounded ONCE.  All logsumexp's subtract the running maximum.
#include "lik.h"

namespace vargp {

constexpr int kLpdMaxWaves = 8;
constexpr int kLpdOutWaves = 4;

// running logsumexp: (m, s) stands for m + log(s); the empty sum is (-inf, 0).  A term of -inf changes nothing; a NaN term makes
// s NaN (it is not dropped).
__device__ __forceinline__ void lse_push(double& m, double& s, double a) {
  if (a > m) {
    s = s * exp(m - a) + 1.0;
    m = a;
  } else if (!(a == -kInf)) {
    s += exp(a - m);
  }
}
__device__ __forceinline__ void lse_merge(double& m, double& s, double m2, double s2) {
  const double mx = fmax(m, m2);
  if (mx == -kInf) {                             // both empty, or all terms -inf: the sums are 0 (or NaN, which is kept)
    s += s2;
    return;
  }
  s = s * exp(m - mx) + s2 * exp(m2 - mx);
  m = mx;
}
__device__ __forceinline__ double lse_value(double m, double s) { return s == 0.0 ? -kInf : m + log(s); }

// Wave 0 of a joint workgroup: the other waves' (max, sum) pairs of each lane's point, merged in wave order
__device__ __forceinline__ void lpd_merge_waves(double& m, double& s, double (*red)[2][kWave], int nw, int lane) {
  for (int q = 1; q < nw; ++q) lse_merge(m, s, red[q][0][lane], red[q][1][lane]);
}

// grid (ceil(B / 64)), block 64 nw.  lpd[b] = logsumexp_s( sum_c lp[s,c,b] ) - log S
template <class LIK>
__global__ __launch_bounds__(kLpdMaxWaves* kWave) void lpd_joint_kernel(const float* __restrict__ mu,
                                                                         const float* __restrict__ var, typename LIK::Args args,
                                                                         float* __restrict__ lpd, int S, int C, int B) {
  __shared__ double red[kLpdMaxWaves][2][kWave];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const size_t b = (size_t)blockIdx.x * kWave + lane;
  const bool live = b < (size_t)B;
  double m = -kInf, sum = 0.0;
  if (live) {
    for (int s = w; s < S; s += nw) {
      double a = 0.0;
      for (int c = 0; c < C; ++c) {
        const size_t i = ((size_t)s * C + c) * (size_t)B + b;
        a += LIK::lp(LIK::cls(args, c), (double)mu[i], (double)var[i], LIK::template target<double>(args, c, b));
      }
      lse_push(m, sum, a);
    }
  }
  red[w][0][lane] = m;
  red[w][1][lane] = sum;
  __syncthreads();
  if (w != 0 || !live) return;
  lpd_merge_waves(m, sum, red, nw, lane);
  double tail = 0.0;
  for (int c = 0; c < C; ++c) tail += LIK::tail(LIK::cls(args, c), LIK::template target<double>(args, c, b));
  lpd[b] = (float)(lse_value(m, sum) - log((double)S) + tail);
}

// grid (ceil(B / 64), ceil(C / 4)), block 256: wave w owns output c = 4 blockIdx.y + w.  lpd_out[c,b] = logsumexp_s lp[s,c,b] - log S
template <class LIK>
__global__ __launch_bounds__(kLpdOutWaves* kWave) void lpd_out_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                                       typename LIK::Args args, float* __restrict__ lpd_out,
                                                                       int S, int C, int B) {
  const int lane = threadIdx.x & (kWave - 1), c = (int)blockIdx.y * kLpdOutWaves + (int)(threadIdx.x >> 6);
  const size_t b = (size_t)blockIdx.x * kWave + lane;
  if (c >= C || b >= (size_t)B) return;
  const typename LIK::Cls cls = LIK::cls(args, c);
  const double y = LIK::template target<double>(args, c, b);
  double m = -kInf, sum = 0.0;
  for (int s = 0; s < S; ++s) {
    const size_t i = ((size_t)s * C + c) * (size_t)B + b;
    lse_push(m, sum, LIK::lp(cls, (double)mu[i], (double)var[i], y));
  }
  lpd_out[(size_t)c * B + b] = (float)(lse_value(m, sum) - log((double)S) + LIK::tail(cls, y));
}

// grid (ceil(B / 64)), block 64 nw; the waves split the S F (hyper-sample, likelihood-sample) pairs.
// lpd[b] = logsumexp_{s,f}( f_y - logsumexp_c f_c ) - log(S F), f_c = mu + sqrt(var) eps.  The label is compared, never used as
// an index: one outside [0, C) is not checked and that point's value is meaningless (f_y stays 0), but nothing is read out of bounds
__global__ __launch_bounds__(kLpdMaxWaves* kWave) void lpd_softmax_kernel(const float* __restrict__ mu,
                                                                           const float* __restrict__ var,
                                                                           const float* __restrict__ eps,
                                                                           const int64_t* __restrict__ y, float* __restrict__ lpd,
                                                                           int S, int F, int C, int B) {
  __shared__ double red[kLpdMaxWaves][2][kWave];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const size_t b = (size_t)blockIdx.x * kWave + lane;
  const bool live = b < (size_t)B;
  const int SF = S * F;
  double m = -kInf, sum = 0.0;
  if (live) {
    const int64_t yb = y[b];
    for (int p = w; p < SF; p += nw) {
      const int s = p / F;
      double cm = -kInf, cs = 0.0, fy = 0.0;
      for (int c = 0; c < C; ++c) {
        const size_t i = ((size_t)s * C + c) * (size_t)B + b, j = ((size_t)p * C + c) * (size_t)B + b;
        const double f = (double)mu[i] + sqrt((double)var[i]) * (double)eps[j];
        if ((int64_t)c == yb) fy = f;
        lse_push(cm, cs, f);
      }
      lse_push(m, sum, fy - lse_value(cm, cs));
    }
  }
  red[w][0][lane] = m;
  red[w][1][lane] = sum;
  __syncthreads();
  if (w != 0 || !live) return;
  lpd_merge_waves(m, sum, red, nw, lane);
  lpd[b] = (float)(lse_value(m, sum) - log((double)SF));
}

static int lpd_waves(int64_t n) { return (int)(n < kLpdMaxWaves ? n : kLpdMaxWaves); }

template <class LIK>
static int lpd_launch(const char* what, const float* mu, const float* var, typename LIK::Args args, float* lpd, float* lpd_out,
                      int S, int C, int B, hipStream_t st) {
  const int nbx = cdiv(B, kWave);
  hipLaunchKernelGGL(lpd_joint_kernel<LIK>, dim3(nbx), dim3(kWave * lpd_waves(S)), 0, st, mu, var, args, lpd, S, C, B);
  if (lpd_out)
    hipLaunchKernelGGL(lpd_out_kernel<LIK>, dim3(nbx, cdiv(C, kLpdOutWaves)), dim3(kWave * kLpdOutWaves), 0, st, mu, var, args,
                       lpd_out, S, C, B);
  return check_launch(what);
}

}  // namespace vargp

using namespace vargp;

#define LPD_CHECK_COMMON(what)                                                                                          \
  VARGP_REQUIRE(mu && var && lpd && S > 0 && C > 0 && B > 0, what ": bad arguments");                                   \
  VARGP_REQUIRE(C <= 65535 * kLpdOutWaves, what ": C too large")
#define LPD_CHECK_TARGET(what) VARGP_REQUIRE(y && (ldy == 0 || ldy >= B), what ": y must be given, ldy 0 or >= B")

extern "C" int vargp_softmax_lpd(const float* mu, const float* var, const float* eps, const int64_t* y, float* lpd, int S, int F,
                                 int C, int B, vargp_stream_t stream) {
  VARGP_REQUIRE(mu && var && eps && y && lpd && S > 0 && F > 0 && C > 0 && B > 0, "softmax_lpd: bad arguments");
  VARGP_REQUIRE((int64_t)S * F <= INT32_MAX, "softmax_lpd: S * F too large");
  hipLaunchKernelGGL(lpd_softmax_kernel, dim3(cdiv(B, kWave)), dim3(kWave * lpd_waves((int64_t)S * F)), 0, as_stream(stream), mu,
                     var, eps, y, lpd, S, F, C, B);
  return check_launch("softmax_lpd");
}

extern "C" int vargp_gauss_lpd(const float* mu, const float* var, const float* y, int64_t ldy, const float* obs_log_var,
                               float* lpd, float* lpd_out, int S, int C, int B, vargp_stream_t stream) {
  LPD_CHECK_COMMON("gauss_lpd");
  LPD_CHECK_TARGET("gauss_lpd");
  VARGP_REQUIRE(obs_log_var, "gauss_lpd: obs_log_var must be given");
  return lpd_launch<Gauss>("gauss_lpd", mu, var, {{y, ldy}, obs_log_var}, lpd, lpd_out, S, C, B,
                              as_stream(stream));
}

extern "C" int vargp_bernoulli_lpd(const float* mu, const float* var, const float* t, int64_t ldt, const int64_t* labels,
                                   int link, float* lpd, float* lpd_out, int S, int C, int B, vargp_stream_t stream) {
  LPD_CHECK_COMMON("bernoulli_lpd");
  VARGP_REQUIRE(link == 0 || link == 1, "bernoulli_lpd: link must be 0 (probit) or 1 (logit)");
  VARGP_REQUIRE((t != nullptr) != (labels != nullptr), "bernoulli_lpd: exactly one of t and labels");
  VARGP_REQUIRE(labels || ldt == 0 || ldt >= B, "bernoulli_lpd: ldt must be 0 or >= B");
  if (link == 0)
    return lpd_launch<Bernoulli<LinkProbit>>("bernoulli_lpd", mu, var, {t, ldt, labels}, lpd, lpd_out, S, C, B, as_stream(stream));
  return lpd_launch<Bernoulli<LinkLogit>>("bernoulli_lpd", mu, var, {t, ldt, labels}, lpd, lpd_out, S, C, B, as_stream(stream));
}

extern "C" int vargp_poisson_lpd(const float* mu, const float* var, const float* y, int64_t ldy, float* lpd, float* lpd_out,
                                 int S, int C, int B, vargp_stream_t stream) {
  LPD_CHECK_COMMON("poisson_lpd");
  LPD_CHECK_TARGET("poisson_lpd");
  return lpd_launch<Poisson>("poisson_lpd", mu, var, {{y, ldy}}, lpd, lpd_out, S, C, B, as_stream(stream));
}

extern "C" int vargp_studentt_lpd(const float* mu, const float* var, const float* y, int64_t ldy, const float* log_scale,
                                  float df, float lognorm, float* lpd, float* lpd_out, int S, int C, int B,
                                  vargp_stream_t stream) {
  LPD_CHECK_COMMON("studentt_lpd");
  LPD_CHECK_TARGET("studentt_lpd");
  VARGP_REQUIRE(log_scale && df > 0.f, "studentt_lpd: log_scale must be given, df > 0");
  return lpd_launch<StudentT>("studentt_lpd", mu, var, {{y, ldy}, log_scale, df, lognorm}, lpd, lpd_out, S, C, B,
                              as_stream(stream));
}
