// What the kernels of the independent-output likelihoods share (indep_lik.hip: the ELBO term E_q[log p] and its gradients;
// lpd.hip: the held-out log predictive density; uncertainty.hip: the predictive entropy and its parts): the quadrature table,
// the target readers and one struct per likelihood.
//   Bernoulli   p(t | f) = Lambda(s f), s = 2 t - 1, Lambda = Phi (probit) or the logistic function (logit)
//   Poisson     p(y | f) = exp(y f - exp(f)) / y!                                                (log link: counts)
//   Student-t   p(y | f) = t_nu((y - f) / sigma_c) / sigma_c,  sigma_c = exp(log_scale[c])       (fixed nu: outliers)
//   Gaussian    p(y | f) = N(y; f, exp(obs_log_var[c]))       (LPD only: its ELBO term has its own launch, gauss_lik.hip)
// None but the Gaussian is in the reference.
//
// A likelihood LIK has
//   real                      the type its ELBO term is evaluated and summed in (Bernoulli: float; the others: double, so that
//                             every output is the formula's value rounded ONCE to fp32)
//   Args                      target and parameters, by value into the kernel;  Cls = cls(args, c): what is constant over output c
//   target<T>(args, c, b)     the target of (c, b) as a T (Bernoulli: the sign s)
//   kHasParam                 does the output have a parameter of its own with a gradient
//   element<GRAD>(cls, mu, var, y, dmu, dvar, dpar) = ell = E_{f ~ N(mu, var)} log p(y | f) and (GRAD) d ell / d (mu, var, parameter)
//   lp(cls, mu, var, y)       the part of log E_{f ~ N(mu, var)} p(y | f) that depends on the hyper-sample;  tail(cls, y): the rest
// Where the expectation has no closed form it is DEFINED by the 20-node Gauss-Hermite rule, and the
// gradients are the exact derivatives of that sum.  The nodes are symmetric and are visited in +-x_k pairs: with g the
// derivative of a term with respect to f,
//   d ell / d mu = sum_{k>0} w^_k (g_k + g_-k),   d ell / d var = sum_{k>0} w^_k x_k (g_k - g_-k) / sqrt(2 var)
// -- the pair difference carries the whole variance gradient, which at small var would otherwise be the small remainder of
// twenty terms of either sign; at var = 0 it is exactly 0 and so is the result.
// Contraction is switched off in every `element` (and the links it calls) so that its GRAD and value-only instantiations round
// alike: the backward's value equals the forward's bit for bit.
#pragma once
#include "common.h"

namespace vargp {

constexpr int kGhPairs = 10;
// x, w = numpy.polynomial.hermite.hermgauss(20): the positive half x[10:], w[10:] / sqrt(pi) and its log (17 digits; fp32
// code reads the table through a cast, which gives the float nearest to the literal)
__device__ constexpr double kGhX[kGhPairs] = {0.24534070830090124, 0.73747372854539439, 1.2340762153953231,
                                              1.7385377121165861,  2.2549740020892757,  2.7888060584281305,
                                              3.3478545673832163,  3.9447640401156252,  4.6036824495507442,
                                              5.3874808900112328};
__device__ constexpr double kGhW[kGhPairs] = {0.26079306344955488,    0.16173933398399998,    0.061506372063976897,
                                              0.013997837447101022,   0.00183010313108049,    0.00012882627996192928,
                                              4.402121090230851e-06,  6.127490259982928e-08,  2.4820623623151755e-10,
                                              1.2578006724379234e-13};
__device__ constexpr double kGhLogW[kGhPairs] = {-1.344028046485978,  -1.8217692891416608, -2.7886144987405204,
                                                 -4.268852429362512,  -6.303382957935046,  -8.957045728135233,
                                                 -12.333424067234969, -16.60789549709157,  -22.11676111764163,
                                                 -29.704241511181127};
constexpr double kInvSqrt2 = 0.70710678118654752440;
constexpr double kInvSqrt2Pi = 0.39894228040143267794;
constexpr double kHalfLog2Pi = 0.9189385332046727;
constexpr double kInf = __builtin_huge_val();

// logsumexp_k( log w^_k + term(f_k) ), f_k = mu + sqrt(2 var) x_k: the twenty terms, their maximum, then the sum in node order
template <class TERM>
__device__ __forceinline__ double gh_lse(double mu, double var, TERM term) {
  const double sd = sqrt(2.0 * var);
  double t[2 * kGhPairs], mx = -kInf;
#pragma unroll
  for (int k = 0; k < kGhPairs; ++k) {
    const double d = sd * kGhX[k];
    t[2 * k] = kGhLogW[k] + term(mu + d);
    t[2 * k + 1] = kGhLogW[k] + term(mu - d);
    mx = fmax(mx, fmax(t[2 * k], t[2 * k + 1]));
  }
  const double sh = mx == -kInf ? 0.0 : mx;      // every term -inf: the sum is 0 and the value log(0) = -inf, not NaN
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 2 * kGhPairs; ++k) s += exp(t[k] - sh);
  return sh + log(s);
}

// y [C, B] with row stride ldy, or one row shared by every output (ldy = 0)
struct Target {
  const float* y;
  int64_t ldy;
  __device__ __forceinline__ float at(int c, size_t b) const { return y[(size_t)c * (size_t)ldy + b]; }
};

// A link: eval(z, lp, dlp) = log Lambda(z) and its derivative; prob(z) = Lambda(z).  fp32.  logp(z) = log Lambda(z) in fp64.
struct LinkProbit {
  // With a = |z| / sqrt2 and the scaled complementary error function erfcx(a) = exp(a^2) erfc(a) (finite and accurate for every
  // a >= 0):  z < 0:  Phi(z) = erfcx(a) exp(-a^2) / 2  ->  log Phi = log(erfcx(a) / 2) - a^2,  phi / Phi = sqrt(2 / pi) / erfcx(a)
  //           z >= 0: Phi(z) = 1 - q, q = erfcx(a) exp(-a^2) / 2  ->  log Phi = log1p(-q),     phi / Phi = exp(-a^2) / (sqrt(2 pi) (1 - q))
  template <bool GRAD>
  static __device__ __forceinline__ void eval(float z, float& lp, float& dlp) {
#pragma clang fp contract(off)
    const float a = fabsf(z) * (float)kInvSqrt2, a2 = a * a, ex = erfcxf(a);
    if (z < 0.f) {
      lp = logf(0.5f * ex) - a2;
      if (GRAD) dlp = (2.f * (float)kInvSqrt2Pi) / ex;
    } else {
      const float e = expf(-a2), q = 0.5f * ex * e;
      lp = log1pf(-q);
      if (GRAD) dlp = (float)kInvSqrt2Pi * e / (1.f - q);
    }
  }
  static __device__ __forceinline__ float prob(float z) { return 0.5f * erfcf(-z * (float)kInvSqrt2); }
  // log Phi(z) in fp64, the two branches of eval: finite for every finite z (uncertainty.hip)
  static __device__ __forceinline__ double logp(double z) {
    const double a = fabs(z) * kInvSqrt2, ex = erfcx(a);
    return z < 0.0 ? log(0.5 * ex) - a * a : log1p(-0.5 * ex * exp(-a * a));
  }
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
  // log sigma(z) in fp64 (uncertainty.hip)
  static __device__ __forceinline__ double logp(double z) { return fmin(z, 0.0) - log1p(exp(-fabs(z))); }
};

// ell = sum_k w^_k log Lambda(s (mu + sqrt(2 var) x_k)) in fp32;
// lp = log Phi(s mu / sqrt(1 + var)) = log(erfc(-z / sqrt2) / 2) (probit, closed form; -inf below z ~ -37.5, where fp64 erfc
// underflows) or logsumexp_k( log w^_k + log sigma(s f_k) ) (logit), in fp64
struct BernoulliArgs {
  const float* t;           // [C, B] with row stride ldt, or one shared row (ldt = 0); or
  int64_t ldt;
  const int64_t* labels;    // one-vs-rest class indices [B]: t[c, b] = (labels[b] == c).  Exactly one of the two is given
};
template <class LINK>
struct Bernoulli {
  using real = float;
  static constexpr bool kHasParam = false;
  using Args = BernoulliArgs;
  struct Cls {};
  static __device__ __forceinline__ Cls cls(const Args&, int) { return Cls{}; }
  template <class T>
  static __device__ __forceinline__ T target(const Args& a, int c, size_t b) {
    // one-vs-rest labels: a label outside [0, C) matches no output (every output of that point is a negative)
    if (a.labels) return a.labels[b] == (int64_t)c ? T(1) : T(-1);
    return T(2) * (T)a.t[(size_t)c * (size_t)a.ldt + b] - T(1);
  }
  template <bool GRAD>
  static __device__ __forceinline__ float element(const Cls&, float mu, float var, float sgn, float& dmu, float& dvar, float&) {
#pragma clang fp contract(off)
    const float sd = sqrtf(2.f * var);
    float ell = 0.f, am = 0.f, av = 0.f;
#pragma unroll
    for (int k = 0; k < kGhPairs; ++k) {
      const float x = (float)kGhX[k], w = (float)kGhW[k];
      const float d = sd * x;
      float lp, gp = 0.f, lm, gm = 0.f;
      LINK::template eval<GRAD>(sgn * (mu + d), lp, gp);
      LINK::template eval<GRAD>(sgn * (mu - d), lm, gm);
      ell += w * (lp + lm);
      if (GRAD) {
        am += w * (gp + gm);
        av += (w * x) * (gp - gm);              // (the product of the two fp32 values)
      }
    }
    if (GRAD) {
      dmu = sgn * am;
      dvar = sgn * av / fmaxf(sd, 1e-30f);      // (var = 0: the pair differences are exactly 0, and so is the result)
    }
    return ell;
  }
  static __device__ __forceinline__ double lp(const Cls&, double mu, double var, double sgn) {
    if (std::is_same<LINK, LinkProbit>::value) return log(0.5 * erfc(-(sgn * mu / sqrt(1.0 + var)) * kInvSqrt2));
    // log sigma(z) = min(z, 0) - log1p(exp(-|z|))
    return gh_lse(mu, var, [sgn](double f) {
      const double z = sgn * f;
      return fmin(z, 0.0) - log1p(exp(-fabs(z)));
    });
  }
  static __device__ __forceinline__ double tail(const Cls&, double) { return 0.0; }
};

// Closed form.  With m = mu + var / 2:  ell = y mu - exp(m) - lgamma(y + 1),  d ell / d mu = y - exp(m),  d ell / d var = -exp(m) / 2.
// y is a non-negative float and is not checked.  exp(m) overflows fp32 above m ~ 88.7: value and gradients are then inf, as the
// formula says -- nothing is clamped.   lp = logsumexp_k( log w^_k + y f_k - exp(f_k) ),  tail = -lgamma(y + 1)
struct Poisson {
  using real = double;
  static constexpr bool kHasParam = false;
  struct Args {
    Target y;
  };
  struct Cls {};
  static __device__ __forceinline__ Cls cls(const Args&, int) { return Cls{}; }
  template <class T>
  static __device__ __forceinline__ T target(const Args& a, int c, size_t b) { return (T)a.y.at(c, b); }
  template <bool GRAD>
  static __device__ __forceinline__ double element(const Cls&, double mu, double var, double y, double& dmu, double& dvar,
                                                   double&) {
#pragma clang fp contract(off)
    const double e = exp(mu + 0.5 * var);
    if (GRAD) {
      dmu = y - e;
      dvar = -0.5 * e;
    }
    return y * mu - e - lgamma(y + 1.0);
  }
  static __device__ __forceinline__ double lp(const Cls&, double mu, double var, double y) {
    return gh_lse(mu, var, [y](double f) { return y * f - exp(f); });
  }
  static __device__ __forceinline__ double tail(const Cls&, double y) { return -lgamma(y + 1.0); }
};

// With r_k = y - (mu + sqrt(2 var) x_k), a_k = r_k^2 / (nu sigma_c^2), q_k = r_k / (nu sigma_c^2 (1 + a_k)):
//   ell = K_c - (nu + 1) / 2 sum_k w^_k log1p(a_k),   K_c = lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi) / 2 - log_scale[c]
//   d ell / d mu           = (nu + 1) sum_{k>0} w^_k (q_k + q_-k)
//   d ell / d var          = (nu + 1) sum_{k>0} w^_k x_k (q_k - q_-k) / sqrt(2 var)
//   d ell / d log_scale[c] = (nu + 1) sum_{k>0} w^_k (r_k q_k + r_-k q_-k) - 1
// The nu-only part of K_c comes from the host, computed in double (`lognorm`): the two lgamma cancel in fp32 at large nu.
//   lp = logsumexp_k( log w^_k - (nu + 1) / 2 log1p(a_k) ),  tail = K_c
struct StudentT {
  using real = double;
  static constexpr bool kHasParam = true;
  struct Args {
    Target y;
    const float* log_scale;
    float df, lognorm;
  };
  struct Cls {
    double inv, np1, k;     // 1 / (nu sigma^2), nu + 1, K_c
  };
  static __device__ __forceinline__ Cls cls(const Args& a, int c) {
    const double ls = a.log_scale[c];
    return Cls{exp(-2.0 * ls) / (double)a.df, (double)a.df + 1.0, (double)a.lognorm - ls};
  }
  template <class T>
  static __device__ __forceinline__ T target(const Args& a, int c, size_t b) { return (T)a.y.at(c, b); }
  template <bool GRAD>
  static __device__ __forceinline__ double element(const Cls& p, double mu, double var, double y, double& dmu, double& dvar,
                                                   double& dpar) {
#pragma clang fp contract(off)
    const double sd = sqrt(2.0 * var), r0 = y - mu;
    double el = 0.0, am = 0.0, av = 0.0, ap = 0.0;
#pragma unroll
    for (int k = 0; k < kGhPairs; ++k) {
      const double d = sd * kGhX[k];
      const double rp = r0 - d, rm = r0 + d;                      // residuals at the nodes +x_k, -x_k
      const double ap_ = rp * rp * p.inv, am_ = rm * rm * p.inv;
      el += kGhW[k] * (log1p(ap_) + log1p(am_));
      if (GRAD) {
        const double qp = rp * p.inv / (1.0 + ap_), qm = rm * p.inv / (1.0 + am_);
        am += kGhW[k] * (qp + qm);
        av += (kGhW[k] * kGhX[k]) * (qp - qm);
        ap += kGhW[k] * (rp * qp + rm * qm);
      }
    }
    if (GRAD) {
      dmu = p.np1 * am;
      dvar = p.np1 * av / fmax(sd, 1e-300);       // (var = 0: the pair differences are exactly 0, and so is the result)
      dpar = p.np1 * ap - 1.0;
    }
    return p.k - 0.5 * p.np1 * el;
  }
  static __device__ __forceinline__ double lp(const Cls& p, double mu, double var, double y) {
    const double inv = p.inv, hnp1 = 0.5 * p.np1;
    return gh_lse(mu, var, [inv, hnp1, y](double f) {
      const double r = y - f;
      return -hnp1 * log1p(r * r * inv);
    });
  }
  static __device__ __forceinline__ double tail(const Cls& p, double) { return p.k; }
};

// lp = log N(y; mu, var + exp(obs_log_var[c])), closed form.  No `element`: the ELBO term and the parameter's gradient are
// gauss_lik.hip's (another launch layout and the reference's mean over outputs)
struct Gauss {
  using real = double;
  static constexpr bool kHasParam = true;
  struct Args {
    Target y;
    const float* obs_log_var;
  };
  struct Cls {
    double obs;
  };
  static __device__ __forceinline__ Cls cls(const Args& a, int c) { return Cls{exp((double)a.obs_log_var[c])}; }
  template <class T>
  static __device__ __forceinline__ T target(const Args& a, int c, size_t b) { return (T)a.y.at(c, b); }
  static __device__ __forceinline__ double lp(const Cls& p, double mu, double var, double y) {
    const double v = var + p.obs, r = y - mu;
    return -kHalfLog2Pi - 0.5 * (log(v) + r * r / v);
  }
  static __device__ __forceinline__ double tail(const Cls&, double) { return 0.0; }
};

}  // namespace vargp
