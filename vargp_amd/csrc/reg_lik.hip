// Two regression likelihoods with independent outputs.  Not in the reference.
//   Poisson, log link (counts):      p(y | f) = exp(y f - exp(f)) / y!
//   Student-t, fixed nu (outliers):  p(y | f) = t_nu((y - f) / sigma_c) / sigma_c,  sigma_c = exp(log_scale[c])
// mu, var [S, C, B]; y [C, B] with row stride ldy, or one row [B] shared by every output (ldy = 0).  Both values SUM over the
// outputs and take the mean over the hyper-samples, nll = - sum_b sum_c mean_s ell[s,c,b] -- the ELBO of C independent outputs,
// as bernoulli_lik.hip has it; that is C times the convention of gauss_lik.hip, which keeps the reference's mean over outputs.
//
// Poisson: closed form.  With m = mu + var / 2:
//   ell = y mu - exp(m) - lgamma(y + 1),   d ell / d mu = y - exp(m),   d ell / d var = -exp(m) / 2
// y is a non-negative float and is not checked.  exp(m) overflows fp32 above m ~ 88.7: value and gradients are then inf, as
// the formula says -- nothing is clamped.
//
// Student-t: the expectation under f ~ N(mu, var) is DEFINED by the 20-node Gauss-Hermite rule, as in
// bernoulli_lik.hip.  With r_k = y - (mu + sqrt(2 var) x_k), a_k = r_k^2 / (nu sigma_c^2), q_k = r_k / (nu sigma_c^2 (1 + a_k)):
//   ell = K_c - (nu + 1) / 2 sum_k w^_k log1p(a_k),   K_c = lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi) / 2 - log_scale[c]
//   d ell / d mu           = (nu + 1) sum_{k>0} w^_k (q_k + q_-k)
//   d ell / d var          = (nu + 1) sum_{k>0} w^_k x_k (q_k - q_-k) / sqrt(2 var)
//   d ell / d log_scale[c] = (nu + 1) sum_{k>0} w^_k (r_k q_k + r_-k q_-k) - 1
// The nodes are visited in +-x_k pairs and the pair difference carries the variance gradient; at var = 0 it is exactly 0 and so
// is the result.  The nu-only part of K_c comes from the host, computed in double (`lognorm`): the two lgamma cancel in fp32 at
// large nu.
//
// Launch layout (that of bernoulli_lik.hip): workgroup (c, j) of a (C, nsplit <= 32) grid handles the elements
// e = j * 256 + tid (+ nsplit * 256 ...) of output c's (S, B) slab, writes gmu / gvar and leaves its partial sums in the
// caller's scratch -- values in ws[c * nsplit + j], Student-t's d / d log_scale behind them; one wavefront then adds them in
// index order.  No float atomics: every sum has a fixed order, two runs are bitwise equal, and the backward's value equals the
// forward's bit for bit (contraction is off in the element arithmetic so that the two instantiations round alike).
// Precision: inputs and outputs are fp32; an element's arithmetic, the partial sums (ws is read as doubles) and the adder run
// in fp64, so every output is the formula's value rounded ONCE to fp32 (the overflow to inf above m ~ 88.7 is that rounding's).
// The launch is bound by latency, not by the fp64 rate.
#include "common.h"

namespace vargp {

constexpr int kRegThreads = 256;
constexpr int kRegMaxSplit = 32;
constexpr int kRegPairs = 10;
// x, w = numpy.polynomial.hermite.hermgauss(20); the positive half x[10:] and w[10:] / sqrt(pi)  (the table of bernoulli_lik.hip)
__device__ constexpr double kRegX[kRegPairs] = {0.24534070830090124, 0.73747372854539439, 1.2340762153953231,
                                                1.7385377121165861,  2.2549740020892757,  2.7888060584281305,
                                                3.3478545673832163,  3.9447640401156252,  4.6036824495507442,
                                                5.3874808900112328};
__device__ constexpr double kRegW[kRegPairs] = {0.26079306344955488,    0.16173933398399998,    0.061506372063976897,
                                                0.013997837447101022,   0.00183010313108049,    0.00012882627996192928,
                                                4.402121090230851e-06,  6.127490259982928e-08,  2.4820623623151755e-10,
                                                1.2578006724379234e-13};

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// block_sum of common.h in fp64: the same order (wave tree, then the waves in index order)
template <int NT>
__device__ __forceinline__ double block_sum_d(double v, double* red /* >= NT/64 doubles of LDS */) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) t += red[i];
  return t;
}

// A likelihood: Args (by value into the kernel), Cls = what is constant over one output, and
//   element<GRAD>(cls, mu, var, y, dmu, dvar, dpar) = ell and (GRAD) d ell / d (mu, var, the output's own parameter)
struct Poisson {
  static constexpr bool kHasParam = false;
  struct Args {};
  struct Cls {};
  static __device__ __forceinline__ Cls cls(const Args&, int) { return Cls{}; }
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
};

struct StudentT {
  static constexpr bool kHasParam = true;
  struct Args {
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
  template <bool GRAD>
  static __device__ __forceinline__ double element(const Cls& p, double mu, double var, double y, double& dmu, double& dvar,
                                                   double& dpar) {
#pragma clang fp contract(off)
    const double sd = sqrt(2.0 * var), r0 = y - mu;
    double el = 0.0, am = 0.0, av = 0.0, ap = 0.0;
#pragma unroll
    for (int k = 0; k < kRegPairs; ++k) {
      const double d = sd * kRegX[k];
      const double rp = r0 - d, rm = r0 + d;                      // residuals at the nodes +x_k, -x_k
      const double ap_ = rp * rp * p.inv, am_ = rm * rm * p.inv;
      el += kRegW[k] * (log1p(ap_) + log1p(am_));
      if (GRAD) {
        const double qp = rp * p.inv / (1.0 + ap_), qm = rm * p.inv / (1.0 + am_);
        am += kRegW[k] * (qp + qm);
        av += (kRegW[k] * kRegX[k]) * (qp - qm);
        ap += kRegW[k] * (rp * qp + rm * qm);
      }
    }
    if (GRAD) {
      dmu = p.np1 * am;
      dvar = p.np1 * av / fmax(sd, 1e-300);       // (var = 0: the pair differences are exactly 0, and so is the result)
      dpar = p.np1 * ap - 1.0;
    }
    return p.k - 0.5 * p.np1 * el;
  }
};

// grid (C, nsplit).  GRAD: gmu, gvar = seed[0] * d nll / d (mu, var).  vpart (may be NULL): [C * nsplit] sums of ell;
// ppart (GRAD, kHasParam): [C * nsplit] sums of d ell / d parameter
template <class LIK, bool GRAD>
__global__ __launch_bounds__(kRegThreads) void reg_nll_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                              const float* __restrict__ y, int64_t ldy, typename LIK::Args args,
                                                              const float* __restrict__ seed, float* __restrict__ gmu,
                                                              float* __restrict__ gvar, double* __restrict__ vpart,
                                                              double* __restrict__ ppart, int S, int C, int B) {
  __shared__ double red[kRegThreads / kWave];
  const int c = blockIdx.x, nsplit = gridDim.y;
  const int SB = S * B;
  const int64_t CB = (int64_t)C * B;
  const double g = GRAD ? -(double)seed[0] / (double)S : 0.0;
  const typename LIK::Cls cls = LIK::cls(args, c);
  const float* yc = y + (int64_t)c * ldy;
  double acc = 0.0, pacc = 0.0;
  for (int64_t e = (int64_t)blockIdx.y * kRegThreads + threadIdx.x; e < SB; e += (int64_t)nsplit * kRegThreads) {
    const int s = (int)(e / B), b = (int)(e - (int64_t)s * B);
    const int64_t i = (int64_t)s * CB + (int64_t)c * B + b;
    double dmu = 0.0, dvar = 0.0, dpar = 0.0;
    acc += LIK::template element<GRAD>(cls, (double)mu[i], (double)var[i], (double)yc[b], dmu, dvar, dpar);
    if (GRAD) {
      gmu[i] = (float)(g * dmu);
      gvar[i] = (float)(g * dvar);
      pacc += dpar;
    }
  }
  if (vpart) {
    acc = block_sum_d<kRegThreads>(acc, red);
    if (threadIdx.x == 0) vpart[(int64_t)c * nsplit + blockIdx.y] = acc;
  }
  if (GRAD && LIK::kHasParam) {
    pacc = block_sum_d<kRegThreads>(pacc, red);
    if (threadIdx.x == 0) ppart[(int64_t)c * nsplit + blockIdx.y] = pacc;
  }
}

// one wavefront.  nll (may be NULL) = -(1 / S) sum_i vpart[i]: lanes stride the array in index order, then the wave tree;
// gpar (may be NULL): gpar[c] = -(seed / S) sum_j ppart[c * nsplit + j], one lane per output, j in order
__global__ __launch_bounds__(kWave) void reg_finish_kernel(const double* __restrict__ vpart, const double* __restrict__ ppart,
                                                           int C, int nsplit, double inv_s, const float* __restrict__ seed,
                                                           float* __restrict__ nll, float* __restrict__ gpar) {
  if (nll) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < C * nsplit; i += kWave) acc += vpart[i];
    acc = wave_sum_d(acc);
    if (threadIdx.x == 0) nll[0] = (float)(-inv_s * acc);
  }
  if (gpar) {
    const double g = -(double)seed[0] * inv_s;
    for (int c = threadIdx.x; c < C; c += kWave) {
      double acc = 0.0;
      for (int j = 0; j < nsplit; ++j) acc += ppart[(int64_t)c * nsplit + j];
      gpar[c] = (float)(g * acc);
    }
  }
}

// rate[s, c, b] = E exp(f) = exp(mu + var / 2)
__global__ __launch_bounds__(kRegThreads) void poisson_predict_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                                      float* __restrict__ rate, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kRegThreads + threadIdx.x;
  if (i < n) rate[i] = (float)exp((double)mu[i] + 0.5 * (double)var[i]);
}

static int reg_nsplit(int S, int B) {
  const int n = cdiv((int64_t)S * B, kRegThreads);
  return n < kRegMaxSplit ? n : kRegMaxSplit;
}

template <class LIK>
static size_t reg_workspace_bytes(int S, int C, int B) {
  if (S <= 0 || C <= 0 || B <= 0) return 0;
  return (size_t)C * reg_nsplit(S, B) * sizeof(double) * (LIK::kHasParam ? 2 : 1);
}

template <class LIK, bool GRAD>
static int reg_launch(const char* what, const float* mu, const float* var, const float* y, int64_t ldy,
                      typename LIK::Args args, const float* seed, float* gmu, float* gvar, float* gpar, float* nll, int S, int C,
                      int B, float* ws, hipStream_t st) {
  const int nsplit = reg_nsplit(S, B);
  double* part = reinterpret_cast<double*>(ws);                   // (8-byte aligned: REG_CHECK_TARGET)
  double* vpart = nll ? part : nullptr;
  double* ppart = GRAD && LIK::kHasParam ? part + (size_t)C * nsplit : nullptr;
  hipLaunchKernelGGL((reg_nll_kernel<LIK, GRAD>), dim3(C, nsplit), dim3(kRegThreads), 0, st, mu, var, y, ldy, args, seed, gmu,
                     gvar, vpart, ppart, S, C, B);
  if (nll || ppart)
    hipLaunchKernelGGL(reg_finish_kernel, dim3(1), dim3(kWave), 0, st, vpart, ppart, C, nsplit, 1.0 / (double)S, seed, nll,
                       ppart ? gpar : nullptr);
  return check_launch(what);
}

}  // namespace vargp

using namespace vargp;

#define REG_CHECK_COMMON(what)                                                                                          \
  VARGP_REQUIRE(mu && var && S > 0 && C > 0 && B > 0, what ": bad arguments");                                          \
  VARGP_REQUIRE((int64_t)S * B <= INT32_MAX && (int64_t)C * kRegMaxSplit <= INT32_MAX, what ": S * B or C too large")
#define REG_CHECK_TARGET(what)                                                                                          \
  VARGP_REQUIRE(y && (ldy == 0 || ldy >= B), what ": y must be given, ldy 0 or >= B");                                 \
  VARGP_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 8 == 0, what ": ws must be 8-byte aligned")

extern "C" size_t vargp_poisson_workspace_bytes(int S, int C, int B) { return reg_workspace_bytes<Poisson>(S, C, B); }

extern "C" int vargp_poisson_nll_fwd(const float* mu, const float* var, const float* y, int64_t ldy, float* nll, int S, int C,
                                     int B, float* ws, size_t ws_bytes, vargp_stream_t stream) {
  REG_CHECK_COMMON("poisson_nll_fwd");
  REG_CHECK_TARGET("poisson_nll_fwd");
  VARGP_REQUIRE(nll && ws && ws_bytes >= vargp_poisson_workspace_bytes(S, C, B), "poisson_nll_fwd: nll / workspace");
  return reg_launch<Poisson, false>("poisson_nll_fwd", mu, var, y, ldy, Poisson::Args{}, nullptr, nullptr, nullptr, nullptr, nll,
                                    S, C, B, ws, as_stream(stream));
}

extern "C" int vargp_poisson_nll_bwd(const float* mu, const float* var, const float* y, int64_t ldy, const float* seed,
                                     float* gmu, float* gvar, float* nll, int S, int C, int B, float* ws, size_t ws_bytes,
                                     vargp_stream_t stream) {
  REG_CHECK_COMMON("poisson_nll_bwd");
  REG_CHECK_TARGET("poisson_nll_bwd");
  VARGP_REQUIRE(seed && gmu && gvar, "poisson_nll_bwd: bad arguments");
  VARGP_REQUIRE(!nll || (ws && ws_bytes >= vargp_poisson_workspace_bytes(S, C, B)), "poisson_nll_bwd: workspace too small");
  return reg_launch<Poisson, true>("poisson_nll_bwd", mu, var, y, ldy, Poisson::Args{}, seed, gmu, gvar, nullptr, nll, S, C, B,
                                   ws, as_stream(stream));
}

extern "C" int vargp_poisson_predict(const float* mu, const float* var, float* rate, int S, int C, int B,
                                     vargp_stream_t stream) {
  REG_CHECK_COMMON("poisson_predict");
  const int64_t n = (int64_t)S * C * B;
  VARGP_REQUIRE(rate && n <= (int64_t)INT32_MAX * kRegThreads, "poisson_predict: bad arguments");
  hipLaunchKernelGGL(poisson_predict_kernel, dim3(cdiv(n, kRegThreads)), dim3(kRegThreads), 0, as_stream(stream), mu, var, rate,
                     n);
  return check_launch("poisson_predict");
}

extern "C" size_t vargp_studentt_workspace_bytes(int S, int C, int B) { return reg_workspace_bytes<StudentT>(S, C, B); }

extern "C" int vargp_studentt_nll_fwd(const float* mu, const float* var, const float* y, int64_t ldy, const float* log_scale,
                                      float df, float lognorm, float* nll, int S, int C, int B, float* ws, size_t ws_bytes,
                                      vargp_stream_t stream) {
  REG_CHECK_COMMON("studentt_nll_fwd");
  REG_CHECK_TARGET("studentt_nll_fwd");
  VARGP_REQUIRE(log_scale && df > 0.f, "studentt_nll_fwd: log_scale must be given, df > 0");
  VARGP_REQUIRE(nll && ws && ws_bytes >= vargp_studentt_workspace_bytes(S, C, B), "studentt_nll_fwd: nll / workspace");
  return reg_launch<StudentT, false>("studentt_nll_fwd", mu, var, y, ldy, StudentT::Args{log_scale, df, lognorm}, nullptr,
                                     nullptr, nullptr, nullptr, nll, S, C, B, ws, as_stream(stream));
}

extern "C" int vargp_studentt_nll_bwd(const float* mu, const float* var, const float* y, int64_t ldy, const float* log_scale,
                                      float df, float lognorm, const float* seed, float* gmu, float* gvar, float* g_log_scale,
                                      float* nll, int S, int C, int B, float* ws, size_t ws_bytes, vargp_stream_t stream) {
  REG_CHECK_COMMON("studentt_nll_bwd");
  REG_CHECK_TARGET("studentt_nll_bwd");
  VARGP_REQUIRE(log_scale && df > 0.f, "studentt_nll_bwd: log_scale must be given, df > 0");
  VARGP_REQUIRE(seed && gmu && gvar && g_log_scale, "studentt_nll_bwd: bad arguments");
  VARGP_REQUIRE(ws && ws_bytes >= vargp_studentt_workspace_bytes(S, C, B), "studentt_nll_bwd: workspace too small");
  return reg_launch<StudentT, true>("studentt_nll_bwd", mu, var, y, ldy, StudentT::Args{log_scale, df, lognorm}, seed, gmu,
                                    gvar, g_log_scale, nll, S, C, B, ws, as_stream(stream));
}
