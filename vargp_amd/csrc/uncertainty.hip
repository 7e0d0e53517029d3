// Predictive entropy of the classification likelihoods, split into its two sources: the last stage (mu, var) -> (total, expected,
// mi).  Not in the reference.  mu, var [S, C, B] are the predictive moments of f under hyper-sample s; all values are in nats.
//   total    = H[ E p(y | theta, f) ]      the entropy of the predictive distribution itself
//   expected = E H[ p(y | theta, f) ]      what every sample agrees on: noise (aleatoric)
//   mi       = max(total - expected, 0)    the mutual information of the label and (theta, f): lack of knowledge (epistemic)
// Softmax, eps [S, F, C, B]; the P = S F samples are p_sf = softmax_c(mu_s + sqrt(var_s) eps_sf):
//   probs[b,c] = mean_sf p_sf[c,b]       total[b] = - sum_c probs[b,c] log probs[b,c]  (0 log 0 = 0)
//   expected[b] = mean_sf H_sf[b],       H_sf = Z - sum_c p_c f_c,  Z = logsumexp_c f_c (max-shifted): log(0) is never evaluated
// Bernoulli (either link), per output (c, b), with f_k = mu + sqrt(2 var) x_k and (x_k, w^_k) the 20-node Gauss-Hermite rule of
// lik.h -- as in indep_lik.hip and lpd.hip the quadrature sums are the DEFINITION, for the probit link too (one rule on both
// sides of Jensen's inequality, so that total_out >= expected_out holds exactly) -- and h(p) = -p log p - (1 - p) log(1 - p):
//   p_out = mean_s sum_k w^_k Lambda(f_k)     total_out = h(p_out)     expected_out = mean_s sum_k w^_k h(Lambda(f_k))
//   mi_out = max(total_out - expected_out, 0);     total, expected, mi [B] = the sums over c of the three
// The 1 - p_out inside h(p_out) is accumulated like p_out itself, mean_s sum_k w^_k Lambda(-f_k): the same number (the weights
// sum to one), with its own digits where p_out is within 1e-16 of one.
// h(Lambda(f)) = -(e^lp lp + e^lm lm) with lp = log Lambda(f), lm = log Lambda(-f) from the links' fp64 forms (lik.h): finite and
// correct at |f| = 30 and beyond.
//
// Launch layout (lpd.hip's).  Lanes run along b (mu / var / eps are contiguous in b: coalesced loads); workgroup j owns the 64
// points [64 j, 64 j + 64).
//   Softmax, two sweeps.  Sweep 1: the nw = min(S F, 8) waves split the samples (wave w: p = w, w + nw, ...); one pass over c per
//   sample keeps the running (max, sum exp, sum exp f) and gives Z_p and H_p; Z_p goes to the workspace [S F][B] (doubles: no
//   factor C), the waves' entropy sums are combined through LDS in wave order and expected[b] follows Z in the workspace [B].
//   Sweep 2: the min(C, 8) waves split the classes (wave w: c = w, w + nw, ...), walk the samples in order, form
//   probs[b,c] = mean_p exp(f_pc - Z_p) and add -p log p; wave 0 combines the waves' sums in wave order and writes total,
//   expected and mi.  Nothing of size S F C B is written; eps is read once per sweep.
//   Bernoulli, one kernel: c outermost; the min(S, 8) waves split the hyper-samples, their (sum p, sum 1 - p, sum h) triples of
//   output c meet in LDS (two buffers, one barrier per output) and wave 0 forms the output's four values and keeps the sums over c.
// No float atomics: every sum has a fixed order and two runs are bitwise equal.  Precision: inputs and outputs are fp32; element
// arithmetic and every sum run in fp64, mi is subtracted in fp64 BEFORE rounding (it can be 1e-6 of total), so each output is the
// definition's value rounded once.
#include "lik.h"

namespace vargp {

constexpr int kUncMaxWaves = 8;

__device__ __forceinline__ double neg_plogp(double p) { return p > 0.0 ? -p * log(p) : 0.0; }

// grid (ceil(B / 64)), block 64 nw.  Z [S F][B] and expected [B] into the workspace
__global__ __launch_bounds__(kUncMaxWaves* kWave) void unc_softmax_sweep1_kernel(const float* __restrict__ mu,
                                                                                  const float* __restrict__ var,
                                                                                  const float* __restrict__ eps,
                                                                                  double* __restrict__ Z, double* __restrict__ expd,
                                                                                  int S, int F, int C, int B) {
  __shared__ double red[kUncMaxWaves][kWave];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const size_t b = (size_t)blockIdx.x * kWave + lane;
  const bool live = b < (size_t)B;
  const int SF = S * F;
  double hsum = 0.0;
  if (live) {
    for (int p = w; p < SF; p += nw) {
      const int s = p / F;
      // m: running maximum; se = sum_c exp(f_c - m); sf = sum_c exp(f_c - m) f_c
      double m = -kInf, se = 0.0, sf = 0.0;
      for (int c = 0; c < C; ++c) {
        const size_t i = ((size_t)s * C + c) * (size_t)B + b, j = ((size_t)p * C + c) * (size_t)B + b;
        const double f = (double)mu[i] + sqrt((double)var[i]) * (double)eps[j];
        if (f > m) {
          const double r = exp(m - f);           // (the first class: exp(-inf) = 0 times the empty sums)
          se = se * r + 1.0;
          sf = sf * r + f;
          m = f;
        } else {
          const double e = exp(f - m);
          se += e;
          sf += e * f;
        }
      }
      const double z = m + log(se);
      Z[(size_t)p * (size_t)B + b] = z;
      hsum += z - sf / se;
    }
  }
  red[w][lane] = hsum;
  __syncthreads();
  if (w != 0 || !live) return;
  for (int q = 1; q < nw; ++q) hsum += red[q][lane];
  expd[b] = hsum / (double)SF;
}

// grid (ceil(B / 64)), block 64 nw; the waves split the classes.  probs [B, C] (may be NULL), total, expected, mi [B]
__global__ __launch_bounds__(kUncMaxWaves* kWave) void unc_softmax_sweep2_kernel(
    const float* __restrict__ mu, const float* __restrict__ var, const float* __restrict__ eps, const double* __restrict__ Z,
    const double* __restrict__ expd, float* __restrict__ probs, float* __restrict__ total, float* __restrict__ expected,
    float* __restrict__ mi, int S, int F, int C, int B) {
  __shared__ double red[kUncMaxWaves][kWave];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const size_t b = (size_t)blockIdx.x * kWave + lane;
  const bool live = b < (size_t)B;
  const int SF = S * F;
  double tot = 0.0;
  if (live) {
    for (int c = w; c < C; c += nw) {
      double acc = 0.0;
      for (int s = 0; s < S; ++s) {
        const size_t i = ((size_t)s * C + c) * (size_t)B + b;
        const double m = (double)mu[i], sd = sqrt((double)var[i]);
        for (int f = 0; f < F; ++f) {
          const size_t p = (size_t)s * F + f;
          acc += exp(m + sd * (double)eps[(p * C + c) * (size_t)B + b] - Z[p * (size_t)B + b]);
        }
      }
      const double pc = acc / (double)SF;
      if (probs) probs[b * (size_t)C + c] = (float)pc;
      tot += neg_plogp(pc);
    }
  }
  red[w][lane] = tot;
  __syncthreads();
  if (w != 0 || !live) return;
  for (int q = 1; q < nw; ++q) tot += red[q][lane];
  const double ex = expd[b];
  total[b] = (float)tot;
  expected[b] = (float)ex;
  mi[b] = (float)fmax(tot - ex, 0.0);
}

// One output under one hyper-sample: p = sum_k w^_k Lambda(f_k), q = sum_k w^_k Lambda(-f_k), h = sum_k w^_k h(Lambda(f_k)), the
// nodes in +-x_k pairs
template <class LINK>
__device__ __forceinline__ void unc_bernoulli_element(double mu, double var, double& p, double& q, double& h) {
  const double sd = sqrt(2.0 * var);
  p = 0.0;
  q = 0.0;
  h = 0.0;
#pragma unroll
  for (int k = 0; k < kGhPairs; ++k) {
    const double d = sd * kGhX[k];
    double pk = 0.0, qk = 0.0, hk = 0.0;
#pragma unroll
    for (int sg = 0; sg < 2; ++sg) {
      const double f = sg ? mu - d : mu + d;
      const double lp = LINK::logp(f), lm = LINK::logp(-f);
      const double ep = exp(lp), em = exp(lm);
      pk += ep;
      qk += em;
      hk -= (ep > 0.0 ? ep * lp : 0.0) + (em > 0.0 ? em * lm : 0.0);
    }
    p += kGhW[k] * pk;
    q += kGhW[k] * qk;
    h += kGhW[k] * hk;
  }
}

// grid (ceil(B / 64)), block 64 nw; the waves split the hyper-samples of one output at a time
template <class LINK>
__global__ __launch_bounds__(kUncMaxWaves* kWave) void unc_bernoulli_kernel(
    const float* __restrict__ mu, const float* __restrict__ var, float* __restrict__ probs, float* __restrict__ total,
    float* __restrict__ expected, float* __restrict__ mi, float* __restrict__ total_out, float* __restrict__ expected_out,
    float* __restrict__ mi_out, int S, int C, int B) {
  __shared__ double red[2][kUncMaxWaves][3][kWave];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const size_t b = (size_t)blockIdx.x * kWave + lane;
  const bool live = b < (size_t)B;
  double tot = 0.0, ex = 0.0, info = 0.0;
  for (int c = 0; c < C; ++c) {                 // (every wave walks every c: the barrier below is reached by all of them)
    double ps = 0.0, qs = 0.0, hs = 0.0;
    if (live) {
      for (int s = w; s < S; s += nw) {
        const size_t i = ((size_t)s * C + c) * (size_t)B + b;
        double p, q, h;
        unc_bernoulli_element<LINK>((double)mu[i], (double)var[i], p, q, h);
        ps += p;
        qs += q;
        hs += h;
      }
    }
    double(*buf)[3][kWave] = red[c & 1];         // two buffers: the waves fill c + 1's while wave 0 still reads c's
    buf[w][0][lane] = ps;
    buf[w][1][lane] = qs;
    buf[w][2][lane] = hs;
    __syncthreads();
    if (w != 0 || !live) continue;
    for (int k = 1; k < nw; ++k) {
      ps += buf[k][0][lane];
      qs += buf[k][1][lane];
      hs += buf[k][2][lane];
    }
    const double p = ps / (double)S, e = hs / (double)S;
    const double t = neg_plogp(p) + neg_plogp(qs / (double)S), m = fmax(t - e, 0.0);
    const size_t o = (size_t)c * (size_t)B + b;
    if (probs) probs[b * (size_t)C + c] = (float)p;
    if (total_out) total_out[o] = (float)t;
    if (expected_out) expected_out[o] = (float)e;
    if (mi_out) mi_out[o] = (float)m;
    tot += t;
    ex += e;
    info += m;
  }
  if (w != 0 || !live) return;
  total[b] = (float)tot;
  expected[b] = (float)ex;
  mi[b] = (float)info;
}

static int unc_waves(int64_t n) { return (int)(n < kUncMaxWaves ? n : kUncMaxWaves); }

}  // namespace vargp

using namespace vargp;

extern "C" size_t vargp_softmax_uncertainty_workspace_bytes(int S, int F, int C, int B) {
  (void)C;
  if (S <= 0 || F <= 0 || B <= 0) return 0;
  return ((size_t)S * (size_t)F + 1) * (size_t)B * sizeof(double);
}

extern "C" int vargp_softmax_uncertainty(const float* mu, const float* var, const float* eps, float* probs, float* total,
                                         float* expected, float* mi, int S, int F, int C, int B, float* ws, size_t ws_bytes,
                                         vargp_stream_t stream) {
  VARGP_REQUIRE(mu && var && eps && total && expected && mi && S > 0 && F > 0 && C > 0 && B > 0,
                "softmax_uncertainty: bad arguments");
  VARGP_REQUIRE((int64_t)S * F <= INT32_MAX, "softmax_uncertainty: S * F too large");
  VARGP_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 7) == 0 &&
                    ws_bytes >= vargp_softmax_uncertainty_workspace_bytes(S, F, C, B),
                "softmax_uncertainty: workspace missing, not 8-byte aligned or too small");
  double* Z = reinterpret_cast<double*>(ws);
  double* expd = Z + (size_t)S * (size_t)F * (size_t)B;
  const int nbx = cdiv(B, kWave);
  hipLaunchKernelGGL(unc_softmax_sweep1_kernel, dim3(nbx), dim3(kWave * unc_waves((int64_t)S * F)), 0, as_stream(stream), mu,
                     var, eps, Z, expd, S, F, C, B);
  hipLaunchKernelGGL(unc_softmax_sweep2_kernel, dim3(nbx), dim3(kWave * unc_waves(C)), 0, as_stream(stream), mu, var, eps, Z,
                     expd, probs, total, expected, mi, S, F, C, B);
  return check_launch("softmax_uncertainty");
}

extern "C" int vargp_bernoulli_uncertainty(const float* mu, const float* var, int link, float* probs, float* total,
                                           float* expected, float* mi, float* total_out, float* expected_out, float* mi_out,
                                           int S, int C, int B, vargp_stream_t stream) {
  VARGP_REQUIRE(mu && var && total && expected && mi && S > 0 && C > 0 && B > 0, "bernoulli_uncertainty: bad arguments");
  VARGP_REQUIRE(link == 0 || link == 1, "bernoulli_uncertainty: link must be 0 (probit) or 1 (logit)");
  const dim3 grid(cdiv(B, kWave)), block(kWave * unc_waves(S));
  if (link == 0)
    hipLaunchKernelGGL(unc_bernoulli_kernel<LinkProbit>, grid, block, 0, as_stream(stream), mu, var, probs, total, expected, mi,
                       total_out, expected_out, mi_out, S, C, B);
  else
    hipLaunchKernelGGL(unc_bernoulli_kernel<LinkLogit>, grid, block, 0, as_stream(stream), mu, var, probs, total, expected, mi,
                       total_out, expected_out, mi_out, S, C, B);
  return check_launch("bernoulli_uncertainty");
}
