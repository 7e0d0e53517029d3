// Gaussian sites of the softmax likelihood over a whole data set (sites.py: fit_q_softmax_; nothing of this is in the reference).
// q factorises over the C classes, so conjugate-computation VI still has one Gaussian site per (class, point); the classes of a
// point are coupled only in how the site parameters are COMPUTED: all C marginals f_c ~ N(mu_cn, var_cn) enter one expectation
// over p = softmax(f).  With the F draws f = mu + sqrt(var) eps of a point:
//   ell_n   = mu_{y_n, n} - mean_f logsumexp(f)                         (E f_y = mu_y exactly)
//   Ep_c    = mean_f p_c,   Ev_c = mean_f p_c (1 - p_c)                 (Bonnet: d ell / d mu_c = [y = c] - E p_c;
//                                                                         Price:  d ell / d var_c = -1/2 E p_c (1 - p_c) <= 0)
//   lam2_cn = w_n Ev_c,     lam1_cn = w_n ([y_n = c] - Ep_c) + lam2_cn mu_cn
//   sums    = (sum_n w_n ell_n, sum_cn lam2_cn, #{n: w_n != 0}, sum_n w_n)
// Per draw the logits are shifted by their maximum and one exp per class is taken.  Lanes run over the points, so every row of
// the [C][N] operands and results is read and written coalesced; a lane walks the F draws of its point one after the other (the
// draws of a point are NOT split over waves: nothing measured says it would pay, and it would cost an LDS reduction of 2 C + 1
// accumulators per point).  The accumulators of Ep and Ev and the draw's logits live in registers for C <= kSmRegC and in LDS as
// [class][lane] above it (3 C x 64 floats: 96 KB at the limit C = kSmMaxC).
// Noise: eps [F][C][N] is read if given; else it is generated here, Philox group ((n F + f) ceil(C / 4) + j) of stream
// kStreamSite at step 0, element l of group j being class 4 j + l (one normal4 serves four classes), so the tensor need not
// exist.  vargp_softmax_site_noise writes out exactly those draws.
// A point of weight 0 is never evaluated: lam1 = lam2 = 0 and it adds exactly nothing.  The points are cut into at most
// kSmMaxChunks chunks (a multiple of 64 points each, from N alone); a chunk is one wave; its sums leave as four fp64 partials and
// a second launch adds them in ascending chunk order: no atomics, two calls on the same input are bitwise equal.
// vargp_softmax_site_grads (below the site kernel) is the same frame with other accumulators: the exact derivatives of the first
// sum for mu and var, per point, for the differentiable softmax site bound.
#include "common.h"
#include "elbo_rng.h"

namespace vargp {

constexpr uint32_t kStreamSite = 2;      // (elbo_rng.h: kStreamTheta = 0, kStreamF = 1)
constexpr int kSmRegC = 16;              // classes whose accumulators live in registers
constexpr int kSmMaxC = 128;
constexpr int kSmMaxChunks = 1024;

struct SmPlan {
  int64_t len;               // points per chunk, a multiple of 64
  int nch;
};
static SmPlan sm_plan(int N) {
  SmPlan o{};
  o.len = round_up(cdiv(N, kSmMaxChunks), 64);
  o.nch = cdiv(N, o.len);
  return o;
}

// what the site kernel and the gradient kernel both read
struct SmIn {
  const float *mu, *var, *w, *eps;
  const int64_t* y;
  uint64_t seed;
  SmPlan p;
  int C, N, F;
};

struct SmArgs : SmIn {
  float *lam1, *lam2, *sums;
  double* ps;                // partials [nch][4]
};

struct SmGradArgs : SmIn {
  const float* gout;         // [1]: the upstream seed, on the device
  float *gmu, *gvar;
};

// the draw's logits and the two accumulators per class of one lane (the sites: Ep, Ev; the gradients: sum p, sum p eps):
// registers (CR > 0) or LDS [class][lane] (CR == 0).  z, the draw's noise, is kept by the gradient kernel alone (a fourth LDS array
// there; in registers an array nobody touches does not exist)
template <int CR> struct SmStore {
  float e_[CR], p_[CR], v_[CR], z_[CR];
  __device__ __forceinline__ SmStore(float*, int, int) {}
  __device__ __forceinline__ float& e(int c) { return e_[c]; }
  __device__ __forceinline__ float& p(int c) { return p_[c]; }
  __device__ __forceinline__ float& v(int c) { return v_[c]; }
  __device__ __forceinline__ float& z(int c) { return z_[c]; }
};
template <> struct SmStore<0> {
  float* b_;
  int C_;
  __device__ __forceinline__ SmStore(float* lds, int C, int lane) : b_(lds + lane), C_(C) {}
  __device__ __forceinline__ float& e(int c) { return b_[c * 64]; }
  __device__ __forceinline__ float& p(int c) { return b_[(C_ + c) * 64]; }
  __device__ __forceinline__ float& v(int c) { return b_[(2 * C_ + c) * 64]; }
  __device__ __forceinline__ float& z(int c) { return b_[(3 * C_ + c) * 64]; }
};

// One draw f of point n: the logits f_c = mu_c + sqrt(var_c) eps_c into st.e (KEEPZ: eps_c into st.z), then st.e(c) = exp(f_c -
// max f) -> (the maximum, the sum of the exponentials).  The draw's noise is read from a.eps or generated, as the header says.
template <bool KEEPZ, int CR>
__device__ __forceinline__ void sm_draw(const SmIn& a, SmStore<CR>& st, int64_t n, int f, float& m, float& s) {
  const int C = a.C, nq = (C + 3) >> 2;
  const int NC = CR ? CR : C, NQ = CR ? (CR + 3) / 4 : nq;       // the class loops' trip counts (CR: constants, fully unrolled)
  constexpr int UC = CR ? CR : 1, UQ = CR ? (CR + 3) / 4 : 1;    // unroll counts: full in registers, none over a run-time C
  const int64_t N = a.N;
  m = -INFINITY;
#pragma unroll UQ
  for (int j = 0; j < NQ; ++j) {
    if (j < nq) {
      float z[4];
      if (a.eps) {
#pragma unroll
        for (int l = 0; l < 4; ++l) z[l] = 4 * j + l < C ? a.eps[((int64_t)f * C + 4 * j + l) * N + n] : 0.f;
      } else {
        normal4(a.seed, kStreamSite, ((uint64_t)n * (uint64_t)a.F + (uint64_t)f) * (uint64_t)nq + (uint64_t)j, 0u, z);
      }
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const int c = 4 * j + l;
        if (c < C) {
          const float fv = fmaf(sqrtf(a.var[c * N + n]), z[l], a.mu[c * N + n]);
          st.e(c) = fv;
          if constexpr (KEEPZ) st.z(c) = z[l];
          m = fmaxf(m, fv);
        }
      }
    }
  }
  s = 0.f;
#pragma unroll UC
  for (int c = 0; c < NC; ++c)
    if (c < C) { const float ev = expf(st.e(c) - m); st.e(c) = ev; s += ev; }
}

// p_c of the draw sm_draw left in st.e, inv = 1 / (the sum it returned)
template <int CR>
__device__ __forceinline__ float sm_prob(SmStore<CR>& st, int c, float inv) { return st.e(c) * inv; }

// grid (nch), 64 threads: lanes = points
template <int CR>
__global__ __launch_bounds__(64) void softmax_sites_kernel(const SmArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm_lds[];
  const int C = a.C, F = a.F, lane = threadIdx.x;
  const int NC = CR ? CR : C;                                    // the class loops' trip count (CR: a constant, fully unrolled)
  const int64_t N = a.N;
  const int64_t cbeg = (int64_t)blockIdx.x * a.p.len;
  const int64_t cend = cbeg + a.p.len < N ? cbeg + a.p.len : N;
  const float invF = 1.f / (float)F;
  SmStore<CR> st(sm_lds, C, lane);
  double s_ell = 0.0, s_l2 = 0.0, s_on = 0.0, s_w = 0.0;

  for (int64_t n = cbeg + lane; n < cend; n += 64) {
    const float wv = a.w ? a.w[n] : 1.f;
    if (wv == 0.f) {
      for (int c = 0; c < C; ++c) { a.lam1[c * N + n] = 0.f; a.lam2[c * N + n] = 0.f; }
      continue;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < C) { st.p(c) = 0.f; st.v(c) = 0.f; }
    float lse = 0.f;
    for (int f = 0; f < F; ++f) {
      float m, s;
      sm_draw<false>(a, st, n, f, m, s);
      const float inv = 1.f / s;
      lse += m + logf(s);
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < C) { const float pv = sm_prob(st, c, inv); st.p(c) += pv; st.v(c) = fmaf(pv, 1.f - pv, st.v(c)); }
    }
    const int64_t yv = a.y[n];
    double l2sum = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c < C) {
        const float l2 = wv * (st.v(c) * invF);
        const float l1 = fmaf(l2, a.mu[c * N + n], wv * ((yv == c ? 1.f : 0.f) - st.p(c) * invF));
        a.lam1[c * N + n] = l1;
        a.lam2[c * N + n] = l2;
        l2sum += (double)l2;
      }
    }
    const float muy = (yv >= 0 && yv < C) ? a.mu[yv * N + n] : NAN;       // a label outside [0, C): the bound is not a number
    s_ell += (double)wv * (double)(muy - lse * invF);
    s_l2 += l2sum;
    s_on += 1.0;
    s_w += (double)wv;
  }
  s_ell = wave_sum(s_ell);
  s_l2 = wave_sum(s_l2);
  s_on = wave_sum(s_on);
  s_w = wave_sum(s_w);
  if (lane == 0) {
    double* ps = a.ps + (int64_t)blockIdx.x * 4;
    ps[0] = s_ell; ps[1] = s_l2; ps[2] = s_on; ps[3] = s_w;
  }
}

// the chunks' partials in ascending chunk order, in fp64.  One workgroup; thread t < 4 owns sum t
__global__ __launch_bounds__(64) void softmax_sites_reduce_kernel(const SmArgs a) {
  const int t = threadIdx.x;
  if (t >= 4) return;
  double s = 0.0;
  for (int q = 0; q < a.p.nch; ++q) s += a.ps[(int64_t)q * 4 + t];
  a.sums[t] = (float)s;
}

// The exact derivatives of the F-sample estimate value = sum_n w_n [mu_{y_n, n} - mean_f logsumexp(f)] for the marginals, seeded by
// s = gout[0] (sites.py: softmax_site_bound; the pathwise derivative for var, NOT the Price estimate of the sites above):
//   gmu_cn  = s w_n ([y_n = c] - mean_f p_c)
//   gvar_cn = -s w_n / (2 sqrt(var_cn)) mean_f (p_c eps_c)   where var_cn > 0, else exactly 0
// The frame, the draws and every p are the site kernel's (sm_draw, sm_prob); the two accumulators per class are sum_f p_c and
// sum_f p_c eps_c.  Nothing is reduced over the points: no partials, no second launch.  A point of weight 0 is not evaluated and
// writes exact zeros.  grid (nch), 64 threads: lanes = points
template <int CR>
__global__ __launch_bounds__(64) void softmax_site_grads_kernel(const SmGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm_lds[];
  const int C = a.C, F = a.F, lane = threadIdx.x;
  const int NC = CR ? CR : C;
  constexpr int UC = CR ? CR : 1;
  const int64_t N = a.N;
  const int64_t cbeg = (int64_t)blockIdx.x * a.p.len;
  const int64_t cend = cbeg + a.p.len < N ? cbeg + a.p.len : N;
  const float invF = 1.f / (float)F, sg = a.gout[0];
  SmStore<CR> st(sm_lds, C, lane);

  for (int64_t n = cbeg + lane; n < cend; n += 64) {
    const float wv = a.w ? a.w[n] : 1.f;
    if (wv == 0.f) {
      for (int c = 0; c < C; ++c) { a.gmu[c * N + n] = 0.f; a.gvar[c * N + n] = 0.f; }
      continue;
    }
#pragma unroll UC
    for (int c = 0; c < NC; ++c)
      if (c < C) { st.p(c) = 0.f; st.v(c) = 0.f; }
    for (int f = 0; f < F; ++f) {
      float m, s;
      sm_draw<true>(a, st, n, f, m, s);
      const float inv = 1.f / s;
#pragma unroll UC
      for (int c = 0; c < NC; ++c)
        if (c < C) { const float pv = sm_prob(st, c, inv); st.p(c) += pv; st.v(c) = fmaf(pv, st.z(c), st.v(c)); }
    }
    const int64_t yv = a.y[n];
    const float sw = sg * wv;
#pragma unroll UC
    for (int c = 0; c < NC; ++c) {
      if (c < C) {
        const float var = a.var[c * N + n];
        a.gmu[c * N + n] = sw * ((yv == c ? 1.f : 0.f) - st.p(c) * invF);
        a.gvar[c * N + n] = var > 0.f ? -sw * (st.v(c) * invF) / (2.f * sqrtf(var)) : 0.f;
      }
    }
  }
}

// eps [F][C][N] as softmax_sites_kernel generates it.  grid (cdiv(N, 64), F), 64 threads: lanes = points
__global__ __launch_bounds__(64) void softmax_site_noise_kernel(float* __restrict__ eps, uint64_t seed, int F, int C, int64_t N) {
  const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int f = blockIdx.y, nq = (C + 3) >> 2;
  if (n >= N) return;
  for (int j = 0; j < nq; ++j) {
    float z[4];
    normal4(seed, kStreamSite, ((uint64_t)n * (uint64_t)F + (uint64_t)f) * (uint64_t)nq + (uint64_t)j, 0u, z);
#pragma unroll
    for (int l = 0; l < 4; ++l)
      if (4 * j + l < C) eps[((int64_t)f * C + 4 * j + l) * N + n] = z[l];
  }
}

}  // namespace vargp

using namespace vargp;

extern "C" size_t vargp_softmax_sites_workspace_bytes(int C, int N) {
  if (C <= 0 || N <= 0) return 0;
  return (size_t)sm_plan(N).nch * 4 * sizeof(double) + 256;
}

extern "C" int vargp_softmax_sites(const float* mu, const float* var, const int64_t* y, const float* w, const float* eps,
                                   uint64_t seed, float* lam1, float* lam2, float* sums, int C, int N, int F, void* ws,
                                   size_t ws_bytes, vargp_stream_t stream) {
  VARGP_REQUIRE(mu && var && y && lam1 && lam2 && sums && ws, "softmax_sites: null pointer");
  VARGP_REQUIRE(N > 0 && F > 0, "softmax_sites: bad dims");
  VARGP_REQUIRE(C >= 2 && C <= kSmMaxC, "softmax_sites: C = %d (2 to %d classes)", C, kSmMaxC);
  VARGP_REQUIRE(F <= 65535, "softmax_sites: F = %d (at most 65535)", F);
  VARGP_REQUIRE(reinterpret_cast<uintptr_t>(ws) % sizeof(double) == 0, "softmax_sites: ws must be 8-byte aligned");
  VARGP_REQUIRE(ws_bytes >= vargp_softmax_sites_workspace_bytes(C, N), "softmax_sites: workspace too small");
  SmArgs a{};
  a.mu = mu; a.var = var; a.w = w; a.eps = eps; a.y = y; a.lam1 = lam1; a.lam2 = lam2; a.sums = sums;
  a.ps = reinterpret_cast<double*>(ws);
  a.seed = seed;
  a.p = sm_plan(N);
  a.C = C; a.N = N; a.F = F;
  hipStream_t st = as_stream(stream);
  ProfScope whole("softmax_sites", st);
  if (C <= kSmRegC) {
    hipLaunchKernelGGL(softmax_sites_kernel<kSmRegC>, dim3(a.p.nch), dim3(64), 0, st, a);
  } else {
    constexpr auto kernel = softmax_sites_kernel<0>;
    if (int rc = reserve_dynamic_lds<kernel>((size_t)3 * kSmMaxC * 64 * sizeof(float), "softmax_sites")) return rc;
    hipLaunchKernelGGL(kernel, dim3(a.p.nch), dim3(64), (size_t)3 * C * 64 * sizeof(float), st, a);
  }
  hipLaunchKernelGGL(softmax_sites_reduce_kernel, dim3(1), dim3(64), 0, st, a);
  return check_launch("softmax_sites");
}

extern "C" int vargp_softmax_site_grads(const float* mu, const float* var, const int64_t* y, const float* w, const float* eps,
                                        uint64_t seed, const float* gout, float* gmu, float* gvar, int C, int N, int F,
                                        vargp_stream_t stream) {
  VARGP_REQUIRE(mu && var && y && gout && gmu && gvar, "softmax_site_grads: null pointer");
  VARGP_REQUIRE(N > 0 && F > 0, "softmax_site_grads: bad dims");
  VARGP_REQUIRE(C >= 2 && C <= kSmMaxC, "softmax_site_grads: C = %d (2 to %d classes)", C, kSmMaxC);
  VARGP_REQUIRE(F <= 65535, "softmax_site_grads: F = %d (at most 65535)", F);
  SmGradArgs a{};
  a.mu = mu; a.var = var; a.w = w; a.eps = eps; a.y = y; a.gout = gout; a.gmu = gmu; a.gvar = gvar;
  a.seed = seed;
  a.p = sm_plan(N);
  a.C = C; a.N = N; a.F = F;
  hipStream_t st = as_stream(stream);
  ProfScope whole("softmax_site_grads", st);
  if (C <= kSmRegC) {
    hipLaunchKernelGGL(softmax_site_grads_kernel<kSmRegC>, dim3(a.p.nch), dim3(64), 0, st, a);
  } else {
    constexpr auto kernel = softmax_site_grads_kernel<0>;
    if (int rc = reserve_dynamic_lds<kernel>((size_t)4 * kSmMaxC * 64 * sizeof(float), "softmax_site_grads")) return rc;
    hipLaunchKernelGGL(kernel, dim3(a.p.nch), dim3(64), (size_t)4 * C * 64 * sizeof(float), st, a);
  }
  return check_launch("softmax_site_grads");
}

extern "C" int vargp_softmax_site_noise(uint64_t seed, float* eps, int F, int C, int N, vargp_stream_t stream) {
  VARGP_REQUIRE(eps, "softmax_site_noise: null pointer");
  VARGP_REQUIRE(N > 0 && F > 0, "softmax_site_noise: bad dims");
  VARGP_REQUIRE(C >= 2 && C <= kSmMaxC, "softmax_site_noise: C = %d (2 to %d classes)", C, kSmMaxC);
  VARGP_REQUIRE(F <= 65535, "softmax_site_noise: F = %d (at most 65535)", F);
  hipStream_t st = as_stream(stream);
  ProfScope whole("softmax_site_noise", st);
  hipLaunchKernelGGL(softmax_site_noise_kernel, dim3(cdiv(N, 64), F), dim3(64), 0, st, eps, seed, F, C, (int64_t)N);
  return check_launch("softmax_site_noise");
}
