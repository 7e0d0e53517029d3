// Gaussian sites of a non-Gaussian likelihood over a whole data set, for G independent outputs over ONE data matrix X [N][D] and
// ONE hyper vector -- what one natural-gradient (conjugate-computation) iteration on q(u) needs of the data (sites.py; nothing of
// this is in the reference).  Given q(u) through alpha [G][Mt] and a symmetric Q [G][Mt][Mt], with k_n = k_theta(Z_g, x_n):
//   mu_n  = alpha_g . k_n,   var_n = max(gamma^2 - k_n^T Q_g k_n, 0)
//   (ell, dmu, dvar) = LIK::element<true>(mu_n, var_n, y_gn)                  (lik.h: the arithmetic of indep_lik.hip)
//   lam2_gn = w_gn max(-2 dvar, 0),   lam1_gn = w_gn dmu + lam2_gn mu_n
//   lam2 [G][N];   c_g = sum_n lam1_gn k_n;   sums_g = (sum_n w ell, sum_n lam2, #{n: w_gn != 0, dvar > 0}, sum_n w)
// K(Z, X) never reaches global memory.  A workgroup owns one (output g, chunk of N) and walks its chunk 64 columns at a time: ALL
// Mt rows of the 64 columns of K are built in LDS as [column][row], 64-row panel by panel, with the distance forms, epilogues and
// masked columns of moments.hip (direct form for D <= kRbfDirectD, slabs of 32 values of d on the MFMA above it).  mu is a plain
// sum over the rows; for the quadratic form, every 64 x 64 tile Q_ij (staged as [k][row]; read TRANSPOSED from global memory,
// which is coalesced and the same quadratic form) is multiplied with panel j of K by 32 v_mfma_f32_32x32x2_f32 per wave (four waves
// as 2 x 2), and the accumulators of (Q K)_i are reduced against panel i of K over the rows.  One wave then evaluates the
// likelihood for the 64 points, and all four add lam1 K to the accumulators of c, which stay in registers for the whole chunk.
// The block needs Mt <= kSiMaxMt (moments_plan.h): 64 (Mt + 1) floats of the at most 160 KB of LDS; above it there is no fused
// pass (sites.py composes the same quantities from the per-op kernels).
// A point of weight 0 is never evaluated: it adds exactly nothing whatever its row of X and its target hold (K is finite for
// finite inputs; the likelihood's derivatives need not be).  Columns behind the end of the chunk are masked as in moments.hip.
// No atomics.  A second launch adds the chunks' partials in ascending chunk order in fp64 and rounds once: two calls on the same
// input are bitwise equal.  The chunking depends on the shapes alone (site_plan).
#include <atomic>

#include "lik.h"
#include "moments_plan.h"

namespace vargp {

typedef float si_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kSiMaxNt = kSiMaxMt / kMoT;
constexpr int kSiStage = 2 * kMoT * kMoDl > 2 * kMoBK * kMoLD ? 2 * kMoT * kMoDl : 2 * kMoBK * kMoLD;
static_assert(kSiMaxMt % kMoT == 0 && kSiMaxNt * 16 == kSiMaxMt / 4, "a wave's quarter of the rows");

// floats of LDS for nt panels: the K block, a tile of Q, the staging area, alpha, exp(-2 theta), norms, mu, lam1, two reduction pads
static constexpr size_t site_lds_floats(int nt) {
  return (size_t)kMoT * (nt * kMoT + 1) + kMoT * kMoLD + kSiStage + nt * kMoT + kRbfDirectD + 2 * kMoT + kMoT + kMoT + 4 * kMoT +
         4 * kMoT;
}
static_assert(site_lds_floats(kSiMaxNt) * sizeof(float) <= 160 * 1024, "the K block of kSiMaxMt rows must fit the LDS");

struct SitePlan {
  int nt, nch;               // 64-row panels, chunks
  int64_t len;               // columns per chunk (a multiple of kMoT)
  double* ps;                // partials of sums [G][nch][4]
  float* pc;                 // partials of c [G][nch][nt * 64]
  size_t bytes;
};

static SitePlan site_plan(void* ws, int G, int Mt, int N) {
  SitePlan o{};
  o.nt = cdiv(Mt, kMoT);
  int64_t want = cdiv(kMoTargetWg, G);
  const int64_t most = cdiv(N, kMoMinChunk);
  want = want < most ? want : most;
  want = want < 1 ? 1 : (want > kMoMaxChunks ? kMoMaxChunks : want);
  o.len = round_up(cdiv(N, want), kMoT);
  o.nch = cdiv(N, o.len);
  char* p = reinterpret_cast<char*>(ws);
  o.ps = reinterpret_cast<double*>(p);
  p += round_up((int64_t)G * o.nch * 4 * (int64_t)sizeof(double), 256);
  o.pc = reinterpret_cast<float*>(p);
  p += round_up((int64_t)G * o.nch * o.nt * kMoT * (int64_t)sizeof(float), 256);
  o.bytes = (size_t)(p - reinterpret_cast<char*>(ws));
  return o;
}

struct SiteArgs {
  const float *theta, *Z, *X, *alpha, *Q, *w;
  float *lam2, *c, *sums;
  SitePlan p;
  int G, Mt, N, D;
};

// grid (nch, G)
template <class LIK, class EPI, bool DIRECT>
__global__ __launch_bounds__(256) void site_kernel(const SiteArgs a, const typename LIK::Args la) {
  using real = typename LIK::real;
  constexpr int T = kMoT, LD = kMoLD, BK = kMoBK;
  extern __shared__ __attribute__((aligned(16))) float si_lds[];
  const int Mt = a.Mt, D = a.D, nt = a.p.nt, MtP = nt * T, LDK = MtP + 1;
  float* Ks = si_lds;                  // the K block: [n][m], m over all nt panels
  float* Ss = Ks + T * LDK;            // a tile of Q: [k = row of panel j][row of panel i]
  float* stage = Ss + T * LD;          // DIRECT: Z_j, X rows; else the slabs of a_j, b: [k][r]
  float* al = stage + kSiStage;        // alpha, zeros behind Mt
  float* wl = al + MtP;                // DIRECT: exp(-2 theta_d)
  float* nrm = wl + kRbfDirectD;       // !DIRECT: |a_j|^2, |b|^2
  float* mus = nrm + 2 * T;            // mu of the step's columns
  float* l1s = mus + T;                // lam1 of the step's columns (0 behind the end)
  float* cred = l1s + T;               // [4][T]
  float* qred = cred + 4 * T;          // [4][32]: the waves' shares of k^T Q k

  const int chunk = blockIdx.x;
  const int64_t g = blockIdx.y;
  const int64_t cbeg = (int64_t)chunk * a.p.len;
  const int64_t cend = cbeg + a.p.len < a.N ? cbeg + a.p.len : a.N;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32, l31 = lane & 31, h = lane >> 5;
  const float g2 = expf(2.f * a.theta[D]);
  const float* __restrict__ Zg = a.Z + g * (int64_t)Mt * D;
  const float* __restrict__ X = a.X;
  const float* __restrict__ Qg = a.Q + g * (int64_t)Mt * Mt;
  const float* __restrict__ wg = a.w ? a.w + g * (int64_t)a.N : nullptr;
  const int Dl = D | 1;
  const typename LIK::Cls cls = LIK::cls(la, (int)g);

  float cacc[kSiMaxNt];
#pragma unroll
  for (int p = 0; p < kSiMaxNt; ++p) cacc[p] = 0.f;
  double s_ell = 0.0, s_l2 = 0.0, s_cl = 0.0, s_w = 0.0;

  for (int e = tid; e < MtP; e += 256) al[e] = e < Mt ? a.alpha[g * Mt + e] : 0.f;
  if constexpr (DIRECT) {
    if (tid < D) wl[tid] = expf(-2.f * a.theta[tid]);
  }

  for (int64_t n0 = cbeg; n0 < cend; n0 += T) {
    // ---- the K block: rows behind Mt and columns behind the end of the chunk are zeros
    if constexpr (DIRECT) {
      float* Xs = stage + T * kMoDl;
      for (int e = tid; e < T * D; e += 256) {
        const int r = e / D, d = e - r * D;
        Xs[r * Dl + d] = n0 + r < cend ? X[(n0 + r) * D + d] : 0.f;
      }
    }
    for (int tj = 0; tj < nt; ++tj) {
      const int j0 = tj * T;
      if constexpr (DIRECT) {
        const float* Xs = stage + T * kMoDl;
        for (int e = tid; e < T * D; e += 256) {
          const int r = e / D, d = e - r * D;
          stage[r * Dl + d] = j0 + r < Mt ? Zg[(int64_t)(j0 + r) * D + d] : 0.f;
        }
        __syncthreads();
        // lanes = rows of the panel, the wave's 16 columns in registers; the point of X is a broadcast read
        const float* zr = stage + lane * Dl;
        const float* xr = Xs + 16 * wave * Dl;
        float d2[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) d2[q] = 0.f;
        for (int d = 0; d < D; ++d) {
          const float zv = zr[d], wv = wl[d];
#pragma unroll
          for (int q = 0; q < 16; ++q) { const float v = zv - xr[q * Dl + d]; d2[q] = fmaf(wv * v, v, d2[q]); }
        }
        const bool rok = j0 + lane < Mt;
#pragma unroll
        for (int q = 0; q < 16; ++q)
          Ks[(16 * wave + q) * LDK + j0 + lane] = (rok && n0 + 16 * wave + q < cend) ? EPI::off(g2, d2[q]) : 0.f;
      } else {
        float* Aj = stage;
        float* Bs = stage + BK * LD;
        si_f32x16 dj;
#pragma unroll
        for (int r = 0; r < 16; ++r) dj[r] = 0.f;
        float nr = 0.f;
        const int k = tid & 31;
        for (int k0 = 0; k0 < D; k0 += BK) {
          const bool kok = k0 + k < D;
          const float sq = kok ? expf(-a.theta[k0 + k]) : 0.f;           // 1 / lengthscale
#pragma unroll
          for (int r = tid >> 5; r < T; r += 8) {
            Aj[k * LD + r] = (kok && j0 + r < Mt) ? sq * Zg[(int64_t)(j0 + r) * D + k0 + k] : 0.f;
            Bs[k * LD + r] = (kok && n0 + r < cend) ? sq * X[(n0 + r) * D + k0 + k] : 0.f;
          }
          __syncthreads();
#pragma unroll
          for (int kk = 0; kk < BK; kk += 2)
            dj = __builtin_amdgcn_mfma_f32_32x32x2f32(Aj[(kk + h) * LD + wr + l31], Bs[(kk + h) * LD + wc + l31], dj, 0, 0, 0);
          if (wave < 2) {
            const float* src = stage + wave * BK * LD + lane;
#pragma unroll
            for (int kk = 0; kk < BK; ++kk) { const float v = src[kk * LD]; nr = fmaf(v, v, nr); }
          }
          __syncthreads();
        }
        if (wave < 2) nrm[wave * T + lane] = nr;
        __syncthreads();
        const int col = wc + l31;
        const bool cok = n0 + col < cend;
        const float nb = nrm[T + col];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wr + (r & 3) + 8 * (r >> 2) + 4 * h;
          Ks[col * LDK + j0 + row] = (cok && j0 + row < Mt) ? EPI::off(g2, nrm[row] + nb - 2.f * dj[r]) : 0.f;
        }
      }
      __syncthreads();
    }

    // ---- mu_n = alpha . k_n: lanes = columns, every wave a quarter of the rows in ascending order
    {
      const float* kr = Ks + lane * LDK;
      float s = 0.f;
      for (int m = wave * (MtP >> 2); m < (wave + 1) * (MtP >> 2); ++m) s = fmaf(kr[m], al[m], s);
      cred[wave * T + lane] = s;
    }

    // ---- k_n^T Q k_n: (Q K)_i = sum_j Q_ij K_j on the MFMA (A = Q_ij [row][k], B = K_j [k][n]), reduced against K_i over the rows
    float qv = 0.f;
    for (int ti = 0; ti < nt; ++ti) {
      const int i0 = ti * T;
      si_f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      for (int tj = 0; tj < nt; ++tj) {
        const int j0 = tj * T;
        for (int e = tid; e < T * T; e += 256) {
          const int k = e >> 6, r = e & 63;
          Ss[k * LD + r] = (i0 + r < Mt && j0 + k < Mt) ? Qg[(int64_t)(j0 + k) * Mt + i0 + r] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < T; kk += 2)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ss[(kk + h) * LD + wr + l31], Ks[(wc + l31) * LDK + j0 + kk + h], acc, 0, 0, 0);
        __syncthreads();
      }
      const float* kc = Ks + (wc + l31) * LDK + i0 + wr + 4 * h;
#pragma unroll
      for (int r = 0; r < 16; ++r) qv = fmaf(acc[r], kc[(r & 3) + 8 * (r >> 2)], qv);
    }
    qv += __shfl_xor(qv, 32, 64);
    if (h == 0) qred[wave * 32 + l31] = qv;
    __syncthreads();

    // ---- the likelihood of the step's points: one wave, a point per lane
    if (tid < T) {
      const int64_t n = n0 + tid;
      const float mu = (cred[tid] + cred[T + tid]) + (cred[2 * T + tid] + cred[3 * T + tid]);
      const float quad = qred[(tid >> 5) * 32 + (tid & 31)] + qred[((tid >> 5) + 2) * 32 + (tid & 31)];
      const float var = fmaxf(g2 - quad, 0.f);
      float l1 = 0.f;
      if (n < cend) {
        const float wv = wg ? wg[n] : 1.f;
        float l2 = 0.f;
        if (wv != 0.f) {
          real dmu = 0, dvar = 0, dpar = 0;
          const real ell = LIK::template element<true>(cls, (real)mu, (real)var, LIK::template target<real>(la, (int)g, (size_t)n),
                                                       dmu, dvar, dpar);
          const bool clamp = dvar > (real)0;
          l2 = clamp ? 0.f : wv * (float)((real)-2 * dvar);
          l1 = fmaf(l2, mu, wv * (float)dmu);
          s_ell += (double)wv * (double)ell;
          s_l2 += (double)l2;
          s_cl += clamp ? 1.0 : 0.0;
          s_w += (double)wv;
        }
        a.lam2[g * (int64_t)a.N + n] = l2;
      }
      l1s[tid] = l1;
    }
    __syncthreads();

    // ---- c += K lam1: lanes = rows of a panel, every wave 16 of the columns
#pragma unroll
    for (int p = 0; p < kSiMaxNt; ++p) {
      if (p < nt) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) s = fmaf(Ks[(16 * wave + q) * LDK + p * T + lane], l1s[16 * wave + q], s);
        cacc[p] += s;
      }
    }
    __syncthreads();
  }

  const int64_t part = g * a.p.nch + chunk;
#pragma unroll
  for (int p = 0; p < kSiMaxNt; ++p) {
    if (p < nt) {
      __syncthreads();
      cred[wave * T + lane] = cacc[p];
      __syncthreads();
      if (tid < T) a.p.pc[(part * nt + p) * T + tid] = (cred[tid] + cred[T + tid]) + (cred[2 * T + tid] + cred[3 * T + tid]);
    }
  }
  if (wave == 0) {
    s_ell = wave_sum(s_ell);
    s_l2 = wave_sum(s_l2);
    s_cl = wave_sum(s_cl);
    s_w = wave_sum(s_w);
    if (lane == 0) {
      double* ps = a.p.ps + part * 4;
      ps[0] = s_ell; ps[1] = s_l2; ps[2] = s_cl; ps[3] = s_w;
    }
  }
}

// The chunks' partials in ascending chunk order, in fp64.  grid (cdiv(Mt, 256) + 1, G): 256 entries of c | the four sums
__global__ __launch_bounds__(256) void site_reduce_kernel(const SiteArgs a) {
  constexpr int T = kMoT;
  const int Mt = a.Mt, nch = a.p.nch, nt = a.p.nt;
  const int64_t g = blockIdx.y;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b < (Mt + 255) / 256) {
    const int i = b * 256 + tid;
    if (i >= Mt) return;
    const float* p = a.p.pc + (g * nch) * (int64_t)(nt * T) + i;
    double s = 0.0;
    for (int q = 0; q < nch; ++q) s += (double)p[(int64_t)q * nt * T];
    a.c[g * Mt + i] = (float)s;
  } else if (tid < 4) {
    const double* p = a.p.ps + (g * nch) * 4 + tid;
    double s = 0.0;
    for (int q = 0; q < nch; ++q) s += p[4 * q];
    a.sums[g * 4 + tid] = (float)s;
  }
}

// hipFuncAttributeMaxDynamicSharedMemorySize is per device and per kernel: one mask per instantiation
template <class LIK, class EPI, bool DIRECT>
static int site_launch_form(const SiteArgs& a, const typename LIK::Args& la, hipStream_t st) {
  static std::atomic<unsigned> attr_mask[2] = {};
  const size_t lds = site_lds_floats(kSiMaxNt) * sizeof(float);
  int dev = 0;
  VARGP_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64, "site_moments: hipGetDevice failed");
  if (!((attr_mask[dev >> 5].load(std::memory_order_acquire) >> (dev & 31)) & 1u)) {
    VARGP_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(site_kernel<LIK, EPI, DIRECT>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess,
                  "site_moments: cannot reserve %zu bytes of LDS", lds);
    attr_mask[dev >> 5].fetch_or(1u << (dev & 31), std::memory_order_release);
  }
  hipLaunchKernelGGL((site_kernel<LIK, EPI, DIRECT>), dim3(a.p.nch, a.G), dim3(256), site_lds_floats(a.p.nt) * sizeof(float), st, a,
                     la);
  return VARGP_OK;
}

template <class LIK, class EPI>
static int site_launch_epi(const SiteArgs& a, const typename LIK::Args& la, hipStream_t st) {
  return a.D <= kRbfDirectD ? site_launch_form<LIK, EPI, true>(a, la, st) : site_launch_form<LIK, EPI, false>(a, la, st);
}

template <class LIK>
static int site_launch(const SiteArgs& a, const typename LIK::Args& la, int nu2, hipStream_t st) {
  switch (nu2) {
    case 0: return site_launch_epi<LIK, EpiRbf>(a, la, st);
    case 1: return site_launch_epi<LIK, EpiMatern<1>>(a, la, st);
    case 3: return site_launch_epi<LIK, EpiMatern<3>>(a, la, st);
    default: return site_launch_epi<LIK, EpiMatern<5>>(a, la, st);
  }
}

}  // namespace vargp

using namespace vargp;

extern "C" int vargp_site_moments_chunks(int G, int Mt, int N, int D) {
  if (G <= 0 || Mt <= 0 || N <= 0 || D <= 0) return 0;
  return site_plan(nullptr, G, Mt, N).nch;
}

extern "C" size_t vargp_site_moments_workspace_bytes(int G, int Mt, int N, int D) {
  if (G <= 0 || Mt <= 0 || N <= 0 || D <= 0) return 0;
  return site_plan(nullptr, G, Mt, N).bytes + 256;
}

extern "C" int vargp_site_moments(const float* theta, const float* Z, const float* X, const float* alpha, const float* Q,
                                  const float* y, int64_t ldy, const float* w, int kind, const float* log_scale, float df,
                                  float lognorm, float* lam2, float* c, float* sums, int G, int Mt, int N, int D, int nu2, void* ws,
                                  size_t ws_bytes, vargp_stream_t stream) {
  VARGP_REQUIRE(theta && Z && X && alpha && Q && y && lam2 && c && sums && ws, "site_moments: null pointer");
  VARGP_REQUIRE(G > 0 && Mt > 0 && N > 0 && D > 0, "site_moments: bad dims");
  VARGP_REQUIRE(kind >= VARGP_SITE_BERNOULLI_PROBIT && kind <= VARGP_SITE_STUDENTT,
                "site_moments: kind = %d (0: Bernoulli probit, 1: Bernoulli logit, 2: Poisson, 3: Student-t)", kind);
  VARGP_REQUIRE(nu2 == 0 || nu2 == 1 || nu2 == 3 || nu2 == 5, "site_moments: nu2 = %d (0: RBF; 1, 3, 5: Matern)", nu2);
  VARGP_REQUIRE(G <= 65535, "site_moments: G = %d (at most 65535)", G);
  VARGP_REQUIRE(Mt <= kSiMaxMt, "site_moments: Mt = %d (at most %d: the K block of all rows lives in LDS)", Mt, kSiMaxMt);
  VARGP_REQUIRE(ldy == 0 || ldy >= N, "site_moments: ldy must be 0 or >= N");
  VARGP_REQUIRE(kind != VARGP_SITE_STUDENTT || (log_scale && df > 0.f), "site_moments: Student-t needs log_scale and df > 0");
  VARGP_REQUIRE(reinterpret_cast<uintptr_t>(ws) % sizeof(double) == 0, "site_moments: ws must be 8-byte aligned");
  VARGP_REQUIRE(ws_bytes >= vargp_site_moments_workspace_bytes(G, Mt, N, D), "site_moments: workspace too small");
  SiteArgs a{};
  a.theta = theta; a.Z = Z; a.X = X; a.alpha = alpha; a.Q = Q; a.w = w; a.lam2 = lam2; a.c = c; a.sums = sums;
  a.p = site_plan(ws, G, Mt, N);
  a.G = G; a.Mt = Mt; a.N = N; a.D = D;
  hipStream_t st = as_stream(stream);
  ProfScope whole("site_moments", st);
  int rc;
  switch (kind) {
    case VARGP_SITE_BERNOULLI_PROBIT: rc = site_launch<Bernoulli<LinkProbit>>(a, {y, ldy, nullptr}, nu2, st); break;
    case VARGP_SITE_BERNOULLI_LOGIT: rc = site_launch<Bernoulli<LinkLogit>>(a, {y, ldy, nullptr}, nu2, st); break;
    case VARGP_SITE_POISSON: rc = site_launch<Poisson>(a, {{y, ldy}}, nu2, st); break;
    default: rc = site_launch<StudentT>(a, {{y, ldy}, log_scale, df, lognorm}, nu2, st); break;
  }
  if (rc != VARGP_OK) return rc;
  hipLaunchKernelGGL(site_reduce_kernel, dim3(cdiv(Mt, 256) + 1, G), dim3(256), 0, st, a);
  return check_launch("site_moments");
}
