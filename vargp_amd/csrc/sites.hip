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
// The block needs Mt <= kSiMaxMt (dataset_pass.h): 64 (Mt + 1) floats of the at most 160 KB of LDS; above it there is no fused
// pass (sites.py composes the same quantities from the per-op kernels).
// A point of weight 0 is never evaluated: it adds exactly nothing whatever its row of X and its target hold (K is finite for
// finite inputs; the likelihood's derivatives need not be).  Columns behind the end of the chunk are masked as in moments.hip.
// No atomics.  A second launch adds the chunks' partials in ascending chunk order in fp64 and rounds once: two calls on the same
// input are bitwise equal.  The chunking depends on the shapes alone (site_plan).
// The same kernel with LIK = SiteMarginals is vargp_site_marginals: the frame up to mu_n and var_n, which it writes out [G][N]; no
// likelihood wave, no accumulators of c, no partials and no reduce launch (the coupled softmax sites of softmax_sites.hip need the
// marginals of ALL outputs of a point at once).  With LIK = Cavity<.> it is vargp_site_cavity: one more MFMA product per step, V K,
// in the registers of Q K, and the leave-one-out cavity of every point's site (the comment at Cavity).
#include "dataset_pass.h"
#include "lik.h"

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
// (the cavity's V K adds nothing to it: a 64 x 64 tile of V is staged where the tile of Q was, its norms leave through qred)
static_assert(kMoT * kMoLD >= kMoT * kMoT && 4 * kMoT >= 4 * 32, "a tile of V fits the tile of Q, its column norms the pad of k^T Q k");

struct SitePlan {
  int nt;                    // 64-row panels
  Chunks ch;                 // ch.nch chunks of ch.len columns
  double* ps;                // partials of sums [G][nch][4]
  float* pc;                 // partials of c [G][nch][nt * 64]
  size_t bytes;
};

static SitePlan site_plan(void* ws, int G, int Mt, int N) {
  SitePlan o{};
  o.nt = cdiv(Mt, kMoT);
  o.ch = chunk_rule(N, G);
  char* p = reinterpret_cast<char*>(ws);
  o.ps = reinterpret_cast<double*>(p);
  p += round_up((int64_t)G * o.ch.nch * 4 * (int64_t)sizeof(double), 256);
  o.pc = reinterpret_cast<float*>(p);
  p += round_up((int64_t)G * o.ch.nch * o.nt * kMoT * (int64_t)sizeof(float), 256);
  o.bytes = (size_t)(p - reinterpret_cast<char*>(ws));
  return o;
}

// Not a likelihood: site_kernel stops after the marginals and writes them
struct SiteMarginals {
  using real = float;
  struct Args { float *mu, *var; };
  struct Cls {};
  static __device__ __forceinline__ Cls cls(const Args&, int) { return {}; }
};
template <class LIK> constexpr bool kSiteMarginals = false;
template <> constexpr bool kSiteMarginals<SiteMarginals> = true;

// A likelihood (or SiteMarginals) with the leave-one-out cavity behind it (vargp_site_cavity; vargp_amd/loo.py).  One more operand,
// V [G][Mv][Mt]: after the accumulators of Q K have been reduced to var, the SAME registers and the same staging tile take V K,
// panel of 64 rows by panel, and leave only its column norms s_n = |V k_n|^2 -- the share of var_n that the new block of q owns.
// With the site (lam1, lam2) of the point and r = 1 - lam2 s, in fp64 from the fp32 moments and rounded once:
//   mu_c = mu - s w dmu / r  (= (mu - s lam1) / r),   var_c = var + lam2 s^2 / r
// r <= 0 or a non-finite result: mu_c = var_c = NaN and the point is counted (per-chunk partials, added by cavity_reduce_kernel).
// A point of weight 0 has lam = 0 and its cavity is written as exactly (mu, var).  No accumulators of c, no lam1 K.
template <class LIK>
struct Cavity {
  using real = typename LIK::real;
  using Lik = LIK;
  struct Args {
    typename LIK::Args lik;
    const float* V;
    float *mu, *var, *s, *mu_c, *var_c, *lam1, *lam2;
    double* pu;              // partials of the unstable points [G][nch]
    int Mv;
  };
};
template <class LIK> struct SiteInner {
  using type = LIK;
  static __device__ __forceinline__ const typename LIK::Args& args(const typename LIK::Args& la) { return la; }
};
template <class LIK> struct SiteInner<Cavity<LIK>> {
  using type = LIK;
  static __device__ __forceinline__ const typename LIK::Args& args(const typename Cavity<LIK>::Args& la) { return la.lik; }
};
template <class LIK> constexpr bool kSiteCavity = false;
template <class LIK> constexpr bool kSiteCavity<Cavity<LIK>> = true;

// Not a likelihood either: site_bwd_kernel with GIVEN per-point seeds (vargp_site_transport_bwd).  Its "element" loads (dmu, dvar)
// = (gm, gv) [G][N] of a point from memory; there are no targets, weights or parameters, and a point whose two seeds are both 0 is
// masked like a point of weight 0
struct SiteTransport {
  using real = float;
  struct Args { const float *gm, *gv; int64_t N; };
  struct Seeds { float gm, gv; };
  struct Cls {};
  static __device__ __forceinline__ Cls cls(const Args&, int) { return {}; }
  template <class T>
  static __device__ __forceinline__ Seeds target(const Args& a, int g, size_t n) {
    return {a.gm[g * a.N + (int64_t)n], a.gv[g * a.N + (int64_t)n]};
  }
  template <bool GRAD>
  static __device__ __forceinline__ float element(const Cls&, float, float, Seeds s, float& dmu, float& dvar, float&) {
    dmu = s.gm;
    dvar = s.gv;
    return 0.f;
  }
  static __device__ __forceinline__ bool live(const Args& a, int g, int64_t n) {
    return a.gm[g * a.N + n] != 0.f || a.gv[g * a.N + n] != 0.f;
  }
};
template <class LIK> constexpr bool kSiteTransport = false;
template <> constexpr bool kSiteTransport<SiteTransport> = true;

struct SiteArgs {
  const float *theta, *Z, *X, *alpha, *Q, *w;
  float *lam2, *c, *sums;
  SitePlan p;
  int G, Mt, N, D;
};

// grid (nch, G)
template <class LIK, class EPI, bool DIRECT>
__global__ __launch_bounds__(256) void site_kernel(const SiteArgs a, const typename LIK::Args la) {
  using L = typename SiteInner<LIK>::type;            // the likelihood itself, also behind Cavity<>
  using real = typename L::real;
  constexpr int T = kMoT, LD = kMoLD, BK = kMoBK;
  constexpr bool MARG = kSiteMarginals<L>, CAV = kSiteCavity<LIK>;
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
  const int64_t cbeg = (int64_t)chunk * a.p.ch.len;
  const int64_t cend = cbeg + a.p.ch.len < a.N ? cbeg + a.p.ch.len : a.N;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32, l31 = lane & 31, h = lane >> 5;
  const float g2 = expf(2.f * a.theta[D]);
  const float* __restrict__ Zg = a.Z + g * (int64_t)Mt * D;
  const float* __restrict__ X = a.X;
  const float* __restrict__ Qg = a.Q + g * (int64_t)Mt * Mt;
  const float* __restrict__ wg = a.w ? a.w + g * (int64_t)a.N : nullptr;
  const int Dl = D | 1;
  const typename L::Args& lla = SiteInner<LIK>::args(la);
  const typename L::Cls cls = L::cls(lla, (int)g);

  float cacc[kSiMaxNt];
#pragma unroll
  for (int p = 0; p < kSiMaxNt; ++p) cacc[p] = 0.f;
  double s_ell = 0.0, s_l2 = 0.0, s_cl = 0.0, s_w = 0.0, s_un = 0.0;

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
        acc = sk_tile(acc, Ss, Ks + j0, LDK, wr + l31, wc + l31, h);
        __syncthreads();
      }
      const float* kc = Ks + (wc + l31) * LDK + i0 + wr + 4 * h;
#pragma unroll
      for (int r = 0; r < 16; ++r) qv = fmaf(acc[r], kc[(r & 3) + 8 * (r >> 2)], qv);
    }
    qv += __shfl_xor(qv, 32, 64);
    if (h == 0) qred[wave * 32 + l31] = qv;
    __syncthreads();

    if constexpr (CAV) {
      // ---- s_n = |V k_n|^2: the wave of the points below takes its shares of k^T Q k out of qred first; then (V K)_i = sum_j
      // V_ij K_j in the registers (Q K)_i had (A = V_ij [row][k], read along its rows: coalesced; B = K_j [k][n]), squared and
      // summed over the rows, and its shares go where those were
      float quad = 0.f;
      if (tid < T) quad = qred[(tid >> 5) * 32 + (tid & 31)] + qred[((tid >> 5) + 2) * 32 + (tid & 31)];
      const float* __restrict__ Vg = la.V + g * (int64_t)la.Mv * Mt;
      float sv = 0.f;
      for (int i0 = 0; i0 < la.Mv; i0 += T) {
        si_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int tj = 0; tj < nt; ++tj) {
          const int j0 = tj * T;
          for (int e = tid; e < T * T; e += 256) {
            const int r = e >> 6, k = e & 63;
            Ss[k * LD + r] = (i0 + r < la.Mv && j0 + k < Mt) ? Vg[(int64_t)(i0 + r) * Mt + j0 + k] : 0.f;
          }
          __syncthreads();
          acc = sk_tile(acc, Ss, Ks + j0, LDK, wr + l31, wc + l31, h);
          __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) sv = fmaf(acc[r], acc[r], sv);
      }
      sv += __shfl_xor(sv, 32, 64);
      if (h == 0) qred[wave * 32 + l31] = sv;
      __syncthreads();

      // ---- the points of the step: marginals, site and cavity; one wave, a point per lane
      if (tid < T && n0 + tid < cend) {
        const int64_t at = g * (int64_t)a.N + n0 + tid;
        const float mu = wave4_sum(cred, tid);
        const float var = fmaxf(g2 - quad, 0.f);
        const float s = qred[(tid >> 5) * 32 + (tid & 31)] + qred[((tid >> 5) + 2) * 32 + (tid & 31)];
        la.mu[at] = mu;
        la.var[at] = var;
        la.s[at] = s;
        if constexpr (!MARG) {
          const float wv = wg ? wg[n0 + tid] : 1.f;
          float l1 = 0.f, l2 = 0.f, mc = mu, vc = var;
          if (wv != 0.f) {
            real dmu = 0, dvar = 0, dpar = 0;
            L::template element<true>(cls, (real)mu, (real)var, L::template target<real>(lla, (int)g, (size_t)(n0 + tid)), dmu, dvar,
                                      dpar);
            l2 = dvar > (real)0 ? 0.f : wv * (float)((real)-2 * dvar);
            l1 = fmaf(l2, mu, wv * (float)dmu);
            const double sd = (double)s, r = 1.0 - (double)l2 * sd;
            mc = (float)((double)mu - sd * ((double)wv * (double)dmu) / r);
            vc = (float)((double)var + (double)l2 * sd * sd / r);
            if (!(r > 0.0) || !isfinite(mc) || !isfinite(vc)) {
              mc = vc = __builtin_nanf("");
              s_un += 1.0;
            }
          }
          la.mu_c[at] = mc;
          la.var_c[at] = vc;
          la.lam1[at] = l1;
          la.lam2[at] = l2;
        }
      }
      __syncthreads();
      continue;
    }

    // ---- the likelihood of the step's points: one wave, a point per lane
    if (tid < T) {
      const int64_t n = n0 + tid;
      const float mu = wave4_sum(cred, tid);
      const float quad = qred[(tid >> 5) * 32 + (tid & 31)] + qred[((tid >> 5) + 2) * 32 + (tid & 31)];
      const float var = fmaxf(g2 - quad, 0.f);
      float l1 = 0.f;
      if constexpr (MARG) {
        if (n < cend) {
          lla.mu[g * (int64_t)a.N + n] = mu;
          lla.var[g * (int64_t)a.N + n] = var;
        }
      } else if (n < cend) {
        const float wv = wg ? wg[n] : 1.f;
        float l2 = 0.f;
        if (wv != 0.f) {
          real dmu = 0, dvar = 0, dpar = 0;
          const real ell = L::template element<true>(cls, (real)mu, (real)var, L::template target<real>(lla, (int)g, (size_t)n),
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
    if constexpr (MARG) continue;

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
  if constexpr (MARG) return;

  const int64_t part = g * a.p.ch.nch + chunk;
  if constexpr (CAV) {
    if (wave == 0) {
      s_un = wave_sum(s_un);
      if (lane == 0) la.pu[part] = s_un;
    }
    return;
  }
#pragma unroll
  for (int p = 0; p < kSiMaxNt; ++p) {
    if (p < nt) {
      __syncthreads();
      cred[wave * T + lane] = cacc[p];
      __syncthreads();
      if (tid < T) a.p.pc[(part * nt + p) * T + tid] = wave4_sum(cred, tid);
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
  const int Mt = a.Mt, nch = a.p.ch.nch, nt = a.p.nt;
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

template <class LIK, class EPI, bool DIRECT>
static int site_launch_form(const SiteArgs& a, const typename LIK::Args& la, hipStream_t st) {
  constexpr auto kernel = site_kernel<LIK, EPI, DIRECT>;
  if (int rc = reserve_dynamic_lds<kernel>(site_lds_floats(kSiMaxNt) * sizeof(float),
                                           kSiteCavity<LIK> ? "site_cavity" : kSiteMarginals<LIK> ? "site_marginals" : "site_moments"))
    return rc;
  hipLaunchKernelGGL(kernel, dim3(a.p.ch.nch, a.G), dim3(256), site_lds_floats(a.p.nt) * sizeof(float), st, a, la);
  return VARGP_OK;
}

// The chunks' counts of unstable points in ascending chunk order.  grid (cdiv(G, 256)): an output per thread
__global__ __launch_bounds__(256) void cavity_reduce_kernel(const double* pu, long long* n_unstable, int G, int nch) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  double s = 0.0;
  for (int q = 0; q < nch; ++q) s += pu[(int64_t)g * nch + q];
  n_unstable[g] = (long long)s;
}

template <class LIK>
static int site_launch(const SiteArgs& a, const typename LIK::Args& la, int nu2, hipStream_t st) {
  return with_epi(nu2, [&](auto epi) {
    using EPI = decltype(epi);
    return a.D <= kRbfDirectD ? site_launch_form<LIK, EPI, true>(a, la, st) : site_launch_form<LIK, EPI, false>(a, la, st);
  });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The backward of the pass's first sum, value_g = sum_n w_gn ell_gn, for theta, Z, alpha and (through gv) Q: the M-step of
// variational EM on the site bound (sites.py: site_bound, fit_sites_).  With Qs = (Q + Q^T) / 2, q_n = k_n^T Qs k_n, the seed s_g
// of output g and u_n = [gamma^2 - q_n > 0] (the variance clamp passes no gradient):
//   gm_n = s_g w_n dmu_n,   gv_n = s_g w_n dvar_n u_n           (the TRUE signed dvar: not lam2)
//   galpha_g = sum_n gm_n k_n;   gQ_g = -sum_n gv_n k_n k_n^T is the caller's (vargp_gram_moments with w = gv)
//   gK[:, n] = gm_n alpha_g - 2 gv_n Qs k_n,   V = gK o (-2 dk/dd2)        (Mt x N, neither ever reaches global memory)
//   r = V 1,  cn = V^T 1,  P = V X,  q_d = sum_n cn_n x_nd^2
//   gZ_i = -wl o (r_i z_i - P_i),   gtheta_d = wl_d sum_g [sum_i z_id (r_i z_id - 2 P_id) + q_d]   (d < D)
//   gtheta_D = sum_g sum_n [2 gm_n mu_n + gv_n (2 gamma^2 - 4 q_n)],   gls_g = s_g sum_n w_n d ell_n / d log_scale_g.
// A workgroup owns (output g, chunk of N, group of 64 NP values of d) and walks its chunk 64 columns at a time.  Per step: the K
// block of ALL Mt rows is built in LDS exactly as the forward builds it, and beside it a second block of the same shape with the
// weight -2 dk/dd2; mu by the forward's sums; every 64 x 64 tile of Qs (staged as [k][row] in the area the K build staged its
// operands in) times panel j of K on the MFMA, the accumulators of ALL panels of Qs K staying in registers (16 nt per lane), and
// q_n reduced from them in the forward's order -- mu and var are bitwise the forward's for a symmetric Q.  One wave evaluates
// LIK::element<true> for the 64 points and leaves gm and gv; V overwrites the weight block in place from the accumulators.
// galpha, r and cn are plain sums over the blocks; P += V X on the same MFMA, the step's 64 rows of X staged 64 values of d at a
// time (waves as 2 row halves x 2 halves of the 64 values, nt NP accumulator tiles per wave for the whole chunk); q rides on the
// staged X.  D > 64 NP: the grid is split over groups of d and every group recomputes V (group 0 alone writes gv, galpha, r and
// the per-point scalars).
// A column behind the end of the chunk OR of weight 0 is masked everywhere: its K, weight and staged X entries are written as
// zeros whatever X and the target hold there (NaN included), so it adds exactly nothing.  No atomics; a last launch adds the
// chunks' partials in ascending chunk order in fp64, forms gZ and gtheta there and rounds once.  The chunking (site_bwd_plan)
// depends on the shapes alone: the forward's rule over G x groups workgroups, capped so that the partials of P stay below
// kSbBudget bytes.
// The same kernel with LIK = SiteTransport is vargp_site_transport_bwd: (gm, gv) [G][N] are GIVEN (the softmax's, from
// softmax_sites.hip: vargp_softmax_site_grads) and carried back to Z, theta, alpha and, through gv_out = gv u, Q.  No likelihood is
// evaluated; u_n is recomputed here; a column whose gm and gv are both 0 is masked like one of weight 0.
constexpr int kSbNPMax = 2;                     // tiles of 64 values of d per group (GEMM form; the direct form has D <= 32: one)
constexpr size_t kSbBudget = 64u << 20;         // bytes of the per-chunk partials of r, galpha and P, at most (one chunk always fits)
constexpr int kSbStage = kSiStage > kMoT * kMoLD ? kSiStage : kMoT * kMoLD;

// floats of LDS for nt panels: the K and weight / V blocks, the shared staging area (operands of K | a tile of Qs | X of the
// step), alpha, exp(-2 theta), norms, gm, gv, cn, the column mask, two reduction pads
static constexpr size_t site_bwd_lds_floats(int nt) {
  return (size_t)2 * kMoT * (nt * kMoT + 1) + kSbStage + nt * kMoT + kRbfDirectD + 2 * kMoT + 4 * kMoT + 4 * kMoT + 4 * kMoT;
}
static_assert(site_bwd_lds_floats(kSiMaxNt) * sizeof(float) <= 160 * 1024, "the K and V blocks of kSiMaxMt rows must fit the LDS");

struct SiteBwdPlan {
  int nt, np, ngrp;          // panels, tiles of d per group, groups of d
  Chunks ch;                 // ch.nch chunks of ch.len columns
  double* ps;                // partials of (gtheta_D, gls) [G][nch][2]
  float *pr, *pa, *pq, *pp;  // partials r [G][nch][nt * 64], galpha alike, q [G][nch][D], P [G][nch][nt * 64][D]
  size_t bytes;
};

static SiteBwdPlan site_bwd_plan(void* ws, int G, int Mt, int N, int D) {
  SiteBwdPlan o{};
  o.nt = cdiv(Mt, kMoT);
  o.np = D <= kRbfDirectD ? 1 : kSbNPMax;
  o.ngrp = cdiv(D, 64 * o.np);
  const int64_t per = (int64_t)G * o.nt * kMoT * (D + 2) * (int64_t)sizeof(float);
  o.ch = chunk_rule(N, (int64_t)G * o.ngrp, (int64_t)kSbBudget / per);
  char* p = reinterpret_cast<char*>(ws);
  auto take = [&](int64_t bytes) { char* q = p; p += round_up(bytes, 256); return q; };
  const int64_t parts = (int64_t)G * o.ch.nch, f = sizeof(float);
  o.ps = reinterpret_cast<double*>(take(parts * 2 * (int64_t)sizeof(double)));
  o.pr = reinterpret_cast<float*>(take(parts * o.nt * kMoT * f));
  o.pa = reinterpret_cast<float*>(take(parts * o.nt * kMoT * f));
  o.pq = reinterpret_cast<float*>(take(parts * D * f));
  o.pp = reinterpret_cast<float*>(take(parts * o.nt * kMoT * D * f));
  o.bytes = (size_t)(p - reinterpret_cast<char*>(ws));
  return o;
}

struct SiteBwdArgs {
  const float *theta, *Z, *X, *alpha, *Q, *w, *gout;
  float *gZ, *gtheta, *galpha, *gv, *gls;
  SiteBwdPlan p;
  int G, Mt, N, D;
};

// grid (nch * ngrp, G): blockIdx.x = chunk * ngrp + group
template <class LIK, class EPI, bool DIRECT, int NP>
__global__ __launch_bounds__(256) void site_bwd_kernel(const SiteBwdArgs a, const typename LIK::Args la) {
  using real = typename LIK::real;
  constexpr int T = kMoT, LD = kMoLD, BK = kMoBK;
  constexpr bool TRANS = kSiteTransport<LIK>;      // the seeds are given: no weights, no upstream seed (they carry both)
  extern __shared__ __attribute__((aligned(16))) float sb_lds[];
  const int Mt = a.Mt, D = a.D, nt = a.p.nt, MtP = nt * T, LDK = MtP + 1, ngrp = a.p.ngrp;
  float* Ks = sb_lds;                  // the K block: [n][m], m over all nt panels
  float* Vs = Ks + T * LDK;            // the weight block, then V: [n][m]
  float* stage = Vs + T * LDK;         // DIRECT: Z_j, X rows; else the slabs of a_j, b: [k][r]
  float* Ss = stage;                   // then a tile of Qs: [k = row of panel j][row of panel i]; then X of the step: [n][d]
  float* al = stage + kSbStage;        // alpha, zeros behind Mt
  float* wl = al + MtP;                // DIRECT: exp(-2 theta_d)
  float* nrm = wl + kRbfDirectD;       // !DIRECT: |a_j|^2, |b|^2
  float* gms = nrm + 2 * T;            // gm of the step's columns (0 where masked)
  float* gvs = gms + T;                // gv
  float* cn = gvs + T;                 // cn
  float* cok = cn + T;                 // 1 for a live column, 0 for a masked one
  float* cred = cok + T;               // [4][T]
  float* qred = cred + 4 * T;          // [4][32]: the waves' shares of k^T Qs k

  const int grp = blockIdx.x % ngrp, chunk = blockIdx.x / ngrp;
  const int dg0 = grp * 64 * NP;
  const int64_t g = blockIdx.y;
  const int64_t cbeg = (int64_t)chunk * a.p.ch.len;
  const int64_t cend = cbeg + a.p.ch.len < a.N ? cbeg + a.p.ch.len : a.N;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32, l31 = lane & 31, h = lane >> 5;
  const int pr = (wave & 1) * 32, pd = (wave >> 1) * 32;
  const float g2 = expf(2.f * a.theta[D]);
  float sg = 1.f;
  if constexpr (!TRANS) sg = a.gout[g];
  const float* __restrict__ Zg = a.Z + g * (int64_t)Mt * D;
  const float* __restrict__ X = a.X;
  const float* __restrict__ Qg = a.Q + g * (int64_t)Mt * Mt;
  const float* __restrict__ wg = a.w ? a.w + g * (int64_t)a.N : nullptr;
  const int Dl = D | 1;
  const typename LIK::Cls cls = LIK::cls(la, (int)g);

  si_f32x16 pacc[NP][kSiMaxNt];
#pragma unroll
  for (int t = 0; t < NP; ++t)
#pragma unroll
    for (int p = 0; p < kSiMaxNt; ++p)
#pragma unroll
      for (int r = 0; r < 16; ++r) pacc[t][p][r] = 0.f;
  float qacc[NP], aacc[kSiMaxNt], racc[kSiMaxNt];
#pragma unroll
  for (int t = 0; t < NP; ++t) qacc[t] = 0.f;
#pragma unroll
  for (int p = 0; p < kSiMaxNt; ++p) aacc[p] = racc[p] = 0.f;
  double s_th = 0.0, s_ls = 0.0;

  for (int e = tid; e < MtP; e += 256) al[e] = e < Mt ? a.alpha[g * Mt + e] : 0.f;
  if constexpr (DIRECT) {
    if (tid < D) wl[tid] = expf(-2.f * a.theta[tid]);
  }

  for (int64_t n0 = cbeg; n0 < cend; n0 += T) {
    if (tid < T) {
      const int64_t n = n0 + tid;
      bool live = n < cend && (!wg || wg[n] != 0.f);
      if constexpr (TRANS) live = live && LIK::live(la, (int)g, n);
      cok[tid] = live ? 1.f : 0.f;
    }
    __syncthreads();
    // ---- the K block and its weight: rows behind Mt and masked columns are zeros
    if constexpr (DIRECT) {
      float* Xs = stage + T * kMoDl;
      for (int e = tid; e < T * D; e += 256) {
        const int r = e / D, d = e - r * D;
        Xs[r * Dl + d] = cok[r] != 0.f ? X[(n0 + r) * D + d] : 0.f;
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
        for (int q = 0; q < 16; ++q) {
          const bool ok = rok && cok[16 * wave + q] != 0.f;
          Ks[(16 * wave + q) * LDK + j0 + lane] = ok ? EPI::off(g2, d2[q]) : 0.f;
          Vs[(16 * wave + q) * LDK + j0 + lane] = ok ? EpiDk<EPI>::w(g2, d2[q]) : 0.f;
        }
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
            Bs[k * LD + r] = (kok && cok[r] != 0.f) ? sq * X[(n0 + r) * D + k0 + k] : 0.f;
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
        const bool cl = cok[col] != 0.f;
        const float nb = nrm[T + col];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wr + (r & 3) + 8 * (r >> 2) + 4 * h;
          const bool ok = cl && j0 + row < Mt;
          const float d2 = nrm[row] + nb - 2.f * dj[r];
          Ks[col * LDK + j0 + row] = ok ? EPI::off(g2, d2) : 0.f;
          Vs[col * LDK + j0 + row] = ok ? EpiDk<EPI>::w(g2, d2) : 0.f;
        }
      }
      __syncthreads();
    }

    // ---- mu_n = alpha . k_n: the forward's sums
    {
      const float* kr = Ks + lane * LDK;
      float s = 0.f;
      for (int m = wave * (MtP >> 2); m < (wave + 1) * (MtP >> 2); ++m) s = fmaf(kr[m], al[m], s);
      cred[wave * T + lane] = s;
    }

    // ---- Qs K: the accumulators of every panel stay in registers; k_n^T Qs k_n from them in the forward's order
    si_f32x16 qk[kSiMaxNt];
    float qv = 0.f;
#pragma unroll
    for (int ti = 0; ti < kSiMaxNt; ++ti) {
      if (ti < nt) {
        const int i0 = ti * T;
        si_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int tj = 0; tj < nt; ++tj) {
          const int j0 = tj * T;
          for (int e = tid; e < T * T; e += 256) {
            const int k = e >> 6, r = e & 63;
            Ss[k * LD + r] = (i0 + r < Mt && j0 + k < Mt)
                                 ? 0.5f * (Qg[(int64_t)(j0 + k) * Mt + i0 + r] + Qg[(int64_t)(i0 + r) * Mt + j0 + k])
                                 : 0.f;
          }
          __syncthreads();
          // (sk_tile's loop, written out: through the shared piece this kernel measured 0.7 % slower at D = 784)
#pragma unroll
          for (int kk = 0; kk < T; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ss[(kk + h) * LD + wr + l31], Ks[(wc + l31) * LDK + j0 + kk + h], acc, 0, 0, 0);
          __syncthreads();
        }
        const float* kc = Ks + (wc + l31) * LDK + i0 + wr + 4 * h;
#pragma unroll
        for (int r = 0; r < 16; ++r) qv = fmaf(acc[r], kc[(r & 3) + 8 * (r >> 2)], qv);
        qk[ti] = acc;
      }
    }
    qv += __shfl_xor(qv, 32, 64);
    if (h == 0) qred[wave * 32 + l31] = qv;
    __syncthreads();

    // ---- the likelihood of the step's points: one wave, a point per lane
    if (tid < T) {
      const int64_t n = n0 + tid;
      const float mu = wave4_sum(cred, tid);
      const float quad = qred[(tid >> 5) * 32 + (tid & 31)] + qred[((tid >> 5) + 2) * 32 + (tid & 31)];
      const float var = fmaxf(g2 - quad, 0.f);
      float gm = 0.f, gv = 0.f;
      if (cok[tid] != 0.f) {
        const float wv = wg ? wg[n] : 1.f;
        real dmu = 0, dvar = 0, dpar = 0;
        LIK::template element<true>(cls, (real)mu, (real)var, LIK::template target<real>(la, (int)g, (size_t)n), dmu, dvar, dpar);
        gm = sg * (wv * (float)dmu);
        gv = g2 - quad > 0.f ? sg * (wv * (float)dvar) : 0.f;
        if (grp == 0) {
          s_th += 2.0 * (double)gm * (double)mu + (double)gv * (2.0 * (double)g2 - 4.0 * (double)quad);
          s_ls += (double)sg * (double)wv * (double)dpar;
        }
      }
      if (grp == 0 && n < cend) a.gv[g * (int64_t)a.N + n] = gv;
      gms[tid] = gm;
      gvs[tid] = gv;
    }
    __syncthreads();

    // ---- V = (gm alpha - 2 gv Qs K) o weight, in place; a masked column has weight 0
    {
      const int col = wc + l31;
      const float gmc = gms[col], gvc = -2.f * gvs[col];
#pragma unroll
      for (int p = 0; p < kSiMaxNt; ++p) {
        if (p < nt) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = p * T + wr + (r & 3) + 8 * (r >> 2) + 4 * h;
            Vs[col * LDK + row] *= fmaf(gvc, qk[p][r], gmc * al[row]);
          }
        }
      }
    }
    __syncthreads();

    // ---- galpha += K gm, r += V 1 (lanes = rows of a panel, every wave 16 of the columns); cn = V^T 1
#pragma unroll
    for (int p = 0; p < kSiMaxNt; ++p) {
      if (p < nt) {
        float s = 0.f, t = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          s = fmaf(Ks[(16 * wave + q) * LDK + p * T + lane], gms[16 * wave + q], s);
          t += Vs[(16 * wave + q) * LDK + p * T + lane];
        }
        aacc[p] += s;
        racc[p] += t;
      }
    }
    {
      const int n = tid >> 2, qd = tid & 3;       // four threads per column, a quarter of the rows each
      const float* vr = Vs + n * LDK;
      float t = 0.f;
      for (int m = qd * (MtP >> 2); m < (qd + 1) * (MtP >> 2); ++m) t += vr[m];
      cred[qd * T + n] = t;
    }
    __syncthreads();
    if (tid < T) cn[tid] = wave4_sum(cred, tid);

    // ---- P += V X, 64 values of d at a time; waves as (row half, half of the 64 values)
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      const int c0 = dg0 + t * 64;
      if (c0 < D) {
        for (int e = tid; e < T * T; e += 256) {
          const int n = e >> 6, c = e & 63;
          Ss[n * LD + c] = (cok[n] != 0.f && c0 + c < D) ? X[(n0 + n) * D + c0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < kSiMaxNt; ++p) {
          if (p < nt) {
#pragma unroll
            for (int kk = 0; kk < T; kk += 2)
              pacc[t][p] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[(kk + h) * LDK + p * T + pr + l31], Ss[(kk + h) * LD + pd + l31],
                                                                pacc[t][p], 0, 0, 0);
          }
        }
        {
          float s = 0.f;
#pragma unroll
          for (int q = 0; q < 16; ++q) { const float xv = Ss[(16 * wave + q) * LD + lane]; s = fmaf(cn[16 * wave + q] * xv, xv, s); }
          qacc[t] += s;
        }
        __syncthreads();
      }
    }
    __syncthreads();
  }

  const int64_t part = g * a.p.ch.nch + chunk;
#pragma unroll
  for (int t = 0; t < NP; ++t) {
    const int d = dg0 + t * 64 + pd + l31;
    if (d < D) {
#pragma unroll
      for (int p = 0; p < kSiMaxNt; ++p) {
        if (p < nt) {
          float* out = a.p.pp + (part * MtP + p * T) * (int64_t)D;
#pragma unroll
          for (int r = 0; r < 16; ++r) out[(int64_t)(pr + (r & 3) + 8 * (r >> 2) + 4 * h) * D + d] = pacc[t][p][r];
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NP; ++t) {
    __syncthreads();
    cred[wave * T + lane] = qacc[t];
    __syncthreads();
    const int d = dg0 + t * 64 + tid;
    if (tid < T && d < D) a.p.pq[part * D + d] = wave4_sum(cred, tid);
  }
  if (grp != 0) return;
#pragma unroll
  for (int p = 0; p < kSiMaxNt; ++p) {
    if (p < nt) {
      __syncthreads();
      cred[wave * T + lane] = aacc[p];
      qred[wave * T + lane] = racc[p];
      __syncthreads();
      if (tid < T) {
        a.p.pa[(part * nt + p) * T + tid] = wave4_sum(cred, tid);
        a.p.pr[(part * nt + p) * T + tid] = wave4_sum(qred, tid);
      }
    }
  }
  if (wave == 0) {
    s_th = wave_sum(s_th);
    s_ls = wave_sum(s_ls);
    if (lane == 0) { a.p.ps[part * 2] = s_th; a.p.ps[part * 2 + 1] = s_ls; }
  }
}

// The chunks' partials in ascending chunk order in fp64, then the outputs.  grid (cdiv(G * Mt * D, 256) + D + cdiv(G * Mt, 256) +
// 1): 256 entries of gZ | one value of d of gtheta (every thread a strided share of the (g, row) pairs and of the partials of q,
// then a fixed tree) | 256 entries of galpha | gtheta_D (the same tree) and gls
__global__ __launch_bounds__(256) void site_bwd_reduce_kernel(const SiteBwdArgs a) {
  constexpr int T = kMoT;
  __shared__ double red[256];
  const int Mt = a.Mt, D = a.D, MtP = a.p.nt * T, nch = a.p.ch.nch, tid = threadIdx.x;
  const int64_t total = (int64_t)a.G * Mt * D, rows = (int64_t)a.G * Mt;
  const int64_t nz = (total + 255) / 256, na = (rows + 255) / 256;
  const int64_t b = blockIdx.x;
  const BwdPartials part{a.p.pr, a.p.pp, a.p.pq, nch, MtP, 1};
  if (b < nz) {
    const int64_t e = b * 256 + tid;
    if (e < total) gz_entry(part, a.theta, a.Z, a.gZ, e, Mt, D);
  } else if (b < nz + D) {
    gtheta_d_block(part, a.theta, a.Z, a.gtheta, red, (int)(b - nz), a.G, Mt, D);
  } else if (b < nz + D + na) {
    const int64_t gm = (b - nz - D) * 256 + tid;
    if (gm >= rows) return;
    const float* p = a.p.pa + (gm / Mt) * nch * MtP + gm % Mt;
    double s = 0.0;
    for (int q = 0; q < nch; ++q) s += (double)p[(int64_t)q * MtP];
    a.galpha[gm] = (float)s;
  } else {
    double s = 0.0;
    for (int64_t e = tid; e < (int64_t)a.G * nch; e += 256) s += a.p.ps[2 * e];
    s = block_tree_sum(red, s);
    if (tid == 0) a.gtheta[D] = (float)s;
    if (a.gls) {
      for (int64_t g = tid; g < a.G; g += 256) {
        double t = 0.0;
        for (int q = 0; q < nch; ++q) t += a.p.ps[2 * (g * nch + q) + 1];
        a.gls[g] = (float)t;
      }
    }
  }
}

template <class LIK, class EPI, bool DIRECT, int NP>
static int site_bwd_launch_form(const SiteBwdArgs& a, const typename LIK::Args& la, hipStream_t st) {
  constexpr auto kernel = site_bwd_kernel<LIK, EPI, DIRECT, NP>;
  if (int rc = reserve_dynamic_lds<kernel>(site_bwd_lds_floats(kSiMaxNt) * sizeof(float),
                                           kSiteTransport<LIK> ? "site_transport_bwd" : "site_bound_bwd"))
    return rc;
  hipLaunchKernelGGL(kernel, dim3(a.p.ch.nch * a.p.ngrp, a.G), dim3(256), site_bwd_lds_floats(a.p.nt) * sizeof(float), st, a, la);
  return VARGP_OK;
}

template <class LIK>
static int site_bwd_launch(const SiteBwdArgs& a, const typename LIK::Args& la, int nu2, hipStream_t st) {
  return with_epi(nu2, [&](auto epi) {
    using EPI = decltype(epi);
    return a.D <= kRbfDirectD ? site_bwd_launch_form<LIK, EPI, true, 1>(a, la, st)
                              : site_bwd_launch_form<LIK, EPI, false, kSbNPMax>(a, la, st);
  });
}

// f(LIK{}, its Args) for the likelihood a (checked) kind names
template <class F>
static int with_site_lik(int kind, const float* y, int64_t ldy, const float* log_scale, float df, float lognorm, F f) {
  switch (kind) {
    case VARGP_SITE_BERNOULLI_PROBIT: return f(Bernoulli<LinkProbit>{}, Bernoulli<LinkProbit>::Args{y, ldy, nullptr});
    case VARGP_SITE_BERNOULLI_LOGIT: return f(Bernoulli<LinkLogit>{}, Bernoulli<LinkLogit>::Args{y, ldy, nullptr});
    case VARGP_SITE_POISSON: return f(Poisson{}, Poisson::Args{{y, ldy}});
    default: return f(StudentT{}, StudentT::Args{{y, ldy}, log_scale, df, lognorm});
  }
}

// The argument checks of both entries, in one order.  ptrs: all of the entry's required pointers are there; st_ok / st_needs: what
// the entry asks of a Student-t call
static int site_check_args(const char* name, bool ptrs, int64_t ldy, int kind, bool st_ok, const char* st_needs, int G, int Mt, int N,
                           int D, int nu2, const void* ws, size_t ws_bytes, size_t ws_need) {
  VARGP_REQUIRE(ptrs, "%s: null pointer", name);
  VARGP_REQUIRE(G > 0 && Mt > 0 && N > 0 && D > 0, "%s: bad dims", name);
  VARGP_REQUIRE(kind >= VARGP_SITE_BERNOULLI_PROBIT && kind <= VARGP_SITE_STUDENTT,
                "%s: kind = %d (0: Bernoulli probit, 1: Bernoulli logit, 2: Poisson, 3: Student-t)", name, kind);
  VARGP_REQUIRE(nu2 == 0 || nu2 == 1 || nu2 == 3 || nu2 == 5, "%s: nu2 = %d (0: RBF; 1, 3, 5: Matern)", name, nu2);
  VARGP_REQUIRE(G <= 65535, "%s: G = %d (at most 65535)", name, G);
  VARGP_REQUIRE(Mt <= kSiMaxMt, "%s: Mt = %d (at most %d: the K block of all rows lives in LDS)", name, Mt, kSiMaxMt);
  VARGP_REQUIRE(ldy == 0 || ldy >= N, "%s: ldy must be 0 or >= N", name);
  VARGP_REQUIRE(kind != VARGP_SITE_STUDENTT || st_ok, "%s: Student-t needs %s", name, st_needs);
  VARGP_REQUIRE(reinterpret_cast<uintptr_t>(ws) % sizeof(double) == 0, "%s: ws must be 8-byte aligned", name);
  VARGP_REQUIRE(ws_bytes >= ws_need, "%s: workspace too small", name);
  return VARGP_OK;
}

}  // namespace vargp

using namespace vargp;

extern "C" int vargp_site_bound_bwd_chunks(int G, int Mt, int N, int D) {
  if (G <= 0 || Mt <= 0 || N <= 0 || D <= 0) return 0;
  return site_bwd_plan(nullptr, G, Mt, N, D).ch.nch;
}

extern "C" size_t vargp_site_bound_bwd_workspace_bytes(int G, int Mt, int N, int D) {
  if (G <= 0 || Mt <= 0 || N <= 0 || D <= 0) return 0;
  return site_bwd_plan(nullptr, G, Mt, N, D).bytes + 256;
}

extern "C" int vargp_site_bound_bwd(const float* theta, const float* Z, const float* X, const float* alpha, const float* Q,
                                    const float* y, int64_t ldy, const float* w, int kind, const float* log_scale, float df,
                                    float lognorm, const float* gout, float* gZ, float* gtheta, float* galpha, float* gv, float* gls,
                                    int G, int Mt, int N, int D, int nu2, void* ws, size_t ws_bytes, vargp_stream_t stream) {
  if (int rc = site_check_args("site_bound_bwd", theta && Z && X && alpha && Q && y && gout && gZ && gtheta && galpha && gv && ws, ldy,
                               kind, log_scale && gls && df > 0.f, "log_scale, gls and df > 0", G, Mt, N, D, nu2, ws, ws_bytes,
                               vargp_site_bound_bwd_workspace_bytes(G, Mt, N, D)))
    return rc;
  SiteBwdArgs a{};
  a.theta = theta; a.Z = Z; a.X = X; a.alpha = alpha; a.Q = Q; a.w = w; a.gout = gout;
  a.gZ = gZ; a.gtheta = gtheta; a.galpha = galpha; a.gv = gv; a.gls = kind == VARGP_SITE_STUDENTT ? gls : nullptr;
  a.p = site_bwd_plan(ws, G, Mt, N, D);
  a.G = G; a.Mt = Mt; a.N = N; a.D = D;
  const int64_t nred = cdiv((int64_t)G * Mt * D, 256) + D + cdiv((int64_t)G * Mt, 256) + 1;
  VARGP_REQUIRE((int64_t)a.p.ch.nch * a.p.ngrp < (1ll << 31) && nred < (1ll << 31),
                "site_bound_bwd: G = %d, Mt = %d, D = %d need too many workgroups", G, Mt, D);
  hipStream_t st = as_stream(stream);
  ProfScope whole("site_bound_bwd", st);
  const int rc = with_site_lik(kind, y, ldy, log_scale, df, lognorm,
                               [&](auto lik, const auto& la) { return site_bwd_launch<decltype(lik)>(a, la, nu2, st); });
  if (rc != VARGP_OK) return rc;
  hipLaunchKernelGGL(site_bwd_reduce_kernel, dim3((unsigned)nred), dim3(256), 0, st, a);
  return check_launch("site_bound_bwd");
}

extern "C" int vargp_site_transport_bwd_chunks(int G, int Mt, int N, int D) { return vargp_site_bound_bwd_chunks(G, Mt, N, D); }

extern "C" size_t vargp_site_transport_bwd_workspace_bytes(int G, int Mt, int N, int D) {
  return vargp_site_bound_bwd_workspace_bytes(G, Mt, N, D);
}

extern "C" int vargp_site_transport_bwd(const float* theta, const float* Z, const float* X, const float* alpha, const float* Q,
                                        const float* gm, const float* gv, float* gZ, float* gtheta, float* galpha, float* gv_out,
                                        int G, int Mt, int N, int D, int nu2, void* ws, size_t ws_bytes, vargp_stream_t stream) {
  // (no targets and no likelihood: the checks of the sibling entry with a shared row of targets and a kind without parameters)
  if (int rc = site_check_args("site_transport_bwd", theta && Z && X && alpha && Q && gm && gv && gZ && gtheta && galpha && gv_out && ws,
                               0, VARGP_SITE_BERNOULLI_PROBIT, true, "", G, Mt, N, D, nu2, ws, ws_bytes,
                               vargp_site_transport_bwd_workspace_bytes(G, Mt, N, D)))
    return rc;
  SiteBwdArgs a{};
  a.theta = theta; a.Z = Z; a.X = X; a.alpha = alpha; a.Q = Q;
  a.gZ = gZ; a.gtheta = gtheta; a.galpha = galpha; a.gv = gv_out;
  a.p = site_bwd_plan(ws, G, Mt, N, D);
  a.G = G; a.Mt = Mt; a.N = N; a.D = D;
  const int64_t nred = cdiv((int64_t)G * Mt * D, 256) + D + cdiv((int64_t)G * Mt, 256) + 1;
  VARGP_REQUIRE((int64_t)a.p.ch.nch * a.p.ngrp < (1ll << 31) && nred < (1ll << 31),
                "site_transport_bwd: G = %d, Mt = %d, D = %d need too many workgroups", G, Mt, D);
  hipStream_t st = as_stream(stream);
  ProfScope whole("site_transport_bwd", st);
  if (int rc = site_bwd_launch<SiteTransport>(a, SiteTransport::Args{gm, gv, (int64_t)N}, nu2, st)) return rc;
  hipLaunchKernelGGL(site_bwd_reduce_kernel, dim3((unsigned)nred), dim3(256), 0, st, a);
  return check_launch("site_transport_bwd");
}

extern "C" int vargp_site_moments_chunks(int G, int Mt, int N, int D) {
  if (G <= 0 || Mt <= 0 || N <= 0 || D <= 0) return 0;
  return site_plan(nullptr, G, Mt, N).ch.nch;
}

extern "C" size_t vargp_site_moments_workspace_bytes(int G, int Mt, int N, int D) {
  if (G <= 0 || Mt <= 0 || N <= 0 || D <= 0) return 0;
  return site_plan(nullptr, G, Mt, N).bytes + 256;
}

extern "C" int vargp_site_moments(const float* theta, const float* Z, const float* X, const float* alpha, const float* Q,
                                  const float* y, int64_t ldy, const float* w, int kind, const float* log_scale, float df,
                                  float lognorm, float* lam2, float* c, float* sums, int G, int Mt, int N, int D, int nu2, void* ws,
                                  size_t ws_bytes, vargp_stream_t stream) {
  if (int rc = site_check_args("site_moments", theta && Z && X && alpha && Q && y && lam2 && c && sums && ws, ldy, kind,
                               log_scale && df > 0.f, "log_scale and df > 0", G, Mt, N, D, nu2, ws, ws_bytes,
                               vargp_site_moments_workspace_bytes(G, Mt, N, D)))
    return rc;
  SiteArgs a{};
  a.theta = theta; a.Z = Z; a.X = X; a.alpha = alpha; a.Q = Q; a.w = w; a.lam2 = lam2; a.c = c; a.sums = sums;
  a.p = site_plan(ws, G, Mt, N);
  a.G = G; a.Mt = Mt; a.N = N; a.D = D;
  hipStream_t st = as_stream(stream);
  ProfScope whole("site_moments", st);
  const int rc = with_site_lik(kind, y, ldy, log_scale, df, lognorm,
                               [&](auto lik, const auto& la) { return site_launch<decltype(lik)>(a, la, nu2, st); });
  if (rc != VARGP_OK) return rc;
  hipLaunchKernelGGL(site_reduce_kernel, dim3(cdiv(Mt, 256) + 1, G), dim3(256), 0, st, a);
  return check_launch("site_moments");
}

extern "C" int vargp_site_marginals(const float* theta, const float* Z, const float* X, const float* alpha, const float* Q, float* mu,
                                    float* var, int G, int Mt, int N, int D, int nu2, vargp_stream_t stream) {
  VARGP_REQUIRE(theta && Z && X && alpha && Q && mu && var, "site_marginals: null pointer");
  VARGP_REQUIRE(G > 0 && Mt > 0 && N > 0 && D > 0, "site_marginals: bad dims");
  VARGP_REQUIRE(nu2 == 0 || nu2 == 1 || nu2 == 3 || nu2 == 5, "site_marginals: nu2 = %d (0: RBF; 1, 3, 5: Matern)", nu2);
  VARGP_REQUIRE(G <= 65535, "site_marginals: G = %d (at most 65535)", G);
  VARGP_REQUIRE(Mt <= kSiMaxMt, "site_marginals: Mt = %d (at most %d: the K block of all rows lives in LDS)", Mt, kSiMaxMt);
  SiteArgs a{};
  a.theta = theta; a.Z = Z; a.X = X; a.alpha = alpha; a.Q = Q;
  a.p = site_plan(nullptr, G, Mt, N);          // the chunking alone: the marginals leave no partials
  a.G = G; a.Mt = Mt; a.N = N; a.D = D;
  hipStream_t st = as_stream(stream);
  ProfScope whole("site_marginals", st);
  if (int rc = site_launch<SiteMarginals>(a, SiteMarginals::Args{mu, var}, nu2, st)) return rc;
  return check_launch("site_marginals");
}

extern "C" int vargp_site_cavity_chunks(int G, int Mt, int N, int D) { return vargp_site_moments_chunks(G, Mt, N, D); }

extern "C" size_t vargp_site_cavity_workspace_bytes(int G, int Mt, int N, int D) {
  if (G <= 0 || Mt <= 0 || N <= 0 || D <= 0) return 0;
  return (size_t)round_up((int64_t)G * site_plan(nullptr, G, Mt, N).ch.nch * (int64_t)sizeof(double), 256) + 256;
}

extern "C" int vargp_site_cavity(const float* theta, const float* Z, const float* X, const float* alpha, const float* Q,
                                 const float* V, const float* y, int64_t ldy, const float* w, int kind, const float* log_scale,
                                 float df, float lognorm, float* mu, float* var, float* s, float* mu_c, float* var_c, float* lam1,
                                 float* lam2, long long* n_unstable, int G, int Mt, int Mv, int N, int D, int nu2, void* ws,
                                 size_t ws_bytes, vargp_stream_t stream) {
  const bool marg = kind < 0;
  // (the marginals form has no targets, no likelihood and no partials: the checks of the site form with a shared row of targets
  // and a kind without parameters)
  if (int rc = site_check_args("site_cavity",
                               theta && Z && X && alpha && Q && V && mu && var && s &&
                                   (marg || (y && mu_c && var_c && lam1 && lam2 && n_unstable && ws)),
                               marg ? 0 : ldy, marg ? VARGP_SITE_BERNOULLI_PROBIT : kind, log_scale && df > 0.f, "log_scale and df > 0", G,
                               Mt, N, D, nu2, marg ? nullptr : ws, marg ? 0 : ws_bytes,
                               marg ? 0 : vargp_site_cavity_workspace_bytes(G, Mt, N, D)))
    return rc;
  VARGP_REQUIRE(Mv > 0 && Mv <= Mt, "site_cavity: Mv = %d (1 to Mt = %d rows of V)", Mv, Mt);
  SiteArgs a{};
  a.theta = theta; a.Z = Z; a.X = X; a.alpha = alpha; a.Q = Q; a.w = w;
  a.p = site_plan(nullptr, G, Mt, N);          // the chunking alone: the partials are the counts at ws
  a.G = G; a.Mt = Mt; a.N = N; a.D = D;
  hipStream_t st = as_stream(stream);
  ProfScope whole("site_cavity", st);
  if (marg) {
    using C = Cavity<SiteMarginals>;
    if (int rc = site_launch<C>(a, C::Args{{}, V, mu, var, s, nullptr, nullptr, nullptr, nullptr, nullptr, Mv}, nu2, st)) return rc;
    return check_launch("site_cavity");
  }
  double* pu = reinterpret_cast<double*>(ws);
  const int rc = with_site_lik(kind, y, ldy, log_scale, df, lognorm, [&](auto lik, const auto& la) {
    using C = Cavity<decltype(lik)>;
    return site_launch<C>(a, typename C::Args{la, V, mu, var, s, mu_c, var_c, lam1, lam2, pu, Mv}, nu2, st);
  });
  if (rc != VARGP_OK) return rc;
  hipLaunchKernelGGL(cavity_reduce_kernel, dim3(cdiv(G, 256)), dim3(256), 0, st, pu, n_unstable, G, a.p.ch.nch);
  return check_launch("site_cavity");
}
