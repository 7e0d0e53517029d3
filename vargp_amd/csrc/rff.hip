// Random-Fourier-feature paths: for every (hyper-sample s, output c) the product of the feature matrix of a point set with
// a block of weight columns,
//
//   p[s, i, r]      = sum_d X[i, d] omega[r, d] / ell[s, d]                         (phases, radians)
//   Phi_s(X)[i, :]  = gamma_s / sqrt(R) [cos p[s, i, :] | sin p[s, i, :]]           (n x 2R)
//   out[s, c, i, k] = sum_j Phi_s(X)[i, j] coef[s, c, j, k]                         (n x N)
//
// Composed from the existing entries -- a GEMM over D, cos / sin, a GEMM over the 2R features -- the S n 2R feature matrix is
// written to memory and read back; here it never leaves the chip.  A workgroup owns 64 points x BN output columns for ALL of R
// and walks the frequencies 64 at a time:
//   1. the 64 x 64 phase tile over D on the f32 MFMA (v_mfma_f32_32x32x2_f32; operands: the points as they are and the
//      frequencies pre-divided by the lengthscales of the hyper-sample, rff_prep_kernel -- the x o w idea of rbf_prep_norm_launch);
//   2. cos / sin and the gamma / sqrt(R) scale on the accumulators, in registers;
//   3. the 128 feature columns of the step staged in LDS as the A operand of the second product, whose accumulators (64 x BN,
//      BN = 64 WN) live across the whole loop over R;
//   4. one store at the end.  No atomics, one summation order: two calls are bitwise equal.
// x_shared = 1: one point set for all outputs, so the C N columns of a hyper-sample sit behind ONE set of features (batch =
// s, column q = c N + k).  x_shared = 0: a point set per output (the inducing points), batch = (s, c), N columns.
//
// sin / cos: the phase is reduced to revolutions first, t = p / (2 pi) as an exact two-term product (p c_hi + p c_lo with
// c_hi + c_lo = 1 / (2 pi) to 2^-50, the rounding error of p c_hi recovered with an fma), frac(t) taken exactly, and the
// hardware v_sin_f32 / v_cos_f32 (input in revolutions) evaluated on the fraction: the error does not grow with |p| beyond the
// fp32 rounding of p itself.  (__sinf / __cosf multiply by a single-float 1 / (2 pi): an error of |p| 2^-25 radians.)
//
// Tiles as pred_cov.hip: four waves as 2 x 2, slabs staged in LDS as [k][64 + 1], fragment maps as in gemm.hip.  The phase
// product's next slab is fetched into registers while the current one is multiplied.  Any n, D, R, N: every staging load is
// guarded and out-of-range elements enter as zeros.
//
// The backward in the points (vargp_rff_paths_bwd, rff_paths_bwd_kernel), gout [S][C][n][N] -> gX [n][D] | [C][n][D]:
//
//   h[s, i, r] = sum_(c, k) gout[s, c, i, k] (-sin p[s, i, r] coef[s, c, r, k] + cos p[s, i, r] coef[s, c, R + r, k])
//   gX[i, d]   = sum_s gamma_s / sqrt(R) sum_r h[s, i, r] omega[r, d] / ell[s, d]
//
// (x_shared = 0: the sum in h runs over k only and gX keeps its c index.)  The same frame: a workgroup owns 64 points x BN = 64 WN
// input dimensions of gX (WN = 1 | 2 | 4, 256-wide tiles of D side by side), one batch entry and one piece of R, and per 64
// frequencies forms
//   1. the phase tile, exactly as the forward kernel (same operands from rff_prep_kernel, same slabs, same prefetch);
//   2. tc = gout coef[:R]^T and ts = gout coef[R:]^T over the C N (or N) columns, slabs of 16 columns of both staged through
//      the area of the phase slabs -- 64 x 64 tiles with the SAME fragment map as the phases (point on the registers,
//      frequency on the lanes);
//   3. h = gamma / sqrt(R) (cos p ts - sin p tc) register by register with rff_sincos, stored to LDS as [frequency][point];
//   4. gacc += h om: h is the A operand, the 64 rows of om (slabs of 64 | 32 | 16 rows through the same staging area) the B
//      operand; gacc (64 x BN) lives across the loop over R.
// Neither p, the features nor h reach memory.  The sum over the hyper-samples and over the pieces of R (as many pieces as bring
// the launch to about 512 workgroups -- a function of the sizes alone) is not done with atomics: every workgroup stores its
// tile of ONE partial sum [s][piece] in the workspace and rff_bwd_reduce_kernel adds them in ascending order (a single
// partial sum is stored to gX directly).  One summation order: two calls are bitwise equal.  A D tile recomputes the phases
// over all of D, which is the price of keeping h on the chip: D = 784 is four tiles.
#include <algorithm>

#include "common.h"

namespace vargp {

typedef float rf_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kRfBM = 64, kRfBR = 64, kRfBK = 32;

struct RffArgs {
  const float *X, *om, *gs, *coef;     // om [S][R][D] = omega / ell_s;  gs [S] = gamma_s / sqrt(R)
  float* out;
  int C, n, D, R, N;
  int shared, Cc, cols;                // Cc = outputs behind one batch entry (C | 1); cols = Cc N
};

__global__ __launch_bounds__(256) void rff_prep_kernel(const float* __restrict__ theta, const float* __restrict__ omega,
                                                       float* __restrict__ om, float* __restrict__ gs, int S, int D, int R) {
  const int64_t RD = (int64_t)R * D, total = (int64_t)S * RD;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < S) gs[i] = expf(theta[i * (D + 1) + D]) / sqrtf((float)R);
  if (i >= total) return;
  const int64_t s = i / RD, rd = i - s * RD;
  om[i] = omega[rd] * expf(-theta[s * (D + 1) + rd % D]);
}

// sin and cos of p radians through revolutions (see the head of the file)
__device__ __forceinline__ void rff_sincos(float p, float& sn, float& cs) {
  constexpr double kInv2Pi = 0.15915494309189533577;
  constexpr float c_hi = (float)kInv2Pi, c_lo = (float)(kInv2Pi - (double)c_hi);
  const float t = p * c_hi;
  const float lo = fmaf(p, c_lo, fmaf(p, c_hi, -t));
  const float u = __builtin_amdgcn_fractf(t) + lo;
  sn = __builtin_amdgcn_sinf(u);
  cs = __builtin_amdgcn_cosf(u);
}

template <int WN>
__global__ __launch_bounds__(256, 2) void rff_paths_kernel(const RffArgs a) {
  constexpr int BM = kRfBM, BR = kRfBR, BK = kRfBK, LD = BM + 1, BN = 64 * WN, LDN = BN + 1;
  constexpr int JK = ((2 * BK * LD) / LDN) & ~1;        // rows of coef that fit the staging area: 64 | 32 | 16
  static_assert(BM == BR && BM * BK == 8 * 256 && JK * BN == 16 * 256 && (2 * BR) % JK == 0, "rff: tile shape");
  __shared__ float stage[2 * BK * LD];                  // the slabs of the phase product; then the slabs of coef
  __shared__ float feat[2 * BR * LD];                   // [cos of 64 frequencies | sin of them][point]
  float* Xs = stage;
  float* Os = stage + BK * LD;

  const int row0 = blockIdx.x * BM, col0 = blockIdx.y * BN;
  const int64_t b = blockIdx.z;
  const int n = a.n, D = a.D, R = a.R, N = a.N;
  const int s = a.shared ? (int)b : (int)(b / a.C);
  const float* __restrict__ Xb = a.shared ? a.X : a.X + (b % a.C) * n * D;
  const float* __restrict__ om = a.om + (int64_t)s * R * D;
  const float g = a.gs[s];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 32, wf = (wave & 1) * 32, wc = (wave & 1) * 32 * WN;
  const int l31 = lane & 31, h = lane >> 5;

  // this thread's column of the coef slabs (256 is a multiple of BN or BN of 256: the same one in every pass)
  const int cq = col0 + tid % BN;
  const bool cq_ok = cq < a.cols;
  const int cq_c = cq_ok ? cq / N : 0, cq_k = cq_ok ? cq - cq_c * N : 0;
  const float* __restrict__ cfq = a.coef + (b * a.Cc + cq_c) * 2 * R * N + cq_k;

  rf_f32x16 oacc[WN];
#pragma unroll
  for (int w = 0; w < WN; ++w)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[w][r] = 0.f;

  // slab (r0, k0) of the phase product, global -> registers -> LDS
  float xr[8], orr[8];
  auto gload = [&](int r0, int k0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = tid + 256 * i, r = e / BK, k = e % BK;
      const bool kok = k0 + k < D;
      xr[i] = (kok && row0 + r < n) ? Xb[(int64_t)(row0 + r) * D + k0 + k] : 0.f;
      orr[i] = (kok && r0 + r < R) ? om[(int64_t)(r0 + r) * D + k0 + k] : 0.f;
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = tid + 256 * i, r = e / BK, k = e % BK;
      Xs[k * LD + r] = xr[i];
      Os[k * LD + r] = orr[i];
    }
  };

  gload(0, 0);
  for (int r0 = 0; r0 < R; r0 += BR) {
    // 1. phases of 64 points x 64 frequencies; this wave: rows wr.., frequencies wf..
    rf_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < D; k0 += BK) {
      lstore();
      __syncthreads();
      int nk = k0 + BK, nr = r0;
      if (nk >= D) { nk = 0; nr = r0 + BR; }
      if (nr < R) gload(nr, nk);
#pragma unroll
      for (int k = 0; k < BK; k += 2) {
        const float af = Xs[(k + h) * LD + wr + l31];
        const float bf = Os[(k + h) * LD + wf + l31];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf, acc, 0, 0, 0);
      }
      __syncthreads();
    }

    // 2. features, in registers; 3. to LDS as [feature][point]
    const bool fok = r0 + wf + l31 < R;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wr + (r & 3) + 8 * (r >> 2) + 4 * h;
      float sn, cs;
      rff_sincos(acc[r], sn, cs);
      feat[(wf + l31) * LD + row] = fok ? g * cs : 0.f;
      feat[(BR + wf + l31) * LD + row] = fok ? g * sn : 0.f;
    }
    __syncthreads();

    // the second product over the 128 features of this step, JK at a time (local feature jj: cos of frequency r0 + jj for
    // jj < 64, sin of frequency r0 + jj - 64 after -- rows r0 + jj and R + r0 + jj - 64 of coef)
    for (int js = 0; js < 2 * BR; js += JK) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int jl = (tid + 256 * i) / BN, jj = js + jl;
        const int f = r0 + (jj & (BR - 1));
        const int64_t j = jj < BR ? f : (int64_t)R + f;
        stage[jl * LDN + tid % BN] = (cq_ok && f < R) ? cfq[j * N] : 0.f;
      }
      __syncthreads();
#pragma unroll 8
      for (int k = 0; k < JK; k += 2) {
        const float af = feat[(js + k + h) * LD + wr + l31];
#pragma unroll
        for (int w = 0; w < WN; ++w)
          oacc[w] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, stage[(k + h) * LDN + wc + 32 * w + l31], oacc[w], 0, 0, 0);
      }
      __syncthreads();
    }
  }

  // 4. the only store
#pragma unroll
  for (int w = 0; w < WN; ++w) {
    const int q = col0 + wc + 32 * w + l31;
    if (q >= a.cols) continue;
    const int c = q / N, k = q - c * N;
    float* __restrict__ o = a.out + (b * a.Cc + c) * n * N + k;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + wr + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (row < n) o[(int64_t)row * N] = oacc[w][r];
    }
  }
}

// ---- backward in the points -------------------------------------------------------------------------------------------------
struct RffBwdArgs {
  const float *X, *om, *gs, *coef, *gout;
  float* dst;                          // gX itself when there is one partial sum, else the partial sums [S KS][Cx][n][D]
  int C, n, D, R, N;
  int shared, Cc, cols;                // as RffArgs
  int KS, steps;                       // the loop over R is cut into KS pieces of `steps` 64-frequency steps
};

// One workgroup: 64 points x BN = 64 WN input dimensions of gX for one batch entry and one piece of R.  Per step of 64
// frequencies: acc = the phase tile (as the forward kernel); tc, ts = gout coef^T for the cos and the sin rows of coef, in the
// SAME fragment positions as acc (point on the registers, frequency on the lanes), so h is formed register by register; h goes
// to LDS as [frequency][point], the A operand of h om, whose accumulators gacc live across the loop.
template <int WN>
__global__ __launch_bounds__(256, 2) void rff_paths_bwd_kernel(const RffBwdArgs a) {
  constexpr int BM = kRfBM, BR = kRfBR, BK = kRfBK, LD = BM + 1, BN = 64 * WN, LDN = BN + 1;
  constexpr int JK = ((2 * BK * LD) / LDN) & ~1;        // rows of om that fit the staging area: 64 | 32 | 16
  constexpr int QK = 16, LDC = 2 * BR + 1;              // columns (c, k) per slab of gout coef^T
  static_assert(BM == BR && BM * BK == 8 * 256 && JK * BN == 16 * 256 && BR % JK == 0, "rff bwd: tile shape");
  static_assert(QK * (LD + LDC) <= 2 * BK * LD && QK * BM == 4 * 256 && QK * 2 * BR == 8 * 256, "rff bwd: slabs of gout, coef");
  __shared__ float stage[2 * BK * LD];                  // the slabs of the phase product; of gout and coef; of om
  __shared__ float hs[BR * LD];                         // h [frequency][point]
  float* Xs = stage;
  float* Os = stage + BK * LD;
  float* Gs = stage;
  float* Cs = stage + QK * LD;

  const int dt = blockIdx.y / a.KS, ks = blockIdx.y - dt * a.KS;
  const int row0 = blockIdx.x * BM, col0 = dt * BN;
  const int64_t b = blockIdx.z;
  const int n = a.n, D = a.D, R = a.R, N = a.N;
  const int s = a.shared ? (int)b : (int)(b / a.C);
  const int cc = a.shared ? 0 : (int)(b % a.C);
  const float* __restrict__ Xb = a.X + (int64_t)cc * n * D;
  const float* __restrict__ om = a.om + (int64_t)s * R * D;
  const float g = a.gs[s];
  const int rbeg = ks * a.steps * BR, rend = min(R, rbeg + a.steps * BR);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 32, wf = (wave & 1) * 32, wc = (wave & 1) * 32 * WN;
  const int l31 = lane & 31, h = lane >> 5;

  // this thread's column of the om slabs
  const int dq = col0 + tid % BN;
  const bool dq_ok = dq < D;
  const float* __restrict__ omd = om + (dq_ok ? dq : 0);

  rf_f32x16 gacc[WN];
#pragma unroll
  for (int w = 0; w < WN; ++w)
#pragma unroll
    for (int r = 0; r < 16; ++r) gacc[w][r] = 0.f;

  float xr[8], orr[8];
  auto gload = [&](int r0, int k0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = tid + 256 * i, r = e / BK, k = e % BK;
      const bool kok = k0 + k < D;
      xr[i] = (kok && row0 + r < n) ? Xb[(int64_t)(row0 + r) * D + k0 + k] : 0.f;
      orr[i] = (kok && r0 + r < R) ? om[(int64_t)(r0 + r) * D + k0 + k] : 0.f;
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = tid + 256 * i, r = e / BK, k = e % BK;
      Xs[k * LD + r] = xr[i];
      Os[k * LD + r] = orr[i];
    }
  };

  gload(rbeg, 0);
  for (int r0 = rbeg; r0 < rend; r0 += BR) {
    // 1. phases of 64 points x 64 frequencies; this wave: rows wr.., frequencies wf..
    rf_f32x16 acc, tc, ts;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = tc[r] = ts[r] = 0.f;
    for (int k0 = 0; k0 < D; k0 += BK) {
      lstore();
      __syncthreads();
      int nk = k0 + BK, nr = r0;
      if (nk >= D) { nk = 0; nr = r0 + BR; }
      if (nr < rend) gload(nr, nk);
#pragma unroll
      for (int k = 0; k < BK; k += 2) {
        const float af = Xs[(k + h) * LD + wr + l31];
        const float bf = Os[(k + h) * LD + wf + l31];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf, acc, 0, 0, 0);
      }
      __syncthreads();
    }

    // 2. gout coef^T over the columns q = (c, k), QK at a time: tc against row r0 + f of coef, ts against row R + r0 + f
    for (int q0 = 0; q0 < a.cols; q0 += QK) {
      const int ql = tid & (QK - 1), il = tid / QK, q = q0 + ql;
      const bool qok = q < a.cols;
      const int qc = qok ? q / N : 0, qk = qok ? q - qc * N : 0;
      const float* __restrict__ gq = a.gout + (b * a.Cc + qc) * n * N + qk;
      const float* __restrict__ cq = a.coef + (b * a.Cc + qc) * 2 * R * N + qk;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = il + 16 * t;
        Gs[ql * LD + i] = (qok && row0 + i < n) ? gq[(int64_t)(row0 + i) * N] : 0.f;
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int jl = il + 16 * t, f = r0 + (jl & (BR - 1));
        const int64_t j = jl < BR ? f : (int64_t)R + f;
        Cs[ql * LDC + jl] = (qok && f < R) ? cq[j * N] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < QK; k += 2) {
        const float af = Gs[(k + h) * LD + wr + l31];
        tc = __builtin_amdgcn_mfma_f32_32x32x2f32(af, Cs[(k + h) * LDC + wf + l31], tc, 0, 0, 0);
        ts = __builtin_amdgcn_mfma_f32_32x32x2f32(af, Cs[(k + h) * LDC + BR + wf + l31], ts, 0, 0, 0);
      }
      __syncthreads();
    }

    // 3. h = gamma / sqrt(R) (cos p ts - sin p tc), in registers; to LDS as [frequency][point].  Frequencies >= R: coef entered
    // as zeros, so h is zero there
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wr + (r & 3) + 8 * (r >> 2) + 4 * h;
      float sn, cs;
      rff_sincos(acc[r], sn, cs);
      hs[(wf + l31) * LD + row] = g * (cs * ts[r] - sn * tc[r]);
    }
    __syncthreads();

    // 4. gacc += h om over the 64 frequencies of this step, JK at a time
    for (int js = 0; js < BR; js += JK) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int jl = (tid + 256 * i) / BN, r = r0 + js + jl;
        stage[jl * LDN + tid % BN] = (dq_ok && r < R) ? omd[(int64_t)r * D] : 0.f;
      }
      __syncthreads();
#pragma unroll 8
      for (int k = 0; k < JK; k += 2) {
        const float af = hs[(js + k + h) * LD + wr + l31];
#pragma unroll
        for (int w = 0; w < WN; ++w)
          gacc[w] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, stage[(k + h) * LDN + wc + 32 * w + l31], gacc[w], 0, 0, 0);
      }
      __syncthreads();
    }
  }

  // the only store: this (hyper-sample, piece of R)'s share of gX
  const int Cx = a.shared ? 1 : a.C;
  float* __restrict__ dst = a.dst + (((int64_t)s * a.KS + ks) * Cx + cc) * n * D;
#pragma unroll
  for (int w = 0; w < WN; ++w) {
    const int d = col0 + wc + 32 * w + l31;
    if (d >= D) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + wr + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (row < n) dst[(int64_t)row * D + d] = gacc[w][r];
    }
  }
}

// gX[e] = sum_p part[p][e], p ascending: one summation order
__global__ __launch_bounds__(256) void rff_bwd_reduce_kernel(const float* __restrict__ part, float* __restrict__ gX, int P,
                                                             int64_t E) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  float acc = part[e];
  for (int p = 1; p < P; ++p) acc += part[(int64_t)p * E + e];
  gX[e] = acc;
}

}  // namespace vargp

using namespace vargp;

// om [S][R][D] and gs [S], each rounded up to 64 floats
static size_t rff_ws_floats(int S, int D, int R) { return (size_t)(round_up((int64_t)S * R * D, 64) + round_up(S, 64)); }

extern "C" size_t vargp_rff_paths_workspace_bytes(int S, int D, int R) {
  if (S <= 0 || D <= 0 || R <= 0) return 0;
  return rff_ws_floats(S, D, R) * sizeof(float) + 256;
}

extern "C" int vargp_rff_paths(const float* theta, const float* X, const float* omega, const float* coef, float* out, int S,
                               int C, int n, int D, int R, int N, int x_shared, void* ws, size_t ws_bytes,
                               vargp_stream_t stream) {
  VARGP_REQUIRE(theta && X && omega && coef && out && ws, "rff_paths: null pointer");
  VARGP_REQUIRE(S > 0 && C > 0 && n > 0 && D > 0 && R > 0 && N > 0, "rff_paths: bad dims");
  VARGP_REQUIRE(x_shared == 0 || x_shared == 1, "rff_paths: x_shared = %d (0 or 1)", x_shared);
  VARGP_REQUIRE((int64_t)S * C <= 65535, "rff_paths: S C = %lld (at most 65535)", (long long)S * C);
  VARGP_REQUIRE((int64_t)C * N <= (1 << 22), "rff_paths: C N = %lld (at most 2^22)", (long long)C * N);
  VARGP_REQUIRE((int64_t)n * D < (1LL << 31) && (int64_t)R * D < (1LL << 31) && (int64_t)2 * R * N < (1LL << 31) &&
                    (int64_t)n * N < (1LL << 31),
                "rff_paths: n D, R D, 2 R N and n N must be below 2^31");
  VARGP_REQUIRE(ws_bytes >= vargp_rff_paths_workspace_bytes(S, D, R), "rff_paths: workspace too small");
  hipStream_t st = as_stream(stream);
  float* om = reinterpret_cast<float*>(ws);
  float* gs = om + round_up((int64_t)S * R * D, 64);
  ProfScope whole("rff_paths", st);
  hipLaunchKernelGGL(rff_prep_kernel, dim3(cdiv((int64_t)S * R * D, 256)), dim3(256), 0, st, theta, omega, om, gs, S, D, R);
  RffArgs a{};
  a.X = X; a.om = om; a.gs = gs; a.coef = coef; a.out = out;
  a.C = C; a.n = n; a.D = D; a.R = R; a.N = N;
  a.shared = x_shared; a.Cc = x_shared ? C : 1; a.cols = a.Cc * N;
  const int nb = x_shared ? S : S * C;
  const dim3 blk(256);
  // the narrowest tile that holds all columns, so that no feature is computed twice; 256-wide tiles beyond that
  if (a.cols <= 64) hipLaunchKernelGGL((rff_paths_kernel<1>), dim3(cdiv(n, kRfBM), 1, nb), blk, 0, st, a);
  else if (a.cols <= 128) hipLaunchKernelGGL((rff_paths_kernel<2>), dim3(cdiv(n, kRfBM), 1, nb), blk, 0, st, a);
  else hipLaunchKernelGGL((rff_paths_kernel<4>), dim3(cdiv(n, kRfBM), cdiv(a.cols, 256), nb), blk, 0, st, a);
  return check_launch("rff_paths");
}

// How the backward is cut: WN (the width of a D tile), the D tiles, and the pieces of R -- enough of them for about 512
// workgroups, a function of the sizes alone, so that the summation order is too.
struct RffBwdPlan {
  int wn, dtiles, KS, steps;
  int64_t E;                           // elements of gX
  size_t part_floats;                  // the partial sums (none when S KS = 1)
};

static RffBwdPlan rff_bwd_plan(int S, int C, int n, int D, int R, int x_shared) {
  RffBwdPlan p{};
  p.wn = D <= 64 ? 1 : D <= 128 ? 2 : 4;
  p.dtiles = cdiv(D, 64 * p.wn);
  const int64_t wgs = (int64_t)cdiv(n, kRfBM) * p.dtiles * (x_shared ? S : (int64_t)S * C);
  const int nsteps = cdiv(R, kRfBR);
  const int want = (int)std::min<int64_t>(nsteps, std::max<int64_t>(1, (512 + wgs - 1) / wgs));
  p.steps = cdiv(nsteps, want);
  p.KS = cdiv(nsteps, p.steps);
  p.E = (int64_t)(x_shared ? 1 : C) * n * D;
  p.part_floats = (int64_t)S * p.KS > 1 ? (size_t)round_up((int64_t)S * p.KS * p.E, 64) : 0;
  return p;
}

extern "C" size_t vargp_rff_paths_bwd_workspace_bytes(int S, int C, int n, int D, int R, int x_shared) {
  if (S <= 0 || C <= 0 || n <= 0 || D <= 0 || R <= 0) return 0;
  return (rff_ws_floats(S, D, R) + rff_bwd_plan(S, C, n, D, R, x_shared).part_floats) * sizeof(float) + 256;
}

extern "C" int vargp_rff_paths_bwd(const float* theta, const float* X, const float* omega, const float* coef, const float* gout,
                                   float* gX, int S, int C, int n, int D, int R, int N, int x_shared, void* ws, size_t ws_bytes,
                                   vargp_stream_t stream) {
  VARGP_REQUIRE(theta && X && omega && coef && gout && gX && ws, "rff_paths_bwd: null pointer");
  VARGP_REQUIRE(S > 0 && C > 0 && n > 0 && D > 0 && R > 0 && N > 0, "rff_paths_bwd: bad dims");
  VARGP_REQUIRE(x_shared == 0 || x_shared == 1, "rff_paths_bwd: x_shared = %d (0 or 1)", x_shared);
  VARGP_REQUIRE((int64_t)S * C <= 65535, "rff_paths_bwd: S C = %lld (at most 65535)", (long long)S * C);
  VARGP_REQUIRE((int64_t)C * N <= (1 << 22), "rff_paths_bwd: C N = %lld (at most 2^22)", (long long)C * N);
  VARGP_REQUIRE((int64_t)n * D < (1LL << 31) && (int64_t)R * D < (1LL << 31) && (int64_t)2 * R * N < (1LL << 31) &&
                    (int64_t)n * N < (1LL << 31),
                "rff_paths_bwd: n D, R D, 2 R N and n N must be below 2^31");
  const RffBwdPlan p = rff_bwd_plan(S, C, n, D, R, x_shared);
  VARGP_REQUIRE(p.E < (1LL << 31), "rff_paths_bwd: gX has %lld elements (below 2^31)", (long long)p.E);
  VARGP_REQUIRE((int64_t)p.dtiles * p.KS <= 65535, "rff_paths_bwd: %d tiles of D x %d pieces of R (at most 65535)", p.dtiles,
                p.KS);
  VARGP_REQUIRE(ws_bytes >= vargp_rff_paths_bwd_workspace_bytes(S, C, n, D, R, x_shared), "rff_paths_bwd: workspace too small");
  hipStream_t st = as_stream(stream);
  float* om = reinterpret_cast<float*>(ws);
  float* gs = om + round_up((int64_t)S * R * D, 64);
  float* part = gs + round_up(S, 64);
  const int P = S * p.KS;
  ProfScope whole("rff_paths_bwd", st);
  hipLaunchKernelGGL(rff_prep_kernel, dim3(cdiv((int64_t)S * R * D, 256)), dim3(256), 0, st, theta, omega, om, gs, S, D, R);
  RffBwdArgs a{};
  a.X = X; a.om = om; a.gs = gs; a.coef = coef; a.gout = gout; a.dst = P > 1 ? part : gX;
  a.C = C; a.n = n; a.D = D; a.R = R; a.N = N;
  a.shared = x_shared; a.Cc = x_shared ? C : 1; a.cols = a.Cc * N;
  a.KS = p.KS; a.steps = p.steps;
  const dim3 grid(cdiv(n, kRfBM), p.dtiles * p.KS, x_shared ? S : S * C), blk(256);
  if (p.wn == 1) hipLaunchKernelGGL((rff_paths_bwd_kernel<1>), grid, blk, 0, st, a);
  else if (p.wn == 2) hipLaunchKernelGGL((rff_paths_bwd_kernel<2>), grid, blk, 0, st, a);
  else hipLaunchKernelGGL((rff_paths_bwd_kernel<4>), grid, blk, 0, st, a);
  if (P > 1) hipLaunchKernelGGL(rff_bwd_reduce_kernel, dim3(cdiv(p.E, 256)), dim3(256), 0, st, part, gX, P, p.E);
  return check_launch("rff_paths_bwd");
}
