// Full predictive covariance of one block of test points, for every (hyper-sample, class):
//
//   Sigma[s, c] = K_theta_s(X, X) - P[s,c]^T P[s,c] + W[s,c]^T W[s,c]        (B x B, fp32)
//
// with P = Lz^-1 Kzx and W = (Lz^-1 chol(S + eps I))^T P, the operands of vargp_predictive_diag_fwd, whose `var` is the
// diagonal of this matrix.  Composed from the existing entries (the gram matrix, then two accumulating GEMMs) the S C B^2
// result passes through memory three times; here a workgroup keeps one tile of it in the MFMA accumulators from the first
// product to the only store:
//   1. the inner products x_i . (w o x_j) over D (f32 MFMA; operands from the RBF pre-pass, rbf_prep_norm_launch) -- or, for
//      D <= kRbfDirectD, the direct distance sum_d w_d (x_id - x_jd)^2 on the VALU, as the gram entries do;
//   2. the kernel epilogue (common.h: EpiRbf / EpiMatern) in place, exactly gamma^2 on the diagonal;
//   3. the same accumulators then take the product over the stacked 2 Mt dimension, [-P; W]^T [P; W];
//   4. one store -- two for a tile below the diagonal, which also writes its mirror image.
// Only tiles that touch the lower triangle are computed, and only entries (i, j), j <= i, of a diagonal tile are stored (to
// both places), so the result is bitwise symmetric.
//
// Tile: BT x BT, BT = 64 WT, four waves as 2 x 2, each wave 32 WT x 32 WT (WT^2 accumulators of v_mfma_f32_32x32x2_f32;
// fragment maps as in gemm.hip).  Slabs of kBK values of the reduction index are staged in LDS as [k][BT + 1]: lanes read
// consecutive floats, and the transposing writes of the X slabs spread over the banks.  Any B, D and Mt: every staging load
// is guarded and out-of-range elements enter as zeros.
#include "common.h"

namespace vargp {

typedef float pc_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kPcBK = 32;
constexpr int kPcSmallB = 256;      // B <= this: 64 x 64 tiles (more workgroups, less padding), above: 128 x 128

struct PredCovWs {
  float *w, *g2, *na, *xs;
  int64_t Dp;
  size_t bytes;
};

static PredCovWs pred_cov_carve(void* ws, int S, int B, int D) {
  PredCovWs o{};
  o.Dp = round_up(D, 4);
  float* p = reinterpret_cast<float*>(ws);
  auto take = [&](int64_t n) { float* q = p; p += round_up(n, 64); return q; };
  o.w = take((int64_t)S * o.Dp);
  o.g2 = take(S);
  o.na = take((int64_t)S * B);
  o.xs = take(D <= kRbfDirectD ? 0 : (int64_t)S * B * D);     // x o w, one copy per hyper-sample
  o.bytes = (size_t)((char*)p - (char*)ws);
  return o;
}

struct PredCovArgs {
  const float *X, *P, *W;      // [B][D]; [S C][Mt][B] twice
  const float *w, *g2, *na, *xs;
  float* out;                  // [S C][B][B]
  int C, B, D, Mt, nt;         // nt = tiles per side
  int64_t Dp;
};

template <int WT, bool DIRECT, class EPI>
__global__ __launch_bounds__(256) void pred_cov_kernel(const PredCovArgs a) {
  constexpr int BT = 64 * WT, LD = BT + 1, BK = kPcBK;
  // [2][BK][LD]: the slabs of the row and of the column operand.  DIRECT: first the raw rows of both point sets,
  // [2][BT][D | 1], with 1/sigma^2 behind them
  constexpr int kSlabs = 2 * BK * LD, kRows = 2 * BT * (kRbfDirectD | 1);
  __shared__ float lds[(DIRECT && kRows > kSlabs ? kRows : kSlabs) + (DIRECT ? kRbfDirectD : 0)];
  float* As = lds;
  float* Bs = lds + BK * LD;

  // lower-triangular tile (ti, tj), tj <= ti, from the linear index
  const int t = blockIdx.x;
  int ti = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  while (ti * (ti + 1) / 2 > t) --ti;
  const int tj = t - ti * (ti + 1) / 2;
  const int row0 = ti * BT, col0 = tj * BT;
  const int64_t b = blockIdx.y;
  const int s = (int)(b / a.C);
  const int B = a.B, D = a.D, Mt = a.Mt;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 32 * WT, wc = (wave & 1) * 32 * WT;     // the wave's corner inside the tile
  const int l31 = lane & 31, h = lane >> 5;
  const float g2 = a.g2[s];

  pc_f32x16 acc[WT][WT];
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int j = 0; j < WT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // one BK-slab of MFMAs from the staged operands
  auto slab = [&]() {
#pragma unroll
    for (int k = 0; k < BK; k += 2) {
      float af[WT], bf[WT];
#pragma unroll
      for (int i = 0; i < WT; ++i) af[i] = As[(k + h) * LD + wr + 32 * i + l31];
#pragma unroll
      for (int j = 0; j < WT; ++j) bf[j] = Bs[(k + h) * LD + wc + 32 * j + l31];
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  };

  if constexpr (DIRECT) {
    // d2 = sum_d w_d (x_id - x_jd)^2 entry by entry: no cancellation, exactly 0 for coincident points
    const int Dl = D | 1;
    float* Xi = lds;
    float* Xj = lds + BT * Dl;
    float* wl = lds + (kRows > kSlabs ? kRows : kSlabs);
    for (int e = tid; e < BT * D; e += 256) {
      const int r = e / D, d = e - r * D;
      Xi[r * Dl + d] = row0 + r < B ? a.X[(int64_t)(row0 + r) * D + d] : 0.f;
      Xj[r * Dl + d] = col0 + r < B ? a.X[(int64_t)(col0 + r) * D + d] : 0.f;
    }
    if (tid < D) wl[tid] = a.w[s * a.Dp + tid];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        const float* xj = Xj + (wc + 32 * j + l31) * Dl;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float* xi = Xi + (wr + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h) * Dl;
          float d2 = 0.f;
          for (int d = 0; d < D; ++d) { const float v = xi[d] - xj[d]; d2 = fmaf(wl[d] * v, v, d2); }
          acc[i][j][r] = d2;
        }
      }
  } else {
    // x_i . (w o x_j): rows from the raw points, columns from the pre-scaled copy of this hyper-sample
    const float* __restrict__ xr = a.X;
    const float* __restrict__ xs = a.xs + (int64_t)s * B * D;
    for (int k0 = 0; k0 < D; k0 += BK) {
#pragma unroll
      for (int e = tid; e < BT * BK; e += 256) {
        const int r = e / BK, k = e % BK;
        const bool kok = k0 + k < D;
        As[k * LD + r] = (kok && row0 + r < B) ? xr[(int64_t)(row0 + r) * D + k0 + k] : 0.f;
        Bs[k * LD + r] = (kok && col0 + r < B) ? xs[(int64_t)(col0 + r) * D + k0 + k] : 0.f;
      }
      __syncthreads();
      slab();
      __syncthreads();
    }
  }

  // the kernel epilogue, in place: the accumulators now hold K(x_i, x_j)
  const float* na = a.na + (int64_t)s * B;
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int j = 0; j < WT; ++j) {
      const int col = col0 + wc + 32 * j + l31;
      const float nc = (!DIRECT && col < B) ? na[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + wr + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
        float d2 = acc[i][j][r];
        if constexpr (!DIRECT) d2 = (row < B ? na[row] : 0.f) + nc - 2.f * d2;
        acc[i][j][r] = row == col ? EPI::diag(g2) : EPI::off(g2, d2);
      }
    }
  if constexpr (DIRECT) __syncthreads();        // the point rows in LDS make way for the P / W slabs

  // + [-P; W]^T [P; W] over the stacked 2 Mt rows (row k of the stack: P_k for k < Mt, W_(k - Mt) after)
  const float* __restrict__ Pb = a.P + b * Mt * B;
  const float* __restrict__ Wb = a.W + b * Mt * B;
  for (int k0 = 0; k0 < 2 * Mt; k0 += BK) {
#pragma unroll
    for (int e = tid; e < BT * BK; e += 256) {
      const int k = e / BT, r = e % BT;
      const int kk = k0 + k;
      const bool isp = kk < Mt;
      const float* src = (isp ? Pb + (int64_t)kk * B : Wb + (int64_t)(kk - Mt) * B);
      const bool kok = kk < 2 * Mt;
      const float va = (kok && row0 + r < B) ? src[row0 + r] : 0.f;
      const float vb = (kok && col0 + r < B) ? src[col0 + r] : 0.f;
      As[k * LD + r] = isp ? -va : va;
      Bs[k * LD + r] = vb;
    }
    __syncthreads();
    slab();
    __syncthreads();
  }

  // the only store: entry (row, col), col <= row, and its mirror image
  float* out = a.out + b * B * B;
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int j = 0; j < WT; ++j) {
      const int col = col0 + wc + 32 * j + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + wr + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row < B && col <= row) {
          const float v = acc[i][j][r];
          out[(int64_t)row * B + col] = v;
          if (col != row) out[(int64_t)col * B + row] = v;
        }
      }
    }
}

template <class EPI>
static void pred_cov_launch(const PredCovArgs& a, int nb, hipStream_t st) {
  const bool direct = a.D <= kRbfDirectD, small = a.B <= kPcSmallB;
  PredCovArgs q = a;
  q.nt = cdiv(a.B, small ? 64 : 128);
  const dim3 grid(q.nt * (q.nt + 1) / 2, nb), blk(256);
  if (small) {
    if (direct) hipLaunchKernelGGL((pred_cov_kernel<1, true, EPI>), grid, blk, 0, st, q);
    else hipLaunchKernelGGL((pred_cov_kernel<1, false, EPI>), grid, blk, 0, st, q);
  } else {
    if (direct) hipLaunchKernelGGL((pred_cov_kernel<2, true, EPI>), grid, blk, 0, st, q);
    else hipLaunchKernelGGL((pred_cov_kernel<2, false, EPI>), grid, blk, 0, st, q);
  }
}

}  // namespace vargp

using namespace vargp;

extern "C" size_t vargp_predictive_cov_workspace_bytes(int S, int B, int D) {
  return pred_cov_carve(nullptr, S, B, D).bytes + 256;
}

extern "C" int vargp_predictive_cov(const float* theta, const float* X, const float* P, const float* W, float* Sigma, int S,
                                    int C, int Mt, int B, int D, int nu2, void* ws, size_t ws_bytes, vargp_stream_t stream) {
  VARGP_REQUIRE(theta && X && P && W && Sigma && ws, "predictive_cov: null pointer");
  VARGP_REQUIRE(S > 0 && C > 0 && Mt > 0 && B > 0 && D > 0, "predictive_cov: bad dims");
  VARGP_REQUIRE(nu2 == 0 || nu2 == 1 || nu2 == 3 || nu2 == 5, "predictive_cov: nu2 = %d (0 = RBF, 1, 3 or 5)", nu2);
  VARGP_REQUIRE((int64_t)S * C <= 65535, "predictive_cov: S C = %lld (at most 65535)", (long long)S * C);
  VARGP_REQUIRE(ws_bytes >= vargp_predictive_cov_workspace_bytes(S, B, D), "predictive_cov: workspace too small");
  const PredCovWs o = pred_cov_carve(ws, S, B, D);
  hipStream_t st = as_stream(stream);
  // 1/sigma^2, gamma^2, the weighted squared norms of the points and (inner-product form) their scaled copies
  int rc = rbf_prep_norm_launch(theta, X, B, nullptr, 0, o.w, o.g2, o.na, nullptr, S, D, o.Dp, st, nullptr,
                                D <= kRbfDirectD ? (float*)nullptr : o.xs);
  if (rc) return rc;
  PredCovArgs a{};
  a.X = X; a.P = P; a.W = W; a.w = o.w; a.g2 = o.g2; a.na = o.na; a.xs = o.xs; a.out = Sigma;
  a.C = C; a.B = B; a.D = D; a.Mt = Mt; a.Dp = o.Dp;
  ProfScope whole("predictive_cov", st);
  if (nu2 == 0) pred_cov_launch<EpiRbf>(a, S * C, st);
  else if (nu2 == 1) pred_cov_launch<EpiMatern<1>>(a, S * C, st);
  else if (nu2 == 3) pred_cov_launch<EpiMatern<3>>(a, S * C, st);
  else pred_cov_launch<EpiMatern<5>>(a, S * C, st);
  return check_launch("predictive_cov");
}
