// Matern / ARD kernel matrices, nu = 1/2, 3/2, 5/2, and their backward.  Everything that depends only on the scaled squared
// distance d2 is the RBF's (rbf.hip, gemm.hip): the pre-pass (1/sigma^2, gamma^2, weighted row norms, the pre-scaled shared
// y), the f32-MFMA distance GEMM -- here with the Matern epilogues of common.h --, the direct form for D <= kRbfDirectD, the
// W.Y / W^T.X products and the finalisation of gX, gY, gtheta.
//
//   K_ij = g2 k(d2_ij)            k as in common.h (matern_k), d2 clamped at 0
//   W_ij = gK_ij * (-2 g2 dk/dd2) (matern_w; the RBF's -2 dk/dd2 is K itself, hence its W = gK o K)
//   gX, gY, gtheta[:, :D] from W exactly as in rbf.hip;  gtheta[:, D] = 2 sum gK o K
// W needs r = sqrt(d2), which K does not give back, so the backward RECOMPUTES the distance product (epilogue EpiDist2: the
// clamped d2, 0 on the diagonal of a self product) instead of carrying d2 over from the forward call: workspaces stay
// call-local, as everywhere in this library (the Python layer pools one scratch buffer per stream).
#include "common.h"

namespace vargp {

struct MaternWs {
  float *w, *g2, *na, *nb, *part, *ys, *Wm, *r, *c, *P, *Q;
  int64_t Dp;
  size_t bytes;
};

// the forward's buffers are the leading part of the backward's (which runs the same distance product first)
static MaternWs matern_carve(void* ws, int S, int C, int M, int N, int D, bool backward) {
  MaternWs o{};
  o.Dp = round_up(D, 4);
  float* p = reinterpret_cast<float*>(ws);
  auto take = [&](int64_t n) { float* q = p; p += round_up(n, 64); return q; };
  o.w = take((int64_t)S * o.Dp);
  o.g2 = take(S);
  o.na = take((int64_t)S * C * M);
  o.nb = take((int64_t)S * C * N);
  o.part = take(D <= kRbfDirectD ? 0 : (int64_t)2 * S * C * M * N);   // split-K partial products (at most 2 splits)
  o.ys = take(D <= kRbfDirectD ? 0 : (int64_t)S * N * D);   // y o w of a shared y (one copy per hyper-sample)
  if (backward) {
    o.Wm = take((int64_t)S * C * M * N);
    o.r = take((int64_t)S * C * M);
    o.c = take((int64_t)S * C * N);
    o.P = take((int64_t)S * C * M * D);
    o.Q = take((int64_t)S * C * N * D);
  }
  o.bytes = (size_t)((char*)p - (char*)ws);
  return o;
}

__global__ void matern_prep_kernel(const float* __restrict__ theta, float* __restrict__ w, float* __restrict__ g2, int D,
                                   int64_t Dp) {
  const int s = blockIdx.x;
  const float* th = theta + (int64_t)s * (D + 1);
  for (int d = threadIdx.x; d < Dp; d += blockDim.x) w[s * Dp + d] = d < D ? expf(-2.f * th[d]) : 0.f;
  if (threadIdx.x == 0) g2[s] = expf(2.f * th[D]);
}

// D <= kRbfDirectD: d2 = sum_d w_d (x_d - y_d)^2 directly (no cancellation; exactly 0 for coincident points, so the
// diagonal of a self product needs no special case).  One thread per entry.
template <class EPI>
__global__ __launch_bounds__(256) void matern_direct_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                            const float* __restrict__ w, const float* __restrict__ g2,
                                                            float* __restrict__ K, int C, int M, int N, int D, int64_t Dp,
                                                            int y_shared, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int n = e % N, m = (e / N) % M, c = (e / ((int64_t)N * M)) % C;
  const int s = e / ((int64_t)N * M * C);
  const float* xr = X + ((int64_t)c * M + m) * D;
  const float* yr = Y ? (y_shared ? Y + (int64_t)n * D : Y + ((int64_t)c * N + n) * D) : X + ((int64_t)c * M + n) * D;
  const float* ws = w + s * Dp;
  float d2 = 0.f;
  for (int d = 0; d < D; ++d) { const float t = xr[d] - yr[d]; d2 = fmaf(ws[d] * t, t, d2); }
  K[e] = EPI::off(g2[s], d2);
}

// split-K: the epilogue over the summed partial inner products (rbf_combine_kernel's job with the epilogue as a parameter)
template <class EPI>
__global__ __launch_bounds__(256) void matern_combine_kernel(const float* __restrict__ part, int nsplit, int64_t sSplit,
                                                             const float* __restrict__ na, const float* __restrict__ nbv,
                                                             const float* __restrict__ g2, float* __restrict__ K,
                                                             int64_t rows_per_s, int N, int64_t nb_stride_s,
                                                             int64_t nb_stride_c, int Mb, int same_xy, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int col = e % N;
  const int64_t row = e / N;                 // s * rows_per_s + (c * Mb + m)
  const int64_t s = row / rows_per_s, rc = row % rows_per_s;
  const int64_t c = rc / Mb;
  const int m = rc % Mb;
  float ab = 0.f;
  for (int k = 0; k < nsplit; ++k) ab += part[k * sSplit + e];
  const float d2 = na[row] + nbv[s * nb_stride_s + c * nb_stride_c + col] - 2.f * ab;
  K[e] = (same_xy && m == col) ? EPI::diag(g2[s]) : EPI::off(g2[s], d2);
}

// W = gK o (-2 g2 dk/dd2) from the recomputed d2, with its row sums r, column sums c, and 2 sum gK o K into gtheta[s, D], in
// one pass.  Grid and accumulation as rbf_w_kernel: (ceil(N/256), ceil(Mb/WROWS), nb), a thread owns one column of a strip of
// WROWS rows; r and c by float atomics (pre-zeroed by the caller), the total with one atomic per block.
constexpr int WROWS = 8;
template <int NU2>
__global__ __launch_bounds__(256) void matern_w_kernel(const float* __restrict__ K, const float* __restrict__ gK,
                                                       const float* d2m, const float* __restrict__ g2, float* W,
                                                       float* __restrict__ r, float* __restrict__ c,
                                                       float* __restrict__ gtheta, int Mb, int N, int Cb, int D) {
  __shared__ float red[4];
  const int col = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const int row0 = blockIdx.y * WROWS;
  const int64_t b = blockIdx.z;
  const bool cok = col < N;
  const int64_t base = b * Mb * N;
  const float g = g2[b / Cb];
  float csum = 0.f, ksum = 0.f;
  const int rend = min(WROWS, Mb - row0);
  for (int rr = 0; rr < rend; ++rr) {
    const int64_t off = base + (int64_t)(row0 + rr) * N + col;
    float v = 0.f;
    if (cok) {
      const float gk = gK[off];
      v = gk * matern_w<NU2>(g, d2m[off]);
      W[off] = v;
      ksum = fmaf(gk, K[off], ksum);
    }
    csum += v;
    const float rs = wave_sum(v);
    if (lane == 0 && rs != 0.f) atomicAdd(&r[b * Mb + row0 + rr], rs);
  }
  if (cok) atomicAdd(&c[b * N + col], csum);
  const float tot = block_sum<256>(ksum, red);
  if (threadIdx.x == 0) atomicAdd(&gtheta[(b / Cb) * (D + 1) + D], 2.f * tot);
}

// Square case (Y = X), as rbf_w_self_kernel: Ws = W + W^T without its diagonal (K_ii = gamma^2 depends on neither x_i nor the
// lengthscales), r = its row sums, and 2 sum gK o K (diagonal included) into gtheta[s, D].  d2 is symmetric, so
// Ws_ij = (gK_ij + gK_ji) w(d2_ij).  d2m and Ws may be the same buffer (a thread reads the entry it then writes); likewise
// d2m and W of matern_w_kernel.
constexpr int kSelfRows = 16;
template <int NU2>
__global__ __launch_bounds__(256) void matern_w_self_kernel(const float* __restrict__ K, const float* __restrict__ gK,
                                                            const float* d2m, const float* __restrict__ g2, float* Ws,
                                                            float* __restrict__ r, float* __restrict__ gtheta, int M, int Cb,
                                                            int D, int nchunk) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63;
  const int64_t b = blockIdx.x / nchunk;
  const int i0 = ((int)blockIdx.x % nchunk) * kSelfRows, i1 = min(M, i0 + kSelfRows);
  const float* Kb = K + b * M * M;
  const float* gKb = gK + b * M * M;
  const float* db = d2m + b * M * M;
  const float g = g2[b / Cb];
  float ksum = 0.f;
  for (int i = i0 + (threadIdx.x >> 6); i < i1; i += 4) {
    float acc = 0.f;
    for (int j = lane; j < M; j += 64) {
      const float gij = gKb[(int64_t)i * M + j];
      const float gs = gij + gKb[(int64_t)j * M + i];
      const float v = i == j ? 0.f : gs * matern_w<NU2>(g, db[(int64_t)i * M + j]);
      Ws[b * M * M + (int64_t)i * M + j] = v;
      acc += v;
      ksum = fmaf(gij, Kb[(int64_t)i * M + j], ksum);
    }
    acc = wave_sum(acc);
    if (lane == 0) r[b * M + i] = acc;
  }
  const float t = block_sum<256>(ksum, red);
  if (threadIdx.x == 0) atomicAdd(&gtheta[(b / Cb) * (D + 1) + D], 2.f * t);
}

// the direct form for a caller that has run the pre-pass itself (the block ELBO program, elbo_tn.hip): out [S, C, M, N], dense
int matern_direct_launch(const float* X, const float* Y, const float* w, const float* g2, float* out, int S, int C, int M, int N,
                         int D, int64_t Dp, int y_shared, int epi, hipStream_t st) {
  const int64_t total = (int64_t)S * C * M * N;
  const dim3 grid(cdiv(total, 256)), blk(256);
  if (epi == kEpiMatern12) hipLaunchKernelGGL(matern_direct_kernel<EpiMatern<1>>, grid, blk, 0, st, X, Y, w, g2, out, C, M, N, D, Dp, y_shared, total);
  else if (epi == kEpiMatern32) hipLaunchKernelGGL(matern_direct_kernel<EpiMatern<3>>, grid, blk, 0, st, X, Y, w, g2, out, C, M, N, D, Dp, y_shared, total);
  else if (epi == kEpiMatern52) hipLaunchKernelGGL(matern_direct_kernel<EpiMatern<5>>, grid, blk, 0, st, X, Y, w, g2, out, C, M, N, D, Dp, y_shared, total);
  else if (epi == kEpiDist2) hipLaunchKernelGGL(matern_direct_kernel<EpiDist2>, grid, blk, 0, st, X, Y, w, g2, out, C, M, N, D, Dp, y_shared, total);
  else VARGP_REQUIRE(false, "matern_direct_launch: epilogue %d", epi);
  return check_launch("matern_gram(direct)");
}

// The distance product of one call with the epilogue `epi` (a DistEpi other than kEpiPlain / kEpiRbf) into out[S, C, M, N]:
// vargp_rbf_gram_fwd's sequence -- pre-pass, then the direct kernel, the fused GEMM, or split-K partials + combine pass.
template <class EPI>
static int matern_dist(const float* theta, const float* X, const float* Y, float* out, int S, int C, int M, int N, int D,
                       int y_shared, const MaternWs& o, int epi, hipStream_t st) {
  const bool self = (Y == nullptr);
  if (D <= kRbfDirectD) {
    hipLaunchKernelGGL(matern_prep_kernel, dim3(S), dim3(256), 0, st, theta, o.w, o.g2, D, o.Dp);
    const int64_t total = (int64_t)S * C * M * N;
    hipLaunchKernelGGL(matern_direct_kernel<EPI>, dim3(cdiv(total, 256)), dim3(256), 0, st, X, Y, o.w, o.g2, out, C, M, N, D,
                       o.Dp, y_shared, total);
    return check_launch("matern_gram(direct)");
  }
  const int64_t xrows = (int64_t)C * M, yrows = y_shared ? N : (int64_t)C * N;
  const bool prescale = y_shared && !self;
  int rc = rbf_prep_norm_launch(theta, X, xrows, Y, self ? (int64_t)0 : yrows, o.w, o.g2, o.na, o.nb, S, D, o.Dp, st,
                                prescale ? o.ys : (float*)nullptr, (float*)nullptr);
  if (rc) return rc;
  // shared Y: the classes' inducing points are just more rows of one [C*M, D] x [D, N] product
  const int Cb = y_shared ? 1 : C, Mb = y_shared ? C * M : M;
  GemmParams p{};
  p.A = X; p.B = self ? X : Y; p.C = out; p.D = nullptr;
  p.M = Mb; p.N = N; p.K = D; p.lda = D; p.ldb = D; p.ldc = N; p.ldd = 0;
  p.nb1 = Cb; p.nb2 = 1;
  p.sA[0] = 0; p.sA[1] = (int64_t)Mb * D;
  p.sB[0] = 0; p.sB[1] = y_shared ? 0 : (int64_t)N * D;
  p.sC[0] = (int64_t)Cb * Mb * N; p.sC[1] = (int64_t)Mb * N;
  p.alpha = 1.f; p.beta = 0.f;
  p.kscale = o.w; p.ks_ld = o.Dp; p.g2 = o.g2;
  p.na = o.na; p.sNa[0] = xrows; p.sNa[1] = Mb;
  p.nbv = self ? o.na : o.nb; p.sNb[0] = self ? xrows : yrows; p.sNb[1] = (self || !y_shared) ? N : 0;
  p.same_xy = self ? 1 : 0;
  if (prescale) { p.B = o.ys; p.sB[0] = (int64_t)N * D; p.kscale = nullptr; }
  const int nsplit = rbf_splitk(Mb, N, D, S * Cb);
  ProfScope whole(self ? "matern_kuu" : "matern_kuf", st);
  if (nsplit > 1) {
    const int64_t total = (int64_t)S * Cb * Mb * N;
    p.splitk = nsplit;
    p.sSplit = total;
    p.C = o.part;
    rc = launch_gemm_epi(p, 0, 1, S * Cb, epi, st, self ? "matern_kuu_gemm" : "matern_kuf_gemm");
    if (rc) return rc;
    hipLaunchKernelGGL(matern_combine_kernel<EPI>, dim3(cdiv(total, 256)), dim3(256), 0, st, o.part, nsplit, p.sSplit, o.na,
                       self ? o.na : o.nb, o.g2, out, (int64_t)Cb * Mb, N, self ? xrows : yrows,
                       (self || !y_shared) ? (int64_t)N : 0, Mb, self ? 1 : 0, total);
  } else {
    rc = launch_gemm_epi(p, 0, 1, S * Cb, epi, st, self ? "matern_kuu_gemm" : "matern_kuf_gemm");
    if (rc) return rc;
  }
  return check_launch("matern_gram(gemm)");
}

template <int NU2>
static int matern_bwd(const float* theta, const float* X, const float* Y, const float* K, const float* gK, float* gX, float* gY,
                      float* gtheta, int S, int C, int M, int N, int D, int y_shared, int accumulate, const MaternWs& o,
                      hipStream_t st) {
  const bool self = (Y == nullptr);
  const int Cb = y_shared ? 1 : C, Mb = y_shared ? C * M : M;
  const int64_t xrows = (int64_t)C * M, yrows = y_shared ? N : (int64_t)C * N;
  const int nb = S * Cb;
  // d2 into Wm, then W over it in place (each thread reads the entry it writes)
  int rc = matern_dist<EpiDist2>(theta, X, Y, o.Wm, S, C, M, N, D, y_shared, o, kEpiDist2, st);
  if (rc) return rc;
  if (!accumulate) zero_async(gtheta, sizeof(float) * (size_t)S * (D + 1), st);
  if (self) {
    const int nchunk = cdiv(M, kSelfRows);
    hipLaunchKernelGGL(matern_w_self_kernel<NU2>, dim3(nb * nchunk), dim3(256), 0, st, K, gK, o.Wm, o.g2, o.Wm, o.r, gtheta, M,
                       Cb, D, nchunk);
  } else {
    zero_async(o.r, sizeof(float) * (size_t)(o.P - o.r), st);   // r and c are adjacent
    hipLaunchKernelGGL(matern_w_kernel<NU2>, dim3(cdiv(N, 256), cdiv(Mb, WROWS), nb), dim3(256), 0, st, K, gK, o.Wm, o.g2,
                       o.Wm, o.r, o.c, gtheta, Mb, N, Cb, D);
  }
  // from here on: rbf_gram_bwd_impl's tail.  P = W . Y   ([Mb, N] x [N, D]) per (s, class-batch)
  GemmParams p{};
  p.A = o.Wm; p.B = self ? X : Y; p.C = o.P;
  p.M = Mb; p.N = D; p.K = N; p.lda = N; p.ldb = D; p.ldc = D;
  p.nb1 = Cb; p.nb2 = 1;
  p.sA[0] = (int64_t)Cb * Mb * N; p.sA[1] = (int64_t)Mb * N;
  p.sB[0] = 0; p.sB[1] = y_shared ? 0 : (int64_t)N * D;
  p.sC[0] = (int64_t)Cb * Mb * D; p.sC[1] = (int64_t)Mb * D;
  p.alpha = 1.f;
  rc = launch_gemm(p, 0, 0, nb, false, st, self ? "matern_kuu_bwd_gemm" : "matern_kuf_bwd_gemm");
  if (rc) return rc;
  rc = rbf_final_launch(X, o.r, o.P, theta, gX, gtheta, xrows, D, o.Dp, S, self ? 1.f : 2.f, accumulate, st);
  if (rc) return rc;
  if (!self) {
    const float* Qp = nullptr;
    if (gY) {  // Q = W^T . X  ([N, Mb] x [Mb, D])
      GemmParams q{};
      q.A = o.Wm; q.B = X; q.C = o.Q;
      q.M = N; q.N = D; q.K = Mb; q.lda = N; q.ldb = D; q.ldc = D;
      q.nb1 = Cb; q.nb2 = 1;
      q.sA[0] = (int64_t)Cb * Mb * N; q.sA[1] = (int64_t)Mb * N;
      q.sB[0] = 0; q.sB[1] = (int64_t)Mb * D;
      q.sC[0] = (int64_t)Cb * N * D; q.sC[1] = (int64_t)N * D;
      q.alpha = 1.f;
      rc = launch_gemm(q, 1, 0, nb, false, st);
      if (rc) return rc;
      Qp = o.Q;
    }
    rc = rbf_final_launch(Y, o.c, Qp, theta, gY, gtheta, yrows, D, o.Dp, S, 0.f, accumulate, st);
    if (rc) return rc;
  }
  return check_launch("matern_gram_bwd");
}

}  // namespace vargp

using namespace vargp;

extern "C" size_t vargp_matern_workspace_bytes(int S, int C, int M, int N, int D, int backward) {
  return matern_carve(nullptr, S, C, M, N, D, backward != 0).bytes + 256;
}

extern "C" int vargp_matern_gram_fwd(const float* theta, const float* X, const float* Y, float* K, int S, int C, int M, int N,
                                     int D, int y_shared, int nu2, void* ws, size_t ws_bytes, vargp_stream_t stream) {
  VARGP_REQUIRE(theta && X && K && ws, "matern_gram_fwd: null pointer");
  VARGP_REQUIRE(S > 0 && C > 0 && M > 0 && D > 0, "matern_gram_fwd: bad dims");
  VARGP_REQUIRE(nu2 == 1 || nu2 == 3 || nu2 == 5, "matern_gram_fwd: nu2 = %d (1, 3 or 5)", nu2);
  if (!Y) { N = M; y_shared = 0; }
  VARGP_REQUIRE(N > 0, "matern_gram_fwd: bad N");
  VARGP_REQUIRE(ws_bytes >= vargp_matern_workspace_bytes(S, C, M, N, D, 0), "matern_gram_fwd: workspace too small");
  const MaternWs o = matern_carve(ws, S, C, M, N, D, false);
  hipStream_t st = as_stream(stream);
  if (nu2 == 1) return matern_dist<EpiMatern<1>>(theta, X, Y, K, S, C, M, N, D, y_shared, o, kEpiMatern12, st);
  if (nu2 == 3) return matern_dist<EpiMatern<3>>(theta, X, Y, K, S, C, M, N, D, y_shared, o, kEpiMatern32, st);
  return matern_dist<EpiMatern<5>>(theta, X, Y, K, S, C, M, N, D, y_shared, o, kEpiMatern52, st);
}

extern "C" int vargp_matern_gram_bwd(const float* theta, const float* X, const float* Y, const float* K, const float* gK,
                                     float* gX, float* gY, float* gtheta, int S, int C, int M, int N, int D, int y_shared,
                                     int nu2, int accumulate, void* ws, size_t ws_bytes, vargp_stream_t stream) {
  VARGP_REQUIRE(theta && X && K && gK && gtheta && ws, "matern_gram_bwd: null pointer");
  VARGP_REQUIRE(S > 0 && C > 0 && M > 0 && D > 0, "matern_gram_bwd: bad dims");
  VARGP_REQUIRE(nu2 == 1 || nu2 == 3 || nu2 == 5, "matern_gram_bwd: nu2 = %d (1, 3 or 5)", nu2);
  if (!Y) { N = M; y_shared = 0; gY = nullptr; }
  VARGP_REQUIRE(N > 0, "matern_gram_bwd: bad N");
  VARGP_REQUIRE(ws_bytes >= vargp_matern_workspace_bytes(S, C, M, N, D, 1), "matern_gram_bwd: workspace too small");
  const MaternWs o = matern_carve(ws, S, C, M, N, D, true);
  hipStream_t st = as_stream(stream);
  if (nu2 == 1) return matern_bwd<1>(theta, X, Y, K, gK, gX, gY, gtheta, S, C, M, N, D, y_shared, accumulate, o, st);
  if (nu2 == 3) return matern_bwd<3>(theta, X, Y, K, gK, gX, gY, gtheta, S, C, M, N, D, y_shared, accumulate, o, st);
  return matern_bwd<5>(theta, X, Y, K, gK, gX, gY, gtheta, S, C, M, N, D, y_shared, accumulate, o, st);
}
