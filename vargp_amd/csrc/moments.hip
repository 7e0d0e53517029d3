// Weighted moments of the cross-kernel over a whole data set, for G independent outputs over ONE data matrix X [N][D] and ONE
// hyper vector -- what the closed-form optimal q(u) of a Gaussian likelihood needs of the data (collapsed.py; nothing of this is
// in the reference).  With k_n = k_theta(Z_g, x_n), an Mt-vector:
//   Phi_g = sum_n w_gn k_n k_n^T,   c_g = sum_n w_gn y_gn k_n,   sums_g = (sum_n w_gn, sum_n w_gn y_gn^2).
// K(Z, X) never reaches global memory.  A workgroup owns one (output g, lower-triangle 64 x 64 tile (ti, tj) of Phi, chunk of N).
// It walks its chunk 64 columns at a time: the two 64-row panels of K behind the tile (one on the diagonal) are built in LDS as
// [column][row], then 32 v_mfma_f32_32x32x2_f32 per wave add w K_i K_j^T over the 64 columns to the tile's accumulators (four
// waves as 2 x 2, fragment maps as in gemm.hip), which stay in registers for the whole chunk.  The tiles of column tj = 0 also
// form their panel's share of c, and tile (0, 0) the two sums.
//   D <= kRbfDirectD: the scaled distance directly, d2 = sum_d w_d (z_d - x_d)^2 in ascending d (the arithmetic of gram.hip's
//   direct form); the Z panels are staged once per workgroup, the 64 points of X once per step.
//   D  > kRbfDirectD: d2 = |a|^2 + |b|^2 - 2 a.b with a = z / lengthscale, b = x / lengthscale: slabs of 32 values of d of both are
//   staged in LDS, a.b on the same MFMA, the squared norms from the staged slabs themselves -- no pre-pass and no buffer over N.
// Columns behind the end of the chunk are MASKED: their K entries and weights are written as zeros whatever X holds there (the
// loads themselves are guarded).  A zero weight multiplies a finite K entry: it adds exactly nothing.
// No atomics.  A second launch adds the chunks' partial tiles in ascending chunk order in fp64, rounds once to fp32 and writes
// entry (i, j), j <= i, to both triangles: Phi is bitwise symmetric and two calls on the same input are bitwise equal.
// The chunking depends on the shapes alone (mom_plan): at most kMoMaxChunks chunks of at least kMoMinChunk columns, as many as
// give the launch about kMoTargetWg workgroups.
#include "common.h"

namespace vargp {

typedef float mo_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMoT = 64;               // tile side of Phi = columns of X per step
constexpr int kMoLD = kMoT + 1;
constexpr int kMoBK = 32;              // values of d per slab (D > kRbfDirectD)
constexpr int kMoDl = kRbfDirectD | 1; // row stride of the staged points (direct form)
constexpr int kMoTargetWg = 1024;
constexpr int kMoMinChunk = 256;
constexpr int kMoMaxChunks = 1024;

struct MomPlan {
  int nt, ntri, nch;         // tiles per side, lower-triangle tiles, chunks
  int64_t len;               // columns per chunk (a multiple of kMoT)
  float *pphi, *pc, *ps;     // partials [G][nch][ntri][64 * 64], [G][nch][nt * 64], [G][nch][2]
  size_t bytes;
};

static MomPlan mom_plan(void* ws, int G, int Mt, int N) {
  MomPlan o{};
  o.nt = cdiv(Mt, kMoT);
  o.ntri = o.nt * (o.nt + 1) / 2;
  int64_t want = cdiv(kMoTargetWg, (int64_t)G * o.ntri);
  const int64_t most = cdiv(N, kMoMinChunk);
  want = want < most ? want : most;
  want = want < 1 ? 1 : (want > kMoMaxChunks ? kMoMaxChunks : want);
  o.len = round_up(cdiv(N, want), kMoT);
  o.nch = cdiv(N, o.len);
  float* p = reinterpret_cast<float*>(ws);
  auto take = [&](int64_t n) { float* q = p; p += round_up(n, 64); return q; };
  o.pphi = take((int64_t)G * o.nch * o.ntri * kMoT * kMoT);
  o.pc = take((int64_t)G * o.nch * o.nt * kMoT);
  o.ps = take((int64_t)G * o.nch * 2);
  o.bytes = (size_t)((char*)p - (char*)ws);
  return o;
}

struct MomArgs {
  const float *theta, *Z, *X, *w, *y;
  float *Phi, *c, *sums;
  MomPlan p;
  int G, Mt, N, D;
};

// lower-triangle tile (ti, tj), tj <= ti, from its linear index
__device__ __forceinline__ void mo_tile(int t, int& ti, int& tj) {
  ti = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  while (ti * (ti + 1) / 2 > t) --ti;
  tj = t - ti * (ti + 1) / 2;
}

// grid (ntri * nch, G): blockIdx.x = chunk * ntri + tile
template <class EPI, bool DIRECT>
__global__ __launch_bounds__(256) void moments_kernel(const MomArgs a) {
  constexpr int T = kMoT, LD = kMoLD, BK = kMoBK;
  __shared__ float Ks[2][T * LD];                                // the K panels of the tile's rows and columns: [n][m]
  __shared__ float stage[DIRECT ? 3 * T * kMoDl : 3 * BK * LD];  // DIRECT: Z_i, Z_j, X rows; else the slabs of a_i, a_j, b: [k][r]
  __shared__ float wl[kRbfDirectD];                              // DIRECT: exp(-2 theta_d)
  __shared__ float wn[T], wyn[T];                                // w_n and w_n y_n of the step's columns (0 behind the end)
  __shared__ float nrm[3][T];                                    // !DIRECT: |a_i|^2, |a_j|^2, |b|^2
  __shared__ float cred[4][T];

  const int Mt = a.Mt, D = a.D, ntri = a.p.ntri;
  const int chunk = blockIdx.x / ntri, t = blockIdx.x - chunk * ntri;
  int ti, tj;
  mo_tile(t, ti, tj);
  const bool two = ti != tj;
  const int i0 = ti * T, j0 = tj * T;
  const int64_t g = blockIdx.y;
  const int64_t cbeg = (int64_t)chunk * a.p.len;
  const int64_t cend = cbeg + a.p.len < a.N ? cbeg + a.p.len : a.N;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32, l31 = lane & 31, h = lane >> 5;
  const float g2 = expf(2.f * a.theta[D]);
  const float* __restrict__ Zg = a.Z + g * (int64_t)Mt * D;
  const float* __restrict__ X = a.X;
  const float* __restrict__ wg = a.w ? a.w + g * (int64_t)a.N : nullptr;
  const float* __restrict__ yg = a.y + g * (int64_t)a.N;
  const int Dl = D | 1;

  mo_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float cacc = 0.f, sw = 0.f, syy = 0.f;

  if constexpr (DIRECT) {
    for (int e = tid; e < T * D; e += 256) {
      const int r = e / D, d = e - r * D;
      stage[r * Dl + d] = i0 + r < Mt ? Zg[(int64_t)(i0 + r) * D + d] : 0.f;
      stage[T * kMoDl + r * Dl + d] = j0 + r < Mt ? Zg[(int64_t)(j0 + r) * D + d] : 0.f;
    }
    if (tid < D) wl[tid] = expf(-2.f * a.theta[tid]);
  }

  for (int64_t n0 = cbeg; n0 < cend; n0 += T) {
    if (tid < T) {
      const int64_t n = n0 + tid;
      float wv = 0.f, yv = 0.f;
      if (n < cend) { wv = wg ? wg[n] : 1.f; yv = yg[n]; }
      wn[tid] = wv;
      wyn[tid] = wv * yv;
      sw += wv;
      syy = fmaf(wv * yv, yv, syy);
    }
    if constexpr (DIRECT) {
      float* Xs = stage + 2 * T * kMoDl;
      for (int e = tid; e < T * D; e += 256) {
        const int r = e / D, d = e - r * D;
        Xs[r * Dl + d] = n0 + r < cend ? X[(n0 + r) * D + d] : 0.f;
      }
      __syncthreads();
      // lanes = rows of the panel, the wave's 16 columns in registers; the point of X is a broadcast read
      for (int p = 0; p < (two ? 2 : 1); ++p) {
        const float* zr = stage + p * T * kMoDl + lane * Dl;
        const float* xr = Xs + 16 * wave * Dl;
        float d2[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) d2[q] = 0.f;
        for (int d = 0; d < D; ++d) {
          const float zv = zr[d], wv = wl[d];
#pragma unroll
          for (int q = 0; q < 16; ++q) { const float v = zv - xr[q * Dl + d]; d2[q] = fmaf(wv * v, v, d2[q]); }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q)
          Ks[p][(16 * wave + q) * LD + lane] = n0 + 16 * wave + q < cend ? EPI::off(g2, d2[q]) : 0.f;
      }
    } else {
      float* Ai = stage;
      float* Aj = stage + BK * LD;
      float* Bs = stage + 2 * BK * LD;
      mo_f32x16 di, dj;
#pragma unroll
      for (int r = 0; r < 16; ++r) di[r] = dj[r] = 0.f;
      float nr = 0.f;
      const int k = tid & 31;
      for (int k0 = 0; k0 < D; k0 += BK) {
        const bool kok = k0 + k < D;
        const float sq = kok ? expf(-a.theta[k0 + k]) : 0.f;           // 1 / lengthscale
#pragma unroll
        for (int r = tid >> 5; r < T; r += 8) {
          Ai[k * LD + r] = (kok && i0 + r < Mt) ? sq * Zg[(int64_t)(i0 + r) * D + k0 + k] : 0.f;
          if (two) Aj[k * LD + r] = (kok && j0 + r < Mt) ? sq * Zg[(int64_t)(j0 + r) * D + k0 + k] : 0.f;
          Bs[k * LD + r] = (kok && n0 + r < cend) ? sq * X[(n0 + r) * D + k0 + k] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
          const float bf = Bs[(kk + h) * LD + wc + l31];
          di = __builtin_amdgcn_mfma_f32_32x32x2f32(Ai[(kk + h) * LD + wr + l31], bf, di, 0, 0, 0);
          if (two) dj = __builtin_amdgcn_mfma_f32_32x32x2f32(Aj[(kk + h) * LD + wr + l31], bf, dj, 0, 0, 0);
        }
        if (wave < 3 && (wave != 1 || two)) {
          const float* src = stage + wave * BK * LD + lane;
#pragma unroll
          for (int kk = 0; kk < BK; ++kk) { const float v = src[kk * LD]; nr = fmaf(v, v, nr); }
        }
        __syncthreads();
      }
      if (wave < 3) nrm[wave][lane] = nr;
      __syncthreads();
      // the wave's 32 x 32 block of each panel: rows wr.. of Z against the columns wc.. of X
      const int col = wc + l31;
      const bool cok = n0 + col < cend;
      const float nb = nrm[2][col];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wr + (r & 3) + 8 * (r >> 2) + 4 * h;
        Ks[0][col * LD + row] = cok ? EPI::off(g2, nrm[0][row] + nb - 2.f * di[r]) : 0.f;
        if (two) Ks[1][col * LD + row] = cok ? EPI::off(g2, nrm[1][row] + nb - 2.f * dj[r]) : 0.f;
      }
    }
    __syncthreads();

    // the symmetric rank update of the step: acc += (K_i o w) K_j^T over the 64 columns
    const float* Ki = Ks[0];
    const float* Kj = Ks[two ? 1 : 0];
#pragma unroll
    for (int kk = 0; kk < T; kk += 2) {
      const int n = kk + h;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ki[n * LD + wr + l31] * wn[n], Kj[n * LD + wc + l31], acc, 0, 0, 0);
    }
    if (tj == 0) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) s = fmaf(Ki[(16 * wave + q) * LD + lane], wyn[16 * wave + q], s);
      cacc += s;
    }
    __syncthreads();
  }

  const int64_t part = g * a.p.nch + chunk;
  float* out = a.p.pphi + (part * ntri + t) * (T * T);
#pragma unroll
  for (int r = 0; r < 16; ++r) out[(wr + (r & 3) + 8 * (r >> 2) + 4 * h) * T + wc + l31] = acc[r];
  if (tj == 0) {
    cred[wave][lane] = cacc;
    __syncthreads();
    if (tid < T) a.p.pc[part * a.p.nt * T + i0 + tid] = (cred[0][tid] + cred[1][tid]) + (cred[2][tid] + cred[3][tid]);
  }
  if (t == 0 && wave == 0) {
    sw = wave_sum(sw);
    syy = wave_sum(syy);
    if (lane == 0) { a.p.ps[part * 2] = sw; a.p.ps[part * 2 + 1] = syy; }
  }
}

// The chunks' partials in ascending chunk order, in fp64.  grid (ntri * 16 + cdiv(Mt, 256) + 1, G): 256 entries of a tile | 256
// entries of c | the two sums
__global__ __launch_bounds__(256) void moments_reduce_kernel(const MomArgs a) {
  constexpr int T = kMoT;
  const int Mt = a.Mt, ntri = a.p.ntri, nch = a.p.nch;
  const int64_t g = blockIdx.y;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b < ntri * 16) {
    const int t = b >> 4, e = (b & 15) * 256 + tid;
    int ti, tj;
    mo_tile(t, ti, tj);
    const int i = ti * T + e / T, j = tj * T + e % T;
    if (i >= Mt || j > i) return;
    const float* p = a.p.pphi + ((g * nch) * ntri + t) * (int64_t)(T * T) + e;
    double s = 0.0;
    for (int q = 0; q < nch; ++q) s += (double)p[(int64_t)q * ntri * (T * T)];
    float* Phi = a.Phi + g * (int64_t)Mt * Mt;
    Phi[(int64_t)i * Mt + j] = (float)s;
    Phi[(int64_t)j * Mt + i] = (float)s;
  } else if (b < ntri * 16 + (Mt + 255) / 256) {
    const int i = (b - ntri * 16) * 256 + tid;
    if (i >= Mt) return;
    const float* p = a.p.pc + (g * nch) * (int64_t)(a.p.nt * T) + i;
    double s = 0.0;
    for (int q = 0; q < nch; ++q) s += (double)p[(int64_t)q * a.p.nt * T];
    a.c[g * Mt + i] = (float)s;
  } else if (tid < 2) {
    const float* p = a.p.ps + (g * nch) * 2 + tid;
    double s = 0.0;
    for (int q = 0; q < nch; ++q) s += (double)p[2 * q];
    a.sums[g * 2 + tid] = (float)s;
  }
}

template <class EPI>
static void moments_launch(const MomArgs& a, hipStream_t st) {
  const dim3 grid(a.p.ntri * a.p.nch, a.G), blk(256);
  if (a.D <= kRbfDirectD) hipLaunchKernelGGL((moments_kernel<EPI, true>), grid, blk, 0, st, a);
  else hipLaunchKernelGGL((moments_kernel<EPI, false>), grid, blk, 0, st, a);
}

}  // namespace vargp

using namespace vargp;

extern "C" int vargp_gram_moments_chunks(int G, int Mt, int N, int D) {
  if (G <= 0 || Mt <= 0 || N <= 0 || D <= 0) return 0;
  return mom_plan(nullptr, G, Mt, N).nch;
}

extern "C" size_t vargp_gram_moments_workspace_bytes(int G, int Mt, int N, int D) {
  if (G <= 0 || Mt <= 0 || N <= 0 || D <= 0) return 0;
  return mom_plan(nullptr, G, Mt, N).bytes + 256;
}

extern "C" int vargp_gram_moments(const float* theta, const float* Z, const float* X, const float* w, const float* y, float* Phi,
                                  float* c, float* sums, int G, int Mt, int N, int D, int nu2, void* ws, size_t ws_bytes,
                                  vargp_stream_t stream) {
  VARGP_REQUIRE(theta && Z && X && y && Phi && c && sums && ws, "gram_moments: null pointer");
  VARGP_REQUIRE(G > 0 && Mt > 0 && N > 0 && D > 0, "gram_moments: bad dims");
  VARGP_REQUIRE(nu2 == 0 || nu2 == 1 || nu2 == 3 || nu2 == 5, "gram_moments: nu2 = %d (0: RBF; 1, 3, 5: Matern)", nu2);
  VARGP_REQUIRE(G <= 65535, "gram_moments: G = %d (at most 65535)", G);
  VARGP_REQUIRE(ws_bytes >= vargp_gram_moments_workspace_bytes(G, Mt, N, D), "gram_moments: workspace too small");
  MomArgs a{};
  a.theta = theta; a.Z = Z; a.X = X; a.w = w; a.y = y; a.Phi = Phi; a.c = c; a.sums = sums;
  a.p = mom_plan(ws, G, Mt, N);
  a.G = G; a.Mt = Mt; a.N = N; a.D = D;
  VARGP_REQUIRE((int64_t)a.p.ntri * a.p.nch < (1ll << 31), "gram_moments: Mt = %d needs too many tiles", Mt);
  hipStream_t st = as_stream(stream);
  ProfScope whole("gram_moments", st);
  switch (nu2) {
    case 0: moments_launch<EpiRbf>(a, st); break;
    case 1: moments_launch<EpiMatern<1>>(a, st); break;
    case 3: moments_launch<EpiMatern<3>>(a, st); break;
    default: moments_launch<EpiMatern<5>>(a, st); break;
  }
  hipLaunchKernelGGL(moments_reduce_kernel, dim3(a.p.ntri * 16 + cdiv(Mt, 256) + 1, G), dim3(256), 0, st, a);
  return check_launch("gram_moments");
}
