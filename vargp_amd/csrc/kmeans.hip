// Lloyd's two steps for G independent sets of K centres over ONE data matrix X [N][D] (the model's layout z [C][M][D]: one set
// per output).  Data-dependent initialisation of the inducing points (vargp_amd/init.py) -- nothing of this is in the reference.
//
// assign:  label[g][n] = argmin_k |x_n - z_gk|^2 (the smallest index on a tie), dist2[g][n] = that distance, clamped at 0.
//   One workgroup owns a tile of BT = 64 WT points and one set, walks the K centres in tiles of BT, keeps a running
//   (minimum, index) per point in registers and stores the two N-vectors only: the N x K distance matrix is never in memory.
//   D > kRbfDirectD: the inner products x . z on v_mfma_f32_32x32x2_f32, slabs of kKmBK values of d staged in LDS as
//   [d][BT + 1] (pred_cov.hip's layout).  The CENTRES are the A operand (rows) and the POINTS the B operand (columns), so that
//   with the C/D map  col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)  a lane's 16 accumulator registers are 16
//   centres of ONE point: the minimum over centres is in-lane compares, one exchange between the half-waves and one merge in LDS
//   of the two waves that share the point columns.  Compared is |z|^2 - 2 x.z; |x|^2 enters the reported distance only.
//   D <= kRbfDirectD: sum_d (x_d - z_d)^2 on the VALU, as every gram entry does: exactly 0 for coincident points.
//   Tile: four waves as 2 x 2, each 32 WT centres x 32 WT points.  WT = 1 when N G <= kKmSmallNG (a grid of 128-point tiles would
//   leave CUs idle); both tiles give bitwise the same result, since an MFMA entry is one d-ordered fmaf chain whatever the tile.
//   Every staging load is guarded: any N, K, D >= 1.
//
// update:  Z[g][k] = mean of the points labelled k in set g, count[g][k] = their number; a centre without points is not written.
//   One workgroup per (slab of 1024 values of d, k, g).  It walks label[g][:] in index order, compacts the indices of its own
//   points into a list in LDS (ballots + a prefix over the waves: a stable placement) and adds those rows in ascending index order,
//   lanes along d, into fp64 accumulators.  No atomics of any kind, no N x K histogram: the order of every sum is fixed by the
//   data alone, so two calls are bitwise equal.  (A one-hot MFMA product over N would multiply 94 GFLOP of zeros per iteration at
//   the Permuted-MNIST size to move 188 MB; the gather moves the 188 MB and re-reads the labels, 240 KB per set, from L2.)
#include "common.h"

namespace vargp {

typedef float km_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kKmBK = 32;
constexpr int64_t kKmSmallNG = 32768;     // N G <= this: 64-point tiles (fewer than 256 workgroups of 128 points otherwise)
constexpr int kKmChunk = 1024;            // labels scanned per pass of the update (4 per thread)
constexpr int kKmList = 4096;             // capacity of the index list in LDS
constexpr int kKmDSlab = 1024;            // values of d per workgroup of the update (4 per thread)

struct KmeansWs {
  float *nx, *nz;       // |x_n|^2 [N], |z_gk|^2 [G K] (inner-product form only)
  size_t bytes;
};

static KmeansWs kmeans_carve(void* ws, int G, int K, int N, int D) {
  KmeansWs o{};
  float* p = reinterpret_cast<float*>(ws);
  auto take = [&](int64_t n) { float* q = p; p += round_up(n, 64); return q; };
  const bool direct = D <= kRbfDirectD;
  o.nx = take(direct ? 0 : (int64_t)N);
  o.nz = take(direct ? 0 : (int64_t)G * K);
  o.bytes = (size_t)((char*)p - (char*)ws);
  return o;
}

// squared norms of the rows of X (rows [0, N)) and of Z (rows [N, N + GK)): one wave per row, lanes along d
__global__ __launch_bounds__(256) void kmeans_norm_kernel(const float* __restrict__ X, const float* __restrict__ Z, float* nx, float* nz,
                                                          int64_t N, int64_t GK, int D) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N + GK) return;
  const float* src = row < N ? X + row * D : Z + (row - N) * D;
  float s = 0.f;
  for (int d = threadIdx.x & 63; d < D; d += 64) s = fmaf(src[d], src[d], s);
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) (row < N ? nx[row] : nz[row - N]) = s;
}

struct KmAssignArgs {
  const float *X, *Z, *nx, *nz;
  int32_t* label;
  float* dist2;
  int K, N, D;
};

// (v, i) <- the smaller of (v, i) and (ov, oi); equal values: the smaller index
__device__ __forceinline__ void km_take(float& v, int& i, float ov, int oi) {
  if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
}

template <int WT, bool DIRECT>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const KmAssignArgs a) {
  constexpr int BT = 64 * WT, LD = BT + 1, BK = kKmBK;
  // [2][BK][LD]: the slabs of the centres and of the points.  DIRECT: the raw rows of both, [2][BT][D | 1].  Afterwards the
  // merge area, [2][BT] values and [2][BT] indices
  constexpr int kSlabs = 2 * BK * LD, kRows = 2 * BT * (kRbfDirectD | 1);
  __shared__ float lds[DIRECT && kRows > kSlabs ? kRows : kSlabs];
  static_assert(4 * BT <= kSlabs, "merge area");
  float* As = lds;
  float* Bs = lds + BK * LD;

  const int K = a.K, N = a.N, D = a.D;
  const int col0 = blockIdx.x * BT;             // first point of the tile
  const int64_t g = blockIdx.y;
  const float* __restrict__ Zg = a.Z + g * K * D;
  const float* __restrict__ X = a.X;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 32 * WT, wc = (wave & 1) * 32 * WT;     // the wave's corner: centres (rows), points (columns)
  const int l31 = lane & 31, h = lane >> 5;

  float best[WT];
  int bidx[WT];
#pragma unroll
  for (int j = 0; j < WT; ++j) { best[j] = INFINITY; bidx[j] = 0; }

  if constexpr (DIRECT) {
    const int Dl = D | 1;
    float* Zi = lds;
    float* Xj = lds + BT * Dl;
    for (int e = tid; e < BT * D; e += 256) {
      const int r = e / D, d = e - r * D;
      Xj[r * Dl + d] = col0 + r < N ? X[(int64_t)(col0 + r) * D + d] : 0.f;
    }
    for (int k0 = 0; k0 < K; k0 += BT) {
      if (k0) __syncthreads();
      for (int e = tid; e < BT * D; e += 256) {
        const int r = e / D, d = e - r * D;
        Zi[r * Dl + d] = k0 + r < K ? Zg[(int64_t)(k0 + r) * D + d] : 0.f;
      }
      __syncthreads();
      // rows in ascending order per lane: a strict < keeps the smallest index
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rl = wr + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
          const int row = k0 + rl;
          const float* zi = Zi + rl * Dl;
#pragma unroll
          for (int j = 0; j < WT; ++j) {
            const float* xj = Xj + (wc + 32 * j + l31) * Dl;
            float d2 = 0.f;
            for (int d = 0; d < D; ++d) { const float v = xj[d] - zi[d]; d2 = fmaf(v, v, d2); }
            if (row < K && d2 < best[j]) { best[j] = d2; bidx[j] = row; }
          }
        }
    }
  } else {
    for (int k0 = 0; k0 < K; k0 += BT) {
      km_f32x16 acc[WT][WT];
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
      for (int d0 = 0; d0 < D; d0 += BK) {
#pragma unroll
        for (int it = 0; it < BT * BK / 256; ++it) {
          const int e = tid + 256 * it, r = e / BK, k = e % BK;
          const bool kok = d0 + k < D;
          As[k * LD + r] = (kok && k0 + r < K) ? Zg[(int64_t)(k0 + r) * D + d0 + k] : 0.f;
          Bs[k * LD + r] = (kok && col0 + r < N) ? X[(int64_t)(col0 + r) * D + d0 + k] : 0.f;
        }
        __syncthreads();
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
        __syncthreads();
      }
      // |z|^2 - 2 x.z of this tile's centres against the running minimum (rows ascending per lane: strict <)
      const float* nz = a.nz + g * K;
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = k0 + wr + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
          const bool ok = row < K;
          const float nr = ok ? nz[row] : 0.f;
#pragma unroll
          for (int j = 0; j < WT; ++j) {
            const float v = fmaf(-2.f, acc[i][j][r], nr);
            if (ok && v < best[j]) { best[j] = v; bidx[j] = row; }
          }
        }
    }
  }

  // the other half-wave holds the other rows of the same points
#pragma unroll
  for (int j = 0; j < WT; ++j) {
    const float ov = __shfl_xor(best[j], 32, 64);
    const int oi = __shfl_xor(bidx[j], 32, 64);
    km_take(best[j], bidx[j], ov, oi);
  }
  // and so does the wave with the same point columns (wave ^ 2)
  __syncthreads();
  float* mv = lds;
  float* mi = lds + 2 * BT;            // the indices, as bit patterns
  if (h == 0) {
#pragma unroll
    for (int j = 0; j < WT; ++j) {
      mv[(wave >> 1) * BT + wc + 32 * j + l31] = best[j];
      mi[(wave >> 1) * BT + wc + 32 * j + l31] = __int_as_float(bidx[j]);
    }
  }
  __syncthreads();
  if (tid < BT && col0 + tid < N) {
    float v = mv[tid];
    int i = __float_as_int(mi[tid]);
    km_take(v, i, mv[BT + tid], __float_as_int(mi[BT + tid]));
    const int64_t o = g * N + col0 + tid;
    a.label[o] = i;
    a.dist2[o] = DIRECT ? v : fmaxf(a.nx[col0 + tid] + v, 0.f);
  }
}

struct KmUpdateArgs {
  const float* X;
  const int32_t* label;
  float* Z;
  int32_t* count;
  int K, N, D;
};

__global__ __launch_bounds__(256) void kmeans_update_kernel(const KmUpdateArgs a) {
  __shared__ int list[kKmList];
  __shared__ int wcnt[16];          // [pass q of the chunk][wave]
  const int N = a.N, D = a.D;
  const int d0 = blockIdx.x * kKmDSlab, k = blockIdx.y;
  const int64_t g = blockIdx.z;
  const int32_t* __restrict__ lab = a.label + g * N;
  const float* __restrict__ X = a.X;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  int fill = 0, total = 0;
  // add rows list[0 .. fill) in order, four loads in flight per accumulator
  auto flush = [&]() {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int d = d0 + tid + 256 * q;
      if (d < D) {
        int i = 0;
        for (; i + 4 <= fill; i += 4) {
          const float v0 = X[(int64_t)list[i] * D + d], v1 = X[(int64_t)list[i + 1] * D + d];
          const float v2 = X[(int64_t)list[i + 2] * D + d], v3 = X[(int64_t)list[i + 3] * D + d];
          acc[q] += (double)v0; acc[q] += (double)v1; acc[q] += (double)v2; acc[q] += (double)v3;
        }
        for (; i < fill; ++i) acc[q] += (double)X[(int64_t)list[i] * D + d];
      }
    }
  };

  for (int n0 = 0; n0 < N; n0 += kKmChunk) {
    // sub-chunk q holds the points n0 + 256 q + tid: (q, wave, lane) ascending is index order
    unsigned long long bal[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = n0 + 256 * q + tid;
      bal[q] = __ballot(n < N && lab[n] == k);
      if (lane == 0) wcnt[4 * q + wave] = __popcll(bal[q]);
    }
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if ((bal[q] >> lane) & 1ull) {
        int pos = fill + before + __popcll(bal[q] & ((1ull << lane) - 1ull));
#pragma unroll
        for (int w = 0; w < 4; ++w) pos += w < wave ? wcnt[4 * q + w] : 0;
        list[pos] = n0 + 256 * q + tid;
      }
#pragma unroll
      for (int w = 0; w < 4; ++w) { before += wcnt[4 * q + w]; }
    }
    all = before;
    fill += all;
    total += all;
    __syncthreads();
    if (fill > kKmList - kKmChunk) {       // the next chunk might not fit
      flush();
      fill = 0;
      __syncthreads();
    }
  }
  flush();

  if (blockIdx.x == 0 && tid == 0) a.count[g * a.K + k] = total;
  if (total > 0) {
    float* z = a.Z + (g * a.K + k) * D;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int d = d0 + tid + 256 * q;
      if (d < D) z[d] = (float)(acc[q] / (double)total);
    }
  }
}

}  // namespace vargp

using namespace vargp;

extern "C" size_t vargp_kmeans_workspace_bytes(int G, int K, int N, int D) {
  if (G <= 0 || K <= 0 || N <= 0 || D <= 0) return 0;
  return kmeans_carve(nullptr, G, K, N, D).bytes + 256;
}

extern "C" int vargp_kmeans_assign(const float* X, const float* Z, int32_t* label, float* dist2, int G, int K, int N, int D,
                                   void* ws, size_t ws_bytes, vargp_stream_t stream) {
  VARGP_REQUIRE(X && Z && label && dist2 && ws, "kmeans_assign: null pointer");
  VARGP_REQUIRE(G > 0 && K > 0 && N > 0 && D > 0, "kmeans_assign: bad dims");
  VARGP_REQUIRE(G <= 65535, "kmeans_assign: G = %d (at most 65535)", G);
  VARGP_REQUIRE((int64_t)N + (int64_t)G * K < (1ll << 31), "kmeans_assign: N + G K = %lld rows (below 2^31)",
                (long long)N + (long long)G * K);
  VARGP_REQUIRE(ws_bytes >= vargp_kmeans_workspace_bytes(G, K, N, D), "kmeans_assign: workspace too small");
  const KmeansWs o = kmeans_carve(ws, G, K, N, D);
  hipStream_t st = as_stream(stream);
  const bool direct = D <= kRbfDirectD, small = (int64_t)N * G <= kKmSmallNG;
  ProfScope whole("kmeans_assign", st);
  if (!direct) {
    const int64_t rows = (int64_t)N + (int64_t)G * K;
    hipLaunchKernelGGL(kmeans_norm_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, X, Z, o.nx, o.nz, (int64_t)N, (int64_t)G * K, D);
  }
  KmAssignArgs a{};
  a.X = X; a.Z = Z; a.nx = o.nx; a.nz = o.nz; a.label = label; a.dist2 = dist2; a.K = K; a.N = N; a.D = D;
  const dim3 grid(cdiv(N, small ? 64 : 128), G), blk(256);
  if (small) {
    if (direct) hipLaunchKernelGGL((kmeans_assign_kernel<1, true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((kmeans_assign_kernel<1, false>), grid, blk, 0, st, a);
  } else {
    if (direct) hipLaunchKernelGGL((kmeans_assign_kernel<2, true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((kmeans_assign_kernel<2, false>), grid, blk, 0, st, a);
  }
  return check_launch("kmeans_assign");
}

extern "C" int vargp_kmeans_update(const float* X, const int32_t* label, float* Z, int32_t* count, int G, int K, int N, int D,
                                   void* ws, size_t ws_bytes, vargp_stream_t stream) {
  VARGP_REQUIRE(X && label && Z && count && ws, "kmeans_update: null pointer");
  VARGP_REQUIRE(G > 0 && K > 0 && N > 0 && D > 0, "kmeans_update: bad dims");
  VARGP_REQUIRE(G <= 65535 && K <= 65535, "kmeans_update: G = %d, K = %d (at most 65535 each)", G, K);
  VARGP_REQUIRE(ws_bytes >= vargp_kmeans_workspace_bytes(G, K, N, D), "kmeans_update: workspace too small");
  KmUpdateArgs a{};
  a.X = X; a.label = label; a.Z = Z; a.count = count; a.K = K; a.N = N; a.D = D;
  hipStream_t st = as_stream(stream);
  ProfScope whole("kmeans_update", st);
  hipLaunchKernelGGL(kmeans_update_kernel, dim3(cdiv(D, kKmDSlab), K, G), dim3(256), 0, st, a);
  return check_launch("kmeans_update");
}
