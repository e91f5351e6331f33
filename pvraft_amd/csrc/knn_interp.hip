// K17: fused cross-set kNN + inverse-distance interpolation (absent in the
// reference, whose evaluation is subset-only): for every query point find
// its k nearest SUPPORT points and blend their values,
//
//   d2_i = |q - s_i|^2 (from coordinate differences)
//   w_i  = 1 / (d2_i + eps), normalised over the k_eff = min(k, N) neighbours
//   out  = sum_i w_i * values[idx_i]
//
// This carries the flow predicted on the sampled cloud to every point of
// the full-resolution scan.  The (M, N) distance matrix never exists.
//
// Geometry: one query per lane, block = 256 queries, grid (ceil(M/256), B).
// Support points are staged through an LDS tile of KI_TILE points shared
// by the whole workgroup, stored as three coordinate planes (x[], y[],
// z[]); in the sweep every lane reads the SAME address, one ds_read_b128
// broadcast (conflict-free) per plane bringing in KI_U = 4 candidates whose
// squares and sums run as packed fp32 ops.  Each lane keeps its running
// k-best (d2, idx) list sorted in CAP statically-indexed registers; the
// four candidates are tested together against the current worst slot, and
// only a hit enters the unrolled compare/shift insertion (see common.h for
// what one dynamic slot index costs).  CAP is a template parameter in
// {3, 8, 16}: k <= 3 (the default serving case) pays for 3 slots, not 16.
//
// Measured at B=1, N=8192, M=131072, C=3, k=3 (profiles/README.md): an
// (x, y, z, pad) float4 tile read one candidate at a time 0.384 ms ->
// coordinate planes 0.353 ms -> next group's LDS reads issued ahead of the
// current group's arithmetic 0.294 ms.
//
// Chip fill: M >= N in the use case (M ~ 100k -> 512 workgroups).  Below
// M = 256 CUs x 256 queries = 65536 the grid has fewer workgroups than
// the chip has CUs; that regime is not a target.
//
// Safety: slots start at (INF, -1) and a candidate enters only through
// d2 < worst, which is false for NaN and +INF distances, so non-finite
// coordinates can only leave slots empty.  The epilogue gives an empty
// slot weight 0 and never dereferences it.  Tile padding rows hold +INF
// coordinates and are rejected by the same comparison.
#include <hip/hip_runtime.h>
#include "common.h"

#define KI_THREADS 256
#define KI_TILE 1024  // support points per LDS tile (3 planes, 12 KB)
#define KI_U 4        // candidates per worst-slot test

typedef float ki_v4f __attribute__((ext_vector_type(4)));
static_assert(KI_U == 4 && KI_TILE % KI_U == 0, "one ki_v4f per candidate group");

int knn_interp_tile_pts() { return KI_TILE; }

template <int CAP>
DEV_INLINE void ki_insert(float (&bd)[CAP], int (&bi)[CAP], float d, int id) {
  // sorted ascending; strict < keeps the earlier (smaller) index on ties.
  // Walks from the worst slot down so bd[s - 1] is read before it moves.
#pragma unroll
  for (int s = CAP - 1; s > 0; --s) {
    if (d < bd[s - 1]) {
      bd[s] = bd[s - 1];
      bi[s] = bi[s - 1];
    } else if (d < bd[s]) {
      bd[s] = d;
      bi[s] = id;
    }
  }
  if (d < bd[0]) {
    bd[0] = d;
    bi[0] = id;
  }
}

template <int CAP>
__global__ __launch_bounds__(KI_THREADS) void knn_interp_kernel(
    const float *__restrict__ sup,   // (B, N, 3)
    const float *__restrict__ val,   // (B, N, C)
    const float *__restrict__ qry,   // (B, M, 3)
    float *__restrict__ out,         // (B, M, C)
    int *__restrict__ out_idx,       // (B, M, keff)
    float *__restrict__ out_w,       // (B, M, keff)
    int N, int M, int C, int keff, float eps) {
  __shared__ ki_v4f s_x[KI_TILE / KI_U], s_y[KI_TILE / KI_U],
      s_z[KI_TILE / KI_U];
  float *const sx = reinterpret_cast<float *>(s_x);
  float *const sy = reinterpret_cast<float *>(s_y);
  float *const sz = reinterpret_cast<float *>(s_z);

  const int b = blockIdx.y;
  const float *cloud = sup + (long)b * N * 3;
  const int q = blockIdx.x * KI_THREADS + threadIdx.x;
  // out-of-range lanes shadow the last query: they keep the barriers
  // uniform and write nothing
  const long qq = (long)b * M + min(q, M - 1);
  const float qx = qry[qq * 3 + 0];
  const float qy = qry[qq * 3 + 1];
  const float qz = qry[qq * 3 + 2];

  float bd[CAP];
  int bi[CAP];
#pragma unroll
  for (int s = 0; s < CAP; ++s) {
    bd[s] = INFINITY;
    bi[s] = -1;
  }

  for (int t0 = 0; t0 < N; t0 += KI_TILE) {
    const int tn = min(KI_TILE, N - t0);
    const int tpad = (tn + KI_U - 1) / KI_U * KI_U;  // <= KI_TILE
    __syncthreads();
    for (int i = threadIdx.x; i < tpad; i += KI_THREADS) {
      float px = INFINITY, py = INFINITY, pz = INFINITY;
      if (i < tn) {
        const float *src = cloud + (long)(t0 + i) * 3;
        px = src[0];
        py = src[1];
        pz = src[2];
      }
      sx[i] = px;
      sy[i] = py;
      sz[i] = pz;
    }
    __syncthreads();

    // the grid gives each SIMD only ~2 waves at M ~ 100k, too few to hide
    // the LDS round trip: the next group's reads are issued before the
    // current group's arithmetic and insertion branches
    const int ng = tpad / KI_U;
    ki_v4f nx = s_x[0], ny = s_y[0], nz = s_z[0];
    for (int g = 0; g < ng; ++g) {
      const int j = g * KI_U;
      // four candidates per coordinate vector: the differences and squares
      // map onto packed fp32 VALU ops with no repacking moves
      const ki_v4f dx = nx - qx;
      const ki_v4f dy = ny - qy;
      const ki_v4f dz = nz - qz;
      const int gn = min(g + 1, ng - 1);
      nx = s_x[gn];
      ny = s_y[gn];
      nz = s_z[gn];
      const ki_v4f dv = dx * dx + dy * dy + dz * dz;
      const float d[KI_U] = {dv.x, dv.y, dv.z, dv.w};
      // fminf drops NaN operands, so a NaN distance cannot open the gate
      // for its group-mates' sake nor be inserted itself
      const float dmin = fminf(fminf(d[0], d[1]), fminf(d[2], d[3]));
      if (dmin < bd[CAP - 1]) {
#pragma unroll
        for (int u = 0; u < KI_U; ++u)
          if (d[u] < bd[CAP - 1]) ki_insert<CAP>(bd, bi, d[u], t0 + j + u);
      }
    }
  }

  if (q >= M) return;

  // ---- epilogue: weights over the first keff slots, blend, store
  float w[CAP];
  float wsum = 0.f;
#pragma unroll
  for (int s = 0; s < CAP; ++s) {
    const bool live = s < keff && bi[s] >= 0;
    w[s] = live ? 1.f / (bd[s] + eps) : 0.f;
    wsum += w[s];
  }
  const float inv = wsum > 0.f ? 1.f / wsum : 0.f;
  int *idst = out_idx + qq * keff;
  float *wdst = out_w + qq * keff;
#pragma unroll
  for (int s = 0; s < CAP; ++s) {
    w[s] *= inv;
    if (s < keff) {
      idst[s] = bi[s];
      wdst[s] = w[s];
    }
  }
  const float *vb = val + (long)b * N * C;
  float *odst = out + qq * C;
  for (int c = 0; c < C; ++c) {
    float acc = 0.f;
#pragma unroll
    for (int s = 0; s < CAP; ++s)
      if (s < keff && bi[s] >= 0) acc += w[s] * vb[(long)bi[s] * C + c];
    odst[c] = acc;
  }
}

void launch_knn_interp(const float *sup, const float *val, const float *qry,
                       float *out, int *out_idx, float *out_w, int B, int N,
                       int M, int C, int keff, float eps, hipStream_t stream) {
  dim3 grid((M + KI_THREADS - 1) / KI_THREADS, B);
  dim3 block(KI_THREADS);
  if (keff <= 3)
    hipLaunchKernelGGL(knn_interp_kernel<3>, grid, block, 0, stream, sup, val,
                       qry, out, out_idx, out_w, N, M, C, keff, eps);
  else if (keff <= 8)
    hipLaunchKernelGGL(knn_interp_kernel<8>, grid, block, 0, stream, sup, val,
                       qry, out, out_idx, out_w, N, M, C, keff, eps);
  else
    hipLaunchKernelGGL(knn_interp_kernel<16>, grid, block, 0, stream, sup, val,
                       qry, out, out_idx, out_w, N, M, C, keff, eps);
}
