// K18: fused Chamfer distance between T warped clouds and a target cloud
// (absent in the reference, which trains on ground-truth flow only).
//
//   w_t = pc1 + f_t                                  (never written to memory)
//   dir 0: for every w_t[b,i]  the nearest pc2[b,j]  -> (d2, idx) (T,B,N)
//   dir 1: for every pc2[b,j]  the nearest w_t[b,i]  -> (d2, idx) (T,B,M)
//   chamfer_t = sum(dir 0) / (B N) + sum(dir 1) / (B M)
//
// Forward geometry: one query per lane, block = 256 queries, grid
// (ceil(max(N, M) / 256), B, ndir * T); z selects flow and direction, so
// one launch covers everything (B=2, T=8, N=M=8192 -> 1024 workgroups on
// 256 CUs, where the per-cloud knn_interp grid would be 64).  The support
// cloud goes through an LDS tile of CH_TILE points stored as three
// coordinate planes; every lane reads the SAME address, one ds_read_b128
// broadcast per plane bringing in CH_U = 4 candidates (the knn_interp.hip
// sweep).  Each lane keeps a single running (best d2, best idx) pair: no
// k-best list, no insertion.
//
// Numerics: d2 from coordinate differences; ascending scan with strict <,
// so ties go to the lowest index; the running best starts at +INF, hence a
// NaN or +INF distance never wins (fminf drops NaN operands, so a NaN
// cannot open the group gate either).  A query with no finite candidate
// keeps idx -1, reports d2 = +INF and adds 0 to the sum.  Tile padding rows
// hold +INF coordinates and are rejected by the same comparison.
//
// Sums: each block folds its 256 lanes in a fixed order (wave butterfly,
// then the four wave sums in order) into one slot of a (T, ndir, B, blocks)
// scratch buffer; the caller folds that with one deterministic sum.
//
// Backward (deterministic, atomic-free): one lane per point i of pc1, grid
// (ceil(N / 256), B, T).  The dir-1 assignment nn2[t,b,:] is swept through
// LDS tiles of int4; a lane compares sixteen indices per step with its own i
// and loads pc2[j] only on a hit (hits average M / N per lane), accumulating
// in ascending j.  The dir-0 term is one gather.
#include <hip/hip_runtime.h>
#include "common.h"

#define CH_THREADS 256
#define CH_TILE 1024   // support points per LDS tile (3 planes, 12 KB)
#define CH_U 4         // candidates per gate test
#define CHB_TILE 2048  // nn2 indices per LDS tile in the backward (8 KB)
#define CHB_G 16       // indices per backward step (four int4 reads)

typedef float ch_v4f __attribute__((ext_vector_type(4)));
typedef int ch_v4i __attribute__((ext_vector_type(4)));
static_assert(CH_U == 4 && CH_TILE % CH_U == 0, "one ch_v4f per candidate group");
static_assert(CHB_G == 16 && CHB_TILE % CHB_G == 0, "four ch_v4i per index step");

int chamfer_tile_pts() { return CH_TILE; }

// fixed-order sum over the block's 256 lanes; valid in thread 0
DEV_INLINE float ch_block_sum(float v, float *s_part) {
  v = wave_sum(v);
  if (lane_id() == 0) s_part[wave_id()] = v;
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < CH_THREADS / WAVE; ++w) r += s_part[w];
  }
  return r;
}

__global__ __launch_bounds__(CH_THREADS) void chamfer_fwd_kernel(
    const float *__restrict__ pc1,   // (B, N, 3)
    const float *__restrict__ flow,  // (T, B, N, 3) or null (= zero flow)
    const float *__restrict__ pc2,   // (B, M, 3)
    float *__restrict__ d2_1,        // (T, B, N)
    int *__restrict__ idx_1,         // (T, B, N)
    float *__restrict__ d2_2,        // (T, B, M) (unused when ndir == 1)
    int *__restrict__ idx_2,         // (T, B, M)
    float *__restrict__ partial,     // (T, ndir, B, gridDim.x)
    int B, int N, int M, int ndir) {
  __shared__ ch_v4f s_x[CH_TILE / CH_U], s_y[CH_TILE / CH_U],
      s_z[CH_TILE / CH_U];
  __shared__ float s_part[CH_THREADS / WAVE];
  float *const sx = reinterpret_cast<float *>(s_x);
  float *const sy = reinterpret_cast<float *>(s_y);
  float *const sz = reinterpret_cast<float *>(s_z);

  const int b = blockIdx.y;
  const int t = blockIdx.z / ndir;
  const int dir = blockIdx.z - t * ndir;
  const int Q = dir == 0 ? N : M;  // queries
  const int S = dir == 0 ? M : N;  // support points
  // the grid is sized for the larger cloud: whole blocks past the end of
  // the smaller one leave before any barrier (their scratch slot stays 0)
  if ((long)blockIdx.x * CH_THREADS >= Q) return;

  const float *p1 = pc1 + (long)b * N * 3;
  const float *fl = flow ? flow + ((long)t * B + b) * N * 3 : nullptr;
  const float *p2 = pc2 + (long)b * M * 3;

  const int q = blockIdx.x * CH_THREADS + threadIdx.x;
  // out-of-range lanes shadow the last query: they keep the barriers
  // uniform and write nothing
  const long qc = min(q, Q - 1);
  float qx, qy, qz;
  if (dir == 0) {
    qx = p1[qc * 3 + 0];
    qy = p1[qc * 3 + 1];
    qz = p1[qc * 3 + 2];
    if (fl) {
      qx += fl[qc * 3 + 0];
      qy += fl[qc * 3 + 1];
      qz += fl[qc * 3 + 2];
    }
  } else {
    qx = p2[qc * 3 + 0];
    qy = p2[qc * 3 + 1];
    qz = p2[qc * 3 + 2];
  }

  float best = INFINITY;
  int bi = -1;

  for (int t0 = 0; t0 < S; t0 += CH_TILE) {
    const int tn = min(CH_TILE, S - t0);
    const int tpad = (tn + CH_U - 1) / CH_U * CH_U;  // <= CH_TILE
    __syncthreads();
    for (int i = threadIdx.x; i < tpad; i += CH_THREADS) {
      float px = INFINITY, py = INFINITY, pz = INFINITY;
      if (i < tn) {
        const long r = (long)(t0 + i) * 3;
        if (dir == 0) {
          px = p2[r + 0];
          py = p2[r + 1];
          pz = p2[r + 2];
        } else {
          px = p1[r + 0];
          py = p1[r + 1];
          pz = p1[r + 2];
          if (fl) {
            px += fl[r + 0];
            py += fl[r + 1];
            pz += fl[r + 2];
          }
        }
      }
      sx[i] = px;
      sy[i] = py;
      sz[i] = pz;
    }
    __syncthreads();

    // next group's LDS reads are issued ahead of the current group's
    // arithmetic (knn_interp.hip measured this at 17%)
    const int ng = tpad / CH_U;
    ch_v4f nx = s_x[0], ny = s_y[0], nz = s_z[0];
    for (int g = 0; g < ng; ++g) {
      const ch_v4f dx = nx - qx;
      const ch_v4f dy = ny - qy;
      const ch_v4f dz = nz - qz;
      const int gn = min(g + 1, ng - 1);
      nx = s_x[gn];
      ny = s_y[gn];
      nz = s_z[gn];
      const ch_v4f dv = dx * dx + dy * dy + dz * dz;
      const float dmin = fminf(fminf(dv.x, dv.y), fminf(dv.z, dv.w));
      if (dmin < best) {
        const int j = t0 + g * CH_U;
        // ascending, strict <: the lowest index among equals stays
        if (dv.x < best) { best = dv.x; bi = j + 0; }
        if (dv.y < best) { best = dv.y; bi = j + 1; }
        if (dv.z < best) { best = dv.z; bi = j + 2; }
        if (dv.w < best) { best = dv.w; bi = j + 3; }
      }
    }
  }

  const bool live = q < Q;
  if (live) {
    const long o = ((long)t * B + b) * Q + q;
    if (dir == 0) {
      d2_1[o] = best;
      idx_1[o] = bi;
    } else {
      d2_2[o] = best;
      idx_2[o] = bi;
    }
  }
  const float r = ch_block_sum(live && bi >= 0 ? best : 0.f, s_part);
  if (threadIdx.x == 0)
    partial[(((long)t * ndir + dir) * B + b) * gridDim.x + blockIdx.x] = r;
}

__global__ __launch_bounds__(CH_THREADS) void chamfer_bwd_kernel(
    const float *__restrict__ pc1,   // (B, N, 3)
    const float *__restrict__ flow,  // (T, B, N, 3)
    const float *__restrict__ pc2,   // (B, M, 3)
    const int *__restrict__ idx_1,   // (T, B, N)
    const int *__restrict__ idx_2,   // (T, B, M)
    const float *__restrict__ gout,  // (T)
    float *__restrict__ dflow,       // (T, B, N, 3)
    int B, int N, int M, float c1, float c2) {
  __shared__ ch_v4i s_i[CHB_TILE / 4];
  int *const si = reinterpret_cast<int *>(s_i);

  const int b = blockIdx.y;
  const int t = blockIdx.z;
  const int i = blockIdx.x * CH_THREADS + threadIdx.x;
  const bool live = i < N;
  // -2 matches neither an assignment nor the -1 of empty / padding slots
  const int me = live ? i : -2;
  const long row = ((long)t * B + b) * N + min(i, N - 1);
  const long prow = (long)b * N + min(i, N - 1);
  const float wx = pc1[prow * 3 + 0] + flow[row * 3 + 0];
  const float wy = pc1[prow * 3 + 1] + flow[row * 3 + 1];
  const float wz = pc1[prow * 3 + 2] + flow[row * 3 + 2];
  const float *p2 = pc2 + (long)b * M * 3;
  const int *nn2 = idx_2 + ((long)t * B + b) * M;

  float ax = 0.f, ay = 0.f, az = 0.f;
  for (int t0 = 0; t0 < M; t0 += CHB_TILE) {
    const int tn = min(CHB_TILE, M - t0);
    const int tpad = (tn + CHB_G - 1) / CHB_G * CHB_G;  // <= CHB_TILE
    __syncthreads();
    for (int j = threadIdx.x; j < tpad; j += CH_THREADS)
      si[j] = j < tn ? nn2[t0 + j] : -1;
    __syncthreads();
    // 16 indices per step, and the next step's four reads issued ahead of
    // this step's compares: at N = 8192 a SIMD holds two waves, too few to
    // hide an LDS round trip per int4
    const int ng = tpad / CHB_G;
    ch_v4i n0 = s_i[0], n1 = s_i[1], n2 = s_i[2], n3 = s_i[3];
    for (int g = 0; g < ng; ++g) {
      const ch_v4i v0 = n0, v1 = n1, v2 = n2, v3 = n3;
      const int gn = min(g + 1, ng - 1) * (CHB_G / 4);
      n0 = s_i[gn + 0];
      n1 = s_i[gn + 1];
      n2 = s_i[gn + 2];
      n3 = s_i[gn + 3];
      const ch_v4i m = (v0 == me) | (v1 == me) | (v2 == me) | (v3 == me);
      if (m.x | m.y | m.z | m.w) {
        const int vv[CHB_G] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w,
                               v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
#pragma unroll
        for (int u = 0; u < CHB_G; ++u)
          if (vv[u] == me) {
            // a hit is never a padding slot, so the row is < M
            const float *p = p2 + (long)(t0 + g * CHB_G + u) * 3;
            ax += wx - p[0];
            ay += wy - p[1];
            az += wz - p[2];
          }
      }
    }
  }
  if (!live) return;

  float fx = 0.f, fy = 0.f, fz = 0.f;
  const int n1 = idx_1[row];
  if (n1 >= 0 && n1 < M) {
    const float *p = p2 + (long)n1 * 3;
    fx = wx - p[0];
    fy = wy - p[1];
    fz = wz - p[2];
  }
  const float g = gout[t];
  dflow[row * 3 + 0] = g * (c1 * fx + c2 * ax);
  dflow[row * 3 + 1] = g * (c1 * fy + c2 * ay);
  dflow[row * 3 + 2] = g * (c1 * fz + c2 * az);
}

// blocks along x, = the last extent of the scratch buffer
int chamfer_fwd_blocks(int N, int M, int ndir) {
  const int Q = ndir == 2 ? max(N, M) : N;
  return (Q + CH_THREADS - 1) / CH_THREADS;
}

void launch_chamfer_fwd(const float *pc1, const float *flow, const float *pc2,
                        float *d2_1, int *idx_1, float *d2_2, int *idx_2,
                        float *partial, int B, int N, int M, int T, int ndir,
                        hipStream_t stream) {
  dim3 grid(chamfer_fwd_blocks(N, M, ndir), B, ndir * T);
  dim3 block(CH_THREADS);
  hipLaunchKernelGGL(chamfer_fwd_kernel, grid, block, 0, stream, pc1, flow,
                     pc2, d2_1, idx_1, d2_2, idx_2, partial, B, N, M, ndir);
}

void launch_chamfer_bwd(const float *pc1, const float *flow, const float *pc2,
                        const int *idx_1, const int *idx_2, const float *gout,
                        float *dflow, int B, int N, int M, int T,
                        hipStream_t stream) {
  dim3 grid((N + CH_THREADS - 1) / CH_THREADS, B, T);
  dim3 block(CH_THREADS);
  const float c1 = 2.f / ((float)B * (float)N);
  const float c2 = 2.f / ((float)B * (float)M);
  hipLaunchKernelGGL(chamfer_bwd_kernel, grid, block, 0, stream, pc1, flow,
                     pc2, idx_1, idx_2, gout, dflow, B, N, M, c1, c2);
}
