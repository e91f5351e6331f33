// K21: Euclidean + flow-consistency clustering of a masked point set (absent
// in the reference): the connected components of the exact radius graph
//
//   i ~ j  <=>  |xyz_i - xyz_j|^2 <= eps^2  and  |flow_i - flow_j|^2 <= feps^2
//
// over the eligible points (masked, six finite numbers), squared distances as
// dx*dx + dy*dy + dz*dz in fp32 against the fp32 products.  Components of at
// least min_points members are the objects, ranked by (size descending,
// smallest member index ascending); the first max_objects are kept.
//   out: labels (B,N) int32 (rank or -1), count (B,M) int32, num_objects (B)
//
// Five launches, the kernel boundaries are the only global synchronisation;
// no lane or workgroup ever waits for another one's progress.
//
//  1. cluster_init_kernel    parent[i] = i (eligible) or -1, size = 0,
//                            rank_of = -1, count = 0, status = 0: every
//                            workspace word that is read later is written
//                            here or by a later kernel before its use.
//  2. cluster_link_kernel    one workgroup per (query block, candidate tile)
//                            pair of the lower triangle, linearised into
//                            grid.x so the grid fills the chip at B = 1
//                            (528 workgroups at N = 8192).  The candidate
//                            tile (CL_TILE points: xyz, flow; x = NaN marks
//                            an ineligible one) is broadcast from LDS, one
//                            query point per lane, candidates j < i only.
//                            Every linked pair is united in the global
//                            parent array: find with path halving, then the
//                            LARGER root is hooked under the SMALLER one by
//                            compare-and-swap.  parent[x] <= x always, a
//                            root is the smallest index of its tree, so the
//                            final forest is unique however the races fall.
//                            parent is read with relaxed agent-scope atomic
//                            loads and written with agent-scope atomics
//                            (the eight XCDs have separate L2s; a stale
//                            parent is still an ancestor and costs a retry).
//                            Every find and every retry loop is capped at
//                            N + 1 steps (a chain of strictly decreasing
//                            indices cannot be longer); a lane that hits the
//                            cap sets status[b].
//  3. cluster_flatten_kernel root[i] = root of i (parent is final now),
//                            size[root] += 1 (integer atomics: exact).
//  4. cluster_rank_kernel    one workgroup per batch element: compacts the
//                            roots with size >= min_points in ascending
//                            order (ballot + prefix), ranks them O(C^2) from
//                            LDS tiles, writes count, num_objects, rank_of.
//  5. cluster_label_kernel   labels[i] = rank_of[root[i]].
// A batch element whose status is set returns labels = -1, num_objects = -1.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), VGPRs /
// LDS bytes / scratch bytes: init 14 / 0 / 0, link 22 / 6144 / 0,
// flatten 6 / 0 / 0, rank 18 / 2064 / 0, label 4 / 0 / 0; no AGPRs.
#include <hip/hip_runtime.h>
#include "common.h"

#define CL_THREADS 256
#define CL_TILE 256  // candidates per LDS tile == queries per workgroup
#define CL_WAVES (CL_THREADS / WAVE)

int cluster_tile() { return CL_TILE; }

DEV_INLINE int cl_load(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(CL_THREADS) void cluster_init_kernel(
    const float *__restrict__ xyz,           // (B, N, 3)
    const float *__restrict__ flow,          // (B, N, 3)
    const unsigned char *__restrict__ mask,  // (B, N)
    int *__restrict__ parent,                // (B, N)
    int *__restrict__ size,                  // (B, N)
    int *__restrict__ rank_of,               // (B, N)
    int *__restrict__ count,                 // (B, M)
    int *__restrict__ status,                // (B)
    int N, int M) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * CL_THREADS + threadIdx.x;
  if (blockIdx.x == 0) {
    for (int m = threadIdx.x; m < M; m += CL_THREADS) count[(long)b * M + m] = 0;
    if (threadIdx.x == 0) status[b] = 0;
  }
  if (i >= N) return;
  const long g = (long)b * N + i;
  bool el = mask[g] != 0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
    el = el && isfinite(xyz[g * 3 + a]) && isfinite(flow[g * 3 + a]);
  parent[g] = el ? i : -1;
  size[g] = 0;
  rank_of[g] = -1;
}

// Root of x's tree, halving the path on the way; -1 when the cap is hit.
DEV_INLINE int cl_find(int *parent, int x, int cap) {
  for (int s = 0; s <= cap; ++s) {
    const int p = cl_load(parent + x);
    if (p == x) return x;
    const int gp = cl_load(parent + p);
    if (gp == p) return p;
    // gp is an ancestor of x; min keeps parent[x] monotone under races
    __hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = gp;
  }
  return -1;
}

// Unites the trees of a and b; returns the root it saw last (an ancestor of
// both from then on), or -1 when a cap is hit.
DEV_INLINE int cl_union(int *parent, int a, int b, int cap) {
  for (int r = 0; r <= cap; ++r) {
    a = cl_find(parent, a, cap);
    b = cl_find(parent, b, cap);
    if (a < 0 || b < 0) return -1;
    if (a == b) return a;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    int expected = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return lo;
    a = hi;  // hi was hooked by someone else meanwhile: go on from there
    b = lo;
  }
  return -1;
}

__global__ __launch_bounds__(CL_THREADS) void cluster_link_kernel(
    const float *__restrict__ xyz, const float *__restrict__ flow,
    int *parent, int *status, int N, float eps2, float feps2) {
  __shared__ float sx[CL_TILE], sy[CL_TILE], sz[CL_TILE];
  __shared__ float sfx[CL_TILE], sfy[CL_TILE], sfz[CL_TILE];
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  // blockIdx.x = qb (qb + 1) / 2 + ct, 0 <= ct <= qb
  const long t = blockIdx.x;
  long qb = (long)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
  if (qb < 0) qb = 0;
  while ((qb + 1) * (qb + 2) / 2 <= t) ++qb;  // float rounding: a step or two
  while (qb * (qb + 1) / 2 > t) --qb;
  const int ct = (int)(t - qb * (qb + 1) / 2);
  xyz += (long)b * N * 3;
  flow += (long)b * N * 3;
  parent += (long)b * N;

  {
    const long j = (long)ct * CL_TILE + tid;
    const bool el = j < N && cl_load(parent + j) >= 0;
    sx[tid] = el ? xyz[j * 3 + 0] : NAN;
    sy[tid] = el ? xyz[j * 3 + 1] : 0.f;
    sz[tid] = el ? xyz[j * 3 + 2] : 0.f;
    sfx[tid] = el ? flow[j * 3 + 0] : 0.f;
    sfy[tid] = el ? flow[j * 3 + 1] : 0.f;
    sfz[tid] = el ? flow[j * 3 + 2] : 0.f;
  }
  __syncthreads();  // the only barrier; nothing below waits on another lane

  const long i = qb * CL_TILE + tid;
  if (i >= N || cl_load(parent + i) < 0) return;
  const float x = xyz[i * 3 + 0], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
  const float fx = flow[i * 3 + 0], fy = flow[i * 3 + 1], fz = flow[i * 3 + 2];
  const int jend = ct == qb ? tid : CL_TILE;  // candidates j < i only
  int hint = (int)i;  // an ancestor of i: finds start here
  bool tripped = false;
  for (int jj = 0; jj < jend; ++jj) {
    const float dx = x - sx[jj], dy = y - sy[jj], dz = z - sz[jj];
    const float d2 = dx * dx + dy * dy + dz * dz;  // NaN for an ineligible j
    const float ex = fx - sfx[jj], ey = fy - sfy[jj], ez = fz - sfz[jj];
    const float f2 = ex * ex + ey * ey + ez * ez;
    if (d2 <= eps2 && f2 <= feps2) {
      const int r = cl_union(parent, hint, ct * CL_TILE + jj, N);
      if (r < 0) {
        tripped = true;
        break;
      }
      hint = r;
    }
  }
  if (tripped)
    __hip_atomic_store(status + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(CL_THREADS) void cluster_flatten_kernel(
    const int *__restrict__ parent, int *__restrict__ root, int *size,
    int *status, int N) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= N) return;
  parent += (long)b * N;
  int x = parent[i];
  if (x < 0) return;
  bool found = false;
  for (int s = 0; s <= N; ++s) {
    const int p = parent[x];
    if (p == x) {
      found = true;
      break;
    }
    x = p;
  }
  if (!found) {
    __hip_atomic_store(status + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = i;
  } else {
    atomicAdd(size + (long)b * N + x, 1);
  }
  root[(long)b * N + i] = x;
}

__global__ __launch_bounds__(CL_THREADS) void cluster_rank_kernel(
    const int *__restrict__ parent, const int *__restrict__ size,
    int *cand,                   // (B, N) workspace: qualifying roots, ascending
    int *__restrict__ rank_of,   // (B, N)
    int *__restrict__ count,     // (B, M)
    int *__restrict__ nobj,      // (B)
    const int *__restrict__ status, int N, int M, int min_points) {
  __shared__ int wcnt[CL_WAVES];
  __shared__ int troot[CL_TILE], tsize[CL_TILE];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  parent += (long)b * N;
  size += (long)b * N;
  cand += (long)b * N;
  rank_of += (long)b * N;
  count += (long)b * M;
  if (status[b] != 0) {  // block-uniform
    if (tid == 0) nobj[b] = -1;
    return;
  }

  int C = 0;  // block-uniform running count
  for (int base = 0; base < N; base += CL_THREADS) {
    const int i = base + tid;
    const bool q = i < N && parent[i] == i && size[i] >= min_points;
    const unsigned long long bal = __ballot(q);
    if (lane_id() == 0) wcnt[wave_id()] = __popcll(bal);
    __syncthreads();
    int off = C, tot = 0;
#pragma unroll
    for (int w = 0; w < CL_WAVES; ++w) {
      const int c = wcnt[w];
      off += w < wave_id() ? c : 0;
      tot += c;
    }
    if (q) cand[off + __popcll(bal & ((1ull << lane_id()) - 1ull))] = i;
    C += tot;
    __syncthreads();
  }

  for (int cbase = 0; cbase < C; cbase += CL_THREADS) {
    const int c = cbase + tid;
    const int myroot = c < C ? cand[c] : 0;
    const int mysize = c < C ? size[myroot] : 0;
    int rank = 0;
    for (int tbase = 0; tbase < C; tbase += CL_TILE) {
      __syncthreads();
      if (tbase + tid < C) {
        const int r = cand[tbase + tid];
        troot[tid] = r;
        tsize[tid] = size[r];
      }
      __syncthreads();
      const int n = min(CL_TILE, C - tbase);
      for (int k = 0; k < n; ++k) {
        const int s = tsize[k];
        rank += (s > mysize || (s == mysize && troot[k] < myroot)) ? 1 : 0;
      }
    }
    if (c < C && rank < M) {
      count[rank] = mysize;
      rank_of[myroot] = rank;
    }
  }
  if (tid == 0) nobj[b] = C < M ? C : M;
}

__global__ __launch_bounds__(CL_THREADS) void cluster_label_kernel(
    const int *__restrict__ parent, const int *__restrict__ root,
    const int *__restrict__ rank_of, const int *__restrict__ status,
    int *__restrict__ labels, int N) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= N) return;
  const long g = (long)b * N + i;
  int lab = -1;
  if (status[b] == 0 && parent[g] >= 0) lab = rank_of[(long)b * N + root[g]];
  labels[g] = lab;
}

// ws: 5 * B * N ints (parent, size, root, rank_of, cand); status: B ints.
void launch_cluster_points(const float *xyz, const float *flow,
                           const unsigned char *mask, int *ws, int *status,
                           int *labels, int *count, int *nobj, int B, int N,
                           int M, float eps, float flow_eps, int min_points,
                           hipStream_t stream) {
  const long BN = (long)B * N;
  int *parent = ws, *size = ws + BN, *root = ws + 2 * BN, *rank_of = ws + 3 * BN,
      *cand = ws + 4 * BN;
  const int nblk = (N + CL_THREADS - 1) / CL_THREADS;
  const dim3 block(CL_THREADS), pts(nblk, B);
  hipLaunchKernelGGL(cluster_init_kernel, pts, block, 0, stream, xyz, flow, mask,
                     parent, size, rank_of, count, status, N, M);
  const float eps2 = eps * eps, feps2 = flow_eps * flow_eps;
  const long tri = (long)nblk * (nblk + 1) / 2;
  hipLaunchKernelGGL(cluster_link_kernel, dim3((unsigned)tri, B), block, 0, stream,
                     xyz, flow, parent, status, N, eps2, feps2);
  hipLaunchKernelGGL(cluster_flatten_kernel, pts, block, 0, stream, parent, root,
                     size, status, N);
  hipLaunchKernelGGL(cluster_rank_kernel, dim3(B), block, 0, stream, parent, size,
                     cand, rank_of, count, nobj, status, N, M, min_points);
  hipLaunchKernelGGL(cluster_label_kernel, pts, block, 0, stream, parent, root,
                     rank_of, status, labels, N);
}
