// K19: flow smoothness over the kNN graph of pc1, for T flows at once
// (absent in the reference).
//
//   smooth_t = 1 / (B N k) * sum_{b,i} sum_{j in idx[b,i]} |f_t[b,j] - f_t[b,i]|^2
//
// Forward: one lane per point, grid (ceil(N / 256), B, T); a lane gathers
// its k neighbour flow rows and each block folds its lanes in a fixed order
// into one slot of a (T, B, blocks) scratch buffer, which the caller sums.
//
// Backward (atomic-free): point i collects its own k edges from idx and the
// edges that point AT it from the inverse adjacency (Graph.csr(): offsets
// (B, N+1), order_n (B, N k) = source point of each edge, sorted by target),
//
//   df_t[b,i] = g_t * 2 / (B N k) * [ sum_{j in idx[i]} (f_i - f_j)
//                                   + sum_{n: i in idx[n]} (f_i - f_n) ]
//
// Neighbour ids outside [0, N) are skipped and CSR bounds are clamped, so a
// malformed graph cannot read out of bounds.
#include <hip/hip_runtime.h>
#include "common.h"

#define FS_THREADS 256

__global__ __launch_bounds__(FS_THREADS) void flow_smooth_fwd_kernel(
    const float *__restrict__ flow,  // (T, B, N, 3)
    const int *__restrict__ idx,     // (B, N, k)
    float *__restrict__ partial,     // (T, B, gridDim.x)
    int B, int N, int k) {
  __shared__ float s_part[FS_THREADS / WAVE];
  const int b = blockIdx.y;
  const int t = blockIdx.z;
  const int i = blockIdx.x * FS_THREADS + threadIdx.x;
  const float *f = flow + ((long)t * B + b) * N * 3;
  float acc = 0.f;
  if (i < N) {
    const float fx = f[(long)i * 3 + 0];
    const float fy = f[(long)i * 3 + 1];
    const float fz = f[(long)i * 3 + 2];
    const int *nb = idx + ((long)b * N + i) * k;
    for (int j = 0; j < k; ++j) {
      const int n = nb[j];
      if (n < 0 || n >= N) continue;
      const float dx = f[(long)n * 3 + 0] - fx;
      const float dy = f[(long)n * 3 + 1] - fy;
      const float dz = f[(long)n * 3 + 2] - fz;
      acc += dx * dx + dy * dy + dz * dz;
    }
  }
  acc = wave_sum(acc);
  if (lane_id() == 0) s_part[wave_id()] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float r = 0.f;
#pragma unroll
    for (int w = 0; w < FS_THREADS / WAVE; ++w) r += s_part[w];
    partial[((long)t * B + b) * gridDim.x + blockIdx.x] = r;
  }
}

__global__ __launch_bounds__(FS_THREADS) void flow_smooth_bwd_kernel(
    const float *__restrict__ flow,     // (T, B, N, 3)
    const int *__restrict__ idx,        // (B, N, k)
    const int *__restrict__ offsets,    // (B, N + 1)
    const int *__restrict__ order_n,    // (B, N k)
    const float *__restrict__ gout,     // (T)
    float *__restrict__ dflow,          // (T, B, N, 3)
    int B, int N, int k, float c) {
  const int b = blockIdx.y;
  const int t = blockIdx.z;
  const int i = blockIdx.x * FS_THREADS + threadIdx.x;
  if (i >= N) return;
  const float *f = flow + ((long)t * B + b) * N * 3;
  const float fx = f[(long)i * 3 + 0];
  const float fy = f[(long)i * 3 + 1];
  const float fz = f[(long)i * 3 + 2];
  float ax = 0.f, ay = 0.f, az = 0.f;
  const int *nb = idx + ((long)b * N + i) * k;
  for (int j = 0; j < k; ++j) {
    const int n = nb[j];
    if (n < 0 || n >= N) continue;
    ax += fx - f[(long)n * 3 + 0];
    ay += fy - f[(long)n * 3 + 1];
    az += fz - f[(long)n * 3 + 2];
  }
  const long E = (long)N * k;
  const int *off = offsets + (long)b * (N + 1);
  const int *src = order_n + (long)b * E;
  const long e0 = max(0L, min((long)off[i], E));
  const long e1 = max(e0, min((long)off[i + 1], E));
  for (long e = e0; e < e1; ++e) {
    const int n = src[e];
    if (n < 0 || n >= N) continue;
    ax += fx - f[(long)n * 3 + 0];
    ay += fy - f[(long)n * 3 + 1];
    az += fz - f[(long)n * 3 + 2];
  }
  const float g = gout[t] * c;
  float *d = dflow + (((long)t * B + b) * N + i) * 3;
  d[0] = g * ax;
  d[1] = g * ay;
  d[2] = g * az;
}

int flow_smooth_blocks(int N) { return (N + FS_THREADS - 1) / FS_THREADS; }

void launch_flow_smooth_fwd(const float *flow, const int *idx, float *partial,
                            int B, int N, int k, int T, hipStream_t stream) {
  dim3 grid(flow_smooth_blocks(N), B, T);
  dim3 block(FS_THREADS);
  hipLaunchKernelGGL(flow_smooth_fwd_kernel, grid, block, 0, stream, flow, idx,
                     partial, B, N, k);
}

void launch_flow_smooth_bwd(const float *flow, const int *idx,
                            const int *offsets, const int *order_n,
                            const float *gout, float *dflow, int B, int N,
                            int k, int T, hipStream_t stream) {
  dim3 grid(flow_smooth_blocks(N), B, T);
  dim3 block(FS_THREADS);
  const float c = 2.f / ((float)B * (float)N * (float)k);
  hipLaunchKernelGGL(flow_smooth_bwd_kernel, grid, block, 0, stream, flow, idx,
                     offsets, order_n, gout, dflow, B, N, k, c);
}
