// Inverse adjacency (CSR) of a kNN graph as a counting sort.
//
// idx (B, N, K) int32: edge (n, j) has id e = j*N + n and target idx[b,n,j].
// Output, per batch row: edge ids ordered by (target, id), the row offsets,
// and the id split into (e % N, e / N) so the walkers need no division.
//
// Four launches replace the argsort / gather / searchsorted chain:
//   count  : in-degree histogram (integer atomics, order-independent)
//   scan   : chunked exclusive scan -> offsets; re-zeroes the histogram so
//            it doubles as the placement cursor
//   place  : bucket the edge ids (slot inside a row = atomic arrival order)
//   rank   : each edge counts the ids of its row below its own and writes
//            itself at that rank -> the result no longer depends on the
//            arrival order.  Quadratic in the row length (~K typically).
#include <hip/hip_runtime.h>

namespace {

constexpr int CSR_THREADS = 256;
constexpr int SCAN_ITEMS = 4;
constexpr int SCAN_CHUNK = CSR_THREADS * SCAN_ITEMS;

// targets outside [0, N) cannot come out of knn_graph; clamped so a bad
// input cannot index out of bounds
__device__ __forceinline__ int csr_target(const int* __restrict__ idx, long i,
                                          int N) {
  const int t = idx[i];
  return t < 0 ? 0 : (t >= N ? N - 1 : t);
}

__global__ __launch_bounds__(CSR_THREADS) void csr_count_kernel(
    const int* __restrict__ idx, int* __restrict__ cnt, int N, int NK) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * CSR_THREADS + threadIdx.x;
  if (i >= NK) return;
  const int t = csr_target(idx, (long)b * NK + i, N);
  atomicAdd(&cnt[(long)b * N + t], 1);
}

// one block per batch row; chunks of SCAN_CHUNK counts with a running carry
__global__ __launch_bounds__(CSR_THREADS) void csr_scan_kernel(
    int* __restrict__ cnt, int* __restrict__ offsets, int N) {
  __shared__ int wave_sum[CSR_THREADS / 64];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  int* c = cnt + (long)b * N;
  int* off = offsets + (long)b * (N + 1);
  int carry = 0;
  for (int base = 0; base < N; base += SCAN_CHUNK) {
    const int i0 = base + tid * SCAN_ITEMS;
    int v[SCAN_ITEMS];
    int tsum = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
      v[i] = (i0 + i < N) ? c[i0 + i] : 0;
      tsum += v[i];
    }
    int inc = tsum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(inc, d, 64);
      if (lane >= d) inc += up;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    int pre = carry, total = 0;
#pragma unroll
    for (int w = 0; w < CSR_THREADS / 64; ++w) {
      const int s = wave_sum[w];
      if (w < wave) pre += s;
      total += s;
    }
    int run = pre + inc - tsum;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
      if (i0 + i < N) {
        off[i0 + i] = run;
        c[i0 + i] = 0;
      }
      run += v[i];
    }
    carry += total;
    __syncthreads();  // wave_sum is rewritten by the next chunk
  }
  if (tid == 0) off[N] = carry;
}

__global__ __launch_bounds__(CSR_THREADS) void csr_place_kernel(
    const int* __restrict__ idx, const int* __restrict__ offsets,
    int* __restrict__ cursor, int* __restrict__ bucket, int N, int K, int NK) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * CSR_THREADS + threadIdx.x;
  if (i >= NK) return;
  const int n = i / K, j = i - n * K;
  const int t = csr_target(idx, (long)b * NK + i, N);
  const int slot = atomicAdd(&cursor[(long)b * N + t], 1);
  bucket[(long)b * NK + offsets[(long)b * (N + 1) + t] + slot] = j * N + n;
}

__global__ __launch_bounds__(CSR_THREADS) void csr_rank_kernel(
    const int* __restrict__ idx, const int* __restrict__ offsets,
    const int* __restrict__ bucket, int* __restrict__ order,
    int* __restrict__ order_n, unsigned char* __restrict__ order_j, int N,
    int K, int NK) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * CSR_THREADS + threadIdx.x;
  if (i >= NK) return;
  const int n = i / K, j = i - n * K;
  const int e = j * N + n;
  const int t = csr_target(idx, (long)b * NK + i, N);
  const int* off = offsets + (long)b * (N + 1);
  const int s = off[t], len = off[t + 1] - s;
  const int* row = bucket + (long)b * NK + s;
  int rank = 0;
  for (int m = 0; m < len; ++m) rank += row[m] < e;
  const long o = (long)b * NK + s + rank;
  order[o] = e;
  order_n[o] = n;
  order_j[o] = (unsigned char)j;
}

}  // namespace

// cnt (B, N) must be zero on entry (left zero by the scan, then used as the
// placement cursor); bucket (B, K*N) is scratch.
void launch_knn_csr(const int* idx, int* cnt, int* bucket, int* order,
                    int* offsets, int* order_n, unsigned char* order_j, int B,
                    int N, int K, hipStream_t stream) {
  const int NK = N * K;
  dim3 grid((NK + CSR_THREADS - 1) / CSR_THREADS, B);
  hipLaunchKernelGGL(csr_count_kernel, grid, dim3(CSR_THREADS), 0, stream, idx,
                     cnt, N, NK);
  hipLaunchKernelGGL(csr_scan_kernel, dim3(B), dim3(CSR_THREADS), 0, stream,
                     cnt, offsets, N);
  hipLaunchKernelGGL(csr_place_kernel, grid, dim3(CSR_THREADS), 0, stream, idx,
                     offsets, cnt, bucket, N, K, NK);
  hipLaunchKernelGGL(csr_rank_kernel, grid, dim3(CSR_THREADS), 0, stream, idx,
                     offsets, bucket, order, order_n, order_j, N, K, NK);
}
