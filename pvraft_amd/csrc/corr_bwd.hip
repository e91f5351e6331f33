// Truncated-correlation backward / forward helpers.
//
// corr_grad_expand: sparse gradient (B, N, K) fp32 + top-K indices (B, N, K)
// i32 -> dense (B, N, M) bf16 / fp32 matrix that the two fmap GEMMs read.
// The composed form (zeros + mul + cast + scatter_) touched the dense
// matrix twice and the sparse one three times; here every output element
// is stored exactly once, zeros included, from an LDS image of its row:
//   zero the image (16-byte LDS stores) | barrier | place round(g * scale)
//   at idx | barrier | stream the image out with 16-byte coalesced stores.
// One workgroup per row.  The product is taken in fp32 and rounded to
// nearest even, the order of `(g * scale).to(bf16)`, so the matrix is
// bit-equal to the composed one.  A row that repeats an index keeps one of
// the competing values (unspecified which, as with scatter_).
//
// corr_gather_xyz: txyz[b, n, k, :] = xyz2[b, idx[b, n, k], :] from the i32
// indices (no int64 copy, no expanded index).  xyz2 of one batch is 96 KB
// and is served by L2; a workgroup assembles 1024 entries (12 KB) in LDS
// and streams them out with 16-byte stores.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include "common.h"

#define CB_THREADS 256

// fp32 -> bf16 bits, round to nearest even (NaN -> quiet NaN)
DEV_INLINE unsigned short cb_bf16_rne(float v) {
  const unsigned u = __float_as_uint(v);
  if (v != v) return 0x7FC0;
  return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

template <typename T>
DEV_INLINE T cb_cvt(float v);
template <>
DEV_INLINE float cb_cvt<float>(float v) { return v; }
template <>
DEV_INLINE unsigned short cb_cvt<unsigned short>(float v) {
  return cb_bf16_rne(v);
}

// copy `bytes` (a multiple of sizeof(V)) from the LDS image to the row
template <typename V>
DEV_INLINE void cb_stream_row(const void *img, void *dst, int bytes) {
  const V *s = (const V *)img;
  V *d = (V *)dst;
  const int n = bytes / (int)sizeof(V);
  for (int i = threadIdx.x; i < n; i += CB_THREADS) d[i] = s[i];
}

// T = float, or unsigned short holding bf16 bits
template <typename T>
__global__ __launch_bounds__(CB_THREADS) void corr_grad_expand_kernel(
    const float *__restrict__ g,   // (R, K)
    const int *__restrict__ idx,   // (R, K)
    T *__restrict__ out,           // (R, M)
    int K, int M, float scale) {
  extern __shared__ uint4 cb_img[];  // ceil(M * sizeof(T) / 16) vectors
  T *img = (T *)cb_img;
  const long r = blockIdx.x;
  const int row_bytes = M * (int)sizeof(T);
  const int nvec = (row_bytes + 15) >> 4;
  for (int i = threadIdx.x; i < nvec; i += CB_THREADS)
    cb_img[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();

  const float *gr = g + r * K;
  const int *ir = idx + r * K;
  if ((K & 3) == 0 &&
      (((unsigned long long)g | (unsigned long long)idx) & 15) == 0) {
    // every row of g / idx starts 16-byte aligned
    for (int k = threadIdx.x * 4; k < K; k += CB_THREADS * 4) {
      const float4 gv = *(const float4 *)(gr + k);
      const int4 iv = *(const int4 *)(ir + k);
      if ((unsigned)iv.x < (unsigned)M) img[iv.x] = cb_cvt<T>(gv.x * scale);
      if ((unsigned)iv.y < (unsigned)M) img[iv.y] = cb_cvt<T>(gv.y * scale);
      if ((unsigned)iv.z < (unsigned)M) img[iv.z] = cb_cvt<T>(gv.z * scale);
      if ((unsigned)iv.w < (unsigned)M) img[iv.w] = cb_cvt<T>(gv.w * scale);
    }
  } else {
    for (int k = threadIdx.x; k < K; k += CB_THREADS) {
      const int m = ir[k];
      if ((unsigned)m < (unsigned)M) img[m] = cb_cvt<T>(gr[k] * scale);
    }
  }
  __syncthreads();

  // widest store the row pitch keeps aligned on every row (the tensor base
  // is allocator-aligned, the image base 16-byte aligned)
  T *dst = out + r * M;
  if ((row_bytes & 15) == 0) cb_stream_row<uint4>(img, dst, row_bytes);
  else if ((row_bytes & 7) == 0) cb_stream_row<uint2>(img, dst, row_bytes);
  else if ((row_bytes & 3) == 0) cb_stream_row<unsigned>(img, dst, row_bytes);
  else cb_stream_row<T>(img, dst, row_bytes);
}

void launch_corr_grad_expand(const float *g, const int *idx, void *out,
                             long rows, int K, int M, float scale, bool bf16,
                             hipStream_t stream) {
  if (rows <= 0) return;
  const size_t esz = bf16 ? 2 : 4;
  const size_t shmem = (((size_t)M * esz + 15) / 16) * 16;  // <= 64 KB
  if (bf16)
    hipLaunchKernelGGL(corr_grad_expand_kernel<unsigned short>,
                       dim3((unsigned)rows), dim3(CB_THREADS), shmem, stream,
                       g, idx, (unsigned short *)out, K, M, scale);
  else
    hipLaunchKernelGGL(corr_grad_expand_kernel<float>, dim3((unsigned)rows),
                       dim3(CB_THREADS), shmem, stream, g, idx, (float *)out,
                       K, M, scale);
}

#define CG_EPT 4                            // entries per thread
#define CG_TILE (CB_THREADS * CG_EPT)       // entries per workgroup

struct CgXyz { float x, y, z; };

__global__ __launch_bounds__(CB_THREADS) void corr_gather_xyz_kernel(
    const int *__restrict__ idx,     // (B * NK)
    const float *__restrict__ xyz2,  // (B, M, 3)
    float *__restrict__ out,         // (B * NK, 3)
    long total, long NK, int M) {
  __shared__ __attribute__((aligned(16))) float tile[CG_TILE * 3];
  const long e0 = (long)blockIdx.x * CG_TILE;
  const long e = e0 + (long)threadIdx.x * CG_EPT;
  if (e < total) {
    int m[CG_EPT];
    if (e + CG_EPT <= total && ((unsigned long long)idx & 15) == 0) {
      const int4 iv = *(const int4 *)(idx + e);  // e % 4 == 0
      m[0] = iv.x; m[1] = iv.y; m[2] = iv.z; m[3] = iv.w;
    } else {
#pragma unroll
      for (int j = 0; j < CG_EPT; ++j) m[j] = (e + j < total) ? idx[e + j] : 0;
    }
    long b = e / NK;
    long bend = (b + 1) * NK;  // first entry of the next batch
#pragma unroll
    for (int j = 0; j < CG_EPT; ++j) {
      if (e + j >= bend) { ++b; bend += NK; }
      const int mm = min(max(m[j], 0), M - 1);
      const CgXyz p = (e + j < total)
          ? *(const CgXyz *)(xyz2 + (b * M + mm) * 3) : CgXyz{0.f, 0.f, 0.f};
      float *t = tile + (threadIdx.x * CG_EPT + j) * 3;
      t[0] = p.x; t[1] = p.y; t[2] = p.z;
    }
  }
  __syncthreads();
  // the tile starts at float 3 * e0, a multiple of 4 floats
  const long f0 = e0 * 3;
  const long fend = total * 3;
  for (int i = threadIdx.x * 4; i < CG_TILE * 3; i += CB_THREADS * 4) {
    const long f = f0 + i;
    if (f + 4 <= fend) {
      *(float4 *)(out + f) = *(const float4 *)(tile + i);
    } else {
      for (int j = 0; j < 4; ++j)
        if (f + j < fend) out[f + j] = tile[i + j];
    }
  }
}

void launch_corr_gather_xyz(const int *idx, const float *xyz2, float *out,
                            int B, long NK, int M, hipStream_t stream) {
  const long total = (long)B * NK;
  if (total <= 0) return;
  const long blocks = (total + CG_TILE - 1) / CG_TILE;
  hipLaunchKernelGGL(corr_gather_xyz_kernel, dim3((unsigned)blocks),
                     dim3(CB_THREADS), 0, stream, idx, xyz2, out, total, NK,
                     M);
}
