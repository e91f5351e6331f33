// Operand staging for the pointwise (1x1-conv) MFMA kernels.
//
// A bf16 operand tile is copied from global memory to LDS ROW BY ROW, as
// it lies in memory: 16-byte global loads, 16-byte LDS stores.  The MFMA
// operand that needs the tile's COLUMNS as its k-contiguous fragments is
// then read back with the gfx950 transposed LDS read (ds_read_b64_tr_b16),
// so no kernel transposes with 2-byte LDS stores on the way in.
//
// k order.  v_mfma_f32_16x16x32_bf16 sums 32 k-slots; lane group g =
// lane >> 4 supplies slots 8g .. 8g+7 of both operands.  Which k each slot
// holds is free as long as both operands agree.  pws_tr_frag() fills group
// g's slots with rows  kb + 4g + {0..3}  and  kb + 16 + 4g + {0..3}: the two
// 32-lane halves of each read then cover 8 CONSECUTIVE tile rows, which a
// row pitch of 8 * odd dwords spreads over all 64 banks (conflict-free;
// MI355X ds_read_b64 banking is per 32-lane half).  pws_row_frag() reads
// the same slots from a tile that already is k-contiguous.
//
// The transposed read gathers across lanes: EXEC must be all ones (no
// early return, no lane-dependent branch around it), every lane's address
// 8-byte aligned and inside the tile -- so tiles are padded, never masked.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

typedef __attribute__((ext_vector_type(8))) __bf16 pws_bf16x8;
typedef __attribute__((ext_vector_type(4))) short pws_i16x4;
typedef __attribute__((ext_vector_type(8))) short pws_i16x8;

typedef uint4 __attribute__((aligned(2))) pws_u4u;  // unaligned global load

#define PWS_THREADS 256

// Row pitch (bf16 elements) for a tile of `cols` columns read with
// pws_tr_frag: the smallest multiple of 16 elements (8 dwords) >= cols whose
// dword count is 8 * odd.
__host__ __device__ constexpr int pws_tr_pitch(int cols) {
  return (((cols + 15) / 16) | 1) * 16;
}

// Row pitch for a k-contiguous tile of `k` (multiple of 32) columns read
// with pws_row_frag: k/2 + 4 dwords == 4 mod 8, 16 rows x 2 groups of a
// half land on distinct banks.
__host__ __device__ inline int pws_row_pitch(int k) { return k + 8; }

__device__ __forceinline__ unsigned pws_relu_mask2(unsigned d, unsigned y) {
  // two packed bf16: keep d where y > 0 (threshold_backward: y <= 0 -> +0;
  // NaN y keeps d)
  const float ylo = __uint_as_float(y << 16);
  const float yhi = __uint_as_float(y & 0xffff0000u);
  unsigned r = d;
  if (ylo <= 0.f) r &= 0xffff0000u;
  if (yhi <= 0.f) r &= 0x0000ffffu;
  return r;
}

// Copy rows [0, nr_pad) x columns [0, nc) of a row-major bf16 matrix into
// the LDS tile s (row pitch `pitch`); nc is a multiple of 8.  Rows >= nr
// and columns >= ncv are written as zero.  `vec` (workgroup-uniform): whole
// 8-column chunks move as 16 bytes; chunks cut by ncv, and everything in
// the non-vec case, go element by element.  With vec the msk / out rows
// must be 16-byte aligned at every chunk; src rows need only their natural
// alignment (a 16-byte global LOAD may be unaligned, as the odd-pitch
// weight slices -- Ci 61, column offsets 61 / 125 -- are).
//   msk : optional ReLU output with src's geometry; elements whose msk is
//         <= 0 are zeroed (the ReLU backward mask)
//   out : optional global copy of the staged (masked) values, rows
//         `ostride` apart -- valid rows / columns only
__device__ __forceinline__ void pws_stage_rows(
    __hip_bfloat16 *s, int pitch, const __hip_bfloat16 *src, long rstride,
    int nr, int nr_pad, int nc, int ncv, bool vec,
    const __hip_bfloat16 *msk, __hip_bfloat16 *out, long ostride) {
  const int n8 = nc >> 3;
  for (int i = threadIdx.x; i < nr_pad * n8; i += PWS_THREADS) {
    const int r = i / n8;
    const int c8 = (i - r * n8) << 3;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (r < nr && c8 < ncv) {
      const long go = (long)r * rstride + c8;
      if (vec && c8 + 8 <= ncv) {
        v = *(const pws_u4u *)(src + go);
        if (msk != nullptr) {
          const uint4 m = *(const uint4 *)(msk + go);
          v.x = pws_relu_mask2(v.x, m.x);
          v.y = pws_relu_mask2(v.y, m.y);
          v.z = pws_relu_mask2(v.z, m.z);
          v.w = pws_relu_mask2(v.w, m.w);
        }
        if (out != nullptr) *(uint4 *)(out + (long)r * ostride + c8) = v;
      } else {
        unsigned short e8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          unsigned short h = 0;
          if (c8 + e < ncv) {
            h = ((const unsigned short *)src)[go + e];
            if (msk != nullptr) {
              const unsigned short m = ((const unsigned short *)msk)[go + e];
              if (__uint_as_float((unsigned)m << 16) <= 0.f) h = 0;
            }
            if (out != nullptr)
              ((unsigned short *)out)[(long)r * ostride + c8 + e] = h;
          }
          e8[e] = h;
        }
        v.x = e8[0] | ((unsigned)e8[1] << 16);
        v.y = e8[2] | ((unsigned)e8[3] << 16);
        v.z = e8[4] | ((unsigned)e8[5] << 16);
        v.w = e8[6] | ((unsigned)e8[7] << 16);
      }
    }
    *(uint4 *)&s[(long)r * pitch + c8] = v;
  }
}

// MFMA operand fragment for 16 tile COLUMNS col0 .. col0+15 (col0 a
// multiple of 4) over tile rows kb .. kb+31 of a row-major LDS tile: lane
// (g = lane >> 4, i = lane & 15) receives column col0 + i of rows
// kb + 4g + {0..3} and kb + 16 + 4g + {0..3}.  All 64 lanes must be active.
//
// NATURAL = true keeps the plain slot order instead (group g holds rows
// kb + 8g .. 8g+7, what a 16-byte row read of a k-contiguous tile gives):
// the MFMA's result depends on which slot a product sits in, so a kernel
// that must reproduce such a tile bit for bit reads this way, at a 2-way
// bank conflict (a half's two groups are 8 rows apart).
template <bool NATURAL = false>
__device__ __forceinline__ pws_bf16x8 pws_tr_frag(const __hip_bfloat16 *s,
                                                  int pitch, int kb, int col0,
                                                  int lane) {
  const int g = lane >> 4;
  const int q = (lane >> 2) & 3;
  const int p = lane & 3;
  const int r0 = NATURAL ? 8 * g : 4 * g;
  const int hi_rows = NATURAL ? 4 : 16;
  const __hip_bfloat16 *a = s + (long)(kb + r0 + q) * pitch + col0 + 4 * p;
  typedef __attribute__((address_space(3))) pws_i16x4 lds_i16x4;
  const pws_i16x4 lo =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4 *)a);
  const pws_i16x4 hi =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4 *)(a + hi_rows * pitch));
  const pws_i16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(pws_bf16x8, v);
}

// The same k-slots from a k-contiguous tile (row = MFMA row/column index,
// columns = k): two 8-byte reads.
__device__ __forceinline__ pws_bf16x8 pws_row_frag(const __hip_bfloat16 *s,
                                                   int pitch, int row, int kb,
                                                   int lane) {
  const int g = lane >> 4;
  const __hip_bfloat16 *a = s + (long)row * pitch + kb + 4 * g;
  const pws_i16x4 lo = *(const pws_i16x4 *)a;
  const pws_i16x4 hi = *(const pws_i16x4 *)(a + 16);
  const pws_i16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(pws_bf16x8, v);
}
