// Training-image resize on the GPU: the Resize((S, S)) of lib/dataset.py:103 (torchvision's
// Resize on a PIL image = Image.resize(..., BILINEAR)) in Pillow's own 8-bit arithmetic
// (libImaging/Resample.c), so a decoded source image resident in HBM gives every stage's
// training image without the host: the bytes equal PIL's (tests/test_gpu_resize.py).
//
// Pillow's resize is separable and pure integer arithmetic once the coefficient tables exist:
// per axis and output position a window (first tap, tap count) and 22-bit fixed-point weights,
//   out = clip8((2^21 + sum_x pixel[xmin + x] * k[x]) >> 22),
// a horizontal pass into a uint8 image [Hin][S][3], then a vertical pass over that.  The tables
// depend on (in, out) only; the host builds them in float64 exactly as Pillow does
// (pggan_amd.data.resize_coeffs) and passes them as device pointers.  Weights are >= 0 and sum
// to 2^22 +- ksize / 2, so an int32 accumulator never overflows, and integer addition is
// associative: a sum split over lanes in any order is still exact.
//
// Two launches per call (one when an axis already has the target size: Pillow skips that pass):
//  (1) horizontal: a workgroup stages RZ_ROWS whole source rows in LDS with 16-byte loads (the
//      one read of the source from HBM; rows are 3 Win bytes with no alignment, so the span is
//      read from its 16-byte-aligned start) and computes all 3 S output bytes of each row.  An
//      output column's taps are split over P lanes (P = 1 for the 5-tap 1024 -> 512, 64 for the
//      513-tap 1024 -> 4) and added with wave shuffles; a tap's weight is loaded once for the
//      RZ_ROWS rows.  Writes the intermediate in the caller's workspace, rows padded to 16 bytes.
//  (2) vertical: a work item is 4 consecutive bytes of an output row (the weights do not depend
//      on the column, so a row is a flat byte array): one dword load per tap, four sums, the
//      taps again split over P lanes.  Reads the intermediate (L2-resident: each row feeds ~2
//      output rows) or, with the horizontal pass skipped, the source.
// Sources are rows of a ragged cache buffer and destinations scattered rows of a batch: both
// are given as a base pointer and per-image int64 byte offsets in device memory.
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

constexpr int RZ_BLOCK = 256;
constexpr int RZ_ROWS = 8;              // source rows per workgroup of the horizontal pass
constexpr int RZ_BITS = 22;             // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int RZ_LDS_MAX = 64 * 1024;   // the horizontal pass's staging limit

// Pillow's clip8((2^21 + sum) >> 22).  The sums are >= 0 (no negative bilinear weight), so only
// the upper clip can act and the arithmetic is unsigned.  That also keeps two adjacent clips
// from being fused into v_ashr_pk_u8_i32: the instruction leaves the upper half of its
// destination as it was, while the code generator (ROCm 7 hipcc) packs further bytes above it
// as if that half were zero -- the signed form gave wrong bytes 2 and 3 of every dword here.
__device__ __forceinline__ uint32_t rz_clip8(int acc) {
  const uint32_t v = ((uint32_t)acc + (1u << (RZ_BITS - 1))) >> RZ_BITS;
  return v > 255u ? 255u : v;
}

// sum over the P lanes (a power of two <= 64) of a lane group
__device__ __forceinline__ int rz_group_sum(int v, int P) {
  for (int o = P >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Horizontal pass.  grid (ceil(Hin / RZ_ROWS), n); dynamic LDS: RZ_ROWS * 3 * Win + 32 bytes.
// dst row y of image i: dst_base + (dst_off ? dst_off[i] : i * dst_img) + y * dst_stride.
__global__ __launch_bounds__(RZ_BLOCK) void rz_horizontal(
    const unsigned char* src_base, const int64_t* src_off, int Hin, int Win, int S,
    const int* kx, const int* bx, int ksx, unsigned char* dst_base, const int64_t* dst_off,
    size_t dst_img, size_t dst_stride, int P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rz_lds[];
  const int img = blockIdx.y, tid = threadIdx.x;
  const int r0 = blockIdx.x * RZ_ROWS;
  const int nr = min(RZ_ROWS, Hin - r0);
  const size_t rowb = (size_t)3 * Win;
  const unsigned char* image = src_base + src_off[img];
  const unsigned char* image_end = image + rowb * Hin;
  const unsigned char* span = image + rowb * r0;
  const int head = (int)((uintptr_t)span & 15);
  const unsigned char* start = span - head;           // 16-byte aligned, inside the image when
  const int nbytes = head + (int)(rowb * nr);         // image starts are aligned as agreed
  for (int o = tid * 16; o < nbytes; o += RZ_BLOCK * 16) {
    uint4 v;
    if (start + o + 16 <= image_end) {
      v = *reinterpret_cast<const uint4*>(start + o);
    } else {   // the image's last bytes: nothing is read past its end
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (start + o + j < image_end) w[j >> 2] |= (uint32_t)start[o + j] << (8 * (j & 3));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4*>(rz_lds + o) = v;
  }
  __syncthreads();
  const unsigned char* rows = rz_lds + head;
  unsigned char* out = dst_base + (dst_off ? (size_t)dst_off[img] : (size_t)img * dst_img) +
                       (size_t)r0 * dst_stride;
  const int ncol = 3 * S, ngroup = RZ_BLOCK / P;
  const int g = tid / P, p = tid % P;
  // uniform trip count: every lane takes part in the shuffles
  for (int c0 = 0; c0 < ncol; c0 += ngroup) {
    const int col = c0 + g;
    const bool live = col < ncol;
    const int xx = live ? col / 3 : 0, ch = live ? col % 3 : 0;
    const int xmin = bx[2 * xx], cnt = live ? bx[2 * xx + 1] : 0;
    const int* k = kx + (size_t)xx * ksx;
    const unsigned char* px = rows + (size_t)xmin * 3 + ch;
    int acc[RZ_ROWS];
#pragma unroll
    for (int r = 0; r < RZ_ROWS; ++r) acc[r] = 0;
    for (int x = p; x < cnt; x += P) {
      const int w = k[x];
#pragma unroll
      for (int r = 0; r < RZ_ROWS; ++r)
        if (r < nr) acc[r] += (int)px[(size_t)r * rowb + (size_t)x * 3] * w;
    }
#pragma unroll
    for (int r = 0; r < RZ_ROWS; ++r) {
      const int s = rz_group_sum(acc[r], P);
      if (live && p == 0 && r < nr) out[(size_t)r * dst_stride + col] = (unsigned char)rz_clip8(s);
    }
  }
}

// Vertical pass.  grid (ceil(S * nchunk * P / RZ_BLOCK), n), nchunk = ceil(3 S / 4).  Input row y
// of image i: in_base + (in_off ? in_off[i] : i * in_img) + y * in_stride.  ALIGNED: every
// input row starts 4-byte aligned and holds 4 * nchunk readable bytes (the padded intermediate,
// or a source with 3 S % 4 == 0); otherwise byte loads.
template <bool ALIGNED>
__global__ __launch_bounds__(RZ_BLOCK) void rz_vertical(
    const unsigned char* in_base, const int64_t* in_off, size_t in_img, size_t in_stride, int S,
    const int* ky, const int* by, int ksy, unsigned char* dst_base, const int64_t* dst_off,
    int P) {
  const int img = blockIdx.y;
  const int rowb = 3 * S, nchunk = (rowb + 3) / 4;
  const int item = (int)(((size_t)blockIdx.x * RZ_BLOCK + threadIdx.x) / P), p = threadIdx.x % P;
  const bool live = item < S * nchunk;
  const int yy = live ? item / nchunk : 0, j = live ? (item % nchunk) * 4 : 0;
  const int ymin = by[2 * yy], cnt = live ? by[2 * yy + 1] : 0;
  const int* k = ky + (size_t)yy * ksy;
  const unsigned char* in = in_base + (in_off ? (size_t)in_off[img] : (size_t)img * in_img) +
                            (size_t)ymin * in_stride + j;
  const int nb = min(4, rowb - j);
  int acc[4] = {0, 0, 0, 0};
  for (int y = p; y < cnt; y += P) {
    const int w = k[y];
    const unsigned char* q = in + (size_t)y * in_stride;
    if (ALIGNED) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(q);
      acc[0] += (int)(v & 255u) * w;
      acc[1] += (int)((v >> 8) & 255u) * w;
      acc[2] += (int)((v >> 16) & 255u) * w;
      acc[3] += (int)(v >> 24) * w;
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (b < nb) acc[b] += (int)q[b] * w;
    }
  }
  uint32_t o = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) o |= rz_clip8(rz_group_sum(acc[b], P)) << (8 * b);
  if (!live || p != 0) return;
  unsigned char* d = dst_base + dst_off[img] + (size_t)yy * rowb + j;
  if (nb == 4 && ((uintptr_t)d & 3) == 0) {
    *reinterpret_cast<uint32_t*>(d) = o;
  } else {
    for (int b = 0; b < nb; ++b) d[b] = (unsigned char)(o >> (8 * b));
  }
}

// Both passes skipped (Pillow returns a copy).  grid (blocks, n), grid-stride over 16-byte units
// when both images are 16-byte aligned, over bytes otherwise.
__global__ __launch_bounds__(RZ_BLOCK) void rz_copy(const unsigned char* src_base,
                                                    const int64_t* src_off,
                                                    unsigned char* dst_base,
                                                    const int64_t* dst_off, size_t bytes) {
  const unsigned char* s = src_base + src_off[blockIdx.y];
  unsigned char* d = dst_base + dst_off[blockIdx.y];
  const size_t t = (size_t)blockIdx.x * RZ_BLOCK + threadIdx.x, nt = (size_t)gridDim.x * RZ_BLOCK;
  size_t done = 0;
  if ((((uintptr_t)s | (uintptr_t)d) & 15) == 0) {
    const size_t n16 = bytes / 16;
    for (size_t i = t; i < n16; i += nt)
      reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(s)[i];
    done = n16 * 16;
  }
  for (size_t i = done + t; i < bytes; i += nt) d[i] = s[i];
}

// lanes per sum: enough that a lane adds ~8 taps, a power of two <= 64
int rz_lanes(int ksize) {
  int P = 1;
  while (P < 64 && ksize > 8 * P) P *= 2;
  return P;
}

size_t rz_mid_stride(int S) { return ((size_t)3 * S + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

size_t pg_resize_workspace_bytes(int n, int Hin, int Win, int S) {
  if (n <= 0 || Hin <= 0 || Win <= 0 || S <= 0 || Win == S || Hin == S) return 0;
  return (size_t)n * Hin * rz_mid_stride(S);
}

int pg_resize_bilinear_u8(int n, int Hin, int Win, int S, const void* src_base,
                          const int64_t* src_off, const int* kx, const int* bx, int ksx,
                          const int* ky, const int* by, int ksy, void* dst_base,
                          const int64_t* dst_off, void* ws, size_t ws_bytes, void* stream) {
  PG_CHECK_ARG(src_base && src_off && dst_base && dst_off && n > 0 && Hin > 0 && Win > 0 && S > 0,
               "resize_bilinear_u8: bad args");
  PG_CHECK_ARG(n <= 65535, "resize_bilinear_u8: n (%d) > 65535 images per call", n);
  PG_CHECK_ARG(Hin <= (1 << 20) && Win <= (1 << 20) && S <= (1 << 15),
               "resize_bilinear_u8: size out of range (%d x %d -> %d)", Hin, Win, S);
  const bool horiz = Win != S, vert = Hin != S;
  PG_CHECK_ARG(!horiz || (kx && bx && ksx > 0), "resize_bilinear_u8: horizontal tables missing");
  PG_CHECK_ARG(!vert || (ky && by && ksy > 0), "resize_bilinear_u8: vertical tables missing");
  const size_t need = pg_resize_workspace_bytes(n, Hin, Win, S);
  PG_CHECK_ARG(need == 0 || (ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0),
               "resize_bilinear_u8: workspace too small or not 16-byte aligned (%zu < %zu)",
               ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const unsigned char* src = reinterpret_cast<const unsigned char*>(src_base);
  unsigned char* dst = reinterpret_cast<unsigned char*>(dst_base);
  unsigned char* mid = reinterpret_cast<unsigned char*>(ws);
  const size_t rowb = (size_t)3 * S;
  if (!horiz && !vert) {
    const size_t bytes = rowb * S;
    const int blocks = (int)((bytes / 16 + RZ_BLOCK - 1) / RZ_BLOCK);
    PG_KLAUNCH(rz_copy, dim3(blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks, n), dim3(RZ_BLOCK), 0,
               st, src, src_off, dst, dst_off, bytes);
    PG_LAUNCH_CHECK();
    return PG_OK;
  }
  const size_t mid_stride = rz_mid_stride(S), mid_img = mid_stride * Hin;
  if (horiz) {
    const size_t lds = (size_t)RZ_ROWS * 3 * Win + 32;
    if (lds > (size_t)RZ_LDS_MAX) {
      pg_set_error("resize_bilinear_u8: source rows of %d pixels do not fit the LDS staging", Win);
      return PG_ERR_UNSUPPORTED;
    }
    const int P = rz_lanes(ksx);
    // the intermediate, or with the vertical pass skipped the destination itself
    PG_KLAUNCH(rz_horizontal, dim3(pg_cdiv(Hin, RZ_ROWS), n), dim3(RZ_BLOCK), (unsigned)lds, st,
               src, src_off, Hin, Win, S, kx, bx, ksx, vert ? mid : dst,
               vert ? (const int64_t*)nullptr : dst_off, mid_img, vert ? mid_stride : rowb, P);
    PG_LAUNCH_CHECK();
  }
  if (vert) {
    const int P = rz_lanes(ksy);
    const int nchunk = (int)((rowb + 3) / 4);
    const size_t threads = (size_t)S * nchunk * P;
    const dim3 grid((unsigned)((threads + RZ_BLOCK - 1) / RZ_BLOCK), n);
    if (horiz) {
      PG_KLAUNCH(rz_vertical<true>, grid, dim3(RZ_BLOCK), 0, st, mid, (const int64_t*)nullptr,
                 mid_img, mid_stride, S, ky, by, ksy, dst, dst_off, P);
    } else if (rowb % 4 == 0) {   // the source itself: rows 4-byte aligned when 3 S % 4 == 0
      PG_KLAUNCH(rz_vertical<true>, grid, dim3(RZ_BLOCK), 0, st, src, src_off, (size_t)0, rowb, S,
                 ky, by, ksy, dst, dst_off, P);
    } else {
      PG_KLAUNCH(rz_vertical<false>, grid, dim3(RZ_BLOCK), 0, st, src, src_off, (size_t)0, rowb, S,
                 ky, by, ksy, dst, dst_off, P);
    }
    PG_LAUNCH_CHECK();
  }
  return PG_OK;
}

}  // extern "C"
