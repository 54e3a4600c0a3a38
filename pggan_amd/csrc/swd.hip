// Sliced Wasserstein distance on Laplacian-pyramid patches (the PGGAN paper's validation
// metric, DESIGN.md "Validation: sliced Wasserstein distance").  Everything here is fp32.
//
//   pg_swd_pyr_down     G_{l+1} = every second sample of (k (x) k) * G_l, k = [1 4 6 4 1] / 16,
//                       mirror boundary (no repeated edge sample); one read, one write
//   pg_swd_descriptors  7x7x3 patches of L_l = G_l - up(G_{l+1}) gathered at given centres; the
//                       up-sampling is evaluated at the 49 pixels of a patch only (polyphase
//                       taps of the zero-insert + 4 k (x) k filter), L_l is never stored
//   pg_swd_stats        per-channel mean and 1 / population std over all descriptors (two pass)
//   pg_swd_project      normalised descriptors times the direction matrix, one row per direction
//   pg_swd_l1           sum |a - b| over the sorted projections
//
// Sums over workgroups: every workgroup stores its fp32 partials into the stream's reduction
// scratch (behind the ticket header, which these kernels never touch) and a one-workgroup
// launch that follows on the same stream adds them in double, in a fixed order.
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

constexpr int SWD_C = 3;                  // image channels
constexpr int SWD_NH = 7;                 // patch side
constexpr int SWD_PP = SWD_NH * SWD_NH;   // 49 values per channel
constexpr int SWD_D = SWD_C * SWD_PP;     // 147 values per descriptor

// the paper evaluates 8-bit images: [-1, 1] -> {0..255}, ties to even
__device__ __forceinline__ float swd_q(float x) {
  return rintf(fminf(fmaxf(fmaf(x, 127.5f, 127.5f), 0.f), 255.f));
}

// mirror without repeating the edge sample; then clamped, so that the positions a partial tile
// stages for outputs it never stores stay inside the image
__device__ __forceinline__ int swd_mirror(int j, int n) {
  j = j < 0 ? -j : j;
  j = j > n - 1 ? 2 * (n - 1) - j : j;
  return j < 0 ? 0 : j;
}

// ---- pyr_down ---------------------------------------------------------------------------
// One workgroup: a 32 x 32 output tile of one image plane.  The 67 x 72 input tile (rows
// 2 oy0 - 2 .., columns 2 ox0 - 4 .., the column origin kept 16-B aligned) is staged once with
// 16-B loads, mirror indices resolved there; a horizontal pass writes 67 x 32 row sums, a
// vertical pass the outputs.  The horizontal pass reads 8-B pairs (lane stride 2 dwords: one
// ds_read_b64 covers the 64 banks without a conflict), the vertical pass consecutive dwords.
constexpr int PD_T = 32;
constexpr int PD_IH = 2 * PD_T + 3;       // 67 staged rows
constexpr int PD_IW = 2 * PD_T + 8;       // 72 staged columns (18 x 16 B)
constexpr int PD_V4 = PD_IW / 4;
constexpr int PD_BLOCK = 256;

__global__ __launch_bounds__(PD_BLOCK) void swd_pyr_down_k(const float* __restrict__ x,
                                                           float* __restrict__ y, int H, int W,
                                                           int quantize) {
  __shared__ __attribute__((aligned(16))) float s_in[PD_IH * PD_IW];
  __shared__ float s_h[PD_IH * PD_T];
  const int tid = threadIdx.x;
  const int Ho = H >> 1, Wo = W >> 1;
  const int ox0 = blockIdx.x * PD_T, oy0 = blockIdx.y * PD_T;
  const float* px = x + (size_t)blockIdx.z * H * W;
  float* py = y + (size_t)blockIdx.z * Ho * Wo;
  const int gx0 = 2 * ox0 - 4, gy0 = 2 * oy0 - 2;

  for (int i = tid; i < PD_IH * PD_V4; i += PD_BLOCK) {
    const int r = i / PD_V4, v = i - r * PD_V4;
    const int gy = swd_mirror(gy0 + r, H);
    const int gx = gx0 + 4 * v;
    const float* row = px + (size_t)gy * W;
    float4 q;
    if (gx >= 0 && gx + 3 < W) {
      q = *reinterpret_cast<const float4*>(row + gx);
    } else {
      q.x = row[swd_mirror(gx, W)];
      q.y = row[swd_mirror(gx + 1, W)];
      q.z = row[swd_mirror(gx + 2, W)];
      q.w = row[swd_mirror(gx + 3, W)];
    }
    if (quantize) {
      q.x = swd_q(q.x); q.y = swd_q(q.y); q.z = swd_q(q.z); q.w = swd_q(q.w);
    }
    *reinterpret_cast<float4*>(&s_in[r * PD_IW + 4 * v]) = q;
  }
  __syncthreads();
  // output column ox reads input columns 2 ox - 2 .. 2 ox + 2 = staged columns 2 ox + 2 .. + 6
  for (int i = tid; i < PD_IH * PD_T; i += PD_BLOCK) {
    const int r = i >> 5, ox = i & 31;
    const float* p = &s_in[r * PD_IW + 2 * ox + 2];
    const float2 a = *reinterpret_cast<const float2*>(p);
    const float2 b = *reinterpret_cast<const float2*>(p + 2);
    const float c = p[4];
    s_h[i] = ((a.x + c) + 4.f * (a.y + b.y) + 6.f * b.x) * 0.0625f;
  }
  __syncthreads();
  for (int i = tid; i < PD_T * PD_T; i += PD_BLOCK) {
    const int oy = i >> 5, ox = i & 31;
    const float* p = &s_h[(2 * oy) * PD_T + ox];
    const float v = ((p[0] + p[4 * PD_T]) + 4.f * (p[PD_T] + p[3 * PD_T]) + 6.f * p[2 * PD_T]) * 0.0625f;
    if (oy0 + oy < Ho && ox0 + ox < Wo) py[(size_t)(oy0 + oy) * Wo + ox0 + ox] = v;
  }
}

// ---- descriptors ------------------------------------------------------------------------
// 1-D polyphase taps of up() at output index o over n coarse samples: the three coarse
// indices i - 1, i, i + 1 (i = o / 2; -1 -> 1 and n -> n - 1, the mirror of the zero-inserted
// signal, which is why the two edges differ) with weights (1 6 1) / 8 at even o, (0 4 4) / 8
// at odd o.
struct Taps {
  int i[3];
  float w[3];
};
__device__ __forceinline__ Taps swd_taps(int o, int n) {
  Taps t;
  const int c = o >> 1;
  t.i[0] = c - 1 < 0 ? 1 : c - 1;
  t.i[1] = c;
  t.i[2] = c + 1 > n - 1 ? n - 1 : c + 1;
  if (o & 1) { t.w[0] = 0.f;    t.w[1] = 0.5f;  t.w[2] = 0.5f; }
  else       { t.w[0] = 0.125f; t.w[1] = 0.75f; t.w[2] = 0.125f; }
  return t;
}

// one wave per patch, four patches per workgroup
constexpr int DS_BLOCK = 256;
__global__ __launch_bounds__(DS_BLOCK) void swd_desc_k(const float* __restrict__ fine,
                                                       const float* __restrict__ coarse,
                                                       const int* __restrict__ pos,
                                                       float* __restrict__ desc, int S, int K,
                                                       long long npatch, int quantize) {
  const long long p = (long long)blockIdx.x * (DS_BLOCK / PG_WAVE) + (threadIdx.x >> 6);
  if (p >= npatch) return;
  const int lane = threadIdx.x & 63;
  const long long b = p / K;
  // centres outside [3, S - 3) are refused by the caller; the clamp keeps a stray one in bounds
  const int cy = min(max(pos[2 * p], 3), S - 4), cx = min(max(pos[2 * p + 1], 3), S - 4);
  const int Sc = S >> 1;
  for (int e = lane; e < SWD_D; e += PG_WAVE) {
    const int c = e / SWD_PP, r = e - c * SWD_PP;
    const int dy = r / SWD_NH, dx = r - dy * SWD_NH;
    const int yy = cy + dy - 3, xx = cx + dx - 3;
    float v = fine[((size_t)(b * SWD_C + c) * S + yy) * S + xx];
    if (quantize) v = swd_q(v);
    if (coarse) {
      const float* pc = coarse + (size_t)(b * SWD_C + c) * Sc * Sc;
      const Taps ty = swd_taps(yy, Sc), tx = swd_taps(xx, Sc);
      float u = 0.f;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float* row = pc + (size_t)ty.i[a] * Sc;
        const float h = tx.w[0] * row[tx.i[0]] + tx.w[1] * row[tx.i[1]] + tx.w[2] * row[tx.i[2]];
        u += ty.w[a] * h;
      }
      v -= u;
    }
    desc[(size_t)p * SWD_D + e] = v;
  }
}

// ---- stats ------------------------------------------------------------------------------
constexpr int RD_BLOCK = 256;
constexpr int RD_MAX_BLOCKS = 4096;

// grid-stride over the n * 147 values; PASS 0: per-channel sums, PASS 1: per-channel sums of
// (x - mean)^2; the workgroup's three fp32 totals go to part[bid * 3 + c]
template <int PASS>
__global__ __launch_bounds__(RD_BLOCK) void swd_stats_part_k(const float* __restrict__ desc,
                                                             size_t total,
                                                             const float* __restrict__ mean3,
                                                             float* __restrict__ part) {
  __shared__ float red[RD_BLOCK / PG_WAVE];
  float m[SWD_C] = {0.f, 0.f, 0.f};
  if (PASS == 1) { m[0] = mean3[0]; m[1] = mean3[1]; m[2] = mean3[2]; }
  float s[SWD_C] = {0.f, 0.f, 0.f};
  const size_t stride = (size_t)gridDim.x * RD_BLOCK;
  for (size_t i = (size_t)blockIdx.x * RD_BLOCK + threadIdx.x; i < total; i += stride) {
    const int c = (int)(i % SWD_D) / SWD_PP;
    float v = desc[i];
    if (PASS == 1) { v -= (c == 0 ? m[0] : c == 1 ? m[1] : m[2]); v *= v; }
    s[0] += c == 0 ? v : 0.f;
    s[1] += c == 1 ? v : 0.f;
    s[2] += c == 2 ? v : 0.f;
  }
#pragma unroll
  for (int c = 0; c < SWD_C; ++c) {
    const float t = block_sum(s[c], red);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * SWD_C + c] = t;
  }
}

// block-wide sum in double, fixed order; result valid in thread 0
__device__ __forceinline__ double swd_block_sum_d(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int st = RD_BLOCK / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  return red[0];
}

// one workgroup: the partials of nb workgroups in double.  PASS 0: mean3 = sum / count;
// PASS 1: rstd3 = 1 / sqrt(sum / count)
template <int PASS>
__global__ __launch_bounds__(RD_BLOCK) void swd_stats_fin_k(const float* __restrict__ part, int nb,
                                                            double count, float* __restrict__ out3) {
  __shared__ double red[RD_BLOCK];
  for (int c = 0; c < SWD_C; ++c) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += RD_BLOCK) s += (double)part[(size_t)b * SWD_C + c];
    const double t = swd_block_sum_d(s, red);
    if (threadIdx.x == 0) out3[c] = PASS == 0 ? (float)(t / count) : (float)(1.0 / sqrt(t / count));
  }
}

// ---- project ----------------------------------------------------------------------------
// proj[p][i] = sum_j ((desc[i][j] - mean[c(j)]) rstd[c(j)]) dirs[j][p].  One workgroup: 64
// descriptors x 64 directions, a 4 x 4 register tile per thread, the 147 terms in three chunks
// of one channel each (so the normalisation constants are uniform per chunk), fp32 FMA.
// A is staged [m][49]: lanes tm = 0..15 read rows tm + 16 a, 49 dwords apart (odd: 16 distinct
// banks, the other lanes of the group read the same addresses); B is staged [k][64] and read
// as one 16-B vector per k.
constexpr int PJ_TM = 64, PJ_TN = 64, PJ_BLOCK = 256;

__global__ __launch_bounds__(PJ_BLOCK) void swd_project_k(const float* __restrict__ desc,
                                                          const float* __restrict__ mean3,
                                                          const float* __restrict__ rstd3,
                                                          const float* __restrict__ dirs,
                                                          float* __restrict__ proj, long long n,
                                                          int P, long long proj_stride) {
  __shared__ float As[PJ_TM * SWD_PP];
  __shared__ __attribute__((aligned(16))) float Bs[SWD_PP * PJ_TN];
  const int tid = threadIdx.x;
  const int tm = tid & 15, tn = tid >> 4;
  const long long i0 = (long long)blockIdx.x * PJ_TM;
  const int p0 = blockIdx.y * PJ_TN;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[a][q] = 0.f;

  for (int c = 0; c < SWD_C; ++c) {
    const float mu = mean3[c], rs = rstd3[c];
    __syncthreads();
    for (int idx = tid; idx < PJ_TM * SWD_PP; idx += PJ_BLOCK) {
      const int m = idx / SWD_PP, k = idx - m * SWD_PP;
      const long long i = i0 + m;
      As[idx] = i < n ? (desc[(size_t)i * SWD_D + c * SWD_PP + k] - mu) * rs : 0.f;
    }
    for (int idx = tid; idx < SWD_PP * PJ_TN; idx += PJ_BLOCK) {
      const int k = idx >> 6, q = idx & 63;
      Bs[idx] = p0 + q < P ? dirs[(size_t)(c * SWD_PP + k) * P + p0 + q] : 0.f;
    }
    __syncthreads();
#pragma unroll 7
    for (int k = 0; k < SWD_PP; ++k) {
      const float4 bv = *reinterpret_cast<const float4*>(&Bs[k * PJ_TN + tn * 4]);
      const float b[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const float av = As[(tm + 16 * a) * SWD_PP + k];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[a][q] = fmaf(av, b[q], acc[a][q]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = p0 + tn * 4 + q;
    if (p >= P) continue;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const long long i = i0 + tm + 16 * a;
      if (i < n) proj[(size_t)p * proj_stride + i] = acc[a][q];
    }
  }
}

// ---- l1 ---------------------------------------------------------------------------------
// grid (chunks, P): workgroup (bx, p) sums |a - b| over its share of row p
__global__ __launch_bounds__(RD_BLOCK) void swd_l1_part_k(const float* __restrict__ a,
                                                          const float* __restrict__ b, long long n,
                                                          long long stride, int vec,
                                                          float* __restrict__ part) {
  __shared__ float red[RD_BLOCK / PG_WAVE];
  const float* ra = a + (size_t)blockIdx.y * stride;
  const float* rb = b + (size_t)blockIdx.y * stride;
  const long long step = (long long)gridDim.x * RD_BLOCK;
  const long long t0 = (long long)blockIdx.x * RD_BLOCK + threadIdx.x;
  float s = 0.f;
  long long done = 0;
  if (vec) {   // rows 16-B aligned: four values per load
    const long long n4 = n >> 2;
    for (long long i = t0; i < n4; i += step) {
      const float4 u = *reinterpret_cast<const float4*>(ra + 4 * i);
      const float4 w = *reinterpret_cast<const float4*>(rb + 4 * i);
      s += (fabsf(u.x - w.x) + fabsf(u.y - w.y)) + (fabsf(u.z - w.z) + fabsf(u.w - w.w));
    }
    done = n4 << 2;
  }
  for (long long i = done + t0; i < n; i += step) s += fabsf(ra[i] - rb[i]);
  const float t = block_sum(s, red);
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

__global__ __launch_bounds__(RD_BLOCK) void swd_l1_fin_k(const float* __restrict__ part, int np,
                                                         float* __restrict__ out) {
  __shared__ double red[RD_BLOCK];
  double s = 0.0;
  for (int b = threadIdx.x; b < np; b += RD_BLOCK) s += (double)part[b];
  const double t = swd_block_sum_d(s, red);
  if (threadIdx.x == 0) out[0] = (float)((double)out[0] + t);
}

bool swd_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
bool swd_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int pg_swd_pyr_down(int B, int H, int W, const float* x, int quantize, float* y, void* stream) {
  PG_CHECK_ARG(x && y, "swd_pyr_down: null pointer");
  PG_CHECK_ARG(B > 0 && B * SWD_C <= 65535, "swd_pyr_down: B (%d) must be in [1, %d]", B,
               65535 / SWD_C);
  PG_CHECK_ARG(H == W && H >= 32 && swd_pow2(H),
               "swd_pyr_down: H = W = a power of two >= 32 (got %d x %d)", H, W);
  PG_CHECK_ARG(swd_al16(x) && swd_al16(y), "swd_pyr_down: x and y must be 16-byte aligned");
  const int nt = pg_cdiv(W / 2, PD_T);
  PG_KLAUNCH(swd_pyr_down_k, dim3(nt, nt, B * SWD_C), dim3(PD_BLOCK), 0, (hipStream_t)stream, x, y,
             H, W, quantize);
  PG_LAUNCH_CHECK();
  return PG_OK;
}

int pg_swd_descriptors(int B, int S, const float* fine, const float* coarse, int K, const int* pos,
                       int quantize, float* desc, void* stream) {
  PG_CHECK_ARG(fine && pos && desc, "swd_descriptors: null pointer");
  PG_CHECK_ARG(B > 0 && K > 0, "swd_descriptors: B (%d) and K (%d) must be positive", B, K);
  PG_CHECK_ARG(S >= 16 && swd_pow2(S), "swd_descriptors: S (%d) must be a power of two >= 16", S);
  const long long np = (long long)B * K;
  const long long nblk = (np + DS_BLOCK / PG_WAVE - 1) / (DS_BLOCK / PG_WAVE);
  PG_CHECK_ARG(nblk <= 0x7fffffffLL, "swd_descriptors: too many patches (%lld)", np);
  PG_KLAUNCH(swd_desc_k, dim3((unsigned)nblk), dim3(DS_BLOCK), 0, (hipStream_t)stream, fine, coarse,
             pos, desc, S, K, np, quantize);
  PG_LAUNCH_CHECK();
  return PG_OK;
}

int pg_swd_stats(size_t n, const float* desc, float* mean3, float* rstd3, void* scratch,
                 void* stream) {
  PG_CHECK_ARG(desc && mean3 && rstd3 && scratch, "swd_stats: null pointer");
  PG_CHECK_ARG(n > 0 && n <= ((size_t)1 << 40), "swd_stats: n (%zu) out of range", n);
  const size_t total = n * SWD_D;
  size_t nbz = (total + (size_t)RD_BLOCK * 16 - 1) / ((size_t)RD_BLOCK * 16);
  const int nb = (int)(nbz < 1 ? 1 : nbz > RD_MAX_BLOCKS ? RD_MAX_BLOCKS : nbz);
  PG_CHECK_ARG(pg_det_fits(nb, SWD_C), "swd_stats: scratch too small");
  float* part = pg_scratch_partials(reinterpret_cast<float*>(scratch));
  const double count = (double)n * SWD_PP;
  hipStream_t st = (hipStream_t)stream;
  PG_KLAUNCH(swd_stats_part_k<0>, dim3(nb), dim3(RD_BLOCK), 0, st, desc, total, mean3, part);
  PG_LAUNCH_CHECK();
  PG_KLAUNCH(swd_stats_fin_k<0>, dim3(1), dim3(RD_BLOCK), 0, st, part, nb, count, mean3);
  PG_LAUNCH_CHECK();
  PG_KLAUNCH(swd_stats_part_k<1>, dim3(nb), dim3(RD_BLOCK), 0, st, desc, total, mean3, part);
  PG_LAUNCH_CHECK();
  PG_KLAUNCH(swd_stats_fin_k<1>, dim3(1), dim3(RD_BLOCK), 0, st, part, nb, count, rstd3);
  PG_LAUNCH_CHECK();
  return PG_OK;
}

int pg_swd_project(size_t n, const float* desc, const float* mean3, const float* rstd3, int P,
                   const float* dirs, float* proj, size_t proj_stride, void* stream) {
  PG_CHECK_ARG(desc && mean3 && rstd3 && dirs && proj, "swd_project: null pointer");
  PG_CHECK_ARG(n > 0 && P > 0, "swd_project: n (%zu) and P (%d) must be positive", n, P);
  PG_CHECK_ARG(proj_stride >= n, "swd_project: proj_stride (%zu) < n (%zu)", proj_stride, n);
  const size_t gx = (n + PJ_TM - 1) / PJ_TM;
  const int gy = pg_cdiv(P, PJ_TN);
  PG_CHECK_ARG(gx <= 0x7fffffffu && gy <= 65535, "swd_project: n (%zu) or P (%d) too large", n, P);
  PG_KLAUNCH(swd_project_k, dim3((unsigned)gx, gy), dim3(PJ_BLOCK), 0, (hipStream_t)stream, desc,
             mean3, rstd3, dirs, proj, (long long)n, P, (long long)proj_stride);
  PG_LAUNCH_CHECK();
  return PG_OK;
}

int pg_swd_l1(int P, size_t n, const float* a, const float* b, size_t stride, float* out,
              void* scratch, void* stream) {
  PG_CHECK_ARG(a && b && out && scratch, "swd_l1: null pointer");
  PG_CHECK_ARG(P > 0 && P <= 65535 && n > 0, "swd_l1: P (%d) in [1, 65535], n (%zu) > 0", P, n);
  PG_CHECK_ARG(stride >= n, "swd_l1: stride (%zu) < n (%zu)", stride, n);
  size_t gxz = (n + (size_t)RD_BLOCK * 8 - 1) / ((size_t)RD_BLOCK * 8);
  const int gx = (int)(gxz < 1 ? 1 : gxz > 64 ? 64 : gxz);
  PG_CHECK_ARG(pg_det_fits((size_t)gx * P, 1), "swd_l1: scratch too small");
  float* part = pg_scratch_partials(reinterpret_cast<float*>(scratch));
  const int vec = swd_al16(a) && swd_al16(b) && stride % 4 == 0;
  hipStream_t st = (hipStream_t)stream;
  PG_KLAUNCH(swd_l1_part_k, dim3(gx, P), dim3(RD_BLOCK), 0, st, a, b, (long long)n,
             (long long)stride, vec, part);
  PG_LAUNCH_CHECK();
  PG_KLAUNCH(swd_l1_fin_k, dim3(1), dim3(RD_BLOCK), 0, st, part, gx * P, out);
  PG_LAUNCH_CHECK();
  return PG_OK;
}

}  // extern "C"
