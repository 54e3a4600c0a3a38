// Multi-scale structural similarity between image pairs (the PGGAN paper's diversity metric,
// DESIGN.md "Validation: MS-SSIM").  Everything here is fp32.
//
//   pg_msssim_scale    one scale of P pairs: the sums over the 3 n^2 window positions of the
//                      ssim and the cs term per pair, and the 2x2-pooled pair for the next
//                      scale, from one read of both images
//   pg_msssim_combine  per pair: clip the five means at 0, raise to the scale weights, multiply
//
// One workgroup of msssim_tile_k: a 32 x 32 tile of window positions of one channel of one
// pair.  It stages the 42 x 44 input tile of both sides once (the tile plus the 10 halo rows and
// columns of the 11-tap window, the column origin a multiple of 32: 16-B loads), quantised and
// shifted by -127.5 there; the 2x2 means of the 32 x 32 inputs under its origin leave from the
// staging registers.  A horizontal pass then filters x, y, x^2, y^2, xy into LDS and a vertical
// pass finishes the five maps in registers, where the two ratios are formed and summed.
// Windows shorter than 11 taps (scales smaller than 11) run the same code with zero taps.
//
// LDS images (64 banks of 4 B; tools/lds_banks.py, msssim()):
//   s_in  [2][42][44]   written and read as 16-B vectors by lanes that walk down the rows: the
//                       pitch 44 = 4 * 11 puts the 16 lanes of a ds_read_b128 group on 16
//                       different 4-bank slots (11 is odd)
//   s_h   [5][42][36]   written as 16-B vectors by the same lanes: pitch 36 = 4 * 9 spreads the
//                       8 lanes of a ds_write_b128 group over the 32 store banks; read by the
//                       vertical pass as consecutive dwords of one row per 32 lanes
//
// Sums over workgroups: every workgroup stores its two fp32 totals into the caller's workspace
// and a launch that follows on the same stream adds a pair's totals in double, in a fixed order.
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

constexpr int MS_C = 3;                        // image channels
constexpr int MS_MAXT = 11;                    // longest window
constexpr int MS_T = 32;                       // tile side, in window positions
constexpr int MS_IH = MS_T + MS_MAXT - 1;      // 42 staged rows
constexpr int MS_IW = 44;                      // 42 staged columns in 11 x 16 B
constexpr int MS_V4 = MS_IW / 4;
constexpr int MS_HP = 36;                      // row pitch of the horizontal sums
constexpr int MS_RP = 48;                      // rows per column group in the horizontal pass' items
constexpr int MS_NQ = 5;                       // x, y, x^2, y^2, xy
constexpr int MS_BLOCK = 256;
constexpr int MS_SCALES = 5;
constexpr float MS_SHIFT = 127.5f;
constexpr float MS_C1 = (0.01f * 255.f) * (0.01f * 255.f);
constexpr float MS_C2 = (0.03f * 255.f) * (0.03f * 255.f);

struct MsTaps {
  float g[MS_MAXT];   // zero from T on
};

// as swd.hip: [-1, 1] -> {0..255}, ties to even
__device__ __forceinline__ float ms_q(float x) {
  return rintf(fminf(fmaxf(fmaf(x, 127.5f, 127.5f), 0.f), 255.f));
}

__device__ __forceinline__ float4 ms_shift(float4 q) {
  return make_float4(q.x - MS_SHIFT, q.y - MS_SHIFT, q.z - MS_SHIFT, q.w - MS_SHIFT);
}

// grid (tiles x * tiles y, 3, P).  a / b: channel 0 of the first pair's two images, the next
// pair img_stride floats on; pa / pb [P][3][S/2][S/2] or both NULL; part [P][3][tiles][2].
// vec: S % 4 == 0 and every pointer and stride 16-B aligned (else the scalar staging).
__global__ __launch_bounds__(MS_BLOCK) void msssim_tile_k(const float* __restrict__ a,
                                                          const float* __restrict__ b,
                                                          size_t img_stride, int S, int n, int ntx,
                                                          MsTaps taps, int quantize, int vec,
                                                          float* __restrict__ pa,
                                                          float* __restrict__ pb,
                                                          float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float s_in[2 * MS_IH * MS_IW];
  __shared__ __attribute__((aligned(16))) float s_h[MS_NQ * MS_IH * MS_HP];
  __shared__ float red[MS_BLOCK / PG_WAVE];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x, c = blockIdx.y, p = blockIdx.z;
  const int ox0 = (tile % ntx) * MS_T, oy0 = (tile / ntx) * MS_T;
  const int So = S >> 1;
  const size_t plane = (size_t)c * S * S;
  const float* src[2] = {a + (size_t)p * img_stride + plane, b + (size_t)p * img_stride + plane};
  float* dst[2] = {pa, pb};
  const size_t oplane = ((size_t)p * MS_C + c) * So * So;

  // ---- staging: two rows per item, so that the 2x2 means leave from the registers
  if (vec) {
    for (int i = tid; i < 2 * (MS_IH / 2) * MS_V4; i += MS_BLOCK) {
      const int img = i / ((MS_IH / 2) * MS_V4), k = i - img * ((MS_IH / 2) * MS_V4);
      const int rp = k / MS_V4, v = k - rp * MS_V4;
      const int gy = oy0 + 2 * rp, gx = ox0 + 4 * v;
      float4 q0 = make_float4(MS_SHIFT, MS_SHIFT, MS_SHIFT, MS_SHIFT), q1 = q0;
      const bool in = gy < S && gx < S;      // S is even and a multiple of 4 here
      if (in) {
        const float* row = src[img] + (size_t)gy * S + gx;
        q0 = *reinterpret_cast<const float4*>(row);
        q1 = *reinterpret_cast<const float4*>(row + S);
        if (quantize) {
          q0.x = ms_q(q0.x); q0.y = ms_q(q0.y); q0.z = ms_q(q0.z); q0.w = ms_q(q0.w);
          q1.x = ms_q(q1.x); q1.y = ms_q(q1.y); q1.z = ms_q(q1.z); q1.w = ms_q(q1.w);
        }
        if (dst[img] && rp < MS_T / 2 && v < MS_T / 4) {   // this tile owns these inputs
          float2 o;
          o.x = (q0.x + q0.y + q1.x + q1.y) * 0.25f;
          o.y = (q0.z + q0.w + q1.z + q1.w) * 0.25f;
          *reinterpret_cast<float2*>(dst[img] + oplane + (size_t)(gy >> 1) * So + (gx >> 1)) = o;
        }
      }
      float* s = &s_in[(img * MS_IH + 2 * rp) * MS_IW + 4 * v];
      *reinterpret_cast<float4*>(s) = ms_shift(q0);
      *reinterpret_cast<float4*>(s + MS_IW) = ms_shift(q1);
    }
  } else {
    for (int i = tid; i < 2 * (MS_IH / 2) * (MS_IW / 2); i += MS_BLOCK) {
      const int img = i / ((MS_IH / 2) * (MS_IW / 2)), k = i - img * ((MS_IH / 2) * (MS_IW / 2));
      const int rp = k / (MS_IW / 2), cp = k - rp * (MS_IW / 2);
      const int gy = oy0 + 2 * rp, gx = ox0 + 2 * cp;
      float q[2][2];
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          float t = MS_SHIFT;
          if (gy + dy < S && gx + dx < S) {
            t = src[img][(size_t)(gy + dy) * S + gx + dx];
            if (quantize) t = ms_q(t);
          }
          q[dy][dx] = t;
        }
      if (dst[img] && rp < MS_T / 2 && cp < MS_T / 2 && gy + 1 < S && gx + 1 < S)
        dst[img][oplane + (size_t)(gy >> 1) * So + (gx >> 1)] =
            (q[0][0] + q[0][1] + q[1][0] + q[1][1]) * 0.25f;
      float* s = &s_in[(img * MS_IH + 2 * rp) * MS_IW + 2 * cp];
      s[0] = q[0][0] - MS_SHIFT;
      s[1] = q[0][1] - MS_SHIFT;
      s[MS_IW] = q[1][0] - MS_SHIFT;
      s[MS_IW + 1] = q[1][1] - MS_SHIFT;
    }
  }
  __syncthreads();

  // ---- horizontal pass: item = (row r, columns 4 j .. 4 j + 3), consecutive lanes walk down r
  // (rows padded to 48 per column group: a lane's row is its lane number mod 16 plus a multiple
  // of 16, which is what keeps the 16 lanes of a read group on different bank slots)
  for (int i = tid; i < MS_RP * (MS_T / 4); i += MS_BLOCK) {
    const int j = i / MS_RP, r = i - j * MS_RP;
    if (r >= MS_IH) continue;
    float xa[16], xb[16];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float4 u = *reinterpret_cast<const float4*>(&s_in[r * MS_IW + 4 * (j + v)]);
      const float4 w = *reinterpret_cast<const float4*>(&s_in[(MS_IH + r) * MS_IW + 4 * (j + v)]);
      xa[4 * v] = u.x; xa[4 * v + 1] = u.y; xa[4 * v + 2] = u.z; xa[4 * v + 3] = u.w;
      xb[4 * v] = w.x; xb[4 * v + 1] = w.y; xb[4 * v + 2] = w.z; xb[4 * v + 3] = w.w;
    }
    float acc[MS_NQ][4];
#pragma unroll
    for (int q = 0; q < MS_NQ; ++q)
#pragma unroll
      for (int o = 0; o < 4; ++o) acc[q][o] = 0.f;
#pragma unroll
    for (int e = 0; e < MS_MAXT + 3; ++e) {
      const float va = xa[e], vb = xb[e];
      const float aa = va * va, bb = vb * vb, ab = va * vb;
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int t = e - o;
        if (t < 0 || t >= MS_MAXT) continue;
        const float g = taps.g[t];
        acc[0][o] = fmaf(g, va, acc[0][o]);
        acc[1][o] = fmaf(g, vb, acc[1][o]);
        acc[2][o] = fmaf(g, aa, acc[2][o]);
        acc[3][o] = fmaf(g, bb, acc[3][o]);
        acc[4][o] = fmaf(g, ab, acc[4][o]);
      }
    }
#pragma unroll
    for (int q = 0; q < MS_NQ; ++q)
      *reinterpret_cast<float4*>(&s_h[(q * MS_IH + r) * MS_HP + 4 * j]) =
          make_float4(acc[q][0], acc[q][1], acc[q][2], acc[q][3]);
  }
  __syncthreads();

  // ---- vertical pass: thread = (column ox, rows 4 rg .. 4 rg + 3), then the two ratios
  const int ox = tid & 31, rg = tid >> 5;
  float f[MS_NQ][4];
#pragma unroll
  for (int q = 0; q < MS_NQ; ++q) {
    float h[MS_MAXT + 3];
#pragma unroll
    for (int e = 0; e < MS_MAXT + 3; ++e) h[e] = s_h[(q * MS_IH + 4 * rg + e) * MS_HP + ox];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      float s = 0.f;
#pragma unroll
      for (int t = 0; t < MS_MAXT; ++t) s = fmaf(taps.g[t], h[o + t], s);
      f[q][o] = s;
    }
  }
  float sum_ssim = 0.f, sum_cs = 0.f;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    // positions >= n are evaluated like the others (their inputs are staged zeros or real
    // pixels: finite, and both denominators are >= c1, c2 up to rounding) and left out of the
    // sums: no branch around the divisions
    const bool live = oy0 + 4 * rg + o < n && ox0 + ox < n;
    const float A = f[0][o], B = f[1][o];
    // the variances are those of the shifted images; the means get the shift back
    const float s11 = fmaf(-A, A, f[2][o]), s22 = fmaf(-B, B, f[3][o]), s12 = fmaf(-A, B, f[4][o]);
    const float v1 = __fadd_rn(__fmul_rn(2.f, s12), MS_C2);
    const float v2 = __fadd_rn(__fadd_rn(s11, s22), MS_C2);
    const float mu1 = A + MS_SHIFT, mu2 = B + MS_SHIFT;
    const float lnum = __fadd_rn(__fmul_rn(2.f, __fmul_rn(mu1, mu2)), MS_C1);
    const float lden = __fadd_rn(__fadd_rn(__fmul_rn(mu1, mu1), __fmul_rn(mu2, mu2)), MS_C1);
    const float cs = v1 / v2;
    sum_cs += live ? cs : 0.f;
    sum_ssim += live ? (lnum / lden) * cs : 0.f;
  }
  const float t0 = block_sum(sum_ssim, red);
  const float t1 = block_sum(sum_cs, red);
  if (tid == 0) {
    float* o = part + (((size_t)p * MS_C + c) * gridDim.x + tile) * 2;
    o[0] = t0;
    o[1] = t1;
  }
}

// one workgroup per pair: its np = 3 * tiles partial pairs in double, in a fixed order
__global__ __launch_bounds__(MS_BLOCK) void msssim_fin_k(const float* __restrict__ part, int np,
                                                         float* __restrict__ sums) {
  __shared__ double red[MS_BLOCK];
  const float* pp = part + (size_t)blockIdx.x * np * 2;
  for (int k = 0; k < 2; ++k) {
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += MS_BLOCK) s += (double)pp[2 * i + k];
    __syncthreads();
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = MS_BLOCK / 2; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) sums[(size_t)blockIdx.x * 2 + k] = (float)red[0];
  }
}

struct MsCounts {
  double n[MS_SCALES];
};

// sums [5][P][2] = (sum ssim, sum cs) per scale and pair
__global__ __launch_bounds__(MS_BLOCK) void msssim_combine_k(const float* __restrict__ sums, int P,
                                                             MsCounts cnt, float* __restrict__ out) {
  const double w[MS_SCALES] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  const int p = blockIdx.x * MS_BLOCK + threadIdx.x;
  if (p >= P) return;
  double v = 1.0;
  for (int s = 0; s < MS_SCALES; ++s) {
    const int k = s == MS_SCALES - 1 ? 0 : 1;
    const double m = (double)sums[((size_t)s * P + p) * 2 + k] / cnt.n[s];
    v *= pow(m > 0.0 ? m : 0.0, w[s]);
  }
  out[p] = (float)v;
}

bool ms_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

size_t pg_msssim_workspace_bytes(int P, int S, int T) {
  if (P < 1 || T < 1 || T > S) return 0;
  const size_t nt = (size_t)pg_cdiv(S - T + 1, MS_T);
  return (size_t)P * MS_C * nt * nt * 2 * sizeof(float);
}

int pg_msssim_scale(int P, int S, int T, const float* taps, const float* a, const float* b,
                    size_t img_stride, int quantize, float* sums, float* pool_a, float* pool_b,
                    void* ws, size_t ws_bytes, void* stream) {
  PG_CHECK_ARG(taps && a && b && sums && ws, "msssim_scale: null pointer");
  PG_CHECK_ARG((pool_a == nullptr) == (pool_b == nullptr),
               "msssim_scale: pool_a and pool_b go together");
  PG_CHECK_ARG(P > 0 && P <= 65535, "msssim_scale: P (%d) must be in [1, 65535]", P);
  PG_CHECK_ARG(S > 0 && S <= 16384, "msssim_scale: S (%d) must be in [1, 16384]", S);
  PG_CHECK_ARG(T >= 1 && T <= MS_MAXT && T <= S,
               "msssim_scale: T (%d) must be in [1, min(%d, S = %d)]", T, MS_MAXT, S);
  PG_CHECK_ARG(!pool_a || S % 2 == 0, "msssim_scale: pooled outputs need an even S (got %d)", S);
  PG_CHECK_ARG(img_stride >= (size_t)MS_C * S * S, "msssim_scale: img_stride (%zu) < 3 S^2",
               img_stride);
  const int n = S - T + 1, nt = pg_cdiv(n, MS_T);
  // a tile pools the inputs under its origin: the tiles must reach the last row and column
  PG_CHECK_ARG(!pool_a || nt * MS_T >= S,
               "msssim_scale: %d tiles of %d do not cover S = %d (pooled outputs)", nt, MS_T, S);
  PG_CHECK_ARG(ws_bytes >= pg_msssim_workspace_bytes(P, S, T),
               "msssim_scale: workspace of %zu B, %zu needed", ws_bytes,
               pg_msssim_workspace_bytes(P, S, T));
  MsTaps tp;
  for (int t = 0; t < MS_MAXT; ++t) tp.g[t] = t < T ? taps[t] : 0.f;
  const int vec = S % 4 == 0 && img_stride % 4 == 0 && ms_al16(a) && ms_al16(b) &&
                  (!pool_a || (ms_al16(pool_a) && ms_al16(pool_b)));
  hipStream_t st = (hipStream_t)stream;
  float* part = reinterpret_cast<float*>(ws);
  PG_KLAUNCH(msssim_tile_k, dim3(nt * nt, MS_C, P), dim3(MS_BLOCK), 0, st, a, b, img_stride, S, n,
             nt, tp, quantize, vec, pool_a, pool_b, part);
  PG_LAUNCH_CHECK();
  PG_KLAUNCH(msssim_fin_k, dim3(P), dim3(MS_BLOCK), 0, st, part, MS_C * nt * nt, sums);
  PG_LAUNCH_CHECK();
  return PG_OK;
}

int pg_msssim_combine(int P, const float* sums, const long long* counts, float* out, void* stream) {
  PG_CHECK_ARG(sums && counts && out, "msssim_combine: null pointer");
  PG_CHECK_ARG(P > 0, "msssim_combine: P (%d) must be positive", P);
  MsCounts c;
  for (int s = 0; s < MS_SCALES; ++s) {
    PG_CHECK_ARG(counts[s] > 0, "msssim_combine: count %d (%lld) must be positive", s, counts[s]);
    c.n[s] = (double)counts[s];
  }
  PG_KLAUNCH(msssim_combine_k, dim3(pg_cdiv(P, MS_BLOCK)), dim3(MS_BLOCK), 0, (hipStream_t)stream,
             sums, P, c, out);
  PG_LAUNCH_CHECK();
  return PG_OK;
}

}  // extern "C"
