// Azimuthally averaged power spectrum of images (DESIGN.md "Validation: power spectrum").
// Everything here is fp32 but the last sum over workgroups, which is taken in double.
//
//   pg_spectrum_profile   per image: luma of the 8-bit image, its unnormalised 2-D DFT, and
//                         |F|^2 summed over the integer radius bins 0 .. R/2
//
// The transform is a real 2-D FFT held in LDS.  Two image rows a, b travel as one complex line
// z = a + i b through a length-R complex FFT; Z(v) and Z(R - v) give the two rows' half spectra
// A(v) = (Z(v) + conj Z(R-v)) / 2, B(v) = (Z(v) - conj Z(R-v)) / 2i, v = 0 .. R/2.  The R/2 + 1
// columns of the half spectrum are then transformed along the rows, and |F|^2 leaves for the
// bins from the registers: the complex 2-D spectrum is never written to memory.  Column v
// stands for v and -v (weight 2) except v = 0 and v = R/2 (= -R/2), which the plane holds once.
//
// One FFT: in-place decimation in frequency, two radix-2 stages per pass over LDS (a radix-4
// butterfly in registers; one radix-2 pass last when log2 R is odd), output in bit-reversed
// order: the value of frequency f lies at position brev(f).  Twiddles exp(-2 pi i j / R),
// j < R/2, are a per-workgroup LDS table filled by sincospif(-j / (R/2)) -- exact rational
// arguments; the factor -i between the two butterflies of the first stage is a swap.
//
// Launch shapes:
//   R <= 64   spectrum_small_k, one workgroup per image: rows, the half spectrum [R/2+1][R]
//             beside them in LDS, columns, bins; writes prof itself (bins summed in double)
//   R >= 128  spectrum_rows_k: a workgroup takes 2 NL rows (NL = min(8, 4096 / R) lines) and
//             stores their half spectra transposed, T[v][row] complex, into the workspace:
//             NL neighbouring lanes store the 2 NL rows of one v, 16 B each, 64 or 128 B
//             contiguous.  spectrum_cols_k: a workgroup loads NL contiguous lines T[v][0..R),
//             transforms them and writes its K + 1 fp32 bin sums to the workspace;
//             spectrum_fin_k adds an image's partials in double in workgroup order.
//             Images go through in chunks whose T fits 32 MB: the workspace stays that small
//             and the column pass reads what the row pass just wrote.
//
// Bins without atomics: for a fixed column v the bin of (u, v) does not fall as |u| grows, so
// bin k of column v is the run umax(k-1) < |u| <= umax(k) with umax(k) = isqrt(k^2 + k - v^2)
// (a float sqrt corrected in integers: exact).  Thread k walks its run in every line of the
// workgroup in a fixed order: bitwise repeatable, and an image's result depends neither on B
// nor on its place in the batch.
//
// LDS image (tools/lds_banks.py, spectrum(); an 8-B element's bank pair is its index mod 32 for
// ds_read_b64, mod 16 for ds_write_b64): a line is R complex elements, element p at
// p + (p >> 5) (one element of padding per 32), lines R + R/32 + 1 apart.  LDS cycles per lane
// group, reads / writes (1 = conflict-free):
//   quarter-span q >= 32   1 / 1: a group takes consecutive elements of one 32-aligned run
//   q = 16                 2 / 1   } a group takes runs of q elements 4 q apart; the padding
//   q = 8                  4 / 2   } moves every 32 / 4q-th run by one bank pair only
//   q = 4                  4 / 4   }
//   q = 2                  2 / 4 (4 / 4 unpadded)
//   q = 1                  1 / 2 (4 / 4 unpadded): elements 4 t land on 4 (t & 7) + (t >> 3)
//   last radix-2 pass      1 / 2 (2 / 2 unpadded)
//   bit-reversed reads of the transposing store: consecutive frequencies lie R/2, R/4 ..
//     elements apart, 27 .. 31 cycles unpadded; the padding spreads them and the odd line
//     pitch keeps the NL lines of neighbouring lanes apart: 1.5 (R = 1024) .. 2.4
//   At R = 1024 two of the five passes are conflict-free and the q = 4 pass is the worst.
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

constexpr int SP_BLOCK = 256;
constexpr int SP_MINR = 8, SP_MAXR = 1024;
constexpr int SP_ONE = 64;                   // largest R of the one-launch form
constexpr int SP_LINE_ELEMS = 4096;          // complex elements a workgroup of the two-launch form holds
constexpr int SP_MAXNL = 8;                  // and its most lines
constexpr size_t SP_CHUNK_BYTES = (size_t)32 << 20;   // of T per chunk of images

__host__ __device__ constexpr int sp_pitch(int R) { return R + (R >> 5) + 1; }
__host__ __device__ constexpr int sp_lines(int R) {
  return SP_LINE_ELEMS / R < SP_MAXNL ? SP_LINE_ELEMS / R : SP_MAXNL;
}
__device__ __forceinline__ int sp_at(int p) { return p + (p >> 5); }

constexpr int SP_BUF = SP_MAXNL * sp_pitch(512);                  // 4232 elements, 33.1 KB
static_assert(sp_lines(1024) * sp_pitch(1024) <= SP_BUF && sp_lines(256) * sp_pitch(256) <= SP_BUF &&
              sp_lines(128) * sp_pitch(128) <= SP_BUF, "the two-launch line buffer");
constexpr int SP_SMALL_A = (SP_ONE / 2) * sp_pitch(SP_ONE);       // packed rows
constexpr int SP_SMALL_B = (SP_ONE / 2 + 1) * sp_pitch(SP_ONE);   // the half spectrum
static_assert((SP_BUF + SP_MAXR / 2) * 8 <= 65536 && (SP_SMALL_A + SP_SMALL_B + SP_ONE / 2) * 8 <= 65536,
              "static LDS per workgroup stays under 64 KB");

// as swd.hip: [-1, 1] -> {0..255}, ties to even
__device__ __forceinline__ float sp_q(float x) {
  return rintf(fminf(fmaxf(fmaf(x, 127.5f, 127.5f), 0.f), 255.f));
}

__device__ __forceinline__ float sp_luma(float r, float g, float b, int quantize) {
  if (quantize) {
    r = sp_q(r);
    g = sp_q(g);
    b = sp_q(b);
  }
  return fmaf(0.114f, b - 127.5f, fmaf(0.587f, g - 127.5f, 0.299f * (r - 127.5f)));
}

__device__ __forceinline__ float2 sp_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 sp_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 sp_mul(float2 a, float2 w) {
  return make_float2(fmaf(a.x, w.x, -a.y * w.y), fmaf(a.x, w.y, a.y * w.x));
}
__device__ __forceinline__ int sp_brev(int f, int logR) { return (int)(__brev((unsigned)f) >> (32 - logR)); }

// tw[j] = exp(-2 pi i j / R), j < R/2 (visible after the next barrier)
__device__ __forceinline__ void sp_twiddles(float2* tw, int R) {
  for (int j = threadIdx.x; j < R / 2; j += SP_BLOCK) {
    float s, c;
    sincospif(-(float)j / (float)(R / 2), &s, &c);
    tw[j] = make_float2(c, s);
  }
}

// rows 2 i, 2 i + 1 (i = first_line ..) of one image as complex lines: items (line, 4 columns)
__device__ __forceinline__ void sp_load_rows(const float* __restrict__ img, int R, int logR,
                                             int first_line, int nlines, int quantize, float2* buf) {
  const size_t plane = (size_t)R * R;
  for (int it = threadIdx.x; it < nlines << (logR - 2); it += SP_BLOCK) {
    const int l = it >> (logR - 2), c = (it & ((R >> 2) - 1)) << 2;
    const float* p = img + (size_t)(2 * (first_line + l)) * R + c;
    float4 ch[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) ch[r][k] = *reinterpret_cast<const float4*>(p + k * plane + (size_t)r * R);
    float2* d = buf + l * sp_pitch(R) + sp_at(c);      // c % 4 == 0: the four share one 32-run
    d[0] = make_float2(sp_luma(ch[0][0].x, ch[0][1].x, ch[0][2].x, quantize),
                       sp_luma(ch[1][0].x, ch[1][1].x, ch[1][2].x, quantize));
    d[1] = make_float2(sp_luma(ch[0][0].y, ch[0][1].y, ch[0][2].y, quantize),
                       sp_luma(ch[1][0].y, ch[1][1].y, ch[1][2].y, quantize));
    d[2] = make_float2(sp_luma(ch[0][0].z, ch[0][1].z, ch[0][2].z, quantize),
                       sp_luma(ch[1][0].z, ch[1][1].z, ch[1][2].z, quantize));
    d[3] = make_float2(sp_luma(ch[0][0].w, ch[0][1].w, ch[0][2].w, quantize),
                       sp_luma(ch[1][0].w, ch[1][1].w, ch[1][2].w, quantize));
  }
}

// nlines complex FFTs of length R in place, frequency f left at position brev(f).  Every thread
// of the workgroup calls it, after a barrier that made buf and tw visible; ends with a barrier.
__device__ __forceinline__ void sp_fft(float2* buf, int nlines, int R, int logR, const float2* tw) {
  const int pitch = sp_pitch(R);
  int lg = logR;                                   // log2 of the span the pass splits
  for (; lg >= 2; lg -= 2) {
    const int q = 1 << (lg - 2), sh = logR - lg;   // twiddle step of the first stage: R / span
    for (int it = threadIdx.x; it < nlines << (logR - 2); it += SP_BLOCK) {
      const int l = it >> (logR - 2), t = it & ((R >> 2) - 1);
      const int j = t & (q - 1), p0 = ((t >> (lg - 2)) << lg) + j;
      float2* x = buf + l * pitch;
      const int i0 = sp_at(p0), i1 = sp_at(p0 + q), i2 = sp_at(p0 + 2 * q), i3 = sp_at(p0 + 3 * q);
      const float2 a0 = x[i0], a1 = x[i1], a2 = x[i2], a3 = x[i3];
      const float2 w1 = tw[j << sh], w2 = tw[j << (sh + 1)];
      // stage of half-span 2 q: pairs (0, 2) and (1, 3), the latter's twiddle is -i w1
      const float2 b0 = sp_add(a0, a2), b2 = sp_mul(sp_sub(a0, a2), w1);
      const float2 b1 = sp_add(a1, a3), d = sp_mul(sp_sub(a1, a3), w1);
      const float2 b3 = make_float2(d.y, -d.x);
      // stage of half-span q: pairs (0, 1) and (2, 3), twiddle w2 = w1^2
      x[i0] = sp_add(b0, b1);
      x[i1] = sp_mul(sp_sub(b0, b1), w2);
      x[i2] = sp_add(b2, b3);
      x[i3] = sp_mul(sp_sub(b2, b3), w2);
    }
    __syncthreads();
  }
  if (lg == 1) {
    for (int it = threadIdx.x; it < nlines << (logR - 1); it += SP_BLOCK) {
      const int l = it >> (logR - 1), p = (it & ((R >> 1) - 1)) << 1;
      float2* x = buf + l * pitch + sp_at(p);      // p even: p + 1 is in the same 32-run
      const float2 a = x[0], b = x[1];
      x[0] = sp_add(a, b);
      x[1] = sp_sub(a, b);
    }
    __syncthreads();
  }
}

// the half spectra (A(v), B(v)) of the two rows packed in the transformed line z
__device__ __forceinline__ float4 sp_untangle(const float2* z, int v, int R, int logR) {
  const float2 z1 = z[sp_at(sp_brev(v, logR))], z2 = z[sp_at(sp_brev((R - v) & (R - 1), logR))];
  return make_float4(0.5f * (z1.x + z2.x), 0.5f * (z1.y - z2.y), 0.5f * (z1.y + z2.y),
                     0.5f * (z2.x - z1.x));
}

// the largest a >= 0 with a^2 <= m, or -1 for m < 0 (m < 2^24: the float holds it exactly)
__device__ __forceinline__ int sp_isqrt(int m) {
  if (m < 0) return -1;
  int a = (int)sqrtf((float)m);
  while (a * a > m) --a;
  while ((a + 1) * (a + 1) <= m) ++a;
  return a;
}

// s + the power of bin k in the transformed columns v0 .. v0 + nlines - 1 (lines of buf), in
// line order; u = -R/2 lies at frequency R/2, which has no positive twin
template <typename Acc>
__device__ __forceinline__ Acc sp_bin(const float2* buf, int nlines, int v0, int R, int logR, int k,
                                      Acc s) {
  const int H = R >> 1;
  for (int l = 0; l < nlines; ++l) {
    const int v = v0 + l;
    int hi = sp_isqrt(k * k + k - v * v);
    const int lo = k == 0 ? -1 : sp_isqrt(k * k - k - v * v);
    hi = hi < H ? hi : H;
    const float2* z = buf + l * sp_pitch(R);
    float t = 0.f;
    // four |u| at a time so that eight reads are in flight; what lies past the run reads
    // element 0 and adds 0, and the sum keeps the order of |u|
    for (int a0 = lo + 1; a0 <= hi; a0 += 4) {
      float p[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = a0 + j <= hi;
        const int a = in ? a0 + j : 0;
        const float2 f = z[sp_at(sp_brev(a, logR))];
        const float2 g = z[sp_at(sp_brev((R - a) & (R - 1), logR))];   // a = 0, H: f again, unused
        const float pf = fmaf(f.x, f.x, f.y * f.y), pg = fmaf(g.x, g.x, g.y * g.y);
        p[j] = in ? (a > 0 && a < H ? pf + pg : pf) : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) t += p[j];
    }
    s += (Acc)((v == 0 || v == H) ? t : 2.f * t);
  }
  return s;
}

// grid (B): one image per workgroup, R <= SP_ONE
__global__ __launch_bounds__(SP_BLOCK) void spectrum_small_k(const float* __restrict__ x, int R,
                                                             int logR, int quantize,
                                                             float* __restrict__ prof) {
  __shared__ __attribute__((aligned(16))) float2 s_a[SP_SMALL_A];
  __shared__ __attribute__((aligned(16))) float2 s_b[SP_SMALL_B];
  __shared__ float2 s_tw[SP_ONE / 2];
  const int H = R >> 1, pitch = sp_pitch(R);
  sp_twiddles(s_tw, R);
  sp_load_rows(x + (size_t)blockIdx.x * 3 * R * R, R, logR, 0, H, quantize, s_a);
  __syncthreads();
  sp_fft(s_a, H, R, logR, s_tw);
  for (int it = threadIdx.x; it < (H + 1) * H; it += SP_BLOCK) {
    const int v = it / H, i = it - v * H;
    const float4 ab = sp_untangle(s_a + i * pitch, v, R, logR);
    float2* d = s_b + v * pitch + sp_at(2 * i);
    d[0] = make_float2(ab.x, ab.y);
    d[1] = make_float2(ab.z, ab.w);
  }
  __syncthreads();
  sp_fft(s_b, H + 1, R, logR, s_tw);
  for (int k = threadIdx.x; k <= H; k += SP_BLOCK)
    prof[(size_t)blockIdx.x * (H + 1) + k] = (float)sp_bin<double>(s_b, H + 1, 0, R, logR, k, 0.0);
}

// grid (R / (2 NL), images of the chunk); T [image][R/2+1][R] complex
__global__ __launch_bounds__(SP_BLOCK) void spectrum_rows_k(const float* __restrict__ x, int R,
                                                            int logR, int quantize,
                                                            float2* __restrict__ T) {
  __shared__ __attribute__((aligned(16))) float2 s_z[SP_BUF];
  __shared__ float2 s_tw[SP_MAXR / 2];
  const int H = R >> 1, NL = sp_lines(R), pitch = sp_pitch(R);
  const int line0 = blockIdx.x * NL;
  sp_twiddles(s_tw, R);
  sp_load_rows(x + (size_t)blockIdx.y * 3 * R * R, R, logR, line0, NL, quantize, s_z);
  __syncthreads();
  sp_fft(s_z, NL, R, logR, s_tw);
  float2* out = T + (size_t)blockIdx.y * (H + 1) * R + 2 * line0;
  for (int it = threadIdx.x; it < (H + 1) * NL; it += SP_BLOCK) {
    const int v = it / NL, i = it - v * NL;
    *reinterpret_cast<float4*>(out + (size_t)v * R + 2 * i) = sp_untangle(s_z + i * pitch, v, R, logR);
  }
}

// grid (ceil((R/2+1) / NL), images of the chunk); part [image][workgroup][R/2+1]
__global__ __launch_bounds__(SP_BLOCK) void spectrum_cols_k(const float2* __restrict__ T, int R,
                                                            int logR, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float2 s_z[SP_BUF];
  __shared__ float2 s_tw[SP_MAXR / 2];
  const int H = R >> 1, NL = sp_lines(R), pitch = sp_pitch(R);
  const int v0 = blockIdx.x * NL;
  const int nl = H + 1 - v0 < NL ? H + 1 - v0 : NL;
  sp_twiddles(s_tw, R);
  const float2* src = T + ((size_t)blockIdx.y * (H + 1) + v0) * R;
  for (int it = threadIdx.x; it < nl << (logR - 1); it += SP_BLOCK) {
    const int l = it >> (logR - 1), p = (it & (H - 1)) << 1;
    const float4 f = *reinterpret_cast<const float4*>(src + (size_t)l * R + p);
    float2* d = s_z + l * pitch + sp_at(p);
    d[0] = make_float2(f.x, f.y);
    d[1] = make_float2(f.z, f.w);
  }
  __syncthreads();
  sp_fft(s_z, nl, R, logR, s_tw);
  float* o = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (H + 1);
  for (int k = threadIdx.x; k <= H; k += SP_BLOCK) o[k] = sp_bin<float>(s_z, nl, v0, R, logR, k, 0.f);
}

// grid (ceil((K+1) / 64), images of the chunk): an image's nwg partials in double, in a fixed
// order: SP_FIN_G groups of 64 lanes (one bin per lane) each add a contiguous range of
// workgroups in workgroup order, eight loads in flight, and group 0 adds the group sums in
// group order
constexpr int SP_FIN_K = 64, SP_FIN_G = SP_BLOCK / SP_FIN_K;
__global__ __launch_bounds__(SP_BLOCK) void spectrum_fin_k(const float* __restrict__ part, int nwg,
                                                           int nk, float* __restrict__ prof) {
  __shared__ double red[SP_FIN_G][SP_FIN_K];
  const int lane = threadIdx.x & (SP_FIN_K - 1), g = threadIdx.x / SP_FIN_K;
  const int k = blockIdx.x * SP_FIN_K + lane;
  const int per = (nwg + SP_FIN_G - 1) / SP_FIN_G;
  const int w0 = g * per, w1 = w0 + per < nwg ? w0 + per : nwg;
  double s = 0.0;
  if (k < nk) {
    const float* p = part + (size_t)blockIdx.y * nwg * nk + k;
    int w = w0;
    for (; w + 8 <= w1; w += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(w + u) * nk];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += (double)v[u];
    }
    for (; w < w1; ++w) s += (double)p[(size_t)w * nk];
  }
  red[g][lane] = s;
  __syncthreads();
  if (g == 0 && k < nk) {
    for (int j = 1; j < SP_FIN_G; ++j) s += red[j][lane];
    prof[(size_t)blockIdx.y * nk + k] = (float)s;
  }
}

bool sp_ok_r(int R) { return R >= SP_MINR && R <= SP_MAXR && (R & (R - 1)) == 0; }
bool sp_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct SpPlan {
  int chunk, nwg;             // images per chunk; column workgroups per image
  size_t t_bytes, part_bytes; // of one chunk
};

SpPlan sp_plan(int B, int R) {
  SpPlan p = {B, 0, 0, 0};
  if (R <= SP_ONE) return p;
  const size_t per = (size_t)(R / 2 + 1) * R * sizeof(float2);
  const size_t fit = SP_CHUNK_BYTES / per;
  p.chunk = (size_t)B < fit ? B : (int)fit;
  p.nwg = pg_cdiv(R / 2 + 1, sp_lines(R));
  p.t_bytes = (size_t)p.chunk * per;
  p.part_bytes = (((size_t)p.chunk * p.nwg * (R / 2 + 1) * sizeof(float)) + 15) & ~(size_t)15;
  return p;
}

}  // namespace

extern "C" {

size_t pg_spectrum_workspace_bytes(int B, int R) {
  if (B < 1 || B > 65535 || !sp_ok_r(R)) return 0;
  const SpPlan p = sp_plan(B, R);
  const size_t n = p.t_bytes + p.part_bytes;
  return n ? n : 16;          // the one-launch form uses none; the pointer rules stay the same
}

int pg_spectrum_profile(int B, int R, const float* x, int quantize, float* prof, void* ws,
                        size_t ws_bytes, void* stream) {
  PG_CHECK_ARG(sp_ok_r(R), "spectrum_profile: R (%d) must be a power of two in [%d, %d]", R, SP_MINR,
               SP_MAXR);
  PG_CHECK_ARG(B >= 1 && B <= 65535, "spectrum_profile: B (%d) must be in [1, 65535]", B);
  PG_CHECK_ARG(x && prof && ws, "spectrum_profile: null pointer");
  PG_CHECK_ARG(sp_al16(x) && sp_al16(prof) && sp_al16(ws),
               "spectrum_profile: x, prof and ws must be 16-byte aligned");
  PG_CHECK_ARG(ws_bytes >= pg_spectrum_workspace_bytes(B, R),
               "spectrum_profile: workspace of %zu B, %zu needed", ws_bytes,
               pg_spectrum_workspace_bytes(B, R));
  int logR = 0;
  while ((1 << logR) < R) ++logR;
  hipStream_t st = (hipStream_t)stream;
  const int nk = R / 2 + 1;
  if (R <= SP_ONE) {
    PG_KLAUNCH(spectrum_small_k, dim3(B), dim3(SP_BLOCK), 0, st, x, R, logR, quantize, prof);
    PG_LAUNCH_CHECK();
    return PG_OK;
  }
  const SpPlan p = sp_plan(B, R);
  float2* T = reinterpret_cast<float2*>(ws);
  float* part = reinterpret_cast<float*>(static_cast<char*>(ws) + p.t_bytes);
  const int NL = sp_lines(R);
  for (int b0 = 0; b0 < B; b0 += p.chunk) {
    const int nb = B - b0 < p.chunk ? B - b0 : p.chunk;
    PG_KLAUNCH(spectrum_rows_k, dim3(R / (2 * NL), nb), dim3(SP_BLOCK), 0, st,
               x + (size_t)b0 * 3 * R * R, R, logR, quantize, T);
    PG_LAUNCH_CHECK();
    PG_KLAUNCH(spectrum_cols_k, dim3(p.nwg, nb), dim3(SP_BLOCK), 0, st, T, R, logR, part);
    PG_LAUNCH_CHECK();
    PG_KLAUNCH(spectrum_fin_k, dim3(pg_cdiv(nk, SP_FIN_K), nb), dim3(SP_BLOCK), 0, st, part, p.nwg,
               nk, prof + (size_t)b0 * nk);
    PG_LAUNCH_CHECK();
  }
  return PG_OK;
}

}  // extern "C"
