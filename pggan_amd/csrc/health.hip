// Training health (DESIGN.md "Training health"): per-tensor statistics of a net's flat fp32
// buffers and the every-step non-finite probe.  Both read the buffers between steps and write
// nothing the step reads.
//
//   pg_tensor_stats      per segment (tensor): sums of squares and largest magnitudes of the
//                        parameter, the gradient and the Adam update, over the finite elements,
//                        and the number of non-finite elements of p, g, m, v
//   pg_nonfinite_watch   first_bad[segment] = tag for every segment that holds a non-finite
//                        element and has no tag yet
//
// A segment table is int64 {offset, count} pairs on the DEVICE: offsets multiples of 16 floats,
// count the tensor's true length, segments disjoint and ascending.  What lies between
// offset + count and the next offset is padding and is never read: whole quads are 16-byte
// loads, the 1 .. 3 elements after a tensor's last whole quad are scalar loads.
//
// Work split without a host plan (the table never leaves the device): the buffer [0, n) is cut
// into ranges of TS_CHUNK floats, one wave per range, four ranges per workgroup -- a large
// tensor spreads over count / TS_CHUNK waves and a run of tiny tensors shares one.  A wave finds
// the first segment that ends behind its range's start by bisection and walks the segments
// until one starts behind the range's end; for each it reduces the intersection over its lanes
// (xor butterfly: a fixed order) and lane 0 stores PG_TS_COLS doubles to partial slot
// s + r (segment + range).  The pairs (s, r) that intersect form a staircase along which s + r
// rises strictly, so the slots are distinct and at most nseg + ranges many: the workspace is
// sized from (nseg, n) alone.  tensor_stats_fin_k, one workgroup per segment, combines the
// segment's slots s + r0 .. s + r1 in slot order with a fixed split over its threads.  No
// atomics anywhere: `out` is bitwise repeatable.
//
// Arithmetic: squares and sums in double (the square of an fp32 value is exact there: 1e25 and
// 1e-30 neither overflow nor vanish); the Adam update u = step_size m / (sqrt(v) / bc2_sqrt +
// eps) from the fp32 m, v and the fp32 scalars widened to double, every operation rounded on
// its own (-ffp-contract=off for this file), where both m and v are finite.  Counts travel as
// int per lane and as exact doubles afterwards.
//
// The watch is one grid-stride pass over [0, n) in 16-byte loads that tests exponent bits only;
// a lane that meets a non-finite quad (never, in a healthy run) bisects the table for the
// quad's segment, skips padding, and stores the tag with a plain vector store where the slot is
// still 0.  Every writer of a slot within a launch writes the same value.
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

constexpr int TS_BLOCK = 256;
constexpr int TS_WAVES = TS_BLOCK / PG_WAVE;
constexpr int TS_CHUNK = 2048;                       // floats per wave: 8 quads per lane
constexpr int TS_QUADS = TS_CHUNK / 4 / PG_WAVE;     // whole quads per lane in a full range
constexpr int TS_COLS = PG_TS_COLS;
static_assert(TS_CHUNK % (4 * PG_WAVE) == 0 && TS_CHUNK % 16 == 0, "ranges start on segment alignment");
static_assert(TS_COLS == 10, "sumsq p g u, maxabs p g u, bad p g m v");

constexpr int NW_BLOCK = 256, NW_UNROLL = 4, NW_MAX_GRID = 2048;

__device__ __forceinline__ bool ts_finite(float x) {
  return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
}

struct TsAcc {
  double sp, sg, su, mu;
  float mp, mg;
  int bp, bg, bm, bv;
};

__device__ __forceinline__ void ts_pg(float x, double& s, float& mx, int& bad) {
  const bool f = ts_finite(x);
  const float a = f ? fabsf(x) : 0.f;
  const double d = (double)a;
  s += d * d;
  mx = fmaxf(mx, a);
  bad += f ? 0 : 1;
}

struct TsIn {
  const float *p, *g, *m, *v;
  double step_size, bc2_sqrt, eps;
};

__device__ __forceinline__ void ts_one(const TsIn& in, bool hp, bool hg, bool hm, bool hv, float p,
                                       float g, float m, float v, TsAcc& a) {
  if (hp) ts_pg(p, a.sp, a.mp, a.bp);
  if (hg) ts_pg(g, a.sg, a.mg, a.bg);
  const bool fm = ts_finite(m), fv = ts_finite(v);
  if (hm) a.bm += fm ? 0 : 1;
  if (hv) a.bv += fv ? 0 : 1;
  if (hm && hv) {
    const bool f = fm && fv;
    const double dm = f ? (double)m : 0.0, dv = f ? (double)v : 0.0;
    const double u = fabs((in.step_size * dm) / (sqrt(dv) / in.bc2_sqrt + in.eps));
    a.su += u * u;
    a.mu = fmax(a.mu, u);
  }
}

template <typename T>
__device__ __forceinline__ T ts_wave(T v, bool take_max) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T w = __shfl_xor(v, o, 64);
    v = take_max ? (v > w ? v : w) : v + w;
  }
  return v;
}

// the largest s with tab[2 s] <= i, or -1
__device__ __forceinline__ int ts_seg_of(int nseg, const long long* __restrict__ tab, long long i) {
  int lo = 0, hi = nseg;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab[2 * mid] <= i) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// grid (ceil(ranges / TS_WAVES)); part [nseg + ranges][TS_COLS]
__global__ __launch_bounds__(TS_BLOCK) void tensor_stats_k(int nseg, const long long* __restrict__ tab,
                                                           long long n, TsIn in,
                                                           double* __restrict__ part) {
  const int lane = threadIdx.x & (PG_WAVE - 1);
  const long long r = (long long)blockIdx.x * TS_WAVES + (threadIdx.x >> 6);
  const long long rb = r * TS_CHUNK;
  if (rb >= n) return;                                 // wave-uniform
  const long long re = rb + TS_CHUNK < n ? rb + TS_CHUNK : n;
  const bool hp = in.p != nullptr, hg = in.g != nullptr, hm = in.m != nullptr, hv = in.v != nullptr;
  // the first segment that ends behind rb
  int lo = 0, hi = nseg;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab[2 * mid] + tab[2 * mid + 1] > rb) hi = mid; else lo = mid + 1;
  }
  for (int s = lo; s < nseg; ++s) {
    const long long off = tab[2 * s], cnt = tab[2 * s + 1];
    if (off >= re) break;
    const long long b = off > rb ? off : rb;           // a multiple of 16: both are
    const long long e = off + cnt < re ? off + cnt : re;
    if (e <= b) continue;
    const int len = (int)(e - b), nq = len >> 2, rem = len & 3;
    TsAcc a = {0.0, 0.0, 0.0, 0.0, 0.f, 0.f, 0, 0, 0, 0};
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // whole quads: TS_QUADS per lane in two batches, every load of a batch in flight at once
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float4 qp[TS_QUADS / 2], qg[TS_QUADS / 2], qm[TS_QUADS / 2], qv[TS_QUADS / 2];
#pragma unroll
      for (int k = 0; k < TS_QUADS / 2; ++k) {
        const int q = (h * (TS_QUADS / 2) + k) * PG_WAVE + lane;
        const bool ok = q < nq;
        const long long i = b + 4 * (long long)(ok ? q : 0);
        qp[k] = ok && hp ? *reinterpret_cast<const float4*>(in.p + i) : z4;
        qg[k] = ok && hg ? *reinterpret_cast<const float4*>(in.g + i) : z4;
        qm[k] = ok && hm ? *reinterpret_cast<const float4*>(in.m + i) : z4;
        qv[k] = ok && hv ? *reinterpret_cast<const float4*>(in.v + i) : z4;
      }
#pragma unroll
      for (int k = 0; k < TS_QUADS / 2; ++k) {
        const int q = (h * (TS_QUADS / 2) + k) * PG_WAVE + lane;
        if (q < nq) {
          ts_one(in, hp, hg, hm, hv, qp[k].x, qg[k].x, qm[k].x, qv[k].x, a);
          ts_one(in, hp, hg, hm, hv, qp[k].y, qg[k].y, qm[k].y, qv[k].y, a);
          ts_one(in, hp, hg, hm, hv, qp[k].z, qg[k].z, qm[k].z, qv[k].z, a);
          ts_one(in, hp, hg, hm, hv, qp[k].w, qg[k].w, qm[k].w, qv[k].w, a);
        }
      }
    }
    // the tensor's last 1 .. 3 elements: scalar loads, the padding behind them is not touched
    if (lane < rem) {
      const long long i = b + 4 * (long long)nq + lane;
      ts_one(in, hp, hg, hm, hv, hp ? in.p[i] : 0.f, hg ? in.g[i] : 0.f, hm ? in.m[i] : 0.f,
             hv ? in.v[i] : 0.f, a);
    }
    const double sp = ts_wave(a.sp, false), sg = ts_wave(a.sg, false), su = ts_wave(a.su, false);
    const float mp = ts_wave(a.mp, true), mg = ts_wave(a.mg, true);
    const double mu = ts_wave(a.mu, true);
    const int bp = ts_wave(a.bp, false), bg = ts_wave(a.bg, false), bm = ts_wave(a.bm, false),
              bv = ts_wave(a.bv, false);
    if (lane == 0) {
      double2* o = reinterpret_cast<double2*>(part + (size_t)(s + r) * TS_COLS);
      o[0] = make_double2(sp, sg);
      o[1] = make_double2(su, (double)mp);
      o[2] = make_double2((double)mg, mu);
      o[3] = make_double2((double)bp, (double)bg);
      o[4] = make_double2((double)bm, (double)bv);
    }
  }
}

// grid (nseg): the slots s + r0 .. s + r1 of segment s, columns 0-2 and 6-9 summed, 3-5 by
// maximum.  Thread t takes a contiguous run of slots in slot order; the threads' values are
// combined by the wave butterfly and then over the waves in wave order: a fixed tree.
__global__ __launch_bounds__(TS_BLOCK) void tensor_stats_fin_k(int nseg, const long long* __restrict__ tab,
                                                               long long n, const double* __restrict__ part,
                                                               double* __restrict__ out) {
  __shared__ double red[TS_WAVES][TS_COLS];
  const int s = blockIdx.x, t = threadIdx.x;
  const long long off = tab[2 * s], cnt = tab[2 * s + 1];
  const long long end = off + cnt < n ? off + cnt : n;
  long long nslot = 0, r0 = 0;
  if (cnt > 0 && off >= 0 && off < end) {
    r0 = off / TS_CHUNK;
    nslot = (end - 1) / TS_CHUNK - r0 + 1;
  }
  const long long per = (nslot + TS_BLOCK - 1) / TS_BLOCK;
  const long long j0 = t * per, j1 = j0 + per < nslot ? j0 + per : nslot;
  double acc[TS_COLS];
#pragma unroll
  for (int c = 0; c < TS_COLS; ++c) acc[c] = 0.0;
  for (long long j = j0; j < j1; ++j) {
    const double2* p = reinterpret_cast<const double2*>(part + (size_t)(s + r0 + j) * TS_COLS);
    double v[TS_COLS];
#pragma unroll
    for (int c = 0; c < TS_COLS / 2; ++c) {
      const double2 d = p[c];
      v[2 * c] = d.x;
      v[2 * c + 1] = d.y;
    }
#pragma unroll
    for (int c = 0; c < TS_COLS; ++c) acc[c] = (c >= 3 && c < 6) ? fmax(acc[c], v[c]) : acc[c] + v[c];
  }
#pragma unroll
  for (int c = 0; c < TS_COLS; ++c) acc[c] = ts_wave(acc[c], c >= 3 && c < 6);
  if ((t & (PG_WAVE - 1)) == 0) {
#pragma unroll
    for (int c = 0; c < TS_COLS; ++c) red[t >> 6][c] = acc[c];
  }
  __syncthreads();
  if (t < TS_COLS) {
    double v = red[0][t];
    for (int w = 1; w < TS_WAVES; ++w) v = (t >= 3 && t < 6) ? fmax(v, red[w][t]) : v + red[w][t];
    out[(size_t)s * TS_COLS + t] = v;
  }
}

// a non-finite element among the four at i0 (bits of `bad`): latch its segment unless it is padding
__device__ __noinline__ void nw_latch(int nseg, const long long* __restrict__ tab, long long i0,
                                      unsigned bad, int tag, int* __restrict__ first_bad) {
  const int s = ts_seg_of(nseg, tab, i0);
  if (s < 0) return;
  const long long end = tab[2 * s] + tab[2 * s + 1];
  bool hit = false;
  for (int j = 0; j < 4; ++j) hit |= ((bad >> j) & 1u) && i0 + j < end;
  if (hit && first_bad[s] == 0) first_bad[s] = tag;
}

__device__ __forceinline__ unsigned nw_bad(unsigned w) { return (w & 0x7f800000u) == 0x7f800000u; }

// grid-stride over the whole quads of x[0, n); the last n % 4 elements by the first lanes
__global__ __launch_bounds__(NW_BLOCK) void nonfinite_watch_k(int nseg, const long long* __restrict__ tab,
                                                              const float* __restrict__ x, long long n,
                                                              int tag, int* __restrict__ first_bad) {
  const long long nq = n >> 2, stride = (long long)gridDim.x * NW_BLOCK;
  const long long t = (long long)blockIdx.x * NW_BLOCK + threadIdx.x;
  const u32x4_t* q = reinterpret_cast<const u32x4_t*>(x);
  for (long long i = t; i < nq; i += NW_UNROLL * stride) {
    u32x4_t w[NW_UNROLL];
#pragma unroll
    for (int k = 0; k < NW_UNROLL; ++k) {
      const long long j = i + k * stride;
      w[k] = q[j < nq ? j : i];
    }
#pragma unroll
    for (int k = 0; k < NW_UNROLL; ++k) {
      const long long j = i + k * stride;
      const unsigned bad = nw_bad(w[k][0]) | nw_bad(w[k][1]) << 1 | nw_bad(w[k][2]) << 2 |
                           nw_bad(w[k][3]) << 3;
      if (bad && j < nq) nw_latch(nseg, tab, 4 * j, bad, tag, first_bad);
    }
  }
  if (t < (n & 3)) {
    const long long i = 4 * nq + t;
    if (nw_bad(__float_as_uint(x[i]))) nw_latch(nseg, tab, i, 1u, tag, first_bad);
  }
}

bool ts_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
size_t ts_ranges(size_t n) { return (n + TS_CHUNK - 1) / TS_CHUNK; }

}  // namespace

extern "C" {

int pg_tensor_stats_chunk(void) { return TS_CHUNK; }

size_t pg_tensor_stats_workspace_bytes(int nseg, size_t n) {
  if (nseg < 1 || n < 1 || n > ((size_t)1 << 40)) return 0;
  return ((size_t)nseg + ts_ranges(n)) * TS_COLS * sizeof(double);
}

int pg_tensor_stats(int nseg, const int64_t* table, size_t n, const float* p, const float* g,
                    const float* m, const float* v, float step_size, float bc2_sqrt, float eps,
                    double* out, void* ws, size_t ws_bytes, void* stream) {
  PG_CHECK_ARG(nseg >= 1 && nseg <= 65535, "tensor_stats: nseg (%d) must be in [1, 65535]", nseg);
  PG_CHECK_ARG(table && out && ws, "tensor_stats: null table, out or workspace");
  PG_CHECK_ARG(n >= 1 && n <= ((size_t)1 << 40), "tensor_stats: n (%zu) out of range", n);
  PG_CHECK_ARG(ts_al16(table) && ts_al16(p) && ts_al16(g) && ts_al16(m) && ts_al16(v) &&
                   ts_al16(out) && ts_al16(ws),
               "tensor_stats: table, p, g, m, v, out and ws must be 16-byte aligned");
  PG_CHECK_ARG(ws_bytes >= pg_tensor_stats_workspace_bytes(nseg, n),
               "tensor_stats: workspace of %zu B, %zu needed", ws_bytes,
               pg_tensor_stats_workspace_bytes(nseg, n));
  PG_CHECK_ARG(!(m || v) || (step_size > 0.f && bc2_sqrt > 0.f && eps >= 0.f),
               "tensor_stats: step_size (%g) and bc2_sqrt (%g) must be positive, eps (%g) not negative",
               (double)step_size, (double)bc2_sqrt, (double)eps);
  hipStream_t st = (hipStream_t)stream;
  const TsIn in = {p, g, m, v, (double)step_size, (double)bc2_sqrt, (double)eps};
  double* part = static_cast<double*>(ws);
  const size_t nr = ts_ranges(n);
  PG_KLAUNCH(tensor_stats_k, dim3((unsigned)((nr + TS_WAVES - 1) / TS_WAVES)), dim3(TS_BLOCK), 0, st,
             nseg, (const long long*)table, (long long)n, in, part);
  PG_LAUNCH_CHECK();
  PG_KLAUNCH(tensor_stats_fin_k, dim3(nseg), dim3(TS_BLOCK), 0, st, nseg, (const long long*)table,
             (long long)n, (const double*)part, out);
  PG_LAUNCH_CHECK();
  return PG_OK;
}

int pg_nonfinite_watch(int nseg, const int64_t* table, const float* x, size_t n, int tag,
                       int* first_bad, void* stream) {
  PG_CHECK_ARG(nseg >= 1, "nonfinite_watch: nseg (%d) must be positive", nseg);
  PG_CHECK_ARG(table && x && first_bad, "nonfinite_watch: null table, x or first_bad");
  PG_CHECK_ARG(n >= 1 && n <= ((size_t)1 << 40), "nonfinite_watch: n (%zu) out of range", n);
  PG_CHECK_ARG(tag > 0, "nonfinite_watch: tag (%d) must be positive (0 means never)", tag);
  PG_CHECK_ARG(ts_al16(table) && ts_al16(x), "nonfinite_watch: table and x must be 16-byte aligned");
  const size_t nq = n >> 2, per = (size_t)NW_BLOCK * NW_UNROLL;
  size_t grid = (nq + per - 1) / per;
  grid = grid < 1 ? 1 : grid > (size_t)NW_MAX_GRID ? (size_t)NW_MAX_GRID : grid;
  PG_KLAUNCH(nonfinite_watch_k, dim3((unsigned)grid), dim3(NW_BLOCK), 0, (hipStream_t)stream, nseg,
             (const long long*)table, x, (long long)n, tag, first_bad);
  PG_LAUNCH_CHECK();
  return PG_OK;
}

}  // extern "C"
