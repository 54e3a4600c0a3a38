// Latent recovery: minimise a multi-scale pixel loss between G(z) and a target over z
// (DESIGN.md "Validation: latent recovery").
//
//   pg_recon_loss    loss, its level-0 term and dL/dimg of a batch, one launch
//   pg_latent_step   PixelNorm backward + Adam on the latent rows, best-so-far kept on the device
//
// pg_recon_loss.  d = img - tgt; d_l = the 2^l x 2^l box average of d (side R_l = R / 2^l);
//   loss[b] = sum_{l < levels} 1 / (3 R_l^2) sum d_l^2,   mse0[b] = the l = 0 term,
//   gimg    = 2 / (3 R^2) sum_l d_l[c, y >> l, x >> l]
// (d loss / d d = sum_l 2 d_l / (3 R_l^2) * 4^-l, and R_l^2 4^l = R^2).  A workgroup owns one
// T x T tile of one plane at a time, T = min(R, 32): whole top-level blocks (2^(levels - 1) <= T).  Thread
// t holds four consecutive pixels of one tile row (one 16-byte load of each input), the
// differences go to LDS, level l is pooled from level l - 1 there ((a + b) + (c + d)) / 4 by
// the first (T >> l)^2 threads, and every thread then sums its pixels' ancestors in level
// order.  The squares are summed per thread in level order, then over the workgroup
// (block_sum) and over the sample's workgroups, a contiguous index range, in a fixed order by
// the last workgroup to arrive: rc_commit2 is common.h's det_commit_seg hand-off with two
// values per workgroup.  No float atomics: the outputs are a function of the inputs.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"

namespace {

constexpr int RC_BLOCK = 256;
constexpr int RC_MAXLEV = 6;
constexpr int RC_GRID = 1024;             // workgroups of a launch, about: 4 per CU
constexpr int RC_MAXB = 2 * RC_BLOCK;     // rc_commit2's tmp holds 2 * B * G <= 4 * RC_BLOCK sums

// det_commit_seg (common.h) for two values per workgroup: v0 / v1 (valid in thread 0) go to
// outputs (0, q) / (1, q), q = bid / (nb / nseg); fin(q, total0, total1) for q < nseg in the
// last workgroup.  part [2][nb]; tmp: LDS of >= 4 * blockDim.x floats; 2 * nseg <= 4 *
// blockDim.x, 2 * nb <= pg_scratch_floats(), nb % nseg == 0.
template <typename Fin>
__device__ __forceinline__ void rc_commit2(float v0, float v1, int nseg, float* scratch, float* tmp,
                                           Fin fin) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const unsigned nb = gridDim.x, bid = blockIdx.x;
  unsigned* ticket = reinterpret_cast<unsigned*>(scratch);
  float* part = pg_scratch_partials(scratch);
  if (tid == 0) {
    __hip_atomic_store(part + bid, v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(part + nb + bid, v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  PG_DET_RELEASE();
  __syncthreads();
  __shared__ unsigned rc_last;
  if (tid == 0) {
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    rc_last = (t == nb - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (!rc_last) return;
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  const int nout = 2 * nseg;
  const unsigned seg = nb / nseg;
  int G = (4 * nt) / nout;
  G = G < 1 ? 1 : G > 64 ? 64 : G;
  if ((unsigned)G > seg) G = (int)seg;
  const unsigned per = (seg + G - 1) / G;
  for (int it = tid; it < nout * G; it += nt) {
    const int o = it % nout, g = it / nout;       // o = k * nseg + q: part + o * seg is its range
    const unsigned j0 = g * per, j1 = j0 + per < seg ? j0 + per : seg;
    const float* p = part + (size_t)o * seg;
    float s = 0.f;
    for (unsigned j = j0; j < j1; ++j)
      s += __hip_atomic_load(p + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tmp[it] = s;
  }
  __syncthreads();
  for (int q = tid; q < nseg; q += nt) {
    float s0 = 0.f, s1 = 0.f;
    for (int g = 0; g < G; ++g) {
      s0 += tmp[g * nout + q];
      s1 += tmp[g * nout + nseg + q];
    }
    fin(q, s0, s1);
  }
  if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid: B * wps workgroups, sample-major: workgroup j of sample b takes tiles j, j + wps, ... of
// the sample's tps = 3 (R / T)^2 tiles (plane-major), the next tile's loads in flight while it
// works on this one, and hands over ONE pair of partials at the end: the hand-off's ticket is
// one word, and one returning atomic per tile (12 k at 1024^2, B = 4) is what the launch would
// then wait for.  lt = log2 T.
__global__ __launch_bounds__(RC_BLOCK) void recon_loss_k(int B, int R, int lt, int levels, int wps,
                                                         const float* __restrict__ img,
                                                         const float* __restrict__ tgt,
                                                         float* __restrict__ gimg,
                                                         float* __restrict__ loss,
                                                         float* __restrict__ mse0,
                                                         float* __restrict__ scratch) {
  // level l at lev + off(l), (T >> l)^2 floats: 1024 + 256 + 64 + 16 + 4 + 1
  __shared__ __attribute__((aligned(16))) float lev[1368];
  __shared__ float red[RC_BLOCK / PG_WAVE];
  __shared__ float tmp[4 * RC_BLOCK];
  const int tid = threadIdx.x;
  const int T = 1 << lt, tpr = R >> lt;                 // tiles per plane row
  const unsigned tiles = (unsigned)tpr * tpr, tps = 3 * tiles;
  const unsigned b = blockIdx.x / wps, j0 = blockIdx.x - b * wps;
  const int q4 = T >> 2;                                // 16-byte groups per tile row
  const bool live = tid < T * q4;
  const int row = tid / q4, col = (tid - row * q4) << 2;
  auto tile_at = [&](unsigned t) {                      // this thread's pixels of the sample's tile t
    const unsigned c = t / tiles, tile = t - c * tiles;
    const unsigned ty = tile / tpr, tx = tile - ty * tpr;
    return (((size_t)b * 3 + c) * R + ((size_t)ty << lt) + row) * R + ((size_t)tx << lt) + col;
  };
  // w_l = 1 / (3 R_l^2) = 4^l / (3 R^2)
  const float w0 = 1.f / (3.f * (float)R * (float)R);
  const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
  f32x4_t ni = zero, nt = zero;
  size_t at_next = 0;
  if (live && j0 < tps) {
    at_next = tile_at(j0);
    ni = *reinterpret_cast<const f32x4_t*>(img + at_next);
    nt = *reinterpret_cast<const f32x4_t*>(tgt + at_next);
  }
  float sq = 0.f, sq0 = 0.f;
  for (unsigned t = j0; t < tps; t += wps) {
    const size_t at = at_next;
    const f32x4_t d = ni - nt;
    if (live && t + wps < tps) {
      at_next = tile_at(t + wps);
      ni = *reinterpret_cast<const f32x4_t*>(img + at_next);
      nt = *reinterpret_cast<const f32x4_t*>(tgt + at_next);
    }
    if (live) *reinterpret_cast<f32x4_t*>(lev + row * T + col) = d;
    const float s0 = ((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])) * w0;
    sq0 += s0;
    sq += s0;
    f32x4_t g = d;
    __syncthreads();
    int off = 0;
    float wl = w0;
    for (int l = 1; l < levels; ++l) {
      const int Tp = T >> (l - 1), Tl = T >> l, nxt = off + Tp * Tp;
      wl *= 4.f;
      if (tid < Tl * Tl) {
        const int y = tid / Tl, x = tid - y * Tl;
        const float* p = lev + off + (2 * y) * Tp + 2 * x;
        const float a = ((p[0] + p[1]) + (p[Tp] + p[Tp + 1])) * 0.25f;
        lev[nxt + tid] = a;
        sq += a * a * wl;
      }
      __syncthreads();
      if (live) {
        const float* pl = lev + nxt + (row >> l) * Tl;
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] += pl[(col + k) >> l];
      }
      off = nxt;
    }
    if (live) *reinterpret_cast<f32x4_t*>(gimg + at) = g * (2.f * w0);
    __syncthreads();      // every read of this tile's levels is done: the next tile takes their place
  }
  const float t_loss = block_sum(sq, red);
  const float t_mse = block_sum(sq0, red);
  rc_commit2(t_loss, t_mse, B, scratch, tmp, [&](int q, float s0, float s1) {
    loss[q] = s0;
    mse0[q] = s1;
  });
}

// One wave per latent row, lane i holds elements i, i + 64, ... (Lz / 64 <= 8 of them).
__global__ __launch_bounds__(PG_WAVE) void latent_step_k(int Lz, float* __restrict__ z,
                                                         const float* __restrict__ gzn,
                                                         float* __restrict__ m, float* __restrict__ v,
                                                         float beta1, float beta2, float omb1,
                                                         float omb2, float eps, float step_size,
                                                         float bc2_sqrt,
                                                         const float* __restrict__ loss,
                                                         float* __restrict__ best_loss,
                                                         float* __restrict__ best_z,
                                                         float* __restrict__ gz_out) {
  const int b = blockIdx.x, lane = threadIdx.x, nj = Lz >> 6;
  const size_t base = (size_t)b * Lz + lane;
  float zz[8], gn[8];
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    zz[j] = gn[j] = 0.f;
    if (j < nj) {
      zz[j] = z[base + 64 * j];
      gn[j] = gzn[base + 64 * j];
    }
    ss += zz[j] * zz[j];
  }
  // 1. the best latent so far: lane 0 alone reads and writes the row's loss pair
  float cur = 0.f, old = 0.f;
  if (lane == 0) {
    cur = loss[b];
    old = best_loss[b];
    if (cur < old) best_loss[b] = cur;
  }
  cur = __shfl(cur, 0, PG_WAVE);
  old = __shfl(old, 0, PG_WAVE);
  if (cur < old) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < nj) best_z[base + 64 * j] = zz[j];
  }
  // 2. PixelNorm backward: gz = r (gzn - zn mean(zn gzn)), zn = z r (lib/layers.py:8-14)
  const float inv = 1.f / (float)Lz;
  const float r = rsqrtf(wave_sum(ss) * inv + 1e-8f);
  float dot = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) dot += (zz[j] * r) * gn[j];
  dot = wave_sum(dot) * inv;
  // 3. Adam, torch's single-tensor update order (misc.hip: adam_update); omb = 1 - beta, rounded
  // once from the host's double
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j >= nj) continue;
    const size_t i = base + 64 * j;
    const float gi = r * (gn[j] - (zz[j] * r) * dot);
    float mi = m[i];
    mi = mi + omb1 * (gi - mi);
    const float vi = v[i] * beta2 + omb2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    z[i] = zz[j] - step_size * (mi / denom);
    if (gz_out) gz_out[i] = gi;
  }
}

bool rc_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int pg_recon_loss(int B, int R, int levels, const float* img, const float* tgt, float* gimg,
                  float* loss, float* mse0, void* scratch, void* stream) {
  PG_CHECK_ARG(img && tgt && gimg && loss && mse0 && scratch,
               "recon_loss: null pointer (scratch required)");
  PG_CHECK_ARG(R >= 4 && R <= 16384 && !(R & (R - 1)),
               "recon_loss: R (%d) must be a power of two in [4, 16384]", R);
  int lr = 0;
  while ((1 << lr) < R) ++lr;
  const int maxlev = lr + 1 < RC_MAXLEV ? lr + 1 : RC_MAXLEV;
  PG_CHECK_ARG(levels >= 1 && levels <= maxlev, "recon_loss: levels (%d) must be in [1, %d] at R = %d",
               levels, maxlev, R);
  PG_CHECK_ARG(B >= 1 && B <= RC_MAXB, "recon_loss: B (%d) must be in [1, %d]", B, RC_MAXB);
  PG_CHECK_ARG(rc_al16(img) && rc_al16(tgt) && rc_al16(gimg),
               "recon_loss: img, tgt and gimg must be 16-byte aligned");
  const int lt = lr < 5 ? lr : 5;                       // T = min(R, 32): lev[] holds 32 x 32
  // workgroups per sample: about four per CU in all, never more than the sample has tiles
  const size_t tpr = (size_t)R >> lt, tps = 3 * tpr * tpr;
  size_t wps = RC_GRID / B > 0 ? RC_GRID / B : 1;
  if (wps > tps) wps = tps;
  const size_t nb = (size_t)B * wps;
  PG_CHECK_ARG(2 * nb <= pg_scratch_floats(), "recon_loss: %zu workgroups do not fit the reduction scratch", nb);
  PG_KLAUNCH(recon_loss_k, dim3((unsigned)nb), dim3(RC_BLOCK), 0, (hipStream_t)stream, B, R, lt,
             levels, (int)wps, img, tgt, gimg, loss, mse0, (float*)scratch);
  PG_LAUNCH_CHECK();
  return PG_OK;
}

int pg_latent_step(int B, int Lz, float* z, const float* gzn, float* m, float* v, double lr,
                   double beta1, double beta2, double eps, int step, const float* loss,
                   float* best_loss, float* best_z, float* gz_out, void* stream) {
  PG_CHECK_ARG(z && gzn && m && v && loss && best_loss && best_z, "latent_step: null pointer");
  PG_CHECK_ARG(B >= 1 && step >= 1, "latent_step: B (%d) and step (%d) must be positive", B, step);
  PG_CHECK_ARG(Lz >= 64 && Lz <= 512 && Lz % 64 == 0,
               "latent_step: Lz (%d) must be a multiple of 64 in [64, 512]", Lz);
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  const float step_size = (float)(lr / bc1);
  const float bc2_sqrt = (float)sqrt(bc2);
  PG_KLAUNCH(latent_step_k, dim3(B), dim3(PG_WAVE), 0, (hipStream_t)stream, Lz, z, gzn, m, v,
             (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps,
             step_size, bc2_sqrt, loss, best_loss, best_z, gz_out);
  PG_LAUNCH_CHECK();
  return PG_OK;
}

}  // extern "C"
