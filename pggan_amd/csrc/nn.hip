// Nearest training images: exact squared L2 between 8-bit images at a comparison resolution,
// in integers (DESIGN.md "Validation: nearest training images").
//
//   pg_nn_descriptors_f32 / _u8   image -> int8 row [Rc][Rc][3] (box-pooled 8-bit pixels - 128)
//                                 and sq = sum of the row's squares
//   pg_nn_search                  merge the k nearest rows of one database chunk into the
//                                 running best lists of Q queries
//
// d^2 = sq_q + sq_x - 2 (q . x).  The dot products run on v_mfma_i32_16x16x64_i8.  One workgroup
// of nn_tile_k (4 waves): NN_ROWS = 64 database rows against NN_QT = 64 queries.  Wave w owns
// rows 16 w .. 16 w + 15 and loads them from memory straight into its A fragments (lane l: row
// l & 15, bytes 16 (l >> 4) .. + 15 of every 64-byte K step): a database byte is used by one
// wave only, so it never passes through LDS.  The queries are shared by the four waves and are
// staged through LDS, NN_KU = 4 K steps (256 bytes of every query) per barrier, double
// buffered; both operands are fetched one slab ahead in registers.  A lane's B fragment of a K
// step is the same 16 bytes of a query row, so both operands see K in the same order, which is
// all a dot product needs.
//
// LDS (64 banks of 4 B): a query slab is [64][272]: the pitch 256 + 16 puts the 16 lanes of a
// ds_read_b128 group (one K offset, 16 rows) on 16 different 16-byte slots.
//
// Epilogue: lane l holds, per query block, query l & 15 against rows 4 (l >> 4) .. + 3
// (the C/D map of the 16x16 forms).  A pair (d^2, index) is packed into one 64-bit key
// d^2 << 32 | index: d^2 <= 255^2 * 49152 < 2^32 and the index is below 2^31, so comparing keys
// compares the pairs lexicographically, and all-ones is (INT64_MAX, -1).  Keys are unique (the
// index is), so "the next smallest" is "the smallest above the last one": selection needs no
// sorted insert.  The tile's keys go to LDS as [row][query]; thread (query, quarter) picks the k
// smallest of its 16 rows, thread (query) merges the four lists and stores the workgroup's k
// keys to the workspace.  nn_merge_k (one wave per query) then picks the k smallest of the
// running list and all workgroups' lists, the same way.  No atomics: the result is a function
// of the set of keys.
#include <hip/hip_runtime.h>

#include <climits>

#include "common.h"

namespace {

typedef int nn_v4i __attribute__((ext_vector_type(4)));
typedef unsigned long long nn_key;

constexpr int NN_ROWS = 64;                    // database rows per workgroup
constexpr int NN_QT = 64;                      // queries per workgroup
constexpr int NN_KU = 4;                       // 64-byte K steps per staged slab
constexpr int NN_PITCH = NN_KU * 64 + 16;      // bytes per query row of a slab
constexpr int NN_BLOCK = 256;
constexpr int NN_MAXK = 16;
constexpr int NN_MAXD = 49152;                 // 3 * 128^2: d^2 < 2^32, the dot product fits int32
constexpr nn_key NN_NONE = ~0ull;              // (INT64_MAX, -1)

// as swd.hip / msssim.hip: [-1, 1] -> {0..255}, ties to even
__device__ __forceinline__ int nn_q(float x) {
  return (int)rintf(fminf(fmaxf(fmaf(x, 127.5f, 127.5f), 0.f), 255.f));
}

// One thread per pooled pixel: the f x f block of its three planes, V = min(f, 4) floats per
// load.  x [B][3][S][S], desc [B][Rc][Rc][3].
template <int V>
__global__ __launch_bounds__(NN_BLOCK) void nn_desc_f32_k(size_t npix, int S, int Rc, int lf,
                                                          const float* __restrict__ x,
                                                          int8_t* __restrict__ desc) {
  const size_t t = (size_t)blockIdx.x * NN_BLOCK + threadIdx.x;
  if (t >= npix) return;
  const int ox = (int)(t % Rc), oy = (int)((t / Rc) % Rc);
  const size_t b = t / ((size_t)Rc * Rc);
  const int f = 1 << lf;
  int8_t o[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* p = x + ((b * 3 + c) * S + (size_t)oy * f) * S + (size_t)ox * f;
    int s = 0;
    for (int y = 0; y < f; ++y) {
      const float* row = p + (size_t)y * S;
      for (int v = 0; v < f; v += V) {
        if constexpr (V == 4) {
          const float4 u = *reinterpret_cast<const float4*>(row + v);
          s += nn_q(u.x) + nn_q(u.y) + nn_q(u.z) + nn_q(u.w);
        } else if constexpr (V == 2) {
          const float2 u = *reinterpret_cast<const float2*>(row + v);
          s += nn_q(u.x) + nn_q(u.y);
        } else {
          s += nn_q(row[v]);
        }
      }
    }
    o[c] = (int8_t)(((s + ((f * f) >> 1)) >> (2 * lf)) - 128);
  }
  int8_t* d = desc + t * 3;
  d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
}

// The same from interleaved bytes, x [B][S][S][3].  VB bytes per unit of one source row: 48 (16
// pixels in three 16-B loads, f >= 16), 12 (4 pixels in three dwords, f = 4, 8), 3 (f = 1, 2).
template <int VB>
__global__ __launch_bounds__(NN_BLOCK) void nn_desc_u8_k(size_t npix, int S, int Rc, int lf,
                                                         const uint8_t* __restrict__ x,
                                                         int8_t* __restrict__ desc) {
  const size_t t = (size_t)blockIdx.x * NN_BLOCK + threadIdx.x;
  if (t >= npix) return;
  const int ox = (int)(t % Rc), oy = (int)((t / Rc) % Rc);
  const size_t b = t / ((size_t)Rc * Rc);
  const int f = 1 << lf;
  const uint8_t* p = x + ((b * S + (size_t)oy * f) * S + (size_t)ox * f) * 3;
  int s[3] = {0, 0, 0};
  for (int y = 0; y < f; ++y) {
    const uint8_t* row = p + (size_t)y * S * 3;
    for (int v = 0; v < 3 * f; v += VB) {
      if constexpr (VB == 3) {
        s[0] += row[v]; s[1] += row[v + 1]; s[2] += row[v + 2];
      } else {
        uint32_t w[VB / 4];
        if constexpr (VB == 48) {
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const uint4 u = *reinterpret_cast<const uint4*>(row + v + 16 * i);
            w[4 * i] = u.x; w[4 * i + 1] = u.y; w[4 * i + 2] = u.z; w[4 * i + 3] = u.w;
          }
        } else {
#pragma unroll
          for (int i = 0; i < 3; ++i) w[i] = *reinterpret_cast<const uint32_t*>(row + v + 4 * i);
        }
#pragma unroll
        for (int e = 0; e < VB; ++e) s[e % 3] += (int)((w[e / 4] >> (8 * (e % 4))) & 255u);
      }
    }
  }
  int8_t* d = desc + t * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = (int8_t)(((s[c] + ((f * f) >> 1)) >> (2 * lf)) - 128);
}

// sq[b] = sum of the squares of row b (one workgroup per row; D % 64 == 0, 16-B loads)
__global__ __launch_bounds__(NN_BLOCK) void nn_sq_k(int D, const int8_t* __restrict__ desc,
                                                    int* __restrict__ sq) {
  __shared__ int red[NN_BLOCK];
  const int8_t* row = desc + (size_t)blockIdx.x * D;
  int s = 0;
  for (int i = threadIdx.x * 16; i < D; i += NN_BLOCK * 16) {
    const nn_v4i u = *reinterpret_cast<const nn_v4i*>(row + i);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int v = (int)(int8_t)((u[e / 4] >> (8 * (e % 4))) & 255);
      s += v * v;
    }
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int st = NN_BLOCK / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) sq[blockIdx.x] = red[0];
}

// grid (row blocks, query blocks of NN_QT).  part [row blocks][Q][k] keys.
__global__ __launch_bounds__(NN_BLOCK) void nn_tile_k(int Q, int N, int D, int k,
                                                      const int8_t* __restrict__ q,
                                                      const int* __restrict__ qsq,
                                                      const int8_t* __restrict__ db,
                                                      const int* __restrict__ dbsq,
                                                      unsigned first_index,
                                                      nn_key* __restrict__ part) {
  // the two query slabs, then the tile's keys [NN_ROWS][NN_QT], then the four lists per query
  __shared__ __attribute__((aligned(16))) unsigned char s_raw[2 * NN_QT * NN_PITCH];
  static_assert(sizeof(nn_key) * NN_ROWS * NN_QT <= sizeof(s_raw), "keys alias the slabs");
  static_assert(sizeof(nn_key) * 4 * NN_MAXK * NN_QT <= sizeof(s_raw), "lists alias the keys");
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, j = lane & 15;
  const int row0 = blockIdx.x * NN_ROWS, q0 = blockIdx.y * NN_QT;

  // A: this lane's database row (the last one again past the end: read, never used)
  const int arow = min(row0 + 16 * wave + j, N - 1);
  const int8_t* ap = db + (size_t)arow * D + 16 * g;
  // staging: thread (row tid / 4, 16-byte part tid % 4 of each K step)
  const int srow = tid >> 2, sp = tid & 3;
  const bool qlive = q0 + srow < Q;
  const int8_t* qp = q + (size_t)(qlive ? q0 + srow : 0) * D + 16 * sp;
  const int nsteps = D >> 6, nslab = (nsteps + NN_KU - 1) / NN_KU;
  const nn_v4i zero = {0, 0, 0, 0};

  nn_v4i a_cur[NN_KU], a_nxt[NN_KU], qs[NN_KU], acc[NN_QT / 16];
#pragma unroll
  for (int b = 0; b < NN_QT / 16; ++b) acc[b] = zero;
#pragma unroll
  for (int u = 0; u < NN_KU; ++u) {
    const bool in = u < nsteps;
    a_nxt[u] = in ? *reinterpret_cast<const nn_v4i*>(ap + u * 64) : zero;
    qs[u] = in && qlive ? *reinterpret_cast<const nn_v4i*>(qp + u * 64) : zero;
  }
  for (int slab = 0; slab < nslab; ++slab) {
    unsigned char* buf = s_raw + (slab & 1) * (NN_QT * NN_PITCH);
#pragma unroll
    for (int u = 0; u < NN_KU; ++u) {
      *reinterpret_cast<nn_v4i*>(buf + srow * NN_PITCH + u * 64 + sp * 16) = qs[u];
      a_cur[u] = a_nxt[u];
    }
    __syncthreads();
    if (slab + 1 < nslab) {
#pragma unroll
      for (int u = 0; u < NN_KU; ++u) {
        const int step = (slab + 1) * NN_KU + u;
        const bool in = step < nsteps;      // steps past D: zeros on both sides add nothing
        a_nxt[u] = in ? *reinterpret_cast<const nn_v4i*>(ap + (size_t)step * 64) : zero;
        qs[u] = in && qlive ? *reinterpret_cast<const nn_v4i*>(qp + (size_t)step * 64) : zero;
      }
    }
#pragma unroll
    for (int u = 0; u < NN_KU; ++u)
#pragma unroll
      for (int b = 0; b < NN_QT / 16; ++b) {
        const nn_v4i bq =
            *reinterpret_cast<const nn_v4i*>(buf + (16 * b + j) * NN_PITCH + u * 64 + 16 * g);
        acc[b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_cur[u], bq, acc[b], 0, 0, 0);
      }
  }
  __syncthreads();      // every read of the slabs is done: the keys take their place

  nn_key* keys = reinterpret_cast<nn_key*>(s_raw);
  nn_key* s_cand = keys;
#pragma unroll
  for (int b = 0; b < NN_QT / 16; ++b) {
    const int qi = q0 + 16 * b + j;
    const long long sq_q = qi < Q ? (long long)qsq[qi] : 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lrow = 16 * wave + 4 * g + r, grow = row0 + lrow;
      nn_key key = NN_NONE;
      if (grow < N && qi < Q) {
        const long long d2 = sq_q + (long long)dbsq[grow] - 2 * (long long)acc[b][r];
        key = ((nn_key)d2 << 32) | (nn_key)(first_index + (unsigned)grow);
      }
      keys[lrow * NN_QT + 16 * b + j] = key;
    }
  }
  __syncthreads();

  {   // thread (query, quarter): the k smallest keys of its 16 rows, ascending
    const int ql = tid & 63, quarter = tid >> 6;
    nn_key v[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) v[c] = keys[(16 * quarter + c) * NN_QT + ql];
    __syncthreads();      // the keys are in registers: the lists take their place
    nn_key last = 0;
    for (int r = 0; r < k; ++r) {
      nn_key m = NN_NONE;
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if ((r == 0 || v[c] > last) && v[c] < m) m = v[c];
      s_cand[(quarter * NN_MAXK + r) * NN_QT + ql] = m;
      last = m;
    }
  }
  __syncthreads();

  if (tid < NN_QT && q0 + tid < Q) {   // merge the four ascending lists
    int p[4] = {0, 0, 0, 0};
    nn_key* out = part + ((size_t)blockIdx.x * Q + q0 + tid) * k;
    for (int r = 0; r < k; ++r) {
      nn_key best = NN_NONE;
      int bj = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const nn_key h = p[c] < k ? s_cand[(c * NN_MAXK + p[c]) * NN_QT + tid] : NN_NONE;
        if (h < best) { best = h; bj = c; }
      }
      out[r] = best;
#pragma unroll
      for (int c = 0; c < 4; ++c) p[c] += c == bj;
    }
  }
}

// One wave per query: the k smallest keys among its running list and the nrb lists of part.
__global__ __launch_bounds__(PG_WAVE) void nn_merge_k(int Q, int nrb, int k,
                                                      const nn_key* __restrict__ part,
                                                      long long* __restrict__ best_d2,
                                                      long long* __restrict__ best_idx) {
  const int qi = blockIdx.x, lane = threadIdx.x;
  nn_key mine = NN_NONE;          // lane r < k: entry r of the running list, read before any store
  if (lane < k) {
    const long long d = best_d2[(size_t)qi * k + lane];
    if (d != LLONG_MAX) mine = ((nn_key)d << 32) | (nn_key)(unsigned)best_idx[(size_t)qi * k + lane];
  }
  const size_t total = (size_t)nrb * k;
  nn_key last = 0;
  for (int r = 0; r < k; ++r) {
    nn_key m = (r == 0 || mine > last) ? mine : NN_NONE;
    for (size_t c = lane; c < total; c += PG_WAVE) {
      const size_t rb = c / k, e = c - rb * k;
      const nn_key v = part[(rb * Q + qi) * k + e];
      if ((r == 0 || v > last) && v < m) m = v;
    }
#pragma unroll
    for (int off = PG_WAVE / 2; off > 0; off >>= 1) {
      const nn_key o = __shfl_xor(m, off);
      m = o < m ? o : m;
    }
    if (lane == 0) {
      best_d2[(size_t)qi * k + r] = m == NN_NONE ? LLONG_MAX : (long long)(m >> 32);
      best_idx[(size_t)qi * k + r] = m == NN_NONE ? -1 : (long long)(m & 0xffffffffull);
    }
    last = m;
  }
}

bool nn_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// log2(S / Rc), or -1 where the pair is not one the kernels take
int nn_check_sizes(int S, int Rc) {
  if (Rc < 8 || Rc > 128 || (Rc & (Rc - 1)) || S < Rc || S > 16384 || (S & (S - 1))) return -1;
  int lf = 0;
  while ((Rc << lf) < S) ++lf;
  return lf;
}

int nn_sq_launch(int B, int D, const int8_t* desc, int* sq, hipStream_t st) {
  PG_KLAUNCH(nn_sq_k, dim3(B), dim3(NN_BLOCK), 0, st, D, desc, sq);
  PG_LAUNCH_CHECK();
  return PG_OK;
}

}  // namespace

extern "C" {

int pg_nn_row_block(void) { return NN_ROWS; }

int pg_nn_descriptors_f32(int B, int S, int Rc, const float* x, int8_t* desc, int* sq,
                          void* stream) {
  PG_CHECK_ARG(x && desc && sq, "nn_descriptors_f32: null pointer");
  PG_CHECK_ARG(B > 0 && B <= 65535, "nn_descriptors_f32: B (%d) must be in [1, 65535]", B);
  const int lf = nn_check_sizes(S, Rc);
  PG_CHECK_ARG(lf >= 0, "nn_descriptors_f32: Rc (%d) must be a power of two in [8, 128] and S "
               "(%d) a power of two >= Rc", Rc, S);
  PG_CHECK_ARG(nn_al16(x) && nn_al16(desc), "nn_descriptors_f32: x and desc must be 16-byte aligned");
  const size_t npix = (size_t)B * Rc * Rc;
  const dim3 grid((unsigned)((npix + NN_BLOCK - 1) / NN_BLOCK));
  hipStream_t st = (hipStream_t)stream;
  if (lf >= 2)
    PG_KLAUNCH(nn_desc_f32_k<4>, grid, dim3(NN_BLOCK), 0, st, npix, S, Rc, lf, x, desc);
  else if (lf == 1)
    PG_KLAUNCH(nn_desc_f32_k<2>, grid, dim3(NN_BLOCK), 0, st, npix, S, Rc, lf, x, desc);
  else
    PG_KLAUNCH(nn_desc_f32_k<1>, grid, dim3(NN_BLOCK), 0, st, npix, S, Rc, lf, x, desc);
  PG_LAUNCH_CHECK();
  return nn_sq_launch(B, 3 * Rc * Rc, desc, sq, st);
}

int pg_nn_descriptors_u8(int B, int S, int Rc, const uint8_t* x, int8_t* desc, int* sq,
                         void* stream) {
  PG_CHECK_ARG(x && desc && sq, "nn_descriptors_u8: null pointer");
  PG_CHECK_ARG(B > 0 && B <= 65535, "nn_descriptors_u8: B (%d) must be in [1, 65535]", B);
  const int lf = nn_check_sizes(S, Rc);
  PG_CHECK_ARG(lf >= 0, "nn_descriptors_u8: Rc (%d) must be a power of two in [8, 128] and S "
               "(%d) a power of two >= Rc", Rc, S);
  PG_CHECK_ARG(nn_al16(x) && nn_al16(desc), "nn_descriptors_u8: x and desc must be 16-byte aligned");
  const size_t npix = (size_t)B * Rc * Rc;
  const dim3 grid((unsigned)((npix + NN_BLOCK - 1) / NN_BLOCK));
  hipStream_t st = (hipStream_t)stream;
  if (lf >= 4)
    PG_KLAUNCH(nn_desc_u8_k<48>, grid, dim3(NN_BLOCK), 0, st, npix, S, Rc, lf, x, desc);
  else if (lf >= 2)
    PG_KLAUNCH(nn_desc_u8_k<12>, grid, dim3(NN_BLOCK), 0, st, npix, S, Rc, lf, x, desc);
  else
    PG_KLAUNCH(nn_desc_u8_k<3>, grid, dim3(NN_BLOCK), 0, st, npix, S, Rc, lf, x, desc);
  PG_LAUNCH_CHECK();
  return nn_sq_launch(B, 3 * Rc * Rc, desc, sq, st);
}

size_t pg_nn_workspace_bytes(int Q, int N, int k) {
  if (Q < 1 || N < 1 || k < 1 || k > NN_MAXK) return 0;
  return (size_t)pg_cdiv(N, NN_ROWS) * Q * k * sizeof(nn_key);
}

int pg_nn_search(int Q, int N, int D, int k, const int8_t* q, const int* qsq, const int8_t* db,
                 const int* dbsq, long long first_index, long long* best_d2, long long* best_idx,
                 void* ws, size_t ws_bytes, void* stream) {
  PG_CHECK_ARG(q && qsq && db && dbsq && best_d2 && best_idx && ws, "nn_search: null pointer");
  PG_CHECK_ARG(k >= 1 && k <= NN_MAXK, "nn_search: k (%d) must be in [1, %d]", k, NN_MAXK);
  PG_CHECK_ARG(D >= 64 && D <= NN_MAXD && D % 64 == 0,
               "nn_search: D (%d) must be a multiple of 64 in [64, %d]", D, NN_MAXD);
  PG_CHECK_ARG(Q >= 1 && Q <= 65535 * NN_QT, "nn_search: Q (%d) must be in [1, %d]", Q,
               65535 * NN_QT);
  PG_CHECK_ARG(N >= 1, "nn_search: N (%d) must be positive", N);
  PG_CHECK_ARG(first_index >= 0 && first_index + N <= (long long)INT_MAX,
               "nn_search: indices %lld .. + %d must stay below 2^31", first_index, N);
  PG_CHECK_ARG(nn_al16(q) && nn_al16(db), "nn_search: q and db must be 16-byte aligned");
  PG_CHECK_ARG(((uintptr_t)ws & 7) == 0, "nn_search: the workspace must be 8-byte aligned");
  PG_CHECK_ARG(ws_bytes >= pg_nn_workspace_bytes(Q, N, k),
               "nn_search: workspace of %zu B, %zu needed", ws_bytes,
               pg_nn_workspace_bytes(Q, N, k));
  hipStream_t st = (hipStream_t)stream;
  const int nrb = pg_cdiv(N, NN_ROWS);
  nn_key* part = reinterpret_cast<nn_key*>(ws);
  PG_KLAUNCH(nn_tile_k, dim3(nrb, pg_cdiv(Q, NN_QT)), dim3(NN_BLOCK), 0, st, Q, N, D, k, q, qsq,
             db, dbsq, (unsigned)first_index, part);
  PG_LAUNCH_CHECK();
  PG_KLAUNCH(nn_merge_k, dim3(Q), dim3(PG_WAVE), 0, st, Q, nrb, k, part, best_d2, best_idx);
  PG_LAUNCH_CHECK();
  return PG_OK;
}

}  // extern "C"
