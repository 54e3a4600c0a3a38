// Included inside conv.hip's anonymous namespace (uses ConvParams, Ty, lrelu_f, ...).
//
// conv_lr_kernel: bf16 3x3 convolution for the low-resolution stages (W = H <= 16 with
// 256-512 channels: M = B*H*W <= 1024 output pixels against N = cout, K = 9 * cin).  The
// output tile is small (TH rows of one image x 16 output channels) and K is split over
// the PG_LR_NW (8) waves of the workgroup instead of over workgroups, so the step needs no fp32
// slabs and no second (split-K epilogue) launch:
//
//   staging  : the tile's (TH+2) x (W+2) input halo with ALL cin channels, once, by
//              LDS-DMA (global_load_lds_dwordx4: one wave-instruction = 1 KiB = 512
//              channels of one pixel; pixel rows padded 32 B for conflict-free fragment
//              reads; out-of-image pixels read a zero row)
//   weights  : the 16 x 9*cin slab of the tile's output channels is streamed once per
//              workgroup straight into registers: each wave issues the A fragments of its
//              whole K range (<= 39 x 16 B per lane) before the halo DMA, so the workgroup
//              pays one memory round trip; nothing is shared across waves, so no LDS)
//   MFMA     : v_mfma_f32_16x16x32_bf16, D[cout][pixel]; wave w owns k-steps w, w+NW, ...
//              (k-step = one tap x 32 channels)
//   reduce   : the NW partial tiles are summed through LDS in wave order (fixed order,
//              deterministic), then the epilogue: bias, leaky-relu, 2x2 pool (+ pre-pool
//              copy), out_scale, lrelu' mask, accumulate -- the conv3x3 flag semantics.
// Reference: lib/layers.py:58-89, lib/blocks.py:113-201 (same math as conv3x3_kernel).

__device__ __attribute__((aligned(16))) bf16_t pg_lr_zero_row[1024];   // zero-initialised

#ifndef PG_LR_NW
// waves per workgroup (K split over them): 8 waves halve each wave's weight fragments and
// double the loads in flight per CU; the 8x8 launches 12.9-14.7 -> 9.6-11.1 us, 4x4 ~flat,
// 16 waves no better (profiles/r6_lr_waves_ab.txt)
#define PG_LR_NW 8
#endif

template <int W, int TH, int NCH>
__global__ __launch_bounds__(64 * PG_LR_NW) void conv_lr_kernel(ConvParams p) {
  constexpr int NWV = PG_LR_NW;
  constexpr int TW2 = W + 2, TH2 = TH + 2;
  constexpr int BM = TH * W, MT = BM / 16;
  constexpr int NKS = 9 * NCH;                  // k-steps (one tap x 32 channels each)
  constexpr int KPW = (NKS + NWV - 1) / NWV;    // k-steps of wave 0 (the others: one fewer at most)
  static_assert(BM % 16 == 0 && MT >= 1 && MT <= 4, "tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r = lane & 15;
  const int tiles_y = p.H / TH;
  // XCD-aware order: the pixel tiles that share one 16-channel weight slab run behind one L2
  int bx = blockIdx.x, by = blockIdx.y;
  if (p.xcd_remap) {
    const int ox = gridDim.x, n = ox * gridDim.y, h = bx + ox * by;
    const int xcd = h & 7, slot = h >> 3, q = n >> 3, rr = n & 7;
    const int Lg = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + slot;
    bx = Lg % ox;
    by = Lg / ox;
  }
  const int b = bx / tiles_y, y0 = (bx - b * tiles_y) * TH;
  const int n0 = by * 16;
  constexpr int cin_p = NCH * 32;
  constexpr int rowb = cin_p * 2;               // bytes of one pixel's channels
  constexpr int PIXB = rowb + 32;               // LDS pixel pitch (conflict-free B reads)
  const bool ups = (p.flags & PG_CONV_UPS_IN) != 0;
  const int ys = ups ? 1 : 0;
  const bf16_t* x = reinterpret_cast<const bf16_t*>(p.x);
  const bf16_t* wpk = reinterpret_cast<const bf16_t*>(p.w);

  // ---- every weight fragment this wave needs (k-steps wid, wid+NW, ...), issued first:
  // one memory round trip for the whole K range (GEMV-style weight streaming, no reuse
  // across waves to share through LDS)
  const bf16_t* wrow = wpk + (size_t)(n0 + r) * 9 * cin_p + 8 * g;   // this lane's weight row
  bf16x8_t wa[KPW];
#pragma unroll
  for (int j = 0; j < KPW; ++j) {
    int ks = wid + NWV * j;
    ks = ks < NKS ? ks : NKS - 1;    // past the end (waves 1-3 at 9*NCH % 4 != 0): never used
    const int tap = ks % 9, ch = ks / 9;
    wa[j] = *reinterpret_cast<const bf16x8_t*>(wrow + tap * cin_p + ch * 32);
  }
  // ---- halo: one LDS-DMA wave-instruction per KiB of a pixel's channels
  {
    constexpr int nq = (rowb + 1023) >> 10;
    for (int hp = wid; hp < TH2 * TW2; hp += NWV) {
      const int hy = hp / TW2, hx = hp - hy * TW2;
      const int yy = y0 + hy - 1, xx = hx - 1;
      const bool in = (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W;
      const bf16_t* src = in ? x + ((size_t)(b * p.Hin + (yy >> ys)) * p.Win + (xx >> ys)) * p.x_cs
                             : pg_lr_zero_row;
#pragma unroll
      for (int q = 0; q < nq; ++q) {
        const int off = q * 1024 + lane * 16;      // byte offset inside the pixel row
        if (off < rowb) {
          const char* gsrc = in ? reinterpret_cast<const char*>(src) + off
                                : reinterpret_cast<const char*>(pg_lr_zero_row) + (off & 1023);
          __builtin_amdgcn_global_load_lds(
              (const void*)gsrc,
              (__attribute__((address_space(3))) void*)(smem + hp * PIXB + q * 1024), 16, 0, 0);
        }
      }
    }
  }
  // pixel of each of this lane's pixel blocks inside the halo (tap (0,0) corner)
  int hoff[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int pix = mt * 16 + r, row = pix / W, col = pix - row * W;
    hoff[mt] = (row * TW2 + col) * PIXB + g * 16;
  }
  f32x4_t acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  __syncthreads();   // vmcnt(0): the halo DMA and the weight fragments have landed

  const int my_n = (NKS - wid + NWV - 1) / NWV;
#pragma unroll
  for (int j = 0; j < KPW; ++j) {
    if (j < my_n) {   // wave-uniform
      const int ks = wid + NWV * j;
      const int tap = ks % 9, ch = ks / 9;
      const int toff = ((tap / 3) * TW2 + (tap % 3)) * PIXB + ch * 64;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const bf16x8_t bx = *reinterpret_cast<const bf16x8_t*>(smem + hoff[mt] + toff);
        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[j], bx, acc[mt], 0, 0, 0);
      }
    }
  }

  // ---- sum the NW waves' partial tiles (wave order), block mt -> red[w][mt][lane]
  __syncthreads();   // every wave is done reading the halo
  f32x4_t* red = reinterpret_cast<f32x4_t*>(smem);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) red[(wid * MT + mt) * 64 + lane] = acc[mt];
  __syncthreads();
  const bool pool = (p.flags & PG_CONV_POOL) != 0;
  // epilogue blocks per wave: the 2x2 pool at W = 16 pairs block mt with mt ^ 1
  constexpr int EB = (W == 16) ? 2 : 1;
  if (wid * EB >= MT) return;
  const bool has_bias = (p.flags & PG_CONV_BIAS) != 0;
  const bool do_lrelu = (p.flags & PG_CONV_LRELU) != 0;
  const bool do_mask = (p.flags & PG_CONV_MASK) != 0;
  const bool do_acc = (p.flags & PG_CONV_ACCUM) != 0;
  const int n = n0 + 4 * g;
  const bool nok = n < p.cout;
  float bv[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) bv[q] = (has_bias && nok) ? p.bias[n + q] : 0.f;
  float v[EB][4];
#pragma unroll
  for (int e = 0; e < EB; ++e) {
    const int mt = wid * EB + e;
    f32x4_t s = red[mt * 64 + lane];
#pragma unroll
    for (int w = 1; w < NWV; ++w) s += red[(w * MT + mt) * 64 + lane];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float u = s[q] + bv[q];
      v[e][q] = do_lrelu ? lrelu_f(u, p.slope) : u;
    }
  }
  bf16_t* y = reinterpret_cast<bf16_t*>(p.y);
  const size_t img = (size_t)b * p.H * p.W;
  if (!pool) {
#pragma unroll
    for (int e = 0; e < EB; ++e) {
      const int pix = (wid * EB + e) * 16 + r, row = pix / W, col = pix - row * W;
      const size_t op = img + (size_t)(y0 + row) * p.W + col;
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = v[e][q] * p.out_scale;
      if (!nok) continue;
      if (do_mask) {
        float m[4];
        Ty<bf16_t>::ld4(reinterpret_cast<const bf16_t*>(p.aux) + op * p.aux_cs + n, m);
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] *= lmask_f(m[q], p.slope);
      }
      bf16_t* dst = y + op * p.y_cs + n;
      if (do_acc) {
        float t[4];
        Ty<bf16_t>::ld4(dst, t);
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] += t[q];
      }
      Ty<bf16_t>::st4(dst, o);
    }
    return;
  }
  // 2x2 pool: horizontal partner lane r ^ 1; vertical partner lane r ^ W (W < 16) or the
  // paired block (W == 16)
  float h[4];
  const int pix0 = (wid * EB) * 16 + r, row0 = pix0 / W, col0 = pix0 - row0 * W;
#pragma unroll
  for (int e = 0; e < EB; ++e) {
    if (p.y2 && nok) {
      const int pix = (wid * EB + e) * 16 + r, row = pix / W, col = pix - row * W;
      Ty<bf16_t>::st4(reinterpret_cast<bf16_t*>(p.y2) +
                          (img + (size_t)(y0 + row) * p.W + col) * p.y2_cs + n, v[e]);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float sm = v[0][q] + __shfl_xor(v[0][q], 1, 64);
    if constexpr (EB == 2) {
      sm += v[1][q] + __shfl_xor(v[1][q], 1, 64);
    } else {
      sm += __shfl_xor(sm, W, 64);
    }
    h[q] = sm * p.out_scale;
  }
  if (nok && (col0 & 1) == 0 && (row0 & 1) == 0) {
    const size_t op = ((size_t)b * (p.H >> 1) + ((y0 + row0) >> 1)) * (p.W >> 1) + (col0 >> 1);
    bf16_t* dst = y + op * p.y_cs + n;
    if (do_acc) {
      float t[4];
      Ty<bf16_t>::ld4(dst, t);
#pragma unroll
      for (int q = 0; q < 4; ++q) h[q] += t[q];
    }
    Ty<bf16_t>::st4(dst, h);
  }
}

bool conv_lr_nch_ok(int cin);

// Which convs take this path: bf16, W = H in {4, 8}, 32-multiple input channels,
// epilogues without PixelNorm / sign bits (those stay on conv3x3_kernel's split-K path)
bool conv_lr_ok(const pg_conv_desc* d) {
  // 16^2 stays on the split-K path: 32 pixel tiles re-stream the 4.7 MB weight slab 32
  // times (measured 34 us against 20 us split-K); at 4^2 / 8^2 conv_lr wins (10 vs 13-15 us,
  // 14 vs 15-21 us, tools/lr_ab.sh)
  if (d->W != d->H || (d->W != 4 && d->W != 8)) return false;
  if (!conv_lr_nch_ok(d->cin) || d->cout % 4 != 0) return false;
  if (d->flags & (PG_CONV_PIXNORM | PG_CONV_PNBWD | PG_CONV_Y2_BITS | PG_CONV_AUX_BITS | PG_CONV_X_BITS))
    return false;
  if ((d->flags & PG_CONV_MASK) && (d->flags & PG_CONV_POOL)) return false;
  return true;
}

template <int W, int TH, int NCH>
int launch_conv_lr(const pg_conv_desc* d, const ConvArgs& a, hipStream_t st) {
  const ConvParams p = conv_params(d, a);
  PG_CHECK_ARG(p.cin_p == NCH * 32 && d->H % TH == 0 && d->x_cs >= p.cin_p && (d->x_cs % 8) == 0,
               "conv_lr: bad geometry (H %d, x_cs %d, cin_p %d)", d->H, d->x_cs, p.cin_p);
  const int halo = (TH + 2) * (W + 2) * (p.cin_p * 2 + 32);
  const int red = PG_LR_NW * (TH * W / 16) * 64 * 16;
  const int lds = halo > red ? halo : red;
  PG_CHECK_ARG(lds <= 160 * 1024, "conv_lr: LDS %d too large", lds);
  PG_LDS_ATTR((conv_lr_kernel<W, TH, NCH>), 160 * 1024);
  dim3 grid(d->B * (d->H / TH), p.cout_p / 16);
  PG_KLAUNCH((conv_lr_kernel<W, TH, NCH>), grid, dim3(64 * PG_LR_NW), lds, st, p);
  PG_LAUNCH_CHECK();
  return PG_OK;
}

template <int W, int TH>
int conv_lr_nch(const pg_conv_desc* d, const ConvArgs& a, hipStream_t st) {
  switch (cinp_of(d->cin) / 32) {
    case 1: return launch_conv_lr<W, TH, 1>(d, a, st);
    case 2: return launch_conv_lr<W, TH, 2>(d, a, st);
    case 4: return launch_conv_lr<W, TH, 4>(d, a, st);
    case 8: return launch_conv_lr<W, TH, 8>(d, a, st);
    case 16: return launch_conv_lr<W, TH, 16>(d, a, st);
    case 17: return launch_conv_lr<W, TH, 17>(d, a, st);
  }
  PG_CHECK_ARG(false, "conv_lr: no kernel for cin %d", d->cin);
  return PG_ERR_ARG;
}

bool conv_lr_nch_ok(int cin) {
  const int n = cinp_of(cin) / 32;
  return cinp_of(cin) % 32 == 0 && (n == 1 || n == 2 || n == 4 || n == 8 || n == 16 || n == 17);
}

int conv_lr_dispatch(const pg_conv_desc* d, const ConvArgs& a, hipStream_t st) {
  switch (d->W) {
    case 4: return conv_lr_nch<4, 4>(d, a, st);
    case 8:
      // whole-image tiles when that still gives 256 workgroups (the merged passes, B = 8):
      // each 16-channel weight slab is streamed by 8 workgroups instead of 16, 17.7 -> 14.0 us
      // per launch (profiles/r5_lowres_tiles.txt)
      if (d->B >= 8) return conv_lr_nch<8, 8>(d, a, st);
      return conv_lr_nch<8, 4>(d, a, st);
  }
  return PG_ERR_ARG;
}
