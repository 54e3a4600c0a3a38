// Included inside conv.hip's anonymous namespace, after conv_hr.inc (uses WgBParams, tr_read8,
// hr_dma16, lds_void_t, the WG_* reduction modes).  The kernel only: which launches it takes,
// and with which plan, is in the LDS-DMA rows of WG_ROWS (conv.hip).
//
// wgrad_dma_kernel: the bf16 3x3 weight gradient of every layer with exact 16 MO / 16 WNC
// channel blocks and whole 8 x 16 tiles (narrow and wide layers alike), dW[o][c][tap] = sum_p gz[p][o] * x[p + tap][c].  It began as the wide layers' kernel
// and is described for them: the same MFMA decomposition as wgrad_bf16_kernel<4, 1, 1, 2> (a
// workgroup owns 64 o x 32 c x 9 taps, K = pixels in 128-pixel tiles of 8 x 16, fragments by
// ds_read_b64_tr_b16) but staged the way conv_hr's wide tiles are:
//
//   * LDS-DMA (buffer_load_dwordx4 ... lds, hr_dma16): each tile's gz rows (128 x 64 ch, 128 B
//     per pixel) and its input halo (10 x 18 pixels x 32 ch, 64 B per pixel) go global -> LDS
//     with no register staging, no zero-fill selects (out-of-image halo pixels get an offset
//     past the buffer range: the hardware loads zeros) and no ds_write; 32 pieces of 1 KiB per
//     tile, 4 per wave, into a 3- or 4-slot ring (WgdGeo::NSLOT) with two or three tiles in flight per barrier.
//     wgrad_bf16_kernel stages through registers: per tile and wave 210 VALU (selects,
//     address math), 130 SALU and 61 LDS instructions beside 72 MFMAs, at one wave per SIMD.
//   * dense LDS rows with XOR-swizzled 16-B slots instead of padding (the DMA writes whole
//     1-KiB pieces): gz row r holds slot s of the 64 channels at slot s ^ ((r & 2) | (r & 8) >> 1),
//     halo pixel P slot s at s ^ (((P >> 3) & 1) * 2) -- the transposed reads of one k-step
//     (rows {0..3, 8..11} + const per 32-lane group) hit 32 distinct bank pairs.
//   * 8 waves, two per SIMD: waves split a tile's four 32-pixel k-steps (wk) and the two
//     16-channel halves (wc); the four k-step partials are summed through LDS at the end in
//     wave order (deterministic).  Every LDS read offset is a per-lane constant computed once
//     (52 registers), so the k-loop issues MFMAs and ds_reads only.
//
// Bias gradient (c-block 0 only): summed from the staged gz rows in LDS.  Split over pixels
// (blockIdx.z) as wgrad_select plans it; the reduction modes are those of
// wgrad_bf16_kernel (WG_DIRECT / WG_SLABS + wgrad_slab_reduce*).  An in-launch combine of the
// slabs (the last split of each output tile summing them in split order) measured slower at
// every split count (64^2 57.0 vs 44.3 us, step 353.0 vs 356.9 img/s,
// profiles/r5_wgrad_combine_ab.txt): the last arriver's serial read is exposed.
// Reference: lib/layers.py:58-89 (autograd's conv2d weight gradient), SURVEY 8(a) a1.

constexpr int WGD_TH = 8, WGD_TW = 16, WGD_BP = WGD_TH * WGD_TW;   // 128-pixel tiles
constexpr int WGD_HPIX = (WGD_TH + 2) * (WGD_TW + 2);               // 180 halo pixels
// tile ring depth: NSLOT - 1 tiles in flight across each barrier.  Four slots for the 32-64
// output-channel gradients (the step: 10.147 -> 10.071 ms with four everywhere; the 1024^2
// 16 -> 32 sign-bit gradient 113.7 -> 107.2 us), three for the 16-output-channel ones, whose
// fourth slot costs a resident workgroup per CU (1024^2 16 -> 16: 56.9 -> 64.3 us)
#ifndef PG_WGD_NSLOT
#define PG_WGD_NSLOT 4
#endif

// Geometry of one instantiation: MO 16-channel o-blocks per wave (BO = 16 MO gz channels per
// workgroup), WNC 16-channel input halves (BC = 16 WNC), 4 x WNC waves (4 k-steps per tile).
template <int MO, int WNC, bool GZB = false>
struct WgdGeo {
  static constexpr int NW = 4 * WNC, NTHR = 64 * NW, KW = 4;
  static constexpr int GRB = 32 * MO, HPB = 32 * WNC;            // bytes per gz row / halo pixel
  static constexpr int GP = WGD_BP * GRB / 1024;                 // gz pieces
  static constexpr int HP = (WGD_HPIX * HPB + 1023) / 1024;      // halo pieces
  static constexpr int NPC = (GP + HP + NW - 1) / NW * NW;       // padded: the same count per wave
  static constexpr int PPW = NPC / NW;
  // GZ_BITS: the lrelu' bits of each gz piece's pixels (BO / 8 bytes each) land in 256 B
  // behind the pieces (one dword DMA per gz piece; lanes past the piece's pixels load zeros)
  static constexpr int GPW = GP / NW;                            // gz pieces per wave
  static constexpr int BITS = GZB ? GP * 256 : 0;
  static constexpr int SLOT = NPC * 1024 + BITS;
  static constexpr int RED = NW * 2304 * 4;                      // epilogue: one o-block per wave
  static constexpr int NSLOT = MO == 1 ? 3 : PG_WGD_NSLOT;
  static_assert(NSLOT >= 3 && NSLOT <= 4, "wgrad_dma: ring of 3-4 slots");
  static constexpr int LDS = NSLOT * SLOT > RED ? NSLOT * SLOT : RED;
};

// LDS placement (conflict-free ds_read_b64_tr_b16: each 32-lane group reads rows / pixels
// {x .. x+3, x+8 .. x+11} + const): position of a gz row r / halo pixel P and the XOR applied
// to its 16-B slot index.  128-B rows: slot ^ ((r & 2) | (r & 8) >> 1); 64-B rows: slot ^
// 2 * bit 3; 32-B rows (one bank octet each, so rows r and r + 8 cannot be separated by a slot
// XOR): the rows themselves permuted, r ^ (bit 3 << 2).  All are involutions.
template <int RB>
__device__ __forceinline__ int wgd_pos(int r) { return RB == 32 ? r ^ (((r >> 3) & 1) << 2) : r; }
template <int RB>
__device__ __forceinline__ int wgd_swz(int r) {
  return RB == 128 ? ((r & 2) | ((r & 8) >> 1)) : RB == 64 ? ((r >> 3) & 1) * 2 : 0;
}

// LDS-DMA of one dword per lane (lane l's 4 B at dst + 4 l), as hr_dma16
__device__ __forceinline__ void wgd_dma4(const void* base, unsigned nrec, lds_void_t* dst, unsigned voff) {
  const size_t a = (size_t)base;
  const unsigned alo = __builtin_amdgcn_readfirstlane((unsigned)a);
  const unsigned ahi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(((size_t)ahi << 32) | alo), 0, __builtin_amdgcn_readfirstlane(nrec), 0x00020000);
  const unsigned m0v = __builtin_amdgcn_readfirstlane((unsigned)(size_t)dst);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\tbuffer_load_dword %2, %3, 0 offen lds\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep) : "s"(m0v), "v"(voff), "s"(rs) : "memory");
}

// GZB (PG_CONV_GZ_BITS, the discriminator's conv-b weight gradients at 512^2 / 1024^2): gz =
// up2(g) * lrelu'(bits).  The gz pieces are DMA'd from the half-resolution g (each row's
// address from its pixel >> 1: the upsample is free), the bits of the same pixels land behind
// them, and each wave masks its OWN pieces in LDS once its vmcnt wait has seen them arrive --
// before the tile's barrier, so no extra barrier and no register staging.
template <int MO, int WNC, bool GZB>
__global__ __launch_bounds__(256 * WNC) void wgrad_dma_kernel(WgBParams p) {   // = WgdGeo::NTHR
#if defined(__HIP_DEVICE_COMPILE__)
  using G = WgdGeo<MO, WNC, GZB>;
  static_assert(!GZB || (G::GP % G::NW == 0 && MO >= 2), "wgrad_dma: GZB needs whole gz pieces per wave");
  constexpr int NW = G::NW, NTHR = G::NTHR, KW = G::KW, GRB = G::GRB, HPB = G::HPB;
  constexpr int BO = 16 * MO, BC = 16 * WNC;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wk = wid % KW, wc = wid / KW;
  const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, pq = i16 & 3;
  // XCD-aware block order, as wgrad_bf16_kernel: a pixel split's workgroups share one L2
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (p.xcd_remap) {
    const int ox = gridDim.x, oy = gridDim.y;
    const int n = ox * oy * gridDim.z;
    const int h = bx + ox * (by + oy * bz);
    const int xcd = h & 7, slot = h >> 3, qq = n >> 3, rr = n & 7;
    const int Lg = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + slot;
    bx = Lg % ox;
    by = (Lg / ox) % oy;
    bz = Lg / (ox * oy);
  }
  const int o0 = bx * BO, c0 = by * BC;
  const bool do_db = p.db && by == 0;

  // ---- DMA of tile t into a ring slot: piece k = wid + NW * j of every wave; the tile origin
  // enters as scalars, the lane's row / slot from its position in the piece
  const unsigned OOB = 0x7fff0000u;
  const int gH = GZB ? p.H >> 1 : p.H, gW = GZB ? p.W >> 1 : p.W;
  const unsigned gz_nrec = (unsigned)((size_t)p.B * gH * gW * p.gz_cs * 2);
  const unsigned gzb_nrec = GZB ? (unsigned)((size_t)p.B * p.H * p.W * p.gzb_cs) : 0u;
  constexpr int PPP = 1024 / GRB;   // pixels per gz piece
  const unsigned x_nrec = (unsigned)((size_t)p.B * p.Hin * p.Win * p.x_cs * 2);
  const int ys = p.ups ? 1 : 0;
  auto dma_tile = [&](int t, char* base) __attribute__((always_inline)) {
    const int tx0 = (t & (p.tiles_x - 1)) * WGD_TW;
    const int tt = t >> p.lg_tx;
    const int ty0 = (tt & (p.tiles_y - 1)) * WGD_TH;
    const int b = tt >> p.lg_ty;
#pragma unroll
    for (int j = 0; j < G::PPW; ++j) {
      const int k = wid + NW * j;   // wave-uniform
      if (k < G::GP) {
        constexpr int SPR = GRB / 16;                     // slots per gz row
        const int pos = k * (1024 / GRB) + lane / SPR;    // LDS row of this lane's 16 B
        const int r = wgd_pos<GRB>(pos), s = (lane % SPR) ^ wgd_swz<GRB>(r);
        const int py = ty0 + (r >> 4), px = tx0 + (r & 15);
        const int gy = GZB ? py >> 1 : py, gx = GZB ? px >> 1 : px;
        const unsigned v = (unsigned)((((b * gH + gy) * gW + gx) * p.gz_cs + o0 + 8 * s) * 2);
        hr_dma16(p.gz, gz_nrec, (lds_void_t*)(base + k * 1024), v, 0);
        if constexpr (GZB) {   // bits: lane = (pixel of the piece, dword of its BO / 8 bytes)
          constexpr int DPP = BO / 32;
          const int pi = lane / DPP;
          unsigned vb = OOB;
          if (pi < PPP) {
            const int r2 = k * PPP + pi;   // GRB >= 64: rows are not permuted
            const int qy = ty0 + (r2 >> 4), qx = tx0 + (r2 & 15);
            vb = (unsigned)(((b * p.H + qy) * p.W + qx) * p.gzb_cs + (o0 >> 3) + 4 * (lane % DPP));
          }
          wgd_dma4(p.gzb, gzb_nrec, (lds_void_t*)(base + G::NPC * 1024 + k * 256), vb);
        }
      } else {
        constexpr int SPP = HPB / 16;                     // slots per halo pixel
        const int pos = (k - G::GP) * (1024 / HPB) + lane / SPP;
        const int P = wgd_pos<HPB>(pos), s = (lane % SPP) ^ wgd_swz<HPB>(P);
        const int hy = P / (WGD_TW + 2), hx = P - hy * (WGD_TW + 2);
        const int yy = ty0 + hy - 1, xx = tx0 + hx - 1;
        unsigned v = OOB;
        if (P < WGD_HPIX && (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W)
          v = (unsigned)((((b * p.Hin + (yy >> ys)) * p.Win + (xx >> ys)) * p.x_cs + c0 + 8 * s) * 2);
        hr_dma16(p.x, x_nrec, (lds_void_t*)(base + k * 1024), v, 0);
      }
    }
  };

  // ---- per-lane LDS read offsets inside a slot (k-step wk of every tile): A = gz rows rA /
  // rB (= rA + 4) of o-block mo; B = halo pixels of rA / rB shifted by each tap
  const int rA = wk * 32 + 8 * g + q, rB = rA + 4;
  auto off_gz = [&](int r, int ol) { return wgd_pos<GRB>(r) * GRB + 16 * ((ol >> 3) ^ wgd_swz<GRB>(r)) + 2 * (ol & 7); };
  // (for 64- and 128-B rows rB keeps rA's swizzle: bits 1 and 3 unchanged, so it is a constant
  // 4 rows on; 32-B rows are permuted and need their own offsets)
  constexpr int NA = GRB == 32 ? 2 : 1;
  int offA[MO][NA], offB[9][2];
#pragma unroll
  for (int mo = 0; mo < MO; ++mo) {
    const int ol = mo * 16 + 4 * pq;
    offA[mo][0] = off_gz(rA, ol);
    if constexpr (NA == 2) offA[mo][NA - 1] = off_gz(rB, ol);
  }
  {
    const int cl = wc * 16 + 4 * pq;
    const int hA = (rA >> 4) * (WGD_TW + 2) + (rA & 15), hB = (rB >> 4) * (WGD_TW + 2) + (rB & 15);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int toff = (tap / 3) * (WGD_TW + 2) + (tap % 3);
      const int PA = hA + toff, PB = hB + toff;
      offB[tap][0] = G::GP * 1024 + wgd_pos<HPB>(PA) * HPB + 16 * ((cl >> 3) ^ wgd_swz<HPB>(PA)) + 2 * (cl & 7);
      offB[tap][1] = G::GP * 1024 + wgd_pos<HPB>(PB) * HPB + 16 * ((cl >> 3) ^ wgd_swz<HPB>(PB)) + 2 * (cl & 7);
    }
  }

  f32x4_t acc[MO][9];
#pragma unroll
  for (int a = 0; a < MO; ++a)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[a][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float bs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bs[e] = 0.f;

  auto compute = [&](const char* sb) __attribute__((always_inline)) {
    bf16x8_t A[MO];
#pragma unroll
    for (int mo = 0; mo < MO; ++mo)
      A[mo] = tr_read8(reinterpret_cast<const bf16_t*>(sb + offA[mo][0]),
                       reinterpret_cast<const bf16_t*>(sb + (NA == 2 ? offA[mo][NA - 1] : offA[mo][0] + 4 * GRB)));
    bf16x8_t Bc = tr_read8(reinterpret_cast<const bf16_t*>(sb + offB[0][0]),
                           reinterpret_cast<const bf16_t*>(sb + offB[0][1]));
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const bf16x8_t Bn = tap + 1 < 9 ? tr_read8(reinterpret_cast<const bf16_t*>(sb + offB[tap + 1][0]),
                                                 reinterpret_cast<const bf16_t*>(sb + offB[tap + 1][1]))
                                      : Bc;
#pragma unroll
      for (int mo = 0; mo < MO; ++mo)
        acc[mo][tap] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[mo], Bc, acc[mo][tap], 0, 0, 0);
      Bc = Bn;
    }
  };
  // bias gradient of c-block 0: thread = channel slot v = tid % GV of rows (tid + NTHR j) / GV
  constexpr int GV = BO / 8;
  auto bias_tile = [&](const char* sb) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < (WGD_BP * GV + NTHR - 1) / NTHR; ++j) {
      const int idx = tid + NTHR * j;
      if ((WGD_BP * GV) % NTHR != 0 && idx >= WGD_BP * GV) break;
      const int r = idx / GV, v = idx % GV;
      const u32x4_t u = *reinterpret_cast<const u32x4_t*>(
          sb + wgd_pos<GRB>(r) * GRB + 16 * (v ^ wgd_swz<GRB>(r)));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bs[2 * e] += bf_lo(u[e]);
        bs[2 * e + 1] += bf_hi(u[e]);
      }
    }
  };

  // ---- the tile ring: tile i in slot i % 3, tiles i+1 and i+2 in flight across its barrier
  const int t_begin = bz * p.tiles_per_split;
  const int t_end = min(p.ntiles, t_begin + p.tiles_per_split);
  const int n = t_end - t_begin;
  auto slot = [&](int i) -> char* { return smem + (i % G::NSLOT) * G::SLOT; };
  // GZB: this wave's gz pieces of a landed tile times lrelu'(bits), in place (lane = its own
  // DMA lane: 16 B at piece + 16 lane, pixel lane / SPR, channel slot s)
  auto mask_tile = [&](char* sb) __attribute__((always_inline)) {
    constexpr int SPR = GRB / 16;
#pragma unroll
    for (int j = 0; j < G::GPW; ++j) {
      const int k = wid + NW * j;
      const int pos = k * PPP + lane / SPR;
      const int s = (lane % SPR) ^ wgd_swz<GRB>(pos);
      const int m = *reinterpret_cast<const unsigned char*>(sb + G::NPC * 1024 + k * 256 + (lane / SPR) * (BO / 8) + s);
      // up2(g) * lrelu'(bits), rounded as the unfused gz (branch-free)
      u32x4_t* q = reinterpret_cast<u32x4_t*>(sb + k * 1024 + lane * 16);
      *q = lrelu_mask_bf16x8(*q, (unsigned)m, p.slope);
    }
  };
  constexpr int OPT = G::PPW + (GZB ? G::GPW : 0);   // vector-memory ops per tile and wave
  constexpr int DEPTH = G::NSLOT - 1;                 // tiles in flight
#pragma unroll
  for (int d = 0; d < DEPTH; ++d)
    if (d < n) dma_tile(t_begin + d, slot(d));
  for (int i = 0; i < n; ++i) {
    // tile i landed: the younger tiles i+1 .. i+DEPTH-1 (those that exist) may stay in flight
    const int younger = min(DEPTH - 1, n - 1 - i);
    if (younger >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * OPT) : "memory");
    else if (younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * OPT) : "memory");
    else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(OPT) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (GZB) mask_tile(slot(i));
    // every wave's pieces of tile i have landed; every wave is done reading tile i-1's slot,
    // which tile i+DEPTH overwrites next
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (i + DEPTH < n) dma_tile(t_begin + i + DEPTH, slot(i + DEPTH));
    compute(slot(i));
    if (do_db) bias_tile(slot(i));
  }

  // ---- epilogue (wgrad_bf16_kernel's): bias gradient, then per o-block the four k-step
  // partials summed through LDS in wave order and written in [o][c][tap] runs
  float* red = reinterpret_cast<float*>(smem);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
  if (do_db) {
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid * 8 + e] = bs[e];
    __syncthreads();
    if (tid < BO && o0 + tid < p.cout) {
      const int v = tid >> 3, e = tid & 7;
      float s = 0.f;
      for (int r = v; r < NTHR; r += GV) s += red[r * 8 + e];
      const int o = o0 + tid;
      if (p.mode == WG_SLABS)
        p.ws[bz * p.slab + (size_t)p.cout * p.cin * 9 + o] = s;
      else
        atomicAdd(p.db + o, s * p.scale);
    }
  }
  float* slab = p.mode == WG_SLABS ? p.ws + bz * p.slab : nullptr;
#pragma unroll 1
  for (int a = 0; a < MO; ++a) {
    __syncthreads();
    float* mine = red + (size_t)wid * 2304 + ((lane >> 4) * 64 + (lane & 15)) * 9;
#pragma unroll
    for (int mo = 0; mo < MO; ++mo)
      if (mo == a) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int j = 0; j < 4; ++j) mine[j * 16 * 9 + t] = acc[mo][t][j];
      }
    __syncthreads();
    constexpr int NOUT = WNC * 2304;   // channel halves x 16 o x 16 c x 9 taps
    constexpr int NPT = NOUT / NTHR;
    static_assert(NPT * NTHR == NOUT, "wgrad_dma: epilogue split");
    float v[NPT];
    int offs[NPT];
#pragma unroll
    for (int k2 = 0; k2 < NPT; ++k2) {
      const int e = tid + NTHR * k2;
      const int m = e / 2304, rem = e - m * 2304;   // m = channel half
      const int ol = rem / 144, rem2 = rem - ol * 144;
      const int cl = rem2 / 9, tap = rem2 - cl * 9;
      float sum = 0.f;
#pragma unroll
      for (int k = 0; k < KW; ++k) sum += red[(size_t)(m * KW + k) * 2304 + rem];
      const int o = o0 + a * 16 + ol;
      const int c = c0 + m * 16 + cl;
      v[k2] = sum;
      offs[k2] = (o < p.cout && c < p.cin) ? (o * p.cin + c) * 9 + tap : -1;
    }
    if (p.mode == WG_DIRECT) {
#pragma unroll
      for (int k2 = 0; k2 < NPT; ++k2)
        if (offs[k2] >= 0) atomicAdd(p.dw + offs[k2], v[k2] * p.scale);
    } else {
#pragma unroll
      for (int k2 = 0; k2 < NPT; ++k2)
        if (offs[k2] >= 0) slab[offs[k2]] = v[k2];
    }
  }
#endif
}
