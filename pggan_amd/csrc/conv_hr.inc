// Included inside conv.hip's anonymous namespace (uses ConvParams, Ty, lrelu_f, ...).
//
// conv_hr_kernel: bf16 3x3 convolution for spatial sizes >= 16 (no image batching in a
// tile), with the tile geometry, channel chunk and K loop fixed at compile time so the
// per-pixel index arithmetic is shifts and multiplies by constants.
//
//   tile     : TH rows x 16 columns of one image (BM = 16*TH output pixels)
//   waves    : NWAVES, wave w owns output rows [w*MT, (w+1)*MT), MT = TH/NWAVES pixel blocks
//   MFMA     : D[cout][pixel] (v_mfma_f32_16x16x32_bf16, A = packed weights [n][tap*CK+c],
//              B = halo pixel shifted by the tap, 8 channels per lane) -> NT = BN/16 blocks
//   epilogue : direct: lane holds 4 consecutive output channels of one pixel; bias, leaky
//              relu, lrelu' mask (aux loads issued before the MFMAs), 2x2 pool (+ y2), ACCUM
//
// PERSIST (all input channels in one chunk): a workgroup keeps the BN x 9 x CK weight
// slab resident in LDS and walks output tiles blockIdx.x, +gridDim.x, ...; the halo of
// the next tile is fetched into registers while the current tile's MFMAs run.
// !PERSIST: one tile per workgroup (blockIdx.y = output-channel block), looping over the
// CK-channel chunks with the next chunk's halo + weights fetched one chunk ahead.

// MODE selects the sign-bit variants at compile time (plain variants carry none of it):
//   0 plain, HR_XB input masked by X_BITS, HR_YB Y2_BITS output, HR_AB AUX_BITS mask,
//   HR_XAB both X_BITS input and AUX_BITS mask
enum { HR_PLAIN = 0, HR_XB = 1, HR_YB = 2, HR_AB = 3, HR_XAB = 4 };

// A/B build switches (tools/ab_build.sh with AB_EXTRA): order pinning in the 8-wave k-loop,
// and the software-pipelined k-loop for the 8-wave tiles
#ifndef PG_HR_NOSB
#define PG_HR_NOSB 0
#endif
#ifndef PG_HR_PIPE8
#define PG_HR_PIPE8 0
#endif

// PD: persistent variants keep the halos of the next PD tiles in flight (register ring)
#ifndef PG_HR_NARROW_WPE
#define PG_HR_NARROW_WPE 1
#endif
// minimum waves per SIMD the register allocation must allow: the persistent narrow tiles
// (CK = 16, BN <= 32: small LDS image) are HBM-latency bound, so occupancy = bytes in flight
template <int CK, int TH, int BN, bool PERSIST, int NWAVES>
constexpr int hr_wpe() {
  return (PERSIST && CK == 16 && BN <= 32 && NWAVES == 4) ? PG_HR_NARROW_WPE : 1;
}

// DB (non-persistent tiles only): two LDS images of the chunk; chunk c+1 is fetched into
// registers before chunk c's MFMAs and written into the other image between its k-steps,
// so each chunk costs one barrier and no stall on the staging writes
// DMA (non-persistent, CK = 32, no input masking): the chunk's halo and weights go
// global -> LDS by buffer_load ... lds into two LDS images (XOR-swizzled instead of
// padded, so both fit: 2 x 75 KiB); chunk c+1 is in flight during chunk c's MFMAs and
// each chunk costs one barrier and no staging VALU / ds_write (see hr_dma_* below).
template <int CK, int TH, int BN>
struct HrDma {
  static constexpr int TW2 = 18, HPIX = (TH + 2) * TW2;
  static constexpr int HPIECES = (HPIX * (CK / 8) + 63) / 64;   // 1-KiB wave pieces
  static constexpr int HREG = HPIECES * 1024;
  static constexpr int WROW = 9 * CK * 2;                       // 9 taps x CK channels
  static constexpr int WPIECES = (BN * 9 * (CK / 8) + 63) / 64;
  static constexpr int WREG = WPIECES * 1024;
  static constexpr int BUF = HREG + WREG;
};
// the 16-B slot swizzle: slot bit 1 ^= bit 2 of the halo column / weight row (conflict-free
// ds_read_b128 fragment reads for every tap shift: brute-force check in tools/lds_banks.py)
__device__ __forceinline__ int hr_swz(int x) { return ((x >> 2) & 1) << 1; }
typedef __attribute__((address_space(3))) void lds_void_t;
// 16 bytes per lane global -> LDS (buffer_load_dwordx4 ... lds): LDS address M0 + 16 * lane.
// Inline asm so the compiler does not track it (see the DMA branch of conv_hr_kernel): the
// caller waits for it with an explicit s_waitcnt vmcnt.  M0 is a reserved register the
// compiler does not accept in a clobber list, so the asm saves whatever M0 holds in a scratch
// SGPR and restores it after the load: a value the compiler keeps in M0 survives.
// The buffer resource is built here from the base address and byte range, every scalar
// operand through readfirstlane: the asm takes them as "s" operands, and where the compiler
// kept one in VGPRs (a value carried around the persistent form's loop) it would not assemble.
__device__ __forceinline__ void hr_dma16(const void* base, unsigned nrec, lds_void_t* dst,
                                         unsigned voff, unsigned soff) {
  const size_t a = (size_t)base;
  const unsigned alo = __builtin_amdgcn_readfirstlane((unsigned)a);
  const unsigned ahi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(((size_t)ahi << 32) | alo), 0, __builtin_amdgcn_readfirstlane(nrec), 0x00020000);
  soff = __builtin_amdgcn_readfirstlane(soff);
  const unsigned m0v = __builtin_amdgcn_readfirstlane((unsigned)(size_t)dst);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep) : "s"(m0v), "v"(voff), "s"(rs), "s"(soff) : "memory");
}

// EF >= 0 (persistent tiles): the launch's flags as a compile-time constant (| HR_EF_Y2 when
// y2 is given) and an EXACT launch: cout == BN and every workgroup walks the same number of
// tiles.  Every flag branch then folds away, the tile loop has no exit test inside and the
// epilogue stores are unconditional (lanes that duplicate a pooled value or a sign-bit word
// store the same bytes), so the loop body is straight-line and the compiler counts the
// in-flight loads exactly: a runtime-flag epilogue's branches made it drain every load and
// every store of the previous tile (vmcnt(0)) before staging each halo, which left these
// HBM-bound kernels latency bound (2.8 of ~5 TB/s).  The lrelu' mask operands of a tile are
// loaded before the next tile's halo, so waiting for them never waits for that prefetch.
constexpr int HR_EF_Y2 = 1 << 20;
template <int CK, int TH, int BN, bool PERSIST, int NWAVES, int MODE, int PD = 1, bool DB = false,
          bool DMA = false, int EF = -1>
__global__ __launch_bounds__(NWAVES * 64) __attribute__((amdgpu_waves_per_eu(hr_wpe<CK, TH, BN, PERSIST, NWAVES>())))
void conv_hr_kernel(ConvParams p) {
  constexpr bool EXACT = EF >= 0;
  static_assert(!EXACT || (PERSIST && !DB && !DMA), "EF: persistent tiles only");
  const int pfl = EXACT ? EF : p.flags;
  constexpr int NTHR = NWAVES * 64;
  constexpr int TW = 16, TW2 = 18, TH2 = TH + 2;
  constexpr int MT = TH / NWAVES, NT = BN / 16;
  constexpr int VPP = CK / 8;                        // 16-byte vectors per halo pixel
  constexpr int KS = (9 * CK + 31) / 32;             // 32-deep k-steps per chunk
  constexpr int NTP = KS * 32 / CK;                  // taps incl. zero padding
  // row paddings that make the ds_read_b128 fragment reads bank-conflict free
  // (tools/lds_banks.py): halo pixel 64 B -> 96 B, weight row +32 B
  constexpr int PIXB = CK * 2 + (CK * 2 >= 64 ? 32 : 0);
  constexpr int WROWB = KS * 64 + 32;
  constexpr int HALO_BYTES = (TH2 * TW2 * PIXB + 15) & ~15;
  constexpr int NHV = TH2 * TW2 * VPP;               // halo vectors per chunk
  constexpr int NWV = BN * NTP * VPP;                // weight vectors per chunk
  constexpr int NH = (NHV + NTHR - 1) / NTHR;
  constexpr int NW = (NWV + NTHR - 1) / NTHR;
  constexpr int UNR = NWAVES > 4 ? 3 : KS;             // k-step unroll (register budget)
  static_assert(TH % NWAVES == 0 && CK % 8 == 0, "geometry");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BUF_BYTES = HALO_BYTES + BN * WROWB;   // one LDS image of a chunk
  char* halo = smem;
  char* wl = smem + HALO_BYTES;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform (SGPR)
  const int g = lane >> 4, r = lane & 15;
  // one-tile-per-workgroup variants: (tile, output-channel block) of this workgroup.  With
  // p.xcd_remap the hardware's round-robin dealing over the 8 XCDs (block h on XCD h % 8, speed
  // only) is undone so that XCD k owns a contiguous band of logical ids, the output-channel
  // block fastest: the blocks of one tile (same halo) and the neighbouring tiles (overlapping
  // halos) run behind one L2, and every conv of a level reads the rows the XCD's previous
  // conv of that level wrote (same band of the same images), which are still in its L2.
  int tile_id = blockIdx.x, cblk = blockIdx.y;
  if (!PERSIST && p.xcd_remap) {
    const int gx = gridDim.x, gy = gridDim.y, n = gx * gy;
    const int h = blockIdx.x + gx * blockIdx.y;
    const int xcd = h & 7, slot = h >> 3, q = n >> 3, rr = n & 7;
    const int Lg = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + slot;
    cblk = Lg % gy;
    tile_id = Lg / gy;
  }
  const int n0 = PERSIST ? 0 : cblk * BN;
  const bool ups = (pfl & PG_CONV_UPS_IN) != 0;
  const int ys = ups ? 1 : 0;
  const bf16_t* xs = reinterpret_cast<const bf16_t*>(p.x);
  const bf16_t* wsrc = reinterpret_cast<const bf16_t*>(p.w);

  // halo staging plan: packed (hy, hx, v) of this thread's vectors, -1 = none
  int hpk[NH];
#pragma unroll
  for (int k = 0; k < NH; ++k) {
    const int i = tid + NTHR * k;
    const int hp = i / VPP, v = i - hp * VPP;
    const int hy = hp / TW2, hx = hp - hy * TW2;
    hpk[k] = i < NHV ? (hy << 16) | (hx << 8) | v : -1;
  }
  constexpr bool xbits_on = MODE == HR_XB || MODE == HR_XAB;
  // X_BITS (always with UPS_IN): the staging items are the 8-channel vectors of the HALF-
  // resolution input window of the tile ((TH/2 + 2) x (TW/2 + 2) pixels), each loaded and
  // scaled by the slope once; store_halo writes its up to four full-resolution children (the
  // 2x2 block it up-samples to, where inside the halo) by selecting per element between g and
  // slope * g with the child's sign bits -- instead of one clamped up2 load and eight
  // multiplies per full-resolution vector.  Item plan: (hy2 << 16) | (hx2 << 8) | (children in
  // the halo << 4) | vector, -1 = none; hl2 = LDS offset of child (0, 0); hg2 / hb2 = the
  // in-image element offset of the vector / byte offset of child (0, 0)'s sign bits relative to
  // the window origin (kernel constants: the per-tile part is one scalar each)
  constexpr int TW2H = TW / 2 + 2, NI2 = (TH / 2 + 2) * TW2H * VPP;
  constexpr int NH2 = xbits_on ? (NI2 + NTHR - 1) / NTHR : 1;
  static_assert(!xbits_on || (TH % 2 == 0 && VPP <= 16), "X_BITS staging plan");
  int hpk2[NH2], hl2[NH2], hg2[NH2], hb2[NH2];
#pragma unroll
  for (int k = 0; k < NH2; ++k) {
    const int i = tid + NTHR * k;
    const int hp = i / VPP, v = i - hp * VPP;
    const int hy2 = hp / TW2H, hx2 = hp - hy2 * TW2H;
    int cm = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int hy = 2 * hy2 - 1 + (c >> 1), hx = 2 * hx2 - 1 + (c & 1);
      cm |= (hy >= 0 && hy < TH2 && hx >= 0 && hx < TW2) ? 1 << c : 0;
    }
    hpk2[k] = (xbits_on && i < NI2) ? (hy2 << 16) | (hx2 << 8) | (cm << 4) | v : -1;
    hl2[k] = ((2 * hy2 - 1) * TW2 + 2 * hx2 - 1) * PIXB + v * 16;
    hg2[k] = (hy2 * p.Win + hx2) * p.x_cs + 8 * v;
    hb2[k] = (2 * hy2 * p.W + 2 * hx2) * p.xb_cs + v;
  }
  // weight staging plan: element offset of this thread's vectors (without chunk base)
  int wsoff[NW];
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    const int i = tid + NTHR * k;
    const int row = i / (NTP * VPP), rem = i - row * (NTP * VPP);
    const int tap = rem / VPP, v = rem - tap * VPP;
    const int n = n0 + row;
    wsoff[k] = (i < NWV && tap < 9 && n < p.cout_p) ? (n * 9 + tap) * p.cin_p + 8 * v : -1;
  }
  auto w_lds = [&](int k) {
    const int i = tid + NTHR * k;
    const int row = i / (NTP * VPP), rem = i - row * (NTP * VPP);
    const int tap = rem / VPP, v = rem - tap * VPP;
    return row * WROWB + tap * CK * 2 + v * 16;
  };
  auto h_lds = [&](int k) {
    const int i = tid + NTHR * k;
    const int hp = i / VPP, v = i - hp * VPP;
    return hp * PIXB + v * 16;
  };

  // per-lane LDS offsets of the pixel fragments and of the tap shifts
  int hoff[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) hoff[mt] = ((wid * MT + mt) * TW2 + r) * PIXB;
  const int tiles_x = p.W / TW, tiles_y = p.H / TH;
  const int ntiles = p.B * tiles_x * tiles_y;
  u32x4_t hbr[PD][NH], wb[NW];
  // PG_CONV_X_BITS: the input is lrelu'-masked on load by sign bits at conv resolution
  // (one byte per staged 8-channel vector), e.g. x = up2(g) * lrelu'(bits) for the
  // input gradient of a conv followed by leaky-relu + 2x2 pool
  // X_BITS: the select-mask table behind the chunk image and the 16-B scratch slot
  // (launch_conv_hr adds them): entry e (a byte of sign bits, 8 elements) = four dwords whose
  // 16-bit halves are all ones where the element's bit is clear (that element takes slope * g);
  // written here, read after the first barrier
  char* xlut = smem + BUF_BYTES * (DB ? 2 : 1) + 16;
  if constexpr (xbits_on) {
    static_assert(NTHR >= 256, "X_BITS: one table entry per thread");
    if (tid < 256) {
      u32x4_t e;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        e[j] = ((tid >> (2 * j)) & 1 ? 0u : 0x0000ffffu) | ((tid >> (2 * j + 1)) & 1 ? 0u : 0xffff0000u);
      *reinterpret_cast<u32x4_t*>(xlut + tid * 16) = e;
    }
  }
  // sign bits per staging item: the four children's bytes (X_BITS) / unused
  constexpr int NHB = xbits_on ? 4 * NH2 : NH;
  int hbitsr[PD][NHB];
  unsigned hokr[PD];   // bit k: halo vector k is inside the image (else staged as zero)

  auto fetch_halo = [&](int t, int c0, u32x4_t (&hb)[NH], int (&hbits)[NHB], unsigned& hok) {
    // tile -> (image, tile row, tile column); the tile counts are powers of two
    const int tx0 = (t & (tiles_x - 1)) * TW;
    const int tt = t >> p.lg_tx;
    const int ty0 = (tt & (tiles_y - 1)) * TH;
    const int b = tt >> p.lg_ty;
    // image base in SGPRs; per-lane offsets inside one image fit 32 bits (<= 1024^2 x 512 ch)
    const bf16_t* xb = xs + (size_t)b * p.Hin * p.Win * p.x_cs + c0;
    const unsigned char* xbb = xbits_on ? p.xbits + (size_t)b * p.H * p.W * p.xb_cs + (c0 >> 3) : nullptr;
    // branch-free: every lane loads (out-of-image lanes read a clamped in-bounds address)
    // and the zero fill is applied when the registers are written to LDS, so nothing
    // touches the loaded values until then and the loads stay in flight across the MFMAs
    // (a load under a per-lane branch or a select right after it makes hipcc wait, vmcnt)
    hok = 0;
    if constexpr (xbits_on) {
      // half-resolution items (see hpk2): the vector once, the four children's sign bytes
      const int Y0 = (ty0 >> 1) - 1, X0 = (tx0 >> 1) - 1;
      // the window origin's offsets (negative at the image's top / left edge: only in-image
      // items use them, the others read offset 0)
      const int g0 = (Y0 * p.Win + X0) * p.x_cs, b0 = (2 * Y0 * p.W + 2 * X0) * p.xb_cs;
      const unsigned bstep = p.xb_cs, brow = p.W * p.xb_cs;
      unsigned go[NH2], bo[NH2];
#pragma unroll
      for (int k = 0; k < NH2; ++k) {
        const int pk = hpk2[k];
        const int Y = Y0 + (pk >> 16), X = X0 + ((pk >> 8) & 0xff);
        const bool ok = (pk >= 0) & ((unsigned)Y < (unsigned)p.Hin) & ((unsigned)X < (unsigned)p.Win);
        go[k] = ok ? (unsigned)(g0 + hg2[k]) : 0u;
        bo[k] = ok ? (unsigned)(b0 + hb2[k]) : 0u;
        hok |= (ok ? 1u : 0u) << k;
      }
      // the offsets are selected before any load (opaque to the compiler, which otherwise
      // splits a load into two predicated ones with a vmcnt(0) between them), then every load
      // of the window goes out back to back: scalar bases + 32-bit lane offsets
#pragma unroll
      for (int k = 0; k < NH2; ++k) asm volatile("" : "+v"(go[k]), "+v"(bo[k]));
#pragma unroll
      for (int k = 0; k < NH2; ++k) hb[k] = *reinterpret_cast<const u32x4_t*>(xb + go[k]);
#pragma unroll
      for (int k = 0; k < NH2; ++k) {
        hbits[4 * k + 0] = xbb[bo[k]];
        hbits[4 * k + 1] = xbb[bo[k] + bstep];
        hbits[4 * k + 2] = xbb[bo[k] + brow];
        hbits[4 * k + 3] = xbb[bo[k] + brow + bstep];
      }
      return;
    }
#pragma unroll
    for (int k = 0; k < NH; ++k) {
      const int pk = hpk[k];
      const int yy = ty0 + (pk >> 16) - 1, xx = tx0 + ((pk >> 8) & 0xff) - 1;
      const bool ok = pk >= 0 && (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W;
      const int yc = ok ? yy : 0, xc = ok ? xx : 0, vc = ok ? (pk & 0xff) : 0;
      hb[k] = *reinterpret_cast<const u32x4_t*>(
          xb + (unsigned)(((yc >> ys) * p.Win + (xc >> ys)) * p.x_cs + 8 * vc));
      hok |= (ok ? 1u : 0u) << k;
    }
  };
  unsigned wok = 0;
#pragma unroll
  for (int k = 0; k < NW; ++k) wok |= (wsoff[k] >= 0 ? 1u : 0u) << k;
  auto fetch_w = [&](int c0) {
#pragma unroll
    for (int k = 0; k < NW; ++k)
      wb[k] = *reinterpret_cast<const u32x4_t*>(wsrc + (wsoff[k] >= 0 ? wsoff[k] + c0 : 0));
  };
  auto store_halo = [&](const u32x4_t (&hb)[NH], const int (&hbits)[NHB], unsigned hok) {
    if constexpr (xbits_on) {
      // each half-resolution vector g: slope * g once (bf16-rounded per element, as
      // round(g * slope) of the full-resolution form), then per child a bitwise select by
      // its sign bits; children outside the halo write the scratch slot (branch-free)
#pragma unroll
      for (int k = 0; k < NH2; ++k) {
        const int pk = hpk2[k];
        const u32x4_t gv = ((hok >> k) & 1u) ? hb[k] : u32x4_t{0u, 0u, 0u, 0u};
        typedef __attribute__((ext_vector_type(2))) float f2_t;
        const f2_t sl = {p.slope, p.slope};
        u32x4_t gs;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f2_t e = f2_t{__uint_as_float(gv[i] << 16), __uint_as_float(gv[i] & 0xffff0000u)} * sl;
          gs[i] = pack_bf16x2(e[0], e[1]);
        }
        const int cm = pk >= 0 ? (pk >> 4) & 15 : 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const unsigned m = (unsigned)hbits[4 * k + c];   // a zero-extended byte
          const u32x4_t mk = *reinterpret_cast<const u32x4_t*>(xlut + (m << 4));
          u32x4_t o;
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] = (mk[i] & gs[i]) | (~mk[i] & gv[i]);
          const int off = hl2[k] + (c >> 1) * TW2 * PIXB + (c & 1) * PIXB;
          *reinterpret_cast<u32x4_t*>(halo + (((cm >> c) & 1) ? off : BUF_BYTES)) = o;
        }
      }
      return;
    }
#pragma unroll
    for (int k = 0; k < NH; ++k) {
      // EXACT: lanes past the halo write a 16-B scratch slot behind the LDS image (no
      // per-lane branch in the loop body)
      if (!EXACT && tid + NTHR * k >= NHV) continue;
      const u32x4_t v = ((hok >> k) & 1u) ? hb[k] : u32x4_t{0u, 0u, 0u, 0u};
      *reinterpret_cast<u32x4_t*>(halo + (tid + NTHR * k < NHV ? h_lds(k) : BUF_BYTES)) = v;
    }
  };
  auto store_w = [&]() {
#pragma unroll
    for (int k = 0; k < NW; ++k)
      if (tid + NTHR * k < NWV)
        *reinterpret_cast<u32x4_t*>(wl + w_lds(k)) = ((wok >> k) & 1u) ? wb[k] : u32x4_t{0u, 0u, 0u, 0u};
  };
  // DB: staging vector j of the chunk (halo vectors 0..NH-1, then weight vectors) written
  // into the LDS image at `base` (plain halo: the X_BITS masking is not used with DB)
  auto store_one = [&](int j, char* base, const u32x4_t (&hb)[NH], unsigned hok) {
    if (j < NH) {
      if (tid + NTHR * j < NHV)
        *reinterpret_cast<u32x4_t*>(base + h_lds(j)) =
            ((hok >> j) & 1u) ? hb[j] : u32x4_t{0u, 0u, 0u, 0u};
    } else {
      const int k = j - NH;
      if (tid + NTHR * k < NWV)
        *reinterpret_cast<u32x4_t*>(base + HALO_BYTES + w_lds(k)) =
            ((wok >> k) & 1u) ? wb[k] : u32x4_t{0u, 0u, 0u, 0u};
    }
  };

  f32x4_t acc[MT][NT];
  // fragment reads of k-step ks: weights (A, one per nt block) and the tap-shifted halo
  // pixel block mt (B)
  auto frag_w = [&](int ks, int nt) {
    return *reinterpret_cast<const bf16x8_t*>(wl + (nt * 16 + r) * WROWB + (ks * 32 + 8 * g) * 2);
  };
  auto frag_x = [&](int ks, int mt) {
    const int k0 = ks * 32 + 8 * g;
    int tap = k0 / CK;
    const int c = k0 - tap * CK;
    tap = tap > 8 ? 8 : tap;   // padded taps: weights are zero, read real data
    const int to = ((tap / 3) * TW2 + (tap % 3)) * PIXB + c * 2;
    return *reinterpret_cast<const bf16x8_t*>(halo + hoff[mt] + to);
  };
  // software-pipelined: the B fragment of the next (ks, mt) block is read before this
  // block's MFMAs, and each A fragment of k-step ks+1 right after its last use in ks, so
  // an MFMA group never waits on the LDS read issued just before it
  auto mma_chunk_plain = [&]() {
#pragma unroll UNR
    for (int ks = 0; ks < KS; ++ks) {
      bf16x8_t wf[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) wf[nt] = frag_w(ks, nt);
      bf16x8_t xf = frag_x(ks, 0);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        // the next pixel block's fragment is read before this block's MFMAs (order pinned)
        const bf16x8_t xn = mt + 1 < MT ? frag_x(ks, mt + 1) : xf;
#if !PG_HR_NOSB
        __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], xf, acc[mt][nt], 0, 0, 0);
#if !PG_HR_NOSB
        __builtin_amdgcn_sched_barrier(0);
#endif
        xf = xn;
      }
    }
  };
  auto mma_chunk_pipe_h = [&](auto&& after_kstep) {
    bf16x8_t wf[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wf[nt] = frag_w(0, nt);
    bf16x8_t xf = frag_x(0, 0);
#pragma unroll UNR
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const bool lastm = mt + 1 == MT;
        const bf16x8_t xn = !lastm ? frag_x(ks, mt + 1) : frag_x(ks + 1 < KS ? ks + 1 : ks, 0);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], xf, acc[mt][nt], 0, 0, 0);
          if (lastm && ks + 1 < KS) wf[nt] = frag_w(ks + 1, nt);
        }
        xf = xn;
      }
      after_kstep(ks);
    }
  };
  auto mma_chunk_pipe = [&]() { mma_chunk_pipe_h([](int) {}); };
  // the 8-wave tiles have no registers left for the pipelined form (it spills there)
  auto mma_chunk = [&]() {
    if constexpr (NWAVES > 4 && !PG_HR_PIPE8) mma_chunk_plain();
    else mma_chunk_pipe();
  };

  const bool has_bias = (pfl & PG_CONV_BIAS) != 0;
  const bool do_lrelu = (pfl & PG_CONV_LRELU) != 0;
  const bool do_mask = (pfl & PG_CONV_MASK) != 0;
  const bool do_acc = (pfl & PG_CONV_ACCUM) != 0;
  const bool pool = (pfl & PG_CONV_POOL) != 0;
  bf16_t* y = reinterpret_cast<bf16_t*>(p.y);
  bf16_t* y2 = reinterpret_cast<bf16_t*>(p.y2);
  const bool has_y2 = EXACT ? (EF & HR_EF_Y2) != 0 : p.y2 != nullptr;
  const bf16_t* aux = reinterpret_cast<const bf16_t*>(p.aux);
  float bv[NT][4];
  auto load_bias = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + nt * 16 + 4 * g + j;
        bv[nt][j] = (has_bias && n < p.cout) ? p.bias[n] : 0.f;
      }
  };
  // the persistent DMA form (PD == 2 on the 8-wave LDS-DMA tile) reloads the bias before each
  // epilogue instead of holding 16 registers across its loop
  if constexpr (!(DMA && DB && NWAVES > 4 && PD == 2)) load_bias();

  const bool do_pn = (pfl & PG_CONV_PIXNORM) != 0;
  // PG_CONV_RGBW (EF tiles): the result (the gradient gz at the fromRGB output) is not stored;
  // each lane accumulates gz[n] * img[i] and gz[n] of its pixels for its 4 channels per nt
  // block (racc[nt][j][i], i = 3: the bias term) and the grid sums them after the tile loop
  constexpr bool rgbw = EXACT && ((EF & PG_CONV_RGBW) != 0);
  // PG_CONV_RGBD (EF tiles): the result is not stored either; the fromRGB input gradient
  // gimg = f W^T gz of each pixel is written (fp32 NCHW), its squared norm summed per sample
  // (the penalties' norms) and, with p.rdw, the R1 tangent's fromRGB weight term
  // rdw += rscale sum gz (x) gimg accumulated in racc
  constexpr bool rgbd = EXACT && ((EF & PG_CONV_RGBD) != 0);
  // PG_CONV_RGBO (EF tiles, PixelNorm forward): the toRGB output img = f2 (W y + rb) of each
  // pixel from the stored (bf16) y, written fp32 NCHW
  constexpr bool rgbo = EXACT && ((EF & PG_CONV_RGBO) != 0);
  float wrg[NT][4][3];   // RGBD / RGBO: the fromRGB / toRGB weights of this lane's channels
  float nq = 0.f;        // RGBD: squared norm of this lane's gimg since the last tile
  if constexpr (rgbd) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) wrg[nt][j][k] = p.rw[(nt * 16 + 4 * g + j) * 3 + k];
  }
  if constexpr (rgbo) {   // toRGB weights [3][cout] (cout == BN: EXACT)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) wrg[nt][j][k] = p.rw[k * BN + nt * 16 + 4 * g + j];
  }
  float racc[NT][4][4];
  float iq[MT][3];   // this tile's image values at the lane's pixels (loaded with the masks)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) racc[nt][j][i] = 0.f;
  auto rgbw_acc = [&](int mt, int nt, const float (&v)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int i = 0; i < 3; ++i) racc[nt][j][i] += v[j] * iq[mt][i];
      racc[nt][j][3] += v[j];
    }
  };
  // RGBD, one pixel (image b, row, col) with this lane's channel values vv[nt][j]: every lane
  // of the pixel gets gimg by two xor-shuffles over the channel groups; the g == 0 lanes store
  // it and count its squared norm
  auto rgbd_px = [&](int b, int row, int col, const float* vv) __attribute__((always_inline)) {
    float q[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] += vv[nt * 4 + j] * wrg[nt][j][k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      q[k] += __shfl_xor(q[k], 16, 64);
      q[k] += __shfl_xor(q[k], 32, 64);
      q[k] *= p.f2;
    }
    if (g == 0) {
      const size_t plane = (size_t)p.H * p.W;
      float* dst = p.gimg + (size_t)b * 3 * plane + (size_t)row * p.W + col;
#pragma unroll
      for (int k = 0; k < 3; ++k) dst[k * plane] = q[k];
      nq += q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
    }
    if (p.rdw) {   // uniform
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int k = 0; k < 3; ++k) racc[nt][j][k] += vv[nt * 4 + j] * q[k];
    }
  };
  // PG_CONV_PNBWD (tiles of <= 32 channels): the y operand is read like a MASK operand
  const bool do_pnb = BN <= 32 && (pfl & PG_CONV_PNBWD) != 0;
  float rpn[MT];
  constexpr bool aux_bits = MODE == HR_AB || MODE == HR_XAB;
  constexpr bool y2_bits = MODE == HR_YB;
  // lrelu' mask of this lane's 4 channels: from bf16 activations, or from the 16 sign bits
  // of its nt block (AUX_BITS; lane group g owns bits 4g..4g+3)
  auto apply_mask = [&](float (&v)[4], const u32x2_t& m) {
    if constexpr (aux_bits) {
      const unsigned nib = (m[0] >> (4 * g)) & 0xfu;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (!((nib >> j) & 1u)) v[j] *= p.slope;
    } else {
      v[0] *= lmask_f(bf_lo(m[0]), p.slope);
      v[1] *= lmask_f(bf_hi(m[0]), p.slope);
      v[2] *= lmask_f(bf_lo(m[1]), p.slope);
      v[3] *= lmask_f(bf_hi(m[1]), p.slope);
    }
  };
  // 16 sign bits (v > 0) of one pixel's nt block gathered from its 4 lane groups; valid in
  // the g == 0 lanes.  All 64 lanes must call it.
  auto sign_bits16 = [&](const float (&v)[4]) -> unsigned {
    unsigned nib = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) nib |= (v[j] > 0.f ? 1u : 0u) << j;
    const unsigned own = EXACT ? (unsigned)__shfl(nib, r, 64) : nib;   // EXACT: same word in every g
    return own | ((unsigned)__shfl(nib, r + 16, 64) << 4) | ((unsigned)__shfl(nib, r + 32, 64) << 8) |
           ((unsigned)__shfl(nib, r + 48, 64) << 12);
  };
  auto epilogue = [&](int t, const u32x2_t (&am)[MT][NT]) {
    // tile -> (image, tile row, tile column); the tile counts are powers of two
    const int tx0 = (t & (tiles_x - 1)) * TW;
    const int tt = t >> p.lg_tx;
    const int ty0 = (tt & (tiles_y - 1)) * TH;
    const int b = tt >> p.lg_ty;
    // per-image bases (scalar); in-image pixel offsets lp / lop are 32-bit
    const size_t img = (size_t)b * p.H * p.W;
    bf16_t* yi = y + img * p.y_cs;
    bf16_t* yo = y + (img >> 2) * p.y_cs;   // pooled output image
    if constexpr (BN <= 32) {
      if (do_pnb && !pool) {
        // PixelNorm + LReLU backward of the result v (= dL/dy): every cout channel of a
        // pixel is in this wave (4 per lane per nt block, lane groups g); y (am) and r (rpn)
        // were loaded with the mask operands, ahead of the MFMAs
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const int lp = (ty0 + wid * MT + mt) * p.W + tx0 + r;
          float gv[NT][4], yv[NT][4];
          float dot = 0.f;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const bool ok = nt * 16 + 4 * g < p.cout;
            yv[nt][0] = bf_lo(am[mt][nt][0]); yv[nt][1] = bf_hi(am[mt][nt][0]);
            yv[nt][2] = bf_lo(am[mt][nt][1]); yv[nt][3] = bf_hi(am[mt][nt][1]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              gv[nt][j] = ok ? acc[mt][nt][j] * p.out_scale : 0.f;
              if (!ok) yv[nt][j] = 0.f;
              dot += yv[nt][j] * gv[nt][j];
            }
          }
          dot += __shfl_xor(dot, 16, 64);
          dot += __shfl_xor(dot, 32, 64);
          const float rn = rpn[mt];
          const float m = dot / (float)p.cout;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const int n = nt * 16 + 4 * g;
            if (!EXACT && n >= p.cout) continue;
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = rn * (gv[nt][j] - yv[nt][j] * m) * lmask_f(yv[nt][j], p.slope);
            Ty<bf16_t>::st4(yi + (unsigned)(lp * p.y_cs + n), o);
          }
        }
        return;
      }
    }
    if (do_pn) {
      // PixelNorm over all cout channels of a pixel: 4 per lane per nt block, the 4 lane
      // groups g hold the rest (n0 == 0, cout_p <= BN checked on the host)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int lp = (ty0 + wid * MT + mt) * p.W + tx0 + r;
        float v[NT][4];
        float ss = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float u = acc[mt][nt][j] + bv[nt][j];
            if (do_lrelu) u = lrelu_f(u, p.slope);
            u = bf2f(f2bf(u));                 // the activation as stored (bf16)
            v[nt][j] = (nt * 16 + 4 * g + j < p.cout) ? u : 0.f;
            ss += v[nt][j] * v[nt][j];
          }
        ss += __shfl_xor(ss, 16, 64);
        ss += __shfl_xor(ss, 32, 64);
        const float rn = rsqrtf(ss / (float)p.cout + 1e-8f);
        float q[3] = {0.f, 0.f, 0.f};   // RGBO
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const int n = nt * 16 + 4 * g;
          if (!EXACT && n >= p.cout) continue;
          float o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = v[nt][j] * rn;
          Ty<bf16_t>::st4(yi + (unsigned)(lp * p.y_cs + n), o);
          if constexpr (rgbo) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float ys = bf2f(f2bf(o[j]));   // y as stored
#pragma unroll
              for (int k = 0; k < 3; ++k) q[k] += ys * wrg[nt][j][k];
            }
          }
        }
        if (has_y2 && (EXACT || g == 0)) (reinterpret_cast<float*>(p.y2) + img)[lp] = rn;
        if constexpr (rgbo) {
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            q[k] += __shfl_xor(q[k], 16, 64);
            q[k] += __shfl_xor(q[k], 32, 64);
          }
          if (g == 0) {
            const size_t plane = (size_t)p.H * p.W;
            float* dst = p.gimg + (size_t)b * 3 * plane + lp;
#pragma unroll
            for (int k = 0; k < 3; ++k) dst[k * plane] = p.f2 * (q[k] + p.rb[k]);
          }
        }
      }
      return;
    }
    if constexpr (NT == 2) {
      // cout tile 32 (a pixel = 64 B): one v_permlane16_swap per packed dword pair gives
      // every lane 8 consecutive channels, so each store instruction writes whole 64-B
      // pixel lines (16 B per lane) instead of two half lines 8 B per lane
      if (!EXACT && n0 + 32 > p.cout) goto narrow;   // both nt blocks must be real channels
      {
        const int cb = n0 + (g & 1) * 16 + (g >> 1) * 8;   // channel base after the swap
        auto swap_store = [&](bf16_t* dst, const float (&a)[4], const float (&c)[4], bool st,
                              bool accum) {
          uint32_t A0 = pack_bf16x2(a[0], a[1]), A1 = pack_bf16x2(a[2], a[3]);
          uint32_t B0 = pack_bf16x2(c[0], c[1]), B1 = pack_bf16x2(c[2], c[3]);
          auto s0 = __builtin_amdgcn_permlane16_swap(A0, B0, false, false);
          auto s1 = __builtin_amdgcn_permlane16_swap(A1, B1, false, false);
          u32x4_t q = u32x4_t{s0[0], s1[0], s0[1], s1[1]};
          if (!st) return;
          if (accum) {
            const u32x4_t o = *reinterpret_cast<const u32x4_t*>(dst);
#pragma unroll
            for (int i = 0; i < 4; ++i)
              q[i] = pack_bf16x2(bf_lo(q[i]) + bf_lo(o[i]), bf_hi(q[i]) + bf_hi(o[i]));
          }
          *reinterpret_cast<u32x4_t*>(dst) = q;
        };
        uint32_t bw2[MT];   // Y2_BITS: 32 sign bits per pre-pool pixel (both nt blocks)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) bw2[mt] = 0;
        bf16_t* y2i = y2 ? y2 + img * p.y2_cs : nullptr;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const int row = ty0 + wid * MT + mt;
          const int lp = row * p.W + tx0 + r;
          float v[2][4];
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              v[nt][j] = acc[mt][nt][j] + bv[nt][j];
              if (do_lrelu) v[nt][j] = lrelu_f(v[nt][j], p.slope);
            }
          if (!pool) {
            // Y2_BITS without the pool: the sign bits of the activation itself (the lrelu'
            // operand of the consumers' MASK), 32 per pixel
            if constexpr (y2_bits) bw2[mt] = sign_bits16(v[0]) | (sign_bits16(v[1]) << 16);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
              for (int j = 0; j < 4; ++j) v[nt][j] *= p.out_scale;
              if (do_mask) apply_mask(v[nt], am[mt][nt]);
            }
            if constexpr (rgbw) {
              rgbw_acc(mt, 0, v[0]);
              rgbw_acc(mt, 1, v[1]);
              continue;
            }
            if constexpr (rgbd) {
              const float vv[8] = {v[0][0], v[0][1], v[0][2], v[0][3], v[1][0], v[1][1], v[1][2], v[1][3]};
              rgbd_px(b, row, tx0 + r, vv);
              continue;
            }
            swap_store(yi + (unsigned)(lp * p.y_cs + cb), v[0], v[1], true, do_acc);
          } else {
            if (mt & 1) continue;
            float u[2][4], h[2][4];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                u[nt][j] = acc[mt + 1][nt][j] + bv[nt][j];
                if (do_lrelu) u[nt][j] = lrelu_f(u[nt][j], p.slope);
              }
            if (do_mask) {
#pragma unroll
              for (int nt = 0; nt < 2; ++nt) {
                apply_mask(v[nt], am[mt][nt]);
                apply_mask(u[nt], am[mt + 1][nt]);
              }
            }
            if constexpr (y2_bits) {
              bw2[mt] = sign_bits16(v[0]) | (sign_bits16(v[1]) << 16);
              bw2[mt + 1] = sign_bits16(u[0]) | (sign_bits16(u[1]) << 16);
            } else if (has_y2 && !do_pnb) {
              swap_store(y2i + (unsigned)(lp * p.y2_cs + cb), v[0], v[1], true, false);
              swap_store(y2i + (unsigned)((lp + p.W) * p.y2_cs + cb), u[0], u[1], true, false);
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const float sm = v[nt][j] + u[nt][j];
                h[nt][j] = (sm + __shfl_xor(sm, 1, 64)) * p.out_scale;
              }
            if (do_pnb) {
              // PixelNorm + LReLU backward of the pooled result (= dL/dy of the pooled pixel,
              // all 32 channels in this wave: 8 per lane over the lane groups g)
              float yv[2][4];
              float dot = 0.f;
#pragma unroll
              for (int nt = 0; nt < 2; ++nt) {
                yv[nt][0] = bf_lo(am[mt][nt][0]); yv[nt][1] = bf_hi(am[mt][nt][0]);
                yv[nt][2] = bf_lo(am[mt][nt][1]); yv[nt][3] = bf_hi(am[mt][nt][1]);
#pragma unroll
                for (int j = 0; j < 4; ++j) dot += yv[nt][j] * h[nt][j];
              }
              dot += __shfl_xor(dot, 16, 64);
              dot += __shfl_xor(dot, 32, 64);
              const float m = dot / (float)p.cout;
#pragma unroll
              for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                  h[nt][j] = rpn[mt] * (h[nt][j] - yv[nt][j] * m) * lmask_f(yv[nt][j], p.slope);
            }
            const int lop = (row >> 1) * (p.W >> 1) + ((tx0 + r) >> 1);
            swap_store(yo + (unsigned)(lop * p.y_cs + cb), h[0], h[1], EXACT || (r & 1) == 0, do_acc);
          }
        }
        if constexpr (y2_bits) {
          if (EXACT || g == 0) {
            unsigned char* yb = reinterpret_cast<unsigned char*>(p.y2) + img * p.y2_cs + (n0 >> 3);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              const int lp = (ty0 + wid * MT + mt) * p.W + tx0 + r;
              *reinterpret_cast<uint32_t*>(yb + (unsigned)(lp * p.y2_cs)) = bw2[mt];
            }
          }
        }
        return;
      }
    }
  narrow:
    // per-pixel sign bits of the pre-pool activation (PG_CONV_Y2_BITS), 16 per nt block
    uint64_t bw[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) bw[mt] = 0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = n0 + nt * 16 + 4 * g;
      if (!EXACT && n >= p.cout) continue;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int row = ty0 + wid * MT + mt;
        const int lp = row * p.W + tx0 + r;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = has_bias ? acc[mt][nt][j] + bv[nt][j] : acc[mt][nt][j];
          if (do_lrelu) v[j] = lrelu_f(v[j], p.slope);
        }
        if (!pool) {
          if constexpr (y2_bits) bw[mt] |= (uint64_t)sign_bits16(v) << (16 * nt);   // no pool
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] *= p.out_scale;
          if (do_mask) apply_mask(v, am[mt][nt]);
          if constexpr (rgbw) {
            rgbw_acc(mt, nt, v);
            continue;
          }
          if constexpr (rgbd) {   // NT == 1 (the 16-channel tile)
            rgbd_px(b, row, tx0 + r, v);
            continue;
          }
          bf16_t* dst = yi + (unsigned)(lp * p.y_cs + n);
          if (do_acc) {
            float o[4];
            Ty<bf16_t>::ld4(dst, o);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += o[j];
          }
          Ty<bf16_t>::st4(dst, v);
        } else {
          // 2x2 sum: horizontal partner lane ^ 1, vertical partner = row mt ^ 1 (same wave)
          if (mt & 1) continue;
          float u[4], h[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            u[j] = acc[mt + 1][nt][j] + bv[nt][j];
            if (do_lrelu) u[j] = lrelu_f(u[j], p.slope);
          }
          if (do_mask) {      // sign-bit mask at the pre-pool resolution (AUX_BITS)
            apply_mask(v, am[mt][nt]);
            apply_mask(u, am[mt + 1][nt]);
          }
          if constexpr (y2_bits) {
            bw[mt] |= (uint64_t)sign_bits16(v) << (16 * nt);
            bw[mt + 1] |= (uint64_t)sign_bits16(u) << (16 * nt);
          } else if (has_y2) {
            bf16_t* y2i = y2 + img * p.y2_cs;
            Ty<bf16_t>::st4(y2i + (unsigned)(lp * p.y2_cs + n), v);
            Ty<bf16_t>::st4(y2i + (unsigned)((lp + p.W) * p.y2_cs + n), u);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float s = v[j] + u[j];
            h[j] = s + __shfl_xor(s, 1, 64);
          }
          if (EXACT || (r & 1) == 0) {   // EXACT: both lanes of a pair store the same sum
            const int lop = (row >> 1) * (p.W >> 1) + ((tx0 + r) >> 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] *= p.out_scale;
            bf16_t* dst = yo + (unsigned)(lop * p.y_cs + n);
            if (do_acc) {
              float o[4];
              Ty<bf16_t>::ld4(dst, o);
#pragma unroll
              for (int j = 0; j < 4; ++j) h[j] += o[j];
            }
            Ty<bf16_t>::st4(dst, h);
          }
        }
      }
    }
    if (y2_bits && (EXACT || g == 0)) {   // compile-time off unless HR_YB
      unsigned char* yb = reinterpret_cast<unsigned char*>(p.y2) + img * p.y2_cs + (n0 >> 3);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int lp = (ty0 + wid * MT + mt) * p.W + tx0 + r;
        unsigned char* dst = yb + (unsigned)(lp * p.y2_cs);
        if constexpr (NT == 1)
          *reinterpret_cast<uint16_t*>(dst) = (uint16_t)bw[mt];
        else if constexpr (NT == 2)
          *reinterpret_cast<uint32_t*>(dst) = (uint32_t)bw[mt];
        else
          *reinterpret_cast<uint64_t*>(dst) = bw[mt];
      }
    }
  };
  // LDS-staged epilogue of the 64-channel LDS-DMA tiles (NT == 4).  The direct form above
  // stores 16 x 8 B per lane, each store instruction touching 16 pixel lines with 32 B: the
  // store tail was a quarter to a third of these launches (kbench with PG_HR_DIAG=4).  Here the
  // finished values go to LDS as [pixel][64 channels] rows of 144 B (the 8-B writes of a lane
  // group land on distinct banks), then every thread copies whole 16-B pieces, so a store
  // instruction writes 8 full 128-B pixel lines.  sfree: an LDS slot no wave reads any more
  // (not the last chunk's); slast: the last chunk's slot (free after the first barrier).
  // The arithmetic per element is the direct form's.
  constexpr int ORS = 144;
  auto stage4 = [&](char* st, int pl, int nt, const float (&o)[4]) {
    u32x2_t q;
    q[0] = pack_bf16x2(o[0], o[1]);
    q[1] = pack_bf16x2(o[2], o[3]);
    *reinterpret_cast<u32x2_t*>(st + pl * ORS + nt * 32 + g * 8) = q;
  };
  // NP staged rows of TC pixels each -> image rows row0.., columns col0.. of a Wo-wide image
  auto copy_out = [&](auto NPC, auto TCC, const char* st, bf16_t* dsti, int cs, int row0, int col0,
                      int Wo) {
    constexpr int NPX = decltype(NPC)::value, TCO = decltype(TCC)::value;
    constexpr int ITER = (NPX * 8 + NTHR - 1) / NTHR;
#pragma unroll
    for (int k = 0; k < ITER; ++k) {
      const int i = tid + k * NTHR;
      const int pl = i >> 3, sg = i & 7;
      const int n = n0 + sg * 8;
      if ((NPX * 8) % NTHR != 0 && i >= NPX * 8) break;
      const u32x4_t v = *reinterpret_cast<const u32x4_t*>(st + pl * ORS + sg * 16);
      if (n < p.cout) {
        const int gp = (row0 + pl / TCO) * Wo + col0 + pl % TCO;
        *reinterpret_cast<u32x4_t*>(dsti + (unsigned)(gp * cs + n)) = v;
      }
    }
  };
  // staging barrier: this wave's LDS writes are done and every wave has arrived (no vmcnt
  // wait: the persistent DMA form keeps the next job's DMAs in flight across it)
  auto lds_barrier = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  // sfree == slast (the persistent form has one free slot): the pre-pool copy is written out
  // before the pooled values are staged over it
  auto epilogue_lds = [&](int t, const u32x2_t (&am)[MT][NT], char* sfree, char* slast) {
    using NFULL = std::integral_constant<int, TH * 16>;
    using NPOOL = std::integral_constant<int, TH * 4>;
    using C16 = std::integral_constant<int, 16>;
    using C8 = std::integral_constant<int, 8>;
    const int tx0 = (t & (tiles_x - 1)) * TW;
    const int tt = t >> p.lg_tx;
    const int ty0 = (tt & (tiles_y - 1)) * TH;
    const int b = tt >> p.lg_ty;
    const size_t img = (size_t)b * p.H * p.W;
    bf16_t* yi = y + img * p.y_cs;
    bf16_t* yo = y + (img >> 2) * p.y_cs;
    if (do_pn) {   // every cout channel of a pixel in this wave (n0 == 0, cout_p <= 64)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int pl = (wid * MT + mt) * 16 + r;
        float v[NT][4];
        float ss = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float u = acc[mt][nt][j] + bv[nt][j];
            if (do_lrelu) u = lrelu_f(u, p.slope);
            u = bf2f(f2bf(u));
            v[nt][j] = (nt * 16 + 4 * g + j < p.cout) ? u : 0.f;
            ss += v[nt][j] * v[nt][j];
          }
        ss += __shfl_xor(ss, 16, 64);
        ss += __shfl_xor(ss, 32, 64);
        const float rn = rsqrtf(ss / (float)p.cout + 1e-8f);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          float o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = v[nt][j] * rn;
          stage4(sfree, pl, nt, o);
        }
        if (has_y2 && g == 0)
          (reinterpret_cast<float*>(p.y2) + img)[(ty0 + wid * MT + mt) * p.W + tx0 + r] = rn;
      }
      lds_barrier();
      copy_out(NFULL{}, C16{}, sfree, yi, p.y_cs, ty0, tx0, p.W);
      return;
    }
    if (!pool) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = n0 + nt * 16 + 4 * g;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const int pl = (wid * MT + mt) * 16 + r;
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[j] = acc[mt][nt][j] + bv[nt][j];
            if (do_lrelu) v[j] = lrelu_f(v[j], p.slope);
            v[j] *= p.out_scale;
          }
          if (do_mask) apply_mask(v, am[mt][nt]);
          if (do_acc && n < p.cout) {
            float o[4];
            Ty<bf16_t>::ld4(yi + (unsigned)(((ty0 + pl / 16) * p.W + tx0 + r) * p.y_cs + n), o);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += o[j];
          }
          stage4(sfree, pl, nt, v);
        }
      }
      lds_barrier();
      copy_out(NFULL{}, C16{}, sfree, yi, p.y_cs, ty0, tx0, p.W);
      return;
    }
    // 2x2 pool: horizontal partner lane ^ 1, vertical partner row mt ^ 1 (same wave)
    uint64_t bw[MT];
    float hh[MT / 2][NT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) bw[mt] = 0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = n0 + nt * 16 + 4 * g;
#pragma unroll
      for (int mt = 0; mt < MT; mt += 2) {
        const int pl = (wid * MT + mt) * 16 + r;
        float v[4], u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = acc[mt][nt][j] + bv[nt][j];
          u[j] = acc[mt + 1][nt][j] + bv[nt][j];
          if (do_lrelu) {
            v[j] = lrelu_f(v[j], p.slope);
            u[j] = lrelu_f(u[j], p.slope);
          }
        }
        if (do_mask) {   // sign-bit mask at the pre-pool resolution (AUX_BITS)
          apply_mask(v, am[mt][nt]);
          apply_mask(u, am[mt + 1][nt]);
        }
        if constexpr (y2_bits) {
          bw[mt] |= (uint64_t)sign_bits16(v) << (16 * nt);
          bw[mt + 1] |= (uint64_t)sign_bits16(u) << (16 * nt);
        } else if (has_y2) {
          stage4(sfree, pl, nt, v);
          stage4(sfree, pl + 16, nt, u);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float sm = v[j] + u[j];
          hh[mt / 2][nt][j] = (sm + __shfl_xor(sm, 1, 64)) * p.out_scale;
        }
        if (do_acc && n < p.cout) {
          const int lop = ((ty0 + wid * MT + mt) >> 1) * (p.W >> 1) + ((tx0 + r) >> 1);
          float o[4];
          Ty<bf16_t>::ld4(yo + (unsigned)(lop * p.y_cs + n), o);
#pragma unroll
          for (int j = 0; j < 4; ++j) hh[mt / 2][nt][j] += o[j];
        }
      }
    }
    if constexpr (y2_bits) {
      if (g == 0) {
        unsigned char* yb = reinterpret_cast<unsigned char*>(p.y2) + img * p.y2_cs + (n0 >> 3);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const int lp = (ty0 + wid * MT + mt) * p.W + tx0 + r;
          *reinterpret_cast<uint64_t*>(yb + (unsigned)(lp * p.y2_cs)) = bw[mt];
        }
      }
    }
    lds_barrier();   // every wave is past its MFMAs: the last chunk's slot is free too
    const bool shared = sfree == slast;
    if (shared && !y2_bits && has_y2) {
      copy_out(NFULL{}, C16{}, sfree, y2 + img * p.y2_cs, p.y2_cs, ty0, tx0, p.W);
      lds_barrier();
    }
    if ((r & 1) == 0) {
#pragma unroll
      for (int m2 = 0; m2 < MT / 2; ++m2)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          stage4(slast, (wid * (MT / 2) + m2) * 8 + (r >> 1), nt, hh[m2][nt]);
    }
    lds_barrier();
    if (!shared && !y2_bits && has_y2) copy_out(NFULL{}, C16{}, sfree, y2 + img * p.y2_cs, p.y2_cs, ty0, tx0, p.W);
    copy_out(NPOOL{}, C8{}, slast, yo, p.y_cs, ty0 >> 1, tx0 >> 1, p.W >> 1);
  };
  auto load_mask = [&](int t, u32x2_t (&am)[MT][NT]) {
    // tile -> (image, tile row, tile column); the tile counts are powers of two
    const int tx0 = (t & (tiles_x - 1)) * TW;
    const int tt = t >> p.lg_tx;
    const int ty0 = (tt & (tiles_y - 1)) * TH;
    const int b = tt >> p.lg_ty;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) am[mt][nt] = u32x2_t{0u, 0u};
    if (!do_mask && !do_pnb) return;   // uniform
    const size_t img = (size_t)b * p.H * p.W;
    if (do_pnb && pool) {
      // PNBWD after the 2x2 pool (BN == 32): y and r of the pooled pixel of rows mt, mt + 1
      // (in the even mt slots; lanes r and r ^ 1 share it)
#pragma unroll
      for (int mt = 0; mt < MT; mt += 2) {
        const int lop = ((ty0 + wid * MT + mt) >> 1) * (p.W >> 1) + ((tx0 + r) >> 1);
        rpn[mt] = reinterpret_cast<const float*>(p.y2)[(img >> 2) + lop];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          am[mt][nt] = *reinterpret_cast<const u32x2_t*>(aux + (img >> 2) * p.aux_cs +
                                                          (unsigned)(lop * p.aux_cs + n0 + nt * 16 + 4 * g));
      }
      return;
    }
    if (do_pnb) {   // PNBWD: r of this lane's pixels (am below holds its 4 channels of y)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        rpn[mt] = reinterpret_cast<const float*>(p.y2)[img + (ty0 + wid * MT + mt) * p.W + tx0 + r];
    }
    // branch-free per lane (clamped channel); lanes with n >= cout never use their mask
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int n = n0 + nt * 16 + 4 * g;
        const int lp = (ty0 + wid * MT + mt) * p.W + tx0 + r;
        if constexpr (aux_bits)
          am[mt][nt][0] = *reinterpret_cast<const uint16_t*>(
              reinterpret_cast<const unsigned char*>(p.aux) + img * p.aux_cs +
              (unsigned)(lp * p.aux_cs + ((n0 + nt * 16) >> 3)));
        else
          am[mt][nt] = *reinterpret_cast<const u32x2_t*>(aux + img * p.aux_cs +
                                                          (unsigned)(lp * p.aux_cs + (n < p.cout ? n : 0)));
      }
  };

  auto load_img = [&](int t) __attribute__((always_inline)) {
    const int tx0 = (t & (tiles_x - 1)) * TW;
    const int tt = t >> p.lg_tx;
    const int ty0 = (tt & (tiles_y - 1)) * TH;
    const int b = tt >> p.lg_ty;
    const size_t plane = (size_t)p.H * p.W;
    const float* ib = p.rimg + (size_t)b * 3 * plane;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const unsigned o = (unsigned)((ty0 + wid * MT + mt) * p.W + tx0 + r);
#pragma unroll
      for (int i = 0; i < 3; ++i) iq[mt][i] = ib[i * plane + o];
    }
  };
  if constexpr (PERSIST) {
    // tile t + d*G of this workgroup sits in ring slot d; the HBM latency of a halo is
    // covered by PD tiles of MFMAs + epilogue instead of one
    const int G = gridDim.x;
    float* nred = reinterpret_cast<float*>(smem + BUF_BYTES * (DB ? 2 : 1) + 16 +
                                           (xbits_on ? 4096 : 0));   // RGBD: [NWAVES][16]
    if constexpr (rgbd) {
      if (tid < NWAVES * 16) nred[tid] = 0.f;   // ordered by the loop's first barrier
    }
    fetch_w(0);
#pragma unroll
    for (int d = 0; d < PD; ++d)   // tiles past the end fetch the last tile (never stored)
      fetch_halo(min((int)blockIdx.x + d * G, ntiles - 1), 0, hbr[d], hbitsr[d], hokr[d]);
    store_w();
    for (int t0 = blockIdx.x; t0 < ntiles; t0 += PD * G) {
#pragma unroll
      for (int d = 0; d < PD; ++d) {
        const int t = t0 + d * G;
        if (EXACT || t < ntiles) {   // EXACT: ntiles % (PD * G) == 0 (host)
          __syncthreads();   // previous tile's fragments consumed
          store_halo(hbr[d], hbitsr[d], hokr[d]);
          __syncthreads();
          u32x2_t am[MT][NT];
          // EXACT: this tile's mask operands before the next halo (in-order load counting)
          if constexpr (EXACT) load_mask(t, am);
          if constexpr (rgbw) load_img(t);
          fetch_halo(min(t + PD * G, ntiles - 1), 0, hbr[d], hbitsr[d], hokr[d]);
          if constexpr (!EXACT) load_mask(t, am);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
          mma_chunk();
          epilogue(t, am);
          if constexpr (rgbd) {
            // this tile's squared norms: one image, so one sum per wave into its LDS slot
            const float sq = wave_sum(nq);
            nq = 0.f;
            if (lane == 0) nred[wid * 16 + (t >> (p.lg_tx + p.lg_ty))] += sq;
          }
        }
      }
    }
    if constexpr (rgbd) {
      // totals: [0, 16) the per-sample squared norms, then (channel, k) of the weight term
      constexpr int NA = 16 + BN * 4;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) racc[nt][j][i] += __shfl_xor(racc[nt][j][i], o, 64);
      float* red = reinterpret_cast<float*>(smem);
      float* tot = red + NWAVES * NA;
      float* tmp = tot + NA;
      __syncthreads();   // every wave is done with the halo image and its norm slots
      if (r == 0) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              red[wid * NA + 16 + (nt * 16 + 4 * g + j) * 4 + i] = i < 3 ? racc[nt][j][i] : 0.f;
      }
      if (lane < 16) red[wid * NA + lane] = nred[wid * 16 + lane];
      __syncthreads();
      for (int q = tid; q < NA; q += NTHR) {
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) sum += red[w * NA + q];
        tot[q] = sum;
      }
      __syncthreads();
      det_commit(tot, NA, p.scratch, tmp, [&](int q, float sum) {
        if (q < 16) {
          if (q < p.B && p.norms) p.norms[q] += sum;
          return;
        }
        const int n = (q - 16) >> 2, i = (q - 16) & 3;
        if (n < p.cout && i < 3 && p.rdw) p.rdw[n * 3 + i] += sum * p.rscale;
      });
    }
    if constexpr (rgbw) {
      // the lane's sums over its pixels -> over the 16 pixel lanes of its channel group ->
      // over the waves (LDS) -> over the grid in workgroup order (det_commit)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) racc[nt][j][i] += __shfl_xor(racc[nt][j][i], o, 64);
      constexpr int NA = BN * 4;   // (channel, term) totals
      float* red = reinterpret_cast<float*>(smem);
      float* tot = red + NWAVES * NA;
      float* tmp = tot + NA;
      __syncthreads();   // every wave is done with the halo image
      if (r == 0) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) red[wid * NA + (nt * 16 + 4 * g + j) * 4 + i] = racc[nt][j][i];
      }
      __syncthreads();
      for (int q = tid; q < NA; q += NTHR) {
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) sum += red[w * NA + q];
        tot[q] = sum;
      }
      __syncthreads();
      det_commit(tot, NA, p.scratch, tmp, [&](int q, float sum) {
        const int n = q >> 2, i = q & 3;
        if (n < p.cout) {
          if (i < 3) p.rdw[n * 3 + i] += sum * p.rscale;
          else if (p.rdb) p.rdb[n] += sum * p.rscale;
        }
      });
    }
  } else if constexpr (DMA) {
    static_assert(CK == 32 && !PERSIST && MODE != HR_XB && MODE != HR_XAB, "DMA: 32-channel chunks, unmasked input");
#if defined(__HIP_DEVICE_COMPILE__)   // buffer-resource builtins exist in the device pass only
    using L = HrDma<CK, TH, BN>;
    constexpr int NP = L::HPIECES + L::WPIECES;
    constexpr int NPW = (NP + NWAVES - 1) / NWAVES;   // pieces per wave (the last round partial)
    const int nch = p.cin_p / CK;
    // persistent form (PD == 2 on the 8-wave asm-DMA tile; p.tpw tiles per workgroup): this
    // workgroup computes tiles tile_id * tpw ... + tpw - 1 as one pipeline of (tile, chunk) jobs
    constexpr bool MULTI = DB && NWAVES > 4 && PD == 2;
    int t = MULTI ? tile_id * p.tpw : tile_id;
    // buffer resources: one input image, the packed weights; out-of-image halo slots and
    // padding slots get an offset past the range check, which loads zeros into LDS
    // one resource over the whole input (all images): a tile's image is an SGPR byte offset
    // added to every halo DMA (img_off), so the persistent form only recomputes scalars per tile
    const unsigned x_nrec = (unsigned)((size_t)p.B * p.Hin * p.Win * p.x_cs * 2);
    const unsigned w_nrec = (unsigned)(p.cout_p * 9 * p.cin_p * 2);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)xs, 0, x_nrec, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
        (void*)wsrc, 0, p.cout_p * 9 * p.cin_p * 2, 0x00020000);
    constexpr unsigned OOB = 0x7fff0000u;
    // NHWC input: a pixel's 32-channel chunk is 64 B at pixel stride x_cs
    const int x_ps = p.x_cs;
    constexpr unsigned x_cb2 = 64u;   // bytes per 32-channel chunk
    // DMA plan: byte offset of this lane's 16 B in piece k of tile tl's chunk (halo pieces
    // first, then weight pieces) and the tile's image offset.  Computed where a chunk is
    // issued (not held in registers): the persistent form keeps the next tile's DMAs in
    // flight across an epilogue, and a held plan spilled there.
    auto piece_off = [&](int k, int tl) __attribute__((always_inline)) -> unsigned {
      const int q = wid + NWAVES * k;
      unsigned v = OOB;
      if (q < L::HPIECES) {
        const int tx0 = (tl & (tiles_x - 1)) * TW;
        const int ty0 = ((tl >> p.lg_tx) & (tiles_y - 1)) * TH;
        const int sl = q * 64 + lane, P = sl >> 2;
        const int hy = P / TW2, hx = P - hy * TW2;
        const int j = (sl & 3) ^ hr_swz(hx);
        const int yy = ty0 + hy - 1, xx = tx0 + hx - 1;
        if (P < L::HPIX && (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W)
          v = (unsigned)((((yy >> ys) * p.Win + (xx >> ys)) * x_ps + 8 * j) * 2);
      } else if (q < NP) {
        const int sl = (q - L::HPIECES) * 64 + lane, nr = sl / (9 * 4), sr = sl - nr * 36;
        const int tap = sr >> 2, j = (sr & 3) ^ hr_swz(nr);
        if (nr < BN && n0 + nr < p.cout_p) v = (unsigned)((((n0 + nr) * 9 + tap) * p.cin_p + 8 * j) * 2);
      }
      return v;
    };
    auto img_off = [&](int tl) __attribute__((always_inline)) -> unsigned {
      return (unsigned)(tl >> (p.lg_tx + p.lg_ty)) * (unsigned)(p.Hin * p.Win * p.x_cs * 2);
    };
    int dtile = t;   // the tile whose chunks dma_chunk issues
    // one-tile forms: the plan held in registers (computed once); MULTI: at each issue
    unsigned voff[MULTI ? 1 : NPW];
    if constexpr (!MULTI) {
#pragma unroll
      for (int k = 0; k < NPW; ++k) voff[k] = piece_off(k, t);
    }
    auto poff = [&](int k) __attribute__((always_inline)) -> unsigned {
      if constexpr (MULTI) return piece_off(k, dtile);
      else return voff[k];
    };
    u32x2_t am[MT][NT];
    int nslot = 2;   // LDS slots of the chunk ring (epilogue_lds stages into a free one)
    if constexpr (NWAVES > 4 && !DB) {
      // the 8-wave tile's builtin DMA form (PG_HR_T3_ASM=0 and the sign-bit modes); the
      // asm form below (DB) loads the masks after the loop: held across it at 256 VGPRs they
      // spilled and that form measured 12 % slower
      auto dma_chunk = [&](int c0, int buf) {
        char* base = smem + buf * L::BUF;
  #pragma unroll
        for (int k = 0; k < NPW; ++k) {
          const int q = wid + NWAVES * k;   // wave-uniform
          if (q < L::HPIECES)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_t*)(base + q * 1024), 16, poff(k),
                                                     img_off(dtile) + (c0 >> 5) * x_cb2, 0, 0);
          else if (q < NP)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void_t*)(base + L::HREG + (q - L::HPIECES) * 1024),
                                                     16, poff(k), c0 * 2, 0, 0);
        }
      };
      // per-lane fragment bases: weight row r (+ swizzled slot g), halo column r + dx
      const int wlane = r * L::WROW + ((g ^ hr_swz(r)) << 4);
      int hl[3];
  #pragma unroll
      for (int dx = 0; dx < 3; ++dx) hl[dx] = (wid * MT * TW2 + r + dx) * 64 + ((g ^ hr_swz(r + dx)) << 4);
  #pragma unroll
      for (int mt = 0; mt < MT; ++mt)
  #pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      dma_chunk(0, 0);
      for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();   // chunk ch landed (vmcnt(0) + barrier); chunk ch-1's reads are done
        if (ch + 1 < nch) dma_chunk((ch + 1) * CK, (ch + 1) & 1);
        else load_mask(t, am);
        const char* cb = smem + (ch & 1) * L::BUF;
        const char* wb = cb + L::HREG + wlane;
        auto rd_w = [&](int ks, int nt) {
          return *reinterpret_cast<const bf16x8_t*>(wb + nt * 16 * L::WROW + ks * 64);
        };
        auto rd_x = [&](int ks, int mt) {   // tap ks = (dy, dx): halo row + dy, column + dx
          return *reinterpret_cast<const bf16x8_t*>(cb + hl[ks % 3] + ((ks / 3) + mt) * TW2 * 64);
        };
  #if PG_HR_DMA_PIPE
        // software-pipelined over the 9 taps: the next tap's weight fragments are read right
        // after their last use in this tap, the next pixel block's halo fragment before the
        // current block's MFMAs, so no MFMA group waits on a read issued just before it
        bf16x8_t wf[NT];
  #pragma unroll
        for (int nt = 0; nt < NT; ++nt) wf[nt] = rd_w(0, nt);
        bf16x8_t xf = rd_x(0, 0);
  #pragma unroll
        for (int ks = 0; ks < 9; ++ks) {
  #pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const bool lastm = mt + 1 == MT;
            const bf16x8_t xn = !lastm ? rd_x(ks, mt + 1) : rd_x(ks + 1 < 9 ? ks + 1 : ks, 0);
  #pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], xf, acc[mt][nt], 0, 0, 0);
              if (lastm && ks + 1 < 9) wf[nt] = rd_w(ks + 1, nt);
            }
            xf = xn;
          }
        }
  #else
  #pragma unroll 1
        for (int dy = 0; dy < 3; ++dy) {
  #pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const int ks = dy * 3 + dx;   // one tap per 32-deep k-step
            bf16x8_t wf[NT];
  #pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              wf[nt] = *reinterpret_cast<const bf16x8_t*>(wb + nt * 16 * L::WROW + ks * 64);
            const char* hb = cb + hl[dx] + dy * TW2 * 64;
            bf16x8_t xf = *reinterpret_cast<const bf16x8_t*>(hb);
  #pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              const bf16x8_t xn = mt + 1 < MT ? *reinterpret_cast<const bf16x8_t*>(hb + (mt + 1) * TW2 * 64) : xf;
  #if !PG_HR_NOSB
              __builtin_amdgcn_sched_barrier(0);
  #endif
  #pragma unroll
              for (int nt = 0; nt < NT; ++nt)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], xf, acc[mt][nt], 0, 0, 0);
  #if !PG_HR_NOSB
              __builtin_amdgcn_sched_barrier(0);
  #endif
              xf = xn;
            }
          }
        }
  #endif
      }
    } else {
      // The DMAs are issued from inline asm (hr_dma16), invisible to the compiler's wait
      // insertion: with the builtin it treated each as a pending write to the staging array
      // and waited vmcnt(0) for the NEXT chunk's DMA before the first fragment read of the
      // current one -- no overlap of staging and MFMAs at all (ISA-checked, with one array
      // or one per slot).  The chunk's arrival is waited for by hand (vmcnt + raw barrier).
      using S0 = std::integral_constant<int, 0>;
      using S1 = std::integral_constant<int, 1>;
      using S2 = std::integral_constant<int, 2>;
      auto slot = [&](auto S) -> char* { return smem + decltype(S)::value * L::BUF; };
      auto dma_chunk = [&](int c0, auto S) __attribute__((always_inline)) {
        char* base = slot(S);
  #pragma unroll
        for (int k = 0; k < NPW; ++k) {
          const int q = wid + NWAVES * k;   // wave-uniform
          if (q < L::HPIECES) {
            if (!(p.diag & 1))
              hr_dma16(xs, x_nrec, (lds_void_t*)(base + q * 1024), poff(k),
                       img_off(dtile) + (c0 >> 5) * x_cb2);
          } else if (q < NP) {
            if (!(p.diag & 2))
              hr_dma16(wsrc, w_nrec, (lds_void_t*)(base + L::HREG + (q - L::HPIECES) * 1024),
                       poff(k), c0 * 2);
          }
        }
      };
      // per-lane fragment bases: weight row r (+ swizzled slot g), halo column r + dx
      const int wlane = r * L::WROW + ((g ^ hr_swz(r)) << 4);
      int hl[3];
  #pragma unroll
      for (int dx = 0; dx < 3; ++dx) hl[dx] = (wid * MT * TW2 + r + dx) * 64 + ((g ^ hr_swz(r + dx)) << 4);
  #pragma unroll
      for (int mt = 0; mt < MT; ++mt)
  #pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      auto compute = [&](auto S) {
        const char* cb = slot(S);
        int hlm[3];   // MULTI: recomputed here, so nothing of it is live across an epilogue
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
          hlm[dx] = MULTI ? (wid * MT * TW2 + r + dx) * 64 + ((g ^ hr_swz(r + dx)) << 4) : hl[dx];
        const char* wb = cb + L::HREG + (MULTI ? r * L::WROW + ((g ^ hr_swz(r)) << 4) : wlane);
        auto rd_w = [&](int ks, int nt) {
          return *reinterpret_cast<const bf16x8_t*>(wb + nt * 16 * L::WROW + ks * 64);
        };
        auto rd_x = [&](int ks, int mt) {   // tap ks = (dy, dx): halo row + dy, column + dx
          return *reinterpret_cast<const bf16x8_t*>(cb + hlm[ks % 3] + ((ks / 3) + mt) * TW2 * 64);
        };
        // software-pipelined over the 9 taps: the next tap's weight fragments are read right
        // after their last use in this tap, the next pixel block's halo fragment before the
        // current block's MFMAs, so no MFMA group waits on a read issued just before it
        bf16x8_t wf[NT];
  #pragma unroll
        for (int nt = 0; nt < NT; ++nt) wf[nt] = rd_w(0, nt);
        bf16x8_t xf = rd_x(0, 0);
  #pragma unroll
        for (int ks = 0; ks < 9; ++ks) {
  #pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const bool lastm = mt + 1 == MT;
            const bf16x8_t xn = !lastm ? rd_x(ks, mt + 1) : rd_x(ks + 1 < 9 ? ks + 1 : ks, 0);
  #pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], xf, acc[mt][nt], 0, 0, 0);
              if (lastm && ks + 1 < 9) wf[nt] = rd_w(ks + 1, nt);
            }
            xf = xn;
          }
          // MULTI: keep the scheduler from hoisting later taps' fragment reads (their
          // registers made the persistent loop spill)
          if constexpr (MULTI) __builtin_amdgcn_sched_barrier(0);
        }
      };
      // DB with DMA: a three-slot ring with two chunks in flight across each barrier (every
      // wave issues exactly NPW DMA instructions per chunk, so a counted vmcnt(NPW) retires
      // chunk ch and leaves chunk ch+1 in flight; raw s_barrier, since __syncthreads' fence
      // would drain it).  Otherwise two slots, one chunk in flight.
      constexpr bool RING = DB && NWAVES <= 4;     // 8 waves with DB: two slots (LDS)
      constexpr bool MASK_LATE = NWAVES > 4;      // no mask registers live across the loop
      constexpr int NSLOT = RING ? 3 : 2;
      nslot = NSLOT;
      static_assert(!RING || NP % NWAVES == 0, "DMA ring: the same DMA count in every wave");
      auto dma_to = [&](int c, int sl) __attribute__((always_inline)) {   // chunk c into slot sl
        if (sl == 0) dma_chunk(c * CK, S0{});
        else if (sl == 1) dma_chunk(c * CK, S1{});
        else if constexpr (RING) dma_chunk(c * CK, S2{});
      };
      if constexpr (MULTI) {
        {
          // Persistent form: jobs j = (tile k, chunk c) in order; job j+1's DMAs (the next
          // chunk, or chunk 0 of the next tile) are issued right after the barrier that retires
          // job j's, so they are in flight during job j's MFMAs and, at a tile's last chunk,
          // during its epilogue, which stages through job j's slot (free after one barrier;
          // the next job lands in the other slot).  No per-workgroup dispatch, prologue or
          // first-chunk wait between tiles: the one-tile form paid them every 1-2 tiles per CU.
          // Waits: each wave waits for its own DMAs of job j+1 right after job j's MFMAs
          // (they had those MFMAs to land), so the barrier at the top of the next job only
          // needs LDS counts: the epilogue's global stores stay in flight across it.
          const int njobs = p.tpw * nch;
          int ch = 0, tn = t;   // chunk of job j; tile of job j+1's DMA
          dma_to(0, 0);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          for (int j = 0; j < njobs; ++j) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (j + 1 < njobs) {
              int c1 = ch + 1;
              if (c1 == nch) {
                c1 = 0;
                dtile = ++tn;
              }
              dma_to(c1, (j + 1) & 1);
            }
            if (ch == 0) {
#pragma unroll
              for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            }
            if (j & 1) compute(S1{});
            else compute(S0{});
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // job j+1's DMAs (and older stores)
            if (++ch == nch) {
              ch = 0;
              load_mask(t, am);
              load_bias();
              if (!(p.diag & 4)) {
                // every wave is done reading job j's slot before it becomes the staging area
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                char* st = smem + (j & 1) * L::BUF;
                if constexpr (NT == 4) epilogue_lds(t, am, st, st);
                else epilogue(t, am);
              }
              ++t;
            }
          }
          return;
        }
      }
      // the epilogue's mask operands first: ordinary loads issued inside the loop made the
      // compiler wait vmcnt(0) (the asm DMAs included) where their registers' paths merge
      if constexpr (!MASK_LATE) load_mask(t, am);
      dma_to(0, 0);
      if constexpr (RING) {
        if (nch > 1) dma_to(1, 1);
      }
      for (int ch = 0; ch < nch; ++ch) {
        if constexpr (RING) {
          if (ch + 1 < nch) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPW) : "memory");
          else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          // the slot refilled below was read in chunk ch-1: all of this wave's LDS reads are
          // back before it arrives, and every wave has arrived before any refill is issued
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
          asm volatile("" ::: "memory");
          if (ch + 2 < nch) dma_to(ch + 2, (ch + 2) % NSLOT);
        } else {
          // chunk ch landed (the only DMA in flight), chunk ch-1's reads are done
          asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
          asm volatile("" ::: "memory");
          if (ch + 1 < nch) dma_to(ch + 1, (ch + 1) & 1);
        }
        const int sl = ch % NSLOT;
        if (sl == 0) compute(S0{});
        else if (sl == 1) compute(S1{});
        else if constexpr (RING) compute(S2{});
      }
      if constexpr (MASK_LATE) load_mask(t, am);
    }
    if (p.diag & 4) return;   // diagnostic builds only (PG_HR_DIAG): no epilogue
    if constexpr (NT == 4) {
      if (!(p.diag & 8))
        return epilogue_lds(t, am, smem + (nch % nslot) * L::BUF, smem + ((nch - 1) % nslot) * L::BUF);
    }
    epilogue(t, am);
#endif
  } else if constexpr (DB) {
    static_assert(MODE == HR_PLAIN && NWAVES <= 4, "DB: plain 4-wave tiles");
    u32x4_t (&hb)[NH] = hbr[0];
    int (&hbits)[NHB] = hbitsr[0];
    unsigned& hok = hokr[0];
    const int t = tile_id;
    const int nch = p.cin_p / CK;
    fetch_halo(t, 0, hb, hbits, hok);
    fetch_w(0);
#pragma unroll
    for (int j = 0; j < NH + NW; ++j) store_one(j, smem, hb, hok);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    u32x2_t am[MT][NT];
    __syncthreads();
    // the staging writes of the next chunk go out from this k-step on, a few per k-step
    constexpr int KS0 = KS / 3;
    constexpr int NSV = NH + NW;
    constexpr int PER = (NSV + (KS - KS0) - 1) / (KS - KS0);
    for (int ch = 0; ch < nch; ++ch) {
      char* cur = smem + (ch & 1) * BUF_BYTES;
      char* nxt = smem + ((ch + 1) & 1) * BUF_BYTES;
      halo = cur;
      wl = cur + HALO_BYTES;
      const bool more = ch + 1 < nch;
      if (more) {
        fetch_halo(t, (ch + 1) * CK, hb, hbits, hok);
        fetch_w((ch + 1) * CK);
      } else {
        load_mask(t, am);
      }
      if (more) {
        mma_chunk_pipe_h([&](int ks) {
          if (ks >= KS0) {
#pragma unroll
            for (int q = 0; q < PER; ++q) {
              const int j = (ks - KS0) * PER + q;
              if (j < NSV) store_one(j, nxt, hb, hok);
            }
          }
        });
      } else {
        mma_chunk_pipe();
      }
      __syncthreads();
    }
    epilogue(t, am);
  } else {
    u32x4_t (&hb)[NH] = hbr[0];
    int (&hbits)[NHB] = hbitsr[0];
    unsigned& hok = hokr[0];
    const int t = tile_id;
    const int nch = p.cin_p / CK;
    fetch_halo(t, 0, hb, hbits, hok);
    fetch_w(0);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    u32x2_t am[MT][NT];
    for (int ch = 0; ch < nch; ++ch) {
      __syncthreads();
      store_halo(hb, hbits, hok);
      store_w();
      __syncthreads();
      if (ch + 1 < nch) {
        fetch_halo(t, (ch + 1) * CK, hb, hbits, hok);
        fetch_w((ch + 1) * CK);
      } else {
        load_mask(t, am);
      }
      mma_chunk();
    }
    epilogue(t, am);
  }
}

// Host side.  HR_ROWS is the one list of conv_hr_kernel variants: a row is an instantiation
// (nothing else is instantiated), its tile label and the rule by which conv_hr_select admits
// a launch to it.  conv_supported, the step plan and conv_hr_dispatch all ask conv_hr_select,
// so a new tile is a new row and nothing else.

// sign-bit mode of a set of flags (at most one bit feature per launch)
constexpr int hr_mode(int flags) {
  if (flags & PG_CONV_X_BITS) return (flags & PG_CONV_AUX_BITS) ? HR_XAB : HR_XB;
  if (flags & PG_CONV_Y2_BITS) return HR_YB;
  if (flags & PG_CONV_AUX_BITS) return HR_AB;
  return HR_PLAIN;
}

struct HrRow {
  int tile;   // the label DESIGN.md, profiles/ and the step plan use
  // conv_hr_kernel's template arguments
  int CK, TH, BN;
  bool PERSIST;
  int NW, MODE, PD;
  bool DB, DMA;
  int EF;      // >= 0: the launch's flags (| HR_EF_Y2 with y2), matched exactly; -1: runtime flags
  int takes;   // EF < 0: the flags a launch may carry (its sign-bit mode must be MODE)
  int hmin;    // smallest H
  bool (*geom)(const pg_conv_desc*);   // further geometry, or nullptr
};

constexpr int HR_BITS = PG_CONV_Y2_BITS | PG_CONV_AUX_BITS | PG_CONV_X_BITS;
constexpr int HR_EPI = PG_CONV_UPS_IN | PG_CONV_BIAS | PG_CONV_LRELU | PG_CONV_MASK | PG_CONV_POOL |
                       PG_CONV_ACCUM | PG_CONV_PIXNORM | HR_BITS;

// a runtime-flag row; the PixelNorm backward epilogue is in the [cout][pixel] tiles of <= 32
// channels.  Ring depth 1: the round-1 sweep measured it fastest for the runtime-flag persistent
// variants (deeper rings cost occupancy)
constexpr HrRow hr_rt(int tile, int CK, int TH, int BN, bool persist, int NW, int mode, bool DB = false,
                      bool DMA = false, bool (*geom)(const pg_conv_desc*) = nullptr) {
  return {tile, CK, TH, BN, persist, NW, mode, 1, DB, DMA, -1, HR_EPI | (BN <= 32 ? PG_CONV_PNBWD : 0),
          16, geom};
}
// a persistent row with its flags fixed at compile time (EF, see conv_hr_kernel), as the engine
// issues them at 128^2 .. 1024^2
constexpr HrRow hr_ef(int tile, int CK, int TH, int BN, int NW, int PD, int hmin, int ef) {
  return {tile, CK, TH, BN, true, NW, hr_mode(ef), PD, false, false, ef, 0, hmin, nullptr};
}

// tile 13: the wide convs whose 16 x 16 tiles would not fill the chip (32^2 at B = 4: 256
// workgroups of 128 pixels)
bool hr_geom_t13(const pg_conv_desc* d) {
  const size_t px = (size_t)d->B * d->H * d->W;
  // where the 16-row tiles (tile 6) already give 256 workgroups with the 64-channel blocks
  // counted, they take the launch: 32^2 512 -> 512 at B = 8 (the merged passes) 55.4 -> 45.7 us
  // per launch, 128 vs 256 KiB of staging per output pixel block (profiles/r5_lowres_tiles.txt)
  if (px / 256 * (((d->cout + 15) & ~15) / 64) >= 256) return false;
  return d->cout > 64 && px / 256 < 64 && px / 128 >= 32;
}
// tile 3: 32-row tiles when they still give a workgroup per CU
bool hr_geom_t3(const pg_conv_desc* d) {
  return (long)d->B * (d->W / 16) * (d->H / 32) * pg_cdiv((d->cout + 15) & ~15, 64) >= 256;
}

constexpr int HR_Y = HR_EF_Y2;
constexpr int HR_PN = PG_CONV_PIXNORM | PG_CONV_LRELU | PG_CONV_BIAS;
constexpr int HR_LB = PG_CONV_LRELU | PG_CONV_BIAS;
constexpr int HR_AM = PG_CONV_AUX_BITS | PG_CONV_MASK;
constexpr int HR_XM = PG_CONV_X_BITS | PG_CONV_MASK | PG_CONV_UPS_IN;

// In the order of preference: tiles 13 - 16, then by channel counts (the tile sweeps of rounds
// 1 - 4 chose these; tiles measured slower were removed); an EF row before its tile's
// runtime-flag rows, which take what no EF row matches.  Tiles 14 - 16 have EF rows only: what
// those do not match goes on to tiles 3 / 6 / 8.
constexpr HrRow HR_ROWS[] = {
    // tile 13 (8 x 16 pixels x 64 channels, LDS-DMA, two LDS slots): the wide convs at 32^2,
    // 2-7 % per launch against conv3x3_kernel.  Not in the asm-DMA form (+8-11 % per launch,
    // profiles/r6_t13_adma_ab.txt)
    {13, 32, 8, 64, false, 4, HR_PLAIN, 1, false, true, -1, HR_EPI & ~PG_CONV_PIXNORM, 16, hr_geom_t13},

#define T14(EF) hr_ef(14, 32, 16, 64, 8, 2, 256, EF)
    // tile 14: the 32 -> 64 sign-bit convs of the discriminator's 512^2 level (conv b forward
    // with Y2_BITS, R1 tangent with AUX_BITS).  One 32-channel chunk per tile: tile 3 ran each
    // workgroup's single DMA, MFMAs and epilogue back to back with one workgroup per CU (nothing
    // overlapped, ~85 us); the persistent form keeps the weight slab in LDS and the next tiles'
    // halos in flight (kbench 90.6 -> 74.0 us, profiles/r4_t14ef_ab.txt).  8 waves (two per SIMD
    // per workgroup, two workgroups per CU) against 4: 74.1 -> 56.4 us (forward), 64.8 -> 53.5
    // (tangent) at B = 4, 142.5 -> 106.1 / 128.3 -> 110.2 at B = 8 (profiles/r6_ef_waves_ab.txt).
    // (PG_CONV_POOL alone -- the generator's 512^2 pooled input gradient -- measured the same as
    // tile 3: 72.5 vs 72.6 us, profiles/r4_bits_kbench.txt: no row)
    T14(PG_CONV_Y2_BITS | PG_CONV_POOL | HR_LB | HR_Y), T14(HR_AM | PG_CONV_POOL),
#undef T14

#define T15(EF) hr_ef(15, 64, 8, 32, 4, 2, 256, EF)
    // tile 15: 64 -> 32 at >= 256^2 with the whole 64-channel K in one chunk: the G conv a
    // forward (up2 input, PixelNorm epilogue) and the D conv-b input gradient (X_BITS, also with
    // the AUX_BITS mask) of the 512^2 level.  Tile 8 (CK = 32, two chunks, one tile per workgroup,
    // runtime flags) ran them at 1.5-2.4 TB/s.  8-row tiles (two workgroups per CU: 67 KiB of LDS)
    // beat 16-row ones (one per CU): at B = 8 158 / 170 us (tile 8) -> 138 / 133 (TH 16) -> 104 /
    // 107 (TH 8); at B = 4 79 / 77 -> 56 / 55 (profiles/r5_t15_ab.txt)
    T15(HR_PN | PG_CONV_UPS_IN), T15(HR_PN | PG_CONV_UPS_IN | HR_Y), T15(HR_XM),
    T15(HR_XM | PG_CONV_AUX_BITS),
#undef T15

#define T16(EF) hr_ef(16, 64, 16, 64, 8, 2, 128, EF)
    // tile 16: 64 -> 64 at >= 128^2 (the 256^2 level: D conv a, G conv b; forward, input
    // gradient, tangent) with the whole 64-channel K in one chunk: the 64 x 9 x 64 weight slab
    // stays in LDS and each workgroup walks its tiles with the next halos in flight.  Tile 3
    // (32-channel chunks, one tile per workgroup, one workgroup per CU) re-read the slab per tile
    // and exposed each tile's first DMA and epilogue
    T16(0), T16(HR_LB), T16(PG_CONV_MASK), T16(HR_PN), T16(HR_PN | HR_Y),
#undef T16

    // The narrow EF tiles 0, 1, 4, 5 (16 / 32 channels at 512^2 / 1024^2).  8 waves against 4:
    // per launch -5 .. +7 % by shape in isolation, the whole step 9.983 -> 9.889 ms in 3 of 3
    // interleaved rounds (more waves per SIMD beside the side stream's weight gradients).
    // Ring depth 2: with depth 1 the loop entry (the first halo the youngest load) and the back
    // edge (the previous tile's stores younger than it) disagree, and the compiler's counting
    // falls back to vmcnt(0) at every halo store; at depth 2 the other slot's loads are younger
    // on both paths (checked in the ISA: no vmcnt(0) in the loop).  Depth 1 is still faster for
    // tiles 1 and 4 (kbench 116 -> 64 / 92 -> 87 us vs 79 / 95 at depth 2: their larger epilogue
    // covers the halo latency); depth 4 measured slower (profiles/r6_tile3_alternatives.txt).
    // A launch whose tile count is no multiple of the depth takes the runtime-flag row.
#define T0(EF) hr_ef(0, 16, 16, 16, 8, 2, 16, EF)
    // tile 0: 16 -> 16 (1024^2: D conv a fwd / dgrad / tangent, G conv b fwd / dgrad)
    T0(0), T0(HR_LB), T0(PG_CONV_MASK), T0(HR_PN), T0(HR_PN | HR_Y),
    // ... with the toRGB output in the epilogue (the generator's top conv b, alpha = 1)
    T0(HR_PN | PG_CONV_RGBO), T0(HR_PN | HR_Y | PG_CONV_RGBO),
    T0(PG_CONV_PNBWD | HR_Y),
    // conv a forward with the sign bits of its activation; its lrelu' consumers from those bits
    // (unpooled Y2_BITS / AUX_BITS exist only as these rows and tile 5's)
    T0(PG_CONV_Y2_BITS | HR_LB | HR_Y), T0(HR_AM),
    // ... with the fromRGB weight gradient in the epilogue (the final backward pass)
    T0(HR_AM | PG_CONV_RGBW),
    // ... with the fromRGB input gradient (the penalty's and the G half's passes)
    T0(HR_AM | PG_CONV_RGBD),
#undef T0
    hr_rt(0, 16, 16, 16, true, 4, HR_PLAIN),

#define T1(EF) hr_ef(1, 16, 16, 32, 8, 1, 16, EF)
    // tile 1: 16 -> 32 (1024^2: D conv b fwd (sign bits) / tangent, G conv a dgrad)
    T1(PG_CONV_Y2_BITS | PG_CONV_POOL | HR_LB | HR_Y), T1(HR_AM | PG_CONV_POOL),
    T1(PG_CONV_POOL), T1(PG_CONV_POOL | PG_CONV_ACCUM),
    // the G conv-a input gradient at 1024^2 with the 512^2 block's PixelNorm backward after the pool
    T1(PG_CONV_POOL | PG_CONV_PNBWD | HR_Y),
#undef T1
    hr_rt(1, 16, 16, 32, true, 4, HR_PLAIN), hr_rt(1, 16, 16, 32, true, 4, HR_YB),
    hr_rt(1, 16, 16, 32, true, 4, HR_AB),

    hr_rt(2, 16, 16, 64, false, 4, HR_PLAIN),

    // tile 3 (32 x 16 pixels x 64 channels): the wide convs at 64^2 - 256^2 and D conv b forward
    // / tangent there (Y2_BITS / AUX_BITS), LDS-DMA double-buffered staging in the inline-asm
    // form (overlapped staging, masks after the loop: A/B 298.0 -> 305.3 img/s, 5-7 % per launch).
    // 16 waves (2 x 4 blocks per wave, four waves per SIMD, 64 VGPRs) against 8 (4 x 4, two per
    // SIMD): 128^2 128 -> 128 24.0 -> 22.9 us at B = 4, 45.3 -> 42.6 at B = 8, 128 -> 256 pooled
    // 85.8 -> 84.5, step 10.249 -> 10.160 ms; the sign-bit modes -4 .. -17 % per launch, step
    // 10.270 -> 10.217 ms (profiles/r6_t3_waves_ab.txt).  (Instantiated in this order hipcc
    // emits the code that was measured; with the plain row first two of the three come out
    // some 60 bytes different.)
    hr_rt(3, 32, 32, 64, false, 16, HR_YB, true, true, hr_geom_t3),
    hr_rt(3, 32, 32, 64, false, 16, HR_AB, true, true, hr_geom_t3),
    hr_rt(3, 32, 32, 64, false, 16, HR_PLAIN, true, true, hr_geom_t3),

#define T4(EF) hr_ef(4, 32, 16, 16, 8, 1, 16, EF)
    // tile 4: 32 -> 16 (1024^2: D conv b dgrad with sign bits, G conv a fwd)
    T4(HR_XM), T4(HR_XM | PG_CONV_AUX_BITS), T4(HR_PN | PG_CONV_UPS_IN),
    T4(HR_PN | PG_CONV_UPS_IN | HR_Y),
#undef T4
    hr_rt(4, 32, 16, 16, true, 4, HR_PLAIN), hr_rt(4, 32, 16, 16, true, 4, HR_XB),
    hr_rt(4, 32, 16, 16, true, 4, HR_XAB),

#define T5(EF) hr_ef(5, 32, 16, 32, 8, 2, 16, EF)
    // tile 5: 32 -> 32 (512^2: D conv a, G conv b), the same launches as tile 0
    T5(0), T5(HR_LB), T5(PG_CONV_MASK), T5(HR_PN), T5(HR_PN | HR_Y),
    T5(HR_PN | PG_CONV_RGBO), T5(HR_PN | HR_Y | PG_CONV_RGBO),
    T5(PG_CONV_PNBWD | HR_Y),
    T5(PG_CONV_Y2_BITS | HR_LB | HR_Y), T5(HR_AM),
    T5(HR_AM | PG_CONV_RGBW),
    T5(HR_AM | PG_CONV_RGBD),
#undef T5
    hr_rt(5, 32, 16, 32, true, 4, HR_PLAIN), hr_rt(5, 32, 16, 32, true, 4, HR_XB),
    hr_rt(5, 32, 16, 32, true, 4, HR_XAB),

    // tile 6 (16 x 16 pixels x 64 channels): tile 3's asm-DMA form on 16-row tiles.  8 waves (two
    // per SIMD) against 4: 64^2 256 -> 256 29.0 -> 24.0 us, 512 -> 256 48.8 -> 41.9 at B = 4,
    // 32^2 512 -> 512 48.5 -> 41.1 at B = 8; step 9.675 -> 9.614 ms (profiles/r6_t6_waves_ab.txt)
    hr_rt(6, 32, 16, 64, false, 8, HR_PLAIN, true, true),

    // tiles 7, 8: more than one 32-channel chunk into 16 / 32 channels, one tile per workgroup
    hr_rt(7, 32, 16, 16, false, 4, HR_PLAIN),
    hr_rt(8, 32, 16, 32, false, 4, HR_PLAIN), hr_rt(8, 32, 16, 32, false, 4, HR_XB),
    hr_rt(8, 32, 16, 32, false, 4, HR_XAB),
};
constexpr int HR_NROWS = sizeof(HR_ROWS) / sizeof(HR_ROWS[0]);
static_assert(HR_ROWS[0].tile == 13, "conv_hr_ok reads tile 13's row");

// Whether row r runs this launch (ef = its flags, | HR_EF_Y2 with y2): the flags, then the
// geometry, then what launch_conv_hr asserts of the row
bool hr_admits(const HrRow& r, const pg_conv_desc* d, int ef) {
  if (r.EF >= 0 ? ef != r.EF || d->cout != r.BN
                : (d->flags & ~r.takes) || hr_mode(d->flags) != r.MODE)
    return false;
  const int cin_p = cinp_of(d->cin), cout_p = (d->cout + 15) & ~15;
  // every variant is [cout][pixel]: the narrowest of 16 / 32 / 64 channels that holds cout,
  // wider outputs in blocks of 64; PixelNorm (and its backward) needs a pixel's channels in one
  if (r.BN != (cout_p <= 16 ? 16 : cout_p <= 32 ? 32 : 64)) return false;
  if ((d->flags & (PG_CONV_PIXNORM | PG_CONV_PNBWD)) && cout_p > r.BN) return false;
  // persistent rows and the 16-channel chunk hold all of K; the others walk 32-channel chunks
  if ((r.PERSIST || r.CK == 16) ? cin_p != r.CK : cin_p % r.CK != 0) return false;
  const int tx = d->W / 16, ty = d->H / r.TH;
  if (d->H < r.hmin || d->H % r.TH || (tx & (tx - 1)) || (ty & (ty - 1))) return false;
  if (r.geom && !r.geom(d)) return false;
  // the EXACT grid: every workgroup walks a multiple of the ring depth
  if (r.EF >= 0 && (d->B * tx * ty) % r.PD) return false;
  if (r.EF >= 0 && (r.EF & PG_CONV_RGBD) && d->B > 16) return false;
  if (r.DMA) {   // one buffer resource over the whole input, see launch_conv_hr
    const int ups = d->flags & PG_CONV_UPS_IN ? 2 : 1;
    if ((size_t)d->B * (d->H / ups) * (d->W / ups) * std::max(d->x_cs, cin_p) * 2 > 0x7fff0000ull)
      return false;
  }
  return true;
}

// The shapes of this path (a conv it holds never falls back to conv3x3_kernel)
bool conv_hr_ok(const pg_conv_desc* d) {
  const int cin_p = cinp_of(d->cin);
  if (d->W < 16 || d->H < 16 || (d->W & 15) || d->B <= 0) return false;
  if (cin_p != 16 && cin_p % 32 != 0) return false;
  // wide outputs only where the 16 x 16 tiles x 64-channel blocks fill the chip, or tile 13 runs
  if (d->cout > 64 && (size_t)d->B * d->H * d->W / 256 * (((d->cout + 15) & ~15) / 64) < 256)
    return hr_admits(HR_ROWS[0], d, d->flags);
  return true;
}

// The variant that runs a conv, or nullptr: a pure function of the descriptor and of whether y2
// is given.  A stride the descriptor leaves 0 (a support query) counts as the smallest valid one.
const HrRow* conv_hr_select(const pg_conv_desc* d, bool y2) {
  if (!conv_hr_ok(d)) return nullptr;
  const int f = d->flags, cin_p = cinp_of(d->cin);
  // MASK with POOL only from sign bits (mask before the pool)
  if ((f & PG_CONV_MASK) && (f & PG_CONV_POOL) && !(f & PG_CONV_AUX_BITS)) return nullptr;
  if ((f & (PG_CONV_Y2_BITS | PG_CONV_AUX_BITS)) && (d->cout & 15)) return nullptr;
  // Y2_BITS without the pool: the sign bits of a 16 / 32-channel activation
  if ((f & PG_CONV_Y2_BITS) && !(f & PG_CONV_POOL) && (cin_p > 32 || (d->cout != 16 && d->cout != 32)))
    return nullptr;
  // X_BITS is staged at half resolution
  if ((f & PG_CONV_X_BITS) && !(f & PG_CONV_UPS_IN)) return nullptr;
  if (f & PG_CONV_PNBWD) {
    if (f & (HR_BITS | PG_CONV_BIAS | PG_CONV_MASK | PG_CONV_ACCUM | PG_CONV_PIXNORM)) return nullptr;
    // after a 2x2 pool: the 32-channel tiles (their swap epilogue; y and r at pooled resolution)
    if (((f & PG_CONV_POOL) && d->cout != 32) || d->cout % 4) return nullptr;
  } else if ((f & PG_CONV_PIXNORM) && !(f & HR_BITS) && (f & (PG_CONV_POOL | PG_CONV_MASK | PG_CONV_ACCUM))) {
    return nullptr;
  }
  {  // the kernel addresses inside one image with 32-bit element offsets
    const size_t cs = std::max({d->x_cs, cin_p, d->y_cs, d->cout, d->aux_cs, d->y2_cs, d->xb_cs});
    if ((size_t)d->H * d->W * (cs + 16) >= (1ull << 31)) return nullptr;
  }
  const int ef = f | (y2 ? HR_EF_Y2 : 0);
  for (const HrRow& r : HR_ROWS)
    if (hr_admits(r, d, ef)) return &r;
  return nullptr;
}

// Launches row I.  The PG_CHECK_ARGs up to the first HIP call assert what conv_hr_select
// promised of the row and check the operands it cannot see.
template <int I>
int launch_conv_hr(const pg_conv_desc* d, const ConvArgs& a, hipStream_t st) {
  constexpr HrRow R = HR_ROWS[I];
  constexpr int CK = R.CK, TH = R.TH, BN = R.BN, NWAVES = R.NW, MODE = R.MODE, PD = R.PD, EF = R.EF;
  constexpr bool PERSIST = R.PERSIST, DB = R.DB, DMA = R.DMA;
  constexpr auto kernel = conv_hr_kernel<CK, TH, BN, PERSIST, NWAVES, MODE, PD, DB, DMA, EF>;
  constexpr int KS = (9 * CK + 31) / 32;
  constexpr int PIXB = CK * 2 + (CK * 2 >= 64 ? 32 : 0);
  constexpr int HALO_BYTES = ((TH + 2) * 18 * PIXB + 15) & ~15;
  // EF: + the 16-B scratch slot of the branch-free halo store
  constexpr int LDS = DMA ? ((DB && NWAVES <= 4) ? 3 : 2) * HrDma<CK, TH, BN>::BUF
                          : (HALO_BYTES + BN * (KS * 64 + 32)) * (DB ? 2 : 1) +
                                ((EF >= 0 || MODE == HR_XB || MODE == HR_XAB) ? 16 : 0) +
                                ((MODE == HR_XB || MODE == HR_XAB) ? 4096 : 0) +   // X_BITS select masks
                                ((EF >= 0 && (EF & PG_CONV_RGBD)) ? NWAVES * 16 * 4 : 0);   // RGBD norms
  static_assert(LDS <= 160 * 1024, "conv_hr: LDS");
  ConvParams p = conv_params(d, a);
  const bool ups = (d->flags & PG_CONV_UPS_IN) != 0;
  PG_CHECK_ARG(!(d->flags & PG_CONV_RGBW) ||
                   (EF >= 0 && (EF & PG_CONV_RGBW) && a.rimg && a.rdw && a.scratch),
               "conv_hr: RGBW needs its EF variant and pg_conv3x3_rgbw's operands");
  PG_CHECK_ARG(!(d->flags & PG_CONV_RGBO) ||
                   (EF >= 0 && (EF & PG_CONV_RGBO) && a.rw && a.rb && a.gimg),
               "conv_hr: RGBO needs its EF variant and pg_conv3x3_rgbo's operands");
  PG_CHECK_ARG(!(d->flags & PG_CONV_RGBD) ||
                   (EF >= 0 && (EF & PG_CONV_RGBD) && a.rw && a.gimg && a.scratch && d->B <= 16),
               "conv_hr: RGBD needs its EF variant, pg_conv3x3_rgbd's operands and B <= 16");
  PG_CHECK_ARG((d->W / 16 & (d->W / 16 - 1)) == 0 && ((d->H / TH) & (d->H / TH - 1)) == 0,
               "conv_hr: tile counts must be powers of two");
  p.lg_tx = 0;
  while ((1 << p.lg_tx) < d->W / 16) ++p.lg_tx;
  p.lg_ty = 0;
  while ((1 << p.lg_ty) < d->H / TH) ++p.lg_ty;
  PG_CHECK_ARG(d->H % TH == 0 && p.cin_p % CK == 0, "conv_hr: bad geometry");
  PG_CHECK_ARG(!(d->flags & PG_CONV_X_BITS) || (a.xbits && d->xb_cs * 8 >= p.cin_p && ups),
               "conv_hr: X_BITS needs UPS_IN and xbits with >= cin/8 bytes per pixel");
  PG_CHECK_ARG(!PERSIST || (p.cin_p == CK && p.cout_p <= BN), "conv_hr: persist needs one chunk");
  PG_CHECK_ARG(EF < 0 || ((d->flags | (a.y2 ? HR_EF_Y2 : 0)) == EF && d->cout == BN),
               "conv_hr: EF variant %d does not match flags %d / cout %d", EF, d->flags, d->cout);
  {  // the kernel addresses inside one image with 32-bit element offsets
    const size_t hw = (size_t)d->H * d->W;
    const size_t cs = std::max({(size_t)d->x_cs, (size_t)d->y_cs, (size_t)d->aux_cs, (size_t)d->y2_cs,
                                (size_t)d->xb_cs});
    PG_CHECK_ARG(hw * (cs + 16) < (1ull << 31), "conv_hr: image too large for 32-bit offsets");
  }
  // LDS-DMA tiles: one buffer resource over the whole input; out-of-image halo slots use
  // offset 0x7fff0000 + the image offset, which must stay past the range and below 2^32
  // (the halo offset of an out-of-image slot is OOB = 0x7fff0000 plus at most the image
  // offset; it reads zeros only while the buffer's range ends at or below OOB)
  PG_CHECK_ARG(!DMA || (size_t)d->B * p.Hin * p.Win * d->x_cs * 2 <= 0x7fff0000ull,
               "conv_hr: input too large for the LDS-DMA tiles");
  const int ntiles = d->B * (d->W / 16) * (d->H / TH);
  // EXACT: every workgroup walks ntiles / grid tiles, a multiple of PD
  PG_CHECK_ARG(EF < 0 || ntiles % PD == 0, "conv_hr: EF needs ntiles %% PD == 0");
  // the launch's own size (not 160 KiB: the RGBW variants also hold det_commit's static word)
  PG_LDS_ATTR(kernel, LDS);
  dim3 grid;
  if (PERSIST) {
    // one resident wave of workgroups (occupancy of this variant x 256 CUs): a larger
    // grid runs as two serial rounds of persistent workgroups
    static int per_cu = 0;
    if (!per_cu) {
      (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kernel, NWAVES * 64, LDS);
      if (per_cu < 1) per_cu = 1;
      if (per_cu > 8) per_cu = 8;
    }
    int g = 256 * per_cu;
    if (EF >= 0) {   // the largest power of two <= g that divides ntiles / PD
      int gp = 1;
      while (gp * 2 <= g && (ntiles / PD) % (gp * 2) == 0) gp *= 2;
      g = gp;
    }
    grid = dim3(ntiles < g ? ntiles : g, 1, 1);
  } else {
    const int cb = pg_cdiv(p.cout_p, BN);
    grid = dim3(ntiles, cb, 1);
    p.tpw = 1;
  }
  PG_KLAUNCH(kernel, grid, dim3(NWAVES * 64), LDS, st, p);
  PG_LAUNCH_CHECK();
  return PG_OK;
}

template <size_t... I>
int launch_hr_row(size_t row, const pg_conv_desc* d, const ConvArgs& a, hipStream_t st,
                  std::index_sequence<I...>) {
  using Fn = int (*)(const pg_conv_desc*, const ConvArgs&, hipStream_t);
  static constexpr Fn fn[] = {launch_conv_hr<(int)I>...};
  return fn[row](d, a, st);
}

int conv_hr_dispatch(const pg_conv_desc* d, const ConvArgs& a, hipStream_t st) {
  const HrRow* r = conv_hr_select(d, a.y2 != nullptr);
  PG_CHECK_ARG(r, "conv3x3_fwd: no conv_hr variant takes flags 0x%x %s y2 for %d -> %d at %dx%d (B %d)",
               d->flags, a.y2 ? "with" : "without", d->cin, d->cout, d->H, d->W, d->B);
  return launch_hr_row(r - HR_ROWS, d, a, st, std::make_index_sequence<HR_NROWS>{});
}

