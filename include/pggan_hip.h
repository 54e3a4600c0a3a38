/* pggan_hip.h — C ABI of libpggan_hip.so, the gfx950 (MI355X) kernels of the
 * PGGAN G+D+R1 training step.
 *
 * The reference (yukyeongleee/pggan) has no native FFI on this path: its ops are
 * torch.nn.Conv2d / nn.Linear inside ConstrainedLayer (lib/layers.py:28-108)
 * and autograd supplies backward and the R1 double-backward
 * (lib/loss.py:125-135).  Each entry point below replaces one reference op (or a
 * fused group of them) and names the reference lines it stands in for.  A
 * maintainer binds these with ctypes.
 *
 * Conventions
 *  - every function returns 0 (PG_OK) or a negative error code; the message is
 *    available from pg_last_error();
 *  - all pointers are DEVICE pointers owned by the caller; the library never
 *    allocates; `stream` is a hipStream_t passed as void* (0 = null stream);
 *  - dtype: PG_F32 (exact-fp32 parity mode) or PG_BF16 (bf16 storage, fp32
 *    accumulation); weights/biases/gradients/optimizer state are always fp32;
 *  - activations are NHWC with an explicit channel stride `*_cs` (elements);
 *    images at the API boundary are NCHW fp32 like the reference;
 *  - kernels are stateless and re-entrant; outputs are written fully unless an
 *    ACCUM flag / "accumulates" note says the result is added;
 *  - results are deterministic: a call repeated on the same inputs and geometry gives
 *    bitwise the same outputs (no order-dependent float atomics).  Sums over workgroups
 *    go through a caller-provided `scratch` (PG_SCRATCH_BYTES, see below).
 */
#ifndef PGGAN_HIP_H
#define PGGAN_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_OK 0
#define PG_ERR_ARG (-1)
#define PG_ERR_HIP (-2)
#define PG_ERR_UNSUPPORTED (-3)

#define PG_F32 0
#define PG_BF16 1

const char* pg_last_error(void);
int pg_version(void);

/* Reduction scratch of the entry points that sum over workgroups (the 1x1 RGB weight and bias
 * gradients, the penalties' per-sample norms, pg_bias_grad, pg_r1_penalty, pg_gp_penalty): each
 * workgroup stores its partial sums there and the last one to finish adds them in workgroup
 * order (a fixed-order sum instead of float atomics), so results are bitwise reproducible.
 * Contract: PG_SCRATCH_BYTES of device memory, zero-filled ONCE by the caller when allocated;
 * one scratch per stream (calls on one stream may share it, calls that can run concurrently on
 * different streams may not); every call returns it to its zero state. */
#define PG_SCRATCH_BYTES (4u << 20)
size_t pg_scratch_bytes(void);

/* ---- equalized-LR 3x3 convolution (lib/layers.py:66-89, ConstrainedLayer.forward :58-63)
 * y = out_scale * post(conv3x3(pre(x), wpk) + bias)
 * wpk: packed weights from pg_conv3x3_pack with the He constant folded in.
 * The same kernel runs the forward pass, the input-gradient pass (dgrad, with
 * PG_PACK_DGRAD weights) and the R1 tangent pass (no bias, PG_CONV_MASK). */
#define PG_CONV_UPS_IN 1  /* x is H/2 x W/2; nearest x2 upsample on load (lib/utils.py:106-118) */
#define PG_CONV_BIAS 2    /* + bias[cout] (fp32, He constant folded) */
#define PG_CONV_LRELU 4   /* leaky relu(slope) on the conv result */
#define PG_CONV_MASK 8    /* multiply by lrelu'(aux) (aux at output resolution, channel stride aux_cs) */
#define PG_CONV_POOL 16   /* 2x2 pool of the activated result (avg: out_scale=0.25, sum: 1.0) */
#define PG_CONV_ACCUM 32  /* y += result */
/* PixelNorm fused into the epilogue (lib/layers.py:8-14 applied after the conv+LReLU of a
 * generator block, lib/blocks.py:128-129,138-139): y = v * rsqrt(mean_c v^2 + 1e-8) with v
 * the activated result rounded to the storage dtype; if y2 != NULL it receives the
 * per-pixel factor rsqrt(...) as fp32 [B*H*W] (for pg_pixnorm_lrelu_bwd_y).  Needs every
 * output channel in one tile: query pg_conv3x3_supported().  Not with POOL/MASK/ACCUM. */
#define PG_CONV_PIXNORM 64
/* Sign-bit masks (bf16, the H,W >= 16 kernel; query pg_conv3x3_supported).  A bit tensor
 * holds the leaky-relu sign (activation > 0) of every channel: [B][H][W][bytes], channel c
 * at byte c/8, bit c%8.  1 bit replaces a 16-bit activation wherever only its sign is read
 * again (the discriminator's conv+LReLU+pool outputs, lib/blocks.py:189-193). */
#define PG_CONV_Y2_BITS 128   /* y2 receives the sign bits of the activated output: with POOL
                                 of the pre-pool output; without POOL (16 / 32 output channels)
                                 of y itself, the lrelu' operand of the layer's later masks */
#define PG_CONV_AUX_BITS 256  /* MASK operand aux is a bit tensor (aux_cs = bytes per pixel);
                                 with POOL the mask applies before pooling; may be combined
                                 with X_BITS (input and output masks both from bits) */
#define PG_CONV_X_BITS 512    /* x is masked on load by lrelu'(xbits) at conv resolution
                                 (the xbits operand; xb_cs = bytes per pixel) */
#define PG_CONV_GZ_BITS 1024  /* wgrad: gz is at H/2 x W/2 and the effective gradient is
                                 up2(gz) * lrelu'(gzbits) (the gzbits operand) */
/* PixelNorm + LReLU backward fused into an input-gradient conv (bf16, H,W >= 16 kernel; query
 * pg_conv3x3_supported): with v the conv result = dL/dy of a PG_CONV_PIXNORM output y, the
 * launch writes dL/du = r * (v - y * mean_c(y * v)) * lrelu'(y), u the pre-norm activation
 * (pg_pixnorm_lrelu_bwd_y without the round trip of v through HBM).  aux = y (storage
 * dtype, aux_cs), y2 = r (fp32 [B*H*W], from the forward).  With POOL (32 output channels):
 * applied to the pooled result, y and r at the pooled resolution (the generator's input
 * gradient through an upsampling conv a, then the previous block's PixelNorm).  Not with
 * BIAS / MASK / ACCUM / PIXNORM / bit flags. */
#define PG_CONV_PNBWD 2048
/* fromRGB weight gradient in the epilogue of the input-gradient conv that produces the
 * fromRGB output's gradient gz (the discriminator's top conv a, lib/blocks.py:153-170 with
 * pggan/nets.py:255): the conv result gz is NOT stored; instead
 *   dw[n*3 + i] += s * sum_pix gz[n] * img[i],  db[n] += s * sum_pix gz[n]
 * (img fp32 NCHW [B][3][H][W], summed over workgroups in a fixed order through `scratch`).
 * Only through pg_conv3x3_rgbw; query pg_conv3x3_supported. */
#define PG_CONV_RGBW 4096
/* fromRGB input gradient in the same epilogue (the penalty's input-gradient pass and the G
 * half's, pggan/nets.py:255 backward): the conv result gz is not stored; instead
 *   gimg[b][i] = f * sum_n W[n][i] gz[n]   (fp32 NCHW, written),
 *   norms[b] += sum_pix sum_i gimg[b][i]^2 (if norms; the R1 / GP squared norms),
 *   dw[n*3 + i] += s * sum_pix gz[n] gimg[i] (if dw; the R1 tangent's fromRGB weight term,
 *                                             s = f / B: gbar = gimg / B)
 * summed over workgroups in a fixed order through `scratch`.  Only through pg_conv3x3_rgbd. */
#define PG_CONV_RGBD 8192
/* toRGB output in the epilogue of the generator's top conv b forward (with PG_CONV_PIXNORM:
 * lib/blocks.py:131-139 then toRGBBlock, lib/blocks.py:153-170, pggan/nets.py:140-156 at
 * alpha = 1): y (and y2 = the PixelNorm factor) are written as by pg_conv3x3_fwd, and
 *   img[b][k] = c * (sum_n w_rgb[k][n] y[n] + b_rgb[k])   (fp32 NCHW, y as stored in bf16)
 * so the top activation is not read back by a separate toRGB pass.  Only through
 * pg_conv3x3_rgbo. */
#define PG_CONV_RGBO 16384

typedef struct {
  int B, H, W;     /* conv output spatial size (after the optional input upsample) */
  int cin, cout;   /* channels as packed (cin: multiple of 8, <=16 or multiple of 32) */
  int x_cs, y_cs, aux_cs, y2_cs; /* channel strides (elements) of x, y, aux, y2 */
  int flags;
  float slope;     /* leaky relu slope */
  float out_scale;
  int xb_cs;       /* bytes per pixel of the X_BITS / GZ_BITS bit tensor */
} pg_conv_desc;

#define PG_PACK_FWD 0    /* wpk[cout_p][9][cin_p]   = scale * W[o][c][tap]          */
#define PG_PACK_DGRAD 1  /* wpk[cin_p16][9][cout_p] = scale * W[o][c][8 - tap]      */
size_t pg_conv3x3_packed_elems(int mode, int cout, int cin);
int pg_conv3x3_pack(int dtype, int mode, int cout, int cin, const float* w_oihw, float scale,
                    void* wpk, void* stream);
/* All conv weights of a net in one launch: for each item, fwd and dgrad packs (as
 * pg_conv3x3_pack) and bias_scaled[o] = scale * bias[o] (bias may be NULL).  `items` is a
 * DEVICE array of n pg_pack_item (built once; the pointers are stable across steps);
 * max_tiles = max over items of ceil(max(cout16, cinp(cout))/32) * ceil(max(cinp(cin), cin16)/32). */
typedef struct {
  const float* w;       /* [cout][cin][3][3] fp32 */
  const float* bias;    /* [cout] or NULL */
  void* fwd;            /* PG_PACK_FWD layout, dtype */
  void* dgrad;          /* PG_PACK_DGRAD layout, dtype */
  float* bias_scaled;   /* [cout] */
  float scale;
  int cout, cin;
  int pad_;
} pg_pack_item;
int pg_conv3x3_pack_batch(int dtype, int n, const pg_pack_item* items, int max_tiles,
                          void* stream);
/* ws: optional fp32 workspace (>= pg_conv3x3_workspace_size bytes) that enables split-K
 * over input-channel chunks for small-spatial convs (deterministic: partial slabs + a
 * reduction/epilogue kernel); NULL or too small -> single pass. */
size_t pg_conv3x3_workspace_size(const pg_conv_desc* d);
/* xbits: the input-mask bit tensor of PG_CONV_X_BITS (bf16), NULL without that flag.  The
 * RGBW / RGBD / RGBO flags are refused here: they have their own entry points below. */
int pg_conv3x3_fwd(int dtype, const pg_conv_desc* d, const void* x, const void* xbits,
                   const void* wpk, const float* bias, const void* aux, void* y, void* y2,
                   void* ws, size_t ws_bytes, void* stream);
/* The input-gradient conv of PG_CONV_RGBW (d->flags includes it, y is not written): x, wpk,
 * aux as pg_conv3x3_fwd; img the fromRGB layer's input image, s its He constant, dw [C*3] /
 * db [C] the fromRGB weight / bias gradients (accumulated), scratch a PG_SCRATCH_BYTES
 * reduction scratch of the stream.  Replaces pg_conv3x3_fwd + pg_from_rgb_bwd(dw, db) of the
 * final backward pass (lib/model.py:95-97 through autograd in the reference). */
int pg_conv3x3_rgbw(int dtype, const pg_conv_desc* d, const void* x, const void* wpk,
                    const void* aux, const float* img, float s, float* dw, float* db,
                    void* scratch, void* stream);
/* The input-gradient conv of PG_CONV_RGBD (d->flags includes it, y not written, B <= 16): x,
 * wpk, aux as pg_conv3x3_fwd; w_rgb [C][3] the fromRGB weights, f their He constant; gimg the
 * image gradient written; norms [B] accumulated or NULL; dw [C*3] accumulated or NULL with
 * scale s; scratch a PG_SCRATCH_BYTES reduction scratch of the stream.  Replaces
 * pg_conv3x3_fwd + pg_from_rgb_bwd(gimg, norms) (+ the tangent's pg_from_rgb_bwd(dw)). */
int pg_conv3x3_rgbd(int dtype, const pg_conv_desc* d, const void* x, const void* wpk,
                    const void* aux, const float* w_rgb, float f, float* gimg, float* norms,
                    float* dw, float s, void* scratch, void* stream);
/* The generator's top conv b forward with PG_CONV_RGBO (d->flags = PIXNORM | LRELU | BIAS |
 * RGBO): x, wpk, bias, y, y2 as pg_conv3x3_fwd; w_rgb [3][C] / b_rgb [3] the toRGB layer's
 * weights and bias, c its He constant, img [B][3][H][W] fp32 written.  Replaces pg_conv3x3_fwd
 * + pg_rgb_out at alpha = 1 (pggan/nets.py:140-156). */
int pg_conv3x3_rgbo(int dtype, const pg_conv_desc* d, const void* x, const void* wpk,
                    const float* bias, void* y, void* y2, const float* w_rgb, const float* b_rgb,
                    float c, float* img, void* stream);
/* 1 if pg_conv3x3_fwd supports d->flags for this shape/dtype (the fused epilogues depend
 * on the tile the dispatcher picks), 0 otherwise.  ws_bytes as passed to the launch. */
int pg_conv3x3_supported(int dtype, const pg_conv_desc* d, size_t ws_bytes);
/* weight gradient, accumulates: dw[o][c][ky][kx] += scale * sum_p gz[p][o] * x[p+tap][c]
 * and, if db != NULL, the bias gradient db[o] += scale * sum_p gz[p][o] (fused: gz is read
 * once).  desc: B,H,W, cin, cout, x_cs, y_cs = gz channel stride, flags may hold
 * PG_CONV_UPS_IN.  bf16: cout and both channel strides must be multiples of 8.  A stride left
 * 0 (x_cs, y_cs, xb_cs) counts as the packed one: cin as packed, cout rounded up to 8, cout / 8. */
/* ws: optional fp32 workspace (>= pg_conv3x3_wgrad_workspace_size bytes, asked with the
 * launch's flags).  When the pixel range is split over workgroups the partial sums go to
 * per-split slabs of ws and a second kernel adds them into dw/db in slab order; NULL or too
 * small -> one split, slower and as deterministic. */
/* gzbits: NULL, or with PG_CONV_GZ_BITS (bf16 only) the sign bits at full resolution (xb_cs
 * bytes per pixel) of a gz given at half resolution (channel stride y_cs). */
size_t pg_conv3x3_wgrad_workspace_size(int dtype, const pg_conv_desc* d);
/* 0 if pg_conv3x3_wgrad refuses this descriptor (shape, strides, flags: not every tile has a
 * PG_CONV_GZ_BITS kernel), otherwise positive.  Which positive value (bf16: the 1-based row of
 * the kernel table) is for diagnostics and tests, not a stable part of the ABI. */
int pg_conv3x3_wgrad_supported(int dtype, const pg_conv_desc* d);
int pg_conv3x3_wgrad(int dtype, const pg_conv_desc* d, const void* x, const void* gz,
                     const void* gzbits, float scale, float* dw, float* db, void* ws,
                     size_t ws_bytes, void* stream);
/* bias gradient, accumulates: db[c] += scale * sum_p g[p][c] */
int pg_bias_grad(int dtype, int npix, int C, int cs, const void* g, float scale, float* db,
                 void* scratch, void* stream);

/* ---- PixelwiseVectorNorm (lib/layers.py:8-14) over the channel axis of NHWC */
int pg_pixnorm_fwd(int dtype, int npix, int C, int cs, const void* x, void* y, void* stream);
/* gz = PN^T(gy) * lrelu'(u), u = the PN input (a leaky-relu output) (lib/blocks.py:128-139) */
int pg_pixnorm_lrelu_bwd(int dtype, int npix, int C, int cs, const void* u, const void* gy,
                         float slope, int apply_mask, void* gz, void* stream);

/* ---- elementwise helpers (NHWC, channel stride cs) */
/* the same backward from the fused conv's outputs (PG_CONV_PIXNORM): y = normalised
 * activation, r = per-pixel factor (fp32 [npix]); u = y / r is never stored */
int pg_pixnorm_lrelu_bwd_y(int dtype, int npix, int C, int cs, const void* y, const float* r,
                           const void* gy, float slope, void* gz, void* stream);
/* out[p] = scale * g[ups ? p/2 : p] * (y ? lrelu'(y[p]) : 1)   (avg-pool backward, lib/blocks.py:193)
 * bits: NULL, or (bf16, C % 8 == 0) the lrelu' operand as sign bits, uint8 [B][H][W][C / 8]
 * (PG_CONV_Y2_BITS of the pooled conv that produced it) instead of the activation y */
int pg_unpool_mask(int dtype, int B, int H, int W, int C, int g_cs, const void* g, int y_cs,
                   const void* y, const void* bits, float scale, float slope, int ups, int out_cs,
                   void* out, void* stream);
/* 2x2 average pool (lib/utils.py:120-124), input B x H x W */
int pg_avgpool2(int dtype, int B, int H, int W, int C, int x_cs, const void* x, int y_cs, void* y,
                void* stream);
/* out = a*x + b*y over n elements (fade-in blends, pggan/nets.py:155-156, 263-265) */
int pg_blend(int dtype, size_t n, float a, const void* x, float b, const void* y, void* out,
             void* stream);

/* ---- RGB layers (toRGBBlock lib/blocks.py:153-170, fromRGBBlock :271-292) */
/* G output image (NCHW fp32): img = alpha*toRGB_s(x) + (1-alpha)*up2(toRGB_{s-1}(xp));
 * xp == NULL -> img = toRGB_s(x) (stage 0).  w: [3][C] fp32 raw, b: [3], c: He constant. */
int pg_rgb_out(int dtype, int B, int R, int C, int x_cs, const void* x, const float* w,
               const float* b, float c, int Cp, int xp_cs, const void* xp, const float* wp,
               const float* bp, float cp, float alpha, float* img, void* stream);
/* backward of pg_rgb_out: writes gx (NHWC, T) and gxp; accumulates dw/db/dwp/dbp */
int pg_rgb_out_bwd(int dtype, int B, int R, int C, int x_cs, const void* x, const float* w,
                   float c, int Cp, int xp_cs, const void* xp, const float* wp, float cp,
                   float alpha, const float* gimg, void* gx, void* gxp, float* dw, float* db,
                   float* dwp, float* dbp, void* scratch, void* stream);
/* the toRGB input gradient fused with the PixelNorm + LReLU backward of its input y (the level's
 * PG_CONV_PIXNORM output, r its per-pixel factor fp32 [B*R*R]): gz = r (v - y mean_c(y v))
 * lrelu'(y), v = c W^T gimg (pg_rgb_out_bwd's gx then pg_pixnorm_lrelu_bwd_y, without v's round
 * trip through HBM); C 16 or 32, alpha = 1 (no fade-in branch).  dw != NULL: also the toRGB
 * weight / bias gradients of the same pass (dw[i][k] += c sum gimg[i] y[k], db[i] += c sum
 * gimg[i] if db; scratch: the stream's PG_SCRATCH_BYTES reduction scratch, else may be NULL): y
 * and gimg are streamed once for both (lib/blocks.py toRGB, pggan/nets.py:140-156) */
int pg_rgb_out_bwd_pn(int dtype, int B, int R, int C, int y_cs, const void* y, const float* r,
                      const float* w, float c, const float* gimg, float slope, int gz_cs, void* gz,
                      float* dw, float* db, void* scratch, void* stream);
/* An image operand of the fromRGB layers, a tensor (x0 alone) or a per-sample mix:
 * img[b] = a[b] * x0[b] + c[b] * x1[b] (NCHW fp32; a, c: DEVICE arrays of B floats; x1 and c
 * may be NULL; a == NULL means img = x0).  The gradient-penalty passes read the interpolated
 * image eps x_real + (1 - eps) x_fake (pggan/loss.py:75) and the penalty-weighted input
 * gradient this way, so neither is materialised. */
typedef struct {
  const float* x0;
  const float* x1;
  const float* a;
  const float* c;
} pg_img_src;
/* fromRGB: y = lrelu(c*(W . img_in + b)), img_in = down ? avgpool2(img) : img; R = output
 * resolution.  b == NULL -> no bias; mask_y != NULL -> tangent mode: y = c*(W . img_in) *
 * lrelu'(mask_y) (no activation).
 * The lrelu sign bits as an operand instead of a bf16 activation (bf16, C % 8 == 0, C <= 64,
 * mask_y NULL): ybits != NULL (forward) also writes the bits of the result y > 0, uint8
 * [B][R][R][C / 8] (channel o at byte o / 8, bit o % 8); mask_bits != NULL (the R1 tangent) masks
 * with those bits where mask_y would be read (16x fewer bytes: 134 MB -> 8.4 MB per launch at
 * 1024^2, 16 channels, B = 4).  At most one of the two. */
int pg_from_rgb(int dtype, int B, int R, int C, const pg_img_src* img, int down, const float* w,
                const float* b, float c, float slope, const void* mask_y, const void* mask_bits,
                int y_cs, void* y, void* ybits, void* stream);
/* backward: gimg[b][i][p] += c * sum_o gz[p(/2)][o] W[o][i] * (down ? 0.25 : 1) (if gimg;
 * gimg_overwrite = 1 writes gimg instead of accumulating into it); norms != NULL: norms[b] +=
 * sum over sample b of the final gimg^2 (the penalties' per-sample squared norms, fused into
 * the pass that writes the input gradient); dw[o][i] += c sum gz*img_in, db[o] += c sum gz (if
 * dw / db; img may be NULL without them) */
int pg_from_rgb_bwd(int dtype, int B, int R, int C, const pg_img_src* img, int down,
                    const float* w, float c, int gz_cs, const void* gz, float* gimg,
                    int gimg_overwrite, float* norms, float* dw, float* db, void* scratch,
                    void* stream);
/* The penalty and the tangent-pass scale from the per-sample squared norms n_b of g = dD/dx:
 * mode 0 (R1, lib/loss.py:125-135): loss_out[0] += 0.5 * sum_b n_b / B, scale_b = 1 / B;
 * mode 1 (WGAN-GP, pggan/loss.py:81-87): loss_out[0] += w * sum_b (sqrt(n_b) - 1)^2,
 * scale_b = 2 w (sqrt(n_b) - 1) / sqrt(n_b) (0 where n_b = 0).  scale: DEVICE [B].  The
 * norms are reset to 0 (ready for the next accumulating pass: no memset per step). */
int pg_penalty_scale(int mode, int B, float* norms, float w, float* loss_out, float* scale,
                     void* stream);

/* real-image fade (pggan/model.py:217-221): out = (1-a)*up2(avgpool2(x)) + a*x, NCHW fp32 */
int pg_img_fade(int B, int C, int R, const float* x, float alpha, float* out, void* stream);

/* ---- equalized linear (lib/layers.py:92-108)
 * x: [B][K] (or NHWC [B][16][C] when PG_LIN_IN_CHW: k = c*16 + hw, the reference's NCHW flatten)
 * y: [B][N] (or NHWC [B][16][N/16] when PG_LIN_OUT_CHW: n = c*16 + hw, pggan/nets.py:130) */
#define PG_LIN_BIAS 1
#define PG_LIN_LRELU 2
#define PG_LIN_MASK 4     /* multiply by lrelu'(aux), aux laid out like y */
#define PG_LIN_IN_CHW 8
#define PG_LIN_OUT_CHW 16
#define PG_LIN_F32_IN 32  /* x is fp32 regardless of dtype */
#define PG_LIN_F32_OUT 64 /* y is fp32 regardless of dtype */
typedef struct {
  int B, K, N;
  int in_cs, out_cs;  /* channel strides for the CHW-mapped sides */
  int flags;
  float scale, slope;
} pg_linear_desc;
/* ws: optional fp32 workspace (>= pg_linear_workspace_size bytes; pass 0 = fwd, 1 = dgrad) for
 * the bf16 split-reduction forms of the two passes below (deterministic: fp32 partials of weight
 * slices in ws, then a small epilogue kernel).  NULL or too small (or the fp32 mode): one pass. */
size_t pg_linear_workspace_size(int dtype, const pg_linear_desc* d, int pass);
int pg_linear_fwd(int dtype, const pg_linear_desc* d, const void* x, const float* w,
                  const float* b, const void* aux, void* y, void* ws, size_t ws_bytes,
                  void* stream);
/* gx[b][k] = scale * sum_n gy[b][n] W[n][k]  (* lrelu'(aux[b][k]) if PG_LIN_MASK); flags
 * IN_CHW/F32_IN describe gx, OUT_CHW/F32_OUT describe gy */
int pg_linear_dgrad(int dtype, const pg_linear_desc* d, const void* gy, const float* w,
                    const void* aux, void* gx, void* ws, size_t ws_bytes, void* stream);
/* accumulates dw[n][k] += scale sum_b gy[b][n] x[b][k]; db[n] += scale sum_b gy[b][n] */
int pg_linear_wgrad(int dtype, const pg_linear_desc* d, const void* x, const void* gy, float* dw,
                    float* db, void* stream);

/* ---- minibatch stddev (lib/blocks.py:204-233), x: [B][HW][C] (cs x_cs) -> y: [B][HW][y_cs]
 * (channel C = group stddev, channels C+1..y_cs-1 = 0) */
int pg_mbstd_fwd(int dtype, int B, int HW, int C, int x_cs, const void* x, int y_cs, void* y,
                 void* stream);
/* gx = gy[:, :C] + d mbstd/dx ^T gy[:, C] */
int pg_mbstd_bwd(int dtype, int B, int HW, int C, int x_cs, const void* x, int y_cs,
                 const void* gy, void* gx, void* stream);
/* R1 second-order pieces at mbstd: tangent output tout = [a, sdot, 0..] and the injection
 * inj = d/dx <a, J^T gy> (added into the second backward), a = tangent at the input */
int pg_mbstd_r1(int dtype, int B, int HW, int C, int x_cs, const void* x, const void* a,
                int y_cs, const void* gy, void* tout, void* inj, void* stream);

/* ---- losses (lib/loss.py:119-135, pggan/loss.py:5-27); all fp32, device-resident scalars
 * logits [B]: loss = mean softplus(target ? -l : l); u = dloss/dl (scaled by w);
 * h = d u / d l (for the R1 double-backward).  loss_out[0] += w * loss. */
int pg_bce_loss(int B, const float* logits, int target, float w, float* loss_out, float* u,
                float* h, void* stream);
/* WGAN-GP mode drift term (pggan/loss.py:94-100 get_drift_loss): loss_out[0] += w * sum_b l_b^2
 * and u_b += 2 w l_b (u: the logit gradient of the real-image BCE, accumulated) */
int pg_drift_loss(int B, const float* logits, float w, float* loss_out, float* u, void* stream);
/* R1 = 0.5 * mean_b sum g^2 accumulated into r1_out[0]; gbar = g / B  (g: [n] fp32, B samples) */
int pg_r1_penalty(int B, size_t n, const float* g, float* r1_out, float* gbar, void* scratch,
                  void* stream);
/* WGAN-GP optional mode (pggan/loss.py:54-92):
 * gp = w * sum_b (||g_b|| - 1)^2 -> gp_out[0] (accumulate); gbar_b = w*2*(||g_b||-1)/||g_b|| g_b;
 * norms[B] workspace */
int pg_gp_penalty(int B, size_t per, const float* g, float w, float* gp_out, float* norms,
                  float* gbar, void* scratch, void* stream);

/* out = x + y*z (fp32; the R1 logit injection u + h*t, pggan/loss.py:16-27) */
int pg_mul_add(size_t n, const float* x, const float* y, const float* z, float* out, void* stream);

/* ---- Adam (torch.optim.Adam, lib/model.py:95-97; single-tensor update order) over one flat
 * fp32 range (the live parameters of a net are kept contiguous; dead ones are not passed) */
int pg_adam(size_t n, float* p, const float* g, float* m, float* v, float lr, float beta1,
            float beta2, float eps, int step, void* stream);

/* Adam with the step count in DEVICE memory, for a step captured once and replayed as a
 * hipGraph: bumps *step, then updates with the bias corrections of the new count taken from
 * `table` (DEVICE, tlen pairs {lr / (1 - beta1^t), sqrt(1 - beta2^t)} for t = 1..tlen, built
 * by pg_adam_table on the host with pg_adam's double arithmetic; counts past tlen use the last
 * pair, which pg_adam_table_len makes exact) -- the same update as pg_adam at that step. */
int pg_adam_table_len(float lr, float beta1, float beta2);
int pg_adam_table(float lr, float beta1, float beta2, int tlen, float* host_table);
int pg_adam_dev(size_t n, float* p, const float* g, float* m, float* v, float beta1, float beta2,
                float eps, const float* table, int tlen, int* step, void* stream);

/* pg_adam / pg_adam_dev with the generator's weight average updated in the same launch:
 * p, m, v exactly as the entry above writes them, then, from the new p still in its register,
 * ema[i] += one_minus_decay * (p[i] - ema[i]) in fp32 (`ema` DEVICE, n floats, laid out as p;
 * one_minus_decay = (float)(1.0 - (double)decay), in (0, 1]).  PG_ERR_ARG on a null pointer or
 * a coefficient outside that range. */
int pg_adam_ema(size_t n, float* p, const float* g, float* m, float* v, float* ema,
                float one_minus_decay, float lr, float beta1, float beta2, float eps, int step,
                void* stream);
int pg_adam_dev_ema(size_t n, float* p, const float* g, float* m, float* v, float* ema,
                    float one_minus_decay, float beta1, float beta2, float eps, const float* table,
                    int tlen, int* step, void* stream);

/* ---- N(0,1) latents (counter-based, deterministic in (seed, offset)) */
int pg_randn(size_t n, uint64_t seed, uint64_t offset, float* out, void* stream);
/* the same draw with the offset in DEVICE memory; *offset then advances by n (graph replay) */
int pg_randn_dev(size_t n, uint64_t seed, uint64_t* offset, float* out, void* stream);
/* dtype conversion helpers */
int pg_cast(int dtype_in, int dtype_out, size_t n, const void* x, void* y, void* stream);

/* ---- training-image augmentation (SURVEY §8(f) GPU input pipeline): the transform chain
 * of lib/dataset.py:106-117 after Resize -- RandomHorizontalFlip(0.5), ColorJitter(0.2, 0.2,
 * 0.2, 0.01) in torchvision's random op order, ToTensor, Normalize(0.5, 0.5) -- on a batch of
 * decoded, resized images: src uint8 [B][H][W][3] (4-byte aligned), dst fp32 [B][3][H][W]
 * (16-byte aligned), params fp32 [B][12] = {flip (0/1), brightness, contrast, saturation,
 * hue factor, fn_idx[0..3] (0 brightness, 1 contrast, 2 saturation, 3 hue), 1 - contrast,
 * 1 - saturation, 0}.
 * Jitter arithmetic: the reference's PIL path (torchvision functional_pil: ImageEnhance
 * Brightness / Contrast / Color blends and the uint8 shift of PIL's HSV hue band) in Pillow's
 * libImaging arithmetic, uint8 after every op: byte-identical to the reference transform.
 * W % 4 == 0.  The caller provides pg_augment_workspace_bytes(B, H, W) of device workspace
 * (16-byte aligned). */
size_t pg_augment_workspace_bytes(int B, int H, int W);
int pg_augment_u8(int B, int H, int W, const void* src, const float* params, float* ws,
                  size_t ws_bytes, float* dst, void* stream);

/* ---- training-image resize (lib/dataset.py:103, Resize((S, S)) on the PIL image = Pillow's
 * Image.resize(.., BILINEAR)): n uint8 RGB images of one source shape [Hin][Win][3] ->
 * [S][S][3] in Pillow's 8-bit arithmetic (libImaging/Resample.c), byte-identical to PIL: a
 * horizontal pass into a uint8 image [Hin][S][3], then a vertical pass, each
 *   out = clip8((2^21 + sum_{x < count} pixel[xmin + x] * k[x]) >> 22)   (int32 sums)
 * with per output position the window (xmin, count) and the 22-bit fixed-point weights k from
 * the caller's tables: kx int32 [S][ksx], bx int32 [S][2] = (xmin, count) for Win -> S, ky / by
 * / ksy for Hin -> S (DEVICE; built on the host in float64 as Pillow builds them, see
 * pggan_amd.data.resize_coeffs; xmin + count <= the input size and count <= ks, the caller's
 * duty).  As in Pillow a pass whose input size equals S is skipped (its tables are not read and
 * may be NULL); with both skipped the call is a copy.
 * Image i is read at src_base + src_off[i] and written at dst_base + dst_off[i] (src_off /
 * dst_off: DEVICE int64 [n], byte offsets: rows of a ragged source cache, scattered rows of a
 * batch).  Source rows are 3 Win bytes, unpadded; every source image starts 16-byte aligned;
 * destinations need no alignment and must not overlap.  Every source byte is read from memory
 * once.  ws: pg_resize_workspace_bytes(n, Hin, Win, S) of device workspace, 16-byte aligned (0
 * bytes when a pass is skipped; ws may then be NULL).  n <= 65535; PG_ERR_UNSUPPORTED when 8
 * source rows (24 Win bytes) do not fit the 64 KiB staging of the horizontal pass. */
size_t pg_resize_workspace_bytes(int n, int Hin, int Win, int S);
int pg_resize_bilinear_u8(int n, int Hin, int Win, int S, const void* src_base,
                          const int64_t* src_off, const int* kx, const int* bx, int ksx,
                          const int* ky, const int* by, int ksy, void* dst_base,
                          const int64_t* dst_off, void* ws, size_t ws_bytes, void* stream);

/* ---- sliced Wasserstein distance on Laplacian-pyramid patches (the PGGAN paper's validation
 * metric; DESIGN.md "Validation: sliced Wasserstein distance").  All fp32; images NCHW
 * [B][3][S][S], S a power of two.  `quantize` != 0 reads the image as 8-bit:
 * q(x) = rint(clip(127.5 x + 127.5, 0, 255)), ties to even (for pyramid level 0).
 * Gaussian pyramid step: filter with k (x) k, k = [1 4 6 4 1] / 16, mirror boundary without
 * repeating the edge sample, keep every second sample from 0: x [B][3][H][W] -> y
 * [B][3][H/2][W/2], H = W a power of two >= 32; x and y 16-byte aligned. */
int pg_swd_pyr_down(int B, int H, int W, const float* x, int quantize, float* y, void* stream);
/* desc [B*K][3][7][7]: the 7x7 patch of fine [B][3][S][S] around each centre pos [B*K][2] =
 * (y, x) int32 (patches b*K .. b*K+K-1 from image b; centres in [3, S-3), the caller's duty),
 * minus, if coarse != NULL ([B][3][S/2][S/2]), up(coarse) at those pixels: zero-insert to
 * double size, filter with 4 k (x) k, same boundary (the Laplacian level, never materialised).
 * quantize applies to fine.  S >= 16. */
int pg_swd_descriptors(int B, int S, const float* fine, const float* coarse, int K, const int* pos,
                       int quantize, float* desc, void* stream);
/* mean3[c], rstd3[c] = per-channel mean and 1 / population standard deviation over the n * 49
 * values of channel c of desc [n][3][49] (two passes: the mean, then the centred squares;
 * fp32 partials per workgroup in `scratch`, combined in double). */
int pg_swd_stats(size_t n, const float* desc, float* mean3, float* rstd3, void* scratch,
                 void* stream);
/* proj[p * proj_stride + i] = sum_j ((desc[i][j] - mean3[c(j)]) * rstd3[c(j)]) * dirs[j * P + p]
 * for i < n, p < P, j < 147, c(j) = j / 49 (fp32 FMA); elements i >= n of a row are not
 * written.  proj_stride >= n. */
int pg_swd_project(size_t n, const float* desc, const float* mean3, const float* rstd3, int P,
                   const float* dirs, float* proj, size_t proj_stride, void* stream);
/* out[0] += sum over p < P, i < n of |a[p * stride + i] - b[p * stride + i]|, in a fixed order
 * (fp32 partials per workgroup in `scratch`, combined in double).  P <= 65535. */
int pg_swd_l1(int P, size_t n, const float* a, const float* b, size_t stride, float* out,
              void* scratch, void* stream);

/* ---- multi-scale structural similarity between image pairs (the PGGAN paper's diversity
 * metric; DESIGN.md "Validation: MS-SSIM").  All fp32; images NCHW [3][S][S].
 * One scale of P pairs.  a / b: the two sides of the first pair, the two sides of pair p at
 * a + p * img_stride and b + p * img_stride (floats; pairs interleaved in one [2P][3][S][S]
 * batch: b = a + 3 S^2, img_stride = 6 S^2).  `quantize` != 0 reads the images as 8-bit like
 * pg_swd_pyr_down (scale 0), otherwise they are taken as they are, on the 0..255 scale.
 * taps: T window weights (HOST memory, read during the call), 1 <= T <= min(11, S); the 2-D
 * window is taps (x) taps, filtering is "valid": n = S - T + 1 positions per axis.  With F the
 * filter, mu1 = F(a), mu2 = F(b), s11 = F(a a) - mu1^2, s22 = F(b b) - mu2^2, s12 = F(a b) -
 * mu1 mu2, c1 = 2.55^2, c2 = 7.65^2, v1 = 2 s12 + c2, v2 = s11 + s22 + c2:
 *   sums[p][0] = sum over the 3 n^2 positions of (2 mu1 mu2 + c1) v1 / ((mu1^2 + mu2^2 + c1) v2)
 *   sums[p][1] = sum over the 3 n^2 positions of v1 / v2
 * (fp32 partials per workgroup in `ws`, combined in double in a fixed order).  pool_a / pool_b
 * [P][3][S/2][S/2], both or neither: the aligned 2x2 means of the two sides as read (after
 * `quantize`), the next scale's input; S must be even.  ws: pg_msssim_workspace_bytes(P, S, T)
 * of device memory.  P <= 65535.  16-byte loads when S % 4 == 0 and a, b, img_stride and the
 * pooled outputs are 16-byte aligned, scalar loads otherwise. */
size_t pg_msssim_workspace_bytes(int P, int S, int T);
int pg_msssim_scale(int P, int S, int T, const float* taps, const float* a, const float* b,
                    size_t img_stride, int quantize, float* sums, float* pool_a, float* pool_b,
                    void* ws, size_t ws_bytes, void* stream);
/* out[p] = prod_{s < 4} max(cs_s, 0)^w_s * max(ssim_4, 0)^w_4 with ssim_s = sums[s][p][0] /
 * counts[s], cs_s = sums[s][p][1] / counts[s], w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333);
 * sums [5][P][2] from five pg_msssim_scale calls, counts: the five 3 n_s^2 (HOST memory),
 * evaluated in double. */
int pg_msssim_combine(int P, const float* sums, const long long* counts, float* out, void* stream);

/* ---- nearest training images: exact squared L2 between 8-bit images in integers (the PGGAN
 * paper's nearest-neighbour figure; DESIGN.md "Validation: nearest training images").
 * Descriptor of an S x S image at the comparison resolution Rc (powers of two, 8 <= Rc <= 128,
 * Rc <= S), f = S / Rc: the 8-bit pixels box-pooled in integers, (sum of the f x f block +
 * f^2 / 2) / f^2 rounded down, minus 128: int8 [Rc][Rc][3] in (y, x, c) order, D = 3 Rc^2 bytes
 * per row.  desc [B][D], sq[b] = sum of the squares of row b.  _f32 takes NCHW fp32
 * [B][3][S][S] in [-1, 1], read as 8-bit like pg_swd_pyr_down; _u8 takes NHWC uint8
 * [B][S][S][3].  x and desc 16-byte aligned; every source byte is read once.  B <= 65535. */
int pg_nn_descriptors_f32(int B, int S, int Rc, const float* x, int8_t* desc, int* sq,
                          void* stream);
int pg_nn_descriptors_u8(int B, int S, int Rc, const uint8_t* x, int8_t* desc, int* sq,
                         void* stream);
/* Merges one database chunk into the running best lists of Q queries: afterwards best_d2[i] /
 * best_idx[i] ([Q][k] int64, 1 <= k <= 16) hold the k smallest pairs (d^2, index), in
 * lexicographic order (a tie goes to the lower index), among the pairs they held and
 * (sq_q[i] + sq_x[j] - 2 q[i] . db[j], first_index + j), j < N.  The caller starts the lists at
 * (INT64_MAX, -1), which is what slots beyond the rows seen so far keep; indices must differ
 * between the chunks of one search, and then the result does not depend on how the database
 * was split.  q [Q][D], db [N][D] int8 rows (16-byte aligned), qsq / dbsq their int32 sums of
 * squares; D a multiple of 64, at most 49152 (so d^2 < 2^32 and the dot product fits int32);
 * first_index + N < 2^31.  The dot products are v_mfma_i32_16x16x64_i8; a workgroup takes
 * pg_nn_row_block() database rows and writes its k best per query to ws, a second launch merges
 * those with the running lists: no atomics, bitwise repeatable.  ws: pg_nn_workspace_bytes(Q, N,
 * k) of device memory, 8-byte aligned. */
int pg_nn_row_block(void);
size_t pg_nn_workspace_bytes(int Q, int N, int k);
int pg_nn_search(int Q, int N, int D, int k, const int8_t* q, const int* qsq, const int8_t* db,
                 const int* dbsq, long long first_index, long long* best_d2, long long* best_idx,
                 void* ws, size_t ws_bytes, void* stream);

/* ---- latent recovery: minimise a multi-scale pixel loss between G(z) and a target over z
 * (DESIGN.md "Validation: latent recovery").
 * pg_recon_loss: img, tgt, gimg fp32 NCHW [B][3][R][R] (16-byte aligned), R a power of two >= 4,
 * 1 <= levels <= min(6, log2 R + 1), B <= 512.  With d = img - tgt and d_l its 2^l x 2^l box
 * average (side R_l = R / 2^l):
 *   loss[b] = sum_{l < levels} 1 / (3 R_l^2) sum_{c,y,x} d_l^2,   mse0[b] = the l = 0 term,
 *   gimg[b][c][y][x] = d loss[b] / d img = 2 / (3 R^2) sum_{l < levels} d_l[c][y >> l][x >> l].
 * One launch: both inputs read once, gimg written once, loss and mse0 WRITTEN (not accumulated)
 * from per-workgroup partials summed in a fixed order through `scratch` (the stream's
 * PG_SCRATCH_BYTES reduction scratch): no float atomics, bitwise repeatable. */
int pg_recon_loss(int B, int R, int levels, const float* img, const float* tgt, float* gimg,
                  float* loss, float* mse0, void* scratch, void* stream);
/* One optimiser step on the latent rows z [B][Lz] (fp32; Lz a multiple of 64, at most 512), one
 * wave per row, in this order:
 *   1. if loss[b] < best_loss[b]: best_loss[b] = loss[b], best_z[b] = z[b] (loss: that of the
 *      current z, as pg_recon_loss wrote it -- the loop reads nothing back per iteration);
 *   2. gz = r (gzn - zn mean(zn gzn)), r = rsqrt(mean(z^2) + 1e-8), zn = z r: the PixelNorm
 *      backward (lib/layers.py:8-14) of gzn [B][Lz], the gradient at zn = pixel_norm(z);
 *   3. Adam on z with gz (m, v [B][Lz]; the 1-based `step`; pg_adam's update order; the
 *      hyper-parameters are doubles, so 1 - beta is rounded to fp32 once, not beta first);
 *   4. gz_out [B][Lz], if not NULL, = gz. */
int pg_latent_step(int B, int Lz, float* z, const float* gzn, float* m, float* v, double lr,
                   double beta1, double beta2, double eps, int step, const float* loss,
                   float* best_loss, float* best_z, float* gz_out, void* stream);

/* ---- radial power spectrum of images (the network-free check of a generator's high
 * frequencies; DESIGN.md "Validation: power spectrum").  All fp32; x NCHW [B][3][R][R], R a
 * power of two, 8 <= R <= 1024, 1 <= B <= 65535.  Per image:
 *   1. `quantize` != 0: q = rint(clip(127.5 x + 127.5, 0, 255)), ties to even, as
 *      pg_swd_pyr_down reads an image; otherwise q = x, taken on the 0..255 scale;
 *   2. luma, shifted: y = 0.299 (q_r - 127.5) + 0.587 (q_g - 127.5) + 0.114 (q_b - 127.5);
 *   3. F(u, v) = sum_{r,c} y(r, c) exp(-2 pi i (u r + v c) / R): unnormalised, no window; the
 *      signed frequencies u, v lie in [-R/2, R/2);
 *   4. (u, v) belongs to radius bin k, the one integer with k^2 - k < u^2 + v^2 <= k^2 + k
 *      ((0, 0): bin 0) -- round(sqrt(u^2 + v^2)) in integers; bins k > R/2 are dropped;
 *   5. prof[b][k] = sum over the full plane of |F(u, v)|^2 in bin k, k = 0 .. R/2.
 * A real 2-D FFT in LDS (twiddles from sincospif of exact arguments); the complex spectrum is
 * never written out.  R <= 64: one launch, one workgroup per image.  Larger R: a row pass
 * that stores the half spectrum transposed in `ws`, a column pass that writes fp32 bin sums
 * per workgroup to `ws`, and a launch that adds an image's partials in double in a fixed order.
 * No float atomics: an image's profile is bitwise repeatable and does not depend on B or on
 * its place in the batch.  ws: pg_spectrum_workspace_bytes(B, R) of device memory (0 for
 * arguments out of range; at most about 33 MB: images are taken in chunks).  x, prof and ws
 * non-null and 16-byte aligned; every failed check is PG_ERR_ARG before any launch. */
size_t pg_spectrum_workspace_bytes(int B, int R);
int pg_spectrum_profile(int B, int R, const float* x, int quantize, float* prof /* [B][R/2+1] */,
                        void* ws, size_t ws_bytes, void* stream);

/* ---- training health: per-tensor statistics of a net's flat fp32 buffers and the every-step
 * non-finite probe (DESIGN.md "Training health"; pggan_amd/health.py).
 * A segment table is a DEVICE array of nseg int64 pairs {offset, count} into one flat fp32
 * buffer of n floats: offsets are multiples of 16 floats, count is the tensor's true element
 * count, segments are disjoint and ascending and end at or before n.  The floats between
 * offset + count and the next offset are padding and are never read (whole quads are 16-byte
 * loads, a tensor's last 1 .. 3 elements scalar loads; every byte is read once).
 *
 * pg_tensor_stats: p, g, m, v are flat fp32 device buffers of n floats with that layout, each
 * nullable.  out [nseg][PG_TS_COLS] doubles (device) is WRITTEN, per segment:
 *   0-2  sumsq_p, sumsq_g, sumsq_u    sums of squares over the finite elements
 *   3-5  maxabs_p, maxabs_g, maxabs_u largest magnitudes over the finite elements
 *   6-9  bad_p, bad_g, bad_m, bad_v   elements that are +-Inf or NaN
 * u = step_size m / (sqrt(v) / bc2_sqrt + eps), the magnitude of the update pg_adam applies from
 * these moments; {step_size, bc2_sqrt} is the pair pg_adam_table holds for that update.  u is
 * evaluated in double from the fp32 m, v and scalars, each operation rounded on its own, and
 * taken only where both m and v are finite (v >= 0, as Adam leaves it).  Columns whose buffer
 * is NULL are 0 (the u columns need both m and v).  All sums are double: the square of an fp32
 * value is exact there.  The buffer is cut into ranges of pg_tensor_stats_chunk() floats, one
 * wave each, whatever the segment sizes; a second launch combines the per-(segment, range)
 * partials in `ws` in a fixed order: no atomics, bitwise repeatable.  ws:
 * pg_tensor_stats_workspace_bytes(nseg, n) of device memory (0 for arguments out of range).
 * table, the buffers, out and ws 16-byte aligned; every failed check is PG_ERR_ARG before any
 * launch.
 *
 * pg_nonfinite_watch: one launch over x[0, n) that tests exponent bits only.  For every
 * segment that holds a non-finite element and whose first_bad [nseg] (device ints, 0 = never)
 * is still 0, first_bad[segment] = tag (> 0).  Nothing is read back; plain vector stores, and
 * every writer of a slot within a launch writes the same value. */
#define PG_TS_COLS 10
int pg_tensor_stats_chunk(void);
size_t pg_tensor_stats_workspace_bytes(int nseg, size_t n);
int pg_tensor_stats(int nseg, const int64_t* table, size_t n, const float* p, const float* g,
                    const float* m, const float* v, float step_size, float bc2_sqrt, float eps,
                    double* out /* [nseg][PG_TS_COLS] */, void* ws, size_t ws_bytes, void* stream);
int pg_nonfinite_watch(int nseg, const int64_t* table, const float* x, size_t n, int tag,
                       int* first_bad /* [nseg] */, void* stream);

/* ---- stream ordering between the engine's streams (weight gradients on a side stream).
 * torch's cross-stream events record with a system-scope release: every record writes back and
 * invalidates the L2 of all XCDs and the next kernel on that stream starts ~6.5 us late.  The
 * two streams are on one device, so these events release to device scope only
 * (hipEventReleaseToDevice).  `timing` != 0: a timing event that skips the system fence
 * (hipEventDisableSystemFence; a default timing event where the runtime rejects that flag), for
 * the bench's per-launch timers.  Handles are opaque. */
int pg_event_create(int timing, void** ev);
int pg_event_record(void* ev, void* stream);
int pg_stream_wait_event(void* stream, void* ev);
int pg_event_elapsed_ms(void* ev_start, void* ev_end, float* ms);
/* A non-blocking stream of the library's own; lowest_priority != 0: at the device's least
 * priority (its own hardware-queue pool, so never the queue of a normal-priority stream) */
int pg_stream_create(int lowest_priority, void** stream);
int pg_stream_destroy(void* stream);
int pg_event_destroy(void* ev);

/* ---- device memory helpers that take part in recordings: zero `bytes` at p / copy `bytes`
 * device to device, asynchronously on `stream` (the step's gradient and loss resets and its
 * input copies, so a recorded step needs no torch op) */
int pg_fill_zero(void* p, size_t bytes, void* stream);
int pg_copy(void* dst, const void* src, size_t bytes, void* stream);

/* ---- launch recorder (the training step replayed from C++; reference hot loop train.py:39-66).
 * Between pg_record_begin and pg_record_end every kernel launch, pg_event_record,
 * pg_stream_wait_event, pg_fill_zero and pg_copy this host thread issues runs as usual AND is
 * appended to a recording (function, geometry, stream, arguments by value).  pg_replay issues
 * the same sequence again on the same streams: one C++ loop instead of the Python layer that
 * produced it, and -- unlike a hipGraph -- the streams and their hardware queues are the
 * recorded ones.  The caller guarantees that every pointer the recording holds still points to
 * the same live buffers and that their contents (inputs, step counters) are meant to be
 * re-read; a recording is replayed on the thread's current device.  Handles are opaque. */
int pg_record_begin(void);
int pg_record_end(void** rec);
int pg_record_count(const void* rec);
int pg_replay(const void* rec);
void pg_record_destroy(void* rec);

/* ---- replay plan: cross-stream bookkeeping a recording carries and its result does not need.
 * pg_record_optimize rewrites a recording once, on the host, over each op's kind, stream and
 * event; it never reorders ops, and eager execution is untouched.  Two rules:
 *   redundant waits  a wait of stream S on event E is dropped when S is already ordered, by its
 *                    own earlier waits (followed transitively: per-stream vector clocks), behind
 *                    the point of E's stream at which E was recorded, or when E was recorded on
 *                    S itself.  What a stream ran before the recording (the previous replay)
 *                    counts as work no other stream is behind yet;
 *   dead records     only with closed != 0, the caller's promise that nothing outside this
 *                    recording consumes an event it records -- no stream wait, and no host-side
 *                    synchronize, query or elapsed-time call on it either (only stream waits
 *                    inside the recording count as uses): a record of E is dropped when no
 *                    surviving wait on E follows it before E's next record or the end.  The
 *                    promise is refused, and the recording left exactly as it was, when the
 *                    recording waits on an event it has not recorded earlier (stats.closed = 0).
 * A third rule, a record right behind a launch issued as that launch's stop event
 * (hipExtLaunchKernel), was built and measured: it gained nothing beside the dropped records
 * and is not part of the pass (DESIGN.md "Streams").
 * Calling it again plans the recording afresh.  `stats` may be null.
 * pg_replay_plan_host runs the same pass on the host over n synthetic ops, three int32 each:
 * kind (PG_OP_*), stream id, event id (any value where the kind has none), ids >= 0; flags_out
 * [n] receives a PG_PLAN_* per op.  It needs no device. */
#define PG_OP_LAUNCH 0
#define PG_OP_RECORD 1
#define PG_OP_WAIT 2
#define PG_OP_FILL 3
#define PG_OP_COPY 4
#define PG_PLAN_KEEP 0
#define PG_PLAN_DROP 1
typedef struct pg_replay_stats {
  int32_t ops, records, records_dropped, waits, waits_dropped;
  int32_t closed; /* whether the closed promise was asked for and accepted */
} pg_replay_stats;
int pg_record_optimize(void* rec, int closed, pg_replay_stats* stats);
int pg_replay_plan_host(const int32_t* ops, int n, int closed, int32_t* flags_out);

/* ---- step plan: the kernel path of every 3x3 conv pass (forward, input
 * gradient, weight gradient) of one train_step at (stage, batch, dtype) -- the layer list of
 * pggan/nets.py:53-119 (G) and :164-239 (D) at scale_index = stage -- and the split-reduction
 * workspace the step needs (the max over its conv / wgrad launches).  Plans are immutable
 * after creation (thread-safe to read); the caller owns the workspace memory. */
typedef struct pg_step_plan pg_step_plan;
int pg_step_plan_create(int dtype, int n_depths, const int* depths, int stage, int batch,
                        pg_step_plan** out);
size_t pg_step_plan_workspace_size(const pg_step_plan* plan);
/* human-readable table of the plan (one line per conv layer) into buf */
int pg_step_plan_describe(const pg_step_plan* plan, char* buf, size_t len);
void pg_step_plan_destroy(pg_step_plan* plan);

#ifdef __cplusplus
}
#endif
#endif
