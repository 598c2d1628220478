/* resshift_hip.h — C ABI of the MI355X-native ResShift sampling engine (libresshift_hip.so).
 *
 * The reference (zsyOAOA/ResShift) is pure Python/PyTorch and has no FFI of its own; its only
 * extension point is the YAML `target:` string resolved by utils/util_common.py:19-29.  The entry
 * points below are therefore exactly what a ctypes binding of the reference's hot path needs:
 * each one replaces the body of one reference call (file:line cited per function), takes plain
 * pointers and sizes, and never sees a torch type.  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (rs_last_error() has the text);
 *   - "dev" pointers are device pointers valid on the current HIP device (e.g. torch
 *     Tensor.data_ptr()); the engine never frees caller memory;
 *   - user-facing image / latent tensors are NCHW fp32 like the reference's; the NHWC fp16/fp32
 *     working layout is internal;
 *   - work is enqueued on the caller's hipStream_t (pass torch's current stream) - every launch, memset and copy of a call, on any
 *     stream, non-blocking ones included: nothing relies on the null stream's legacy ordering (tests/test_streams_gpu.py runs every
 *     entry on a side stream behind a producer that is still running).  After one warm-up call of the same shapes (the scratch arena
 *     grows and a timestep's FiLM row is built behind a stream synchronise, on first use) the network, sampling, tile and image calls
 *     return without waiting for the stream; rs_jpeg_encode's host wrapper, the debug trace and the rs_op_* test entries may wait;
 *   - one engine per device, not thread-safe.  An engine's scratch (arena, GroupNorm pools, tickets, FiLM rows, key staging) is shared
 *     by its calls, so the caller orders the calls of ONE engine across streams (event / stream wait); calls of different engines, and
 *     the stateless rs_tile_* / image operators, need no ordering among themselves: there is no device-global scratch;
 *   - precision: RS_PREC_F16 = fp16 storage / fp32 accumulate MFMA, RS_PREC_F32 = fp32 storage /
 *     exact fp32 MFMA, RS_PREC_SPLIT = (hi, lo) fp16 pair storage (x = hi + lo * 2^-11, 4 bytes per
 *     element) / three fp16 MFMAs per product, fp32 accumulate: fp32-class results at 1/3 of the
 *     fp16 matrix rate (the precision that keeps the VQ codes of ldm/modules/vqvae/quantize.py:276-285);
 *   - size limit: no single working tensor that an MFMA conv, GEMM or fused attention kernel reads may reach 0xF0000000 bytes (3.75 GiB;
 *     RS_BUFFER_BYTES_LIMIT in csrc/common.h - those kernels add 32-bit byte offsets to a buffer descriptor).  The engine finds out while
 *     it plans the call, before anything is launched: the call returns -7 and rs_last_error() names the layer, the operand, its bytes, the
 *     limit and the largest batch that fits that operand (faceir at 512 x 512 in split storage: 59 images per call; the realsr autoencoder at
 *     256 x 256: 119 in split and in fp16 storage).  Chunking a larger batch is the caller's business.  Every kernel family is
 *     tested against float64 on operands past 2^31 bytes, or past 2^31 elements (tests/test_large_tensors_gpu.py).
 */
#ifndef RESSHIFT_HIP_H
#define RESSHIFT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_PREC_F16 0
#define RS_PREC_F32 1
#define RS_PREC_SPLIT 2
#define RS_MAX_LEVELS 8
#define RS_MAX_STEPS 64
/* most images one per-image call may carry (rs_sample_step with mixed step indices, rs_axpbypcz_rows, rs_unet_forward with unequal
 * timesteps): their coefficients / FiLM row pointers travel as kernel arguments */
#define RS_MAX_ROWS 64

typedef struct rs_engine rs_engine;

/* models/unet.py:632-657 (UNetModelSwin.__init__ arguments that shape the network) */
typedef struct rs_unet_config {
    int image_size, in_channels, model_channels, out_channels;
    int n_levels;
    int channel_mult[RS_MAX_LEVELS];
    int num_res_blocks[RS_MAX_LEVELS];
    int n_attn_res;
    int attention_resolutions[RS_MAX_LEVELS];
    int swin_depth, swin_embed_dim, window_size, num_heads;
    float mlp_ratio;
    int cond_lq, cond_mask, lq_size;
} rs_unet_config;

/* ldm/models/autoencoder.py:13-26 + ldm/modules/diffusionmodules/model.py:452-456,550-554 (ddconfig) */
typedef struct rs_ae_config {
    int ch, n_levels;
    int ch_mult[RS_MAX_LEVELS];
    int num_res_blocks[RS_MAX_LEVELS];   /* per level (an int in the YAML is broadcast, model.py:464-468) */
    int in_channels, out_ch, z_channels, embed_dim, n_embed, resolution;
    int n_attn_res;
    int attn_resolutions[RS_MAX_LEVELS];
} rs_ae_config;

typedef struct rs_config {
    rs_unet_config unet;
    rs_ae_config ae;
    int has_unet;     /* build the UNetModelSwin graph   */
    int has_ae;       /* build the VQModelTorch graph    */
    int enable_f16;   /* pack fp16 weights  */
    int enable_f32;   /* pack fp32 weights (exact mode) */
    int enable_split; /* pack (hi, lo) fp16 pair weights (RS_PREC_SPLIT) */
} rs_config;

/* Arguments of one full sampling call: gaussian_diffusion.py:367-472 (p_sample_loop) */
typedef struct rs_sample_args {
    const float* y;        /* dev, [B,3,h,w] LR image in [-1,1]                     */
    const float* mask;     /* dev, [B,1,h,w] or NULL (inpainting, sampler.py:140)    */
    const float* noise;    /* dev, [steps+1][B,Cz,hz,wz]: prior noise then one per step in loop order (t=T-1..0) */
    float* out;            /* dev, [B,3,h*sf,w*sf] decoded image (not clamped)       */
    float* z_out;          /* dev, optional [B,Cz,hz,wz] final latent before VQ      */
    int32_t* idx_out;      /* dev, optional [B*hz*wz] VQ code indices                */
    int B, h, w, sf, steps;
    /* per-step scalars, index = timestep t (float64 numpy -> float, gaussian_diffusion.py:143-161,602) */
    float inv_std[RS_MAX_STEPS];   /* 1/sqrt(eta_t*kappa^2+1)              (_scale_input)       */
    float coef1[RS_MAX_STEPS];     /* eta_{t-1}/eta_t                      (posterior_mean_coef1) */
    float coef2[RS_MAX_STEPS];     /* alpha_t/eta_t                        (posterior_mean_coef2) */
    float sigma[RS_MAX_STEPS];     /* exp(0.5*posterior_log_variance_clipped[t])              */
    int tmap[RS_MAX_STEPS];        /* respace.py:61-70 timestep_map                           */
    float prior_scale;             /* kappa*sqrt_eta_{T-1}                 (prior_sample)       */
    float scale_factor;            /* diffusion.params.scale_factor                           */
    int prec_encode, prec_decode;
    int prec_unet[RS_MAX_STEPS];   /* precision of the UNet call at timestep t */
    void* stream;                  /* hipStream_t */
} rs_sample_args;

/* Arguments of one step of a batch whose images may be at different steps (rs_sample_step; continuous batching): one p_sample
 * (gaussian_diffusion.py:332-365) of image b at step index t[b] */
typedef struct rs_step_args {
    const rs_sample_args* sched;   /* the schedule: its inv_std / coef1 / coef2 / sigma / tmap tables, steps and the LR geometry h, w, sf
                                      are read (its B, tensors and precisions are not) */
    float* x;              /* dev, [B,Cz,hz,wz] x_t in, x_{t-1} out (in place)                        */
    float* pred_xstart;    /* dev, optional [B,Cz,hz,wz] the UNet's prediction of x_0                 */
    const float* y;        /* dev, [B,3,h,w] LR conditioning of each image                            */
    const float* mask;     /* dev, [B,1,h,w] or NULL                                                  */
    const float* noise;    /* dev, [B,Cz,hz,wz] this step's draw of each image (unused for t[b] = 0) */
    const int* t;          /* HOST, [B] step indices into the schedule's tables (0 .. steps-1)        */
    int B;                 /* images; unequal t[] allows at most RS_MAX_ROWS                         */
    int prec;              /* UNet precision of this step                                             */
    void* stream;          /* hipStream_t */
} rs_step_args;

/* ---- lifetime ------------------------------------------------------------------------------ */
rs_engine* rs_create(const rs_config* cfg);
void rs_destroy(rs_engine* e);
const char* rs_last_error(void);

/* ---- weights: replaces utils/util_net.py:86-98 (reload_model) + sampler.py:108-112 ----------- */
/* hand over one state_dict entry (fp32 host memory, reference key name, reference shape) */
int rs_load_tensor(rs_engine* e, const char* state_dict_key, const float* host, const int64_t* shape, int ndim);
/* size of the packed device blob for this config; layout is a pure function of the config */
size_t rs_weight_bytes(rs_engine* e);
/* caller-owned device storage for the blob (so the caller can RCCL-broadcast it as one message) */
int rs_bind_weight_blob(rs_engine* e, void* dev, size_t bytes);
/* pack everything loaded so far into the bound blob (GEMM-ready [Cout][kh][kw][Cin] fp16/fp32,
 * expanded relative-position bias tables, codebook, ...); only the broadcasting rank needs to call it */
int rs_pack_weights(rs_engine* e);
/* broadcast the bound blob from rank `root` over the HOST's RCCL communicator (`rccl_comm`: an ncclComm_t; one ncclBroadcast of
 * rs_weight_bytes() bytes, in place, on `stream`): what replaces the reference's per-rank checkpoint load (sampler.py:66-77, utils/util_net.py
 * reload_model) for a host without torch.distributed.  RCCL is dlopen'ed at call time - no link dependency.  The call synchronises `stream`
 * before it returns, so the received bytes are there: every rank calls rs_weights_ready() afterwards, which reads the blob's header and
 * per-layer flags back with plain copies, and needs no synchronisation of the caller's in between. */
int rs_bcast_weights(rs_engine* e, void* rccl_comm, int root, void* stream);
/* tell the engine the blob content is valid (after pack or after a broadcast) */
int rs_weights_ready(rs_engine* e);

/* ---- network calls ------------------------------------------------------------------------- */
/* models/unet.py:865-895 UNetModelSwin.forward(x, timesteps, lq, mask).  x [B,Cz,H,W], lq [B,3,Hl,Wl],
 * mask [B,1,Hl,Wl] or NULL, out [B,out_channels,H,W]; t_host = B timestep values on the host - any values (unequal ones: per-image
 * FiLM rows, at most RS_MAX_ROWS images). */
int rs_unet_forward(rs_engine* e, const float* x, const int* t_host, const float* lq, const float* mask, float* out,
                    int B, int H, int W, int Hl, int Wl, int prec, void* stream);
/* ldm/models/autoencoder.py:28-31 VQModelTorch.encode: img [B,3,H,W] -> z [B,embed_dim,H/f,W/f] */
int rs_vq_encode(rs_engine* e, const float* img, float* z, int B, int H, int W, int prec, void* stream);
/* ldm/models/autoencoder.py:33-40 VQModelTorch.decode: z [B,embed_dim,h,w] -> img [B,out_ch,h*f,w*f] */
int rs_vq_decode(rs_engine* e, const float* z, float* img, int32_t* idx_out, int B, int h, int w, int force_not_quantize,
                 int prec, void* stream);
/* F.interpolate(y, scale_factor=sf, mode='bicubic') — gaussian_diffusion.py:503-504; NCHW in / NCHW out */
int rs_bicubic(rs_engine* e, const float* y, float* out, int B, int C, int H, int W, int sf, void* stream);
/* the whole loop: encode_first_stage -> prior_sample -> steps x (UNet + posterior update) -> decode */
int rs_sample(rs_engine* e, const rs_sample_args* a);
/* the same loop in three parts, for a scheduler that admits and retires images at every step (continuous batching; rs_sample is
 * begin + steps x step + end with the same launches):
 *   rs_sample_begin: encode_first_stage(y, up_sample) -> * scale_factor -> prior_sample with a->noise = the prior draw [B,Cz,hz,wz]
 *                    -> x_T [B,Cz,hz,wz] (reads y, noise, B, h, w, sf, prior_scale, scale_factor, prec_encode, stream);
 *   rs_sample_step:  one step of every image at its own step index (rs_step_args).  Equal indices run the launches of rs_sample's
 *                    step; unequal ones add one FiLM gather launch and take the elementwise coefficients per image - each image gets
 *                    bit for bit what it gets in a homogeneous batch of the same size.  Feature-extractor configs compute the conditioning features per call;
 *   rs_sample_end:   x_0 -> z_out, idx_out, out (reads out, z_out, idx_out, B, h, w, sf, scale_factor, prec_decode, stream). */
int rs_sample_begin(rs_engine* e, const rs_sample_args* a, float* x_T);
int rs_sample_step(rs_engine* e, const rs_step_args* s);
int rs_sample_end(rs_engine* e, const rs_sample_args* a, const float* x_0);
/* compute and cache the FiLM rows of these (network) timesteps now: the first call at a timestep otherwise builds its row and
 * synchronises the stream once (a scheduler calls this with the schedule's tmap before its first step) */
int rs_film_prewarm(rs_engine* e, const int* timesteps, int n, void* stream);
/* fp32 y = a*x + b*z + c*n on device (posterior mean / prior sample for the step-wise API) */
int rs_axpbypcz(const float* x, const float* z, const float* n, float* y, float a, float b, float c, long long count, void* stream);
/* the same with one coefficient triple per image (host arrays a[B], b[B], c[B]; b / c may be NULL when z / n are): image r covers elements
 * [r * per_image_count, (r + 1) * per_image_count); c[r] == 0 skips image r's noise term.  B <= RS_MAX_ROWS.  Per-sample
 * _extract_into_tensor arithmetic of the host mirror (gaussian_diffusion.py:92-105): _scale_input, posterior mean, p_sample, q_sample */
int rs_axpbypcz_rows(const float* x, const float* z, const float* n, float* y, const float* a, const float* b, const float* c,
                     long long per_image_count, int B, void* stream);

/* ---- per-request seeds: Philox noise generated inside the sampler ---------------------------------
 * A draw is a pure function of (seed, stream, draw index, element index): element i (index in the image's OWN latent [Cz,hz,wz], NCHW
 * order) of draw k (k = 0: the prior draw of prior_sample, gaussian_diffusion.py:446,517-529; k = steps - t: the draw of the step at step
 * index t, :358) is Box-Muller on Philox4x32-10 with counter (i / 4, k, stream, 0) and key (seed & 0xffffffff, seed >> 32); words
 * (w0, w1) give elements 4q, 4q+1 and (w2, w3) elements 4q+2, 4q+3: u1 = ((wa >> 8) + 1) 2^-24, u2 = (wb >> 8) 2^-24,
 * r = sqrtf(-2 logf(u1)), pair = (r cospi(2 u2), r sinpi(2 u2)).  `seed` names the request, `stream` a sub-request (the tile index
 * inside an image; 0 for a whole image).  Equal keys give equal noise bits in any call, batch, slot or process. */
typedef struct rs_noise_key {
    uint64_t seed;
    uint32_t stream;
    uint32_t reserved;     /* must be 0 */
} rs_noise_key;
/* out[b][i] = normal i of draw draw[b] of keys[b] (dense fp32 [B][per_image_count]; keys and draw are HOST arrays): the definition
 * above made callable, for tests and for a host that wants tensors.  -2: B outside 1 .. RS_MAX_ROWS, null pointer, reserved != 0,
 * negative draw, per_image_count < 1. */
int rs_noise_fill(const rs_noise_key* keys, const int* draw, float* out, long long per_image_count, int B, void* stream);
/* rs_sample / rs_sample_begin / rs_sample_step with the noise generated in registers by the kernel that consumes it: image b uses
 * keys[b] (HOST array of a->B resp. s->B keys) and the `noise` member of the struct is ignored.  Same launches as the tensor calls
 * (rs_last_launch_count), bit for bit what the tensor call gives when fed rs_noise_fill's output.  rs_sample_seeded accepts any B
 * (keys of a batch above RS_MAX_ROWS are copied to the device once per call); rs_sample_step_seeded keeps rs_sample_step's
 * RS_MAX_ROWS rule for mixed step indices.  -2: null keys, reserved != 0, B out of range. */
int rs_sample_seeded(rs_engine* e, const rs_sample_args* a, const rs_noise_key* keys);
int rs_sample_begin_seeded(rs_engine* e, const rs_sample_args* a, float* x_T, const rs_noise_key* keys);
int rs_sample_step_seeded(rs_engine* e, const rs_step_args* s, const rs_noise_key* keys);

/* overlap-average tiling of large images (utils/util_image.py:889-979 ImageSpliterTh.update / .gather): NCHW fp32,
 * acc[b,c,h0:h0+th,w0:w0+tw] += tile, count[h0:h0+th,w0:w0+tw] += 1; finalize divides acc by count in place */
int rs_tile_accumulate(float* acc, float* count, const float* tile, int B, int C, int H, int W, int h0, int w0, int th, int tw,
                       void* stream);
int rs_tile_finalize(float* acc, const float* count, int B, int C, int H, int W, void* stream);
/* fp32 planes [planes][H][W] -> [planes][Ho][Wo]: out[i][j] = scale * in[refl(h0 + i)][refl(w0 + j)], refl(i) = i < n ? i : 2(n-1) - i.
 * The host mirror's data movement on the device: reflect padding of the LQ batch (sampler.py:130-138), the tile crop of the
 * tiled path (utils/util_image.py:946-952; the window must then lie inside the plane) and the latent scaling of
 * encode_first_stage (models/gaussian_diffusion.py:514).  -2 when the window overhangs the plane by a full plane size or more. */
int rs_window_copy(const float* in, float* out, long long planes, int H, int W, int h0, int w0, int Ho, int Wo, float scale, void* stream);

/* ---- tile pool (resshift_amd/tilepool.py): tiles of DIFFERENT images in one launch -------------------------------
 * One descriptor per tile, passed by value to the kernels (host array, at most RS_MAX_ROWS per call).  (H, W) is the LR plane of the
 * tile's image, (h0, w0, th, tw) the tile's window in it (utils/util_image.py:946-952; th = min(pch_size, H), likewise tw). */
typedef struct rs_tile_desc {
    const float* src;      /* gather:  dev, [C_src,H,W] LR planes of the tile's image (the mask, if any, as last plane) */
    float* acc;            /* scatter: dev, [C,H*sf,W*sf] running sum of the tile's image                              */
    float* count;          /* scatter: dev, [H*sf,W*sf] tiles that covered each pixel so far                           */
    int H, W, h0, w0, th, tw;
} rs_tile_desc;
/* for tile k < n: out_lq[k] [3,Hp,Wp] (and out_mask[k] [1,Hp,Wp] when C_src == 4, else out_mask is NULL) = the window of desc[k].src,
 * reflect-padded on the bottom / right edge RELATIVE TO THE WINDOW (row i reads window row i < th ? i : 2(th-1) - i), which is
 * F.pad(mode='reflect') of the cropped tile (sampler.py:130-138 after util_image.py:946-952).  One launch instead of a crop, the
 * channel split and two paddings per tile.  -2: n outside 1 .. RS_MAX_ROWS, C_src not 3 / 4, a null pointer, a window that leaves its
 * plane, th > Hp or tw > Wp, a reflect pad of a full tile side or more. */
int rs_tile_gather(const rs_tile_desc* desc, int n, int C_src, float* out_lq, float* out_mask, int Hp, int Wp, void* stream);
/* for tile k < n: desc[k].acc[:, h0*sf : (h0+th)*sf, w0*sf : (w0+tw)*sf] += tiles[k][:, :th*sf, :tw*sf] (tiles [n,C,Hp_out,Wp_out]) and
 * desc[k].count += 1 there: ImageSpliterTh.update (util_image.py:954-970) for tiles of several images at once.  Tiles of one call may
 * overlap in one canvas: every canvas element is written by ONE thread, which adds the covering tiles in index order onto the value
 * already there - the bits of n successive rs_tile_accumulate calls in index order, no atomics.  Descriptors with the same `acc` must
 * agree in count, H and W; distinct canvases must not alias.  -2: as rs_tile_gather, sf < 1, th*sf > Hp_out or tw*sf > Wp_out. */
int rs_tile_scatter(const rs_tile_desc* desc, int n, int C, int sf, const float* tiles, int Hp_out, int Wp_out, void* stream);

/* ---- feathered tile blending (opt-in; the uniform average above stays the default and keeps its bits) -------------
 * Overlapping tiles are independent samples, so a uniform average steps by (A + B)/2 - A at every overlap edge.  Feathering weights a
 * tile down towards its own edges, so that the blend crosses an overlap in a ramp.  For a tile whose HR window is nh x nw pixels
 * (nh = th*sf, nw = tw*sf; for rs_tile_accumulate_weighted, whose arguments are HR pixels already, nh = th, nw = tw) and ramp widths
 * Rh, Rw in HR pixels, the same for every tile of a call (the host passes (chop_size - chop_stride) * sf for both):
 *     w1(p, n, R) = 1                                    if R == 0
 *                 = min(1, (min(p, n-1-p) + 0.5) / R)    otherwise          (symmetric, in (0, 1], n < 2R ramps up to less than 1)
 *     w(i, j)     = w1(i, nh, Rh) * w1(j, nw, Rw)
 *     acc  [.., y0+i, x0+j] += w(i, j) * tile[.., i, j]
 *     count[    y0+i, x0+j] += w(i, j)                    (the count plane holds a weight SUM now)
 * and the output is acc / count: rs_tile_finalize, unchanged.  Image borders need no special case: where one tile covers a pixel its
 * weight cancels in the division.  In fp32: w1 = fminf(1, ((float)min(p, n-1-p) + 0.5f) * (1.0f / (float)R)), w = w1h * w1w rounded
 * once, sum = fmaf(w, v, sum), count = count + w - the same expressions in both entry points, so rs_tile_scatter_weighted gives the
 * bits of rs_tile_accumulate_weighted called tile by tile in index order (one writer per canvas element, no atomics), and R = 0 gives
 * the bits of the unweighted calls.  tests/_feather_ref.py restates this in float64.
 * -2 (with rs_last_error): Rh < 0 or Rw < 0; accumulate: a null pointer, B, C, th or tw < 1, a window that leaves the canvas;
 * scatter: everything rs_tile_scatter rejects. */
int rs_tile_accumulate_weighted(float* acc, float* count, const float* tile, int B, int C, int H, int W, int h0, int w0, int th, int tw,
                                int Rh, int Rw, void* stream);
int rs_tile_scatter_weighted(const rs_tile_desc* desc, int n, int C, int sf, const float* tiles, int Hp_out, int Wp_out, int Rh, int Rw,
                             void* stream);

/* ---- colour correction against the low-quality input (opt-in) ----------------------------------------
 * A sample drifts in tone and colour from its input, and every tile of a large image drifts on its own.  The remedy keeps the sample's
 * detail and takes the low frequencies (wavelet) or the per-channel statistics (adain) from the up-sampled input: the
 * `color_fix = wavelet | adain` switch of StableSR's and of later ResShift samplers.  Stateless, like the rs_tile_* family.
 *   sr  [B,C,H*sf,W*sf]  fp32 NCHW in [-1,1]: the sample        lq  [B,C,H,W]  fp32 NCHW in [-1,1]: its input        sf >= 1
 *   up(lq) = rs_bicubic's definition (F.interpolate(mode='bicubic', align_corners=False): A = -0.75, border-clamped taps, the expressions
 *            of bicubic_up_kernel in csrc/elementwise.hip); up = identity at sf = 1.
 * RS_COLOR_FIX_WAVELET:  out = clamp(sr - L(sr - up(lq)), -1, 1)
 *   L = B_16 o B_8 o B_4 o B_2 o B_1, five a-trous levels, B_1 applied first (the order matters at the borders).  B_d is the separable
 *   3x3 kernel [1/4 1/2 1/4]^T [1/4 1/2 1/4] with dilation d: a horizontal pass, then a vertical one, each
 *       y[i] = 1/4 (x[clamp(i - d, 0, n-1)] + x[clamp(i + d, 0, n-1)]) + 1/2 x[i]
 *   (replicate padding of the level's OWN input).  This is high(sr) + low(up(lq)) of StableSR's wavelet_reconstruction: the decomposition
 *   is linear, replicate padding included, so it is written on the one difference image D = sr - up(lq).  Total reach: 31 pixels.
 *   In fp32: y = fmaf(0.25f, a + c, 0.5f * b) for the taps (a, b, c) - one expression for every pixel, clamped index or not, so the value
 *   of a pixel is a function of the image alone, not of the launch geometry.
 * RS_COLOR_FIX_ADAIN:  per image and channel  out = clamp((sr - mean_sr) * std_lq / std_sr + mean_lq, -1, 1)
 *   std = sqrt(unbiased variance + 1e-5) (a one-pixel plane has variance 0); the lq statistics are taken over the LR plane itself.  The
 *   variance comes from centred values (per-chunk means, chunks merged by Chan's update in a fixed order) - never E[x^2] - mean^2 - and
 *   without floating-point atomics: a plane's statistics do not depend on the batch it travels in.
 * tests/_colorfix_ref.py restates both in float64.
 * `work`: device scratch of rs_color_fix_work_bytes(...) bytes (0 for wavelet: work may be null), 4-byte aligned; `out` must not overlap
 * `sr` or `lq` (workgroups read sr in their neighbours' tiles).  Argument errors are found before anything is launched, -2 with
 * rs_last_error() starting "rs_color_fix: ": a null pointer, a dimension or sf below 1, an unknown mode, an overlapping out, a
 * workspace that is too small. */
#define RS_COLOR_FIX_WAVELET 1
#define RS_COLOR_FIX_ADAIN 2
size_t rs_color_fix_work_bytes(int B, int C, int H, int W, int sf, int mode);
int rs_color_fix(const float* sr, const float* lq, float* out, int B, int C, int H, int W, int sf, int mode, void* work, size_t work_bytes,
                 void* stream);

/* ---- antialiased resize to any output size (opt-in) ---------------------------------------------------
 * The network produces its own factor only (sf = 4, 2 or 1); another output scale ("x2 from the x4 model", "x3") is a resample of its
 * result.  The function is MATLAB's imresize with antialiasing - the resampler of the SR literature and of the reference's data
 * pipeline (utils/util_image.py:imresize_np), so it also makes bicubic LQ inputs the way the models were trained on.  Stateless.
 *   in  [B,C,H,W]  fp32 NCHW, contiguous, only read        out  [B,C,Ho,Wo]  fp32 NCHW, contiguous
 * One axis, input length n, output length m, scale s > 0:   a = min(s, 1),   kw = 4 / a,   P = ceil(kw) + 2.
 * Output index i (0-based), taps k = 0 .. P-1:
 *       u    = (i + 1) / s + 0.5 (1 - 1/s)
 *       left = floor(u - kw / 2)
 *       tap k has the 1-based index j = left + k and the raw weight  a * cubic(a * (u - j))
 *   cubic = Keys' kernel with A = -0.5:   1.5|x|^3 - 2.5|x|^2 + 1  for |x| <= 1,   -0.5|x|^3 + 2.5|x|^2 - 4|x| + 2  for 1 < |x| <= 2,
 *   0 otherwise.  The weights are divided by their sum.  The tap reads in[mirror(j - 1)]; mirror is the symmetric reflection of period 2n
 *   that repeats the edge sample, applied as often as needed:   q = (j - 1) mod 2n,   q < n ? q : 2n - 1 - q.
 * The image is resized along H first, then along W; both passes in fp32, taps accumulated in ascending order.  No clamp unless `clamp`.
 * This is imresize_np(..., antialiasing=True): its removal of zero-weight columns changes no value, its single reflection is the case
 * P <= n.  (rs_bicubic / F.interpolate differ: A = -0.75 and clamped borders; F.interpolate(antialias=True) clamps and renormalises at
 * the borders where this definition mirrors.)
 * Coordinates are part of the definition: u and left in fp64 from the integer output index, the distance u - j formed in fp64 and
 * rounded to fp32 once; weights and sums are fp32.  A pixel's value is a function of its plane and its output index only - not of the
 * tile, the batch, the grid or the pointer alignment; no floating-point atomics.  tests/_resize_ref.py restates this in float64.
 * `clamp` = 1 clamps the result to [-1, 1] (the samplers), 0 leaves it as computed.  The caller chooses Ho, Wo and the scales:
 * imresize's rules are Ho = ceil(H s) for a given scale, s_h = Ho / H and s_w = Wo / W for a given size.
 * Argument errors are found before anything is launched, -2 with rs_last_error() starting "rs_resize: ": a null pointer, a
 * non-positive size, a scale outside [1/8, 8] (1/8 bounds P at 34), an `out` that is or overlaps `in`, a clamp other than 0 or 1. */
int rs_resize(const float* in, float* out, int B, int C, int H, int W, int Ho, int Wo, double scale_h, double scale_w, int clamp,
              void* stream);

/* ---- image metrics: PSNR and SSIM against ground truth -------------------------------------------------
 * The scores of the restoration literature, as the reference's utils/util_image.py calculate_psnr / calculate_ssim compute them on
 * uint8 images, for a whole batch in two launches.  Stateless.
 *   a, b  two batches of one shape; each is either uint8 [B,H,W,C] (x_is_float = 0) or fp32 [B,C,H,W] in [-1,1] (x_is_float = 1), which
 *         is first quantised exactly as rs_output_to_u8 quantises it (x*0.5+0.5, clamp, *255, round half to even - one device function).
 *   C is 1 or 3.  ycbcr = 1 (C == 3 only): both images are replaced by MATLAB's rounded luma
 *         Y = 16 + round((65481 r + 128553 g + 24966 b) / 255000)     in exact integer arithmetic, ties to even.
 *         (Deviation: the reference evaluates 16 + (65.481 r + 128.553 g + 24.966 b) / 255 in float64 and rounds; at the 194 RGB triples
 *         whose exact value is a tie, float64 noise - the order of the dot product - decides, and numpy's own paths disagree with each
 *         other there.  The integer form differs from every float64 form only at those triples.)
 *   `border` pixels are cropped from every side; the cropped height and width must be >= 11.
 *   PSNR: sse_out[i] = the sum over the cropped pixels and channels of (a - b)^2, an exact 64-bit integer; the caller forms
 *         psnr = 20 log10(255 / sqrt(sse / n)), n = channels * cropped height * cropped width, inf at sse == 0.
 *   SSIM: per channel, with the 11-tap window g[i] = exp(-(i - 5)^2 / 4.5) / sum (sigma = 1.5, fp64), applied along rows and columns
 *         ("valid": no padding) to a, b, a^2, b^2, ab:   mu1, mu2, s1 = E[a^2] - mu1^2, s2 = E[b^2] - mu2^2, s12 = E[ab] - mu1 mu2,
 *         map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),   C1 = 6.5025, C2 = 58.5225;
 *         ssim_out[i] = the mean of the map over its (H' - 10)(W' - 10) positions, then the mean over the channels.  All of it in fp64.
 * sse_out [B] int64 and ssim_out [B] fp64 are device memory.  No floating-point atomics: every sum has an order fixed by the image's
 * shape, so image i's results are the same bits run to run and whatever else the batch holds.  Identical images give sse 0 and ssim 1.0
 * exactly.  tests/_metrics_ref.py restates the definition in numpy.
 * `work`: device scratch of rs_metrics_work_bytes(...) bytes (0 for a geometry rs_metrics refuses), 8-byte aligned.  Argument errors
 * are found before anything is launched, -2 with rs_last_error() starting "rs_metrics: ": a null pointer, a flag other than 0 or 1, a
 * non-positive size, C other than 1 or 3, ycbcr without C == 3, a negative border, a cropped image below 11 x 11 (both sizes are
 * named), a workspace that is too small or misaligned.
 * rs_rgb_to_y_u8: the same Y as an op of its own, interleaved uint8 [pixels,3] -> uint8 [pixels]. */
size_t rs_metrics_work_bytes(int B, int C, int H, int W, int border, int ycbcr);
int rs_metrics(const void* a, const void* b, int a_is_float, int b_is_float, int B, int C, int H, int W, int border, int ycbcr,
               long long* sse_out, double* ssim_out, void* work, size_t work_bytes, void* stream);
int rs_rgb_to_y_u8(const uint8_t* rgb_hwc, uint8_t* y, size_t pixels, void* stream);

/* ---- degradation: LQ test sets from ground truth ----------------------------------------------------------
 * The operators of the reference's Real-ESRGAN degradation (basicsr/data/realesrgan_dataset.py:240-363 degrade_fun), with which the LQ
 * inputs of the `realsr` configurations are made from ground-truth images; resshift_amd/degrade.py draws a plan and runs them in the
 * recipe's order.  Stateless.  Tensors are fp32 NCHW, contiguous, with values nominally in [0, 1]; inputs are only read.  Every output
 * value is a function of its image and its own index alone, every sum has a fixed order, nothing is atomic: a batch is bit for bit its
 * B = 1 calls.  tests/_degrade_ref.py restates all of it in float64.  Argument errors are found before anything is launched, -2 with
 * rs_last_error() starting "rs_<name>: ".
 *
 * rs_filter2d: basicsr/utils/img_process_util.py filter2D.  A CROSS-CORRELATION - the kernel is not flipped:
 *       out[b,c,i,j] = sum_{u,v} kernels[kb,u,v] * in[b,c,refl(i + u - k/2, H),refl(j + v - k/2, W)],   taps in row-major ascending order,
 *   refl = torch's `reflect`, which does not repeat the edge sample:  refl(q, n) = |q| for q < n, 2 (n - 1) - q otherwise.
 *   kernels [Bk,k,k] fp32 device; Bk = 1 (one kernel for the batch, kb = 0) or B (one per image, for all its channels, kb = b).  k odd,
 *   k <= 21, k / 2 < min(H, W).  clamp = 1 clamps the result to [0, 1].  One launch, no padded copy; not in place.
 * rs_interp: F.interpolate(x, mode = "area" (RS_INTERP_AREA) | "bilinear" | "bicubic", align_corners=False), NO antialiasing - the resize the
 *   degradation uses.  (rs_resize is another function: MATLAB's antialiased kernel, A = -0.5, mirrored borders.)
 *   scale_h = scale_w = 0: a size (Ho, Wo) was given and source coordinates step by H / Ho;  scale_h, scale_w > 0: a scale factor was given,
 *   Ho = floor(H * scale_h) (likewise Wo) is required and source coordinates step by 1 / scale, as torch has it.  Either way the scales
 *   (Ho / H resp. scale_h) must lie in [1/8, 8].   src(i) = step * (i + 0.5) - 0.5  in fp64; the fraction src - floor(src) is rounded to
 *   fp32 once; weights and sums are fp32.
 *     bicubic:  taps floor(src) - 1 .. floor(src) + 2, indices clamped to the image, Keys' cubic with A = -0.75, rows of four then the column.
 *     bilinear: src below 0 is 0; taps floor(src) and floor(src) + 1 (clamped), weights 1 - t and t.
 *     area:     adaptive average pooling, the mean over the integer window [floor(i H / Ho), ceil((i + 1) H / Ho)) x (likewise for W).
 *   clamp = 1 clamps the result to [0, 1].  Not in place.
 * rs_jpeg: basicsr/utils/diffjpeg.py DiffJPEG(differentiable=False); C = 3; quality [B] is a HOST array (by value to the kernel, B <=
 *   RS_MAX_ROWS), each in (0, 100) exclusive: factor = (q < 50 ? 5000 / q : 200 - 2 q) / 100 in fp32, 0 at q = 100, where the reference
 *   divides by it.  Per 16 x 16 MCU - H and W are padded on the right / bottom with zeros in RGB, inside the kernel, and cropped on the
 *   store - forward: x 255; Y = .299 R + .587 G + .114 B, Cb = -.168736 R - .331264 G + .5 B + 128, Cr = .5 R - .418688 G - .081312 B +
 *   128; chroma 2 x 2 mean; - 128; the 8 x 8 DCT  F[u,v] = s[u,v] sum_{x,y} f[x,y] cos((2x+1) u pi/16) cos((2y+1) v pi/16),  s = 1/4
 *   a[u] a[v], a[0] = 1/sqrt 2, as a row pass and a column pass, of the four Y blocks and the two chroma blocks; q = rint(F / (table *
 *   factor)) - an fp32 product, a true division, ties to even - with the luminance resp. chrominance table of the JPEG standard's Annex
 *   K.  Inverse: q * (table * factor); f = 1/4 sum a[u] a[v] F[u,v] cos.. + 128; chroma by pixel repetition; R = Y + 1.402 Cr', G = Y -
 *   .344136 Cb' - .714136 Cr', B = Y + 1.772 Cb' (Cb' = Cb - 128, Cr' = Cr - 128); clamp to [0, 255]; / 255.  The INPUT is not clamped:
 *   that is the caller's, as in the reference.  All constants are the float32 roundings of the reference's double values.  One launch,
 *   coefficients never leave LDS / registers; `out` may be `in`.
 * rs_add_noise: out = x + (sigma[b] / 255) n, clamped to [0, 1] when clamp = 1 (basicsr/data/degradations.py add_gaussian_noise_pt).  n =
 *   the normals rs_noise_fill writes for (keys[b], draw[b]) and per_image_count C*H*W, element by element - or, where gray[b] = 1, those for
 *   H*W, shared by the image's channels.  keys, draw, sigma, gray are HOST arrays [B], B <= RS_MAX_ROWS.  In fp32: x + c * n with c =
 *   (float)(sigma / 255), the product and the sum rounded separately, as the reference's tensor operations round them.  `out` may be `x`.
 * rs_unit_to_u8: planar fp32 [B,C,H,W] in [0,1] -> interleaved uint8 [B,H,W,C] = clamp(rint(x * 255), 0, 255), ties to even: the recipe's last
 *   line, and what becomes the PNG. */
#define RS_INTERP_AREA 0
#define RS_INTERP_BILINEAR 1
#define RS_INTERP_BICUBIC 2
int rs_filter2d(const float* in, const float* kernels, float* out, int B, int C, int H, int W, int k, int Bk, int clamp, void* stream);
int rs_interp(const float* in, float* out, int B, int C, int H, int W, int Ho, int Wo, double scale_h, double scale_w, int mode, int clamp,
              void* stream);
int rs_jpeg(const float* in, float* out, const float* quality, int B, int C, int H, int W, void* stream);
int rs_add_noise(const float* x, float* out, const rs_noise_key* keys, const int* draw, const float* sigma, const int* gray, int B, int C, int H,
                 int W, int clamp, void* stream);
int rs_unit_to_u8(const float* src_f32_nchw, void* dst_u8_nhwc, int B, int C, int H, int W, void* stream);

/* ---- face degradation: a real JPEG codec and a 41-tap blur under a resize -------------------------------------------
 * The two operators the reference's face recipe (datapipe/face_degradation_testing.py face_degradation) needs beyond the ones above;
 * resshift_amd/degrade.py FacePlan / Degrader.run_face runs it.  Same conventions: stateless, fp32 NCHW contiguous, inputs only read,
 * one launch, a batch is bit for bit its B = 1 calls, argument errors -2 with rs_last_error() starting "rs_<name>: " before any launch.
 *
 * rs_jpeg_codec: libjpeg's baseline JPEG round trip at 4:2:0 - what cv2.imencode('.jpg', .., [IMWRITE_JPEG_QUALITY, q]) + imdecode and
 *   PIL save(quality=q, subsampling=2) + open compute; the (lossless) entropy stage is never materialised.  C = 3 in RGB order; H, W >= 8;
 *   quality [B] is a HOST array of integers 1 .. 100 (by value to the kernel, B <= RS_MAX_ROWS).  Not in place.
 *   In:  u = (int) rintf(fminf(fmaxf(x, 0), 1) * 255.f);   out: (float) v / 255.f, a true fp32 division.  Everything between is 32-bit
 *   integer arithmetic (>> arithmetic, FIX16(c) = (int)(c 65536 + .5), DESCALE(x, n) = (x + (1 << (n - 1))) >> n), so the result does not
 *   depend on the mapping, the batch or the position in it.  tests/_jpeg_ref.py is this definition in numpy, equal to Pillow's libjpeg-turbo
 *   on every byte.
 *   Forward: Y = (FIX16(.299) R + FIX16(.587) G + FIX16(.114) B + 32768) >> 16;  Cb = (-FIX16(.16874) R - FIX16(.33126) G + FIX16(.5) B +
 *   (128 << 16) + 32767) >> 16;  Cr = (FIX16(.5) R - FIX16(.41869) G - FIX16(.08131) B + (128 << 16) + 32767) >> 16.  Edges: pixels are
 *   replicated on the right at full resolution up to a multiple of 16, at the bottom at full resolution up to an EVEN row count only;
 *   chroma is down-sampled 2 x 2 as (a + b + c + d + bias) >> 2 with bias 1 on even output columns and 2 on odd ones; then the down-sampled
 *   chroma rows and the Y rows are replicated up to the MCU multiple.  - 128; jfdctint.c's "islow" DCT (rows, then columns; CONST_BITS 13,
 *   PASS1_BITS 2; output x 8) on every 8 x 8 block; q = sign(c) ((|c| + (d >> 1)) / d) with d = 8 t[u,v];  t = clamp((base s + 50) / 100,
 *   1, 255), s = q < 50 ? 5000 / q : 200 - 2 q in integer divisions, base = Annex K's luminance / chrominance table in natural order.
 *   Inverse: q t; jidctint.c's "islow" IDCT (columns with DESCALE 11, then rows with DESCALE 18); + 128; clamp to 0 .. 255.  Chroma
 *   "fancy" (triangle) up-sampling over the REAL ceil(H/2) x ceil(W/2) samples: vertically s = 3 near + far (far = the row above for the
 *   upper output row, below for the lower; the first / last real row stand in for a missing one), horizontally even = (3 s[j] + s[j-1] +
 *   8) >> 4, odd = (3 s[j] + s[j+1] + 7) >> 4 (the first / last real column stand in likewise).  R = Y + ((FIX16(1.402) cr + 32768) >>
 *   16), B = Y + ((FIX16(1.772) cb + 32768) >> 16), G = Y + ((-FIX16(.34414) cb - FIX16(.71414) cr + 32768) >> 16) with cb, cr = chroma -
 *   128; clamp to 0 .. 255.
 * rs_blur_resize: out = bilinear(filter2D(in, kernels), size = (Ho, Wo)), the filter evaluated only at the samples the resize reads; no
 *   blurred tensor exists.  filter2D is rs_filter2d's function (same taps, same order) with k odd, k <= 41, k / 2 < min(H, W), Bk = 1 or
 *   B; bilinear is rs_interp's size-given rule (steps H / Ho, W / Wo) with the scales Ho / H, Wo / W in [1/64, 64].  kernels == NULL (then
 *   k must be 0): the resize alone.  At Ho = H, Wo = W the result is rs_filter2d's, bit for bit.  clamp = 1 clamps the result to [0, 1].
 *   Not in place. */
int rs_jpeg_codec(const float* in, float* out, const int* quality, int B, int C, int H, int W, void* stream);
int rs_blur_resize(const float* in, const float* kernels, float* out, int B, int C, int H, int W, int Ho, int Wo, int k, int Bk, int clamp,
                   void* stream);

/* ---- JPEG files: libjpeg's baseline encoder on the device -------------------------------------------------------------
 * rs_jpeg_encode: uint8 RGB images -> finished baseline JPEG FILES in device memory, byte for byte what libjpeg writes for them at 4:2:0 with
 *   its default tables - PIL.Image.save(format="JPEG", quality=q, subsampling=2) - so that only compressed bytes cross PCIe.  The forward
 *   path is rs_jpeg_codec's above (one definition, csrc/jpeg_common.h), from the 8-bit pixels on; this call adds the entropy stage the codec
 *   never materialises.  tests/_jpeg_enc_ref.py is the definition in numpy, equal to Pillow's libjpeg-turbo on every byte.  Same conventions
 *   as the block above: stateless, inputs only read, a batch is byte for byte its B = 1 calls, argument errors -2 with rs_last_error()
 *   starting "rs_jpeg_encode: " before any launch.  Several launches on `stream`; no kernel waits for another workgroup.
 *   in: uint8 [B,H,W,3] on the device (what rs_output_to_u8 / rs_unit_to_u8 write); C must be 3; 8 <= H, W <= 65535 and at most about 55
 *   megapixels (the two-level prefix sum of the stuffing pass); every image of a call has the same size and its own quality, a HOST array of
 *   integers 1 .. 100 (by value to the kernels, B <= RS_MAX_ROWS).  out: B rows of out_pitch >= rs_jpeg_encode_bound(H, W) bytes on the
 *   device; image b's file is out[b * out_pitch .. + nbytes[b]) and NO byte at or beyond nbytes[b] of a row is written.  nbytes: int [B] on
 *   the device.  workspace: rs_jpeg_encode_workspace(B, H, W) bytes on the device, 16-byte aligned, contents irrelevant before and after.
 *   in, out, nbytes and workspace must not overlap.
 *   Blocks.  Quantised coefficients in zigzag order, in scan order: per MCU (16 x 16 pixels) Y00, Y01, Y10, Y11, Cb, Cr, MCUs row-major.
 *   libjpeg transforms only ceil(H/8) x ceil(W/8) Y blocks; an MCU's Y positions beyond them are DUMMY blocks (jccoefct.c compress_data): all
 *   63 AC coefficients zero, the DC that of the preceding block of the MCU, which may be a dummy itself.  Chroma is never a dummy.
 *   Codes.  Per block the DC difference against the previous block of the same component in scan order (0 before the first; dummies take part),
 *   as its magnitude category n (Annex K.3 DC table of the component) and n extra bits; then run / category symbols (Annex K.3 AC table)
 *   with n extra bits, ZRL (0xF0) for every 16 zeros of a longer run, EOB (0x00) unless coefficient 63 is non-zero.  Extra bits of v < 0 are
 *   v + 2^n - 1.  Bits fill bytes MSB first; the last byte is padded with 1-bits; every 0xFF byte of the scan is followed by 0x00.
 *   File.  SOI, APP0 (JFIF 1.01, units 0, density 1 x 1), DQT luminance, DQT chrominance (8-bit, zigzag order), SOF0 (8-bit, H, W, components
 *   1 / 2 / 3 sampled 0x22 / 0x11 / 0x11 with tables 0 / 1 / 1), DHT DC0, AC0, DC1, AC1, SOS (one interleaved scan), the scan from offset 623,
 *   EOI.  Only the DQT payloads depend on the quality, only SOF0 on the size.
 *   Bound.  The longest code of a block: the longest DC code with its extra bits (chrominance category 11: 11 + 11 bits) and 63 coefficients
 *   of the longest AC code with its extra bits (16 + 10, so no EOB): 22 + 63 * 26 = 1660 bits, derived from the code tables at compile time.
 *   rs_jpeg_encode_bound(H, W) = 623 + 2 * ceil(6 * ceil(H/16) * ceil(W/16) * 1660 / 8) + 2: every byte of the scan stuffed, plus EOI.  The
 *   coder clamps categories to 11 (DC) and 10 (AC) - beyond what 8-bit samples reach - so no input overruns it.  Both size queries return 0
 *   for sizes rs_jpeg_encode refuses. */
size_t rs_jpeg_encode_bound(int H, int W);
size_t rs_jpeg_encode_workspace(int B, int H, int W);
int rs_jpeg_encode(const void* in_u8_nhwc, void* out, int* nbytes, const int* quality, void* workspace, int B, int C, int H, int W,
                   size_t out_pitch, void* stream);

/* uint8 pre / post processing on the device.
 * rs_u8_to_input:  interleaved uint8 [B,H,W,C] -> planar fp32 [B,C,H,W] in [-1,1]  ((v/255 - 0.5)/0.5; replaces
 *                  datapipe/datasets.py:59-63 ToTensor + Normalize on the host)
 * rs_output_to_u8: planar fp32 [-1,1] -> interleaved uint8: x*0.5+0.5, optional inpainting blend with the LQ input
 *                  sr*m + lq*(1-m) (sampler.py:218-222; lq and mask both null or both set, mask is [B,1,H,W] in [-1,1]),
 *                  clamp, *255, round-half-even, RGB->BGR when `bgr` (utils/util_image.py:245-269 tensor2img) */
int rs_u8_to_input(const void* src_u8_nhwc, float* dst_f32_nchw, int B, int H, int W, int C, void* stream);
int rs_output_to_u8(const float* sr_f32_nchw, const float* lq_f32_nchw, const float* mask_f32_n1hw, void* dst_u8_nhwc, int B, int H,
                    int W, int C, int bgr, void* stream);

/* ---- introspection --------------------------------------------------------------------------- */
/* bytes of scratch arena currently allocated; number of kernel launches issued by the last call (the network's own: a debug
 * trace's capture copies are not counted) */
size_t rs_arena_bytes(rs_engine* e);
long long rs_last_launch_count(rs_engine* e);
/* profiling of the MFMA implicit-GEMM kernel family: when enabled every igemm launch of the next call is
 * bracketed by hipEvents on the launch stream.  rs_profile_get fills out[9] = {fp16-input igemm FLOPs,
 * fp32-input igemm FLOPs, summed igemm kernel milliseconds, igemm launch count, algorithmic HBM bytes (every
 * operand and result counted once), split-input igemm FLOPs, GroupNorm kernel milliseconds, GroupNorm count, GroupNorm
 * algorithmic bytes (input read once + output written once)} of the last call (counts are always maintained; the time is 0 unless
 * profiling was on).  The cost of an empty event pair, measured on the same stream, is subtracted from every
 * bracket so that the sum is the kernels' own duration. */
int rs_profile_enable(rs_engine* e, int on);
int rs_profile_get(rs_engine* e, double* out9);
/* the same per kernel family of the MFMA path, in this order: halo conv fp16 (igemm4), halo conv split storage, implicit GEMM fp16
 * (igemm2 / igemm3 / igemm), implicit GEMM split storage, implicit GEMM fp32 (exact), fused qkv + window attention + projection,
 * fused Swin MLP, and the split-storage variants of those two.  out[3 f + 0] = algorithmic FLOPs, [3 f + 1] = kernel milliseconds,
 * [3 f + 2] = launches; returns the number of families (9) or -1 when cap < 27. */
int rs_profile_families(rs_engine* e, double* out, int cap);
/* debug trace (tests only): while enabled, every network call records named intermediate activations.  A record copies
 * the tensor, on the call's stream at the point where it is produced, into a capture region of the trace (dense fp32 NCHW); the traced
 * call runs the same kernels with the same parameters and scratch layout as an untraced one, and a fused path has no record for a tensor
 * it never stores.  The capture region is allocated while tracing is on only (rs_debug_enable(e, 0) frees it), apart from the scratch
 * arena.  UNet names: in.0, in.N, in.N.res (blocks with Swin), mid.res1, mid.swin, mid.res2, out.J, out.J.res (blocks with Swin or
 * upsampling), out.J.swin (Swin followed by upsampling); inner records (conv1, embed, blkK.qkv / attn / proj / out) carry their block's
 * name as prefix: in.N.res.conv1, mid.swin.embed, out.J.swin.blk1.out ...  rs_debug_count = records of the last call (= its capture
 * copies); rs_last_launch_count counts the network's launches only, never the capture copies.  fetch copies record i into caller memory
 * (B*C*H*W floats, stream-ordered after the call); fetch_rows copies images b0 .. b0 + nb - 1 of it only (nb*C*H*W floats), so that a
 * caller that looks at a few images of a large batch never holds a whole record.  Autoencoder names (rs_vq_encode / rs_vq_decode): enc.in,
 * enc.down.L.block.I, enc.down.L.ds, enc.mid.block_1, enc.mid.attn, enc.mid.block_2, enc.out (conv_out; the quant_conv is the call's
 * output); dec.zq (not with force_not_quantize), dec.pq, dec.in, dec.mid.block_1, dec.mid.attn, dec.mid.block_2, dec.up.L.block.I,
 * dec.up.L.us (the image is the call's output); inner records: <block>.conv1, <attn>.norm / q / k / o, dec.zq.z. */
/* text table of the last profiled call: per (part, kernel family, M, N, K) launch shape of the MFMA family - launches, summed kernel ms
 * (hipEvents on the launch stream), algorithmic flops - and the wall ms of the encoder / UNet / decoder parts (measurement, d of SURVEY 8:
 * where a pass's time goes per reference module - ldm/modules/diffusionmodules/model.py Encoder / Decoder, models/unet.py UNetModelSwin).
 * Returns the bytes needed incl. the terminating 0; copies at most cap. */
int rs_profile_shapes(rs_engine* e, char* buf, int cap);
int rs_debug_enable(rs_engine* e, int on);
int rs_debug_count(rs_engine* e);
int rs_debug_info(rs_engine* e, int i, char* name, int name_cap, int* dims_bchw);
int rs_debug_fetch(rs_engine* e, int i, float* out_nchw_dev, void* stream);
int rs_debug_fetch_rows(rs_engine* e, int i, int b0, int nb, float* out_nchw_dev, void* stream);

/* ---- op-level entry points (used by tests/ to check each kernel against torch on its own) ---- */
/* NHWC conv / linear through the MFMA implicit GEMM or the direct kernels (auto-selected).
 * x0 [B,Hs,Ws,C0] (+ optional x1 [B,Hs,Ws,C1] concatenated on C), w_ref in the reference layout
 * [Cout][C0+C1][KH][KW] fp32 on the HOST (packed internally), bias fp32 host or NULL, res/out NHWC. */
int rs_op_conv2d(const void* x0, const void* x1, const float* w_ref_host, const float* bias_host, const void* res, void* y,
                 int B, int Hs, int Ws, int C0, int C1, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho,
                 int Wo, int up, int act, int in_prec, int out_prec, int force_direct, void* stream);
/* rs_op_conv2d on views into wider buffers: ld0 / ld1 / ldy / ldres are the row strides, in elements, of x0 / x1 / y / res (the pixel record
 * of split storage is [ld hi | ld lo]).  plan_out (may be NULL) receives the plan the launch EXECUTED - kernel (ConvKernel of csrc/common.h),
 * pixel tile, channel tile, small-plane segment, split-K factor, pixels per statistics slab - or six zeros when a direct kernel took it. */
int rs_op_conv2d_ex(const void* x0, const void* x1, const float* w_ref_host, const float* bias_host, const void* res, void* y,
                    int B, int Hs, int Ws, int C0, int C1, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho,
                    int Wo, int up, int act, int in_prec, int out_prec, int force_direct, int ld0, int ld1, int ldy, int ldres,
                    int plan_out[6], void* stream);
/* the plan rs_op_conv2d_ex would execute for this layer (has_res: a residual is added; nz: batched-GEMM count, 1 for a conv).  Host only:
 * touches no device.  out[6] as plan_out above; returns the planner's return code (0, or -2: no kernel takes the launch). */
int rs_op_conv_plan(int B, int Hs, int Ws, int C0, int C1, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo,
                    int up, int act, int in_prec, int out_prec, int ld0, int ld1, int ldy, int ldres, int has_res, int nz, int out[6]);
/* timing probe for one implicit-GEMM conv shape: device-resident NHWC input, weights already packed [Cout][KH*KW*Cin]
 * in the input precision; runs `reps` launches between two hipEvents and returns the average ms per launch. */
int rs_op_conv2d_bench(const void* x0, const void* w_packed_dev, const float* bias_dev, const void* res, void* y, int B, int Hs,
                       int Ws, int Cin, int Cout, int KH, int KW, int stride, int pad, int Ho, int Wo, int up, int act, int in_prec,
                       int out_prec, int reps, float* ms_out, void* stream);
/* halo-tile 3x3 conv with the GroupNorm affine + activation of its input fused in (igemm4.hip): y = conv3x3(act_in(x * coef[b][0][c]
 * + coef[b][1][c])) (+res); x / res / y NHWC device tensors in `prec` storage (RS_PREC_F16 or RS_PREC_SPLIT), coef_dev [B][2][Cin]
 * fp32 device (null: plain conv), act_in 0 / 2 (none / SiLU), weights [Cout][Cin][3][3] fp32 host.  `ystats_dev` (may be null):
 * [B][H*W / rs_op_conv3x3_halo_stats_px(...)][Cout][2] fp32 device, receives the per-(image, 256-pixel slab, channel) sum / sum of squares of the stored
 * output (the GroupNorm statistics the kernel - or, for its split-K launches on the 16x16 / 8x8 planes, the reduce kernel - leaves
 * for the consuming GroupNorm).  Returns an error when the shape is not eligible for that kernel. */
int rs_op_conv3x3_halo(const void* x, const float* coef_dev, int act_in, const float* w_ref_host, const float* bias_host, const void* res,
                       void* y, int B, int H, int W, int Cin, int Cout, int prec, float* ystats_dev, void* stream);
/* the same layer on the Winograd F(2x2,3x3) kernel (wino.hip; RS_PREC_SPLIT tensors only): U = G g G^T packed on the host, one checked launch;
 * reps > 0: `reps` more launches between two hipEvents, *ms_out = average ms per launch.  ystats_dev (may be null): [B][H*W / 128][Cout][2]
 * (one slab per 8 x 16 pixel tile).  Replaces the reference's nn.Conv2d(3x3, padding 1) behind GroupNorm + SiLU (models/unet.py:128-147,186-206; ldm/modules/diffusionmodules/
 * model.py:100-149).  Returns an error when the shape is not eligible (Cin % 32, Cout % 64, planes that tile by 8 x 16, Cin <= 640). */
int rs_op_conv3x3_wino(const void* x, const float* coef_dev, int act_in, const float* w_ref_host, const float* bias_host, const void* res,
                       void* y, int B, int H, int W, int Cin, int Cout, float* ystats_dev, int reps, float* ms_out, void* stream);
/* pixels per statistics slab rs_op_conv3x3_halo uses for this shape (0: shape not eligible / no statistics): ystats_dev is
 * [B][H*W / slab][Cout][2] (256- or 128-pixel tiles of the kernel variant, or the reduce kernel's slabs for its split-K launches) */
int rs_op_conv3x3_halo_stats_px(int B, int H, int W, int Cin, int Cout, int prec);
/* batched NT GEMM: y[z][m][n] = scale * sum_k a[z][m][k] * b[z][n][k]  (+bias[n]) */
int rs_op_gemm_nt(const void* a, const void* b, const float* bias_dev, void* y, int nz, int M, int N, int K, float scale,
                  int in_prec, int out_prec, void* stream);
int rs_op_groupnorm(const void* x, void* y, const float* gamma_host, const float* beta_host, const float* film_dev, int B, int HW,
                    int C, int groups, float eps, int act, int prec, void* stream);
int rs_op_window_attention(const void* qkv, void* out, const float* bias_table_host /*[225][heads]*/, int B, int H, int W,
                           int heads, int shift, int prec, void* stream);
/* fused qkv projection + window attention (fp16, 6 heads of 32): x [B,H,W,192] normalised tokens, wqkv [576][192] fp16 device,
 * bqkv [576] fp32 device, table as in rs_op_window_attention (host); out [B,H,W,192].  With wproj_dev ([192][192] fp16) and
 * bproj_dev the output projection is fused as well and `res` (fp16 [B,H,W,192], may be null) is added: out = res + proj(attn) */
int rs_op_window_attention_qkv(const void* x, const void* wqkv_dev, const float* bqkv_dev, const void* wproj_dev, const float* bproj_dev,
                               const void* res, void* out, const float* table_host, int B, int H, int W, int heads, int shift, void* stream);
/* the same on split storage (RS_PREC_SPLIT): x / res / out are (hi, lo) pair tensors, wqkv_dev [576][192 hi | 192 lo] and wproj_dev
 * [192][192 hi | 192 lo] fp16 on the device; `xcoef_dev` (may be null) is a GroupNorm affine [B][2][192] applied to x on the fly
 * (models/swin_transformer.py:85-145,238-277 in one launch, win_attn_split.hip) */
int rs_op_window_attention_qkv_split(const void* x, const void* wqkv_dev, const float* bqkv_dev, const void* wproj_dev, const float* bproj_dev,
                                     const void* res, void* out, const float* table_host, const float* xcoef_dev, int B, int H, int W, int heads,
                                     int shift, void* stream);
/* streaming attention of the autoencoder's AttnBlock (ldm/modules/diffusionmodules/model.py:179-203), fp16 device tensors: q, k
 * [nz][T][C], vt [nz][C][T] (v transposed, without its bias), bv_dev [C] fp32 (v bias, may be null), o [nz][T][C] =
 * softmax(q k^T / sqrt(C)) v + bv; C in {128, 256, 512}, T a multiple of 128 (ae_attn.hip) */
int rs_op_ae_flash_attention(const void* q, const void* k, const void* vt, const float* bv_dev, void* o, int nz, int T, int C, void* stream);
/* the same on split storage (RS_PREC_SPLIT tensors of (hi, lo) fp16 pairs: q, k, o records [C hi | C lo] per token, vt rows [T hi | T lo] per
 * channel); C = 512, T a multiple of 64 (ae_attn_split.hip; the reference's memory-efficient AttnBlock is model.py:205-268) */
int rs_op_ae_flash_attention_split(const void* q, const void* k, const void* vt, const float* bv_dev, void* o, int nz, int T, int C, void* stream);
/* fused Swin MLP, fp16 device tensors: y[M][E] = res + fc2(GELU(fc1(x))) with fc1 weights [HD][E], fc2 weights [E][HD]
 * (row-major fp16, device), fp32 biases; res may be null (models/swin_transformer.py:17-33,279) */
int rs_op_swin_mlp(const void* x, const void* w1_dev, const float* b1_dev, const void* w2_dev, const float* b2_dev, const void* res, void* y,
                   int M, int E, int HD, void* stream);
/* the same on split storage (RS_PREC_SPLIT tensors of (hi, lo) fp16 pairs): weights packed [rows][K hi | K lo] fp16 on the device */
int rs_op_swin_mlp_split(const void* x, const void* w1_dev, const float* b1_dev, const void* w2_dev, const float* b2_dev, const void* res, void* y,
                         int M, int E, int HD, void* stream);
/* the last Swin block of a BasicLayer + its patch_unembed (models/swin_transformer.py:279,515,521-528) in one launch, split storage:
 * y[M][NO] = Wu (x + fc2(GELU(fc1(x a + d))) + b2) + bu with the GroupNorm affine (a, d) = xcoef_dev [M / HW][2][E]; w2cat_dev = the product
 * matrix [NO][HD + E] = [Wu W2 | Wu] packed [rows][K hi | K lo], bcat_dev = Wu b2 + bu; E = 192, HD = 768, NO = 160, HW % 128 == 0 */
int rs_op_swin_mlp_split_unembed(const void* x, const float* xcoef_dev, const void* w1_dev, const float* b1_dev, const void* w2cat_dev, const float* bcat_dev,
                                 void* y, int M, int HW, int E, int HD, int NO, void* stream);
int rs_op_softmax_rows(const float* s, void* out, long long nrows, int ncols, int out_prec, void* stream);
int rs_op_vq(const float* z, const float* codebook_dev, float* zq, int32_t* idx, long long N, int NE, int D, void* stream);
int rs_op_nchw_to_nhwc(const float* in, void* out, int B, int C, int HW, int out_prec, void* stream);
int rs_op_nhwc_to_nchw(const void* in, float* out, int B, int C, int HW, int in_prec, void* stream);
/* storage conversion of an NHWC tensor [npix][C] between any two of RS_PREC_F16 / RS_PREC_F32 / RS_PREC_SPLIT (tests feed and
 * read split-storage tensors through it) */
int rs_op_convert(const void* src, int src_prec, void* dst, int dst_prec, int C, long long npix, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RESSHIFT_HIP_H */
