/*
 * ssr_hip.h — C ABI of libssr_hip.so: the MI355X (gfx950) kernels under the ESRGAN hot path of
 * allenai/satlas-super-resolution.
 *
 * The reference has no native layer: its "kernels" are the ATen/cuDNN ops that its Python issues
 * (SURVEY.md §2.3).  Each entry point below names the reference call site(s) (file:line, relative
 * to /root/reference) whose device work it replaces.  All entry points
 *   - take raw device pointers, sizes and a hipStream_t (as void*); no torch types;
 *   - never allocate, never synchronise, are hipGraph-capturable;
 *   - return 0 on success, a negative SSR_E* code on a bad descriptor, or the positive hipError_t
 *     of a failed launch.
 *
 * Data layout: activations are NHWC ("pixel-major"), element type fp32 (SSR_F32) or bf16
 * (SSR_BF16); a tensor is described by (base pointer, channel stride `cs` = channels of the
 * underlying buffer, channel offset `coff`), so a conv can read/write a channel slice of a wider
 * buffer — this is how the dense blocks run without torch.cat (rrdbnet_arch.py:39-42).
 * Channel strides/offsets are multiples of 8 elements.  Master weights are fp32 OIHW exactly as in
 * the reference's state_dict; kernels consume packed copies produced by ssr_pack_weights.
 */
#ifndef SSR_HIP_H
#define SSR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSR_F32 0
#define SSR_BF16 1
/* fp32 tensors in HBM, bf16 matrix cores on split operands (hi + lo, three MFMAs per product, fp32 accumulation): the
 * arithmetic mode that meets the 1e-3 parity gate at matrix-core speed.  Storage, packing and every non-MFMA entry point
 * treat it exactly as SSR_F32. */
#define SSR_F32X3 2
/* FORWARD convolutions only (ssr_conv2d, ssr_conv2d_batch; the forward table of ssr_pack_weights), round 6: fp32 tensors in HBM,
 * fp16 matrix cores on split operands - an activation is staged as hi = f16(x), lo = f16(x - hi); the packed weights hold
 * hi = f16(2^SSR_F32H_WSHIFT w), lo = f16(2^SSR_F32H_WSHIFT w - hi) in the SSR_F32X3 row layout ([16 hi | 16 lo], 64 bytes); a product
 * is a_lo w_hi + a_hi w_lo + a_hi w_hi (three v_mfma_f32_32x32x16_f16, fp32 accumulation) and the accumulators are multiplied by
 * 2^-SSR_F32H_WSHIFT before the epilogue.  Two 11-bit pieces carry 22 bits of an operand (bf16 pieces: 16), so a pre-activation is
 * as close to the fp32 value as another fp32 summation order is, and its LeakyReLU decision is an fp32 evaluation's - at the split-bf16
 * mode's speed.  The weight shift keeps the lo pieces of ordinary convolution weights (|w| down to 2^-17 x 2^-SHIFT) in fp16's
 * normal range; activations are staged unscaled: an element below 2^-3 keeps an ABSOLUTE error of 2^-25 (its lo piece is an fp16
 * subnormal, which gfx950's matrix cores and converters keep), and |x| must stay below 65504 (beyond: inf -> NaN outputs, loudly).
 * Gradients (1e-7 .. 1e-4 in this model) do not fit fp16's range without a per-tensor scale: backward convolutions and weight
 * gradients of the mode that uses this code (hip.F32H in the Python layer) stay SSR_F32X3. */
#define SSR_F32H 3
#define SSR_F32H_WSHIFT 10

#define SSR_OK 0
#define SSR_EINVAL (-1)   /* bad descriptor (unsupported geometry / alignment) */
#define SSR_EUNSUP (-2)   /* combination not instantiated */

#define SSR_ACT_NONE 0
#define SSR_ACT_LRELU 1   /* LeakyReLU(0.2): rrdbnet_arch.py:32, discriminator_arch.py:44-68 */
#define SSR_ACT_RELU 2    /* ReLU: the VGG19 feature extractor of the perceptual loss (ssr_esrgan_model.py:153-160) */

/* A channel-sliced NHWC view. */
typedef struct ssr_view {
    void* p;          /* base pointer of the buffer (element type = desc dtype) */
    int32_t cs;       /* channels of the underlying buffer (pixel stride, in elements) */
    int32_t coff;     /* first channel of the slice */
} ssr_view;

/*
 * Direct (im2col-free) convolution on MFMA.  One descriptor covers
 *   forward:  nn.Conv2d 3x3 s1 p1 (rrdbnet_arch.py:26-30,99-112; discriminator_arch.py:28,34-40),
 *             4x4 s2 p1 (discriminator_arch.py:30-32), with F.interpolate(x2,'nearest') folded into
 *             the input read (`up`=2; rrdbnet_arch.py:127-128: source index = floor(o/2)),
 *   dgrad:    the same kernel with flipped/transposed packed weights; the stride-2 transposed conv is
 *             run as four 2x2 output-parity classes (oys/oyo/oxs/oxo),
 * plus the fused epilogue that replaces the reference's elementwise ops:
 *   s0 = alpha * act(acc + bias)                     -> y0 (optional)
 *   s1 = s0 + beta1*r1[c<r1_nc] + beta2*r2[c<r2_nc] (+ y_old if accumulate) -> y1 (optional)
 *   s2 = s1 * lrelu'(m) for channels in [m_c0, m_c1) -> y
 * (bias+LeakyReLU: rrdbnet_arch.py:38-41; x5*0.2+x and out*0.2+x: :44,:68; feat+body_feat: :125;
 *  lrelu(...)+skip: discriminator_arch.py:53-64; LeakyReLU backward masks and grad fan-in sums for
 *  autograd's backward of all of the above.)
 */
typedef struct ssr_conv_desc {
    int32_t dtype;            /* SSR_F32 | SSR_BF16 (x, w, y*, r*, m element type) */
    /* input side */
    ssr_view x;
    int32_t N, Hi, Wi;        /* stored input dims */
    int32_t up;               /* 1, or 2 = nearest x2 upsample on read (logical dims Hi*up x Wi*up) */
    int32_t Cin;              /* channels contracted from x (multiple of 8) */
    ssr_view x2;              /* optional second input (p == NULL: none): the contraction runs over the channel */
    int32_t Cin2;             /*   concatenation [x(Cin) | x2(Cin2)] — "gather" form of the dense-block backward */
    /* packed weights, chunk-major [Cin chunk][KH*KW][CoutPad][CK]; CK = ssr_conv2d_ck(dtype, KH) input
     * channels per chunk (32 bf16 / 16 fp32; half of that for 4x4 kernels), Cin zero-padded to a multiple */
    const void* w;
    int32_t CoutPad;          /* multiple of 32 */
    const float* bias;        /* Cout floats or NULL */
    /* geometry: grid position (gy,gx), tap (ty,tx) reads logical input (gy*stride+ty-pad_y, gx*stride+tx-pad_x) */
    int32_t KH, KW, stride, pad_y, pad_x;
    int32_t Gh, Gw;           /* output grid */
    /* output side: grid (gy,gx) -> stored pixel (gy*oys+oyo, gx*oxs+oxo) of Ho x Wo buffers */
    int32_t Ho, Wo, oys, oyo, oxs, oxo;
    int32_t Cout;             /* valid output channels (<= CoutPad) */
    ssr_view y, y0, y1;       /* y required; y0/y1 optional (p == NULL) */
    float alpha;
    int32_t act;
    ssr_view r1; int32_t r1_nc; float beta1;
    ssr_view r2; int32_t r2_nc; float beta2;
    int32_t accumulate;
    ssr_view m; int32_t m_c0, m_c1;   /* mask source: m[p, m.coff + c] for output channel c */
    /* 0, or 1 = space-to-depth evaluation of a 4x4 stride-2 pad-1 layer (KH = KW = 4, stride = 2, pad = 1, up = 1, even
     * Hi / Wi, Cin a power-of-two multiple of 32; see ssr_conv2d_s2d_ok): the layer is computed as a 2x2 stride-1
     * convolution over the view  x'[Y, X, q*Cin + c] = x[2Y-1 + (q>>1), 2X-1 + (q&1), c]  (zero outside), which the
     * big-tile kernel gathers while staging — nothing is materialised.  `w` must then be packed with
     * ssr_pack_item.fwd_s2d = 1: [q*Cin/32 + chunk][2x2 taps (dy,dx)][CoutPad][32], tap (ky,kx) = (2dy + (q>>1), 2dx + (q&1)). */
    int32_t s2d;
    /* 0: the mask `m` is LeakyReLU' (1 | 0.2 by the sign of m); 1: ReLU' (1 | 0) — backward through the VGG19 layers */
    int32_t m_relu;
    /* ---- LeakyReLU decision fix-up of the split-bf16 mode (SSR_F32X3; round 4).  The three-product split rounds a product at
     * 2^-16 instead of 2^-24: ~10x more pre-activations land on the other side of zero than in an fp32 evaluation, and every such
     * decision moves all upstream gradients by 0.8 x its gradient (measured: conv_first.weight 25 % of elements outside the 1e-3
     * gate with 48 of 22.8 M decisions flipped).  With fix_list set on a LeakyReLU layer the epilogue appends every output whose
     * pre-activation satisfies |v| < fix_thr to the list and ssr_conv2d_fixup recomputes exactly those from the fp32 inputs and
     * the UNPACKED fp32 weights in double precision and rewrites y: the decisions are then those of an exact evaluation (the
     * backward reads them from the sign of the stored output), all other outputs keep their 1e-5 accuracy.
     *   fix_list: int32 [4 + 2 * fix_cap]: [0] entries appended (may exceed fix_cap: the surplus is dropped), [1] internal ticket,
     *             [2] high-water mark of [0] (diagnostics), [3] unused; then (stored output pixel index, channel) pairs.  Zeroed
     *             once by the host; ssr_conv2d_fixup resets [0] and [1].
     *   w_ref: the layer's weights as the reference stores them, fp32 [Cout][w_ref_cin][KH][KW]; w_ref_sigma: NULL or the
     *          spectral-norm sigma (the effective weight is w_ref / sigma[0]).
     * Supported: stride 1, one input view (x2 = NULL), up 1 | 2, y only (no y0 / y1 / r1 / r2 / m / accumulate), alpha 1. */
    int32_t* fix_list;
    int32_t fix_cap;
    float fix_thr;
    const float* w_ref;
    const float* w_ref_sigma;
    int32_t w_ref_cin;
} ssr_conv_desc;

int ssr_conv2d(const ssr_conv_desc* d, void* stream);
/* recompute the outputs the launch of `d` listed in d->fix_list (see the fix_* fields); a no-op launch when the list is empty */
int ssr_conv2d_fixup(const ssr_conv_desc* d, void* stream);
/* n <= 4 descriptors (host array) of identical geometry in ONE launch where the kernel family supports it (the four
 * output-parity classes of a 4x4 stride-2 dgrad, built by the host as 2x2 stride-1 convolutions); otherwise n launches. */
int ssr_conv2d_batch(const ssr_conv_desc* ds, int32_t n, void* stream);
/* test / tuning hook: force a kernel family. 0 = automatic (ssr_conv2d), 1 = weight-stationary persistent
 * kernel (SSR_EUNSUP if the descriptor does not fit it), 2 = skip it (K-resident or pipelined kernel),
 * 3 = pipelined kernel only, 4 = big-tile kernel (32x16 pixels x 64 channels per workgroup; SSR_EUNSUP if unfit),
 * 5 = thin-output VALU kernel (Cout <= 8, Cin <= 64; SSR_EUNSUP if unfit).  SSR_F32X3 descriptors: 4 = the split-mode big-tile
 * kernel (csrc/conv_big_x3.hip), 6 = the producer / MFMA-wave ring kernel for small grids (csrc/conv_x3q.hip, round 5), 7 = the register-tiled
 * kernel that took those layers over in round 6 (csrc/conv_x3r.hip: four pixel tiles per MFMA wave, K split over four waves). */
int ssr_conv2d_impl(const ssr_conv_desc* d, void* stream, int32_t impl);
/* Which kernel instantiation ssr_conv2d dispatches this descriptor to, encoded as
 * KH*1000 + stride*100 + NT*10 + WAVES (NT = 32-channel output tiles per wave, WAVES per workgroup);
 * used by bench.py to attribute launch durations to kernel symbols.  Negative on error. */
int ssr_conv2d_variant(const ssr_conv_desc* d);
/* A dependent CHAIN of n (2..4) stride-1 3x3 SSR_F32X3 convolutions over one grid in ONE persistent launch (csrc/conv_x3c.hip): the dense
 * block's conv1..conv4 (rrdbnet_arch.py:37-41: each reads the channel prefix the earlier ones extend) or the slices 4..1 of its gather-form
 * backward.  The workgroups of an image hand their results to each other through memory (write-through stores, per-tile flag words,
 * bounded polls); a later descriptor may read what an earlier one writes, nothing else may alias.
 *   state: ssr_conv2d_chain_state_bytes(N, Gh, Gw) bytes of device memory, zeroed ONCE by the host, owned by the launches of ONE stream
 *          (consecutive launches reuse it: tickets, epoch and flags re-arm themselves; concurrent chains need one each).
 * When the list does not qualify (ssr_conv2d_chain_ok: 32 output channels each, one of the straight-line epilogues - bias + LeakyReLU,
 * plain, or LeakyReLU-backward mask - shared by all, <= 64 tiles per image) or state is NULL: n ssr_conv2d launches, same results
 * (forward chains bit for bit; backward chains sum K in the opposite direction). */
int ssr_conv2d_chain(const ssr_conv_desc* ds, int32_t n, void* state, void* stream);
int ssr_conv2d_chain_ok(const ssr_conv_desc* ds, int32_t n);
int64_t ssr_conv2d_chain_state_bytes(int32_t N, int32_t Gh, int32_t Gw);
/* The kernel symbol ssr_conv2d launches for this descriptor as rocprofv3 prints it (without the "void (anonymous namespace)::" prefix and
 * the argument list), e.g. "conv_x3r_kernel<1, 1, 0, 8, 2>" (NTW, NU, EP, TH, AM): the key under which bench.py, tools/pmc_traffic.py, tools/pmc_sq.py and
 * tools/roofline_check.py file a launch, so that roofline.kernel can be found in profiles/ by name.  buflen >= 48. */
int ssr_conv2d_symbol(const ssr_conv_desc* d, char* buf, int32_t buflen);
/* the same for the launch of ssr_conv2d_impl(d, stream, impl): the symbol of a forced family (SSR_EUNSUP where the launch would be) */
int ssr_conv2d_symbol_impl(const ssr_conv_desc* d, int32_t impl, char* buf, int32_t buflen);
/* input channels per packed weight chunk for a KHxKH kernel in `dtype` */
int ssr_conv2d_ck(int32_t dtype, int32_t KH);
/* 1 if a 4x4 stride-2 layer of this shape can run through the space-to-depth path (ssr_conv_desc.s2d), else 0 */
int ssr_conv2d_s2d_ok(int32_t dtype, int32_t Cin, int32_t Cout, int32_t CoutPad);

/*
 * Fused ResidualDenseBlock (rrdbnet_arch.py:37-44, and :68 for the third block of an RRDB), bf16,
 * num_feat 64 / num_grow_ch 32.  One launch keeps the whole dense block of an 8x8 or 8x16 tile (with its 5-pixel halo)
 * resident in LDS; only the weights are streamed.
 *   forward : in = x (64 ch) -> x1..x4 written to channels [64,192) of `slices`,
 *             out[0,64) = alpha5*(conv5(cat(x..x4)) + b5) + beta1*x + beta2*r2;
 *             w[k] = forward-packed weights of conv1..5 (ssr_pack_weights, 32-channel chunks), bias[k] their biases.
 *   backward: in = d_out (64 ch, gradient w.r.t. the block output) -> dpre4..dpre1 (pre-activation gradients of
 *             conv4..conv1, masked with lrelu'(x_k) read from `mask` = the forward `slices` buffer) written to
 *             channels [64,192) of `slices`; out[0,64) = d x = gathered dgrad + beta1*d_out + beta2*r2;
 *             w[j] = gather-packed weights of slice 4-j (ssr_pack_dgrad_gather; conv5's 0.2/0.04 folded in),
 *             bias = NULL, alpha5 = 1.
 */
typedef struct ssr_rdb_desc {
    int32_t dtype, N, H, W;
    ssr_view in, slices, out, mask;
    const void* w[5];
    const float* bias[5];
    float alpha5, beta1;
    ssr_view r2;
    float beta2;
    /* optional L2 warm-up: the five weight arrays of the NEXT launch on this stream (NULL / 0 = none).  Every block
     * touches its share of the lines of its own XCD's L2 while it computes, so that the next dense block's weight
     * stream (479 KB, re-read by all 256 blocks) hits L2 instead of the Infinity Cache / HBM. */
    const void* w_next[5];
    int32_t w_next_bytes[5];
    /* which kernel runs THIS launch: 0 = automatic (SSR_RDB_TILE from the environment, else the 8 x 16 tiles of csrc/rdb_tile.hip
     * when the launch gives (nearly) every CU a workgroup, else the 8 x 8 tiles of csrc/rdb_fwd.hip), 8 = 8 x 8 tiles, 16 = 8 x 16
     * tiles.  Both kernels add the same products in the same order: their results are bit-identical (tests/test_gpu_rdb_tile.py,
     * tests/test_gpu_rdb_stress.py).  A per-descriptor field, not library state: two plans may share the library. */
    int32_t tile;
} ssr_rdb_desc;
int ssr_rdb_forward(const ssr_rdb_desc* d, void* stream);
int ssr_rdb_backward(const ssr_rdb_desc* d, void* stream);
/* the kernel ssr_rdb_forward / ssr_rdb_backward run for this descriptor: 8 = 8 x 8 tiles, 16 = 8 x 16 tiles */
int ssr_rdb_tile_of(const ssr_rdb_desc* d);

/*
 * Weight gradient (autograd's convolution_backward weight/bias part, triggered at
 * ssr_esrgan_model.py:192,221,227):
 *   dW[co][ci][ky][kx] += alpha * sum_{n,gy,gx} dY[n, gy, gx, co] * X[n, gy*stride+ky-pad_y, gx*stride+kx-pad_x, ci]
 *   db[co]             += alpha * sum dY
 * dW/db are fp32 in the reference's OIHW layout.  Many layers can be processed by one launch: the
 * host passes device tables of layer descriptors and of work items (layer, co/ci tile, pixel-tile range).
 */
typedef struct ssr_wgrad_layer {
    ssr_view x;               /* forward input (same meaning as ssr_conv_desc.x) */
    ssr_view dy;              /* gradient w.r.t. the conv output (pre-activation), Gh x Gw pixels */
    int32_t N, Hi, Wi, up, Cin, Cout;
    int32_t pad_y, pad_x, Gh, Gw;
    float alpha;
    float* dw;                /* [Cout][Cin_w][KH][KW] fp32 */
    int32_t Cin_w;            /* Cin of the weight tensor (== real input channels; <= Cin) */
    float* db;                /* [Cout] or NULL */
} ssr_wgrad_layer;

typedef struct ssr_wgrad_item {
    int32_t layer, co0, ci0, tile_begin, tile_end, atomic;
    /* second 32-channel block of output gradients contracted with the SAME input patch (kernels with
     * ssr_wgrad_co_tile() == 64 only): nco == 2 -> channels co0_b.. of layer_b, which must read the same x view, ci0 and
     * geometry as `layer` (it may be `layer` itself: the other half of a 64-output conv).  nco == 0 or 1: single. */
    int32_t nco, layer_b, co0_b;
} ssr_wgrad_item;

int ssr_conv2d_wgrad(const ssr_wgrad_layer* layers_dev, const ssr_wgrad_item* items_dev, int32_t n_items,
                     int32_t dtype, int32_t KH, int32_t KW, int32_t stride, void* stream);
/* number of pixel tiles of a layer in the wgrad kernel selected by (dtype, KH): host helper for building items */
int32_t ssr_wgrad_tiles(int32_t N, int32_t Gh, int32_t Gw, int32_t dtype, int32_t KH);
/* input-channel width of a work item (ci0 must be a multiple of it; co0 a multiple of 32) for that kernel */
int32_t ssr_wgrad_ci_tile(int32_t dtype, int32_t KH);
/* 64 when that kernel takes paired items (nco == 2), else 32 */
int32_t ssr_wgrad_co_tile(int32_t dtype, int32_t KH);

/*
 * Weight packing (once per optimizer step; replaces cuDNN's internal filter transforms).
 * Table entry: src fp32 OIHW -> fwd [tap][CoutPad][CinPad] and dgrad layouts, optionally scaled by
 * 1/sigma (spectral norm, W_orig/sigma: torch.nn.utils.spectral_norm at discriminator_arch.py:30-39).
 */
typedef struct ssr_pack_item {
    const float* src;         /* [Cout][Cin][KH][KW] */
    const float* inv_scale;   /* device scalar sigma (weights are divided by it) or NULL */
    void* dst_fwd;            /* [CinPad/ck_fwd][KH*KW][CoutPad][ck_fwd] or NULL */
    void* dst_dgrad;          /* stride 1: [CoutPadI/ck_dgrad][KH*KW (taps flipped)][CinPadO][ck_dgrad];
                                 stride 2 (4x4): [4 parity classes][CoutPadI/ck_dgrad][4 taps][CinPadO][ck_dgrad];
                                 or NULL */
    int32_t Cout, Cin, KH, KW, stride;
    int32_t CoutPad, CinPad;      /* fwd padding */
    int32_t CinPadO, CoutPadI;    /* dgrad: "output" channels (=Cin) padded to 32, "input" (=Cout) padded to ck_dgrad */
    int32_t ck_fwd, ck_dgrad;     /* channels per chunk of the consuming kernels (ssr_conv2d_ck) */
    int32_t fwd_s2d;              /* 1: dst_fwd in the space-to-depth order of ssr_conv_desc.s2d (4x4 stride 2, ck_fwd = 32) */
} ssr_pack_item;

int ssr_pack_weights(const ssr_pack_item* items_dev, int32_t n_items, int32_t dtype, void* stream);

/*
 * Packed weights for the "gather" form of the dense-block backward (rrdbnet_arch.py:37-44 under autograd):
 *   d x_k = sum_{j > k} conv3x3( dpre_j , rot180(W_j[:, slice_k])^T )
 * i.e. ONE convolution per channel slice over the channel concatenation of all later pre-activation
 * gradients — the mirror image of the concat-free forward.  One table entry copies the slice of one later
 * conv into its K range of the gathered weight: dst[chunk][tap'][o][cc] with k = chunk*ck + cc,
 * value = scale * src[k - kbase][ci0 + o][8 - tap'] for kbase <= k < kbase + Cout (rows o >= nci are zero).
 */
typedef struct ssr_pack_seg {
    const float* src;         /* later conv, fp32 OIHW [Cout][Cin][3][3] */
    void* dst;                /* [Kpad/ck][9][rows_pad][ck] */
    float scale;              /* residual scaling folded in (0.2 / 0.04 for conv5: rrdbnet_arch.py:44,68) */
    int32_t Cout, Cin;        /* of src */
    int32_t ci0, nci;         /* slice of src's input channels = output channels of the gathered conv */
    int32_t kbase;            /* offset of src's Cout channels inside the concatenated K */
    int32_t rows_pad, ck;
} ssr_pack_seg;
int ssr_pack_dgrad_gather(const ssr_pack_seg* items_dev, int32_t n_items, int32_t dtype, void* stream);

/* dst[p, c] += src[p, c] over npix pixels and C channels of two NHWC views */
int ssr_add_views(ssr_view dst, ssr_view src, int32_t dtype, int64_t npix, int32_t C, void* stream);

/* ---- layout conversion at the plugin boundary (NCHW fp32 tensors of the reference API) ---- */
/* dst NHWC[n,h,w,coff+c] = src NCHW fp32 [n,c,h,w] * scale, optionally through pixel_unshuffle
 * (arch_util.py:769-785; `unshuffle` = 1 none | 2 | 4) and nearest upsampling by `up`
 * (lr_resized, ssr_esrgan_model.py:133). */
int ssr_nchw_to_nhwc(const float* src, int32_t N, int32_t C, int32_t H, int32_t W, ssr_view dst, int32_t dtype,
                     int32_t unshuffle, int32_t up, float scale, void* stream);
/* the inverse (outputs and gradients): dst NCHW fp32 [n,c,h,w] = src NHWC [n,h,w,coff+c], converted to fp32; dst is OVERWRITTEN */
int ssr_nhwc_to_nchw(ssr_view src, int32_t dtype, float* dst, int32_t N, int32_t C, int32_t H, int32_t W,
                     void* stream);
int ssr_fill(void* p, int64_t n_elems, int32_t dtype, float value, void* stream);

/* ---- bilinear x2 (align_corners=False): discriminator_arch.py:50,55,60 ---- */
/* y[n,2H,2W,C] = bilinear(a (+ b)) ; b optional (skip-add folded into the read) */
int ssr_bilinear2x_fwd(ssr_view a, ssr_view b, ssr_view y, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C,
                       void* stream);
/* s1 = bilinear2x^T(dy) (+ r if r.p) -> y1 (optional); y = s1 * lrelu'(m) (m optional) */
int ssr_bilinear2x_bwd(ssr_view dy, ssr_view r, ssr_view y1, ssr_view y, ssr_view m, int32_t dtype, int32_t N,
                       int32_t H, int32_t W, int32_t C, void* stream);
/* OR-ed into `dtype` of the two calls above: the per-pixel kernels for this call whatever the shape.  Default: layers whose
 * channels are whole groups of eight 16-byte vectors (64 in bf16, 32 in fp32 storage) use the LDS-tile kernels (same arithmetic,
 * same order: identical bytes in bf16).  A per-call flag, not library state.  Environment (read once): SSR_BILINEAR_FLAT=1. */
#define SSR_BILINEAR_FLAT 0x100
/* nearest x2 backward (2x2 sum) with the same epilogue: rrdbnet_arch.py:127-128 backward */
int ssr_nearest2x_bwd(ssr_view dy, ssr_view r, ssr_view y1, ssr_view y, ssr_view m, int32_t dtype, int32_t N,
                      int32_t H, int32_t W, int32_t C, void* stream);

/* ---- spectral norm (torch.nn.utils.spectral_norm, discriminator_arch.py:7,26,30-39) ---- */
typedef struct ssr_sn_item {
    const float* w;           /* weight_orig as [rows = Cout][cols = Cin*KH*KW] */
    float* u;                 /* [rows] in/out */
    float* v;                 /* [cols] in/out */
    float* sigma;             /* out: scalar */
    float* tmp;               /* [rows + cols + 4] scratch */
    int32_t rows, cols;
} ssr_sn_item;
/* one power iteration (train mode) for every layer in the table, then sigma = u.(W v);
 * with power_iter = 0 only sigma is recomputed (eval mode) */
int ssr_spectral_norm(const ssr_sn_item* items_dev, int32_t n_items, int32_t max_rows, int32_t max_cols,
                      int32_t power_iter, void* stream);
/* backward through W_sn = W/sigma: dW_orig += (dW_sn - <dW_sn, W_sn> u v^T) / sigma */
/* tmp: SSR_SN_BWD_SLOTS floats of scratch per item (per-block partial sums of <dW_sn, W>, added in index order: the result
 * does not depend on the order in which the blocks finish; nothing to zero) */
#define SSR_SN_BWD_SLOTS 64
typedef struct ssr_sn_bwd_item {
    const float* dw_sn; const float* w; const float* u; const float* v; const float* sigma;
    float* dw; float* tmp; int32_t rows, cols;
} ssr_sn_bwd_item;
int ssr_spectral_norm_bwd(const ssr_sn_bwd_item* items_dev, int32_t n_items, int32_t max_elems, void* stream);

/* ---- losses (BasicSR L1Loss / GANLoss('vanilla'); call sites ssr_esrgan_model.py:148,182,218,224) ---- */
/* USMSharp of BasicSR (img_process_util.USMSharp(radius=50, sigma=0), built at ssr_esrgan_model.py:31, applied to the
 * ground truth at :109): 51x51 Gaussian (sigma 8) blur with reflect padding, thresholded residual mask, soft blend.
 * src/dst: `planes` contiguous fp32 H x W planes (NCHW tensors: planes = N*C); src is multiplied by in_scale first
 * (1/255 for uint8-valued input), dst is in [0,1].  H*W <= 16384 (SSR_EUNSUP beyond), H, W > 25. */
int ssr_usm_sharp(const float* src, float* dst, int32_t planes, int32_t H, int32_t W, float in_scale, float weight,
                  float threshold, void* stream);

/* Deterministic reductions (run-to-run bit-identical results; the reference's fp32 CPU path is).
 * SSR_DETERMINISTIC OR-ed into the dtype of the two loss calls: loss_out / mean_out are arrays of SSR_LOSS_SLOTS floats, block b
 * adds its partial sum to slot b (single writer per slot and launch) and the reader adds the slots in index order; without the
 * flag: one fp32 atomicAdd per block into loss_out[0] (arrival order). */
#define SSR_DETERMINISTIC 0x200
#define SSR_LOSS_SLOTS 256
/* loss_out[0] += weight * mean|a-b| over (N,H,W,C valid); grad (optional) = weight*sign(a-b)/numel */
int ssr_l1_loss(ssr_view a, ssr_view b, ssr_view grad, int32_t dtype, int64_t npix, int32_t C, float weight,
                float* loss_out, void* stream);
/* SSIM loss of train.ssim_opt (SSIMLoss; csrc/ssim.hip; additive: the ABI version stays 3).  x (the generator's output), y (the target)
 * and grad are NHWC views of N x H x W pixels with C valid channels; fp32 storage for SSR_F32 / SSR_F32X3, bf16 for SSR_BF16, fp32
 * arithmetic in both.  Per channel plane: S = the 5 x 5 Gaussian-window (sigma 1.5) SSIM over 2-pixel reflect padding (edge not
 * repeated), C1 = 1e-4, C2 = 9e-4, eps = 1e-12;  loss_out[0] += weight * mean(clamp((1 - S) / 2, 0, 1)) over N*H*W*C elements
 * (SSR_DETERMINISTIC in dtype: per-block slots as ssr_l1_loss, at most SSR_LOSS_SLOTS blocks).  grad (optional: a null view gives the
 * loss only) receives d loss / d x: accumulate 0 writes the C valid channels, 1 adds to them (bf16: one rounding of the sum); channels
 * >= C of grad are never written, channels >= C of x and y never read.  The gradient is a gather (no float atomics): two launches
 * on the same inputs give the same bytes.  Null x or y, N or C <= 0, H or W < 3, or a view narrower than coff + C: SSR_EINVAL; another
 * dtype: SSR_EUNSUP; no launch in either case. */
int ssr_ssim_loss(ssr_view x, ssr_view y, ssr_view grad, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, float weight,
                  int32_t accumulate, float* loss_out, void* stream);
/* BCE-with-logits against constant target t: loss_out[0] += weight*mean(softplus(x) - x*t);
 * mean_out[0] += mean(x) (optional); grad = weight*(sigmoid(x)-t)/numel (optional) */
int ssr_bce_logits_loss(ssr_view x, ssr_view grad, int32_t dtype, int64_t npix, float target, float weight,
                        float* loss_out, float* mean_out, void* stream);
/* The other pixel and GAN losses of BasicSR 1.4.2 (csrc/losses.hip; additive: the ABI version stays 3), with the conventions of
 * ssr_l1_loss / ssr_bce_logits_loss: NHWC views, fp32 storage for SSR_F32 / SSR_F32X3 and bf16 for SSR_BF16 (fp32 terms, fp64 partial
 * sums), grad optional (a null view gives the loss only; channels outside the C valid ones are never written), loss_out[0] +=
 * weight * mean(...), SSR_DETERMINISTIC in dtype: per-block slots, at most SSR_LOSS_SLOTS blocks.  One launch each, the inputs read
 * once, no scratch.
 * ssr_pixel_loss (basicsr/losses/basic_loss.py: MSELoss, CharbonnierLoss; reduction 'mean'), d = a - b, n = npix * C:
 *   kind 1 MSE          weight * mean(d^2)                grad = 2 * weight * d / n
 *   kind 2 Charbonnier  weight * mean(sqrt(d^2 + eps))    grad = weight * d / (n * sqrt(d^2 + eps)), 0 where d == 0
 *   (eps: BasicSR's default is 1e-12; not read by kind 1).
 * ssr_gan_loss (basicsr/losses/gan_loss.py: GANLoss.forward), one logit x per pixel, n = npix, w = weight (the caller passes 1 for
 * is_disc and loss_weight otherwise, as for ssr_bce_logits_loss); target_val is the label of gan_type 1 and not read by the others
 * (GANLoss.get_target_label); is_disc is read by gan_type 4 only:
 *   gan_type 1 lsgan          w * mean((x - target_val)^2)                                     grad = 2 w (x - target_val) / n
 *   gan_type 2 wgan           real: -w * mean(x), fake: w * mean(x)                            grad = -+ w / n
 *   gan_type 3 wgan_softplus  real: w * mean(softplus(-x)), fake: w * mean(softplus(x))        grad = w (sigmoid(x) - 1) / n, w sigmoid(x) / n
 *   gan_type 4 hinge          is_disc: real w * mean(relu(1 - x)), fake w * mean(relu(1 + x))  grad = -+ w / n where the relu's argument
 *                             is > 0 (strictly, as torch), else 0;  generator: -w * mean(x)    grad = -w / n
 *   softplus(z) = max(z, 0) + log1p(exp(-|z|)).  mean_out[0] += mean(x) (optional).
 * A null input, npix or C <= 0, a view narrower than coff + C, eps < 0 (or NaN): SSR_EINVAL; another dtype, kind or gan_type:
 * SSR_EUNSUP; no launch in either case. */
int ssr_pixel_loss(ssr_view a, ssr_view b, ssr_view grad, int32_t dtype, int64_t npix, int32_t C, int32_t kind, float eps, float weight,
                   float* loss_out, void* stream);
int ssr_gan_loss(ssr_view x, ssr_view grad, int32_t dtype, int64_t npix, int32_t gan_type, int32_t target_is_real, int32_t is_disc,
                 float target_val, float weight, float* loss_out, float* mean_out, void* stream);

/* dst[e] += sum over p = 0 .. parts-1 (in that order) of src[p * stride + e], e < n: the fixed-order sum of per-split partial
 * weight gradients (deterministic mode: each pixel-range split of a layer is given its own partial dW / db as `dw` / `db` of a
 * layer-table entry of its own, so that every gradient element has ONE writer per launch) */
typedef struct ssr_reduce_item { float* dst; const float* src; int64_t n, stride; int32_t parts, pad_; } ssr_reduce_item;
int ssr_wgrad_reduce(const ssr_reduce_item* items_dev, int32_t n_items, int64_t max_elems, void* stream);

/* ---- optimizer: torch.optim.Adam (weight_decay 0, eps 1e-8) over a flat fp32 arena, with the
 *      BasicSR model_ema update fused (ssr_esrgan_model.py:193,228,230-231) ---- */
typedef struct ssr_adam_args {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
    float* ema;               /* NULL or EMA arena: ema = ema*decay + p*(1-decay) */
    int64_t n;
    const float* lr;          /* device scalar */
    int32_t* step;            /* device counter, incremented by the kernel launch */
    float beta1, beta2, eps, ema_decay, grad_scale;
} ssr_adam_args;
int ssr_adam_step(const ssr_adam_args* a, void* stream);

/* y = a*x + b*y over n fp32 elements (grad averaging / accumulation helpers) */
int ssr_axpby_f32(float a, const float* x, float b, float* y, int64_t n, void* stream);

/* ---- non-finite guard of the optimizer step (csrc/finite.hip) ----
 * ssr_nonfinite_scan: *flag = 1 if any element of the n_ranges (1..SSR_SCAN_MAX_RANGES) fp32 ranges srcs[k][0, ns[k]) is NaN or +-Inf
 *   (a bit test on the exponent).  The flag is only ever set, never cleared: the caller starts it at 0.  srcs / ns are host arrays;
 *   every pointer 4-byte aligned, ns[k] >= 0 (0: nothing to scan).  SSR_EINVAL without a launch otherwise.
 * ssr_adam_step_guarded: reads *flag on the device.  0: exactly ssr_adam_step (same arithmetic, *step += 1).  Non-zero: param, exp_avg,
 *   exp_avg_sq and *step are left as they are, the EMA (if any) still gets ema = ema*decay + p*(1-decay) from the unchanged p, and
 *   *skipped += 1.  *flag is 0 afterwards either way.  No host synchronisation: a step with both launches is capturable. */
#define SSR_SCAN_MAX_RANGES 8
int ssr_nonfinite_scan(const float* const* srcs, const int64_t* ns, int32_t n_ranges, int32_t* flag, void* stream);
int ssr_adam_step_guarded(const ssr_adam_args* a, int32_t* flag, int32_t* skipped, void* stream);

/* ---- BasicSR's other optimizers (csrc/optim.hip): the single-tensor arithmetic of torch.optim.Adam / AdamW / SGD / RMSprop over a
 *      flat fp32 arena, with what ssr_adam_step has (grad_scale folded in, lr and step on the device, the model_ema blend fused).
 * kind SSR_OPT_ADAM    g += weight_decay p (coupled); exp_avg, exp_avg_sq; SSR_OPT_AMSGRAD: max_exp_avg_sq = max(max_exp_avg_sq,
 *                      exp_avg_sq) takes exp_avg_sq's place in the denominator.  With weight_decay 0 and no amsgrad the call IS
 *                      ssr_adam_step[_guarded] (forwarded: the same bits).
 *      SSR_OPT_ADAMW   p *= 1 - lr weight_decay first (decoupled), then Adam's update; amsgrad as above.
 *      SSR_OPT_SGD     g += weight_decay p; momentum != 0: momentum_buffer = g while *step == 0 (the first applied step), afterwards
 *                      momentum buf + (1 - dampening) g; SSR_OPT_NESTEROV: g += momentum buf, otherwise g = buf; p -= lr g.
 *      SSR_OPT_RMSPROP g += weight_decay p; square_avg = alpha square_avg + (1 - alpha) g^2; SSR_OPT_CENTERED: grad_avg lerps to g by
 *                      1 - alpha and avg = sqrt(square_avg - grad_avg^2) (not clamped, as torch), otherwise avg = sqrt(square_avg);
 *                      avg += eps; momentum > 0: momentum_buffer = momentum buf + g / avg, p -= lr buf; otherwise p -= lr g / avg.
 * A state arena is needed exactly when its option is on (max_exp_avg_sq: amsgrad; momentum_buffer: momentum != 0; grad_avg: centered)
 * and is neither read nor written otherwise (pass NULL).  SSR_EINVAL without a launch: a null param / grad / lr / step or a needed arena,
 * n <= 0, a flag of another kind, momentum < 0, nesterov without momentum or with dampening.  SSR_EUNSUP: another kind.
 * Both launches end with *step += 1.  ssr_optim_step_guarded reads *flag on the device like ssr_adam_step_guarded: non-zero leaves
 * param, every state arena and *step as they are, moves only the EMA (toward the unchanged p), *skipped += 1; *flag is 0 afterwards. */
#define SSR_OPT_ADAM 0
#define SSR_OPT_ADAMW 1
#define SSR_OPT_SGD 2
#define SSR_OPT_RMSPROP 3
#define SSR_OPT_AMSGRAD 1
#define SSR_OPT_NESTEROV 2
#define SSR_OPT_CENTERED 4
typedef struct ssr_optim_args {
    float* param; const float* grad;
    float* exp_avg; float* exp_avg_sq; float* max_exp_avg_sq;      /* Adam, AdamW */
    float* momentum_buffer;                                        /* SGD, RMSprop */
    float* square_avg; float* grad_avg;                            /* RMSprop */
    float* ema;               /* NULL or EMA arena: ema = ema*decay + p*(1-decay) */
    int64_t n;
    const float* lr;          /* device scalar */
    int32_t* step;            /* device counter of applied steps, incremented by the launch */
    int32_t kind, flags;
    float beta1, beta2, eps, weight_decay, momentum, dampening, alpha, ema_decay, grad_scale;
} ssr_optim_args;
int ssr_optim_step(const ssr_optim_args* a, void* stream);
int ssr_optim_step_guarded(const ssr_optim_args* a, int32_t* flag, int32_t* skipped, void* stream);

/* ---- image quantisation and validation metrics (csrc/metrics.hip) ----
 * ssr_quantize_u8: fp32 NCHW -> uint8 NHWC, clamp(0,1) * 255 then mode 0: round half to even (basicsr tensor2img as called at
 *   /root/reference/ssr/models/ssr_esrgan_model.py:302-305), mode 1: truncate (astype(uint8) at /root/reference/ssr/infer_grid.py:60-64,
 *   infer.py:58-60).
 * ssr_metric_shift_sums: a, b uint8 [H][W][C], C <= 4.  For every offset pair (ro, co) in [0, max_offset]^2 and channel c writes
 *   out[((ro*(max_offset+1) + co)*C + c)*2 + {0,1}] = sum d, sum d^2 (exact, int64) over the window of
 *   (H-2*crop-max_offset) x (W-2*crop-max_offset) pixels, d = a[y+crop+ro][x+crop+co][c] - b[y+crop+max_offset-ro][x+crop+max_offset-co][c]:
 *   max_offset 0 -> PSNR (basicsr calculate_psnr), 8 -> cPSNR (/root/reference/ssr/metrics/cpsnr.py:36-55).
 * ssr_metric_ssim_sums: out[c] = sum over the valid region of the SSIM map of channel c (11x11 Gaussian window, sigma 1.5, fp64;
 *   basicsr calculate_ssim); the caller divides by (H-2*crop-10)*(W-2*crop-10). */
int ssr_quantize_u8(const float* src_nchw, uint8_t* dst_nhwc, int32_t N, int32_t C, int32_t H, int32_t W, int32_t mode, void* stream);
/* ssr_quantize_u8 that also adds the number of NaN / +-Inf samples of src into the device counter *nonfinite in the same pass (one
 * atomic per wave; the caller zeroes the counter).  The bytes it writes are ssr_quantize_u8's. */
int ssr_quantize_u8_checked(const float* src_nchw, uint8_t* dst_nhwc, int32_t N, int32_t C, int32_t H, int32_t W, int32_t mode,
                            int32_t* nonfinite, void* stream);
int ssr_metric_shift_sums(const uint8_t* a, const uint8_t* b, int32_t H, int32_t W, int32_t C, int32_t crop, int32_t max_offset,
                          int64_t* out, void* stream);
int ssr_metric_ssim_sums(const uint8_t* a, const uint8_t* b, int32_t H, int32_t W, int32_t C, int32_t crop, double* out, void* stream);

/* ---- scene inference: a whole Sentinel-2 image stack in, one super-resolved mosaic out (csrc/scene.hip) ----
 * A scene is uint8 [T][H][W][3] in device memory, H and W multiples of 32 (SSR_EUNSUP otherwise); chunk (i, j) of the
 * gh x gw = H/32 x W/32 grid has id i*gw + j.  Scene, mosaic and view base pointers are 16-byte aligned.  Chunk and frame ids are
 * DEVICE arrays, so one generator plan (and its captured forward graph) serves every batch of a scene; an item whose chunk id (or one
 * of whose frame ids) lies outside the scene is skipped: nothing is read or written for it.
 * ssr_scene_zero_scan: has_zero[(i*gw + j)*T + t] = 1 if any of the 3072 bytes of frame t of chunk (i, j) is 0, else 0: the validity
 *   test `[0, 0, 0] in ts` of format_s2naip_data (ssr/utils/infer_utils.py:12-20), which on an ndarray means "any sample equals 0".
 * ssr_scene_gather: the generator's NHWC input for a batch of B chunks (dst: [B, 32, 32, cs] of `dtype` storage, SSR_F32 / SSR_F32X3
 *   or SSR_BF16): channel k*3 + c of pixel (y, x) of item b = scene[frame_ids[b*n + k]][32 i + y][32 j + x][c] / 255 with (i, j) =
 *   chunk_ids[b] - the frame-major stacking, `.float() / 255` (as ATen divides by a host scalar on the device: x * fp32(1/255)) and layout change of infer_utils.py:33-38 followed by
 *   ssr_nchw_to_nhwc's rounding to the storage type, bit for bit.  Channels 3n .. cs of the view are not written.  n > T, n > 512 or
 *   an unknown dtype: SSR_EUNSUP.
 * ssr_scene_scatter_u8: the generator's NHWC output (src: [B, 128, 128, cs], C <= 8 channels used) -> mosaic uint8 [Ho][Wo][C]
 *   (Ho, Wo multiples of 128): item b lands at rows 128 i .., columns 128 j .. (stitch, infer_utils.py:41-60) after
 *   ssr_quantize_u8's mode-1 arithmetic: clamp(0, 1) * 255, truncated (infer_grid.py:60-64).  The number of NaN / +-Inf samples among
 *   the C channels is added to the device counter *nonfinite (one atomic per wave that saw any; the caller zeroes it), as
 *   ssr_quantize_u8_checked does. */
int ssr_scene_zero_scan(const uint8_t* scene, int32_t T, int32_t H, int32_t W, uint8_t* has_zero, void* stream);
int ssr_scene_gather(const uint8_t* scene, int32_t T, int32_t H, int32_t W, const int32_t* chunk_ids, const int32_t* frame_ids,
                     int32_t B, int32_t n, ssr_view dst, int32_t dtype, void* stream);
int ssr_scene_scatter_u8(ssr_view src, int32_t dtype, const int32_t* chunk_ids, int32_t B, int32_t C, uint8_t* mosaic, int32_t Ho,
                         int32_t Wo, int32_t* nonfinite, void* stream);

/* ---- scene inference, overlapping chunks blended in the output (csrc/scene.hip; additive: the ABI version stays 3) ----
 * H and W are ANY values >= 32 (SSR_EUNSUP below that).  The place of chunk b is origins[2b], origins[2b + 1] = (y0, x0), the
 * low-resolution pixel of its first sample (a DEVICE array of int32 pairs); an item whose origin lies outside
 * [0, H - 32] x [0, W - 32] (or one of whose frame ids lies outside [0, T)) is skipped: nothing is read or written for it.  The scene
 * pointer needs no alignment: nothing outside the rows of a chunk is read.
 * ssr_scene_zero_scan_at: has_zero[b*T + t] = 1 if any of the 3072 bytes of frame t of the window at origin b is 0, else 0.
 * ssr_scene_gather_at: ssr_scene_gather with the chunk at the origin: the same x * fp32(1/255) and storage rounding, the same
 *   conditions on dst, n and dtype.
 * ssr_scene_blend_add: the generator's NHWC output (src: [B, 128, 128, cs], C <= 8 channels used, coff + C <= cs) is added into
 *   acc, uint32 [Ho][Wo][C] (Ho = 4H, Wo = 4W, 16-byte aligned, zeroed by the caller): for sample v of pixel (r, col) of item b
 *     f = (uint32) (fminf(fmaxf(v, 0), 1) * 65535.0f)         fp32 multiply, truncation; NaN -> 0
 *     acc[4 y0 + r][4 x0 + col][c] += f * window[r] * window[col]
 *   with window a DEVICE array int32[128] (weights <= 64, so one term stays below 2^28).  The adds are integer atomics: items of one
 *   launch, and launches, may overlap, and the sums do not depend on the order of arrival.  The number of NaN / +-Inf samples among
 *   the C channels is added to *nonfinite as ssr_scene_scatter_u8 does.  Ho or Wo below 128 or no multiple of 4: SSR_EUNSUP.
 * ssr_scene_blend_finish: mosaic[y][x][c] = (uint8) ((uint64) acc[y][x][c] * 255 / ((uint64) Sy[y] * Sx[x] * 65535)), truncating as
 *   the reference's quantiser does; Sy int32 [Ho] and Sx int32 [Wo] (device) are the sums of the window weights of the chunks that
 *   cover the row / column (a zero sum gives 0).  mosaic is uint8 [Ho][Wo][C], 4-byte aligned. */
int ssr_scene_zero_scan_at(const uint8_t* scene, int32_t T, int32_t H, int32_t W, const int32_t* origins, int32_t n_chunks,
                           uint8_t* has_zero, void* stream);
int ssr_scene_gather_at(const uint8_t* scene, int32_t T, int32_t H, int32_t W, const int32_t* origins, const int32_t* frame_ids,
                        int32_t B, int32_t n, ssr_view dst, int32_t dtype, void* stream);
int ssr_scene_blend_add(ssr_view src, int32_t dtype, const int32_t* origins, int32_t B, int32_t C, const int32_t* window,
                        uint32_t* acc, int32_t Ho, int32_t Wo, int32_t* nonfinite, void* stream);
int ssr_scene_blend_finish(const uint32_t* acc, const int32_t* Sy, const int32_t* Sx, int32_t C, uint8_t* mosaic, int32_t Ho,
                           int32_t Wo, void* stream);

/* ---- scene inference for multi-band generators (csrc/scene.hip; additive: the ABI version stays 3) ----
 * The option `s2_bands: [tci, b05, ...]` of the dataset at inference: beside the TCI scene, uint8 [T][H][W][3], lie K >= 1 extra
 * bands as uint8 [K][T][H][W], one plane per band (a band PNG decodes straight into its plane).  Neither pointer needs an alignment.
 * ssr_scene_gather_bands: ssr_scene_gather_at with 3 + K channels per chosen frame.  For item b, pixel (y, x), slot s < n and
 *   f = frame_ids[b*n + s], (y0, x0) = origins[2b], origins[2b + 1]: channel s*(3 + K) + c of dst is tci[f][y0 + y][x0 + x][c] for
 *   c < 3 and bands[c - 3][f][y0 + y][x0 + x] otherwise - frame-major, TCI first, then the bands in the order given, which is
 *   S2NAIPDataset._load_s2(...)[frames].reshape(-1, 32, 32) - each x * fp32(1/255), then rounded to the storage type, as
 *   ssr_scene_gather does.  Channels n*(3 + K) .. cs of the view are not written; grid chunks are the origins (32 i, 32 j).  An item
 *   whose origin lies outside [0, H - 32] x [0, W - 32] or one of whose frame ids lies outside [0, T) is skipped: nothing is read
 *   or written for it.  A null pointer, K < 1 or n*(3 + K) channels that do not fit the view: SSR_EINVAL; H or W below 32, n > T,
 *   n > 512, more than 64 KiB of row staging (n*(26 + 10 K) words) or an unknown dtype: SSR_EUNSUP.  The zero test stays
 *   ssr_scene_zero_scan(_at) over the TCI: the extra bands take no part in the choice of frames. */
int ssr_scene_gather_bands(const uint8_t* tci, const uint8_t* bands, int32_t K, int32_t T, int32_t H, int32_t W,
                           const int32_t* origins, const int32_t* frame_ids, int32_t B, int32_t n, ssr_view dst, int32_t dtype,
                           void* stream);

/* ---- scene inference, each chunk's clearest frames chosen on the device (csrc/scene.hip; additive: the ABI version stays 3) ----
 * The option `frame_select: clearest`.  Both entries replace, for that policy, the frame choice of `select_frames` /
 * format_s2naip_data (ssr/utils/infer_utils.py:12-31: `random.sample` among the frames without a zero sample); the policy itself is
 * this project's own and has no counterpart file in the reference.  ESA's TCI encodes 0 as NODATA and 255 as SATURATED.
 * ssr_scene_frame_keys: for frame t of the 32 x 32 window at origins[2b], origins[2b + 1] = (y0, x0) of the TCI scene uint8
 *   [T][H][W][3] (H, W >= 32, SSR_EUNSUP below that; no alignment needed, nothing outside the rows of a window is read)
 *     z = pixels with AT LEAST ONE zero sample among R, G, B       (z > 0 is ssr_scene_zero_scan_at's flag)
 *     s = pixels whose THREE samples are all 255                   (never also in z: z + s <= 1024)
 *     keys[b*T + t] = (z << 16) | s
 *   keys is a DEVICE array uint32 [n_chunks][T], 4-byte aligned; the T words of an origin outside [0, H - 32] x [0, W - 32] are not
 *   written.  A null pointer, a size <= 0 or more than 2^30 items: SSR_EINVAL.
 * ssr_scene_rank_frames: frame_ids[b*n + r] = the frame of rank r < n among the T frames of chunk b ordered by (key, frame index)
 *   ascending - fewest NODATA pixels first, then fewest saturated ones, then the lower index - an exact integer ranking without
 *   atomics: every run writes the same words.  frame_ids is the int32 [n_chunks][n] DEVICE array the three gather entries read.
 *   Because z leads the key every frame without a zero precedes every frame with one: the chosen SET is one the reference's rule
 *   can draw.  T > 1024 or n > T: SSR_EUNSUP; a null pointer or a size <= 0: SSR_EINVAL. */
int ssr_scene_frame_keys(const uint8_t* scene, int32_t T, int32_t H, int32_t W, const int32_t* origins, int32_t n_chunks,
                         uint32_t* keys, void* stream);
int ssr_scene_rank_frames(const uint32_t* keys, int32_t n_chunks, int32_t T, int32_t n, int32_t* frame_ids, void* stream);

/* ---- scene inference, NODATA carried through to the mosaic (csrc/scene.hip; additive: the ABI version stays 3) ----
 * The option `nodata: keep`.  The policy is this project's own: no counterpart in the reference, whose infer_grid.py writes
 * whatever the generator makes of zero input.  ESA's TCI encodes 0 as NODATA: a low-resolution pixel of a frame HAS DATA if none of
 * its three TCI samples is 0 (the complement of ssr_scene_frame_keys' z; extra bands take no part).
 * ssr_scene_support_add: support is a DEVICE array int32 [H][W], 4-byte aligned, which the caller zeroes once per scene.  For each
 *   of the B chunks at origins[2b], origins[2b + 1] = (y0, x0) and each pixel (y, x) of its 32 x 32 window,
 *     support[y0 + y][x0 + x] += the number of slots k < n whose frame frame_ids[b*n + k] has data at (y0 + y, x0 + x)
 *   by integer atomics: any arrival order of overlapping chunks gives the same words.  It counts what the gather entries fed to
 *   the generator: a chunk whose origin lies outside [0, H - 32] x [0, W - 32] or one of whose frame ids lies outside [0, T) adds
 *   nothing, as the gathers skip it.  The scene is uint8 [T][H][W][3] (H, W >= 32, SSR_EUNSUP below that, as n > T or n > 512); no
 *   alignment needed, nothing outside the rows of a window is read.  A null pointer, a size <= 0 or B > 2^20: SSR_EINVAL.
 * ssr_scene_apply_nodata: rewrites the mosaic uint8 [Ho][Wo][C] (Ho = 4 H, Wo = 4 W, 1 <= C <= 8, 4-byte aligned) in place: with
 *   s = support[y / 4][x / 4], sample (y, x, c) becomes 0 if s < min_support, else max(1, sample) - 0 stays reserved for NODATA in
 *   the output as it is in ESA's input.  support_u8, if not null, receives min(support, 255) as uint8 [H][W].  min_support < 1, a
 *   null mosaic or support, C outside 1 .. 8: SSR_EINVAL; Ho or Wo no multiple of 4: SSR_EUNSUP. */
int ssr_scene_support_add(const uint8_t* scene, int32_t T, int32_t H, int32_t W, const int32_t* origins, const int32_t* frame_ids,
                          int32_t B, int32_t n, int32_t* support, void* stream);
int ssr_scene_apply_nodata(uint8_t* mosaic, int32_t Ho, int32_t Wo, int32_t C, const int32_t* support, int32_t min_support,
                           uint8_t* support_u8, void* stream);

/* ---- scene inference, self-ensemble over the eight flips and transposes (csrc/scene.hip; additive: the ABI version stays 3) ----
 * The option `self_ensemble: true`: BasicSR's `val.self_ensemble` transform set (SRModel.test_selfensemble: 'v', 'h', 't'), averaged
 * by this project's integer blend instead of a float mean.  A transform id tf in 0 .. 7 has three bits, applied in this order to the
 * two spatial axes of a chunk P: bit 0 flips the columns, bit 1 flips the rows, bit 2 transposes.  So pixel (y, x) of a 32 x 32
 * chunk lands at (y', x') with x' = tf & 1 ? 31 - x : x, y' = tf & 2 ? 31 - y : y, swapped if tf & 4; the inverse undoes the bits in
 * the opposite order, on 128 x 128 outputs.  The generator rows are (chunk, tf) pairs: origins, frame_ids and tf are per ROW.
 * ssr_scene_gather_tf: row b of dst is the transform tf[b] of the chunk ssr_scene_gather_at (bands == null, K == 0) or
 *   ssr_scene_gather_bands (bands uint8 [K][T][H][W], K >= 1) writes for origins[2b .. 2b + 1] and frame_ids[b*n ..]: the same
 *   x * fp32(1/255) and storage rounding, the same channel order, so with tf[b] == 0 the same bytes.  tf is a DEVICE array int32 [B].
 *   A row whose origin lies outside the scene, one of whose frame ids lies outside [0, T) or whose tf lies outside [0, 7] is skipped:
 *   nothing is read or written for it.  Conditions and return codes as ssr_scene_gather_bands, with K == 0 allowed (bands is then
 *   not read; bands == null with K >= 1: SSR_EINVAL).
 * ssr_scene_blend_add_tf: ssr_scene_blend_add of the INVERSE transform tf[b] of item b's output, with 13 fractional bits:
 *     f = (uint32) (fminf(fmaxf(v, 0), 1) * 8191.0f)          fp32 multiply, truncation; NaN -> 0
 *     acc[4 y0 + r][4 x0 + col][c] += f * window[r] * window[col]        v = sample c of the pixel of src that the inverse puts at (r, col)
 *   window is indexed by the place in the accumulator (it is symmetric).  8 * 125 * 125 * 8191 < 2^32: the eight rows of every chunk
 *   of a scene fit the uint32 words where 16 fractional bits would not.  Rows skipped as above add nothing and count nothing;
 *   non-finite samples are counted over every row that is not skipped.  Other conditions as ssr_scene_blend_add.
 * ssr_scene_blend_finish_scaled: ssr_scene_blend_finish with the denominator's scale as an argument,
 *     mosaic[y][x][c] = (uint8) ((uint64) acc[y][x][c] * 255 / ((uint64) Sy[y] * Sx[x] * scale)),
 *   scale = 8 * 8191 for the self-ensemble (65535 gives ssr_scene_blend_finish).  scale < 1: SSR_EINVAL. */
int ssr_scene_gather_tf(const uint8_t* tci, const uint8_t* bands, int32_t K, int32_t T, int32_t H, int32_t W, const int32_t* origins,
                        const int32_t* frame_ids, const int32_t* tf, int32_t B, int32_t n, ssr_view dst, int32_t dtype, void* stream);
int ssr_scene_blend_add_tf(ssr_view src, int32_t dtype, const int32_t* origins, const int32_t* tf, int32_t B, int32_t C,
                           const int32_t* window, uint32_t* acc, int32_t Ho, int32_t Wo, int32_t* nonfinite, void* stream);
int ssr_scene_blend_finish_scaled(const uint32_t* acc, const int32_t* Sy, const int32_t* Sx, int32_t C, int32_t scale, uint8_t* mosaic,
                                  int32_t Ho, int32_t Wo, void* stream);

/* ---- scene inference from raw Sentinel-2 L1C: reprojection onto the grid (csrc/reproject.hip; additive: the ABI version stays 3) ----
 * The model's grid is Web-Mercator at 2 pi R / 2^22 m per pixel (R = 6378137), global pixel (px, py) from x = -pi R, y = +pi R, py
 * southwards; ESA's rasters are UTM.  satlas_super_resolution_amd/s2_reproject.py states every formula (`source_coords`,
 * `warp_bilinear`); these two entries compute them on the device.
 * ssr_merc_to_utm_coords: coords is a DEVICE array int32 [h][w][2], 8-byte aligned.  For the CENTRE of pixel (px0 + j, py0 + i) of
 *   the window: longitude and latitude (lat = atan(sinh(y / R))), then easting E and northing N in the WGS84 UTM zone of `epsg` by
 *   the Krueger series through n^6 (k0 = 0.9996, false easting 500 000, false northing 10 000 000 for 327zz, central meridian
 *   6 zone - 183), all in fp64; u = (E - ulx) / xdim - 0.5, v = (N - uly) / ydim - 0.5;
 *     coords[i][j] = (floor(u 65536 + 0.5), floor(v 65536 + 0.5))   where -0.5 <= u < cols - 0.5 and -0.5 <= v < rows - 0.5,
 *     coords[i][j] = (INT32_MIN, INT32_MIN)                         elsewhere (the sentinel).
 *   SSR_EINVAL: a null or misaligned coords, w, h, rows or cols <= 0, a negative px0 / py0 or a window that leaves the 2^22 grid,
 *   xdim <= 0, ydim >= 0, a non-finite ulx / uly / xdim / ydim.  SSR_EUNSUP: an epsg outside 32601 .. 32660 and 32701 .. 32760, w or
 *   h above 4096, rows or cols above 32767 (the coordinates would not fit the 16.16 words).
 * ssr_scene_warp_bilinear: src uint8 [T][Hs][Ws][C], C = 1 or 3, ANY address (no alignment is assumed); coords as above, shared
 *   by the T frames; dst uint8 [T][h][w][C].  x0 = U >> 16 (arithmetic), fx = U & 0xffff, likewise y; the four neighbours are
 *   clamped into the raster, so no coordinate makes the kernel read outside src;
 *     dst = ((65536 - fx)(65536 - fy) p00 + fx (65536 - fy) p10 + (65536 - fx) fy p01 + fx fy p11 + 2^31) >> 32   in 64-bit integers,
 *   0 in every channel at the sentinel.  mode 0 (blend): that; mode 1 (propagate): a pixel one of whose neighbours with NON-ZERO
 *   weight has a zero among its C samples is 0 in every channel.  Every pixel is written whole by one thread, nothing is
 *   accumulated: a second launch writes the same bytes.  SSR_EINVAL: a null pointer, a misaligned coords, a size <= 0, another
 *   mode.  SSR_EUNSUP: C not 1 or 3, w or h above 4096, Hs or Ws above 32767, T above 65535. */
int ssr_merc_to_utm_coords(int32_t px0, int32_t py0, int32_t w, int32_t h, int32_t epsg, double ulx, double uly, double xdim,
                           double ydim, int32_t rows, int32_t cols, int32_t* coords, void* stream);
int ssr_scene_warp_bilinear(const uint8_t* src, int32_t T, int32_t Hs, int32_t Ws, int32_t C, const int32_t* coords, int32_t h,
                            int32_t w, int32_t mode, uint8_t* dst, void* stream);

/* ---- VGG19 perceptual loss glue (csrc/vgg.hip; the convolutions run through ssr_conv2d with SSR_ACT_RELU / m_relu) ----
 * ssr_channel_affine: y[p, c] (+)= x[p, c] * scale[c] + shift[c] for c < C <= 8 (host float arrays, copied into the launch):
 *   the input normalisation (x - mean) / std of the feature extractor and, with accumulate = 1, its adjoint.
 * ssr_relu_maxpool2_fwd: P[N, H/2, W/2, C] = maxpool2x2(relu(F[N, H, W, C])), H and W even.
 * ssr_relu_maxpool2_bwd: gF (+)= the adjoint: each window's gradient goes to its first maximum (row-major) if F there is > 0. */
typedef struct ssr_vec8 { float v[8]; } ssr_vec8;
int ssr_channel_affine(ssr_view x, ssr_view y, int32_t dtype, int64_t npix, int32_t C, const float* scale, const float* shift,
                       int32_t accumulate, void* stream);
int ssr_relu_maxpool2_fwd(ssr_view f, ssr_view p, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
int ssr_relu_maxpool2_bwd(ssr_view f, ssr_view gp, ssr_view gf, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C,
                          int32_t accumulate, void* stream);

/* ---- Gram-matrix style term of the perceptual loss (csrc/gram.hip; PerceptualLoss with style_weight > 0, criterion 'l1':
 *      l_g_style at ssr_esrgan_model.py:154-160) ----
 * Features f are NHWC [N, HW, C] (HW = H*W pixels, C % 64 == 0); fp32 storage (SSR_F32 / SSR_F32X3) runs exact fp32 MFMA, SSR_BF16
 * bf16 MFMA, both with fp32 accumulation.  Every result is run-to-run bit-identical (no float atomics outside ssr_gram_l1's
 * non-deterministic loss sum).
 * ssr_gram_splits: the pixel splits ssr_gram_fwd uses for this shape; ws must hold splits * N * C * C floats when splits > 1.
 * ssr_gram_fwd: g[n] = scale * f[n]^T f[n], fp32 [N, C, C], exactly symmetric; the partial matrices of the splits (ws) are added
 *   in split order.
 * ssr_gram_l1: loss_out[0] += weight * sum |gx - gt| over n elements (SSR_DETERMINISTIC in dtype: per-block slots as ssr_l1_loss);
 *   sgn (optional, element type = dtype) = sign(gx - gt), 0 where equal.
 * ssr_gram_bwd: gf[n] (+)= coef * f[n] sgn[n] ([HW x C] x [C x C] per image; sgn symmetric, element type = dtype). */
int ssr_gram_splits(int32_t N, int32_t HW, int32_t C);
int ssr_gram_fwd(ssr_view f, float* g, float* ws, int32_t dtype, int32_t N, int32_t HW, int32_t C, float scale, void* stream);
int ssr_gram_l1(const float* gx, const float* gt, void* sgn, int32_t dtype, int64_t n, float weight, float* loss_out, void* stream);
int ssr_gram_bwd(ssr_view f, const void* sgn, ssr_view gf, int32_t dtype, int32_t N, int32_t HW, int32_t C, float coef,
                 int32_t accumulate, void* stream);

/* ---- LPIPS validation metric (csrc/lpips.hip; `calculate_lpips`, lpips_model 'vgg'; additive: the ABI version stays 3).  The VGG16
 *      convolutions run through ssr_conv2d in SSR_F32 with SSR_ACT_RELU, the pooling behind a tap through ssr_relu_maxpool2_fwd ----
 * ssr_lpips_input: the scaling layer.  u is uint8 [npix][3]; y an NHWC fp32 view (SSR_F32 / SSR_F32X3 storage) of npix pixels with
 *   at least coff + 8 channels, 16-byte aligned (cs % 4 == 0, coff % 4 == 0).  Network channel c = 0, 1, 2 receives, every step
 *   rounded to fp32 in this order (IEEE division, so a numpy float32 restatement gives the same bits),
 *       v = (float)u[p][perm[c]] / 255.0f;   if (normalize) v = 2.0f * v - 1.0f;   y[p][coff + c] = (v - shift[c]) / scale[c];
 *   channels coff + 3 .. coff + 7 are written as 0.  shift, scale (3 floats, scale != 0) and perm (3 ints in 0 .. 2; {2, 1, 0}
 *   feeds an RGB image as BGR) are host arrays, copied into the launch.  A null pointer, npix <= 0, a bad perm or scale, a view
 *   narrower than coff + 8 or misaligned: SSR_EINVAL; bf16 storage: SSR_EUNSUP; no launch in either case.
 * ssr_lpips_layer: one tap.  fa, fb are NHWC fp32 views of N x HW pixels with C valid channels (the features of the two images,
 *   taken BEFORE the ReLU when relu = 1, which the kernel then applies; 16-byte aligned as above), w holds C floats on the device
 *   (16-byte aligned).  With a^[p][c] = a[p][c] / (sqrt(sum_c a[p][c]^2) + 1e-10), the norm in fp64 (a pixel that is all zero
 *   gives 0 / 1e-10 = 0),
 *       partial[n][b] = block b's share of (1 / HW) sum_p sum_c w[c] * (a^[p][c] - b^[p][c])^2        (double, b < nblk)
 *   where the difference is formed directly in fp64 from the two normalised values (never from the expanded square, which
 *   cancels for similar images) and rounded to fp32, d * d and then w[c] * (d * d) are fp32 products, and all sums are fp64.
 *   Every partial is written (no atomics, no zeroing needed); the caller adds partial[n][0 .. nblk) in index order.  Identical
 *   fa and fb give exactly 0.0; two launches on the same inputs give the same bytes.
 *   SSR_EUNSUP: bf16 storage, C % 64 != 0 or C > 512.  SSR_EINVAL: a null pointer, N, HW or C <= 0, N > 65535, a view narrower
 *   than coff + C or misaligned.  No launch in any of these cases.
 * ssr_lpips_layer_blocks: nblk for this shape (>= 1; SSR_EINVAL for a size <= 0). */
int ssr_lpips_input(const uint8_t* u, ssr_view y, int32_t dtype, int64_t npix, const float* shift, const float* scale,
                    const int32_t* perm, int32_t normalize, void* stream);
int ssr_lpips_layer_blocks(int32_t N, int32_t HW, int32_t C);
int ssr_lpips_layer(ssr_view fa, ssr_view fb, const float* w, int32_t dtype, int32_t N, int32_t HW, int32_t C, int32_t relu,
                    double* partial, void* stream);

/* ---- The geometries of LPIPS's AlexNet backbone outside ssr_conv2d's families (csrc/conv_direct.hip; `calculate_lpips`, lpips_model
 *      'alexnet'; additive: the ABI version stays 3) ----
 * ssr_conv_direct: exact-fp32 direct convolution, y = [relu](conv(x, w) + bias).  x is an NHWC fp32 view (SSR_F32 / SSR_F32X3
 *   storage) of N x Hi x Wi pixels of which the Cin channels from x.coff on are contracted; y an NHWC fp32 view of N x Ho x Wo pixels,
 *   Ho = (Hi + 2 pad - K) / stride + 1 (floor; Wo likewise), of which the Cout channels from y.coff on are written and no other.  w is
 *   ONE device array [K * K][Cin][Cout] of fp32 (tap ky * K + kx; the reference layout [Cout][Cin][K][K] permuted (2, 3, 1, 0) on the
 *   host; a layer with fewer input channels than the view, as the 3 of ssr_lpips_input's 8, pads Cin with ZERO weights), bias Cout
 *   floats or NULL.  Square odd kernels K <= 11, stride 1 .. 4, symmetric zero padding pad <= K / 2, Cin % 8 == 0, Cout % 32 == 0,
 *   both <= 512; any input grid with at least one output pixel, grids smaller than the kernel included.  Arithmetic:
 *   v_mfma_f32_32x32x2_f32, per output ONE fp32 accumulator chain over ky, kx, c ascending (tap rows wholly in the padding skipped),
 *   bias added last; no split of K, no atomics: two launches give the same bytes, and an image's bytes depend neither on N nor on the
 *   other images of the launch.  Both views 16-byte aligned (cs % 4 == 0, coff % 4 == 0), w 16-byte aligned.
 *   SSR_EINVAL: a null x, y or w, a size <= 0, pad < 0, Hi + 2 pad < K (or Wi), a view narrower than coff + channels or misaligned.
 *   SSR_EUNSUP: bf16 storage, K even or > 11, stride > 4, pad > K / 2, Cin % 8, Cout % 32, Cin or Cout > 512.  No launch in either case.
 * ssr_maxpool3s2_fwd: P[N, (H - 3) / 2 + 1, (W - 3) / 2 + 1, C] = maxpool 3x3 stride 2 of F[N, H, W, C], no padding, floor mode
 *   (trailing rows and columns that do not fill a window are dropped), after max(0, .) when relu != 0; fp32 NHWC views, 16-byte
 *   aligned as above; bit-exact (a NaN in a window gives NaN).  SSR_EINVAL: a null view, N or C <= 0, H or W < 3, a view narrower
 *   than coff + C or misaligned; SSR_EUNSUP: bf16 storage, C % 4 != 0.  No launch in either case. */
int ssr_conv_direct(ssr_view x, ssr_view y, const float* w, const float* bias, int32_t dtype, int32_t N, int32_t Hi, int32_t Wi,
                    int32_t Cin, int32_t Cout, int32_t K, int32_t stride, int32_t pad, int32_t relu, void* stream);
int ssr_maxpool3s2_fwd(ssr_view f, ssr_view p, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t relu, void* stream);

/* SSR_F32X3 weight gradients: split an fp32 buffer (n % 4 == 0 elements) into bf16 planes hi = bf16(x), lo = bf16(x - hi); the
 * bf16 wgrad kernel then accumulates (x_hi, dy_hi) + (x_hi, dy_lo) + (x_lo, dy_hi) into the fp32 gradient. */
int ssr_split_bf16(const float* x, void* hi, void* lo, int64_t n, void* stream);
/* the same for a device table of buffers in ONE launch (every n % 8 == 0, 16-byte aligned pointers; max_n = the largest n): what
 * engine.WgradBatch issues in front of the three split passes of a batch */
typedef struct ssr_split_item {
    const float* x;
    void* hi;
    void* lo;
    int64_t n;
} ssr_split_item;
int ssr_split_bf16_multi(const ssr_split_item* items_dev, int32_t n_items, int64_t max_n, void* stream);

/* ---- L2Model's networks: SRCNN and HighResNet (csrc/l2net.hip; additive: the ABI version stays 3) ----
 * What lies between the convolutions of ssr/archs/srcnn_arch.py and highresnet_arch.py.  The 3 x 3 reflect-padded convolutions
 * themselves (arch_util.py:89-96,105-112,229-236: padding='same', padding_mode='reflect') run through ssr_conv2d / ssr_conv2d_wgrad
 * with pad 0 over an (H+2) x (W+2) buffer whose border these kernels fill; their data gradient is the pad-2 full correlation onto
 * that grid.  SSR_F32 storage only; every view is 16-byte aligned (cs % 4 == 0, coff % 4 == 0) and C % 4 == 0.
 *
 * Image mapping (`group`, `fold`; 1, 1 = none): image n = b * group + r of the layer lands in image b * fold + r % fold of the output
 * buffer, at channels out.coff + (r / fold) * C.  fold 1: the revisits-as-channels view of SRCNN (srcnn_arch.py:183-185); fold =
 * half the revisits: torch.cat([first_half, second_half], dim=-3) of FusionBlock (arch_util.py:285-297).  Nothing is materialised.
 *
 * ssr_prelu_reflect_fwd (arch_util.py:100-102,116-118,171,240: PReLU, Dropout(0.5), x + DoubleConv(x)), per element, each step
 *   rounded to fp32 in this order:
 *       v = pre;  v = v > 0 ? v : a * v  (a = slope[0], read on the device);  mask: v = keep ? v * 2 : 0;  res: v = res + v
 *   written to pixel (y + out_pad, x + out_pad) of the [.., H + 2 out_pad, W + 2 out_pad, out.cs] buffer and, with out_pad = 1, to the
 *   border pixels that reflect it (edge not repeated: padded row 0 = interior row 1, padded row H + 1 = interior row H - 2), in the
 *   same launch.  mask: NULL or packed keep bits, bit (e & 31) of word (e >> 5) for element e = ((n H + y) W + x) C + c of `pre`.
 *   res: optional residual, [N, H + 2 res_pad, W + 2 res_pad, res.cs] read at the interior, image n (not mapped).
 * ssr_prelu_reflect_bwd: g (and the optional g2, the residual branch's gradient) are gradients laid out like `out` (own pad flags,
 *   the same image mapping).  Per element, fp32:  t = ONE running sum, started with its first term, of the interior sample and the
 *   border samples that reflected it, rows in increasing padded row index and, inside a row, columns in increasing padded column
 *   index (at most 3 x 3 terms, 2 x 2 where H, W >= 4), all of g's terms first, then g2's;  mask: t = keep ? t * 2 : 0;  dpre = pre > 0 ? t : a * t (0 counts as
 *   negative, as torch);  dslope[0] += sum over all elements of (pre > 0 ? 0 : pre * t): fp64 per-block partials in `partial`
 *   (SSR_L2_SLOTS doubles of scratch) added in block order by a second launch - no float atomics, the same bytes every run.
 * SSR_EINVAL without a launch: a null desc / pre / slope / out (fwd) / g, dpre, dslope, partial (bwd), N, C <= 0, H or W < 2, C % 4,
 *   a misaligned view, a view narrower than coff + C (out / g / g2: coff + ceil(group / fold) * C), group or fold < 1, N % group,
 *   a pad flag other than 0 | 1. */
#define SSR_L2_SLOTS 1024
typedef struct ssr_prelu_reflect_desc {
    int32_t N, H, W, C;
    ssr_view pre;
    const float* slope;
    const uint32_t* mask;
    int32_t group, fold;
    ssr_view out; int32_t out_pad;            /* forward */
    ssr_view res; int32_t res_pad;
    ssr_view g; int32_t g_pad;                /* backward */
    ssr_view g2; int32_t g2_pad;
    ssr_view dpre;
    float* dslope;
    double* partial;
    ssr_view tsum;                            /* optional [N, H, W, tsum.cs]: receives t before the mask (a chain of residual blocks
                                                 passes the total gradient of a block's output on to the block before it) */
} ssr_prelu_reflect_desc;
int ssr_prelu_reflect_fwd(const ssr_prelu_reflect_desc* d, void* stream);
int ssr_prelu_reflect_bwd(const ssr_prelu_reflect_desc* d, void* stream);
/* PixelShuffleBlock (arch_util.py:564-598) with sr_kernel_size 1: PixelShuffle(zoom), conv 1x1 Cm -> Cm (Cm = hidden / zoom^2), PReLU,
 * conv 1x1 Cm -> Cout, PReLU ('same' reflect padding of a 1 x 1 kernel pads nothing).  x: [N, H, W, hidden]; y, gy: [N, zoom H,
 * zoom W, cs] with Cout valid channels (the others are never written / read); the shuffle is an index computation:
 *       u[c] = x[n, Y / zoom, X / zoom, c zoom^2 + (Y % zoom) zoom + X % zoom]
 * w1 [Cm][Cm], b1 [Cm], s1 [1], w2 [Cout][Cm], b2 [Cout], s2 [1] as the state_dict holds them.  fp32 arithmetic, sums in channel order.
 * ssr_sr_tail_bwd recomputes the forward from x, writes dx [N, H, W, hidden] (every element exactly once) and ADDS the six parameter
 * gradients to dw1 .. ds2 (dx.cs must equal x.cs): per-block fp64 partials in `scratch`, added in block order by a second launch (no float atomics).
 * scratch: ssr_sr_tail_scratch_bytes() bytes, 16-byte aligned, nothing to zero.
 * SSR_EINVAL: a null pointer, a size <= 0, hidden % zoom^2, a view narrower than its channels; SSR_EUNSUP: Cm > 32 or Cout > 8. */
typedef struct ssr_sr_tail_desc {
    int32_t N, H, W, hidden, zoom, Cout;
    ssr_view x;
    const float *w1, *b1, *s1, *w2, *b2, *s2;
    ssr_view y;                               /* forward */
    ssr_view gy, dx;                          /* backward */
    float *dw1, *db1, *ds1, *dw2, *db2, *ds2;
    void* scratch;
} ssr_sr_tail_desc;
int ssr_sr_tail_fwd(const ssr_sr_tail_desc* d, void* stream);
int ssr_sr_tail_bwd(const ssr_sr_tail_desc* d, void* stream);
int64_t ssr_sr_tail_scratch_bytes(int32_t N, int32_t H, int32_t W, int32_t hidden, int32_t zoom, int32_t Cout);
/* Dropout(p = 0.5) keep bits (arch_util.py:102,118; torch's own stream is not reproduced, this generator is the promise):
 * Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (j & 0xffffffff, j >> 32, step[0], layer) gives words 4j .. 4j+3
 * of `bits`; n_words % 4 == 0.  step is a DEVICE counter (a captured launch replays with the current value); advance = 1 adds 1 to
 * it behind the mask launch (the last dropout site of a forward).  A null pointer, n_words <= 0 or n_words % 4: SSR_EINVAL. */
int ssr_dropout_mask(uint32_t* bits, int64_t n_words, uint64_t seed, int32_t* step, int32_t layer, int32_t advance, void* stream);
/* L2Model's pixel terms in one pass (ssr/models/ssr_l2_model.py:60-84 builds 0.3 mse + 0.4 mae + 0.3 ssim): over npix pixels with C valid
 * channels, d = a - b, n = npix C:  sums[0] += sum d^2 / n,  sums[1] += sum |d| / n  (fp64 per-block partials in `partial`,
 * SSR_L2_SLOTS x 2 doubles, added in block order by a second launch);  grad (optional) = w_mse * 2 d / n + w_l1 * sign(d) / n over the
 * C valid channels, written, not added.  ssr_ssim_loss then adds its term with accumulate = 1. */
int ssr_mse_l1_loss(ssr_view a, ssr_view b, ssr_view grad, int64_t npix, int32_t C, float w_mse, float w_l1, float* sums,
                    double* partial, void* stream);

/* ---- SelfAttentionBlock of OSMObjDiscriminator (ssr/archs/osm_obj_discriminator_arch.py:8-31; used at :51,:53,:76,:78) ----
 * NHWC fp32 views of Bo images of N tokens (token i = h * W + w: the reference's view(B, -1, W * H), :20-21,:25) and C channels,
 * dk = C / 8.  Weights as the state_dict holds them: wq, wk [dk][C] (query_conv / key_conv .weight, 1x1), wv [C][C], biases, gamma [1].
 * csrc/attention.hip; exact fp32 arithmetic (plain FMA) whatever the arithmetic mode of the network around it.
 *   ssr_self_attention_fwd (:16-31):  q = Wq x + bq, k = Wk x + bk, v = Wv x + bv;  e[i][j] = q_i . k_j;  a = softmax_j(e), max-subtracted;
 *       out_i = sum_j a[i][j] v_j;  y = fma(gamma, out, x).  With `save` set it also stores, per image, a [N][N], q [N][dk], k [N][dk],
 *       v [N][C], out [N][C] (ssr_self_attention_save_floats(N, C) floats per image): what the backward reads instead of recomputing.
 *   ssr_self_attention_bwd (autograd's backward of :16-31), from dy and the saved tensors: dx = dy + dq Wq + dk Wk + dv Wv (the residual
 *       path included), multiplied by relu'(x) = (x > 0) when relu_mask is set (x is the output of the ReLU at :75,:77: dx is then the
 *       gradient of that layer's pre-activation); and, when the seven gradient pointers are set (all or none), dWq, dbq, dWk, dbk, dWv,
 *       dbv, dgamma are ADDED to, summed over tokens and images in index order by one writer per element: no float atomics, two runs
 *       give the same bytes.  dbk is zero in exact arithmetic (a constant added to every key shifts a softmax row uniformly); what is
 *       added is rounding residue.  scratch: ssr_self_attention_scratch_floats(Bo, N, C) floats, nothing to zero.
 * SSR_EINVAL without a launch: a null descriptor or required pointer, Bo <= 0, C % 8 != 0, N not in {4, 8, 16, 32, 64}, a view that is
 * not 16-byte aligned (p, cs % 4, coff % 4) or narrower than coff + C, a weight matrix / save / scratch that is not 16-byte aligned,
 * some but not all gradient pointers.  SSR_EUNSUP: C % 32 != 0 or C > 256.  Nothing may alias except y == x. */
typedef struct ssr_attn_desc {
    int32_t Bo, N, C;
    ssr_view x;
    const float *wq, *bq, *wk, *bk, *wv, *bv, *gamma;
    ssr_view y;                               /* forward */
    float* save;                              /* forward: optional, written; backward: required, read */
    ssr_view dy, dx;                          /* backward */
    int32_t relu_mask;
    float *dwq, *dbq, *dwk, *dbk, *dwv, *dbv, *dgamma;
    float* scratch;
} ssr_attn_desc;
int ssr_self_attention_fwd(const ssr_attn_desc* d, void* stream);
int ssr_self_attention_bwd(const ssr_attn_desc* d, void* stream);
int64_t ssr_self_attention_save_floats(int32_t N, int32_t C);
int64_t ssr_self_attention_scratch_floats(int32_t Bo, int32_t N, int32_t C);
/* dst[p, c] = y[p, c] > 0 ? g[p, c] : 0 over C channels of npix pixels of three fp32 views: the gradient of a ReLU's pre-activation
 * from its output (torch.relu at osm_obj_discriminator_arch.py:79, whose input gradient arrives from outside the plan) */
int ssr_relu_bwd(ssr_view g, ssr_view y, ssr_view dst, int64_t npix, int32_t C, void* stream);

/* ---- object crops of OSMObjESRGANModel (ssr/models/osm_objs_esrgan_model.py:166-181): cut a box out of an image, resize it to
 *      SSR_OBJ_CROP x SSR_OBJ_CROP as torchvision.transforms.functional.resize does (bilinear, align_corners = False), and the
 *      transpose of that.  csrc/obj_crop.hip; plain fp32 FMA.
 * Tap rule, per axis of n_in source pixels, scale = n_in / 32: support = scale if antialias and scale >= 1, else 1; center =
 * scale * (i + 0.5); first = max(int(center - support + 0.5), 0); count = min(int(center + support + 0.5), n_in) - first;
 * w_j = max(0, 1 - |(j + first - center + 0.5) / support|), normalised to sum 1.  The 2-D weight is the product of the axes' weights.
 * boxes: DEVICE int32 [Bo][5] = (b, x1, y1, x2, y2), the crop being image b, rows y1 .. y2 - 1, columns x1 .. x2 - 1.  The kernels
 * read them from memory when they run: a captured graph replays with whatever the array holds then.  Because they are data, a bad
 * box cannot be a return code: a box that is empty, reaches outside [B, H, W] or has a side above SSR_OBJ_MAX_SIDE is REFUSED on the
 * device - its crop is written as zeros, it receives no gradient, and nothing is read or written through it.
 *   ssr_obj_crop_resize_fwd: src is an NHWC fp32 view of [B, H, W] pixels whose channels 0..2 (from src.coff) are read; dst an NHWC
 *       fp32 view of [Bo, 32, 32] pixels whose channels 0..2 receive the crop and 3..7 are written as 0 (the first object
 *       convolution reads 8 channels).
 *   ssr_obj_crop_resize_bwd: g is the crops' gradient (a view like dst; channels 0..2 read); dimg[b, y, x, c] += grad_scale * sum
 *       over the objects o of image b in index order, first[b] <= o < first[b + 1] (first: DEVICE int32 [B + 1]; an object whose box
 *       names another image is skipped), then over the outputs (oy, ox) in row-major order whose taps reach (y, x), for c = 0..2.  One
 *       writer per image pixel, no atomics: two runs give the same bytes.  Channels >= 3 and pixels no served box covers are not
 *       written at all.
 * dtype is the storage code of the views: SSR_F32 / SSR_F32X3 (fp32).  SSR_EUNSUP: SSR_BF16 (as the object branch), more than 65535
 * images or tile rows.  SSR_EINVAL without a launch: any other dtype, a null pointer, B, H, W or Bo <= 0, an image view that is not
 * 4-byte aligned or narrower than coff + 3, a crop view that is not 16-byte aligned (p, cs % 4, coff % 4) or narrower than coff + 8,
 * g aliasing dimg. */
#define SSR_OBJ_CROP 32
#define SSR_OBJ_MAX_SIDE 128
int ssr_obj_crop_resize_fwd(ssr_view src, int32_t dtype, int32_t B, int32_t H, int32_t W, const int32_t* boxes, int32_t Bo,
                            ssr_view dst, int32_t antialias, void* stream);
int ssr_obj_crop_resize_bwd(ssr_view g, const int32_t* boxes, const int32_t* first, int32_t Bo, ssr_view dimg, int32_t dtype,
                            int32_t B, int32_t H, int32_t W, float grad_scale, int32_t antialias, void* stream);

/* ---- The vision tower of the CLIPScore validation metric (csrc/vit.hip; `calculate_clipscore`: SigLIP ViT-SO400M-14, CLIP ViT-B/16;
 *      clipscore_metric.py; additive: the ABI version stays 3) ----
 * Every tensor is an fp32 ROW view: row i, channel c of view v is ((float*)v.p)[i * v.cs + v.coff + c], so a buffer can be a channel
 * slice of a wider one (q, k, v: three slices of one packed [rows, 3 C] buffer) or a strided row set (the class-token rows of a batch:
 * cs = T * C).  16-byte aligned (p, cs % 4 == 0, coff % 4 == 0) unless said otherwise.  dtype is the storage code: SSR_F32 / SSR_F32X3
 * (fp32); SSR_BF16: SSR_EUNSUP; any other code: SSR_EINVAL.  No float atomics and no split reductions: two launches give the same
 * bytes, and an image's bytes depend neither on the batch size nor on its place in the batch.  A refused call launches nothing.
 *
 * ssr_linear: Y[M, Nout] = act(X[M, K] W[Nout, K]^T + bias) (+ R).  w is a contiguous row-major [Nout][K] device array (16-byte
 *   aligned: what a state_dict's nn.Linear weight is; no packing step), bias Nout floats or NULL, r a view like y or a null view
 *   (r.p == NULL).  act: SSR_VIT_ACT_NONE | _QUICK_GELU (v / (1 + expf(-1.702 v))) | _GELU_TANH (0.5 v (1 + tanhf(sqrt(2 / pi) (v +
 *   0.044715 v^3)))) | _GELU_ERF (0.5 v (1 + erff(v / sqrt 2))), evaluated in fp32.  Arithmetic: v_mfma_f32_32x32x2_f32, per output ONE
 *   fp32 accumulator chain over k ascending (pairs (0, 1), (2, 3), ..), then the bias, then the activation, then the residual last,
 *   one fp32 rounding each.  Any M >= 1; K % 4 == 0 and Nout % 4 == 0 (SSR_EUNSUP otherwise, as M or Nout above 2^22); the tails of
 *   all three dimensions are masked: nothing outside X[M, K], W[Nout, K], R and Y[M, Nout] is read or written.  r may alias y (each
 *   element is read before it is written, by the same thread); x must not alias y.
 *   SSR_EINVAL: a null x, y or w, a size <= 0, an unknown act, a view narrower than its channels or misaligned.
 * ssr_layernorm_fwd: y[i, :] = (x[i, :] - mean_i) / sqrt(var_i + eps) * gamma + beta over C channels, biased variance; mean, then the
 *   sum of squared deviations from it, then the affine map are all formed in fp64 and the result rounded to fp32 once (rows with a
 *   large mean and a small variance lose nothing).  gamma, beta: C floats, 16-byte aligned.  y may alias x.
 *   SSR_EUNSUP: C % 4 != 0 or C > 2048.  SSR_EINVAL: a null pointer, rows or C <= 0, eps < 0, a bad view.
 * ssr_mha_fwd: y = softmax_j(q_i . k_j * scale) v per (image n, head h): q, y have N * Tq rows (row n * Tq + i), k, v N * Tk rows, and
 *   head h is channels h * d .. h * d + d - 1 of each view.  Max-subtracted softmax in fp32 (expf), plain fp32 FMA, the keys taken 64 at
 *   a time with a running maximum and sum, so any Tk works (K and V need not fit the LDS); Tq = 1 is the attention-pooling head.
 *   SSR_EUNSUP: d % 8 != 0 or d > 128, N or heads > 65535, Tq or Tk > 2^20.  SSR_EINVAL: a size <= 0, a NaN scale, a bad view.
 *   y must not alias q, k or v.
 * ssr_vit_patch_input: uint8 images u [N][H][W][3] -> the patch matrix y [N * grid^2, 3 p^2], row n * grid^2 + gy * grid + gx, column
 *   c * p^2 + py * p + px (the flattening of a patch-embedding weight [C, 3, p, p], so the embedding is ssr_linear):
 *       v = (float)u[n][rowidx[gy p + py]][colidx[gx p + px]][perm[c]] / 255.0f;   if (mean) v = (v - mean[c]) / std[c];
 *   every step rounded to fp32 (IEEE division; no fused multiply-add).  rowidx, colidx: DEVICE int32 [grid * p], the source row /
 *   column of every row / column of the resized image: the caller builds them by running the resize it wants to match (F.interpolate,
 *   mode 'nearest') over an index ramp, so the device restates no rounding rule.  An entry outside the image writes 0 and reads
 *   nothing.  perm (3 ints in 0 .. 2; {2, 1, 0} feeds an RGB image as BGR), mean, std (3 floats each, both or neither; std != 0) are
 *   host arrays copied into the launch.  y needs 3 p^2 channels.  SSR_EUNSUP: p > 64, grid > 1024.
 * ssr_vit_tokens: x[n T + t, :] = (t < ncls ? cls : e[n G + t - ncls, :]) + pos[t, :] over C channels, ncls = (cls != NULL), T = G +
 *   ncls; cls C floats or NULL, pos a contiguous [T][C] array; one fp32 addition.  C % 4 (SSR_EUNSUP otherwise).
 * ssr_cosine_pairs: f holds 2 N rows of E channels (rows 0 .. N - 1: the first image of every pair, N .. 2 N - 1: the second; 4-byte
 *   alignment is enough).  out[n] = dot / max(sqrt(na) * sqrt(nb), 1e-8) with dot, na, nb fp64 sums in index order of exact products:
 *   torch.nn.functional.cosine_similarity as torch <= 1.11 computes it; later versions clamp each norm on its own, which differs only
 *   for a norm below 1e-8 [recalled].  out: N doubles, 8-byte aligned. */
#define SSR_VIT_ACT_NONE 0
#define SSR_VIT_ACT_QUICK_GELU 1
#define SSR_VIT_ACT_GELU_TANH 2
#define SSR_VIT_ACT_GELU_ERF 3
int ssr_linear(ssr_view x, const float* w, const float* bias, ssr_view r, ssr_view y, int32_t dtype, int32_t M, int32_t K,
               int32_t Nout, int32_t act, void* stream);
int ssr_layernorm_fwd(ssr_view x, const float* gamma, const float* beta, ssr_view y, int32_t dtype, int32_t rows, int32_t C,
                      double eps, void* stream);
int ssr_mha_fwd(ssr_view q, ssr_view k, ssr_view v, ssr_view y, int32_t dtype, int32_t N, int32_t Tq, int32_t Tk, int32_t heads,
                int32_t d, float scale, void* stream);
int ssr_vit_patch_input(const uint8_t* u, int32_t N, int32_t H, int32_t W, const int32_t* rowidx, const int32_t* colidx,
                        int32_t grid, int32_t p, ssr_view y, int32_t dtype, const int32_t* perm, const float* mean,
                        const float* std, void* stream);
int ssr_vit_tokens(ssr_view e, const float* cls, const float* pos, ssr_view x, int32_t dtype, int32_t N, int32_t G, int32_t C,
                   void* stream);
int ssr_cosine_pairs(ssr_view f, int32_t dtype, int32_t N, int32_t E, double* out, void* stream);

/* ---- The tower's backward pass, for the CLIP loss of train.clip_opt (csrc/vit_bwd.hip; clip_loss.py; additive: the ABI version stays
 *      3) ----  Row views, dtype codes and the determinism rule as above.  Only the gradient with respect to the IMAGE is formed: the
 * linear data gradients dX = dY W are ssr_linear on a transposed weight copy, and there is no weight gradient.
 *
 * ssr_vit_float_input: as ssr_vit_patch_input for an fp32 NHWC image view img [N][H][W][img.cs] (4-byte aligned, any channel count >=
 *   coff + 3), of which channels coff + perm[c] are read:  v = img[n][rowidx[..]][colidx[..]][perm[c]];  if (mean) v = (v - mean[c]) /
 *   std[c].  There is no / 255: fed with (float)u / 255.0f (IEEE division) it gives ssr_vit_patch_input's bytes.  perm must be a
 *   permutation of {0, 1, 2} (SSR_EINVAL otherwise).
 * ssr_vit_float_input_bwd: its transpose in gather form.  rowrange [H][2], colrange [W][2] (DEVICE int32): the half-open range of
 *   rows / columns of the resized image that read source row / column i (clip_loss.nearest_inverse_ranges; an empty range: nothing
 *   reads it).  Ranges are clamped to 0 .. grid * p: rows and columns the patch matrix does not hold carry no gradient.  Per source
 *   element (n, y, x, c): the fp64 sum of dpatch over its rows, then columns, ascending, divided by std[c] (std == NULL: by nothing),
 *   rounded to fp32 once and ADDED to dimg[n][y][x][perm[c]] (one writer per element; other channels and prior content stay).
 * ssr_layernorm_bwd: x is the forward's input; mean and rstd are recomputed from it in fp64 as ssr_layernorm_fwd forms them.  With
 *   g = dy * gamma and xhat = (x - mean) rstd:  out = rstd (g - mean(g) - xhat mean(g xhat)) (+ r), formed in fp64 and rounded once;
 *   the residual r (optional, r.p == NULL: none) is one fp32 addition.  out may alias dy or r.  SSR_EUNSUP: C % 4 or C > 2048.
 * ssr_vit_act_fwd: post = act(pre), the very device function of ssr_linear's epilogue: ssr_linear with SSR_VIT_ACT_NONE followed by
 *   this pass gives the bytes of ssr_linear with `act` (without a residual).  ssr_vit_act_bwd: dpre = dpost * act'(pre) in fp32.  rows
 *   of C channels, C % 4 (SSR_EUNSUP otherwise); post may alias pre, dpre may alias dpost.
 * ssr_mha_bwd: the backward of ssr_mha_fwd for head dims 64 and 72 (SSR_EUNSUP otherwise), any Tq and Tk (Tq = 1: the pooling head).
 *   With S = q k^T scale, P = softmax(S), dP = dy v^T, delta_i = sum_j P_ij dP_ij, dS = P (dP - delta):  dv = P^T dy, dk = scale dS^T
 *   q, dq = scale dS k.  The softmax statistics are recomputed here (the running maximum and sum of the forward, over the same key
 *   tiles), nothing is taken from ssr_mha_fwd.  dq may be a null view (a query that is a parameter).  ws: ssr_mha_bwd_ws_floats(N, Tq,
 *   heads) = 3 N heads Tq floats of scratch (maximum, 1 / sum, delta per query row), written by the first launch and read by the second.
 *   dq comes from blocks that own 64 queries and walk the keys in order, dk and dv from blocks that own 64 keys and walk the queries
 *   in order.  dq, dk, dv must not alias an input.  SSR_EINVAL: a size <= 0, a NaN scale, a null ws, a bad view.
 * ssr_feature_l1: loss[0] += weight * mean|fx - fg| over B rows of E channels (4-byte aligned views), the sum of |fx - fg| formed in
 *   fp64 in index order by one thread;  dfx (optional) = weight / (B E) * sign(fx - fg), sign(0) = 0.  flags: 0 or SSR_DETERMINISTIC; one
 *   block and one writer either way, so the scalar lands in slot 0 of a slotted buffer.  B E <= 2^24 (SSR_EUNSUP beyond). */
int ssr_vit_float_input(ssr_view img, int32_t N, int32_t H, int32_t W, const int32_t* rowidx, const int32_t* colidx, int32_t grid,
                        int32_t p, ssr_view y, int32_t dtype, const int32_t* perm, const float* mean, const float* std, void* stream);
int ssr_vit_float_input_bwd(ssr_view dpatch, int32_t N, int32_t H, int32_t W, const int32_t* rowrange, const int32_t* colrange,
                            int32_t grid, int32_t p, ssr_view dimg, int32_t dtype, const int32_t* perm, const float* std, void* stream);
int ssr_layernorm_bwd(ssr_view x, const float* gamma, ssr_view dy, ssr_view r, ssr_view out, int32_t dtype, int32_t rows, int32_t C,
                      double eps, void* stream);
int ssr_vit_act_fwd(ssr_view pre, ssr_view post, int32_t dtype, int32_t rows, int32_t C, int32_t act, void* stream);
int ssr_vit_act_bwd(ssr_view pre, ssr_view dpost, ssr_view dpre, int32_t dtype, int32_t rows, int32_t C, int32_t act, void* stream);
int64_t ssr_mha_bwd_ws_floats(int32_t N, int32_t Tq, int32_t heads);
int ssr_mha_bwd(ssr_view q, ssr_view k, ssr_view v, ssr_view dy, ssr_view dq, ssr_view dk, ssr_view dv, float* ws, int32_t dtype,
                int32_t N, int32_t Tq, int32_t Tk, int32_t heads, int32_t d, float scale, void* stream);
int ssr_feature_l1(ssr_view fx, ssr_view fg, ssr_view dfx, int32_t B, int32_t E, float weight, float* loss, int32_t flags, void* stream);

/* ---- The tower linears on split operands (csrc/linear_split.hip; `tower_arithmetic: split` of train.clip_opt and of
 *      calculate_clipscore; additive: the ABI version stays 3) ----
 * ssr_linear_split: ssr_linear's product, Y[M, Nout] = act(X[M, K] W[Nout, K]^T + bias) (+ R), with the same views, epilogue order
 *   (bias, activation, residual last, one fp32 rounding each), shape rules (any M >= 1, K % 4 == 0, Nout % 4 == 0, M and Nout up to
 *   2^22, all three tails masked) and aliasing rules.  Only the contraction differs: every fp32 operand is two 16-bit pieces, hi =
 *   round16(v) and lo = round16(v - hi), and per group of 16 consecutive k the fp32 accumulator receives x_hi w_hi, then x_hi w_lo, then
 *   x_lo w_hi (v_mfma_f32_32x32x16_f16 / _bf16; x_lo w_lo is dropped), groups ascending: one fixed chain per output, no atomics, no
 *   split-K, so two launches give the same bytes and a row's bytes depend neither on M nor on the row's place.
 *   pieces = SSR_SPLIT_F16 (the forward): fp16 pieces, W multiplied by 2^SSR_F32H_WSHIFT before its split and the accumulator by
 *     2^-SSR_F32H_WSHIFT before the bias (the convolutions' SSR_F32H convention).  Domain |x| < 65504, |w| < 64: beyond it a piece is
 *     infinite and the output not finite.  Error against the exact product <= 2^-20 sum|x w| + 2^-25 sum|w| + 2^-35 sum|x|.
 *   pieces = SSR_SPLIT_BF16 (the data gradient dX = dY W, whose values of 1e-8 .. 1e-4 lie below fp16's range): bf16 pieces, no scale.
 *     Error <= 2^-16 sum|x w|.
 *   wpk: the packed weight, ssr_linear_split_pack_bytes(Nout, K) = 32 Nout ceil(K / 8) bytes, 16-byte aligned, written once by
 *   ssr_linear_split_pack from a contiguous row-major [Nout][K] fp32 device array with the SAME `pieces`:
 *       entry [n][kg], kg < ceil(K / 8), row-major, 32 bytes = [ 8 hi pieces of W[n][8 kg .. 8 kg + 7] | their 8 lo pieces ]
 *   (k >= K inside the last entry: zeros): each 16-byte half is one lane's MFMA operand, so the kernel stages entries into LDS as
 *   they are; X is split while it is staged.  Two packs of one matrix give the same bytes.
 *   SSR_EINVAL: a null x, y, w, wpk or out, a size <= 0, an unknown act or pieces, a view narrower than its channels or misaligned.
 *   SSR_EUNSUP: K % 4, Nout % 4, M or Nout above 2^22.  A refused call launches nothing. */
#define SSR_SPLIT_F16 1
#define SSR_SPLIT_BF16 2
int64_t ssr_linear_split_pack_bytes(int32_t Nout, int32_t K);
int ssr_linear_split_pack(const float* w, int32_t Nout, int32_t K, int32_t pieces, void* out, void* stream);
int ssr_linear_split(ssr_view x, const void* wpk, const float* bias, ssr_view r, ssr_view y, int32_t pieces, int32_t M, int32_t K,
                     int32_t Nout, int32_t act, void* stream);

/* ---- The tower's self-attention on the fp32-input matrix core (csrc/mha_mfma.hip; `tower_attention: mfma` of train.clip_opt and of
 *      calculate_clipscore; additive: the ABI version stays 3) ----
 * ssr_mha_mfma_fwd: ssr_mha_fwd's result, y = softmax_j(q_i . k_j * scale) v per (image, head), with the same views, row and head
 *   layout, max-subtracted softmax in fp32 (expf) and key tiles of 64 with a running maximum and sum (any Tq, Tk >= 1, tails masked:
 *   nothing outside the views is read or written).  Only the matrix products differ: q k^T and P v run on v_mfma_f32_32x32x2_f32, whose
 *   result is a k-ordered fp32 fmaf chain, so against ssr_mha_fwd only the order of the additions changes.  Head dims 64 and 72
 *   (SSR_EUNSUP otherwise; 72 is padded to 96 in registers on the output side, never in memory).  A block owns 128 queries.
 *   SSR_EUNSUP: a dtype other than F32, d not 64 or 72, N or heads > 65535, Tq or Tk > 2^20.  SSR_EINVAL: a size <= 0, a NaN scale, a
 *   bad view.  y must not alias q, k or v.
 * ssr_mha_mfma_bwd: ssr_mha_bwd's result, dS = P (dP - delta), dv = P^T dy, dk = scale dS^T q, dq = scale dS k, the statistics
 *   recomputed (nothing is taken from the forward), dq optionally a null view; q k^T, dy v^T, P^T dy, dS^T q and dS k on the same
 *   instruction, the softmax, its rescaling and delta on the vector unit in fp32.  Two launches as ssr_mha_bwd: blocks that own 128
 *   queries walk the keys (statistics, delta, dq), blocks that own 128 keys walk the queries (dk, dv).  ws:
 *   ssr_mha_mfma_bwd_ws_floats(N, Tq, heads) = 3 N heads Tq floats of scratch (maximum, 1 / sum, delta per query row), written by the
 *   first launch and read by the second.  dq, dk, dv must not alias an input.  Error codes as ssr_mha_bwd (a null ws: SSR_EINVAL).
 * Both: no atomics, one fixed order of additions per output (two launches give the same bytes), and an image's bytes depend neither
 *   on N nor on its place in the batch.  A refused call launches nothing. */
int ssr_mha_mfma_fwd(ssr_view q, ssr_view k, ssr_view v, ssr_view y, int32_t dtype, int32_t N, int32_t Tq, int32_t Tk, int32_t heads,
                     int32_t d, float scale, void* stream);
int64_t ssr_mha_mfma_bwd_ws_floats(int32_t N, int32_t Tq, int32_t heads);
int ssr_mha_mfma_bwd(ssr_view q, ssr_view k, ssr_view v, ssr_view dy, ssr_view dq, ssr_view dk, ssr_view dv, float* ws, int32_t dtype,
                     int32_t N, int32_t Tq, int32_t Tk, int32_t heads, int32_t d, float scale, void* stream);

/* ---- PNG decode on the device (csrc/png_decode.hip, csrc/png_inflate.h; `png_decode: device` of infer_grid; additive: the ABI
 *      version stays 3) ----
 * ssr_png_decode: n PNG images per launch, 8-bit grayscale (channels 1) or RGB (channels 3), not interlaced.  `streams` is one device
 *   buffer of streams_len bytes holding the images' zlib streams (the concatenated IDAT payloads; the host parses the container),
 *   `items` a device array: item i's stream is streams[src_off .. src_off + src_len), its pixels go to dst[dst_off .. dst_off + height
 *   width channels) as tight [H][W][C] bytes, and its raw scanlines (height (width channels + 1) bytes, ssr_png_scratch_bytes rounded
 *   to 16) may use scratch[raw_off ..).  Items' dst and scratch ranges must not overlap each other.  status[i] receives
 *       0 ok, 1 truncated input, 2 bad zlib header (CM, window, FDICT, FCHECK), 3 bad block type, 4 bad stored LEN/NLEN, 5 bad code
 *       lengths, 6 invalid symbol, 7 distance too far back, 8 output overrun (more than the raw image), 9 output short, 10 bad filter
 *       byte, 11 Adler-32 mismatch, 12 bad descriptor (the item does not fit streams_len / dst_len / scratch_len, a size outside 1 ..
 *       32768, channels not 1 or 3, more than 2^24 raw bytes: nothing of the item is read or written)
 *   and 0 is the only success.  Whatever the stream holds, an item reads only its stream and writes only inside its own dst and
 *   scratch ranges, and its decode ends: every step of the decoder consumes input or produces output.  A failed item's dst range
 *   holds unspecified bytes.  Stored, fixed and dynamic blocks, distances up to 32768 (the window is the raw image itself),
 *   incomplete code sets as zlib takes them (a single code of length 1; no distance code at all), over-subscribed sets refused.
 *   One wave per item; lds_pool (0 .. ssr_png_lds_pool_max()) is the LDS a block gets beyond its code tables: an item's stream is
 *   staged there when it fits and its raw scanlines live in the rest when they fit, otherwise global memory serves (same bytes
 *   either way).  Two launches on the same input give the same bytes.
 *   SSR_EINVAL: a null pointer, n <= 0, a negative length or lds_pool.  SSR_EUNSUP: n > 2^20, lds_pool above the maximum.  A refused
 *   call launches nothing.
 * ssr_png_decode_host: the same decoder (the same source text) on the CPU, every pointer a host pointer; the twin of the CPU tests.
 * ssr_stack_zero_scan: over B decoded stacks uint8 [T_b][32][32][3] at buf[offs[b] ..) (offs, T: device arrays), has_zero[b][t] = 1
 *   where frame t holds a zero sample, 0 where it does not and for t >= T_b (has_zero: uint8 [B][Tmax]; the rule of select_frames /
 *   format_s2naip_data).  A stack that does not lie inside buf_len, or with T_b > Tmax, reads nothing and gives zeros.
 * ssr_stack_gather: out uint8 [B][n][32][32][3] = frames frame_ids[b][k] of stack b, first uint8 [B][32][32][3] = frame 0 of every
 *   stack.  A frame id outside 0 .. T_b - 1 or a stack outside buf_len makes its copy a no-op.
 *   Both: SSR_EINVAL for a null pointer or a size <= 0, SSR_EUNSUP above 2^30 (stack, frame) pairs. */
typedef struct ssr_png_item {
    int64_t src_off, dst_off, raw_off;
    int32_t src_len, width, height, channels;
} ssr_png_item;
int64_t ssr_png_scratch_bytes(int32_t width, int32_t height, int32_t channels);
int32_t ssr_png_lds_pool_max(void);
int ssr_png_decode(const uint8_t* streams, int64_t streams_len, const ssr_png_item* items, int32_t n, uint8_t* dst, int64_t dst_len,
                   uint8_t* scratch, int64_t scratch_len, int32_t* status, int32_t lds_pool, void* stream);
int ssr_png_decode_host(const uint8_t* streams, int64_t streams_len, const ssr_png_item* items, int32_t n, uint8_t* dst, int64_t dst_len,
                        uint8_t* scratch, int64_t scratch_len, int32_t* status);
int ssr_stack_zero_scan(const uint8_t* buf, int64_t buf_len, const int64_t* offs, const int32_t* T, int32_t B, int32_t Tmax,
                        uint8_t* has_zero, void* stream);
int ssr_stack_gather(const uint8_t* buf, int64_t buf_len, const int64_t* offs, const int32_t* T, const int32_t* frame_ids, int32_t B,
                     int32_t n, uint8_t* out, uint8_t* first, void* stream);

/* library / device info: writes "gfx950 CUs=256 ..." style text */
int ssr_device_info(char* buf, int32_t buflen);
int ssr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SSR_HIP_H */
