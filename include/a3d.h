/*
 * a3d.h -- C ABI of liba3d_hip.so: the MI355X (gfx950) kernels of the PlaneRCNN per-frame
 * detection path of Articulation3D.
 *
 * The reference is pure Python on top of detectron2 / torchvision / torch operators; it has no FFI
 * of its own.  Each entry point below therefore names the reference call site (file:line under
 * /root/reference/articulation3d/articulation3d/, "pkg/") whose operator it replaces.  A maintainer
 * binds these with ctypes exactly as articulation3d_amd/_lib.py does.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name says host; no allocation inside; caller owns
 *     all buffers, workspaces are sized by the *_workspace_bytes helpers;
 *   - all activations are fp32 NHWC (channels innermost);
 *   - stream-ordered on `stream` (a hipStream_t passed as void*), re-entrant, no global state;
 *   - returns 0 (A3D_OK) or a negative error code; nothing is thrown.
 */
#ifndef A3D_H
#define A3D_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define A3D_OK 0
#define A3D_ERR_ARG (-1)
#define A3D_ERR_LAUNCH (-2)
#define A3D_ERR_UNSUPPORTED (-3)

#define A3D_ACT_NONE 0
#define A3D_ACT_RELU 1
#define A3D_ACT_LEAKY 2 /* slope 0.01, pkg/modeling/depth_net/depth_head.py:36 */

int a3d_version(void);
/* sizeof() of a descriptor struct, for bindings to verify their mirror of the layout.  id: 0 a3d_conv_desc, 1 a3d_rpn_desc,
 * 2 a3d_boxdet_desc, 3 a3d_roialign_desc, 4 a3d_paste_desc, 5 a3d_pack_desc, 6 a3d_wgrad_desc, 7 a3d_roialign_bwd_desc,
 * 8 a3d_match_desc, 9 a3d_rpn_loss_desc, 10 a3d_box_loss_desc, 11 a3d_roi_sample_desc, 12 a3d_sweep_desc, 13 a3d_transpose_item,
 * 14 a3d_axis_loss_desc, 15 a3d_mask_targets_desc, 16 a3d_mask_loss_desc, 17 a3d_plane_loss_desc,
 * 18 a3d_bn_train_desc, 19 a3d_depth_loss_desc, 20 a3d_pred_bwd_desc, 21 a3d_render_layer, 22 a3d_render_piece,
 * 23 a3d_render_desc, 24 a3d_mesh_desc, 25 a3d_eval_match_desc, 26 a3d_eval_ap_desc, 27 a3d_depth_l1_desc,
 * 28 a3d_eval_mask_counts_desc, 29 a3d_eval_plane_match_desc; 0 for an unknown id. */
size_t a3d_struct_size(int id);

/* ------------------------------------------------------------------------------------------------
 * Pre-processing.  Replaces PlaneRCNN.preprocess_image (pkg/modeling/meta_arch/planercnn.py:188-196)
 * + the HWC->CHW float cast of PlaneRCNN_Branch.inference (pkg/utils/arti_vis.py:58).
 * Output: [B,H,W,4] fp32, channel 3 = 0, value = (x - mean[c]) / std[c].
 * ---------------------------------------------------------------------------------------------- */
int a3d_preprocess_u8hwc(const uint8_t *frames /*[B,H,W,3]*/, float *out, int B, int H, int W,
                         const float mean[3], const float std[3], void *stream);
int a3d_preprocess_f32chw(const float *images /*[B,3,H,W]*/, float *out, int B, int H, int W,
                          const float mean[3], const float std[3], void *stream);

/* Input front end: frames of any size, uint8 HWC in the reader's channel order, to the detector's input in ONE
 * pass: `cv2.resize(im, (Wd, Hd))` (tools/inference.py:216; OpenCV's fixed-point INTER_LINEAR on uint8, the 2x2 INTER_AREA
 * switch at an exact 2x decimation, plain copy at equal sizes) + the RGB -> BGR flip `im[:, :, ::-1]` (:218, swap_rb = 1) +
 * float cast + (x - mean[c]) / std[c] (arti_vis.py:58, planercnn.py:188-196).  out [B,Hd,Wd,4] fp32 (channel 3 = 0), mean / std in
 * the OUTPUT channel order; out_u8 (optional) [B,Hd,Wd,3] = the resized frame in the source order (the reference's `frames` list). */
int a3d_preprocess_resize_u8(const uint8_t *frames /*[B,Hs,Ws,3]*/, float *out, uint8_t *out_u8, int B, int Hs, int Ws, int Hd, int Wd,
                             int swap_rb, const float mean[3], const float std[3], void *stream);

/* ------------------------------------------------------------------------------------------------
 * Fused convolution / linear as an fp32-MFMA implicit GEMM.
 * Replaces every Conv2d / Linear / ConvTranspose2d reached on the path:
 *   backbone + FPN + RPN head (planercnn.py:150,168 -> detectron2), box head (roi_heads.py:186-187),
 *   mask head (roi_heads.py:237), plane head (plane_head.py:71-80), axis head (axis_head.py:95-120),
 *   depth head (depth_head.py:32-46,80-87).
 *   y[m, n] = act( scale[n] * sum_k X[m, k] * w[n, k] + shift[n] + res[m, n] )
 * m = (b, oh, ow); k = (kh, kw, c) with c running over source 0 then source 1 (channel concat).
 * ---------------------------------------------------------------------------------------------- */
typedef struct a3d_conv_desc {
    const float *x;     /* source 0, NHWC [B,H,W,Cin]                                              */
    const float *x2;    /* optional source 1 [B,H,W,Cin2] concatenated after source 0, or NULL     */
    const float *w;     /* packed weights [Cout][Kpad], k = (kh*KW + kw)*(Cin+Cin2) + c            */
    const float *scale; /* [Cout] or NULL (=1)   -- folded BatchNorm scale                         */
    const float *shift; /* [Cout] or NULL (=0)   -- bias / folded BatchNorm shift                  */
    const float *res;   /* residual [B,Ho,Wo,Cout] (or [B,Ho/2,Wo/2,Cout] when res_ups) or NULL    */
    float *y;           /* [B,Ho,Wo,Cout]  (pixshuf: [B,2Ho,2Wo,Cout/4])                           */
    float *workspace;   /* split-K partials or the Winograd-domain input, a3d_conv_workspace_bytes(); may be NULL
                           if splitk == 1 and w_wino == NULL                                       */
    int B, H, W, Cin, Cin2;
    int Ho, Wo, Cout; /* Cout % 4 == 0 */
    int KH, KW, stride, pad;
    int Kpad;    /* row length of w in floats, multiple of 32, >= KH*KW*(Cin+Cin2)                  */
    int ups;     /* 1: the logical input is the nearest x2 upsampling of the sources (depth deconv) */
    int act;     /* A3D_ACT_*                                                                       */
    int res_ups; /* 1: residual is nearest x2 upsampled (FPN top-down add)                          */
    int pixshuf; /* 1: ConvTranspose2d k2 s2 as GEMM with columns (dy,dx,co) scattered to 2x2 blocks */
    int stem;    /* 1: x is [B,H,W,4] (a3d_preprocess_*), 7x7 s2 p3, w packed [Cout][7][8][4]        */
    int splitk;  /* >= 1; >1 writes partials to workspace and reduces in a second launch (precision 1: plain output rows
                    only -- no res_ups / pixshuf / phase --, splitk <= Kpad / 32)                        */
    const int *m_dev; /* optional DEVICE int: live row count (<= B*Ho*Wo); tiles past it exit at once,
                         so ragged per-ROI batches need no host synchronisation                      */
    int tune;         /* 0 = library picks the kernel variant; 1 = (the round-1 general kernel: removed in round 4, A3D_ERR_UNSUPPORTED);
                         2 = direct implicit GEMM even when w_wino is given; 5 / 6 = never / always use the persistent
                         pointwise kernel on eligible 1x1 layers; 7 = two-launch Winograd where the one-launch kernel would
                         run; precision 2: 8 = the narrow split-operand kernels (64-wide Winograd GEMM, 128 x 128 direct),
                         9 = the wide direct kernel whatever the problem size, 10 / 11 = its narrow kernel with 128 x 64 /
                         128 x 128 tiles, 12 = per-lane accumulator stores instead of the row-major epilogue through LDS (the
                         same bits; A/B runs); precision 3: 13 / 14 = always / never the activation-stationary pointwise kernel on an
                         eligible 1x1 layer (Cin 64 / 128 / 256, Cout % 128 == 0; the same bits); 17 = the small-grid pointwise kernel (one wave per
                         32 x 32 output tile, csrc/conv_sg_h2.hip; Cin % 64 == 0, Cout % 32 == 0) whatever the grid size -- tune 0 takes it for
                         launches of up to 1280 such tiles (single frames), 10 / 11 never (the same bits); 15 / 16 = the tap-outer / the patch-resident
                         form of a 3x3 s1 p1 layer (phase 5: every launch is patch-resident by default, 15 is the bit-equality link to
                         the four-launch form; phase 0: 16 forces the patch-resident kernel on a layer whose map its tiles fit badly;
                         the two forms reduce in different orders: equal to fp32 rounding, not bit for bit); Winograd layers: 23 = the
                         lockstep loop of the 128-tile fp16x2 GEMM instead of its ping-pong loop, 24 = 64-tile blocks (two workgroups per
                         CU), 25 (precision 2) = 128-tile blocks whatever the problem size -- all the same bits (A/B runs, equality tests);
                         precision 1 with w_bf16: 30 / 31 = the LDS-DMA kernel with 128- / 256-channel tiles whatever the size, 32 = never it;
                         33 / 34 = always / never the activation-stationary pointwise kernel (csrc/conv_bf16xs.hip) on a 1x1 layer it can
                         run (the same bits);
                         >= 100: explicit tile variant.
                         `tune` is the ONLY way to choose a variant: the library reads no environment variable and has no process-global
                         switch (developer builds with -DA3D_ABLATIONS excepted, see csrc/a3d_common.h). */
    int phase;        /* 0, or 1..4 = output phase (dy,dx) = ((phase-1)>>1, (phase-1)&1) of a 3x3 pad-1 convolution over a
                         nearest-x2 upsampled input, evaluated on the SOURCE grid as a 2x2 convolution with pre-summed
                         taps (KH = KW = 2, stride 1, pad ignored; taps read source rows oh-1+dy .. oh+dy): the four
                         phases write the interleaved pixels (2oh+dy, 2ow+dx) of y [B,2Ho,2Wo,Cout] -- 4/9 of the FLOPs
                         of convolving the upsampled tensor (depth decoder, depth_head.py:40-46).
                         5 = ALL FOUR phases in one launch (fp16x2 only, precision 3 with w_x3): KH = KW = 3, stride 1, pad 1 on
                         the source grid, Cout = 4 x the real channel count C (32 | C), y [B,2Ho,2Wo,C]; GEMM column
                         128 g + 32 p + c holds phase p = 2 dy + dx of output channel 32 g + c, its filter = that phase's
                         pre-summed 2x2 taps at rows kh - dy, columns kw - dx of the 3x3 neighbourhood (zero elsewhere;
                         scale / shift in the same column order).  The kernel skips the zero blocks: the 16 tap-phase
                         products of the four-launch form in the same order per output -- bit-identical -- with every
                         activation chunk loaded and split once for the phases that share it (round 3)                */
    const float *w_wino; /* optional Winograd-domain weights U = G g G^T, [16][Cout][Cin+Cin2] (3x3 s1 p1 only):
                            when given (and workspace holds a3d_conv_workspace_bytes) the layer runs as
                            F(2x2,3x3): 2.25x fewer MFMA cycles, same result within fp32 rounding           */
    const float *gate;   /* optional [B,Ho,Wo,Cout]: outputs are zeroed where gate <= 0 -- the ReLU backward of the
                            training step (section "Training step" below): y = dgrad(...) * (forward activation > 0).
                            Plain output layout only (no pixshuf / phase)                                     */
    int precision;       /* 0: fp32 MFMA (the inference / parity path).  1: bf16 MFMA with fp32 accumulation -- both operands
                            are rounded to bf16 (nearest-even) while they are staged in LDS, tensors stay fp32 in memory: the
                            arithmetic of torch.autocast(bfloat16), which the reference's training config asks for
                            (plain convolutions / linears only: no stem, ups, phase, pixshuf, concat, split-K).
                            2: fp32-grade on the bf16 pipe -- each fp32 operand is split EXACTLY into three bf16 terms in LDS and
                            six bf16 MFMAs per k step reproduce the fp32 product to 2^-24 relative (csrc/conv_bf16x3.hip);
                            same layer kinds as 1 plus the phase convs and their equal-width 2-source concat, Cin % 16 == 0.
                            Opt-in: the default everywhere is 0                                                  */
    const void *w_wino_x3; /* precision 2 on a Winograd layer: w_wino split into three bf16 planes, chunk-major
                            [16][(Cin+Cin2)/32][3][Cout][32] (a3d_split_bf16x3 with outer = 16, rows = Cout, cols = Cin+Cin2);
                            the layer then runs F(2x2,3x3) with the split-operand GEMM                                */
    const float *w_wino_cm; /* optional: the Winograd-domain weights chunk-major in the one-launch kernel's LDS-image order,
                            [Cin/8][16][ceil(Cout/64)][2 h][64 r][4 j] = w_wino[f][64 t + r][8 c + 4 h + j], zero for channels
                            past Cout (ops.winograd_weights_chunk_major).
                            With it a plain 3x3 s1 p1 layer (one source, no upsampling, precision 0, tune 0) runs
                            the ONE-launch Winograd kernel that transforms the input inside the GEMM loader
                            (csrc/conv_wino_fused.hip): no workspace, no 16-plane tensor in HBM                          */
    const void *w_x3;    /* optional, precision 2 on a direct (non-Winograd) layer: w split into three bf16 planes in 16-deep
                            chunk-major order [Kpad/16][3][Cout][16] (a3d_split_bf16x3_chunk with outer = 1, rows = Cout,
                            cols = Kpad, chunk = 16).  With it, wide and large layers run the 256 x 256-tile kernel that
                            moves the weight planes global -> LDS by LDS-DMA (csrc/conv_bf16x3_wide.hip); results are
                            bit-identical to the kernel that splits w on the fly                                       */
    /* ---- precision 3 ("fp16x2"): fp32-grade products from an exact-to-2^-22 two-way fp16 split of each operand, THREE fp16 MFMAs
     * per k step (csrc/conv_bf16x3.hip).  fp16 has 5 exponent bits, so every operand row is scaled by a power of two taken from the
     * largest magnitude of ITS image / ROI -- a frame's result never depends on what else is in the batch:                        */
    const float *in_amax;  /* DEVICE [B]: max |x[b]| (an upper bound is fine) per input image b; required at precision 3            */
    const float *in_amax2; /* DEVICE [B] for source 1 (x2), or NULL                                                                 */
    float *y_amax;         /* optional DEVICE [B], zero-initialised by the caller: the launch raises y_amax[b] to max |y[b]| (atomic
                              max; any precision of the split-operand kernels) so that the next layer has its in_amax for free      */
    float w_scale;         /* precision 3: power of two that puts max |w| (Winograd layers: max |w_wino|) in [2^14, 2^15)           */
    float *wino_m;         /* optional, precision 3 Winograd layers: a3d_wino_m_bytes() of scratch.  With it SMALL problems (a few
                              workgroups in the one-launch form: single frames, the coarsest pyramid levels) run plane-split: 16 x as
                              many workgroups each compute ONE Winograd plane's product into wino_m [16][tiles][Cout], and a second
                              launch folds the planes in the same order and applies the epilogue -- the same bits, a 16th of the
                              per-workgroup latency                                                                                 */
    int io_bf16;           /* precision 1 only (the training step's autocast arithmetic): which tensors are STORED as bf16 in HBM
                              instead of fp32 -- bit 0: x, bit 1: y, bit 2: res, bit 3: gate (x / y / res / gate then point at bf16
                              data).  The kernel rounds its operands to bf16 anyway, so a bf16 x gives the same products; y is
                              rounded to nearest even on the way out.  BASELINE configs[4]: bf16 activations and gradients.       */
    /* ---- precision 3 with the ACTIVATIONS pre-split by their producer (round 4): x_h2 replaces x (x may then be NULL).  Layout
     * [B,H,W][Cin/16][h | l][16] fp16 -- per pixel (or per row of a linear layer) and 16-channel chunk the two fp16 planes of
     * x * s(b), s(b) = the power of two that puts in_amax[b] in [2^14, 2^15): exactly the bits the loaders of the split-operand
     * kernels compute from the fp32 tensor, and the same bytes (2 + 2 per element).  Producers: a3d_roi_align_fpn with out_h2 (the
     * workgroup that pools a ROI knows the ROI's maximum before it stores) and a3d_presplit_f16x2 (one pass over a finished tensor).
     * The wide direct kernel then moves BOTH operands global -> LDS by LDS-DMA through a 4-stage ring: no activation registers, no
     * split arithmetic and no VGPR -> LDS stores in its loop; results are bit-identical to the launch on the fp32 tensor. */
    const void *x_h2;      /* source 0 pre-split, or NULL                                                                            */
    const void *x2_h2;     /* source 1 pre-split (required with x_h2 when Cin2 > 0), or NULL                                        */
    /* ---- phase 5 only (round 4): the layer's output feeds NOTHING but a 3x3 pad-1 convolution to ONE channel (the depth head's
     * depth_pred behind deconv5, pkg/modeling/depth_net/depth_head.py:51,88).  With dot_w / dot_y set the launch does not store its
     * [B,2H,2W,C] output (y may be NULL; C = Cout / 4 must be 64); it stores, per output pixel, the nine dot products of the pixel's
     * channel vector with the nine taps' weights, dot_y [B][9][2H][2W], and a3d_tapsum9 adds the shifted planes: a 177 MB round trip
     * instead of the 1.26 GB one (64 frames), one launch less.  Equal to the two launches to fp32 rounding of the 576-term sum. */
    const float *dot_w;    /* [9][C] = the one-channel filter as [kh][kw][c], or NULL                                                */
    float *dot_y;          /* [B][9][2H][2W], or NULL                                                                                */
    /* ---- Winograd layers, precision 3 (round 5): the layer's transformed tiles are a SLICE of a larger V buffer -- its tiles occupy
     * [wino_t_off, wino_t_off + tiles) of `wino_t_total` tiles per (plane, chunk, h | l) run of `workspace`.  0 / 0 = the layer's own
     * buffer.  Several layers that apply the SAME filter to different maps (the RPN head's 3x3 conv over the pyramid levels,
     * SURVEY K5) then transform into one buffer and a3d_wino_gemm_levels multiplies all of it in ONE launch. */
    int wino_t_off, wino_t_total;
    /* ---- precision 1 (round 5): the filter ALSO as bf16, [Cout][Kpad] in w's layout, rounded to nearest even from w (the training step keeps
     * fp32 master weights and rounds its flat parameter buffer once per step: a3d_f32_to_bf16_scaled).  With it large launches run the
     * kernel that moves both operands global -> LDS by LDS-DMA on 256-pixel tiles (csrc/conv_bf16w.hip); the products are those of the
     * kernel that rounds w on the fly: bit-identical results.  NULL: that kernel.  HBM-bound 1x1 layers (Cin 32 / 128 / 256 / 512, residual and
     * gate stored bf16 or absent) run csrc/conv_bf16xs.hip with it: a wave's 32 pixels stay in registers as MFMA fragments while the
     * workgroup walks every output channel -- again the same bits. */
    const void *w_bf16;
} a3d_conv_desc;

size_t a3d_conv_workspace_bytes(const a3d_conv_desc *d);
/* bytes of a3d_conv_desc.wino_m if this launch would use it (0: the problem is large enough for the one-launch form, or not a
 * precision-3 Winograd layer) */
size_t a3d_wino_m_bytes(const a3d_conv_desc *d);
int a3d_conv2d_nhwc_f32(const a3d_conv_desc *d, void *stream);
/* The ResNet stem in ONE launch (round 4, fp16x2 arithmetic): 7x7 s2 p3 convolution + folded FrozenBN + ReLU + 3x3 s2 p1 max-pool
 * (detectron2 BasicStem.forward behind pkg/modeling/meta_arch/planercnn.py:150).  d as for a3d_conv2d_nhwc_f32 on the stem (stem = 1,
 * precision 3, w_x3, in_amax, w_scale, Ho x Wo = the CONV output size) except that d->y / d->y_amax are the POOLED tensor
 * [B, (Ho - 1) / 2 + 1, (Wo - 1) / 2 + 1, 64] and its maxima.  Bit-identical to the conv launch followed by a3d_maxpool3x3s2_nhwc.
 * A3D_ERR_UNSUPPORTED: not that layer / arithmetic (the caller runs the two launches). */
int a3d_stem_conv_pool(const a3d_conv_desc *d, void *stream);
/* y[b][oh][ow] = bias + sum over t = 3 kh + kw of g[b][t][oh + kh - 1][ow + kw - 1] (zero outside): the second half of a 3x3 pad-1
 * convolution to one channel whose per-pixel tap products a phase-5 launch stored (a3d_conv_desc.dot_y). */
int a3d_tapsum9(const float *g, float bias, float *y, int B, int H, int W, void *stream);
/* src [outer][rows][cols] fp32 (cols % 32 == 0) -> dst [outer][cols/32][3][rows][32] bf16 with src == hi + mid + lo exactly
 * (round-to-nearest-even at each level). */
int a3d_split_bf16x3(const float *src, void *dst, int outer, int rows, int cols, void *stream);
/* The same with `chunk`-deep column chunks (16 or 32; cols % chunk == 0): dst [outer][cols/chunk][3][rows][chunk]. */
int a3d_split_bf16x3_chunk(const float *src, void *dst, int outer, int rows, int cols, int chunk, void *stream);
/* The fp16x2 counterpart (precision 3): src * scale == hi + lo (fp16, to 2^-22 relative); dst [outer][cols/chunk][2][rows][chunk]. */
int a3d_split_f16x2_chunk(const float *src, void *dst, int outer, int rows, int cols, int chunk, float scale, void *stream);
/* Activation pre-split for a3d_conv_desc.x_h2: x [B][n] fp32 (n % 16 == 0: pixels x channels of image b, channels % 16 == 0) ->
 * dst [B][n/16][h | l][16] fp16 of x * s(b), s(b) from amax[b] as the kernels derive it (a3d_conv_desc.in_amax); amax2 optional
 * (second source of a channel concat: both share max(amax[b], amax2[b])).  One HBM-bound pass, same byte count in and out. */
int a3d_presplit_f16x2(const float *x, void *dst, const float *amax, const float *amax2, int B, size_t n, void *stream);
/* out[b] = max(out[b], max |x[b, 0..n)|) for b < B (out zero-initialised by the caller): the in_amax of a tensor that no kernel of
 * this library produced. */
int a3d_absmax_rows(const float *x, float *out, int B, size_t n, void *stream);

/* The two launches of the Winograd form, individually (a3d_conv2d_nhwc_f32 issues both when d->w_wino is set):
 * x (+x2) -> d->workspace = V[16][tiles][Cin+Cin2]   (HBM-bound), then V, d->w_wino -> y   (MFMA-bound). */
int a3d_wino_input_transform(const a3d_conv_desc *d, void *stream);
int a3d_wino_gemm(const a3d_conv_desc *d, void *stream);
/* ONE GEMM launch for n <= 5 Winograd layers (precision 3) that share filter (w_wino_x3, w_scale, scale, shift, act), channel counts and
 * `workspace`, whose slices [wino_t_off, wino_t_off + tiles) are consecutive and fill wino_t_total: the shared-filter RPN conv over the
 * pyramid levels (StandardRPNHead, planercnn.py:168) as one launch over the concatenated tiles, with a per-level table for the output
 * maps, the per-image scales and the recorded maxima.  The partial rounds of the small levels vanish (p3-p6 at 64 frames: 5 + 2 + 1 + 1
 * rounds of the chip -> 6.25) and every output element is computed exactly as by its own launch: bit-identical. */
int a3d_wino_gemm_levels(const a3d_conv_desc *levels, int n, void *stream);
/* Back-to-back pointwise pair across a ResNet bottleneck boundary (round 6; detectron2 BottleneckBlock reached from
 * pkg/modeling/meta_arch/planercnn.py:29,150): d1 = conv3 + FrozenBN + residual + ReLU of block i, d2 = conv1 + FrozenBN + ReLU of block i + 1,
 * ONE launch.  d1 as for a3d_conv2d_nhwc_f32 on the activation-stationary fp16x2 kernel (1x1 stride 1, precision 3, w_x3, in_amax, w_scale,
 * res set, Cin 64 or 128); d2: 1x1 stride 1 over d1's output (Cin = d1->Cout, Cout 64 / 128 for d1->Cin 64 / 128), precision 2 with
 * w_x3 = its bf16x3 planes [Cin/16][3][Cout][16] (a3d_split_bf16x3_chunk), scale / shift / act, y, optional y_amax; no residual.
 * d1->y (and d1->y_amax) are stored exactly as the single launch stores them; d2->y equals a3d_conv2d_nhwc_f32(d2) on that tensor bit for
 * bit -- without reading it back from HBM.  A3D_ERR_UNSUPPORTED: not such a pair (issue the two launches). */
int a3d_conv_b2b(const a3d_conv_desc *d1, const a3d_conv_desc *d2, void *stream);
/* The kernel instantiation the LAST conv launch of the calling thread dispatched, as it appears in a rocprofv3 kernel trace
 * ("conv_pw_kernel<2,2,16> 128x128 persistent", "wino_gemm_kernel<1,32>", ...); "" before the first launch.  For measurement
 * code: launches are labelled with what the dispatcher did, not with a host-side copy of its selection rules.
 * This label is the library's one piece of state beside the per-device "dynamic LDS opted in" bits: a thread_local buffer, written and
 * read by the calling thread only (re-entrancy is not affected; it carries no configuration). */
const char *a3d_last_conv_variant(void);

/* Max-pool 3x3 stride 2 pad 1 (ResNet stem) and kernel-1 stride-2 pool (FPN LastLevelMaxPool = p6). */
int a3d_maxpool3x3s2_nhwc(const float *x, float *y, int B, int H, int W, int C, void *stream);
int a3d_subsample2_nhwc(const float *x, float *y, int B, int H, int W, int C, void *stream);

/* Bilinear resize, align_corners=False (depth_head.py:82,88). */
int a3d_resize_bilinear_nhwc(const float *x, float *y, int B, int H, int W, int C, int Ho, int Wo, void *stream);

/* 3x3 pad-1 convolution to ONE output channel (depth_head.py:68 depth_pred). w: [3][3][C], y: [B,H,W]. */
int a3d_conv3x3_to1_nhwc(const float *x, const float *w, float bias, float *y, int B, int H, int W, int C,
                         void *stream);

/* ------------------------------------------------------------------------------------------------
 * RPN proposal selection.  Replaces detectron2 RPN.predict_proposals / find_top_rpn_proposals reached
 * from planercnn.py:168 (anchor grid, Box2BoxTransform.apply_deltas, per-level top-k, clip, non-empty
 * filter, batched_nms with level as category, first post_topk): SURVEY.md A.4-A.6.
 * head[l]: [B, Hf, Wf, CH] fp32, channels [0,A) objectness logits, [A,5A) deltas (a*4+coord).
 * Outputs are fixed-size: slots >= out_count[b] are zero boxes / level -1.
 * ---------------------------------------------------------------------------------------------- */
typedef struct a3d_rpn_desc {
    const float *head[5];
    int Hf[5], Wf[5], stride[5];
    float cell_anchors[5][3][4]; /* per level, per anchor: x1,y1,x2,y2 around (0,0) */
    int B, L, A, CH;
    int img_h, img_w;
    int pre_topk, post_topk;
    float nms_thresh, min_size;
    float weights[4];
    float scale_clamp;
    void *workspace;    /* a3d_group_buffers_bytes(B*L) */
    float *out_boxes;   /* [B, post_topk, 4] xyxy */
    float *out_scores;  /* [B, post_topk] objectness logits */
    int *out_level;     /* [B, post_topk] */
    int *out_pos;       /* [B, post_topk] (level << 10) | rank-in-level : tie-break position */
    int *out_count;     /* [B] */
} a3d_rpn_desc;

size_t a3d_group_buffers_bytes(int n_groups);
/* bytes of a3d_rpn_desc.workspace: pre_topk <= 1024 (inference) equals a3d_group_buffers_bytes(B*L); up to 2048 (the
 * training configuration's PRE_NMS_TOPK_TRAIN 2000) adds the global suppression words of the 2048-candidate NMS. */
size_t a3d_rpn_workspace_bytes(int B, int L, int pre_topk);
int a3d_rpn_proposals(const a3d_rpn_desc *d, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Fast R-CNN box inference.  Replaces FastRCNNOutputLayers.inference reached from
 * pkg/modeling/roi_heads/roi_heads.py:206 (softmax, per-class apply_deltas, clip, score > thresh,
 * batched_nms with class as category, first topk): SURVEY.md A.8.
 * pred: [B*R, CH]: channels [0,C] class logits (C = background), [C+1, C+1+4C) per-class deltas.
 * ---------------------------------------------------------------------------------------------- */
typedef struct a3d_boxdet_desc {
    const float *pred;
    const float *prop_boxes; /* [B, R, 4] */
    const int *prop_count;   /* [B] */
    int B, R, C, CH;
    int img_h, img_w;
    float score_thresh, nms_thresh;
    int topk;
    float weights[4];
    float scale_clamp;
    void *workspace;   /* a3d_group_buffers_bytes(B*C) */
    float *out_boxes;  /* [B, topk, 4] */
    float *out_scores; /* [B, topk] */
    int *out_classes;  /* [B, topk] (-1 in unused slots) */
    int *out_pos;      /* [B, topk] proposal_row*C + class */
    int *out_count;    /* [B] */
} a3d_boxdet_desc;

int a3d_box_detections(const a3d_boxdet_desc *d, void *stream);

/* Greedy NMS over caller-sorted groups of <= 1024 boxes each (torchvision.ops.nms semantics, strict >).
 * g_boxes [G,1024,4] score-descending, g_valid [G,1024], g_n [G] -> g_keep [G,1024]. */
int a3d_group_nms(const float *g_boxes, const int *g_valid, const int *g_n, int *g_keep, int n_groups, float thresh,
                  void *stream);

/* ------------------------------------------------------------------------------------------------
 * ROIPooler: FPN level assignment + ROIAlign.  Replaces detectron2 ROIPooler / torchvision roi_align
 * built at pkg/modeling/roi_heads/roi_heads.py:50-55,74-79 and called at :185,:236,:250,:268
 * (SURVEY.md A.7).  feat[l]: NHWC [B,Hf,Wf,C]; boxes [B,R,4]; count[b] live boxes of image b (NULL = R).
 * Output row of box (b, r) = (row_offset ? row_offset[b] : b*R) + r, layout [row, P, P, C].
 * ---------------------------------------------------------------------------------------------- */
typedef struct a3d_roialign_desc {
    const float *feat[4];
    int Hf[4], Wf[4];
    float scale[4];
    int L, C;
    const float *boxes;
    const int *count;
    const int *row_offset;
    int B, R;
    int P, sampling_ratio, aligned;
    float *out;
    int *out_level; /* optional [rows] */
    int *order_ws;  /* optional [B*R] int32 workspace (R <= 1024): the library first sorts every image's live boxes by (level, y, x)
                       into it and walks them in that order, with each XCD taking whole images, so that workgroups running
                       side by side touch neighbouring feature cells (L2 hits instead of re-fetches).  The OUTPUT rows do not
                       move and the values are bit-identical to the unsorted walk: only the schedule changes. */
    float *out_amax; /* optional [rows]: max |pooled[row]| over the row's finite values, written by the workgroup that pools the
                        row (no atomics; rows of dead slots are not touched).  It is a3d_conv_desc.in_amax of the layers that consume
                        the pooled rows: every ROI is scaled by ITS OWN maximum (round 2 used a3d_roi_amax's level-wide bound, which
                        scaled a faint ROI by the hottest cell of its image). */
    const float *level_amax[4]; /* optional, with window_count: per level [B] = max |feat[l][b]| */
    int *window_count; /* optional: += number of live ROIs whose own maximum is below 2^-16 of their level's.  The backbone's per-image
                          block exponents leave every feature with an absolute error of ~2^-40 of its level's maximum; relative to
                          such a ROI that exceeds fp32's own rounding.  The default arithmetic counts these ROIs instead of passing
                          them silently (0 on every frame of the test and bench clips; A3D_PRECISION=2 is the remedy). */
    void *out_h2;      /* optional, INSTEAD of out (round 4; C == 256, P*P*C*4 <= 120 KiB: the 7x7 box pooler): the pooled rows pre-split
                          for the fp16x2 GEMM that consumes them, [rows][P*P*C/16][h | l][16] fp16 of pooled * s(row), s(row) = the
                          power of two that puts out_amax[row] in [2^14, 2^15) -- a3d_conv_desc.x_h2 of the box head's fc1
                          (roi_heads.py:185-187).  The workgroup keeps the row in LDS until its maximum is known.  Same pooled
                          values as `out` (the split is exact to 2^-22 of the row's maximum). */
    int serial;        /* walk of a ROI's cells.  0 = bin by bin, a bin's loads issued together.  1 = bin by bin, one load at a time (the
                          same bits as 0: schedule only; kept for the bit-equality test and tools/roi_bench.py).  2 (round 6; P = 7,
                          C = 256, `out`) = the rolling-window walk: a wave owns two adjacent bin rows and walks the ROI's cell
                          columns once -- 675 instead of 980 cell loads per typical ROI -- summing in (column, row) order: equal to
                          0 / 1 to fp32 rounding, not bit for bit; ROIs whose geometry does not fit (a bin without samples, bins
                          narrower than a cell, more than 8 cell rows per bin-row pair) take walk 0 -- a function of the ROI alone.
                          The Python layer passes 2 for the 7x7 box pooler (ops.ROI_ROLLING). */
} a3d_roialign_desc;

int a3d_roi_align_fpn(const a3d_roialign_desc *d, void *stream);

/* out[row of (b, r)] = max over the L levels of level_amax[l][b], for the live boxes r < count[b]: an upper bound of max |pooled[row]|
 * (rows as in a3d_roi_align_fpn).  Superseded on the detection path by a3d_roialign_desc.out_amax (the ROI's own maximum); kept for
 * callers that pool with their own kernel. */
int a3d_roi_amax(const float *const level_amax[4], int L, const int *count, const int *row_offset, int B, int R, float *out, void *stream);

/* offsets[b] = sum_{i<b} min(count[i], cap); offsets[B] = total.  (compacts ragged per-image ROI lists) */
int a3d_count_offsets(const int *count, int *offsets, int B, int cap, void *stream);

/* Skinny output layer: y[m, 0:N] = x[m, :] . w[n, :] + bias[n], N <= 8, with the first norm_n outputs
 * L2-normalised (F.normalize eps 1e-12) and/or sigmoid.  plane_head.py:80-82, axis_head.py:106-107,120,
 * Mask R-CNN predictor + sigmoid (roi_heads.py:237). */
int a3d_linear_small(const float *x, const float *w, const float *bias, float *y, int M, const int *m_dev, int K,
                     int N, int norm_n, int sigmoid, void *stream);

/* ------------------------------------------------------------------------------------------------
 * detector_postprocess + paste_masks_in_image + override_depth fused.  Replaces
 * pkg/modeling/postprocessing.py:47-69, pkg/layers/mask_ops.py:41-60,128-129 and
 * pkg/utils/arti_vis.py:90-99,125-149.  One slot per (image b, detection r < R).
 * ---------------------------------------------------------------------------------------------- */
typedef struct a3d_paste_desc {
    const float *boxes;      /* [B,R,4] pred_boxes */
    const float *scores;     /* [B,R] */
    const int *count;        /* [B] */
    const int *row_offset;   /* [B] compact row of (b,0) in mask_prob / normals */
    const float *mask_prob;  /* [rows, MS, MS] sigmoid mask probabilities */
    const float *normals;    /* [rows, 3] pred_plane unit normals, or NULL */
    const float *depth;      /* [B,H,W] or NULL */
    int B, R, MS, H, W;
    float post_score_thresh; /* 0.1, planercnn.py:217 */
    float mask_thresh;       /* 0.5, MODEL.ROI_MASK_HEAD.MASK_THRESHOLD */
    float focal, cx, cy;     /* 571.623718, 319.5, 239.5: arti_vis.py:101-104 */
    int clip_boxes;          /* 1: Boxes.clip to the image first (detector_postprocess, postprocessing.py:58);
                                0: paste with the boxes as given (bare paste_masks_in_image, mask_ops.py:68) */
    unsigned char *masks;    /* [B,R,H,W] 0/1 or NULL (mask never materialised) */
    float *planes;           /* [B,R,3] normal * offset (process()'s pred_plane) */
    int *area;               /* [B,R] */
    int *keep;               /* [B,R] survives score>=thresh and non-empty clip */
    float *out_boxes;        /* [B,R,4] clipped */
} a3d_paste_desc;

int a3d_paste_lsq(const a3d_paste_desc *d, void *stream);

/* Plane-offset least squares from dense masks of ONE image: PlaneRCNN_Branch.override_depth
 * (pkg/utils/arti_vis.py:125-149).  depth [H,W], masks [D,H,W] (non-zero = inside), normals [D,3] -> out [D,3]. */
int a3d_plane_offset_dense(const float *depth, const float *masks, const float *normals, float *out, int D, int H,
                           int W, float focal, float cx, float cy, void *stream);
/* The same with the pasted masks as they are (uint8 / bool bytes, non-zero = set): no float copy of the masks.  Identical results. */
int a3d_plane_offset_dense_u8(const float *depth, const unsigned char *masks, const float *normals, float *out, int D, int H, int W,
                              float focal, float cx, float cy, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Fixed-size detection records = payload of the frame-sharded all-gather.  One record
 * carries the fields create_instances() builds (pkg/utils/arti_vis.py:162-186):
 *   [0:4] box xyxy  [4] score  [5] class  [6:9] plane normal*offset  [9:12] rot axis  [12:14] tran axis
 *   [14:14+MS*MS] soft mask.   Kept detections of image b are compacted to records[b, 0:rec_count[b]].
 * ---------------------------------------------------------------------------------------------- */
typedef struct a3d_pack_desc {
    const float *boxes;     /* [B,R,4] clipped boxes (a3d_paste_lsq out_boxes) */
    const float *scores;    /* [B,R] */
    const int *classes;     /* [B,R] */
    const int *count;       /* [B] */
    const int *row_offset;  /* [B] */
    const int *keep;        /* [B,R] */
    const float *planes;    /* [B,R,3] or NULL */
    const float *rot_axis;  /* [rows,3] or NULL */
    const float *tran_axis; /* [rows,2] or NULL */
    const float *mask_prob; /* [rows,MS,MS] or NULL */
    int B, R, MS;
    float *records;         /* [B,R,a3d_record_floats(MS)] */
    int *rec_count;         /* [B] */
} a3d_pack_desc;

int a3d_record_floats(int MS);
int a3d_detections_pack(const a3d_pack_desc *d, void *stream);

/* COCO run-length encoding of pasted masks: the `segmentation` field of the reference's per-frame record
 * (pkg/utils/arti_vis.py:66-67 -> instances_to_coco_json -> pycocotools mask.encode; decoded again at :179-186).  masks [D,H,W] uint8
 * (non-zero = set), H * W <= 393 216.  pos[d, k] = the k-th COLUMN-major index i >= 1 with m[i] != m[i-1] (increasing), count[d] = how many
 * there are (only the first `cap` are stored: re-run with cap >= max count if it was exceeded), first[d] = m[0] != 0.  The run
 * lengths are the differences of {0, pos..., H*W}, with a leading 0 when first is set (cocoapi's convention). */
int a3d_mask_rle(const unsigned char *masks, int D, int H, int W, int cap, int *pos, int *count, int *first, void *stream);

/* ================================================================================================
 * Training step (BASELINE configs[4]: config/step1_bbox.yaml).
 * Replaces, under autograd, the training branch of PlaneRCNN.forward (pkg/modeling/meta_arch/planercnn.py:83-123),
 * the box branch of PlaneRCNNROIHeads.forward (pkg/modeling/roi_heads/roi_heads.py:93-117,190-204) and the SGD step
 * of the detectron2 trainer behind tools/train_net.py:84-117.  Data gradients of convolutions reuse
 * a3d_conv2d_nhwc_f32 with a3d_weight_transpose'd filters and the `gate` epilogue (ReLU backward).
 * ============================================================================================== */

/* dw[co][kh][kw][ci] (=/+=) scale[co] * sum_pixels dy[b,oh,ow,co] * x[b, oh*stride+kh-pad, ow*stride+kw-pad, ci]
 * (autograd's weight gradient of every Conv2d / Linear on the trainable path; dw has the packed forward layout). */
typedef struct a3d_wgrad_desc {
    const float *x;     /* forward input NHWC [B,H,W,Cin]                    */
    const float *dy;    /* gradient of the layer output [B,Ho,Wo,Cout]       */
    const float *scale; /* optional [Cout]: folded FrozenBN scale that followed the conv in the forward pass */
    float *dw;          /* [Cout][KH][KW][Cin]                               */
    float *workspace;   /* a3d_wgrad_workspace_bytes()                       */
    int B, H, W, Cin, Ho, Wo, Cout; /* Cin % 4 == 0, Cout % 4 == 0           */
    int KH, KW, stride, pad;
    int splitk;         /* >= 1 pixel slices (summed in slice order: deterministic) */
    int accumulate;     /* 1: dw += (weights shared by several call sites, e.g. the RPN head over 5 levels) */
    int precision;      /* 0: fp32 MFMA; 1: bf16 MFMA, fp32 accumulation; 2: fp32-grade 3-way bf16 split (see a3d_conv_desc.precision) */
    int io_bf16;        /* precision 1 only: bit 0: x is stored as bf16, bit 1: dy is stored as bf16 (dw stays fp32)              */
    int defer_reduce;   /* 1: launch the partial-sum kernel only; the caller keeps `workspace` alive and folds the slices of MANY layers
                           in one launch later (a3d_wgrad_reduce_batch).  Same sums in the same order: bit-identical dw.  Not with
                           accumulate (a chain of launches into one dw is ordered by its reduces).                                  */
    const int *p_dev;   /* optional DEVICE int: the live output-pixel count, a multiple of Ho*Wo and <= B*Ho*Wo (ragged per-ROI batches,
                           rows compacted to the front).  Pixels past it are never read; the `splitk` slices divide the LIVE pixels.
                           NULL, or a count equal to B*Ho*Wo, gives the bits of the full reduction.                                  */
} a3d_wgrad_desc;
size_t a3d_wgrad_workspace_bytes(const a3d_wgrad_desc *d);
int a3d_conv_wgrad_nhwc_f32(const a3d_wgrad_desc *d, void *stream);
/* Workgroup tiles of ONE pixel slice and the length of the pixel reduction of the kernel form the library runs this descriptor on (round 4: the
 * bf16 arithmetic has two forms -- csrc/conv_wgrad_tr.hip takes the stride-1 3x3 pad-1 and 1x1 layers with three taps / 256 input channels per
 * workgroup): what a caller sizes `splitk` by.  Returns the form (0: first form, 1 / 3: taps per workgroup of the second) or a negative error. */
int a3d_wgrad_tiles(const a3d_wgrad_desc *d, int *tiles, int *reduction);
/* The slice reduction of n deferred weight-gradient launches in ONE launch (round 4: at the reference's 2 images per GPU the 63 per-layer
 * reduce launches of a training step were 17 us of latency each, 11 % of the step).  table: DEVICE array of n a3d_wgrad_desc whose
 * workspace / scale / dw / Cout / KH / KW / Cin / splitk fields are read (x, dy are not).  Every layer: dw = scale * sum over slices
 * in slice order -- the arithmetic of the per-launch reduce.  tools/train_net.py:84-104 (the backward of DDP's step). */
int a3d_wgrad_reduce_batch(const a3d_wgrad_desc *table, int n, void *stream);

/* wt[ci][KH-1-kh][KW-1-kw][co] = scale[co] * w[co][kh][kw][ci]: the filter of the data gradient. */
int a3d_weight_transpose(const float *w, const float *scale, float *wt, int Cout, int KH, int KW, int Cin, void *stream);
/* The same for n filters in ONE launch: table = DEVICE array of n items.  The data-gradient filters of every trainable layer are
 * re-derived each step: 50 launches of ~6 us each at 2 images per GPU. */
typedef struct a3d_transpose_item {
    const float *w, *scale;
    float *wt;
    int Cout, KH, KW, Cin;
    int block0; /* first 32 x 32 x tap block of this filter in the launch's flat block index (exclusive prefix sum, filled by the caller) */
    int pad_;
} a3d_transpose_item;
int a3d_weight_transpose_batch(const a3d_transpose_item *table, int n, int total_blocks, void *stream);
/* U = G g G^T of a packed 3x3 filter [Cout][3][3][Cin] -> [16][Cout][Cin] (a3d_conv_desc.w_wino), on the device. */
int a3d_wino_weight_transform(const float *w, float *U, int Cout, int Cin, void *stream);

/* y [B,Ho,Wo,C] (=/+=) x [B,ceil(Ho/2),ceil(Wo/2),C] at even pixels, 0 elsewhere (backward of a3d_subsample2_nhwc and
 * of the input sub-sampling of a stride-2 1x1 convolution). */
int a3d_zero_insert2_nhwc(const float *x, float *y, int B, int H, int W, int C, int Ho, int Wo, int accumulate, void *stream);
/* y [B,H,W,C] += 2x2 block sums of x [B,2H,2W,C] (backward of the nearest-x2 upsampling of the FPN top-down path). */
int a3d_sumpool2_add_nhwc(const float *x, float *y, int B, int H, int W, int C, void *stream);
/* out[c] (=/+=) sum_m dy[m,c]  (bias gradients). */
size_t a3d_colsum_workspace_bytes(int C);
int a3d_colsum(const float *dy, float *out, float *workspace, int M, int C, int accumulate, void *stream);
/* dy stored as bf16 (the bf16 training step keeps its activation gradients that way): the same sums, in the same order, as a3d_colsum on
 * the widened values.  C % 4 == 0. */
int a3d_colsum_bf16(const void *dy, float *out, float *workspace, int M, int C, int accumulate, void *stream);
/* The same over the first *m_dev rows of dy only (m_dev: DEVICE int, <= M; ragged per-ROI batches): rows past it are never read, the
 * slices divide the live rows.  bf16: dy stored as bf16.  C % 4 == 0, dy 16-byte (bf16: 8-byte) aligned. */
int a3d_colsum_rows(const void *dy, int bf16, float *out, float *workspace, int M, const int *m_dev, int C, int accumulate, void *stream);

/* Axis loss of the articulation head's training stage (config/step2_axis.yaml; pkg/modeling/roi_heads/axis_head.py:95-201), forward AND
 * backward in one launch.  Rows are the compacted foreground ROIs [0, *live).  Per live row r: image row_img[r], matched ground truth
 * row_gt[r] -> gt_rot = gt_rot_axis[img][g] / gt_tran = gt_tran_axis[img][g], each [sin, cos, offset, valid].
 *   rot  = [normalize(raw_rot[r,0:2]), raw_rot[r,2]],   loss_rot  = W * mean over valid rows' 3 elements of smooth_l1(rot - gt_rot[0:3])
 *   tran = normalize(raw_tran[r,0:2]),                   loss_tran = W * mean over valid rows' 2 elements of
 *                                                                     smooth_l1(double_angle(tran) - double_angle(gt_tran[0:2]))
 * normalize: v / max(|v|, 1e-12) (F.normalize); double_angle(s, c) = (2sc, c^2 - s^2); valid: [3] >= 0.5; a loss whose valid column sums
 * below 1 is 0 with zero gradients (the reference's early return).  smooth_l1 with beta < 1e-5 is |x| (gradient sign(x), 0 at 0).
 * Outputs: loss[2] = (loss_rot, loss_tran); d_rot [rows,3] / d_tran [rows,2] = gradients of (loss_rot + loss_tran) with respect to the raw
 * rows, dead rows written as zeros.  One workgroup, fixed summation order, no atomics: bit-reproducible. */
typedef struct a3d_axis_loss_desc {
    const float *raw_rot;       /* [rows,rot_pitch]: rotation (2) | offset (1) */
    const float *raw_tran;      /* [rows,tran_pitch] */
    const int *live;            /* DEVICE int: live rows (<= rows) */
    const int *row_img;         /* [rows] */
    const int *row_gt;          /* [rows] */
    const float *gt_rot_axis;   /* [B, max_gt, 4] */
    const float *gt_tran_axis;  /* [B, max_gt, 4] */
    float *loss;                /* [2] */
    float *d_rot;               /* [rows,rot_pitch]: columns 3.. written as zeros */
    float *d_tran;              /* [rows,tran_pitch]: columns 2.. written as zeros */
    int rows;
    int rot_pitch, tran_pitch;  /* row pitch (floats) of raw_rot / d_rot (>= 3) and raw_tran / d_tran (>= 2) */
    int B, max_gt;
    float beta, loss_weight;
} a3d_axis_loss_desc;
int a3d_axis_loss(const a3d_axis_loss_desc *d, void *stream);

/* Mask head's training step (the mask share of config/step3_plane.yaml; detectron2 mask_rcnn_loss with bitmask ground truth), csrc/mask_train.hip.
 *
 * a3d_mask_targets: BitMasks.crop_and_resize(proposal_boxes, S) of the matched ground-truth mask per compact foreground row:
 *   targets[r] = ROIAlign((S, S), 1.0, sampling_ratio 0, aligned)(mask[b][row_gt[r]], box of row r) >= 0.5, uint8 0 / 1, fp32 arithmetic.
 * Half-pixel offset, no clamp of the box size, grid ceil(roi_h / S) x ceil(roi_w / S) per bin, divisor max(grid, 1), samples outside
 * [-1, H] x [-1, W] count as 0, the border rule of the pooler.  Row r belongs to image b with row_offset[b] <= r < row_offset[b + 1]; its box
 * is boxes[b][r - row_offset[b]].  A box without area (or not finite, or more than 32768 samples per bin on a side -- not a proposal of
 * any image) and a row whose slot / ground-truth index is out of range give an all-zero target.  Rows past *live are neither read nor
 * written.  No atomics, a fixed summation order: bit-reproducible. */
typedef struct a3d_mask_targets_desc {
    const uint8_t *masks;   /* [B, max_gt, H, W] 0 / non-zero */
    const float *boxes;     /* [B, cap, 4] */
    const int *count;       /* [B] live slots per image */
    const int *row_offset;  /* [B+1] exclusive prefix sum of count */
    const int *row_gt;      /* [rows] */
    const int *live;        /* DEVICE int: live rows (<= rows) */
    uint8_t *targets;       /* [rows, S, S] */
    int B, max_gt, H, W, cap, rows, S;
    int pad_;
} a3d_mask_targets_desc;
int a3d_mask_targets(const a3d_mask_targets_desc *d, void *stream);

/* a3d_mask_loss: the class-agnostic 256 -> 1 predictor, the mean BCE-with-logits and their backward pass in ONE pass over the deconv's
 * activation.  yu [rows, P, P, 4 * C]: the 2x2-stride-2 deconv's output after ReLU in UNSHUFFLED layout, channel (dy, dx, co) of input
 * pixel (iy, ix) = output pixel (2 iy + dy, 2 ix + dx), channel co.  Per live output pixel
 *   z = w . yu[pixel] + b,  t = targets[r][2 iy + dy][2 ix + dx],  loss += max(z, 0) - z t + log1p(exp(-|z|)),
 *   dz = (sigmoid(z) - t) / (*live * 4 P P),  dyu = dz * w * (yu > 0),  dw += dz * yu,  db += dz.
 * yu is read once and dyu written once; dw [C], db and the loss leave through per-workgroup partials (workspace) and a second launch
 * that sums them in a fixed order -- no atomics, the same bits on every run.  out = [dw (C) | db | loss].  *live == 0: loss 0 and every
 * gradient exactly 0.  Rows past *live are neither read nor written (dyu, z).  C == 256 (one wave, four channels per lane). */
typedef struct a3d_mask_loss_desc {
    const float *yu;         /* [rows, P, P, 4C] */
    const uint8_t *targets;  /* [rows, 2P, 2P] */
    const float *w;          /* [C] */
    const float *b;          /* [1] */
    const int *live;         /* DEVICE int */
    float *dyu;              /* [rows, P, P, 4C] */
    float *z;                /* [rows, 2P, 2P] logits, or NULL */
    float *out;              /* [C + 2]: dw | db | loss */
    float *workspace;        /* a3d_mask_loss_workspace_bytes() */
    int rows, P, C;
    int pad_;
} a3d_mask_loss_desc;
size_t a3d_mask_loss_workspace_bytes(void);
int a3d_mask_loss(const a3d_mask_loss_desc *d, void *stream);

/* Plane-normal head's training step (the plane share of config/step3_plane.yaml; pkg/modeling/roi_heads/plane_head.py:80-82, :96-124),
 * csrc/plane_train.hip.  a3d_plane_loss: the 1024 -> 3 predictor, F.normalize, plane_rcnn_loss and the backward pass of all three in ONE
 * pass over the FC's activation h [rows, K] (after ReLU).  Rows are the compacted foreground ROIs [0, *live), *live clamped to
 * [0, rows].  Per live row r with gt = gt_planes[row_img[r]][row_gt[r]]:
 *   raw = w . h[r] + b,  pred = raw / max(|raw|, 1e-12),  t = gt / max(|gt|, 1e-12)   (normal_only == 0: pred = raw, t = gt),
 *   loss = k sum |pred - t|,  k = loss_weight / *live  (an L1 SUM over rows and components divided by the ROW count),
 *   draw = backward of the normalisation of k sign(pred - t)  (sign 0 at 0; below the eps clamp no tangential term passes),
 *   dh[r] = (h[r] > 0) ? w^T draw : 0,  dw += draw x h[r],  db += draw.
 * A row whose row_img / row_gt is out of range contributes nothing to the loss or to any gradient (its dh row is written as zeros) and
 * still counts in the divisor.  h is read once and dh written once; dw, db and the loss leave through per-wave partials (workspace) and
 * a second launch that sums them in a fixed order -- no atomics, the same bits on every run.  out = [dw (3K) | db (3) | loss].
 * *live == 0: loss 0 and dw / db exactly 0.  Rows at or past *live are never read and their dh / raw never written.
 * K % 256 == 0 (A3D_ERR_ARG otherwise; K > 1024: A3D_ERR_UNSUPPORTED); h, dh, w and workspace 16-byte aligned. */
typedef struct a3d_plane_loss_desc {
    const float *h;          /* [rows, K] */
    const float *w;          /* [3, K] */
    const float *b;          /* [3] */
    const int *live;         /* DEVICE int */
    const int *row_img;      /* [rows] */
    const int *row_gt;       /* [rows] */
    const float *gt_planes;  /* [B, max_gt, 3] */
    float *workspace;        /* a3d_plane_loss_workspace_bytes(K) */
    float *out;              /* [3K + 3 + 1]: dw | db | loss */
    float *dh;               /* [rows, K] */
    float *raw;              /* [rows, 3]: the predictor's output before the normalisation, or NULL */
    int rows, K, B, max_gt;
    float loss_weight;
    int normal_only;
} a3d_plane_loss_desc;
size_t a3d_plane_loss_workspace_bytes(int K); /* 0 for a K the launch refuses as an argument error */
int a3d_plane_loss(const a3d_plane_loss_desc *d, void *stream);

/* Depth head's training step (the depth share of config/step3_plane.yaml; pkg/modeling/depth_net/depth_head.py:32-46, :80-89 and its
 * l1LossMask), csrc/depth_train.hip.  All tensors fp32 NHWC; no atomics, no host synchronisation: sums leave through per-workgroup
 * partials that a later launch folds in a fixed order, so every call gives the same bits.
 *
 * Training-mode BatchNorm2d over z [N = B H W, C], C 64 or 128, N >= 2 (anything else: A3D_ERR_ARG before any launch).
 * a3d_bn_train_forward (three launches): per workgroup (count, mean, M2 about that mean) over its rows, merged in partial order ->
 *   mean, var (BIASED), invstd = 1 / sqrt(var + eps);  y = act(gamma (z - mean) invstd + beta), act A3D_ACT_RELU or A3D_ACT_LEAKY;
 *   running_mean = (1 - momentum) running_mean + momentum mean, running_var likewise with the UNBIASED N / (N - 1) var (skipped when
 *   both are NULL).  The variance is never formed as E[z^2] - E[z]^2.
 * a3d_bn_train_backward (three launches: partial sums, their fold, apply): g = dy act'(y) (1 where y > 0, else 0 or 0.01),
 *   xh = (z - mean) invstd;  dgamma = sum g xh,  dbeta = sum g,  dz = gamma invstd (g - dbeta / N - xh dgamma / N).
 *   Row r of dy is read at dy + r dy_pitch + dy_off: a channel slice of a wider tensor (dy_pitch, dy_off multiples of 4).
 * z, y, dy, dz, workspace 16-byte aligned. */
typedef struct a3d_bn_train_desc {
    const float *z;         /* [N, C] the conv's output */
    const float *gamma;     /* [C] */
    const float *beta;      /* [C] */
    float *y;               /* [N, C]: forward output, backward input */
    float *mean;            /* [C]: forward output, backward input */
    float *invstd;          /* [C]: forward output, backward input */
    float *var;             /* [C] forward output or NULL */
    float *running_mean;    /* [C] updated in place by the forward call, or NULL */
    float *running_var;     /* [C] */
    const float *dy;        /* backward */
    float *dz;              /* [N, C] backward */
    float *dgamma;          /* [C] backward */
    float *dbeta;           /* [C] backward */
    float *workspace;       /* a3d_bn_train_workspace_bytes(N, C) */
    int N, C, act, dy_pitch, dy_off;
    float eps, momentum;
    int pad_;
} a3d_bn_train_desc;
size_t a3d_bn_train_workspace_bytes(int N, int C); /* 0 for a shape the launches refuse */
int a3d_bn_train_forward(const a3d_bn_train_desc *d, void *stream);
int a3d_bn_train_backward(const a3d_bn_train_desc *d, void *stream);

/* The masked L1 depth loss and its gradient with respect to the low-resolution prediction d [B, h, w] (depth_pred's output):
 *   pred = bilinear x2 of d (align_corners false, the arithmetic of a3d_resize_bilinear_nhwc, never stored),  mask = gt > 1e-4,
 *   out[0] = loss_weight sum |pred - gt| mask / max(sum mask, 1),  out[1] = sum mask,
 *   dd = the gradient of out[0]: each low-resolution pixel GATHERS sign(pred - gt) mask times its bilinear weight over its up to 4 x 4
 *   output pixels (sign 0 at a tie), then one more launch scales by loss_weight / max(sum mask, 1) from the device-side count.
 * Everything masked out: loss 0, gradient 0. */
typedef struct a3d_depth_loss_desc {
    const float *d;    /* [B, h, w] */
    const float *gt;   /* [B, 2h, 2w] */
    float *dd;         /* [B, h, w] */
    float *out;        /* [2]: loss | live pixel count */
    float *workspace;  /* a3d_depth_loss_workspace_bytes() */
    int B, h, w;
    float loss_weight;
} a3d_depth_loss_desc;
size_t a3d_depth_loss_workspace_bytes(void);
int a3d_depth_loss(const a3d_depth_loss_desc *d, void *stream);

/* Backward of a3d_conv3x3_to1_nhwc (C = 64): x [B, H, W, 64], g [B, H, W] the gradient of its output, w [9, 64] (tap-major) ->
 * dx [B, H, W, 64], out = [dw (9 x 64, tap-major) | db].  x read once, dx written once; dw / db through per-workgroup partials. */
typedef struct a3d_pred_bwd_desc {
    const float *x;
    const float *g;
    const float *w;
    float *dx;
    float *out;        /* [9 * 64 + 1] */
    float *workspace;  /* a3d_pred_bwd_workspace_bytes() */
    int B, H, W, C;
} a3d_pred_bwd_desc;
size_t a3d_pred_bwd_workspace_bytes(void);
int a3d_depth_pred_backward(const a3d_pred_bwd_desc *d, void *stream);

/* out[b, 2y + i, 2x + j, :] = cat(a[b, y, x, :], b2[b, y, x, :]), i, j in {0, 1}: the dense input of a deconv block's weight gradient
 * (nearest x2 upsampling of the channel concat).  Ca, Cb multiples of 4. */
int a3d_ups2_concat(const float *a, const float *b2, float *out, int B, int H, int W, int Ca, int Cb, void *stream);

/* Gradient of a3d_resize_bilinear_nhwc with respect to its input: dx [B, H, W, C] = gather of dy [B, Ho, Wo, C] (every input pixel
 * collects the output pixels that read it, in output order).  C % 4 == 0; meant for the decoder's one small resize. */
int a3d_resize_bilinear_backward_nhwc(const float *dy, float *dx, int B, int H, int W, int C, int Ho, int Wo, void *stream);

/* Gradient of a3d_roi_align_fpn with respect to the pyramid: dfeat[level] += scatter(dout).  dfeat must hold the
 * gradient accumulated so far (or zeros).  Adaptive sampling (sampling_ratio 0) only: the box pooler. */
typedef struct a3d_roialign_bwd_desc {
    float *dfeat[4];
    int Hf[4], Wf[4];
    float scale[4];
    int L, C;
    const float *boxes;    /* [B,R,4] */
    const int *count;      /* [B] or NULL */
    const int *row_offset; /* [B] or NULL */
    int B, R, P, sampling_ratio, aligned;
    const float *dout;     /* [rows,P,P,C] */
} a3d_roialign_bwd_desc;
int a3d_roi_align_fpn_backward(const a3d_roialign_bwd_desc *d, void *stream);
/* The same gradient WITHOUT atomics (round 4): the pyramid in 8 x 8-cell tiles, a bit per (image, tile, ROI slot) marked by a first launch,
 * one workgroup per tile that sums its ROIs in slot order in LDS and adds the tile to dfeat once -- bit-reproducible, ~8 x fewer bytes
 * to memory.  workspace: a3d_roi_align_bwd_workspace_bytes(d) bytes (zeroed by the call). */
size_t a3d_roi_align_bwd_workspace_bytes(const a3d_roialign_bwd_desc *d);
int a3d_roi_align_fpn_backward_gather(const a3d_roialign_bwd_desc *d, void *workspace, void *stream);

/* detectron2 Matcher over pairwise_iou(gt, boxes) (RPN.label_and_sample_anchors, ROIHeads.label_and_sample_proposals):
 * matched_idx[b,i] = argmax_g IoU (first maximum), label[b,i] = labels[k] for IoU in [thresholds[k-1], thresholds[k]),
 * and with allow_low_quality every box attaining some gt's best IoU gets label 1.  Images without gt: labels[0]. */
typedef struct a3d_match_desc {
    const float *boxes;     /* [*, N, 4]; image b reads boxes + b*box_batch_stride*4 (stride 0: shared anchors) */
    const int *box_count;   /* [B] live boxes per image or NULL (= N) */
    const float *gt_boxes;  /* [B, Gmax, 4] */
    const int *gt_count;    /* [B] */
    int B, N, Gmax, box_batch_stride;
    float thresholds[2];
    int labels[3];
    int n_thresholds;       /* 1 or 2 */
    int allow_low_quality;
    unsigned int *gt_best;  /* scratch [B, Gmax] (allow_low_quality only) */
    int *matched_idx;       /* [B, N] */
    signed char *label;     /* [B, N] */
    float *matched_iou;     /* [B, N] or NULL */
} a3d_match_desc;
int a3d_match_boxes(const a3d_match_desc *d, void *stream);

/* detectron2 subsample_labels on the device (RPN._subsample_labels): out[b,i] = 1 / 0 for a uniformly random subset of
 * at most max_pos positives (label 1) and negatives (label 0) up to `num` in total, -1 elsewhere.  Counter-based RNG:
 * the subset is a function of (seed, b, i) only.  N < 2^17. */
int a3d_sample_labels(const signed char *labels, signed char *out, int B, int N, int num, int max_pos, unsigned long long seed,
                      void *stream);

/* add_ground_truth_to_proposals: out [B, R+Gmax, 4] = [live proposals | ground truth | zeros], out_count = both counts. */
int a3d_append_gt_boxes(const float *props, const int *count, const float *gt, const int *gt_count, float *out, int *out_count,
                        int B, int R, int Gmax, void *stream);

/* ROIHeads._sample_proposals + the gathers that follow it (roi_heads.py:93-95 -> detectron2 label_and_sample_proposals):
 * class of box i = gt_classes[matched_idx[i]] if match_label[i] == 1 else num_classes (background; also when the image
 * has no ground truth); keeps a random subset of <= max_fg foreground boxes and background boxes up to `num`;
 * outputs are fixed-size [B, num] (foreground first), slots >= out_count[b] are zero boxes of the background class. */
typedef struct a3d_roi_sample_desc {
    const float *boxes;        /* [B, N, 4] (a3d_append_gt_boxes output) */
    const int *box_count;      /* [B] */
    const float *gt_boxes;     /* [B, Gmax, 4] */
    const int *gt_classes;     /* [B, Gmax] */
    const int *gt_count;       /* [B] */
    const int *matched_idx;    /* [B, N] (a3d_match_boxes) */
    const signed char *match_label; /* [B, N] */
    int B, N, Gmax, num_classes, num, max_fg;
    unsigned long long seed;
    float *out_boxes;          /* [B, num, 4] */
    float *out_gt_boxes;       /* [B, num, 4] */
    int *out_classes;          /* [B, num] */
    int *out_index;            /* [B, num] index into boxes, -1 for unused slots */
    int *out_count;            /* [B] */
} a3d_roi_sample_desc;
int a3d_sample_rois(const a3d_roi_sample_desc *d, void *stream);

/* RPN.losses + its gradient with respect to the head outputs (layout of a3d_rpn_desc.head).  loss[0] = loss_rpn_cls,
 * loss[1] = loss_rpn_loc.  labels: -1 ignore, 0 negative, 1 positive AFTER sub-sampling; anchor order: level-major,
 * then (y, x, a). */
typedef struct a3d_rpn_loss_desc {
    const float *head[5];
    float *dhead[5];
    int Hf[5], Wf[5], stride[5];
    float cell_anchors[5][3][4];
    int B, L, A, CH, Atotal, Gmax;
    const signed char *labels; /* [B, Atotal] */
    const int *matched_idx;    /* [B, Atotal] */
    const float *gt_boxes;     /* [B, Gmax, 4] */
    float weights[4];          /* Box2BoxTransform weights (1,1,1,1) */
    float normalizer;          /* RPN.BATCH_SIZE_PER_IMAGE * images */
    float *workspace;          /* a3d_loss_workspace_bytes() */
    float *loss;               /* [2] */
} a3d_rpn_loss_desc;
size_t a3d_loss_workspace_bytes(void);
int a3d_rpn_loss(const a3d_rpn_loss_desc *d, void *stream);

/* FastRCNNOutputLayers.losses + gradient with respect to the fused predictor output rows:
 * pred[r] = [K+1 class scores (K = background) | 4K deltas, class-major | padding up to pitch].
 * loss[0] = loss_cls (mean cross entropy), loss[1] = loss_box_reg (L1 on foreground rows / M). */
typedef struct a3d_box_loss_desc {
    const float *pred;     /* [M, pitch] */
    float *dpred;          /* [M, pitch] */
    const int *gt_classes; /* [M] in [0, K] */
    const float *boxes;    /* [M,4] sampled proposal boxes */
    const float *gt_boxes; /* [M,4] matched ground truth (unused for background rows) */
    int M, num_classes, pitch;
    float weights[4];      /* (10,10,5,5) */
    float *workspace;      /* a3d_loss_workspace_bytes() */
    float *loss;           /* [2] */
    const int *count;      /* optional [M / R]: rows are R per image and only the first count[b] of image b are live; the
                              others get zero gradient and the losses are normalised by the live row count.  NULL: all live */
    int R;
} a3d_box_loss_desc;
int a3d_box_loss(const a3d_box_loss_desc *d, void *stream);

/* torch.optim.SGD (momentum, weight decay) over a flat buffer; n % 4 == 0.
 * d = grad_scale*g + wd*p;  buf = first ? d : momentum*buf + d;  p -= lr*buf */
int a3d_sgd_momentum(float *p, const float *g, float *buf, size_t n, float lr, float momentum, float wd, float grad_scale,
                     int first, void *stream);
/* The same update with the gradient read as bf16 (the all-reduced bf16 payload where the collective left it: tools/train_net.py:110's
 * DDP with bf16_compress_hook widens into .grad first; widening is exact, so the result equals a3d_bf16_to_f32 + a3d_sgd_momentum bit
 * for bit, minus one pass over the flat buffer). */
int a3d_sgd_momentum_bf16g(float *p, const void *g_bf16, float *buf, size_t n, float lr, float momentum, float wd, float grad_scale,
                           int first, void *stream);

/* bf16 payload of the data-parallel gradient all-reduce (BASELINE configs[4]; torch DDP's bf16_compress_hook behind
 * tools/train_net.py:110): dst_bf16[i] = bf16(src[i] * scale) (round to nearest even; scale = 1 / world size), and the widening
 * back after the collective.  n % 4 == 0. */
int a3d_f32_to_bf16_scaled(const float *src, void *dst_bf16, size_t n, float scale, void *stream);
int a3d_bf16_to_f32(const void *src_bf16, float *dst, size_t n, void *stream);

/* ================================================================================================
 * Hypothesis sweeps of the temporal optimiser.  Replace the per-hypothesis / per-frame Python loops
 * inside optimize_planes_3dc and optimize_planes_3d_trans (pkg/utils/opt_utils.py:400-476, 540-611, 700-768, 838-905):
 * lift a mask onto its plane (get_pcd, pkg/utils/vis.py:86-102), apply every rigid hypothesis, re-project
 * (project2D, vis.py:62-83) into one binary mask per hypothesis, IoU against the tracked detections' masks.
 * Masks are bit-packed: words = ceil(H*W/32), bit i of word w = pixel 32w+i (row-major).
 * ============================================================================================== */
#define A3D_SWEEP_MAX_HYP 64
int a3d_masks_pack_bits(const unsigned char *masks /*[n,H,W], non-zero = set*/, unsigned int *bits /*[n,words]*/, int n, int H, int W,
                        void *stream);
int a3d_masks_unpack_bits(const unsigned int *bits, unsigned char *masks /*[n,H,W] 0/1*/, int n, int H, int W, void *stream);

typedef struct a3d_sweep_desc {
    const unsigned char *mask; /* [H,W] source mask (pred_mask.nonzero())                                     */
    int H, W;
    float normal[3];           /* unit plane normal in the optimiser's camera frame ((a,b,c) -> (a,-c,b) swap)  */
    float offset;              /* plane offset = |plane|                                                     */
    double focal, cx, cy;      /* vis.py intrinsics: 517.97, W/2, H/2                                          */
    float pivot[3];            /* point the rotations turn about (a 3-D point of the axis); 0 for translations */
    const float *xforms;       /* [A][12]: R (row-major 3x3) then t; point' = R (point - pivot) + pivot + t      */
    int A;                     /* hypotheses, <= A3D_SWEEP_MAX_HYP                                             */
    unsigned int *out_bits;    /* [A, words], cleared by the call                                              */
} a3d_sweep_desc;
int a3d_project_hypotheses(const a3d_sweep_desc *d, void *stream);

/* iou[f*A + a] = |target_f & proj_a| / |target_f | proj_a|  (opt_utils.py:470-475). */
int a3d_mask_iou_matrix(const unsigned int *target_bits /*[F,words]*/, const unsigned int *proj_bits /*[A,words]*/, float *iou, int F,
                        int A, int H, int W, void *stream);

/* ================================================================================================
 * The clip's visualisation panels (the reference's output.mp4 row, tools/inference.py:230-276): per frame a "seg" panel
 * (the frame with box outlines and articulation-axis arrows blended over it) and a surface-normal panel, in one launch
 * over tables the host builds once per clip (articulation3d_amd/render.py).  Everything is on the device.
 *
 * The law (held bit for bit by tests/render_ref.py):
 *   seg panel     start from the frame's pixel; apply the frame's layers [layer_off[f], layer_off[f+1]) in table order.
 *                 A layer covers a pixel at most once, however many of its pieces do; where it does, every channel
 *                 becomes (old*(256-alpha) + color*alpha + 128) >> 8.
 *                 MASK layer: covered = the mask bit.  POLY layer: covered = OR over its pieces; inside a piece iff
 *                 e >= 0 for each of its n half-planes, px = x + 0.5f, py = y + 0.5f, e = (A*px + B*py) + C in fp32,
 *                 in that order, no contraction.  The cull boxes (a layer's, a piece's) are supersets of the coverage and
 *                 never change it.
 *   normal panel  n = sum_i bit_i * normal_i (component-wise, fp32, the frame's instances [inst_off[f], inst_off[f+1]) in
 *                 ascending order); v = (n + 1.0f) / 2.0f * 255.0f; byte = low 8 bits of v truncated toward zero to
 *                 int32.  For v in [0, 256) and at most two overlapping masks that is get_normal_map (arti_vis.py:203-215:
 *                 matmul of the 0/1 masks with F.normalize(plane), astype(uint8)); the wrap outside that range is this
 *                 library's choice (numpy leaves the cast unspecified there).  Normals must be finite.
 * Frame f's seg panel goes to out[f, :, col : col+W, :], its normal panel to out[f, :, col+W : col+2W, :].
 * ============================================================================================== */
#define A3D_RENDER_MASK 0
#define A3D_RENDER_POLY 1
#define A3D_RENDER_MAX_HALFPLANES 4
typedef struct a3d_render_layer {
    int kind;               /* A3D_RENDER_MASK | A3D_RENDER_POLY                                               */
    int alpha;              /* 0 .. 256                                                                        */
    unsigned char color[4]; /* R, G, B (in the frames' channel order), pad                                     */
    int x0, y0, x1, y1;     /* cull box: the layer covers no pixel outside [x0,x1) x [y0,y1)                   */
    int p0, p1;             /* MASK: p0 = row of `bits`;  POLY: pieces [p0, p1)                                */
} a3d_render_layer;
typedef struct a3d_render_piece {
    int n;                  /* half-planes in use, 0 .. 4 (0 covers nothing)                                   */
    float abc[A3D_RENDER_MAX_HALFPLANES][3]; /* (A, B, C): inside is e >= 0                                    */
    int x0, y0, x1, y1;     /* the piece's own cull box, as the layer's: a superset of what the piece covers   */
} a3d_render_piece;
typedef struct a3d_render_desc {
    const unsigned char *frames;    /* [F,H,W,3] uint8                                                         */
    const int *layer_off;           /* [F+1] ascending offsets into `layers`                                   */
    const a3d_render_layer *layers; /* [n_layers]                                                              */
    const a3d_render_piece *pieces; /* [n_pieces]                                                              */
    const int *inst_off;            /* [F+1] ascending offsets into inst_row / normals                         */
    const int *inst_row;            /* [n_inst] row of `bits`                                                  */
    const float *normals;           /* [n_inst,3] unit normals                                                 */
    const unsigned int *bits;       /* [n_masks, ceil(H*W/32)]: bit i of word w = pixel 32w+i (row-major)       */
    unsigned char *out;             /* [F,H,pitch,3] uint8                                                     */
    int F, H, W, pitch, col;
    int n_layers, n_pieces, n_inst, n_masks;
    int pad_;
} a3d_render_desc;
/* A3D_ERR_ARG before any launch: F < 0, H or W < 1, col < 0, col + 2W > pitch, a negative count, or a null table with a
 * non-zero count (frames / out / layer_off / inst_off with F > 0).  F == 0 is a no-op.  Table entries that point outside
 * their tables (a layer range past n_layers, a piece past n_pieces, a mask row past n_masks) are skipped, never read. */
int a3d_render_panels(const a3d_render_desc *d, void *stream);

/* ================================================================================================
 * The dense mesh of one mask on its plane, in up to 16 rigid poses (the reference's --save-obj block, tools/inference.py:44-168,
 * over get_single_image_mesh's reduce_size=False branch, pkg/utils/vis.py:579-600).  Everything is on the device; the call
 * does no host synchronisation.  normal / offset / focal / cx / cy / pivot / xforms mean exactly what they mean in a3d_sweep_desc.
 *
 * The law (held bit for bit by tests/mesh_ref.py):
 *   lattice   pixels (y, x) with y % stride == 0 and x % stride == 0; Lh = ceil(H/stride), Lw = ceil(W/stride).  A lattice pixel
 *             is live iff its mask bit XOR invert is 1 (bit i of word w = pixel 32w+i, words = ceil(H*W/32)).  Bits at or past
 *             H*W in the last word are never live, whatever they hold.
 *   vertices  vertex k is the k-th live lattice pixel in row-major order; n_verts is their number.
 *   position  in float64: rx = (x - cx)/focal, ry = (y - cy)/focal, den = n0*rx + n1*ry + n2, depth = offset/den;
 *             p = ((float)(depth*rx), (float)(depth*ry), (float)depth).  Per pose a, in fp32, left to right, no contraction:
 *             q = p - pivot, t_i = (m[3i]*qx + m[3i+1]*qy + m[3i+2]*qz) + pivot_i + m[9+i], m = xforms[a].  With flip_yz,
 *             t_y and t_z are negated last (exact: the reference's --webvis matrix diag(1,-1,-1)).  verts[a, k, :] = t.
 *   uv        uvs[k] = ((float)((double)x / W), (float)(1.0 + (-(double)y) / H)).
 *   faces     0-based indices local to the mesh, in the row-major order of their first vertex.  For a live (y, x) with
 *             y + stride < H and x + stride < W: first [v(y,x), v(y+s,x+s), v(y,x+s)] if (y,x+s) and (y+s,x+s) are live,
 *             then [v(y,x), v(y+s,x), v(y+s,x+s)] if (y+s,x) and (y+s,x+s) are live (the reference's "upper right" /
 *             "bottom left" pair and its winding).  n_faces is their number.
 *   counts    counts[0] = n_verts, counts[1] = n_faces: the TRUE numbers even when they exceed cap_v / cap_f.  Nothing is
 *             ever written at or past a capacity; rows past the counts are left untouched.
 * Worst case for a lattice: cap_v = Lh*Lw, cap_f = 2*(Lh-1)*(Lw-1).  Non-finite vertices (a plane edge-on to a ray) are
 * whatever IEEE gives.
 * ============================================================================================== */
#define A3D_MESH_MAX_POSES 16
typedef struct a3d_mesh_desc {
    const unsigned int *bits;  /* [ceil(H*W/32)] one bit-packed mask (a row of a3d_masks_pack_bits' output)            */
    int H, W, stride, invert;  /* stride >= 1; invert 0 / 1                                                            */
    float normal[3];           /* as a3d_sweep_desc                                                                    */
    float offset;
    double focal, cx, cy;
    float pivot[3];
    int A;                     /* poses, 1 .. A3D_MESH_MAX_POSES                                                       */
    const float *xforms;       /* [A][12]: R (row-major 3x3) then t; point' = R (point - pivot) + pivot + t            */
    int flip_yz;               /* 0 / 1                                                                                */
    int cap_v, cap_f;          /* rows of verts (per pose) / uvs, rows of faces                                        */
    int pad_;
    float *verts;              /* [A, cap_v, 3]                                                                        */
    float *uvs;                /* [cap_v, 2]                                                                           */
    int *faces;                /* [cap_f, 3]                                                                           */
    int *counts;               /* [2]                                                                                  */
    void *workspace;           /* a3d_mesh_workspace_bytes bytes, 4-byte aligned; contents are scratch                  */
} a3d_mesh_desc;
/* 0 when H, W or stride is out of range. */
size_t a3d_mesh_workspace_bytes(int H, int W, int stride);
/* A3D_ERR_ARG before any launch: a null descriptor, bits / xforms / counts / workspace null, verts or uvs null with cap_v > 0,
 * faces null with cap_f > 0, H or W < 1, stride < 1, H*W >= 2^30 (2*H*W faces must fit int32), A outside 1 .. 16, a negative
 * capacity. */
int a3d_mesh_build(const a3d_mesh_desc *d, void *stream);

/* ================================================================================================
 * Evaluation: the reference's articulation AP (ArtiEvaluator -> evaluate_for_arti_axis, pkg/evaluation/arti_evaluation.py:262-665,
 * over pkg/utils/metrics.py and pkg/utils/VOCap.py) and its depth_l1_dist (pkg/evaluation/scannet_evaluation.py:241-248), on the
 * device: one launch matches every detection of every image, one launch turns the sorted true-positive bits into the AP table.
 * The law is stated in numpy float64 by tests/eval_ref.py; articulation3d_amd/evaluation.py lists the departures from the reference.
 *
 * a3d_eval_match, per image i with detections [det_off[i], det_off[i+1]) and ground truths [gt_off[i], gt_off[i+1]):
 *   line      of a detection, per kind (rot: (sin, cos, off) = det[9:12]; tran: (sin, cos) = det[12:14], off = 0).  In fp32:
 *             cx = (x1 + x2) / 2, cy = (y1 + y2) / 2, p = off * 100, x = (p * cos) + cx, y = (p * sin) + cy.  Then float64:
 *             sin == 0 -> (x, 0, x, H-1);  k = -(cos / sin);  k == 0 -> (0, y, W-1, y);  otherwise the candidates, in this order,
 *             v = y - k*x in [0, H) -> (0, v);  v = (k*(W-1) + y) - k*x in [0, H) -> (W-1, v);  v = x - y/k in [0, W) -> (v, 0);
 *             v = (x - y/k) + (H-1)/k in [0, W) -> (v, H-1);  the line is the first candidate and the first later one that differs
 *             from it (the first again if none does), (0, 0, 1, 1) if there is no candidate.  Every coordinate is truncated toward 0.
 *   iou       float64 from the fp32 boxes: area = (x2 - x1) * (y2 - y1), w = min(x2) - max(x1), h = min(y2) - max(y1), both clamped
 *             at 0, inter = w * h, iou = inter > 0 ? inter / ((area_d + area_g) - inter) : 0.  A detection's ground truth is the
 *             argmax (lowest index on ties); it is valid iff that iou > filter_iou.  No ground truth: not valid.
 *   ea        against the ground truth's line of the ground truth's kind; 0 if that line is invalid, or either line has equal end
 *             points.  angle(l) = x1 == x2 ? -pi/2 : atan((y1 - y2) / (x1 - x2));  d = |angle_p - angle_g|, d = min(d, pi - d),
 *             sa = max(0, 1 - d*2/pi)^2;  c = sqrt(dy^2 + dx^2) of the two mid points / max(W, H), se = max(0, 1 - c)^2;  ea = sa*se.
 *   normal    n = plane / max(|plane|, 1e-12) (plane = det[6:9]), dot = (n0*g0 + (-n2)*(-g1)) + n1*g2 with g the ground truth's raw
 *             normal; err = acos(clamp(dot, -1, 1)) / pi * 180, or 180 if |g| > 1.1.
 *   rank      the number of detections j of the image with score_j > score_d, or score_j == score_d and j < d.
 *   tp        bit m (0 bbox, 1 bbox+axis, 2 bbox+normal, 3 bbox+normal+axis) is set iff the detection QUALIFIES for m -- valid, its
 *             class equals its ground truth's, iou > iou_thresh, and ea > iou_thresh / err < normal_thresh where m names them -- and
 *             no detection of lower rank qualifies for m with the same ground truth.
 * Outputs for a detection that is not valid: gt_id -1, iou its best iou (0 without ground truths), ea 0, normal_err 180, tp 0.
 * ============================================================================================== */
#define A3D_EVAL_DET_COLS 14 /* the detection record's head (a3d_detections_pack): box 0:4, score 4, class 5, plane 6:9, rot 9:12, tran 12:14 */
#define A3D_EVAL_GT_FCOLS 7  /* box xyxy 0:4, raw normal 4:7                                                                           */
#define A3D_EVAL_GT_ICOLS 12 /* class 0, kind 1 (0 rot, 1 tran), rot line x1 y1 x2 y2 2:6, rot valid 6, tran line 7:11, tran valid 11 */
#define A3D_EVAL_MAX_GT 64   /* ground truths per image                                                                                */
#define A3D_EVAL_MAX_CLASSES 64
typedef struct a3d_eval_match_desc {
    const float *det;            /* [N, A3D_EVAL_DET_COLS] fp32                                                              */
    const float *gt_f;           /* [M, A3D_EVAL_GT_FCOLS] fp32                                                              */
    const int *gt_i;             /* [M, A3D_EVAL_GT_ICOLS] int32                                                             */
    const int *det_off;          /* [I+1] device copy of det_off_host                                                        */
    const int *gt_off;           /* [I+1] device copy of gt_off_host                                                         */
    const int *det_off_host;     /* [I+1] HOST: 0 = off[0] <= off[1] <= ... <= off[I] = N; validated before the launch       */
    const int *gt_off_host;      /* [I+1] HOST: likewise, ending at M, no image with more than A3D_EVAL_MAX_GT               */
    int I, N, M;
    int img_h, img_w;            /* the lines' image size (the reference's 480 x 640)                                        */
    int pad_;
    double filter_iou, iou_thresh, normal_thresh;
    int *gt_id;                  /* [N] index within the image's ground truths, -1 when not valid                            */
    double *iou, *ea, *normal_err; /* [N] each                                                                               */
    int *rank;                   /* [N]                                                                                      */
    unsigned char *tp;           /* [N]                                                                                      */
} a3d_eval_match_desc;
/* A3D_ERR_ARG before any launch: a null descriptor, I / N / M negative, img_h or img_w < 1, null host offsets with I > 0, offsets
 * that do not start at 0, descend, or do not end at N / M, an image with more than 64 ground truths, a null device table that has
 * rows, a null output with N > 0, a NaN threshold, I == 0 with N or M not 0.  I == 0 is a no-op.  The kernel clamps the device offsets to N / M: a device copy that differs
 * from the validated host one gives wrong numbers, never a read or write outside the tables. */
int a3d_eval_match(const a3d_eval_match_desc *d, void *stream);

/* AP per (metric m, class c): the entries of class c are tp[seg_off[c] .. seg_off[c+1]), already in descending score order.  In
 * float64: t_i / f_i the inclusive counts of set / clear bit m up to entry i, rec_i = t_i / npos[c], prec_i = t_i / (t_i + f_i),
 * mpre_i = max(prec_j, j >= i), ap = sum over the entries where rec changes of (rec_i - rec_(i-1)) * mpre_i, rec_(-1) = 0 (VOCap.py's
 * closing sentinel (1, 0) adds nothing).  ap[m*C + c]; 0 for a class without entries or with npos[c] <= 0.  n_entries[c] = the
 * segment's length. */
typedef struct a3d_eval_ap_desc {
    const unsigned char *tp;     /* [seg_off[C]] true-positive bits, a3d_eval_match's tp gathered in sorted order             */
    const int *seg_off_host;     /* [C+1] HOST, 0 first, ascending                                                           */
    const int *npos_host;        /* [C] HOST: annotations of class c in the whole dataset                                    */
    int C;                       /* 1 .. A3D_EVAL_MAX_CLASSES                                                                */
    int pad_;
    double *ap;                  /* [4, C]                                                                                   */
    int *n_entries;              /* [C]                                                                                      */
} a3d_eval_ap_desc;
/* A3D_ERR_ARG before any launch: a null descriptor or host table, C outside 1 .. 64, offsets that do not start at 0 or descend,
 * tp null with entries, a null output. */
int a3d_eval_ap(const a3d_eval_ap_desc *d, void *stream);

/* Per image b: sum[b] = sum over pixels of |pred - gt| * [gt > 1e-4] in float64, count[b] the number of such pixels.  One workgroup
 * per image adds in a fixed order (no atomics): two runs give identical bits.  The caller's dataset value is the mean over images
 * of sum / max(count, 1). */
typedef struct a3d_depth_l1_desc {
    const float *pred, *gt;      /* [B,H,W] fp32 each                                                                        */
    int B, H, W, pad_;
    double *sum;                 /* [B]                                                                                      */
    int *count;                  /* [B]                                                                                      */
} a3d_depth_l1_desc;
/* A3D_ERR_ARG before any launch: a null descriptor, B < 0, H or W < 1, H*W >= 2^31, a null pointer with B > 0.  B == 0 is a no-op. */
int a3d_depth_l1(const a3d_depth_l1_desc *d, void *stream);

/* ================================================================================================
 * Evaluation of the plane stage: the reference's ScanNet box / mask / plane AP and plane statistics (ScannetEvaluator ->
 * evaluate_for_planes, pkg/evaluation/scannet_evaluation.py:254-450, over compare_planes of pkg/utils/metrics.py:6-19 and
 * pkg/utils/VOCap.py).  Two launches (csrc/plane_eval.hip) in front of a3d_eval_ap, which is reused as it is.  The law is stated in
 * numpy float64 by tests/plane_eval_ref.py; articulation3d_amd/evaluation_planes.py lists the departures from the reference.
 *
 * The ground truth is ONE fp32 table, A3D_PLANE_GT_COLS columns per row: box xyxy 0:4, plane (normal * offset) 4:7, class 7.
 *
 * a3d_eval_mask_counts, per detection n of image i (detections [det_off[i], det_off[i+1]), ground truths [gt_off[i], gt_off[i+1])):
 *   g         the ground truth with the largest box IoU, by a3d_eval_match's law (float64 from the fp32 boxes, lowest index on ties;
 *             one device function serves both); gt_id[n] = g, or -1 for an image without ground truth.
 *   mask      row det_slot[n] of `masks` (uint8 [S,H,W], non-zero = set, read as the detector wrote it); a slot outside [0, S) is an
 *             empty mask.
 *   inter[n]  the number of pixels p < H*W that are set in the mask AND in row g of gt_bits (bit p & 31 of word p >> 5, the layout
 *             of a3d_masks_pack_bits); 0 without ground truth.
 *   uni[n]    the number of pixels p < H*W set in either; the mask's own area without ground truth.
 * Bits of the last word at or past H*W are never read as pixels.  Integer sums only (integer atomics on counters the call zeroes
 * first): the result does not depend on the order of arrival.  The work is spread over (detection, block of 16 384 pixels); a lane
 * reads 16 mask bytes per load wherever the ADDRESS is 16-byte aligned -- a mask row starts at slot*H*W bytes, any alignment -- and
 * the bytes before and after the aligned part of a block one by one.
 *
 * a3d_eval_plane_match, per image, one wave, in float64:
 *   g, rank   as in a3d_eval_match; box_iou = the IoU with g.
 *   mask_iou  uni > 0 ? inter / uni : 0 (two empty masks: 0).
 *   planes    compare_planes: for p = det[6:9] and for the ground truth's plane, off = sqrt((p0*p0 + p1*p1) + p2*p2) + 1e-5,
 *             n = p / off;  d = sqrt((dx*dx + dy*dy) + dz*dz) of n_p - n_g, clamped to [0, 2];
 *             normal_err = 2 * asin(d / 2) / pi * 180;  offset_err = |off_p - off_g|.
 *   tp        bit 0 box (box_iou > iou_thresh), bit 1 mask (mask_iou > iou_thresh), bit 2 plane (normal_err < normal_thresh and
 *             offset_err < offset_thresh): set iff the detection QUALIFIES -- its class (det[5], truncated) equals its ground
 *             truth's and the test holds -- and no detection of lower rank qualifies for the same bit with the same ground truth.
 *             Bit 3 is always 0.  There is no filter_iou: every detection is an AP entry.
 * An image without ground truth: gt_id -1, box_iou 0, mask_iou 0, normal_err 180, offset_err +inf, tp 0.
 * ============================================================================================== */
#define A3D_PLANE_GT_COLS 8
typedef struct a3d_eval_mask_counts_desc {
    const float *det;            /* [N, A3D_EVAL_DET_COLS] fp32 (only the box columns are read)                              */
    const float *gt;             /* [M, A3D_PLANE_GT_COLS] fp32                                                              */
    const int *det_off;          /* [I+1] device copy of det_off_host                                                        */
    const int *gt_off;           /* [I+1] device copy of gt_off_host                                                         */
    const int *det_off_host;     /* [I+1] HOST: 0 = off[0] <= off[1] <= ... <= off[I] = N; validated before the launch       */
    const int *gt_off_host;      /* [I+1] HOST: likewise, ending at M, no image with more than A3D_EVAL_MAX_GT               */
    const unsigned char *masks;  /* [S,H,W] uint8, non-zero = set                                                            */
    const int *det_slot;         /* [N] the row of `masks` of detection n                                                    */
    const unsigned int *gt_bits; /* [M, ceil(H*W/32)] a3d_masks_pack_bits' layout                                            */
    int I, N, M, S, H, W;
    int *gt_id, *inter, *uni;    /* [N] each                                                                                 */
} a3d_eval_mask_counts_desc;
/* A3D_ERR_ARG before any launch: a null descriptor, I / N / M / S negative, H or W < 1, H*W >= 2^31, null host offsets with I > 0,
 * offsets that do not start at 0, descend, or do not end at N / M, an image with more than A3D_EVAL_MAX_GT ground truths, I == 0
 * with N or M not 0, null device offsets, det_slot / det / an output null with N > 0, gt / gt_bits null with M > 0, masks null with
 * S > 0.  I == 0 and N == 0 are no-ops.  The kernels clamp the device offsets to N / M, the slots to S and the ground truth to the
 * image's range: wrong device tables give wrong numbers, never an access outside a buffer. */
int a3d_eval_mask_counts(const a3d_eval_mask_counts_desc *d, void *stream);

typedef struct a3d_eval_plane_match_desc {
    const float *det;            /* [N, A3D_EVAL_DET_COLS] fp32                                                              */
    const float *gt;             /* [M, A3D_PLANE_GT_COLS] fp32                                                              */
    const int *det_off;          /* [I+1] device copy of det_off_host                                                        */
    const int *gt_off;           /* [I+1] device copy of gt_off_host                                                         */
    const int *det_off_host;     /* [I+1] HOST, validated as above                                                           */
    const int *gt_off_host;      /* [I+1] HOST, validated as above                                                           */
    const int *inter, *uni;      /* [N] each: a3d_eval_mask_counts' columns                                                  */
    int I, N, M, pad_;
    double iou_thresh, normal_thresh, offset_thresh;
    int *gt_id, *rank;           /* [N] each                                                                                 */
    double *box_iou, *mask_iou, *normal_err, *offset_err; /* [N] each                                                        */
    unsigned char *tp;           /* [N]                                                                                      */
} a3d_eval_plane_match_desc;
/* A3D_ERR_ARG before any launch: as a3d_eval_mask_counts for the descriptor, the counts and the offsets; gt null with M > 0; det,
 * inter, uni or an output null with N > 0; a NaN threshold.  I == 0 and N == 0 are no-ops.  The device offsets are clamped. */
int a3d_eval_plane_match(const a3d_eval_plane_match_desc *d, void *stream);

/* ================================================================================================
 * Motion-JPEG: the clip's visualisation rows as a video (the reference's output.mp4, tools/inference.py:254-276, is H.264 through
 * imageio; this library writes baseline JPEG frames for an AVI container, articulation3d_amd/video.py).  Every frame is the entropy
 * data of a JFIF image -- 8-bit, Y / Cb / Cr at 4:4:4, the Annex K tables of ITU-T T.81, a restart interval of one MCU row -- and
 * the host puts the headers around it.  Integer arithmetic only.
 *
 * The law (held byte for byte by tests/mjpeg_ref.py, which tests/test_mjpeg_host.py holds to libjpeg):
 *   geometry  rows = ceil(H/8) segments per frame, mcus = ceil(W/8) MCUs per segment, an MCU = one Y, one Cb, one Cr block.  The
 *             pixel of a block at (y, x) past the image is the pixel at (min(y, H-1), min(x, W-1)).
 *   colour    Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *             Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *             Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16      (>> arithmetic; libjpeg's constants and rounding)
 *   DCT       X = component - 128;  T = (X C13' + 512) >> 10 over rows, F = (C13 T + 32768) >> 16 over columns,
 *             C13[k][n] = rint(8192 a(k) cos((2n+1) k pi / 16)), a(0) = sqrt(1/8), a(k>0) = 1/2.  Every intermediate is within int32:
 *             |X C13'| <= 128 * 23168, |T| <= 2896, |C13 T| <= 23168 * 2896 = 67 094 528.
 *   quantise  q = sign(F) * ((|F| + (Q >> 1)) / Q);  Q = clamp((t * s + 50) / 100, 1, 255) of the Annex K value t,
 *             s = quality < 50 ? 5000 / quality : 200 - 2 * quality  (libjpeg's jpeg_set_quality).  Coefficients travel in zigzag order.
 *   entropy   per segment: the three DC predictors start at 0; Huffman symbols as in the standard (ZRL for runs over 15, EOB when a
 *             block ends in zeros, one's complement amplitudes of negative values); the last byte is filled with 1-bits; every 0xFF
 *             byte, the filled one included, is followed by 0x00.
 *   stream    a frame's data is its segments in order with RSTm, m = row mod 8, behind every segment but the last; frame f's data
 *             is packed[frame_off[f] .. frame_off[f+1]).
 * A block is at most A3D_JPEG_BLOCK_BITS = 9 + 11 + 63 * (16 + 10) bits (|DC difference| <= 2040: category 11; |AC| < 1024: category
 * 10), stuffing at most doubles a segment: a3d_jpeg_slot_bytes is that worst case, so no input can overrun a slot.  The result of a
 * frame does not depend on F or on the frames beside it.
 * ============================================================================================== */
#define A3D_JPEG_BLOCK_BITS 1658
#define A3D_JPEG_HUFF_VALS 162
/* HOST tables, for the headers: bits [4][16] and vals [4][A3D_JPEG_HUFF_VALS] (zero-filled past a table's symbols), the Annex K Huffman
 * specifications in the order DC0, AC0, DC1, AC1. */
int a3d_jpeg_tables(unsigned char *bits, unsigned char *vals);
/* HOST: out [2][64] = the two tables scaled for `quality`, natural order.  A3D_ERR_ARG outside 1 .. 100. */
int a3d_jpeg_quant(int quality, unsigned char *out);
/* Bytes of one segment's slot for frames W wide (a multiple of 16); 0 for W outside 1 .. 65535. */
size_t a3d_jpeg_slot_bytes(int W);
/* frames uint8 [F,H,pitch,3] RGB (pitch >= W pixels per row, so a view into wider rows works) -> seg_len [F*rows] the bytes of every
 * segment, written at slots + s * slot_bytes; seg_off [F*rows] its place in the packed stream; frame_off [F+1].  coef (16-byte
 * aligned, F * rows * mcus * 192 int16) is scratch.  Three launches, no synchronisation.  A3D_ERR_ARG before any launch: F < 0, H or W outside
 * 1 .. 65535, pitch < W, quality outside 1 .. 100, a null pointer (frame_off always; the others with F > 0), a misaligned coef, or
 * F * rows * (slot_bytes + 2) above 2^31 - 1 (the offsets are int32: encode fewer frames per call). */
int a3d_jpeg_encode(const unsigned char *frames, int F, int H, int W, int pitch, int quality, short *coef, unsigned char *slots,
                    int *seg_len, int *seg_off, int *frame_off, void *stream);
/* Copies every segment to packed + seg_off[s] and puts its RST marker behind it.  packed_bytes is the size of the destination (the
 * host reads frame_off[F] first): a segment that would end past it is left out, never written.  F == 0 is a no-op. */
int a3d_jpeg_pack(const unsigned char *slots, const int *seg_off, const int *seg_len, int F, int H, int W, unsigned char *packed,
                  long long packed_bytes, void *stream);

/* ================================================================================================
 * JPEG decode: the entropy-coded bytes of F baseline JPEG frames of one geometry -> uint8 [F,H,pitch,3] RGB on the device, byte for
 * byte what libjpeg's default decoder (PIL's Image.open(f).convert("RGB")) returns.  The host (articulation3d_amd/video.py) parses the
 * headers, finds every unit's bytes and refuses what is outside the law.  Integer arithmetic only.
 *
 * The law (held byte for byte by tests/jpeg_decode_ref.py, which tests/test_jpeg_decode_host.py holds to libjpeg):
 *   accepted  SOF0, 8-bit, one interleaved scan.  One component (grey, returned as R = G = B) or three (Y, Cb, Cr) with chroma 1x1
 *             and luma hs x vs = 1x1, 2x1 or 2x2 (4:4:4, 4:2:2, 4:2:0).  8-bit quantisation tables.  Any Huffman tables; a file
 *             without any DHT segment uses the Annex K tables of a3d_jpeg_tables (the AVI "MJPG" convention).  Any restart
 *             interval, or none.  The host refuses everything else: progressive, arithmetic, 12-bit, 16-bit quantisation tables,
 *             other sampling factors, several scans, 2 or 4 components, H or W outside 1 .. 65535, a missing SOI, SOF or SOS.
 *   geometry  an MCU is 8 hs x 8 vs pixels; there are mx = ceil(W / 8 hs) by my = ceil(H / 8 vs) MCUs in raster order; within an MCU
 *             each component contributes its v x h blocks in raster order.  A unit is one restart interval of n MCUs (the last one
 *             of a frame is short; intervals need not align with MCU rows), or the whole scan when n = 0: ceil(mx my / n) units per
 *             frame.  The DC predictors are zero at the start of every unit.  In entropy-coded data FF 00 is the data byte FF, and
 *             FF D0 .. D7 occurs only as a restart marker, which the host removes.
 *   entropy   symbol, run / size, ZRL, EOB and one's-complement extension as in the standard; a DC value accumulates modulo 2^16.
 *             A unit that needs bits past its byte range reads zeros and makes the frame A3D_JPEG_SHORT.  A bit pattern that matches
 *             no code of at most 16 bits, a DC symbol above 15, or a run that passes coefficient 63 (a ZRL that ends past 64
 *             included) makes it A3D_JPEG_BAD_CODE and ends the unit; its remaining blocks stay zero.  A unit writes only its own
 *             blocks: no stream content can make a read or a write leave the buffers of the call.
 *   IDCT      libjpeg's jidctint ("islow") on dequantised coefficients, CONST_BITS 13, PASS1_BITS 2, constants 2446, 3196, 4433,
 *             6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172: pass 1 over columns descales by 11, pass 2 over rows
 *             by 18, sample = clamp(v + 128, 0, 255) (a plain clamp).
 *   domain    the law holds for frames in which every dequantised coefficient and every pass-1 output is within +-16383: the
 *             absolute gain of a pass over all its intermediates is 61 214, and 61 214 x 16 383 < 2^31, so everything fits int32.
 *             Outside, libjpeg's own routines disagree with each other: the frame is A3D_JPEG_RANGE and its pixels are unspecified
 *             (real encoders stay about four times below the bound).
 *   upsample  libjpeg's "fancy" filters.  dw = ceil(W / hs), dh = ceil(H / vs) is the chroma plane's true size; neighbour indices
 *             are clamped to [0, dw-1] and [0, dh-1].
 *             2x1:  out[2i] = (3 in[i] + in[i-1] + 1) >> 2,  out[2i+1] = (3 in[i] + in[i+1] + 2) >> 2.
 *             2x2:  s = 3 near + far vertically (an even output row takes the row above as far, an odd one the row below), then
 *                   out[2i] = (3 s[i] + s[i-1] + 8) >> 4,  out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4.
 *             A chroma plane with dw <= 2 is replicated instead, in both directions.
 *   colour    R = Y + ((91881 Cr' + 32768) >> 16),  G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16),
 *             B = Y + ((116130 Cb' + 32768) >> 16),  Cb' = Cb - 128, Cr' = Cr - 128, >> arithmetic, clamped to 0 .. 255.
 *   status    per frame, the largest that occurred of 0 < A3D_JPEG_RANGE < A3D_JPEG_BAD_CODE < A3D_JPEG_SHORT: the cause, not its
 *             consequences (zeros read past a unit may match no code; a unit cut short leaves garbage coefficients).
 * The result of a frame does not depend on F or on the frames beside it.
 * ============================================================================================== */
#define A3D_JPEG_RANGE 1
#define A3D_JPEG_BAD_CODE 2
#define A3D_JPEG_SHORT 3
/* One table set: quant [3][64] (per component, natural order), then per component its DC and its AC Huffman specification, each
 * bits[16] + vals[256] (zero-filled past the table's symbols).  Specifications, not lookups: the kernel builds its own form. */
#define A3D_JPEG_TABSET_BYTES (192 + 6 * (16 + 256))
/* Elements PER FRAME of the two scratch buffers of a3d_jpeg_decode: coef (int16; a frame's status word in its last 16 bytes) and
 * planes (uint8, the components at their padded sizes).  A3D_ERR_ARG for a geometry outside the law. */
int a3d_jpeg_decode_scratch(int H, int W, int ncomp, int hs, int vs, size_t *coef_elems, size_t *plane_elems);
typedef struct {
    int F, H, W, pitch;          /* rgb is [F,H,pitch,3], pitch >= W pixels per row                                          */
    int ncomp, hs, vs;           /* 1 or 3 components; the luma sampling factors                                             */
    int n_units, n_sets;
    long long data_bytes;        /* all units of all frames, concatenated without their markers, still stuffed              */
    /* HOST, read before any launch: */
    const int *unit_off;         /* [n_units+1] unit u is bytes unit_off[u] .. unit_off[u+1] of the data                     */
    const int *frame_unit;       /* [F+1] frame f owns units frame_unit[f] .. frame_unit[f+1]                                */
    const int *frame_ri;         /* [F] restart interval in MCUs, 0 = none                                                  */
    const int *frame_set;        /* [F] index of the frame's table set                                                      */
    const unsigned char *sets;   /* [n_sets][A3D_JPEG_TABSET_BYTES]                                                         */
    /* DEVICE: */
    const unsigned char *d_data; /* data_bytes rounded up to a multiple of 4 are readable; 4-byte aligned                    */
    const int *d_meta;           /* the four host tables in the order above, back to back                                    */
    const unsigned char *d_sets; /* `sets` on the device, 8-byte aligned                                                    */
    short *coef;                 /* scratch, F * coef_elems, 16-byte aligned                                                 */
    unsigned char *planes;       /* scratch, F * plane_elems, 8-byte aligned                                                 */
    unsigned char *rgb;          /* out; bytes of a row past W pixels are left alone                                         */
    int *status;                 /* out [F]                                                                                  */
} a3d_jpeg_decode_desc;
/* One memset and three launches (entropy, dequantise + IDCT, upsample + colour) on the stream, no synchronisation.  The kernels read
 * the device copies and clamp whatever they find there.  A3D_ERR_ARG before any launch: a null pointer, a misaligned buffer, a
 * geometry outside the law, pitch < W, F outside 0 .. 65535, an offset table that is not monotonic or does not start at 0 and end
 * at data_bytes / n_units, a frame whose unit count is not ceil(mx my / interval), a table index out of range, a Huffman
 * specification whose codes do not fit their lengths, or data_bytes above 2^31 - 1.  F == 0 is a no-op.
 * The entropy launch synchronises itself: a unit (above all a scan without restart intervals) is decoded by many lanes at once, in
 * subsequences of A3D_JPEG_SPLIT_BYTES.  No stream content can make a read or a write leave the buffers of the call, and a unit
 * writes only its own blocks.  The result does not depend on the subsequence size, on F or on the frames beside a frame: it is exact
 * by construction, never by a stream happening to synchronise.
 *   scheme    a unit's stuffed bytes are cut into subsequences of S = max(subsequence size, ceil(unit bytes / L)) bytes, one lane each; the
 *             L <= 1024 lanes of a unit share a workgroup (short units share one), so nothing synchronises across workgroups.  A
 *             decoder state between two syntax elements is (bit position, block slot within the MCU, zig-zag index; 0 = a DC symbol
 *             is next).  Round 0 walks every subsequence from (its first bit, slot 0, index 0), the first from the unit's start; in
 *             each later round a lane takes its left neighbour's exit state as its entry and walks again if that differs from the
 *             entry it last used, until a round changes nothing or as many rounds as subsequences have run: after round r the lanes
 *             0 .. r hold their true states, so the fixed point is the sequential walk.  A speculative walk carries on past an
 *             inconsistency (it consumes what the law consumes, ends the block, goes to the next slot); the rule affects the number
 *             of rounds only.  A prefix sum of the blocks each lane began places its blocks; the first inconsistency of the true chain
 *             inside the unit's blocks ends the unit as in the law, and the last lane reads zeros past the unit until its blocks are
 *             done (SHORT over BAD_CODE, the cause).  A second walk from the true entries stores AC values and DC differences, and a
 *             sum per unit and component, modulo 2^16, turns the differences into DC values.
 *   cost      the launch is the latency of one lane's walks.  Against one lane per unit walking once (the launch this one replaced) it is
 *             2.1 - 17 x shorter where units are longer than some 1 KB, and 1.1 - 2.1 x LONGER where a unit is one or a few
 *             subsequences (restart intervals of 1 - 5 MCUs of a 480 x 640 frame: 300 - 710 us against 150 - 500 us for 8 - 32
 *             frames), which end to end costs up to 18 % of the frames/s of such a stream at 8 frames per call and nothing
 *             measurable at 32 (MEASUREMENTS.md, "JPEG decode: one entropy kernel").  */
#define A3D_JPEG_SPLIT_BYTES 32 /* the fastest of 32 .. 256 for three of four classes of stream (MEASUREMENTS.md, "JPEG decode") */
int a3d_jpeg_decode(const a3d_jpeg_decode_desc *d, void *stream);
/* a3d_jpeg_decode with an explicit subsequence size in place of A3D_JPEG_SPLIT_BYTES: the same descriptor, scratch, validation,
 * A3D_ERR_ARG cases, status codes and result; split_bytes < 1 is A3D_ERR_ARG as well. */
int a3d_jpeg_decode_split(const a3d_jpeg_decode_desc *d, int split_bytes, void *stream);

/* ================================================================================================
 * PNG: the lossless sibling of the Motion-JPEG writer (articulation3d_amd/png.py).  uint8 [F,H,pitch,3] RGB frames on the device ->
 * per frame the deflate blocks of one zlib stream: filtering, LZ77 and Huffman coding run on the device, the host builds each
 * frame's Huffman code from a histogram the device leaves and writes the container (signature, IHDR, one IDAT = 78 01 | the packed
 * segments | 03 00 | Adler-32, IEND, the chunk CRCs).  8-bit truecolour, no interlace.  Integer arithmetic only.
 *
 * The law (held byte for byte by tests/png_ref.py, which tests/test_png_host.py holds to zlib's inflate and to PIL):
 *   filter    stride = 1 + 3 W bytes per filtered row: the filter type, then the filtered samples (bpp = 3).  With x the byte, a the
 *             byte 3 to its left, b the byte above, c the byte above a (bytes outside the image are 0; the row above row 0 is zeros):
 *             0 None x, 1 Sub x - a, 2 Up x - b, 3 Average x - floor((a + b) / 2), 4 Paeth x - P(a, b, c) with the standard
 *             predictor (p = a + b - c; the nearest of a, b, c to p, ties in that order), all modulo 256.  A row takes the type
 *             whose filtered samples have the smallest sum of (v < 128 ? v : 256 - v); ties go to the lowest type.
 *   segments  a frame's H * stride filtered bytes are cut into segments of R = max(1, ceil(8192 / stride)) whole rows, the last one
 *             possibly shorter: S = ceil(H / R) segments of n <= 16384 bytes (W <= A3D_PNG_MAX_W, so that stride <= 16384).  One
 *             workgroup codes one segment.
 *   tokens    at byte i of a segment (g = its index in the frame) the candidate distances are d = 1, 3 and stride.  A candidate
 *             needs g - d >= 0: its source may lie in the segment before.  L_d(i) = the number of k = 0, 1, ... with
 *             f[g + k] == f[g + k - d], counted up to the first failure, capped at 258 and at n - i.  The candidate with the longest
 *             L wins, ties go to the smallest d.  L >= 3: a match (L, d), i += L; otherwise the literal f[g], i += 1.  Greedy from
 *             i = 0, no lazy matching.  (On the device L_d is a bit scan over equality masks, and the token starts are found by
 *             pointer doubling over next[i]: after round r the first 2^(r+1) tokens are marked.)
 *   symbols   RFC 1951's: literals 0 .. 255, end of block 256, lengths 257 .. 285 and distances 0 .. 29 with their extra bits.
 *   histogram per frame 286 literal / length counts and 30 distance counts over the tokens of all its segments, plus one end of
 *             block per segment.  The host turns it into the frame's code (articulation3d_amd/png.py: huffman_lengths,
 *             dynamic_header) and hands back a table of A3D_PNG_TAB_WORDS words per frame: words 0 .. 315 the symbols' codes as
 *             (bit-reversed code | length << 16), literal / length first; word 316 the bits of the block header; from word
 *             A3D_PNG_HDR_AT the header as a bit string, LSB first, starting with BFINAL = 0, BTYPE = 10, zero past its end.
 *   coding    a segment takes the cheapest in bytes of (ties go to the lowest number)
 *               0 stored   00 | LEN | NLEN | the n bytes: n + 5 bytes
 *               1 fixed    BFINAL 0, BTYPE 01, the tokens in the fixed code, end of block, then an empty stored block
 *               2 dynamic  the frame's header, the tokens in the frame's code, end of block, then an empty stored block
 *             where the empty stored block is 000, zero bits up to a byte boundary, 00 00 FF FF (a sync flush).  So every segment
 *             ends on a byte boundary, segments concatenate as bytes, and no segment takes more than n + 5 bytes.  Bits are
 *             packed LSB first, Huffman codes most significant bit first, extra bits as integers (RFC 1951, 3.1.1).
 *   Adler     per segment s1 = sum of b_k (uint32) and s2 = sum of (n - k) b_k (uint64), k = 0 .. n - 1: the host folds them.
 *   stream    frame f's deflate data is packed[frame_off[f] .. frame_off[f+1]), its segments in order.
 * The result of a frame does not depend on F or on the frames beside it.
 * ============================================================================================== */
#define A3D_PNG_MAX_W 5461
#define A3D_PNG_SEG_BYTES 8192 /* a segment is the fewest whole rows that reach this many filtered bytes */
#define A3D_PNG_SYMS 316       /* 286 literal / length + 30 distance */
#define A3D_PNG_HDR_AT 320
#define A3D_PNG_TAB_WORDS 400  /* a dynamic header is at most 17 + 19 * 3 + 316 * 7 = 2286 bits */
/* Bytes of one segment's slot for frames W wide: the largest segment + 5, rounded up to 16; 0 for W outside 1 .. A3D_PNG_MAX_W. */
size_t a3d_png_slot_bytes(int W);
/* frames uint8 [F,H,pitch,3] -> filt [F][H*stride] the filtered bytes; tok uint16 [F][H*stride]: 0 where no token starts, else
 * L | (0, 1, 2 for d = 1, 3, stride) << 9 with L = 1 for a literal; hist int32 [F][A3D_PNG_SYMS]; s1 uint32 [F*S], s2 uint64 [F*S].
 * One memset and two launches, no synchronisation.  A3D_ERR_ARG before any launch: F < 0, H outside 1 .. 65535, W outside
 * 1 .. A3D_PNG_MAX_W, pitch < W, a null pointer with F > 0, or F * H * stride or F * S * slot_bytes above 2^31 - 1. */
int a3d_png_scan(const unsigned char *frames, int F, int H, int W, int pitch, unsigned char *filt, unsigned short *tok, int *hist,
                 unsigned int *s1, unsigned long long *s2, void *stream);
/* filt, tok of a3d_png_scan and tab uint32 [F][A3D_PNG_TAB_WORDS] (device) -> every segment coded at slots + s * slot_bytes, seg_len
 * [F*S] its bytes, kind [F*S] its coding, seg_off [F*S] its place in the packed stream, frame_off [F+1].  Two launches.  The kernel
 * clamps what it finds in tab (a length to 15 bits, the header to its words), so no table can make a write leave a slot.
 * A3D_ERR_ARG as a3d_png_scan (frame_off always non-null). */
int a3d_png_emit(const unsigned char *filt, const unsigned short *tok, const unsigned int *tab, int F, int H, int W,
                 unsigned char *slots, int *seg_len, int *seg_off, int *frame_off, int *kind, void *stream);
/* Copies every segment to packed + seg_off[s].  packed_bytes is the size of the destination (the host reads frame_off[F] first): a
 * segment that would end past it is left out, never written.  F == 0 is a no-op. */
int a3d_png_pack(const unsigned char *slots, const int *seg_off, const int *seg_len, int F, int H, int W, unsigned char *packed,
                 long long packed_bytes, void *stream);

/* ================================================================================================
 * PNG decode: the deflate bodies of F PNG frames of one geometry -> uint8 [F,H,pitch,3] RGB on the device, byte for byte PIL's
 * Image.open(f).convert("RGB").  The host (articulation3d_amd/png.py: png_parse) walks the chunks, checks every CRC, IHDR and the zlib
 * header and refuses what is outside the law; inflate, the Adler-32, unfiltering and the conversion run on the device.  Integers only.
 *
 * The law (held byte for byte by tests/png_decode_ref.py, which tests/test_png_decode_host.py holds to zlib's inflate and to PIL):
 *   accepted  bit depth 8; colour type 0, 2, 4 or 6 (1, 3, 2 or 4 channels); interlace 0, compression 0, filter method 0.  Grey is
 *             replicated to R = G = B, an alpha channel is dropped, tRNS and every other ancillary chunk are ignored.  The host
 *             refuses: palette, bit depths 1, 2, 4 and 16, Adam7, a bad signature, a chunk CRC that does not match, a missing IHDR,
 *             IDAT or IEND, IDAT chunks that are not consecutive, a zlib header outside CM = 8, CINFO <= 7, FDICT = 0 with a valid
 *             FCHECK, H or W of 0, a raw size H * (1 + W * channels) above 2^31 - 1.
 *   body      a frame's bytes are its IDAT payloads concatenated, without the two bytes of the zlib header: deflate blocks, then,
 *             byte-aligned behind the final block, the Adler-32 of the raw bytes, big-endian.  Anything behind it is ignored.
 *   inflate   RFC 1951 in full: stored, fixed and dynamic blocks, any number of them; distances up to 32 768 whatever CINFO says;
 *             out[p + k] = out[p - d + k mod d] for a copy of a length above its distance d.  A set of code lengths is illegal when
 *             it is over-subscribed, or incomplete with a code longer than one bit (zlib's rule: one code of one bit, or none at all,
 *             passes; a pattern such a set gives no code consumes one bit and is A3D_PNGD_BAD_CODE).  The code-length code itself must
 *             be complete.  A code is consumed only if all its bits lie inside the stream; so are extra bits and header fields.
 *   unfilter  per row of 1 + W * channels raw bytes: the type, then the samples.  The filter distance is bpp = channels; a = the
 *             sample bpp to the left, b = above, c = above a; neighbours outside the image are 0; all arithmetic mod 256.
 *             0 None x, 1 Sub x + a, 2 Up x + b, 3 Average x + floor((a + b) / 2) on the 9-bit sum, 4 Paeth x + P(a, b, c) with
 *             p = a + b - c and the nearest of a, b, c to p, ties in that order.  A type above 4 counts as 0 and flags the frame.
 *   status    per frame 0 or the FIRST thing that went wrong, in stream order, then the filter bytes, then the checksum:
 *             A3D_PNGD_SHORT     bits needed past the stream's end (a stored block longer than the bytes left included); the final
 *                                block ends before the raw size is reached; fewer than 4 bytes are left for the Adler-32.
 *             A3D_PNGD_BAD_CODE  BTYPE 3; LEN != ~NLEN; HLIT above 286 or HDIST above 30; an illegal set of code lengths; no code
 *                                for the end of block; literal / length symbol 286 or 287; distance symbol 30 or 31; repeat code 16
 *                                with nothing before it; a repeat that runs past HLIT + HDIST.
 *             A3D_PNGD_FAR       a distance that reaches before the first output byte (checked before the length).
 *             A3D_PNGD_LONG      output that would pass the raw size (for a stored block: what the bytes left of it would
 *                                write).  The walk stops there; nothing is written past the raw size.
 *             A3D_PNGD_FILTER    a filter byte above 4.
 *             A3D_PNGD_ADLER     the checksum differs from the four bytes where the walk ended.
 *             The pixels of a flagged frame are outside the law.  Inside it: no stream content makes a read or a write leave the
 *             buffers of the call or touch another frame's bytes, every loop is bounded by the stream's bit count or by the raw size,
 *             and a frame's result does not depend on F or on the frames beside it.
 *   scheme    inflate: one wave per frame.  The decode tables live in LDS (a 10-bit primary lookup for literal / length and for
 *             distance codes; a longer code resolves through the first / count / offset rows of its length), built by all 64 lanes
 *             from the block's code lengths.  One lane walks the codes and hands tokens over in batches of 64; all lanes place the
 *             literals and run the batch's copies in order, each copy lane-parallel, in an LDS ring of the last 32 768 bytes.
 *             Adler-32: one workgroup per frame, a = 1 + sum b_j, b = N + sum (N - j) b_j mod 65521.  unfilter + convert: one wave per
 *             frame, bands of 64 rows in sequence; lane r owns row r of a band and reconstructs pixel t - r at step t, b and c come
 *             from lane r - 1 by a cross-lane move; only the row above a band is read back from memory.
 * ============================================================================================== */
#define A3D_PNGD_SHORT 1
#define A3D_PNGD_BAD_CODE 2
#define A3D_PNGD_FAR 3
#define A3D_PNGD_LONG 4
#define A3D_PNGD_FILTER 5
#define A3D_PNGD_ADLER 6
/* Bytes PER FRAME of the `raw` scratch of a3d_png_decode: the raw size rounded up to 16, then 16 bytes (the stored and the computed
 * Adler-32).  A3D_ERR_ARG for a geometry outside the law. */
int a3d_png_decode_scratch(int H, int W, int channels, size_t *raw_bytes);
typedef struct {
    int F, H, W, pitch;          /* rgb is [F,H,pitch,3], pitch >= W pixels per row                                          */
    int channels;                /* 1 grey, 2 grey + alpha, 3 RGB, 4 RGBA                                                    */
    long long data_bytes;        /* the frames' bodies, back to back                                                         */
    const int *frame_off;        /* HOST [F+1], read before any launch: frame f is bytes frame_off[f] .. frame_off[f+1]      */
    const unsigned char *d_data; /* DEVICE: data_bytes rounded up to a multiple of 4 are readable; 4-byte aligned            */
    const int *d_frame_off;      /* frame_off on the device                                                                  */
    unsigned char *raw;          /* scratch, F * raw_bytes, 16-byte aligned                                                  */
    unsigned char *rgb;          /* out; bytes of a row past W pixels are left alone                                         */
    int *status;                 /* out [F]                                                                                  */
} a3d_png_decode_desc;
/* One memset and three launches (inflate, Adler-32, unfilter + convert) on the stream, no synchronisation.  The kernels clamp what
 * they find in the device copy of the offsets.  A3D_ERR_ARG before any launch: a null pointer, a misaligned buffer, a geometry
 * outside the law (channels outside 1 .. 4, H or W below 1, a raw size above 2^31 - 1), pitch < W, F outside 0 .. 65535, offsets that
 * are not monotonic or do not start at 0 and end at data_bytes, or data_bytes above 2^31 - 1.  F == 0 is a no-op. */
int a3d_png_decode(const a3d_png_decode_desc *d, void *stream);

#ifdef __cplusplus
}
#endif
#endif
