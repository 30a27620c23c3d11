/*
 * cer_hip.h -- C-ABI of libcer_hip.so, the MI355X (gfx950) hot path for
 * feature-based compound emotion recognition.
 *
 * The reference (sbelharbi/feature-vs-text-compound-emotion) is pure Python /
 * torch.nn and has NO native interface.  Each entry point below therefore
 * replaces the stock torch op(s) that the reference executes at the cited
 * file:line; the Python host in feature_vs_text_compound_emotion_amd/ binds
 * them with ctypes and mirrors the reference's nn.Module surface on top.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch tensors keep
 *     them alive); the library never allocates, frees or retains them;
 *   - activations are channels-last: images [N,H,W,C], sequences [B,L,C];
 *   - all launches are asynchronous on the `stream` argument (a hipStream_t
 *     passed as void*; NULL = the default stream); no hidden device sync;
 *   - every function returns 0 on success, a negative cer_status otherwise;
 *     cer_last_error() returns a thread-local description.  No exception or
 *     abort crosses the boundary.
 */
#ifndef CER_HIP_H
#define CER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum cer_status {
    CER_OK = 0,
    CER_ERR_INVALID_ARG = -1,
    CER_ERR_UNSUPPORTED = -2,
    CER_ERR_HIP = -3,
    CER_ERR_WORKSPACE = -4
};

enum cer_act { CER_ACT_NONE = 0, CER_ACT_PRELU = 1, CER_ACT_LEAKY = 2, CER_ACT_RELU = 3, CER_ACT_GELU = 4 };

/* Storage type of the 16-bit tensors of a launch (cer_conv_desc.storage and the *_n16 entry points):
 * 0 = none (fp32 tensors / split hi+lo bf16 pairs, as the pointers say); otherwise every 16-bit tensor is ONE plane of
 * bf16 or IEEE half -- the reference's own GPU recipe is fp16 autocast (trainer.py:14-15,341,367), BASELINE cfg5 asks
 * for "bf16 storage / fp32 accumulate". */
enum cer_storage { CER_STORE_NONE = 0, CER_STORE_BF16 = 1, CER_STORE_F16 = 2 };

const char *cer_last_error(void);
int cer_version(void);

/* ------------------------------------------------------------------------
 * Implicit-GEMM convolution / linear layer on the fp32 matrix cores.
 *
 *   y = act2( mask * act1( conv(affine_in(x), w) + bias ) + residual )
 *
 * Replaces nn.Conv2d + BatchNorm2d + PReLU + residual add
 * (reference models/arcface_model.py:44-60, :130-132), nn.Conv2d + ReLU
 * (models/backbone.py:41-52), the causal dilated nn.Conv1d + Chomp1d +
 * LeakyReLU + residual of models/temporal_convolutional_model.py:21-56, and
 * every nn.Linear on the path (a 1x1 "conv" on an [M,1,1,K] image).
 *
 *   x        [N,H,W,Cin] (or [N,Cin,H,W] when x_nchw != 0; small-Cin path only)
 *   w        [Cout][Kpad], K index = (kh*KW + kw)*Cin + c, zero padded to a
 *            multiple of 32 (cer_conv_kpad)
 *   in_scale/in_shift  [Cin] or NULL: per-channel affine applied to in-bounds
 *            input pixels only (zero padding stays zero) -- the pre-conv
 *            BatchNorm of bottleneck_IR in eval mode
 *   bias     [Cout] or NULL;  alpha [Cout] PReLU slopes (act1 == CER_ACT_PRELU)
 *   residual [N,Hr,Wr,Cout] or NULL, sampled at (ho*res_stride, wo*res_stride)
 *            (MaxPool2d(1,stride) shortcut == spatial subsample)
 *   mask     [N,Ho,Wo,Cout] or NULL (pre-scaled dropout mask)
 *   aux      [N,Ho,Wo,Cout] or NULL: receives mask*act1(conv+bias), the value before
 *            the residual add (saved for the backward pass of a TemporalBlock)
 *   stats    [cer_conv2d_stats_tiles(d, bf16x3)][2][Cout] or NULL: per-tile sum and sum of squares
 *            of the RAW conv result over valid pixels (deterministic partials for the
 *            train-mode BatchNorm that follows; reduce with cer_bn_finalize)
 *   split_k  >= 1; > 1 needs `workspace` of cer_conv2d_workspace_bytes()
 * ---------------------------------------------------------------------- */
typedef struct cer_conv_desc {
    int32_t N, H, W, Cin;
    int32_t Ho, Wo, Cout;
    int32_t KH, KW, stride, dil_h, dil_w, pad_t, pad_l;
    int32_t x_nchw;
    int32_t res_stride, Hr, Wr;
    int32_t act1, act2;
    float slope;          /* LeakyReLU slope */
    int32_t split_k;
    int32_t tile;         /* 0 = auto; else forces a tile config (testing / tuning) */
    int32_t x_ld, y_ld;   /* pitch in floats between pixels of x / rows of y; 0 = dense (Cin / Cout).
                             Lets a layer read or write a column slice of a wider [rows, ld] buffer. */
    int32_t storage;      /* cer_storage: narrow (single 16-bit plane) operands / outputs, see cer_conv_io */
    /* Space-to-depth hand-over between the two 3x3 convs of a stride-2 bottleneck_IR unit (models/arcface_model.py:38-41):
     *   y_s2d != 0: the 16-bit output planes (y_hi / y_lo) are stored as [N, Ho/2, Wo/2, 4*Cout] with
     *       ys[n][i][j][blk*Cout + c] = y[n][2i+py][2j+px][c], blk = 3 - 2*py - px -- same bytes, the stores permuted.
     *       Window / patch kernels only (3x3 / stride 1 / pad 1), even Ho and Wo, no fp32 / second output, no residual.
     *   x_s2d != 0: x_hi / x_lo are such a tensor standing for the [N, H, W, Cin] input of THIS 3x3 / stride 2 / pad 1
     *       conv (H, W even, Cin % 64 == 0 -- narrow storage: % 128 --, Wo <= 126, x_ld = 0), and the K columns of w are
     *       in the kernel's step order (cer_conv_s2d_k_order).  The conv then runs window-resident (conv_b3_s2d_kernel /
     *       conv_n16_s2d_kernel) instead of gathering nine tap tiles per channel chunk.
     *   Split (bf16x3) and narrow operands only. */
    int32_t x_s2d, y_s2d;
} cer_conv_desc;

int cer_conv_kpad(int KH, int KW, int Cin);
/* K-column order of the weights of an x_s2d conv: order[j] (j < 9*Cin) = the column (kh*3 + kw)*Cin + c of the ordinary
 * [Cout][9*Cin] layout that column j of the permuted matrix holds.  chunk = 32 (bf16x3 operands) or 64 (narrow storage):
 * the channels of one kernel step; Cin % (2*chunk) == 0.  Host array of 9*Cin ints. */
int cer_conv_s2d_k_order(int Cin, int chunk, int32_t *order);
size_t cer_conv2d_workspace_bytes(const cer_conv_desc *d);
/* rows of `stats` the launch will write; kernel_family: 0 = fp32 kernel, 1 = bf16x3 (split operands), 2 = narrow (n16) */
int cer_conv2d_stats_tiles(const cer_conv_desc *d, int kernel_family);
int cer_conv2d_fwd(const cer_conv_desc *d, const float *x, const float *w,
                   const float *in_scale, const float *in_shift,
                   const float *bias, const float *alpha,
                   const float *residual, const float *mask,
                   float *y, float *aux, float *stats, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Unified entry point: every operand and output of one conv / linear launch.
 *
 * bf16x3 mode (x_hi != NULL): operands are SPLIT tensors, value = hi + lo with hi = bf16(v),
 * lo = bf16(v - hi) (two bf16 planes, NHWC / [Cout][Kpad] like the fp32 layouts).  Products are
 * evaluated as hi*hi + hi*lo + lo*hi on the bf16 matrix cores with fp32 accumulation: <= 2^-15 relative error per product
 * (|logit error| 1.3e-6 on the full model) at a 5.3x higher matrix ceiling than the fp32 MFMA path.
 * Outputs (any subset): y fp32; (y_hi, y_lo) split; (y2_hi, y2_lo) = split(out*s2[c]+t2[c]), the next
 * layer's eval-mode pre-conv BatchNorm applied by the producer (the zero padding of the consumer
 * then stays exactly zero).  The residual may be fp32 (`residual`) or split (`res_hi`, `res_lo`).
 *
 * Narrow mode (desc.storage = CER_STORE_BF16 / CER_STORE_F16): x_hi, w_hi, res_hi, y_hi are single planes of that type
 * and every *_lo pointer must be NULL; ONE v_mfma_f32_16x16x32_{bf16,f16} per 32-deep product, fp32 accumulate, fp32
 * epilogue (bias / bias9 / PReLU / residual / batch statistics), one rounding at the store.  This is what the
 * reference's --amp recipe computes (fp16 autocast) and BASELINE cfg5's "bf16 storage".  With fp32 operands
 * (x, w given; the Cin = 3 stem) and storage != 0 the fp32 kernel runs and y_hi receives the narrow plane.
 * ---------------------------------------------------------------------- */
typedef struct cer_conv_io {
    const float *x, *w;                       /* fp32 mode operands */
    const uint16_t *x_hi, *x_lo, *w_hi, *w_lo;  /* bf16x3 mode operands */
    const float *in_scale, *in_shift, *bias, *alpha, *residual, *mask;
    const uint16_t *res_hi, *res_lo;
    float *y, *aux, *stats;
    uint16_t *y_hi, *y_lo;
    const float *s2, *t2;
    uint16_t *y2_hi, *y2_lo;
    /* [9][Cout] border-dependent bias (replaces `bias`) of a stride-1 "same" conv whose INPUT BatchNorm was folded
     * into the weights: row 3*ry + rx with ry / rx = 0 on the first, 2 on the last, 1 on the other output rows /
     * columns -- the input shift only contributes through the taps that fall inside the image. */
    const float *bias9;
} cer_conv_io;

int cer_conv2d_run(const cer_conv_desc *d, const cer_conv_io *io, void *workspace, size_t workspace_bytes, void *stream);
/* The bf16x3 kernel variant cer_conv2d_run launches for this descriptor (desc.tile, or the automatic choice when it is 0):
 * 41/42/44/45 = conv_b3_dma16_kernel<128x128 / 128x64 / 64x128 / 64x64>, see csrc/conv_b3.hip.  0 = invalid. */
int cer_conv2d_b3_tile(const cer_conv_desc *d);
/* The narrow kernel variant for this descriptor: 61..67 = conv_n16_kernel tiles (csrc/conv_n16.hip).  0 = invalid. */
int cer_conv2d_n16_tile(const cer_conv_desc *d);

/* v' = v*scale[c]+shift[c] (channels-last; scale/shift may be NULL) -> one 16-bit plane of `storage` (bf16 / half),
 * round-to-nearest-even; and back (tests, fp32 consumers). */
int cer_to_n16(const float *x, const float *scale, const float *shift, int C, uint16_t *out, size_t n, int storage,
               void *stream);
int cer_from_n16(const uint16_t *x, float *out, size_t n, int storage, void *stream);

/* Elementwise passes of the released encoder units that hand a SPLIT tensor (hi / lo bf16 planes) straight to the matrix-core
 * kernels -- replace "torch op -> fp32 tensor -> cer_split_bf16" pairs in the backward of a bottleneck_IR unit
 * (reference models/arcface_model.py:44-60; PReLU :54, BatchNorm2d :53,57):
 *   cer_prelu_split        t = prelu(x) -> split
 *   cer_prelu_bwd_split    torch's PReLU backward; dx as fp32 (dx) and / or split (dx_hi, dx_lo); dalpha_terms as cer_prelu_bwd
 * (cer_bn_rows_bwd_apply writes the BatchNorm backward's dx as a split tensor, or with the shortcut branch's gradient added.) */
int cer_prelu_split(const float *x, const float *alpha, uint16_t *hi, uint16_t *lo, size_t rows, int C, void *stream);
int cer_prelu_bwd_split(const float *dy, const float *x, const float *alpha, float *dx, uint16_t *dx_hi, uint16_t *dx_lo,
                        float *dalpha_terms, size_t rows, int C, void *stream);

/* v' = v*scale[c]+shift[c] (channels-last, C channels; scale/shift may be NULL) -> (bf16(v'), bf16(v' - bf16(v'))),
 * round-to-nearest-even on both parts. */
int cer_split_bf16(const float *x, const float *scale, const float *shift, int C, uint16_t *hi, uint16_t *lo, size_t n,
                   void *stream);

/* Pack an OIHW (torch) conv weight into [Cout][Kpad] with optional per-output
 * scale (BatchNorm fold).  w_oihw [Cout,Cin,KH,KW]; out_scale [Cout] or NULL.
 * transpose != 0 writes the data-gradient filter instead: [Cin][Kpad'] with
 * k = tap*Cout + o (taps flipped when flip != 0), so that
 * dX = cer_conv2d_fwd(dY, packed_T) with the padding mirrored. */
int cer_pack_conv_weight(const float *w_oihw, const float *out_scale, float *w_packed,
                         int Cout, int Cin, int KH, int KW, int flip, int transpose, void *stream);

/* rows x / ||x||_2, no epsilon (reference models/arcface_model.py:17-20). */
int cer_l2norm_rows(const float *x, float *y, int rows, int cols, void *stream);

/* Backward of cer_l2norm_rows: x is the forward INPUT; dx = (dy - y (y.dy)) / ||x|| with y = x/||x||.  Used when the
 * encoder head is released for training (reference base/parameter_control.py:55-103, first release group). */
int cer_l2norm_rows_bwd(const float *dy, const float *x, float *dx, int rows, int cols, void *stream);

/* max-pool 2x2 stride 2 on NHWC (reference models/backbone.py:45-46). */
/* ------------------------------------------------------------------------
 * IR-50 input layer: Conv2d(3, 64, 3x3, stride 1, pad 1) [+ BatchNorm2d + PReLU] (reference models/arcface_model.py:130-132,
 * :148) as a direct convolution on the vector ALUs -- the layer is write-bound (27 multiply-adds per output value), so in
 * model.train() it is cheaper to run it twice than to store its raw result for the batch-statistics BatchNorm:
 *   statistics pass (y, y_hi, y_lo, scale, shift, alpha all NULL): stats [cer_stem_conv3x3_stats_rows(N, H)][2][64] receives the
 *       per-block sum / sum of squares of the RAW conv result (reduce with cer_bn_finalize);
 *   apply pass (an output given): out = prelu(conv * scale[c] + shift[c], alpha[c]) (NULL scale / shift / alpha = 1 / 0 / none)
 *       stored as fp32 (y) and / or split bf16 planes (y_hi, y_lo; storage = 0) or ONE narrow plane (y_hi; storage =
 *       CER_STORE_BF16 / CER_STORE_F16); stats (optional) then receives the partial statistics of `out`.
 * x [N, 3, H, W] fp32 (NCHW frames as the reference feeds them); w [64][Kpad] packed like every conv weight
 * (K index = (kh*3 + kw)*3 + c, Kpad = cer_conv_kpad(3, 3, 3)); outputs NHWC [N, H, W, 64]. */
int cer_stem_conv3x3_stats_rows(int N, int H);
int cer_stem_conv3x3(const float *x, const float *w, int Kpad, const float *scale, const float *shift, const float *alpha,
                     float *y, uint16_t *y_hi, uint16_t *y_lo, int storage, float *stats, int N, int H, int W, void *stream);

int cer_maxpool2x2_nhwc(const float *x, float *y, int N, int H, int W, int C, void *stream);

/* Video-frame input transform of the reference Dataset, fused (base/dataset.py:487-508,
 * base/transforms3D.py:33-143): uint8 frames [n][H][W][3] -> GroupScale(size) (== PIL
 * Image.resize BILINEAR, Pillow's 8-bit fixed-point antialiased triangle filter, reproduced
 * bit for bit) -> crop (x1, y1) to crop x crop -> optional horizontal flip -> /255 -> (v - mean) / std,
 * written as fp32 [n][3][crop][crop] (and optionally the uint8 HWC image before the float stage).
 * hbounds/vbounds [size][2] = (first input index, tap count); hcoef/vcoef [size][ksize] = Pillow's
 * integer coefficients (2^22 scale), computed by the host.  crop_xyf [groups][3] = (x1, y1, flip), one
 * triple per `frames_per_group` consecutive frames (GroupRandomCrop / GroupRandomHorizontalFlip draw
 * once per clip).  max_band_rows = the largest number of input rows any band of cer_frames_band_rows()
 * output rows needs (sizes the LDS). */
int cer_frames_band_rows(void);
int cer_frames_transform(const uint8_t *frames, int n_frames, int H, int W, const int32_t *hbounds, const int32_t *hcoef,
                         int hksize, const int32_t *vbounds, const int32_t *vcoef, int vksize, int size, int crop,
                         const int32_t *crop_xyf, int frames_per_group, int max_band_rows, float mean, float stdv,
                         float *out, uint8_t *out_u8, void *stream);

/* ------------------------------------------------------------------------
 * Trainable tail (rows = B*L frames, channels-last).  Forward AND backward,
 * because this is the part of the model the reference actually trains
 * (models/model.py:432-433 freezes the encoders).
 * ---------------------------------------------------------------------- */

/* torch.nn.utils.weight_norm(dim=0): w = g*v/||v|| per output row of E = Cin*k
 * elements (reference models/temporal_convolutional_model.py:24,30).  norm [rows] is saved
 * for the backward, which returns dv [rows,E] and dg [rows]. */
int cer_weight_norm_fwd(const float *v, const float *g, float *w, float *norm, int rows, int E, void *stream);
int cer_weight_norm_bwd(const float *dw, const float *v, const float *g, const float *norm,
                        float *dv, float *dg, int rows, int E, void *stream);
/* The same forward for a [Cout][Cin][k] 1-D filter, writing in the same launch the two packed layouts the conv kernels read
 * (cer_pack_conv_weight's): wp_fwd [Cout][cer_conv_kpad(k,1,Cin)] and the flipped, transposed data-gradient filter
 * wp_dgrad [Cin][cer_conv_kpad(k,1,Cout)] -- the TCN (temporal_convolutional_model.py:24-38) re-normalises every step. */
int cer_weight_norm_fwd_packed(const float *v, const float *g, float *w, float *norm, float *wp_fwd, float *wp_dgrad, int Cout,
                               int Cin, int k, void *stream);
/* The backward on the weight-gradient kernel's split partial slabs [splits][rows * E] (summed in the order 0 .. splits-1). */
int cer_weight_norm_bwd_partials(const float *dw_parts, int splits, const float *v, const float *g, const float *norm, float *dv,
                                 float *dg, int rows, int E, void *stream);

/* Weight gradient of the causal dilated conv1d / linear layers:
 * dW[co][ci][j] = sum_r dZ[r][co] * X[r-(k-1-j)*dil][ci], rows never cross a length-L sequence.
 * dz [R,dz_ld], x [R,x_ld], dw [Cout,Cin,k] (torch layout).  Linear: k = 1. */
/* workspace (optional; both kernels below): with cer_conv_wgrad_workspace_bytes(R, Cout, Cin, k) bytes the rows are split over
 * blocks and the partial results added in a fixed order (the tail's layers have R = B * L = 1024 rows and few output tiles);
 * without it (NULL / too small) one block per tile and tap walks all rows. */
size_t cer_conv_wgrad_workspace_bytes(long long R, int Cout, int Cin, int k);
int cer_conv1d_wgrad(const float *dz, int dz_ld, const float *x, int x_ld, float *dw,
                     int R, int L, int Cout, int Cin, int k, int dil, void *workspace, size_t workspace_bytes, void *stream);
/* cer_conv1d_wgrad of a weight-normed conv followed by its weight-norm backward, in two launches: (dv, dg) instead of dW.
 * workspace: max(cer_conv_wgrad_workspace_bytes(R, Cout, Cin, k), Cout * Cin * k * 4) bytes. */
int cer_conv1d_wgrad_weight_norm_bwd(const float *dz, int dz_ld, const float *x, int x_ld, int R, int L, int Cout, int Cin, int k,
                                     int dil, const float *v, const float *g, const float *norm, float *dv, float *dg,
                                     void *workspace, size_t workspace_bytes, void *stream);

/* 2-D weight gradient (encoder units released for training, reference base/parameter_control.py:55-103):
 * dW[co][ci][kh][kw] = sum over output pixels (n,ho,wo) of dZ[n,ho,wo,co] * X[n, ho*stride-pad_t+kh, wo*stride-pad_l+kw, ci]
 * (zero outside the image).  dz dense [N*Ho*Wo, Cout], x dense NHWC, dw in torch's OIHW layout. */
int cer_conv2d_wgrad(const float *dz, const float *x, float *dw, int N, int H, int W, int Ho, int Wo, int Cout, int Cin,
                     int KH, int KW, int stride, int pad_t, int pad_l, void *workspace, size_t workspace_bytes, void *stream);
/* The same on the bf16 matrix cores with split hi/lo operands ("bf16x3": three MFMAs per product, <= 2^-15 relative per
 * product, fp32 accumulation), the pixel range split over blocks and reduced in a fixed order: the weight gradient of the
 * reference's released encoder units (base/parameter_control.py:55-103 un-freezes IR-50 stage 4 and half of stage 3; their
 * backward is torch autograd's conv2d weight gradient, models/arcface_model.py:44-60).  Cout and Cin must be multiples of 4
 * (CER_ERR_UNSUPPORTED otherwise: use cer_conv2d_wgrad); the output tile is 128 x 128, so channel counts below 128 waste
 * matrix-core work but stay correct. */
size_t cer_conv2d_wgrad_b3_workspace_bytes(int N, int Ho, int Wo, int Cout, int Cin, int KH, int KW);
int cer_conv2d_wgrad_b3(const float *dz, const float *x, float *dw, int N, int H, int W, int Ho, int Wo, int Cout, int Cin,
                        int KH, int KW, int stride, int pad_t, int pad_l, void *workspace, size_t workspace_bytes, void *stream);
/* The same on operands that are split tensors already (hi / lo bf16 planes, cer_split_bf16): the loader copies instead of
 * converting -- twice as fast when the caller has the split tensors anyway (the released units' convs consume them). */
int cer_conv2d_wgrad_b3s(const uint16_t *dz_hi, const uint16_t *dz_lo, const uint16_t *x_hi, const uint16_t *x_lo, float *dw,
                         int N, int H, int W, int Ho, int Wo, int Cout, int Cin, int KH, int KW, int stride, int pad_t, int pad_l,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Channels-last PReLU with per-channel slopes (arcface_model.py:54).  Backward: dx = x > 0 ? dy : alpha*dy, and
 * dalpha_terms = x > 0 ? 0 : x*dy, whose column sum (cer_col_sum) is the slope gradient. */
int cer_prelu_fwd(const float *x, const float *alpha, float *y, size_t rows, int C, void *stream);
int cer_prelu_bwd(const float *dy, const float *x, const float *alpha, float *dx, float *dalpha_terms, size_t rows, int C,
                  void *stream);

/* out[c] = sum_r a[r][c] * (b ? (b[r][c]-mean[c])*invstd[c] : 1); a == NULL (with b and mean): the centred second moment
 * sum_r ((b[r][c]-mean[c])*invstd[c])^2; deterministic tree.
 * Bias gradients and the BatchNorm / LayerNorm parameter gradients. */
size_t cer_col_sum_workspace_bytes(int R, int C);
int cer_col_sum(const float *a, int a_ld, const float *b, int b_ld, const float *mean, const float *invstd,
                float *out, int R, int C, void *workspace, size_t workspace_bytes, void *stream);

/* dz = dy * mask * leaky'(y) for y = mask*leaky(z)  (Dropout + LeakyReLU backward). */
int cer_act_mask_bwd(const float *dy, const float *y, const float *mask, float *dz, size_t n, float slope, void *stream);
/* TemporalBlock tail out = leaky(a2 + res), a2 = mask2*leaky(z2):
 * du = dout*leaky'(out)  (gradient of res and of a2),  dz2 = du*mask2*leaky'(a2). */
int cer_tblock_tail_bwd(const float *dout, const float *out, const float *a2, const float *mask2,
                        float *du, float *dz2, size_t n, float slope, void *stream);

/* BatchNorm1d over rows (reference models/model.py:475,515).  train != 0: batch statistics,
 * running stats updated in place (unbiased variance, `momentum`), save_mean/save_invstd written.
 * train == 0: running statistics. */
size_t cer_bn_rows_fwd_workspace_bytes(int R, int C);   /* 0 for R <= 2048; larger R reduce the statistics in two column sums */
/* y == NULL with train != 0: statistics pass alone (save_mean / save_invstd, running buffers updated), nothing is written --
 * the released encoder units apply the normalisation inside the pass that follows (affine + split, or cer_bn_apply_nhwc
 * with the shortcut add), so the separate apply pass over the activation would be read-once-write-once traffic for nothing. */
int cer_bn_rows_fwd(const float *x, int x_ld, const float *w, const float *b, float *running_mean,
                    float *running_var, float *save_mean, float *save_invstd, float *y, int y_ld,
                    int R, int C, int train, float eps, float momentum, void *workspace, size_t workspace_bytes, void *stream);

/* The row BatchNorm split at its statistics, so that a cross-rank exchange can sit between the local reduction
 * and its use (synchronised BatchNorm over data-parallel ranks).  Forward:
 *   cer_bn_rows_moments  moments [3][C] float64 = (count, mean, M2 = sum (x - mean)^2) of the rows of x (pitch x_ld);
 *   cer_bn_rows_merge    K gathered moment blocks [K][3][C] merged in block order (Chan's pairwise update) -> save_mean,
 *                        save_invstd (1 / sqrt(var + eps), biased var) and, when non-NULL, the running update with the
 *                        unbiased variance of the union; every caller with the same blocks gets the same bits;
 *   cer_bn_rows_apply    y = (x - mean) * invstd * w + b, y with pitch y_ld (a column slice of a wider buffer).
 * Backward, in two calls so that the same exchange can sit between them (local BatchNorm: the local sums, count = R):
 *   cer_bn_rows_bwd_sums   sums [2][C] float32 = (sum dy, sum dy * x_hat) over the local rows -- db and dw of this rank; one
 *                          pass over dy and x when the rows are dense, C % 4 == 0 and R spans several slabs, two column sums
 *                          otherwise; workspace as cer_col_sum;
 *   cer_bn_rows_bwd_apply  train != 0: dx = w * invstd * (dy - (sum_dy + x_hat * sum_dy_xhat) / count) with sums and count of
 *                          the batch the statistics were taken over, for the local rows; train == 0: dx = dy * w * invstd.
 *                          The outputs given pick the pass: dx_hi and dx_lo -> dx as a split tensor (hi / lo bf16 planes);
 *                          else add -> fp32 dx = BatchNorm-backward(dy) + add (add may alias dx), the gradient of a released
 *                          encoder unit's input as the sum of its residual branch (through the unit's first BatchNorm) and
 *                          its shortcut branch (models/arcface_model.py:58-60) in one pass; else fp32 dx with pitches dy_ld /
 *                          x_ld.  The split and addend forms are train mode over dense rows, C % 4 == 0, 16-byte aligned. */
int cer_bn_rows_moments(const float *x, int x_ld, int R, int C, double *moments, void *stream);
int cer_bn_rows_merge(const double *moments, int K, int C, float eps, float momentum, float *save_mean, float *save_invstd,
                      float *running_mean, float *running_var, void *stream);
int cer_bn_rows_apply(const float *x, int x_ld, const float *mean, const float *invstd, const float *w, const float *b,
                      float *y, int y_ld, int R, int C, void *stream);
int cer_bn_rows_bwd_sums(const float *dy, int dy_ld, const float *x, int x_ld, const float *save_mean, const float *save_invstd,
                         float *sums, int R, int C, void *workspace, size_t workspace_bytes, void *stream);
int cer_bn_rows_bwd_apply(const float *dy, int dy_ld, const float *x, int x_ld, const float *save_mean,
                          const float *save_invstd, const float *w, const float *sums, double count, int train,
                          const float *add, float *dx, uint16_t *dx_hi, uint16_t *dx_lo, int R, int C, void *stream);
/* The forward statistics of the released encoder units' row BatchNorms (dense rows, C % 4 == 0, 16-byte aligned):
 *   cer_bn_rows_moments_large  moments [3][C] float64 like cer_bn_rows_moments, for any R (up to 51 M rows and R * C > 2^31):
 *                              ONE read of x by many row slabs, each summing about its own first row in fp32, then the slab
 *                              partials merged in float64 in a fixed order (deterministic); workspace of
 *                              cer_bn_rows_moments_large_workspace_bytes(R, C) bytes. */
size_t cer_bn_rows_moments_large_workspace_bytes(int R, int C);
int cer_bn_rows_moments_large(const float *x, int R, int C, double *moments, void *workspace, size_t workspace_bytes, void *stream);

/* LFAN cross-modal attention core (reference models/transformer.py:11-19,133-159): for each
 * (row, head) an M x M softmax over MODALITIES, vals = softmax(q k^T/sqrt(hd)) v + v.
 * qkv[m] [R, H*3*hd] rows laid out [head][q|k|v]; vals [R, H*M*hd]; probs [R,H,M,M] saved. */
int cer_lfan_attn_fwd(const float *const *qkv, float *vals, float *probs, int R, int H, int M, int hd, void *stream);
int cer_lfan_attn_bwd(const float *const *qkv, const float *dvals, const float *probs, float *const *dqkv,
                      int R, int H, int M, int hd, void *stream);

/* y = LayerNorm(x*mask)*gamma+beta (mask = pre-scaled dropout mask or NULL), rows of C.
 * Backward returns dx w.r.t. the un-masked x; scratch holds R*C floats. */
int cer_layernorm_fwd(const float *x, const float *mask, const float *gamma, const float *beta, float *y, int y_ld,
                      float *save_mean, float *save_rstd, int R, int C, float eps, void *stream);
int cer_layernorm_bwd(const float *dy, int dy_ld, const float *x, const float *mask, const float *gamma,
                      const float *save_mean, const float *save_rstd, float *dx, float *dgamma, float *dbeta,
                      float *scratch, int R, int C, void *workspace, size_t workspace_bytes, void *stream);

/* nn.CrossEntropyLoss(reduction='mean') on [R,C] logits with FLOAT labels cast to long
 * (reference experiment.py:133, trainer.py:380-383); dlogits may be NULL.  Label semantics as torch: -100 (ignore_index)
 * rows are skipped (zero gradient, mean over the other rows); any other value outside [0, C), or NaN, is an error:
 * the row is never dereferenced, loss and that row's gradient become NaN and *bad_labels (device int, may be NULL)
 * receives the number of such rows, which the host wrapper turns into the exception torch raises. */
int cer_cross_entropy(const float *logits, const float *labels, float *loss, float *dlogits, int *bad_labels, int R, int C,
                      void *stream);

/* Train-mode BatchNorm2d inside the vision encoder (the reference's model.train() also puts
 * the frozen IR-50's BatchNorms in batch-statistics mode).
 * cer_bn_finalize: reduce `tiles` partial rows [tiles][2][C] (sum, sum of squares over `count`
 * elements per channel) in double precision -> scale = gamma*invstd, shift = beta - mean*scale;
 * updates running_mean/var in place (unbiased variance, `momentum`) when non-NULL.
 * cer_bn_apply_nhwc: out = mask * prelu(y*scale+shift) + (res*res_scale+res_shift), residual
 * sampled with res_stride like the conv epilogue; optionally emits the partial statistics of
 * `out` ([cer_bn_apply_stats_tiles(P)][2][C]) for the next BatchNorm. */
size_t cer_bn_finalize_workspace_bytes(int tiles, int C);
int cer_bn_finalize(const float *partials, int tiles, int C, double count, const float *gamma, const float *beta,
                    float *running_mean, float *running_var, float momentum, float eps,
                    float *scale, float *shift, void *workspace, size_t workspace_bytes, void *stream);
/* cer_bn_finalize in two steps, for statistics synchronised across data-parallel ranks (the all-reduce of `sums` goes
 * between them): cer_bn_partial_sums reduces the partials exactly as cer_bn_finalize does into sums [2][C] float64
 * (sum | sum of squares; workspace as cer_bn_finalize), cer_bn_finalize_sums applies cer_bn_finalize's formula to sums over
 * `count` elements.  With one rank the pair gives cer_bn_finalize's bits. */
int cer_bn_partial_sums(const float *partials, int tiles, int C, double *sums, void *workspace, size_t workspace_bytes,
                        void *stream);
int cer_bn_finalize_sums(const double *sums, int C, double count, const float *gamma, const float *beta, float *running_mean,
                         float *running_var, float momentum, float eps, float *scale, float *shift, void *stream);
int cer_bn_apply_stats_tiles(int P);
int cer_bn_apply_nhwc(const float *y, const float *scale, const float *shift, const float *alpha,
                      const float *res, const float *res_scale, const float *res_shift, const float *mask,
                      float *out, float *stats, int N, int Ho, int Wo, int C, int res_stride, int Hr, int Wr,
                      void *stream);
/* The same pass for the bf16x3 encoder: the residual may come as a split tensor (res_hi/res_lo instead of res) and
 * the result is stored split (out_hi/out_lo) -- what the next conv reads directly -- and/or as fp32 (`out`); the
 * statistics are taken from the fp32 value before the split. */
int cer_bn_apply_nhwc_b3(const float *y, const float *scale, const float *shift, const float *alpha, const float *res,
                         const uint16_t *res_hi, const uint16_t *res_lo, const float *res_scale, const float *res_shift,
                         const float *mask, float *out, uint16_t *out_hi, uint16_t *out_lo, float *stats, int N, int Ho,
                         int Wo, int C, int res_stride, int Hr, int Wr, void *stream);

/* The same pass on NARROW tensors (cer_storage: one bf16 / half plane each): the conv result comes as fp32 (`y`) or narrow
 * (`y16`, exactly one of the two), the residual as fp32 or narrow, the result goes to `out16` and/or fp32 `out`;
 * arithmetic and statistics are fp32 (taken before the final rounding).  16-byte accesses: C % 8 == 0. */
int cer_bn_apply_nhwc_n16(const float *y, const uint16_t *y16, const float *scale, const float *shift, const float *alpha,
                          const float *res, const uint16_t *res16, const float *res_scale, const float *res_shift,
                          const float *mask, float *out, uint16_t *out16, float *stats, int N, int Ho, int Wo, int C,
                          int res_stride, int Hr, int Wr, int storage, void *stream);

/* Fold the per-input-channel affine (scale, shift) of a BatchNorm in FRONT of a 3x3 / stride 1 / pad 1 conv into the conv
 * (reference arcface_model.py:53-54: BatchNorm2d -> Conv2d; in model.train() the affine only exists after the batch
 * reduction): w_packed [Cout][Kpad] (cer_pack_conv_weight) -> w * scale[c] as fp32 (w_f32), split hi/lo (w_hi, w_lo,
 * storage 0) or one narrow plane (w_hi, storage bf16 / f16), plus bias9 [9][Cout] (see cer_conv_io.bias9).  One launch. */
int cer_fold_bn_3x3(const float *w_packed, const float *scale, const float *shift, int Cout, int Cin, float *w_f32,
                    uint16_t *w_hi, uint16_t *w_lo, int storage, float *bias9, void *stream);

/* Nesterov SGD over flat buffers (reference instantiators.py:74-92: torch.optim.SGD(momentum .9, nesterov, wd 1e-4);
 * trainer.py:385-391): d = grad + wd*p; buf = first_step ? d : mu*buf + (1-damp)*d; d = nesterov ? d + mu*buf : buf;
 * p -= lr*d -- torch's _single_tensor_sgd operation by operation, one launch for the whole model.  n % 4 == 0,
 * 16-byte aligned buffers. */
int cer_sgd_nesterov_flat(float *param, const float *grad, float *momentum_buf, size_t n, float lr, float momentum,
                          float dampening, float weight_decay, int nesterov, int first_step, void *stream);

/* torch.optim.Adam(betas, eps, weight_decay, amsgrad) over flat buffers (reference instantiators.py:81-92; L2 weight decay,
 * not AdamW), step `step` >= 1 (the count AFTER this update, as torch's state['step']): d = grad + wd*p; m = lerp(m, d, 1-b1);
 * v = b2*v + (1-b2)*d*d; amsgrad: vmax = max(vmax, v); p += step_size * m / (sqrt(v or vmax) / bc2_sqrt + eps) with
 * step_size = -lr / (1 - b1^step), bc2_sqrt = sqrt(1 - b2^step) computed here in double -- the non-capturable branch of
 * torch's _multi_tensor_adam element by element, one launch.  max_exp_avg_sq may be NULL unless amsgrad; n % 4 == 0,
 * 16-byte aligned buffers. */
int cer_adam_flat(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *max_exp_avg_sq, size_t n,
                  double lr, double beta1, double beta2, double eps, double weight_decay, int amsgrad, int64_t step,
                  void *stream);

/* Loss scaling over the flat buffers (torch.amp.GradScaler's contract for an optimiser with _step_supports_amp_scaling), no host
 * read of device state.  cer_amp_check_unscale_flat: torch._amp_foreach_non_finite_check_and_unscale_ over the whole bucket in
 * one launch -- *found_inf = 1.0f if any input element is Inf / NaN (never reset), and, when inv_scale (a device scalar) is
 * given, every element becomes *inv_scale == 1 ? g : g * *inv_scale; inv_scale NULL: check only, grad is not written.
 * n % 4 == 0, grad 16-byte aligned. */
int cer_amp_check_unscale_flat(float *grad, size_t n, const float *inv_scale, float *found_inf, void *stream);

/* cer_sgd_nesterov_flat / cer_adam_flat with a device-side skip: if *found_inf != 0 nothing changes (parameters, moments,
 * *applied); otherwise, when grad_scale is given, each gradient is first unscaled by (float)(1 / (double)*grad_scale) and
 * written back into grad, then the update runs with the per-element arithmetic of the plain entry points, and *applied (the
 * device-resident count of applied steps, int64) is incremented by a second one-thread launch on the same stream.  SGD: the
 * momentum buffer is initialised on the first applied step (*applied == 0).  Adam: step k = *applied + 1 reads
 * bias_correction[2(k-1)] = 1 - beta1^k and bias_correction[2(k-1)+1] = sqrt(1 - beta2^k) (double, host-computed; k is
 * clamped to table_len, whose last entry must then hold for every later k) and forms -lr / (1 - beta1^k) in double. */
int cer_sgd_nesterov_flat_amp(float *param, float *grad, float *momentum_buf, size_t n, float lr, float momentum,
                              float dampening, float weight_decay, int nesterov, const float *grad_scale, const float *found_inf,
                              int64_t *applied, void *stream);
int cer_adam_flat_amp(float *param, float *grad, float *exp_avg, float *exp_avg_sq, float *max_exp_avg_sq, size_t n,
                      double lr, double beta1, double beta2, double eps, double weight_decay, int amsgrad,
                      const double *bias_correction, int64_t table_len, const float *grad_scale, const float *found_inf,
                      int64_t *applied, void *stream);

/* out[i][:] = src[index[i]][:], zeros where index[i] < 0 or >= n_src: the token -> frame spreading of the BERT rows
 * (abaw5_pre_processing/base/speech.py:690-738) and the edge-padded frame indexing of VGGish rows
 * (base/preprocessing.py:992-1018); the index plan is host logic.  cols % 4 == 0. */
int cer_gather_rows(const float *src, const int64_t *index, float *out, int n_out, int cols, int64_t n_src, void *stream);

/* Token rows of one or more sentences -> the rows of spans of frames, the index plan formed in the kernel
 * (speech.py:690-738, align_word_embedding_new).  tok [tok_rows][hidden]; segments [n_segments][4] int32 = (out_first,
 * n_frames, n_tokens, index_first); tok_index [n_index] int32; out [out_rows][hidden]; all device pointers.  For segment g
 * and 0 <= i < n_frames, with n = min(n_tokens, n_frames) and q, r = divmod(n_frames, n):
 *   out[out_first + i][:] = tok[tok_index[index_first + j(i)]][:],  j(i) = i / (q + 1) if i < r (q + 1), else
 *   r + (i - r (q + 1)) / q   (the first r tokens get one frame more; tokens beyond the frame count are dropped);
 *   n <= 0: the row becomes zeros.  Rows of out that no segment covers are not written; the caller keeps the segments'
 * output ranges disjoint.  The tables are never trusted with an address: output rows outside [0, out_rows) are skipped, the
 * index position is clamped into [0, n_index) and the token row into [0, tok_rows).  Null pointers, sizes < 1,
 * hidden % 4 != 0 and tok / out / segments not 16-byte aligned return CER_ERR_INVALID_ARG before any launch. */
int cer_text_spread_rows(const float *tok, int64_t tok_rows, int hidden, const int32_t *segments, int n_segments,
                         const int32_t *tok_index, int n_index, float *out, int64_t out_rows, void *stream);

/* The reference's standardisation of the vggish and bert rows (base/dataset.py:516-539 wraps them in
 * transforms.Normalize(mean, std); the statistics are base/dataset.py:272-325), csrc/feature_norm.hip.
 *
 * cer_feature_moments_update: rows [M][C] fp32 dense, acc [2][C] float64, both device memory:
 *   acc[0][c] += sum_m rows[m][c],  acc[1][c] += sum_m rows[m][c]^2,
 * float64 adds in ascending row order per column, nothing else: the bits of acc depend on the sequence of rows only, not
 * on how it was split over calls (the calls of one stream are ordered).  No atomics.  NaN / Inf propagate per column.
 *
 * cer_standardize_rows: out[m][c] = (x[m][c] - mean[c]) / std[c] in fp32, one subtraction and one correctly rounded
 * division (tensor.sub_(mean).div_(std)); mean, std [C] fp32; out == x is allowed; C % 4 == 0, float4 moves.
 *
 * Both refuse with CER_ERR_INVALID_ARG before any launch, the entry's name at the head of cer_last_error(): a null pointer,
 * M < 1, C outside [1, 2^20] (standardize: [4, 2^20] and C % 4 != 0), M * C >= 2^31, rows not 4-byte / acc not 8-byte aligned
 * (standardize: x, mean, std, out not 16-byte aligned). */
int cer_feature_moments_update(const float *rows, int64_t M, int C, double *acc, void *stream);
int cer_standardize_rows(const float *x, int64_t M, int C, const float *mean, const float *std, float *out, void *stream);

/* ------------------------------------------------------------------------
 * Audio / text encoder front ends and attention.
 * ---------------------------------------------------------------------- */

/* VGGish log-mel front end (reference abaw5_pre_processing/base/vggish/mel_features.py:75-114,
 * 207-236; vggish_input.py:84-98): pcm [clips][num_samples] int16 at 16 kHz -> /32768 -> `pad_samples`
 * of edge padding -> periodic-Hann 400/160 frames -> |DFT 512| -> mel_matrix [257][64] (float64,
 * host-computed constant) -> log(x + log_offset).  logmel [clips][cer_logmel_num_frames()][64] fp32;
 * the DFT and mel product run in float64 like the reference's numpy. */
int cer_logmel_num_frames(int num_samples, int pad_samples);
int cer_logmel_fwd(const int16_t *pcm, int clips, int num_samples, int pad_samples, const double *mel_matrix,
                   float log_offset, float *logmel, void *stream);
/* The same log-mel on samples that already are float64 in [-1, 1) (the output of cer_resample_pcm), with no padding:
 * samples [clips][num_samples] -> logmel [clips][cer_logmel_num_frames(num_samples, 0)][64].  One kernel template, two
 * sample types; clips <= 65535. */
int cer_logmel_f64_fwd(const double *samples, int clips, int num_samples, const double *mel_matrix, float log_offset,
                       float *logmel, void *stream);
/* Mixdown + edge padding + polyphase resampling ahead of the log-mel (vggish_input.py:51-56,93-98; the reference calls
 * resampy.resample): pcm [clips][num_samples][channels] int16 ->
 *   x[k] = mean over channels of pcm[k][:] / 32768 for k < num_samples, x[num_samples - 1] for the `pad_samples` after
 *   that, 0 outside;   out[c][n] = sum_j taps[r][j] * x[q - J + j],  q = (n M) div L, r = (n M) mod L, J = (T - 2) / 2
 * in float64.  taps [L][T] float64 (T even, >= 2) is device memory built by the caller
 * (audio_backbone.resample_taps: a Kaiser-windowed sinc at the L phases); out [clips][n_out] float64; clips <= 65535.
 * Any n_out is memory-safe: inputs outside the padded signal read as zero. */
int cer_resample_pcm(const int16_t *pcm, int clips, int num_samples, int channels, int pad_samples, const double *taps,
                     int L, int M, int T, int n_out, double *out, void *stream);
/* examples[c][e][f][:] = logmel[c][starts[e]+f][:] (my_frame, mel_features.py:21-49; the caller
 * computes `starts` with the reference's round-half-to-even rule).  `starts` is device memory and is NOT bounds-checked
 * here: every start must lie in [0, frames_per_clip - win].  The tensor wrapper (ops.frame_examples) takes the starts as
 * host integers, refuses any outside that range before the launch and uploads them itself. */
int cer_frame_examples(const float *logmel, const int *starts, float *examples, int clips, int frames_per_clip,
                       int n_examples, int win, void *stream);

/* BERT embeddings: y[b][s] = LayerNorm(word[ids[b][s]] + pos[s] + type[0]) (transformers
 * BertEmbeddings; reference call site abaw5_pre_processing/base/speech.py:603-606). ids int64.
 * An id outside [0, vocab) is CLAMPED to the nearest valid row (id < 0 reads row 0, id >= vocab reads row vocab - 1);
 * nn.Embedding raises instead, which BertEncoderHIP.forward restates for ids that arrive on the host.  S > max_pos is
 * CER_ERR_INVALID_ARG. */
int cer_bert_embed_ln(const long long *ids, const float *word, const float *pos, const float *type,
                      const float *gamma, const float *beta, float *y, int B, int S, int Hd, int vocab,
                      int max_pos, float eps, void *stream);

/* out = softmax(q k^T * scale + key mask) v on the fp32 matrix cores (flash style, exact fp32).
 * Element (b, s, h, d) of a tensor sits at ptr + b*strides[0] + s*strides[1] + h*strides[2] + d.
 * key_mask [B][Sk] (1 = attend) or NULL.  D in {32, 64, 128}.  Replaces BertSelfAttention and the
 * nn.MultiheadAttention of the JMT/MT heads (reference models/model.py:716-750, 967-972).
 * lse [B][H][Sq] (optional, dense) receives log(sum_k exp(score)) over the visible keys.
 * Degenerate rows: a query with NO visible key (its batch row's mask is all zero) gets out = 0 and lse = +inf, never NaN
 * (torch's softmax returns NaN there).  Rows query >= Sq of out / lse are never written, keys >= Sk never read. */
int cer_attention_fwd(const float *q, const float *k, const float *v, const int *key_mask, float *out, float *lse,
                      int B, int H, int Sq, int Sk, int D, const long long *q_strides, const long long *k_strides,
                      const long long *v_strides, const long long *o_strides, float scale, void *stream);
/* Backward of cer_attention_fwd (JMT/MT heads train through nn.MultiheadAttention).  lse [B,H,Sq] is the
 * forward's optional output; delta [B,H,Sq] is scratch.  Two recompute passes (one owning queries, one
 * owning keys), no atomics: deterministic.  dout may have other strides than out (do_strides).
 * Degenerate rows: a query whose lse is +inf (no visible key) has P = exp(score - inf) = 0 everywhere, so its dq = 0 and it
 * adds nothing to dk or dv; a masked key gets dk = dv = 0.  Every row < Sq of dq and < Sk of dk / dv is written (zeros
 * included), no row beyond them is. */
int cer_attention_bwd(const float *q, const float *k, const float *v, const float *out, const float *dout,
                      const float *lse, const int *key_mask, float *delta, float *dq, float *dk, float *dv,
                      int B, int H, int Sq, int Sk, int D, const long long *q_strides, const long long *k_strides,
                      const long long *v_strides, const long long *o_strides, const long long *do_strides,
                      const long long *dq_strides, const long long *dk_strides, const long long *dv_strides,
                      float scale, void *stream);

/* ------------------------------------------------------------------------
 * Evaluation path on the device (reference trainer.py:436-523, 832-892; metrics.py:43-193).
 * ---------------------------------------------------------------------- */

/* Stitch the outputs of the sliding inference windows of ONE video (trainer.py:832-892): out[f][c] = sum over the windows
 * covering frame f, in window order, of win_out[w][f - starts[w]][c], divided by the number of such windows.
 * win_out [nw][Lw][C], starts [nw] (device int32), out [total][C].  The caller keeps every window inside the video and
 * every frame inside a window (eval_device.py checks both before the launch): a frame no window covers is written as 0,
 * where the reference's 0 / 0 gives NaN. */
int cer_window_stitch(const float *win_out, const int *starts, int nw, int Lw, int C, int total, float *out, void *stream);

/* cer_window_stitch for V videos in one launch.  win_out [nw][Lw][C] holds the videos' windows, video after video, each in
 * window order; video v owns windows [win_offsets[v], win_offsets[v+1]) and rows [frame_offsets[v], frame_offsets[v+1]) of
 * out [R][C]; win_start[w] is window w's start frame inside its own video.  All pointers are device pointers (int32 offsets,
 * V+1 entries each).  Every element equals the one-video cer_window_stitch result bit for bit. */
int cer_window_stitch_multi(const float *win_out, const int *win_start, const int *win_offsets, const int *frame_offsets,
                            int V, int nw, int Lw, int C, int R, float *out, void *stream);

/* cer_window_stitch on live streams: the frames that became final, stitched from a ring of each stream's last window outputs.
 * wring [S][K][W][C] fp32: regular window i of a stream (frames [i H, i H + W)) sits in slot i % (K - 1), slot K - 1 holds
 * its tail window [n - W, n) or its single short window [0, n), n < W.  row_stream / row_frame [P] (device int32): row p of
 * out [P][C] is frame row_frame[p] of stream row_stream[p]; win_done / tail_start [S] (device int32): the stream's regular
 * windows done so far and the start of its tail window (-1: none).  Per element the regular windows still in the ring
 * (win_done - (K - 1) .. win_done - 1) are walked in ascending start, then the tail: a float sum from 0.f and one division by
 * (float)count, the bits of cer_window_stitch on the same window outputs; a frame no live window covers is written as 0.
 * The tables are never trusted with an address: the stream is clamped into [0, S), slots are remainders modulo K - 1, window
 * rows outside [0, W) are skipped.  Null pointers, S, W, C, H or P < 1, K < 2, H > W and buffers that are not 4-byte aligned
 * return CER_ERR_INVALID_ARG before any launch. */
int cer_window_stitch_stream(const float *wring, int S, int K, int W, int C, int H, const int32_t *row_stream,
                             const int32_t *row_frame, int P, const int32_t *win_done, const int32_t *tail_start, float *out,
                             void *stream);

/* Accumulate (+=) the confusion counts of a batch of V videos: logits [R][C] (the videos' frames concatenated), labels [R]
 * (float class ids), video_offsets [V+1] (device int32 row offsets; the caller makes them rise strictly from 0 to R, the
 * kernels read rows [video_offsets[v], video_offsets[v+1]) unchecked).  Every argmax is numpy.argmax: the first NaN if
 * there is one, otherwise the first maximum.  frame_cm [C][C]: counts[label][argmax]; video_cm
 * [3][C][C]: the same per video for the reference's three frame -> video decisions (majority vote / mean logits / mean
 * softmax probabilities, metrics.py:118-139); ignore_class >= 0 drops the LAST logit column and skips frames / videos
 * labelled ignore_class (C-EXPR-DB's 'Other', metrics.py:62-84); video_pred [V][3] (optional) receives the decisions;
 * *bad counts labels outside [0, C) and videos with mixed labels (the reference asserts on those).  F1 / accuracy / the
 * normalised confusion matrix are functions of these counts (host side: one [4][C][C] copy per evaluation). */
int cer_eval_accumulate(const float *logits, const float *labels, const int *video_offsets, int V, int R, int C,
                        int ignore_class, unsigned long long *frame_cm, unsigned long long *video_cm, int *video_pred, int *bad,
                        void *stream);

/* ------------------------------------------------------------------------
 * The regression task (reference models/model.py:400,523,681,1164; base/loss_function.py; base/logger.py:213-351).
 * ---------------------------------------------------------------------- */

/* y = tanh(x), elementwise fp32 (the REGRESSION output of LFAN / CAN / JMT / MT).  tanh is evaluated in double and rounded
 * once.  +-inf -> +-1, NaN -> NaN, |x| >= 20 -> exactly +-1.  Backward from the saved output: dx = dy * (1 - y * y), the
 * product taken in double and rounded once. */
int cer_tanh_fwd(const float *x, float *y, size_t n, void *stream);
int cer_tanh_bwd(const float *dy, const float *y, float *dx, size_t n, void *stream);

/* The reference's CCCLoss(gold, pred) with weights=None (base/loss_function.py:6-24) and its gradient with respect to pred.
 * gold, pred [B][L][D] dense; *loss one float; dpred [B][L][D] or NULL; col_ws [B * D] doubles of scratch.  Per column
 * (b, d), n = L: means gm, pm; S = sum (g - gm)(p - pm); Vg, Vp the unbiased variances; m = gm - pm; Q = Vg + Vp + m^2;
 *   loss = (1 / N) sum over columns of (L - 2 S / Q),                                   N = B * L * D
 *   dpred[j] = ( -2 (g_j - gm) / Q + (2 S / Q^2) (2 (p_j - pm) / (n - 1) - 2 m / n) ) / N.
 * All sums are double: one 256-thread block per column (two passes, wave shuffles, fixed-order LDS tree), then one block
 * adds the column terms in index order.  No atomics: two calls give identical bits.  The reference's `+ 1e-50` is 0 in its
 * fp32 arithmetic and is not added: a column with Q = 0 (gold and pred the same constant) or L = 1 gives a NaN loss and a
 * NaN gradient in THAT column only, as the reference does. */
int cer_ccc_loss(const float *gold, const float *pred, float *loss, float *dpred, double *col_ws, int B, int L, int D,
                 void *stream);

/* Sufficient statistics of RMSE / Pearson's r / Lin's CCC per video: pred, label [R] (the frames of V videos, concatenated),
 * video_offsets [V+1] (device int32; the caller makes them rise strictly from 0 to R, rows are read unchecked);
 * moments [V][8] double = {n, mean_p, mean_l, M2_p, M2_l, C_pl, SSE, 0} with M2 / C the centred sums and
 * SSE = sum (p - l)^2.  One block per video, two passes, double, fixed-order tree: deterministic. */
int cer_regression_moments(const float *pred, const float *label, const int *video_offsets, int V, int R, double *moments,
                           void *stream);

/* y += x */
int cer_add_inplace(float *y, const float *x, size_t n, void *stream);

/* Pre-scaled dropout keep-mask, a pure function of (seed, offset + i). */
int cer_dropout_mask(float *mask, size_t n, float p, uint64_t seed, uint64_t offset, void *stream);

/* y = x >= 0 ? x : slope*x  (F.leaky_relu between fc1/bn1 and fc2 of the CAN / JMT heads,
 * reference models/model.py:676,1160; backward = cer_act_mask_bwd). */
int cer_leaky_relu_fwd(const float *x, float *y, size_t n, float slope, void *stream);

/* CAN attention-fusion gate (reference models/model.py:561-566): out = softmax(z) * c over rows of C;
 * prob is saved for the backward, which returns dz and dc. */
int cer_softmax_gate_fwd(const float *z, const float *c, float *out, float *prob, int R, int C, void *stream);
int cer_softmax_gate_bwd(const float *dout, const float *prob, const float *c, float *dz, float *dc, int R, int C,
                         void *stream);

/* Elementwise part of a fully-connected layer's backward, one pass over dense-or-pitched rows (the released VGGish
 * embedding layers): dz = da * (a > 0) with a the SAVED post-ReLU output of the layer ([R, C], dense) given as
 * a_kind = CER_FC_ACT_F32 (float), _SPLIT (a = hi plane, a_lo = lo plane), _BF16 / _F16 (one plane); CER_FC_ACT_NONE with
 * a = a_lo = NULL applies no mask (the output layer).  dz goes to the split planes dz_hi / dz_lo (bf16x3 operand; both or
 * neither) and / or to fp32 dz (dense [R, C]); db[c] = sum_r dz[r][c], per-slab partials folded in slab order (no atomics:
 * bit-identical from run to run).  C % 4 == 0, da_ld >= C, a / outputs / workspace 16-byte aligned;
 * workspace: cer_fc_bwd_workspace_bytes(R, C). */
enum cer_fc_act_kind { CER_FC_ACT_NONE = 0, CER_FC_ACT_F32 = 1, CER_FC_ACT_SPLIT = 2, CER_FC_ACT_BF16 = 3, CER_FC_ACT_F16 = 4 };
size_t cer_fc_bwd_workspace_bytes(int R, int C);
int cer_fc_bwd_elem(const float *da, int da_ld, const void *a, const uint16_t *a_lo, int a_kind, uint16_t *dz_hi,
                    uint16_t *dz_lo, float *dz, float *db, int R, int C, void *workspace, size_t workspace_bytes, void *stream);

/* y[r, 0:C] (pitch y_ld) = x[r, 0:C] (pitch x_ld). */
int cer_copy_cols(const float *x, int x_ld, float *y, int y_ld, int R, int C, void *stream);

/* ------------------------------------------------------------------------
 * Streaming TCN: a TemporalBlock (reference models/temporal_convolutional_model.py:21-56) run on c new frames of S streams,
 * its causal taps read from rings of past frames.
 *
 * A ring is [S][R][C] fp32, channels-last, R a power of two.  The device keeps no counters: the host says where the
 * rows of a launch sit, in one of two ways.  An all-zero ring is a stream with no past: exactly the reference's left zero
 * padding.  The two entry families share one validation and launch path and one kernel body; they differ only in how a row
 * finds its stream and position.
 *
 * Lockstep (cer_tcn_stream_conv, cer_tcn_stream_append): all streams advance together: the host keeps the write
 * position `head` in [0, R) and passes it in.  Row (s, i), i < c, is the frame at slot (head + i) & (R - 1).
 *
 * cer_tcn_stream_conv, for every row (s, i) and output channel o:
 *     z   = bias[o] + sum_{j < k, ci < Cin} w[o][j][ci] * ring[s][(head + i - (k - 1 - j) * dil) & (R - 1)][ci]
 *     v   = leaky(z)                                         res_ring == NULL  (a block's first conv)
 *     v   = leaky(leaky(z) + res)                            res_ring != NULL  (its second conv)
 *     res = res_ring[s][(res_head + i) & (res_R - 1)][o]                                   res_w == NULL, res_C == Cout
 *         = res_bias[o] + sum_ci res_w[o][ci] * res_ring[s][(res_head + i) & (res_R - 1)][ci]      the 1x1 downsample
 *   v goes to out_ring[s][(out_head + i) & (out_R - 1)][o] and / or out_dense[s * c + i][o] (either may be NULL, not both).
 *   leaky(t) = t >= 0 ? t : slope * t.  out_ring and out_dense must not overlap any ring the launch reads.
 *   w is packed [Cout4][k][Cin4] with Cout4 / Cin4 the channel counts rounded up to a multiple of 4 and the padding zero;
 *   res_w likewise [Cout4][res_C4].  Packed weights are 16-byte aligned; rings may sit at any float address.
 *   Any Cin, Cout, k, dil >= 1; 1 <= c <= R - (k - 1) * dil.
 *
 * Each output is a fixed-order fp32 sum: it depends on its stream's own history only, never on S, c, head, the number
 * of wraps or the other rows of the launch (no split over workgroups along K, no atomics, no path picked by row count).
 *
 * cer_tcn_stream_append: ring[s][(head + i) & (R - 1)][:] = rows[s * c + i][:] -- the first block's input.
 *
 * Invalid descriptors (null pointers, R not a power of two, head outside [0, R), c too large for R) return
 * CER_ERR_INVALID_ARG before any launch, with a cer_last_error() text that begins with the refusing entry's name.
 *
 * Row table (cer_tcn_stream_conv_rows, cer_tcn_stream_append_rows): streams advance independently.  The M rows of a
 * launch are named by two int32 arrays of length M in device memory: row_stream[m] is the stream of row m and row_pos[m]
 * that frame's position in its own stream, unwrapped, modulo 2^30.  cer_tcn_stream_conv_rows is cer_tcn_stream_conv with
 * s = row_stream[m] and with row_pos[m] in place of head + i, res_head + i and out_head + i alike: tap j reads slot
 * (row_pos[m] - (k - 1 - j) * dil) & (R - 1), the residual and the written slot are row_pos[m] & (res_R - 1) and
 * row_pos[m] & (out_R - 1), and out_dense row m is row m.  Each launch masks row_pos with its own ring lengths, so one
 * table serves every level of a net and there are no per-ring heads.  cer_tcn_stream_append_rows:
 * ring[row_stream[m]][row_pos[m] & (R - 1)][:] = rows[m][:].
 *   A stream's rows in one launch must be consecutive positions and must not exceed max_count.  max_count is the largest
 *   number of rows any one stream has in the table; the host passes it because the entry point cannot read the table.
 *   More rows of a stream than R - (k - 1) * dil would overwrite history that the launch still reads.
 *   The sums, their order and the reduction trees are those of the lockstep entry points: a row's result is the same bits
 *   through either.
 *   The table's contents are never trusted with an address: row_stream[m] is clamped into [0, S) and every slot is masked
 *   by its ring length, so a wrong table gives wrong numbers and never an access outside a ring.
 *   Refused with CER_ERR_INVALID_ARG before any launch: a null table; and, by the checks shared with cer_tcn_stream_conv
 *   (there with M = S * c and max_count = c): a null pointer; M < 1; R, out_R or res_R not a power of two (2^30 is the
 *   largest an int32 holds); (k - 1) * dil + max_count > R; max_count > out_R or res_R; the residual-width and
 *   weight-alignment rules; ceil(M / 8) > 65535.
 * ---------------------------------------------------------------------- */
typedef struct cer_tcn_stream_desc {
    int32_t S, c;              /* streams, new frames per stream */
    int32_t Cin, Cout, k, dil; /* the conv */
    int32_t R, head;           /* the ring the taps read */
    int32_t res_C, res_R, res_head; /* the residual ring (read when res_ring != NULL) */
    int32_t out_R, out_head;   /* the ring written (when out_ring != NULL) */
    float slope;
} cer_tcn_stream_desc;

int cer_tcn_stream_conv(const cer_tcn_stream_desc *d, const float *ring, const float *w, const float *bias,
                        const float *res_ring, const float *res_w, const float *res_bias, float *out_ring, float *out_dense,
                        void *stream);
int cer_tcn_stream_append(const float *rows, float *ring, int S, int c, int C, int R, int head, void *stream);

typedef struct cer_tcn_stream_rows_desc {
    int32_t S, M, max_count;   /* streams, rows in the table, the largest number of rows of one stream */
    int32_t Cin, Cout, k, dil; /* the conv */
    int32_t R;                 /* the ring the taps read */
    int32_t res_C, res_R;      /* the residual ring (read when res_ring != NULL) */
    int32_t out_R;             /* the ring written (when out_ring != NULL) */
    float slope;
} cer_tcn_stream_rows_desc;

int cer_tcn_stream_conv_rows(const cer_tcn_stream_rows_desc *d, const int32_t *row_stream, const int32_t *row_pos,
                             const float *ring, const float *w, const float *bias, const float *res_ring, const float *res_w,
                             const float *res_bias, float *out_ring, float *out_dense, void *stream);
int cer_tcn_stream_append_rows(const float *rows, float *ring, const int32_t *row_stream, const int32_t *row_pos, int S, int M,
                               int max_count, int C, int R, void *stream);

/* ------------------------------------------------------------------------
 * Streaming log-mel front end: cer_logmel_fwd and cer_frame_examples run on PCM chunks of S independent streams.
 *
 * State: a sample ring [S][Rs] int16 and a log-mel ring [S][Rm][64] fp32; Rs and Rm are powers of two up to 2^30.  The
 * device keeps no counters.  The host says what a launch does in int32 tables in device memory; sample positions and row
 * numbers in them are unwrapped, modulo 2^30 (every ring length divides 2^30, so the mask R - 1 finds the slot).  One push
 * is the three launches below on one HIP stream, in this order.
 *
 * cer_logmel_stream_append: segments [4][num_segments] = stream, position of the segment's first sample, count, offset.
 *     offset >= 0:  ring[stream][(pos + i) & (Rs - 1)] = packed[offset + i]                          for i < count
 *     offset <  0:  ring[stream][(pos + i) & (Rs - 1)] = ring[stream][(pos - 1) & (Rs - 1)]          (repeat the sample before)
 *   packed holds packed_len samples; an index past it reads as 0.  max_count is the largest count in the table (the entry
 *   cannot read it); a larger count is cut to it.  A stream has at most one segment in a launch.
 * cer_logmel_stream_rows: rows [3][num_rows] = stream, position of the row's first sample, row number.  Row m is the
 *   log-mel of the 400 samples ring[stream][(pos + n) & (Rs - 1)], n < 400, computed by the one device function that
 *   cer_logmel_fwd runs (csrc/logmel_row.h): the same bits as that entry gives the same samples.  It is written to
 *   logmel_ring[stream][row & (Rm - 1)][0 .. 63].
 * cer_logmel_stream_examples: examples [2][num_examples] = stream, start row.
 *     out[e][f][:] = logmel_ring[stream][(start + f) & (Rm - 1)][:]   for f < win;   out [num_examples][win][64].
 *
 * The tables are never trusted with an address: a stream index is clamped into [0, S), every position is masked with its
 * ring length and every read of `packed` is bounded by packed_len.  A wrong table gives wrong numbers, never an access
 * outside a ring or outside the packed input.
 * Refused with CER_ERR_INVALID_ARG before any launch, with a cer_last_error() text that begins with the entry's name: a null
 * pointer; a count (packed_len, num_segments, max_count, num_rows, num_examples, win, S) below 1; Rs or Rm not a power of
 * two up to 2^30; Rs < 400; max_count >= Rs; Rm < win; more than 65535 segments; a log-mel ring or an output of
 * cer_logmel_stream_examples that is not 16-byte aligned.
 * ---------------------------------------------------------------------- */
int cer_logmel_stream_append(const int16_t *packed, int packed_len, const int32_t *segments, int num_segments, int max_count,
                             int16_t *ring, int S, int Rs, void *stream);
int cer_logmel_stream_rows(const int16_t *ring, int S, int Rs, const int32_t *rows, int num_rows, const double *mel_matrix,
                           float log_offset, float *logmel_ring, int Rm, void *stream);
int cer_logmel_stream_examples(const float *logmel_ring, int S, int Rm, const int32_t *examples, int num_examples, int win,
                               float *out, void *stream);

/* ------------------------------------------------------------------------
 * Streaming resampler: cer_resample_pcm run on PCM chunks, in front of the streaming log-mel.  Any input rate, any number of
 * interleaved channels.
 *
 * State: a mixed-input ring [S][Rin] float64 (the channel mean of pcm / 32768 at the input rate) and a 16 kHz sample ring
 * [S][Rs] float64 (the resampler's output, in [-1, 1)), then the log-mel ring above; Rin and Rs are powers of two up to 2^30.
 * The device keeps no counters; tables and positions as above (int32, unwrapped modulo 2^30).  One push is four launches on
 * one HIP stream: cer_resample_stream_append, cer_resample_stream_outputs, cer_logmel_stream_rows_f64,
 * cer_logmel_stream_examples.
 *
 * cer_resample_stream_append: segments [4][num_segments] = stream, position of the segment's first input sample, count,
 *   offset in frames.  packed holds packed_frames frames of `channels` interleaved int16 samples.
 *     offset >= 0:  in_ring[stream][(pos + i) & (Rin - 1)] = (sum_ch packed[offset + i][ch] / 32768.0) / channels   for i < count
 *     offset <  0:  in_ring[stream][(pos + i) & (Rin - 1)] = in_ring[stream][(pos - 1) & (Rin - 1)]   (repeat the sample before)
 *   A frame past packed_frames reads as 0; a count above max_count is cut to it.  history: how many inputs before the new
 *   ones the caller still needs (T - 1 for a table of T taps per phase); only checked against Rin.
 * cer_resample_stream_outputs: segments [7][num_segments] = stream, position n0 of the first output, count, r0, position of
 *   input q0, lo, hi, where q0 = (n0 M) div L and r0 = (n0 M) mod L in the caller's unbounded integers.  For i < count, with
 *   q = (r0 + i M) div L, r = (r0 + i M) mod L (64-bit) and J = (T - 2) / 2:
 *     out_ring[stream][(n0 + i) & (Rs - 1)] = sum_{j < T} taps[r][j] * x[q - J + j]
 *     x[k] = in_ring[stream][(pos_q0 + k) & (Rin - 1)]  for lo <= k < hi,  0 otherwise
 *   [lo, hi) is the stream's valid input range relative to q0 (before its first sample and at or after its last appended
 *   sample the ring holds old samples, so those inputs are zero by this check, never a ring read); it is cut to the Rin
 *   inputs before hi.  taps is [L][T] float64.  The sum is the device function cer_resample_pcm runs
 *   (csrc/resample_row.h), in the order j = 0 .. T - 1: the same bits as that entry gives the same inputs.
 * cer_logmel_stream_rows_f64: cer_logmel_stream_rows on the float64 16 kHz ring (samples already in [-1, 1)).
 *
 * The tables are never trusted with an address: a stream index is clamped into [0, S), a count is cut to max_count, every
 * position is masked with its ring length, every read of `packed` is bounded by packed_frames and r0 is reduced modulo L.
 * Refused with CER_ERR_INVALID_ARG before any launch, with a cer_last_error() text that begins with the entry's name: a null
 * pointer; a count (packed_frames, channels, num_segments, max_count, num_rows, S) below 1 or history < 0; a ring length
 * that is not a power of two up to 2^30; Rs < 400 for the rows; history + max_count > Rin or max_count >= Rin for the append;
 * Rin < T, max_count > Rs, T odd or < 2, L or M <= 0, or 256 M / L + T > 2^24 (the inputs one block walks through) for the
 * outputs; more than 65535 segments.
 * ---------------------------------------------------------------------- */
int cer_resample_stream_append(const int16_t *packed, int packed_frames, int channels, const int32_t *segments,
                               int num_segments, int max_count, int history, double *in_ring, int S, int Rin, void *stream);
int cer_resample_stream_outputs(const double *in_ring, int S, int Rin, const int32_t *segments, int num_segments,
                                int max_count, const double *taps, int L, int M, int T, double *out_ring, int Rs, void *stream);
int cer_logmel_stream_rows_f64(const double *ring, int S, int Rs, const int32_t *rows, int num_rows, const double *mel_matrix,
                               float log_offset, float *logmel_ring, int Rm, void *stream);

/* ------------------------------------------------------------------------
 * Streaming frame transform: cer_frames_transform on raw camera frames of S independent streams.
 *
 * State: one ring u8ring [S][Rf][crop][crop][3] uint8, the GroupScale -> crop -> flip result of each stream's last Rf
 * frames, channels last; Rf is a power of two up to 2^30.  The ring holds the bytes (return_u8 of cer_frames_transform), not
 * the floats: the float is a pure function of the byte.  The device keeps no counters.  Rows are named as for the streaming
 * TCN: row_stream[m] is the stream of row m, row_pos[m] that frame's number in its stream, unwrapped, modulo 2^30; its
 * slot is row_pos[m] & (Rf - 1).
 *
 * cer_frames_stream_append: frames [n_frames][H][W][3] uint8 packed; row m of the table is packed frame m (frame
 *   n_frames - 1 for m >= n_frames).  The coefficient tables, size, crop and max_band_rows are those of
 *   cer_frames_transform; crop_xyf is [S][3] = (x1, y1, flip), one entry per STREAM.  The kernel is the one
 *   cer_frames_transform launches (csrc/frames_kernel.h), so
 *     u8ring[row_stream[m]][row_pos[m] & (Rf - 1)] = out_u8 of cer_frames_transform for that frame and that crop entry.
 *   max_count is the largest number of rows any one stream has in the table (the entry cannot read it).
 * cer_frames_stream_gather: out[m][c][y][x] = ((float)v / 255.0f - mean) / stdv for the byte
 *   v = u8ring[row_stream[m]][row_pos[m] & (Rf - 1)][y][x][c]; out is [num_rows][3][crop][crop] fp32, the expression
 *   cer_frames_transform applies to the same byte.
 *
 * The tables are never trusted with an address: a stream index is clamped into [0, S), a position is masked with Rf - 1,
 * the packed frame index is bounded by n_frames, and x1, y1 are clamped into [0, size - crop].  A wrong table gives wrong
 * numbers, never an access outside the ring or the packed input.
 * Refused before any launch, with a cer_last_error() text that begins with the entry's name: a null pointer; a count or a
 * dimension below 1; Rf not a power of two up to 2^30; crop > size; max_count > Rf; more than 65535 rows or frames per call
 * (CER_ERR_INVALID_ARG); a band of input rows that needs more than the 160 KiB LDS (CER_ERR_UNSUPPORTED).
 * ---------------------------------------------------------------------- */
int cer_frames_stream_append(const uint8_t *frames, int n_frames, int H, int W, const int32_t *hbounds, const int32_t *hcoef,
                             int hksize, const int32_t *vbounds, const int32_t *vcoef, int vksize, int size, int crop,
                             const int32_t *crop_xyf, int max_band_rows, const int32_t *row_stream, const int32_t *row_pos,
                             int num_rows, int max_count, uint8_t *u8ring, int S, int Rf, void *stream);
int cer_frames_stream_gather(const uint8_t *u8ring, int S, int Rf, int crop, const int32_t *row_stream, const int32_t *row_pos,
                             int num_rows, float mean, float stdv, float *out, void *stream);

/* ------------------------------------------------------------------------
 * Per-frame face boxes on full camera frames (csrc/frames_box.hip): PIL's Image.crop(box) -> cer_frames_transform, per frame.
 *
 * boxes [rows][4] int32 = (x0, y0, x1, y1) per launch row, PIL's (left, upper, right, lower), right and lower exclusive; the
 * part of a box outside the H x W frame reads as 0.  Row f gives the bytes (and floats) cer_frames_transform gives the
 * contiguous zero-padded slice of its frame; a box equal to the whole frame gives the bits of the unboxed entries.
 *
 * The coefficients of every side n = 1 .. max_side come from one table store, built once per (size, max_side):
 *   box_meta [max_side + 1][4] int32 = (offset of the bounds, offset of the coefficients, ksize, band span) of side n, the
 *     offsets counted in int32 from box_data (row 0 repeats row 1);
 *   box_data: for each n the bounds [size][2] and coefficients [size][ksize] of cer_frames_transform for n -> size.
 * max_band_rows = the largest band span and max_ksize = the largest ksize of any n <= max_side: they size the LDS, which is
 * bounded by (size, crop, max_side) and does not depend on H x W.
 *
 * cer_frames_transform_boxes: the clip form; rows = n_frames, the other arguments as in cer_frames_transform.
 * cer_frames_stream_append_boxes: the ring form; row m reads packed frame m (clamped below n_frames) and box m, the other
 *   arguments as in cer_frames_stream_append.
 *
 * The box table is never trusted with an address: a coordinate is clamped into +-2^20, width and height into
 * [1, max_side], every input pixel is fetched through a range check against the frame, and the streamed tables are treated
 * as in cer_frames_stream_append.  A wrong table gives wrong numbers, never an access outside the packed frames or the ring.
 * Refused before any launch, with a cer_last_error() text that begins with the entry's name: a null pointer; a count or a
 * dimension below 1; crop > size; max_side outside 1 .. 2^20; max_band_rows > max_side; Rf not a power of two up to 2^30;
 * max_count > Rf; more than 65535 rows or frames per call (CER_ERR_INVALID_ARG); an LDS need above 160 KiB
 * (CER_ERR_UNSUPPORTED).
 * ---------------------------------------------------------------------- */
int cer_frames_transform_boxes(const uint8_t *frames, int n_frames, int H, int W, const int32_t *boxes, const int32_t *box_meta,
                               const int32_t *box_data, int max_side, int max_band_rows, int max_ksize, int size, int crop,
                               const int32_t *crop_xyf, int frames_per_group, float mean, float stdv, float *out,
                               uint8_t *out_u8, void *stream);
int cer_frames_stream_append_boxes(const uint8_t *frames, int n_frames, int H, int W, const int32_t *boxes,
                                   const int32_t *box_meta, const int32_t *box_data, int max_side, int max_band_rows,
                                   int max_ksize, int size, int crop, const int32_t *crop_xyf, const int32_t *row_stream,
                                   const int32_t *row_pos, int num_rows, int max_count, uint8_t *u8ring, int S, int Rf,
                                   void *stream);

/* ------------------------------------------------------------------------
 * 8-bit 4:2:0 frames (NV12 from hardware decoders, I420 from software ones), converted to RGB where the kernel reads a pixel.
 *
 * A frame of an H x W picture, H and W even, is H * 3 / 2 rows of W bytes: the Y plane [H][W], then
 *   CER_YUV_NV12: the interleaved chroma [H / 2][W / 2][2], U first;
 *   CER_YUV_I420: the U plane [H / 2][W / 2], then the V plane [H / 2][W / 2].
 * Pixel (x, y) takes the chroma sample (x >> 1, y >> 1): nearest siting, no interpolation.  With c = Y - yoff, u = U - 128,
 * v = V - 128, h = 1 << (CER_YUV_PREC - 1), in int32 with an arithmetic (flooring) shift,
 *   R = clip8((cy c + crv v + h) >> CER_YUV_PREC)
 *   G = clip8((cy c + cgu u + cgv v + h) >> CER_YUV_PREC)
 *   B = clip8((cy c + cbu u + h) >> CER_YUV_PREC)
 * The five coefficients are the matrix (BT.601, BT.709, limited or full range) times 2^CER_YUV_PREC, rounded by the host.
 *
 * The four _yuv entries are their RGB siblings with `frames` [n_frames][H * 3 / 2][W] and a cer_yuv420; H and W stay the
 * picture's, boxes stay in luma pixels.  Only the pixel fetch differs, so each gives the bits its sibling gives the
 * converted RGB frames; a box tap outside the picture still contributes RGB 0 (not YUV 0 converted).  The chroma address is
 * derived from the clamped luma index, so the tables are trusted exactly as little as by the siblings.
 * Refused before any launch: what the sibling refuses (the unboxed pair in the sibling's words), a null descriptor, odd H or W, a picture above 2^29 pixels, an
 * unknown layout, a coefficient beyond +-2^20 (the sums must stay in int32) and yoff outside 0 .. 255 (CER_ERR_INVALID_ARG).
 * ---------------------------------------------------------------------- */
#define CER_YUV_PREC 14
#define CER_YUV_NV12 0
#define CER_YUV_I420 1

typedef struct cer_yuv420 {
    int32_t layout;                  /* CER_YUV_NV12 or CER_YUV_I420 */
    int32_t cy, crv, cgu, cgv, cbu;  /* times 2^CER_YUV_PREC */
    int32_t yoff;                    /* 16 for limited range, 0 for full */
} cer_yuv420;

int cer_frames_transform_yuv(const uint8_t *frames, const cer_yuv420 *yuv, int n_frames, int H, int W, const int32_t *hbounds,
                             const int32_t *hcoef, int hksize, const int32_t *vbounds, const int32_t *vcoef, int vksize,
                             int size, int crop, const int32_t *crop_xyf, int frames_per_group, int max_band_rows, float mean,
                             float stdv, float *out, uint8_t *out_u8, void *stream);
int cer_frames_stream_append_yuv(const uint8_t *frames, const cer_yuv420 *yuv, int n_frames, int H, int W,
                                 const int32_t *hbounds, const int32_t *hcoef, int hksize, const int32_t *vbounds,
                                 const int32_t *vcoef, int vksize, int size, int crop, const int32_t *crop_xyf,
                                 int max_band_rows, const int32_t *row_stream, const int32_t *row_pos, int num_rows,
                                 int max_count, uint8_t *u8ring, int S, int Rf, void *stream);
int cer_frames_transform_boxes_yuv(const uint8_t *frames, const cer_yuv420 *yuv, int n_frames, int H, int W,
                                   const int32_t *boxes, const int32_t *box_meta, const int32_t *box_data, int max_side,
                                   int max_band_rows, int max_ksize, int size, int crop, const int32_t *crop_xyf,
                                   int frames_per_group, float mean, float stdv, float *out, uint8_t *out_u8, void *stream);
int cer_frames_stream_append_boxes_yuv(const uint8_t *frames, const cer_yuv420 *yuv, int n_frames, int H, int W,
                                       const int32_t *boxes, const int32_t *box_meta, const int32_t *box_data, int max_side,
                                       int max_band_rows, int max_ksize, int size, int crop, const int32_t *crop_xyf,
                                       const int32_t *row_stream, const int32_t *row_pos, int num_rows, int max_count,
                                       uint8_t *u8ring, int S, int Rf, void *stream);

/* ------------------------------------------------------------------------
 * Per-frame affine maps on full camera frames (csrc/frames_affine.hip): PIL's Image.transform((A, A), AFFINE, a, BILINEAR)
 * -> cer_frames_transform, per frame; A = align_size.  This is how a face is aligned from five landmarks: the similarity
 * that puts them on a template, inverted, is the affine of its frame.
 *
 * affines [rows][6] float64, 8-byte aligned = (a0 .. a5) per launch row, Pillow's coefficients: with xin = x + 0.5 and
 * yin = y + 0.5, pixel (x, y) of the A x A face is sampled at X = (a0 xin + a1 yin) + a2, Y = (a3 xin + a4 yin) + a5 of the
 * H x W frame.  Every step below is float64 and none is fused:
 *   the pixel is (0, 0, 0) unless X >= 0 && X < W && Y >= 0 && Y < H (so a NaN is outside);
 *   X -= 0.5, Y -= 0.5; ix = floor(X), iy = floor(Y); dx = X - ix, dy = Y - iy;
 *   x0 = clamp(ix, 0, W - 1), x1 = clamp(ix + 1, 0, W - 1), row0 = clamp(iy, 0, H - 1);
 *   v1 = p[row0][x0] + (p[row0][x1] - p[row0][x0]) dx;
 *   v2 = 0 <= iy + 1 < H ? p[iy + 1][x0] + (p[iy + 1][x1] - p[iy + 1][x0]) dx : v1;
 *   byte = (uint8) trunc(v1 + (v2 - v1) dy).
 * Row f gives the bytes (and floats) cer_frames_transform gives that A x A picture.  Under the _yuv entries the four
 * pixels are converted (cer_yuv420) and then interpolated: the bits of the RGB entries on the converted frames.
 *
 * bounds [size][2] and coef [size][ksize] are the rows of cer_frames_transform for A -> size and serve both passes (the
 * face is square); max_band_rows = the most rows of the face one band of cer_frames_band_rows() output rows needs, over
 * every crop offset.  A block keeps the warped rows of its band in LDS: cer_frames_affine_lds_bytes() bytes, bounded by
 * (size, crop, align_size) whatever H x W.
 *
 * cer_frames_transform_affine: the clip form; rows = n_frames, the other arguments as in cer_frames_transform.
 * cer_frames_stream_append_affine: the ring form; row m reads packed frame m (clamped below n_frames) and affine m, the
 *   other arguments as in cer_frames_stream_append.
 *
 * The affine table is never trusted with an address: its values are only compared and multiplied, a coordinate becomes an
 * integer after the range test above has passed, and every pixel is fetched at an index clamped into the frame; the streamed
 * tables are treated as in cer_frames_stream_append.  NaN, infinities and huge values give the all-zero picture.
 * Refused before any launch, with a cer_last_error() text that begins with the entry's name: a null pointer; a count or a
 * dimension below 1; crop > size; align_size outside 1 .. 2^14; max_band_rows > align_size; ksize > 2 align_size + 3; a
 * frame above 2^29 pixels; a misaligned affine table; Rf not a power of two up to 2^30; max_count > Rf; more than 65535 rows
 * or frames per call; what the _yuv descriptor check refuses (CER_ERR_INVALID_ARG); an align_size whose LDS need exceeds
 * 160 KiB (CER_ERR_UNSUPPORTED).
 * ---------------------------------------------------------------------- */
size_t cer_frames_affine_lds_bytes(int align_size, int max_band_rows, int ksize, int crop);
int cer_frames_transform_affine(const uint8_t *frames, int n_frames, int H, int W, const double *affines, const int32_t *bounds,
                                const int32_t *coef, int ksize, int align_size, int max_band_rows, int size, int crop,
                                const int32_t *crop_xyf, int frames_per_group, float mean, float stdv, float *out,
                                uint8_t *out_u8, void *stream);
int cer_frames_stream_append_affine(const uint8_t *frames, int n_frames, int H, int W, const double *affines,
                                    const int32_t *bounds, const int32_t *coef, int ksize, int align_size, int max_band_rows,
                                    int size, int crop, const int32_t *crop_xyf, const int32_t *row_stream,
                                    const int32_t *row_pos, int num_rows, int max_count, uint8_t *u8ring, int S, int Rf,
                                    void *stream);
int cer_frames_transform_affine_yuv(const uint8_t *frames, const cer_yuv420 *yuv, int n_frames, int H, int W,
                                    const double *affines, const int32_t *bounds, const int32_t *coef, int ksize, int align_size,
                                    int max_band_rows, int size, int crop, const int32_t *crop_xyf, int frames_per_group,
                                    float mean, float stdv, float *out, uint8_t *out_u8, void *stream);
int cer_frames_stream_append_affine_yuv(const uint8_t *frames, const cer_yuv420 *yuv, int n_frames, int H, int W,
                                        const double *affines, const int32_t *bounds, const int32_t *coef, int ksize,
                                        int align_size, int max_band_rows, int size, int crop, const int32_t *crop_xyf,
                                        const int32_t *row_stream, const int32_t *row_pos, int num_rows, int max_count,
                                        uint8_t *u8ring, int S, int Rf, void *stream);

/* ------------------------------------------------------------------------
 * Surfaces: frames read in place, in the byte order and with the row pitch a capture API or a decoder hands them out.
 *
 * A cer_surface says where the three bytes of pixel (x, y) of an H x W picture lie in frame m of `frames`.  With
 * base = frames + m * frame_stride, xs = x >> xshift, ys = y >> yshift:
 *   a = base[offset[0] + y  * pitch[0] + x  * step[0] + pos[0]]
 *   b = base[offset[1] + ys * pitch[1] + xs * step[1] + pos[1]]
 *   c = base[offset[2] + ys * pitch[1] + xs * step[1] + pos[2]]
 * and the format fixes the shifts and says what (a, b, c) are:
 *   CER_SURFACE_PACKED   (R, G, B) themselves; no shifts.  step[0] == step[1] = 3 or 4 bytes per pixel, pos[] = the byte of
 *                        R, G, B inside a pixel (BGR: 2 1 0; RGBA: 0 1 2; BGRA: 2 1 0), the three offsets and the two pitches
 *                        equal.  A fourth byte is never loaded.
 *   CER_SURFACE_YUV420   (Y, U, V), xshift = yshift = 1: a luma plane and chroma at half resolution.  step[0] = 1, pos[] = 0;
 *                        step[1] = 2 for interleaved chroma (NV12: offset[2] = offset[1] + 1; NV21: offset[1] = offset[2] + 1),
 *                        1 for planes (I420: the U plane first; YV12: the V plane first).  No layout needs a format of its own.
 *   CER_SURFACE_YUV422   (Y, U, V), xshift = 1, yshift = 0: one plane of 4-byte pairs.  step[0] = 2, step[1] = 4;
 *                        YUYV: pos = 0 1 3; UYVY: pos = 1 0 2; the three offsets and the two pitches equal.
 * (Y, U, V) become RGB through the expression of cer_yuv420 above, with this descriptor's cy .. yoff; PACKED ignores them
 * but they are checked all the same.  Nothing has to be aligned and planes may overlap: they are only read.
 *
 * The six _surface entries are their RGB siblings with `frames_bytes`, the extent of `frames` the caller vouches for, and a
 * cer_surface after `frames`; H and W stay the picture's, boxes stay in picture pixels.  Only the pixel fetch differs, so
 * each gives the bits its sibling gives the converted, tightly packed RGB frames; what lies outside the picture is RGB 0.
 *
 * The descriptor is checked, not trusted.  Refused before any launch, with the entry's name at the head of cer_last_error()
 * (CER_ERR_INVALID_ARG): a null descriptor; an unknown format; a coefficient beyond +-2^20 or yoff outside 0 .. 255; steps,
 * positions, offsets or pitches that are not one of the patterns above; odd W (YUV422), odd H or W (YUV420); a picture
 * above 2^29 pixels; a negative offset, pitch or stride, or one of 2^40 or more; a pitch below the bytes of a row (W * step[0]
 * for plane 0, W / 2 * step[1] for 4:2:0 chroma); a plane whose last row ends past frame_stride; and
 * (n_frames - 1) * frame_stride plus the used extent of a frame -- the largest end of a plane -- above frames_bytes, in
 * arithmetic that cannot wrap (comparisons and one division of non-negative 64-bit values).  Then what the sibling refuses.
 * After that check the kernels form a pixel address from a frame index below n_frames, 0 <= y < H and 0 <= x < W only (the
 * clamped indices the siblings use): it is at least frames, and at most frames + (n_frames - 1) * frame_stride + the end of
 * its plane - 1 < frames + frames_bytes.  So every load lies in [frames, frames + frames_bytes), and the box, affine and row
 * tables are trusted exactly as little as by the siblings.
 * ---------------------------------------------------------------------- */
#define CER_SURFACE_PACKED 0
#define CER_SURFACE_YUV420 1
#define CER_SURFACE_YUV422 2

typedef struct cer_surface {
    int32_t format;                  /* CER_SURFACE_PACKED, CER_SURFACE_YUV420 or CER_SURFACE_YUV422 */
    int32_t cy, crv, cgu, cgv, cbu;  /* as in cer_yuv420 */
    int32_t yoff;
    int32_t step[2];                 /* bytes from one sample to the next in a row: of a, and of b and c */
    int32_t pos[3];                  /* byte of a, b, c inside its sample */
    int64_t frame_stride;            /* bytes from frame m to frame m + 1 */
    int64_t pitch[2];                /* bytes from one row to the next: of a, and of b and c */
    int64_t offset[3];               /* byte offset of the planes of a, b, c inside a frame */
} cer_surface;

int cer_frames_transform_surface(const uint8_t *frames, size_t frames_bytes, const cer_surface *surface, int n_frames, int H,
                                 int W, const int32_t *hbounds, const int32_t *hcoef, int hksize, const int32_t *vbounds,
                                 const int32_t *vcoef, int vksize, int size, int crop, const int32_t *crop_xyf,
                                 int frames_per_group, int max_band_rows, float mean, float stdv, float *out, uint8_t *out_u8,
                                 void *stream);
int cer_frames_stream_append_surface(const uint8_t *frames, size_t frames_bytes, const cer_surface *surface, int n_frames, int H,
                                     int W, const int32_t *hbounds, const int32_t *hcoef, int hksize, const int32_t *vbounds,
                                     const int32_t *vcoef, int vksize, int size, int crop, const int32_t *crop_xyf,
                                     int max_band_rows, const int32_t *row_stream, const int32_t *row_pos, int num_rows,
                                     int max_count, uint8_t *u8ring, int S, int Rf, void *stream);
int cer_frames_transform_boxes_surface(const uint8_t *frames, size_t frames_bytes, const cer_surface *surface, int n_frames,
                                       int H, int W, const int32_t *boxes, const int32_t *box_meta, const int32_t *box_data,
                                       int max_side, int max_band_rows, int max_ksize, int size, int crop,
                                       const int32_t *crop_xyf, int frames_per_group, float mean, float stdv, float *out,
                                       uint8_t *out_u8, void *stream);
int cer_frames_stream_append_boxes_surface(const uint8_t *frames, size_t frames_bytes, const cer_surface *surface, int n_frames,
                                           int H, int W, const int32_t *boxes, const int32_t *box_meta, const int32_t *box_data,
                                           int max_side, int max_band_rows, int max_ksize, int size, int crop,
                                           const int32_t *crop_xyf, const int32_t *row_stream, const int32_t *row_pos,
                                           int num_rows, int max_count, uint8_t *u8ring, int S, int Rf, void *stream);
int cer_frames_transform_affine_surface(const uint8_t *frames, size_t frames_bytes, const cer_surface *surface, int n_frames,
                                        int H, int W, const double *affines, const int32_t *bounds, const int32_t *coef,
                                        int ksize, int align_size, int max_band_rows, int size, int crop,
                                        const int32_t *crop_xyf, int frames_per_group, float mean, float stdv, float *out,
                                        uint8_t *out_u8, void *stream);
int cer_frames_stream_append_affine_surface(const uint8_t *frames, size_t frames_bytes, const cer_surface *surface, int n_frames,
                                            int H, int W, const double *affines, const int32_t *bounds, const int32_t *coef,
                                            int ksize, int align_size, int max_band_rows, int size, int crop,
                                            const int32_t *crop_xyf, const int32_t *row_stream, const int32_t *row_pos,
                                            int num_rows, int max_count, uint8_t *u8ring, int S, int Rf, void *stream);

/* ------------------------------------------------------------------------
 * Running video-level decisions of S live streams (csrc/decision_stream.hip): logit rows in, the three decisions of
 * metrics.py:118-139 out -- majority vote over the frame predictions, argmax of the mean logits, argmax of the mean softmax
 * probabilities -- over the first nc = C - (drop_last ? 1 : 0) columns.
 *
 * State.  Whole-stream (W = 0: all frames since the stream's reset): votes [S][C] and first [S][C] int64 (frames predicted
 * as class c; index since reset of the first of them, INT64_MAX while there is none), slog [S][C] and sprob [S][C] float64
 * (sums of the logits and of the probabilities).  A reset stream has votes = slog = sprob = 0 and first = INT64_MAX.
 * Window (W >= 1: the last min(n, W) frames): zring [S][R][C] fp32, the logits themselves, R a power of two >= W +
 * max_count; nothing is accumulated across calls, a decision is recomputed from the window's rows.  Without `classify`
 * (regression outputs) only slog / zring exist and only the mean of the rows is defined.
 *
 * Arithmetic, one definition for both modes: prediction = the first NaN, otherwise the first maximum (numpy.argmax);
 * probability = expf(z[c]) / (expf(z[0]) + ... + expf(z[nc - 1])) in fp32 without max subtraction; column sums
 * acc += (double)value, one chain per (stream, class) in time order -- continued from the accumulators whole-stream,
 * started at the window's oldest row otherwise; mean = sum / n in double (the decisions compare the doubles; outputs are
 * rounded once to fp32); vote ties go to the class first seen earliest (inside the window, in window mode).  A result is
 * the same bits however the rows were cut into pushes, whatever max_count, the ring position, S or the other streams.
 *
 * Tables.  The device keeps no counters.  segments [6][num_segments] int32 = stream, count, offset of the stream's first new
 * row in `rows`, ring position of that row (unwrapped, modulo 2^30), and the stream's frames since reset BEFORE the push as a
 * 64-bit value (low word, then high word).  A stream has at most one segment per push.  cer_decision_stream_read takes the
 * same six fields, one column per stream in stream order (the stream field is not read): count = rows in the window
 * (ignored when W = 0), position = where the next row would go, frames = frames since reset.  One block of 64 lanes per
 * segment (per stream for a read); no atomics, no flags, no scratch.
 *
 * cer_decision_stream_push: appends `count` rows per segment.  track [M][3] int32 (may be NULL) receives the three
 * decisions as they stand AFTER each new row, track_means [M][2][C] fp32 (may be NULL) the mean logits and the mean
 * probabilities after it (the dropped column: its mean logit, and 0; without classify the second half is 0).
 * cer_decision_stream_read: decisions [S][3] int32 (-1 for a stream with no frame; NULL without classify) and means
 * [S][2][C] fp32 (NaN for a stream with no frame).  It takes the descriptor of the pushes; M only has to be >= 1.
 *
 * The tables are never trusted with an address: the stream is clamped into [0, S), a count is cut to max_count (to W in a
 * read), positions are masked with R - 1, and every access to `rows`, `track` and `track_means` is bounded by M (a row
 * outside reads as 0).  A wrong table gives wrong numbers, never an access outside the state or the packed rows.
 * Refused with CER_ERR_INVALID_ARG before any launch, with a cer_last_error() text that begins with the entry's name: a null
 * pointer (descriptor, rows, table, a state tensor of the mode, the outputs of a read); C < 2 or C > 16; S, M or max_count
 * < 1; W < 0; for W >= 1, R not a power of two or W + max_count > R; drop_last with C < 3 or without classify; a track
 * without classify; num_segments < 1.
 * ---------------------------------------------------------------------- */
typedef struct cer_decision_stream_desc {
    int32_t S, C;              /* streams, columns of a row */
    int32_t M, max_count;      /* packed rows of the push, the largest count of one stream */
    int32_t W, R;              /* window length (0: whole-stream) and ring length (read when W >= 1) */
    int32_t drop_last;         /* decide over the first C - 1 columns */
    int32_t classify;          /* 0: rows are regression outputs, only their mean is kept */
} cer_decision_stream_desc;

int cer_decision_stream_push(const cer_decision_stream_desc *d, const float *rows, const int32_t *segments, int num_segments,
                             long long *votes, long long *first, double *slog, double *sprob, float *zring, int32_t *track,
                             float *track_means, void *stream);
int cer_decision_stream_read(const cer_decision_stream_desc *d, const int32_t *table, const long long *votes,
                             const long long *first, const double *slog, const double *sprob, const float *zring,
                             int32_t *decisions, float *means, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CER_HIP_H */
