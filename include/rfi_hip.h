/* rfi_hip.h -- C ABI of librfi_hip.so, the MI355X (gfx950) implementation of the
 * rfi_toolbox segmentation hot path.
 *
 * The reference (preshanth/rfi_toolbox v0.2.0) is pure Python and has no FFI
 * layer of its own; its boundary for this path is the torch.nn.Module object
 * protocol plus two plain functions.  Each group below names the reference
 * interface it replaces (paths relative to the reference root).  The Python
 * binding that a maintainer would add is shown in INTEGRATION.md and shipped in
 * rfi_toolbox_amd/_lib.py (ctypes; the header is also cffi-ABI-mode parsable).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; the message of
 *     the last failure on the calling thread is rfi_last_error().
 *   - plain pointers + sizes only.  `mem` arguments say where a buffer lives:
 *     RFI_HOST (pageable/pinned host memory) or RFI_DEVICE (HBM on the ctx's GPU).
 *     Buffers are caller-owned and never retained past the call.
 *   - images are NHWC float32 (what Preprocessor emits, preprocessor.py:380-404);
 *     the NCHW entry points exist because UNet.forward takes NCHW (unet.py:60).
 *   - a handle is bound to one GPU and one HIP stream and is not thread-safe:
 *     one host thread per handle, one process per GPU.
 */
#ifndef RFI_HIP_H
#define RFI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RFI_HIP_ABI_VERSION 1

enum { RFI_HOST = 0, RFI_DEVICE = 1 };

typedef struct rfi_ctx rfi_ctx;
typedef struct rfi_model rfi_model;

/* ---- library / context ------------------------------------------------------------ */
int         rfi_abi_version(void);
const char* rfi_last_error(void);
int rfi_device_count(int* count);
int rfi_ctx_create(int device_id, rfi_ctx** out);
int rfi_ctx_destroy(rfi_ctx* ctx);
/* backward-pass overlap (weight-gradient kernels on a side stream next to the dgrad / batch-norm
 * chain; results are bit-identical either way).  On by default; off = every kernel alone on the
 * main stream, which is what per-kernel timings and rocprofv3 comparisons want. */
int rfi_ctx_set_overlap(rfi_ctx* ctx, int enabled);
int rfi_ctx_synchronize(rfi_ctx* ctx);
/* the hipStream_t every kernel of this ctx is launched on (for event timing / interop) */
int rfi_ctx_stream(rfi_ctx* ctx, void** hip_stream);
int rfi_ctx_device_name(rfi_ctx* ctx, char* buf, size_t buflen);
/* the device allocations the ctx holds now (rfi_malloc, models, scratch): their number and bytes (host only) */
int rfi_ctx_allocations(rfi_ctx* ctx, int64_t* count, uint64_t* bytes);

/* device memory owned by the ctx (freed at rfi_ctx_destroy if still live) */
int rfi_malloc(rfi_ctx* ctx, size_t bytes, void** dptr);
int rfi_free(rfi_ctx* ctx, void* dptr);
int rfi_memcpy(rfi_ctx* ctx, void* dst, int dst_mem, const void* src, int src_mem, size_t bytes);
int rfi_memset(rfi_ctx* ctx, void* dptr, int value, size_t bytes);

/* HIP-event stopwatch on the ctx stream: start; ...launches...; stop -> elapsed ms (syncs) */
int rfi_timer_start(rfi_ctx* ctx);
int rfi_timer_stop(rfi_ctx* ctx, float* elapsed_ms);

/* per-kernel-family HIP-event profile of everything launched while enabled.
 * families: see rfi_profile_family_name(); flops/bytes are ALGORITHMIC counts. */
int rfi_profile_enable(rfi_ctx* ctx, int on);
int rfi_profile_reset(rfi_ctx* ctx);
int rfi_profile_family_count(void);
const char* rfi_profile_family_name(int family);
int rfi_profile_get(rfi_ctx* ctx, int family, int64_t* launches, double* total_ms,
                    double* flops, double* bytes);
/* every profiled launch in stream order as CSV (family, shape label, ms, GFLOP, TFLOP/s, MB, GB/s) */
int rfi_profile_dump(rfi_ctx* ctx, const char* csv_path);

/* ---- model: replaces rfi_toolbox.models.UNet (models/unet.py:41-77; UNetBigger :79-118
 *      is depth=5) as constructed by scripts/train_model.py:111, evaluate_model.py:34 ---- */
int rfi_unet_create(rfi_ctx* ctx, int in_channels, int out_channels, int init_features,
                    int depth, rfi_model** out);
/* the "3-layer CNN segmenter" of BASELINE.json configs[0]/[1] (not a reference
 * class -- nearest text is the elided example README.md:379-398): Conv3x3(in->width,p1)+ReLU ->
 * Conv3x3(width->width,p1)+ReLU -> Conv1x1(width->out) logits.  Entries: encoder.0.weight/bias,
 * encoder.2.weight/bias, decoder.0.weight/bias.  Every rfi_model_* / rfi_train_* call below applies. */
int rfi_cnn3_create(rfi_ctx* ctx, int in_channels, int out_channels, int width, rfi_model** out);
/* "U-Net with a ResNet-18 encoder" of BASELINE.json configs[2] (not a reference class and
 * no torchvision / segmentation_models_pytorch here: builder-defined, oracle/resnet_unet_ref.py).  stem Conv3x3(bias
 * =False)+BN+ReLU at full resolution; layer1..4 of two BasicBlocks each (widths f, 2f, 4f, 8f; stride 2 + 1x1
 * projection entering layers 2-4); then the reference's bottleneck / DecoderBlocks / final_conv (models/unet.py:30-77)
 * with the four stage outputs as skips.  H and W must be multiples of 16; init_features a multiple of 4.
 * Entries: stem.0.weight, stem.1.*, layer{l}.{b}.conv1.weight, .bn1.*, .conv2.weight, .bn2.*, .downsample.0.weight,
 * .downsample.1.*, bottleneck.conv.*, decoder{l}.up.*, decoder{l}.conv.conv.*, final_conv.*.  Compute modes:
 * 2 (float32 by 3 x bf16, default), 0 (native float32 MFMA), 4 (bf16 operands); 1 / 3 run as 4 / 2 (the plane
 * data flow exists for the plain U-Net only). */
int rfi_unet_resnet_create(rfi_ctx* ctx, int in_channels, int out_channels, int init_features, rfi_model** out);
/* The per-RoI mask branch of Mask R-CNN (BASELINE.json configs[3], north_star "per-pixel mask head"; SURVEY.md 8a row A11;
 * not in the reference and no torchvision here: builder-defined as the published head, oracle/mask_head_ref.py):
 * conv_layers x [Conv3x3(C->C, p1)+bias -> ReLU] -> ConvTranspose2d(C->C, k2, s2)+bias -> ReLU -> Conv1x1(C->K).  Input:
 * RoIAlign-ed features [R, h, w, C] (rfi_op_roi_align), output logits [R, 2h, 2w, K]; labels of the training calls are
 * [R, 2h, 2w] uint8 and the loss is the mean BCE-with-logits over them (K = 1; rfi_model_set_loss(m, 1, alpha, gamma)
 * switches to a focal loss).  Entries: mask_fcn{1..L}.weight/bias, conv5_mask.weight/bias, mask_fcn_logits.weight/bias.
 * Every rfi_model_* / rfi_train_* call applies with n = R; rfi_model_input_grad returns the gradient w.r.t. the input
 * features of the last backward pass ([R, h, w, C]) for rfi_op_roi_align_backward / rfi_op_roi_align_ml_backward. */
int rfi_mask_head_create(rfi_ctx* ctx, int in_channels, int conv_layers, int out_channels, rfi_model** out);
int rfi_model_input_grad(rfi_model* m, float* dx, int dx_mem);
/* The RPN head (Faster R-CNN; SURVEY 8a A11, not in the reference): conv_layers x [Conv3x3(C->C, p1)+bias -> ReLU] -> ONE
 * Conv1x1(C -> 5 A): per pixel A objectness logits followed by A x 4 box deltas (anchor-major), i.e. cls_logits and
 * bbox_pred of the usual implementation stacked.  Entries: conv.{i}.0.weight/bias, head.weight/bias.  forward gives
 * [N, H, W, 5 A]; its loss needs per-anchor targets and lives outside the model: rfi_op_rpn_loss produces
 * d(loss)/d(head output), rfi_model_backward_dlogits (after a forward pass on the same input) turns it into parameter
 * gradients and the input gradient (rfi_model_input_grad), rfi_train_apply steps the optimiser.  Also valid for the
 * mask head. */
int rfi_rpn_head_create(rfi_ctx* ctx, int in_channels, int conv_layers, int anchors_per_pixel, rfi_model** out);
/* The ResNet-50-FPN backbone of the Mask R-CNN path (not in the reference: the published networks with the
 * layer names and the FROZEN BatchNorm of the usual detection backbone, oracle/backbone_ref.py).  base_width 64 and
 * fpn_channels 256 give ResNet-50; both must be multiples of 4, H and W multiples of 64.  Entries: body.conv1.weight,
 * body.bn1.{weight,bias,running_mean,running_var}, body.layer{1..4}.{b}.conv{1,2,3}.weight / .bn{1,2,3}.* /
 * .downsample.{0.weight,1.*}, fpn.inner_blocks.{i}.0.{weight,bias}, fpn.layer_blocks.{i}.0.{weight,bias}; BatchNorm entries
 * are buffers (never updated), every conv weight and FPN bias is a parameter of rfi_train_apply.
 * backbone_forward: feats[0..4] = P2..P6, [n, h >> (2 + i), w >> (2 + i), fpn_channels] each (null entries are skipped);
 * backbone_backward (after a forward pass on the same input): dfeats[i] = d(loss)/d(P_{2+i}) (null = zero) -> parameter
 * gradients. */
/* The box head (not in the reference: two FC layers + ReLU on the flattened RoI features, then class scores and
 * per-class box deltas -- TwoMLPHead + FastRCNNPredictor of the usual implementation, oracle/mask_head_ref.py): input
 * [R, in_features] (n = R, h = w = 1), output [R, num_outputs] with num_outputs = 5 K1 = K1 class logits followed by K1 x 4
 * deltas (cls_score and bbox_pred stacked).  Entries: fc6.weight [hidden, in_features, 1, 1] / .bias, fc7..., head.weight /
 * .bias.  Loss outside the model: rfi_op_fastrcnn_loss (labels int32 in [0, K1), 0 = background; targets [R][4]; mean
 * cross-entropy + smooth L1 (beta) of the ground-truth class's deltas over the foreground RoIs, both / R) ->
 * rfi_model_backward_dlogits -> rfi_model_input_grad / rfi_train_apply. */
int rfi_box_head_create(rfi_ctx* ctx, int in_features, int hidden, int fc_layers, int num_outputs, rfi_model** out);
/* x += y on the device (n % 4 == 0): sums the feature-map gradients of several branches */
int rfi_op_add_inplace(rfi_ctx* ctx, float* x, const float* y, int64_t n);
/* fastrcnn_loss: head, labels, targets, dhead (the gradient of classification + box w.r.t. the head output) and
 * loss2_dev[0..1] = (classification, box) all live on the device; workspace: rfi_op_rpn_loss_ws_bytes() bytes of device
 * memory the caller keeps until the stream has passed.  Does not allocate or synchronise. */
int rfi_op_fastrcnn_loss(rfi_ctx* ctx, const float* head, int64_t rois, int num_classes, const int32_t* labels, const float* targets,
                         float beta, float* dhead, void* workspace, float* loss2_dev);
int rfi_resnet50_fpn_create(rfi_ctx* ctx, int in_channels, int base_width, int fpn_channels, rfi_model** out);
int rfi_backbone_forward(rfi_model* m, const float* x, int x_mem, int n, int h, int w, float* const feats[5], int feats_mem);
int rfi_backbone_backward(rfi_model* m, const float* x, int x_mem, int n, int h, int w, const float* const dfeats[5],
                          int dfeats_mem);
int rfi_model_backward_dlogits(rfi_model* m, const float* x, int x_mem, const float* dlogits, int dlogits_mem, int n, int h,
                               int w);
/* A backward pass OVERWRITES the model's gradient buffer.  To sum the gradients of several passes (a head shared by the
 * pyramid levels, several micro-batches): phase 0 zeroes an accumulator, phase 1 adds the current gradients to it (call
 * after each backward pass), phase 2 copies the sum into the gradient buffer, ready for rfi_train_apply. */
int rfi_model_grad_accumulate(rfi_model* m, int phase);
int rfi_model_destroy(rfi_model* m);
/* variants of models/unet.py:120-268 on the same graph: UNetDifferentActivation's activation
 * (0 = ReLU, 0 < s < 1 = LeakyReLU(negative_slope=s), after every BatchNorm) and UNetOverfit's head
 * (forward returns sigmoid(logits), :196; the training step then applies BCE-with-logits + dice to THAT
 * output, as scripts/train_model.py:120,146 does with whatever the model returns). */
int rfi_model_set_activation(rfi_model* m, float negative_slope);
/* arithmetic of the conv / transposed-conv / weight-gradient contractions (tensors in HBM, BatchNorm,
 * loss and the optimiser are float32 in every mode):
 *   2 (default) float32 by splitting: every float32 operand is the exact sum of three bfloat16 pieces and a
 *     product block is six v_mfma_f32_32x32x16_bf16 (float32 accumulate; the three piece products below
 *     2^-24 of the product are dropped).  Error against float64 is that of the native float32 MFMA path
 *     (tests/test_gpu_ops.py runs both against the same tolerances), at 2.7x its matrix-pipe rate.
 *   0 native float32 MFMA (v_mfma_f32_32x32x2_f32, an exact fmaf chain).
 *   1 bfloat16: operands rounded to bfloat16 (RNE), float32 accumulate -- a builder-chosen reduced-precision mode,
 *     NOT the reference's arithmetic (float32 on CPU; float16 autocast + GradScaler on a GPU,
 *     scripts/train_model.py:131,144). */
int rfi_model_set_compute_dtype(rfi_model* m, int dtype);
int rfi_model_set_head_sigmoid(rfi_model* m, int enabled);
/* training loss: 0 = mean BCE-with-logits + dice, the reference's (scripts/train_model.py:120-128,146; default);
 * 1 = sigmoid focal loss, mean over elements (NOT in the reference; builder-defined as
 * Lin et al. 2017 / torchvision.ops.sigmoid_focal_loss: alpha_t (1 - p_t)^gamma BCEwithLogits; alpha < 0
 * disables the alpha weighting);
 * 2 = the same BCE mean + (1/K) sum_k [1 - (2 I_k + 1) / (P_k + T_k + 1)], the dice term of every output channel k on its
 * own (I_k = sum p t, P_k = sum p, T_k = sum t over the batch's pixels of channel k); class-bit labels only.  With one
 * channel it is kind 0.  d/dx_{i,k} = (p - t) / (n h w K) + (1/K) p (1 - p) ((2 I_k + 1) / D_k^2 - 2 t / D_k), D_k = P_k + T_k + 1.
 * With class-bit labels kind 0 is the reference's code on the K-channel tensor (BCE mean over all n h w K elements + ONE
 * dice term over all of them) and kind 1 the focal mean over all of them. */
int rfi_model_set_loss(rfi_model* m, int kind, float alpha, float gamma);
/* An ignore bit in the label byte and per-channel positive weights, two weights on the terms of the sums above.  Both are
 * per-model switches, off by default, for the models class-bit labels support (the plain U-Net without a sigmoid head);
 * the other models refuse them.  While neither is set every path and launch is the one described above.
 *   rfi_model_set_ignore(m, 1): a pixel whose label has bit 7 (RFI_LABEL_IGNORE) set is IGNORED.  Label maps: the target of a
 *     pixel that is not ignored is (label & 0x7F) != 0, so a bool or 0/1 mask means what it meant.  Class-bit labels: the
 *     pixel is ignored for all channels, which needs out_channels <= 7.  With the switch off bit 7 is what it was: RFI in
 *     a map, channel 7's target (or nothing) in class bits.  rfi_model_eval_batch / _eval_batch_classes then count over
 *     the pixels that are not ignored; rfi_model_eval_sweep refuses (its pooled count is the size of the label array).
 *   rfi_model_set_pos_weight(m, w, k): k == out_channels weights, each finite and >= 0, checked before anything is
 *     launched; NULL or k == 0 clears them.  For loss kinds 0 and 2; with focal (which has alpha) either call order fails.
 * With v_i = 1 where pixel i is not ignored (else 0), pi_k the weight of channel k (1 when unset), N_v = K sum_i v_i and
 * p = sigmoid(x):
 *   BCE  = sum v [pi t softplus(-x) + (1 - t) softplus(x)] / N_v  (torch's BCEWithLogitsLoss(pos_weight = pi) over the
 *          valid elements; 0 when N_v = 0);
 *   dice sums I = sum v p t, P = sum v p, T = sum v t, pooled (kind 0) or per channel (kind 2); the dice terms and their
 *          1/K mean are formed from them as above.  The weights do not enter the dice term;
 *   focal = the mean of the focal element over the valid elements, 0 when there are none;
 *   dlogits: at a valid element v (t ? -pi (1 - p) : p) / N_v plus the dice derivative from the masked sums; at an
 *          ignored element every bit is +0.0.  A batch whose pixels are all ignored gives the loss 0.0f and a zero
 *          gradient, nothing non-finite.
 * Reductions: five double sums per class (the four above and the valid count, whole numbers and therefore exact), per
 * block in a fixed order, float32 final combination, bitwise reproducible; with nothing ignored and unit weights the sums
 * are those of the class-bit kernels bit for bit.  N_v stays on the device: rfi_train_step_async reads nothing back. */
#define RFI_LABEL_IGNORE 0x80
int rfi_model_set_ignore(rfi_model* m, int enabled);
int rfi_model_set_pos_weight(rfi_model* m, const float* weights_host, int k);
/* what a label byte means.  RFI_LABELS_MAP (default): non-zero == RFI; the loss and the evaluation need one output channel.
 * RFI_LABELS_CLASS_BITS: the target of output channel k is (label >> k) & 1, 1 <= out_channels <= 8, bits at and above
 * out_channels are ignored; the label tensors keep their shape (n x h x w uint8).  U-Net models without a sigmoid head and
 * without the ResNet encoder only.  The K-channel loss sums are taken in one pass (four double sums per class, per-block
 * partials in a fixed order, float32 final combination): bitwise reproducible. */
enum { RFI_LABELS_MAP = 0, RFI_LABELS_CLASS_BITS = 1 };
int rfi_model_set_label_mode(rfi_model* m, int mode);
/* deterministic init with torch's default distributions (kaiming-uniform(a=sqrt5) conv
 * weights/biases, BN gamma=1 beta=0, running stats 0/1) from a 64-bit seed */
int rfi_model_init(rfi_model* m, uint64_t seed);

/* state_dict surface (train_model.py:179, evaluate_model.py:35): entries are in the
 * reference's state_dict order with the reference's key names and shapes; float32
 * except num_batches_tracked (int64).  Values cross the boundary in the reference's
 * layouts (Conv2d OIHW, ConvTranspose2d IOHW); the library converts. */
int rfi_model_entry_count(rfi_model* m, int* n);
int rfi_model_entry_info(rfi_model* m, int index, const char** name, int* ndim,
                         int64_t dims[4], int* is_int64, int* is_parameter);
int rfi_model_load_entry(rfi_model* m, const char* name, const void* host, size_t bytes);
int rfi_model_store_entry(rfi_model* m, const char* name, void* host, size_t bytes);
int rfi_model_param_count(rfi_model* m, int64_t* n_scalars);   /* == sum(p.numel()) */

/* .train() / .eval()  (train_model.py:136,157) */
int rfi_model_set_training(rfi_model* m, int training);

/* model(x) -> logits (N,out,H,W)  (unet.py:60-77; train_model.py:145).  In training mode
 * BatchNorm uses batch statistics and updates the running buffers exactly as the
 * reference does, including the encoder's double EMA update (unet.py:28). */
/* Synchronisation of the model entry points that take tensors with a memory-space argument (forward_nhwc / forward_nchw,
 * backward_dlogits, input_grad, backbone_forward / backward): with a HOST pointer among the arguments the call returns when the
 * data is in place; when every tensor argument is a DEVICE pointer it returns as soon as the work is enqueued on the
 * context's stream (the next call that hands data to the host -- rfi_memcpy, a loss scalar, rfi_ctx_synchronize --
 * waits).  RFI_SYNC_ALWAYS=1 restores a synchronisation at the end of every call. */
int rfi_model_forward_nhwc(rfi_model* m, const float* x, int x_mem, int n, int h, int w,
                           float* logits, int logits_mem);
int rfi_model_forward_nchw(rfi_model* m, const float* x, int x_mem, int n, int h, int w,
                           float* logits, int logits_mem);

/* ---- optimisation step: replaces the body of the loop in scripts/train_model.py:139-154
 *      zero_grad -> forward -> BCEWithLogits(mean)+dice (:120-128,146) -> backward ->
 *      clip_grad_norm_(max_norm) (:149) -> Adam(lr, betas, eps, coupled L2 weight_decay)
 *      (:130,150).  labels are uint8 (N,H,W), non-zero == RFI.  float32 results throughout (the
 *      reference's CPU path; autocast/GradScaler are off there, :131,144); how the contractions
 *      reach them is rfi_model_set_compute_dtype's business. ---- */
typedef struct rfi_hyper {   /* doubles: the reference's hyper-parameters are python floats */
    double lr, beta1, beta2, eps, weight_decay, max_grad_norm;
} rfi_hyper;

/* Data parallel: when the model's context holds a communicator of more than one rank (rfi_comm_init),
 * rfi_train_step and rfi_train_step_async all-reduce(sum) the flat gradient buffer over the ranks before
 * clipping and apply the MEAN gradient (grad_scale = 1/world), so every rank makes the identical update.
 * BatchNorm batch statistics, running buffers and the dice term stay LOCAL to each rank's batch (torch DDP
 * broadcasts rank 0's buffers every step; here they are only taken from rank 0 at checkpoint time).
 * With the ignore bit on (rfi_model_set_ignore) each rank also divides by its OWN valid count N_v: the ranks' losses are
 * means over their own valid elements, and the update is the mean of those gradients. */
int rfi_train_step(rfi_model* m, const float* x_nhwc, int x_mem, const uint8_t* labels,
                   int labels_mem, int n, int h, int w, const rfi_hyper* hp, float* loss_out);
/* same step split in two so a data-parallel caller can all-reduce the gradients in between */
int rfi_train_forward_backward(rfi_model* m, const float* x_nhwc, int x_mem,
                               const uint8_t* labels, int labels_mem, int n, int h, int w,
                               float* loss_out);
int rfi_train_apply(rfi_model* m, const rfi_hyper* hp, float grad_scale, float* grad_norm_out);
/* loss only, no update (validation loop, train_model.py:157-167) */
int rfi_model_loss(rfi_model* m, const float* x_nhwc, int x_mem, const uint8_t* labels,
                   int labels_mem, int n, int h, int w, float* loss_out);
/* non-blocking variant used by bench loops: enqueue one full step, no host sync */
int rfi_train_step_async(rfi_model* m, const float* x_dev, const uint8_t* labels_dev,
                         int n, int h, int w, const rfi_hyper* hp);
int rfi_model_last_loss(rfi_model* m, float* loss_out, float* grad_norm_out);   /* syncs */

/* flat gradient / parameter buffers (device pointers, library layout) + gradient access
 * by reference name in reference layout (what p.grad would hold after backward) */
int rfi_model_grad_buffer(rfi_model* m, float** dptr, int64_t* n_floats);
int rfi_model_param_buffer(rfi_model* m, float** dptr, int64_t* n_floats);
int rfi_model_store_grad(rfi_model* m, const char* name, void* host, size_t bytes);
int rfi_model_store_adam(rfi_model* m, const char* name, void* host_m, void* host_v, size_t bytes,
                         int64_t* step);
/* resume: load Adam moments of one parameter (reference layout) / set the step counter
 * (the optimizer_state_dict the reference saves, train_model.py:180) */
int rfi_model_load_adam(rfi_model* m, const char* name, const void* host_m, const void* host_v,
                        size_t bytes);
int rfi_model_set_adam_step(rfi_model* m, int64_t step);
int rfi_model_algorithmic_flops(rfi_model* m, int n, int h, int w, double* fwd, double* step);
/* read an internal activation / gradient buffer of the last prepared shape (parity debugging):
 * "encY1.<l>" "encY2.<l>" "decY1.<l>" "decY2.<l>" "concat.<l>" "pool.<l>" "bottY1" "bottY2" "logits"
 * "dlogits" "gA.<l>" "gB.<l>" "dconcat.<l>" "dpool.<l>" "gBottA" "gBottB" (raw NHWC fp32), and
 * "chan.<conv index>" = [running_mean|running_var|mean|invstd|scale|shift|c1|c2] x Cout.
 * Plain U-Net on a plane data flow ("bfloat16", "float32_planes"): a tensor the mode stores as
 * bfloat16 comes back as the exact float32 values of its elements, dense NHWC, under the same name;
 * gA / gB hold the ENCODER's gradients (the decoder phase's are overwritten within the pass).
 * The plane tensors: "xin", "a1e.<l>" "skip.<l>" "pooled.<l>" "up.<l>" "a1d.<l>" "a1b" (activations
 * as the contractions read them), "upin.<l>" (transposed convs on the plane kernels only), "upf.<l>"
 * (the float32 transposed-conv output, where a conversion pass follows it), "dYa.<l>" "dYb.<l>"
 * "dYaE.<l>" "dYbE.<l>" "dYbottA" "dYbottB" (BatchNorm-backward outputs of the decoder's / encoder's /
 * bottleneck's second and first conv).  "<name>:pad" = the padding lanes of a bfloat16 / plane
 * tensor, [pixels][16 * chunks - C] (empty when C % 16 == 0): zeros, if the pass is right.
 * ResNet-encoder U-Net on the bfloat16 data flow (init_features % 16 == 0): its encoder's bfloat16
 * tensors as float32 values, each with the element count of its last writer: "xin" ("xin:pad"),
 * "stemY" "a0" "dY0" (the stem's raw output, activation, BatchNorm-backward output); per block
 * b = 0..7 "rY1.<b>" "rY2.<b>" (raw outputs of conv1 / conv2), "rA1.<b>" (act(BN1(Y1))), "rA.<b>"
 * (the block output; odd b below the last level: the decoder's skip tensor itself), "rdY1.<b>"
 * "rdY2.<b>" (BatchNorm-backward outputs); on the stride-2 blocks 2, 4, 6 also "rYd.<b>" "rdYd.<b>"
 * (the 1x1 projection); "rskip" (the last stage's output as the decoder's skip), "rpool" (its 2x2
 * max), "rdpool" (the gradient w.r.t. rpool); and the scratch every block reuses, which holds its
 * last writer's values, [n h w][init_features]: "rdz.0" (block 0's dz), "rdz.1" (the stem's
 * g = dX + dz of block 0), "rdA1" (block 0's conv2 input gradient), "rdX" (block 0's conv1 input
 * gradient).  A block index out of range, "rYd" / "rdYd" on a stride-1 block and every one of
 * these names on a model that is not on this flow are errors.
 * ResNet-50-FPN backbone (conv indices in state_dict order of the conv weights): "conv.<i>" raw
 * output of conv i before its frozen BatchNorm, on its own output grid (0: the stem at H/2; FPN
 * inner / layer blocks: the lateral / the pyramid level), "pool" the pooled stem, "block.<b>" the
 * output of Bottleneck b (0..15), "merged.<i>" the top-down merged map of FPN level i (0..3),
 * "dmerged.<i>" its gradient (valid after a backward pass); all NHWC fp32.
 * Mask head, RPN head and box head (read-only views of buffers the passes keep anyway, fp32):
 * "y.<i>" the raw output (before ReLU) of 3x3 / FC layer i = 0..layers-1, [n h w][C] or
 * [R][hidden]; "dy.<i>" its gradient dY_i as a backward pass leaves it (after the ReLU mask);
 * "u" / "du" the same two of the transposed conv, [n 2h 2w][C] (the mask head only); "dx" the
 * gradient w.r.t. the input.  A layer index out of range, "u" / "du" on the RPN or box head and
 * every one of these names on another model are errors.
 * host == NULL only reports the element count. */
int rfi_model_debug_tensor(rfi_model* m, const char* name, float* host, size_t host_floats,
                           int64_t* n_floats);

/* one batch of scripts/evaluate_model.py:40-51 entirely on device: forward in the CURRENT mode,
 * sigmoid > threshold, confusion counts against the uint8 labels (non-zero == positive) */
int rfi_model_eval_batch(rfi_model* m, const float* x_nhwc, int x_mem, const uint8_t* labels,
                         int labels_mem, int n, int h, int w, float threshold, int64_t* tp,
                         int64_t* fp, int64_t* fn);
/* the same for a model with class-bit labels: one forward pass, then one kernel that thresholds sigmoid(logit) of every
 * channel and counts against the channel's label bit.  counts: out_channels x 3 on the host, (tp, fp, fn) per channel */
int rfi_model_eval_batch_classes(rfi_model* m, const float* x_nhwc, int x_mem, const uint8_t* labels, int labels_mem, int n,
                                 int h, int w, float threshold, int64_t* counts);
/* rfi_model_eval_batch for n_thresholds cuts from ONE forward pass: forward in the current mode, then
 * rfi_threshold_sweep's kernel with kind LOGITS on what eval_batch thresholds (logits, or the probabilities of a
 * sigmoid-head model: sigmoid of the model's output, as evaluate_model.py:44 does), one group.  counts: K x 3. */
int rfi_model_eval_sweep(rfi_model* m, const float* x_nhwc, int x_mem, const uint8_t* labels, int labels_mem,
                         int n, int h, int w, const float* thresholds_host, int n_thresholds, int64_t* counts_host);

/* ---- data-parallel gradient exchange (new; the reference has no multi-GPU path) -------
 * RCCL over xGMI: ncclAllReduce(sum) of the flat gradient buffer on the ctx stream.
 * librccl.so is dlopen()ed on first use.  id_buf: 128 bytes (ncclUniqueId). */
int rfi_comm_unique_id(void* id_buf128);
int rfi_comm_init(rfi_ctx* ctx, const void* id_buf128, int rank, int world_size);
int rfi_comm_destroy(rfi_ctx* ctx);
int rfi_comm_allreduce_sum_f32(rfi_ctx* ctx, float* dptr, int64_t count);
int rfi_model_allreduce_grads(rfi_model* m);   /* all-reduce(sum) of the grad buffer */
/* Inside rfi_train_step / rfi_train_step_async the exchange is BUCKETED and overlapped with the backward pass:
 * contiguous ranges of the flat gradient buffer (head + decoder1, decoder2, ..., bottleneck, encoderD, ..., encoder1
 * -- the order the backward pass finishes them) are all-reduced on a separate HIP stream as soon as their last
 * producer kernel has been enqueued.  rfi_comm_emulate(ctx, W) (tests on ONE GPU; W >= 2, 0 = off) replaces every
 * bucket's all-reduce by "multiply the range by W" and the step applies grad_scale = 1/W: the step then equals the
 * plain step bit for bit iff every element is exchanged exactly once, after its producers and before clip + Adam. */
int rfi_comm_emulate(rfi_ctx* ctx, int world);

/* ---- preprocessing: replaces the per-patch hot loop of Preprocessor.create_dataset
 *      (preprocessing/preprocessor.py:366-384: _extract_channels_from_complex :562-606 /
 *      _from_real :608-644, then _apply_sam2_normalization :765-783) for a stack of
 *      patches already tiled/rotated by the host.  in: (n,ps_h,ps_w) complex128/complex64
 *      (interleaved re,im) or float64/float32 real; out: NHWC float32 (n,ps_h,ps_w,3). ---- */
enum { RFI_C128 = 0, RFI_C64 = 1, RFI_F64 = 2, RFI_F32 = 3 };
int rfi_preprocess_patches(rfi_ctx* ctx, const void* patches, int patches_mem, int dtype,
                           int n, int ps_h, int ps_w, float* out_nhwc, int out_mem);

/* ---- preprocessing, gather form: the augmentation views (preprocessor.py:413-446), the zero-padded
 *      tiling (:478-560, patchify :22-42) and the blank-patch test (:746-756) resolved ON DEVICE from
 *      the waterfall itself.  `planes`: n_planes x C x T (all baselines x polarisations), complex or
 *      real as above; `flags`: uint8, same shape, non-zero == RFI.  A patch is named by a table entry;
 *      the host only shuffles / truncates the table (the reference's global-RNG permutation, :758-763). */
typedef struct rfi_patch_src {
    int32_t plane;        /* (baseline, polarisation) plane index */
    int32_t view;         /* 0 plane, 1 plane[::-1,:], 2 plane.T, 3 plane.T[::-1,:] */
    int32_t row0, col0;   /* tile origin in view coordinates; pixels past the view's edge are zero padding */
} rfi_patch_src;
/* any_out[i] = 1 when patch i holds a flagged pixel (host array of n bytes) */
int rfi_patch_any_flag(rfi_ctx* ctx, const uint8_t* flags, int flags_mem, int n_planes, int c, int t,
                       const rfi_patch_src* table_host, int n, int ps, uint8_t* any_out_host);
/* images (n,ps,ps,3) float32 NHWC and, when flags != NULL, labels (n,ps,ps) uint8 of the table's patches */
int rfi_preprocess_gather(rfi_ctx* ctx, const void* planes, int planes_mem, int dtype, int n_planes,
                          int c, int t, const uint8_t* flags, int flags_mem,
                          const rfi_patch_src* table_host, int n, int ps, float* out_nhwc, int out_mem,
                          uint8_t* out_labels, int labels_mem);

/* ---- preprocessing, order-statistic branches (preprocessor.py:646-745) on device, for a stack of
 *      patches (n, ps_h, ps_w) already cut by the host:
 *      rfi_preprocess_real: REAL float64 or float32 input (float32: every result rounded to float32, i.e. NumPy's
 *      float32 arithmetic on a float32 array): optional median normalise (:646-670), stretch
 *      (0 none, 1 SQRT, 2 LOG10; infinities <- MAD of the patch's finite values, :672-706), optional second
 *      normalise, then the 3-channel extraction of :608-644 + ImageNet normalisation -> out_nhwc; when
 *      flags_out != NULL also the MAD flags of the PROCESSED patches (:708-745, |x - med| > sigma * MAD).
 *      rfi_mad_flags: the same flags for any input dtype (complex: of |z|), nothing else; complex64 / float32 input in
 *      float32 arithmetic like rfi_preprocess_real, |z| of a complex64 rounded once as the C library's hypotf is.  Any n: stacks of
 *      more than 65,535 patches are walked in chunks (here and in rfi_preprocess_patches / _gather). ---- */
int rfi_preprocess_real(rfi_ctx* ctx, const void* patches, int patches_mem, int dtype, int n, int ps_h,
                        int ps_w, int stretch, int normalize_before, int normalize_after, double flag_sigma,
                        float* out_nhwc, int out_mem, uint8_t* flags_out, int flags_mem);
int rfi_mad_flags(rfi_ctx* ctx, const void* patches, int patches_mem, int dtype, int n, int ps_h, int ps_w,
                  double flag_sigma, uint8_t* flags_out, int flags_mem);

/* ---- synthetic data on device (the step in front of the path): the sample model of
 *      SyntheticDataGenerator._generate_single_sample (data_generation/synthetic_generator.py:520-815)
 *      with a counter-based per-pixel random stream (Philox4x32-10) instead of NumPy's sequential global
 *      one -- distribution-level parity, exact for bandpass / signal / mask given the event table.
 *      Events are drawn by the host (a few dozen per sample); kind 0 fills channels [r0,r1) x times
 *      [c0,c1) with `amp`; kind 1 is a frequency sweep from channel r0 to r1 of width c0 and power-law
 *      order c1 (1 or 2).  Output: planes (n_samples, n_pol, C, T) complex128/complex64 and uint8 flags. */
typedef struct rfi_event {
    int32_t kind, r0, r1, c0, c1;
    int32_t pad_;
    double amp;
} rfi_event;
int rfi_generate_waterfalls(rfi_ctx* ctx, uint64_t seed, int n_samples, int n_pol, int c, int t,
                            double noise_mjy, int bandpass, int bandpass_order, double pol_corr,
                            const rfi_event* events_host, const int32_t* event_offsets_host,
                            int out_dtype, void* planes_out, int planes_mem, uint8_t* flags_out, int flags_mem);

/* ---- metrics: replaces the reductions of evaluation/metrics.py:25-172.  pred/true are
 *      uint8 or float32 arrays of `count` elements, non-zero == positive (:36-37). ---- */
enum { RFI_U8 = 0, RFI_FLOAT32 = 1 };
int rfi_confusion_counts(rfi_ctx* ctx, const void* pred, int pred_dtype, int pred_mem,
                         const void* truth, int truth_dtype, int truth_mem, int64_t count,
                         int64_t* tp, int64_t* fp, int64_t* fn);
/* sigmoid(logit) > threshold on device (evaluate_model.py:44-47), u8 out */
int rfi_threshold_logits(rfi_ctx* ctx, const float* logits_dev, int64_t count, float threshold,
                         uint8_t* mask_dev);
/* counts[g][k] = (tp, fp, fn) of "p > thresholds[k]" against truth over group g, for every k at once.
 * p = scores[i] (RFI_VALUES_PROBS) or 1.0f / (1.0f + expf(-scores[i])) (RFI_VALUES_LOGITS: the expression
 * of rfi_threshold_logits and rfi_stitch_patches).  truth: RFI_U8 or RFI_FLOAT32, non-zero == positive
 * (rfi_confusion_counts' rule).  A NaN score is flagged at no threshold.  thresholds: host, float32, finite,
 * strictly increasing, 1 <= n_thresholds <= 1024.  Groups: count / group_elems contiguous runs of group_elems
 * elements (count % group_elems == 0, at most 65535 groups; group_elems == count: one group).  Device pointers
 * need only their element's alignment (a slice of a larger array is fine).
 * counts_host: n_groups x n_thresholds x 3 int64.  One call, one synchronisation.
 * Arithmetic: an element's bin is b = the number of thresholds strictly below p (binary search; NaN gives bin 0);
 * each element adds 1 to hist[2*b + positive] on the device (integer adds, so the result is exact and independent of
 * their order); then tp[k] = sum over b > k of hist[b][1], fp[k] = sum over b > k of hist[b][0], fn[k] = P - tp[k]
 * with P the number of positives (these K + 1 suffix sums run on the host). */
int rfi_threshold_sweep(rfi_ctx* ctx, const float* scores, int scores_mem, int kind, const void* truth, int truth_dtype,
                        int truth_mem, int64_t count, int64_t group_elems, const float* thresholds_host,
                        int n_thresholds, int64_t* counts_host);

/* ---- whole-observation prediction: the inverse of the inference-mode tiling of Preprocessor.create_dataset
 *      (preprocessing/preprocessor.py:281,317-351 keeps `original_shapes` for it; nothing in the reference inverts it).
 *      Tiling of an n_planes x C x T stack by `rfi_tiling`:
 *        views 1, 2 or 4 select views {0}, {0,1}, {0,1,2,3} (rfi_patch_src's meanings);
 *        tile origins along an axis of length L: 0 when L <= ps, else 0, s, 2s, ..., k*s with k = ceil((L-ps)/s);
 *        edge RFI_EDGE_PAD: the last tile may run past the edge (zero padding; s == ps is the reference's tiling),
 *        edge RFI_EDGE_SHIFT: the last origin is L-ps instead, so no tile holds padding;
 *        patch order: plane-major, then view, then tile row, then tile column (row-major in view coordinates).
 *      Stitch: per waterfall pixel, every (view, tile) that covers it is visited in ascending view, tile row, tile
 *      column order; each visit reads p = 1.0f / (1.0f + expf(-x)) (kind RFI_VALUES_LOGITS) or x itself
 *      (RFI_VALUES_PROBS); combine RFI_COMBINE_MEAN: float32 running sum in that order / float32 count,
 *      RFI_COMBINE_MAX: the maximum.  flag = combined > threshold.  Padding never reaches the output.  Gather form,
 *      no atomics: bitwise reproducible. ---- */
typedef struct rfi_tiling {
    int32_t ps, stride, edge, views;
} rfi_tiling;
enum { RFI_EDGE_PAD = 0, RFI_EDGE_SHIFT = 1 };
enum { RFI_COMBINE_MEAN = 0, RFI_COMBINE_MAX = 1 };
enum { RFI_VALUES_LOGITS = 0, RFI_VALUES_PROBS = 1 };
/* host only: the number of patches one C x T plane is cut into */
int rfi_tiling_count(int c, int t, const rfi_tiling* tiling, int64_t* patches_per_plane);
/* host only: the patches of n_units planes of C x T (an axis of length 0 has the one origin 0) as table entries, in the patch
 * order above with `plane` counting the units; writes n_units x patches_per_plane entries (none for n_units == 0), an error
 * when `capacity` entries do not hold them */
int rfi_tiling_table(int c, int t, const rfi_tiling* tiling, int n_units, rfi_patch_src* table_host, int64_t capacity);
/* values: n_planes x patches_per_plane patches of ps x ps float32 in the order above; flags: n_planes x C x T uint8;
 * prob (optional, NULL = none): n_planes x C x T float32 combined values.  Returns when the outputs are in place. */
int rfi_stitch_patches(rfi_ctx* ctx, const float* values, int values_mem, int kind, int n_planes, int c, int t,
                       const rfi_tiling* tiling, int combine, float threshold, uint8_t* flags, int flags_mem,
                       float* prob, int prob_mem);
/* the same for patches of n_classes channel-last values (n_planes x patches_per_plane x ps x ps x n_classes): class k is
 * stitched on its own into plane `plane * n_classes + k` of flags / prob (n_planes x n_classes x C x T).  n_classes == 1 is
 * rfi_stitch_patches */
int rfi_stitch_patches_classes(rfi_ctx* ctx, const float* values, int values_mem, int kind, int n_planes, int n_classes, int c,
                               int t, const rfi_tiling* tiling, int combine, float threshold, uint8_t* flags, int flags_mem,
                               float* prob, int prob_mem);
/* the whole pipeline on a model with 3 input channels and 1 output channel: planes (n_planes x C x T, RFI_C128 or
 * RFI_C64, host or device) are streamed through in chunks of whole planes -- upload, gather + channel extraction
 * (rfi_preprocess_gather's kernels), EVAL-mode forward in sub-batches of `batch` patches (BatchNorm on the running
 * statistics whatever the model's mode; running buffers untouched), stitch of the model's output (logits, or the
 * probabilities of a sigmoid-head model: never sigmoided twice), download.  Device workspace is bounded by one chunk
 * (at most 1 GiB, held in the context's grow-only scratch for later calls); a single plane too large for it is an
 * error.  Returns when the outputs are in place. */
int rfi_model_predict_flags(rfi_model* m, const void* planes, int planes_mem, int dtype, int n_planes, int c, int t,
                            const rfi_tiling* tiling, int batch, int combine, float threshold, uint8_t* flags,
                            int flags_mem, float* prob, int prob_mem);

/* ---- flagging-quality statistics: the reductions of evaluation/statistics.py:10-229 over a whole array.
 *      data: `count` elements of dtype RFI_C128 / RFI_C64 / RFI_F64 / RFI_F32 (complex: |z| by NumPy's rule
 *      L * sqrt(fma(S/L, S/L, 1)), L = max(|re|,|im|), S = min, in the input's precision); flags: `count` bytes of
 *      flags_dtype RFI_U8 (non-zero == flagged) or NULL (nothing flagged).  `want` is a bit set of RFI_FS_ALL (the
 *      statistics of every element -> all_out), RFI_FS_CLEAN (of the unflagged elements -> clean_out) and
 *      RFI_FS_MEDIANS (also median and MAD).  Medians, MAD and max are exact and, like mean and std, in float32
 *      for float32 / complex64 input (float32 values returned as doubles); mean and std are two-pass fp64 sums.
 *      Any NaN among a view's values makes its mean, std, median, MAD and max NaN (np.median, not nanmedian);
 *      an empty view has count 0 and NaN statistics.  One call, one device synchronisation, bitwise reproducible;
 *      with no flag set the unflagged view is bit-identical to the all view. ---- */
typedef struct rfi_flag_stats {
    int64_t count;       /* elements in the view */
    int64_t flagged;     /* flagged elements of the whole input */
    double mean, std, median, mad, max;
} rfi_flag_stats;
enum { RFI_FS_ALL = 1, RFI_FS_CLEAN = 2, RFI_FS_MEDIANS = 4 };
int rfi_flag_statistics(rfi_ctx* ctx, const void* data, int data_mem, int dtype, int64_t count,
                        const void* flags, int flags_mem, int flags_dtype, int want,
                        rfi_flag_stats* all_out, rfi_flag_stats* clean_out);

/* ---- RFISimulator on device: the 4-polarisation coherent-phase waterfalls and full-truth masks of
 *      rfi_toolbox/core/simulator.py:147-237 (generate_rfi) and :137-145 (generate_clean_data), n_samples at once.
 *      Physics and order of addition are the reference's, in fp64; the random stream is Philox4x32-10
 *      (10 rounds, multipliers 0xD2511F53 / 0xCD9E8D57, key bumps 0x9E3779B9 / 0xBB67AE85), key (seed lo, seed hi),
 *      counter (c0 position, c1 event, c2 stream, c3 global sample index = first_sample + s).  A draw depends
 *      on nothing else, so results do not depend on the launch geometry or on how samples are split into calls.
 *
 *      Word -> value mappings (a, b, w: 32-bit words):
 *        u53(a, b)      = ((a >> 5) * 2^26 + (b >> 6)) * 2^-53          in [0, 1) (NumPy's random_sample rule)
 *        uniform(lo,hi) = lo + (hi - lo) * u53                           (NumPy's order of operations)
 *        randint(lo,hi) = lo + ((uint64) w * (hi - lo)) >> 32            in [lo, hi)
 *        sign(w)        = w >> 31 ? -1.0 : +1.0
 *        power(w)       = power_range[((uint64) w * n_power) >> 32]
 *        normals        = Box-Muller: r = sqrt(-2 ln((a + 1) 2^-32)), th = 2 pi b 2^-32 -> (r cos th, r sin th)
 *
 *      Event table (drawn on device into events_dev, RFI_SIM_SLOTS(T, F) records per sample, in this order):
 *        slot 0                header: i0 = number of broadband chunks (2 or 3), v0 = baseline_frac
 *        slots 1..3            broadband chunks (only the first i0 are used)
 *        NN = int(F * 0.05)    narrowband channels;  NB = int(T * 0.1) burst rows
 *        5 linear sweeps, then 5 quadratic sweeps.
 *      Event e of category k draws 20 words w0..w19 = Philox(c0 = j, c1 = e, c2 = k, c3 = sample), j = 0..4 in turn
 *      (k: 0 header, 1 broadband, 2 narrowband, 3 burst, 4 linear, 5 quadratic):
 *        header      baseline_frac = u53(w0, w1) (unless given), chunks = 2 + randint(0, 2) of w2
 *        broadband   i0 start = randint(0, max(1, F - 101)) of w0, i1 width = randint(50, min(150, F - 1 - start))
 *                    of w1, i2 drifting = u53(w4, w5) < drift_prob;           phase extent (width, T)
 *        narrowband  i0 channel = randint(0, F) of w0, i1 drifting (w4, w5), i2 power index of w1, v0 its power;
 *                    phase extent (1, T)
 *        burst       i0 row = randint(0, T) of w0, i2 power index of w1, v0 its power; phase extent (F, 1), fixed
 *        linear      i0 start_t = randint(0, T/2) of w0, i1 start_f = randint(0, F/2) of w1, i2 drifting (w4, w5),
 *                    v0 slope = uniform(-2, 2) of (w16, w17);                 phase extent (1, T/2)
 *        quadratic   i0 start_t = randint(0, T/4) of w0, i1 start_f = randint(0, F/4) of w1, i2 direction =
 *                    sign(w2), drifting;                                      phase extent (1, T/4)
 *      Phase parameters of _draw_event_phase (simulator.py:69-90), extent (w, nt), bl = baseline_frac:
 *        r0 = (uniform(0.5, 1 + bl max_time_fringes) of (w8, w9) / nt) sign(w10)
 *        s0 = (uniform(0.5, 1 + bl max_freq_fringes) of (w12, w13) / w) sign(w11)
 *        phi0 = uniform(0, 2 pi) of (w14, w15)
 *        sdot = drifting ? ((uniform(0.5, 1 + bl max_freq_fringes) of (w6, w7) / w) sign(w3) - s0) / nt : 0
 *
 *      Per-pixel and per-point draws (position, event, stream):
 *        (t F + f, 0, 8)  -> normals RR (re, im), RL (re, im);  (t F + f, 1, 8) -> LR, LL
 *        (t F + f, b, 9)  -> broadband chunk b: modulation uniform(0.5, 2) of (w0, w1), power of w2
 *        (t, k, 10)       -> narrowband k: modulation of (w0, w1);   (f, k, 11) -> burst k: modulation of (w0, w1)
 *        (i, k, 12)       -> linear sweep k, point i: power of w0;    (t, k, 13) -> quadratic sweep k, point t
 *        (t F + f, 0, 14) -> cross-hand factors uniform(0, 1): RL of (w0, w1), LR of (w2, w3)
 *
 *      Per pixel, one gather in the reference's order: RR = noise + broadband (chunk order) + narrowband + bursts
 *      + linear sweeps + quadratic sweeps; LL the same without the quadratic sweeps; RL/LR = noise + factor RR.
 *      Mask: broadband / narrowband / burst pixels with |field| > detect_floor, sweep points with
 *      amp > detect_floor.  gibbs_ringing convolves broadband rows with gibbs_kernel (np.convolve 'same', zero
 *      outside the chunk) and spreads narrowband / burst lines to +-8 channels / rows (kernel cut at the edges);
 *      it never changes the mask.  No atomics: every run is bitwise reproducible.
 *
 *      Sizes: T >= 4, F >= 52 (the reference's randint bounds; clean: T, F >= 1), T F < 2^32, first_sample + n_samples <= 2^32,
 *      1 <= n_power <= 1024.  Outputs (device memory, written in full):
 *        out_layout RFI_SIM_C128 / RFI_SIM_C64: (n, 4, T, F) complex in the order RR, RL, LR, LL;
 *        RFI_SIM_NCHW: (n, 8, T, F) float32, channels RR.re RR.im RL.re RL.im LR.re LR.im LL.re LL.im;
 *        RFI_SIM_NHWC: (n, T, F, 8) float32, the same channels last.  Float outputs are the fp64 values rounded
 *        once.  mask_dev: (n, T, F) uint8.  events_dev: n RFI_SIM_SLOTS(T, F) records (may be NULL when clean);
 *      baseline_frac_dev: n doubles, each sample's baseline_frac (may be NULL).
 *      clean != 0 is generate_clean_data: noise only, an empty mask, no event table; any T, F >= 1.  power_range_dev and
 *      events_dev are device pointers.  Stream-ordered on the context's stream; no synchronisation. ---- */
typedef struct rfi_sim_event {
    int32_t i0, i1, i2, i3;
    double s0, sdot, r0, phi0;   /* phase parameters (header: unused) */
    double v0, v1;               /* v0: power (narrowband, burst), slope (linear), baseline_frac (header) */
} rfi_sim_event;
typedef struct rfi_sim_params {
    int32_t time_bins, freq_bins;
    int32_t n_power;             /* entries of power_range_dev */
    int32_t gibbs_ringing;
    int32_t clean;
    int32_t fixed_baseline;      /* 1: every sample uses baseline_frac; 0: drawn per sample */
    double baseline_frac, detect_floor, drift_prob, max_time_fringes, max_freq_fringes;
    double gibbs_kernel[17];     /* _make_gibbs_kernel(8, 2.0), used when gibbs_ringing */
} rfi_sim_params;
enum { RFI_SIM_C128 = 0, RFI_SIM_C64 = 1, RFI_SIM_NCHW = 2, RFI_SIM_NHWC = 3 };
#define RFI_SIM_SLOTS(T, F) (14 + (int)((double)(F) * 0.05) + (int)((double)(T) * 0.1))
int rfi_simulate_rfi(rfi_ctx* ctx, uint64_t seed, uint64_t first_sample, int n_samples, const rfi_sim_params* params,
                     const double* power_range_dev, int out_layout, void* out_dev, uint8_t* mask_dev,
                     rfi_sim_event* events_dev, double* baseline_frac_dev);

/*      rfi_sim_inject: the events of rfi_simulate_rfi ADDED to visibilities that already exist (RFISimulator.inject), so that
 *      a measured background gets an exact truth.  The event table and every per-pixel draw are those of rfi_simulate_rfi
 *      for the same (seed, first_sample + s); stream 8 (the noise) is not drawn.  params->clean must be 0.
 *
 *      data_dev / out_dev: (n, 4, R, S) complex128 (layout RFI_SIM_C128) or complex64 (RFI_SIM_C64), RR, RL, LR, LL; out_dev
 *      may be data_dev.  rows RFI_INJECT_ROWS_TIME: the planes are (T, F), simulator pixel (t, f) is element [t][f];
 *      RFI_INJECT_ROWS_CHANNEL: they are (F, T) and pixel (t, f) is element [f][t].  mask_dev (n, R, S) uint8 is laid out
 *      like the planes.  sigma_dev: n doubles, the noise scale of each sample's data (finite and positive: the caller checks).
 *      flags_dev: NULL, or uint8 prior flags (n, 4, R, S) (flag_pols 4) or (n, R, S) (flag_pols 1: all four polarisations).
 *
 *      Per pixel, in fp64 (complex64 is widened): rr = RR and ll = LL as loaded, S = 0.  Every contribution v that
 *      rfi_simulate_rfi adds to RR / LL is added in its order as c = (sigma v.re, sigma v.im), each product rounded once
 *      and then added (no fused multiply-add): rr += c, ll += c (the quadratic sweeps: rr only), and S += c whenever rr
 *      gets c.  With gibbs_ringing v is the convolved / spread value.  With sigma = 1.0 this is rfi_simulate_rfi's arithmetic
 *      on its noise.  Cross hands, with the factors frl, flr of draw (t F + f, 0, 14):
 *        RFI_INJECT_CROSS_INJECTED   rl = RL + frl S, lr = LR + flr S             (only where something was added to RR)
 *        RFI_INJECT_CROSS_REFERENCE  rl = RL + frl rr, lr = LR + flr rr           (the reference's rule on the whole RR)
 *      A visibility to which nothing was added, and a visibility whose flag is set, is stored exactly as loaded, bit for bit
 *      (tracked with a flag, not left to x + 0); S does not depend on RR's flag.  Every other one is the fp64 value rounded
 *      once to the data's type.  The mask is rfi_simulate_rfi's: decided in noise units, before sigma, whatever the flags.
 *      events_dev, baseline_frac_dev: as rfi_simulate_rfi fills them.  Sizes: those of rfi_simulate_rfi with clean == 0.
 *      Device pointers only; stream-ordered on the context's stream; no atomics, nothing allocates or synchronises;
 *      results do not depend on the launch geometry.
 *
 *      rfi_sim_transpose_planes: dst[i][c][r] = src[i][r][c] for n byte planes of rows x cols (device, dst != src), the
 *      orientation change of rfi_sim_family_bits' output for a RFI_INJECT_ROWS_CHANNEL batch.  Stream-ordered. */
enum { RFI_INJECT_ROWS_TIME = 0, RFI_INJECT_ROWS_CHANNEL = 1 };
enum { RFI_INJECT_CROSS_INJECTED = 0, RFI_INJECT_CROSS_REFERENCE = 1 };
int rfi_sim_inject(rfi_ctx* ctx, uint64_t seed, uint64_t first_sample, int n_samples, const rfi_sim_params* params,
                   const double* power_range_dev, int layout, int rows, int cross_hand, const void* data_dev,
                   const uint8_t* flags_dev, int flag_pols, const double* sigma_dev, void* out_dev, uint8_t* mask_dev,
                   rfi_sim_event* events_dev, double* baseline_frac_dev);
int rfi_sim_transpose_planes(rfi_ctx* ctx, const uint8_t* src_dev, int64_t n, int rows, int cols, uint8_t* dst_dev);

/*      Per-emitter targets of a generated batch (rfi_toolbox_amd.core.event_instances): one event is one instance.
 *      Both calls take the (seed, first_sample, n_samples, params, power_range_dev, events_dev) of the rfi_simulate_rfi call
 *      that made the batch (sample s draws with c3 = first_sample + s) and recompute, with the pixel kernel's own device
 *      functions, the pixels each event ALONE flags: broadband chunk b < header.i0 its pixels with |field| > detect_floor,
 *      narrowband / burst lines likewise, a sweep its points with amp > detect_floor.  The union over a sample's events is
 *      mask_dev; a pixel flagged by several events is in each of their masks; gibbs_ringing changes nothing.  A sweep that
 *      wraps in frequency (% F) stays one event whose tight box may span the band.
 *
 *      rfi_sim_event_table: with S = RFI_SIM_SLOTS(T, F) - 1, event slot l (1 .. S; slot 0 is the header) of sample i has
 *        entry i S + l - 1:  area int32 [n S] = pixels the event flags;  box int32 [n S][4] = (xmin, ymin, xmax, ymax),
 *        inclusive, x the channel and y the time row, (0, 0, 0, 0) when area is 0.  An unused broadband slot
 *        (b >= header.i0) has area 0.  This is the table rfi_op_instances_select takes with n_components[i] = S and
 *        comp_base[i] = i S; its `component` is then the event slot.  box 16-byte aligned.
 *      rfi_sim_instances: for j < count[i], labels[i][j] (int32 [n][max_instances]) = the class of slot component[i][j]:
 *        class_mode RFI_SIM_CLASS_SINGLE 1 for every event; RFI_SIM_CLASS_FAMILY 1 broadband, 2 narrowband, 3 burst,
 *        4 linear sweep, 5 quadratic sweep (the slot ranges of RFI_SIM_SLOTS); rows >= count[i] are left alone.  With
 *        masks != NULL, masks uint8 [sum of count][T][F]: masks[base[i] + j] is written in full, 1 where that event flags
 *        the pixel and 0 elsewhere (a slot that is no live event gives class 0 and an empty plane).  component, count,
 *        base: the outputs of rfi_op_instances_select.
 *      Sizes: those of rfi_simulate_rfi with clean == 0, and 1 <= max_instances <= 256.  Device pointers only; stream-ordered
 *      on the context's stream; nothing allocates or synchronises; no atomics: results are bitwise reproducible and do not
 *      depend on the launch geometry. */
enum { RFI_SIM_CLASS_SINGLE = 0, RFI_SIM_CLASS_FAMILY = 1 };
int rfi_sim_event_table(rfi_ctx* ctx, uint64_t seed, uint64_t first_sample, int n_samples, const rfi_sim_params* params,
                        const double* power_range_dev, const rfi_sim_event* events_dev, int32_t* area, int32_t* box);
int rfi_sim_instances(rfi_ctx* ctx, uint64_t seed, uint64_t first_sample, int n_samples, const rfi_sim_params* params,
                      const double* power_range_dev, const rfi_sim_event* events_dev, const int32_t* component, const int32_t* count,
                      const int32_t* base, int max_instances, int class_mode, int32_t* labels, uint8_t* masks);
/* per-family segmentation targets of the same batch (rfi_toolbox_amd.core.family_masks), class-bit labels for
 * rfi_model_set_label_mode: bits uint8 [n_samples][T][F], bit cat - 1 set where an event of category cat (1 broadband, 2
 * narrowband, 3 burst, 4 linear sweep, 5 quadratic sweep) flags the pixel -- the OR by category of the instance masks of
 * every event, without forming them.  bits != 0 is mask_dev; gibbs_ringing changes nothing.  A gather over all event slots,
 * 16 bytes stored at a time; sizes and guarantees as above. */
int rfi_sim_family_bits(rfi_ctx* ctx, uint64_t seed, uint64_t first_sample, int n_samples, const rfi_sim_params* params,
                        const double* power_range_dev, const rfi_sim_event* events_dev, uint8_t* bits);

/* ---- input normalisation of 8-channel data (datasets/rfi_mask_dataset.py:99-156, scripts/normalize_rfi_data.py).
 *
 *      rfi_norm_statistics: statistics of populations of real scalars held in device memory, dtype RFI_F64 or
 *      RFI_F32 (complex data is passed as its interleaved real scalars: every statistic here is invariant under
 *      permutation).  chunks / counts: `n_chunks` device pointers and their scalar counts (host arrays).
 *        segment == 0   one population: the concatenation of all chunks (n_out must be 1);
 *        segment  > 0   n_chunks must be 1; the chunk is cut into n_out = counts[0] / segment populations of
 *                       `segment` consecutive scalars each, all handled by the same launches.
 *      Per population (out, a host array of n_out records): count, the number of non-finite values, min, max, the fp64
 *      mean and POPULATION variance (two-pass), and for the median, the 25 % and the 75 % quantile (q[0], q[1], q[2])
 *      the two bracketing order statistics of NumPy's default linear method: virtual index v = q (count - 1) formed in
 *      fp64 by rfi_norm_bracket, ranks floor(v) and min(floor(v) + 1, count - 1).  The interpolation between the
 *      brackets is left to the caller; with quantiles == 0 the order statistics are not computed (q is NaN), which
 *      leaves 2 reads of the data instead of 6 (float32: 3).  min, max and the order statistics are exact (radix selection); the sums are
 *      taken over fixed 8192-scalar tiles of the population's index range and reduced in a fixed order, so every
 *      result is bitwise reproducible and independent of how the population is split into chunks.  With
 *      nonfinite != 0 the other fields are unspecified.  Populations: at most 4096, each non-empty.  Synchronises.
 *
 *      rfi_norm_apply: dst = float32((double(src) - centre) / scale), fp64 arithmetic on the exact source value,
 *      rounded once; a pair with scale == 0 writes zeros (min-max normalisation of a constant population).  params_dev
 *      NULL: the pair (centre, scale) for every sample; else a device array of n (centre, scale) pairs, one per
 *      sample.  Source (device): dtype RFI_F64 / RFI_F32 in layout RFI_NORM_NCHW (n, 8, T, F) or RFI_NORM_NHWC
 *      (n, T, F, 8); RFI_C128 / RFI_C64 (n, 4, T, F) in the order RR, RL, LR, LL (src_layout RFI_NORM_NCHW), giving
 *      the channels RR.re RR.im RL.re ... LL.im.  Destination (device): float32 in RFI_NORM_NCHW or RFI_NORM_NHWC;
 *      pixels = T F.  dst may equal src when both have the same dtype and layout, and must not overlap it otherwise.
 *      Stream-ordered on the context's stream; no synchronisation. ---- */
typedef struct rfi_norm_stats {
    int64_t count, nonfinite;
    double min, max, mean, var;
    double q[3][2];      /* [median, 25 %, 75 %][lower, upper bracket] */
} rfi_norm_stats;
enum { RFI_NORM_NCHW = 0, RFI_NORM_NHWC = 1 };
/* ranks[0], ranks[1] = the bracketing 0-based ranks of quantile q among count values; *frac = v - floor(v) */
int rfi_norm_bracket(int64_t count, double q, int64_t* ranks, double* frac);
int rfi_norm_statistics(rfi_ctx* ctx, const void* const* chunks, const int64_t* counts, int n_chunks, int dtype,
                        int64_t segment, int quantiles, rfi_norm_stats* out, int n_out);
int rfi_norm_apply(rfi_ctx* ctx, const void* src_dev, int dtype, int src_layout, int n, int64_t pixels, double centre,
                   double scale, const double* params_dev, float* dst_dev, int dst_layout);

/* ---- whole-observation prediction for 8-channel models: tiling, views, polarisation stacking and normalisation of
 *      rfi_norm_apply in one pass, and the pipeline of rfi_model_predict_flags built on it.
 *
 *      rfi_norm_gather: planes (n_samples, 4, C, T), RFI_C128 or RFI_C64, in the order RR, RL, LR, LL; a table entry's
 *      `plane` is the SAMPLE index and names all four of its planes, `view`, `row0`, `col0` are rfi_patch_src's and apply
 *      to each of them alike.  out_nhwc (n, ps, ps, 8) float32 with the channels RR.re RR.im RL.re ... LL.im
 *      (rfi_norm_apply's order).  Every output value is
 *          scale == 0 ? 0.0f : (float)(((double)x - centre) / scale)
 *      -- rfi_norm_apply's expression: fp64 on the exact source value, a real division, rounded once -- with
 *      (centre, scale) the call's pair when params_host is NULL, else params_host[plane], one {centre, scale} array of
 *      two doubles per sample (n_samples of them, contiguous).  A pixel past the view's edge is the visibility 0 + 0j sent through the same
 *      expression: it is normalised like a sample of no signal, not written as a literal zero.  No atomics; the result
 *      does not depend on the launch geometry.  planes, table_host and out_nhwc are host or device operands as in
 *      rfi_preprocess_gather (the table and the pairs always host); buffers need only their element's alignment and the
 *      table may name any origin.
 *
 *      rfi_model_predict_flags_pol: rfi_model_predict_flags for a model with 8 input channels, 1 output channel and an
 *      output map the size of its input.  The unit of chunking, stitching and output is the sample (one baseline: 4
 *      complex planes in, one C x T plane of flags out): flags and the optional prob are (n_samples, C, T).  The patches
 *      are rfi_norm_gather's, with the same meaning of centre, scale and params_host (n_samples pairs); chunks, the
 *      two-slot upload and download, the eval-mode forward at the full batch and the stitch are those of
 *      rfi_model_predict_flags, and so are the workspace bound (counted with 4 complex planes per sample and 8-channel
 *      image batches) and the error for a single sample that exceeds it.  A model with class-bit labels
 *      (rfi_model_set_label_mode) and K = 2 .. 8 output channels, a per-family flagger, is taken too: every channel is stitched on its own, as
 *      rfi_stitch_patches_classes does, flags and prob are (n_samples, K, C, T), and the workspace bound counts K values
 *      per patch pixel. ---- */
int rfi_norm_gather(rfi_ctx* ctx, const void* planes, int planes_mem, int dtype, int n_samples, int c, int t,
                    const rfi_patch_src* table_host, int n, int ps, double centre, double scale,
                    const double (*params_host)[2], float* out_nhwc, int out_mem);
int rfi_model_predict_flags_pol(rfi_model* m, const void* planes, int planes_mem, int dtype, int n_samples, int c, int t,
                                const rfi_tiling* tiling, int batch, int combine, float threshold, double centre,
                                double scale, const double (*params_host)[2], uint8_t* flags, int flags_mem, float* prob,
                                int prob_mem);

/* ---- validity-aware 8-channel input: prior flags and non-finite samples carried through the normalisation, the
 *      gather and the prediction of 8-channel models.  With no flags and finite data the entry points above are the
 *      ones to call, and nothing of theirs changes; these are separate kernels beside them.
 *
 *      Invalid visibility.  A visibility (one polarisation of one pixel) is INVALID when its prior flag is non-zero, or
 *      its real part is non-finite, or its imaginary part is non-finite.  For real 8-channel input, polarisation p of a
 *      pixel is invalid when its flag is set or channel 2 p or 2 p + 1 is non-finite.  Prior flags are bytes (non-zero
 *      == flagged), RFI_VALID_FLAGS_POL: (n, 4, T, F), one per visibility, or RFI_VALID_FLAGS_BASELINE: (n, T, F), one
 *      per pixel, applying to all four polarisations.  A NULL flags pointer means no prior flag: non-finite values only.
 *
 *      rfi_valid_map: the invalid map of device data in any of rfi_norm_apply's six source forms: map_dev (n, 4, pixels)
 *      bytes, 1 == invalid, and counts[n] (host or device by counts_mem, or NULL), the invalid visibilities per sample.
 *      One read of the data, one byte written per visibility; integer atomics only.  Stream-ordered; synchronises only
 *      to hand host counts back.
 *
 *      rfi_valid_statistics: rfi_norm_statistics over the VALID scalars only (both scalars of a valid visibility,
 *      neither of an invalid one).  Chunk i has the invalid map maps[i] (device, as rfi_valid_map writes it), the form
 *      forms[i] of its scalars -- RFI_VALID_SRC_COMPLEX: interleaved (n, 4, pixels) pairs; RFI_VALID_SRC_PLANAR:
 *      (n, 8, pixels); RFI_VALID_SRC_NHWC: (n, pixels, 8) -- and pixels[i]; counts[i] is a multiple of 8 pixels[i].
 *      Segment and dataset modes as rfi_norm_statistics.  Per population: count is the number of valid scalars; min, max
 *      and the six order statistics are exact over them, the brackets formed from the population's OWN valid count by
 *      rfi_norm_bracket's fp64 rule, evaluated on the device (v = q (count - 1), ranks floor(v) and min(floor(v) + 1,
 *      count - 1)); mean and population variance are two-pass fp64 sums over the same fixed 8192-scalar index tiles, an
 *      invalid scalar contributing nothing, divided by count: bitwise reproducible and independent of chunking and launch
 *      geometry.  When no scalar is invalid the whole record is bit-identical to rfi_norm_statistics'.  A population
 *      with no valid scalar has count 0 and NaN in every other statistic.  nonfinite counts the non-finite scalars among
 *      those the map calls valid (0 for a map from rfi_valid_map).  No floating-point atomics.  Synchronises.
 *
 *      rfi_valid_apply: rfi_norm_apply where both channels of an invalid visibility (map_dev, (n, 4, pixels)) are
 *      written as `fill`, a float32 in normalised units; a valid scalar gets rfi_norm_apply's expression unchanged.  In
 *      place under rfi_norm_apply's rule; the map must not overlap the destination.  Stream-ordered.
 *
 *      rfi_valid_gather: rfi_norm_gather with optional prior flags (n_samples, 4, C, T) or (n_samples, C, T), host or
 *      device like `planes`, and `fill`.  Validity is decided inline from the loaded value and its flag byte; a pixel
 *      past the view's edge stays the normalised value of 0 + 0j and counts as valid.
 *
 *      rfi_model_predict_flags_valid: rfi_model_predict_flags_pol with prior flags `prior` (streamed through the same
 *      two-slot chunk upload as the planes when host memory) and `fill`: the network sees rfi_valid_gather's tiles, and
 *      flags / prob are the model's on that input.  merged (optional, (n_samples, 4, C, T) bytes, host or device; 1
 *      output channel only): merged[b][p] = flags[b] | invalid[b][p], one pass after each chunk's stitch, so a non-finite
 *      or prior-flagged visibility comes back flagged.  The workspace bound counts the prior flag bytes and the merged
 *      output next to rfi_model_predict_flags_pol's.  The (centre, scale) pairs are the caller's: for per-sample
 *      normalisation take them from rfi_valid_statistics. ---- */
enum { RFI_VALID_FLAGS_POL = 0, RFI_VALID_FLAGS_BASELINE = 1 };
enum { RFI_VALID_SRC_COMPLEX = 0, RFI_VALID_SRC_PLANAR = 1, RFI_VALID_SRC_NHWC = 2 };
int rfi_valid_map(rfi_ctx* ctx, const void* src_dev, int dtype, int src_layout, int n, int64_t pixels, const uint8_t* flags_dev,
                  int flags_form, uint8_t* map_dev, int64_t* counts, int counts_mem);
int rfi_valid_statistics(rfi_ctx* ctx, const void* const* chunks, const int64_t* counts, const uint8_t* const* maps,
                         const int* forms, const int64_t* pixels, int n_chunks, int dtype, int64_t segment, int quantiles,
                         rfi_norm_stats* out, int n_out);
int rfi_valid_apply(rfi_ctx* ctx, const void* src_dev, int dtype, int src_layout, int n, int64_t pixels, double centre,
                    double scale, const double* params_dev, const uint8_t* map_dev, float fill, float* dst_dev, int dst_layout);
int rfi_valid_gather(rfi_ctx* ctx, const void* planes, int planes_mem, int dtype, int n_samples, int c, int t,
                     const rfi_patch_src* table_host, int n, int ps, double centre, double scale,
                     const double (*params_host)[2], const uint8_t* flags, int flags_mem, int flags_form, float fill,
                     float* out_nhwc, int out_mem);
int rfi_model_predict_flags_valid(rfi_model* m, const void* planes, int planes_mem, int dtype, int n_samples, int c, int t,
                                  const rfi_tiling* tiling, int batch, int combine, float threshold, double centre,
                                  double scale, const double (*params_host)[2], const uint8_t* prior, int prior_mem,
                                  int prior_form, float fill, uint8_t* flags, int flags_mem, float* prob, int prob_mem,
                                  uint8_t* merged, int merged_mem);
/* The label planes of an observation cut into the tiles rfi_norm_gather / rfi_valid_gather cut the data into, for training
 * with the ignore bit (rfi_model_set_ignore).  labels (n_samples, C, T) bytes, one plane per sample (a map or class bits);
 * invalid: NULL, or the invalid map (n_samples, 4, C, T) as rfi_valid_map writes it (RFI_VALID_FLAGS_POL) or one byte per
 * pixel (n_samples, C, T) (RFI_VALID_FLAGS_BASELINE), non-zero == invalid.  table_host: n_tiles entries of rfi_tiling_table,
 * so the tile order is that of the data tiles by construction.  out (n_tiles, ps, ps) bytes: label | RFI_LABEL_IGNORE where
 * the pixel is invalid -- under the POL form where any (RFI_LABEL_INVALID_ANY) or all (RFI_LABEL_INVALID_ALL) of its four
 * polarisations are -- the label elsewhere, and pad_value (0 .. 255; RFI_LABEL_IGNORE keeps the padding of edge tiles out
 * of the loss) past a view's edge.  One launch per 65535 tiles, no synchronisation when everything is device-resident;
 * n_tiles == 0 is a no-op. */
enum { RFI_LABEL_INVALID_ANY = 0, RFI_LABEL_INVALID_ALL = 1 };
int rfi_label_gather(rfi_ctx* ctx, const uint8_t* labels, int labels_mem, int n_samples, int c, int t, const uint8_t* invalid,
                     int invalid_mem, int invalid_form, int rule, const rfi_patch_src* table_host, int n_tiles, int ps,
                     int pad_value, uint8_t* out, int out_mem);

/* ---- training augmentation (scripts/train_model.py:44-53,70-75, --augment): HorizontalFlip, VerticalFlip, Rotate and
 *      ShiftScaleRotate of a batch and its masks, as flips and ONE resampling through the composed affine transform.
 *      Distribution-level parity: the reference resamples once per transform with its library's own random stream.
 *
 *      x (n, h, w, c) float32 NHWC, 1 <= c <= 16; y (n, h, w) bytes; the outputs have the same shapes in separate
 *      buffers (a gather is never in place).  Sample i of call number `call` draws u[0..11] from three Philox4x32-10
 *      blocks k = 0, 1, 2 with counter (i, call_lo, call_hi, k) and key (seed_lo, seed_hi), the words in order,
 *      u = (word + 0.5) 2^-32 in fp64.  Gates: hflip u0 < p_hflip, vflip u1 < p_vflip, rotate u2 < p_rotate,
 *      shift-scale-rotate u3 < p_ssr.  theta1 = (2 u4 - 1) rotate_limit_deg, theta2 = (2 u5 - 1) ssr_rotate_limit_deg,
 *      s = 1 + (2 u6 - 1) scale_limit, dx = (2 u7 - 1) shift_limit w, dy = (2 u8 - 1) shift_limit h.  About the centre
 *      c = ((w - 1) / 2, (h - 1) / 2) the forward map of pixel coordinates is M = SSR R(theta1) Fv Fh,
 *      SSR = [s cos -s sin dx; s sin s cos dy], gated-off factors the identity; output pixel (xo, yo) reads the source
 *      position M^-1 ((xo, yo) - c) + c, all in fp64.  Image: bilinear over floor and floor + 1, each index reflected
 *      on its own (reflect-101: period 2 (N - 1), the edge pixel not repeated), weights and sum in fp64, one rounding
 *      to float32.  Mask: the byte at (floor(sx + 0.5), floor(sy + 0.5)), reflected the same way.  A sample with the
 *      rotate and ssr gates both off is a copy with the flips applied, bit for bit (non-finite values included).
 *      No atomics: the output is a function of the arguments alone.
 *
 *      rfi_augment_params (host only, no context): gates[n][4] = (hflip, vflip, rotate, ssr) and inv[n][6] = the
 *      row-major 2 x 3 map from an output pixel to its source position, from the same function the kernel evaluates.
 *      rfi_augment_batch: x, y host or device (x_mem, y_mem), x_out, y_out device; one launch on the context's stream,
 *      no synchronisation when the inputs are device-resident.  Probabilities in [0, 1], limits >= 0, scale_limit < 1,
 *      h w <= 2^30; with c % 4 == 0 the float buffers must be 16-byte aligned.  n == 0 is a no-op. ---- */
typedef struct rfi_augment_config {
    uint64_t seed;
    float p_hflip, p_vflip, p_rotate, rotate_limit_deg, p_ssr, shift_limit, scale_limit, ssr_rotate_limit_deg;
} rfi_augment_config;
int rfi_augment_params(const rfi_augment_config* cfg, uint64_t call, int n, int h, int w, int32_t* gates, double* inv);
int rfi_augment_batch(rfi_ctx* ctx, const float* x, int x_mem, const uint8_t* y, int y_mem, int n, int h, int w, int c,
                      const rfi_augment_config* cfg, uint64_t call, float* x_out, uint8_t* y_out);

/* ---- statistical baseline flagger: SumThreshold with a masked smooth background fit and the scale-invariant-rank (SIR)
 *      operator (Offringa et al. 2010, MNRAS 405, 155; Offringa, van de Gronde & Roerdink 2012, A&A 539, A95).  The reference
 *      takes its statistical flaggers from CASA and has no code for this: the semantics below are this project's own, and
 *      tests/sumthreshold_ref.py restates them in NumPy; the library equals it bit for bit (it is built with
 *      -ffp-contract=off, so the operations below are the operations executed).
 *
 *      Planes are (n_planes, C, T) with time contiguous; axis 1 = time, 0 = frequency.  Flags are bytes, non-zero == flagged.
 *
 *      Per plane: X float32 = |z| for complex input (the rule of rfi_flag_statistics, in the input's precision, then rounded
 *      to float32), float64 input rounded to float32.  F = prior | ~isfinite(X); non-finite X are then 0.  B = 0 (float32).
 *      For it = 0 .. iterations - 1:
 *        1  R = X - B in float32.
 *        2  med, mad = NumPy's float32 median of the unflagged R and float32 median of |R - med| (what rfi_flag_statistics
 *           returns with RFI_FS_CLEAN | RFI_FS_MEDIANS).  No unflagged sample, or mad == 0: the plane is finished and goes to
 *           SIR.
 *        3  sigma = 1.4826 * (double) mad.
 *        4  ladder, in double: s = base_sensitivity * 2^(iterations - 1 - it) (repeated doubling); p_0 = 1, p_k = p_{k-1} * rho;
 *           chi_k = ((s * chi_1) * sigma) / p_k, k = 0 .. levels - 1.
 *        5  for each k, M = 2^k: F = pass(R, med, F, M, chi_k, time), then F = pass(R, med, F, M, chi_k, frequency).
 *        6  if it < iterations - 1: B = smooth(X, F).
 *      pass (snapshot semantics: reads F_in, writes F_out; skipped when M exceeds the line length): level 0 is
 *        d_i = unflagged_i ? (double) R_i - (double) med : 0.0, n_i = unflagged_i; level j is d_j(i) = d_{j-1}(i) +
 *        d_{j-1}(i + 2^(j-1)), likewise n (a balanced tree).  Window i, wholly inside the line, hits iff n >= 1 and
 *        fabs(d) > (double) n * chi.  F_out = F_in | the M samples of every hitting window.
 *      smooth: u = 1.0 for unflagged samples, else 0.0; x = u * (double) X.  N1(c, t) = sum over d = -Ht .. Ht ascending of
 *        w_t[d + Ht] * x(c, t + d), taps outside the plane skipped, each product rounded, then added, from 0.0 in double;
 *        D1 the same over u.  The same along frequency on N1 and D1 with w_f gives N2, D2.  B = D2 > 0 ? (float)(N2 / D2) : 0.
 *        The weight tables cross this interface as data: no exponential is evaluated in the library.
 *      SIR, after the last iteration, along time and then along frequency on the result: q = floor(eta * 1024 + 0.5) is formed
 *        by the caller; q == 0 skips it.  Sample k of a line ends flagged iff some a <= k <= b has
 *        1024 * #flagged[a..b] >= (1024 - q) * (b - a + 1): with P the int32 prefix sums of (flagged ? q : q - 1024), iff
 *        max_{j > k} P_j >= min_{j <= k} P_j.
 *      No float atomics; every output is a function of the arguments alone.
 *
 *      rfi_sumthreshold_ladder (host only, no context): chi_out[levels] of `iteration` for a given sigma, by the inline
 *        function the device evaluates.
 *      rfi_sumthreshold_pass: values float32, flags_in / flags_out bytes, host or device; window a power of two in 1 .. 128;
 *        threshold_host / center_host: one double per plane.  A window longer than the line copies the flags.
 *      rfi_masked_smooth: values float32, flags bytes -> out float32; weights_*_host: 2 half + 1 doubles each.
 *      rfi_sir_operator: 0 <= q <= 1023.
 *      rfi_sumthreshold_flag: data of dtype RFI_C128 / C64 / F64 / F32, prior flags optional (NULL).  Planes are processed in
 *        chunks whose workspace (26 bytes per sample, plus staging for host buffers) stays within the context's 1 GiB
 *        grow-only scratch; a single plane too large for it is an error.  Between the upload and the download nothing is read
 *        back: medians, MADs and thresholds stay in device memory.  With device-resident data, prior and flags_out the call
 *        only enqueues work on the context's stream.
 *      Sizes: 1 <= C, T <= 2^20; 1 <= iterations; 1 <= levels <= 8; rho > 1; half widths >= 0. ---- */
typedef struct rfi_sumthreshold_config {
    int32_t iterations, levels;
    double base_sensitivity, chi_1, rho;
    int32_t half_t, half_f;     /* half widths of the smoothing tables (time, frequency) */
    int32_t sir_q;              /* floor(eta * 1024 + 0.5), 0 .. 1023 */
    int32_t pad_;
} rfi_sumthreshold_config;
int rfi_sumthreshold_ladder(const rfi_sumthreshold_config* cfg, double sigma, int iteration, double* chi_out);
int rfi_sumthreshold_pass(rfi_ctx* ctx, const float* values, int values_mem, const uint8_t* flags_in, int flags_mem, int n_planes,
                          int c, int t, int window, int axis, const double* threshold_host, const double* center_host,
                          uint8_t* flags_out, int out_mem);
int rfi_masked_smooth(rfi_ctx* ctx, const float* values, int values_mem, const uint8_t* flags, int flags_mem, int n_planes, int c,
                      int t, const double* weights_t_host, int half_t, const double* weights_f_host, int half_f, float* out,
                      int out_mem);
int rfi_sir_operator(rfi_ctx* ctx, const uint8_t* flags_in, int flags_mem, int n_planes, int c, int t, int axis, int q,
                     uint8_t* flags_out, int out_mem);
int rfi_sumthreshold_flag(rfi_ctx* ctx, const void* data, int data_mem, int dtype, const uint8_t* prior, int prior_mem, int n_planes,
                          int c, int t, const rfi_sumthreshold_config* cfg, const double* weights_t_host,
                          const double* weights_f_host, uint8_t* flags_out, int out_mem);

/* ---- CASA-style baseline flaggers: TFCrop, RFlag and the flag extension (the `tfcrop`, `rflag` and `extend` modes of CASA's
 *      flagdata, which the reference toolbox calls and has no code for).  The semantics below are this project's own,
 *      tests/casa_flaggers_ref.py restates them in NumPy and the library equals it bit for bit.  Planes are (n_planes, C, T)
 *      with time contiguous; flags are bytes, non-zero == flagged.  Every plane is cut along time into chunks of `ntime`
 *      samples (the last may be shorter); the unit of work is (plane, chunk) and nothing crosses a chunk boundary.  All sums
 *      below run sequentially in ascending index from 0.0 in double, a sample outside the mask adding +0.0.
 *
 *      Robust fit of a line y_0 .. y_{L-1} (float32) with mask u: w = u; for j = 0 .. 4:
 *        1  shape "line": one piece of degree 1; shape "poly": that at j = 0, then min(2 j + 1, maxnpieces) pieces of degree 3.
 *           Piece p of n covers samples floor(p L / n) .. floor((p + 1) L / n) - 1 (possibly none).
 *        2  per piece of m samples: x_i = (double)(2 i - (m - 1)) / (double)(m - 1) (0 for m = 1), x2 = x x, x3 = x2 x, x4 = x2 x2,
 *           x5 = x4 x, x6 = x3 x3; S_q = sum_w x^q (q = 0 .. 6), B_q = sum_w x^q (double) y (q = 0 .. 3), k = #w.  d = min(degree,
 *           k - 1).  The normal equations A_rs = S_{r+s}, b_r = B_r (r, s <= d) are padded to 4 x 4 with identity rows (b = 0).
 *           Elimination without pivoting: for p = 0 .. 3, r = p + 1 .. 3: f = A_rp / A_pp; A_rs = A_rs - f A_ps (s = p + 1 .. 3);
 *           b_r = b_r - f b_p.  Back substitution for r = 3 .. 0: s = b_r; s = s - A_rt c_t (t = r + 1 .. 3 ascending); c_r = s / A_rr.
 *           fit_i = ((c_3 x + c_2) x + c_1) x + c_0; r_i = (double) y_i - fit_i.
 *        3  over the w-samples of the whole line: n, s1 = sum r, s2 = sum r r; mean = s1 / n; var = s2 / n - mean mean;
 *           sigma = sqrt(var > 0 ? var : 0), 0 for n = 0.  Unless sigma > 0 the iteration ends here with w as it is.
 *        4  w = w & (fabs(r) <= cutoff sigma).
 *      The line's new flags are u & ~w.
 *
 *      TFCrop: X, F as for the SumThreshold flagger (|z| by the same rule, float32; F = prior | ~isfinite(X); non-finite X <- 0).
 *        Per chunk: m_c = (float)(sum over the unflagged t of (double) X / count), channels without a sample masked; the robust
 *        fit of m along frequency (freqfit, freqcutoff) gives b_c = the fit of its last iteration that ran (its flags are
 *        dropped); Y = (float)((double) X / b_c) where b_c > 0 and finite, else X.  Time stage: the robust fit of every channel
 *        Y[c, :] (timefit, timecutoff) with u = ~F; frequency stage: of every time sample Y[:, t] (freqfit, freqcutoff).
 *        flagdimension orders them (freqtime: time stage first); a stage sees the flags of the one before.
 *      RFlag (complex input only, all in double): F = prior | a non-finite part; non-finite z <- 0.  Both analyses read this F.
 *        Time, per channel of a chunk: over the unflagged samples of t - h .. t + h inside the chunk (h = winsize / 2), n >= 2:
 *        means m = sum / n per part, v = sum (re - m_re)^2 / n + sum (im - m_im)^2 / n, rms_t = sqrt(v > 0 ? v : 0).  Over the
 *        rms_t that exist: med = NumPy's median (the mean (a + b) / 2 of the two middle order statistics), dev = median of
 *        |rms_t - med|; (c, t) is flagged iff rms_t exists and rms_t > timedevscale (med + dev); timedev replaces med + dev.
 *        Spectral, per time sample: the same means and d_t = sqrt(v) across the unflagged channels (n >= 2); one threshold per
 *        chunk, freqdevscale (median + MAD of the d_t that exist), freqdev replacing median + MAD; an unflagged (c, t) whose d_t
 *        exists is flagged iff sqrt((re - a_re)^2 + (im - a_im)^2) > threshold.  A line without a value has threshold
 *        scale * inf.  The result is pinned for data whose variances stay finite.
 *      Extend, per chunk, each step on a snapshot of the one before: growaround (more than 4 of the 8 neighbours inside the
 *        chunk flagged); growtime ((double)(100 count) > growtime (double) n flags the channel for the chunk); growfreq (the same
 *        per time sample across the channels); flagneartime; flagnearfreq.
 *
 *      Planes are processed in groups whose workspace stays within the context's 1 GiB scratch (tfcrop 35, rflag 26, extend 2
 *      bytes per sample, a little per plane, plus staging for host buffers); a single plane too large for it is an error.
 *      Nothing is read back between the upload and the download; with device-resident buffers a call only enqueues work.
 *      timedev_host: NULL or n_planes * C doubles; freqdev_host: NULL or n_planes doubles.
 *      Sizes: 1 <= C, T <= 2^20; 1 <= ntime; 1 <= maxnpieces; winsize odd >= 1; cutoffs and scales >= 0; 0 <= grow* <= 100. ---- */
enum { RFI_TFCROP_FREQTIME = 0, RFI_TFCROP_TIMEFREQ = 1, RFI_TFCROP_TIME = 2, RFI_TFCROP_FREQ = 3 };
typedef struct rfi_tfcrop_config {
    int32_t ntime;              /* a value >= T means the whole axis */
    int32_t timefit, freqfit;   /* 0 "line", 1 "poly" */
    int32_t maxnpieces, flagdimension, pad_;
    double timecutoff, freqcutoff;
} rfi_tfcrop_config;
typedef struct rfi_rflag_config {
    int32_t ntime, winsize;
    double timedevscale, freqdevscale;
} rfi_rflag_config;
typedef struct rfi_extend_config {
    int32_t ntime, growaround, flagneartime, flagnearfreq;
    double growtime, growfreq;
} rfi_extend_config;
int rfi_tfcrop_flag(rfi_ctx* ctx, const void* data, int data_mem, int dtype, const uint8_t* prior, int prior_mem, int n_planes, int c,
                    int t, const rfi_tfcrop_config* cfg, uint8_t* flags_out, int out_mem);
int rfi_rflag_flag(rfi_ctx* ctx, const void* data, int data_mem, int dtype, const uint8_t* prior, int prior_mem, int n_planes, int c,
                   int t, const rfi_rflag_config* cfg, const double* timedev_host, const double* freqdev_host, uint8_t* flags_out,
                   int out_mem);
int rfi_extend_flags(rfi_ctx* ctx, const uint8_t* flags_in, int flags_mem, int n_planes, int c, int t, const rfi_extend_config* cfg,
                     uint8_t* flags_out, int out_mem);

/* ---- connected components: labelling of binary planes, the component table, despeckling and the detector's instance
 *      targets (csrc/components.hip; rfi_toolbox_amd/components.py).  Not in the reference; the labelling equals
 *      scipy.ndimage.label bit for bit and tests/components_ref.py restates the rest in NumPy.  All integer work: results are
 *      exact and do not depend on launch geometry or on the order of atomics.
 *
 *      Input: n planes [n][H][W] of RFI_U8 or RFI_FLOAT32; any non-zero element is foreground (rfi_confusion_counts' rule;
 *      NaN is non-zero).  Planes are independent: the last row of plane i and the first row of plane i + 1 are not
 *      neighbours.  connectivity 4 (edge neighbours) or 8 (edge and corner neighbours).  H, W >= 1, H W <= 2^30, n <= 65535.
 *
 *      Labels: int32 [n][H][W], 0 for background; the components of a plane are numbered 1 .. K by the smallest linear index
 *      y W + x each one contains -- scipy.ndimage.label(mask != 0, generate_binary_structure(2, 1 | 2)).  n_components[i] = K.
 *      Table: with comp_base[i] = the exclusive prefix sum of n_components (the caller's; `total` = its sum, < 2^31),
 *      component l of plane i has slot comp_base[i] + l - 1: area int32 [total]; box int32 [total][4] = (xmin, ymin, xmax,
 *      ymax), inclusive.
 *      Despeckle (components_keep): out uint8 [n][H][W] = foreground AND area of its component >= min_area.
 *      Instances, per plane: a component survives when area >= min_area, xmax - xmin + 1 >= min_side and ymax - ymin + 1 >=
 *      min_side.  The G = max_instances (1 .. 256) survivors of largest area are kept, ties to the smaller label, and written
 *      in descending area, ties ascending label, whether or not anything was cut: boxes float32 [n][G][4] = (xmin, ymin,
 *      xmax + 1, ymax + 1) (the half-open boxes of the detector's targets), labels int32 [n][G] = 1, component int32 [n][G] =
 *      the label the slot came from; rows >= count[i] are zero.  count [n]; n_survivors [n] (> count: the plane was cut);
 *      base [n] = the exclusive prefix sum of count.  instance_masks: masks uint8 [sum of count][H][W],
 *      masks[base[i] + j] = (labels_i == component[i][j]).
 *
 *      Method: label equivalence with union-find -- a pixel starts as its own parent, a union is atomicMin on the larger
 *      root, judged by the value the atomic returned; tiles of 32 x 64 pixels in LDS, unions across the tile borders, then
 *      flatten / count roots / scan / rank / renumber in launches of their own.  components_limits gives the tile's height and
 *      width and the pixels of one root count (where the code's paths change).  The selection orders keys
 *      (~area << 32 | label); with more than G survivors the G-th key is found by a radix select first.
 *
 *      Every pointer is a device pointer; nothing here allocates or synchronises.  workspace: rfi_components_ws_bytes(n, h, w)
 *      bytes (0 for sizes out of range), 256-byte aligned, kept until the stream has passed; box and boxes 16-byte aligned.
 *      copy_rows: `rows` rows of width_bytes from src (rows src_pitch bytes apart) to dst (dst_pitch), device to device on
 *      the context's stream: how instance targets of stride G reach the detector's buffers of another stride. ---- */
int rfi_components_limits(int32_t* tile_h, int32_t* tile_w, int32_t* scan_block);      /* host only */
size_t rfi_components_ws_bytes(int n, int h, int w);                                    /* host only */
int rfi_op_label_components(rfi_ctx* ctx, const void* masks, int dtype, int n, int h, int w, int connectivity, void* workspace,
                            int32_t* labels, int32_t* n_components);
int rfi_op_component_table(rfi_ctx* ctx, const int32_t* labels, int n, int h, int w, const int32_t* comp_base, int64_t total,
                           int32_t* area, int32_t* box);
int rfi_op_components_keep(rfi_ctx* ctx, const int32_t* labels, int n, int h, int w, const int32_t* comp_base, const int32_t* area,
                           int min_area, uint8_t* out);
int rfi_op_instances_select(rfi_ctx* ctx, const int32_t* n_components, const int32_t* comp_base, const int32_t* area, const int32_t* box,
                            int n, int min_area, int min_side, int max_instances, float* boxes, int32_t* labels, int32_t* count,
                            int32_t* n_survivors, int32_t* base, int32_t* component);
int rfi_op_instance_masks(rfi_ctx* ctx, const int32_t* labels, int n, int h, int w, const int32_t* component, const int32_t* count,
                          const int32_t* base, int max_instances, uint8_t* masks);
int rfi_op_copy_rows(rfi_ctx* ctx, const void* src, size_t src_pitch, void* dst, size_t dst_pitch, size_t width_bytes, size_t rows);

/* ---- instance matching: scoring a detector's output against per-instance ground truth (csrc/instance_match.hip;
 *      rfi_toolbox_amd/evaluation/detection.py).  Not in the reference; tests/instance_match_ref.py restates every rule in NumPy
 *      and the results are equal bit for bit: integers, and float32 / float64 in the operation order pinned here.
 *
 *      An image i has det_count[i] detections in slots 0 .. D - 1 and gt_count[i] ground truths in slots 0 .. G - 1
 *      (1 <= D, G <= 256, 1 <= n <= 65535; counts are cut to 0 .. D and 0 .. G).  Every output entry whose detection slot is
 *      >= det_count[i] or whose ground-truth slot is >= gt_count[i] is 0 (IoU, intersection) or -1 (matches), and no kernel reads
 *      a mask, box, score or label behind a count: those slots may hold anything.
 *
 *      pack_masks: masks uint8 [m][H][W], any non-zero byte foreground; H, W >= 1, H W <= 2^24, 1 <= m < 2^31; no alignment is
 *      asked of `masks`.  With Wc = ceil(W / 64): bits uint64 [m][H][Wc], pixel (y, x) is bit x & 63 of word [y][x >> 6], the
 *      bits of a row's last word beyond W are zero; area int32 [m] = the foreground pixels; extent int32 [m][4] = (first row,
 *      first word column, last row + 1, last word column + 1) over the non-zero words, (0, 0, 0, 0) for an empty mask.
 *
 *      mask_iou: each side is (bits, area, extent) over `planes` packed planes plus count [n] and base [n]; slot s of image i is
 *      plane base[i] + s (detections: base[i] = i D; targets: the exclusive prefix sum of count).  A plane index outside
 *      0 .. planes - 1 counts as an empty mask of area 0; extents are cut to the plane.  inter int32 [n][D][G] = sum of
 *      popcount(a & b) over the words inside both extents; union = area_d + area_g - inter in integers;
 *      iou float32 [n][D][G] = (float)((double)inter / (double)union), 0 where union == 0.
 *
 *      box_iou: boxes float32 [n][D][4] and [n][G][4] = (x1, y1, x2, y2), all in float32 without contraction, in the order of
 *      the detector's own IoU: iw = max(min(ax2, bx2) - max(ax1, bx1), 0), ih likewise from y, inter = iw * ih,
 *      union = ((ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1)) - inter, iou = inter / union, 0 where union <= 0.
 *
 *      match_instances: COCO's evaluateImg without crowd or ignore regions, for T thresholds (`thresholds`: T float32 on the
 *      HOST, 1 <= T <= 32, each finite and in (0, 1]) in one launch.  Per (image, threshold t): the detections are taken in
 *      descending score, ties by ascending slot (the order is computed here, the input need not be sorted; -0 counts as +0);
 *      each takes the still-unmatched ground truth of greatest iou among those with iou >= t, ties to the lowest slot, and,
 *      with class_aware != 0, among those with gt_labels == its det_labels only; a detection with no such ground truth stays
 *      unmatched.  det_match int32 [n][T][D] and gt_match int32 [n][T][G] hold the partner's slot or -1.
 *
 *      Method: a wave packs 64 bytes into one word with one ballot; the IoU runs one workgroup per (image, detection) with the
 *      detection's extent window in LDS (up to 4096 words; read in place beyond), waves over ground truths, lanes over the
 *      words of the shared window; matching is one wave per (image, threshold).
 *
 *      Every pointer but `thresholds` is a device pointer aligned to its element size; nothing here allocates or
 *      synchronises. ---- */
int rfi_op_pack_masks(rfi_ctx* ctx, const uint8_t* masks, int64_t m, int h, int w, uint64_t* bits, int32_t* area, int32_t* extent);
int rfi_op_mask_iou(rfi_ctx* ctx, const uint64_t* det_bits, const int32_t* det_area, const int32_t* det_extent, const int32_t* det_count,
                    const int32_t* det_base, int64_t det_planes, const uint64_t* gt_bits, const int32_t* gt_area, const int32_t* gt_extent,
                    const int32_t* gt_count, const int32_t* gt_base, int64_t gt_planes, int n, int d, int g, int h, int w, int32_t* inter,
                    float* iou);
int rfi_op_box_iou(rfi_ctx* ctx, const float* det_boxes, const int32_t* det_count, const float* gt_boxes, const int32_t* gt_count, int n, int d,
                   int g, float* iou);
int rfi_op_match_instances(rfi_ctx* ctx, const float* iou, const float* scores, const int32_t* det_labels, const int32_t* det_count,
                           const int32_t* gt_labels, const int32_t* gt_count, int n, int d, int g, const float* thresholds, int t,
                           int class_aware, int32_t* det_match, int32_t* gt_match);

/* ---- instance stitch: the detections of the tiles of an observation -> one event per emitter of the whole plane
 *      (csrc/instance_stitch.hip; rfi_toolbox_amd/inference.py stitch_instances, detect_observation).  The instance counterpart
 *      of rfi_stitch_patches.  Not in the reference; tests/instance_stitch_ref.py restates every rule in NumPy and the results
 *      are equal bit for bit.
 *
 *      Input: the detections of N = n_planes x patches_per_plane tiles in rfi_tiling order, in the layout of
 *      MaskRCNN.detect(out="device"): boxes float32 [N][D][4] xyxy in tile coordinates, scores float32 [N][D], labels int32 [N][D],
 *      counts int32 [N] (cut to 0 .. D), masks uint8 [N][D][ps][ps], any non-zero byte foreground; 1 <= D <= 256; slot j of
 *      tile i is valid when j < counts[i], and nothing behind a count is read.
 *
 *      Geometry (what rfi_stitch_patches inverts): tile pixel (r, c) of a tile with origin (row0, col0) in view v is view
 *      pixel (row0 + r, col0 + c), dropped when it lies past the view's edge (padding); the views are plane, plane[::-1, :],
 *      plane.T, plane.T[::-1, :].  A tile's rectangle is the image of its non-padding pixels in plane coordinates.  A box maps
 *      with the same transform in float32, one operation per step: add the origin as float (x += col0, y += row0); a mirrored
 *      view (1, 3) makes y = (float)L - y with L the view's row count; a transposed view (2, 3) swaps x and y; x1 <= x2 and
 *      y1 <= y2 are restored by swapping the pair; clip x to [0, T] and y to [0, C].
 *
 *      Members: a valid slot with score >= min_score whose mask has at least min_area (>= 1) non-zero pixels inside the plane.
 *      Links: two members of one plane are linked when they come from different tiles, carry the same label (class_aware != 0
 *      only), and either their tile rectangles intersect and the two masks share a plane pixel, or their tile rectangles are
 *      disjoint and a pixel of one is adjacent to a pixel of the other (connectivity 8: Chebyshev distance 1; 4: Manhattan
 *      distance 1).  Members of one tile are never linked.
 *      Events: the connected components of the link graph.  id = the smallest member index i D + j; mask = OR of the members'
 *      masks on the plane; box = min / min / max / max of the members' mapped boxes; score = the maximum member score; label =
 *      the label of the member with the highest score, ties to the smaller member index (with class_aware the common label).
 *      Output per plane: events by descending score, ties to the smaller id; the first max_events (1 .. 256 = E) are written:
 *      out_boxes float32 [P][E][4], out_scores [P][E], out_labels int32 [P][E], out_counts int32 [P], out_masks uint8
 *      [P][E][C][T] (0 / 1; NULL = not wanted), all zero behind out_counts.  rfi_mask uint8 [P][C][T] is the OR of ALL members'
 *      masks, whether or not the cap cut their event: flags do not depend on max_events.
 *
 *      Known limit: the link test is boolean.  Two same-class emitters that touch across a seam merge, and with overlapping
 *      tiles two same-class emitters that cross merge; the simulator's families put crossing lines in different classes, so
 *      class_aware keeps those apart.
 *
 *      Limits: n_planes <= 65535, C T < 2^31, N D < 2^31, patches_per_plane x D <= 65536 (one sort segment per plane).
 *      Device pointers aligned to their element size (masks aligned to 16 bytes with ps % 16 == 0 are read with 16-byte
 *      loads); stream-ordered: nothing is synchronised, the workspace is the context's grow-only scratch. ---- */
int rfi_stitch_instances(rfi_ctx* ctx, const float* boxes, const float* scores, const int32_t* labels, const int32_t* counts,
                         const uint8_t* masks, int n_planes, int c, int t, const rfi_tiling* tiling, int d, int max_events, int min_area,
                         float min_score, int class_aware, int connectivity, float* out_boxes, float* out_scores, int32_t* out_labels,
                         int32_t* out_counts, uint8_t* rfi_mask, uint8_t* out_masks);

/* ---- kernel-level entry points (device pointers only).  Used by the parity tests to
 *      check each HIP kernel against the oracle in isolation.  impl: 0 auto, 1 direct VALU,
 *      2 MFMA implicit GEMM in native float32 (v_mfma_f32_32x32x2_f32), 3 MFMA implicit GEMM with bfloat16
 *      operands rounded in registers, 4 MFMA implicit GEMM, float32 by 3 x bf16 splitting in registers (the
 *      models' default arithmetic), 5 / 6 the plane kernels (bf16 pieces staged by LDS-DMA from plane tensors;
 *      3x3 convolutions) in the 3 x bf16 / bf16 arithmetic -- the kernels of the bfloat16 compute mode. ---- */
int rfi_op_conv3x3(rfi_ctx* ctx, int impl, const float* x, int n, int h, int w, int cin,
                   const float* w_oihw, const float* bias, int cout,
                   const float* in_scale, const float* in_shift, int in_relu, float* y);
/* 1x1 stride-1 conv (a GEMM over the pixels): the Bottleneck / pyramid / fully connected layers of the detector (A11). */
int rfi_op_conv1x1(rfi_ctx* ctx, int impl, const float* x, int n, int h, int w, int cin, const float* w_oihw, const float* bias,
                   int cout, const float* in_scale, const float* in_shift, int in_relu, float* y);
int rfi_op_conv3x3_dgrad(rfi_ctx* ctx, int impl, const float* dy, int n, int h, int w, int cout,
                         const float* w_oihw, int cin, float* dx);
int rfi_op_conv3x3_wgrad(rfi_ctx* ctx, int impl, const float* x, const float* dy, int n, int h,
                         int w, int cin, int cout, const float* in_scale, const float* in_shift,
                         int in_relu, float* dw_oihw);
/* stride-2 convolutions of the ResNet-style encoder (ksize 3: Conv2d(k3, s2, p1, bias=False) run as a 2x2 stride-1
 * convolution on the space-to-depth input; ksize 1: Conv2d(k1, s2, bias=False), the projection shortcut).  h, w =
 * INPUT size (even), cin % 4 == 0; y / dy are n x h/2 x w/2 x cout, dx is n x h x w x cin. */
int rfi_op_conv_s2(rfi_ctx* ctx, int impl, int ksize, const float* x, int n, int h, int w, int cin,
                   const float* w_oihw, int cout, float* y);
int rfi_op_conv_s2_dgrad(rfi_ctx* ctx, int impl, int ksize, const float* dy, int n, int h, int w, int cout,
                         const float* w_oihw, int cin, float* dx);
int rfi_op_conv_s2_wgrad(rfi_ctx* ctx, int impl, int ksize, const float* x, const float* dy, int n, int h, int w,
                         int cin, int cout, float* dw_oihw);
int rfi_op_convt2x2(rfi_ctx* ctx, int impl, const float* x, int n, int h, int w, int cin,
                    const float* w_iohw, const float* bias, int cout, float* y);
int rfi_op_convt2x2_dgrad(rfi_ctx* ctx, int impl, const float* dy, int n, int h, int w, int cout,
                          const float* w_iohw, int cin, float* dx);
int rfi_op_convt2x2_wgrad(rfi_ctx* ctx, int impl, const float* x, const float* dy, int n, int h,
                          int w, int cin, int cout, float* dw_iohw);
/* Building blocks of the Mask R-CNN path of BASELINE.json configs[3].  NOT in the reference
 * (no detector code exists there, docs/API.md:180 and README.md:90 only name one); defined by the published
 * algorithms: RoIAlign (He et al. 2017; the sampling rules of the public torchvision.ops.roi_align: rois =
 * r x (batch index, x1, y1, x2, y2), bilinear samples, sampling_ratio <= 0 -> ceil(roi extent / bins), `aligned`
 * shifts by half a pixel) over an NHWC float32 feature map, out [r][ph][pw][c]; and the FPN top-down merge (Lin et
 * al. 2017): out = lateral + nearest-neighbour 2x upsampling of top [n][ceil(h/2)][ceil(w/2)][c].  Device pointers.
 * RoIs with x2 >= x1 and y2 >= y1 only: a RoI of zero width or height is sampled on its edge (`aligned`; otherwise its extent
 * is raised to one pixel) and roi_align_backward is the adjoint of that; inverted boxes (x2 < x1 or y2 < y1) are outside the
 * contract of the forward and the backward pass alike. */
int rfi_op_roi_align(rfi_ctx* ctx, const float* x, int n, int h, int w, int c, const float* rois, int r,
                     float spatial_scale, int ph, int pw, int sampling_ratio, int aligned, float* out);
/* roi_align_backward: the gradient w.r.t. the feature map, by gather.  Contract: the RoIs are sorted by batch index
 * (ascending), c % 4 == 0, and every element of dx [n][h][w][c] is WRITTEN exactly once (no prior zeroing, no accumulation).
 * No float atomics: bit-reproducible.  Device pointers; does not allocate or synchronise. */
int rfi_op_roi_align_backward(rfi_ctx* ctx, const float* dout, int n, int h, int w, int c, const float* rois_sorted, int r,
                              float spatial_scale, int ph, int pw, int sampling_ratio, int aligned, float* dx);
/* mask_targets: the training targets of the mask branch -- RoIAlign (rules above, scale 1, not aligned) of one-channel
 * uint8 instance masks [g][h][w], thresholded at 0.5: rois[r] = (instance index, x1, y1, x2, y2) -> out uint8 [r][ph][pw].
 * Device pointers. */
int rfi_op_mask_targets(rfi_ctx* ctx, const uint8_t* masks, int g, int h, int w, const float* rois, int r, int ph, int pw,
                        int sampling_ratio, uint8_t* out);
/* Region-proposal pieces (not in the reference: Faster R-CNN's box parameterisation and RPN loss, greedy IoU
 * NMS, oracle/detection_ref.py).  All tensors device pointers unless named *_host.
 * box_decode: boxes[n][4] = decode(anchors[n_anchors][4] repeating, deltas[n][4]) (weights 1, dw/dh <= log(1000/16)),
 *   clipped to [0, clip_w] x [0, clip_h] when clip_w > 0.
 * nms: boxes sorted by descending score -> indices kept by greedy suppression at IoU > iou_threshold (host array of n ints).
 * rpn_loss: head output [pixels][5 A] (A objectness logits, then A x 4 deltas), labels int8 [pixels A] in {1, 0, -1 =
 *   not sampled}, regression targets [pixels A][4]; with count = max(*num_sampled_dev, 1), an int32 on the device (the
 *   sampler's count): objectness = sum BCE over sampled / count, box = sum smooth-L1 (beta) over positives / count; dhead =
 *   gradient of (objectness + box) w.r.t. the head output; loss2_dev[0..1] = (objectness, box) on the device.  Workspace:
 *   rfi_op_rpn_loss_ws_bytes() bytes of device memory the caller keeps until the stream has passed.  Does not allocate or
 *   synchronise. */
int rfi_op_box_decode(rfi_ctx* ctx, const float* anchors, int64_t n_anchors, const float* deltas, int64_t n, float clip_h,
                      float clip_w, float* boxes);
int rfi_op_nms(rfi_ctx* ctx, const float* boxes_sorted, int n, float iou_threshold, int32_t* keep_host, int* n_keep);
/* Batched forms -- one launch for every image of a batch, all tensors device pointers.
 * anchor_match_batched: the Matcher + BoxCoder.encode of RPN / RoI training -- per anchor the first-argmax ground truth,
 *   label 1 (IoU >= fg_iou, or, with allow_low_quality, the anchor attains some ground truth's best IoU), 0 (IoU < bg_iou, or
 *   gt_count[b] == 0), -1 (between); matched = ground-truth index for labels 1 (else -1); targets (may be null) = encoded
 *   deltas of the positives, zeros elsewhere.  Anchors shared by the images (anchor_stride 0: [n][4]) or per image
 *   (anchor_stride = n: [images][n][4] with anchor_count[b] valid rows -- the proposals of the RoI stage; null: all n);
 *   gt_boxes [images][gt_max][4] (gt_max >= 1) with gt_count[b] valid rows; labels / matched [images][n], targets
 *   [images][n][4].  A row beyond anchor_count[b] gets label -2.  A zero-area anchor and a zero-area ground truth have no IoU
 *   (union 0): the pair never matches, so an anchor with nothing but such pairs gets label 0, matched -1 and zero targets, and
 *   such a ground truth makes no low-quality match.  best_ws: a workspace of images x gt_max floats on the
 *   device that the caller keeps until the stream has passed.  Does not allocate or synchronise.
 * nms_batched: `sets` independent sets of at most k <= 256 boxes, each sorted by descending score ([sets][k][4], count[s]
 *   valid rows) -> keep uint8 [sets][k] (1 kept, 0 suppressed or beyond count). */
int rfi_op_anchor_match_batched(rfi_ctx* ctx, const float* anchors, int64_t n, int64_t anchor_stride, const int32_t* anchor_count,
                                const float* gt_boxes, int images, int gt_max, const int32_t* gt_count, float fg_iou, float bg_iou,
                                int allow_low_quality, float* best_ws, int8_t* labels, int32_t* matched, float* targets);
int rfi_op_nms_batched(rfi_ctx* ctx, const float* boxes_sorted, const int32_t* count, int sets, int k, float iou_threshold, uint8_t* keep);
int rfi_op_rpn_loss(rfi_ctx* ctx, const float* head, int64_t pixels, int anchors_per_pixel, const int8_t* labels,
                    const float* targets, const int32_t* num_sampled_dev, float beta, float* dhead, void* workspace,
                    float* loss2_dev);
size_t rfi_op_rpn_loss_ws_bytes(void);
/* ---- The detector's box bookkeeping on the device (csrc/detect_sample.hip): the work rfi_toolbox_amd.models.MaskRCNN did in
 * NumPy between the GPU stages (the reference has no detector, so no reference interface is replaced: SURVEY 8a A11).  All
 * pointers are device pointers unless named *_host; nothing here synchronises or allocates.
 * segsort_u64: n_segs segments of `stride` (a power of two, 2 .. 65536) 64-bit keys, each sorted ascending in place (up to
 *   8192 keys: one launch sorting in LDS; longer segments: a multi-pass bitonic sort through global memory).
 * sample_keys: labels [images][n] (1 positive, 0 negative) -> keys [images][stride] = class << 48 | r << 16 | i with
 *   r = Philox4x32-10(counter (i, image, stream0 + class, step), key seed).x; rows >= count[image] (null: n) get ~0.
 * rpn_sample_apply: from the SORTED keys, `batch` anchors per image (at most max_pos positive, smallest keys first) keep their
 *   label, other labels >= 0 become -1; labels / targets are written level by level (level l holds anchors
 *   [level_off[l], level_off[l + 1]) of every image: [images][count_l] and [..][4]); *n_sampled += anchors sampled.
 * topk_keys / topk_decode: keys of the objectness logits of head [images][pixels][5 A] (descending, ties by anchor index);
 *   from the sorted keys the k best are decoded against `anchors`, clipped, boxes under min_size moved behind the rest
 *   (score -inf) -> slot `level` of boxes [images][levels][k][4], scores [images][levels][k], counts [images][levels].
 * proposals_select: per image the post_nms best kept candidates (descending score, ties level-major) followed by its
 *   ground-truth boxes -> props [images][pmax][4], pcount [images].
 * roi_sample: `batch` proposals per image, at most max_pos with matcher label 1 -> sel [images][batch] (positives first, -1
 *   padding), nsel / npos [images].  roi_compact: the batch's RoIs, image-major and compact: rois [R][5], class labels
 *   (gt_labels [images][gt_max] of the matched instance; 0 background), targets, matched instance (-1), pyramid level
 *   0 + [area >= t1] + [area >= t2] + [area >= t3], img_start [images + 1]; the foreground rows again (rois_fg, rois_gt with
 *   the global instance index gt_base[image] + matched as column 0, level_fg, fg_start); counts = (R, Rf).
 * roi_align_ml / _backward: RoIAlign where RoI r uses map level[r] of four ([n][h0 >> k][w0 >> k][c], scale scale0 / 2^k; host
 *   arrays of device pointers); the row count is read from count_dev, max_rois sizes the launch; backward ADDS into dmaps.
 * readback_begin / _end: a copy of <= 2048 bytes to the host that waits for the work enqueued BEFORE begin only. */
/* ---- per-patch order statistics on their own (csrc/order_stats.hip; rfi_preprocess_real and rfi_mad_flags build on them), for
 *      the kernel-level parity tests.  v: n patches of `per` float64 values; device pointers throughout.
 *      median[i] = the median (mean of the two middle values for an even count) of patch i's participating values: every
 *      value that is not NaN (np.nanmedian) or, with finite_only, not NaN and not +-inf; absdev != 0: of |v - centre[i]|
 *      instead.  NaN when nothing participates.  count (may be NULL): how many values took part.  f32 != 0: the doubles hold
 *      float32 values and every arithmetic result is rounded to float32 (NumPy's float32 arithmetic on a float32 array). */
int rfi_op_patch_median(rfi_ctx* ctx, const double* v, int n, int per, int absdev, const double* centre, int finite_only, int f32,
                        double* median, int32_t* count);
int rfi_op_segsort_u64(rfi_ctx* ctx, uint64_t* keys, int n_segs, int stride);
int rfi_op_sample_keys(rfi_ctx* ctx, const int8_t* labels, int images, int n, const int32_t* count, uint64_t seed, uint32_t step,
                       uint32_t stream0, uint64_t* keys, int stride);
int rfi_op_rpn_sample_apply(rfi_ctx* ctx, const uint64_t* keys_sorted, int images, int n, int stride, int batch, int max_pos,
                            const int8_t* labels, const float* targets, int levels, const int32_t* level_off_host,
                            int8_t* const* level_labels_host, float* const* level_targets_host, int32_t* n_sampled);
int rfi_op_topk_keys(rfi_ctx* ctx, const float* head, int images, int pixels, int anchors_per_pixel, uint64_t* keys, int stride);
int rfi_op_topk_decode(rfi_ctx* ctx, const uint64_t* keys_sorted, int images, int stride, int pixels, int anchors_per_pixel, int k,
                       const float* head, const float* anchors, float clip_h, float clip_w, float min_size, float* boxes, float* scores,
                       int32_t* counts, int levels, int level);
int rfi_op_proposals_select(rfi_ctx* ctx, const float* boxes, const float* scores, const uint8_t* keep, int images, int levels, int k,
                            int post_nms, const float* gt_boxes, int gt_max, const int32_t* gt_count, int pmax, float* props,
                            int32_t* pcount);
int rfi_op_roi_sample(rfi_ctx* ctx, const int8_t* labels, const int32_t* pcount, int images, int pmax, int batch, int max_pos,
                      uint64_t seed, uint32_t step, uint32_t stream0, int32_t* sel, int32_t* nsel, int32_t* npos);
int rfi_op_roi_compact(rfi_ctx* ctx, const int32_t* sel, const int32_t* nsel, const int32_t* npos, int images, int batch, int pmax,
                       const float* props, const int32_t* matched, const float* targets, const int32_t* gt_labels, int gt_max,
                       const int32_t* gt_base, float t1, float t2, float t3, float* rois, int32_t* cls, float* tgt, int32_t* gt,
                       int32_t* level, int32_t* img_start, float* rois_fg, float* rois_gt, int32_t* level_fg, int32_t* fg_start,
                       int32_t* counts);
int rfi_op_roi_align_ml(rfi_ctx* ctx, const float* const* maps_host, int n, int h0, int w0, int c, float scale0, const float* rois,
                        const int32_t* level, const int32_t* count_dev, int max_rois, int ph, int pw, int sampling_ratio, float* out);
int rfi_op_roi_align_ml_backward(rfi_ctx* ctx, float* const* dmaps_host, int n, int h0, int w0, int c, float scale0, const float* dout,
                                 const float* rois, const int32_t* level, const int32_t* img_start, int max_rois, int ph, int pw,
                                 int sampling_ratio);
/* ---- Detector inference on the device (csrc/detect_infer.hip): what rfi_toolbox_amd.models.MaskRCNN.predict does in NumPy
 * behind the box head and the mask head; MaskRCNN.detect chains these with the entry points above.  All pointers are device
 * pointers; nothing here synchronises or allocates.  Box tensors are 16-byte aligned.
 * detect_candidates: head [images pmax][5 k1] (k1 class logits, then k1 x 4 deltas; row b pmax + r = proposal r of image b),
 *   props [images][pmax][4] with pcount[b] valid rows, pmax <= 256.  Per image and foreground class c = 1 .. k1 - 1:
 *   prob = softmax(logits)[c] in float32, class c's deltas decoded against the proposal (weights 1, dw / dh <= log(1000/16))
 *   and clipped to [0, clip_w] x [0, clip_h]; rows with prob > score_thresh and both sides >= min_size, sorted by descending
 *   prob (ties: ascending proposal index) -> set b (k1 - 1) + c - 1 of boxes [sets][pmax][4], scores [sets][pmax] (-inf behind
 *   the count), counts [sets]: the input form of rfi_op_nms_batched.
 * detect_select: from the candidate sets ([images][classes][k], classes <= 32 sets of k <= 256) and the NMS keep bytes, per
 *   image the max_det best kept boxes (descending score, ties class-major, then by position in the class's set) ->
 *   det_boxes [images][max_det][4] (zero padded), det_scores, det_labels (int32, 1-based class; 0 padding), det_count
 *   [images], and the mask branch's RoI list rois [images max_det][5] (image, x1, y1, x2, y2; padding rows: a zero box of their
 *   own image) with level = [area >= t1] + [area >= t2] + [area >= t3].
 * rois_from_boxes: props [images][pmax][4] + pcount -> rois [images pmax][5] + level at a fixed stride of pmax rows per image
 *   (rows beyond pcount[b]: a zero box of image b, whatever props holds there).
 * mask_paste: logits [images max_det][28][28] -> p = sigmoid, bilinear sample at (px + 0.5 - x1) / max(x2 - x1, 1e-6) * 28 - 0.5
 *   (indices clamped to [0, 27], fractions to [0, 1]) for the pixels of [max(floor(x1), 0), min(ceil(x2), w)) x [.. y ..),
 *   mask = v > 0.5, 0 elsewhere and for slots >= det_count[b]; rfi_mask [images][h][w] = OR over the image's instances;
 *   masks [images][max_det][h][w] is written unless null.  max_det <= 256, w % 4 == 0, masks 4-byte aligned. */
int rfi_op_detect_candidates(rfi_ctx* ctx, const float* head, const float* props, const int32_t* pcount, int images, int pmax, int k1,
                             float clip_h, float clip_w, float score_thresh, float min_size, float* boxes, float* scores,
                             int32_t* counts);
int rfi_op_detect_select(rfi_ctx* ctx, const float* boxes, const float* scores, const uint8_t* keep, int images, int classes, int k,
                         int max_det, float t1, float t2, float t3, float* det_boxes, float* det_scores, int32_t* det_labels,
                         int32_t* det_count, float* rois, int32_t* level);
int rfi_op_rois_from_boxes(rfi_ctx* ctx, const float* props, const int32_t* pcount, int images, int pmax, float t1, float t2, float t3,
                           float* rois, int32_t* level);
int rfi_op_mask_paste(rfi_ctx* ctx, const float* logits, const float* det_boxes, const int32_t* det_count, int images, int max_det, int h,
                      int w, uint8_t* rfi_mask, uint8_t* masks);
/* ---- elementwise kernels of the bfloat16 data flow (ResNet-style encoder, BatchNorm backward), for the kernel-level parity
 *      tests.  bfloat16 tensors are dense [m][c] arrays of uint16 bit patterns, c % 8 == 0, 16-byte aligned.  No counterpart
 *      in the reference (its tensors are float32): these are the builder's reduced-precision storage forms of
 *      relu(BN(y) + shortcut) (torchvision-style BasicBlock tail), of the masked sum of gradient terms at a block output,
 *      and of nn.BatchNorm2d's training-mode backward in front of a (Leaky)ReLU with slope `slope` (1: no activation).
 *      bn_backward16: dgamma / dbeta / dbias (dbias may be null) are float32 [c]; dy is bfloat16. ---- */
int rfi_op_bn_add_relu16(rfi_ctx* ctx, const uint16_t* y, const float* scale, const float* shift, const uint16_t* s, const float* s_scale,
                         const float* s_shift, int64_t m, int c, uint16_t* out);
int rfi_op_relu_mask_sum16(rfi_ctx* ctx, const uint16_t* g0, const uint16_t* g1, const float* g2_f32, const uint16_t* g2_bf16,
                           int64_t g2_stride, const uint16_t* a, int64_t m, int c, uint16_t* dz);
int rfi_op_bn_backward16(rfi_ctx* ctx, const uint16_t* da, const uint16_t* y, int64_t m, int c, const float* gamma, const float* scale,
                         const float* shift, const float* mean, const float* invstd, float slope, uint16_t* dy, float* dgamma,
                         float* dbeta, float* dbias);
int rfi_readback_begin(rfi_ctx* ctx, const void* src_dev, size_t bytes);
int rfi_readback_end(rfi_ctx* ctx, void* dst_host, size_t bytes);
int rfi_op_fpn_merge(rfi_ctx* ctx, const float* lateral, const float* top, int n, int h, int w, int c, float* out);
int rfi_op_fpn_merge_backward(rfi_ctx* ctx, const float* dout, int n, int h, int w, int c, float* dtop);
int rfi_op_bn_stats(rfi_ctx* ctx, const float* y, int64_t m, int c, float* mean, float* var_biased);
/* a = relu(y*scale+shift): skip (n,h,w,c) and 2x2 max-pooled (n,h/2,w/2,c) */
int rfi_op_bn_relu_pool(rfi_ctx* ctx, const float* y, int n, int h, int w, int c, const float* scale,
                        const float* shift, float* skip, float* pooled);
/* da = dskip + max-pool routing of dpool (first maximum in row-major window order wins) */
int rfi_op_pool_bwd_merge(rfi_ctx* ctx, const float* y, int n, int h, int w, int c, const float* scale,
                          const float* shift, const float* dskip, const float* dpool, float* da);
/* train-mode BatchNorm+ReLU backward of y (m,c) with affine gamma/beta: da (grad w.r.t. the
 * activated output) is overwritten with dy; dgamma, dbeta, dbias(=sum dy) are written */
int rfi_op_bn_relu_backward(rfi_ctx* ctx, const float* y, int64_t m, int c, const float* gamma,
                            const float* beta, float* da_inout, float* dgamma, float* dbeta, float* dbias);

#ifdef __cplusplus
}
#endif
#endif /* RFI_HIP_H */
