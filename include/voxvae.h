/* voxvae.h -- C ABI of libvoxvae.so: the MI355X (gfx950) voxel VAE reconstruction hot path.
 *
 * The reference (bogus2000/anytime-3D-reconstruction) has NO FFI / plugin / operator interface: it is
 * Python on TensorFlow and its seam is the Python API of src/net_core + src/module.  The
 * drop-in for that seam is the Python package in anytime-3d-reconstruction_amd/src/ (same module paths, names,
 * signatures).  This header is the boundary UNDER that package: what a maintainer of the reference would bind
 * (ctypes stub in INTEGRATION.md) to replace the TensorFlow ops each function cites.  Citations are
 * /root/reference paths.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; tensors are dense, channels-last
 *     (NDHWC), cubic grids with a power-of-two side; `stream` is a hipStream_t passed as void*.
 *   - activations/weights are VV_F32 or VV_BF16 (`dtype`); statistics, losses, logits, probabilities, latents
 *     are always float32.
 *   - functions return 0 (VV_OK) or a negative vv_status; they never throw, never allocate, never
 *     synchronise; scratch comes from the caller (`*_workspace_bytes`).  No global state: thread-safe per stream.
 *   - memory discipline: an entry reads and writes only inside the tensors it was given.  A workspace is write-before-read
 *     (whatever it held before the call does not matter; vv_convT3d_final_bce_metrics_fwd is a complete forward too,
 *     alone or behind vv_convT3d_final_bce_fwd on the same workspace); an entry touches no more than its
 *     `*_workspace_bytes` query says, and a `workspace_bytes` argument beyond that minimum changes nothing (one
 *     workspace may serve every layer of a stream).
 */
#ifndef VOXVAE_H
#define VOXVAE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { VV_F32 = 0, VV_BF16 = 1, VV_FP8 = 2 /* OCP e4m3fn, 1 byte; MFMA layers with cin % 128 == 0 only */ } vv_dtype;
typedef enum { VV_ACT_NONE = 0, VV_ACT_ELU = 1, VV_ACT_RELU = 2, VV_ACT_LRELU = 3 } vv_act;
/* How an entry with a `schedule` argument cuts its work (the *_ex entries of the 4^3 <-> 2^3 layers).  The results are the same bits
 * either way.  VV_SCHED_LATENCY: for one batch at a time -- every launch is cut fine enough to fill the device on its own.
 * VV_SCHED_THROUGHPUT: for a caller that keeps several independent batches in flight on different streams -- fewer, longer
 * workgroups, so that a launch costs the device less in total while another batch's workgroups fill the rest of it. */
typedef enum { VV_SCHED_LATENCY = 0, VV_SCHED_THROUGHPUT = 1 } vv_schedule;
typedef enum {
    VV_OK = 0,
    VV_ERR_NULL = -1,       /* required pointer is NULL */
    VV_ERR_SHAPE = -2,      /* unsupported / inconsistent shape */
    VV_ERR_DTYPE = -3,
    VV_ERR_ALIGN = -4,      /* pointer not 16-byte aligned */
    VV_ERR_WORKSPACE = -5,  /* workspace too small */
    VV_ERR_LAUNCH = -6      /* hipGetLastError() != hipSuccess after launch */
} vv_status;

int vv_abi_version(void);
const char *vv_status_string(int status);
/* hipGetErrorString of the HIP error behind this thread's most recent VV_ERR_LAUNCH. */
const char *vv_last_hip_error(void);

/* ---------------------------------------------------------------------------------------------------------
 * Weight packing: Keras variable layouts -> the K-contiguous [N][K] panels the MFMA kernels stream.
 * One-off per weight update; device to device. */

/* Conv3D kernel [4,4,4,Cin,Cout] (autoencoder3D.py:27) -> packed [Cout][64*Cin], k = tap*Cin + ci. */
int vv_pack_conv_k4(const float *w_keras, void *packed, int cin, int cout, int dtype, void *stream);
/* Conv3DTranspose kernel [4,4,4,Cout,Cin] (autoencoder3D.py:42) stride 2 -> 8 output-parity panels
 * packed [8][Cout][8*Cin]; parity p = (pd,ph,pw), k = (ad,ah,aw)*Cin + ci, tap t = 1 - p + 2a per axis. */
int vv_pack_convT_k4s2(const float *w_keras, void *packed, int cin, int cout, int dtype, void *stream);
/* Final encoder Conv3D k4 s1 SAME (pad 1/2) followed by the spatial mean (autoencoder3D.py:86-91) is linear in
 * its input: packed [Cout][S^3*Cin] with W_eff[i] = (1/S^3) * sum_o w[i - o + 1]  (S = input side). */
int vv_pack_conv_k4s1_meanpool(const float *w_keras, void *packed, int side, int cin, int cout, int dtype, void *stream);
/* The same final encoder conv position by position, for final_pool = 'max' (autoencoder3D.py:92-93: tf.reduce_max is not linear):
 * packed [S^3*Cout][S^3*Cin], row (o, co), column (i, ci) = w[i - o + 1][ci][co] (0 outside the 4 taps); a vv_dense_fwd with this
 * panel gives the conv output [B][S^3][Cout], vv_max_over_positions the pooled [B][Cout]. */
int vv_pack_conv_k4s1_full(const float *w_keras, void *packed, int side, int cin, int cout, int dtype, void *stream);
int vv_max_over_positions(const float *x, float *out, int batch, int npos, int channels, void *stream);
/* y = sigmoid(x), float32, n elements (in place allowed): encoder3D's final_activation 'sigmoid' (autoencoder3D.py:97-99). */
int vv_sigmoid_f32(const float *x, float *y, long n, void *stream);
/* First decoder Conv3DTranspose k4 s1 SAME on the S^3 x Cin seed (autoencoder3D.py:127-128, first loop
 * iteration) as one dense panel: packed [S^3*Cout][S^3*Cin], row (o,co), col (j,ci) = w[o - j + 1][co][ci]. */
int vv_pack_convT_k4s1_dense(const float *w_keras, void *packed, int side, int cin, int cout, int dtype, void *stream);
/* Dense kernel [In,Out] (autoencoder3D.py:59) -> packed [Out][In]. */
int vv_pack_dense(const float *w_keras, void *packed, int in, int out, int dtype, void *stream);
/* BatchNormalization(training=False) folded to y = x*scale + shift (autoencoder3D.py:31,46,62):
 * scale = gamma/sqrt(var+eps); shift = beta + (bias - mean)*scale.  bias may be NULL.  `repeat` tiles the C
 * channel vector (used when a spatial layer is run as one dense panel). */
int vv_fold_bn(const float *gamma, const float *beta, const float *mean, const float *var, const float *bias,
               float eps, float *scale, float *shift, int channels, int repeat, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Layers (inference form: conv -> folded BN -> activation).  scale/shift may be NULL (identity). */

/* conv3DEnc with Cin = 1: Conv3D k4 s2 SAME on the occupancy grid + BN + act (autoencoder3D.py:26-39, first
 * loop iteration :84-85) on the same MFMA tile engine, K = the 64 taps gathered from x.  x [B,D,D,D,1] float32;
 * w_packed = vv_pack_conv_k4(cin = 1) = [Cout][64]; y [B,D/2,D/2,D/2,Cout] dtype. */
int vv_conv3d_first_fwd(const float *x, const void *w_packed, const float *scale, const float *shift, void *y,
                        int batch, int side, int cout, int act, int dtype, void *stream);
/* Same with a separate output element type: out_dtype VV_FP8 (e4m3fn) is available for dtype VV_BF16, Cout 64, side >= 32
 * (the hand-over into an fp8 second layer); otherwise out_dtype must equal dtype. */
int vv_conv3d_first_fwd_io(const float *x, const void *w_packed, const float *scale, const float *shift, void *y,
                           int batch, int side, int cout, int act, int dtype, int out_dtype, void *stream);

/* conv3DEnc, Cin % 64 == 0: Conv3D k4 s2 SAME + BN + act as an implicit GEMM on MFMA
 * (autoencoder3D.py:26-39).  x [B,D,D,D,Cin]; w = vv_pack_conv_k4; y [B,D/2,...,Cout]. */
size_t vv_conv3d_k4s2_workspace_bytes(int batch, int side, int cin, int cout, int dtype);
int vv_conv3d_k4s2_fwd(const void *x, const void *w_packed, const float *scale, const float *shift, void *y,
                       int batch, int side, int cin, int cout, int act, int dtype, void *workspace,
                       size_t workspace_bytes, void *stream);

/* conv3DDec stride 2: Conv3DTranspose k4 s2 SAME + BN + act as 8 output-parity implicit GEMMs
 * (autoencoder3D.py:41-54).  x [B,D,D,D,Cin]; w = vv_pack_convT_k4s2; y [B,2D,2D,2D,Cout]. */
size_t vv_convT3d_k4s2_workspace_bytes(int batch, int side, int cin, int cout, int dtype);
int vv_convT3d_k4s2_fwd(const void *x, const void *w_packed, const float *scale, const float *shift, void *y,
                        int batch, int side, int cin, int cout, int act, int dtype, void *workspace,
                        size_t workspace_bytes, void *stream);

/* The two stride-2 layers with separate operand / output element types: dtype VV_FP8 runs the implicit GEMM on
 * v_mfma_f32_32x32x16_fp8_fp8 (x and w_packed in OCP e4m3fn, one byte per element; cin % 128 == 0; per-output-channel
 * weight scales belong in `scale`), out_dtype chooses what the epilogue stores (VV_FP8 for the next fp8 layer, VV_BF16
 * for a bf16 consumer, VV_F32).  dtype VV_BF16 with out_dtype VV_FP8 is the hand-over into an fp8 stretch.  New in this
 * build (BASELINE config 5): the reference is float32 only.  Workspace: the *_workspace_bytes query with `dtype`. */
int vv_conv3d_k4s2_fwd_io(const void *x, const void *w_packed, const float *scale, const float *shift, void *y,
                          int batch, int side, int cin, int cout, int act, int dtype, int out_dtype, void *workspace,
                          size_t workspace_bytes, void *stream);
int vv_convT3d_k4s2_fwd_io(const void *x, const void *w_packed, const float *scale, const float *shift, void *y,
                           int batch, int side, int cin, int cout, int act, int dtype, int out_dtype, void *workspace,
                           size_t workspace_bytes, void *stream);

/* Direct variant of vv_conv3d_k4s2_fwd for the widest encoder layer (bf16, Cin 64 -> Cout 128, side >= 16): per input
 * phase q (x index parity per axis) the layer is a k2 s1 convolution over the phase sub-grid, so a 4x8x8 box of
 * outputs stages 8 phase tiles of 5x9x9 voxels in LDS instead of 64 im2col tiles; same vv_pack_conv_k4 weights.
 * vv_conv3d_k4s2_direct_supported() says whether a shape is covered (callers fall back to vv_conv3d_k4s2_fwd). */
int vv_conv3d_k4s2_direct_supported(int side, int cin, int cout, int dtype);
int vv_conv3d_k4s2_direct_fwd(const void *x, const void *w_packed, const float *scale, const float *shift, void *y,
                              int batch, int side, int cin, int cout, int act, int dtype, void *stream);
/* Same with the output stored as VV_BF16 or VV_FP8 (e4m3fn: the hand-over to an fp8 layer without a conversion pass). */
int vv_conv3d_k4s2_direct_fwd_io(const void *x, const void *w_packed, const float *scale, const float *shift, void *y,
                                 int batch, int side, int cin, int cout, int act, int dtype, int out_dtype, void *stream);
/* fp8 twin of the direct 64 -> 128 layer (conv_direct_fp8.hip): x and w_packed (vv_pack_conv_k4 with dtype VV_FP8, from a
 * kernel already divided by its per-output-channel scale; the scale belongs in `scale`) in OCP e4m3fn, block-scaled K = 64
 * MFMA, y stored as VV_FP8 or VV_BF16.  Input side >= 16. */
int vv_conv3d_k4s2_direct_fp8_supported(int side, int cin, int cout);
int vv_conv3d_k4s2_direct_fp8_fwd(const void *x, const void *w_packed, const float *scale, const float *shift, void *y,
                                  int batch, int side, int cin, int cout, int act, int out_dtype, void *stream);

/* Direct variant of vv_convT3d_k4s2_fwd for the widest decoder layer (bf16, Cin 128 -> Cout 64, side >= 8): the input
 * halo tile of a 4x4x8 block of cells is staged in LDS once and serves all 8 parities x 8 taps; weights come from the
 * MFMA-fragment-ordered panel of vv_pack_convT_k4s2_frag ([8 parity][8 tap][Cin/16][Cout/32][64 lanes][8]).
 * vv_convT3d_k4s2_direct_supported() says whether a shape is covered (callers fall back to vv_convT3d_k4s2_fwd). */
int vv_convT3d_k4s2_direct_supported(int side, int cin, int cout, int dtype);
int vv_pack_convT_k4s2_frag(const float *w_keras, void *packed, int cin, int cout, void *stream);
int vv_convT3d_k4s2_direct_fwd(const void *x, const void *w_frag, const float *scale, const float *shift, void *y,
                               int batch, int side, int cin, int cout, int act, int dtype, void *stream);
/* fp8 twin of the direct transposed layer (convt_direct_fp8.hip): x and w_frag in OCP e4m3fn (w_frag from
 * vv_pack_convT_k4s2_frag_fp8, which converts a float32 Keras kernel already divided by its per-output-channel scale; the
 * scale belongs in `scale`), block-scaled K = 64 MFMA, y stored as VV_BF16 or VV_FP8 (out_dtype; VV_FP8 feeds the fp8 form of
 * vv_convT3d_final_bce_fwd).  Cin 128 -> Cout 64, side >= 8. */
int vv_convT3d_k4s2_direct_fp8_supported(int side, int cin, int cout);
int vv_pack_convT_k4s2_frag_fp8(const float *w_keras, void *packed, int cin, int cout, void *stream);
int vv_convT3d_k4s2_direct_fp8_fwd(const void *x, const void *w_frag, const float *scale, const float *shift, void *y,
                                   int batch, int side, int cin, int cout, int act, int out_dtype, void *stream);

/* conv3DEnc / conv3DDec between the 8^3 and the 4^3 grid (autoencoder3D.py:26-54; the 32^3 model's 128 -> 256 and
 * 256 -> 128 layers, the 64^3 model's 256 -> 512 and 512 -> 256) with four whole samples resident in LDS per workgroup
 * and the taps that fall into the SAME padding skipped at MFMA-tile granularity in d and h (bf16 only).
 *   conv : x [B,8,8,8,Cin] -> y [B,4,4,4,Cout], Cin % 64 == 0, Cout % 64 == 0; w_skip = vv_pack_conv_k4_skip
 *          = [64 taps][Cin/64][Cout][64]
 *   convT: x [B,4,4,4,Cin] -> y [B,8,8,8,Cout], Cin % 64 == 0, Cout % 128 == 0; w_skip = vv_pack_convT_k4s2_skip
 *          = [8 parities][8 taps][Cin/64][Cout][64], tap t = 1 - p + 2a per axis
 * No workspace; batches whose input passes 2 GiB go out as several launches. */
int vv_conv3d_k4s2_skip_supported(int side, int cin, int cout, int dtype);
int vv_convT3d_k4s2_skip_supported(int side, int cin, int cout, int dtype);
int vv_pack_conv_k4_skip(const float *w_keras, void *packed, int cin, int cout, void *stream);
/* Several of the two images above in one call (round 4: the training step needs nine per step and each single call is a 5-8 us launch):
 * kinds[j] = 0: vv_pack_conv_k4_skip, 1: vv_pack_convT_k4s2_skip of (w_keras[j], cin[j], cout[j]) into packed[j]; one launch per kind (and per
 * eight jobs); bit-identical to the single calls.  The arrays are HOST arrays of njobs entries. */
int vv_pack_skip_images(const int *kinds, const float *const *w_keras, void *const *packed, const int *cin, const int *cout, int njobs,
                        void *stream);
int vv_pack_convT_k4s2_skip(const float *w_keras, void *packed, int cin, int cout, void *stream);
int vv_conv3d_k4s2_skip_fwd(const void *x, const void *w_skip, const float *scale, const float *shift, void *y, int batch,
                            int side, int cin, int cout, int act, int dtype, void *stream);
int vv_convT3d_k4s2_skip_fwd(const void *x, const void *w_skip, const float *scale, const float *shift, void *y, int batch,
                             int side, int cin, int cout, int act, int dtype, void *stream);

/* conv3DDec 8^3 x 128 -> 16^3 x 64 (autoencoder3D.py:41-54; the 32^3 model's widest decoder layer) with one WHOLE sample
 * resident in LDS per workgroup (128 KiB, no halo: out-of-grid taps read a zero row), all eight waves on the same output
 * parity sharing each weight chunk through an LDS ring (bf16 only).  w_skip = vv_pack_convT_k4s2_skip's image.  One
 * workgroup per (sample, parity split); the 8 parities are split over 2 / 4 / 8 workgroups until the grid holds two rounds
 * of workgroups per CU (VV_CTW_PS overrides; VV_CTW_SHAPE=32 selects the 32x32x16 MFMA form, default 16x16x32).  Replaces vv_convT3d_k4s2_direct_fwd at this shape; no workspace. */
int vv_convT3d_k4s2_whole_supported(int side, int cin, int cout, int dtype);
int vv_convT3d_k4s2_whole_fwd(const void *x, const void *w_skip, const float *scale, const float *shift, void *y, int batch,
                              int side, int cin, int cout, int act, int dtype, void *stream);

/* conv3DEnc / conv3DDec between the 4^3 and the 2^3 grid (the 32^3 model's 256 -> 512 and 512 -> 256 layers) as a
 * position-major split-K GEMM: rows = the batch at one output position, K = that position's valid (tap, 64-channel chunk)
 * pairs cut into equal shares over the workgroups, 256 x 128 tiles, 3-stage LDS-DMA ring (bf16 only).  Weights in the
 * vv_pack_conv_k4_skip / vv_pack_convT_k4s2_skip layouts.  Workspace = float32 slabs of the positions that are cut into
 * several shares (summed in share order: deterministic).
 *   conv : x [B,4,4,4,Cin] -> y [B,2,2,2,Cout];  convT: x [B,2,2,2,Cin] -> y [B,4,4,4,Cout];  Cin % 64 == 0, Cout % 8 == 0 */
int vv_conv3d_k4s2_pos_supported(int side, int cin, int cout, int dtype);
int vv_convT3d_k4s2_pos_supported(int side, int cin, int cout, int dtype);
size_t vv_conv3d_k4s2_pos_workspace_bytes(int batch, int cin, int cout);
size_t vv_convT3d_k4s2_pos_workspace_bytes(int batch, int cin, int cout);
int vv_conv3d_k4s2_pos_fwd(const void *x, const void *w_skip, const float *scale, const float *shift, void *y, int batch,
                           int side, int cin, int cout, int act, int dtype, void *workspace, size_t workspace_bytes, void *stream);
int vv_convT3d_k4s2_pos_fwd(const void *x, const void *w_skip, const float *scale, const float *shift, void *y, int batch,
                            int side, int cin, int cout, int act, int dtype, void *workspace, size_t workspace_bytes, void *stream);
/* The same with a `schedule` (vv_schedule; anything else: VV_ERR_SHAPE); the entries above are VV_SCHED_LATENCY.  bf16 is the only
 * element type of this form, so these take none.  VV_SCHED_THROUGHPUT: one workgroup walks ALL K shares of its output position and
 * adds them up in registers, in the share order and with the float32 sums of the split form -- every output byte is the same; no
 * slabs are written and no second launch sums them.  The workspace query and check are those of the split form for either schedule
 * (the folded form does not touch the workspace). */
int vv_conv3d_k4s2_pos_fwd_ex(const void *x, const void *w_skip, const float *scale, const float *shift, void *y, int batch,
                              int side, int cin, int cout, int act, int schedule, void *workspace, size_t workspace_bytes,
                              void *hip_stream);
int vv_convT3d_k4s2_pos_fwd_ex(const void *x, const void *w_skip, const float *scale, const float *shift, void *y, int batch,
                               int side, int cin, int cout, int act, int schedule, void *workspace, size_t workspace_bytes,
                               void *hip_stream);

/* y[M,N] = act((x[M,K] @ w_packed[N,K]^T) * scale[N] + shift[N]): linearTransform (autoencoder3D.py:56-70) and
 * the two layers packed as dense panels above.  K % 8 == 0 (bf16) / % 4 (f32), N % 4 == 0 (tails are masked).
 * out_dtype may differ from dtype (the encoder output is float32). */
size_t vv_dense_workspace_bytes(int m, int n, int k, int dtype);
int vv_dense_fwd(const void *x, const void *w_packed, const float *scale, const float *shift, void *y, int m, int n,
                 int k, int act, int dtype, int out_dtype, void *workspace, size_t workspace_bytes, void *stream);

/* The latent tail of the evaluation path in two launches (latent_tail.hip): encoder tail (the vv_pack_conv_k4s1_meanpool
 * panel w5 [E][K5] applied to the last stride-2 activation h [B][K5]) -> slice | clip | sampling | KL (as vv_reparam_kl_fwd,
 * no dropout) -> linearTransform + BN + act (wd [lin][L], vv_pack_dense) -> first decoder layer as a dense panel
 * (w1 [n1][lin], vv_pack_convT_k4s1_dense) + BN + act.  Outputs: enc_out [B][E] (optional), z [B][L], z_act bf16 (optional),
 * kl [B] (variational), h1 [B][n1] bf16 = the input of the first stride-2 decoder layer.  variational: E = 2L, else E = L and
 * z = enc_out.  bf16 only; L % 32 == 0, lin % 32 == 0, n1 % 16 == 0.  e5_scale: optional per-channel factor on enc_out. */
int vv_latent_tail_supported(int K5, int E, int L, int lin, int n1, int variational, int dtype);
size_t vv_latent_tail_workspace_bytes(int batch, int K5, int E, int n1);
int vv_latent_tail_fwd(const void *h, const void *w5, const float *e5_scale, const float *eps, const void *wd, const float *scale_d,
                       const float *shift_d, const void *w1, const float *scale_1, const float *shift_1, float *enc_out, float *z,
                       void *z_act, float *kl, void *h1, int batch, int K5, int E, int L, int lin, int n1, int variational, int act,
                       int dtype, void *workspace, size_t workspace_bytes, void *stream);

/* The last stride-2 encoder layer (conv3DEnc at 4^3 -> 2^3, autoencoder3D.py:26-39 / :84-85) AND the latent tail above in three
 * launches (posgemm.hip + latent_tail.hip): the convolution leaves only its float32 split-K partial sums, and the encoder-tail
 * kernel sums them in share order, applies that layer's folded BN (scale4 / shift4, may be NULL) + act and rounds to bf16 while it
 * builds its own operand -- the same values, in the same order, as vv_conv3d_k4s2_pos_fwd followed by vv_latent_tail_fwd, without the
 * reduce launch and without the [B][2^3][cout4] activation in memory.  x4 [B][4^3][cin4] bf16, w4_skip = vv_pack_conv_k4_skip's
 * image; K5 = 8 * cout4; the other arguments as vv_latent_tail_fwd.  cout4 % 256 == 0, E % 16 == 0, E <= 128. */
int vv_conv_pos_latent_tail_supported(int cin4, int cout4, int E, int L, int lin, int n1, int variational, int dtype);
size_t vv_conv_pos_latent_tail_workspace_bytes(int batch, int cin4, int cout4, int E);
int vv_conv_pos_latent_tail_fwd(const void *x4, const void *w4_skip, const float *scale4, const float *shift4, int cin4, int cout4,
                                const void *w5, const float *e5_scale, const float *eps, const void *wd, const float *scale_d,
                                const float *shift_d, const void *w1, const float *scale_1, const float *shift_1, float *enc_out,
                                float *z, void *z_act, float *kl, void *h1, int batch, int E, int L, int lin, int n1, int variational,
                                int act, int dtype, void *workspace, size_t workspace_bytes, void *stream);
/* The same with a `schedule` (vv_schedule, as vv_conv3d_k4s2_pos_fwd_ex: bf16 only, no element type; the entry above is
 * VV_SCHED_LATENCY).  VV_SCHED_THROUGHPUT: the convolution leaves ONE float32 slab per output position, its shares already summed in
 * share order; every output byte is the same.  The workspace query serves either schedule. */
int vv_conv_pos_latent_tail_fwd_ex(const void *x4, const void *w4_skip, const float *scale4, const float *shift4, int cin4, int cout4,
                                   const void *w5, const float *e5_scale, const float *eps, const void *wd, const float *scale_d,
                                   const float *shift_d, const void *w1, const float *scale_1, const float *shift_1, float *enc_out,
                                   float *z, void *z_act, float *kl, void *h1, int batch, int E, int L, int lin, int n1, int variational,
                                   int act, int schedule, void *workspace, size_t workspace_bytes, void *hip_stream);

/* ---------------------------------------------------------------------------------------------------------
 * Latent ops */

/* slice | clip(-10,10) | sampling | Dropout | kl_loss vs N(0,I), fused (nolbo.py:1417-1431, 1464-1470;
 * function.py:35-38, 84-98).  enc_out [B,2L]; eps [B,L] (the tf.random.normal draw, injected);
 * drop_mask [B,L] in {0,1} or NULL, drop_scale = 1/(1-rate); z [B,L] float32; z_act [B,L] = the same values in
 * the activation dtype `act_dtype` that feeds the decoder (may be NULL); kl [B] (may be NULL); mean/logvar [B,L]
 * outputs may be NULL. */
int vv_reparam_kl_fwd(const float *enc_out, const float *eps, const float *drop_mask, float drop_scale, float *z,
                      void *z_act, int act_dtype, float *kl, float *mean, float *logvar, int batch, int latent,
                      void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Decoder tail + losses, fused: Conv3DTranspose k4 s2 SAME -> 1 channel (logits), tf.sigmoid, binary_loss
 * (gamma, epsilon clip) and voxelPrecisionRecall at p >= 0.5 (autoencoder3D.py:129-136; function.py:73-82,
 * 100-115; nolbo.py:1496-1499).  x [B,D,D,D,Cin] dtype; w_keras [4,4,4,1,Cin] float32; target [B,2D,2D,2D]
 * float32; probs/logits [B,2D,2D,2D] float32 (either may be NULL); stats [B,4] = per-sample (bce,TP,FP,FN). */
/* dtype VV_FP8: x in OCP e4m3fn (side >= 8; the kernel quantises w_keras per tap itself); probabilities, logits and the sums
 * stay float32. */
size_t vv_convT3d_final_bce_workspace_bytes(int batch, int side);
int vv_convT3d_final_bce_fwd(const void *x, const float *w_keras, const float *target, float *probs, float *logits,
                             float *stats, int batch, int side, int cin, float gamma, float epsilon, int dtype,
                             void *workspace, size_t workspace_bytes, void *stream);
/* Same, plus the batch metrics of nolbo.py:1498-1501 in the same reduction launch: metrics4 = (mean bce, mean TP/(TP+FP+1e-10),
 * mean TP/(TP+FN+1e-10), mean IoU) -- what vv_shape_metrics computes from `stats`. */
int vv_convT3d_final_bce_metrics_fwd(const void *x, const float *w_keras, const float *target, float *probs, float *logits,
                                     float *stats, float *metrics4, int batch, int side, int cin, float gamma, float epsilon,
                                     int dtype, void *workspace, size_t workspace_bytes, void *stream);

/* Batch means of nolbo.py:1498-1501: out[0..3] = mean_b bce, mean_b TP/(TP+FP+1e-10), mean_b TP/(TP+FN+1e-10),
 * mean_b TP/max(TP+FP+FN,1) (IoU: not in the reference). */
int vv_shape_metrics(const float *stats, float *out4, int batch, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Sampled-mean reconstruction (final_mean.hip): the "anytime" inference of nolbo_test.py:167-180 -- K latents drawn from
 * an object's posterior, every one decoded, the occupancy PROBABILITIES averaged.
 * --------------------------------------------------------------------------------------------------------- */
/* The K draws of nolbo_test.py:169-173 (`sampling(mean, logVar)` K times; function.py:35-38) in one launch:
 * z[(b K + k), l] = mean[b,l] + sqrt(exp(logvar[b,l])) * eps[b,k,l].  mean/logvar [B,L], eps [B,K,L] (the injected
 * tf.random.normal draw), z float32 [B K, L] (may be NULL), z_act the same values in act_dtype (VV_F32 / VV_BF16; may be
 * NULL; both NULL: VV_ERR_NULL).  Nothing is clipped: the caller passes the log-variance its model class uses. */
int vv_sample_latents(const float *mean, const float *logvar, const float *eps, float *z, void *z_act, int act_dtype,
                      int objects, int samples, int latent, void *stream);
/* The last decoder layer over the K samples of each object with `tf.reduce_mean(decoder(latents), axis=0)`
 * (nolbo_test.py:174-177) inside the kernel: x [B K, side^3, 64] (VV_F32 / VV_BF16; sample k of object b is row b K + k),
 * w_keras [4,4,4,1,64]; mean_probs [B,(2 side)^3] float32 = (1/K) sum_k sigmoid(logit_k), summed in float32 in a fixed order
 * (autoencoder3D.py:129-136).  target [B,(2 side)^3] float32 or NULL; stats [B,4] = (bce, TP, FP, FN) of the AVERAGED
 * prediction (binary_loss with the float32 epsilon clip, counts at mean >= 0.5: function.py:73-82, 100-115), required
 * exactly when target is given.  1 <= samples <= 1024, objects * samples <= 65535; with VV_BF16 at side >= 8 the samples of ONE
 * object must also stay below 2 GiB (32-bit buffer offsets: samples * side^3 * 128 B, i.e. samples < 512 at side 32, < 64 at side
 * 64), else VV_ERR_SHAPE; larger calls are cut into launches of whole objects.  Per-sample probabilities and logits
 * never reach device memory.  The workspace holds the stats partials and, when the K samples of an object are split over
 * workgroups to fill the chip, at most 8 float32 partial grids per object; it does not depend on samples for samples >= 8. */
size_t vv_convT3d_final_mean_workspace_bytes(int objects, int samples, int side);
int vv_convT3d_final_mean_fwd(const void *x, const float *w_keras, const float *target, float *mean_probs, float *stats,
                              int objects, int samples, int side, int cin, float gamma, float epsilon, int dtype,
                              void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Missing-modality evaluation (nolbo.py:1472-1518; AE: 1277-1322; Pascal: 877-918).  prototypes = the
 * category_vectors array [C,L]; mask [B,L] in {0,1} is the np.random.choice draw of nolbo.py:1475, injected. */

/* z_out = z*mask, then where(z_out == 0, mean_c prototypes, z_out)  (nolbo.py:1477-1482).  z_act (optional) receives the same
 * values as act_dtype, VV_F32 or VV_BF16; any other act_dtype with z_act given is VV_ERR_DTYPE. */
int vv_latent_mask_fill(const float *z, const float *mask, const float *prototypes, int classes, float *z_out,
                        void *z_act, int act_dtype, int batch, int latent, void *stream);
/* argmin[b] = first argmin_c sum_j mask_bj (z_bj - P_cj)^2; mask NULL = all ones (nolbo.py:1489-1493, 1505-1506).
 * argmin[b] is always in [0, classes): only distances below +inf compete (NaN and +inf never do), and a row that has none
 * (a non-finite latent, say) gets 0. */
int vv_nearest_category(const float *z, const float *mask, const float *prototypes, int classes, int *argmin, int batch,
                        int latent, void *stream);
/* z_corr = where(mask == 0, P[argmin] + eps2, z)  (nolbo.py:1507-1510; eps2 = the second normal draw, injected).  Every
 * argmin[b] must be in [0, classes) of `prototypes` (what vv_nearest_category writes).  z_act / act_dtype as in
 * vv_latent_mask_fill. */
int vv_latent_correct(const float *z, const float *mask, const float *prototypes, const int *argmin, const float *eps2,
                      float *z_corr, void *z_act, int act_dtype, int batch, int latent, void *stream);
/* acc[0] = mean_b [argmin_b == argmax_c onehot_bc]  (nolbo.py:1493-1494). */
int vv_category_accuracy(const int *argmin, const float *onehot, int classes, float *acc, int batch, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Stand-alone loss ops with the signatures of src/module/function.py (the fused kernels above are what the
 * model classes use; these serve callers that compose the ops themselves). */

/* binary_loss(xPred probabilities, xTarget, epsilon, gamma, b_range) -> [B]  (function.py:73-82). */
int vv_binary_loss(const float *pred, const float *target, float epsilon, float gamma, float b_range, float *out, int batch,
                   long voxels, void *stream);
/* voxelPrecisionRecall(xTarget, xPred, prob) -> TP,FP,FN [B]  (function.py:100-115). */
int vv_voxel_precision_recall(const float *target, const float *pred, float prob, float *tp, float *fp, float *fn, int batch,
                              long voxels, void *stream);
/* kl_loss(mean, logVar, mean_target, logVar_target) -> [B]  (function.py:84-98). */
int vv_kl_loss(const float *mean, const float *logvar, const float *mean_target, const float *logvar_target, float *out,
               int batch, int latent, void *stream);
/* regulizer_loss (function.py:40-71): pairwise hinge on the scaled L1 distance of latent means,
 * out[i] = sum_j same_class(i,j) * min(sum_l |m_i - m_j| / exp(0.5 lv_i) - dist_in_z_space, 0)^2; class_input may be
 * NULL (every pair counts).  mean, logvar [B,L]; class_input [B,C]; out [B]. */
int vv_regulizer_loss(const float *mean, const float *logvar, const float *class_input, float dist_in_z_space,
                      float *out, int batch, int latent, int class_dim, void *stream);
/* sampling(mu, logVar) = mu + sqrt(exp(logVar))*eps, eps injected  (function.py:35-38). */
int vv_sampling(const float *mu, const float *logvar, const float *eps, float *out, long n, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Precision / recall-vs-threshold counts (pr_curve.hip): the sweep of modelnetAE3.ipynb / pascalAE3.ipynb cell 2 over the
 * `_gt.npy` / `_pred.npy` arrays of test_modelnet_VAE.py:128-130, 159-165, in one streaming pass over device memory for every threshold.
 *   pred        float32 [batch][voxels] probabilities
 *   target      float32 [batch][voxels] (target_packed == 0; a voxel is occupied iff y > 0.5) or packed bits (target_packed == 1: voxel v is
 *               bit v & 7 of byte v >> 3 of a row of voxels / 8 bytes, the layout of vv_pack_bits; voxels % 8 != 0: VV_ERR_SHAPE)
 *   thresholds  float32 [nthr], 1 <= nthr <= 256, any order, duplicates allowed.  For threshold i
 *               TP_i = #{occupied and p > t_i}, FP_i = #{not occupied and p > t_i} with an ordered float32 `>`: a NaN probability exceeds
 *               nothing (it still counts in `totals`), denormals compare as they do in IEEE arithmetic (nothing is flushed).  FN_i is not
 *               stored: FN_i = occupied - TP_i.  An inclusive threshold is a host matter: p >= t <=> p > nextafter(t, -inf) in float32.
 *   sorted      != 0: the caller's promise that thresholds are non-decreasing (a wave then stops at the first threshold none of its
 *               voxels exceeds).  A false promise may give wrong counts, never a wrong address.
 *   group       int32 [batch] or NULL (everything in group 0): sample b is counted into group[b]; a sample whose index is outside
 *               [0, ngroups) is counted nowhere and writes nowhere.
 *   tp_fp       int64 [ngroups][nthr][2] = (TP, FP), ADDED to;  totals int64 [ngroups][2] = (occupied voxels, all voxels), ADDED to:
 *               one pair of buffers accumulates a whole test split.  All arithmetic is integer (32-bit partial counts per 4096-voxel
 *               piece of a sample in the workspace, added to the accumulators by a second launch): the result does not depend on any order.
 * Rows need no alignment beyond that of their element type. */
size_t vv_pr_curve_workspace_bytes(int batch, long voxels, int nthr);
int vv_pr_curve_accumulate(const float *pred, const void *target, int target_packed, const float *thresholds, int nthr, int sorted,
                           const int *group, int ngroups, long long *tp_fp, long long *totals, void *workspace, size_t workspace_bytes,
                           int batch, long voxels, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Occupancy grids -> posed point clouds (voxel_points.hip): objRescaleTransform of src/visualizer/visualizer.py:171-188 for a batch, on
 * the device.  Per object b with grid side D: the occupied cells (i, j, k) in increasing flat index v = (i D + j) D + k (numpy's
 * `offset[mask]` order), lo / hi = their per-axis minimum / maximum, ext = hi - lo, E = max(ext), scale = max(h, w, l) / E (0 when
 * E == 0), q = (cell - lo) scale - (ext scale) / 2 per axis, point = P[:3,:3] q + P[:3,3] in float32.
 *   occ           packed == 0: float32 [batch][D^3], at any 4-byte address; a cell is occupied iff p > prob with an ordered compare (a NaN cell is
 *                 not occupied).  packed != 0: bits, cell v = bit v & 7 of byte v >> 3 of a row of D^3 / 8 bytes
 *                 (the layout of vv_pack_bits; D^3 % 8 != 0: VV_ERR_SHAPE), `prob` is ignored.
 *   surface_only  != 0: only occupied cells on the grid boundary or with an unoccupied face neighbour are counted and emitted; bbox (and
 *                 so the scale) is that of ALL occupied cells either way, so the result is the ordered subset of the full one.
 *   side          1 .. 128, any value.
 *   counts        int32 [batch]: cells emitted per object.   bbox int32 [batch][6] = (lo_i, lo_j, lo_k, hi_i, hi_j, hi_k); an object
 *                 without an occupied cell has (D, D, D, -1, -1, -1) and emits nothing.
 *   offsets       int64 [batch + 1]: exclusive prefix of counts; offsets[batch] is the total.
 *   dims          float32 [batch][3] = (h, w, l);  pose float32 [batch][16], row-major 4x4 of which rows 0 .. 2 are used, or NULL (identity).
 *   points        float32 [capacity][3]: object b's points at rows offsets[b] .. offsets[b + 1] - 1, in cell order (no sort: a cell's row
 *                 is offsets[b] + the count of its object's earlier 4096-cell pieces + its rank inside its piece).  Rows >= capacity
 *                 are not written: nothing past capacity * 3 floats is touched and offsets[batch] > capacity tells the caller.
 * vv_voxel_points_count fills counts / bbox / offsets and the workspace (per-piece counts, prefixes and boxes); vv_voxel_points_emit
 * needs that workspace and the same occ / packed / prob / surface_only / batch / side.  Integer arithmetic and plain stores only: a given
 * input gives the same bits on every run.  Pointers need the alignment of their element type and no more. */
size_t vv_voxel_points_workspace_bytes(int batch, int side);
int vv_voxel_points_count(const void *occ, int packed, float prob, int surface_only, int batch, int side, int *counts, int *bbox,
                          long long *offsets, void *workspace, size_t workspace_bytes, void *stream);
int vv_voxel_points_emit(const void *occ, int packed, float prob, int surface_only, const float *dims, const float *pose,
                         const long long *offsets, const int *bbox, float *points, long long capacity, const void *workspace,
                         size_t workspace_bytes, int batch, int side, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Detections -> posed objects (object_pose.hip, pose_solve.h): getObjectInRealWorld of src/visualizer/visualizer.py:237-308 without its
 * point-cloud step (that is vv_voxel_points_*), for n detections of one frame and one camera.  Per detection: the "too close" pre-filter
 * on the normalised box (x1 > 0.1, x2 < 0.9, y2 < 0.9), pixel scaling, the -5 degree elevation correction, R = RA RE RI in kitti axes,
 * the ray rotation through the box centre, the translation fit of getTranslation (:79-146: 128 corner-to-box-edge assignments k, in the
 * loop nest's execution order; per k the right singular vector of the smallest singular value of a 4x4 matrix, the reference's
 * acceptance tests, the IoU of the reprojected box; the largest IoU wins, ties go to the lowest k), the 4x4 pose, the eight projected
 * corners, the post-filter X[2] > 0.1.  All arithmetic is float64; the interface is float32 / int32.
 *   bbox2d      float32 [n][5] = (x1, y1, x2, y2, objectness), normalised;  bbox3d float32 [n][3] = (w, h, l);
 *   sin_aei / cos_aei   float32 [n][3] = sine / cosine of (azimuth, elevation, in-plane rotation).  A detection with a NaN among these
 *               14 numbers is not kept (candidate -2).
 *   image_col, image_row   the image size in pixels;  proj / proj_inv: HOST pointers to 16 doubles each (row-major 4x4), read during the
 *               call and passed to the kernel by value -- also by vv_object_pose, whose other pointers are device pointers.
 *   n           1 .. 65536.
 *   per detection i:  keep int32 [n] (0 / 1);  candidate int32 [n] = the winning k, -1 when every candidate was rejected (translation 0),
 *               -2 when the detection did not reach the fit;  iou float32 [n] = the winner's IoU (-1 without one).
 *   compacted, row r = the r-th kept detection in input order:  count int32 [1];  index int32 [n] = its i;  pose float32 [n][16];
 *               size float32 [n][3] = (h, l, w);  box2d int32 [n][4] = the pixel box truncated toward zero;  box3d_proj float32 [n][16] =
 *               [2][2][2][2] in the reference's (i, j, k, xy) order.  Rows at or past count are not written.
 * vv_object_pose: two launches on `stream` (a wave per detection; one workgroup compacting with ballots and population counts: no
 * atomics, no sort, the same bits on every run); workspace of vv_object_pose_workspace_bytes(n) bytes (0 for a refused n).
 * vv_object_pose_host: the same code compiled for the CPU, every pointer a host pointer, no stream, no workspace; `translation`, when
 * not NULL, receives the float64 translation of every detection, float64 [n][3] (zeros without a winner); sweeps > 0 overrides the
 * solver's number of Jacobi sweeps (<= 64; 0: the built-in count, which the device always uses).
 * Pointers need the alignment of their element type and no more. */
size_t vv_object_pose_workspace_bytes(int n);
int vv_object_pose(const float *bbox2d, const float *bbox3d, const float *sin_aei, const float *cos_aei, int n, double image_col,
                   double image_row, const double *proj, const double *proj_inv, int *keep, int *candidate, float *iou, int *count,
                   int *index, float *pose, float *size, int *box2d, float *box3d_proj, void *workspace, size_t workspace_bytes,
                   void *stream);
int vv_object_pose_host(const float *bbox2d, const float *bbox3d, const float *sin_aei, const float *cos_aei, int n, double image_col,
                        double image_row, const double *proj, const double *proj_inv, int *keep, int *candidate, float *iou, int *count,
                        int *index, float *pose, float *size, int *box2d, float *box3d_proj, double *translation, int sweeps);
/* The reference's single-object helpers from the same header, on the host, float64 in and out (row-major matrices):
 * getTranslation(proj, R [9], (x_min, y_min, x_max, y_max) in pixels, (w, h, l)) -> translation [3] (zeros without a winner), and when
 * not NULL the winning k (-1: none) and its IoU;  getRay(proj_inv, (px, py)) -> unit ray [3];  getRayRotation(ray) -> R [9];
 * get3DbboxProjection(proj, R, t, w, h, l) -> corners [2][2][2][2]. */
int vv_pose_translation_host(const double *proj, const double *rotation, const double *box2d, const double *whl, double *translation,
                             int *candidate, double *iou);
int vv_pose_ray_host(const double *proj_inv, double px, double py, double *ray);
int vv_pose_ray_rotation_host(const double *ray, double *rotation);
int vv_pose_box_projection_host(const double *proj, const double *rotation, const double *translation, double w, double h, double l,
                                double *corners);

/* ---------------------------------------------------------------------------------------------------------
 * Detector head -> selected detections (detect_decode.hip, detect_decode.h): nolbo_test.getPred of src/module/nolbo_test.py:81-153 with
 * its _encOutPartitioning (:214-255) and function.nonMaximumSuppresion (src/module/function.py:117-150), for `batch` independent frames
 * (the reference does frame 0 only).  All arithmetic is float32 in the reference's operation order and with its roundings under numpy 2.
 *   head        float32, batch frames of grid_row x grid_col cells with channels = predictor_num * W values each, W = 1 + 4 + 3 + 2 Z + 9
 *               (Z = z_dim; the reference: 5 predictors, Z = 16, 245 channels).  layout 0: [batch][row][col][channel] (channels
 *               innermost); layout 1: [batch][channel][row][col] (planes: what the torch head holds before its final permute).  Any other
 *               layout, or channels != predictor_num * W: VV_ERR_SHAPE.
 *               Per predictor, in this order: objectness 1 (sigmoid) | bbox2D 4 = (h, w, x, y): exp, exp, sigmoid, sigmoid | bbox3D 3
 *               (relu) | inst_mean Z | inst_log_var Z | sin 3 (tanh) | cos 3 (tanh) | rad_log_var 3.  exp, sigmoid and tanh are the
 *               header's own (fmaf polynomials, no library call): exp overflows to +inf above 88.72283 as numpy's does and returns 0
 *               below -87.3, sigmoid returns 0 below -87; a NaN stays a NaN.
 *   limits      batch >= 1; 1 <= predictor_num <= 16; 1 <= z_dim <= 64; N = grid_row * grid_col * (top_1 ? 1 : predictor_num) <= 4096
 *               candidate slots per frame.  Anything else: VV_ERR_SHAPE.
 *   candidates  cells in row-major order; inside a cell the predictors in descending objectness, equal values the lower predictor first.
 *               A predictor is a candidate when objectness > obj_thresh (strict; a NaN never is).  top_1 != 0: only the cell's first
 *               predictor in that order can be one.
 *   box         (col_min, row_min, col_max, row_max): t = f32(f32(row) + y), q = f32(t / grid_row) (correctly rounded),
 *               row_min = f32(q - f32(h / 2)), row_max = f32(q + f32(h / 2)); columns likewise with x, w, grid_col.
 *   NMS         greedy: candidates in descending objectness, equal values the HIGHER candidate index first (a stable ascending sort read
 *               from its end; numpy's argsort gives no rule).  A pick suppresses every live candidate with IoU > iou_thresh (strict; a
 *               NaN IoU -- 0/0, inf/inf -- suppresses nothing): area = (rMax - rMin) * (cMax - cMin), inter = max(0, .) * max(0, .),
 *               union = f32(area_i + area_j) - inter, IoU = inter / union, max / min returning NaN for a NaN operand as numpy's do.
 *   outputs     per frame b, rows in PICK order, row r of frame b at [b * N + r]:  count int32 [batch];  index int32 [batch][N] = cell *
 *               predictor_num + predictor;  bbox2d float32 [batch][N][5] = (col_min, row_min, col_max, row_max, objectness) -- the row
 *               vv_object_pose takes;  bbox3d float32 [batch][N][3] = (field 1, field 0, field 2) as the reference swaps them;
 *               inst_mean, inst_log_var float32 [batch][N][Z];  sin_aei, cos_aei, rad_log_var float32 [batch][N][3].  Rows at or past
 *               count[b] are not written.
 * vv_detect_decode: ONE launch on the hipStream_t `hip_stream`, a 256-thread workgroup per frame, candidates in LDS (up to 135232 bytes), no workspace;
 * ballots and population counts, a counting rank and a scan with one barrier per pick: no atomics, no sort, the same bits on every run.
 * vv_detect_decode_host: the same code compiled for the CPU, every pointer a host pointer, no stream.  The two agree bit for bit.
 * vv_detect_activation_host: the header's exp (which 0), sigmoid (1) or tanh (2) of n float32 values, on the host.
 * Pointers need the alignment of their element type and no more. */
int vv_detect_decode(const float *head, int layout, int batch, int grid_row, int grid_col, int predictor_num, int z_dim, int channels,
                     float obj_thresh, float iou_thresh, int top_1, int *count, int *index, float *bbox2d, float *bbox3d,
                     float *inst_mean, float *inst_log_var, float *sin_aei, float *cos_aei, float *rad_log_var, void *hip_stream);
int vv_detect_decode_host(const float *head, int layout, int batch, int grid_row, int grid_col, int predictor_num, int z_dim, int channels,
                          float obj_thresh, float iou_thresh, int top_1, int *count, int *index, float *bbox2d, float *bbox3d,
                          float *inst_mean, float *inst_log_var, float *sin_aei, float *cos_aei, float *rad_log_var);
int vv_detect_activation_host(const float *x, float *y, long n, int which);

/* ---------------------------------------------------------------------------------------------------------
 * The latent stage of the multi-modal model nolboSingleObject (src/module/nolbo.py:49-324): everything between the image encoder's head
 * output and the decoder's input.  enc_out float32 [B, 2 Lc + 2 Li] = [mean_c | logVar_c | mean_i | logVar_i]; every latent-shaped array
 * is [category (Lc) | instance (Li)], float32.  1 <= Lc, Li <= 64; 1 <= classes, insts <= 256; B >= 1; else VV_ERR_SHAPE.  NULL and shape
 * checks come before any launch.  Pointers need the alignment of their element type and no more.  The arithmetic is csrc/mm_latent.h:
 * float32, exp from csrc/detect_decode.h, correctly rounded division and square root, no contraction, every sum in one fixed order, no
 * atomics -- the same bits on every run, and the *_host entries (the same header in loops on the CPU, host pointers, no stream) agree
 * with the device entries bit for bit.
 *
 * vv_mm_latent_eval  (getEval, nolbo.py:183-252; two launches: a workgroup per sample, then one workgroup for the accuracies)
 *   eps [B, Lc+Li]      the category draw, then the instance draw (the order of the reference's two `sampling` calls, :196-197)
 *   mask [B, Lc]        in {0,1}: the np.random.choice draw of :202, or NULL (missing_prob == 0);  eps2 [B, Lc]: the draw of :242,
 *                       required exactly when mask is given (a mismatch is VV_ERR_NULL)
 *   prior_cat [C, Lc]   the category prior's means;  prior_inst [B, I, Li]: the instance prior's means of EACH sample (:166-181)
 *   cat_onehot [B, C], inst_onehot [B, I]
 *   z [B, Lc+Li]        logVar clipped to [-10, 10]; z = mean + sqrt(exp(logVar)) eps (:185-197); with a mask the category half is
 *                       z_c mask, and every element of it that compares equal to 0 -- an unmasked +-0 too -- takes the column mean of
 *                       prior_cat (:204-208).  The instance half is never masked.
 *   z_corr [B, Lc+Li]   mask given (then required): where(mask == 0, prior_cat[idx 2] + eps2, z_c) | z_i (:239-252)
 *   z_act, z_corr_act   optional: the same values as act_dtype (VV_F32 / VV_BF16, round to nearest even); any other act_dtype with one of
 *                       them given is VV_ERR_DTYPE
 *   idx int32 [B, 4]    first argmin of the squared distance: z_c to prior_cat (:218-219), z_i to prior_inst[b] (:225-226), the masked
 *                       distance sum_j mask_j (z_c - P)_j^2 (:239-240), z_c_corr to prior_cat (:248-249).  Only distances below +inf
 *                       compete; a row that has none gets 0.  Without a mask columns 2 and 3 repeat column 0.
 *   acc float32 [3]     acc_cat, acc_inst, acc_cat_corrected against the first argmax of the one-hots (:219-227, :249-250); without a mask
 *                       acc[2] = acc[0]. */
int vv_mm_latent_eval(const float *enc_out, const float *eps, const float *mask, const float *eps2, const float *prior_cat,
                      const float *prior_inst, const float *cat_onehot, const float *inst_onehot, float *z, float *z_corr, void *z_act,
                      void *z_corr_act, int act_dtype, int *idx, float *acc, int batch, int lc, int li, int classes, int insts,
                      void *hip_stream);
int vv_mm_latent_eval_host(const float *enc_out, const float *eps, const float *mask, const float *eps2, const float *prior_cat,
                           const float *prior_inst, const float *cat_onehot, const float *inst_onehot, float *z, float *z_corr, void *z_act,
                           void *z_corr_act, int act_dtype, int *idx, float *acc, int batch, int lc, int li, int classes, int insts);
/* vv_mm_latent_train_fwd  (fit, nolbo.py:93-140; one launch)
 *   mean_cp, lv_cp [B, Lc]; mean_ip, lv_ip [B, Li]   the two prior networks' outputs for each sample (:95-97), not clipped
 *   eps, eps_p [B, Lc+Li]   the posterior's and the prior's draws (:110-115);  noise [B, Lc+Li] in {0,1} or NULL (:119-123)
 *   z_in = where(noise == 0, z, z_prior); noise NULL: z_in = z.  z_in_act: optional twin as in vv_mm_latent_eval.
 *   kl [B]  = kl_loss(category) + kl_loss(instance) against the given priors (function.py:84-98)
 *   reg [B] = regulizer_loss(mean_cp, lv_cp, 3 Lc) + regulizer_loss(mean_ip, lv_ip, 3 Li, class_input = cat_onehot [B, classes])
 *             (function.py:40-71): the scale is exp(0.5 lv_i) of row i, the hinge keeps d^2 where d <= 0, the instance term counts the
 *             pairs whose one-hot rows are equal.
 * vv_mm_latent_train_bwd  (one launch): for total = mean_b kl + mean_b reg + shape, with dz_in [B, Lc+Li] = d shape / d z_in and
 *   inv_batch = 1 / B, writes d_enc_out [B, 2 Lc + 2 Li] and the gradients of the four prior outputs (each may be NULL: a constant
 *   log-variance has none).  A log-variance gradient passes the clip where -10 <= raw <= 10 (as vv_reparam_kl_bwd); d|x|/dx at 0 is 0;
 *   row i receives the (i, j) and the (j, i) pairs, summed over j in ascending order. */
int vv_mm_latent_train_fwd(const float *enc_out, const float *eps, const float *mean_cp, const float *lv_cp, const float *mean_ip,
                           const float *lv_ip, const float *eps_p, const float *noise, const float *cat_onehot, float *z_in, void *z_in_act,
                           int act_dtype, float *kl, float *reg, int batch, int lc, int li, int classes, void *hip_stream);
int vv_mm_latent_train_fwd_host(const float *enc_out, const float *eps, const float *mean_cp, const float *lv_cp, const float *mean_ip,
                                const float *lv_ip, const float *eps_p, const float *noise, const float *cat_onehot, float *z_in,
                                void *z_in_act, int act_dtype, float *kl, float *reg, int batch, int lc, int li, int classes);
int vv_mm_latent_train_bwd(const float *enc_out, const float *eps, const float *mean_cp, const float *lv_cp, const float *mean_ip,
                           const float *lv_ip, const float *eps_p, const float *noise, const float *cat_onehot, const float *dz_in,
                           float inv_batch, float *d_enc_out, float *d_mean_cp, float *d_lv_cp, float *d_mean_ip, float *d_lv_ip, int batch,
                           int lc, int li, int classes, void *hip_stream);
int vv_mm_latent_train_bwd_host(const float *enc_out, const float *eps, const float *mean_cp, const float *lv_cp, const float *mean_ip,
                                const float *lv_ip, const float *eps_p, const float *noise, const float *cat_onehot, const float *dz_in,
                                float inv_batch, float *d_enc_out, float *d_mean_cp, float *d_lv_cp, float *d_mean_ip, float *d_lv_ip,
                                int batch, int lc, int li, int classes);

/* ---------------------------------------------------------------------------------------------------------
 * The latent stage of the models with ONE latent group and ONE learned prior: nolboSingleObject_instOnly (src/module/nolbo.py:326-540),
 * nolboSingleObject_category_only (:984-1204) and nolboSingleObject_modelnet_category_only (:1594-1787).  enc_out float32 [B, 2 L] =
 * [mean | logVar]; every other array is float32 [B, L] unless stated.  1 <= L <= 64; B >= 1; 1 <= insts <= 256; else VV_ERR_SHAPE.
 * NULL and shape checks come before any launch.  Pointers need the alignment of their element type and no more.  The arithmetic is
 * csrc/prior_latent.h on the scalar helpers of csrc/mm_latent.h: float32, exp from csrc/detect_decode.h, correctly rounded division and
 * square root, no contraction, no atomics, EVERY sum in ascending index order (over l, over the prior table's rows, over the batch j)
 * -- the same bits on every run, and the *_host entries (the same header in loops on the CPU, host pointers, no stream) agree with the
 * device entries bit for bit.  There is no dtype argument: a bfloat16 twin (round to nearest even) is written where its pointer is
 * given.
 *
 * vv_prior_latent_train_fwd  (fit, nolbo.py:365-403, :1023-1063; one launch: a wave per sample, the batch walked in pieces through LDS)
 *   mean_p, lv_p        the prior network's outputs for each sample, not clipped;  eps, eps_p: the posterior's and the prior's draws
 *   keep                in {0,1} or NULL;  dist: dist_in_z_space (10 L for instOnly, 3 L for category_only)
 *   z = mean + sqrt(exp(clip(logVar, -10, 10))) eps;  z_prior = mean_p + sqrt(exp(lv_p)) eps_p
 *   z_in                keep NULL: z; else where(keep == 1, z, z_prior) (:1047) -- all zeros: instOnly's decoder(z_prior) branch (:386)
 *   z_in_bf16           optional twin of z_in
 *   kl [B]              kl_loss against the given prior (function.py:84-98)
 *   reg [B]             regulizer_loss(mean_p, lv_p, dist) without a class input (function.py:40-71): d_ij = sum_l |m_i - m_j|_l /
 *                       exp(0.5 lv_i)_l - dist;  reg_i = sum_j (d_ij <= 0 ? d_ij^2 : 0) over j ascending, j = i included
 * vv_prior_latent_train_bwd  (one launch): for total = mean_b kl + reg_weight mean_b reg + shape, with dz_in = d shape / d z_in and
 *   inv_batch = 1 / B, writes d_enc_out [B, 2 L], d_mean_p and d_lv_p (each of the last two may be NULL: a constant log-variance has no
 *   gradient).  dz_in goes to the posterior where the element took z and to the prior where it took z_prior.  A log-variance gradient
 *   passes the clip where -10 <= raw <= 10 (as vv_reparam_kl_bwd); d|x|/dx at 0 is 0; row i receives the (i, j) and the (j, i) pairs,
 *   summed over j in ascending order. */
int vv_prior_latent_train_fwd(const float *enc_out, const float *eps, const float *mean_p, const float *lv_p, const float *eps_p,
                              const float *keep, float dist, float *z_in, void *z_in_bf16, float *kl, float *reg, int batch, int latent,
                              void *hip_stream);
int vv_prior_latent_train_fwd_host(const float *enc_out, const float *eps, const float *mean_p, const float *lv_p, const float *eps_p,
                                   const float *keep, float dist, float *z_in, void *z_in_bf16, float *kl, float *reg, int batch,
                                   int latent);
int vv_prior_latent_train_bwd(const float *enc_out, const float *eps, const float *mean_p, const float *lv_p, const float *eps_p,
                              const float *keep, float dist, const float *dz_in, float inv_batch, float reg_weight, float *d_enc_out,
                              float *d_mean_p, float *d_lv_p, int batch, int latent, void *hip_stream);
int vv_prior_latent_train_bwd_host(const float *enc_out, const float *eps, const float *mean_p, const float *lv_p, const float *eps_p,
                                   const float *keep, float dist, const float *dz_in, float inv_batch, float reg_weight,
                                   float *d_enc_out, float *d_mean_p, float *d_lv_p, int batch, int latent);
/* vv_inst_latent_eval  (instOnly.getEval, nolbo.py:417-485; one launch: a workgroup per sample)
 *   mask in {0,1} or NULL (missing_prob == 0);  fill: the N(0,1) draw of :438, required exactly when mask is given (a mismatch is
 *                       VV_ERR_NULL)
 *   prior [insts, L]    the instance prior's means
 *   z                   the sample; with a mask z mask, and every element that compares equal to 0 -- an unmasked +-0 too -- takes
 *                       fill (:435-439)
 *   idx int32 [B]       first argmin over i of sum_l mask_l (z - prior_i)_l^2 (:460-462; the mask counts as ones when NULL).  Only
 *                       distances below +inf compete; a row that has none gets 0.
 *   z_corr              prior[idx], the whole row (:474)
 *   z_bf16, z_corr_bf16 optional twins */
int vv_inst_latent_eval(const float *enc_out, const float *eps, const float *mask, const float *fill, const float *prior, float *z,
                        float *z_corr, void *z_bf16, void *z_corr_bf16, int *idx, int batch, int latent, int insts, void *hip_stream);
int vv_inst_latent_eval_host(const float *enc_out, const float *eps, const float *mask, const float *fill, const float *prior, float *z,
                             float *z_corr, void *z_bf16, void *z_corr_bf16, int *idx, int batch, int latent, int insts);

/* ---------------------------------------------------------------------------------------------------------
 * The image encoder: Darknet19 and head2D (src/net_core/darknet.py:83-94 Darknet19Conv, :96-133 the backbone, :135-168 convHead /
 * head2D) as channels-last 2D layers.  Here grids are NOT cubic and NOT powers of two: x [B,R,C,Cin], any batch, rows, cols >= 1.
 *
 *   y[b,r,c,co] = act(scale[co] * sum_{tr,tc,ci} x[b, r+tr-p, c+tc-p, ci] * w[tr,tc,ci,co] + shift[co]),   p = ksize / 2
 *
 * Conv2D(ksize in {1, 3}, strides 1, 'same', no bias) -> BatchNormalization folded by vv_fold_bn (Keras epsilon 1e-3) -> activation;
 * taps outside the image contribute zero.  An implicit GEMM with rows m = (b R + r) C + c, K = ksize^2 Cin, N = Cout on MFMA with f32
 * accumulation: dtype VV_BF16 = v_mfma_f32_32x32x16_bf16, VV_F32 = v_mfma_f32_32x32x2_f32 (the exact-f32 parity mode).  x and w_packed
 * have `dtype`, y has `out_dtype` (VV_BF16 or VV_F32, chosen separately: the head's last convolution stores f32 from bf16 operands);
 * scale / shift are float32 [Cout] and may be NULL (identity).  One rounding: the f32 accumulator goes through the f32 fold and the
 * activation and is rounded once to out_dtype.
 *   cin      3 or a multiple of 32.  cin == 3 is the IMAGE: x is float32 [B,R,C,3] whatever `dtype` says, and is rounded to `dtype`
 *            as it is read.
 *   cout     any value >= 1 (the packed image is padded to a multiple of 64 channels, the stores are masked).
 *   act      VV_ACT_*; VV_ACT_LRELU uses `alpha` as its slope (darknet.py:87-88 uses 0.1; the 3D layers' entries keep their 0.3).
 *   limits   every tensor at most 2^31 - 1 elements, else VV_ERR_SHAPE (cut the batch); so is every other shape above not taken.
 *            All of it is decided before any launch.
 *   small M  K is cut into vv_conv2d_splits(...) shares when the tiles alone would not fill the device; each share writes a float32
 *            slab into the workspace and one more launch sums them in share order (no atomics: the same bits on every run).
 *            1 share = one launch, no workspace.  vv_conv2d_workspace_bytes is the minimum; more changes nothing.
 * vv_pack_conv2d: Keras kernel [k,k,cin,cout] float32 -> [ceil(k*k*cin/32)][ceil(cout/64)*64][32] of `dtype`, zero padded
 *            (vv_conv2d_packed_bytes bytes; device to device).
 * vv_maxpool2d_same_fwd: MaxPool2D(2, 2, 'same') (darknet.py:100-124): y [B,ceil(R/2),ceil(C/2),channels], ceil mode -- for an odd
 *            size the last window is one wide (padding only at the end).  Exact in either dtype.
 * head2D's last_pooling (darknet.py:165-168): 'max' is vv_max_over_positions on the float32 head output; 'average' has no entry
 *            here and stays a reduction of the caller on that float32 output.
 * The stream parameter is a hipStream_t passed as void*, like every `stream` above.  x, w_packed, y and the workspace are 16-byte aligned. */
size_t vv_conv2d_packed_bytes(int ksize, int cin, int cout, int dtype);
int vv_pack_conv2d(const float *w_keras, void *packed, int ksize, int cin, int cout, int dtype, void *hip_stream);
int vv_conv2d_supported(int ksize, int cin, int cout, int dtype, int out_dtype);
int vv_conv2d_splits(int batch, int rows, int cols, int ksize, int cin, int cout);
size_t vv_conv2d_workspace_bytes(int batch, int rows, int cols, int ksize, int cin, int cout, int dtype);
int vv_conv2d_fwd(const void *x, const void *w_packed, const float *scale, const float *shift, void *y, int batch, int rows, int cols,
                  int cin, int cout, int ksize, int act, float alpha, int dtype, int out_dtype, void *workspace, size_t workspace_bytes,
                  void *hip_stream);
int vv_maxpool2d_same_fwd(const void *x, void *y, int batch, int rows, int cols, int channels, int dtype, void *hip_stream);

/* The layers Darknet53 / Darknet53Tiny add to that (darknet.py:11-81): a stride-2 convolution, a residual add in the epilogue and the
 * stride-1 pool.  The same kernels, weights packed by vv_pack_conv2d as for any k3 layer; statuses, limits and alignment as above.
 *
 *   stride   1: the 'same' convolution of vv_conv2d_fwd (ksize 1 or 3).  2: ZeroPadding2D(((1,0),(1,0))) + 'valid' k3 s2
 *            (Darknet53Conv, darknet.py:11-31); ksize == 3, rows, cols >= 2, cin a multiple of 32, else VV_ERR_SHAPE:
 *              y[b,ro,co,n] = act(scale[n] * sum_{tr,tc,ci} x[b, 2ro+tr-1, 2co+tc-1, ci] * w[tr,tc,ci,n] + shift[n]) (+ residual)
 *            on the output grid floor(rows/2) x floor(cols/2); a tap with index -1 is zero, and for an odd size the last input row /
 *            column is never read.  rows, cols are always the INPUT grid.
 *   residual NULL, or a tensor of y's shape in the operand type `dtype`, 16-byte aligned, not overlapping y:
 *              y = round_once(act(scale * acc + shift) + residual)
 *            added in float32 behind the activation (darknet.py:33-38), in the one-launch form and in the split-K epilogue alike (the
 *            shares still summed 0, 1, 2, ...).  Either stride.
 *   small M  vv_conv2d_ex_splits / _workspace_bytes decide on the OUTPUT's rows; at stride 1 they equal the queries above.
 * vv_conv2d_ex_fwd(stride 1, residual NULL) runs the very kernel of vv_conv2d_fwd: the same bits.
 * vv_maxpool2d_s1_same_fwd: MaxPool2D(2, 1, 'same') (darknet.py:77): y has x's grid, y[r,c] = max x[r..min(r+1,R-1), c..min(c+1,C-1)]
 *            (padding only at the end).  Exact in either dtype. */
int vv_conv2d_ex_supported(int ksize, int stride, int cin, int cout, int dtype, int out_dtype);
int vv_conv2d_ex_splits(int batch, int rows, int cols, int ksize, int stride, int cin, int cout);
size_t vv_conv2d_ex_workspace_bytes(int batch, int rows, int cols, int ksize, int stride, int cin, int cout, int dtype);
int vv_conv2d_ex_fwd(const void *x, const void *w_packed, const float *scale, const float *shift, const void *residual, void *y, int batch,
                     int rows, int cols, int cin, int cout, int ksize, int stride, int act, float alpha, int dtype, int out_dtype,
                     void *workspace, size_t workspace_bytes, void *hip_stream);
int vv_maxpool2d_s1_same_fwd(const void *x, void *y, int batch, int rows, int cols, int channels, int dtype, void *hip_stream);

/* ---------------------------------------------------------------------------------------------------------
 * Training path (nolboSingleObject_modelnet_category_{VAE,AE}.fit, nolbo.py:1411-1447 / 1230-1258).  float32.
 * Data gradients reuse the forward kernels: d(Conv3D k4 s2)/d(input) = vv_convT3d_k4s2_fwd with the SAME Keras
 * kernel array packed by vv_pack_convT_k4s2 (read as [4,4,4,Cout_T = Cin, Cin_T = Cout]); d(Conv3DTranspose k4 s2)/
 * d(input) = vv_conv3d_k4s2_fwd with vv_pack_conv_k4 of the same array; Dense: vv_dense_fwd with the Keras
 * [in,out] array as the [N][K] panel. */

/* BatchNormalization(training=True) statistics over x[rows][channels] (autoencoder3D.py:31,46,62): batch mean,
 * biased variance, rstd = 1/sqrt(var+eps), folded scale = gamma*rstd, shift = beta - mean*scale; moving statistics
 * updated in place with `momentum` (Keras 0.99) when the pointers are non-NULL. */
size_t vv_bn_workspace_bytes(long rows, int channels);
int vv_bn_train_stats(const void *x, long rows, int channels, const float *gamma, const float *beta, float eps,
                      float momentum, float *mean, float *var, float *rstd, float *scale, float *shift,
                      float *moving_mean, float *moving_var, int dtype, void *workspace, size_t workspace_bytes,
                      void *stream);
/* Batch statistics from per-block column sums a producer kernel left (round 4): the widest decoder layer's training-mode forward,
 * vv_convT3d_k4s2_whole_stats_fwd (raw bf16 output + partial[(block * 2 + {sum, sum of squares}) * cout + channel], block = sample;
 * vv_convT3d_k4s2_whole_stats_blocks(batch) blocks), and the finalisation of vv_bn_train_stats on such partials: the statistics
 * sweep over the layer's output is not run.  Same results as vv_convT3d_k4s2_whole_fwd + vv_bn_train_stats up to the float32
 * summation order of the column sums (finalised in double). */
int vv_convT3d_k4s2_whole_stats_blocks(int batch);
int vv_convT3d_k4s2_whole_stats_fwd(const void *x, const void *w_skip, void *y, float *stats_partial, size_t stats_bytes, int batch,
                                    int side, int cin, int cout, int dtype, void *stream);
int vv_bn_finalize_stats(const float *partial, int nblocks, long rows, int channels, const float *gamma, const float *beta, float eps,
                         float momentum, float *mean, float *var, float *rstd, float *scale, float *shift, float *moving_mean,
                         float *moving_var, void *stream);
/* y = act(x*scale + shift) */
int vv_bn_act_fwd(const void *x, const float *scale, const float *shift, void *y, long rows, int channels, int act,
                  int dtype, void *stream);
/* Backward of act(BN(x)): given dy = dL/dy, writes dgamma, dbeta [channels] and dx = dL/dx [rows][channels]. */
int vv_bn_act_bwd(const void *x, const void *dy, const float *scale, const float *shift, const float *mean,
                  const float *rstd, float *dgamma, float *dbeta, void *dx, long rows, int channels, int act,
                  int dtype, void *workspace, size_t workspace_bytes, void *stream);

/* Weight gradients as reduction-over-rows GEMMs on the exact-f32 MFMA: dw[m][n] = sum_r a[r][m] * g[r][n].  The operands
 * may be float32 or bf16 independently (*_dtype; bf16 is widened when staged); dw is always float32. */
size_t vv_wgrad_workspace_bytes(long rows, int m, int n);
int vv_wgrad_dense(const void *a, const void *g, float *dw, long rows, int m, int n, int lda, int a_dtype, int g_dtype,
                   void *workspace, size_t workspace_bytes, void *stream);
/* a[r][(t,ci)] = src[b, 2o-1+t, ci] gathered over the half-size grid (zero in the SAME padding); g [B*(side/2)^3][cout].
 * Conv3D k4 s2 (src = layer input, g = dL/d(conv out)): dw = Keras [4,4,4,cin,cout].  Conv3DTranspose k4 s2 (src =
 * dL/d(out) on the big grid, g = layer input): dw = Keras [4,4,4,Cout,Cin] with (cin, cout) := (Cout, Cin).
 * cin == 1 (first conv / last transposed conv) or cin % 64 == 0. */
int vv_wgrad_conv_k4s2(const void *src, const void *g, float *dw, int batch, int side, int cin, int cout, int src_dtype,
                       int g_dtype, void *workspace, size_t workspace_bytes, void *stream);
/* Adjoints of vv_pack_conv_k4s1_meanpool / vv_pack_convT_k4s1_dense: panel gradient -> Keras kernel gradient. */
int vv_unpack_meanpool_grad(const float *dpanel, float *dw, int side, int cin, int cout, void *stream);
int vv_unpack_convT_dense_grad(const float *dpanel, float *dw, int side, int cin, int cout, void *stream);
/* out[cols][rows] = in[rows][cols]^T (panel transposes for the dense-panel data gradients). */
int vv_transpose_f32(const float *in, float *out, int rows, int cols, void *stream);
/* out[c] = sum_r x[r][c] (Dense bias gradient). */
int vv_colsum(const void *x, float *out, long rows, int cols, int dtype, void *stream);

/* dlogit = d(mean_b binary_loss_b)/dlogit through sigmoid and the epsilon clip (function.py:73-82). */
int vv_bce_bwd(const float *probs, const float *target, float *dlogit, int batch, long voxels, float gamma, float epsilon,
               float inv_batch, void *stream);
/* Backward of vv_reparam_kl_fwd for total = mean_b KL + ...: d_enc_out [B,2L] from dz [B,L]. */
int vv_reparam_kl_bwd(const float *enc_out, const float *eps, const float *dz, const float *drop_mask, float drop_scale,
                      float *d_enc_out, int batch, int latent, float inv_batch, void *stream);
/* Keras Adam: m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; param -= lr_t m / (sqrt(v) + eps),
 * lr_t = lr sqrt(1-b2^t)/(1-b1^t) computed by the caller (nolbo.py:1402, 1441). */
int vv_adam_step(float *param, const float *grad, float *m, float *v, long n, float lr_t, float beta1, float beta2,
                 float epsilon, void *stream);

/* vv_adam_step for every variable in one launch: chunk_table is a device array of nchunks records
 * { float *param; const float *grad; float *m; float *v; long n; } (40 bytes, pointers already offset, n <= 16384). */
int vv_adam_step_multi(const void *chunk_table, int nchunks, float lr_t, float beta1, float beta2, float epsilon,
                       void *stream);

/* vv_adam_step_multi with an l2 regulariser (loss term coef/2 * sum w^2 per chunk) folded into the gradient, and the
 * regulariser's sum w^2 left behind by the same pass (AE3D.py:82-87).  chunk_table is a device array of nchunks records
 * { float *param; const float *grad; float *m; float *v; long n; float coef; float pad; } (48 bytes, pointers already
 * offset, n <= 16384).  Per element g_eff = fma(coef, w, grad), then the Adam rule on g_eff; a chunk with coef == 0
 * gives vv_adam_step_multi's bits.  sumsq_partial [nchunks] float32: sum w^2 of the chunk's weights BEFORE the update
 * (the weights the forward pass used) where coef != 0, summed in a fixed order (no atomics: the same state gives the
 * same bits), and 0 where coef == 0.  grad is only read. */
int vv_adam_step_multi_l2(const void *chunk_table, int nchunks, float lr_t, float beta1, float beta2, float epsilon,
                          float *sumsq_partial, void *hip_stream);
/* The six scalars of one AE3D.fit step (AE3D.py:67-90) from stats [batch,4] = per-sample (bce, TP, FP, FN) and the
 * partials of vv_adam_step_multi_l2 (nchunks may be 0), every sum in double in a fixed order:
 * out6 = (reg = l2 * sum w^2, pred = sum bce * inv_global_batch, reg + pred, sum TP * inv_global_batch, FP, FN). */
int vv_ae3d_step_scalars(const float *stats, int batch, const float *sumsq_partial, int nchunks, float l2,
                         float inv_global_batch, float *out6, void *hip_stream);

/* dst[i] = (dst type) src[i] between float32 and bf16 (round to nearest even): operand casts of the mixed-precision
 * training step. */
int vv_convert(const void *src, void *dst, long n, int src_dtype, int dst_dtype, void *stream);

/* ---- bit-packed occupancy grids (modelnet_dataset.py:74-91 keeps float32 grids on the host and copies a batch per
 * iteration; 32^3 voxels are 4 KiB as bits).  Voxel v of a sample is bit (v & 7) of byte v >> 3.
 * vv_unpack_bits_gather: out[b][v] = bit v of sample index[b] (index NULL: b) as 0.0f / 1.0f; voxels % 8 == 0.
 * vv_pack_bits: bit = x >= threshold, over n floats (n % 8 == 0). */
int vv_unpack_bits_gather(const void *packed, const int *index, float *out, int batch, long voxels, void *stream);
int vv_pack_bits(const float *x, void *packed, float threshold, long n, void *stream);

/* ---- Bernoulli keep masks from a counter-based generator, and inverted dropout on a float32 latent (csrc/keep_mask.h: the
 * dropout mask of fit, nolbo.py:1423-1425, and the missing-latent mask of getEval, :1475-1476; keep = u >= p in both).
 * vv_keep_mask: keep [batch, latent] float32 (1.0f kept, 0.0f dropped), the mask format of vv_reparam_kl_fwd / _bwd.
 *   Element e = b * latent + j is word e & 3 of the Philox4x32-10 block with counter (blk_lo, blk_hi, offset_lo, offset_hi),
 *   blk = e >> 2, and key (seed_lo, seed_hi); u = float(word >> 8) * 2^-24 in [0, 1 - 2^-24]; keep = u >= rate.  One launch.
 * vv_keep_mask_host: the same arithmetic in a loop on host pointers, bit for bit the device's mask; needs no GPU.
 * vv_mask_scale: y = (x * keep) * scale in float32 (two roundings), x, keep, y [batch, latent]; x and y are distinct
 *   buffers.  The forward of autoencoder dropout on the encoder output and its backward on dz.  One launch.
 * Refused before any launch: a NULL pointer (VV_ERR_NULL); batch <= 0, latent <= 0 or more than 2^31 - 1 elements, a rate
 * that is NaN or outside [0, 1) (VV_ERR_SHAPE).  Pointers need float alignment and no more. */
int vv_keep_mask(float *keep, int batch, int latent, float rate, unsigned long long seed, unsigned long long offset,
                 void *hip_stream);
int vv_keep_mask_host(float *keep, int batch, int latent, float rate, unsigned long long seed, unsigned long long offset);
int vv_mask_scale(const float *x, const float *keep, float scale, float *y, int batch, int latent, void *hip_stream);

/* ---- Pascal3D image batches built on the device (csrc/augment.h states every expression and the table of random draws): the
 * reference's input pipeline, pascal3D.py:216-242 calling datasetUtils.py:91-152 -- crop the box with a random border, flip, Invert
 * and Add per channel, cv2.warpAffine semantics with a random scale and translation (bilinear, constant border 0, the result held
 * as an integer level), cv2.resize INTER_CUBIC semantics (half-pixel centres, Keys a = -0.75, replicate, no antialiasing), / 255.
 * The function is defined in floating point (IEEE float64 for the warp and the cubic stage, written once for host and device); cv2's
 * fixed-point coefficient tables are not modelled.  The entries below apply Invert and Add, as they always did; GaussianBlur and
 * AddToHueAndSaturation (datasetUtils.py:64-89, the other two of imgAug's four) are applied by the _ex entries further down, per
 * sample and opt-in through a second table.
 *   images      one uint8 arena of HWC 3-channel images of differing sizes
 *   image_meta  int64 [n_images][3] = (byte offset, rows, cols), rows and cols at most 16383
 *   params      int32 [batch][16]: 0 image index; 1..4 crop row0, col0, rows h, cols w in the padded image's coordinates; 5 flip
 *               bits (0 horizontal, 1 vertical); 6 scale as float32 bits; 7, 8 dRow, dCol; 9 invert bits per channel; 10..12
 *               additive value per channel; 13, 14 rowPad, colPad (a zero border; coordinates outside the image read 0); 15 zero
 *   out         float32 [batch][out_rows][out_cols][3], channel order as stored
 * vv_augment_images: ONE launch on `hip_stream` for the batch, a workgroup per 16 x 16 output tile; the tile's footprint of warped
 *   levels is built in LDS (48 KiB) and the cubic stage runs out of it; a tile whose footprint does not fit takes the direct
 *   per-pixel form (csrc/augment.hip states the rule).  No workspace, no atomics: the same bits on every run.
 * vv_augment_images_host: the same code on host pointers, no stream; bit for bit the device's output.
 * vv_augment_draw: params rows from (image_index [batch], boxes [batch][4] = colMin, rowMin, colMax, rowMax float32) on
 *   Philox4x32-10 (csrc/keep_mask.h): sample b owns blocks 8b .. 8b+7 of counter (blk, offset) under key seed.  augmentation = 0:
 *   border 0.1, no flip, scale 1, no translation, no colour change.  One launch, a thread per sample.
 * vv_augment_draw_host: the same on host pointers; bit for bit the device's rows.
 * vv_augment_check_host: the admissibility of params rows against image_meta alone (host pointers).
 * Refused before any launch: a NULL pointer (VV_ERR_NULL); n_images < 1, batch < 1 (images: > 65535), out_rows or out_cols < 1 or
 * > 32767 (VV_ERR_SHAPE); a pointer below its element's alignment (VV_ERR_ALIGN).  The host entries also refuse, with VV_ERR_SHAPE
 * and before anything is written by vv_augment_images_host: an image index outside n_images, h or w < 1, a crop outside the padded
 * image, a scale that is not positive and finite, a box whose crop is empty.  The device entries cannot read params without a round
 * trip: there a refused row's workgroups write nothing, and vv_augment_draw marks a refused sample's row (word 0 = -1) so that
 * vv_augment_images leaves its output untouched. */
int vv_augment_images(const unsigned char *images, const long long *image_meta, int n_images, const int *params, int batch,
                      int out_rows, int out_cols, float *out, void *hip_stream);
int vv_augment_images_host(const unsigned char *images, const long long *image_meta, int n_images, const int *params, int batch,
                           int out_rows, int out_cols, float *out);
int vv_augment_draw(const long long *image_meta, int n_images, const int *image_index, const float *boxes, int batch,
                    int augmentation, unsigned long long seed, unsigned long long offset, int *params, void *hip_stream);
int vv_augment_draw_host(const long long *image_meta, int n_images, const int *image_index, const float *boxes, int batch,
                         int augmentation, unsigned long long seed, unsigned long long offset, int *params);
int vv_augment_check_host(const long long *image_meta, int n_images, const int *params, int batch);

/* ---- All four colour operations of the reference's imgAug (datasetUtils.py:64-89 builds iaa.Sequential([GaussianBlur(sigma=(0, 3.0)),
 * Invert(0.05, per_channel=True), Add((-10, 10), per_channel=0.5), AddToHueAndSaturation((-20, 20))]), each gated by :98-103) on the
 * flipped crop, in that order: blur -> invert -> add -> hue/saturation.  csrc/augment.h 1a and 1b state both new stages: the blur is
 * scipy.ndimage.gaussian_filter(mode='mirror', truncate 4) in float64 with one rounding at the end and weights from the header's own
 * exponential; hue/saturation goes through OpenCV's 8-bit HSV (integer forward, float32 inverse) with channel 0 taken as R.  Not
 * modelled: scipy's summation order, cv2.GaussianBlur's fixed-point path, and the agreement of the HSV chain with cv2 is not measured.
 *   colour      int32 [batch][4]: 0 flags (bit 0 blur, bit 1 hue/saturation); 1 sigma as float32 bits, 0 <= sigma <= 16; 2 hue add
 *               in H units, -179 .. 179; 3 saturation add, -255 .. 255.  A row of zeros is vv_augment_images' result bit for bit.
 *   workspace   vv_augment_colour_workspace_bytes(max_rows, max_cols, batch) bytes (pure host arithmetic; 0 for arguments out of
 *               range): one slab of max_rows * max_cols 32-bit words per sample, sample b owns slab b.  Written before it is read;
 *               the result does not depend on workspace_bytes beyond that minimum.
 * vv_augment_draw_ex (replaces datasetUtils.py:98-103's choice of the four and imgaug's draws of sigma and value): vv_augment_draw's
 *   launch, which also fills `colour` from the same Philox blocks (slots 4, 6, 20, 21); the params rows are vv_augment_draw's bit for
 *   bit.  augmentation = 0 and a refused sample: a colour row of zeros.
 * vv_augment_images_ex (replaces datasetUtils.py:64-89 and :101-103 in front of :137-152): TWO launches on `hip_stream`.  The colour
 *   pre-pass, 32 x 32 tiles of a flagged sample's crop (as many workgroups per sample as a max_rows x max_cols crop has tiles, each
 *   sample's workgroups walking that sample's own tiles: h * w alone decides whether a crop fits), writes the finished source
 *   levels into the sample's slab; then vv_augment_images' kernel, reading a flagged sample's source from its slab.  colour == NULL is
 *   vv_augment_images.
 * The _host entries are the same code on host pointers (the workspace too), bit for bit the device's output.
 * Refused before any launch, besides what vv_augment_images / vv_augment_draw refuse: workspace or (draw) colour NULL (VV_ERR_NULL);
 *   max_rows or max_cols < 1 or > 32767 (VV_ERR_SHAPE); workspace_bytes below the minimum (VV_ERR_WORKSPACE).  A row is inadmissible
 *   when its params row is, when its colour row is (other flag bits, sigma NaN, negative or above 16, hue or saturation out of range),
 *   or when it has a flag set and h * w exceeds max_rows * max_cols: the host entry returns VV_ERR_SHAPE before anything is written;
 *   on the device such a row's workgroups write nothing in either launch. */
int vv_augment_draw_ex(const long long *image_meta, int n_images, const int *image_index, const float *boxes, int batch,
                       int augmentation, unsigned long long seed, unsigned long long offset, int *params, int *colour,
                       void *hip_stream);
int vv_augment_draw_ex_host(const long long *image_meta, int n_images, const int *image_index, const float *boxes, int batch,
                            int augmentation, unsigned long long seed, unsigned long long offset, int *params, int *colour);
size_t vv_augment_colour_workspace_bytes(int max_rows, int max_cols, int batch);
int vv_augment_images_ex(const unsigned char *images, const long long *image_meta, int n_images, const int *params, int batch,
                         int out_rows, int out_cols, float *out, const int *colour, void *workspace, size_t workspace_bytes,
                         int max_rows, int max_cols, void *hip_stream);
int vv_augment_images_ex_host(const unsigned char *images, const long long *image_meta, int n_images, const int *params, int batch,
                              int out_rows, int out_cols, float *out, const int *colour, void *workspace, size_t workspace_bytes,
                              int max_rows, int max_cols);

/* ---- Viewpoint clustering (csrc/kmeans_cosine.h states every expression, the tie rule and the summation order): the reference's
 * kmeans_cosine._kmeans, src/module/function.py:166-191.  All arithmetic is IEEE float64.
 *   x          float64 [n][6] = (sin a, sin e, sin i, cos a, cos e, cos i) per point
 *   centres    float64 [k][6], in-out: the initial centres on entry, the centres after the last update on return
 *   xtoc       int32 [n]: the nearest centre of every point, the LOWEST index among equals (np.argmin's rule)
 *   distance   float64 [n]: the distance to that centre.  Both are the last iteration's assignment, taken before its update
 *   iterations int32 [1]: the iterations that did work.  An iteration that changes no label makes every later one a repetition, bit
 *              for bit; those are not run (host) or return at their first instruction (device), and the result is that of max_iter
 *              full iterations
 *   workspace  vv_kmeans_cosine_workspace_bytes(n, k) bytes (pure host arithmetic; 0 for arguments out of range), 8-byte aligned.
 *              Written before it is read; the result does not depend on its contents or on workspace_bytes beyond that minimum.
 * vv_kmeans_cosine: every pointer a device pointer; 2 * max_iter launches on `hip_stream`, enqueued by this one call with no read-back
 *   in between (per iteration: a workgroup per 256 points with the centres in LDS, then the chunk-order reduction).  No atomics: the
 *   same bits on every run, and the bits of the host entry.
 * vv_kmeans_cosine_host: the same code on host pointers, no stream, no workspace; needs no GPU.
 * vv_kmeans_cosine_assign / _assign_host: xtoc (and distance, unless NULL) of points against given centres; one launch.
 * Refused before any launch: a NULL required pointer (VV_ERR_NULL); n < 1, n > 1048576, k < 1, k > 1024, max_iter < 1 or
 *   max_iter > 65536 (VV_ERR_SHAPE); a pointer below its element's alignment (VV_ERR_ALIGN); a short workspace (VV_ERR_WORKSPACE). */
size_t vv_kmeans_cosine_workspace_bytes(int n, int k);
int vv_kmeans_cosine(const double *x, int n, double *centres, int k, int max_iter, int *xtoc, double *distance, int *iterations,
                     void *workspace, size_t workspace_bytes, void *hip_stream);
int vv_kmeans_cosine_host(const double *x, int n, double *centres, int k, int max_iter, int *xtoc, double *distance, int *iterations);
int vv_kmeans_cosine_assign(const double *x, int n, const double *centres, int k, int *xtoc, double *distance, void *hip_stream);
int vv_kmeans_cosine_assign_host(const double *x, int n, const double *centres, int k, int *xtoc, double *distance);

#ifdef __cplusplus
}
#endif
#endif
